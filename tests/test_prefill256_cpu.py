"""Prefill at d_head = 256 without a device: the four exports, the C-level refusals with their statuses and order,
every one before any HIP call, total_q = 0, the siblings' words for a 256-wide tensor, one signature in the three modules and the
wrapper's errors before the library loads."""
import ctypes
import inspect
import os

import pytest
import torch

import flash_attention
from flash_attention_from_scratch_amd import _capi
from flash_attention_from_scratch_amd import flash_attention as inner
from flash_attention_from_scratch_amd import flash_attention_kernels as fak
from tests.conftest import ROOT
from tests.test_prefill_kvcache_cpu import _contig, _paged
from tests.test_sinks_cpu import _ref, _sk
from tests.test_softcap_cpu import _cap, _w
from tests.test_varlen_qk_cpu import _fwd, _kv, _vl

SYMBOLS = ("fa_fwd_varlen_qk_d256_supported", "fa_fwd_launch_varlen_qk_d256", "fa_fwd_varlen_kvcache_d256_supported",
           "fa_fwd_launch_varlen_kvcache_d256")
NAMES = ("forward_varlen_d256", "forward_varlen_kvcache_d256")


def _launch(side, args=None, kv=None, vq=None, key=None, window=_w(), cap=None, opts=None, lse=16):
    """one launch of the packed ("qk") or the cache ("kvcache") entry on host-only arguments -> (status, message)"""
    args = args or _fwd(d_head=256, seq_stride=8 * 256, head_stride=256)
    kv = kv or _kv(kv_batch_stride=4096 * 2 * 256, kv_seq_stride=2 * 256, kv_head_stride=256)
    key = key or (_vl(T=5000, max_seqlen=4096) if side == "qk" else _contig())
    rc = getattr(_capi.load(), f"fa_fwd_launch_varlen_{side}_d256")(ctypes.byref(args), ctypes.byref(kv), ctypes.byref(vq or _vl()), ctypes.byref(key),
                                                                     _ref(window), _ref(cap), _ref(opts), ctypes.c_void_p(lse) if lse else None, None)
    return rc, _capi.last_error()


def test_the_four_symbols_are_exported_and_declared_and_the_calls_have_one_signature():
    header = open(os.path.join(ROOT, "include", "fa_hip.h")).read()
    assert set(SYMBOLS) <= set(_capi.EXPORTED_SYMBOLS) and all(f" {name}(" in header for name in SYMBOLS)
    libs = [ctypes.CDLL(os.path.join(ROOT, "flash_attention_from_scratch_amd", "lib", so)) for so in ("libfa_hip.so", "libfa_hip_jitter.so")]
    assert all(hasattr(lib, name) for lib in libs for name in SYMBOLS) and _capi.load().fa_abi_version() == 6
    assert libs[0].fa_num_kernels() == libs[1].fa_num_kernels()
    cfg = _capi.make_config(fak.varlen_config(torch.bfloat16))
    for name in SYMBOLS[::2]:
        fn = getattr(_capi.load(), name)
        assert fn(ctypes.byref(cfg), None) == 1 and fn(None, None) == 0
        assert [fn(ctypes.byref(cfg), ctypes.byref(_capi.make_opts(**o))) for o in (dict(causal=True), dict(speculative=True), dict(prescaled_q=True),
                                                                                    dict(stats_ptr=16))] == [1, 0, 0, 0]
    for name in NAMES:
        assert getattr(flash_attention, name) is getattr(inner, name)
        assert inspect.signature(getattr(inner, name)) == inspect.signature(getattr(fak, name))
    assert str(inspect.signature(fak.forward_varlen_d256)) == ("(q, k, v, cu_seqlens, max_seqlen, softcap=0.0, causal=False, timed=False, "
                                                               "cu_seqlens_k=None, max_seqlen_k=None, *, window_size=(-1, -1))")
    assert str(inspect.signature(fak.forward_varlen_kvcache_d256)) == (
        "(q, k_cache, v_cache, cu_seqlens_q, max_seqlen_q, cache_seqlens, softcap=0.0, block_table=None, causal=False, max_seqlen_k=None, "
        "timed=False, *, window_size=(-1, -1))")


# in the siblings' order: opts, d_head, the layouts, the cache, then the window's rules, and a non-null fa_softcap last
REFUSALS = [(dict(opts=_capi.make_opts(speculative=True), args=_fwd(d_head=128)), -3, "without speculative"),
            (dict(args=_fwd(d_head=128), window=None), -4, "d256 supports d_head = 256 only (got 128)"),
            (dict(vq=_vl(n_seqs=0), window=None), -4, "n_seqs must be at least 1"),
            (dict(window=None, cap=_cap(-1.0)), -1, "fa_window is null"),
            (dict(window=_w(5, 3), opts=_capi.make_opts(causal=True), cap=_cap(-1.0)), -4, "causal means right = 0"),
            (dict(cap=_cap(struct_size=4)), -4, "fa_softcap.struct_size"),
            (dict(cap=_cap(-1.0)), -4, "must be finite and > 0"),
            (dict(cap=_cap(float("inf"))), -4, "must be finite and > 0")]


@pytest.mark.parametrize("side", ["qk", "kvcache"])
@pytest.mark.parametrize("over,status,text", REFUSALS, ids=[r[2] for r in REFUSALS])
def test_the_refusals_their_statuses_and_their_order(side, over, status, text):
    rc, msg = _launch(side, **over)
    assert rc == status and text in msg, (rc, msg)


def test_the_cache_rules_come_before_the_window_and_total_q_zero_is_ok():
    rc, msg = _launch("kvcache", key=_paged(page_size=32), window=None)
    assert rc == -3 and "multiple of 64" in msg, (rc, msg)
    rc, msg = _launch("kvcache", key=_contig(batch=2), window=None)
    assert rc == -4 and "one batch entry per sequence" in msg, (rc, msg)
    ms = ctypes.c_float(-1.0)
    for side in ("qk", "kvcache"):
        for cap in (None, _cap()):
            assert _launch(side, vq=_vl(T=0), cap=cap, opts=_capi.make_opts(ms=ms))[0] == 0 and ms.value == 0.0
    # the d128 and the d64 siblings keep their words for a 256-wide tensor
    tail = (ctypes.byref(_kv()), ctypes.byref(_vl()), ctypes.byref(_vl()), ctypes.byref(_w()))
    rc = _capi.load().fa_fwd_launch_varlen_qk_softcap(ctypes.byref(_fwd(d_head=256)), *tail, ctypes.byref(_cap()), None, ctypes.c_void_p(16), None)
    assert rc == -4 and "Tensor d_head (256) does not match kernel configuration d_head (128)" in _capi.last_error()
    rc = _capi.load().fa_fwd_launch_varlen_qk_d64(ctypes.byref(_fwd(d_head=256)), *tail, ctypes.byref(_sk()), None, ctypes.c_void_p(16), None)
    assert rc == -4 and "fa_fwd_launch_varlen_qk_d64 supports d_head = 64 only (got 256)" in _capi.last_error()


def test_a_bad_window_then_a_bad_softcap_are_value_errors_before_the_library_loads(monkeypatch):
    monkeypatch.setattr(_capi, "load", lambda: (_ for _ in ()).throw(AssertionError("the library was asked")))
    q, cu = torch.zeros((8, 8, 256), dtype=torch.bfloat16), torch.tensor([0, 8], dtype=torch.int32)
    for mod in (flash_attention, fak):
        for call in (lambda **kw: mod.forward_varlen_d256(q, q, q, cu, 8, **kw), lambda **kw: mod.forward_varlen_kvcache_d256(q, q, q, cu, 8, cu, **kw)):
            for bad in (-1.0, float("inf"), float("nan"), True, torch.zeros(())):
                with pytest.raises(ValueError, match="softcap"):
                    call(softcap=bad)
                with pytest.raises(ValueError, match="causal means right = 0"):   # a bad window first
                    call(softcap=bad, causal=True, window_size=(5, 3))
            with pytest.raises(ValueError, match="window_size"):
                call(window_size=(-2, 0))
            with pytest.raises(RuntimeError, match="must be a CUDA tensor"):   # (good arguments get as far as the device check)
                call(softcap=4.0)
