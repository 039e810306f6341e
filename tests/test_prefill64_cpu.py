"""Prefill at d_head = 64 without a device: the four exports, the C-level refusals with their statuses and order,
every one before any HIP call, total_q = 0, and the wrapper's errors before the library loads."""
import ctypes
import os

import pytest
import torch

import flash_attention
from flash_attention_from_scratch_amd import _capi
from flash_attention_from_scratch_amd import flash_attention_kernels as fak
from tests.conftest import ROOT
from tests.test_prefill_kvcache_cpu import _contig, _paged
from tests.test_sinks_cpu import _ref, _sk, _w
from tests.test_varlen_qk_cpu import _fwd, _kv, _vl

SYMBOLS = ("fa_fwd_varlen_qk_d64_supported", "fa_fwd_launch_varlen_qk_d64", "fa_fwd_varlen_kvcache_d64_supported", "fa_fwd_launch_varlen_kvcache_d64")


def _launch(side, args=None, kv=None, vq=None, key=None, window=_w(), sinks=None, opts=None, lse=16):
    """one launch of the packed ("qk") or the cache ("kvcache") entry on host-only arguments -> (status, message)"""
    args = args or _fwd(d_head=64, seq_stride=8 * 64, head_stride=64)
    kv = kv or _kv(kv_batch_stride=4096 * 2 * 64, kv_seq_stride=2 * 64, kv_head_stride=64)
    key = key or (_vl(T=5000, max_seqlen=4096) if side == "qk" else _contig())
    rc = getattr(_capi.load(), f"fa_fwd_launch_varlen_{side}_d64")(ctypes.byref(args), ctypes.byref(kv), ctypes.byref(vq or _vl()), ctypes.byref(key),
                                                                    _ref(window), _ref(sinks), _ref(opts), ctypes.c_void_p(lse) if lse else None, None)
    return rc, _capi.last_error()


def test_the_four_symbols_are_exported_and_declared():
    header = open(os.path.join(ROOT, "include", "fa_hip.h")).read()
    assert set(SYMBOLS) <= set(_capi.EXPORTED_SYMBOLS) and all(f" {name}(" in header for name in SYMBOLS)
    libs = [ctypes.CDLL(os.path.join(ROOT, "flash_attention_from_scratch_amd", "lib", so)) for so in ("libfa_hip.so", "libfa_hip_jitter.so")]
    assert all(hasattr(lib, name) for lib in libs for name in SYMBOLS) and _capi.load().fa_abi_version() == 6
    cfg = _capi.make_config(fak.varlen_config(torch.bfloat16))
    for name in SYMBOLS[::2]:
        fn = getattr(_capi.load(), name)
        assert fn(ctypes.byref(cfg), None) == 1 and fn(None, None) == 0
        assert [fn(ctypes.byref(cfg), ctypes.byref(_capi.make_opts(**o))) for o in (dict(causal=True), dict(speculative=True), dict(prescaled_q=True),
                                                                                    dict(stats_ptr=16))] == [1, 0, 0, 0]
    for name in ("forward_varlen_d64", "forward_varlen_kvcache_d64"):
        assert getattr(flash_attention, name).__module__.endswith("flash_attention") and hasattr(fak, name)


# in the siblings' order: opts, d_head, the layouts, the cache, then the window's rules, and a non-null fa_sinks last
REFUSALS = [(dict(opts=_capi.make_opts(speculative=True), args=_fwd(d_head=128)), -3, "without speculative"),
            (dict(args=_fwd(d_head=128), window=None), -4, "d_head = 64 only"),
            (dict(vq=_vl(n_seqs=0), window=None), -4, "n_seqs must be at least 1"),
            (dict(window=None, sinks=_sk(n_heads=2)), -1, "fa_window is null"),
            (dict(window=_w(5, 3), opts=_capi.make_opts(causal=True), sinks=_sk(ptr=None)), -4, "causal means right = 0"),
            (dict(sinks=_sk(ptr=None)), -1, "fa_sinks.sinks is null"),
            (dict(sinks=_sk(n_heads=2)), -4, "fa_sinks.n_heads")]


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
        for sinks in (None, _sk()):
            assert _launch(side, vq=_vl(T=0), sinks=sinks, opts=_capi.make_opts(ms=ms))[0] == 0 and ms.value == 0.0
    # the d128 siblings keep their words
    rc = _capi.load().fa_fwd_launch_varlen_qk_sinks(ctypes.byref(_fwd(d_head=64)), ctypes.byref(_kv()), ctypes.byref(_vl()), ctypes.byref(_vl()),
                                                    ctypes.byref(_w()), ctypes.byref(_sk()), None, ctypes.c_void_p(16), None)
    assert rc == -4 and "Tensor d_head (64) does not match kernel configuration d_head (128)" in _capi.last_error()


def test_a_bad_window_is_a_value_error_and_bad_sinks_a_runtime_error_before_the_library_loads(monkeypatch):
    monkeypatch.setattr(_capi, "load", lambda: (_ for _ in ()).throw(AssertionError("the library was asked")))
    q, cu = torch.zeros((8, 8, 64), dtype=torch.bfloat16), torch.tensor([0, 8], dtype=torch.int32)
    for mod in (flash_attention, fak):
        for call in (lambda **kw: mod.forward_varlen_d64(q, q, q, cu, 8, **kw), lambda **kw: mod.forward_varlen_kvcache_d64(q, q, q, cu, 8, cu, **kw)):
            for bad in (1.0, torch.zeros(8, dtype=torch.float64), torch.zeros(7), torch.zeros(16)[::2]):
                with pytest.raises(RuntimeError, match="sinks"):
                    call(sinks=bad)
                with pytest.raises(ValueError, match="causal means right = 0"):   # a bad window first
                    call(sinks=bad, causal=True, window_size=(5, 3))
            with pytest.raises(ValueError, match="window_size"):
                call(window_size=(-2, 0))
            with pytest.raises(RuntimeError, match="must be a CUDA tensor"):   # (good arguments get as far as the device check)
                call(sinks=torch.zeros(8))
