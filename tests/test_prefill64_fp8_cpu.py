"""Prefill against an fp8 cache at d_head = 64 without a device: the two exports, `supported`, the C refusals with
their statuses and order -- the 16-bit d64 entry's first, then the fp8 side's -- every one before any HIP call, total_q = 0, the
wrapper's errors before the library loads, and one signature in the three modules."""
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
from tests.test_prefill_kvcache_fp8_cpu import _sc
from tests.test_sinks_cpu import _ref, _sk, _w
from tests.test_varlen_qk_cpu import _fwd, _kv, _vl

SYMBOLS = ("fa_fwd_varlen_kvcache_fp8_d64_supported", "fa_fwd_launch_varlen_kvcache_fp8_d64")


def _launch(args=None, kv=None, vq=None, key=None, scales=None, window=_w(), sinks=None, opts=None, lse=16):
    """one launch on host-only arguments (the cache's strides count bytes) -> (status, message)"""
    args = args or _fwd(d_head=64, seq_stride=8 * 64, head_stride=64)
    kv = kv or _kv(kv_batch_stride=4096 * 2 * 64, kv_seq_stride=2 * 64, kv_head_stride=64)
    rc = _capi.load().fa_fwd_launch_varlen_kvcache_fp8_d64(ctypes.byref(args), ctypes.byref(kv), ctypes.byref(vq or _vl()), ctypes.byref(key or _contig()),
                                                           _ref(scales or _sc()), _ref(window), _ref(sinks), _ref(opts), ctypes.c_void_p(lse) if lse else None, None)
    return rc, _capi.last_error()


def test_the_two_symbols_are_exported_and_declared_and_supported_is_the_16_bit_entrys():
    header = open(os.path.join(ROOT, "include", "fa_hip.h")).read()
    assert set(SYMBOLS) <= set(_capi.EXPORTED_SYMBOLS) and all(f" {name}(" in header for name in SYMBOLS)
    libs = [ctypes.CDLL(os.path.join(ROOT, "flash_attention_from_scratch_amd", "lib", so)) for so in ("libfa_hip.so", "libfa_hip_jitter.so")]
    assert all(hasattr(lib, name) for lib in libs for name in SYMBOLS) and _capi.load().fa_abi_version() == 6
    fn, want = _capi.load().fa_fwd_varlen_kvcache_fp8_d64_supported, _capi.load().fa_fwd_varlen_kvcache_d64_supported
    cfg = _capi.make_config(fak.varlen_config(torch.bfloat16))
    assert fn(None, None) == want(None, None) == 0 and fn(ctypes.byref(cfg), None) == want(ctypes.byref(cfg), None) == 1
    for o in (dict(causal=True), dict(speculative=True), dict(prescaled_q=True), dict(stats_ptr=16)):
        assert fn(ctypes.byref(cfg), ctypes.byref(_capi.make_opts(**o))) == want(ctypes.byref(cfg), ctypes.byref(_capi.make_opts(**o)))


# what fa_fwd_launch_varlen_kvcache_d64 refuses comes first, in its order and words, whatever the fp8 side holds ...
BAD8 = _sc(kv_dtype=0, descale_batch_stride=1)
REFUSALS = [(dict(opts=_capi.make_opts(speculative=True), args=_fwd(d_head=128), scales=BAD8), -3, "without speculative"),
            (dict(args=_fwd(d_head=128), window=None, scales=BAD8), -4, "d_head = 64 only"),
            (dict(vq=_vl(n_seqs=0), window=None, scales=BAD8), -4, "n_seqs must be at least 1"),
            (dict(key=_paged(page_size=32), window=None, scales=BAD8), -3, "multiple of 64"),
            (dict(key=_contig(batch=2), window=None, scales=BAD8), -4, "one batch entry per sequence"),
            (dict(window=None, sinks=_sk(n_heads=2), scales=BAD8), -1, "fa_window is null"),
            (dict(window=_w(5, 3), opts=_capi.make_opts(causal=True), sinks=_sk(ptr=None), scales=BAD8), -4, "causal means right = 0"),
            (dict(sinks=_sk(ptr=None), scales=BAD8), -1, "fa_sinks.sinks is null"),
            (dict(sinks=_sk(n_heads=2), scales=BAD8), -4, "fa_sinks.n_heads"),
            # ... then the fp8 side, in fa_fwd_launch_varlen_kvcache_fp8's words and in this order
            (dict(sinks=_sk(), scales=BAD8), -2, "kv_dtype"),
            (dict(scales=_sc(descale_batch_stride=1), kv=_kv(kv_batch_stride=4096 * 2 * 64, kv_seq_stride=2 * 64 + 8, kv_head_stride=64)), -4, "descale_batch_stride"),
            (dict(scales=_sc(v_descale=18), kv=_kv(kv_batch_stride=4096 * 2 * 64, kv_seq_stride=2 * 64 + 8, kv_head_stride=64)), -5, "multiples of 16 bytes"),
            (dict(scales=_sc(v_descale=18)), -5, "k_descale and v_descale must be 4-byte aligned")]


@pytest.mark.parametrize("over,status,text", REFUSALS, ids=[r[2] for r in REFUSALS])
def test_the_refusals_their_statuses_and_their_order(over, status, text):
    rc, msg = _launch(**over)
    assert rc == status and text in msg, (rc, msg)


def test_total_q_zero_is_ok():
    ms = ctypes.c_float(-1.0)
    for sinks in (None, _sk()):
        assert _launch(vq=_vl(T=0), sinks=sinks, opts=_capi.make_opts(ms=ms))[0] == 0 and ms.value == 0.0


def test_the_wrappers_errors_come_before_the_library_loads(monkeypatch):
    monkeypatch.setattr(_capi, "load", lambda: (_ for _ in ()).throw(AssertionError("the library was asked")))
    q, cu, ones = torch.zeros((8, 8, 64), dtype=torch.bfloat16), torch.tensor([0, 8], dtype=torch.int32), torch.ones((1, 2))
    k16 = torch.zeros((1, 128, 2, 64), dtype=torch.bfloat16)
    k8 = k16.to(torch.float8_e4m3fn)
    for mod in (flash_attention, fak):
        fn = lambda k, v, **kw: mod.forward_varlen_kvcache_d64(q, k, v, cu, 8, cu[1:], **kw)   # noqa: E731
        for given in ({}, dict(k_descale=ones), dict(v_descale=ones)):
            with pytest.raises(RuntimeError, match="(?s)fp8.*pass ones"):
                fn(k8, k8, **given)
            with pytest.raises(ValueError, match="window_size"):   # a bad window first
                fn(k8, k8, window_size=(-2, 0), **given)
        with pytest.raises(RuntimeError, match="belong to an fp8"):
            fn(k16, k16, k_descale=ones, v_descale=ones)
        with pytest.raises(RuntimeError, match="must be torch.float8_e4m3fn"):
            fn(k16.to(torch.float8_e5m2), k16.to(torch.float8_e5m2), k_descale=ones, v_descale=ones)
        with pytest.raises(RuntimeError, match="one data type"):
            fn(k8, k16, k_descale=ones, v_descale=ones)
        with pytest.raises(RuntimeError, match="k_descale must be an fp32"):
            fn(k8, k8, k_descale=torch.ones((1, 3)), v_descale=ones)
        with pytest.raises(RuntimeError, match="must be a CUDA tensor"):   # (good arguments get as far as the device check)
            fn(k8, k8, k_descale=ones, v_descale=ones)


def test_one_signature_in_the_three_modules():
    sigs = [inspect.signature(getattr(mod, "forward_varlen_kvcache_d64")) for mod in (flash_attention, inner, fak)]
    last = list(sigs[0].parameters.values())[-3:]
    assert sigs[0] == sigs[1] == sigs[2] and [(p.name, p.default, p.kind) for p in last] == [
        ("window_size", (-1, -1), inspect.Parameter.KEYWORD_ONLY), ("k_descale", None, inspect.Parameter.KEYWORD_ONLY),
        ("v_descale", None, inspect.Parameter.KEYWORD_ONLY)]
