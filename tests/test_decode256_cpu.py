"""KV-cache decode at d_head = 256 without a device: the four exports, the split rule and the workspace through the
C ABI against the rule as written, the refusals with their statuses and order, batch = 0, the d128 and d64 entries' words, and one
signature in the three modules with the wrapper's errors before the library loads."""
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
from tests.test_decode_cpu import _args
from tests.test_sinks_cpu import _ref
from tests.test_softcap_cpu import _cap, _w

SYMBOLS = tuple(f"fa_decode_d256_{what}" for what in ("supported", "num_splits", "workspace_bytes", "launch"))


def _call(what, args, window, cap, *more):
    return getattr(_capi.load(), f"fa_decode_d256_{what}")(_ref(args), _ref(window), _ref(cap), *more), _capi.last_error()


def test_the_four_symbols_are_exported_and_declared():
    header = open(os.path.join(ROOT, "include", "fa_hip.h")).read()
    assert set(SYMBOLS) <= set(_capi.EXPORTED_SYMBOLS) and all(f" {name}(" in header for name in SYMBOLS)
    libs = [ctypes.CDLL(os.path.join(ROOT, "flash_attention_from_scratch_amd", "lib", so)) for so in ("libfa_hip.so", "libfa_hip_jitter.so")]
    assert all(hasattr(lib, name) for lib in libs for name in SYMBOLS) and _capi.load().fa_abi_version() == 6


@pytest.mark.parametrize("batch,Hkv,max_k,window", [(1, 2, 0, (-1, -1)), (8, 8, 32768, (-1, -1)), (64, 8, 32768, (-1, -1)), (8, 8, 32768, (4095, 0)),
                                                    (2, 1, 300, (-1, -1)), (1, 1, 32768, (2000, -1)), (3, 2, 32768, (1000, 30))])
def test_the_split_count_and_the_workspace_are_the_rules(batch, Hkv, max_k, window):
    """256 workgroups wanted (powers of two), at least 256 keys of the bound per split, at most 128 splits; the bound is the window's
    span left + seqlen_q + right when both sides are bounded and that is less; the cap does not enter; the partials are 256 wide"""
    Sq, H, cache = 2, 8, 32768
    bound = max_k or cache
    if window[0] >= 0 and window[1] >= 0:
        bound = min(bound, window[0] + Sq + window[1])
    s = 1
    while batch * Hkv * s < 256 and s < 128:
        s *= 2
    want = max(1, min(s, -(-bound // 256)))
    po = 4 * want * batch * Hkv * (Sq * (H // Hkv)) * 256
    args = _args(batch=batch, Sq=Sq, H=H, Hkv=Hkv, cache=cache, d_head=256, max_seqlen_k=max_k)
    for cap in (None, _cap(50.0)):
        assert _call("supported", args, _w(*window), cap)[0] == 1
        assert _call("num_splits", args, _w(*window), cap)[0] == want
        assert _call("workspace_bytes", args, _w(*window), cap)[0] == (0 if want == 1 else po + ((po // 256 + 15) & ~15))
    args.num_splits = 7
    assert _call("num_splits", args, _w(*window), None)[0] == 7


REFUSALS = [(dict(d_head=128), _w(), None, -4, "d_head = 256 only"), (dict(d_head=128, Sq=9, H=8, Hkv=1), _w(), None, -4, "d_head = 256 only"),
            (dict(d_head=256, Sq=17, H=4, Hkv=2), _w(), None, -3, "32 packed query rows"),
            (dict(d_head=256, Sq=17, H=4, Hkv=2, paged=(8, 32, 4)), _w(), None, -3, "32 packed query rows"),
            (dict(d_head=256, paged=(8, 32, 4)), None, None, -3, "multiple of 64"), (dict(d_head=256, dtype=7), _w(), None, -2, "Only fp16 and bf16"),
            (dict(d_head=256), None, _cap(-1.0), -1, "fa_window is null"), (dict(d_head=256, causal=1), _w(5, 3), _cap(-1.0), -4, "causal means right = 0"),
            (dict(d_head=256), _w(), _cap(-1.0), -4, "softcap (-1) must be finite and > 0"), (dict(d_head=256), _w(), _cap(struct_size=4), -4, "fa_softcap.struct_size"),
            (dict(d_head=256, batch=1, Hkv=1, workspace=None), _w(), None, -1, "fa_decode_d256_workspace_bytes(args, window, softcap)")]


@pytest.mark.parametrize("over,window,cap,status,text", REFUSALS, ids=[f"{i}: {r[4]}" for i, r in enumerate(REFUSALS)])
def test_the_refusals_their_statuses_and_their_order(over, window, cap, status, text):
    """d_head first, then the rows and the page size, then the window's rules, then a non-null cap's: an input that breaks two
    reports the first"""
    rc, msg = _call("launch", _args(**over), window, cap, None, None)
    assert rc == status and text in msg, (rc, msg)
    if "workspace" not in text:   # (the queries refuse what the launch refuses of the shapes)
        assert _call("supported", _args(**over), window, cap)[0] == 0 and _call("num_splits", _args(**over), window, cap)[0] == status
        assert _call("workspace_bytes", _args(**over), window, cap)[0] == status


def test_batch_zero_is_ok_and_the_d128_and_d64_entries_keep_their_words():
    ms = ctypes.c_float(-1.0)
    assert _call("launch", _args(batch=0, d_head=256), _w(), _cap(50.0), None, ctypes.byref(ms))[0] == 0 and ms.value == 0.0
    lib = _capi.load()
    assert lib.fa_decode_launch(_ref(_args(d_head=256)), None, None) == -4 and "decode supports d_head = 128 only (got 256)" in _capi.last_error()
    assert lib.fa_decode_d64_launch(_ref(_args(d_head=256)), _ref(_w()), None, None, None) == -4
    assert "fa_decode_d64 serves d_head = 64 only (got 256" in _capi.last_error()
    assert lib.fa_decode_softcap_launch(_ref(_args(Sq=9, H=8, Hkv=1)), _ref(_w()), _ref(_cap()), None, None) == -3
    assert "<= 64 packed query rows" in _capi.last_error()


@pytest.mark.parametrize("name", ["forward_kvcache_d256", "kvcache_d256_num_splits"])
def test_one_signature_in_the_three_modules_and_bad_values_before_the_library_loads(name, monkeypatch):
    assert len({str(inspect.signature(getattr(mod, name))) for mod in (flash_attention, inner, fak)}) == 1
    monkeypatch.setattr(_capi, "load", lambda: (_ for _ in ()).throw(AssertionError("the library was asked")))
    q = torch.zeros((2, 1, 8, 256), dtype=torch.bfloat16)
    for mod in (flash_attention, fak):
        for bad in (-1.0, float("nan"), True, torch.zeros(())):
            with pytest.raises(ValueError, match="softcap"):
                getattr(mod, name)(q, q, q, q, bad)
            with pytest.raises(ValueError, match="causal means right = 0"):   # a bad window first
                getattr(mod, name)(q, q, q, q, softcap=bad, causal=True, window_size=(5, 3))
