"""KV-cache decode at d_head = 64 without a device: the four exports, the split rule and the workspace through the
C ABI against the rule as written, the refusals and their statuses, batch = 0, and the wrapper's errors before the library loads."""
import ctypes
import os

import pytest
import torch

import flash_attention
from flash_attention_from_scratch_amd import _capi
from flash_attention_from_scratch_amd import flash_attention_kernels as fak
from tests.conftest import ROOT
from tests.test_decode_cpu import _args
from tests.test_sinks_cpu import _ref, _sk, _w

SYMBOLS = tuple(f"fa_decode_d64_{what}" for what in ("supported", "num_splits", "workspace_bytes", "launch"))


def _call(what, args, window, sinks, *more):
    return getattr(_capi.load(), f"fa_decode_d64_{what}")(_ref(args), _ref(window), _ref(sinks), *more), _capi.last_error()


def test_the_four_symbols_are_exported_and_declared():
    header = open(os.path.join(ROOT, "include", "fa_hip.h")).read()
    assert set(SYMBOLS) <= set(_capi.EXPORTED_SYMBOLS) and all(f" {name}(" in header for name in SYMBOLS)
    libs = [ctypes.CDLL(os.path.join(ROOT, "flash_attention_from_scratch_amd", "lib", so)) for so in ("libfa_hip.so", "libfa_hip_jitter.so")]
    assert all(hasattr(lib, name) for lib in libs for name in SYMBOLS) and _capi.load().fa_abi_version() == 6


@pytest.mark.parametrize("batch,Hkv,max_k,window", [(1, 2, 0, (-1, -1)), (8, 8, 65536, (-1, -1)), (64, 8, 65536, (-1, -1)), (8, 8, 65536, (127, 0)),
                                                    (2, 1, 300, (-1, -1)), (1, 1, 65536, (2000, -1)), (3, 2, 65536, (1000, 30))])
def test_the_split_count_and_the_workspace_are_the_rules(batch, Hkv, max_k, window):
    """256 workgroups wanted (powers of two), at least 256 keys of the bound per split, at most 128 splits; the bound is the window's
    span left + seqlen_q + right when both sides are bounded and that is less; the partials are 64 wide"""
    Sq, H, cache = 2, 8, 65536
    bound = max_k or cache
    if window[0] >= 0 and window[1] >= 0:
        bound = min(bound, window[0] + Sq + window[1])
    s = 1
    while batch * Hkv * s < 256 and s < 128:
        s *= 2
    want = max(1, min(s, -(-bound // 256)))
    po = 4 * want * batch * Hkv * (Sq * (H // Hkv)) * 64
    args = _args(batch=batch, Sq=Sq, H=H, Hkv=Hkv, cache=cache, d_head=64, max_seqlen_k=max_k)
    for sinks in (None, _sk()):
        assert _call("supported", args, _w(*window), sinks)[0] == 1
        assert _call("num_splits", args, _w(*window), sinks)[0] == want
        assert _call("workspace_bytes", args, _w(*window), sinks)[0] == (0 if want == 1 else po + ((po // 64 + 15) & ~15))
    args.num_splits = 7
    assert _call("num_splits", args, _w(*window), None)[0] == 7


REFUSALS = [(dict(d_head=128), _w(), None, -4, "d_head = 64 only"), (dict(d_head=64, Sq=9, H=8, Hkv=1), _w(), None, -3, "64 packed query rows"),
            (dict(d_head=64, paged=(8, 32, 4)), _w(), None, -3, "multiple of 64"), (dict(d_head=64, dtype=7), _w(), None, -2, "Only fp16 and bf16"),
            (dict(d_head=64), None, None, -1, "fa_window is null"), (dict(d_head=64, causal=1), _w(5, 3), None, -4, "causal means right = 0"),
            (dict(d_head=64), _w(), _sk(ptr=None), -1, "fa_sinks.sinks is null"), (dict(d_head=64), _w(), _sk(n_heads=2), -4, "fa_sinks.n_heads"),
            (dict(d_head=64, batch=1, Hkv=1, workspace=None), _w(), None, -1, "fa_decode_d64_workspace_bytes")]


@pytest.mark.parametrize("over,window,sinks,status,text", REFUSALS, ids=[r[4] for r in REFUSALS])
def test_the_refusals_and_their_statuses(over, window, sinks, status, text):
    rc, msg = _call("launch", _args(**over), window, sinks, None, None)
    assert rc == status and text in msg, (rc, msg)
    if "workspace" not in text:   # (the queries refuse what the launch refuses of the shapes)
        assert _call("supported", _args(**over), window, sinks)[0] == 0 and _call("num_splits", _args(**over), window, sinks)[0] == status
        assert _call("workspace_bytes", _args(**over), window, sinks)[0] == status


def test_batch_zero_is_ok_and_the_d128_entry_keeps_its_words():
    ms = ctypes.c_float(-1.0)
    assert _call("launch", _args(batch=0, d_head=64), _w(), _sk(), None, ctypes.byref(ms))[0] == 0 and ms.value == 0.0
    assert _capi.load().fa_decode_launch(_ref(_args(d_head=64)), None, None) == -4
    assert "decode supports d_head = 128 only (got 64)" in _capi.last_error()


def test_a_bad_window_is_a_value_error_and_bad_sinks_a_runtime_error_before_the_library_loads(monkeypatch):
    monkeypatch.setattr(_capi, "load", lambda: (_ for _ in ()).throw(AssertionError("the library was asked")))
    q = torch.zeros((2, 1, 8, 64), dtype=torch.bfloat16)
    for mod in (flash_attention, fak):
        for fn in (mod.forward_kvcache_d64, mod.kvcache_d64_num_splits):
            for bad in (1.0, torch.zeros(8, dtype=torch.float64), torch.zeros(7), torch.zeros(16)[::2]):
                with pytest.raises(RuntimeError, match="sinks"):
                    fn(q, q, q, q, sinks=bad)
                with pytest.raises(ValueError, match="causal means right = 0"):   # a bad window first
                    fn(q, q, q, q, sinks=bad, causal=True, window_size=(5, 3))
            with pytest.raises(ValueError, match="window_size"):
                fn(q, q, q, q, window_size=(-2, 0))
