"""Attention sinks in KV-cache decode and cache prefill without a device: the two signatures in the three modules,
the validator's order, the ten exports, the C refusals in their order with the windowed sibling's words, the decode's split count."""
import ctypes
import inspect
import itertools
import os

import pytest
import torch

import flash_attention
from flash_attention_from_scratch_amd import _capi
from flash_attention_from_scratch_amd import flash_attention_kernels as fak
from tests.conftest import ROOT
from tests.test_decode_cpu import _args
from tests.test_decode_fp8_cpu import _args as _args8
from tests.test_prefill_kvcache_cpu import _contig, _fwd, _kv, _vl
from tests.test_prefill_window_cpu import _scales
from tests.test_sinks_cpu import _bad_sinks, _ref, _sk, _w

PREFILL, DECODE = ("varlen_kvcache", "varlen_kvcache_fp8"), (("fa_decode", _args), ("fa_decode_fp8", _args8))
NEW_SYMBOLS = tuple(f"fa_fwd_{what}{form}_sinks{tail}" for form in PREFILL for what, tail in (("", "_supported"), ("launch_", "")))
NEW_SYMBOLS += tuple(f"{form}_sinks_{what}" for form, _ in DECODE for what in ("supported", "num_splits", "launch"))


def test_the_two_signatures_in_the_three_modules():
    import flash_attention_from_scratch_amd.flash_attention as inner
    for mod in (flash_attention, inner, fak):
        for plain, sunk, behind in ((mod.forward_kvcache, mod.forward_kvcache_sinks, 4), (mod.forward_varlen_kvcache, mod.forward_varlen_kvcache_sinks, 6)):
            base, sig = inspect.signature(plain).parameters, inspect.signature(sunk).parameters
            names = [n for n in base if n != "softcap"]
            assert list(sig) == names[:behind] + ["sinks"] + names[behind:] and sig["sinks"].default is inspect.Parameter.empty, (mod, sunk)
            assert all(sig[n].default == base[n].default and sig[n].kind == base[n].kind for n in names), (mod, sunk)


def test_a_bad_sinks_is_a_runtime_error_before_the_library_and_a_bad_window_comes_first(monkeypatch):
    monkeypatch.setattr(_capi, "load", lambda: (_ for _ in ()).throw(AssertionError("the library was asked")))
    q4, q3 = torch.zeros((2, 1, 8, 128), dtype=torch.bfloat16), torch.zeros((2, 8, 128), dtype=torch.bfloat16)
    for mod, bad in ((m, b) for m in (flash_attention, fak) for b in _bad_sinks(8)):
        for kw, error, text in ({}, RuntimeError, "sinks"), (dict(causal=True, window_size=(5, 3)), ValueError, "causal means right = 0"):
            with pytest.raises(error, match=text):
                mod.forward_kvcache_sinks(q4, q4, q4, q4, bad, **kw)
            with pytest.raises(error, match=text):
                mod.forward_varlen_kvcache_sinks(q3, q4, q4, q4, 1, q4, bad, **kw)


def test_the_symbols_are_exported_and_declared():
    """(tests/test_host_cpu.py and tests/test_prefill_kvcache_cpu.py hold every EXPORTED_SYMBOLS entry to both libraries and the header)"""
    header = open(os.path.join(ROOT, "include", "fa_hip.h")).read()
    assert len(NEW_SYMBOLS) == 10 and set(NEW_SYMBOLS) <= set(_capi.EXPORTED_SYMBOLS) and all(f" {name}(" in header for name in NEW_SYMBOLS)
    libs = [ctypes.CDLL(os.path.join(ROOT, "flash_attention_from_scratch_amd", "lib", so)) for so in ("libfa_hip.so", "libfa_hip_jitter.so")]
    assert all(hasattr(lib, name) for lib in libs for name in NEW_SYMBOLS)
    assert _capi.load().fa_abi_version() == 6 and ctypes.sizeof(_capi.FaSinks) == 16


def _call(name, *argv):
    """one call of an entry point on host-only arguments -> (status, message)"""
    return getattr(_capi.load(), name)(*[_ref(x) if isinstance(x, ctypes.Structure) else x for x in argv]), _capi.last_error()


def _prefill(form, kind, window, *sinks, args=None, lse=16):
    scales = [_scales()] if form.endswith("fp8") else []
    return _call(f"fa_fwd_launch_{form}_{kind}", args or _fwd(), _kv(), _vl(), _contig(), *scales, window, *sinks, _capi.make_opts(),
                 ctypes.c_void_p(lse), None)


REFUSALS = [(None, -1, "fa_sinks is null"), (_sk(ptr=None, struct_size=0, n_heads=3), -1, "fa_sinks.sinks is null"),
            (_sk(struct_size=15, n_heads=3), -4, "fa_sinks.struct_size"), (_sk(n_heads=2), -4, "fa_sinks.n_heads")]


@pytest.mark.parametrize("sinks,status,text", REFUSALS, ids=[r[2] for r in REFUSALS])
def test_the_sinks_refusals_in_their_order_behind_the_siblings(sinks, status, text):
    for window in (_w(), _w(100, 0)):   # ((-1, -1) is legal here and means no window)
        for form in PREFILL:
            rc, msg = _prefill(form, "sinks", window, sinks)
            assert rc == status and text in msg, (form, rc, msg)
            # what the windowed sibling refuses comes first, with its status and words: a null fa_window, a bad d_head, a null lse
            for w, over in ((None, {}), (window, dict(args=_fwd(d_head=64))), (window, dict(lse=None))):
                got, want = _prefill(form, "sinks", w, sinks, **over), _prefill(form, "window", w, **over)
                assert got[0] == want[0] < 0 and got[1] == want[1].replace(f"{form}_window", f"{form}_sinks"), (got, want)
        for form, make in DECODE:
            launch, splits = _call(f"{form}_sinks_launch", make(), window, sinks, None, None), _call(f"{form}_sinks_num_splits", make(), window, sinks)
            assert launch[0] == splits[0] == status and text in launch[1] and text in splits[1], (form, launch, splits)
            assert _call(f"{form}_sinks_supported", make(), window, sinks)[0] == 0
            for w, over in ((None, {}), (window, dict(Sq=9, H=8, Hkv=1)), (_w(2000, 0), dict(workspace=None))):
                got, want = _call(f"{form}_sinks_launch", make(**over), w, sinks, None, None), _call(f"{form}_window_launch", make(**over), w, None, None)
                assert got[0] == want[0] < 0 and got[1] == want[1].replace(f"{form}_window_launch", f"{form}_sinks_launch"), (got, want)


def test_the_split_count_is_the_windowed_entrys():
    shapes = [dict(batch=1), dict(batch=64), dict(batch=8, Sq=16), dict(batch=2, num_splits=7), dict(batch=3, max_seqlen_k=300)]
    for (form, make), shape, window in itertools.product(DECODE, shapes, (_w(), _w(100, 0), _w(63, 3), _w(2000, -1))):
        want = _call(f"{form}_window_num_splits", make(**shape), window)[0]
        assert want >= 1 and _call(f"{form}_sinks_num_splits", make(**shape), window, _sk())[0] == want, (form, shape)
        assert _call(f"{form}_sinks_supported", make(**shape), window, _sk())[0] == 1
