"""KV-cache decode at d_head = 64 against an fp8 cache without a device: the four exports, the split rule and the
workspace equal to the 16-bit entry's, the refusals -- the 16-bit entry's first, then the fp8 side's -- batch = 0, and the wrapper's
errors before the library loads."""
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
from tests.test_decode_cpu import _args as _args16
from tests.test_decode_fp8_cpu import _args as _args8
from tests.test_sinks_cpu import _ref, _sk, _w

SYMBOLS = tuple(f"fa_decode_fp8_d64_{what}" for what in ("supported", "num_splits", "workspace_bytes", "launch"))


def _call(what, args, window, sinks, *more, entry="fa_decode_fp8_d64_"):
    return getattr(_capi.load(), entry + what)(_ref(args), _ref(window), _ref(sinks), *more), _capi.last_error()


def test_the_four_symbols_are_exported_and_declared_and_batch_zero_is_ok():
    header = open(os.path.join(ROOT, "include", "fa_hip.h")).read()
    assert set(SYMBOLS) <= set(_capi.EXPORTED_SYMBOLS) and all(f" {name}(" in header for name in SYMBOLS)
    libs = [ctypes.CDLL(os.path.join(ROOT, "flash_attention_from_scratch_amd", "lib", so)) for so in ("libfa_hip.so", "libfa_hip_jitter.so")]
    assert all(hasattr(lib, name) for lib in libs for name in SYMBOLS) and _capi.load().fa_abi_version() == 6
    ms = ctypes.c_float(-1.0)   # batch = 0 is OK without a device
    assert _call("launch", _args8(batch=0, d_head=64), _w(), _sk(), None, ctypes.byref(ms))[0] == 0 and ms.value == 0.0


@pytest.mark.parametrize("batch,Hkv,max_k,window", [(1, 2, 0, (-1, -1)), (8, 8, 65536, (-1, -1)), (64, 8, 65536, (-1, -1)), (8, 8, 65536, (127, 0)),
                                                    (2, 1, 300, (-1, -1)), (3, 2, 65536, (1000, 30))])
def test_the_split_count_and_the_workspace_are_the_16_bit_entrys(batch, Hkv, max_k, window):
    shape = dict(batch=batch, Sq=2, H=8, Hkv=Hkv, cache=65536, d_head=64, max_seqlen_k=max_k)
    for sinks in (None, _sk()):
        for what in ("supported", "num_splits", "workspace_bytes"):
            want = _call(what, _args16(**shape), _w(*window), sinks, entry="fa_decode_d64_")[0]
            assert want > 0 or what == "workspace_bytes"
            assert _call(what, _args8(**shape), _w(*window), sinks)[0] == want, what


# (over, window, sinks, status, text): what fa_decode_d64_launch refuses comes first, in its words, whatever the fp8 side holds
BAD8 = dict(kv_dtype=0, descale_batch_stride=1)
REFUSALS = [(dict(d_head=128, **BAD8), _w(), None, -4, "d_head = 64 only"), (dict(d_head=64, Sq=9, H=8, Hkv=1, **BAD8), _w(), None, -3, "64 packed query rows"),
            (dict(d_head=64, paged=(8, 32, 4), **BAD8), _w(), None, -3, "multiple of 64"), (dict(d_head=64, dtype=7, **BAD8), _w(), None, -2, "Only fp16 and bf16"),
            (dict(d_head=64, **BAD8), None, None, -1, "fa_window is null"), (dict(d_head=64, causal=1, **BAD8), _w(5, 3), None, -4, "causal means right = 0"),
            (dict(d_head=64, **BAD8), _w(), _sk(ptr=None), -1, "fa_sinks.sinks is null"), (dict(d_head=64, **BAD8), _w(), _sk(n_heads=2), -4, "fa_sinks.n_heads"),
            (dict(d_head=64, batch=1, Hkv=1, workspace=None, kv_dtype=0), _w(), None, -1, "fa_decode_fp8_d64_workspace_bytes"),
            # ... then the fp8 side, in fa_decode_fp8_sinks_launch's words
            (dict(d_head=64, **BAD8), _w(), _sk(), -2, "kv_dtype"), (dict(d_head=64, descale_batch_stride=1), _w(), None, -4, "descale_batch_stride"),
            (dict(d_head=64, kv_seq_stride=264), _w(), None, -5, "multiples of 16 bytes"),
            (dict(d_head=64, v_descale=18), _w(), None, -5, "k_descale and v_descale must be 4-byte aligned")]


@pytest.mark.parametrize("over,window,sinks,status,text", REFUSALS, ids=[r[4] for r in REFUSALS])
def test_the_refusals_and_their_statuses(over, window, sinks, status, text):
    rc, msg = _call("launch", _args8(**over), window, sinks, None, None)
    assert rc == status and text in msg, (rc, msg)
    if "workspace" not in text and "aligned" not in text:   # (the queries refuse what the launch refuses of the shapes)
        assert _call("supported", _args8(**over), window, sinks)[0] == 0 and _call("num_splits", _args8(**over), window, sinks)[0] == status
        assert _call("workspace_bytes", _args8(**over), window, sinks)[0] == status


def test_the_wrappers_errors_come_before_the_library_loads(monkeypatch):
    monkeypatch.setattr(_capi, "load", lambda: (_ for _ in ()).throw(AssertionError("the library was asked")))
    q, lens, ones = torch.zeros((2, 1, 8, 64), dtype=torch.bfloat16), torch.zeros(2, dtype=torch.int32), torch.ones((2, 2))
    k8 = torch.zeros((2, 128, 2, 64)).to(torch.float8_e4m3fn)
    for mod in (flash_attention, fak):
        for fn in (mod.forward_kvcache_d64, mod.kvcache_d64_num_splits):
            for given in ({}, dict(k_descale=ones), dict(v_descale=ones)):
                with pytest.raises(RuntimeError, match="(?s)fp8.*pass ones"):
                    fn(q, k8, k8, lens, **given)
                with pytest.raises(ValueError, match="window_size"):   # a bad window first
                    fn(q, k8, k8, lens, window_size=(-2, 0), **given)
            with pytest.raises(RuntimeError, match="16-bit"):
                fn(q, k8.to(torch.bfloat16), k8.to(torch.bfloat16), lens, k_descale=ones)


@pytest.mark.parametrize("name", ["forward_kvcache_d64", "kvcache_d64_num_splits"])
def test_one_signature_in_the_three_modules(name):
    sigs = [inspect.signature(getattr(mod, name)) for mod in (flash_attention, inner, fak)]
    assert sigs[0] == sigs[1] == sigs[2] and [(p.name, p.default) for p in list(sigs[0].parameters.values())[-2:]] == [("k_descale", None), ("v_descale", None)]
