"""The packed backward at d_head = 64 without a device: the two exports, the C-level refusals in their order with the siblings'
words before any HIP call, both totals zero, the workspace from the split rule, the wrapper's errors before the library loads, the signatures."""
import ctypes
import inspect
import os

import pytest
import torch

import flash_attention
from flash_attention_from_scratch_amd import _capi
from flash_attention_from_scratch_amd import flash_attention_kernels as fak
from tests.conftest import ROOT
from tests.test_bwd_window_cpu import MAX_LEN
from tests.test_sinks_cpu import _ref, _sk, _w
from tests.test_varlen_qk_cpu import _bwd, _expected_split

SYMBOLS = ("fa_bwd_varlen_qk_d64_workspace_bytes", "fa_bwd_launch_varlen_qk_d64")


def _bwd64(H=8, Hkv=2, **over):
    """test_varlen_qk_cpu's host-only arguments with 64-wide rows"""
    strides = {f"{t}_{s}_stride": n for t, h in (("q", H), ("out", H), ("kv", Hkv), ("dkv", Hkv)) for s, n in (("seq", h * 64), ("head", 64))}
    return _bwd(H=H, Hkv=Hkv, **{**dict(d_head=64), **strides, **over})


def _launch(window=_w(), sinks=None, dsinks=16, entry="d64", **over):
    argv = [ctypes.byref(_bwd64(**over) if entry == "d64" else _bwd(**over)), _ref(window)]
    if entry != "window":
        argv += [_ref(sinks), ctypes.c_void_p(dsinks) if dsinks is not None else None]
    rc = getattr(_capi.load(), f"fa_bwd_launch_varlen_qk_{entry}")(*argv, None, None)
    return rc, _capi.last_error()


def test_the_two_symbols_are_exported_and_declared():
    header = open(os.path.join(ROOT, "include", "fa_hip.h")).read()
    assert set(SYMBOLS) <= set(_capi.EXPORTED_SYMBOLS) and all(f" {name}(" in header for name in SYMBOLS)
    libs = [ctypes.CDLL(os.path.join(ROOT, "flash_attention_from_scratch_amd", "lib", so)) for so in ("libfa_hip.so", "libfa_hip_jitter.so")]
    assert all(hasattr(lib, name) for lib in libs for name in SYMBOLS) and _capi.load().fa_abi_version() == 6
    assert list(_capi.load().fa_bwd_launch_varlen_qk_d64.argtypes) == list(_capi.load().fa_bwd_launch_varlen_qk_sinks.argtypes)
    assert all(getattr(flash_attention, name).__module__.endswith("flash_attention") for name in ("backward_varlen_d64", "attention_varlen_d64"))


# in order: the windowed sibling's (the head dimension behind the dtype, in front of the layouts), the window's, a non-null fa_sinks', a null dsinks
REFUSALS = [(dict(dtype=7, d_head=128), {}, -2, "fp16 and bf16"),
            (dict(d_head=128, Hkv=3), {}, -4, "d_head = 64 only (got 128"),
            (dict(Hkv=3, lse=None), {}, -4, "divide"),
            (dict(lse=None), dict(window=None), -1, "lse is null"),
            (dict(workspace=None), dict(window=None), -1, "workspace is null"),
            (dict(), dict(window=None, sinks=_sk(n_heads=7)), -1, "fa_window is null"),
            (dict(causal=1), dict(window=_w(5, 3), sinks=_sk(ptr=None)), -4, "causal means right = 0"),
            (dict(max_seqlen_k=MAX_LEN + 1, T=0, Tk=0), dict(sinks=_sk(ptr=None)), -4, "max_seqlen_k too large for a window"),
            (dict(max_seqlen=MAX_LEN + 1, max_seqlen_k=512, T=0, Tk=0), dict(sinks=_sk(ptr=None)), -4, "max_seqlen_q too large for a window"),
            (dict(), dict(sinks=_sk(ptr=None), dsinks=None), -1, "fa_sinks.sinks is null"),
            (dict(), dict(sinks=_sk(struct_size=8, n_heads=7), dsinks=None), -4, "fa_sinks.struct_size"),
            (dict(), dict(sinks=_sk(n_heads=2), dsinks=None), -4, "fa_sinks.n_heads"),
            (dict(T=0, Tk=0), dict(sinks=_sk(), dsinks=None), -1, "dsinks is null")]


@pytest.mark.parametrize("over,call,status,text", REFUSALS, ids=[r[3] for r in REFUSALS])
def test_the_refusals_their_statuses_and_their_order(over, call, status, text):
    rc, msg = _launch(**call, **over)
    assert rc == status and text in msg, (rc, msg)


def test_the_siblings_words_both_totals_zero_and_the_siblings_keep_theirs():
    for over in (dict(lse=None), dict(dk=None), dict(workspace=20), dict(Hkv=3), dict(struct_size=8), dict(k_over=dict(n_seqs=4))):
        (rc, msg), (rc0, msg0) = _launch(**over), _launch(entry="window", **over)
        assert rc == rc0 < 0 and msg == msg0.replace("fa_bwd_varlen_qk_workspace_bytes", "fa_bwd_varlen_qk_d64_workspace_bytes"), (msg, msg0)
    ms = ctypes.c_float(-1.0)
    for sinks, dsinks in ((None, None), (_sk(), ctypes.c_void_p(16))):
        rc = _capi.load().fa_bwd_launch_varlen_qk_d64(ctypes.byref(_bwd64(T=0, Tk=0)), ctypes.byref(_w()), _ref(sinks), dsinks, None, ctypes.byref(ms))
        assert rc == 0 and ms.value == 0.0
    assert _capi.load().fa_bwd_launch_varlen_qk_d64(None, None, None, None, None, None) == -1
    for entry in ("sinks", "window"):   # (a 64-wide q into the d128 entries: their words, unchanged)
        rc, msg = _launch(entry=entry, sinks=_sk(), d_head=64)
        assert rc == -4 and "the backward supports d_head = 128 only (got 64)" in msg


@pytest.mark.parametrize("n_seqs,max_k,H,Hkv,causal", [(8, 600, 8, 2, 0), (8, 600, 4, 4, 0), (8, 600, 8, 2, 1), (8, 1024, 8, 2, 0), (8, 4096, 8, 2, 0),
                                                     (4, 8192, 64, 8, 1), (1, 1000, 8, 1, 0)])
def test_the_workspace_follows_from_the_split_rule(n_seqs, max_k, H, Hkv, causal):
    """delta rounded up to 16 bytes, then split > 1: (n_kv_heads * split, total_k, 2, 64) fp32; the GPU file's heads get 4 and 1"""
    Tq, Tk = 886, 1337
    a = _bwd64(H=H, Hkv=Hkv, n_seqs=n_seqs, T=Tq, Tk=Tk, max_seqlen=300, max_seqlen_k=max_k, causal=causal)
    split = _expected_split(n_seqs, max_k, H, Hkv, causal)
    want = ((4 * H * Tq + 15) & ~15) + (4 * Hkv * split * Tk * 2 * 64 if split > 1 else 0)
    assert _capi.load().fa_bwd_varlen_qk_d64_workspace_bytes(ctypes.byref(a)) == want
    if (n_seqs, max_k, causal) == (8, 600, 0):
        assert split == (4 if (H, Hkv) == (8, 2) else 1)
    assert _capi.load().fa_bwd_varlen_qk_d64_workspace_bytes(ctypes.byref(_bwd64(d_head=128))) == -4


def test_the_wrappers_errors_come_before_the_library_loads(monkeypatch):
    monkeypatch.setattr(_capi, "load", lambda: (_ for _ in ()).throw(AssertionError("the library was asked")))
    q, cu, lse = torch.zeros((8, 8, 64), dtype=torch.bfloat16), torch.tensor([0, 8], dtype=torch.int32), torch.zeros((8, 8))
    for mod in (flash_attention, fak):
        call = lambda **kw: mod.backward_varlen_d64(q, q, q, q, lse, q, cu, 8, **kw)   # noqa: E731
        for bad in (1.0, torch.zeros(8, dtype=torch.float64), torch.zeros(7), torch.zeros(16)[::2]):
            with pytest.raises(RuntimeError, match="sinks"):
                call(sinks=bad)
            with pytest.raises(ValueError, match="causal means right = 0"):   # a bad window first
                call(sinks=bad, causal=True, window_size=(5, 3))
        with pytest.raises(ValueError, match="window_size"):
            mod.backward_varlen_d64(None, None, None, None, None, None, None, None, window_size=(-2, 0))
        with pytest.raises(RuntimeError, match="must be a CUDA tensor"):   # (good arguments get as far as the device check)
            call(sinks=torch.zeros(8))
    for sinks in (None, torch.zeros(8), torch.zeros(8, dtype=torch.bfloat16)):   # (q's dtype is converted, None is no sinks)
        with pytest.raises(RuntimeError, match="must be a CUDA tensor"):
            flash_attention.attention_varlen_d64(q, q, q, cu, 8, sinks)


def test_the_signatures():
    import flash_attention_from_scratch_amd.flash_attention as inner

    bwd = ["q", "k", "v", "o", "lse", "dout", "cu_seqlens", "max_seqlen", "sinks", "window_size", "causal", "timed", "cu_seqlens_k", "max_seqlen_k"]
    for mod in (flash_attention, inner, fak):
        sig = inspect.signature(mod.backward_varlen_d64)
        assert list(sig.parameters) == bwd and [sig.parameters[n].default for n in bwd[8:]] == [None, (-1, -1), False, False, None, None], mod
        assert list(inspect.signature(mod.backward_varlen_sinks).parameters) == bwd   # (pinned: unchanged)
    sig = inspect.signature(inner.attention_varlen_d64)
    assert list(sig.parameters) == ["q", "k", "v", "cu_seqlens", "max_seqlen", "sinks", "causal", "cu_seqlens_k", "max_seqlen_k", "window_size"]
    assert sig.parameters["window_size"].kind is inspect.Parameter.KEYWORD_ONLY and sig.parameters["sinks"].default is None
