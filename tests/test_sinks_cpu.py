"""Learned attention sinks in the varlen forward, backward and autograd path without a device: the Python surface
(forward_varlen_sinks, backward_varlen_sinks, attention_varlen_sinks in the three modules, the pinned functions unchanged), the
sinks validator, the exports (symbols, prototypes, every refusal before any HIP call and in its order, the sibling's first),
the ISA the build keeps for the new slices, and the proof that the inputs of tests/test_sinks_gpu.py discriminate: on each case of
its matrix an fp32 result WITHOUT the sinks misses the project's rules on o, dq and dk by a factor of 4 at least, all-zero and
negated dsinks miss the dsinks rule by as much, and the kernel's own dsinks formula stays well inside it."""
import ctypes
import inspect
import os
import re
import subprocess

import pytest
import torch

import beacon_inputs as bi
import flash_attention
import sinks_inputs as si
from flash_attention_from_scratch_amd import _capi
from flash_attention_from_scratch_amd import flash_attention_kernels as fak
from tests.conftest import ROOT
from tests.test_bwd_window_cpu import BAD_WINDOWS, MAX_LEN, WINDOW_REFUSALS
from tests.test_varlen_qk_cpu import _bwd, _fwd, _kv, _vl

BUILD = os.path.join(ROOT, "flash_attention_from_scratch_amd", "csrc", "build")
JITTER = os.path.join(ROOT, "flash_attention_from_scratch_amd", "lib", "libfa_hip_jitter.so")
NEW_SYMBOLS = ("fa_fwd_varlen_qk_sinks_supported", "fa_fwd_launch_varlen_qk_sinks", "fa_bwd_varlen_qk_sinks_workspace_bytes",
               "fa_bwd_launch_varlen_qk_sinks")


# ---- 1: signatures ----------------------------------------------------------------------------------------------------------------

def test_python_surface():
    import flash_attention_from_scratch_amd.flash_attention as inner

    fwd = ["q", "k", "v", "cu_seqlens", "max_seqlen", "sinks", "causal", "timed", "cu_seqlens_k", "max_seqlen_k", "window_size"]
    bwd = ["q", "k", "v", "o", "lse", "dout", "cu_seqlens", "max_seqlen", "sinks", "window_size", "causal", "timed", "cu_seqlens_k",
           "max_seqlen_k"]
    for mod in (flash_attention, inner, fak):
        sig = inspect.signature(mod.forward_varlen_sinks)
        assert list(sig.parameters) == fwd, mod
        assert [sig.parameters[n].default for n in fwd[6:]] == [False, False, None, None, (-1, -1)]
        assert sig.parameters["window_size"].kind is inspect.Parameter.KEYWORD_ONLY
        assert sig.parameters["sinks"].default is inspect.Parameter.empty and "softcap" not in sig.parameters
        sig = inspect.signature(mod.backward_varlen_sinks)
        assert list(sig.parameters) == bwd, mod
        assert [sig.parameters[n].default for n in bwd[9:]] == [(-1, -1), False, False, None, None]
        assert sig.parameters["sinks"].default is inspect.Parameter.empty
        assert all(p.kind is inspect.Parameter.POSITIONAL_OR_KEYWORD for p in sig.parameters.values())
    att = ["q", "k", "v", "cu_seqlens", "max_seqlen", "sinks", "causal", "cu_seqlens_k", "max_seqlen_k", "window_size"]
    for mod in (flash_attention, inner):
        sig = inspect.signature(mod.attention_varlen_sinks)
        assert list(sig.parameters) == att, mod
        assert [sig.parameters[n].default for n in att[6:]] == [False, None, None, (-1, -1)]
        assert sig.parameters["window_size"].kind is inspect.Parameter.KEYWORD_ONLY
    for name in ("forward_varlen_sinks", "backward_varlen_sinks", "attention_varlen_sinks"):
        assert getattr(flash_attention, name) is getattr(inner, name)
    # the pinned functions keep their signatures
    for mod in (flash_attention, inner, fak):
        params = inspect.signature(mod.forward_varlen).parameters
        assert list(params) == ["q", "k", "v", "cu_seqlens", "max_seqlen", "causal", "timed", "cu_seqlens_k", "max_seqlen_k", "window_size", "softcap"]
        for name in ("backward_varlen", "backward_varlen_window", "backward_varlen_softcap", "forward_varlen"):
            assert "sinks" not in inspect.signature(getattr(mod, name)).parameters, (mod, name)
        assert list(inspect.signature(mod.backward_varlen).parameters) == bwd[:8] + bwd[10:]
        assert list(inspect.signature(mod.backward_varlen_window).parameters) == bwd[:8] + ["window_size"] + bwd[10:]
        assert list(inspect.signature(mod.backward_varlen_softcap).parameters) == bwd[:8] + ["softcap"] + bwd[9:]
    for mod in (flash_attention, inner):
        assert list(inspect.signature(mod.attention_varlen).parameters) == att[:5] + att[6:] + ["softcap"]
    assert list(inspect.signature(inner._AttentionVarlen.forward).parameters) == [
        "ctx", "q", "k", "v", "cu_seqlens", "max_seqlen", "causal", "cu_seqlens_k", "max_seqlen_k", "window_size", "softcap"]
    # the new autograd function: sinks is an input with a gradient, everything behind it has none
    params = list(inspect.signature(inner._AttentionVarlenSinks.forward).parameters)
    assert params[:5] == ["ctx", "q", "k", "v", "sinks"]
    nones = ", ".join(["None"] * (len(params) - 5))
    assert re.search(rf"return dq, dk, dv, dsinks, {nones}\n", inspect.getsource(inner._AttentionVarlenSinks.backward))
    # the conversion to fp32 happens outside the Function, so that autograd casts the gradient back
    assert ".float()" in inspect.getsource(inner.attention_varlen_sinks)
    assert ".float()" not in inspect.getsource(inner._AttentionVarlenSinks)


# ---- 2: the validator -------------------------------------------------------------------------------------------------------------

def _bad_sinks(n_heads):
    good = torch.zeros(n_heads)
    return [None, 1.0, [0.0] * n_heads, good.double(), good.to(torch.bfloat16), good.to(torch.int32), torch.zeros(n_heads + 1),
            torch.zeros(n_heads - 1), torch.zeros((n_heads, 1)), torch.zeros((1, n_heads)), torch.zeros(()), torch.zeros(2 * n_heads)[::2]]


def test_bad_sinks_are_runtime_errors_before_the_library_is_loaded(monkeypatch):
    """CPU tensors of the right shapes: good sinks get as far as "must be a CUDA tensor", bad ones raise their own message -- and
    never load the library; a bad window raises first"""
    q = torch.zeros((8, 4, 128), dtype=torch.bfloat16)
    lse = torch.zeros((4, 8))
    cu = torch.tensor([0, 8], dtype=torch.int32)
    good = torch.zeros(4)

    def no_library():
        raise AssertionError("the library was asked")
    monkeypatch.setattr(_capi, "load", no_library)
    fak._check_sinks(good, q)
    for mod in (flash_attention, fak):
        with pytest.raises(RuntimeError, match="must be a CUDA tensor"):
            mod.forward_varlen_sinks(q, q, q, cu, 8, good)
        with pytest.raises(RuntimeError, match="must be a CUDA tensor"):
            mod.backward_varlen_sinks(q, q, q, q, lse, q, cu, 8, good)
    for sinks in (good, good.to(torch.bfloat16)):   # (q's dtype is accepted by the autograd entry and converted)
        with pytest.raises(RuntimeError, match="must be a CUDA tensor"):
            flash_attention.attention_varlen_sinks(q, q, q, cu, 8, sinks)
    for bad in _bad_sinks(4):
        for mod in (flash_attention, fak):
            with pytest.raises(RuntimeError, match="sinks must"):
                mod.forward_varlen_sinks(q, q, q, cu, 8, bad)
            with pytest.raises(RuntimeError, match="sinks must"):
                mod.backward_varlen_sinks(q, q, q, q, lse, q, cu, 8, bad)
        if isinstance(bad, torch.Tensor) and (bad.dtype == torch.bfloat16 or (bad.dim() == 1 and bad.shape[0] == 4)):
            continue   # (the autograd entry converts q's dtype and a strided vector)
        with pytest.raises(RuntimeError, match="sinks must"):
            flash_attention.attention_varlen_sinks(q, q, q, cu, 8, bad)
    with pytest.raises(RuntimeError, match="sinks must be fp32"):   # (neither fp32 nor q's dtype)
        flash_attention.attention_varlen_sinks(q, q, q, cu, 8, good.to(torch.float16))
    for window, causal, text in BAD_WINDOWS:
        for bad in (None, torch.zeros(5)):
            with pytest.raises(ValueError, match=text):
                flash_attention.forward_varlen_sinks(q, q, q, cu, 8, bad, causal=causal, window_size=window)
            with pytest.raises(ValueError, match=text):
                flash_attention.backward_varlen_sinks(q, q, q, q, lse, q, cu, 8, bad, window, causal=causal)
            with pytest.raises(ValueError, match=text):
                flash_attention.backward_varlen_sinks(None, None, None, None, None, None, None, None, bad, window, causal=causal)
            with pytest.raises(ValueError, match=text):
                flash_attention.attention_varlen_sinks(q, q, q, cu, 8, bad, causal=causal, window_size=window)


# ---- 3: the C ABI -----------------------------------------------------------------------------------------------------------------

def _w(left=-1, right=-1, **over):
    w = _capi.make_window(left, right)
    for name, value in over.items():
        setattr(w, name, value)
    return w


def _sk(n_heads=8, ptr=16, **over):
    s = _capi.make_sinks(ptr, n_heads)
    for name, value in over.items():
        setattr(s, name, value)
    return s


def _ref(x):
    return ctypes.byref(x) if x is not None else None


def _launch_fwd(window, sinks, entry="sinks", args=None, kv=None, vq=None, key=None, opts=None, lse=16):
    """one launch of the sinks forward (or of its windowed sibling) on host-only arguments -> (status, message)"""
    lib = _capi.load()
    args, kv, vq, opts = args or _fwd(), kv or _kv(), vq or _vl(), opts or _capi.make_opts()
    key = key or _vl(T=5000, max_seqlen=4096)
    argv = [ctypes.byref(args), ctypes.byref(kv), ctypes.byref(vq), ctypes.byref(key), _ref(window)]
    if entry == "sinks":
        argv.append(_ref(sinks))
    rc = getattr(lib, f"fa_fwd_launch_varlen_qk_{entry}")(*argv, ctypes.byref(opts), ctypes.c_void_p(lse) if lse is not None else None, None)
    return rc, _capi.last_error()


def _launch_bwd(window, sinks, entry="sinks", dsinks=16, **over):
    lib = _capi.load()
    a = _bwd(**over)
    argv = [ctypes.byref(a), _ref(window)]
    if entry == "sinks":
        argv += [_ref(sinks), ctypes.c_void_p(dsinks) if dsinks is not None else None]
    rc = getattr(lib, f"fa_bwd_launch_varlen_qk_{entry}")(*argv, None, None)
    return rc, _capi.last_error()


def test_symbols_prototypes_and_abi_version():
    assert set(NEW_SYMBOLS) <= set(_capi.EXPORTED_SYMBOLS)
    for path in (_capi.LIB_PATH, JITTER):
        nm = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True)
        exported = set(re.findall(r" T (fa_[a-z_0-9]+)", nm.stdout))
        assert set(NEW_SYMBOLS) <= exported, (path, set(NEW_SYMBOLS) - exported)
    header = re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "fa_hip.h")).read(), flags=re.S))
    assert "typedef struct fa_sinks { uint32_t struct_size; int32_t n_heads; const float *sinks; } fa_sinks;" in header
    assert "int fa_fwd_varlen_qk_sinks_supported(const fa_fwd_config *cfg, const fa_fwd_opts *opts);" in header
    assert ("int fa_fwd_launch_varlen_qk_sinks(const fa_fwd_args *args, const fa_kv_layout *kv, const fa_varlen_layout *varlen_q, "
            "const fa_varlen_layout *varlen_k, const fa_window *window, const fa_sinks *sinks, const fa_fwd_opts *opts, float *lse, "
            "void *stream);") in header
    assert "int64_t fa_bwd_varlen_qk_sinks_workspace_bytes(const fa_bwd_varlen_qk_args *args);" in header
    assert ("int fa_bwd_launch_varlen_qk_sinks(const fa_bwd_varlen_qk_args *args, const fa_window *window, const fa_sinks *sinks, "
            "float *dsinks, void *stream, float *ms);") in header
    lib = _capi.load()
    assert lib.fa_abi_version() == 6 and _capi.FA_ABI_VERSION == 6   # additive: no struct grew
    assert ctypes.sizeof(_capi.FaSinks) == 16 and ctypes.sizeof(_capi.FaWindow) == 12 and ctypes.sizeof(_capi.FaSoftcap) == 8
    assert _capi.FaSinks.sinks.offset == 8 and _capi.FaSinks.n_heads.offset == 4
    want = list(lib.fa_fwd_launch_varlen_qk_window.argtypes)
    fn = lib.fa_fwd_launch_varlen_qk_sinks
    assert list(fn.argtypes) == want[:-3] + [ctypes.POINTER(_capi.FaSinks)] + want[-3:] and fn.restype == ctypes.c_int
    want = list(lib.fa_bwd_launch_varlen_qk_window.argtypes)
    fn = lib.fa_bwd_launch_varlen_qk_sinks
    assert list(fn.argtypes) == want[:2] + [ctypes.POINTER(_capi.FaSinks), ctypes.c_void_p] + want[2:] and fn.restype == ctypes.c_int
    supported = lib.fa_fwd_varlen_qk_sinks_supported
    cfg = _capi.make_config(fak.varlen_config(torch.bfloat16))
    for o in (None, _capi.make_opts(causal=True), _capi.make_opts(speculative=True)):
        assert supported(ctypes.byref(cfg), _ref(o)) == lib.fa_fwd_varlen_supported(ctypes.byref(cfg), _ref(o))
    assert supported(ctypes.byref(cfg), None) == 1 and supported(None, None) == 0


def test_the_workspace_query_is_at_least_the_siblings():
    lib = _capi.load()
    for over in (dict(), dict(H=32, Hkv=8, T=32768, max_seqlen=8192, n_seqs=4), dict(causal=1), dict(T=0, Tk=0)):
        a = _bwd(**over)
        assert lib.fa_bwd_varlen_qk_sinks_workspace_bytes(ctypes.byref(a)) >= lib.fa_bwd_varlen_qk_workspace_bytes(ctypes.byref(a)) >= 0
    bad = _bwd(d_head=64)
    assert lib.fa_bwd_varlen_qk_sinks_workspace_bytes(ctypes.byref(bad)) == lib.fa_bwd_varlen_qk_workspace_bytes(ctypes.byref(bad)) < 0
    assert lib.fa_bwd_varlen_qk_sinks_workspace_bytes(None) < 0
    src = inspect.getsource(fak._backward_varlen)
    assert "fa_bwd_varlen_qk_sinks_workspace_bytes" in src and "fa_bwd_launch_varlen_qk_sinks" in src


SINKS_REFUSALS = [   # (fa_sinks, dsinks, status, text, forward too)
    (None, 16, -1, "fa_sinks is null", True),
    (_sk(ptr=None), 16, -1, "fa_sinks.sinks is null", True),
    (_sk(ptr=None, struct_size=0, n_heads=3), 16, -1, "fa_sinks.sinks is null", True),   # (null before shape)
    (_sk(), None, -1, "dsinks is null", False),
    (_sk(struct_size=0, n_heads=3), None, -1, "dsinks is null", False),                   # (null before shape)
    (_sk(struct_size=0), 16, -4, "fa_sinks.struct_size", True),
    (_sk(struct_size=8), 16, -4, "fa_sinks.struct_size", True),
    (_sk(struct_size=15, n_heads=3), 16, -4, "fa_sinks.struct_size", True),               # (struct_size before n_heads)
    (_sk(n_heads=7), 16, -4, "fa_sinks.n_heads", True),
    (_sk(n_heads=2), 16, -4, "fa_sinks.n_heads", True),                                   # (per QUERY head: not n_kv_heads)
    (_sk(n_heads=0), 16, -4, "fa_sinks.n_heads", True),
    (_sk(n_heads=-8), 16, -4, "fa_sinks.n_heads", True),
]


@pytest.mark.parametrize("case", SINKS_REFUSALS, ids=[str(i) for i in range(len(SINKS_REFUSALS))])
def test_sinks_refusals_without_a_device(case):
    sinks, dsinks, status, text, forward_too = case
    for window in (_w(), _w(127, 0), _w(63, 3)):   # ((-1, -1) is legal here and means no window)
        rc, msg = _launch_bwd(window, sinks, dsinks=dsinks)
        assert rc == status and text in msg, (rc, msg)
        if forward_too:
            rc, msg = _launch_fwd(window, sinks)
            assert rc == status and text in msg, (rc, msg)
    if sinks is None:   # (this level has no "off": the message says whose job that is)
        assert "windowed entry point" in _launch_fwd(_w(), None)[1] and "windowed entry point" in _launch_bwd(_w(), None)[1]


def test_the_windows_refusals_arrive_before_the_sinks():
    bad = _sk(n_heads=7)
    for window, causal, status, text in WINDOW_REFUSALS:
        for sinks, dsinks in ((bad, 16), (None, None)):
            rc, msg = _launch_fwd(window, sinks, opts=_capi.make_opts(causal=bool(causal)))
            assert rc == status and text in msg, (rc, msg)
            rc, msg = _launch_bwd(window, sinks, dsinks=dsinks, causal=causal)
            assert rc == status and text in msg, (rc, msg)
    for side in (dict(max_seqlen=MAX_LEN + 1), dict(max_seqlen_k=MAX_LEN + 1)):
        rc, msg = _launch_bwd(_w(100, 0), bad, T=0, Tk=0, **side)
        assert rc == -4 and "too large for a window" in msg
    rc, msg = _launch_fwd(_w(100, 0), bad, args=_fwd(T=0), vq=_vl(T=0, max_seqlen=MAX_LEN + 1))
    assert rc == -4 and "too large for a window" in msg
    rc, msg = _launch_fwd(_w(100, 0), bad, args=_fwd(T=0), vq=_vl(T=0), key=_vl(T=0, max_seqlen=MAX_LEN + 1))
    assert rc == -4 and "too large for a window" in msg
    # ... and the sinks' own before "nothing to do": both totals zero with bad sinks is still refused, with good ones FA_OK
    assert _launch_bwd(_w(), bad, T=0, Tk=0)[0] == -4 and _launch_fwd(_w(), bad, args=_fwd(T=0), vq=_vl(T=0))[0] == -4
    assert _launch_bwd(_w(), _sk(), dsinks=None, T=0, Tk=0)[0] == -1
    ms = ctypes.c_float(-1.0)
    lib = _capi.load()
    assert lib.fa_bwd_launch_varlen_qk_sinks(ctypes.byref(_bwd(T=0, Tk=0)), ctypes.byref(_w()), ctypes.byref(_sk()), ctypes.c_void_p(16), None,
                                             ctypes.byref(ms)) == 0
    assert ms.value == 0.0
    assert _launch_fwd(_w(), _sk(), args=_fwd(T=0), vq=_vl(T=0))[0] == 0


def test_what_the_windowed_sibling_refuses_arrives_first_with_its_words():
    bad_w, bad = _w(-5, -5), _sk(n_heads=7)
    vl = lambda **kw: _capi.make_varlen_layout(kw.pop("cu", 16), kw.pop("n_seqs", 3), kw.pop("T", 1000), kw.pop("max_seqlen", 512))   # noqa: E731
    cases = [(dict(lse=None), -1, "lse is null"), (dict(dk=None), -1, "null tensor pointer"), (dict(workspace=None), -1, "workspace is null"),
             (dict(dtype=7), -2, "fp16 and bf16"), (dict(d_head=64), -4, "d_head = 128"), (dict(Hkv=3), -4, "divide"),
             (dict(kv_seq_stride=2 * 128 + 4), -5, "multiples of 8"), (dict(workspace=20), -5, "workspace must be 16-byte"),
             (dict(varlen=vl(cu=18)), -5, "cu_seqlens must be 4-byte"), (dict(struct_size=8), -4, "fa_bwd_varlen_qk_args.struct_size"),
             (dict(k_over=dict(n_seqs=4)), -4, "n_seqs mismatch"), (dict(q_seq_stride=(1 << 23) + 8), -4, "too large")]
    for over, status, text in cases:
        for window, sinks, dsinks in ((bad_w, bad, 16), (None, None, None), (_w(), bad, None)):
            rc, msg = _launch_bwd(window, sinks, dsinks=dsinks, **over)
            assert rc == status and text in msg, (over, rc, msg)
            rc0, msg0 = _launch_bwd(window, None, entry="window", **over)
            assert rc0 == rc and msg0 == msg, (msg0, msg)
    lib = _capi.load()
    assert lib.fa_bwd_launch_varlen_qk_sinks(None, ctypes.byref(bad_w), ctypes.byref(bad), None, None, None) == -1
    fwd_cases = [(dict(lse=None), -1, "lse is null"), (dict(args=_fwd(d_head=64)), -4, "d_head"), (dict(vq=_vl(cu=18)), -5, "cu_seqlens must be 4-byte")]
    new, sibling = "fa_fwd_launch_varlen_qk_sinks", "fa_fwd_launch_varlen_qk_window"
    for over, status, text in fwd_cases:
        rc, msg = _launch_fwd(bad_w, bad, **over)
        assert rc == status and text in msg, (over, rc, msg)
        rc0, msg0 = _launch_fwd(bad_w, None, entry="window", **over)
        assert rc0 == rc and msg0.replace(sibling, new) == msg, (msg0, msg)


# ---- 4: the kept ISA --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dt", [15, 5])
def test_the_forward_slice_is_kept_with_two_kernels_mfma_no_scratch_no_vector_spill(dt):
    path = os.path.join(BUILD, f"varlen_sinks_dt{dt}", "fa_inst_varlen-hip-amdgcn-amd-amdhsa-gfx950.s")
    assert os.path.exists(path), "the build keeps the ISA of every slice under csrc/build (make -C flash_attention_from_scratch_amd/csrc)"
    text = open(path).read()
    names = set(re.findall(r"^\s+\.name:\s+(_Z\w+)$", text, re.M))
    want = {f"_ZN2fa26fa_fwd_kernel_varlen_sinksILi{dt}ELi1ELi4ELi64ELb1ELb1ELb{opt}ELb1ELb1ELb1ELi128ELi0ELi1EEEv"
            "NS_4SunkINS_8WindowedINS_18KernelArgsVarlenQKEEEEE" for opt in (0, 1)}   # (with and without the first-block skip)
    assert names == want, names ^ want
    for name in want:
        assert re.search(rf"^{name}:", text, flags=re.M), name
    mine, other = ("bf16", "_f16") if dt == 15 else ("_f16", "bf16")
    mfma = set(re.findall(r"\bv_mfma_\w+", text))
    assert mfma and all(mine in m for m in mfma) and not any(other in m for m in mfma), mfma
    assert "scratch_" not in text
    assert re.findall(r"\.amdhsa_private_segment_fixed_size (\d+)", text) == ["0", "0"]
    assert re.findall(r"\.private_segment_fixed_size:\s+(\d+)", text) == ["0", "0"]
    assert re.findall(r"; ScratchSize: (\d+)", text) == ["0", "0"]
    assert re.findall(r"\.vgpr_spill_count:\s+(\d+)", text) == ["0", "0"]
    print(f"varlen_sinks dt{dt}: vgpr_count", re.findall(r"\.vgpr_count:\s+(\d+)", text), "sgpr_spill_count",
          re.findall(r"\.sgpr_spill_count:\s+(\d+)", text))


def test_the_backward_unit_is_kept_with_one_kernel_no_mfma_no_scratch_no_spills_no_atomics():
    """the unit builds none of the header's kernels (dQ, dK, dV are the window unit's, unchanged): one kernel, the dsinks reduction"""
    path = os.path.join(BUILD, "bwd_varlen_sinks", "fa_bwd_varlen_sinks-hip-amdgcn-amd-amdhsa-gfx950.s")
    assert os.path.exists(path), "the build keeps the ISA of every slice under csrc/build (make -C flash_attention_from_scratch_amd/csrc)"
    text = open(path).read()
    names = re.findall(r"^\s+\.name:\s+(_Z\w+)$", text, re.M)
    assert names == ["_ZN2fa27fa_bwd_dsinks_varlen_kernelENS_18BwdVarlenSinksArgsE"], names
    assert not re.findall(r"\bv_mfma_\w+", text)
    assert "scratch_" not in text and "atomic" not in text   # a fixed order of sums
    assert re.findall(r"\.amdhsa_private_segment_fixed_size (\d+)", text) == ["0"]
    assert re.findall(r"; ScratchSize: (\d+)", text) == ["0"]
    assert re.findall(r"\.vgpr_spill_count:\s+(\d+)", text) == ["0"] and re.findall(r"\.sgpr_spill_count:\s+(\d+)", text) == ["0"]
    assert "v_exp_f32" in text
    # ... and the window unit still holds the kernels the sinks backward runs
    window = open(os.path.join(BUILD, "bwd_varlen_window", "fa_bwd_varlen_window-hip-amdgcn-amd-amdhsa-gfx950.s")).read()
    for kernel in ("25fa_bwd_dkdv_varlen_kernel", "23fa_bwd_dq_varlen_kernel"):
        for dt in (15, 5):
            assert f"_ZN2fa{kernel}INS_19BwdVarlenWindowArgsELi{dt}ELb0EEEvT_" in window


# ---- 5: the inputs discriminate ---------------------------------------------------------------------------------------------------

PROOF = [(heads, window, dtype) for heads in si.HEADS for window in si.WINDOWS for dtype in si.DTYPES]


@pytest.mark.parametrize("case", PROOF, ids=str)
def test_the_inputs_reject_missing_sinks_and_wrong_dsinks(case):
    """For each case of the GPU matrix, with SINKS_LIVE, seed 0.  On the sequences the proof leans on (PROOF_SEQS): the 16-bit
    reference passes the forward rule, and the fp32 result WITHOUT sinks misses bi.compare on o and bi.grad_rule on dq and dk by a
    factor >= 4.  On the whole launch: all-zero and negated dsinks miss the dsinks rule by a factor >= 4, and the kernel's own
    formula, in fp32 from o32 rounded to 16 bit and lse32, stays at ratio <= 0.5.
    (Measured minima over the 32 cases: o 17.6, dq 40.8, dk 39.9, zero 51, negated 103; the formula's worst 0.39.)"""
    heads, window, dtype = case
    inp = si.inputs(heads, dtype)
    z = si.SINKS_LIVE(heads[0])
    for i in si.PROOF_SEQS:
        q, k, v, dout = si.sequence(inp, i)
        r = si.reference(heads, dtype, window, i)
        assert bi.compare(r["o16"], None, r["o32"], r["lse32"], r["o16"], dtype)["ok"]
        o_n, _, g_n, _ = si.sink_backward(q, k, v, dout, None, window, torch.float32)
        res = bi.compare(o_n, None, r["o32"], r["lse32"], r["o16"], dtype)
        ratios = dict(o=res["err"] / res["bound"])
        for name, j in (("dq", 0), ("dk", 1)):
            ratios[name] = bi.grad_rule(g_n[j], r["g32"][j], r["g16"][j])["ratio"]
        print(f"{case} sequence {inp['pairs'][i]}: without sinks, err / bound " + ", ".join(f"{n} {x:.1f}" for n, x in ratios.items()))
        assert min(ratios.values()) >= 4.0, (case, inp["pairs"][i], ratios)
    d32, d16 = si.dsinks_references(heads, dtype, window)
    zero = bi.grad_rule(torch.zeros_like(d32), d32, d16)["ratio"]
    negated = bi.grad_rule(-d32, d32, d16)["ratio"]
    formula = torch.zeros_like(d32)
    for i, r in enumerate(si.references(heads, dtype, window)):
        dout = si.sequence(inp, i)[3]
        formula += si.dsinks_formula(r["o32"].to(dtype), r["lse32"], dout, z)
    own = bi.grad_rule(formula, d32, d16)["ratio"]
    print(f"{case} dsinks: zero {zero:.1f}, negated {negated:.1f}, the kernel's formula {own:.2f}")
    assert zero >= 4.0 and negated >= 4.0, (case, zero, negated)
    assert own <= 0.5, (case, own)


def test_the_reference_restates_the_definition():
    """the eager reference against the closed form on one sequence: lse = log(exp(z) + sum exp(s)), dead rows o = 0 and lse = z,
    z = -inf the call without sinks (a dead row's lse = -inf), no NaN, and autograd's dsinks = the formula's"""
    heads, dtype, window = (8, 2), torch.bfloat16, (100, -1, True)
    inp = si.inputs(heads, dtype)
    z = si.SINKS_EDGE(heads[0])
    for i in (1, 5, 6):   # (129, 300), (5, 0): every row dead, (257, 130): the first rows dead under the causal mask
        q, k, v, dout = si.sequence(inp, i)
        o, lse, g, dz = si.sink_backward(q, k, v, dout, z, window, torch.float32)
        o_n, lse_n, g_n, _ = si.sink_backward(q, k, v, dout, None, window, torch.float32)
        dead = si.dead_rows(q.shape[0], k.shape[0], window)
        assert not any(bool(torch.isnan(t).any()) for t in (o, lse, dz, *g))
        assert bool((o[dead] == 0).all()) and bool((g[0][dead] == 0).all())
        assert torch.equal(lse[:, dead], z[:, None].expand(-1, int(dead.sum())))
        assert torch.allclose(lse[:, ~dead], torch.logaddexp(lse_n[:, ~dead], z[:, None].expand(-1, int((~dead).sum()))), atol=1e-5, rtol=0)
        assert torch.equal(o[:, 2], o_n[:, 2]) and torch.equal(lse[2], lse_n[2]) and dz[2] == 0 and dz[1] == 0
        assert bool((o[~dead][:, 0].abs() < 1e-30).all()) and bool(((lse[0] - 120.0).abs() < 1e-3).all())
        assert torch.allclose(dz, si.dsinks_formula(o, lse, dout, z), atol=1e-5, rtol=1e-4)
