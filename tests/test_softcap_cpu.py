"""Logit soft-capping in the varlen forward, backward and autograd path without a device: the Python surface
(softcap= keyword only on forward_varlen and attention_varlen, backward_varlen_softcap in the three modules, the validator), the
three exports (symbols, prototypes, every refusal before any HIP call and in its order, the sibling's first), the ISA the build
keeps for the two new slices, and the proof that the inputs of tests/test_softcap_gpu.py discriminate: on each case of its
matrix an fp32 result WITHOUT the cap, and fp32 gradients with the factor 1 - tanh^2 dropped, miss the project's rules by a factor
of 4 at least."""
import ctypes
import inspect
import os
import re
import subprocess

import pytest
import torch

import beacon_inputs as bi
import flash_attention
import softcap_inputs as sc
from flash_attention_from_scratch_amd import _capi
from flash_attention_from_scratch_amd import flash_attention_kernels as fak
from tests.conftest import ROOT
from tests.test_prefill_kvcache_cpu import _fwd, _kv, _vl
from tests.test_varlen_qk_cpu import _bwd

BUILD = os.path.join(ROOT, "flash_attention_from_scratch_amd", "csrc", "build")
JITTER = os.path.join(ROOT, "flash_attention_from_scratch_amd", "lib", "libfa_hip_jitter.so")
NEW_SYMBOLS = ("fa_fwd_varlen_qk_softcap_supported", "fa_fwd_launch_varlen_qk_softcap", "fa_bwd_launch_varlen_qk_softcap")


# ---- 1: signatures ----------------------------------------------------------------------------------------------------------------

def test_python_surface():
    import flash_attention_from_scratch_amd.flash_attention as inner

    for mod in (flash_attention, inner, fak):
        params = inspect.signature(mod.forward_varlen).parameters
        assert list(params)[-2:] == ["window_size", "softcap"], mod
        assert params["softcap"].kind is inspect.Parameter.KEYWORD_ONLY and params["softcap"].default == 0.0
    for mod in (flash_attention, inner):
        params = inspect.signature(mod.attention_varlen).parameters
        assert list(params)[-2:] == ["window_size", "softcap"], mod
        assert params["softcap"].kind is inspect.Parameter.KEYWORD_ONLY and params["softcap"].default == 0.0
    want = ["q", "k", "v", "o", "lse", "dout", "cu_seqlens", "max_seqlen", "softcap", "window_size", "causal", "timed", "cu_seqlens_k",
            "max_seqlen_k"]
    for mod in (flash_attention, inner, fak):
        sig = inspect.signature(mod.backward_varlen_softcap)
        assert list(sig.parameters) == want, mod
        assert [sig.parameters[n].default for n in want[9:]] == [(-1, -1), False, False, None, None]
        assert sig.parameters["softcap"].default is inspect.Parameter.empty
        assert all(p.kind is inspect.Parameter.POSITIONAL_OR_KEYWORD for p in sig.parameters.values())
    assert flash_attention.backward_varlen_softcap is inner.backward_varlen_softcap
    assert flash_attention.backward_varlen_window is inner.backward_varlen_window
    for mod in (flash_attention, inner, fak):   # (these keep their signatures)
        for name in ("backward_varlen", "backward_varlen_window", "forward_kvcache"):
            assert "softcap" not in inspect.signature(getattr(mod, name)).parameters, (mod, name)
    # the autograd function: one more trailing argument with a default, one more None from the backward
    fwd = inspect.signature(inner._AttentionVarlen.forward).parameters
    assert list(fwd)[-2:] == ["window_size", "softcap"] and fwd["softcap"].default == 0.0
    assert "ctx.softcap" in inspect.getsource(inner._AttentionVarlen.forward)
    nones = ", ".join(["None"] * (len(fwd) - 1 - 3))   # (one per input that is not q, k, v; fwd counts ctx)
    assert re.search(rf"return dq, dk, dv, {nones}\n", inspect.getsource(inner._AttentionVarlen.backward))


# ---- 2: the validator -------------------------------------------------------------------------------------------------------------

BAD_SOFTCAPS = [-1.0, float("nan"), float("inf"), True, "5", torch.tensor(5.0), None]


def test_the_validator():
    assert fak._softcap(0) is None and fak._softcap(0.0) is None and fak._softcap(-0.0) is None
    assert fak._softcap(30) == 30.0 and isinstance(fak._softcap(30), float) and fak._softcap(50.0) == 50.0
    for bad in BAD_SOFTCAPS + [float("-inf"), -1, False, [5.0], 10 ** 400]:
        with pytest.raises(ValueError, match="softcap"):
            fak._softcap(bad)


def test_bad_softcaps_are_value_errors_before_any_tensor_is_looked_at(monkeypatch):
    """CPU tensors of the right shapes: a good softcap gets as far as "must be a CUDA tensor", a bad one never does -- and never
    loads the library either"""
    q = torch.zeros((8, 4, 128), dtype=torch.bfloat16)
    lse = torch.zeros((4, 8))
    cu = torch.tensor([0, 8], dtype=torch.int32)

    def no_library():
        raise AssertionError("the library was asked")
    for mod in (flash_attention, fak):
        with pytest.raises(RuntimeError, match="must be a CUDA tensor"):
            mod.forward_varlen(q, q, q, cu, 8, softcap=4.0)
        with pytest.raises(RuntimeError, match="must be a CUDA tensor"):
            mod.backward_varlen_softcap(q, q, q, q, lse, q, cu, 8, 4.0)
    with pytest.raises(RuntimeError, match="must be a CUDA tensor"):
        flash_attention.attention_varlen(q, q, q, cu, 8, softcap=4.0)
    monkeypatch.setattr(_capi, "load", no_library)
    for bad in BAD_SOFTCAPS:
        for mod in (flash_attention, fak):
            with pytest.raises(ValueError, match="softcap"):
                mod.forward_varlen(q, q, q, cu, 8, softcap=bad)
            with pytest.raises(ValueError, match="softcap"):
                mod.backward_varlen_softcap(q, q, q, q, lse, q, cu, 8, bad)
            with pytest.raises(ValueError, match="softcap"):
                mod.backward_varlen_softcap(None, None, None, None, None, None, None, None, bad)
        with pytest.raises(ValueError, match="softcap"):
            flash_attention.attention_varlen(q, q, q, cu, 8, softcap=bad)
    # the window's bad values still raise first, with their own text
    from tests.test_bwd_window_cpu import BAD_WINDOWS

    for window, causal, text in BAD_WINDOWS:
        with pytest.raises(ValueError, match=text):
            flash_attention.forward_varlen(q, q, q, cu, 8, causal=causal, window_size=window, softcap=-1.0)
        with pytest.raises(ValueError, match=text):
            flash_attention.backward_varlen_softcap(q, q, q, q, lse, q, cu, 8, -1.0, window, causal=causal)
        with pytest.raises(ValueError, match=text):
            flash_attention.attention_varlen(q, q, q, cu, 8, causal=causal, window_size=window, softcap=-1.0)


# ---- 3: the C ABI -----------------------------------------------------------------------------------------------------------------

def _w(left=-1, right=-1, **over):
    w = _capi.make_window(left, right)
    for name, value in over.items():
        setattr(w, name, value)
    return w


def _cap(softcap=4.0, **over):
    c = _capi.make_softcap(softcap)
    for name, value in over.items():
        setattr(c, name, value)
    return c


def _launch_fwd(window, cap, entry="softcap", args=None, kv=None, vq=None, key=None, opts=None, lse=16):
    """one launch of the soft-capped forward (or of its windowed sibling) on host-only arguments -> (status, message)"""
    lib = _capi.load()
    args, kv, vq, opts = args or _fwd(), kv or _kv(), vq or _vl(), opts or _capi.make_opts()
    key = key or _vl(T=5000, max_seqlen=4096)
    argv = [ctypes.byref(args), ctypes.byref(kv), ctypes.byref(vq), ctypes.byref(key), ctypes.byref(window) if window is not None else None]
    if entry == "softcap":
        argv.append(ctypes.byref(cap) if cap is not None else None)
    rc = getattr(lib, f"fa_fwd_launch_varlen_qk_{entry}")(*argv, ctypes.byref(opts), ctypes.c_void_p(lse) if lse is not None else None, None)
    return rc, _capi.last_error()


def _launch_bwd(window, cap, entry="softcap", **over):
    lib = _capi.load()
    a = _bwd(**over)
    argv = [ctypes.byref(a), ctypes.byref(window) if window is not None else None]
    if entry == "softcap":
        argv.append(ctypes.byref(cap) if cap is not None else None)
    rc = getattr(lib, f"fa_bwd_launch_varlen_qk_{entry}")(*argv, None, None)
    return rc, _capi.last_error()


def test_symbols_prototypes_and_abi_version():
    assert set(NEW_SYMBOLS) <= set(_capi.EXPORTED_SYMBOLS)
    for path in (_capi.LIB_PATH, JITTER):
        nm = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True)
        exported = set(re.findall(r" T (fa_[a-z_0-9]+)", nm.stdout))
        assert set(NEW_SYMBOLS) <= exported, (path, set(NEW_SYMBOLS) - exported)
    header = re.sub(r"\s+", " ", open(os.path.join(ROOT, "include", "fa_hip.h")).read())
    assert "typedef struct fa_softcap { uint32_t struct_size;" in header and "float softcap;" in header
    assert "int fa_fwd_varlen_qk_softcap_supported(const fa_fwd_config *cfg, const fa_fwd_opts *opts);" in header
    assert ("int fa_fwd_launch_varlen_qk_softcap(const fa_fwd_args *args, const fa_kv_layout *kv, const fa_varlen_layout *varlen_q, "
            "const fa_varlen_layout *varlen_k, const fa_window *window, const fa_softcap *softcap, const fa_fwd_opts *opts, float *lse, "
            "void *stream);") in header
    assert ("int fa_bwd_launch_varlen_qk_softcap(const fa_bwd_varlen_qk_args *args, const fa_window *window, const fa_softcap *softcap, "
            "void *stream, float *ms);") in header
    lib = _capi.load()
    assert lib.fa_abi_version() == 6 and _capi.FA_ABI_VERSION == 6   # additive: no struct grew
    assert ctypes.sizeof(_capi.FaSoftcap) == 8 and ctypes.sizeof(_capi.FaWindow) == 12
    want = list(lib.fa_fwd_launch_varlen_qk_window.argtypes)
    fn = lib.fa_fwd_launch_varlen_qk_softcap
    assert list(fn.argtypes) == want[:-3] + [ctypes.POINTER(_capi.FaSoftcap)] + want[-3:] and fn.restype == ctypes.c_int
    want = list(lib.fa_bwd_launch_varlen_qk_window.argtypes)
    fn = lib.fa_bwd_launch_varlen_qk_softcap
    assert list(fn.argtypes) == want[:2] + [ctypes.POINTER(_capi.FaSoftcap)] + want[2:] and fn.restype == ctypes.c_int
    supported = lib.fa_fwd_varlen_qk_softcap_supported
    cfg = _capi.make_config(fak.varlen_config(torch.bfloat16))
    for o in (None, _capi.make_opts(causal=True), _capi.make_opts(speculative=True)):
        op = ctypes.byref(o) if o is not None else None
        assert supported(ctypes.byref(cfg), op) == lib.fa_fwd_varlen_supported(ctypes.byref(cfg), op)
    assert supported(ctypes.byref(cfg), None) == 1 and supported(None, None) == 0


SOFTCAP_REFUSALS = [
    (None, -1, "fa_softcap is null"),
    (_cap(struct_size=4), -4, "fa_softcap.struct_size"),
    (_cap(struct_size=0), -4, "fa_softcap.struct_size"),
    (_cap(0.0), -4, "softcap"),
    (_cap(-0.0), -4, "softcap"),
    (_cap(-1.0), -4, "softcap"),
    (_cap(float("nan")), -4, "softcap"),
    (_cap(float("inf")), -4, "softcap"),
    (_cap(float("-inf")), -4, "softcap"),
]


@pytest.mark.parametrize("case", SOFTCAP_REFUSALS, ids=[str(i) for i in range(len(SOFTCAP_REFUSALS))])
def test_softcap_refusals_without_a_device(case):
    cap, status, text = case
    for window in (_w(), _w(100, 0), _w(63, 3)):   # ((-1, -1) is legal here and means no window)
        for rc, msg in (_launch_fwd(window, cap), _launch_bwd(window, cap)):
            assert rc == status and text in msg, (rc, msg)
    if cap is not None and cap.struct_size == 8:   # (this level has no "off": the message says whose job 0 is)
        assert "windowed entry point" in _launch_fwd(_w(), cap)[1] and "windowed entry point" in _launch_bwd(_w(), cap)[1]


def test_the_windows_refusals_arrive_before_the_caps():
    from tests.test_bwd_window_cpu import MAX_LEN, WINDOW_REFUSALS

    bad_cap = _cap(-1.0)
    for window, causal, status, text in WINDOW_REFUSALS:
        for cap in (bad_cap, None):
            rc, msg = _launch_fwd(window, cap, opts=_capi.make_opts(causal=bool(causal)))
            assert rc == status and text in msg, (rc, msg)
            rc, msg = _launch_bwd(window, cap, causal=causal)
            assert rc == status and text in msg, (rc, msg)
    for side in (dict(max_seqlen=MAX_LEN + 1), dict(max_seqlen_k=MAX_LEN + 1)):
        rc, msg = _launch_bwd(_w(100, 0), bad_cap, T=0, Tk=0, **side)
        assert rc == -4 and "too large for a window" in msg
    rc, msg = _launch_fwd(_w(100, 0), bad_cap, args=_fwd(T=0), vq=_vl(T=0, max_seqlen=MAX_LEN + 1))
    assert rc == -4 and "too large for a window" in msg
    rc, msg = _launch_fwd(_w(100, 0), bad_cap, args=_fwd(T=0), vq=_vl(T=0), key=_vl(T=0, max_seqlen=MAX_LEN + 1))
    assert rc == -4 and "too large for a window" in msg
    # ... and the cap's own before "nothing to do": both totals zero with a bad cap is still refused, with a good one FA_OK
    assert _launch_bwd(_w(), bad_cap, T=0, Tk=0)[0] == -4 and _launch_fwd(_w(), bad_cap, args=_fwd(T=0), vq=_vl(T=0))[0] == -4
    ms = ctypes.c_float(-1.0)
    lib = _capi.load()
    assert lib.fa_bwd_launch_varlen_qk_softcap(ctypes.byref(_bwd(T=0, Tk=0)), ctypes.byref(_w()), ctypes.byref(_cap()), None, ctypes.byref(ms)) == 0
    assert ms.value == 0.0
    assert _launch_fwd(_w(), _cap(), args=_fwd(T=0), vq=_vl(T=0))[0] == 0


def test_what_the_windowed_sibling_refuses_arrives_first_with_its_words():
    bad_w, bad_cap = _w(-5, -5), _cap(-1.0)
    vl = lambda **kw: _capi.make_varlen_layout(kw.pop("cu", 16), kw.pop("n_seqs", 3), kw.pop("T", 1000), kw.pop("max_seqlen", 512))   # noqa: E731
    cases = [(dict(lse=None), -1, "lse is null"), (dict(dk=None), -1, "null tensor pointer"), (dict(workspace=None), -1, "workspace is null"),
             (dict(dtype=7), -2, "fp16 and bf16"), (dict(d_head=64), -4, "d_head = 128"), (dict(Hkv=3), -4, "divide"),
             (dict(kv_seq_stride=2 * 128 + 4), -5, "multiples of 8"), (dict(workspace=20), -5, "workspace must be 16-byte"),
             (dict(varlen=vl(cu=18)), -5, "cu_seqlens must be 4-byte"), (dict(struct_size=8), -4, "fa_bwd_varlen_qk_args.struct_size"),
             (dict(k_over=dict(n_seqs=4)), -4, "n_seqs mismatch"), (dict(q_seq_stride=(1 << 23) + 8), -4, "too large")]
    new, sibling = "fa_bwd_launch_varlen_qk_softcap", "fa_bwd_launch_varlen_qk_window"
    for over, status, text in cases:
        for window, cap in ((bad_w, bad_cap), (None, None), (_w(), bad_cap)):
            rc, msg = _launch_bwd(window, cap, **over)
            assert rc == status and text in msg, (over, rc, msg)
            rc0, msg0 = _launch_bwd(window, None, entry="window", **over)
            assert rc0 == rc and msg0.replace(sibling, new) == msg.replace(sibling, new), (msg0, msg)
    lib = _capi.load()
    assert lib.fa_bwd_launch_varlen_qk_softcap(None, ctypes.byref(bad_w), ctypes.byref(bad_cap), None, None) == -1
    fwd_cases = [(dict(lse=None), -1, "lse is null"), (dict(args=_fwd(d_head=64)), -4, "d_head"), (dict(vq=_vl(cu=18)), -5, "cu_seqlens must be 4-byte")]
    new, sibling = "fa_fwd_launch_varlen_qk_softcap", "fa_fwd_launch_varlen_qk_window"
    for over, status, text in fwd_cases:
        rc, msg = _launch_fwd(bad_w, bad_cap, **over)
        assert rc == status and text in msg, (over, rc, msg)
        rc0, msg0 = _launch_fwd(bad_w, None, entry="window", **over)
        assert rc0 == rc and msg0.replace(sibling, new) == msg, (msg0, msg)


def test_the_backward_is_sized_by_the_two_range_workspace_query():
    """no workspace query of its own: the sibling's bytes are what the launch asks for (a workspace one 16-byte step short cannot be
    told from the host, so the claim checked here is the header's and the wrapper's: one query, fa_bwd_varlen_qk_workspace_bytes)"""
    header = open(os.path.join(ROOT, "include", "fa_hip.h")).read()
    assert "fa_bwd_varlen_qk_softcap_workspace_bytes" not in header
    assert not any("softcap_workspace" in s for s in _capi.EXPORTED_SYMBOLS)
    assert "fa_bwd_varlen_qk_workspace_bytes(args) sizes the backward" in re.sub(r"\s*\n \*\s*", " ", header)
    src = inspect.getsource(fak._backward_varlen)
    assert "fa_bwd_varlen_qk_workspace_bytes" in src and "fa_bwd_launch_varlen_qk_softcap" in src
    lib = _capi.load()
    a = _bwd(workspace=None)
    assert lib.fa_bwd_varlen_qk_workspace_bytes(ctypes.byref(a)) > 0
    rc, msg = _launch_bwd(_w(), _cap(), workspace=None)
    assert rc == -1 and "fa_bwd_varlen_qk_workspace_bytes" in msg


# ---- 4: the kept ISA --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dt", [15, 5])
def test_the_forward_slice_is_kept_with_two_kernels_mfma_no_scratch_no_vector_spill(dt):
    path = os.path.join(BUILD, f"varlen_softcap_dt{dt}", "fa_inst_varlen-hip-amdgcn-amd-amdhsa-gfx950.s")
    assert os.path.exists(path), "the build keeps the ISA of every slice under csrc/build (make -C flash_attention_from_scratch_amd/csrc)"
    text = open(path).read()
    names = set(re.findall(r"^\s+\.name:\s+(_Z\w+)$", text, re.M))
    want = {f"_ZN2fa28fa_fwd_kernel_varlen_softcapILi{dt}ELi1ELi4ELi64ELb1ELb1ELb{opt}ELb1ELb1ELb1ELi128ELi0ELi1EEEvNS_23KernelArgsVarlenSoftcapE"
            for opt in (0, 1)}   # (with and without the first-block skip)
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
    assert "v_exp_f32" in text and "v_rcp_f32" in text
    print(f"varlen_softcap dt{dt}: vgpr_count", re.findall(r"\.vgpr_count:\s+(\d+)", text), "sgpr_spill_count",
          re.findall(r"\.sgpr_spill_count:\s+(\d+)", text))


def test_the_backward_slice_is_kept_with_six_kernels_mfma_no_scratch_no_spills_no_atomics():
    path = os.path.join(BUILD, "bwd_varlen_softcap", "fa_bwd_varlen_softcap-hip-amdgcn-amd-amdhsa-gfx950.s")
    assert os.path.exists(path), "the build keeps the ISA of every slice under csrc/build (make -C flash_attention_from_scratch_amd/csrc)"
    text = open(path).read()
    names = set(re.findall(r"^\s+\.name:\s+(_Z\w+)$", text, re.M))
    want = {f"_ZN2fa32fa_bwd_dkdv_reduce_varlen_kernelINS_20BwdVarlenSoftcapArgsELi{dt}EEEvT_" for dt in (15, 5)}
    for kernel in ("25fa_bwd_dkdv_varlen_kernel", "23fa_bwd_dq_varlen_kernel"):   # (one per dtype: the window carries the causal mask)
        want |= {f"_ZN2fa{kernel}INS_20BwdVarlenSoftcapArgsELi{dt}ELb0EEEvT_" for dt in (15, 5)}
    assert names == want, names ^ want
    bodies = {}
    for name in want:
        m = re.search(rf"^{name}:[^\n]*\n(.*?)^\s+\.end_amdhsa_kernel", text, flags=re.M | re.S)
        assert m, name
        bodies[name] = m.group(1)
    for name, body in bodies.items():
        if "reduce" in name:
            continue
        mine, other = ("bf16", "_f16") if "Li15E" in name else ("_f16", "bf16")
        mfma = set(re.findall(r"\bv_mfma_\w+", body))
        assert mfma and all(mine in m for m in mfma) and not any(other in m for m in mfma), (name, mfma)
        assert "v_exp_f32" in body and "v_rcp_f32" in body, name
    assert "scratch_" not in text
    assert re.findall(r"\.amdhsa_private_segment_fixed_size (\d+)", text) == ["0"] * 6
    assert re.findall(r"\.private_segment_fixed_size:\s+(\d+)", text) == ["0"] * 6
    assert re.findall(r"; ScratchSize: (\d+)", text) == ["0"] * 6
    assert re.findall(r"\.vgpr_spill_count:\s+(\d+)", text) == ["0"] * 6
    assert "atomic" not in text   # a fixed order of sums
    print("bwd_varlen_softcap:", re.findall(r"\.vgpr_count:\s+(\d+)", text), re.findall(r"\.sgpr_spill_count:\s+(\d+)", text))


# ---- 5: the inputs discriminate ---------------------------------------------------------------------------------------------------

PROOF = [(heads, window, softcap, dtype) for heads in sc.HEADS for window in sc.WINDOWS for softcap in sc.CAPS for dtype in sc.DTYPES]


@pytest.mark.parametrize("case", PROOF, ids=str)
def test_the_inputs_reject_a_missing_cap_and_a_dropped_tanh_derivative(case):
    """For each case of the GPU matrix, on the sequences the proof leans on (softcap_inputs.PROOF_SEQS: the ones with enough keys
    per row): (a) the fp32 capped reference and (b) the 16-bit one make the rules' bounds; (c) the fp32 UNCAPPED result misses
    bi.compare on o and bi.grad_rule on dq and dk by a factor >= 4; (d) fp32 gradients of the straight-through cap (the forward
    capped, the factor 1 - tanh^2 dropped) miss bi.grad_rule on dq and dk by a factor >= 4.  The 16-bit reference itself passes."""
    heads, window, softcap, dtype = case
    inp = sc.inputs(heads, dtype)
    for i in sc.PROOF_SEQS:
        q, k, v, dout = sc.sequence(inp, i)
        r = sc.reference(heads, dtype, window, softcap, i)
        assert bi.compare(r["o16"], None, r["o32"], r["lse32"], r["o16"], dtype)["ok"]
        o_c, _, g_c = sc.capped_backward(q, k, v, dout, window, torch.float32, None)
        _, _, g_d = sc.capped_backward(q, k, v, dout, window, torch.float32, softcap, straight_through=True)
        res = bi.compare(o_c, None, r["o32"], r["lse32"], r["o16"], dtype)
        ratios = dict(o=res["err"] / res["bound"])
        for name, j in (("dq", 0), ("dk", 1)):
            ratios[f"{name} uncapped"] = bi.grad_rule(g_c[j], r["g32"][j], r["g16"][j])["ratio"]
            ratios[f"{name} straight-through"] = bi.grad_rule(g_d[j], r["g32"][j], r["g16"][j])["ratio"]
        print(f"{case} sequence {inp['pairs'][i]}: err / bound " + ", ".join(f"{n} {x:.1f}" for n, x in ratios.items()))
        assert min(ratios.values()) >= 4.0, (case, inp["pairs"][i], ratios)


def test_the_linear_cap_does_not_discriminate_and_is_used_as_an_accuracy_case_only():
    """softcap = 50 on the same inputs: the uncapped fp32 result PASSES the forward rule in bf16 -- so tests/test_softcap_gpu.py uses
    it only where the question is the tanh near 0"""
    heads, window, dtype = (4, 4), (-1, -1, True), torch.bfloat16
    q, k, v, dout = sc.sequence(sc.inputs(heads, dtype), 0)
    r = sc.reference(heads, dtype, window, sc.LINEAR_CAP, 0)
    o_c, _ = sc.capped_attention(q, k, v, window, torch.float32, None)
    res = bi.compare(o_c, None, r["o32"], r["lse32"], r["o16"], dtype)
    assert res["err"] / res["bound"] < 1.0
