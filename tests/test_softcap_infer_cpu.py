"""Logit soft-capping in KV-cache decode and cache prefill without a device: the Python surface
(forward_kvcache_softcap in the three modules, softcap= keyword only on forward_varlen_kvcache, forward_kvcache unchanged, the
validator's order), the ten exports (symbols, prototypes, every refusal before any HIP call and in its order, the windowed
sibling's first and in its words), the decode's split count and workspace (the windowed entry's: the capped decodes have no
workspace query of their own, as tests/test_softcap_cpu.py asks of every soft-capped entry), the ISA the build keeps for
the four new slices, and the proof that the inputs of tests/test_softcap_infer_gpu.py discriminate: on each case of its matrix an
fp32 result WITHOUT the cap, and for an fp8 cache an fp32 result that caps the raw undescaled score and applies k_descale behind
it, miss the project's rule on o by a factor of 2 at least."""
import ctypes
import inspect
import os
import re
import subprocess

import pytest
import torch

import beacon_inputs as bi
import flash_attention
import softcap_infer_inputs as si
import softcap_inputs as sc
from flash_attention_from_scratch_amd import _capi
from flash_attention_from_scratch_amd import flash_attention_kernels as fak
from tests.conftest import ROOT
from tests.test_decode_cpu import _args, _kernels
from tests.test_decode_fp8_cpu import _args as _args8
from tests.test_prefill_kvcache_cpu import _contig, _fwd, _kv, _paged, _vl
from tests.test_prefill_window_cpu import _scales
from tests.test_softcap_cpu import SOFTCAP_REFUSALS, _cap, _w

BUILD = os.path.join(ROOT, "flash_attention_from_scratch_amd", "csrc", "build")
JITTER = os.path.join(ROOT, "flash_attention_from_scratch_amd", "lib", "libfa_hip_jitter.so")
PREFILL_FORMS = ("varlen_kvcache", "varlen_kvcache_fp8")
DECODE_FORMS = ("fa_decode", "fa_decode_fp8")
NEW_SYMBOLS = tuple(f"fa_fwd_{what}{form}_softcap{tail}" for form in PREFILL_FORMS for what, tail in (("", "_supported"), ("launch_", "")))
NEW_SYMBOLS += tuple(f"{form}_softcap_{what}" for form in DECODE_FORMS for what in ("supported", "num_splits", "launch"))


# ---- 1: signatures ----------------------------------------------------------------------------------------------------------------

def _modules():
    import flash_attention_from_scratch_amd.flash_attention as inner
    return flash_attention, inner, fak


def test_python_surface():
    base = ["q", "k_cache", "v_cache", "cache_seqlens", "block_table", "causal", "return_lse", "max_seqlen_k", "num_splits", "timed",
            "k_descale", "v_descale", "window_size", "k", "v", "rotary_cos", "rotary_sin", "rotary_interleaved", "advance_seqlens"]
    for mod in _modules():
        plain = inspect.signature(mod.forward_kvcache)
        assert list(plain.parameters) == base and len(base) == 19, mod   # (unchanged: its 19 parameters)
        sig = inspect.signature(mod.forward_kvcache_softcap)
        assert list(sig.parameters) == base[:4] + ["softcap"] + base[4:], mod
        assert sig.parameters["softcap"].default is inspect.Parameter.empty
        assert all(p.kind is inspect.Parameter.POSITIONAL_OR_KEYWORD for p in sig.parameters.values())
        for name in base[4:]:   # (forward_kvcache's defaults)
            assert sig.parameters[name].default == plain.parameters[name].default, (mod, name)
        params = inspect.signature(mod.forward_varlen_kvcache).parameters
        assert list(params)[-2:] == ["window_size", "softcap"], mod
        assert params["softcap"].kind is inspect.Parameter.KEYWORD_ONLY and params["softcap"].default == 0.0
        assert params["window_size"].kind is inspect.Parameter.KEYWORD_ONLY and params["window_size"].default == (-1, -1)
    outer, inner, _ = _modules()
    assert outer.forward_kvcache_softcap is inner.forward_kvcache_softcap
    # one body: the capped call shares forward_kvcache's checks instead of copying them
    for fn in (fak.forward_kvcache, fak.forward_kvcache_softcap):
        src = inspect.getsource(fn)
        assert "_forward_kvcache(" in src and "_decode_args" not in src and "append_kvcache(" not in src


# ---- 2: the validator -------------------------------------------------------------------------------------------------------------

def test_bad_values_are_value_errors_before_any_tensor_is_looked_at_a_bad_window_first(monkeypatch):
    from tests.test_prefill_window_cpu import BAD_WINDOWS
    from tests.test_softcap_cpu import BAD_SOFTCAPS

    t = torch.zeros(1)
    q = torch.zeros((8, 4, 128), dtype=torch.bfloat16)
    for mod in (flash_attention, fak):   # (a good softcap gets as far as the tensors)
        with pytest.raises(RuntimeError):
            mod.forward_kvcache_softcap(q, q, q, q, 4.0)
        with pytest.raises(RuntimeError):
            mod.forward_varlen_kvcache(q, q, q, q, 8, q, softcap=4.0)

    def no_library():
        raise AssertionError("the library was asked")
    monkeypatch.setattr(_capi, "load", no_library)
    for mod in (flash_attention, fak):
        for bad in BAD_SOFTCAPS:
            with pytest.raises(ValueError, match="softcap"):
                mod.forward_kvcache_softcap(t, t, t, t, bad)
            with pytest.raises(ValueError, match="softcap"):
                mod.forward_kvcache_softcap(None, None, None, None, softcap=bad)
            with pytest.raises(ValueError, match="softcap"):
                mod.forward_varlen_kvcache(t, t, t, t, 8, t, softcap=bad)
            with pytest.raises(ValueError, match="softcap"):
                mod.forward_varlen_kvcache(None, None, None, None, None, None, softcap=bad)
        for window, causal, text in BAD_WINDOWS:   # the window's bad values raise first, with their own text
            with pytest.raises(ValueError, match=text):
                mod.forward_kvcache_softcap(t, t, t, t, -1.0, causal=causal, window_size=window)
            with pytest.raises(ValueError, match=text):
                mod.forward_varlen_kvcache(t, t, t, t, 8, t, causal=causal, window_size=window, softcap=-1.0)


# ---- 3: the C ABI -----------------------------------------------------------------------------------------------------------------

def test_symbols_prototypes_and_abi_version():
    assert len(NEW_SYMBOLS) == 10 and set(NEW_SYMBOLS) <= set(_capi.EXPORTED_SYMBOLS)
    for path in (_capi.LIB_PATH, JITTER):
        nm = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True)
        exported = set(re.findall(r" T (fa_[a-z_0-9]+)", nm.stdout))
        assert set(NEW_SYMBOLS) <= exported, (path, set(NEW_SYMBOLS) - exported)
    header = re.sub(r"\s+", " ", open(os.path.join(ROOT, "include", "fa_hip.h")).read())
    for name in NEW_SYMBOLS:
        assert re.search(rf"\b{name}\(", header), name
    assert ("int fa_fwd_launch_varlen_kvcache_softcap(const fa_fwd_args *args, const fa_kv_layout *kv, const fa_varlen_layout *varlen_q, "
            "const fa_kvcache_layout *cache, const fa_window *window, const fa_softcap *softcap, const fa_fwd_opts *opts, float *lse, "
            "void *stream);") in header
    assert ("int fa_decode_fp8_softcap_launch(const fa_decode_fp8_args *args, const fa_window *window, const fa_softcap *softcap, "
            "void *stream, float *ms);") in header
    assert "int fa_decode_softcap_num_splits(const fa_decode_args *args, const fa_window *window, const fa_softcap *softcap);" in header
    # no workspace query of their own: the windowed sibling's sizes the launch, and the header says so
    assert not any("softcap_workspace" in name for name in _capi.EXPORTED_SYMBOLS) and "softcap_workspace" not in header
    assert "fa_decode_window_workspace_bytes(args, window) / fa_decode_fp8_window_workspace_bytes(args, window) size the launch" in header.replace(" * ", " ")
    lib = _capi.load()
    assert lib.fa_abi_version() == 6 and _capi.FA_ABI_VERSION == 6   # additive: no struct grew, fa_softcap is reused
    assert ctypes.sizeof(_capi.FaSoftcap) == 8 and ctypes.sizeof(_capi.FaWindow) == 12
    cap_p = ctypes.POINTER(_capi.FaSoftcap)
    for form in PREFILL_FORMS:   # the windowed sibling's parameters with the fa_softcap behind the fa_window
        want, fn = list(getattr(lib, f"fa_fwd_launch_{form}_window").argtypes), getattr(lib, f"fa_fwd_launch_{form}_softcap")
        assert list(fn.argtypes) == want[:-3] + [cap_p] + want[-3:] and fn.restype == ctypes.c_int
        assert want[-4] == ctypes.POINTER(_capi.FaWindow)
        supported = getattr(lib, f"fa_fwd_{form}_softcap_supported")
        cfg = _capi.make_config(fak.varlen_config(torch.bfloat16))
        for o in (None, _capi.make_opts(causal=True), _capi.make_opts(speculative=True)):
            op = ctypes.byref(o) if o is not None else None
            assert supported(ctypes.byref(cfg), op) == lib.fa_fwd_varlen_supported(ctypes.byref(cfg), op)
        assert supported(ctypes.byref(cfg), None) == 1 and supported(None, None) == 0
    for form in DECODE_FORMS:
        for what in ("supported", "num_splits", "launch"):
            sibling, fn = getattr(lib, f"{form}_window_{what}"), getattr(lib, f"{form}_softcap_{what}")
            want = list(sibling.argtypes)
            assert list(fn.argtypes) == want[:2] + [cap_p] + want[2:] and fn.restype == sibling.restype, (form, what)


def _p(x):
    return ctypes.byref(x) if x is not None else None


def _launch_prefill(form, window, cap, capped=True, args=None, kv=None, vq=None, key=None, opts=None, lse=16):
    """one launch of the capped prefill `form` (or of its windowed sibling) on host-only arguments -> (status, message)"""
    lib = _capi.load()
    args, kv, vq, opts, key = args or _fwd(), kv or _kv(), vq or _vl(), opts or _capi.make_opts(), key or _contig()
    argv = [_p(args), _p(kv), _p(vq), _p(key)] + ([_p(_scales())] if form.endswith("fp8") else []) + [_p(window)]
    if capped:
        argv.append(_p(cap))
    fn = getattr(lib, f"fa_fwd_launch_{form}_{'softcap' if capped else 'window'}")
    rc = fn(*argv, _p(opts), ctypes.c_void_p(lse) if lse is not None else None, None)
    return rc, _capi.last_error()


def _decode_all(form, a, window, cap, capped=True):
    """the three entries of a capped decode form (or its windowed sibling's) on host-only arguments -> [(status, message)] for
    launch and num_splits, and supported as 0 / 1"""
    lib = _capi.load()
    tail = [_p(window)] + ([_p(cap)] if capped else [])
    kind = "softcap" if capped else "window"
    out = []
    for what, more in (("launch", [None, None]), ("num_splits", []), ("supported", [])):
        rc = getattr(lib, f"{form}_{kind}_{what}")(_p(a), *tail, *more)
        out.append((rc, _capi.last_error()))
    return out


@pytest.mark.parametrize("case", SOFTCAP_REFUSALS, ids=[str(i) for i in range(len(SOFTCAP_REFUSALS))])
def test_softcap_refusals_without_a_device(case):
    cap, status, text = case
    for window in (_w(), _w(100, 0), _w(63, 3)):   # ((-1, -1) is legal here and means no window)
        for form in PREFILL_FORMS:
            rc, msg = _launch_prefill(form, window, cap)
            assert rc == status and text in msg, (form, rc, msg)
            if cap is not None and cap.struct_size == 8:   # (this level has no "off": the message names the sibling)
                assert "windowed entry point" in msg
        for form, make in zip(DECODE_FORMS, (_args, _args8)):
            launch, splits, supported = _decode_all(form, make(), window, cap)
            assert launch[0] == splits[0] == status and supported[0] == 0, (form, launch, splits, supported)
            assert text in launch[1] and text in splits[1]


def test_the_windows_refusals_arrive_before_the_caps():
    from tests.test_prefill_window_cpu import MAX_LEN
    from tests.test_prefill_window_cpu import WINDOW_REFUSALS as PREFILL_WINDOW_REFUSALS
    from tests.test_window_cpu import WINDOW_REFUSALS as DECODE_WINDOW_REFUSALS

    bad_cap = _cap(-1.0)
    for window, causal, status, text in PREFILL_WINDOW_REFUSALS:
        for form in PREFILL_FORMS:
            for cap in (bad_cap, None):
                rc, msg = _launch_prefill(form, window, cap, opts=_capi.make_opts(causal=causal))
                assert rc == status and text in msg, (form, rc, msg)
    for form in PREFILL_FORMS:   # the size bound, and "nothing to do" behind the cap's own rules
        rc, msg = _launch_prefill(form, _w(100, 0), bad_cap, args=_fwd(T=0), vq=_vl(T=0, max_seqlen=MAX_LEN + 1))
        assert rc == -4 and "too large for a window" in msg
        assert _launch_prefill(form, _w(), bad_cap, args=_fwd(T=0), vq=_vl(T=0))[0] == -4
        assert _launch_prefill(form, _w(), _cap(), args=_fwd(T=0), vq=_vl(T=0))[0] == 0
    for kw, over, status, text in DECODE_WINDOW_REFUSALS:
        for form, make in zip(DECODE_FORMS, (_args, _args8)):
            for cap in (bad_cap, None):
                launch, splits, supported = _decode_all(form, make(**over), kw["window"], cap)
                assert launch[0] == splits[0] == status and supported[0] == 0, (form, launch)
                assert text in launch[1] and text in splits[1]


def test_what_the_windowed_sibling_refuses_arrives_first_with_its_words():
    from tests.test_window_cpu import BASE_REFUSALS

    bad_w, bad_cap = _w(-5, -5), _cap(-1.0)
    cases = [(dict(lse=None), -1, "lse is null"), (dict(args=_fwd(d_head=64)), -4, "d_head"), (dict(vq=_vl(cu=18)), -5, "cu_seqlens must be 4-byte"),
             (dict(key=_paged(page_size=96), kv=_kv(bs=96 * 256)), -3, "multiple of 64"), (dict(key=_contig(cache_seqlens=None)), -1, "cache_seqlens is null")]
    for form in PREFILL_FORMS:
        new, sibling = f"fa_fwd_launch_{form}_softcap", f"fa_fwd_launch_{form}_window"
        for over, status, text in cases:
            for window, cap in ((bad_w, bad_cap), (_w(), None)):
                rc, msg = _launch_prefill(form, window, cap, **over)
                assert rc == status and text in msg, (form, over, rc, msg)
                rc0, msg0 = _launch_prefill(form, window, None, capped=False, **over)
                assert rc0 == rc and msg0.replace(sibling, new) == msg, (msg0, msg)
    lib = _capi.load()
    for form, make in zip(DECODE_FORMS, (_args, _args8)):
        new, sibling = f"{form}_softcap_", f"{form}_window_"
        for over, status, text in BASE_REFUSALS:
            for window, cap in ((_w(2000, 0), bad_cap), (_w(2000, 0), None)):   # (more than one split, so the workspace is asked for)
                got = _decode_all(form, make(**over), window, cap)[0]
                want = _decode_all(form, make(**over), window, None, capped=False)[0]
                assert got[0] == want[0] == status and text in got[1], (form, over, got, want)
                # the sibling's words -- its workspace query included, which sizes the capped launch too -- but for the entry's own name
                assert want[1] == got[1] or want[1].replace(sibling + "launch", new + "launch") == got[1], (want, got)
        assert getattr(lib, f"{form}_softcap_launch")(None, _p(bad_w), _p(bad_cap), None, None) == -1
        # an empty batch is "nothing to do" only behind the cap's own rules
        ms = ctypes.c_float(-1.0)
        assert getattr(lib, f"{form}_softcap_launch")(_p(make(batch=0, workspace=None)), _p(_w()), _p(bad_cap), None, _p(ms)) == -4
        assert getattr(lib, f"{form}_softcap_launch")(_p(make(batch=0, workspace=None)), _p(_w()), _p(_cap()), None, _p(ms)) == 0
        assert ms.value == 0.0
    # fp8: the descales' rules are the sibling's too
    rc = lib.fa_decode_fp8_softcap_launch(_p(_args8(k_descale=6)), _p(_w(100, 0)), _p(bad_cap), None, None)
    assert rc == -5 and "k_descale and v_descale" in _capi.last_error()
    rc = lib.fa_decode_fp8_softcap_launch(_p(_args8(kv_dtype=2)), _p(_w(100, 0)), _p(bad_cap), None, None)
    assert rc == -2 and "kv_dtype" in _capi.last_error()


# ---- 4: the decode's split count and workspace ---------------------------------------------------------------------------------------

def test_the_split_count_and_the_workspace_are_the_windowed_entrys():
    from tests.test_window_cpu import WIDE, WINDOW_SPLITS

    lib = _capi.load()
    windows = [w for _, w, _ in WINDOW_SPLITS] + WIDE
    shapes = [s for s, _, _ in WINDOW_SPLITS]
    checked = 0
    for batch, Sq, H, Hkv, cap_len, max_k, forced, causal in shapes:
        for window in windows:
            if causal and window[1] not in (-1, 0):
                continue
            for paged in (False, True):
                kw = dict(batch=batch, Sq=Sq, H=H, Hkv=Hkv, max_seqlen_k=max_k, num_splits=forced, causal=causal)
                if paged:
                    kw["paged"] = (batch * (cap_len // 64) + 1, 64, cap_len // 64)
                else:
                    kw["cache"] = cap_len
                for form, make in zip(DECODE_FORMS, (_args, _args8)):
                    a, w = make(**kw), _w(*window)
                    want = getattr(lib, f"{form}_window_num_splits")(_p(a), _p(w))
                    want_ws = getattr(lib, f"{form}_window_workspace_bytes")(_p(a), _p(w))
                    # the launch asks for the windowed entry's bytes, by that query's name, when the rule splits
                    if want_ws > 0:
                        rc = getattr(lib, f"{form}_softcap_launch")(_p(make(workspace=None, **kw)), _p(w), _p(_cap(50.0)), None, None)
                        assert rc == -1 and f"{form}_window_workspace_bytes(args, window)" in _capi.last_error(), (kw, window)
                    assert want >= 1
                    for softcap in (0.5, 50.0, 1e30):   # the cap does not enter the rule
                        c = _cap(softcap)
                        assert getattr(lib, f"{form}_softcap_num_splits")(_p(a), _p(w), _p(c)) == want
                        assert getattr(lib, f"{form}_softcap_supported")(_p(a), _p(w), _p(c)) == 1
                    checked += 1
    assert checked > 500


# ---- 5: the kept ISA --------------------------------------------------------------------------------------------------------------

PREFILL_SLICES = [("varlen_kvcache_softcap", "fa_inst_varlen", "36fa_fwd_kernel_varlen_kvcache_softcap", "23KernelArgsVarlenKVCacheE", 1),
                  ("varlen_kvcache_fp8_softcap", "fa_inst_varlen", "40fa_fwd_kernel_varlen_kvcache_fp8_softcap",
                   "26KernelArgsVarlenKVCacheFp8E", 0)]


def _no_scratch_no_spill_no_atomics(text, n, stats_counter=False):
    """stats_counter: the forward text's optional diagnostic counter (fa_fwd_opts.stats, never set by the varlen launches) is the one
    atomic there, an integer add per kernel as in the windowed sibling: no sum of the result goes through an atomic"""
    assert "scratch_" not in text
    assert re.findall(r"\.amdhsa_private_segment_fixed_size (\d+)", text) == ["0"] * n
    assert re.findall(r"\.private_segment_fixed_size:\s+(\d+)", text) == ["0"] * n
    assert re.findall(r"; ScratchSize: (\d+)", text) == ["0"] * n
    assert re.findall(r"\.vgpr_spill_count:\s+(\d+)", text) == ["0"] * n
    atomics = re.findall(r"^\s+(\w*atomic\w*)", text, re.M)
    assert atomics == (["global_atomic_add"] * n if stats_counter else []), atomics


@pytest.mark.parametrize("dt", [15, 5])
@pytest.mark.parametrize("folder,unit,kernel,args,dma", PREFILL_SLICES, ids=["16bit", "fp8"])
def test_the_prefill_slices_are_kept_with_two_kernels_mfma_no_scratch_no_vector_spill(folder, unit, kernel, args, dma, dt):
    path = os.path.join(BUILD, f"{folder}_dt{dt}", f"{unit}-hip-amdgcn-amd-amdhsa-gfx950.s")
    assert os.path.exists(path), "the build keeps the ISA of every slice under csrc/build (make -C flash_attention_from_scratch_amd/csrc)"
    text = open(path).read()
    names = set(re.findall(r"^\s+\.name:\s+(_Z\w+)$", text, re.M))
    want = {f"_ZN2fa{kernel}ILi{dt}ELi1ELi4ELi64ELb1ELb1ELb{opt}ELb1ELb{dma}ELb1ELi128ELi0ELi1EEEvNS_10SoftcappedINS_8WindowedINS_{args}EEEE"
            for opt in (0, 1)}   # (with and without the first-block skip)
    assert names == want, names ^ want
    for name in want:
        assert re.search(rf"^{name}:", text, flags=re.M), name
    mine, other = ("bf16", "_f16") if dt == 15 else ("_f16", "bf16")
    mfma = set(re.findall(r"\bv_mfma_\w+", text))
    assert mfma and all(mine in m for m in mfma) and not any(other in m for m in mfma), mfma
    _no_scratch_no_spill_no_atomics(text, 2, stats_counter=True)
    sibling = open(os.path.join(BUILD, f"{folder.replace('softcap', 'window')}_dt{dt}", f"{unit.replace('softcap', 'window')}-hip-amdgcn-amd-amdhsa-gfx950.s")).read()
    assert len(re.findall(r"atomic", sibling)) == len(re.findall(r"atomic", text)) == 2
    assert "v_exp_f32" in text and "v_rcp_f32" in text
    print(f"{folder} dt{dt}: vgpr_count", re.findall(r"\.vgpr_count:\s+(\d+)", text), "sgpr_count", re.findall(r"\.sgpr_count:\s+(\d+)", text),
          "sgpr_spill_count", re.findall(r"\.sgpr_spill_count:\s+(\d+)", text))


DECODE_SLICES = [("decode_softcap", "fa_decode_softcap", "17DecodeSoftcapArgs", 16), ("decode_fp8_softcap", "fa_decode_fp8_softcap", "20DecodeFp8SoftcapArgs", 8)]


@pytest.mark.parametrize("folder,unit,args,loads", DECODE_SLICES, ids=["16bit", "fp8"])
def test_the_decode_units_are_kept_with_twelve_split_kernels_mfma_no_scratch_no_vector_spill(folder, unit, args, loads):
    path = os.path.join(BUILD, folder, f"{unit}-hip-amdgcn-amd-amdhsa-gfx950.s")
    assert os.path.exists(path), "the build keeps the ISA of every slice under csrc/build (make -C flash_attention_from_scratch_amd/csrc)"
    text = open(path).read()
    names = set(re.findall(r"^\s+\.name:\s+(_Z\w+)$", text, re.M))
    want = {f"_ZN2fa22fa_decode_split_kernelINS_{args}ELi{dt}ELi{nt}ELb{p}EEEvT_" for dt in (15, 5) for nt in (1, 2, 4) for p in (0, 1)}
    assert len(want) == 12
    want |= {f"_ZN2fa24fa_decode_combine_kernelILi{dt}EEEvNS_10DecodeArgsE" for dt in (15, 5)}
    assert names == want, names ^ want
    _no_scratch_no_spill_no_atomics(text, 14)
    for name, body in _kernels(text).items():
        if "split_kernel" not in name:
            continue
        mine, other = ("_bf16", "_f16") if f"{args}ELi15E" in name else ("_f16", "_bf16")
        mfma = set(re.findall(r"\bv_mfma_\w+", body))
        assert mfma == {f"v_mfma_f32_16x16x32{mine}"}, (name, mfma)
        assert "v_exp_f32" in body and "v_rcp_f32" in body, name
    table = re.findall(r"\.name:\s+(_ZN2fa22fa_decode_split\w+)\n(?:.*\n)*?\s+\.sgpr_count:\s+(\d+)\n(?:.*\n)*?\s+\.vgpr_count:\s+(\d+)", text)
    print(f"{folder}: (kernel, sgpr, vgpr)", [(n[len('_ZN2fa22fa_decode_split_kernelINS_'):], s, v) for n, s, v in table])


@pytest.mark.parametrize("folder,unit,args,loads", DECODE_SLICES, ids=["16bit", "fp8"])
def test_the_capped_prefetch_stays_in_flight(folder, unit, args, loads):
    """tests/test_window_cpu.py's property (test_window_prefetch_stays_in_flight), kept under the cap: in each half of the unrolled
    loop, between the prefetch's last load and the first transposed LDS read of the P V products, no wait goes below the next
    unit's loads (16, fp8: 8).  The 16- and 32-row forms, as there."""
    kernels = _kernels(open(os.path.join(BUILD, folder, f"{unit}-hip-amdgcn-amd-amdhsa-gfx950.s")).read())
    checked = 0
    for name, body in kernels.items():
        if "split_kernel" not in name or "ELi4ELb" in name:
            continue
        halves = 0
        for block in re.split(r"^\.LBB\d+_\d+:", body, flags=re.M):
            ops = re.findall(r"^\s+(global_load_dwordx4|ds_read_b64_tr_b16|s_waitcnt[^\n]*vmcnt\((\d+)\))", block, re.M)
            kinds = [o[0].split()[0] for o in ops]
            if kinds.count("global_load_dwordx4") < loads or "ds_read_b64_tr_b16" not in kinds:
                continue
            last_load = max(i for i, k in enumerate(kinds) if k == "global_load_dwordx4")
            first_read = kinds.index("ds_read_b64_tr_b16")
            if first_read < last_load:
                continue
            waits = [int(o[1]) for o in ops[last_load:first_read] if o[1]]
            assert waits and min(waits) >= loads, (name, waits)
            halves += 1
        assert halves == 2, (name, halves)
        checked += 1
    assert checked == 8


# ---- 6: the inputs discriminate ---------------------------------------------------------------------------------------------------

def _ratio(o_wrong, r, dtype):
    res = bi.compare(o_wrong, None, r["o32"], r["lse32"], r["o16"], dtype)
    return res["err"] / res["bound"]


def _proof(kind, inp, refs, cache, window, softcap, dtype):
    """the two wrong restatements against the rule on o, per entry with enough keys -> {entry: {name: err / bound}}"""
    out = {}
    for b, n in enumerate(inp["lens"]):
        q, k, v = si.entry(inp, b, cache)
        if n < si.PROOF_MIN_KEYS or q.shape[0] == 0:
            continue
        r = refs[b]
        assert bi.compare(r["o16"], None, r["o32"], r["lse32"], r["o16"], dtype)["ok"]   # (the 16-bit reference itself passes)
        ratios = dict(uncapped=_ratio(sc.capped_attention(q, k, v, window, torch.float32, None)[0], r, dtype))
        if cache is not None:
            ratios["raw cap"] = _ratio(si.raw_cap_then_descale(q, cache["k8"][b, :n], v, cache["kd"][b], window, softcap), r, dtype)
        out[(kind, b, n)] = ratios
    return out


PROOF = [(window, softcap, dtype, fp8) for window in si.WINDOWS for softcap in si.CAPS for dtype in si.DTYPES for fp8 in (False, True)]


@pytest.mark.parametrize("case", PROOF, ids=str)
def test_the_inputs_reject_a_missing_cap_and_a_cap_of_the_raw_fp8_score(case):
    """For each discriminating case of the GPU matrix and each entry with at least 31 keys: (a) the fp32 UNCAPPED result and (b), fp8,
    an fp32 result that caps the raw undescaled score and applies k_descale behind it, miss bi.compare on o by a factor >= 2.
    Lengths 0 and 1 never discriminate (one softmax whatever the logit): excluded here, not from the GPU tests."""
    window, softcap, dtype, fp8 = case
    found = {}
    shapes = [(Sq, si.HEADS) for Sq in si.DECODE_SEQLENS_Q] + [(8, si.HEADS_64)]
    for Sq, heads in shapes:
        inp = si.decode_inputs(dtype, Sq, heads)
        cache = si.fp8_cache("decode", dtype, Sq, heads) if fp8 else None
        found.update(_proof(f"decode Sq={Sq} heads={heads}", inp, si.decode_reference(dtype, Sq, window, softcap, fp8, heads), cache, window,
                            softcap, dtype))
    inp = si.prefill_inputs(dtype)
    cache = si.fp8_cache("prefill", dtype) if fp8 else None
    found.update(_proof("prefill", inp, si.prefill_reference(dtype, window, softcap, fp8), cache, window, softcap, dtype))
    assert len(found) == 4 * 5 + 4
    worst = {}
    for key, ratios in found.items():
        for name, x in ratios.items():
            if x < worst.get(name, (float("inf"),))[0]:
                worst[name] = (x, key)
    print(f"{case}: worst err / bound " + ", ".join(f"{name} {x:.1f} at {key}" for name, (x, key) in worst.items()))
    for key, ratios in found.items():
        assert min(ratios.values()) >= 2.0, (case, key, ratios)


def test_the_linear_cap_does_not_discriminate_and_is_used_as_an_accuracy_case_only():
    dtype, window = torch.bfloat16, (-1, -1, True)
    inp = si.decode_inputs(dtype, 4)
    refs = si.decode_reference(dtype, 4, window, si.LINEAR_CAP)
    b = inp["lens"].index(1000)
    q, k, v = si.entry(inp, b)
    assert _ratio(sc.capped_attention(q, k, v, window, torch.float32, None)[0], refs[b], dtype) < 1.0
