"""Sliding-window attention in the varlen backward and the autograd path without a device: the export
fa_bwd_launch_varlen_qk_window (symbol, prototype, validation before any HIP call, the sibling's refusals first), the Python
surface (backward_varlen_window in the three modules, attention_varlen's keyword-only window_size), the ISA the build keeps for
the windowed slice, the bench tool's host tile counts against a brute-force count, and the inputs of
tests/test_bwd_window_gpu.py against masks that are off by one at either edge of the window."""
import ctypes
import importlib.util
import inspect
import os
import re
import subprocess

import pytest
import torch

import beacon_inputs as bi
import flash_attention
import window_backward_inputs as wb
from flash_attention_from_scratch_amd import _capi
from flash_attention_from_scratch_amd import flash_attention_kernels as fak
from tests.conftest import ROOT
from tests.test_varlen_qk_cpu import _bwd

BUILD = os.path.join(ROOT, "flash_attention_from_scratch_amd", "csrc", "build")
JITTER = os.path.join(ROOT, "flash_attention_from_scratch_amd", "lib", "libfa_hip_jitter.so")
NEW = "fa_bwd_launch_varlen_qk_window"
MAX_LEN = (1 << 30) - 128


def _w(left=-1, right=-1, **over):
    w = _capi.make_window(left, right)
    for name, value in over.items():
        setattr(w, name, value)
    return w


def _launch(window, windowed=True, **over):
    """one launch of the windowed entry (or of its sibling) on host-only arguments -> (status, message)"""
    lib = _capi.load()
    a = _bwd(**over)
    if windowed:
        rc = lib.fa_bwd_launch_varlen_qk_window(ctypes.byref(a), ctypes.byref(window) if window is not None else None, None, None)
    else:
        rc = lib.fa_bwd_launch_varlen_qk(ctypes.byref(a), None, None)
    return rc, _capi.last_error()


# ---- export and prototype ---------------------------------------------------------------------------------------------------------

def test_symbol_prototype_and_abi_version():
    assert NEW in _capi.EXPORTED_SYMBOLS
    for path in (_capi.LIB_PATH, JITTER):
        nm = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True)
        assert NEW in set(re.findall(r" T (fa_[a-z_0-9]+)", nm.stdout)), path
    header = open(os.path.join(ROOT, "include", "fa_hip.h")).read()
    assert re.search(rf"\bint {NEW}\(const fa_bwd_varlen_qk_args \*args, const fa_window \*window, void \*stream, float \*ms\);", header)
    lib = _capi.load()
    assert lib.fa_abi_version() == 6 and _capi.FA_ABI_VERSION == 6   # additive: no struct grew, fa_window is reused
    assert ctypes.sizeof(_capi.FaWindow) == 12
    fn, sibling = lib.fa_bwd_launch_varlen_qk_window, lib.fa_bwd_launch_varlen_qk
    want = list(sibling.argtypes)
    assert list(fn.argtypes) == want[:1] + [ctypes.POINTER(_capi.FaWindow)] + want[1:] and fn.restype == ctypes.c_int


# ---- refusals ---------------------------------------------------------------------------------------------------------------------

WINDOW_REFUSALS = [
    (None, 0, -1, "fa_window is null"),
    (_w(struct_size=8), 0, -4, "fa_window.struct_size"),
    (_w(struct_size=0), 0, -4, "fa_window.struct_size"),
    (_w(-2, 0), 0, -4, "left and right must be -1"),
    (_w(0, -2), 0, -4, "left and right must be -1"),
    (_w(10, 1), 1, -4, "causal means right = 0"),
    (_w(-1, 5), 1, -4, "causal means right = 0"),
]


@pytest.mark.parametrize("case", WINDOW_REFUSALS, ids=[str(i) for i in range(len(WINDOW_REFUSALS))])
def test_window_refusals_without_a_device(case):
    window, causal, status, text = case
    rc, msg = _launch(window, causal=causal)
    assert rc == status and text in msg, (rc, msg)


def test_the_size_bound_at_2_30_minus_128_and_one_above():
    """max_seqlen of either side: at the bound the call passes (both totals zero: it returns before a device is asked), one above
    it is refused; the sibling has no such bound"""
    w = _w(100, 0)
    for n, status, text in ((MAX_LEN, 0, ""), (MAX_LEN + 1, -4, "too large for a window")):
        for side in (dict(max_seqlen=n), dict(max_seqlen_k=n)):
            rc, msg = _launch(w, T=0, Tk=0, **side)
            assert rc == status and text in msg, (n, side, rc, msg)
            assert _launch(None, windowed=False, T=0, Tk=0, **side)[0] == 0
    # (the bound is the last of the window's rules: a bad window is refused first)
    rc, msg = _launch(_w(-2, 0), T=0, Tk=0, max_seqlen=MAX_LEN + 1)
    assert rc == -4 and "left and right must be -1" in msg


def test_what_the_unwindowed_entry_refuses_arrives_first():
    """the sibling's refusals, each with a window that is itself refused: the sibling's status and words win"""
    bad = _w(-5, -5)
    vl = lambda **kw: _capi.make_varlen_layout(kw.pop("cu", 16), kw.pop("n_seqs", 3), kw.pop("T", 1000), kw.pop("max_seqlen", 512))   # noqa: E731
    cases = [(dict(lse=None), -1, "lse is null"), (dict(dk=None), -1, "null tensor pointer"), (dict(workspace=None), -1, "workspace is null"),
             (dict(dtype=7), -2, "fp16 and bf16"), (dict(d_head=64), -4, "d_head = 128"), (dict(Hkv=3), -4, "divide"),
             (dict(kv_seq_stride=2 * 128 + 4), -5, "multiples of 8"), (dict(workspace=20), -5, "workspace must be 16-byte"),
             (dict(varlen=vl(cu=18)), -5, "cu_seqlens must be 4-byte"), (dict(struct_size=8), -4, "fa_bwd_varlen_qk_args.struct_size"),
             (dict(k_over=dict(n_seqs=4)), -4, "n_seqs mismatch"), (dict(q_seq_stride=(1 << 23) + 8), -4, "too large")]
    for over, status, text in cases:
        for window in (bad, None):
            rc, msg = _launch(window, **over)
            assert rc == status and text in msg, (over, rc, msg)
            rc0, msg0 = _launch(None, windowed=False, **over)   # (the sibling's words, but for the entry's own name in them)
            assert rc0 == rc and msg0.replace("fa_bwd_launch_varlen_qk", NEW) == msg.replace("fa_bwd_launch_varlen_qk_window", NEW)
    lib = _capi.load()
    assert lib.fa_bwd_launch_varlen_qk_window(None, ctypes.byref(bad), None, None) == -1
    rc, msg = _launch(bad)
    assert rc == -4 and "left and right must be -1" in msg


def test_both_totals_zero_return_ok_without_a_device():
    lib = _capi.load()
    for window, causal in ((_w(), 0), (_w(0, 0), 1), (_w(5, -1), 1), (_w(2 ** 31 - 1, 2 ** 31 - 1), 0)):
        ms = ctypes.c_float(-1.0)
        rc = lib.fa_bwd_launch_varlen_qk_window(ctypes.byref(_bwd(T=0, Tk=0, causal=causal)), ctypes.byref(window), None, ctypes.byref(ms))
        assert rc == 0 and ms.value == 0.0, _capi.last_error()


# ---- the Python surface -----------------------------------------------------------------------------------------------------------

def test_python_surface():
    import flash_attention_from_scratch_amd.flash_attention as inner

    want = ["q", "k", "v", "o", "lse", "dout", "cu_seqlens", "max_seqlen", "window_size", "causal", "timed", "cu_seqlens_k", "max_seqlen_k"]
    for mod in (flash_attention, inner, fak):
        sig = inspect.signature(mod.backward_varlen_window)
        assert list(sig.parameters) == want, mod
        assert [sig.parameters[n].default for n in want[9:]] == [False, False, None, None]
        assert sig.parameters["window_size"].default is inspect.Parameter.empty
    assert flash_attention.backward_varlen_window is inner.backward_varlen_window
    for fn in (flash_attention.attention_varlen, inner.attention_varlen):
        p = inspect.signature(fn).parameters["window_size"]
        assert p.kind is inspect.Parameter.KEYWORD_ONLY and p.default == (-1, -1)
    for fn in (flash_attention.backward_varlen, fak.backward_varlen):   # (the unwindowed backward keeps its signature)
        assert "window_size" not in inspect.signature(fn).parameters


# the ten bad window_size values of tests/test_prefill_window_cpu.py
BAD_WINDOWS = [((1,), False, "pair of Python ints"), ("ab", False, "pair of Python ints"), ((1.0, 0), False, "pair of Python ints"),
               ((True, 0), False, "pair of Python ints"), ((-2, 0), False, "must be -1"), ((0, -2), False, "must be -1"),
               ((2 ** 31, 0), False, "32-bit"), ((4, 5), True, "causal means right = 0"), (5, False, "pair of Python ints"),
               ((torch.tensor(3), 0), False, "pair of Python ints")]


def test_bad_window_sizes_are_value_errors_before_any_tensor_is_looked_at():
    from tests.test_prefill_window_cpu import BAD_WINDOWS as theirs

    assert len(BAD_WINDOWS) == 10 and [(repr(w), c, t) for w, c, t in BAD_WINDOWS] == [(repr(w), c, t) for w, c, t in theirs]
    for window, causal, text in BAD_WINDOWS:
        for fn in (flash_attention.backward_varlen_window, fak.backward_varlen_window):
            with pytest.raises(ValueError, match=text):
                fn(None, None, None, None, None, None, None, None, window, causal=causal)
        with pytest.raises(ValueError, match=text):
            flash_attention.attention_varlen(None, None, None, None, None, causal=causal, window_size=window)
    # (a good window gets as far as the tensors)
    with pytest.raises(AttributeError):
        fak.backward_varlen_window(None, None, None, None, None, None, None, None, (16, 0))


# ---- the kept ISA -----------------------------------------------------------------------------------------------------------------

def test_the_windowed_slice_is_kept_with_its_six_kernels_mfma_no_scratch_no_spills_no_atomics():
    path = os.path.join(BUILD, "bwd_varlen_window", "fa_bwd_varlen_window-hip-amdgcn-amd-amdhsa-gfx950.s")
    assert os.path.exists(path), "the build keeps the ISA of every slice under csrc/build (make -C flash_attention_from_scratch_amd/csrc)"
    text = open(path).read()
    names = set(re.findall(r"^\s+\.name:\s+(_Z\w+)$", text, re.M))
    want = {f"_ZN2fa32fa_bwd_dkdv_reduce_varlen_kernelINS_19BwdVarlenWindowArgsELi{dt}EEEvT_" for dt in (15, 5)}
    for kernel in ("25fa_bwd_dkdv_varlen_kernel", "23fa_bwd_dq_varlen_kernel"):   # (one per dtype: the window carries the causal mask)
        want |= {f"_ZN2fa{kernel}INS_19BwdVarlenWindowArgsELi{dt}ELb0EEEvT_" for dt in (15, 5)}
    assert names == want, names ^ want
    for name in want:
        assert re.search(rf"^{name}:", text, flags=re.M), name
    assert "v_mfma_f32_32x32x16_bf16" in text and "v_mfma_f32_32x32x16_f16" in text and "ds_read_b64_tr_b16" in text
    assert "scratch_" not in text
    assert re.findall(r"\.private_segment_fixed_size:\s+(\d+)", text) == ["0"] * 6
    assert re.findall(r"; ScratchSize: (\d+)", text) == ["0"] * 6
    assert re.findall(r"\.vgpr_spill_count:\s+(\d+)", text) == ["0"] * 6
    assert re.findall(r"\.sgpr_spill_count:\s+(\d+)", text) == ["0"] * 6
    assert "atomic" not in text   # a fixed order of sums
    print("bwd_varlen_window:", re.findall(r"\.vgpr_count:\s+(\d+)", text), re.findall(r"\.sgpr_count:\s+(\d+)", text))


# ---- the tile ranges --------------------------------------------------------------------------------------------------------------

def _bench():
    path = os.path.join(ROOT, "flash_attention_from_scratch_amd", "tools", "bwd_window_bench.py")
    spec = importlib.util.spec_from_file_location("bwd_window_bench", path)
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    return bench


def test_the_bench_counts_tiles_of_both_kernels_as_the_rule_does():
    bench = _bench()
    pairs = wb.PAIRS + [(165, 197), (37, 1000), (128, 192), (129, 65), (512, 512), (1000, 300)]
    windows = [bi.window_sides(*w) for w in wb.WINDOWS] + [(31, 0), (127, 0), (128, 0), (1000, 0), (-1, -1), (-1, 0), (0, 300), (0, 1000)]
    empties = 0
    for n_q, n_k in pairs:
        for left, right in windows:
            brute = wb.visited_tiles_brute(n_q, n_k, left, right)
            assert bench.visited_tiles(n_q, n_k, left, right) == brute, (n_q, n_k, left, right)
            empties += brute[0] == 0 or brute[1] == 0
    assert empties > len(windows)   # ((0, 50), (50, 0) and more: ranges that visit nothing are among them)
    # whole blocks that visit nothing inside a sequence that is not empty: rows dead from below, keys above every ceiling
    assert wb.visited_tiles_brute(700, 130, 0, 0) == (4, 4) and bench.visited_tiles(700, 130, -1, -1) == (6 * 3, 2 * 11)
    assert bench.visited_tiles(4096, 4096, -1, 0) == (sum(2 * b + 2 for b in range(32)),) * 2


# ---- the inputs prove something ---------------------------------------------------------------------------------------------------

PROOF = [(n_q, n_k, w, torch.bfloat16) for n_q, n_k, w in wb.PROOF_CASES] + \
        [(257, 513, (0, 0), torch.float16), (130, 700, (64, 0), torch.float16), (700, 130, (3, 2), torch.bfloat16),
         (300, 300, (-1, 5), torch.float16), (65, 63, (5, -1), torch.bfloat16), (257, 513, (0, 64), torch.bfloat16)]


@pytest.mark.parametrize("case", PROOF, ids=str)
def test_the_inputs_reject_a_mask_off_by_one_at_either_edge(case):
    """On the GPU test's own sequences, fp32 eager autograd with the lower or the upper edge of the window moved by one must be
    rejected by the gradient rule for at least one of dq, dk, dv; the conditions the construction promises are asserted first."""
    n_q, n_k, (left, right), dtype = case
    n_q, n_k = bi.cpu_cap(n_q), bi.cpu_cap(n_k)
    seq = wb.sequence(n_q, n_k, (4, 2), dtype, left, right, seed=3)
    o32, lse32, dout = wb.forward_and_dout(seq, seed=11)
    p, several = bi.target_probabilities(seq, lse32)
    ds, _ = bi.target_ds(seq, dout, o32, lse32)
    assert bool(several.any()) or (left, right) == (0, 0)   # ((0, 0): every row sees one key, p = 1 and dS = 0 by construction)
    if bool(several.any()):
        assert bi.P_LO <= p[several].min().item() and p[several].max().item() <= bi.P_HI, (p[several].min().item(), p[several].max().item())
        assert ds[several].abs().min().item() >= bi.DS_FLOOR, ds[several].abs().min().item()
    g32, g16 = wb.eager_backward(seq, dout, torch.float32), wb.eager_backward(seq, dout, dtype)
    for g, r32, r16 in zip(g16, g32, g16):
        assert bi.grad_rule(g, r32, r16)["ok"]
    muts = wb.mutants(seq, left, right)
    assert muts
    for delta, delta_lo, extra in muts:
        gm = wb.eager_backward(seq, dout, torch.float32, delta=delta, delta_lo=delta_lo, extra=extra)
        ratios = [bi.grad_rule(g, r32, r16)["ratio"] for g, r32, r16 in zip(gm, g32, g16)]
        print(f"{case} mutant hi{delta:+d} lo{delta_lo:+d}: err / bound dq {ratios[0]:.1f} dk {ratios[1]:.1f} dv {ratios[2]:.1f}")
        assert max(ratios) > 1.0, (case, delta, delta_lo, ratios)
