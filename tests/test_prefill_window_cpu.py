"""Sliding-window attention in the packed forward and the cache prefill without a device: the six
fa_fwd_*varlen*_window exports (symbols, prototypes, validation before any HIP call, in the unwindowed entries' order), the
keyword-only window_size of forward_varlen and forward_varlen_kvcache, the ISA the build keeps for the six windowed slices, the
bench tool's host tile count, and the beacon inputs of tests/test_prefill_window_gpu.py against deliberately wrong masks."""
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
from flash_attention_from_scratch_amd import _capi
from flash_attention_from_scratch_amd import flash_attention_kernels as fak
from tests.conftest import ROOT
from tests.test_prefill_kvcache_cpu import _contig, _fwd, _kv, _paged, _vl

BUILD = os.path.join(ROOT, "flash_attention_from_scratch_amd", "csrc", "build")
JITTER = os.path.join(ROOT, "flash_attention_from_scratch_amd", "lib", "libfa_hip_jitter.so")
FORMS = ("varlen_qk", "varlen_kvcache", "varlen_kvcache_fp8")
NEW_SYMBOLS = tuple(f"fa_fwd_{what}{form}_window{tail}" for form in FORMS for what, tail in (("", "_supported"), ("launch_", "")))
MAX_LEN = (1 << 30) - 128


def _w(left=-1, right=-1, **over):
    w = _capi.make_window(left, right)
    for name, value in over.items():
        setattr(w, name, value)
    return w


def _scales(**over):
    fields = dict(k_descale=16, v_descale=16, descale_batch_stride=2)
    fields.update(over)
    return _capi.make_kvcache_fp8_scales(**fields)


def _launch(form, window, windowed=True, args=None, kv=None, vq=None, key=None, sc=None, opts=None, lse=16):
    """one launch of `form` (its windowed entry, or its unwindowed sibling) on host-only arguments -> (status, message)"""
    lib = _capi.load()
    args, kv, vq, opts = args or _fwd(), kv or _kv(), vq or _vl(), opts or _capi.make_opts()
    if key is None:
        key = _vl(T=5000, max_seqlen=4096) if form == "varlen_qk" else _contig()
    argv = [ctypes.byref(args), ctypes.byref(kv), ctypes.byref(vq), ctypes.byref(key)]
    if form == "varlen_kvcache_fp8":
        argv.append(ctypes.byref(sc or _scales()))
    if windowed:
        argv.append(ctypes.byref(window) if window is not None else None)
    fn = getattr(lib, f"fa_fwd_launch_{form}_window" if windowed else f"fa_fwd_launch_{form}")
    rc = fn(*argv, ctypes.byref(opts), ctypes.c_void_p(lse) if lse is not None else None, None)
    return rc, _capi.last_error()


def test_symbols_prototypes_and_abi_version():
    assert len(NEW_SYMBOLS) == 6 and set(NEW_SYMBOLS) <= set(_capi.EXPORTED_SYMBOLS)
    for path in (_capi.LIB_PATH, JITTER):
        nm = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True)
        exported = set(re.findall(r" T (fa_[a-z_0-9]+)", nm.stdout))
        assert set(NEW_SYMBOLS) <= exported, (path, set(NEW_SYMBOLS) - exported)
    header = open(os.path.join(ROOT, "include", "fa_hip.h")).read()
    for name in NEW_SYMBOLS:
        assert re.search(rf"\b{name}\(", header), name
    lib = _capi.load()
    assert lib.fa_abi_version() == 6 and _capi.FA_ABI_VERSION == 6   # additive: no struct grew, fa_window is reused
    assert ctypes.sizeof(_capi.FaWindow) == 12
    for form in FORMS:
        sibling, launch = getattr(lib, f"fa_fwd_launch_{form}"), getattr(lib, f"fa_fwd_launch_{form}_window")
        want = list(sibling.argtypes)
        assert list(launch.argtypes) == want[:-3] + [ctypes.POINTER(_capi.FaWindow)] + want[-3:] and launch.restype == ctypes.c_int
        supported = getattr(lib, f"fa_fwd_{form}_window_supported")
        assert len(supported.argtypes) == 2 and supported.restype == ctypes.c_int
        cfg = _capi.make_config(fak.varlen_config(torch.bfloat16))
        for o in (None, _capi.make_opts(causal=True), _capi.make_opts(speculative=True)):
            op = ctypes.byref(o) if o is not None else None
            assert supported(ctypes.byref(cfg), op) == lib.fa_fwd_varlen_supported(ctypes.byref(cfg), op)
        assert supported(None, None) == 0


WINDOW_REFUSALS = [
    (None, False, -1, "fa_window is null"),
    (_w(struct_size=8), False, -4, "fa_window.struct_size"),
    (_w(struct_size=0), False, -4, "fa_window.struct_size"),
    (_w(-2, 0), False, -4, "left and right must be -1"),
    (_w(0, -2), False, -4, "left and right must be -1"),
    (_w(10, 1), True, -4, "causal means right = 0"),
    (_w(-1, 5), True, -4, "causal means right = 0"),
]


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("case", WINDOW_REFUSALS, ids=[str(i) for i in range(len(WINDOW_REFUSALS))])
def test_window_refusals_without_a_device(form, case):
    window, causal, status, text = case
    rc, msg = _launch(form, window, opts=_capi.make_opts(causal=causal))
    assert rc == status and text in msg, (rc, msg)


@pytest.mark.parametrize("form", FORMS)
def test_the_size_bound_at_2_30_minus_128_and_one_above(form):
    """the key bound (the cache's capacity; packed: the key side's max_seqlen) and the query side's max_seqlen: at the bound the call
    passes (total_q = 0 returns before a device is asked), one above it is refused"""
    w = _w(100, 0)
    for n, status, text in ((MAX_LEN, 0, ""), (MAX_LEN + 1, -4, "too large for a window")):
        if form == "varlen_qk":
            key, kv = _vl(T=0, max_seqlen=n), None
        else:
            key, kv = _contig(seqlen_cache=n), _kv(bs=n * 256)
        rc, msg = _launch(form, w, args=_fwd(T=0), vq=_vl(T=0), key=key, kv=kv)
        assert rc == status and text in msg, (n, rc, msg)
        rc, msg = _launch(form, w, args=_fwd(T=0), vq=_vl(T=0, max_seqlen=n))
        assert rc == status and text in msg, (n, rc, msg)
        # (the unwindowed sibling has no such bound)
        assert _launch(form, None, windowed=False, args=_fwd(T=0), vq=_vl(T=0, max_seqlen=n))[0] == 0


@pytest.mark.parametrize("form", FORMS)
def test_what_the_unwindowed_entry_refuses_arrives_first(form):
    """three of the sibling's refusals, each with a window that is itself refused: the sibling's status and message win"""
    bad = _w(-5, -5)
    cases = [(dict(lse=None), -1, "lse is null"), (dict(args=_fwd(d_head=64)), -4, "d_head"), (dict(vq=_vl(cu=18)), -5, "cu_seqlens must be 4-byte")]
    if form != "varlen_qk":
        cases.append((dict(key=_paged(page_size=96), kv=_kv(bs=96 * 256)), -3, "multiple of 64"))
    for over, status, text in cases:
        rc, msg = _launch(form, bad, **over)
        assert rc == status and text in msg, (over, rc, msg)
        rc0, msg0 = _launch(form, None, windowed=False, **over)   # (the sibling's words, but for the entry's own name in them)
        assert rc0 == rc and msg0.replace(f"fa_fwd_launch_{form}", f"fa_fwd_launch_{form}_window") == msg
    rc, msg = _launch(form, bad)
    assert rc == -4 and "left and right must be -1" in msg


@pytest.mark.parametrize("form", FORMS)
def test_total_q_zero_returns_ok_without_a_device(form):
    for window, causal in ((_w(), False), (_w(0, 0), True), (_w(5, -1), True), (_w(2 ** 31 - 1, 2 ** 31 - 1), False)):
        ms = ctypes.c_float(-1.0)
        rc, msg = _launch(form, window, args=_fwd(T=0), vq=_vl(T=0), opts=_capi.make_opts(causal=causal, ms=ms))
        assert rc == 0 and ms.value == 0.0, msg


def test_window_size_is_keyword_only_in_both_wrappers():
    import flash_attention_from_scratch_amd.flash_attention as inner

    for fn in (flash_attention.forward_varlen, inner.forward_varlen, fak.forward_varlen, flash_attention.forward_varlen_kvcache,
               inner.forward_varlen_kvcache, fak.forward_varlen_kvcache):
        p = inspect.signature(fn).parameters["window_size"]
        assert p.kind is inspect.Parameter.KEYWORD_ONLY and p.default == (-1, -1), fn
        assert "window_size" not in fn.__code__.co_varnames[:fn.__code__.co_argcount]
    for fn in (flash_attention.backward_varlen, fak.backward_varlen):
        assert "window_size" not in inspect.signature(fn).parameters   # (open: DESIGN.md 10.13)


# the ten window_size values of tests/test_wrapper_refusals_cpu.py that forward_kvcache refuses or takes: the eight bad ones, and two
# more bad ones of tests/test_window_cpu.py
BAD_WINDOWS = [((1,), False, "pair of Python ints"), ("ab", False, "pair of Python ints"), ((1.0, 0), False, "pair of Python ints"),
               ((True, 0), False, "pair of Python ints"), ((-2, 0), False, "must be -1"), ((0, -2), False, "must be -1"),
               ((2 ** 31, 0), False, "32-bit"), ((4, 5), True, "causal means right = 0"), (5, False, "pair of Python ints"),
               ((torch.tensor(3), 0), False, "pair of Python ints")]


def test_bad_window_sizes_are_value_errors_before_any_tensor_is_looked_at():
    assert len(BAD_WINDOWS) == 10
    for window, causal, text in BAD_WINDOWS:
        for fn in (flash_attention.forward_varlen_kvcache, fak.forward_varlen_kvcache):
            with pytest.raises(ValueError, match=text):
                fn(None, None, None, None, None, None, causal=causal, window_size=window)
        for fn in (flash_attention.forward_varlen, fak.forward_varlen):
            with pytest.raises(ValueError, match=text):
                fn(None, None, None, None, None, causal=causal, window_size=window)
    # (a good window gets as far as the tensors)
    with pytest.raises(RuntimeError, match="must be a tensor"):
        fak.forward_varlen_kvcache(None, None, None, None, None, None, window_size=(16, 0))


SLICES = [("varlen_window", "fa_inst_varlen", "27fa_fwd_kernel_varlen_window"),
          ("varlen_kvcache_window", "fa_inst_varlen", "35fa_fwd_kernel_varlen_kvcache_window"),
          ("varlen_kvcache_fp8_window", "fa_inst_varlen", "39fa_fwd_kernel_varlen_kvcache_fp8_window")]


@pytest.mark.parametrize("folder,unit,kernel", SLICES, ids=[s[0] for s in SLICES])
@pytest.mark.parametrize("dt", [15, 5])
def test_windowed_slices_are_kept_with_two_kernels_no_scratch_and_no_vector_spill(folder, unit, kernel, dt):
    path = os.path.join(BUILD, f"{folder}_dt{dt}", f"{unit}-hip-amdgcn-amd-amdhsa-gfx950.s")
    assert os.path.exists(path), "the build keeps the ISA of every slice under csrc/build (make -C flash_attention_from_scratch_amd/csrc)"
    text = open(path).read()
    assert len(re.findall(rf"^_ZN2fa{kernel}I\w+:", text, flags=re.M)) == 2
    assert len(re.findall(r"^\s+\.name:\s+_Z\w+$", text, flags=re.M)) == 2       # ... and no other kernel
    assert re.findall(r"; ScratchSize: (\d+)", text) == ["0", "0"]
    assert re.findall(r"\.private_segment_fixed_size:\s+(\d+)", text) == ["0", "0"]
    assert re.findall(r"\.vgpr_spill_count:\s+(\d+)", text) == ["0", "0"]
    assert re.findall(r"; Occupancy: (\d+)", text) == ["1", "1"]
    sgpr_spills = re.findall(r"\.sgpr_spill_count:\s+(\d+)", text)   # (scalars spilled to lanes are allowed: DESIGN.md 10.13 records them)
    print(f"{folder} dt{dt}: sgpr_spill_count {sgpr_spills}")
    assert len(sgpr_spills) == 2


def test_the_bench_counts_tiles_as_the_rule_does():
    path = os.path.join(ROOT, "flash_attention_from_scratch_amd", "tools", "prefill_window_bench.py")
    spec = importlib.util.spec_from_file_location("prefill_window_bench", path)
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    pairs = [(165, 197), (37, 1000), (1, 777), (128, 192), (300, 100), (0, 300), (200, 0), (64, 64), (129, 65), (300, 1000), (512, 1536)]
    windows = [(0, 0), (1, 0), (31, 0), (63, 0), (64, 0), (127, 0), (128, 0), (200, 3), (-1, 5), (5, -1), (0, 64), (1000, 0), (-1, -1), (-1, 0)]
    for n_q, n_k in pairs:
        for left, right in windows:
            lo, hi = bi.window_bounds(n_q, n_k, left, right)
            tiles = 0
            for r0 in range(0, n_q, 128):   # brute force: the tiles that hold a key some row of the block sees, and every tile between
                live = [r for r in range(r0, min(r0 + 128, n_q)) if hi[r] >= lo[r]]
                if live:
                    tiles += int(max(hi[r] for r in live)) // 64 - int(min(lo[r] for r in live)) // 64 + 1
            assert bench.visited_tiles(n_q, n_k, left, right) == tiles, (n_q, n_k, left, right)
    # the figures the GPU test's sequences were chosen by
    assert [bench.visited_tiles(300, 1000, -1, 0)] == [44]
    assert {bench.visited_tiles(300, 1000, w, 0) for w in (0, 1, 31, 63, 64, 127, 128)} <= set(range(8, 18))
    assert bi.window_lo_min(197, 165, 0) == 32 and bi.window_lo_min(777, 1, 0) == 776 and bi.window_lo_min(1000, 300, 0) == 700
    assert int((lambda b: (b[1] < b[0]).sum())(bi.window_bounds(300, 100, 0, 0))) == 200


# ---- the beacon inputs of the GPU test against wrong masks ---------------------------------------------------------------------

BEACON_PAIRS = [(165, 197), (37, 1000), (300, 1000), (129, 65)]
BEACON_WINDOWS = [(0, 0), (1, 0), (63, 0), (64, 0), (127, 0), (128, 0), (200, 3)]


def _beacon_positions():
    path = os.path.join(ROOT, "tests", "test_prefill_window_gpu.py")
    spec = importlib.util.spec_from_file_location("_prefill_window_gpu_positions", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert mod.BEACON_PAIRS == BEACON_PAIRS and mod.BEACON_WINDOWS == BEACON_WINDOWS
    return mod.beacon_positions


@pytest.mark.parametrize("pair", BEACON_PAIRS, ids=str)
@pytest.mark.parametrize("w", BEACON_WINDOWS, ids=str)
def test_beacons_reject_a_mask_shifted_by_one_at_either_edge(pair, w):
    """eager attention with the upper edge moved by +-1 (delta) or the lower edge by +-1 (delta_lo) must fail beacon_inputs.compare
    on the inputs the GPU test feeds the kernels (cpu_cap lengths: the remainder by 64 on top of 1024 keys), in some phase."""
    n_q, n_k = bi.cpu_cap(pair[0]), bi.cpu_cap(pair[1])
    dtype = torch.bfloat16
    listed = _beacon_positions()(n_q, n_k, *w)
    lo_b = bi.window_lo_min(n_k, n_q, w[0])
    assert listed and all(lo_b <= p < n_k for p in listed)
    phase, n_phases = 0, 1
    while phase < n_phases:
        s = bi.build_window_sequence(n_q, n_k, 8, 2, listed, dtype, w[0], w[1], phase, seed=phase)
        n_phases, phase = s["n_phases"], phase + 1
        o32, lse32, o16 = bi.references(s)
        assert bi.compare(o16, None, o32, lse32, o16, dtype)["ok"] and bi.compare(o32, lse32, o32, lse32, o16, dtype)["ok"]
        live = s["diag"] >= s["lo"]
        # (the key behind the last one and the key below the first exist in k: rows n_k and lo - 1; where no live row has a key below
        # its window, lo = 0 throughout, a lower edge moved down is the same mask)
        mutants = [(1, 0), (-1, 0), (0, 1)] + ([(0, -1)] if bool((s["lo"][live] >= 1).any()) else [])
        for delta, delta_lo in mutants:
            o, lse = bi.eager(s["q"], s["k"][:n_k + 1], s["v"][:n_k + 1], s["diag"], torch.float32, delta=delta, lo=s["lo"], delta_lo=delta_lo)
            res = bi.compare(o, lse, o32, lse32, o16, dtype)
            assert not res["ok"], (pair, w, phase, delta, delta_lo, res)
