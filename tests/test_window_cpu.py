"""Sliding-window decode without a device: fa_window and the fa_decode_window_* / fa_decode_fp8_window_* entry points (struct
layout, exports, validation before any HIP call, the split rule and the workspace size), the ISA the build keeps for the two
windowed slices, and the window_size keyword of forward_kvcache."""
import ctypes
import inspect
import os
import re
import subprocess

import pytest
import torch

from flash_attention_from_scratch_amd import _capi
from flash_attention_from_scratch_amd import flash_attention_kernels as fak
from tests.conftest import ROOT
from tests.test_decode_cpu import _args, _kernels
from tests.test_decode_fp8_cpu import _args as _args8
from tests.test_varlen_cpu import _layout

BUILD = os.path.join(ROOT, "flash_attention_from_scratch_amd", "csrc", "build")
JITTER = os.path.join(ROOT, "flash_attention_from_scratch_amd", "lib", "libfa_hip_jitter.so")
NEW_SYMBOLS = tuple(f"fa_decode{fp8}_window_{what}" for fp8 in ("", "_fp8") for what in ("supported", "num_splits", "workspace_bytes", "launch"))


def _w(left=-1, right=-1, **over):
    w = _capi.make_window(left, right)
    for name, value in over.items():
        setattr(w, name, value)
    return w


def _entry(lib, fp8, what):
    return getattr(lib, f"fa_decode{'_fp8' if fp8 else ''}_window_{what}")


def test_window_struct_mirror_matches_the_header():
    got, want = _layout(_capi.FaWindow, "fa_window")
    assert got == want
    assert ctypes.sizeof(_capi.FaWindow) == 12


def test_window_symbols_and_abi_version():
    assert set(NEW_SYMBOLS) <= set(_capi.EXPORTED_SYMBOLS)
    for path in (_capi.LIB_PATH, JITTER):
        nm = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True)
        exported = set(re.findall(r" T (fa_[a-z_0-9]+)", nm.stdout))
        assert set(NEW_SYMBOLS) <= exported, (path, set(NEW_SYMBOLS) - exported)
    header = open(os.path.join(ROOT, "include", "fa_hip.h")).read()
    for name in NEW_SYMBOLS:
        assert re.search(rf"\b{name}\(", header), name
    lib = _capi.load()
    assert lib.fa_abi_version() == 6   # additive: no struct grew
    assert ctypes.sizeof(_capi.FaDecodeArgs) == 4 * 4 + 8 * 8 + 20 * 8


WINDOW_REFUSALS = [
    (dict(window=None), {}, -1, "fa_window is null"),
    (dict(window=_w(struct_size=8)), {}, -4, "fa_window.struct_size"),
    (dict(window=_w(struct_size=0)), {}, -4, "fa_window.struct_size"),
    (dict(window=_w(-2, 0)), {}, -4, "left and right must be -1"),
    (dict(window=_w(0, -2)), {}, -4, "left and right must be -1"),
    (dict(window=_w(-7, -7)), {}, -4, "left and right must be -1"),
    (dict(window=_w(10, 1)), dict(causal=1), -4, "causal means right = 0"),
    (dict(window=_w(-1, 5)), dict(causal=1), -4, "causal means right = 0"),
    (dict(window=_w(100, 0)), dict(cache=(1 << 30) - 127, kv_batch_stride=((1 << 30) - 127) * 256), -4, "cache too large for a window"),
]
# what the unwindowed entry refuses, a sample of every status (the whole list: tests/test_decode_cpu.py)
BASE_REFUSALS = [
    (dict(q=None), -1, "null tensor pointer"), (dict(cache_seqlens=None), -1, "cache_seqlens is null"),
    (dict(batch=1, Hkv=1, workspace=None), -1, "workspace is null"), (dict(dtype=7), -2, "Only fp16 and bf16"),
    (dict(Sq=9, H=8, Hkv=1), -3, "64 packed query rows"), (dict(paged=(10, 96, 4)), -3, "multiple of 64"),
    (dict(struct_size=8), -4, "struct_size"), (dict(d_head=64), -4, "d_head = 128"), (dict(max_seqlen_k=4097), -4, "max_seqlen_k"),
    (dict(num_splits=1025), -4, "num_splits"), (dict(kv_seq_stride=0), -4, "kv strides"),
    (dict(q_head_stride=132), -5, "q strides"), (dict(k=8), -5, "16-byte aligned"), (dict(cache_seqlens=18), -5, "4-byte aligned"),
    (dict(batch=1, Hkv=1, workspace=8), -5, "workspace must be 16-byte aligned"),
]


@pytest.mark.parametrize("fp8", [False, True], ids=["16bit", "fp8"])
@pytest.mark.parametrize("case", WINDOW_REFUSALS, ids=[str(i) for i in range(len(WINDOW_REFUSALS))])
def test_window_refusals_without_a_device(fp8, case):
    kw, over, status, text = case
    lib = _capi.load()
    a = (_args8 if fp8 else _args)(**over)
    w = kw["window"]
    wp = ctypes.byref(w) if w is not None else None
    rc = _entry(lib, fp8, "launch")(ctypes.byref(a), wp, None, None)
    assert rc == status, (rc, _capi.last_error())
    assert text in _capi.last_error()
    assert _entry(lib, fp8, "supported")(ctypes.byref(a), wp) == 0
    assert _entry(lib, fp8, "num_splits")(ctypes.byref(a), wp) == status
    assert _entry(lib, fp8, "workspace_bytes")(ctypes.byref(a), wp) == status


@pytest.mark.parametrize("fp8", [False, True], ids=["16bit", "fp8"])
@pytest.mark.parametrize("over,status,text", BASE_REFUSALS, ids=[f"{i}:{s}" for i, (_, s, _) in enumerate(BASE_REFUSALS)])
def test_window_entries_refuse_what_the_unwindowed_ones_refuse(fp8, over, status, text):
    lib = _capi.load()
    a = (_args8 if fp8 else _args)(**over)
    w = _w(2000, 0)   # (more than one split, so the workspace is asked for)
    rc = _entry(lib, fp8, "launch")(ctypes.byref(a), ctypes.byref(w), None, None)
    assert rc == status, (rc, _capi.last_error())
    assert text in _capi.last_error()
    assert (lib.fa_decode_fp8_launch if fp8 else lib.fa_decode_launch)(ctypes.byref(a), None, None) == status


def test_window_fp8_refusals_and_empty_batch():
    lib = _capi.load()
    w = _w(100, 0)
    rc = lib.fa_decode_fp8_window_launch(ctypes.byref(_args8(kv_dtype=2)), ctypes.byref(w), None, None)
    assert rc == -2 and "kv_dtype" in _capi.last_error()
    rc = lib.fa_decode_fp8_window_launch(ctypes.byref(_args8(k_descale=6)), ctypes.byref(w), None, None)
    assert rc == -5 and "k_descale and v_descale" in _capi.last_error()
    assert lib.fa_decode_window_launch(None, ctypes.byref(w), None, None) == -1
    assert lib.fa_decode_fp8_window_launch(None, ctypes.byref(w), None, None) == -1
    assert lib.fa_decode_window_supported(None, ctypes.byref(w)) == 0
    for fp8 in (False, True):
        ms = ctypes.c_float(-1.0)
        a = (_args8 if fp8 else _args)(batch=0, workspace=None)
        assert _entry(lib, fp8, "launch")(ctypes.byref(a), ctypes.byref(w), None, ctypes.byref(ms)) == 0   # no device needed
        assert ms.value == 0.0
        for window, causal in ((_w(), 0), (_w(0, 0), 0), (_w(5, -1), 1), (_w(5, 0), 1), (_w(2 ** 31 - 1, 2 ** 31 - 1), 0)):
            assert _entry(lib, fp8, "supported")(ctypes.byref((_args8 if fp8 else _args)(causal=causal)), ctypes.byref(window)) == 1


# (batch, Sq, H, Hkv, capacity, max_seqlen_k, forced, causal), (left, right) -> splits.  The unwindowed rule (the smallest power of
# two s with batch * Hkv * s >= 256, at most ceil(bound / 256), at most 128) with bound = min(max_seqlen_k or capacity,
# left + Sq + right) when both sides are bounded, causal counting as right = 0.
WINDOW_SPLITS = [
    ((1, 1, 32, 8, 65536, 0, 0, 0), (255, 0), 1),        # 256 keys: one split
    ((1, 1, 32, 8, 65536, 0, 0, 1), (255, -1), 1),       # ... causal is right = 0
    ((1, 1, 32, 8, 65536, 0, 0, 0), (256, 0), 2),        # 257 keys
    ((1, 1, 32, 8, 65536, 0, 0, 0), (1023, 0), 4),       # 1024 keys
    ((1, 1, 32, 8, 65536, 0, 0, 0), (1024, 0), 5),
    ((1, 4, 8, 2, 65536, 0, 0, 1), (1020, -1), 4),       # 1020 + 4 + 0
    ((1, 4, 8, 2, 65536, 0, 0, 0), (1000, 21), 5),       # 1000 + 4 + 21 = 1025
    ((1, 1, 32, 8, 65536, 0, 0, 0), (4096, 0), 17),      # ceil(4097 / 256), below the 32 the grid wants
    ((1, 1, 32, 8, 65536, 0, 0, 0), (8191, 0), 32),      # the grid's count: the window allows 32
    ((8, 1, 32, 8, 65536, 0, 0, 0), (4096, 0), 4),       # ... and here 4
    ((8, 1, 32, 8, 65536, 0, 0, 0), (600, 0), 3),
    ((64, 1, 32, 8, 65536, 0, 0, 0), (4096, 0), 1),
    ((1, 1, 32, 8, 65536, 700, 0, 0), (4096, 0), 3),     # max_seqlen_k is the smaller bound
    ((1, 1, 32, 8, 65536, 0, 0, 0), (0, 0), 1),          # one key; never below 1
    ((1, 1, 32, 8, 65536, 0, 7, 0), (255, 0), 7),        # forced
]
# wider than the bound, or a side unbounded: fa_decode_num_splits' value
WIDE = [(-1, -1), (65536, 0), (2 ** 31 - 1, 0), (100, -1), (-1, 0), (-1, 100), (2 ** 31 - 1, 2 ** 31 - 1)]


@pytest.mark.parametrize("shape,window,want", WINDOW_SPLITS, ids=[str(i) for i in range(len(WINDOW_SPLITS))])
@pytest.mark.parametrize("paged", [False, True], ids=["contiguous", "paged"])
def test_window_split_rule_and_workspace(shape, window, want, paged):
    lib = _capi.load()
    batch, Sq, H, Hkv, cap, max_k, forced, causal = shape
    kw = dict(batch=batch, Sq=Sq, H=H, Hkv=Hkv, max_seqlen_k=max_k, num_splits=forced, causal=causal)
    if paged:
        per_seq = cap // 64
        kw["paged"] = (batch * per_seq + 1, 64, per_seq)
    else:
        kw["cache"] = cap
    w = _w(*window)
    rows = Sq * (H // Hkv)
    part_o = 4 * want * batch * Hkv * rows * 128
    part_lse = (4 * want * batch * Hkv * rows + 15) // 16 * 16
    for fp8 in (False, True):   # the fp8 entry agrees with the 16-bit one
        a = (_args8 if fp8 else _args)(**kw)
        assert _entry(lib, fp8, "num_splits")(ctypes.byref(a), ctypes.byref(w)) == want, _capi.last_error()
        assert _entry(lib, fp8, "workspace_bytes")(ctypes.byref(a), ctypes.byref(w)) == (0 if want == 1 else part_o + part_lse)


@pytest.mark.parametrize("window", WIDE, ids=[str(w) for w in WIDE])
@pytest.mark.parametrize("shape", [(1, 1, 32, 8, 65536, 0), (3, 4, 8, 2, 65536, 0), (1, 1, 32, 8, 65536, 700), (64, 1, 32, 8, 8192, 0),
                                   (1, 1, 16, 1, 1 << 20, 0)], ids=str)
def test_a_window_wider_than_the_bound_splits_as_the_unwindowed_call(window, shape):
    lib = _capi.load()
    batch, Sq, H, Hkv, cap, max_k = shape
    kw = dict(batch=batch, Sq=Sq, H=H, Hkv=Hkv, cache=cap, max_seqlen_k=max_k)
    w = _w(*window)
    a, a8 = _args(**kw), _args8(**kw)
    want = lib.fa_decode_num_splits(ctypes.byref(a))
    assert want >= 1
    assert lib.fa_decode_window_num_splits(ctypes.byref(a), ctypes.byref(w)) == want
    assert lib.fa_decode_fp8_window_num_splits(ctypes.byref(a8), ctypes.byref(w)) == want
    assert lib.fa_decode_window_workspace_bytes(ctypes.byref(a), ctypes.byref(w)) == lib.fa_decode_workspace_bytes(ctypes.byref(a))
    assert lib.fa_decode_fp8_window_workspace_bytes(ctypes.byref(a8), ctypes.byref(w)) == lib.fa_decode_workspace_bytes(ctypes.byref(a))


SLICES = [("decode_window", "fa_decode_window", "16DecodeWindowArgs", 16), ("decode_fp8_window", "fa_decode_fp8_window", "19DecodeFp8WindowArgs", 8)]


@pytest.mark.parametrize("folder,unit,args,loads", SLICES, ids=["16bit", "fp8"])
def test_window_slice_isa(folder, unit, args, loads):
    """The windowed instantiations live in slices of their own (the unwindowed slices' kernel sets are pinned by
    tests/test_decode_cpu.py and tests/test_decode_fp8_cpu.py): the expected kernels, no scratch, no spill."""
    path = os.path.join(BUILD, folder, f"{unit}-hip-amdgcn-amd-amdhsa-gfx950.s")
    assert os.path.exists(path), "the build keeps the windowed decode slice's ISA (-save-temps=obj)"
    text = open(path).read()
    assert "scratch_" not in text
    sizes = re.findall(r"\.amdhsa_private_segment_fixed_size (\d+)", text)
    assert sizes and all(s == "0" for s in sizes)
    spills = re.findall(r"\.vgpr_spill_count:\s+(\d+)", text)
    assert spills and all(s == "0" for s in spills)
    names = set(re.findall(r"^\s+\.name:\s+(_Z\w+)$", text, re.M))
    want = {f"_ZN2fa22fa_decode_split_kernelINS_{args}ELi{dt}ELi{nt}ELb{p}EEEvT_" for dt in (15, 5) for nt in (1, 2, 4) for p in (0, 1)}
    want |= {f"_ZN2fa24fa_decode_combine_kernelILi{dt}EEEvNS_10DecodeArgsE" for dt in (15, 5)}
    assert names == want, names ^ want
    for name, body in _kernels(text).items():   # each dtype's kernels use that dtype's MFMA only
        if f"split_kernelINS_{args}ELi15E" in name:
            assert "v_mfma_f32_16x16x32_bf16" in body and "v_mfma_f32_16x16x32_f16" not in body
        if f"split_kernelINS_{args}ELi5E" in name:
            assert "v_mfma_f32_16x16x32_f16" in body and "v_mfma_f32_16x16x32_bf16" not in body


@pytest.mark.parametrize("folder,unit,args,loads", SLICES, ids=["16bit", "fp8"])
def test_window_prefetch_stays_in_flight(folder, unit, args, loads):
    """The unwindowed slices' property (tests/test_decode_cpu.py: test_decode_prefetch_stays_in_flight), kept by the windowed
    forms: in each half of the unrolled loop, between the prefetch's last load and the first transposed LDS read of the P V
    products, no wait goes below the next unit's loads (16, fp8: 8).  The 16- and 32-row forms, as there."""
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


def test_window_keyword_and_its_value_errors():
    import flash_attention
    import flash_attention_from_scratch_amd.flash_attention as inner

    for fn in (flash_attention.forward_kvcache, inner.forward_kvcache, fak.forward_kvcache):
        params = list(inspect.signature(fn).parameters.values())
        # behind the cache's own keywords and in front of the fused append's, whose place at the end tests/test_kvcache_append_cpu.py pins
        assert params[12].name == "window_size" and params[12].default == (-1, -1)
        assert [p.name for p in params[10:12]] == ["k_descale", "v_descale"] and params[13].name == "k" and len(params) == 19
    assert fak._window((-1, -1), False) is None and fak._window([-1, -1], True) is None
    assert fak._window((5, 0), True) == (5, 0) and fak._window((5, -1), True) == (5, -1) and fak._window((0, 7), False) == (0, 7)
    bad = [((-2, 0), False, "must be -1"), ((0, -2), False, "must be -1"), ((3, 1), True, "causal means right = 0"),
           ((3,), False, "pair of Python ints"), (5, False, "pair of Python ints"), ((1.0, 0), False, "pair of Python ints"),
           ((True, 0), False, "pair of Python ints"), ((torch.tensor(3), 0), False, "pair of Python ints"),
           ((2 ** 31, 0), False, "32-bit")]
    t = torch.zeros(1)   # (the window is checked before the tensors: no device, no library call)
    for window, causal, text in bad:
        with pytest.raises(ValueError, match=text):
            fak._window(window, causal)
        with pytest.raises(ValueError, match=text):
            flash_attention.forward_kvcache(t, t, t, t, causal=causal, window_size=window)
        with pytest.raises(ValueError, match=text):
            fak.kvcache_num_splits(t, t, t, t, causal=causal, window_size=window)
