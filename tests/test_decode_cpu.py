"""KV-cache decode without a device: the C ABI of fa_decode_launch (struct layout, exports, validation before any HIP call, the
split rule and the workspace size) and the ISA the build keeps for the decode slice."""
import ctypes
import os
import re
import subprocess

import pytest

from flash_attention_from_scratch_amd import _capi
from tests.conftest import ROOT
from tests.test_varlen_cpu import _layout

BUILD = os.path.join(ROOT, "flash_attention_from_scratch_amd", "csrc", "build")
NEW_SYMBOLS = ("fa_decode_supported", "fa_decode_num_splits", "fa_decode_workspace_bytes", "fa_decode_launch")
JITTER = os.path.join(ROOT, "flash_attention_from_scratch_amd", "lib", "libfa_hip_jitter.so")


def test_decode_struct_mirror_matches_the_header():
    got, want = _layout(_capi.FaDecodeArgs, "fa_decode_args")
    assert got == want
    assert ctypes.sizeof(_capi.FaDecodeArgs) == 4 * 4 + 8 * 8 + 20 * 8


def test_decode_symbols_abi_version_and_registry():
    assert set(NEW_SYMBOLS) <= set(_capi.EXPORTED_SYMBOLS)
    for path in (_capi.LIB_PATH, JITTER):
        nm = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True)
        exported = set(re.findall(r" T (fa_[a-z_0-9]+)", nm.stdout))
        assert set(NEW_SYMBOLS) <= exported, (path, set(NEW_SYMBOLS) - exported)
    lib = _capi.load()
    assert lib.fa_abi_version() == 6
    twin = ctypes.CDLL(JITTER)   # the decode kernels are outside the registry: the count is the twin's
    twin.fa_num_kernels.restype = ctypes.c_int
    assert lib.fa_num_kernels() == twin.fa_num_kernels()


def _args(batch=2, Sq=1, H=8, Hkv=2, cache=4096, paged=None, **over):
    """Contiguous by default; paged=(num_pages, page_size, max_pages_per_seq).  Pointers are fake but aligned: no launch
    here reaches a device."""
    f = dict(dtype=15, q=16, k=16, v=16, o=16, lse=16, cache_seqlens=16, workspace=16, batch=batch, seqlen_q=Sq, n_heads=H, n_kv_heads=Hkv,
             q_batch_stride=Sq * H * 128, q_seq_stride=H * 128, q_head_stride=128,
             o_batch_stride=Sq * H * 128, o_seq_stride=H * 128, o_head_stride=128, kv_seq_stride=Hkv * 128, kv_head_stride=128)
    if paged:
        num_pages, page_size, per_seq = paged
        f.update(block_table=16, num_pages=num_pages, page_size=page_size, max_pages_per_seq=per_seq, block_table_stride=per_seq,
                 kv_batch_stride=page_size * Hkv * 128)
    else:
        f.update(seqlen_cache=cache, kv_batch_stride=cache * Hkv * 128)
    f.update(over)
    return _capi.make_decode_args(**f)


REFUSALS = [
    # null pointers
    (dict(q=None), -1, "null tensor pointer"), (dict(k=None), -1, "null tensor pointer"), (dict(v=None), -1, "null tensor pointer"),
    (dict(o=None), -1, "null tensor pointer"), (dict(cache_seqlens=None), -1, "cache_seqlens is null"),
    (dict(batch=1, Hkv=1, workspace=None), -1, "workspace is null"),
    # dtype
    (dict(dtype=7), -2, "Only fp16 and bf16"),
    # no kernel: packed rows, page size
    (dict(Sq=9, H=8, Hkv=1), -3, "64 packed query rows"), (dict(Sq=65, H=8, Hkv=8), -3, "64 packed query rows"),
    (dict(paged=(10, 32, 4)), -3, "multiple of 64"), (dict(paged=(10, 96, 4)), -3, "multiple of 64"),
    # sizes, strides, struct_size
    (dict(struct_size=8), -4, "struct_size"), (dict(d_head=64), -4, "d_head = 128"), (dict(batch=-1), -4, "batch"),
    (dict(Sq=0), -4, "seqlen_q"), (dict(H=8, Hkv=3), -4, "n_kv_heads"), (dict(Hkv=0), -4, "n_kv_heads"),
    (dict(cache=0), -4, "seqlen_cache"), (dict(paged=(0, 64, 4)), -4, "num_pages"), (dict(paged=(10, 64, 0)), -4, "max_pages_per_seq"),
    (dict(paged=(10, 64, 4), block_table_stride=3), -4, "block_table_stride"),
    (dict(max_seqlen_k=4097), -4, "max_seqlen_k"), (dict(max_seqlen_k=-1), -4, "max_seqlen_k"),
    (dict(num_splits=-1), -4, "num_splits"), (dict(num_splits=1025), -4, "num_splits"),
    (dict(q_seq_stride=0), -4, "q strides"), (dict(o_seq_stride=-8), -4, "o strides"), (dict(kv_seq_stride=0), -4, "kv strides"),
    (dict(kv_batch_stride=0), -4, "kv strides"),
    # alignment
    (dict(q_head_stride=132), -5, "q strides"), (dict(kv_seq_stride=260), -5, "kv strides"), (dict(o_batch_stride=1028), -5, "o strides"),
    (dict(q=24), -5, "16-byte aligned"), (dict(k=8), -5, "16-byte aligned"), (dict(v=4), -5, "16-byte aligned"), (dict(o=2), -5, "16-byte aligned"),
    (dict(cache_seqlens=18), -5, "4-byte aligned"), (dict(lse=6), -5, "4-byte aligned"),
    (dict(paged=(10, 64, 4), block_table=10), -5, "4-byte aligned"),
    (dict(batch=1, Hkv=1, workspace=8), -5, "workspace must be 16-byte aligned"),
]


@pytest.mark.parametrize("over,status,text", REFUSALS, ids=[f"{i}:{s}" for i, (_, s, _) in enumerate(REFUSALS)])
def test_decode_launch_refusals_without_a_device(over, status, text):
    lib = _capi.load()
    a = _args(**over)
    rc = lib.fa_decode_launch(ctypes.byref(a), None, None)
    assert rc == status, (rc, _capi.last_error())
    assert text in _capi.last_error()
    if status == -3:
        assert lib.fa_decode_supported(ctypes.byref(a)) == 0
    if status in (-2, -3, -4) or "strides" in text:   # (what does not depend on a pointer's value is refused by the queries too)
        assert lib.fa_decode_num_splits(ctypes.byref(a)) == status
        assert lib.fa_decode_workspace_bytes(ctypes.byref(a)) == status


def test_decode_null_args_and_empty_batch():
    lib = _capi.load()
    assert lib.fa_decode_launch(None, None, None) == -1
    assert lib.fa_decode_supported(None) == 0
    ms = ctypes.c_float(-1.0)
    assert lib.fa_decode_launch(ctypes.byref(_args(batch=0, workspace=None)), None, ctypes.byref(ms)) == 0   # no device needed
    assert ms.value == 0.0
    assert lib.fa_decode_launch(ctypes.byref(_args(batch=0, paged=(10, 64, 4))), None, None) == 0
    for dtype in (5, 15):
        assert lib.fa_decode_supported(ctypes.byref(_args(dtype=dtype))) == 1
        assert lib.fa_decode_supported(ctypes.byref(_args(dtype=dtype, Sq=8, H=8, Hkv=1))) == 1     # 64 rows
        assert lib.fa_decode_supported(ctypes.byref(_args(dtype=dtype, Sq=64, H=4, Hkv=4))) == 1
        assert lib.fa_decode_supported(ctypes.byref(_args(dtype=dtype, paged=(100, 256, 7)))) == 1


# (batch, Sq, H, Hkv, capacity, max_seqlen_k, forced) -> splits.  The rule: the smallest power of two s with batch * Hkv * s >= 256,
# at most ceil(max_seqlen_k / 256), at most 128.
SPLITS = [
    ((64, 1, 32, 8, 8192, 0, 0), 1),          # 512 workgroups already: the rule gives 1
    ((256, 1, 16, 1, 65536, 0, 0), 1),
    ((8, 1, 32, 8, 65536, 0, 0), 4),
    ((1, 1, 32, 8, 65536, 0, 0), 32),
    ((3, 4, 8, 2, 65536, 0, 0), 64),          # 6 * 64 >= 256 > 6 * 32
    ((1, 1, 32, 8, 1024, 0, 0), 4),           # capped by the bound: ceil(1024 / 256)
    ((1, 1, 32, 8, 65536, 1000, 0), 4),       # ... by max_seqlen_k, not the capacity
    ((1, 1, 32, 8, 65536, 700, 0), 3),
    ((2, 1, 8, 8, 100, 0, 0), 1),
    ((1, 1, 16, 1, 65536, 0, 0), 128),        # capped by the maximum (256 wanted, 256 allowed by the bound)
    ((1, 1, 16, 1, 1 << 20, 0, 0), 128),
    ((1, 1, 32, 8, 65536, 0, 7), 7),          # forced
    ((64, 1, 32, 8, 8192, 0, 200), 200),
    ((1, 1, 32, 8, 256, 0, 1), 1),
]


@pytest.mark.parametrize("shape,want", SPLITS, ids=[str(i) for i in range(len(SPLITS))])
@pytest.mark.parametrize("paged", [False, True], ids=["contiguous", "paged"])
def test_decode_split_rule_and_workspace(shape, want, paged):
    lib = _capi.load()
    batch, Sq, H, Hkv, cap, max_k, forced = shape
    kw = dict(batch=batch, Sq=Sq, H=H, Hkv=Hkv, max_seqlen_k=max_k, num_splits=forced)
    if paged:
        per_seq = (cap + 63) // 64   # (a capacity off the page size: the same bound through max_seqlen_k)
        kw["paged"] = (batch * per_seq + 1, 64, per_seq)
        kw["max_seqlen_k"] = max_k or cap
    else:
        kw["cache"] = cap
    a = _args(**kw)
    assert lib.fa_decode_num_splits(ctypes.byref(a)) == want, _capi.last_error()
    rows = Sq * (H // Hkv)
    part_o = 4 * want * batch * Hkv * rows * 128
    part_lse = (4 * want * batch * Hkv * rows + 15) // 16 * 16
    assert lib.fa_decode_workspace_bytes(ctypes.byref(a)) == (0 if want == 1 else part_o + part_lse)


def _kernels(text):
    """{kernel name: its ISA text} of a kept .s"""
    out = {}
    for m in re.finditer(r"^(_Z\w+):.*?\n\s*\.end_amdhsa_kernel", text, re.M | re.S):
        out[m.group(1)] = m.group(0)
    return out


def test_decode_slice_isa():
    path = os.path.join(BUILD, "decode", "fa_decode-hip-amdgcn-amd-amdhsa-gfx950.s")
    assert os.path.exists(path), "the build keeps the decode slice's ISA (-save-temps=obj)"
    text = open(path).read()
    assert "v_mfma_f32_16x16x32_bf16" in text and "v_mfma_f32_16x16x32_f16" in text
    assert "global_load_dwordx4" in text and "ds_read_b64_tr_b16" in text
    assert "scratch_" not in text
    sizes = re.findall(r"\.amdhsa_private_segment_fixed_size (\d+)", text)
    assert sizes and all(s == "0" for s in sizes)
    assert all(s == "0" for s in re.findall(r"\.vgpr_spill_count:\s+(\d+)", text))
    names = set(re.findall(r"^\s+\.name:\s+(_Z\w+)$", text, re.M))
    want = {f"_ZN2fa22fa_decode_split_kernelINS_10DecodeArgsELi{dt}ELi{nt}ELb{p}EEEvT_" for dt in (15, 5) for nt in (1, 2, 4) for p in (0, 1)}
    want |= {f"_ZN2fa24fa_decode_combine_kernelILi{dt}EEEvNS_10DecodeArgsE" for dt in (15, 5)}
    assert names == want, names ^ want
    for name, body in _kernels(text).items():   # each dtype's kernels use that dtype's MFMA only
        if "split_kernelINS_10DecodeArgsELi15E" in name:
            assert "v_mfma_f32_16x16x32_bf16" in body and "v_mfma_f32_16x16x32_f16" not in body
        if "split_kernelINS_10DecodeArgsELi5E" in name:
            assert "v_mfma_f32_16x16x32_f16" in body and "v_mfma_f32_16x16x32_bf16" not in body


def test_forward_kvcache_is_exposed():
    import flash_attention
    import flash_attention_from_scratch_amd.flash_attention as inner
    from flash_attention_from_scratch_amd import flash_attention_kernels as fak

    assert flash_attention.forward_kvcache is inner.forward_kvcache
    assert callable(fak.forward_kvcache)


def test_decode_prefetch_stays_in_flight():
    """The 16- and 32-row forms hold the next unit's K and V (16 global_load_dwordx4) in flight under the current unit's work: in
    each half of the unrolled loop, between the prefetch's last load and the first transposed LDS read of the P V products, no
    wait goes below vmcnt(16).  (In the second half the allocator drains the previous unit's loads BEFORE it issues the prefetch,
    earlier in the block; this test pins the overlap under the unit's work, not that drain: DESIGN.md 10.)"""
    path = os.path.join(BUILD, "decode", "fa_decode-hip-amdgcn-amd-amdhsa-gfx950.s")
    kernels = _kernels(open(path).read())
    checked = 0
    for name, body in kernels.items():
        if "split_kernel" not in name or "ELi4ELb" in name:
            continue
        halves = 0
        for block in re.split(r"^\.LBB\d+_\d+:", body, flags=re.M):
            ops = re.findall(r"^\s+(global_load_dwordx4|ds_read_b64_tr_b16|s_waitcnt[^\n]*vmcnt\((\d+)\))", block, re.M)
            kinds = [o[0].split()[0] for o in ops]
            if kinds.count("global_load_dwordx4") < 16 or "ds_read_b64_tr_b16" not in kinds:
                continue
            last_load = max(i for i, k in enumerate(kinds) if k == "global_load_dwordx4")
            first_read = kinds.index("ds_read_b64_tr_b16")
            if first_read < last_load:
                continue
            waits = [int(o[1]) for o in ops[last_load:first_read] if o[1]]
            assert waits and min(waits) >= 16, (name, waits)
            halves += 1
        assert halves == 2, (name, halves)
        checked += 1
    assert checked == 8
