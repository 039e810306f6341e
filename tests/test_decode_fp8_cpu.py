"""The fp8-cache decode path without a device: the C ABI of fa_decode_fp8_launch (struct layout, exports, validation before any
HIP call, the split rule and the workspace size against fa_decode_*), the ISA the build keeps for the slice, and
quantize_kvcache_fp8 on the CPU."""
import ctypes
import os
import re
import subprocess

import pytest
import torch

from flash_attention_from_scratch_amd import _capi
from tests.conftest import ROOT
from tests.test_decode_cpu import SPLITS, _args as _args16, _kernels
from tests.test_varlen_cpu import _layout

BUILD = os.path.join(ROOT, "flash_attention_from_scratch_amd", "csrc", "build")
ISA = os.path.join(BUILD, "decode_fp8", "fa_decode_fp8-hip-amdgcn-amd-amdhsa-gfx950.s")
NEW_SYMBOLS = ("fa_decode_fp8_supported", "fa_decode_fp8_num_splits", "fa_decode_fp8_workspace_bytes", "fa_decode_fp8_launch")
JITTER = os.path.join(ROOT, "flash_attention_from_scratch_amd", "lib", "libfa_hip_jitter.so")
LOADS_PER_UNIT = 8   # global_load_dwordx4 per 32-key unit: 4 of K (2 key tiles x 2 halves of d) and 4 of V (8 whole rows each)


def test_fp8_struct_mirror_matches_the_header():
    got, want = _layout(_capi.FaDecodeFp8Args, "fa_decode_fp8_args")
    assert got == want
    assert ctypes.sizeof(_capi.FaDecodeFp8Args) == ctypes.sizeof(_capi.FaDecodeArgs) + 3 * 8 + 8   # (kv_dtype and 4 bytes of padding)
    assert ctypes.sizeof(_capi.FaDecodeArgs) == 4 * 4 + 8 * 8 + 20 * 8
    lead = [f[0] for f in _capi.FaDecodeArgs._fields_]
    assert [f[0] for f in _capi.FaDecodeFp8Args._fields_][:len(lead)] == lead
    assert all(getattr(_capi.FaDecodeFp8Args, f).offset == getattr(_capi.FaDecodeArgs, f).offset for f in lead)


def test_fp8_symbols_abi_version_and_registry():
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
    """tests/test_decode_cpu.py's arguments with K / V strides in bytes and both descales.  Pointers are fake but aligned: no
    launch here reaches a device."""
    f = dict(dtype=15, q=16, k=16, v=16, o=16, lse=16, cache_seqlens=16, workspace=16, batch=batch, seqlen_q=Sq, n_heads=H, n_kv_heads=Hkv,
             q_batch_stride=Sq * H * 128, q_seq_stride=H * 128, q_head_stride=128,
             o_batch_stride=Sq * H * 128, o_seq_stride=H * 128, o_head_stride=128, kv_seq_stride=Hkv * 128, kv_head_stride=128,
             k_descale=16, v_descale=16, descale_batch_stride=Hkv)
    if paged:
        num_pages, page_size, per_seq = paged
        f.update(block_table=16, num_pages=num_pages, page_size=page_size, max_pages_per_seq=per_seq, block_table_stride=per_seq,
                 kv_batch_stride=page_size * Hkv * 128)
    else:
        f.update(seqlen_cache=cache, kv_batch_stride=cache * Hkv * 128)
    f.update(over)
    return _capi.make_decode_fp8_args(**f)


REFUSALS = [
    # the new rules: kv_dtype
    (dict(kv_dtype=0), -2, "kv_dtype"), (dict(kv_dtype=2), -2, "kv_dtype"), (dict(kv_dtype=-1), -2, "kv_dtype"),
    # ... K / V strides in bytes: multiples of 16 (8 passes the 16-bit path's rule), tensors 16-byte aligned
    (dict(kv_seq_stride=264), -5, "multiples of 16 bytes"), (dict(kv_head_stride=136), -5, "multiples of 16 bytes"),
    (dict(kv_batch_stride=4096 * 256 + 8), -5, "multiples of 16 bytes"), (dict(kv_seq_stride=260), -5, "kv strides"),
    (dict(k=8), -5, "16-byte aligned"), (dict(v=24), -5, "16-byte aligned"),
    # ... descales: 4-byte aligned, stride >= n_kv_heads
    (dict(k_descale=18), -5, "k_descale and v_descale must be 4-byte aligned"), (dict(v_descale=17), -5, "k_descale and v_descale must be 4-byte aligned"),
    (dict(descale_batch_stride=1), -4, "descale_batch_stride"), (dict(descale_batch_stride=0, v_descale=None), -4, "descale_batch_stride"),
    (dict(descale_batch_stride=-2, k_descale=None), -4, "descale_batch_stride"),
    (dict(struct_size=ctypes.sizeof(_capi.FaDecodeArgs)), -4, "fa_decode_fp8_args.struct_size"),
    # a sample of the inherited ones
    (dict(q=None), -1, "null tensor pointer"), (dict(k=None), -1, "null tensor pointer"), (dict(cache_seqlens=None), -1, "cache_seqlens is null"),
    (dict(batch=1, Hkv=1, workspace=None), -1, "workspace is null"),
    (dict(dtype=7), -2, "Only fp16 and bf16"),
    (dict(Sq=9, H=8, Hkv=1), -3, "64 packed query rows"), (dict(paged=(10, 32, 4)), -3, "multiple of 64"),
    (dict(d_head=64), -4, "d_head = 128"), (dict(H=8, Hkv=3), -4, "n_kv_heads"), (dict(cache=0), -4, "seqlen_cache"),
    (dict(paged=(10, 64, 4), block_table_stride=3), -4, "block_table_stride"), (dict(max_seqlen_k=4097), -4, "max_seqlen_k"),
    (dict(num_splits=1025), -4, "num_splits"), (dict(kv_seq_stride=0), -4, "kv strides"), (dict(q_seq_stride=0), -4, "q strides"),
    (dict(q_head_stride=132), -5, "q strides"), (dict(o=2), -5, "16-byte aligned"), (dict(cache_seqlens=18), -5, "4-byte aligned"),
    (dict(batch=1, Hkv=1, workspace=8), -5, "workspace must be 16-byte aligned"),
]


@pytest.mark.parametrize("over,status,text", REFUSALS, ids=[f"{i}:{s}" for i, (_, s, _) in enumerate(REFUSALS)])
def test_fp8_launch_refusals_without_a_device(over, status, text):
    lib = _capi.load()
    a = _args(**over)
    rc = lib.fa_decode_fp8_launch(ctypes.byref(a), None, None)
    assert rc == status, (rc, _capi.last_error())
    assert text in _capi.last_error()
    if status in (-2, -3):
        assert lib.fa_decode_fp8_supported(ctypes.byref(a)) == 0
    if status in (-2, -3, -4) or "strides" in text or "multiples of 16" in text:   # (refused by the queries too: no pointer's value is involved)
        assert lib.fa_decode_fp8_num_splits(ctypes.byref(a)) == status
        assert lib.fa_decode_fp8_workspace_bytes(ctypes.byref(a)) == status


def test_fp8_null_args_absent_descales_and_empty_batch():
    lib = _capi.load()
    assert lib.fa_decode_fp8_launch(None, None, None) == -1
    assert lib.fa_decode_fp8_supported(None) == 0
    ms = ctypes.c_float(-1.0)
    assert lib.fa_decode_fp8_launch(ctypes.byref(_args(batch=0, workspace=None)), None, ctypes.byref(ms)) == 0   # no device needed
    assert ms.value == 0.0
    for dtype in (5, 15):
        assert lib.fa_decode_fp8_supported(ctypes.byref(_args(dtype=dtype))) == 1
        assert lib.fa_decode_fp8_supported(ctypes.byref(_args(dtype=dtype, Sq=8, H=8, Hkv=1))) == 1     # 64 rows
        assert lib.fa_decode_fp8_supported(ctypes.byref(_args(dtype=dtype, paged=(100, 256, 7)))) == 1
    # either descale, or both, may be absent; the stride is then not looked at
    assert lib.fa_decode_fp8_supported(ctypes.byref(_args(k_descale=None))) == 1
    assert lib.fa_decode_fp8_supported(ctypes.byref(_args(v_descale=None))) == 1
    assert lib.fa_decode_fp8_supported(ctypes.byref(_args(k_descale=None, v_descale=None, descale_batch_stride=0))) == 1
    assert lib.fa_decode_fp8_supported(ctypes.byref(_args(descale_batch_stride=5))) == 1


@pytest.mark.parametrize("shape,want", SPLITS, ids=[str(i) for i in range(len(SPLITS))])
@pytest.mark.parametrize("paged", [False, True], ids=["contiguous", "paged"])
def test_fp8_split_rule_and_workspace_equal_the_16_bit_path(shape, want, paged):
    lib = _capi.load()
    batch, Sq, H, Hkv, cap, max_k, forced = shape
    kw = dict(batch=batch, Sq=Sq, H=H, Hkv=Hkv, max_seqlen_k=max_k, num_splits=forced)
    if paged:
        per_seq = (cap + 63) // 64
        kw["paged"] = (batch * per_seq + 1, 64, per_seq)
        kw["max_seqlen_k"] = max_k or cap
    else:
        kw["cache"] = cap
    a8, a16 = _args(**kw), _args16(**kw)
    assert lib.fa_decode_fp8_num_splits(ctypes.byref(a8)) == lib.fa_decode_num_splits(ctypes.byref(a16)) == want, _capi.last_error()
    assert lib.fa_decode_fp8_workspace_bytes(ctypes.byref(a8)) == lib.fa_decode_workspace_bytes(ctypes.byref(a16))


def test_fp8_slice_isa():
    assert os.path.exists(ISA), "the build keeps the fp8 decode slice's ISA (-save-temps=obj)"
    text = open(ISA).read()
    assert "global_load_dwordx4" in text and "ds_read_b64_tr_b16" in text
    assert "scratch_" not in text
    sizes = re.findall(r"\.amdhsa_private_segment_fixed_size (\d+)", text)
    assert sizes and all(s == "0" for s in sizes)
    assert all(s == "0" for s in re.findall(r"\.private_segment_fixed_size:\s+(\d+)", text))
    assert all(s == "0" for s in re.findall(r"\.vgpr_spill_count:\s+(\d+)", text))
    assert all(s == "0" for s in re.findall(r"\.sgpr_spill_count:\s+(\d+)", text))
    names = set(re.findall(r"^\s+\.name:\s+(_Z\w+)$", text, re.M))
    want = {f"_ZN2fa22fa_decode_split_kernelINS_13DecodeFp8ArgsELi{dt}ELi{nt}ELb{p}EEEvT_" for dt in (15, 5) for nt in (1, 2, 4) for p in (0, 1)}
    want |= {f"_ZN2fa24fa_decode_combine_kernelILi{dt}EEEvNS_10DecodeArgsE" for dt in (15, 5)}   # the 16-bit path's, from its header
    assert names == want, names ^ want
    kernels = _kernels(text)
    assert set(kernels) == want
    for name, body in kernels.items():   # each dtype's kernels convert to, and multiply in, that dtype only
        if "split_kernelINS_13DecodeFp8ArgsELi15E" in name:
            assert "v_mfma_f32_16x16x32_bf16" in body and "v_mfma_f32_16x16x32_f16" not in body
            assert "v_cvt_scalef32_pk_bf16_fp8" in body and "v_cvt_scalef32_pk_f16_fp8" not in body
        if "split_kernelINS_13DecodeFp8ArgsELi5E" in name:
            assert "v_mfma_f32_16x16x32_f16" in body and "v_mfma_f32_16x16x32_bf16" not in body
            assert "v_cvt_scalef32_pk_f16_fp8" in body and "v_cvt_scalef32_pk_bf16_fp8" not in body
        if "combine" in name:
            assert "v_cvt_scalef32" not in body and "v_mfma" not in body


def test_fp8_prefetch_stays_in_flight():
    """tests/test_decode_cpu.py's test_decode_prefetch_stays_in_flight with this path's load count: a 32-key unit is
    LOADS_PER_UNIT = 8 global_load_dwordx4 (K: 2 key tiles x 2 halves of d, 16 bytes per lane; V: 4 loads of 8 whole 128-byte
    rows).  In each half of the unrolled loop, between the prefetch's last load and the first transposed LDS read of the P V
    products, no wait goes below vmcnt(8): the next unit's K and V stay in flight under the current unit's conversions, products
    and softmax.  The 16- and 32-row forms, as there."""
    kernels = _kernels(open(ISA).read())
    checked = 0
    for name, body in kernels.items():
        if "split_kernel" not in name or "ELi4ELb" in name:
            continue
        halves = 0
        for block in re.split(r"^\.LBB\d+_\d+:", body, flags=re.M):
            ops = re.findall(r"^\s+(global_load_dwordx4|ds_read_b64_tr_b16|s_waitcnt[^\n]*vmcnt\((\d+)\))", block, re.M)
            kinds = [o[0].split()[0] for o in ops]
            if kinds.count("global_load_dwordx4") < LOADS_PER_UNIT or "ds_read_b64_tr_b16" not in kinds:
                continue
            last_load = max(i for i, k in enumerate(kinds) if k == "global_load_dwordx4")
            first_read = kinds.index("ds_read_b64_tr_b16")
            if first_read < last_load:
                continue
            waits = [int(o[1]) for o in ops[last_load:first_read] if o[1]]
            assert waits and min(waits) >= LOADS_PER_UNIT, (name, waits)
            halves += 1
        assert halves == 2, (name, halves)
        checked += 1
    assert checked == 8


def test_fp8_python_interface_is_exposed():
    import inspect

    import flash_attention
    import flash_attention_from_scratch_amd.flash_attention as inner
    from flash_attention_from_scratch_amd import flash_attention_kernels as fak

    assert flash_attention.quantize_kvcache_fp8 is inner.quantize_kvcache_fp8
    for fn in (flash_attention.forward_kvcache, fak.forward_kvcache):
        p = inspect.signature(fn).parameters
        assert p["k_descale"].default is None and p["v_descale"].default is None


# ---- quantize_kvcache_fp8 on the CPU -------------------------------------------------------------------------------------------

def _e4m3_step(x):
    """The spacing of e4m3fn around |x| (fp32 tensor): 2^(floor(log2 |x|) - 3) for normals, 2^-9 below 2^-6."""
    e = torch.floor(torch.log2(x.abs().clamp_min(2.0 ** -6)))
    return torch.exp2(e - 3)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
def test_quantize_round_trip(dtype):
    """|float(x8) * descale - x| <= half an e4m3 step at |x| / descale, times the head's descale; amax maps to 448."""
    import flash_attention

    gen = torch.Generator().manual_seed(0)
    k = (torch.randn((3, 70, 2, 128), generator=gen) * torch.tensor([0.01, 1.0, 30.0])[:, None, None, None]).to(dtype)
    v = torch.randn((3, 70, 2, 128), generator=gen).to(dtype)
    v[1, :, 0] = 0                    # an all-zero head
    v[2, 5, 1, 7] = 100.0             # an outlier that sets its head's scale
    k8, v8, kd, vd = flash_attention.quantize_kvcache_fp8(k, v)
    assert k8.dtype == v8.dtype == torch.float8_e4m3fn and k8.shape == k.shape and v8.shape == v.shape
    assert kd.dtype == vd.dtype == torch.float32 and tuple(kd.shape) == tuple(vd.shape) == (3, 2)
    for x, x8, d in ((k, k8, kd), (v, v8, vd)):
        x = x.float()
        amax = x.abs().amax(dim=(1, 3))
        assert torch.equal(d, torch.where(amax > 0, amax / 448.0, torch.ones_like(amax)))
        assert bool((d > 0).all()) and bool(torch.isfinite(d).all())
        scaled = x / d[:, None, :, None]
        err = (x8.float() - scaled).abs()
        assert bool((err <= 0.5 * _e4m3_step(scaled)).all()), err.max()
        # ... and in the cache's own units: half a step times the head's descale (and fp32's rounding of x / d and of x8 * d)
        back = x8.float() * d[:, None, :, None]
        assert bool(((back - x).abs() <= 0.5 * _e4m3_step(scaled) * d[:, None, :, None] + 2.0 ** -22 * x.abs()).all())
        assert bool(torch.equal(x8.float().abs().amax(dim=(1, 3)), torch.where(amax > 0, torch.full_like(amax, 448.0), torch.zeros_like(amax))))
        codes = x8.view(torch.uint8)
        assert not bool(((codes & 0x7F) == 0x7F).any())          # no NaN code from finite input
        assert bool(((codes & 0x7F) == 0)[x == 0].all())          # zeros stay zero
    assert vd[1, 0].item() == 1.0 and bool((v8[1, :, 0].view(torch.uint8) == 0).all())


def test_quantize_zeros_and_every_code_is_exact_in_16_bit():
    import flash_attention

    z = torch.zeros((2, 5, 3, 128), dtype=torch.bfloat16)
    k8, v8, kd, vd = flash_attention.quantize_kvcache_fp8(z, z)
    assert bool((k8.view(torch.uint8) == 0).all()) and bool((v8.view(torch.uint8) == 0).all())
    assert bool((kd == 1).all()) and bool((vd == 1).all())
    # what lets the kernel convert without an error of its own: every finite code is exact in bf16 and fp16
    codes = torch.arange(256, dtype=torch.uint8).view(torch.float8_e4m3fn).float()
    finite = torch.isfinite(codes)
    assert int((~finite).sum()) == 2
    for dtype in (torch.bfloat16, torch.float16):
        assert torch.equal(codes[finite].to(dtype).float(), codes[finite])
