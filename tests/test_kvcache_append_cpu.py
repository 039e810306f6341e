"""The KV-cache append without a device: the C ABI of fa_kvcache_append_launch (struct layout, exports,
validation before any HIP call), the Python signatures and argument errors, the ISA the build keeps for the slice, and the
torch reference of tests/kvcache_append_ref.py against hand-checked rows."""
import ctypes
import inspect
import os
import re
import subprocess

import pytest
import torch

from flash_attention_from_scratch_amd import _capi
from tests import kvcache_append_ref as ref
from tests.conftest import ROOT
from tests.test_decode_cpu import _kernels
from tests.test_varlen_cpu import _layout

BUILD = os.path.join(ROOT, "flash_attention_from_scratch_amd", "csrc", "build")
ISA = os.path.join(BUILD, "kvcache_append", "fa_kvcache_append-hip-amdgcn-amd-amdhsa-gfx950.s")
JITTER = os.path.join(ROOT, "flash_attention_from_scratch_amd", "lib", "libfa_hip_jitter.so")


def test_struct_mirror_matches_the_header():
    got, want = _layout(_capi.FaKvcacheAppendArgs, "fa_kvcache_append_args")
    assert got == want
    assert ctypes.sizeof(_capi.FaKvcacheAppendArgs) == 5 * 4 + 4 + 13 * 8 + 27 * 8   # (4 bytes of padding behind the five int32)
    assert _capi.FaKvcacheAppendArgs.struct_size.offset == 0


def test_symbol_is_exported_by_both_libraries():
    assert "fa_kvcache_append_launch" in _capi.EXPORTED_SYMBOLS
    for path in (_capi.LIB_PATH, JITTER):
        nm = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True)
        assert "fa_kvcache_append_launch" in set(re.findall(r" T (fa_[a-z_0-9]+)", nm.stdout)), path
    assert _capi.load().fa_abi_version() == 6


def _args(batch=3, Sn=1, Sq=1, H=8, Hkv=2, cache=256, paged=None, rotary=64, with_q=True, fp8=False, **over):
    """Pointers are fake but aligned: no launch here reaches a device."""
    f = dict(dtype=15, kv_dtype=1 if fp8 else 0, k_new=16, v_new=32, k=48, v=64, cache_seqlens=16, seqlens_out=16,
             batch=batch, seqlen_new=Sn, n_kv_heads=Hkv, new_batch_stride=Sn * Hkv * 128, new_seq_stride=Hkv * 128, new_head_stride=128,
             kv_seq_stride=Hkv * 128, kv_head_stride=128)
    if paged:
        num_pages, page_size, per_seq = paged
        f.update(block_table=16, num_pages=num_pages, page_size=page_size, max_pages_per_seq=per_seq, block_table_stride=per_seq,
                 kv_batch_stride=page_size * Hkv * 128)
    else:
        f.update(seqlen_cache=cache, kv_batch_stride=cache * Hkv * 128)
    if rotary:
        f.update(rotary_cos=16, rotary_sin=16, rotary_dim=rotary, seqlen_ro=cache, rotary_seq_stride=rotary // 2)
    if with_q and rotary:
        n = batch * Sq * H * 128 * 2
        f.update(q=1 << 20, q_out=(1 << 20) + n, seqlen_q=Sq, n_heads=H,
                 q_batch_stride=Sq * H * 128, q_seq_stride=H * 128, q_head_stride=128,
                 qo_batch_stride=Sq * H * 128, qo_seq_stride=H * 128, qo_head_stride=128)
    if fp8:
        f.update(k_descale=16, v_descale=16, descale_batch_stride=Hkv)
    f.update(over)
    return _capi.make_kvcache_append_args(**f)


Q0 = 1 << 20
REFUSALS = [
    # nulls
    (dict(k=None), -1, "null cache pointer"), (dict(v=None), -1, "null cache pointer"),
    (dict(k_new=None), -1, "null new-row pointer"), (dict(v_new=None), -1, "null new-row pointer"),
    (dict(cache_seqlens=None), -1, "cache_seqlens or seqlens_out is null"), (dict(seqlens_out=None), -1, "cache_seqlens or seqlens_out is null"),
    (dict(q_out=None), -1, "q_out is null"),
    # dtype / kv_dtype
    (dict(dtype=7), -2, "Only fp16 and bf16"), (dict(dtype=0), -2, "Only fp16 and bf16"),
    (dict(kv_dtype=2), -2, "kv_dtype"), (dict(kv_dtype=-1), -2, "kv_dtype"),
    # page size
    (dict(paged=(12, 32, 4)), -3, "multiple of 64"), (dict(paged=(12, 96, 4)), -3, "multiple of 64"),
    # sizes
    (dict(struct_size=8), -4, "fa_kvcache_append_args.struct_size"), (dict(d_head=64), -4, "d_head = 128"),
    (dict(batch=-1), -4, "must not be negative"), (dict(Sn=-1), -4, "must not be negative"), (dict(Hkv=0), -4, "n_kv_heads must be positive"),
    (dict(cache=0, seqlen_ro=4), -4, "seqlen_cache"), (dict(paged=(0, 64, 4)), -4, "paged cache"),
    (dict(paged=(12, 64, 4), block_table_stride=3), -4, "block_table_stride"), (dict(Sq=0), -4, "seqlen_q and n_heads"),
    (dict(n_heads=0), -4, "seqlen_q and n_heads"),
    # strides not positive
    (dict(new_seq_stride=0), -4, "new strides"), (dict(new_head_stride=0), -4, "new strides"), (dict(new_batch_stride=-8), -4, "new strides"),
    (dict(kv_seq_stride=0), -4, "kv strides"), (dict(kv_batch_stride=0), -4, "kv strides"), (dict(q_seq_stride=0), -4, "q strides"),
    (dict(qo_head_stride=0), -4, "q_out strides"),
    # rotary
    (dict(rotary_dim=24), -4, "rotary_dim"), (dict(rotary_dim=0), -4, "rotary_dim"), (dict(rotary_dim=144), -4, "rotary_dim"),
    (dict(rotary_dim=8), -4, "rotary_dim"), (dict(rotary_sin=None), -4, "come together"), (dict(rotary_cos=None), -4, "come together"),
    (dict(seqlen_ro=0), -4, "seqlen_ro"), (dict(rotary_seq_stride=16), -4, "rotary_seq_stride"),
    (dict(rotary=0, q=Q0, q_out=Q0 * 2), -4, "without rotary tables"),
    # q_out overlapping q (the same tensor, half way in, and the last 16 bytes)
    (dict(q_out=Q0), -4, "overlaps"), (dict(q_out=Q0 + 3 * 8 * 128), -4, "overlaps"), (dict(q_out=Q0 - 3 * 8 * 128 * 2 + 16), -4, "overlaps"),
    # descales
    (dict(k_descale=16), -4, "belong to an fp8 cache"), (dict(v_descale=16), -4, "belong to an fp8 cache"),
    (dict(fp8=True, descale_batch_stride=1), -4, "descale_batch_stride"),
    # alignment
    (dict(new_seq_stride=260), -5, "new strides"), (dict(kv_head_stride=132), -5, "kv strides"), (dict(q_batch_stride=8 * 128 + 4), -5, "q strides"),
    (dict(qo_seq_stride=8 * 128 + 2), -5, "q_out strides"), (dict(fp8=True, kv_seq_stride=264), -5, "kv strides"),
    (dict(rotary_seq_stride=36), -5, "rotary_seq_stride"),
    (dict(k=56), -5, "16-byte aligned"), (dict(v_new=8), -5, "16-byte aligned"), (dict(q=Q0 - 4096 + 2), -5, "16-byte aligned"),
    (dict(rotary_cos=24), -5, "16-byte aligned"), (dict(cache_seqlens=18), -5, "4-byte aligned"), (dict(seqlens_out=17), -5, "4-byte aligned"),
    (dict(paged=(12, 64, 4), block_table=6), -5, "4-byte aligned"), (dict(fp8=True, k_descale=2), -5, "4-byte aligned"),
]


@pytest.mark.parametrize("over,status,text", REFUSALS, ids=[f"{i}:{s}" for i, (_, s, _) in enumerate(REFUSALS)])
def test_launch_refusals_without_a_device(over, status, text):
    lib = _capi.load()
    a = _args(**over)
    rc = lib.fa_kvcache_append_launch(ctypes.byref(a), None, None)
    assert rc == status, (rc, _capi.last_error())
    assert text in _capi.last_error()


def test_null_args_and_empty_batch():
    lib = _capi.load()
    assert lib.fa_kvcache_append_launch(None, None, None) == -1
    for kw in (dict(), dict(fp8=True), dict(paged=(12, 64, 4)), dict(rotary=0, with_q=False), dict(Sn=0, k_new=None, v_new=None), dict(dtype=5)):
        ms = ctypes.c_float(-1.0)
        assert lib.fa_kvcache_append_launch(ctypes.byref(_args(batch=0, **kw)), None, ctypes.byref(ms)) == 0, _capi.last_error()   # no device needed
        assert ms.value == 0.0


def test_python_interface():
    import flash_attention
    import flash_attention_from_scratch_amd.flash_attention as inner
    from flash_attention_from_scratch_amd import flash_attention_kernels as fak

    assert flash_attention.append_kvcache is inner.append_kvcache
    for fn in (flash_attention.append_kvcache, fak.append_kvcache):
        p = inspect.signature(fn).parameters
        assert list(p) == ["k_cache", "v_cache", "k", "v", "cache_seqlens", "block_table", "q", "rotary_cos", "rotary_sin",
                           "rotary_interleaved", "causal", "k_descale", "v_descale", "seqlens_out"]
        assert all(p[n].default is None for n in ("block_table", "q", "rotary_cos", "rotary_sin", "k_descale", "v_descale", "seqlens_out"))
        assert p["rotary_interleaved"].default is False and p["causal"].default is False
    for fn in (flash_attention.forward_kvcache, fak.forward_kvcache):
        p = inspect.signature(fn).parameters
        assert list(p)[-6:] == ["k", "v", "rotary_cos", "rotary_sin", "rotary_interleaved", "advance_seqlens"]
        assert list(p)[:12] == ["q", "k_cache", "v_cache", "cache_seqlens", "block_table", "causal", "return_lse", "max_seqlen_k",
                                "num_splits", "timed", "k_descale", "v_descale"]
        assert all(p[n].default is None for n in ("k", "v", "rotary_cos", "rotary_sin"))
        assert p["rotary_interleaved"].default is False and p["advance_seqlens"].default is False


def test_python_argument_errors():
    """Raised before any launch (CPU tensors would be refused next: none of these gets that far, or that refusal is the point)."""
    import flash_attention

    q = torch.zeros((2, 1, 8, 128), dtype=torch.bfloat16)
    kc = torch.zeros((2, 64, 2, 128), dtype=torch.bfloat16)
    k = torch.zeros((2, 1, 2, 128), dtype=torch.bfloat16)
    lens = torch.zeros(2, dtype=torch.int32)
    cos = torch.zeros((64, 32), dtype=torch.bfloat16)
    with pytest.raises(RuntimeError, match="k and v come together"):
        flash_attention.forward_kvcache(q, kc, kc, lens, rotary_cos=cos, rotary_sin=cos)      # rotary without k / v
    with pytest.raises(RuntimeError, match="k and v come together"):
        flash_attention.forward_kvcache(q, kc, kc, lens, k=k)                                  # k without v
    with pytest.raises(RuntimeError, match="k and v come together"):
        flash_attention.forward_kvcache(q, kc, kc, lens, advance_seqlens=True)
    with pytest.raises(RuntimeError, match="seqlen_new == seqlen_q"):
        flash_attention.forward_kvcache(q, kc, kc, lens, causal=True, k=k.expand(2, 3, 2, 128), v=k.expand(2, 3, 2, 128), rotary_cos=cos, rotary_sin=cos)
    with pytest.raises(RuntimeError, match="come together"):
        flash_attention.append_kvcache(kc, kc, k, k, lens, rotary_cos=cos)
    with pytest.raises(RuntimeError, match="without rotary_cos"):
        flash_attention.append_kvcache(kc, kc, k, k, lens, q=q)
    with pytest.raises(RuntimeError, match="CUDA tensor"):                                    # no fallback for CPU tensors
        flash_attention.append_kvcache(kc, kc, k, k, lens)


def test_slice_isa():
    assert os.path.exists(ISA), "the build keeps the append slice's ISA (-save-temps=obj)"
    text = open(ISA).read()
    assert "global_load_dwordx4" in text and "global_store_dwordx4" in text
    assert "scratch_" not in text
    sizes = re.findall(r"\.amdhsa_private_segment_fixed_size (\d+)", text)
    assert sizes and all(s == "0" for s in sizes)
    fixed = re.findall(r"\.private_segment_fixed_size:\s+(\d+)", text)
    assert len(fixed) == 4 and all(s == "0" for s in fixed)
    assert all(s == "0" for s in re.findall(r"\.vgpr_spill_count:\s+(\d+)", text))
    # (the fp8 forms keep about ten of their ~70 scalar arguments in VGPR lanes: v_writelane / v_readlane, not memory)
    assert all(int(s) <= 16 for s in re.findall(r"\.sgpr_spill_count:\s+(\d+)", text))
    names = set(re.findall(r"^\s+\.name:\s+(_Z\w+)$", text, re.M))
    want = {f"_ZN2fa24fa_kvcache_append_kernelILi{dt}ELb{f}EEEvNS_10AppendArgsE" for dt in (15, 5) for f in (0, 1)}
    assert names == want, names ^ want
    kernels = _kernels(text)
    assert set(kernels) == want
    for name, body in kernels.items():
        assert "s_barrier" in body                                       # the lengths' store waits for every thread's read
        assert "global_atomic" not in body and not re.search(r"^\s+ds_", body, re.M)   # no atomics, no LDS
        if "ELb0E" in name:                                              # the rotary arithmetic: nothing fused (the fp8 form's division has FMAs of its own)
            assert not re.search(r"v_(pk_)?(fma|fmac|mad|mac)_f32", body)
        assert ("v_div_scale_f32" in body) == ("ELb1E" in name)          # IEEE division only where there is an fp8 cache


# ---- the reference itself, on the CPU, against rows worked out by hand --------------------------------------------------------

def _tables(seqlen_ro, half, dtype):
    """Row p: cos = 0.5, sin = 0.25 -- except row 2: cos = 0, sin = 1 (a quarter turn), and row 5: cos = 1, sin = 0 (identity)."""
    cos = torch.full((seqlen_ro, half), 0.5).to(dtype)
    sin = torch.full((seqlen_ro, half), 0.25).to(dtype)
    cos[2], sin[2] = 0.0, 1.0
    if seqlen_ro > 5:
        cos[5], sin[5] = 1.0, 0.0
    return cos, sin


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
def test_reference_rotary_by_hand(dtype):
    x = torch.zeros((1, 1, 128), dtype=dtype)
    x[0, 0, :8] = torch.tensor([2.0, 4.0, 6.0, 8.0, 1.0, 3.0, 5.0, 7.0]).to(dtype)
    x[0, 0, 8:] = 9.0
    cos, sin = _tables(8, 4, dtype)                # rotary_dim 8 here: the reference takes any even dimension
    # non-interleaved: pairs (0, 4), (1, 5), (2, 6), (3, 7); c = 0.5, s = 0.25: o1 = 0.5 x1 - 0.25 x2, o2 = 0.25 x1 + 0.5 x2
    got = ref.rotary_ref(x, cos, sin, [0], False)[0, 0]
    assert got[:8].float().tolist() == [0.75, 1.25, 1.75, 2.25, 1.0, 2.5, 4.0, 5.5]
    assert bool((got[8:] == 9).all())              # beyond rotary_dim: unchanged
    # interleaved: pairs (0, 1), (2, 3), (4, 5), (6, 7)
    got = ref.rotary_ref(x, cos, sin, [0], True)[0, 0]
    assert got[:8].float().tolist() == [0.0, 2.5, 1.0, 5.5, -0.25, 1.75, 0.75, 4.75]
    # a quarter turn (row 2): o1 = -x2, o2 = x1; the identity (row 5)
    got = ref.rotary_ref(x, cos, sin, [2], False)[0, 0]
    assert got[:8].float().tolist() == [-1.0, -3.0, -5.0, -7.0, 2.0, 4.0, 6.0, 8.0]
    assert torch.equal(ref.rotary_ref(x, cos, sin, [5], True), x)
    # rounded once: 3 * 0.3333 (bf16 / fp16 of 1/3) is not representable -- the result is the 16-bit rounding of the fp32 sum
    c = torch.full((1, 4), 1.0 / 3.0).to(dtype)
    s = torch.full((1, 4), 1.0 / 7.0).to(dtype)
    got = ref.rotary_ref(x, c, s, [0], False)[0, 0]
    want0 = (torch.tensor(2.0) * c[0, 0].float() - torch.tensor(1.0) * s[0, 0].float()).to(dtype)
    assert got[0] == want0 and got[0].float() != 2.0 * c[0, 0].float() - s[0, 0].float()


def test_reference_positions_by_hand():
    """Keys: position len + t, clamped to the last table row.  q: len + i with causal, len without (flash-attn's rule)."""
    assert ref.q_rows(10, 3, True, 64) == [10, 11, 12]
    assert ref.q_rows(10, 3, False, 64) == [10, 10, 10]
    assert ref.q_rows(62, 3, True, 64) == [62, 63, 63]
    assert ref.q_rows(100, 2, False, 64) == [63, 63]
    dtype = torch.bfloat16
    cos, sin = _tables(4, 8, dtype)                # rotary_dim 16, seqlen_ro 4: positions >= 3 use row 3
    kc = torch.zeros((2, 8, 1, 128), dtype=dtype)
    k = torch.zeros((2, 2, 1, 128), dtype=dtype)
    k[..., :8], k[..., 8:16] = 2.0, 4.0
    q = k.clone()
    # entry 0: len 1 -> keys at positions 1 (row 1: c .5 s .25) and 2 (row 2: quarter turn); entry 1: len 7 -> one key fits, row 3
    kc2, vc2, lens, q_rot = ref.append_ref(kc, kc, k, k, [1, 7], q=q, cos=cos, sin=sin, causal=True)
    assert lens == [3, 8]
    assert kc2[0, 1, 0, :16].float().tolist() == [0.0] * 8 + [2.5] * 8          # 1 - 1, 0.5 + 2
    assert kc2[0, 2, 0, :16].float().tolist() == [-4.0] * 8 + [2.0] * 8         # -x2, x1
    assert kc2[1, 7, 0, :16].float().tolist() == [0.0] * 8 + [2.5] * 8
    assert torch.equal(vc2[0, 1:3], k[0]) and torch.equal(vc2[1, 7], k[1, 0])   # V is never rotated
    assert int((kc2 != 0).any(dim=-1).sum()) == 3 and int((vc2 != 0).any(dim=-1).sum()) == 3   # the dropped token went nowhere
    assert q_rot[0, 0, 0, :16].float().tolist() == [0.0] * 8 + [2.5] * 8 and q_rot[0, 1, 0, :16].float().tolist() == [-4.0] * 8 + [2.0] * 8
    _, _, _, q_rot = ref.append_ref(kc, kc, k, k, [2, 7], q=q, cos=cos, sin=sin, causal=False)
    assert q_rot[0, 0, 0, :16].float().tolist() == q_rot[0, 1, 0, :16].float().tolist() == [-4.0] * 8 + [2.0] * 8   # both rows at len = 2
    # clamps of len: negative is 0, beyond the capacity writes nothing
    kc2, _, lens, _ = ref.append_ref(kc, kc, k, k, [-5, 10 ** 6])
    assert lens == [2, 8] and torch.equal(kc2[0, :2], k[0]) and not bool(kc2[1].any())
    # paged: entries beyond the pool are clamped into it
    pages = torch.zeros((3, 4, 1, 128), dtype=dtype)
    table = torch.tensor([[9, 1], [-3, 2]], dtype=torch.int32)
    kc2, _, lens, _ = ref.append_ref(pages, pages, k, k, [0, 3], block_table=table)
    assert lens == [2, 5]
    assert torch.equal(kc2[2, :2], k[0]) and torch.equal(kc2[0, 3], k[1, 0]) and torch.equal(kc2[2, 0], k[1, 1])   # (two entries on page 2: the test's own abuse)


def test_reference_quantization_by_hand():
    """e4m3fn(clamp(x / descale, -448, 448)), round to nearest even: 1.0 = 0x38, steps of 1/8 up to 2."""
    x = torch.zeros((1, 2, 128), dtype=torch.bfloat16)
    x[0, 0, :8] = torch.tensor([3.0, 2.125, 2.375, 1000.0, -1000.0, 2.0 ** -9, 2.0 ** -10, float("nan")]).to(torch.bfloat16)
    x[0, 1, :4] = torch.tensor([1.5, 1.0625, 1.1875, -0.75]).to(torch.bfloat16)
    d = torch.tensor([2.0, 1.0])
    got = ref.quantize_ref(x, d).view(torch.uint8)
    # head 0, descale 2: 1.5 -> 0x3c; 1.0625 is a tie between 1.0 (0x38) and 1.125 (0x39) -> even 0x38; 1.1875 a tie between 0x39
    # and 0x3a -> 0x3a; 500 saturates at 448 = 0x7e; 2^-10 is half the smallest subnormal 2^-9 = 0x01 -> a tie -> even 0x00;
    # 2^-11 rounds to 0; NaN stays NaN
    assert got[0, 0, :7].tolist() == [0x3C, 0x38, 0x3A, 0x7E, 0xFE, 0x00, 0x00]
    assert got[0, 0, 7].item() & 0x7F == 0x7F       # (either NaN code: the sign of a NaN behind clamp() is the torch backend's)
    assert got[0, 1, :4].tolist() == [0x3C, 0x38, 0x3A, 0xB4]
    assert got[0, 0, 8:].tolist() == [0] * 120
    # no descale = 1, and the whole expression is quantize_kvcache_fp8's with its own descale
    import flash_attention
    assert torch.equal(ref.quantize_ref(x[:, 1:], None).view(torch.uint8), got[:, 1:])
    gen = torch.Generator().manual_seed(1)
    k = torch.randn((2, 5, 3, 128), generator=gen).to(torch.float16)
    k8, _, kd, _ = flash_attention.quantize_kvcache_fp8(k, k)
    for b in range(2):
        assert torch.equal(ref.quantize_ref(k[b], kd[b]).view(torch.uint8), k8[b].view(torch.uint8))
