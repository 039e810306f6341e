"""Grouped-query attention on the MI355X: the forward (fa_fwd_launch_gqa) against the LSE forward on K / V expanded with
repeat_interleave, bit for bit, and against fp32; the backward (fa_bwd_launch_gqa) with its split and unsplit dK / dV paths;
attention() end to end against torch SDPA's enable_gqa.

Gradient parity follows tests/test_backward_gpu.py (flash-attn's rule): against fp32 autograd of eager attention on the same
16-bit inputs (K / V expanded with repeat_interleave, so dK / dV sum the group), max|g - g32| <= 2 max|g_torch16 - g32| + 1e-4
and ||g - g32|| / ||g32|| <= 2 ||g_torch16 - g32|| / ||g32|| + 1e-3, with g_torch16 autograd of eager attention in the
16-bit dtype."""
import dataclasses

import pytest
import torch

import flash_attention
from flash_attention_from_scratch_amd import flash_attention_kernels as fak
from flash_helpers import kernel_configs as kc

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
DTYPES = {torch.bfloat16: kc.DType.BF16, torch.float16: kc.DType.FP16}
O_TOL = {torch.bfloat16: 2.0 ** -6, torch.float16: 2.0 ** -9}


@pytest.fixture(autouse=True)
def _no_tf32():
    old = torch.backends.cuda.matmul.allow_tf32
    torch.backends.cuda.matmul.allow_tf32 = False
    yield
    torch.backends.cuda.matmul.allow_tf32 = old


def _cfg(dtype, speculative=True):
    return dataclasses.replace(kc.best_config(DTYPES[dtype]), speculative_softmax=speculative, adaptive_softmax=False)


def _inputs(B, S, H, Hkv, dtype, seed=0, layout="plain"):
    gen = torch.Generator().manual_seed(seed)
    if layout == "packed":   # one (B, S, H + 2 Hkv, D) buffer: q, k, v are views with seq stride (H + 2 Hkv) 128
        buf = torch.randn((B, S, H + 2 * Hkv, 128), generator=gen).to(dtype).to(DEV)
        return buf[:, :, :H], buf[:, :, H:H + Hkv], buf[:, :, H + Hkv:]
    q = torch.randn((B, S, H, 128), generator=gen).to(dtype).to(DEV)
    if layout == "padded":   # K / V rows of 136 elements per head, the first 128 used: kv seq stride 136 Hkv (not % 128)
        kv = torch.randn((2, B, S, Hkv, 136), generator=gen).to(dtype).to(DEV)
        return q, kv[0][..., :128], kv[1][..., :128]
    return q, *(torch.randn((B, S, Hkv, 128), generator=gen).to(dtype).to(DEV) for _ in range(2))


def _expand(t, G):
    return t.repeat_interleave(G, dim=2).contiguous()


def _mask(S):
    return torch.ones((S, S), dtype=torch.bool, device=DEV).triu(1)


def _eager(q, k, v, causal, dtype):
    """softmax(q k^T / sqrt d) v in `dtype` with K / V expanded to q's heads, (B, S, H, D)"""
    G = q.shape[2] // k.shape[2]
    k, v = k.repeat_interleave(G, dim=2), v.repeat_interleave(G, dim=2)
    s = torch.einsum("bqhd,bkhd->bhqk", q.to(dtype), k.to(dtype)) / 128 ** 0.5
    if causal:
        s = s.masked_fill(_mask(q.shape[1]), float("-inf"))
    return torch.einsum("bhqk,bkhd->bqhd", torch.softmax(s, dim=-1), v.to(dtype))


def _ref_lse(q, k, causal):
    G = q.shape[2] // k.shape[2]
    s = torch.einsum("bqhd,bkhd->bhqk", q.float(), k.repeat_interleave(G, dim=2).float()) / 128 ** 0.5
    if causal:
        s = s.masked_fill(_mask(q.shape[1]), float("-inf"))
    return torch.logsumexp(s, dim=-1)


def _bits(x):
    return x.view(torch.int16) if x.dtype in (torch.bfloat16, torch.float16) else x.view(torch.int32)


def _same(a, b):
    return torch.equal(_bits(a), _bits(b))


# ---- forward ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", list(DTYPES))
@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("speculative", [True, False])
@pytest.mark.parametrize("shape", [(1, 256, 8), (2, 1024, 8), (1, 4096, 16)])
@pytest.mark.parametrize("div", [1, 2, 4, 0])   # Hkv = H / div; 0: MQA (Hkv = 1)
def test_gqa_forward_matches_expanded_kv_bit_for_bit(dtype, causal, speculative, shape, div):
    B, S, H = shape
    Hkv = 1 if div == 0 else H // div
    q, k, v = _inputs(B, S, H, Hkv, dtype, seed=S + H + Hkv)
    cfg = _cfg(dtype, speculative)
    o, lse = flash_attention.forward_ex(cfg, q, k, v, causal=causal, return_lse=True)
    o_m, lse_m = flash_attention.forward_ex(cfg, q, _expand(k, H // Hkv), _expand(v, H // Hkv), causal=causal, return_lse=True)
    torch.cuda.synchronize()
    assert o.shape == q.shape and lse.shape == (B, H, S)
    assert _same(o, o_m) and _same(lse, lse_m)
    assert (lse - _ref_lse(q, k, causal)).abs().max().item() <= 1e-3
    assert (o.float() - _eager(q.float(), k.float(), v.float(), causal, torch.float32)).abs().max().item() <= O_TOL[dtype]
    # without return_lse: the same O
    assert _same(flash_attention.forward_ex(cfg, q, k, v, causal=causal), o)


@pytest.mark.parametrize("dtype", list(DTYPES))
@pytest.mark.parametrize("layout", ["packed", "padded"])
@pytest.mark.parametrize("causal", [False, True])
def test_gqa_forward_kv_layouts(dtype, layout, causal):
    B, S, H, Hkv = 2, 1024, 8, 2
    q, k, v = _inputs(B, S, H, Hkv, dtype, seed=5, layout=layout)
    assert k.stride(1) == (H + 2 * Hkv) * 128 if layout == "packed" else k.stride(1) == 136 * Hkv
    cfg = _cfg(dtype)
    o, lse = flash_attention.forward_ex(cfg, q, k, v, causal=causal, return_lse=True)
    o_c, lse_c = flash_attention.forward_ex(cfg, q.contiguous(), k.contiguous(), v.contiguous(), causal=causal, return_lse=True)
    torch.cuda.synchronize()
    assert _same(o, o_c) and _same(lse, lse_c)


@pytest.mark.parametrize("dtype", list(DTYPES))
@pytest.mark.parametrize("entry", ["plain", "masked"])
def test_gqa_forward_on_items_the_speculative_pass_redoes(dtype, entry):
    """A key of K / V head 0 aligned with one query row of head 0 at 8x its size: that row's logit rises ~130 binades above
    its first tile's max, the speculative first pass fails the items of query heads 0 .. G-1 that see it, and the second pass
    redoes them (the plain form as 128-row halves) -- through the same K / V head: O and lse stay bit-identical to the
    expanded launch, and lse is within 1e-3 + 2e-6 |lse| of fp64."""
    B, S, H, Hkv = 1, 1024, 4, 2
    q, k, v = _inputs(B, S, H, Hkv, dtype, seed=9)
    k[0, 700, 0] = (8 * q[0, 300, 0].float()).to(dtype)
    cfg = _cfg(dtype, True)
    stats = torch.zeros(2, dtype=torch.int32, device=DEV)
    if entry == "plain":
        o, lse, _ = fak.forward_lse(cfg, q, k, v, stats=stats)
        o_m, lse_m, _ = fak.forward_lse(cfg, q, _expand(k, 2), _expand(v, 2))
    else:
        o, lse = flash_attention.forward_ex(cfg, q, k, v, return_lse=True, stats=stats)
        o_m, lse_m = flash_attention.forward_ex(cfg, q, _expand(k, 2), _expand(v, 2), return_lse=True)
    torch.cuda.synchronize()
    assert stats[1].item() > 0
    assert _same(o, o_m) and _same(lse, lse_m)
    ref = torch.logsumexp(torch.einsum("bqhd,bkhd->bhqk", q.double(), k.repeat_interleave(2, dim=2).double()) / 128 ** 0.5, dim=-1)
    assert ((lse.double() - ref).abs() <= 1e-3 + 2e-6 * ref.abs()).all()


def test_forward_keeps_the_reference_same_shape_error():
    q, k, v = _inputs(1, 256, 4, 2, torch.bfloat16)
    with pytest.raises(RuntimeError, match="same shape"):
        flash_attention.forward(kc.best_config(kc.DType.BF16), q, k, v)


def test_gqa_forward_other_configurations_are_refused():
    q, k, v = _inputs(1, 256, 4, 2, torch.bfloat16)
    ring = [c for c in kc.get_all_supported_configs() if c.dtype == kc.DType.BF16 and c.d_head == 128 and c.B_r == 128
            and c.B_c == 64 and c.n_warps == 4 and c.mma_double_buffer_loads][0]
    with pytest.raises(RuntimeError, match="grouped-query attention"):
        flash_attention.forward_ex(ring, q, k, v)


# ---- backward --------------------------------------------------------------------------------------------------------

def _grads(q, k, v, dout, causal, dtype):
    leaves = [t.detach().to(dtype).requires_grad_(True) for t in (q, k, v)]
    _eager(*leaves, causal, dtype).backward(dout.to(dtype))
    return [t.grad.float() for t in leaves]


def _check_parity(got, q, k, v, dout, causal, dtype):
    g32 = _grads(q, k, v, dout, causal, torch.float32)
    g16 = _grads(q, k, v, dout, causal, dtype)
    for name, g, r32, r16 in zip(("dq", "dk", "dv"), got, g32, g16):
        g = g.float()
        assert g.shape == r32.shape, name
        assert torch.isfinite(g).all(), name
        bound = 2 * (r16 - r32).abs().max().item() + 1e-4
        err = (g - r32).abs().max().item()
        assert err <= bound, (name, err, bound)
        rel = ((g - r32).norm() / r32.norm()).item()
        rel16 = ((r16 - r32).norm() / r32.norm()).item()
        assert rel <= 2 * rel16 + 1e-3, (name, rel, rel16)


def _torch_o_lse(q, k, v, causal, dtype):
    return _eager(q.float(), k.float(), v.float(), causal, torch.float32).to(dtype).contiguous(), _ref_lse(q, k, causal).contiguous()


# (B, S, H, Hkv): the dK / dV split (fa_capi.hip, bwd_gqa_split) is 8 / 8 at (1, 1024, 8, 1), 1 / 2 at (8, 2048, 4, 2)
# (256 workgroups plain; causal asks for 1024), 2 / 2 at (2, 512, 4, 2) -- both paths, both masks
@pytest.mark.parametrize("dtype", list(DTYPES))
@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("shape,layout", [((1, 1024, 8, 1), "plain"), ((8, 2048, 4, 2), "plain"), ((2, 512, 4, 2), "padded"),
                                          ((2, 512, 6, 3), "packed")])
def test_gqa_backward(dtype, causal, shape, layout):
    B, S, H, Hkv = shape
    G = H // Hkv
    q, k, v = _inputs(B, S, H, Hkv, dtype, seed=7 * S + H + Hkv, layout=layout)
    dout = torch.randn((B, S, H, 128), generator=torch.Generator().manual_seed(S)).to(dtype).to(DEV)
    o, lse = _torch_o_lse(q, k, v, causal, dtype)
    dq, dk, dv = flash_attention.backward(q, k, v, o, lse, dout, causal=causal)
    # (the MHA backward wants one stride set for q, k, v: q contiguous like the expanded K / V)
    dq_m, _, _ = flash_attention.backward(q.contiguous(), _expand(k, G), _expand(v, G), o, lse, dout, causal=causal)
    again = flash_attention.backward(q, k, v, o, lse, dout, causal=causal)
    torch.cuda.synchronize()
    assert dq.shape == q.shape and dk.shape == k.shape and dv.shape == v.shape
    assert all(g.dtype == dtype and g.is_contiguous() for g in (dq, dk, dv))
    assert _same(dq, dq_m)
    for x, y in zip((dq, dk, dv), again):   # run to run: the same bits
        assert _same(x, y)
    _check_parity((dq, dk, dv), q, k, v, dout, causal, dtype)


@pytest.mark.parametrize("dtype", list(DTYPES))
@pytest.mark.parametrize("causal", [False, True])
def test_attention_with_gqa_matches_sdpa(dtype, causal):
    B, S, H, Hkv = 2, 1024, 8, 2
    q, k, v = _inputs(B, S, H, Hkv, dtype, seed=11)
    g = torch.randn((B, S, H, 128), generator=torch.Generator().manual_seed(5)).to(dtype).to(DEV)
    leaves = [t.clone().requires_grad_(True) for t in (q, k, v)]
    out = flash_attention.attention(*leaves, causal=causal)
    out.backward(g)
    ref = [t.detach().float().transpose(1, 2).requires_grad_(True) for t in (q, k, v)]
    o32 = torch.nn.functional.scaled_dot_product_attention(*ref, is_causal=causal, enable_gqa=True)
    o32.backward(g.float().transpose(1, 2))
    o16 = _eager(q, k, v, causal, dtype).float()
    o32 = o32.detach().transpose(1, 2)
    assert (out.detach().float() - o32).abs().max().item() <= 2 * (o16 - o32).abs().max().item() + 1e-4
    g16 = _grads(q, k, v, g, causal, dtype)
    for name, leaf, r, r16 in zip(("dq", "dk", "dv"), leaves, ref, g16):
        r32 = r.grad.transpose(1, 2)
        assert leaf.grad.shape == leaf.shape, name
        err = (leaf.grad.float() - r32).abs().max().item()
        assert err <= 2 * (r16 - r32).abs().max().item() + 1e-4, (name, err)
