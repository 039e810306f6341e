"""The training path on the MI355X: the forward's row log-sum-exp, the HIP backward and the autograd Function.

Gradient parity follows flash-attn's rule: against fp32 autograd of eager attention computed from the same 16-bit inputs,
max|g - g32| <= 2 max|g_torch16 - g32| + 1e-4 for each of dQ, dK, dV, where g_torch16 is autograd of eager attention in the
16-bit dtype; and ||g - g32|| / ||g32|| <= 2 ||g_torch16 - g32|| / ||g32|| + 1e-3 (relative L2)."""
import dataclasses

import pytest
import torch

import flash_attention
from flash_attention_from_scratch_amd import flash_attention_kernels as fak
from flash_helpers import kernel_configs as kc
from tests.conftest import load_seam_golden

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
DTYPES = {torch.bfloat16: kc.DType.BF16, torch.float16: kc.DType.FP16}


def _cfg(dtype, speculative=True):
    return dataclasses.replace(kc.best_config(DTYPES[dtype]), speculative_softmax=speculative, adaptive_softmax=False)


def _inputs(B, S, H, dtype, seed=0, layout="plain"):
    gen = torch.Generator().manual_seed(seed)
    if layout == "packed":   # (B, S, 3, H, D): qkv_seq_stride = 3 H 128
        qkv = torch.randn((B, S, 3, H, 128), generator=gen).to(dtype).to(DEV)
        return qkv[:, :, 0], qkv[:, :, 1], qkv[:, :, 2]
    if layout == "padded":   # qkv_seq_stride = 136 H: each row of a (B, S, H, 136) buffer, the first 128 used
        buf = torch.randn((3, B, S, H * 136), generator=gen).to(dtype).to(DEV)
        return tuple(buf[i].view(B, S, H, 136)[..., :128] for i in range(3))
    return tuple(torch.randn((B, S, H, 128), generator=gen).to(dtype).to(DEV) for _ in range(3))


def _scores(q, k):
    return torch.einsum("bqhd,bkhd->bhqk", q.float(), k.float()) / 128 ** 0.5


def _causal_mask(S):
    return torch.ones((S, S), dtype=torch.bool, device=DEV).triu(1)


def _eager(q, k, v, causal, dtype):
    """softmax(q k^T / sqrt d) v in `dtype` (materialised S), (B, S, H, D)"""
    s = torch.einsum("bqhd,bkhd->bhqk", q.to(dtype), k.to(dtype)) / 128 ** 0.5
    if causal:
        s = s.masked_fill(_causal_mask(q.shape[1]), float("-inf"))
    p = torch.softmax(s, dim=-1)
    return torch.einsum("bhqk,bkhd->bqhd", p, v.to(dtype))


def _ref_lse(q, k, causal):
    s = _scores(q, k)
    if causal:
        s = s.masked_fill(_causal_mask(q.shape[1]), float("-inf"))
    return torch.logsumexp(s, dim=-1)


def _grads(q, k, v, dout, causal, dtype):
    leaves = [t.detach().to(dtype).requires_grad_(True) for t in (q, k, v)]
    _eager(*leaves, causal, dtype).backward(dout.to(dtype))
    return [t.grad.float() for t in leaves]


@pytest.fixture(autouse=True)
def _no_tf32():
    old = torch.backends.cuda.matmul.allow_tf32
    torch.backends.cuda.matmul.allow_tf32 = False
    yield
    torch.backends.cuda.matmul.allow_tf32 = old


def _forward(cfg, q, k, v, causal, entry, lse, stats=None):
    """entry "plain": flash_attention_kernels.forward / forward_lse with allow_ragged=False -- without the mask the plain
    device forms (fa_fwd_kernel64<DT, false, ...> and its LSE twin, whose speculative second pass redoes a failed item as
    128-row halves); "masked": forward_ex, which always passes allow_ragged=True -- the masked forms, causal as asked.
    -> o, or (o, lse)"""
    if entry == "plain":
        if lse:
            o, l, _ = fak.forward_lse(cfg, q, k, v, causal=causal, stats=stats)
            return o, l
        return fak.forward(cfg, q, k, v, causal=causal, stats=stats)[0]
    return flash_attention.forward_ex(cfg, q, k, v, causal=causal, stats=stats, return_lse=lse)


@pytest.mark.parametrize("dtype", list(DTYPES))
@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("shape", [(1, 256, 1), (2, 1024, 3), (1, 4096, 2)])
@pytest.mark.parametrize("speculative", [True, False])
@pytest.mark.parametrize("entry", ["plain", "masked"])
def test_lse_matches_fp32_and_o_is_bit_identical(dtype, causal, shape, speculative, entry):
    B, S, H = shape
    q, k, v = _inputs(B, S, H, dtype, seed=S + H)
    cfg = _cfg(dtype, speculative)
    o_ref = _forward(cfg, q, k, v, causal, entry, lse=False)
    o, lse = _forward(cfg, q, k, v, causal, entry, lse=True)
    torch.cuda.synchronize()
    assert lse.dtype == torch.float32 and lse.shape == (B, H, S) and lse.is_contiguous()
    assert torch.equal(o.view(torch.int16), o_ref.view(torch.int16))
    err = (lse - _ref_lse(q, k, causal)).abs().max().item()
    assert err <= 1e-3, err


@pytest.mark.parametrize("tag", ["bf16", "fp16"])
@pytest.mark.parametrize("entry", ["plain", "masked"])
def test_lse_on_items_the_speculative_pass_redoes(tag, entry):
    """The seam golden's planted spikes make the speculative first pass fail items (the plain form redoes them as 128-row
    halves, the masked form whole): O stays bit-identical to the launch without LSE, and every row's LSE -- those of the
    spiked heads, whose items are the redone ones, in particular -- is within 1e-3 + 2e-6 |lse| of the fp64 value."""
    g = load_seam_golden(tag)
    dtype = g["dtype"]
    q, k, v = (g[n].to(DEV) for n in ("q", "k", "v"))
    cfg = _cfg(dtype, True)
    stats = torch.zeros(2, dtype=torch.int32, device=DEV)
    o_ref = _forward(cfg, q, k, v, False, entry, lse=False)
    o, lse = _forward(cfg, q, k, v, False, entry, lse=True, stats=stats)
    torch.cuda.synchronize()
    assert stats[1].item() > 0
    assert torch.equal(o.view(torch.int16), o_ref.view(torch.int16))
    ref = torch.logsumexp(torch.einsum("bqhd,bkhd->bhqk", q.double(), k.double()) / 128 ** 0.5, dim=-1)
    bound = 1e-3 + 2e-6 * ref.abs()
    bad = (lse.double() - ref).abs() > bound
    assert not bad.any(), ((lse.double() - ref).abs() / bound).max().item()
    spiked = {(int(b), int(h)) for (b, h, *_rest) in g["spikes"]}
    assert spiked
    for b, h in spiked:   # (the rows of the items that ran twice)
        err = (lse[b, h].double() - ref[b, h]).abs()
        assert (err <= bound[b, h]).all(), (b, h, err.max().item())


def _check_parity(got, q, k, v, dout, causal, dtype):
    g32 = _grads(q, k, v, dout, causal, torch.float32)
    g16 = _grads(q, k, v, dout, causal, dtype)
    for name, g, r32, r16 in zip(("dq", "dk", "dv"), got, g32, g16):
        g = g.float()
        assert torch.isfinite(g).all(), name
        bound = 2 * (r16 - r32).abs().max().item() + 1e-4
        err = (g - r32).abs().max().item()
        assert err <= bound, (name, err, bound)
        rel = ((g - r32).norm() / r32.norm()).item()
        rel16 = ((r16 - r32).norm() / r32.norm()).item()
        assert rel <= 2 * rel16 + 1e-3, (name, rel, rel16)


def _torch_o_lse(q, k, v, causal, dtype):
    """O (16-bit) and lse made by torch: isolates the backward from the forward"""
    o = _eager(q.float(), k.float(), v.float(), causal, torch.float32).to(dtype)
    return o.contiguous(), _ref_lse(q, k, causal).contiguous()


@pytest.mark.parametrize("dtype", list(DTYPES))
@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("shape,layout", [((1, 256, 1), "plain"), ((2, 512, 3), "plain"), ((2, 2048, 4), "plain"),
                                          ((1, 8192, 1), "plain"), ((2, 512, 3), "packed"), ((1, 768, 2), "padded"),
                                          ((1, 1280, 2), "plain")])
def test_backward_gradients_from_torch_o_and_lse(dtype, causal, shape, layout):
    B, S, H = shape
    q, k, v = _inputs(B, S, H, dtype, seed=7 * S + H, layout=layout)
    dout = torch.randn((B, S, H, 128), generator=torch.Generator().manual_seed(S)).to(dtype).to(DEV)
    o, lse = _torch_o_lse(q, k, v, causal, dtype)
    got = flash_attention.backward(q, k, v, o, lse, dout, causal=causal)
    torch.cuda.synchronize()
    for g in got:
        assert g.shape == q.shape and g.dtype == dtype and g.is_contiguous()
    _check_parity(got, q, k, v, dout, causal, dtype)


@pytest.mark.parametrize("dtype", list(DTYPES))
@pytest.mark.parametrize("causal", [False, True])
def test_backward_is_deterministic(dtype, causal):
    q, k, v = _inputs(2, 2048, 4, dtype, seed=3)
    dout = torch.randn_like(q.float()).to(dtype)
    o, lse = flash_attention.forward_ex(_cfg(dtype), q, k, v, causal=causal, return_lse=True)
    a = flash_attention.backward(q, k, v, o, lse, dout, causal=causal)
    b = flash_attention.backward(q, k, v, o, lse, dout, causal=causal)
    torch.cuda.synchronize()
    for x, y in zip(a, b):
        assert torch.equal(x.view(torch.int16), y.view(torch.int16))


@pytest.mark.parametrize("dtype", list(DTYPES))
@pytest.mark.parametrize("causal", [False, True])
def test_attention_autograd_end_to_end(dtype, causal):
    B, S, H = 2, 1024, 3
    q, k, v = _inputs(B, S, H, dtype, seed=11)
    g = torch.randn((B, S, H, 128), generator=torch.Generator().manual_seed(5)).to(dtype).to(DEV)
    leaves = [t.clone().requires_grad_(True) for t in (q, k, v)]
    out = flash_attention.attention(*leaves, causal=causal)
    out.backward(g)
    cfg = kc.best_config(DTYPES[dtype], S, masked=causal)
    o, lse = flash_attention.forward_ex(cfg, q, k, v, causal=causal, return_lse=True)
    direct = flash_attention.backward(q, k, v, o, lse, g, causal=causal)
    torch.cuda.synchronize()
    assert torch.equal(out.detach().view(torch.int16), o.view(torch.int16))
    for leaf, d in zip(leaves, direct):
        assert torch.equal(leaf.grad.view(torch.int16), d.view(torch.int16))
    _check_parity([t.grad for t in leaves], q, k, v, g, causal, dtype)


def test_out_of_scope_forms_are_refused():
    q, k, v = _inputs(1, 256, 1, torch.bfloat16)
    ring = [c for c in kc.get_all_supported_configs() if c.dtype == kc.DType.BF16 and c.d_head == 128 and c.B_r == 128
            and c.B_c == 64 and c.n_warps == 4 and c.mma_double_buffer_loads][0]
    with pytest.raises(RuntimeError, match="log-sum-exp"):
        flash_attention.forward_ex(ring, q, k, v, return_lse=True)
    o, lse = flash_attention.forward_ex(_cfg(torch.bfloat16), q, k, v, return_lse=True)
    q2, k2, v2 = _inputs(1, 1000, 1, torch.bfloat16)
    with pytest.raises(RuntimeError, match="seq_len"):
        flash_attention.backward(q2, k2, v2, q2, torch.zeros((1, 1, 1000), device=DEV), q2)
