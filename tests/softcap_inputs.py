"""Inputs and eager references for the logit soft-capping tests (tests/test_softcap_cpu.py, tests/test_softcap_gpu.py).

One packed launch of N(0, 1) q, k, v and dout from the CPU generator; the reference is an fp32 (or 16-bit) eager restatement of
the rule -- logit = softcap tanh(s / softcap) on the keys a row sees, s = q . k / sqrt(128), -inf elsewhere, the cap BEFORE the
mask -- per sequence, with autograd for the gradients.  Two deliberately wrong restatements serve the CPU proof that the inputs
discriminate: no cap at all, and a straight-through cap (the forward capped, the gradient passed as if the cap were linear: the
factor 1 - tanh^2 dropped).  References are computed once per case and shared (nobody writes into them).

Plain helper module: no tests, no fixtures."""
import functools
import math

import torch

import beacon_inputs as bi

D = 128
# the smallest shapes that reach every seam: 128-row Q blocks, 64-key tiles, 128-key dK / dV blocks, 32-row / 32-key cells, rows
# without keys ((5, 0); the first rows of (257, 130) under a causal mask), keys without rows ((0, 5))
PAIRS = [(300, 300), (129, 300), (64, 1), (1, 1), (0, 5), (5, 0), (257, 130)]
HEADS = [(4, 4), (8, 2)]               # (8, 2): group 4, the dK / dV split
WINDOWS = [(-1, -1, False), (-1, -1, True), (100, -1, True), (63, 3, False)]   # (left, right, causal); causal: right = 0
CAPS = [0.5, 4.0]                      # both discriminate on these inputs (tests/test_softcap_cpu.py proves it)
LINEAR_CAP = 50.0                      # nearly linear on these inputs: an accuracy case for the tanh near 0, no discriminator
DTYPES = [torch.bfloat16, torch.float16]
# the sequences the proof leans on: enough keys per row for the cap to move o, dq and dk far beyond the rules' bounds
PROOF_SEQS = [0, 1, 6]


def make_inputs(heads, dtype, seed=0, pairs=None):
    """-> dict: packed q, dout (total_q, H, 128), k, v (total_k, Hkv, 128) in dtype on the CPU, cu_q, cu_k (lists), pairs"""
    pairs = PAIRS if pairs is None else pairs
    n_heads, n_kv = heads
    gen = torch.Generator().manual_seed(1000 + seed)
    total_q, total_k = sum(p[0] for p in pairs), sum(p[1] for p in pairs)
    q = torch.randn((total_q, n_heads, D), generator=gen).to(dtype)
    k = torch.randn((total_k, n_kv, D), generator=gen).to(dtype)
    v = torch.randn((total_k, n_kv, D), generator=gen).to(dtype)
    dout = torch.randn((total_q, n_heads, D), generator=gen).to(dtype)
    cu_q, cu_k = [0], [0]
    for n_q, n_k in pairs:
        cu_q.append(cu_q[-1] + n_q)
        cu_k.append(cu_k[-1] + n_k)
    return dict(q=q, k=k, v=v, dout=dout, cu_q=cu_q, cu_k=cu_k, pairs=list(pairs), heads=heads, dtype=dtype)


def sequence(inp, i):
    """sequence i of make_inputs' dict -> (q, k, v, dout) slices"""
    (q0, q1), (k0, k1) = inp["cu_q"][i:i + 2], inp["cu_k"][i:i + 2]
    return inp["q"][q0:q1], inp["k"][k0:k1], inp["v"][k0:k1], inp["dout"][q0:q1]


def capped_attention(q, k, v, window, dtype, softcap, straight_through=False):
    """Eager attention of ONE sequence in `dtype` arithmetic under window (left, right, causal) with the logits capped before the
    mask (softcap None or 0: no cap) -> o (n_q, H, 128) in dtype, lse fp32 (H, n_q).  A row that sees no key: o = 0, lse = -inf.
    straight_through: the forward's values, but the cap's derivative taken as 1."""
    n_q, n_k = q.shape[0], k.shape[0]
    left, right = bi.window_sides(*window)
    lo, hi = bi.window_bounds(n_q, n_k, left, right)
    group = q.shape[1] // k.shape[1]
    kk, vv = k.to(dtype).repeat_interleave(group, dim=1), v.to(dtype).repeat_interleave(group, dim=1)
    s = torch.einsum("qhd,khd->hqk", q.to(dtype), kk) * (1.0 / math.sqrt(D))
    if softcap:
        capped = softcap * torch.tanh(s / softcap)
        s = s + (capped - s).detach() if straight_through else capped
    keys = torch.arange(n_k)[None, :]
    hidden = (keys > hi[:, None]) | (keys < lo[:, None])
    s = s.masked_fill(hidden[None], bi.NEG_INF)
    dead = hidden.all(dim=1)[None, :, None]
    lse = torch.logsumexp(s.float().masked_fill(dead, 0.0), dim=-1).masked_fill(dead[..., 0], bi.NEG_INF)
    p = torch.softmax(s.masked_fill(dead, 0.0), dim=-1).masked_fill(dead, 0.0)
    return torch.einsum("hqk,khd->qhd", p, vv), lse.detach()


def capped_backward(q, k, v, dout, window, dtype, softcap, straight_through=False):
    """autograd through capped_attention in `dtype` arithmetic -> (o, lse, [dq, dk, dv] as fp32)"""
    leaves = [t.detach().to(dtype).requires_grad_(True) for t in (q, k, v)]
    o, lse = capped_attention(*leaves, window, dtype, softcap, straight_through)
    o.backward(dout.to(dtype))
    return o.detach(), lse, [t.grad.float() for t in leaves]


@functools.lru_cache(maxsize=None)
def inputs(heads, dtype, seed=0):
    return make_inputs(heads, dtype, seed)


@functools.lru_cache(maxsize=None)
def reference(heads, dtype, window, softcap, i, seed=0):
    """Sequence i of inputs(heads, dtype, seed): dict(o32, lse32, g32, o16, g16) -- fp32 and 16-bit eager with the cap and the
    mask, forward and autograd.  Cached: shared by the tests, never written to."""
    q, k, v, dout = sequence(inputs(heads, dtype, seed), i)
    o32, lse32, g32 = capped_backward(q, k, v, dout, window, torch.float32, softcap)
    o16, _, g16 = capped_backward(q, k, v, dout, window, dtype, softcap)
    return dict(o32=o32, lse32=lse32, g32=g32, o16=o16, g16=g16)


def references(heads, dtype, window, softcap, seed=0):
    """reference() of every sequence of the launch"""
    return [reference(heads, dtype, window, softcap, i, seed) for i in range(len(inputs(heads, dtype, seed)["pairs"]))]


def dead_rows(n_q, n_k, window):
    """the rows of a sequence that see no key -> bool (n_q,)"""
    left, right = bi.window_sides(*window)
    lo, hi = bi.window_bounds(n_q, n_k, left, right)
    return (hi < lo) | (n_k == 0)


def unseen_keys(n_q, n_k, window):
    """the keys of a sequence no row sees -> bool (n_k,)"""
    left, right = bi.window_sides(*window)
    lo, hi = bi.window_bounds(n_q, n_k, left, right)
    keys = torch.arange(n_k)[None, :]
    seen = (keys >= lo[:, None]) & (keys <= hi[:, None])
    return ~seen.any(dim=0) if n_q else torch.ones(n_k, dtype=torch.bool)
