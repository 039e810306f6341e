"""Inputs and eager references for the attention-sink tests (tests/test_sinks_cpu.py, tests/test_sinks_gpu.py).

The packed launch is softcap_inputs' (N(0, 1) q, k, v and dout from the CPU generator, the PAIRS that reach every seam); the
reference is an eager restatement of the rule per sequence, with autograd: head h's sink z = sinks[h] is ONE MORE COLUMN of logits
whose value row is zero, so lse = log(exp(z) + sum_j exp(s_j)) and o = sum_j exp(s_j - lse) v_j over the keys a row sees.  A row
that sees no key has the sink as its softmax's only member: o = 0, lse = z.  z = -inf is "no sink": the column is masked like any
key, and a row that then has nothing at all gives o = 0, lse = -inf.  It runs in fp32 and in 16-bit arithmetic and returns, beside
o, lse and dq, dk, dv, that sequence's share of dsinks.  References are computed once per case and shared (nobody writes into them).

Plain helper module: no tests, no fixtures."""
import functools
import math

import torch

import beacon_inputs as bi
from softcap_inputs import D, DTYPES, HEADS, PAIRS, PROOF_SEQS, WINDOWS, dead_rows, inputs, make_inputs, sequence, unseen_keys  # noqa: F401


def SINKS_LIVE(n_heads):
    """sinks that matter on N(0, 1) inputs: exp(4 .. 7) against a row's sum of exp(s_j), s_j ~ N(0, 1)"""
    return torch.linspace(4.0, 7.0, n_heads)


def SINKS_EDGE(n_heads):
    """... with head 0 far above every logit, head 1 far below, and head 2 without a sink"""
    z = SINKS_LIVE(n_heads).clone()
    z[0], z[1], z[2] = 120.0, -120.0, bi.NEG_INF
    return z


def sink_attention(q, k, v, sinks, window, dtype):
    """Eager attention of ONE sequence in `dtype` arithmetic under window (left, right, causal) with the sink as one more column
    of logits and a zero value row (sinks None: no such column) -> o (n_q, H, 128) in dtype, lse fp32 (H, n_q)."""
    n_q, n_k = q.shape[0], k.shape[0]
    left, right = bi.window_sides(*window)
    lo, hi = bi.window_bounds(n_q, n_k, left, right)
    group = q.shape[1] // k.shape[1]
    kk, vv = k.to(dtype).repeat_interleave(group, dim=1), v.to(dtype).repeat_interleave(group, dim=1)
    s = torch.einsum("qhd,khd->hqk", q.to(dtype), kk) * (1.0 / math.sqrt(D))
    keys = torch.arange(n_k)[None, :]
    hidden = (keys > hi[:, None]) | (keys < lo[:, None])
    s = s.masked_fill(hidden[None], bi.NEG_INF)
    if sinks is not None:
        s = torch.cat([s, sinks.to(dtype)[:, None, None].expand(-1, n_q, 1)], dim=-1)
    dead = (s.detach() == bi.NEG_INF).all(dim=-1, keepdim=True)   # (nothing at all: no key and no sink)
    lse = torch.logsumexp(s.float().masked_fill(dead, 0.0), dim=-1).masked_fill(dead[..., 0], bi.NEG_INF)
    p = torch.softmax(s.masked_fill(dead, 0.0), dim=-1).masked_fill(dead, 0.0)
    return torch.einsum("hqk,khd->qhd", p[..., :n_k], vv), lse.detach()


def sink_backward(q, k, v, dout, sinks, window, dtype):
    """autograd through sink_attention in `dtype` arithmetic -> (o, lse, [dq, dk, dv] as fp32, dsinks as fp32 (H,) or None)"""
    leaves = [t.detach().to(dtype).requires_grad_(True) for t in (q, k, v)]
    z = None if sinks is None else sinks.detach().to(dtype).requires_grad_(True)
    o, lse = sink_attention(*leaves, z, window, dtype)
    o.backward(dout.to(dtype))
    grads = [t.grad.float() if t.grad is not None else torch.zeros_like(t, dtype=torch.float32) for t in leaves]
    dz = None if z is None else (z.grad.float() if z.grad is not None else torch.zeros(z.shape))
    return o.detach(), lse, grads, dz


@functools.lru_cache(maxsize=None)
def reference(heads, dtype, window, i, seed=0):
    """Sequence i of inputs(heads, dtype, seed) under SINKS_LIVE: dict(o32, lse32, g32, dz32, o16, g16, dz16) -- fp32 and 16-bit
    eager, forward and autograd.  Cached: shared by the tests, never written to."""
    q, k, v, dout = sequence(inputs(heads, dtype, seed), i)
    z = SINKS_LIVE(heads[0])
    o32, lse32, g32, dz32 = sink_backward(q, k, v, dout, z, window, torch.float32)
    o16, _, g16, dz16 = sink_backward(q, k, v, dout, z, window, dtype)
    return dict(o32=o32, lse32=lse32, g32=g32, dz32=dz32, o16=o16, g16=g16, dz16=dz16)


def references(heads, dtype, window, seed=0):
    """reference() of every sequence of the launch"""
    return [reference(heads, dtype, window, i, seed) for i in range(len(inputs(heads, dtype, seed)["pairs"]))]


def dsinks_references(heads, dtype, window, seed=0):
    """the launch's dsinks: the sequences' shares summed -> (fp32 eager, 16-bit eager), each fp32 (H,)"""
    refs = references(heads, dtype, window, seed)
    return sum(r["dz32"] for r in refs), sum(r["dz16"] for r in refs)


def dsinks_rule(dsinks, heads, dtype, window, seed=0):
    """bi.grad_rule on the (n_heads,) vector summed over the launch"""
    return bi.grad_rule(dsinks, *dsinks_references(heads, dtype, window, seed))


def dsinks_formula(o, lse, dout, sinks):
    """the kernel's own formula for one sequence, in fp32: - sum_rows exp(z - lse) delta, delta = rowsum(dout * o); a row with
    lse = -inf or a head with z = -inf adds nothing -> fp32 (H,)"""
    delta = (dout.float() * o.float()).sum(dim=-1).transpose(0, 1)   # (H, n_q)
    z = sinks.float()[:, None]
    w = torch.exp(z - lse)
    w = torch.where((z == bi.NEG_INF) | (lse == bi.NEG_INF), torch.zeros_like(w), w)
    return -(w * delta).sum(dim=1)
