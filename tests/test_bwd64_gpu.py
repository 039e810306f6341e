"""The packed backward at d_head = 64 on the MI355X against eager attention per sequence with autograd at 1 / sqrt(64),
fp32 and 16-bit, the sink one more logit column with a zero value row (sinks_inputs.sink_backward's text at D = 64), by
beacon_inputs.grad_rule unchanged; dead rows and unseen keys are exact zeros.  The pairs cross every block, tile and wave seam; the one
they do not cross -- a dK / dV workgroup that sweeps several query heads: split = group on a small grid -- takes a loose max_seqlen_k."""
import ctypes
import functools
import math

import pytest
import torch

import beacon_inputs as bi
import flash_attention as fa
from flash_attention_from_scratch_amd import _capi
from tests.test_bwd64_cpu import _bwd64

pytestmark = pytest.mark.gpu
DEV, D = "cuda:0", 64
PAIRS = [(300, 300), (129, 300), (64, 1), (1, 1), (0, 5), (5, 0), (257, 130), (130, 600)]      # (len_q, len_k)
WINDOWS = [(-1, -1, False), (-1, -1, True), (0, -1, True), (100, -1, True), (63, 3, False)]    # (left, right, causal)
DTYPES = pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
HEADS = pytest.mark.parametrize("heads", [(8, 2), (4, 4)], ids=["8x2", "4x4"])
_i32 = functools.partial(torch.tensor, dtype=torch.int32, device=DEV)
_cu = lambda lens: _i32([0] + torch.tensor(lens).cumsum(0).tolist())   # noqa: E731
_sinks = lambda H: torch.linspace(4.0, 7.0, H)   # noqa: E731
_same = lambda a, b: all(torch.equal(x.view(torch.uint8), y.view(torch.uint8)) for x, y in zip(a, b))   # noqa: E731


@functools.lru_cache(maxsize=None)
def _inputs(dtype, heads, pairs=tuple(PAIRS)):
    """per sequence N(0, 1) q, k, v, dout on the CPU: q, dout (len_q, H, 64), k, v (len_k, Hkv, 64)"""
    (H, Hkv), gen = heads, torch.Generator().manual_seed(6464)
    q, dout = ([torch.randn((nq, H, D), generator=gen).to(dtype) for nq, _ in pairs] for _ in range(2))
    k, v = ([torch.randn((nk, Hkv, D), generator=gen).to(dtype) for _, nk in pairs] for _ in range(2))
    return q, k, v, dout


@functools.lru_cache(maxsize=None)
def _packed(dtype, heads, pairs=tuple(PAIRS)):   # ... and packed, on the device
    return tuple(torch.cat(t).to(DEV) for t in _inputs(dtype, heads, pairs))


def _seen(nq, nk, window):   # (nq, nk) bool: the keys each row sees
    lo, hi = bi.window_bounds(nq, nk, *bi.window_sides(*window))
    keys = torch.arange(nk)[None, :]
    return (keys >= lo[:, None]) & (keys <= hi[:, None])


def eager_backward(q, k, v, dout, z, window, dtype):
    """autograd through eager attention of ONE sequence in `dtype` arithmetic -> ([dq, dk, dv] fp32, dz fp32 (H,) or None)"""
    leaves = [t.detach().to(dtype).requires_grad_(True) for t in (q, k, v)]
    zz = None if z is None else z.detach().to(dtype).requires_grad_(True)
    group = q.shape[1] // k.shape[1]
    kk, vv = (t.repeat_interleave(group, dim=1) for t in leaves[1:])
    s = torch.einsum("qhd,khd->hqk", leaves[0], kk) * (1.0 / math.sqrt(D))
    s = s.masked_fill(~_seen(q.shape[0], k.shape[0], window)[None], bi.NEG_INF)
    if zz is not None:
        s = torch.cat([s, zz[:, None, None].expand(-1, q.shape[0], 1)], dim=-1)
    dead = (s.detach() == bi.NEG_INF).all(dim=-1, keepdim=True)   # (nothing at all: no key and no sink)
    p = torch.softmax(s.masked_fill(dead, 0.0), dim=-1).masked_fill(dead, 0.0)
    torch.einsum("hqk,khd->qhd", p[..., :k.shape[0]], vv).backward(dout.to(dtype))
    grads = [t.grad.float() if t.grad is not None else torch.zeros_like(t, dtype=torch.float32) for t in leaves]
    return grads, None if zz is None else (zz.grad.float() if zz.grad is not None else torch.zeros(zz.shape))


@functools.lru_cache(maxsize=None)
def _refs(dtype, heads, window, sunk):   # per sequence (g32, g16, dz32, dz16); shared, never written to
    q, k, v, dout = _inputs(dtype, heads)
    z = _sinks(heads[0]) if sunk else None
    both = [[eager_backward(q[b], k[b], v[b], dout[b], z, window, t) for t in (torch.float32, dtype)] for b in range(len(PAIRS))]
    return [(r32[0], r16[0], r32[1], r16[1]) for r32, r16 in both]


def _run(dtype, heads, window, z, max_k=None, one_range=False, pairs=PAIRS):
    """forward_varlen_d64, then backward_varlen_d64 on its o and lse -> (dq, dk, dv, dsinks)"""
    q, k, v, dout = _packed(dtype, heads, tuple(pairs))
    sides = {} if one_range else dict(cu_seqlens_k=_cu([p[1] for p in pairs]), max_seqlen_k=max_k or max(p[1] for p in pairs))
    cu, max_q = _cu([p[0] for p in pairs]), max(p[0] for p in pairs)
    o, lse = fa.forward_varlen_d64(q, k, v, cu, max_q, z, causal=window[2], window_size=window[:2], **sides)
    return fa.backward_varlen_d64(q, k, v, o, lse, dout, cu, max_q, z, window[:2], causal=window[2], **sides)


def _check(got, dtype, heads, window, sunk):
    """grad_rule per sequence and gradient, the exact zeros, the rule on dsinks summed over the launch; prints the worst ratios"""
    dq, dk, dv = (g.cpu() for g in got[:3])
    refs, rq, rk, worst = _refs(dtype, heads, window, sunk), 0, 0, {}
    for (nq, nk), (g32, g16, _, _) in zip(PAIRS, refs):
        mine = (dq[rq:rq + nq], dk[rk:rk + nk], dv[rk:rk + nk])
        for name, g, r32, r16 in zip(("dq", "dk", "dv"), mine, g32, g16):
            assert g.shape == r32.shape, (nq, nk, name)
            if not g.numel():   # (an empty side: nothing to compare)
                continue
            res = bi.grad_rule(g, r32, r16)
            worst[name] = max(worst.get(name, 0.0), res["ratio"])
            assert res["ok"], (nq, nk, name, res)
        seen = _seen(nq, nk, window)
        assert bool((mine[0][~seen.any(dim=1)] == 0).all()), (nq, nk, "dq of a row that sees no key")
        assert bool((mine[1][~seen.any(dim=0)] == 0).all()) and bool((mine[2][~seen.any(dim=0)] == 0).all()), (nq, nk, "an unseen key")
        rq, rk = rq + nq, rk + nk
    if sunk:
        res = bi.grad_rule(got[3].cpu(), sum(r[2] for r in refs), sum(r[3] for r in refs))
        worst["dsinks"] = res["ratio"]
        assert res["ok"], ("dsinks", res)
    print(f"bwd64 {dtype} {heads} {window} sinks={sunk}: worst err / bound {worst}")


@DTYPES
@HEADS
@pytest.mark.parametrize("sunk", [False, True], ids=["plain", "sinks"])
@pytest.mark.parametrize("window", WINDOWS, ids=str)
def test_parity_and_the_bit_identities(dtype, heads, sunk, window):
    """one packed launch of all pairs: the rule per sequence, the exact zeros; two runs, and None against -inf sinks, the same bits"""
    z = _sinks(heads[0]).to(DEV) if sunk else None
    got = _run(dtype, heads, window, z)
    assert (got[3] is None) == (not sunk) and (not sunk or (got[3].dtype == torch.float32 and got[3].shape == (heads[0],)))
    _check(got, dtype, heads, window, sunk)
    again = _run(dtype, heads, window, z)
    assert _same(got[:3], again[:3]) and (not sunk or _same(got[3:], again[3:]))
    if not sunk:
        off = _run(dtype, heads, window, torch.full((heads[0],), bi.NEG_INF, device=DEV))
        assert _same(got[:3], off[:3]) and bool((off[3] == 0).all())


@DTYPES
@pytest.mark.parametrize("max_k,window", [(1024, (63, 3, False)), (4096, (-1, -1, False)), (4096, (100, -1, True))], ids=str)
def test_a_sweep_over_several_query_heads(dtype, max_k, window):
    """a loose max_seqlen_k enlarges the grid, so the split rule gives (8, 2) a split of 2 or 1: a dK / dV workgroup sweeps 2 or 4 heads"""
    _check(_run(dtype, (8, 2), window, _sinks(8).to(DEV), max_k=max_k), dtype, (8, 2), window, True)


@DTYPES
def test_one_range_autograd_and_a_16_bit_sinks_parameter(dtype):
    heads, window, pairs = (8, 2), (100, -1, True), [(n, n) for n, _ in PAIRS]
    z = _sinks(8).to(DEV)
    assert _same(_run(dtype, heads, window, z, one_range=True, pairs=pairs), _run(dtype, heads, window, z, pairs=pairs))
    cu, cuk = _cu([p[0] for p in PAIRS]), _cu([p[1] for p in PAIRS])
    for sinks in (z.clone().requires_grad_(True), z.to(dtype).requires_grad_(True), None):
        q, k, v = (t.clone().requires_grad_(True) for t in _packed(dtype, heads)[:3])
        fa.attention_varlen_d64(q, k, v, cu, 300, sinks, causal=True, cu_seqlens_k=cuk, max_seqlen_k=600, window_size=(100, -1)).backward(_packed(dtype, heads)[3])
        want = _run(dtype, heads, window, None if sinks is None else sinks.detach().float())
        assert _same((q.grad, k.grad, v.grad), want[:3])
        if sinks is not None:
            assert sinks.grad.dtype == sinks.dtype and torch.equal(sinks.grad, want[3].to(sinks.dtype))


@DTYPES
def test_edge_sinks(dtype):
    """heads 0, 1, 2 at +120, -120, -inf: all finite, heads 1 and 2 the no-sink gradients under the rule (MHA: dk, dv per query head)"""
    heads, window = (4, 4), (100, -1, True)
    z = _sinks(4)
    z[0], z[1], z[2] = 120.0, -120.0, bi.NEG_INF
    got = [g.cpu() for g in _run(dtype, heads, window, z.to(DEV))]
    assert all(bool(torch.isfinite(g.float()).all()) for g in got) and got[3][2].item() == 0.0
    rq = rk = 0
    for (nq, nk), (g32, g16, _, _) in zip(PAIRS, _refs(dtype, heads, window, False)):
        for g, r32, r16 in zip((got[0][rq:rq + nq], got[1][rk:rk + nk], got[2][rk:rk + nk]), g32, g16):
            assert not g.numel() or bi.grad_rule(g[:, 1:3], r32[:, 1:3], r16[:, 1:3])["ok"], (nq, nk)
        rq, rk = rq + nq, rk + nk


def test_a_captured_graph_sees_the_offsets_and_the_sinks_rewritten_in_place():
    dtype, heads, window = torch.bfloat16, (8, 2), (100, -1, True)
    q, k, v, dout = _packed(dtype, heads)
    lens, moved = PAIRS, [list(p) for p in PAIRS]   # moved: the same totals, two sequences' rows dealt to their neighbours
    moved[0][0], moved[1][0], moved[0][1], moved[7][1] = 200, 229, 500, 400
    cu, cuk, z = _cu([p[0] for p in lens]), _cu([p[1] for p in lens]), _sinks(8).to(DEV)   # (made outside the capture)

    def step():
        o, lse = fa.forward_varlen_d64(q, k, v, cu, 300, z, causal=True, cu_seqlens_k=cuk, max_seqlen_k=600, window_size=window[:2])
        return (o, lse) + fa.backward_varlen_d64(q, k, v, o, lse, dout, cu, 300, z, window[:2], causal=True, cu_seqlens_k=cuk, max_seqlen_k=600)

    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        step()   # (warm-up outside the capture)
    torch.cuda.current_stream().wait_stream(stream)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        got = step()
    for new, shift in ((lens, 0.0), (lens[::-1], 1.0), (moved, -2.0), (lens, 0.0)):
        cu.copy_(_cu([p[0] for p in new])), cuk.copy_(_cu([p[1] for p in new])), z.copy_(_sinks(8).to(DEV) + shift)
        graph.replay()
        torch.cuda.synchronize()
        assert _same(got, step()), new


def test_refusals_on_device_tensors():
    dtype, heads = torch.bfloat16, (8, 2)
    q, k, v, dout = _packed(dtype, heads)
    cu, cuk = _cu([p[0] for p in PAIRS]), _cu([p[1] for p in PAIRS])
    o, lse = fa.forward_varlen_d64(q, k, v, cu, 300, cu_seqlens_k=cuk, max_seqlen_k=600)
    wide = lambda t: torch.cat([t, t], dim=-1)   # noqa: E731
    with pytest.raises(RuntimeError, match="d_head = 64 only"):
        fa.backward_varlen_d64(wide(q), wide(k), wide(v), wide(o), lse, wide(dout), cu, 300, cu_seqlens_k=cuk, max_seqlen_k=600)
    with pytest.raises(RuntimeError, match="d_head = 128 only"):
        fa.backward_varlen_sinks(q, k, v, o, lse, dout, cu, 300, _sinks(8).to(DEV), cu_seqlens_k=cuk, max_seqlen_k=600)
    # sinks without dsinks, through the C ABI (refused before any pointer is followed: test_bwd64_cpu's host-only arguments)
    args = _bwd64(n_seqs=len(PAIRS), T=q.shape[0], Tk=k.shape[0], max_seqlen=300, max_seqlen_k=600)
    w, sk = _capi.make_window(-1, -1), _capi.make_sinks(_sinks(8).to(DEV).data_ptr(), 8)
    rc = _capi.load().fa_bwd_launch_varlen_qk_d64(ctypes.byref(args), ctypes.byref(w), ctypes.byref(sk), None, None, None)
    assert rc == -1 and "dsinks is null" in _capi.last_error()
