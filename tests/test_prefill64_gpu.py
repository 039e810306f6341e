"""Prefill at d_head = 64 on the MI355X: forward_varlen_d64 and forward_varlen_kvcache_d64 against eager attention
per sequence at 1 / sqrt(64), fp32 and 16-bit, the sink one more logit column with a zero value row.  The pass rule is
beacon_inputs.compare unchanged; rows that see no key are exact (o = 0, lse = z or -inf).  q is N(0, 1) * 3, as in
test_decode64_gpu.py: a row's weight sits on a handful of keys, so a dropped or misplaced 16-key group moves o beyond the bound.
The pairs cross every 256-row block, 64-row wave and 64-key tile seam; (513, 582) is 2 R + 1 rows for the kernel's R = 256."""
import functools
import math

import pytest
import torch

import beacon_inputs as bi
import flash_attention as fa

pytestmark = pytest.mark.gpu
DEV, D, CACHE = "cuda:0", 64, 1024
PAIRS = [(300, 300), (129, 300), (64, 1), (1, 1), (0, 5), (5, 0), (257, 130), (130, 1000), (513, 582)]   # (len_q, len_k)
WINDOWS = [(-1, -1, False), (-1, -1, True), (0, -1, True), (100, -1, True), (63, 3, False)]                # (left, right, causal)
DTYPES = pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
HEADS = pytest.mark.parametrize("heads", [(8, 2), (4, 4)], ids=["8x2", "4x4"])
_i32 = functools.partial(torch.tensor, dtype=torch.int32, device=DEV)
_cu = lambda lens: _i32([0] + torch.tensor(lens).cumsum(0).tolist())   # noqa: E731


def _same(a, b):
    return all(torch.equal(x.view(torch.uint8), y.view(torch.uint8)) for x, y in zip(a, b))


@functools.lru_cache(maxsize=None)
def _inputs(dtype, heads, pairs=tuple(PAIRS)):
    """per sequence q (len_q, H, 64) * 3 and k, v (len_k, Hkv, 64) on the CPU; the packed tensors on the device; the caches there: name ->
    (k_cache, v_cache, kwargs), contiguous and pages of 64 and 256 behind a shuffled block_table with three pages nobody names; "nan":
    rows at or beyond the sequence's length and the unnamed pages hold NaN"""
    (H, Hkv), gen, B = heads, torch.Generator().manual_seed(6417), len(pairs)
    q = [(torch.randn((nq, H, D), generator=gen) * 3).to(dtype) for nq, _ in pairs]
    k, v = ([torch.randn((nk, Hkv, D), generator=gen).to(dtype) for _, nk in pairs] for _ in range(2))
    caches = {}
    for tag, fill in (("", 0.0), (" nan", float("nan"))):
        kk, vv = (torch.full((B, CACHE, Hkv, D), fill, dtype=dtype) for _ in range(2))
        for b, (_, nk) in enumerate(pairs):
            kk[b, :nk], vv[b, :nk] = k[b], v[b]
        caches["contiguous" + tag] = (kk.to(DEV), vv.to(DEV), {})
        for page in (64, 256):
            n = CACHE // page
            table = torch.randperm(B * n + 3, generator=gen)[:B * n]
            pages = [torch.full((B * n + 3, page, Hkv, D), fill, dtype=dtype).index_copy_(0, table, t.view(B * n, page, Hkv, D)) for t in (kk, vv)]
            caches[f"pages of {page}{tag}"] = (pages[0].to(DEV), pages[1].to(DEV), dict(block_table=table.view(B, n).to(torch.int32).to(DEV)))
    return q, k, v, tuple(torch.cat(t).to(DEV) for t in (q, k, v)), caches


def eager(q, k, v, z, window, dtype):
    """ONE sequence in `dtype` arithmetic (sinks_inputs.sink_attention's text at the scale of 64): q (nq, H, 64), k, v (nk, Hkv, 64),
    z (H,) or None, window (left, right, causal) -> o (nq, H, 64), lse fp32 (H, nq)"""
    lo, hi = bi.window_bounds(q.shape[0], k.shape[0], *bi.window_sides(*window))
    kk, vv = (t.to(dtype).repeat_interleave(q.shape[1] // k.shape[1], dim=1) for t in (k, v))
    s = torch.einsum("qhd,khd->hqk", q.to(dtype), kk) * (1.0 / math.sqrt(D))
    keys = torch.arange(k.shape[0])[None, :]
    s = s.masked_fill(((keys > hi[:, None]) | (keys < lo[:, None]))[None], bi.NEG_INF)
    sink = torch.full((q.shape[1],), bi.NEG_INF) if z is None else z
    s = torch.cat([s, sink.to(dtype)[:, None, None].expand(-1, q.shape[0], 1)], dim=-1)
    dead = (s == bi.NEG_INF).all(dim=-1, keepdim=True)   # (nothing at all: no key and no sink)
    lse = torch.logsumexp(s.float().masked_fill(dead, 0.0), dim=-1).masked_fill(dead[..., 0], bi.NEG_INF)
    p = torch.softmax(s.masked_fill(dead, 0.0), dim=-1).masked_fill(dead, 0.0)
    return torch.einsum("hqk,khd->qhd", p[..., :-1], vv), lse


@functools.lru_cache(maxsize=None)
def _refs(dtype, heads, window, sunk):
    """(o32, lse32, o16) per sequence; shared, never written to"""
    q, k, v = _inputs(dtype, heads)[:3]
    z = torch.linspace(4.0, 7.0, heads[0]) if sunk else None
    seqs = [(q[b], k[b], v[b], z, window) for b in range(len(PAIRS))]
    return [eager(*e, torch.float32) + eager(*e, dtype)[:1] for e in seqs]


def _packed(dtype, heads, window, z, **kw):
    q, k, v = _inputs(dtype, heads)[3]
    return fa.forward_varlen_d64(q, k, v, _cu([p[0] for p in PAIRS]), max(p[0] for p in PAIRS), z, causal=window[2], cu_seqlens_k=_cu([p[1] for p in PAIRS]),
                                 max_seqlen_k=max(p[1] for p in PAIRS), window_size=window[:2], **kw)


def _cached(dtype, heads, cache, window, z, lens=None, q=None, cu=None, max_q=None):
    (kc, vc, more), lens = _inputs(dtype, heads)[4][cache], _i32([p[1] for p in PAIRS]) if lens is None else lens
    return fa.forward_varlen_kvcache_d64(_inputs(dtype, heads)[3][0] if q is None else q, kc, vc, _cu([p[0] for p in PAIRS]) if cu is None else cu,
                                         max(p[0] for p in PAIRS) if max_q is None else max_q, lens, z, causal=window[2], window_size=window[:2], **more)


@DTYPES
@HEADS
@pytest.mark.parametrize("sunk", [False, True], ids=["plain", "sinks"])
@pytest.mark.parametrize("window", WINDOWS, ids=str)
def test_parity_and_the_bit_identities(dtype, heads, sunk, window):
    """one packed launch of all pairs: the rule per sequence, dead rows exact; two runs, None against -inf, and every cache -- paged,
    NaN-poisoned -- the same bits"""
    zc = torch.linspace(4.0, 7.0, heads[0]) if sunk else None
    z = zc.to(DEV) if sunk else None
    o, lse = _packed(dtype, heads, window, z)
    row = 0
    for (nq, nk), (o32, lse32, o16) in zip(PAIRS, _refs(dtype, heads, window, sunk)):
        got_o, got_lse = o[row:row + nq].cpu(), lse[:, row:row + nq].cpu()
        res = bi.compare(got_o, got_lse, o32, lse32, o16, dtype)
        assert res["ok"], (nq, nk, res)
        lo, hi = bi.window_bounds(nq, nk, *bi.window_sides(*window))
        want = zc[:, None] if sunk else torch.full((heads[0], 1), bi.NEG_INF)
        assert bool((got_o[hi < lo] == 0).all()) and torch.equal(got_lse[:, hi < lo], want.expand(-1, int((hi < lo).sum()))), (nq, nk)
        row += nq
    assert _same((o, lse), _packed(dtype, heads, window, z))
    if not sunk:
        assert _same((o, lse), _packed(dtype, heads, window, torch.full((heads[0],), bi.NEG_INF, device=DEV)))
    for cache in _inputs(dtype, heads)[4]:
        assert _same((o, lse), _cached(dtype, heads, cache, window, z)), cache


@DTYPES
@pytest.mark.parametrize("Sq", [1, 5, 16])
def test_agreement_with_decode(dtype, Sq):
    """Sq rows per sequence on the same paged cache: the prefill meets the reference and forward_kvcache_d64's o and lse"""
    heads, window, B = (8, 2), (100, -1, True), len(PAIRS)
    qs = (torch.randn((B, Sq, 8, D), generator=torch.Generator().manual_seed(64)) * 3).to(dtype).to(DEV)
    z, lens = torch.linspace(4.0, 7.0, 8).to(DEV), _i32([p[1] for p in PAIRS])
    o, lse = _cached(dtype, heads, "pages of 64", window, z, q=qs.reshape(B * Sq, 8, D), cu=_i32(list(range(0, B * Sq + 1, Sq))), max_q=Sq)
    kc, vc, more = _inputs(dtype, heads)[4]["pages of 64"]
    od, lsed = fa.forward_kvcache_d64(qs, kc, vc, lens, z, return_lse=True, causal=True, window_size=window[:2], **more)
    assert float((o.view(B, Sq, 8, D).float() - od.float()).abs().max()) <= bi.O_TOL[dtype]
    assert float((lse.view(8, B, Sq).permute(1, 0, 2) - lsed).abs().nan_to_num(0.0).max()) <= bi.LSE_TOL
    k, v = _inputs(dtype, heads)[1:3]
    for b in range(B):
        e = (qs[b].cpu(), k[b], v[b], z.cpu(), window)
        res = bi.compare(o.view(B, Sq, 8, D)[b].cpu(), lse.view(8, B, Sq)[:, b].cpu(), *eager(*e, torch.float32), eager(*e, dtype)[0], dtype)
        assert res["ok"], (b, res)


@DTYPES
def test_edge_sinks(dtype):
    """z = +120: o = 0, lse = 120, no NaN; z = -120: the no-sink values within tolerance"""
    heads, window = (8, 2), (100, -1, True)
    o0, lse0 = _packed(dtype, heads, window, None)
    o, lse = _packed(dtype, heads, window, torch.full((8,), 120.0, device=DEV))
    assert bool((o == 0).all()) and float((lse - 120.0).abs().max()) <= bi.LSE_TOL and not bool(torch.isnan(lse).any())
    o, lse = _packed(dtype, heads, window, torch.full((8,), -120.0, device=DEV))
    live = lse0 != bi.NEG_INF
    assert float((o.float() - o0.float()).abs().max()) <= bi.O_TOL[dtype] and float((lse[live] - lse0[live]).abs().max()) <= bi.LSE_TOL
    assert bool((lse[~live] == -120.0).all()) and not bool(torch.isnan(o.float()).any())


def test_a_captured_graph_sees_the_lengths_and_the_sinks_rewritten_in_place():
    dtype, heads, window = torch.bfloat16, (8, 2), (-1, -1, True)
    base = [p[1] for p in PAIRS]
    lens, z, cu = _i32(base), torch.linspace(4.0, 7.0, 8).to(DEV), _cu([p[0] for p in PAIRS])   # (made outside the capture)
    step = lambda: _cached(dtype, heads, "pages of 256", window, z, lens=lens, cu=cu)   # noqa: E731
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        step()   # (warm-up outside the capture)
    torch.cuda.current_stream().wait_stream(stream)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        got = step()
    for new_lens, shift in ((base, 0.0), (base[::-1], 1.0), ([n // 2 for n in base], -2.0), (base, 0.0)):
        lens.copy_(_i32(new_lens)), z.copy_(torch.linspace(4.0, 7.0, 8).to(DEV) + shift)
        graph.replay()
        torch.cuda.synchronize()
        assert _same(got, step()), new_lens


def test_refusals_on_device_tensors():
    heads = (8, 2)
    q, k, v = _inputs(torch.bfloat16, heads)[3]
    (kc, vc, _), (kp, vp, table) = (_inputs(torch.bfloat16, heads)[4][c] for c in ("contiguous", "pages of 64"))
    cu, lens = _cu([p[0] for p in PAIRS]), _i32([p[1] for p in PAIRS])
    wide = lambda t: torch.cat([t, t], dim=-1)   # noqa: E731
    with pytest.raises(RuntimeError, match="d_head = 64 only"):
        fa.forward_varlen_d64(wide(q), wide(k), wide(v), cu, 513, cu_seqlens_k=_cu([p[1] for p in PAIRS]), max_seqlen_k=1000)
    with pytest.raises(RuntimeError, match="d_head = 64 only"):
        fa.forward_varlen_kvcache_d64(wide(q), wide(kc), wide(vc), cu, 513, lens)
    with pytest.raises(RuntimeError, match="multiple of 64"):
        fa.forward_varlen_kvcache_d64(q, kp.view(-1, 32, 2, D), vp.view(-1, 32, 2, D), cu, 513, lens, **table)
    with pytest.raises(RuntimeError, match="fp8"):
        fa.forward_varlen_kvcache_d64(q, kc.to(torch.float8_e4m3fn), vc.to(torch.float8_e4m3fn), cu, 513, lens)
    with pytest.raises(RuntimeError, match="sinks"):
        fa.forward_varlen_kvcache_d64(q, kc, vc, cu, 513, lens, torch.zeros(4, device=DEV))
