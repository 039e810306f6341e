"""Prefill at d_head = 256 on the MI355X: forward_varlen_d256 and forward_varlen_kvcache_d256 against eager attention
per sequence at 1 / sqrt(256), fp32 and 16-bit, the cap in front of the mask.  The pass rule is beacon_inputs.compare unchanged; rows
that see no key are exact (o = 0, lse = -inf).  q is N(0, 1) * 3, as in test_decode256_gpu.py: a row's weight sits on a handful of
keys, so a dropped or misplaced 16-key group moves o beyond the bound.  The pairs cross every 128-row block, 32-row wave and 64-key
tile seam.  The dropped-group count on the CPU against the fp32 reference (each 16-key group a row sees removed in turn) is
test_decode256_gpu.py's for the same inputs' distribution; it was NOT repeated for these pairs."""
import functools
import math

import pytest
import torch

import beacon_inputs as bi
import flash_attention as fa

pytestmark = pytest.mark.gpu
DEV, D, CACHE = "cuda:0", 256, 1024
PAIRS = [(300, 300), (129, 300), (64, 1), (1, 1), (0, 5), (5, 0), (257, 130), (130, 1000), (33, 95)]   # (len_q, len_k)
WINDOWS = [(-1, -1, False), (-1, -1, True), (0, -1, True), (100, -1, True), (63, 3, False)]            # (left, right, causal)
DTYPES = pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
HEADS = pytest.mark.parametrize("heads", [(4, 2), (2, 2)], ids=["4x2", "2x2"])
_i32 = functools.partial(torch.tensor, dtype=torch.int32, device=DEV)
_cu = lambda lens: _i32([0] + torch.tensor(lens).cumsum(0).tolist())   # noqa: E731


def _same(a, b):
    return all(torch.equal(x.view(torch.uint8), y.view(torch.uint8)) for x, y in zip(a, b))


@functools.lru_cache(maxsize=None)
def _inputs(dtype, heads):
    """per sequence q (len_q, H, 256) * 3 and k, v (len_k, Hkv, 256) on the CPU; the packed tensors on the device; the caches there: name
    -> (k_cache, v_cache, kwargs), contiguous and pages of 64 and 256 behind a shuffled block_table with three pages nobody names;
    "nan": rows at or beyond the sequence's length and the unnamed pages hold NaN"""
    (H, Hkv), gen, B = heads, torch.Generator().manual_seed(25621), len(PAIRS)
    q = [(torch.randn((nq, H, D), generator=gen) * 3).to(dtype) for nq, _ in PAIRS]
    k, v = ([torch.randn((nk, Hkv, D), generator=gen).to(dtype) for _, nk in PAIRS] for _ in range(2))
    caches = {}
    for tag, fill in (("", 0.0), (" nan", float("nan"))):
        kk, vv = (torch.full((B, CACHE, Hkv, D), fill, dtype=dtype) for _ in range(2))
        for b, (_, nk) in enumerate(PAIRS):
            kk[b, :nk], vv[b, :nk] = k[b], v[b]
        caches["contiguous" + tag] = (kk.to(DEV), vv.to(DEV), {})
        for page in (64, 256):
            n = CACHE // page
            table = torch.randperm(B * n + 3, generator=gen)[:B * n]
            pages = [torch.full((B * n + 3, page, Hkv, D), fill, dtype=dtype).index_copy_(0, table, t.view(B * n, page, Hkv, D)) for t in (kk, vv)]
            caches[f"pages of {page}{tag}"] = (pages[0].to(DEV), pages[1].to(DEV), dict(block_table=table.view(B, n).to(torch.int32).to(DEV)))
    return q, k, v, tuple(torch.cat(t).to(DEV) for t in (q, k, v)), caches


def eager(q, k, v, cap, window, dtype):
    """ONE sequence in `dtype` arithmetic: q (nq, H, 256), k, v (nk, Hkv, 256), cap 0 = none, window (left, right, causal)
    -> o (nq, H, 256), lse fp32 (H, nq)"""
    lo, hi = bi.window_bounds(q.shape[0], k.shape[0], *bi.window_sides(*window))
    kk, vv = (t.to(dtype).repeat_interleave(q.shape[1] // k.shape[1], dim=1) for t in (k, v))
    s = torch.einsum("qhd,khd->hqk", q.to(dtype), kk) * (1.0 / math.sqrt(D))
    if cap:
        s = cap * torch.tanh(s / cap)
    keys = torch.arange(k.shape[0])[None, :]
    s = s.masked_fill(((keys > hi[:, None]) | (keys < lo[:, None]))[None], bi.NEG_INF)
    dead = (s == bi.NEG_INF).all(dim=-1, keepdim=True)
    lse = torch.logsumexp(s.float().masked_fill(dead, 0.0), dim=-1).masked_fill(dead[..., 0], bi.NEG_INF)
    p = torch.softmax(s.masked_fill(dead, 0.0), dim=-1).masked_fill(dead, 0.0)
    return torch.einsum("hqk,khd->qhd", p, vv), lse


@functools.lru_cache(maxsize=None)
def _refs(dtype, heads, window, cap):
    """(o32, lse32, o16) per sequence; shared, never written to"""
    q, k, v = _inputs(dtype, heads)[:3]
    seqs = [(q[b], k[b], v[b], cap, window) for b in range(len(PAIRS))]
    return [eager(*e, torch.float32) + eager(*e, dtype)[:1] for e in seqs]


def _packed(dtype, heads, window, cap):
    q, k, v = _inputs(dtype, heads)[3]
    return fa.forward_varlen_d256(q, k, v, _cu([p[0] for p in PAIRS]), max(p[0] for p in PAIRS), cap, causal=window[2],
                                  cu_seqlens_k=_cu([p[1] for p in PAIRS]), max_seqlen_k=max(p[1] for p in PAIRS), window_size=window[:2])


def _cached(dtype, heads, cache, window, cap, lens=None, q=None, cu=None, max_q=None):
    (kc, vc, more), lens = _inputs(dtype, heads)[4][cache], _i32([p[1] for p in PAIRS]) if lens is None else lens
    return fa.forward_varlen_kvcache_d256(_inputs(dtype, heads)[3][0] if q is None else q, kc, vc, _cu([p[0] for p in PAIRS]) if cu is None else cu,
                                          max(p[0] for p in PAIRS) if max_q is None else max_q, lens, cap, causal=window[2], window_size=window[:2],
                                          **more)


@DTYPES
@HEADS
@pytest.mark.parametrize("cap", [0.0, 4.0], ids=["plain", "cap 4"])
@pytest.mark.parametrize("tile", ["64", "32"])
@pytest.mark.parametrize("window", WINDOWS, ids=str)
def test_parity_and_the_bit_identities(monkeypatch, dtype, heads, cap, tile, window):
    """one packed launch of all pairs at either tile form: the rule per sequence, dead rows exact; two runs and every cache -- paged,
    NaN-poisoned -- the same bits"""
    monkeypatch.setenv("FA_PREFILL256_TILE", tile)
    o, lse = _packed(dtype, heads, window, cap)
    row = 0
    for (nq, nk), (o32, lse32, o16) in zip(PAIRS, _refs(dtype, heads, window, cap)):
        got_o, got_lse = o[row:row + nq].cpu(), lse[:, row:row + nq].cpu()
        res = bi.compare(got_o, got_lse, o32, lse32, o16, dtype)
        assert res["ok"], (nq, nk, res)
        lo, hi = bi.window_bounds(nq, nk, *bi.window_sides(*window))
        assert bool((got_o[hi < lo] == 0).all()) and bool((got_lse[:, hi < lo] == bi.NEG_INF).all()), (nq, nk)
        row += nq
    assert _same((o, lse), _packed(dtype, heads, window, cap))
    for cache in _inputs(dtype, heads)[4]:
        assert _same((o, lse), _cached(dtype, heads, cache, window, cap)), cache


@DTYPES
@pytest.mark.parametrize("Sq", [1, 5, 16])
def test_agreement_with_decode(dtype, Sq):
    """Sq rows per sequence on the same paged cache: the prefill meets the reference and forward_kvcache_d256's o and lse"""
    heads, window, cap, B, H = (4, 2), (100, -1, True), 4.0, len(PAIRS), 4
    qs = (torch.randn((B, Sq, H, D), generator=torch.Generator().manual_seed(256)) * 3).to(dtype).to(DEV)
    lens = _i32([p[1] for p in PAIRS])
    o, lse = _cached(dtype, heads, "pages of 64", window, cap, q=qs.reshape(B * Sq, H, D), cu=_i32(list(range(0, B * Sq + 1, Sq))), max_q=Sq)
    kc, vc, more = _inputs(dtype, heads)[4]["pages of 64"]
    od, lsed = fa.forward_kvcache_d256(qs, kc, vc, lens, cap, return_lse=True, causal=True, window_size=window[:2], **more)
    assert float((o.view(B, Sq, H, D).float() - od.float()).abs().max()) <= bi.O_TOL[dtype]
    assert float((lse.view(H, B, Sq).permute(1, 0, 2) - lsed).abs().nan_to_num(0.0).max()) <= bi.LSE_TOL
    k, v = _inputs(dtype, heads)[1:3]
    for b in range(B):
        e = (qs[b].cpu(), k[b], v[b], cap, window)
        res = bi.compare(o.view(B, Sq, H, D)[b].cpu(), lse.view(H, B, Sq)[:, b].cpu(), *eager(*e, torch.float32), eager(*e, dtype)[0], dtype)
        assert res["ok"], (b, res)


def test_a_captured_graph_sees_the_lengths_rewritten_in_place():
    dtype, heads, window, cap = torch.bfloat16, (4, 2), (-1, -1, True), 4.0
    base = [p[1] for p in PAIRS]
    lens, cu = _i32(base), _cu([p[0] for p in PAIRS])   # (made outside the capture)
    step = lambda: _cached(dtype, heads, "pages of 256", window, cap, lens=lens, cu=cu)   # noqa: E731
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        step()   # (warm-up outside the capture: the device's one-time setup is not capturable)
    torch.cuda.current_stream().wait_stream(stream)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        got = step()
    for new_lens in (base, base[::-1], [n // 2 for n in base], base):
        lens.copy_(_i32(new_lens))
        graph.replay()
        torch.cuda.synchronize()
        assert _same(got, step()), new_lens


def test_refusals_on_device_tensors():
    heads = (4, 2)
    q, k, v = _inputs(torch.bfloat16, heads)[3]
    (kc, vc, _), (kp, vp, table) = (_inputs(torch.bfloat16, heads)[4][c] for c in ("contiguous", "pages of 64"))
    cu, lens = _cu([p[0] for p in PAIRS]), _i32([p[1] for p in PAIRS])
    half = lambda t: t[..., :128].contiguous()   # noqa: E731
    with pytest.raises(RuntimeError, match="d_head = 256 only"):
        fa.forward_varlen_d256(half(q), half(k), half(v), cu, 300, cu_seqlens_k=_cu([p[1] for p in PAIRS]), max_seqlen_k=1000)
    with pytest.raises(RuntimeError, match="d_head = 256 only"):
        fa.forward_varlen_kvcache_d256(half(q), half(kc), half(vc), cu, 300, lens)
    with pytest.raises(RuntimeError, match="multiple of 64"):
        fa.forward_varlen_kvcache_d256(q, kp.view(-1, 32, 2, D), vp.view(-1, 32, 2, D), cu, 300, lens, **table)
    with pytest.raises(RuntimeError, match="fp8"):
        fa.forward_varlen_kvcache_d256(q, kc.to(torch.float8_e4m3fn), vc.to(torch.float8_e4m3fn), cu, 300, lens)
    with pytest.raises(ValueError, match="softcap"):
        fa.forward_varlen_kvcache_d256(q, kc, vc, cu, 300, lens, -1.0)
