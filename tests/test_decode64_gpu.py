"""KV-cache decode at d_head = 64 on the MI355X: forward_kvcache_d64 against eager attention per batch entry at
1 / sqrt(64), fp32 and 16-bit, the sink one more logit column with a zero value row.  The pass rule is beacon_inputs.compare unchanged;
rows that see no key are exact (o = 0, lse = z or -inf).  q is N(0, 1) * 3: the logits' standard deviation is near 3 and a row's
weight sits on a handful of keys, so a dropped, doubled or misplaced 16-key group moves o beyond the bound.  Checked once on the
CPU for the 1000-key entry, every case of the parity test, each 16-key group removed from the fp32 reference in turn: fp16, every
group moves o past compare's bound; bf16, the median group by 3 to 40 bounds, and the least-weighted group stays under the bound
in 10 of the 36 cases (at least 54 of 63 groups pass there)."""
import functools
import math

import pytest
import torch

import beacon_inputs as bi
import flash_attention as fa

pytestmark = pytest.mark.gpu
DEV, D, H, HKV = "cuda:0", 64, 8, 2
DTYPES = pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
LENS, CACHE = [0] + bi.WINDOW_LENGTHS, bi.WINDOW_CACHE_LEN
WINDOWS = [(-1, -1, False), (-1, -1, True), (0, -1, True), (63, 0, False), (100, -1, True), (200, 3, False)]   # (left, right, causal)
Z = torch.linspace(4.0, 7.0, H)
_i32 = functools.partial(torch.tensor, dtype=torch.int32, device=DEV)


def _same(a, b):
    return all(torch.equal(x.view(torch.uint8), y.view(torch.uint8)) for x, y in zip(a, b))


@functools.lru_cache(maxsize=None)
def _inputs(dtype):
    """q (B, 16, H, 64) * 3, k, v (B, CACHE, HKV, 64) on the CPU, q on the device, and the caches there: name -> (k_cache, v_cache, kwargs),
    contiguous and pages of 64 and 256 behind a shuffled block_table with three pages nobody names; "nan": rows at or beyond the
    entry's length and the unnamed pages hold NaN"""
    gen, B = torch.Generator().manual_seed(6400), len(LENS)
    q, k, v = (torch.randn(s, generator=gen).to(dtype) for s in ((B, 16, H, D), (B, CACHE, HKV, D), (B, CACHE, HKV, D)))
    caches = {}
    for tag, fill in (("", 0.0), (" nan", float("nan"))):
        kk, vv = k.clone(), v.clone()
        for b, n in enumerate(LENS if tag else []):
            kk[b, n:], vv[b, n:] = fill, fill
        caches["contiguous" + tag] = (kk.to(DEV), vv.to(DEV), {})
        for page in (64, 256):
            n = CACHE // page
            table = torch.randperm(B * n + 3, generator=gen)[:B * n]
            pages = [torch.full((B * n + 3, page, HKV, D), fill, dtype=dtype).index_copy_(0, table, t.view(B * n, page, HKV, D)) for t in (kk, vv)]
            caches[f"pages of {page}{tag}"] = (pages[0].to(DEV), pages[1].to(DEV), dict(block_table=table.view(B, n).to(torch.int32).to(DEV)))
    return (q * 3).to(dtype), k, v, caches, (q * 3).to(dtype).to(DEV)


def eager(q, k, v, z, window, dtype):
    """ONE batch entry in `dtype` arithmetic: q (Sq, H, 64), k, v (n, HKV, 64), z (H,) or None, window (left, right, causal)
    -> o (Sq, H, 64), lse fp32 (H, Sq)"""
    lo, hi = bi.window_bounds(q.shape[0], k.shape[0], *bi.window_sides(*window))
    kk, vv = (t.to(dtype).repeat_interleave(H // HKV, dim=1) for t in (k, v))
    s = torch.einsum("qhd,khd->hqk", q.to(dtype), kk) * (1.0 / math.sqrt(D))
    keys = torch.arange(k.shape[0])[None, :]
    s = s.masked_fill(((keys > hi[:, None]) | (keys < lo[:, None]))[None], bi.NEG_INF)
    sink = torch.full((H,), bi.NEG_INF) if z is None else z
    s = torch.cat([s, sink.to(dtype)[:, None, None].expand(-1, q.shape[0], 1)], dim=-1)
    dead = (s == bi.NEG_INF).all(dim=-1, keepdim=True)   # (nothing at all: no key and no sink)
    lse = torch.logsumexp(s.float().masked_fill(dead, 0.0), dim=-1).masked_fill(dead[..., 0], bi.NEG_INF)
    p = torch.softmax(s.masked_fill(dead, 0.0), dim=-1).masked_fill(dead, 0.0)
    return torch.einsum("hqk,khd->qhd", p[..., :-1], vv), lse


@functools.lru_cache(maxsize=None)
def _refs(dtype, Sq, window, sunk):
    """(o32, lse32, o16) per entry; shared, never written to"""
    q, k, v = _inputs(dtype)[:3]
    entries = [(q[b, :Sq], k[b, :n], v[b, :n], Z if sunk else None, window) for b, n in enumerate(LENS)]
    return [eager(*e, torch.float32) + eager(*e, dtype)[:1] for e in entries]


def _run(dtype, Sq, cache, window, z, **kw):
    (kc, vc, more), lens = _inputs(dtype)[3][cache], kw.pop("lens", None)
    return fa.forward_kvcache_d64(_inputs(dtype)[4][:, :Sq], kc, vc, _i32(LENS) if lens is None else lens, z, return_lse=True,
                                  window_size=window[:2], causal=window[2], **more, **kw)


@DTYPES
@pytest.mark.parametrize("Sq", [1, 5, 16])
@pytest.mark.parametrize("sunk", [False, True], ids=["plain", "sinks"])
@pytest.mark.parametrize("unit", ["64", "32"])
def test_parity_every_split_count_and_the_bit_identities(dtype, Sq, sunk, unit, monkeypatch):
    """Both units of the kernel, the shipped one and the one it was measured against; 4, 20 and 64 packed rows (NT 1, 2, 4); per window and split count: the rule, dead rows exact, lse one split's to 1e-5 (the
    sink counted once), two runs the same bits, and the same bits again from every paged and every NaN-poisoned cache"""
    monkeypatch.setenv("FA_DECODE64_UNIT", unit)
    z = Z.to(DEV) if sunk else None
    for window in WINDOWS:
        one = None
        for ns in (1, 3, 16, 0):
            o, lse = _run(dtype, Sq, "contiguous", window, z, num_splits=ns)
            for b, (o32, lse32, o16) in enumerate(_refs(dtype, Sq, window, sunk)):
                res = bi.compare(o[b].cpu(), lse[b].cpu(), o32, lse32, o16, dtype)
                assert res["ok"], (window, ns, b, res)
                lo, hi = bi.window_bounds(Sq, LENS[b], *bi.window_sides(*window))
                want = Z[:, None] if sunk else torch.full((H, 1), bi.NEG_INF)
                assert bool((o[b].cpu()[hi < lo] == 0).all()) and torch.equal(lse[b].cpu()[:, hi < lo], want.expand(-1, int((hi < lo).sum()))), (window, ns, b)
            one = lse if one is None else one
            assert float(((lse - one).abs() / one.abs().clamp_min(1.0)).nan_to_num(0.0).max()) <= 1e-5, (window, ns)
            for cache in _inputs(dtype)[3]:
                assert _same((o, lse), _run(dtype, Sq, cache, window, z, num_splits=ns)), (window, ns, cache)


@DTYPES
def test_edge_sinks(dtype):
    """z = +120: o = 0, lse = 120, no NaN; z = -120: the no-sink values within tolerance; None and -inf: the same bits"""
    window = (100, -1, True)
    for ns in (1, 3):
        o0, lse0 = _run(dtype, 5, "pages of 64", window, None, num_splits=ns)
        o, lse = _run(dtype, 5, "pages of 64", window, torch.full((H,), 120.0, device=DEV), num_splits=ns)
        assert bool((o == 0).all()) and float((lse - 120.0).abs().max()) <= bi.LSE_TOL and not bool(torch.isnan(lse).any())
        o, lse = _run(dtype, 5, "pages of 64", window, torch.full((H,), -120.0, device=DEV), num_splits=ns)
        live = lse0 != bi.NEG_INF
        assert float((o.float() - o0.float()).abs().max()) <= bi.O_TOL[dtype] and float((lse[live] - lse0[live]).abs().max()) <= bi.LSE_TOL
        assert bool((lse[~live] == -120.0).all()) and not bool(torch.isnan(o.float()).any())
        assert _same((o0, lse0), _run(dtype, 5, "pages of 64", window, torch.full((H,), bi.NEG_INF, device=DEV), num_splits=ns))


def test_a_captured_graph_sees_the_lengths_and_the_sinks_rewritten_in_place():
    dtype, window = torch.bfloat16, (-1, -1, True)
    lens, z = _i32(LENS), Z.to(DEV)
    assert fa.kvcache_d64_num_splits(_inputs(dtype)[4][:, :5], *_inputs(dtype)[3]["pages of 256"][:2], lens, z, causal=True,
                                     **_inputs(dtype)[3]["pages of 256"][2]) == 16
    step = lambda: _run(dtype, 5, "pages of 256", window, z, lens=lens)   # noqa: E731
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        step()   # (warm-up outside the capture)
    torch.cuda.current_stream().wait_stream(stream)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        got = step()
    for new_lens, new_z in ((LENS, Z), (LENS[::-1], Z + 1.0), ([n // 2 for n in LENS], Z.flip(0)), (LENS, Z)):
        lens.copy_(_i32(new_lens)), z.copy_(new_z)
        graph.replay()
        torch.cuda.synchronize()
        assert _same(got, step()), new_lens


def test_refusals_on_device_tensors():
    q, (k, v, _) = _inputs(torch.bfloat16)[4][:, :1], _inputs(torch.bfloat16)[3]["contiguous"]
    (kp, vp, table), lens = _inputs(torch.bfloat16)[3]["pages of 64"], _i32(LENS)
    with pytest.raises(RuntimeError, match="d_head = 64 only"):
        fa.forward_kvcache_d64(torch.cat([q, q], dim=-1), torch.cat([k, k], dim=-1), torch.cat([v, v], dim=-1), lens)
    with pytest.raises(RuntimeError, match="64 packed query rows"):
        fa.forward_kvcache_d64(torch.zeros((len(LENS), 65, HKV, D), dtype=torch.bfloat16, device=DEV), k, v, lens)
    with pytest.raises(RuntimeError, match="multiple of 64"):
        fa.forward_kvcache_d64(q, kp.view(-1, 32, HKV, D), vp.view(-1, 32, HKV, D), lens, **table)
    with pytest.raises(RuntimeError, match="fp8"):
        fa.forward_kvcache_d64(q, k.to(torch.float8_e4m3fn), v.to(torch.float8_e4m3fn), lens)
    with pytest.raises(RuntimeError, match="sinks"):
        fa.forward_kvcache_d64(q, k, v, lens, Z[:4].to(DEV))
