"""KV-cache decode at d_head = 256 on the MI355X: forward_kvcache_d256 against eager attention per batch entry at
1 / sqrt(256), fp32 and 16-bit, with and without the logit cap.  The pass rule is beacon_inputs.compare unchanged; rows that see no key
are exact (o = 0, lse = -inf).  q is N(0, 1) * 3: the logits' standard deviation is near 3 and a row's weight sits on a handful of
keys, so a dropped, doubled or misplaced 16-key group moves o beyond the bound.  Checked once on the CPU for the 1000-key entry, every
case of the parity test (48 per dtype), each 16-key group a row sees removed from the fp32 reference in turn: fp16, every group of
every case moves o past compare's bound (1234 of 1234); bf16, 1171 of 1234, every group in 42 of the 48 cases -- the loosest are
the single uncapped row of (4, 2, 1) without a window (34 of 63 groups) and with (200, 3) (13 of 14), the others miss one or two
of 63.  fp16 carries the index computations where bf16's bound is loose."""
import functools
import math

import pytest
import torch

import beacon_inputs as bi
import flash_attention as fa

pytestmark = pytest.mark.gpu
DEV, D, H = "cuda:0", 256, 4
DTYPES = pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
SHAPES = [(4, 2, 1), (4, 2, 8), (4, 2, 16), (4, 1, 8)]   # (H, Hkv, Sq): 2, 16, 32 and 32 packed rows
LENS, CACHE = [0] + bi.WINDOW_LENGTHS, bi.WINDOW_CACHE_LEN
WINDOWS = [(-1, -1, False), (-1, -1, True), (0, -1, True), (63, 0, False), (100, -1, True), (200, 3, False)]   # (left, right, causal)
_i32 = functools.partial(torch.tensor, dtype=torch.int32, device=DEV)


def _same(a, b):
    return all(torch.equal(x.view(torch.uint8), y.view(torch.uint8)) for x, y in zip(a, b))


@functools.lru_cache(maxsize=None)
def _inputs(dtype):
    """q (B, 16, H, 256) * 3, k, v (B, CACHE, 2, 256) on the CPU, q on the device, and the caches there: name -> (k_cache, v_cache, kwargs),
    contiguous and pages of 64 and 256 behind a shuffled block_table with three pages nobody names; "nan": rows at or beyond the
    entry's length and the unnamed pages hold NaN.  One K / V head: the first head's view of the same tensors"""
    gen, B = torch.Generator().manual_seed(25600), len(LENS)
    q, k, v = (torch.randn(s, generator=gen).to(dtype) for s in ((B, 16, H, D), (B, CACHE, 2, D), (B, CACHE, 2, D)))
    caches = {}
    for tag, fill in (("", 0.0), (" nan", float("nan"))):
        kk, vv = k.clone(), v.clone()
        for b, n in enumerate(LENS if tag else []):
            kk[b, n:], vv[b, n:] = fill, fill
        caches["contiguous" + tag] = (kk.to(DEV), vv.to(DEV), {})
        for page in (64, 256):
            n = CACHE // page
            table = torch.randperm(B * n + 3, generator=gen)[:B * n]
            pages = [torch.full((B * n + 3, page, 2, D), fill, dtype=dtype).index_copy_(0, table, t.view(B * n, page, 2, D)) for t in (kk, vv)]
            caches[f"pages of {page}{tag}"] = (pages[0].to(DEV), pages[1].to(DEV), dict(block_table=table.view(B, n).to(torch.int32).to(DEV)))
    return (q * 3).to(dtype), k, v, caches, (q * 3).to(dtype).to(DEV)


def eager(q, k, v, cap, window, dtype):
    """ONE batch entry in `dtype` arithmetic: q (Sq, H, 256), k, v (n, Hkv, 256), cap 0 = none, window (left, right, causal)
    -> o (Sq, H, 256), lse fp32 (H, Sq)"""
    lo, hi = bi.window_bounds(q.shape[0], k.shape[0], *bi.window_sides(*window))
    kk, vv = (t.to(dtype).repeat_interleave(H // k.shape[1], dim=1) for t in (k, v))
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
def _refs(dtype, Hkv, Sq, window, cap):
    """(o32, lse32, o16) per entry; shared, never written to"""
    q, k, v = _inputs(dtype)[:3]
    entries = [(q[b, :Sq], k[b, :n, :Hkv], v[b, :n, :Hkv], cap, window) for b, n in enumerate(LENS)]
    return [eager(*e, torch.float32) + eager(*e, dtype)[:1] for e in entries]


def _run(dtype, Hkv, Sq, cache, window, cap, **kw):
    (kc, vc, more), lens = _inputs(dtype)[3][cache], kw.pop("lens", None)
    return fa.forward_kvcache_d256(_inputs(dtype)[4][:, :Sq], kc[:, :, :Hkv], vc[:, :, :Hkv], _i32(LENS) if lens is None else lens, cap,
                                   return_lse=True, window_size=window[:2], causal=window[2], **more, **kw)


@DTYPES
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "h%d_kv%d_q%d" % s)
@pytest.mark.parametrize("cap", [0.0, 4.0], ids=["plain", "cap4"])
@pytest.mark.parametrize("unit", ["16", "32"])
def test_parity_every_split_count_and_the_bit_identities(dtype, shape, cap, unit, monkeypatch):
    """Both units of the kernel (beyond 16 rows only the 16-key unit exists); 2, 16 and 32 packed rows (NT 1, 2), GQA and MQA; a cap small
    enough that tanh bends the logits; per window and split count: the rule, dead rows exact, lse one split's to 1e-5, two runs the
    same bits, and the same bits again from every paged and every NaN-poisoned cache"""
    monkeypatch.setenv("FA_DECODE256_UNIT", unit)
    _, Hkv, Sq = shape
    for window in WINDOWS:
        one = None
        for ns in (1, 3, 16, 0):
            o, lse = _run(dtype, Hkv, Sq, "contiguous", window, cap, num_splits=ns)
            for b, (o32, lse32, o16) in enumerate(_refs(dtype, Hkv, Sq, window, cap)):
                res = bi.compare(o[b].cpu(), lse[b].cpu(), o32, lse32, o16, dtype)
                assert res["ok"], (window, ns, b, res)
                lo, hi = bi.window_bounds(Sq, LENS[b], *bi.window_sides(*window))
                assert bool((o[b].cpu()[hi < lo] == 0).all()) and bool((lse[b].cpu()[:, hi < lo] == bi.NEG_INF).all()), (window, ns, b)
            one = lse if one is None else one
            assert float(((lse - one).abs() / one.abs().clamp_min(1.0)).nan_to_num(0.0).max()) <= 1e-5, (window, ns)
            for cache in _inputs(dtype)[3]:
                assert _same((o, lse), _run(dtype, Hkv, Sq, cache, window, cap, num_splits=ns)), (window, ns, cache)


def test_a_captured_graph_sees_the_lengths_rewritten_in_place():
    dtype, window, lens = torch.bfloat16, (-1, -1, True), _i32(LENS)
    step = lambda: _run(dtype, 2, 8, "pages of 256", window, 4.0, lens=lens)   # noqa: E731
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        step()   # (warm-up outside the capture)
    torch.cuda.current_stream().wait_stream(stream)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        got = step()
    for new_lens in (LENS, LENS[::-1], [n // 2 for n in LENS], LENS):
        lens.copy_(_i32(new_lens))
        graph.replay()
        torch.cuda.synchronize()
        assert _same(got, step()), new_lens


def test_refusals_on_device_tensors():
    q, (k, v, _), lens = _inputs(torch.bfloat16)[4][:, :1], _inputs(torch.bfloat16)[3]["contiguous"], _i32(LENS)
    with pytest.raises(RuntimeError, match="d_head = 256 only"):
        fa.forward_kvcache_d256(q[..., :128], k[..., :128], v[..., :128], lens)
    with pytest.raises(RuntimeError, match="32 packed query rows"):
        fa.forward_kvcache_d256(torch.zeros((len(LENS), 33, 2, D), dtype=torch.bfloat16, device=DEV), k, v, lens)
    with pytest.raises(ValueError, match="softcap"):
        fa.forward_kvcache_d256(q, k, v, lens, -1.0)
