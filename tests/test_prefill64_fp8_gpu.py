"""Prefill against an fp8 (e4m3fn) KV cache at d_head = 64 on the MI355X: forward_varlen_kvcache_d64(k_descale=,
v_descale=).  The anchor is the 16-bit call: every e4m3 value is exact in bf16 and fp16 and a power-of-two descale commutes with every
rounding on the path, so with unit or power-of-two descales o and lse have the BITS of forward_varlen_kvcache_d64 on the dequantized
cache.  Beside it: general descales against fp32 eager attention per sequence on the dequantized keys with the project's rule
(beacon_inputs.compare: |O - O32| <= max(O_TOL, 2 |O_eager16 - O32|), O_TOL 2^-6 bf16 / 2^-9 fp16, lse within 1e-3, rows without keys
exact), the decode on the same cache, a replayed graph, determinism and the refusals.  One launch of PAIRS: ragged and whole tiles,
several pages, empty sides, more queries than keys, two 256-row blocks."""
import functools

import pytest
import torch

import flash_attention as fa
from tests import beacon_inputs as bi
from tests.test_prefill64_gpu import eager
from tests.test_prefill_kvcache_fp8_gpu import DEV, F8, NAN8, U8, _cu, _dequant, _descales, _form, _lens, _same

pytestmark = pytest.mark.gpu
D, CAP = 64, 1024
PAIRS = [(165, 197), (37, 1000), (1, 777), (300, 100), (0, 300), (200, 0), (64, 64), (513, 582)]   # (len_q, len_k)
LENS_Q, LENS_K, B = [p[0] for p in PAIRS], [p[1] for p in PAIRS], len(PAIRS)
WINDOWS = [(-1, -1, False), (-1, -1, True), (127, 0, False), (64, 64, False)]   # (left, right, causal)
CASES = [pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"]),
         pytest.mark.parametrize("heads", [(8, 2), (4, 4)], ids=["8x2", "4x4"]),
         pytest.mark.parametrize("form", ["contiguous", "page64", "page256"]),
         pytest.mark.parametrize("sunk", [False, True], ids=["plain", "sinks"]),
         pytest.mark.parametrize("window", WINDOWS, ids=str)]


def cases(fn):
    for mark in CASES:
        fn = mark(fn)
    return fn


def _sinks(heads, sunk):
    return torch.linspace(4.0, 7.0, heads[0]).to(DEV) if sunk else None


def _call(q, kc, vc, table, z, window, cu=None, lens=None, max_q=None, **kw):
    return fa.forward_varlen_kvcache_d64(q, kc, vc, _cu(LENS_Q)[0] if cu is None else cu, max(LENS_Q) if max_q is None else max_q,
                                         _lens(LENS_K) if lens is None else lens, z, block_table=table, causal=window[2], window_size=window[:2], **kw)


@functools.lru_cache(maxsize=None)
def _case8(heads):
    """q (fp32, * 3: a row's weight on a handful of keys) and contiguous e4m3fn caches, every row random; shared, never written"""
    gen = torch.Generator().manual_seed(640 + heads[1])
    q = torch.randn((sum(LENS_Q), heads[0], D), generator=gen) * 3
    k8, v8 = (torch.randn((B, CAP, heads[1], D), generator=gen).to(DEV).to(F8) for _ in range(2))
    return q.to(DEV), k8, v8


@functools.lru_cache(maxsize=None)
def _ref16(dtype, heads, sunk, window, mode):
    """the 16-bit call on the dequantized contiguous cache, which is exact in dtype: the bits every fp8 launch must repeat"""
    q, k8, v8 = _case8(heads)
    kd, vd = _descales(mode, heads[1], B)
    k16, v16 = _dequant(k8, kd).to(dtype), _dequant(v8, vd).to(dtype)
    assert torch.equal(k16.float(), _dequant(k8, kd)) and torch.equal(v16.float(), _dequant(v8, vd))
    return _call(q.to(dtype), k16, v16, None, _sinks(heads, sunk), window)


@cases
@pytest.mark.parametrize("mode", ["ones", "pow2"])
def test_the_bits_of_the_16_bit_call_on_the_dequantized_cache(dtype, heads, form, sunk, window, mode):
    q, k8, v8 = _case8(heads)
    kd, vd = _descales(mode, heads[1], B)
    kc, vc, table = _form(form, k8, v8, LENS_K)
    o, lse = _call(q.to(dtype), kc, vc, table, _sinks(heads, sunk), window, k_descale=kd, v_descale=vd)
    o_ref, lse_ref = _ref16(dtype, heads, sunk, window, mode)
    assert o.dtype == dtype and lse.dtype == torch.float32
    assert _same(lse, lse_ref), "lse"
    assert _same(o, o_ref), "o"


@functools.lru_cache(maxsize=None)
def _quantized(heads):
    """q and a cache from quantize_kvcache_fp8: general descales, one per (sequence, head)"""
    gen = torch.Generator().manual_seed(650 + heads[1])
    q = torch.randn((sum(LENS_Q), heads[0], D), generator=gen) * 3
    k8, v8, kd, vd = fa.quantize_kvcache_fp8(*(torch.randn((B, CAP, heads[1], D), generator=gen).to(DEV) * s for s in (1.7, 0.6)))
    assert kd.unique().numel() == B * heads[1]
    return q.to(DEV), k8, v8, kd, vd


@functools.lru_cache(maxsize=None)
def _refs(dtype, heads, sunk, window):
    """(o32, lse32, o16) per sequence on the dequantized keys (quantization error enters no bar); shared, never written"""
    q, k8, v8, kd, vd = _quantized(heads)
    q, kdq, vdq = q.to(dtype).cpu(), _dequant(k8, kd).cpu(), _dequant(v8, vd).cpu()
    z, cu = (torch.linspace(4.0, 7.0, heads[0]) if sunk else None), _cu(LENS_Q)[1]
    seqs = [(q[cu[b]:cu[b + 1]], kdq[b, :n], vdq[b, :n], z, window) for b, n in enumerate(LENS_K)]
    return [eager(*e, torch.float32) + eager(*e, dtype)[:1] for e in seqs]


@cases
def test_general_descales_against_fp32_eager_per_sequence(dtype, heads, form, sunk, window):
    """rows at or beyond len_k and unused pages hold the NaN code, unused table entries junk"""
    q, k8, v8, kd, vd = _quantized(heads)
    kc, vc, table = _form(form, k8, v8, LENS_K, poison=True)
    assert bool((kc.view(U8) == NAN8).any())
    z = _sinks(heads, sunk)
    o, lse = _call(q.to(dtype), kc, vc, table, z, window, k_descale=kd, v_descale=vd)
    cu = _cu(LENS_Q)[1]
    for b, ((nq, nk), (o32, lse32, o16)) in enumerate(zip(PAIRS, _refs(dtype, heads, sunk, window))):
        got_o, got_lse = o[cu[b]:cu[b + 1]].cpu(), lse[:, cu[b]:cu[b + 1]].cpu()
        res = bi.compare(got_o, got_lse, o32, lse32, o16, dtype)
        print(f"seq {b} {(nq, nk)}: |O - O32| = {res['err']:.3e} bound = {res['bound']:.3e}, |lse - lse32| = {res['lse_err']:.3e}")
        assert res["ok"], (nq, nk, res)
        lo, hi = bi.window_bounds(nq, nk, *bi.window_sides(*window))
        want = z.cpu()[:, None] if sunk else torch.full((heads[0], 1), bi.NEG_INF)
        assert bool((got_o[hi < lo] == 0).all()) and torch.equal(got_lse[:, hi < lo], want.expand(-1, int((hi < lo).sum()))), (nq, nk)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("Sq", [1, 5, 16])
def test_agreement_with_decode(dtype, Sq):
    """Sq rows per sequence against forward_kvcache_d64 on the same paged fp8 cache and descales, within the rule"""
    heads, window = (8, 2), (100, -1, True)
    _, k8, v8, kd, vd = _quantized(heads)
    kp, vp, table = _form("page64", k8, v8, LENS_K, poison=True)
    qs = (torch.randn((B, Sq, 8, D), generator=torch.Generator().manual_seed(64)) * 3).to(dtype).to(DEV)
    z, lens = _sinks(heads, True), _lens(LENS_K)
    o, lse = _call(qs.reshape(B * Sq, 8, D), kp, vp, table, z, window, cu=_cu([Sq] * B)[0], lens=lens, max_q=Sq, k_descale=kd, v_descale=vd)
    od, lsed = fa.forward_kvcache_d64(qs, kp, vp, lens, z, block_table=table, return_lse=True, causal=True, window_size=window[:2],
                                      k_descale=kd, v_descale=vd)
    o, lse = o.view(B, Sq, 8, D), lse.view(8, B, Sq)
    assert float((lse.permute(1, 0, 2) - lsed).abs().nan_to_num(0.0).max()) <= bi.LSE_TOL
    kdq, vdq = _dequant(k8, kd).cpu(), _dequant(v8, vd).cpu()
    for b, n in enumerate(LENS_K):
        e = (qs[b].cpu(), kdq[b, :n], vdq[b, :n], z.cpu(), window)
        o32, lse32 = eager(*e, torch.float32)
        o16 = eager(*e, dtype)[0]
        assert bi.compare(o[b].cpu(), lse[:, b].cpu(), o32, lse32, o16, dtype)["ok"], b
        assert float((o[b].float() - od[b].float()).abs().max()) <= max(bi.O_TOL[dtype], 2 * float((o16.float() - o32).abs().max())), b


def test_a_graph_replays_lengths_offsets_table_descales_and_sinks_rewritten_in_place():
    dtype, heads, window = torch.bfloat16, (8, 2), (-1, -1, True)
    q, k8, v8, kd0, vd0 = _quantized(heads)
    q = q.to(dtype)
    kp, vp, t0 = _form("page256", k8, v8, [CAP] * B)   # (every page named: any length up to CAP is served)
    z, kd, vd, table = _sinks(heads, True), kd0.clone(), vd0.clone(), t0.clone()   # (made outside the capture)
    cu, lens = _cu(LENS_Q)[0], _lens(LENS_K)
    step = lambda: _call(q, kp, vp, table, z, window, cu=cu, lens=lens, k_descale=kd, v_descale=vd)   # noqa: E731
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        step()   # (warm-up outside the capture)
    torch.cuda.current_stream().wait_stream(stream)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        got = step()
    for lq, lk, shift, scale, flip in ((LENS_Q, LENS_K, 0.0, 1.0, False), (LENS_Q[::-1], LENS_K[::-1], 1.0, 0.5, True),
                                       (LENS_Q, [n // 2 for n in LENS_K], -2.0, 3.0, False), (LENS_Q, LENS_K, 0.0, 1.0, False)):
        cu.copy_(_cu(lq)[0]), lens.copy_(_lens(lk)), z.copy_(_sinks(heads, True) + shift), kd.copy_(kd0 * scale), vd.copy_(vd0 / scale)
        table.copy_(t0.flip(0) if flip else t0)
        graph.replay()
        torch.cuda.synchronize()
        assert all(_same(a, b) for a, b in zip(got, step())), (lq, lk)


def test_two_calls_give_the_same_bits():
    q, k8, v8, kd, vd = _quantized((8, 2))
    kc, vc, table = _form("page64", k8, v8, LENS_K)
    a, b = (_call(q.to(torch.bfloat16), kc, vc, table, _sinks((8, 2), True), (127, 0, False), k_descale=kd, v_descale=vd) for _ in range(2))
    assert _same(a[0], b[0]) and _same(a[1], b[1])


def test_refusals_on_device_tensors():
    q = torch.zeros((8, 4, D), dtype=torch.bfloat16, device=DEV)
    cu, lens = _lens([0, 4, 8]), _lens([4, 4])
    cache = torch.zeros((2, 128, 2, D), dtype=torch.bfloat16, device=DEV)
    c8, ones, fn = cache.to(F8), torch.ones((2, 2), device=DEV), fa.forward_varlen_kvcache_d64
    for kw in (dict(), dict(k_descale=ones), dict(v_descale=ones)):
        with pytest.raises(RuntimeError, match="fp8 cache is not served without both.*pass ones"):
            fn(q, c8, c8, cu, 4, lens, **kw)
    with pytest.raises(RuntimeError, match="belong to an fp8"):
        fn(q, cache, cache, cu, 4, lens, k_descale=ones, v_descale=ones)
    with pytest.raises(RuntimeError, match="must be torch.float8_e4m3fn"):
        fn(q, cache.to(torch.float8_e5m2), cache.to(torch.float8_e5m2), cu, 4, lens, k_descale=ones, v_descale=ones)
    with pytest.raises(RuntimeError, match="one data type"):
        fn(q, c8, cache, cu, 4, lens, k_descale=ones, v_descale=ones)
    for bad in (ones.double(), torch.ones((3, 2), device=DEV), ones.cpu()):   # dtype, shape, device
        with pytest.raises(RuntimeError, match="k_descale must be"):
            fn(q, c8, c8, cu, 4, lens, k_descale=bad, v_descale=ones)
    with pytest.raises(RuntimeError, match="multiple of 64"):
        fn(q, c8.view(8, 32, 2, D), c8.view(8, 32, 2, D), cu, 4, lens, block_table=torch.zeros((2, 4), dtype=torch.int32, device=DEV),
           k_descale=ones, v_descale=ones)
