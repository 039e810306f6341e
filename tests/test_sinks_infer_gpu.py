"""Attention sinks in KV-cache decode and cache prefill on the MI355X: forward_kvcache_sinks and
forward_varlen_kvcache_sinks, 16-bit and fp8 cache, contiguous and pages of 64.  The oracle is sinks_inputs.sink_attention per batch
entry or sequence, fp32 and 16-bit eager, on the dequantized cache for fp8; the pass rule is beacon_inputs.compare (O_TOL / LSE_TOL),
rows that see no key exact: o = 0, lse = z."""
import functools
import itertools

import pytest
import torch

import beacon_inputs as bi
import flash_attention as fa
import sinks_inputs as sk
import softcap_infer_inputs as si

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CASES = pytest.mark.parametrize("dtype,fp8", list(itertools.product(si.DTYPES, (False, True))), ids=lambda x: str(x).replace("torch.", ""))
Z = sk.SINKS_LIVE(si.HEADS[0])
_i32 = functools.partial(torch.tensor, dtype=torch.int32, device=DEV)


def _same(a, b):
    return all(x.shape == y.shape and torch.equal(x.contiguous().view(torch.uint8), y.contiguous().view(torch.uint8)) for x, y in zip(a, b))


def _kw(window):
    return dict(window_size=window[:2], causal=window[2])


def _caches(inp, cache):
    k, v, kw = inp["k"].to(DEV), inp["v"].to(DEV), {}
    if cache is not None:
        k, v, kw = cache["k8"].to(DEV), cache["v8"].to(DEV), dict(k_descale=cache["kd"].to(DEV), v_descale=cache["vd"].to(DEV))
    kp, vp, table = si.paginate(k, v, 64)
    return [(k, v, kw), (kp, vp, dict(block_table=table, **kw))]


@functools.lru_cache(maxsize=None)
def _refs(kind, dtype, Sq, window, fp8):
    """(o32, lse32, o16) per entry under Z; shared, never written to"""
    inp = si.decode_inputs(dtype, Sq) if kind == "decode" else si.prefill_inputs(dtype)
    qkv = [si.entry(inp, b, si.fp8_cache(kind, dtype, Sq) if fp8 else None) for b in range(len(inp["lens"]))]
    return [sk.sink_attention(*e, Z, window, torch.float32) + sk.sink_attention(*e, Z, window, dtype)[:1] for e in qkv]


def _check(tag, o, lse, cu, refs, dtype, window, n_keys):
    """o (rows, H, 128), lse (H, rows), entry b at rows cu[b] .. cu[b + 1] - 1"""
    for b, (o32, lse32, o16) in enumerate(refs):
        ob, lb = o[cu[b]:cu[b + 1]].cpu(), lse[:, cu[b]:cu[b + 1]].cpu()
        res = bi.compare(ob, lb, o32, lse32, o16, dtype)
        assert res["ok"], (tag, b, res)
        lo, hi = bi.window_bounds(ob.shape[0], n_keys[b], *bi.window_sides(*window))
        dead = hi < lo   # rows that see no key: the sink is the softmax's only member
        assert bool((ob[dead] == 0).all()) and torch.equal(lb[:, dead], Z[:, None].expand(-1, int(dead.sum()))), (tag, b)


def _prefill(inp, k, v, kw, window):
    return fa.forward_varlen_kvcache_sinks(inp["q"].to(DEV), k, v, _i32(inp["cu_q"]), max(p[0] for p in si.PREFILL_PAIRS), _i32(inp["lens"]),
                                           Z.to(DEV), **_kw(window), **kw)


@CASES
@pytest.mark.parametrize("Sq", [1, 8, 16])
def test_decode_parity_and_every_split_count_counts_the_sink_once(dtype, fp8, Sq):
    """4, 32 and 64 packed rows; num_splits 1, 3, 16 and the rule's: lse of every split count is one split's to fp32 rounding (a sink
    per split, or none, misses by log(splits) or by log(1 + exp(z - lse))); the prefill on the same rows is within the rule too"""
    inp = si.decode_inputs(dtype, Sq)
    B, q, lens = len(inp["lens"]), inp["q"].to(DEV), _i32(inp["lens"])
    cu = list(range(0, (B + 1) * Sq, Sq))
    for window in si.WINDOWS:
        refs = _refs("decode", dtype, Sq, window, fp8)
        for k, v, kw in _caches(inp, si.fp8_cache("decode", dtype, Sq) if fp8 else None):
            one = None
            for ns in (1, 3, 16, 0):
                o, lse = fa.forward_kvcache_sinks(q, k, v, lens, Z.to(DEV), return_lse=True, num_splits=ns, **_kw(window), **kw)
                _check(f"decode {window} splits={ns}", o.flatten(0, 1), lse.permute(1, 0, 2).flatten(1), cu, refs, dtype, window, inp["lens"])
                one = lse if one is None else one
                assert float(((lse - one).abs() / one.abs().clamp_min(1.0)).max()) <= 1e-5, (window, ns)
            o, lse = fa.forward_varlen_kvcache_sinks(q.flatten(0, 1), k, v, _i32(cu), Sq, lens, Z.to(DEV), **_kw(window), **kw)
            _check(f"prefill on decode's rows {window}", o, lse, cu, refs, dtype, window, inp["lens"])


@CASES
def test_decode_edge_sinks(dtype, fp8):
    """z = +120 (head 0): o = 0, lse = 120; z = -120 and -inf (heads 1, 2): forward_kvcache's values; no NaN; no key, no sink: -inf"""
    inp, window = si.decode_inputs(dtype, 8), si.WINDOWS[2]
    q, lens = inp["q"].to(DEV), _i32(inp["lens"])
    for (k, v, kw), ns in itertools.product(_caches(inp, si.fp8_cache("decode", dtype, 8) if fp8 else None), (1, 3)):
        o, lse = fa.forward_kvcache_sinks(q, k, v, lens, sk.SINKS_EDGE(8).to(DEV), return_lse=True, num_splits=ns, **_kw(window), **kw)
        o0, lse0 = fa.forward_kvcache(q, k, v, lens, return_lse=True, num_splits=ns, **_kw(window), **kw)
        assert not bool(torch.isnan(o.float()).any()) and not bool(torch.isnan(lse).any())
        assert bool((o[:, :, 0] == 0).all()) and float((lse[:, 0] - 120.0).abs().max()) <= bi.LSE_TOL
        assert float((o[:, :, 1:3].float() - o0[:, :, 1:3].float()).abs().max()) <= bi.O_TOL[dtype]
        live = lse0[:, 1:3] != bi.NEG_INF
        assert float((lse[:, 1:3][live] - lse0[:, 1:3][live]).abs().max()) <= bi.LSE_TOL
        assert inp["lens"][0] == 0 and bool((lse[0, 2] == bi.NEG_INF).all()) and bool((lse[0, 1] == -120.0).all())


@CASES
def test_the_fused_step_is_append_then_decode_and_a_captured_graph_sees_sinks_rewritten_in_place(dtype, fp8):
    inp, gen = si.decode_inputs(dtype, 1), torch.Generator().manual_seed(7100)
    kc0, vc0, kw = _caches(inp, si.fp8_cache("decode", dtype, 1) if fp8 else None)[1]
    pos = torch.arange(si.DECODE_CACHE_LEN, dtype=torch.float32)[:, None] * 10000.0 ** (-torch.arange(32, dtype=torch.float32) / 32)[None, :]
    rot = dict(rotary_cos=torch.cos(pos).to(dtype).to(DEV), rotary_sin=torch.sin(pos).to(dtype).to(DEV))
    call = dict(causal=True, window_size=(100, -1), return_lse=True, **kw)
    zs = [Z, sk.SINKS_EDGE(8), Z + 1.0]
    feeds = [[torch.randn((len(si.DECODE_LENGTHS), 1, h, si.D), generator=gen).to(dtype).to(DEV) for h in (8, 2, 2)] for _ in zs]
    # eager: append_kvcache, then the decode with sinks, three tokens
    kc_e, vc_e, lens_e, want = kc0.clone(), vc0.clone(), _i32(si.DECODE_LENGTHS), []
    for (q, k, v), z in zip(feeds, zs):
        lens_e, q_rot = fa.append_kvcache(kc_e, vc_e, k, v, lens_e, block_table=kw["block_table"], q=q, causal=True, k_descale=kw.get("k_descale"),
                                          v_descale=kw.get("v_descale"), **rot)
        want.append(fa.forward_kvcache_sinks(q_rot, kc_e, vc_e, lens_e, z.to(DEV), **call))
    # one captured graph of the fused step, replayed with sinks rewritten in place
    kc_g, vc_g, lens_g, z_g = kc0.clone(), vc0.clone(), _i32(si.DECODE_LENGTHS), Z.to(DEV)
    q_s, k_s, v_s = (t.clone() for t in feeds[0])
    step = lambda: fa.forward_kvcache_sinks(q_s, kc_g, vc_g, lens_g, z_g, k=k_s, v=v_s, advance_seqlens=True, **rot, **call)   # noqa: E731
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        assert _same(step(), want[0])   # (warm-up outside the capture, and the fused call's own bits)
    torch.cuda.current_stream().wait_stream(stream)
    graph = torch.cuda.CUDAGraph()
    for capture in (True, False):   # (the warm-up's append is undone, then the capture's own)
        kc_g.copy_(kc0), vc_g.copy_(vc0), lens_g.copy_(_i32(si.DECODE_LENGTHS))
        if capture:
            with torch.cuda.graph(graph):
                got = step()
    for i, ((q, k, v), z) in enumerate(zip(feeds, zs)):
        q_s.copy_(q), k_s.copy_(k), v_s.copy_(v), z_g.copy_(z)
        graph.replay()
        torch.cuda.synchronize()
        assert _same(got, want[i]), i
    assert _same((kc_g, vc_g), (kc_e, vc_e)) and lens_g.tolist() == lens_e.tolist()


@CASES
def test_prefill_parity_and_bit_identities(dtype, fp8):
    inp = si.prefill_inputs(dtype)
    pow2 = si.fp8_cache("prefill", dtype, pow2=True)
    for window in si.WINDOWS:
        for k, v, kw in _caches(inp, si.fp8_cache("prefill", dtype) if fp8 else None):
            o, lse = _prefill(inp, k, v, kw, window)
            _check(f"prefill {window}", o, lse, inp["cu_q"], _refs("prefill", dtype, 1, window, fp8), dtype, window, inp["lens"])
            assert _same((o, lse), _prefill(inp, k, v, kw, window))   # two runs, the same bits
        if not fp8:   # the packed forward with sinks on the same keys gathered
            kg, vg = (torch.cat([inp[n][b, :m] for b, m in enumerate(inp["lens"])]).to(DEV) for n in ("k", "v"))
            packed = fa.forward_varlen_sinks(inp["q"].to(DEV), kg, vg, _i32(inp["cu_q"]), max(p[0] for p in si.PREFILL_PAIRS), Z.to(DEV),
                                             cu_seqlens_k=_i32([0] + list(itertools.accumulate(inp["lens"]))), max_seqlen_k=max(inp["lens"]), **_kw(window))
            assert _same((o, lse), packed), window
        else:     # power-of-two descales: the 16-bit call on the dequantized cache
            o16 = _prefill(inp, pow2["k"].to(dtype).to(DEV), pow2["v"].to(dtype).to(DEV), {}, window)
            o8 = _prefill(inp, pow2["k8"].to(DEV), pow2["v8"].to(DEV), dict(k_descale=pow2["kd"].to(DEV), v_descale=pow2["vd"].to(DEV)), window)
            assert _same(o8, o16), window


def test_refusals_on_device_tensors():
    inp = si.decode_inputs(torch.bfloat16, 8)
    q, k, v, lens, z = inp["q"].to(DEV), inp["k"].to(DEV), inp["v"].to(DEV), _i32(inp["lens"]), Z.to(DEV)
    for bad in (None, Z, z.double(), z[:4], z.repeat(2)[::2]):   # not a tensor, the CPU's, fp64, 4 heads, strided
        with pytest.raises(RuntimeError, match="sinks"):
            fa.forward_kvcache_sinks(q, k, v, lens, bad)
        with pytest.raises(RuntimeError, match="sinks"):
            fa.forward_varlen_kvcache_sinks(q.flatten(0, 1), k, v, _i32(list(range(0, 64, 8))), 8, lens, bad)
    with pytest.raises(ValueError, match="causal means right = 0"):   # a bad window first
        fa.forward_kvcache_sinks(q, k, v, lens, None, causal=True, window_size=(5, 3))
    with pytest.raises(RuntimeError, match="64 packed query rows"):   # the sibling's refusal, in its words
        fa.forward_kvcache_sinks(torch.zeros((7, 17, 8, 128), dtype=torch.bfloat16, device=DEV), k, v, lens, z)
