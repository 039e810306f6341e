"""Logit soft-capping in KV-cache decode and cache prefill on the MI355X: flash_attention.forward_kvcache_softcap and
flash_attention.forward_varlen_kvcache(softcap=), 16-bit and fp8 cache, contiguous and paged.

The oracle is softcap_inputs.capped_attention per batch entry (tests/softcap_infer_inputs.py): fp32 eager with the cap before the
mask, on the dequantized cache for fp8.  The tolerance rule is beacon_inputs.compare: max|O - O32| <= max(O_TOL[dtype],
2 max|O_eager16 - O32|), lse 1e-3 absolute, -inf exactly for rows that see no key.  tests/test_softcap_infer_cpu.py proves that
caps 0.5 and 4.0 discriminate on these inputs (a missing cap, and for fp8 a cap of the raw undescaled score, miss the rule by 2x at
least); 50.0 asks for accuracy near 0 only.  The bit-identity tests fail on a wrong kernel far below any tolerance."""
import math

import pytest
import torch

import beacon_inputs as bi
import softcap_infer_inputs as si

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
IDS = ["bf16", "fp16"]
NAN_CODE = 0x7F   # e4m3fn's NaN


def _fa():
    import flash_attention
    return flash_attention


@pytest.fixture(autouse=True)
def _no_tf32():
    old = torch.backends.cuda.matmul.allow_tf32
    torch.backends.cuda.matmul.allow_tf32 = False
    yield
    torch.backends.cuda.matmul.allow_tf32 = old


def _bits(t):
    return t.view({1: torch.uint8, 2: torch.int16, 4: torch.int32}[t.element_size()])


def _same(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _lens(lens):
    return torch.tensor(lens, dtype=torch.int32, device=DEV)


def _window_kw(window):
    left, right, causal = window
    return dict(window_size=(left, right), causal=causal)


def _caches(inp, fp8_cache):
    """-> [(name, k, v, keyword arguments of the cache)]: contiguous and pages of 64 and 256, on the device"""
    kw = {}
    if fp8_cache is not None:
        k, v = fp8_cache["k8"].to(DEV), fp8_cache["v8"].to(DEV)
        kw = dict(k_descale=fp8_cache["kd"].to(DEV), v_descale=fp8_cache["vd"].to(DEV))
    else:
        k, v = inp["k"].to(DEV), inp["v"].to(DEV)
    out = [("contiguous", k, v, kw)]
    for page in si.PAGE_SIZES:
        kp, vp, table = si.paginate(k, v, page)
        out.append((f"page{page}", kp, vp, dict(block_table=table, **kw)))
    return out


def _check_entries(tag, o_entries, lse_entries, refs, dtype, stats):
    """bi.compare per entry; a row that sees no key: o = 0 and lse = -inf exactly"""
    for b, (o, lse, r) in enumerate(zip(o_entries, lse_entries, refs)):
        res = bi.compare(o, lse, r["o32"], r["lse32"], r["o16"], dtype)
        stats["ratio"] = max(stats.get("ratio", 0.0), res["err"] / res["bound"])
        stats["lse"] = max(stats.get("lse", 0.0), res["lse_err"])
        assert res["ok"], (tag, b, res)
        dead = r["lse32"] == bi.NEG_INF                         # (H, n_q)
        if bool(dead.any()):
            assert bool((o.float().permute(1, 0, 2)[dead] == 0).all()), (tag, b)
            assert bool((lse[dead] == bi.NEG_INF).all()), (tag, b)


def _decode_entries(o, lse):
    o, lse = o.cpu(), lse.cpu()
    return list(o), list(lse)                                    # o[b] (Sq, H, 128), lse[b] (H, Sq)


def _prefill_entries(o, lse, cu_q):
    o, lse = o.cpu(), lse.cpu()
    return [o[a:b] for a, b in zip(cu_q, cu_q[1:])], [lse[:, a:b] for a, b in zip(cu_q, cu_q[1:])]


def _prefill_call(fa, inp, k, v, kw, window=(-1, -1, False), softcap=0.0, with_softcap=True):
    cu = torch.tensor(inp["cu_q"], dtype=torch.int32, device=DEV)
    max_q = max(b - a for a, b in zip(inp["cu_q"], inp["cu_q"][1:]))
    more = dict(softcap=softcap) if with_softcap else {}
    return fa.forward_varlen_kvcache(inp["q"].to(DEV), k, v, cu, max_q, _lens(inp["lens"]), **_window_kw(window), **kw, **more)


# ---- 1: parity ----------------------------------------------------------------------------------------------------------------------

DECODE_SHAPES = [(Sq, si.HEADS) for Sq in si.DECODE_SEQLENS_Q] + [(8, si.HEADS_64)]   # 4, 16, 32 and 64 packed rows
ALL_CAPS = si.CAPS + [si.LINEAR_CAP]


@pytest.mark.parametrize("dtype", si.DTYPES, ids=IDS)
@pytest.mark.parametrize("fp8", [False, True], ids=["16bit", "fp8"])
@pytest.mark.parametrize("Sq,heads", DECODE_SHAPES, ids=[f"Sq{Sq}-H{h[0]}-{h[1]}" for Sq, h in DECODE_SHAPES])
def test_decode_against_fp32_eager(dtype, fp8, Sq, heads):
    fa = _fa()
    inp = si.decode_inputs(dtype, Sq, heads)
    caches = _caches(inp, si.fp8_cache("decode", dtype, Sq, heads) if fp8 else None)
    q, lens_t = inp["q"].to(DEV), _lens(inp["lens"])
    stats = {}
    for window in si.WINDOWS:
        for cap in ALL_CAPS:
            refs = si.decode_reference(dtype, Sq, window, cap, fp8, heads)
            for name, k, v, kw in caches:
                o, lse = fa.forward_kvcache_softcap(q, k, v, lens_t, cap, return_lse=True, **_window_kw(window), **kw)
                _check_entries(f"decode {name} {window} cap={cap}", *_decode_entries(o, lse), refs, dtype, stats)
    print(f"decode {dtype} fp8={fp8} Sq={Sq} heads={heads}: worst err / bound {stats['ratio']:.3f}, worst |lse - lse32| {stats['lse']:.2e}")


@pytest.mark.parametrize("dtype", si.DTYPES, ids=IDS)
@pytest.mark.parametrize("fp8", [False, True], ids=["16bit", "fp8"])
def test_prefill_against_fp32_eager(dtype, fp8):
    fa = _fa()
    inp = si.prefill_inputs(dtype)
    caches = _caches(inp, si.fp8_cache("prefill", dtype) if fp8 else None)
    stats = {}
    for window in si.WINDOWS:
        for cap in ALL_CAPS:
            refs = si.prefill_reference(dtype, window, cap, fp8)
            for name, k, v, kw in caches:
                o, lse = _prefill_call(fa, inp, k, v, kw, window, cap)
                _check_entries(f"prefill {name} {window} cap={cap}", *_prefill_entries(o, lse, inp["cu_q"]), refs, dtype, stats)
    print(f"prefill {dtype} fp8={fp8}: worst err / bound {stats['ratio']:.3f}, worst |lse - lse32| {stats['lse']:.2e}")


# ---- 2: bit identity ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", si.DTYPES, ids=IDS)
@pytest.mark.parametrize("window", si.WINDOWS, ids=str)
def test_the_16_bit_prefill_is_the_packed_forward_on_the_same_keys_gathered(dtype, window):
    fa = _fa()
    inp = si.prefill_inputs(dtype)
    cu_k = [0]
    for n in inp["lens"]:
        cu_k.append(cu_k[-1] + n)
    k = torch.cat([inp["k"][b, :n] for b, n in enumerate(inp["lens"])]).to(DEV)
    v = torch.cat([inp["v"][b, :n] for b, n in enumerate(inp["lens"])]).to(DEV)
    cu_q = torch.tensor(inp["cu_q"], dtype=torch.int32, device=DEV)
    max_q = max(p[0] for p in si.PREFILL_PAIRS)
    for cap in si.CAPS:
        o_p, lse_p = fa.forward_varlen(inp["q"].to(DEV), k, v, cu_q, max_q, cu_seqlens_k=torch.tensor(cu_k, dtype=torch.int32, device=DEV),
                                       max_seqlen_k=max(inp["lens"]), softcap=cap, **_window_kw(window))
        for name, kc, vc, kw in _caches(inp, None):
            o, lse = _prefill_call(fa, inp, kc, vc, kw, window, cap)
            assert _same(o, o_p) and _same(lse, lse_p), (name, cap)


@pytest.mark.parametrize("dtype", si.DTYPES, ids=IDS)
@pytest.mark.parametrize("window", [si.WINDOWS[0], si.WINDOWS[2]], ids=str)
def test_the_fp8_prefill_with_power_of_two_descales_is_the_16_bit_prefill_on_the_dequantized_cache(dtype, window):
    """a power-of-two descale commutes with every rounding: S k_descale is exact, so cap_k = k_descale (2 log2 e / A) applied to the
    raw S gives the 16-bit form's tanh argument bit for bit, and v_descale folded into 1 / l scales the fp32 P V sums exactly"""
    fa = _fa()
    inp = si.prefill_inputs(dtype)
    c = si.fp8_cache("prefill", dtype, pow2=True)
    k16, v16 = c["k"].to(dtype), c["v"].to(dtype)
    assert torch.equal(k16.float(), c["k"]) and torch.equal(v16.float(), c["v"])   # (the dequantized values are exact in the 16-bit type)
    scales = dict(k_descale=c["kd"].to(DEV), v_descale=c["vd"].to(DEV))
    for cap in si.CAPS:
        o16, lse16 = _prefill_call(fa, inp, k16.to(DEV), v16.to(DEV), {}, window, cap)
        o8, lse8 = _prefill_call(fa, inp, c["k8"].to(DEV), c["v8"].to(DEV), scales, window, cap)
        assert _same(o8, o16) and _same(lse8, lse16), cap


@pytest.mark.parametrize("dtype", si.DTYPES, ids=IDS)
@pytest.mark.parametrize("fp8", [False, True], ids=["16bit", "fp8"])
def test_softcap_zero_is_the_call_without_it_and_two_runs_give_the_same_bits(dtype, fp8):
    fa = _fa()
    window = si.WINDOWS[2]
    inp = si.decode_inputs(dtype, 4)
    name, k, v, kw = _caches(inp, si.fp8_cache("decode", dtype, 4) if fp8 else None)[1]
    q, lens_t = inp["q"].to(DEV), _lens(inp["lens"])
    for w in (si.WINDOWS[0], window):
        base = fa.forward_kvcache(q, k, v, lens_t, return_lse=True, **_window_kw(w), **kw)
        for zero in (0.0, 0):
            got = fa.forward_kvcache_softcap(q, k, v, lens_t, zero, return_lse=True, **_window_kw(w), **kw)
            assert _same(got[0], base[0]) and _same(got[1], base[1])
    a = fa.forward_kvcache_softcap(q, k, v, lens_t, 4.0, return_lse=True, num_splits=3, **_window_kw(window), **kw)
    b = fa.forward_kvcache_softcap(q, k, v, lens_t, 4.0, return_lse=True, num_splits=3, **_window_kw(window), **kw)
    assert _same(a[0], b[0]) and _same(a[1], b[1])
    assert not _same(a[0], base[0])   # (and the cap is not a no-op)
    inp = si.prefill_inputs(dtype)
    name, k, v, kw = _caches(inp, si.fp8_cache("prefill", dtype) if fp8 else None)[2]
    for w in (si.WINDOWS[0], window):
        base = _prefill_call(fa, inp, k, v, kw, w, with_softcap=False)
        for zero in (0.0, 0):
            got = _prefill_call(fa, inp, k, v, kw, w, zero)
            assert _same(got[0], base[0]) and _same(got[1], base[1])
    a, b = _prefill_call(fa, inp, k, v, kw, window, 4.0), _prefill_call(fa, inp, k, v, kw, window, 4.0)
    assert _same(a[0], b[0]) and _same(a[1], b[1])
    assert not _same(a[0], base[0])


def _rotary(dtype, n, dim=64):
    pos = torch.arange(n, dtype=torch.float32)[:, None]
    freq = 10000.0 ** (-torch.arange(dim // 2, dtype=torch.float32) / (dim // 2))[None, :]
    return torch.cos(pos * freq).to(dtype).to(DEV), torch.sin(pos * freq).to(dtype).to(DEV)


def _step_feed(dtype, B, heads, seed):
    gen = torch.Generator().manual_seed(7000 + seed)
    q = torch.randn((B, 1, heads[0], si.D), generator=gen).to(dtype).to(DEV)
    k = torch.randn((B, 1, heads[1], si.D), generator=gen).to(dtype).to(DEV)
    v = torch.randn((B, 1, heads[1], si.D), generator=gen).to(dtype).to(DEV)
    return q, k, v


STEP_LENS = [0, 1, 31, 64, 65, 300, 1000]


@pytest.mark.parametrize("dtype", si.DTYPES, ids=IDS)
@pytest.mark.parametrize("fp8", [False, True], ids=["16bit", "fp8"])
def test_the_fused_append_is_the_append_followed_by_the_capped_decode(dtype, fp8):
    """forward_kvcache_softcap(k=, v=, rotary ...) against append_kvcache followed by forward_kvcache_softcap: the append is unchanged,
    the cap belongs to the attention only"""
    fa = _fa()
    inp = si.decode_inputs(dtype, 1)
    name, kc, vc, kw = _caches(inp, si.fp8_cache("decode", dtype, 1) if fp8 else None)[1]   # (pages of 64)
    cos, sin = _rotary(dtype, si.DECODE_CACHE_LEN)
    q, k, v = _step_feed(dtype, len(STEP_LENS), si.HEADS, 0)
    call = dict(causal=True, window_size=(100, -1), return_lse=True, **kw)
    kc1, vc1, lens1 = kc.clone(), vc.clone(), _lens(STEP_LENS)
    o1, lse1 = fa.forward_kvcache_softcap(q, kc1, vc1, lens1, 4.0, k=k, v=v, rotary_cos=cos, rotary_sin=sin, **call)
    kc2, vc2, lens2 = kc.clone(), vc.clone(), _lens(STEP_LENS)
    new_lens, q_rot = fa.append_kvcache(kc2, vc2, k, v, lens2, block_table=kw["block_table"], q=q, rotary_cos=cos, rotary_sin=sin, causal=True,
                                        k_descale=kw.get("k_descale"), v_descale=kw.get("v_descale"))
    o2, lse2 = fa.forward_kvcache_softcap(q_rot, kc2, vc2, new_lens, 4.0, **call)
    assert _same(kc1, kc2) and _same(vc1, vc2) and lens1.tolist() == STEP_LENS
    assert _same(o1, o2) and _same(lse1, lse2)
    o3, _ = fa.forward_kvcache(q_rot, kc2, vc2, new_lens, **call)
    assert not _same(o1, o3)


# ---- 3: decode and prefill agree; forced splits -----------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", si.DTYPES, ids=IDS)
@pytest.mark.parametrize("fp8", [False, True], ids=["16bit", "fp8"])
def test_decode_and_prefill_agree_on_the_same_rows(dtype, fp8):
    """the same rows, cap and cache through both calls: each within the rule of the fp32 reference, so their difference within the
    two bounds' sum (the triangle inequality; nothing measured went into it), lse within twice the rule's 1e-3"""
    fa = _fa()
    Sq = 4
    inp = si.decode_inputs(dtype, Sq)
    B = len(inp["lens"])
    q, lens_t = inp["q"].to(DEV), _lens(inp["lens"])
    cu = torch.arange(0, (B + 1) * Sq, Sq, dtype=torch.int32, device=DEV)
    for window in si.WINDOWS:
        for cap in si.CAPS:
            refs = si.decode_reference(dtype, Sq, window, cap, fp8)
            for name, k, v, kw in _caches(inp, si.fp8_cache("decode", dtype, Sq) if fp8 else None)[:2]:
                if fp8:   # (the prefill refuses an fp8 cache without both descales; both are given here)
                    assert "k_descale" in kw and "v_descale" in kw
                o_d, lse_d = fa.forward_kvcache_softcap(q, k, v, lens_t, cap, return_lse=True, **_window_kw(window), **kw)
                o_p, lse_p = fa.forward_varlen_kvcache(q.reshape(B * Sq, *q.shape[2:]), k, v, cu, Sq, lens_t, softcap=cap, **_window_kw(window), **kw)
                o_p, lse_p = o_p.reshape(B, Sq, *o_p.shape[1:]).cpu(), lse_p.reshape(-1, B, Sq).permute(1, 0, 2).cpu()
                o_d, lse_d = o_d.cpu(), lse_d.cpu()
                for b, r in enumerate(refs):
                    res_d = bi.compare(o_d[b], lse_d[b], r["o32"], r["lse32"], r["o16"], dtype)
                    res_p = bi.compare(o_p[b], lse_p[b], r["o32"], r["lse32"], r["o16"], dtype)
                    assert res_d["ok"] and res_p["ok"], (name, window, cap, b, res_d, res_p)
                    assert (o_d[b].float() - o_p[b].float()).abs().max().item() <= res_d["bound"] + res_p["bound"]
                    live = r["lse32"] != bi.NEG_INF
                    assert torch.equal(lse_d[b] == bi.NEG_INF, ~live) and torch.equal(lse_p[b] == bi.NEG_INF, ~live)
                    if bool(live.any()):
                        assert (lse_d[b][live] - lse_p[b][live]).abs().max().item() <= 2 * bi.LSE_TOL


@pytest.mark.parametrize("dtype", si.DTYPES, ids=IDS)
@pytest.mark.parametrize("fp8", [False, True], ids=["16bit", "fp8"])
def test_forced_splits(dtype, fp8):
    """num_splits 1, 3 and 16 (length 1000 is in the batch): o within the rule, lse agreeing to 1e-5 relative, as the window test does"""
    fa = _fa()
    Sq, window, cap = 4, si.WINDOWS[1], 4.0
    inp = si.decode_inputs(dtype, Sq)
    assert 1000 in inp["lens"]
    refs = si.decode_reference(dtype, Sq, window, cap, fp8)
    q, lens_t = inp["q"].to(DEV), _lens(inp["lens"])
    for name, k, v, kw in _caches(inp, si.fp8_cache("decode", dtype, Sq) if fp8 else None)[::2]:
        base = None
        for ns in (1, 3, 16):
            o, lse = fa.forward_kvcache_softcap(q, k, v, lens_t, cap, return_lse=True, num_splits=ns, **_window_kw(window), **kw)
            _check_entries(f"splits={ns} {name}", *_decode_entries(o, lse), refs, dtype, {})
            lse = lse.cpu()
            if base is None:
                base = lse
                continue
            live = base != bi.NEG_INF
            assert torch.equal(lse == bi.NEG_INF, ~live)
            rel = ((lse[live] - base[live]).abs() / base[live].abs().clamp_min(1.0)).max().item()
            print(f"{name} splits={ns}: max rel |lse - lse(1 split)| = {rel:.3e}")
            assert rel <= 1e-5, (ns, rel)


# ---- 4: isolation under the cap ---------------------------------------------------------------------------------------------------

def _poison_below(t, lens, n_q, left, nan):
    """NaN in every cache row below each entry's lo_min"""
    out = t.clone()
    raw = out.view(torch.uint8) if out.element_size() == 1 else out
    for b, n in enumerate(lens):
        raw[b, :si.lo_min(n, n_q[b], left)] = nan
    return out


def _paginate_poisoned(k, v, lens, n_q, left, page, nan):
    """the poisoned caches in pages; every table entry of a page wholly below lo_min points at a page of NaN"""
    kp, vp, table = si.paginate(k, v, page)
    dead = min(set(range(kp.shape[0])) - set(table.flatten().tolist()))   # (the paginator leaves three pages unused)
    for t in (kp, vp):
        (t.view(torch.uint8) if t.element_size() == 1 else t)[dead] = nan
    for b, n in enumerate(lens):
        table[b, :si.lo_min(n, n_q[b], left) // page] = dead
    return kp, vp, table


@pytest.mark.parametrize("fp8", [False, True], ids=["16bit", "fp8"])
def test_isolation_under_the_cap(fp8):
    """NaN in every cache row below lo_min, and table entries of pages wholly below it pointed at a NaN page, give the clean run's
    bits in both calls: tanh(NaN) does not get in"""
    fa = _fa()
    dtype, left, cap = torch.bfloat16, 100, 4.0
    nan = NAN_CODE if fp8 else math.nan
    kw_w = dict(window_size=(left, -1), causal=True)
    # decode
    Sq = 4
    inp = si.decode_inputs(dtype, Sq)
    name, k, v, kw = _caches(inp, si.fp8_cache("decode", dtype, Sq) if fp8 else None)[0]
    q, lens_t, n_q = inp["q"].to(DEV), _lens(inp["lens"]), [Sq] * len(inp["lens"])
    clean = fa.forward_kvcache_softcap(q, k, v, lens_t, cap, return_lse=True, **kw_w, **kw)
    kn, vn = _poison_below(k, inp["lens"], n_q, left, nan), _poison_below(v, inp["lens"], n_q, left, nan)
    assert not _same(kn, k)   # (the poison is there: length 1000 has lo_min 896)
    got = fa.forward_kvcache_softcap(q, kn, vn, lens_t, cap, return_lse=True, **kw_w, **kw)
    assert bool(torch.isfinite(got[0].float()).all()) and _same(got[0], clean[0]) and _same(got[1], clean[1])
    for page in si.PAGE_SIZES:
        kp, vp, table = _paginate_poisoned(kn, vn, inp["lens"], n_q, left, page, nan)
        got = fa.forward_kvcache_softcap(q, kp, vp, lens_t, cap, return_lse=True, block_table=table, **kw_w, **kw)
        assert bool(torch.isfinite(got[0].float()).all()) and _same(got[0], clean[0]) and _same(got[1], clean[1]), page
    # prefill
    inp = si.prefill_inputs(dtype)
    name, k, v, kw = _caches(inp, si.fp8_cache("prefill", dtype) if fp8 else None)[0]
    n_q = [p[0] for p in si.PREFILL_PAIRS]
    clean = _prefill_call(fa, inp, k, v, kw, (left, -1, True), cap)
    kn, vn = _poison_below(k, inp["lens"], n_q, left, nan), _poison_below(v, inp["lens"], n_q, left, nan)
    assert not _same(kn, k)   # ((37, 1000): lo_min 863)
    got = _prefill_call(fa, inp, kn, vn, kw, (left, -1, True), cap)
    assert bool(torch.isfinite(got[0].float()).all()) and _same(got[0], clean[0]) and _same(got[1], clean[1])
    for page in si.PAGE_SIZES:
        kp, vp, table = _paginate_poisoned(kn, vn, inp["lens"], n_q, left, page, nan)
        got = _prefill_call(fa, inp, kp, vp, dict(block_table=table, **kw), (left, -1, True), cap)
        assert bool(torch.isfinite(got[0].float()).all()) and _same(got[0], clean[0]) and _same(got[1], clean[1]), page


# ---- 5: saturation ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", si.DTYPES, ids=IDS)
@pytest.mark.parametrize("fp8", [False, True], ids=["16bit", "fp8"])
def test_saturated_logits_stay_finite_and_within_the_rule(dtype, fp8):
    """q scaled by 64: |s| / softcap reaches the hundreds, exp2 overflows to +inf and underflows to 0 -- the logits saturate to
    +- softcap without a NaN, in both calls"""
    fa = _fa()
    Sq, window, cap = 4, si.WINDOWS[1], 4.0
    inp = si.decode_inputs(dtype, Sq)
    cache = si.fp8_cache("decode", dtype, Sq) if fp8 else None
    q64 = (inp["q"].float() * 64.0).to(dtype)
    big = dict(inp, q=q64)
    refs = [si.reference_entry(*si.entry(big, b, cache), window, dtype, cap) for b in range(len(inp["lens"]))]
    assert max(r["lse32"][r["lse32"] != bi.NEG_INF].max().item() for r in refs if bool((r["lse32"] != bi.NEG_INF).any())) <= cap + math.log(1000) + 1e-3
    name, k, v, kw = _caches(inp, cache)[1]
    B = len(inp["lens"])
    lens_t = _lens(inp["lens"])
    o, lse = fa.forward_kvcache_softcap(q64.to(DEV), k, v, lens_t, cap, return_lse=True, **_window_kw(window), **kw)
    assert bool(torch.isfinite(o.float()).all()) and not bool(torch.isnan(lse).any())
    _check_entries("saturated decode", *_decode_entries(o, lse), refs, dtype, {})
    cu = torch.arange(0, (B + 1) * Sq, Sq, dtype=torch.int32, device=DEV)
    o, lse = fa.forward_varlen_kvcache(q64.to(DEV).reshape(B * Sq, *q64.shape[2:]), k, v, cu, Sq, lens_t, softcap=cap, **_window_kw(window), **kw)
    assert bool(torch.isfinite(o.float()).all()) and not bool(torch.isnan(lse).any())
    _check_entries("saturated prefill", *_prefill_entries(o, lse, list(range(0, (B + 1) * Sq, Sq))), refs, dtype, {})


# ---- 6: graph capture -------------------------------------------------------------------------------------------------------------

def test_a_captured_decode_step_with_the_fused_append_and_a_cap_replays_the_eager_steps_bits():
    """one graph of a decode step (append, rotate, advance_seqlens=True, capped windowed attention), replayed over three tokens:
    every replay's o and lse, the lengths and the caches are the eager steps' bits"""
    fa = _fa()
    dtype, steps, cap = torch.bfloat16, 3, 4.0
    inp = si.decode_inputs(dtype, 1)
    _, kc0, vc0, kw = _caches(inp, None)[2]   # (pages of 256)
    cos, sin = _rotary(dtype, si.DECODE_CACHE_LEN)
    feeds = [_step_feed(dtype, len(STEP_LENS), si.HEADS, 10 + i) for i in range(steps)]
    call = dict(causal=True, window_size=(100, -1), return_lse=True, rotary_cos=cos, rotary_sin=sin, advance_seqlens=True, **kw)
    kc_e, vc_e, lens_e, want = kc0.clone(), vc0.clone(), _lens(STEP_LENS), []
    for q, k, v in feeds:
        want.append(fa.forward_kvcache_softcap(q, kc_e, vc_e, lens_e, cap, k=k, v=v, **call))
    torch.cuda.synchronize()
    assert lens_e.tolist() == [n + steps for n in STEP_LENS]
    kc_g, vc_g, lens_g = kc0.clone(), vc0.clone(), _lens(STEP_LENS)
    q_s, k_s, v_s = (t.clone() for t in feeds[0])

    def step():
        return fa.forward_kvcache_softcap(q_s, kc_g, vc_g, lens_g, cap, k=k_s, v=v_s, **call)

    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        step()                                                            # warm-up outside the capture ...
    torch.cuda.current_stream().wait_stream(stream)
    kc_g.copy_(kc0), vc_g.copy_(vc0), lens_g.copy_(_lens(STEP_LENS))      # ... whose append is undone
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        o_s, lse_s = step()
    kc_g.copy_(kc0), vc_g.copy_(vc0), lens_g.copy_(_lens(STEP_LENS))
    for i, (q, k, v) in enumerate(feeds):
        q_s.copy_(q), k_s.copy_(k), v_s.copy_(v)
        graph.replay()
        torch.cuda.synchronize()
        assert _same(o_s, want[i][0]) and _same(lse_s, want[i][1]), i
        assert lens_g.tolist() == [n + i + 1 for n in STEP_LENS]
    assert _same(kc_g, kc_e) and _same(vc_g, vc_e)


# ---- 7: refusals on device tensors ------------------------------------------------------------------------------------------------

def test_refusals_on_device_tensors():
    fa = _fa()
    dtype = torch.bfloat16
    inp = si.decode_inputs(dtype, 4)
    q, k, v, lens_t = inp["q"].to(DEV), inp["k"].to(DEV), inp["v"].to(DEV), _lens(inp["lens"])
    for bad in (-1.0, float("nan"), float("inf"), True, "4", torch.tensor(4.0, device=DEV), None):
        with pytest.raises(ValueError, match="softcap"):
            fa.forward_kvcache_softcap(q, k, v, lens_t, bad)
        with pytest.raises(ValueError, match="softcap"):
            fa.forward_varlen_kvcache(q.reshape(-1, 8, 128), k, v, torch.arange(0, 32, 4, dtype=torch.int32, device=DEV), 4, lens_t, softcap=bad)
    with pytest.raises(ValueError, match="causal means right = 0"):   # a bad window first
        fa.forward_kvcache_softcap(q, k, v, lens_t, -1.0, causal=True, window_size=(5, 3))
    # what forward_kvcache refuses, the capped call refuses in its words: more than 64 packed rows, a dtype mismatch, k without v
    q17 = torch.zeros((7, 17, 8, 128), dtype=dtype, device=DEV)
    for call in (lambda **kw: fa.forward_kvcache(q17, k, v, lens_t, **kw), lambda **kw: fa.forward_kvcache_softcap(q17, k, v, lens_t, 4.0, **kw)):
        with pytest.raises(RuntimeError, match="64 packed query rows"):
            call()
    with pytest.raises(RuntimeError, match="same data type|one data type|dtype"):
        fa.forward_kvcache_softcap(q, k.to(torch.float16), v.to(torch.float16), lens_t, 4.0)
    with pytest.raises(RuntimeError, match="k and v come together"):
        fa.forward_kvcache_softcap(q, k, v, lens_t, 4.0, k=q[:, :1, :2])
    # the prefill: an fp8 cache without both descales is refused with or without a cap
    c = si.fp8_cache("decode", dtype, 4)
    with pytest.raises(RuntimeError, match="k_descale and v_descale"):
        fa.forward_varlen_kvcache(q.reshape(-1, 8, 128), c["k8"].to(DEV), c["v8"].to(DEV), torch.arange(0, 32, 4, dtype=torch.int32, device=DEV), 4,
                                  lens_t, softcap=4.0)
