"""Decode attention against an fp8 (e4m3fn) K / V cache on the MI355X: flash_attention.forward_kvcache with k_descale / v_descale
(DESIGN.md 10.7).

The oracle is always fp32 eager attention on the DEQUANTIZED cache, float(k8) * k_descale and float(v8) * v_descale, so the
quantization error never enters a bar.  The bar is tests/test_decode_gpu.py's: max|O - O32| <= max(O_TOL[dtype],
2 * max|O_eager16 - O32|), O_eager16 the same eager attention in Q's 16-bit type on the same dequantized values (it rounds
value * descale to 16 bit, which the kernel does not: the reference alone stays inside the bar); lse 1e-3 absolute, -inf exactly.
"""
import math

import pytest
import torch

from tests import beacon_inputs as bi
from tests.test_decode_gpu import DEV, DTYPES, LSE_TOL, O_TOL, _eager

pytestmark = pytest.mark.gpu

F8 = torch.float8_e4m3fn
LENGTHS = [0, 1, 2, 3, 17, 31, 32, 33, 63, 64, 65, 127, 129, 257, 1000, 4097]
NAN_CODE = 0x7F


def _fa():
    import flash_attention
    return flash_attention


@pytest.fixture(autouse=True)
def _no_tf32():
    old = torch.backends.cuda.matmul.allow_tf32
    torch.backends.cuda.matmul.allow_tf32 = False
    yield
    torch.backends.cuda.matmul.allow_tf32 = old


def _descales(gen, B, Hkv, centre):
    """Positive, different for every (batch, head), none a power of two: centre * (0.75 .. 1.25)."""
    d = (centre * (0.75 + 0.5 * torch.rand((B, Hkv), generator=gen, device=DEV))).float()
    mant, _ = torch.frexp(d)
    assert bool((mant != 0.5).all()) and d.unique().numel() == d.numel() and bool((d > 0).all())
    return d


def _inputs(dtype, lens, Sq, H, Hkv, cache_len=None, seed=0, descales=True):
    """Seeded, drawn on the device.  The cache's VALUES float(x8) * descale are about N(0, 1): x8 is N(0, 1) / descale rounded to
    e4m3fn (saturating), the descales about 1 / 100.  Without descales x8 is N(0, 1) rounded.
    -> q, k8, v8, k_descale, v_descale (or None), the dequantized fp32 k and v, the lengths on the device."""
    gen = torch.Generator(device=DEV).manual_seed(seed)
    B = len(lens)
    cache_len = cache_len or max(max(lens), 1)
    q = torch.randn((B, Sq, H, 128), generator=gen, device=DEV).to(dtype)
    kd = _descales(gen, B, Hkv, 0.011) if descales else None
    vd = _descales(gen, B, Hkv, 0.013) if descales else None
    out = [q]
    deq = []
    for d in (kd, vd):
        x = torch.randn((B, cache_len, Hkv, 128), generator=gen, device=DEV)
        x8 = (x / d[:, None, :, None] if descales else x).clamp(-448.0, 448.0).to(F8)
        assert not bool(((x8.view(torch.uint8) & 0x7F) == NAN_CODE).any())
        out.append(x8)
        deq.append(x8.float() * d[:, None, :, None] if descales else x8.float())
    return out + [kd, vd] + deq + [torch.tensor(lens, dtype=torch.int32, device=DEV)]


class _Oracle:
    """fp32 eager and 16-bit eager on the dequantized cache, computed once and shared by the launches of a case"""

    def __init__(self, q, kdq, vdq, lens, causal):
        self.dtype = q.dtype
        self.o32, self.lse32 = _eager(q, kdq, vdq, lens, causal, torch.float32)
        o16, _ = _eager(q, kdq, vdq, lens, causal, q.dtype)
        self.ref_err = (o16.float() - self.o32).abs().max().item()
        self.bound = max(O_TOL[q.dtype], 2.0 * self.ref_err)

    def check(self, tag, o, lse):
        err = (o.float() - self.o32).abs().max().item()
        print(f"{tag}: max|O - O32| = {err:.3e}  bound = {self.bound:.3e} (O_TOL {O_TOL[self.dtype]:.3e}, eager16 {self.ref_err:.3e})")
        assert torch.isfinite(o.float()).all(), tag
        assert err <= self.bound, f"{tag}: {err} > {self.bound}"
        inf = torch.isinf(self.lse32)
        assert torch.equal(torch.isinf(lse) & (lse < 0), inf), f"{tag}: -inf rows of lse differ"
        lerr = (lse[~inf] - self.lse32[~inf]).abs().max().item() if (~inf).any() else 0.0
        print(f"{tag}: max|lse - lse32| = {lerr:.3e}  bound = {LSE_TOL:.1e}")
        assert lerr <= LSE_TOL, f"{tag}: lse {lerr}"


def _same(a, b):
    return torch.equal(a.view(torch.int16 if a.element_size() == 2 else torch.int32), b.view(torch.int16 if b.element_size() == 2 else torch.int32))


# ---- 1. against fp32 eager ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("causal", [False, True], ids=["plain", "causal"])
@pytest.mark.parametrize("H,Hkv,Sq", [(8, 8, 1), (8, 2, 4), (8, 2, 8), (8, 1, 8), (8, 8, 16)])
def test_against_fp32_eager(dtype, causal, H, Hkv, Sq):
    """One batch mixing every length class (0 .. 3 against seqlen_q 4, 8, 16 under causal; both sides of the 32-key unit, the
    64-key tile and the wave's four-unit round; 4097: the loop's unroll and split boundaries), descales that differ per
    (batch, head), num_splits 0 (the rule), 1, 3, 8."""
    q, k8, v8, kd, vd, kdq, vdq, lens_t = _inputs(dtype, LENGTHS, Sq, H, Hkv, seed=Sq + H + Hkv)
    oracle = _Oracle(q, kdq, vdq, LENGTHS, causal)
    for ns in (0, 1, 3, 8):
        o, lse = _fa().forward_kvcache(q, k8, v8, lens_t, causal=causal, return_lse=True, num_splits=ns, k_descale=kd, v_descale=vd)
        oracle.check(f"fp8 eager {dtype} causal={causal} H={H} Hkv={Hkv} Sq={Sq} splits={ns}", o, lse)


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("given", ["none", "k", "v"])
def test_absent_descales_mean_one(dtype, given):
    """Both descales absent (the cache holds the values themselves), and either one alone."""
    lens = [0, 5, 64, 130, 1000, 4097]
    q, k8, v8, _, _, kdq, vdq, lens_t = _inputs(dtype, lens, 4, 8, 2, seed=11, descales=False)
    kw = {}
    if given != "none":
        d = _descales(torch.Generator(device=DEV).manual_seed(12), len(lens), 2, 0.7)
        kw[f"{given}_descale"] = d
        if given == "k":
            kdq = kdq * d[:, None, :, None]
        else:
            vdq = vdq * d[:, None, :, None]
    oracle = _Oracle(q, kdq, vdq, lens, True)
    for ns in (0, 1):
        o, lse = _fa().forward_kvcache(q, k8, v8, lens_t, causal=True, return_lse=True, num_splits=ns, **kw)
        oracle.check(f"fp8 descales given={given} {dtype} splits={ns}", o, lse)


# ---- 2. beacons --------------------------------------------------------------------------------------------------------------

BEACON_LENGTHS = [1, 2, 33, 64, 65, 130, 1000, 4097]
BEACON_CACHE_LEN = 4352   # a multiple of both page sizes, and rows behind the longest entry


def _paginate8(k8, v8, lens, page_size, poison, seed=3):
    """tests/test_decode_gpu.py's _paginate on the fp8 bytes: the contiguous caches scattered into shuffled pages.  poison: unused
    pages and rows at or beyond len hold the NaN code 0x7f, and block_table entries beyond the used pages hold out-of-range
    page numbers."""
    k, v = k8.view(torch.uint8), v8.view(torch.uint8)
    B, cache_len, Hkv, D = k.shape
    per_seq = (cache_len + page_size - 1) // page_size
    num_pages = B * per_seq + 3
    perm = torch.randperm(num_pages, generator=torch.Generator().manual_seed(seed))[:B * per_seq].view(B, per_seq)
    kp = torch.full((num_pages, page_size, Hkv, D), NAN_CODE if poison else 0, dtype=torch.uint8, device=k.device)
    vp = kp.clone()
    table = perm.to(torch.int32).clone()
    for b, n in enumerate(lens):
        used = (n + page_size - 1) // page_size
        for p in range(used):
            rows = min(page_size, n - p * page_size) if poison else min(page_size, cache_len - p * page_size)
            kp[perm[b, p], :rows] = k[b, p * page_size:p * page_size + rows]
            vp[perm[b, p], :rows] = v[b, p * page_size:p * page_size + rows]
        if poison:
            table[b, used:] = torch.tensor([-7, num_pages, 2 ** 30][b % 3], dtype=torch.int32)
    return kp.view(F8), vp.view(F8), table.to(k.device)


def _beacon_fp8_cache(first, lens, Hkv, dtype):
    """The fp8 cache of a batch of beacon entries (`first`: one build_sequence dict per entry of `lens`, keys up to the capacity)
    -> k8, v8, k_descale, v_descale and the dequantized fp32 k and v the oracle runs on.  K is stored as +- 1 with
    k_descale[b, :] = a / sqrt(128), exact and different for every batch entry; V goes through quantize_kvcache_fp8.  Shared
    with tests/test_window_beacon_gpu.py."""
    B = len(lens)
    k16, v16 = torch.stack([s["k"] for s in first]), torch.stack([s["v"] for s in first])
    k8 = torch.sign(k16.float()).to(F8)
    assert bool((k8.float().abs() == 1).all())
    kd = torch.tensor([math.sqrt(bi._beta_k(n) * math.sqrt(bi.D)) / math.sqrt(bi.D) for n in lens], device=DEV).float()[:, None].repeat(1, Hkv).contiguous()
    assert kd[:, 0].unique().numel() >= B - 1   # (lengths 1 and 2 share beta_k)
    assert bool(((k8.float() * kd[:, None, :, None]).to(dtype) == k16).all())   # the beacons' K, before its rounding to 16 bit
    _, v8, _, vd = _fa().quantize_kvcache_fp8(k16, v16)
    return k8, v8, kd, vd, k8.float() * kd[:, None, :, None], v8.float() * vd[:, None, :, None]


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("causal", [False, True], ids=["plain", "causal"])
@pytest.mark.parametrize("H,Hkv,Sq", bi.DECODE_SHAPES)
def test_decode_fp8_on_beacons(dtype, causal, H, Hkv, Sq):
    """tests/test_beacon_gpu.py's decode test with the cache in fp8.  The beacons' K is +- a / sqrt(128) with a depending on the
    entry's length: the cache stores +- 1 and k_descale[b, :] = a / sqrt(128), exact and different for every batch entry, so a
    wrong descale index, or a key lost or doubled at a seam, moves a row's target probability by a factor.  V goes through
    quantize_kvcache_fp8.  Every launch is preceded by the CPU check that every target's fp32 probability on the dequantized
    inputs lies in [P_LO, P_HI]; the paged launches (shuffled pages of 64 and 256) repeat the contiguous one's bits."""
    from flash_attention_from_scratch_amd import flash_attention_kernels as fak

    fa = _fa()
    lens, cap = BEACON_LENGTHS, BEACON_CACHE_LEN
    lens_t = torch.tensor(lens, dtype=torch.int32, device=DEV)
    first = [bi.build_sequence(Sq, n, H, Hkv, [0], dtype, causal, n_alloc=cap, seed=b, device=DEV) for b, n in enumerate(lens)]
    k8, v8, kd, vd, kdq, vdq = _beacon_fp8_cache(first, lens, Hkv, dtype)
    paged = [_paginate8(k8, v8, lens, page_size, poison=False) for page_size in (64, 256)]
    q0 = torch.stack([s["q"] for s in first])
    failures, worst_o, worst_lse, p_lo, p_hi = [], 0.0, 0.0, 1.0, 0.0
    for splits in bi.DECODE_SPLITS:
        ns = splits or fak.kvcache_num_splits(q0, k8, v8, lens_t)
        phase, n_phases = 0, 1
        while phase < n_phases:
            seqs = [bi.build_sequence(Sq, n, H, Hkv, bi.decode_positions(n, Sq, ns), dtype, causal, phase, seed=b, device=DEV,
                                      kv=(kdq[b], vdq[b])) for b, n in enumerate(lens)]
            n_phases, phase = max(s["n_phases"] for s in seqs), phase + 1
            for b, s in enumerate(seqs):   # on the CPU, before any launch: the targets carry their probability on these inputs
                c = dict(s, q=s["q"].cpu(), k=s["k"][:lens[b] + 1].cpu(), v=s["v"][:lens[b] + 1].cpu())
                p, several = bi.target_probabilities(c, bi.eager(c["q"], c["k"][:lens[b]], c["v"][:lens[b]], c["diag"], torch.float32)[1])
                if bool(several.any()):
                    p_lo, p_hi = min(p_lo, p[several].min().item()), max(p_hi, p[several].max().item())
                    assert bi.P_LO <= p[several].min().item() and p[several].max().item() <= bi.P_HI, (lens[b], ns, p[several].min(), p[several].max())
            q = torch.stack([s["q"] for s in seqs])
            o, lse = fa.forward_kvcache(q, k8, v8, lens_t, causal=causal, return_lse=True, num_splits=splits, k_descale=kd, v_descale=vd)
            for b, s in enumerate(seqs):
                res = bi.compare(o[b], lse[b], *bi.references(s), dtype)
                worst_o, worst_lse = max(worst_o, res["err"] / res["bound"]), max(worst_lse, res["lse_err"] / bi.LSE_TOL)
                if not res["ok"]:
                    print(f"FAIL len {lens[b]} splits {ns} phase {phase - 1}: {res}")
                    failures.append((lens[b], ns, phase - 1, res))
            for (kp, vp, table), page_size in zip(paged, (64, 256)):
                o_p, lse_p = fa.forward_kvcache(q, kp, vp, lens_t, block_table=table, causal=causal, return_lse=True, num_splits=splits,
                                                k_descale=kd, v_descale=vd)
                assert _same(o, o_p) and _same(lse, lse_p), (page_size, ns)
    print(f"fp8 beacons {dtype} causal={causal} H={H} Hkv={Hkv} Sq={Sq}: worst |O - O32| / bound = {worst_o:.3f}, "
          f"worst |lse - lse32| / 1e-3 = {worst_lse:.3f}, target probabilities {p_lo:.3f} .. {p_hi:.3f}")
    assert not failures, failures[:4]


# ---- 3. determinism ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("ns", [0, 5], ids=["rule", "forced5"])
def test_deterministic(dtype, ns):
    lens = [1000, 4097, 77, 0]
    q, k8, v8, kd, vd, _, _, lens_t = _inputs(dtype, lens, 4, 8, 2, seed=2)
    fa = _fa()
    o1, l1 = fa.forward_kvcache(q, k8, v8, lens_t, causal=True, return_lse=True, num_splits=ns, k_descale=kd, v_descale=vd)
    o2, l2 = fa.forward_kvcache(q, k8, v8, lens_t, causal=True, return_lse=True, num_splits=ns, k_descale=kd, v_descale=vd)
    assert _same(o1, o2) and _same(l1, l2)


# ---- 4. isolation ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("ns", [0, 3], ids=["rule", "forced3"])
def test_isolation(dtype, ns):
    """The NaN code 0x7f in every cache row at or beyond len and in every unused page, out-of-range page numbers in every unused
    block_table entry: results are finite and bitwise those of the clean run; a len = 0 entry's o is exactly 0."""
    lens = [0, 1, 63, 64, 65, 257, 1000, 1500]
    q, k8, v8, kd, vd, kdq, vdq, lens_t = _inputs(dtype, lens, 4, 8, 2, cache_len=2048, seed=5)
    fa = _fa()
    kw = dict(causal=False, return_lse=True, num_splits=ns, k_descale=kd, v_descale=vd)
    o_clean, lse_clean = fa.forward_kvcache(q, k8, v8, lens_t, **kw)
    _Oracle(q, kdq, vdq, lens, False).check(f"fp8 isolation clean {dtype} splits={ns}", o_clean, lse_clean)
    kn, vn = k8.view(torch.uint8).clone(), v8.view(torch.uint8).clone()
    for b, n in enumerate(lens):
        kn[b, n:] = NAN_CODE
        vn[b, n:] = NAN_CODE
    assert bool(torch.isnan(kn.view(F8)[0].float()).all())
    o, lse = fa.forward_kvcache(q, kn.view(F8), vn.view(F8), lens_t, **kw)
    assert torch.isfinite(o.float()).all() and not torch.isnan(lse).any()
    assert _same(o, o_clean) and _same(lse, lse_clean)
    assert (o[0] == 0).all() and torch.isinf(lse[0]).all()
    kp, vp, table = _paginate8(k8, v8, lens, 64, poison=True)
    o_p, lse_p = fa.forward_kvcache(q, kp, vp, lens_t, block_table=table, **kw)
    assert torch.isfinite(o_p.float()).all() and not torch.isnan(lse_p).any()
    assert _same(o_p, o_clean) and _same(lse_p, lse_clean)


# ---- 5. graph capture --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("paged", [False, True], ids=["contiguous", "paged"])
def test_graph_capture_replays_new_lengths_and_descales(paged):
    """One capture, replayed after cache_seqlens and both descales changed in place: the host reads none of them."""
    dtype = torch.bfloat16
    lens_a, lens_b = [100, 2048, 7, 0], [1500, 3, 640, 65]
    q, k8, v8, kd, vd, kdq, vdq, lens_t = _inputs(dtype, lens_a, 2, 8, 2, cache_len=2048, seed=8)
    fa = _fa()
    kw = dict(causal=True, return_lse=True, k_descale=kd, v_descale=vd)
    kc_, vc_ = k8, v8
    if paged:
        kc_, vc_, table = _paginate8(k8, v8, [2048] * 4, 256, poison=False)
        kw["block_table"] = table
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        fa.forward_kvcache(q, kc_, vc_, lens_t, **kw)   # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(stream)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        o, lse = fa.forward_kvcache(q, kc_, vc_, lens_t, **kw)
    graph.replay()
    torch.cuda.synchronize()
    _Oracle(q, kdq, vdq, lens_a, True).check("fp8 graph first", o.clone(), lse.clone())
    gen = torch.Generator(device=DEV).manual_seed(9)
    kd2, vd2 = _descales(gen, 4, 2, 0.017), _descales(gen, 4, 2, 0.005)
    k_values, v_values = k8.float() * kd2[:, None, :, None], v8.float() * vd2[:, None, :, None]
    lens_t.copy_(torch.tensor(lens_b, dtype=torch.int32))
    kd.copy_(kd2)
    vd.copy_(vd2)
    graph.replay()
    torch.cuda.synchronize()
    o_r, lse_r = o.clone(), lse.clone()
    _Oracle(q, k_values, v_values, lens_b, True).check("fp8 graph replay", o_r, lse_r)
    o_f, lse_f = fa.forward_kvcache(q, kc_, vc_, lens_t, **kw)   # a fresh eager call on the new lengths and descales
    assert _same(o_r, o_f) and _same(lse_r, lse_f)


# ---- 6. refusals -------------------------------------------------------------------------------------------------------------

def test_refusals_on_device():
    fa = _fa()
    q, k8, v8, kd, vd, _, _, lens_t = _inputs(torch.bfloat16, [10, 10], 1, 8, 2, cache_len=64)
    k16 = torch.zeros(k8.shape, dtype=torch.bfloat16, device=DEV)
    with pytest.raises(RuntimeError, match="one data type"):      # mixed cache dtypes
        fa.forward_kvcache(q, k8, k16, lens_t)
    with pytest.raises(RuntimeError, match="one data type"):
        fa.forward_kvcache(q, k16, v8, lens_t)
    e5m2 = k8.view(torch.uint8).view(torch.float8_e5m2)
    with pytest.raises(RuntimeError, match="float8_e4m3fn"):      # other float8 dtypes
        fa.forward_kvcache(q, e5m2, e5m2, lens_t)
    with pytest.raises(RuntimeError, match="fp8"):                # descales with a 16-bit cache
        fa.forward_kvcache(q, k16, k16, lens_t, k_descale=kd)
    with pytest.raises(RuntimeError, match="fp8"):
        fa.forward_kvcache(q, k16, k16, lens_t, v_descale=vd)
    with pytest.raises(RuntimeError, match="k_descale must be"):  # a wrong descale shape, dtype, device
        fa.forward_kvcache(q, k8, v8, lens_t, k_descale=kd[:, :1].contiguous())
    with pytest.raises(RuntimeError, match="v_descale must be"):
        fa.forward_kvcache(q, k8, v8, lens_t, v_descale=vd.t().contiguous().view(-1))
    with pytest.raises(RuntimeError, match="k_descale must be"):
        fa.forward_kvcache(q, k8, v8, lens_t, k_descale=kd.double())
    with pytest.raises(RuntimeError, match="CUDA tensor"):
        fa.forward_kvcache(q, k8, v8, lens_t, v_descale=vd.cpu())
    with pytest.raises(RuntimeError, match="Only fp16 and bf16"):  # fp8 q
        fa.forward_kvcache(k8[:, :1].contiguous(), k8, v8, lens_t)
    o = fa.forward_kvcache(q, k8, v8, lens_t, k_descale=kd, v_descale=vd)   # ... and the call these were derived from is served
    assert torch.isfinite(o.float()).all()
