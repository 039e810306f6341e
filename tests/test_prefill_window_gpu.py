"""Sliding-window attention in the packed forward and the cache prefill on the MI355X: forward_varlen(window_size=) and
forward_varlen_kvcache(window_size=).

Query row r of a sequence sits at p = r + (len_k - len_q) and sees the keys max(0, p - left) .. min(len_k - 1, p + right); causal
means right = 0.  Checked: fp32 eager per sequence with the window mask (|O - O32| <= max(O_TOL, 2 |O_eager16 - O32|), lse within
1e-3, the rows without keys exactly); every cache form against the windowed packed path, bit for bit; a window that reaches every key
against the unwindowed call, bit for bit; the fp8 cache against the 16-bit windowed call on the dequantized cache; isolation from
everything below the sequence's floor lo_b = max(0, len_k - len_q - left); forward_kvcache(window_size=) on the same cache;
position-sensitive inputs; determinism; a graph replayed over rewritten lengths, offsets and table.
The sequences are the smallest that reach every path: ragged and whole tiles, a floor inside a tile and on its boundary, one and
three Q blocks, floors several pages up, empty sides, rows dead from below."""
import functools
import math

import pytest
import torch

import beacon_inputs as bi
import flash_attention

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
DTYPES = [torch.bfloat16, torch.float16]
O_TOL = bi.O_TOL
LSE_TOL = 1e-3
NEG_INF = float("-inf")
HEADS = [(8, 2), (4, 4), (4, 1)]
PAIRS = [(165, 197), (37, 1000), (1, 777), (128, 192), (300, 100), (0, 300), (200, 0), (64, 64), (129, 65), (300, 1000)]
CAP = 1024   # rows per sequence of the caches (a multiple of both page sizes)
WINDOWS = [(0, 0), (1, 0), (31, 0), (63, 0), (64, 0), (127, 0), (128, 0), (200, 3), (-1, 5), (5, -1), (0, 64), (1000, 0)]
FORMS = ["contiguous", "page64", "page256"]
LENS_Q, LENS_K = [p[0] for p in PAIRS], [p[1] for p in PAIRS]
MQ, MK = max(LENS_Q), max(LENS_K)


def _wid(w):
    return f"w{w[0]}_{w[1]}"


def _call(w):
    """a window of the table -> (causal, window_size): causal where right = 0"""
    return w[1] == 0, w


@pytest.fixture(autouse=True)
def _no_tf32():
    old = torch.backends.cuda.matmul.allow_tf32
    torch.backends.cuda.matmul.allow_tf32 = False
    yield
    torch.backends.cuda.matmul.allow_tf32 = old


def _cu(lengths):
    cu = [0]
    for n in lengths:
        cu.append(cu[-1] + n)
    return torch.tensor(cu, dtype=torch.int32, device=DEV), cu


def _lens(lens):
    return torch.tensor(lens, dtype=torch.int32, device=DEV)


def _bits(x):
    return x.view(torch.int16) if x.dtype in (torch.bfloat16, torch.float16) else x.view(torch.int32)


def _same(a, b):
    return a.shape == b.shape and torch.equal(_bits(a.contiguous()), _bits(b.contiguous()))


def _lo_b(n_q, n_k, left):
    return bi.window_lo_min(n_k, n_q, left)


@functools.lru_cache(maxsize=None)
def _inputs(dtype, heads):
    """PAIRS as packed q, k, v: made once, shared, never written"""
    Hq, Hkv = heads
    gen = torch.Generator().manual_seed(500 + Hkv)
    q = torch.randn((sum(LENS_Q), Hq, 128), generator=gen).to(dtype).to(DEV)
    k, v = (torch.randn((sum(LENS_K), Hkv, 128), generator=gen).to(dtype).to(DEV) for _ in range(2))
    cuq_t, cuq = _cu(LENS_Q)
    cuk_t, cuk = _cu(LENS_K)
    return dict(q=q, k=k, v=v, cuq_t=cuq_t, cuq=cuq, cuk_t=cuk_t, cuk=cuk)


def _packed(c, w, k=None, v=None):
    causal, ws = _call(w)
    return flash_attention.forward_varlen(c["q"], c["k"] if k is None else k, c["v"] if v is None else v, c["cuq_t"], MQ, causal=causal,
                                          cu_seqlens_k=c["cuk_t"], max_seqlen_k=MK, window_size=ws)


@functools.lru_cache(maxsize=None)
def _packed_ref(dtype, heads, w):
    """the windowed packed call on _inputs: computed once per case, shared, never written"""
    out = _packed(_inputs(dtype, heads), w)
    torch.cuda.synchronize()
    return out


def _cache(form, k, v, cuk, left=None, poison=False, junk_first=-1, seed=3):
    """packed keys -> (k_cache, v_cache, block_table or None, lens).  poison (with the window's left): NaN in every cache row at or
    beyond len_k and below the sequence's floor lo_b, in every unused page and every page wholly below lo_b, whose table entries hold
    -1 and 2^30 in turn (starting with junk_first)."""
    B, Hkv = len(PAIRS), k.shape[1]
    if k.dtype == torch.float8_e4m3fn:   # (an fp8 cache is built as bytes: no poison asked for one here)
        assert not poison
        return tuple(t if t is None or t.dtype == torch.int32 else t.view(torch.float8_e4m3fn)
                     for t in _cache(form, k.view(torch.uint8), v.view(torch.uint8), cuk, seed=seed))
    fill = math.nan if poison else 0.0
    kc = torch.full((B, CAP, Hkv, 128), fill, dtype=k.dtype, device=DEV)
    vc = torch.full_like(kc, fill)
    floors = [(_lo_b(nq, nk, left) if poison else 0) for nq, nk in PAIRS]
    for b, (nq, nk) in enumerate(PAIRS):
        kc[b, floors[b]:nk] = k[cuk[b] + floors[b]:cuk[b + 1]]
        vc[b, floors[b]:nk] = v[cuk[b] + floors[b]:cuk[b + 1]]
    if form == "contiguous":
        return kc, vc, None
    P = int(form[4:])
    per_seq = CAP // P
    num_pages = B * per_seq + 3
    perm = torch.randperm(num_pages, generator=torch.Generator().manual_seed(seed))[:B * per_seq].view(B, per_seq)
    kp = torch.full((num_pages, P, Hkv, 128), fill, dtype=k.dtype, device=DEV)
    vp = torch.full_like(kp, fill)
    table = perm.to(torch.int32).clone()
    junk = [junk_first, 2 ** 30 if junk_first == -1 else -1]
    for b, (nq, nk) in enumerate(PAIRS):
        first, used = floors[b] // P, (nk + P - 1) // P
        for p in range(per_seq):
            if first <= p < used:
                kp[perm[b, p]] = kc[b, p * P:(p + 1) * P]
                vp[perm[b, p]] = vc[b, p * P:(p + 1) * P]
            elif poison:
                table[b, p] = junk[p % 2]
    return kp, vp, table.to(DEV)


def _prefill(c, kc, vc, table, w, **more):
    causal, ws = _call(w)
    return flash_attention.forward_varlen_kvcache(c["q"], kc, vc, c["cuq_t"], MQ, _lens(LENS_K), block_table=table, causal=causal,
                                                  window_size=ws, **more)


def _check_sequence(tag, o, lse, q, k, v, w, dtype):
    """one sequence's o (n_q, H, 128) and lse (H, n_q) against fp32 eager with the window mask; the rows without keys exactly"""
    nq, nk = q.shape[0], k.shape[0]
    if nq == 0:
        return
    if nk == 0:
        assert (o == 0).all() and (lse == NEG_INF).all(), tag
        return
    lo, hi = bi.window_bounds(nq, nk, *w)
    o32, l32 = bi.eager(q.float(), k.float(), v.float(), hi, torch.float32, lo=lo)
    o16, _ = bi.eager(q, k, v, hi, dtype, lo=lo)
    err, ref_err = (o.float() - o32).abs().max().item(), (o16.float() - o32).abs().max().item()
    bound = max(O_TOL[dtype], 2.0 * ref_err)
    print(f"{tag} ({nq}, {nk}) {w}: |O - O32| = {err:.3e} bound = {bound:.3e} (eager16 {ref_err:.3e})")
    assert torch.isfinite(o.float()).all(), tag
    assert err <= bound, (tag, err, bound)
    dead = (hi < lo).to(DEV)
    assert torch.equal(lse == NEG_INF, dead[None, :].expand_as(lse)) and not torch.isnan(lse).any(), tag
    assert (o[dead] == 0).all(), tag
    if (~dead).any():
        lerr = (lse[:, ~dead] - l32[:, ~dead]).abs().max().item()
        print(f"{tag}: |lse - lse32| = {lerr:.3e} bound = {LSE_TOL:.1e}")
        assert lerr <= LSE_TOL, (tag, lerr)


# ---- 1. fp32 eager per sequence ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("w", WINDOWS, ids=_wid)
@pytest.mark.parametrize("form", ["packed", "page64"])
def test_against_fp32_eager_per_sequence(dtype, w, form):
    heads = HEADS[0] if form == "packed" or w not in ((0, 0), (200, 3)) else HEADS[2]
    c = _inputs(dtype, heads)
    if form == "packed":
        o, lse = _packed_ref(dtype, heads, w)
    else:
        o, lse = _prefill(c, *_cache(form, c["k"], c["v"], c["cuk"]), w)
        torch.cuda.synchronize()
    cuq, cuk = c["cuq"], c["cuk"]
    for i in range(len(PAIRS)):
        sq, sk = slice(cuq[i], cuq[i + 1]), slice(cuk[i], cuk[i + 1])
        _check_sequence(f"seq {i}", o[sq], lse[:, sq], c["q"][sq], c["k"][sk], c["v"][sk], w, dtype)


# ---- 2. the packed path's bits -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("heads", HEADS)
@pytest.mark.parametrize("form", FORMS)
def test_bit_identical_to_the_windowed_packed_path(dtype, heads, form):
    c = _inputs(dtype, heads)
    kc, vc, table = _cache(form, c["k"], c["v"], c["cuk"])
    for w in WINDOWS:
        o, lse = _prefill(c, kc, vc, table, w, max_seqlen_k=None if table is None else MK)
        torch.cuda.synchronize()
        o_ref, lse_ref = _packed_ref(dtype, heads, w)
        assert o.shape == c["q"].shape and lse.shape == (heads[0], c["q"].shape[0]) and lse.dtype == torch.float32
        assert _same(o, o_ref), ("o", w)
        assert _same(lse, lse_ref), ("lse", w)


# ---- 3. the whole window -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("whole", [(True, (MK, -1)), (False, (MK, -1)), (False, (-1, MK)), (True, (MK + 7, 0))],
                         ids=["causal_left", "plain_left", "plain_right", "causal_left_right0"])
@pytest.mark.parametrize("form", ["packed"] + FORMS)
def test_the_whole_window_gives_the_unwindowed_bits(dtype, whole, form):
    """a window that reaches every key, through the windowed entry: the bits of the call without window_size"""
    causal, ws = whole
    heads = HEADS[0]
    c = _inputs(dtype, heads)
    if form == "packed":
        args = (c["q"], c["k"], c["v"], c["cuq_t"], MQ)
        kw = dict(causal=causal, cu_seqlens_k=c["cuk_t"], max_seqlen_k=MK)
        fn = flash_attention.forward_varlen
    else:
        kc, vc, table = _cache(form, c["k"], c["v"], c["cuk"])
        args = (c["q"], kc, vc, c["cuq_t"], MQ, _lens(LENS_K))
        kw = dict(block_table=table, causal=causal)
        fn = flash_attention.forward_varlen_kvcache
    o, lse = fn(*args, **kw, window_size=ws)
    o_ref, lse_ref = fn(*args, **kw)
    torch.cuda.synchronize()
    assert _same(lse, lse_ref), "lse"
    assert _same(o, o_ref), "o"


# ---- 4. fp8 --------------------------------------------------------------------------------------------------------------------

def _descales(mode, Hkv):
    B = len(PAIRS)
    if mode == "ones":
        return torch.ones((B, Hkv), device=DEV), torch.ones((B, Hkv), device=DEV)
    b, h = torch.arange(B)[:, None], torch.arange(Hkv)[None, :]
    return torch.exp2(((b + 2 * h) % 6 - 3).float()).to(DEV), torch.exp2(((2 * b + h + 1) % 6 - 3).float()).to(DEV)


def _per_row(d):
    """(n_seqs, Hkv) descales -> (total_k, Hkv, 1): each packed key row's"""
    return torch.cat([d[b].expand(n, -1) for b, n in enumerate(LENS_K)])[:, :, None]


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("mode", ["ones", "pow2"])
@pytest.mark.parametrize("form", FORMS)
def test_fp8_cache_gives_the_16_bit_windowed_bits_on_the_dequantized_cache(dtype, mode, form):
    heads = HEADS[0]
    c = _inputs(dtype, heads)
    k8, v8 = c["k"].to(torch.float8_e4m3fn), c["v"].to(torch.float8_e4m3fn)
    kd, vd = _descales(mode, heads[1])
    k16, v16 = (k8.float() * _per_row(kd)).to(dtype), (v8.float() * _per_row(vd)).to(dtype)
    assert torch.equal(k16.float(), k8.float() * _per_row(kd)) and torch.equal(v16.float(), v8.float() * _per_row(vd))   # exact
    kc, vc, table = _cache(form, k8, v8, c["cuk"])
    for w in WINDOWS:
        o, lse = _prefill(c, kc, vc, table, w, k_descale=kd, v_descale=vd)
        o_ref, lse_ref = _packed(c, w, k16, v16)
        torch.cuda.synchronize()
        assert o.dtype == dtype and _same(lse, lse_ref), ("lse", w)
        assert _same(o, o_ref), ("o", w)


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("form", ["contiguous", "page256"])
def test_fp8_quantized_cache_against_fp32_eager_per_sequence(dtype, form):
    heads = HEADS[0]
    c = _inputs(dtype, heads)
    gen = torch.Generator().manual_seed(77)
    k, v = (torch.randn((len(PAIRS), CAP, heads[1], 128), generator=gen).to(DEV) * s for s in (1.7, 0.6))
    k8, v8, kd, vd = flash_attention.quantize_kvcache_fp8(k, v)
    kdq, vdq = k8.float() * kd[:, None, :, None], v8.float() * vd[:, None, :, None]
    pk8, pv8 = (torch.cat([t[b, :n] for b, n in enumerate(LENS_K)]) for t in (k8, v8))
    kc, vc, table = _cache(form, pk8, pv8, c["cuk"])
    for w in ((0, 0), (63, 0), (200, 3), (5, -1)):
        o, lse = _prefill(c, kc, vc, table, w, k_descale=kd, v_descale=vd)
        torch.cuda.synchronize()
        for i, n in enumerate(LENS_K):
            sq = slice(c["cuq"][i], c["cuq"][i + 1])
            _check_sequence(f"seq {i}", o[sq], lse[:, sq], c["q"][sq], kdq[i, :n], vdq[i, :n], w, dtype)


# ---- 5. isolation --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("w", [(0, 0), (31, 0), (200, 3)], ids=_wid)
@pytest.mark.parametrize("form", ["packed"] + FORMS)
def test_isolation_below_the_floor(dtype, w, form):
    """NaN in everything the window does not name: cache rows below lo_b and at or beyond len_k, unused pages and pages wholly below
    lo_b with their table entries -1 and 2^30 in turn, the packed key rows below lo_b.  The bits of the clean run."""
    heads = HEADS[0]
    c = _inputs(dtype, heads)
    floors = [_lo_b(nq, nk, w[0]) for nq, nk in PAIRS]
    assert sum(f >= 64 for f in floors) >= 3, floors
    if form == "packed":
        k, v = c["k"].clone(), c["v"].clone()
        for b, f in enumerate(floors):
            k[c["cuk"][b]:c["cuk"][b] + f] = math.nan
            v[c["cuk"][b]:c["cuk"][b] + f] = math.nan
        o, lse = _packed(c, w, k, v)
        torch.cuda.synchronize()
        o_ref, lse_ref = _packed_ref(dtype, heads, w)
        assert _same(o, o_ref) and _same(lse, lse_ref)
        return
    o_ref, lse_ref = _prefill(c, *_cache(form, c["k"], c["v"], c["cuk"]), w)
    for junk_first in (-1, 2 ** 30):
        kc, vc, table = _cache(form, c["k"], c["v"], c["cuk"], left=w[0], poison=True, junk_first=junk_first)
        assert torch.isnan(kc.float()).any()
        o, lse = _prefill(c, kc, vc, table, w)
        torch.cuda.synchronize()
        assert _same(o, o_ref), junk_first
        assert _same(lse, lse_ref), junk_first


# ---- 6. the decode kernel on the same cache ------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("w", [(0, 0), (31, 0), (63, 0), (200, 3)], ids=_wid)
@pytest.mark.parametrize("shape", [(1, 4, 4), (4, 8, 2), (16, 4, 1), (3, 4, 4), (8, 8, 1)])   # (seqlen_q, Hq, Hkv): seqlen_q * G <= 64
def test_agrees_with_forward_kvcache_under_the_window(dtype, w, shape):
    Sq, Hq, Hkv = shape
    assert Sq * (Hq // Hkv) <= 64
    lens = [1, 2, 33, 64, 65, 130, 143, 1000]
    B, P = len(lens), 256
    causal, ws = _call(w)
    gen = torch.Generator().manual_seed(41)
    q = torch.randn((B, Sq, Hq, 128), generator=gen).to(dtype).to(DEV)
    kc_, vc_ = (torch.randn((B, CAP, Hkv, 128), generator=gen).to(dtype).to(DEV) for _ in range(2))
    table = torch.randperm(B * CAP // P, generator=gen).to(torch.int32).view(B, CAP // P).to(DEV)
    kp, vp = (torch.empty((B * CAP // P, P, Hkv, 128), dtype=dtype, device=DEV) for _ in range(2))
    kp[table.long().flatten()] = kc_.view(-1, P, Hkv, 128)
    vp[table.long().flatten()] = vc_.view(-1, P, Hkv, 128)
    lens_t = _lens(lens)
    o_d, lse_d = flash_attention.forward_kvcache(q, kp, vp, lens_t, block_table=table, causal=causal, return_lse=True, window_size=ws)
    cuq_t, _ = _cu([Sq] * B)
    o, lse = flash_attention.forward_varlen_kvcache(q.reshape(B * Sq, Hq, 128), kp, vp, cuq_t, Sq, lens_t, block_table=table, causal=causal,
                                                    window_size=ws)
    torch.cuda.synchronize()
    o, lse = o.view(B, Sq, Hq, 128), lse.view(Hq, B, Sq)
    lse_d = lse_d.permute(1, 0, 2)
    assert torch.equal(lse == NEG_INF, lse_d == NEG_INF)
    live = lse != NEG_INF
    assert (lse[live] - lse_d[live]).abs().max().item() <= LSE_TOL
    for b in range(B):
        qb, kb, vb = q[b], kc_[b, :lens[b]], vc_[b, :lens[b]]
        _check_sequence(f"batch {b}", o[b], lse[:, b], qb, kb, vb, w, dtype)
        lo, hi = bi.window_bounds(Sq, lens[b], *w)
        o32, _ = bi.eager(qb.float(), kb.float(), vb.float(), hi, torch.float32, lo=lo)
        tol = max(O_TOL[dtype], 2 * (bi.eager(qb, kb, vb, hi, dtype, lo=lo)[0].float() - o32).abs().max().item())
        err = (o[b].float() - o_d[b].float()).abs().max().item()
        print(f"batch {b} (len {lens[b]}): |O_prefill - O_decode| {err:.3e} tol {tol:.3e}")
        assert err <= tol, (b, lens[b], err, tol)


# ---- 7. beacons ----------------------------------------------------------------------------------------------------------------

BEACON_PAIRS = [(165, 197), (37, 1000), (300, 1000), (129, 65)]
BEACON_WINDOWS = [(0, 0), (1, 0), (63, 0), (64, 0), (127, 0), (128, 0), (200, 3)]


def beacon_positions(n_q, n_k, left, right, page_sizes=(64, 256)):
    """the positions the prefill's window moves, all inside [lo_b, n_k): each Q block's floor and ceiling and their neighbours, both
    sides of the tile boundaries in the floor tile and the next, both sides of the first page boundary above lo_b"""
    lo, hi = bi.window_bounds(n_q, n_k, left, right)
    lo_b = bi.window_lo_min(n_k, n_q, left)
    pos = [lo_b, lo_b + 1, n_k - 2, n_k - 1]
    for r0 in range(0, n_q, 128):
        r1 = min(r0 + 128, n_q) - 1
        if hi[r1] >= 0:
            pos += [int(lo[r0]) - 1, int(lo[r0]), int(lo[r0]) + 1, int(hi[r1]) - 1, int(hi[r1]), int(hi[r1]) + 1]
    tl = lo_b // 64
    pos += [p for b in (64 * tl + 64, 64 * tl + 128) for p in (b - 1, b)]
    pos += [p for P in page_sizes for p in (P * (lo_b // P + 1) - 1, P * (lo_b // P + 1))]
    seen, out = set(), []
    for p in pos:
        if lo_b <= p < n_k and p not in seen:
            seen.add(p)
            out.append(p)
    return out


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("w", BEACON_WINDOWS, ids=_wid)
def test_on_beacons(dtype, w):
    Hq, Hkv = HEADS[0]
    causal, ws = _call(w)
    seqs = []
    for i, (nq, nk) in enumerate(BEACON_PAIRS):
        listed, phase, n_phases = beacon_positions(nq, nk, *w), 0, 1
        while phase < n_phases:
            seqs.append(bi.build_window_sequence(nq, nk, Hq, Hkv, listed, dtype, w[0], w[1], phase, n_alloc=CAP, seed=10 * i + phase, device=DEV))
            n_phases, phase = seqs[-1]["n_phases"], phase + 1
    q, k, v, cuq, cuk = bi.pack(seqs)
    cuq_t = torch.tensor(cuq, dtype=torch.int32, device=DEV)
    cuk_t = torch.tensor(cuk, dtype=torch.int32, device=DEV)
    mq, mk = max(s["n_q"] for s in seqs), max(s["n_k"] for s in seqs)
    outs = {"packed": flash_attention.forward_varlen(q, k, v, cuq_t, mq, causal=causal, cu_seqlens_k=cuk_t, max_seqlen_k=mk, window_size=ws)}
    for P in (64, 256):
        B = len(seqs)
        table = torch.randperm(B * CAP // P, generator=torch.Generator().manual_seed(P)).to(torch.int32).view(B, CAP // P).to(DEV)
        kp, vp = (torch.empty((B * CAP // P, P, Hkv, 128), dtype=dtype, device=DEV) for _ in range(2))
        kp[table.long().flatten()] = torch.stack([s["k"][:CAP] for s in seqs]).view(-1, P, Hkv, 128)
        vp[table.long().flatten()] = torch.stack([s["v"][:CAP] for s in seqs]).view(-1, P, Hkv, 128)
        outs[f"page{P}"] = flash_attention.forward_varlen_kvcache(q, kp, vp, cuq_t, mq, _lens([s["n_k"] for s in seqs]), block_table=table,
                                                                  causal=causal, window_size=ws)
    torch.cuda.synchronize()
    for i, s in enumerate(seqs):
        o32, lse32, o16 = bi.references(s)
        sq = slice(cuq[i], cuq[i + 1])
        for name, (o, lse) in outs.items():
            res = bi.compare(o[sq], lse[:, sq], o32, lse32, o16, dtype)
            print(f"{name} seq {i} ({s['n_q']}, {s['n_k']}) {w}: {res}")
            assert res["ok"], (name, i, res)


# ---- 8, 9. determinism and a graph ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("form", ["packed", "page64"])
def test_deterministic(dtype, form):
    heads, w = HEADS[0], (63, 0)
    c = _inputs(dtype, heads)
    if form == "packed":
        a, b = _packed(c, w), _packed(c, w)
    else:
        kc, vc, table = _cache(form, c["k"], c["v"], c["cuk"])
        a, b = _prefill(c, kc, vc, table, w), _prefill(c, kc, vc, table, w)
    torch.cuda.synchronize()
    assert _same(a[0], b[0]) and _same(a[1], b[1])


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
def test_graph_replays_rewritten_lengths_offsets_and_table(dtype):
    """One captured graph, replayed after cache_seqlens, cu_seqlens_q and block_table are rewritten in place so that a sequence's floor
    crosses a tile boundary and a page boundary (left 31, pages of 64: floors 32 -> 69 and 100 -> 64 -> 200); each replay against an eager call."""
    Hq, Hkv, P, B, w = 8, 2, 64, 3, (31, 0)
    steps = [([20, 130, 7], [83, 261, 500]), ([57, 130, 40], [157, 225, 500]), ([100, 31, 130], [100, 262, 1000])]
    for lq, lk in steps:
        print([_lo_b(a, b, w[0]) for a, b in zip(lq, lk)])
    gen = torch.Generator().manual_seed(9)
    q = torch.randn((400, Hq, 128), generator=gen).to(dtype).to(DEV)
    kp, vp = (torch.randn((B * CAP // P + 2, P, Hkv, 128), generator=gen).to(dtype).to(DEV) for _ in range(2))
    lens_t, cuq_t = _lens(steps[0][1]), _cu(steps[0][0])[0]
    table = torch.zeros((B, CAP // P), dtype=torch.int32, device=DEV)
    tables = [torch.randperm(B * CAP // P + 2, generator=gen)[:B * CAP // P].to(torch.int32).view(B, -1).to(DEV) for _ in steps]
    table.copy_(tables[0])
    call = lambda: flash_attention.forward_varlen_kvcache(q, kp, vp, cuq_t, 130, lens_t, block_table=table, causal=True, window_size=w)   # noqa: E731
    call()
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(stream):
        call()
        with torch.cuda.graph(graph, stream=stream):
            o_g, lse_g = call()
    torch.cuda.current_stream().wait_stream(stream)
    for (lq, lk), t in zip(steps, tables):
        lens_t.copy_(_lens(lk))
        cuq_t.copy_(_cu(lq)[0])
        table.copy_(t)
        graph.replay()
        o, lse = call()
        torch.cuda.synchronize()
        n = sum(lq)
        assert _same(o_g[:n], o[:n]) and _same(lse_g[:, :n], lse[:, :n]), (lq, lk)
