"""Sliding-window (local) attention in KV-cache decode on the MI355X: flash_attention.forward_kvcache(window_size=).

The oracle is fp32 eager attention per batch entry with the window mask: query row i of an entry with n keys, at position
p = n - seqlen_q + i, sees key j iff max(0, p - left) <= j <= min(n - 1, p + right) (-1 = unbounded, causal = right 0).  The
tolerance rule is tests/test_decode_gpu.py's: max|O - O32| <= max(O_TOL[dtype], 2 * max|O_eager16 - O32|), lse 1e-3 absolute,
-inf exactly for rows that see no key.

What these inputs can see: they are N(0, 1), so every key weighs about 1 / w in a row that sees w keys, and a key lost, doubled
or leaked at an edge or a seam moves lse by ln(1 + 1 / w) and o by about |v| / w.  Against lse 1e-3 and O_TOL 2^-6 (bf16) a
single-key error shows in o up to about 100 keys and in lse up to about 1000: the small windows (left 0, 1, 31) catch a uniform
off-by-one, test_split_consistency at left 1000 sits on the bar, and (200, 3) is seen by lse alone.  What they cannot see: an
error that depends on where lo_min falls in a tile, unit, page or split, and anything at the widths models use (1024, 4096).
The poisoning tests pin what lies BELOW lo_min; the keys between lo_min and a later row's own first key, which are fetched and
must be masked, and the first key above a bounded right edge are pinned by tests/test_window_beacon_gpu.py, on inputs where
every such key carries about half of some row's probability.
"""
import math

import pytest
import torch

from tests.test_decode_gpu import DEV, DTYPES, LSE_TOL, O_TOL, _inputs, _paginate

pytestmark = pytest.mark.gpu

LENGTHS = [0, 1, 2, 3, 17, 63, 64, 65, 127, 129, 257, 1000, 4096]
LEFTS = [0, 1, 31, 32, 63, 64, 65, 200, 5000]


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
    return t.view(torch.int16 if t.element_size() == 2 else torch.int32)


def _same(a, b):
    return torch.equal(_bits(a), _bits(b))


def _bounds(window, causal):
    left, right = window
    return left, (0 if causal else right)


def _lo_min(n, Sq, left):
    return 0 if left < 0 else max(0, n - Sq - left)


def _eager(q, k, v, lens, window, causal, dtype):
    """-> (o (B, Sq, H, D) in dtype arithmetic, lse fp32 (B, H, Sq)); rows without keys: 0 and -inf.  Only the keys from the
    entry's lo_min on are touched, so a poisoned cache gives the clean result here too."""
    B, Sq, H, D = q.shape
    G = H // k.shape[2]
    left, right = _bounds(window, causal)
    o = torch.zeros((B, Sq, H, D), dtype=dtype, device=q.device)
    lse = torch.full((B, H, Sq), -math.inf, dtype=torch.float32, device=q.device)
    for b, n in enumerate(lens):
        if n == 0:
            continue
        lo = _lo_min(n, Sq, left)
        qb = q[b].to(dtype).transpose(0, 1)                                         # (H, Sq, D)
        kb = k[b, lo:n].to(dtype).repeat_interleave(G, dim=1).transpose(0, 1)        # (H, n - lo, D)
        vb = v[b, lo:n].to(dtype).repeat_interleave(G, dim=1).transpose(0, 1)
        s = (qb @ kb.transpose(1, 2)) * (1.0 / math.sqrt(D))
        p = n - Sq + torch.arange(Sq, device=q.device)[:, None]
        j = torch.arange(lo, n, device=q.device)[None, :]
        seen = torch.ones((Sq, n - lo), dtype=torch.bool, device=q.device)
        if left >= 0:
            seen &= j >= p - left
        if right >= 0:
            seen &= j <= p + right
        s = s.masked_fill(~seen, -math.inf)
        row_lse = torch.logsumexp(s.float(), dim=-1)                                 # (H, Sq)
        pr = torch.softmax(s, dim=-1)
        pr = torch.where(torch.isfinite(row_lse)[..., None], pr, torch.zeros_like(pr))
        o[b] = (pr @ vb).transpose(0, 1)
        lse[b] = row_lse
    return o, lse


class _Oracle:
    """fp32 and 16-bit eager, computed once and shared by the launches of a case (k, v: the cache's values, 16-bit or fp32)"""

    def __init__(self, q, k, v, lens, window, causal):
        self.dtype = q.dtype
        self.o32, self.lse32 = _eager(q, k, v, lens, window, causal, torch.float32)
        o16, _ = _eager(q, k, v, lens, window, causal, q.dtype)
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


# ---- 1. against fp32 eager ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("Sq", [1, 4])
@pytest.mark.parametrize("H,Hkv", [(8, 8), (8, 2), (8, 1)])
def test_against_fp32_eager(dtype, Sq, H, Hkv):
    """Every length class mixed in one batch (len < seqlen_q, windows that reach below key 0, a lo_min in a tile's second 32-key
    unit: len 129, left 31 ... among them), every left with right -1, right 0 and causal, plus (200, 3) without causal; the
    rule's split; the contiguous cache and pages of 64 and 256 keys.  One oracle per window, shared by the three caches."""
    q, k, v, lens_t = _inputs(dtype, LENGTHS, Sq, H, Hkv, seed=11 + Sq + Hkv)
    caches = [("contiguous", k, v, {})]
    for page in (64, 256):
        kp, vp, table = _paginate(k, v, LENGTHS, page, poison=False)
        caches.append((f"page{page}", kp, vp, {"block_table": table}))
    cases = [((left, right), causal) for left in LEFTS for right, causal in ((-1, False), (0, False), (-1, True))]
    cases.append(((200, 3), False))
    fa = _fa()
    for window, causal in cases:
        oracle = _Oracle(q, k, v, LENGTHS, window, causal)
        for name, kc, vc, kw in caches:
            o, lse = fa.forward_kvcache(q, kc, vc, lens_t, causal=causal, return_lse=True, window_size=window, **kw)
            oracle.check(f"window {window} causal={causal} {name} {dtype} H={H} Hkv={Hkv} Sq={Sq}", o, lse)


# ---- 2. splits -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("n,left", [(1000, 100), (20000, 1000)], ids=["len1000", "len20000"])
def test_split_consistency(dtype, n, left):
    """Forced splits 1, 3, 16 over a window of few tiles (most splits are empty) and over one that starts far from tile 0: each
    meets the tolerance rule, and lse agrees across split counts within 1e-5, |d| / max(|lse|, 1)."""
    lens = [n, n - 37, 5]
    q, k, v, lens_t = _inputs(dtype, lens, 4, 8, 2, seed=21)
    oracle = _Oracle(q, k, v, lens, (left, -1), True)
    fa = _fa()
    base = None
    for ns in (1, 3, 16):
        o, lse = fa.forward_kvcache(q, k, v, lens_t, causal=True, return_lse=True, num_splits=ns, window_size=(left, -1))
        oracle.check(f"splits={ns} len={n} left={left} {dtype}", o, lse)
        if base is None:
            base = lse
        else:
            rel = ((lse - base).abs() / base.abs().clamp_min(1.0)).max().item()
            print(f"splits={ns}: max rel |lse - lse(1 split)| = {rel:.3e}")
            assert rel <= 1e-5, (ns, rel)


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("causal", [False, True], ids=["plain", "causal"])
def test_whole_cache_window_is_the_unwindowed_call(dtype, causal):
    """left >= every length, right = -1, the same forced split: the bits of the call without window_size."""
    lens = [0, 3, 65, 1000, 4096]
    q, k, v, lens_t = _inputs(dtype, lens, 4, 8, 2, seed=22)
    fa = _fa()
    for ns in (1, 5):
        o0, l0 = fa.forward_kvcache(q, k, v, lens_t, causal=causal, return_lse=True, num_splits=ns)
        for left in (4096, 2 ** 31 - 1):
            o1, l1 = fa.forward_kvcache(q, k, v, lens_t, causal=causal, return_lse=True, num_splits=ns, window_size=(left, -1))
            assert _same(o0, o1) and _same(l0, l1), (ns, left)


# ---- 3. isolation ---------------------------------------------------------------------------------------------------------------

ISO_LENS = [0, 1, 63, 65, 257, 1000, 1500, 2048]


def _poison_below(k, v, lens, Sq, left, nan):
    kn, vn = k.clone(), v.clone()
    for b, n in enumerate(lens):
        lo = _lo_min(n, Sq, left)
        kn[b, :lo] = nan
        vn[b, :lo] = nan
    return kn, vn


def _paginate_poisoned(paginate, kn, vn, lens, Sq, left, page, nan):
    """The poisoned caches in pages; every table entry of a page wholly below lo_min points at a page of NaN."""
    kp, vp, table = paginate(kn, vn, [kn.shape[1]] * len(lens), page, poison=False)
    dead = min(set(range(kp.shape[0])) - set(table.flatten().tolist()))   # (the paginator leaves three pages unused)
    for t in (kp, vp):
        (t.view(torch.uint8) if t.element_size() == 1 else t)[dead] = nan
    for b, n in enumerate(lens):
        table[b, :_lo_min(n, Sq, left) // page] = dead
    return kp, vp, table


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("ns", [0, 3], ids=["rule", "forced3"])
@pytest.mark.parametrize("left,causal", [(0, True), (31, True), (100, False), (200, True)])
def test_isolation(dtype, ns, left, causal):
    """NaN in every K and V row below each entry's lo_min, and every table entry of a page wholly below it pointed at a page of
    NaN: o and lse are the clean run's bits."""
    Sq = 4
    q, k, v, lens_t = _inputs(dtype, ISO_LENS, Sq, 8, 2, cache_len=2048, seed=23)
    fa = _fa()
    kw = dict(causal=causal, return_lse=True, num_splits=ns, window_size=(left, -1))
    o_clean, lse_clean = fa.forward_kvcache(q, k, v, lens_t, **kw)
    _Oracle(q, k, v, ISO_LENS, (left, -1), causal).check(f"isolation clean left={left} {dtype}", o_clean, lse_clean)
    kn, vn = _poison_below(k, v, ISO_LENS, Sq, left, math.nan)
    assert bool(torch.isnan(kn[-1, 0]).all())   # (the poison is there)
    o, lse = fa.forward_kvcache(q, kn, vn, lens_t, **kw)
    assert torch.isfinite(o.float()).all()
    assert _same(o, o_clean) and _same(lse, lse_clean)
    for page in (64, 256):
        kp, vp, table = _paginate_poisoned(_paginate, kn, vn, ISO_LENS, Sq, left, page, math.nan)
        o_p, lse_p = fa.forward_kvcache(q, kp, vp, lens_t, block_table=table, **kw)
        assert torch.isfinite(o_p.float()).all()
        assert _same(o_p, o_clean) and _same(lse_p, lse_clean), page


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("ns", [0, 5], ids=["rule", "forced5"])
def test_deterministic(dtype, ns):
    lens = [1000, 4096, 77, 0]
    q, k, v, lens_t = _inputs(dtype, lens, 4, 8, 2, seed=24)
    fa = _fa()
    o1, l1 = fa.forward_kvcache(q, k, v, lens_t, causal=True, return_lse=True, num_splits=ns, window_size=(300, -1))
    o2, l2 = fa.forward_kvcache(q, k, v, lens_t, causal=True, return_lse=True, num_splits=ns, window_size=(300, -1))
    assert _same(o1, o2) and _same(l1, l2)


@pytest.mark.parametrize("paged", [False, True], ids=["contiguous", "paged"])
def test_graph_capture_replays_new_lengths(paged):
    """One capture, replayed after cache_seqlens changed in place: the window's start moves across tile and page boundaries
    (left 100: lo_min 196 -> 1396, 896 -> 26, 0 -> 536, 0 -> 0) and the host reads no length."""
    dtype = torch.bfloat16
    lens_a, lens_b = [300, 1000, 7, 0], [1500, 130, 640, 65]
    window = (100, -1)
    q, k, v, lens_t = _inputs(dtype, lens_a, 4, 8, 2, cache_len=2048, seed=25)
    fa = _fa()
    kw = dict(causal=True, return_lse=True, window_size=window)
    kc_, vc_ = k, v
    if paged:
        kc_, vc_, table = _paginate(k, v, [2048] * 4, 256, poison=False)
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
    _Oracle(q, k, v, lens_a, window, True).check("graph first", o.clone(), lse.clone())
    lens_t.copy_(torch.tensor(lens_b, dtype=torch.int32))
    graph.replay()
    torch.cuda.synchronize()
    o_g, lse_g = o.clone(), lse.clone()
    _Oracle(q, k, v, lens_b, window, True).check("graph replay", o_g, lse_g)
    o_e, lse_e = fa.forward_kvcache(q, kc_, vc_, lens_t, **kw)   # the eager launch with the same lengths: the same bits
    assert _same(o_g, o_e) and _same(lse_g, lse_e)


# ---- 4. the fp8 cache -------------------------------------------------------------------------------------------------------------

def _fp8():
    import tests.test_decode_fp8_gpu as t8
    return t8


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("Sq", [1, 4])
def test_fp8_against_fp32_eager(dtype, Sq):
    """The eager-parity case at one GQA shape, against the dequantized cache, descales that differ per (batch, head)."""
    q, k8, v8, kd, vd, kdq, vdq, lens_t = _fp8()._inputs(dtype, LENGTHS, Sq, 8, 2, seed=31 + Sq)
    cases = [((left, right), causal) for left in LEFTS for right, causal in ((-1, False), (0, False), (-1, True))]
    cases.append(((200, 3), False))
    fa = _fa()
    for window, causal in cases:
        o, lse = fa.forward_kvcache(q, k8, v8, lens_t, causal=causal, return_lse=True, k_descale=kd, v_descale=vd, window_size=window)
        _Oracle(q, kdq, vdq, LENGTHS, window, causal).check(f"fp8 window {window} causal={causal} {dtype} Sq={Sq}", o, lse)


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("ns", [0, 3], ids=["rule", "forced3"])
def test_fp8_isolation(dtype, ns):
    """e4m3 NaN (0x7f) in every byte below lo_min, dead pages below it: the clean run's bits."""
    t8 = _fp8()
    Sq, left = 4, 100
    q, k8, v8, kd, vd, kdq, vdq, lens_t = t8._inputs(dtype, ISO_LENS, Sq, 8, 2, cache_len=2048, seed=32)
    fa = _fa()
    kw = dict(causal=True, return_lse=True, num_splits=ns, k_descale=kd, v_descale=vd, window_size=(left, -1))
    o_clean, lse_clean = fa.forward_kvcache(q, k8, v8, lens_t, **kw)
    _Oracle(q, kdq, vdq, ISO_LENS, (left, -1), True).check(f"fp8 isolation clean {dtype}", o_clean, lse_clean)
    kn, vn = _poison_below(k8.view(torch.uint8), v8.view(torch.uint8), ISO_LENS, Sq, left, t8.NAN_CODE)
    o, lse = fa.forward_kvcache(q, kn.view(t8.F8), vn.view(t8.F8), lens_t, **kw)
    assert torch.isfinite(o.float()).all()
    assert _same(o, o_clean) and _same(lse, lse_clean)
    kp, vp, table = _paginate_poisoned(t8._paginate8, kn, vn, ISO_LENS, Sq, left, 64, t8.NAN_CODE)
    o_p, lse_p = fa.forward_kvcache(q, kp, vp, lens_t, block_table=table, **kw)
    assert torch.isfinite(o_p.float()).all()
    assert _same(o_p, o_clean) and _same(lse_p, lse_clean)


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
def test_fp8_whole_cache_window_is_the_unwindowed_call(dtype):
    lens = [0, 3, 65, 1000, 4096]
    q, k8, v8, kd, vd, _, _, lens_t = _fp8()._inputs(dtype, lens, 4, 8, 2, seed=33)
    fa = _fa()
    for ns in (1, 5):
        kw = dict(causal=True, return_lse=True, num_splits=ns, k_descale=kd, v_descale=vd)
        o0, l0 = fa.forward_kvcache(q, k8, v8, lens_t, **kw)
        o1, l1 = fa.forward_kvcache(q, k8, v8, lens_t, window_size=(4096, -1), **kw)
        assert _same(o0, o1) and _same(l0, l1), ns


# ---- 4b. 64 packed rows: the four-row-tile forms (their own kernels, at the register file's end) ---------------------------------

@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("fp8", [False, True], ids=["16bit", "fp8"])
def test_64_packed_rows(dtype, fp8):
    """seqlen_q 8 x group 8: parity, and the isolation case's bits, contiguous and paged, the rule's split and a forced odd one."""
    Sq, lens = 8, [0, 5, 65, 129, 1000, 2048]
    if fp8:
        t8 = _fp8()
        q, k, v, kd, vd, kdq, vdq, lens_t = t8._inputs(dtype, lens, Sq, 8, 1, cache_len=2048, seed=35)
        extra, nan, paginate = dict(k_descale=kd, v_descale=vd), t8.NAN_CODE, t8._paginate8
        raw = lambda t: t.view(torch.uint8)      # noqa: E731
        back = lambda t: t.view(t8.F8)           # noqa: E731
    else:
        q, k, v, lens_t = _inputs(dtype, lens, Sq, 8, 1, cache_len=2048, seed=35)
        kdq, vdq, extra, nan, paginate = k, v, {}, math.nan, _paginate
        raw = back = lambda t: t                 # noqa: E731
    fa = _fa()
    for window, causal in (((0, -1), True), ((31, -1), True), ((100, 0), False), ((200, 3), False), ((5000, -1), True)):
        oracle = _Oracle(q, kdq, vdq, lens, window, causal)
        kn, vn = _poison_below(raw(k), raw(v), lens, Sq, window[0], nan)
        kp, vp, table = _paginate_poisoned(paginate, kn, vn, lens, Sq, window[0], 64, nan)
        for ns in (0, 3):
            kw = dict(causal=causal, return_lse=True, num_splits=ns, window_size=window, **extra)
            o, lse = fa.forward_kvcache(q, k, v, lens_t, **kw)
            oracle.check(f"64 rows window {window} causal={causal} splits={ns} fp8={fp8} {dtype}", o, lse)
            o_n, lse_n = fa.forward_kvcache(q, back(kn), back(vn), lens_t, **kw)
            assert _same(o_n, o) and _same(lse_n, lse), (window, ns)
            o_p, lse_p = fa.forward_kvcache(q, back(kp), back(vp), lens_t, block_table=table, **kw)
            assert _same(o_p, o) and _same(lse_p, lse), (window, ns)


# ---- 5. with the append ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
def test_append_then_window(dtype):
    """k= / v= with advance_seqlens and a window: append_kvcache followed by the windowed decode, bit for bit; the window
    applies to the advanced lengths."""
    lens = [0, 60, 129, 1000]
    Sq, window = 4, (64, -1)
    q, k, v, lens_t = _inputs(dtype, lens, Sq, 8, 2, cache_len=1100, seed=41)
    gen = torch.Generator(device=DEV).manual_seed(42)
    k_new = torch.randn((len(lens), Sq, 2, 128), generator=gen, device=DEV).to(dtype)
    v_new = torch.randn((len(lens), Sq, 2, 128), generator=gen, device=DEV).to(dtype)
    fa = _fa()
    k1, v1, lens1 = k.clone(), v.clone(), lens_t.clone()
    o1, l1 = fa.forward_kvcache(q, k1, v1, lens1, causal=True, return_lse=True, k=k_new, v=v_new, advance_seqlens=True,
                                window_size=window)
    k2, v2, lens2 = k.clone(), v.clone(), lens_t.clone()
    fa.append_kvcache(k2, v2, k_new, v_new, lens2, seqlens_out=lens2)
    o2, l2 = fa.forward_kvcache(q, k2, v2, lens2, causal=True, return_lse=True, window_size=window)
    after = [n + Sq for n in lens]
    assert lens1.tolist() == after and lens2.tolist() == after
    assert _same(k1, k2) and _same(v1, v2)
    assert _same(o1, o2) and _same(l1, l2)
    _Oracle(q, k2, v2, after, window, True).check(f"append {dtype}", o1, l1)
