"""Prefill against an fp8 (e4m3fn) KV cache on the MI355X: flash_attention.forward_varlen_kvcache(k_descale=, v_descale=)
(DESIGN.md 10.10).

The anchor is the 16-bit call: every e4m3 value is exact in bf16 and in fp16, and a power-of-two descale commutes with every
rounding on the path, so with unit or power-of-two descales o and lse must have the BITS of forward_varlen_kvcache on the
dequantized cache -- the transport, the cache walk, the conversion and the descales' indices are then exact, whatever the
tolerance.  Beside it: general descales against fp32 eager attention per sequence on the dequantized cache with the project's rule,
|O - O32| <= max(O_TOL, 2 |O_eager16 - O32|) (O_TOL 2^-6 bf16 / 2^-9 fp16), lse within 1e-3, rows without keys exactly 0 / -inf;
beacon inputs; isolation; garbage in the device arrays; forward_kvcache on the same fp8 cache; a chunked prefill through
append_kvcache; determinism; a graph whose lengths, offsets, table and descales are rewritten between replays.
The shapes are the sibling file's (tests/test_prefill_kvcache_gpu.py), declared again here: ragged and whole tiles, one and several Q
blocks, one and several pages, a page of one tile and of four, empty sides, more queries than keys."""
import ctypes
import functools
import math

import pytest
import torch

import flash_attention
from flash_attention_from_scratch_amd import _capi
from flash_attention_from_scratch_amd import flash_attention_kernels as fak
from tests import beacon_inputs as bi

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
F8 = torch.float8_e4m3fn
U8 = torch.uint8
NAN8 = 0x7f   # e4m3fn's NaN code
DTYPES = [torch.bfloat16, torch.float16]
O_TOL = {torch.bfloat16: 2.0 ** -6, torch.float16: 2.0 ** -9}
LSE_TOL = 1e-3
HEADS = [(4, 4), (8, 2), (4, 1)]
NEG_INF = float("-inf")
# (len_q, len_k) per sequence
PAIRS = [(165, 197), (37, 1000), (1, 777), (128, 192), (300, 100), (0, 300), (200, 0), (64, 64), (129, 65)]
CAP = 1024   # rows per sequence of the caches built from PAIRS (a multiple of both page sizes)
FORMS = ["contiguous", "page64", "page256"]
B = len(PAIRS)
LENS_Q, LENS_K = [p[0] for p in PAIRS], [p[1] for p in PAIRS]


@pytest.fixture(autouse=True)
def _no_tf32():
    old = torch.backends.cuda.matmul.allow_tf32
    torch.backends.cuda.matmul.allow_tf32 = False
    yield
    torch.backends.cuda.matmul.allow_tf32 = old


def _cu(lengths, first=0):
    cu = [first]
    for n in lengths:
        cu.append(cu[-1] + n)
    return torch.tensor(cu, dtype=torch.int32, device=DEV), cu


def _lens(lens):
    return torch.tensor(lens, dtype=torch.int64).to(torch.int32).to(DEV)


def _bits(x):
    return x.view(torch.int16) if x.dtype in (torch.bfloat16, torch.float16) else x.view(torch.int32)


def _same(a, b):
    return a.shape == b.shape and torch.equal(_bits(a.contiguous()), _bits(b.contiguous()))


def _paginate(kc, vc, lens, page_size, poison, seed=3, spare=3, junk=(-1, 2 ** 30)):
    """Contiguous caches (16-bit, or fp8 as bytes) scattered into shuffled pages -> (k pages, v pages, block_table).  poison:
    unused pages and rows at or beyond len hold NaN (bytes: the code 0x7f), and the block_table entries beyond the used pages
    hold `junk` in turn."""
    n_seqs, cap, Hkv, D = kc.shape
    per_seq = (cap + page_size - 1) // page_size
    num_pages = n_seqs * per_seq + spare
    perm = torch.randperm(num_pages, generator=torch.Generator().manual_seed(seed))[:n_seqs * per_seq].view(n_seqs, per_seq)
    fill = (NAN8 if kc.dtype == U8 else math.nan) if poison else 0
    kp = torch.full((num_pages, page_size, Hkv, D), fill, dtype=kc.dtype, device=kc.device)
    vp = torch.full_like(kp, fill)
    table = perm.to(torch.int32).clone()
    for b, n in enumerate(lens):
        used = (n + page_size - 1) // page_size
        for p in range(used):
            rows = min(page_size, n - p * page_size)
            kp[perm[b, p], :rows] = kc[b, p * page_size:p * page_size + rows]
            vp[perm[b, p], :rows] = vc[b, p * page_size:p * page_size + rows]
        if poison:
            table[b, used:] = torch.tensor([j if j is not None else num_pages for j in junk] * per_seq, dtype=torch.int64)[:per_seq - used].to(torch.int32)
    return kp, vp, table.to(kc.device)


def _form(form, kc, vc, lens, poison=False, seed=3, junk=(-1, 2 ** 30)):
    """contiguous caches (n_seqs, cap, Hkv, 128), 16-bit or fp8, in the named form -> (k_cache, v_cache, block_table or None); poison:
    the rows at or beyond len hold NaN"""
    fp8 = kc.dtype == F8
    if fp8:
        kc, vc = kc.view(U8), vc.view(U8)
    if poison:
        kc, vc = kc.clone(), vc.clone()
        for b, n in enumerate(lens):
            kc[b, n:] = NAN8 if fp8 else math.nan
            vc[b, n:] = NAN8 if fp8 else math.nan
    table = None
    if form != "contiguous":
        kc, vc, table = _paginate(kc, vc, lens, int(form[4:]), poison, seed=seed, junk=junk)
    return (kc.view(F8), vc.view(F8), table) if fp8 else (kc, vc, table)


@functools.lru_cache(maxsize=None)
def _case8(heads):
    """PAIRS as fp32 q and contiguous e4m3fn caches (every row random, also beyond len_k): computed once, shared, never written."""
    Hq, Hkv = heads
    gen = torch.Generator().manual_seed(200 + Hkv)
    q = torch.randn((sum(LENS_Q), Hq, 128), generator=gen)
    k8, v8 = (torch.randn((B, CAP, Hkv, 128), generator=gen).to(DEV).to(F8) for _ in range(2))
    cuq_t, cuq = _cu(LENS_Q)
    return dict(q=q.to(DEV), k8=k8, v8=v8, cuq_t=cuq_t, cuq=cuq, mq=max(LENS_Q), mk=max(LENS_K))


def _descales(mode, Hkv, n_seqs=B):
    """-> (k_descale, v_descale) fp32 (n_seqs, Hkv): ones, or powers of two 2^a, a in [-3, 2], different per (sequence, head) and
    between K and V"""
    if mode == "ones":
        return torch.ones((n_seqs, Hkv), device=DEV), torch.ones((n_seqs, Hkv), device=DEV)
    b, h = torch.arange(n_seqs)[:, None], torch.arange(Hkv)[None, :]
    ak, av = (b + 2 * h) % 6 - 3, (2 * b + h + 1) % 6 - 3
    assert ak.min() == -3 and ak.max() == 2 and av.min() >= -3 and av.max() <= 2 and (ak != av).any()
    return torch.exp2(ak.float()).to(DEV), torch.exp2(av.float()).to(DEV)


def _dequant(x8, d):
    return x8.float() * d[:, None, :, None]


@functools.lru_cache(maxsize=None)
def _ref16(dtype, causal, heads, mode):
    """The 16-bit call on the dequantized cache (exact in dtype for these descales), contiguous: the bits every fp8 launch on _case8
    must repeat.  Computed once per case."""
    c = _case8(heads)
    kd, vd = _descales(mode, heads[1])
    k16, v16 = _dequant(c["k8"], kd).to(dtype), _dequant(c["v8"], vd).to(dtype)
    assert torch.equal(k16.float(), _dequant(c["k8"], kd)) and torch.equal(v16.float(), _dequant(c["v8"], vd))   # exact
    o, lse = flash_attention.forward_varlen_kvcache(c["q"].to(dtype), k16, v16, c["cuq_t"], c["mq"], _lens(LENS_K), causal=causal)
    torch.cuda.synchronize()
    return o, lse


def _mask(n_q, n_k):
    """True where query r must NOT see key j: j > r + (n_k - n_q)"""
    return ~torch.ones((n_q, n_k), dtype=torch.bool, device=DEV).tril(diagonal=n_k - n_q)


def _eager(q, k, v, causal, dtype):
    """one sequence: q (n_q, H, D), k / v (n_k, Hkv, D), n_q, n_k >= 1 -> o (n_q, H, D) in `dtype`; a row without keys gives 0"""
    G = q.shape[1] // k.shape[1]
    k, v = k.repeat_interleave(G, dim=1), v.repeat_interleave(G, dim=1)
    s = torch.einsum("qhd,khd->hqk", q.to(dtype), k.to(dtype)) / 128 ** 0.5
    if causal:
        m = _mask(q.shape[0], k.shape[0])
        s = s.masked_fill(m, NEG_INF)
        dead = m.all(dim=1)
        p = torch.softmax(s.masked_fill(dead[None, :, None], 0.0), dim=-1).masked_fill(dead[None, :, None], 0.0)
    else:
        p = torch.softmax(s, dim=-1)
    return torch.einsum("hqk,khd->qhd", p, v.to(dtype))


def _lse32(q, k, causal):
    G = q.shape[1] // k.shape[1]
    s = torch.einsum("qhd,khd->hqk", q.float(), k.repeat_interleave(G, dim=1).float()) / 128 ** 0.5
    if causal:
        s = s.masked_fill(_mask(q.shape[0], k.shape[0]), NEG_INF)
    return torch.logsumexp(s, dim=-1)   # (-inf for a row without keys)


def _check_sequence(tag, o, lse, q, k, v, causal, dtype):
    """one sequence's o (n_q, H, D) and lse (H, n_q) against the fp32 rule on k, v (the DEQUANTIZED keys, fp32: quantization error
    enters no bar); the rows without keys exactly"""
    nq, nk = q.shape[0], k.shape[0]
    if nq == 0:
        return
    if nk == 0:
        assert (o == 0).all() and (lse == NEG_INF).all(), tag
        return
    o32 = _eager(q.float(), k.float(), v.float(), causal, torch.float32)
    o16 = _eager(q, k, v, causal, dtype).float()
    err = (o.float() - o32).abs().max().item()
    ref_err = (o16 - o32).abs().max().item()
    bound = max(O_TOL[dtype], 2.0 * ref_err)
    print(f"{tag} ({nq}, {nk}): |O - O32| = {err:.3e} bound = {bound:.3e} (eager16 {ref_err:.3e})")
    assert torch.isfinite(o.float()).all(), tag
    assert err <= bound, (tag, err, bound)
    l32 = _lse32(q, k, causal)
    live = torch.isfinite(l32)
    assert torch.equal(lse == NEG_INF, ~live) and not torch.isnan(lse).any(), tag
    dead = max(nq - nk, 0) if causal else 0   # the first `dead` rows see no key
    assert int((~live[0]).sum()) == dead and (o[:dead] == 0).all(), tag
    if live.any():
        lerr = (lse[live] - l32[live]).abs().max().item()
        print(f"{tag}: |lse - lse32| = {lerr:.3e} bound = {LSE_TOL:.1e}")
        assert lerr <= LSE_TOL, (tag, lerr)


def _launch_c(q, kc, vc, o, lse, cuq_t, n_seqs, mq, lens_t, table, causal, kd, vd, max_seqlen_k=0):
    """the launch through the C ABI on the caller's o and lse (q, o contiguous (T, H, 128); lse (H, T)); kd, vd: rows of one stride"""
    lib = _capi.load()
    Tq, Hq = q.shape[0], q.shape[1]
    args = _capi.FaFwdArgs(q=q.data_ptr(), k=kc.data_ptr(), v=vc.data_ptr(), o=o.data_ptr(), batch=1, seq_len=Tq, n_heads=Hq, d_head=128,
                           batch_stride=0, seq_stride=q.stride(0), head_stride=q.stride(1), cfg=_capi.make_config(fak.varlen_config(q.dtype)))
    kv = _capi.make_kv_layout(kc.shape[2], kc.stride(0), kc.stride(1), kc.stride(2))
    vq = _capi.make_varlen_layout(cuq_t.data_ptr(), n_seqs, Tq, mq)
    paged = table is not None
    layout = _capi.make_kvcache_layout(
        cache_seqlens=lens_t.data_ptr(), block_table=table.data_ptr() if paged else None, seqlen_cache=0 if paged else kc.shape[1],
        batch=0 if paged else kc.shape[0], num_pages=kc.shape[0] if paged else 0, page_size=kc.shape[1] if paged else 0,
        max_pages_per_seq=table.shape[1] if paged else 0, block_table_stride=table.stride(0) if paged else 0, max_seqlen_k=max_seqlen_k)
    assert kd.stride(0) == vd.stride(0) and kd.stride(1) == vd.stride(1) == 1
    sc = _capi.make_kvcache_fp8_scales(k_descale=kd.data_ptr(), v_descale=vd.data_ptr(), descale_batch_stride=kd.stride(0))
    opts = _capi.make_opts(causal=causal)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    _capi.check(lib.fa_fwd_launch_varlen_kvcache_fp8(ctypes.byref(args), ctypes.byref(kv), ctypes.byref(vq), ctypes.byref(layout),
                                                     ctypes.byref(sc), ctypes.byref(opts), ctypes.c_void_p(lse.data_ptr()), stream))


# ---- 1, 2. the 16-bit call's bits at unit and at power-of-two descales -------------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("causal", [False, True], ids=["plain", "causal"])
@pytest.mark.parametrize("heads", HEADS)
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("mode", ["ones", "pow2"])
def test_bit_identical_to_the_16_bit_call_on_the_dequantized_cache(dtype, causal, heads, form, mode):
    c = _case8(heads)
    kd, vd = _descales(mode, heads[1])
    kc, vc, table = _form(form, c["k8"], c["v8"], LENS_K)
    o, lse = flash_attention.forward_varlen_kvcache(c["q"].to(dtype), kc, vc, c["cuq_t"], c["mq"], _lens(LENS_K), block_table=table, causal=causal,
                                                    max_seqlen_k=None if table is None else c["mk"], k_descale=kd, v_descale=vd)
    torch.cuda.synchronize()
    o_ref, lse_ref = _ref16(dtype, causal, heads, mode)
    assert o.shape == o_ref.shape and o.dtype == dtype and lse.shape == (heads[0], sum(LENS_Q)) and lse.dtype == torch.float32
    assert _same(lse, lse_ref), "lse"
    assert _same(o, o_ref), "o"


# ---- 3. general descales against fp32 eager per sequence ---------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _quantized_case(heads):
    Hq, Hkv = heads
    gen = torch.Generator().manual_seed(300 + Hkv)
    q = torch.randn((sum(LENS_Q), Hq, 128), generator=gen).to(DEV)
    k, v = (torch.randn((B, CAP, Hkv, 128), generator=gen).to(DEV) * s for s in (1.7, 0.6))
    k8, v8, kd, vd = flash_attention.quantize_kvcache_fp8(k, v)
    assert kd.shape == (B, Hkv) and kd.unique().numel() == B * Hkv
    return dict(q=q, k8=k8, v8=v8, kd=kd, vd=vd, kdq=_dequant(k8, kd), vdq=_dequant(v8, vd))


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("causal", [False, True], ids=["plain", "causal"])
@pytest.mark.parametrize("heads", HEADS)
@pytest.mark.parametrize("form", FORMS)
def test_general_descales_against_fp32_eager_per_sequence(dtype, causal, heads, form):
    c = _quantized_case(heads)
    q = c["q"].to(dtype)
    kc, vc, table = _form(form, c["k8"], c["v8"], LENS_K, poison=True)
    cuq_t, cuq = _cu(LENS_Q)
    o, lse = flash_attention.forward_varlen_kvcache(q, kc, vc, cuq_t, max(LENS_Q), _lens(LENS_K), block_table=table, causal=causal,
                                                    k_descale=c["kd"], v_descale=c["vd"])
    torch.cuda.synchronize()
    for i, n in enumerate(LENS_K):
        sq = slice(cuq[i], cuq[i + 1])
        _check_sequence(f"seq {i}", o[sq], lse[:, sq], q[sq], c["kdq"][i, :n], c["vdq"][i, :n], causal, dtype)


# ---- 4. beacons ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("causal", [False, True], ids=["plain", "causal"])
@pytest.mark.parametrize("heads", HEADS)
def test_on_beacons(dtype, causal, heads):
    """tests/beacon_inputs.py on PAIRS with the cache in fp8.  The beacons' K is +- a / sqrt(128) with a depending on the sequence's
    length: the cache stores +- 1 and k_descale[b, :] = a / sqrt(128), so a wrong descale index, or a key lost or doubled at a tile,
    page or ragged seam, moves a row's target probability by a factor.  V goes through quantize_kvcache_fp8.  Every launch is preceded by
    the CPU check that every target's fp32 probability on the dequantized inputs lies in [P_LO, P_HI]; the paged launches repeat the
    contiguous one's bits."""
    Hq, Hkv = heads
    first = [bi.build_sequence(nq, nk, Hq, Hkv, [0], dtype, causal, n_alloc=CAP, seed=b, device=DEV) for b, (nq, nk) in enumerate(PAIRS)]
    assert all(s["k"].shape[0] == CAP for s in first)
    k16, v16 = torch.stack([s["k"] for s in first]), torch.stack([s["v"] for s in first])
    k8 = torch.sign(k16.float()).to(F8)
    assert bool((k8.float().abs() == 1).all())
    kd = torch.tensor([math.sqrt(bi._beta_k(n) * math.sqrt(bi.D)) / math.sqrt(bi.D) for n in LENS_K], device=DEV).float()[:, None].repeat(1, Hkv).contiguous()
    assert kd[:, 0].unique().numel() >= B - 2
    assert bool((_dequant(k8, kd).to(dtype) == k16).all())   # the beacons' K, before its rounding to 16 bit
    _, v8, _, vd = flash_attention.quantize_kvcache_fp8(k16, v16)
    kdq, vdq = _dequant(k8, kd), _dequant(v8, vd)
    caches = [_form(form, k8, v8, LENS_K) for form in FORMS]
    cuq_t, cuq = _cu(LENS_Q)
    lens_t = _lens(LENS_K)
    failures, worst_o, worst_lse, p_lo, p_hi = [], 0.0, 0.0, 1.0, 0.0
    phase, n_phases = 0, 1
    while phase < n_phases:
        seqs = [bi.build_sequence(nq, nk, Hq, Hkv, bi.varlen_positions(nq, nk), dtype, causal, phase, seed=b, device=DEV, kv=(kdq[b], vdq[b]))
                for b, (nq, nk) in enumerate(PAIRS)]
        n_phases, phase = max(s["n_phases"] for s in seqs), phase + 1
        for s in seqs:   # on the CPU, before any launch: the targets carry their probability on these inputs
            if s["n_q"] == 0 or s["n_k"] == 0:
                continue
            c = dict(s, q=s["q"].cpu(), k=s["k"][:s["n_k"] + 1].cpu(), v=s["v"][:s["n_k"] + 1].cpu())
            p, several = bi.target_probabilities(c, bi.eager(c["q"], c["k"][:s["n_k"]], c["v"][:s["n_k"]], c["diag"], torch.float32)[1])
            if bool(several.any()):
                p_lo, p_hi = min(p_lo, p[several].min().item()), max(p_hi, p[several].max().item())
                assert bi.P_LO <= p[several].min().item() and p[several].max().item() <= bi.P_HI, (s["n_q"], s["n_k"], p[several].min(), p[several].max())
        q = torch.cat([s["q"] for s in seqs])
        got = [flash_attention.forward_varlen_kvcache(q, kc, vc, cuq_t, max(LENS_Q), lens_t, block_table=table, causal=causal, k_descale=kd, v_descale=vd)
               for kc, vc, table in caches]
        torch.cuda.synchronize()
        o, lse = got[0]
        for b, s in enumerate(seqs):
            sq = slice(cuq[b], cuq[b + 1])
            res = bi.compare(o[sq], lse[:, sq], *bi.references(s), dtype)
            worst_o, worst_lse = max(worst_o, res["err"] / res["bound"]), max(worst_lse, res["lse_err"] / bi.LSE_TOL)
            if not res["ok"]:
                print(f"FAIL pair {PAIRS[b]} phase {phase - 1}: {res}")
                failures.append((PAIRS[b], phase - 1, res))
        for form, (o_p, lse_p) in zip(FORMS[1:], got[1:]):
            assert _same(o, o_p) and _same(lse, lse_p), (form, phase - 1)
    print(f"fp8 prefill beacons {dtype} causal={causal} heads={heads}: worst |O - O32| / bound = {worst_o:.3f}, "
          f"worst |lse - lse32| / 1e-3 = {worst_lse:.3f}, target probabilities {p_lo:.3f} .. {p_hi:.3f}, {n_phases} phases")
    assert not failures, failures[:4]


# ---- 5. isolation ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("causal", [False, True], ids=["plain", "causal"])
@pytest.mark.parametrize("heads", HEADS)
@pytest.mark.parametrize("form", FORMS)
def test_isolation(dtype, causal, heads, form):
    """The NaN code 0x7f in every unused page and every cache row at or beyond len_k, NaN in the q rows outside the sequences'
    ranges and in the descale rows of no sequence, -7, num_pages and 2^30 in the unused block_table entries: the rows of the
    ranges are bit-identical to the clean run (and to the 16-bit call), and the rows of o and lse outside every range keep
    their sentinel."""
    c = _case8(heads)
    Hq, Hkv = heads
    M, SENT = 37, 777.0
    Tq = sum(LENS_Q)
    cuq_t, _ = _cu(LENS_Q, first=M)
    lens_t = _lens(LENS_K)
    kd, vd = _descales("pow2", Hkv)
    got = []
    for poison in (False, True):
        kc, vc, table = _form(form, c["k8"], c["v8"], LENS_K, poison=poison, junk=(-7, None, 2 ** 30))
        assert bool((kc.view(U8) == NAN8).any()) == poison   # (randn never rounds to the NaN code)
        q = torch.full((Tq + 2 * M, Hq, 128), math.nan if poison else 0.0, dtype=dtype, device=DEV)
        q[M:M + Tq] = c["q"].to(dtype)
        scales = torch.full((2, B + 2, Hkv), math.nan if poison else 1.0, device=DEV)
        scales[0, 1:B + 1], scales[1, 1:B + 1] = kd, vd
        o = torch.full_like(q, math.nan if poison else SENT)
        o[:M] = SENT
        o[M + Tq:] = SENT
        lse = torch.full((Hq, Tq + 2 * M), SENT, dtype=torch.float32, device=DEV)
        _launch_c(q, kc, vc, o, lse, cuq_t, B, max(LENS_Q), lens_t, table, causal, scales[0, 1:B + 1], scales[1, 1:B + 1])
        torch.cuda.synchronize()
        assert (o[:M] == SENT).all() and (o[M + Tq:] == SENT).all(), poison
        assert (lse[:, :M] == SENT).all() and (lse[:, M + Tq:] == SENT).all(), poison
        got.append((o[M:M + Tq], lse[:, M:M + Tq]))
    (o_clean, lse_clean), (o_p, lse_p) = got
    assert torch.isfinite(o_p.float()).all() and not torch.isnan(lse_p).any()
    assert _same(o_p, o_clean) and _same(lse_p, lse_clean)
    o_ref, lse_ref = _ref16(dtype, causal, heads, "pow2")
    assert _same(o_clean, o_ref) and _same(lse_clean, lse_ref)   # (the range's offset in q moves no bit either)


# ---- 6. garbage stays inside -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("causal", [False, True], ids=["plain", "causal"])
@pytest.mark.parametrize("form", FORMS)
def test_garbage_in_the_device_arrays_stays_inside_the_tensors(dtype, causal, form):
    """cache_seqlens of -5 and 2^30, block_table entries out of range inside the used pages, cu_seqlens_q beyond total_q: every
    index is clamped (len_k to [0, capacity], an entry to [0, num_pages), the query range to [0, total_q]), so the launch
    completes, the margins around o and lse keep their sentinel, nothing undefined is formed from the finite inputs, and the next
    launch on the device gives the 16-bit call's bits.  (The property is read from results and sentinels; nothing here is meant
    to fault.)"""
    Hq, Hkv, n_seqs, cap, Tq, M, SENT = 8, 2, 4, 512, 400, 64, 777.0
    gen = torch.Generator().manual_seed(71)
    q = torch.randn((Tq, Hq, 128), generator=gen).to(dtype).to(DEV)
    if form == "contiguous":
        kc, vc = (torch.randn((n_seqs, cap, Hkv, 128), generator=gen).to(DEV).to(F8) for _ in range(2))
        table = None
    else:
        page = int(form[4:])
        per_seq = cap // page
        kc, vc = (torch.randn((n_seqs * per_seq + 2, page, Hkv, 128), generator=gen).to(DEV).to(F8) for _ in range(2))
        table = torch.tensor([-3, 2 ** 30, kc.shape[0], 1, -(2 ** 31), 2 ** 31 - 1, 0, 5] * (n_seqs * per_seq), dtype=torch.int64)[:n_seqs * per_seq]
        table = table.to(torch.int32).view(n_seqs, per_seq).to(DEV)
    lens_t = _lens([-5, 2 ** 30, 300, -(2 ** 31)])
    cuq_t = _lens([-7, 100, 5000, 2 ** 30, 2 ** 31 - 1])
    kd, vd = _descales("pow2", Hkv, n_seqs)
    ob = torch.full((Tq + 2 * M, Hq, 128), SENT, dtype=dtype, device=DEV)
    lse_in = torch.full((Hq * Tq + 2 * M,), SENT, dtype=torch.float32, device=DEV)
    lse_v = lse_in[M:M + Hq * Tq].view(Hq, Tq)
    _launch_c(q, kc, vc, ob[M:M + Tq], lse_v, cuq_t, n_seqs, 256, lens_t, table, causal, kd, vd)
    torch.cuda.synchronize()
    assert (ob[:M] == SENT).all() and (ob[M + Tq:] == SENT).all()
    assert (lse_in[:M] == SENT).all() and (lse_in[M + Hq * Tq:] == SENT).all()
    assert not torch.isnan(ob.float()).any() and not torch.isnan(lse_in).any()
    # a later launch on the device still works
    c = _case8((8, 2))
    kd9, vd9 = _descales("pow2", 2)
    kc2, vc2, table2 = _form(form, c["k8"], c["v8"], LENS_K)
    o, lse = flash_attention.forward_varlen_kvcache(c["q"].to(dtype), kc2, vc2, c["cuq_t"], c["mq"], _lens(LENS_K), block_table=table2,
                                                    causal=causal, k_descale=kd9, v_descale=vd9)
    torch.cuda.synchronize()
    o_ref, lse_ref = _ref16(dtype, causal, (8, 2), "pow2")
    assert _same(o, o_ref) and _same(lse, lse_ref)


# ---- 7. the decode kernel on the same fp8 paged cache --------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("causal", [False, True], ids=["plain", "causal"])
@pytest.mark.parametrize("shape", [(1, 4, 4), (4, 8, 2), (16, 4, 1), (3, 4, 4), (8, 8, 1)])   # (seqlen_q, Hq, Hkv): seqlen_q * G <= 64
def test_agrees_with_forward_kvcache(dtype, causal, shape):
    Sq, Hq, Hkv = shape
    assert Sq * (Hq // Hkv) <= 64
    lens = [777, 1, 0, 2048, 5, 300, Sq, max(Sq - 1, 0)]   # cache_seqlens, the new tokens included; some shorter than seqlen_q
    n, cap = len(lens), 2048
    gen = torch.Generator().manual_seed(41)
    q = torch.randn((n, Sq, Hq, 128), generator=gen).to(dtype).to(DEV)
    k8, v8, kd, vd = flash_attention.quantize_kvcache_fp8(*(torch.randn((n, cap, Hkv, 128), generator=gen).to(DEV) * s for s in (1.3, 0.8)))
    kdq, vdq = _dequant(k8, kd), _dequant(v8, vd)
    kp, vp, table = _form("page256", k8, v8, lens, poison=True)   # one paged cache object for both calls
    lens_t = _lens(lens)
    o_d, lse_d = flash_attention.forward_kvcache(q, kp, vp, lens_t, block_table=table, causal=causal, return_lse=True, k_descale=kd, v_descale=vd)
    cuq_t, _ = _cu([Sq] * n)
    o, lse = flash_attention.forward_varlen_kvcache(q.reshape(n * Sq, Hq, 128), kp, vp, cuq_t, Sq, lens_t, block_table=table, causal=causal,
                                                    k_descale=kd, v_descale=vd)
    torch.cuda.synchronize()
    o, lse = o.view(n, Sq, Hq, 128), lse.view(Hq, n, Sq)
    lse_d = lse_d.permute(1, 0, 2)
    assert torch.equal(lse == NEG_INF, lse_d == NEG_INF)
    live = lse != NEG_INF
    assert (lse[live] - lse_d[live]).abs().max().item() <= LSE_TOL
    for b in range(n):
        dead = Sq if lens[b] == 0 else (max(Sq - lens[b], 0) if causal else 0)
        assert (lse[:, b, :dead] == NEG_INF).all() and torch.isfinite(lse[:, b, dead:]).all(), b
        assert (o[b, :dead] == 0).all() and (o_d[b, :dead] == 0).all(), b
        if lens[b] == 0:
            continue
        qb, kb, vb = q[b], kdq[b, :lens[b]], vdq[b, :lens[b]]
        _check_sequence(f"batch {b}", o[b], lse[:, b], qb, kb, vb, causal, dtype)
        o32 = _eager(qb.float(), kb, vb, causal, torch.float32)
        tol = max(O_TOL[dtype], 2 * (_eager(qb, kb, vb, causal, dtype).float() - o32).abs().max().item())
        err = (o[b].float() - o_d[b].float()).abs().max().item()
        print(f"batch {b} (len {lens[b]}): |O_prefill - O_decode| {err:.3e} tol {tol:.3e}")
        assert err <= tol, (b, lens[b], err, tol)


# ---- 8. chunked prefill end to end ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
def test_chunked_prefill_end_to_end(dtype):
    """Three sequences with 0, 100 and 257 keys already cached take two chunks of 130 tokens each: append_kvcache quantizes a chunk's
    keys into the paged fp8 cache with fixed descales and advances the lengths in place, forward_varlen_kvcache(causal=True) attends
    from the chunk's queries.  Every chunk's rows against causal fp32 eager on the cache as it stands, dequantized."""
    Hq, Hkv, page, chunk, n_chunks = 8, 2, 64, 130, 2
    prior = [0, 100, 257]
    n = len(prior)
    full = [p + chunk * n_chunks for p in prior]
    gen = torch.Generator().manual_seed(51)
    T = sum(full)
    q_all = torch.randn((T, Hq, 128), generator=gen).to(dtype).to(DEV)
    k_all, v_all = (torch.randn((T, Hkv, 128), generator=gen).to(dtype).to(DEV) for _ in range(2))
    _, cu = _cu(full)
    kd = (torch.tensor([[5.0, 5.5], [6.0, 4.5], [5.25, 6.5]]) / 448.0).to(DEV)
    vd = (torch.tensor([[4.5, 6.0], [5.0, 5.75], [6.25, 5.0]]) / 448.0).to(DEV)
    cap = 576
    per_seq = cap // page
    num_pages = n * per_seq + 3
    perm = torch.randperm(num_pages, generator=torch.Generator().manual_seed(3))[:n * per_seq].view(n, per_seq)
    kp = torch.full((num_pages, page, Hkv, 128), NAN8, dtype=U8, device=DEV)   # everything NaN until it is written
    vp = torch.full_like(kp, NAN8)
    for b, m in enumerate(prior):
        for j in range(0, m, page):
            rows = min(page, m - j)
            for pages, src, d in ((kp, k_all, kd), (vp, v_all, vd)):
                x = src[cu[b] + j:cu[b] + j + rows].float() / d[b][None, :, None]
                pages[perm[b, j // page], :rows] = x.clamp(-448.0, 448.0).to(F8).view(U8)
    kp, vp = kp.view(F8), vp.view(F8)
    table = perm.to(torch.int32).to(DEV)
    lens_t = _lens(prior)
    cuq_t, _ = _cu([chunk] * n)
    for c in range(n_chunks):
        rows = [slice(cu[b] + prior[b] + c * chunk, cu[b] + prior[b] + (c + 1) * chunk) for b in range(n)]
        k_new = torch.stack([k_all[r] for r in rows])
        v_new = torch.stack([v_all[r] for r in rows])
        flash_attention.append_kvcache(kp, vp, k_new, v_new, lens_t, block_table=table, seqlens_out=lens_t, k_descale=kd, v_descale=vd)
        q_chunk = torch.cat([q_all[r] for r in rows])
        o, lse = flash_attention.forward_varlen_kvcache(q_chunk, kp, vp, cuq_t, chunk, lens_t, block_table=table, causal=True,
                                                        k_descale=kd, v_descale=vd)
        torch.cuda.synchronize()
        assert lens_t.tolist() == [m + (c + 1) * chunk for m in prior]
        for b in range(n):
            m = prior[b] + (c + 1) * chunk
            used = (m + page - 1) // page
            kb, vb = (torch.cat([pages.view(U8)[perm[b, p]] for p in range(used)])[:m].view(F8).float() * d[b][None, :, None]
                      for pages, d in ((kp, kd), (vp, vd)))
            assert torch.isfinite(kb).all() and torch.isfinite(vb).all()
            sq = slice(b * chunk, (b + 1) * chunk)
            _check_sequence(f"chunk {c} seq {b}", o[sq], lse[:, sq], q_chunk[sq], kb, vb, True, dtype)


# ---- 9, 10. determinism and graph capture --------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("form", FORMS)
def test_deterministic(dtype, form):
    c = _quantized_case((8, 2))
    kc, vc, table = _form(form, c["k8"], c["v8"], LENS_K)
    args = (c["q"].to(dtype), kc, vc, _cu(LENS_Q)[0], max(LENS_Q), _lens(LENS_K))
    a = flash_attention.forward_varlen_kvcache(*args, block_table=table, causal=True, k_descale=c["kd"], v_descale=c["vd"])
    b = flash_attention.forward_varlen_kvcache(*args, block_table=table, causal=True, k_descale=c["kd"], v_descale=c["vd"])
    torch.cuda.synchronize()
    assert _same(a[0], b[0]) and _same(a[1], b[1])


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
def test_graph_replays_rewritten_lengths_offsets_table_and_descales(dtype):
    """One capture, replayed after cache_seqlens, cu_seqlens_q, block_table and both descales were rewritten in place: the host
    reads none of them, so the replay has the bits of a fresh call on the new contents."""
    Hq, Hkv, Tq, cap, page, n = 8, 2, 600, 512, 64, 3
    gen = torch.Generator().manual_seed(17)
    q = torch.randn((Tq, Hq, 128), generator=gen).to(dtype).to(DEV)
    k8, v8 = (torch.randn((n, cap, Hkv, 128), generator=gen).to(DEV).to(F8) for _ in range(2))
    # two paginations of the same rows in one pool of pages: the second table names other pages
    kp1, vp1, t1 = _form("page64", k8, v8, [cap] * n, seed=5)
    kp2, vp2, t2 = _form("page64", k8, v8, [cap] * n, seed=6)
    kp, vp = torch.cat([kp1.view(U8), kp2.view(U8)]).view(F8), torch.cat([vp1.view(U8), vp2.view(U8)]).view(F8)
    tables = [t1, t2 + kp1.shape[0], t1]
    layouts = [([300, 200, 100], [512, 130, 64]), ([1, 470, 129], [65, 500, 0]), ([0, 300, 300], [300, 17, 512])]   # (len_q, len_k): one total_q
    scales = [tuple(torch.rand((n, Hkv), generator=gen).to(DEV) * 0.02 + s for _ in range(2)) for s in (0.004, 0.01, 0.007)]
    mq = 470
    assert _capi.load().fa_init() == 0   # (the per-device setup queries the device: before the capture)
    cuq_t, lens_t, table = _cu(layouts[0][0])[0], _lens(layouts[0][1]), tables[0].clone()
    kd, vd = scales[0][0].clone(), scales[0][1].clone()
    flash_attention.forward_varlen_kvcache(q, kp, vp, cuq_t, mq, lens_t, block_table=table, causal=True, k_descale=kd, v_descale=vd)   # (warm up)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        got = flash_attention.forward_varlen_kvcache(q, kp, vp, cuq_t, mq, lens_t, block_table=table, causal=True, k_descale=kd, v_descale=vd)
    for (lq, lk), tb, (kd_new, vd_new) in zip(layouts, tables, scales):
        cuq_t.copy_(_cu(lq)[0])
        lens_t.copy_(_lens(lk))
        table.copy_(tb)
        kd.copy_(kd_new)
        vd.copy_(vd_new)
        for t in got:
            t.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        want = flash_attention.forward_varlen_kvcache(q, kp, vp, _cu(lq)[0], mq, _lens(lk), block_table=tb.clone(), causal=True,
                                                      k_descale=kd_new.clone(), v_descale=vd_new.clone())
        torch.cuda.synchronize()
        assert _same(want[0], got[0]) and _same(want[1], got[1]), (lq, lk)
        _, cuq = _cu(lq)
        kdq, vdq = _dequant(k8, kd_new), _dequant(v8, vd_new)
        for i in range(n):   # ... and they are the right ones
            sq = slice(cuq[i], cuq[i + 1])
            _check_sequence(f"graph seq {i}", got[0][sq], got[1][:, sq], q[sq], kdq[i, :lk[i]], vdq[i, :lk[i]], True, dtype)


# ---- 11. refusals on the device ------------------------------------------------------------------------------------------------------

def test_refusals_on_device():
    q = torch.zeros((8, 4, 128), dtype=torch.bfloat16, device=DEV)
    cu = torch.tensor([0, 4, 8], dtype=torch.int32, device=DEV)
    lens = torch.tensor([4, 4], dtype=torch.int32, device=DEV)
    cache = torch.zeros((2, 96, 2, 128), dtype=torch.bfloat16, device=DEV)
    c8 = cache.to(F8)
    ones = torch.ones((2, 2), device=DEV)
    fn = flash_attention.forward_varlen_kvcache
    for kw in (dict(), dict(k_descale=ones), dict(v_descale=ones)):
        with pytest.raises(RuntimeError, match="fp8 cache is not served without both"):
            fn(q, c8, c8, cu, 4, lens, **kw)
    with pytest.raises(RuntimeError, match="belong to an fp8"):
        fn(q, cache, cache, cu, 4, lens, k_descale=ones, v_descale=ones)
    with pytest.raises(RuntimeError, match="one data type"):
        fn(q, c8, cache, cu, 4, lens, k_descale=ones, v_descale=ones)
    with pytest.raises(RuntimeError, match="must be torch.float8_e4m3fn"):
        fn(q, cache.to(torch.float8_e5m2), cache.to(torch.float8_e5m2), cu, 4, lens, k_descale=ones, v_descale=ones)
    for bad in (ones.double(), torch.ones((3, 2), device=DEV), torch.ones((2, 4), device=DEV)[:, ::2], ones.cpu()):
        with pytest.raises(RuntimeError, match="k_descale must be"):
            fn(q, c8, c8, cu, 4, lens, k_descale=bad, v_descale=ones)
    with pytest.raises(RuntimeError, match="multiple of 64"):
        fn(q, c8, c8, cu, 4, lens, block_table=torch.zeros((2, 1), dtype=torch.int32, device=DEV), k_descale=ones, v_descale=ones)
    with pytest.raises(RuntimeError, match="one batch entry per sequence"):
        fn(q, c8[:1], c8[:1], cu, 4, lens, k_descale=ones, v_descale=ones)
    odd = torch.zeros((2, 96, 2, 136), dtype=torch.bfloat16, device=DEV).to(F8)[..., :128]   # a head stride of 136 bytes
    with pytest.raises(RuntimeError, match="multiples of 16"):
        fn(q, odd, odd, cu, 4, lens, k_descale=ones, v_descale=ones)
    # descale rows of two strides, or of a stride shorter than a row (expanded), are served (copied), like the call these were derived from
    wide = torch.ones((2, 4), device=DEV)[:, :2]
    for kd_, vd_ in ((wide, ones), (torch.ones((1, 2), device=DEV).expand(2, 2), ones)):
        o, lse = fn(q, c8, c8, cu, 4, lens, k_descale=kd_, v_descale=vd_)
        torch.cuda.synchronize()
        assert (o == 0).all() and torch.isfinite(lse).all()
