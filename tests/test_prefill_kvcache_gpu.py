"""Prefill against a KV cache on the MI355X: flash_attention.forward_varlen_kvcache.

The main oracle is the packed path: forward_varlen(cu_seqlens_k=) on the same keys packed walks the same 64-key tiles in the same
order with the same arithmetic, so o and lse must have its bits, for a contiguous and for a paged cache.  Beside it: fp32 eager
attention per sequence with the decode tests' rule, |O - O32| <= max(O_TOL, 2 |O_eager16 - O32|) (O_TOL 2^-6 bf16 / 2^-9 fp16), lse
within 1e-3, rows without keys exactly 0 / -inf; isolation from everything the lengths and the table do not name; garbage in the
three device arrays; forward_kvcache on the same paged cache; a chunked prefill through append_kvcache; determinism and a graph.
The shapes are the smallest that reach every path: ragged and whole tiles, one and several Q blocks, one and several pages, a page
of one tile and of four, empty sides, more queries than keys."""
import ctypes
import functools
import math

import pytest
import torch

import flash_attention
from flash_attention_from_scratch_amd import _capi
from flash_attention_from_scratch_amd import flash_attention_kernels as fak

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
DTYPES = [torch.bfloat16, torch.float16]
O_TOL = {torch.bfloat16: 2.0 ** -6, torch.float16: 2.0 ** -9}
LSE_TOL = 1e-3
HEADS = [(4, 4), (8, 2), (4, 1)]
NEG_INF = float("-inf")
# (len_q, len_k) per sequence
PAIRS = [(165, 197), (37, 1000), (1, 777), (128, 192), (300, 100), (0, 300), (200, 0), (64, 64), (129, 65)]
CAP = 1024   # rows per sequence of the caches built from PAIRS (a multiple of both page sizes)
FORMS = ["contiguous", "page64", "page256"]


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


@functools.lru_cache(maxsize=None)
def _packed_case(dtype, causal, heads):
    """PAIRS as packed q, k, v with forward_varlen(cu_seqlens_k=)'s o and lse on them: computed once, shared, never written."""
    Hq, Hkv = heads
    gen = torch.Generator().manual_seed(100 + Hkv)
    Tq, Tk = sum(p[0] for p in PAIRS), sum(p[1] for p in PAIRS)
    q = torch.randn((Tq, Hq, 128), generator=gen).to(dtype).to(DEV)
    k, v = (torch.randn((Tk, Hkv, 128), generator=gen).to(dtype).to(DEV) for _ in range(2))
    cuq_t, cuq = _cu([p[0] for p in PAIRS])
    cuk_t, cuk = _cu([p[1] for p in PAIRS])
    mq, mk = max(p[0] for p in PAIRS), max(p[1] for p in PAIRS)
    o, lse = flash_attention.forward_varlen(q, k, v, cuq_t, mq, causal=causal, cu_seqlens_k=cuk_t, max_seqlen_k=mk)
    torch.cuda.synchronize()
    return dict(q=q, k=k, v=v, cuq_t=cuq_t, cuq=cuq, cuk=cuk, mq=mq, mk=mk, o=o, lse=lse)


def _contiguous(k, v, cuk, cap, fill=0.0):
    """packed keys -> (n_seqs, cap, Hkv, 128) caches, sequence b's keys at rows 0 .. len - 1 of entry b, `fill` beyond"""
    B = len(cuk) - 1
    kc = torch.full((B, cap) + tuple(k.shape[1:]), fill, dtype=k.dtype, device=k.device)
    vc = torch.full_like(kc, fill)
    for b in range(B):
        n = cuk[b + 1] - cuk[b]
        kc[b, :n] = k[cuk[b]:cuk[b + 1]]
        vc[b, :n] = v[cuk[b]:cuk[b + 1]]
    return kc, vc


def _paginate(kc, vc, lens, page_size, poison, seed=3, spare=3):
    """Contiguous caches scattered into shuffled pages -> (k pages, v pages, block_table).  poison: unused pages and rows at or
    beyond len hold NaN, and the block_table entries beyond the used pages hold -1 and 2^30 in turn."""
    B, cap, Hkv, D = kc.shape
    per_seq = (cap + page_size - 1) // page_size
    num_pages = B * per_seq + spare
    perm = torch.randperm(num_pages, generator=torch.Generator().manual_seed(seed))[:B * per_seq].view(B, per_seq)
    fill = math.nan if poison else 0.0
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
            junk = torch.tensor([-1, 2 ** 30] * per_seq, dtype=torch.int32)
            table[b, used:] = junk[:per_seq - used]
    return kp, vp, table.to(kc.device)


def _cache(form, k, v, cuk, cap, poison=False, seed=3):
    """-> (k_cache, v_cache, block_table or None) holding the packed keys in the named form"""
    kc, vc = _contiguous(k, v, cuk, cap, fill=math.nan if poison else 0.0)
    if form == "contiguous":
        return kc, vc, None
    lens = [cuk[b + 1] - cuk[b] for b in range(len(cuk) - 1)]
    return _paginate(kc, vc, lens, int(form[4:]), poison, seed=seed)


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
    """one sequence's o (n_q, H, D) and lse (H, n_q) against the fp32 rule; the rows without keys exactly"""
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


def _launch_c(q, kc, vc, o, lse, cuq_t, n_seqs, mq, lens_t, table, causal, max_seqlen_k=0):
    """the launch through the C ABI on the caller's o and lse (q, o contiguous (T, H, 128); lse (H, T))"""
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
    opts = _capi.make_opts(causal=causal)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    _capi.check(lib.fa_fwd_launch_varlen_kvcache(ctypes.byref(args), ctypes.byref(kv), ctypes.byref(vq), ctypes.byref(layout),
                                                 ctypes.byref(opts), ctypes.c_void_p(lse.data_ptr()), stream))


# ---- 1. the packed path's bits -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("causal", [False, True], ids=["plain", "causal"])
@pytest.mark.parametrize("heads", HEADS)
@pytest.mark.parametrize("form", FORMS)
def test_bit_identical_to_the_packed_path(dtype, causal, heads, form):
    c = _packed_case(dtype, causal, heads)
    kc, vc, table = _cache(form, c["k"], c["v"], c["cuk"], CAP)
    lens_t = _lens([p[1] for p in PAIRS])
    # (the contiguous cache with the capacity as the bound, the paged ones with the packed call's bound: the same clamp)
    o, lse = flash_attention.forward_varlen_kvcache(c["q"], kc, vc, c["cuq_t"], c["mq"], lens_t, block_table=table, causal=causal,
                                                    max_seqlen_k=None if table is None else c["mk"])
    torch.cuda.synchronize()
    assert o.shape == c["q"].shape and lse.shape == (heads[0], c["q"].shape[0]) and lse.dtype == torch.float32
    assert _same(o, c["o"]), "o"
    assert _same(lse, c["lse"]), "lse"


# ---- 2. fp32 eager per sequence ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("causal", [False, True], ids=["plain", "causal"])
@pytest.mark.parametrize("heads", HEADS)
@pytest.mark.parametrize("form", ["contiguous", "page64"])
def test_against_fp32_eager_per_sequence(dtype, causal, heads, form):
    c = _packed_case(dtype, causal, heads)
    kc, vc, table = _cache(form, c["k"], c["v"], c["cuk"], CAP)
    o, lse = flash_attention.forward_varlen_kvcache(c["q"], kc, vc, c["cuq_t"], c["mq"], _lens([p[1] for p in PAIRS]), block_table=table,
                                                    causal=causal)
    torch.cuda.synchronize()
    cuq, cuk = c["cuq"], c["cuk"]
    for i in range(len(PAIRS)):
        sq, sk = slice(cuq[i], cuq[i + 1]), slice(cuk[i], cuk[i + 1])
        _check_sequence(f"seq {i}", o[sq], lse[:, sq], c["q"][sq], c["k"][sk], c["v"][sk], causal, dtype)


# ---- 3. isolation ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("causal", [False, True], ids=["plain", "causal"])
@pytest.mark.parametrize("heads", HEADS)
@pytest.mark.parametrize("form", FORMS)
def test_isolation(dtype, causal, heads, form):
    """NaN in every unused page, in every cache row at or beyond len_k and in the q rows outside the sequences' ranges, -1 and
    2^30 in the unused block_table entries: the rows of the ranges are bit-identical to the clean run, and the rows of o and lse
    outside every range keep their sentinel."""
    c = _packed_case(dtype, causal, heads)
    Hq, M, SENT = heads[0], 37, 777.0
    Tq = c["q"].shape[0]
    cuq_t, _ = _cu([p[0] for p in PAIRS], first=M)
    lens_t = _lens([p[1] for p in PAIRS])
    got = []
    for poison in (False, True):
        kc, vc, table = _cache(form, c["k"], c["v"], c["cuk"], CAP, poison=poison)
        q = torch.full((Tq + 2 * M, Hq, 128), math.nan if poison else 0.0, dtype=dtype, device=DEV)
        q[M:M + Tq] = c["q"]
        o = torch.full_like(q, math.nan if poison else SENT)
        o[:M] = SENT
        o[M + Tq:] = SENT
        lse = torch.full((Hq, Tq + 2 * M), SENT, dtype=torch.float32, device=DEV)
        _launch_c(q, kc, vc, o, lse, cuq_t, len(PAIRS), c["mq"], lens_t, table, causal)
        torch.cuda.synchronize()
        assert (o[:M] == SENT).all() and (o[M + Tq:] == SENT).all(), poison
        assert (lse[:, :M] == SENT).all() and (lse[:, M + Tq:] == SENT).all(), poison
        got.append((o[M:M + Tq], lse[:, M:M + Tq]))
    (o_clean, lse_clean), (o_p, lse_p) = got
    assert torch.isfinite(o_p.float()).all() and not torch.isnan(lse_p).any()
    assert _same(o_p, o_clean) and _same(lse_p, lse_clean)
    assert _same(o_clean, c["o"]) and _same(lse_clean, c["lse"])   # (the range's offset in q moves no bit either)


# ---- 4. garbage stays inside -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("causal", [False, True], ids=["plain", "causal"])
@pytest.mark.parametrize("form", FORMS)
def test_garbage_in_the_device_arrays_stays_inside_the_tensors(dtype, causal, form):
    """cache_seqlens of -5 and 2^30, block_table entries out of range inside the used pages, cu_seqlens_q beyond total_q: every
    index is clamped (len_k to [0, capacity], an entry to [0, num_pages), the query range to [0, total_q]), so the launch
    completes, the margins around o and lse keep their sentinel, nothing undefined is formed from the finite inputs, and the next
    launch on the device gives the packed path's bits."""
    Hq, Hkv, B, cap, Tq, M, SENT = 8, 2, 4, 512, 400, 64, 777.0
    gen = torch.Generator().manual_seed(71)
    q = torch.randn((Tq, Hq, 128), generator=gen).to(dtype).to(DEV)
    if form == "contiguous":
        kc, vc = (torch.randn((B, cap, Hkv, 128), generator=gen).to(dtype).to(DEV) for _ in range(2))
        table = None
    else:
        page = int(form[4:])
        per_seq = cap // page
        kc, vc = (torch.randn((B * per_seq + 2, page, Hkv, 128), generator=gen).to(dtype).to(DEV) for _ in range(2))
        table = torch.tensor([-3, 2 ** 30, kc.shape[0], 1, -(2 ** 31), 2 ** 31 - 1, 0, 5] * (B * per_seq), dtype=torch.int64)[:B * per_seq]
        table = table.to(torch.int32).view(B, per_seq).to(DEV)
    lens_t = _lens([-5, 2 ** 30, 300, -(2 ** 31)])
    cuq_t = _lens([-7, 100, 5000, 2 ** 30, 2 ** 31 - 1])
    ob = torch.full((Tq + 2 * M, Hq, 128), SENT, dtype=dtype, device=DEV)
    lse_in = torch.full((Hq * Tq + 2 * M,), SENT, dtype=torch.float32, device=DEV)
    lse_v = lse_in[M:M + Hq * Tq].view(Hq, Tq)
    _launch_c(q, kc, vc, ob[M:M + Tq], lse_v, cuq_t, B, 256, lens_t, table, causal)
    torch.cuda.synchronize()
    assert (ob[:M] == SENT).all() and (ob[M + Tq:] == SENT).all()
    assert (lse_in[:M] == SENT).all() and (lse_in[M + Hq * Tq:] == SENT).all()
    assert not torch.isnan(ob.float()).any() and not torch.isnan(lse_in).any()
    # a later launch on the device still works
    c = _packed_case(dtype, causal, (8, 2))
    kc2, vc2, table2 = _cache(form, c["k"], c["v"], c["cuk"], CAP)
    o, lse = flash_attention.forward_varlen_kvcache(c["q"], kc2, vc2, c["cuq_t"], c["mq"], _lens([p[1] for p in PAIRS]), block_table=table2,
                                                    causal=causal)
    torch.cuda.synchronize()
    assert _same(o, c["o"]) and _same(lse, c["lse"])


# ---- 5. the decode kernel on the same paged cache ----------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("causal", [False, True], ids=["plain", "causal"])
@pytest.mark.parametrize("shape", [(1, 4, 4), (4, 8, 2), (16, 4, 1), (3, 4, 4), (8, 8, 1)])   # (seqlen_q, Hq, Hkv): seqlen_q * G <= 64
def test_agrees_with_forward_kvcache(dtype, causal, shape):
    Sq, Hq, Hkv = shape
    assert Sq * (Hq // Hkv) <= 64
    lens = [777, 1, 0, 2048, 5, 300, Sq, max(Sq - 1, 0)]   # cache_seqlens, the new tokens included; some shorter than seqlen_q
    B, cap = len(lens), 2048
    gen = torch.Generator().manual_seed(41)
    q = torch.randn((B, Sq, Hq, 128), generator=gen).to(dtype).to(DEV)
    kc_, vc_ = (torch.randn((B, cap, Hkv, 128), generator=gen).to(dtype).to(DEV) for _ in range(2))
    kp, vp, table = _paginate(kc_, vc_, lens, 256, poison=True)   # one paged cache object for both calls
    lens_t = _lens(lens)
    o_d, lse_d = flash_attention.forward_kvcache(q, kp, vp, lens_t, block_table=table, causal=causal, return_lse=True)
    cuq_t, _ = _cu([Sq] * B)
    o, lse = flash_attention.forward_varlen_kvcache(q.reshape(B * Sq, Hq, 128), kp, vp, cuq_t, Sq, lens_t, block_table=table, causal=causal)
    torch.cuda.synchronize()
    o, lse = o.view(B, Sq, Hq, 128), lse.view(Hq, B, Sq)
    lse_d = lse_d.permute(1, 0, 2)
    assert torch.equal(lse == NEG_INF, lse_d == NEG_INF)
    live = lse != NEG_INF
    assert (lse[live] - lse_d[live]).abs().max().item() <= LSE_TOL
    for b in range(B):
        dead = Sq if lens[b] == 0 else (max(Sq - lens[b], 0) if causal else 0)
        assert (lse[:, b, :dead] == NEG_INF).all() and torch.isfinite(lse[:, b, dead:]).all(), b
        assert (o[b, :dead] == 0).all() and (o_d[b, :dead] == 0).all(), b
        if lens[b] == 0:
            continue
        qb, kb, vb = q[b], kc_[b, :lens[b]], vc_[b, :lens[b]]
        _check_sequence(f"batch {b}", o[b], lse[:, b], qb, kb, vb, causal, dtype)
        o32 = _eager(qb.float(), kb.float(), vb.float(), causal, torch.float32)
        tol = max(O_TOL[dtype], 2 * (_eager(qb, kb, vb, causal, dtype).float() - o32).abs().max().item())
        err = (o[b].float() - o_d[b].float()).abs().max().item()
        print(f"batch {b} (len {lens[b]}): |O_prefill - O_decode| {err:.3e} tol {tol:.3e}")
        assert err <= tol, (b, lens[b], err, tol)


# ---- 6. chunked prefill end to end ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
def test_chunked_prefill_end_to_end(dtype):
    """Three sequences with 0, 100 and 257 keys already cached take two chunks of 130 tokens each: append_kvcache writes a chunk's
    keys into the paged cache and advances the lengths in place, forward_varlen_kvcache(causal=True) attends from the chunk's
    queries.  The chunks' outputs are the rows of causal forward_varlen over each whole sequence, bit for bit: a row meets the
    same 64-key tiles, last to first, from its diagonal's tile down."""
    Hq, Hkv, page, chunk, n_chunks = 8, 2, 64, 130, 2
    prior = [0, 100, 257]
    B = len(prior)
    full = [n + chunk * n_chunks for n in prior]
    gen = torch.Generator().manual_seed(51)
    T = sum(full)
    q_all = torch.randn((T, Hq, 128), generator=gen).to(dtype).to(DEV)
    k_all, v_all = (torch.randn((T, Hkv, 128), generator=gen).to(dtype).to(DEV) for _ in range(2))
    cu_t, cu = _cu(full)
    o_ref, lse_ref = flash_attention.forward_varlen(q_all, k_all, v_all, cu_t, max(full), causal=True)
    # the cache: the prior keys in shuffled pages, everything else NaN until a chunk is appended
    cap = 576
    per_seq = cap // page
    num_pages = B * per_seq + 3
    perm = torch.randperm(num_pages, generator=torch.Generator().manual_seed(3))[:B * per_seq].view(B, per_seq)
    kp = torch.full((num_pages, page, Hkv, 128), math.nan, dtype=dtype, device=DEV)
    vp = torch.full_like(kp, math.nan)
    for b, n in enumerate(prior):
        for j in range(0, n, page):
            rows = min(page, n - j)
            kp[perm[b, j // page], :rows] = k_all[cu[b] + j:cu[b] + j + rows]
            vp[perm[b, j // page], :rows] = v_all[cu[b] + j:cu[b] + j + rows]
    table = perm.to(torch.int32).to(DEV)
    lens_t = _lens(prior)
    cuq_t, _ = _cu([chunk] * B)
    for c in range(n_chunks):
        rows = [slice(cu[b] + prior[b] + c * chunk, cu[b] + prior[b] + (c + 1) * chunk) for b in range(B)]
        k_new = torch.stack([k_all[r] for r in rows])
        v_new = torch.stack([v_all[r] for r in rows])
        flash_attention.append_kvcache(kp, vp, k_new, v_new, lens_t, block_table=table, seqlens_out=lens_t)
        q_chunk = torch.cat([q_all[r] for r in rows])
        o, lse = flash_attention.forward_varlen_kvcache(q_chunk, kp, vp, cuq_t, chunk, lens_t, block_table=table, causal=True)
        torch.cuda.synchronize()
        assert lens_t.tolist() == [n + (c + 1) * chunk for n in prior]
        for b, r in enumerate(rows):
            assert _same(o[b * chunk:(b + 1) * chunk], o_ref[r]), (c, b, "o")
            assert _same(lse[:, b * chunk:(b + 1) * chunk], lse_ref[:, r]), (c, b, "lse")


# ---- 7. determinism and graph capture ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("form", FORMS)
def test_deterministic(dtype, form):
    c = _packed_case(dtype, True, (8, 2))
    kc, vc, table = _cache(form, c["k"], c["v"], c["cuk"], CAP)
    lens_t = _lens([p[1] for p in PAIRS])
    a = flash_attention.forward_varlen_kvcache(c["q"], kc, vc, c["cuq_t"], c["mq"], lens_t, block_table=table, causal=True)
    b = flash_attention.forward_varlen_kvcache(c["q"], kc, vc, c["cuq_t"], c["mq"], lens_t, block_table=table, causal=True)
    torch.cuda.synchronize()
    assert _same(a[0], b[0]) and _same(a[1], b[1])


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
def test_graph_replays_rewritten_lengths_offsets_and_table(dtype):
    """One capture, replayed after cache_seqlens, cu_seqlens_q and block_table were rewritten in place: the host reads none of
    them, so the replay has the bits of a fresh call on the new contents."""
    Hq, Hkv, Tq, cap, page, B = 8, 2, 600, 512, 64, 3
    gen = torch.Generator().manual_seed(17)
    q = torch.randn((Tq, Hq, 128), generator=gen).to(dtype).to(DEV)
    kc, vc = (torch.randn((B, cap, Hkv, 128), generator=gen).to(dtype).to(DEV) for _ in range(2))
    # two paginations of the same rows in one pool of pages: the second table names other pages
    kp1, vp1, t1 = _paginate(kc, vc, [cap] * B, page, poison=False, seed=5)
    kp2, vp2, t2 = _paginate(kc, vc, [cap] * B, page, poison=False, seed=6)
    kp, vp = torch.cat([kp1, kp2]), torch.cat([vp1, vp2])
    tables = [t1, t2 + kp1.shape[0], t1]
    layouts = [([300, 200, 100], [512, 130, 64]), ([1, 470, 129], [65, 500, 0]), ([0, 300, 300], [300, 17, 512])]   # (len_q, len_k): one total_q
    mq = 470
    assert _capi.load().fa_init() == 0   # (the per-device setup queries the device: before the capture)
    cuq_t, lens_t, table = _cu(layouts[0][0])[0], _lens(layouts[0][1]), tables[0].clone()
    flash_attention.forward_varlen_kvcache(q, kp, vp, cuq_t, mq, lens_t, block_table=table, causal=True)   # (warm up outside the capture)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        got = flash_attention.forward_varlen_kvcache(q, kp, vp, cuq_t, mq, lens_t, block_table=table, causal=True)
    for (lq, lk), tb in zip(layouts, tables):
        cuq_t.copy_(_cu(lq)[0])
        lens_t.copy_(_lens(lk))
        table.copy_(tb)
        for t in got:
            t.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        want = flash_attention.forward_varlen_kvcache(q, kp, vp, _cu(lq)[0], mq, _lens(lk), block_table=tb.clone(), causal=True)
        torch.cuda.synchronize()
        assert _same(want[0], got[0]) and _same(want[1], got[1]), (lq, lk)
        _, cuq = _cu(lq)
        for i in range(B):   # ... and they are the right ones
            sq = slice(cuq[i], cuq[i + 1])
            _check_sequence(f"graph seq {i}", got[0][sq], got[1][:, sq], q[sq], kc[i, :lk[i]], vc[i, :lk[i]], True, dtype)


def test_refusals_on_device():
    q = torch.zeros((8, 4, 128), dtype=torch.bfloat16, device=DEV)
    cu = torch.tensor([0, 4, 8], dtype=torch.int32, device=DEV)
    lens = torch.tensor([4, 4], dtype=torch.int32, device=DEV)
    cache = torch.zeros((2, 96, 2, 128), dtype=torch.bfloat16, device=DEV)
    with pytest.raises(RuntimeError, match="multiple of 64"):
        flash_attention.forward_varlen_kvcache(q, cache, cache, cu, 4, lens, block_table=torch.zeros((2, 1), dtype=torch.int32, device=DEV))
    with pytest.raises(RuntimeError, match="one batch entry per sequence"):
        flash_attention.forward_varlen_kvcache(q, cache[:1], cache[:1], cu, 4, lens)
    with pytest.raises(RuntimeError, match="fp8 cache is not served"):
        flash_attention.forward_varlen_kvcache(q, cache.to(torch.float8_e4m3fn), cache.to(torch.float8_e4m3fn), cu, 4, lens)
    o, lse = flash_attention.forward_varlen_kvcache(q, cache, cache, cu, 4, lens)   # ... and the call these were derived from is served
    torch.cuda.synchronize()
    assert (o == 0).all() and torch.isfinite(lse).all()
