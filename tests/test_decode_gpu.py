"""KV-cache decode attention on the MI355X: flash_attention.forward_kvcache.

The oracle is fp32 eager attention per batch entry (K / V sliced to the entry's length, expanded with repeat_interleave,
bottom-right causal mask).  Tolerance for O: max|O - O32| <= max(O_TOL[dtype], 2 * max|O_eager16 - O32|), O_eager16 the same
eager attention in the 16-bit type on the same inputs -- the project's absolute rule (2^-6 bf16, 2^-9 fp16) is too tight for a
short softmax even for torch's own 16-bit arithmetic, and the factor 2 is the one the gradient rule gives torch's 16-bit result.
lse: 1e-3 absolute, -inf exactly.
"""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

O_TOL = {torch.bfloat16: 2.0 ** -6, torch.float16: 2.0 ** -9}
LSE_TOL = 1e-3
DTYPES = [torch.bfloat16, torch.float16]
DEV = "cuda:0"
LENGTHS = [0, 1, 2, 3, 17, 63, 64, 65, 127, 129, 257, 1000, 4096, 33000]


def _fa():
    import flash_attention
    return flash_attention


def _eager(q, k, v, lens, causal, dtype):
    """-> (o (B, Sq, H, D) in dtype arithmetic, lse fp32 (B, H, Sq)); rows without keys: 0 and -inf."""
    B, Sq, H, D = q.shape
    G = H // k.shape[2]
    o = torch.zeros((B, Sq, H, D), dtype=dtype, device=q.device)
    lse = torch.full((B, H, Sq), -math.inf, dtype=torch.float32, device=q.device)
    for b, n in enumerate(lens):
        if n == 0:
            continue
        qb = q[b].to(dtype).transpose(0, 1)                                       # (H, Sq, D)
        kb = k[b, :n].to(dtype).repeat_interleave(G, dim=1).transpose(0, 1)        # (H, n, D)
        vb = v[b, :n].to(dtype).repeat_interleave(G, dim=1).transpose(0, 1)
        s = (qb @ kb.transpose(1, 2)) * (1.0 / math.sqrt(D))
        if causal:
            i = torch.arange(Sq, device=q.device)[:, None]
            j = torch.arange(n, device=q.device)[None, :]
            s = s.masked_fill(j > n - Sq + i, -math.inf)
        row_lse = torch.logsumexp(s.float(), dim=-1)                                # (H, Sq)
        p = torch.softmax(s, dim=-1)
        p = torch.where(torch.isfinite(row_lse)[..., None], p, torch.zeros_like(p))
        o[b] = (p @ vb).transpose(0, 1)
        lse[b] = row_lse
    return o, lse


def _check(tag, o, lse, q, k, v, lens, causal):
    dtype = q.dtype
    o32, lse32 = _eager(q, k, v, lens, causal, torch.float32)
    o16, _ = _eager(q, k, v, lens, causal, dtype)
    err = (o.float() - o32).abs().max().item()
    ref_err = (o16.float() - o32).abs().max().item()
    bound = max(O_TOL[dtype], 2.0 * ref_err)
    print(f"{tag}: max|O - O32| = {err:.3e}  bound = {bound:.3e} (O_TOL {O_TOL[dtype]:.3e}, eager16 {ref_err:.3e})")
    assert torch.isfinite(o.float()).all(), tag
    assert err <= bound, f"{tag}: {err} > {bound}"
    if lse is not None:
        inf = torch.isinf(lse32)
        assert torch.equal(torch.isinf(lse) & (lse < 0), inf), f"{tag}: -inf rows of lse differ"
        lerr = (lse[~inf] - lse32[~inf]).abs().max().item() if (~inf).any() else 0.0
        print(f"{tag}: max|lse - lse32| = {lerr:.3e}  bound = {LSE_TOL:.1e}")
        assert lerr <= LSE_TOL, f"{tag}: lse {lerr}"


def _inputs(dtype, lens, Sq, H, Hkv, cache_len=None, seed=0):
    """Seeded N(0, 1), drawn on the device (the >= 32k caches would take minutes from the CPU generator)."""
    gen = torch.Generator(device=DEV).manual_seed(seed)
    B = len(lens)
    cache_len = cache_len or max(max(lens), 1)
    q = torch.randn((B, Sq, H, 128), generator=gen, device=DEV).to(dtype)
    k = torch.randn((B, cache_len, Hkv, 128), generator=gen, device=DEV).to(dtype)
    v = torch.randn((B, cache_len, Hkv, 128), generator=gen, device=DEV).to(dtype)
    return q, k, v, torch.tensor(lens, dtype=torch.int32, device=DEV)


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("causal", [False, True], ids=["plain", "causal"])
@pytest.mark.parametrize("H,Hkv,Sq", [(8, 8, 1), (8, 8, 4), (8, 8, 8), (8, 8, 16), (8, 2, 1), (8, 2, 4), (8, 2, 8), (8, 1, 1), (8, 1, 4),
                                      (8, 1, 8)])
def test_against_fp32_eager(dtype, causal, H, Hkv, Sq):
    """Every length class of the list mixed within one batch (so len < seqlen_q under causal is covered: 0, 1, 2, 3 against
    seqlen_q 4, 8, 16), the rule's split."""
    q, k, v, lens_t = _inputs(dtype, LENGTHS, Sq, H, Hkv)
    o, lse = _fa().forward_kvcache(q, k, v, lens_t, causal=causal, return_lse=True)
    _check(f"eager {dtype} causal={causal} H={H} Hkv={Hkv} Sq={Sq}", o, lse, q, k, v, LENGTHS, causal)


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("causal", [False, True], ids=["plain", "causal"])
def test_split_consistency(dtype, causal):
    """num_splits 1, 2, 3, 8, the rule's and one larger than the tile count (empty splits) all meet the tolerance rule, and lse
    agrees with the one-split launch to 1e-5, measured as |d| / max(|lse|, 1): relative where |lse| >= 1, absolute below.
    The bound is the issue's.  Measured on an MI355X over these inputs (both dtypes, plain and causal, 20 comparisons): at most
    1.3e-7, one or two ulp of fp32 re-association; the figure is printed per split count before it is asserted."""
    lens = [5, 64, 130, 1000, 4096, 300]
    q, k, v, lens_t = _inputs(dtype, lens, 4, 8, 2, seed=1)
    fa = _fa()
    base_lse = None
    for ns in (1, 2, 3, 8, 0, 200):
        o, lse = fa.forward_kvcache(q, k, v, lens_t, causal=causal, return_lse=True, num_splits=ns)
        _check(f"splits={ns} {dtype} causal={causal}", o, lse, q, k, v, lens, causal)
        if base_lse is None:
            base_lse = lse
        else:
            rel = ((lse - base_lse).abs() / base_lse.abs().clamp_min(1.0)).max().item()
            print(f"splits={ns}: max rel |lse - lse(1 split)| = {rel:.3e}")
            assert rel <= 1e-5, (ns, rel)


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("ns", [0, 5], ids=["rule", "forced5"])
def test_deterministic(dtype, ns):
    lens = [1000, 4096, 77, 0]
    q, k, v, lens_t = _inputs(dtype, lens, 4, 8, 2, seed=2)
    fa = _fa()
    o1, l1 = fa.forward_kvcache(q, k, v, lens_t, causal=True, return_lse=True, num_splits=ns)
    o2, l2 = fa.forward_kvcache(q, k, v, lens_t, causal=True, return_lse=True, num_splits=ns)
    assert torch.equal(o1.view(torch.int16), o2.view(torch.int16))
    assert torch.equal(l1.view(torch.int32), l2.view(torch.int32))


def _paginate(k, v, lens, page_size, poison, seed=3):
    """The contiguous caches scattered into shuffled pages.  poison: unused pages and rows at or beyond len hold NaN, and
    block_table entries beyond the used pages hold out-of-range page numbers."""
    B, cache_len, Hkv, D = k.shape
    per_seq = (cache_len + page_size - 1) // page_size
    num_pages = B * per_seq + 3
    gen = torch.Generator().manual_seed(seed)
    perm = torch.randperm(num_pages, generator=gen)[:B * per_seq].view(B, per_seq)
    fill = math.nan if poison else 0.0
    kp = torch.full((num_pages, page_size, Hkv, D), fill, dtype=k.dtype, device=k.device)
    vp = torch.full_like(kp, fill)
    table = perm.to(torch.int32).clone()
    for b, n in enumerate(lens):
        used = (n + page_size - 1) // page_size
        for p in range(used):
            rows = min(page_size, n - p * page_size) if poison else min(page_size, cache_len - p * page_size)
            kp[perm[b, p], :rows] = k[b, p * page_size:p * page_size + rows]
            vp[perm[b, p], :rows] = v[b, p * page_size:p * page_size + rows]
        if poison:
            table[b, used:] = torch.tensor([-7, num_pages, 2 ** 30][b % 3], dtype=torch.int32)
    return kp, vp, table.to(k.device)


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("page_size", [64, 256])
@pytest.mark.parametrize("ns", [1, 4], ids=["split1", "split4"])
def test_paged_equals_contiguous(dtype, page_size, ns):
    lens = [0, 1, 63, 64, 65, 257, 1000, 2048]
    q, k, v, lens_t = _inputs(dtype, lens, 4, 8, 2, cache_len=2048, seed=4)
    fa = _fa()
    o_c, lse_c = fa.forward_kvcache(q, k, v, lens_t, causal=True, return_lse=True, num_splits=ns)
    kp, vp, table = _paginate(k, v, lens, page_size, poison=False)
    o_p, lse_p = fa.forward_kvcache(q, kp, vp, lens_t, block_table=table, causal=True, return_lse=True, num_splits=ns)
    assert torch.equal(o_c.view(torch.int16), o_p.view(torch.int16))
    assert torch.equal(lse_c.view(torch.int32), lse_p.view(torch.int32))
    _check(f"paged {dtype} page={page_size} splits={ns}", o_p, lse_p, q, k, v, lens, True)


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("ns", [0, 3], ids=["rule", "forced3"])
def test_isolation(dtype, ns):
    """NaN in every cache row at or beyond len and in every unused page, out-of-range page numbers in every unused block_table
    entry: results are finite and bitwise those of the clean run; a len = 0 entry's o is exactly 0."""
    lens = [0, 1, 63, 64, 65, 257, 1000, 1500]
    q, k, v, lens_t = _inputs(dtype, lens, 4, 8, 2, cache_len=2048, seed=5)
    fa = _fa()
    o_clean, lse_clean = fa.forward_kvcache(q, k, v, lens_t, causal=False, return_lse=True, num_splits=ns)
    kn, vn = k.clone(), v.clone()
    for b, n in enumerate(lens):
        kn[b, n:] = math.nan
        vn[b, n:] = math.nan
    o, lse = fa.forward_kvcache(q, kn, vn, lens_t, causal=False, return_lse=True, num_splits=ns)
    assert torch.isfinite(o.float()).all()
    assert torch.equal(o.view(torch.int16), o_clean.view(torch.int16))
    assert torch.equal(lse.view(torch.int32), lse_clean.view(torch.int32))
    assert (o[0] == 0).all() and torch.isinf(lse[0]).all()
    kp, vp, table = _paginate(k, v, lens, 64, poison=True)
    o_p, lse_p = fa.forward_kvcache(q, kp, vp, lens_t, block_table=table, causal=False, return_lse=True, num_splits=ns)
    assert torch.isfinite(o_p.float()).all()
    assert torch.equal(o_p.view(torch.int16), o_clean.view(torch.int16))
    assert torch.equal(lse_p.view(torch.int32), lse_clean.view(torch.int32))


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
def test_gqa_packing_matches_mha_on_expanded_kv(dtype):
    """Within the tolerance rule (the packed rows of a group share one launch's row tiles with other heads than under MHA, and
    the rule's split differs with n_kv_heads, so the bits are not pinned)."""
    lens = [17, 129, 1000, 4096]
    q, k, v, lens_t = _inputs(dtype, lens, 4, 8, 2, seed=6)
    fa = _fa()
    o_g, lse_g = fa.forward_kvcache(q, k, v, lens_t, causal=True, return_lse=True)
    ke, ve = k.repeat_interleave(4, dim=2), v.repeat_interleave(4, dim=2)
    o_m, lse_m = fa.forward_kvcache(q, ke, ve, lens_t, causal=True, return_lse=True)
    _check(f"gqa {dtype}", o_g, lse_g, q, k, v, lens, True)
    _check(f"mha-expanded {dtype}", o_m, lse_m, q, ke, ve, lens, True)
    assert (lse_g - lse_m).abs().max().item() <= LSE_TOL


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
def test_cross_check_with_forward_ex(dtype):
    """MHA, causal, a 256-key cache with len = 256 and its last 64 positions as the queries: the bottom-right mask of the decode
    call is the top-left mask of rows 192..255 of the full 256-row problem."""
    from flash_helpers import kernel_configs as kc

    gen = torch.Generator().manual_seed(7)
    q_all, k, v = (torch.randn((2, 256, 1, 128), generator=gen).to(dtype).to(DEV) for _ in range(3))
    fa = _fa()
    cfg = kc.best_config(kc.DType.BF16 if dtype == torch.bfloat16 else kc.DType.FP16, 256, masked=True)
    o_full = fa.forward_ex(cfg, q_all, k, v, causal=True)
    o_full = o_full[0] if isinstance(o_full, tuple) else o_full
    lens = [256, 256]
    lens_t = torch.tensor(lens, dtype=torch.int32, device=DEV)
    q = q_all[:, 192:].contiguous()
    o, lse = fa.forward_kvcache(q, k, v, lens_t, causal=True, return_lse=True)
    _check(f"cross {dtype}", o, lse, q, k, v, lens, True)
    o32, _ = _eager(q, k, v, lens, True, torch.float32)
    o16, _ = _eager(q, k, v, lens, True, dtype)
    bound = max(O_TOL[dtype], 2.0 * (o16.float() - o32).abs().max().item())
    err_full = (o_full[:, 192:].float() - o32).abs().max().item()
    diff = (o.float() - o_full[:, 192:].float()).abs().max().item()
    print(f"cross {dtype}: forward_ex rows 192..255 vs O32 {err_full:.3e}, decode vs forward_ex {diff:.3e}, bound {bound:.3e}")
    assert err_full <= bound and diff <= 2.0 * bound


def test_refusals_on_device():
    fa = _fa()
    q, k, v, lens_t = _inputs(torch.bfloat16, [10, 10], 9, 8, 1)
    with pytest.raises(RuntimeError, match="64 packed query rows"):
        fa.forward_kvcache(q, k, v, lens_t)
    q, k, v, lens_t = _inputs(torch.bfloat16, [10, 10], 1, 8, 2, cache_len=96)
    table = torch.zeros((2, 1), dtype=torch.int32, device=DEV)
    with pytest.raises(RuntimeError, match="multiple of 64"):
        fa.forward_kvcache(q, k.reshape(2, 96, 2, 128), v, lens_t, block_table=table)


@pytest.mark.parametrize("paged", [False, True], ids=["contiguous", "paged"])
def test_graph_capture_replays_new_lengths(paged):
    """One capture, replayed after cache_seqlens changed in place: the host does not read the lengths."""
    dtype = torch.bfloat16
    lens_a, lens_b = [100, 2048, 7, 0], [1500, 3, 640, 65]
    q, k, v, lens_t = _inputs(dtype, lens_a, 2, 8, 2, cache_len=2048, seed=8)
    fa = _fa()
    kw = {}
    kc_, vc_ = k, v
    if paged:
        kc_, vc_, table = _paginate(k, v, [2048] * 4, 256, poison=False)
        kw["block_table"] = table
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        fa.forward_kvcache(q, kc_, vc_, lens_t, causal=True, return_lse=True, **kw)   # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(stream)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        o, lse = fa.forward_kvcache(q, kc_, vc_, lens_t, causal=True, return_lse=True, **kw)
    graph.replay()
    torch.cuda.synchronize()
    _check("graph first", o.clone(), lse.clone(), q, k, v, lens_a, True)
    lens_t.copy_(torch.tensor(lens_b, dtype=torch.int32))
    graph.replay()
    torch.cuda.synchronize()
    _check("graph replay", o.clone(), lse.clone(), q, k, v, lens_b, True)
