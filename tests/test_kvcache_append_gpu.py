"""The KV-cache append on the MI355X: flash_attention.append_kvcache and forward_kvcache(k=, v=, rotary_*).

The reference is tests/kvcache_append_ref.py -- eager torch on the same device -- and every comparison with it is bit for bit:
the copied rows, the rotary arithmetic (fp32, unfused, rounded once), the e4m3fn bytes, the lengths, and o / lse of the decode
behind the append against the same decode on a cache and q the reference prepared.  Only the last test block also uses a
tolerance: the existing decode rule against fp32 eager attention (tests/test_decode_gpu.py).

Shapes: batch 3, 2 K / V heads, 8 query heads; capacity 256 contiguous, or 12 shuffled pages of 64 with 4 per sequence;
1 or 3 new tokens; lengths [0, 63, 250]: an empty entry, an append across a page boundary, and one near the capacity."""
import pytest
import torch

from tests import kvcache_append_ref as ref
from tests.test_decode_gpu import DEV, DTYPES, _check

pytestmark = pytest.mark.gpu

B, HKV, H, D = 3, 2, 8, 128
CAP, PAGE, NPAGES, PER_SEQ = 256, 64, 12, 4
LENS = [0, 63, 250]
IDS = ["bf16", "fp16"]


def _fa():
    import flash_attention
    return flash_attention


def _bits(t):
    return t.view(torch.uint8 if t.element_size() == 1 else torch.int16)


def _same(a, b):
    return torch.equal(_bits(a), _bits(b))


def _table(seed=5):
    """12 pages, shuffled, 4 per sequence: no page twice"""
    gen = torch.Generator().manual_seed(seed)
    return torch.randperm(NPAGES, generator=gen).to(torch.int32).reshape(B, PER_SEQ).to(DEV)


def _sentinel_cache(dtype, paged, fp8):
    """Every element of both caches differs from its neighbours in a position-dependent way: element e of the cache holds the
    bit pattern e mod a prime (K) or another prime (V), so a row written to the wrong place, or a byte touched outside the
    written rows, changes the comparison with the reference."""
    shape = (NPAGES, PAGE, HKV, D) if paged else (B, CAP, HKV, D)
    n = shape[0] * shape[1] * shape[2] * shape[3]
    e = torch.arange(n, device=DEV, dtype=torch.int64)
    if fp8:
        k = (e % 251).to(torch.uint8).view(torch.float8_e4m3fn).reshape(shape)
        v = (e % 241).to(torch.uint8).view(torch.float8_e4m3fn).reshape(shape)
    else:
        k = (e % 32749).to(torch.int16).view(dtype).reshape(shape)
        v = (e % 32719).to(torch.int16).view(dtype).reshape(shape)
    return k, v


def _coded_rows(dtype, seqlen_new):
    """New rows that carry their (b, t, h) code: k[b, t, h, d] = +-(1 + 16 b + 4 t + h) by the parity of d, v the same + 0.5,
    negated (all exact in bf16 and fp16, and no two rows alike)"""
    b = torch.arange(B, device=DEV)[:, None, None, None]
    t = torch.arange(seqlen_new, device=DEV)[None, :, None, None]
    h = torch.arange(HKV, device=DEV)[None, None, :, None]
    d = torch.arange(D, device=DEV)[None, None, None, :]
    code = (1 + 16 * b + 4 * t + h).float() * torch.where(d % 2 == 0, 1.0, -1.0)
    return code.to(dtype).contiguous(), (-code - 0.5).to(dtype).contiguous()


def _random(dtype, seqlen_new, seqlen_q, seed):
    gen = torch.Generator(device=DEV).manual_seed(seed)
    q = torch.randn((B, seqlen_q, H, D), generator=gen, device=DEV).to(dtype)
    k = torch.randn((B, seqlen_new, HKV, D), generator=gen, device=DEV).to(dtype)
    v = torch.randn((B, seqlen_new, HKV, D), generator=gen, device=DEV).to(dtype)
    return q, k, v


def _rotary_tables(dtype, seqlen_ro, rotary_dim):
    pos = torch.arange(seqlen_ro, device=DEV, dtype=torch.float32)[:, None]
    inv = 10000.0 ** (-torch.arange(0, rotary_dim, 2, device=DEV, dtype=torch.float32) / rotary_dim)[None, :]
    return torch.cos(pos * inv).to(dtype).contiguous(), torch.sin(pos * inv).to(dtype).contiguous()


def _lens(values):
    return torch.tensor(values, dtype=torch.int32, device=DEV)


# ---- 1. copy and isolation -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("paged", [False, True], ids=["contiguous", "paged"])
@pytest.mark.parametrize("seqlen_new", [1, 3])
def test_copy_and_isolation(dtype, paged, seqlen_new):
    kc, vc = _sentinel_cache(dtype, paged, False)
    k, v = _coded_rows(dtype, seqlen_new)
    table = _table() if paged else None
    want_k, want_v, want_lens, _ = ref.append_ref(kc, vc, k, v, LENS, block_table=table)
    lens_t = _lens(LENS)
    out, q_rot = _fa().append_kvcache(kc, vc, k, v, lens_t, block_table=table)
    torch.cuda.synchronize()
    assert q_rot is None and out.dtype == torch.int32
    assert out.tolist() == want_lens == [n + seqlen_new for n in LENS]
    assert lens_t.tolist() == LENS                                       # out of place: the input lengths stay
    # the written rows equal the new rows bit for bit ...
    for b, n in enumerate(LENS):
        for t in range(seqlen_new):
            pos = n + t
            page, row = (int(table[b, pos // PAGE]), pos % PAGE) if paged else (b, pos)
            assert _same(kc[page, row], k[b, t]) and _same(vc[page, row], v[b, t]), (b, t)
    # ... and every other byte of both caches is unchanged (the reference started from the same sentinels)
    assert _same(kc, want_k) and _same(vc, want_v)
    fresh_k, fresh_v = _sentinel_cache(dtype, paged, False)
    assert int((_bits(kc) != _bits(fresh_k)).any(dim=-1).sum()) <= B * seqlen_new * HKV
    assert int((_bits(vc) != _bits(fresh_v)).any(dim=-1).sum()) <= B * seqlen_new * HKV


# ---- 2. rotary ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("interleaved", [False, True], ids=["halves", "interleaved"])
@pytest.mark.parametrize("rotary_dim", [128, 64, 16])
@pytest.mark.parametrize("causal", [False, True], ids=["plain", "causal"])
def test_rotary_bits(dtype, interleaved, rotary_dim, causal):
    """q_out and the cached K equal fp32 eager x1 c - x2 s / x1 s + x2 c rounded once.  seqlen_ro = 200 < 250: the third entry's
    keys and query rows all use the last table row (the clamp); the paged cache on rotary_dim 64."""
    paged = rotary_dim == 64
    kc, vc = _sentinel_cache(dtype, paged, False)
    q, k, v = _random(dtype, 3, 3, seed=rotary_dim + interleaved)
    cos, sin = _rotary_tables(dtype, 200, rotary_dim)
    table = _table() if paged else None
    want_k, want_v, want_lens, want_q = ref.append_ref(kc, vc, k, v, LENS, block_table=table, q=q, cos=cos, sin=sin,
                                                       interleaved=interleaved, causal=causal)
    q_before = q.clone()
    out, q_rot = _fa().append_kvcache(kc, vc, k, v, _lens(LENS), block_table=table, q=q, rotary_cos=cos, rotary_sin=sin,
                                      rotary_interleaved=interleaved, causal=causal)
    torch.cuda.synchronize()
    assert out.tolist() == want_lens
    assert _same(q, q_before) and q_rot.data_ptr() != q.data_ptr()
    assert _same(q_rot, want_q)
    assert _same(kc, want_k) and _same(vc, want_v)
    if rotary_dim < D:                                                   # beyond rotary_dim: unchanged
        assert _same(q_rot[..., rotary_dim:], q[..., rotary_dim:])
    assert not _same(q_rot[..., :rotary_dim], q[..., :rotary_dim])
    if causal:                                                           # rows of one entry at different positions ...
        assert _same(q_rot[1, 1], ref.rotary_ref(q[1, 1:2], cos, sin, [64], interleaved)[0])
    else:                                                                # ... or all at len
        assert _same(q_rot[1, 1], ref.rotary_ref(q[1, 1:2], cos, sin, [63], interleaved)[0])
    assert _same(q_rot[2, 0], ref.rotary_ref(q[2, 0:1], cos, sin, [199], interleaved)[0])   # 250 -> the last row


# ---- 3. fp8 ------------------------------------------------------------------------------------------------------------------------

DESCALES = [[0.5, 1.0], [2.0, 0.75], [0.125, 3.0]]


def _fp8_rows(dtype, seqlen_new, seed):
    """Random rows (scaled so that some values saturate) with, in every (b, t, h) row, elements 0 .. 7 set to descale times:
    two exact e4m3 ties (1.0625 -> 1.0, 1.1875 -> 1.25), three values in the subnormal range (2^-7, 3 * 2^-10: a tie, 2^-11),
    two beyond 448 (1000, -460), and 449 (rounds down to 448 without the clamp, too); one NaN in row (1, 0, 1)."""
    _, k, v = _random(dtype, seqlen_new, 1, seed)
    d = torch.tensor(DESCALES, device=DEV)[:, None, :, None]
    special = torch.tensor([1.0625, 1.1875, 2.0 ** -7, 3 * 2.0 ** -10, 2.0 ** -11, 1000.0, -460.0, 449.0], device=DEV)
    k, v = (k.float() * 3.0 * d).to(dtype), (v.float() * 200.0 * d).to(dtype)
    k[..., :8] = (special * d).to(dtype)
    v[..., 8:16] = (-special * d.flip(2)).to(dtype)                     # (V's descales are K's with the heads swapped)
    k[1, 0, 1, 20] = float("nan")
    v[1, 0, 1, 21] = float("nan")
    return k.contiguous(), v.contiguous()


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("paged", [False, True], ids=["contiguous", "paged"])
@pytest.mark.parametrize("seqlen_new", [1, 3])
def test_fp8_bytes(dtype, paged, seqlen_new):
    kc, vc = _sentinel_cache(dtype, paged, True)
    k, v = _fp8_rows(dtype, seqlen_new, seed=seqlen_new)
    kd, vd = torch.tensor(DESCALES, device=DEV), torch.tensor(DESCALES, device=DEV).flip(1).contiguous()
    table = _table() if paged else None
    want_k, want_v, want_lens, _ = ref.append_ref(kc, vc, k, v, LENS, block_table=table, k_descale=kd, v_descale=vd)
    out, _ = _fa().append_kvcache(kc, vc, k, v, _lens(LENS), block_table=table, k_descale=kd, v_descale=vd)
    torch.cuda.synchronize()
    assert out.tolist() == want_lens
    assert _same(kc, want_k) and _same(vc, want_v)                       # the reference expression's bytes, and nothing else touched
    codes = _bits(want_k)
    assert bool((codes == 0x7E).any()) and bool((codes == 0xFE).any()) and bool(((codes & 0x7F) == 0x7F).any())   # saturated, and the NaN
    # ... which are also the quantization of what the 16-bit append wrote
    k16, v16 = torch.zeros(kc.shape, dtype=dtype, device=DEV), torch.zeros(kc.shape, dtype=dtype, device=DEV)
    _fa().append_kvcache(k16, v16, k, v, _lens(LENS), block_table=table)
    for b, n in enumerate(LENS):
        for t in range(seqlen_new):
            pos = n + t
            page, row = (int(table[b, pos // PAGE]), pos % PAGE) if paged else (b, pos)
            assert _same(kc[page, row], ref.quantize_ref(k16[page, row][None], kd[b])[0]), (b, t)
            assert _same(vc[page, row], ref.quantize_ref(v16[page, row][None], vd[b])[0]), (b, t)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("interleaved", [False, True], ids=["halves", "interleaved"])
def test_fp8_with_rotary_and_without_descales(dtype, interleaved):
    """The rotated, 16-bit-rounded key is what gets quantized; absent descales mean 1 (K given, V absent)."""
    kc, vc = _sentinel_cache(dtype, True, True)
    q, k, v = _random(dtype, 3, 3, seed=9)
    cos, sin = _rotary_tables(dtype, CAP, 64)
    kd, table = torch.tensor(DESCALES, device=DEV) * 0.02, _table()
    want_k, want_v, _, want_q = ref.append_ref(kc, vc, k, v, LENS, block_table=table, q=q, cos=cos, sin=sin, interleaved=interleaved,
                                               causal=True, k_descale=kd)
    _, q_rot = _fa().append_kvcache(kc, vc, k, v, _lens(LENS), block_table=table, q=q, rotary_cos=cos, rotary_sin=sin,
                                    rotary_interleaved=interleaved, causal=True, k_descale=kd)
    torch.cuda.synchronize()
    assert _same(q_rot, want_q) and _same(kc, want_k) and _same(vc, want_v)


# ---- 4. clamps ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("fp8", [False, True], ids=["16bit", "fp8"])
def test_length_clamps(dtype, fp8):
    """len = 255 with three new tokens writes one row and returns 256; len = -5 behaves as 0; len = 10^6 writes nothing.  Finite
    checks of the clamping rule: every byte outside the legal rows is unchanged."""
    lens = [255, -5, 10 ** 6]
    kc, vc = _sentinel_cache(dtype, False, fp8)
    fresh_k, _ = _sentinel_cache(dtype, False, fp8)
    k, v = _coded_rows(dtype, 3)
    want_k, want_v, want_lens, _ = ref.append_ref(kc, vc, k, v, lens)
    out, _ = _fa().append_kvcache(kc, vc, k, v, _lens(lens))
    torch.cuda.synchronize()
    assert out.tolist() == want_lens == [256, 3, 256]
    assert _same(kc, want_k) and _same(vc, want_v)
    changed = (_bits(kc) != _bits(fresh_k)).any(dim=-1).any(dim=-1)      # (batch, row)
    assert changed[0].nonzero().flatten().tolist() in ([255], [])         # (a sentinel may equal the new row's bytes by chance: never more rows)
    assert set(changed[1].nonzero().flatten().tolist()) <= {0, 1, 2}
    assert not bool(changed[2].any())
    if not fp8:
        assert _same(kc[0, 255], k[0, 0]) and _same(kc[1, :3], k[1])


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_block_table_clamps(dtype):
    """block_table entries num_pages + 7 and -3 land in pages num_pages - 1 and 0 (decode's rule); nothing else is touched."""
    lens = [0, 10, 100]
    table = torch.tensor([[NPAGES + 7, 1, 2, 3], [-3, 4, 5, 6], [7, 8, 9, 10]], dtype=torch.int32, device=DEV)
    kc, vc = _sentinel_cache(dtype, True, False)
    fresh_k, _ = _sentinel_cache(dtype, True, False)
    k, v = _coded_rows(dtype, 3)
    want_k, want_v, want_lens, _ = ref.append_ref(kc, vc, k, v, lens, block_table=table)
    out, _ = _fa().append_kvcache(kc, vc, k, v, _lens(lens), block_table=table)
    torch.cuda.synchronize()
    assert out.tolist() == want_lens == [3, 13, 103]
    assert _same(kc, want_k) and _same(vc, want_v)
    assert _same(kc[NPAGES - 1, 0:3], k[0]) and _same(kc[0, 10:13], k[1]) and _same(kc[8, 36:39], k[2])
    changed = (_bits(kc) != _bits(fresh_k)).any(dim=-1).any(dim=-1)      # (page, row)
    assert set(changed.any(dim=1).nonzero().flatten().tolist()) <= {NPAGES - 1, 0, 8}


# ---- 5. end to end -----------------------------------------------------------------------------------------------------------------

def _value_cache(dtype, paged, fp8, seed):
    """A cache of N(0, 1) values (fp8: quantized with the descales used below) -- every row, valid or not"""
    gen = torch.Generator(device=DEV).manual_seed(seed)
    shape = (NPAGES, PAGE, HKV, D) if paged else (B, CAP, HKV, D)
    k = torch.randn(shape, generator=gen, device=DEV)
    v = torch.randn(shape, generator=gen, device=DEV)
    if fp8:
        return (k / 0.02).clamp(-448, 448).to(torch.float8_e4m3fn), (v / 0.02).clamp(-448, 448).to(torch.float8_e4m3fn)
    return k.to(dtype), v.to(dtype)


def _logical(cache, table, descale):
    """(B, CAP, HKV, D) fp32 values of a (paged, fp8) cache"""
    x = cache.float()
    if table is not None:
        x = x[table.long().flatten()].reshape(B, PER_SEQ * PAGE, HKV, D)
    return x * descale[:, None, :, None] if descale is not None else x


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("fp8", [False, True], ids=["16bit", "fp8"])
@pytest.mark.parametrize("paged", [False, True], ids=["contiguous", "paged"])
@pytest.mark.parametrize("ns", [1, 4], ids=["split1", "split4"])
def test_forward_kvcache_with_append(dtype, fp8, paged, ns):
    """forward_kvcache(k=, v=, rotary_*) against forward_kvcache on a cache and q the torch reference prepared: o and lse bit for
    bit, and both within the decode tolerance rule of fp32 eager attention over the appended cache."""
    fa = _fa()
    seqlen = 3
    kc, vc = _value_cache(dtype, paged, fp8, seed=21)
    q, k, v = _random(dtype, seqlen, seqlen, seed=22)
    cos, sin = _rotary_tables(dtype, CAP, 64)
    table = _table() if paged else None
    kd = vd = None
    if fp8:
        kd = torch.tensor(DESCALES, device=DEV) * 0.02
        vd = kd.flip(1).contiguous()
    want_k, want_v, want_lens, want_q = ref.append_ref(kc, vc, k, v, LENS, block_table=table, q=q, cos=cos, sin=sin, causal=True,
                                                       k_descale=kd, v_descale=vd)
    kw = dict(block_table=table, causal=True, return_lse=True, num_splits=ns, k_descale=kd, v_descale=vd)
    o_ref, lse_ref = fa.forward_kvcache(want_q, want_k, want_v, _lens(want_lens), **kw)
    lens_t = _lens(LENS)
    o, lse = fa.forward_kvcache(q, kc, vc, lens_t, k=k, v=v, rotary_cos=cos, rotary_sin=sin, **kw)
    torch.cuda.synchronize()
    assert lens_t.tolist() == LENS                                       # not advanced unless asked
    assert _same(kc, want_k) and _same(vc, want_v)
    assert _same(o, o_ref) and torch.equal(lse.view(torch.int32), lse_ref.view(torch.int32))
    _check(f"append e2e {dtype} fp8={fp8} paged={paged} ns={ns}", o, lse, want_q, _logical(kc, table, kd), _logical(vc, table, vd), want_lens, True)


# ---- 6. in place and under a graph -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("fp8", [False, True], ids=["16bit", "fp8"])
@pytest.mark.parametrize("paged", [False, True], ids=["contiguous", "paged"])
def test_in_place_step_under_a_graph(dtype, fp8, paged):
    """One decode step (append, rotate, quantize, advance, attend) captured once with advance_seqlens=True into static buffers
    and replayed three times with new k / v / q copied in: lengths, caches and every replay's o equal the eager loop's, which
    advances out of place (seqlens_out=None through append_kvcache, then the decode), bit for bit."""
    fa = _fa()
    steps = 3
    kc0, vc0 = _value_cache(dtype, paged, fp8, seed=31)
    table = _table() if paged else None
    cos, sin = _rotary_tables(dtype, CAP, 128)
    kd = vd = None
    if fp8:
        kd = torch.tensor(DESCALES, device=DEV) * 0.02
        vd = kd.flip(1).contiguous()
    feeds = [_random(dtype, 1, 1, seed=40 + i) for i in range(steps)]
    kw = dict(block_table=table, causal=True, k_descale=kd, v_descale=vd, max_seqlen_k=CAP)

    # the eager loop, out of place
    kc_e, vc_e, lens_e, o_e = kc0.clone(), vc0.clone(), _lens(LENS), []
    for q, k, v in feeds:
        new_lens, q_rot = fa.append_kvcache(kc_e, vc_e, k, v, lens_e, block_table=table, q=q, rotary_cos=cos, rotary_sin=sin, causal=True,
                                            k_descale=kd, v_descale=vd)
        assert new_lens.data_ptr() != lens_e.data_ptr()
        o_e.append(fa.forward_kvcache(q_rot, kc_e, vc_e, new_lens, **kw))
        lens_e = new_lens
    torch.cuda.synchronize()
    assert lens_e.tolist() == [n + steps for n in LENS]

    # the in-place step, eager: the same results
    kc_i, vc_i, lens_i = kc0.clone(), vc0.clone(), _lens(LENS)
    for i, (q, k, v) in enumerate(feeds):
        o = fa.forward_kvcache(q, kc_i, vc_i, lens_i, k=k, v=v, rotary_cos=cos, rotary_sin=sin, advance_seqlens=True, **kw)
        assert _same(o, o_e[i]), i
    torch.cuda.synchronize()
    assert lens_i.tolist() == lens_e.tolist() and _same(kc_i, kc_e) and _same(vc_i, vc_e)

    # ... and captured
    kc_g, vc_g, lens_g = kc0.clone(), vc0.clone(), _lens(LENS)
    q_s, k_s, v_s = (t.clone() for t in feeds[0])

    def step():
        return fa.forward_kvcache(q_s, kc_g, vc_g, lens_g, k=k_s, v=v_s, rotary_cos=cos, rotary_sin=sin, advance_seqlens=True, **kw)

    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        step()                                                           # warm-up outside the capture ...
    torch.cuda.current_stream().wait_stream(stream)
    kc_g.copy_(kc0), vc_g.copy_(vc0), lens_g.copy_(_lens(LENS))          # ... whose append is undone
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        o_s = step()
    kc_g.copy_(kc0), vc_g.copy_(vc0), lens_g.copy_(_lens(LENS))          # (a capture launches nothing; for symmetry)
    for i, (q, k, v) in enumerate(feeds):
        q_s.copy_(q), k_s.copy_(k), v_s.copy_(v)
        graph.replay()
        torch.cuda.synchronize()
        assert _same(o_s, o_e[i]), i
        assert lens_g.tolist() == [n + i + 1 for n in LENS]
    assert _same(kc_g, kc_e) and _same(vc_g, vc_e)
