"""Packed sequences with separate Q and K / V lengths on the MI355X: forward_varlen / backward_varlen / attention_varlen with
cu_seqlens_k, max_seqlen_k.

Against fp32 per sequence (each sequence's query rows and key rows sliced out, eager attention with the bottom-right mask
tril(diagonal = n_k - n_q) on them), with the project's tolerances (tests/test_varlen_gpu.py): |O - O32| <= 2^-6 (bf16) / 2^-9
(fp16), |lse - lse32| <= 1e-3 on finite rows, and per gradient max|g - g32| <= 2 max|g_torch16 - g32| + 1e-4 and
||g - g32|| / ||g32|| <= 2 ||g_torch16 - g32|| / ||g32|| + 1e-3.  A row that sees no key: o = 0, lse = -inf, dq = 0, exactly; a
key no query sees: dk = dv = 0, exactly.

Against the existing kernels: with cu_seqlens_k = cu_seqlens every output has forward_varlen's / backward_varlen's bits; against
forward_kvcache on the same rows, the decode tests' rule (this pins the bottom-right convention to the one already shipped)."""
import ctypes

import pytest
import torch

import flash_attention
from flash_attention_from_scratch_amd import _capi
from flash_attention_from_scratch_amd import flash_attention_kernels as fak

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
DTYPES = [torch.bfloat16, torch.float16]
O_TOL = {torch.bfloat16: 2.0 ** -6, torch.float16: 2.0 ** -9}
HEADS = [(4, 4), (8, 2), (4, 1)]
NEG_INF = float("-inf")
# (len_q, len_k) per sequence, and loose bounds (max_seqlen_q, max_seqlen_k) or None for the tight ones
PAIR_SETS = {
    "prefill": ([(512, 4096), (37, 1000), (1, 777), (128, 128 + 64)], None),
    "cross": ([(1000, 300), (256, 2500), (65, 63)], None),
    "q_longer": ([(300, 100), (129, 1), (64, 64)], None),
    "empties": ([(0, 300), (200, 130), (300, 0), (0, 0), (17, 40)], None),
    "loose": ([(37, 1000), (300, 100), (128, 192)], (1024, 2048)),
}
# tests/test_varlen_gpu.py's LENGTH_SETS (equal sides)
LENGTH_SETS = {
    "aligned": ([256, 1024, 512], None),
    "edges": ([1, 63, 64, 65, 127, 129, 257, 1000], None),
    "empty": ([0, 300, 0, 17], None),
    "one_ragged": ([2500], None),
    "mixed_tight": ([4096, 37, 2048, 999], 4096),
    "mixed_loose": ([4096, 37, 2048, 999], 8192),
}


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


def _inputs(pairs, Hq, Hkv, dtype, seed=0):
    gen = torch.Generator().manual_seed(seed)
    Tq, Tk = sum(p[0] for p in pairs), sum(p[1] for p in pairs)
    q, dout = (torch.randn((Tq, Hq, 128), generator=gen).to(dtype).to(DEV) for _ in range(2))
    k, v = (torch.randn((Tk, Hkv, 128), generator=gen).to(dtype).to(DEV) for _ in range(2))
    return q, k, v, dout


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
        dead = m.all(dim=1)   # rows above the shifted diagonal: softmax of a row of -inf is NaN; they are defined as 0
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


def _grads(q, k, v, dout, causal, dtype):
    leaves = [t.detach().to(dtype).requires_grad_(True) for t in (q, k, v)]
    _eager(*leaves, causal, dtype).backward(dout.to(dtype))
    return [t.grad.float() for t in leaves]


def _bits(x):
    return x.view(torch.int16) if x.dtype in (torch.bfloat16, torch.float16) else x.view(torch.int32)


def _same(a, b):
    return torch.equal(_bits(a), _bits(b))


def _check_grad(name, g, r32, r16):
    g = g.float()
    assert torch.isfinite(g).all(), name
    bound = 2 * (r16 - r32).abs().max().item() + 1e-4
    err = (g - r32).abs().max().item()
    print(f"{name}: max err {err:.3e} bound {bound:.3e}")
    assert err <= bound, (name, err, bound)
    if r32.norm().item() > 0:
        rel = ((g - r32).norm() / r32.norm()).item()
        rel16 = ((r16 - r32).norm() / r32.norm()).item()
        print(f"{name}: rel {rel:.3e} bound {2 * rel16 + 1e-3:.3e}")
        assert rel <= 2 * rel16 + 1e-3, (name, rel, rel16)


def _bounds(pairs, loose):
    return loose or (max(p[0] for p in pairs), max(p[1] for p in pairs))


def _run(q, k, v, dout, cuq_t, cuk_t, mq, mk, causal):
    o, lse = flash_attention.forward_varlen(q, k, v, cuq_t, mq, causal=causal, cu_seqlens_k=cuk_t, max_seqlen_k=mk)
    dq, dk, dv = flash_attention.backward_varlen(q, k, v, o, lse, dout, cuq_t, mq, causal=causal, cu_seqlens_k=cuk_t, max_seqlen_k=mk)
    return o, lse, dq, dk, dv


def _check_sequences(pairs, cuq, cuk, q, k, v, dout, got, causal, dtype):
    """every sequence of a launch against the fp32 rule; the rows without keys and the unseen keys exactly"""
    o, lse, dq, dk, dv = got
    for i, (nq, nk) in enumerate(pairs):
        sq, sk = slice(cuq[i], cuq[i + 1]), slice(cuk[i], cuk[i + 1])
        if nq == 0:   # keys no query sees
            assert (dk[sk] == 0).all() and (dv[sk] == 0).all(), i
            continue
        if nk == 0:   # rows that see no key
            assert (o[sq] == 0).all() and (lse[:, sq] == NEG_INF).all() and (dq[sq] == 0).all(), i
            continue
        o32 = _eager(q[sq].float(), k[sk].float(), v[sk].float(), causal, torch.float32)
        err = (o[sq].float() - o32).abs().max().item()
        print(f"seq {i} ({nq}, {nk}): |O - O32| {err:.3e}")
        assert err <= O_TOL[dtype], (i, nq, nk, err)
        l32 = _lse32(q[sq], k[sk], causal)
        live = torch.isfinite(l32)
        assert torch.equal(torch.isfinite(lse[:, sq]), live), i
        if live.any():
            lerr = (lse[:, sq][live] - l32[live]).abs().max().item()
            assert lerr <= 1e-3, (i, nq, nk, lerr)
        dead_rows = ~live[0]   # (the same rows for every head)
        n_dead = int(dead_rows.sum())
        assert n_dead == (max(nq - nk, 0) if causal else 0)
        if n_dead:
            assert (o[sq][dead_rows] == 0).all() and (lse[:, sq][:, dead_rows] == NEG_INF).all() and (dq[sq][dead_rows] == 0).all(), i
        g32 = _grads(q[sq], k[sk], v[sk], dout[sq], causal, torch.float32)
        g16 = _grads(q[sq], k[sk], v[sk], dout[sq], causal, dtype)
        for nm, g, r32, r16 in zip(("dq", "dk", "dv"), (dq[sq], dk[sk], dv[sk]), g32, g16):
            _check_grad(f"{nm}[seq {i}, ({nq}, {nk})]", g, r32, r16)


# ---- 1. fp32 parity per sequence; 2. the rows without keys and the unseen keys ----------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("heads", HEADS)
@pytest.mark.parametrize("name", list(PAIR_SETS))
def test_varlen_qk_matches_fp32_per_sequence(dtype, causal, heads, name):
    pairs, loose = PAIR_SETS[name]
    Hq, Hkv = heads
    mq, mk = _bounds(pairs, loose)
    q, k, v, dout = _inputs(pairs, Hq, Hkv, dtype, seed=len(pairs) + Hkv)
    cuq_t, cuq = _cu([p[0] for p in pairs])
    cuk_t, cuk = _cu([p[1] for p in pairs])
    got = _run(q, k, v, dout, cuq_t, cuk_t, mq, mk, causal)
    torch.cuda.synchronize()
    o, lse, dq, dk, dv = got
    assert o.shape == q.shape and lse.shape == (Hq, q.shape[0]) and dq.shape == q.shape and dk.shape == k.shape and dv.shape == v.shape
    for t in (o, dq, dk, dv):
        assert torch.isfinite(t.float()).all()
    assert not torch.isnan(lse).any() and not (lse == float("inf")).any()
    _check_sequences(pairs, cuq, cuk, q, k, v, dout, got, causal, dtype)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("heads", HEADS)
def test_varlen_qk_rows_without_keys_and_unseen_keys_are_written_exactly(dtype, causal, heads):
    """Through the C ABI, which takes the output pointers: every output filled with NaN before the call, so that a skipped store
    shows.  o = 0, lse = -inf, dq = 0 for the rows without keys; dk = dv = 0 for the keys no query sees; all else finite."""
    Hq, Hkv = heads
    pairs = [(0, 300), (300, 0), (300, 100), (40, 200), (0, 0), (129, 1), (0, 130)]
    mq, mk = 300, 300
    q, k, v, dout = _inputs(pairs, Hq, Hkv, dtype, seed=31)
    cuq_t, cuq = _cu([p[0] for p in pairs])
    cuk_t, cuk = _cu([p[1] for p in pairs])
    Tq, Tk = q.shape[0], k.shape[0]
    o, dq = (torch.full_like(q, float("nan")) for _ in range(2))
    dk, dv = (torch.full_like(k, float("nan")) for _ in range(2))
    lse = torch.full((Hq, Tq), float("nan"), dtype=torch.float32, device=DEV)
    _launch_c(q, k, v, dout, o, lse, dq, dk, dv, cuq_t, cuk_t, len(pairs), Tq, Tk, mq, mk, Hq, Hkv, dtype, causal)
    torch.cuda.synchronize()
    for nm, t in (("o", o), ("dq", dq), ("dk", dk), ("dv", dv)):
        assert torch.isfinite(t.float()).all(), nm
    assert not torch.isnan(lse).any()
    for i, (nq, nk) in enumerate(pairs):
        sq, sk = slice(cuq[i], cuq[i + 1]), slice(cuk[i], cuk[i + 1])
        dead = nq if nk == 0 else (max(nq - nk, 0) if causal else 0)   # the first `dead` rows see no key
        assert (o[sq][:dead] == 0).all() and (dq[sq][:dead] == 0).all() and (lse[:, sq][:, :dead] == NEG_INF).all(), i
        assert torch.isfinite(lse[:, sq][:, dead:]).all(), i
        if nq == 0:
            assert (dk[sk] == 0).all() and (dv[sk] == 0).all(), i
        elif nk:
            assert (dv[sk].float().abs().amax(dim=(1, 2)) > 0).all(), i   # every key of a live sequence is seen by its last row
    _check_sequences(pairs, cuq, cuk, q, k, v, dout, (o, lse, dq, dk, dv), causal, dtype)


def _launch_c(q, k, v, dout, o, lse, dq, dk, dv, cuq_t, cuk_t, n_seqs, Tq, Tk, mq, mk, Hq, Hkv, dtype, causal):
    """forward + backward through the C ABI on the caller's buffers (contiguous (T, H, 128) views)"""
    lib = _capi.load()
    cfg = _capi.make_config(fak.varlen_config(dtype))
    args = _capi.FaFwdArgs(q=q.data_ptr(), k=k.data_ptr(), v=v.data_ptr(), o=o.data_ptr(), batch=1, seq_len=Tq, n_heads=Hq,
                           d_head=128, batch_stride=0, seq_stride=Hq * 128, head_stride=128, cfg=cfg)
    kv = _capi.make_kv_layout(Hkv, 0, Hkv * 128, 128)
    vq = _capi.make_varlen_layout(cuq_t.data_ptr(), n_seqs, Tq, mq)
    vk = _capi.make_varlen_layout(cuk_t.data_ptr(), n_seqs, Tk, mk)
    opts = _capi.make_opts(causal=causal)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    _capi.check(lib.fa_fwd_launch_varlen_qk(ctypes.byref(args), ctypes.byref(kv), ctypes.byref(vq), ctypes.byref(vk), ctypes.byref(opts),
                                            ctypes.c_void_p(lse.data_ptr()), stream))
    b = _capi.FaBwdVarlenQKArgs(
        struct_size=ctypes.sizeof(_capi.FaBwdVarlenQKArgs),
        q=q.data_ptr(), k=k.data_ptr(), v=v.data_ptr(), o=o.data_ptr(), dout=dout.data_ptr(),
        lse=ctypes.cast(ctypes.c_void_p(lse.data_ptr()), ctypes.POINTER(ctypes.c_float)),
        dq=dq.data_ptr(), dk=dk.data_ptr(), dv=dv.data_ptr(), workspace=16, n_heads=Hq, n_kv_heads=Hkv, d_head=128,
        q_seq_stride=Hq * 128, q_head_stride=128, out_seq_stride=Hq * 128, out_head_stride=128,
        kv_seq_stride=Hkv * 128, kv_head_stride=128, dkv_seq_stride=Hkv * 128, dkv_head_stride=128,
        dtype=15 if dtype == torch.bfloat16 else 5, causal=int(causal), varlen=vq, varlen_k=vk)
    ws = torch.empty(max(lib.fa_bwd_varlen_qk_workspace_bytes(ctypes.byref(b)), 16), dtype=torch.uint8, device=DEV)
    b.workspace = ws.data_ptr()
    _capi.check(lib.fa_bwd_launch_varlen_qk(ctypes.byref(b), stream, None))
    return ws


# ---- 3. equal sides are the existing path, bit for bit --------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("heads", HEADS)
@pytest.mark.parametrize("name", list(LENGTH_SETS))
def test_varlen_qk_with_equal_sides_is_the_varlen_path_bit_for_bit(dtype, causal, heads, name):
    lengths, max_seqlen = LENGTH_SETS[name]
    Hq, Hkv = heads
    max_seqlen = max_seqlen or max(lengths)
    q, k, v, dout = _inputs([(n, n) for n in lengths], Hq, Hkv, dtype, seed=3)
    cu_t, _ = _cu(lengths)
    cuk_t = cu_t.clone()
    o_e, lse_e = flash_attention.forward_varlen(q, k, v, cu_t, max_seqlen, causal=causal)
    g_e = flash_attention.backward_varlen(q, k, v, o_e, lse_e, dout, cu_t, max_seqlen, causal=causal)
    got = _run(q, k, v, dout, cu_t, cuk_t, max_seqlen, max_seqlen, causal)
    torch.cuda.synchronize()
    for nm, a, b in zip(("o", "lse", "dq", "dk", "dv"), (o_e, lse_e) + tuple(g_e), got):
        assert _same(a, b), nm


# ---- 4. the decode kernel's convention ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("shape", [(1, 4, 4), (4, 8, 2), (16, 4, 1), (3, 4, 4), (8, 8, 1)])   # (seqlen_q, Hq, Hkv): seqlen_q * G <= 64
def test_varlen_qk_agrees_with_forward_kvcache(dtype, causal, shape):
    Sq, Hq, Hkv = shape
    assert Sq * (Hq // Hkv) <= 64
    lens = [777, 1, 0, 2048, 5, 300, Sq, max(Sq - 1, 0)]   # cache_seqlens, the new tokens included; some shorter than seqlen_q
    B, cap = len(lens), 2048
    gen = torch.Generator().manual_seed(41)
    q = torch.randn((B, Sq, Hq, 128), generator=gen).to(dtype).to(DEV)
    kc_, vc_ = (torch.randn((B, cap, Hkv, 128), generator=gen).to(dtype).to(DEV) for _ in range(2))
    lens_t = torch.tensor(lens, dtype=torch.int32, device=DEV)
    o_d, lse_d = flash_attention.forward_kvcache(q, kc_, vc_, lens_t, causal=causal, return_lse=True)
    # the same rows packed: Q (B * Sq, Hq, 128), every sequence Sq rows; K / V the valid prefix of each cache row, packed
    cuq_t, cuq = _cu([Sq] * B)
    cuk_t, cuk = _cu(lens)
    kp = torch.cat([kc_[b, :lens[b]] for b in range(B)])
    vp = torch.cat([vc_[b, :lens[b]] for b in range(B)])
    o, lse = flash_attention.forward_varlen(q.reshape(B * Sq, Hq, 128), kp, vp, cuq_t, Sq, causal=causal, cu_seqlens_k=cuk_t, max_seqlen_k=cap)
    torch.cuda.synchronize()
    o, lse = o.view(B, Sq, Hq, 128), lse.view(Hq, B, Sq)
    assert lse_d.shape == (B, Hq, Sq)
    lse_d = lse_d.permute(1, 0, 2)
    # -inf rows match exactly, and are the rows the bottom-right rule names
    assert torch.equal(lse == NEG_INF, lse_d == NEG_INF)
    for b in range(B):
        dead = Sq if lens[b] == 0 else (max(Sq - lens[b], 0) if causal else 0)
        assert (lse[:, b, :dead] == NEG_INF).all() and torch.isfinite(lse[:, b, dead:]).all(), b
        assert (o[b, :dead] == 0).all() and (o_d[b, :dead] == 0).all(), b
    live = lse != NEG_INF
    assert (lse[live] - lse_d[live]).abs().max().item() <= 1e-3
    for b in range(B):
        if lens[b] == 0:
            continue
        qb, kb, vb = q[b], kc_[b, :lens[b]], vc_[b, :lens[b]]
        o32 = _eager(qb.float(), kb.float(), vb.float(), causal, torch.float32)
        o16 = _eager(qb, kb, vb, causal, dtype).float()
        tol = max(O_TOL[dtype], 2 * (o16 - o32).abs().max().item())
        err = (o[b].float() - o_d[b].float()).abs().max().item()
        print(f"batch {b} (len {lens[b]}): |O_varlen_qk - O_decode| {err:.3e} tol {tol:.3e}")
        assert err <= tol, (b, lens[b], err, tol)


# ---- 5. isolation and bounds ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("heads", HEADS)
def test_varlen_qk_nothing_outside_is_read_or_written(dtype, causal, heads):
    """Between the live sequences lie neighbours whose rows are all NaN -- query rows without keys on one side, key rows without
    queries on the other -- and 256 NaN rows surround all inputs; the outputs are written, through the C ABI, into buffers
    filled with a sentinel.  The live sequences' results are finite and bit-identical to the run of the same layout on clean
    tensors; the NaN neighbours get their exact zeros and -inf; the margins stay untouched."""
    Hq, Hkv = heads
    live = [(37, 1000), (300, 100), (1, 65), (129, 257), (64, 70)]
    pairs, is_live = [], []
    for a, b in live:   # ... each followed by a (19, 0) and a (0, 45) neighbour
        pairs += [(a, b), (19, 0), (0, 45)]
        is_live += [True, False, False]
    M, mq, mk = 256, 300, 1000
    q0, k0, v0, do0 = _inputs(pairs, Hq, Hkv, dtype, seed=21)
    cuq_t, cuq = _cu([p[0] for p in pairs])
    cuk_t, cuk = _cu([p[1] for p in pairs])
    Tq, Tk = q0.shape[0], k0.shape[0]
    ref = _run(q0, k0, v0, do0, cuq_t, cuk_t, mq, mk, causal)   # clean tensors, the same layout (the same dK / dV split)
    nan = float("nan")

    def padded(src, cu):
        buf = torch.full((src.shape[0] + 2 * M,) + tuple(src.shape[1:]), nan, dtype=dtype, device=DEV)
        for j, alive in enumerate(is_live):
            if alive:
                buf[M + cu[j]:M + cu[j + 1]] = src[cu[j]:cu[j + 1]]
        return buf

    qp, dop, kp, vp = padded(q0, cuq), padded(do0, cuq), padded(k0, cuk), padded(v0, cuk)
    SENT = 777.0
    ob, dqb = (torch.full((Tq + 2 * M, Hq, 128), SENT, dtype=dtype, device=DEV) for _ in range(2))
    dkb, dvb = (torch.full((Tk + 2 * M, Hkv, 128), SENT, dtype=dtype, device=DEV) for _ in range(2))
    lse_in = torch.full((Hq * Tq + 2 * M,), SENT, dtype=torch.float32, device=DEV)   # (lse is contiguous: margins around the (H, T) block)
    lse_v = lse_in[M:M + Hq * Tq].view(Hq, Tq)
    _launch_c(qp[M:], kp[M:], vp[M:], dop[M:], ob[M:], lse_v, dqb[M:], dkb[M:], dvb[M:], cuq_t, cuk_t, len(pairs), Tq, Tk, mq, mk,
              Hq, Hkv, dtype, causal)
    torch.cuda.synchronize()
    for nm, buf in (("o", ob), ("dq", dqb), ("dk", dkb), ("dv", dvb)):
        assert (buf[:M] == SENT).all() and (buf[-M:] == SENT).all(), nm
        assert torch.isfinite(buf[M:-M].float()).all(), nm
    assert (lse_in[:M] == SENT).all() and (lse_in[M + Hq * Tq:] == SENT).all()
    for j, alive in enumerate(is_live):
        rq, rk = slice(cuq[j], cuq[j + 1]), slice(cuk[j], cuk[j + 1])
        sq, sk = slice(M + cuq[j], M + cuq[j + 1]), slice(M + cuk[j], M + cuk[j + 1])
        if not alive:   # NaN rows: queries without keys (o = 0, lse = -inf, dq = 0) or keys without queries (dk = dv = 0)
            assert (ob[sq] == 0).all() and (dqb[sq] == 0).all() and (dkb[sk] == 0).all() and (dvb[sk] == 0).all(), j
            assert (lse_v[:, rq] == NEG_INF).all(), j
            continue
        for nm, got, want in (("o", ob[sq], ref[0][rq]), ("dq", dqb[sq], ref[2][rq]), ("dk", dkb[sk], ref[3][rk]), ("dv", dvb[sk], ref[4][rk])):
            assert _same(got, want), (nm, j)
        assert _same(lse_v[:, rq].contiguous(), ref[1][:, rq].contiguous()), j


GARBAGE = {
    "negative": ([-5, 100, -7, 400], [0, -300, 200, 700]),
    "decreasing": ([0, 300, 100, 400], [700, 500, 200, 0]),
    "beyond_total": ([0, 100, 5000, 1 << 30], [0, 9000, 9100, 1 << 30]),
    "int_extremes": ([-(1 << 31), (1 << 31) - 1, -(1 << 31), (1 << 31) - 1], [(1 << 31) - 1, -(1 << 31), (1 << 31) - 1, 0]),
}


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("name", list(GARBAGE))
def test_varlen_qk_garbage_offsets_stay_inside_the_tensors(dtype, causal, name):
    """cu_seqlens_* that violate their contract: the clamping rule keeps every derived row inside the tensors (first row in
    [0, total], length in [0, min(max, rest)]), so the sentinel margins stay untouched and the launches complete.  Results for a
    violated contract are unspecified; rows that the clamped ranges do not cover are not written."""
    Hq, Hkv, Tq, Tk, M = 8, 2, 400, 700, 256
    cq, ck = GARBAGE[name]
    gen = torch.Generator().manual_seed(61)
    mk = lambda T, Hh: torch.randn((T + 2 * M, Hh, 128), generator=gen).to(dtype).to(DEV)   # noqa: E731
    qp, dop, kp, vp = mk(Tq, Hq), mk(Tq, Hq), mk(Tk, Hkv), mk(Tk, Hkv)
    SENT = 777.0
    ob, dqb = (torch.full((Tq + 2 * M, Hq, 128), SENT, dtype=dtype, device=DEV) for _ in range(2))
    dkb, dvb = (torch.full((Tk + 2 * M, Hkv, 128), SENT, dtype=dtype, device=DEV) for _ in range(2))
    lse_in = torch.full((Hq * Tq + 2 * M,), SENT, dtype=torch.float32, device=DEV)
    lse_v = lse_in[M:M + Hq * Tq].view(Hq, Tq)
    cuq_t = torch.tensor(cq, dtype=torch.int64).to(torch.int32).to(DEV)
    cuk_t = torch.tensor(ck, dtype=torch.int64).to(torch.int32).to(DEV)
    _launch_c(qp[M:], kp[M:], vp[M:], dop[M:], ob[M:], lse_v, dqb[M:], dkb[M:], dvb[M:], cuq_t, cuk_t, 3, Tq, Tk, 256, 512,
              Hq, Hkv, dtype, causal)
    torch.cuda.synchronize()
    for nm, buf in (("o", ob), ("dq", dqb), ("dk", dkb), ("dv", dvb)):
        assert (buf[:M] == SENT).all() and (buf[-M:] == SENT).all(), nm
        assert not torch.isnan(buf.float()).any(), nm   # finite inputs, clamped ranges: nothing undefined is formed
    assert (lse_in[:M] == SENT).all() and (lse_in[M + Hq * Tq:] == SENT).all()
    assert not torch.isnan(lse_in).any()


# ---- 6. determinism and packed views ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("causal", [False, True])
def test_varlen_qk_is_deterministic_and_takes_packed_views(dtype, causal):
    pairs = [(512, 4096), (37, 1000), (300, 100), (999, 2048)]
    Hq, Hkv = 8, 2
    Tq, Tk = sum(p[0] for p in pairs), sum(p[1] for p in pairs)
    gen = torch.Generator().manual_seed(8)
    qkv = torch.randn((Tq, 3, Hq, 128), generator=gen).to(dtype).to(DEV)   # a packed (total, 3, H, 128) buffer: Q is a view of it
    kvbuf = torch.randn((Tk, 2 * Hkv, 128), generator=gen).to(dtype).to(DEV)   # K, V from another tensor, one stride set
    q, k, v = qkv[:, 0], kvbuf[:, :Hkv], kvbuf[:, Hkv:]
    dout = torch.randn((Tq, Hq, 128), generator=gen).to(dtype).to(DEV)
    cuq_t, _ = _cu([p[0] for p in pairs])
    cuk_t, _ = _cu([p[1] for p in pairs])
    a = _run(q, k, v, dout, cuq_t, cuk_t, 999, 4096, causal)
    b = _run(q, k, v, dout, cuq_t, cuk_t, 999, 4096, causal)
    c = _run(q.contiguous(), k.contiguous(), v.contiguous(), dout, cuq_t, cuk_t, 999, 4096, causal)
    torch.cuda.synchronize()
    assert q.stride(0) == 3 * Hq * 128 and k.stride(0) == 2 * Hkv * 128
    for x, y, z in zip(a, b, c):
        assert _same(x, y)   # run to run
        assert _same(x, z)   # views against contiguous tensors


# ---- 7. autograd -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("causal", [False, True])
def test_attention_varlen_with_key_lengths_end_to_end(dtype, causal):
    pairs = [(300, 1000), (0, 50), (1000, 300), (17, 17), (64, 0), (512, 700)]
    Hq, Hkv = 8, 2
    q, k, v, g = _inputs(pairs, Hq, Hkv, dtype, seed=13)
    cuq_t, cuq = _cu([p[0] for p in pairs])
    cuk_t, cuk = _cu([p[1] for p in pairs])
    leaves = [t.clone().requires_grad_(True) for t in (q, k, v)]
    out = flash_attention.attention_varlen(*leaves, cuq_t, 1000, causal=causal, cu_seqlens_k=cuk_t, max_seqlen_k=1000)
    out.backward(g)
    torch.cuda.synchronize()
    assert out.shape == q.shape and leaves[1].grad.shape == k.shape and leaves[2].grad.shape == v.shape
    lse = torch.empty((Hq, q.shape[0]), dtype=torch.float32, device=DEV)
    for i, (nq, nk) in enumerate(pairs):   # (lse is not returned by attention_varlen: the fp32 rule's own, for _check_sequences)
        sq, sk = slice(cuq[i], cuq[i + 1]), slice(cuk[i], cuk[i + 1])
        lse[:, sq] = _lse32(q[sq], k[sk], causal) if nq and nk else NEG_INF
    got = (out.detach(), lse, leaves[0].grad, leaves[1].grad, leaves[2].grad)
    _check_sequences(pairs, cuq, cuk, q, k, v, g, got, causal, dtype)


# ---- 8. graph capture -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES)
def test_varlen_qk_launches_replay_from_a_graph_with_rewritten_offsets(dtype):
    Hq, Hkv, Tq, Tk = 8, 2, 1400, 3000
    gen = torch.Generator().manual_seed(17)
    q, dout = (torch.randn((Tq, Hq, 128), generator=gen).to(dtype).to(DEV) for _ in range(2))
    k, v = (torch.randn((Tk, Hkv, 128), generator=gen).to(dtype).to(DEV) for _ in range(2))
    layouts = [   # (lengths_q, lengths_k): the same totals and bounds, other sequences
        ([300, 1000, 100], [2000, 300, 700]),
        ([1000, 0, 400], [100, 1900, 1000]),
        ([17, 383, 1000], [0, 1000, 2000]),
    ]
    mq, mk = 1000, 2000
    assert _capi.load().fa_init() == 0   # (the per-device setup queries the device: before the capture)
    cuq_t, cuk_t = _cu(layouts[0][0])[0], _cu(layouts[0][1])[0]
    _run(q, k, v, dout, cuq_t, cuk_t, mq, mk, True)   # (warm up outside the capture)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        got = _run(q, k, v, dout, cuq_t, cuk_t, mq, mk, True)
    for lq, lk in layouts:
        cuq_t.copy_(_cu(lq)[0])
        cuk_t.copy_(_cu(lk)[0])
        for t in got:
            t.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        want = _run(q, k, v, dout, _cu(lq)[0], _cu(lk)[0], mq, mk, True)
        torch.cuda.synchronize()
        for nm, x, y in zip(("o", "lse", "dq", "dk", "dv"), want, got):
            assert _same(x, y), (nm, lq, lk)
