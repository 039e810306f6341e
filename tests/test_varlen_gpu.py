"""Packed variable-length sequences on the MI355X: forward_varlen / backward_varlen / attention_varlen.

Against fp32 per sequence (each sequence sliced out, eager attention on it), with the project's tolerances
(tests/test_gqa_gpu.py, tests/test_backward_gpu.py): |O - O32| <= 2^-6 (bf16) / 2^-9 (fp16), |lse - lse32| <= 1e-3, and per
gradient max|g - g32| <= 2 max|g_torch16 - g32| + 1e-4 and ||g - g32|| / ||g32|| <= 2 ||g_torch16 - g32|| / ||g32|| + 1e-3.

Against the existing kernels, bit for bit:
  - forward, MHA: O of sequence i equals forward_ex(varlen_config, q_i, k_i, v_i, causal) (allow_ragged) wherever that launch
    is served by the masked 32-row variant.  Plain launches with len % 256 == 0 go through the hand-placed ring form
    (fa_kernel_info.ring_form; lazy rescale, other rounding points): those cases -- plain, lengths 256, 512, 1024, 2048, 4096 --
    keep the fp32 rule only.
  - backward, lengths all multiples of 256, same o / lse / dout: dQ of sequence i equals backward() on it as a batch of one,
    MHA and GQA; dK / dV equal it where the two launches use the same split: always for MHA (no split); for GQA where
    bwd_varlen_split(n_seqs, max_seqlen, ...) == bwd_gqa_split(1, len_i, ...), computed in the test from the workspace sizes.
    The other cases fall under the fp32 rule."""
import ctypes
import json
import os

import pytest
import torch

import flash_attention
from flash_attention_from_scratch_amd import _capi
from flash_attention_from_scratch_amd import flash_attention_kernels as fak
from flash_attention_from_scratch_amd.tools import record_varlen_bits as rec
from tests.conftest import GOLDEN

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
DTYPES = [torch.bfloat16, torch.float16]
O_TOL = {torch.bfloat16: 2.0 ** -6, torch.float16: 2.0 ** -9}
H = 4
HEADS = [(4, 4), (8, 2), (4, 1)]
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


def _inputs(lengths, Hq, Hkv, dtype, seed=0):
    gen = torch.Generator().manual_seed(seed)
    T = sum(lengths)
    q, dout = (torch.randn((T, Hq, 128), generator=gen).to(dtype).to(DEV) for _ in range(2))
    k, v = (torch.randn((T, Hkv, 128), generator=gen).to(dtype).to(DEV) for _ in range(2))
    return q, k, v, dout


def _eager(q, k, v, causal, dtype):
    """one sequence (n, H, D) -> o (n, H, D) in `dtype`, K / V expanded to q's heads"""
    G = q.shape[1] // k.shape[1]
    k, v = k.repeat_interleave(G, dim=1), v.repeat_interleave(G, dim=1)
    s = torch.einsum("qhd,khd->hqk", q.to(dtype), k.to(dtype)) / 128 ** 0.5
    if causal:
        n = q.shape[0]
        s = s.masked_fill(torch.ones((n, n), dtype=torch.bool, device=q.device).triu(1), float("-inf"))
    return torch.einsum("hqk,khd->qhd", torch.softmax(s, dim=-1), v.to(dtype))


def _lse32(q, k, causal):
    G = q.shape[1] // k.shape[1]
    s = torch.einsum("qhd,khd->hqk", q.float(), k.repeat_interleave(G, dim=1).float()) / 128 ** 0.5
    if causal:
        n = q.shape[0]
        s = s.masked_fill(torch.ones((n, n), dtype=torch.bool, device=q.device).triu(1), float("-inf"))
    return torch.logsumexp(s, dim=-1)


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


def _hkv(div):
    return 1 if div == 0 else H // div


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("div", [1, 4, 0])   # Hkv = H, H / 4 (8 query heads, 2 K / V heads), 1 (MQA)
@pytest.mark.parametrize("name", list(LENGTH_SETS))
def test_varlen_matches_fp32_per_sequence(dtype, causal, div, name):
    lengths, max_seqlen = LENGTH_SETS[name]
    Hq = 8 if div == 4 else H   # Hkv = H / 4 = 2 with 8 query heads
    Hkv = Hq // 4 if div == 4 else _hkv(div)
    max_seqlen = max_seqlen or max(lengths)
    q, k, v, dout = _inputs(lengths, Hq, Hkv, dtype, seed=len(lengths) + Hkv)
    cu_t, cu = _cu(lengths)
    o, lse = flash_attention.forward_varlen(q, k, v, cu_t, max_seqlen, causal=causal)
    dq, dk, dv = flash_attention.backward_varlen(q, k, v, o, lse, dout, cu_t, max_seqlen, causal=causal)
    torch.cuda.synchronize()
    assert o.shape == q.shape and lse.shape == (Hq, sum(lengths)) and dk.shape == k.shape and dv.shape == v.shape
    for t in (o, lse, dq, dk, dv):
        assert torch.isfinite(t.float()).all()
    for i, n in enumerate(lengths):
        if n == 0:
            continue
        sl = slice(cu[i], cu[i + 1])
        o32 = _eager(q[sl].float(), k[sl].float(), v[sl].float(), causal, torch.float32)
        err = (o[sl].float() - o32).abs().max().item()
        assert err <= O_TOL[dtype], (i, n, err)
        lerr = (lse[:, sl] - _lse32(q[sl], k[sl], causal)).abs().max().item()
        assert lerr <= 1e-3, (i, n, lerr)
        g32 = _grads(q[sl], k[sl], v[sl], dout[sl], causal, torch.float32)
        g16 = _grads(q[sl], k[sl], v[sl], dout[sl], causal, dtype)
        for nm, g, r32, r16 in zip(("dq", "dk", "dv"), (dq[sl], dk[sl], dv[sl]), g32, g16):
            _check_grad(f"{nm}[seq {i}, len {n}]", g, r32, r16)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("name", list(LENGTH_SETS))
def test_varlen_forward_is_the_masked_32_row_kernel_bit_for_bit(dtype, causal, name):
    lengths, max_seqlen = LENGTH_SETS[name]
    max_seqlen = max_seqlen or max(lengths)
    q, k, v, _ = _inputs(lengths, H, H, dtype, seed=3)
    cu_t, cu = _cu(lengths)
    o, _ = flash_attention.forward_varlen(q, k, v, cu_t, max_seqlen, causal=causal)
    cfg = fak.varlen_config(dtype)
    ring = _capi.query(cfg).ring_form   # plain launches with seq_len % 256 == 0 take the ring form (other rounding points)
    checked = 0
    for i, n in enumerate(lengths):
        if n == 0 or (not causal and ring and n % 256 == 0):
            continue   # (fp32 rule only: test_varlen_matches_fp32_per_sequence)
        sl = slice(cu[i], cu[i + 1])
        o_d = flash_attention.forward_ex(cfg, q[sl][None].contiguous(), k[sl][None].contiguous(), v[sl][None].contiguous(), causal=causal)
        assert _same(o[sl], o_d[0]), (i, n)
        checked += 1
    torch.cuda.synchronize()
    assert checked > 0 or name == "aligned"


def _dense_split(S, Hq, Hkv, causal):
    base = _capi.FaBwdArgs(batch=1, seq_len=S, n_heads=Hq, d_head=128, qkv_batch_stride=S * Hq * 128, qkv_seq_stride=Hq * 128,
                           qkv_head_stride=128, out_batch_stride=S * Hq * 128, out_seq_stride=Hq * 128, out_head_stride=128,
                           dtype=15, causal=int(causal))
    a = _capi.FaBwdGqaArgs(base=base, n_kv_heads=Hkv, kv_batch_stride=S * Hkv * 128, kv_seq_stride=Hkv * 128, kv_head_stride=128,
                           dkv_batch_stride=S * Hkv * 128, dkv_seq_stride=Hkv * 128, dkv_head_stride=128)
    extra = _capi.load().fa_bwd_gqa_workspace_bytes(ctypes.byref(a)) - 4 * Hq * S
    return 1 if extra == 0 else extra // (4 * Hkv * S * 2 * 128)


def _varlen_split(n_seqs, T, max_seqlen, Hq, Hkv, causal):
    a = _capi.FaBwdVarlenArgs(n_heads=Hq, n_kv_heads=Hkv, d_head=128, q_seq_stride=Hq * 128, q_head_stride=128,
                              out_seq_stride=Hq * 128, out_head_stride=128, kv_seq_stride=Hkv * 128, kv_head_stride=128,
                              dkv_seq_stride=Hkv * 128, dkv_head_stride=128, dtype=15, causal=int(causal),
                              varlen=_capi.make_varlen_layout(16, n_seqs, T, max_seqlen))
    extra = _capi.load().fa_bwd_varlen_workspace_bytes(ctypes.byref(a)) - ((4 * Hq * T + 15) & ~15)
    return 1 if extra == 0 else extra // (4 * Hkv * T * 2 * 128)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("heads", [(4, 4), (8, 2), (8, 1)])
def test_varlen_backward_matches_the_dense_backward_bit_for_bit(dtype, causal, heads):
    Hq, Hkv = heads
    lengths = [256, 1024, 512]
    q, k, v, dout = _inputs(lengths, Hq, Hkv, dtype, seed=11)
    cu_t, cu = _cu(lengths)
    o, lse = flash_attention.forward_varlen(q, k, v, cu_t, 1024, causal=causal)
    dq, dk, dv = flash_attention.backward_varlen(q, k, v, o, lse, dout, cu_t, 1024, causal=causal)
    vs = _varlen_split(3, sum(lengths), 1024, Hq, Hkv, causal)
    compared_dkv = 0
    for i, n in enumerate(lengths):
        sl = slice(cu[i], cu[i + 1])
        one = [t[sl][None].contiguous() for t in (q, k, v, o, dout)]
        lse_i = lse[:, sl][None].contiguous()
        dq_d, dk_d, dv_d = flash_attention.backward(one[0], one[1], one[2], one[3], lse_i, one[4], causal=causal)
        assert _same(dq[sl], dq_d[0]), ("dq", i, n)
        if Hq == Hkv or _dense_split(n, Hq, Hkv, causal) == vs:   # MHA: always; GQA: where the splits agree
            assert _same(dk[sl], dk_d[0]) and _same(dv[sl], dv_d[0]), ("dk / dv", i, n)
            compared_dkv += 1
    torch.cuda.synchronize()
    assert Hq != Hkv or compared_dkv == len(lengths)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("causal", [False, True])
def test_varlen_isolation_between_sequences(dtype, causal):
    lengths = [300, 129, 64, 1000]
    Hq, Hkv = 8, 2
    q, k, v, dout = _inputs(lengths, Hq, Hkv, dtype, seed=5)
    cu_t, cu = _cu(lengths)

    def run(q, k, v, dout):
        o, lse = flash_attention.forward_varlen(q, k, v, cu_t, 1000, causal=causal)
        return (o, lse) + tuple(flash_attention.backward_varlen(q, k, v, o, lse, dout, cu_t, 1000, causal=causal))

    ref = run(q, k, v, dout)
    j = 1
    sl = slice(cu[j], cu[j + 1])
    gen = torch.Generator().manual_seed(99)
    changed = [t.clone() for t in (q, k, v, dout)]
    for t in changed:
        t[sl] = torch.randn(t[sl].shape, generator=gen).to(dtype).to(DEV) * 3
    got = run(*changed)
    torch.cuda.synchronize()
    keep = torch.ones(sum(lengths), dtype=torch.bool, device=DEV)
    keep[sl] = False
    for nm, a, b in zip(("o", "lse", "dq", "dk", "dv"), ref, got):
        if nm == "lse":
            assert _same(a[:, keep], b[:, keep]), nm
            assert not _same(a[:, sl], b[:, sl])
        else:
            assert _same(a[keep], b[keep]), nm


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("heads", [(4, 4), (8, 2), (4, 1)])
def test_varlen_nothing_outside_is_read_or_written(dtype, causal, heads):
    """Q, K, V, dO with 256 NaN rows in front and behind, the outputs written into buffers filled with a sentinel (through the C
    ABI, which takes the output pointers): results finite and bit-identical to the run without margins, margins untouched."""
    Hq, Hkv = heads
    lengths = [1, 63, 65, 129, 257, 1000]
    T, M = sum(lengths), 256
    q, k, v, dout = _inputs(lengths, Hq, Hkv, dtype, seed=21)
    cu_t, cu = _cu(lengths)
    o_ref, lse_ref = flash_attention.forward_varlen(q, k, v, cu_t, 1000, causal=causal)
    g_ref = flash_attention.backward_varlen(q, k, v, o_ref, lse_ref, dout, cu_t, 1000, causal=causal)

    def pad(t):
        buf = torch.full((T + 2 * M,) + tuple(t.shape[1:]), float("nan"), dtype=t.dtype, device=DEV)
        buf[M:M + T] = t
        return buf

    qp, kp, vp, dop = (pad(t) for t in (q, k, v, dout))
    SENT = 777.0
    ob, dqb = (torch.full((T + 2 * M, Hq, 128), SENT, dtype=dtype, device=DEV) for _ in range(2))
    dkb, dvb = (torch.full((T + 2 * M, Hkv, 128), SENT, dtype=dtype, device=DEV) for _ in range(2))
    lse_in = torch.full((Hq * T + 2 * M,), SENT, dtype=torch.float32, device=DEV)   # (lse is contiguous: margins around the (H, T) block)
    lib = _capi.load()
    cfg = _capi.make_config(fak.varlen_config(dtype))
    args = _capi.FaFwdArgs(q=qp[M:].data_ptr(), k=kp[M:].data_ptr(), v=vp[M:].data_ptr(), o=ob[M:].data_ptr(), batch=1, seq_len=T,
                           n_heads=Hq, d_head=128, batch_stride=0, seq_stride=Hq * 128, head_stride=128, cfg=cfg)
    kv = _capi.make_kv_layout(Hkv, 0, Hkv * 128, 128)
    vl = _capi.make_varlen_layout(cu_t.data_ptr(), len(lengths), T, 1000)
    opts = _capi.make_opts(causal=causal)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    lse_ptr = lse_in[M:].data_ptr()
    _capi.check(lib.fa_fwd_launch_varlen(ctypes.byref(args), ctypes.byref(kv), ctypes.byref(vl), ctypes.byref(opts),
                                         ctypes.c_void_p(lse_ptr), stream))
    b = _capi.FaBwdVarlenArgs(
        q=qp[M:].data_ptr(), k=kp[M:].data_ptr(), v=vp[M:].data_ptr(), o=ob[M:].data_ptr(), dout=dop[M:].data_ptr(),
        lse=ctypes.cast(ctypes.c_void_p(lse_ptr), ctypes.POINTER(ctypes.c_float)),
        dq=dqb[M:].data_ptr(), dk=dkb[M:].data_ptr(), dv=dvb[M:].data_ptr(), workspace=16, n_heads=Hq, n_kv_heads=Hkv, d_head=128,
        q_seq_stride=Hq * 128, q_head_stride=128, out_seq_stride=Hq * 128, out_head_stride=128,
        kv_seq_stride=Hkv * 128, kv_head_stride=128, dkv_seq_stride=Hkv * 128, dkv_head_stride=128,
        dtype=15 if dtype == torch.bfloat16 else 5, causal=int(causal), varlen=vl)
    ws = torch.empty(lib.fa_bwd_varlen_workspace_bytes(ctypes.byref(b)), dtype=torch.uint8, device=DEV)
    b.workspace = ws.data_ptr()
    _capi.check(lib.fa_bwd_launch_varlen(ctypes.byref(b), stream, None))
    torch.cuda.synchronize()
    lse_got = lse_in[M:M + Hq * T].view(Hq, T)
    for nm, ref, buf in (("o", o_ref, ob), ("dq", g_ref[0], dqb), ("dk", g_ref[1], dkb), ("dv", g_ref[2], dvb)):
        inner = buf[M:M + T]
        assert torch.isfinite(inner.float()).all(), nm
        assert _same(inner, ref), nm
        assert (buf[:M] == SENT).all() and (buf[M + T:] == SENT).all(), nm
    assert torch.isfinite(lse_got).all() and _same(lse_got.contiguous(), lse_ref)
    assert (lse_in[:M] == SENT).all() and (lse_in[M + Hq * T:] == SENT).all()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("causal", [False, True])
def test_varlen_is_deterministic_and_takes_packed_qkv_views(dtype, causal):
    lengths = [4096, 37, 2048, 999]
    Hq, Hkv = 8, 2
    T = sum(lengths)
    gen = torch.Generator().manual_seed(8)
    buf = torch.randn((T, Hq + 2 * Hkv, 128), generator=gen).to(dtype).to(DEV)
    q, k, v = buf[:, :Hq], buf[:, Hq:Hq + Hkv], buf[:, Hq + Hkv:]
    dout = torch.randn((T, Hq, 128), generator=gen).to(dtype).to(DEV)
    cu_t, _ = _cu(lengths)

    def run(q, k, v):
        o, lse = flash_attention.forward_varlen(q, k, v, cu_t, 4096, causal=causal)
        return (o, lse) + tuple(flash_attention.backward_varlen(q, k, v, o, lse, dout, cu_t, 4096, causal=causal))

    a, b, c = run(q, k, v), run(q, k, v), run(q.contiguous(), k.contiguous(), v.contiguous())
    torch.cuda.synchronize()
    assert k.stride(0) == (Hq + 2 * Hkv) * 128
    for x, y, z in zip(a, b, c):
        assert _same(x, y)   # run to run
        assert _same(x, z)   # views of one packed buffer against contiguous tensors


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("causal", [False, True])
def test_attention_varlen_end_to_end(dtype, causal):
    lengths = [300, 0, 1000, 17, 512]
    Hq, Hkv = 8, 2
    q, k, v, g = _inputs(lengths, Hq, Hkv, dtype, seed=13)
    cu_t, cu = _cu(lengths)
    leaves = [t.clone().requires_grad_(True) for t in (q, k, v)]
    out = flash_attention.attention_varlen(*leaves, cu_t, 1000, causal=causal)
    out.backward(g)
    ref = [t.detach().float().requires_grad_(True) for t in (q, k, v)]
    o32 = torch.cat([_eager(ref[0][cu[i]:cu[i + 1]], ref[1][cu[i]:cu[i + 1]], ref[2][cu[i]:cu[i + 1]], causal, torch.float32)
                     for i in range(len(lengths)) if lengths[i]])
    o32.backward(g.float())
    assert (out.detach().float() - o32.detach()).abs().max().item() <= O_TOL[dtype]
    for i, n in enumerate(lengths):
        if n == 0:
            continue
        sl = slice(cu[i], cu[i + 1])
        g16 = _grads(q[sl], k[sl], v[sl], g[sl], causal, dtype)
        for nm, leaf, r, r16 in zip(("dq", "dk", "dv"), leaves, ref, g16):
            _check_grad(f"{nm}[seq {i}]", leaf.grad[sl], r.grad[sl], r16)


@pytest.mark.parametrize("dtype", DTYPES)
def test_varlen_launches_replay_from_a_graph(dtype):
    lengths = [300, 1000, 17]
    q, k, v, dout = _inputs(lengths, 8, 2, dtype, seed=17)
    cu_t, _ = _cu(lengths)
    assert _capi.load().fa_init() == 0   # (the per-device setup queries the device: before the capture)
    o_e, lse_e = flash_attention.forward_varlen(q, k, v, cu_t, 1000, causal=True)
    g_e = flash_attention.backward_varlen(q, k, v, o_e, lse_e, dout, cu_t, 1000, causal=True)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        o_g, lse_g = flash_attention.forward_varlen(q, k, v, cu_t, 1000, causal=True)
        g_g = flash_attention.backward_varlen(q, k, v, o_g, lse_g, dout, cu_t, 1000, causal=True)
    for t in (o_g, lse_g) + tuple(g_g):
        t.zero_()
    graph.replay()
    torch.cuda.synchronize()
    for x, y in zip((o_e, lse_e) + tuple(g_e), (o_g, lse_g) + tuple(g_g)):
        assert _same(x, y)


@pytest.fixture(scope="module")
def recorded_bits():
    return json.load(open(os.path.join(GOLDEN, "varlen_equal_sides_bits.json")))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("heads", HEADS)
@pytest.mark.parametrize("name", list(LENGTH_SETS))
def test_varlen_reproduces_the_recorded_bits(recorded_bits, dtype, causal, heads, name):
    """tests/golden/varlen_equal_sides_bits.json: SHA-256 of o, lse, dq, dk, dv as forward_varlen / backward_varlen without the
    key side gave them before the forward with one range was folded into the forward with two (tools/record_varlen_bits.py;
    the bits of one hipcc, regenerated with profiles/r06/toolchain.json).  Both spellings of the call reproduce every hash."""
    lengths, max_seqlen = LENGTH_SETS[name]
    max_seqlen = max_seqlen or max(lengths)
    q, k, v, dout = _inputs(lengths, heads[0], heads[1], dtype, seed=recorded_bits["seed"])
    cu_t, _ = _cu(lengths)
    want = recorded_bits["cases"][rec.case_id(dtype, causal, heads, name)]
    for key_side in ({}, dict(cu_seqlens_k=cu_t.clone(), max_seqlen_k=max_seqlen)):
        o, lse = flash_attention.forward_varlen(q, k, v, cu_t, max_seqlen, causal=causal, **key_side)
        grads = flash_attention.backward_varlen(q, k, v, o, lse, dout, cu_t, max_seqlen, causal=causal, **key_side)
        torch.cuda.synchronize()
        for nm, x in zip(rec.NAMES, (o, lse) + tuple(grads)):
            assert rec.sha256_of(x) == want[nm], (nm, sorted(key_side))
