"""Learned attention sinks in the varlen forward, backward and autograd path on the MI355X: forward_varlen_sinks,
backward_varlen_sinks, fa_bwd_launch_varlen_qk_sinks and attention_varlen_sinks on the N(0, 1) inputs of tests/sinks_inputs.py, for
which tests/test_sinks_cpu.py proves on the CPU that a kernel without the sinks misses the rules below by a factor of 4 at least,
and that zero or negated dsinks miss theirs by as much.

One packed launch holds (len_q, len_k) = (300, 300), (129, 300), (64, 1), (1, 1), (0, 5), (5, 0), (257, 130): more than one 128-row
block, 64-key tile and 128-key dK / dV block, ragged ends, rows that see no key and keys no row sees.  The reference is an fp32
eager restatement with the sink as one more column of logits (sinks_inputs.sink_attention), per sequence: the forward by bi.compare
(max|o - o32| <= max(O_TOL, 2 max|o16 - o32|), lse within LSE_TOL), the gradients by bi.grad_rule against fp32 and 16-bit eager
autograd, dsinks by bi.grad_rule on the (n_heads,) vector summed over the launch.  Each test prints its worst figures before it
asserts (DESIGN.md 9.6 quotes them)."""
import ctypes

import pytest
import torch

import flash_attention
from flash_attention_from_scratch_amd import _capi
from tests import beacon_inputs as bi
from tests import sinks_inputs as si

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
NAN16 = 0x7FC0   # a NaN in bf16 and in fp16
FAR = 1 << 30
IDS = dict(ids=str)


@pytest.fixture(autouse=True)
def _no_tf32():
    old = torch.backends.cuda.matmul.allow_tf32
    torch.backends.cuda.matmul.allow_tf32 = False
    yield
    torch.backends.cuda.matmul.allow_tf32 = old


def _same(a, b):
    view = torch.int16 if a.dtype in (torch.bfloat16, torch.float16) else torch.int32
    return a.shape == b.shape and torch.equal(a.contiguous().view(view), b.contiguous().view(view))


class _Launch:
    """One packed launch of sinks_inputs' sequences under one window and one sinks vector, on the device (the tensors are made on
    the CPU: the ones the CPU proof is about).  sinks None: SINKS_LIVE, the vector of the cached references."""

    def __init__(self, heads, dtype, window, sinks=None, seed=0, pairs=None):
        self.heads, self.dtype, self.window, self.seed = heads, dtype, window, seed
        self.causal, self.window_size = window[2], (window[0], window[1])
        self.inp = si.inputs(heads, dtype, seed) if pairs is None else si.make_inputs(heads, dtype, seed, pairs)
        self.shared = pairs is None and sinks is None   # (the cached references are these inputs')
        self.sinks_cpu = si.SINKS_LIVE(heads[0]) if sinks is None else sinks
        self.sinks = self.sinks_cpu.to(DEV)
        self.q, self.k, self.v, self.dout = (self.inp[n].to(DEV) for n in ("q", "k", "v", "dout"))
        self.cuq, self.cuk, self.pairs = self.inp["cu_q"], self.inp["cu_k"], self.inp["pairs"]
        self.cuq_t, self.cuk_t = (torch.tensor(c, dtype=torch.int32, device=DEV) for c in (self.cuq, self.cuk))
        self.mq, self.mk = max(max(p[0] for p in self.pairs), 1), max(max(p[1] for p in self.pairs), 1)

    def refs(self):
        if self.shared:
            return si.references(self.heads, self.dtype, self.window, self.seed)
        out = []
        for i in range(len(self.pairs)):
            q, k, v, dout = si.sequence(self.inp, i)
            o32, lse32, g32, dz32 = si.sink_backward(q, k, v, dout, self.sinks_cpu, self.window, torch.float32)
            o16, _, g16, dz16 = si.sink_backward(q, k, v, dout, self.sinks_cpu, self.window, self.dtype)
            out.append(dict(o32=o32, lse32=lse32, g32=g32, dz32=dz32, o16=o16, g16=g16, dz16=dz16))
        return out

    def sides(self, mq=None, mk=None, sides=True):
        return dict(cu_seqlens_k=self.cuk_t, max_seqlen_k=mk or self.mk) if sides else {}

    def forward(self, mq=None, mk=None, sides=True, sinks=None):
        return flash_attention.forward_varlen_sinks(self.q, self.k, self.v, self.cuq_t, mq or self.mq, self.sinks if sinks is None else sinks,
                                                    causal=self.causal, window_size=self.window_size, **self.sides(mq, mk, sides))

    def forward_without_sinks(self):
        return flash_attention.forward_varlen(self.q, self.k, self.v, self.cuq_t, self.mq, causal=self.causal, window_size=self.window_size,
                                              **self.sides())

    def backward(self, o, lse, mq=None, mk=None, sides=True):
        return flash_attention.backward_varlen_sinks(self.q, self.k, self.v, o, lse, self.dout, self.cuq_t, mq or self.mq, self.sinks,
                                                     self.window_size, causal=self.causal, **self.sides(mq, mk, sides))

    def abi_args(self, o, lse, outs):
        """fa_bwd_varlen_qk_args on this launch's tensors, with the caller's outputs -> (args, workspace, split)"""
        q, k = self.q, self.k
        dq, dk, dv = outs
        a = _capi.FaBwdVarlenQKArgs(
            struct_size=ctypes.sizeof(_capi.FaBwdVarlenQKArgs), q=q.data_ptr(), k=k.data_ptr(), v=self.v.data_ptr(), o=o.data_ptr(),
            dout=self.dout.data_ptr(), lse=ctypes.cast(ctypes.c_void_p(lse.data_ptr()), ctypes.POINTER(ctypes.c_float)),
            dq=dq.data_ptr(), dk=dk.data_ptr(), dv=dv.data_ptr(), workspace=16, n_heads=q.shape[1], n_kv_heads=k.shape[1], d_head=128,
            q_seq_stride=q.stride(0), q_head_stride=q.stride(1), out_seq_stride=o.stride(0), out_head_stride=o.stride(1),
            kv_seq_stride=k.stride(0), kv_head_stride=k.stride(1), dkv_seq_stride=dk.stride(0), dkv_head_stride=dk.stride(1),
            dtype=15 if self.dtype == torch.bfloat16 else 5, causal=int(self.causal),
            varlen=_capi.make_varlen_layout(self.cuq_t.data_ptr(), len(self.pairs), q.shape[0], self.mq),
            varlen_k=_capi.make_varlen_layout(self.cuk_t.data_ptr(), len(self.pairs), k.shape[0], self.mk))
        lib = _capi.load()
        nbytes = lib.fa_bwd_varlen_qk_sinks_workspace_bytes(ctypes.byref(a))
        assert nbytes >= lib.fa_bwd_varlen_qk_workspace_bytes(ctypes.byref(a)) > 0, _capi.last_error()
        sibling = lib.fa_bwd_varlen_qk_workspace_bytes(ctypes.byref(a))
        delta = (4 * q.shape[1] * q.shape[0] + 15) & ~15
        per_split = 4 * k.shape[1] * k.shape[0] * 2 * 128
        assert (sibling - delta) % per_split == 0
        split = (sibling - delta) // per_split or 1
        ws = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
        a.workspace = ws.data_ptr()
        return a, ws, split

    def nan_outputs(self):
        outs = [torch.full(t.shape, NAN16, dtype=torch.int16, device=DEV).view(self.dtype) for t in (self.q, self.k, self.k)]
        dsinks = torch.full((self.heads[0],), float("nan"), device=DEV)
        assert all(bool(torch.isnan(t).all()) for t in outs + [dsinks])
        return outs, dsinks

    def backward_abi_into_nan(self, o, lse, entry="sinks", window_size=None):
        """the C ABI call (the sinks entry, or its windowed sibling on the same o and lse) on outputs whose storage holds NaN
        -> (dq, dk, dv), dsinks, split"""
        outs, dsinks = self.nan_outputs()
        a, ws, split = self.abi_args(o, lse, outs)
        w = _capi.make_window(*(window_size or self.window_size))
        stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        lib = _capi.load()
        if entry == "sinks":
            sk = _capi.make_sinks(self.sinks.data_ptr(), self.heads[0])
            _capi.check(lib.fa_bwd_launch_varlen_qk_sinks(ctypes.byref(a), ctypes.byref(w), ctypes.byref(sk), ctypes.c_void_p(dsinks.data_ptr()),
                                                          stream, None))
        else:
            _capi.check(lib.fa_bwd_launch_varlen_qk_window(ctypes.byref(a), ctypes.byref(w), stream, None))
        torch.cuda.synchronize()
        return outs, dsinks, split

    def check_forward(self, o, lse, tag):
        """bi.compare per sequence, and o = 0, lse = z exactly on the rows that see no key -> the worst err / bound; asserts"""
        o, lse = o.cpu(), lse.cpu()
        worst, worst_lse, failures = 0.0, 0.0, []
        for i, ((n_q, n_k), r) in enumerate(zip(self.pairs, self.refs())):
            sq = slice(self.cuq[i], self.cuq[i + 1])
            res = bi.compare(o[sq], lse[:, sq], r["o32"], r["lse32"], r["o16"], self.dtype)
            worst, worst_lse = max(worst, res["err"] / res["bound"]), max(worst_lse, res["lse_err"])
            if not res["ok"]:
                failures.append((i, n_q, n_k, res))
            dead = si.dead_rows(n_q, n_k, self.window)
            assert bool((o[sq][dead] == 0).all()), (tag, i, "o of a row that sees no key")
            assert torch.equal(lse[:, sq][:, dead], self.sinks_cpu[:, None].expand(-1, int(dead.sum()))), (tag, i, "lse of a row that sees no key")
        print(f"sinks forward {tag}: worst err / bound {worst:.3f}, worst lse error {worst_lse:.2e}")
        assert not failures, failures[:4]

    def check_backward(self, grads, dsinks, tag):
        """bi.grad_rule per sequence, the exact zeros, and the dsinks rule on the launch's sum -> asserts"""
        grads = [g.cpu() for g in grads]
        ratio, failures = {"dq": 0.0, "dk": 0.0, "dv": 0.0}, []
        refs = self.refs()
        for i, ((n_q, n_k), r) in enumerate(zip(self.pairs, refs)):
            sq, sk = slice(self.cuq[i], self.cuq[i + 1]), slice(self.cuk[i], self.cuk[i + 1])
            mine = (grads[0][sq], grads[1][sk], grads[2][sk])
            for name, g, r32, r16 in zip(("dq", "dk", "dv"), mine, r["g32"], r["g16"]):
                assert g.shape == r32.shape, (tag, i, name)
                if not g.numel():   # (an empty side: nothing to compare)
                    continue
                res = bi.grad_rule(g, r32, r16)
                ratio[name] = max(ratio[name], res["ratio"])
                if not res["ok"]:
                    failures.append((i, n_q, n_k, name, res))
            assert bool((mine[0][si.dead_rows(n_q, n_k, self.window)] == 0).all()), (tag, i, "dq of a row that sees no key")
            unseen = si.unseen_keys(n_q, n_k, self.window)
            assert bool((mine[1][unseen] == 0).all()) and bool((mine[2][unseen] == 0).all()), (tag, i, "dk / dv of a key no row sees")
        res = bi.grad_rule(dsinks.cpu(), sum(r["dz32"] for r in refs), sum(r["dz16"] for r in refs))
        print(f"sinks backward {tag}: worst err / bound dq {ratio['dq']:.3f} dk {ratio['dk']:.3f} dv {ratio['dv']:.3f} dsinks {res['ratio']:.3f}")
        assert not failures, failures[:4]
        assert res["ok"], (tag, "dsinks", res)


# ---- 1: the forward against fp32 eager ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", si.DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("heads", si.HEADS, **IDS)
@pytest.mark.parametrize("window", si.WINDOWS, **IDS)
def test_forward_against_fp32_eager(dtype, heads, window):
    L = _Launch(heads, dtype, window)
    o, lse = L.forward()
    L.check_forward(o, lse, f"{dtype} heads={heads} window={window}")


# ---- 2: sinks far above, far below, and none ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", si.DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("heads", si.HEADS, **IDS)
@pytest.mark.parametrize("window", si.WINDOWS, **IDS)
def test_sinks_far_above_far_below_and_none(dtype, heads, window):
    """SINKS_EDGE: head 0's sink at +120 (lse = 120, o = 0, nothing overflows), head 1's at -120 and head 2's at -inf (both: the
    call without sinks; head 2's dead rows keep lse = -inf); no NaN anywhere, dsinks included, and dsinks[1] = dsinks[2] = 0"""
    z = si.SINKS_EDGE(heads[0])
    L = _Launch(heads, dtype, window, sinks=z)
    o, lse = L.forward()
    o0, lse0 = L.forward_without_sinks()
    grads = L.backward(o, lse)
    torch.cuda.synchronize()
    o, lse, o0, lse0 = o.cpu(), lse.cpu(), o0.cpu(), lse0.cpu()
    assert bool(torch.isfinite(o).all()) and not bool(torch.isnan(lse).any())
    dead = torch.cat([si.dead_rows(n_q, n_k, window) for n_q, n_k in L.pairs])
    assert bool(torch.isfinite(lse[[0, 1] + list(range(3, heads[0]))]).all())
    assert torch.equal(lse[2] == bi.NEG_INF, dead) and torch.equal(lse[:, dead][[0, 1]], z[[0, 1], None].expand(-1, int(dead.sum())))
    assert bool(((lse[0] - 120.0).abs() <= 1e-3).all()) and bool((o[:, 0] == 0).all())
    worst = 0.0
    for i, (n_q, n_k) in enumerate(L.pairs):
        sq = slice(L.cuq[i], L.cuq[i + 1])
        live = ~si.dead_rows(n_q, n_k, window)
        for h in (1, 2):   # (forward_varlen's values under the rule, with its fp32 lse as the reference's)
            mine, theirs = o[sq][live][:, h:h + 1], o0[sq][live][:, h:h + 1]
            res = bi.compare(mine, lse[h:h + 1, sq][:, live], theirs.float(), lse0[h:h + 1, sq][:, live], theirs, dtype)
            worst = max(worst, res["err"] / res["bound"])
            assert res["ok"], (i, h, res)
    print(f"sinks edge {dtype} heads={heads} window={window}: heads 1, 2 against forward_varlen, worst err / bound {worst:.3f}")
    for g in grads:
        assert bool(torch.isfinite(g).all())
    dsinks = grads[3].cpu()
    assert dsinks[1] == 0 and dsinks[2] == 0
    # (dq of head 0 is 0 too: P underflows beside a sink 120 above it)
    assert bool((grads[0][:, 0] == 0).all())


# ---- 3: the backward through the C ABI ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", si.DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("heads", si.HEADS, **IDS)
@pytest.mark.parametrize("window", si.WINDOWS, **IDS)
def test_backward_through_the_c_abi_into_nan(dtype, heads, window):
    """every row and key of every sequence and every head's dsinks is written, rows that see no key and keys no row sees with exact
    zeros; the wrapper gives the same bits; (4, 4) runs without a dK / dV split, (8, 2) with 4"""
    L = _Launch(heads, dtype, window)
    o, lse = L.forward()
    grads, dsinks, split = L.backward_abi_into_nan(o, lse)
    assert split == (1 if heads[0] == heads[1] else 4), split
    for g in grads + [dsinks]:
        assert not bool(torch.isnan(g).any())
    L.check_backward(grads, dsinks, f"{dtype} heads={heads} window={window} split={split}")
    for a, b in zip(grads + [dsinks], L.backward(o, lse)):
        assert _same(a, b)


# ---- 4: dQ, dK, dV are the window form's bits --------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", si.DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("heads", si.HEADS, **IDS)
@pytest.mark.parametrize("window", si.WINDOWS, **IDS)
def test_dq_dk_dv_are_the_window_forms_bits(dtype, heads, window):
    """on the same (o, lse): backward_varlen_window's, and with (-1, -1) its C ABI call with left = right = 2^30 (causal: right
    arrives as 0 either way)"""
    L = _Launch(heads, dtype, window)
    o, lse = L.forward()
    mine = L.backward(o, lse)[:3]
    if L.window_size == (-1, -1):
        want, _, _ = L.backward_abi_into_nan(o, lse, entry="window", window_size=(FAR, 0 if L.causal else FAR))
    else:
        want = flash_attention.backward_varlen_window(L.q, L.k, L.v, o, lse, L.dout, L.cuq_t, L.mq, L.window_size, causal=L.causal, **L.sides())
    torch.cuda.synchronize()
    for name, a, b in zip(("dq", "dk", "dv"), mine, want):
        assert _same(a, b), name


# ---- 5: autograd -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", si.DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("window", [(-1, -1, False), (100, -1, True), (63, 3, False)], **IDS)
@pytest.mark.parametrize("sides", [True, False], ids=["two ranges", "one range"])
def test_attention_varlen_sinks_is_forward_plus_backward(dtype, window, sides):
    pairs = None if sides else [(300, 300), (64, 64), (257, 257), (1, 1)]
    L = _Launch((8, 2), dtype, window, sinks=si.SINKS_LIVE(8), seed=5, pairs=pairs)
    leaves = [t.detach().clone().requires_grad_(True) for t in (L.q, L.k, L.v, L.sinks)]
    out = flash_attention.attention_varlen_sinks(*leaves[:3], L.cuq_t, L.mq, leaves[3], causal=L.causal, window_size=L.window_size,
                                                 **L.sides(sides=sides))
    out.backward(L.dout)
    o, lse = L.forward(sides=sides)
    grads = L.backward(o, lse, sides=sides)
    torch.cuda.synchronize()
    assert _same(out, o)
    for name, leaf, g in zip(("dq", "dk", "dv", "dsinks"), leaves, grads):
        assert leaf.grad.dtype == leaf.dtype and _same(leaf.grad, g), name
    # (and the sinks are in there: the call without them gives other bits)
    assert not _same(o, flash_attention.forward_varlen(L.q, L.k, L.v, L.cuq_t, L.mq, causal=L.causal, window_size=L.window_size,
                                                       **L.sides(sides=sides))[0])


@pytest.mark.parametrize("dtype", si.DTYPES, ids=["bf16", "fp16"])
def test_the_gradient_reaches_a_16_bit_sinks_parameter_in_its_dtype(dtype):
    L = _Launch((8, 2), dtype, (127, -1, True), sinks=si.SINKS_LIVE(8).to(dtype).float(), seed=4)
    param = L.sinks.to(dtype).requires_grad_(True)
    assert torch.equal(param.float(), L.sinks)
    leaves = [t.detach().clone().requires_grad_(True) for t in (L.q, L.k, L.v)]
    out = flash_attention.attention_varlen_sinks(*leaves, L.cuq_t, L.mq, param, causal=True, window_size=L.window_size, **L.sides())
    out.backward(L.dout)
    o, lse = L.forward()
    dsinks = L.backward(o, lse)[3]
    torch.cuda.synchronize()
    assert _same(out, o)
    assert param.grad is not None and param.grad.dtype == dtype and param.grad.shape == (8,)
    assert _same(param.grad, dsinks.to(dtype)) and bool((param.grad != 0).all())


# ---- 6: bounds and determinism -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", si.DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("window", [(-1, -1, True), (63, 3, False)], **IDS)
def test_equal_sides_give_the_one_range_call_bits(dtype, window):
    L = _Launch((8, 2), dtype, window, sinks=si.SINKS_LIVE(8), seed=2, pairs=[(300, 300), (64, 64), (257, 257), (1, 1), (130, 130)])
    assert L.cuq == L.cuk
    o, lse = L.forward()
    two = L.backward(o, lse)
    o1, lse1 = L.forward(sides=False)
    one = L.backward(o1, lse1, sides=False)
    torch.cuda.synchronize()
    for name, a, b in zip(("o", "lse", "dq", "dk", "dv", "dsinks"), (o, lse) + tuple(two), (o1, lse1) + tuple(one)):
        assert _same(a, b), name
    L.check_forward(o, lse, f"equal sides {dtype} window={window}")
    L.check_backward(two[:3], two[3], f"equal sides {dtype} window={window}")


@pytest.mark.parametrize("dtype", si.DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("window", [(-1, -1, True), (63, 3, False)], **IDS)
def test_loose_max_seqlens_give_the_tight_bits(dtype, window):
    """bounds far above every length: grids with workgroups that return at once.  (4, 4) has no dK / dV split under either bound,
    so every gradient's bits must agree (the split is a function of max_seqlen_k); dsinks knows no bound at all."""
    L = _Launch((4, 4), dtype, window, seed=1, sinks=si.SINKS_LIVE(4))
    o_t, lse_t = L.forward()
    tight = L.backward(o_t, lse_t)
    o, lse = L.forward(1024, 2048)
    loose = L.backward(o, lse, 1024, 2048)
    torch.cuda.synchronize()
    for name, a, b in zip(("o", "lse", "dq", "dk", "dv", "dsinks"), (o, lse) + tuple(loose), (o_t, lse_t) + tuple(tight)):
        assert _same(a, b), name


@pytest.mark.parametrize("heads", si.HEADS, **IDS)
def test_two_runs_give_the_same_bits(heads):
    L = _Launch(heads, torch.bfloat16, (63, 3, False), seed=6, sinks=si.SINKS_LIVE(heads[0]))
    o, lse = L.forward()
    first = L.backward(o, lse)
    o2, lse2 = L.forward()
    again = L.backward(o2, lse2)
    torch.cuda.synchronize()
    for a, b in zip((o, lse) + tuple(first), (o2, lse2) + tuple(again)):
        assert _same(a, b)


# ---- 7: graph capture --------------------------------------------------------------------------------------------------------------

def test_one_graph_of_forward_and_backward_replays_after_cu_seqlens_and_sinks_are_rewritten():
    """the launches read both offset arrays and the sinks on the device: a captured forward + backward serves other lengths of the
    same totals and other sinks"""
    dtype, window = torch.bfloat16, (100, -1, True)
    first = _Launch((8, 2), dtype, window, sinks=si.SINKS_LIVE(8), seed=7, pairs=[(300, 300), (130, 200), (257, 130)])
    second = _Launch((8, 2), dtype, window, sinks=si.SINKS_LIVE(8).flip(0) - 2.0, seed=8, pairs=[(100, 330), (330, 170), (257, 130)])
    assert first.q.shape == second.q.shape and first.k.shape == second.k.shape and first.cuq != second.cuq
    mq, mk = 512, 512
    q, k, v, dout, sinks = (t.clone() for t in (first.q, first.k, first.v, first.dout, first.sinks))
    cuq, cuk = first.cuq_t.clone(), first.cuk_t.clone()

    def step():
        o, lse = flash_attention.forward_varlen_sinks(q, k, v, cuq, mq, sinks, causal=True, cu_seqlens_k=cuk, max_seqlen_k=mk,
                                                      window_size=first.window_size)
        return (o, lse) + tuple(flash_attention.backward_varlen_sinks(q, k, v, o, lse, dout, cuq, mq, sinks, first.window_size, causal=True,
                                                                      cu_seqlens_k=cuk, max_seqlen_k=mk))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()   # (warm-up: the library and the allocator)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs = step()
    for L in (first, second, first):
        for dst, src in ((q, L.q), (k, L.k), (v, L.v), (dout, L.dout), (cuq, L.cuq_t), (cuk, L.cuk_t), (sinks, L.sinks)):
            dst.copy_(src)
        graph.replay()
        torch.cuda.synchronize()
        o, lse = L.forward(mq, mk)
        want = (o, lse) + tuple(L.backward(o, lse, mq, mk))
        torch.cuda.synchronize()
        for name, a, b in zip(("o", "lse", "dq", "dk", "dv", "dsinks"), outs, want):
            assert _same(a, b), name


# ---- 8: refusals on device tensors -------------------------------------------------------------------------------------------------

def test_refusals_on_device_tensors():
    L = _Launch((4, 4), torch.bfloat16, (5, 0, False), sinks=si.SINKS_LIVE(4), seed=9, pairs=[(64, 64)])
    o, lse = L.forward()
    good = L.sinks
    bad_sinks = [None, 1.0, good.cpu(), good.double(), good.to(torch.bfloat16), torch.zeros(5, device=DEV), torch.zeros((4, 1), device=DEV),
                 torch.zeros(8, device=DEV)[::2]]
    for bad in bad_sinks:
        with pytest.raises(RuntimeError, match="sinks must"):   # (not L.forward: its None means the launch's own sinks)
            flash_attention.forward_varlen_sinks(L.q, L.k, L.v, L.cuq_t, L.mq, bad, window_size=L.window_size)
        with pytest.raises(RuntimeError, match="sinks must"):
            flash_attention.backward_varlen_sinks(L.q, L.k, L.v, o, lse, L.dout, L.cuq_t, L.mq, bad, L.window_size)
    for bad in bad_sinks[:4] + bad_sinks[5:7]:
        with pytest.raises(RuntimeError, match="sinks must"):
            flash_attention.attention_varlen_sinks(L.q, L.k, L.v, L.cuq_t, L.mq, bad, window_size=L.window_size)
    # the sibling's refusals keep their type and text
    with pytest.raises(ValueError, match="causal means right = 0"):
        flash_attention.backward_varlen_sinks(L.q, L.k, L.v, o, lse, L.dout, L.cuq_t, L.mq, good, (5, 5), causal=True)
    with pytest.raises(ValueError, match="cu_seqlens_k and max_seqlen_k"):
        flash_attention.backward_varlen_sinks(L.q, L.k, L.v, o, lse, L.dout, L.cuq_t, L.mq, good, (5, 0), cu_seqlens_k=L.cuk_t)
    with pytest.raises(RuntimeError, match="lse must be"):
        flash_attention.backward_varlen_sinks(L.q, L.k, L.v, o, lse[:, :10], L.dout, L.cuq_t, L.mq, good, (5, 0))
    with pytest.raises(ValueError, match="cu_seqlens_k and max_seqlen_k"):
        flash_attention.forward_varlen_sinks(L.q, L.k, L.v, L.cuq_t, L.mq, good, cu_seqlens_k=L.cuk_t)
    with pytest.raises(ValueError, match="cu_seqlens_k and max_seqlen_k"):
        flash_attention.attention_varlen_sinks(L.q, L.k, L.v, L.cuq_t, L.mq, good, max_seqlen_k=64)
    # the C ABI on the same tensors: the sinks' own rules behind the window's, those behind the sibling's
    outs, dsinks = L.nan_outputs()
    a, ws, _ = L.abi_args(o, lse, outs)
    lib = _capi.load()
    w, sk, dz = _capi.make_window(5, 0), _capi.make_sinks(good.data_ptr(), 4), ctypes.c_void_p(dsinks.data_ptr())
    launch = lib.fa_bwd_launch_varlen_qk_sinks
    assert launch(ctypes.byref(a), ctypes.byref(w), None, dz, None, None) == -1 and "fa_sinks is null" in _capi.last_error()
    assert launch(ctypes.byref(a), None, ctypes.byref(sk), dz, None, None) == -1 and "fa_window is null" in _capi.last_error()
    assert launch(ctypes.byref(a), ctypes.byref(w), ctypes.byref(sk), None, None, None) == -1 and "dsinks is null" in _capi.last_error()
    wrong = _capi.make_sinks(good.data_ptr(), 8)
    assert launch(ctypes.byref(a), ctypes.byref(w), ctypes.byref(wrong), dz, None, None) == -4 and "fa_sinks.n_heads" in _capi.last_error()
    torch.cuda.synchronize()
    assert all(bool(torch.isnan(t).all()) for t in outs + [dsinks])   # (a refused call writes nothing)
