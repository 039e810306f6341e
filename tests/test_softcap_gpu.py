"""Logit soft-capping in the varlen forward, backward and autograd path on the MI355X: forward_varlen(softcap=),
backward_varlen_softcap, fa_bwd_launch_varlen_qk_softcap and attention_varlen(softcap=) on the N(0, 1) inputs of
tests/softcap_inputs.py, for which tests/test_softcap_cpu.py proves on the CPU that a kernel without the cap, or with the cap but
without the factor 1 - tanh^2 in dS, misses the rules below by a factor of 4 at least.

One packed launch holds (len_q, len_k) = (300, 300), (129, 300), (64, 1), (1, 1), (0, 5), (5, 0), (257, 130): more than one 128-row
block, 64-key tile and 128-key dK / dV block, ragged ends, rows that see no key and keys no row sees.  The reference is an fp32
eager restatement with the cap before the mask (softcap_inputs.capped_attention), per sequence: the forward by bi.compare
(max|o - o32| <= max(O_TOL, 2 max|o16 - o32|), lse within LSE_TOL, -inf rows exact), the gradients by bi.grad_rule against fp32
and 16-bit eager autograd.  Each test prints its worst figures before it asserts (DESIGN.md 9.5 quotes them)."""
import ctypes

import pytest
import torch

import flash_attention
from flash_attention_from_scratch_amd import _capi
from tests import beacon_inputs as bi
from tests import softcap_inputs as sc

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
NAN16 = 0x7FC0   # a NaN in bf16 and in fp16
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
    """One packed launch of softcap_inputs' sequences under one window and one cap, on the device (the tensors are made on the
    CPU: the ones the CPU proof is about)."""

    def __init__(self, heads, dtype, window, softcap, seed=0, pairs=None):
        self.heads, self.dtype, self.window, self.softcap, self.seed = heads, dtype, window, softcap, seed
        self.causal, self.window_size = window[2], (window[0], window[1])
        self.inp = sc.inputs(heads, dtype, seed) if pairs is None else sc.make_inputs(heads, dtype, seed, pairs)
        self.shared = pairs is None   # (the cached references are these inputs')
        self.q, self.k, self.v, self.dout = (self.inp[n].to(DEV) for n in ("q", "k", "v", "dout"))
        self.cuq, self.cuk, self.pairs = self.inp["cu_q"], self.inp["cu_k"], self.inp["pairs"]
        self.cuq_t, self.cuk_t = (torch.tensor(c, dtype=torch.int32, device=DEV) for c in (self.cuq, self.cuk))
        self.mq, self.mk = max(max(p[0] for p in self.pairs), 1), max(max(p[1] for p in self.pairs), 1)

    def refs(self):
        if self.shared:
            return sc.references(self.heads, self.dtype, self.window, self.softcap, self.seed)
        out = []
        for i in range(len(self.pairs)):
            q, k, v, dout = sc.sequence(self.inp, i)
            o32, lse32, g32 = sc.capped_backward(q, k, v, dout, self.window, torch.float32, self.softcap)
            o16, _, g16 = sc.capped_backward(q, k, v, dout, self.window, self.dtype, self.softcap)
            out.append(dict(o32=o32, lse32=lse32, g32=g32, o16=o16, g16=g16))
        return out

    def forward(self, mq=None, mk=None, sides=True, **kw):
        if sides:
            kw.update(cu_seqlens_k=self.cuk_t, max_seqlen_k=mk or self.mk)
        kw.setdefault("softcap", self.softcap)
        return flash_attention.forward_varlen(self.q, self.k, self.v, self.cuq_t, mq or self.mq, causal=self.causal,
                                              window_size=self.window_size, **kw)

    def backward(self, o, lse, mq=None, mk=None, sides=True, **cap):
        kw = dict(cu_seqlens_k=self.cuk_t, max_seqlen_k=mk or self.mk) if sides else {}
        return flash_attention.backward_varlen_softcap(self.q, self.k, self.v, o, lse, self.dout, self.cuq_t, mq or self.mq,
                                                       cap.get("softcap", self.softcap), self.window_size, causal=self.causal, **kw)

    def abi_args(self, o, lse, outs, mq=None, mk=None):
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
            varlen=_capi.make_varlen_layout(self.cuq_t.data_ptr(), len(self.pairs), q.shape[0], mq or self.mq),
            varlen_k=_capi.make_varlen_layout(self.cuk_t.data_ptr(), len(self.pairs), k.shape[0], mk or self.mk))
        nbytes = _capi.load().fa_bwd_varlen_qk_workspace_bytes(ctypes.byref(a))
        assert nbytes > 0, _capi.last_error()
        delta = (4 * q.shape[1] * q.shape[0] + 15) & ~15
        per_split = 4 * k.shape[1] * k.shape[0] * 2 * 128
        assert (nbytes - delta) % per_split == 0
        split = (nbytes - delta) // per_split or 1
        ws = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
        a.workspace = ws.data_ptr()
        return a, ws, split

    def backward_abi_into_nan(self, o, lse):
        """the C ABI call on outputs whose storage holds NaN -> (dq, dk, dv), split"""
        outs = [torch.full(t.shape, NAN16, dtype=torch.int16, device=DEV).view(self.dtype) for t in (self.q, self.k, self.k)]
        assert all(bool(torch.isnan(t).all()) for t in outs)
        a, ws, split = self.abi_args(o, lse, outs)
        w, cap = _capi.make_window(*self.window_size), _capi.make_softcap(self.softcap)
        stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        _capi.check(_capi.load().fa_bwd_launch_varlen_qk_softcap(ctypes.byref(a), ctypes.byref(w), ctypes.byref(cap), stream, None))
        torch.cuda.synchronize()
        return outs, split

    def check_forward(self, o, lse, tag):
        """bi.compare per sequence, and o = 0 on the rows that see no key -> the worst err / bound; asserts"""
        o, lse = o.cpu(), lse.cpu()
        worst, worst_lse, failures = 0.0, 0.0, []
        for i, ((n_q, n_k), r) in enumerate(zip(self.pairs, self.refs())):
            sq = slice(self.cuq[i], self.cuq[i + 1])
            res = bi.compare(o[sq], lse[:, sq], r["o32"], r["lse32"], r["o16"], self.dtype)
            worst, worst_lse = max(worst, res["err"] / res["bound"]), max(worst_lse, res["lse_err"])
            if not res["ok"]:
                failures.append((i, n_q, n_k, res))
            dead = sc.dead_rows(n_q, n_k, self.window)
            assert bool((o[sq][dead] == 0).all()), (tag, i, "o of a row that sees no key")
            assert bool((lse[:, sq][:, dead] == bi.NEG_INF).all()), (tag, i, "lse of a row that sees no key")
        print(f"softcap forward {tag}: worst err / bound {worst:.3f}, worst lse error {worst_lse:.2e}")
        assert not failures, failures[:4]

    def check_backward(self, grads, tag):
        """bi.grad_rule per sequence, and the exact zeros -> the worst err / bound per gradient; asserts"""
        grads = [g.cpu() for g in grads]
        ratio, failures = {"dq": 0.0, "dk": 0.0, "dv": 0.0}, []
        for i, ((n_q, n_k), r) in enumerate(zip(self.pairs, self.refs())):
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
            assert bool((mine[0][sc.dead_rows(n_q, n_k, self.window)] == 0).all()), (tag, i, "dq of a row that sees no key")
            unseen = sc.unseen_keys(n_q, n_k, self.window)
            assert bool((mine[1][unseen] == 0).all()) and bool((mine[2][unseen] == 0).all()), (tag, i, "dk / dv of a key no row sees")
        print(f"softcap backward {tag}: worst err / bound dq {ratio['dq']:.3f} dk {ratio['dk']:.3f} dv {ratio['dv']:.3f}")
        assert not failures, failures[:4]


# ---- 1, 2: the forward against fp32 eager ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", sc.DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("heads", sc.HEADS, **IDS)
@pytest.mark.parametrize("window", sc.WINDOWS, **IDS)
@pytest.mark.parametrize("softcap", sc.CAPS + [sc.LINEAR_CAP], **IDS)
def test_forward_against_fp32_eager(dtype, heads, window, softcap):
    """softcap 0.5 and 4.0 discriminate (a kernel without the cap misses this rule by a factor of 4 at least: the CPU proof);
    50.0 is nearly linear on these inputs and checks the tanh near 0"""
    L = _Launch(heads, dtype, window, softcap)
    o, lse = L.forward()
    L.check_forward(o, lse, f"{dtype} heads={heads} window={window} softcap={softcap}")


# ---- 3: the backward through the C ABI ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", sc.DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("heads", sc.HEADS, **IDS)
@pytest.mark.parametrize("window", sc.WINDOWS, **IDS)
@pytest.mark.parametrize("softcap", sc.CAPS, **IDS)
def test_backward_through_the_c_abi_into_nan(dtype, heads, window, softcap):
    """every row and key of every sequence is written, rows that see no key and keys no row sees with exact zeros; the wrapper gives
    the same bits; (4, 4) runs without a dK / dV split, (8, 2) with one"""
    L = _Launch(heads, dtype, window, softcap)
    o, lse = L.forward()
    grads, split = L.backward_abi_into_nan(o, lse)
    assert (split == 1) if heads[0] == heads[1] else (split > 1), split
    for g in grads:
        assert not bool(torch.isnan(g).any())
    L.check_backward(grads, f"{dtype} heads={heads} window={window} softcap={softcap} split={split}")
    for a, b in zip(grads, L.backward(o, lse)):
        assert _same(a, b)


# ---- 4: autograd -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", sc.DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("window", [(-1, -1, False), (100, -1, True), (63, 3, False)], **IDS)
@pytest.mark.parametrize("sides", [True, False], ids=["two ranges", "one range"])
def test_attention_varlen_carries_the_cap_to_both_passes(dtype, window, sides):
    pairs = None if sides else [(300, 300), (64, 64), (257, 257), (1, 1)]
    L = _Launch((8, 2), dtype, window, 4.0, seed=5, pairs=pairs)
    kw = dict(cu_seqlens_k=L.cuk_t, max_seqlen_k=L.mk) if sides else {}
    leaves = [t.detach().clone().requires_grad_(True) for t in (L.q, L.k, L.v)]
    out = flash_attention.attention_varlen(*leaves, L.cuq_t, L.mq, causal=L.causal, window_size=L.window_size, softcap=4.0, **kw)
    out.backward(L.dout)
    o, lse = L.forward(sides=sides)
    grads = L.backward(o, lse, sides=sides)
    torch.cuda.synchronize()
    assert _same(out, o)
    for name, leaf, g in zip(("dq", "dk", "dv"), leaves, grads):
        assert _same(leaf.grad, g), name
    # (and the cap is in there: the uncapped call gives other bits)
    assert not _same(o, L.forward(sides=sides, softcap=0.0)[0])


# ---- 5: off means unchanged --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", sc.DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("window", [(-1, -1, False), (-1, -1, True), (63, 3, False)], **IDS)
@pytest.mark.parametrize("off", [0.0, 0], ids=["0.0", "int 0"])
def test_softcap_zero_is_the_call_without_the_keyword(dtype, window, off):
    L = _Launch((8, 2), dtype, window, off, seed=6)
    kw = dict(cu_seqlens_k=L.cuk_t, max_seqlen_k=L.mk)
    o0, lse0 = flash_attention.forward_varlen(L.q, L.k, L.v, L.cuq_t, L.mq, causal=L.causal, window_size=L.window_size, **kw)
    o, lse = L.forward()
    assert _same(o, o0) and _same(lse, lse0)
    want = flash_attention.backward_varlen_window(L.q, L.k, L.v, o0, lse0, L.dout, L.cuq_t, L.mq, L.window_size, causal=L.causal, **kw)
    for a, b in zip(L.backward(o, lse), want):
        assert _same(a, b)
    both = []
    for more in (dict(softcap=off), {}):
        leaves = [t.detach().clone().requires_grad_(True) for t in (L.q, L.k, L.v)]
        out = flash_attention.attention_varlen(*leaves, L.cuq_t, L.mq, causal=L.causal, window_size=L.window_size, **kw, **more)
        out.backward(L.dout)
        both.append([out] + [t.grad for t in leaves])
    torch.cuda.synchronize()
    for a, b, w in zip(both[0], both[1], (o0,) + tuple(want)):
        assert _same(a, b) and _same(a, w)


# ---- 6: equal sides ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", sc.DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("window", [(-1, -1, True), (63, 3, False)], **IDS)
def test_equal_sides_give_the_one_range_call_bits(dtype, window):
    L = _Launch((8, 2), dtype, window, 4.0, seed=2, pairs=[(300, 300), (64, 64), (257, 257), (1, 1), (130, 130)])
    assert L.cuq == L.cuk
    o, lse = L.forward()
    two = L.backward(o, lse)
    o1, lse1 = L.forward(sides=False)
    one = L.backward(o1, lse1, sides=False)
    torch.cuda.synchronize()
    for name, a, b in zip(("o", "lse", "dq", "dk", "dv"), (o, lse) + tuple(two), (o1, lse1) + tuple(one)):
        assert _same(a, b), name
    L.check_forward(o, lse, f"equal sides {dtype} window={window}")
    L.check_backward(two, f"equal sides {dtype} window={window}")


# ---- 7: loose bounds ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", sc.DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("window", [(-1, -1, True), (63, 3, False)], **IDS)
def test_loose_max_seqlens_give_the_tight_bits(dtype, window):
    """bounds far above every length: grids with workgroups that return at once.  (4, 4) has no dK / dV split under either bound,
    so every gradient's bits must agree (the split is a function of max_seqlen_k)."""
    L = _Launch((4, 4), dtype, window, 0.5, seed=1)
    o_t, lse_t = L.forward()
    tight = L.backward(o_t, lse_t)
    o, lse = L.forward(1024, 2048)
    loose = L.backward(o, lse, 1024, 2048)
    torch.cuda.synchronize()
    for name, a, b in zip(("o", "lse", "dq", "dk", "dv"), (o, lse) + tuple(loose), (o_t, lse_t) + tuple(tight)):
        assert _same(a, b), name


# ---- 8: determinism and graph capture ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("heads", sc.HEADS, **IDS)
def test_two_runs_give_the_same_bits(heads):
    L = _Launch(heads, torch.bfloat16, (63, 3, False), 4.0, seed=6)
    o, lse = L.forward()
    first = L.backward(o, lse)
    o2, lse2 = L.forward()
    again = L.backward(o2, lse2)
    torch.cuda.synchronize()
    for a, b in zip((o, lse) + tuple(first), (o2, lse2) + tuple(again)):
        assert _same(a, b)


def test_one_graph_of_forward_and_backward_replays_after_cu_seqlens_are_rewritten():
    """the launches read both offset arrays on the device: a captured forward + backward serves other lengths of the same totals"""
    dtype, window, cap = torch.bfloat16, (100, -1, True), 4.0
    first = _Launch((8, 2), dtype, window, cap, seed=7, pairs=[(300, 300), (130, 200), (257, 130)])
    second = _Launch((8, 2), dtype, window, cap, seed=8, pairs=[(100, 330), (330, 170), (257, 130)])
    assert first.q.shape == second.q.shape and first.k.shape == second.k.shape and first.cuq != second.cuq
    mq, mk = 512, 512
    q, k, v, dout = (t.clone() for t in (first.q, first.k, first.v, first.dout))
    cuq, cuk = first.cuq_t.clone(), first.cuk_t.clone()

    def step():
        o, lse = flash_attention.forward_varlen(q, k, v, cuq, mq, causal=True, cu_seqlens_k=cuk, max_seqlen_k=mk, window_size=first.window_size,
                                                softcap=cap)
        return (o, lse) + tuple(flash_attention.backward_varlen_softcap(q, k, v, o, lse, dout, cuq, mq, cap, first.window_size, causal=True,
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
        for dst, src in ((q, L.q), (k, L.k), (v, L.v), (dout, L.dout), (cuq, L.cuq_t), (cuk, L.cuk_t)):
            dst.copy_(src)
        graph.replay()
        torch.cuda.synchronize()
        o, lse = L.forward(mq, mk)
        want = (o, lse) + tuple(L.backward(o, lse, mq, mk))
        torch.cuda.synchronize()
        for name, a, b in zip(("o", "lse", "dq", "dk", "dv"), outs, want):
            assert _same(a, b), name


# ---- 9: refusals on device tensors -------------------------------------------------------------------------------------------------

def test_refusals_on_device_tensors():
    L = _Launch((4, 4), torch.bfloat16, (5, 0, False), 4.0, seed=9, pairs=[(64, 64)])
    o, lse = L.forward()
    for bad in (-1.0, float("nan"), float("inf"), True, "5", torch.tensor(5.0, device=DEV), None):
        with pytest.raises(ValueError, match="softcap"):
            L.forward(softcap=bad)
        with pytest.raises(ValueError, match="softcap"):
            L.backward(o, lse, softcap=bad)
        with pytest.raises(ValueError, match="softcap"):
            flash_attention.attention_varlen(L.q, L.k, L.v, L.cuq_t, L.mq, softcap=bad)
    # the sibling's refusals keep their type and text
    with pytest.raises(ValueError, match="causal means right = 0"):
        flash_attention.backward_varlen_softcap(L.q, L.k, L.v, o, lse, L.dout, L.cuq_t, L.mq, 4.0, (5, 5), causal=True)
    with pytest.raises(ValueError, match="cu_seqlens_k and max_seqlen_k"):
        flash_attention.backward_varlen_softcap(L.q, L.k, L.v, o, lse, L.dout, L.cuq_t, L.mq, 4.0, (5, 0), cu_seqlens_k=L.cuk_t)
    with pytest.raises(RuntimeError, match="lse must be"):
        flash_attention.backward_varlen_softcap(L.q, L.k, L.v, o, lse[:, :10], L.dout, L.cuq_t, L.mq, 4.0, (5, 0))
    with pytest.raises(ValueError, match="cu_seqlens_k and max_seqlen_k"):
        flash_attention.forward_varlen(L.q, L.k, L.v, L.cuq_t, L.mq, cu_seqlens_k=L.cuk_t, softcap=4.0)
    # the C ABI on the same tensors: the cap's own rules behind the window's, those behind the sibling's
    outs = [torch.empty_like(t) for t in (L.q, L.k, L.k)]
    a, ws, _ = L.abi_args(o, lse, outs)
    lib = _capi.load()
    w, cap = _capi.make_window(5, 0), _capi.make_softcap(4.0)
    assert lib.fa_bwd_launch_varlen_qk_softcap(ctypes.byref(a), ctypes.byref(w), None, None, None) == -1 and "fa_softcap is null" in _capi.last_error()
    assert lib.fa_bwd_launch_varlen_qk_softcap(ctypes.byref(a), None, ctypes.byref(cap), None, None) == -1 and "fa_window is null" in _capi.last_error()
    zero = _capi.make_softcap(0.0)
    assert lib.fa_bwd_launch_varlen_qk_softcap(ctypes.byref(a), ctypes.byref(w), ctypes.byref(zero), None, None) == -4 and "softcap" in _capi.last_error()
