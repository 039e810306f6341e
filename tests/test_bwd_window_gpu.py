"""The sliding-window varlen backward and the autograd path on the MI355X: fa_bwd_launch_varlen_qk_window,
flash_attention.backward_varlen_window and attention_varlen(window_size=) on the inputs of tests/window_backward_inputs.py --
every live row's head 0 targets the last key of its window, head 1 the first, and the query leaks onto the keys just outside,
so a mask off by one at either edge, a tile left out of a sweep or visited without its mask moves a gradient far beyond the
rule (tests/test_bwd_window_cpu.py shows that on the CPU for masks off by one).

One packed launch holds (len_q, len_k) = (300, 300), (130, 700), (700, 130), (257, 513), (64, 64), (1, 200), (65, 63),
(0, 50), (50, 0): more than one 128-row block and 64-row tile on either side, ragged ends, a sequence whose first rows see no
key, and empty sides.  The comparison is the project's gradient rule (bi.grad_rule), per sequence: against fp32 autograd of
eager attention with the window mask on the same 16-bit inputs, max|g - g32| <= 2 max|g16 - g32| + 1e-4 and
||g - g32|| / ||g32|| <= 2 ||g16 - g32|| / ||g32|| + 1e-3.  Each test prints its worst err / bound per gradient before it
asserts (DESIGN.md 9.4 quotes them)."""
import ctypes

import pytest
import torch

import flash_attention
from flash_attention_from_scratch_amd import _capi
from tests import beacon_inputs as bi
from tests import window_backward_inputs as wb

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
DTYPES = [torch.bfloat16, torch.float16]
NAN16 = 0x7FC0   # a NaN in bf16 and in fp16


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
    """The packed sequences of one launch under one window, with their references' forward and dout; the conditions the
    construction promises are asserted on these very tensors.  The inputs are made on the CPU (its generator: the same tensors
    wherever the test runs, the ones tests/test_bwd_window_cpu.py's proof is about) and moved to the device."""

    def __init__(self, heads, dtype, window, pairs=wb.PAIRS, seed=0, conditions=True):
        self.heads, self.dtype = heads, dtype
        self.left, self.right = bi.window_sides(*window)
        self.causal = window[2]
        self.window_size = (window[0], window[1])
        self.seqs, self.fwd = [], []
        p_lo, p_hi, ds_min = 1.0, 0.0, float("inf")
        for i, (n_q, n_k) in enumerate(pairs):
            seq = wb.sequence(n_q, n_k, heads, dtype, self.left, self.right, seed=seed + 10 * i + 3)
            o32, lse32, dout = wb.forward_and_dout(seq, seed=3000 + seed + 10 * i)
            p, several = bi.target_probabilities(seq, lse32)
            ds, _ = bi.target_ds(seq, dout, o32, lse32)
            if bool(several.any()):
                p_lo, p_hi = min(p_lo, p[several].min().item()), max(p_hi, p[several].max().item())
                ds_min = min(ds_min, ds[several].abs().min().item())
            self.seqs.append({name: t.to(DEV) if name in ("q", "k", "v") else t for name, t in seq.items()})
            self.fwd.append((o32.to(DEV), lse32.to(DEV), dout.to(DEV)))
        self.conditions = (p_lo, p_hi, ds_min)
        if conditions:
            assert bi.P_LO <= p_lo and p_hi <= bi.P_HI and ds_min >= bi.DS_FLOOR, (window, self.conditions)
        self.q, self.k, self.v, self.cuq, self.cuk = bi.pack(self.seqs)
        self.dout = torch.cat([f[2] for f in self.fwd])
        self.cuq_t, self.cuk_t = (torch.tensor(c, dtype=torch.int32, device=DEV) for c in (self.cuq, self.cuk))
        self.mq, self.mk = max(max(s["n_q"] for s in self.seqs), 1), max(max(s["n_k"] for s in self.seqs), 1)

    def forward(self, mq=None, mk=None, window_size=None, sides=True):
        kw = dict(cu_seqlens_k=self.cuk_t, max_seqlen_k=mk or self.mk) if sides else {}
        return flash_attention.forward_varlen(self.q, self.k, self.v, self.cuq_t, mq or self.mq, causal=self.causal,
                                              window_size=self.window_size if window_size is None else window_size, **kw)

    def backward(self, o, lse, mq=None, mk=None, window_size=None, sides=True):
        kw = dict(cu_seqlens_k=self.cuk_t, max_seqlen_k=mk or self.mk) if sides else {}
        return flash_attention.backward_varlen_window(self.q, self.k, self.v, o, lse, self.dout, self.cuq_t, mq or self.mq,
                                                      self.window_size if window_size is None else window_size, causal=self.causal, **kw)

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
            varlen=_capi.make_varlen_layout(self.cuq_t.data_ptr(), len(self.seqs), q.shape[0], mq or self.mq),
            varlen_k=_capi.make_varlen_layout(self.cuk_t.data_ptr(), len(self.seqs), k.shape[0], mk or self.mk))
        nbytes = _capi.load().fa_bwd_varlen_qk_workspace_bytes(ctypes.byref(a))
        assert nbytes > 0, _capi.last_error()
        delta = (4 * q.shape[1] * q.shape[0] + 15) & ~15
        per_split = 4 * k.shape[1] * k.shape[0] * 2 * 128
        assert (nbytes - delta) % per_split == 0
        split = (nbytes - delta) // per_split or 1
        ws = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
        a.workspace = ws.data_ptr()
        return a, ws, split

    def backward_abi_into_nan(self, o, lse, mq=None, mk=None):
        """the C ABI call on outputs whose storage holds NaN -> (dq, dk, dv), split"""
        outs = [torch.full(t.shape, NAN16, dtype=torch.int16, device=DEV).view(self.dtype) for t in (self.q, self.k, self.k)]
        assert all(bool(torch.isnan(t).all()) for t in outs)
        a, ws, split = self.abi_args(o, lse, outs, mq, mk)
        w = _capi.make_window(*self.window_size)
        stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        _capi.check(_capi.load().fa_bwd_launch_varlen_qk_window(ctypes.byref(a), ctypes.byref(w), stream, None))
        torch.cuda.synchronize()
        return outs, split

    def check(self, grads, tag):
        """the gradient rule per sequence, and the exact zeros -> the worst err / bound per gradient; asserts"""
        ratio, failures = {"dq": 0.0, "dk": 0.0, "dv": 0.0}, []
        for i, (seq, (_, _, dout)) in enumerate(zip(self.seqs, self.fwd)):
            sq, sk = slice(self.cuq[i], self.cuq[i + 1]), slice(self.cuk[i], self.cuk[i + 1])
            mine = (grads[0][sq], grads[1][sk], grads[2][sk])
            g32, g16 = wb.eager_backward(seq, dout, torch.float32), wb.eager_backward(seq, dout, self.dtype)
            for name, g, r32, r16 in zip(("dq", "dk", "dv"), mine, g32, g16):
                assert g.shape == r32.shape, (tag, i, name)
                if not g.numel():   # (an empty side: nothing to compare)
                    continue
                res = bi.grad_rule(g, r32, r16)
                ratio[name] = max(ratio[name], res["ratio"])
                if not res["ok"]:
                    failures.append((i, seq["n_q"], seq["n_k"], name, res))
            dead = (seq["diag"] < seq["lo"]).to(DEV)
            assert bool((mine[0][dead] == 0).all()), (tag, i, "dq of a row that sees no key")
            unseen = wb.unseen_keys(seq).to(DEV)
            assert bool((mine[1][unseen] == 0).all()) and bool((mine[2][unseen] == 0).all()), (tag, i, "dk / dv of a key no row sees")
        print(f"window backward {tag}: worst err / bound dq {ratio['dq']:.3f} dk {ratio['dk']:.3f} dv {ratio['dv']:.3f}, "
              f"target probabilities {self.conditions[0]:.3f} .. {self.conditions[1]:.3f}, smallest |dS| {self.conditions[2]:.2f}")
        assert not failures, failures[:4]
        return ratio


# ---- 1, 2: against the reference, and the exact zeros ------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("heads", wb.HEADS, ids=str)
@pytest.mark.parametrize("window", wb.WINDOWS, ids=str)
def test_against_eager_autograd_with_exact_zeros(dtype, heads, window):
    """through the C ABI on outputs that hold NaN: every row and key of every sequence is written, rows that see no key and keys
    no row sees with exact zeros; the wrapper gives the same bits.  (4, 4) runs without a dK / dV split, the other two with one."""
    L = _Launch(heads, dtype, window)
    o, lse = L.forward()
    grads, split = L.backward_abi_into_nan(o, lse)
    assert split == (1 if heads[0] == heads[1] else 4), split
    for g in grads:
        assert not bool(torch.isnan(g).any())
    L.check(grads, f"{dtype} heads={heads} window={window} split={split}")
    for a, b in zip(grads, L.backward(o, lse)):
        assert _same(a, b)


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("window", [(63, 0, False), (100, -1, True), (17, 9, False), (-1, 5, False)], ids=str)
def test_loose_max_seqlens(dtype, window):
    """the second launch: max_seqlen bounds far above every length (grids with workgroups that return at once).  The dK / dV split
    is a function of max_seqlen_k: under the loose bound the plain launches run without one (288 workgroups), the causal ones
    with the tight launch's 4, and where the splits agree the tight launch's bits come out; dq does not depend on the split."""
    L = _Launch((8, 2), dtype, window, seed=1)
    o, lse = L.forward(*wb.LOOSE)
    grads, split = L.backward_abi_into_nan(o, lse, *wb.LOOSE)
    assert split == (4 if window[2] else 1), split
    L.check(grads, f"loose {dtype} window={window} split={split}")
    o_t, lse_t = L.forward()
    assert _same(o, o_t) and _same(lse, lse_t)
    tight = L.backward(o_t, lse_t)
    assert _same(grads[0], tight[0])
    if split == 4:   # (the tight launch's split: test_against_eager_autograd_with_exact_zeros asserts it)
        assert _same(grads[1], tight[1]) and _same(grads[2], tight[2])


# ---- 3: equal sides ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("window", [(0, 0, False), (64, -1, True), (17, 9, False), (5, -1, False)], ids=str)
def test_equal_sides_give_the_one_range_call_bits(dtype, window):
    L = _Launch((8, 2), dtype, window, pairs=[(300, 300), (64, 64), (257, 257), (1, 1), (130, 130)], seed=2)
    assert L.cuq == L.cuk
    o, lse = L.forward()
    two = L.backward(o, lse)
    o1, lse1 = L.forward(sides=False)
    one = L.backward(o1, lse1, sides=False)
    torch.cuda.synchronize()
    for name, a, b in zip(("o", "lse", "dq", "dk", "dv"), (o, lse) + tuple(two), (o1, lse1) + tuple(one)):
        assert _same(a, b), name
    L.check(two, f"equal sides {dtype} window={window}")


# ---- 4: a window that covers everything --------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("causal", [False, True], ids=["plain", "causal"])
def test_covering_window_against_the_unwindowed_backward(dtype, causal):
    """left >= every len_k, right = -1, through the windowed entry, on the UNWINDOWED forward's o and lse: within the rule, and
    within the rule's bound of backward_varlen.  The bits are reported, not asserted: the windowed kernels mask with a select on
    p, the plain kernels with S = -inf (DESIGN.md 9.4 says which form differs)."""
    L = _Launch((8, 2), dtype, (1000, -1, causal), seed=4)
    o, lse = L.forward(window_size=(-1, -1))
    ow, lsew = L.forward()
    print(f"covering window {dtype} causal={causal}: forward bits equal: o {_same(o, ow)} lse {_same(lse, lsew)}")
    win = L.backward(o, lse)
    plain = flash_attention.backward_varlen(L.q, L.k, L.v, o, lse, L.dout, L.cuq_t, L.mq, causal=causal, cu_seqlens_k=L.cuk_t, max_seqlen_k=L.mk)
    torch.cuda.synchronize()
    L.check(win, f"covering {dtype} causal={causal}")
    same = [_same(a, b) for a, b in zip(win, plain)]
    print(f"covering window {dtype} causal={causal}: backward bits equal to backward_varlen: dq {same[0]} dk {same[1]} dv {same[2]}")
    for i, (seq, (_, _, dout)) in enumerate(zip(L.seqs, L.fwd)):
        sq, sk = slice(L.cuq[i], L.cuq[i + 1]), slice(L.cuk[i], L.cuk[i + 1])
        g32, g16 = wb.eager_backward(seq, dout, torch.float32), wb.eager_backward(seq, dout, dtype)
        for name, a, b, r32, r16, s in zip(("dq", "dk", "dv"), win, plain, g32, g16, (sq, sk, sk)):
            bound = bi.grad_bounds(r32, r16)["bound"] if r32.numel() else 0.0
            if not a[s].numel():
                continue
            diff = (a[s].float() - b[s].float()).abs().max().item()
            assert diff <= bound, (i, name, diff, bound)


# ---- 5: autograd -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("window", [(63, 0, False), (100, -1, True), (17, 9, False), (-1, -1, False), (-1, -1, True)], ids=str)
@pytest.mark.parametrize("sides", [True, False], ids=["two ranges", "one range"])
def test_attention_varlen_carries_the_window_to_both_passes(dtype, window, sides):
    pairs = wb.PAIRS if sides else [(300, 300), (64, 64), (257, 257)]
    L = _Launch((8, 2), dtype, window, pairs=pairs, seed=5, conditions=False)
    kw = dict(cu_seqlens_k=L.cuk_t, max_seqlen_k=L.mk) if sides else {}
    leaves = [t.detach().clone().requires_grad_(True) for t in (L.q, L.k, L.v)]
    out = flash_attention.attention_varlen(*leaves, L.cuq_t, L.mq, causal=L.causal, window_size=L.window_size, **kw)
    out.backward(L.dout)
    o, lse = L.forward(sides=sides)
    grads = L.backward(o, lse, sides=sides)
    torch.cuda.synchronize()
    assert _same(out, o)
    for name, leaf, g in zip(("dq", "dk", "dv"), leaves, grads):
        assert _same(leaf.grad, g), name
    if L.window_size == (-1, -1):   # today's attention_varlen, bit for bit
        old = [t.detach().clone().requires_grad_(True) for t in (L.q, L.k, L.v)]
        out0 = flash_attention.attention_varlen(*old, L.cuq_t, L.mq, causal=L.causal, **kw)
        out0.backward(L.dout)
        plain = flash_attention.backward_varlen(L.q, L.k, L.v, o, lse, L.dout, L.cuq_t, L.mq, causal=L.causal, **kw)
        assert _same(out0, out)
        for name, leaf, a, g in zip(("dq", "dk", "dv"), leaves, old, plain):
            assert _same(leaf.grad, a.grad) and _same(a.grad, g), name


# ---- 6: determinism ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("heads", [(4, 4), (8, 2)], ids=str)
def test_two_runs_give_the_same_bits(heads):
    L = _Launch(heads, torch.bfloat16, (17, 9, False), seed=6, conditions=False)
    o, lse = L.forward()
    first = L.backward(o, lse)
    again = L.backward(o, lse)
    torch.cuda.synchronize()
    for a, b in zip(first, again):
        assert _same(a, b)


# ---- 7: graph capture --------------------------------------------------------------------------------------------------------------

def test_one_graph_of_forward_and_backward_replays_after_cu_seqlens_are_rewritten():
    """the launches read both offset arrays on the device: a captured forward + backward serves other lengths under the same bounds"""
    dtype, window = torch.bfloat16, (63, 0, False)
    first = _Launch((8, 2), dtype, window, pairs=[(300, 300), (130, 700), (257, 513)], seed=7, conditions=False)
    second = _Launch((8, 2), dtype, window, pairs=[(100, 400), (330, 600), (257, 513)], seed=8, conditions=False)
    assert first.q.shape == second.q.shape and first.k.shape == second.k.shape and first.cuq != second.cuq
    mq, mk = 512, 1024
    q, k, v, dout = (t.clone() for t in (first.q, first.k, first.v, first.dout))
    cuq, cuk = first.cuq_t.clone(), first.cuk_t.clone()

    def step():
        o, lse = flash_attention.forward_varlen(q, k, v, cuq, mq, cu_seqlens_k=cuk, max_seqlen_k=mk, window_size=first.window_size)
        return (o, lse) + tuple(flash_attention.backward_varlen_window(q, k, v, o, lse, dout, cuq, mq, first.window_size, cu_seqlens_k=cuk,
                                                                       max_seqlen_k=mk))
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


# ---- 8: refusals on device tensors -------------------------------------------------------------------------------------------------

def test_refusals_on_device_tensors():
    L = _Launch((4, 4), torch.bfloat16, (5, 0, False), pairs=[(64, 64)], seed=9, conditions=False)
    o, lse = L.forward()
    with pytest.raises(ValueError, match="causal means right = 0"):
        flash_attention.backward_varlen_window(L.q, L.k, L.v, o, lse, L.dout, L.cuq_t, L.mq, (5, 5), causal=True)
    with pytest.raises(ValueError, match="cu_seqlens_k and max_seqlen_k"):
        flash_attention.backward_varlen_window(L.q, L.k, L.v, o, lse, L.dout, L.cuq_t, L.mq, (5, 0), cu_seqlens_k=L.cuk_t)
    with pytest.raises(RuntimeError, match="lse must be"):
        flash_attention.backward_varlen_window(L.q, L.k, L.v, o, lse[:, :10], L.dout, L.cuq_t, L.mq, (5, 0))
    # the C ABI on the same tensors: the window's own rules behind the sibling's
    outs = [torch.empty_like(t) for t in (L.q, L.k, L.k)]
    a, ws, _ = L.abi_args(o, lse, outs)
    lib = _capi.load()
    a.causal = 1
    w = _capi.make_window(5, 5)
    assert lib.fa_bwd_launch_varlen_qk_window(ctypes.byref(a), ctypes.byref(w), None, None) == -4 and "causal means right = 0" in _capi.last_error()
    assert lib.fa_bwd_launch_varlen_qk_window(ctypes.byref(a), None, None, None) == -1 and "fa_window is null" in _capi.last_error()
