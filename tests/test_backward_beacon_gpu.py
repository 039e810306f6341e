"""The backward on cell-covering beacon inputs on the MI355X ("Backward cells"): flash_attention.backward dense and
GQA (the three regimes of the dK / dV split) and backward_varlen, on the inputs of tests/beacon_inputs.py's backward section.
Every live (32-row band, 32-key cell) pair under the shifted diagonal holds some (row, head)'s target key, the target carries
about half of its row's probability, and dout is constructed so that |dS| on the target is at least DS_FLOOR: a 32 x 32 product
left out of one accumulator, a diagonal flag wrong for one tile, a delta or lse row read from its neighbour, a head or a split
part lost from a key block's sum all move a gradient by far more than the rule allows.  tests/test_beacon_cpu.py
(test_backward_cells_reject_every_mutant) shows that on the CPU, on inputs of the same generator; the conditions that proof
rests on -- coverage, the target probabilities, DS_FLOOR -- are asserted here again on this file's own tensors before each launch.

The comparison is the gradient rule of tests/test_backward_gpu.py (bi.grad_rule), per sequence or batch entry: against fp32
autograd of eager attention on the same 16-bit inputs, max|g - g32| <= 2 max|g16 - g32| + 1e-4 and
||g - g32|| / ||g32|| <= 2 ||g16 - g32|| / ||g32|| + 1e-3.  Each test prints its worst err / bound per gradient before it
asserts (DESIGN.md 4 quotes them)."""
import ctypes

import pytest
import torch

import flash_attention
from flash_attention_from_scratch_amd import _capi
from flash_helpers import kernel_configs as kc
from tests import beacon_inputs as bi

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
DTYPES = [torch.bfloat16, torch.float16]
KC_DTYPE = {torch.bfloat16: kc.DType.BF16, torch.float16: kc.DType.FP16}


@pytest.fixture(autouse=True)
def _no_tf32():
    old = torch.backends.cuda.matmul.allow_tf32
    torch.backends.cuda.matmul.allow_tf32 = False
    yield
    torch.backends.cuda.matmul.allow_tf32 = old


def _same(a, b):
    view = torch.int16 if a.dtype in (torch.bfloat16, torch.float16) else torch.int32
    return a.shape == b.shape and torch.equal(a.contiguous().view(view), b.contiguous().view(view))


class _Worst:
    """the conditions on one launch's inputs, and its worst err / bound per gradient, printed before the verdict"""

    def __init__(self, family):
        self.family, self.failures = family, []
        self.ratio = {"dq": 0.0, "dk": 0.0, "dv": 0.0}
        self.p_lo, self.p_hi, self.ds = 1.0, 0.0, float("inf")

    def inputs(self, tag, phases, seed):
        """The phases of one (n_q, n_k) (one sequence or batch entry each): coverage, the probabilities and DS_FLOOR asserted
        -> [(seq, o32, lse32, dout)]"""
        assert bi.cell_coverage(phases) == ([], [], []), (tag, bi.cell_coverage(phases))
        out = []
        for n, seq in enumerate(phases):
            o32, lse32, _ = bi.references(seq)
            dout = bi.beacon_dout(seq, o32, seed=seed + n)
            p, several = bi.target_probabilities(seq, lse32)
            ds, _ = bi.target_ds(seq, dout, o32, lse32)
            if bool(several.any()):
                self.p_lo, self.p_hi = min(self.p_lo, p[several].min().item()), max(self.p_hi, p[several].max().item())
                self.ds = min(self.ds, ds[several].abs().min().item())
            out.append((seq, o32, lse32, dout))
        assert bi.P_LO <= self.p_lo and self.p_hi <= bi.P_HI and self.ds >= bi.DS_FLOOR, (tag, self.p_lo, self.p_hi, self.ds)
        return out

    def check(self, tag, seq, dout, grads):
        dtype = seq["q"].dtype
        g32, g16 = bi.eager_backward(seq, dout, torch.float32), bi.eager_backward(seq, dout, dtype)
        for name, g, r32, r16 in zip(("dq", "dk", "dv"), grads, g32, g16):
            res = bi.grad_rule(g, r32, r16)
            self.ratio[name] = max(self.ratio[name], res["ratio"])
            if not res["ok"]:
                print(f"FAIL {tag} {name}: {res}")
                self.failures.append((tag, name, res))

    def verdict(self):
        print(f"backward beacon {self.family}: worst err / bound dq {self.ratio['dq']:.3f} dk {self.ratio['dk']:.3f} "
              f"dv {self.ratio['dv']:.3f}, target probabilities {self.p_lo:.3f} .. {self.p_hi:.3f}, smallest |dS| {self.ds:.2f}")
        assert not self.failures, self.failures[:4]


def _dense_batch(worst, B, S, H, Hkv, dtype, causal, seed):
    """B batch entries with seeds of their own -> entries [(seq, o32, lse32, dout)], q, k, v, dout (B, S, heads, 128), and
    O (16 bit) and lse (B, H, S) made by torch in fp32"""
    entries = []
    for b in range(B):
        seq = bi.build_cell_sequence(S, S, H, Hkv, dtype, causal, seed=seed + 17 * b, device=DEV)
        assert seq["n_phases"] == 1
        entries += worst.inputs(f"batch entry {b}", [seq], 1000 + seed + 17 * b)
    q = torch.stack([e[0]["q"] for e in entries])
    k, v = (torch.stack([e[0][name][:S] for e in entries]) for name in ("k", "v"))
    dout = torch.stack([e[3] for e in entries])
    o = torch.stack([e[1] for e in entries]).to(dtype)
    lse = torch.stack([e[2] for e in entries]).contiguous()
    return entries, q, k, v, dout, o, lse


# ---- dense ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("causal", [False, True], ids=["plain", "causal"])
@pytest.mark.parametrize("S,source", [(256, "torch"), (512, "torch"), (1024, "torch"), (256, "forward_ex"), (512, "forward_ex"),
                                      (1024, "forward_ex"), (512, "packed")])
def test_dense_backward_on_beacon_cells(dtype, causal, S, source):
    """S = 256: two key blocks, the smallest sweep; S = 1024: eight.  "torch": O and lse made by torch in fp32, which isolates
    the backward; "forward_ex": the forward's own O and lse; "packed": q, k, v views of one (B, S, 3, H, 128) buffer."""
    B, H = 2, 4
    worst = _Worst(f"dense {dtype} S={S} causal={causal} {source}")
    entries, q, k, v, dout, o, lse = _dense_batch(worst, B, S, H, H, dtype, causal, seed=S + 3)
    if source == "packed":
        qkv = torch.stack([q, k, v], dim=2)
        q, k, v = qkv[:, :, 0], qkv[:, :, 1], qkv[:, :, 2]
        assert q.stride(1) == 3 * H * 128
    if source == "forward_ex":
        cfg = kc.best_config(KC_DTYPE[dtype], S, masked=causal)
        o, lse = flash_attention.forward_ex(cfg, q, k, v, causal=causal, return_lse=True)
    grads = flash_attention.backward(q, k, v, o, lse, dout, causal=causal)
    torch.cuda.synchronize()
    for g in grads:
        assert g.shape == (B, S, H, 128) and g.dtype == dtype
    for b, (seq, _, _, d) in enumerate(entries):
        worst.check(f"batch entry {b}", seq, d, [g[b] for g in grads])
    worst.verdict()


# ---- GQA: the three regimes of the dK / dV split ---------------------------------------------------------------------------------------

def _rule_split(B, S, H, Hkv, causal):
    """the smallest divisor of G = H / Hkv for which batch x Hkv x split x S / 128 workgroups reach 256 (1024
    under the causal mask), else G"""
    group, workgroups = H // Hkv, B * Hkv * (S // 128)
    for split in range(1, group + 1):
        if group % split == 0 and workgroups * split >= (1024 if causal else 256):
            return split
    return group


def _abi_split(B, S, H, Hkv, causal):
    """the split the C ABI's two workspace sizes imply: the GQA backward's less the MHA backward's is the fp32 partials,
    split x batch x Hkv x S x 2 x 128 floats, none for split = 1"""
    base = _capi.FaBwdArgs(batch=B, seq_len=S, n_heads=H, d_head=128, qkv_batch_stride=S * H * 128, qkv_seq_stride=H * 128,
                           qkv_head_stride=128, out_batch_stride=S * H * 128, out_seq_stride=H * 128, out_head_stride=128,
                           dtype=15, causal=int(causal))
    a = _capi.FaBwdGqaArgs(base=base, n_kv_heads=Hkv, kv_batch_stride=S * Hkv * 128, kv_seq_stride=Hkv * 128, kv_head_stride=128,
                           dkv_batch_stride=S * Hkv * 128, dkv_seq_stride=Hkv * 128, dkv_head_stride=128)
    lib = _capi.load()
    gqa, mha = lib.fa_bwd_gqa_workspace_bytes(ctypes.byref(a)), lib.fa_bwd_workspace_bytes(ctypes.byref(base))
    assert gqa >= mha > 0, (gqa, mha, _capi.last_error())
    extra = gqa - mha
    assert extra % (4 * B * Hkv * S * 2 * 128) == 0
    return 1 if extra == 0 else extra // (4 * B * Hkv * S * 2 * 128)


# (B, S, H, Hkv), mask -> the split the documented rule gives
GQA_CASES = [((8, 1024, 8, 4), False, 1),    # 256 workgroups: one workgroup sweeps all G = 2 heads
             ((8, 1024, 8, 4), True, 2),     # causal asks for 1024: split = G
             ((4, 1024, 16, 2), False, 4),   # 1 < split < G: 4 of 8, two heads per part
             ((1, 512, 8, 1), False, 8),     # 4 workgroups: split = G under both masks
             ((1, 512, 8, 1), True, 8)]


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("shape,causal,split", GQA_CASES)
def test_gqa_backward_on_beacon_cells(dtype, shape, causal, split):
    """Every query head has targets of its own in every 128-key block it sees (cell_coverage), so a head or a part lost from a
    block's sum shows; dQ is bit-identical to the MHA backward on K / V expanded with repeat_interleave."""
    B, S, H, Hkv = shape
    assert _rule_split(B, S, H, Hkv, causal) == split == _abi_split(B, S, H, Hkv, causal)
    worst = _Worst(f"gqa {dtype} {shape} causal={causal} split={split}")
    entries, q, k, v, dout, o, lse = _dense_batch(worst, B, S, H, Hkv, dtype, causal, seed=S + H + Hkv)
    dq, dk, dv = flash_attention.backward(q, k, v, o, lse, dout, causal=causal)
    G = H // Hkv
    dq_m, _, _ = flash_attention.backward(q, k.repeat_interleave(G, dim=2).contiguous(), v.repeat_interleave(G, dim=2).contiguous(),
                                          o, lse, dout, causal=causal)
    torch.cuda.synchronize()
    assert dq.shape == q.shape and dk.shape == k.shape and dv.shape == v.shape
    assert _same(dq, dq_m)
    for b, (seq, _, _, d) in enumerate(entries):
        worst.check(f"batch entry {b}", seq, d, (dq[b], dk[b], dv[b]))
    worst.verdict()


# ---- varlen -----------------------------------------------------------------------------------------------------------------------

def _varlen_launch(worst, pairs, heads, dtype, causal, seed):
    """One packed launch of `pairs`, a pair that needs several phases repeated, one copy per phase -> entries, packed tensors"""
    entries = []
    for i, (n_q, n_k) in enumerate(pairs):
        phases, phase, n_phases = [], 0, 1
        while phase < n_phases:
            phases.append(bi.build_cell_sequence(n_q, n_k, heads[0], heads[1], dtype, causal, phase, seed=seed + 10 * i + phase, device=DEV))
            n_phases, phase = phases[-1]["n_phases"], phase + 1
        entries += worst.inputs(f"pair ({n_q}, {n_k})", phases, 2000 + seed + 10 * i)
    q, k, v, cuq, cuk = bi.pack([e[0] for e in entries])
    dout = torch.cat([e[3] for e in entries])
    return entries, q, k, v, dout, cuq, cuk


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("causal", [False, True], ids=["plain", "causal"])
@pytest.mark.parametrize("heads", bi.BACKWARD_HEADS)
def test_varlen_backward_on_beacon_cells(dtype, causal, heads):
    """One packed launch of (512, 512), (300, 300), (129, 300), (64, 1), cells clipped to each sequence, through forward_varlen
    and backward_varlen with cu_seqlens_k; the equal-length subset gives the same bits without cu_seqlens_k."""
    worst = _Worst(f"varlen {dtype} causal={causal} heads={heads}")
    entries, q, k, v, dout, cuq, cuk = _varlen_launch(worst, bi.BACKWARD_VARLEN_PAIRS, heads, dtype, causal, seed=5)
    cuq_t, cuk_t = (torch.tensor(c, dtype=torch.int32, device=DEV) for c in (cuq, cuk))
    mq, mk = max(e[0]["n_q"] for e in entries), max(e[0]["n_k"] for e in entries)
    o, lse = flash_attention.forward_varlen(q, k, v, cuq_t, mq, causal=causal, cu_seqlens_k=cuk_t, max_seqlen_k=mk)
    grads = flash_attention.backward_varlen(q, k, v, o, lse, dout, cuq_t, mq, causal=causal, cu_seqlens_k=cuk_t, max_seqlen_k=mk)
    torch.cuda.synchronize()
    for i, (seq, _, _, d) in enumerate(entries):
        sq, sk = slice(cuq[i], cuq[i + 1]), slice(cuk[i], cuk[i + 1])
        worst.check(f"seq {i} ({seq['n_q']}, {seq['n_k']})", seq, d, (grads[0][sq], grads[1][sk], grads[2][sk]))
    # the equal-length subset: one range and two ranges, the same bits
    equal = [p for p in bi.BACKWARD_VARLEN_PAIRS if p[0] == p[1]]
    assert len(equal) >= 2
    _, q, k, v, dout, cuq, cuk = _varlen_launch(_Worst("equal"), equal, heads, dtype, causal, seed=5)
    assert cuq == cuk
    cu_t, m = torch.tensor(cuq, dtype=torch.int32, device=DEV), max(p[0] for p in equal)
    o, lse = flash_attention.forward_varlen(q, k, v, cu_t, m, causal=causal, cu_seqlens_k=cu_t, max_seqlen_k=m)
    two = flash_attention.backward_varlen(q, k, v, o, lse, dout, cu_t, m, causal=causal, cu_seqlens_k=cu_t, max_seqlen_k=m)
    o_e, lse_e = flash_attention.forward_varlen(q, k, v, cu_t, m, causal=causal)
    one = flash_attention.backward_varlen(q, k, v, o_e, lse_e, dout, cu_t, m, causal=causal)
    torch.cuda.synchronize()
    for name, a, b in zip(("o", "lse", "dq", "dk", "dv"), (o, lse) + tuple(two), (o_e, lse_e) + tuple(one)):
        assert _same(a, b), name
    worst.verdict()
