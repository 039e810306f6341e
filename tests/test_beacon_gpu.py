"""Position-sensitive inputs on the MI355X: forward_kvcache, forward_varlen / backward_varlen (with and without cu_seqlens_k)
and forward_ex on the beacon inputs of tests/beacon_inputs.py, where one designated key carries about half of each row's
probability and every key position the kernels treat specially is some row's target -- a key lost, or counted twice, at a
seam moves o by more than 1 instead of by 1 / n.  tests/test_beacon_cpu.py shows on the CPU that the comparison used here
rejects every such mutant -- on inputs of the same generator, not the same tensors (other lengths and capacities, another
device's random stream), so the condition that proof rests on is asserted here again, at the full lengths: every target's fp32
probability lies in [0.25, 0.75] wherever the row sees two keys or more.

The comparison is tests/test_decode_gpu.py's, per sequence or batch entry: max|O - O32| <= max(O_TOL, 2 max|O_eager16 - O32|),
lse within 1e-3 on live rows, -inf rows exact; the gradients by tests/test_varlen_qk_gpu.py's rule, per sequence.  Each test
prints its worst err / bound before it asserts (DESIGN.md 4 quotes them)."""
import pytest
import torch

import flash_attention
from flash_attention_from_scratch_amd import flash_attention_kernels as fak
from tests import beacon_inputs as bi
from tests.test_decode_gpu import _paginate
from tests.test_varlen_qk_gpu import _check_grad, _same

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
DTYPES = [torch.bfloat16, torch.float16]


@pytest.fixture(autouse=True)
def _no_tf32():
    old = torch.backends.cuda.matmul.allow_tf32
    torch.backends.cuda.matmul.allow_tf32 = False
    yield
    torch.backends.cuda.matmul.allow_tf32 = old


class _Worst:
    """the worst err / bound of a family, printed before the assertions' verdict is final"""

    def __init__(self, family):
        self.family, self.o, self.lse, self.failures = family, 0.0, 0.0, []
        self.p_lo, self.p_hi = 1.0, 0.0

    def check(self, tag, o, lse, seq, dtype):
        refs = bi.references(seq)
        p, several = bi.target_probabilities(seq, refs[1])
        if bool(several.any()):
            self.p_lo, self.p_hi = min(self.p_lo, p[several].min().item()), max(self.p_hi, p[several].max().item())
        res = bi.compare(o, lse, *refs, dtype)
        self.o, self.lse = max(self.o, res["err"] / res["bound"]), max(self.lse, res["lse_err"] / bi.LSE_TOL)
        if not res["ok"]:
            print(f"FAIL {tag}: {res}")
            self.failures.append((tag, res))

    def verdict(self):
        print(f"beacon {self.family}: worst |O - O32| / bound = {self.o:.3f}, worst |lse - lse32| / 1e-3 = {self.lse:.3f}, "
              f"target probabilities {self.p_lo:.3f} .. {self.p_hi:.3f}")
        assert bi.P_LO <= self.p_lo and self.p_hi <= bi.P_HI, (self.p_lo, self.p_hi)
        assert not self.failures, self.failures[:4]


# ---- decode -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("causal", [False, True], ids=["plain", "causal"])
@pytest.mark.parametrize("H,Hkv,Sq", bi.DECODE_SHAPES)
def test_decode_on_beacons(dtype, causal, H, Hkv, Sq):
    """One batch of all lengths; the caches (beacons up to the capacity, so the rows at and beyond len are finite and match the
    last rows' queries) are built once, contiguous and in shuffled pages of 64 and 256; per split count the queries point at
    that count's positions (in as many launches as the longest list needs rows), and the paged launches repeat the
    contiguous one's bits.  A row that sees a single key (the entry of length 1; under the causal mask the first live row of
    the short entries) has probability 1 on it: there a key counted twice shows in lse only, not in o."""
    lens, cap = bi.DECODE_LENGTHS, bi.DECODE_CACHE_LEN
    lens_t = torch.tensor(lens, dtype=torch.int32, device=DEV)
    first = [bi.build_sequence(Sq, n, H, Hkv, [0], dtype, causal, n_alloc=cap, seed=b, device=DEV) for b, n in enumerate(lens)]
    k, v = torch.stack([s["k"] for s in first]), torch.stack([s["v"] for s in first])
    paged = [_paginate(k, v, lens, page_size, poison=False) for page_size in (64, 256)]
    worst = _Worst(f"decode {dtype} causal={causal} H={H} Hkv={Hkv} Sq={Sq}")
    for splits in bi.DECODE_SPLITS:
        ns = splits or fak.kvcache_num_splits(torch.stack([s["q"] for s in first]), k, v, lens_t)
        phase, n_phases = 0, 1
        while phase < n_phases:
            seqs = [bi.build_sequence(Sq, n, H, Hkv, bi.decode_positions(n, Sq, ns), dtype, causal, phase, seed=b, device=DEV,
                                      kv=(k[b], v[b])) for b, n in enumerate(lens)]
            n_phases, phase = max(s["n_phases"] for s in seqs), phase + 1
            q = torch.stack([s["q"] for s in seqs])
            o, lse = flash_attention.forward_kvcache(q, k, v, lens_t, causal=causal, return_lse=True, num_splits=splits)
            for b, s in enumerate(seqs):
                worst.check(f"len {lens[b]} splits {ns} phase {phase - 1}", o[b], lse[b], s, dtype)
            for (kp, vp, table), page_size in zip(paged, (64, 256)):
                o_p, lse_p = flash_attention.forward_kvcache(q, kp, vp, lens_t, block_table=table, causal=causal, return_lse=True,
                                                             num_splits=splits)
                assert _same(o, o_p) and _same(lse, lse_p), (page_size, ns)
    worst.verdict()


# ---- varlen, one and two ranges, forward and backward ------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("causal", [False, True], ids=["plain", "causal"])
@pytest.mark.parametrize("heads", bi.VARLEN_HEADS)
@pytest.mark.parametrize("name", list(bi.VARLEN_FAMILIES))
def test_varlen_on_beacons(dtype, causal, heads, name):
    """forward_varlen with cu_seqlens_k, and for the equal-length family without it too (the same bits), then the same
    launch through backward_varlen: the backward's run on a peaked softmax, P near 1/2 on one key."""
    Hq, Hkv = heads
    seqs, (mq, mk) = bi.varlen_family(name, Hq, Hkv, dtype, causal, device=DEV)
    q, k, v, cuq, cuk = bi.pack(seqs)
    dout = torch.randn(q.shape, generator=torch.Generator(device=DEV).manual_seed(99), device=DEV).to(dtype)
    cuq_t, cuk_t = (torch.tensor(c, dtype=torch.int32, device=DEV) for c in (cuq, cuk))
    o, lse = flash_attention.forward_varlen(q, k, v, cuq_t, mq, causal=causal, cu_seqlens_k=cuk_t, max_seqlen_k=mk)
    grads = flash_attention.backward_varlen(q, k, v, o, lse, dout, cuq_t, mq, causal=causal, cu_seqlens_k=cuk_t, max_seqlen_k=mk)
    if name == "equal":
        o_e, lse_e = flash_attention.forward_varlen(q, k, v, cuq_t, mq, causal=causal)
        grads_e = flash_attention.backward_varlen(q, k, v, o_e, lse_e, dout, cuq_t, mq, causal=causal)
        for nm, a, b in zip(("o", "lse", "dq", "dk", "dv"), (o, lse) + tuple(grads), (o_e, lse_e) + tuple(grads_e)):
            assert _same(a, b), nm
    worst = _Worst(f"varlen {name} {dtype} causal={causal} heads={heads}")
    for i, s in enumerate(seqs):
        sq = slice(cuq[i], cuq[i + 1])
        worst.check(f"seq {i} ({s['n_q']}, {s['n_k']})", o[sq], lse[:, sq], s, dtype)
    grad_failures = []
    for i, s in enumerate(seqs):   # the gradients, per sequence, against autograd through the eager forward in fp32 and in 16 bit
        sq, sk = slice(cuq[i], cuq[i + 1]), slice(cuk[i], cuk[i + 1])
        ref = []
        for ref_dtype in (torch.float32, dtype):
            leaves = [t.detach().to(ref_dtype).requires_grad_(True) for t in (q[sq], k[sk], v[sk])]
            bi.eager(*leaves, s["diag"], ref_dtype)[0].backward(dout[sq].to(ref_dtype))
            ref.append([t.grad.float() for t in leaves])
        for nm, g, r32, r16 in zip(("dq", "dk", "dv"), (grads[0][sq], grads[1][sk], grads[2][sk]), *ref):
            try:
                _check_grad(f"{nm}[seq {i}, ({s['n_q']}, {s['n_k']})]", g, r32, r16)
            except AssertionError as e:   # (collected, so that the forward's verdict and every gradient are reported together)
                grad_failures.append(str(e))
    worst.verdict()
    assert not grad_failures, grad_failures[:4]


# ---- the dense masked forward ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("n,causal", bi.DENSE_CASES)
def test_forward_ex_on_beacons(dtype, n, causal):
    """The default configuration's masked forms: ragged causal (S = 1000, o only: no log-sum-exp for a ragged length), causal
    with the log-sum-exp (S = 1024) and plain (S = 4096)."""
    from flash_helpers import kernel_configs as kc

    seq = bi.build_sequence(n, n, 4, 4, bi.dense_positions(n), dtype, causal, seed=5, device=DEV)
    cfg = kc.best_config(kc.DType.BF16 if dtype == torch.bfloat16 else kc.DType.FP16, n, masked=True)
    q, k, v = (t.contiguous() for t in (seq["q"][None], seq["k"][None, :n], seq["v"][None, :n]))
    if n % 256 == 0:
        o, lse = flash_attention.forward_ex(cfg, q, k, v, causal=causal, return_lse=True)
    else:   # the row log-sum-exp is written for seq_len % 256 == 0 only (fa_fwd_launch_lse refuses the rest): o alone
        o, lse = flash_attention.forward_ex(cfg, q, k, v, causal=causal), None
    worst = _Worst(f"forward_ex {dtype} S={n} causal={causal}")
    worst.check(f"S {n}", o[0], None if lse is None else lse[0], seq, dtype)
    worst.verdict()
