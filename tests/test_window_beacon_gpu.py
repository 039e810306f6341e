"""Sliding-window decode on position-sensitive inputs on the MI355X: flash_attention.forward_kvcache(window_size=) on the two-sided
beacon inputs of tests/beacon_inputs.py.  Every query row has a target key with about half of its
probability and leaks 1.5 times the target's score towards the first key above AND the first key below its window, and every
key the window moves is some row's target: each row's own first and last key, lo_min and the key above it, the 32-key unit,
64-key tile, page and split boundaries counted from lo_min's tile, the ragged end.  So a key lost, doubled or leaked at an edge or
a seam moves o by a large fraction of |v| and lse by about ln 2, whatever the window's width -- on the N(0, 1) inputs of
tests/test_window_decode_gpu.py it moves them by 1 / width.  tests/test_beacon_cpu.py (test_window_family_rejects_every_mutant)
shows on the CPU, for every length, window and split count launched here, that the comparison rejects both edges shifted by
+- 1, each listed key dropped or doubled and both fetch clamps failing; it holds on inputs of the same generator, not the same
tensors, so the probability condition it rests on is asserted here again before every launch.

The comparison is tests/test_decode_gpu.py's, per batch entry: max|O - O32| <= max(O_TOL, 2 max|O_eager16 - O32|), lse within
1e-3 on live rows, -inf rows exact.  The paged launches (shuffled pages of 64 and 256) repeat the contiguous one's bits.  For the
fp8 cache K is stored as +- 1 with the beacons' amplitude in k_descale (tests/test_decode_fp8_gpu.py's construction) and the
oracle runs on the dequantized cache.  Each case prints its worst figures before it asserts (DESIGN.md 4 quotes them)."""
import pytest
import torch

import flash_attention
from flash_attention_from_scratch_amd import flash_attention_kernels as fak
from tests import beacon_inputs as bi
from tests.test_decode_fp8_gpu import _beacon_fp8_cache, _paginate8
from tests.test_decode_gpu import _paginate
from tests.test_varlen_qk_gpu import _same

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
DTYPES = [torch.bfloat16, torch.float16]


@pytest.fixture(autouse=True)
def _no_tf32():
    old = torch.backends.cuda.matmul.allow_tf32
    torch.backends.cuda.matmul.allow_tf32 = False
    yield
    torch.backends.cuda.matmul.allow_tf32 = old


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("fp8", [False, True], ids=["16bit", "fp8"])
@pytest.mark.parametrize("H,Hkv,Sq", bi.DECODE_SHAPES)
def test_window_decode_on_beacons(dtype, fp8, H, Hkv, Sq):
    """One batch of all lengths (1 and 2 are shorter than every seqlen_q); the caches (beacons up to the capacity: the key
    behind every row's window is finite and is the one its query leaks towards) are built once, contiguous and in shuffled
    pages of 64 and 256; per window and split count the queries point at that pair's window_positions, in as many launches as
    the longest list needs.  (8, 1, 8) runs the 64-packed-row kernels.  Most splits are empty on the narrow windows."""
    lens, cap = bi.WINDOW_LENGTHS, bi.WINDOW_CACHE_LEN
    assert cap % 256 == 0 and cap > max(lens) and min(lens) < Sq
    lens_t = torch.tensor(lens, dtype=torch.int32, device=DEV)
    first = [bi.build_sequence(Sq, n, H, Hkv, [0], dtype, False, n_alloc=cap, seed=b, device=DEV) for b, n in enumerate(lens)]
    q0 = torch.stack([s["q"] for s in first])
    if fp8:
        k, v, kd, vd, k_ref, v_ref = _beacon_fp8_cache(first, lens, Hkv, dtype)
        extra = dict(k_descale=kd, v_descale=vd)
        paged = [_paginate8(k, v, lens, page_size, poison=False) for page_size in (64, 256)]
    else:
        k, v = torch.stack([s["k"] for s in first]), torch.stack([s["v"] for s in first])
        k_ref, v_ref, extra = k, v, {}
        paged = [_paginate(k, v, lens, page_size, poison=False) for page_size in (64, 256)]
    failures, worst_o, worst_lse, p_lo, p_hi, launches = [], 0.0, 0.0, 1.0, 0.0, 0
    for left, right, causal in bi.WINDOWS:
        side = bi.window_sides(left, right, causal)
        for splits in bi.WINDOW_SPLITS:
            ns = splits or fak.kvcache_num_splits(q0, k, v, lens_t, causal=causal, window_size=(left, right))
            phase, n_phases = 0, 1
            while phase < n_phases:
                seqs = [bi.build_window_sequence(Sq, n, H, Hkv, bi.window_positions(n, Sq, *side, ns), dtype, *side, phase, seed=b,
                                                 device=DEV, kv=(k_ref[b], v_ref[b])) for b, n in enumerate(lens)]
                n_phases, phase = max(s["n_phases"] for s in seqs), phase + 1
                refs = [bi.references(s) for s in seqs]
                for b, (s, ref) in enumerate(zip(seqs, refs)):   # before the launch: the targets carry their probability on these tensors
                    p, several = bi.target_probabilities(s, ref[1])
                    if bool(several.any()):
                        lo_b, hi_b = p[several].min().item(), p[several].max().item()
                        p_lo, p_hi = min(p_lo, lo_b), max(p_hi, hi_b)
                        assert bi.P_LO <= lo_b and hi_b <= bi.P_HI, (lens[b], (left, right, causal), ns, lo_b, hi_b)
                q = torch.stack([s["q"] for s in seqs])
                kw = dict(causal=causal, return_lse=True, num_splits=splits, window_size=(left, right), **extra)
                o, lse = flash_attention.forward_kvcache(q, k, v, lens_t, **kw)
                launches += 1
                for b, ref in enumerate(refs):
                    res = bi.compare(o[b], lse[b], *ref, dtype)
                    worst_o, worst_lse = max(worst_o, res["err"] / res["bound"]), max(worst_lse, res["lse_err"] / bi.LSE_TOL)
                    if not res["ok"]:
                        print(f"FAIL window {(left, right, causal)} len {lens[b]} splits {ns} phase {phase - 1}: {res}")
                        failures.append(((left, right, causal), lens[b], ns, phase - 1, res))
                for (kp, vp, table), page_size in zip(paged, (64, 256)):
                    o_p, lse_p = flash_attention.forward_kvcache(q, kp, vp, lens_t, block_table=table, **kw)
                    if not (_same(o, o_p) and _same(lse, lse_p)):
                        print(f"FAIL window {(left, right, causal)} splits {ns} phase {phase - 1}: pages of {page_size} differ")
                        failures.append(((left, right, causal), f"page {page_size}", ns, phase - 1))
    print(f"window beacons {'fp8' if fp8 else '16-bit'} {dtype} H={H} Hkv={Hkv} Sq={Sq}: worst |O - O32| / bound = {worst_o:.3f}, "
          f"worst |lse - lse32| / 1e-3 = {worst_lse:.3f}, target probabilities {p_lo:.3f} .. {p_hi:.3f}, {launches} contiguous launches")
    assert not failures, failures[:4]
