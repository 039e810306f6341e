"""Packed sequences with separate Q and K / V lengths, timing (the sibling of varlen_bench.py).  One JSON line per case; all arms
of a case alternate in one process, event-timed medians after two warm-up rounds:
  - "parity":  the backward on equal sides with the key side given (the two-range kernels) against backward_varlen without it
               (the one-range kernels) on the same tensors -- the uniform 16 x 4096 batch and varlen_bench.py's mixed batch.
               The arm without the key side runs TWICE per round; the spread between its two medians is the margin the
               ratio is read against (`bwd_margin`).  The forward is one kernel either way and is not timed here
               (profiles/training/varlen_fold_parity_bf16.jsonl: the run, forward included, on which it was folded).
  - "prefill": chunked prefill, len_q in {512, 2048} against len_k in {8192, 32768}, causal (bottom-right), batch 8, H / Hkv =
               32 / 8 and 16 / 16: ms and useful TFLOP/s on the shifted-causal FLOP count (4 d per visible (query, key) pair
               forward, 10 d backward), forward and forward + backward.
  - "sdpa":    on the prefill cases small enough for it, torch's scaled_dot_product_attention, one call per sequence on sliced
               tensors with an explicit bottom-right mask, K / V heads expanded beforehand.  batch calls against one launch:
               this flatters the new path by the launch count.
Kernel times of their own: run it under `rocprofv3 --kernel-trace --stats -- python .../varlen_qk_bench.py --arms prefill --reps 3`.

    python flash_attention_from_scratch_amd/tools/varlen_qk_bench.py [--reps N] [--arms parity,prefill,sdpa] [--out FILE]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402

import flash_attention  # noqa: E402
from flash_attention_from_scratch_amd.tools.varlen_bench import mixed_lengths  # noqa: E402


def _median(x):
    return sorted(x)[len(x) // 2]


def _cu(lengths):
    out = [0]
    for n in lengths:
        out.append(out[-1] + n)
    return torch.tensor(out, dtype=torch.int32).cuda()


def _tensors(Tq, Tk, H, Hkv, dtype):
    gen = torch.Generator().manual_seed(0)
    q, dout = (torch.randn((Tq, H, 128), generator=gen).to(dtype).cuda() for _ in range(2))
    k, v = (torch.randn((Tk, Hkv, 128), generator=gen).to(dtype).cuda() for _ in range(2))
    return q, k, v, dout


def parity(case, lengths, H, Hkv, causal, dtype, reps):
    T, m = sum(lengths), max(lengths)
    q, k, v, dout = _tensors(T, T, H, Hkv, dtype)
    cu, cuk = _cu(lengths), _cu(lengths)
    t = {name: [] for name in ("bwd_old_a", "bwd_new", "bwd_old_b")}
    o, lse = flash_attention.forward_varlen(q, k, v, cu, m, causal=causal)
    for i in range(reps + 2):
        *_, b0 = flash_attention.backward_varlen(q, k, v, o, lse, dout, cu, m, causal=causal, timed=True)
        *_, b1 = flash_attention.backward_varlen(q, k, v, o, lse, dout, cu, m, causal=causal, timed=True, cu_seqlens_k=cuk, max_seqlen_k=m)
        *_, b2 = flash_attention.backward_varlen(q, k, v, o, lse, dout, cu, m, causal=causal, timed=True)
        if i > 1:
            for name, ms in zip(t, (b0, b1, b2)):
                t[name].append(ms)
    med = {name: _median(x) for name, x in t.items()}
    line = {"arm": "parity", "case": case, "n_seqs": len(lengths), "total_tokens": T, "n_heads": H, "n_kv_heads": Hkv,
            "dtype": str(dtype).replace("torch.", ""), "causal": causal, "reps": reps, **{name + "_ms": ms for name, ms in med.items()}}
    old = 0.5 * (med["bwd_old_a"] + med["bwd_old_b"])
    line["bwd_new_over_old"] = med["bwd_new"] / old
    line["bwd_margin"] = abs(med["bwd_old_a"] - med["bwd_old_b"]) / old   # the one-range arm against itself
    return line


def _pairs(len_q, len_k):
    """visible (query, key) pairs of one sequence under the bottom-right causal mask"""
    return sum(min(len_k, max(0, r + len_k - len_q + 1)) for r in range(len_q))


def prefill(len_q, len_k, batch, H, Hkv, dtype, reps, sdpa):
    q, k, v, dout = _tensors(batch * len_q, batch * len_k, H, Hkv, dtype)
    cuq, cuk = _cu([len_q] * batch), _cu([len_k] * batch)
    fwd, bwd, ref_f, ref_fb = [], [], [], []
    if sdpa:
        G = H // Hkv
        mask = torch.ones((len_q, len_k), dtype=torch.bool, device="cuda").tril(diagonal=len_k - len_q)
        seqs = []
        for b in range(batch):   # (batch, heads, seq, d) views of one sequence each; K / V expanded to the query heads, untimed
            qs = q[b * len_q:(b + 1) * len_q].transpose(0, 1)[None].detach().requires_grad_(True)
            ks, vs = (t[b * len_k:(b + 1) * len_k].repeat_interleave(G, dim=1).transpose(0, 1)[None].detach().requires_grad_(True) for t in (k, v))
            seqs.append((qs, ks, vs, dout[b * len_q:(b + 1) * len_q].transpose(0, 1)[None]))
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
    for i in range(reps + 2):
        o, lse, f = flash_attention.forward_varlen(q, k, v, cuq, len_q, causal=True, timed=True, cu_seqlens_k=cuk, max_seqlen_k=len_k)
        *_, b = flash_attention.backward_varlen(q, k, v, o, lse, dout, cuq, len_q, causal=True, timed=True, cu_seqlens_k=cuk, max_seqlen_k=len_k)
        if sdpa:
            ev[0].record()
            outs = [torch.nn.functional.scaled_dot_product_attention(qs, ks, vs, attn_mask=mask) for qs, ks, vs, _ in seqs]
            ev[1].record()
            for out, (qs, ks, vs, g) in zip(outs, seqs):
                out.backward(g)
                qs.grad = ks.grad = vs.grad = None
            ev[2].record()
            torch.cuda.synchronize()
        if i > 1:
            fwd.append(f), bwd.append(b)
            if sdpa:
                ref_f.append(ev[0].elapsed_time(ev[1])), ref_fb.append(ev[0].elapsed_time(ev[2]))
    flop_f = 4.0 * 128 * H * batch * _pairs(len_q, len_k)
    f_ms, b_ms = _median(fwd), _median(bwd)
    line = {"arm": "prefill", "len_q": len_q, "len_k": len_k, "batch": batch, "n_heads": H, "n_kv_heads": Hkv, "causal": True,
            "dtype": str(dtype).replace("torch.", ""), "reps": reps, "fwd_ms": f_ms, "bwd_ms": b_ms, "fwd_bwd_ms": f_ms + b_ms,
            "fwd_tflops": flop_f / f_ms * 1e-9, "fwd_bwd_tflops": 3.5 * flop_f / (f_ms + b_ms) * 1e-9,
            "fwd_workgroups": batch * H * ((len_q + 127) // 128)}
    if sdpa:
        line.update({"sdpa_calls": batch, "sdpa_fwd_ms": _median(ref_f), "sdpa_fwd_bwd_ms": _median(ref_fb),
                     "fwd_over_sdpa": f_ms / _median(ref_f), "fwd_bwd_over_sdpa": (f_ms + b_ms) / _median(ref_fb)})
    return line


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--arms", default="parity,prefill,sdpa")
    ap.add_argument("--dtype", choices=("bf16", "fp16"), default="bf16")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "training", "varlen_qk_bench_bf16.jsonl"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "varlen_qk_bench.py needs the GPU"
    dtype = torch.bfloat16 if a.dtype == "bf16" else torch.float16
    arms = a.arms.split(",")
    lines = []

    def emit(line):
        lines.append(line)
        print(json.dumps(line), flush=True)
        torch.cuda.empty_cache()

    if "parity" in arms:
        for case, lengths in (("uniform", [4096] * 16), ("mixed", mixed_lengths())):
            for Hkv in (16, 4):
                for causal in (False, True):
                    emit(parity(case, lengths, 16, Hkv, causal, dtype, a.reps))
    if "prefill" in arms:
        for H, Hkv in ((32, 8), (16, 16)):
            for len_k in (8192, 32768):
                for len_q in (512, 2048):
                    emit(prefill(len_q, len_k, 8, H, Hkv, dtype, a.reps, "sdpa" in arms and len_k == 8192))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.writelines(json.dumps(ln) + "\n" for ln in lines)


if __name__ == "__main__":
    main()
