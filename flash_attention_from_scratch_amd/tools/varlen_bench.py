"""Packed variable-length sequences, timing (the sibling of gqa_bench.py): one JSON line per (case, Hkv, causal) with, in one
process, alternating, event-timed medians of the varlen forward + LSE and the varlen backward next to the dense path:
  - "uniform": the packed batch 16 x 4096 against forward_ex(..., return_lse=True) + backward on the same (16, 4096, H, 128);
  - "mixed":   lengths drawn once with a fixed seed, 64 .. 8192, about 64 k tokens (the list is in the line), against what a
               user of the dense path must do: pad every sequence to the longest length rounded up to 256 and run it.
               `padded_token_share` is the share of the padded batch's tokens that are padding.
Kernel times of their own: run it under `rocprofv3 --kernel-trace --stats -- python .../varlen_bench.py`.

    python flash_attention_from_scratch_amd/tools/varlen_bench.py [--reps N] [--kv-heads 16,4] [--out FILE]
"""
import argparse
import json
import os
import random
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402

import flash_attention  # noqa: E402
from flash_helpers import kernel_configs as kc  # noqa: E402

H = 16


def _median(x):
    return sorted(x)[len(x) // 2]


def mixed_lengths(seed=0, total=65536):
    rng = random.Random(seed)
    out = []
    while sum(out) < total - 8192:
        out.append(rng.randint(64, 8192))
    return out


def run(case, lengths, Hkv, causal, dtype, reps):
    gen = torch.Generator().manual_seed(0)
    T, n, S = sum(lengths), len(lengths), (max(lengths) + 255) // 256 * 256
    q, dout = (torch.randn((T, H, 128), generator=gen).to(dtype).cuda() for _ in range(2))
    k, v = (torch.randn((T, Hkv, 128), generator=gen).to(dtype).cuda() for _ in range(2))
    cu = torch.tensor([0] + [sum(lengths[:i + 1]) for i in range(n)], dtype=torch.int32).cuda()
    qd, doutd = (torch.randn((n, S, H, 128), generator=gen).to(dtype).cuda() for _ in range(2))   # the dense (padded) batch
    kd, vd = (torch.randn((n, S, Hkv, 128), generator=gen).to(dtype).cuda() for _ in range(2))
    cfg = kc.best_config(kc.DType.BF16 if dtype == torch.bfloat16 else kc.DType.FP16, S, masked=causal)
    f_v, b_v, f_d, b_d = [], [], [], []
    for i in range(reps + 2):   # (two warm-up rounds)
        o, lse, t0 = flash_attention.forward_varlen(q, k, v, cu, max(lengths), causal=causal, timed=True)
        od, lsed, t1 = flash_attention.forward_ex(cfg, qd, kd, vd, causal=causal, timed=True, return_lse=True)
        *_, t2 = flash_attention.backward_varlen(q, k, v, o, lse, dout, cu, max(lengths), causal=causal, timed=True)
        *_, t3 = flash_attention.backward(qd, kd, vd, od, lsed, doutd, causal=causal, timed=True)
        if i > 1:
            f_v.append(t0), f_d.append(t1), b_v.append(t2), b_d.append(t3)
    line = {"case": case, "n_seqs": n, "total_tokens": T, "dense_shape": [n, S, H, 128], "n_heads": H, "n_kv_heads": Hkv,
            "dtype": str(dtype).replace("torch.", ""), "causal": causal, "reps": reps,
            "varlen_fwd_lse_ms": _median(f_v), "dense_fwd_lse_ms": _median(f_d), "varlen_bwd_ms": _median(b_v), "dense_bwd_ms": _median(b_d),
            "padded_token_share": 1.0 - T / (n * S)}
    line["fwd_varlen_over_dense"] = line["varlen_fwd_lse_ms"] / line["dense_fwd_lse_ms"]
    line["bwd_varlen_over_dense"] = line["varlen_bwd_ms"] / line["dense_bwd_ms"]
    line["fwd_bwd_varlen_over_dense"] = (line["varlen_fwd_lse_ms"] + line["varlen_bwd_ms"]) / (line["dense_fwd_lse_ms"] + line["dense_bwd_ms"])
    if case == "mixed":
        line["lengths"] = lengths
    return line


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--kv-heads", default="16,4")
    ap.add_argument("--dtype", choices=("bf16", "fp16"), default="bf16")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "training", "varlen_bench_bf16.jsonl"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "varlen_bench.py needs the GPU"
    dtype = torch.bfloat16 if a.dtype == "bf16" else torch.float16
    lines = []
    for case, lengths in (("uniform", [4096] * 16), ("mixed", mixed_lengths())):
        for Hkv in (int(x) for x in a.kv_heads.split(",")):
            for causal in (False, True):
                lines.append(run(case, lengths, Hkv, causal, dtype, a.reps))
                print(json.dumps(lines[-1]), flush=True)
                torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.writelines(json.dumps(ln) + "\n" for ln in lines)


if __name__ == "__main__":
    main()
