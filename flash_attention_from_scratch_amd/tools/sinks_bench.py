"""Learned attention sinks on the varlen forward and backward, timing (the sibling of softcap_bench.py): one JSON line per window
with, in one process, alternating, event-timed medians of the forward and of the backward in three arms on the same tensors --
packed causal self-attention, `batch` sequences of `seqlen` tokens (32k tokens), (H, Hkv) = (32, 8), each backward on the o and lse
of its own forward:
  - "sinks":   fa_fwd_launch_varlen_qk_sinks / fa_bwd_launch_varlen_qk_sinks at the window, sinks = linspace(4, 7, H);
  - "window":  the same call without sinks THROUGH THE WINDOWED ENTRY at the same window -- for no window that is left = seqlen,
               the window text with nothing to skip, since (-1, -1) itself takes the unwindowed entry.  sinks / window isolates the
               sinks: the forward's item end, and in the backward the dsinks kernel (dQ, dK, dV are the window form's kernels);
  - "window2": "window" a second time: the A/A spread the other ratio is read against.
Windows: none, (127, 0) (gpt-oss's local layers) and (1023, 0).  Clocks are whatever the device runs at.  Written to
profiles/training/sinks_bench_<dtype>.jsonl unless --out says otherwise.

    python flash_attention_from_scratch_amd/tools/sinks_bench.py [--reps N] [--out FILE]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

H, HKV = 32, 8
WINDOWS = [-1, 127, 1023]   # left; causal (right = 0); -1: no window
ARMS = ("sinks", "window", "window2")


def run(B, S, left, dtype, reps):
    import torch

    import flash_attention
    from flash_attention_from_scratch_amd.tools.decode_bench import _median, _timed

    gen = torch.Generator(device="cuda").manual_seed(0)
    q = torch.randn((B * S, H, 128), generator=gen, device="cuda").to(dtype)
    k = torch.randn((B * S, HKV, 128), generator=gen, device="cuda").to(dtype)
    v = torch.randn((B * S, HKV, 128), generator=gen, device="cuda").to(dtype)
    dout = torch.randn((B * S, H, 128), generator=gen, device="cuda").to(dtype)
    cu = torch.arange(B + 1, dtype=torch.int32, device="cuda") * S
    sinks = torch.linspace(4.0, 7.0, H, device="cuda")
    with_sinks = (-1, -1) if left < 0 else (left, 0)
    windowed = (S, 0) if left < 0 else (left, 0)   # (the windowed entry at the same keys)

    def forward(name):
        if name == "sinks":
            return flash_attention.forward_varlen_sinks(q, k, v, cu, S, sinks, causal=True, window_size=with_sinks)
        return flash_attention.forward_varlen(q, k, v, cu, S, causal=True, window_size=windowed)
    fwd = {name: forward(name) for name in ARMS}

    def backward(name):
        o, lse = fwd[name]
        if name == "sinks":
            return flash_attention.backward_varlen_sinks(q, k, v, o, lse, dout, cu, S, sinks, with_sinks, causal=True)
        return flash_attention.backward_varlen_window(q, k, v, o, lse, dout, cu, S, windowed, causal=True)
    times = {(p, name): [] for p in ("fwd", "bwd") for name in ARMS}
    for i in range(reps + 2):   # (two warm-up rounds)
        for name in ARMS:
            for p, call in (("fwd", forward), ("bwd", backward)):
                t = _timed(lambda: call(name))
                if i > 1:
                    times[p, name].append(t)
    line = {"batch": B, "seqlen": S, "window_left": left, "n_heads": H, "n_kv_heads": HKV, "dtype": str(dtype).replace("torch.", ""),
            "reps": reps}
    line.update({f"{p}_{name}_ms": _median(ts) for (p, name), ts in times.items()})
    for p in ("fwd", "bwd"):
        line[f"{p}_sinks_over_window"] = line[f"{p}_sinks_ms"] / line[f"{p}_window_ms"]
        line[f"{p}_window2_over_window"] = line[f"{p}_window2_ms"] / line[f"{p}_window_ms"]
    return line


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--dtype", choices=("bf16", "fp16"), default="bf16")
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--seqlen", type=int, default=8192)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch

    if a.out is None:
        a.out = os.path.join(ROOT, "profiles", "training", f"sinks_bench_{a.dtype}.jsonl")
    assert torch.cuda.is_available(), "sinks_bench.py needs the GPU"
    dtype = torch.bfloat16 if a.dtype == "bf16" else torch.float16
    lines = []
    for left in WINDOWS:
        lines.append(run(a.batch, a.seqlen, left, dtype, a.reps))
        print(json.dumps(lines[-1]), flush=True)
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "w") as f:
        f.writelines(json.dumps(ln) + "\n" for ln in lines)


if __name__ == "__main__":
    main()
