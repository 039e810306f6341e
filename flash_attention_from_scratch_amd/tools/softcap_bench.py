"""Logit soft-capping on the varlen forward and backward, timing (the sibling of bwd_window_bench.py): one JSON line per window
with, in one process, alternating, event-timed medians of the forward and of the backward in four arms on the same tensors --
packed causal self-attention, `batch` sequences of `seqlen` tokens (32k tokens), (H, Hkv) = (32, 8), each backward on the o and lse
of its own forward:
  - "cap":     softcap = 50 at the window: fa_fwd_launch_varlen_qk_softcap / fa_bwd_launch_varlen_qk_softcap;
  - "window":  the same call without softcap THROUGH THE WINDOWED ENTRY at the same window -- for (-1, -1) that is left = seqlen,
               the window text with nothing to skip, since (-1, -1) itself takes the unwindowed entry.  cap / window isolates the cap;
  - "plain":   (-1, -1) only: the unwindowed causal entry.  window / plain prices running the window text, which the soft-capped
               kernels always do;
  - "window2": "window" a second time: the A/A spread the other ratios are read against.
Clocks are whatever the device runs at.  Written to profiles/training/softcap_bench_<dtype>.jsonl unless --out says otherwise.

    python flash_attention_from_scratch_amd/tools/softcap_bench.py [--reps N] [--out FILE]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

H, HKV = 32, 8
SOFTCAP = 50.0
WINDOWS = [-1, 1024, 4096]   # left; causal (right = 0); -1: no window


def arms(S, left):
    """-> {arm: (window_size, softcap)} for one window; "plain" only where there is no window"""
    base = (S, 0) if left < 0 else (left, 0)   # (the windowed entry at the same keys)
    out = {"cap": ((-1, -1) if left < 0 else (left, 0), SOFTCAP), "window": (base, 0.0)}
    if left < 0:
        out["plain"] = ((-1, -1), 0.0)
    out["window2"] = (base, 0.0)
    return out


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
    todo = arms(S, left)

    def forward(name):
        window, cap = todo[name]
        return flash_attention.forward_varlen(q, k, v, cu, S, causal=True, window_size=window, softcap=cap)
    fwd = {name: forward(name) for name in todo}

    def backward(name):   # (softcap 0: backward_varlen_window itself; (-1, -1) as well: backward_varlen itself)
        window, cap = todo[name]
        o, lse = fwd[name]
        return flash_attention.backward_varlen_softcap(q, k, v, o, lse, dout, cu, S, cap, window, causal=True)
    times = {(p, name): [] for p in ("fwd", "bwd") for name in todo}
    for i in range(reps + 2):   # (two warm-up rounds)
        for name in todo:
            for p, call in (("fwd", forward), ("bwd", backward)):
                t = _timed(lambda: call(name))
                if i > 1:
                    times[p, name].append(t)
    line = {"batch": B, "seqlen": S, "window_left": left, "softcap": SOFTCAP, "n_heads": H, "n_kv_heads": HKV,
            "dtype": str(dtype).replace("torch.", ""), "reps": reps}
    line.update({f"{p}_{name}_ms": _median(ts) for (p, name), ts in times.items()})
    for p in ("fwd", "bwd"):
        line[f"{p}_cap_over_window"] = line[f"{p}_cap_ms"] / line[f"{p}_window_ms"]
        line[f"{p}_window2_over_window"] = line[f"{p}_window2_ms"] / line[f"{p}_window_ms"]
        if "plain" in todo:
            line[f"{p}_window_over_plain"] = line[f"{p}_window_ms"] / line[f"{p}_plain_ms"]
            line[f"{p}_cap_over_plain"] = line[f"{p}_cap_ms"] / line[f"{p}_plain_ms"]
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
        a.out = os.path.join(ROOT, "profiles", "training", f"softcap_bench_{a.dtype}.jsonl")
    assert torch.cuda.is_available(), "softcap_bench.py needs the GPU"
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
