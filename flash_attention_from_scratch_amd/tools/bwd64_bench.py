"""The packed backward at d_head = 64, timing (the sibling of sinks_bench.py): one JSON line per window with, in one
process, alternating, medians of the backward in three arms, every one timed by the launch's own events (timed=True) --
packed causal self-attention, `batch` sequences of `seqlen` tokens (32k tokens), (H, Hkv) = (64, 8), sinks = linspace(4, 7, H):
  - "d64":    backward_varlen_d64 on the d64 tensors and forward_varlen_d64's o and lse;                                        (a)
  - "pad128": backward_varlen_sinks on the same tensors zero-padded to 128 and forward_varlen_sinks's o and lse of those -- the
              only way to serve the shape without this kernel; its softmax scale is 1 / sqrt(128), which timing does not see;  (b)
  - "d64_2":  "d64" a second time: the A/A spread the other ratio is read against.
Beside them "fwd_bwd_ms": attention_varlen_d64(...).backward(dout), forward plus backward through autograd, between two events on
the stream (the autograd call has no timer of its own).  Windows: none, (127, 0) (gpt-oss's local layers) and (1023, 0).  Clocks
are whatever the device runs at.  Written to profiles/training/bwd64_bench_<dtype>.jsonl unless --out says otherwise.

    python flash_attention_from_scratch_amd/tools/bwd64_bench.py [--reps N] [--out FILE]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

H, HKV = 64, 8
WINDOWS = [-1, 127, 1023]   # left; causal (right = 0); -1: no window
ARMS = ("d64", "pad128", "d64_2")


def run(B, S, left, dtype, reps):
    import torch

    import flash_attention
    from flash_attention_from_scratch_amd.tools.decode_bench import _median, _timed

    gen = torch.Generator(device="cuda").manual_seed(0)
    q, dout = (torch.randn((B * S, H, 64), generator=gen, device="cuda").to(dtype) for _ in range(2))
    k, v = (torch.randn((B * S, HKV, 64), generator=gen, device="cuda").to(dtype) for _ in range(2))
    cu = torch.arange(B + 1, dtype=torch.int32, device="cuda") * S
    sinks = torch.linspace(4.0, 7.0, H, device="cuda")
    window = (-1, -1) if left < 0 else (left, 0)
    pad = lambda t: torch.nn.functional.pad(t, (0, 64))   # noqa: E731
    q2, k2, v2, dout2 = pad(q), pad(k), pad(v), pad(dout)
    o, lse = flash_attention.forward_varlen_d64(q, k, v, cu, S, sinks, causal=True, window_size=window)
    o2, lse2 = flash_attention.forward_varlen_sinks(q2, k2, v2, cu, S, sinks, causal=True, window_size=window)

    def backward(name):
        if name == "pad128":
            return flash_attention.backward_varlen_sinks(q2, k2, v2, o2, lse2, dout2, cu, S, sinks, window, causal=True, timed=True)[-1]
        return flash_attention.backward_varlen_d64(q, k, v, o, lse, dout, cu, S, sinks, window, causal=True, timed=True)[-1]

    leaves = [t.clone().requires_grad_(True) for t in (q, k, v)]

    def fwd_bwd():
        flash_attention.attention_varlen_d64(*leaves, cu, S, sinks, causal=True, window_size=window).backward(dout)

    times = {name: [] for name in ARMS + ("fwd_bwd",)}
    for i in range(reps + 2):   # (two warm-up rounds)
        for name in ARMS:
            t = backward(name)
            if i > 1:
                times[name].append(t)
        t = _timed(fwd_bwd)
        if i > 1:
            times["fwd_bwd"].append(t)
    line = {"batch": B, "seqlen": S, "window_left": left, "n_heads": H, "n_kv_heads": HKV, "dtype": str(dtype).replace("torch.", ""),
            "reps": reps}
    line.update({f"{name}_ms": _median(ts) for name, ts in times.items()})
    line["d64_over_pad128"] = line["d64_ms"] / line["pad128_ms"]
    line["d64_2_over_d64"] = line["d64_2_ms"] / line["d64_ms"]
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
        a.out = os.path.join(ROOT, "profiles", "training", f"bwd64_bench_{a.dtype}.jsonl")
    assert torch.cuda.is_available(), "bwd64_bench.py needs the GPU"
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
