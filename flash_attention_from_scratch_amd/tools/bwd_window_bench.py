"""Sliding-window varlen backward, timing (the sibling of prefill_window_bench.py): one JSON line per case with, in one process,
alternating, event-timed medians of four arms on the same tensors -- packed causal self-attention, `batch` sequences of
`seqlen` tokens, (H, Hkv) = (32, 8), each arm on the o and lse of its own forward:
  - "window": flash_attention.backward_varlen_window(causal=True, window_size=(W, 0));
  - "full":   flash_attention.backward_varlen(causal=True): the unwindowed causal backward (the one-range kernels);
  - "whole":  the windowed entry with left >= seqlen: the window code with nothing to skip;
  - "full2":  "full" a second time: the A/A spread the other ratios are read against.
`tile_ratio_dq` and `tile_ratio_dkdv` are visited_tiles(window) / visited_tiles(full) of the two sweep kernels, counted on the
host from the rule (64-key tiles per 128-row Q block; 64-row tiles per 128-key block): the time ratio window_over_full is to be
read beside them.  Clocks are whatever the device runs at.  Written to profiles/training/bwd_window_bench_<dtype>.jsonl unless
--out says otherwise.

    python flash_attention_from_scratch_amd/tools/bwd_window_bench.py [--reps N] [--out FILE]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

H, HKV = 32, 8


def _tiles(lo, hi, n):
    """64-row tiles that hold lo .. hi of 0 .. n - 1"""
    lo, hi = max(lo, 0), min(hi, n - 1)
    return hi // 64 - lo // 64 + 1 if hi >= lo else 0


def visited_tiles(len_q, len_k, left, right):
    """-> (key tiles the dQ kernel visits, row tiles the dK / dV kernel sweeps) for one (sequence, head) under window (left, right),
    -1 = unbounded, causal as right = 0, shift = len_k - len_q: a dQ workgroup with rows r0 .. r1 visits the key tiles of
    r0 + shift - left .. r1 + shift + right, a dK / dV workgroup with keys k0 .. k1 the row tiles of k0 - shift - right ..
    k1 - shift + left (each clamped to the other side's range; an empty range: none)."""
    far = 1 << 30
    left, right = (far if left < 0 else left), (far if right < 0 else right)
    shift = len_k - len_q
    dq = sum(_tiles(r0 + shift - left, min(r0 + 128, len_q) - 1 + shift + right, len_k) for r0 in range(0, len_q, 128))
    dkdv = sum(_tiles(k0 - shift - right, min(k0 + 128, len_k) - 1 - shift + left, len_q) for k0 in range(0, len_k, 128))
    return dq, dkdv


def run(B, S, W, dtype, reps):
    import torch

    import flash_attention
    from flash_attention_from_scratch_amd.tools.decode_bench import _median, _timed

    gen = torch.Generator(device="cuda").manual_seed(0)
    q = torch.randn((B * S, H, 128), generator=gen, device="cuda").to(dtype)
    k = torch.randn((B * S, HKV, 128), generator=gen, device="cuda").to(dtype)
    v = torch.randn((B * S, HKV, 128), generator=gen, device="cuda").to(dtype)
    dout = torch.randn((B * S, H, 128), generator=gen, device="cuda").to(dtype)
    cu = torch.arange(B + 1, dtype=torch.int32, device="cuda") * S
    windows = {"window": (W, 0), "full": (-1, -1), "whole": (S, 0), "full2": (-1, -1)}
    fwd = {name: flash_attention.forward_varlen(q, k, v, cu, S, causal=True, window_size=w) for name, w in windows.items() if name != "full2"}
    fwd["full2"] = fwd["full"]

    def call(name):   # ((-1, -1): backward_varlen itself)
        o, lse = fwd[name]
        return flash_attention.backward_varlen_window(q, k, v, o, lse, dout, cu, S, windows[name], causal=True)
    times = {name: [] for name in windows}
    for i in range(reps + 2):   # (two warm-up rounds)
        for name in windows:
            t = _timed(lambda: call(name))
            if i > 1:
                times[name].append(t)
    t_win, t_full = visited_tiles(S, S, W, 0), visited_tiles(S, S, -1, 0)
    line = {"batch": B, "seqlen": S, "window_left": W, "n_heads": H, "n_kv_heads": HKV, "dtype": str(dtype).replace("torch.", ""),
            "reps": reps, "tiles_window_dq": t_win[0], "tiles_full_dq": t_full[0], "tile_ratio_dq": t_win[0] / t_full[0],
            "tiles_window_dkdv": t_win[1], "tiles_full_dkdv": t_full[1], "tile_ratio_dkdv": t_win[1] / t_full[1]}
    line.update({f"{name}_ms": _median(ts) for name, ts in times.items()})
    line["window_over_full"] = line["window_ms"] / line["full_ms"]
    line["whole_over_full"] = line["whole_ms"] / line["full_ms"]
    line["full2_over_full"] = line["full2_ms"] / line["full_ms"]
    return line


def cases():
    for B, S in ((8, 4096), (4, 8192), (1, 32768)):
        for W in (1024, 4096):
            if W < S:
                yield B, S, W


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--dtype", choices=("bf16", "fp16"), default="bf16")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch

    if a.out is None:
        a.out = os.path.join(ROOT, "profiles", "training", f"bwd_window_bench_{a.dtype}.jsonl")
    assert torch.cuda.is_available(), "bwd_window_bench.py needs the GPU"
    dtype = torch.bfloat16 if a.dtype == "bf16" else torch.float16
    lines = []
    for c in cases():
        lines.append(run(*c, dtype, a.reps))
        print(json.dumps(lines[-1]), flush=True)
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "w") as f:
        f.writelines(json.dumps(ln) + "\n" for ln in lines)


if __name__ == "__main__":
    main()
