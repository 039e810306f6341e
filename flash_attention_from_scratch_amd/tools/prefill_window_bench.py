"""Sliding-window prefill against a KV cache, timing (the sibling of window_bench.py and prefill_bench.py): one JSON line per case
with, in one process, alternating, event-timed medians of four arms on the same tensors -- a chunk of `chunk` query rows per
sequence behind a cached prefix (len_k = prefix + chunk, every one of them valid), (H, Hkv) = (32, 8), causal:
  - "window": flash_attention.forward_varlen_kvcache(causal=True, window_size=(W, 0));
  - "full":   the same call without window_size: every Q block walks down to key 0 (what a caller without the keyword runs);
  - "whole":  the windowed entry with left >= len_k: the window code with nothing to skip;
  - "full2":  "full" a second time: the A/A spread the other ratios are read against.
Cases: chunk 512, 2048 x prefix 8k, 64k x W 1024, 4096 x batch 1, 8, contiguous and in shuffled 256-row pages; --kv-dtype fp8 runs
them on the e4m3fn cache.  `tile_ratio` is visited_tiles(window) / visited_tiles(full), counted on the host from the rule (64-key
tiles per 128-row Q block): the time ratio window_over_full is to be read beside it.  Clocks are whatever the device runs at.
Written to profiles/inference/prefill_window_bench_<kv>.jsonl unless --out says otherwise.

    python flash_attention_from_scratch_amd/tools/prefill_window_bench.py [--kv-dtype fp8] [--reps N] [--out FILE]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

H, HKV = 32, 8


def visited_tiles(len_q, len_k, left, right):
    """64-key tiles the Q blocks (128 rows each) of one (sequence, head) visit under window (left, right), -1 = unbounded, causal as
    right = 0: block rows r0 .. r1 at positions p = r + len_k - len_q walk from tile min(len_k - 1, p_r1 + right) / 64 down to tile
    max(0, p_r0 - left) / 64; a block whose last row sees no key visits none."""
    tiles = 0
    for r0 in range(0, len_q, 128):
        r1 = min(r0 + 128, len_q) - 1
        hi = len_k - 1 if right < 0 else min(len_k - 1, r1 + len_k - len_q + right)
        lo = 0 if left < 0 else max(0, r0 + len_k - len_q - left)
        if hi >= 0:
            tiles += hi // 64 - lo // 64 + 1
    return tiles


def run(case, B, chunk, prefix, W, page_size, fp8, dtype, reps):
    import torch

    import flash_attention
    from flash_attention_from_scratch_amd.tools.decode_bench import _median, _quantize, _timed

    len_k = prefix + chunk
    gen = torch.Generator(device="cuda").manual_seed(0)
    q = torch.randn((B * chunk, H, 128), generator=gen, device="cuda").to(dtype)
    k = torch.randn((B, len_k, HKV, 128), generator=gen, device="cuda").to(dtype)
    v = torch.randn((B, len_k, HKV, 128), generator=gen, device="cuda").to(dtype)
    cuq = torch.arange(B + 1, dtype=torch.int32, device="cuda") * chunk
    lens = torch.full((B,), len_k, dtype=torch.int32, device="cuda")
    kw = {}
    if fp8:
        k, v, kd, vd = _quantize(k, v)
        kw.update(k_descale=kd, v_descale=vd)
    if page_size:
        per_seq = len_k // page_size
        perm = torch.randperm(B * per_seq, generator=torch.Generator().manual_seed(1)).to("cuda")

        def paginate(t):
            out = torch.empty((B * per_seq, page_size, HKV, 128), dtype=t.dtype, device="cuda")
            out[perm] = t.view(B * per_seq, page_size, HKV, 128)
            return out
        k, v = paginate(k), paginate(v)
        kw["block_table"] = perm.view(B, per_seq).to(torch.int32)

    def call(**window):
        return flash_attention.forward_varlen_kvcache(q, k, v, cuq, chunk, lens, causal=True, **kw, **window)
    arms = {"window": dict(window_size=(W, 0)), "full": {}, "whole": dict(window_size=(len_k, 0)), "full2": {}}
    times = {name: [] for name in arms}
    for i in range(reps + 2):   # (two warm-up rounds)
        for name, window in arms.items():
            t = _timed(lambda: call(**window))
            if i > 1:
                times[name].append(t)
    t_win, t_full = visited_tiles(chunk, len_k, W, 0), visited_tiles(chunk, len_k, -1, 0)
    line = {"case": case, "batch": B, "chunk": chunk, "prefix": prefix, "len_k": len_k, "window_left": W, "n_heads": H, "n_kv_heads": HKV,
            "page_size": page_size, "dtype": str(dtype).replace("torch.", ""), "kv_dtype": "fp8_e4m3fn" if fp8 else "16bit", "reps": reps,
            "tiles_window": t_win, "tiles_full": t_full, "tile_ratio": t_win / t_full}
    line.update({f"{name}_ms": _median(ts) for name, ts in times.items()})
    line["window_over_full"] = line["window_ms"] / line["full_ms"]
    line["whole_over_full"] = line["whole_ms"] / line["full_ms"]
    line["full2_over_full"] = line["full2_ms"] / line["full_ms"]
    return line


def cases():
    for page_size in (0, 256):
        for B in (1, 8):
            for prefix in (8192, 65536):
                for chunk in (512, 2048):
                    for W in (1024, 4096):
                        yield ("paged" if page_size else "contiguous"), B, chunk, prefix, W, page_size


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--dtype", choices=("bf16", "fp16"), default="bf16")
    ap.add_argument("--kv-dtype", choices=("16bit", "fp8"), default="16bit")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch

    fp8 = a.kv_dtype == "fp8"
    if a.out is None:
        a.out = os.path.join(ROOT, "profiles", "inference", f"prefill_window_bench_{'fp8' if fp8 else a.dtype}.jsonl")
    assert torch.cuda.is_available(), "prefill_window_bench.py needs the GPU"
    dtype = torch.bfloat16 if a.dtype == "bf16" else torch.float16
    lines = []
    for c in cases():
        lines.append(run(*c, fp8, dtype, a.reps))
        print(json.dumps(lines[-1]), flush=True)
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "w") as f:
        f.writelines(json.dumps(ln) + "\n" for ln in lines)


if __name__ == "__main__":
    main()
