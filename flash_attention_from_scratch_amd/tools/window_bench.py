"""Sliding-window decode, timing (the sibling of decode_bench.py): one JSON line per case with, in one process, alternating,
event-timed medians of three arms on the same tensors, every key of the cache valid, seqlen_q = 1, (H, Hkv) = (32, 8), all with
the split rule's num_splits:
  - "window": flash_attention.forward_kvcache(window_size=(W, 0)) on the full cache (for one query row right = 0 masks nothing;
              with both sides bounded the split rule counts the window's keys);
  - "full":   the same call without window_size: every key of the cache is streamed (what a caller without the keyword runs,
              masking aside);
  - "only":   the call without window_size on a cache that holds just the W + 1 keys the window sees (the floor: the same
              bytes, no window arithmetic, tiles that start at key 0).
Cases: batch 1, 8, 64 x cache 8k, 64k x W 1024, 4096, contiguous bf16; one case in shuffled 256-row pages and one on the fp8
cache.  `gbps_*` is achieved bytes / s = (the K and V bytes the arm has to read + Q + O) / time -- the window's for "window"
and "only", the cache's for "full".  Clocks are whatever the device runs at.  Written to
profiles/inference/window_bench_<dtype>.jsonl unless --out says otherwise.

    python flash_attention_from_scratch_amd/tools/window_bench.py [--reps N] [--out FILE]
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
from flash_attention_from_scratch_amd import flash_attention_kernels as fak  # noqa: E402
from flash_attention_from_scratch_amd.tools.decode_bench import _median, _quantize, _timed  # noqa: E402

H, HKV, SQ = 32, 8, 1


def run(case, B, cache_len, W, page_size, fp8, dtype, reps):
    gen = torch.Generator(device="cuda").manual_seed(0)
    q = torch.randn((B, SQ, H, 128), generator=gen, device="cuda").to(dtype)
    k = torch.randn((B, cache_len, HKV, 128), generator=gen, device="cuda").to(dtype)
    v = torch.randn((B, cache_len, HKV, 128), generator=gen, device="cuda").to(dtype)
    lens = torch.full((B,), cache_len, dtype=torch.int32, device="cuda")
    seen = W + 1   # the keys one query row sees
    lens_only = torch.full((B,), seen, dtype=torch.int32, device="cuda")
    kw = {}
    if fp8:
        k, v, kd, vd = _quantize(k, v)
        kw.update(k_descale=kd, v_descale=vd)
    k_only, v_only = k[:, cache_len - seen:].contiguous(), v[:, cache_len - seen:].contiguous()
    kw_full = dict(kw)
    if page_size:
        per_seq = cache_len // page_size
        perm = torch.randperm(B * per_seq, generator=torch.Generator().manual_seed(1)).to("cuda")

        def paginate(t):
            out = torch.empty((B * per_seq, page_size, HKV, 128), dtype=t.dtype, device="cuda")
            out[perm] = t.view(B * per_seq, page_size, HKV, 128)
            return out
        k, v = paginate(k), paginate(v)
        kw_full["block_table"] = perm.view(B, per_seq).to(torch.int32)
    window = (W, 0)
    t_w, t_f, t_o = [], [], []
    for i in range(reps + 2):   # (two warm-up rounds)
        t0 = _timed(lambda: flash_attention.forward_kvcache(q, k, v, lens, window_size=window, **kw_full))
        t1 = _timed(lambda: flash_attention.forward_kvcache(q, k, v, lens, **kw_full))
        t2 = _timed(lambda: flash_attention.forward_kvcache(q, k_only, v_only, lens_only, **kw))
        if i > 1:
            t_w.append(t0), t_f.append(t1), t_o.append(t2)
    kv_bytes = (1 if fp8 else 2) * 2 * B * HKV * 128   # K and V, per key
    qo_bytes = 2 * 2 * B * SQ * H * 128
    line = {"case": case, "batch": B, "cache_len": cache_len, "window_left": W, "n_heads": H, "n_kv_heads": HKV, "seqlen_q": SQ,
            "page_size": page_size, "dtype": str(dtype).replace("torch.", ""), "kv_dtype": "fp8_e4m3fn" if fp8 else "16bit", "reps": reps,
            "num_splits_window": fak.kvcache_num_splits(q, k, v, lens, block_table=kw_full.get("block_table"), window_size=window),
            "num_splits_full": fak.kvcache_num_splits(q, k, v, lens, block_table=kw_full.get("block_table")),
            "num_splits_only": fak.kvcache_num_splits(q, k_only, v_only, lens_only),
            "bytes_window": kv_bytes * seen + qo_bytes, "bytes_full": kv_bytes * cache_len + qo_bytes,
            "window_ms": _median(t_w), "full_ms": _median(t_f), "only_ms": _median(t_o)}
    line["gbps_window"] = line["bytes_window"] / (line["window_ms"] * 1e-3) / 1e9
    line["gbps_full"] = line["bytes_full"] / (line["full_ms"] * 1e-3) / 1e9
    line["gbps_only"] = line["bytes_window"] / (line["only_ms"] * 1e-3) / 1e9
    line["window_over_full"] = line["window_ms"] / line["full_ms"]
    line["window_over_only"] = line["window_ms"] / line["only_ms"]
    return line


def cases():
    for B in (1, 8, 64):
        for n in (8192, 65536):
            for W in (1024, 4096):
                yield "uniform", B, n, W, 0, False
    yield "paged", 8, 65536, 4096, 256, False
    yield "fp8", 8, 65536, 4096, 0, True


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--dtype", choices=("bf16", "fp16"), default="bf16")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.out is None:
        a.out = os.path.join(ROOT, "profiles", "inference", f"window_bench_{a.dtype}.jsonl")
    assert torch.cuda.is_available(), "window_bench.py needs the GPU"
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
