"""Attention sinks on the inference path, timing (the sibling of softcap_infer_bench.py): one JSON line per case with, in one
process, alternating, event-timed medians of three arms on the same tensors, (H, Hkv) = (32, 8), causal, every key of the cache valid:
  - "sinks":   forward_kvcache_sinks / forward_varlen_kvcache_sinks at the window, sinks = linspace(4, 7);
  - "window":  the same call without sinks THROUGH THE WINDOWED ENTRY at the same window -- for no window that is left = the cache's
               length, the window text with nothing to skip, since (-1, -1) itself takes the unwindowed entry.  sinks / window
               isolates the sink;
  - "window2": "window" a second time: the A/A spread the ratio is read against.
Decode: seqlen_q 1, batch 8 and 64 against a 64k cache, windows none and (127, 0), 16-bit and fp8 cache.  Prefill: a chunk of 2048
query rows behind a 64k prefix, the same windows, both caches.  Clocks are whatever the device runs at.  Written to
profiles/inference/sinks_infer_bench_<dtype>.jsonl unless --out says otherwise.

    python flash_attention_from_scratch_amd/tools/sinks_infer_bench.py [--reps N] [--out FILE]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

H, HKV = 32, 8
CACHE = 65536
CHUNK = 2048
LEFT = 127
# (call, batch, window left (-1: none), fp8 cache)
CASES = [("decode", batch, left, fp8) for fp8 in (False, True) for batch in (8, 64) for left in (-1, LEFT)]
CASES += [("prefill", 1, left, fp8) for fp8 in (False, True) for left in (-1, LEFT)]
ARMS = ("sinks", "window", "window2")


def run(call, batch, left, fp8, dtype, reps):
    import torch

    import flash_attention
    from flash_attention_from_scratch_amd.tools.decode_bench import _median, _quantize, _timed

    gen = torch.Generator(device="cuda").manual_seed(0)
    n_q = 1 if call == "decode" else CHUNK
    len_k = CACHE if call == "decode" else CACHE + CHUNK
    base = min(batch, 8)   # (a 64-entry cache repeats eight entries' values: the bytes read are what is timed)
    k = torch.randn((base, len_k, HKV, 128), generator=gen, device="cuda").to(dtype)
    v = torch.randn((base, len_k, HKV, 128), generator=gen, device="cuda").to(dtype)
    kw = {}
    if fp8:
        k, v, kd, vd = _quantize(k, v)
        kw = dict(k_descale=kd.repeat(batch // base, 1), v_descale=vd.repeat(batch // base, 1))
    kv_dtype = k.dtype
    k, v = (t.view(torch.uint8).repeat(batch // base, 1, 1, 1).view(kv_dtype) for t in (k, v))   # (an fp8 cache is moved around as bytes)
    lens = torch.full((batch,), len_k, dtype=torch.int32, device="cuda")
    sinks = torch.linspace(4.0, 7.0, H, device="cuda")
    sunk_window = (-1, -1) if left < 0 else (left, 0)
    plain_window = (len_k, 0) if left < 0 else (left, 0)   # (the windowed entry at the same keys)
    if call == "decode":
        q = torch.randn((batch, 1, H, 128), generator=gen, device="cuda").to(dtype)

        def forward(name):
            if name == "sinks":
                return flash_attention.forward_kvcache_sinks(q, k, v, lens, sinks, causal=True, window_size=sunk_window, **kw)
            return flash_attention.forward_kvcache(q, k, v, lens, causal=True, window_size=plain_window, **kw)
    else:
        q = torch.randn((batch * CHUNK, H, 128), generator=gen, device="cuda").to(dtype)
        cu = torch.arange(batch + 1, dtype=torch.int32, device="cuda") * CHUNK

        def forward(name):
            if name == "sinks":
                return flash_attention.forward_varlen_kvcache_sinks(q, k, v, cu, CHUNK, lens, sinks, causal=True, window_size=sunk_window, **kw)
            return flash_attention.forward_varlen_kvcache(q, k, v, cu, CHUNK, lens, causal=True, window_size=plain_window, **kw)
    times = {name: [] for name in ARMS}
    for i in range(reps + 2):   # (two warm-up rounds)
        for name in ARMS:
            t = _timed(lambda: forward(name))
            if i > 1:
                times[name].append(t)
    line = {"call": call, "batch": batch, "seqlen_q": n_q, "len_k": len_k, "window_left": left, "kv_dtype": "fp8" if fp8 else "16bit",
            "n_heads": H, "n_kv_heads": HKV, "dtype": str(dtype).replace("torch.", ""), "reps": reps}
    line.update({f"{name}_ms": _median(ts) for name, ts in times.items()})
    line["sinks_over_window"] = line["sinks_ms"] / line["window_ms"]
    line["window2_over_window"] = line["window2_ms"] / line["window_ms"]
    return line


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--dtype", choices=("bf16", "fp16"), default="bf16")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch

    if a.out is None:
        a.out = os.path.join(ROOT, "profiles", "inference", f"sinks_infer_bench_{a.dtype}.jsonl")
    assert torch.cuda.is_available(), "sinks_infer_bench.py needs the GPU"
    dtype = torch.bfloat16 if a.dtype == "bf16" else torch.float16
    lines = []
    for case in CASES:
        lines.append(run(*case, dtype, a.reps))
        print(json.dumps(lines[-1]), flush=True)
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "w") as f:
        f.writelines(json.dumps(ln) + "\n" for ln in lines)


if __name__ == "__main__":
    main()
