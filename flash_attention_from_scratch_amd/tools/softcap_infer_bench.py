"""Logit soft-capping on the inference path, timing (the sibling of softcap_bench.py): one JSON line per case with, in one process,
alternating, event-timed medians of four arms on the same tensors, (H, Hkv) = (32, 8), causal, every key of the cache valid:
  - "cap":     softcap = 50 at the window: forward_kvcache_softcap / forward_varlen_kvcache(softcap=);
  - "window":  the same call without softcap THROUGH THE WINDOWED ENTRY at the same window -- for no window that is left = the cache's
               length, the window text with nothing to skip, since (-1, -1) itself takes the unwindowed entry.  cap / window isolates
               the cap;
  - "plain":   no window only: the unwindowed entry.  window / plain prices running the window text, which the soft-capped kernels
               always do;
  - "window2": "window" a second time: the A/A spread the other ratios are read against.
Decode: seqlen_q 1, batch 8 and 64 against a 64k cache, windows none and (4096, 0), 16-bit and fp8 cache, and one row on shuffled
256-row pages.  Prefill: prefill_window_bench.py's chunk of 2048 query rows behind a 64k prefix, both caches.  Clocks are whatever
the device runs at.  Written to profiles/inference/softcap_infer_bench_<dtype>.jsonl unless --out says otherwise.

    python flash_attention_from_scratch_amd/tools/softcap_infer_bench.py [--reps N] [--out FILE]
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
CACHE = 65536
CHUNK = 2048
# (call, batch, window left (-1: none), fp8 cache, paged)
CASES = [("decode", batch, left, fp8, False) for fp8 in (False, True) for batch in (8, 64) for left in (-1, 4096)]
CASES += [("decode", 8, 4096, False, True)]
CASES += [("prefill", 1, left, fp8, False) for fp8 in (False, True) for left in (-1, 4096)]


def arms(len_k, left):
    """-> {arm: (window_size, softcap)} for one window; "plain" only where there is no window"""
    base = (len_k, 0) if left < 0 else (left, 0)   # (the windowed entry at the same keys)
    out = {"cap": ((-1, -1) if left < 0 else (left, 0), SOFTCAP), "window": (base, 0.0)}
    if left < 0:
        out["plain"] = ((-1, -1), 0.0)
    out["window2"] = (base, 0.0)
    return out


def run(call, batch, left, fp8, paged, dtype, reps):
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
    k, v = (t.view(torch.uint8) if fp8 else t for t in (k, v))   # (an fp8 cache is moved around as bytes)
    k, v = k.repeat(batch // base, 1, 1, 1), v.repeat(batch // base, 1, 1, 1)
    if paged:
        page = 256
        perm = torch.randperm(batch * len_k // page, generator=torch.Generator().manual_seed(1))
        pages = lambda t: t.reshape(-1, page, HKV, 128)[torch.argsort(perm).cuda()]   # noqa: E731  (entry b's page p lies at perm[b, p])
        k, v = pages(k), pages(v)
        kw["block_table"] = perm.view(batch, -1).to(torch.int32).cuda()
    k, v = k.view(kv_dtype), v.view(kv_dtype)
    lens = torch.full((batch,), len_k, dtype=torch.int32, device="cuda")
    todo = arms(len_k, left)
    if call == "decode":
        q = torch.randn((batch, 1, H, 128), generator=gen, device="cuda").to(dtype)

        def forward(name):
            window, cap = todo[name]
            return flash_attention.forward_kvcache_softcap(q, k, v, lens, cap, causal=True, window_size=window, **kw)
    else:
        q = torch.randn((batch * CHUNK, H, 128), generator=gen, device="cuda").to(dtype)
        cu = torch.arange(batch + 1, dtype=torch.int32, device="cuda") * CHUNK

        def forward(name):
            window, cap = todo[name]
            return flash_attention.forward_varlen_kvcache(q, k, v, cu, CHUNK, lens, causal=True, window_size=window, softcap=cap, **kw)
    times = {name: [] for name in todo}
    for i in range(reps + 2):   # (two warm-up rounds)
        for name in todo:
            t = _timed(lambda: forward(name))
            if i > 1:
                times[name].append(t)
    line = {"call": call, "batch": batch, "seqlen_q": n_q, "len_k": len_k, "window_left": left, "kv_dtype": "fp8" if fp8 else "16bit",
            "paged": paged, "softcap": SOFTCAP, "n_heads": H, "n_kv_heads": HKV, "dtype": str(dtype).replace("torch.", ""), "reps": reps}
    line.update({f"{name}_ms": _median(ts) for name, ts in times.items()})
    line["cap_over_window"] = line["cap_ms"] / line["window_ms"]
    line["window2_over_window"] = line["window2_ms"] / line["window_ms"]
    if "plain" in todo:
        line["window_over_plain"] = line["window_ms"] / line["plain_ms"]
        line["cap_over_plain"] = line["cap_ms"] / line["plain_ms"]
    return line


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--dtype", choices=("bf16", "fp16"), default="bf16")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch

    if a.out is None:
        a.out = os.path.join(ROOT, "profiles", "inference", f"softcap_infer_bench_{a.dtype}.jsonl")
    assert torch.cuda.is_available(), "softcap_infer_bench.py needs the GPU"
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
