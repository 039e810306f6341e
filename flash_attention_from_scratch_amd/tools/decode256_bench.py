"""KV-cache decode at d_head = 256, timing (the sibling of decode64_bench.py): one JSON line per case with, in one
process, alternating, medians on (H, Hkv) = (16, 8), seqlen_q 1, causal, every key of a 32k cache valid.  The library's arms are timed
by the launch's own device events around its kernels (timed=True: fa_decode_*_launch's ms); torch's arm has no such clock and is
timed by events around the Python call.
  - "d256":     forward_kvcache_d256 on the d256 cache;                                                                  (a)
  - "d256_2":   the same call a second time: the A/A spread every ratio is read against;
  - "d256_u16", "d256_u32": the same call with the kernel's 16-key and 32-key unit named outright (FA_DECODE256_UNIT), one of which
                is the shipped one: the number behind the choice of unit;
  - "d128":     forward_kvcache_softcap at d_head 128 on a cache of the SAME BYTES (twice the keys, the window twice as long);  (b)
  - "sdpa":     torch's scaled_dot_product_attention on the d256 tensors, the keys the window sees, WITHOUT a cap (it has none:
                under a cap a user's eager path does more than this arm).                                                 (c)
Batch 8 and 64, windows none and (4095, 0), softcap 0 and 50.  Bytes per call are K and V of the keys a row sees.  Clocks are whatever
the device runs at.  The gate: (a) below (c) by more than the A/A spread in every case (exit status 1 otherwise); (a) / (b) and the
cap's cost (cap against no cap at the same batch and window: "cap_over_plain") are reported, not gated.  Written to
profiles/inference/decode256_bench_<dtype>.jsonl unless --out says otherwise.

    python flash_attention_from_scratch_amd/tools/decode256_bench.py [--reps N] [--out FILE]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

H, HKV, CACHE, LEFT, CAP = 16, 8, 32768, 4095, 50.0
CASES = [(batch, left, cap) for batch in (8, 64) for left in (-1, LEFT) for cap in (0.0, CAP)]   # (batch, window left (-1: none), softcap)
ARMS = ("d256", "d128", "d256_2", "d256_u16", "d256_u32", "sdpa")


def run(batch, left, cap, dtype, reps):
    import torch
    import torch.nn.functional as F

    import flash_attention
    from flash_attention_from_scratch_amd.tools.decode_bench import _median, _timed

    gen = torch.Generator(device="cuda").manual_seed(0)
    base = min(batch, 8)   # (a 64-entry cache repeats eight entries' values: the bytes read are what is timed)
    rand = lambda *shape: torch.randn(shape, generator=gen, device="cuda").to(dtype)   # noqa: E731
    k256, v256, k128, v128 = rand(base, CACHE, HKV, 256), rand(base, CACHE, HKV, 256), rand(base, 2 * CACHE, HKV, 128), rand(base, 2 * CACHE, HKV, 128)
    k256, v256, k128, v128 = (t.repeat(batch // base, 1, 1, 1) for t in (k256, v256, k128, v128))
    q256, q128 = rand(batch, 1, H, 256), rand(batch, 1, H, 128)
    lens, double = (torch.full((batch,), n, dtype=torch.int32, device="cuda") for n in (CACHE, 2 * CACHE))
    seen = CACHE if left < 0 else left + 1
    ks, vs = (t[:, CACHE - seen:].transpose(1, 2) for t in (k256, v256))   # (batch, Hkv, keys, 256), a view
    call = dict(causal=True, window_size=(-1, -1) if left < 0 else (left, 0), timed=True)
    call128 = dict(causal=True, window_size=(-1, -1) if left < 0 else (2 * left + 1, 0), timed=True)   # (the same bytes)

    def unit(keys):
        os.environ["FA_DECODE256_UNIT"] = keys
        try:
            return flash_attention.forward_kvcache_d256(q256, k256, v256, lens, cap, **call)[-1]
        finally:
            del os.environ["FA_DECODE256_UNIT"]

    forward = {   # -> ms
        "d256": lambda: flash_attention.forward_kvcache_d256(q256, k256, v256, lens, cap, **call)[-1],
        "d128": lambda: flash_attention.forward_kvcache_softcap(q128, k128, v128, double, cap, **call128)[-1],
        "d256_u16": lambda: unit("16"),
        "d256_u32": lambda: unit("32"),
        "sdpa": lambda: _timed(lambda: F.scaled_dot_product_attention(q256.transpose(1, 2), ks, vs, enable_gqa=True)),
    }
    forward["d256_2"] = forward["d256"]
    arms, sdpa_error = ARMS, None
    try:   # (torch's baseline is reported where this torch has a kernel for the shape; the HIP arms are never skipped)
        forward["sdpa"]()
        torch.cuda.synchronize()
    except Exception as e:   # noqa: BLE001
        arms, sdpa_error = ARMS[:-1], f"{type(e).__name__}: {str(e)[:200]}"
    times = {name: [] for name in arms}
    for i in range(reps + 2):   # (two warm-up rounds)
        for name in arms:
            t = forward[name]()
            if i > 1:
                times[name].append(t)
    line = {"batch": batch, "seqlen_q": 1, "len_k": CACHE, "window_left": left, "softcap": cap, "n_heads": H, "n_kv_heads": HKV,
            "dtype": str(dtype).replace("torch.", ""), "reps": reps}
    line.update({f"{name}_ms": _median(ts) for name, ts in times.items()})
    # K and V of the keys a row sees: 512 bytes a key and tensor in every arm ("d128": twice the keys, half as wide)
    line.update({f"{name}_gbps": 2 * batch * HKV * seen * 512 / (line[f"{name}_ms"] * 1e6) for name in arms})
    for name in arms[1:]:
        line[f"d256_over_{name}"] = line["d256_ms"] / line[f"{name}_ms"]
    if sdpa_error:
        line["sdpa_error"] = sdpa_error
    else:
        line["gate_d256_beats_sdpa"] = line["d256_over_sdpa"] < 1.0 - abs(1.0 - line["d256_over_d256_2"])
    return line


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--dtype", choices=("bf16", "fp16"), default="bf16")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch

    if a.out is None:
        a.out = os.path.join(ROOT, "profiles", "inference", f"decode256_bench_{a.dtype}.jsonl")
    assert torch.cuda.is_available(), "decode256_bench.py needs the GPU"
    dtype = torch.bfloat16 if a.dtype == "bf16" else torch.float16
    lines = []
    for case in CASES:
        lines.append(run(*case, dtype, a.reps))
        if lines[-1]["softcap"]:   # (the case before it is the same batch and window without the cap)
            lines[-1]["cap_over_plain"] = lines[-1]["d256_ms"] / lines[-2]["d256_ms"]
        print(json.dumps(lines[-1]), flush=True)
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "w") as f:
        f.writelines(json.dumps(ln) + "\n" for ln in lines)
    sys.exit(0 if all(ln.get("gate_d256_beats_sdpa", False) for ln in lines) else 1)


if __name__ == "__main__":
    main()
