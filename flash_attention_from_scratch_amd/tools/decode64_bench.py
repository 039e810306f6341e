"""KV-cache decode at d_head = 64, timing (the sibling of sinks_infer_bench.py): one JSON line per case with, in one
process, alternating, medians on (H, Hkv) = (64, 8), seqlen_q 1, causal, every key of a 64k cache valid, sinks = linspace(4, 7).
The library's arms are timed by the launch's own device events around its kernels (timed=True: fa_decode_*_launch's ms), so a
launch of a few microseconds is not buried under the Python call's fixed 30 us; torch's arm has no such clock and is timed by
events around the Python call.
  - "d64":     forward_kvcache_d64 on the d64 cache;                                                        (a)
  - "d64_2":   the same call a second time: the A/A spread every ratio is read against;
  - "d64_u32", "d64_u64": the same call with the kernel's 32-key and 64-key unit named outright (FA_DECODE64_UNIT), one of which is
               the shipped one: the number behind the choice of unit;
  - "d128":    forward_kvcache_sinks at d_head 128 on a cache of the SAME BYTES (half the keys);            (b)
  - "padded":  forward_kvcache_sinks on the same keys zero-padded to 128 (twice the bytes, and the softmax scale of 128: what a
               caller could do without this kernel -- timed, not a result anyone wants);                     (c)
  - "sdpa":    torch's scaled_dot_product_attention on the d64 tensors, the keys the window sees, no sinks (it has none).   (d)
Batch 8 and 64, windows none and (127, 0).  Bytes per call are K and V of the keys a row sees; achieved bytes/s follow from the
shapes where the cache streams (under the window a launch moves 128 keys a row: its time is no bandwidth, and none is given).  Clocks are whatever the device runs at.  The gate: (a) beats (c) by more than the A/A spread in every case (exit status 1
otherwise).  Written to profiles/inference/decode64_bench_<dtype>.jsonl unless --out says otherwise.

    python flash_attention_from_scratch_amd/tools/decode64_bench.py [--reps N] [--out FILE]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

H, HKV, CACHE, LEFT = 64, 8, 65536, 127
CASES = [(batch, left) for batch in (8, 64) for left in (-1, LEFT)]   # (batch, window left (-1: none))
ARMS = ("d64", "d128", "padded", "d64_2", "d64_u32", "d64_u64", "sdpa")


def run(batch, left, dtype, reps):
    import torch
    import torch.nn.functional as F

    import flash_attention
    from flash_attention_from_scratch_amd.tools.decode_bench import _median, _timed

    gen = torch.Generator(device="cuda").manual_seed(0)
    base = min(batch, 8)   # (a 64-entry cache repeats eight entries' values: the bytes read are what is timed)
    rand = lambda *shape: torch.randn(shape, generator=gen, device="cuda").to(dtype)   # noqa: E731
    k64, v64, k128, v128 = rand(base, CACHE, HKV, 64), rand(base, CACHE, HKV, 64), rand(base, CACHE // 2, HKV, 128), rand(base, CACHE // 2, HKV, 128)
    k64, v64, k128, v128 = (t.repeat(batch // base, 1, 1, 1) for t in (k64, v64, k128, v128))
    kpad, vpad = (F.pad(t, (0, 64)) for t in (k64, v64))
    q64, q128 = rand(batch, 1, H, 64), rand(batch, 1, H, 128)
    qpad = F.pad(q64, (0, 64))
    lens, half = (torch.full((batch,), n, dtype=torch.int32, device="cuda") for n in (CACHE, CACHE // 2))
    sinks = torch.linspace(4.0, 7.0, H, device="cuda")
    window = (-1, -1) if left < 0 else (left, 0)
    seen = CACHE if left < 0 else left + 1
    ks, vs = (t[:, CACHE - seen:].transpose(1, 2) for t in (k64, v64))   # (batch, Hkv, keys, 64), a view
    call = dict(causal=True, window_size=window, timed=True)

    def unit(keys):
        os.environ["FA_DECODE64_UNIT"] = keys
        try:
            return flash_attention.forward_kvcache_d64(q64, k64, v64, lens, sinks, **call)[-1]
        finally:
            del os.environ["FA_DECODE64_UNIT"]

    forward = {   # -> ms
        "d64": lambda: flash_attention.forward_kvcache_d64(q64, k64, v64, lens, sinks, **call)[-1],
        "d128": lambda: flash_attention.forward_kvcache_sinks(q128, k128, v128, half, sinks, **call)[-1],
        "padded": lambda: flash_attention.forward_kvcache_sinks(qpad, kpad, vpad, lens, sinks, **call)[-1],
        "d64_u32": lambda: unit("32"),
        "d64_u64": lambda: unit("64"),
        "sdpa": lambda: _timed(lambda: F.scaled_dot_product_attention(q64.transpose(1, 2), ks, vs, enable_gqa=True)),
    }
    forward["d64_2"] = forward["d64"]
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
    line = {"batch": batch, "seqlen_q": 1, "len_k": CACHE, "window_left": left, "n_heads": H, "n_kv_heads": HKV,
            "dtype": str(dtype).replace("torch.", ""), "reps": reps}
    line.update({f"{name}_ms": _median(ts) for name, ts in times.items()})
    # K and V of the keys a row sees, in the arm's own layout ("d128" without a window: half the keys, twice as wide)
    seen128 = CACHE // 2 if left < 0 else seen
    nbytes = {"d64": seen * 64, "d64_u32": seen * 64, "d64_u64": seen * 64, "d128": seen128 * 128, "padded": seen * 128, "sdpa": seen * 64}
    if left < 0:
        line.update({f"{name}_gbps": 2 * 2 * batch * HKV * n / (line[f"{name}_ms"] * 1e6) for name, n in nbytes.items() if name in arms})
    for name in arms[1:]:
        line[f"d64_over_{name}"] = line["d64_ms"] / line[f"{name}_ms"]
    if sdpa_error:
        line["sdpa_error"] = sdpa_error
    line["gate_d64_beats_padded"] = line["d64_over_padded"] < 1.0 - abs(1.0 - line["d64_over_d64_2"])
    return line


FP8_FORMS = (("32", "1"), ("32", "2"), ("64", "1"))   # (FA_DECODE64_UNIT, FA_DECODE64_AHEAD): the fp8 kernel's instantiated forms
FP8_ARMS = ("d64", "fp8", "d64_2", "fp8_2") + tuple(f"fp8_u{u}a{d}" for u, d in FP8_FORMS)


def run_fp8(batch, left, dtype, reps):
    """--kv-dtype fp8: the fp8 call ("fp8": the shipped form; "fp8_u<unit>a<ahead>": each form named outright)
    against the 16-bit d64 call ("d64") on the cache it was quantized from, A/A beside both, same process, alternating, medians of
    the launch's own ms.  Bytes: K and V of the keys a row sees, one byte an element for fp8, two for 16-bit."""
    import torch

    import flash_attention
    from flash_attention_from_scratch_amd.tools.decode_bench import _median

    gen = torch.Generator(device="cuda").manual_seed(0)
    base = min(batch, 8)
    rand = lambda *shape: torch.randn(shape, generator=gen, device="cuda").to(dtype)   # noqa: E731
    k16, v16, q = rand(base, CACHE, HKV, 64), rand(base, CACHE, HKV, 64), rand(batch, 1, H, 64)
    k8, v8, kd, vd = flash_attention.quantize_kvcache_fp8(k16, v16)
    k8, v8 = k8.view(torch.uint8), v8.view(torch.uint8)   # (repeated as bytes)
    k16, v16, k8, v8, kd, vd = (t.repeat(batch // base, *([1] * (t.dim() - 1))).contiguous() for t in (k16, v16, k8, v8, kd, vd))
    k8, v8 = k8.view(torch.float8_e4m3fn), v8.view(torch.float8_e4m3fn)
    lens = torch.full((batch,), CACHE, dtype=torch.int32, device="cuda")
    sinks = torch.linspace(4.0, 7.0, H, device="cuda")
    call = dict(causal=True, window_size=(-1, -1) if left < 0 else (left, 0), timed=True)
    seen = CACHE if left < 0 else left + 1

    def fp8(form=None):
        os.environ.update(dict(zip(("FA_DECODE64_UNIT", "FA_DECODE64_AHEAD"), form)) if form else {})
        try:
            return flash_attention.forward_kvcache_d64(q, k8, v8, lens, sinks, k_descale=kd, v_descale=vd, **call)[-1]
        finally:
            for name in ("FA_DECODE64_UNIT", "FA_DECODE64_AHEAD") if form else ():
                del os.environ[name]

    forward = {"d64": lambda: flash_attention.forward_kvcache_d64(q, k16, v16, lens, sinks, **call)[-1], "fp8": fp8}
    forward.update({"d64_2": forward["d64"], "fp8_2": fp8}, **{f"fp8_u{u}a{d}": (lambda form=(u, d): fp8(form)) for u, d in FP8_FORMS})
    times = {name: [] for name in FP8_ARMS}
    for i in range(reps + 2):   # (two warm-up rounds)
        for name in FP8_ARMS:
            t = forward[name]()
            if i > 1:
                times[name].append(t)
    line = {"kv_dtype": "fp8_e4m3fn", "batch": batch, "seqlen_q": 1, "len_k": CACHE, "window_left": left, "n_heads": H, "n_kv_heads": HKV,
            "dtype": str(dtype).replace("torch.", ""), "reps": reps}
    line.update({f"{name}_ms": _median(ts) for name, ts in times.items()})
    if left < 0:
        line.update({f"{name}_gbps": 2 * (2 if name.startswith("d64") else 1) * batch * HKV * seen * 64 / (line[f"{name}_ms"] * 1e6) for name in FP8_ARMS})
    line.update({f"{name}_over_d64": line[f"{name}_ms"] / line["d64_ms"] for name in FP8_ARMS[1:]})
    line["fp8_over_fp8_2"] = line["fp8_ms"] / line["fp8_2_ms"]
    return line


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--dtype", choices=("bf16", "fp16"), default="bf16")
    ap.add_argument("--kv-dtype", choices=("16", "fp8"), default="16", help="fp8: the fp8 cache's forms against the 16-bit d64 call")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch

    fp8 = a.kv_dtype == "fp8"
    if a.out is None:
        a.out = os.path.join(ROOT, "profiles", "inference", f"decode64_{'fp8_' if fp8 else ''}bench_{a.dtype}.jsonl")
    assert torch.cuda.is_available(), "decode64_bench.py needs the GPU"
    dtype = torch.bfloat16 if a.dtype == "bf16" else torch.float16
    lines = []
    for case in CASES:
        lines.append((run_fp8 if fp8 else run)(*case, dtype, a.reps))
        print(json.dumps(lines[-1]), flush=True)
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "w") as f:
        f.writelines(json.dumps(ln) + "\n" for ln in lines)
    sys.exit(0 if fp8 or all(ln["gate_d64_beats_padded"] for ln in lines) else 1)


if __name__ == "__main__":
    main()
