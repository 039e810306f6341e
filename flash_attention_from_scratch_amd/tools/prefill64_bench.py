"""Prefill at d_head = 64, timing (decode64_bench.py's protocol): one JSON line per case with, in one process,
alternating, medians after two warm-up rounds, bf16 by default, (H, Hkv) = (64, 8), causal, sinks = linspace(4, 7).  Every arm is the
library's and is timed by the launch's own device events (timed=True).
  - "d64":    forward_varlen_d64 / forward_varlen_kvcache_d64 on the d64 tensors;                                          (a)
  - "padded": forward_varlen_sinks / forward_varlen_kvcache_sinks, the d128 entries, on the same tensors zero-padded to 128 (twice the
              bytes and the softmax scale of 128: the only thing a caller could do without this kernel -- timed, not a result);  (b)
  - "d64_2":  (a) a second time: the A/A spread every ratio is read against.
Cases: packed 8 x 4096, and a 2048-row chunk behind a 64k prefix at batch 8 in a paged cache (pages of 256), each without a window and
with (127, 0).  The gate: (a) / (b) < 1 by more than the A/A spread in every case (exit status 1 otherwise).  Ungated, from shapes: the
windowed cases' visited-tile ratio (64-key tiles the d64 kernel's 256-row workgroups visit, over the unwindowed case's), and one more
line, the useful TFLOP/s of (a) on a non-causal batch 4 x 16 heads x 4096 (4 B H S^2 D operations).  Clocks are whatever the device
runs at.  Written to profiles/inference/prefill64_bench_<dtype>.jsonl unless --out says otherwise.

--kv-dtype fp8 times forward_varlen_kvcache_d64 against an e4m3fn cache instead, the same protocol: the chunk cases
and 8 x 4096 rows against a contiguous cache of 4096 keys; written to profiles/inference/prefill64_fp8_bench_<dtype>.jsonl.
  - "fp8":     the call on the fp8 cache and its descales;                                                                     (a)
  - "dequant": what a caller could do without it: dequantize the whole cache to 16 bit (torch, timed by events around it), then the
               16-bit call (timed by its own events);                                                                           (b)
  - "bf16":    the 16-bit call on the cache the fp8 one was quantized from (half the bytes are the fp8 arm's to win);            (c)
  - "fp8_2":   (a) a second time, the A/A spread.
Reported per line, not gated (exit status 0): whether (a) / (b) < 1 by more than the A/A spread, and (a) / (c) beside it.

    python flash_attention_from_scratch_amd/tools/prefill64_bench.py [--reps N] [--out FILE] [--kv-dtype fp8]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

H, HKV, BATCH, PAGE, LEFT = 64, 8, 8, 256, 127
CASES = [(kind, left) for kind in ("packed", "chunk") for left in (-1, LEFT)]   # (case, window left (-1: none))
ARMS = ("d64", "padded", "d64_2")


def visited_tiles(len_q, len_k, left, rows=256):
    """64-key tiles the causal d64 kernel's workgroups of `rows` rows visit for one sequence and head"""
    total = 0
    for r0 in range(0, len_q, rows):
        r1 = min(r0 + rows, len_q) - 1
        lo = 0 if left < 0 else max(0, r0 + len_k - len_q - left)
        total += (r1 + len_k - len_q) // 64 - lo // 64 + 1
    return total


def _alternate(forward, reps):
    from flash_attention_from_scratch_amd.tools.decode_bench import _median

    times = {name: [] for name in forward}
    for i in range(reps + 2):   # (two warm-up rounds)
        for name, fn in forward.items():
            t = fn()
            if i > 1:
                times[name].append(t)
    return {f"{name}_ms": _median(ts) for name, ts in times.items()}


def run(kind, left, dtype, reps):
    import torch
    import torch.nn.functional as F

    import flash_attention as fa

    gen = torch.Generator(device="cuda").manual_seed(0)
    rand = lambda *shape: torch.randn(shape, generator=gen, device="cuda").to(dtype)   # noqa: E731
    i32 = lambda x: torch.tensor(x, dtype=torch.int32, device="cuda")   # noqa: E731
    pad = lambda t: F.pad(t, (0, 64))   # noqa: E731
    sinks = torch.linspace(4.0, 7.0, H, device="cuda")
    call = dict(causal=True, window_size=(-1, -1) if left < 0 else (left, 0), timed=True)
    len_q, len_k = (4096, 4096) if kind == "packed" else (2048, 65536 + 2048)
    q, cu = rand(BATCH * len_q, H, 64), i32(list(range(0, BATCH * len_q + 1, len_q)))
    if kind == "packed":
        k, v = rand(BATCH * len_k, HKV, 64), rand(BATCH * len_k, HKV, 64)
        qp, kp, vp = pad(q), pad(k), pad(v)
        forward = {"d64": lambda: fa.forward_varlen_d64(q, k, v, cu, len_q, sinks, **call)[-1],
                   "padded": lambda: fa.forward_varlen_sinks(qp, kp, vp, cu, len_q, sinks, **call)[-1]}
    else:
        n = len_k // PAGE
        k, v = rand(BATCH * n, PAGE, HKV, 64), rand(BATCH * n, PAGE, HKV, 64)
        table = torch.randperm(BATCH * n, generator=torch.Generator().manual_seed(0)).view(BATCH, n).to(torch.int32).cuda()
        lens, (qp, kp, vp) = i32([len_k] * BATCH), (pad(t) for t in (q, k, v))
        forward = {"d64": lambda: fa.forward_varlen_kvcache_d64(q, k, v, cu, len_q, lens, sinks, block_table=table, **call)[-1],
                   "padded": lambda: fa.forward_varlen_kvcache_sinks(qp, kp, vp, cu, len_q, lens, sinks, block_table=table, **call)[-1]}
    forward["d64_2"] = forward["d64"]
    line = {"case": kind, "batch": BATCH, "len_q": len_q, "len_k": len_k, "window_left": left, "n_heads": H, "n_kv_heads": HKV,
            "dtype": str(dtype).replace("torch.", ""), "reps": reps}
    line.update(_alternate(forward, reps))
    line["d64_over_padded"] = line["d64_ms"] / line["padded_ms"]
    line["d64_over_d64_2"] = line["d64_ms"] / line["d64_2_ms"]
    if left >= 0:
        line["visited_tile_ratio"] = visited_tiles(len_q, len_k, left) / visited_tiles(len_q, len_k, -1)
    line["gate_d64_beats_padded"] = line["d64_over_padded"] < 1.0 - abs(1.0 - line["d64_over_d64_2"])
    return line


def run_fp8(kind, left, dtype, reps):
    """one case against an fp8 cache: "chunk" as in run(), "contiguous": 8 x 4096 rows against a contiguous cache of 4096 keys"""
    import torch

    import flash_attention as fa

    gen = torch.Generator(device="cuda").manual_seed(0)
    i32 = lambda x: torch.tensor(x, dtype=torch.int32, device="cuda")   # noqa: E731
    sinks = torch.linspace(4.0, 7.0, H, device="cuda")
    call = dict(causal=True, window_size=(-1, -1) if left < 0 else (left, 0), timed=True)
    len_q, len_k = (4096, 4096) if kind == "contiguous" else (2048, 65536 + 2048)
    q, cu, lens = torch.randn((BATCH * len_q, H, 64), generator=gen, device="cuda").to(dtype), i32(list(range(0, BATCH * len_q + 1, len_q))), i32([len_k] * BATCH)
    k16, v16 = (torch.randn((BATCH, len_k, HKV, 64), generator=gen, device="cuda").to(dtype) for _ in range(2))
    k8, v8, kd, vd = fa.quantize_kvcache_fp8(k16, v16)
    more, owner = {}, torch.arange(BATCH, device="cuda")   # (owner: the sequence whose descale a cache entry or page takes)
    if kind == "chunk":   # pages of 256 behind a shuffled table
        n = len_k // PAGE
        table = torch.randperm(BATCH * n, generator=torch.Generator().manual_seed(0)).cuda()
        scatter = lambda t: torch.empty_like(t.view(BATCH * n, PAGE, HKV, 64)).index_copy_(0, table, t.view(BATCH * n, PAGE, HKV, 64))   # noqa: E731
        k16, v16, k8, v8 = scatter(k16), scatter(v16), scatter(k8.view(torch.uint8)).view(k8.dtype), scatter(v8.view(torch.uint8)).view(v8.dtype)
        owner = torch.empty(BATCH * n, dtype=torch.int64, device="cuda").index_copy_(0, table, torch.arange(BATCH, device="cuda").repeat_interleave(n))
        more = dict(block_table=table.view(BATCH, n).to(torch.int32))
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def dequant():
        start.record()
        kk, vv = (t8.to(dtype) * d[owner][:, None, :, None].to(dtype) for t8, d in ((k8, kd), (v8, vd)))
        stop.record()
        ms = fa.forward_varlen_kvcache_d64(q, kk, vv, cu, len_q, lens, sinks, **more, **call)[-1]   # (synchronizes: timed)
        return start.elapsed_time(stop) + ms

    forward = {"fp8": lambda: fa.forward_varlen_kvcache_d64(q, k8, v8, cu, len_q, lens, sinks, k_descale=kd, v_descale=vd, **more, **call)[-1],
               "dequant": dequant, "bf16": lambda: fa.forward_varlen_kvcache_d64(q, k16, v16, cu, len_q, lens, sinks, **more, **call)[-1]}
    forward["fp8_2"] = forward["fp8"]
    line = {"case": kind, "kv_dtype": "fp8_e4m3fn", "batch": BATCH, "len_q": len_q, "len_k": len_k, "window_left": left, "n_heads": H, "n_kv_heads": HKV,
            "dtype": str(dtype).replace("torch.", ""), "reps": reps}
    line.update(_alternate(forward, reps))
    line["fp8_over_dequant"] = line["fp8_ms"] / line["dequant_ms"]
    line["fp8_over_bf16"] = line["fp8_ms"] / line["bf16_ms"]
    line["fp8_over_fp8_2"] = line["fp8_ms"] / line["fp8_2_ms"]
    line["fp8_beats_dequant"] = line["fp8_over_dequant"] < 1.0 - abs(1.0 - line["fp8_over_fp8_2"])
    return line


def dense_rate(dtype, reps):
    """ungated: the useful TFLOP/s of (a) on a non-causal batch of 4 sequences x 16 heads x 4096"""
    import torch

    import flash_attention as fa

    B, Hd, S = 4, 16, 4096
    gen = torch.Generator(device="cuda").manual_seed(1)
    q, k, v = (torch.randn((B * S, Hd, 64), generator=gen, device="cuda").to(dtype) for _ in range(3))
    cu = torch.tensor(list(range(0, B * S + 1, S)), dtype=torch.int32, device="cuda")
    ms = _alternate({"d64": lambda: fa.forward_varlen_d64(q, k, v, cu, S, timed=True)[-1]}, reps)["d64_ms"]
    return {"case": "dense", "batch": B, "len_q": S, "len_k": S, "n_heads": Hd, "n_kv_heads": Hd, "causal": False, "dtype": str(dtype).replace("torch.", ""),
            "reps": reps, "d64_ms": ms, "d64_useful_tflops": 4.0 * B * Hd * S * S * 64 / (ms * 1e9)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=11)
    ap.add_argument("--dtype", choices=("bf16", "fp16"), default="bf16")
    ap.add_argument("--out", default=None)
    ap.add_argument("--kv-dtype", choices=("16bit", "fp8"), default="16bit")
    a = ap.parse_args()
    import torch

    fp8 = a.kv_dtype == "fp8"
    if a.out is None:
        a.out = os.path.join(ROOT, "profiles", "inference", f"prefill64_{'fp8_' if fp8 else ''}bench_{a.dtype}.jsonl")
    assert torch.cuda.is_available(), "prefill64_bench.py needs the GPU"
    assert a.reps >= 10, "medians of at least 10"
    dtype = torch.bfloat16 if a.dtype == "bf16" else torch.float16
    lines = []
    if fp8:
        for case in (("chunk", -1), ("chunk", LEFT), ("contiguous", -1)):
            lines.append(run_fp8(*case, dtype, a.reps))
            print(json.dumps(lines[-1]), flush=True)
            torch.cuda.empty_cache()
        lines[-1].update(device=torch.cuda.get_device_name(0), torch=torch.__version__, hip=torch.version.hip)
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            f.writelines(json.dumps(ln) + "\n" for ln in lines)
        sys.exit(0)
    for case in CASES:
        lines.append(run(*case, dtype, a.reps))
        print(json.dumps(lines[-1]), flush=True)
        torch.cuda.empty_cache()
    lines.append(dense_rate(dtype, a.reps))
    lines[-1].update(device=torch.cuda.get_device_name(0), torch=torch.__version__, hip=torch.version.hip)
    print(json.dumps(lines[-1]), flush=True)
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "w") as f:
        f.writelines(json.dumps(ln) + "\n" for ln in lines)
    sys.exit(0 if all(ln["gate_d64_beats_padded"] for ln in lines[:-1]) else 1)


if __name__ == "__main__":
    main()
