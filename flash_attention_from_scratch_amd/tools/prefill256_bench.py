"""Prefill at d_head = 256, timing (prefill64_bench.py's protocol): one JSON line per case with, in one process,
alternating, medians after two warm-up rounds, bf16 by default, (H, Hkv) = (16, 8), causal.
  - "d256_t64", "d256_t32": forward_varlen_d256 / forward_varlen_kvcache_d256 at either tile form (FA_PREFILL256_TILE), timed by the
              launch's own device events (timed=True);                                                                        (a)
  - "d128":   forward_varlen / forward_varlen_kvcache, the d128 entries, on tensors of the same bytes (2 H heads of 128: another
              function, the same traffic -- timed the same way, reported, not a result);                                     (b)
  - "sdpa":   torch's scaled_dot_product_attention per sequence on the keys the window sees (gathered from the pages and expanded to H
              heads outside the timing), uncapped, timed by events around the loop over the sequences;                       (c)
  - "d256_2": (a) at the shipped form a second time: the A/A spread every ratio is read against.
Cases: packed 8 x 4096, and a 2048-row chunk behind a 32k prefix at batch 8 in a paged cache (pages of 256), each without a window and
with (4095, 0), and with cap 0 and 50.  The gate: (a, shipped form) / (c) < 1 by more than the A/A spread in every case (exit status 1
otherwise).  Reported, not gated: (a) / (b) and the useful TFLOP/s of (a) (4 H D per (row, key the row sees)).  Clocks are whatever
the device runs at.  Written to profiles/inference/prefill256_bench_<dtype>.jsonl unless --out says otherwise.

    python flash_attention_from_scratch_amd/tools/prefill256_bench.py [--reps N] [--out FILE]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from flash_attention_from_scratch_amd.tools.prefill64_bench import _alternate   # noqa: E402

H, HKV, BATCH, PAGE, LEFT, D = 16, 8, 8, 256, 4095, 256
CASES = [(kind, left, cap) for kind in ("packed", "chunk") for left in (-1, LEFT) for cap in (0.0, 50.0)]
SHIPPED = "d256_t64"


def seen_pairs(len_q, len_k, left):
    """(row, key) pairs of one causal sequence and head"""
    return sum(min(r + len_k - len_q, len_k - 1) - (0 if left < 0 else max(0, r + len_k - len_q - left)) + 1 for r in range(len_q))


def run(kind, left, cap, dtype, reps):
    import torch
    import torch.nn.functional as F

    import flash_attention as fa

    gen = torch.Generator(device="cuda").manual_seed(0)
    rand = lambda *shape: torch.randn(shape, generator=gen, device="cuda").to(dtype)   # noqa: E731
    i32 = lambda x: torch.tensor(x, dtype=torch.int32, device="cuda")   # noqa: E731
    call = dict(causal=True, window_size=(-1, -1) if left < 0 else (left, 0), timed=True)
    len_q, len_k = (4096, 4096) if kind == "packed" else (2048, 32768 + 2048)
    q, cu = rand(BATCH * len_q, H, D), i32(list(range(0, BATCH * len_q + 1, len_q)))
    q2 = q.view(-1, 2 * H, 128)
    if kind == "packed":
        k, v = rand(BATCH * len_k, HKV, D), rand(BATCH * len_k, HKV, D)
        keys = [(k[b * len_k:(b + 1) * len_k], v[b * len_k:(b + 1) * len_k]) for b in range(BATCH)]
        d256 = lambda: fa.forward_varlen_d256(q, k, v, cu, len_q, cap, **call)[-1]   # noqa: E731
        d128 = lambda: fa.forward_varlen(q2, k.view(-1, 2 * HKV, 128), v.view(-1, 2 * HKV, 128), cu, len_q, softcap=cap, **call)[-1]   # noqa: E731
    else:
        n = len_k // PAGE
        k, v = rand(BATCH * n, PAGE, HKV, D), rand(BATCH * n, PAGE, HKV, D)
        table = torch.randperm(BATCH * n, generator=torch.Generator().manual_seed(0)).view(BATCH, n).cuda()
        keys = [(k[table[b]].view(len_k, HKV, D), v[table[b]].view(len_k, HKV, D)) for b in range(BATCH)]
        table, lens = table.to(torch.int32), i32([len_k] * BATCH)
        d256 = lambda: fa.forward_varlen_kvcache_d256(q, k, v, cu, len_q, lens, cap, block_table=table, **call)[-1]   # noqa: E731
        d128 = lambda: fa.forward_varlen_kvcache(q2, k.view(-1, PAGE, 2 * HKV, 128), v.view(-1, PAGE, 2 * HKV, 128), cu, len_q, lens,   # noqa: E731
                                                 block_table=table, softcap=cap, **call)[-1]
    # (c): the keys any row of the sequence sees, (1, H, n, 256) per sequence, and the rows' mask among them (None: plain top-left causal)
    lo = 0 if left < 0 else max(0, len_k - len_q - left)
    sd = [(q[b * len_q:(b + 1) * len_q].transpose(0, 1)[None],
           kk[lo:].repeat_interleave(H // HKV, dim=1).transpose(0, 1)[None].contiguous(),
           vv[lo:].repeat_interleave(H // HKV, dim=1).transpose(0, 1)[None].contiguous()) for b, (kk, vv) in enumerate(keys)]
    mask = None
    if len_k - lo != len_q or left >= 0:
        pos, key = torch.arange(len_q, device="cuda")[:, None] + (len_k - len_q), torch.arange(lo, len_k, device="cuda")[None, :]
        mask = (key <= pos) & ((key >= pos - left) if left >= 0 else True)
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def sdpa():
        start.record()
        for qq, kk, vv in sd:
            F.scaled_dot_product_attention(qq, kk, vv, attn_mask=mask, is_causal=mask is None)
        stop.record()
        torch.cuda.synchronize()
        return start.elapsed_time(stop)

    def at(tile):
        def go():
            os.environ["FA_PREFILL256_TILE"] = tile
            try:
                return d256()
            finally:
                del os.environ["FA_PREFILL256_TILE"]
        return go

    forward = {"d256_t64": at("64"), "d256_t32": at("32"), "d128": d128, "sdpa": sdpa, "d256_2": at(SHIPPED[-2:])}
    line = {"case": kind, "batch": BATCH, "len_q": len_q, "len_k": len_k, "window_left": left, "softcap": cap, "n_heads": H, "n_kv_heads": HKV,
            "dtype": str(dtype).replace("torch.", ""), "reps": reps}
    line.update(_alternate(forward, reps))
    a = line[SHIPPED + "_ms"]
    line["d256_over_sdpa"], line["d256_over_d128"], line["d256_over_d256_2"] = a / line["sdpa_ms"], a / line["d128_ms"], a / line["d256_2_ms"]
    line["t64_over_t32"] = line["d256_t64_ms"] / line["d256_t32_ms"]
    line["d256_useful_tflops"] = 4.0 * BATCH * H * D * seen_pairs(len_q, len_k, left) / (a * 1e9)
    line["gate_d256_beats_sdpa"] = line["d256_over_sdpa"] < 1.0 - abs(1.0 - line["d256_over_d256_2"])
    return line


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=11)
    ap.add_argument("--dtype", choices=("bf16", "fp16"), default="bf16")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch

    if a.out is None:
        a.out = os.path.join(ROOT, "profiles", "inference", f"prefill256_bench_{a.dtype}.jsonl")
    assert torch.cuda.is_available(), "prefill256_bench.py needs the GPU"
    assert a.reps >= 10, "medians of at least 10"
    dtype = torch.bfloat16 if a.dtype == "bf16" else torch.float16
    lines = []
    for case in CASES:
        lines.append(run(*case, dtype, a.reps))
        print(json.dumps(lines[-1]), flush=True)
        torch.cuda.empty_cache()
    lines[-1].update(device=torch.cuda.get_device_name(0), torch=torch.__version__, hip=torch.version.hip)
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "w") as f:
        f.writelines(json.dumps(ln) + "\n" for ln in lines)
    sys.exit(0 if all(ln["gate_d256_beats_sdpa"] for ln in lines) else 1)


if __name__ == "__main__":
    main()
