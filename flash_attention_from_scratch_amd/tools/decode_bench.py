"""KV-cache decode attention, timing (the sibling of varlen_bench.py): one JSON line per case with, in one process,
alternating, event-timed medians of three arms on the same tensors:
  - "rule":   flash_attention.forward_kvcache with the split rule's num_splits;
  - "split1": the same with num_splits = 1 (what split-KV is measured against);
  - "sdpa":   torch.nn.functional.scaled_dot_product_attention (enable_gqa) on K / V sliced to the length -- one call for a
              uniform batch, one call per batch entry for mixed lengths (what a user without a varlen decode must do).
Cases: batch 1, 8, 64 x cache length 1k, 8k, 64k x (H, Hkv) (32, 8), (16, 16), (16, 1) x seqlen_q 1, 4, every key valid;
the contiguous cache and the same cache in shuffled 256-row pages; and mixed lengths within one batch.  All
without the causal mask (for seqlen_q 1 it is the same problem).  `gbps_*` is achieved bytes / s = (the K and V bytes that are
valid + Q + O) / time.  Clocks are whatever the device runs at.
Kernel times of their own: run it under `rocprofv3 --kernel-trace --stats -- python .../decode_bench.py`.

--kv-dtype fp8: the same cases with two arms instead, alternating in one process, both with the split rule's num_splits:
  - "fp8":   forward_kvcache on the cache quantized to e4m3fn with per (batch, K / V head) descales (quantize_kvcache_fp8);
  - "16bit": forward_kvcache on the 16-bit cache the fp8 one was quantized from (the yardstick).
`gbps_fp8` counts K and V at 1 byte per element, `gbps_16bit` at 2; `fp8_over_16bit` is the time ratio.  Written to
profiles/inference/decode_fp8_bench_<dtype>.jsonl unless --out says otherwise.

    python flash_attention_from_scratch_amd/tools/decode_bench.py [--reps N] [--quick] [--kv-dtype {16bit,fp8}] [--out FILE]
"""
import argparse
import json
import os
import random
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

import flash_attention  # noqa: E402
from flash_attention_from_scratch_amd import flash_attention_kernels as fak  # noqa: E402


def _median(x):
    return sorted(x)[len(x) // 2]


def _timed(fn):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop)


def _quantize(k, v, chunk=4):
    """quantize_kvcache_fp8 a few batch entries at a time (its fp32 temporaries are several times a 64k cache's size)"""
    parts = [flash_attention.quantize_kvcache_fp8(k[b:b + chunk], v[b:b + chunk]) for b in range(0, k.shape[0], chunk)]
    return tuple(torch.cat([p[i] for p in parts]) for i in range(4))


def run_fp8(case, lengths, cache_len, H, Hkv, Sq, page_size, dtype, reps):
    B = len(lengths)
    gen = torch.Generator(device="cuda").manual_seed(0)
    q = torch.randn((B, Sq, H, 128), generator=gen, device="cuda").to(dtype)
    k = torch.randn((B, cache_len, Hkv, 128), generator=gen, device="cuda").to(dtype)
    v = torch.randn((B, cache_len, Hkv, 128), generator=gen, device="cuda").to(dtype)
    lens = torch.tensor(lengths, dtype=torch.int32, device="cuda")
    k8, v8, kd, vd = _quantize(k, v)
    kw = {}
    if page_size:
        per_seq = cache_len // page_size
        perm = torch.randperm(B * per_seq, generator=torch.Generator().manual_seed(1)).to("cuda")

        def paginate(t):
            out = torch.empty((B * per_seq, page_size, Hkv, 128), dtype=torch.uint8 if t.dtype == torch.float8_e4m3fn else t.dtype, device="cuda")
            out[perm] = (t.view(torch.uint8) if t.dtype == torch.float8_e4m3fn else t).view(B * per_seq, page_size, Hkv, 128)
            return out.view(t.dtype)
        k, v, k8, v8 = paginate(k), paginate(v), paginate(k8), paginate(v8)
        kw["block_table"] = perm.view(B, per_seq).to(torch.int32)
    t_8, t_16 = [], []
    for i in range(reps + 2):   # (two warm-up rounds)
        t0 = _timed(lambda: flash_attention.forward_kvcache(q, k8, v8, lens, k_descale=kd, v_descale=vd, **kw))
        t1 = _timed(lambda: flash_attention.forward_kvcache(q, k, v, lens, **kw))
        if i > 1:
            t_8.append(t0), t_16.append(t1)
    uniform = len(set(lengths)) == 1
    kv_elems, qo_bytes = 2 * sum(lengths) * Hkv * 128, 2 * 2 * B * Sq * H * 128
    line = {"case": case, "batch": B, "cache_len": cache_len, "lengths": lengths if not uniform else lengths[0], "n_heads": H,
            "n_kv_heads": Hkv, "seqlen_q": Sq, "page_size": page_size, "dtype": str(dtype).replace("torch.", ""), "kv_dtype": "fp8_e4m3fn",
            "reps": reps, "num_splits_rule": fak.kvcache_num_splits(q, k8, v8, lens, **kw),
            "bytes_fp8": kv_elems + qo_bytes, "bytes_16bit": 2 * kv_elems + qo_bytes, "fp8_ms": _median(t_8), "16bit_ms": _median(t_16)}
    line["gbps_fp8"] = line["bytes_fp8"] / (line["fp8_ms"] * 1e-3) / 1e9
    line["gbps_16bit"] = line["bytes_16bit"] / (line["16bit_ms"] * 1e-3) / 1e9
    line["fp8_over_16bit"] = line["fp8_ms"] / line["16bit_ms"]
    return line


def run(case, lengths, cache_len, H, Hkv, Sq, page_size, dtype, reps):
    B = len(lengths)
    gen = torch.Generator(device="cuda").manual_seed(0)
    q = torch.randn((B, Sq, H, 128), generator=gen, device="cuda").to(dtype)
    k = torch.randn((B, cache_len, Hkv, 128), generator=gen, device="cuda").to(dtype)
    v = torch.randn((B, cache_len, Hkv, 128), generator=gen, device="cuda").to(dtype)
    lens = torch.tensor(lengths, dtype=torch.int32, device="cuda")
    kw = {}
    kc_, vc_ = k, v
    if page_size:
        per_seq = cache_len // page_size
        perm = torch.randperm(B * per_seq, generator=torch.Generator().manual_seed(1)).to("cuda")
        kc_ = torch.empty((B * per_seq, page_size, Hkv, 128), dtype=dtype, device="cuda")
        vc_ = torch.empty_like(kc_)
        kc_[perm] = k.view(B * per_seq, page_size, Hkv, 128)
        vc_[perm] = v.view(B * per_seq, page_size, Hkv, 128)
        kw["block_table"] = perm.view(B, per_seq).to(torch.int32)
    uniform = len(set(lengths)) == 1
    qs = q.transpose(1, 2)   # (B, H, Sq, D) views for SDPA
    ks, vs = k.transpose(1, 2), v.transpose(1, 2)

    def sdpa():
        if uniform:
            return F.scaled_dot_product_attention(qs, ks[:, :, :lengths[0]], vs[:, :, :lengths[0]], enable_gqa=H != Hkv)
        return [F.scaled_dot_product_attention(qs[b:b + 1], ks[b:b + 1, :, :n], vs[b:b + 1, :, :n], enable_gqa=H != Hkv)
                for b, n in enumerate(lengths)]

    t_rule, t_one, t_sdpa = [], [], []
    for i in range(reps + 2):   # (two warm-up rounds)
        t0 = _timed(lambda: flash_attention.forward_kvcache(q, kc_, vc_, lens, **kw))
        t1 = _timed(lambda: flash_attention.forward_kvcache(q, kc_, vc_, lens, num_splits=1, **kw))
        t2 = _timed(sdpa)
        if i > 1:
            t_rule.append(t0), t_one.append(t1), t_sdpa.append(t2)
    nbytes = 2 * (2 * sum(lengths) * Hkv * 128 + 2 * B * Sq * H * 128)
    line = {"case": case, "batch": B, "cache_len": cache_len, "lengths": lengths if not uniform else lengths[0], "n_heads": H,
            "n_kv_heads": Hkv, "seqlen_q": Sq, "page_size": page_size, "dtype": str(dtype).replace("torch.", ""), "reps": reps,
            "num_splits_rule": fak.kvcache_num_splits(q, kc_, vc_, lens, **kw), "bytes": nbytes,
            "rule_ms": _median(t_rule), "split1_ms": _median(t_one), "sdpa_ms": _median(t_sdpa)}
    for arm in ("rule", "split1", "sdpa"):
        line[f"gbps_{arm}"] = nbytes / (line[f"{arm}_ms"] * 1e-3) / 1e9
    line["rule_over_split1"] = line["rule_ms"] / line["split1_ms"]
    line["rule_over_sdpa"] = line["rule_ms"] / line["sdpa_ms"]
    return line


def mixed_lengths(batch, cache_len, seed=0):
    rng = random.Random(seed)
    return [rng.randint(1, cache_len) for _ in range(batch)]


def cases(quick):
    heads = ((32, 8), (16, 16), (16, 1))
    for B in (1, 8, 64):
        for n in (1024, 8192, 65536):
            for H, Hkv in heads:
                for Sq in (1, 4):
                    if quick and (Sq == 4 or n == 8192):
                        continue
                    yield "uniform", [n] * B, n, H, Hkv, Sq, 0
                    if not quick:
                        yield "paged", [n] * B, n, H, Hkv, Sq, 256
    for B in (8, 64):
        for H, Hkv in heads:
            yield "mixed", mixed_lengths(B, 65536), 65536, H, Hkv, 1, 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--quick", action="store_true", help="seqlen_q 1, contiguous, 1k and 64k caches only")
    ap.add_argument("--dtype", choices=("bf16", "fp16"), default="bf16")
    ap.add_argument("--kv-dtype", choices=("16bit", "fp8"), default="16bit", help="fp8: the e4m3fn cache against the 16-bit one")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    fp8 = a.kv_dtype == "fp8"
    if a.out is None:
        a.out = os.path.join(ROOT, "profiles", "inference", f"decode_fp8_bench_{a.dtype}.jsonl" if fp8 else "decode_bench_bf16.jsonl")
    assert torch.cuda.is_available(), "decode_bench.py needs the GPU"
    dtype = torch.bfloat16 if a.dtype == "bf16" else torch.float16
    lines = []
    for c in cases(a.quick):
        lines.append((run_fp8 if fp8 else run)(*c, dtype, a.reps))
        print(json.dumps(lines[-1]), flush=True)
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.writelines(json.dumps(ln) + "\n" for ln in lines)


if __name__ == "__main__":
    main()
