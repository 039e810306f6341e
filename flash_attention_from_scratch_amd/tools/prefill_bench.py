"""Chunked prefill against a KV cache, timing (the sibling of varlen_qk_bench.py).  One JSON line per case; all arms of a case
alternate in one process, event-timed medians after two warm-up rounds, the whole measurement repeated `--runs` times:
  (a) forward_varlen_kvcache on a paged cache whose pages are shuffled (page_size 256 by default);
  (b) forward_varlen_kvcache on the contiguous cache;
  (c) forward_varlen(cu_seqlens_k=) on K / V already gathered into packed form, the gather not timed -- it runs TWICE per round,
      and the spread between its two medians is the margin the ratios are read against;
  (d) the gather (every sequence's valid rows out of the contiguous cache into one packed tensor, torch.cat of slices: what a
      caller without the new entry point does once per chunk; a paged cache would need an index on top) plus (c).
Cases: a chunk of 512 and 2048 query tokens per sequence behind prefixes of 0, 8k and 64k cached keys (cache_seqlens = prefix +
chunk: the chunk's own keys are in the cache), causal (bottom-right), H / Hkv = 32 / 8 and 16 / 16.  Per case: the median over
the runs of (a) / (c), (b) / (c) and (d) / (c), the median margin, and whether (a) / (c) and (b) / (c) lie inside 1 + margin.

--kv-dtype fp8: the same cases with three arms instead, on paged caches of one table, alternating in one process:
  (a) forward_varlen_kvcache(k_descale=, v_descale=) on the e4m3fn cache (quantize_kvcache_fp8 of the 16-bit one);
  (b) forward_varlen_kvcache on the 16-bit cache the fp8 one was quantized from -- it runs twice per round, and the spread between
      its two medians is the margin;
  (c) what a caller without the fp8 form does once per chunk: dequantize the used pages of the fp8 cache into a 16-bit copy
      (float(x8) * descale of the page's sequence), then (b) on the copy.
Per case: fp8 / 16-bit, fp8 / (dequantize + 16-bit), the margin, and the error of (a) against (b) on the dequantized cache (both
compute in the 16-bit type; with general descales the dequantized values round once more in (b) and (c)).

    python flash_attention_from_scratch_amd/tools/prefill_bench.py [--reps N] [--runs N] [--batch N] [--page-size N] [--kv-dtype {16bit,fp8}] [--out FILE]
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402

import flash_attention  # noqa: E402


def _median(x):
    return sorted(x)[len(x) // 2]


def _cu(lengths):
    out = [0]
    for n in lengths:
        out.append(out[-1] + n)
    return torch.tensor(out, dtype=torch.int32).cuda()


def _pairs(len_q, len_k):
    """visible (query, key) pairs of one sequence under the bottom-right causal mask (len_q <= len_k)"""
    return len_q * (len_k - len_q) + len_q * (len_q + 1) // 2


def _toolchain():
    try:
        out = subprocess.run(["/opt/rocm/bin/hipcc", "--version"], capture_output=True, text=True, check=True).stdout
        return next((ln.strip() for ln in out.splitlines() if "HIP version" in ln), out.splitlines()[0].strip())
    except (OSError, subprocess.CalledProcessError, IndexError):
        return "unknown"


def case(chunk, prefix, batch, H, Hkv, page_size, dtype, reps, runs):
    len_k = prefix + chunk
    cap = (len_k + page_size - 1) // page_size * page_size
    gen = torch.Generator(device="cuda").manual_seed(0)
    q = torch.randn((batch * chunk, H, 128), generator=gen, device="cuda").to(dtype)
    kc, vc = (torch.randn((batch, cap, Hkv, 128), generator=gen, device="cuda").to(dtype) for _ in range(2))
    per_seq = cap // page_size
    perm = torch.randperm(batch * per_seq, generator=torch.Generator().manual_seed(1))
    table = perm.view(batch, per_seq).to(torch.int32).cuda()
    kp, vp = (torch.empty((batch * per_seq, page_size, Hkv, 128), dtype=dtype, device="cuda") for _ in range(2))
    kp[perm.cuda()] = kc.view(batch * per_seq, page_size, Hkv, 128)
    vp[perm.cuda()] = vc.view(batch * per_seq, page_size, Hkv, 128)
    lens = torch.full((batch,), len_k, dtype=torch.int32, device="cuda")
    cuq, cuk = _cu([chunk] * batch), _cu([len_k] * batch)

    def gather():
        return torch.cat([kc[b, :len_k] for b in range(batch)]), torch.cat([vc[b, :len_k] for b in range(batch)])

    kpk, vpk = gather()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    # the arms agree bit for bit (checked once, outside the timing)
    want = flash_attention.forward_varlen(q, kpk, vpk, cuq, chunk, causal=True, cu_seqlens_k=cuk, max_seqlen_k=len_k)
    for got in (flash_attention.forward_varlen_kvcache(q, kp, vp, cuq, chunk, lens, block_table=table, causal=True),
                flash_attention.forward_varlen_kvcache(q, kc, vc, cuq, chunk, lens, causal=True)):
        assert torch.equal(got[0].view(torch.int16), want[0].view(torch.int16)) and torch.equal(got[1], want[1])
    per_run = []
    for _ in range(runs):
        t = {name: [] for name in ("paged", "contiguous", "packed_a", "packed_b", "gather_packed")}
        for i in range(reps + 2):
            *_, c1 = flash_attention.forward_varlen(q, kpk, vpk, cuq, chunk, causal=True, timed=True, cu_seqlens_k=cuk, max_seqlen_k=len_k)
            *_, a = flash_attention.forward_varlen_kvcache(q, kp, vp, cuq, chunk, lens, block_table=table, causal=True, timed=True)
            *_, b = flash_attention.forward_varlen_kvcache(q, kc, vc, cuq, chunk, lens, causal=True, timed=True)
            *_, c2 = flash_attention.forward_varlen(q, kpk, vpk, cuq, chunk, causal=True, timed=True, cu_seqlens_k=cuk, max_seqlen_k=len_k)
            ev[0].record()
            kg, vg = gather()
            flash_attention.forward_varlen(q, kg, vg, cuq, chunk, causal=True, cu_seqlens_k=cuk, max_seqlen_k=len_k)
            ev[1].record()
            torch.cuda.synchronize()
            d = ev[0].elapsed_time(ev[1])
            del kg, vg
            if i > 1:
                for name, ms in zip(t, (a, b, c1, c2, d)):
                    t[name].append(ms)
        per_run.append({name: _median(x) for name, x in t.items()})
    packed = [0.5 * (r["packed_a"] + r["packed_b"]) for r in per_run]
    ratio = lambda name: _median([r[name] / p for r, p in zip(per_run, packed)])   # noqa: E731
    margin = _median([abs(r["packed_a"] - r["packed_b"]) / p for r, p in zip(per_run, packed)])
    flop = 4.0 * 128 * H * batch * _pairs(chunk, len_k)
    paged_ms = _median([r["paged"] for r in per_run])
    line = {"chunk": chunk, "prefix": prefix, "batch": batch, "n_heads": H, "n_kv_heads": Hkv, "page_size": page_size, "causal": True,
            "dtype": str(dtype).replace("torch.", ""), "reps": reps, "runs": runs,
            **{name + "_ms": _median([r[name] for r in per_run]) for name in per_run[0]},
            "paged_tflops": flop / paged_ms * 1e-9, "paged_over_packed": ratio("paged"), "contiguous_over_packed": ratio("contiguous"),
            "gather_packed_over_packed": ratio("gather_packed"), "margin": margin,
            "paged_over_gather_packed": _median([r["paged"] / r["gather_packed"] for r in per_run])}
    line["paged_inside_margin"] = line["paged_over_packed"] <= 1.0 + margin
    line["contiguous_inside_margin"] = line["contiguous_over_packed"] <= 1.0 + margin
    return line


def case_fp8(chunk, prefix, batch, H, Hkv, page_size, dtype, reps, runs):
    len_k = prefix + chunk
    cap = (len_k + page_size - 1) // page_size * page_size
    gen = torch.Generator(device="cuda").manual_seed(0)
    q = torch.randn((batch * chunk, H, 128), generator=gen, device="cuda").to(dtype)
    kc, vc = (torch.randn((batch, cap, Hkv, 128), generator=gen, device="cuda").to(dtype) for _ in range(2))
    k8c, v8c, kd, vd = flash_attention.quantize_kvcache_fp8(kc, vc)
    per_seq = cap // page_size
    perm = torch.randperm(batch * per_seq, generator=torch.Generator().manual_seed(1))
    table = perm.view(batch, per_seq).to(torch.int32).cuda()
    shape = (batch * per_seq, page_size, Hkv, 128)
    kp, vp = (torch.empty(shape, dtype=dtype, device="cuda") for _ in range(2))
    kp[perm.cuda()] = kc.view(shape)
    vp[perm.cuda()] = vc.view(shape)
    k8, v8 = (torch.empty(shape, dtype=torch.uint8, device="cuda") for _ in range(2))
    k8[perm.cuda()] = k8c.view(torch.uint8).view(shape)
    v8[perm.cuda()] = v8c.view(torch.uint8).view(shape)
    k8, v8 = k8.view(torch.float8_e4m3fn), v8.view(torch.float8_e4m3fn)
    del kc, vc, k8c, v8c
    lens = torch.full((batch,), len_k, dtype=torch.int32, device="cuda")
    cuq = _cu([chunk] * batch)
    used = table.flatten().long()                                   # (every page of the table is in use: cap - len_k < page_size)
    seq_of_page = torch.arange(batch, device="cuda").repeat_interleave(per_seq)

    def dequantize():
        kq, vq = (torch.empty(shape, dtype=dtype, device="cuda") for _ in range(2))
        kq[used] = (k8[used].float() * kd[seq_of_page][:, None, :, None]).to(dtype)
        vq[used] = (v8[used].float() * vd[seq_of_page][:, None, :, None]).to(dtype)
        return kq, vq

    fp8 = lambda **kw: flash_attention.forward_varlen_kvcache(q, k8, v8, cuq, chunk, lens, block_table=table, causal=True,   # noqa: E731
                                                              k_descale=kd, v_descale=vd, **kw)
    b16 = lambda k, v, **kw: flash_attention.forward_varlen_kvcache(q, k, v, cuq, chunk, lens, block_table=table, causal=True, **kw)   # noqa: E731
    kq, vq = dequantize()
    got, want = fp8(), b16(kq, vq)
    err = (got[0].float() - want[0].float()).abs().max().item()
    lse_err = (got[1] - want[1]).abs().max().item()
    del kq, vq, got, want
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    per_run = []
    for _ in range(runs):
        t = {name: [] for name in ("fp8", "b16_a", "b16_b", "dequant_b16")}
        for i in range(reps + 2):
            *_, b1 = b16(kp, vp, timed=True)
            *_, a = fp8(timed=True)
            *_, b2 = b16(kp, vp, timed=True)
            ev[0].record()
            kq, vq = dequantize()
            b16(kq, vq)
            ev[1].record()
            torch.cuda.synchronize()
            d = ev[0].elapsed_time(ev[1])
            del kq, vq
            if i > 1:
                for name, ms in zip(t, (a, b1, b2, d)):
                    t[name].append(ms)
        per_run.append({name: _median(x) for name, x in t.items()})
    b16_ms = [0.5 * (r["b16_a"] + r["b16_b"]) for r in per_run]
    margin = _median([abs(r["b16_a"] - r["b16_b"]) / p for r, p in zip(per_run, b16_ms)])
    flop = 4.0 * 128 * H * batch * _pairs(chunk, len_k)
    fp8_ms = _median([r["fp8"] for r in per_run])
    return {"chunk": chunk, "prefix": prefix, "batch": batch, "n_heads": H, "n_kv_heads": Hkv, "page_size": page_size, "causal": True,
            "dtype": str(dtype).replace("torch.", ""), "kv_dtype": "fp8_e4m3fn", "reps": reps, "runs": runs,
            **{name + "_ms": _median([r[name] for r in per_run]) for name in per_run[0]},
            "fp8_tflops": flop / fp8_ms * 1e-9, "fp8_over_b16": _median([r["fp8"] / p for r, p in zip(per_run, b16_ms)]),
            "fp8_over_dequant_b16": _median([r["fp8"] / r["dequant_b16"] for r in per_run]), "margin": margin,
            "max_abs_o_minus_b16": err, "max_abs_lse_minus_b16": lse_err}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--page-size", type=int, default=256)
    ap.add_argument("--dtype", choices=("bf16", "fp16"), default="bf16")
    ap.add_argument("--kv-dtype", choices=("16bit", "fp8"), default="16bit", help="fp8: the e4m3fn cache against the 16-bit one")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    fp8 = a.kv_dtype == "fp8"
    a.out = a.out or os.path.join(ROOT, "profiles", "inference", f"prefill_kvcache_{'fp8_' if fp8 else ''}bench_{a.dtype}.jsonl")
    assert torch.cuda.is_available(), "prefill_bench.py needs the GPU"
    dtype = torch.bfloat16 if a.dtype == "bf16" else torch.float16
    lines = [{"tool": "prefill_bench.py" + (" --kv-dtype fp8" if fp8 else ""), "toolchain": _toolchain(), "torch": torch.__version__, "device": torch.cuda.get_device_name(0)}]
    print(json.dumps(lines[0]), flush=True)
    for H, Hkv in ((32, 8), (16, 16)):
        for prefix in (0, 8192, 65536):
            for chunk in (512, 2048):
                lines.append((case_fp8 if fp8 else case)(chunk, prefix, a.batch, H, Hkv, a.page_size, dtype, a.reps, a.runs))
                print(json.dumps(lines[-1]), flush=True)
                torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.writelines(json.dumps(ln) + "\n" for ln in lines)


if __name__ == "__main__":
    main()
