"""One decode step with the K / V append in front of it, timing (the sibling of decode_bench.py): one JSON line per case with,
in one process, alternating, event-timed medians on the same tensors of
  - "decode":       (a) flash_attention.forward_kvcache alone on a cache that already holds the new token (the floor);
  - "decode_graph": the same, captured once and replayed;
  - "fused":        (b) forward_kvcache(k=, v=, rotary_cos=, rotary_sin=): the append kernel (append, rotary, quantize, lengths),
                    then the same decode, eager;
  - "fused_graph":  (b) captured once and replayed;
  - "append":       flash_attention.append_kvcache alone (the extra launch by itself);
  - "torch":        (c) the step in eager torch -- gather cos / sin at device-side positions, rotate q and the new k in fp32,
                    index_put the rows through cache_seqlens (+ quantize for an fp8 cache), lengths + 1 -- then the same decode.
Every arm attends over the same number of keys: the lengths are not advanced between repetitions (each repetition rewrites the
same cache row), so (b) - (a) is the cost of the append and (c) - (a) the cost of doing it in eager torch.
Cases: decode_bench.py's uniform rows at 1k / 8k / 64k keys x batch 1 / 8 / 64, (n_heads, n_kv_heads) = (32, 8), seqlen_q = 1,
contiguous cache; and one chunk case (seqlen_q = seqlen_new = 16, MHA 16 heads, batch 1, 8k keys), which prices the
one-workgroup-per-batch-entry mapping of the append kernel.  Clocks are whatever the device runs at.

    python flash_attention_from_scratch_amd/tools/append_bench.py [--reps N] [--quick] [--kv-dtype {16bit,fp8}] [--out FILE]
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

ROTARY_DIM = 128
DESCALE = 0.02


def _median(x):
    return sorted(x)[len(x) // 2]


def _timed(fn):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop)


def _captured(fn):
    """fn captured into a graph after a warm-up on a side stream -> the graph's replay"""
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        fn()
    torch.cuda.current_stream().wait_stream(stream)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        fn()
    return graph.replay


def _torch_step(q, k, v, kc, vc, lens, cos, sin, kd, vd):
    """The append in eager torch, without a host read of lens: -> (q rotated, the new lengths)"""
    B, T = k.shape[0], k.shape[1]
    pos = lens.long()[:, None] + torch.arange(T, device=k.device)[None, :]          # (B, T)
    c, s = cos[pos].float()[:, :, None, :], sin[pos].float()[:, :, None, :]

    def rotate(x):
        x1, x2 = x[..., :ROTARY_DIM // 2].float(), x[..., ROTARY_DIM // 2:].float()
        return torch.cat((x1 * c - x2 * s, x1 * s + x2 * c), dim=-1).to(x.dtype)

    q_rot, k_rot = rotate(q), rotate(k)
    rows = torch.arange(B, device=k.device)[:, None].expand(B, T)
    if kc.dtype == torch.float8_e4m3fn:
        k8 = (k_rot.float() / kd[:, None, :, None]).clamp(-448.0, 448.0).to(torch.float8_e4m3fn)
        v8 = (v.float() / vd[:, None, :, None]).clamp(-448.0, 448.0).to(torch.float8_e4m3fn)
        kc.view(torch.uint8)[rows, pos] = k8.view(torch.uint8)
        vc.view(torch.uint8)[rows, pos] = v8.view(torch.uint8)
    else:
        kc[rows, pos] = k_rot
        vc[rows, pos] = v
    return q_rot, lens + T


def run(case, B, keys, H, Hkv, Sq, dtype, fp8, reps):
    gen = torch.Generator(device="cuda").manual_seed(0)
    q = torch.randn((B, Sq, H, 128), generator=gen, device="cuda").to(dtype)
    k = torch.randn((B, Sq, Hkv, 128), generator=gen, device="cuda").to(dtype)
    v = torch.randn((B, Sq, Hkv, 128), generator=gen, device="cuda").to(dtype)
    kc = torch.empty((B, keys, Hkv, 128), dtype=torch.float8_e4m3fn if fp8 else dtype, device="cuda")
    vc = torch.empty_like(kc)
    for b in range(B):   # (entry by entry: the fp32 temporaries of a 64k x 64 cache would not fit beside it)
        for t in (kc, vc):
            x = torch.randn((keys, Hkv, 128), generator=gen, device="cuda")
            t[b] = (x / DESCALE).clamp(-448.0, 448.0).to(t.dtype) if fp8 else x.to(dtype)
    kd = torch.full((B, Hkv), DESCALE, device="cuda") if fp8 else None
    vd = kd.clone() if fp8 else None
    pos = torch.arange(keys, device="cuda", dtype=torch.float32)[:, None]
    inv = 10000.0 ** (-torch.arange(0, ROTARY_DIM, 2, device="cuda", dtype=torch.float32) / ROTARY_DIM)[None, :]
    cos, sin = torch.cos(pos * inv).to(dtype), torch.sin(pos * inv).to(dtype)
    before = torch.full((B,), keys - Sq, dtype=torch.int32, device="cuda")   # the lengths in front of the append ...
    after = torch.full((B,), keys, dtype=torch.int32, device="cuda")         # ... and behind it
    kw = dict(k_descale=kd, v_descale=vd, causal=Sq > 1, max_seqlen_k=keys)

    def decode():
        return flash_attention.forward_kvcache(q, kc, vc, after, **kw)

    def fused():
        return flash_attention.forward_kvcache(q, kc, vc, before, k=k, v=v, rotary_cos=cos, rotary_sin=sin, **kw)

    def append():
        return flash_attention.append_kvcache(kc, vc, k, v, before, q=q, rotary_cos=cos, rotary_sin=sin, causal=Sq > 1, k_descale=kd, v_descale=vd)

    def eager():
        q_rot, lens = _torch_step(q, k, v, kc, vc, before, cos, sin, kd, vd)
        return flash_attention.forward_kvcache(q_rot, kc, vc, lens, **kw)

    arms = {"decode": decode, "decode_graph": _captured(decode), "fused": fused, "fused_graph": _captured(fused), "append": append,
            "torch": eager}
    times = {name: [] for name in arms}
    for i in range(reps + 2):   # (two warm-up rounds)
        for name, fn in arms.items():
            t = _timed(fn)
            if i > 1:
                times[name].append(t)
    line = {"case": case, "batch": B, "keys": keys, "n_heads": H, "n_kv_heads": Hkv, "seqlen_q": Sq, "seqlen_new": Sq,
            "dtype": str(dtype).replace("torch.", ""), "kv_dtype": "fp8_e4m3fn" if fp8 else "16bit", "rotary_dim": ROTARY_DIM, "reps": reps}
    for name in arms:
        line[f"{name}_ms"] = _median(times[name])
    line["fused_minus_decode_us"] = 1e3 * (line["fused_ms"] - line["decode_ms"])
    line["fused_graph_minus_decode_graph_us"] = 1e3 * (line["fused_graph_ms"] - line["decode_graph_ms"])
    line["torch_minus_decode_us"] = 1e3 * (line["torch_ms"] - line["decode_ms"])
    line["fused_over_decode"] = line["fused_ms"] / line["decode_ms"]
    line["fused_over_torch"] = line["fused_ms"] / line["torch_ms"]
    line["fused_graph_over_torch"] = line["fused_graph_ms"] / line["torch_ms"]
    return line


def cases(quick):
    for B in (1, 8, 64):
        for keys in (1024, 8192, 65536):
            if quick and keys == 8192:
                continue
            yield "step", B, keys, 32, 8, 1
    yield "chunk", 1, 8192, 16, 16, 16


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--quick", action="store_true", help="1k and 64k keys only")
    ap.add_argument("--dtype", choices=("bf16", "fp16"), default="bf16")
    ap.add_argument("--kv-dtype", choices=("16bit", "fp8"), default="16bit")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    fp8 = a.kv_dtype == "fp8"
    if a.out is None:
        a.out = os.path.join(ROOT, "profiles", "inference", "append_bench_fp8.jsonl" if fp8 else f"append_bench_{a.dtype}.jsonl")
    assert torch.cuda.is_available(), "append_bench.py needs the GPU"
    dtype = torch.bfloat16 if a.dtype == "bf16" else torch.float16
    lines = []
    for c in cases(a.quick):
        lines.append(run(*c, dtype, fp8, a.reps))
        print(json.dumps(lines[-1]), flush=True)
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.writelines(json.dumps(ln) + "\n" for ln in lines)


if __name__ == "__main__":
    main()
