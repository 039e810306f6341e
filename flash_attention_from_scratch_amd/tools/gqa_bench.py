"""Grouped-query attention timing (the sibling of bwd_bench.py): one JSON line per (shape, Hkv, causal) with, in one process,
alternating, event-timed medians of
  - the GQA forward with LSE (fa_fwd_launch_gqa) next to the MHA forward with LSE at the same (B, S, H) (K / V with H heads),
  - the GQA backward (fa_bwd_launch_gqa) next to the MHA backward,
  - torch SDPA with enable_gqa=True, forward + backward (its default backend; `sdpa_backend` names it),
and the dK / dV grid of the GQA backward: workgroups (batch * n_kv_heads * split * seq_len / 128) and split (> 1: the group's
query heads are spread over `split` workgroups and their fp32 partials summed by a reduction kernel).  Kernel times of their
own: run it under `rocprofv3 --kernel-trace --stats -- python flash_attention_from_scratch_amd/tools/gqa_bench.py`.

    python flash_attention_from_scratch_amd/tools/gqa_bench.py [--reps N] [--kv-heads 16,4,2,1] [--shape B,S,H] [--dtype bf16]
"""
import argparse
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402

import flash_attention  # noqa: E402
from flash_attention_from_scratch_amd import _capi  # noqa: E402
from flash_helpers import kernel_configs as kc  # noqa: E402


def _median(x):
    return sorted(x)[len(x) // 2]


def split_of(B, S, H, Hkv, causal):
    """the GQA backward's dK / dV split for this shape, read off fa_bwd_gqa_workspace_bytes (delta, then the partials)"""
    lib = _capi.load()
    base = _capi.FaBwdArgs(batch=B, seq_len=S, n_heads=H, d_head=128, qkv_batch_stride=S * H * 128, qkv_seq_stride=H * 128,
                           qkv_head_stride=128, out_batch_stride=S * H * 128, out_seq_stride=H * 128, out_head_stride=128,
                           dtype=15, causal=int(causal))
    a = _capi.FaBwdGqaArgs(base=base, n_kv_heads=Hkv, kv_batch_stride=S * Hkv * 128, kv_seq_stride=Hkv * 128, kv_head_stride=128,
                           dkv_batch_stride=S * Hkv * 128, dkv_seq_stride=Hkv * 128, dkv_head_stride=128)
    extra = lib.fa_bwd_gqa_workspace_bytes(ctypes.byref(a)) - 4 * B * H * S
    return 1 if extra == 0 else extra // (4 * B * Hkv * S * 2 * 128)


def _time(fn, reps):
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ev[0].record()
    fn()
    ev[1].record()
    torch.cuda.synchronize()
    return ev[0].elapsed_time(ev[1])


def run(B, S, H, Hkv, causal, dtype, reps):
    gen = torch.Generator().manual_seed(0)
    q, dout = (torch.randn((B, S, H, 128), generator=gen).to(dtype).cuda() for _ in range(2))
    k, v = (torch.randn((B, S, Hkv, 128), generator=gen).to(dtype).cuda() for _ in range(2))
    km, vm = k.repeat_interleave(H // Hkv, dim=2).contiguous(), v.repeat_interleave(H // Hkv, dim=2).contiguous()
    cfg = kc.best_config(kc.DType.BF16 if dtype == torch.bfloat16 else kc.DType.FP16, S, masked=causal)
    f_g, f_m, b_g, b_m = [], [], [], []
    for i in range(reps + 1):
        o, lse, t0 = flash_attention.forward_ex(cfg, q, k, v, causal=causal, timed=True, return_lse=True)
        om, lsem, t1 = flash_attention.forward_ex(cfg, q, km, vm, causal=causal, timed=True, return_lse=True)
        *_, t2 = flash_attention.backward(q, k, v, o, lse, dout, causal=causal, timed=True)
        *_, t3 = flash_attention.backward(q, km, vm, om, lsem, dout, causal=causal, timed=True)
        if i:
            f_g.append(t0), f_m.append(t1), b_g.append(t2), b_m.append(t3)
    split = split_of(B, S, H, Hkv, causal) if Hkv != H else 1
    line = {"shape": [B, S, H, 128], "n_kv_heads": Hkv, "dtype": str(dtype).replace("torch.", ""), "causal": causal,
            "gqa_fwd_lse_ms": _median(f_g), "mha_fwd_lse_ms": _median(f_m), "gqa_bwd_ms": _median(b_g), "mha_bwd_ms": _median(b_m),
            "dkdv_workgroups": B * Hkv * split * (S // 128), "dkdv_split": split}
    line["fwd_gqa_over_mha"] = line["gqa_fwd_lse_ms"] / line["mha_fwd_lse_ms"]
    line["bwd_gqa_over_mha"] = line["gqa_bwd_ms"] / line["mha_bwd_ms"]
    if Hkv == H:
        line["note"] = "Hkv == H: both columns take the MHA path"
    try:
        leaves = [t.detach().transpose(1, 2).clone().requires_grad_(True) for t in (q, k, v)]
        g = dout.transpose(1, 2)

        def sdpa():
            out = torch.nn.functional.scaled_dot_product_attention(*leaves, is_causal=causal, enable_gqa=Hkv != H)
            torch.autograd.grad(out, leaves, g)
        sdpa()
        line["torch_sdpa_gqa_fwd_bwd_ms"] = _median([_time(sdpa, 1) for _ in range(max(3, reps // 2))])
        line["gqa_fwd_bwd_over_sdpa"] = (line["gqa_fwd_lse_ms"] + line["gqa_bwd_ms"]) / line["torch_sdpa_gqa_fwd_bwd_ms"]
    except RuntimeError as e:
        line["torch_sdpa_gqa_fwd_bwd_ms"] = None
        line["sdpa_error"] = str(e)[:120]
    return line


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--kv-heads", default="16,4,2,1")
    ap.add_argument("--shape", default="4,4096,16")
    ap.add_argument("--dtype", choices=("bf16", "fp16"), default="bf16")
    ap.add_argument("--causal", choices=("both", "plain", "causal"), default="both")
    a = ap.parse_args()
    dtype = torch.bfloat16 if a.dtype == "bf16" else torch.float16
    B, S, H = (int(x) for x in a.shape.split(","))
    masks = {"both": (False, True), "plain": (False,), "causal": (True,)}[a.causal]
    for Hkv in (int(x) for x in a.kv_heads.split(",")):
        for causal in masks:
            print(json.dumps(run(B, S, H, Hkv, causal, dtype, a.reps)), flush=True)
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
