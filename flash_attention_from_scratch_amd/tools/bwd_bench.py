"""The training path's timing: one JSON line per (shape, causal) with the forward with and without LSE (alternating, same
process; without the mask the plain forms bench.py times, with it the causal forms), the HIP backward, torch's eager backward (materialised S in the 16-bit dtype) and the backward of torch SDPA's
default backend on the same inputs.  FLOP convention: forward 4 B H S^2 d, backward 2.5x that, both halved for causal;
`share` is of the 2.5 PF dense-MFMA figure.  Kernel times of their own: run this under
`rocprofv3 --kernel-trace --stats -- python flash_attention_from_scratch_amd/tools/bwd_bench.py`.

    python flash_attention_from_scratch_amd/tools/bwd_bench.py [--reps N] [--shapes c1|sweep|all]
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
from flash_attention_from_scratch_amd import flash_attention_kernels as fak  # noqa: E402
from flash_helpers import kernel_configs as kc  # noqa: E402

PEAK = 2.5e15
C1 = [(4, 4096, 16)]
SWEEP = [(16 * 4096 // s, s, 16) for s in (1024, 2048, 4096, 8192, 16384)]   # constant tokens


def _median(x):
    return sorted(x)[len(x) // 2]


def _eager_out(q, k, v, causal):
    s = torch.einsum("bqhd,bkhd->bhqk", q, k) / q.shape[-1] ** 0.5
    if causal:
        s = s.masked_fill(torch.ones(s.shape[-2:], dtype=torch.bool, device=q.device).triu(1), float("-inf"))
    return torch.einsum("bhqk,bkhd->bqhd", torch.softmax(s, dim=-1), v)


def _time_backward(make_out, leaves, dout, reps):
    """ms of the backward of make_out() alone (event-timed around torch.autograd.grad)"""
    out = make_out()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    t = []
    for _ in range(reps):
        ev[0].record()
        torch.autograd.grad(out, leaves, dout, retain_graph=True)
        ev[1].record()
        torch.cuda.synchronize()
        t.append(ev[0].elapsed_time(ev[1]))
    return _median(t[1:] if len(t) > 1 else t)


def run(B, S, H, causal, dtype, reps):
    gen = torch.Generator().manual_seed(0)
    q, k, v, dout = (torch.randn((B, S, H, 128), generator=gen).to(dtype).cuda() for _ in range(4))
    cfg = kc.best_config(kc.DType.BF16 if dtype == torch.bfloat16 else kc.DType.FP16, S, masked=causal)
    fwd, fwd_lse, bwd = [], [], []
    for i in range(reps + 1):
        if causal:   # the causal forms (forward_ex)
            _, t0 = flash_attention.forward_ex(cfg, q, k, v, causal=True, timed=True)
            o, lse, t1 = flash_attention.forward_ex(cfg, q, k, v, causal=True, timed=True, return_lse=True)
        else:        # the plain forms, as bench.py times the forward (at S >= 16384 the forward without LSE takes the
            # alternating-direction form, the one with LSE the plain walk)
            _, t0 = fak.forward(cfg, q, k, v, benchmark=True)
            o, lse, t1 = fak.forward_lse(cfg, q, k, v, benchmark=True)
        *_, t2 = flash_attention.backward(q, k, v, o, lse, dout, causal=causal, timed=True)
        if i:
            fwd.append(t0), fwd_lse.append(t1), bwd.append(t2)
    flop_f = 4.0 * B * H * S * S * 128 / (2 if causal else 1)
    flop_b = 2.5 * flop_f
    line = {"shape": [B, S, H, 128], "dtype": str(dtype).replace("torch.", ""), "causal": causal,
            "fwd_forms": "causal (forward_ex)" if causal else "plain (flash_attention_kernels.forward / forward_lse)",
            "fwd_ms": _median(fwd), "fwd_lse_ms": _median(fwd_lse), "bwd_ms": _median(bwd)}
    line["fwd_lse_over_fwd"] = line["fwd_lse_ms"] / line["fwd_ms"]
    line["fwd_lse_tflops"] = flop_f / line["fwd_lse_ms"] / 1e9
    line["bwd_tflops"] = flop_b / line["bwd_ms"] / 1e9
    line["bwd_share_of_2p5pf"] = line["bwd_tflops"] * 1e12 / PEAK
    leaves = [t.detach().clone().requires_grad_(True) for t in (q, k, v)]
    try:
        line["torch_eager_bwd_ms"] = _time_backward(lambda: _eager_out(*leaves, causal), leaves, dout, 3)
    except torch.OutOfMemoryError:
        line["torch_eager_bwd_ms"] = None
    torch.cuda.empty_cache()
    try:
        qt, kt, vt = (t.transpose(1, 2) for t in leaves)
        sdpa = lambda: torch.nn.functional.scaled_dot_product_attention(qt, kt, vt, is_causal=causal)  # noqa: E731
        line["torch_sdpa_bwd_ms"] = _time_backward(sdpa, leaves, dout.transpose(1, 2), 3)
        line["torch_sdpa_backend"] = _sdpa_backend(qt, kt, vt, causal)
    except RuntimeError as e:
        line["torch_sdpa_bwd_ms"], line["torch_sdpa_backend"] = None, f"unavailable: {str(e)[:80]}"
    return line


def _sdpa_backend(q, k, v, causal):
    """which backend the default SDPA dispatch takes here (the first one that accepts the inputs, in torch's order)"""
    from torch.nn.attention import SDPBackend, sdpa_kernel
    for be in (SDPBackend.FLASH_ATTENTION, SDPBackend.EFFICIENT_ATTENTION, SDPBackend.MATH):
        try:
            with sdpa_kernel(be):
                torch.nn.functional.scaled_dot_product_attention(q[:, :, :256], k[:, :, :256], v[:, :, :256], is_causal=causal)
            return be.name
        except RuntimeError:
            continue
    return "unknown"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--shapes", choices=("c1", "sweep", "all"), default="all")
    ap.add_argument("--dtype", choices=("bf16", "fp16"), default="bf16")
    a = ap.parse_args()
    dtype = torch.bfloat16 if a.dtype == "bf16" else torch.float16
    shapes = {"c1": C1, "sweep": SWEEP, "all": C1 + [s for s in SWEEP if s not in C1]}[a.shapes]
    for B, S, H in shapes:
        for causal in (False, True):
            print(json.dumps(run(B, S, H, causal, dtype, a.reps)), flush=True)
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
