"""`flash_attention_kernels` -- Python mirror of the reference's pybind module
(/root/reference/src/flash_attention.cu:34-140) over the C ABI of libfa_hip.so.

    forward(kernel_cfg, q, k, v, o, benchmark=False) -> (Tensor, float)

Same argument meaning, same checks in the same order with the same messages
(RuntimeError, as TORCH_CHECK raises), same ownership rule for `o`, launch on
torch's current stream, blocking only when benchmark=True.  PyTorch-ROCm is
plumbing here (device memory, current stream); the computation is the HIP kernel
behind fa_fwd_launch.  There is no eager/CPU fallback: a missing library or a
non-gfx950 device raises.

`kernel_cfg.optimized_softmax` has the reference's meaning only (the first KV block skips the
rescale; same result with or without).  This build's extensions are asked for explicitly: a
`flash_helpers.kernel_configs.NativeKernelConfig` (what `best_config()` returns) carries
`speculative_softmax` / `prescaled_q`, which travel in `fa_fwd_opts` beside the 13-field key.  A plain
13-field config with `optimized_softmax` selects the speculative softmax only under
FA_ALLOW_SPECULATIVE=1 (the round-2 mapping, kept for sweeps).
"""

import ctypes
import math
import os

import torch

from . import _capi


_STATS_DTYPES = tuple(d for d in (torch.int32, getattr(torch, "uint32", None)) if d is not None)  # (torch.uint32: torch >= 2.3)


def _check_input(t, name):
    # CHECK_INPUT, src/include/cuda_utils.cuh:5-11
    if not t.is_cuda:
        raise RuntimeError(f"{name} must be a CUDA tensor")
    if not t.is_contiguous():
        raise RuntimeError(f"{name} must be contiguous")


def _native_options(kernel_cfg):
    """-> (speculative, prescaled_q); speculative is False, True, "adaptive" (fa_speculative_mode) or None = "where the
    config has a speculative variant" (FA_ALLOW_SPECULATIVE=1 on a plain config)."""
    spec = bool(getattr(kernel_cfg, "speculative_softmax", False))
    if spec and getattr(kernel_cfg, "adaptive_softmax", False):
        spec = "adaptive"
    if not spec and getattr(kernel_cfg, "optimized_softmax", False) and os.environ.get("FA_ALLOW_SPECULATIVE", "") == "1":
        spec = None  # "if the config has a speculative variant": resolved against the registry below
    return spec, bool(getattr(kernel_cfg, "prescaled_q", False))


def forward(kernel_cfg, q, k, v, o=None, benchmark=False, causal=False, allow_ragged=False, stats=None):
    """Reference signature plus keyword-only-by-convention wideners (default off, so the
    reference behaviour -- including its errors for seq_len not a multiple of the tiles -- is
    unchanged): `causal` applies a causal mask, `allow_ragged` accepts any seq_len, `stats` is an
    int32 / uint32 device tensor of >= 2 elements whose [0] the kernel increases by the number of work
    items it computed and whose [1] by the number the speculative softmax had to compute twice
    (fa_fwd_stats)."""
    return _forward(kernel_cfg, q, k, v, o, benchmark, causal, allow_ragged, stats, None)


def is_gqa(q, k, v):
    """Grouped-query attention inputs: k and v of one shape (batch, seq_len, n_kv_heads, d_head) with fewer heads than q."""
    return q.dim() == 4 and k.dim() == 4 and k.shape == v.shape and k.shape[2] != q.shape[2] and \
        (k.shape[0], k.shape[1], k.shape[3]) == (q.shape[0], q.shape[1], q.shape[3])


def forward_lse(kernel_cfg, q, k, v, o=None, benchmark=False, causal=False, allow_ragged=False, stats=None):
    """forward(), and the row log-sum-exp: -> (o, lse, ms), lse an fp32 (batch, n_heads, seq_len) tensor,
    lse[b, h, i] = ln sum_j exp(q_i . k_j / sqrt(d)) (fa_fwd_launch_lse).  The same O bits as forward() with the same
    arguments.  RuntimeError where the configuration has no such form (only the persistent (256, 64, 4) + buffer
    configuration at d_head 128 has one; seq_len % 256 == 0, seq_stride % 128 == 0).
    Grouped-query attention (is_gqa: k, v with n_kv_heads heads, n_kv_heads dividing n_heads; query head h reads K / V
    head h / (n_heads / n_kv_heads)) goes through fa_fwd_launch_gqa; k and v may be views with a contiguous last dimension
    (one stride set for both), q is made contiguous."""
    if q.dim() != 4:
        raise RuntimeError("q must have shape (batch, seq_len, n_heads, d_head)")
    lse = torch.empty((q.shape[0], q.shape[2], q.shape[1]), dtype=torch.float32, device=q.device)
    o, ms = _forward(kernel_cfg, q, k, v, o, benchmark, causal, allow_ragged, stats, lse)
    return o, lse, ms


def _forward(kernel_cfg, q, k, v, o, benchmark, causal, allow_ragged, stats, lse):
    masked = bool(causal or allow_ragged)
    gqa = lse is not None and is_gqa(q, k, v)
    if gqa:
        q = q if not q.is_cuda or q.is_contiguous() else q.contiguous()
        for t, name in ((k, "k"), (v, "v")):
            if not t.is_cuda:
                raise RuntimeError(f"{name} must be a CUDA tensor")
            if t.stride(3) != 1 or t.stride() != k.stride():
                raise RuntimeError("grouped-query attention: k and v need one stride set and a contiguous last dimension")
        if q.shape[2] % k.shape[2] != 0:
            raise RuntimeError(f"grouped-query attention: the K / V heads ({k.shape[2]}) must divide the query heads ({q.shape[2]})")
    _check_input(q, "q")
    if not gqa:
        _check_input(k, "k")
        _check_input(v, "v")

    q_dtype = q.dtype
    if q_dtype not in (torch.float16, torch.bfloat16):
        raise RuntimeError("Only fp16 and bf16 are supported")
    if k.dtype != q_dtype or v.dtype != q_dtype:
        raise RuntimeError("Input tensors must have the same data type")
    if q.dim() != 4:
        raise RuntimeError("q must have shape (batch, seq_len, n_heads, d_head)")

    cfg = _capi.make_config(kernel_cfg)
    lib = _capi.load()
    if not lib.fa_fwd_supported(ctypes.byref(cfg)):
        raise RuntimeError("Kernel configuration was not found in flash_kernels (libfa_hip.so registry)")
    if masked and not lib.fa_fwd_masked_supported(ctypes.byref(cfg)):
        raise RuntimeError("Kernel configuration has no causal / ragged-length variant in libfa_hip.so")
    speculative, prescaled_q = _native_options(kernel_cfg)
    if speculative is None:  # FA_ALLOW_SPECULATIVE=1: where the variant exists
        probe = _capi.make_opts(causal=causal, allow_ragged=allow_ragged, speculative=True, prescaled_q=prescaled_q)
        speculative = bool(lib.fa_fwd_ex_supported(ctypes.byref(cfg), ctypes.byref(probe)))
    if speculative and masked:
        # the masked forms of the 32- / 16-rows-per-wave kernels keep the running max (no speculative build): the request is
        # dropped there, as kc.softmax_mode(cfg, masked=True) and the oracle's blockwise_for_config report
        probe = _capi.make_opts(causal=causal, allow_ragged=allow_ragged, speculative=True, prescaled_q=prescaled_q)
        if not lib.fa_fwd_ex_supported(ctypes.byref(cfg), ctypes.byref(probe)):
            plain = _capi.make_opts(causal=causal, allow_ragged=allow_ragged, speculative=False, prescaled_q=prescaled_q)
            if lib.fa_fwd_ex_supported(ctypes.byref(cfg), ctypes.byref(plain)):
                speculative = False
    if speculative or prescaled_q:
        probe = _capi.make_opts(causal=causal, allow_ragged=allow_ragged, speculative=speculative, prescaled_q=prescaled_q)
        if not lib.fa_fwd_ex_supported(ctypes.byref(cfg), ctypes.byref(probe)):
            raise RuntimeError("Kernel configuration has no device variant with the requested native options "
                               f"(speculative_softmax={speculative}, prescaled_q={prescaled_q}, masked={masked}) in libfa_hip.so")
    cfg_dtype = kernel_cfg.dtype.to_torch_dtype() if hasattr(kernel_cfg.dtype, "to_torch_dtype") else None
    if cfg_dtype is None:
        cfg_dtype = {5: torch.float16, 15: torch.bfloat16}[int(kernel_cfg.dtype)]
    if cfg_dtype != q_dtype:
        raise RuntimeError("Kernel configuration dtype does not match input dtype")

    if q.shape != k.shape and not gqa:
        raise RuntimeError("Query and key tensors have same shape")
    if q.shape != v.shape and not gqa:
        raise RuntimeError("Query and value tensors have same shape")
    batch, seq_len, n_heads, d_head = q.shape
    if not allow_ragged and seq_len % cfg.B_r != 0:
        raise RuntimeError("Only multiples of B_r are supported for seq_len Q currently")
    if not allow_ragged and seq_len % cfg.B_c != 0:
        raise RuntimeError("Only multiples of B_c are supported for seq_len K currently")

    if o is not None:
        if o.dtype != q_dtype:
            raise RuntimeError("Output tensor must have the same dtype as inputs")
        if o.shape != q.shape:
            raise RuntimeError("Query and output tensors have same shape")
        _check_input(o, "o")
    else:
        o = torch.empty_like(q)

    args = _capi.FaFwdArgs(
        q=q.data_ptr(), k=k.data_ptr(), v=v.data_ptr(), o=o.data_ptr(),
        batch=batch, seq_len=seq_len, n_heads=n_heads, d_head=d_head,
        batch_stride=q.stride(0), seq_stride=q.stride(1), head_stride=q.stride(2),
        cfg=cfg,
    )
    stats_ptr = None
    if stats is not None:
        if not stats.is_cuda or stats.device != q.device or stats.dtype not in _STATS_DTYPES \
                or stats.numel() < 2 or not stats.is_contiguous():
            raise RuntimeError("stats must be a contiguous int32 / uint32 tensor of >= 2 elements on q's device")
        stats_ptr = stats.data_ptr()
    with torch.cuda.device(q.device):
        stream = ctypes.c_void_p(torch.cuda.current_stream(q.device).cuda_stream)
        if lse is not None:
            ms = ctypes.c_float(0.0)
            opts = _capi.make_opts(causal=causal, allow_ragged=allow_ragged, speculative=speculative,
                                   prescaled_q=prescaled_q, ms=ms if benchmark else None, stats_ptr=stats_ptr)
            if gqa:
                if not lib.fa_fwd_gqa_supported(ctypes.byref(cfg), ctypes.byref(opts)):
                    raise RuntimeError("Kernel configuration has no grouped-query attention form (only the persistent "
                                       "(B_r 256, B_c 64, 4 warps) + buffer configuration at d_head 128, without prescaled_q)")
                kv = _capi.make_kv_layout(k.shape[2], k.stride(0), k.stride(1), k.stride(2))
                _capi.check(lib.fa_fwd_launch_gqa(ctypes.byref(args), ctypes.byref(kv), ctypes.byref(opts),
                                                  ctypes.c_void_p(lse.data_ptr()), stream))
                return o, float(ms.value)
            if not lib.fa_fwd_lse_supported(ctypes.byref(cfg), ctypes.byref(opts)):
                raise RuntimeError("Kernel configuration has no form that writes the row log-sum-exp (only the persistent "
                                   "(B_r 256, B_c 64, 4 warps) + buffer configuration at d_head 128, without prescaled_q)")
            _capi.check(lib.fa_fwd_launch_lse(ctypes.byref(args), ctypes.byref(opts), ctypes.c_void_p(lse.data_ptr()), stream))
            return o, float(ms.value)
        if masked or speculative or prescaled_q or stats_ptr is not None:
            ms = ctypes.c_float(0.0)
            opts = _capi.make_opts(causal=causal, allow_ragged=allow_ragged, speculative=speculative,
                                   prescaled_q=prescaled_q, ms=ms if benchmark else None, stats_ptr=stats_ptr)
            _capi.check(lib.fa_fwd_launch_ex(ctypes.byref(args), ctypes.byref(opts), stream))
            return o, float(ms.value)
        if benchmark:
            ms = ctypes.c_float(0.0)
            _capi.check(lib.fa_fwd_launch_timed(ctypes.byref(args), stream, ctypes.byref(ms)))
            return o, float(ms.value)
        _capi.check(lib.fa_fwd_launch(ctypes.byref(args), stream))
    return o, 0.0


def backward(q, k, v, o, lse, dout, causal=False, timed=False):
    """dQ, dK, dV of attention softmax(q k^T / sqrt d) v (causal: key j contributes to query i iff j <= i) from the forward's
    o and lse (forward_lse) and the gradient dout (fa_bwd_launch).  q, k, v share one stride set (a packed QKV view passes
    as it is), o and dout another; the gradients come back contiguous.  d_head 128, bf16 / fp16, seq_len % 256 == 0.  The
    workspace is allocated with torch on the tensors' stream.  -> (dq, dk, dv), or (dq, dk, dv, ms) if timed (blocks).
    Grouped-query attention (is_gqa(q, k, v)): fa_bwd_launch_gqa, k and v with one stride set of their own; dk and dv have
    k's n_kv_heads heads."""
    if is_gqa(q, k, v):
        return _backward_gqa(q, k, v, o, lse, dout, causal, timed)
    for t, name in ((q, "q"), (k, "k"), (v, "v"), (o, "o"), (dout, "dout"), (lse, "lse")):
        if not t.is_cuda:
            raise RuntimeError(f"{name} must be a CUDA tensor")
    if q.dtype not in (torch.float16, torch.bfloat16):
        raise RuntimeError("Only fp16 and bf16 are supported")
    if any(t.dtype != q.dtype for t in (k, v, o, dout)):
        raise RuntimeError("q, k, v, o and dout must have the same data type")
    if q.dim() != 4 or any(t.shape != q.shape for t in (k, v, o, dout)):
        raise RuntimeError("q, k, v, o and dout must have one shape (batch, seq_len, n_heads, d_head)")
    if k.stride() != q.stride() or v.stride() != q.stride():
        raise RuntimeError("q, k and v must share their strides")
    if q.stride(3) != 1:
        raise RuntimeError("the last dimension of q, k and v must be contiguous")
    o, dout = o.contiguous(), dout.contiguous()
    batch, seq_len, n_heads, d_head = q.shape
    if lse.dtype != torch.float32 or tuple(lse.shape) != (batch, n_heads, seq_len) or not lse.is_contiguous():
        raise RuntimeError("lse must be a contiguous fp32 (batch, n_heads, seq_len) tensor")
    dq, dk, dv = torch.empty_like(o), torch.empty_like(o), torch.empty_like(o)
    lib = _capi.load()
    args = _capi.FaBwdArgs(
        q=q.data_ptr(), k=k.data_ptr(), v=v.data_ptr(), o=o.data_ptr(), dout=dout.data_ptr(),
        lse=ctypes.cast(ctypes.c_void_p(lse.data_ptr()), ctypes.POINTER(ctypes.c_float)),
        dq=dq.data_ptr(), dk=dk.data_ptr(), dv=dv.data_ptr(), workspace=None,
        batch=batch, seq_len=seq_len, n_heads=n_heads, d_head=d_head,
        qkv_batch_stride=q.stride(0), qkv_seq_stride=q.stride(1), qkv_head_stride=q.stride(2),
        out_batch_stride=o.stride(0), out_seq_stride=o.stride(1), out_head_stride=o.stride(2),
        dtype=15 if q.dtype == torch.bfloat16 else 5, causal=1 if causal else 0,
    )
    nbytes = lib.fa_bwd_workspace_bytes(ctypes.byref(args))
    _capi.check(nbytes if nbytes < 0 else 0)
    with torch.cuda.device(q.device):
        workspace = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=q.device)   # (on the current stream's allocator)
        args.workspace = workspace.data_ptr()
        stream = ctypes.c_void_p(torch.cuda.current_stream(q.device).cuda_stream)
        ms = ctypes.c_float(0.0)
        _capi.check(lib.fa_bwd_launch(ctypes.byref(args), stream, ctypes.byref(ms) if timed else None))
    return (dq, dk, dv, float(ms.value)) if timed else (dq, dk, dv)


def _backward_gqa(q, k, v, o, lse, dout, causal, timed):
    for t, name in ((q, "q"), (k, "k"), (v, "v"), (o, "o"), (dout, "dout"), (lse, "lse")):
        if not t.is_cuda:
            raise RuntimeError(f"{name} must be a CUDA tensor")
    if q.dtype not in (torch.float16, torch.bfloat16):
        raise RuntimeError("Only fp16 and bf16 are supported")
    if any(t.dtype != q.dtype for t in (k, v, o, dout)):
        raise RuntimeError("q, k, v, o and dout must have the same data type")
    if any(t.shape != q.shape for t in (o, dout)):
        raise RuntimeError("q, o and dout must have one shape (batch, seq_len, n_heads, d_head)")
    if v.stride() != k.stride() or k.stride(3) != 1 or q.stride(3) != 1:
        raise RuntimeError("grouped-query attention: k and v need one stride set; q, k and v a contiguous last dimension")
    o, dout = o.contiguous(), dout.contiguous()
    batch, seq_len, n_heads, d_head = q.shape
    n_kv = k.shape[2]
    if lse.dtype != torch.float32 or tuple(lse.shape) != (batch, n_heads, seq_len) or not lse.is_contiguous():
        raise RuntimeError("lse must be a contiguous fp32 (batch, n_heads, seq_len) tensor")
    dq = torch.empty_like(o)
    dk = torch.empty((batch, seq_len, n_kv, d_head), dtype=q.dtype, device=q.device)
    dv = torch.empty_like(dk)
    lib = _capi.load()
    base = _capi.FaBwdArgs(
        q=q.data_ptr(), k=k.data_ptr(), v=v.data_ptr(), o=o.data_ptr(), dout=dout.data_ptr(),
        lse=ctypes.cast(ctypes.c_void_p(lse.data_ptr()), ctypes.POINTER(ctypes.c_float)),
        dq=dq.data_ptr(), dk=dk.data_ptr(), dv=dv.data_ptr(), workspace=None,
        batch=batch, seq_len=seq_len, n_heads=n_heads, d_head=d_head,
        qkv_batch_stride=q.stride(0), qkv_seq_stride=q.stride(1), qkv_head_stride=q.stride(2),
        out_batch_stride=o.stride(0), out_seq_stride=o.stride(1), out_head_stride=o.stride(2),
        dtype=15 if q.dtype == torch.bfloat16 else 5, causal=1 if causal else 0,
    )
    args = _capi.FaBwdGqaArgs(
        base=base, n_kv_heads=n_kv,
        kv_batch_stride=k.stride(0), kv_seq_stride=k.stride(1), kv_head_stride=k.stride(2),
        dkv_batch_stride=dk.stride(0), dkv_seq_stride=dk.stride(1), dkv_head_stride=dk.stride(2),
    )
    nbytes = lib.fa_bwd_gqa_workspace_bytes(ctypes.byref(args))
    _capi.check(nbytes if nbytes < 0 else 0)
    with torch.cuda.device(q.device):
        workspace = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=q.device)   # (on the current stream's allocator)
        args.base.workspace = workspace.data_ptr()
        stream = ctypes.c_void_p(torch.cuda.current_stream(q.device).cuda_stream)
        ms = ctypes.c_float(0.0)
        _capi.check(lib.fa_bwd_launch_gqa(ctypes.byref(args), stream, ctypes.byref(ms) if timed else None))
    return (dq, dk, dv, float(ms.value)) if timed else (dq, dk, dv)


# ---- packed variable-length sequences (fa_fwd_launch_varlen / fa_bwd_launch_varlen) ------------------------------------------

def varlen_config(dtype):
    """The configuration whose masked variant the varlen forward is the twin of: (B_r 128, B_c 64, 4 warps) + buffer."""
    from .flash_helpers import kernel_configs as kc

    name = kc.DType.BF16 if dtype == torch.bfloat16 else kc.DType.FP16
    return kc.FlashForwardKernelConfig(name, 128, 128, 64, 4, True, True, True, 0, 0, 0, True, False)


def _qk_sides(cu_seqlens_k, max_seqlen_k):
    """Separate K / V lengths are given (both of cu_seqlens_k and max_seqlen_k) or not (neither)."""
    if (cu_seqlens_k is None) != (max_seqlen_k is None):
        raise ValueError("cu_seqlens_k and max_seqlen_k go together: give both (separate Q and K / V lengths) or neither")
    return cu_seqlens_k is not None


def _check_varlen(q, k, v, cu_seqlens, max_seqlen, others=(), cu_seqlens_k=None, max_seqlen_k=None):
    if cu_seqlens_k is not None:
        others = tuple(others) + ((cu_seqlens_k, "cu_seqlens_k"),)
    for t, name in ((q, "q"), (k, "k"), (v, "v"), (cu_seqlens, "cu_seqlens")) + tuple(others):
        if not t.is_cuda:
            raise RuntimeError(f"{name} must be a CUDA tensor")
    if q.dtype not in (torch.float16, torch.bfloat16):
        raise RuntimeError("Only fp16 and bf16 are supported")
    if any(t.dtype != q.dtype for t in (k, v) + tuple(t for t, name in others if name not in ("lse", "cu_seqlens_k"))):
        raise RuntimeError("q, k, v (o and dout) must have the same data type")
    if q.dim() != 3 or k.dim() != 3 or k.shape != v.shape or k.shape[2] != q.shape[2] or (cu_seqlens_k is None and k.shape[0] != q.shape[0]):
        raise RuntimeError("packed sequences: q must have shape (total_tokens, n_heads, d_head), k and v (total_tokens, n_kv_heads, d_head)")
    if k.shape[1] < 1 or q.shape[1] % k.shape[1] != 0:
        raise RuntimeError(f"grouped-query attention: the K / V heads ({k.shape[1]}) must divide the query heads ({q.shape[1]})")
    if q.stride(2) != 1 or k.stride(2) != 1 or v.stride() != k.stride():
        raise RuntimeError("packed sequences: q, k, v need a contiguous last dimension, k and v one stride set")
    if cu_seqlens.dtype != torch.int32 or cu_seqlens.dim() != 1 or cu_seqlens.numel() < 2 or not cu_seqlens.is_contiguous():
        raise RuntimeError("cu_seqlens must be a contiguous int32 tensor of n_seqs + 1 entries on q's device")
    if not isinstance(max_seqlen, int) or isinstance(max_seqlen, bool):
        raise RuntimeError("max_seqlen must be a Python int (a bound on every sequence's length; the device is not asked)")
    if cu_seqlens_k is not None:
        if cu_seqlens_k.dtype != torch.int32 or cu_seqlens_k.dim() != 1 or not cu_seqlens_k.is_contiguous() or \
                cu_seqlens_k.numel() != cu_seqlens.numel():
            raise RuntimeError("cu_seqlens_k must be a contiguous int32 tensor with as many entries as cu_seqlens, on q's device")
        if not isinstance(max_seqlen_k, int) or isinstance(max_seqlen_k, bool):
            raise RuntimeError("max_seqlen_k must be a Python int (a bound on every sequence's K / V length; the device is not asked)")


def _varlen_layouts(q, k, cu_seqlens, max_seqlen, cu_seqlens_k, max_seqlen_k):
    """-> the launch's fa_varlen_layout(s): one for Q and K / V, or with the key side given (query side, key side)"""
    n_seqs = cu_seqlens.numel() - 1
    if cu_seqlens_k is None:
        return (_capi.make_varlen_layout(cu_seqlens.data_ptr(), n_seqs, q.shape[0], max_seqlen),)
    return (_capi.make_varlen_layout(cu_seqlens.data_ptr(), n_seqs, q.shape[0], max(max_seqlen, 1)),   # (a bound of 0: nothing but empties)
            _capi.make_varlen_layout(cu_seqlens_k.data_ptr(), n_seqs, k.shape[0], max(max_seqlen_k, 1)))


def forward_varlen(q, k, v, cu_seqlens, max_seqlen, causal=False, timed=False, cu_seqlens_k=None, max_seqlen_k=None, *,
                   window_size=(-1, -1), softcap=0.0):
    """Attention over packed sequences with the row log-sum-exp (fa_fwd_launch_varlen): q (total_tokens, n_heads, 128), k and v
    (total_tokens, n_kv_heads, 128), cu_seqlens an int32 device tensor of n_seqs + 1 row offsets, max_seqlen a Python int.
    Strided views (a packed QKV buffer) pass as they are.  -> (o, lse[, ms]); o contiguous, lse fp32 (n_heads, total_tokens).
    No device synchronisation unless timed.

    cu_seqlens_k / max_seqlen_k (both or neither, else ValueError): separate K / V lengths (fa_fwd_launch_varlen_qk).  cu_seqlens
    and max_seqlen are then Q's -- q is (total_q, n_heads, 128), lse (n_heads, total_q) -- and k, v are (total_k, n_kv_heads, 128)
    with sequence i's keys at rows cu_seqlens_k[i] .. cu_seqlens_k[i + 1] - 1.  Any lengths >= 0 on either side.  causal is then
    BOTTOM-RIGHT aligned, as in forward_kvcache and flash-attn: query r of a sequence sees keys j <= r + (len_k - len_q).  A row
    that sees no key (len_k = 0; causal rows r < len_q - len_k) gives o = 0 and lse = -inf.  Left at None: k and v share
    cu_seqlens and max_seqlen (the same kernel with one range for both sides).

    window_size=(left, right), keyword only, Python ints, -1 = unbounded (flash-attn's): query row r of a sequence, at position
    p = r + (len_k - len_q), sees the keys max(0, p - left) .. min(len_k - 1, p + right); causal means right = 0.  (-1, -1) takes
    the entry points above unchanged, anything else fa_fwd_launch_varlen_qk_window (one range given: on both sides), which visits
    no key tile outside a Q block's window and fetches no key row below it.  Bad values are a ValueError.  The gradients of a
    windowed forward are backward_varlen_window's (attention_varlen(window_size=) pairs the two); backward_varlen takes no window.

    softcap, keyword only, a Python float or int, finite and >= 0 (flash-attn's): the logit of a key the row sees becomes
    softcap * tanh(s / softcap), s = q . k / sqrt(128); masked keys stay -inf, lse is the log-sum-exp of the capped logits.  0 is
    off: the call above, the same entry points and bits.  Anything else goes through fa_fwd_launch_varlen_qk_softcap with the window
    ((-1, -1) included; one range given: on both sides).  Bad values are a ValueError.  The gradients are backward_varlen_softcap's
    (attention_varlen(softcap=) pairs the two)."""
    window = _window(window_size, causal)
    cap = _softcap(softcap)
    return _forward_varlen(q, k, v, cu_seqlens, max_seqlen, causal, timed, cu_seqlens_k, max_seqlen_k, window, cap)


def forward_varlen_sinks(q, k, v, cu_seqlens, max_seqlen, sinks, causal=False, timed=False, cu_seqlens_k=None, max_seqlen_k=None, *,
                         window_size=(-1, -1)):
    """forward_varlen with learned attention sinks (gpt-oss's `sinks`, flash-attn's learnable_sink; fa_fwd_launch_varlen_qk_sinks):
    every other argument is forward_varlen's, with its meaning and checks (one range given: on both sides; (-1, -1) included).
    sinks, required: a contiguous fp32 tensor of shape (n_heads,) on q's device, one logit z per QUERY head that joins the
    softmax's denominator and has no value vector: lse = log(exp(z) + sum_j exp(s_j)), o = sum_j exp(s_j - lse) v_j.  A row that
    sees no key gives o = 0 and lse = z; z = -inf means no sink for that head (forward_varlen's values; a dead row's lse = -inf).
    The host never reads sinks.  No softcap here, and no "off": without sinks, call forward_varlen.  -> (o, lse[, ms]).  A bad
    window_size is a ValueError before any tensor is looked at; a bad sinks a RuntimeError before the library is loaded.  The
    gradients are backward_varlen_sinks's (attention_varlen_sinks pairs the two)."""
    window = _window(window_size, causal)
    _check_sinks(sinks, q)
    return _forward_varlen(q, k, v, cu_seqlens, max_seqlen, causal, timed, cu_seqlens_k, max_seqlen_k, window, None, sinks)


def _check_sinks(sinks, q, name="sinks"):
    """sinks as forward_varlen_sinks and backward_varlen_sinks take it: a contiguous fp32 tensor of shape (n_heads,) on q's device
    (checked in front of _check_varlen, so against q only where q is a packed tensor at all)"""
    if not isinstance(sinks, torch.Tensor):
        raise RuntimeError(f"{name} must be a tensor: fp32, contiguous, of shape (n_heads,), on q's device (got {type(sinks).__name__})")
    if sinks.dtype != torch.float32:
        raise RuntimeError(f"{name} must be fp32 (got {sinks.dtype}; attention_varlen_sinks converts for you)")
    if sinks.dim() != 1 or not sinks.is_contiguous():
        raise RuntimeError(f"{name} must be a contiguous tensor of shape (n_heads,) (got shape {tuple(sinks.shape)}, strides {sinks.stride()})")
    if isinstance(q, torch.Tensor) and q.dim() == 3:
        if sinks.shape[0] != q.shape[1]:
            raise RuntimeError(f"{name} must have shape (n_heads,) = ({q.shape[1]},): one logit per query head (got {tuple(sinks.shape)})")
        if sinks.device != q.device:
            raise RuntimeError(f"{name} must be on q's device ({q.device}, got {sinks.device})")


def _forward_varlen(q, k, v, cu_seqlens, max_seqlen, causal, timed, cu_seqlens_k, max_seqlen_k, window, cap, sinks=None):
    """forward_varlen (window: _window's, cap: _softcap's) and forward_varlen_sinks (sinks a checked tensor, cap None)"""
    qk = _qk_sides(cu_seqlens_k, max_seqlen_k)
    _check_varlen(q, k, v, cu_seqlens, max_seqlen, cu_seqlens_k=cu_seqlens_k, max_seqlen_k=max_seqlen_k)
    total, n_heads, d_head = q.shape
    lib = _capi.load()
    cfg = _capi.make_config(varlen_config(q.dtype))
    o = torch.empty((total, n_heads, d_head), dtype=q.dtype, device=q.device)
    lse = torch.empty((n_heads, total), dtype=torch.float32, device=q.device)
    if q.stride() != o.stride():   # (the launch has one stride set for q and o)
        q = q.contiguous()
    args = _capi.FaFwdArgs(q=q.data_ptr(), k=k.data_ptr(), v=v.data_ptr(), o=o.data_ptr(), batch=1, seq_len=total, n_heads=n_heads,
                           d_head=d_head, batch_stride=0, seq_stride=q.stride(0), head_stride=q.stride(1), cfg=cfg)
    kv = _capi.make_kv_layout(k.shape[1], 0, k.stride(0), k.stride(1))
    sides = _varlen_layouts(q, k, cu_seqlens, max_seqlen, cu_seqlens_k, max_seqlen_k)
    ms = ctypes.c_float(0.0)
    opts = _capi.make_opts(causal=causal, ms=ms if timed else None)
    with torch.cuda.device(q.device):
        stream = ctypes.c_void_p(torch.cuda.current_stream(q.device).cuda_stream)
        if sinks is not None:
            w, sk = _capi.make_window(*(window or (-1, -1))), _capi.make_sinks(sinks.data_ptr(), n_heads)
            _capi.check(lib.fa_fwd_launch_varlen_qk_sinks(ctypes.byref(args), ctypes.byref(kv), ctypes.byref(sides[0]), ctypes.byref(sides[-1]),
                                                          ctypes.byref(w), ctypes.byref(sk), ctypes.byref(opts),
                                                          ctypes.c_void_p(lse.data_ptr()), stream))
            return (o, lse, float(ms.value)) if timed else (o, lse)
        if cap is not None:
            w, sc = _capi.make_window(*(window or (-1, -1))), _capi.make_softcap(cap)
            _capi.check(lib.fa_fwd_launch_varlen_qk_softcap(ctypes.byref(args), ctypes.byref(kv), ctypes.byref(sides[0]), ctypes.byref(sides[-1]),
                                                            ctypes.byref(w), ctypes.byref(sc), ctypes.byref(opts),
                                                            ctypes.c_void_p(lse.data_ptr()), stream))
            return (o, lse, float(ms.value)) if timed else (o, lse)
        if window is not None:
            w = _capi.make_window(*window)
            _capi.check(lib.fa_fwd_launch_varlen_qk_window(ctypes.byref(args), ctypes.byref(kv), ctypes.byref(sides[0]), ctypes.byref(sides[-1]),
                                                           ctypes.byref(w), ctypes.byref(opts), ctypes.c_void_p(lse.data_ptr()), stream))
            return (o, lse, float(ms.value)) if timed else (o, lse)
        launch = lib.fa_fwd_launch_varlen_qk if qk else lib.fa_fwd_launch_varlen
        _capi.check(launch(ctypes.byref(args), ctypes.byref(kv), *(ctypes.byref(s) for s in sides), ctypes.byref(opts),
                           ctypes.c_void_p(lse.data_ptr()), stream))
    return (o, lse, float(ms.value)) if timed else (o, lse)


def backward_varlen(q, k, v, o, lse, dout, cu_seqlens, max_seqlen, causal=False, timed=False, cu_seqlens_k=None, max_seqlen_k=None):
    """dQ, dK, dV over packed sequences from forward_varlen's o and lse and the gradient dout (fa_bwd_launch_varlen).  q, and
    k / v (one stride set), may be strided views; o and dout are made contiguous; the gradients come back contiguous, dk and dv
    with k's n_kv_heads heads.  -> (dq, dk, dv[, ms]).

    cu_seqlens_k / max_seqlen_k (both or neither, else ValueError): separate K / V lengths as in forward_varlen
    (fa_bwd_launch_varlen_qk), causal bottom-right aligned.  A row that saw no key (lse = -inf) gets dq = 0; a key no query
    sees (len_q = 0: under the bottom-right mask the last row sees every key) gets dk = dv = 0, written.

    No window: the gradients of forward_varlen(window_size=) are backward_varlen_window's."""
    return _backward_varlen(q, k, v, o, lse, dout, cu_seqlens, max_seqlen, causal, timed, cu_seqlens_k, max_seqlen_k, None)


def backward_varlen_window(q, k, v, o, lse, dout, cu_seqlens, max_seqlen, window_size, causal=False, timed=False, cu_seqlens_k=None,
                           max_seqlen_k=None):
    """backward_varlen under forward_varlen's window_size=(left, right): dQ, dK, dV from the WINDOWED forward's o and lse, by the
    forward's rule (row r at p = r + (len_k - len_q) sees the keys max(0, p - left) .. min(len_k - 1, p + right); causal means
    right = 0).  (-1, -1) is backward_varlen, unchanged; anything else fa_bwd_launch_varlen_qk_window (one range given: on both
    sides), whose kernels visit no tile outside a block's window.  A row that sees no key (lse = -inf) gets dq = 0; a key no row
    sees gets dk = dv = 0, written.  Bad window_size values are a ValueError before any tensor is looked at."""
    window = _window(window_size, causal)
    return _backward_varlen(q, k, v, o, lse, dout, cu_seqlens, max_seqlen, causal, timed, cu_seqlens_k, max_seqlen_k, window)


def backward_varlen_softcap(q, k, v, o, lse, dout, cu_seqlens, max_seqlen, softcap, window_size=(-1, -1), causal=False, timed=False,
                            cu_seqlens_k=None, max_seqlen_k=None):
    """The backward of a soft-capped (and possibly windowed) forward_varlen: dQ, dK, dV from ITS o and lse under the same softcap
    and window_size.  With t = tanh(s / softcap), s = q . k / sqrt(128): dS = P (dP - delta) (1 - t^2), dQ = dS K / sqrt(128),
    dK = dS^T Q / sqrt(128), dV = P^T dO (fa_bwd_launch_varlen_qk_softcap; one range given: on both sides).  softcap == 0 is
    backward_varlen_window with the same arguments, unchanged.  A row that sees no key gets dq = 0; a key no row sees gets
    dk = dv = 0, written.  Bad window_size or softcap values are a ValueError before any tensor is looked at."""
    window = _window(window_size, causal)
    cap = _softcap(softcap)
    return _backward_varlen(q, k, v, o, lse, dout, cu_seqlens, max_seqlen, causal, timed, cu_seqlens_k, max_seqlen_k, window, cap)


def backward_varlen_sinks(q, k, v, o, lse, dout, cu_seqlens, max_seqlen, sinks, window_size=(-1, -1), causal=False, timed=False,
                          cu_seqlens_k=None, max_seqlen_k=None):
    """The backward of forward_varlen_sinks: dQ, dK, dV and dsinks from ITS o and lse under the same sinks and window_size
    (fa_bwd_launch_varlen_qk_sinks; one range given: on both sides).  dQ, dK, dV are backward_varlen_window's kernels on that lse,
    bit for bit ((-1, -1): its call with left = right = 2^30); dsinks[h] = - sum_rows exp(sinks[h] - lse[h, row]) delta[h, row], fp32
    of shape (n_heads,), summed in a fixed order.  -> (dq, dk, dv, dsinks[, ms]).  A row that sees no key gets dq = 0 and adds
    exactly 0 to dsinks; a key no row sees gets dk = dv = 0, written; a head with sinks[h] = -inf gets dsinks[h] = 0.  A bad
    window_size is a ValueError before any tensor is looked at, a bad sinks a RuntimeError before the library is loaded."""
    window = _window(window_size, causal)
    _check_sinks(sinks, q)
    return _backward_varlen(q, k, v, o, lse, dout, cu_seqlens, max_seqlen, causal, timed, cu_seqlens_k, max_seqlen_k, window, None, sinks)


def _backward_varlen(q, k, v, o, lse, dout, cu_seqlens, max_seqlen, causal, timed, cu_seqlens_k, max_seqlen_k, window, cap=None,
                     sinks=None):
    """backward_varlen (window None), backward_varlen_window (window (left, right): the two-range arguments, given or not),
    backward_varlen_softcap (cap a float: the two-range arguments and a window, (-1, -1) where none is given) and
    backward_varlen_sinks (sinks a checked tensor: as with a cap, and dsinks behind dv in the result)"""
    qk = _qk_sides(cu_seqlens_k, max_seqlen_k)
    _check_varlen(q, k, v, cu_seqlens, max_seqlen, others=((o, "o"), (dout, "dout"), (lse, "lse")),
                  cu_seqlens_k=cu_seqlens_k, max_seqlen_k=max_seqlen_k)
    total, n_heads, d_head = q.shape
    total_k, n_kv = k.shape[0], k.shape[1]
    total_name = "total_q" if qk else "total_tokens"
    if o.shape != q.shape or dout.shape != q.shape:
        raise RuntimeError(f"q, o and dout must have one shape ({total_name}, n_heads, d_head)")
    if lse.dtype != torch.float32 or tuple(lse.shape) != (n_heads, total) or not lse.is_contiguous():
        raise RuntimeError(f"lse must be a contiguous fp32 (n_heads, {total_name}) tensor")
    o, dout = o.contiguous(), dout.contiguous()
    dq = torch.empty_like(o)
    dk = torch.empty((total_k, n_kv, d_head), dtype=q.dtype, device=q.device)
    dv = torch.empty_like(dk)
    lib = _capi.load()
    sides = _varlen_layouts(q, k, cu_seqlens, max_seqlen, cu_seqlens_k, max_seqlen_k)
    fields = dict(
        q=q.data_ptr(), k=k.data_ptr(), v=v.data_ptr(), o=o.data_ptr(), dout=dout.data_ptr(),
        lse=ctypes.cast(ctypes.c_void_p(lse.data_ptr()), ctypes.POINTER(ctypes.c_float)),
        dq=dq.data_ptr(), dk=dk.data_ptr(), dv=dv.data_ptr(), workspace=16,
        n_heads=n_heads, n_kv_heads=n_kv, d_head=d_head,
        q_seq_stride=q.stride(0), q_head_stride=q.stride(1), out_seq_stride=o.stride(0), out_head_stride=o.stride(1),
        kv_seq_stride=k.stride(0), kv_head_stride=k.stride(1), dkv_seq_stride=dk.stride(0), dkv_head_stride=dk.stride(1),
        dtype=15 if q.dtype == torch.bfloat16 else 5, causal=1 if causal else 0, varlen=sides[0],
    )
    dsinks = None
    if qk or window is not None or cap is not None or sinks is not None:
        args = _capi.FaBwdVarlenQKArgs(struct_size=ctypes.sizeof(_capi.FaBwdVarlenQKArgs), varlen_k=sides[-1], **fields)
        workspace_bytes, launch = lib.fa_bwd_varlen_qk_workspace_bytes, lib.fa_bwd_launch_varlen_qk
        if sinks is not None:
            # (no rows on either side: the launch returns at once and writes nothing -- the sum over no rows is 0)
            dsinks = (torch.empty if total or total_k else torch.zeros)((n_heads,), dtype=torch.float32, device=q.device)
            w, sk = _capi.make_window(*(window or (-1, -1))), _capi.make_sinks(sinks.data_ptr(), n_heads)
            workspace_bytes = lib.fa_bwd_varlen_qk_sinks_workspace_bytes
            launch = lambda a, stream, ms: lib.fa_bwd_launch_varlen_qk_sinks(   # noqa: E731
                a, ctypes.byref(w), ctypes.byref(sk), ctypes.c_void_p(dsinks.data_ptr()), stream, ms)
        elif cap is not None:
            w, sc = _capi.make_window(*(window or (-1, -1))), _capi.make_softcap(cap)
            launch = lambda a, stream, ms: lib.fa_bwd_launch_varlen_qk_softcap(a, ctypes.byref(w), ctypes.byref(sc), stream, ms)   # noqa: E731
        elif window is not None:
            w = _capi.make_window(*window)
            launch = lambda a, stream, ms: lib.fa_bwd_launch_varlen_qk_window(a, ctypes.byref(w), stream, ms)   # noqa: E731
    else:
        args = _capi.FaBwdVarlenArgs(**fields)
        workspace_bytes, launch = lib.fa_bwd_varlen_workspace_bytes, lib.fa_bwd_launch_varlen
    nbytes = workspace_bytes(ctypes.byref(args))
    _capi.check(nbytes if nbytes < 0 else 0)
    with torch.cuda.device(q.device):
        workspace = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=q.device)   # (on the current stream's allocator)
        args.workspace = workspace.data_ptr()
        stream = ctypes.c_void_p(torch.cuda.current_stream(q.device).cuda_stream)
        ms = ctypes.c_float(0.0)
        _capi.check(launch(ctypes.byref(args), stream, ctypes.byref(ms) if timed else None))
    grads = (dq, dk, dv) if sinks is None else (dq, dk, dv, dsinks)
    return grads + (float(ms.value),) if timed else grads


# ---- KV-cache decode (fa_decode_launch) ------------------------------------------------------------------------------------

def _decode_needs_copy(t):
    """A view the launch cannot take as it is: last dimension not contiguous, strides not multiples of 8 elements, or a base
    that is not 16-byte aligned."""
    return t.stride(-1) != 1 or any(s % 8 for s in t.stride()[:-1]) or t.data_ptr() % 16 != 0


_FLOAT8_DTYPES = tuple(getattr(torch, n) for n in ("float8_e4m3fn", "float8_e4m3fnuz", "float8_e5m2", "float8_e5m2fnuz") if hasattr(torch, n))


def _window(window_size, causal):
    """window_size=(left, right) as forward_kvcache and forward_varlen_kvcache take it -> None for (-1, -1) (the unwindowed entry
    points), else (left, right).  Bad values are a ValueError before the library is asked."""
    if (not isinstance(window_size, (tuple, list)) or len(window_size) != 2
            or any(not isinstance(w, int) or isinstance(w, bool) for w in window_size)):
        raise ValueError(f"window_size must be a pair of Python ints (left, right), -1 = unbounded (got {window_size!r})")
    left, right = window_size
    if left < -1 or right < -1:
        raise ValueError(f"window_size {(left, right)}: left and right must be -1 (unbounded) or not negative")
    if not -2 ** 31 <= left < 2 ** 31 or not -2 ** 31 <= right < 2 ** 31:
        raise ValueError(f"window_size {(left, right)}: left and right are 32-bit (pass -1 for unbounded)")
    if causal and right not in (-1, 0):
        raise ValueError(f"causal means right = 0: window_size {(left, right)} cannot be causal as well (pass right = -1 or 0)")
    return None if (left, right) == (-1, -1) else (left, right)


def _softcap(softcap):
    """softcap as forward_varlen, attention_varlen, backward_varlen_softcap, forward_varlen_kvcache and forward_kvcache_softcap take
    it -> None for 0 (no cap: the entry points
    without one), else the float.  A Python float or int (no bool, no tensor), finite and >= 0; anything else is a ValueError before
    the library is asked."""
    if isinstance(softcap, bool) or not isinstance(softcap, (int, float)):
        raise ValueError(f"softcap must be a Python float or int, finite and >= 0, 0 = off (got {softcap!r})")
    try:
        value = float(softcap)
    except OverflowError:   # (an int beyond the floats)
        value = float("inf")
    if not math.isfinite(value) or value < 0:
        raise ValueError(f"softcap {softcap!r}: must be finite and >= 0 (0 = off)")
    return None if value == 0 else value


def _need_tensors(named):
    for t, name in named:
        if not isinstance(t, torch.Tensor):
            raise RuntimeError(f"{name} must be a tensor")


def _need_device(named, anchor, whose):
    """Every (tensor, name) is a CUDA tensor on anchor's device, which the message calls `whose` device."""
    for t, name in named:
        if not t.is_cuda:
            raise RuntimeError(f"{name} must be a CUDA tensor")
        if t.device != anchor.device:
            raise RuntimeError(f"{name} must be on {whose} device ({anchor.device}, got {t.device})")


class _CacheSide:
    """The cache side of forward_kvcache, append_kvcache and forward_varlen_kvcache -- k_cache, v_cache, cache_seqlens, block_table
    and the descales -- with the checks the three share, one definition each.  A caller runs the stages where its own checks sit
    (a call that breaks two rules reports the first; tests/test_wrapper_refusals_*.py pin that); `entries` ("batch" / "n_seqs") and
    `whose` ("q's" / "the cache's" device) are the words their messages differ by.  dtypes() sets .fp8; .paged is set at once."""

    def __init__(self, k_cache, v_cache, cache_seqlens, block_table, k_descale, v_descale, entries, whose):
        self.k_cache, self.v_cache, self.cache_seqlens, self.block_table = k_cache, v_cache, cache_seqlens, block_table
        self.k_descale, self.v_descale, self.entries, self.whose = k_descale, v_descale, entries, whose
        self.paged = block_table is not None

    def _descales(self):
        return ((self.k_descale, "k_descale"), (self.v_descale, "v_descale"))

    def dtypes(self, like, fp8_needs_descales=None):
        """The cache's data type: fp8 (then e4m3fn, both) or `like`'s (None: the caller compares); descales only with fp8, and
        with `fp8_needs_descales` (a message) both of them."""
        k_cache, v_cache = self.k_cache, self.v_cache
        self.fp8 = fp8 = k_cache.dtype in _FLOAT8_DTYPES or v_cache.dtype in _FLOAT8_DTYPES
        given = [t for t, _ in self._descales() if t is not None]
        if fp8 and k_cache.dtype != v_cache.dtype:
            raise RuntimeError(f"k_cache and v_cache must have one data type (got {k_cache.dtype} and {v_cache.dtype})")
        if fp8 and k_cache.dtype != torch.float8_e4m3fn:
            raise RuntimeError(f"an fp8 cache must be torch.float8_e4m3fn (got {k_cache.dtype})")
        if fp8 and fp8_needs_descales and len(given) < 2:
            raise RuntimeError(fp8_needs_descales)
        if not fp8 and like is not None and k_cache.dtype != like.dtype:
            raise RuntimeError("Input tensors must have the same data type")
        if not fp8 and given:
            raise RuntimeError("k_descale / v_descale belong to an fp8 (torch.float8_e4m3fn) cache; this cache is 16-bit")
        return fp8

    def lengths(self, n, contiguous_needs):
        """A contiguous cache has n entries (`contiguous_needs`: the caller's words for that); cache_seqlens is n int32."""
        if not self.paged and self.k_cache.shape[0] != n:
            raise RuntimeError(f"a contiguous cache needs {contiguous_needs} (pass block_table for a paged cache)")
        t = self.cache_seqlens
        if t.dtype != torch.int32 or tuple(t.shape) != (n,) or not t.is_contiguous():
            raise RuntimeError(f"cache_seqlens must be a contiguous int32 tensor of {self.entries} entries on {self.whose} device")

    def table(self, n, max_seqlen_k=None):
        """block_table is (n, max_pages_per_seq) int32; max_seqlen_k, where the caller has one, a Python int."""
        t = self.block_table
        if t is not None and (t.dtype != torch.int32 or t.dim() != 2 or t.shape[0] != n or t.stride(1) != 1):
            raise RuntimeError(f"block_table must be an int32 ({self.entries}, max_pages_per_seq) tensor on {self.whose} device with a "
                               "contiguous last dimension")
        if max_seqlen_k is not None and (not isinstance(max_seqlen_k, int) or isinstance(max_seqlen_k, bool)):
            raise RuntimeError("max_seqlen_k must be a Python int (a bound on every length; the device is not asked)")

    def descales(self, n):
        """The descales decode and the append take: contiguous fp32 (n, n_kv_heads), or None."""
        n_kv = self.k_cache.shape[2]
        for t, name in self._descales():
            if t is not None and (t.dtype != torch.float32 or tuple(t.shape) != (n, n_kv) or not t.is_contiguous()):
                raise RuntimeError(f"{name} must be a contiguous fp32 (batch, n_kv_heads) = ({n}, {n_kv}) tensor on {self.whose} device")

    def strides(self):
        """The caches pass as they are, so the launch must be able to address them: one stride set, 16-byte units and base."""
        k_cache, v_cache = self.k_cache, self.v_cache
        kv_unit = 16 if self.fp8 else 8   # 16 bytes
        if (_decode_needs_copy(k_cache) or _decode_needs_copy(v_cache) or k_cache.stride() != v_cache.stride()
                or any(s % kv_unit for s in k_cache.stride()[:-1])):
            # (a serving cache is gigabytes: copying it on every call would be silently slow)
            raise RuntimeError(f"k_cache and v_cache need one stride set, a contiguous last dimension, strides that are multiples of {kv_unit} "
                               "elements and a 16-byte aligned base")

    def geometry(self):
        """The fields every cache struct has: the two device arrays and the sizes of a paged or a contiguous cache."""
        k_cache, bt = self.k_cache, self.block_table
        sizes = ((0, k_cache.shape[0], k_cache.shape[1], bt.shape[1], bt.stride(0)) if self.paged else (k_cache.shape[1], 0, 0, 0, 0))
        return dict(zip(("seqlen_cache", "num_pages", "page_size", "max_pages_per_seq", "block_table_stride"), sizes),
                    cache_seqlens=self.cache_seqlens.data_ptr(), block_table=bt.data_ptr() if self.paged else None)


def kvcache_num_splits(q, k_cache, v_cache, cache_seqlens, block_table=None, max_seqlen_k=None, num_splits=0, causal=False,
                       window_size=(-1, -1)):
    """The split count forward_kvcache uses for these arguments (fa_decode_num_splits, or fa_decode_fp8_num_splits for an fp8
    cache: the same rule; with a window_size other than (-1, -1) their _window_ forms, whose rule also reads causal): the same
    checks, nothing allocated, no launch."""
    window = _window(window_size, causal)
    _, args, fp8 = _decode_args(q, k_cache, v_cache, cache_seqlens, block_table, causal, max_seqlen_k, num_splits, None, None)
    lib = _capi.load()
    if window is not None:
        w = _capi.make_window(*window)
        return _capi.check((lib.fa_decode_fp8_window_num_splits if fp8 else lib.fa_decode_window_num_splits)(ctypes.byref(args), ctypes.byref(w)))
    return _capi.check((lib.fa_decode_fp8_num_splits if fp8 else lib.fa_decode_num_splits)(ctypes.byref(args)))


def _decode_args(q, k_cache, v_cache, cache_seqlens, block_table, causal, max_seqlen_k, num_splits, k_descale, v_descale):
    """forward_kvcache's checks -> (q as the launch takes it, fa_decode_args or fa_decode_fp8_args still without o, lse and
    workspace, whether the cache is fp8)."""
    optional = ((block_table, "block_table"), (k_descale, "k_descale"), (v_descale, "v_descale"))
    _need_device([(q, "q"), (k_cache, "k_cache"), (v_cache, "v_cache"), (cache_seqlens, "cache_seqlens")]
                 + [(t, name) for t, name in optional if t is not None], q, "q's")
    if q.dtype not in (torch.float16, torch.bfloat16):
        raise RuntimeError("Only fp16 and bf16 are supported")
    cache = _CacheSide(k_cache, v_cache, cache_seqlens, block_table, k_descale, v_descale, "batch", "q's")
    fp8 = cache.dtypes(like=q)
    if q.dim() != 4 or k_cache.dim() != 4 or k_cache.shape != v_cache.shape or k_cache.shape[3] != q.shape[3]:
        raise RuntimeError("q must have shape (batch, seqlen_q, n_heads, d_head), k_cache and v_cache one shape (batch or "
                           "num_pages, seqlen_cache or page_size, n_kv_heads, d_head)")
    batch, seqlen_q, n_heads, d_head = q.shape
    cache.lengths(batch, "q's batch size")
    cache.table(batch, max_seqlen_k)
    cache.descales(batch)
    if _decode_needs_copy(q):
        q = q.contiguous()
    cache.strides()
    fields = dict(
        dtype=15 if q.dtype == torch.bfloat16 else 5, causal=1 if causal else 0, num_splits=int(num_splits),
        q=q.data_ptr(), k=k_cache.data_ptr(), v=v_cache.data_ptr(),
        batch=batch, seqlen_q=seqlen_q, n_heads=n_heads, n_kv_heads=k_cache.shape[2], d_head=d_head,
        max_seqlen_k=0 if max_seqlen_k is None else max_seqlen_k,
        q_batch_stride=q.stride(0), q_seq_stride=q.stride(1), q_head_stride=q.stride(2),
        o_batch_stride=seqlen_q * n_heads * d_head, o_seq_stride=n_heads * d_head, o_head_stride=d_head,   # (o: contiguous)
        kv_batch_stride=k_cache.stride(0), kv_seq_stride=k_cache.stride(1), kv_head_stride=k_cache.stride(2), **cache.geometry(),
    )
    if not fp8:
        return q, _capi.make_decode_args(**fields), False
    args = _capi.make_decode_fp8_args(
        k_descale=k_descale.data_ptr() if k_descale is not None else None,
        v_descale=v_descale.data_ptr() if v_descale is not None else None,
        descale_batch_stride=k_cache.shape[2], **fields)
    return q, args, True


def append_kvcache(k_cache, v_cache, k, v, cache_seqlens, block_table=None, q=None, rotary_cos=None, rotary_sin=None,
                   rotary_interleaved=False, causal=False, k_descale=None, v_descale=None, seqlens_out=None):
    """The step in front of a decode (fa_kvcache_append_launch): write the new rows k, v (batch, seqlen_new, n_kv_heads, 128) into
    the cache IN PLACE at positions cache_seqlens[b] + t (contiguous, or paged through block_table; a token past the capacity is
    dropped), rotate the new keys -- and q, into a new tensor -- with rotary_cos / rotary_sin (seqlen_ro, rotary_dim / 2) of q's
    dtype, quantize for a torch.float8_e4m3fn cache with k_descale / v_descale (the bytes of quantize_kvcache_fp8's expression), and
    write min(cache_seqlens + seqlen_new, capacity) to seqlens_out (None: a new tensor; cache_seqlens itself: in place).
    q row i is rotated at position cache_seqlens[b] + i with causal, else at cache_seqlens[b].  -> (seqlens_out, q_rot or None).
    One kernel on the current stream; the host reads no device array; graph-capturable."""
    _need_tensors(((k_cache, "k_cache"), (v_cache, "v_cache"), (k, "k"), (v, "v"), (cache_seqlens, "cache_seqlens")))
    rotary = rotary_cos is not None or rotary_sin is not None
    if rotary and (rotary_cos is None or rotary_sin is None):
        raise RuntimeError("rotary_cos and rotary_sin come together")
    if q is not None and not rotary:
        raise RuntimeError("q is given without rotary_cos / rotary_sin: there is nothing to do to it")
    dev = k_cache.device
    named = [(k_cache, "k_cache"), (v_cache, "v_cache"), (k, "k"), (v, "v"), (cache_seqlens, "cache_seqlens"), (block_table, "block_table"),
             (q, "q"), (rotary_cos, "rotary_cos"), (rotary_sin, "rotary_sin"), (k_descale, "k_descale"), (v_descale, "v_descale"),
             (seqlens_out, "seqlens_out")]
    _need_device([(t, name) for t, name in named if t is not None], k_cache, "k_cache's")
    if k.dtype not in (torch.float16, torch.bfloat16):
        raise RuntimeError("Only fp16 and bf16 are supported")
    if v.dtype != k.dtype or any(t is not None and t.dtype != k.dtype for t in (q, rotary_cos, rotary_sin)):
        raise RuntimeError("Input tensors must have the same data type (k, v, q, rotary_cos, rotary_sin)")
    if k_cache.dtype != v_cache.dtype:   # (this path also compares two 16-bit caches)
        raise RuntimeError(f"k_cache and v_cache must have one data type (got {k_cache.dtype} and {v_cache.dtype})")
    cache = _CacheSide(k_cache, v_cache, cache_seqlens, block_table, k_descale, v_descale, "batch", "the cache's")
    fp8 = cache.dtypes(like=k)
    if k.dim() != 4 or k.shape != v.shape or k_cache.dim() != 4 or k_cache.shape != v_cache.shape or k_cache.shape[2:] != k.shape[2:]:
        raise RuntimeError("k and v must have one shape (batch, seqlen_new, n_kv_heads, d_head), k_cache and v_cache one shape (batch or "
                           "num_pages, seqlen_cache or page_size, n_kv_heads, d_head)")
    batch, seqlen_new, n_kv_heads, d_head = k.shape
    cache.lengths(batch, "k's batch size")
    if seqlens_out is not None and (seqlens_out.dtype != torch.int32 or tuple(seqlens_out.shape) != (batch,) or not seqlens_out.is_contiguous()):
        raise RuntimeError("seqlens_out must be a contiguous int32 tensor of batch entries on the cache's device (or cache_seqlens itself)")
    cache.table(batch)
    cache.descales(batch)
    if rotary:
        if rotary_cos.dim() != 2 or rotary_cos.shape != rotary_sin.shape or rotary_cos.shape[0] < 1:
            raise RuntimeError("rotary_cos and rotary_sin must have one shape (seqlen_ro, rotary_dim / 2)")
        rotary_dim = 2 * rotary_cos.shape[1]
        if rotary_dim % 16 != 0 or not 16 <= rotary_dim <= d_head:
            raise RuntimeError(f"rotary_dim (2 * rotary_cos.shape[1] = {rotary_dim}) must be a multiple of 16 in [16, {d_head}]")
        if _decode_needs_copy(rotary_cos) or _decode_needs_copy(rotary_sin) or rotary_cos.stride() != rotary_sin.stride():
            rotary_cos, rotary_sin = rotary_cos.contiguous(), rotary_sin.contiguous()
    if q is not None:
        if q.dim() != 4 or q.shape[0] != batch or q.shape[3] != d_head or q.shape[2] % n_kv_heads != 0:
            raise RuntimeError("q must have shape (batch, seqlen_q, n_heads, d_head) with k's batch and d_head and n_heads a multiple of n_kv_heads")
        if _decode_needs_copy(q):
            q = q.contiguous()
    if _decode_needs_copy(k) or _decode_needs_copy(v) or k.stride() != v.stride():
        k, v = k.contiguous(), v.contiguous()
    cache.strides()
    with torch.cuda.device(dev):
        if seqlens_out is None:
            seqlens_out = torch.empty_like(cache_seqlens)
        q_out = torch.empty(q.shape, dtype=q.dtype, device=dev) if q is not None else None
        args = _capi.make_kvcache_append_args(
            dtype=15 if k.dtype == torch.bfloat16 else 5, kv_dtype=_capi.FA_KV_FP8_E4M3FN if fp8 else 0, causal=1 if causal else 0,
            rotary_interleaved=1 if rotary_interleaved else 0,
            k_new=k.data_ptr(), v_new=v.data_ptr(), k=k_cache.data_ptr(), v=v_cache.data_ptr(),
            q=q.data_ptr() if q is not None else None, q_out=q_out.data_ptr() if q is not None else None,
            rotary_cos=rotary_cos.data_ptr() if rotary else None, rotary_sin=rotary_sin.data_ptr() if rotary else None,
            seqlens_out=seqlens_out.data_ptr(),
            k_descale=k_descale.data_ptr() if k_descale is not None else None,
            v_descale=v_descale.data_ptr() if v_descale is not None else None,
            batch=batch, seqlen_new=seqlen_new, seqlen_q=q.shape[1] if q is not None else 0, n_heads=q.shape[2] if q is not None else 0,
            n_kv_heads=n_kv_heads, d_head=d_head,
            rotary_dim=rotary_dim if rotary else 0, seqlen_ro=rotary_cos.shape[0] if rotary else 0,
            rotary_seq_stride=rotary_cos.stride(0) if rotary else 0,
            new_batch_stride=k.stride(0), new_seq_stride=k.stride(1), new_head_stride=k.stride(2),
            kv_batch_stride=k_cache.stride(0), kv_seq_stride=k_cache.stride(1), kv_head_stride=k_cache.stride(2),
            descale_batch_stride=n_kv_heads, **cache.geometry(),
        )
        if q is not None:
            args.q_batch_stride, args.q_seq_stride, args.q_head_stride = q.stride(0), q.stride(1), q.stride(2)
            args.qo_batch_stride, args.qo_seq_stride, args.qo_head_stride = q_out.stride(0), q_out.stride(1), q_out.stride(2)
        stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        _capi.check(_capi.load().fa_kvcache_append_launch(ctypes.byref(args), stream, None))
    return seqlens_out, q_out


def forward_kvcache(q, k_cache, v_cache, cache_seqlens, block_table=None, causal=False, return_lse=False, max_seqlen_k=None,
                    num_splits=0, timed=False, k_descale=None, v_descale=None, window_size=(-1, -1), k=None, v=None, rotary_cos=None,
                    rotary_sin=None, rotary_interleaved=False, advance_seqlens=False):
    """Decode attention against a K / V cache (fa_decode_launch): q (batch, seqlen_q, n_heads, 128); k_cache, v_cache
    (batch, seqlen_cache, n_kv_heads, 128), or with block_table (batch, max_pages_per_seq) int32 on the device
    (num_pages, page_size, n_kv_heads, 128); cache_seqlens (batch,) int32 on the device, the valid keys of each entry (the
    newest tokens included).  causal is bottom-right aligned.  -> o [, lse fp32 (batch, n_heads, seqlen_q)] [, ms].  The host
    reads neither cache_seqlens nor block_table; no device synchronisation unless timed.  The caches pass as they are (strided
    views included) and are refused if the launch cannot address them; q is copied if it has to be.
    A torch.float8_e4m3fn cache takes fa_decode_fp8_launch: k_descale, v_descale (fp32 (batch, n_kv_heads) on the device, None = 1;
    never read by the host) scale the cache's values, key j of entry b and K / V head h standing for float(k8[j]) * k_descale[b, h].
    With k, v (batch, seqlen_new, n_kv_heads, 128): cache_seqlens counts the keys BEFORE this call (flash-attn's meaning);
    append_kvcache writes the new rows first (rotating them and q with rotary_cos / rotary_sin, quantizing for an fp8 cache), and
    the attention runs over cache_seqlens + seqlen_new keys with the rotated q, on the same stream.  advance_seqlens writes the new
    lengths into cache_seqlens in place (one captured graph is then a whole decode step).  max_seqlen_k bounds the lengths after
    the append; timed's ms stays the decode's alone.
    window_size=(left, right), Python ints, -1 = unbounded: query row i, at position p = len - seqlen_q + i, sees the keys
    max(0, p - left) .. min(len - 1, p + right); causal means right = 0.  (-1, -1) takes the entry points above unchanged, anything
    else fa_decode_window_launch / fa_decode_fp8_window_launch, which fetch nothing below the lowest key a row sees.  With k / v
    the window applies to the lengths after the append.  Bad values are a ValueError.
    (Logit soft-capping: forward_kvcache_softcap, the same call with a softcap.)"""
    return _forward_kvcache(q, k_cache, v_cache, cache_seqlens, block_table, causal, return_lse, max_seqlen_k, num_splits, timed, k_descale,
                            v_descale, _window(window_size, causal), k, v, rotary_cos, rotary_sin, rotary_interleaved, advance_seqlens, None)


def forward_kvcache_softcap(q, k_cache, v_cache, cache_seqlens, softcap, block_table=None, causal=False, return_lse=False,
                            max_seqlen_k=None, num_splits=0, timed=False, k_descale=None, v_descale=None, window_size=(-1, -1), k=None,
                            v=None, rotary_cos=None, rotary_sin=None, rotary_interleaved=False, advance_seqlens=False):
    """forward_kvcache with logit soft-capping (fa_decode_softcap_launch, fa_decode_fp8_softcap_launch for an fp8 cache): every other
    argument is forward_kvcache's, with its meaning, checks and defaults.  softcap, required, a Python float or int, finite and >= 0
    (flash-attn's): the logit of a key the row sees becomes softcap * tanh(s / softcap), s = q . k / sqrt(128) on the dequantized
    key; masked keys stay -inf, lse is the log-sum-exp of the capped logits.  0 is off: forward_kvcache with the same arguments, the
    same entry points and bits.  Anything else goes through the capped entry points with the window, (-1, -1) included; the split
    count and the workspace are the windowed entry's.  With k / v the append runs first, unchanged: the cap belongs to the attention
    only.  A bad window_size is reported first, then a bad softcap: both a ValueError before any tensor is looked at."""
    window = _window(window_size, causal)
    return _forward_kvcache(q, k_cache, v_cache, cache_seqlens, block_table, causal, return_lse, max_seqlen_k, num_splits, timed, k_descale,
                            v_descale, window, k, v, rotary_cos, rotary_sin, rotary_interleaved, advance_seqlens, _softcap(softcap))


def _forward_kvcache(q, k_cache, v_cache, cache_seqlens, block_table, causal, return_lse, max_seqlen_k, num_splits, timed, k_descale,
                     v_descale, window, k, v, rotary_cos, rotary_sin, rotary_interleaved, advance_seqlens, cap):
    """The one body of forward_kvcache (cap None) and forward_kvcache_softcap (cap a float, or None for 0); window: _window's."""
    if k is not None or v is not None or rotary_cos is not None or rotary_sin is not None or advance_seqlens:
        if k is None or v is None:
            raise RuntimeError("k and v come together; rotary_cos / rotary_sin and advance_seqlens need them (the append is what they act on)")
        rotary = rotary_cos is not None or rotary_sin is not None
        if rotary and causal and k.dim() == 4 and q.dim() == 4 and k.shape[1] != q.shape[1]:
            raise RuntimeError(f"rotary with causal needs seqlen_new == seqlen_q (got {k.shape[1]} and {q.shape[1]}): query row i is "
                               "rotated at the position of new key i")
        if q.dim() == 4 and k.dim() == 4 and q.shape[0] != k.shape[0]:
            raise RuntimeError("k and v need q's batch size")
        cache_seqlens, q_rot = append_kvcache(k_cache, v_cache, k, v, cache_seqlens, block_table=block_table, q=q if rotary else None,
                                              rotary_cos=rotary_cos, rotary_sin=rotary_sin, rotary_interleaved=rotary_interleaved,
                                              causal=causal, k_descale=k_descale, v_descale=v_descale,
                                              seqlens_out=cache_seqlens if advance_seqlens else None)
        if rotary:
            q = q_rot
    q, args, fp8 = _decode_args(q, k_cache, v_cache, cache_seqlens, block_table, causal, max_seqlen_k, num_splits, k_descale, v_descale)
    batch, seqlen_q, n_heads, d_head = q.shape
    o = torch.empty((batch, seqlen_q, n_heads, d_head), dtype=q.dtype, device=q.device)
    lse = torch.empty((batch, n_heads, seqlen_q), dtype=torch.float32, device=q.device) if return_lse else None
    args.o, args.lse = o.data_ptr(), (lse.data_ptr() if return_lse else None)
    lib = _capi.load()
    if cap is not None:   # (the capped entry points always take a window: (-1, -1) is none)
        w, sc = _capi.make_window(*(window or (-1, -1))), _capi.make_softcap(cap)
        # (no workspace query of their own: the windowed entry's bytes for the same arguments are what the launch asks for)
        sized, run = ((lib.fa_decode_fp8_window_workspace_bytes, lib.fa_decode_fp8_softcap_launch) if fp8 else
                      (lib.fa_decode_window_workspace_bytes, lib.fa_decode_softcap_launch))
        workspace_bytes = lambda a: sized(a, ctypes.byref(w))                                           # noqa: E731
        launch = lambda a, stream, ms: run(a, ctypes.byref(w), ctypes.byref(sc), stream, ms)            # noqa: E731
    elif window is None:
        workspace_bytes, launch = ((lib.fa_decode_fp8_workspace_bytes, lib.fa_decode_fp8_launch) if fp8 else
                                   (lib.fa_decode_workspace_bytes, lib.fa_decode_launch))
    else:
        w = _capi.make_window(*window)
        sized, run = ((lib.fa_decode_fp8_window_workspace_bytes, lib.fa_decode_fp8_window_launch) if fp8 else
                      (lib.fa_decode_window_workspace_bytes, lib.fa_decode_window_launch))
        workspace_bytes = lambda a: sized(a, ctypes.byref(w))                         # noqa: E731
        launch = lambda a, stream, ms: run(a, ctypes.byref(w), stream, ms)            # noqa: E731
    nbytes = workspace_bytes(ctypes.byref(args))
    _capi.check(nbytes if nbytes < 0 else 0)
    with torch.cuda.device(q.device):
        workspace = torch.empty(nbytes, dtype=torch.uint8, device=q.device) if nbytes > 0 else None   # (on the current stream's allocator)
        args.workspace = workspace.data_ptr() if workspace is not None else None
        stream = ctypes.c_void_p(torch.cuda.current_stream(q.device).cuda_stream)
        ms = ctypes.c_float(0.0)
        _capi.check(launch(ctypes.byref(args), stream, ctypes.byref(ms) if timed else None))
    out = (o, lse) if return_lse else (o,)
    if timed:
        out = out + (float(ms.value),)
    return out[0] if len(out) == 1 else out


def forward_varlen_kvcache(q, k_cache, v_cache, cu_seqlens_q, max_seqlen_q, cache_seqlens, block_table=None, causal=False,
                           max_seqlen_k=None, timed=False, k_descale=None, v_descale=None, *, window_size=(-1, -1), softcap=0.0):
    """Prefill against a K / V cache (fa_fwd_launch_varlen_kvcache): forward_varlen(cu_seqlens_k=) whose keys are read from the
    cache in place.  q (total_q, n_heads, 128) packed, cu_seqlens_q an int32 device tensor of n_seqs + 1 row offsets, max_seqlen_q
    a Python int; k_cache, v_cache (n_seqs, seqlen_cache, n_kv_heads, 128), or with block_table (n_seqs, max_pages_per_seq) int32 on
    the device (num_pages, page_size, n_kv_heads, 128); cache_seqlens (n_seqs,) int32 on the device, the valid keys of each
    sequence, the chunk's own (already appended) included.  causal is bottom-right aligned.  -> (o, lse[, ms]); o contiguous, lse
    fp32 (n_heads, total_q).  The host reads no device array; no device synchronisation unless timed.  The caches pass as they
    are and are refused if the launch cannot address them.
    A torch.float8_e4m3fn cache takes fa_fwd_launch_varlen_kvcache_fp8 when BOTH k_descale and v_descale are given: fp32
    (n_seqs, n_kv_heads) on q's device, last dimension contiguous, never read by the host; key j of sequence b (the sequence, also
    for a paged cache) and K / V head h stands for float(k8[j]) * k_descale[b, h], likewise V.  Unlike forward_kvcache, where None
    means 1, an fp8 cache with a descale missing is refused here: pass tensors of ones for an unscaled cache.  A descale with a
    16-bit cache is refused.
    window_size=(left, right), keyword only, Python ints, -1 = unbounded: forward_kvcache's rule with len_q for seqlen_q -- query
    row r of sequence b, at position p = r + (len_k - len_q), sees the keys max(0, p - left) .. min(len_k - 1, p + right); causal
    means right = 0.  (-1, -1) takes the entry points above unchanged, anything else fa_fwd_launch_varlen_kvcache_window /
    fa_fwd_launch_varlen_kvcache_fp8_window: a Q block visits only the key tiles of its rows' windows, and no cache row, page
    or block_table entry wholly below the sequence's lowest visible key max(0, len_k - len_q - left) is read.  Bad values are a
    ValueError, before any tensor is looked at.
    softcap, keyword only, a Python float or int, finite and >= 0 (forward_varlen's): the logit of a key the row sees becomes
    softcap * tanh(s / softcap), s = q . k / sqrt(128) on the dequantized key; masked keys stay -inf, lse is the log-sum-exp of the
    capped logits.  0 is off: the call above, the same entry points and bits.  Anything else goes through
    fa_fwd_launch_varlen_kvcache_softcap / fa_fwd_launch_varlen_kvcache_fp8_softcap with the window, (-1, -1) included.  A bad
    window_size is reported first, then a bad softcap."""
    window = _window(window_size, causal)
    cap = _softcap(softcap)
    tensors = [(q, "q"), (k_cache, "k_cache"), (v_cache, "v_cache"), (cu_seqlens_q, "cu_seqlens_q"), (cache_seqlens, "cache_seqlens")]
    if block_table is not None:
        tensors.append((block_table, "block_table"))
    _need_tensors(tensors)
    cache = _CacheSide(k_cache, v_cache, cache_seqlens, block_table, k_descale, v_descale, "n_seqs", "q's")
    fp8 = cache.dtypes(like=None, fp8_needs_descales=(
        "forward_varlen_kvcache: an fp8 cache is not served without both k_descale and v_descale (fp32 (n_seqs, "
        "n_kv_heads) tensors on q's device; pass ones for an unscaled cache -- None does not mean 1 here)"))
    if fp8:
        tensors += [(k_descale, "k_descale"), (v_descale, "v_descale")]
        _need_tensors(tensors[-2:])
        if k_cache.dim() == 4 and cu_seqlens_q.dim() == 1 and cu_seqlens_q.numel() >= 2:   # (what they are is checked before where they are)
            want = (cu_seqlens_q.numel() - 1, k_cache.shape[2])
            for t, name in tensors[-2:]:
                if t.dtype != torch.float32 or tuple(t.shape) != want or t.stride(1) != 1:
                    raise RuntimeError(f"{name} must be an fp32 (n_seqs, n_kv_heads) = {want} tensor on q's device with a contiguous "
                                       "last dimension")
    _need_device(tensors, q, "q's")
    if q.dtype not in (torch.float16, torch.bfloat16):
        raise RuntimeError("Only fp16 and bf16 are supported")
    if not fp8 and (k_cache.dtype != q.dtype or v_cache.dtype != q.dtype):
        raise RuntimeError("Input tensors must have the same data type")
    if q.dim() != 3 or k_cache.dim() != 4 or k_cache.shape != v_cache.shape or k_cache.shape[3] != q.shape[2]:
        raise RuntimeError("q must have shape (total_q, n_heads, d_head), k_cache and v_cache one shape (n_seqs or num_pages, "
                           "seqlen_cache or page_size, n_kv_heads, d_head)")
    total, n_heads, d_head = q.shape
    n_kv = k_cache.shape[2]
    if n_kv < 1 or n_heads % n_kv != 0:
        raise RuntimeError(f"grouped-query attention: the K / V heads ({n_kv}) must divide the query heads ({n_heads})")
    if cu_seqlens_q.dtype != torch.int32 or cu_seqlens_q.dim() != 1 or cu_seqlens_q.numel() < 2 or not cu_seqlens_q.is_contiguous():
        raise RuntimeError("cu_seqlens_q must be a contiguous int32 tensor of n_seqs + 1 entries on q's device")
    n_seqs = cu_seqlens_q.numel() - 1
    if not isinstance(max_seqlen_q, int) or isinstance(max_seqlen_q, bool):
        raise RuntimeError("max_seqlen_q must be a Python int (a bound on every sequence's query rows; the device is not asked)")
    cache.lengths(n_seqs, "one batch entry per sequence")
    cache.table(n_seqs, max_seqlen_k)
    if q.stride(2) != 1:
        raise RuntimeError("packed sequences: q needs a contiguous last dimension")
    cache.strides()
    if fp8 and (k_descale.stride(0) != v_descale.stride(0) or k_descale.stride(0) < n_kv or k_descale.data_ptr() % 4 or v_descale.data_ptr() % 4):
        # (the launch has one row stride for both, at least a row long -- an expanded or single row has any: two small copies)
        k_descale, v_descale = k_descale.contiguous(), v_descale.contiguous()
    lib = _capi.load()
    cfg = _capi.make_config(varlen_config(q.dtype))
    with torch.cuda.device(q.device):
        o = torch.empty((total, n_heads, d_head), dtype=q.dtype, device=q.device)
        lse = torch.empty((n_heads, total), dtype=torch.float32, device=q.device)
        if q.stride() != o.stride():   # (the launch has one stride set for q and o)
            q = q.contiguous()
        args = _capi.FaFwdArgs(q=q.data_ptr(), k=k_cache.data_ptr(), v=v_cache.data_ptr(), o=o.data_ptr(), batch=1, seq_len=total,
                               n_heads=n_heads, d_head=d_head, batch_stride=0, seq_stride=q.stride(0), head_stride=q.stride(1), cfg=cfg)
        kv = _capi.make_kv_layout(n_kv, k_cache.stride(0), k_cache.stride(1), k_cache.stride(2))
        vq = _capi.make_varlen_layout(cu_seqlens_q.data_ptr(), n_seqs, total, max(max_seqlen_q, 1))   # (a bound of 0: nothing but empties)
        kc = _capi.make_kvcache_layout(batch=0 if cache.paged else k_cache.shape[0], max_seqlen_k=0 if max_seqlen_k is None else max_seqlen_k,
                                       **cache.geometry())
        ms = ctypes.c_float(0.0)
        opts = _capi.make_opts(causal=causal, ms=ms if timed else None)
        stream = ctypes.c_void_p(torch.cuda.current_stream(q.device).cuda_stream)
        # (a window goes in front of opts, and picks the entry point's _window form; a cap behind it picks the _softcap form, which
        # always takes a window: (-1, -1) is none)
        form = "" if window is None else "_window"
        w = [ctypes.byref(_capi.make_window(*window))] if window is not None else []
        if cap is not None:
            form = "_softcap"
            w = [ctypes.byref(_capi.make_window(*(window or (-1, -1)))), ctypes.byref(_capi.make_softcap(cap))]
        tail = w + [ctypes.byref(opts), ctypes.c_void_p(lse.data_ptr()), stream]
        if fp8:
            sc = _capi.make_kvcache_fp8_scales(k_descale=k_descale.data_ptr(), v_descale=v_descale.data_ptr(),
                                               descale_batch_stride=k_descale.stride(0))
            launch = getattr(lib, "fa_fwd_launch_varlen_kvcache_fp8" + form)
            _capi.check(launch(ctypes.byref(args), ctypes.byref(kv), ctypes.byref(vq), ctypes.byref(kc), ctypes.byref(sc), *tail))
        else:
            launch = getattr(lib, "fa_fwd_launch_varlen_kvcache" + form)
            _capi.check(launch(ctypes.byref(args), ctypes.byref(kv), ctypes.byref(vq), ctypes.byref(kc), *tail))
    return (o, lse, float(ms.value)) if timed else (o, lse)


def quantize_kvcache_fp8(k, v):
    """A contiguous 16-bit (or fp32) cache (batch, seqlen_cache, n_kv_heads, d_head) -> (k8, v8, k_descale, v_descale): e4m3fn
    caches of the same shape and fp32 (batch, n_kv_heads) descales, amax / 448 per (batch entry, K / V head) -- 448 is e4m3fn's
    largest finite value -- and 1 for an all-zero head.  Plain torch (callers, tests, the bench); value ~ float(x8) * descale."""
    def one(t):
        if t.dim() != 4:
            raise RuntimeError("quantize_kvcache_fp8 takes (batch, seqlen_cache, n_kv_heads, d_head) tensors")
        x = t.float()
        amax = x.abs().amax(dim=(1, 3))
        descale = torch.where(amax > 0, amax / 448.0, torch.ones_like(amax))
        x8 = (x / descale[:, None, :, None]).clamp(-448.0, 448.0).to(torch.float8_e4m3fn)
        return x8, descale.contiguous()
    k8, k_descale = one(k)
    v8, v_descale = one(v)
    return k8, v8, k_descale, v_descale
