"""ctypes binding of libfa_hip.so (include/fa_hip.h).  No torch imports here.

This is the stub INTEGRATION.md shows for the reference side: the reference's
pybind entry (src/flash_attention.cu:137-140) reduces to filling ``fa_fwd_args``
and calling ``fa_fwd_launch``.
"""

import ctypes
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# FA_HIP_LIB: another build of the same library (tests/test_gpu_parity.py runs the timing-perturbed FA_JITTER build,
# lib/libfa_hip_jitter.so, through the same binding).  Not a fallback: the named file must exist.
LIB_PATH = os.environ.get("FA_HIP_LIB") or os.path.join(_HERE, "lib", "libfa_hip.so")

FA_FP16, FA_BF16 = 5, 15

CONFIG_FIELDS = (
    "dtype", "d_head", "B_r", "B_c", "n_warps", "async_copy", "eager_load_blocks",
    "swizzled", "Q_mma_load_K_tiles", "K_mma_load_K_tiles", "V_mma_load_K_tiles",
    "mma_double_buffer_loads", "optimized_softmax",
)

# every symbol include/fa_hip.h declares (tests check the library exports them all)
EXPORTED_SYMBOLS = (
    "fa_init", "fa_fwd_supported", "fa_fwd_lds_bytes", "fa_fwd_launch",
    "fa_fwd_launch_timed", "fa_num_kernels", "fa_get_kernel", "fa_last_error", "fa_version",
    "fa_fwd_masked_supported", "fa_fwd_launch_masked", "fa_device_state",
    "fa_fwd_ex_supported", "fa_fwd_launch_ex", "fa_fwd_query",
    "fa_adaptive_state", "fa_adaptive_state_for", "fa_adaptive_reset", "fa_adaptive_simulate", "fa_get_kernel_sized", "fa_fwd_query_sized", "fa_abi_version",
    "fa_fwd_lse_supported", "fa_fwd_launch_lse", "fa_bwd_workspace_bytes", "fa_bwd_launch",
    "fa_fwd_gqa_supported", "fa_fwd_launch_gqa", "fa_bwd_gqa_workspace_bytes", "fa_bwd_launch_gqa",
    "fa_fwd_varlen_supported", "fa_fwd_launch_varlen", "fa_bwd_varlen_workspace_bytes", "fa_bwd_launch_varlen",
    "fa_fwd_varlen_qk_supported", "fa_fwd_launch_varlen_qk", "fa_bwd_varlen_qk_workspace_bytes", "fa_bwd_launch_varlen_qk",
    "fa_decode_supported", "fa_decode_num_splits", "fa_decode_workspace_bytes", "fa_decode_launch",
    "fa_decode_fp8_supported", "fa_decode_fp8_num_splits", "fa_decode_fp8_workspace_bytes", "fa_decode_fp8_launch",
    "fa_kvcache_append_launch",
    "fa_fwd_varlen_kvcache_supported", "fa_fwd_launch_varlen_kvcache",
    "fa_fwd_varlen_kvcache_fp8_supported", "fa_fwd_launch_varlen_kvcache_fp8",
    "fa_decode_window_supported", "fa_decode_window_num_splits", "fa_decode_window_workspace_bytes", "fa_decode_window_launch",
    "fa_decode_fp8_window_supported", "fa_decode_fp8_window_num_splits", "fa_decode_fp8_window_workspace_bytes",
    "fa_decode_fp8_window_launch",
    "fa_fwd_varlen_qk_window_supported", "fa_fwd_launch_varlen_qk_window",
    "fa_fwd_varlen_kvcache_window_supported", "fa_fwd_launch_varlen_kvcache_window",
    "fa_fwd_varlen_kvcache_fp8_window_supported", "fa_fwd_launch_varlen_kvcache_fp8_window",
    "fa_bwd_launch_varlen_qk_window",
    "fa_fwd_varlen_qk_softcap_supported", "fa_fwd_launch_varlen_qk_softcap", "fa_bwd_launch_varlen_qk_softcap",
    "fa_fwd_varlen_qk_sinks_supported", "fa_fwd_launch_varlen_qk_sinks", "fa_bwd_varlen_qk_sinks_workspace_bytes",
    "fa_bwd_launch_varlen_qk_sinks",
    "fa_fwd_varlen_kvcache_softcap_supported", "fa_fwd_launch_varlen_kvcache_softcap",
    "fa_fwd_varlen_kvcache_fp8_softcap_supported", "fa_fwd_launch_varlen_kvcache_fp8_softcap",
    "fa_decode_softcap_supported", "fa_decode_softcap_num_splits", "fa_decode_softcap_launch",
    "fa_decode_fp8_softcap_supported", "fa_decode_fp8_softcap_num_splits", "fa_decode_fp8_softcap_launch",
)
FA_KV_FP8_E4M3FN = 1  # fa_kv_dtype
FA_SPECULATIVE_OFF, FA_SPECULATIVE_ALWAYS, FA_SPECULATIVE_ADAPTIVE = 0, 1, 2  # fa_speculative_mode
FA_ABI_VERSION = 6
SOFTMAX_MODES = ("eager", "first_block_skip", "lazy", "speculative")  # fa_softmax_mode


class FaFwdConfig(ctypes.Structure):
    _fields_ = [(name, ctypes.c_int32) for name in CONFIG_FIELDS]


class FaFwdArgs(ctypes.Structure):
    _fields_ = [
        ("q", ctypes.c_void_p), ("k", ctypes.c_void_p), ("v", ctypes.c_void_p),
        ("o", ctypes.c_void_p),
        ("batch", ctypes.c_int64), ("seq_len", ctypes.c_int64), ("n_heads", ctypes.c_int64),
        ("d_head", ctypes.c_int64),
        ("batch_stride", ctypes.c_int64), ("seq_stride", ctypes.c_int64),
        ("head_stride", ctypes.c_int64),
        ("cfg", FaFwdConfig),
    ]


class FaKernelInfo(ctypes.Structure):
    _fields_ = [
        ("cfg", FaFwdConfig), ("threads", ctypes.c_int32), ("lds_bytes", ctypes.c_int32),
        ("num_regs", ctypes.c_int32), ("scratch_bytes", ctypes.c_int32),
        ("rows_per_wave", ctypes.c_int32), ("masked", ctypes.c_int32),
        ("softmax_mode", ctypes.c_int32), ("prescaled_q", ctypes.c_int32),
        # ABI 5: the ring form of a 32-rows-per-wave configuration (include/fa_hip.h)
        ("ring_form", ctypes.c_int32), ("ring_softmax_mode", ctypes.c_int32),
        ("ring_num_regs", ctypes.c_int32), ("ring_scratch_bytes", ctypes.c_int32),
        ("ring_lds_bytes", ctypes.c_int32), ("persistent", ctypes.c_int32), ("alt_form", ctypes.c_int32),
        ("ring_threads", ctypes.c_int32),
    ]


class FaFwdStats(ctypes.Structure):
    """fa_fwd_stats: two uint32 counters in DEVICE memory the kernel adds to."""

    _fields_ = [("items", ctypes.c_uint32), ("items_redone", ctypes.c_uint32)]


class FaFwdOpts(ctypes.Structure):
    """fa_fwd_opts: the extensions of fa_fwd_launch_ex (zero = the reference's launch)."""

    _fields_ = [
        ("struct_size", ctypes.c_uint32), ("causal", ctypes.c_int32), ("allow_ragged", ctypes.c_int32),
        ("speculative", ctypes.c_int32), ("prescaled_q", ctypes.c_int32),
        ("ms", ctypes.POINTER(ctypes.c_float)), ("stats", ctypes.c_void_p),
    ]


class FaBwdArgs(ctypes.Structure):   # fa_bwd_args
    _fields_ = [
        ("q", ctypes.c_void_p), ("k", ctypes.c_void_p), ("v", ctypes.c_void_p),
        ("o", ctypes.c_void_p), ("dout", ctypes.c_void_p), ("lse", ctypes.POINTER(ctypes.c_float)),
        ("dq", ctypes.c_void_p), ("dk", ctypes.c_void_p), ("dv", ctypes.c_void_p), ("workspace", ctypes.c_void_p),
        ("batch", ctypes.c_int64), ("seq_len", ctypes.c_int64), ("n_heads", ctypes.c_int64), ("d_head", ctypes.c_int64),
        ("qkv_batch_stride", ctypes.c_int64), ("qkv_seq_stride", ctypes.c_int64), ("qkv_head_stride", ctypes.c_int64),
        ("out_batch_stride", ctypes.c_int64), ("out_seq_stride", ctypes.c_int64), ("out_head_stride", ctypes.c_int64),
        ("dtype", ctypes.c_int32), ("causal", ctypes.c_int32),
    ]


class FaKvLayout(ctypes.Structure):   # fa_kv_layout (grouped-query attention: K's and V's heads and strides)
    _fields_ = [
        ("struct_size", ctypes.c_uint32), ("n_kv_heads", ctypes.c_int64),
        ("kv_batch_stride", ctypes.c_int64), ("kv_seq_stride", ctypes.c_int64), ("kv_head_stride", ctypes.c_int64),
    ]


class FaBwdGqaArgs(ctypes.Structure):   # fa_bwd_gqa_args
    _fields_ = [
        ("base", FaBwdArgs), ("n_kv_heads", ctypes.c_int64),
        ("kv_batch_stride", ctypes.c_int64), ("kv_seq_stride", ctypes.c_int64), ("kv_head_stride", ctypes.c_int64),
        ("dkv_batch_stride", ctypes.c_int64), ("dkv_seq_stride", ctypes.c_int64), ("dkv_head_stride", ctypes.c_int64),
    ]


class FaVarlenLayout(ctypes.Structure):   # fa_varlen_layout (packed sequences: cu_seqlens on the device, and the host's bounds)
    _fields_ = [
        ("struct_size", ctypes.c_uint32), ("cu_seqlens", ctypes.c_void_p),
        ("n_seqs", ctypes.c_int64), ("total_tokens", ctypes.c_int64), ("max_seqlen", ctypes.c_int64),
    ]


class FaBwdVarlenArgs(ctypes.Structure):   # fa_bwd_varlen_args
    _fields_ = [
        ("q", ctypes.c_void_p), ("k", ctypes.c_void_p), ("v", ctypes.c_void_p),
        ("o", ctypes.c_void_p), ("dout", ctypes.c_void_p), ("lse", ctypes.POINTER(ctypes.c_float)),
        ("dq", ctypes.c_void_p), ("dk", ctypes.c_void_p), ("dv", ctypes.c_void_p), ("workspace", ctypes.c_void_p),
        ("n_heads", ctypes.c_int64), ("n_kv_heads", ctypes.c_int64), ("d_head", ctypes.c_int64),
        ("q_seq_stride", ctypes.c_int64), ("q_head_stride", ctypes.c_int64),
        ("out_seq_stride", ctypes.c_int64), ("out_head_stride", ctypes.c_int64),
        ("kv_seq_stride", ctypes.c_int64), ("kv_head_stride", ctypes.c_int64),
        ("dkv_seq_stride", ctypes.c_int64), ("dkv_head_stride", ctypes.c_int64),
        ("dtype", ctypes.c_int32), ("causal", ctypes.c_int32),
        ("varlen", FaVarlenLayout),
    ]


class FaBwdVarlenQKArgs(ctypes.Structure):   # fa_bwd_varlen_qk_args (varlen: the query rows; varlen_k: the key rows)
    _fields_ = [("struct_size", ctypes.c_uint32)] + FaBwdVarlenArgs._fields_ + [("varlen_k", FaVarlenLayout)]


class FaDecodeArgs(ctypes.Structure):   # fa_decode_args (KV-cache decode: contiguous or paged cache, lengths on the device)
    _fields_ = [
        ("struct_size", ctypes.c_uint32), ("dtype", ctypes.c_int32), ("causal", ctypes.c_int32), ("num_splits", ctypes.c_int32),
        ("q", ctypes.c_void_p), ("k", ctypes.c_void_p), ("v", ctypes.c_void_p), ("o", ctypes.c_void_p), ("lse", ctypes.c_void_p),
        ("cache_seqlens", ctypes.c_void_p), ("block_table", ctypes.c_void_p), ("workspace", ctypes.c_void_p),
        ("batch", ctypes.c_int64), ("seqlen_q", ctypes.c_int64), ("n_heads", ctypes.c_int64), ("n_kv_heads", ctypes.c_int64),
        ("d_head", ctypes.c_int64), ("seqlen_cache", ctypes.c_int64), ("num_pages", ctypes.c_int64), ("page_size", ctypes.c_int64),
        ("max_pages_per_seq", ctypes.c_int64), ("block_table_stride", ctypes.c_int64), ("max_seqlen_k", ctypes.c_int64),
        ("q_batch_stride", ctypes.c_int64), ("q_seq_stride", ctypes.c_int64), ("q_head_stride", ctypes.c_int64),
        ("o_batch_stride", ctypes.c_int64), ("o_seq_stride", ctypes.c_int64), ("o_head_stride", ctypes.c_int64),
        ("kv_batch_stride", ctypes.c_int64), ("kv_seq_stride", ctypes.c_int64), ("kv_head_stride", ctypes.c_int64),
    ]


def make_decode_args(**fields):
    """fa_decode_args with struct_size set; d_head defaults to 128, everything not given to 0 / null."""
    a = FaDecodeArgs(struct_size=ctypes.sizeof(FaDecodeArgs), d_head=128)
    for name, value in fields.items():
        setattr(a, name, value)
    return a


class FaDecodeFp8Args(ctypes.Structure):   # fa_decode_fp8_args (fa_decode_args' fields, then the fp8 cache's descales and encoding)
    _fields_ = FaDecodeArgs._fields_ + [
        ("k_descale", ctypes.c_void_p), ("v_descale", ctypes.c_void_p), ("descale_batch_stride", ctypes.c_int64),
        ("kv_dtype", ctypes.c_int32),
    ]


def make_decode_fp8_args(**fields):
    """fa_decode_fp8_args with struct_size set; d_head defaults to 128, kv_dtype to e4m3fn, everything not given to 0 / null."""
    a = FaDecodeFp8Args(struct_size=ctypes.sizeof(FaDecodeFp8Args), d_head=128, kv_dtype=FA_KV_FP8_E4M3FN)
    for name, value in fields.items():
        setattr(a, name, value)
    return a


class FaWindow(ctypes.Structure):   # fa_window (sliding-window attention: keys seen below / above a row's position, -1 = unbounded)
    _fields_ = [("struct_size", ctypes.c_uint32), ("left", ctypes.c_int32), ("right", ctypes.c_int32)]


def make_window(left=-1, right=-1):
    return FaWindow(struct_size=ctypes.sizeof(FaWindow), left=left, right=right)


class FaSoftcap(ctypes.Structure):   # fa_softcap (logit soft-capping: softcap * tanh(s / softcap), softcap > 0 and finite)
    _fields_ = [("struct_size", ctypes.c_uint32), ("softcap", ctypes.c_float)]


def make_softcap(softcap):
    return FaSoftcap(struct_size=ctypes.sizeof(FaSoftcap), softcap=softcap)


class FaSinks(ctypes.Structure):   # fa_sinks (learned attention sinks: one fp32 logit per query head in the softmax's denominator)
    _fields_ = [("struct_size", ctypes.c_uint32), ("n_heads", ctypes.c_int32), ("sinks", ctypes.c_void_p)]


def make_sinks(sinks_ptr, n_heads):
    return FaSinks(struct_size=ctypes.sizeof(FaSinks), n_heads=n_heads, sinks=sinks_ptr)


class FaKvcacheAppendArgs(ctypes.Structure):   # fa_kvcache_append_args (the append / rotary / quantize / advance step in front of a decode)
    _fields_ = [
        ("struct_size", ctypes.c_uint32), ("dtype", ctypes.c_int32), ("kv_dtype", ctypes.c_int32), ("causal", ctypes.c_int32),
        ("rotary_interleaved", ctypes.c_int32),
        ("k_new", ctypes.c_void_p), ("v_new", ctypes.c_void_p), ("k", ctypes.c_void_p), ("v", ctypes.c_void_p),
        ("q", ctypes.c_void_p), ("q_out", ctypes.c_void_p), ("rotary_cos", ctypes.c_void_p), ("rotary_sin", ctypes.c_void_p),
        ("cache_seqlens", ctypes.c_void_p), ("seqlens_out", ctypes.c_void_p), ("block_table", ctypes.c_void_p),
        ("k_descale", ctypes.c_void_p), ("v_descale", ctypes.c_void_p),
        ("batch", ctypes.c_int64), ("seqlen_new", ctypes.c_int64), ("seqlen_q", ctypes.c_int64), ("n_heads", ctypes.c_int64),
        ("n_kv_heads", ctypes.c_int64), ("d_head", ctypes.c_int64), ("seqlen_cache", ctypes.c_int64), ("num_pages", ctypes.c_int64),
        ("page_size", ctypes.c_int64), ("max_pages_per_seq", ctypes.c_int64), ("block_table_stride", ctypes.c_int64),
        ("rotary_dim", ctypes.c_int64), ("seqlen_ro", ctypes.c_int64), ("rotary_seq_stride", ctypes.c_int64),
        ("new_batch_stride", ctypes.c_int64), ("new_seq_stride", ctypes.c_int64), ("new_head_stride", ctypes.c_int64),
        ("q_batch_stride", ctypes.c_int64), ("q_seq_stride", ctypes.c_int64), ("q_head_stride", ctypes.c_int64),
        ("qo_batch_stride", ctypes.c_int64), ("qo_seq_stride", ctypes.c_int64), ("qo_head_stride", ctypes.c_int64),
        ("kv_batch_stride", ctypes.c_int64), ("kv_seq_stride", ctypes.c_int64), ("kv_head_stride", ctypes.c_int64),
        ("descale_batch_stride", ctypes.c_int64),
    ]


def make_kvcache_append_args(**fields):
    """fa_kvcache_append_args with struct_size set; d_head defaults to 128, everything not given to 0 / null."""
    a = FaKvcacheAppendArgs(struct_size=ctypes.sizeof(FaKvcacheAppendArgs), d_head=128)
    for name, value in fields.items():
        setattr(a, name, value)
    return a


class FaKvcacheLayout(ctypes.Structure):   # fa_kvcache_layout (the key side of a prefill: a contiguous or paged cache, lengths on the device)
    _fields_ = [
        ("struct_size", ctypes.c_uint32), ("cache_seqlens", ctypes.c_void_p), ("block_table", ctypes.c_void_p),
        ("seqlen_cache", ctypes.c_int64), ("num_pages", ctypes.c_int64), ("page_size", ctypes.c_int64),
        ("max_pages_per_seq", ctypes.c_int64), ("block_table_stride", ctypes.c_int64), ("max_seqlen_k", ctypes.c_int64),
        ("batch", ctypes.c_int64),
    ]


def make_kvcache_layout(**fields):
    """fa_kvcache_layout with struct_size set; everything not given is 0 / null."""
    a = FaKvcacheLayout(struct_size=ctypes.sizeof(FaKvcacheLayout))
    for name, value in fields.items():
        setattr(a, name, value)
    return a


class FaKvcacheFp8Scales(ctypes.Structure):   # fa_kvcache_fp8_scales (the fp8 side of a prefill against an fp8 cache: encoding and descales)
    _fields_ = [
        ("struct_size", ctypes.c_uint32), ("kv_dtype", ctypes.c_int32), ("k_descale", ctypes.c_void_p), ("v_descale", ctypes.c_void_p),
        ("descale_batch_stride", ctypes.c_int64),
    ]


def make_kvcache_fp8_scales(**fields):
    """fa_kvcache_fp8_scales with struct_size set; kv_dtype defaults to e4m3fn, everything not given to 0 / null."""
    a = FaKvcacheFp8Scales(struct_size=ctypes.sizeof(FaKvcacheFp8Scales), kv_dtype=FA_KV_FP8_E4M3FN)
    for name, value in fields.items():
        setattr(a, name, value)
    return a


def make_varlen_layout(cu_seqlens_ptr, n_seqs, total_tokens, max_seqlen):
    return FaVarlenLayout(struct_size=ctypes.sizeof(FaVarlenLayout), cu_seqlens=cu_seqlens_ptr, n_seqs=n_seqs,
                          total_tokens=total_tokens, max_seqlen=max_seqlen)


def make_kv_layout(n_kv_heads, batch_stride, seq_stride, head_stride):
    return FaKvLayout(struct_size=ctypes.sizeof(FaKvLayout), n_kv_heads=n_kv_heads, kv_batch_stride=batch_stride,
                      kv_seq_stride=seq_stride, kv_head_stride=head_stride)


class FaAdaptiveInfo(ctypes.Structure):
    """fa_adaptive_info: the adaptive speculative mode's record on one device."""

    _fields_ = [(name, ctypes.c_uint32) for name in
                ("available", "launches", "demoted", "reports", "hold", "mode", "remaining", "last_report")]


def make_opts(causal=False, allow_ragged=False, speculative=False, prescaled_q=False, ms=None, stats_ptr=None):
    """`speculative`: False / True, or "adaptive" (= 2, FA_SPECULATIVE_ADAPTIVE)."""
    o = FaFwdOpts()
    o.struct_size = ctypes.sizeof(FaFwdOpts)
    o.causal, o.allow_ragged = int(bool(causal)), int(bool(allow_ragged))
    adaptive = speculative == "adaptive" or (not isinstance(speculative, bool) and speculative == FA_SPECULATIVE_ADAPTIVE)
    o.speculative = FA_SPECULATIVE_ADAPTIVE if adaptive else int(bool(speculative))
    o.prescaled_q = int(bool(prescaled_q))
    if ms is not None:
        o.ms = ctypes.pointer(ms)
    o.stats = stats_ptr
    return o


class FaError(RuntimeError):
    """Non-zero fa_status; message from fa_last_error() (RuntimeError like TORCH_CHECK)."""

    def __init__(self, status, message):
        super().__init__(message)
        self.status = status


_lib = None


def load():
    """Load libfa_hip.so or fail loudly -- there is no CPU / eager fallback."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"{LIB_PATH} is missing: the HIP extension is not built. Run "
            "`python -c 'import __graft_entry__ as g; g.build()'` or "
            "`make -C flash_attention_from_scratch_amd/csrc`. "
            "flash_attention has no fallback path."
        )
    lib = ctypes.CDLL(LIB_PATH)
    cfg_p, args_p = ctypes.POINTER(FaFwdConfig), ctypes.POINTER(FaFwdArgs)
    lib.fa_init.restype = ctypes.c_int
    lib.fa_init.argtypes = []
    lib.fa_device_state.restype = ctypes.c_int
    lib.fa_device_state.argtypes = [ctypes.c_int] + [ctypes.POINTER(ctypes.c_int)] * 3
    lib.fa_fwd_supported.restype = ctypes.c_int
    lib.fa_fwd_supported.argtypes = [cfg_p]
    lib.fa_fwd_lds_bytes.restype = ctypes.c_int
    lib.fa_fwd_lds_bytes.argtypes = [cfg_p]
    lib.fa_fwd_launch.restype = ctypes.c_int
    lib.fa_fwd_launch.argtypes = [args_p, ctypes.c_void_p]
    lib.fa_fwd_launch_timed.restype = ctypes.c_int
    lib.fa_fwd_launch_timed.argtypes = [args_p, ctypes.c_void_p, ctypes.POINTER(ctypes.c_float)]
    lib.fa_fwd_masked_supported.restype = ctypes.c_int
    lib.fa_fwd_masked_supported.argtypes = [cfg_p]
    lib.fa_fwd_launch_masked.restype = ctypes.c_int
    lib.fa_fwd_launch_masked.argtypes = [args_p, ctypes.c_int, ctypes.c_void_p, ctypes.POINTER(ctypes.c_float)]
    lib.fa_fwd_ex_supported.restype = ctypes.c_int
    lib.fa_fwd_ex_supported.argtypes = [cfg_p, ctypes.POINTER(FaFwdOpts)]
    lib.fa_fwd_query.restype = ctypes.c_int
    lib.fa_fwd_query.argtypes = [cfg_p, ctypes.POINTER(FaFwdOpts), ctypes.POINTER(FaKernelInfo)]
    lib.fa_fwd_launch_ex.restype = ctypes.c_int
    lib.fa_fwd_launch_ex.argtypes = [args_p, ctypes.POINTER(FaFwdOpts), ctypes.c_void_p]
    lib.fa_num_kernels.restype = ctypes.c_int
    lib.fa_num_kernels.argtypes = []
    lib.fa_get_kernel.restype = ctypes.c_int
    lib.fa_get_kernel.argtypes = [ctypes.c_int, ctypes.POINTER(FaKernelInfo)]
    lib.fa_adaptive_state.restype = ctypes.c_int
    lib.fa_adaptive_state.argtypes = [ctypes.c_int, ctypes.POINTER(FaAdaptiveInfo)]
    lib.fa_adaptive_state_for.restype = ctypes.c_int
    lib.fa_adaptive_state_for.argtypes = [ctypes.c_int, ctypes.POINTER(FaFwdConfig), ctypes.POINTER(FaFwdOpts), ctypes.POINTER(FaAdaptiveInfo)]
    lib.fa_adaptive_reset.restype = ctypes.c_int
    lib.fa_adaptive_reset.argtypes = [ctypes.c_int]
    lib.fa_adaptive_simulate.restype = ctypes.c_int
    lib.fa_adaptive_simulate.argtypes = [ctypes.c_int, ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_int32),
                                         ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(FaAdaptiveInfo)]
    lib.fa_get_kernel_sized.restype = ctypes.c_int
    lib.fa_get_kernel_sized.argtypes = [ctypes.c_int, ctypes.POINTER(FaKernelInfo), ctypes.c_uint32]
    lib.fa_fwd_query_sized.restype = ctypes.c_int
    lib.fa_fwd_query_sized.argtypes = [cfg_p, ctypes.POINTER(FaFwdOpts), ctypes.POINTER(FaKernelInfo), ctypes.c_uint32]
    lib.fa_abi_version.restype = ctypes.c_int
    lib.fa_abi_version.argtypes = []
    lib.fa_fwd_lse_supported.restype = ctypes.c_int
    lib.fa_fwd_lse_supported.argtypes = [cfg_p, ctypes.POINTER(FaFwdOpts)]
    lib.fa_fwd_launch_lse.restype = ctypes.c_int
    lib.fa_fwd_launch_lse.argtypes = [args_p, ctypes.POINTER(FaFwdOpts), ctypes.c_void_p, ctypes.c_void_p]
    lib.fa_bwd_workspace_bytes.restype = ctypes.c_int64
    lib.fa_bwd_workspace_bytes.argtypes = [ctypes.POINTER(FaBwdArgs)]
    lib.fa_bwd_launch.restype = ctypes.c_int
    lib.fa_bwd_launch.argtypes = [ctypes.POINTER(FaBwdArgs), ctypes.c_void_p, ctypes.POINTER(ctypes.c_float)]
    lib.fa_fwd_gqa_supported.restype = ctypes.c_int
    lib.fa_fwd_gqa_supported.argtypes = [cfg_p, ctypes.POINTER(FaFwdOpts)]
    lib.fa_fwd_launch_gqa.restype = ctypes.c_int
    lib.fa_fwd_launch_gqa.argtypes = [args_p, ctypes.POINTER(FaKvLayout), ctypes.POINTER(FaFwdOpts), ctypes.c_void_p, ctypes.c_void_p]
    lib.fa_bwd_gqa_workspace_bytes.restype = ctypes.c_int64
    lib.fa_bwd_gqa_workspace_bytes.argtypes = [ctypes.POINTER(FaBwdGqaArgs)]
    lib.fa_bwd_launch_gqa.restype = ctypes.c_int
    lib.fa_bwd_launch_gqa.argtypes = [ctypes.POINTER(FaBwdGqaArgs), ctypes.c_void_p, ctypes.POINTER(ctypes.c_float)]
    lib.fa_fwd_varlen_supported.restype = ctypes.c_int
    lib.fa_fwd_varlen_supported.argtypes = [cfg_p, ctypes.POINTER(FaFwdOpts)]
    lib.fa_fwd_launch_varlen.restype = ctypes.c_int
    lib.fa_fwd_launch_varlen.argtypes = [args_p, ctypes.POINTER(FaKvLayout), ctypes.POINTER(FaVarlenLayout), ctypes.POINTER(FaFwdOpts),
                                         ctypes.c_void_p, ctypes.c_void_p]
    lib.fa_bwd_varlen_workspace_bytes.restype = ctypes.c_int64
    lib.fa_bwd_varlen_workspace_bytes.argtypes = [ctypes.POINTER(FaBwdVarlenArgs)]
    lib.fa_bwd_launch_varlen.restype = ctypes.c_int
    lib.fa_bwd_launch_varlen.argtypes = [ctypes.POINTER(FaBwdVarlenArgs), ctypes.c_void_p, ctypes.POINTER(ctypes.c_float)]
    lib.fa_fwd_varlen_qk_supported.restype = ctypes.c_int
    lib.fa_fwd_varlen_qk_supported.argtypes = [cfg_p, ctypes.POINTER(FaFwdOpts)]
    lib.fa_fwd_launch_varlen_qk.restype = ctypes.c_int
    lib.fa_fwd_launch_varlen_qk.argtypes = [args_p, ctypes.POINTER(FaKvLayout), ctypes.POINTER(FaVarlenLayout), ctypes.POINTER(FaVarlenLayout),
                                            ctypes.POINTER(FaFwdOpts), ctypes.c_void_p, ctypes.c_void_p]
    lib.fa_fwd_varlen_kvcache_supported.restype = ctypes.c_int
    lib.fa_fwd_varlen_kvcache_supported.argtypes = [cfg_p, ctypes.POINTER(FaFwdOpts)]
    lib.fa_fwd_launch_varlen_kvcache.restype = ctypes.c_int
    lib.fa_fwd_launch_varlen_kvcache.argtypes = [args_p, ctypes.POINTER(FaKvLayout), ctypes.POINTER(FaVarlenLayout),
                                                 ctypes.POINTER(FaKvcacheLayout), ctypes.POINTER(FaFwdOpts), ctypes.c_void_p, ctypes.c_void_p]
    lib.fa_bwd_varlen_qk_workspace_bytes.restype = ctypes.c_int64
    lib.fa_bwd_varlen_qk_workspace_bytes.argtypes = [ctypes.POINTER(FaBwdVarlenQKArgs)]
    lib.fa_bwd_launch_varlen_qk.restype = ctypes.c_int
    lib.fa_bwd_launch_varlen_qk.argtypes = [ctypes.POINTER(FaBwdVarlenQKArgs), ctypes.c_void_p, ctypes.POINTER(ctypes.c_float)]
    lib.fa_decode_supported.restype = ctypes.c_int
    lib.fa_decode_supported.argtypes = [ctypes.POINTER(FaDecodeArgs)]
    lib.fa_decode_num_splits.restype = ctypes.c_int
    lib.fa_decode_num_splits.argtypes = [ctypes.POINTER(FaDecodeArgs)]
    lib.fa_decode_workspace_bytes.restype = ctypes.c_int64
    lib.fa_decode_workspace_bytes.argtypes = [ctypes.POINTER(FaDecodeArgs)]
    lib.fa_decode_launch.restype = ctypes.c_int
    lib.fa_decode_launch.argtypes = [ctypes.POINTER(FaDecodeArgs), ctypes.c_void_p, ctypes.POINTER(ctypes.c_float)]
    lib.fa_fwd_varlen_kvcache_fp8_supported.restype = ctypes.c_int
    lib.fa_fwd_varlen_kvcache_fp8_supported.argtypes = [cfg_p, ctypes.POINTER(FaFwdOpts)]
    lib.fa_fwd_launch_varlen_kvcache_fp8.restype = ctypes.c_int
    lib.fa_fwd_launch_varlen_kvcache_fp8.argtypes = [args_p, ctypes.POINTER(FaKvLayout), ctypes.POINTER(FaVarlenLayout),
                                                     ctypes.POINTER(FaKvcacheLayout), ctypes.POINTER(FaKvcacheFp8Scales),
                                                     ctypes.POINTER(FaFwdOpts), ctypes.c_void_p, ctypes.c_void_p]
    lib.fa_decode_fp8_supported.restype = ctypes.c_int
    lib.fa_decode_fp8_supported.argtypes = [ctypes.POINTER(FaDecodeFp8Args)]
    lib.fa_decode_fp8_num_splits.restype = ctypes.c_int
    lib.fa_decode_fp8_num_splits.argtypes = [ctypes.POINTER(FaDecodeFp8Args)]
    lib.fa_decode_fp8_workspace_bytes.restype = ctypes.c_int64
    lib.fa_decode_fp8_workspace_bytes.argtypes = [ctypes.POINTER(FaDecodeFp8Args)]
    lib.fa_decode_fp8_launch.restype = ctypes.c_int
    lib.fa_decode_fp8_launch.argtypes = [ctypes.POINTER(FaDecodeFp8Args), ctypes.c_void_p, ctypes.POINTER(ctypes.c_float)]
    for name, args_t in (("fa_decode_window", FaDecodeArgs), ("fa_decode_fp8_window", FaDecodeFp8Args)):
        pair = [ctypes.POINTER(args_t), ctypes.POINTER(FaWindow)]
        for suffix, restype, more in (("supported", ctypes.c_int, []), ("num_splits", ctypes.c_int, []),
                                      ("workspace_bytes", ctypes.c_int64, []),
                                      ("launch", ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(ctypes.c_float)])):
            fn = getattr(lib, f"{name}_{suffix}")
            fn.restype, fn.argtypes = restype, pair + more
    # the sliding-window forms of the packed forward and the prefills: the sibling's arguments with an fa_window in front of opts
    for name, sibling in (("varlen_qk_window", "varlen_qk"), ("varlen_kvcache_window", "varlen_kvcache"),
                          ("varlen_kvcache_fp8_window", "varlen_kvcache_fp8")):
        fn = getattr(lib, f"fa_fwd_{name}_supported")
        fn.restype, fn.argtypes = ctypes.c_int, [cfg_p, ctypes.POINTER(FaFwdOpts)]
        fn, argtypes = getattr(lib, f"fa_fwd_launch_{name}"), list(getattr(lib, f"fa_fwd_launch_{sibling}").argtypes)
        fn.restype, fn.argtypes = ctypes.c_int, argtypes[:-3] + [ctypes.POINTER(FaWindow)] + argtypes[-3:]
    # ... and of the packed backward: the sibling's arguments with an fa_window behind them
    lib.fa_bwd_launch_varlen_qk_window.restype = ctypes.c_int
    lib.fa_bwd_launch_varlen_qk_window.argtypes = [ctypes.POINTER(FaBwdVarlenQKArgs), ctypes.POINTER(FaWindow), ctypes.c_void_p,
                                                   ctypes.POINTER(ctypes.c_float)]
    # the soft-capped forms of the two: the windowed sibling's arguments with an fa_softcap behind the fa_window
    lib.fa_fwd_varlen_qk_softcap_supported.restype = ctypes.c_int
    lib.fa_fwd_varlen_qk_softcap_supported.argtypes = [cfg_p, ctypes.POINTER(FaFwdOpts)]
    argtypes = list(lib.fa_fwd_launch_varlen_qk_window.argtypes)
    lib.fa_fwd_launch_varlen_qk_softcap.restype = ctypes.c_int
    lib.fa_fwd_launch_varlen_qk_softcap.argtypes = argtypes[:-3] + [ctypes.POINTER(FaSoftcap)] + argtypes[-3:]
    argtypes = list(lib.fa_bwd_launch_varlen_qk_window.argtypes)
    lib.fa_bwd_launch_varlen_qk_softcap.restype = ctypes.c_int
    lib.fa_bwd_launch_varlen_qk_softcap.argtypes = argtypes[:2] + [ctypes.POINTER(FaSoftcap)] + argtypes[2:]
    # the forms with attention sinks: the windowed sibling's arguments with an fa_sinks behind the fa_window, in the backward
    # dsinks (n_heads fp32 on the device) behind that; the backward has a workspace query of its own (the two-range one's value)
    lib.fa_fwd_varlen_qk_sinks_supported.restype = ctypes.c_int
    lib.fa_fwd_varlen_qk_sinks_supported.argtypes = [cfg_p, ctypes.POINTER(FaFwdOpts)]
    argtypes = list(lib.fa_fwd_launch_varlen_qk_window.argtypes)
    lib.fa_fwd_launch_varlen_qk_sinks.restype = ctypes.c_int
    lib.fa_fwd_launch_varlen_qk_sinks.argtypes = argtypes[:-3] + [ctypes.POINTER(FaSinks)] + argtypes[-3:]
    lib.fa_bwd_varlen_qk_sinks_workspace_bytes.restype = ctypes.c_int64
    lib.fa_bwd_varlen_qk_sinks_workspace_bytes.argtypes = [ctypes.POINTER(FaBwdVarlenQKArgs)]
    argtypes = list(lib.fa_bwd_launch_varlen_qk_window.argtypes)
    lib.fa_bwd_launch_varlen_qk_sinks.restype = ctypes.c_int
    lib.fa_bwd_launch_varlen_qk_sinks.argtypes = argtypes[:2] + [ctypes.POINTER(FaSinks), ctypes.c_void_p] + argtypes[2:]
    # ... and of both cache prefills and both decodes: again the windowed sibling's arguments with an fa_softcap behind the fa_window
    for name in ("varlen_kvcache", "varlen_kvcache_fp8"):
        fn = getattr(lib, f"fa_fwd_{name}_softcap_supported")
        fn.restype, fn.argtypes = ctypes.c_int, [cfg_p, ctypes.POINTER(FaFwdOpts)]
        fn, argtypes = getattr(lib, f"fa_fwd_launch_{name}_softcap"), list(getattr(lib, f"fa_fwd_launch_{name}_window").argtypes)
        fn.restype, fn.argtypes = ctypes.c_int, argtypes[:-3] + [ctypes.POINTER(FaSoftcap)] + argtypes[-3:]
    for name in ("fa_decode", "fa_decode_fp8"):
        for suffix in ("supported", "num_splits", "launch"):   # (sized by the windowed sibling's workspace query)
            fn, sibling = getattr(lib, f"{name}_softcap_{suffix}"), getattr(lib, f"{name}_window_{suffix}")
            fn.restype, fn.argtypes = sibling.restype, sibling.argtypes[:2] + [ctypes.POINTER(FaSoftcap)] + sibling.argtypes[2:]
    lib.fa_kvcache_append_launch.restype = ctypes.c_int
    lib.fa_kvcache_append_launch.argtypes = [ctypes.POINTER(FaKvcacheAppendArgs), ctypes.c_void_p, ctypes.POINTER(ctypes.c_float)]
    lib.fa_last_error.restype = ctypes.c_char_p
    lib.fa_last_error.argtypes = []
    lib.fa_version.restype = ctypes.c_char_p
    lib.fa_version.argtypes = []
    _lib = lib
    return lib


def last_error():
    return load().fa_last_error().decode("utf-8", "replace")


def check(status):
    if status < 0:
        raise FaError(status, last_error())
    return status


def make_config(kernel_cfg) -> FaFwdConfig:
    """Read the 13 attributes by name, as the reference does (flash_attention.cu:16-32).
    `dtype` may be a DType (IntEnum) or anything int() accepts."""
    values = {}
    for name in CONFIG_FIELDS:
        values[name] = int(getattr(kernel_cfg, name))
    return FaFwdConfig(**values)


def supported(kernel_cfg) -> bool:
    cfg = make_config(kernel_cfg)
    return bool(load().fa_fwd_supported(ctypes.byref(cfg)))


def masked_supported(kernel_cfg) -> bool:
    cfg = make_config(kernel_cfg)
    return bool(load().fa_fwd_masked_supported(ctypes.byref(cfg)))


def ex_supported(kernel_cfg, **opts) -> bool:
    """fa_fwd_ex_supported: is there a device variant for the config with these fa_fwd_opts
    (causal, allow_ragged, speculative, prescaled_q)?"""
    cfg = make_config(kernel_cfg)
    o = make_opts(**opts)
    return bool(load().fa_fwd_ex_supported(ctypes.byref(cfg), ctypes.byref(o)))


def query(kernel_cfg, **opts) -> FaKernelInfo:
    """fa_fwd_query: the device variant that serves the config with these fa_fwd_opts (raises FaError if none)."""
    cfg = make_config(kernel_cfg)
    o = make_opts(**opts)
    info = FaKernelInfo()
    check(load().fa_fwd_query(ctypes.byref(cfg), ctypes.byref(o), ctypes.byref(info)))
    return info


def lds_bytes(kernel_cfg) -> int:
    cfg = make_config(kernel_cfg)
    return check(load().fa_fwd_lds_bytes(ctypes.byref(cfg)))


def kernels():
    """List of FaKernelInfo for every device variant in the library."""
    lib = load()
    out = []
    for i in range(lib.fa_num_kernels()):
        info = FaKernelInfo()
        check(lib.fa_get_kernel(i, ctypes.byref(info)))
        out.append(info)
    return out


def version() -> str:
    return load().fa_version().decode()


def device_state(device: int):
    """(inited, status, num_cus) of libfa_hip.so's per-device setup for `device` (fa_device_state)."""
    a, b, c = ctypes.c_int(0), ctypes.c_int(0), ctypes.c_int(0)
    check(load().fa_device_state(int(device), ctypes.byref(a), ctypes.byref(b), ctypes.byref(c)))
    return bool(a.value), b.value, c.value


def adaptive_state(device: int, kernel_cfg=None, **opts) -> dict:
    """fa_adaptive_state: the adaptive speculative mode's records on `device` taken together, as a dict; with
    `kernel_cfg` (and causal= / allow_ragged= / prescaled_q=) fa_adaptive_state_for: the record of the one device variant
    that serves that configuration (records are per variant since ABI 5)."""
    info = FaAdaptiveInfo()
    if kernel_cfg is None:
        check(load().fa_adaptive_state(int(device), ctypes.byref(info)))
    else:
        cfg = make_config(kernel_cfg)
        o = make_opts(**opts)
        check(load().fa_adaptive_state_for(int(device), ctypes.byref(cfg), ctypes.byref(o), ctypes.byref(info)))
    return {name: int(getattr(info, name)) for name, _ in FaAdaptiveInfo._fields_}


def adaptive_reset(device: int) -> None:
    check(load().fa_adaptive_reset(int(device)))


def adaptive_simulate(report_word, probe_state):
    """fa_adaptive_simulate: the adaptive policy on a fresh state, scripted -- launch i sees report_word[i] and
    probe_state[i] (-1 none, 0 pending, 1 complete, 2 error).  -> ([run_i], final state dict); run: 0 speculative,
    1 demoted, 2 probe."""
    n = len(report_word)
    assert len(probe_state) == n
    rep = (ctypes.c_uint32 * n)(*report_word)
    prb = (ctypes.c_int32 * n)(*probe_state)
    run = (ctypes.c_int32 * n)()
    info = FaAdaptiveInfo()
    check(load().fa_adaptive_simulate(n, rep, prb, run, ctypes.byref(info)))
    return list(run), {name: int(getattr(info, name)) for name, _ in FaAdaptiveInfo._fields_}
