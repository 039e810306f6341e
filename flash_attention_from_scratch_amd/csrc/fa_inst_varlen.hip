// fa_inst_varlen.hip -- the forward over packed variable-length sequences, every form of it: one translation unit per form and
// dtype, -DFA_VARLEN_KEYS=<0|1|2> -DFA_VARLEN_EXTRA=<0|1|2|3> -DFA_INST_DT=<5|15> (csrc/Makefile: VARLEN_FORMS).
//   keys   0 packed keys (fa_fwd_launch_varlen, fa_fwd_launch_varlen_qk) | 1 a KV cache, contiguous or paged (..._kvcache) |
//          2 an fp8 (e4m3fn) KV cache (..._kvcache_fp8)
//   extra  0 nothing | 1 a sliding window (..._window) | 2 a sliding window and logit soft-capping (..._softcap) |
//          3 a sliding window and attention sinks (fa_fwd_launch_varlen_qk_sinks; packed keys only)
// The two numbers make fa_fwd_kernel.hpp define that form's kernel, fa_fwd_kernel_varlen<_kvcache|_kvcache_fp8><_window|_softcap|_sinks>,
// from the body of fa_fwd_kernel (which this unit then does not have): the masked 32-rows-per-wave kernel at the
// (B_r 128, B_c 64, 4 warps) + buffer shape, with and without the first-block skip -- the twins of the two masked entries of
// that shape.  Against an fp8 cache it runs on the register-staged transport (DMA = false: the DMA cannot convert).  Compiled
// with the flags of the slice that builds those entries, so that one contraction pattern gives one set of bits.  A slice per
// form: each form keeps its two kernels and its code whatever the others become.  Not in the registry, like fa_inst_lse.hip.
#if !defined(FA_VARLEN_KEYS) || !defined(FA_VARLEN_EXTRA) || !defined(FA_INST_DT)
#error "define FA_VARLEN_KEYS (0 = packed, 1 = KV cache, 2 = fp8 KV cache), FA_VARLEN_EXTRA (0 = none, 1 = window, 2 = softcap, 3 = sinks) and FA_INST_DT (5 = fp16, 15 = bf16)"
#endif
#include "fa_fwd_kernel.hpp"

namespace fa {

#define FA_CAT2(a, b) a##b
#define FA_CAT(a, b) FA_CAT2(a, b)
#define FA_VARLEN_DMA (FA_VARLEN_KEYS != 2)
FA_VARLEN_NAME(kernel_fn_varlen, ) FA_VARLEN_NAME(varlen, FA_CAT(_kernel_dt, FA_INST_DT))(bool first_block_skip) {
    //                                                                         DT          QT NW BC  SWZ   EAGER OPT   PIPE  DMA            MASK  D
    if (first_block_skip) return &FA_VARLEN_NAME(fa_fwd_kernel_varlen, )<FA_INST_DT, 1, 4, 64, true, true, true, true, FA_VARLEN_DMA, true, 128>;
    return &FA_VARLEN_NAME(fa_fwd_kernel_varlen, )<FA_INST_DT, 1, 4, 64, true, true, false, true, FA_VARLEN_DMA, true, 128>;
}
#if FA_VARLEN_KEYS == 0 && FA_VARLEN_EXTRA == 0
int FA_CAT(varlen_lds_bytes_dt, FA_INST_DT)() {   // (every form's LDS)
    return FwdTraits<FA_INST_DT, 1, 4, 64, true, true, false, true, true, true, 128>::kLdsBytes;
}
#endif

}  // namespace fa
