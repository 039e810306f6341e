// fa_inst_varlen_kvcache_fp8_window.hip -- the packed variable-length forward whose keys come from an fp8 (e4m3fn) KV cache,
// contiguous or paged, under a sliding window (fa_fwd_kernel_varlen_kvcache_fp8_window; fa_fwd_launch_varlen_kvcache_fp8_window),
// one translation unit per Q dtype (-DFA_INST_DT=<5|15>).  FA_KERNEL_VARLEN_WINDOW beside the fp8 cache slice's three macros makes
// fa_fwd_kernel.hpp define that kernel from the text of fa_fwd_kernel_varlen_kvcache_fp8 (which this unit then does not have) on
// the register-staged transport (DMA = false): the same two forms, with and without the first-block skip, compiled with the
// varlen slices' flags.  A slice of its own: the unwindowed slice keeps its two kernels and its code.  Not in the registry.
#define FA_KERNEL_VARLEN
#define FA_KERNEL_VARLEN_KVCACHE
#define FA_KERNEL_VARLEN_KVCACHE_FP8
#define FA_KERNEL_VARLEN_WINDOW
#include "fa_fwd_kernel.hpp"

#ifndef FA_INST_DT
#error "define FA_INST_DT (5 = fp16, 15 = bf16)"
#endif

namespace fa {

#define FA_CAT2(a, b) a##b
#define FA_CAT(a, b) FA_CAT2(a, b)
kernel_fn_varlen_kvcache_fp8_window FA_CAT(varlen_kvcache_fp8_window_kernel_dt, FA_INST_DT)(bool first_block_skip) {
    //                                                                     DT          QT NW BC  SWZ   EAGER OPT   PIPE  DMA    MASK  D
    if (first_block_skip) return &fa_fwd_kernel_varlen_kvcache_fp8_window<FA_INST_DT, 1, 4, 64, true, true, true, true, false, true, 128>;
    return &fa_fwd_kernel_varlen_kvcache_fp8_window<FA_INST_DT, 1, 4, 64, true, true, false, true, false, true, 128>;
}

}  // namespace fa
