// fa_inst_varlen_kvcache_fp8_softcap.hip -- the packed variable-length forward whose keys come from an fp8 (e4m3fn) KV cache,
// contiguous or paged, with logit soft-capping (fa_fwd_kernel_varlen_kvcache_fp8_softcap; fa_fwd_launch_varlen_kvcache_fp8_softcap),
// one translation unit per Q dtype (-DFA_INST_DT=<5|15>).  FA_KERNEL_VARLEN_SOFTCAP beside the windowed fp8 cache slice's four
// macros makes fa_fwd_kernel.hpp define that kernel from the text of fa_fwd_kernel_varlen_kvcache_fp8_window (which this unit then
// does not have) on the register-staged transport (DMA = false): the same two forms, with and without the first-block skip,
// compiled with the varlen slices' flags.  k_descale sits in the cap's constant here, not in the exponent's (fa_fwd_kernel.hpp).
// A slice of its own: the other cache slices keep their kernels and their code.  Not in the registry.
#define FA_KERNEL_VARLEN
#define FA_KERNEL_VARLEN_KVCACHE
#define FA_KERNEL_VARLEN_KVCACHE_FP8
#define FA_KERNEL_VARLEN_WINDOW
#define FA_KERNEL_VARLEN_SOFTCAP
#include "fa_fwd_kernel.hpp"

#ifndef FA_INST_DT
#error "define FA_INST_DT (5 = fp16, 15 = bf16)"
#endif

namespace fa {

#define FA_CAT2(a, b) a##b
#define FA_CAT(a, b) FA_CAT2(a, b)
kernel_fn_varlen_kvcache_fp8_softcap FA_CAT(varlen_kvcache_fp8_softcap_kernel_dt, FA_INST_DT)(bool first_block_skip) {
    //                                                                      DT          QT NW BC  SWZ   EAGER OPT   PIPE  DMA    MASK  D
    if (first_block_skip) return &fa_fwd_kernel_varlen_kvcache_fp8_softcap<FA_INST_DT, 1, 4, 64, true, true, true, true, false, true, 128>;
    return &fa_fwd_kernel_varlen_kvcache_fp8_softcap<FA_INST_DT, 1, 4, 64, true, true, false, true, false, true, 128>;
}

}  // namespace fa
