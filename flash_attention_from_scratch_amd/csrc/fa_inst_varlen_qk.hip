// fa_inst_varlen_qk.hip -- the forward over packed sequences with separate Q and K / V lengths (fa_fwd_kernel_varlen_qk;
// fa_fwd_launch_varlen_qk), one translation unit per dtype (-DFA_INST_DT=<5|15>).  FA_KERNEL_VARLEN_QK makes fa_fwd_kernel.hpp
// define fa_fwd_kernel_varlen_qk from the body of fa_fwd_kernel_varlen (which this unit then does not have, nor fa_fwd_kernel):
// the same two forms of the (B_r 128, B_c 64, 4 warps) + buffer shape, with and without the first-block skip.  Compiled with
// the flags of fa_inst_varlen.hip, so that equal Q and K ranges give that kernel's bits.  Not in the registry.
#define FA_KERNEL_VARLEN_QK
#include "fa_fwd_kernel.hpp"

#ifndef FA_INST_DT
#error "define FA_INST_DT (5 = fp16, 15 = bf16)"
#endif

namespace fa {

#define FA_CAT2(a, b) a##b
#define FA_CAT(a, b) FA_CAT2(a, b)
kernel_fn_varlen_qk FA_CAT(varlen_qk_kernel_dt, FA_INST_DT)(bool first_block_skip) {
    //                                                     DT          QT NW BC  SWZ   EAGER OPT   PIPE  DMA   MASK  D
    if (first_block_skip) return &fa_fwd_kernel_varlen_qk<FA_INST_DT, 1, 4, 64, true, true, true, true, true, true, 128>;
    return &fa_fwd_kernel_varlen_qk<FA_INST_DT, 1, 4, 64, true, true, false, true, true, true, 128>;
}

}  // namespace fa
