// fa_inst_varlen.hip -- the forward over packed variable-length sequences (fa_fwd_kernel_varlen; fa_fwd_launch_varlen,
// fa_fwd_launch_varlen_qk), one translation unit per dtype (-DFA_INST_DT=<5|15>).  FA_KERNEL_VARLEN makes fa_fwd_kernel.hpp
// define fa_fwd_kernel_varlen from the body of fa_fwd_kernel (which this unit then does not have): the masked
// 32-rows-per-wave kernel at the (B_r 128, B_c 64, 4 warps) + buffer shape, with and without the first-block skip -- the twins
// of the two masked entries of that shape.  Compiled with the flags of the slice that builds those entries, so that one
// contraction pattern gives one set of bits.  Not in the registry, like fa_inst_lse.hip.
#define FA_KERNEL_VARLEN
#include "fa_fwd_kernel.hpp"

#ifndef FA_INST_DT
#error "define FA_INST_DT (5 = fp16, 15 = bf16)"
#endif

namespace fa {

#define FA_CAT2(a, b) a##b
#define FA_CAT(a, b) FA_CAT2(a, b)
kernel_fn_varlen FA_CAT(varlen_kernel_dt, FA_INST_DT)(bool first_block_skip) {
    //                                                  DT          QT NW BC  SWZ   EAGER OPT   PIPE  DMA   MASK  D
    if (first_block_skip) return &fa_fwd_kernel_varlen<FA_INST_DT, 1, 4, 64, true, true, true, true, true, true, 128>;
    return &fa_fwd_kernel_varlen<FA_INST_DT, 1, 4, 64, true, true, false, true, true, true, 128>;
}
int FA_CAT(varlen_lds_bytes_dt, FA_INST_DT)() {
    return FwdTraits<FA_INST_DT, 1, 4, 64, true, true, false, true, true, true, 128>::kLdsBytes;
}

}  // namespace fa
