// fa_inst_gqa.hip -- the persistent kernel's grouped-query attention forms (fa_fwd_kernel64_gqa, fa_gqa64.inc: the LSE forms,
// plain and causal, speculative and lazy, with K / V heads and strides of their own; fa_fwd_launch_gqa), one translation unit
// per dtype (-DFA_INST_DT=<5|15>).  FA_KERNEL64_GQA makes fa_fwd_kernel64.hpp define fa_fwd_kernel64_gqa from the body of
// fa_fwd_kernel64 (which this unit then does not have, nor fa_fwd_kernel64_lse).  Not in the registry, like fa_inst_lse.hip.
#define FA_KERNEL64_LSE
#define FA_KERNEL64_GQA
#include "fa_fwd_kernel64.hpp"

#ifndef FA_INST_DT
#error "define FA_INST_DT (5 = fp16, 15 = bf16)"
#endif

namespace fa {

#define FA_CAT2(a, b) a##b
#define FA_CAT(a, b) FA_CAT2(a, b)
kernel_fn_gqa FA_CAT(gqa_kernel_dt, FA_INST_DT)(bool masked, bool spec) {
    if (masked) return spec ? &fa_fwd_kernel64_gqa<FA_INST_DT, true, true> : &fa_fwd_kernel64_gqa<FA_INST_DT, true, false>;
    return spec ? &fa_fwd_kernel64_gqa<FA_INST_DT, false, true> : &fa_fwd_kernel64_gqa<FA_INST_DT, false, false>;
}

}  // namespace fa
