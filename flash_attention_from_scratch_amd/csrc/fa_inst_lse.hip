// fa_inst_lse.hip -- the persistent kernel's forms that also write the row log-sum-exp (fa_fwd_kernel64_lse: plain and causal,
// speculative and lazy; fa_fwd_launch_lse), one translation unit per dtype (-DFA_INST_DT=<5|15>).  FA_KERNEL64_LSE makes
// fa_fwd_kernel64.hpp define fa_fwd_kernel64_lse from the body of fa_fwd_kernel64 (which this unit then does not have).  Not
// in the registry: the launcher takes the twin of the entry fa_fwd_launch_ex would take (fa_capi.hip).
#define FA_KERNEL64_LSE
#include "fa_fwd_kernel64.hpp"

#ifndef FA_INST_DT
#error "define FA_INST_DT (5 = fp16, 15 = bf16)"
#endif

namespace fa {

#define FA_CAT2(a, b) a##b
#define FA_CAT(a, b) FA_CAT2(a, b)
kernel_fn_lse FA_CAT(lse_kernel_dt, FA_INST_DT)(bool masked, bool spec) {
    if (masked) return spec ? &fa_fwd_kernel64_lse<FA_INST_DT, true, true> : &fa_fwd_kernel64_lse<FA_INST_DT, true, false>;
    return spec ? &fa_fwd_kernel64_lse<FA_INST_DT, false, true> : &fa_fwd_kernel64_lse<FA_INST_DT, false, false>;
}

}  // namespace fa
