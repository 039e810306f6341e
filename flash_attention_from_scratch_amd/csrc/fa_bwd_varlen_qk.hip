// fa_bwd_varlen_qk.hip -- the translation unit of the backward over packed sequences with separate Q and K / V lengths: the
// kernels of fa_bwd_varlen.hpp in their two-range form (BwdVarlenQKArgs) for both dtypes and both masks, behind the header's
// enqueue of one backward (bwd_varlen_enqueue_any).  Shapes and pointers are validated by the caller (fa_bwd_launch_varlen_qk,
// fa_capi.hip).  The flags of fa_bwd_varlen.hip: same contraction, same bits.
#include <hip/hip_runtime.h>

#include "fa_bwd_varlen.hpp"

namespace fa {

hipError_t bwd_varlen_qk_enqueue(const BwdVarlenQKArgs &a, int dtype, bool causal, hipStream_t s) {
    if (dtype == 15) return causal ? bwd_varlen_enqueue_any<BwdVarlenQKArgs, 15, true>(a, s) : bwd_varlen_enqueue_any<BwdVarlenQKArgs, 15, false>(a, s);
    return causal ? bwd_varlen_enqueue_any<BwdVarlenQKArgs, 5, true>(a, s) : bwd_varlen_enqueue_any<BwdVarlenQKArgs, 5, false>(a, s);
}

}  // namespace fa
