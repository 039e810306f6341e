// fa_bwd_varlen_softcap.hip -- the translation unit of the backward over packed sequences with logit soft-capping: the kernels
// of fa_bwd_varlen.hpp in their soft-capped form (BwdVarlenSoftcapArgs: the window form plus the cap) for both dtypes, behind the
// header's enqueue of one backward (bwd_varlen_enqueue_any).  One instantiation per dtype: the window carries the causal
// mask as right = 0, and no window at all as left = right = 2^30.  Shapes, pointers, the window and the cap are validated by the
// caller (fa_bwd_launch_varlen_qk_softcap, fa_capi.hip).  The flags of fa_bwd_varlen.hip: same contraction.  A unit of its own, so
// that the other three slices keep their kernels.
#include <hip/hip_runtime.h>

#include "fa_bwd_varlen.hpp"

namespace fa {

hipError_t bwd_varlen_softcap_enqueue(const BwdVarlenSoftcapArgs &a, int dtype, hipStream_t s) {
    return dtype == 15 ? bwd_varlen_enqueue_any<BwdVarlenSoftcapArgs, 15, false>(a, s) : bwd_varlen_enqueue_any<BwdVarlenSoftcapArgs, 5, false>(a, s);
}

}  // namespace fa
