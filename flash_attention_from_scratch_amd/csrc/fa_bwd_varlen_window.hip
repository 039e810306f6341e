// fa_bwd_varlen_window.hip -- the translation unit of the backward over packed sequences under a sliding window: the kernels
// of fa_bwd_varlen.hpp in their window form (BwdVarlenWindowArgs) for both dtypes, behind the header's enqueue of one backward
// (bwd_varlen_enqueue_any).  One instantiation per dtype: the window carries the causal mask as right = 0.  Shapes,
// pointers and the window are validated by the caller (fa_bwd_launch_varlen_qk_window, fa_capi.hip).  The flags of
// fa_bwd_varlen.hip: same contraction.  A unit of its own, so that the one- and two-range slices keep their kernels.
#include <hip/hip_runtime.h>

#include "fa_bwd_varlen.hpp"

namespace fa {

hipError_t bwd_varlen_window_enqueue(const BwdVarlenWindowArgs &a, int dtype, hipStream_t s) {
    return dtype == 15 ? bwd_varlen_enqueue_any<BwdVarlenWindowArgs, 15, false>(a, s) : bwd_varlen_enqueue_any<BwdVarlenWindowArgs, 5, false>(a, s);
}

}  // namespace fa
