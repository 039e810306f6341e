// fa_decode_window.hip -- the sliding-window decode path's translation unit: the split kernel of fa_decode_kernel.hpp in its
// windowed 16-bit form (DecodeWindowArgs) for both dtypes, the three row-tile counts and both cache addressings, the decode path's
// combine kernel (the partial format is the same), and the enqueue of one decode.  Shapes, pointers and the window are validated
// by the caller (fa_decode_window_launch, fa_capi.hip).  A unit of its own so that fa_decode.hip's kernels stay as they are.
#include <hip/hip_runtime.h>

#include "fa_decode_kernel.hpp"

namespace fa {

hipError_t decode_window_enqueue(const DecodeWindowArgs &a, int dtype, hipStream_t s) { return decode_enqueue_any(a, dtype, s); }

}  // namespace fa
