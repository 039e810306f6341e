// fa_decode_sinks.hip -- the decode path with attention sinks: the split kernel of fa_decode_kernel.hpp in its windowed 16-bit form
// with sinks (DecodeSinksArgs) for both dtypes, the three row-tile counts and both cache addressings, the combine kernel that adds
// the sink (the partials are sink-free), and the enqueue of one decode.  Shapes, pointers, the window and the sinks are validated by
// the caller (fa_decode_sinks_launch, fa_capi.hip).  A unit of its own so that the other decode units' kernels stay as they are.
#include <hip/hip_runtime.h>

#include "fa_decode_kernel.hpp"

namespace fa {

hipError_t decode_sinks_enqueue(const DecodeSinksArgs &a, int dtype, hipStream_t s) { return decode_enqueue_any(a, dtype, s); }

}  // namespace fa
