// fa_decode_softcap.hip -- the soft-capped decode path's translation unit: the split kernel of fa_decode_kernel.hpp in its capped
// windowed 16-bit form (DecodeSoftcapArgs) for both dtypes, the three row-tile counts and both cache addressings, the decode path's
// combine kernel (the partial format is the same), and the enqueue of one decode.  Shapes, pointers, the window and the cap are
// validated by the caller (fa_decode_softcap_launch, fa_capi.hip).  A unit of its own so that the other decode units' kernels stay
// as they are.
#include <hip/hip_runtime.h>

#include "fa_decode_kernel.hpp"

namespace fa {

hipError_t decode_softcap_enqueue(const DecodeSoftcapArgs &a, int dtype, hipStream_t s) { return decode_enqueue_any(a, dtype, s); }

}  // namespace fa
