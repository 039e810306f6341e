// fa_decode_fp8.hip -- the fp8-cache decode path's translation unit: the split kernel of fa_decode_kernel.hpp in its fp8 form
// (DecodeFp8Args) for both Q dtypes, the three row-tile counts and both cache addressings, the 16-bit path's combine kernel (the
// partial format is the same), and the enqueue of one decode (one or two launches on one stream).  Shapes and pointers are
// validated by the caller (fa_decode_fp8_launch, fa_capi.hip).  Outside the registry.
#include <hip/hip_runtime.h>

#include "fa_decode_kernel.hpp"

namespace fa {

hipError_t decode_fp8_enqueue(const DecodeFp8Args &a, int dtype, hipStream_t s) { return decode_enqueue_any(a, dtype, s); }

}  // namespace fa
