// fa_decode.hip -- the decode path's translation unit: the split kernel of fa_decode_kernel.hpp in its 16-bit form (DecodeArgs)
// for both dtypes, the three row-tile counts and both cache addressings, the combine kernel, and the enqueue of one decode (one
// or two launches on one stream).  Shapes and pointers are validated by the caller (fa_decode_launch, fa_capi.hip).  Outside
// the registry.
#include <hip/hip_runtime.h>

#include "fa_decode_kernel.hpp"

namespace fa {

hipError_t decode_enqueue(const DecodeArgs &a, int dtype, hipStream_t s) { return decode_enqueue_any(a, dtype, s); }

}  // namespace fa
