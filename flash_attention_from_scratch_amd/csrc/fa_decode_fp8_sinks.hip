// fa_decode_fp8_sinks.hip -- the decode against an fp8 cache with attention sinks: the split kernel of fa_decode_kernel.hpp in its
// windowed fp8 form with sinks (DecodeFp8SinksArgs) for both Q dtypes, the three row-tile counts and both cache addressings, the
// combine kernel that adds the sink, and the enqueue of one decode.  Validated by the caller (fa_decode_fp8_sinks_launch,
// fa_capi.hip).  A unit of its own so that the other decode units' kernels stay as they are.
#include <hip/hip_runtime.h>

#include "fa_decode_kernel.hpp"

namespace fa {

hipError_t decode_fp8_sinks_enqueue(const DecodeFp8SinksArgs &a, int dtype, hipStream_t s) { return decode_enqueue_any(a, dtype, s); }

}  // namespace fa
