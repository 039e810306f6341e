// fa_decode_fp8_softcap.hip -- the soft-capped decode against an fp8 cache: the split kernel of fa_decode_kernel.hpp in its capped
// windowed fp8 form (DecodeFp8SoftcapArgs) for both Q dtypes, the three row-tile counts and both cache addressings, the combine
// kernel, and the enqueue of one decode.  Validated by the caller (fa_decode_fp8_softcap_launch, fa_capi.hip).  A unit of its own
// so that the other decode units' kernels stay as they are.
#include <hip/hip_runtime.h>

#include "fa_decode_kernel.hpp"

namespace fa {

hipError_t decode_fp8_softcap_enqueue(const DecodeFp8SoftcapArgs &a, int dtype, hipStream_t s) { return decode_enqueue_any(a, dtype, s); }

}  // namespace fa
