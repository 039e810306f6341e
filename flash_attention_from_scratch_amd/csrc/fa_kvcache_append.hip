// fa_kvcache_append.hip -- the KV-cache append's translation unit: the kernel of fa_kvcache_append_kernel.hpp for both 16-bit
// dtypes and both cache types (16-bit, fp8 e4m3fn), and its enqueue (one launch, one workgroup per batch entry).  Shapes and
// pointers are validated by the caller (fa_kvcache_append_launch, fa_capi.hip).  Outside the registry.
#include <hip/hip_runtime.h>

#include "fa_kvcache_append_kernel.hpp"

namespace fa {

template <int DT, bool FP8>
static hipError_t kvcache_append_enqueue_t(const AppendArgs &a, int batch, hipStream_t s) {
    void *params[] = {(void *)&a};
    return hipLaunchKernel((const void *)&fa_kvcache_append_kernel<DT, FP8>, dim3((unsigned)batch), dim3(append::THREADS), params, 0, s);
}

hipError_t kvcache_append_enqueue(const AppendArgs &a, int batch, int dtype, bool fp8, hipStream_t s) {
    if (dtype == 15) return fp8 ? kvcache_append_enqueue_t<15, true>(a, batch, s) : kvcache_append_enqueue_t<15, false>(a, batch, s);
    return fp8 ? kvcache_append_enqueue_t<5, true>(a, batch, s) : kvcache_append_enqueue_t<5, false>(a, batch, s);
}

}  // namespace fa
