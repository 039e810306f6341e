// fa_decode_fp8.hip -- the fp8-cache decode path's translation unit: the split kernel of fa_decode_fp8_kernel.hpp for both Q dtypes,
// the three row-tile counts and both cache addressings, the 16-bit path's combine kernel (the partial format is the same), and
// the enqueue of one decode (one or two launches on one stream).  Shapes and pointers are validated by the caller
// (fa_decode_fp8_launch, fa_capi.hip).  Outside the registry.
#include <hip/hip_runtime.h>

#include "fa_decode_fp8_kernel.hpp"

namespace fa {

template <int DT, int NT, bool PAGED>
static hipError_t decode_fp8_enqueue_t(const DecodeFp8Args &a, hipStream_t s) {
    void *params[] = {(void *)&a};
    const hipError_t rc = hipLaunchKernel((const void *)&fa_decode_fp8_split_kernel<DT, NT, PAGED>,
                                          dim3((unsigned)((int64_t)a.d.batch * a.d.n_kv_heads * a.d.num_splits)), dim3(decode::THREADS), params, 0, s);
    if (rc != hipSuccess || a.d.num_splits == 1) return rc;
    void *cparams[] = {(void *)&a.d};
    return hipLaunchKernel((const void *)&fa_decode_combine_kernel<DT>, dim3((unsigned)((int64_t)a.d.batch * a.d.n_kv_heads * a.d.rows)), dim3(64),
                           cparams, 0, s);
}

template <int DT>
static hipError_t decode_fp8_enqueue_dt(const DecodeFp8Args &a, hipStream_t s) {
    const bool paged = a.d.block_table != nullptr;
    switch (decode::row_tiles(a.d.rows)) {
    case 1: return paged ? decode_fp8_enqueue_t<DT, 1, true>(a, s) : decode_fp8_enqueue_t<DT, 1, false>(a, s);
    case 2: return paged ? decode_fp8_enqueue_t<DT, 2, true>(a, s) : decode_fp8_enqueue_t<DT, 2, false>(a, s);
    default: return paged ? decode_fp8_enqueue_t<DT, 4, true>(a, s) : decode_fp8_enqueue_t<DT, 4, false>(a, s);
    }
}

hipError_t decode_fp8_enqueue(const DecodeFp8Args &a, int dtype, hipStream_t s) {
    return dtype == 15 ? decode_fp8_enqueue_dt<15>(a, s) : decode_fp8_enqueue_dt<5>(a, s);
}

}  // namespace fa
