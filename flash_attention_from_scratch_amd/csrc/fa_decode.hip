// fa_decode.hip -- the decode path's translation unit: the split kernel of fa_decode_kernel.hpp for both dtypes, the three row-tile
// counts and both cache addressings, the combine kernel, and the enqueue of one decode (one or two launches on one stream).
// Shapes and pointers are validated by the caller (fa_decode_launch, fa_capi.hip).  Outside the registry.
#include <hip/hip_runtime.h>

#include "fa_decode_kernel.hpp"

namespace fa {

template <int DT, int NT, bool PAGED>
static hipError_t decode_enqueue_t(const DecodeArgs &a, hipStream_t s) {
    void *params[] = {(void *)&a};
    const hipError_t rc = hipLaunchKernel((const void *)&fa_decode_split_kernel<DT, NT, PAGED>,
                                          dim3((unsigned)((int64_t)a.batch * a.n_kv_heads * a.num_splits)), dim3(decode::THREADS), params, 0, s);
    if (rc != hipSuccess || a.num_splits == 1) return rc;
    return hipLaunchKernel((const void *)&fa_decode_combine_kernel<DT>, dim3((unsigned)((int64_t)a.batch * a.n_kv_heads * a.rows)), dim3(64),
                           params, 0, s);
}

template <int DT>
static hipError_t decode_enqueue_dt(const DecodeArgs &a, hipStream_t s) {
    const bool paged = a.block_table != nullptr;
    switch (decode::row_tiles(a.rows)) {
    case 1: return paged ? decode_enqueue_t<DT, 1, true>(a, s) : decode_enqueue_t<DT, 1, false>(a, s);
    case 2: return paged ? decode_enqueue_t<DT, 2, true>(a, s) : decode_enqueue_t<DT, 2, false>(a, s);
    default: return paged ? decode_enqueue_t<DT, 4, true>(a, s) : decode_enqueue_t<DT, 4, false>(a, s);
    }
}

hipError_t decode_enqueue(const DecodeArgs &a, int dtype, hipStream_t s) {
    return dtype == 15 ? decode_enqueue_dt<15>(a, s) : decode_enqueue_dt<5>(a, s);
}

}  // namespace fa
