// fa_bwd.hip -- the backward's translation unit: the delta / dK dV / dQ kernels of fa_bwd_kernel.hpp for both dtypes and
// both masks, and the enqueue of one backward (three launches on one stream), also for grouped-query attention.  Shapes and pointers are validated by the
// caller (fa_bwd_launch, fa_capi.hip).
#include <hip/hip_runtime.h>

#include "fa_bwd_gqa.hpp"

namespace fa {

template <int DT, bool CAUSAL>
static hipError_t bwd_enqueue_t(const BwdArgs &a, hipStream_t s) {
    const int64_t rows = (int64_t)a.n_bh * a.seq_len;
    void *params[] = {(void *)&a};
    hipError_t rc = hipLaunchKernel((const void *)&fa_bwd_delta_kernel<DT>, dim3((unsigned)((rows + 15) / 16)), dim3(256), params, 0, s);
    if (rc != hipSuccess) return rc;
    const dim3 grid((unsigned)(a.n_bh * (a.seq_len / bwd::KB))), block(bwd::THREADS);
    rc = hipLaunchKernel((const void *)&fa_bwd_dkdv_kernel<DT, CAUSAL>, grid, block, params, 0, s);
    if (rc != hipSuccess) return rc;
    return hipLaunchKernel((const void *)&fa_bwd_dq_kernel<DT, CAUSAL>, grid, block, params, 0, s);
}

// grouped-query attention: delta, dK / dV (one workgroup per K / V head, split and key block), their fixed-order sum when
// split > 1, dQ -- three or four launches on one stream
template <int DT, bool CAUSAL>
static hipError_t bwd_gqa_enqueue_t(const BwdGqaArgs &g, hipStream_t s) {
    const BwdArgs &a = g.base;
    const int64_t rows = (int64_t)a.n_bh * a.seq_len;
    void *params_b[] = {(void *)&a};
    void *params[] = {(void *)&g};
    hipError_t rc = hipLaunchKernel((const void *)&fa_bwd_delta_kernel<DT>, dim3((unsigned)((rows + 15) / 16)), dim3(256), params_b, 0, s);
    if (rc != hipSuccess) return rc;
    const int64_t n_bkv = a.n_bh / g.group;
    const dim3 block(bwd::THREADS);
    rc = hipLaunchKernel((const void *)&fa_bwd_dkdv_gqa_kernel<DT, CAUSAL>, dim3((unsigned)(n_bkv * g.split * (a.seq_len / bwd::KB))), block,
                         params, 0, s);
    if (rc != hipSuccess) return rc;
    if (g.split > 1) {
        const int64_t n = n_bkv * a.seq_len * 2 * (bwd::D / 8);
        rc = hipLaunchKernel((const void *)&fa_bwd_dkdv_reduce_kernel<DT>, dim3((unsigned)((n + 255) / 256)), dim3(256), params, 0, s);
        if (rc != hipSuccess) return rc;
    }
    return hipLaunchKernel((const void *)&fa_bwd_dq_gqa_kernel<DT, CAUSAL>, dim3((unsigned)(a.n_bh * (a.seq_len / bwd::KB))), block, params, 0, s);
}

hipError_t bwd_gqa_enqueue(const BwdGqaArgs &g, int dtype, bool causal, hipStream_t s) {
    if (dtype == 15) return causal ? bwd_gqa_enqueue_t<15, true>(g, s) : bwd_gqa_enqueue_t<15, false>(g, s);
    return causal ? bwd_gqa_enqueue_t<5, true>(g, s) : bwd_gqa_enqueue_t<5, false>(g, s);
}

hipError_t bwd_enqueue(const BwdArgs &a, int dtype, bool causal, hipStream_t s) {
    if (dtype == 15) return causal ? bwd_enqueue_t<15, true>(a, s) : bwd_enqueue_t<15, false>(a, s);
    return causal ? bwd_enqueue_t<5, true>(a, s) : bwd_enqueue_t<5, false>(a, s);
}

}  // namespace fa
