// fa_bwd_varlen.hip -- the varlen backward's translation unit: the kernels of fa_bwd_varlen.hpp in their one-range form
// (BwdVarlenArgs) for both dtypes and both masks, and the enqueue of one backward over packed sequences (three or four launches
// on one stream).  Shapes and pointers are validated by the caller (fa_bwd_launch_varlen, fa_capi.hip).  The flags of
// fa_bwd.hip: same contraction, same bits.
#include <hip/hip_runtime.h>

#include "fa_bwd_varlen.hpp"

namespace fa {

// delta, dK / dV (one workgroup per sequence, K / V head, split part and key block of max_seqlen), their fixed-order sum
// when split > 1, dQ.  The grids depend on the host's arguments alone: cu_seqlens is never read here.
template <int DT, bool CAUSAL>
static hipError_t bwd_varlen_enqueue_t(const BwdVarlenArgs &a, hipStream_t s) {
    const int64_t rows = (int64_t)a.n_heads * a.total_tokens;
    void *params[] = {(void *)&a};
    hipError_t rc = hipLaunchKernel((const void *)&fa_bwd_delta_varlen_kernel<DT>, dim3((unsigned)((rows + 15) / 16)), dim3(256), params, 0, s);
    if (rc != hipSuccess) return rc;
    const int64_t n_kv = a.n_heads / a.group;
    const dim3 block(bwd::THREADS);
    rc = hipLaunchKernel((const void *)&fa_bwd_dkdv_varlen_kernel<BwdVarlenArgs, DT, CAUSAL>,
                         dim3((unsigned)((int64_t)a.n_seqs * n_kv * a.split * a.n_blocks)), block, params, 0, s);
    if (rc != hipSuccess) return rc;
    if (a.split > 1) {
        const int64_t n = n_kv * a.total_tokens * 2 * (bwd::D / 8);
        rc = hipLaunchKernel((const void *)&fa_bwd_dkdv_reduce_varlen_kernel<BwdVarlenArgs, DT>, dim3((unsigned)((n + 255) / 256)), dim3(256), params, 0, s);
        if (rc != hipSuccess) return rc;
    }
    return hipLaunchKernel((const void *)&fa_bwd_dq_varlen_kernel<BwdVarlenArgs, DT, CAUSAL>, dim3((unsigned)((int64_t)a.n_seqs * a.n_heads * a.n_blocks)),
                           block, params, 0, s);
}

// the delta launch alone (fa_bwd_varlen_qk.hip: the same kernel over the query rows of a launch with separate K / V lengths)
hipError_t bwd_varlen_delta_enqueue(const BwdVarlenArgs &a, int dtype, hipStream_t s) {
    const int64_t rows = (int64_t)a.n_heads * a.total_tokens;
    void *params[] = {(void *)&a};
    const void *fn = dtype == 15 ? (const void *)&fa_bwd_delta_varlen_kernel<15> : (const void *)&fa_bwd_delta_varlen_kernel<5>;
    return hipLaunchKernel(fn, dim3((unsigned)((rows + 15) / 16)), dim3(256), params, 0, s);
}

hipError_t bwd_varlen_enqueue(const BwdVarlenArgs &a, int dtype, bool causal, hipStream_t s) {
    if (dtype == 15) return causal ? bwd_varlen_enqueue_t<15, true>(a, s) : bwd_varlen_enqueue_t<15, false>(a, s);
    return causal ? bwd_varlen_enqueue_t<5, true>(a, s) : bwd_varlen_enqueue_t<5, false>(a, s);
}

}  // namespace fa
