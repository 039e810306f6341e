// fa_bwd_varlen64.hip -- the translation unit of the packed backward at d_head = 64 (fa_bwd_launch_varlen_qk_d64):
// fa_bwd64_kernel.hpp's kernels for both dtypes, the sinks' own gradient, and the enqueue of one backward.  Shapes, pointers, the
// window and the sinks are validated by the caller (fa_capi.hip).  A unit of its own: the d128 units keep their kernels.
#include <hip/hip_runtime.h>

#include "fa_bwd64_kernel.hpp"

namespace fa {

// dsinks[h] = - sum over the rows of head h of exp(sinks[h] - lse[h][row]) delta[h][row] (the sink's softmax weight times
// (dP - delta) with dP = dO . 0 = 0), over all total_q rows like the delta kernel: fa_bwd_dsinks_varlen_kernel's sum on this
// unit's arguments.  One workgroup of 1024 threads per head: thread t adds rows t, t + 1024, ... in that order, a wave's 64 lanes
// by a butterfly, the 16 waves' sums in wave order by one thread -- fp32, a fixed order, no atomics.  A row with lse = -inf and a
// head with z = -inf add exactly 0 by a select: exp(-inf - -inf) is never formed.
constexpr int BWD64_DSINKS_THREADS = 1024;
__global__ void __launch_bounds__(BWD64_DSINKS_THREADS) fa_bwd64_dsinks_kernel(const Bwd64Args a) {
    __shared__ float wave_sum[BWD64_DSINKS_THREADS / 64];
    const int hq = blockIdx.x, tid = threadIdx.x;
    const float z = a.sinks[hq];
    const float *lse = a.lse + (int64_t)hq * a.total_q;
    const float *delta = a.delta + (int64_t)hq * a.total_q;
    const float ninf = -__builtin_inff();
    float acc = 0.0f;
    for (int row = tid; row < a.total_q; row += BWD64_DSINKS_THREADS) {
        const float l = lse[row];
        const float w = __builtin_amdgcn_exp2f((z - l) * bwd64::LOG2E);
        acc += (z == ninf || l == ninf) ? 0.0f : w * delta[row];
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) acc += __shfl_xor(acc, m, 64);
    if ((tid & 63) == 0) wave_sum[tid >> 6] = acc;
    __syncthreads();
    if (tid == 0) {
        float sum = 0.0f;
        for (int w = 0; w < BWD64_DSINKS_THREADS / 64; ++w) sum += wave_sum[w];
        a.dsinks[hq] = z == ninf ? 0.0f : 0.0f - sum;
    }
}

template <int DT>
static hipError_t bwd64_enqueue_dt(const Bwd64Args &a, hipStream_t s) {
    void *params[] = {(void *)&a};
    const int64_t n_kv = a.n_heads / a.group;
    const dim3 block(bwd64::THREADS);
    hipError_t rc = hipSuccess;
    if (a.total_q > 0) {   // (no query rows: only the zeros of dK / dV, and of dsinks, are left to write)
        const int64_t rows = (int64_t)a.n_heads * a.total_q;
        rc = hipLaunchKernel((const void *)&fa_bwd64_delta_kernel<DT>, dim3((unsigned)((rows + 31) / 32)), dim3(256), params, 0, s);
        if (rc != hipSuccess) return rc;
    }
    if (a.total_k > 0) {   // (no key rows: nothing to write, and the dQ kernel stores zeros)
        rc = hipLaunchKernel((const void *)&fa_bwd64_dkdv_kernel<DT>, dim3((unsigned)((int64_t)a.n_seqs * n_kv * a.split * a.n_blocks_k)), block,
                             params, 0, s);
        if (rc != hipSuccess) return rc;
        if (a.split > 1) {
            const int64_t n = n_kv * a.total_k * 2 * (bwd64::D / 8);
            rc = hipLaunchKernel((const void *)&fa_bwd64_reduce_kernel<DT>, dim3((unsigned)((n + 255) / 256)), dim3(256), params, 0, s);
            if (rc != hipSuccess) return rc;
        }
    }
    if (a.total_q > 0) {
        rc = hipLaunchKernel((const void *)&fa_bwd64_dq_kernel<DT>, dim3((unsigned)((int64_t)a.n_seqs * a.n_heads * a.n_blocks_q)), block, params,
                             0, s);
        if (rc != hipSuccess) return rc;
    }
    if (!a.sinks) return hipSuccess;
    return hipLaunchKernel((const void *)&fa_bwd64_dsinks_kernel, dim3((unsigned)a.n_heads), dim3(BWD64_DSINKS_THREADS), params, 0, s);
}

hipError_t bwd64_enqueue(const Bwd64Args &a, int dtype, hipStream_t s) {
    return dtype == 15 ? bwd64_enqueue_dt<15>(a, s) : bwd64_enqueue_dt<5>(a, s);
}

}  // namespace fa
