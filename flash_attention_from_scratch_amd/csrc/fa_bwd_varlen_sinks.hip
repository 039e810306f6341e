// fa_bwd_varlen_sinks.hip -- the translation unit of the backward over packed sequences with learned attention sinks
// (fa_bwd_launch_varlen_qk_sinks; fa_bwd_varlen.hpp says why dQ, dK, dV are the window form's kernels unchanged).  It builds none of
// the header's kernels: one backward here is the window unit's enqueue (fa_bwd_varlen_window.hip: delta -> dK / dV (+ reduce) ->
// dQ, left = right = 2^30 where there is no window) and, behind it on the same stream, the one kernel this unit holds, the
// sinks' own gradient.  Shapes, pointers, the window and the sinks are validated by the caller (fa_capi.hip).
#include <hip/hip_runtime.h>

#include "fa_bwd_varlen.hpp"

namespace fa {

hipError_t bwd_varlen_window_enqueue(const BwdVarlenWindowArgs &a, int dtype, hipStream_t s);   // fa_bwd_varlen_window.hip

// dsinks[h] = - sum over the rows of head h of exp(sinks[h] - lse[h][row]) delta[h][row]: the sink's softmax weight times
// (dP - delta) with dP = dO . 0 = 0.  lse is the forward's (it includes the sink, so the weight is <= 1 and the exponent <= 0),
// delta the (n_heads, total_q) fp32 the delta kernel left in the workspace.
// The rows: all total_q of them, without a sequence lookup, like the delta kernel -- under the cu_seqlens contract ([0] = 0,
// [n_seqs] = total_q, non-decreasing) every row belongs to a sequence.
// One workgroup of 1024 threads per head.  Thread t adds rows t, t + 1024, ... in that order, the 64 lanes of a wave are summed
// by a butterfly, the 16 waves' sums in wave order by one thread: fp32, a fixed order, no atomics, no partials in memory -- the
// same inputs give the same bits from any launch history.  A row with lse = -inf (dead, without a sink) and a head with
// z = -inf contribute exactly 0 by a select: exp(-inf - -inf) is never formed.
constexpr int DSINKS_THREADS = 1024;
__global__ void __launch_bounds__(DSINKS_THREADS) fa_bwd_dsinks_varlen_kernel(const BwdVarlenSinksArgs a) {
    __shared__ float wave_sum[DSINKS_THREADS / 64];
    const int hq = blockIdx.x, tid = threadIdx.x;
    const float z = a.sinks[hq];
    const float *lse = a.w.lse + (int64_t)hq * a.w.total_tokens;
    const float *delta = a.w.delta + (int64_t)hq * a.w.total_tokens;
    const float ninf = -__builtin_inff();
    float acc = 0.0f;
    for (int row = tid; row < a.w.total_tokens; row += DSINKS_THREADS) {
        const float l = lse[row];
        const float w = __builtin_amdgcn_exp2f((z - l) * 1.4426950408889634074f);
        acc += (z == ninf || l == ninf) ? 0.0f : w * delta[row];
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) acc += __shfl_xor(acc, m, 64);
    if ((tid & 63) == 0) wave_sum[tid >> 6] = acc;
    __syncthreads();
    if (tid == 0) {
        float sum = 0.0f;
        for (int w = 0; w < DSINKS_THREADS / 64; ++w) sum += wave_sum[w];
        a.dsinks[hq] = z == ninf ? 0.0f : 0.0f - sum;
    }
}

hipError_t bwd_varlen_sinks_enqueue(const BwdVarlenSinksArgs &a, int dtype, hipStream_t s) {
    const hipError_t rc = bwd_varlen_window_enqueue(a.w, dtype, s);
    if (rc != hipSuccess) return rc;
    void *params[] = {(void *)&a};
    return hipLaunchKernel((const void *)&fa_bwd_dsinks_varlen_kernel, dim3((unsigned)a.w.n_heads), dim3(DSINKS_THREADS), params, 0, s);
}

}  // namespace fa
