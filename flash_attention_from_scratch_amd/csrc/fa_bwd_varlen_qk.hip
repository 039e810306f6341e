// fa_bwd_varlen_qk.hip -- the translation unit of the backward over packed sequences with separate Q and K / V lengths: the
// kernels of fa_bwd_varlen.hpp in their two-range form (BwdVarlenQKArgs) for both dtypes and both masks, and the enqueue of one
// backward (three or four launches on one stream).  Shapes and pointers are validated by the caller (fa_bwd_launch_varlen_qk,
// fa_capi.hip).  The flags of fa_bwd_varlen.hip: same contraction, same bits.
#include <hip/hip_runtime.h>

#include "fa_bwd_varlen.hpp"

namespace fa {

// fa_bwd_varlen.hip: fa_bwd_delta_varlen_kernel as that unit builds it, over the (n_heads, total_tokens) rows of o and dout
hipError_t bwd_varlen_delta_enqueue(const BwdVarlenArgs &a, int dtype, hipStream_t s);

// delta over total_q, dK / dV (one workgroup per sequence, K / V head, split part and key block of max_seqlen_k), their
// fixed-order sum over total_k when split > 1, dQ (per Q block of max_seqlen_q).  The grids depend on the host's arguments
// alone: neither cu_seqlens is read here.
template <int DT, bool CAUSAL>
static hipError_t bwd_varlen_qk_enqueue_t(const BwdVarlenQKArgs &a, hipStream_t s) {
    BwdVarlenArgs d = {};   // what the delta kernel reads
    d.o = a.o;
    d.dout = a.dout;
    d.delta = a.delta;
    d.out_ss = a.out_ss;
    d.out_hs = a.out_hs;
    d.n_heads = a.n_heads;
    d.total_tokens = a.total_tokens;
    hipError_t rc = hipSuccess;
    if (a.total_tokens > 0) {   // (no query rows: only the zeros of dK / dV are left to write)
        rc = bwd_varlen_delta_enqueue(d, DT, s);
        if (rc != hipSuccess) return rc;
    }
    void *params[] = {(void *)&a};
    const int64_t n_kv = a.n_heads / a.group;
    const dim3 block(bwd::THREADS);
    if (a.total_k > 0) {   // (no key rows: nothing to write, and the dQ kernel stores zeros)
        rc = hipLaunchKernel((const void *)&fa_bwd_dkdv_varlen_kernel<BwdVarlenQKArgs, DT, CAUSAL>,
                             dim3((unsigned)((int64_t)a.n_seqs * n_kv * a.split * a.n_blocks_k)), block, params, 0, s);
        if (rc != hipSuccess) return rc;
        if (a.split > 1) {
            const int64_t n = n_kv * a.total_k * 2 * (bwd::D / 8);
            rc = hipLaunchKernel((const void *)&fa_bwd_dkdv_reduce_varlen_kernel<BwdVarlenQKArgs, DT>, dim3((unsigned)((n + 255) / 256)), dim3(256), params, 0, s);
            if (rc != hipSuccess) return rc;
        }
    }
    if (a.total_tokens == 0) return hipSuccess;
    return hipLaunchKernel((const void *)&fa_bwd_dq_varlen_kernel<BwdVarlenQKArgs, DT, CAUSAL>, dim3((unsigned)((int64_t)a.n_seqs * a.n_heads * a.n_blocks)),
                           block, params, 0, s);
}

hipError_t bwd_varlen_qk_enqueue(const BwdVarlenQKArgs &a, int dtype, bool causal, hipStream_t s) {
    if (dtype == 15) return causal ? bwd_varlen_qk_enqueue_t<15, true>(a, s) : bwd_varlen_qk_enqueue_t<15, false>(a, s);
    return causal ? bwd_varlen_qk_enqueue_t<5, true>(a, s) : bwd_varlen_qk_enqueue_t<5, false>(a, s);
}

}  // namespace fa
