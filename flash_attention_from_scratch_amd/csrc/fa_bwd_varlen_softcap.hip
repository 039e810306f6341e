// fa_bwd_varlen_softcap.hip -- the translation unit of the backward over packed sequences with logit soft-capping: the kernels
// of fa_bwd_varlen.hpp in their soft-capped form (BwdVarlenSoftcapArgs: the window form plus the cap) for both dtypes, and the
// enqueue of one backward (three or four launches on one stream).  One instantiation per dtype: the window carries the causal
// mask as right = 0, and no window at all as left = right = 2^30.  Shapes, pointers, the window and the cap are validated by the
// caller (fa_bwd_launch_varlen_qk_softcap, fa_capi.hip).  The flags of fa_bwd_varlen.hip: same contraction.  A unit of its own, so
// that the other three slices keep their kernels.
#include <hip/hip_runtime.h>

#include "fa_bwd_varlen.hpp"

namespace fa {

// fa_bwd_varlen.hip: fa_bwd_delta_varlen_kernel as that unit builds it, over the (n_heads, total_tokens) rows of o and dout
// (delta = sum_d dO O does not know of the cap)
hipError_t bwd_varlen_delta_enqueue(const BwdVarlenArgs &a, int dtype, hipStream_t s);

// fa_bwd_varlen_window.hip's sequence of launches and grids (host arguments alone)
template <int DT>
static hipError_t bwd_varlen_softcap_enqueue_t(const BwdVarlenSoftcapArgs &a, hipStream_t s) {
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
        rc = hipLaunchKernel((const void *)&fa_bwd_dkdv_varlen_kernel<BwdVarlenSoftcapArgs, DT, false>,
                             dim3((unsigned)((int64_t)a.n_seqs * n_kv * a.split * a.n_blocks_k)), block, params, 0, s);
        if (rc != hipSuccess) return rc;
        if (a.split > 1) {
            const int64_t n = n_kv * a.total_k * 2 * (bwd::D / 8);
            rc = hipLaunchKernel((const void *)&fa_bwd_dkdv_reduce_varlen_kernel<BwdVarlenSoftcapArgs, DT>, dim3((unsigned)((n + 255) / 256)), dim3(256), params, 0, s);
            if (rc != hipSuccess) return rc;
        }
    }
    if (a.total_tokens == 0) return hipSuccess;
    return hipLaunchKernel((const void *)&fa_bwd_dq_varlen_kernel<BwdVarlenSoftcapArgs, DT, false>, dim3((unsigned)((int64_t)a.n_seqs * a.n_heads * a.n_blocks)),
                           block, params, 0, s);
}

hipError_t bwd_varlen_softcap_enqueue(const BwdVarlenSoftcapArgs &a, int dtype, hipStream_t s) {
    return dtype == 15 ? bwd_varlen_softcap_enqueue_t<15>(a, s) : bwd_varlen_softcap_enqueue_t<5>(a, s);
}

}  // namespace fa
