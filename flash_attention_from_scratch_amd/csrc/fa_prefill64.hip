// fa_prefill64.hip -- the prefill path at d_head = 64: the kernel of fa_prefill64_kernel.hpp for both dtypes and
// both key sides (packed keys; a 16-bit cache, contiguous or paged by a null test of block_table at run time) -- four kernels -- and
// the enqueue of one launch.  Shapes, pointers, the window and the sinks are validated by the caller (fwd_launch_varlen_d64,
// fa_capi.hip).  A unit of its own: the d128 varlen slices keep their kernels.
#include <hip/hip_runtime.h>

#include "fa_prefill64_kernel.hpp"

namespace fa {

template __global__ void fa_prefill64_kernel<15, false>(const Prefill64Args);
template __global__ void fa_prefill64_kernel<15, true>(const Prefill64Args);
template __global__ void fa_prefill64_kernel<5, false>(const Prefill64Args);
template __global__ void fa_prefill64_kernel<5, true>(const Prefill64Args);

// one workgroup per (sequence, head, 256-row block of max_seqlen_q): host-visible numbers only
hipError_t prefill64_enqueue(const Prefill64Args &args, int dtype, bool cache, int64_t n_seqs, hipStream_t s) {
    const void *fn = dtype == 15 ? (cache ? (const void *)&fa_prefill64_kernel<15, true> : (const void *)&fa_prefill64_kernel<15, false>)
                                 : (cache ? (const void *)&fa_prefill64_kernel<5, true> : (const void *)&fa_prefill64_kernel<5, false>);
    void *params[] = {(void *)&args};
    return hipLaunchKernel(fn, dim3((unsigned)(n_seqs * args.n_heads * args.n_q_blocks)), dim3(prefill64::THREADS), params, 0, s);
}

}  // namespace fa
