// fa_prefill64_fp8.hip -- the prefill at d_head = 64 against an fp8 (e4m3fn) cache: fa_prefill64_kernel.hpp's FP8 form
// for both dtypes -- two kernels, contiguous or paged by a null test of block_table at run time -- and the enqueue of one launch.  Shapes,
// pointers, strides (bytes), descales, the window and the sinks are validated by the caller (fwd_launch_varlen, fa_capi.hip).  A unit
// of its own: the 16-bit kernels of fa_prefill64.hip keep theirs.
#include <hip/hip_runtime.h>

#include "fa_prefill64_kernel.hpp"

namespace fa {

template __global__ void fa_prefill64_kernel<15, true, true>(const Prefill64Args);
template __global__ void fa_prefill64_kernel<5, true, true>(const Prefill64Args);

// the 16-bit launch's grid: one workgroup per (sequence, head, 256-row block of max_seqlen_q)
hipError_t prefill64_fp8_enqueue(const Prefill64Args &args, int dtype, int64_t n_seqs, hipStream_t s) {
    const void *fn = dtype == 15 ? (const void *)&fa_prefill64_kernel<15, true, true> : (const void *)&fa_prefill64_kernel<5, true, true>;
    void *params[] = {(void *)&args};
    return hipLaunchKernel(fn, dim3((unsigned)(n_seqs * args.n_heads * args.n_q_blocks)), dim3(prefill64::THREADS), params, 0, s);
}

}  // namespace fa
