// fa_prefill256.hip -- the prefill path at d_head = 256: the kernel of fa_prefill256_kernel.hpp for both dtypes,
// both key sides (packed keys; a 16-bit cache, contiguous or paged by a null test of block_table at run time), with and without the
// cap and at both tile forms (sixteen kernels; FA_PREFILL256_TILE=64 or =32 in the environment names a form outright:
// tools/prefill256_bench.py's arms and the tests), the enqueue of one launch and the per-device opt-in to their dynamic LDS.  Shapes,
// pointers, the window and the cap are validated by the caller (fwd_launch_varlen, fa_capi.hip).  A unit of its own: the d128 varlen
// slices and the d64 unit keep their kernels.
#include <hip/hip_runtime.h>

#include <cstdlib>
#include <cstring>

#include "fa_prefill256_kernel.hpp"

namespace fa {

template <int DT, int TILE> static const void *prefill256_kernel(bool cache, bool capped) {
    if (cache) return capped ? (const void *)&fa_prefill256_kernel<DT, true, true, TILE> : (const void *)&fa_prefill256_kernel<DT, true, false, TILE>;
    return capped ? (const void *)&fa_prefill256_kernel<DT, false, true, TILE> : (const void *)&fa_prefill256_kernel<DT, false, false, TILE>;
}
static const void *prefill256_kernel(int dtype, bool cache, bool capped, int tile) {
    if (tile == 64) return dtype == 15 ? prefill256_kernel<15, 64>(cache, capped) : prefill256_kernel<5, 64>(cache, capped);
    return dtype == 15 ? prefill256_kernel<15, 32>(cache, capped) : prefill256_kernel<5, 32>(cache, capped);
}

// more than 64 KiB of LDS is dynamic LDS a function has to be opted in to, once per device (with that device current)
hipError_t prefill256_device_init() {
    for (int i = 0; i < 16; ++i) {
        const int tile = (i & 8) ? 32 : 64;
        const hipError_t rc = hipFuncSetAttribute(prefill256_kernel((i & 4) ? 5 : 15, (i & 2) != 0, (i & 1) != 0, tile),
                                                  hipFuncAttributeMaxDynamicSharedMemorySize, prefill256::lds_bytes(tile));
        if (rc != hipSuccess) return rc;
    }
    return hipSuccess;
}

// one workgroup per (sequence, 128-row block of max_seqlen_q, head): host-visible numbers only
hipError_t prefill256_enqueue(const Prefill256Args &args, int dtype, bool cache, bool capped, int64_t n_seqs, hipStream_t s) {
    const char *env = std::getenv("FA_PREFILL256_TILE");   // (read per launch: a test sets it for one call)
    const int tile = env && std::strcmp(env, "64") == 0 ? 64 : env && std::strcmp(env, "32") == 0 ? 32 : prefill256::TILE_SHIPPED;
    void *params[] = {(void *)&args};
    return hipLaunchKernel(prefill256_kernel(dtype, cache, capped, tile), dim3((unsigned)(n_seqs * args.n_q_blocks * args.n_heads)),
                           dim3(prefill256::THREADS), params, (size_t)prefill256::lds_bytes(tile), s);
}

}  // namespace fa
