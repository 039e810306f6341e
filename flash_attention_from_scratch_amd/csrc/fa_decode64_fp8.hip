// fa_decode64_fp8.hip -- the decode path at d_head = 64 against an fp8 (e4m3fn) cache: the split kernel of fa_decode64_kernel.hpp in
// its fp8 form (Decode64Fp8Args) for both Q dtypes, the three row-tile counts and both cache addressings (twelve kernels) at each of
// the three (unit, prefetch distance) forms it was measured in -- (32, 1), (32, 2) and (64, 1), the shipped one
// among them -- and the enqueue of one decode.  (64, 2) is not built: it would hold 128 keys in flight per wave where (32, 2) and
// (64, 1) hold 64, and at 64 rows its three register sets of 32 no longer fit beside Q^T, O^T and S^T without scratch.
// FA_DECODE64_UNIT=32 or =64 and, at the 32-key unit, FA_DECODE64_AHEAD=1 or =2 in the environment name a form outright
// (tools/decode64_bench.py's arms and one test).  The combine kernel is the 16-bit form's, on the same partials.  Shapes, pointers,
// the window, the sinks and the descales are validated by the caller (fa_decode_fp8_d64_launch, fa_capi.hip).  A unit of its own: the
// 16-bit unit's kernels stay as they are.
#include <hip/hip_runtime.h>

#include <cstdlib>
#include <cstring>

#include "fa_decode64_kernel.hpp"

namespace fa {

static_assert(decode64::FP8_UNIT_SHIPPED == 32 || decode64::FP8_DIST_SHIPPED == 1, "the 64-key unit runs one unit ahead");

// the split kernel and, for num_splits > 1, the combine kernel on stream s
template <int DT, int NT, bool PAGED, int UNIT, int DIST>
static hipError_t decode64_fp8_enqueue_t(const Decode64Fp8Args &args, hipStream_t s) {
    const DecodeArgs &a = args.w.d;
    void *params[] = {(void *)&args}, *cparams[] = {(void *)&args.w};
    const hipError_t rc = hipLaunchKernel((const void *)&fa_decode64_split_kernel<DT, NT, PAGED, UNIT, Decode64Fp8Args, DIST>,
                                          dim3((unsigned)((int64_t)a.batch * a.n_kv_heads * a.num_splits)), dim3(decode64::THREADS), params, 0, s);
    if (rc != hipSuccess || a.num_splits == 1) return rc;
    return hipLaunchKernel((const void *)&fa_decode64_combine_kernel<DT>, dim3((unsigned)((int64_t)a.batch * a.n_kv_heads * a.rows)), dim3(64),
                           cparams, 0, s);
}

hipError_t decode64_fp8_enqueue(const Decode64Fp8Args &args, int dtype, hipStream_t s) {
    const bool paged = args.w.d.block_table != nullptr, bf16 = dtype == 15;
    const char *env_u = std::getenv("FA_DECODE64_UNIT"), *env_d = std::getenv("FA_DECODE64_AHEAD");   // (read per launch: a test sets them for one call)
    const int unit = env_u && std::strcmp(env_u, "32") == 0 ? 32 : env_u && std::strcmp(env_u, "64") == 0 ? 64 : decode64::FP8_UNIT_SHIPPED;
    const int dist = unit == 64 ? 1 : env_d && std::strcmp(env_d, "1") == 0 ? 1 : env_d && std::strcmp(env_d, "2") == 0 ? 2 : decode64::FP8_DIST_SHIPPED;
    auto go = [&](auto nt, auto unit, auto dist) {
        constexpr int NT = decltype(nt)::value, UNIT = decltype(unit)::value, DIST = decltype(dist)::value;
        if (bf16) return paged ? decode64_fp8_enqueue_t<15, NT, true, UNIT, DIST>(args, s) : decode64_fp8_enqueue_t<15, NT, false, UNIT, DIST>(args, s);
        return paged ? decode64_fp8_enqueue_t<5, NT, true, UNIT, DIST>(args, s) : decode64_fp8_enqueue_t<5, NT, false, UNIT, DIST>(args, s);
    };
    auto rows = [&](auto unit, auto dist) {
        switch (decode::row_tiles(args.w.d.rows)) {
        case 1: return go(IntTag<1>{}, unit, dist);
        case 2: return go(IntTag<2>{}, unit, dist);
        default: return go(IntTag<4>{}, unit, dist);
        }
    };
    if (unit == 64) return rows(IntTag<64>{}, IntTag<1>{});
    return dist == 1 ? rows(IntTag<32>{}, IntTag<1>{}) : rows(IntTag<32>{}, IntTag<2>{});
}

}  // namespace fa
