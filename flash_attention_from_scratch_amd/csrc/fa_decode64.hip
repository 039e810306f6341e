// fa_decode64.hip -- the decode path at d_head = 64: the split kernel of fa_decode64_kernel.hpp for both dtypes, the three row-tile
// counts and both cache addressings (twelve kernels) at the shipped unit, the same twelve at the other unit it was measured against
// (FA_DECODE64_UNIT=32 or =64 in the environment names a unit outright: tools/decode64_bench.py's arms and one test),
// its combine kernel, and the enqueue of one decode.  Shapes, pointers, the
// window and the sinks are validated by the caller (fa_decode_d64_launch, fa_capi.hip).  A unit of its own: the d128 units' kernels
// stay as they are.
#include <hip/hip_runtime.h>

#include <cstdlib>
#include <cstring>

#include "fa_decode64_kernel.hpp"

namespace fa {

// the split kernel and, for num_splits > 1, the combine kernel on stream s
template <int DT, int NT, bool PAGED, int UNIT>
static hipError_t decode64_enqueue_t(const Decode64Args &args, hipStream_t s) {
    const DecodeArgs &a = args.d;
    void *params[] = {(void *)&args};
    const hipError_t rc = hipLaunchKernel((const void *)&fa_decode64_split_kernel<DT, NT, PAGED, UNIT>,
                                          dim3((unsigned)((int64_t)a.batch * a.n_kv_heads * a.num_splits)), dim3(decode64::THREADS), params, 0, s);
    if (rc != hipSuccess || a.num_splits == 1) return rc;
    return hipLaunchKernel((const void *)&fa_decode64_combine_kernel<DT>, dim3((unsigned)((int64_t)a.batch * a.n_kv_heads * a.rows)), dim3(64),
                           params, 0, s);
}

hipError_t decode64_enqueue(const Decode64Args &args, int dtype, hipStream_t s) {
    const bool paged = args.d.block_table != nullptr, bf16 = dtype == 15;
    const char *env = std::getenv("FA_DECODE64_UNIT");   // (read per launch: a test sets it for one call)
    const int unit = env && std::strcmp(env, "32") == 0 ? 32 : env && std::strcmp(env, "64") == 0 ? 64 : decode64::UNIT_SHIPPED;
    auto go = [&](auto nt, auto unit) {
        constexpr int NT = decltype(nt)::value, UNIT = decltype(unit)::value;
        if (bf16) return paged ? decode64_enqueue_t<15, NT, true, UNIT>(args, s) : decode64_enqueue_t<15, NT, false, UNIT>(args, s);
        return paged ? decode64_enqueue_t<5, NT, true, UNIT>(args, s) : decode64_enqueue_t<5, NT, false, UNIT>(args, s);
    };
    auto rows = [&](auto unit) {
        switch (decode::row_tiles(args.d.rows)) {
        case 1: return go(IntTag<1>{}, unit);
        case 2: return go(IntTag<2>{}, unit);
        default: return go(IntTag<4>{}, unit);
        }
    };
    return unit == 32 ? rows(IntTag<32>{}) : rows(IntTag<64>{});
}

}  // namespace fa
