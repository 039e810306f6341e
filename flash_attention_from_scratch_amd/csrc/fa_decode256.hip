// fa_decode256.hip -- the decode path at d_head = 256: the split kernel of fa_decode256_kernel.hpp for both dtypes, both row-tile
// counts, both cache addressings and with and without the cap (sixteen kernels) at the 16-key unit, the eight one-row-tile kernels at
// the 32-key unit it was measured against (FA_DECODE256_UNIT=16 or =32 in the environment names a unit outright:
// tools/decode256_bench.py's arms and one test), its combine kernel, and the enqueue of one decode.  Shapes, pointers, the window and
// the cap are validated by the caller (fa_decode_d256_launch, fa_capi.hip).  A unit of its own: the d128 and d64 units' kernels stay
// as they are.
#include <hip/hip_runtime.h>

#include <cstdlib>
#include <cstring>

#include "fa_decode256_kernel.hpp"

namespace fa {

// the split kernel and, for num_splits > 1, the combine kernel on stream s
template <int DT, int NT, bool PAGED, int UNIT, bool CAP>
static hipError_t decode256_enqueue_t(const Decode256Args &args, hipStream_t s) {
    const DecodeArgs &a = args.d;
    void *params[] = {(void *)&args};
    const hipError_t rc = hipLaunchKernel((const void *)&fa_decode256_split_kernel<DT, NT, PAGED, UNIT, CAP>,
                                          dim3((unsigned)((int64_t)a.batch * a.n_kv_heads * a.num_splits)), dim3(decode256::THREADS), params, 0, s);
    if (rc != hipSuccess || a.num_splits == 1) return rc;
    return hipLaunchKernel((const void *)&fa_decode256_combine_kernel<DT>, dim3((unsigned)((int64_t)a.batch * a.n_kv_heads * a.rows)), dim3(64),
                           params, 0, s);
}

hipError_t decode256_enqueue(const Decode256Args &args, int dtype, bool capped, hipStream_t s) {
    const bool paged = args.d.block_table != nullptr, bf16 = dtype == 15;
    const char *env = std::getenv("FA_DECODE256_UNIT");   // (read per launch: a test sets it for one call)
    const int unit = env && std::strcmp(env, "16") == 0 ? 16 : env && std::strcmp(env, "32") == 0 ? 32 : decode256::UNIT_SHIPPED;
    auto go = [&](auto nt, auto unit, auto cap) {
        constexpr int NT = decltype(nt)::value, UNIT = decltype(unit)::value;
        constexpr bool CAP = decltype(cap)::value;
        if (bf16) return paged ? decode256_enqueue_t<15, NT, true, UNIT, CAP>(args, s) : decode256_enqueue_t<15, NT, false, UNIT, CAP>(args, s);
        return paged ? decode256_enqueue_t<5, NT, true, UNIT, CAP>(args, s) : decode256_enqueue_t<5, NT, false, UNIT, CAP>(args, s);
    };
    // (17 .. 32 rows: the 16-key unit is the only one built, whatever the environment names)
    auto rows = [&](auto cap) {
        if (args.d.rows > 16) return go(IntTag<2>{}, IntTag<16>{}, cap);
        return unit == 16 ? go(IntTag<1>{}, IntTag<16>{}, cap) : go(IntTag<1>{}, IntTag<32>{}, cap);
    };
    return capped ? rows(BoolTag<true>{}) : rows(BoolTag<false>{});
}

}  // namespace fa
