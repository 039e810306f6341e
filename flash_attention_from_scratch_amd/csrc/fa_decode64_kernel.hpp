// fa_decode64_kernel.hpp -- KV-cache decode attention at d_head = 64 for gfx950: a few query rows per sequence
// against a long 16-bit K / V cache of a per-sequence length the DEVICE holds, with a sliding window and optional attention sinks.
// A text of its own beside fa_decode_kernel.hpp (d_head = 128, whose units stand at the register file's edge): at 64 a key is 128
// bytes, so what the d128 kernel pays per 32-key unit -- two row exchanges, a rescale of O^T, the waits, a page lookup -- would buy
// half the bytes.  So the unit a wave visits is a parameter of this text, UNIT: the whole 64-key tile (8 KiB of K and 8 KiB of V per
// visit, the d128 unit's 16 KiB: what this text was designed around, and what is described below) or 32 keys.  Measured side by side
//  the 32-key unit is as fast where the cache streams and faster under a short window, where it puts twice the
// waves on a row's few keys: it is the one shipped (UNIT_SHIPPED); the other stays instantiated behind FA_DECODE64_UNIT for the bench.
// At UNIT = 32 read below: two key tiles, four V loads, a [32 keys] image, one k-step per d-tile, half the prefetch registers, and
// one running maximum and sum per 32 keys.
//
//  * Split kernel, grid batch * n_kv_heads * num_splits, 4 waves.  The rows = seqlen_q * group query rows that share one K / V head
//    (row r = query position r / group, head kv_head * group + r % group) are the N dimension of v_mfma_f32_16x16x32_{bf16,f16}:
//    NT = 1, 2 or 4 tiles of 16 rows, rows past the last one padded (masked, never stored).  Both products are transposed, so a
//    lane (li = lane & 15, g = lane >> 4) owns query row 16 nt + li:
//        S^T = K Q^T     four 16-key tiles x KS = 2 k-steps; A = 16 keys x 32 d straight from global memory, lane (li, g): key
//                        16 kt + li, d 32 ks + 8 g .. + 7 (16 bytes).  The operand layout ties a lane to ONE key and to a quarter
//                        of a k-step, so a load covers 64-byte half rows; the two k-steps' loads of a key tile are issued back to
//                        back and ask for the two halves of the same sixteen 128-byte rows.  B = Q^T, resident: NT * 2 operands.
//        O^T = V^T P^T   DT16 = 4 d-tiles x two 32-key k-steps; A = V^T by two ds_read_b64_tr_b16 from a wave-private
//                        [64 keys][64 d] LDS image, B = P^T, the S^T accumulators of key tiles 2 h and 2 h + 1 packed in place
//                        (lane group g: keys 4 g .. 4 g + 3 of each).
//    V is fetched in whole rows, 8 keys per load: lane (r = lane >> 3, c = lane & 7) of load i takes key 8 i + vk(r), d 8 c .. + 7,
//    vk(r) = (r >> 1) + 4 (r & 1), and writes its 16 bytes to row 8 i + vk of the image.
//  * The image's row pitch is VROW = 160 bytes = 128 + 32.  Reads: a 32-lane half of a transposed read covers 32 bytes of each of
//    8 consecutive keys; 160 = 5 * 32 with 5 odd, so the eight 32-byte pieces start at the eight different multiples of 32 modulo
//    the 256 bytes of the 64 banks -- every bank once.  Writes: sixteen lanes write two whole rows of 128 bytes; rows k and k + 4
//    lie 640 = 2 * 256 + 128 bytes apart, so the pair vk pairs up (0 4, 1 5, 2 6, 3 7) fills the 256 bytes exactly -- every bank
//    once again.  (Consecutive keys, 160 apart, would overlap in 32 bytes; a pitch of 128 serves the writes and puts all eight
//    keys of a read on the same 32 banks.  The d128 image's 288 = 256 + 32 is the same read argument over 256-byte rows, whose
//    sixteen writing lanes cover ONE row.)
//  * A workgroup reads the length, takes its contiguous share of the key tiles [lo_min / 64, ceil(len / 64)) -- the d128 windowed
//    formula -- and its waves take that share's tiles round-robin.  K AND V of the wave's next tile are requested before the
//    current tile's work, whatever NT is: at NT = 4, Q^T takes 32 VGPRs, O^T 64, S^T 64 and the two prefetch sets 64 each.
//  * One running maximum and sum per row per 64 keys.  The merge of the four waves and the epilogue are the d128 kernel's.
//  * The window is always in: one form, (-1, -1) runs through it; lo <= key < hi per row as one unsigned compare.
//  * Fetch contract (include/fa_hip.h, as at d128): len is clamped to [0, max_len]; a key at or beyond len is FETCHED from key
//    len - 1, one below lo_min = max(0, len - seqlen_q - left) from key lo_min, both masked; block_table entries are clamped to
//    [0, num_pages); no key, page or table entry wholly below lo_min is touched; the prefetch behind a wave's last tile reads one
//    valid row.  page_size % 64 == 0: a tile lies in one page and costs one scalar block_table load.
//  * Sinks are a nullable pointer and act in the epilogue only; no sink is z = -inf through the same instructions, so a null
//    pointer and a tensor of -inf give the same bits.  One split: wave 0's lane folds z into its row behind the merge, against a
//    common maximum (a row without keys: o = 0, lse = z; no inf - inf).  More splits: the partials (num_splits, batch, n_kv_heads,
//    rows, 64) fp32 and lse are sink-free, and fa_decode64_combine_kernel, 64 threads with one d each, takes z as the first member
//    of its fixed-order sums.  No atomics: the same bits for the same inputs and the same num_splits.
//  * scale = 1 / sqrt(64); c = scale * log2(e), rounded once from the double product.
//
// What an fp8 cache changes (OCP e4m3fn, Decode64Fp8Args: the arguments above and one fp32 descale per (batch entry, K / V head) and
// tensor; `if constexpr (FP8)` marks every site).  A key is 64 bytes, not 128, and everything above that was argued
// from 128 is argued again here.  Q, O, the grid, the four waves, NT, the transposed products, the split of the key tiles, the units'
// round-robin, the merge, the sink-free partials, fa_decode64_combine_kernel, the window and the fetch contract are as above, word
// for word (strides and offsets of the cache count bytes).
//  * K: ONE 16-byte load per lane and 16-key tile serves both k-steps.  Lane (li, g) loads key 16 kt + li, d 16 g .. 16 g + 15: the
//    four lanes of a key ask for its whole 64-byte row, so a wave load covers sixteen whole rows (the 16-bit form's covers sixteen
//    half rows, and needs its second load for the other halves).  Bytes 8 s .. 8 s + 7 of the load are the lane's A operand of k-step
//    s: element e of k-step s in lane group g multiplies d = 16 g + 8 s + e.  Q^T is loaded once in the same permutation of d (a dot
//    product does not mind the order of its terms).  K stays fp8 in the prefetch registers -- 4 VGPRs per key tile against 8 -- and
//    is converted with cvt_fp8x8 (v_cvt_scalef32_pk_{bf16,f16}_fp8, scale 1: every finite e4m3fn value is exact in both) right before
//    its two MFMAs.
//  * V: whole 64-byte rows, four lanes per key, sixteen keys per load: lane (q = (lane >> 2) & 3, c = lane & 3) of lane group g
//    and load i takes key 16 i + vk8, d 16 c .. + 15, vk8 = 8 (g >> 1) + 2 (g & 1) + (q & 1) + 4 (q >> 1).  It converts its 16
//    values and writes them to row 16 i + vk8 of the wave's 16-bit image as two 16-byte writes, columns 32 c and 32 c + 16 (bytes).
//    The image, its pitch VROW = 160 and the transposed reads are the 16-bit form's: nothing of the read argument changes.
//    Writes: sixteen lanes (one lane group g, what a 16-byte write serves per pass) now cover FOUR rows, and one write of a lane
//    covers only half of the lane's 32 bytes.  In 16-byte slots modulo the banks' 256 bytes, row k starts at 10 k mod 16 -- always
//    even -- and a lane's two halves are slots 10 k + 2 c + {0, 1}.  Written "low halves first", a pass would put its sixteen lanes
//    on the eight even slots: a two-way conflict under ANY map of lanes to keys, which is why the 16-bit form's pairing alone does
//    not carry over.  So the lanes of odd q write their HIGH half first (h = q & 1: the first write goes to slot 10 k + 2 c + h, the
//    second to 10 k + 2 c + 1 - h; the halves are picked on the fp8 words, four v_cndmask per load, before the conversion).  A pass
//    then wants two rows on the even slots and two on the odd ones, each pair covering all eight: rows k and k' cover disjoint
//    halves of the even (odd) slots iff 10 (k - k') = 8 mod 16, i.e. k - k' = 4 mod 8 -- the 16-bit form's pairs (k, k + 4) again.
//    vk8 deals a pass the rows {k, k + 4} with h = 0 and {k + 1, k + 5} with h = 1, k = 8 (g >> 1) + 2 (g & 1): group 0 writes
//    rows 0 4 (slots 0 2 4 6, 8 10 12 14) and 1 5 (11 13 15 1, 3 5 7 9) -- every bank once, in both writes.
//  * Prefetch: a 32-key unit is 2 K and 2 V loads of 16 bytes per lane (16-bit: 4 and 4) and 16 VGPRs (32).  With the 16-bit form's
//    one unit ahead a wave would keep half the bytes in flight, so the distance is a parameter of this text beside UNIT: DIST = 1 or
//    2 units ahead, DIST + 1 register sets taken in turn.  At NT = 4 and UNIT = 32: Q^T 32, O^T 64, S^T 32 and three sets of 16.
//    (32, 1), (32, 2) and (64, 1) are instantiated and measured side by side ((64, 2) would keep twice the others'
//    most in flight and, at NT = 4, needs scratch: not built); FA_DECODE64_UNIT and FA_DECODE64_AHEAD name one outright.  Where the
//    cache streams the three are within the A/A spread of each other; under a short window (32, 1) is the fastest: it is shipped.
//  * Descales: one scalar each per workgroup, read once; a null pointer means 1; no address depends on either.  k_descale folds
//    into c = k_descale * (log2(e) / 8) (a float product; with k_descale = 1 the 16-bit form's c): S^T and m stay in raw logit
//    units, and lse = m * k_descale / 8 + log l (a positive descale keeps the maximum the maximum).  v_descale folds into the final
//    1 / l.  The sink meets the dequantized logit: ms = m * k_descale / 8 in the epilogue; the partials' lse carry it too, so the
//    combine kernel is unchanged.  A row without keys: o = 0, lse = z.
#pragma once
#include "fa_decode_kernel.hpp"

namespace fa {

struct Decode64Args {
    DecodeArgs d;           // part_o: (num_splits, batch, n_kv_heads, rows, 64)
    int32_t left, right;    // -1 = unbounded (causal: right = 0)
    const float *sinks;     // (n_heads) fp32, DEVICE, or null
};

// the 16-bit form's arguments (k, v: the fp8 bytes; kv_*: strides in bytes) and the descales
struct Decode64Fp8Args {
    Decode64Args w;
    const float *k_descale, *v_descale;   // (batch, n_kv_heads), row stride ds_bs; null = 1
    int64_t ds_bs;
};

namespace decode64 {
constexpr int D = 64, TILE = 64, NWAVES = 4, THREADS = NWAVES * 64;
constexpr int VROW = 160;              // bytes per key of the V image (the argument is at the head of this file)
constexpr int UNIT_SHIPPED = 32;       // keys per wave visit: 32 or 64, measured side by side
constexpr int FP8_UNIT_SHIPPED = 32, FP8_DIST_SHIPPED = 1;   // the fp8 form's unit and prefetch distance, measured side by side
__host__ __device__ inline const Decode64Args &common(const Decode64Args &a) { return a; }
__host__ __device__ inline const Decode64Args &common(const Decode64Fp8Args &a) { return a.w; }
template <class ARGS> constexpr bool is_fp8 = std::is_same_v<ARGS, Decode64Fp8Args>;
}  // namespace decode64

// One text for both caches: ARGS names the form, DIST the units a wave's loads run ahead of its work (16-bit: 1).  (The two are the
// kernel's own parameters, defaulted -- behind a shared body called from two kernels the 16-bit kernels' instructions come out in
// another order; so they keep theirs, and only their mangled names grow by the two defaults.)
template <int DT, int NT, bool PAGED, int UNIT, class ARGS = Decode64Args, int DIST = 1>
__global__ void __launch_bounds__(decode64::THREADS) fa_decode64_split_kernel(const ARGS full) {
    using E = Elem<DT>;
    using vec8 = typename E::vec8;
    using namespace decode64;
    constexpr bool FP8 = is_fp8<ARGS>;
    static_assert(UNIT == 64 || UNIT == 32, "a unit is a whole 64-key tile or half of one");
    static_assert(DIST == 1 || (FP8 && DIST == 2), "one unit ahead; an fp8 cache: one or two");
    const Decode64Args &args = common(full);
    constexpr int KS = D / 32, DT16 = D / 16, KT = UNIT / 16, VL = FP8 ? UNIT / 16 : UNIT / 8, UPT = TILE / UNIT;   // (VL: V loads, UPT: units per tile)
    constexpr int VBYTES = UNIT * VROW;   // one wave's image
    constexpr int MERGE = NT * DT16 * 64 * 16;   // one wave's accumulators
    constexpr int MAIN = NWAVES * VBYTES > MERGE ? NWAVES * VBYTES : MERGE;
    __shared__ __attribute__((aligned(16))) char smem[MAIN + (NWAVES + 1) * NT * 16 * 4];
    const DecodeArgs &a = args.d;
    struct KRegs16 { vec8 r[KT][KS]; };   // one 64-key unit in the prefetch registers: 16 bytes per lane and load
    struct KRegs8 { u32x4 r[KT]; };       // (fp8: one load per key tile, both k-steps)
    using KRegs = std::conditional_t<FP8, KRegs8, KRegs16>;
    struct VRegs { std::conditional_t<FP8, u32x4, s16x8> r[VL]; };
    [[maybe_unused]] const uint8_t *const k8 = (const uint8_t *)a.k, *const v8 = (const uint8_t *)a.v;   // fp8: the cache's bytes

    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int li = lane & 15, g = lane >> 4;
    // V's load shape: key 8 i + vk, d 8 vc .. (fp8: key 16 i + vk, d 16 vc .., and vh: the lane writes its high half first)
    const int vc = FP8 ? lane & 3 : lane & 7;
    const int vk = FP8 ? 8 * (g >> 1) + 2 * (g & 1) + ((lane >> 2) & 1) + 4 * ((lane >> 3) & 1) : (lane >> 4) + 4 * ((lane >> 3) & 1);
    [[maybe_unused]] const bool vh = (lane >> 2) & 1;
    const int nsp = a.num_splits;
    const int split = blockIdx.x % nsp, kvh = (blockIdx.x / nsp) % a.n_kv_heads, b = blockIdx.x / (nsp * a.n_kv_heads);

    int len = a.cache_seqlens[b];
    len = len < 0 ? 0 : (len > a.max_len ? a.max_len : len);
    const int n_tiles = (len + TILE - 1) / TILE;
    int lo_min = 0;   // the lowest key a row of this workgroup sees (<= len - 1 when len > 0)
    if (args.left >= 0) {
        const int64_t lo = (int64_t)len - a.seqlen_q - args.left;
        lo_min = lo > 0 ? (int)lo : 0;
    }
    const int tl = lo_min / TILE, nt_w = n_tiles - tl;   // (len = 0: lo_min = 0, no tile)
    const int t0 = tl + (int)((int64_t)nt_w * split / nsp), t1 = tl + (int)((int64_t)nt_w * (split + 1) / nsp);
    // the split's units: whole tiles, less the units of its lowest tile wholly below lo_min and of its last one at or beyond len
    const int n_units = (len + UNIT - 1) / UNIT;
    const int u_begin = UPT * t0 > lo_min / UNIT ? UPT * t0 : lo_min / UNIT, u_end = UPT * t1 < n_units ? UPT * t1 : n_units;

    [[maybe_unused]] float kd = 1.0f, vd = 1.0f;
    if constexpr (FP8) {
        kd = full.k_descale ? full.k_descale[(int64_t)b * full.ds_bs + kvh] : 1.0f;
        vd = full.v_descale ? full.v_descale[(int64_t)b * full.ds_bs + kvh] : 1.0f;
    }

    // Q^T, resident (fp8: in K's permutation of d); pos: the row's position p = len - seqlen_q + query position, from which each unit derives the row's bounds
    // p - w_left and min(len, p + w_right + 1) -- neither needs its clamp at 0, keys are not negative
    vec8 Qr[NT][KS];
    int pos[NT];
    constexpr int FAR = (1 << 30) + 64;   // unbounded, or beyond what any length reaches (the host: len <= 2^30 - 128; p >= -64): all one
    const int w_left = args.left < 0 || args.left > FAR ? FAR : args.left;
    const int w_right = args.right < 0 || args.right > FAR ? FAR : args.right;
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
        const int r = nt * 16 + li;
        const bool valid = r < a.rows;
        const int rr = valid ? r : 0, qi = rr / a.group, qh = kvh * a.group + rr % a.group;
        const uint16_t *qp = a.q + (int64_t)b * a.q_bs + (int64_t)qi * a.q_ss + (int64_t)qh * a.q_hs + g * (FP8 ? 16 : 8);
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) Qr[nt][ks] = *(const vec8 *)(qp + ks * (FP8 ? 8 : 32));
        pos[nt] = !valid ? -(1 << 30) - 66 : len - a.seqlen_q + qi;   // (a padded row: p + w_right + 1 < 0)
    }

    float scale, c;   // logits (fp8: raw logits) -> logits, and -> the exponent of exp2
    if constexpr (FP8) {
        scale = kd * 0.125f;
        c = kd * 0.18033688011112042592f;   // log2(e) / 8
    } else {
        scale = 1.0f / __builtin_sqrtf((float)D);
        c = (float)((double)scale * 1.4426950408889634074);
    }
    const float ninf = -__builtin_inff();

    f32x4 O[NT][DT16];
    float m[NT], l[NT];
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
#pragma unroll
        for (int t = 0; t < DT16; ++t) O[nt][t] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
        m[nt] = ninf;
        l[nt] = 0.0f;
    }

    // One unit's K and V, 16 loads of 16 bytes per lane.  A unit at or beyond u_end (the prefetch behind a wave's last unit) is
    // still loaded, every lane from one row of unit `u_valid`: one cached row instead of 16 KiB, and the number of loads in flight
    // is the same on every path.  A key below lo_min comes from key lo_min, one at or beyond len from key len - 1.
    auto load_unit = [&](int u, int u_valid, KRegs &Kr, VRegs &Vr) {
        const bool real = u < u_end;
        const int key0 = (real ? u : u_valid) * UNIT;
        int64_t base;
        int row0;
        if constexpr (PAGED) {
            const int page = key0 / a.page_size;
            // a scalar load (the compiler's own would be a vector load behind the unit's own: waiting for it would drain them all)
            int p;
            asm volatile("s_load_dword %0, %1, 0x0\n\ts_waitcnt lgkmcnt(0)" : "=s"(p) : "s"(a.block_table + (int64_t)b * a.bt_bs + page) : "memory");
            p = p < 0 ? 0 : (p >= a.num_pages ? a.num_pages - 1 : p);
            base = (int64_t)p * a.kv_bs + (int64_t)kvh * a.kv_hs;
            row0 = key0 - page * a.page_size;
        } else {
            base = (int64_t)b * a.kv_bs + (int64_t)kvh * a.kv_hs;
            row0 = key0;
        }
        const int first = lo_min > key0 ? lo_min - key0 : 0;
        const int last = real ? len - 1 - key0 : first;
        auto clamp_key = [&](int ko) {
            ko = ko < first ? first : ko;
            return ko < last ? ko : last;
        };
        if constexpr (FP8) {
#pragma unroll
            for (int kt = 0; kt < KT; ++kt) Kr.r[kt] = *(const u32x4 *)(k8 + base + (int64_t)(row0 + clamp_key(kt * 16 + li)) * a.kv_ss + g * 16);
#pragma unroll
            for (int i = 0; i < VL; ++i) Vr.r[i] = *(const u32x4 *)(v8 + base + (int64_t)(row0 + clamp_key(i * 16 + vk)) * a.kv_ss + vc * 16);
        } else {
#pragma unroll
            for (int kt = 0; kt < KT; ++kt) {
                const uint16_t *kp = a.k + base + (int64_t)(row0 + clamp_key(kt * 16 + li)) * a.kv_ss + g * 8;
#pragma unroll
                for (int ks = 0; ks < KS; ++ks) Kr.r[kt][ks] = *(const vec8 *)(kp + ks * 32);
            }
#pragma unroll
            for (int i = 0; i < VL; ++i) Vr.r[i] = *(const s16x8 *)(a.v + base + (int64_t)(row0 + clamp_key(i * 8 + vk)) * a.kv_ss + vc * 8);
        }
    };

    char *vs = smem + wave * VBYTES;
    char *vwr = vs + vk * VROW + vc * (FP8 ? 32 : 16);   // (fp8: the lane's 32 bytes; its first write goes to + 16 vh, its second to + 16 (1 - vh))
    const char *vrd = vs + (4 * g + (li >> 2)) * VROW + (li & 3) * 8;   // lane 4 q + p of a group: row q, columns 4 p ..
    auto compute_unit = [&](int u, const KRegs &Kr, const VRegs &Vr) {
        if constexpr (FP8) {
#pragma unroll
            for (int i = 0; i < VL; ++i) {
                const u32x4 w = Vr.r[i];
                *(vec8 *)(vwr + i * 16 * VROW + (vh ? 16 : 0)) = cvt_fp8x8<DT>(vh ? w[2] : w[0], vh ? w[3] : w[1]);
                *(vec8 *)(vwr + i * 16 * VROW + (vh ? 0 : 16)) = cvt_fp8x8<DT>(vh ? w[0] : w[2], vh ? w[1] : w[3]);
            }
        } else {
#pragma unroll
            for (int i = 0; i < VL; ++i) *(s16x8 *)(vwr + i * 8 * VROW) = Vr.r[i];
        }
        f32x4 S[NT][KT];
#pragma unroll
        for (int nt = 0; nt < NT; ++nt)
#pragma unroll
            for (int kt = 0; kt < KT; ++kt) S[nt][kt] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
        for (int kt = 0; kt < KT; ++kt)
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) {
                vec8 ka;
                if constexpr (FP8) ka = cvt_fp8x8<DT>(Kr.r[kt][2 * ks], Kr.r[kt][2 * ks + 1]);
                else ka = Kr.r[kt][ks];
#pragma unroll
                for (int nt = 0; nt < NT; ++nt) S[nt][kt] = E::mfma16(ka, Qr[nt][ks], S[nt][kt]);
            }
        vec8 Pb[NT][UNIT / 32];
        const int key_g = u * UNIT + 4 * g;
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
            // lo <= key < hi as ONE unsigned compare, key - lo < span
            const int hi = pos[nt] + w_right + 1 < len ? pos[nt] + w_right + 1 : len;
            const int lo = (int)((unsigned)pos[nt] - (unsigned)w_left);   // (a padded row may wrap: hi < 0 masks it)
            const unsigned span = hi > lo ? (unsigned)hi - (unsigned)lo : 0u;
            const unsigned from_lo = (unsigned)key_g - (unsigned)lo;
            float s[4 * KT];
            float mx = ninf;
#pragma unroll
            for (int j = 0; j < 4 * KT; ++j) {   // element j: key 16 (j >> 2) + 4 g + (j & 3) of the unit
                const bool seen = from_lo + (unsigned)(16 * (j >> 2) + (j & 3)) < span;
                s[j] = seen ? S[nt][j >> 2][j & 3] : ninf;
                mx = fmaxf(mx, s[j]);
            }
            const float m_new = fmaxf(m[nt], quad_max(mx));
            const float m_ref = m_new == ninf ? 0.0f : m_new;   // a row that has seen no key yet: no inf - inf
            const float alpha = __builtin_amdgcn_exp2f((m[nt] - m_ref) * c);
            m[nt] = m_new;
            l[nt] *= alpha;
#pragma unroll
            for (int t = 0; t < DT16; ++t) O[nt][t] *= alpha;
            const float neg_mc = -(m_ref * c);
            float p[4 * KT], rowsum = 0.0f;
#pragma unroll
            for (int j = 0; j < 4 * KT; ++j) {
                p[j] = __builtin_amdgcn_exp2f(__builtin_fmaf(s[j], c, neg_mc));
                rowsum += p[j];
            }
            l[nt] += rowsum;
#pragma unroll
            for (int h = 0; h < UNIT / 32; ++h) Pb[nt][h] = E::pack8(p + 8 * h);
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // the wave's V image is written
#pragma unroll
        for (int h = 0; h < UNIT / 32; ++h)
#pragma unroll
            for (int t = 0; t < DT16; ++t) {
                s16x8 av;
                av.lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((FA_LDS(s16x4) *)(vrd + h * 32 * VROW + t * 32));
                av.hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((FA_LDS(s16x4) *)(vrd + (h * 32 + 16) * VROW + t * 32));
#pragma unroll
                for (int nt = 0; nt < NT; ++nt) O[nt][t] = E::mfma16(__builtin_bit_cast(vec8, av), Pb[nt][h], O[nt][t]);
            }
        asm volatile("" ::: "memory");   // ... and read before the next unit's is written
    };

    // Two register sets, A and B, taken in turn (the loop is unrolled by two, so no set is ever copied into the other): a unit's
    // loads are issued before the previous unit's work and waited for with the next unit's loads still in flight.
    // fp8: DIST + 1 sets taken in turn the same way; set s holds the unit of step s, and its loads were issued DIST steps before.
    if constexpr (FP8) {
        KRegs Kr[DIST + 1];
        VRegs Vr[DIST + 1];
        int u = u_begin + wave;
        // (the calls are inlined by attribute: left to its cost model, the inliner keeps the 64-row, 64-key form's compute_unit a
        // call, with its closure and the register sets in scratch; on the lambdas themselves the attribute would reach the 16-bit kernels)
        if (u < u_end) static_for<0, DIST>([&](auto d) __attribute__((always_inline)) {
            [[clang::always_inline]] load_unit(u + decltype(d)::value * NWAVES, u, Kr[decltype(d)::value], Vr[decltype(d)::value]);
        });
        while (u < u_end) {
            static_for<0, DIST + 1>([&](auto step) __attribute__((always_inline)) {
                constexpr int s = decltype(step)::value, into = (s + DIST) % (DIST + 1);
                if (u < u_end) {   // (false once: so are the steps behind it, u stays)
                    [[clang::always_inline]] load_unit(u + DIST * NWAVES, u, Kr[into], Vr[into]);
                    __builtin_amdgcn_sched_barrier(0);
                    [[clang::always_inline]] compute_unit(u, Kr[s], Vr[s]);
                    u += NWAVES;
                }
            });
        }
    } else {
        KRegs Ka, Kb;
        VRegs Va, Vb;
        int u = u_begin + wave;
        if (u < u_end) load_unit(u, u, Ka, Va);
        while (u < u_end) {
            load_unit(u + NWAVES, u, Kb, Vb);
            __builtin_amdgcn_sched_barrier(0);   // the requests go out before the unit's work, not where the scheduler finds room
            compute_unit(u, Ka, Va);
            u += NWAVES;
            if (u >= u_end) break;
            load_unit(u + NWAVES, u, Ka, Va);
            __builtin_amdgcn_sched_barrier(0);
            compute_unit(u, Kb, Vb);
            u += NWAVES;
        }
    }

    // the four waves' states into wave 0: one reference per row for all of them, then plain sums in wave order
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) l[nt] = quad_sum(l[nt]);
    float *m_sh = (float *)(smem + MAIN), *l_sh = m_sh + NWAVES * NT * 16, *o_sh = (float *)smem;
    __syncthreads();   // every wave is done with its V image
    if (g == 0) {
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) m_sh[(wave * NT + nt) * 16 + li] = m[nt];
    }
    __syncthreads();
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
        float m_all = ninf;
#pragma unroll
        for (int w = 0; w < NWAVES; ++w) m_all = fmaxf(m_all, m_sh[(w * NT + nt) * 16 + li]);
        const float m_ref = m_all == ninf ? 0.0f : m_all;
        const float alpha = __builtin_amdgcn_exp2f((m[nt] - m_ref) * c);
        m[nt] = m_all;
        l[nt] *= alpha;
#pragma unroll
        for (int t = 0; t < DT16; ++t) O[nt][t] *= alpha;
    }
    for (int w = 1; w < NWAVES; ++w) {
        if (wave == w) {
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) {
#pragma unroll
                for (int t = 0; t < DT16; ++t) *(f32x4 *)(o_sh + ((nt * DT16 + t) * 64 + lane) * 4) = O[nt][t];
                if (g == 0) l_sh[nt * 16 + li] = l[nt];
            }
        }
        __syncthreads();
        if (wave == 0) {
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) {
#pragma unroll
                for (int t = 0; t < DT16; ++t) O[nt][t] += *(const f32x4 *)(o_sh + ((nt * DT16 + t) * 64 + lane) * 4);
                l[nt] += l_sh[nt * 16 + li];
            }
        }
        __syncthreads();
    }
    if (wave != 0) return;

    // lane (li, g) holds row 16 nt + li, d 16 t + 4 g .. + 3
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
        const int r = nt * 16 + li;
        if (r >= a.rows) continue;
        const bool any = l[nt] > 0.0f;
        const int qi = r / a.group, qh = kvh * a.group + r % a.group;
        if (nsp == 1) {
            // The row's sink joins here, once; none is z = -inf.  Natural units against a common maximum, so that neither term
            // overflows; a row without keys takes 0 for its m = -inf and is selected out (o = 0, lse = z), so no inf - inf is
            // formed (where l > 0, m is finite and so is M)
            const float z = args.sinks ? args.sinks[qh] : ninf, ms = any ? m[nt] * scale : 0.0f;
            const float M = fmaxf(ms, z);
            const float al = __expf(ms - M), l_all = __builtin_fmaf(l[nt], al, __expf(z - M));
            float inv = any ? al / l_all : 0.0f;
            if constexpr (FP8) inv = any ? vd * al / l_all : 0.0f;
            const float lse = any ? M + __logf(l_all) : z;
            uint16_t *op = a.o + (int64_t)b * a.o_bs + (int64_t)qi * a.o_ss + (int64_t)qh * a.o_hs + 4 * g;
#pragma unroll
            for (int t = 0; t < DT16; ++t) {
                u32x2 w;
                w[0] = E::pack2(O[nt][t][0] * inv, O[nt][t][1] * inv);
                w[1] = E::pack2(O[nt][t][2] * inv, O[nt][t][3] * inv);
                *(u32x2 *)(op + 16 * t) = w;
            }
            if (a.lse && g == 0) a.lse[((int64_t)b * a.n_heads + qh) * a.seqlen_q + qi] = lse;
        } else {   // a sink-free partial: o normalised, lse = -inf for a row that saw no key in this split
            const float inv = any ? (FP8 ? vd : 1.0f) / l[nt] : 0.0f;
            const int64_t row = (((int64_t)split * a.batch + b) * a.n_kv_heads + kvh) * a.rows + r;
            float *pp = a.part_o + row * D + 4 * g;
#pragma unroll
            for (int t = 0; t < DT16; ++t) *(f32x4 *)(pp + 16 * t) = O[nt][t] * inv;
            if (g == 0) a.part_lse[row] = any ? m[nt] * scale + __logf(l[nt]) : ninf;
        }
    }
}

// one workgroup of 64 threads per (batch, K / V head, row); thread i: d i.  The row's sink (none: z = -inf) is the first member of
// the fixed-order sums: mx = max(z, max_s lse_s), sum = exp(z - mx) + sum_s exp(lse_s - mx), lse = mx + log sum,
// o = sum_s exp(lse_s - lse) o_s in split order, rounded once; mx = -inf (no key, no sink): o = 0, lse = -inf.
template <int DT>
__global__ void __launch_bounds__(64) fa_decode64_combine_kernel(const Decode64Args args) {
    using E = Elem<DT>;
    const DecodeArgs &a = args.d;
    const int64_t row = blockIdx.x, n_rows = (int64_t)a.batch * a.n_kv_heads * a.rows;
    const int r = (int)(row % a.rows), kvh = (int)((row / a.rows) % a.n_kv_heads), b = (int)(row / ((int64_t)a.rows * a.n_kv_heads));
    const int qi = r / a.group, qh = kvh * a.group + r % a.group;
    const float ninf = -__builtin_inff(), z = args.sinks ? args.sinks[qh] : ninf;
    float mx = z;
    for (int s = 0; s < a.num_splits; ++s) mx = fmaxf(mx, a.part_lse[s * n_rows + row]);
    float lse = ninf, o = 0.0f;
    if (mx != ninf) {
        float sum = __expf(z - mx);
        for (int s = 0; s < a.num_splits; ++s) sum += __expf(a.part_lse[s * n_rows + row] - mx);
        lse = mx + __logf(sum);
        for (int s = 0; s < a.num_splits; ++s)
            o = __builtin_fmaf(__expf(a.part_lse[s * n_rows + row] - lse), a.part_o[(s * n_rows + row) * decode64::D + threadIdx.x], o);
    }
    uint16_t *op = a.o + (int64_t)b * a.o_bs + (int64_t)qi * a.o_ss + (int64_t)qh * a.o_hs;
    op[threadIdx.x] = (uint16_t)E::pack2(o, 0.0f);
    if (a.lse && threadIdx.x == 0) a.lse[((int64_t)b * a.n_heads + qh) * a.seqlen_q + qi] = lse;
}

hipError_t decode64_enqueue(const Decode64Args &a, int dtype, hipStream_t s);          // fa_decode64.hip
hipError_t decode64_fp8_enqueue(const Decode64Fp8Args &a, int dtype, hipStream_t s);   // fa_decode64_fp8.hip

}  // namespace fa
