// fa_decode_kernel.hpp -- KV-cache decode attention for gfx950: a few query rows per sequence against a long K / V cache of
// a per-sequence length the DEVICE holds, the cache in Q's 16-bit type or in fp8 (OCP e4m3fn).
// HBM-bound: K and V are read once, ~2 * rows FLOP per byte.  One text of the split kernel serves both caches: ARGS names
// the form (DecodeArgs: 16-bit, DecodeFp8Args: fp8) and `if constexpr (FP8)` marks every site where they differ.
//
//  * Split kernel, grid batch * n_kv_heads * num_splits, 4 waves.  The rows = seqlen_q * group query rows that share one K / V
//    head (row r = query position r / group, head kv_head * group + r % group) are the N dimension of
//    v_mfma_f32_16x16x32_{bf16,f16}: NT = 1, 2 or 4 tiles of 16 rows, rows past the last one padded (masked, never stored).
//    Both products are transposed as in fa_fwd_kernel16.hpp, so a lane owns one query row and the statistics need two
//    row exchanges:
//        S^T = K Q^T     A = 16 keys x 32 d straight from global memory (16 bytes per lane), B = Q^T resident in VGPRs
//        O^T = V^T P^T   A = V^T by two ds_read_b64_tr_b16 from a wave-private [32 keys][128 d] LDS image, B = P^T, the
//                        S^T accumulators of two 16-key tiles packed in place (lane group g: keys 4g .. 4g+3 of each)
//    A workgroup reads the length, takes its contiguous share of the ceil(len / 64) key tiles, and its waves take that share's
//    32-key units round-robin, each prefetching its next unit's K and V into registers under the current unit's work.  No
//    workgroup barrier inside the loop: the V image is the wave's own (DS operations of one wave complete in order).  At
//    the end the waves agree on the row maxima through LDS and wave 0 adds the others' accumulators in wave order.
//    num_splits == 1: o and lse are written; else an fp32 (o normalised, lse) partial per split, lse = -inf for an empty one.
//  * Combine kernel, one 64-thread workgroup per (batch, head, row): lse = logsumexp_s lse_s, o = sum_s exp(lse_s - lse) o_s
//    in split order, rounded once.  No atomics: the same bits for the same inputs and the same num_splits.
//  * Clamping (include/fa_hip.h): len to [0, max_len]; a key at or beyond len is FETCHED from key len - 1 (K and V: a
//    p = 0 would not silence a NaN in V) and masked in S; block_table entries to [0, num_pages), only those of pages below
//    ceil(len / page_size) read.  page_size % 64 == 0, so a 32-key unit lies in one page.
//
// What fp8 changes (one fp32 descale per (batch entry, K / V head) and tensor; Q, O, the partials and the combine kernel, the
// grid, the four waves, the row packing, the split of the key tiles, the clamping and the merge of the waves are as above):
//  * K and V are fetched as fp8, 16 bytes per lane and load, 8 loads per 32-key unit (the 16-bit form: 16):
//        K   lane (li, g), load (kt, j): key 16 kt + li, d 64 j + 16 g .. + 15 -- 64-byte row segments, as in the 16-bit form.
//            Bytes 8 h .. 8 h + 7 of the load are the lane's A operand of MFMA k-step s = 2 j + h, so k-step s, lane group g,
//            element e multiplies d = 64 (s >> 1) + 16 g + 8 (s & 1) + e; Q^T is loaded in the same permutation of d (a dot
//            product does not mind the order of its terms)
//        V   lane (r = lane >> 3, c = lane & 7), load i: key 8 i + r, d 16 c .. + 15 -- whole 128-byte rows
//    K stays fp8 in the prefetch registers and is converted to Q's type (v_cvt_scalef32_pk_{bf16,f16}_fp8, scale 1: every finite
//    e4m3 value is exact in both) right before its MFMAs; V is converted before it is written to the wave's 16-bit LDS image,
//    whose layout and transposed reads are unchanged.
//  * k_descale is folded into the exponent's constant c = k_descale / sqrt(128) * log2(e) (a float product; the 16-bit form
//    rounds the double product once): S and the running maximum m stay in raw (undescaled) logit units, and
//    lse = m * k_descale / sqrt(128) + log(l).  (A positive descale keeps the maximum the maximum.)  v_descale is folded into
//    the final 1 / l.  Both are one scalar per workgroup; no address depends on either.
//  * A prefetch register set is 32 VGPRs instead of 64, so the 64-row form holds V a unit ahead as the others do.
//
// What a sliding window changes (DecodeWindowArgs / DecodeFp8WindowArgs: the forms above and (left, right), -1 = unbounded;
// `if constexpr (WINDOW)` marks the sites).  Row i at position p = len - seqlen_q + i sees the keys
// max(0, p - left) .. min(len - 1, p + right); causal arrives as right = 0.  lo_min = max(0, len - seqlen_q - left) is the
// lowest key any row of the workgroup sees:
//  * the workgroup's key tiles are [lo_min / 64, ceil(len / 64)), shared by the splits with the same formula, and the first
//    32-key unit a wave visits is at or above lo_min / 32: no key, page or block_table entry wholly below lo_min is touched;
//  * a lane whose key lies below lo_min FETCHES key lo_min (as one at or beyond len fetches len - 1) and is masked;
//  * the mask is lo <= key < hi per row, both derived from the row's position.  The partial format, the combine kernel and the
//    merge are unchanged.
//
// What logit soft-capping changes (DecodeSoftcapArgs / DecodeFp8SoftcapArgs: the windowed forms -- a window of (-1, -1) runs through
// them -- and the cap's A = softcap sqrt(128) and 1 / A; `if constexpr (CAP)` marks the sites):
//  * in compute_unit every S accumulator goes through A tanh(S / A) = A - 2 A / (exp2(S cap_k) + 1), cap_k = 2 log2(e) / A, one
//    v_exp_f32 and one v_rcp_f32 per element, right behind the S^T MFMAs and in front of the `seen` select, a row tile at a time
//    (no second S-sized array lives): a masked key stays -inf (tanh(-inf) = -1 would bring it back to life).  exp2 overflowing
//    gives A, underflowing -A: no NaN at either end;
//  * fp8: a tanh between S and the exponent forbids folding k_descale into c, so it goes into cap_k = k_descale 2 log2(e) / A, one
//    scalar per workgroup; the capped S is in the 16-bit form's units, scale and c are the 16-bit form's constants, and
//    lse = m / sqrt(128) + log(l).  The combine kernel, the partial format, the merge, the fetch contract and lo_min are unchanged.
#pragma once
#include <type_traits>

#include "fa_fwd_kernel16.hpp"

namespace fa {

struct DecodeArgs {
    const uint16_t *q, *k, *v;
    uint16_t *o;
    float *lse;                    // (batch, n_heads, seqlen_q) or null
    const int32_t *cache_seqlens;  // (batch)
    const int32_t *block_table;    // (batch, bt_bs) or null
    float *part_o, *part_lse;      // (num_splits, batch, n_kv_heads, rows, 128) and (num_splits, batch, n_kv_heads, rows)
    int64_t q_bs, q_ss, q_hs, o_bs, o_ss, o_hs;
    int64_t kv_bs, kv_ss, kv_hs;   // kv_bs: batch stride, or the page stride of a paged cache
    int64_t bt_bs;
    int32_t batch, seqlen_q, n_heads, n_kv_heads, group, rows;
    int32_t max_len, page_size, num_pages, num_splits, causal;
};

// the 16-bit path's arguments (k, v: the fp8 bytes; kv_*: strides in bytes = elements) and the descales
struct DecodeFp8Args {
    DecodeArgs d;
    const float *k_descale, *v_descale;   // (batch, n_kv_heads), row stride ds_bs; null = 1
    int64_t ds_bs;
};

// ... and a sliding window: left / right keys a row sees below / above its own position, -1 = unbounded (causal: right = 0)
struct DecodeWindowArgs {
    DecodeArgs d;
    int32_t left, right;
};
struct DecodeFp8WindowArgs {
    DecodeFp8Args f;
    int32_t left, right;
};

// ... and logit soft-capping on the windowed forms: A = softcap * sqrt(128) and 1 / A (the host rounds each once)
struct DecodeSoftcapArgs {
    DecodeWindowArgs w;
    float cap_a, cap_inv_a;
};
struct DecodeFp8SoftcapArgs {
    DecodeFp8WindowArgs w;
    float cap_a, cap_inv_a;
};

namespace decode {
constexpr int D = 128, UNIT = 32, TILE = 64, NWAVES = 4, THREADS = NWAVES * 64;
constexpr int VROW = 288;              // bytes per key of the V image: 256 + 32, so the 8 keys a 32-lane half's transposed read
                                       // covers (32 bytes of each) fall on all 64 banks
constexpr int VBYTES = UNIT * VROW;    // one wave's image
constexpr int row_tiles(int rows) { return rows <= 16 ? 1 : rows <= 32 ? 2 : 4; }

// what both forms share of their arguments
__host__ __device__ inline const DecodeArgs &common(const DecodeArgs &a) { return a; }
__host__ __device__ inline const DecodeArgs &common(const DecodeFp8Args &a) { return a.d; }
__host__ __device__ inline const DecodeArgs &common(const DecodeWindowArgs &a) { return a.d; }
__host__ __device__ inline const DecodeArgs &common(const DecodeFp8WindowArgs &a) { return a.f.d; }
__host__ __device__ inline const DecodeArgs &common(const DecodeSoftcapArgs &a) { return a.w.d; }
__host__ __device__ inline const DecodeArgs &common(const DecodeFp8SoftcapArgs &a) { return a.w.f.d; }
// the fp8 forms' descales
__host__ __device__ inline const DecodeFp8Args &fp8_part(const DecodeFp8Args &a) { return a; }
__host__ __device__ inline const DecodeFp8Args &fp8_part(const DecodeFp8WindowArgs &a) { return a.f; }
__host__ __device__ inline const DecodeFp8Args &fp8_part(const DecodeFp8SoftcapArgs &a) { return a.w.f; }
template <class ARGS> constexpr bool is_cap = std::is_same_v<ARGS, DecodeSoftcapArgs> || std::is_same_v<ARGS, DecodeFp8SoftcapArgs>;
template <class ARGS>
constexpr bool is_fp8 = std::is_same_v<ARGS, DecodeFp8Args> || std::is_same_v<ARGS, DecodeFp8WindowArgs> || std::is_same_v<ARGS, DecodeFp8SoftcapArgs>;
template <class ARGS> constexpr bool is_window = std::is_same_v<ARGS, DecodeWindowArgs> || std::is_same_v<ARGS, DecodeFp8WindowArgs> || is_cap<ARGS>;

// (eight e4m3fn values as eight values of Q's type: cvt_fp8x8, fa_fwd_kernel.hpp)
}  // namespace decode

template <class ARGS, int DT, int NT, bool PAGED>
__global__ void __launch_bounds__(decode::THREADS) fa_decode_split_kernel(const ARGS args) {
    using E = Elem<DT>;
    using vec8 = typename E::vec8;
    using namespace decode;
    constexpr bool FP8 = is_fp8<ARGS>, WINDOW = is_window<ARGS>, CAP = is_cap<ARGS>;
    constexpr int KS = D / 32, DT16 = D / 16;
    constexpr int MERGE = NT * DT16 * 64 * 16;   // one wave's accumulators
    constexpr int MAIN = NWAVES * VBYTES > MERGE ? NWAVES * VBYTES : MERGE;
    __shared__ __attribute__((aligned(16))) char smem[MAIN + (NWAVES + 1) * NT * 16 * 4];
    const DecodeArgs &a = common(args);
    [[maybe_unused]] const uint8_t *const k8 = (const uint8_t *)a.k, *const v8 = (const uint8_t *)a.v;   // fp8: the cache's bytes
    // one 32-key unit in the prefetch registers: 16 bytes per lane and load
    using KRegs = std::conditional_t<FP8, u32x4[2][2], vec8[2][KS]>;
    using VRegs = std::conditional_t<FP8, u32x4[4], s16x8[8]>;

    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int li = lane & 15, g = lane >> 4;
    [[maybe_unused]] const int vr = lane >> 3, vc = lane & 7;   // fp8: V's load shape
    const int nsp = a.num_splits;
    const int split = blockIdx.x % nsp, kvh = (blockIdx.x / nsp) % a.n_kv_heads, b = blockIdx.x / (nsp * a.n_kv_heads);

    int len = a.cache_seqlens[b];
    len = len < 0 ? 0 : (len > a.max_len ? a.max_len : len);
    const int n_tiles = (len + TILE - 1) / TILE;
    [[maybe_unused]] int lo_min = 0;   // window: the lowest key a row of this workgroup sees (<= len - 1 when len > 0)
    int t0, t1;
    if constexpr (WINDOW) {
        // (the capped forms' window is a member of a member, written out beside the windowed forms' line here and below: one more
        // value or inlined call in front of it would renumber the blocks the windowed units' kept ISA names)
        if constexpr (CAP) {
            if (args.w.left >= 0) {
                const int64_t lo = (int64_t)len - a.seqlen_q - args.w.left;
                lo_min = lo > 0 ? (int)lo : 0;
            }
        } else if (args.left >= 0) {
            const int64_t lo = (int64_t)len - a.seqlen_q - args.left;
            lo_min = lo > 0 ? (int)lo : 0;
        }
        const int tl = lo_min / TILE, nt_w = n_tiles - tl;   // (len = 0: lo_min = 0, no tile)
        t0 = tl + (int)((int64_t)nt_w * split / nsp);
        t1 = tl + (int)((int64_t)nt_w * (split + 1) / nsp);
    } else {
        t0 = (int)((int64_t)n_tiles * split / nsp);
        t1 = (int)((int64_t)n_tiles * (split + 1) / nsp);
    }
    const int n_units = (len + UNIT - 1) / UNIT;
    const int u_end = 2 * t1 < n_units ? 2 * t1 : n_units;
    float kd = 1.0f, vd = 1.0f;
    if constexpr (FP8) {
        const DecodeFp8Args &f = fp8_part(args);
        kd = f.k_descale ? f.k_descale[(int64_t)b * f.ds_bs + kvh] : 1.0f;
        vd = f.v_descale ? f.v_descale[(int64_t)b * f.ds_bs + kvh] : 1.0f;
    }

    // Q^T, resident (fp8: in K's permutation of d); lim: the first key a row does not see.  Window: lim holds the row's position
    // p instead (one register per row tile, as before), and each unit derives the row's bounds p - w_left and
    // min(len, p + w_right + 1) from it -- neither needs its clamp at 0, keys are not negative
    vec8 Qr[NT][KS];
    int lim[NT];
    [[maybe_unused]] int w_left = 0, w_right = 0;
    if constexpr (WINDOW) {   // unbounded, or beyond what any length reaches (the host: len <= 2^30 - 128; p >= -seqlen_q >= -64): all one
        constexpr int FAR = (1 << 30) + 64;
        if constexpr (CAP) {
            w_left = args.w.left < 0 || args.w.left > FAR ? FAR : args.w.left;
            w_right = args.w.right < 0 || args.w.right > FAR ? FAR : args.w.right;
        } else {
            w_left = args.left < 0 || args.left > FAR ? FAR : args.left;
            w_right = args.right < 0 || args.right > FAR ? FAR : args.right;
        }
    }
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
        const int r = nt * 16 + li;
        const bool valid = r < a.rows;
        const int rr = valid ? r : 0, qi = rr / a.group, qh = kvh * a.group + rr % a.group;
        const uint16_t *qp = a.q + (int64_t)b * a.q_bs + (int64_t)qi * a.q_ss + (int64_t)qh * a.q_hs + g * (FP8 ? 16 : 8);
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) Qr[nt][ks] = *(const vec8 *)(qp + (FP8 ? (ks >> 1) * 64 + (ks & 1) * 8 : ks * 32));
        if constexpr (WINDOW) {
            lim[nt] = !valid ? -(1 << 30) - 66 : len - a.seqlen_q + qi;   // (a padded row: p + w_right + 1 < 0)
        } else {
            lim[nt] = !valid ? 0 : (a.causal ? len - a.seqlen_q + qi + 1 : len);
        }
    }

    float scale, c;   // logits (fp8: raw logits) -> logits, and -> the exponent of exp2
    // CAP: S -> A tanh(S / A) = cap_a + cap_m2a / (exp2(S cap_k) + 1); fp8: S is raw, so k_descale goes into cap_k, not into c
    [[maybe_unused]] float cap_a = 0.0f, cap_m2a = 0.0f, cap_k = 0.0f;
    if constexpr (CAP) {
        cap_a = args.cap_a;
        cap_m2a = -2.0f * args.cap_a;
        cap_k = kd * (args.cap_inv_a * 2.8853900817779268f);   // 2 log2(e) / A (16-bit: kd = 1)
    }
    if constexpr (FP8 && !CAP) {
        scale = kd / __builtin_sqrtf((float)D);
        c = scale * 1.4426950408889634074f;
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

    // one 32-key unit's K (16-bit: the A operands of S^T, key 16 kt + li, d 32 ks + 8 g ..) and V (16-bit: key 4 i + g,
    // d 8 li ..: whole rows per instruction; fp8: the shapes at the head of this file), 16 bytes per lane and load; keys at or
    // beyond len come from key len - 1.  A unit at or beyond u_end (the prefetch behind a wave's last unit) is still loaded,
    // every lane from the first row of unit `u_valid`: one cached row instead of 16 (fp8: 8) KiB, and the number of loads in
    // flight stays the same on every path, so the waits can be counted.  Window: a key below lo_min comes from key lo_min (the
    // wave's first unit may begin below it), and so does the prefetch behind the last unit when that is unit `u_valid`'s first row
    auto clamp_key = [](int ko, [[maybe_unused]] int first, int last) {
        if constexpr (WINDOW) ko = ko < first ? first : ko;
        return ko < last ? ko : last;
    };
    auto load_unit = [&](int u, int u_valid, KRegs &Kr, VRegs &Vr, auto want_k, auto want_v) {
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
        [[maybe_unused]] int first = 0;
        if constexpr (WINDOW) first = lo_min > key0 ? lo_min - key0 : 0;
        const int last = real ? len - 1 - key0 : first;
        if constexpr (FP8) {
#pragma unroll
            for (int kt = 0; kt < 2 && decltype(want_k)::value; ++kt) {
                const int ko = clamp_key(kt * 16 + li, first, last);
                const uint8_t *kp = k8 + base + (int64_t)(row0 + ko) * a.kv_ss + g * 16;
#pragma unroll
                for (int j = 0; j < 2; ++j) Kr[kt][j] = *(const u32x4 *)(kp + j * 64);
            }
#pragma unroll
            for (int i = 0; i < 4 && decltype(want_v)::value; ++i) {
                const int ko = clamp_key(i * 8 + vr, first, last);
                Vr[i] = *(const u32x4 *)(v8 + base + (int64_t)(row0 + ko) * a.kv_ss + vc * 16);
            }
        } else {
#pragma unroll
            for (int kt = 0; kt < 2 && decltype(want_k)::value; ++kt) {
                const int ko = clamp_key(kt * 16 + li, first, last);
                const uint16_t *kp = a.k + base + (int64_t)(row0 + ko) * a.kv_ss + g * 8;
#pragma unroll
                for (int ks = 0; ks < KS; ++ks) Kr[kt][ks] = *(const vec8 *)(kp + ks * 32);
            }
#pragma unroll
            for (int i = 0; i < 8 && decltype(want_v)::value; ++i) {
                const int ko = clamp_key(i * 4 + g, first, last);
                Vr[i] = *(const s16x8 *)(a.v + base + (int64_t)(row0 + ko) * a.kv_ss + li * 8);
            }
        }
    };

    char *vs = smem + wave * VBYTES;
    const char *vrd = vs + (4 * g + (li >> 2)) * VROW + (li & 3) * 8;   // T10: lane 4q + p of a group: row q, columns 4p ..
    auto compute_unit = [&](int u, const KRegs &Kr, const VRegs &Vr) {
        if constexpr (FP8) {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                char *wp = vs + (i * 8 + vr) * VROW + vc * 32;
                *(vec8 *)wp = cvt_fp8x8<DT>(Vr[i][0], Vr[i][1]);
                *(vec8 *)(wp + 16) = cvt_fp8x8<DT>(Vr[i][2], Vr[i][3]);
            }
        } else {
#pragma unroll
            for (int i = 0; i < 8; ++i) *(s16x8 *)(vs + (i * 4 + g) * VROW + li * 16) = Vr[i];
        }
        f32x4 S[NT][2];
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) S[nt][0] = S[nt][1] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
        for (int ks = 0; ks < KS; ++ks)
#pragma unroll
            for (int kt = 0; kt < 2; ++kt) {
                vec8 ka;
                if constexpr (FP8) ka = cvt_fp8x8<DT>(Kr[kt][ks >> 1][2 * (ks & 1)], Kr[kt][ks >> 1][2 * (ks & 1) + 1]);
                else ka = Kr[kt][ks];
#pragma unroll
                for (int nt = 0; nt < NT; ++nt) S[nt][kt] = E::mfma16(ka, Qr[nt][ks], S[nt][kt]);
            }
        vec8 Pb[NT];
        const int key_g = u * UNIT + 4 * g;
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
            float s[8];
            float mx = ninf;
            // window: lo <= key < hi as ONE unsigned compare, key - lo < span (two compares per element hold two lane masks each)
            [[maybe_unused]] unsigned from_lo = 0, span = 0;
            if constexpr (WINDOW) {
                const int hi = lim[nt] + w_right + 1 < len ? lim[nt] + w_right + 1 : len;
                const int lo = (int)((unsigned)lim[nt] - (unsigned)w_left);   // (a padded row may wrap: hi < 0 masks it)
                span = hi > lo ? (unsigned)hi - (unsigned)lo : 0u;
                from_lo = (unsigned)key_g - (unsigned)lo;
            }
#pragma unroll
            for (int j = 0; j < 8; ++j) {   // element j: key 16 (j >> 2) + 4 g + (j & 3) of the unit
                bool seen;
                if constexpr (WINDOW) seen = from_lo + (unsigned)(16 * (j >> 2) + (j & 3)) < span;
                else seen = key_g + 16 * (j >> 2) + (j & 3) < lim[nt];
                if constexpr (CAP) {
                    const float e = __builtin_amdgcn_exp2f(S[nt][j >> 2][j & 3] * cap_k);
                    const float capped = __builtin_fmaf(__builtin_amdgcn_rcpf(e + 1.0f), cap_m2a, cap_a);
                    s[j] = seen ? capped : ninf;
                } else {
                    s[j] = seen ? S[nt][j >> 2][j & 3] : ninf;
                }
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
            float p[8], rowsum = 0.0f;
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                p[j] = __builtin_amdgcn_exp2f(__builtin_fmaf(s[j], c, neg_mc));
                rowsum += p[j];
            }
            l[nt] += rowsum;
            Pb[nt] = E::pack8(p);
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // the wave's V image is written
#pragma unroll
        for (int t = 0; t < DT16; ++t) {
            s16x8 av;
            av.lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((FA_LDS(s16x4) *)(vrd + t * 32));
            av.hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((FA_LDS(s16x4) *)(vrd + t * 32 + 16 * VROW));
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) O[nt][t] = E::mfma16(__builtin_bit_cast(vec8, av), Pb[nt], O[nt][t]);
        }
        asm volatile("" ::: "memory");   // ... and read before the next unit's is written
    };

    // Two register sets, A and B, taken in turn (the loop is unrolled by two, so no set is ever copied into the other): a
    // unit's loads are issued before the previous unit's work and waited for with the next unit's loads still in flight.
    // 16-bit cache, 64 rows: Q^T and O^T take 192 registers, so only K is held a unit ahead; V is requested at the top of its
    // own unit and arrives under the S^T products and the softmax (with V a unit ahead as well that form spills).
    {
        constexpr bool V_AHEAD = FP8 || NT < 4;
        using Ahead = BoolTag<V_AHEAD>;
        using Late = BoolTag<!V_AHEAD>;
        KRegs Ka, Kb;
        VRegs Va, Vb;
        int u = 2 * t0 + wave;
        if constexpr (WINDOW) u = (2 * t0 > lo_min / UNIT ? 2 * t0 : lo_min / UNIT) + wave;   // (only the lowest tile's first unit can lie below)
        if (u < u_end) load_unit(u, u, Ka, Va, BoolTag<true>{}, Ahead{});
        while (u < u_end) {
            if constexpr (!V_AHEAD) load_unit(u, u, Ka, Va, BoolTag<false>{}, Late{});
            load_unit(u + NWAVES, u, Kb, Vb, BoolTag<true>{}, Ahead{});
            if constexpr (V_AHEAD) __builtin_amdgcn_sched_barrier(0);   // the requests go out before the unit's work, not where the scheduler finds room
            compute_unit(u, Ka, Va);
            u += NWAVES;
            if (u >= u_end) break;
            if constexpr (!V_AHEAD) load_unit(u, u, Kb, Vb, BoolTag<false>{}, Late{});
            load_unit(u + NWAVES, u, Ka, Va, BoolTag<true>{}, Ahead{});
            if constexpr (V_AHEAD) __builtin_amdgcn_sched_barrier(0);
            compute_unit(u, Kb, Vb);
            u += NWAVES;
        }
    }

    // (Window, whose 64-row fp8 form stands at the register file's end: what the lines below need of the lane's coordinates and of
    // the logits' scale is made again from what the loop keeps -- else the allocator holds r = 16 nt + li, the lane and the scale
    // in registers of their own across the loop, and spills them; likewise the reciprocal behind r / group.  The same values,
    // the same operations.)
    int li_e = li, g_e = g, group_e = a.group;
    [[maybe_unused]] float kd_e = kd;
    if constexpr (CAP) asm volatile("" : "+v"(li_e), "+v"(g_e), "+s"(group_e));   // (the cap's scale is a constant: no descale behind the loop)
    else if constexpr (WINDOW) asm volatile("" : "+v"(li_e), "+v"(g_e), "+s"(kd_e), "+s"(group_e));
    const int lane_e = WINDOW ? (g_e << 4 | li_e) : lane;
    const float scale_e = WINDOW && FP8 && !CAP ? kd_e / __builtin_sqrtf((float)D) : scale;

    // the four waves' states into wave 0: one reference per row for all of them, then plain sums in wave order
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) l[nt] = quad_sum(l[nt]);
    float *m_sh = (float *)(smem + MAIN), *l_sh = m_sh + NWAVES * NT * 16, *o_sh = (float *)smem;
    __syncthreads();   // every wave is done with its V image
    if (g_e == 0) {
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) m_sh[(wave * NT + nt) * 16 + li_e] = m[nt];
    }
    __syncthreads();
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
        float m_all = ninf;
#pragma unroll
        for (int w = 0; w < NWAVES; ++w) m_all = fmaxf(m_all, m_sh[(w * NT + nt) * 16 + li_e]);
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
                for (int t = 0; t < DT16; ++t) *(f32x4 *)(o_sh + ((nt * DT16 + t) * 64 + lane_e) * 4) = O[nt][t];
                if (g_e == 0) l_sh[nt * 16 + li_e] = l[nt];
            }
        }
        __syncthreads();
        if (wave == 0) {
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) {
#pragma unroll
                for (int t = 0; t < DT16; ++t) O[nt][t] += *(const f32x4 *)(o_sh + ((nt * DT16 + t) * 64 + lane_e) * 4);
                l[nt] += l_sh[nt * 16 + li_e];
            }
        }
        __syncthreads();
    }
    if (wave != 0) return;

    // lane (li, g) holds row 16 nt + li, d 16 t + 4 g .. + 3 (fp8: m is a raw logit, l a sum of undescaled V's weights)
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
        const int r = nt * 16 + li_e;
        if (r >= a.rows) continue;
        const bool any = l[nt] > 0.0f;
        const float inv = any ? vd / l[nt] : 0.0f;
        const float lse = any ? m[nt] * scale_e + __logf(l[nt]) : ninf;
        const int qi = r / group_e, qh = kvh * group_e + r % group_e;
        if (nsp == 1) {
            uint16_t *op = a.o + (int64_t)b * a.o_bs + (int64_t)qi * a.o_ss + (int64_t)qh * a.o_hs + 4 * g_e;
#pragma unroll
            for (int t = 0; t < DT16; ++t) {
                u32x2 w;
                w[0] = E::pack2(O[nt][t][0] * inv, O[nt][t][1] * inv);
                w[1] = E::pack2(O[nt][t][2] * inv, O[nt][t][3] * inv);
                *(u32x2 *)(op + 16 * t) = w;
            }
            if (a.lse && g_e == 0) a.lse[((int64_t)b * a.n_heads + qh) * a.seqlen_q + qi] = lse;
        } else {
            const int64_t row = (((int64_t)split * a.batch + b) * a.n_kv_heads + kvh) * a.rows + r;
            float *pp = a.part_o + row * D + 4 * g_e;
#pragma unroll
            for (int t = 0; t < DT16; ++t) *(f32x4 *)(pp + 16 * t) = O[nt][t] * inv;
            if (g_e == 0) a.part_lse[row] = lse;
        }
    }
}

// one workgroup of 64 threads per (batch, K / V head, row); thread i: d 2 i, 2 i + 1
template <int DT>
__global__ void __launch_bounds__(64) fa_decode_combine_kernel(const DecodeArgs a) {
    using E = Elem<DT>;
    const int64_t row = blockIdx.x, n_rows = (int64_t)a.batch * a.n_kv_heads * a.rows;
    const int r = (int)(row % a.rows), kvh = (int)((row / a.rows) % a.n_kv_heads), b = (int)(row / ((int64_t)a.rows * a.n_kv_heads));
    const int qi = r / a.group, qh = kvh * a.group + r % a.group;
    const float ninf = -__builtin_inff();
    float mx = ninf;
    for (int s = 0; s < a.num_splits; ++s) mx = fmaxf(mx, a.part_lse[s * n_rows + row]);
    float lse = ninf, o0 = 0.0f, o1 = 0.0f;
    if (mx != ninf) {
        float sum = 0.0f;
        for (int s = 0; s < a.num_splits; ++s) sum += __expf(a.part_lse[s * n_rows + row] - mx);
        lse = mx + __logf(sum);
        for (int s = 0; s < a.num_splits; ++s) {
            const float w = __expf(a.part_lse[s * n_rows + row] - lse);
            const float2 v = *(const float2 *)(a.part_o + (s * n_rows + row) * decode::D + 2 * threadIdx.x);
            o0 = __builtin_fmaf(w, v.x, o0);
            o1 = __builtin_fmaf(w, v.y, o1);
        }
    }
    uint16_t *op = a.o + (int64_t)b * a.o_bs + (int64_t)qi * a.o_ss + (int64_t)qh * a.o_hs;
    *(unsigned *)(op + 2 * threadIdx.x) = E::pack2(o0, o1);
    if (a.lse && threadIdx.x == 0) a.lse[((int64_t)b * a.n_heads + qh) * a.seqlen_q + qi] = lse;
}

// The enqueue of one decode in either form: the split kernel and, for num_splits > 1, the combine kernel (the partial format
// is the same, so the fp8 form launches it on its DecodeArgs part) on stream s.  Instantiated by fa_decode.hip (DecodeArgs),
// fa_decode_fp8.hip (DecodeFp8Args), fa_decode_window.hip (DecodeWindowArgs), fa_decode_fp8_window.hip (DecodeFp8WindowArgs),
// fa_decode_softcap.hip (DecodeSoftcapArgs) and fa_decode_fp8_softcap.hip (DecodeFp8SoftcapArgs), which hold the kernels.
template <class ARGS, int DT, int NT, bool PAGED>
static hipError_t decode_enqueue_t(const ARGS &args, hipStream_t s) {
    const DecodeArgs &a = decode::common(args);
    void *params[] = {(void *)&args}, *cparams[] = {(void *)&a};
    const hipError_t rc = hipLaunchKernel((const void *)&fa_decode_split_kernel<ARGS, DT, NT, PAGED>,
                                          dim3((unsigned)((int64_t)a.batch * a.n_kv_heads * a.num_splits)), dim3(decode::THREADS), params, 0, s);
    if (rc != hipSuccess || a.num_splits == 1) return rc;
    return hipLaunchKernel((const void *)&fa_decode_combine_kernel<DT>, dim3((unsigned)((int64_t)a.batch * a.n_kv_heads * a.rows)), dim3(64),
                           cparams, 0, s);
}

template <class ARGS>
static hipError_t decode_enqueue_any(const ARGS &args, int dtype, hipStream_t s) {
    const DecodeArgs &a = decode::common(args);
    const bool paged = a.block_table != nullptr, bf16 = dtype == 15;
    auto go = [&](auto nt) {
        constexpr int NT = decltype(nt)::value;
        if (bf16) return paged ? decode_enqueue_t<ARGS, 15, NT, true>(args, s) : decode_enqueue_t<ARGS, 15, NT, false>(args, s);
        return paged ? decode_enqueue_t<ARGS, 5, NT, true>(args, s) : decode_enqueue_t<ARGS, 5, NT, false>(args, s);
    };
    switch (decode::row_tiles(a.rows)) {
    case 1: return go(IntTag<1>{});
    case 2: return go(IntTag<2>{});
    default: return go(IntTag<4>{});
    }
}

hipError_t decode_enqueue(const DecodeArgs &a, int dtype, hipStream_t s);          // fa_decode.hip
hipError_t decode_fp8_enqueue(const DecodeFp8Args &a, int dtype, hipStream_t s);   // fa_decode_fp8.hip
hipError_t decode_window_enqueue(const DecodeWindowArgs &a, int dtype, hipStream_t s);          // fa_decode_window.hip
hipError_t decode_fp8_window_enqueue(const DecodeFp8WindowArgs &a, int dtype, hipStream_t s);   // fa_decode_fp8_window.hip
hipError_t decode_softcap_enqueue(const DecodeSoftcapArgs &a, int dtype, hipStream_t s);          // fa_decode_softcap.hip
hipError_t decode_fp8_softcap_enqueue(const DecodeFp8SoftcapArgs &a, int dtype, hipStream_t s);   // fa_decode_fp8_softcap.hip

}  // namespace fa
