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
#pragma once
#include "fa_decode_kernel.hpp"

namespace fa {

struct Decode64Args {
    DecodeArgs d;           // part_o: (num_splits, batch, n_kv_heads, rows, 64)
    int32_t left, right;    // -1 = unbounded (causal: right = 0)
    const float *sinks;     // (n_heads) fp32, DEVICE, or null
};

namespace decode64 {
constexpr int D = 64, TILE = 64, NWAVES = 4, THREADS = NWAVES * 64;
constexpr int VROW = 160;              // bytes per key of the V image (the argument is at the head of this file)
constexpr int UNIT_SHIPPED = 32;       // keys per wave visit: 32 or 64, measured side by side
}  // namespace decode64

template <int DT, int NT, bool PAGED, int UNIT>
__global__ void __launch_bounds__(decode64::THREADS) fa_decode64_split_kernel(const Decode64Args args) {
    using E = Elem<DT>;
    using vec8 = typename E::vec8;
    using namespace decode64;
    static_assert(UNIT == 64 || UNIT == 32, "a unit is a whole 64-key tile or half of one");
    constexpr int KS = D / 32, DT16 = D / 16, KT = UNIT / 16, VL = UNIT / 8, UPT = TILE / UNIT;   // (VL: V loads, UPT: units per tile)
    constexpr int VBYTES = UNIT * VROW;   // one wave's image
    constexpr int MERGE = NT * DT16 * 64 * 16;   // one wave's accumulators
    constexpr int MAIN = NWAVES * VBYTES > MERGE ? NWAVES * VBYTES : MERGE;
    __shared__ __attribute__((aligned(16))) char smem[MAIN + (NWAVES + 1) * NT * 16 * 4];
    const DecodeArgs &a = args.d;
    struct KRegs { vec8 r[KT][KS]; };   // one 64-key unit in the prefetch registers: 16 bytes per lane and load
    struct VRegs { s16x8 r[VL]; };

    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int li = lane & 15, g = lane >> 4;
    const int vc = lane & 7, vk = (lane >> 4) + 4 * ((lane >> 3) & 1);   // V's load shape: key 8 i + vk, d 8 vc ..
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

    // Q^T, resident; pos: the row's position p = len - seqlen_q + query position, from which each unit derives the row's bounds
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
        const uint16_t *qp = a.q + (int64_t)b * a.q_bs + (int64_t)qi * a.q_ss + (int64_t)qh * a.q_hs + g * 8;
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) Qr[nt][ks] = *(const vec8 *)(qp + ks * 32);
        pos[nt] = !valid ? -(1 << 30) - 66 : len - a.seqlen_q + qi;   // (a padded row: p + w_right + 1 < 0)
    }

    const float scale = 1.0f / __builtin_sqrtf((float)D);
    const float c = (float)((double)scale * 1.4426950408889634074);
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
#pragma unroll
        for (int kt = 0; kt < KT; ++kt) {
            const uint16_t *kp = a.k + base + (int64_t)(row0 + clamp_key(kt * 16 + li)) * a.kv_ss + g * 8;
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) Kr.r[kt][ks] = *(const vec8 *)(kp + ks * 32);
        }
#pragma unroll
        for (int i = 0; i < VL; ++i) Vr.r[i] = *(const s16x8 *)(a.v + base + (int64_t)(row0 + clamp_key(i * 8 + vk)) * a.kv_ss + vc * 8);
    };

    char *vs = smem + wave * VBYTES;
    char *vwr = vs + vk * VROW + vc * 16;
    const char *vrd = vs + (4 * g + (li >> 2)) * VROW + (li & 3) * 8;   // lane 4 q + p of a group: row q, columns 4 p ..
    auto compute_unit = [&](int u, const KRegs &Kr, const VRegs &Vr) {
#pragma unroll
        for (int i = 0; i < VL; ++i) *(s16x8 *)(vwr + i * 8 * VROW) = Vr.r[i];
        f32x4 S[NT][KT];
#pragma unroll
        for (int nt = 0; nt < NT; ++nt)
#pragma unroll
            for (int kt = 0; kt < KT; ++kt) S[nt][kt] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
        for (int kt = 0; kt < KT; ++kt)
#pragma unroll
            for (int ks = 0; ks < KS; ++ks)
#pragma unroll
                for (int nt = 0; nt < NT; ++nt) S[nt][kt] = E::mfma16(Kr.r[kt][ks], Qr[nt][ks], S[nt][kt]);
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
    {
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
            const float inv = any ? al / l_all : 0.0f;
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
            const float inv = any ? 1.0f / l[nt] : 0.0f;
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

hipError_t decode64_enqueue(const Decode64Args &a, int dtype, hipStream_t s);   // fa_decode64.hip

}  // namespace fa
