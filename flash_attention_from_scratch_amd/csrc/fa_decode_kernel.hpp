// fa_decode_kernel.hpp -- KV-cache decode attention for gfx950: a few query rows per sequence against a long K / V cache of
// a per-sequence length the DEVICE holds.  HBM-bound: K and V are read once, ~2 * rows FLOP per byte.
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
#pragma once
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

namespace decode {
constexpr int D = 128, UNIT = 32, TILE = 64, NWAVES = 4, THREADS = NWAVES * 64;
constexpr int VROW = 288;              // bytes per key of the V image: 256 + 32, so the 8 keys a 32-lane half's transposed read
                                       // covers (32 bytes of each) fall on all 64 banks
constexpr int VBYTES = UNIT * VROW;    // one wave's image
constexpr int row_tiles(int rows) { return rows <= 16 ? 1 : rows <= 32 ? 2 : 4; }
}  // namespace decode

template <int DT, int NT, bool PAGED>
__global__ void __launch_bounds__(decode::THREADS) fa_decode_split_kernel(const DecodeArgs a) {
    using E = Elem<DT>;
    using vec8 = typename E::vec8;
    using namespace decode;
    constexpr int KS = D / 32, DT16 = D / 16;
    constexpr int MERGE = NT * DT16 * 64 * 16;   // one wave's accumulators
    constexpr int MAIN = NWAVES * VBYTES > MERGE ? NWAVES * VBYTES : MERGE;
    __shared__ __attribute__((aligned(16))) char smem[MAIN + (NWAVES + 1) * NT * 16 * 4];

    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int li = lane & 15, g = lane >> 4;
    const int nsp = a.num_splits;
    const int split = blockIdx.x % nsp, kvh = (blockIdx.x / nsp) % a.n_kv_heads, b = blockIdx.x / (nsp * a.n_kv_heads);

    int len = a.cache_seqlens[b];
    len = len < 0 ? 0 : (len > a.max_len ? a.max_len : len);
    const int n_tiles = (len + TILE - 1) / TILE;
    const int t0 = (int)((int64_t)n_tiles * split / nsp), t1 = (int)((int64_t)n_tiles * (split + 1) / nsp);
    const int n_units = (len + UNIT - 1) / UNIT;
    const int u_end = 2 * t1 < n_units ? 2 * t1 : n_units;

    // Q^T, resident; lim: the first key a row does not see
    vec8 Qr[NT][KS];
    int lim[NT];
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
        const int r = nt * 16 + li;
        const bool valid = r < a.rows;
        const int rr = valid ? r : 0, qi = rr / a.group, qh = kvh * a.group + rr % a.group;
        const uint16_t *qp = a.q + (int64_t)b * a.q_bs + (int64_t)qi * a.q_ss + (int64_t)qh * a.q_hs + g * 8;
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) Qr[nt][ks] = *(const vec8 *)(qp + ks * 32);
        lim[nt] = !valid ? 0 : (a.causal ? len - a.seqlen_q + qi + 1 : len);
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

    // one 32-key unit's K (the A operands of S^T: key 16 kt + li, d 32 ks + 8 g ..) and V (key 4 i + g, d 8 li ..: whole rows
    // per instruction), 16 bytes per lane and load; keys at or beyond len come from key len - 1.  A unit at or beyond u_end
    // (the prefetch behind a wave's last unit) is still loaded, every lane from the first row of unit `u_valid`: one cached
    // row instead of 16 KiB, and the number of loads in flight stays the same on every path, so the waits can be counted
    auto load_unit = [&](int u, int u_valid, vec8 (&Kr)[2][KS], s16x8 (&Vr)[8], auto want_k, auto want_v) {
        const bool real = u < u_end;
        const int key0 = (real ? u : u_valid) * UNIT;
        int64_t base;
        int row0;
        if constexpr (PAGED) {
            const int page = key0 / a.page_size;
            // a scalar load (the compiler's own would be a vector load behind the unit's 16: waiting for it would drain them all)
            int p;
            asm volatile("s_load_dword %0, %1, 0x0\n\ts_waitcnt lgkmcnt(0)" : "=s"(p) : "s"(a.block_table + (int64_t)b * a.bt_bs + page) : "memory");
            p = p < 0 ? 0 : (p >= a.num_pages ? a.num_pages - 1 : p);
            base = (int64_t)p * a.kv_bs + (int64_t)kvh * a.kv_hs;
            row0 = key0 - page * a.page_size;
        } else {
            base = (int64_t)b * a.kv_bs + (int64_t)kvh * a.kv_hs;
            row0 = key0;
        }
        const int last = real ? len - 1 - key0 : 0;
#pragma unroll
        for (int kt = 0; kt < 2 && decltype(want_k)::value; ++kt) {
            const int ko = kt * 16 + li < last ? kt * 16 + li : last;
            const uint16_t *kp = a.k + base + (int64_t)(row0 + ko) * a.kv_ss + g * 8;
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) Kr[kt][ks] = *(const vec8 *)(kp + ks * 32);
        }
#pragma unroll
        for (int i = 0; i < 8 && decltype(want_v)::value; ++i) {
            const int ko = i * 4 + g < last ? i * 4 + g : last;
            Vr[i] = *(const s16x8 *)(a.v + base + (int64_t)(row0 + ko) * a.kv_ss + li * 8);
        }
    };

    char *vs = smem + wave * VBYTES;
    const char *vrd = vs + (4 * g + (li >> 2)) * VROW + (li & 3) * 8;   // T10: lane 4q + p of a group: row q, columns 4p ..
    auto compute_unit = [&](int u, const vec8 (&Kr)[2][KS], const s16x8 (&Vr)[8]) {
#pragma unroll
        for (int i = 0; i < 8; ++i) *(s16x8 *)(vs + (i * 4 + g) * VROW + li * 16) = Vr[i];
        f32x4 S[NT][2];
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) S[nt][0] = S[nt][1] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
        for (int ks = 0; ks < KS; ++ks)
#pragma unroll
            for (int kt = 0; kt < 2; ++kt)
#pragma unroll
                for (int nt = 0; nt < NT; ++nt) S[nt][kt] = E::mfma16(Kr[kt][ks], Qr[nt][ks], S[nt][kt]);
        vec8 Pb[NT];
        const int key_g = u * UNIT + 4 * g;
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
            float s[8];
            float mx = ninf;
#pragma unroll
            for (int j = 0; j < 8; ++j) {   // element j: key 16 (j >> 2) + 4 g + (j & 3) of the unit
                s[j] = key_g + 16 * (j >> 2) + (j & 3) < lim[nt] ? S[nt][j >> 2][j & 3] : ninf;
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
    // 64 rows: Q^T and O^T take 192 registers, so only K is held a unit ahead; V is requested at the top of its own unit
    // and arrives under the S^T products and the softmax (with V a unit ahead as well that form spills).
    {
        constexpr bool V_AHEAD = NT < 4;
        using Ahead = BoolTag<V_AHEAD>;
        using Late = BoolTag<!V_AHEAD>;
        vec8 Ka[2][KS], Kb[2][KS];
        s16x8 Va[8], Vb[8];
        int u = 2 * t0 + wave;
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
        const float inv = any ? 1.0f / l[nt] : 0.0f;
        const float lse = any ? m[nt] * scale + __logf(l[nt]) : ninf;
        const int qi = r / a.group, qh = kvh * a.group + r % a.group;
        if (nsp == 1) {
            uint16_t *op = a.o + (int64_t)b * a.o_bs + (int64_t)qi * a.o_ss + (int64_t)qh * a.o_hs + 4 * g;
#pragma unroll
            for (int t = 0; t < DT16; ++t) {
                u32x2 w;
                w[0] = E::pack2(O[nt][t][0] * inv, O[nt][t][1] * inv);
                w[1] = E::pack2(O[nt][t][2] * inv, O[nt][t][3] * inv);
                *(u32x2 *)(op + 16 * t) = w;
            }
            if (a.lse && g == 0) a.lse[((int64_t)b * a.n_heads + qh) * a.seqlen_q + qi] = lse;
        } else {
            const int64_t row = (((int64_t)split * a.batch + b) * a.n_kv_heads + kvh) * a.rows + r;
            float *pp = a.part_o + row * D + 4 * g;
#pragma unroll
            for (int t = 0; t < DT16; ++t) *(f32x4 *)(pp + 16 * t) = O[nt][t] * inv;
            if (g == 0) a.part_lse[row] = lse;
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

// the split kernel and, for num_splits > 1, the combine kernel on stream s (fa_decode.hip)
hipError_t decode_enqueue(const DecodeArgs &a, int dtype, hipStream_t s);

}  // namespace fa
