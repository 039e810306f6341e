// fa_bwd_gqa.hpp -- the backward for grouped-query attention (fa_bwd_launch_gqa): query head h reads K / V head h / group.
//
// The kernels of fa_bwd_kernel.hpp with their K / V addressing widened; the tile arithmetic (S, dP, dS, the five MFMA
// products, the operand orientation and the LDS images) is theirs, line for line.  Their own text, so that the MHA kernels
// keep theirs and their code.
//   delta               fa_bwd_delta_kernel itself (per query head)
//   fa_bwd_dq_gqa_kernel    fa_bwd_dq_kernel with the K / V tiles of head h / group: the same dQ bits as the MHA backward on K / V
//                           expanded with repeat_interleave
//   fa_bwd_dkdv_gqa_kernel  one workgroup per (batch * K / V head, split part, 128-key block).  The wave keeps dK^T / dV^T of its
//                           32 keys in fp32 accumulators while the workgroup sweeps the Q / dO tiles of group / split query heads
//                           of the group, one head after the other (causal: each from the diagonal on)
//   fa_bwd_dkdv_reduce_kernel  split > 1 only: the sum of a row's split partials, in order, scaled and rounded once
// No float atomics and no waiting between workgroups: the same inputs give the same bits.  split is a function of the shape
// alone (fa_capi.hip, bwd_gqa_split): the same shape takes the same path on every device.
#pragma once
#include "fa_bwd_kernel.hpp"

namespace fa {

struct BwdGqaArgs {
    BwdArgs base;                     // Q, O, dO, dQ, lse, delta: n_heads heads (qkv_* = Q's strides); k, v, dk, dv: see below
    int64_t kv_bs, kv_ss, kv_hs;      // K, V: n_heads / group heads (elements)
    int64_t dkv_bs, dkv_ss, dkv_hs;   // dK, dV
    float *part;                      // split > 1: (batch * n_kv_heads * split, seq_len, 2, 128) fp32 dK^T | dV^T, unscaled
    int32_t group, split;             // query heads per K / V head; workgroups per (K / V head, key block), divides group
};

// dK, dV of one 128-key block of one K / V head, summed over group / split query heads.
// Grid: batch * n_kv_heads * split * seq_len / 128 workgroups of 256 threads.
template <int DT, bool CAUSAL>
__global__ void __launch_bounds__(bwd::THREADS, 1) fa_bwd_dkdv_gqa_kernel(const BwdGqaArgs g) {
    using namespace bwd;
    using E = Elem<DT>;
    using vec8 = typename E::vec8;
    const BwdArgs &a = g.base;
    __shared__ __attribute__((aligned(16))) char img_q[TBYTES];
    __shared__ __attribute__((aligned(16))) char img_do[TBYTES];
    __shared__ __attribute__((aligned(16))) float lse_s[TROWS];   // -lse sqrt(d) of the tile's rows
    __shared__ __attribute__((aligned(16))) float dl_s[TROWS];    // -delta
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 31, h = lane >> 5;
    int wg, kb;   // wg = (batch * n_kv_heads + K / V head) * split + part
    block_coords(a.seq_len / KB, wg, kb);
    const int n_kv = a.n_heads / g.group, bkv = wg / g.split, b = bkv / n_kv, hk = bkv % n_kv;
    const int n_hq = g.group / g.split;   // query heads of the sweep: hk * group + part * n_hq + 0 .. n_hq - 1
    int bh = b * a.n_heads + hk * g.group + (wg % g.split) * n_hq;
    const int64_t kv_head = (int64_t)b * g.kv_bs + (int64_t)hk * g.kv_hs;
    int64_t qkv_head = (int64_t)(bh / a.n_heads) * a.qkv_bs + (int64_t)(bh % a.n_heads) * a.qkv_hs;
    int64_t out_head = (int64_t)(bh / a.n_heads) * a.out_bs + (int64_t)(bh % a.n_heads) * a.out_hs;
    const int key = kb * KB + 32 * wave + r;   // this lane's key (the accumulators' column)
    // K, V of the wave's 32 keys: the B operands of S = Q K^T and dP = dO V^T, resident for the whole sweep
    vec8 Kb[8], Vb[8];
    {
        const uint16_t *kr = a.k + kv_head + (int64_t)key * g.kv_ss + 8 * h;
        const uint16_t *vr = a.v + kv_head + (int64_t)key * g.kv_ss + 8 * h;
#pragma unroll
        for (int ks = 0; ks < 8; ++ks) {
            Kb[ks] = *(const vec8 *)(kr + 16 * ks);
            Vb[ks] = *(const vec8 *)(vr + 16 * ks);
        }
    }
    const float c = (float)((double)(1.0f / __builtin_sqrtf((float)D)) * 1.4426950408889634074);
    const float lse_scale = -log2e_over_c();
    f32x16 dV[4], dK[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        dV[t] = f32x16{};
        dK[t] = f32x16{};
    }
    const int n_it = a.seq_len / TROWS;
    const int it0 = CAUSAL ? kb * (KB / TROWS) : 0;   // causal: the Q tiles from the diagonal on
    const float *lse_bh = a.lse + (int64_t)bh * a.seq_len;
    const float *dl_bh = a.delta + (int64_t)bh * a.seq_len;
    TileRegs tq, tdo;
    float lse_r = 0.0f, dl_r = 0.0f;
    auto load = [&](int it) {
        tile_load(tq, a.q + qkv_head + (int64_t)it * TROWS * a.qkv_ss, a.qkv_ss, tid);
        tile_load(tdo, a.dout + out_head + (int64_t)it * TROWS * a.out_ss, a.out_ss, tid);
        if (tid < TROWS) {
            lse_r = lse_bh[it * TROWS + tid] * lse_scale;
            dl_r = -dl_bh[it * TROWS + tid];
        }
    };
    load(it0);
    for (int j = 0; j < n_hq; ++j) {
        for (int it = it0; it < n_it; ++it) {
            __syncthreads();   // every wave is done with the previous tile's images
            tile_store(img_q, tq, tid);
            tile_store(img_do, tdo, tid);
            if (tid < TROWS) {
                lse_s[tid] = lse_r;
                dl_s[tid] = dl_r;
            }
            __syncthreads();
            if (it + 1 < n_it) {
                load(it + 1);   // in flight under this tile's MFMAs
            } else if (j + 1 < n_hq) {   // ... or the next query head's first tile
                ++bh;
                qkv_head = (int64_t)(bh / a.n_heads) * a.qkv_bs + (int64_t)(bh % a.n_heads) * a.qkv_hs;
                out_head = (int64_t)(bh / a.n_heads) * a.out_bs + (int64_t)(bh % a.n_heads) * a.out_hs;
                lse_bh += a.seq_len;
                dl_bh += a.seq_len;
                load(it0);
            }
            const bool diag = CAUSAL && it * TROWS < kb * KB + KB;   // a tile that holds queries before some key of the block
#pragma unroll
            for (int mt = 0; mt < TROWS / 32; ++mt) {
                const int rb = 32 * mt;
                f32x16 S, dP;
                // rows of registers 4g .. 4g + 3: rb + 8 g + 4 h + 0 .. 3
#pragma unroll
                for (int gg = 0; gg < 4; ++gg) {
                    const f32x4 l4 = *(const f32x4 *)(lse_s + rb + 8 * gg + 4 * h);
                    const f32x4 d4 = *(const f32x4 *)(dl_s + rb + 8 * gg + 4 * h);
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        S[4 * gg + e] = l4[e];
                        dP[4 * gg + e] = d4[e];
                    }
                }
#pragma unroll
                for (int ks = 0; ks < 8; ++ks) S = E::mfma(row_read<vec8>(img_q, rb, ks, lane), Kb[ks], S);
#pragma unroll
                for (int ks = 0; ks < 8; ++ks) dP = E::mfma(row_read<vec8>(img_do, rb, ks, lane), Vb[ks], dP);
#pragma unroll
                for (int i = 0; i < 16; ++i) {
                    float p = __builtin_amdgcn_exp2f(c * S[i]);
                    if (diag) {
                        const int query = it * TROWS + rb + (i & 3) + 8 * (i >> 2) + 4 * h;
                        p = key > query ? 0.0f : p;
                    }
                    S[i] = p;                 // P
                    dP[i] = p * dP[i];        // dS = P (dP - delta)
                }
#pragma unroll
                for (int s = 0; s < 2; ++s) {
                    const vec8 pb = acc_operand<DT>(S, s), db = acc_operand<DT>(dP, s);
#pragma unroll
                    for (int t = 0; t < 4; ++t) {
                        dV[t] = E::mfma(tr_read<vec8>(img_do, rb, s, t, lane), pb, dV[t]);
                        dK[t] = E::mfma(tr_read<vec8>(img_q, rb, s, t, lane), db, dK[t]);
                    }
                }
            }
        }
    }
    // dK^T / dV^T: column = this lane's key, rows d = 32 t + 8 gg + 4 h + 0 .. 3
    if (g.split > 1) {   // the fp32 partials, unscaled: fa_bwd_dkdv_reduce_kernel rounds their sum
        float *pk = g.part + ((int64_t)wg * a.seq_len + key) * (2 * D) + 4 * h;
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
            for (int gg = 0; gg < 4; ++gg) {
                *(f32x4 *)(pk + 32 * t + 8 * gg) = f32x4{dK[t][4 * gg], dK[t][4 * gg + 1], dK[t][4 * gg + 2], dK[t][4 * gg + 3]};
                *(f32x4 *)(pk + D + 32 * t + 8 * gg) = f32x4{dV[t][4 * gg], dV[t][4 * gg + 1], dV[t][4 * gg + 2], dV[t][4 * gg + 3]};
            }
        return;
    }
    const float inv_sqrt_d = 1.0f / __builtin_sqrtf((float)D);
    const int64_t dkv_row = (int64_t)b * g.dkv_bs + (int64_t)hk * g.dkv_hs + (int64_t)key * g.dkv_ss + 4 * h;
    uint16_t *dk = a.dk + dkv_row;
    uint16_t *dv = a.dv + dkv_row;
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int gg = 0; gg < 4; ++gg) {
            store4<DT>(dk + 32 * t + 8 * gg, dK[t], gg, inv_sqrt_d);
            store4<DT>(dv + 32 * t + 8 * gg, dV[t], gg, 1.0f);
        }
}

// split > 1: dK, dV of one (batch * K / V head, key) row = the sum of its `split` partials in order, scaled and rounded once.
// One thread per 8 elements of a dK or dV row.  Grid: batch * n_kv_heads * seq_len * 2 * 16 / 256 workgroups of 256 threads.
template <int DT>
__global__ void __launch_bounds__(256) fa_bwd_dkdv_reduce_kernel(const BwdGqaArgs g) {
    using namespace bwd;
    const BwdArgs &a = g.base;
    const int n_kv = a.n_heads / g.group;
    const int64_t n = (int64_t)(a.n_bh / g.group) * a.seq_len * 2 * (D / 8);
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= n) return;
    const int c8 = (int)(idx % (D / 8)), which = (int)((idx / (D / 8)) & 1);   // 8-element chunk; 0 dK, 1 dV
    const int64_t row = idx / (2 * (D / 8));   // bkv * seq_len + key
    const int64_t bkv = row / a.seq_len, key = row % a.seq_len;
    const int64_t plane = (int64_t)a.seq_len * 2 * D;   // floats per partial
    const float *src = g.part + (bkv * g.split * a.seq_len + key) * (2 * D) + which * D + 8 * c8;
    f32x4 lo = *(const f32x4 *)src, hi = *(const f32x4 *)(src + 4);
    for (int s = 1; s < g.split; ++s) {
        lo += *(const f32x4 *)(src + s * plane);
        hi += *(const f32x4 *)(src + s * plane + 4);
    }
    const float scale = which ? 1.0f : 1.0f / __builtin_sqrtf((float)D);
    float f[8];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        f[e] = lo[e] * scale;
        f[4 + e] = hi[e] * scale;
    }
    uint16_t *dst = (which ? a.dv : a.dk) + (bkv / n_kv) * g.dkv_bs + (bkv % n_kv) * g.dkv_hs + key * g.dkv_ss + 8 * c8;
    *(typename Elem<DT>::vec8 *)dst = Elem<DT>::pack8(f);
}

// dQ of one 128-row Q block, K / V of head h / group.  Grid: n_bh * seq_len / 128 workgroups of 256 threads.
template <int DT, bool CAUSAL>
__global__ void __launch_bounds__(bwd::THREADS, 1) fa_bwd_dq_gqa_kernel(const BwdGqaArgs g) {
    using namespace bwd;
    using E = Elem<DT>;
    using vec8 = typename E::vec8;
    const BwdArgs &a = g.base;
    __shared__ __attribute__((aligned(16))) char img_k[TBYTES];
    __shared__ __attribute__((aligned(16))) char img_v[TBYTES];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 31, h = lane >> 5;
    const int nqb = a.seq_len / KB;
    int bh, qb;
    block_coords(nqb, bh, qb);
    if (CAUSAL) qb = nqb - 1 - qb;   // the longest sweeps first
    const int64_t qkv_head = (int64_t)(bh / a.n_heads) * a.qkv_bs + (int64_t)(bh % a.n_heads) * a.qkv_hs;
    const int64_t out_head = (int64_t)(bh / a.n_heads) * a.out_bs + (int64_t)(bh % a.n_heads) * a.out_hs;
    const int64_t kv_head = (int64_t)(bh / a.n_heads) * g.kv_bs + (int64_t)((bh % a.n_heads) / g.group) * g.kv_hs;
    const int query = qb * KB + 32 * wave + r;   // this lane's query (the accumulators' column)
    // Q, dO of the wave's 32 rows: the B operands of S^T = K Q^T and dP^T = V dO^T
    vec8 Qb[8], Ob[8];
    {
        const uint16_t *qr = a.q + qkv_head + (int64_t)query * a.qkv_ss + 8 * h;
        const uint16_t *gr = a.dout + out_head + (int64_t)query * a.out_ss + 8 * h;
#pragma unroll
        for (int ks = 0; ks < 8; ++ks) {
            Qb[ks] = *(const vec8 *)(qr + 16 * ks);
            Ob[ks] = *(const vec8 *)(gr + 16 * ks);
        }
    }
    const float c = (float)((double)(1.0f / __builtin_sqrtf((float)D)) * 1.4426950408889634074);
    const float lse_q = a.lse[(int64_t)bh * a.seq_len + query] * -log2e_over_c();
    const float dl_q = -a.delta[(int64_t)bh * a.seq_len + query];
    f32x16 dQ[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) dQ[t] = f32x16{};
    const int n_kt = CAUSAL ? (qb + 1) * (KB / TROWS) : a.seq_len / TROWS;
    TileRegs tk, tv;
    auto load = [&](int kt) {
        tile_load(tk, a.k + kv_head + (int64_t)kt * TROWS * g.kv_ss, g.kv_ss, tid);
        tile_load(tv, a.v + kv_head + (int64_t)kt * TROWS * g.kv_ss, g.kv_ss, tid);
    };
    load(0);
    for (int kt = 0; kt < n_kt; ++kt) {
        __syncthreads();
        tile_store(img_k, tk, tid);
        tile_store(img_v, tv, tid);
        __syncthreads();
        if (kt + 1 < n_kt) load(kt + 1);
        const bool diag = CAUSAL && kt * TROWS + TROWS > qb * KB;   // a tile that holds keys after some query of the block
#pragma unroll
        for (int mt = 0; mt < TROWS / 32; ++mt) {
            const int rb = 32 * mt;
            f32x16 S, dP;
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                S[i] = lse_q;
                dP[i] = dl_q;
            }
#pragma unroll
            for (int ks = 0; ks < 8; ++ks) S = E::mfma(row_read<vec8>(img_k, rb, ks, lane), Qb[ks], S);
#pragma unroll
            for (int ks = 0; ks < 8; ++ks) dP = E::mfma(row_read<vec8>(img_v, rb, ks, lane), Ob[ks], dP);
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                float p = __builtin_amdgcn_exp2f(c * S[i]);
                if (diag) {
                    const int key = kt * TROWS + rb + (i & 3) + 8 * (i >> 2) + 4 * h;
                    p = key > query ? 0.0f : p;
                }
                dP[i] = p * dP[i];        // dS^T
            }
#pragma unroll
            for (int s = 0; s < 2; ++s) {
                const vec8 db = acc_operand<DT>(dP, s);
#pragma unroll
                for (int t = 0; t < 4; ++t) dQ[t] = E::mfma(tr_read<vec8>(img_k, rb, s, t, lane), db, dQ[t]);
            }
        }
    }
    const float inv_sqrt_d = 1.0f / __builtin_sqrtf((float)D);
    uint16_t *dq = a.dq + out_head + (int64_t)query * a.out_ss + 4 * h;
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int gg = 0; gg < 4; ++gg) store4<DT>(dq + 32 * t + 8 * gg, dQ[t], gg, inv_sqrt_d);
}

}  // namespace fa
