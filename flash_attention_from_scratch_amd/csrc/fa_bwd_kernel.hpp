// fa_bwd_kernel.hpp -- the attention backward (dQ, dK, dV) for d_head 128, gfx950, compiler-scheduled.
//
// Recompute P from Q, K and the forward's row log-sum-exp (lse[b, h, i] = ln sum_j exp(q_i . k_j / sqrt d), fp32), never
// storing the N x N scores.  With c = log2(e) / sqrt(d):
//   delta_i = sum_d dO_id O_id               (fa_bwd_delta_kernel: a preprocess pass into the fp32 workspace)
//   p       = exp2(c s - lse log2 e)
//   dV     += P^T dO          dP = dO V^T          dS = P o (dP - delta)
//   dK     += dS^T Q / sqrt d                      dQ += dS K / sqrt d
// P and dS are rounded to the input dtype as MFMA operands; everything accumulates in fp32.
//
// Two main kernels, no float atomics and no waiting between workgroups, so the same inputs give the same bits:
//   fa_bwd_dkdv_kernel  one workgroup per (batch*head, 128-key block); wave w owns keys 32w .. 32w+31 of the block and keeps
//                       dK^T and dV^T of them in accumulator registers while the workgroup sweeps the 64-row Q / dO tiles
//                       (causal: from the diagonal on).  Five products per tile pair: S, dP, dV^T, dK^T (+ none for dQ).
//   fa_bwd_dq_kernel    one workgroup per (batch*head, 128-row Q block); wave w owns rows 32w .. 32w+31 and keeps dQ^T in
//                       accumulators while the workgroup sweeps the 64-key K / V tiles (causal: up to the diagonal).
//                       Three products: S^T, dP^T, dQ^T.
// Seven MFMA products per tile pair instead of five; dQ needs no cross-workgroup sum.
//
// Orientation (cdna_hip_programming.md 3, "an accumulator tile as the next MFMA's operand"): an mfma_f32_32x32x16 result
// has its column on the lane and its rows in the 16 registers, so a following product that sums over its ROW index takes
// it as the B operand with no lane movement.  dK / dV kernel: S and dP with the KEY on the lane (rows = queries), then
// dV^T = dO^T P and dK^T = Q^T dS sum over the queries.  dQ kernel: S^T and dP^T with the QUERY on the lane, then
// dQ^T = K^T dS^T sums over the keys.  The row constants ride in the accumulators' initial value: S starts at
// -lse sqrt(d) (so c S' = c s - lse log2 e) and dP at -delta.
//
// LDS: every tile (Q, dO or K, V; 64 rows x 128 halves) has ONE image with 256-B rows and the chunk XOR of
// cdna_hip_programming.md T10 (b), read by rows (ds_read_b128: the A operand of S / dP) and by columns
// (ds_read_b64_tr_b16: the A operand of the transposed products).  Tiles travel global -> registers -> LDS, the next one
// in flight under the current one's MFMAs.
#pragma once
#include "fa_fwd_kernel.hpp"

namespace fa {

struct BwdArgs {
    const uint16_t *q, *k, *v;   // qkv strides
    const uint16_t *o, *dout;    // out strides
    const float *lse;            // (n_bh, seq_len), contiguous
    float *delta;                // workspace: (n_bh, seq_len)
    uint16_t *dq, *dk, *dv;      // out strides
    int64_t qkv_bs, qkv_ss, qkv_hs;   // elements
    int64_t out_bs, out_ss, out_hs;
    int32_t seq_len, n_heads, n_bh;
};

namespace bwd {

constexpr int D = 128;
constexpr int TROWS = 64;                 // rows of an LDS tile
constexpr int TBYTES = TROWS * 2 * D;     // 16 KiB
constexpr int THREADS = 256;
constexpr int CHUNKS = TROWS * 16 / THREADS;   // 16-B chunks of a tile per thread (4)
constexpr int KB = 128;                   // keys per dK / dV workgroup, Q rows per dQ workgroup (4 waves x 32)

// byte offset of 16-B chunk `ch` of row `row` in a tile image (T10 (b): conflict-free row and transposed reads)
FA_DEV unsigned img_off(int row, int ch) {
    return 256u * (unsigned)row + 16u * (unsigned)(ch ^ (((row & 3) << 2) | ((row >> 2) & 3)));
}

struct TileRegs {
    u32x4 v[CHUNKS];
};
FA_DEV void tile_load(TileRegs &t, const uint16_t *rows0, int64_t ss, int tid) {
#pragma unroll
    for (int u = 0; u < CHUNKS; ++u) {
        const int c = tid + THREADS * u, row = c >> 4, ch = c & 15;
        t.v[u] = *(const u32x4 *)(rows0 + (int64_t)row * ss + ch * 8);
    }
}
FA_DEV void tile_store(char *img, const TileRegs &t, int tid) {
#pragma unroll
    for (int u = 0; u < CHUNKS; ++u) {
        const int c = tid + THREADS * u;
        *(u32x4 *)(img + img_off(c >> 4, c & 15)) = t.v[u];
    }
}

// A operand, rows: lane (r, h) gets row rb + r, elements 16 ks + 8 h .. + 7
template <class vec8> FA_DEV vec8 row_read(const char *img, int rb, int ks, int lane) {
    return *(const vec8 *)(img + img_off(rb + (lane & 31), 2 * ks + (lane >> 5)));
}

// A operand, transposed: element j of lane (r, h) = image[row rb + 16 s + 8 (j >> 2) + 4 h + (j & 3)][col 32 t + r] -- the
// k order of an accumulator tile's registers 8 s .. 8 s + 7 taken as the B operand.  Two ds_read_b64_tr_b16: per group of 16
// lanes a 4-row x 16-column block, lane 4q + p addressing row q, columns 4p .. 4p + 3.  EXEC must be full (no divergence).
template <class vec8> FA_DEV vec8 tr_read(const char *img, int rb, int s, int t, int lane) {
    const int q = (lane >> 2) & 3, p = lane & 3, g1 = (lane >> 4) & 1, h = lane >> 5;
    const int row = rb + 16 * s + 4 * h + q, ch = 4 * t + 2 * g1 + (p >> 1);
    typedef FA_LDS(s16x4) lds_s16x4;
    const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4 *)(img + img_off(row, ch) + 8 * (p & 1)));
    const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4 *)(img + img_off(row + 8, ch) + 8 * (p & 1)));
    const s16x8 r = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
    return __builtin_bit_cast(vec8, r);
}

// registers 8 s .. 8 s + 7 of an accumulator tile, rounded to the 16-bit type: the B operand of k step s
template <int DT> FA_DEV typename Elem<DT>::vec8 acc_operand(const f32x16 &x, int s) {
    float f[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) f[j] = x[8 * s + j];
    return Elem<DT>::pack8(f);
}

// workgroup -> (batch*head, block): XCD-aware when the grid is a multiple of 8 (workgroups are dealt round-robin over the
// eight XCDs; consecutive blocks of one head then share an XCD's L2 copy of the operands they all stream)
FA_DEV void block_coords(int n_blocks, int &bh, int &blk) {
    int bid = (int)blockIdx.x;
    const int n = (int)gridDim.x;
    if ((n & 7) == 0) bid = (bid & 7) * (n >> 3) + (bid >> 3);
    bh = bid / n_blocks;
    blk = bid % n_blocks;
}

// 4 accumulator rows (d = 32 t + 8 g + 4 h .. + 3) of one column, scaled, RNE to 16 bit: one 8-byte store
template <int DT> FA_DEV void store4(uint16_t *dst, const f32x16 &x, int g, float scale) {
    u32x2 w;
    w[0] = Elem<DT>::pack2(x[4 * g] * scale, x[4 * g + 1] * scale);
    w[1] = Elem<DT>::pack2(x[4 * g + 2] * scale, x[4 * g + 3] * scale);
    *(u32x2 *)dst = w;
}

FA_DEV float log2e_over_c() {   // sqrt(d) as the forward's c = rsqrt(d) log2(e) (fa_fwd_kernel64.hpp) sees it
    const float c = (float)((double)(1.0f / __builtin_sqrtf((float)D)) * 1.4426950408889634074);
    return 1.4426950408889634f / c;
}

}  // namespace bwd

// delta_i = sum_d dO_id O_id (fp32 products of the 16-bit values), 16 lanes per row
template <int DT>
__global__ void __launch_bounds__(256) fa_bwd_delta_kernel(const BwdArgs a) {
    using E = Elem<DT>;
    const int64_t rows = (int64_t)a.n_bh * a.seq_len;
    const int64_t row = (int64_t)blockIdx.x * 16 + (threadIdx.x >> 4);
    const int part = threadIdx.x & 15;
    float acc = 0.0f;
    if (row < rows) {
        const int bh = (int)(row / a.seq_len), i = (int)(row % a.seq_len);
        const int64_t off = (int64_t)(bh / a.n_heads) * a.out_bs + (int64_t)(bh % a.n_heads) * a.out_hs + (int64_t)i * a.out_ss + part * 8;
        const typename E::vec8 o = *(const typename E::vec8 *)(a.o + off);
        const typename E::vec8 g = *(const typename E::vec8 *)(a.dout + off);
#pragma unroll
        for (int j = 0; j < 8; ++j) acc += (float)o[j] * (float)g[j];
    }
#pragma unroll
    for (int m = 8; m >= 1; m >>= 1) acc += __shfl_xor(acc, m, 16);
    if (row < rows && part == 0) a.delta[row] = acc;
}

// dK, dV of one 128-key block.  Grid: n_bh * seq_len / 128 workgroups of 256 threads.
template <int DT, bool CAUSAL>
__global__ void __launch_bounds__(bwd::THREADS, 1) fa_bwd_dkdv_kernel(const BwdArgs a) {
    using namespace bwd;
    using E = Elem<DT>;
    using vec8 = typename E::vec8;
    __shared__ __attribute__((aligned(16))) char img_q[TBYTES];
    __shared__ __attribute__((aligned(16))) char img_do[TBYTES];
    __shared__ __attribute__((aligned(16))) float lse_s[TROWS];   // -lse sqrt(d) of the tile's rows
    __shared__ __attribute__((aligned(16))) float dl_s[TROWS];    // -delta
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 31, h = lane >> 5;
    int bh, kb;
    block_coords(a.seq_len / KB, bh, kb);
    const int64_t qkv_head = (int64_t)(bh / a.n_heads) * a.qkv_bs + (int64_t)(bh % a.n_heads) * a.qkv_hs;
    const int64_t out_head = (int64_t)(bh / a.n_heads) * a.out_bs + (int64_t)(bh % a.n_heads) * a.out_hs;
    const int key = kb * KB + 32 * wave + r;   // this lane's key (the accumulators' column)
    // K, V of the wave's 32 keys: the B operands of S = Q K^T and dP = dO V^T, resident for the whole sweep
    vec8 Kb[8], Vb[8];
    {
        const uint16_t *kr = a.k + qkv_head + (int64_t)key * a.qkv_ss + 8 * h;
        const uint16_t *vr = a.v + qkv_head + (int64_t)key * a.qkv_ss + 8 * h;
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
    for (int it = it0; it < n_it; ++it) {
        __syncthreads();   // every wave is done with the previous tile's images
        tile_store(img_q, tq, tid);
        tile_store(img_do, tdo, tid);
        if (tid < TROWS) {
            lse_s[tid] = lse_r;
            dl_s[tid] = dl_r;
        }
        __syncthreads();
        if (it + 1 < n_it) load(it + 1);   // in flight under this tile's MFMAs
        const bool diag = CAUSAL && it * TROWS < kb * KB + KB;   // a tile that holds queries before some key of the block
#pragma unroll
        for (int mt = 0; mt < TROWS / 32; ++mt) {
            const int rb = 32 * mt;
            f32x16 S, dP;
            // rows of registers 4g .. 4g + 3: rb + 8 g + 4 h + 0 .. 3
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const f32x4 l4 = *(const f32x4 *)(lse_s + rb + 8 * g + 4 * h);
                const f32x4 d4 = *(const f32x4 *)(dl_s + rb + 8 * g + 4 * h);
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    S[4 * g + e] = l4[e];
                    dP[4 * g + e] = d4[e];
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
    // dK^T / dV^T: column = this lane's key, rows d = 32 t + 8 g + 4 h + 0 .. 3
    const float inv_sqrt_d = 1.0f / __builtin_sqrtf((float)D);
    uint16_t *dk = a.dk + out_head + (int64_t)key * a.out_ss + 4 * h;
    uint16_t *dv = a.dv + out_head + (int64_t)key * a.out_ss + 4 * h;
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            store4<DT>(dk + 32 * t + 8 * g, dK[t], g, inv_sqrt_d);
            store4<DT>(dv + 32 * t + 8 * g, dV[t], g, 1.0f);
        }
}

// dQ of one 128-row Q block.  Grid: n_bh * seq_len / 128 workgroups of 256 threads.
template <int DT, bool CAUSAL>
__global__ void __launch_bounds__(bwd::THREADS, 1) fa_bwd_dq_kernel(const BwdArgs a) {
    using namespace bwd;
    using E = Elem<DT>;
    using vec8 = typename E::vec8;
    __shared__ __attribute__((aligned(16))) char img_k[TBYTES];
    __shared__ __attribute__((aligned(16))) char img_v[TBYTES];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 31, h = lane >> 5;
    const int nqb = a.seq_len / KB;
    int bh, qb;
    block_coords(nqb, bh, qb);
    if (CAUSAL) qb = nqb - 1 - qb;   // the longest sweeps first
    const int64_t qkv_head = (int64_t)(bh / a.n_heads) * a.qkv_bs + (int64_t)(bh % a.n_heads) * a.qkv_hs;
    const int64_t out_head = (int64_t)(bh / a.n_heads) * a.out_bs + (int64_t)(bh % a.n_heads) * a.out_hs;
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
        tile_load(tk, a.k + qkv_head + (int64_t)kt * TROWS * a.qkv_ss, a.qkv_ss, tid);
        tile_load(tv, a.v + qkv_head + (int64_t)kt * TROWS * a.qkv_ss, a.qkv_ss, tid);
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
        for (int g = 0; g < 4; ++g) store4<DT>(dq + 32 * t + 8 * g, dQ[t], g, inv_sqrt_d);
}

}  // namespace fa
