// fa_bwd64_kernel.hpp -- the backward over packed variable-length sequences at d_head = 64 for gfx950 (DESIGN.md 9.7;
// fa_bwd_launch_varlen_qk_d64): dQ, dK, dV from fa_prefill64_kernel.hpp's (o, lse) under two ranges, a sliding window that is
// always present (none: left = right = 2^30, causal: right = 0) and optional attention sinks, whose own gradient it adds.  A text of
// its own beside fa_bwd_varlen.hpp, whose tile arithmetic is tied to 256-byte rows and one wave per SIMD.
//
// The mathematics is fa_bwd_kernel.hpp's at the scale 1 / sqrt(64): delta = rowsum(dO o O), P = exp2(c s - lse log2 e),
// dV += P^T dO, dP = dO V^T, dS = P o (dP - delta), dK += dS^T Q / 8, dQ += dS K / 8.  c = log2(e) / 8 is rounded once from the
// double product, 1 / 8 is exact.  With sinks the forward's lse holds the sink, P sums to less than 1 per row, delta is unchanged
// (the sink's value row is 0) and dS stands; dsinks[h] = - sum_rows exp(z_h - lse) delta.
//
// The split (DESIGN.md 9.7 weighs it against 64 per wave at one wave per SIMD): a wave owns 32 keys (dK / dV) or 32 rows (dQ), a
// workgroup of 4 waves 128, and TWO workgroups share a CU -- two waves per SIMD, __launch_bounds__(256, 2).  At 64 a 64 x 32 tile pair
// is 8 MFMAs per product instead of 16 while exp2, the mask, dS, the packing, the barrier and the address work per tile stay, so
// what runs beside the MFMA pipe is relatively twice as dear as at 128; the second wave's MFMAs run under the first one's softmax
// and dS.  The accumulators halve (dK^T + dV^T of 32 keys: 64 registers, dQ^T of 32 rows: 32) and so do the tiles (8 KiB), which
// pays for both the second wave and a second LDS image:
//   fa_bwd64_delta_kernel   delta per (head, query row), 8 lanes per 128-byte row, fp32 into the workspace
//   fa_bwd64_dkdv_kernel    one workgroup per (sequence, K / V head, split part, 128-key block of max_seqlen_k): K, V of the
//                           wave's 32 keys resident as B operands; it sweeps the 64-row Q / dO tiles of the block's window over
//                           group / split query heads; fp32 accumulators rounded once, or (split > 1) written as fp32 partials
//   fa_bwd64_reduce_kernel  split > 1: a key row's partials summed in split order, scaled and rounded once
//   fa_bwd64_dq_kernel      one workgroup per (sequence, head, 128-row block of max_seqlen_q): Q, dO of the wave's 32 rows resident;
//                           it sweeps the 64-key K / V tiles of the block's window
//   fa_bwd64_dsinks_kernel  one workgroup per head over lse and delta (fa_bwd_dsinks_varlen_kernel's sum, restated in
//                           fa_bwd_varlen64.hip so that fa_bwd_varlen_sinks.hip keeps its text).  The delta it reads is the dQ
//                           kernel's: with sinks that kernel writes each row's sum_j P_j dP_j (fp32, over the keys the row sees)
//                           over the delta kernel's rowsum(dO o O) -- the same number without O's rounding to 16 bit
// The split rule is bwd_dkdv_split's on the key side's grid (fa_capi.hip), a function of the shape alone.
//
// Products (v_mfma_f32_32x32x16_{bf16,f16}; an accumulator has its column on the lane and its rows in the 16 registers, so a
// product that sums over that row index takes it as the B operand with no lane movement):
//   dK / dV kernel  S = Q K^T and dP = dO V^T with the KEY on the lane: A = tile rows by ds_read_b128, B = K / V resident; then
//                   dV^T = dO^T P and dK^T = Q^T dS: A = the same images by ds_read_b64_tr_b16, B = P / dS packed in place.
//   dQ kernel       S^T = K Q^T and dP^T = V dO^T with the QUERY on the lane (lse and delta are lane-local scalars), then
//                   dQ^T = K^T dS^T.
// The accumulators start at 0; the row's -lse log2(e) joins in the exponent's fma, exp2(fma(S, c, -lse log2 e)), and -delta in
// dS = p (dP + -delta): one instruction each, like the d128 kernels' `c * S` from a biased accumulator, without their 32 moves.
//
// LDS.  A tile (Q, dO or K, V: 64 rows x 64 halves) has ONE image with 128-byte rows, read by rows and by columns.  Byte offset of
// 16-byte chunk ch (0 .. 7) of row r: 128 r + 16 (ch ^ f(r)), f(r) = 4 ((r >> 1) & 1) | ((r >> 2) & 3).  LDS has 64 banks of 4 bytes:
//  * written by ds_write_b128, 16 lanes a pass: lanes 16 k .. 16 k + 15 hold the 8 chunks of rows 2 k and 2 k + 1, which share
//    f: 16 different 16-byte slots of one 256-byte line -- every bank once;
//  * read by rows (ds_read_b128, 16 lanes a pass: one chunk of 16 consecutive rows): a row's slot in its 256-byte line is
//    8 (r & 1) + (ch ^ f(r)); over 16 consecutive rows (r >> 1) & 7 takes every value and f is a bijection of it (its bits
//    reordered), so each parity's 8 rows take 8 different slots -- every bank once.  Unswizzled: 2 slots, an 8-way conflict;
//  * read by columns (ds_read_b64_tr_b16, 32 lanes a pass: rows 4 m .. 4 m + 3, the 4 chunks 4 t .. 4 t + 3, 8 bytes per
//    lane): rows 4 m and 4 m + 1 have f's bit 2 clear, rows 4 m + 2 and 4 m + 3 set, and the low bits equal, so the four rows take
//    chunk groups t, t, t ^ 1, t ^ 1 on parities 0, 1, 0, 1 -- 16 different slots, every bank once.  This is what
//    fa_prefill64_kernel.hpp's XOR (r >> 1) & 7 (an image read by rows only) does not give: there rows 4 m and 4 m + 2 fall on
//    the same four slots, a 2-way conflict on every transposed read; hence bit 1 of the row goes to bit 2 of the XOR.
//  Tiles travel global -> registers -> LDS into one of TWO images: tile i + 1 is loaded before tile i's MFMAs and stored behind
//  them into the image tile i - 1 used, so a tile costs ONE barrier (the d128 kernels: two).  2 x 16 KiB (+ 1 KiB of row statistics
//  in the dK / dV kernel) per workgroup, two workgroups per CU.
//
// Window, ends, dead rows: the d128 window form's rules and argument (the header comment of fa_bwd_varlen.hpp), which hold here
// because KB = 128 and the tile of 64 rows are the same.  Row r at p = r + shift, shift = len_k - len_q, sees keys
// max(0, p - left) .. min(len_k - 1, p + right).  A block visits only the tiles of its window (bwd::window_tiles); none: it stores
// zeros -- rows that see no key get dq = 0 and keys no row sees dk = dv = 0, WRITTEN.  The mask is a select on p behind the
// workgroup-uniform `outside`, true only on a tile that reaches outside some row's window or past either end.  A dead row (one that
// sees no key) has lse = -inf without a sink -- its exponent's addend is set to -inf, p = exp2(-inf) = 0, its delta to 0 -- or the
// finite z with one: then exp2 may give anything up to +inf, but r + shift + right < 0 <= every key, so every tile that holds r is
// `outside` (its last term) and the select's `key > query + shift + right` makes p exactly 0; dS = 0 (dP - delta) with both finite.
// Nothing of a dead row reaches dK / dV, its dq is 0, and with delta = 0 (o = 0) it adds exactly 0 to dsinks.
// Rows beyond a range's end are fetched from THAT range's last row (bwd::seq_range_of clamps both ranges, so a cu_seqlens violation
// cannot fault) and masked by the same select (query >= len_q, key >= len_k: such tiles are `outside` by `edge`); a lane whose own
// key or row lies beyond the end feeds only its own accumulator column, which is never stored.
// Positions are 32-bit (the host bounds max_seqlen on both sides by 2^30 - 128); every element offset is formed in 64 bits.
// No float atomics, no waiting between workgroups, no scratch; the host reads no device array.
#pragma once
#include "fa_bwd_varlen.hpp"   // bwd::seq_range_of, window_tiles, block_coords, acc_operand, store4 (none of them knows d_head)

namespace fa {

struct Bwd64Args {
    const uint16_t *q, *k, *v;        // q_* / kv_* strides
    const uint16_t *o, *dout;         // out_* strides
    const float *lse;                 // (n_heads, total_q), contiguous
    float *delta;                     // workspace: (n_heads, total_q)
    uint16_t *dq, *dk, *dv;           // dq: out_* strides; dk, dv: dkv_*
    const int32_t *cu_q, *cu_k;       // n_seqs + 1 entries each
    float *part;                      // split > 1: (n_kv_heads * split, total_k, 2, 64) fp32 dK^T | dV^T, unscaled
    const float *sinks;               // (n_heads) fp32, or null: no sinks
    float *dsinks;                    // (n_heads) fp32, written when sinks is given
    int64_t q_ss, q_hs;               // elements
    int64_t out_ss, out_hs;
    int64_t kv_ss, kv_hs;
    int64_t dkv_ss, dkv_hs;
    int32_t n_seqs, n_heads;
    int32_t total_q, max_seqlen_q, total_k, max_seqlen_k;
    int32_t group, split;             // query heads per K / V head; workgroups per (K / V head, key block), divides group
    int32_t n_blocks_q, n_blocks_k;   // ceil(max_seqlen / 128) of either side
    int32_t left, right;              // unbounded: 2^30; causal: right = 0
};

namespace bwd64 {

constexpr int D = 64;
constexpr int TROWS = bwd::TROWS;          // rows of an LDS tile (64: bwd::window_tiles counts in them)
constexpr int TBYTES = TROWS * 2 * D;      // 8 KiB
constexpr int THREADS = 256;
constexpr int CHUNKS = TROWS * 8 / THREADS;   // 16-byte chunks of a tile per thread (2)
constexpr int KB = 128;                    // keys per dK / dV workgroup, rows per dQ workgroup (4 waves x 32)
constexpr int KS = D / 16, DT32 = D / 32;  // k-steps of S / dP; 32-wide d tiles of the transposed products
constexpr float C = (float)(0.125 * 1.4426950408889634074);   // log2(e) / sqrt(64), rounded once
constexpr float SCALE = 0.125f;            // 1 / sqrt(64), exact
constexpr float LOG2E = 1.4426950408889634074f;

FA_DEV unsigned img_off(int row, int ch) {
    return 128u * (unsigned)row + 16u * (unsigned)(ch ^ ((((row >> 1) & 1) << 2) | ((row >> 2) & 3)));
}

struct TileRegs {
    u32x4 v[CHUNKS];
};
// tile rows first .. first + 63 of a sequence, row first + r fetched from row min(first + r, last)
FA_DEV void tile_load(TileRegs &t, const uint16_t *seq_rows, int64_t ss, int first, int last, int tid) {
#pragma unroll
    for (int u = 0; u < CHUNKS; ++u) {
        const int c = tid + THREADS * u, ch = c & 7;
        int row = first + (c >> 3);
        row = row < last ? row : last;
        t.v[u] = *(const u32x4 *)(seq_rows + (int64_t)row * ss + ch * 8);
    }
}
FA_DEV void tile_store(char *img, const TileRegs &t, int tid) {
#pragma unroll
    for (int u = 0; u < CHUNKS; ++u) {
        const int c = tid + THREADS * u;
        *(u32x4 *)(img + img_off(c >> 3, c & 7)) = t.v[u];
    }
}

// A operand, rows: lane (r, h) gets row rb + r, elements 16 ks + 8 h .. + 7
template <class vec8> FA_DEV vec8 row_read(const char *img, int rb, int ks, int lane) {
    return *(const vec8 *)(img + img_off(rb + (lane & 31), 2 * ks + (lane >> 5)));
}

// A operand, transposed: element j of lane (r, h) = image[row rb + 16 s + 8 (j >> 2) + 4 h + (j & 3)][col 32 t + r], the k order of
// an accumulator's registers 8 s .. 8 s + 7 taken as the B operand.  Two ds_read_b64_tr_b16: per group of 16 lanes a 4-row x
// 16-column block, lane 4 q + p addressing row q, columns 4 p .. 4 p + 3.  EXEC must be full.
template <class vec8> FA_DEV vec8 tr_read(const char *img, int rb, int s, int t, int lane) {
    const int q = (lane >> 2) & 3, p = lane & 3, g1 = (lane >> 4) & 1, h = lane >> 5;
    const int row = rb + 16 * s + 4 * h + q, ch = 4 * t + 2 * g1 + (p >> 1);
    typedef FA_LDS(s16x4) lds_s16x4;
    const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4 *)(img + img_off(row, ch) + 8 * (p & 1)));
    const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4 *)(img + img_off(row + 8, ch) + 8 * (p & 1)));
    const s16x8 r = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
    return __builtin_bit_cast(vec8, r);
}

// a row's (or key's) place outside the window of `query` at `shift`, or beyond either end: p becomes 0
FA_DEV bool hidden(const Bwd64Args &a, int key, int query, int shift, int klen, int len) {
    return key < query + shift - a.left || key > query + shift + a.right || key >= klen || query >= len;
}

}  // namespace bwd64

// delta_i = sum_d dO_id O_id per (head, query row): 8 lanes per row, 32 rows per workgroup.  Grid: ceil(n_heads total_q / 32)
template <int DT>
__global__ void __launch_bounds__(256) fa_bwd64_delta_kernel(const Bwd64Args a) {
    using E = Elem<DT>;
    const int64_t rows = (int64_t)a.n_heads * a.total_q;
    const int64_t row = (int64_t)blockIdx.x * 32 + (threadIdx.x >> 3);
    const int part = threadIdx.x & 7;
    float acc = 0.0f;
    if (row < rows) {
        const int64_t hd = row / a.total_q, i = row % a.total_q;
        const int64_t off = hd * a.out_hs + i * a.out_ss + part * 8;
        const typename E::vec8 o = *(const typename E::vec8 *)(a.o + off);
        const typename E::vec8 g = *(const typename E::vec8 *)(a.dout + off);
#pragma unroll
        for (int j = 0; j < 8; ++j) acc += (float)o[j] * (float)g[j];
    }
#pragma unroll
    for (int m = 4; m >= 1; m >>= 1) acc += __shfl_xor(acc, m, 8);
    if (row < rows && part == 0) a.delta[row] = acc;
}

// dK, dV of one 128-key block of one K / V head of one sequence, summed over group / split query heads.
// Grid: n_seqs * n_kv_heads * split * n_blocks_k workgroups of 256 threads.
template <int DT>
__global__ void __launch_bounds__(bwd64::THREADS, 2) fa_bwd64_dkdv_kernel(const Bwd64Args a) {
    using namespace bwd64;
    using E = Elem<DT>;
    using vec8 = typename E::vec8;
    __shared__ __attribute__((aligned(16))) char img[2][2][TBYTES];   // [image][Q | dO]
    __shared__ __attribute__((aligned(16))) float stat[2][2][TROWS];  // [image][-lse log2(e) | -delta] of the tile's rows
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 31, h = lane >> 5;
    int wg, kb;   // wg = (sequence * n_kv_heads + K / V head) * split + part
    bwd::block_coords(a.n_blocks_k, wg, kb);
    const int n_kv = a.n_heads / a.group, skv = wg / a.split, seq = skv / n_kv, hk = skv % n_kv, sp = wg % a.split;
    int row0, len, krow0, klen;   // the sequence's query rows and key rows
    bwd::seq_range_of(a.cu_q, a.total_q, a.max_seqlen_q, seq, row0, len);
    bwd::seq_range_of(a.cu_k, a.total_k, a.max_seqlen_k, seq, krow0, klen);
    if (kb * KB >= klen) return;   // (workgroup-uniform, before any barrier)
    const int last = len - 1, klast = klen - 1, shift = klen - len;
    const int n_hq = a.group / a.split;   // query heads of the sweep: hk * group + part * n_hq + 0 .. n_hq - 1
    int hq = hk * a.group + sp * n_hq;
    const uint16_t *q_seq = a.q + (int64_t)row0 * a.q_ss + (int64_t)hq * a.q_hs;
    const uint16_t *do_seq = a.dout + (int64_t)row0 * a.out_ss + (int64_t)hq * a.out_hs;
    const float *lse_h = a.lse + (int64_t)hq * a.total_q + row0;
    const float *dl_h = a.delta + (int64_t)hq * a.total_q + row0;
    const int key = kb * KB + 32 * wave + r;   // this lane's key (the accumulators' column)
    const int key_c = key < klast ? key : klast;
    vec8 Kb[KS], Vb[KS];   // K, V of the wave's 32 keys, resident
    {
        const int64_t kv_row = (int64_t)(krow0 + key_c) * a.kv_ss + (int64_t)hk * a.kv_hs + 8 * h;
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
            Kb[ks] = *(const vec8 *)(a.k + kv_row + 16 * ks);
            Vb[ks] = *(const vec8 *)(a.v + kv_row + 16 * ks);
        }
    }
    f32x16 dV[DT32], dK[DT32];
#pragma unroll
    for (int t = 0; t < DT32; ++t) {
        dV[t] = f32x16{};
        dK[t] = f32x16{};
    }
    // key j is seen by rows j - shift - right .. j - shift + left: the block's keys (up to the sequence's last) by tiles it0 .. n_it - 1
    int it0, n_it;
    bwd::window_tiles(kb * KB - shift - a.right, (kb * KB + KB - 1 < klast ? kb * KB + KB - 1 : klast) - shift + a.left, len, it0, n_it);
    const int steps = (n_it - it0) * n_hq;   // (tile, query head) pairs of the sweep, heads outermost
    TileRegs tq, tdo;
    float nl_r = 0.0f, nd_r = 0.0f;
    auto load = [&](int it) {
        tile_load(tq, q_seq, a.q_ss, it * TROWS, last, tid);
        tile_load(tdo, do_seq, a.out_ss, it * TROWS, last, tid);
        if (tid < TROWS) {
            const int row = it * TROWS + tid;
            const int row_c = row < last ? row : last;
            const float lse_v = lse_h[row_c];
            const bool live = row < len && lse_v != -__builtin_inff();   // (a row without key or sink: p = exp2(-inf) = 0, delta 0)
            nl_r = live ? lse_v * -LOG2E : -__builtin_inff();
            nd_r = live ? -dl_h[row_c] : 0.0f;
        }
    };
    auto stash = [&](int b) {
        tile_store(img[b][0], tq, tid);
        tile_store(img[b][1], tdo, tid);
        if (tid < TROWS) {
            stat[b][0][tid] = nl_r;
            stat[b][1][tid] = nd_r;
        }
    };
    if (steps > 0) {   // (no row sees the block: nothing to fetch -- len_q may be 0)
        load(it0);
        stash(0);
    }
    __syncthreads();
    const bool key_edge = kb * KB + KB > klen;   // a block that holds keys beyond the sequence
    int it = it0, b = 0;
    for (int step = 0; step < steps; ++step, b ^= 1) {
        const bool more = step + 1 < steps;
        int it_next = it + 1;
        if (more) {   // the next tile, or the next query head's first: in flight under this tile's MFMAs
            if (it_next == n_it) {
                it_next = it0;
                q_seq += a.q_hs;
                do_seq += a.out_hs;
                lse_h += a.total_q;
                dl_h += a.total_q;
            }
            load(it_next);
        }
        // a tile that holds rows or keys beyond the sequence, or reaches outside some row's window: its last row's floor above the
        // block's first key, or its first row's ceiling below the block's last
        const bool edge = key_edge || it * TROWS + TROWS > len;
        const bool outside = edge || it * TROWS + TROWS - 1 + shift - a.left > kb * KB || it * TROWS + shift + a.right < kb * KB + KB - 1;
        const char *img_q = img[b][0], *img_do = img[b][1];
#pragma unroll
        for (int mt = 0; mt < TROWS / 32; ++mt) {
            const int rb = 32 * mt;
            f32x16 S = {}, dP = {};
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) S = E::mfma(row_read<vec8>(img_q, rb, ks, lane), Kb[ks], S);
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) dP = E::mfma(row_read<vec8>(img_do, rb, ks, lane), Vb[ks], dP);
            // rows of registers 4 g .. 4 g + 3: rb + 8 g + 4 h + 0 .. 3
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const f32x4 l4 = *(const f32x4 *)(stat[b][0] + rb + 8 * g + 4 * h);
                const f32x4 d4 = *(const f32x4 *)(stat[b][1] + rb + 8 * g + 4 * h);
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int i = 4 * g + e;
                    float p = __builtin_amdgcn_exp2f(__builtin_fmaf(S[i], C, l4[e]));
                    if (outside) p = hidden(a, key, it * TROWS + rb + 8 * g + 4 * h + e, shift, klen, len) ? 0.0f : p;
                    S[i] = p;                        // P
                    dP[i] = p * (dP[i] + d4[e]);     // dS = P (dP - delta)
                }
            }
#pragma unroll
            for (int s = 0; s < 2; ++s) {
                const vec8 pb = bwd::acc_operand<DT>(S, s), db = bwd::acc_operand<DT>(dP, s);
#pragma unroll
                for (int t = 0; t < DT32; ++t) {
                    dV[t] = E::mfma(tr_read<vec8>(img_do, rb, s, t, lane), pb, dV[t]);
                    dK[t] = E::mfma(tr_read<vec8>(img_q, rb, s, t, lane), db, dK[t]);
                }
            }
        }
        if (more) stash(b ^ 1);   // (the image the previous tile used: every wave left it at the last barrier)
        __syncthreads();
        it = it_next;
    }
    if (key >= klen) return;   // (behind the last barrier and the last transposed read)
    // dK^T / dV^T: column = this lane's key, rows d = 32 t + 8 g + 4 h + 0 .. 3
    if (a.split > 1) {   // the fp32 partials, unscaled: fa_bwd64_reduce_kernel rounds their sum
        float *pk = a.part + (((int64_t)hk * a.split + sp) * a.total_k + krow0 + key) * (2 * D) + 4 * h;
#pragma unroll
        for (int t = 0; t < DT32; ++t)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                *(f32x4 *)(pk + 32 * t + 8 * g) = f32x4{dK[t][4 * g], dK[t][4 * g + 1], dK[t][4 * g + 2], dK[t][4 * g + 3]};
                *(f32x4 *)(pk + D + 32 * t + 8 * g) = f32x4{dV[t][4 * g], dV[t][4 * g + 1], dV[t][4 * g + 2], dV[t][4 * g + 3]};
            }
        return;
    }
    const int64_t dkv_row = (int64_t)(krow0 + key) * a.dkv_ss + (int64_t)hk * a.dkv_hs + 4 * h;
#pragma unroll
    for (int t = 0; t < DT32; ++t)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            bwd::store4<DT>(a.dk + dkv_row + 32 * t + 8 * g, dK[t], g, SCALE);
            bwd::store4<DT>(a.dv + dkv_row + 32 * t + 8 * g, dV[t], g, 1.0f);
        }
}

// split > 1: dK, dV of one (K / V head, key token) row = the sum of its `split` partials in order, scaled and rounded once.
// One thread per 8 elements of a dK or dV row.  Grid: ceil(n_kv_heads total_k 2 8 / 256) workgroups of 256 threads.
// (every key row belongs to a sequence under the cu_seqlens contract, so every partial row was written)
template <int DT>
__global__ void __launch_bounds__(256) fa_bwd64_reduce_kernel(const Bwd64Args a) {
    using namespace bwd64;
    const int n_kv = a.n_heads / a.group;
    const int64_t n = (int64_t)n_kv * a.total_k * 2 * (D / 8);
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= n) return;
    const int c8 = (int)(idx % (D / 8)), which = (int)((idx / (D / 8)) & 1);   // 8-element chunk; 0 dK, 1 dV
    const int64_t row = idx / (2 * (D / 8));   // hk * total_k + token
    const int64_t hk = row / a.total_k, tok = row % a.total_k;
    const int64_t plane = (int64_t)a.total_k * 2 * D;   // floats per partial
    const float *src = a.part + (hk * a.split * a.total_k + tok) * (2 * D) + which * D + 8 * c8;
    f32x4 lo = *(const f32x4 *)src, hi = *(const f32x4 *)(src + 4);
    for (int s = 1; s < a.split; ++s) {
        lo += *(const f32x4 *)(src + s * plane);
        hi += *(const f32x4 *)(src + s * plane + 4);
    }
    const float scale = which ? 1.0f : SCALE;
    float f[8];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        f[e] = lo[e] * scale;
        f[4 + e] = hi[e] * scale;
    }
    uint16_t *dst = (which ? a.dv : a.dk) + hk * a.dkv_hs + tok * a.dkv_ss + 8 * c8;
    *(typename Elem<DT>::vec8 *)dst = Elem<DT>::pack8(f);
}

// dQ of one 128-row block of one head of one sequence, K / V of head h / group.  Grid: n_seqs * n_heads * n_blocks_q workgroups.
template <int DT>
__global__ void __launch_bounds__(bwd64::THREADS, 2) fa_bwd64_dq_kernel(const Bwd64Args a) {
    using namespace bwd64;
    using E = Elem<DT>;
    using vec8 = typename E::vec8;
    __shared__ __attribute__((aligned(16))) char img[2][2][TBYTES];   // [image][K | V]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 31, h = lane >> 5;
    int sh, qb;   // sh = sequence * n_heads + head
    bwd::block_coords(a.n_blocks_q, sh, qb);
    const int seq = sh / a.n_heads, hq = sh % a.n_heads;
    int row0, len, krow0, klen;
    bwd::seq_range_of(a.cu_q, a.total_q, a.max_seqlen_q, seq, row0, len);
    bwd::seq_range_of(a.cu_k, a.total_k, a.max_seqlen_k, seq, krow0, klen);
    if (qb * KB >= len) return;   // (workgroup-uniform, before any barrier)
    const int last = len - 1, klast = klen - 1, shift = klen - len;
    const uint16_t *k_seq = a.k + (int64_t)krow0 * a.kv_ss + (int64_t)(hq / a.group) * a.kv_hs;
    const uint16_t *v_seq = a.v + (int64_t)krow0 * a.kv_ss + (int64_t)(hq / a.group) * a.kv_hs;
    const int query = qb * KB + 32 * wave + r;   // this lane's row (the accumulators' column)
    const int query_c = query < last ? query : last;
    vec8 Qb[KS], Ob[KS];   // Q, dO of the wave's 32 rows, resident
    {
        const uint16_t *qr = a.q + (int64_t)(row0 + query_c) * a.q_ss + (int64_t)hq * a.q_hs + 8 * h;
        const uint16_t *gr = a.dout + (int64_t)(row0 + query_c) * a.out_ss + (int64_t)hq * a.out_hs + 8 * h;
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
            Qb[ks] = *(const vec8 *)(qr + 16 * ks);
            Ob[ks] = *(const vec8 *)(gr + 16 * ks);
        }
    }
    const int64_t stat = (int64_t)hq * a.total_q + row0 + query_c;
    const float lse_v = a.lse[stat];
    const bool live = query < len && lse_v != -__builtin_inff();   // (as in the dK / dV kernel)
    const float nl = live ? lse_v * -LOG2E : -__builtin_inff();
    const float nd = live ? -a.delta[stat] : 0.0f;
    f32x16 dQ[DT32];
#pragma unroll
    for (int t = 0; t < DT32; ++t) dQ[t] = f32x16{};
    float pdp = 0.0f;   // sum over this lane's keys of P dP: with the other half's, the row's delta from the unrounded P (for dsinks)
    // the block's rows (up to the sequence's last) see the keys from its first row's floor to its last row's ceiling: tiles kt0 .. n_kt - 1
    int kt0, n_kt;
    bwd::window_tiles(qb * KB + shift - a.left, (qb * KB + KB - 1 < last ? qb * KB + KB - 1 : last) + shift + a.right, klen, kt0, n_kt);
    TileRegs tk, tv;
    auto load = [&](int kt) {
        tile_load(tk, k_seq, a.kv_ss, kt * TROWS, klast, tid);
        tile_load(tv, v_seq, a.kv_ss, kt * TROWS, klast, tid);
    };
    auto stash = [&](int b) {
        tile_store(img[b][0], tk, tid);
        tile_store(img[b][1], tv, tid);
    };
    if (kt0 < n_kt) {   // (no key in the window: nothing to fetch -- len_k may be 0)
        load(kt0);
        stash(0);
    }
    __syncthreads();
    const bool query_edge = qb * KB + KB > len;   // a block that holds rows beyond the sequence
    int b = 0;
    for (int kt = kt0; kt < n_kt; ++kt, b ^= 1) {
        const bool more = kt + 1 < n_kt;
        if (more) load(kt + 1);   // in flight under this tile's MFMAs
        // a tile that holds rows or keys beyond the sequence, or reaches outside some row's window: its first key below the block's
        // last row's floor, or its last key above the block's first row's ceiling
        const bool edge = query_edge || kt * TROWS + TROWS > klen;
        const bool outside = edge || kt * TROWS < qb * KB + KB - 1 + shift - a.left || kt * TROWS + TROWS - 1 > qb * KB + shift + a.right;
        const char *img_k = img[b][0], *img_v = img[b][1];
#pragma unroll
        for (int mt = 0; mt < TROWS / 32; ++mt) {
            const int rb = 32 * mt;
            f32x16 S = {}, dP = {};
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) S = E::mfma(row_read<vec8>(img_k, rb, ks, lane), Qb[ks], S);
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) dP = E::mfma(row_read<vec8>(img_v, rb, ks, lane), Ob[ks], dP);
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                float p = __builtin_amdgcn_exp2f(__builtin_fmaf(S[i], C, nl));
                if (outside) p = hidden(a, kt * TROWS + rb + (i & 3) + 8 * (i >> 2) + 4 * h, query, shift, klen, len) ? 0.0f : p;
                pdp = __builtin_fmaf(p, dP[i], pdp);
                dP[i] = p * (dP[i] + nd);   // dS^T
            }
#pragma unroll
            for (int s = 0; s < 2; ++s) {
                const vec8 db = bwd::acc_operand<DT>(dP, s);
#pragma unroll
                for (int t = 0; t < DT32; ++t) dQ[t] = E::mfma(tr_read<vec8>(img_k, rb, s, t, lane), db, dQ[t]);
            }
        }
        if (more) stash(b ^ 1);
        __syncthreads();
    }
    pdp += __shfl_xor(pdp, 32, 64);   // (the lane pair (r, 0), (r, 1) holds one row; every lane is still here)
    if (query >= len) return;
    // with sinks: the row's delta again, as sum_j P_j dP_j in fp32 -- rowsum(dO o O) without the rounding of O to 16 bit, which alone
    // would cost dsinks (a sum over every row of the head) more than the 16-bit eager reference errs by.  The row's one reader in
    // this kernel was this lane pair, the dK / dV kernel is done, and the dsinks kernel behind this one reads it
    if (a.sinks && h == 0) a.delta[stat] = pdp;
    uint16_t *dq = a.dq + (int64_t)(row0 + query) * a.out_ss + (int64_t)hq * a.out_hs + 4 * h;
#pragma unroll
    for (int t = 0; t < DT32; ++t)
#pragma unroll
        for (int g = 0; g < 4; ++g) bwd::store4<DT>(dq + 32 * t + 8 * g, dQ[t], g, SCALE);
}

// One backward: delta over total_q, dK / dV and (split > 1) their fixed-order sum over total_k, dQ, and with sinks their gradient,
// on one stream.  The grids depend on the host's arguments alone.  fa_bwd_varlen64.hip
hipError_t bwd64_enqueue(const Bwd64Args &a, int dtype, hipStream_t s);

}  // namespace fa
