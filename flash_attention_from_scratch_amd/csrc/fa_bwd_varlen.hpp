// fa_bwd_varlen.hpp -- the backward over packed variable-length sequences, with one range per sequence (fa_bwd_launch_varlen,
// BwdVarlenArgs), with separate Q and K / V ranges (fa_bwd_launch_varlen_qk, BwdVarlenQKArgs), or with two ranges under a sliding
// window (fa_bwd_launch_varlen_qk_window, BwdVarlenWindowArgs).  One text of each kernel serves all three: ARGS names the form,
// `if constexpr (QK)` / `if constexpr (WIN)` mark every site where they differ, and each form is instantiated in a translation
// unit of its own (fa_bwd_varlen.hip, fa_bwd_varlen_qk.hip, fa_bwd_varlen_window.hip), so the one-range kernels carry none of the
// second range's code and neither carries the window's.
//
// One range: Q, dO, dQ, O are (total_tokens, n_heads, 128), K, V, dK, dV (total_tokens, n_kv_heads, 128), and sequence i owns
// token rows cu_seqlens[i] .. cu_seqlens[i + 1] - 1 (cu_seqlens on the DEVICE: the host never reads it, the launch stays
// asynchronous).
//
// The kernels of fa_bwd_gqa.hpp (MHA is their group = 1 case) with the workgroup -> (sequence, head, 128-row block) lookup in
// front; the tile arithmetic (S, dP, dS, the five MFMA products, the operand orientation, the LDS images, the order of the
// fp32 sums) is theirs, line for line, so that a sequence whose length is a multiple of 256 gets the dense kernels' bits.
//   fa_bwd_delta_varlen_kernel        delta per (head, query token): no sequence lookup at all, one form
//   fa_bwd_dkdv_varlen_kernel         one workgroup per (sequence, K / V head, split part, 128-key block of max_seqlen)
//   fa_bwd_dkdv_reduce_varlen_kernel  split > 1 only: the sum of a key row's split partials, in order, scaled and rounded once
//   fa_bwd_dq_varlen_kernel           one workgroup per (sequence, head, 128-row Q block of max_seqlen)
// A workgroup whose block starts at or beyond its sequence's length returns at once (before any barrier).  Rows of a tile,
// and resident K / V or Q / dO rows, beyond the sequence's end are fetched from the sequence's LAST row (never from another
// sequence or from beyond total_tokens) and their p is exactly 0: under the causal mask by the dense kernels' select
// (key >= len or query >= len joins key > query); without the mask by starting the row's S at -inf, so that exp2 gives 0 --
// a select behind exp2 would keep hipcc from fusing p * dP with its fp16 rounding as it does in the plain dense kernels, and
// the bits would differ from theirs.  A lane whose own key (dK / dV) or query (dQ) lies beyond the end only feeds its own
// accumulator column, which is never stored.  Nothing a neighbouring sequence holds reaches a result.
// cu_seqlens is the caller's (non-decreasing, [0] = 0, [n_seqs] = total_tokens, lengths <= max_seqlen), but a violation
// cannot fault: seq_range() clamps the first row to [0, total_tokens] and the length to [0, min(max_seqlen, what is left)].
// No float atomics, no waiting between workgroups, no scratch: the same inputs give the same bits.
//
// What the second range adds: K, V, dK, dV are (total_k, n_kv_heads, 128) and sequence i owns key rows cu_seqlens_k[i] ..
// cu_seqlens_k[i + 1] - 1 (on the device too); the dK / dV grid and the partials run over max_seqlen_k and total_k.
//  * The causal mask is bottom-right aligned: query r of a sequence sees keys j <= r + shift, shift = len_k - len_q.  Equal
//    ranges (shift = 0) give the one-range kernels' bits.
//  * A query row that saw no key (len_k = 0, or causal r < len_q - len_k) has lse = -inf and is treated as a row beyond the
//    end (S starts at -inf, delta = 0): dq = 0, nothing of it in dK / dV.
//  * A range of length 0 fetches nothing (the first tile's load is guarded).  A key no query sees (len_q = 0) gets
//    dk = dv = 0, written.
//  * Rows beyond either range's end are fetched from THAT range's last row; both ranges are clamped by seq_range's rule, each
//    against its own total and max_seqlen.
//
// What the window adds (fa_bwd_launch_varlen_qk_window, BwdVarlenWindowArgs, fa_bwd_varlen_window.hip): the
// third form of the same text, selected by the argument type (`if constexpr (WIN)`; QK now reads "not the one-range form"), so
// the other two forms keep their names and their instructions.  The forward's rule: query r at p = r + shift sees the keys
// max(0, p - left) .. min(len_k - 1, p + right), unbounded = 2^30, causal = (right = 0): no CAUSAL instantiation.
//  * dQ: a block with rows r0 .. r1 visits the key tiles of max(0, r0 + shift - left) .. min(len_k - 1, r1 + shift + right), the
//    first prefetch being the first VISITED tile; dK / dV: a block with keys k0 .. k1 sweeps the row tiles of
//    max(0, k0 - shift - right) .. min(len_q - 1, k1 - shift + left).  An empty range sweeps nothing and stores zeros: rows that
//    see no key, and keys no row sees (below every floor, above every ceiling), are WRITTEN as zeros.
//  * The mask is a select on p (key < lo_r, key > hi_r, key >= len_k, query >= len_q) behind the workgroup-uniform `outside`:
//    only a tile that reaches outside some row's window or past either end pays for it, as under `diag` / `edge`.
//  * Positions fit 32 bits: the host refuses max_seqlen on either side above 2^30 - 128.
// Split, partials, reduce, grids and the workspace are the two-range form's.
//
// What soft-capping adds (fa_bwd_launch_varlen_qk_softcap, BwdVarlenSoftcapArgs, fa_bwd_varlen_softcap.hip): the
// fourth form, the window form (`WIN` reads "has a window": a softcap without one arrives with left = right = 2^30) plus
// `if constexpr (CAP)`.  The forward's logit of a seen key is softcap tanh(s / softcap), s = q . k / sqrt(d).  The other forms start
// the S accumulator at -lse sqrt(d) so that exp2(c S) is P at once; a tanh in between forbids that, so here S starts at 0,
// t = tanh(S / A) with A = softcap sqrt(d), p = exp2(c A t - lse log2(e)) (a dead row's -inf gives p = 0, never inf - inf), and
// dS = p (dP - delta) (1 - t^2).  t lives in S's registers until p replaces it; the masks behind are the window form's.
//
// What attention sinks add (fa_bwd_launch_varlen_qk_sinks, BwdVarlenSinksArgs, fa_bwd_varlen_sinks.hip): no form of
// these kernels at all.  Head h's sink is one more logit z = sinks[h] in the softmax's denominator with a zero value vector.  With
// the forward's lse (which includes the sink) P = exp(S - lse) sums to less than 1 per row, delta = rowsum(dO o O) is unchanged
// (the sink's value is 0) and dS = P o (dP - delta) stands: dQ, dK, dV are what the WINDOW form computes from that lse, so the
// sink backward runs fa_bwd_varlen_window.hip's kernels as they are (no window: left = right = 2^30) and adds one reduction,
// dsinks[h] = - sum_rows exp(z - lse) delta (fa_bwd_dsinks_varlen_kernel, in that unit).
// Why the window form and not the unwindowed ones: a row that sees no key now has a FINITE lse (= z), so it is not `dead` in
// load() / lse_q above -- its S starts at -z sqrt(d) like any live row's and exp2 gives some p > 0, possibly +inf.  The unwindowed
// forms would let that p through (their only guard for such a row is S = -inf from lse == -inf).  The window form masks by a
// SELECT on p behind `outside`, and `outside` is true on every tile a dead row appears in:
//  * a row r is dead iff len_k = 0 (no dK / dV workgroup gets past its first test, dQ sweeps no tile) or r + shift + right < 0;
//  * dK / dV: a swept tile `it` that holds r has it * 64 <= r, so it * 64 + shift + right < 0 <= kb * 128 + 127: the last term of
//    `outside`; dQ: a block qb that holds r has qb * 128 <= r, so qb * 128 + shift + right < 0 <= kt * 64 + 63: the last term
//    of `outside` there;
//  * the select's `key > query + shift + right` holds for every key >= 0, so p = 0 exactly (a select, so even p = +inf goes), dS = 0 *
//    (dP - delta) with both finite: dq = 0 for that row and nothing of it in dK / dV.  delta of such a row is 0 (o = 0), so it adds
//    exactly 0 to dsinks as well.
// A head with z = -inf has the lse of the call without sinks, -inf on its dead rows: the `dead` path as ever.
#pragma once
#include <type_traits>

#include "fa_bwd_kernel.hpp"

namespace fa {

struct BwdVarlenArgs {
    const uint16_t *q, *k, *v;        // q_* / kv_* strides
    const uint16_t *o, *dout;         // out_* strides
    const float *lse;                 // (n_heads, total_tokens), contiguous
    float *delta;                     // workspace: (n_heads, total_tokens)
    uint16_t *dq, *dk, *dv;           // dq: out_* strides; dk, dv: dkv_*
    const int32_t *cu_seqlens;        // n_seqs + 1 entries
    float *part;                      // split > 1: (n_kv_heads * split, total_tokens, 2, 128) fp32 dK^T | dV^T, unscaled
    int64_t q_ss, q_hs;               // elements
    int64_t out_ss, out_hs;
    int64_t kv_ss, kv_hs;
    int64_t dkv_ss, dkv_hs;
    int32_t n_seqs, total_tokens, max_seqlen, n_heads;
    int32_t group, split;             // query heads per K / V head; workgroups per (K / V head, key block), divides group
    int32_t n_blocks;                 // ceil(max_seqlen / 128): blocks of the grid per (sequence, head)
};

struct BwdVarlenQKArgs {
    const uint16_t *q, *k, *v;        // q_* / kv_* strides
    const uint16_t *o, *dout;         // out_* strides
    const float *lse;                 // (n_heads, total_tokens), contiguous
    float *delta;                     // workspace: (n_heads, total_tokens)
    uint16_t *dq, *dk, *dv;           // dq: out_* strides; dk, dv: dkv_*
    const int32_t *cu_seqlens;        // n_seqs + 1 entries: the query rows
    const int32_t *cu_seqlens_k;      // n_seqs + 1 entries: the key rows
    float *part;                      // split > 1: (n_kv_heads * split, total_k, 2, 128) fp32 dK^T | dV^T, unscaled
    int64_t q_ss, q_hs;               // elements
    int64_t out_ss, out_hs;
    int64_t kv_ss, kv_hs;
    int64_t dkv_ss, dkv_hs;
    int32_t n_seqs, total_tokens, max_seqlen, n_heads;   // total_tokens, max_seqlen: the query side
    int32_t total_k, max_seqlen_k;
    int32_t group, split;             // query heads per K / V head; workgroups per (K / V head, key block), divides group
    int32_t n_blocks, n_blocks_k;     // ceil(max_seqlen / 128), ceil(max_seqlen_k / 128): blocks of the grids
};

// ... under a sliding window (fa_bwd_launch_varlen_qk_window): the two ranges' fields and (left, right), the keys a row sees
// below and above its position; unbounded arrives as 2^30, causal as right = 0 (the kernels are instantiated without CAUSAL)
struct BwdVarlenWindowArgs : BwdVarlenQKArgs {
    int32_t left, right;
};

// ... with logit soft-capping (fa_bwd_launch_varlen_qk_softcap): the window's fields (none: left = right = 2^30) and
// A = softcap sqrt(d), 1 / A, which the host computes in double and rounds once
struct BwdVarlenSoftcapArgs : BwdVarlenWindowArgs {
    float cap_a, cap_inv_a;
};

// ... with attention sinks (fa_bwd_launch_varlen_qk_sinks): the window form's arguments, as its kernels take them, and what the
// sinks' own gradient reads and writes
struct BwdVarlenSinksArgs {
    BwdVarlenWindowArgs w;
    const float *sinks;   // (n_heads) fp32
    float *dsinks;        // (n_heads) fp32, written
};

namespace bwd {

// sequence -> first row and length, clamped so that every row0 + i, 0 <= i < len, is a row of the tensors
FA_DEV void seq_range(const BwdVarlenArgs &a, int seq, int &row0, int &len) {
    const int64_t lo = a.cu_seqlens[seq], hi = a.cu_seqlens[seq + 1];
    const int64_t total = a.total_tokens;
    const int64_t r0 = lo < 0 ? 0 : (lo > total ? total : lo);
    int64_t n = hi - r0;
    const int64_t cap = total - r0 < a.max_seqlen ? total - r0 : a.max_seqlen;
    n = n < 0 ? 0 : (n > cap ? cap : n);
    row0 = (int)r0;
    len = (int)n;
}

// ... of one of two ranges, by the same rule against that side's total and max_seqlen
FA_DEV void seq_range_of(const int32_t *cu, int64_t total, int64_t max_len, int seq, int &row0, int &len) {
    const int64_t lo = cu[seq], hi = cu[seq + 1];
    const int64_t r0 = lo < 0 ? 0 : (lo > total ? total : lo);
    int64_t n = hi - r0;
    const int64_t cap = total - r0 < max_len ? total - r0 : max_len;
    n = n < 0 ? 0 : (n > cap ? cap : n);
    row0 = (int)r0;
    len = (int)n;
}
FA_DEV void seq_range_q(const BwdVarlenQKArgs &a, int seq, int &row0, int &len) {
    seq_range_of(a.cu_seqlens, a.total_tokens, a.max_seqlen, seq, row0, len);
}
FA_DEV void seq_range_k(const BwdVarlenQKArgs &a, int seq, int &row0, int &len) {
    seq_range_of(a.cu_seqlens_k, a.total_k, a.max_seqlen_k, seq, row0, len);
}

// the key side's rows and 128-key blocks: the one range's, or the second range's
__host__ __device__ inline int32_t total_k(const BwdVarlenArgs &a) { return a.total_tokens; }
__host__ __device__ inline int32_t total_k(const BwdVarlenQKArgs &a) { return a.total_k; }
__host__ __device__ inline int32_t n_blocks_k(const BwdVarlenArgs &a) { return a.n_blocks; }
__host__ __device__ inline int32_t n_blocks_k(const BwdVarlenQKArgs &a) { return a.n_blocks_k; }

// the 64-row tiles [first, end) that hold rows (or keys) lo .. hi of 0 .. n - 1; none of them: first = end = 0
FA_DEV void window_tiles(int lo, int hi, int n, int &first, int &end) {
    lo = lo > 0 ? lo : 0;
    hi = hi < n - 1 ? hi : n - 1;
    first = hi < lo ? 0 : lo / TROWS;
    end = hi < lo ? 0 : hi / TROWS + 1;
}

// soft-capping: tanh(S / A) of a raw logit S = q . k, as 1 - 2 / (exp2(S k) + 1) with k = 2 log2(e) / A (one v_exp_f32, one
// v_rcp_f32).  exp2 overflowing to +inf gives 1, underflowing to 0 gives -1: no NaN at either end.
FA_DEV float cap_tanh(float s, float k) {
    const float e = __builtin_amdgcn_exp2f(s * k);
    return __builtin_fmaf(__builtin_amdgcn_rcpf(e + 1.0f), -2.0f, 1.0f);
}

// tile_load with the tile's rows clamped to the sequence: row first + r comes from row min(first + r, last)
FA_DEV void tile_load_clamped(TileRegs &t, const uint16_t *seq_rows, int64_t ss, int first, int last, int tid) {
#pragma unroll
    for (int u = 0; u < CHUNKS; ++u) {
        const int c = tid + THREADS * u, ch = c & 15;
        int row = first + (c >> 4);
        row = row < last ? row : last;
        t.v[u] = *(const u32x4 *)(seq_rows + (int64_t)row * ss + ch * 8);
    }
}

}  // namespace bwd

// delta_i = sum_d dO_id O_id per (head, token), 16 lanes per row: fa_bwd_delta_kernel's sum over the packed layout
template <int DT>
__global__ void __launch_bounds__(256) fa_bwd_delta_varlen_kernel(const BwdVarlenArgs a) {
    using E = Elem<DT>;
    const int64_t rows = (int64_t)a.n_heads * a.total_tokens;
    const int64_t row = (int64_t)blockIdx.x * 16 + (threadIdx.x >> 4);
    const int part = threadIdx.x & 15;
    float acc = 0.0f;
    if (row < rows) {
        const int64_t hd = row / a.total_tokens, i = row % a.total_tokens;
        const int64_t off = hd * a.out_hs + i * a.out_ss + part * 8;
        const typename E::vec8 o = *(const typename E::vec8 *)(a.o + off);
        const typename E::vec8 g = *(const typename E::vec8 *)(a.dout + off);
#pragma unroll
        for (int j = 0; j < 8; ++j) acc += (float)o[j] * (float)g[j];
    }
#pragma unroll
    for (int m = 8; m >= 1; m >>= 1) acc += __shfl_xor(acc, m, 16);
    if (row < rows && part == 0) a.delta[row] = acc;
}

// dK, dV of one 128-key block of one K / V head of one sequence, summed over group / split query heads.
// Grid: n_seqs * n_kv_heads * split * n_blocks_k workgroups of 256 threads.  The sweep runs over the Q tiles of len_q; two
// ranges: a block no query sees (len_q = 0) sweeps nothing and stores zeros.
template <class ARGS, int DT, bool CAUSAL>
__global__ void __launch_bounds__(bwd::THREADS, 1) fa_bwd_dkdv_varlen_kernel(const ARGS a) {
    using namespace bwd;
    using E = Elem<DT>;
    using vec8 = typename E::vec8;
    constexpr bool WIN = std::is_base_of_v<BwdVarlenWindowArgs, ARGS>;
    constexpr bool CAP = std::is_same_v<ARGS, BwdVarlenSoftcapArgs>;
    constexpr bool QK = !std::is_same_v<ARGS, BwdVarlenArgs>;
    static_assert(!(WIN && CAUSAL), "the window carries the causal mask as right = 0");
    __shared__ __attribute__((aligned(16))) char img_q[TBYTES];
    __shared__ __attribute__((aligned(16))) char img_do[TBYTES];
    __shared__ __attribute__((aligned(16))) float lse_s[TROWS];   // -lse sqrt(d) of the tile's rows (CAP: -lse log2(e))
    __shared__ __attribute__((aligned(16))) float dl_s[TROWS];    // -delta
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 31, h = lane >> 5;
    int wg, kb;   // wg = (sequence * n_kv_heads + K / V head) * split + part
    block_coords(n_blocks_k(a), wg, kb);
    const int n_kv = a.n_heads / a.group, skv = wg / a.split, seq = skv / n_kv, hk = skv % n_kv, sp = wg % a.split;
    int row0, len, krow0, klen;   // the sequence's query rows and key rows
    if constexpr (QK) {
        seq_range_q(a, seq, row0, len);
        seq_range_k(a, seq, krow0, klen);
    } else {
        seq_range(a, seq, row0, len);
        krow0 = row0;
        klen = len;
    }
    if (kb * KB >= klen) return;   // (workgroup-uniform, before any barrier)
    const int last = len - 1, klast = klen - 1;
    const int shift = QK ? klen - len : 0;   // causal, bottom-right: query r sees keys <= r + shift
    const int n_hq = a.group / a.split;   // query heads of the sweep: hk * group + part * n_hq + 0 .. n_hq - 1
    int hq = hk * a.group + sp * n_hq;
    const uint16_t *q_seq = a.q + (int64_t)row0 * a.q_ss + (int64_t)hq * a.q_hs;
    const uint16_t *do_seq = a.dout + (int64_t)row0 * a.out_ss + (int64_t)hq * a.out_hs;
    const int key = kb * KB + 32 * wave + r;   // this lane's key (the accumulators' column)
    const int key_c = key < klast ? key : klast;
    // K, V of the wave's 32 keys: the B operands of S = Q K^T and dP = dO V^T, resident for the whole sweep
    vec8 Kb[8], Vb[8];
    {
        const int64_t kv_row = (int64_t)(krow0 + key_c) * a.kv_ss + (int64_t)hk * a.kv_hs + 8 * h;
        const uint16_t *kr = a.k + kv_row;
        const uint16_t *vr = a.v + kv_row;
#pragma unroll
        for (int ks = 0; ks < 8; ++ks) {
            Kb[ks] = *(const vec8 *)(kr + 16 * ks);
            Vb[ks] = *(const vec8 *)(vr + 16 * ks);
        }
    }
    const float c = (float)((double)(1.0f / __builtin_sqrtf((float)D)) * 1.4426950408889634074);
    const float lse_scale = CAP ? -1.4426950408889634f : -log2e_over_c();
    // soft-capping: S starts at 0 and p = exp2(c (A t + lse_s)), t = tanh(S / A) -- the constants of cap_tanh and of that fma
    [[maybe_unused]] float cap_k = 0.0f, cap_ca = 0.0f;
    if constexpr (CAP) {
        cap_k = a.cap_inv_a * 2.8853900817779268f;
        cap_ca = c * a.cap_a;
    }
    f32x16 dV[4], dK[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        dV[t] = f32x16{};
        dK[t] = f32x16{};
    }
    // window: key j is seen by rows j - shift - right .. j - shift + left, so the block's keys (up to the sequence's last) by the
    // tiles win_it0 .. win_end - 1
    [[maybe_unused]] int win_it0 = 0, win_end = 0;
    if constexpr (WIN) window_tiles(kb * KB - shift - a.right, (kb * KB + KB - 1 < klast ? kb * KB + KB - 1 : klast) - shift + a.left, len, win_it0, win_end);
    const int n_it = WIN ? win_end : (len + TROWS - 1) / TROWS;
    // causal: the Q tiles from the diagonal on (one range: it0 * 64 = kb * 128 < len), that is from the first one that can see
    // the block (two ranges; it0 >= n_it: no query sees it)
    int it0 = 0;
    if constexpr (CAUSAL && QK) it0 = (kb * KB - shift > 0 ? kb * KB - shift : 0) / TROWS;
    else if constexpr (CAUSAL) it0 = kb * (KB / TROWS);
    else if constexpr (WIN) it0 = win_it0;
    const float *lse_h = a.lse + (int64_t)hq * a.total_tokens + row0;
    const float *dl_h = a.delta + (int64_t)hq * a.total_tokens + row0;
    TileRegs tq, tdo;
    float lse_r = 0.0f, dl_r = 0.0f;
    auto load = [&](int it) {
        tile_load_clamped(tq, q_seq, a.q_ss, it * TROWS, last, tid);
        tile_load_clamped(tdo, do_seq, a.out_ss, it * TROWS, last, tid);
        if (tid < TROWS) {
            const int row = it * TROWS + tid;
            const bool in = row < len;
            if constexpr (QK) {
                // (a row that saw no key has lse = -inf: a row beyond the end, or lse * lse_scale = +inf would reach dK / dV as NaN)
                const float lse_v = in ? lse_h[in ? row : 0] : -__builtin_inff();
                const bool live = in && lse_v != -__builtin_inff();
                lse_r = live ? lse_v * lse_scale : -__builtin_inff();   // S = -inf, p = exp2(-inf) = 0
                dl_r = live ? -dl_h[in ? row : 0] : 0.0f;
            } else {
                lse_r = in ? lse_h[in ? row : 0] * lse_scale : -__builtin_inff();   // S = -inf, p = exp2(-inf) = 0
                dl_r = in ? -dl_h[in ? row : 0] : 0.0f;
            }
        }
    };
    if (!QK || it0 < n_it) load(it0);   // (two ranges: len_q = 0 has no row to fetch)
    const bool key_edge = kb * KB + KB > klen;   // a block that holds keys beyond the sequence
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
                ++hq;
                q_seq += a.q_hs;
                do_seq += a.out_hs;
                lse_h += a.total_tokens;
                dl_h += a.total_tokens;
                load(it0);
            }
            const bool diag = CAUSAL && it * TROWS + shift < kb * KB + KB;   // a tile that holds queries before some key of the block
            const bool edge = key_edge || it * TROWS + TROWS > len;  // ... or rows / keys beyond the sequence
            // window: ... or a tile that reaches outside some row's window: its last row's floor above the block's first key, or its
            // first row's ceiling below the block's last
            [[maybe_unused]] bool outside = false;
            if constexpr (WIN) outside = edge || it * TROWS + TROWS - 1 + shift - a.left > kb * KB || it * TROWS + shift + a.right < kb * KB + KB - 1;
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
                        S[4 * gg + e] = CAP ? 0.0f : l4[e];   // (CAP: the row's term joins behind the tanh)
                        dP[4 * gg + e] = d4[e];
                    }
                }
#pragma unroll
                for (int ks = 0; ks < 8; ++ks) S = E::mfma(row_read<vec8>(img_q, rb, ks, lane), Kb[ks], S);
#pragma unroll
                for (int ks = 0; ks < 8; ++ks) dP = E::mfma(row_read<vec8>(img_do, rb, ks, lane), Vb[ks], dP);
#pragma unroll
                for (int i = 0; i < 16; ++i) {
                    float p;
                    [[maybe_unused]] float dt = 1.0f;   // CAP: d tanh = 1 - t^2
                    if constexpr (CAP) {   // (a dead row's lse_s = -inf: p = exp2(-inf) = 0, no inf - inf)
                        const float t = cap_tanh(S[i], cap_k);
                        p = __builtin_amdgcn_exp2f(__builtin_fmaf(t, cap_ca, lse_s[rb + (i & 3) + 8 * (i >> 2) + 4 * h]));
                        dt = __builtin_fmaf(-t, t, 1.0f);
                    } else {
                        p = __builtin_amdgcn_exp2f(c * S[i]);
                    }
                    const int query = it * TROWS + rb + (i & 3) + 8 * (i >> 2) + 4 * h;
                    if constexpr (CAUSAL) {   // (plain: rows beyond the end have S = -inf, see load())
                        if (diag) p = key > query + shift ? 0.0f : p;
                        if (edge) p = (key >= klen || query >= len) ? 0.0f : p;
                    }
                    if constexpr (WIN) {
                        if (outside) p = (key < query + shift - a.left || key > query + shift + a.right || key >= klen || query >= len) ? 0.0f : p;
                    }
                    S[i] = p;                 // P
                    dP[i] = p * dP[i];        // dS = P (dP - delta)
                    if constexpr (CAP) dP[i] *= dt;   // ... (1 - t^2)
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
    if (key >= klen) return;   // (behind the last barrier and the last transposed read)
    // dK^T / dV^T: column = this lane's key, rows d = 32 t + 8 gg + 4 h + 0 .. 3
    if (a.split > 1) {   // the fp32 partials, unscaled: fa_bwd_dkdv_reduce_varlen_kernel rounds their sum
        float *pk = a.part + (((int64_t)hk * a.split + sp) * total_k(a) + krow0 + key) * (2 * D) + 4 * h;
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
    const int64_t dkv_row = (int64_t)(krow0 + key) * a.dkv_ss + (int64_t)hk * a.dkv_hs + 4 * h;
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

// split > 1: dK, dV of one (K / V head, key token) row = the sum of its `split` partials in order, scaled and rounded once.
// One thread per 8 elements of a dK or dV row.  Grid: n_kv_heads * total_k * 2 * 16 / 256 workgroups of 256 threads.
// (every key row belongs to a sequence -- cu_seqlens[0] = 0, [n_seqs] = total, on the key side -- so every partial row was written)
template <class ARGS, int DT>
__global__ void __launch_bounds__(256) fa_bwd_dkdv_reduce_varlen_kernel(const ARGS a) {
    using namespace bwd;
    const int n_kv = a.n_heads / a.group;
    const int64_t n = (int64_t)n_kv * total_k(a) * 2 * (D / 8);
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= n) return;
    const int c8 = (int)(idx % (D / 8)), which = (int)((idx / (D / 8)) & 1);   // 8-element chunk; 0 dK, 1 dV
    const int64_t row = idx / (2 * (D / 8));   // hk * total_k + token
    const int64_t hk = row / total_k(a), tok = row % total_k(a);
    const int64_t plane = (int64_t)total_k(a) * 2 * D;   // floats per partial
    const float *src = a.part + (hk * a.split * total_k(a) + tok) * (2 * D) + which * D + 8 * c8;
    f32x4 lo = *(const f32x4 *)src, hi = *(const f32x4 *)(src + 4);
    for (int s = 1; s < a.split; ++s) {
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
    uint16_t *dst = (which ? a.dv : a.dk) + hk * a.dkv_hs + tok * a.dkv_ss + 8 * c8;
    *(typename Elem<DT>::vec8 *)dst = Elem<DT>::pack8(f);
}

// dQ of one 128-row Q block of one sequence, K / V of head h / group.  Grid: n_seqs * n_heads * n_blocks workgroups of 256 threads.
// The sweep runs over the key tiles of len_k; two ranges: a block that sees no key (len_k = 0, or causal rows above the shifted
// diagonal) sweeps nothing and stores zeros.
template <class ARGS, int DT, bool CAUSAL>
__global__ void __launch_bounds__(bwd::THREADS, 1) fa_bwd_dq_varlen_kernel(const ARGS a) {
    using namespace bwd;
    using E = Elem<DT>;
    using vec8 = typename E::vec8;
    constexpr bool WIN = std::is_base_of_v<BwdVarlenWindowArgs, ARGS>;
    constexpr bool CAP = std::is_same_v<ARGS, BwdVarlenSoftcapArgs>;
    constexpr bool QK = !std::is_same_v<ARGS, BwdVarlenArgs>;
    static_assert(!(WIN && CAUSAL), "the window carries the causal mask as right = 0");
    __shared__ __attribute__((aligned(16))) char img_k[TBYTES];
    __shared__ __attribute__((aligned(16))) char img_v[TBYTES];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 31, h = lane >> 5;
    int sh, qb;   // sh = sequence * n_heads + head
    block_coords(a.n_blocks, sh, qb);
    if (CAUSAL) qb = a.n_blocks - 1 - qb;   // the longest sweeps first
    const int seq = sh / a.n_heads, hq = sh % a.n_heads;
    int row0, len, krow0, klen;   // the sequence's query rows and key rows
    if constexpr (QK) {
        seq_range_q(a, seq, row0, len);
        seq_range_k(a, seq, krow0, klen);
    } else {
        seq_range(a, seq, row0, len);
        krow0 = row0;
        klen = len;
    }
    if (qb * KB >= len) return;   // (workgroup-uniform, before any barrier)
    const int last = len - 1, klast = klen - 1;
    const int shift = QK ? klen - len : 0;   // causal, bottom-right: query r sees keys <= r + shift
    const uint16_t *k_seq = a.k + (int64_t)krow0 * a.kv_ss + (int64_t)(hq / a.group) * a.kv_hs;
    const uint16_t *v_seq = a.v + (int64_t)krow0 * a.kv_ss + (int64_t)(hq / a.group) * a.kv_hs;
    const int query = qb * KB + 32 * wave + r;   // this lane's query (the accumulators' column)
    const int query_c = query < last ? query : last;
    // Q, dO of the wave's 32 rows: the B operands of S^T = K Q^T and dP^T = V dO^T
    vec8 Qb[8], Ob[8];
    {
        const uint16_t *qr = a.q + (int64_t)(row0 + query_c) * a.q_ss + (int64_t)hq * a.q_hs + 8 * h;
        const uint16_t *gr = a.dout + (int64_t)(row0 + query_c) * a.out_ss + (int64_t)hq * a.out_hs + 8 * h;
#pragma unroll
        for (int ks = 0; ks < 8; ++ks) {
            Qb[ks] = *(const vec8 *)(qr + 16 * ks);
            Ob[ks] = *(const vec8 *)(gr + 16 * ks);
        }
    }
    const float c = (float)((double)(1.0f / __builtin_sqrtf((float)D)) * 1.4426950408889634074);
    const int64_t stat = (int64_t)hq * a.total_tokens + row0 + query_c;
    float lse_q, dl_q;
    if constexpr (QK) {
        // (a row that saw no key has lse = -inf: its S starts at -inf, p = exp2(-inf) = 0, rather than at lse * scale = +inf)
        const float lse_v = a.lse[stat];
        const bool dead = lse_v == -__builtin_inff();
        lse_q = query < len ? (dead ? -__builtin_inff() : lse_v * (CAP ? -1.4426950408889634f : -log2e_over_c())) : 0.0f;
        dl_q = query < len && !dead ? -a.delta[stat] : 0.0f;
    } else {
        lse_q = query < len ? a.lse[stat] * -log2e_over_c() : 0.0f;
        dl_q = query < len ? -a.delta[stat] : 0.0f;
    }
    [[maybe_unused]] float cap_k = 0.0f, cap_ca = 0.0f;   // soft-capping: as in the dK / dV kernel
    if constexpr (CAP) {
        cap_k = a.cap_inv_a * 2.8853900817779268f;
        cap_ca = c * a.cap_a;
    }
    f32x16 dQ[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) dQ[t] = f32x16{};
    const int n_all = (klen + TROWS - 1) / TROWS;
    // causal: cut at the block's last row's diagonal, (qb + 1) * 128 - 1 + shift; two ranges: no tile when that lies before key 0
    int n_diag = (qb + 1) * (KB / TROWS);
    if constexpr (QK) n_diag = (qb + 1) * KB + shift > 0 ? ((qb + 1) * KB + shift + TROWS - 1) / TROWS : 0;
    // window: the block's rows (up to the sequence's last) see the keys from its first row's floor to its last row's ceiling: the
    // tiles kt0 .. win_end - 1
    [[maybe_unused]] int kt0 = 0, win_end = 0;
    if constexpr (WIN) window_tiles(qb * KB + shift - a.left, (qb * KB + KB - 1 < last ? qb * KB + KB - 1 : last) + shift + a.right, klen, kt0, win_end);
    const int n_kt = WIN ? win_end : (CAUSAL && n_diag < n_all ? n_diag : n_all);
    TileRegs tk, tv;
    auto load = [&](int kt) {
        tile_load_clamped(tk, k_seq, a.kv_ss, kt * TROWS, klast, tid);
        tile_load_clamped(tv, v_seq, a.kv_ss, kt * TROWS, klast, tid);
    };
    if (!QK || n_kt > 0) load(kt0);   // (two ranges: len_k = 0 has no row to fetch; window: the first VISITED tile)
    const bool query_edge = qb * KB + KB > len;   // a block that holds rows beyond the sequence
    for (int kt = kt0; kt < n_kt; ++kt) {
        __syncthreads();
        tile_store(img_k, tk, tid);
        tile_store(img_v, tv, tid);
        __syncthreads();
        if (kt + 1 < n_kt) load(kt + 1);
        const bool diag = CAUSAL && kt * TROWS + TROWS > qb * KB + shift;   // a tile that holds keys after some query of the block
        const bool edge = query_edge || kt * TROWS + TROWS > klen;   // ... or rows / keys beyond the sequence
        // window: ... or a tile that reaches outside some row's window: its first key below the block's last row's floor, or its
        // last key above the block's first row's ceiling
        [[maybe_unused]] bool outside = false;
        if constexpr (WIN) outside = edge || kt * TROWS < qb * KB + KB - 1 + shift - a.left || kt * TROWS + TROWS - 1 > qb * KB + shift + a.right;
#pragma unroll
        for (int mt = 0; mt < TROWS / 32; ++mt) {
            const int rb = 32 * mt;
            f32x16 S, dP;
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                S[i] = CAP ? 0.0f : lse_q;
                dP[i] = dl_q;
                if (!CAUSAL && !WIN && edge) {   // keys beyond the end: S = -inf, p = exp2(-inf) = 0
                    const int key = kt * TROWS + rb + (i & 3) + 8 * (i >> 2) + 4 * h;
                    S[i] = key >= klen ? -__builtin_inff() : lse_q;
                }
            }
#pragma unroll
            for (int ks = 0; ks < 8; ++ks) S = E::mfma(row_read<vec8>(img_k, rb, ks, lane), Qb[ks], S);
#pragma unroll
            for (int ks = 0; ks < 8; ++ks) dP = E::mfma(row_read<vec8>(img_v, rb, ks, lane), Ob[ks], dP);
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                float p;
                [[maybe_unused]] float dt = 1.0f;   // CAP: d tanh = 1 - t^2
                if constexpr (CAP) {   // (a dead row's lse_q = -inf: p = exp2(-inf) = 0, no inf - inf)
                    const float t = cap_tanh(S[i], cap_k);
                    p = __builtin_amdgcn_exp2f(__builtin_fmaf(t, cap_ca, lse_q));
                    dt = __builtin_fmaf(-t, t, 1.0f);
                } else {
                    p = __builtin_amdgcn_exp2f(c * S[i]);
                }
                const int key = kt * TROWS + rb + (i & 3) + 8 * (i >> 2) + 4 * h;
                if constexpr (CAUSAL) {
                    if (diag) p = key > query + shift ? 0.0f : p;
                    if (edge) p = (key >= klen || query >= len) ? 0.0f : p;
                }
                if constexpr (WIN) {
                    if (outside) p = (key < query + shift - a.left || key > query + shift + a.right || key >= klen || query >= len) ? 0.0f : p;
                }
                dP[i] = p * dP[i];        // dS^T
                if constexpr (CAP) dP[i] *= dt;   // ... (1 - t^2)
            }
#pragma unroll
            for (int s = 0; s < 2; ++s) {
                const vec8 db = acc_operand<DT>(dP, s);
#pragma unroll
                for (int t = 0; t < 4; ++t) dQ[t] = E::mfma(tr_read<vec8>(img_k, rb, s, t, lane), db, dQ[t]);
            }
        }
    }
    if (query >= len) return;
    const float inv_sqrt_d = 1.0f / __builtin_sqrtf((float)D);
    uint16_t *dq = a.dq + (int64_t)(row0 + query) * a.out_ss + (int64_t)hq * a.out_hs + 4 * h;
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int gg = 0; gg < 4; ++gg) store4<DT>(dq + 32 * t + 8 * gg, dQ[t], gg, inv_sqrt_d);
}

// fa_bwd_varlen.hip: fa_bwd_delta_varlen_kernel as that unit builds it, over the (n_heads, total_tokens) rows of o and dout
// (delta = sum_d dO O knows neither of a second range, nor of a window, nor of a cap)
hipError_t bwd_varlen_delta_enqueue(const BwdVarlenArgs &a, int dtype, hipStream_t s);

// One backward of a two-range form (ARGS: BwdVarlenQKArgs, BwdVarlenWindowArgs, BwdVarlenSoftcapArgs), three or four launches on
// one stream; the unit that calls this builds that form's kernels.  Delta over total_q, dK / dV (one workgroup per sequence,
// K / V head, split part and key block of max_seqlen_k), their fixed-order sum over total_k when split > 1, dQ (per Q block of
// max_seqlen_q).  The grids depend on the host's arguments alone: neither cu_seqlens nor a window sizes one (a workgroup whose
// window reaches no row or no key returns its zeros at once).
template <class ARGS, int DT, bool CAUSAL>
static hipError_t bwd_varlen_enqueue_any(const ARGS &a, hipStream_t s) {
    BwdVarlenArgs d = {};   // what the delta kernel reads
    d.o = a.o;
    d.dout = a.dout;
    d.delta = a.delta;
    d.out_ss = a.out_ss;
    d.out_hs = a.out_hs;
    d.n_heads = a.n_heads;
    d.total_tokens = a.total_tokens;
    hipError_t rc = hipSuccess;
    if (a.total_tokens > 0) {   // (no query rows: only the zeros of dK / dV are left to write)
        rc = bwd_varlen_delta_enqueue(d, DT, s);
        if (rc != hipSuccess) return rc;
    }
    void *params[] = {(void *)&a};
    const int64_t n_kv = a.n_heads / a.group;
    const dim3 block(bwd::THREADS);
    if (a.total_k > 0) {   // (no key rows: nothing to write, and the dQ kernel stores zeros)
        rc = hipLaunchKernel((const void *)&fa_bwd_dkdv_varlen_kernel<ARGS, DT, CAUSAL>,
                             dim3((unsigned)((int64_t)a.n_seqs * n_kv * a.split * a.n_blocks_k)), block, params, 0, s);
        if (rc != hipSuccess) return rc;
        if (a.split > 1) {
            const int64_t n = n_kv * a.total_k * 2 * (bwd::D / 8);
            rc = hipLaunchKernel((const void *)&fa_bwd_dkdv_reduce_varlen_kernel<ARGS, DT>, dim3((unsigned)((n + 255) / 256)), dim3(256), params, 0, s);
            if (rc != hipSuccess) return rc;
        }
    }
    if (a.total_tokens == 0) return hipSuccess;
    return hipLaunchKernel((const void *)&fa_bwd_dq_varlen_kernel<ARGS, DT, CAUSAL>, dim3((unsigned)((int64_t)a.n_seqs * a.n_heads * a.n_blocks)),
                           block, params, 0, s);
}

}  // namespace fa
