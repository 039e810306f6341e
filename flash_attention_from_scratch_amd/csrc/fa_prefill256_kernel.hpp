// fa_prefill256_kernel.hpp -- prefill attention at d_head = 256 for gfx950: many packed query rows per sequence
// against keys from a packed tensor or a 16-bit K / V cache (contiguous or paged), with a sliding window and optional logit
// soft-capping (the Gemma-2 / Gemma-3 shapes); forward only, o and lse.  A text of its own beside fa_prefill64_kernel.hpp: at 256
// O^T of 32 rows is 128 accumulator registers a lane and the resident Q^T 64, so a wave takes 32 rows (not 64) and a SIMD one wave
// (not two), and a 64-key tile is 64 KiB of K and V, so the LDS ring is counted in whole tiles of dynamic LDS, not in a static 48 KiB.
//
//  * Grid n_seqs * ceil(max_seqlen_q / 128) * n_heads, host-visible numbers only, the head the fastest index: the heads of one K / V
//    group are neighbouring workgroups and find each other's K / V tiles in L2.  Workgroup (b, qb, h) owns rows 128 qb .. of sequence
//    b, 4 waves of 32 rows, one wave per SIMD (__launch_bounds__(256, 1): 512 registers a lane).  A workgroup whose block starts at or
//    beyond len_q returns before any barrier or DMA.  Per lane: O^T 8 x 16 = 128, S^T 16 per 32 keys, P 8 per 32 keys, Q^T 16 x 4 = 64.
//  * Both products are transposed, v_mfma_f32_32x32x16_{bf16,f16}; lane (r31 = lane & 31, hi = lane >> 5) owns query row r31 of its
//    wave, so m, l and the rescale are lane-local and a row maximum costs one v_permlane32_swap:
//        S^T = K Q^T     NT = TILE / 32 key tiles x 16 k-steps; A = K rows by ds_read_b128 from the K image, B = Q^T resident (row r,
//                        d 16 ks + 8 hi .. + 7).  C: lane holds keys 32 nt + (j & 3) + 8 (j >> 2) + 4 hi, j = 0 .. 15
//        O^T = V^T P^T   eight 32-d tiles x TILE / 16 16-key k-steps; B = P^T, the S^T registers 8 half .. 8 half + 7 of key tile nt packed
//                        in place, A = V^T by two ds_read_b64_tr_b16 that pick the same keys (4 hi + 0 .. 3 and 8 + 4 hi + 0 .. 3 of
//                        the 16): a contraction index may be permuted when both operands agree.
//    Every operand is read one step ahead of its MFMAs and the scheduler is held to the phases (sched_barrier), as at 64.
//  * TILE, the keys of one LDS stage, is a parameter of this text, and so is the ring: (64 keys, 2 stages, requested one tile ahead:
//    128 KiB) or (32 keys, 3 stages, requested two ahead: 96 KiB).  Both are instantiated (DESIGN.md 10.21 has them side by side);
//    TILE_SHIPPED names the one a launch takes, FA_PREFILL256_TILE=64 or =32 in the environment names one outright.  Transport is
//    global -> LDS by DMA (global_load_lds_dwordx4, 1 KiB per wave instruction, TILE / 4 pieces per wave and tile: half K, half V).
//    The waits are counted: before the barrier of tile i a wave waits until at most the pieces of tile i + 1 are in flight (two
//    ahead; one ahead, or the walk's last tile: vmcnt(0)); the one barrier per tile publishes tile i and frees tile i - 1's stage,
//    which the next request then takes.
//  * The DMA writes LDS lane-linearly, so both images are made by permuting the lanes' SOURCE addresses.  Rows are 512 bytes here:
//      K image [TILE keys][512 bytes], the 16-byte chunk index (0 .. 31) XOR (key & 15).  A ds_read_b128 serves 16 lanes at a time
//        (256 bytes, every bank once at best); they ask for one chunk c of 16 consecutive keys.  Unswizzled, key k's chunk lies at
//        byte (512 k + 16 c) mod 256 = 16 c mod 256: ONE place for sixteen lanes, a 16-way conflict.  With the XOR the sixteen keys
//        take the sixteen values of (c ^ k) & 15, sixteen different 16-byte slots of the 256 -- every bank once.  (Bit 4 of c is left
//        alone: it moves all sixteen lanes by the same 256 bytes.)  A piece of K is 2 whole rows (lane: key 2 i + lane / 32, the chunk
//        its slot holds): global reads of 512 contiguous bytes.
//      V image [TILE / 8 key groups][8 d tiles][8 keys][32 d]: 512-byte subtiles.  A ds_read_b64_tr_b16 wave instruction (lane 16 g +
//        4 q + p: key 4 (g >> 1) + q, d 16 (g & 1) + 4 p .. + 3 of a subtile) reads 8 keys x 64 bytes = the 512 contiguous bytes of
//        one subtile: every bank twice, which is what 512 bytes cost.  All reads of a tile are one base and immediate offsets.  A
//        piece of V is two neighbouring subtiles of one key group (lane: d tile 2 dp + lane / 32, key (lane & 31) / 4, 16 bytes at
//        d 8 (lane & 3)): global reads of 128 contiguous bytes per key.
//  * Row r of a sequence sits at p = r + (len_k - len_q) and sees keys lo_r = max(0, p - left) .. hi_r = min(len_k - 1, p + right),
//    -1 unbounded, causal arriving as right = 0.  Both grow with r: the workgroup (rows r0 .. r1) visits tiles lo_r0 / TILE ..
//    hi_r1 / TILE in ascending order and nothing else, a wave computes only the tiles lo_w0 / TILE .. hi_w1 / TILE of its own rows,
//    and a tile runs the mask code (lo <= key < hi as one unsigned compare per element) only if it reaches above hi of the wave's
//    first row, below lo of its last, or across len_k; every other tile takes the unmasked visit.
//  * Softmax: the reference arithmetic -- running maximum m with rescale, fp32, p = exp2(s c - m c), c = log2(e) / sqrt(256) rounded
//    once from the double product; l is summed from the fp32 p, the lane pair's halves added in the epilogue.
//  * Soft-capping is a template flag, CAP: the uncapped kernels hold none of its instructions.  Every S accumulator goes through
//    A tanh(S / A) = A - 2 A / (exp2(S cap_k) + 1), A = softcap * 16, cap_k = 2 log2(e) / A -- fa_decode256_kernel.hpp's form --
//    right behind the S^T MFMAs and in front of every mask: a masked key stays -inf, and lse is taken over the capped logits.
//  * Fetch contract (include/fa_hip.h, the d128 and d64 forms'): lengths clamped as fa_varlen_layout / fa_kvcache_layout say; a key
//    below the workgroup's floor lo_r0 is FETCHED from key lo_r0, one at or beyond len_k from key len_k - 1 (both lie in the tile
//    that asks), and masked; block_table entries are clamped to [0, num_pages); page_size % 64 == 0, so a tile lies in one page; one
//    table lookup per page crossed (requested a page ahead of its use), none below the floor tile's page or above the top tile's.
//    Positions are 32-bit (the host bounds lengths by 2^30 - 128), every element offset is formed in 64 bits, a lane's byte offset
//    inside a tile (< 64 rows) in 32.
//  * A row without keys: o = 0, lse = -inf.  The packed and the cache form differ only in how a tile's base address is found: the
//    same bits on the same keys.  Fixed walk order, no atomics, no workspace.
#pragma once
#include "fa_fwd_kernel.hpp"

namespace fa {

struct Prefill256Args {
    const uint16_t *q, *k, *v;
    uint16_t *o;
    float *lse;                    // (n_heads, total_q)
    const int32_t *cu_q;           // n_seqs + 1 row offsets of q / o / lse
    const int32_t *cu_k;           // packed keys: n_seqs + 1 row offsets of k / v
    const int32_t *cache_seqlens;  // cache: (n_seqs) valid keys
    const int32_t *block_table;    // paged cache: (n_seqs, bt_stride); null: contiguous
    int64_t q_ss, q_hs;            // q's and o's token and head strides (elements)
    int64_t kv_ss, kv_hs;          // k's and v's
    int64_t page_stride;           // cache: elements between pages (contiguous: between batch entries)
    int32_t n_heads, group, n_q_blocks;
    int32_t total_q, max_seqlen_q;
    int32_t total_k, max_seqlen_k;   // packed keys
    int32_t bt_stride, num_pages, tiles_per_page, max_len;   // cache; tiles_per_page counts 64 keys (contiguous: it covers the whole entry)
    int32_t left, right;           // -1 = unbounded (causal: right = 0)
    float cap_a, cap_inv_a;        // A = softcap * sqrt(256) and 1 / A (the host rounds each once); read by the capped kernels only
};

namespace prefill256 {
constexpr int D = 256, NWAVES = 4, THREADS = NWAVES * 64, RW = 32, R = NWAVES * RW, ROW_BYTES = D * 2;
constexpr int TILE_SHIPPED = 64;   // keys per LDS stage: 64 (two stages) or 32 (three), measured side by side
constexpr int stages(int tile) { return tile == 64 ? 2 : 3; }
constexpr int lds_bytes(int tile) { return stages(tile) * 2 * tile * ROW_BYTES; }   // K then V per stage: 128 KiB or 96 KiB
}  // namespace prefill256

template <int DT, bool CACHE, bool CAP, int TILE>
__global__ void __launch_bounds__(prefill256::THREADS, 1) fa_prefill256_kernel(const Prefill256Args a) {
    static_assert(TILE == 64 || TILE == 32, "a stage is one 64-key tile or one 32-key tile");
    using E = Elem<DT>;
    using vec8 = typename E::vec8;
    using namespace prefill256;
    constexpr int KS = D / 16, DT32 = D / 32, NT = TILE / 32, SLICES = TILE / 16;
    constexpr int STAGES = stages(TILE), AHEAD = STAGES - 1;
    constexpr int TILE_BYTES = TILE * ROW_BYTES, STAGE_BYTES = 2 * TILE_BYTES;
    constexpr int HALF_PIECES = TILE_BYTES / 1024 / NWAVES, PIECES = 2 * HALF_PIECES;   // DMA pieces per wave and tile
    extern __shared__ __attribute__((aligned(1024))) char smem[];

    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int r31 = lane & 31, hi = lane >> 5;
    const int h = blockIdx.x % a.n_heads, bq = blockIdx.x / a.n_heads;
    const int qb = bq % a.n_q_blocks, b = bq / a.n_q_blocks;

    // the sequence's rows and keys, clamped so that every row derived below is a row of the tensors whatever the device arrays hold
    int64_t q_row0 = a.cu_q[b], q_len64 = a.cu_q[b + 1];
    q_row0 = q_row0 < 0 ? 0 : (q_row0 > a.total_q ? a.total_q : q_row0);
    q_len64 -= q_row0;
    {
        const int64_t cap = a.total_q - q_row0 < a.max_seqlen_q ? a.total_q - q_row0 : a.max_seqlen_q;
        q_len64 = q_len64 < 0 ? 0 : (q_len64 > cap ? cap : q_len64);
    }
    if ((int64_t)qb * R >= q_len64) return;   // (workgroup-uniform; before any barrier or DMA)
    const int len_q = (int)q_len64;
    int64_t k_row0 = 0, k_len64;
    if constexpr (CACHE) {
        k_len64 = a.cache_seqlens[b];
        k_len64 = k_len64 < 0 ? 0 : (k_len64 > a.max_len ? a.max_len : k_len64);
    } else {
        k_row0 = a.cu_k[b];
        k_len64 = a.cu_k[b + 1];
        k_row0 = k_row0 < 0 ? 0 : (k_row0 > a.total_k ? a.total_k : k_row0);
        k_len64 -= k_row0;
        const int64_t cap = a.total_k - k_row0 < a.max_seqlen_k ? a.total_k - k_row0 : a.max_seqlen_k;
        k_len64 = k_len64 < 0 ? 0 : (k_len64 > cap ? cap : k_len64);
    }
    const int len_k = (int)k_len64, shift = len_k - len_q;

    // the window: a row's bounds from its position (lengths <= 2^30 - 128, so p + w_right + 1 and p - w_left stay inside 32 bits)
    constexpr int FAR = (1 << 30) + 64;   // unbounded, or beyond what any length reaches: all one
    const int w_left = a.left < 0 || a.left > FAR ? FAR : a.left;
    const int w_right = a.right < 0 || a.right > FAR ? FAR : a.right;
    auto lo_of = [&](int r) { const int x = r + shift - w_left; return x > 0 ? x : 0; };
    auto hi_of = [&](int r) { const int x = r + shift + w_right; return x < len_k - 1 ? x : len_k - 1; };   // (< lo: the row sees no key)
    const int r0 = qb * R, r1 = (r0 + R < len_q ? r0 + R : len_q) - 1;
    const int wg_lo = lo_of(r0), wg_hi = hi_of(r1);
    const int t_lo = wg_lo / TILE, n_tiles = wg_hi >= wg_lo ? wg_hi / TILE - t_lo + 1 : 0;
    // the wave's own rows w0 .. w1 and the tiles they see (none: a wave past len_q, or rows above every key)
    const int w0 = r0 + wave * RW, w1 = (w0 + RW < len_q ? w0 + RW : len_q) - 1;
    const bool wave_live = w0 < len_q && hi_of(w1) >= lo_of(w0);
    const int wt_lo = wave_live ? lo_of(w0) / TILE : 1, wt_hi = wave_live ? hi_of(w1) / TILE : 0;
    const int plain_lo = w0 < len_q ? lo_of(w1) : 0, plain_hi = w0 < len_q ? hi_of(w0) : -1;   // a tile inside [plain_lo, plain_hi] needs no mask

    const float scale = 1.0f / 16.0f;   // logits, and c: the exponent of exp2
    const float c = (float)((double)scale * 1.4426950408889634074);
    // CAP: S -> A tanh(S / A) = cap_a + cap_m2a / (exp2(S cap_k) + 1)
    [[maybe_unused]] float cap_a = 0.0f, cap_m2a = 0.0f, cap_k = 0.0f;
    if constexpr (CAP) {
        cap_a = a.cap_a;
        cap_m2a = -2.0f * a.cap_a;
        cap_k = a.cap_inv_a * 2.8853900817779268f;   // 2 log2(e) / A
    }
    const float ninf = -__builtin_inff();

    f32x16 O[DT32];
#pragma unroll
    for (int t = 0; t < DT32; ++t)
#pragma unroll
        for (int j = 0; j < 16; ++j) O[t][j] = 0.0f;
    float m = ninf, l = 0.0f;
    int row_lo;
    unsigned row_span;
    {
        const int p = w0 + r31 + shift;   // (a row past len_q: computed, never stored)
        const int lo = p - w_left > 0 ? p - w_left : 0, hi1 = p + w_right + 1 < len_k ? p + w_right + 1 : len_k;
        row_lo = lo;
        row_span = hi1 > lo ? (unsigned)(hi1 - lo) : 0u;
    }

    const int kvh = h / a.group;
    const uint16_t *Kg = a.k + (int64_t)kvh * a.kv_hs, *Vg = a.v + (int64_t)kvh * a.kv_hs;
    const unsigned smem_base = __builtin_amdgcn_readfirstlane(lds_addr(smem));
    const unsigned row_bytes = (unsigned)(a.kv_ss * sizeof(uint16_t));

    // the walk over the key tiles, ascending: tile t's base offset (elements from k / v).  Cache: page and tile-in-page by counters,
    // the page's table entry requested when the walk enters the page before it (a scalar load through the constant address space:
    // nothing writes the table while the kernel runs) -- one lookup per page crossed, none outside [floor page, top page]
    typedef const __attribute__((address_space(4))) int32_t *table_ptr;
    const table_ptr bt_row = (table_ptr)(unsigned long long)(a.block_table + (int64_t)b * a.bt_stride);
    const bool paged = CACHE && a.block_table != nullptr;
    const int tpp = CACHE ? a.tiles_per_page * (64 / TILE) : 1;
    int walk_page = 0, walk_tip = 0, walk_entry = b, walk_next = b, page_hi = 0;
    if (CACHE && n_tiles > 0) {
        walk_page = t_lo / tpp;
        walk_tip = t_lo - walk_page * tpp;
        page_hi = (t_lo + n_tiles - 1) / tpp;
        if (paged) {
            walk_entry = bt_row[walk_page];
            walk_next = walk_page < page_hi ? bt_row[walk_page + 1] : walk_entry;
        }
    }
    // per-lane source offsets of a piece, less the row: K's chunk is swizzled by the IMAGE row's key (2 i + lane / 32: its low four bits
    // are 2 (i & 7) + lane / 32, and i & 7 = (wave + 4 j) & 7), V's is d tile 2 dp + lane / 32 (dp = wave: pieces wave + 4 j are key
    // group j), 16 bytes at d 8 (lane & 3)
    const int k_row = lane >> 5, v_row = (lane & 31) >> 2;
    const unsigned v_col = (unsigned)((2 * wave + (lane >> 5)) * 64 + (lane & 3) * 16);
    int issued = 0;   // tiles requested so far
    auto issue_tile = [&]() {
        const int t = t_lo + issued, stage = issued % STAGES;
        int64_t base;
        if constexpr (CACHE) {
            const int e = walk_entry < 0 ? 0 : (walk_entry >= a.num_pages ? a.num_pages - 1 : walk_entry);
            base = (int64_t)e * a.page_stride + (int64_t)walk_tip * TILE * a.kv_ss;
        } else {
            base = (k_row0 + (int64_t)t * TILE) * a.kv_ss;
        }
        // the tile's rows that may be fetched: [first, last], both inside the tile (the floor tile holds wg_lo, the top tile wg_hi)
        const int key0 = t * TILE;
        const int first = wg_lo > key0 ? wg_lo - key0 : 0, last = len_k - 1 - key0 < TILE - 1 ? len_k - 1 - key0 : TILE - 1;
        const unsigned dst = smem_base + stage * STAGE_BYTES;
#pragma unroll
        for (int j = 0; j < HALF_PIECES; ++j) {
            const int i = wave + NWAVES * j;   // piece i of K: keys 2 i, 2 i + 1; piece i of V: key group j, d tiles 2 wave, 2 wave + 1
            int kr = 2 * i + k_row, vr = 8 * j + v_row;
            const int swz = kr & 15;
            kr = kr < first ? first : (kr > last ? last : kr);
            vr = vr < first ? first : (vr > last ? last : vr);
            glds16_sv(Kg + base, (unsigned)kr * row_bytes + (unsigned)(((lane & 31) ^ swz) << 4), dst + i * 1024);
            glds16_sv(Vg + base, (unsigned)vr * row_bytes + v_col, dst + TILE_BYTES + (NWAVES * j + wave) * 1024);
        }
        ++issued;
        if constexpr (CACHE) {
            if (++walk_tip == tpp) {   // on to the next page: its entry was requested a page ago, the one behind it is requested now
                walk_tip = 0;
                ++walk_page;
                walk_entry = walk_next;
                if (paged && walk_page < page_hi) walk_next = bt_row[walk_page + 1];
            }
        }
    };

    // per-lane LDS read offsets: K's A operand (row r31 of a 32-key tile, chunk (2 ks + hi) ^ swizzle) and V^T's transposed reads
    const int k_rd = r31 * ROW_BYTES, k_swz = r31 & 15;
    const int li = lane & 15, lg = lane >> 4;
    const int v_rd = (4 * (lg >> 1) + (li >> 2)) * 64 + (lg & 1) * 32 + (li & 3) * 8;

    vec8 Qr[KS];
    auto visit = [&](int t, int stage, auto masked_tag) {
        constexpr bool MASKED = decltype(masked_tag)::value;
        const char *kt = smem + stage * STAGE_BYTES, *vt = kt + TILE_BYTES;
        f32x16 S[NT];
#pragma unroll
        for (int nt = 0; nt < NT; ++nt)
#pragma unroll
            for (int j = 0; j < 16; ++j) S[nt][j] = 0.0f;
        // (an operand is read one step ahead of its MFMAs, and the scheduler is held to that: what it hoists further costs registers
        // the budget lacks)
        auto read_k = [&](int s) {   // step s: k-step s / NT, key tile s % NT
            return *(const vec8 *)(kt + (s % NT) * 32 * ROW_BYTES + k_rd + (((2 * (s / NT) + hi) ^ k_swz) << 4));
        };
        vec8 ka[2];
        ka[0] = read_k(0);
#pragma unroll
        for (int s = 0; s < KS * NT; ++s) {
            if (s + 1 < KS * NT) ka[(s + 1) & 1] = read_k(s + 1);
            S[s % NT] = E::mfma(ka[s & 1], Qr[s / NT], S[s % NT]);
            __builtin_amdgcn_sched_barrier(0);
        }
        vec8 Pb[NT][2];
        {
            if constexpr (CAP) {
#pragma unroll
                for (int nt = 0; nt < NT; ++nt)
#pragma unroll
                    for (int j = 0; j < 16; ++j) {
                        const float e = __builtin_amdgcn_exp2f(S[nt][j] * cap_k);
                        S[nt][j] = __builtin_fmaf(__builtin_amdgcn_rcpf(e + 1.0f), cap_m2a, cap_a);
                    }
            }
            if constexpr (MASKED) {   // lo <= key < hi as ONE unsigned compare, key - lo < span
                const unsigned from_lo = (unsigned)(t * TILE + 4 * hi) - (unsigned)row_lo;
#pragma unroll
                for (int nt = 0; nt < NT; ++nt)
#pragma unroll
                    for (int j = 0; j < 16; ++j) {
                        const bool seen = from_lo + (unsigned)(32 * nt + (j & 3) + 8 * (j >> 2)) < row_span;
                        S[nt][j] = seen ? S[nt][j] : ninf;
                    }
            }
            float mx = ninf;
#pragma unroll
            for (int nt = 0; nt < NT; ++nt)
#pragma unroll
                for (int j = 0; j < 16; ++j) mx = fmaxf(mx, S[nt][j]);
            const float m_new = fmaxf(m, pair_max(mx));
            const float m_ref = m_new == ninf ? 0.0f : m_new;   // a row that has seen no key yet: no inf - inf
            const float alpha = __builtin_amdgcn_exp2f((m - m_ref) * c);
            m = m_new;
            // (the compiler keeps O^T in accumulation registers, which no VALU instruction reads: the rescale is 128 copies out, 128
            // products and 128 copies back.  Skipping it in a tile that raises no maximum of the wave's rows -- alpha = 1 in every
            // lane, one ballot -- was built and costs 184 to 380 bytes of scratch a lane: not taken)
#pragma unroll
            for (int dt = 0; dt < DT32; ++dt)
#pragma unroll
                for (int j = 0; j < 16; ++j) O[dt][j] *= alpha;
            const float neg_mc = -(m_ref * c);
            float rowsum = 0.0f;
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) {
                float p[16];
#pragma unroll
                for (int j = 0; j < 16; ++j) {
                    p[j] = __builtin_amdgcn_exp2f(__builtin_fmaf(S[nt][j], c, neg_mc));
                    rowsum += p[j];
                }
                Pb[nt][0] = E::pack8(p);
                Pb[nt][1] = E::pack8(p + 8);
            }
            l = __builtin_fmaf(l, alpha, rowsum);
        }
        __builtin_amdgcn_sched_barrier(0);
        auto read_v = [&](int s) {   // step s: 16-key slice s >> 3 (key tile s >> 4, half (s >> 3) & 1), d tile s & 7
            const char *vp = vt + v_rd + (s >> 3) * 8192 + (s & 7) * 512;
            s16x8 av;
            av.lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((FA_LDS(s16x4) *)(vp));
            av.hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((FA_LDS(s16x4) *)(vp + 4096));
            return __builtin_bit_cast(vec8, av);
        };
        vec8 va[2];
        va[0] = read_v(0);
#pragma unroll
        for (int s = 0; s < SLICES * DT32; ++s) {
            if (s + 1 < SLICES * DT32) va[(s + 1) & 1] = read_v(s + 1);
            O[s & 7] = E::mfma(va[s & 1], Pb[s >> 4][(s >> 3) & 1], O[s & 7]);
            __builtin_amdgcn_sched_barrier(0);
        }
    };

    if (n_tiles > 0) {
        issue_tile();
        if (AHEAD > 1 && n_tiles > 1) issue_tile();
        // Q^T, resident: row r (one past len_q reads row len_q - 1), d 16 ks + 8 hi .. + 7.  The empty asm is the registers' first use:
        // the loads' wait stands here, in front of the loop, not in it
        {
            const int r = w0 + r31, rr = r < len_q ? r : len_q - 1;
            const uint16_t *qp = a.q + (q_row0 + rr) * a.q_ss + (int64_t)h * a.q_hs + 8 * hi;
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) Qr[ks] = *(const vec8 *)(qp + 16 * ks);
        }
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) asm volatile("" : "+v"(Qr[ks]));
        int stage = 0;
        for (int it = 0; it < n_tiles; ++it) {
            // tile `it` has landed: this wave's pieces by the counted wait, the other waves' by the barrier, which also tells that
            // every wave is done with tile it - 1 -- whose stage the next request takes
            if (AHEAD > 1 && it + 1 < n_tiles)
                asm volatile("s_waitcnt vmcnt(%0)" ::"n"(PIECES) : "memory");
            else
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            wg_barrier();
            if (issued < n_tiles) issue_tile();
            const int t = t_lo + it;
            if (t >= wt_lo && t <= wt_hi) {   // (wave-uniform)
                if (t * TILE >= plain_lo && t * TILE + TILE - 1 <= plain_hi)
                    visit(t, stage, BoolTag<false>{});
                else
                    visit(t, stage, BoolTag<true>{});
            }
            stage = stage + 1 == STAGES ? 0 : stage + 1;
        }
    }

    // Epilogue.  A row without keys takes 0 for its m = -inf and is selected out (o = 0, lse = -inf), so no inf - inf is formed.
    // Lane (r31, hi) holds row r31, d 32 dt + 8 j4 + 4 hi .. + 3.
    {
        const int r = w0 + r31;
        const float l_row = pair_sum(l);
        if (r >= len_q) return;
        const bool any = l_row > 0.0f;
        const float inv = any ? 1.0f / l_row : 0.0f;
        const float lse = any ? m * scale + __logf(l_row) : ninf;
        uint16_t *op = a.o + (q_row0 + r) * a.q_ss + (int64_t)h * a.q_hs + 4 * hi;
#pragma unroll
        for (int dt = 0; dt < DT32; ++dt)
#pragma unroll
            for (int j4 = 0; j4 < 4; ++j4) {
                u32x2 w;
                w[0] = E::pack2(O[dt][4 * j4] * inv, O[dt][4 * j4 + 1] * inv);
                w[1] = E::pack2(O[dt][4 * j4 + 2] * inv, O[dt][4 * j4 + 3] * inv);
                *(u32x2 *)(op + 32 * dt + 8 * j4) = w;
            }
        if (hi == 0) a.lse[(int64_t)h * a.total_q + q_row0 + r] = lse;
    }
}

// fa_prefill256.hip: one launch on stream s, and the per-device opt-in to the kernels' dynamic LDS (outside any capture: the device's init)
hipError_t prefill256_enqueue(const Prefill256Args &a, int dtype, bool cache, bool capped, int64_t n_seqs, hipStream_t s);
hipError_t prefill256_device_init();

}  // namespace fa
