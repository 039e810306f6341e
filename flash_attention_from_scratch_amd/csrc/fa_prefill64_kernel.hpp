// fa_prefill64_kernel.hpp -- prefill attention at d_head = 64 for gfx950: many packed query rows per sequence
// against keys from a packed tensor or a 16-bit K / V cache (contiguous or paged), with a sliding window and optional attention
// sinks; forward only, o and lse.  A text of its own beside fa_fwd_kernel.hpp (whose varlen forms are the 32-rows-per-wave kernel
// at one wave per SIMD): at 64 a 64-key tile is half the MFMA work while the softmax, the masks, the barrier and the address work
// per tile stay, and O^T is half the accumulators -- so a wave takes 64 rows here and two waves share a SIMD.
//
//  * Grid n_seqs * n_heads * ceil(max_seqlen_q / 256), host-visible numbers only; workgroup (b, h, qb) owns rows 256 qb .. of
//    sequence b, 4 waves of 64 rows (two 32-row tiles QT).  A workgroup whose block starts at or beyond len_q returns before any
//    barrier or DMA.  Per lane: O^T 64 + S^T 64 + P 32 + Q^T 32 registers and the row state -- inside the 256 that two waves per
//    SIMD leave (__launch_bounds__(256, 2)); 48 KiB of LDS, two workgroups per CU.
//  * Both products are transposed, v_mfma_f32_32x32x16_{bf16,f16}; lane (r31 = lane & 31, hi = lane >> 5) owns query rows
//    32 qt + r31 of its wave, so m, l and the rescale are lane-local and a row maximum costs one v_permlane32_swap:
//        S^T = K Q^T     two 32-key tiles x four k-steps; A = K rows by ds_read_b128 from the K image, B = Q^T resident (loaded
//                        once: row r, d 16 ks + 8 hi .. + 7).  C: lane holds keys 32 nt + (j & 3) + 8 (j >> 2) + 4 hi, j = 0 .. 15
//        O^T = V^T P^T   two 32-d tiles x four 16-key k-steps; B = P^T, the S^T registers 8 half .. 8 half + 7 of key tile nt packed in
//                        place, A = V^T by two ds_read_b64_tr_b16 that pick the same keys (4 hi + 0 .. 3 and 8 + 4 hi + 0 .. 3 of the
//                        16): a contraction index may be permuted when both operands agree, so P never leaves its registers.
//  * One tile is 64 keys: 8 KiB of K and 8 KiB of V, global -> LDS by DMA (global_load_lds_dwordx4, 1 KiB per wave instruction,
//    16 pieces per tile, 4 per wave), a ring of 3 stages requested two tiles ahead.  The waits are counted: before the barrier of
//    tile i a wave waits until at most the 4 pieces of tile i + 1 are in flight (vmcnt(4); the walk's last tile: vmcnt(0)); the one
//    barrier per tile publishes tile i and frees tile i - 1's stage, which the request for tile i + 2 then takes.
//  * The DMA writes LDS lane-linearly, so both images are made by permuting the lanes' SOURCE addresses.  Rows are 128 bytes here:
//      K image [64 keys][128 bytes], the 16-byte chunk index XOR ((key >> 1) & 7).  A ds_read_b128 serves 16 lanes at a time (256
//        bytes, every bank once at best); they ask for one chunk c of 16 consecutive keys.  Unswizzled, key k's chunk lies at byte
//        (128 k + 16 c) mod 256: two places for sixteen lanes, an 8-way conflict.  With the XOR the eight key pairs take the
//        eight chunk slots of a 128-byte half and a pair's two keys the two halves: sixteen different 16-byte slots of the 256 --
//        every bank once.  (At d128, 256-byte rows, the XOR is key & 15; a pitch of 128 + 16 would do as well and cost 1 KiB a tile
//        and the DMA's lane-linear write: a piece would no longer be 8 whole rows.)
//      V image [8 key groups][2 d halves][8 keys][32 d]: 512-byte subtiles.  A ds_read_b64_tr_b16 wave instruction (lane 16 g + 4 q
//        + p: key 4 (g >> 1) + q, d 16 (g & 1) + 4 p .. + 3 of a subtile) reads 8 keys x 64 bytes = the 512 contiguous bytes of one
//        subtile: every bank twice, which is what 512 bytes cost.  All 16 reads of a tile are one base and immediate offsets.
//    A piece of K is 8 whole rows (lane: key 8 i + lane / 8, the chunk its slot holds), a piece of V one key group (lane: d half
//    lane / 32, key (lane & 31) / 4, 16 bytes at d 8 (lane & 3)): global reads of 128 and of 64 contiguous bytes.
//  * Row r of a sequence sits at p = r + (len_k - len_q) and sees keys lo_r = max(0, p - left) .. hi_r = min(len_k - 1, p + right),
//    -1 unbounded, causal arriving as right = 0.  Both grow with r: the workgroup (rows r0 .. r1) visits tiles lo_r0 / 64 ..
//    hi_r1 / 64 in ascending order and nothing else, a wave computes only the tiles lo_w0 / 64 .. hi_w1 / 64 of its own rows, and a
//    tile runs the mask code (lo <= key < hi as one unsigned compare per element) only if it reaches above hi of the wave's first
//    row, below lo of its last, or across len_k; every other tile takes the unmasked visit.
//  * Softmax: the reference arithmetic -- running maximum m with rescale, fp32, p = exp2(s c - m c), c = log2(e) / sqrt(64) rounded
//    once from the double product; l is summed from the fp32 p, the lane pair's halves added in the epilogue.
//  * Fetch contract (include/fa_hip.h, the d128 forms'): lengths clamped as fa_varlen_layout / fa_kvcache_layout say; a key below
//    the workgroup's floor lo_r0 is FETCHED from key lo_r0, one at or beyond len_k from key len_k - 1 (both lie in the tile that
//    asks), and masked; block_table entries are clamped to [0, num_pages); page_size % 64 == 0, so a tile lies in one page; one
//    table lookup per page crossed (requested a tile ahead of its use), none below the floor tile's page or above the top tile's.
//    Positions are 32-bit (the host bounds lengths by 2^30 - 128), every element offset is formed in 64 bits, a lane's byte offset
//    inside a tile (< 64 rows) in 32.
//  * Sinks are a nullable pointer and act in the epilogue only, folded against max(m, z); none is z = -inf through the same
//    instructions, so a null pointer and a tensor of -inf give the same bits.  A row without keys: o = 0, lse = z.
//  * The packed and the cache form differ only in how a tile's base address is found: the same bits on the same keys.  Fixed walk
//    order, no atomics, no workspace.
//  * FP8: the cache holds e4m3fn bytes, its strides count bytes.  The DMA cannot convert, so the raw tile (4 KiB of K,
//    4 KiB of V) lands in a ring of three 8-KiB raw stages behind two 16-bit stages (56 KiB, still two workgroups per CU), and at the
//    tile seam, when S and P are dead, each lane converts the 32 bytes it fetched itself into the two images above, byte for byte
//    (convert_tile): the visit, the masks and the epilogue are the 16-bit form's text and arithmetic, so with power-of-two descales
//    the bits are the 16-bit form's on the dequantized cache.  k_descale multiplies c and the epilogue's scale (S and m stay raw
//    logits), v_descale the final 1 / l; the sink meets the dequantized logit.
#pragma once
#include "fa_fwd_kernel.hpp"

namespace fa {

struct Prefill64Args {
    const uint16_t *q, *k, *v;
    uint16_t *o;
    float *lse;                    // (n_heads, total_q)
    const int32_t *cu_q;           // n_seqs + 1 row offsets of q / o / lse
    const int32_t *cu_k;           // packed keys: n_seqs + 1 row offsets of k / v
    const int32_t *cache_seqlens;  // cache: (n_seqs) valid keys
    const int32_t *block_table;    // paged cache: (n_seqs, bt_stride); null: contiguous
    const float *sinks;            // (n_heads) fp32 or null
    int64_t q_ss, q_hs;            // q's and o's token and head strides (elements)
    int64_t kv_ss, kv_hs;          // k's and v's
    int64_t page_stride;           // cache: elements between pages (contiguous: between batch entries)
    int32_t n_heads, group, n_q_blocks;
    int32_t total_q, max_seqlen_q;
    int32_t total_k, max_seqlen_k;   // packed keys
    int32_t bt_stride, num_pages, tiles_per_page, max_len;   // cache (contiguous: tiles_per_page covers the whole entry)
    int32_t left, right;           // -1 = unbounded (causal: right = 0)
    const float *k_descale, *v_descale;   // fp8 cache: (n_seqs, n_kv_heads) fp32, row stride ds_bs; null = 1
    int64_t ds_bs;
};

namespace prefill64 {
constexpr int D = 64, TILE = 64, NWAVES = 4, THREADS = NWAVES * 64, RW = 64, R = NWAVES * RW, STAGES = 3;
constexpr int TILE_BYTES = TILE * D * 2, STAGE_BYTES = 2 * TILE_BYTES;   // K then V
constexpr int PIECES = 2 * TILE_BYTES / 1024 / NWAVES;                   // DMA pieces per wave and tile: 2 of K, 2 of V
// the fp8 cache's transport (FP8, below): two converted stages in front of a ring of three raw ones, 56 KiB
constexpr int RAW_TILE_BYTES = TILE * D, RAW_STAGE_BYTES = 2 * RAW_TILE_BYTES, RAW_PIECES = 2;   // per wave and tile: 1 KiB of K, 1 of V
constexpr int CONV_STAGES = 2, RAW_BASE = CONV_STAGES * STAGE_BYTES, FP8_LDS_BYTES = RAW_BASE + STAGES * RAW_STAGE_BYTES;
template <bool FP8> struct KvElem { typedef uint16_t type; };
template <> struct KvElem<true> { typedef uint8_t type; };   // (an fp8 cache's strides count bytes)
}  // namespace prefill64

template <int DT, bool CACHE, bool FP8 = false>
__global__ void __launch_bounds__(prefill64::THREADS, 2) fa_prefill64_kernel(const Prefill64Args a) {
    static_assert(CACHE || !FP8, "fp8 keys live in a cache");
    using E = Elem<DT>;
    using vec8 = typename E::vec8;
    using namespace prefill64;
    using KV = typename KvElem<FP8>::type;
    constexpr int KS = D / 16, DT32 = D / 32, QT = RW / 32, NT = TILE / 32;
    __shared__ __attribute__((aligned(1024))) char smem[FP8 ? FP8_LDS_BYTES : STAGES * STAGE_BYTES];

    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int r31 = lane & 31, hi = lane >> 5;
    const int qb = blockIdx.x % a.n_q_blocks, bh = blockIdx.x / a.n_q_blocks;
    const int h = bh % a.n_heads, b = bh / a.n_heads;

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

    // (fp8 cache: k_descale times both constants, one scalar per workgroup -- S and the running maximum stay raw logits, and the
    // exponents, the rescale and the epilogue's m scale come out in dequantized units; a power of two changes no rounding)
    float kd = 1.0f;
    if constexpr (FP8) kd = a.k_descale ? a.k_descale[(int64_t)b * a.ds_bs + h / a.group] : 1.0f;
    const float scale0 = 1.0f / __builtin_sqrtf((float)D);
    const float scale = FP8 ? scale0 * kd : scale0;
    const float c = FP8 ? (float)((double)scale0 * 1.4426950408889634074) * kd : (float)((double)scale0 * 1.4426950408889634074);
    const float ninf = -__builtin_inff();

    f32x16 O[QT][DT32];
    float m[QT], l[QT];
    int row_lo[QT];
    unsigned row_span[QT];
#pragma unroll
    for (int qt = 0; qt < QT; ++qt) {
#pragma unroll
        for (int t = 0; t < DT32; ++t)
#pragma unroll
            for (int j = 0; j < 16; ++j) O[qt][t][j] = 0.0f;
        m[qt] = ninf;
        l[qt] = 0.0f;
        const int p = w0 + 32 * qt + r31 + shift;   // (a row past len_q: computed, never stored)
        const int lo = p - w_left > 0 ? p - w_left : 0, hi1 = p + w_right + 1 < len_k ? p + w_right + 1 : len_k;
        row_lo[qt] = lo;
        row_span[qt] = hi1 > lo ? (unsigned)(hi1 - lo) : 0u;
    }

    const int kvh = h / a.group;
    const KV *Kg = (const KV *)a.k + (int64_t)kvh * a.kv_hs, *Vg = (const KV *)a.v + (int64_t)kvh * a.kv_hs;
    const unsigned smem_base = __builtin_amdgcn_readfirstlane(lds_addr(smem));
    const unsigned row_bytes = (unsigned)(a.kv_ss * sizeof(KV));

    // the walk over the key tiles, ascending: tile t's base offset (elements from k / v).  Cache: page and tile-in-page by counters,
    // the page's table entry requested when the walk enters the page before it (a scalar load through the constant address space:
    // nothing writes the table while the kernel runs) -- one lookup per page crossed, none outside [floor page, top page]
    typedef const __attribute__((address_space(4))) int32_t *table_ptr;
    const table_ptr bt_row = (table_ptr)(unsigned long long)(a.block_table + (int64_t)b * a.bt_stride);
    const bool paged = CACHE && a.block_table != nullptr;
    const int tpp = CACHE ? a.tiles_per_page : 1;
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
        if constexpr (FP8) {
            // raw bytes: the wave's piece is keys 16 wave .. + 15 of K and of V, lane: key 16 wave + lane / 4, bytes 16 (lane & 3) .. + 15
            // of its 64 -- the same clamp, and the lane that fetched a chunk is the one that converts it (convert_tile)
            const unsigned dst = smem_base + RAW_BASE + stage * RAW_STAGE_BYTES + wave * 1024;
            int ln = lane;
            asm volatile("" : "+v"(ln));   // (formed per tile, as in convert_tile)
            int r = 16 * wave + (ln >> 2);
            r = r < first ? first : (r > last ? last : r);
            const unsigned off = (unsigned)r * row_bytes + (unsigned)((ln & 3) << 4);
            glds16_sv(Kg + base, off, dst);
            glds16_sv(Vg + base, off, dst + RAW_TILE_BYTES);
        }
        const unsigned dst = smem_base + stage * STAGE_BYTES;
#pragma unroll
        for (int j = 0; j < (FP8 ? 0 : PIECES / 2); ++j) {
            const int i = wave + NWAVES * j;   // piece i: keys 8 i .. 8 i + 7 of K and of V
            int kr = 8 * i + (lane >> 3), vr = 8 * i + ((lane & 31) >> 2);
            const int swz = (kr >> 1) & 7;
            kr = kr < first ? first : (kr > last ? last : kr);
            vr = vr < first ? first : (vr > last ? last : vr);
            glds16_sv(Kg + base, (unsigned)kr * row_bytes + (unsigned)(((lane & 7) ^ swz) << 4), dst + i * 1024);
            glds16_sv(Vg + base, (unsigned)vr * row_bytes + (unsigned)((lane >> 5) * 64 + (lane & 3) * 16), dst + TILE_BYTES + i * 1024);
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

    // fp8: raw stage `raw` -> converted stage `conv`, the images the DMA builds for a 16-bit cache, byte for byte.  A lane converts the
    // 16 + 16 bytes it fetched itself (so the raw ring needs no barrier: its own vmcnt wait is all), lane-linear ds_read_b128s.  K:
    // chunks 2 q and 2 q + 1 of key 16 wave + lane / 4 go to slots (2 q + e) ^ swizzle of its 128-byte row -- sixteen lanes are four
    // consecutive keys x four q: the two even keys share a 128-byte half of the 256 and differ in the swizzle's bit 0, so with e
    // fixed one takes the even slots and the other the odd ones; the odd keys likewise in the other half: every bank once.  V: the 32
    // contiguous bytes at [key / 8][q / 2][key % 8][16 (q & 1) ..]; q and q + 2 lie 512 bytes apart, the same banks, so the lanes of
    // q >= 2 write their two halves in the other order.
    auto convert_tile = [&](int raw, int conv) {
        int ln = lane;
        asm volatile("" : "+v"(ln));   // (the lane's offsets are formed here, per tile: held across the visit they cost registers the budget lacks)
        const char *rp = smem + RAW_BASE + raw * RAW_STAGE_BYTES + wave * 1024 + ln * 16;
        char *kt = smem + conv * STAGE_BYTES, *vt = kt + TILE_BYTES;
        const u32x4 k8 = *(const u32x4 *)rp, v8 = *(const u32x4 *)(rp + RAW_TILE_BYTES);
        const int key = 16 * wave + (ln >> 2), q4 = ln & 3, swz = (key >> 1) & 7;
        *(vec8 *)(kt + key * 128 + (((2 * q4) ^ swz) << 4)) = cvt_fp8x8<DT>(k8[0], k8[1]);
        *(vec8 *)(kt + key * 128 + (((2 * q4 + 1) ^ swz) << 4)) = cvt_fp8x8<DT>(k8[2], k8[3]);
        char *vp = vt + (key >> 3) * 1024 + (q4 >> 1) * 512 + (key & 7) * 64 + (q4 & 1) * 32;
        const bool flip = q4 >> 1;
        const vec8 v_lo = cvt_fp8x8<DT>(v8[0], v8[1]), v_hi = cvt_fp8x8<DT>(v8[2], v8[3]);
        *(vec8 *)(vp + (flip ? 16 : 0)) = flip ? v_hi : v_lo;
        *(vec8 *)(vp + (flip ? 0 : 16)) = flip ? v_lo : v_hi;
    };

    // per-lane LDS read offsets: K's A operand (row r31 of a 32-key tile, chunk (2 ks + hi) ^ swizzle) and V^T's transposed reads
    const int k_rd = r31 * 128, k_swz = (r31 >> 1) & 7;
    const int li = lane & 15, lg = lane >> 4;
    const int v_rd = (4 * (lg >> 1) + (li >> 2)) * 64 + (lg & 1) * 32 + (li & 3) * 8;

    vec8 Qr[QT][KS];
    auto visit = [&](int t, int stage, auto masked_tag) {
        constexpr bool MASKED = decltype(masked_tag)::value;
        const char *kt = smem + stage * STAGE_BYTES, *vt = kt + TILE_BYTES;
        f32x16 S[QT][NT];
#pragma unroll
        for (int qt = 0; qt < QT; ++qt)
#pragma unroll
            for (int nt = 0; nt < NT; ++nt)
#pragma unroll
                for (int j = 0; j < 16; ++j) S[qt][nt][j] = 0.0f;
        // (an operand is read one step ahead of its MFMAs, and the scheduler is held to that: what it hoists further costs registers
        // the budget lacks)
        auto read_k = [&](int s) { return *(const vec8 *)(kt + (s & 1) * 32 * 128 + k_rd + (((2 * (s >> 1) + hi) ^ k_swz) << 4)); };
        vec8 ka[2];
        ka[0] = read_k(0);
#pragma unroll
        for (int s = 0; s < KS * NT; ++s) {   // step s: k-step s >> 1, key tile s & 1
            if (s + 1 < KS * NT) ka[(s + 1) & 1] = read_k(s + 1);
#pragma unroll
            for (int qt = 0; qt < QT; ++qt) S[qt][s & 1] = E::mfma(ka[s & 1], Qr[qt][s >> 1], S[qt][s & 1]);
            __builtin_amdgcn_sched_barrier(0);
        }
        vec8 Pb[QT][NT][2];
#pragma unroll
        for (int qt = 0; qt < QT; ++qt) {
            __builtin_amdgcn_sched_barrier(0);   // (a phase at a time: what the scheduler hoists across costs registers the budget lacks)
            if constexpr (MASKED) {   // lo <= key < hi as ONE unsigned compare, key - lo < span
                const unsigned from_lo = (unsigned)(t * TILE + 4 * hi) - (unsigned)row_lo[qt];
#pragma unroll
                for (int nt = 0; nt < NT; ++nt)
#pragma unroll
                    for (int j = 0; j < 16; ++j) {
                        const bool seen = from_lo + (unsigned)(32 * nt + (j & 3) + 8 * (j >> 2)) < row_span[qt];
                        S[qt][nt][j] = seen ? S[qt][nt][j] : ninf;
                    }
            }
            float mx = ninf;
#pragma unroll
            for (int nt = 0; nt < NT; ++nt)
#pragma unroll
                for (int j = 0; j < 16; ++j) mx = fmaxf(mx, S[qt][nt][j]);
            const float m_new = fmaxf(m[qt], pair_max(mx));
            const float m_ref = m_new == ninf ? 0.0f : m_new;   // a row that has seen no key yet: no inf - inf
            const float alpha = __builtin_amdgcn_exp2f((m[qt] - m_ref) * c);
            m[qt] = m_new;
#pragma unroll
            for (int dt = 0; dt < DT32; ++dt)
#pragma unroll
                for (int j = 0; j < 16; ++j) O[qt][dt][j] *= alpha;
            const float neg_mc = -(m_ref * c);
            float rowsum = 0.0f;
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) {
                float p[16];
#pragma unroll
                for (int j = 0; j < 16; ++j) {
                    p[j] = __builtin_amdgcn_exp2f(__builtin_fmaf(S[qt][nt][j], c, neg_mc));
                    rowsum += p[j];
                }
                Pb[qt][nt][0] = E::pack8(p);
                Pb[qt][nt][1] = E::pack8(p + 8);
            }
            l[qt] = __builtin_fmaf(l[qt], alpha, rowsum);
        }
        __builtin_amdgcn_sched_barrier(0);
        auto read_v = [&](int s) {   // step s: 16-key slice s >> 1 (key tile s >> 2, half (s >> 1) & 1), d tile s & 1
            const char *vp = vt + v_rd + (s >> 1) * 2048 + (s & 1) * 512;
            s16x8 av;
            av.lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((FA_LDS(s16x4) *)(vp));
            av.hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((FA_LDS(s16x4) *)(vp + 1024));
            return __builtin_bit_cast(vec8, av);
        };
        vec8 va[2];
        va[0] = read_v(0);
#pragma unroll
        for (int s = 0; s < 2 * NT * DT32; ++s) {
            if (s + 1 < 2 * NT * DT32) va[(s + 1) & 1] = read_v(s + 1);
#pragma unroll
            for (int qt = 0; qt < QT; ++qt) O[qt][s & 1] = E::mfma(va[s & 1], Pb[qt][s >> 2][(s >> 1) & 1], O[qt][s & 1]);
            __builtin_amdgcn_sched_barrier(0);
        }
    };

    if (n_tiles > 0) {
        issue_tile();
        if (n_tiles > 1) issue_tile();
        if constexpr (FP8)
            if (n_tiles > 2) issue_tile();   // (the raw ring runs three tiles ahead)
        // Q^T, resident: row r (one past len_q reads row len_q - 1), d 16 ks + 8 hi .. + 7.  The empty asm is the registers' first use:
        // the loads' wait stands here, in front of the loop, not in it
#pragma unroll
        for (int qt = 0; qt < QT; ++qt) {
            const int r = w0 + 32 * qt + r31, rr = r < len_q ? r : len_q - 1;
            const uint16_t *qp = a.q + (q_row0 + rr) * a.q_ss + (int64_t)h * a.q_hs + 8 * hi;
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) Qr[qt][ks] = *(const vec8 *)(qp + 16 * ks);
        }
#pragma unroll
        for (int qt = 0; qt < QT; ++qt)
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) asm volatile("" : "+v"(Qr[qt][ks]));
        if constexpr (FP8) {
            // One barrier per tile, with a prologue that converts tile 0.  Iteration `it`: the wave's own raw pieces of tile it + 1 have
            // landed (at most tile it + 2's two in flight); the barrier publishes converted tile `it` and tells that every wave is done
            // with tile it - 1, whose converted stage tile it + 1 takes; raw tile it + 3 is requested into the raw stage of tile `it`,
            // which this wave alone read, an iteration ago; then convert it + 1, visit `it`.
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            convert_tile(0, 0);
            int raw = 1;   // tile it + 1's raw stage
            for (int it = 0; it < n_tiles; ++it) {
                if (it + 2 < n_tiles)
                    asm volatile("s_waitcnt vmcnt(%0)" ::"n"(RAW_PIECES) : "memory");
                else
                    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                wg_barrier();
                if (issued < n_tiles) issue_tile();
                if (it + 1 < n_tiles) convert_tile(raw, (it + 1) & 1);
                raw = raw + 1 == STAGES ? 0 : raw + 1;
                const int t = t_lo + it;
                if (t >= wt_lo && t <= wt_hi) {   // (wave-uniform)
                    if (t * TILE >= plain_lo && t * TILE + TILE - 1 <= plain_hi)
                        visit(t, it & 1, BoolTag<false>{});
                    else
                        visit(t, it & 1, BoolTag<true>{});
                }
            }
        }
        int stage = 0;
        for (int it = 0; it < (FP8 ? 0 : n_tiles); ++it) {
            // tile `it` has landed: this wave's pieces by the counted wait, the other waves' by the barrier, which also tells that
            // every wave is done with tile it - 1 -- whose stage the request for tile it + 2 takes
            if (it + 1 < n_tiles)
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

    // Epilogue.  The row's sink joins here, once; none is z = -inf.  Natural units against a common maximum, so that neither term
    // overflows; a row without keys takes 0 for its m = -inf and is selected out (o = 0, lse = z), so no inf - inf is formed
    // (where l > 0, m is finite and so is M).  Lane (r31, hi) holds row 32 qt + r31, d 32 dt + 8 j4 + 4 hi .. + 3.
    const float z = a.sinks ? a.sinks[h] : ninf;
#pragma unroll
    for (int qt = 0; qt < QT; ++qt) {
        const int r = w0 + 32 * qt + r31;
        const float l_row = pair_sum(l[qt]);
        if (r >= len_q) continue;
        const bool any = l_row > 0.0f;
        const float ms = any ? m[qt] * scale : 0.0f;
        const float M = fmaxf(ms, z);
        const float al = __expf(ms - M), l_all = __builtin_fmaf(l_row, al, __expf(z - M));
        float inv = any ? al / l_all : 0.0f;
        if constexpr (FP8) inv *= a.v_descale ? a.v_descale[(int64_t)b * a.ds_bs + kvh] : 1.0f;   // (read here, not held across the loop)
        const float lse = any ? M + __logf(l_all) : z;
        uint16_t *op = a.o + (q_row0 + r) * a.q_ss + (int64_t)h * a.q_hs + 4 * hi;
#pragma unroll
        for (int dt = 0; dt < DT32; ++dt)
#pragma unroll
            for (int j4 = 0; j4 < 4; ++j4) {
                u32x2 w;
                w[0] = E::pack2(O[qt][dt][4 * j4] * inv, O[qt][dt][4 * j4 + 1] * inv);
                w[1] = E::pack2(O[qt][dt][4 * j4 + 2] * inv, O[qt][dt][4 * j4 + 3] * inv);
                *(u32x2 *)(op + 32 * dt + 8 * j4) = w;
            }
        if (hi == 0) a.lse[(int64_t)h * a.total_q + q_row0 + r] = lse;
    }
}

hipError_t prefill64_enqueue(const Prefill64Args &a, int dtype, bool cache, int64_t n_seqs, hipStream_t s);   // fa_prefill64.hip
hipError_t prefill64_fp8_enqueue(const Prefill64Args &a, int dtype, int64_t n_seqs, hipStream_t s);            // fa_prefill64_fp8.hip

}  // namespace fa
