// fa_decode256_kernel.hpp -- KV-cache decode attention at d_head = 256 for gfx950: a few query rows per sequence
// against a long 16-bit K / V cache of a per-sequence length the DEVICE holds, with a sliding window and optional logit soft-capping
// (the Gemma-2 / Gemma-3 shapes: two query heads per K / V head, a 4096-key window, a cap of 50).  A text of its own beside
// fa_decode_kernel.hpp (d_head = 128) and fa_decode64_kernel.hpp (64): a key is 512 bytes, and per 16 query rows O^T alone is 64
// accumulator registers a lane and the resident Q^T 32, so neither the d128 kernel's 64 rows nor its 32-key unit carry over.
//
//  * Split kernel, grid batch * n_kv_heads * num_splits, 4 waves, one wave per SIMD (512 registers a lane).  The rows = seqlen_q *
//    group query rows that share one K / V head (row r = query position r / group, head kv_head * group + r % group) are the N
//    dimension of v_mfma_f32_16x16x32_{bf16,f16}: NT = 1 or 2 tiles of 16 rows (32 rows at most: four tiles would take 384 registers
//    before S^T and any prefetch), rows past the last one padded (masked, never stored).  Both products are transposed, so a lane
//    (li = lane & 15, g = lane >> 4) owns query row 16 nt + li:
//        S^T = K Q^T     KT = UNIT / 16 key tiles x KS = 8 k-steps; A = 16 keys x 32 d straight from global memory, lane (li, g): key
//                        16 kt + li, d 32 ks + 8 g .. + 7 (16 bytes).  The operand layout ties a lane to ONE key and to a quarter of a
//                        k-step, so one load covers a 64-byte piece of each of sixteen rows; the eight loads of a key tile are issued
//                        back to back in k-step order, so the two halves of a 128-byte line are asked for by neighbouring
//                        instructions and a row's four lines one behind the other -- sixteen whole 512-byte rows per key tile, no
//                        other tile's request between them.  B = Q^T: NT = 1, resident, 8 operands = 32 registers; NT = 2, where
//                        O^T takes 128 registers that VALU instructions rescale (so VGPRs) and the compiler, with a resident Q^T's
//                        64 more, needs scratch: a workgroup-wide [32 rows][256 d] LDS image written once, one 16-byte read per
//                        MFMA.  Its row pitch is QROW = 528 = 512 + 16: the sixteen lanes of a group read the same column of
//                        sixteen rows, 16 * li modulo 256 -- every bank once.
//        O^T = V^T P^T   DT16 = 16 d-tiles, a key tile at a time; A = V^T by ONE ds_read_b64_tr_b16 per d-tile from a wave-private
//                        [16 keys][256 d] LDS image, B = P^T, the tile's four S^T accumulators packed in place (lane group g: keys
//                        4 g .. 4 g + 3).  The shipped unit IS one key tile, so the product is the 16-key form of the same
//                        instruction family, v_mfma_f32_16x16x16_{bf16,f16} -- the same operand layouts (A: lane (li, g) = d li,
//                        keys 4 g ..; B: row li, keys 4 g ..), no zero half multiplied; a 32-key unit sends its two tiles through
//                        the same image one behind the other (DS operations of a wave complete in order), so the image is 8.5 KiB
//                        a wave for either unit.
//    V is fetched in whole 512-byte rows, 32 lanes a key, two keys per load: lane (r = lane >> 5, c = lane & 31) of load i takes key
//    2 i + r, d 8 c .. + 7, and writes its 16 bytes to row (2 i + r) % 16 of the image.
//  * The image's row pitch is VROW = 544 bytes = 512 + 32.  Reads: a 32-lane half of a transposed read covers 32 bytes (one d-tile)
//    of each of 8 consecutive keys; 544 = 17 * 32 with 17 odd, so the eight 32-byte pieces start at the eight different multiples
//    of 32 modulo the 256 bytes of the 64 banks -- every bank once.  Writes: a 16-byte write is served sixteen lanes at a time, and
//    sixteen consecutive lanes hold c = 0 .. 15 or 16 .. 31 of ONE key: 256 contiguous bytes of one image row (the d128 image's
//    sixteen lanes cover one whole 256-byte row, the d64 image's two 128-byte rows that have to be paired).  256 contiguous bytes
//    are 64 consecutive 4-byte words, one per bank whatever the row's offset is -- every bank once under ANY pitch that keeps the
//    16-byte alignment, so the pitch is the reads' to choose and the lanes' key order is free: consecutive keys, which also makes
//    one V load two whole rows (eight whole 128-byte lines) of global memory.
//  * UNIT, the keys a wave visits at once, is a parameter of this text: 16 keys (8 KiB of K and 8 KiB of V per visit -- the d128
//    unit's 16 KiB) or 32.  Both are instantiated and were measured side by side; UNIT_SHIPPED is the faster, the
//    other stays behind FA_DECODE256_UNIT for the bench.  K and V are held ONE unit ahead in every form, two register sets taken in
//    turn; what that costs a lane:
//        (NT 1, 16)  two sets of 32 + 32 registers = 128, beside Q^T 32, O^T 64, S^T 4
//        (NT 2, 16)  128, beside O^T 128, S^T 8 (Q^T in LDS)
//        (NT 1, 32)  two sets of 64 + 64 = 256, beside Q^T 32, O^T 64, S^T 8
//        (NT 2, 32)  not built: 256 beside O^T 128 and S^T 16 needs scratch, and so does the form that holds only K ahead and
//                    requests V at the top of its own unit (192); beyond 16 rows FA_DECODE256_UNIT has nothing to choose.
//    So a wave keeps 16 KiB (unit 16) or 32 KiB (unit 32) in flight beside the unit it works on.  No kernel uses scratch.
//  * A workgroup reads the length, takes its contiguous share of the key tiles [lo_min / 64, ceil(len / 64)) -- the d128 windowed
//    formula -- and its waves take that share's units round-robin.  One running maximum and sum per row per unit.  The merge of the
//    four waves and the epilogue are the d128 kernel's over sixteen d-tiles.
//  * The window is always in: one form, (-1, -1) runs through it; lo <= key < hi per row as one unsigned compare.
//  * Soft-capping is a template flag, CAP: the uncapped kernels hold none of its instructions.  Every S accumulator goes through
//    A tanh(S / A) = A - 2 A / (exp2(S cap_k) + 1), A = softcap * 16, cap_k = 2 log2(e) / A -- the d128 decode's form, one v_exp_f32
//    and one v_rcp_f32 per element -- right behind the S^T MFMAs and in front of the `seen` select: a masked key stays -inf, and lse
//    is taken over the capped logits.  exp2 overflowing gives A, underflowing -A: no NaN at either end.  The partials and the
//    combine kernel do not know of it.
//  * Fetch contract (include/fa_hip.h, d128's word for word): len is clamped to [0, max_len]; a key at or beyond len is FETCHED from
//    key len - 1, one below lo_min = max(0, len - seqlen_q - left) from key lo_min, both masked; block_table entries are clamped to
//    [0, num_pages); no key, page or table entry wholly below lo_min is touched; the prefetch behind a wave's last unit reads one
//    valid row.  page_size % 64 == 0: a unit lies in one page and costs one scalar block_table load.
//  * num_splits == 1: o and lse are written; else fp32 partials (num_splits, batch, n_kv_heads, rows, 256), o normalised, and lse
//    (-inf for a row that saw no key in the split), which fa_decode256_combine_kernel, 64 threads with four d each, sums in split
//    order.  No atomics: the same bits for the same inputs and the same num_splits.
//  * scale = 1 / sqrt(256) = 1 / 16; c = scale * log2(e), rounded once from the double product.
#pragma once
#include "fa_decode_kernel.hpp"

namespace fa {

struct Decode256Args {
    DecodeArgs d;             // part_o: (num_splits, batch, n_kv_heads, rows, 256)
    int32_t left, right;      // -1 = unbounded (causal: right = 0)
    float cap_a, cap_inv_a;   // A = softcap * sqrt(256) and 1 / A (the host rounds each once); read by the capped kernels only
};

namespace decode256 {
constexpr int D = 256, TILE = 64, NWAVES = 4, THREADS = NWAVES * 64, MAX_ROWS = 32;
constexpr int VROW = 544;          // bytes per key of the V image (the argument is at the head of this file)
constexpr int QROW = 528;          // bytes per row of the Q^T image (NT = 2), likewise
constexpr int UNIT_SHIPPED = 16;   // keys per wave visit: 16 or 32, measured side by side

// the 16-key form of the products' instruction (a 16-key unit's O^T): A lane (li, g) = row li, k 4 g .. + 3, B likewise by column
template <int DT> static FA_DEV f32x4 mfma16_k16(s16x4 a, s16x4 b, f32x4 c) {
    if constexpr (DT == 15) {
        return __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(a, b, c, 0, 0, 0);
    } else {
        typedef _Float16 f16x4 __attribute__((ext_vector_type(4)));
        return __builtin_amdgcn_mfma_f32_16x16x16f16(__builtin_bit_cast(f16x4, a), __builtin_bit_cast(f16x4, b), c, 0, 0, 0);
    }
}
}  // namespace decode256

template <int DT, int NT, bool PAGED, int UNIT, bool CAP>
__global__ void __launch_bounds__(decode256::THREADS) fa_decode256_split_kernel(const Decode256Args args) {
    using E = Elem<DT>;
    using vec8 = typename E::vec8;
    using namespace decode256;
    static_assert(UNIT == 16 || UNIT == 32, "a unit is one 16-key tile or two");
    static_assert(NT == 1 || (NT == 2 && UNIT == 16), "at most 32 packed rows; beyond 16 the 16-key unit only (32 keys need scratch)");
    constexpr int KS = D / 32, DT16 = D / 16, KT = UNIT / 16, VL = UNIT / 2, UPT = TILE / UNIT;   // (VL: V loads, UPT: units per tile)
    constexpr int VBYTES = 16 * VROW;                    // one wave's image: one key tile
    constexpr int MERGE = NT * DT16 * 64 * 16;           // one wave's accumulators
    constexpr int MAIN = NWAVES * VBYTES > MERGE ? NWAVES * VBYTES : MERGE;
    constexpr bool Q_LDS = NT == 2;                      // Q^T resident in registers, or in LDS (32 rows: the registers are O^T's)
    constexpr int STATS = (NWAVES + 1) * NT * 16 * 4, QBYTES = Q_LDS ? NT * 16 * QROW : 0;
    __shared__ __attribute__((aligned(16))) char smem[MAIN + STATS + QBYTES];
    const DecodeArgs &a = args.d;
    struct KRegs { vec8 r[KT][KS]; };   // one unit in the prefetch registers: 16 bytes per lane and load
    struct VRegs { s16x8 r[VL]; };

    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int li = lane & 15, g = lane >> 4;
    const int vr = lane >> 5, vc = lane & 31;   // V's load shape: key 2 i + vr, d 8 vc ..
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
    [[maybe_unused]] vec8 Qr[Q_LDS ? 1 : NT][KS];
    int pos[NT];
    constexpr int FAR = (1 << 30) + 64;   // unbounded, or beyond what any length reaches (the host: len <= 2^30 - 128; p >= -32): all one
    const int w_left = args.left < 0 || args.left > FAR ? FAR : args.left;
    const int w_right = args.right < 0 || args.right > FAR ? FAR : args.right;
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
        const int r = nt * 16 + li;
        const bool valid = r < a.rows;
        const int rr = valid ? r : 0, qi = rr / a.group, qh = kvh * a.group + rr % a.group;
        if constexpr (!Q_LDS) {
            const uint16_t *qp = a.q + (int64_t)b * a.q_bs + (int64_t)qi * a.q_ss + (int64_t)qh * a.q_hs + g * 8;
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) Qr[nt][ks] = *(const vec8 *)(qp + ks * 32);
        }
        pos[nt] = !valid ? -(1 << 30) - 66 : len - a.seqlen_q + qi;   // (a padded row: p + w_right + 1 < 0)
    }

    // Q^T in LDS: the workgroup's 32 rows x 512 bytes, written once by all four waves (thread i: 16-byte pieces i, i + 256, ..), row
    // pitch QROW; lane (li, g) reads row 16 nt + li, bytes 64 ks + 16 g .. as its B operand
    const char *q_sh = smem + MAIN + STATS + li * QROW + g * 16;
    if constexpr (Q_LDS) {
#pragma unroll
        for (int i = 0; i < NT * 16 * 32 / THREADS; ++i) {
            const int piece = i * THREADS + threadIdx.x, r = piece >> 5, valid = r < a.rows;
            const int rr = valid ? r : 0, qi = rr / a.group, qh = kvh * a.group + rr % a.group;
            const uint16_t *qp = a.q + (int64_t)b * a.q_bs + (int64_t)qi * a.q_ss + (int64_t)qh * a.q_hs + (piece & 31) * 8;
            *(s16x8 *)(smem + MAIN + STATS + r * QROW + (piece & 31) * 16) = *(const s16x8 *)qp;
        }
        __syncthreads();
    }

    const float scale = 1.0f / 16.0f;   // logits, and c: the exponent of exp2
    const float c = (float)((double)scale * 1.4426950408889634074);
    // CAP: S -> A tanh(S / A) = cap_a + cap_m2a / (exp2(S cap_k) + 1)
    [[maybe_unused]] float cap_a = 0.0f, cap_m2a = 0.0f, cap_k = 0.0f;
    if constexpr (CAP) {
        cap_a = args.cap_a;
        cap_m2a = -2.0f * args.cap_a;
        cap_k = args.cap_inv_a * 2.8853900817779268f;   // 2 log2(e) / A
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

    // One unit's K (8 KT loads) and V (VL loads), 16 bytes per lane and load.  A unit at or beyond u_end (the prefetch behind a
    // wave's last unit) is still loaded, every lane from one row of unit `u_valid`: one cached row instead of the unit's bytes, and
    // the number of loads in flight is the same on every path.  A key below lo_min comes from key lo_min, one at or beyond len from
    // key len - 1.
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
        for (int i = 0; i < VL; ++i) Vr.r[i] = *(const s16x8 *)(a.v + base + (int64_t)(row0 + clamp_key(i * 2 + vr)) * a.kv_ss + vc * 8);
    };

    char *vs = smem + wave * VBYTES;
    char *vwr = vs + vr * VROW + vc * 16;
    const char *vrd = vs + (4 * g + (li >> 2)) * VROW + (li & 3) * 8;   // lane 4 q + p of a group: row q, columns 4 p ..
    auto compute_unit = [&](int u, const KRegs &Kr, const VRegs &Vr) {
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
                for (int nt = 0; nt < NT; ++nt) {
                    vec8 qb;
                    if constexpr (Q_LDS) qb = *(const vec8 *)(q_sh + nt * 16 * QROW + ks * 64);
                    else qb = Qr[nt][ks];
                    S[nt][kt] = E::mfma16(Kr.r[kt][ks], qb, S[nt][kt]);
                }
        vec8 Pb[NT];   // (key tile kt: half kt; a 16-key unit fills the low half)
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
            float p[8] = {}, rowsum = 0.0f;
#pragma unroll
            for (int j = 0; j < 4 * KT; ++j) {
                p[j] = __builtin_amdgcn_exp2f(__builtin_fmaf(s[j], c, neg_mc));
                rowsum += p[j];
            }
            l[nt] += rowsum;
            Pb[nt] = E::pack8(p);
        }
        // a key tile at a time through the wave's 16-key image
#pragma unroll
        for (int kt = 0; kt < KT; ++kt) {
#pragma unroll
            for (int i = 0; i < 8; ++i) *(s16x8 *)(vwr + i * 2 * VROW) = Vr.r[8 * kt + i];
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // the wave's V image is written
#pragma unroll
            for (int t = 0; t < DT16; ++t) {
                const s16x4 av = __builtin_amdgcn_ds_read_tr16_b64_v4i16((FA_LDS(s16x4) *)(vrd + t * 32));
#pragma unroll
                for (int nt = 0; nt < NT; ++nt) {
                    const s16x8 pb = __builtin_bit_cast(s16x8, Pb[nt]);
                    O[nt][t] = mfma16_k16<DT>(av, kt == 0 ? pb.lo : pb.hi, O[nt][t]);
                }
            }
            asm volatile("" ::: "memory");   // ... and read before the next tile's is written
        }
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
        } else {   // a partial: o normalised, lse = -inf for a row that saw no key in this split
            const int64_t row = (((int64_t)split * a.batch + b) * a.n_kv_heads + kvh) * a.rows + r;
            float *pp = a.part_o + row * D + 4 * g;
#pragma unroll
            for (int t = 0; t < DT16; ++t) *(f32x4 *)(pp + 16 * t) = O[nt][t] * inv;
            if (g == 0) a.part_lse[row] = lse;
        }
    }
}

// one workgroup of 64 threads per (batch, K / V head, row); thread i: d 4 i .. 4 i + 3.  Fixed-order sums: mx = max_s lse_s,
// lse = mx + log sum_s exp(lse_s - mx), o = sum_s exp(lse_s - lse) o_s in split order, rounded once; mx = -inf (no key): o = 0, lse = -inf.
template <int DT>
__global__ void __launch_bounds__(64) fa_decode256_combine_kernel(const Decode256Args args) {
    using E = Elem<DT>;
    const DecodeArgs &a = args.d;
    const int64_t row = blockIdx.x, n_rows = (int64_t)a.batch * a.n_kv_heads * a.rows;
    const int r = (int)(row % a.rows), kvh = (int)((row / a.rows) % a.n_kv_heads), b = (int)(row / ((int64_t)a.rows * a.n_kv_heads));
    const int qi = r / a.group, qh = kvh * a.group + r % a.group;
    const float ninf = -__builtin_inff();
    float mx = ninf;
    for (int s = 0; s < a.num_splits; ++s) mx = fmaxf(mx, a.part_lse[s * n_rows + row]);
    float lse = ninf;
    f32x4 o = {0.0f, 0.0f, 0.0f, 0.0f};
    if (mx != ninf) {
        float sum = 0.0f;
        for (int s = 0; s < a.num_splits; ++s) sum += __expf(a.part_lse[s * n_rows + row] - mx);
        lse = mx + __logf(sum);
        for (int s = 0; s < a.num_splits; ++s) {
            const float w = __expf(a.part_lse[s * n_rows + row] - lse);
            const f32x4 v = *(const f32x4 *)(a.part_o + (s * n_rows + row) * decode256::D + 4 * threadIdx.x);
#pragma unroll
            for (int j = 0; j < 4; ++j) o[j] = __builtin_fmaf(w, v[j], o[j]);
        }
    }
    uint16_t *op = a.o + (int64_t)b * a.o_bs + (int64_t)qi * a.o_ss + (int64_t)qh * a.o_hs;
    u32x2 w;
    w[0] = E::pack2(o[0], o[1]);
    w[1] = E::pack2(o[2], o[3]);
    *(u32x2 *)(op + 4 * threadIdx.x) = w;
    if (a.lse && threadIdx.x == 0) a.lse[((int64_t)b * a.n_heads + qh) * a.seqlen_q + qi] = lse;
}

hipError_t decode256_enqueue(const Decode256Args &a, int dtype, bool capped, hipStream_t s);   // fa_decode256.hip

}  // namespace fa
