// fa_fwd_kernel.hpp -- Flash-Attention-2 forward for CDNA4 / gfx950 (MI355X).
//
// Hand-written HIP; not a translation of the reference's CUDA.  It computes what
// /root/reference/src/include/forward_kernel.cuh:85-204 (flash_forward_kernel) and
// :19-83 (process_kv_block) compute -- O = softmax(Q K^T / sqrt(d)) V for one
// (batch, head, Q block) per workgroup, KV blocks visited last-to-first, raw-logit
// running max, base-2 exponent with c = rsqrt(d)*log2(e), P rounded RNE to the
// 16-bit type before P.V, l summed from fp32 P with the cross-lane reduction
// deferred to the epilogue (softmax.cuh:13-128) -- but is organised for wave64 MFMA:
//
//  * Both products are computed TRANSPOSED so every softmax statistic is lane-local:
//      S^T = K  Q^T   v_mfma_f32_32x32x16 (A = K tile rows from LDS, B = Q^T in VGPRs)
//      O^T = V^T P^T  v_mfma_f32_32x32x16 (A = V^T via ds_read_b64_tr_b16, B = P^T)
//    In the 32x32 C layout (col = lane&31, row = (reg&3) + 8*(reg>>2) + 4*(lane>>5))
//    lane L then owns ONE query (column L&31) and 16 keys per 32-key tile; the other
//    16 keys sit in lane L^32.  Row max = in-register max + one v_permlane32_swap;
//    the rescale factor, m and l are per-lane scalars.
//  * The P^T B-operand needs, per lane, keys {8*(lane>>5) + j}; the C layout hands
//    the lane keys {4*(lane>>5) + (j&3) + 8*(j>>2)}.  Since a contraction index may
//    be permuted freely if both operands agree, V^T's A-operand is fetched with the
//    SAME key permutation (two transpose-reads per operand pick keys 4hi+0..3 and
//    8+4hi+0..3).  P therefore goes from the softmax registers straight into the
//    MFMA with just a v_cvt_pk -- no LDS round trip, no cross-lane shuffle.
//  * Q lives in VGPRs for the whole kernel (it IS the B operand layout: 16 B per
//    lane per 16-wide k step), loaded once straight from global memory.
//  * K and V tiles are DMA'd global->LDS (global_load_lds_dwordx4, 1 KiB per
//    wave-instruction), double-buffered, one barrier per KV tile.  The DMA writes
//    LDS lane-linearly, so both LDS images are produced by permuting the per-lane
//    SOURCE address:
//      K image  [key][128 d], 256 B rows, 16-B chunk index XOR (key & 15)  ->
//               conflict-free ds_read_b128 for the A operand (16-lane groups hit 16
//               distinct slots of the 256-B bank row);
//      V image  [key/8][d/32][8 keys][32 d] 512-B subtiles -> every
//               ds_read_b64_tr_b16 wave-instruction reads 512 contiguous bytes, all
//               32 reads of a tile are one base VGPR + immediate offsets.
//  * Workgroup ids are remapped so all Q blocks of one (batch, head) run on the
//    same XCD (block id mod 8) and share that XCD's L2 copy of the head's K/V.
//
// Template parameters select the device variant behind the reference's 13-field
// config (fa_capi.hip maps config -> variant; tools/generate_kernel_instantiations.py lists them):
//   DT      5 = fp16, 15 = bf16 (torch ScalarType codes)
//   QT      32-row Q tiles per wave (rows per wave = 32*QT)
//   NWAVES  wave64 wavefronts per workgroup  (B_r = 32*QT*NWAVES)
//   BC      keys per LDS tile (B_c)
//   SWZ     XOR-swizzled K image             (cfg.swizzled)
//   EAGER   prefetch next tile, 2 LDS buffers (cfg.eager_load_blocks)
//   OPT     the reference's cfg.optimized_softmax -- first KV block skips the rescale -- on the single-stage, register-staged
//           and masked variants; on the double-buffered LDS-DMA variants the speculative softmax (SPEC below), which only
//           fa_fwd_opts.speculative selects (fa_registry.hpp: softmax_mode_of)
//   DMA     K/V tiles by global->LDS DMA (cfg.async_copy = 1, the cp.async analogue) or,
//           DMA = false, through registers: coalesced global_load_dwordx4 issued a visit
//           ahead, written to LDS with ds_write_b128 after the barrier that frees the stage
//   MASK    scope widener beyond the reference: seq_len need not be a multiple
//           of the tiles (keys >= seq_len masked, rows >= seq_len not stored) and an optional
//           causal mask (KV tiles above the diagonal are never visited)
//   PIPE    software-pipelined loop with two S accumulators: while the matrix pipe forms
//           S(i+1) = K(i+1) Q^T and then O += V(i) P(i), the vector ALU turns the finished
//           S(i) into P(i); every MFMA has ~4-5 VALU ops and 1-2 LDS operand reads pinned
//           beside it (cfg.mma_double_buffer_loads; 32 rows per wave, B_c <= 64)
//   ABL     0 in every shipped variant; tools/ablate.hip removes one cost at a time
#pragma once

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>
#include <type_traits>

namespace fa {

struct KernelArgs {
    const void *q;
    const void *k;
    const void *v;
    void *o;
    int64_t batch_stride;  // elements
    int64_t seq_stride;
    int64_t head_stride;
    int32_t seq_len;
    int32_t n_heads;
    int32_t n_bh;          // batch * heads
    int32_t n_q_blocks;
    int32_t n_kv_blocks;
    int32_t causal;        // MASK variants only: key j contributes to query i iff j <= i
    uint32_t *stats = nullptr;  // nullptr, or two device counters the kernel adds to (fa_fwd_stats: items, items_redone)
    // adaptive speculative softmax (fa_fwd_opts.speculative == 2): nullptr, or one word of pinned HOST memory into which a
    // workgroup that had to compute an item twice stores this launch's sequence number -- written only then, so a
    // launch without failures costs nothing; the library reads it, without waiting, at its next launches
    uint32_t *redo_flag = nullptr;
    uint32_t redo_seq = 0;
#ifdef FA_TRACE
    unsigned long long *trace;  // tools/segment_timer.hip only: [wave][visit][8] s_memtime stamps
    int32_t trace_block;
    int32_t trace_visit;        // tools/trace64.hip: the one visit whose gap stamps are recorded
#endif
};

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
typedef short s16x4 __attribute__((ext_vector_type(4)));
typedef short s16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));

#define FA_LDS(type) __attribute__((address_space(3))) type
#define FA_DEV __device__ __forceinline__

// (see KernelArgs::redo_flag)  Every writer of a launch stores the same value: a plain system-scope store, no atomic
FA_DEV void report_redo(const KernelArgs &args) {
    if (args.redo_flag) __hip_atomic_store(args.redo_flag, args.redo_seq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}

template <bool B> struct BoolTag { static constexpr bool value = B; };
template <int I> struct IntTag { static constexpr int value = I; };
// f(IntTag<I>{}) for I = BEGIN .. END-1: unrolled by construction (a `#pragma unroll` loop whose
// unrolled size passes LLVM's pragma threshold is silently left rolled, and every register array
// it indexes then lives in scratch)
template <int BEGIN, int END, class F> __device__ __forceinline__ void static_for(F &&f) {
    if constexpr (BEGIN < END) {
        f(IntTag<BEGIN>{});
        static_for<BEGIN + 1, END>(f);
    }
}

template <int DT> struct Elem;

// Speculative softmax (fa_fwd_opts.speculative): a row of the first pass is accepted when its l = sum of P stays below this.
// Every P of the row is <= l, so below the limit fp32 exp2 did not overflow, the 16-bit P is in range (fp16: P < 65504)
// and the fp32 accumulators hold |O| <= l max|V| -- finite for every fp16 V; for bf16 (|V| up to 2^127) the verdict also
// looks at the accumulators themselves.  bf16: 2^64 (~44 nats above the first visited tile's max), fp16: 2^15 (~10 nats).
// !(l < limit) is also true for NaN and +inf.
template <int DT> __device__ constexpr float spec_limit() { return DT == 5 ? 32768.0f : 18446744073709551616.0f; }
// The persistent kernel's guard (fa_fwd_kernel64.hpp): every four visits a wave looks at its running row sums; a row
// whose sum has passed this threshold (bf16 2^32; fp16 2^13) is brought back to l in [1, 2) -- O and l multiplied by an exact
// power of two, the row's reference moved by as many binades -- so that slowly or moderately rising logits never reach the
// limit at all; only a jump beyond the limit within four visits (256 keys) still fails the item.  fp16: N(0, 1) rows
// reach l ~ 0.15 n on their own (2^11.3 at n = 16384 keys, unlucky rows 2.5x that), and a rescue costs the wave ~700
// instructions: with round 3's 2^11 every wave took it near the end of a 16384-key item and the speculative softmax gained
// nothing there (C3: 1228 vs 1226 lazy); 2^13 leaves the rescues to rows that need them and still two binades below the
// limit 2^15 (a jump of more than 4x inside 256 keys fails either way: profiles/r04/fp16_guard_threshold.txt).
// With the guard the persistent kernel checks O for inf / NaN itself whenever a row sum has passed the threshold, so
// its limit only has to keep P = 2^x finite in fp32 and in the 16-bit type: bf16 2^120 (a single jump of ~83 nats inside
// four visits), fp16 2^15 as above.
template <int DT> __device__ constexpr float spec_limit64() { return DT == 5 ? 32768.0f : 1.329227995784916e36f; }
#ifndef FA_FP16_GUARD
#define FA_FP16_GUARD 8192.0f
#endif
template <int DT> __device__ constexpr float spec_guard() { return DT == 5 ? FA_FP16_GUARD : 4294967296.0f; }

template <> struct Elem<15> {  // bf16
    typedef bf16x8 vec8;
    static FA_DEV f32x16 mfma(vec8 a, vec8 b, f32x16 c) {
        return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0);
    }
    static FA_DEV f32x4 mfma16(vec8 a, vec8 b, f32x4 c) {
        return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
    }
    // Inline-asm MFMA forms with the register FILE of each operand chosen by hand (64-rows-per-
    // wave schedule): accumulator in AGPRs ("a") or VGPRs ("v"), B operand Q resident in AGPRs.
    // hipcc neither schedules nor hazard-pads these: see the call sites for the wait states.
    static FA_DEV void mfma_acc_a_q(f32x16 &acc, vec8 a, vec8 q) {  // acc(AGPR) += a * q(AGPR)
        asm volatile("v_mfma_f32_32x32x16_bf16 %0, %1, %2, %0" : "+a"(acc) : "v"(a), "a"(q));
    }
    static FA_DEV void mfma_acc_a_q0(f32x16 &acc, vec8 a, vec8 q) {  // acc(AGPR) = a * q(AGPR)
        asm volatile("v_mfma_f32_32x32x16_bf16 %0, %1, %2, 0" : "=a"(acc) : "v"(a), "a"(q));
    }
    static FA_DEV void mfma_acc_v_q(f32x16 &acc, vec8 a, vec8 q) {  // acc(VGPR) += a * q(AGPR)
        asm volatile("v_mfma_f32_32x32x16_bf16 %0, %1, %2, %0" : "+v"(acc) : "v"(a), "a"(q));
    }
    static FA_DEV void mfma_acc_v_q0(f32x16 &acc, vec8 a, vec8 q) {
        asm volatile("v_mfma_f32_32x32x16_bf16 %0, %1, %2, 0" : "=v"(acc) : "v"(a), "a"(q));
    }
    static FA_DEV void mfma_acc_v_qc(f32x16 &acc, vec8 a, vec8 q, const f32x16 &cin) {  // acc(VGPR) = a * q(AGPR) + cin(VGPR)
        // "=&v": a 32x32 MFMA needs D and C identical or fully disjoint; without the early clobber the allocator may overlap
        // them partially once cin is dead behind the statement
        asm volatile("v_mfma_f32_32x32x16_bf16 %0, %1, %2, %3" : "=&v"(acc) : "v"(a), "a"(q), "v"(cin));
    }
    static FA_DEV void mfma_acc_a_p(f32x16 &acc, vec8 a, u32x4 p) {  // acc(AGPR) += a * p(VGPR, packed >= 1 step ago)
        asm volatile("v_mfma_f32_32x32x16_bf16 %0, %1, %2, %0" : "+a"(acc) : "v"(a), "v"(p));
    }
    static FA_DEV void mfma_zero_a(f32x16 &acc, vec8 z) {  // acc(AGPR) = z * z + 0 with z = 0: 16 registers cleared by one instruction
        asm volatile("v_mfma_f32_32x32x16_bf16 %0, %1, %1, 0" : "=a"(acc) : "v"(z));
    }
    static FA_DEV unsigned pack2(float x, float y) {  // RNE, low half = x
        typedef __bf16 pair_t __attribute__((ext_vector_type(2)));
        pair_t r;
        r[0] = (__bf16)x;
        r[1] = (__bf16)y;
        return __builtin_bit_cast(unsigned, r);
    }
    // RNE fp32 -> bf16 (v_cvt_pk_bf16_f32), load_store.cuh:345-349 semantics
    static FA_DEV vec8 pack8(const float *p) {
        vec8 r;
#pragma unroll
        for (int j = 0; j < 8; ++j) r[j] = (__bf16)p[j];
        return r;
    }
};

template <> struct Elem<5> {  // fp16
    typedef f16x8 vec8;
    static FA_DEV f32x16 mfma(vec8 a, vec8 b, f32x16 c) {
        return __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b, c, 0, 0, 0);
    }
    static FA_DEV f32x4 mfma16(vec8 a, vec8 b, f32x4 c) {
        return __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, c, 0, 0, 0);
    }
    // Inline-asm MFMA forms with the register FILE of each operand chosen by hand (64-rows-per-
    // wave schedule): accumulator in AGPRs ("a") or VGPRs ("v"), B operand Q resident in AGPRs.
    // hipcc neither schedules nor hazard-pads these: see the call sites for the wait states.
    static FA_DEV void mfma_acc_a_q(f32x16 &acc, vec8 a, vec8 q) {  // acc(AGPR) += a * q(AGPR)
        asm volatile("v_mfma_f32_32x32x16_f16 %0, %1, %2, %0" : "+a"(acc) : "v"(a), "a"(q));
    }
    static FA_DEV void mfma_acc_a_q0(f32x16 &acc, vec8 a, vec8 q) {  // acc(AGPR) = a * q(AGPR)
        asm volatile("v_mfma_f32_32x32x16_f16 %0, %1, %2, 0" : "=a"(acc) : "v"(a), "a"(q));
    }
    static FA_DEV void mfma_acc_v_q(f32x16 &acc, vec8 a, vec8 q) {  // acc(VGPR) += a * q(AGPR)
        asm volatile("v_mfma_f32_32x32x16_f16 %0, %1, %2, %0" : "+v"(acc) : "v"(a), "a"(q));
    }
    static FA_DEV void mfma_acc_v_q0(f32x16 &acc, vec8 a, vec8 q) {
        asm volatile("v_mfma_f32_32x32x16_f16 %0, %1, %2, 0" : "=v"(acc) : "v"(a), "a"(q));
    }
    static FA_DEV void mfma_acc_v_qc(f32x16 &acc, vec8 a, vec8 q, const f32x16 &cin) {  // acc(VGPR) = a * q(AGPR) + cin(VGPR)
        // "=&v": a 32x32 MFMA needs D and C identical or fully disjoint; without the early clobber the allocator may overlap
        // them partially once cin is dead behind the statement
        asm volatile("v_mfma_f32_32x32x16_f16 %0, %1, %2, %3" : "=&v"(acc) : "v"(a), "a"(q), "v"(cin));
    }
    static FA_DEV void mfma_acc_a_p(f32x16 &acc, vec8 a, u32x4 p) {  // acc(AGPR) += a * p(VGPR, packed >= 1 step ago)
        asm volatile("v_mfma_f32_32x32x16_f16 %0, %1, %2, %0" : "+a"(acc) : "v"(a), "v"(p));
    }
    static FA_DEV void mfma_zero_a(f32x16 &acc, vec8 z) {  // acc(AGPR) = z * z + 0 with z = 0: 16 registers cleared by one instruction
        asm volatile("v_mfma_f32_32x32x16_f16 %0, %1, %1, 0" : "=a"(acc) : "v"(z));
    }
    static FA_DEV unsigned pack2(float x, float y) {  // RNE, low half = x
        typedef _Float16 pair_t __attribute__((ext_vector_type(2)));
        pair_t r;
        r[0] = (_Float16)x;
        r[1] = (_Float16)y;
        return __builtin_bit_cast(unsigned, r);
    }
    static FA_DEV vec8 pack8(const float *p) {
        vec8 r;
#pragma unroll
        for (int j = 0; j < 8; ++j) r[j] = (_Float16)p[j];
        return r;
    }
};

// eight e4m3fn values (two dwords, lowest byte first) as eight values of Q's type: exact, every e4m3 value is a bf16 and an fp16
// (the fp8 caches: fa_decode_kernel.hpp, and fa_fwd_kernel_varlen_kvcache_fp8 below)
template <int DT>
static FA_DEV typename Elem<DT>::vec8 cvt_fp8x8(unsigned w0, unsigned w1) {
    u32x4 r;
    if constexpr (DT == 15) {
        r[0] = __builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(w0, 1.0f, false));
        r[1] = __builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(w0, 1.0f, true));
        r[2] = __builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(w1, 1.0f, false));
        r[3] = __builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(w1, 1.0f, true));
    } else {
        r[0] = __builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_scalef32_pk_f16_fp8(w0, 1.0f, false));
        r[1] = __builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_scalef32_pk_f16_fp8(w0, 1.0f, true));
        r[2] = __builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_scalef32_pk_f16_fp8(w1, 1.0f, false));
        r[3] = __builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_scalef32_pk_f16_fp8(w1, 1.0f, true));
    }
    return __builtin_bit_cast(typename Elem<DT>::vec8, r);
}

// a product that keeps its own rounding: never contracted into an fma with the add that consumes it
static FA_DEV float mul_rounded(float a, float b) {
#pragma clang fp contract(off)
    return a * b;
}

// Single-instruction VALU forms for the hand-placed schedule: plain C++ lets hipcc SLP-pack adjacent
// f32 adds into v_pk_add_f32 and canonicalise fmaxf inputs, both slower beside MFMAs.
static FA_DEV float vmax3(float a, float b, float c) {
    float d;
    asm("v_max3_f32 %0, %1, %2, %3" : "=v"(d) : "v"(a), "v"(b), "v"(c));
    return d;
}
static FA_DEV float vmax2(float a, float b) {
    float d;
    asm("v_max_f32 %0, %1, %2" : "=v"(d) : "v"(a), "v"(b));
    return d;
}
static FA_DEV float vadd(float a, float b) {
    float d;
    asm("v_add_f32 %0, %1, %2" : "=v"(d) : "v"(a), "v"(b));
    return d;
}

// max over the two lanes that share a query column (lane, lane^32).
static FA_DEV float pair_max(float x) {
    auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(x), __float_as_uint(x), false, false);
    return fmaxf(__uint_as_float(r[0]), __uint_as_float(r[1]));
}
static FA_DEV float pair_sum(float x) {
    auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(x), __float_as_uint(x), false, false);
    return __uint_as_float(r[0]) + __uint_as_float(r[1]);
}

// 16-byte-per-lane global -> LDS DMA (1 KiB per wave-instruction).  Written as inline
// asm on purpose: hipcc tracks the builtin form as an LDS write and puts a full
// `s_waitcnt vmcnt(0)` in front of the next ds_read of the same __shared__ array,
// which would serialise every prefetch with the compute it is meant to hide under.
// The kernel counts these loads itself: each wave executes dma_wait_all() before the
// barrier that publishes a stage (cdna_hip_programming.md 5.7 item 1).
// LDS destination = M0 (wave-uniform byte address) + lane * 16.
static FA_DEV void glds16(const void *gsrc, unsigned lds_dst_wave_uniform) {
    unsigned keep;  // M0 is compiler-reserved: save / restore it inside the statement
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\t"
                 "global_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep)
                 : "v"(gsrc), "s"(lds_dst_wave_uniform)
                 : "memory");
}
// Same with the address split as SGPR base (wave-uniform: tensor + head + tile offset,
// computed on the scalar ALU) + 32-bit per-lane byte offset: no vector ALU work per piece.
static FA_DEV void glds16_sv(const void *base_wave_uniform, unsigned lane_byte_off,
                             unsigned lds_dst_wave_uniform) {
    unsigned keep;
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 0\n\t"
                 "global_load_lds_dwordx4 %1, %2\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep)
                 : "v"(lane_byte_off), "s"(base_wave_uniform), "s"(lds_dst_wave_uniform)
                 : "memory");
}
// Variant that leaves M0 changed (3 instructions instead of 5).  Only for kernels in which hipcc
// itself never needs M0 (no LDS-DMA builtin, no s_movrel / sendmsg): the 64-row pinned schedule.
// s_nop 3: five wait states between whatever hipcc put in front and the load -- the scalar base may just have come
// back from a VGPR lane (v_readlane: hipcc parks scalars there), and a vector-memory instruction must not read an
// SGPR a vector instruction wrote fewer than 5 wait states earlier; hipcc pads that for its own loads only
// (tools/isa_lint64.py, finding SGPRVM).  Used at the prologue and the item seams, not in the steady-state visits.
static FA_DEV void glds16_sv_m0(const void *base_wave_uniform, unsigned lane_byte_off,
                                unsigned lds_dst_wave_uniform) {
    asm volatile("s_mov_b32 m0, %2\n\ts_nop 3\n\tglobal_load_lds_dwordx4 %0, %1"
                 :
                 : "v"(lane_byte_off), "s"(base_wave_uniform), "s"(lds_dst_wave_uniform)
                 : "memory");
}
// ... and with the M0 write split off (the caller wrote M0 at least one instruction earlier)
static FA_DEV void glds16_issue(const void *base_wave_uniform, unsigned lane_byte_off) {
    asm volatile("global_load_lds_dwordx4 %0, %1" : : "v"(lane_byte_off), "s"(base_wave_uniform) : "memory");
}
// The same three with an IMMEDIATE offset (round 6).  The instruction adds it to the global address AND to the LDS
// destination (measured: M0 = base + 2048, offset:1024 lands at base + 3072 what lies 1024 bytes behind the lane's
// address), so the pieces of one tile that a wave requests can share ONE M0 value when they are neighbours in the LDS
// image: destination = M0 + 1024 j, the lane offsets carry -1024 j to compensate (fa_fwd_kernel64.hpp).
template <int OFF> static FA_DEV void glds16_sv_off(const void *base_wave_uniform, unsigned lane_byte_off, unsigned lds_dst_wave_uniform) {
    static_assert(OFF >= 0 && OFF < 4096, "13-bit signed immediate");
    unsigned keep;
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 0\n\t"
                 "global_load_lds_dwordx4 %1, %2 offset:%4\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep)
                 : "v"(lane_byte_off), "s"(base_wave_uniform), "s"(lds_dst_wave_uniform), "n"(OFF)
                 : "memory");
}
template <int OFF> static FA_DEV void glds16_sv_m0_off(const void *base_wave_uniform, unsigned lane_byte_off, unsigned lds_dst_wave_uniform) {
    static_assert(OFF >= 0 && OFF < 4096, "13-bit signed immediate");
    asm volatile("s_mov_b32 m0, %2\n\ts_nop 3\n\tglobal_load_lds_dwordx4 %0, %1 offset:%3"
                 :
                 : "v"(lane_byte_off), "s"(base_wave_uniform), "s"(lds_dst_wave_uniform), "n"(OFF)
                 : "memory");
}
template <int OFF> static FA_DEV void glds16_issue_off(const void *base_wave_uniform, unsigned lane_byte_off) {
    static_assert(OFF >= 0 && OFF < 4096, "13-bit signed immediate");
    asm volatile("global_load_lds_dwordx4 %0, %1 offset:%2" : : "v"(lane_byte_off), "s"(base_wave_uniform), "n"(OFF) : "memory");
}
static FA_DEV void dma_wait_all() { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); }
// workgroup barrier that the compiler may not move LDS traffic across and that does
// not drain VMEM (in-flight DMA survives it)
static FA_DEV void wg_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }
#ifdef FA_TRACE
#define FA_STAMP(visit, k)                                                                  \
    do {                                                                                    \
        if (blockIdx.x == (unsigned)args.trace_block && visit < 64) {                       \
            unsigned long long t_;                                                          \
            asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t_)::"memory");      \
            if (lane == 0) args.trace[(wave * 64 + (visit)) * 8 + (k)] = t_;                \
        }                                                                                   \
    } while (0)
#else
#define FA_STAMP(visit, k) do { } while (0)
#endif

// Instruction-group pins for the LLVM scheduler (mask: 0x8 MFMA, 0x100 DS read).
// Left alone, hipcc feeds each MFMA from an LDS read issued one or two instructions
// earlier, so every MFMA eats the LDS latency (measured 57 cycles per MFMA instead of
// 32).  These sequences keep `depth` operand reads in flight ahead of the matrix pipe.
template <int N_MFMA, int READS_PER_MFMA, int DEPTH>
static FA_DEV void sched_mfma_fed_from_lds() {
    constexpr int kReads = N_MFMA * READS_PER_MFMA;
    constexpr int kPre = DEPTH < kReads ? DEPTH : kReads;
    __builtin_amdgcn_sched_group_barrier(0x100, kPre, 0);
#pragma unroll
    for (int i = 0; i < N_MFMA; ++i) {
        __builtin_amdgcn_sched_group_barrier(0x8, 1, 0);
        if (kPre + (i + 1) * READS_PER_MFMA <= kReads)
            __builtin_amdgcn_sched_group_barrier(0x100, READS_PER_MFMA, 0);
    }
}

static FA_DEV unsigned lds_addr(const char *p) {
    return (unsigned)(unsigned long long)(FA_LDS(const char) *)p;
}

template <int DT, int QT, int NWAVES, int BC, bool SWZ, bool EAGER, bool OPT, bool PIPE, bool DMA = true,
          bool MASK = false, int D = 128, int KSPLIT = 1>
struct FwdTraits {
    static_assert(!PIPE || EAGER, "the pipelined loop needs both LDS stages");
    static_assert(DMA || EAGER, "register-staged tiles are only built double-buffered");
    static_assert(D == 128 || D == 64, "d_head 128 (the reference's scope) or 64 (widener)");
    static_assert(DMA || D == 128, "the register-staged transport is only built for d_head 128");
    static constexpr int kRowsPerWave = 32 * QT;
    static constexpr int kBr = kRowsPerWave * NWAVES / KSPLIT;  // KSPLIT waves share a row group (key split)
    static constexpr int kBc = BC;
    static constexpr int kThreads = NWAVES * 64;
    static constexpr int kTileBytes = BC * 2 * D;               // one K or V tile
    // LDS ring depth per tensor: 4 for the 64-rows-per-wave schedule (tiles fetched 3 visits ahead)
    static constexpr int kStages = (QT == 2 && PIPE) ? 4 : (EAGER ? 2 : 1);
    static constexpr int kKvBytes = 2 * kStages * kTileBytes;   // K + V, all stages
    static constexpr int kOutBytes = kBr * 2 * D;               // O tile staged for the epilogue
    // The 64-rows-per-wave schedule is a PERSISTENT kernel: one workgroup per CU walks the
    // (batch*head, Q block) items and keeps the K/V tile stream running across item seams, so its
    // O staging (8 KB per wave, one 32-row Q tile at a time) lives beside the rings, not in them.
    static constexpr bool kPersistent = (QT == 2 && PIPE);
    // key split: 16 KB of 16-bit row staging + per row group 16 KB of fp32 O and (m, l) handed over in the epilogue
    static constexpr int kMergeBytes = KSPLIT == 2 ? 2 * kRowsPerWave * 2 * D + 2 * (kRowsPerWave * D * 4 + 2 * 64 * 4) : 0;
    static constexpr int kPlainBytes = kKvBytes > kOutBytes ? kKvBytes : kOutBytes;
    static constexpr int kLdsBytes = kPersistent ? kKvBytes + NWAVES * 32 * 2 * D
                                                 : (kPlainBytes > kMergeBytes ? kPlainBytes : kMergeBytes);
};

// VARLEN (packed variable-length sequences, the training path: fa_fwd_launch_varlen, fa_fwd_launch_varlen_qk):
// fa_fwd_kernel_varlen is the body of fa_fwd_kernel whose workgroup finds its sequence's rows in cu_seqlens on the device,
// addresses K / V with a head count and strides of their own (grouped-query attention) and also writes the row log-sum-exp.
// Only fa_inst_varlen.hip names a form (FA_VARLEN_KEYS / FA_VARLEN_EXTRA below, from which FA_KERNEL_VARLEN and its siblings
// follow), and gets that form's kernel INSTEAD of fa_fwd_kernel (MASK forms only): the
// product's kernels keep their names and, compiled from the same text, their code.  FA_KV_SS32 is the K / V seq stride in
// the body.
// Sequence i owns query rows cu_seqlens[i] .. of q / o / lse (the range KernelArgsVarlen describes) and key rows
// cu_seqlens_k[i] .. of k / v; each range is clamped against its own total and max_seqlen (first row in [0, total], length in
// [0, min(max_seqlen, what is left)]).  The causal diagonal is bottom-right aligned: query r sees keys j <= r + (len_k -
// len_q) -- FA_SHIFTED(row) is the last key a row sees.  A row that sees no key gives o = 0, lse = -inf.
// fa_fwd_launch_varlen is the launch whose two ranges are one.
struct KernelArgsVarlen {
    KernelArgs base;             // q, k, v, o; Q's and O's seq (token) and head strides; n_heads; n_bh = n_seqs * n_heads;
                                 // n_q_blocks = ceil(max_seqlen / B_r); causal.  batch_stride, seq_len, n_kv_blocks: unused
    const int32_t *cu_seqlens;   // n_seqs + 1 row offsets (DEVICE); sequence i owns rows cu_seqlens[i] .. cu_seqlens[i + 1] - 1
    float *lse;                  // (n_heads, total_tokens) fp32
    int64_t kv_seq_stride, kv_head_stride;   // K, V: n_heads / group heads (elements)
    int32_t group;               // query heads per K / V head
    int32_t total_tokens, max_seqlen;
};
struct KernelArgsVarlenQK {
    KernelArgsVarlen v;            // cu_seqlens, total_tokens, max_seqlen: the QUERY side; n_q_blocks = ceil(max_seqlen_q / B_r)
    const int32_t *cu_seqlens_k;   // n_seqs + 1 row offsets of k / v (DEVICE)
    int32_t total_k, max_seqlen_k;
};
typedef void (*kernel_fn_varlen)(const KernelArgsVarlenQK);
// VARLEN against a KV cache (prefill behind a cached prefix: fa_fwd_launch_varlen_kvcache): fa_fwd_kernel_varlen_kvcache is
// fa_fwd_kernel_varlen whose sequence b takes its key rows from a cache instead of a packed range.  Key side 1 defines
// FA_KERNEL_VARLEN_KVCACHE (beside FA_KERNEL_VARLEN) and gives that kernel INSTEAD of
// fa_fwd_kernel_varlen.  len_k = cache_seqlens[b], clamped to [0, max_len]; tile t (keys 64 t ..) lies at
//   page_stride * entry + (t % tiles_per_page) * 64 * kv_seq_stride + kv_head * kv_head_stride      (elements from k / v)
// with entry = clamp(block_table[b][t / tiles_per_page], 0, num_pages - 1), or = b for a contiguous cache (block_table null:
// page_stride is the batch stride and tiles_per_page covers the whole cache, so the page index is always 0).  A tile lies in one
// page (page_size % 64 == 0), so only this workgroup-uniform base differs from the packed kernel; the per-lane offsets, the
// ragged-tile rule (rows beyond len_k are fetched from row len_k - 1, the same tile, the same page), the masks, the MFMA /
// softmax body and the epilogue are its text.  Only table entries of pages below ceil(len_k / page_size) are read.
struct KernelArgsVarlenKVCache {
    KernelArgsVarlen v;            // the QUERY side, as in KernelArgsVarlenQK; kv_seq_stride, kv_head_stride: the cache's
    const int32_t *cache_seqlens;  // (n_seqs) valid keys per sequence (DEVICE)
    const int32_t *block_table;    // (n_seqs, bt_stride) page numbers (DEVICE), or null: contiguous cache
    int64_t page_stride;           // elements between pages (contiguous cache: between batch entries)
    int32_t bt_stride, num_pages;
    int32_t tiles_per_page;        // page_size / 64 (contiguous cache: ceil(seqlen_cache / 64))
    int32_t max_len;               // min(capacity, max_seqlen_k)
};
typedef void (*kernel_fn_varlen_kvcache)(const KernelArgsVarlenKVCache);
// ... against an fp8 (e4m3fn) cache (fa_fwd_launch_varlen_kvcache_fp8): fa_fwd_kernel_varlen_kvcache_fp8 is
// fa_fwd_kernel_varlen_kvcache with one more way to FETCH a tile.  Key side 2 defines
// FA_KERNEL_VARLEN_KVCACHE_FP8 (beside the other two) and gives that kernel INSTEAD; `if constexpr (FP8)` (or an #ifdef arm where
// a name exists in one form only) marks every site where the two differ.  k and v hold one byte per element, so the cache's
// strides count bytes.  The DMA cannot convert, so the tiles take the register-staged transport (DMA == false) with the
// conversion between the load and the LDS write: the LDS images are byte for byte what the DMA builds from the dequantized
// cache, and everything behind them is the 16-bit kernel's.  Key j of sequence b, K / V head g stands for
// float(k8[j]) * k_descale[b][g], likewise V: k_descale goes into the exponent's constant c (S and the running max stay raw
// logits), v_descale into the final 1 / l.  No address depends on either.
struct KernelArgsVarlenKVCacheFp8 {
    KernelArgsVarlenKVCache c;            // k, v: the fp8 bytes; kv_seq_stride, kv_head_stride, page_stride: bytes
    const float *k_descale, *v_descale;   // (n_seqs, n_kv_heads) fp32 (DEVICE), row stride ds_bs; null = 1
    int64_t ds_bs;
};
typedef void (*kernel_fn_varlen_kvcache_fp8)(const KernelArgsVarlenKVCacheFp8);
// A sliding window on any of the three (fa_fwd_launch_varlen_qk_window, fa_fwd_launch_varlen_kvcache_window,
// fa_fwd_launch_varlen_kvcache_fp8_window): the form's arguments and (left, right), -1 = unbounded, causal arriving as right = 0
// (args.causal then only orders the Q blocks).  Extra 1 defines FA_KERNEL_VARLEN_WINDOW beside the key side's
// macros and gives fa_fwd_kernel_varlen*_window INSTEAD; `if constexpr (WIN)` or an #ifdef arm marks every site that differs
// (DESIGN.md 10.13).  Query row r of sequence b sits at position p = r + (len_k - len_q) and sees the keys
// lo_r = max(0, p - left) .. hi_r = min(len_k - 1, p + right); a row with hi_r < lo_r (p + right < 0) gives o = 0, lse = -inf.
// Both bounds grow with r, so a workgroup owning rows r0 .. r1 visits the tiles hi_r1 / 64 down to lo_r0 / 64 and nothing else:
// n_kv stays "top tile + 1" (the tile arithmetic: kv0, ragged_rows, FA_ST_TILE), FA_N_VISITS is the visit count every
// comparison against `it` uses (n_kv itself in the other forms).  No key below the workgroup's floor lo_r0 is fetched: in
// the floor tile a lane whose row lies below it fetches row lo_r0 (the same tile, the same page) and is masked, as rows at or
// beyond len_k fetch row len_k - 1; no table entry of a page wholly below the floor is read.
template <class A> struct Windowed {
    A a;
    int32_t left, right;
};
typedef Windowed<KernelArgsVarlenQK> KernelArgsVarlenWindow;
typedef Windowed<KernelArgsVarlenKVCache> KernelArgsVarlenKVCacheWindow;
typedef Windowed<KernelArgsVarlenKVCacheFp8> KernelArgsVarlenKVCacheFp8Window;
typedef void (*kernel_fn_varlen_window)(const KernelArgsVarlenWindow);
typedef void (*kernel_fn_varlen_kvcache_window)(const KernelArgsVarlenKVCacheWindow);
typedef void (*kernel_fn_varlen_kvcache_fp8_window)(const KernelArgsVarlenKVCacheFp8Window);
// Logit soft-capping on the packed forward (fa_fwd_launch_varlen_qk_softcap): the logit of a key a row sees is
// softcap tanh(s / softcap), s = q . k / sqrt(d).  Extra 2 defines FA_KERNEL_VARLEN_SOFTCAP beside the windowed
// slice's two macros and gives fa_fwd_kernel_varlen_softcap INSTEAD of fa_fwd_kernel_varlen_window: the windowed text (a window of
// (-1, -1) runs through it) with one more step, FA_CAP_S, on every S tile right behind qk() and in front of the masks -- a masked
// key stays -inf (tanh(-inf) = -1 would bring it back to life).  The step replaces the raw S = q . k by A tanh(S / A),
// A = softcap sqrt(d), so c, the running max, alpha and the lse line behind it stand as they are.  The host passes A and 1 / A.
struct KernelArgsVarlenSoftcap {
    KernelArgsVarlenWindow w;
    float cap_a, cap_inv_a;
};
typedef void (*kernel_fn_varlen_softcap)(const KernelArgsVarlenSoftcap);
// ... and on both cache prefills (fa_fwd_launch_varlen_kvcache_softcap, fa_fwd_launch_varlen_kvcache_fp8_softcap):
// extra 2 on key side 1 or 2 defines FA_KERNEL_VARLEN_SOFTCAP beside the windowed
// cache slice's macros and gives fa_fwd_kernel_varlen_kvcache_softcap / fa_fwd_kernel_varlen_kvcache_fp8_softcap INSTEAD of the windowed
// kernel.  16-bit cache: the same step.  fp8 cache: a tanh between S and the exponent forbids folding k_descale into c, so the
// descale goes into the cap's constant instead, cap_k = k_descale 2 log2(e) / A (one scalar per workgroup): the capped S is in the
// 16-bit form's units, c is the plain constant and the lse line is the 16-bit form's.
template <class W> struct Softcapped {
    W w;
    float cap_a, cap_inv_a;
};
typedef Softcapped<KernelArgsVarlenKVCacheWindow> KernelArgsVarlenKVCacheSoftcap;
typedef Softcapped<KernelArgsVarlenKVCacheFp8Window> KernelArgsVarlenKVCacheFp8Softcap;
typedef void (*kernel_fn_varlen_kvcache_softcap)(const KernelArgsVarlenKVCacheSoftcap);
typedef void (*kernel_fn_varlen_kvcache_fp8_softcap)(const KernelArgsVarlenKVCacheFp8Softcap);
// A learned attention sink on the packed forward (fa_fwd_launch_varlen_qk_sinks): query head h carries one more
// logit z = sinks[h] that joins the softmax's denominator and has no value vector,
//   lse = ln(exp(z) + sum_j exp(s_j)),   o = sum_j exp(s_j - lse) v_j;   z = -inf: no sink for that head.
// Extra 3 defines FA_KERNEL_VARLEN_SINKS beside the windowed slice's two macros and gives fa_fwd_kernel_varlen_sinks INSTEAD of
// fa_fwd_kernel_varlen_window: the windowed text (a window of (-1, -1) runs through it) whose loop is untouched.  Two sites differ:
// the n_kv == 0 exit writes lse = z, and the end of an item folds the sink into l (sink_end below: the lse line and the
// epilogue's 1 / l).  A row that saw no key (l = 0) gives o = 0 and lse = z exactly.  sinks[h] is a workgroup-uniform load made
// at the end, not held across the loop.  Built for packed keys only.
template <class W> struct Sunk {
    W w;
    const float *sinks;   // (n_heads) fp32 (DEVICE)
};
typedef Sunk<KernelArgsVarlenWindow> KernelArgsVarlenSinks;
typedef void (*kernel_fn_varlen_sinks)(const KernelArgsVarlenSinks);
static_assert(std::is_standard_layout<KernelArgsVarlenSinks>::value && offsetof(KernelArgsVarlenSinks, w) == 0,
              "packed: sinks > window > QK");
// Every wrapper's first member sits at offset 0, so the widest struct of a key side starts with the arguments of each narrower form:
// the host fills that one struct and passes the address of the member the chosen kernel takes (fa_capi.hip, fwd_launch_varlen).
// (KernelArgsVarlenSoftcap repeats Softcapped<KernelArgsVarlenWindow> field for field; it stays a struct of its own because its
// name is part of fa_fwd_kernel_varlen_softcap's mangled name.)
static_assert(std::is_standard_layout<KernelArgsVarlenSoftcap>::value && std::is_standard_layout<KernelArgsVarlenKVCacheSoftcap>::value &&
                  std::is_standard_layout<KernelArgsVarlenKVCacheFp8Softcap>::value,
              "the varlen forms' arguments are standard layout");
static_assert(offsetof(KernelArgsVarlenSoftcap, w) == 0 && offsetof(KernelArgsVarlenWindow, a) == 0, "packed: softcap > window > QK");
static_assert(offsetof(KernelArgsVarlenKVCacheSoftcap, w) == 0 && offsetof(KernelArgsVarlenKVCacheWindow, a) == 0,
              "cache: softcap > window > cache");
static_assert(offsetof(KernelArgsVarlenKVCacheFp8Softcap, w) == 0 && offsetof(KernelArgsVarlenKVCacheFp8Window, a) == 0 &&
                  offsetof(KernelArgsVarlenKVCacheFp8, c) == 0,
              "fp8 cache: softcap > window > fp8 > cache");

// The form a translation unit builds is named once, by two numbers on its command line (fa_inst_varlen.hip, csrc/Makefile):
//   FA_VARLEN_KEYS   0 packed keys (cu_seqlens_k) | 1 a KV cache | 2 an fp8 KV cache
//   FA_VARLEN_EXTRA  0 nothing | 1 a sliding window | 2 a sliding window and logit soft-capping |
//                    3 a sliding window and attention sinks (packed keys only)
// The FA_KERNEL_VARLEN_* macros of the body's arms, the kernel's name (FA_VARLEN_NAME(fa_fwd_kernel_varlen, )) and its argument
// follow from them here: a new key side or extra is one arm below, one in front of the kernel's body, and its arms in the body.
#ifdef FA_VARLEN_KEYS
#define FA_KERNEL_VARLEN
#if FA_VARLEN_KEYS == 0
#define FA_VARLEN_KEYS_SFX
#define FA_VARLEN_KEY_ARGS KernelArgsVarlenQK
#define FA_VARLEN_KEY_PARAM qa
#define FA_VARLEN_CAP_ARGS KernelArgsVarlenSoftcap
#elif FA_VARLEN_KEYS == 1
#define FA_KERNEL_VARLEN_KVCACHE
#define FA_VARLEN_KEYS_SFX _kvcache
#define FA_VARLEN_KEY_ARGS KernelArgsVarlenKVCache
#define FA_VARLEN_KEY_PARAM qa
#define FA_VARLEN_CAP_ARGS KernelArgsVarlenKVCacheSoftcap
#elif FA_VARLEN_KEYS == 2
#define FA_KERNEL_VARLEN_KVCACHE
#define FA_KERNEL_VARLEN_KVCACHE_FP8
#define FA_VARLEN_KEYS_SFX _kvcache_fp8
#define FA_VARLEN_KEY_ARGS KernelArgsVarlenKVCacheFp8
#define FA_VARLEN_KEY_PARAM fa8   // (qa is its cache member)
#define FA_VARLEN_CAP_ARGS KernelArgsVarlenKVCacheFp8Softcap
#else
#error "FA_VARLEN_KEYS: 0 = packed, 1 = KV cache, 2 = fp8 KV cache"
#endif
#if FA_VARLEN_EXTRA == 0
#define FA_VARLEN_EXTRA_SFX
#elif FA_VARLEN_EXTRA == 1
#define FA_KERNEL_VARLEN_WINDOW
#define FA_VARLEN_EXTRA_SFX _window
#elif FA_VARLEN_EXTRA == 2
#define FA_KERNEL_VARLEN_WINDOW
#define FA_KERNEL_VARLEN_SOFTCAP
#define FA_VARLEN_EXTRA_SFX _softcap
#elif FA_VARLEN_EXTRA == 3
#if FA_VARLEN_KEYS != 0
#error "FA_VARLEN_EXTRA 3 (attention sinks) is built for packed keys only (FA_VARLEN_KEYS 0)"
#endif
#define FA_KERNEL_VARLEN_WINDOW
#define FA_KERNEL_VARLEN_SINKS
#define FA_VARLEN_EXTRA_SFX _sinks
#else
#error "FA_VARLEN_EXTRA: 0 = none, 1 = sliding window, 2 = sliding window and soft-capping, 3 = sliding window and sinks"
#endif
#define FA_CAT4_(a, b, c, d) a##b##c##d
#define FA_CAT4(a, b, c, d) FA_CAT4_(a, b, c, d)
#define FA_VARLEN_NAME(pre, post) FA_CAT4(pre, FA_VARLEN_KEYS_SFX, FA_VARLEN_EXTRA_SFX, post)   // e.g. pre_kvcache_fp8_softcap post
#endif
#ifdef FA_KERNEL_VARLEN_SOFTCAP   // (built on the windowed forms: extra 2 defines both)
#define FA_CAP_S(S) cap_S(S)
#else
#define FA_CAP_S(S)
#endif
#ifdef FA_KERNEL_VARLEN_WINDOW
#define FA_VARLEN_WINDOW true
#define FA_N_VISITS n_vis
#else
#define FA_VARLEN_WINDOW false
#define FA_N_VISITS n_kv
#endif
#ifdef FA_KERNEL_VARLEN_KVCACHE_FP8
#define FA_FP8_CACHE true
#define FA_ST_SS32 kv_ss   // the K / V seq stride of the register-staged transport: the cache's (bytes) ...
#ifdef FA_KERNEL_VARLEN_SOFTCAP
// (soft-capped: k_descale sits in the cap's constant, so c and the lse line are the 16-bit form's)
#define FA_K_DESCALED(c0) c0
#define FA_LSE_M_TIMES_C(m, c) m * c
#else
#define FA_K_DESCALED(c0) (fa8.k_descale ? (c0) * fa8.k_descale[(int64_t)b * fa8.ds_bs + h / va.group] : (c0))
// m c of the LSE line, rounded before log2 l is added.  With c a compile-time constant (every other form) hipcc moves the
// product into finite_or_zero's select, which keeps it from contracting with the add; with c a run-time value (c0 k_descale)
// it would form fma(m, c, log2 l) and lse would differ from the 16-bit cache's in the last bit.
#define FA_LSE_M_TIMES_C(m, c) mul_rounded(m, c)
#endif
#else
#define FA_FP8_CACHE false
#define FA_K_DESCALED(c0) c0
#define FA_LSE_M_TIMES_C(m, c) m * c
#define FA_ST_SS32 ss      // ... or the dense kernels', Q's (no other varlen form is built on that transport: the static_assert)
#endif
// the register-staged transport's tile: the fp8 cache's is found by the walk (the caller passes its base), a tensor's by its number
#ifdef FA_KERNEL_VARLEN_KVCACHE_FP8
#define FA_ST_TILE(tensor, it) (tensor)
#else
#define FA_ST_TILE(tensor, it) tensor + (int64_t)(n_kv - 1 - it) * tile_stride
#endif
#ifdef FA_KERNEL_VARLEN
#define FA_KV_SS32 kv_ss
#define FA_SEQ_LEN v_seq_len
#define FA_N_KV_BLOCKS ((v_seq_len + BC - 1) / BC)
#define FA_Q_LEN q_len
#define FA_Q_LEN_END q_len_v
#define FA_SHIFTED(row) ((row) + kq_shift)
#else
#define FA_KV_SS32 ss
#define FA_SEQ_LEN args.seq_len
#define FA_N_KV_BLOCKS args.n_kv_blocks
#define FA_Q_LEN S_len
#define FA_Q_LEN_END S_len
#define FA_SHIFTED(row) (row)
#endif

// ---------------------------------------------------------------------------------
// The kernel.  d_head = 128 is the reference's scope (README.md:7-15); D = 64 is a widener.
// ---------------------------------------------------------------------------------
// ABL (tools/ablate.hip only; 0 in every shipped variant) removes one cost at a time to
// attribute cycles: 1 no v_exp, 2 no softmax VALU at all, 4 no LDS operand reads,
// 8 no barriers / DMA waits, 16 no DMA, 32 plain loads instead of DMA (data discarded);
// experiments: 64 s_setprio(1) around the MFMA clusters (-3 %), 128 operand prefetch 12 deep
// (no change).  Results are wrong by construction when ABL & 63 != 0.
// KSPLIT = 2 (the reference's (B_r 64, B_c 64, 4 warps) configs): B_r / n_warps = 16 rows per wave would
// mean 16x16x32 MFMAs whose K / V operands feed ONE 16-cycle MFMA each -- 256 B/clk of LDS reads per CU
// at full matrix rate, the whole LDS bandwidth.  So the four waves are two row groups of 32 rows x two KEY
// groups instead: wave w works on rows 32 (w & 1) .. +31 and on the 32-key half (w >> 1) of every 64-key
// LDS tile with 32x32x16 MFMAs (half the LDS bytes per flop), keeps its own (m, l, O) over its half of
// the keys, and the two partial results of a row group are merged once, in the epilogue, through LDS
// (the in-workgroup form of a split-KV reduction: m = max, l and O rescaled to it and added).
template <int DT, int QT, int NWAVES, int BC, bool SWZ, bool EAGER, bool OPT, bool PIPE, bool DMA = true,
          bool MASK = false, int D = 128, int ABL = 0, int KSPLIT = 1>
__global__ void
#ifdef FA_KERNEL_VARLEN
// (one workgroup per SIMD set: with m live up to the LSE store the 256-register budget of two waves per SIMD spills)
__launch_bounds__(NWAVES * 64, 1)
// (the argument by the extra, sa > wa > the key side's, which is qa itself or, against an fp8 cache, fa8 > qa)
#if FA_VARLEN_EXTRA == 2
FA_VARLEN_NAME(fa_fwd_kernel_varlen, )(const FA_VARLEN_CAP_ARGS sa) {
    const Windowed<FA_VARLEN_KEY_ARGS> &wa = sa.w;
    const FA_VARLEN_KEY_ARGS &FA_VARLEN_KEY_PARAM = wa.a;
#elif FA_VARLEN_EXTRA == 3
FA_VARLEN_NAME(fa_fwd_kernel_varlen, )(const Sunk<Windowed<FA_VARLEN_KEY_ARGS>> sa) {
    const Windowed<FA_VARLEN_KEY_ARGS> &wa = sa.w;
    const FA_VARLEN_KEY_ARGS &FA_VARLEN_KEY_PARAM = wa.a;
#elif FA_VARLEN_EXTRA == 1
FA_VARLEN_NAME(fa_fwd_kernel_varlen, )(const Windowed<FA_VARLEN_KEY_ARGS> wa) {
    const FA_VARLEN_KEY_ARGS &FA_VARLEN_KEY_PARAM = wa.a;
#else
FA_VARLEN_NAME(fa_fwd_kernel_varlen, )(const FA_VARLEN_KEY_ARGS FA_VARLEN_KEY_PARAM) {
#endif
#if FA_VARLEN_KEYS == 2
    const KernelArgsVarlenKVCache &qa = fa8.c;
#endif
    // (the fp8 cache's form: the same kernel on the register-staged transport, which can convert)
    static_assert(MASK && DMA != FA_FP8_CACHE && KSPLIT == 1 && ABL == 0 && QT == 1,
                  "the varlen form is the masked LDS-DMA kernel; against an fp8 cache, the masked register-staged one");
    const KernelArgsVarlen &va = qa.v;  // (the query side)
    const KernelArgs &args = va.base;   // (seq_len and n_kv_blocks are the sequence's: FA_SEQ_LEN, FA_N_KV_BLOCKS)
#else
__launch_bounds__(NWAVES * 64, (QT == 1) ? 2 : 1)
fa_fwd_kernel(const KernelArgs args) {
#endif
    using E = Elem<DT>;
    using vec8 = typename E::vec8;
    using TR = FwdTraits<DT, QT, NWAVES, BC, SWZ, EAGER, OPT, PIPE, DMA, MASK, D, KSPLIT>;
    enum : bool { FP8 = FA_FP8_CACHE };      // K / V are e4m3fn bytes (fa_fwd_kernel_varlen_kvcache_fp8 only)
    enum : bool { WIN = FA_VARLEN_WINDOW };  // a sliding window (the fa_fwd_kernel_varlen*_window forms only)
    static_assert(!FP8 || (D == 128 && BC == 64 && NWAVES == 4), "the fp8 transport is built for 64-key tiles of d_head 128, four waves");
    static_assert(KSPLIT == 1 || (KSPLIT == 2 && NWAVES == 4 && QT == 1 && BC == 64 && DMA && !MASK && D == 128),
                  "the key split is built for (B_r 64, B_c 64, 4 waves)");
    constexpr int ROWB = 2 * D;              // bytes per K / V / O row (256, or 128 at d_head 64)
    constexpr int CPR = D / 8;               // 16-B chunks per row (16 / 8)
    constexpr int RPP = 64 / CPR;            // tile rows per 1-KiB DMA piece (4 / 8)
    constexpr int DSUB = D / 32;             // 32-wide d subtiles per key group of the V image
    // row -> XOR mask of the 16-B chunk index: 16 consecutive rows must land on 16 distinct
    // 16-B slots of the 256-B LDS bank row (d_head 64: two rows share a bank row)
    auto swz_of = [](int row) { return D == 128 ? (row & 15) : ((row >> 1) & 7); };
    constexpr int NT = BC / 32;              // 32-key tiles per LDS tile
    constexpr int NTW = NT / KSPLIT;         // ... of which this wave works on NTW, from tile NT0 on
    constexpr int KS = D / 16;               // k steps of the QK^T contraction
    constexpr int DTILES = D / 32;           // 32-wide d tiles of O^T
    constexpr int TILE = TR::kTileBytes;
    constexpr int N_DMA = BC / RPP;          // 1-KiB DMA pieces per K (or V) tile
    static_assert(N_DMA % NWAVES == 0, "tile/wave split");
    constexpr int DMA_PER_WAVE = N_DMA / NWAVES;
#ifdef FA_NO_SCHED
    constexpr bool SCHED = false;
#else
    constexpr bool SCHED = (QT == 1);
#endif

    extern __shared__ __attribute__((aligned(16))) char smem[];
    // LDS carve: K stage 0 | K stage 1 | V stage 0 | V stage 1
    constexpr int V_BASE = TR::kStages * TILE;

    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int r31 = lane & 31;
    const int hi = lane >> 5;
    const int wave_r = KSPLIT == 2 ? (wave & 1) : wave;   // row group of this wave
    const int NT0 = KSPLIT == 2 ? (wave >> 1) * NTW : 0;  // first 32-key tile (of an LDS tile) of its key group

    // ---- workgroup -> (batch*head, Q block); XCD-aware when n_bh % 8 == 0 --------
    const int nq = args.n_q_blocks;
    // item -> (batch*head, Q block).  Workgroups are dealt round-robin over the 8 XCDs, so items
    // congruent mod 8 share an L2: give each XCD whole heads (all Q blocks of a head read the same
    // K / V).
    auto item_coords = [&](int bid, int &bh_out, int &qb_out) {
        if ((args.n_bh & 7) == 0) {
            const int xcd = bid & 7, local = bid >> 3;
            bh_out = (local / nq) * 8 + xcd;
            qb_out = local % nq;
        } else {
            bh_out = bid / nq;
            qb_out = bid % nq;
        }
    };
    int bh, qb;
    item_coords(blockIdx.x, bh, qb);
    if (MASK && args.causal) qb = nq - 1 - qb;  // longest rows first
    const int b = bh / args.n_heads, h = bh % args.n_heads;
    const int64_t ss = args.seq_stride;
    typedef std::conditional_t<FA_FP8_CACHE, uint8_t, uint16_t> kv_elem;   // what a K / V stride counts
#ifdef FA_KERNEL_VARLEN
    // b is the sequence: its first row and length from cu_seqlens, clamped so that every row this workgroup derives is a row
    // of the tensors whatever cu_seqlens holds (first row in [0, total_tokens], length in [0, min(max_seqlen, what is left)])
    int64_t v_row0 = va.cu_seqlens[b], v_len = va.cu_seqlens[b + 1];
    v_row0 = v_row0 < 0 ? 0 : (v_row0 > va.total_tokens ? va.total_tokens : v_row0);
    v_len -= v_row0;
    {
        const int64_t cap = va.total_tokens - v_row0 < va.max_seqlen ? va.total_tokens - v_row0 : va.max_seqlen;
        v_len = v_len < 0 ? 0 : (v_len > cap ? cap : v_len);
    }
    if ((int64_t)qb * TR::kBr >= v_len) return;   // (workgroup-uniform; before any barrier or DMA)
    // ... and its key rows from cu_seqlens_k, by the same rule against total_k and max_seqlen_k
    const int q_len = (int)v_len;
#ifdef FA_KERNEL_VARLEN_KVCACHE
    // ... and its key count from cache_seqlens, clamped to [0, max_len]; the rows themselves are found tile by tile (kc_*)
    int64_t k_row0 = 0, k_len = qa.cache_seqlens[b];
    k_len = k_len < 0 ? 0 : (k_len > qa.max_len ? qa.max_len : k_len);
#else
    int64_t k_row0 = qa.cu_seqlens_k[b], k_len = qa.cu_seqlens_k[b + 1];
    k_row0 = k_row0 < 0 ? 0 : (k_row0 > qa.total_k ? qa.total_k : k_row0);
    k_len -= k_row0;
    {
        const int64_t cap = qa.total_k - k_row0 < qa.max_seqlen_k ? qa.total_k - k_row0 : qa.max_seqlen_k;
        k_len = k_len < 0 ? 0 : (k_len > cap ? cap : k_len);
    }
#endif
    const int v_seq_len = (int)k_len;          // FA_SEQ_LEN, FA_N_KV_BLOCKS, ragged_rows and the key clamp: the K range
    const int kq_shift = v_seq_len - q_len;    // bottom-right diagonal: query r sees keys <= r + kq_shift
    // len_q for the epilogue's row tests, parked in a vector register across the loop (the scalar file is full there: held
    // as a scalar it is spilled to a lane and back; 372 of 512 vector registers are in use)
    int q_len_v;
    asm("v_mov_b32 %0, %1" : "=v"(q_len_v) : "s"(q_len));
    const int64_t kv_ss = va.kv_seq_stride;
    const int64_t head_off = v_row0 * ss + (int64_t)h * args.head_stride;
    const int64_t kv_head_off = k_row0 * kv_ss + (int64_t)(h / va.group) * va.kv_head_stride;
    const uint16_t *Qg = (const uint16_t *)args.q + head_off;
    const kv_elem *Kg = (const kv_elem *)args.k + kv_head_off;   // (fp8: the strides count bytes)
    const kv_elem *Vg = (const kv_elem *)args.v + kv_head_off;
    uint16_t *Og = (uint16_t *)args.o + head_off;
#else
    const int64_t head_off = (int64_t)b * args.batch_stride + (int64_t)h * args.head_stride;
    const uint16_t *Qg = (const uint16_t *)args.q + head_off;
    const kv_elem *Kg = (const kv_elem *)args.k + head_off;
    const kv_elem *Vg = (const kv_elem *)args.v + head_off;
    uint16_t *Og = (uint16_t *)args.o + head_off;
#endif

    // ---- per-lane DMA source offsets (elements), invariant over tiles ------------
    // piece i (wave-uniform) covers LDS chunks [64 i, 64 i + 64) of a tile.
    //   K: chunk p -> key p>>4, 16-B chunk (p&15) ^ (key&15)
    //   V: chunk p -> subtile p>>5 = (key>>3)*4 + (d>>5); inside: key&7 = (p&31)>>2,
    //      d&31 = (p&3)*8
    const int k_row_in_piece = lane / CPR;                                 // 0..RPP-1
    // swizzle of tile row RPP*i + k_row_in_piece; i = wave + NWAVES*j and RPP*NWAVES % 16 == 0
    const int k_swz = SWZ ? swz_of(RPP * wave + k_row_in_piece) : 0;
    const int64_t k_lane_off = (int64_t)k_row_in_piece * FA_KV_SS32 + (((lane & (CPR - 1)) ^ k_swz) << 3);
    const int v_sub_in_piece = lane >> 5;                                  // 0..1
    const int v_w = lane & 31;
    const int64_t v_lane_row = (v_w >> 2);                                 // key & 7
    const int v_lane_d = (v_w & 3) * 8;

    // KV blocks are visited last-to-first (forward_kernel.cuh:142,175-184): visit
    // index `it` is sequence block n_kv-1-it.
    // KV tiles this workgroup visits: all of them, or up to its last row's diagonal
    const int S_len = FA_SEQ_LEN;
    const int wg_row0 = qb * TR::kBr;
    int n_kv_ = FA_N_KV_BLOCKS;
#ifdef FA_KERNEL_VARLEN_WINDOW
    // the window's distances: unbounded, or beyond what any position reaches, is FAR (the host: lengths <= 2^30 - 128, so a
    // position lies in (-2^30, 2^30) and position -+ distance stays inside 32 bits)
    constexpr int FAR = 1 << 30;
    const int w_left = wa.left < 0 || wa.left > FAR ? FAR : wa.left;
    const int w_right = wa.right < 0 || wa.right > FAR ? FAR : wa.right;
    // the workgroup's key range: from its first row's floor to its last row's ceiling (both bounds grow with the row)
    const int wg_last_row = (wg_row0 + TR::kBr < q_len ? wg_row0 + TR::kBr : q_len) - 1;
    const int wg_hi = FA_SHIFTED(wg_last_row) + w_right < S_len - 1 ? FA_SHIFTED(wg_last_row) + w_right : S_len - 1;   // (< 0: no key at all)
    const int wg_lo = FA_SHIFTED(wg_row0) - w_left > 0 ? FA_SHIFTED(wg_row0) - w_left : 0;   // (<= wg_hi wherever wg_hi >= 0)
    n_kv_ = wg_hi < 0 ? 0 : (int)((unsigned)wg_hi / BC) + 1;
    const int n_vis = n_kv_ - (int)((unsigned)wg_lo / BC);   // tiles wg_hi / 64 down to wg_lo / 64
#else
    constexpr int wg_lo = 0;   // (no floor: floor_row)
#endif
    if (!WIN && MASK && args.causal) {
        const int last_row = (wg_row0 + TR::kBr < FA_Q_LEN ? wg_row0 + TR::kBr : FA_Q_LEN) - 1;
#ifdef FA_KERNEL_VARLEN
        const int need = FA_SHIFTED(last_row) < 0 ? 0 : FA_SHIFTED(last_row) / BC + 1;   // (no key at all: len_q - len_k rows or more above)
#else
        const int need = last_row / BC + 1;
#endif
        n_kv_ = need < n_kv_ ? need : n_kv_;
    }
    const int n_kv = n_kv_;
#ifdef FA_KERNEL_VARLEN
    if (n_kv == 0) {
        // no tile to visit (len_k = 0, or causal rows that all lie above the shifted diagonal): o = 0 and lse = -inf for the
        // workgroup's valid rows, whole 256-B rows as the epilogue stores them.  Workgroup-uniform, before any DMA or barrier.
        const int64_t z_row0 = (int64_t)wg_row0 + wave * TR::kRowsPerWave;
        const int z_rsub = lane / CPR, z_chunk = lane & (CPR - 1);
        float *z_lse = va.lse + ((int64_t)h * va.total_tokens + v_row0);
#pragma unroll
        for (int i = 0; i < TR::kRowsPerWave / RPP; ++i) {
            const int64_t row = z_row0 + RPP * i + z_rsub;
            if (row < q_len) *(s16x8 *)(Og + row * ss + z_chunk * 8) = s16x8{};
        }
#ifdef FA_KERNEL_VARLEN_SINKS
        // (the sink is the softmax's only member: lse = z)
        if (lane < TR::kRowsPerWave && z_row0 + lane < q_len) z_lse[z_row0 + lane] = sa.sinks[h];
#else
        if (lane < TR::kRowsPerWave && z_row0 + lane < q_len) z_lse[z_row0 + lane] = -__builtin_inff();
#endif
        return;
    }
#endif
    const unsigned smem_base = __builtin_amdgcn_readfirstlane(lds_addr(smem));
    // DMA addressing: SGPR base = head base + tile offset (scalar ALU), VGPR = 32-bit
    // per-lane byte offset of this wave's piece inside a tile (invariant over tiles).
    unsigned k_off[DMA_PER_WAVE], v_off[DMA_PER_WAVE];
#pragma unroll
    for (int j = 0; j < DMA_PER_WAVE; ++j) {
        const int i = wave + NWAVES * j;  // piece index, wave-uniform; keys 4i .. 4i+3
        k_off[j] = (unsigned)(((int64_t)(RPP * i) * FA_KV_SS32 + k_lane_off) * 2);
        const int sub = 2 * i + v_sub_in_piece;  // subtiles 2i, 2i+1
        v_off[j] = (unsigned)(((8 * (sub / DSUB) + v_lane_row) * FA_KV_SS32 + (sub % DSUB) * 32 + v_lane_d) * 2);
    }
    const int64_t tile_stride = (int64_t)BC * FA_KV_SS32;  // elements between consecutive KV blocks
#ifdef FA_KERNEL_VARLEN_KVCACHE
    // The walk over the cache's tiles, last to first, by counters (no division in the loop): kc_page / kc_tip are the page and
    // the tile inside it of the next K tile to request, kc_cur that page's table entry.  When the walk leaves a page, the entry
    // of the page below is requested behind the DMA pieces of that K request: a whole visit before the next K request uses it.  The
    // table is read through the constant address space (nothing writes it while the kernel runs): a workgroup-uniform SCALAR
    // load whose wait the compiler places at the first use -- as a global load between the DMA's inline asm it becomes a vector
    // load that is waited for (vmcnt(0): the K tile just requested) on the spot.  K is requested one tile ahead of V, so V's
    // base is the last K base or the one before it (kc_last, kc_prev).
    // The register-staged transport (the fp8 cache's) asks in another order -- prologue K0 V0 K1 V1 K2, visit `it` K(it+3) then
    // V(it+2) -- but K tiles still come in visit order, each once, so kc_offset / kc_step and the table entry's lead (requested
    // behind one K request, used by the next) stand as they are; only the V rule is derived again.  V0 and V1 are requested
    // right behind their own K: kc_last.  V(j), j >= 2, is requested in visit j - 2 behind K(j + 1) if that tile exists
    // (j + 1 < n): the last K request is one tile ahead and V's base is kc_prev; else K(j) was the walk's last request (K(n - 1)
    // was requested in visit n - 4 or in the prologue, and nothing since): kc_last.  K2, requested between V1 and V2, moves K1's base
    // out of (kc_last, kc_prev) only after V1 has used it.  One pair of bases serves both orders: the DMA's rule with its
    // `it > 0` read `it >= 2` (load_v), and no counter of V's own.  (n: the visit count, FA_N_VISITS.)
    // WIN: the walk starts at the top tile as ever and ends at the floor tile; kc_step's look-ahead stops at that tile's page
    // (kc_page_lo), so the entry of a page wholly below the workgroup's floor is never read.
    typedef const __attribute__((address_space(4))) int32_t *kc_table_ptr;
    const int kc_tpp = qa.tiles_per_page;
    int kc_page = (n_kv - 1) / kc_tpp;
    int kc_tip = (n_kv - 1) - kc_page * kc_tpp;
    const bool kc_paged = qa.block_table != nullptr;
    const kc_table_ptr kc_row = (kc_table_ptr)(unsigned long long)(qa.block_table + (int64_t)b * qa.bt_stride);
    int kc_cur = kc_paged ? kc_row[kc_page] : b;   // (contiguous cache: the "page" is the batch entry)
#ifdef FA_KERNEL_VARLEN_WINDOW
    const int kc_page_lo = (int)((unsigned)wg_lo / BC) / kc_tpp;   // the floor tile's page: no entry below it is read
#else
    constexpr int kc_page_lo = 0;
#endif
    int64_t kc_last = 0, kc_prev = 0;
    auto kc_offset = [&]() {   // the next K tile's offset (elements): the entry clamped to a page of the cache
        const int p = kc_cur < 0 ? 0 : (kc_cur >= qa.num_pages ? qa.num_pages - 1 : kc_cur);
        kc_prev = kc_last;
        kc_last = (int64_t)p * qa.page_stride + (int64_t)kc_tip * tile_stride;
        return kc_last;
    };
    auto kc_step = [&]() {     // ... and on to the tile below it
        if (kc_tip != 0) {
            --kc_tip;
            return;
        }
        kc_tip = kc_tpp - 1;
        --kc_page;
        if (kc_paged && kc_page >= kc_page_lo) kc_cur = kc_row[kc_page];
    };
#endif
    f32x4 abl_dummy[2 * DMA_PER_WAVE];  // ABL & 32 only: landing registers of plain loads
    // MASK: rows of the last sequence block that lie beyond seq_len are fetched from the last
    // valid row instead (their logits are masked, their P is exactly 0).
    // WIN: the floor tile is ragged from below -- its rows below the workgroup's floor are fetched from the floor's row
    // (floor_row), and it takes the ragged path even when all 64 rows are valid.  A tile may be clamped at both ends.
    auto ragged_rows = [&](int it) -> int {  // valid rows of visit it's tile if it is ragged, else 0
        const int kv0 = (n_kv - 1 - it) * BC;
        if constexpr (WIN) {
            if (kv0 < wg_lo) return kv0 + BC > S_len ? S_len - kv0 : BC;
        }
        return (MASK && kv0 + BC > S_len) ? S_len - kv0 : 0;
    };
    auto floor_row = [&](int it) -> int {  // first fetched row of visit it's tile (WIN; < valid: wg_lo <= wg_hi < S_len)
        const int kv0 = (n_kv - 1 - it) * BC;
        return wg_lo > kv0 ? wg_lo - kv0 : 0;
    };
    auto issue_k = [&](int it, int stage) {
#ifdef FA_KERNEL_VARLEN_KVCACHE
        const kv_elem *base = Kg + kc_offset();   // (K tiles are requested in visit order, each once)
#else
        const kv_elem *base = Kg + (int64_t)(n_kv - 1 - it) * tile_stride;
#endif
        const unsigned kdst = smem_base + stage * TILE;
        if (ABL & 16) return;
        if (const int valid = ragged_rows(it)) {
#pragma unroll
            for (int j = 0; j < DMA_PER_WAVE; ++j) {
                int row = RPP * (wave + NWAVES * j) + k_row_in_piece;
                row = row < valid ? row : valid - 1;
                if constexpr (WIN) row = row < floor_row(it) ? floor_row(it) : row;
                const unsigned off = (unsigned)(((int64_t)row * FA_KV_SS32 + (((lane & (CPR - 1)) ^ k_swz) << 3)) * 2);
                glds16_sv(base, off, kdst + (wave + NWAVES * j) * 1024);
            }
#ifdef FA_KERNEL_VARLEN_KVCACHE
            kc_step();
#endif
            return;
        }
#pragma unroll
        for (int j = 0; j < DMA_PER_WAVE; ++j) {
            if (ABL & 32)
                asm volatile("global_load_dwordx4 %0, %1, %2" : "=v"(abl_dummy[j]) : "v"(k_off[j]), "s"(base) : "memory");
            else
                glds16_sv(base, k_off[j], kdst + (wave + NWAVES * j) * 1024);
        }
#ifdef FA_KERNEL_VARLEN_KVCACHE
        kc_step();
#endif
    };
    auto issue_v = [&](int it, int stage) {
#ifdef FA_KERNEL_VARLEN_KVCACHE
        // V(it) follows K(it + 1) except in the prologue and at the last tile: then K(it) was the last K request
        const kv_elem *base = Vg + ((it > 0 && it + 1 < FA_N_VISITS) ? kc_prev : kc_last);
#else
        const kv_elem *base = Vg + (int64_t)(n_kv - 1 - it) * tile_stride;
#endif
        const unsigned vdst = smem_base + V_BASE + stage * TILE;
        if (ABL & 16) return;
        if (const int valid = ragged_rows(it)) {
#pragma unroll
            for (int j = 0; j < DMA_PER_WAVE; ++j) {
                const int sub = 2 * (wave + NWAVES * j) + v_sub_in_piece;
                int row = 8 * (sub / DSUB) + (int)v_lane_row;
                row = row < valid ? row : valid - 1;
                if constexpr (WIN) row = row < floor_row(it) ? floor_row(it) : row;
                const unsigned off = (unsigned)(((int64_t)row * FA_KV_SS32 + (sub % DSUB) * 32 + v_lane_d) * 2);
                glds16_sv(base, off, vdst + (wave + NWAVES * j) * 1024);
            }
            return;
        }
#pragma unroll
        for (int j = 0; j < DMA_PER_WAVE; ++j) {
            if (ABL & 32)
                asm volatile("global_load_dwordx4 %0, %1, %2" : "=v"(abl_dummy[DMA_PER_WAVE + j]) : "v"(v_off[j]), "s"(base) : "memory");
            else
                glds16_sv(base, v_off[j], vdst + (wave + NWAVES * j) * 1024);
        }
    };
    // Register-staged transport (DMA == false).  Piece i = 4 tile rows; lane L moves the
    // 16-B chunk (row 4i + L/16, chunk L%16): fully coalesced 256-B rows from global, and a
    // per-lane LDS address builds the same K / V images the DMA path builds by permuting
    // its source.  One set of landing registers per tile kind lives across a whole visit.
    // fp8 cache: a tile is 64 keys x 128 bytes, two 16-byte loads per lane (piece i = 8 tile rows; lane L fetches bytes
    // 16 c .. 16 c + 15, c = L % 8, of row 8 i + L / 8: whole 128-byte rows from global), converted behind the barrier into the
    // two 16-bit chunks 2c, 2c + 1 of the K image's row (XOR key & 15: the second chunk is the first's address ^ 16) or the matching
    // 32 bytes of the V image's subtile [key / 8][c / 2], row key & 7, half c & 1.
    // (enumerators, like FP8: the other forms' code does not change by a name)
    enum : int {
        ST_PER_WAVE = FP8 ? DMA_PER_WAVE / 2 : DMA_PER_WAVE,   // landing registers (16 bytes per lane) per tile
        ST_ROWS = FP8 ? 8 : 4,                                 // tile rows per piece
        ST_ESZ = FP8 ? 1 : 2                                   // bytes per K / V element
    };
    f32x4 kreg[ST_PER_WAVE], vreg[ST_PER_WAVE];
    const int st_r = FP8 ? lane >> 3 : lane >> 4, st_c = FP8 ? lane & 7 : lane & 15;
    // (FA_ST_SS32 names a local of this kernel: ss, or kv_ss in the fp8 cache's form)
    const unsigned st_goff = (unsigned)((((int64_t)(ST_ROWS * wave + st_r)) * FA_ST_SS32 + st_c * (16 / ST_ESZ)) * ST_ESZ);
    const unsigned st_gstep = (unsigned)(((int64_t)(ST_ROWS * NWAVES)) * FA_ST_SS32 * ST_ESZ);  // bytes between a wave's pieces
    const int st_krow = FP8 ? 8 * (wave & 1) + st_r : 4 * (wave & 3) + st_r;                // (tile row) & 15
    const unsigned st_kwr = FP8 ? (8 * wave + st_r) * 256 + (((2 * st_c) ^ (SWZ ? st_krow : 0)) << 4)
                                : wave * 1024 + st_r * 256 + ((st_c ^ (SWZ ? st_krow : 0)) << 4);
    const unsigned st_vwr = FP8 ? wave * 2048 + (st_c >> 1) * 512 + st_r * 64 + (st_c & 1) * 32
                                : (wave >> 1) * 2048 + ((wave & 1) * 4 + st_r) * 64 + (st_c >> 2) * 512 + (st_c & 3) * 16;
    auto load_tile = [&](const kv_elem *tensor, int it, f32x4 (&reg)[ST_PER_WAVE]) {
        // (FA_ST_TILE uses the locals n_kv and tile_stride, except in the fp8 cache's form, where `tensor` is the tile already)
        const char *tile = (const char *)(FA_ST_TILE(tensor, it));
        if (const int valid = ragged_rows(it)) {   // (rows beyond the end come from the last valid row, as the DMA fetches them)
#pragma unroll
            for (int j = 0; j < ST_PER_WAVE; ++j) {
                int row = ST_ROWS * (wave + NWAVES * j) + st_r;
                row = row < valid ? row : valid - 1;
                if constexpr (WIN) row = row < floor_row(it) ? floor_row(it) : row;
                reg[j] = *(const f32x4 *)(tile + ((int64_t)row * FA_ST_SS32 + st_c * (16 / ST_ESZ)) * ST_ESZ);
            }
            return;
        }
#pragma unroll
        for (int j = 0; j < ST_PER_WAVE; ++j) reg[j] = *(const f32x4 *)(tile + st_goff + j * st_gstep);
    };
#ifdef FA_KERNEL_VARLEN_KVCACHE_FP8
    // (the cache's tiles: the walk's bases, K in visit order and V by the rule derived at kc_offset)
    auto load_k = [&](int it) {
        load_tile(Kg + kc_offset(), it, kreg);
        kc_step();
    };
    auto load_v = [&](int it) { load_tile(Vg + ((it >= 2 && it + 1 < FA_N_VISITS) ? kc_prev : kc_last), it, vreg); };
#else
    auto load_k = [&](int it) { load_tile(Kg, it, kreg); };
    auto load_v = [&](int it) { load_tile(Vg, it, vreg); };
#endif
    auto store_k = [&](int stage) {
        char *dst = smem + stage * TILE + st_kwr;
        if constexpr (FP8) {
#pragma unroll
            for (int j = 0; j < ST_PER_WAVE; ++j) {
                const u32x4 w = __builtin_bit_cast(u32x4, kreg[j]);
                *(vec8 *)(dst + j * 8192) = cvt_fp8x8<DT>(w[0], w[1]);
                *(vec8 *)(smem + stage * TILE + ((st_kwr ^ 16) + j * 8192)) = cvt_fp8x8<DT>(w[2], w[3]);
            }
            return;
        }
#pragma unroll
        for (int j = 0; j < ST_PER_WAVE; ++j) *(f32x4 *)(dst + j * NWAVES * 1024) = kreg[j];
    };
    auto store_v = [&](int stage) {
        char *dst = smem + V_BASE + stage * TILE + st_vwr;
        if constexpr (FP8) {
#pragma unroll
            for (int j = 0; j < ST_PER_WAVE; ++j) {
                const u32x4 w = __builtin_bit_cast(u32x4, vreg[j]);
                *(vec8 *)(dst + j * 8192) = cvt_fp8x8<DT>(w[0], w[1]);
                *(vec8 *)(dst + j * 8192 + 16) = cvt_fp8x8<DT>(w[2], w[3]);
            }
            return;
        }
#pragma unroll
        for (int j = 0; j < ST_PER_WAVE; ++j) *(f32x4 *)(dst + j * (NWAVES / 2) * 2048) = vreg[j];
    };
    auto dma_wait = [&]() { if (DMA && !(ABL & 8)) dma_wait_all(); };
    auto barrier = [&]() { if (!(ABL & 8)) wg_barrier(); };
    auto wait_and_barrier = [&]() {
        dma_wait();
        barrier();
    };

#ifdef FA_TRACE
    if (blockIdx.x == (unsigned)args.trace_block && lane == 0)
        args.trace[(wave * 64 + 63) * 8 + 7] = __builtin_amdgcn_s_getreg((31 << 11) | 4);  // HW_REG_HW_ID
#endif
    // ---- prologue: first tiles in flight, then Q -> VGPRs --------------------------
    auto first_requests = [&]() {
        if (EAGER && DMA) {
            issue_k(0, 0);
            issue_v(0, 0);
        }
        if (!DMA) {
            load_k(0);
            load_v(0);
        }
    };
    first_requests();

    vec8 Qr[QT][KS];
#pragma unroll
    for (int qt = 0; qt < QT; ++qt) {
        int64_t row = (int64_t)qb * TR::kBr + wave_r * TR::kRowsPerWave + qt * 32 + r31;
        if (MASK && row >= FA_Q_LEN) row = FA_Q_LEN - 1;  // rows past the end are computed, never stored
        const uint16_t *qp = Qg + row * ss + hi * 8;
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) Qr[qt][ks] = *(const vec8 *)(qp + ks * 16);
    }

    // forward_kernel.cuh:150-151 (fp32 product of rsqrt(d) and log2 e)
    // (fp8 cache: times k_descale, FA_K_DESCALED, which reads the locals fa8, b, h and va -- one multiply per workgroup; S and the running max stay raw logits, and
    // exp2(s c - m c), the rescale factors and lse = ln l + m c come out in descaled units: a positive descale keeps the max the max)
    const float c = FA_K_DESCALED((float)((double)(1.0f / __builtin_sqrtf((float)D)) * 1.4426950408889634074));

    f32x16 O[QT][DTILES];
    float m[QT], l[QT];
    auto reset_state = [&]() {
#pragma unroll
        for (int qt = 0; qt < QT; ++qt) {
            m[qt] = -__builtin_inff();
            l[qt] = 0.0f;
#pragma unroll
            for (int t = 0; t < DTILES; ++t)
#pragma unroll
                for (int r = 0; r < 16; ++r) O[qt][t][r] = 0.0f;
        }
    };
    reset_state();

    // per-lane LDS read offsets
    //   K A-operand: row 32*nt + r31, chunk (2*ks + hi) ^ (r31 & 15)
    const int ka_swz = SWZ ? swz_of(r31) : 0;
    const int ka_base = r31 * ROWB;
    //   V^T A-operand (transpose read): see header comment
    const int li = lane & 15, lg = lane >> 4;
    const int va_base = (4 * (lg >> 1) + (li >> 2)) * 64 + (lg & 1) * 32 + (li & 3) * 8;

    // ---- MASK: logits of keys >= seq_len, or above the causal diagonal, become -inf ---------
    const int wave_row0 = wg_row0 + wave_r * TR::kRowsPerWave;
#ifdef FA_KERNEL_VARLEN_WINDOW
    // WIN: a tile needs the mask if it reaches above the ceiling of the wave's first row (the lowest ceiling: this covers the
    // keys >= len_k too) or below the floor of its last row (the highest floor); a tile inside every row's window does not.
    // mask_S finds each row's two bounds again from the row (nothing more is carried across the loop).
    auto tile_needs_mask = [&](int it) -> bool {  // wave-uniform
        const int kv0 = (n_kv - 1 - it) * BC;
        const int p0 = FA_SHIFTED(wave_row0);
        const int hi_first = p0 + w_right < S_len - 1 ? p0 + w_right : S_len - 1;
        return kv0 + BC - 1 > hi_first || kv0 < p0 + (TR::kRowsPerWave - 1) - w_left;
    };
    auto mask_S = [&](f32x16 (&S)[QT][NTW], int it) {
        const int kv0 = (n_kv - 1 - it) * BC;
#pragma unroll
        for (int qt = 0; qt < QT; ++qt) {
            const int p = FA_SHIFTED(wave_row0 + qt * 32 + r31);
            const int hi_r = p + w_right < S_len - 1 ? p + w_right : S_len - 1;   // last live key (< lo_r: a row that sees none)
            const int lo_r = p - w_left;                                          // first live key (keys are not negative: no clamp at 0)
#pragma unroll
            for (int nt = 0; nt < NTW; ++nt)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int key = kv0 + 32 * (NT0 + nt) + (r & 3) + 8 * (r >> 2) + 4 * hi;
                    S[qt][nt][r] = (key < lo_r || key > hi_r) ? -__builtin_inff() : S[qt][nt][r];
                }
        }
    };
#else
    auto tile_needs_mask = [&](int it) -> bool {  // wave-uniform
        const int kv0 = (n_kv - 1 - it) * BC;
        return MASK && (kv0 + BC > S_len || (args.causal && kv0 + BC - 1 > FA_SHIFTED(wave_row0)));
    };
    auto mask_S = [&](f32x16 (&S)[QT][NTW], int it) {
        const int kv0 = (n_kv - 1 - it) * BC;
#pragma unroll
        for (int qt = 0; qt < QT; ++qt) {
            const int q_row = wave_row0 + qt * 32 + r31;
            const int limit = args.causal ? (FA_SHIFTED(q_row) < S_len - 1 ? FA_SHIFTED(q_row) : S_len - 1) : S_len - 1;  // last live key
#pragma unroll
            for (int nt = 0; nt < NTW; ++nt)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int key = kv0 + 32 * (NT0 + nt) + (r & 3) + 8 * (r >> 2) + 4 * hi;
                    S[qt][nt][r] = key > limit ? -__builtin_inff() : S[qt][nt][r];
                }
        }
    };
#endif
#ifdef FA_KERNEL_VARLEN_SOFTCAP
    // FA_CAP_S: S -> A tanh(S / A) with tanh(x) = 1 - 2 / (exp2(2 x log2 e) + 1), one v_exp_f32 and one v_rcp_f32 per element.
    // exp2 overflowing to +inf gives 1 - 2 / inf = 1 and underflowing to 0 gives 1 - 2 = -1: no NaN at either end.
#ifdef FA_KERNEL_VARLEN_KVCACHE_FP8
    // (fp8 cache: S arrives in raw, undescaled units; k_descale times the constant brings the tanh's argument to the 16-bit form's)
    const float cap_a = sa.cap_a, cap_m2a = -2.0f * sa.cap_a,
                cap_k = (fa8.k_descale ? fa8.k_descale[(int64_t)b * fa8.ds_bs + h / va.group] : 1.0f) * (sa.cap_inv_a * 2.8853900817779268f);
#else
    const float cap_a = sa.cap_a, cap_m2a = -2.0f * sa.cap_a, cap_k = sa.cap_inv_a * 2.8853900817779268f;   // 2 log2(e) / A
#endif
    auto cap_S = [&](f32x16 (&S)[QT][NTW]) {
#pragma unroll
        for (int qt = 0; qt < QT; ++qt)
#pragma unroll
            for (int nt = 0; nt < NTW; ++nt)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const float e = __builtin_amdgcn_exp2f(S[qt][nt][r] * cap_k);
                    S[qt][nt][r] = __builtin_fmaf(__builtin_amdgcn_rcpf(e + 1.0f), cap_m2a, cap_a);
                }
    };
#endif
    // a row whose keys were all masked so far has m = -inf: exponentiate against 0 instead
    auto finite_or_zero = [&](float mval) { return (MASK && mval == -__builtin_inff()) ? 0.0f : mval; };

    // ---- S^T = K Q^T ------------------------------------------------------------
    auto qk = [&](int stage, f32x16 (&S)[QT][NTW]) {
        const char *kt = smem + stage * TILE;
#pragma unroll
        for (int qt = 0; qt < QT; ++qt)
#pragma unroll
            for (int nt = 0; nt < NTW; ++nt)
#pragma unroll
                for (int r = 0; r < 16; ++r) S[qt][nt][r] = 0.0f;
        // ks outer / key-tile inner: consecutive MFMAs accumulate into different tiles
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
#pragma unroll
            for (int nt = 0; nt < NTW; ++nt) {
                const int off = (NT0 + nt) * 32 * ROWB + ka_base + (((2 * ks + hi) ^ ka_swz) << 4);
                const vec8 a = (ABL & 4) ? Qr[0][(ks + nt) % KS] : *(const vec8 *)(kt + off);
#pragma unroll
                for (int qt = 0; qt < QT; ++qt) S[qt][nt] = E::mfma(a, Qr[qt][ks], S[qt][nt]);
            }
        }
        if (SCHED && !PIPE) sched_mfma_fed_from_lds<NTW * KS * QT, 1, (ABL & 128) ? 12 : 8>();
    };

    // ---- online softmax, lane-local (softmax.cuh:85-105) --------------------------
    // Updates m, l; returns P (16-bit, MFMA B-operand order) and the rescale factor
    // alpha = exp2((m_prev - m_new) c) that (l, O) must be multiplied by BEFORE P.V
    // of this tile is accumulated (scale_l_O, softmax.cuh:36-49).  l is rescaled here;
    // O by rescale_O() -- skipped when alpha == 1 in every lane (multiplying by 1.0f is
    // the identity, so the skip is bit-exact).
    auto softmax = [&](f32x16 (&S)[QT][NTW], vec8 (&Pb)[QT][NTW][2], float (&alpha)[QT], auto first_tag, auto fast_tag) {
        constexpr bool FIRST = decltype(first_tag)::value;
        constexpr bool FAST = decltype(fast_tag)::value;  // speculative: m stays the first tile's row max
        if (ABL & 2) {
#pragma unroll
            for (int qt = 0; qt < QT; ++qt) {
                alpha[qt] = 1.0f;
#pragma unroll
                for (int nt = 0; nt < NTW; ++nt) {
                    float p[16];
#pragma unroll
                    for (int r = 0; r < 16; ++r) p[r] = S[qt][nt][r];
                    Pb[qt][nt][0] = E::pack8(p);
                    Pb[qt][nt][1] = E::pack8(p + 8);
                }
            }
            return;
        }
#pragma unroll
        for (int qt = 0; qt < QT; ++qt) {
            float mx = S[qt][0][0];
            if constexpr (!FAST || FIRST) {
#pragma unroll
                for (int nt = 0; nt < NTW; ++nt)
#pragma unroll
                    for (int r = 0; r < 16; ++r) mx = fmaxf(mx, S[qt][nt][r]);
                mx = pair_max(mx);
            }
            float m_new;
            if (FAST && !FIRST) {
                m_new = m[qt];
                alpha[qt] = 1.0f;
            } else if (FIRST && OPT) {
                m_new = mx;
                alpha[qt] = 1.0f;
            } else {
                m_new = fmaxf(m[qt], mx);
                alpha[qt] = __builtin_amdgcn_exp2f((m[qt] - finite_or_zero(m_new)) * c);
                l[qt] *= alpha[qt];
            }
            m[qt] = m_new;
            const float neg_msc = -(finite_or_zero(m_new) * c);
            float rowsum = 0.0f;
#pragma unroll
            for (int nt = 0; nt < NTW; ++nt) {
                float p[16];
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    // exponentiate_tensor, softmax.cuh:51-64: exp2(s*c - m*c)
                    p[r] = __builtin_fmaf(S[qt][nt][r], c, neg_msc);
                    if (!(ABL & 1)) p[r] = __builtin_amdgcn_exp2f(p[r]);
                    rowsum += p[r];  // fp32 P, before rounding (softmax.cuh:66-83)
                }
                Pb[qt][nt][0] = E::pack8(p);
                Pb[qt][nt][1] = E::pack8(p + 8);
            }
            l[qt] = (FIRST && OPT) ? rowsum : l[qt] + rowsum;
        }
    };

    auto rescale_O = [&](const float (&alpha)[QT]) {
#pragma unroll
        for (int qt = 0; qt < QT; ++qt) {
            if (__all(alpha[qt] == 1.0f)) continue;  // wave-uniform
#pragma unroll
            for (int t = 0; t < DTILES; ++t)
#pragma unroll
                for (int r = 0; r < 16; ++r) O[qt][t][r] *= alpha[qt];
        }
    };

    // ---- O^T += V^T P^T ------------------------------------------------------------
    auto pv = [&](int stage, const vec8 (&Pb)[QT][NTW][2]) {
        const char *vt = smem + V_BASE + stage * TILE;
        // 16-key slice outer / d tile inner: consecutive MFMAs hit different accumulators
#pragma unroll
        for (int nt = 0; nt < NTW; ++nt) {
#pragma unroll
            for (int half = 0; half < 2; ++half) {
#pragma unroll
                for (int t = 0; t < DTILES; ++t) {
                    const int s16 = 2 * (NT0 + nt) + half;
                    const char *vp = vt + va_base + s16 * (DSUB * 1024) + t * 512;
                    const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((FA_LDS(s16x4) *)(vp));
                    const s16x4 up =
                        __builtin_amdgcn_ds_read_tr16_b64_v4i16((FA_LDS(s16x4) *)(vp + DSUB * 512));
                    s16x8 av;
                    av.lo = lo;
                    av.hi = up;
                    const vec8 a = (ABL & 4) ? Qr[0][(t + s16) % KS] : __builtin_bit_cast(vec8, av);
#pragma unroll
                    for (int qt = 0; qt < QT; ++qt)
                        O[qt][t] = E::mfma(a, Pb[qt][nt][half], O[qt][t]);
                }
            }
        }
        if (SCHED && !PIPE) sched_mfma_fed_from_lds<DTILES * NTW * 2 * QT, 2, (ABL & 128) ? 12 : 8>();
    };

    using TrueTag = BoolTag<true>;
    using FalseTag = BoolTag<false>;

    static_assert(!(QT == 2 && PIPE), "the 64-rows-per-wave pipelined schedule lives in fa_fwd_kernel64.hpp");
    // SPEC (the OPT build of the double-buffered plain variants; reached through fa_fwd_opts.speculative): the speculative softmax of
    // fa_fwd_kernel64.hpp on a one-item workgroup.  attempt<FAST> keeps the row max of the
    // FIRST visited tile as the reference for every tile -- no row max, no rescale factor, no O rescale --
    // and checks the row sums l >= every P against the overflow limit at the end; if any wave of the
    // workgroup fails, all of them run the item again with the running max (attempt<SAFE>): the K / V
    // stream simply starts over.
    // (not on the register-staged transport: with its landing registers live across both attempts two
    // of those variants spill)
    constexpr bool SPEC = OPT && EAGER && !MASK && DMA;
    auto attempt = [&](auto fast_tag) -> bool {
    constexpr bool FAST = decltype(fast_tag)::value;
    if constexpr (PIPE) {
        // In-wave software pipeline with two S accumulators.  While the matrix pipe forms
        // S(it+1) = K(it+1) Q^T and then O += V(it) P(it), the VALU turns the finished S(it)
        // into P(it): every MFMA of the visit has ~4-5 independent VALU ops and 1-2 LDS
        // operand reads scheduled beside it (sched_group_barrier pins the interleave), so a
        // wave keeps the matrix pipe and the vector ALU busy together regardless of what
        // its SIMD partner is doing.  Per visit `it` (S_cur = S(it), complete):
        //   top    : barrier (K(it+1), V(it) landed; stages of K(it), V(it-1) free);
        //            DMA K(it+2), V(it+1); m/alpha/l update from the row max found last
        //            visit; O *= alpha only if some lane's max moved
        //   MFMA   : 8*NT x QK^T(it+1)  ->  4*NT x P.V(it) keys 0-31  ->  ... keys 32-63 ...
        //   VALU   : P = exp2(S_cur*c - m*c), row sums, 16-bit pack, tile by tile, then the
        //            row max of S(it+1)
        // O is only ever rescaled while no P.V is in flight (start of a visit), so the
        // factor applies to exactly the terms accumulated so far (guide T13 hazard).
        f32x16 Sa[QT][NTW], Sb[QT][NTW];
        float mx[QT];     // row max of the S tile that becomes S_cur next
        auto row_max = [&](f32x16 (&S)[QT][NTW]) {
#pragma unroll
            for (int qt = 0; qt < QT; ++qt) {
                float v = S[qt][0][0];
#pragma unroll
                for (int nt = 0; nt < NTW; ++nt)
#pragma unroll
                    for (int r = 0; r < 16; ++r) v = fmaxf(v, S[qt][nt][r]);
                mx[qt] = pair_max(v);
            }
        };
        auto visit = [&](int it, f32x16 (&S_cur)[QT][NTW], f32x16 (&S_nxt)[QT][NTW], auto last_tag) {
            constexpr bool LAST = decltype(last_tag)::value;
            FA_STAMP(it, 0);
            wait_and_barrier();
            FA_STAMP(it, 1);
            if (DMA) {
                if (it + 2 < FA_N_VISITS) issue_k(it + 2, it & 1);
                if (it + 1 < FA_N_VISITS) issue_v(it + 1, (it + 1) & 1);
            } else {
                // registers hold K(it+2), V(it+1) (loaded during the previous visit); their
                // LDS stages were freed by the barrier above.  Then start K(it+3), V(it+2).
                if (it + 2 < FA_N_VISITS) store_k(it & 1);
                if (it + 1 < FA_N_VISITS) store_v((it + 1) & 1);
                if (it + 3 < FA_N_VISITS) load_k(it + 3);
                if (it + 2 < FA_N_VISITS) load_v(it + 2);
            }
            // scale_l_O (softmax.cuh:36-49) with the new running max
            float neg_msc[QT], rowsum[QT];
#pragma unroll
            for (int qt = 0; qt < QT; ++qt) {
                if constexpr (FAST) {  // m = the first tile's row max (set once, below): nothing moves
                    neg_msc[qt] = -(m[qt] * c);
                    rowsum[qt] = 0.0f;
                    continue;
                }
                const float m_new = fmaxf(m[qt], mx[qt]);
                const float alpha = __builtin_amdgcn_exp2f((m[qt] - finite_or_zero(m_new)) * c);
                l[qt] *= alpha;
                m[qt] = m_new;
                neg_msc[qt] = -(finite_or_zero(m_new) * c);
                rowsum[qt] = 0.0f;
                if (!(OPT && it == 0) && !__all(alpha == 1.0f)) {
#pragma unroll
                    for (int t = 0; t < DTILES; ++t)
#pragma unroll
                        for (int r = 0; r < 16; ++r) O[qt][t][r] *= alpha;
                }
            }
            FA_STAMP(it, 2);
            // ---- matrix stream 1: S_nxt = K(it+1) Q^T ---------------------------------
            if (!LAST) {
                qk((it + 1) & 1, S_nxt);
                FA_CAP_S(S_nxt);
                if (MASK && tile_needs_mask(it + 1)) mask_S(S_nxt, it + 1);
            }
            // ---- vector stream: P = exp2(S_cur c - m c) (softmax.cuh:51-83) -------------
            vec8 P[QT][NTW][2];
#pragma unroll
            for (int nt = 0; nt < NTW; ++nt) {
#pragma unroll
                for (int qt = 0; qt < QT; ++qt) {
                    float p[16];
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        p[r] = __builtin_fmaf(S_cur[qt][nt][r], c, neg_msc[qt]);
                        if (!(ABL & 1)) p[r] = __builtin_amdgcn_exp2f(p[r]);
                        rowsum[qt] += p[r];
                    }
                    P[qt][nt][0] = E::pack8(p);
                    P[qt][nt][1] = E::pack8(p + 8);
                }
            }
            // ---- matrix stream 2: O += V(it) P --------------------------------------------
            pv(it & 1, P);
            if (!LAST && !FAST) row_max(S_nxt);
#pragma unroll
            for (int qt = 0; qt < QT; ++qt) l[qt] += rowsum[qt];
            if (SCHED) {
                // interleave: 8 operand reads ahead, then per MFMA 1-2 reads + 5 VALU/TRANS
                constexpr int N_QK = LAST ? 0 : NTW * KS * QT, N_PV = DTILES * NTW * 2 * QT;
                __builtin_amdgcn_sched_group_barrier(0x100, 8, 0);
#pragma unroll
                for (int i = 0; i < N_QK; ++i) {
                    __builtin_amdgcn_sched_group_barrier(0x8, 1, 0);
                    __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
                    __builtin_amdgcn_sched_group_barrier(0x402, 5, 0);
                }
#pragma unroll
                for (int i = 0; i < N_PV; ++i) {
                    __builtin_amdgcn_sched_group_barrier(0x8, 1, 0);
                    __builtin_amdgcn_sched_group_barrier(0x100, 2, 0);
                    __builtin_amdgcn_sched_group_barrier(0x402, 5, 0);
                }
            }
            FA_STAMP(it, 3);
        };
        if (DMA) {
            wait_and_barrier();  // K(0), V(0) landed
            if (FA_N_VISITS > 1) issue_k(1, 1);
            qk(0, Sa);
            FA_CAP_S(Sa);
            if (MASK && tile_needs_mask(0)) mask_S(Sa, 0);
            row_max(Sa);
            if constexpr (FAST) {
#pragma unroll
                for (int qt = 0; qt < QT; ++qt) m[qt] = mx[qt];
            }
        } else {
            // registers: K(0), V(0) -> LDS; then K(1), V(1) in flight; after S(0): K(1) -> LDS,
            // K(2) in flight.  Invariant at the top of visit `it`: LDS holds K(it+1), V(it)
            // (published by that visit's barrier), registers hold K(it+2), V(it+1).
            store_k(0);
            store_v(0);
            if (FA_N_VISITS > 1) { load_k(1); load_v(1); }
            barrier();
            qk(0, Sa);
            FA_CAP_S(Sa);
            if (MASK && tile_needs_mask(0)) mask_S(Sa, 0);
            row_max(Sa);
            if constexpr (FAST) {
#pragma unroll
                for (int qt = 0; qt < QT; ++qt) m[qt] = mx[qt];
            }
            if (FA_N_VISITS > 1) store_k(1);
            if (FA_N_VISITS > 2) load_k(2);
        }
        int it = 0;
        for (; it + 2 < FA_N_VISITS; it += 2) {
            visit(it, Sa, Sb, FalseTag{});
            visit(it + 1, Sb, Sa, FalseTag{});
        }
        if (it + 2 == FA_N_VISITS) {
            visit(it, Sa, Sb, FalseTag{});
            visit(it + 1, Sb, Sa, TrueTag{});
        } else {
            visit(it, Sa, Sb, TrueTag{});
        }
    } else if (EAGER) {
        // tile `it` lives in stage it&1; its DMA was issued one visit earlier.
        auto visit = [&](int it, auto first_tag) {
            const int stage = it & 1;
            FA_STAMP(it, 0);
            wait_and_barrier();  // tile `it` landed for every wave; stage^1 free again
            FA_STAMP(it, 1);
            if (DMA) {
                if (it + 1 < FA_N_VISITS) {
                    issue_k(it + 1, stage ^ 1);
                    issue_v(it + 1, stage ^ 1);
                }
            } else {
                // registers hold tile it+1 (loaded during the previous visit)
                if (it + 1 < FA_N_VISITS) { store_k(stage ^ 1); store_v(stage ^ 1); }
                if (it + 2 < FA_N_VISITS) { load_k(it + 2); load_v(it + 2); }
            }
            f32x16 S[QT][NTW];
            vec8 P[QT][NTW][2];
            float alpha[QT];
            if (ABL & 64) __builtin_amdgcn_s_setprio(1);
            qk(stage, S);
            if (ABL & 64) __builtin_amdgcn_s_setprio(0);
            FA_CAP_S(S);
            if (MASK && tile_needs_mask(it)) mask_S(S, it);
            FA_STAMP(it, 2);
            softmax(S, P, alpha, first_tag, fast_tag);
            if (!decltype(first_tag)::value && !FAST) rescale_O(alpha);
            FA_STAMP(it, 3);
            if (ABL & 64) __builtin_amdgcn_s_setprio(1);
            pv(stage, P);
            if (ABL & 64) __builtin_amdgcn_s_setprio(0);
            FA_STAMP(it, 4);
        };
        if (!DMA) {
            store_k(0);
            store_v(0);
            if (FA_N_VISITS > 1) { load_k(1); load_v(1); }
        }
        if (OPT) visit(0, TrueTag{}); else visit(0, FalseTag{});
        for (int it = 1; it < FA_N_VISITS; ++it) visit(it, FalseTag{});
    } else {
        for (int it = 0; it < FA_N_VISITS; ++it) {
            if (it > 0) barrier();  // everyone done reading the single stage
            issue_k(it, 0);
            issue_v(it, 0);
            wait_and_barrier();
            f32x16 S[QT][NTW];
            vec8 P[QT][NTW][2];
            float alpha[QT];
            qk(0, S);
            FA_CAP_S(S);
            if (MASK && tile_needs_mask(it)) mask_S(S, it);
            if (OPT && it == 0) {
                softmax(S, P, alpha, TrueTag{}, FalseTag{});
            } else {
                softmax(S, P, alpha, FalseTag{}, FalseTag{});
                rescale_O(alpha);
            }
            pv(0, P);
        }
    }

    barrier();  // every wave is done with the K/V stages
    if constexpr (FAST) {
        // every P of a row is <= its l: below the limit nothing overflowed (fp32 exp2, the 16-bit P, fp32 O);
        // NaN fails the compare too.  One verdict per workgroup, through the idle LDS.
        constexpr float kLimit = spec_limit<DT>();
        bool bad = false;
#pragma unroll
        for (int qt = 0; qt < QT; ++qt) bad |= !(pair_sum(l[qt]) < kLimit);
        if constexpr (DT == 15) {
            // bf16: |O| <= l max|V| stays finite below the limit only for |V| < 2^63 -- so look at what the accumulators
            // hold (o - o is 0 for a finite o, NaN for inf / NaN) instead of bounding it.  fp16: 2^15 * 65504 is finite.
            float nonfinite = 0.0f;
#pragma unroll
            for (int qt = 0; qt < QT; ++qt)
#pragma unroll
                for (int t = 0; t < DTILES; ++t)
#pragma unroll
                    for (int r = 0; r < 16; ++r) nonfinite += O[qt][t][r] - O[qt][t][r];
            bad |= !(nonfinite == 0.0f);
        }
        const int wave_bad = __ballot(bad) != 0 ? 1 : 0;
        if (lane == 0) *(int *)(smem + wave * 4) = wave_bad;
        barrier();
        int any = 0;
#pragma unroll
        for (int w = 0; w < NWAVES; ++w) any |= *(const int *)(smem + w * 4);
        any = __builtin_amdgcn_readfirstlane(any);
        barrier();  // (flags read before anything is staged or requested over them)
        return any == 0;
    }
    return true;
    };  // attempt
    bool done = false;
    if constexpr (SPEC) done = attempt(TrueTag{});
    if (SPEC && !done && threadIdx.x == 0) report_redo(args);
    if (args.stats && threadIdx.x == 0) {  // fa_fwd_stats: one item per workgroup; redone = the speculative pass failed
        atomicAdd(args.stats, 1u);
        if (SPEC && !done) atomicAdd(args.stats + 1, 1u);
    }
    if (!done) {
        if constexpr (SPEC) {  // start over with the running max
            reset_state();
            first_requests();
        }
        attempt(FalseTag{});
    }

#ifdef FA_KERNEL_VARLEN
    // (FA_LSE_M_TIMES_C: m * c, in the fp8 cache's form with a rounding of its own; it names nothing but its arguments)
    // lse = ln l + m / sqrt d in the kernel's own units (m c is log2): one fp32 per valid row; both lane halves hold it
    // (this (sequence, head)'s rows of lse, found again here rather than kept in registers across the loop)
    int64_t l_row0 = va.cu_seqlens[b];
    l_row0 = l_row0 < 0 ? 0 : (l_row0 > va.total_tokens ? va.total_tokens : l_row0);
    float *lse_rows = va.lse + ((int64_t)h * va.total_tokens + l_row0);
#ifdef FA_KERNEL_VARLEN_SINKS
    // The sink joins the denominator here, in log2 units against a common maximum so that neither term overflows:
    //   M = max(m c, z log2 e),  l' = l exp2(m c - M) + exp2(z log2 e - M),  o = O exp2(m c - M) / l',  lse = (log2 l' + M) ln 2.
    // z far above every logit: the first factor underflows to 0, l' = 1, lse = z, o = 0; far below: its term underflows and
    // nothing changes.  A row with l = 0 (m = -inf: it saw no key) gives o = 0 and lse = z exactly -- with z = -inf that is
    // -inf, and no exp2(-inf - -inf) is formed: where l > 0, m and with it M are finite.  z = -inf on a live row: M = m c, the
    // factor is exp2(0) = 1, the sink's term 0: the windowed kernel's values.
    const float sink_z = sa.sinks[h];   // (workgroup-uniform, read here and not held across the loop)
    auto sink_end = [&](float l_row, float m_row, float &scale, float &lse_row) {
        const float mc = m_row * c, zc = sink_z * 1.4426950408889634074f;
        const float M = fmaxf(mc, zc);
        const float a = __builtin_amdgcn_exp2f(mc - M);
        const float l_all = l_row * a + __builtin_amdgcn_exp2f(zc - M);
        const bool dead = l_row == 0.0f;
        scale = dead ? 0.0f : a / l_all;
        lse_row = dead ? sink_z : (__builtin_amdgcn_logf(l_all) + M) * 0.693147180559945309f;
    };
#pragma unroll
    for (int qt = 0; qt < QT; ++qt) {
        const int row = wave_row0 + qt * 32 + r31;
        float scale, lse_row;
        sink_end(pair_sum(l[qt]), m[qt], scale, lse_row);
        if (hi == 0 && row < FA_Q_LEN_END) lse_rows[row] = lse_row;
    }
#else
#pragma unroll
    for (int qt = 0; qt < QT; ++qt) {
        const float l_row = pair_sum(l[qt]);
        const int row = wave_row0 + qt * 32 + r31;
        if (hi == 0 && row < FA_Q_LEN_END)   // (a row without keys: l = 0, m = -inf -> ln 0 + 0 = -inf)
            lse_rows[row] = (__builtin_amdgcn_logf(l_row) + FA_LSE_M_TIMES_C(finite_or_zero(m[qt]), c)) * 0.693147180559945309f;
    }
#endif
#endif
    if ((ABL & 32) && args.seq_len < 0) {  // never true: keeps the landing registers allocated
#pragma unroll
        for (int j = 0; j < 2 * DMA_PER_WAVE; ++j) *(f32x4 *)(Og + j * 8 + lane * 64) = abl_dummy[j];
    }
    // ---- epilogue: finish l, normalise, RNE to 16 bit, store ----------------------
    // (final_softmax_normalization softmax.cuh:107-128; forward_kernel.cuh:186-203)
    // Like the reference, O goes through shared memory so that global stores are whole
    // 256-B rows (16 B per lane, 4 rows per wave-instruction) instead of 8-B pieces at a
    // row stride.  Each wave stages only its own rows; the 16-B chunk index is XORed with
    // (row & 15) so both the 8-B writes and the 16-B reads are bank-conflict free.
    if constexpr (KSPLIT == 2) {
        // Merge the two key groups of a row group (see the template comment): the wave of key group 1 hands
        // its (m, l, O) -- per-lane values in the same layout as its partner's -- over through LDS, lane-linear
        // (16-B chunk j of lane L at (64 j + L) * 16: conflict-free both ways), behind the 16 KB the two storing
        // waves stage their 16-bit rows in.  m = max(m0, m1); l and O are brought to it and added
        // (exp2((m_i - m) c), the factor scale_l_O applies, softmax.cuh:36-49) -- per lane: the factors are the
        // same in the two lanes that share a row, so the deferred lane-pair sum of l commutes with the merge.
        static_assert(QT == 1, "one 32-row tile per wave");
        char *xo = smem + 2 * TR::kRowsPerWave * ROWB + wave_r * (DTILES * 4 * 64 * 16 + 2 * 64 * 4);
        float *xml = (float *)(xo + DTILES * 4 * 64 * 16);
        if (NT0 != 0) {
#pragma unroll
            for (int t = 0; t < DTILES; ++t)
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    *(f32x4 *)(xo + ((4 * t + j) * 64 + lane) * 16) =
                        f32x4{O[0][t][4 * j], O[0][t][4 * j + 1], O[0][t][4 * j + 2], O[0][t][4 * j + 3]};
            xml[lane] = m[0];
            xml[64 + lane] = l[0];
        }
        barrier();
        if (NT0 != 0) return;  // (no barrier follows: the storing waves work on wave-private LDS from here on)
        const float m1 = xml[lane], l1 = xml[64 + lane];
        const float m_all = fmaxf(m[0], m1);
        const float a0 = __builtin_amdgcn_exp2f((m[0] - m_all) * c), a1 = __builtin_amdgcn_exp2f((m1 - m_all) * c);
        l[0] = l[0] * a0 + l1 * a1;
#pragma unroll
        for (int t = 0; t < DTILES; ++t)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const f32x4 o1 = *(const f32x4 *)(xo + ((4 * t + j) * 64 + lane) * 16);
#pragma unroll
                for (int e = 0; e < 4; ++e) O[0][t][4 * j + e] = O[0][t][4 * j + e] * a0 + o1[e] * a1;
            }
    }
    {
        char *stage_o = smem + wave_r * (TR::kRowsPerWave * ROWB);
#pragma unroll
        for (int qt = 0; qt < QT; ++qt) {
#ifdef FA_KERNEL_VARLEN_SINKS
            float inv, lse_unused;   // (a row that saw no key: o = 0)
            sink_end(pair_sum(l[qt]), m[qt], inv, lse_unused);
#elif defined(FA_KERNEL_VARLEN)
            const float l_all = pair_sum(l[qt]);
#ifdef FA_KERNEL_VARLEN_KVCACHE_FP8
            // ... with v_descale folded in (read here, not held across the loop)
            const float inv = l_all == 0.0f ? 0.0f : (1.0f / l_all) * (fa8.v_descale ? fa8.v_descale[(int64_t)b * fa8.ds_bs + h / va.group] : 1.0f);
#else
            const float inv = l_all == 0.0f ? 0.0f : 1.0f / l_all;   // a row that saw no key: o = 0, not 0 / 0
#endif
#else
            const float inv = 1.0f / pair_sum(l[qt]);
#endif
            const int row = qt * 32 + r31;
            char *wp = stage_o + row * ROWB + hi * 8;
#pragma unroll
            for (int t = 0; t < DTILES; ++t) {
                float o[16];
#pragma unroll
                for (int r = 0; r < 16; ++r) o[r] = O[qt][t][r] * inv;
                // regs 4rq..4rq+3 : d = 32t + 8rq + 4hi + 0..3  -> chunk 4t + rq, half hi
                const s16x8 lo_s = __builtin_bit_cast(s16x8, E::pack8(o));
                const s16x8 up_s = __builtin_bit_cast(s16x8, E::pack8(o + 8));
                *(s16x4 *)(wp + (((4 * t + 0) ^ swz_of(row)) << 4)) = lo_s.lo;
                *(s16x4 *)(wp + (((4 * t + 1) ^ swz_of(row)) << 4)) = lo_s.hi;
                *(s16x4 *)(wp + (((4 * t + 2) ^ swz_of(row)) << 4)) = up_s.lo;
                *(s16x4 *)(wp + (((4 * t + 3) ^ swz_of(row)) << 4)) = up_s.hi;
            }
        }
        const int64_t row0 = (int64_t)qb * TR::kBr + wave_r * TR::kRowsPerWave;
        const int rsub = lane / CPR, chunk = lane & (CPR - 1);
#pragma unroll
        for (int i = 0; i < TR::kRowsPerWave / RPP; ++i) {
            const int row = RPP * i + rsub;
            const s16x8 v = *(const s16x8 *)(stage_o + row * ROWB + ((chunk ^ swz_of(row)) << 4));
            if (!MASK || row0 + row < FA_Q_LEN_END) *(s16x8 *)(Og + (row0 + row) * ss + chunk * 8) = v;
        }
    }
}

}  // namespace fa
