// fa_kvcache_append_kernel.hpp -- the step in front of a KV-cache decode: append the new K / V rows to the
// cache at the positions the device-side lengths name, rotate the new keys and the query (rotary embedding), quantize for an
// fp8 cache, advance the lengths.  One kernel, one workgroup of 1024 threads per batch entry:
//  * len = clamp(cache_seqlens[b], 0, max_len), read once by every thread before anything is written.  New token t goes to cache
//    position len + t and is dropped at or beyond max_len; a paged cache is addressed as decode does (page = position /
//    page_size, block_table entry clamped to [0, num_pages)).  No address depends on anything else the device arrays hold.
//  * A work item is one 16-byte chunk (8 elements of d) of one row: 16 items per row.  Non-interleaved rotary pairs element i
//    with i + rotary_dim / 2: the item of chunk c < rotary_dim / 16 loads chunk c and chunk c + rotary_dim / 16, rotates and
//    stores both, and the items of the upper half's chunks do nothing -- no cross-lane traffic.  Interleaved rotary pairs
//    (2 i, 2 i + 1): four pairs inside one chunk.  Chunks at or beyond rotary_dim are copied.
//  * o1 = x1 c - x2 s, o2 = x1 s + x2 c in fp32 with unfused multiplies and adds, rounded once to the 16-bit type: the bits of
//    eager torch.  The key at position p uses table row min(p, seqlen_ro - 1); query row i uses position len + i with causal,
//    len otherwise (flash-attn's rule).  V is never rotated.
//  * fp8 cache: the (rotated, 16-bit-rounded) value x is stored as e4m3fn(clamp(x / descale, -448, 448)): IEEE fp32 division,
//    then round-to-nearest-even done in integer arithmetic (the algorithm of c10::Float8_e4m3fn, so ties, subnormals and NaN
//    give torch's bytes by construction); 8-byte stores (a chunk is 8 bytes of cache).
//  * seqlens_out[b] = min(len + seqlen_new, max_len) is stored by thread 0 behind a barrier: workgroup b is the only reader
//    and the only writer of entry b, so seqlens_out may be cache_seqlens itself.  No atomics, no flags.
#pragma once
#include <hip/hip_fp16.h>
#include <hip/hip_runtime.h>

#include <cstdint>

namespace fa {

struct AppendArgs {
    const uint16_t *k_new, *v_new;   // (batch, seqlen_new, n_kv_heads, 128), strides new_*
    void *k, *v;                     // the cache: 16-bit or e4m3fn elements, strides kv_* in elements of its type
    const uint16_t *q;               // (batch, seqlen_q, n_heads, 128) or null (no rotary)
    uint16_t *q_out;
    const uint16_t *cos, *sin;       // (seqlen_ro, rotary_dim / 2), row stride ro_ss; null = no rotary
    const int32_t *cache_seqlens;    // (batch)
    int32_t *seqlens_out;            // (batch); may be cache_seqlens
    const int32_t *block_table;      // (batch, bt_bs) or null
    const float *k_descale, *v_descale;   // (batch, n_kv_heads), row stride ds_bs; null = 1 (fp8 cache only)
    int64_t new_bs, new_ss, new_hs, q_bs, q_ss, q_hs, qo_bs, qo_ss, qo_hs;
    int64_t kv_bs, kv_ss, kv_hs;     // kv_bs: batch stride, or the page stride of a paged cache
    int64_t bt_bs, ds_bs, ro_ss;
    int32_t seqlen_new, seqlen_q, n_heads, n_kv_heads;
    int32_t max_len, page_size, num_pages;   // max_len: the capacity; page_size, num_pages: 0 for a contiguous cache
    int32_t rotary_dim, seqlen_ro, interleaved, causal;   // rotary_dim 0 = no rotary
};

namespace append {
// 16 waves: the loop is latency-bound (load, rotate, store), so a chunk of tokens for one entry wants as few trips as a workgroup allows
constexpr int THREADS = 1024, D = 128, CHUNKS = D / 8;

template <int DT>
static __device__ __forceinline__ float to_f32(uint32_t h) {
    if constexpr (DT == 15) return __uint_as_float(h << 16);
    else return __half2float(__ushort_as_half((unsigned short)h));
}

// round to nearest even; a NaN becomes the type's quiet NaN as torch's conversion gives it (bf16: 0x7fc0)
template <int DT>
static __device__ __forceinline__ uint32_t from_f32(float f) {
    if constexpr (DT == 15) {
        const uint32_t u = __float_as_uint(f);
        if (f != f) return 0x7fc0u;
        return (u + 0x7fffu + ((u >> 16) & 1u)) >> 16;
    } else {
        return (uint32_t)__half_as_ushort(__float2half_rn(f));
    }
}

// e4m3fn(clamp(x / d, -448, 448)), round to nearest even (c10::Float8_e4m3fn's integer algorithm); NaN -> 0x7f | sign
static __device__ __forceinline__ uint32_t to_e4m3(float x, float d) {
    float f = __fdiv_rn(x, d);
    f = f > 448.0f ? 448.0f : (f < -448.0f ? -448.0f : f);   // (a NaN passes both comparisons)
    uint32_t u = __float_as_uint(f);
    const uint32_t sign = u & 0x80000000u;
    u ^= sign;
    uint32_t r;
    if (u >= (1087u << 20)) {            // beyond 480: only a NaN gets here behind the clamp
        r = 0x7fu;
    } else if (u < (121u << 23)) {       // below 2^-6: e4m3's subnormals, rounded by an fp32 add
        r = __float_as_uint(__fadd_rn(__uint_as_float(u), __uint_as_float(141u << 23))) - (141u << 23);
    } else {
        const uint32_t odd = (u >> 20) & 1u;
        u += ((uint32_t)(7 - 127) << 23) + 0x7ffffu;
        u += odd;
        r = u >> 20;
    }
    return r | (sign >> 24);
}

// one pair: o1 = x1 c - x2 s, o2 = x1 s + x2 c, each product and sum rounded on its own
static __device__ __forceinline__ void rotate(float x1, float x2, float c, float s, float &o1, float &o2) {
    o1 = __fsub_rn(__fmul_rn(x1, c), __fmul_rn(x2, s));
    o2 = __fadd_rn(__fmul_rn(x1, s), __fmul_rn(x2, c));
}

// What one item stores: chunk c0 (x0) and, for a non-interleaved rotary pair, chunk c1 (x1); n = 0: nothing (the chunk is the
// upper half of a pair another item owns)
struct Item {
    uint4 x0, x1;
    int n, c1;
};

// row: the 128 elements of one (token, head); cosr / sinr: the table rows of its position (used only when half > 0);
// half = rotary_dim / 16, the chunks per half of the rotated part
template <int DT>
static __device__ __forceinline__ Item load_item(const uint16_t *row, int c, const uint16_t *cosr, const uint16_t *sinr, int half, bool interleaved) {
    Item it;
    it.n = 1;
    it.c1 = c;
    it.x0 = it.x1 = make_uint4(0, 0, 0, 0);
    if (!interleaved && c >= half && c < 2 * half) {   // the upper half of a pair: the item of chunk c - half owns it
        it.n = 0;
        return it;
    }
    it.x0 = *(const uint4 *)(row + 8 * c);
    if (c >= 2 * half) return it;   // beyond rotary_dim (or no rotary): pass through
    if (interleaved) {
        const uint2 cs = *(const uint2 *)(cosr + 4 * c), sn = *(const uint2 *)(sinr + 4 * c);
        const uint32_t xw[4] = {it.x0.x, it.x0.y, it.x0.z, it.x0.w};
        const uint32_t cw[2] = {cs.x, cs.y}, sw[2] = {sn.x, sn.y};
        uint32_t ow[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const uint32_t cj = (cw[j >> 1] >> (16 * (j & 1))) & 0xffffu, sj = (sw[j >> 1] >> (16 * (j & 1))) & 0xffffu;
            float o1, o2;
            rotate(to_f32<DT>(xw[j] & 0xffffu), to_f32<DT>(xw[j] >> 16), to_f32<DT>(cj), to_f32<DT>(sj), o1, o2);
            ow[j] = from_f32<DT>(o1) | (from_f32<DT>(o2) << 16);
        }
        it.x0 = make_uint4(ow[0], ow[1], ow[2], ow[3]);
        return it;
    }
    const uint4 hi = *(const uint4 *)(row + 8 * (c + half));
    const uint4 cs = *(const uint4 *)(cosr + 8 * c), sn = *(const uint4 *)(sinr + 8 * c);
    const uint32_t aw[4] = {it.x0.x, it.x0.y, it.x0.z, it.x0.w}, bw[4] = {hi.x, hi.y, hi.z, hi.w};
    const uint32_t cw[4] = {cs.x, cs.y, cs.z, cs.w}, sw[4] = {sn.x, sn.y, sn.z, sn.w};
    uint32_t lo_w[4], hi_w[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        float a1, a2, b1, b2;
        rotate(to_f32<DT>(aw[j] & 0xffffu), to_f32<DT>(bw[j] & 0xffffu), to_f32<DT>(cw[j] & 0xffffu), to_f32<DT>(sw[j] & 0xffffu), a1, a2);
        rotate(to_f32<DT>(aw[j] >> 16), to_f32<DT>(bw[j] >> 16), to_f32<DT>(cw[j] >> 16), to_f32<DT>(sw[j] >> 16), b1, b2);
        lo_w[j] = from_f32<DT>(a1) | (from_f32<DT>(b1) << 16);
        hi_w[j] = from_f32<DT>(a2) | (from_f32<DT>(b2) << 16);
    }
    it.x0 = make_uint4(lo_w[0], lo_w[1], lo_w[2], lo_w[3]);
    it.x1 = make_uint4(hi_w[0], hi_w[1], hi_w[2], hi_w[3]);
    it.n = 2;
    it.c1 = c + half;
    return it;
}

// eight 16-bit values -> eight e4m3fn bytes, lowest element first
template <int DT>
static __device__ __forceinline__ uint2 quantize8(uint4 x, float d) {
    const uint32_t w[4] = {x.x, x.y, x.z, x.w};
    uint32_t b[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) b[j] = to_e4m3(to_f32<DT>(w[j] & 0xffffu), d) | (to_e4m3(to_f32<DT>(w[j] >> 16), d) << 8);
    return make_uint2(b[0] | (b[1] << 16), b[2] | (b[3] << 16));
}
}  // namespace append

template <int DT, bool FP8>
__global__ void __launch_bounds__(append::THREADS) fa_kvcache_append_kernel(const AppendArgs a) {
    using namespace append;
    const int b = blockIdx.x;
    int len = a.cache_seqlens[b];
    len = len < 0 ? 0 : (len > a.max_len ? a.max_len : len);
    const int half = a.rotary_dim >> 4;
    const bool interleaved = a.interleaved != 0;
    const int last_ro = a.seqlen_ro - 1;

    // K, then V: (token, head, chunk) items
    const int kv_items = a.seqlen_new * a.n_kv_heads * CHUNKS;
    for (int i = threadIdx.x; i < 2 * kv_items; i += THREADS) {
        const bool is_v = i >= kv_items;
        const int r = is_v ? i - kv_items : i;
        const int c = r & (CHUNKS - 1), h = (r >> 4) % a.n_kv_heads, t = (r >> 4) / a.n_kv_heads;
        const int pos = len + t;
        if (pos >= a.max_len) continue;   // no room: the token is dropped
        const uint16_t *row = (is_v ? a.v_new : a.k_new) + (int64_t)b * a.new_bs + (int64_t)t * a.new_ss + (int64_t)h * a.new_hs;
        const int rot = is_v ? 0 : half;
        const int rr = pos < last_ro ? pos : last_ro;
        const Item it = load_item<DT>(row, c, a.cos + (int64_t)rr * a.ro_ss, a.sin + (int64_t)rr * a.ro_ss, rot, interleaved);
        if (it.n == 0) continue;
        int64_t base;
        if (a.page_size > 0) {
            const int page = pos / a.page_size;
            int p = a.block_table[(int64_t)b * a.bt_bs + page];
            p = p < 0 ? 0 : (p >= a.num_pages ? a.num_pages - 1 : p);
            base = (int64_t)p * a.kv_bs + (int64_t)(pos - page * a.page_size) * a.kv_ss;
        } else {
            base = (int64_t)b * a.kv_bs + (int64_t)pos * a.kv_ss;
        }
        base += (int64_t)h * a.kv_hs;
        if constexpr (FP8) {
            const float *ds = is_v ? a.v_descale : a.k_descale;
            const float d = ds ? ds[(int64_t)b * a.ds_bs + h] : 1.0f;
            uint8_t *dst = (uint8_t *)(is_v ? a.v : a.k) + base;
            *(uint2 *)(dst + 8 * c) = quantize8<DT>(it.x0, d);
            if (it.n == 2) *(uint2 *)(dst + 8 * it.c1) = quantize8<DT>(it.x1, d);
        } else {
            uint16_t *dst = (uint16_t *)(is_v ? a.v : a.k) + base;
            *(uint4 *)(dst + 8 * c) = it.x0;
            if (it.n == 2) *(uint4 *)(dst + 8 * it.c1) = it.x1;
        }
    }

    // Q (only with tables): row i at position len + i with causal, len otherwise
    if (a.q && half > 0) {
        const int q_items = a.seqlen_q * a.n_heads * CHUNKS;
        for (int i = threadIdx.x; i < q_items; i += THREADS) {
            const int c = i & (CHUNKS - 1), h = (i >> 4) % a.n_heads, t = (i >> 4) / a.n_heads;
            const int pos = a.causal ? len + t : len;
            const int rr = pos < last_ro ? pos : last_ro;
            const uint16_t *row = a.q + (int64_t)b * a.q_bs + (int64_t)t * a.q_ss + (int64_t)h * a.q_hs;
            const Item it = load_item<DT>(row, c, a.cos + (int64_t)rr * a.ro_ss, a.sin + (int64_t)rr * a.ro_ss, half, interleaved);
            if (it.n == 0) continue;
            uint16_t *dst = a.q_out + (int64_t)b * a.qo_bs + (int64_t)t * a.qo_ss + (int64_t)h * a.qo_hs;
            *(uint4 *)(dst + 8 * c) = it.x0;
            if (it.n == 2) *(uint4 *)(dst + 8 * it.c1) = it.x1;
        }
    }

    __syncthreads();   // every thread has its len: entry b may now be overwritten (seqlens_out may be cache_seqlens)
    if (threadIdx.x == 0) {
        const int64_t next = (int64_t)len + a.seqlen_new;
        a.seqlens_out[b] = next > a.max_len ? a.max_len : (int32_t)next;
    }
}

// one launch on s; arguments validated by the caller (fa_kvcache_append_launch, fa_capi.hip)
hipError_t kvcache_append_enqueue(const AppendArgs &a, int batch, int dtype, bool fp8, hipStream_t s);

}  // namespace fa
