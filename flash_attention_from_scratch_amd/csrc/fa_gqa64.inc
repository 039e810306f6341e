// fa_gqa64.inc -- grouped-query attention in the persistent kernel (included by fa_fwd_kernel64.hpp).
// fa_fwd_kernel64_gqa is the LSE form (fa_fwd_kernel64_lse) whose K and V have n_heads / group heads and strides of their
// own; query head h reads K / V head h / group (flash-attn's and torch SDPA's convention).  Only fa_inst_gqa.hip defines
// FA_KERNEL64_GQA (with FA_KERNEL64_LSE) and gets that kernel instead of the other two.  What differs is the K / V
// addressing alone, through two macros the kernel body uses (defined here):
//   FA_KV_SS           the K / V seq stride: the per-lane DMA offsets and the tile step
//   FA_KV_OFF(b, h, o) the K / V head base of an item (the first item and set_next; the second pass of the speculative
//                      softmax walks the same code, so a redone item reads the same head)
// and the product's forms get `ss` and `o` back, the text they were compiled from before.  Q requests, the O epilogue and
// lse keep Q's strides and heads.  Same items in the same order, same arithmetic per item: O and lse are bit-identical to
// the LSE form on K / V expanded to n_heads heads (repeat_interleave).
// The kernel's own signature and arguments: fa_gqa64_kernel.inc.
struct KernelArgsGqa {
    KernelArgsLse lse;                                        // Q / O strides, n_heads (query heads), lse
    int64_t kv_batch_stride, kv_seq_stride, kv_head_stride;   // K and V, elements
    int32_t group;                                            // query heads per K / V head
};
typedef void (*kernel_fn_gqa)(const KernelArgsGqa);
#ifdef FA_KERNEL64_GQA
#define FA_KV_SS kv_ss
#define FA_KV_OFF(b, h, off) kv_off_of(b, h)
#else
#define FA_KV_SS ss
#define FA_KV_OFF(b, h, off) off
#endif
