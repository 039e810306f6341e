// fa_gqa64_kernel.inc -- (included by fa_fwd_kernel64.hpp in place of the kernel's signature when FA_KERNEL64_GQA is defined,
// i.e. only by fa_inst_gqa.hip) the signature of fa_fwd_kernel64_gqa and its K / V arguments; KernelArgsGqa and the K / V
// addressing macros are in fa_gqa64.inc.
template <int DT, bool MASK, bool SPEC, int ABL = 0, bool RAG = false, bool PSQ = false, int QTP = 2, bool ALT = false, int NW = 4>
__global__ void __launch_bounds__(256, 1) fa_fwd_kernel64_gqa(const KernelArgsGqa args_gqa) {
    static_assert(QTP == 2 && NW == 4 && !RAG && !PSQ && !ALT, "grouped-query attention: the 64-row plain and causal LSE forms");
    constexpr bool LSE = true;
    const KernelArgs &args = args_gqa.lse.base;
    // (the epilogue's lse base and row count live in VGPRs, as in fa_fwd_kernel64_lse)
    float *lse = args_gqa.lse.lse;
    int lse_len = args.seq_len;
    asm volatile("" : "+v"(lse), "+v"(lse_len));
    const int64_t kv_ss = args_gqa.kv_seq_stride;
    // The K / V head base of an item, b * kv_batch_stride + (h / group) * kv_head_stride: formed in VGPRs from strides kept in
    // VGPRs and read back as one scalar.  Held in SGPRs, the three values cost the general visits of the speculative forms two
    // spill reloads (the 512-register waves leave no SGPR to spare); here they cost item seams a few vector instructions.
    int64_t kv_bs = args_gqa.kv_batch_stride, kv_hs = args_gqa.kv_head_stride;
    int kv_group = args_gqa.group;
    asm volatile("" : "+v"(kv_bs), "+v"(kv_hs), "+v"(kv_group));
    auto kv_off_of = [&](int b_, int h_) -> int64_t {
        const int64_t o = (int64_t)b_ * kv_bs + (int64_t)(h_ / kv_group) * kv_hs;
        const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)o), hi32 = __builtin_amdgcn_readfirstlane((unsigned)(o >> 32));
        return (int64_t)(((unsigned long long)hi32 << 32) | lo);
    };
