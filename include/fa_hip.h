/*
 * fa_hip.h -- C ABI of libfa_hip.so, the MI355X (gfx950) Flash-Attention-2 forward.
 *
 * This is the drop-in boundary for the one hot path of
 * sonnyli/flash_attention_from_scratch: everything the reference's pybind module
 * `flash_attention_kernels` (src/flash_attention.cu) does below its tensor checks.
 * Plain pointers and sizes only -- no torch / ATen types -- so any host language
 * can bind it (ctypes stub: flash_attention_from_scratch_amd/_capi.py; see
 * INTEGRATION.md for the binding a reference maintainer would add).
 *
 * Reference interface each entry point replaces (paths under /root/reference):
 *   fa_fwd_config      <- FlashForwardKernelConfig, src/include/flash_attention.cuh:34-52
 *                         (13 fields, same order; Python side kernel_configs.py:106-120)
 *   fa_fwd_args        <- flash::ForwardKernelArgs, src/include/flash_attention.cuh:8-27
 *                         + the launcher locals of src/flash_attention.cu:58-108
 *   fa_fwd_supported   <- forward_kernels.contains(cfg), src/flash_attention.cu:60-61
 *   fa_fwd_lds_bytes   <- FlashForwardKernelConfig::smem_bytes(), flash_attention.cuh:54-56
 *   fa_fwd_launch      <- kernel<<<grid, block, smem, stream>>>(args), flash_attention.cu:110-126
 *   fa_fwd_launch_timed<- the benchmark=True event bracket, flash_attention.cu:119-132
 *   fa_fwd_launch_ex   <- the same launch with this library's NATIVE extensions (no reference counterpart):
 *                         causal / ragged seq_len, the speculative softmax, the pre-scaled Q, event timing,
 *                         device-side statistics -- one options struct (fa_fwd_opts)
 *   fa_init            <- PYBIND11_MODULE body (max dynamic smem opt-in), flash_attention.cu:142-149
 *   fa_num_kernels / fa_get_kernel <- iteration over the forward_kernels map,
 *                         src/include/flash_kernels.cuh:14-186
 *
 * Error behaviour: functions return 0 on success or a negative fa_status; the
 * message (the reference's TORCH_CHECK text where one exists) is available from
 * fa_last_error() on the calling thread.  Unlike the reference (which never calls
 * cudaGetLastError), launch failures are reported.
 *
 * Threading / streams: no internal threads.  Launches are asynchronous on the caller's
 * stream (graph-capturable); fa_fwd_launch_timed blocks on its stop event.  State:
 *   - fa_fwd_launch, fa_fwd_launch_timed, fa_fwd_launch_masked and fa_fwd_launch_ex with
 *     speculative = 0 or 1 are STATELESS, as the reference's launcher is
 *     (src/flash_attention.cu:42,118,126-131): nothing but the const kernel registry and
 *     the one-time per-device setup (fa_init) outlives a call, the same inputs give the
 *     same bits from any thread, process or stream.
 *   - fa_fwd_launch_ex with speculative = 2 (FA_SPECULATIVE_ADAPTIVE; what
 *     flash_helpers.kernel_configs.best_config() asks for) is NOT: it keeps, per device and
 *     per device variant, a small record (fa_adaptive_info) behind one mutex, one word of
 *     pinned host memory the kernels report into and one event; which of two valid variants
 *     serves a launch depends on that record, so the last bits of its output may differ from
 *     run to run on data that makes the speculative softmax fail.  The record is per process
 *     (two processes on one device do not see each other's).  See fa_speculative_mode.
 */
#ifndef FA_HIP_H
#define FA_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* torch ScalarType codes, as the reference's DType enum (kernel_configs.py:12-13). */
typedef enum fa_dtype { FA_FP16 = 5, FA_BF16 = 15 } fa_dtype;

typedef enum fa_status {
    FA_OK = 0,
    FA_ERR_NULL = -1,        /* null pointer argument */
    FA_ERR_DTYPE = -2,       /* "Only fp16 and bf16 are supported" */
    FA_ERR_NO_KERNEL = -3,   /* "Kernel configuration was not found ..." */
    FA_ERR_SHAPE = -4,       /* seq_len not a multiple of B_r / B_c, bad d_head, ... */
    FA_ERR_ALIGN = -5,       /* pointers / strides not 16-byte compatible */
    FA_ERR_LAUNCH = -6,      /* HIP launch or event error */
    FA_ERR_DEVICE = -7       /* not a gfx950 device / no device */
} fa_status;

/* The reference's 13-field kernel key.  Booleans are 0/1 ints. */
typedef struct fa_fwd_config {
    int32_t dtype;                   /* fa_dtype */
    int32_t d_head;                  /* 128 */
    int32_t B_r;                     /* Q rows per workgroup */
    int32_t B_c;                     /* keys per LDS tile */
    int32_t n_warps;                 /* wave64 wavefronts per workgroup */
    int32_t async_copy;              /* K/V by direct global->LDS DMA */
    int32_t eager_load_blocks;       /* double-buffered K/V prefetch */
    int32_t swizzled;                /* XOR-swizzled K image in LDS */
    int32_t Q_mma_load_K_tiles;      /* operand-fetch hints: validated, see DESIGN.md */
    int32_t K_mma_load_K_tiles;
    int32_t V_mma_load_K_tiles;
    int32_t mma_double_buffer_loads;
    int32_t optimized_softmax;       /* the reference's meaning and nothing else: the first KV block skips the
                                        (l, O) rescale (softmax.cuh:85-105, forward_kernel.cuh:158-161).  The
                                        result is identical with or without it (the skipped factor is exp2(-inf)
                                        = 0 on l = O = 0), so device variants whose schedule has no first-block
                                        rescale to skip accept the flag and ignore it (fa_kernel_info.softmax_mode
                                        says what a variant does).  The speculative softmax is NOT selected by
                                        this field: fa_fwd_opts.speculative */
} fa_fwd_config;

/* How a device variant keeps exp2 in range (fa_kernel_info.softmax_mode).  All four give the same real
 * result; the first two are the reference's arithmetic bit for bit, the other two move the rounding
 * point of P and are checked against the same tolerances. */
typedef enum fa_softmax_mode {
    FA_SOFTMAX_EAGER = 0,            /* running row max, (l, O) rescaled at every tile (softmax.cuh:85-105) */
    FA_SOFTMAX_FIRST_BLOCK_SKIP = 1, /* the same, first KV block skips the rescale (the reference's optimized_softmax) */
    FA_SOFTMAX_LAZY = 2,             /* running row max, moved only when some row's max rose by > 8 binades */
    FA_SOFTMAX_SPECULATIVE = 3       /* reference = row max of the item's first visited tile, no per-tile max;
                                        the row sums are checked at the end and an item that fails is computed
                                        again with the running max (counted: fa_fwd_stats.items_redone) */
} fa_softmax_mode;

/*
 * One forward call.  q, k, v, o are DEVICE pointers to (batch, seq_len, n_heads,
 * d_head) tensors of the 16-bit dtype in cfg.dtype whose last dimension is
 * contiguous; the three strides are in ELEMENTS and shared by all four tensors
 * (flash_attention.cuh:14-19).  o may alias none of the inputs.  Strides must be positive multiples of 8;
 * seq_stride additionally <= (2^32 - 1) / (2 max(B_r, B_c)) (32-bit per-lane offsets inside a tile); the
 * batch and head strides are used in 64-bit arithmetic.
 */
typedef struct fa_fwd_args {
    const void *q;
    const void *k;
    const void *v;
    void *o;
    int64_t batch;
    int64_t seq_len;
    int64_t n_heads;
    int64_t d_head;
    int64_t batch_stride;
    int64_t seq_stride;
    int64_t head_stride;
    fa_fwd_config cfg;
} fa_fwd_args;

/* Resource report of one registered kernel (code-object metadata via HIP). */
typedef struct fa_kernel_info {
    fa_fwd_config cfg;       /* canonical config of the device variant */
    int32_t threads;         /* workgroup size */
    int32_t lds_bytes;       /* dynamic LDS per workgroup */
    int32_t num_regs;        /* VGPR+AGPR per lane (hipFuncAttributes.numRegs) */
    int32_t scratch_bytes;   /* per-thread scratch; 0 = no spills */
    int32_t rows_per_wave;   /* Q rows owned by one wavefront */
    int32_t masked;          /* 1: the causal / ragged-length variant of cfg; 2: the same for the persistent
                                (256, 64, 4) kernel, which needs seq_len >= B_c when seq_len % B_r != 0 */
    int32_t softmax_mode;    /* fa_softmax_mode of this device variant */
    int32_t prescaled_q;     /* 1: the variant folds the softmax scale into a 16-bit copy of Q (fa_fwd_opts.prescaled_q) */
    /* ABI 5: the RING FORM of a 32-rows-per-wave configuration -- (B_r 128, B_c 64, 4 warps) + buffer, the reference's own
     * winning tile shape: launches with seq_len % 256 == 0 are served by the hand-placed persistent kernel with one
     * 32-row Q tile per wave (the machinery of the (256, 64, 4) kernel: its lazy rescale for the plain variant,
     * bit-identical to that kernel's non-speculative form, and its speculative schedule for the speculative variant,
     * whose failed items are redone by the lazy one), the other multiples of B_r by the variant described above. */
    int32_t ring_form;           /* 1: such a form exists for this variant.  Round 6: it runs EIGHT waves of one Q tile each (512
                                    threads; two of the configuration's 128-row Q blocks make one 256-row item, counted as two in
                                    fa_fwd_stats) sharing one set of K / V rings -- same bits as the four-wave form of ABI 5 */
    int32_t ring_softmax_mode;   /* its fa_softmax_mode (FA_SOFTMAX_LAZY or FA_SOFTMAX_SPECULATIVE) */
    int32_t ring_num_regs;       /* VGPR+AGPR per lane of the ring form */
    int32_t ring_scratch_bytes;  /* 0 = no spills */
    /* ABI 6: what a launch of the ring form occupies -- lds_bytes / threads above describe the OTHER form */
    int32_t ring_lds_bytes;      /* dynamic LDS per workgroup of the ring form (160 KiB: one workgroup per CU); 0 without one */
    int32_t persistent;          /* 1: the variant (`fn`; a ring form always) is launched as one workgroup per CU that walks the
                                    (batch*head, Q block) items itself -- the grid is min(items, CUs rounded down to 8) */
    int32_t alt_form;            /* 1: long sequences run a second device form of this variant, whose speculative first pass
                                    walks every second round of a head's Q blocks [K / V tile 0, then last-to-second] so that
                                    the tail a round left in the XCD's L2 is read again first (taken when batch * heads is a
                                    multiple of 8 and seq_len / B_r is a multiple of 2 * grid / 8: seq_len 16384, 32768, ... on
                                    256 CUs).  Same tiles and arithmetic per tile; which way an item walks depends on its Q
                                    block and the CU count only, never on the batch.  (FA_HIP_NO_ALT in the environment, read
                                    once per process, sends such launches through the plain form: a MEASUREMENT switch for
                                    A/B runs -- profiles/r06/c3_alt_ab.txt, tools/l2_stride_probe.py -- that nothing sets) */
    int32_t ring_threads;        /* workgroup size of the ring form (512: eight waves, round 6); 0 without one */
} fa_kernel_info;

/* Device-side statistics (optional, fa_fwd_opts.stats): a DEVICE pointer to two 32-bit counters the
 * kernel ADDS to (zero them yourself).  items = work items (batch*head, Q block) computed;
 * items_redone = items the speculative softmax had to compute a second time because a row sum
 * exceeded its limit -- the cost of such an item is 2x.  0 for every other softmax mode.  The persistent kernel keeps a
 * workgroup's failures in a 64-bit mask of its walk ordinals, and ordinals >= 63 share the last bit: on a problem with
 * more than 63 items per workgroup (> ~16 000 items on a 256-CU device) a failure at ordinal >= 63 makes the workgroup
 * compute, and count, ALL its items from ordinal 63 on again -- items_redone is what ran twice, which there can exceed
 * what had to. */
typedef struct fa_fwd_stats {
    uint32_t items;
    uint32_t items_redone;
} fa_fwd_stats;

/* fa_fwd_opts.speculative.  ADAPTIVE: the speculative variant, except that the library watches the failure reports of its
 * speculative launches on the device (a failed item costs its workgroup a second item time, and a launch ends with its
 * slowest workgroup: one failing item in a thousand costs a quarter of a 4-items-per-CU launch, everything failing 2x):
 *   NORMAL   every launch speculative; a report -> the next `hold` adaptive launches take the NON-speculative variant of cfg
 *   DEMOTED  ... after which ONE launch probes the speculative variant again (an event is recorded behind it)
 *   PROBING  launches stay demoted until the probe has completed (hipEventQuery, never a wait); a probe that reported too
 *            doubles `hold` (32 ... 4096), one that did not returns the device to NORMAL.
 * The report is one word of pinned host memory a failing workgroup stores into; the library reads it when an adaptive
 * launch is enqueued and never waits for the device.  Both variants compute the same real result within the same
 * tolerance (they round P at different points), so WHICH of the two served a launch -- which depends on when a report
 * arrived -- is visible only in the last bits: ask for 0 or 1 where bit-reproducible output matters.  A launch made
 * during a stream capture is always speculative (nothing adaptive is recorded into a graph).  State per device AND per
 * device variant (ABI 5: a failing fp16 layer no longer demotes a benign bf16 one on the same device, and a probe's verdict
 * belongs to the configuration that probed): fa_adaptive_state (the device's records taken together),
 * fa_adaptive_state_for (one configuration's), fa_adaptive_reset (all of the device's). */
typedef enum fa_speculative_mode {
    FA_SPECULATIVE_OFF = 0,
    FA_SPECULATIVE_ALWAYS = 1,
    FA_SPECULATIVE_ADAPTIVE = 2
} fa_speculative_mode;

typedef struct fa_adaptive_info {
    uint32_t available;      /* 1: the pinned report word exists on this device (else ADAPTIVE behaves like ALWAYS) */
    uint32_t launches;       /* adaptive launches enqueued so far (fa_adaptive_state: summed over the device's records) */
    uint32_t demoted;        /* ... of which took the non-speculative variant */
    uint32_t reports;        /* distinct failure reports acted on */
    uint32_t hold;           /* current length of a demotion, in adaptive launches */
    uint32_t mode;           /* 0 NORMAL, 1 DEMOTED, 2 PROBING */
    uint32_t remaining;      /* DEMOTED: launches of the hold still to come */
    uint32_t last_report;    /* sequence number of the most recent launch that reported (0: none yet) */
} fa_adaptive_info;

/* Options of fa_fwd_launch_ex: this library's extensions beyond the reference's launch.  Zero-initialise,
 * set struct_size = sizeof(fa_fwd_opts), then set what you need. */
typedef struct fa_fwd_opts {
    uint32_t struct_size;    /* sizeof(fa_fwd_opts) of the caller's header */
    int32_t causal;          /* key j contributes to query i iff j <= i (masked variant of cfg); seq_len still has to be a
                                multiple of B_r and B_c unless allow_ragged is set too */
    int32_t allow_ragged;    /* accept seq_len that is not a multiple of B_r / B_c (masked variant of cfg) */
    int32_t speculative;     /* fa_speculative_mode.  1: the speculative-softmax variant of cfg (FA_SOFTMAX_SPECULATIVE); 2: the same,
                                adaptively -- see fa_speculative_mode below.  A row may rise, above the max of
                                its LAST 64 keys (visited first), by ~44 nats (bf16) / ~10 nats (fp16) before its item is
                                computed a second time; the persistent kernel also re-centres rising rows every four visits,
                                so there only a JUMP of ~83 nats (bf16) / ~1.4-10 nats (fp16) inside 256 keys fails.  The result is
                                right either way; fa_fwd_stats counts the items that ran twice.  See INTEGRATION.md 5 */
    int32_t prescaled_q;     /* 1: logits from a 16-bit Q * (log2 e / sqrt d) instead of an fp32 multiply per logit: a logit moves by
                                ~|k| |q c| 2^-9 (bf16) / 2^-12 (fp16) -- FA-3 / Triton practice, not the reference's arithmetic;
                                inside the reference's tolerance rule on benchmark-like data, outside it when keys of very
                                large norm (~30 sigma) appear; see DESIGN.md 3.7 */
    float *ms;               /* HOST pointer or NULL: bracket the launch with events, block, return elapsed ms */
    fa_fwd_stats *stats;     /* DEVICE pointer or NULL */
} fa_fwd_opts;

/* One-time setup for the CURRENT device (idempotent; also called lazily by every launch): arch check,
 * CU count, the > 48 KB dynamic-LDS opt-in of every kernel function.  State is kept per device ordinal,
 * so a host that drives several GPUs from one process initialises each at its first call there
 * (the reference: device guard src/flash_attention.cu:42 + module init :142-149).  fa_fwd_launch itself is
 * one plain kernel launch -- capturable into a hipGraph -- but this setup queries the device: call
 * fa_init() on the device BEFORE starting a stream capture there. */
int fa_init(void);

/* Introspection of that per-device state (tests): has `device` been initialised, with which status,
 * and how many CUs cap the persistent grid there.  Any out pointer may be NULL.  Safe to call from any
 * thread at any time: `inited` is published (release) after status and num_cus are final. */
int fa_device_state(int device, int *inited, int *status, int *num_cus);

/* 1 if a device kernel exists for cfg, else 0 (never negative). */
int fa_fwd_supported(const fa_fwd_config *cfg);

/* Dynamic LDS bytes the kernel for cfg uses, or a negative fa_status. */
int fa_fwd_lds_bytes(const fa_fwd_config *cfg);

/* Enqueue the forward on `stream` (a hipStream_t; NULL = default stream). */
int fa_fwd_launch(const fa_fwd_args *args, void *stream);

/* Same, bracketed by hipEvents on `stream`; blocks; *ms = elapsed milliseconds. */
int fa_fwd_launch_timed(const fa_fwd_args *args, void *stream, float *ms);

/*
 * Scope wideners beyond the reference (README.md:7-15 lists them as unsupported):
 * an optional causal mask (key j contributes to query i iff j <= i; equal Q/K lengths) and
 * seq_len that is NOT a multiple of B_r / B_c.  Same argument contract as fa_fwd_launch
 * otherwise.  ms == NULL: asynchronous; ms != NULL: timed like fa_fwd_launch_timed.
 * fa_fwd_masked_supported: 1 if a masked device variant exists for cfg.
 */
int fa_fwd_masked_supported(const fa_fwd_config *cfg);
int fa_fwd_launch_masked(const fa_fwd_args *args, int causal, void *stream, float *ms);

/* The general launch: fa_fwd_launch (opts == NULL or all zero), fa_fwd_launch_timed (opts->ms) and
 * fa_fwd_launch_masked (opts->causal / allow_ragged) are special cases of it.  fa_fwd_ex_supported: 1 if a
 * device variant exists for cfg with these options. */
int fa_fwd_ex_supported(const fa_fwd_config *cfg, const fa_fwd_opts *opts);
/* Which device variant would serve cfg with these options (opts may be NULL)?  Fills *out like fa_get_kernel
 * -- softmax_mode says what the variant does with the softmax -- or returns FA_ERR_NO_KERNEL. */
int fa_fwd_query(const fa_fwd_config *cfg, const fa_fwd_opts *opts, fa_kernel_info *out);
int fa_fwd_launch_ex(const fa_fwd_args *args, const fa_fwd_opts *opts, void *stream);

/*
 * The training path: the forward that also writes the row log-sum-exp, and the backward (dQ, dK, dV).
 *
 * lse[b, h, i] = ln sum_j exp(q_i . k_j / sqrt(d_head)) over the keys query i sees (causal: j <= i), fp32, in a contiguous
 * (batch, n_heads, seq_len) DEVICE buffer -- the convention of flash-attn's softmax_lse and of torch's flash SDPA logsumexp.
 *
 * fa_fwd_lse_supported: 1 if fa_fwd_launch_lse serves cfg with these options, else 0.  Served: the persistent 64-rows-per-
 * wave configuration (B_r 256, B_c 64, 4 warps) + buffer, d_head 128, bf16 / fp16, plain or causal, speculative (1 or 2) or
 * not, allow_ragged or not (a ragged seq_len is refused at the launch).  Not served: prescaled_q, every other configuration
 * (the 32- and 16-rows-per-wave kernels, the ring form).
 * fa_fwd_launch_lse: fa_fwd_launch_ex (opts: causal, speculative, ms, stats) with the same O bits as that call on the same
 * device variant, plus lse.  seq_len must be a multiple of 256 and seq_stride a multiple of 128 (FA_ERR_SHAPE otherwise).
 * Long sequences that fa_fwd_launch_ex sends through the alternating-direction form (fa_kernel_info.alt_form) take the
 * plain walk here: O then differs from fa_fwd_launch_ex in the fp32 summation order only.
 */
int fa_fwd_lse_supported(const fa_fwd_config *cfg, const fa_fwd_opts *opts);
int fa_fwd_launch_lse(const fa_fwd_args *args, const fa_fwd_opts *opts, float *lse, void *stream);

/*
 * One backward: given Q, K, V, the forward's O and lse and the gradient dO, writes dQ, dK and dV.  d_head 128, bf16 / fp16,
 * seq_len a multiple of 256, causal (key j contributes to query i iff j <= i) or not.  All pointers are DEVICE pointers.
 * q, k, v, o, dout, dq, dk, dv point to (batch, seq_len, n_heads, d_head) tensors of the 16-bit dtype with a contiguous
 * last dimension, 16-byte aligned; lse and workspace (fp32) need 4-byte alignment.
 * q, k, v share the qkv_* strides (a packed (B, S, 3, H, D) QKV passes without a copy), o, dout, dq, dk, dv the out_*
 * strides; all strides are in elements, positive multiples of 8, and seq_stride * 256 * 2 bytes must fit 32 bits.
 * dq, dk, dv are overwritten, and may alias none of the inputs.  workspace: fa_bwd_workspace_bytes(args) bytes of device
 * memory (fp32 delta_i = sum_d dO_id O_id), private to the call until it completes.
 * Deterministic: no float atomics, no ordering between workgroups -- the same inputs give the same bits.
 * fa_bwd_launch enqueues on `stream`; ms != NULL brackets the launches with events, blocks and returns the elapsed ms.
 */
typedef struct fa_bwd_args {
    const void *q;
    const void *k;
    const void *v;
    const void *o;
    const void *dout;
    const float *lse;        /* (batch, n_heads, seq_len) fp32, contiguous */
    void *dq;
    void *dk;
    void *dv;
    void *workspace;
    int64_t batch;
    int64_t seq_len;
    int64_t n_heads;
    int64_t d_head;
    int64_t qkv_batch_stride;
    int64_t qkv_seq_stride;
    int64_t qkv_head_stride;
    int64_t out_batch_stride;
    int64_t out_seq_stride;
    int64_t out_head_stride;
    int32_t dtype;           /* fa_dtype */
    int32_t causal;
} fa_bwd_args;
int64_t fa_bwd_workspace_bytes(const fa_bwd_args *args);              /* bytes, or a negative fa_status */
int fa_bwd_launch(const fa_bwd_args *args, void *stream, float *ms);

/*
 * Grouped-query attention (GQA; multi-query attention is n_kv_heads = 1): K and V have n_kv_heads heads, n_kv_heads divides
 * n_heads, and query head h reads K / V head h / (n_heads / n_kv_heads) -- the convention of flash-attn and of torch SDPA's
 * enable_gqa.  Q, O, dO, dQ and lse keep n_heads heads; K, V, dK and dV have n_kv_heads heads and strides of their own.
 *
 * fa_kv_layout: K's and V's head count and strides (elements; K and V share them).  struct_size = sizeof(fa_kv_layout).
 * fa_fwd_gqa_supported: 1 if fa_fwd_launch_gqa serves cfg with these options (the configurations and options
 * fa_fwd_lse_supported serves), else 0.
 * fa_fwd_launch_gqa: fa_fwd_launch_lse with K / V described by kv (args: Q, O, n_heads and their strides; args->k, ->v
 * the K / V pointers).  O and lse are bit-identical to fa_fwd_launch_lse on K / V expanded to n_heads heads.  lse is
 * required (FA_ERR_NULL).  Refused before any HIP call: configurations without the form and prescaled_q
 * (FA_ERR_NO_KERNEL); n_kv_heads < 1 or not dividing n_heads, seq_len % 256 != 0 (ragged lengths included), seq_stride %
 * 128 != 0, K / V strides that are not positive or whose 256 rows * kv_seq_stride * 2 bytes exceed 32 bits (FA_ERR_SHAPE);
 * K / V strides not multiples of 8 (FA_ERR_ALIGN).
 */
typedef struct fa_kv_layout {
    uint32_t struct_size;
    int64_t n_kv_heads;
    int64_t kv_batch_stride;
    int64_t kv_seq_stride;
    int64_t kv_head_stride;
} fa_kv_layout;
int fa_fwd_gqa_supported(const fa_fwd_config *cfg, const fa_fwd_opts *opts);
int fa_fwd_launch_gqa(const fa_fwd_args *args, const fa_kv_layout *kv, const fa_fwd_opts *opts, float *lse, void *stream);

/*
 * The backward of grouped-query attention.  base: as for fa_bwd_launch, with qkv_* the strides of Q alone, out_* those of
 * O, dO and dQ, and base.k, .v, .dk, .dv pointing to (batch, seq_len, n_kv_heads, d_head) tensors with the kv_* (K, V) and
 * dkv_* (dK, dV) strides.  dQ is bit-identical to fa_bwd_launch on K / V expanded to n_heads heads; dK and dV sum the
 * group's query heads in fp32 and are rounded once.  When batch * n_kv_heads * seq_len / 128 workgroups would be too few
 * for the device (fewer than 256 plain, 1024 causal), a group's heads are split across workgroups whose fp32 partials
 * are summed in a fixed order: the workspace (fa_bwd_gqa_workspace_bytes) then holds them too, and workspace must be
 * 16-byte aligned.  Deterministic like fa_bwd_launch.
 */
typedef struct fa_bwd_gqa_args {
    fa_bwd_args base;
    int64_t n_kv_heads;
    int64_t kv_batch_stride;
    int64_t kv_seq_stride;
    int64_t kv_head_stride;
    int64_t dkv_batch_stride;
    int64_t dkv_seq_stride;
    int64_t dkv_head_stride;
} fa_bwd_gqa_args;
int64_t fa_bwd_gqa_workspace_bytes(const fa_bwd_gqa_args *args);      /* bytes, or a negative fa_status */
int fa_bwd_launch_gqa(const fa_bwd_gqa_args *args, void *stream, float *ms);

/*
 * Packed variable-length sequences (flash-attn's varlen interface), forward with lse and backward, MHA and GQA / MQA, plain
 * and causal, bf16 / fp16, d_head 128.  All tokens of all sequences lie in one (total_tokens, heads, 128) tensor; sequence i
 * owns token rows cu_seqlens[i] .. cu_seqlens[i + 1] - 1; Q and K / V share cu_seqlens; a query attends to the keys of its
 * own sequence only (causal: at or before its own position in it).  Any length >= 0 is valid.
 *
 * fa_varlen_layout: cu_seqlens is a DEVICE pointer to n_seqs + 1 int32 (4-byte aligned) which the host never reads: the
 * launches stay asynchronous and graph-capturable.  The contract is the caller's -- non-decreasing, cu_seqlens[0] = 0,
 * cu_seqlens[n_seqs] = total_tokens, every length <= max_seqlen (a loose bound only costs idle workgroups) -- but a
 * violation cannot fault: every kernel clamps a sequence's first row to [0, total_tokens] and its length to [0, min(max_seqlen,
 * total_tokens - first row)].  Results for a violated contract are unspecified; memory outside the tensors is never touched.
 *
 * fa_fwd_launch_varlen: args carries q, o (token stride seq_stride, head_stride), k, v, n_heads, d_head and cfg; args->batch,
 * ->seq_len and ->batch_stride are IGNORED.  kv: K's and V's heads and strides (kv_batch_stride ignored; n_kv_heads = n_heads
 * for MHA).  lse: (n_heads, total_tokens) fp32, contiguous (flash-attn's layout for packed input), required.  opts: causal and
 * ms; speculative, prescaled_q and stats have no varlen form and are refused (FA_ERR_NO_KERNEL), allow_ragged is implied.
 * Served (fa_fwd_varlen_supported): the configurations whose masked variant is the 32-rows-per-wave kernel of the
 * (B_r 128, B_c 64, 4 warps) + buffer shape at d_head 128; O of sequence i is bit-identical to fa_fwd_launch_ex (allow_ragged)
 * of that variant on the sequence alone.  total_tokens = 0 returns FA_OK without a launch.
 *
 * fa_bwd_launch_varlen: q_* are Q's strides, out_* those of O, dO and dQ, kv_* of K and V, dkv_* of dK and dV (elements,
 * positive multiples of 8, token stride * 256 * 2 bytes within 32 bits).  The dK / dV kernel runs n_seqs * n_kv_heads * split *
 * ceil(max_seqlen / 128) workgroups; split is the smallest divisor of n_heads / n_kv_heads for which that count reaches 256
 * (1024 causal), else the whole group: a function of n_seqs, max_seqlen, the head counts and causal, never of what
 * cu_seqlens holds.  workspace: fa_bwd_varlen_workspace_bytes bytes (delta, and the split's fp32 partials), 16-byte aligned.
 * Deterministic like fa_bwd_launch; for sequences whose length is a multiple of 256 dQ has fa_bwd_launch's bits, dK / dV too
 * where the two launches use the same split.
 */
typedef struct fa_varlen_layout {
    uint32_t struct_size;
    const int32_t *cu_seqlens;
    int64_t n_seqs;
    int64_t total_tokens;
    int64_t max_seqlen;
} fa_varlen_layout;
int fa_fwd_varlen_supported(const fa_fwd_config *cfg, const fa_fwd_opts *opts);
int fa_fwd_launch_varlen(const fa_fwd_args *args, const fa_kv_layout *kv, const fa_varlen_layout *varlen, const fa_fwd_opts *opts,
                         float *lse, void *stream);
typedef struct fa_bwd_varlen_args {
    const void *q;
    const void *k;
    const void *v;
    const void *o;
    const void *dout;
    const float *lse;        /* (n_heads, total_tokens) fp32, contiguous */
    void *dq;
    void *dk;
    void *dv;
    void *workspace;
    int64_t n_heads;
    int64_t n_kv_heads;
    int64_t d_head;
    int64_t q_seq_stride;
    int64_t q_head_stride;
    int64_t out_seq_stride;
    int64_t out_head_stride;
    int64_t kv_seq_stride;
    int64_t kv_head_stride;
    int64_t dkv_seq_stride;
    int64_t dkv_head_stride;
    int32_t dtype;           /* fa_dtype */
    int32_t causal;
    fa_varlen_layout varlen;
} fa_bwd_varlen_args;
int64_t fa_bwd_varlen_workspace_bytes(const fa_bwd_varlen_args *args);   /* bytes, or a negative fa_status */
int fa_bwd_launch_varlen(const fa_bwd_varlen_args *args, void *stream, float *ms);

/*
 * Packed sequences with SEPARATE Q and K / V lengths (flash-attn's cu_seqlens_q / cu_seqlens_k): cross-attention, chunked
 * prefill behind a prefix, verification of many speculative rows -- forward with lse and backward.  q, o, dout, dq are
 * (total_q, n_heads, 128), k, v, dk, dv (total_k, n_kv_heads, 128); sequence i owns query rows varlen_q.cu_seqlens[i] ..
 * [i + 1] - 1 and key rows varlen_k.cu_seqlens[i] .. [i + 1] - 1.  Two fa_varlen_layout, one per side: n_seqs must match,
 * total_tokens and max_seqlen are that side's; each is clamped by the rule above against its own bounds.  Any lengths >= 0
 * are valid, independently.  causal is BOTTOM-RIGHT aligned, as in fa_decode_launch: query r of a sequence sees keys
 * j <= r + (len_k - len_q).  A row that sees no key (len_k = 0; causal rows r < len_q - len_k) gives o = 0, lse = -inf,
 * dq = 0; a key no query sees (len_q = 0: under the bottom-right mask the last row sees every key) gets dk = dv = 0, written.
 * lse is (n_heads, total_q) fp32.
 *
 * fa_fwd_launch_varlen_qk / fa_fwd_varlen_qk_supported: the arguments, the served configurations and the refusals of
 * fa_fwd_launch_varlen.  total_q = 0 returns FA_OK without a launch; total_k = 0 with total_q > 0 launches and writes the
 * zeros and -inf.  One kernel serves both: fa_fwd_launch_varlen is this launch with its one layout on both sides, so with
 * varlen_k equal to varlen_q, o and lse are bit-identical to fa_fwd_launch_varlen's.
 *
 * fa_bwd_varlen_qk_args: the fields of fa_bwd_varlen_args (varlen: the QUERY side) behind a struct_size, and varlen_k.  The
 * dK / dV kernel runs n_seqs * n_kv_heads * split * ceil(max_seqlen_k / 128) workgroups, split by fa_bwd_launch_varlen's rule
 * with max_seqlen_k in place of max_seqlen; partials and their sum run over total_k.  The dQ kernel runs n_seqs * n_heads *
 * ceil(max_seqlen_q / 128) workgroups.  workspace: fa_bwd_varlen_qk_workspace_bytes bytes, 16-byte aligned.  Deterministic;
 * with equal sides dq, dk, dv are bit-identical to fa_bwd_launch_varlen's and the workspace size is the same (kernels of
 * its own beside fa_bwd_launch_varlen's, which are the faster ones for one range: checks, split and workspace are shared).
 */
int fa_fwd_varlen_qk_supported(const fa_fwd_config *cfg, const fa_fwd_opts *opts);
int fa_fwd_launch_varlen_qk(const fa_fwd_args *args, const fa_kv_layout *kv, const fa_varlen_layout *varlen_q,
                            const fa_varlen_layout *varlen_k, const fa_fwd_opts *opts, float *lse, void *stream);
typedef struct fa_bwd_varlen_qk_args {
    uint32_t struct_size;    /* sizeof(fa_bwd_varlen_qk_args) */
    const void *q;
    const void *k;
    const void *v;
    const void *o;
    const void *dout;
    const float *lse;        /* (n_heads, total_q) fp32, contiguous */
    void *dq;
    void *dk;
    void *dv;
    void *workspace;
    int64_t n_heads;
    int64_t n_kv_heads;
    int64_t d_head;
    int64_t q_seq_stride;
    int64_t q_head_stride;
    int64_t out_seq_stride;
    int64_t out_head_stride;
    int64_t kv_seq_stride;
    int64_t kv_head_stride;
    int64_t dkv_seq_stride;
    int64_t dkv_head_stride;
    int32_t dtype;           /* fa_dtype */
    int32_t causal;          /* bottom-right aligned */
    fa_varlen_layout varlen;     /* the query rows */
    fa_varlen_layout varlen_k;   /* the key rows */
} fa_bwd_varlen_qk_args;
int64_t fa_bwd_varlen_qk_workspace_bytes(const fa_bwd_varlen_qk_args *args);   /* bytes, or a negative fa_status */
int fa_bwd_launch_varlen_qk(const fa_bwd_varlen_qk_args *args, void *stream, float *ms);

/*
 * Prefill against a KV cache (flash-attn's flash_attn_varlen_func(..., block_table=)): fa_fwd_launch_varlen_qk whose key side is
 * a cache, contiguous or paged, instead of a packed tensor -- chunked prefill behind a cached prefix, prompt processing behind a
 * shared prefix, verification of more speculative rows than fa_decode_launch serves.  Forward only, with lse.
 *
 * args, kv, varlen_q, opts, lse, stream: as for fa_fwd_launch_varlen_qk; args->k, ->v are the caches and kv their strides:
 *   contiguous cache (block_table null):  (n_seqs, seqlen_cache, n_kv_heads, 128); kv_batch_stride is the batch stride;
 *   paged cache (block_table non-null):   (num_pages, page_size, n_kv_heads, 128); kv_batch_stride is the PAGE stride, and
 *     block_table is a DEVICE (n_seqs, max_pages_per_seq) int32 array, row stride block_table_stride: key j of sequence b
 *     is row j % page_size of page block_table[b][j / page_size]             (the two shapes of fa_decode_args).
 * fa_kvcache_layout: struct_size = sizeof(fa_kvcache_layout).  cache_seqlens: DEVICE (n_seqs) int32, the valid keys of each
 * sequence, the chunk's own keys (which the caller has already written, with fa_kvcache_append_launch for one) included.  The
 * host reads neither it nor block_table: launches are asynchronous and graph-capturable.  max_seqlen_k: the host's bound on
 * every length, 0 = the capacity.
 * causal is BOTTOM-RIGHT aligned: query r of sequence b sees keys j <= r + (len_k - len_q).  A row that sees no key gives
 * o = 0, lse = -inf.  The grid is n_seqs * n_heads * ceil(max_seqlen_q / 128) workgroups: no split, no workspace, no atomics,
 * the same bits for the same inputs -- and the bits of fa_fwd_launch_varlen_qk on the same keys packed.
 *
 * Clamping: len_k to [0, min(capacity, max_seqlen_k)], capacity = seqlen_cache (paged: max_pages_per_seq * page_size); the
 * query range by fa_varlen_layout's rule; every block_table entry used to [0, num_pages), and only entries of pages below
 * ceil(len_k / page_size) are read; cache rows at or beyond len_k are never fetched (their lanes fetch row len_k - 1, which
 * lies in the same page, and are masked).  So neither stale rows nor unused pages nor unused block_table entries reach a
 * result, and no address outside the tensors is formed, whatever the three device arrays hold.
 *
 * Served (fa_fwd_varlen_kvcache_supported): the configurations and options of fa_fwd_launch_varlen.  Refused before any HIP
 * call: what fa_fwd_launch_varlen refuses, and null cache_seqlens (FA_ERR_NULL); page_size % 64 != 0 (FA_ERR_NO_KERNEL);
 * struct_size, sizes that are not positive, block_table_stride < max_pages_per_seq, max_seqlen_k outside [0, capacity], a
 * contiguous cache whose kv_batch_stride is not positive with n_seqs > 1, lengths beyond 32 bits (FA_ERR_SHAPE); strides not
 * multiples of 8, cache_seqlens or block_table not 4-byte aligned (FA_ERR_ALIGN); a contiguous cache whose batch is not
 * n_seqs (FA_ERR_SHAPE: sequence b reads batch entry b).  total_q = 0 returns FA_OK without a launch.
 */
typedef struct fa_kvcache_layout {
    uint32_t struct_size;         /* sizeof(fa_kvcache_layout) */
    const int32_t *cache_seqlens;
    const int32_t *block_table;   /* null = contiguous cache */
    int64_t seqlen_cache;         /* contiguous cache: rows per batch entry (ignored when paged) */
    int64_t num_pages;            /* paged cache only, like the next three */
    int64_t page_size;
    int64_t max_pages_per_seq;
    int64_t block_table_stride;
    int64_t max_seqlen_k;         /* 0 = capacity */
    int64_t batch;                /* contiguous cache: its batch entries, which must be n_seqs (ignored when paged) */
} fa_kvcache_layout;
int fa_fwd_varlen_kvcache_supported(const fa_fwd_config *cfg, const fa_fwd_opts *opts);
int fa_fwd_launch_varlen_kvcache(const fa_fwd_args *args, const fa_kv_layout *kv, const fa_varlen_layout *varlen_q,
                                 const fa_kvcache_layout *cache, const fa_fwd_opts *opts, float *lse, void *stream);

/*
 * The same prefill against an fp8 K / V cache (the cache of fa_decode_fp8_launch and fa_kvcache_append_launch; enum fa_kv_dtype
 * below).  args->k, ->v hold OCP e4m3fn bytes in the two shapes above, one byte per element, so kv's strides count BYTES; q, o
 * and lse are fa_fwd_launch_varlen_kvcache's.  fa_kvcache_layout is unchanged; the fp8 side travels in fa_kvcache_fp8_scales:
 * struct_size = sizeof(fa_kvcache_fp8_scales), kv_dtype = FA_KV_FP8_E4M3FN (anything else is FA_ERR_DTYPE), and k_descale,
 * v_descale (either may be null, which means 1): fp32 DEVICE arrays (n_seqs, n_kv_heads), row stride descale_batch_stride
 * elements -- b is the SEQUENCE index for both cache shapes.  Key j of sequence b, K / V head h stands for
 * float(k8[j]) * k_descale[b][h], likewise V; the result is the 16-bit call's on those values (bit for bit when the descaled
 * values are exact in q's type and the descales are powers of two).  The host never reads the descales (like the lengths and the
 * table they may change between graph replays); they must be finite and positive, which is not checked, and no address
 * depends on them.  An e4m3 NaN in a valid row propagates; at or beyond len_k it is never fetched.
 * Grid, clamping, causal rule, empty rows, determinism: fa_fwd_launch_varlen_kvcache's.  One launch, no split, no workspace.
 * Refused before any HIP call: what fa_fwd_launch_varlen_kvcache refuses, and kv_dtype (FA_ERR_DTYPE); kv strides not
 * multiples of 16 bytes, k / v not 16-byte aligned, descale pointers not 4-byte aligned (FA_ERR_ALIGN); struct_size,
 * descale_batch_stride < n_kv_heads with a descale given (FA_ERR_SHAPE).  total_q = 0 returns FA_OK without a device.
 */
typedef struct fa_kvcache_fp8_scales {
    uint32_t struct_size;         /* sizeof(fa_kvcache_fp8_scales) */
    int32_t kv_dtype;             /* fa_kv_dtype: FA_KV_FP8_E4M3FN */
    const float *k_descale;       /* DEVICE (n_seqs, n_kv_heads) fp32; null = 1 */
    const float *v_descale;
    int64_t descale_batch_stride;
} fa_kvcache_fp8_scales;
int fa_fwd_varlen_kvcache_fp8_supported(const fa_fwd_config *cfg, const fa_fwd_opts *opts);
int fa_fwd_launch_varlen_kvcache_fp8(const fa_fwd_args *args, const fa_kv_layout *kv, const fa_varlen_layout *varlen_q,
                                     const fa_kvcache_layout *cache, const fa_kvcache_fp8_scales *scales, const fa_fwd_opts *opts,
                                     float *lse, void *stream);

/*
 * KV-cache decode attention (forward only): a few query rows per sequence against a long K / V cache whose valid length per
 * batch entry lies in DEVICE memory.  bf16 / fp16, d_head 128, MHA and GQA / MQA (query head h reads K / V head
 * h / (n_heads / n_kv_heads)), softmax scale 1 / sqrt(128).
 *
 * q, o: (batch, seqlen_q, n_heads, 128) with the q_* / o_* strides (elements).  k, v (one stride set, kv_*):
 *   contiguous cache (block_table null):  (batch, seqlen_cache, n_kv_heads, 128); kv_batch_stride is the batch stride;
 *   paged cache (block_table non-null):   (num_pages, page_size, n_kv_heads, 128); kv_batch_stride is the PAGE stride, and
 *     block_table is a DEVICE (batch, max_pages_per_seq) int32 array, row stride block_table_stride: key j of batch entry b
 *     is row j % page_size of page block_table[b][j / page_size].
 * cache_seqlens: DEVICE (batch) int32, the number of valid keys of each entry, the newest tokens (which the caller has already
 * written into the cache, with fa_kvcache_append_launch for one) included.  The host never reads it or block_table: launches are asynchronous and graph-capturable,
 * and every grid and split count is a function of the host-visible arguments alone.
 * causal: bottom-right aligned -- query row i sees keys j <= len - seqlen_q + i; else every row sees all len keys.  A row that
 * sees no key gives o = 0 and lse = -inf.  lse (may be null): fp32 (batch, n_heads, seqlen_q), natural log, contiguous.
 *
 * Clamping: len is clamped to [0, capacity], capacity = seqlen_cache (paged: max_pages_per_seq * page_size);
 * every block_table entry used is clamped to [0, num_pages), and only entries of pages below ceil(len / page_size) are read;
 * cache rows at or beyond len are never fetched (their lanes fetch row len - 1 and are masked), so neither their contents
 * nor unused pages nor unused block_table entries reach a result, and no address outside the tensors is formed.
 *
 * Served (fa_decode_supported = 1): seqlen_q * (n_heads / n_kv_heads) <= 64 packed rows and, paged, page_size % 64 == 0;
 * anything else is FA_ERR_NO_KERNEL.  max_seqlen_k: the host's bound on every length, 0 = capacity; it only steers the split rule.
 * num_splits: 0 = the rule -- the smallest power of two s with batch * n_kv_heads * s >= 256, at most ceil(max_seqlen_k / 256)
 * and at most 128 (fa_decode_num_splits) -- or a forced count in [1, 1024].  With more than one split the workspace
 * (fa_decode_workspace_bytes bytes of device memory, 16-byte aligned; 0 bytes for one split) holds fp32 partials that a second
 * kernel combines in split order: no atomics, the same bits for the same arguments.
 * Refused before any HIP call: null pointers (FA_ERR_NULL); dtype (FA_ERR_DTYPE); row count / page size (FA_ERR_NO_KERNEL);
 * struct_size, sizes, strides not positive (FA_ERR_SHAPE); strides not multiples of 8, tensors not 16-byte aligned, int32
 * arrays and lse not 4-byte aligned, workspace not 16-byte aligned (FA_ERR_ALIGN).  batch = 0 returns FA_OK without a device.
 */
typedef struct fa_decode_args {
    uint32_t struct_size;      /* sizeof(fa_decode_args) */
    int32_t dtype;             /* fa_dtype */
    int32_t causal;
    int32_t num_splits;        /* 0 = the rule */
    const void *q;
    const void *k;
    const void *v;
    void *o;
    float *lse;                /* may be null */
    const int32_t *cache_seqlens;
    const int32_t *block_table;   /* null = contiguous cache */
    void *workspace;           /* needed when fa_decode_workspace_bytes > 0 */
    int64_t batch;
    int64_t seqlen_q;
    int64_t n_heads;
    int64_t n_kv_heads;
    int64_t d_head;
    int64_t seqlen_cache;      /* contiguous cache: rows per batch entry (ignored when paged) */
    int64_t num_pages;         /* paged cache only, like the next three */
    int64_t page_size;
    int64_t max_pages_per_seq;
    int64_t block_table_stride;
    int64_t max_seqlen_k;      /* 0 = capacity */
    int64_t q_batch_stride;
    int64_t q_seq_stride;
    int64_t q_head_stride;
    int64_t o_batch_stride;
    int64_t o_seq_stride;
    int64_t o_head_stride;
    int64_t kv_batch_stride;   /* paged: the page stride */
    int64_t kv_seq_stride;
    int64_t kv_head_stride;
} fa_decode_args;
int fa_decode_supported(const fa_decode_args *args);
int fa_decode_num_splits(const fa_decode_args *args);                 /* the split count the launch uses, or a negative fa_status */
int64_t fa_decode_workspace_bytes(const fa_decode_args *args);        /* bytes, or a negative fa_status */
int fa_decode_launch(const fa_decode_args *args, void *stream, float *ms);

/*
 * The same decode against an fp8 K / V cache.  k and v hold OCP e4m3fn bytes (torch.float8_e4m3fn; not MI300's fnuz
 * encoding) in the shapes and addressings of fa_decode_args, one byte per element, so the kv_* strides count bytes; q and o
 * stay bf16 / fp16 (dtype).  kv_dtype names the cache's encoding: FA_KV_FP8_E4M3FN is the only value served, anything else
 * is FA_ERR_DTYPE.
 * k_descale, v_descale (either may be null, which means 1): fp32 DEVICE arrays (batch, n_kv_heads), row stride
 * descale_batch_stride elements.  Key j of entry b, K / V head h stands for float(k8[j]) * k_descale[b][h], likewise V; the
 * result is softmax(q k^T / sqrt(128)) v on those values, with lse from the same logits.  The host never reads the descales
 * (like cache_seqlens they may change between graph replays).  They must be finite and positive: the caller's contract, not
 * checked; whatever they hold, no address depends on them.  An e4m3 NaN (0x7f, 0xff) in a valid row propagates as a 16-bit
 * NaN does; at or beyond len it is never fetched.
 * Everything else -- causal, empty rows, the clamping, the split rule (the same function of the same arguments, the same
 * constants), the workspace size and format, the fixed-order combine, determinism -- is fa_decode_launch's.
 * Refused before any HIP call, as fa_decode_launch does, and additionally: kv_dtype (FA_ERR_DTYPE); kv_* strides not
 * multiples of 16 bytes, k / v not 16-byte aligned, descale pointers not 4-byte aligned (FA_ERR_ALIGN);
 * descale_batch_stride < n_kv_heads with a descale given (FA_ERR_SHAPE).
 */
typedef enum fa_kv_dtype {
    FA_KV_FP8_E4M3FN = 1
} fa_kv_dtype;

typedef struct fa_decode_fp8_args {
    uint32_t struct_size;      /* sizeof(fa_decode_fp8_args) */
    int32_t dtype;             /* fa_dtype of q and o */
    int32_t causal;
    int32_t num_splits;        /* 0 = the rule */
    const void *q;
    const void *k;             /* fp8 bytes */
    const void *v;
    void *o;
    float *lse;                /* may be null */
    const int32_t *cache_seqlens;
    const int32_t *block_table;   /* null = contiguous cache */
    void *workspace;           /* needed when fa_decode_fp8_workspace_bytes > 0 */
    int64_t batch;
    int64_t seqlen_q;
    int64_t n_heads;
    int64_t n_kv_heads;
    int64_t d_head;
    int64_t seqlen_cache;
    int64_t num_pages;
    int64_t page_size;
    int64_t max_pages_per_seq;
    int64_t block_table_stride;
    int64_t max_seqlen_k;      /* 0 = capacity */
    int64_t q_batch_stride;
    int64_t q_seq_stride;
    int64_t q_head_stride;
    int64_t o_batch_stride;
    int64_t o_seq_stride;
    int64_t o_head_stride;
    int64_t kv_batch_stride;   /* bytes = elements; paged: the page stride */
    int64_t kv_seq_stride;
    int64_t kv_head_stride;
    const float *k_descale;    /* DEVICE (batch, n_kv_heads) fp32, may be null (= 1) */
    const float *v_descale;
    int64_t descale_batch_stride;   /* elements; >= n_kv_heads when a descale is given */
    int32_t kv_dtype;          /* fa_kv_dtype */
} fa_decode_fp8_args;
int fa_decode_fp8_supported(const fa_decode_fp8_args *args);
int fa_decode_fp8_num_splits(const fa_decode_fp8_args *args);          /* the split count the launch uses, or a negative fa_status */
int64_t fa_decode_fp8_workspace_bytes(const fa_decode_fp8_args *args); /* bytes, or a negative fa_status */
int fa_decode_fp8_launch(const fa_decode_fp8_args *args, void *stream, float *ms);

/*
 * Sliding-window (local) attention for both decodes (flash-attn's window_size=(left, right)).  fa_window: struct_size =
 * sizeof(fa_window); left, right: how many keys a query row sees below and above its own position, -1 = unbounded.  With
 * p = len - seqlen_q + i the position of query row i (the bottom-right alignment of `causal`), the row sees key j iff
 *     max(0, p - left) <= j <= min(len - 1, p + right);
 * args->causal means right = 0 (causal with right > 0 is refused; right = -1 or 0 may accompany it).  A row that sees no key
 * gives o = 0 and lse = -inf.  (-1, -1) computes what the unwindowed entry point computes, and with a forced num_splits the
 * same bits.  Everything else -- shapes, strides, the cache's two addressings, the fp8 descales, the workspace format, the
 * fixed-order combine, determinism, graph capture -- is fa_decode_launch's and fa_decode_fp8_launch's.
 *
 * Clamping, extended downwards.  lo_min = max(0, len - seqlen_q - left) (0 for left = -1) is the lowest key any row of the
 * batch entry sees.  No key below lo_min is fetched, and no block_table entry of a page that lies wholly below lo_min is read;
 * a lane whose key would fall below lo_min fetches key lo_min and is masked, as a lane at or beyond len fetches len - 1.  So
 * stale rows, freed or reused pages and garbage table entries below the window cannot reach a result.  Keys from lo_min up
 * to a later row's own lower bound are valid keys of the entry and are fetched for all of its rows.
 *
 * The split rule (fa_decode_window_num_splits) is fa_decode_num_splits' with its key bound replaced by
 * min(max_seqlen_k or capacity, left + seqlen_q + right) when both sides are bounded (causal: right = 0), the old bound
 * otherwise: a window wider than the bound gives the unwindowed count.  The workspace follows the split count.
 * Refused before any HIP call: what the unwindowed entry point refuses; a null fa_window (FA_ERR_NULL); its struct_size, left or
 * right below -1, causal with right > 0, a capacity above 2^30 - 128 keys (FA_ERR_SHAPE).
 */
typedef struct fa_window {
    uint32_t struct_size;      /* sizeof(fa_window) */
    int32_t left;              /* -1 = unbounded */
    int32_t right;             /* -1 = unbounded */
} fa_window;
int fa_decode_window_supported(const fa_decode_args *args, const fa_window *window);
int fa_decode_window_num_splits(const fa_decode_args *args, const fa_window *window);          /* or a negative fa_status */
int64_t fa_decode_window_workspace_bytes(const fa_decode_args *args, const fa_window *window); /* bytes, or a negative fa_status */
int fa_decode_window_launch(const fa_decode_args *args, const fa_window *window, void *stream, float *ms);
int fa_decode_fp8_window_supported(const fa_decode_fp8_args *args, const fa_window *window);
int fa_decode_fp8_window_num_splits(const fa_decode_fp8_args *args, const fa_window *window);
int64_t fa_decode_fp8_window_workspace_bytes(const fa_decode_fp8_args *args, const fa_window *window);
int fa_decode_fp8_window_launch(const fa_decode_fp8_args *args, const fa_window *window, void *stream, float *ms);

/*
 * The same window for the step before decode: the packed forward with separate Q and K / V lengths and both prefills against a
 * cache.  Each entry takes its unwindowed sibling's arguments (fa_fwd_launch_varlen_qk, fa_fwd_launch_varlen_kvcache,
 * fa_fwd_launch_varlen_kvcache_fp8) and an fa_window in front of opts.  For sequence b, len_q and len_k are clamped as the
 * sibling clamps them; query row r sits at position p = r + (len_k - len_q) and sees key j iff
 *     max(0, p - left) <= j <= min(len_k - 1, p + right);
 * opts->causal means right = 0 (causal with right > 0 is refused; right = -1 or 0 may accompany it).  A row that sees no key
 * (p + right < 0) gives o = 0 and lse = -inf.  (-1, -1), or any window that reaches every key, gives the unwindowed entry's
 * bits; the three entries give one another's bits on the same keys, as their siblings do.  Grid, strides, descales, lse,
 * determinism, graph capture: the sibling's.  One launch, no split, no workspace.  The backward of the packed form is
 * fa_bwd_launch_varlen_qk_window (below); fa_bwd_launch_varlen and fa_bwd_launch_varlen_qk take no window, and the o and lse of
 * a windowed forward are not theirs.
 *
 * Clamping, extended downwards.  A workgroup owns 128 query rows r0 .. r1 of one (sequence, head) and visits only the 64-key
 * tiles from its last row's upper bound down to its first row's lower bound lo_r0 = max(0, r0 + len_k - len_q - left), which
 * is at least the sequence's lo_b = max(0, len_k - len_q - left) (0 for left = -1).  No key below lo_r0 is fetched, and no
 * block_table entry of a page that lies wholly below it is read; a lane whose key would fall below lo_r0 fetches key lo_r0
 * (the same tile, the same page) and is masked, as a lane at or beyond len_k fetches len_k - 1.  So stale rows, freed or
 * reused pages and garbage table entries below lo_b cannot reach a result, nor can packed key rows of the sequence below it.
 *
 * Served (fa_fwd_varlen_*_window_supported): what the sibling serves.  Refused before any HIP call: what the sibling refuses,
 * first and with its message; then a null fa_window (FA_ERR_NULL); its struct_size, left or right below -1, causal with right >
 * 0, and a key bound (the cache's capacity; packed: the key side's max_seqlen) or the query side's max_seqlen above
 * 2^30 - 128 (FA_ERR_SHAPE: the kernel adds positions and distances in 32 bits).  total_q = 0 returns FA_OK without a device.
 */
int fa_fwd_varlen_qk_window_supported(const fa_fwd_config *cfg, const fa_fwd_opts *opts);
int fa_fwd_launch_varlen_qk_window(const fa_fwd_args *args, const fa_kv_layout *kv, const fa_varlen_layout *varlen_q,
                                   const fa_varlen_layout *varlen_k, const fa_window *window, const fa_fwd_opts *opts, float *lse,
                                   void *stream);
int fa_fwd_varlen_kvcache_window_supported(const fa_fwd_config *cfg, const fa_fwd_opts *opts);
int fa_fwd_launch_varlen_kvcache_window(const fa_fwd_args *args, const fa_kv_layout *kv, const fa_varlen_layout *varlen_q,
                                        const fa_kvcache_layout *cache, const fa_window *window, const fa_fwd_opts *opts, float *lse,
                                        void *stream);
int fa_fwd_varlen_kvcache_fp8_window_supported(const fa_fwd_config *cfg, const fa_fwd_opts *opts);
int fa_fwd_launch_varlen_kvcache_fp8_window(const fa_fwd_args *args, const fa_kv_layout *kv, const fa_varlen_layout *varlen_q,
                                            const fa_kvcache_layout *cache, const fa_kvcache_fp8_scales *scales,
                                            const fa_window *window, const fa_fwd_opts *opts, float *lse, void *stream);

/*
 * The backward of fa_fwd_launch_varlen_qk_window: dQ, dK, dV from the windowed forward's o and lse under the same rule (the
 * arguments of fa_bwd_launch_varlen_qk and the forward's fa_window; args->causal means right = 0).  Kernels of their own (the
 * windowed form of fa_bwd_launch_varlen_qk's): a dQ workgroup, owning rows r0 .. r1 = min(r0 + 127, len_q - 1), visits the 64-key
 * tiles from max(0, r0 + shift - left) / 64 to min(len_k - 1, r1 + shift + right) / 64, shift = len_k - len_q; a dK / dV
 * workgroup, owning keys k0 .. k1 = min(k0 + 127, len_k - 1), sweeps the 64-row Q tiles from max(0, k0 - shift - right) / 64 to
 * min(len_q - 1, k1 - shift + left) / 64; an empty range sweeps nothing and stores zeros.  A row that sees no key
 * (lse = -inf) gets dq = 0; a key no row sees -- below every row's floor, above every row's ceiling, or len_q = 0 -- gets
 * dk = dv = 0, written.  Grids, the dK / dV split, the workspace and its layout are fa_bwd_launch_varlen_qk's:
 * fa_bwd_varlen_qk_workspace_bytes(args) sizes this call too.  Deterministic, no atomics, graph-capturable.  A window that reaches
 * every key gives fa_bwd_launch_varlen_qk's gradients within rounding, not its bits in the plain form.
 *
 * Refused before any HIP call: what fa_bwd_launch_varlen_qk refuses, first and with its message; then a null fa_window
 * (FA_ERR_NULL); its struct_size, left or right below -1, causal with right > 0, and max_seqlen of either side above
 * 2^30 - 128 (FA_ERR_SHAPE).  total_q = total_k = 0 returns FA_OK without a device.
 */
int fa_bwd_launch_varlen_qk_window(const fa_bwd_varlen_qk_args *args, const fa_window *window, void *stream, float *ms);

/*
 * Logit soft-capping on the packed training path (flash-attn's softcap=).  With s = q . k / sqrt(128), the logit
 * of a key a row sees is softcap * tanh(s / softcap); a key the row does not see (mask, window, beyond the lengths) stays -inf --
 * the cap is applied before any mask.  lse is the log-sum-exp of the capped logits (natural units), o = softmax(capped) v; a row
 * that sees no key still gives o = 0, lse = -inf, dq = 0, and a key no row sees dk = dv = 0, written.  The backward, with
 * t = tanh(s / softcap): dS = P (dP - delta) (1 - t^2), dQ = dS K / sqrt(128), dK = dS^T Q / sqrt(128), dV = P^T dO; delta is
 * unchanged.  fa_softcap: struct_size = sizeof(fa_softcap); softcap finite and > 0.  This level has no "off": without a cap, call
 * fa_fwd_launch_varlen_qk_window / fa_bwd_launch_varlen_qk_window (or their unwindowed siblings).
 *
 * Both launches take the arguments of their windowed sibling, a window included: (-1, -1) is legal there and means none (a caller
 * with one range passes its layout on both sides).  Kernels of their own (the windowed text plus the cap; the sibling's tile
 * ranges, grids, dK / dV split and workspace: fa_bwd_varlen_qk_workspace_bytes(args) sizes the backward).  tanh is
 * 1 - 2 / (exp2(2 x log2 e) + 1) on the hardware's exp2 and reciprocal: absolute error a few 1e-7, times softcap on the logit;
 * it saturates to +-1 without a NaN.  Deterministic, no atomics, graph-capturable.
 *
 * Refused before any HIP call, in this order: what the windowed sibling refuses, with its status and message; then a null
 * fa_softcap (FA_ERR_NULL); then its struct_size, or a softcap that is NaN, infinite or <= 0 (FA_ERR_SHAPE).
 */
typedef struct fa_softcap {
    uint32_t struct_size;      /* sizeof(fa_softcap) */
    float softcap;             /* > 0, finite */
} fa_softcap;
int fa_fwd_varlen_qk_softcap_supported(const fa_fwd_config *cfg, const fa_fwd_opts *opts);
int fa_fwd_launch_varlen_qk_softcap(const fa_fwd_args *args, const fa_kv_layout *kv, const fa_varlen_layout *varlen_q,
                                    const fa_varlen_layout *varlen_k, const fa_window *window, const fa_softcap *softcap,
                                    const fa_fwd_opts *opts, float *lse, void *stream);
int fa_bwd_launch_varlen_qk_softcap(const fa_bwd_varlen_qk_args *args, const fa_window *window, const fa_softcap *softcap,
                                    void *stream, float *ms);

/*
 * Learned attention sinks on the packed training path (gpt-oss's `sinks`, flash-attn's learnable_sink / s_aux).
 * Query head h carries one more logit z = sinks[h] that joins the softmax's denominator and has no value vector (per QUERY head,
 * under grouped-query attention too).  With s_j = q . k_j / sqrt(128) over the keys a row sees (lengths, bottom-right causal rule
 * and window exactly as in fa_fwd_launch_varlen_qk_window):
 *     lse = log(exp(z) + sum_j exp(s_j))   (natural units),      o = sum_j exp(s_j - lse) v_j.
 * A row that sees no key gives o = 0 and lse = z (not -inf: the sink is the softmax's only member), dq = 0, and adds exactly 0 to
 * dsinks; a key no row sees gets dk = dv = 0, written.  z = -inf means "no sink for this head": o and lse are those of the call
 * without sinks (a dead row's lse = -inf), dsinks[h] = 0, no NaN anywhere.  z = +inf and NaN are unspecified; the host never reads
 * sinks.  The sink cannot overflow: it is folded in against max(row max, z), so z far above every logit gives lse = z, o -> 0, and
 * z far below changes nothing.  Not combined with soft-capping: these calls take no fa_softcap.
 *
 * The backward: dQ, dK, dV are what fa_bwd_launch_varlen_qk_window computes from this lse (its kernels, unchanged: P = exp(S - lse)
 * then sums to less than 1 per row, delta is unchanged), and
 *     dsinks[h] = - sum over the rows of head h of exp(z - lse[h][row]) * delta[h][row]
 * is written to `dsinks`, n_heads fp32 on the device (fp32 sums in a fixed order, no atomics: the same inputs give the same bits).
 * Both launches take the arguments of their windowed sibling, a window included: (-1, -1) is legal there and means none.
 * fa_bwd_varlen_qk_sinks_workspace_bytes(args) sizes the backward's workspace (the sibling's value).  Graph-capturable.  This level
 * has no "off": without sinks, call the windowed entry points (or their unwindowed siblings).
 *
 * Refused before any HIP call, in this order: what the windowed sibling refuses, with its status and message; then a null fa_sinks
 * or fa_sinks.sinks, and in the backward a null dsinks (FA_ERR_NULL); then a struct_size below sizeof(fa_sinks), or n_heads that is
 * not the call's (FA_ERR_SHAPE).  total_q = total_k = 0 returns FA_OK without a device, like the sibling, and writes nothing: the
 * sum over no rows, dsinks = 0, is then the caller's to write.
 */
typedef struct fa_sinks {
    uint32_t struct_size;      /* sizeof(fa_sinks) */
    int32_t n_heads;           /* the call's n_heads: one logit per query head */
    const float *sinks;        /* (n_heads) fp32, DEVICE */
} fa_sinks;
int fa_fwd_varlen_qk_sinks_supported(const fa_fwd_config *cfg, const fa_fwd_opts *opts);
int fa_fwd_launch_varlen_qk_sinks(const fa_fwd_args *args, const fa_kv_layout *kv, const fa_varlen_layout *varlen_q,
                                  const fa_varlen_layout *varlen_k, const fa_window *window, const fa_sinks *sinks,
                                  const fa_fwd_opts *opts, float *lse, void *stream);
int64_t fa_bwd_varlen_qk_sinks_workspace_bytes(const fa_bwd_varlen_qk_args *args);
int fa_bwd_launch_varlen_qk_sinks(const fa_bwd_varlen_qk_args *args, const fa_window *window, const fa_sinks *sinks, float *dsinks,
                                  void *stream, float *ms);

/*
 * Logit soft-capping on the inference path: the cache prefill and the decode, 16-bit and fp8 cache.  The same
 * definition as above: the logit of a key a row sees is softcap * tanh(s / softcap), s = q . k / sqrt(128) on the DEQUANTIZED key,
 * applied before any mask; lse is the log-sum-exp of the capped logits, a row that sees no key gives o = 0, lse = -inf.
 *
 * Every entry takes the arguments of its windowed sibling (fa_fwd_launch_varlen_kvcache_window, .._fp8_window, fa_decode_window_*,
 * fa_decode_fp8_window_*), a window included -- (-1, -1) is legal there and means none -- and an fa_softcap behind it.  Kernels of
 * their own (the windowed text plus the cap): the sibling's fetch contract, tile ranges, grids and partial format.  An fp8 cache's
 * k_descale goes into the tanh's argument (a tanh between the raw product and the exponent forbids folding it into the exponent's
 * constant); v_descale stays in the final 1 / l.  The decode's split count and workspace are the windowed entry's for the same
 * arguments: the cap does not enter the rule.  The capped decodes therefore have no workspace query of their own:
 * fa_decode_window_workspace_bytes(args, window) / fa_decode_fp8_window_workspace_bytes(args, window) size the launch.
 * Deterministic, no atomics, graph-capturable.
 *
 * Refused before any HIP call, in this order: what the windowed sibling refuses, with its status and message; then a null
 * fa_softcap (FA_ERR_NULL); then its struct_size, or a softcap that is NaN, infinite or <= 0 (FA_ERR_SHAPE).  This level has no
 * "off": without a cap, call the windowed sibling.
 */
int fa_fwd_varlen_kvcache_softcap_supported(const fa_fwd_config *cfg, const fa_fwd_opts *opts);
int fa_fwd_launch_varlen_kvcache_softcap(const fa_fwd_args *args, const fa_kv_layout *kv, const fa_varlen_layout *varlen_q,
                                         const fa_kvcache_layout *cache, const fa_window *window, const fa_softcap *softcap,
                                         const fa_fwd_opts *opts, float *lse, void *stream);
int fa_fwd_varlen_kvcache_fp8_softcap_supported(const fa_fwd_config *cfg, const fa_fwd_opts *opts);
int fa_fwd_launch_varlen_kvcache_fp8_softcap(const fa_fwd_args *args, const fa_kv_layout *kv, const fa_varlen_layout *varlen_q,
                                             const fa_kvcache_layout *cache, const fa_kvcache_fp8_scales *scales, const fa_window *window,
                                             const fa_softcap *softcap, const fa_fwd_opts *opts, float *lse, void *stream);
int fa_decode_softcap_supported(const fa_decode_args *args, const fa_window *window, const fa_softcap *softcap);
int fa_decode_softcap_num_splits(const fa_decode_args *args, const fa_window *window, const fa_softcap *softcap);
int fa_decode_softcap_launch(const fa_decode_args *args, const fa_window *window, const fa_softcap *softcap, void *stream, float *ms);
int fa_decode_fp8_softcap_supported(const fa_decode_fp8_args *args, const fa_window *window, const fa_softcap *softcap);
int fa_decode_fp8_softcap_num_splits(const fa_decode_fp8_args *args, const fa_window *window, const fa_softcap *softcap);
int fa_decode_fp8_softcap_launch(const fa_decode_fp8_args *args, const fa_window *window, const fa_softcap *softcap, void *stream,
                                 float *ms);

/*
 * The step in front of a decode: append seqlen_new new K / V rows per batch entry to the cache IN PLACE, at the positions the
 * device-side lengths name, optionally rotate the new keys and the query (rotary embedding), quantize for an fp8 cache, and
 * advance the lengths.  One kernel on `stream`; the host reads none of the device arrays, so the launch is asynchronous and
 * graph-capturable, and fa_decode_launch / fa_decode_fp8_launch behind it on the same stream sees the appended cache.
 *
 * Per batch entry b, len = clamp(cache_seqlens[b], 0, capacity) (capacity as in fa_decode_args):
 *  - k_new, v_new (batch, seqlen_new, n_kv_heads, 128), dtype, one stride set (new_*): row t goes to cache position len + t,
 *    addressed as fa_decode_args addresses the cache (contiguous, or paged through block_table with every entry used clamped to
 *    [0, num_pages)); a token whose position is >= capacity is dropped.  kv_dtype 0: the cache has q's dtype and the kv_*
 *    strides count its elements; FA_KV_FP8_E4M3FN: e4m3fn bytes, strides in bytes, and the row is stored as
 *    e4m3fn(clamp(x / descale[b][h], -448, 448)) -- IEEE fp32 division, round to nearest even, NaN stays NaN (0x7f / 0xff): the
 *    bytes of torch's (x.float() / descale).clamp(-448, 448).to(torch.float8_e4m3fn).  k_descale / v_descale as in
 *    fa_decode_fp8_args (null = 1); they belong to an fp8 cache only.
 *  - rotary_cos, rotary_sin (both or neither): (seqlen_ro, rotary_dim / 2) tables of dtype, row stride rotary_seq_stride;
 *    rotary_dim a multiple of 16 in [16, 128], elements at or beyond it pass through.  rotary_interleaved 0 pairs element i with
 *    i + rotary_dim / 2, 1 pairs 2 i with 2 i + 1; o1 = x1 c - x2 s, o2 = x1 s + x2 c in fp32 with unfused multiplies and adds,
 *    rounded once to dtype (the bits of the same expression in eager torch).  The key at position p uses table row
 *    min(p, seqlen_ro - 1).  V is never rotated; without tables K is copied bit for bit.
 *  - q (batch, seqlen_q, n_heads, 128), with tables only, is rotated into q_out (same shape, its own strides; must not overlap
 *    q): row i uses position len + i with causal, else len (flash-attn's rule).  q may be null (keys only).
 *  - seqlens_out[b] = min(len + seqlen_new, capacity).  seqlens_out may be cache_seqlens itself (in-place advance): entry b is
 *    read and written by one workgroup, the store behind a barrier.
 * Two batch entries that map to one page are the caller's contract violation: the result there is undefined, the addresses
 * stay in range.  seqlen_new = 0 is served (a given q is rotated, the lengths are copied); k_new / v_new may then be null.
 * Refused before any HIP call: null pointers, q without q_out (FA_ERR_NULL); dtype, kv_dtype (FA_ERR_DTYPE); page_size % 64 != 0
 * (FA_ERR_NO_KERNEL); struct_size, sizes, strides not positive, rotary_dim not a multiple of 16 in [16, 128], one table
 * without the other, q without tables, q_out overlapping q, descales with a 16-bit cache (FA_ERR_SHAPE);
 * strides not multiples of 16 bytes, tensors and tables not 16-byte aligned, int32 / fp32 arrays not 4-byte aligned
 * (FA_ERR_ALIGN).  batch = 0 returns FA_OK without a device.
 */
typedef struct fa_kvcache_append_args {
    uint32_t struct_size;      /* sizeof(fa_kvcache_append_args) */
    int32_t dtype;             /* fa_dtype of k_new, v_new, q, q_out and the tables */
    int32_t kv_dtype;          /* 0 = the cache has dtype; or fa_kv_dtype */
    int32_t causal;            /* only the position rule of q */
    int32_t rotary_interleaved;
    const void *k_new;
    const void *v_new;
    void *k;                   /* the cache, written in place */
    void *v;
    const void *q;             /* may be null */
    void *q_out;
    const void *rotary_cos;    /* both null = no rotary */
    const void *rotary_sin;
    const int32_t *cache_seqlens;
    int32_t *seqlens_out;      /* may be cache_seqlens */
    const int32_t *block_table;   /* null = contiguous cache */
    const float *k_descale;    /* fp8 cache only; DEVICE (batch, n_kv_heads) fp32, may be null (= 1) */
    const float *v_descale;
    int64_t batch;
    int64_t seqlen_new;
    int64_t seqlen_q;          /* ignored without q */
    int64_t n_heads;           /* ignored without q */
    int64_t n_kv_heads;
    int64_t d_head;
    int64_t seqlen_cache;      /* contiguous cache: rows per batch entry (ignored when paged) */
    int64_t num_pages;         /* paged cache only, like the next three */
    int64_t page_size;
    int64_t max_pages_per_seq;
    int64_t block_table_stride;
    int64_t rotary_dim;        /* with tables only */
    int64_t seqlen_ro;
    int64_t rotary_seq_stride;
    int64_t new_batch_stride;
    int64_t new_seq_stride;
    int64_t new_head_stride;
    int64_t q_batch_stride;
    int64_t q_seq_stride;
    int64_t q_head_stride;
    int64_t qo_batch_stride;   /* q_out's */
    int64_t qo_seq_stride;
    int64_t qo_head_stride;
    int64_t kv_batch_stride;   /* elements of the cache's type; paged: the page stride */
    int64_t kv_seq_stride;
    int64_t kv_head_stride;
    int64_t descale_batch_stride;   /* elements; >= n_kv_heads when a descale is given */
} fa_kvcache_append_args;
int fa_kvcache_append_launch(const fa_kvcache_append_args *args, void *stream, float *ms);

/* The adaptive speculative mode's record on `device` (fa_speculative_mode), and a reset of its demotion state (tests,
 * or a caller that knows its data has changed character). */
int fa_adaptive_state(int device, fa_adaptive_info *out);
/* ... of the ONE device variant that serves cfg with these options when it runs speculatively (opts may be NULL; its
 * `speculative` field is ignored).  FA_ERR_NO_KERNEL if cfg has no speculative variant. */
int fa_adaptive_state_for(int device, const fa_fwd_config *cfg, const fa_fwd_opts *opts, fa_adaptive_info *out);
int fa_adaptive_reset(int device);
/* The policy alone, on a fresh state and without a device (tests): launch i sees report_word[i] in the pinned word and
 * probe_state[i] for its outstanding probe (-1 none, 0 pending, 1 complete, 2 error); run[i] = 0 speculative, 1 the
 * non-speculative sibling, 2 the probe (speculative, an event recorded behind it). */
int fa_adaptive_simulate(int n, const uint32_t *report_word, const int32_t *probe_state, int32_t *run, fa_adaptive_info *final_state);

/* Registry enumeration: distinct device variants built into this library.  fa_get_kernel / fa_fwd_query write
 * sizeof(fa_kernel_info) bytes of THIS library's header; fa_kernel_info has grown (0.2 -> 0.3: softmax_mode,
 * prescaled_q), so a client that may run against a newer library than the header it was compiled with calls the _sized
 * forms, which write at most out_size bytes (whole leading fields; the struct only ever grows at its end), or checks
 * fa_abi_version() first.  ABI history: INTEGRATION.md 6. */
int fa_num_kernels(void);
int fa_get_kernel(int index, fa_kernel_info *out);
int fa_get_kernel_sized(int index, fa_kernel_info *out, uint32_t out_size);
int fa_fwd_query_sized(const fa_fwd_config *cfg, const fa_fwd_opts *opts, fa_kernel_info *out, uint32_t out_size);

/* Increases whenever a struct of this header grows or an entry point changes meaning (6 = this header: fa_kernel_info grew
 * by ring_lds_bytes, persistent, alt_form and ring_threads; the speculative first pass of the persistent kernel walks K / V first-to-last; 5: the
 * adaptive record per device variant, fa_adaptive_state_for, the four ring_* fields). */
#define FA_ABI_VERSION 6
int fa_abi_version(void);

/* Message for the last non-zero status on this thread ("" if none). */
const char *fa_last_error(void);

/* Library version string, e.g. "fa_hip 0.4 gfx950". */
const char *fa_version(void);

#ifdef __cplusplus
}
#endif
#endif /* FA_HIP_H */
