// fa_capi.hip -- C ABI of libfa_hip.so (declared in include/fa_hip.h).
//
// Host-side launcher for the gfx950 forward kernel: the work
// /root/reference/src/flash_attention.cu:58-134 does after its torch checks
// (config -> kernel lookup, shape checks, grid/block/LDS, optional event timing),
// with no torch types.  Tensor-level checks (device, contiguity, dtype equality,
// output allocation, current stream) stay in the Python shim
// flash_attention_from_scratch_amd/flash_attention_kernels.py.
#include <hip/hip_runtime.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <atomic>
#include <cmath>
#include <mutex>
#include <vector>

#include "../../include/fa_hip.h"
#include "fa_bwd_gqa.hpp"
#include "fa_bwd_varlen.hpp"
#include "fa_decode_kernel.hpp"
#include "fa_kvcache_append_kernel.hpp"
#include "fa_registry.hpp"

extern "C" {
fa::KernelTable fa_inst_table_dt15_qt1();
fa::KernelTable fa_inst_table_dt15_qt2();
fa::KernelTable fa_inst_table_dt5_qt1();
fa::KernelTable fa_inst_table_dt5_qt2();
fa::KernelTable fa_inst16_table_dt15();
fa::KernelTable fa_inst16_table_dt5();
}
namespace fa {
// fa_inst_lse.hip: the persistent kernel's forms that also write the row log-sum-exp (fa_fwd_kernel64_lse)
kernel_fn_lse lse_kernel_dt15(bool masked, bool spec);
kernel_fn_lse lse_kernel_dt5(bool masked, bool spec);
// fa_inst_gqa.hip: their grouped-query attention forms (fa_fwd_kernel64_gqa)
kernel_fn_gqa gqa_kernel_dt15(bool masked, bool spec);
kernel_fn_gqa gqa_kernel_dt5(bool masked, bool spec);
// fa_bwd.hip: delta, dK / dV and dQ of one backward, enqueued on `s`
hipError_t bwd_enqueue(const BwdArgs &a, int dtype, bool causal, hipStream_t s);
hipError_t bwd_gqa_enqueue(const BwdGqaArgs &g, int dtype, bool causal, hipStream_t s);
// fa_inst_varlen.hip: the packed variable-length forward, one slice per form and dtype.  The forms, X(key side, extra, suffix):
// key side 0 packed keys (equal or separate Q and K / V lengths) | 1 a KV cache | 2 an fp8 (e4m3fn) KV cache; extra 0 nothing |
// 1 a sliding window | 2 a sliding window and logit soft-capping | 3 a sliding window and attention sinks (packed keys only).  A new form is one entry here (and one in csrc/Makefile's
// VARLEN_FORMS, and its arm in fa_fwd_kernel.hpp).
#define FA_VARLEN_FORMS(X)                                                       \
    X(0, 0, )             X(0, 1, _window)             X(0, 2, _softcap)         X(0, 3, _sinks) \
    X(1, 0, _kvcache)     X(1, 1, _kvcache_window)     X(1, 2, _kvcache_softcap) \
    X(2, 0, _kvcache_fp8) X(2, 1, _kvcache_fp8_window) X(2, 2, _kvcache_fp8_softcap)
#define FA_X(KEYS, EXTRA, SFX)                                              \
    kernel_fn_varlen##SFX varlen##SFX##_kernel_dt15(bool first_block_skip); \
    kernel_fn_varlen##SFX varlen##SFX##_kernel_dt5(bool first_block_skip);
FA_VARLEN_FORMS(FA_X)
#undef FA_X
int varlen_lds_bytes_dt15();   // (every form's LDS)
// fa_bwd_varlen.hip / fa_bwd_varlen_qk.hip: the packed backward, and its form with separate Q and K / V lengths
hipError_t bwd_varlen_enqueue(const BwdVarlenArgs &a, int dtype, bool causal, hipStream_t s);
hipError_t bwd_varlen_qk_enqueue(const BwdVarlenQKArgs &a, int dtype, bool causal, hipStream_t s);
// fa_bwd_varlen_window.hip: ... under a sliding window (causal arrives as right = 0)
hipError_t bwd_varlen_window_enqueue(const BwdVarlenWindowArgs &a, int dtype, hipStream_t s);
// fa_bwd_varlen_softcap.hip: ... with logit soft-capping on top
hipError_t bwd_varlen_softcap_enqueue(const BwdVarlenSoftcapArgs &a, int dtype, hipStream_t s);
// fa_bwd_varlen_sinks.hip: the window form's backward from an lse that includes the sinks, then the sinks' own gradient
hipError_t bwd_varlen_sinks_enqueue(const BwdVarlenSinksArgs &a, int dtype, hipStream_t s);
}  // namespace fa

namespace {

thread_local char g_err[512] = "";

__attribute__((cold)) int fail(int code, const char *fmt, ...) {   // (cold: the rules around a refusal stay small enough to inline)
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return code;
}

std::vector<fa::KernelEntry> &registry() {
    static std::vector<fa::KernelEntry> all = [] {
        std::vector<fa::KernelEntry> v;
        const fa::KernelTable tables[] = {
            fa_inst_table_dt15_qt1(), fa_inst_table_dt15_qt2(), fa_inst_table_dt5_qt1(),
            fa_inst_table_dt5_qt2(),  fa_inst16_table_dt15(),   fa_inst16_table_dt5(),
        };
        for (const auto &t : tables)
            for (int i = 0; i < t.count; ++i) v.push_back(t.entries[i]);
        return v;
    }();
    return all;
}

bool valid_load_tiles(int v) { return v == 0 || v == 2 || v == 4 || v == 8; }

// Config -> device variant.  The operand-fetch hints (load_K_tiles, double
// buffer) are validated with the reference's rules
// (static_kernel_configuration.cuh:13-35) and then ignored: on CDNA4 the
// compiler schedules LDS->MFMA operand reads and all hint values share one variant.
// cfg.optimized_softmax keeps the reference's meaning (the first KV block skips the rescale): it selects the
// variant built that way where one exists (softmax_mode 1) and is ignored where the schedule has no first-block
// rescale to skip (the result is the same either way).  The speculative softmax and the pre-scaled Q are this
// library's extensions and are asked for explicitly (fa_fwd_opts).
struct Want {
    bool masked = false;       // the causal / ragged-length variant of the configuration
    bool ragged = false;       // ... and seq_len may be off the tile sizes (fa_fwd_opts.allow_ragged)
    bool speculative = false;
    bool prescaled_q = false;
};
const fa::KernelEntry *find_kernel(const fa_fwd_config *c, const char **why, const Want &w = Want()) {
    static const char *kNotFound = "Kernel configuration was not found in the libfa_hip.so registry";
    *why = kNotFound;
    if (c->d_head != 128 && c->d_head != 64) { *why = "Only d_head = 128 (and 64) is supported"; return nullptr; }
    if (c->n_warps <= 0 || c->B_r <= 0 || c->B_r % c->n_warps != 0) return nullptr;
    if (!valid_load_tiles(c->Q_mma_load_K_tiles) || !valid_load_tiles(c->K_mma_load_K_tiles) ||
        !valid_load_tiles(c->V_mma_load_K_tiles))
        return nullptr;
    if (c->Q_mma_load_K_tiles != 0 && c->Q_mma_load_K_tiles != c->K_mma_load_K_tiles)
        return nullptr;
    const int rows_per_wave = c->B_r / c->n_warps;
    // mma_double_buffer_loads selects the software-pipelined loop where one is built;
    // otherwise it is a hint like the load_K_tiles fields and the plain loop is used.
    // Preference among the variants of one shape: the pipelined flag as asked, then the softmax mode --
    // speculative if (and only if) asked for; else the first-block-skip build for optimized_softmax where it
    // exists; else the eager / lazy build.
    const fa::KernelEntry *best = nullptr;
    int best_score = -1;
    for (const auto &e : registry()) {
        if (!(e.d_head == c->d_head && e.dtype == c->dtype && e.rows_per_wave == rows_per_wave &&
              e.n_waves == c->n_warps && e.B_c == c->B_c && e.swizzled == (c->swizzled != 0) &&
              e.eager == (c->eager_load_blocks != 0) && e.async_copy == (c->async_copy != 0) &&
              (e.masked != 0) == w.masked && (e.prescaled_q != 0) == w.prescaled_q))
            continue;
        if ((e.softmax_mode == FA_SOFTMAX_SPECULATIVE) != w.speculative) continue;
        const bool pipe_match = e.pipelined == (c->mma_double_buffer_loads != 0);
        if (!pipe_match && e.pipelined) continue;  // the plain loop stands in for a pipelined one that is not built, never the reverse
        const bool fbs = e.softmax_mode == FA_SOFTMAX_FIRST_BLOCK_SKIP;
        if (fbs && !c->optimized_softmax) continue;
        const int score = (pipe_match ? 2 : 0) + (fbs ? 1 : 0);
        if (score > best_score) { best = &e; best_score = score; }
    }
    if (!best && (w.speculative || w.prescaled_q))
        *why = "Kernel configuration has no device variant with the requested options (speculative softmax / pre-scaled Q) "
               "in the libfa_hip.so registry";
    return best;
}

// One-time setup PER DEVICE (the reference's device guard + module init, src/flash_attention.cu:42,142-149):
// the arch check, the CU count that caps the persistent grid and the > 48 KB dynamic-LDS opt-in of every
// kernel function all belong to the device that is current at the call, so a process that drives several
// GPUs gets each of them initialised at its first launch there, and a failure on one device (not a gfx950)
// does not stick to the others.
// Adaptive speculative softmax (fa_fwd_opts.speculative == FA_SPECULATIVE_ADAPTIVE).  A speculative launch whose
// first pass fails some item computes that item twice, and a launch ends with its slowest workgroup: ONE failing item
// costs a whole item time, everything failing 2x.  The kernels report such a launch by storing its
// sequence number into one word of pinned host memory (KernelArgs::redo_flag; a launch without failures writes
// nothing).  The library reads that word -- a plain host read, it never waits for the device -- whenever an adaptive
// launch is enqueued:
//   NORMAL    every launch speculative.  A new report -> DEMOTED for `hold` launches (this one included).
//   DEMOTED   the non-speculative sibling of the configuration serves the launch; when the hold has run out the next
//             launch is a PROBE: speculative again, with an event recorded behind it.
//   PROBING   launches are demoted until the probe's event has completed (hipEventQuery: no wait); then either the probe
//             reported too -> DEMOTED with `hold` doubled (32 ... 4096), or it did not -> NORMAL, `hold` back to 32.
// So steady bad data costs one speculative launch per hold; the host running ahead of the device costs at most the
// launches enqueued before the first report lands.  Both variants give a valid result (they differ in the rounding point
// of P); which one served a given launch depends on when a report arrived, so bit-reproducible callers ask for
// speculative = 0 or 1 instead.  During a stream capture the mode behaves like ALWAYS (no event is recorded into a graph).
// The policy itself is plain arithmetic over (the report word as read now, what the probe's event says): kept apart from
// HIP so that the CPU tier can script it (fa_adaptive_simulate; tests/test_host_cpu.py).
struct AdaptivePolicy {
    enum { NORMAL = 0, DEMOTED = 1, PROBING = 2 };
    enum { PROBE_NA = -1, PROBE_PENDING = 0, PROBE_COMPLETE = 1, PROBE_ERROR = 2 };
    enum { RUN_SPECULATIVE = 0, RUN_DEMOTED = 1, RUN_PROBE = 2 };
    uint32_t seq = 0;        // adaptive launches enqueued on this device so far
    uint32_t seen = 0;       // the last report acted on
    uint32_t mode = NORMAL;
    uint32_t remaining = 0;  // DEMOTED: launches of the hold still to come
    uint32_t probe_seq = 0;
    uint32_t hold = 32;
    uint32_t demoted = 0;    // adaptive launches that took the non-speculative variant
    uint32_t reports = 0;    // distinct failure reports acted on

    // One adaptive launch.  `rep`: the report word, read AFTER the probe's event was queried (a probe that has completed
    // has its report in memory by then); `probe`: PROBE_* (only looked at while PROBING).
    int step(uint32_t rep, int probe) {
        ++seq;
        const bool fresh = rep != seen;   // a speculative launch that has completed since computed items twice
        if (fresh) { seen = rep; ++reports; }
        if (mode == PROBING) {
            if (fresh) {                            // the probe (or a straggler from before the hold) failed: a longer hold
                if (hold < 4096) hold *= 2;
                mode = DEMOTED;
                remaining = hold;
            } else if (probe == PROBE_COMPLETE) {   // the probe ran clean
                mode = NORMAL;
                hold = 32;
            } else if (probe == PROBE_ERROR) {
                mode = NORMAL;
            }
        } else if (fresh) {                         // NORMAL or DEMOTED: (another) failure reported
            mode = DEMOTED;
            remaining = hold;
        }
        if (mode == DEMOTED) {
            if (remaining > 0) { --remaining; ++demoted; return RUN_DEMOTED; }
            mode = PROBING;                         // the hold has run out: this launch is the probe
            probe_seq = seq;
            return RUN_PROBE;
        }
        if (mode == PROBING) { ++demoted; return RUN_DEMOTED; }
        return RUN_SPECULATIVE;
    }
    void reset(uint32_t rep_now) { seen = rep_now; mode = NORMAL; remaining = 0; hold = 32; demoted = 0; reports = 0; }
};
// Round 5: ONE RECORD PER DEVICE VARIANT (the registry index of the speculative entry that a launch asked for), each with
// its own report word and probe event: a failing workload demotes its own configuration only -- an fp16 attention-sink layer
// no longer drags a benign bf16 one down with it, and a clean probe of one configuration no longer resets another's hold
// (ADVICE r04).  What stays shared is the mutex (launches are enqueued one at a time per device anyway).
struct AdaptiveSlot {
    AdaptivePolicy p;
    hipEvent_t probe_done = nullptr;  // created at the slot's first probe
};
struct AdaptiveState {
    std::mutex mu;
    uint32_t *flag_host = nullptr;  // hipHostMalloc'ed (mapped, coherent) words, one per slot; null: no pinned memory -> always speculative
    uint32_t *flag_dev = nullptr;   // the same words as the device addresses them
    std::vector<AdaptiveSlot> slot; // registry().size() records, allocated with the report words at the device's init (ADVICE
                                    // r05: a fixed 512 x 64 static array put 1.3 MB of initialised data into the library)
    int n_slots() const { return (int)slot.size(); }
};
struct DeviceState {
    std::once_flag once;
    int status = FA_OK;
    char err[256] = "";
    int num_cus = 256;  // persistent variants launch one workgroup per CU
    AdaptiveState adaptive;
    std::atomic<int> inited{0};  // published LAST (release): a reader that sees 1 sees the final status and num_cus
};
constexpr int kMaxDevices = 64;
DeviceState g_dev[kMaxDevices];

void do_init_body(int dev, DeviceState *st) {
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, dev) != hipSuccess) {
        st->status = FA_ERR_DEVICE;
        snprintf(st->err, sizeof(st->err), "hipGetDeviceProperties failed for device %d", dev);
        return;
    }
    st->num_cus = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0) {
        st->status = FA_ERR_DEVICE;
        snprintf(st->err, sizeof(st->err),
                 "Flash Attention (HIP) requires gfx950 / MI355X (device %d: %s)", dev, prop.gcnArchName);
        return;
    }
    // flash_attention.cu:142-149: opt in to large dynamic shared memory per kernel (a per-device
    // attribute of the function: applied with `dev` current)
    for (const auto &e : registry()) {
        // (each function by ITS OWN LDS size: the ring form's 160 KB does not depend on what the compiler-scheduled body of
        // the same entry uses -- ADVICE r05)
        const struct { fa::kernel_fn fn; int bytes; } fns[] = {{e.fn, e.lds_bytes}, {e.fn_ragged, e.lds_bytes}, {e.fn_ring, e.ring_lds_bytes},
                                                                 {e.fn_alt, e.lds_bytes}};
        for (const auto &f : fns) {
            if (!f.fn || f.bytes <= 48 * 1024) continue;
            const hipError_t rc = hipFuncSetAttribute((const void *)f.fn, hipFuncAttributeMaxDynamicSharedMemorySize, f.bytes);
            if (rc != hipSuccess) {
                st->status = FA_ERR_LAUNCH;
                snprintf(st->err, sizeof(st->err), "hipFuncSetAttribute(%d B LDS) on device %d: %s", f.bytes, dev,
                         hipGetErrorString(rc));
                return;
            }
        }
    }
    // the forms that also write the row log-sum-exp (fa_fwd_launch_lse): the persistent kernel's LDS
    for (int i = 0; i < 16; ++i) {   // (i & 8: their grouped-query attention forms)
        const bool masked = (i & 1) != 0, spec = (i & 2) != 0;
        const void *fn = (i & 8) ? ((i & 4) ? (const void *)fa::gqa_kernel_dt5(masked, spec) : (const void *)fa::gqa_kernel_dt15(masked, spec))
                                 : ((i & 4) ? (const void *)fa::lse_kernel_dt5(masked, spec) : (const void *)fa::lse_kernel_dt15(masked, spec));
        const hipError_t rc = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, fa::RingTraits<2>::kLdsBytes);
        if (rc != hipSuccess) {
            st->status = FA_ERR_LAUNCH;
            snprintf(st->err, sizeof(st->err), "hipFuncSetAttribute(%d B LDS, LSE form) on device %d: %s", fa::RingTraits<2>::kLdsBytes,
                     dev, hipGetErrorString(rc));
            return;
        }
    }
    // the varlen forward (fa_fwd_launch_varlen, fa_fwd_launch_varlen_qk): the 32-rows-per-wave kernel's 64 KiB
    for (int i = 0; i < 4; ++i) {
        const void *fn = (i & 2) ? (const void *)fa::varlen_kernel_dt5((i & 1) != 0) : (const void *)fa::varlen_kernel_dt15((i & 1) != 0);
        const hipError_t rc = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, fa::varlen_lds_bytes_dt15());
        if (rc != hipSuccess) {
            st->status = FA_ERR_LAUNCH;
            snprintf(st->err, sizeof(st->err), "hipFuncSetAttribute(%d B LDS, varlen form) on device %d: %s", fa::varlen_lds_bytes_dt15(),
                     dev, hipGetErrorString(rc));
            return;
        }
    }
    // ... and its form against a KV cache (fa_fwd_launch_varlen_kvcache)
    for (int i = 0; i < 4; ++i) {
        const void *fn = (i & 2) ? (const void *)fa::varlen_kvcache_kernel_dt5((i & 1) != 0) : (const void *)fa::varlen_kvcache_kernel_dt15((i & 1) != 0);
        const hipError_t rc = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, fa::varlen_lds_bytes_dt15());
        if (rc != hipSuccess) {
            st->status = FA_ERR_LAUNCH;
            snprintf(st->err, sizeof(st->err), "hipFuncSetAttribute(%d B LDS, varlen KV-cache form) on device %d: %s",
                     fa::varlen_lds_bytes_dt15(), dev, hipGetErrorString(rc));
            return;
        }
    }
    // ... and against an fp8 KV cache (fa_fwd_launch_varlen_kvcache_fp8)
    for (int i = 0; i < 4; ++i) {
        const void *fn = (i & 2) ? (const void *)fa::varlen_kvcache_fp8_kernel_dt5((i & 1) != 0) : (const void *)fa::varlen_kvcache_fp8_kernel_dt15((i & 1) != 0);
        const hipError_t rc = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, fa::varlen_lds_bytes_dt15());
        if (rc != hipSuccess) {
            st->status = FA_ERR_LAUNCH;
            snprintf(st->err, sizeof(st->err), "hipFuncSetAttribute(%d B LDS, varlen fp8 KV-cache form) on device %d: %s",
                     fa::varlen_lds_bytes_dt15(), dev, hipGetErrorString(rc));
            return;
        }
    }
    // ... and the sliding-window forms of the three (fa_fwd_launch_varlen_qk_window, _kvcache_window, _kvcache_fp8_window)
    for (int i = 0; i < 12; ++i) {
        const bool fbs = (i & 1) != 0, dt5 = (i & 2) != 0;
        const void *fn = i < 4 ? (dt5 ? (const void *)fa::varlen_window_kernel_dt5(fbs) : (const void *)fa::varlen_window_kernel_dt15(fbs))
                       : i < 8 ? (dt5 ? (const void *)fa::varlen_kvcache_window_kernel_dt5(fbs) : (const void *)fa::varlen_kvcache_window_kernel_dt15(fbs))
                               : (dt5 ? (const void *)fa::varlen_kvcache_fp8_window_kernel_dt5(fbs) : (const void *)fa::varlen_kvcache_fp8_window_kernel_dt15(fbs));
        const hipError_t rc = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, fa::varlen_lds_bytes_dt15());
        if (rc != hipSuccess) {
            st->status = FA_ERR_LAUNCH;
            snprintf(st->err, sizeof(st->err), "hipFuncSetAttribute(%d B LDS, varlen sliding-window form %d) on device %d: %s",
                     fa::varlen_lds_bytes_dt15(), i, dev, hipGetErrorString(rc));
            return;
        }
    }
    // ... and the soft-capped form of the packed one (fa_fwd_launch_varlen_qk_softcap)
    for (int i = 0; i < 4; ++i) {
        const void *fn = (i & 2) ? (const void *)fa::varlen_softcap_kernel_dt5((i & 1) != 0) : (const void *)fa::varlen_softcap_kernel_dt15((i & 1) != 0);
        const hipError_t rc = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, fa::varlen_lds_bytes_dt15());
        if (rc != hipSuccess) {
            st->status = FA_ERR_LAUNCH;
            snprintf(st->err, sizeof(st->err), "hipFuncSetAttribute(%d B LDS, varlen soft-capped form) on device %d: %s", fa::varlen_lds_bytes_dt15(),
                     dev, hipGetErrorString(rc));
            return;
        }
    }
    // ... and the form with attention sinks (fa_fwd_launch_varlen_qk_sinks)
    for (int i = 0; i < 4; ++i) {
        const void *fn = (i & 2) ? (const void *)fa::varlen_sinks_kernel_dt5((i & 1) != 0) : (const void *)fa::varlen_sinks_kernel_dt15((i & 1) != 0);
        const hipError_t rc = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, fa::varlen_lds_bytes_dt15());
        if (rc != hipSuccess) {
            st->status = FA_ERR_LAUNCH;
            snprintf(st->err, sizeof(st->err), "hipFuncSetAttribute(%d B LDS, varlen sinks form) on device %d: %s", fa::varlen_lds_bytes_dt15(), dev,
                     hipGetErrorString(rc));
            return;
        }
    }
}

void do_init(int dev, DeviceState *st) {
    do_init_body(dev, st);
    if (st->status == FA_OK) {  // the adaptive mode's report word (see AdaptiveState); without it the mode stays speculative
        void *h = nullptr, *d = nullptr;
        const size_t bytes = sizeof(uint32_t) * registry().size();
        if (hipHostMalloc(&h, bytes, hipHostMallocMapped | hipHostMallocCoherent) == hipSuccess && h &&
            hipHostGetDevicePointer(&d, h, 0) == hipSuccess && d) {
            memset(h, 0, bytes);
            st->adaptive.slot = std::vector<AdaptiveSlot>(registry().size());
            st->adaptive.flag_host = (uint32_t *)h;
            st->adaptive.flag_dev = (uint32_t *)d;
        } else {
            (void)hipGetLastError();
            if (h) (void)hipHostFree(h);
        }
    }
    st->inited.store(1, std::memory_order_release);
}

// State of the CURRENT device, initialised on first use; nullptr (and the thread's error set) if there is none.
DeviceState *current_device(int *status) {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) {
        (void)hipGetLastError();
        *status = fail(FA_ERR_DEVICE, "no HIP device available");
        return nullptr;
    }
    if (dev < 0 || dev >= kMaxDevices) {
        *status = fail(FA_ERR_DEVICE, "device ordinal %d out of range (max %d)", dev, kMaxDevices - 1);
        return nullptr;
    }
    DeviceState *st = &g_dev[dev];
    std::call_once(st->once, do_init, dev, st);
    *status = st->status == FA_OK ? FA_OK : fail(st->status, "%s", st->err);
    return st->status == FA_OK ? st : nullptr;
}

int validate(const fa_fwd_args *a, const fa::KernelEntry **out, const Want &want = Want()) {
    const bool masked = want.masked;
    if (!a || !a->q || !a->k || !a->v || !a->o) return fail(FA_ERR_NULL, "null pointer argument");
    if (a->cfg.dtype != FA_FP16 && a->cfg.dtype != FA_BF16)
        return fail(FA_ERR_DTYPE, "Only fp16 and bf16 are supported");
    const char *why = "";
    const fa::KernelEntry *e = find_kernel(&a->cfg, &why, want);
    if (!e)
        return fail(FA_ERR_NO_KERNEL, "%s%s", why,
                    masked ? " (no causal / ragged-length variant is built for this configuration)" : "");
    if (a->d_head != a->cfg.d_head)
        return fail(FA_ERR_SHAPE, "Tensor d_head (%lld) does not match kernel configuration d_head (%d)",
                    (long long)a->d_head, a->cfg.d_head);
    if (a->batch <= 0 || a->seq_len <= 0 || a->n_heads <= 0)
        return fail(FA_ERR_SHAPE, "batch, seq_len and n_heads must be positive");
    // masked == 2 (persistent kernel): a causal-only form for seq_len % B_r == 0 and a second form for every
    // other seq_len >= B_c, which fetches a tile that would reach beyond the sequence as its last B_c keys
    if (masked && want.ragged && e->masked == 2 && a->seq_len % a->cfg.B_r != 0 && (a->seq_len < a->cfg.B_c || !e->fn_ragged))
        return fail(FA_ERR_SHAPE, "the masked variant of this configuration needs seq_len >= B_c (%d) when "
                                  "seq_len is not a multiple of B_r", a->cfg.B_c);
    // (a causal launch that did not also ask for allow_ragged keeps the reference's divisibility rules)
    if (!(masked && want.ragged) && a->seq_len % a->cfg.B_r != 0)
        return fail(FA_ERR_SHAPE, "Only multiples of B_r are supported for seq_len Q currently");
    if (!(masked && want.ragged) && a->seq_len % a->cfg.B_c != 0)
        return fail(FA_ERR_SHAPE, "Only multiples of B_c are supported for seq_len K currently");
    if (a->seq_len > INT32_MAX - 1024 || a->batch * a->n_heads > INT32_MAX ||
        a->batch * a->n_heads * ((a->seq_len + a->cfg.B_r - 1) / a->cfg.B_r) > INT32_MAX)
        return fail(FA_ERR_SHAPE, "problem too large for a 1-D grid");
    // The kernels keep per-lane offsets inside a tile / Q block in 32 bits (row * seq_stride * 2 bytes for up
    // to max(B_r, B_c) rows); the batch and head strides only enter 64-bit scalar bases.  All four tensors
    // share the strides, so a zero or negative one would make rows of O alias.
    if (a->seq_stride <= 0 || a->batch_stride < 0 || a->head_stride < 0 ||
        (a->batch > 1 && a->batch_stride == 0) || (a->n_heads > 1 && a->head_stride == 0))
        return fail(FA_ERR_SHAPE, "strides must be positive (batch %lld, seq %lld, head %lld elements)",
                    (long long)a->batch_stride, (long long)a->seq_stride, (long long)a->head_stride);
    {
        const int64_t rows = a->cfg.B_r > a->cfg.B_c ? a->cfg.B_r : a->cfg.B_c;
        if (a->seq_stride > (int64_t)0xffffffffLL / (2 * rows))
            return fail(FA_ERR_SHAPE, "seq_stride %lld too large: %lld rows * seq_stride * 2 bytes must fit 32 bits",
                        (long long)a->seq_stride, (long long)rows);
    }
    // 16-byte vector accesses: element strides must be multiples of 8, pointers 16-B aligned.
    if ((a->batch_stride | a->seq_stride | a->head_stride) & 7)
        return fail(FA_ERR_ALIGN, "strides must be multiples of 8 elements (16 bytes)");
    if (((uintptr_t)a->q | (uintptr_t)a->k | (uintptr_t)a->v | (uintptr_t)a->o) & 15)
        return fail(FA_ERR_ALIGN, "q, k, v, o must be 16-byte aligned");
    *out = e;
    return FA_OK;
}

// lse != nullptr (fa_fwd_launch_lse; e is a persistent 64-rows-per-wave entry, checked by the caller): the twin of e's
// kernel that also writes the row log-sum-exp, always the plain walk (no alternating-direction twin is built); kv != nullptr as
// well (fa_fwd_launch_gqa, validated by the caller): that kernel's grouped-query attention form
int launch(const fa_fwd_args *a, const fa::KernelEntry *e, const DeviceState *dev, hipStream_t stream, int causal = 0,
           fa_fwd_stats *stats = nullptr, uint32_t *redo_flag = nullptr, uint32_t redo_seq = 0, float *lse = nullptr,
           const fa_kv_layout *kv = nullptr) {
    fa::KernelArgs ka;
    ka.stats = (uint32_t *)stats;
    ka.redo_flag = redo_flag;
    ka.redo_seq = redo_seq;
    ka.q = a->q;
    ka.k = a->k;
    ka.v = a->v;
    ka.o = a->o;
    ka.batch_stride = a->batch_stride;
    ka.seq_stride = a->seq_stride;
    ka.head_stride = a->head_stride;
    ka.seq_len = (int32_t)a->seq_len;
    ka.n_heads = (int32_t)a->n_heads;
    ka.n_bh = (int32_t)(a->batch * a->n_heads);
    ka.n_q_blocks = (int32_t)((a->seq_len + a->cfg.B_r - 1) / a->cfg.B_r);   // exact unless masked
    ka.n_kv_blocks = (int32_t)((a->seq_len + a->cfg.B_c - 1) / a->cfg.B_c);
    ka.causal = causal;
    fa::kernel_fn fn = e->fn;
    if (e->masked == 2 && a->seq_len % a->cfg.B_r != 0) {  // ragged form: whole ring rounds of K / V tiles
        fn = e->fn_ragged;
        ka.n_kv_blocks = ka.n_q_blocks * (a->cfg.B_r / a->cfg.B_c);
    }
    // 1-D grid over (batch*head, Q block); the kernel un-maps it XCD-aware.
    // (reference: dim3(n_Q_blocks, n_heads, batch), flash_attention.cu:110-112)
    // Persistent variants: one workgroup per CU (a multiple of 8, so an item keeps its XCD) that
    // walks items blockIdx.x, + gridDim.x, ... itself.
    // the ring form of a 32-rows-per-wave configuration (KernelEntry::fn_ring): seq_len a multiple of 256
    bool persistent = e->persistent != 0;
    int lds_bytes = e->lds_bytes;
    unsigned threads = (unsigned)e->threads;
    if (e->fn_ring && a->seq_len % 256 == 0 && !causal) {
        fn = e->fn_ring;
        lds_bytes = e->ring_lds_bytes;
        persistent = true;
        if (e->ring_threads) threads = (unsigned)e->ring_threads;
        if (e->ring_rows) ka.n_q_blocks = (int32_t)(a->seq_len / e->ring_rows);   // (the ring form's own items: 256 rows)
    }
    unsigned n_wg = (unsigned)(ka.n_bh * ka.n_q_blocks);
    if (persistent) {
        const unsigned cap = (unsigned)(dev->num_cus & ~7) ? (unsigned)(dev->num_cus & ~7) : 8u;
        if (n_wg > cap) n_wg = cap;
    }
    // a long head (its Q blocks fill an even number of rounds of an XCD's n_wg / 8 workgroups): the form that walks every second
    // round [tile 0, then last-to-second] (KernelEntry::fn_alt) -- a function of the sequence length and the CU count alone
    // (FA_HIP_NO_ALT in the environment, read once per process: a MEASUREMENT switch -- the same launch through the plain form,
    // for the A/B of profiles/r06/c3_alt_ab.txt; nothing in the product sets it)
    static const bool no_alt = getenv("FA_HIP_NO_ALT") != nullptr;
    if (!no_alt && persistent && fn == e->fn && e->fn_alt && (ka.n_bh & 7) == 0 && n_wg >= 16 && ka.n_q_blocks % (2 * (int)(n_wg >> 3)) == 0)
        fn = e->fn_alt;
    const dim3 grid(n_wg);
    const dim3 block(threads);
    void *params[] = {&ka};
    fa::KernelArgsLse kal{ka, lse};
    if (lse) {
        const bool masked = e->masked != 0, spec = e->softmax_mode == FA_SOFTMAX_SPECULATIVE;
        fn = (fa::kernel_fn)(a->cfg.dtype == FA_BF16 ? fa::lse_kernel_dt15(masked, spec) : fa::lse_kernel_dt5(masked, spec));
        params[0] = &kal;
    }
    fa::KernelArgsGqa kag{kal, 0, 0, 0, 1};
    if (lse && kv) {
        const bool masked = e->masked != 0, spec = e->softmax_mode == FA_SOFTMAX_SPECULATIVE;
        fn = (fa::kernel_fn)(a->cfg.dtype == FA_BF16 ? fa::gqa_kernel_dt15(masked, spec) : fa::gqa_kernel_dt5(masked, spec));
        kag.kv_batch_stride = kv->kv_batch_stride;
        kag.kv_seq_stride = kv->kv_seq_stride;
        kag.kv_head_stride = kv->kv_head_stride;
        kag.group = (int32_t)(a->n_heads / kv->n_kv_heads);
        params[0] = &kag;
    }
    hipError_t rc = hipLaunchKernel((const void *)fn, grid, block, params, (size_t)lds_bytes, stream);
    if (rc != hipSuccess) return fail(FA_ERR_LAUNCH, "hipLaunchKernel: %s", hipGetErrorString(rc));
    return FA_OK;
}

}  // namespace

extern "C" {

int fa_init(void) {
    int rc = FA_OK;
    (void)current_device(&rc);
    return rc;
}

int fa_device_state(int device, int *inited, int *status, int *num_cus) {
    if (device < 0 || device >= kMaxDevices) return fail(FA_ERR_DEVICE, "device ordinal %d out of range", device);
    const DeviceState &st = g_dev[device];
    const int done = st.inited.load(std::memory_order_acquire);  // 0: nothing below is final yet
    if (inited) *inited = done;
    if (status) *status = done ? st.status : FA_OK;
    if (num_cus) *num_cus = done ? st.num_cus : 0;
    return FA_OK;
}

int fa_fwd_supported(const fa_fwd_config *cfg) {
    if (!cfg) return 0;
    const char *why;
    return find_kernel(cfg, &why) != nullptr;
}

int fa_fwd_lds_bytes(const fa_fwd_config *cfg) {
    if (!cfg) return fail(FA_ERR_NULL, "null config");
    const char *why = "";
    const fa::KernelEntry *e = find_kernel(cfg, &why);
    if (!e) return fail(FA_ERR_NO_KERNEL, "%s", why);
    return e->lds_bytes;
}

// Enqueue (ms == nullptr) or enqueue between two events on the stream and wait for the second one
// (flash_attention.cu:119-132).  Whatever was created is destroyed on every path.
// `probe` (an adaptive probe launch): its event is recorded right behind the kernel, its policy told if that failed, and
// the device's adaptive lock -- held by the caller until then, so that no other thread queries an event that has not
// been recorded -- is released BEFORE the timed path waits for the stop event (a timed probe used to keep
// every other thread's adaptive launch on the device out for the kernel's whole duration).
struct ProbeHook {
    AdaptiveSlot *slot = nullptr;
    std::unique_lock<std::mutex> *lock = nullptr;
    void after_launch(int launch_rc, hipStream_t s) {
        if (!slot) return;
        if (launch_rc != FA_OK || hipEventRecord(slot->probe_done, s) != hipSuccess) {
            (void)hipGetLastError();
            slot->p.mode = AdaptivePolicy::NORMAL;  // (no event to wait for; a failing probe reports like any launch)
        }
        if (lock && lock->owns_lock()) lock->unlock();
        slot = nullptr;
    }
};
static int launch_maybe_timed(const fa_fwd_args *args, const fa::KernelEntry *e, const DeviceState *dev,
                              hipStream_t s, int causal, float *ms, fa_fwd_stats *stats = nullptr,
                              uint32_t *redo_flag = nullptr, uint32_t redo_seq = 0, ProbeHook probe = ProbeHook(),
                              float *lse = nullptr, const fa_kv_layout *kv = nullptr) {
    if (!ms) {
        const int rc0 = launch(args, e, dev, s, causal, stats, redo_flag, redo_seq, lse, kv);
        probe.after_launch(rc0, s);
        return rc0;
    }
    hipEvent_t start = nullptr, stop = nullptr;
    hipError_t hrc = hipEventCreate(&start);
    if (hrc == hipSuccess) hrc = hipEventCreate(&stop);
    if (hrc == hipSuccess) hrc = hipEventRecord(start, s);
    int rc = FA_OK;
    if (hrc == hipSuccess) {
        rc = launch(args, e, dev, s, causal, stats, redo_flag, redo_seq, lse, kv);
        probe.after_launch(rc, s);
        hrc = hipEventRecord(stop, s);  // (recorded even if the launch failed: nothing is left pending)
        if (hrc == hipSuccess) hrc = hipEventSynchronize(stop);
    }
    float elapsed = 0.0f;
    if (hrc == hipSuccess && rc == FA_OK) hrc = hipEventElapsedTime(&elapsed, start, stop);
    probe.after_launch(FA_ERR_LAUNCH, s);  // (only if the events could not even be created: nothing was launched)
    if (start) (void)hipEventDestroy(start);
    if (stop) (void)hipEventDestroy(stop);
    if (rc != FA_OK) return rc;
    if (hrc != hipSuccess) return fail(FA_ERR_LAUNCH, "event timing / kernel execution: %s", hipGetErrorString(hrc));
    *ms = elapsed;
    return FA_OK;
}

int fa_fwd_launch(const fa_fwd_args *args, void *stream) {
    const fa::KernelEntry *e = nullptr;
    int rc = validate(args, &e);
    if (rc != FA_OK) return rc;
    const DeviceState *dev = current_device(&rc);
    if (!dev) return rc;
    return launch(args, e, dev, (hipStream_t)stream);
}

int fa_fwd_launch_timed(const fa_fwd_args *args, void *stream, float *ms) {
    if (!ms) return fail(FA_ERR_NULL, "null ms pointer");
    const fa::KernelEntry *e = nullptr;
    int rc = validate(args, &e);
    if (rc != FA_OK) return rc;
    const DeviceState *dev = current_device(&rc);
    if (!dev) return rc;
    return launch_maybe_timed(args, e, dev, (hipStream_t)stream, 0, ms);
}

int fa_fwd_masked_supported(const fa_fwd_config *cfg) {
    if (!cfg) return 0;
    const char *why;
    Want w;
    w.masked = true;
    return find_kernel(cfg, &why, w) != nullptr;
}

int fa_fwd_launch_masked(const fa_fwd_args *args, int causal, void *stream, float *ms) {
    fa_fwd_opts o;
    memset(&o, 0, sizeof(o));
    o.struct_size = (uint32_t)sizeof(o);
    o.causal = causal;
    o.allow_ragged = 1;
    o.ms = ms;
    return fa_fwd_launch_ex(args, &o, stream);
}

// fa_fwd_opts as this library understands it: a caller built against an older (shorter) header passes a
// smaller struct_size and gets zeros for the fields it does not know.
static int read_opts(const fa_fwd_opts *in, fa_fwd_opts *o) {
    memset(o, 0, sizeof(*o));
    if (!in) return FA_OK;
    if (in->struct_size < sizeof(uint32_t) || in->struct_size > 4096)
        return fail(FA_ERR_SHAPE, "fa_fwd_opts.struct_size (%u) is not set: zero the struct and set it to sizeof(fa_fwd_opts)",
                    in->struct_size);
    memcpy(o, in, in->struct_size < sizeof(*o) ? in->struct_size : sizeof(*o));
    // (checked HERE so that fa_fwd_ex_supported, fa_fwd_query and fa_fwd_launch_ex agree: ADVICE r04)
    if (o->speculative < 0 || o->speculative > FA_SPECULATIVE_ADAPTIVE)
        return fail(FA_ERR_SHAPE, "fa_fwd_opts.speculative must be 0, 1 (always) or 2 (adaptive), not %d", o->speculative);
    return FA_OK;
}

// hipEventQuery is not a capture-safe call: with another thread's stream in a global-mode capture it would invalidate
// that capture.  Queried in relaxed mode (this thread's view only); if the mode cannot be switched the probe counts as
// still pending -- the policy stays demoted, which is always valid.
static int query_probe(hipEvent_t ev) {
    hipStreamCaptureMode mode = hipStreamCaptureModeRelaxed;
    if (hipThreadExchangeStreamCaptureMode(&mode) != hipSuccess) { (void)hipGetLastError(); return AdaptivePolicy::PROBE_PENDING; }
    const hipError_t q = hipEventQuery(ev);
    if (q != hipSuccess) (void)hipGetLastError();
    if (hipThreadExchangeStreamCaptureMode(&mode) != hipSuccess) (void)hipGetLastError();
    return q == hipSuccess ? AdaptivePolicy::PROBE_COMPLETE
                           : (q == hipErrorNotReady ? AdaptivePolicy::PROBE_PENDING : AdaptivePolicy::PROBE_ERROR);
}

int fa_fwd_ex_supported(const fa_fwd_config *cfg, const fa_fwd_opts *opts) {
    if (!cfg) return 0;
    fa_fwd_opts o;
    if (read_opts(opts, &o) != FA_OK) return 0;
    const char *why;
    Want w;
    w.masked = o.causal || o.allow_ragged;
    w.ragged = o.allow_ragged != 0;
    w.speculative = o.speculative != 0;
    w.prescaled_q = o.prescaled_q != 0;
    return find_kernel(cfg, &why, w) != nullptr;
}

// Does the entry the options select have a form that writes the row log-sum-exp?  (the persistent 64-rows-per-wave kernel,
// plain or causal, without the pre-scaled Q: fa_fwd_kernel64_lse; allow_ragged selects the masked entry, whose seq_len % 256
// == 0 launches fa_fwd_launch_lse serves with its causal form -- a ragged seq_len is refused there)
static bool lse_form(const fa_fwd_config *cfg, const fa_fwd_opts &o, const fa::KernelEntry *e) {
    return e && e->persistent && e->rows_per_wave == 64 && e->d_head == 128 && !e->prescaled_q &&
           !o.prescaled_q && cfg->d_head == 128 && (cfg->dtype == FA_BF16 || cfg->dtype == FA_FP16);
}

// fa_fwd_launch_ex, fa_fwd_launch_lse (lse != nullptr; the caller has checked lse_form) and fa_fwd_launch_gqa (kv != nullptr too)
static int launch_ex_impl(const fa_fwd_args *args, const fa_fwd_opts *opts, void *stream, float *lse, const fa_kv_layout *kv = nullptr) {
    fa_fwd_opts o;
    int rc = read_opts(opts, &o);
    if (rc != FA_OK) return rc;
    Want w;
    w.masked = o.causal || o.allow_ragged;
    w.ragged = o.allow_ragged != 0;
    w.speculative = o.speculative != 0;
    w.prescaled_q = o.prescaled_q != 0;
    const fa::KernelEntry *e = nullptr;
    rc = validate(args, &e, w);
    if (rc != FA_OK) return rc;
    if (o.stats && ((uintptr_t)o.stats & 3)) return fail(FA_ERR_ALIGN, "fa_fwd_opts.stats must be 4-byte aligned");
    DeviceState *dev = current_device(&rc);
    if (!dev) return rc;
    uint32_t *redo_flag = nullptr;
    uint32_t redo_seq = 0;
    ProbeHook hook;
    std::unique_lock<std::mutex> probe_lock;
    if (o.speculative == FA_SPECULATIVE_ADAPTIVE && dev->adaptive.flag_host) {
        // (the speculative variant exists: validated above.  Its non-speculative sibling serves a demoted launch)
        hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
        if (hipStreamIsCapturing((hipStream_t)stream, &cap) != hipSuccess) { (void)hipGetLastError(); cap = hipStreamCaptureStatusNone; }
        AdaptiveState &ad = dev->adaptive;
        const int idx = (int)(e - registry().data());   // the record of THIS device variant
        bool demote = false;
        if (cap == hipStreamCaptureStatusNone && idx >= 0 && idx < ad.n_slots()) {
            AdaptiveSlot &sl = ad.slot[idx];
            probe_lock = std::unique_lock<std::mutex>(ad.mu);
            int probe = AdaptivePolicy::PROBE_NA;
            if (sl.p.mode == AdaptivePolicy::PROBING) probe = query_probe(sl.probe_done);   // has the probe finished?  (never a wait)
            const uint32_t rep = __atomic_load_n(ad.flag_host + idx, __ATOMIC_ACQUIRE);   // (behind the query: see step())
            int run = sl.p.step(rep, probe);
            if (run == AdaptivePolicy::RUN_PROBE && !sl.probe_done &&
                hipEventCreateWithFlags(&sl.probe_done, hipEventDisableTiming) != hipSuccess) {
                (void)hipGetLastError();
                sl.probe_done = nullptr;
                sl.p.mode = AdaptivePolicy::NORMAL;   // no event to probe with: speculative, reports still demote
                run = AdaptivePolicy::RUN_SPECULATIVE;
            }
            demote = run == AdaptivePolicy::RUN_DEMOTED;
            redo_flag = ad.flag_dev + idx;
            redo_seq = sl.p.seq;
            // (a probe keeps the lock until its event is recorded -- ProbeHook: another thread's launch must not query an
            // event that has not been recorded yet, it would read as complete)
            if (run == AdaptivePolicy::RUN_PROBE) { hook.slot = &sl; hook.lock = &probe_lock; }
            else probe_lock.unlock();
        }
        if (demote) {
            Want w2 = w;
            w2.speculative = false;
            const fa::KernelEntry *e2 = nullptr;
            if (validate(args, &e2, w2) == FA_OK) {
                e = e2;
                redo_flag = nullptr;
            }  // (no such sibling: the speculative variant stays)
        }
    }
    return launch_maybe_timed(args, e, dev, (hipStream_t)stream, o.causal != 0, o.ms, o.stats, redo_flag, redo_seq, hook, lse, kv);
}

int fa_fwd_launch_ex(const fa_fwd_args *args, const fa_fwd_opts *opts, void *stream) {
    return launch_ex_impl(args, opts, stream, nullptr);
}

int fa_fwd_lse_supported(const fa_fwd_config *cfg, const fa_fwd_opts *opts) {
    if (!cfg) return 0;
    fa_fwd_opts o;
    if (read_opts(opts, &o) != FA_OK) return 0;
    const char *why;
    Want w;
    w.masked = o.causal || o.allow_ragged;
    w.ragged = o.allow_ragged != 0;
    w.speculative = o.speculative != 0;
    w.prescaled_q = o.prescaled_q != 0;
    return lse_form(cfg, o, find_kernel(cfg, &why, w)) ? 1 : 0;
}

int fa_fwd_launch_lse(const fa_fwd_args *args, const fa_fwd_opts *opts, float *lse, void *stream) {
    if (!args) return fail(FA_ERR_NULL, "null pointer argument");
    if (!lse) return fail(FA_ERR_NULL, "lse is null: fa_fwd_launch_lse needs a (batch, n_heads, seq_len) fp32 buffer");
    if ((uintptr_t)lse & 3) return fail(FA_ERR_ALIGN, "lse must be 4-byte aligned");
    fa_fwd_opts o;
    int rc = read_opts(opts, &o);
    if (rc != FA_OK) return rc;
    if (!fa_fwd_lse_supported(&args->cfg, opts))
        return fail(FA_ERR_NO_KERNEL, "the row log-sum-exp is written by the persistent (B_r 256, B_c 64, 4 warps) + buffer "
                                      "configuration at d_head 128 only, plain or causal, without prescaled_q");
    if (args->seq_len % 256 != 0)
        return fail(FA_ERR_SHAPE, "fa_fwd_launch_lse needs seq_len %% 256 == 0 (got %lld)", (long long)args->seq_len);
    // (the persistent kernel's Q request assumes it: a separate fix for every entry point)
    if (args->seq_stride % 128 != 0)
        return fail(FA_ERR_SHAPE, "fa_fwd_launch_lse needs seq_stride %% 128 == 0 (got %lld)", (long long)args->seq_stride);
    return launch_ex_impl(args, opts, stream, lse);
}

namespace {
// one stride set of the backward: positive multiples of 8, 32-bit per-lane row offsets inside a 256-row block
int check_strides(const char *which, int64_t batch, int64_t n_heads, int64_t bs, int64_t ss, int64_t hs) {
    if (ss <= 0 || bs < 0 || hs < 0 || (batch > 1 && bs == 0) || (n_heads > 1 && hs == 0))
        return fail(FA_ERR_SHAPE, "%s strides must be positive (batch %lld, seq %lld, head %lld elements)", which, (long long)bs,
                    (long long)ss, (long long)hs);
    if ((bs | ss | hs) & 7) return fail(FA_ERR_ALIGN, "%s strides must be multiples of 8 elements (16 bytes)", which);
    if (ss > (int64_t)0xffffffffLL / (2 * 256))
        return fail(FA_ERR_SHAPE, "%s seq_stride %lld too large: 256 rows * seq_stride * 2 bytes must fit 32 bits", which, (long long)ss);
    return FA_OK;
}

int bwd_validate(const fa_bwd_args *a) {
    if (!a) return fail(FA_ERR_NULL, "null pointer argument");
    if (a->dtype != FA_FP16 && a->dtype != FA_BF16) return fail(FA_ERR_DTYPE, "Only fp16 and bf16 are supported");
    if (a->d_head != 128) return fail(FA_ERR_SHAPE, "the backward supports d_head = 128 only (got %lld)", (long long)a->d_head);
    if (a->batch <= 0 || a->seq_len <= 0 || a->n_heads <= 0) return fail(FA_ERR_SHAPE, "batch, seq_len and n_heads must be positive");
    if (a->seq_len % 256 != 0)
        return fail(FA_ERR_SHAPE, "the backward needs seq_len %% 256 == 0 (got %lld)", (long long)a->seq_len);
    if (a->seq_len > INT32_MAX / 2 || a->batch * a->n_heads > INT32_MAX / 2 || a->batch * a->n_heads * (a->seq_len / 128) > INT32_MAX)
        return fail(FA_ERR_SHAPE, "problem too large for a 1-D grid");
    int rc = check_strides("qkv", a->batch, a->n_heads, a->qkv_batch_stride, a->qkv_seq_stride, a->qkv_head_stride);
    if (rc != FA_OK) return rc;
    return check_strides("out", a->batch, a->n_heads, a->out_batch_stride, a->out_seq_stride, a->out_head_stride);
}
}  // namespace

int64_t fa_bwd_workspace_bytes(const fa_bwd_args *args) {
    const int rc = bwd_validate(args);
    if (rc != FA_OK) return rc;
    return (int64_t)sizeof(float) * args->batch * args->n_heads * args->seq_len;
}

namespace {
// fa_bwd_launch / fa_bwd_launch_gqa: a validated a's pointer checks, then the kernels' argument block (strides as given)
int bwd_prepare(const fa_bwd_args *a, fa::BwdArgs *out) {
    if (!a->q || !a->k || !a->v || !a->o || !a->dout || !a->dq || !a->dk || !a->dv)
        return fail(FA_ERR_NULL, "null tensor pointer (q, k, v, o, dout, dq, dk and dv are all needed)");
    if (!a->lse) return fail(FA_ERR_NULL, "lse is null: the backward needs the forward's (batch, n_heads, seq_len) fp32 lse");
    if (!a->workspace) return fail(FA_ERR_NULL, "workspace is null: allocate fa_bwd_workspace_bytes(args) bytes of device memory");
    if (((uintptr_t)a->q | (uintptr_t)a->k | (uintptr_t)a->v | (uintptr_t)a->o | (uintptr_t)a->dout | (uintptr_t)a->dq |
         (uintptr_t)a->dk | (uintptr_t)a->dv) & 15)
        return fail(FA_ERR_ALIGN, "q, k, v, o, dout, dq, dk, dv must be 16-byte aligned");
    // (the kernels read lse and delta as single floats)
    if (((uintptr_t)a->lse | (uintptr_t)a->workspace) & 3) return fail(FA_ERR_ALIGN, "lse and workspace must be 4-byte aligned");
    fa::BwdArgs &ba = *out;
    ba.q = (const uint16_t *)a->q;
    ba.k = (const uint16_t *)a->k;
    ba.v = (const uint16_t *)a->v;
    ba.o = (const uint16_t *)a->o;
    ba.dout = (const uint16_t *)a->dout;
    ba.lse = a->lse;
    ba.delta = (float *)a->workspace;
    ba.dq = (uint16_t *)a->dq;
    ba.dk = (uint16_t *)a->dk;
    ba.dv = (uint16_t *)a->dv;
    ba.qkv_bs = a->qkv_batch_stride;
    ba.qkv_ss = a->qkv_seq_stride;
    ba.qkv_hs = a->qkv_head_stride;
    ba.out_bs = a->out_batch_stride;
    ba.out_ss = a->out_seq_stride;
    ba.out_hs = a->out_head_stride;
    ba.seq_len = (int32_t)a->seq_len;
    ba.n_heads = (int32_t)a->n_heads;
    ba.n_bh = (int32_t)(a->batch * a->n_heads);
    return FA_OK;
}

// enqueue() on s; ms != nullptr: bracketed by events, blocking, the elapsed ms into *ms
extern "C++" {   // (a template, inside the extern "C" block)
template <class F> int enqueue_timed(F enqueue, hipStream_t s, float *ms) {
    if (!ms) {
        const hipError_t hrc = enqueue();
        return hrc == hipSuccess ? FA_OK : fail(FA_ERR_LAUNCH, "hipLaunchKernel (backward): %s", hipGetErrorString(hrc));
    }
    hipEvent_t start = nullptr, stop = nullptr;
    hipError_t hrc = hipEventCreate(&start);
    if (hrc == hipSuccess) hrc = hipEventCreate(&stop);
    if (hrc == hipSuccess) hrc = hipEventRecord(start, s);
    hipError_t lrc = hipSuccess;
    if (hrc == hipSuccess) {
        lrc = enqueue();
        hrc = hipEventRecord(stop, s);
        if (hrc == hipSuccess) hrc = hipEventSynchronize(stop);
    }
    float elapsed = 0.0f;
    if (hrc == hipSuccess && lrc == hipSuccess) hrc = hipEventElapsedTime(&elapsed, start, stop);
    if (start) (void)hipEventDestroy(start);
    if (stop) (void)hipEventDestroy(stop);
    if (lrc != hipSuccess) return fail(FA_ERR_LAUNCH, "hipLaunchKernel (backward): %s", hipGetErrorString(lrc));
    if (hrc != hipSuccess) return fail(FA_ERR_LAUNCH, "event timing / kernel execution: %s", hipGetErrorString(hrc));
    *ms = elapsed;
    return FA_OK;
}
}

// Grouped-query attention: n_kv_heads divides n_heads, and K / V strides the kernels can address
int kv_validate(const char *which, int64_t batch, int64_t n_heads, int64_t n_kv_heads, int64_t bs, int64_t ss, int64_t hs) {
    if (n_kv_heads < 1 || n_kv_heads > n_heads || n_heads % n_kv_heads != 0)
        return fail(FA_ERR_SHAPE, "grouped-query attention needs n_kv_heads (%lld) to divide n_heads (%lld)", (long long)n_kv_heads,
                    (long long)n_heads);
    return check_strides(which, batch, n_kv_heads, bs, ss, hs);
}

int bwd_gqa_validate(const fa_bwd_gqa_args *g) {
    if (!g) return fail(FA_ERR_NULL, "null pointer argument");
    int rc = bwd_validate(&g->base);
    if (rc != FA_OK) return rc;
    const fa_bwd_args &a = g->base;
    rc = kv_validate("kv", a.batch, a.n_heads, g->n_kv_heads, g->kv_batch_stride, g->kv_seq_stride, g->kv_head_stride);
    if (rc != FA_OK) return rc;
    return check_strides("dkv", a.batch, g->n_kv_heads, g->dkv_batch_stride, g->dkv_seq_stride, g->dkv_head_stride);
}

// Workgroups per (K / V head, key block) of a dK / dV kernel: the smallest divisor of the group that gives the grid at least
// 256 workgroups (one per CU of an MI355X), 1024 causal (a causal block's sweep is 1 .. seq_len / 128 tiles long: the
// dispatcher evens that out only with several workgroups per CU).  `workgroups`: the grid without a split.  A function of the
// shape alone.
int64_t bwd_dkdv_split(int64_t group, int64_t workgroups, bool causal) {
    const int64_t want = causal ? 1024 : 256;
    for (int64_t s = 1; s < group; ++s)
        if (group % s == 0 && workgroups * s >= want) return s;
    return group;
}
int64_t bwd_gqa_split(const fa_bwd_gqa_args *g) {
    const fa_bwd_args &a = g->base;
    return bwd_dkdv_split(a.n_heads / g->n_kv_heads, a.batch * g->n_kv_heads * (a.seq_len / 128), a.causal != 0);
}

int64_t bwd_gqa_part_bytes(const fa_bwd_gqa_args *g, int64_t split) {   // the split's fp32 partials
    const fa_bwd_args &a = g->base;
    return split > 1 ? (int64_t)sizeof(float) * a.batch * g->n_kv_heads * split * a.seq_len * 2 * 128 : 0;
}
}  // namespace

int fa_bwd_launch(const fa_bwd_args *a, void *stream, float *ms) {
    int rc = bwd_validate(a);
    if (rc != FA_OK) return rc;
    fa::BwdArgs ba;
    rc = bwd_prepare(a, &ba);
    if (rc != FA_OK) return rc;
    DeviceState *dev = current_device(&rc);
    if (!dev) return rc;
    const hipStream_t s = (hipStream_t)stream;
    return enqueue_timed([&] { return fa::bwd_enqueue(ba, a->dtype, a->causal != 0, s); }, s, ms);
}

int64_t fa_bwd_gqa_workspace_bytes(const fa_bwd_gqa_args *g) {
    const int rc = bwd_gqa_validate(g);
    if (rc != FA_OK) return rc;
    return fa_bwd_workspace_bytes(&g->base) + bwd_gqa_part_bytes(g, bwd_gqa_split(g));
}

int fa_bwd_launch_gqa(const fa_bwd_gqa_args *g, void *stream, float *ms) {
    int rc = bwd_gqa_validate(g);
    if (rc != FA_OK) return rc;
    const fa_bwd_args *a = &g->base;
    fa::BwdGqaArgs ga;
    rc = bwd_prepare(a, &ga.base);
    if (rc != FA_OK) return rc;
    const int64_t split = bwd_gqa_split(g);
    if (split > 1 && ((uintptr_t)a->workspace & 15))
        return fail(FA_ERR_ALIGN, "workspace must be 16-byte aligned (it holds the fp32 partials of dK / dV)");
    DeviceState *dev = current_device(&rc);
    if (!dev) return rc;
    ga.kv_bs = g->kv_batch_stride;
    ga.kv_ss = g->kv_seq_stride;
    ga.kv_hs = g->kv_head_stride;
    ga.dkv_bs = g->dkv_batch_stride;
    ga.dkv_ss = g->dkv_seq_stride;
    ga.dkv_hs = g->dkv_head_stride;
    // (behind delta: B * H * seq_len floats, a multiple of 1 KiB)
    ga.part = split > 1 ? (float *)((char *)a->workspace + fa_bwd_workspace_bytes(a)) : nullptr;
    ga.group = (int32_t)(a->n_heads / g->n_kv_heads);
    ga.split = (int32_t)split;
    const hipStream_t s = (hipStream_t)stream;
    return enqueue_timed([&] { return fa::bwd_gqa_enqueue(ga, a->dtype, a->causal != 0, s); }, s, ms);
}

int fa_fwd_gqa_supported(const fa_fwd_config *cfg, const fa_fwd_opts *opts) {
    return fa_fwd_lse_supported(cfg, opts);
}

int fa_fwd_launch_gqa(const fa_fwd_args *args, const fa_kv_layout *kv, const fa_fwd_opts *opts, float *lse, void *stream) {
    if (!args || !kv) return fail(FA_ERR_NULL, "null pointer argument");
    if (!lse) return fail(FA_ERR_NULL, "lse is null: fa_fwd_launch_gqa needs a (batch, n_heads, seq_len) fp32 buffer");
    if (kv->struct_size < sizeof(fa_kv_layout))
        return fail(FA_ERR_SHAPE, "fa_kv_layout.struct_size (%u) is smaller than this library's (%zu)", kv->struct_size, sizeof(fa_kv_layout));
    fa_fwd_opts o;
    int rc = read_opts(opts, &o);
    if (rc != FA_OK) return rc;
    if (!fa_fwd_gqa_supported(&args->cfg, opts))
        return fail(FA_ERR_NO_KERNEL, "grouped-query attention is served by the persistent (B_r 256, B_c 64, 4 warps) + buffer "
                                      "configuration at d_head 128 only, plain or causal, without prescaled_q");
    if (args->n_heads <= 0) return fail(FA_ERR_SHAPE, "batch, seq_len and n_heads must be positive");
    rc = kv_validate("kv", args->batch, args->n_heads, kv->n_kv_heads, kv->kv_batch_stride, kv->kv_seq_stride, kv->kv_head_stride);
    if (rc != FA_OK) return rc;
    // (fa_fwd_launch_lse checks seq_len, Q's seq_stride and lse's alignment, and validates the rest before any HIP call)
    if (args->seq_len % 256 != 0)
        return fail(FA_ERR_SHAPE, "fa_fwd_launch_gqa needs seq_len %% 256 == 0 (got %lld)", (long long)args->seq_len);
    if (args->seq_stride % 128 != 0)
        return fail(FA_ERR_SHAPE, "fa_fwd_launch_gqa needs seq_stride %% 128 == 0 (got %lld)", (long long)args->seq_stride);
    if ((uintptr_t)lse & 3) return fail(FA_ERR_ALIGN, "lse must be 4-byte aligned");
    return launch_ex_impl(args, opts, stream, lse, kv);
}

// ---- the KV cache, as decode, the append and the cache prefill see it ------------------------------------------------------------
// One description of a contiguous or paged cache, filled by one constructor per public struct (each in front of its path), and one
// set of rules over it.  The rules are small functions that every path calls where its own order of checks has them: that order is
// observable -- an input that breaks two rules reports the first -- and tests/test_host_corpus_cpu.py pins it.
namespace {
extern "C++" {   // (inside the file's extern "C" block: internal linkage, so that nothing here is exported; templates need it too)
struct CacheView {
    const int32_t *cache_seqlens = nullptr, *block_table = nullptr;   // block_table: null = a contiguous cache
    int64_t seqlen_cache = 0, num_pages = 0, page_size = 0, max_pages_per_seq = 0, block_table_stride = 0, max_seqlen_k = 0;
    int64_t entries = 0, n_kv_heads = 0;       // entries: batch, or the prefill's n_seqs
    int64_t kv_bs = 0, kv_ss = 0, kv_hs = 0;   // elements (an fp8 cache: bytes)
    bool fp8 = false;
    const float *k_descale = nullptr, *v_descale = nullptr;
    int64_t descale_bs = 0;
    const char *words_4b = "";   // the path's name for the pointers cache_alignment checks
    bool paged() const { return block_table != nullptr; }
    int64_t capacity() const { return paged() ? max_pages_per_seq * page_size : seqlen_cache; }   // keys per entry
    int64_t slots() const { return paged() ? num_pages : entries; }                                // the cache tensors' first size
};

// one stride set: positive where the size asks for it, multiples of `unit` elements (16 bytes)
int stride_set(const char *which, int64_t unit, int64_t n0, int64_t n1, int64_t n2, int64_t bs, int64_t ss, int64_t hs) {
    if (ss <= 0 || bs < 0 || hs < 0 || (n0 > 1 && bs == 0) || (n2 > 1 && hs == 0) || (n1 > 1 && ss == 0))
        return fail(FA_ERR_SHAPE, "%s strides must be positive (batch %lld, seq %lld, head %lld elements)", which, (long long)bs,
                    (long long)ss, (long long)hs);
    if ((bs | ss | hs) & (unit - 1)) return fail(FA_ERR_ALIGN, "%s strides must be multiples of %lld elements (16 bytes)", which, (long long)unit);
    return FA_OK;
}

// the page rule (no kernel serves another page size).  The append asks it ahead of its sizes, where page_size may still be bad.
int cache_page_rule(const CacheView &c) {
    if (c.paged() && c.page_size > 0 && c.page_size % 64 != 0)
        return fail(FA_ERR_NO_KERNEL, "paged cache: page_size must be a multiple of 64 (got %lld)", (long long)c.page_size);
    return FA_OK;
}

// the sizes of a paged or a contiguous cache
int cache_sizes(const CacheView &c) {
    if (!c.paged()) return c.seqlen_cache > 0 ? FA_OK : fail(FA_ERR_SHAPE, "seqlen_cache must be positive (got %lld)", (long long)c.seqlen_cache);
    if (c.page_size <= 0 || c.num_pages <= 0 || c.max_pages_per_seq <= 0)
        return fail(FA_ERR_SHAPE, "paged cache: num_pages, page_size and max_pages_per_seq must be positive");
    if (const int rc = cache_page_rule(c)) return rc;
    if (c.block_table_stride < c.max_pages_per_seq)
        return fail(FA_ERR_SHAPE, "block_table_stride (%lld) is smaller than max_pages_per_seq (%lld)", (long long)c.block_table_stride,
                    (long long)c.max_pages_per_seq);
    if (c.num_pages > INT32_MAX / 2 || c.page_size > INT32_MAX / 2 || c.max_pages_per_seq > INT32_MAX / 2)
        return fail(FA_ERR_SHAPE, "cache too large: lengths are 32-bit");
    return FA_OK;
}

// ... and, behind them, the capacity and the host's bound on the lengths (0 = the capacity; the append has none)
int cache_bounds(const CacheView &c) {
    const int64_t cap = c.capacity();
    if (cap > INT32_MAX / 2) return fail(FA_ERR_SHAPE, "cache too large: lengths are 32-bit");
    if (c.max_seqlen_k < 0 || c.max_seqlen_k > cap)
        return fail(FA_ERR_SHAPE, "max_seqlen_k (%lld) must lie in [0, %lld] (0 = the cache's capacity)", (long long)c.max_seqlen_k, (long long)cap);
    return FA_OK;
}

// the cache's stride set (decode and the append; the prefill's token and head strides take the packed tensors' rules)
int cache_strides(const CacheView &c, int64_t unit) { return stride_set("kv", unit, c.slots(), c.capacity(), c.n_kv_heads, c.kv_bs, c.kv_ss, c.kv_hs); }

// an fp8 cache's strides count bytes (decode and the prefill; the append words the same rule as stride_set's, unit 16)
int cache_fp8_strides(const CacheView &c) {
    if (c.fp8 && ((c.kv_bs | c.kv_ss | c.kv_hs) & 15)) return fail(FA_ERR_ALIGN, "kv strides of an fp8 cache must be multiples of 16 bytes");
    return FA_OK;
}

int cache_descale_stride(const CacheView &c) {
    if ((c.k_descale || c.v_descale) && c.descale_bs < c.n_kv_heads)
        return fail(FA_ERR_SHAPE, "descale_batch_stride (%lld) is smaller than n_kv_heads (%lld)", (long long)c.descale_bs, (long long)c.n_kv_heads);
    return FA_OK;
}

// the 4-byte pointers: the lengths, the block table and what else the path names with them in words_4b
int cache_alignment(const CacheView &c, uintptr_t others = 0) {
    if (((uintptr_t)c.cache_seqlens | (uintptr_t)c.block_table | others) & 3) return fail(FA_ERR_ALIGN, "%s must be 4-byte aligned", c.words_4b);
    return FA_OK;
}
int cache_descale_alignment(const CacheView &c) {
    if (((uintptr_t)c.k_descale | (uintptr_t)c.v_descale) & 3) return fail(FA_ERR_ALIGN, "k_descale and v_descale must be 4-byte aligned");
    return FA_OK;
}

// the geometry, from any struct with these members (a public struct, or the prefill's layout)
template <class A> void cache_geometry(CacheView &c, const A &a) {
    c.cache_seqlens = a.cache_seqlens;
    c.block_table = a.block_table;
    c.seqlen_cache = a.seqlen_cache;
    c.num_pages = a.num_pages;
    c.page_size = a.page_size;
    c.max_pages_per_seq = a.max_pages_per_seq;
    c.block_table_stride = a.block_table_stride;
}
// ... and the stride set and the heads of a struct that carries them itself (decode and the append)
template <class A> void cache_tensors(CacheView &c, const A &a) {
    cache_geometry(c, a);
    c.entries = a.batch;
    c.n_kv_heads = a.n_kv_heads;
    c.kv_bs = a.kv_batch_stride;
    c.kv_ss = a.kv_seq_stride;
    c.kv_hs = a.kv_head_stride;
}
template <class A> void cache_descales(CacheView &c, const A &a) {
    c.k_descale = a.k_descale;
    c.v_descale = a.v_descale;
    c.descale_bs = a.descale_batch_stride;
}
}
}  // namespace

// ---- fa_window: the rules every windowed entry point shares (decode, the packed forward and backward, the prefills) ---------
namespace {
constexpr int64_t kWindowMaxLen = (1 << 30) - 128;   // the kernels add a row's position and its clamped distances in 32 bits
int window_right(const fa_window *w, int causal) { return causal ? 0 : w->right; }

// (called behind the unwindowed entry's own rules: the cache is valid)
int window_validate(const fa_window *w, int causal, int64_t capacity) {
    if (!w) return fail(FA_ERR_NULL, "fa_window is null: (left, right) is needed (-1 = unbounded; the unwindowed entry point takes none)");
    if (w->struct_size < sizeof(fa_window))
        return fail(FA_ERR_SHAPE, "fa_window.struct_size (%u) is smaller than this library's (%zu)", w->struct_size, sizeof(fa_window));
    if (w->left < -1 || w->right < -1)
        return fail(FA_ERR_SHAPE, "window (%d, %d): left and right must be -1 (unbounded) or not negative", w->left, w->right);
    if (causal && w->right > 0)
        return fail(FA_ERR_SHAPE, "causal means right = 0: a window with right = %d cannot be causal as well (pass right = -1 or 0)", w->right);
    if (capacity > kWindowMaxLen) return fail(FA_ERR_SHAPE, "cache too large for a window: at most 2^30 - 128 keys per entry");
    return FA_OK;
}
}  // namespace

// ---- packed variable-length sequences: one range for Q and K / V (fa_*_varlen) or one each (fa_*_varlen_qk) ------------------
// One host path, of two ranges; the entry points with one fa_varlen_layout pass it for both sides.  Each entry point keeps its
// own name, and its name for the query side's total, in its messages.  The forward has one kernel; the backward keeps the
// single-range kernels beside the two-range ones (theirs are faster), so the two backward entries share the
// checks, the split and the argument fill and differ in the kernels they enqueue.
namespace {
int varlen_validate(const fa_varlen_layout *vl) {
    if (!vl) return fail(FA_ERR_NULL, "null pointer argument");
    if (vl->struct_size < sizeof(fa_varlen_layout))
        return fail(FA_ERR_SHAPE, "fa_varlen_layout.struct_size (%u) is smaller than this library's (%zu)", vl->struct_size,
                    sizeof(fa_varlen_layout));
    if (!vl->cu_seqlens) return fail(FA_ERR_NULL, "cu_seqlens is null: a DEVICE pointer to n_seqs + 1 int32 row offsets is needed");
    if ((uintptr_t)vl->cu_seqlens & 3) return fail(FA_ERR_ALIGN, "cu_seqlens must be 4-byte aligned");
    if (vl->n_seqs < 1) return fail(FA_ERR_SHAPE, "n_seqs must be at least 1 (got %lld)", (long long)vl->n_seqs);
    if (vl->total_tokens < 0) return fail(FA_ERR_SHAPE, "total_tokens must not be negative (got %lld)", (long long)vl->total_tokens);
    if (vl->max_seqlen < 1) return fail(FA_ERR_SHAPE, "max_seqlen must be at least 1 (got %lld)", (long long)vl->max_seqlen);
    if (vl->total_tokens > INT32_MAX / 2 || vl->max_seqlen > INT32_MAX / 2 || vl->n_seqs > INT32_MAX / 2)
        return fail(FA_ERR_SHAPE, "problem too large for a 1-D grid");
    return FA_OK;
}

// the two layouts of one launch: each valid by itself, one sequence count
int varlen_qk_validate(const fa_varlen_layout *vq, const fa_varlen_layout *vk) {
    int rc = varlen_validate(vq);
    if (rc != FA_OK) return rc;
    if ((rc = varlen_validate(vk)) != FA_OK) return rc;
    if (vq->n_seqs != vk->n_seqs)
        return fail(FA_ERR_SHAPE, "n_seqs mismatch: the query side has %lld sequences, the key side %lld", (long long)vq->n_seqs,
                    (long long)vk->n_seqs);
    return FA_OK;
}

// one stride set of a packed tensor: token and head strides, positive multiples of 8, 32-bit offsets inside a 256-row block
int check_strides_varlen(const char *which, int64_t n_heads, int64_t ss, int64_t hs) {
    return check_strides(which, 1, n_heads, 0, ss, hs);
}

// every grid of a varlen launch: (sequences * heads * parts) workgroups per 128-row block of max_seqlen
int varlen_grid_check(const fa_varlen_layout *vl, int64_t heads_times_parts) {
    const int64_t blocks = (vl->max_seqlen + 127) / 128;
    if (heads_times_parts > INT32_MAX || vl->n_seqs * heads_times_parts > INT32_MAX || vl->n_seqs * heads_times_parts * blocks > INT32_MAX)
        return fail(FA_ERR_SHAPE, "problem too large for a 1-D grid");
    return FA_OK;
}

const fa::KernelEntry *varlen_entry(const fa_fwd_config *cfg, const char **why) {
    Want w;
    w.masked = true;
    w.ragged = true;
    const fa::KernelEntry *e = find_kernel(cfg, why, w);
    if (e && !(e->rows_per_wave == 32 && e->n_waves == 4 && e->B_c == 64 && e->pipelined && e->async_copy && e->swizzled && e->eager &&
               e->masked == 1 && e->d_head == 128))
        e = nullptr;
    return e;
}
const char *kNoVarlen = "packed variable-length sequences are served by the (B_r 128, B_c 64, 4 warps) + buffer configuration at d_head "
                        "128 only, plain or causal, without speculative, prescaled_q and stats";

// the cache side of fa_fwd_launch_varlen_kvcache and its fp8 form (`sc`): `c` already holds kv's strides and heads and vq's n_seqs,
// all validated; each struct is read once its own struct_size has passed
int kvcache_validate(CacheView &c, const fa_kvcache_layout *kc, const fa_kvcache_fp8_scales *sc) {
    if (kc->struct_size < sizeof(fa_kvcache_layout))
        return fail(FA_ERR_SHAPE, "fa_kvcache_layout.struct_size (%u) is smaller than this library's (%zu)", kc->struct_size,
                    sizeof(fa_kvcache_layout));
    cache_geometry(c, *kc);
    c.max_seqlen_k = kc->max_seqlen_k;
    c.words_4b = "cache_seqlens and block_table";
    if (!c.cache_seqlens) return fail(FA_ERR_NULL, "cache_seqlens is null: a DEVICE pointer to n_seqs int32 lengths is needed");
    int rc = cache_sizes(c);
    if (rc != FA_OK) return rc;
    // (the two rules only this path has, where it has always asked them: its kernel keeps the table's stride in 32 bits, and its
    // contiguous cache has a batch size of its own to compare)
    if (c.paged() && c.block_table_stride > INT32_MAX / 2) return fail(FA_ERR_SHAPE, "cache too large: lengths are 32-bit");
    if (!c.paged() && kc->batch != c.entries)
        return fail(FA_ERR_SHAPE, "a contiguous cache needs one batch entry per sequence: batch (%lld) must equal n_seqs (%lld)",
                    (long long)kc->batch, (long long)c.entries);
    if ((rc = cache_bounds(c)) != FA_OK) return rc;
    // (the token and head strides passed the packed tensors' rules in fwd_launch_varlen: what is left is the first stride)
    if (c.kv_bs < 0 || (c.slots() > 1 && c.kv_bs == 0))
        return fail(FA_ERR_SHAPE, "kv strides must be positive (the cache's %s stride is %lld elements)", c.paged() ? "page" : "batch",
                    (long long)c.kv_bs);
    if (c.kv_bs & 7) return fail(FA_ERR_ALIGN, "kv strides must be multiples of 8 elements (16 bytes)");
    if ((rc = cache_alignment(c)) != FA_OK || !sc) return rc;
    if (sc->struct_size < sizeof(fa_kvcache_fp8_scales))
        return fail(FA_ERR_SHAPE, "fa_kvcache_fp8_scales.struct_size (%u) is smaller than this library's (%zu)", sc->struct_size,
                    sizeof(fa_kvcache_fp8_scales));
    if (sc->kv_dtype != FA_KV_FP8_E4M3FN)
        return fail(FA_ERR_DTYPE, "kv_dtype (%d) is not served: the fp8 cache is e4m3fn (FA_KV_FP8_E4M3FN)", sc->kv_dtype);
    cache_descales(c, *sc);
    if ((rc = cache_descale_stride(c)) != FA_OK) return rc;
    return cache_descale_alignment(c);
}

// ---- fa_softcap: the rules of the soft-capped entry points (called behind the windowed sibling's own rules) -----------------
int softcap_validate(const fa_softcap *c) {
    if (!c) return fail(FA_ERR_NULL, "fa_softcap is null: a softcap > 0 is needed (without a cap, call the windowed entry point: this level has no \"off\")");
    if (c->struct_size < sizeof(fa_softcap))
        return fail(FA_ERR_SHAPE, "fa_softcap.struct_size (%u) is smaller than this library's (%zu)", c->struct_size, sizeof(fa_softcap));
    if (!(c->softcap > 0.0f) || !std::isfinite(c->softcap))
        return fail(FA_ERR_SHAPE, "softcap (%g) must be finite and > 0 (0 = no cap is the windowed entry point's job: this level has no \"off\")",
                    (double)c->softcap);
    return FA_OK;
}
// what the kernels take: A = softcap sqrt(d_head) and 1 / A, computed in double and rounded once (d_head = 128)
void softcap_constants(const fa_softcap *c, float *a, float *inv_a) {
    const double A = (double)c->softcap * std::sqrt(128.0);
    *a = (float)A;
    *inv_a = (float)(1.0 / A);
}

// ---- fa_sinks: the rules of the entry points with attention sinks (called behind the windowed sibling's own rules) ----------
// (`dsinks`: the backward's output, refused beside the sinks; `want_dsinks` false: the forward, which has none)
int sinks_validate(const fa_sinks *sk, int64_t n_heads, bool want_dsinks, const float *dsinks) {
    if (!sk) return fail(FA_ERR_NULL, "fa_sinks is null: one fp32 logit per query head is needed (without sinks, call the windowed entry point: this level has no \"off\")");
    if (!sk->sinks) return fail(FA_ERR_NULL, "fa_sinks.sinks is null: a device pointer to n_heads fp32 logits is needed");
    if (want_dsinks && !dsinks) return fail(FA_ERR_NULL, "dsinks is null: the backward writes the sinks' gradient, n_heads fp32, there");
    if (sk->struct_size < sizeof(fa_sinks))
        return fail(FA_ERR_SHAPE, "fa_sinks.struct_size (%u) is smaller than this library's (%zu)", sk->struct_size, sizeof(fa_sinks));
    if (sk->n_heads != n_heads)
        return fail(FA_ERR_SHAPE, "fa_sinks.n_heads (%d) does not match the call's n_heads (%lld): sinks are per query head", sk->n_heads,
                    (long long)n_heads);
    return FA_OK;
}

// the kernel of a form of the varlen forward (FA_VARLEN_FORMS), by key side, extra and dtype
const void *varlen_kernel(int keys, int extra, bool bf16, bool first_block_skip) {
#define FA_X(KEYS, EXTRA, SFX)          \
    if (keys == KEYS && extra == EXTRA) \
        return bf16 ? (const void *)fa::varlen##SFX##_kernel_dt15(first_block_skip) : (const void *)fa::varlen##SFX##_kernel_dt5(first_block_skip);
    FA_VARLEN_FORMS(FA_X)
#undef FA_X
    return nullptr;
}

// What a public entry point asks of fwd_launch_varlen beyond the arguments all of them share: its name and its name for the query
// side's total (for the messages), and its form.  The form comes from the entry point, never from a pointer being null.
enum { KEYS_PACKED = 0, KEYS_CACHE = 1, KEYS_FP8_CACHE = 2 };   // fa_inst_varlen.hip's key side ...
enum { EXTRA_NONE = 0, EXTRA_WINDOW = 1, EXTRA_SOFTCAP = 2, EXTRA_SINKS = 3 };   // ... and extra
struct VarlenCall {
    const char *entry, *total;
    int keys, extra;
    const fa_varlen_layout *vk;        // KEYS_PACKED: the key side's ranges
    const fa_kvcache_layout *kc;       // a cache: its layout (vk is not used)
    const fa_kvcache_fp8_scales *sc;   // KEYS_FP8_CACHE: k, v are bytes, kv's strides count bytes, `sc` holds the descales
    const fa_window *w;                // EXTRA_WINDOW and up (null is refused, behind everything the entry itself refuses)
    const fa_softcap *cap;             // EXTRA_SOFTCAP (refused behind the window's rules)
    const fa_sinks *sinks;             // EXTRA_SINKS, KEYS_PACKED only (refused behind the window's rules)
};
int fwd_launch_varlen(const VarlenCall &call, const fa_fwd_args *args, const fa_kv_layout *kv, const fa_varlen_layout *vq,
                      const fa_fwd_opts *opts, float *lse, void *stream) {
    const bool cache_side = call.keys != KEYS_PACKED, fp8_side = call.keys == KEYS_FP8_CACHE;
    const bool windowed = call.extra != EXTRA_NONE, capped = call.extra == EXTRA_SOFTCAP;
    const bool sunk = call.extra == EXTRA_SINKS;   // (packed keys only: its one entry point)
    const fa_varlen_layout *vk = cache_side ? vq : call.vk;   // (one valid layout for the checks both launches share)
    if (!args || !kv || !vq || !vk || (cache_side && !call.kc) || (fp8_side && !call.sc)) return fail(FA_ERR_NULL, "null pointer argument");
    if (!args->q || !args->k || !args->v || !args->o) return fail(FA_ERR_NULL, "null pointer argument");
    if (!lse) return fail(FA_ERR_NULL, "lse is null: %s needs a (n_heads, %s) fp32 buffer", call.entry, call.total);
    if (args->cfg.dtype != FA_FP16 && args->cfg.dtype != FA_BF16) return fail(FA_ERR_DTYPE, "Only fp16 and bf16 are supported");
    if (kv->struct_size < sizeof(fa_kv_layout))
        return fail(FA_ERR_SHAPE, "fa_kv_layout.struct_size (%u) is smaller than this library's (%zu)", kv->struct_size, sizeof(fa_kv_layout));
    fa_fwd_opts o;
    int rc = read_opts(opts, &o);
    if (rc != FA_OK) return rc;
    if (!fa_fwd_varlen_supported(&args->cfg, opts)) return fail(FA_ERR_NO_KERNEL, "%s", kNoVarlen);
    if (args->d_head != 128)
        return fail(FA_ERR_SHAPE, "Tensor d_head (%lld) does not match kernel configuration d_head (%d)", (long long)args->d_head, 128);
    if (args->n_heads <= 0) return fail(FA_ERR_SHAPE, "n_heads must be positive");
    if ((rc = varlen_qk_validate(vq, vk)) != FA_OK) return rc;
    if (kv->n_kv_heads < 1 || kv->n_kv_heads > args->n_heads || args->n_heads % kv->n_kv_heads != 0)
        return fail(FA_ERR_SHAPE, "grouped-query attention needs n_kv_heads (%lld) to divide n_heads (%lld)", (long long)kv->n_kv_heads,
                    (long long)args->n_heads);
    if ((rc = check_strides_varlen("q", args->n_heads, args->seq_stride, args->head_stride)) != FA_OK) return rc;
    // (an fp8 cache's strides count bytes: its own alignment rule first, so that no message about elements is reached with one)
    CacheView cache;   // (kv's and vq's part now; the layout's and the scales' in kvcache_validate, behind their struct_size)
    cache.entries = vq->n_seqs;
    cache.n_kv_heads = kv->n_kv_heads;
    cache.kv_bs = kv->kv_batch_stride;
    cache.kv_ss = kv->kv_seq_stride;
    cache.kv_hs = kv->kv_head_stride;
    cache.fp8 = fp8_side;
    if ((rc = cache_fp8_strides(cache)) != FA_OK) return rc;
    if ((rc = check_strides_varlen(fp8_side ? "kv (fp8 cache: bytes for elements)" : "kv", kv->n_kv_heads, kv->kv_seq_stride, kv->kv_head_stride)) != FA_OK) return rc;
    if ((rc = varlen_grid_check(vq, args->n_heads)) != FA_OK) return rc;
    if (((uintptr_t)args->q | (uintptr_t)args->k | (uintptr_t)args->v | (uintptr_t)args->o) & 15)
        return fail(FA_ERR_ALIGN, "q, k, v, o must be 16-byte aligned");
    if ((uintptr_t)lse & 3) return fail(FA_ERR_ALIGN, "lse must be 4-byte aligned");
    if (cache_side && (rc = kvcache_validate(cache, call.kc, fp8_side ? call.sc : nullptr)) != FA_OK) return rc;
    if (windowed) {   // (the key bound: the cache's capacity, or the packed key side's max_seqlen; then the query side's)
        if ((rc = window_validate(call.w, o.causal, cache_side ? cache.capacity() : 0)) != FA_OK) return rc;
        if (!cache_side && vk->max_seqlen > kWindowMaxLen)
            return fail(FA_ERR_SHAPE, "max_seqlen_k too large for a window: at most 2^30 - 128 keys per sequence");
        if (vq->max_seqlen > kWindowMaxLen)
            return fail(FA_ERR_SHAPE, "max_seqlen_q too large for a window: at most 2^30 - 128 query rows per sequence");
    }
    if (capped && (rc = softcap_validate(call.cap)) != FA_OK) return rc;
    if (sunk && (rc = sinks_validate(call.sinks, args->n_heads, false, nullptr)) != FA_OK) return rc;
    if (vq->total_tokens == 0) {   // (no query rows: nothing to write)
        if (o.ms) *o.ms = 0.0f;
        return FA_OK;
    }
    DeviceState *dev = current_device(&rc);
    if (!dev) return rc;
    const char *why;
    const fa::KernelEntry *e = varlen_entry(&args->cfg, &why);
    // the widest arguments of each key side: every narrower form's are their first member, and the member's address is what its kernel takes
    fa::KernelArgsVarlenSoftcap pa;
    fa::KernelArgsVarlenKVCacheSoftcap c16;
    fa::KernelArgsVarlenKVCacheFp8Softcap c8;
    fa::KernelArgsVarlenKVCacheFp8 &fa8 = c8.w.a;
    fa::KernelArgsVarlenKVCache &ca = fp8_side ? fa8.c : c16.w.a;
    fa::KernelArgsVarlenQK &qa = pa.w.a;
    fa::KernelArgsVarlen &va = cache_side ? ca.v : qa.v;
    va.base.q = args->q;
    va.base.k = args->k;
    va.base.v = args->v;
    va.base.o = args->o;
    va.base.batch_stride = 0;
    va.base.seq_stride = args->seq_stride;
    va.base.head_stride = args->head_stride;
    va.base.seq_len = 0;
    va.base.n_heads = (int32_t)args->n_heads;
    va.base.n_bh = (int32_t)(vq->n_seqs * args->n_heads);
    va.base.n_q_blocks = (int32_t)((vq->max_seqlen + 127) / 128);
    va.base.n_kv_blocks = 0;
    va.base.causal = o.causal != 0;
    va.cu_seqlens = vq->cu_seqlens;
    va.lse = lse;
    va.kv_seq_stride = kv->kv_seq_stride;
    va.kv_head_stride = kv->kv_head_stride;
    va.group = (int32_t)(args->n_heads / kv->n_kv_heads);
    va.total_tokens = (int32_t)vq->total_tokens;
    va.max_seqlen = (int32_t)vq->max_seqlen;
    if (!cache_side) {
        qa.cu_seqlens_k = vk->cu_seqlens;
        qa.total_k = (int32_t)vk->total_tokens;
        qa.max_seqlen_k = (int32_t)vk->max_seqlen;
    } else {
        const int64_t cap_k = cache.capacity();
        ca.cache_seqlens = cache.cache_seqlens;
        ca.block_table = cache.block_table;
        ca.page_stride = kv->kv_batch_stride;
        ca.bt_stride = cache.paged() ? (int32_t)cache.block_table_stride : 0;
        ca.num_pages = (int32_t)cache.slots();
        ca.tiles_per_page = (int32_t)(cache.paged() ? cache.page_size / 64 : (cap_k + 63) / 64);   // (contiguous: one "page" per entry)
        ca.max_len = (int32_t)(cache.max_seqlen_k > 0 ? cache.max_seqlen_k : cap_k);
    }
    if (fp8_side) {
        fa8.k_descale = cache.k_descale;
        fa8.v_descale = cache.v_descale;
        fa8.ds_bs = cache.descale_bs;
    }
    // the window and the cap into the key side's arguments, and the member the form's kernel takes (all three at offset 0: the
    // static_asserts of fa_fwd_kernel.hpp)
    auto form_args = [&](auto &s) -> void * {
        if (!windowed) return &s.w.a;
        s.w.left = call.w->left;   // (causal as right = 0: the kernel's one rule for both)
        s.w.right = window_right(call.w, o.causal);
        if (!capped) return &s.w;
        softcap_constants(call.cap, &s.cap_a, &s.cap_inv_a);
        return &s;
    };
    void *kernel_args = fp8_side ? form_args(c8) : cache_side ? form_args(c16) : form_args(pa);
    fa::KernelArgsVarlenSinks ps;   // (the sinks form: the packed side's windowed arguments, filled above, and the pointer)
    if (sunk) {
        ps.w = pa.w;
        ps.sinks = call.sinks->sinks;
        kernel_args = &ps;
    }
    const void *fn = varlen_kernel(call.keys, call.extra, args->cfg.dtype == FA_BF16, e->softmax_mode == FA_SOFTMAX_FIRST_BLOCK_SKIP);
    const dim3 grid((unsigned)(va.base.n_bh * va.base.n_q_blocks)), block((unsigned)e->threads);
    const hipStream_t s = (hipStream_t)stream;
    return enqueue_timed([&] {
        void *params[] = {kernel_args};
        return hipLaunchKernel(fn, grid, block, params, (size_t)e->lds_bytes, s);
    }, s, o.ms);
}

// fa_bwd_varlen_args as the arguments of two ranges: its one layout on both sides
fa_bwd_varlen_qk_args both_sides(const fa_bwd_varlen_args *a) {
    fa_bwd_varlen_qk_args b;
    b.struct_size = sizeof(b);
    b.q = a->q;
    b.k = a->k;
    b.v = a->v;
    b.o = a->o;
    b.dout = a->dout;
    b.lse = a->lse;
    b.dq = a->dq;
    b.dk = a->dk;
    b.dv = a->dv;
    b.workspace = a->workspace;
    b.n_heads = a->n_heads;
    b.n_kv_heads = a->n_kv_heads;
    b.d_head = a->d_head;
    b.q_seq_stride = a->q_seq_stride;
    b.q_head_stride = a->q_head_stride;
    b.out_seq_stride = a->out_seq_stride;
    b.out_head_stride = a->out_head_stride;
    b.kv_seq_stride = a->kv_seq_stride;
    b.kv_head_stride = a->kv_head_stride;
    b.dkv_seq_stride = a->dkv_seq_stride;
    b.dkv_head_stride = a->dkv_head_stride;
    b.dtype = a->dtype;
    b.causal = a->causal;
    b.varlen = b.varlen_k = a->varlen;
    return b;
}

// the dK / dV split: bwd_dkdv_split on the key side's grid -- host-visible arguments only, never what cu_seqlens holds
int64_t bwd_varlen_split(const fa_bwd_varlen_qk_args *a) {
    return bwd_dkdv_split(a->n_heads / a->n_kv_heads, a->varlen.n_seqs * a->n_kv_heads * ((a->varlen_k.max_seqlen + 127) / 128),
                          a->causal != 0);
}
int64_t bwd_varlen_delta_bytes(const fa_bwd_varlen_qk_args *a) {   // (n_heads, total_q) fp32, rounded up to 16 bytes
    return ((int64_t)sizeof(float) * a->n_heads * a->varlen.total_tokens + 15) & ~(int64_t)15;
}

// own_key_side: the caller gave varlen_k (fa_*_varlen_qk), whose rows the reduce kernel's grid runs over
int bwd_varlen_validate(const fa_bwd_varlen_qk_args *a, bool own_key_side) {
    if (!a) return fail(FA_ERR_NULL, "null pointer argument");
    if (a->struct_size < sizeof(fa_bwd_varlen_qk_args))
        return fail(FA_ERR_SHAPE, "fa_bwd_varlen_qk_args.struct_size (%u) is smaller than this library's (%zu)", a->struct_size,
                    sizeof(fa_bwd_varlen_qk_args));
    if (a->dtype != FA_FP16 && a->dtype != FA_BF16) return fail(FA_ERR_DTYPE, "Only fp16 and bf16 are supported");
    if (a->d_head != 128) return fail(FA_ERR_SHAPE, "the backward supports d_head = 128 only (got %lld)", (long long)a->d_head);
    if (a->n_heads <= 0) return fail(FA_ERR_SHAPE, "n_heads must be positive");
    int rc = varlen_qk_validate(&a->varlen, &a->varlen_k);
    if (rc != FA_OK) return rc;
    if (a->n_kv_heads < 1 || a->n_kv_heads > a->n_heads || a->n_heads % a->n_kv_heads != 0)
        return fail(FA_ERR_SHAPE, "grouped-query attention needs n_kv_heads (%lld) to divide n_heads (%lld)", (long long)a->n_kv_heads,
                    (long long)a->n_heads);
    if ((rc = check_strides_varlen("q", a->n_heads, a->q_seq_stride, a->q_head_stride)) != FA_OK) return rc;
    if ((rc = check_strides_varlen("out", a->n_heads, a->out_seq_stride, a->out_head_stride)) != FA_OK) return rc;
    if ((rc = check_strides_varlen("kv", a->n_kv_heads, a->kv_seq_stride, a->kv_head_stride)) != FA_OK) return rc;
    if ((rc = check_strides_varlen("dkv", a->n_kv_heads, a->dkv_seq_stride, a->dkv_head_stride)) != FA_OK) return rc;
    if (a->n_heads * a->varlen.total_tokens > (int64_t)INT32_MAX * 8 ||
        (own_key_side && a->n_kv_heads * a->varlen_k.total_tokens > (int64_t)INT32_MAX / 2))
        return fail(FA_ERR_SHAPE, "problem too large for a 1-D grid");
    if ((rc = varlen_grid_check(&a->varlen, a->n_heads)) != FA_OK) return rc;
    return varlen_grid_check(&a->varlen_k, a->n_heads);   // (n_kv_heads * split <= n_heads)
}

int64_t bwd_varlen_workspace_bytes(const fa_bwd_varlen_qk_args *a, bool own_key_side) {
    const int rc = bwd_varlen_validate(a, own_key_side);
    if (rc != FA_OK) return rc;
    const int64_t split = bwd_varlen_split(a);
    return bwd_varlen_delta_bytes(a) + (split > 1 ? (int64_t)sizeof(float) * a->n_kv_heads * split * a->varlen_k.total_tokens * 2 * 128 : 0);
}

// what a backward entry point refuses before it looks at the device; in its messages `total` is its name for the query side's
// total, `workspace_fn` its workspace function
int bwd_varlen_checks(const fa_bwd_varlen_qk_args *a, bool own_key_side, const char *total, const char *workspace_fn) {
    int rc = bwd_varlen_validate(a, own_key_side);
    if (rc != FA_OK) return rc;
    if (!a->q || !a->k || !a->v || !a->o || !a->dout || !a->dq || !a->dk || !a->dv)
        return fail(FA_ERR_NULL, "null tensor pointer (q, k, v, o, dout, dq, dk and dv are all needed)");
    if (!a->lse) return fail(FA_ERR_NULL, "lse is null: the backward needs the forward's (n_heads, %s) fp32 lse", total);
    if (!a->workspace) return fail(FA_ERR_NULL, "workspace is null: allocate %s(args) bytes of device memory", workspace_fn);
    if (((uintptr_t)a->q | (uintptr_t)a->k | (uintptr_t)a->v | (uintptr_t)a->o | (uintptr_t)a->dout | (uintptr_t)a->dq |
         (uintptr_t)a->dk | (uintptr_t)a->dv) & 15)
        return fail(FA_ERR_ALIGN, "q, k, v, o, dout, dq, dk, dv must be 16-byte aligned");
    if ((uintptr_t)a->lse & 3) return fail(FA_ERR_ALIGN, "lse must be 4-byte aligned");
    if ((uintptr_t)a->workspace & 15) return fail(FA_ERR_ALIGN, "workspace must be 16-byte aligned (it holds delta and the fp32 partials of dK / dV)");
    return FA_OK;
}

// the kernels' arguments of two ranges from the host's
void bwd_varlen_fill(fa::BwdVarlenQKArgs &va, const fa_bwd_varlen_qk_args *a) {
    const int64_t split = bwd_varlen_split(a);
    va.q = (const uint16_t *)a->q;
    va.k = (const uint16_t *)a->k;
    va.v = (const uint16_t *)a->v;
    va.o = (const uint16_t *)a->o;
    va.dout = (const uint16_t *)a->dout;
    va.lse = a->lse;
    va.delta = (float *)a->workspace;
    va.dq = (uint16_t *)a->dq;
    va.dk = (uint16_t *)a->dk;
    va.dv = (uint16_t *)a->dv;
    va.cu_seqlens = a->varlen.cu_seqlens;
    va.part = split > 1 ? (float *)((char *)a->workspace + bwd_varlen_delta_bytes(a)) : nullptr;
    va.q_ss = a->q_seq_stride;
    va.q_hs = a->q_head_stride;
    va.out_ss = a->out_seq_stride;
    va.out_hs = a->out_head_stride;
    va.kv_ss = a->kv_seq_stride;
    va.kv_hs = a->kv_head_stride;
    va.dkv_ss = a->dkv_seq_stride;
    va.dkv_hs = a->dkv_head_stride;
    va.n_seqs = (int32_t)a->varlen.n_seqs;
    va.total_tokens = (int32_t)a->varlen.total_tokens;
    va.max_seqlen = (int32_t)a->varlen.max_seqlen;
    va.n_heads = (int32_t)a->n_heads;
    va.group = (int32_t)(a->n_heads / a->n_kv_heads);
    va.split = (int32_t)split;
    va.n_blocks = (int32_t)((a->varlen.max_seqlen + 127) / 128);
    va.cu_seqlens_k = a->varlen_k.cu_seqlens;
    va.total_k = (int32_t)a->varlen_k.total_tokens;
    va.max_seqlen_k = (int32_t)a->varlen_k.max_seqlen;
    va.n_blocks_k = (int32_t)((a->varlen_k.max_seqlen + 127) / 128);
}
// ... and what the kernels of one range take of them (fa::BwdVarlenArgs, in its field order)
fa::BwdVarlenArgs one_range(const fa::BwdVarlenQKArgs &w) {
    return {w.q,    w.k,    w.v,     w.o,     w.dout,  w.lse,   w.delta,  w.dq,      w.dk,           w.dv,         w.cu_seqlens, w.part,
            w.q_ss, w.q_hs, w.out_ss, w.out_hs, w.kv_ss, w.kv_hs, w.dkv_ss, w.dkv_hs, w.n_seqs,       w.total_tokens, w.max_seqlen,
            w.n_heads, w.group, w.split, w.n_blocks};
}
}  // namespace

int fa_fwd_varlen_supported(const fa_fwd_config *cfg, const fa_fwd_opts *opts) {
    if (!cfg) return 0;
    fa_fwd_opts o;
    if (read_opts(opts, &o) != FA_OK) return 0;
    if (o.speculative || o.prescaled_q || o.stats) return 0;
    if (cfg->dtype != FA_BF16 && cfg->dtype != FA_FP16) return 0;
    const char *why;
    return varlen_entry(cfg, &why) ? 1 : 0;
}
int fa_fwd_varlen_qk_supported(const fa_fwd_config *cfg, const fa_fwd_opts *opts) { return fa_fwd_varlen_supported(cfg, opts); }

int fa_fwd_launch_varlen(const fa_fwd_args *args, const fa_kv_layout *kv, const fa_varlen_layout *vl, const fa_fwd_opts *opts, float *lse,
                         void *stream) {
    return fwd_launch_varlen({"fa_fwd_launch_varlen", "total_tokens", KEYS_PACKED, EXTRA_NONE, vl}, args, kv, vl, opts, lse, stream);
}
int fa_fwd_launch_varlen_qk(const fa_fwd_args *args, const fa_kv_layout *kv, const fa_varlen_layout *vq, const fa_varlen_layout *vk,
                            const fa_fwd_opts *opts, float *lse, void *stream) {
    return fwd_launch_varlen({"fa_fwd_launch_varlen_qk", "total_q", KEYS_PACKED, EXTRA_NONE, vk}, args, kv, vq, opts, lse, stream);
}

int fa_fwd_varlen_kvcache_supported(const fa_fwd_config *cfg, const fa_fwd_opts *opts) { return fa_fwd_varlen_supported(cfg, opts); }

int fa_fwd_launch_varlen_kvcache(const fa_fwd_args *args, const fa_kv_layout *kv, const fa_varlen_layout *vq, const fa_kvcache_layout *kc,
                                 const fa_fwd_opts *opts, float *lse, void *stream) {
    return fwd_launch_varlen({"fa_fwd_launch_varlen_kvcache", "total_q", KEYS_CACHE, EXTRA_NONE, nullptr, kc}, args, kv, vq, opts, lse, stream);
}

int fa_fwd_varlen_kvcache_fp8_supported(const fa_fwd_config *cfg, const fa_fwd_opts *opts) { return fa_fwd_varlen_supported(cfg, opts); }

int fa_fwd_launch_varlen_kvcache_fp8(const fa_fwd_args *args, const fa_kv_layout *kv, const fa_varlen_layout *vq, const fa_kvcache_layout *kc,
                                     const fa_kvcache_fp8_scales *sc, const fa_fwd_opts *opts, float *lse, void *stream) {
    return fwd_launch_varlen({"fa_fwd_launch_varlen_kvcache_fp8", "total_q", KEYS_FP8_CACHE, EXTRA_NONE, nullptr, kc, sc}, args, kv, vq, opts, lse, stream);
}

// the sliding-window forms of the three: the same body with an fa_window (served: what the sibling serves)
int fa_fwd_varlen_qk_window_supported(const fa_fwd_config *cfg, const fa_fwd_opts *opts) { return fa_fwd_varlen_supported(cfg, opts); }
int fa_fwd_launch_varlen_qk_window(const fa_fwd_args *args, const fa_kv_layout *kv, const fa_varlen_layout *vq, const fa_varlen_layout *vk,
                                   const fa_window *w, const fa_fwd_opts *opts, float *lse, void *stream) {
    return fwd_launch_varlen({"fa_fwd_launch_varlen_qk_window", "total_q", KEYS_PACKED, EXTRA_WINDOW, vk, nullptr, nullptr, w}, args, kv, vq, opts, lse, stream);
}
// ... with logit soft-capping: the windowed packed body with an fa_softcap behind the window (served: what the sibling serves)
int fa_fwd_varlen_qk_softcap_supported(const fa_fwd_config *cfg, const fa_fwd_opts *opts) { return fa_fwd_varlen_supported(cfg, opts); }
int fa_fwd_launch_varlen_qk_softcap(const fa_fwd_args *args, const fa_kv_layout *kv, const fa_varlen_layout *vq, const fa_varlen_layout *vk,
                                    const fa_window *w, const fa_softcap *cap, const fa_fwd_opts *opts, float *lse, void *stream) {
    return fwd_launch_varlen({"fa_fwd_launch_varlen_qk_softcap", "total_q", KEYS_PACKED, EXTRA_SOFTCAP, vk, nullptr, nullptr, w, cap}, args, kv, vq, opts,
                             lse, stream);
}
int fa_fwd_varlen_kvcache_window_supported(const fa_fwd_config *cfg, const fa_fwd_opts *opts) { return fa_fwd_varlen_supported(cfg, opts); }
int fa_fwd_launch_varlen_kvcache_window(const fa_fwd_args *args, const fa_kv_layout *kv, const fa_varlen_layout *vq,
                                        const fa_kvcache_layout *kc, const fa_window *w, const fa_fwd_opts *opts, float *lse, void *stream) {
    return fwd_launch_varlen({"fa_fwd_launch_varlen_kvcache_window", "total_q", KEYS_CACHE, EXTRA_WINDOW, nullptr, kc, nullptr, w}, args, kv, vq, opts,
                             lse, stream);
}
int fa_fwd_varlen_kvcache_fp8_window_supported(const fa_fwd_config *cfg, const fa_fwd_opts *opts) { return fa_fwd_varlen_supported(cfg, opts); }
int fa_fwd_launch_varlen_kvcache_fp8_window(const fa_fwd_args *args, const fa_kv_layout *kv, const fa_varlen_layout *vq,
                                            const fa_kvcache_layout *kc, const fa_kvcache_fp8_scales *sc, const fa_window *w,
                                            const fa_fwd_opts *opts, float *lse, void *stream) {
    return fwd_launch_varlen({"fa_fwd_launch_varlen_kvcache_fp8_window", "total_q", KEYS_FP8_CACHE, EXTRA_WINDOW, nullptr, kc, sc, w}, args, kv, vq, opts,
                             lse, stream);
}
// ... with attention sinks: the windowed packed body with an fa_sinks behind the window (served: what the sibling serves)
int fa_fwd_varlen_qk_sinks_supported(const fa_fwd_config *cfg, const fa_fwd_opts *opts) { return fa_fwd_varlen_supported(cfg, opts); }
int fa_fwd_launch_varlen_qk_sinks(const fa_fwd_args *args, const fa_kv_layout *kv, const fa_varlen_layout *vq, const fa_varlen_layout *vk,
                                  const fa_window *w, const fa_sinks *sinks, const fa_fwd_opts *opts, float *lse, void *stream) {
    return fwd_launch_varlen({"fa_fwd_launch_varlen_qk_sinks", "total_q", KEYS_PACKED, EXTRA_SINKS, vk, nullptr, nullptr, w, nullptr, sinks}, args, kv, vq,
                             opts, lse, stream);
}
// ... and both windowed cache prefills with logit soft-capping: an fa_softcap behind the window (served: what the sibling serves)
int fa_fwd_varlen_kvcache_softcap_supported(const fa_fwd_config *cfg, const fa_fwd_opts *opts) { return fa_fwd_varlen_supported(cfg, opts); }
int fa_fwd_launch_varlen_kvcache_softcap(const fa_fwd_args *args, const fa_kv_layout *kv, const fa_varlen_layout *vq,
                                         const fa_kvcache_layout *kc, const fa_window *w, const fa_softcap *cap, const fa_fwd_opts *opts,
                                         float *lse, void *stream) {
    return fwd_launch_varlen({"fa_fwd_launch_varlen_kvcache_softcap", "total_q", KEYS_CACHE, EXTRA_SOFTCAP, nullptr, kc, nullptr, w, cap}, args, kv, vq,
                             opts, lse, stream);
}
int fa_fwd_varlen_kvcache_fp8_softcap_supported(const fa_fwd_config *cfg, const fa_fwd_opts *opts) { return fa_fwd_varlen_supported(cfg, opts); }
int fa_fwd_launch_varlen_kvcache_fp8_softcap(const fa_fwd_args *args, const fa_kv_layout *kv, const fa_varlen_layout *vq,
                                             const fa_kvcache_layout *kc, const fa_kvcache_fp8_scales *sc, const fa_window *w,
                                             const fa_softcap *cap, const fa_fwd_opts *opts, float *lse, void *stream) {
    return fwd_launch_varlen({"fa_fwd_launch_varlen_kvcache_fp8_softcap", "total_q", KEYS_FP8_CACHE, EXTRA_SOFTCAP, nullptr, kc, sc, w, cap}, args, kv, vq,
                             opts, lse, stream);
}

int64_t fa_bwd_varlen_workspace_bytes(const fa_bwd_varlen_args *a) {
    if (!a) return fail(FA_ERR_NULL, "null pointer argument");
    const fa_bwd_varlen_qk_args b = both_sides(a);
    return bwd_varlen_workspace_bytes(&b, false);
}
int64_t fa_bwd_varlen_qk_workspace_bytes(const fa_bwd_varlen_qk_args *a) { return bwd_varlen_workspace_bytes(a, true); }

int fa_bwd_launch_varlen(const fa_bwd_varlen_args *args, void *stream, float *ms) {
    if (!args) return fail(FA_ERR_NULL, "null pointer argument");
    const fa_bwd_varlen_qk_args b = both_sides(args), *a = &b;
    int rc = bwd_varlen_checks(a, false, "total_tokens", "fa_bwd_varlen_workspace_bytes");
    if (rc != FA_OK) return rc;
    if (a->varlen.total_tokens == 0) {
        if (ms) *ms = 0.0f;
        return FA_OK;
    }
    DeviceState *dev = current_device(&rc);
    if (!dev) return rc;
    fa::BwdVarlenQKArgs both;
    bwd_varlen_fill(both, a);
    const fa::BwdVarlenArgs va = one_range(both);
    const hipStream_t s = (hipStream_t)stream;
    return enqueue_timed([&] { return fa::bwd_varlen_enqueue(va, a->dtype, a->causal != 0, s); }, s, ms);
}

int fa_bwd_launch_varlen_qk(const fa_bwd_varlen_qk_args *a, void *stream, float *ms) {
    int rc = bwd_varlen_checks(a, true, "total_q", "fa_bwd_varlen_qk_workspace_bytes");
    if (rc != FA_OK) return rc;
    if (a->varlen.total_tokens == 0 && a->varlen_k.total_tokens == 0) {
        if (ms) *ms = 0.0f;
        return FA_OK;
    }
    DeviceState *dev = current_device(&rc);
    if (!dev) return rc;
    fa::BwdVarlenQKArgs va;
    bwd_varlen_fill(va, a);
    const hipStream_t s = (hipStream_t)stream;
    return enqueue_timed([&] { return fa::bwd_varlen_qk_enqueue(va, a->dtype, a->causal != 0, s); }, s, ms);
}

// the sliding-window form: the sibling's checks, then the window's (the forward's: fwd_launch_varlen); split, workspace and the
// argument fill are the sibling's, the kernels take (left, right) with -1 as 2^30 and causal as right = 0
// `capped`: fa_bwd_launch_varlen_qk_softcap -- its fa_softcap `cap` refused behind the window's rules, and the soft-capped kernels
static int bwd_launch_varlen_window(const fa_bwd_varlen_qk_args *a, const fa_window *w, bool capped, const fa_softcap *cap, void *stream,
                                    float *ms) {
    int rc = bwd_varlen_checks(a, true, "total_q", "fa_bwd_varlen_qk_workspace_bytes");
    if (rc != FA_OK) return rc;
    if ((rc = window_validate(w, a->causal, 0)) != FA_OK) return rc;
    if (a->varlen_k.max_seqlen > kWindowMaxLen)
        return fail(FA_ERR_SHAPE, "max_seqlen_k too large for a window: at most 2^30 - 128 keys per sequence");
    if (a->varlen.max_seqlen > kWindowMaxLen)
        return fail(FA_ERR_SHAPE, "max_seqlen_q too large for a window: at most 2^30 - 128 query rows per sequence");
    if (capped && (rc = softcap_validate(cap)) != FA_OK) return rc;
    if (a->varlen.total_tokens == 0 && a->varlen_k.total_tokens == 0) {
        if (ms) *ms = 0.0f;
        return FA_OK;
    }
    DeviceState *dev = current_device(&rc);
    if (!dev) return rc;
    fa::BwdVarlenSoftcapArgs ca;   // (the wider form: the window form's arguments are its base)
    fa::BwdVarlenWindowArgs &va = ca;
    bwd_varlen_fill(va, a);
    constexpr int32_t kFar = 1 << 30;   // unbounded: beyond every position (kWindowMaxLen), and p - kFar, p + kFar fit 32 bits
    const int32_t right = window_right(w, a->causal);
    va.left = w->left < 0 || w->left > kFar ? kFar : w->left;
    va.right = right < 0 || right > kFar ? kFar : right;
    const hipStream_t s = (hipStream_t)stream;
    if (capped) {
        softcap_constants(cap, &ca.cap_a, &ca.cap_inv_a);
        return enqueue_timed([&] { return fa::bwd_varlen_softcap_enqueue(ca, a->dtype, s); }, s, ms);
    }
    return enqueue_timed([&] { return fa::bwd_varlen_window_enqueue(va, a->dtype, s); }, s, ms);
}
int fa_bwd_launch_varlen_qk_window(const fa_bwd_varlen_qk_args *a, const fa_window *w, void *stream, float *ms) {
    return bwd_launch_varlen_window(a, w, false, nullptr, stream, ms);
}
// ... with logit soft-capping: the sibling's checks and the window's, then the cap's
int fa_bwd_launch_varlen_qk_softcap(const fa_bwd_varlen_qk_args *a, const fa_window *w, const fa_softcap *cap, void *stream, float *ms) {
    return bwd_launch_varlen_window(a, w, true, cap, stream, ms);
}
// ... with attention sinks: the sibling's checks and the window's, then the sinks'.  The kernels are the window form's (the
// forward's lse holds the sink; fa_bwd_varlen.hpp), and one more reduces lse and the workspace's delta to dsinks.  No partials: the
// workspace is the sibling's.  (No query rows but key rows: the window form writes the zeros of dK / dV and dsinks is written, as zeros.)
int64_t fa_bwd_varlen_qk_sinks_workspace_bytes(const fa_bwd_varlen_qk_args *a) { return bwd_varlen_workspace_bytes(a, true); }
int fa_bwd_launch_varlen_qk_sinks(const fa_bwd_varlen_qk_args *a, const fa_window *w, const fa_sinks *sinks, float *dsinks, void *stream, float *ms) {
    int rc = bwd_varlen_checks(a, true, "total_q", "fa_bwd_varlen_qk_workspace_bytes");
    if (rc != FA_OK) return rc;
    if ((rc = window_validate(w, a->causal, 0)) != FA_OK) return rc;
    if (a->varlen_k.max_seqlen > kWindowMaxLen)
        return fail(FA_ERR_SHAPE, "max_seqlen_k too large for a window: at most 2^30 - 128 keys per sequence");
    if (a->varlen.max_seqlen > kWindowMaxLen)
        return fail(FA_ERR_SHAPE, "max_seqlen_q too large for a window: at most 2^30 - 128 query rows per sequence");
    if ((rc = sinks_validate(sinks, a->n_heads, true, dsinks)) != FA_OK) return rc;
    if (a->varlen.total_tokens == 0 && a->varlen_k.total_tokens == 0) {   // (like the sibling: no device, nothing written)
        if (ms) *ms = 0.0f;
        return FA_OK;
    }
    DeviceState *dev = current_device(&rc);
    if (!dev) return rc;
    fa::BwdVarlenSinksArgs sa;
    bwd_varlen_fill(sa.w, a);
    constexpr int32_t kFar = 1 << 30;   // (as in bwd_launch_varlen_window)
    const int32_t right = window_right(w, a->causal);
    sa.w.left = w->left < 0 || w->left > kFar ? kFar : w->left;
    sa.w.right = right < 0 || right > kFar ? kFar : right;
    sa.sinks = sinks->sinks;
    sa.dsinks = dsinks;
    const hipStream_t s = (hipStream_t)stream;
    return enqueue_timed([&] { return fa::bwd_varlen_sinks_enqueue(sa, a->dtype, s); }, s, ms);
}

// ---- KV-cache decode ------------------------------------------------------------------------------------------------------
// fa_decode_args and fa_decode_fp8_args carry the same members under the same names (the fp8 struct adds its encoding and
// descales), so one text over either struct serves the twenty-two entry points: a planner (validate, then the split count) for the
// sixteen queries and one launch body for the six launches (the soft-capped forms: four queries, two launches).  What only one struct has sits in the two decode_struct_rules.
namespace {
extern "C++" {   // (as for the cache's rules above; the two overloads need it as well)
constexpr int64_t kDecodeMaxRows = 64, kDecodeWantWgs = 256, kDecodeKeysPerSplit = 256, kDecodeMaxSplits = 128, kDecodeMaxForced = 1024;

int decode_struct_rules(const fa_decode_args *a, CacheView &) {
    if (a->struct_size < sizeof(fa_decode_args))
        return fail(FA_ERR_SHAPE, "fa_decode_args.struct_size (%u) is smaller than this library's (%zu)", a->struct_size, sizeof(fa_decode_args));
    return FA_OK;
}
int decode_struct_rules(const fa_decode_fp8_args *a, CacheView &c) {
    if (a->struct_size < sizeof(fa_decode_fp8_args))
        return fail(FA_ERR_SHAPE, "fa_decode_fp8_args.struct_size (%u) is smaller than this library's (%zu)", a->struct_size,
                    sizeof(fa_decode_fp8_args));
    if (a->kv_dtype != FA_KV_FP8_E4M3FN)
        return fail(FA_ERR_DTYPE, "kv_dtype (%d) is not served: the fp8 cache is e4m3fn (FA_KV_FP8_E4M3FN)", a->kv_dtype);
    c.fp8 = true;
    cache_descales(c, *a);
    return FA_OK;
}

struct DecodePlan {
    int status = FA_OK;
    int64_t splits = 0;
    CacheView cache;
};
int plan_splits(const DecodePlan &p) { return p.status != FA_OK ? p.status : (int)p.splits; }

// everything but the pointers' values: dtype, kernel, sizes, strides -- in the order of the statuses' numbers; fills `c`
template <class A> int decode_validate(const A *a, CacheView &c) {
    if (!a) return fail(FA_ERR_NULL, "null pointer argument");
    int rc = decode_struct_rules(a, c);
    if (rc != FA_OK) return rc;
    if (a->dtype != FA_FP16 && a->dtype != FA_BF16) return fail(FA_ERR_DTYPE, "Only fp16 and bf16 are supported");
    if (a->d_head != 128) return fail(FA_ERR_SHAPE, "decode supports d_head = 128 only (got %lld)", (long long)a->d_head);
    if (a->batch < 0 || a->seqlen_q <= 0 || a->n_heads <= 0) return fail(FA_ERR_SHAPE, "batch must not be negative, seqlen_q and n_heads must be positive");
    if (a->batch > INT32_MAX / 2 || a->n_heads > INT32_MAX / 2) return fail(FA_ERR_SHAPE, "problem too large for a 1-D grid");
    if (a->n_kv_heads < 1 || a->n_kv_heads > a->n_heads || a->n_heads % a->n_kv_heads != 0)
        return fail(FA_ERR_SHAPE, "grouped-query attention needs n_kv_heads (%lld) to divide n_heads (%lld)", (long long)a->n_kv_heads,
                    (long long)a->n_heads);
    const int64_t group = a->n_heads / a->n_kv_heads;
    if (a->seqlen_q > kDecodeMaxRows || a->seqlen_q * group > kDecodeMaxRows)
        return fail(FA_ERR_NO_KERNEL, "decode serves seqlen_q * (n_heads / n_kv_heads) <= 64 packed query rows (got %lld * %lld): use the "
                                      "forward entry points for longer queries", (long long)a->seqlen_q, (long long)group);
    cache_tensors(c, *a);
    c.max_seqlen_k = a->max_seqlen_k;
    c.words_4b = "cache_seqlens, block_table and lse";
    if ((rc = cache_sizes(c)) != FA_OK || (rc = cache_bounds(c)) != FA_OK) return rc;
    if (a->num_splits < 0 || a->num_splits > kDecodeMaxForced)
        return fail(FA_ERR_SHAPE, "num_splits (%d) must lie in [0, %lld] (0 = the split rule)", a->num_splits, (long long)kDecodeMaxForced);
    if ((rc = stride_set("q", 8, a->batch, a->seqlen_q, a->n_heads, a->q_batch_stride, a->q_seq_stride, a->q_head_stride)) != FA_OK) return rc;
    if ((rc = stride_set("o", 8, a->batch, a->seqlen_q, a->n_heads, a->o_batch_stride, a->o_seq_stride, a->o_head_stride)) != FA_OK) return rc;
    if ((rc = cache_strides(c, 8)) != FA_OK) return rc;
    if (a->batch * a->n_kv_heads * kDecodeMaxForced > INT32_MAX || a->batch * a->n_heads * a->seqlen_q > INT32_MAX)
        return fail(FA_ERR_SHAPE, "problem too large for a 1-D grid");
    if ((rc = cache_descale_stride(c)) != FA_OK) return rc;   // (the fp8 side's two: nothing to refuse in a 16-bit cache)
    return cache_fp8_strides(c);
}

// The split rule: a pure function of batch, n_kv_heads and the host's key bound.  The smallest power of two that gives
// the grid one workgroup per CU of an MI355X (256, the count the GQA backward's split uses), while a split keeps at
// least 256 keys of the bound, at most 128.  With a window the bound is the keys a workgroup can visit, left + seqlen_q +
// right, when both sides are bounded (and that is less).
template <class A> int64_t decode_splits(const A *a, const CacheView &c, const fa_window *w) {
    if (a->num_splits > 0) return a->num_splits;
    int64_t max_k = c.max_seqlen_k > 0 ? c.max_seqlen_k : c.capacity();
    if (w && w->left >= 0 && window_right(w, a->causal) >= 0) {
        const int64_t span = (int64_t)w->left + a->seqlen_q + window_right(w, a->causal);
        max_k = span < max_k ? span : max_k;
    }
    int64_t s = 1;
    while (a->batch * a->n_kv_heads * s < kDecodeWantWgs && s < kDecodeMaxSplits) s *= 2;
    const int64_t by_keys = (max_k + kDecodeKeysPerSplit - 1) / kDecodeKeysPerSplit;
    return s < by_keys ? s : (by_keys < 1 ? 1 : by_keys);
}

// The planner of every decode entry point: the arguments (either struct) and, for a window form, its fa_window (null is refused
// there) -> status, split count and the cache as validated.  `capped`: a soft-capped form, its fa_softcap refused behind the
// window's rules; the cap does not enter the split rule.
template <class A> DecodePlan decode_plan(const A *a, bool windowed, const fa_window *w, bool capped = false, const fa_softcap *cap = nullptr) {
    DecodePlan p;
    p.status = decode_validate(a, p.cache);
    if (p.status == FA_OK && windowed) p.status = window_validate(w, a->causal, p.cache.capacity());
    if (p.status == FA_OK && capped) p.status = softcap_validate(cap);
    if (p.status == FA_OK) p.splits = decode_splits(a, p.cache, windowed ? w : nullptr);
    return p;
}

template <class A> int64_t decode_part_o_bytes(const A *a, int64_t splits) {
    return (int64_t)sizeof(float) * splits * a->batch * a->n_kv_heads * (a->seqlen_q * (a->n_heads / a->n_kv_heads)) * 128;
}

// the workspace of a plan: the fp32 partial o (a multiple of 512 bytes), then the partial lse; none for one split
template <class A> int64_t plan_workspace(const A *a, const DecodePlan &p) {
    if (p.status != FA_OK) return p.status;
    if (p.splits == 1) return 0;
    const int64_t po = decode_part_o_bytes(a, p.splits);
    return po + ((po / 128 + 15) & ~(int64_t)15);
}

// the kernels' arguments from validated ones
template <class A> void decode_fill(fa::DecodeArgs &d, const A *a, const CacheView &c, int64_t splits) {
    d.q = (const uint16_t *)a->q;
    d.k = (const uint16_t *)a->k;
    d.v = (const uint16_t *)a->v;
    d.o = (uint16_t *)a->o;
    d.lse = a->lse;
    d.cache_seqlens = c.cache_seqlens;
    d.block_table = c.block_table;
    d.part_o = splits > 1 ? (float *)a->workspace : nullptr;
    d.part_lse = splits > 1 ? (float *)((char *)a->workspace + decode_part_o_bytes(a, splits)) : nullptr;
    d.q_bs = a->q_batch_stride;
    d.q_ss = a->q_seq_stride;
    d.q_hs = a->q_head_stride;
    d.o_bs = a->o_batch_stride;
    d.o_ss = a->o_seq_stride;
    d.o_hs = a->o_head_stride;
    d.kv_bs = c.kv_bs;
    d.kv_ss = c.kv_ss;
    d.kv_hs = c.kv_hs;
    d.bt_bs = c.paged() ? c.block_table_stride : 0;
    d.batch = (int32_t)a->batch;
    d.seqlen_q = (int32_t)a->seqlen_q;
    d.n_heads = (int32_t)a->n_heads;
    d.n_kv_heads = (int32_t)a->n_kv_heads;
    d.group = (int32_t)(a->n_heads / a->n_kv_heads);
    d.rows = d.seqlen_q * d.group;
    d.max_len = (int32_t)c.capacity();
    d.page_size = c.paged() ? (int32_t)c.page_size : 0;
    d.num_pages = c.paged() ? (int32_t)c.num_pages : 0;
    d.num_splits = (int32_t)splits;
    d.causal = a->causal != 0;
}

// The launch of all six forms; `ws_query`: the entry point's workspace query (a capped form: its windowed sibling's), for its message.  `capped`: a soft-capped form (always
// windowed), its fa_softcap refused behind everything the windowed sibling refuses.
template <class A>
int decode_launch(const A *a, bool windowed, const fa_window *w, const char *ws_query, void *stream, float *ms, bool capped = false,
                  const fa_softcap *cap = nullptr) {
    if (!a) return fail(FA_ERR_NULL, "null pointer argument");
    if (!a->q || !a->k || !a->v || !a->o) return fail(FA_ERR_NULL, "null tensor pointer (q, k, v and o are all needed)");
    if (!a->cache_seqlens) return fail(FA_ERR_NULL, "cache_seqlens is null: a DEVICE pointer to batch int32 lengths is needed");
    const DecodePlan p = decode_plan(a, windowed, w);
    if (p.status != FA_OK) return p.status;
    if (a->batch == 0) {   // (nothing to do -- behind the cap's own rules, as in the packed form)
        if (capped && softcap_validate(cap) != FA_OK) return softcap_validate(cap);
        if (ms) *ms = 0.0f;
        return FA_OK;
    }
    const CacheView &c = p.cache;
    if (p.splits > 1 && !a->workspace)
        return fail(FA_ERR_NULL, "workspace is null: allocate %s(%s) bytes of device memory", ws_query, windowed ? "args, window" : "args");
    if (((uintptr_t)a->q | (uintptr_t)a->k | (uintptr_t)a->v | (uintptr_t)a->o) & 15) return fail(FA_ERR_ALIGN, "q, k, v, o must be 16-byte aligned");
    int rc = cache_alignment(c, (uintptr_t)a->lse);
    if (rc != FA_OK) return rc;
    // (fa_decode_fp8_launch asks the descales' alignment in front of the workspace's, its window form behind it: both orders kept)
    if (!windowed && (rc = cache_descale_alignment(c)) != FA_OK) return rc;
    if (p.splits > 1 && ((uintptr_t)a->workspace & 15)) return fail(FA_ERR_ALIGN, "workspace must be 16-byte aligned (it holds the splits' fp32 partials)");
    if (windowed && (rc = cache_descale_alignment(c)) != FA_OK) return rc;
    if (capped && (rc = softcap_validate(cap)) != FA_OK) return rc;
    DeviceState *dev = current_device(&rc);
    if (!dev) return rc;
    fa::DecodeFp8WindowArgs k;   // (the widest form: the other three's arguments are its members)
    decode_fill(k.f.d, a, c, p.splits);
    k.f.k_descale = c.k_descale;
    k.f.v_descale = c.v_descale;
    k.f.ds_bs = c.descale_bs;
    k.left = windowed ? w->left : -1;
    k.right = windowed ? window_right(w, a->causal) : -1;
    const fa::DecodeWindowArgs kw = {k.f.d, k.left, k.right};
    fa::DecodeSoftcapArgs ks = {kw, 0.0f, 0.0f};
    fa::DecodeFp8SoftcapArgs ks8 = {k, 0.0f, 0.0f};
    if (capped) {
        softcap_constants(cap, &ks.cap_a, &ks.cap_inv_a);
        ks8.cap_a = ks.cap_a;
        ks8.cap_inv_a = ks.cap_inv_a;
    }
    const hipStream_t s = (hipStream_t)stream;
    return enqueue_timed([&] {
        if (capped) return c.fp8 ? fa::decode_fp8_softcap_enqueue(ks8, a->dtype, s) : fa::decode_softcap_enqueue(ks, a->dtype, s);
        if (c.fp8) return windowed ? fa::decode_fp8_window_enqueue(k, a->dtype, s) : fa::decode_fp8_enqueue(k.f, a->dtype, s);
        return windowed ? fa::decode_window_enqueue(kw, a->dtype, s) : fa::decode_enqueue(k.f.d, a->dtype, s);
    }, s, ms);
}
}
}  // namespace

int fa_decode_supported(const fa_decode_args *a) { return decode_plan(a, false, nullptr).status == FA_OK; }
int fa_decode_num_splits(const fa_decode_args *a) { return plan_splits(decode_plan(a, false, nullptr)); }
int64_t fa_decode_workspace_bytes(const fa_decode_args *a) { return plan_workspace(a, decode_plan(a, false, nullptr)); }
int fa_decode_launch(const fa_decode_args *a, void *stream, float *ms) {
    return decode_launch(a, false, nullptr, "fa_decode_workspace_bytes", stream, ms);
}

int fa_decode_fp8_supported(const fa_decode_fp8_args *a) { return decode_plan(a, false, nullptr).status == FA_OK; }
int fa_decode_fp8_num_splits(const fa_decode_fp8_args *a) { return plan_splits(decode_plan(a, false, nullptr)); }
int64_t fa_decode_fp8_workspace_bytes(const fa_decode_fp8_args *a) { return plan_workspace(a, decode_plan(a, false, nullptr)); }
int fa_decode_fp8_launch(const fa_decode_fp8_args *a, void *stream, float *ms) {
    return decode_launch(a, false, nullptr, "fa_decode_fp8_workspace_bytes", stream, ms);
}

int fa_decode_window_supported(const fa_decode_args *a, const fa_window *w) { return decode_plan(a, true, w).status == FA_OK; }
int fa_decode_window_num_splits(const fa_decode_args *a, const fa_window *w) { return plan_splits(decode_plan(a, true, w)); }
int64_t fa_decode_window_workspace_bytes(const fa_decode_args *a, const fa_window *w) { return plan_workspace(a, decode_plan(a, true, w)); }
int fa_decode_window_launch(const fa_decode_args *a, const fa_window *w, void *stream, float *ms) {
    return decode_launch(a, true, w, "fa_decode_window_workspace_bytes", stream, ms);
}

int fa_decode_fp8_window_supported(const fa_decode_fp8_args *a, const fa_window *w) { return decode_plan(a, true, w).status == FA_OK; }
int fa_decode_fp8_window_num_splits(const fa_decode_fp8_args *a, const fa_window *w) { return plan_splits(decode_plan(a, true, w)); }
int64_t fa_decode_fp8_window_workspace_bytes(const fa_decode_fp8_args *a, const fa_window *w) { return plan_workspace(a, decode_plan(a, true, w)); }
int fa_decode_fp8_window_launch(const fa_decode_fp8_args *a, const fa_window *w, void *stream, float *ms) {
    return decode_launch(a, true, w, "fa_decode_fp8_window_workspace_bytes", stream, ms);
}

// ... with logit soft-capping: the windowed forms with an fa_softcap behind the window.  The split count is the windowed entry's for
// the same arguments, and so is the workspace: no workspace query of their own (as the soft-capped backward has none), the launch is
// sized by fa_decode_window_workspace_bytes / fa_decode_fp8_window_workspace_bytes.
int fa_decode_softcap_supported(const fa_decode_args *a, const fa_window *w, const fa_softcap *cap) {
    return decode_plan(a, true, w, true, cap).status == FA_OK;
}
int fa_decode_softcap_num_splits(const fa_decode_args *a, const fa_window *w, const fa_softcap *cap) {
    return plan_splits(decode_plan(a, true, w, true, cap));
}
int fa_decode_softcap_launch(const fa_decode_args *a, const fa_window *w, const fa_softcap *cap, void *stream, float *ms) {
    return decode_launch(a, true, w, "fa_decode_window_workspace_bytes", stream, ms, true, cap);
}

int fa_decode_fp8_softcap_supported(const fa_decode_fp8_args *a, const fa_window *w, const fa_softcap *cap) {
    return decode_plan(a, true, w, true, cap).status == FA_OK;
}
int fa_decode_fp8_softcap_num_splits(const fa_decode_fp8_args *a, const fa_window *w, const fa_softcap *cap) {
    return plan_splits(decode_plan(a, true, w, true, cap));
}
int fa_decode_fp8_softcap_launch(const fa_decode_fp8_args *a, const fa_window *w, const fa_softcap *cap, void *stream, float *ms) {
    return decode_launch(a, true, w, "fa_decode_fp8_window_workspace_bytes", stream, ms, true, cap);
}

// ---- the KV-cache append in front of a decode --------------------------------------------------------------------------------
namespace {
// the bytes [p, p + extent) a (n0, n1, n2, 128) tensor of 16-bit elements spans
int64_t append_extent(int64_t n0, int64_t n1, int64_t n2, int64_t bs, int64_t ss, int64_t hs) {
    return 2 * ((n0 - 1) * bs + (n1 - 1) * ss + (n2 - 1) * hs + 128);
}

// fills `c` once the struct's size has passed
int append_validate(const fa_kvcache_append_args *a, CacheView &c) {
    if (!a) return fail(FA_ERR_NULL, "null pointer argument");
    if (a->struct_size < sizeof(fa_kvcache_append_args))
        return fail(FA_ERR_SHAPE, "fa_kvcache_append_args.struct_size (%u) is smaller than this library's (%zu)", a->struct_size,
                    sizeof(fa_kvcache_append_args));
    if (!a->k || !a->v) return fail(FA_ERR_NULL, "null cache pointer (k and v are both needed)");
    if (a->seqlen_new > 0 && (!a->k_new || !a->v_new)) return fail(FA_ERR_NULL, "null new-row pointer (k_new and v_new are both needed)");
    if (!a->cache_seqlens || !a->seqlens_out)
        return fail(FA_ERR_NULL, "cache_seqlens or seqlens_out is null: DEVICE pointers to batch int32 lengths are needed (they may be one pointer)");
    if (a->q && !a->q_out) return fail(FA_ERR_NULL, "q_out is null: q is rotated into a separate tensor");
    if (a->dtype != FA_FP16 && a->dtype != FA_BF16) return fail(FA_ERR_DTYPE, "Only fp16 and bf16 are supported");
    if (a->kv_dtype != 0 && a->kv_dtype != FA_KV_FP8_E4M3FN)
        return fail(FA_ERR_DTYPE, "kv_dtype (%d) is not served: 0 (the cache has dtype) or FA_KV_FP8_E4M3FN", a->kv_dtype);
    cache_tensors(c, *a);
    cache_descales(c, *a);
    c.fp8 = a->kv_dtype == FA_KV_FP8_E4M3FN;
    c.words_4b = "cache_seqlens, seqlens_out, block_table, k_descale and v_descale";
    int rc = cache_page_rule(c);   // (this path reports the page size in front of its other sizes)
    if (rc != FA_OK) return rc;
    if (a->d_head != 128) return fail(FA_ERR_SHAPE, "the append supports d_head = 128 only (got %lld)", (long long)a->d_head);
    if (a->batch < 0 || a->seqlen_new < 0 || a->n_kv_heads <= 0)
        return fail(FA_ERR_SHAPE, "batch and seqlen_new must not be negative, n_kv_heads must be positive");
    if (a->batch > INT32_MAX / 2 || a->seqlen_new > INT32_MAX / 2 || a->n_kv_heads > INT32_MAX / 2 || a->seqlen_new * a->n_kv_heads > INT32_MAX / 64)
        return fail(FA_ERR_SHAPE, "problem too large: the append's item counts are 32-bit");
    if ((rc = cache_sizes(c)) != FA_OK || (rc = cache_bounds(c)) != FA_OK) return rc;
    const bool rotary = a->rotary_cos || a->rotary_sin;
    if (rotary) {
        if (!a->rotary_cos || !a->rotary_sin) return fail(FA_ERR_SHAPE, "rotary_cos and rotary_sin come together (one of them is null)");
        if (a->rotary_dim < 16 || a->rotary_dim > 128 || a->rotary_dim % 16 != 0)
            return fail(FA_ERR_SHAPE, "rotary_dim (%lld) must be a multiple of 16 in [16, 128]", (long long)a->rotary_dim);
        if (a->seqlen_ro <= 0 || a->seqlen_ro > INT32_MAX / 2) return fail(FA_ERR_SHAPE, "seqlen_ro (%lld) must be positive", (long long)a->seqlen_ro);
        if (a->rotary_seq_stride < a->rotary_dim / 2)
            return fail(FA_ERR_SHAPE, "rotary_seq_stride (%lld) is smaller than rotary_dim / 2 (%lld)", (long long)a->rotary_seq_stride,
                        (long long)a->rotary_dim / 2);
    }
    if (a->q) {
        if (!rotary) return fail(FA_ERR_SHAPE, "q is given without rotary tables: there is nothing to do to it");
        if (a->seqlen_q <= 0 || a->n_heads <= 0) return fail(FA_ERR_SHAPE, "seqlen_q and n_heads must be positive when q is given");
        if (a->seqlen_q > INT32_MAX / 2 || a->n_heads > INT32_MAX / 2 || a->seqlen_q * a->n_heads > INT32_MAX / 64)
            return fail(FA_ERR_SHAPE, "problem too large: the append's item counts are 32-bit");
    }
    if (!c.fp8 && (a->k_descale || a->v_descale))
        return fail(FA_ERR_SHAPE, "k_descale / v_descale belong to an fp8 cache (kv_dtype FA_KV_FP8_E4M3FN); this cache is 16-bit");
    if ((rc = cache_descale_stride(c)) != FA_OK) return rc;
    if (a->seqlen_new > 0 &&
        (rc = stride_set("new", 8, a->batch, a->seqlen_new, a->n_kv_heads, a->new_batch_stride, a->new_seq_stride, a->new_head_stride)) != FA_OK)
        return rc;
    if ((rc = cache_strides(c, c.fp8 ? 16 : 8)) != FA_OK) return rc;   // (an fp8 cache's 16 bytes, in this path's own words)
    if (a->q) {
        if ((rc = stride_set("q", 8, a->batch, a->seqlen_q, a->n_heads, a->q_batch_stride, a->q_seq_stride, a->q_head_stride)) != FA_OK) return rc;
        if ((rc = stride_set("q_out", 8, a->batch, a->seqlen_q, a->n_heads, a->qo_batch_stride, a->qo_seq_stride, a->qo_head_stride)) != FA_OK)
            return rc;
        if (a->batch > 0) {
            const uintptr_t q0 = (uintptr_t)a->q, o0 = (uintptr_t)a->q_out;
            const uintptr_t q1 = q0 + (uintptr_t)append_extent(a->batch, a->seqlen_q, a->n_heads, a->q_batch_stride, a->q_seq_stride, a->q_head_stride);
            const uintptr_t o1 = o0 + (uintptr_t)append_extent(a->batch, a->seqlen_q, a->n_heads, a->qo_batch_stride, a->qo_seq_stride, a->qo_head_stride);
            if (q0 < o1 && o0 < q1) return fail(FA_ERR_SHAPE, "q_out overlaps q: the rotated query needs a tensor of its own");
        }
    }
    if (rotary && (a->rotary_seq_stride & 7)) return fail(FA_ERR_ALIGN, "rotary_seq_stride must be a multiple of 8 elements (16 bytes)");
    if (((uintptr_t)a->k | (uintptr_t)a->v | (uintptr_t)a->k_new | (uintptr_t)a->v_new | (uintptr_t)a->q | (uintptr_t)a->q_out |
         (uintptr_t)a->rotary_cos | (uintptr_t)a->rotary_sin) & 15)
        return fail(FA_ERR_ALIGN, "k, v, k_new, v_new, q, q_out, rotary_cos and rotary_sin must be 16-byte aligned");
    return cache_alignment(c, (uintptr_t)a->seqlens_out | (uintptr_t)a->k_descale | (uintptr_t)a->v_descale);
}
}  // namespace

int fa_kvcache_append_launch(const fa_kvcache_append_args *a, void *stream, float *ms) {
    CacheView c;
    int rc = append_validate(a, c);
    if (rc != FA_OK) return rc;
    if (a->batch == 0) {
        if (ms) *ms = 0.0f;
        return FA_OK;
    }
    DeviceState *dev = current_device(&rc);
    if (!dev) return rc;
    const bool rotary = a->rotary_cos != nullptr, fp8 = c.fp8, with_q = rotary && a->q;
    fa::AppendArgs d;
    d.k_new = (const uint16_t *)a->k_new;
    d.v_new = (const uint16_t *)a->v_new;
    d.k = a->k;
    d.v = a->v;
    d.q = with_q ? (const uint16_t *)a->q : nullptr;
    d.q_out = with_q ? (uint16_t *)a->q_out : nullptr;
    d.cos = (const uint16_t *)a->rotary_cos;
    d.sin = (const uint16_t *)a->rotary_sin;
    d.cache_seqlens = c.cache_seqlens;
    d.seqlens_out = a->seqlens_out;
    d.block_table = c.block_table;
    d.k_descale = c.k_descale;   // (null for a 16-bit cache: validated)
    d.v_descale = c.v_descale;
    d.new_bs = a->new_batch_stride;
    d.new_ss = a->new_seq_stride;
    d.new_hs = a->new_head_stride;
    d.q_bs = a->q_batch_stride;
    d.q_ss = a->q_seq_stride;
    d.q_hs = a->q_head_stride;
    d.qo_bs = a->qo_batch_stride;
    d.qo_ss = a->qo_seq_stride;
    d.qo_hs = a->qo_head_stride;
    d.kv_bs = c.kv_bs;
    d.kv_ss = c.kv_ss;
    d.kv_hs = c.kv_hs;
    d.bt_bs = c.paged() ? c.block_table_stride : 0;
    d.ds_bs = c.descale_bs;
    d.ro_ss = rotary ? a->rotary_seq_stride : 0;
    d.seqlen_new = (int32_t)a->seqlen_new;
    d.seqlen_q = with_q ? (int32_t)a->seqlen_q : 0;
    d.n_heads = with_q ? (int32_t)a->n_heads : 0;
    d.n_kv_heads = (int32_t)a->n_kv_heads;
    d.max_len = (int32_t)c.capacity();
    d.page_size = c.paged() ? (int32_t)c.page_size : 0;
    d.num_pages = c.paged() ? (int32_t)c.num_pages : 0;
    d.rotary_dim = rotary ? (int32_t)a->rotary_dim : 0;
    d.seqlen_ro = rotary ? (int32_t)a->seqlen_ro : 0;
    d.interleaved = a->rotary_interleaved != 0;
    d.causal = a->causal != 0;
    const hipStream_t s = (hipStream_t)stream;
    const int batch = (int)a->batch;
    return enqueue_timed([&] { return fa::kvcache_append_enqueue(d, batch, a->dtype, fp8, s); }, s, ms);
}

static void add_slot(const AdaptiveState &ad, int idx, fa_adaptive_info *out) {
    const AdaptivePolicy &p = ad.slot[idx].p;
    out->launches += p.seq;
    out->demoted += p.demoted;
    out->reports += p.reports;
    if (p.mode != AdaptivePolicy::NORMAL || out->hold < p.hold) {   // the record that is (or was longest) demoted
        if (p.hold >= out->hold) { out->hold = p.hold; out->remaining = p.remaining; }
        if (p.mode > out->mode) out->mode = p.mode;
    }
    if (ad.flag_host) { const uint32_t r = __atomic_load_n(ad.flag_host + idx, __ATOMIC_RELAXED); if (r > out->last_report) out->last_report = r; }
}

int fa_adaptive_state(int device, fa_adaptive_info *out) {
    if (!out) return fail(FA_ERR_NULL, "null output");
    if (device < 0 || device >= kMaxDevices) return fail(FA_ERR_DEVICE, "device ordinal %d out of range", device);
    memset(out, 0, sizeof(*out));
    out->hold = 32;
    DeviceState &st = g_dev[device];
    if (!st.inited.load(std::memory_order_acquire)) return FA_OK;
    AdaptiveState &ad = st.adaptive;
    std::lock_guard<std::mutex> lock(ad.mu);
    // the device's records taken together: counters summed; mode / hold / remaining of the record that is demoted (or was
    // demoted longest)
    for (int i = 0; i < ad.n_slots(); ++i) add_slot(ad, i, out);
    out->available = ad.flag_host != nullptr;
    return FA_OK;
}

int fa_adaptive_state_for(int device, const fa_fwd_config *cfg, const fa_fwd_opts *opts, fa_adaptive_info *out) {
    if (!out || !cfg) return fail(FA_ERR_NULL, "null pointer argument");
    if (device < 0 || device >= kMaxDevices) return fail(FA_ERR_DEVICE, "device ordinal %d out of range", device);
    fa_fwd_opts o;
    int rc = read_opts(opts, &o);
    if (rc != FA_OK) return rc;
    Want w;
    w.masked = o.causal || o.allow_ragged;
    w.ragged = o.allow_ragged != 0;
    w.speculative = true;
    w.prescaled_q = o.prescaled_q != 0;
    const char *why = "";
    const fa::KernelEntry *e = find_kernel(cfg, &why, w);
    if (!e) return fail(FA_ERR_NO_KERNEL, "%s", why);
    memset(out, 0, sizeof(*out));
    out->hold = 32;
    DeviceState &st = g_dev[device];
    if (!st.inited.load(std::memory_order_acquire)) return FA_OK;
    AdaptiveState &ad = st.adaptive;
    std::lock_guard<std::mutex> lock(ad.mu);
    const int idx = (int)(e - registry().data());
    if (idx >= 0 && idx < ad.n_slots()) {
        const AdaptivePolicy &p = ad.slot[idx].p;
        out->launches = p.seq; out->demoted = p.demoted; out->reports = p.reports;
        out->hold = p.hold; out->mode = p.mode; out->remaining = p.remaining;
        out->last_report = ad.flag_host ? __atomic_load_n(ad.flag_host + idx, __ATOMIC_RELAXED) : 0u;
    }
    out->available = ad.flag_host != nullptr;
    return FA_OK;
}

int fa_adaptive_simulate(int n, const uint32_t *report_word, const int32_t *probe_state, int32_t *run, fa_adaptive_info *final_state) {
    if (n < 0 || (n > 0 && (!report_word || !probe_state || !run))) return fail(FA_ERR_NULL, "null pointer argument");
    AdaptivePolicy p;
    for (int i = 0; i < n; ++i) run[i] = p.step(report_word[i], probe_state[i]);
    if (final_state) {
        memset(final_state, 0, sizeof(*final_state));
        final_state->available = 1;
        final_state->launches = p.seq;
        final_state->demoted = p.demoted;
        final_state->reports = p.reports;
        final_state->hold = p.hold;
        final_state->mode = p.mode;
        final_state->remaining = p.remaining;
        final_state->last_report = n > 0 ? report_word[n - 1] : 0u;
    }
    return FA_OK;
}

int fa_adaptive_reset(int device) {
    if (device < 0 || device >= kMaxDevices) return fail(FA_ERR_DEVICE, "device ordinal %d out of range", device);
    DeviceState &st = g_dev[device];
    if (!st.inited.load(std::memory_order_acquire)) return FA_OK;
    AdaptiveState &ad = st.adaptive;
    std::lock_guard<std::mutex> lock(ad.mu);
    for (int i = 0; i < ad.n_slots(); ++i)
        ad.slot[i].p.reset(ad.flag_host ? __atomic_load_n(ad.flag_host + i, __ATOMIC_RELAXED) : 0u);
    return FA_OK;
}

int fa_num_kernels(void) { return (int)registry().size(); }

static void fill_info(const fa::KernelEntry &e, fa_kernel_info *out);

int fa_fwd_query(const fa_fwd_config *cfg, const fa_fwd_opts *opts, fa_kernel_info *out) {
    if (!cfg || !out) return fail(FA_ERR_NULL, "null pointer argument");
    fa_fwd_opts o;
    int rc = read_opts(opts, &o);
    if (rc != FA_OK) return rc;
    Want w;
    w.masked = o.causal || o.allow_ragged;
    w.ragged = o.allow_ragged != 0;
    w.speculative = o.speculative != 0;
    w.prescaled_q = o.prescaled_q != 0;
    const char *why = "";
    const fa::KernelEntry *e = find_kernel(cfg, &why, w);
    if (!e) return fail(FA_ERR_NO_KERNEL, "%s", why);
    fill_info(*e, out);
    return FA_OK;
}

int fa_get_kernel(int index, fa_kernel_info *out) {
    if (!out) return fail(FA_ERR_NULL, "null output");
    if (index < 0 || index >= (int)registry().size()) return fail(FA_ERR_SHAPE, "index out of range");
    fill_info(registry()[index], out);
    return FA_OK;
}

static void fill_info(const fa::KernelEntry &e, fa_kernel_info *out) {
    memset(out, 0, sizeof(*out));
    out->cfg.dtype = e.dtype;
    out->cfg.d_head = e.d_head;
    out->cfg.B_r = e.rows_per_wave * e.n_waves;
    out->cfg.B_c = e.B_c;
    out->cfg.n_warps = e.n_waves;
    out->cfg.async_copy = e.async_copy;
    out->cfg.eager_load_blocks = e.eager;
    out->cfg.swizzled = e.swizzled;
    out->cfg.optimized_softmax = e.softmax_mode == FA_SOFTMAX_FIRST_BLOCK_SKIP;  // (the reference's meaning only)
    out->cfg.mma_double_buffer_loads = e.pipelined;
    out->softmax_mode = e.softmax_mode;
    out->prescaled_q = e.prescaled_q;
    out->threads = e.threads;
    out->lds_bytes = e.lds_bytes;
    out->rows_per_wave = e.rows_per_wave;
    out->masked = e.masked;
    out->num_regs = -1;
    out->scratch_bytes = -1;
    hipFuncAttributes attr;
    if (hipFuncGetAttributes(&attr, (const void *)e.fn) == hipSuccess) {
        out->num_regs = attr.numRegs;
        out->scratch_bytes = (int32_t)attr.localSizeBytes;
    } else {
        (void)hipGetLastError();  // no device: resource fields stay -1
    }
    out->ring_form = e.fn_ring ? 1 : 0;
    out->ring_lds_bytes = e.fn_ring ? e.ring_lds_bytes : 0;
    out->persistent = e.persistent;
    out->alt_form = e.fn_alt ? 1 : 0;
    out->ring_threads = e.fn_ring ? (e.ring_threads ? e.ring_threads : e.threads) : 0;
    out->ring_softmax_mode = e.fn_ring ? (e.softmax_mode == FA_SOFTMAX_SPECULATIVE ? FA_SOFTMAX_SPECULATIVE : FA_SOFTMAX_LAZY) : 0;
    out->ring_num_regs = out->ring_scratch_bytes = e.fn_ring ? -1 : 0;
    if (e.fn_ring) {
        if (hipFuncGetAttributes(&attr, (const void *)e.fn_ring) == hipSuccess) {
            out->ring_num_regs = attr.numRegs;
            out->ring_scratch_bytes = (int32_t)attr.localSizeBytes;
        } else {
            (void)hipGetLastError();
        }
    }
}

int fa_get_kernel_sized(int index, fa_kernel_info *out, uint32_t out_size) {
    if (!out) return fail(FA_ERR_NULL, "null output");
    fa_kernel_info full;
    const int rc = fa_get_kernel(index, &full);
    if (rc != FA_OK) return rc;
    memcpy(out, &full, out_size < sizeof(full) ? out_size : sizeof(full));
    return FA_OK;
}

int fa_fwd_query_sized(const fa_fwd_config *cfg, const fa_fwd_opts *opts, fa_kernel_info *out, uint32_t out_size) {
    if (!out) return fail(FA_ERR_NULL, "null pointer argument");
    fa_kernel_info full;
    const int rc = fa_fwd_query(cfg, opts, &full);
    if (rc != FA_OK) return rc;
    memcpy(out, &full, out_size < sizeof(full) ? out_size : sizeof(full));
    return FA_OK;
}

int fa_abi_version(void) { return FA_ABI_VERSION; }

const char *fa_last_error(void) { return g_err; }

const char *fa_version(void) { return "fa_hip 0.6 gfx950"; }

}  // extern "C"
