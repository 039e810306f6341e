"""Inputs and eager references for the tests of logit soft-capping on the inference path (tests/test_softcap_infer_cpu.py,
tests/test_softcap_infer_gpu.py): KV-cache decode (forward_kvcache_softcap) and cache prefill
(forward_varlen_kvcache(softcap=)), 16-bit and fp8 cache.

N(0, 1) q, k, v from the CPU generator, heads (8, 2).  The reference is softcap_inputs.capped_attention per batch entry, fp32 and
16-bit -- logit = softcap tanh(s / softcap) on the keys a row sees, s = q . k / sqrt(128), -inf elsewhere, the cap BEFORE the
mask; for an fp8 cache it runs on the dequantized cache.  Two deliberately wrong restatements serve the CPU proof that the inputs
discriminate: no cap at all, and (fp8) a cap of the RAW undescaled score with k_descale applied behind it.  References are
computed once per case and shared (nobody writes into them).

Plain helper module: no tests, no fixtures."""
import functools
import math

import torch

import beacon_inputs as bi
import softcap_inputs as sc

D = sc.D
HEADS = (8, 2)
DTYPES = sc.DTYPES
WINDOWS = sc.WINDOWS                   # (left, right, causal)
CAPS = [0.5, 4.0]                      # both discriminate on these inputs (tests/test_softcap_infer_cpu.py proves it)
LINEAR_CAP = 50.0                      # nearly linear here: an accuracy case for the tanh near 0, no discriminator
# decode: one batch of mixed lengths; seqlen_q 1, 4, 8 x group 4 = 4, 16, 32 packed rows (one, two row tiles), and seqlen_q 8 x
# group 8 = 64 packed rows (four row tiles) on heads (8, 1)
DECODE_LENGTHS = [0, 1, 31, 64, 65, 300, 1000]
DECODE_SEQLENS_Q = [1, 4, 8]
DECODE_CACHE_LEN = 1024                # a multiple of both page sizes
HEADS_64 = (8, 1)
PAGE_SIZES = [64, 256]
# prefill: (len_q, len_k) per sequence
PREFILL_PAIRS = [(165, 197), (37, 1000), (129, 65), (0, 300), (5, 0), (300, 1000)]
PREFILL_CACHE_LEN = 1024
PROOF_MIN_KEYS = 31                    # the proof's entries: at least this many keys (a row of 0 or 1 keys has one softmax whatever the logit)
F8 = torch.float8_e4m3fn


def quantize(k, v):
    """flash_attention_kernels.quantize_kvcache_fp8's expression (descales about amax / 448 per (entry, head)) -> k8, v8, kd, vd"""
    from flash_attention_from_scratch_amd.flash_attention_kernels import quantize_kvcache_fp8
    return quantize_kvcache_fp8(k, v)


def dequantize(x8, descale):
    """the fp32 values an fp8 cache (B, S, Hkv, D) with descales (B, Hkv) stands for"""
    return x8.float() * descale[:, None, :, None]


@functools.lru_cache(maxsize=None)
def decode_inputs(dtype, seqlen_q, heads=HEADS, seed=0):
    """-> dict: q (B, Sq, H, 128), k, v (B, DECODE_CACHE_LEN, Hkv, 128) in dtype on the CPU, lens"""
    n_heads, n_kv = heads
    gen = torch.Generator().manual_seed(4000 + 10 * seqlen_q + seed)
    B = len(DECODE_LENGTHS)
    q = torch.randn((B, seqlen_q, n_heads, D), generator=gen).to(dtype)
    k = torch.randn((B, DECODE_CACHE_LEN, n_kv, D), generator=gen).to(dtype)
    v = torch.randn((B, DECODE_CACHE_LEN, n_kv, D), generator=gen).to(dtype)
    return dict(q=q, k=k, v=v, lens=list(DECODE_LENGTHS), heads=heads, dtype=dtype)


@functools.lru_cache(maxsize=None)
def prefill_inputs(dtype, seed=0):
    """-> dict: q packed (total_q, H, 128), k, v (n_seqs, PREFILL_CACHE_LEN, Hkv, 128) in dtype on the CPU, cu_q, lens (the keys)"""
    n_heads, n_kv = HEADS
    gen = torch.Generator().manual_seed(5000 + seed)
    cu_q = [0]
    for n_q, _ in PREFILL_PAIRS:
        cu_q.append(cu_q[-1] + n_q)
    q = torch.randn((cu_q[-1], n_heads, D), generator=gen).to(dtype)
    k = torch.randn((len(PREFILL_PAIRS), PREFILL_CACHE_LEN, n_kv, D), generator=gen).to(dtype)
    v = torch.randn((len(PREFILL_PAIRS), PREFILL_CACHE_LEN, n_kv, D), generator=gen).to(dtype)
    return dict(q=q, k=k, v=v, cu_q=cu_q, lens=[p[1] for p in PREFILL_PAIRS], heads=HEADS, dtype=dtype)


@functools.lru_cache(maxsize=None)
def fp8_cache(kind, dtype, seqlen_q=1, heads=HEADS, pow2=False):
    """The fp8 form of decode_inputs' (kind "decode") or prefill_inputs' (kind "prefill") cache -> dict: k8, v8, kd, vd and the
    dequantized fp32 k, v the reference runs on.  pow2: the descales rounded up to powers of two before quantizing, so that the
    dequantized values are exact in both 16-bit types and a 16-bit cache can hold them."""
    inp = decode_inputs(dtype, seqlen_q, heads) if kind == "decode" else prefill_inputs(dtype)
    k8, v8, kd, vd = quantize(inp["k"].float(), inp["v"].float())
    if pow2:
        kd, vd = (torch.exp2(torch.ceil(torch.log2(t))) for t in (kd, vd))
        k8 = (inp["k"].float() / kd[:, None, :, None]).to(F8)
        v8 = (inp["v"].float() / vd[:, None, :, None]).to(F8)
    return dict(k8=k8, v8=v8, kd=kd, vd=vd, k=dequantize(k8, kd), v=dequantize(v8, vd))


def entry(inp, b, cache=None):
    """batch entry / sequence b -> (q rows (n_q, H, 128), its valid keys k, v (len, Hkv, 128)); cache: an fp8_cache dict, whose
    dequantized values replace the 16-bit ones"""
    n = inp["lens"][b]
    q = inp["q"][b] if "cu_q" not in inp else inp["q"][inp["cu_q"][b]:inp["cu_q"][b + 1]]
    src = cache if cache is not None else inp
    return q, src["k"][b, :n], src["v"][b, :n]


def reference_entry(q, k, v, window, dtype, softcap):
    """-> dict(o32, lse32, o16): softcap_inputs.capped_attention in fp32 and in dtype"""
    o32, lse32 = sc.capped_attention(q, k, v, window, torch.float32, softcap)
    o16, _ = sc.capped_attention(q, k, v, window, dtype, softcap)
    return dict(o32=o32, lse32=lse32, o16=o16)


@functools.lru_cache(maxsize=None)
def decode_reference(dtype, seqlen_q, window, softcap, fp8=False, heads=HEADS):
    """one dict per batch entry of decode_inputs; fp8: on the dequantized cache"""
    inp = decode_inputs(dtype, seqlen_q, heads)
    cache = fp8_cache("decode", dtype, seqlen_q, heads) if fp8 else None
    return [reference_entry(*entry(inp, b, cache), window, dtype, softcap) for b in range(len(inp["lens"]))]


@functools.lru_cache(maxsize=None)
def prefill_reference(dtype, window, softcap, fp8=False):
    inp = prefill_inputs(dtype)
    cache = fp8_cache("prefill", dtype) if fp8 else None
    return [reference_entry(*entry(inp, b, cache), window, dtype, softcap) for b in range(len(inp["lens"]))]


def raw_cap_then_descale(q, k8, v, kd, window, softcap):
    """The wrong fp8 restatement, fp32: the cap on the RAW score q . float(k8) / sqrt(128), k_descale (Hkv,) applied behind it ->
    o (n_q, H, 128).  (What a kernel computes that caps S where the uncapped fp8 form keeps it, in undescaled units.)"""
    n_q, n_k = q.shape[0], k8.shape[0]
    left, right = bi.window_sides(*window)
    lo, hi = bi.window_bounds(n_q, n_k, left, right)
    group = q.shape[1] // k8.shape[1]
    kk, vv = k8.float().repeat_interleave(group, dim=1), v.float().repeat_interleave(group, dim=1)
    s = torch.einsum("qhd,khd->hqk", q.float(), kk) * (1.0 / math.sqrt(D))
    s = softcap * torch.tanh(s / softcap) * kd.repeat_interleave(group)[:, None, None]
    keys = torch.arange(n_k)[None, :]
    hidden = (keys > hi[:, None]) | (keys < lo[:, None])
    s = s.masked_fill(hidden[None], bi.NEG_INF)
    dead = hidden.all(dim=1)[None, :, None]
    p = torch.softmax(s.masked_fill(dead, 0.0), dim=-1).masked_fill(dead, 0.0)
    return torch.einsum("hqk,khd->qhd", p, vv)


def paginate(k, v, page_size, seed=3):
    """Contiguous caches (B, S, Hkv, D), S a multiple of page_size, of any dtype scattered into shuffled pages with three spare ones
    -> (k pages, v pages, block_table int32 (B, S / page_size)); on the caches' device"""
    B, cache_len, n_kv, d = k.shape
    per_seq = cache_len // page_size
    num_pages = B * per_seq + 3
    perm = torch.randperm(num_pages, generator=torch.Generator().manual_seed(seed))[:B * per_seq]
    out = []
    for t in (k, v):
        raw = t.view(torch.uint8) if t.element_size() == 1 else t
        pages = torch.zeros((num_pages, page_size, n_kv, d), dtype=raw.dtype, device=t.device)
        pages[perm.to(t.device)] = raw.reshape(B * per_seq, page_size, n_kv, d)
        out.append(pages.view(t.dtype))
    return out[0], out[1], perm.view(B, per_seq).to(torch.int32).to(k.device)


def lo_min(n, n_q, left):
    """the lowest key any row of an entry with n keys and n_q query rows sees"""
    return bi.window_lo_min(n, n_q, left)
