"""`flash_attention` -- the reference's public API, unchanged
(/root/reference/flash_attention/__init__.py:7-17):

    forward(kernel_cfg, q, k, v, o=None) -> Tensor
    forward_timed(kernel_cfg, q, k, v, o=None) -> (Tensor, milliseconds)

This build's additions: forward_ex (causal, ragged seq_len, the row log-sum-exp), backward (dQ, dK, dV) and
attention (a torch.autograd.Function over the two).
"""

import torch

from .. import flash_attention_kernels


def forward(kernel_cfg, q, k, v, o=None):
    return flash_attention_kernels.forward(kernel_cfg, q, k, v, o, benchmark=False)[0]


def forward_timed(kernel_cfg, q, k, v, o=None):
    out, runtime_ms = flash_attention_kernels.forward(kernel_cfg, q, k, v, o, benchmark=True)
    return out, runtime_ms


def forward_ex(kernel_cfg, q, k, v, o=None, causal=False, timed=False, stats=None, return_lse=False):
    """Scope wideners beyond the reference API: optional causal mask, and any
    seq_len (not only multiples of B_r / B_c).  `stats`: optional device tensor of two 32-bit counters
    (items computed, items the speculative softmax computed twice; fa_fwd_stats in include/fa_hip.h).
    Returns Tensor, or (Tensor, ms) if timed.  return_lse: also the row log-sum-exp, an fp32 (batch, n_heads, seq_len)
    tensor (ln sum_j exp(q_i . k_j / sqrt d)), with the same O bits -> (Tensor, lse) or (Tensor, lse, ms); RuntimeError
    where the configuration has no such form (fa_fwd_launch_lse in include/fa_hip.h).
    Grouped-query attention: k and v of shape (batch, seq_len, n_kv_heads, d_head), n_kv_heads dividing n_heads (query
    head h reads K / V head h / (n_heads / n_kv_heads)); served by the configurations with the row log-sum-exp, which is
    computed and dropped unless return_lse (fa_fwd_launch_gqa)."""
    if flash_attention_kernels.is_gqa(q, k, v) and not return_lse:
        out, _, ms = flash_attention_kernels.forward_lse(kernel_cfg, q, k, v, o, benchmark=timed, causal=causal,
                                                         allow_ragged=True, stats=stats)
        return (out, ms) if timed else out
    if return_lse:
        out, lse, ms = flash_attention_kernels.forward_lse(kernel_cfg, q, k, v, o, benchmark=timed, causal=causal,
                                                           allow_ragged=True, stats=stats)
        return (out, lse, ms) if timed else (out, lse)
    out, ms = flash_attention_kernels.forward(kernel_cfg, q, k, v, o, benchmark=timed, causal=causal,
                                              allow_ragged=True, stats=stats)
    return (out, ms) if timed else out


def backward(q, k, v, o, lse, dout, causal=False, timed=False):
    """dQ, dK, dV from the forward's o and lse (forward_ex(..., return_lse=True)) and the gradient dout -> (dq, dk, dv), or
    (dq, dk, dv, ms) if timed.  Deterministic: the same inputs give the same bits.  Grouped-query attention (k, v with
    n_kv_heads heads): dk and dv have n_kv_heads heads."""
    return flash_attention_kernels.backward(q, k, v, o, lse, dout, causal=causal, timed=timed)


def _needs_copy(t):
    # the forward with LSE needs seq_stride % 128 == 0 and one stride set for q, k, v
    return t.stride(3) != 1 or t.stride(1) % 128 != 0


class _Attention(torch.autograd.Function):
    @staticmethod
    def forward(ctx, q, k, v, causal):
        from flash_helpers import kernel_configs as kc

        if flash_attention_kernels.is_gqa(q, k, v):   # (K / V have strides of their own)
            if _needs_copy(q):
                q = q.contiguous()
            if _needs_copy(k) or v.stride() != k.stride():
                k, v = k.contiguous(), v.contiguous()
        elif _needs_copy(q) or k.stride() != q.stride() or v.stride() != q.stride():
            q, k, v = q.contiguous(), k.contiguous(), v.contiguous()
        name = kc.DType.BF16 if q.dtype == torch.bfloat16 else kc.DType.FP16
        cfg = kc.best_config(name, q.shape[1], masked=causal)
        o, lse = forward_ex(cfg, q, k, v, causal=causal, return_lse=True)
        ctx.save_for_backward(q, k, v, o, lse)
        ctx.causal = causal
        return o

    @staticmethod
    def backward(ctx, dout):
        q, k, v, o, lse = ctx.saved_tensors
        dq, dk, dv = backward(q, k, v, o, lse, dout.contiguous(), causal=ctx.causal)
        return dq, dk, dv, None


def attention(q, k, v, causal=False):
    """softmax(q k^T / sqrt d) v with gradients: (batch, seq_len, n_heads, 128) bf16 / fp16 tensors, seq_len % 256 == 0.
    The forward is best_config(dtype, seq_len, masked=causal) with the row log-sum-exp; the backward is the HIP backward.
    Grouped-query attention: k and v may have n_kv_heads heads (dividing n_heads); their gradients then have as many."""
    return _Attention.apply(q, k, v, causal)


def forward_varlen(q, k, v, cu_seqlens, max_seqlen, causal=False, timed=False, cu_seqlens_k=None, max_seqlen_k=None, *,
                   window_size=(-1, -1), softcap=0.0):
    """Packed variable-length sequences: q (total_tokens, n_heads, 128), k / v (total_tokens, n_kv_heads, 128), cu_seqlens an
    int32 device tensor of n_seqs + 1 row offsets, max_seqlen a Python int (no device sync) -> (o, lse[, ms]) with lse fp32
    (n_heads, total_tokens).  A query attends to the keys of its own sequence (causal: at or before its position in it).

    With cu_seqlens_k and max_seqlen_k (both or neither: one alone is a ValueError) Q and K / V have lengths of their own:
    cu_seqlens / max_seqlen are Q's, k / v are (total_k, n_kv_heads, 128) with sequence i's keys at rows cu_seqlens_k[i] ..
    cu_seqlens_k[i + 1] - 1, any lengths >= 0 on either side.  causal is then bottom-right aligned (forward_kvcache's and
    flash-attn's rule): query r sees keys j <= r + (len_k - len_q); a row that sees no key gives o = 0, lse = -inf.

    Sliding-window (local) attention: window_size=(left, right), keyword only, two Python ints, -1 = unbounded.
    Query row r, at position p = r + (len_k - len_q), sees the keys max(0, p - left) .. min(len_k - 1, p + right); causal means
    right = 0; bad values are a ValueError.  (-1, -1) is the call above, unchanged.  The gradients of a windowed forward are
    backward_varlen_window's, and attention_varlen(window_size=) pairs the two; backward_varlen takes no window --
    do not feed it a windowed forward's o and lse.

    Logit soft-capping (flash-attn's softcap): softcap, keyword only, a Python float or int, finite and >= 0.  The
    logit of a key the row sees becomes softcap * tanh(s / softcap), s = q . k / sqrt(128); the cap comes before every mask, so a
    key the row does not see stays -inf; lse is the log-sum-exp of the capped logits.  0 is off: the call above, unchanged.  Bad
    values are a ValueError.  The gradients of a soft-capped forward are backward_varlen_softcap's, and attention_varlen(softcap=)
    pairs the two."""
    return flash_attention_kernels.forward_varlen(q, k, v, cu_seqlens, max_seqlen, causal=causal, timed=timed,
                                                  cu_seqlens_k=cu_seqlens_k, max_seqlen_k=max_seqlen_k, window_size=window_size,
                                                  softcap=softcap)


def forward_kvcache(q, k_cache, v_cache, cache_seqlens, block_table=None, causal=False, return_lse=False, max_seqlen_k=None,
                    num_splits=0, timed=False, k_descale=None, v_descale=None, window_size=(-1, -1), k=None, v=None, rotary_cos=None,
                    rotary_sin=None, rotary_interleaved=False, advance_seqlens=False):
    """Decode attention against a K / V cache: q (batch, seqlen_q, n_heads, 128) against k_cache / v_cache
    (batch, seqlen_cache, n_kv_heads, 128) -- or, with block_table (batch, max_pages_per_seq) int32, pages (num_pages,
    page_size, n_kv_heads, 128) -- of which cache_seqlens (batch,) int32 ON THE DEVICE says how many keys are valid, the newest
    tokens included.  seqlen_q * n_heads / n_kv_heads <= 64; causal is bottom-right aligned; a row without keys gives o = 0,
    lse = -inf.  num_splits = 0 takes the split rule (a function of the shapes and max_seqlen_k alone).  -> o, or (o, lse) with
    return_lse, each with ms appended if timed.  No device synchronisation unless timed; graph-capturable.

    An fp8 cache: k_cache / v_cache of dtype torch.float8_e4m3fn in the same shapes, q and o still bf16 / fp16.
    k_descale, v_descale: fp32 (batch, n_kv_heads) ON THE DEVICE, None = 1, finite and positive; key j of entry b and K / V head
    h stands for float(k8[j]) * k_descale[b, h], likewise V (quantize_kvcache_fp8 makes such a cache).  Other float8 dtypes,
    K and V of different dtypes, and descales with a 16-bit cache are refused.

    A fused decode step: with k, v (batch, seqlen_new, n_kv_heads, 128), cache_seqlens counts the keys BEFORE
    the call (flash-attn's flash_attn_with_kvcache); the new rows are appended in place first (append_kvcache: rotated with
    rotary_cos / rotary_sin (seqlen_ro, rotary_dim / 2) like q, quantized for an fp8 cache) and the attention covers
    cache_seqlens + seqlen_new keys.  advance_seqlens=True also writes the new lengths into cache_seqlens.  max_seqlen_k bounds the
    lengths after the append.  Rotary without k / v, k without v, and rotary under causal with seqlen_new != seqlen_q are refused.

    Sliding-window (local) attention (flash-attn's window_size): window_size=(left, right), two Python ints, -1 =
    unbounded.  Query row i, at position p = len - seqlen_q + i, sees the keys max(0, p - left) .. min(len - 1, p + right); causal
    means right = 0 (causal with another bounded right is a ValueError, like values below -1).  (-1, -1) is the call above,
    unchanged.  The kernel fetches no key below the lowest one a row of the batch entry sees and reads no block_table entry of a
    page wholly below it: such rows and pages may be stale, freed or reused.  With k / v the window applies to the lengths after
    the append."""
    return flash_attention_kernels.forward_kvcache(q, k_cache, v_cache, cache_seqlens, block_table=block_table, causal=causal,
                                                   return_lse=return_lse, max_seqlen_k=max_seqlen_k, num_splits=num_splits, timed=timed,
                                                   k_descale=k_descale, v_descale=v_descale, k=k, v=v, rotary_cos=rotary_cos,
                                                   rotary_sin=rotary_sin, rotary_interleaved=rotary_interleaved,
                                                   advance_seqlens=advance_seqlens, window_size=window_size)


def forward_kvcache_softcap(q, k_cache, v_cache, cache_seqlens, softcap, block_table=None, causal=False, return_lse=False,
                            max_seqlen_k=None, num_splits=0, timed=False, k_descale=None, v_descale=None, window_size=(-1, -1), k=None,
                            v=None, rotary_cos=None, rotary_sin=None, rotary_interleaved=False, advance_seqlens=False):
    """forward_kvcache with logit soft-capping (flash-attn's softcap, Gemma-2's attention): every other argument is
    forward_kvcache's, with its meaning, checks and defaults -- both cache types, paged and contiguous, the window, the fused
    append.  softcap, required, a Python float or int, finite and >= 0: the logit of a key the row sees becomes
    softcap * tanh(s / softcap), s = q . k / sqrt(128) on the dequantized key, applied before any mask (a masked key stays -inf);
    lse is the log-sum-exp of the capped logits.  0 is off: forward_kvcache with the same arguments, bit for bit.  With k / v the
    append runs first, unchanged: the cap belongs to the attention only.  The split count and the workspace are the windowed
    call's.  A bad window_size is reported first, then a bad softcap: both a ValueError before any tensor is looked at."""
    return flash_attention_kernels.forward_kvcache_softcap(q, k_cache, v_cache, cache_seqlens, softcap, block_table=block_table,
                                                           causal=causal, return_lse=return_lse, max_seqlen_k=max_seqlen_k,
                                                           num_splits=num_splits, timed=timed, k_descale=k_descale, v_descale=v_descale,
                                                           window_size=window_size, k=k, v=v, rotary_cos=rotary_cos, rotary_sin=rotary_sin,
                                                           rotary_interleaved=rotary_interleaved, advance_seqlens=advance_seqlens)


def forward_varlen_kvcache(q, k_cache, v_cache, cu_seqlens_q, max_seqlen_q, cache_seqlens, block_table=None, causal=False,
                           max_seqlen_k=None, timed=False, k_descale=None, v_descale=None, *, window_size=(-1, -1), softcap=0.0):
    """Prefill against a K / V cache (flash-attn's flash_attn_varlen_func(..., block_table=)): chunked prefill
    behind a cached prefix, prompts behind a shared prefix, verification of more rows than forward_kvcache serves.  q
    (total_q, n_heads, 128) holds the query rows of all sequences packed, sequence i's at rows cu_seqlens_q[i] ..
    cu_seqlens_q[i + 1] - 1 (int32, n_seqs + 1 entries ON THE DEVICE), at most max_seqlen_q (a Python int) each.  The keys are
    read from the cache in place: k_cache / v_cache (n_seqs, seqlen_cache, n_kv_heads, 128) -- or, with block_table
    (n_seqs, max_pages_per_seq) int32, pages (num_pages, page_size, n_kv_heads, 128), page_size a multiple of 64 -- of which
    cache_seqlens (n_seqs,) int32 ON THE DEVICE says how many are valid, the chunk's own keys (appended before this call, with
    append_kvcache for one) included.  causal is bottom-right aligned: query r sees keys j <= r + (len_k - len_q); a row that sees
    no key gives o = 0, lse = -inf.  max_seqlen_k (a Python int) bounds every length, None = the capacity.
    -> (o, lse[, ms]) with lse fp32 (n_heads, total_q): bit for bit forward_varlen(cu_seqlens_k=) on the same keys packed.  bf16 /
    fp16.  No device synchronisation unless timed; graph-capturable; the same inputs give the same bits.
    An fp8 cache (torch.float8_e4m3fn, the cache append_kvcache writes and forward_kvcache decodes against) is served when BOTH
    k_descale and v_descale are given: fp32 (n_seqs, n_kv_heads) ON THE DEVICE, last dimension contiguous, never read by the host.
    Key j of sequence b (the sequence index, for a paged cache too), K / V head h stands for float(k8[j]) * k_descale[b, h],
    likewise V, and the result is the 16-bit call's on those values.  Note the asymmetry with forward_kvcache, where a missing
    descale means 1: here an fp8 cache with either descale missing is refused -- pass ones for an unscaled cache.  A descale with
    a 16-bit cache, caches of two dtypes and fp8 encodings other than e4m3fn are refused.

    Sliding-window (local) attention (forward_kvcache's window_size, so a model with local layers prefills and
    decodes by one rule): window_size=(left, right), keyword only, two Python ints, -1 = unbounded.  Query row r of sequence b, at
    position p = r + (len_k - len_q), sees the keys max(0, p - left) .. min(len_k - 1, p + right); causal means right = 0 (causal
    with another bounded right is a ValueError, like values below -1).  (-1, -1) is the call above, unchanged.  Each block of 128
    query rows visits only the key tiles of its rows' windows; no cache row, page or block_table entry wholly below
    max(0, len_k - len_q - left) is read, so such rows and pages may be stale, freed or reused.  Both cache types, paged and
    contiguous; bit for bit forward_varlen(cu_seqlens_k=, window_size=) on the same keys packed.

    Logit soft-capping (forward_varlen's softcap, so a model trained with a cap prefills and decodes by one rule):
    softcap, keyword only, a Python float or int, finite and >= 0.  The logit of a key the row sees becomes
    softcap * tanh(s / softcap), s = q . k / sqrt(128) on the dequantized key, applied before any mask; lse is the log-sum-exp of the
    capped logits.  0 is the call above, unchanged.  With or without a window, both cache types; with a 16-bit cache bit for bit
    forward_varlen(cu_seqlens_k=, window_size=, softcap=) on the same keys packed.  A bad window_size is reported first, then a bad
    softcap, both a ValueError before any tensor is looked at."""
    return flash_attention_kernels.forward_varlen_kvcache(q, k_cache, v_cache, cu_seqlens_q, max_seqlen_q, cache_seqlens,
                                                          block_table=block_table, causal=causal, max_seqlen_k=max_seqlen_k, timed=timed,
                                                          k_descale=k_descale, v_descale=v_descale, window_size=window_size, softcap=softcap)


def append_kvcache(k_cache, v_cache, k, v, cache_seqlens, block_table=None, q=None, rotary_cos=None, rotary_sin=None,
                   rotary_interleaved=False, causal=False, k_descale=None, v_descale=None, seqlens_out=None):
    """The step in front of a decode, one HIP kernel: write the new rows k, v (batch, seqlen_new, n_kv_heads, 128)
    into the cache IN PLACE at positions cache_seqlens[b] + t -- contiguous, or paged through block_table; a token past the
    capacity is dropped -- rotating the new keys, and q into a new tensor, with rotary_cos / rotary_sin (seqlen_ro, rotary_dim / 2;
    rotary_interleaved pairs (2 i, 2 i + 1), else (i, i + rotary_dim / 2); bit-identical to fp32 eager torch rounded once), and
    quantizing for a torch.float8_e4m3fn cache with k_descale / v_descale (the bytes quantize_kvcache_fp8's expression gives).
    q row i takes position cache_seqlens[b] + i with causal, else cache_seqlens[b].  min(cache_seqlens + seqlen_new, capacity) goes to
    seqlens_out: None allocates it, cache_seqlens itself advances in place.  -> (seqlens_out, q_rot or None).  The host reads no
    device array; graph-capturable."""
    return flash_attention_kernels.append_kvcache(k_cache, v_cache, k, v, cache_seqlens, block_table=block_table, q=q,
                                                  rotary_cos=rotary_cos, rotary_sin=rotary_sin, rotary_interleaved=rotary_interleaved,
                                                  causal=causal, k_descale=k_descale, v_descale=v_descale, seqlens_out=seqlens_out)


def quantize_kvcache_fp8(k, v):
    """A contiguous 16-bit cache (batch, seqlen_cache, n_kv_heads, 128) -> (k8, v8, k_descale, v_descale) for forward_kvcache:
    torch.float8_e4m3fn caches and fp32 (batch, n_kv_heads) descales, amax / 448 per (batch entry, K / V head), 1 for an all-zero
    head.  Plain torch."""
    return flash_attention_kernels.quantize_kvcache_fp8(k, v)


def backward_varlen(q, k, v, o, lse, dout, cu_seqlens, max_seqlen, causal=False, timed=False, cu_seqlens_k=None, max_seqlen_k=None):
    """dQ, dK, dV over packed sequences from forward_varlen's o and lse -> (dq, dk, dv[, ms]).  Deterministic.
    cu_seqlens_k / max_seqlen_k (both or neither): separate K / V lengths as in forward_varlen, causal bottom-right aligned; a
    row that saw no key gets dq = 0, a key no query sees gets dk = dv = 0 (written, not skipped)."""
    return flash_attention_kernels.backward_varlen(q, k, v, o, lse, dout, cu_seqlens, max_seqlen, causal=causal, timed=timed,
                                                   cu_seqlens_k=cu_seqlens_k, max_seqlen_k=max_seqlen_k)


def backward_varlen_window(q, k, v, o, lse, dout, cu_seqlens, max_seqlen, window_size, causal=False, timed=False, cu_seqlens_k=None,
                           max_seqlen_k=None):
    """backward_varlen for forward_varlen(window_size=)'s o and lse, under the same window: row r at position
    p = r + (len_k - len_q) sees the keys max(0, p - left) .. min(len_k - 1, p + right), causal means right = 0.  (-1, -1) is
    backward_varlen, unchanged; bad values are a ValueError.  A row that sees no key gets dq = 0; a key no row sees -- below
    every row's floor or above every row's ceiling -- gets dk = dv = 0, written.  Deterministic."""
    return flash_attention_kernels.backward_varlen_window(q, k, v, o, lse, dout, cu_seqlens, max_seqlen, window_size, causal=causal,
                                                          timed=timed, cu_seqlens_k=cu_seqlens_k, max_seqlen_k=max_seqlen_k)


def backward_varlen_softcap(q, k, v, o, lse, dout, cu_seqlens, max_seqlen, softcap, window_size=(-1, -1), causal=False, timed=False,
                            cu_seqlens_k=None, max_seqlen_k=None):
    """The backward of forward_varlen(softcap=[, window_size=]): dQ, dK, dV from that forward's o and lse under the same softcap and
    window.  With t = tanh(s / softcap): dS = P (dP - delta) (1 - t^2).  softcap == 0 is backward_varlen_window
    with the same arguments, unchanged; bad values are a ValueError.  A row that sees no key gets dq = 0; a key no row sees gets
    dk = dv = 0, written.  Deterministic."""
    return flash_attention_kernels.backward_varlen_softcap(q, k, v, o, lse, dout, cu_seqlens, max_seqlen, softcap, window_size,
                                                           causal=causal, timed=timed, cu_seqlens_k=cu_seqlens_k,
                                                           max_seqlen_k=max_seqlen_k)


def forward_varlen_sinks(q, k, v, cu_seqlens, max_seqlen, sinks, causal=False, timed=False, cu_seqlens_k=None, max_seqlen_k=None, *,
                         window_size=(-1, -1)):
    """forward_varlen with learned attention sinks (gpt-oss's `sinks`, flash-attn's learnable_sink): sinks is a
    contiguous fp32 (n_heads,) tensor on q's device, one logit z per QUERY head that joins the softmax's denominator and has no
    value vector -- lse = log(exp(z) + sum_j exp(s_j)), o = sum_j exp(s_j - lse) v_j over the keys the row sees.  Every other
    argument is forward_varlen's (no softcap).  A row that sees no key gives o = 0 and lse = z; z = -inf means no sink for that
    head.  -> (o, lse[, ms]).  A bad window_size is a ValueError, a bad sinks a RuntimeError.  Without sinks, call forward_varlen."""
    return flash_attention_kernels.forward_varlen_sinks(q, k, v, cu_seqlens, max_seqlen, sinks, causal=causal, timed=timed,
                                                        cu_seqlens_k=cu_seqlens_k, max_seqlen_k=max_seqlen_k, window_size=window_size)


def backward_varlen_sinks(q, k, v, o, lse, dout, cu_seqlens, max_seqlen, sinks, window_size=(-1, -1), causal=False, timed=False,
                          cu_seqlens_k=None, max_seqlen_k=None):
    """The backward of forward_varlen_sinks: dQ, dK, dV and dsinks from that forward's o and lse under the same sinks and window
     -> (dq, dk, dv, dsinks[, ms]), dsinks fp32 of shape (n_heads,).  dQ, dK, dV are backward_varlen_window's
    kernels on the lse that holds the sink; dsinks[h] = - sum_rows exp(sinks[h] - lse[h, row]) delta[h, row].  A row that sees no
    key gets dq = 0; a key no row sees gets dk = dv = 0, written; sinks[h] = -inf gives dsinks[h] = 0.  Deterministic."""
    return flash_attention_kernels.backward_varlen_sinks(q, k, v, o, lse, dout, cu_seqlens, max_seqlen, sinks, window_size,
                                                         causal=causal, timed=timed, cu_seqlens_k=cu_seqlens_k, max_seqlen_k=max_seqlen_k)


def _varlen_needs_copy(t):
    return t.stride(2) != 1 or t.stride(0) % 8 != 0 or t.stride(1) % 8 != 0 or t.data_ptr() % 16 != 0


class _AttentionVarlen(torch.autograd.Function):
    @staticmethod
    def forward(ctx, q, k, v, cu_seqlens, max_seqlen, causal, cu_seqlens_k, max_seqlen_k, window_size=(-1, -1), softcap=0.0):
        if _varlen_needs_copy(q):
            q = q.contiguous()
        if _varlen_needs_copy(k) or _varlen_needs_copy(v) or v.stride() != k.stride():
            k, v = k.contiguous(), v.contiguous()
        o, lse = forward_varlen(q, k, v, cu_seqlens, max_seqlen, causal=causal, cu_seqlens_k=cu_seqlens_k, max_seqlen_k=max_seqlen_k,
                                window_size=window_size, softcap=softcap)
        ctx.qk = cu_seqlens_k is not None
        if ctx.qk:
            ctx.save_for_backward(q, k, v, o, lse, cu_seqlens, cu_seqlens_k)
        else:
            ctx.save_for_backward(q, k, v, o, lse, cu_seqlens)
        ctx.max_seqlen, ctx.max_seqlen_k, ctx.causal, ctx.window_size = max_seqlen, max_seqlen_k, causal, tuple(window_size)
        ctx.softcap = softcap
        return o

    @staticmethod
    def backward(ctx, dout):
        q, k, v, o, lse, cu_seqlens = ctx.saved_tensors[:6]
        cu_seqlens_k = ctx.saved_tensors[6] if ctx.qk else None
        # (softcap 0: backward_varlen_window itself; (-1, -1) as well: backward_varlen itself)
        dq, dk, dv = backward_varlen_softcap(q, k, v, o, lse, dout.contiguous(), cu_seqlens, ctx.max_seqlen, ctx.softcap, ctx.window_size,
                                             causal=ctx.causal, cu_seqlens_k=cu_seqlens_k, max_seqlen_k=ctx.max_seqlen_k)
        return dq, dk, dv, None, None, None, None, None, None, None


def attention_varlen(q, k, v, cu_seqlens, max_seqlen, causal=False, cu_seqlens_k=None, max_seqlen_k=None, *, window_size=(-1, -1),
                     softcap=0.0):
    """softmax(q k^T / sqrt d) v over packed sequences, with gradients (flash-attn's flash_attn_varlen_func): the varlen forward
    with the row log-sum-exp and the varlen HIP backward.  k and v may have n_kv_heads heads.

    cu_seqlens_k / max_seqlen_k (both or neither: one alone is a ValueError) give K / V lengths of their own -- cross-attention,
    chunked prefill behind a prefix: cu_seqlens / max_seqlen are then Q's, k / v are (total_k, n_kv_heads, 128), and causal is
    bottom-right aligned: query r of a sequence sees keys j <= r + (len_k - len_q).  A row that sees no key gives o = 0 and
    dq = 0; a key no query sees gets dk = dv = 0.  Both offset arrays are saved for the backward.

    window_size=(left, right), keyword only: forward_varlen's sliding window, carried to both passes (the windowed forward and
    backward_varlen_window), so a model with local layers trains by the rule it is served by.  Bad values are a ValueError before
    any tensor is looked at; (-1, -1) is the call above, bit for bit.

    softcap, keyword only: forward_varlen's logit soft-capping, carried to both passes (the soft-capped forward and
    backward_varlen_softcap), with or without a window.  Bad values are a ValueError before any tensor is looked at (a bad window
    first); 0 is the call above, bit for bit."""
    flash_attention_kernels._window(window_size, causal)
    flash_attention_kernels._softcap(softcap)
    if (cu_seqlens_k is None) != (max_seqlen_k is None):
        raise ValueError("cu_seqlens_k and max_seqlen_k go together: give both (separate Q and K / V lengths) or neither")
    return _AttentionVarlen.apply(q, k, v, cu_seqlens, max_seqlen, causal, cu_seqlens_k, max_seqlen_k, tuple(window_size), softcap)


class _AttentionVarlenSinks(torch.autograd.Function):
    @staticmethod
    def forward(ctx, q, k, v, sinks, cu_seqlens, max_seqlen, causal, cu_seqlens_k, max_seqlen_k, window_size=(-1, -1)):
        if _varlen_needs_copy(q):
            q = q.contiguous()
        if _varlen_needs_copy(k) or _varlen_needs_copy(v) or v.stride() != k.stride():
            k, v = k.contiguous(), v.contiguous()
        o, lse = forward_varlen_sinks(q, k, v, cu_seqlens, max_seqlen, sinks, causal=causal, cu_seqlens_k=cu_seqlens_k,
                                      max_seqlen_k=max_seqlen_k, window_size=window_size)
        ctx.qk = cu_seqlens_k is not None
        if ctx.qk:
            ctx.save_for_backward(q, k, v, o, lse, sinks, cu_seqlens, cu_seqlens_k)
        else:
            ctx.save_for_backward(q, k, v, o, lse, sinks, cu_seqlens)
        ctx.max_seqlen, ctx.max_seqlen_k, ctx.causal, ctx.window_size = max_seqlen, max_seqlen_k, causal, tuple(window_size)
        return o

    @staticmethod
    def backward(ctx, dout):
        q, k, v, o, lse, sinks, cu_seqlens = ctx.saved_tensors[:7]
        cu_seqlens_k = ctx.saved_tensors[7] if ctx.qk else None
        dq, dk, dv, dsinks = backward_varlen_sinks(q, k, v, o, lse, dout.contiguous(), cu_seqlens, ctx.max_seqlen, sinks, ctx.window_size,
                                                   causal=ctx.causal, cu_seqlens_k=cu_seqlens_k, max_seqlen_k=ctx.max_seqlen_k)
        return dq, dk, dv, dsinks, None, None, None, None, None, None


def attention_varlen_sinks(q, k, v, cu_seqlens, max_seqlen, sinks, causal=False, cu_seqlens_k=None, max_seqlen_k=None, *,
                           window_size=(-1, -1)):
    """attention_varlen with learned attention sinks, with gradients for q, k, v AND sinks (gpt-oss's attention): the
    forward and backward of forward_varlen_sinks / backward_varlen_sinks under one window.  sinks: (n_heads,) on q's device, fp32 or
    q's dtype -- a 16-bit parameter is converted to fp32 here, outside the autograd function, so its gradient comes back in its own
    dtype.  Every other argument is attention_varlen's (no softcap).  A bad window_size is a ValueError before any tensor is looked
    at, a bad sinks a RuntimeError.  Without sinks, call attention_varlen."""
    flash_attention_kernels._window(window_size, causal)
    if (cu_seqlens_k is None) != (max_seqlen_k is None):
        raise ValueError("cu_seqlens_k and max_seqlen_k go together: give both (separate Q and K / V lengths) or neither")
    if isinstance(sinks, torch.Tensor) and isinstance(q, torch.Tensor) and sinks.dtype == q.dtype and sinks.dtype != torch.float32:
        sinks = sinks.float()
    if isinstance(sinks, torch.Tensor) and sinks.dim() == 1 and not sinks.is_contiguous():
        sinks = sinks.contiguous()
    flash_attention_kernels._check_sinks(sinks, q)
    return _AttentionVarlenSinks.apply(q, k, v, sinks, cu_seqlens, max_seqlen, causal, cu_seqlens_k, max_seqlen_k, tuple(window_size))
