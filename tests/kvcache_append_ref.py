"""The eager-torch statement of append_kvcache the append tests compare against: tests/test_kvcache_append_cpu.py
runs it on the CPU against hand-checked rows, tests/test_kvcache_append_gpu.py on the device against the kernel, bit for bit.
Host loops over the batch entries and the new tokens: a reference, not a fast path."""
import torch


def rotary_ref(x, cos, sin, rows, interleaved):
    """x (S, H, D) 16-bit, cos / sin (seqlen_ro, rotary_dim / 2) of x's dtype, rows: S table rows (already clamped) -> x rotated:
    o1 = x1 c - x2 s, o2 = x1 s + x2 c in fp32, each product and sum its own eager op (nothing fused), rounded once."""
    rd = 2 * cos.shape[1]
    idx = torch.as_tensor(rows, dtype=torch.long, device=x.device)
    c = cos[idx].float()[:, None, :]
    s = sin[idx].float()[:, None, :]
    xf = x.float()
    x1, x2 = (xf[..., 0:rd:2], xf[..., 1:rd:2]) if interleaved else (xf[..., :rd // 2], xf[..., rd // 2:rd])
    o1 = x1 * c - x2 * s
    o2 = x1 * s + x2 * c
    out = x.clone()
    if interleaved:
        out[..., 0:rd:2] = o1.to(x.dtype)
        out[..., 1:rd:2] = o2.to(x.dtype)
    else:
        out[..., :rd // 2] = o1.to(x.dtype)
        out[..., rd // 2:rd] = o2.to(x.dtype)
    return out


def quantize_ref(x, descale):
    """x (S, H, D) 16-bit, descale (H) fp32 or None -> e4m3fn: quantize_kvcache_fp8's expression with a given descale"""
    xf = x.float()
    if descale is not None:
        xf = xf / descale[None, :, None]
    return xf.clamp(-448.0, 448.0).to(torch.float8_e4m3fn)


def q_rows(length, seqlen_q, causal, seqlen_ro):
    """flash-attn's rule: query row i at position len + i with causal, else len; the table row is clamped to the last one"""
    return [min(length + i if causal else length, seqlen_ro - 1) for i in range(seqlen_q)]


def append_ref(k_cache, v_cache, k, v, lens, block_table=None, q=None, cos=None, sin=None, interleaved=False, causal=False,
               k_descale=None, v_descale=None):
    """-> (k_cache', v_cache', lens', q_rot or None) on clones; lens: a list of ints (the host's copy of cache_seqlens)."""
    kc, vc = k_cache.clone(), v_cache.clone()
    fp8 = kc.dtype == torch.float8_e4m3fn
    batch, seqlen_new = k.shape[0], k.shape[1]
    if block_table is None:
        capacity = kc.shape[1]
    else:
        page_size, num_pages = kc.shape[1], kc.shape[0]
        capacity = block_table.shape[1] * page_size
        table = block_table.tolist()
    out_lens, q_rot = [], (q.clone() if q is not None else None)
    for b in range(batch):
        length = min(max(int(lens[b]), 0), capacity)
        out_lens.append(min(length + seqlen_new, capacity))
        if q is not None:
            q_rot[b] = rotary_ref(q[b], cos, sin, q_rows(length, q.shape[1], causal, cos.shape[0]), interleaved)
        n = min(seqlen_new, capacity - length)
        if n <= 0:
            continue
        kb, vb = k[b, :n], v[b, :n]
        if cos is not None:
            kb = rotary_ref(kb, cos, sin, [min(length + t, cos.shape[0] - 1) for t in range(n)], interleaved)
        if fp8:
            kb = quantize_ref(kb, k_descale[b] if k_descale is not None else None)
            vb = quantize_ref(vb, v_descale[b] if v_descale is not None else None)
        for t in range(n):
            pos = length + t
            if block_table is None:
                page, row = b, pos
            else:
                page, row = min(max(table[b][pos // page_size], 0), num_pages - 1), pos % page_size
            # (through uint8 / int16 views: index assignment is not implemented for every float8 build)
            kc.view(torch.uint8 if fp8 else torch.int16)[page, row] = kb[t].view(torch.uint8 if fp8 else torch.int16)
            vc.view(torch.uint8 if fp8 else torch.int16)[page, row] = vb[t].view(torch.uint8 if fp8 else torch.int16)
    return kc, vc, out_lens, q_rot
