"""Layouts that put a small attention problem at byte offsets beyond 2 GiB and 4 GiB (the tests are
tests/test_large_offsets_cpu.py and tests/test_large_offsets_gpu.py).

The principle: a small problem sits inside a large allocation so that the rows a launch names lie on both sides of the 2^31 and
the 2^32 BYTE marks of each tensor; whatever the launch does not name holds poison (NaN in 16-bit inputs, the NaN code 0x7f in
fp8 bytes, a sentinel in outputs).  The result has to equal, bit for bit, the same call on a COMPACT copy of the same rows,
renumbered -- the library's own small-offset result, which the rest of the suite compares with fp32 eager.

This module knows shapes, strides, tables and row numbers only: it imports nothing of the code under test and allocates nothing
but small index arrays.  Every layout is a dict with
    "tensors": {name: Tensor}   the large tensors, each with the rows it names in the large and in the compact form;
    "bytes":   {name: int}      every device allocation of a test on the layout (large, compact, outputs, temporaries);
and the numbers a test needs to build both forms."""
import random
from dataclasses import dataclass

import numpy as np

GIB = 1 << 30
MARK31, MARK32 = 1 << 31, 1 << 32
BUDGET = 24 * GIB          # no GPU test allocates more (what the dense 4 GiB test already wants free)
HEADROOM = 2 * GIB         # a test skips only with less than its bytes + this free
D = 128
NAN16 = 0x7FC0             # a NaN in bf16 and in fp16
NAN8 = 0x7F                # e4m3fn's NaN
PAIRS = ((300, 300), (129, 300), (257, 130), (64, 1))   # (len_q, len_k) of the real sequences, in turn
ROW_STRIDE_BYTES = 4096    # the token stride of the strided K / V views (a slice of a wider head axis)


@dataclass
class Tensor:
    """One large tensor: `rows` are the row numbers (units of row_bytes from the base) the launch names, `compact_rows` the same
    rows in the compact form, in the same order.  nbytes / compact_nbytes: the two allocations."""
    nbytes: int
    row_bytes: int
    rows: np.ndarray
    compact_rows: np.ndarray
    compact_nbytes: int
    compact_row_bytes: int = 0   # 0: row_bytes (a strided view's compact form is contiguous: a shorter row)

    def offsets(self):
        return self.rows.astype(np.int64) * self.row_bytes


def region(offsets):
    """0 below 2^31, 1 in [2^31, 2^32), 2 at or above 2^32"""
    offsets = np.asarray(offsets, dtype=np.int64)
    return (offsets >= MARK31).astype(np.int64) + (offsets >= MARK32)


def as_uint32(offsets):
    return np.asarray(offsets, dtype=np.int64) & 0xFFFFFFFF


def as_int32(offsets):
    low = as_uint32(offsets)
    return np.where(low >= MARK31, low - MARK32, low)


def item_marks(n_items, item_bytes):
    """The items (pages, batch entries, samples: item_bytes bytes each, back to back) at the six marks of an allocation -- the
    first, the last wholly below 2 GiB, the first at or above it, the same two at 4 GiB, the last -- and the one that straddles a
    mark where item_bytes does not divide it.  Sorted, without repeats, only those the allocation has."""
    out = {0, n_items - 1}
    for mark in (MARK31, MARK32):
        out.update((mark // item_bytes - 1, -(-mark // item_bytes)))
        if mark % item_bytes:
            out.add(mark // item_bytes)
    return sorted(i for i in out if 0 <= i < n_items)


# ---- K / V caches ---------------------------------------------------------------------------------------------------------------

def paged_pool(page_size, elem_bytes=2, n_kv=2, batch=4, pages_per_seq=6, seed=0):
    """(num_pages, page_size, n_kv, 128), about 5 GiB per cache.  block_table (batch, pages_per_seq) picks the pages at the marks
    and filler pages from all three regions, shuffled; the compact pool holds exactly the used pages, its table their ranks."""
    page_bytes = page_size * n_kv * D * elem_bytes
    num_pages = 5 * GIB // page_bytes
    marks = item_marks(num_pages, page_bytes)
    rng = random.Random(1000 * seed + page_size + elem_bytes)
    edges = (0, MARK31 // page_bytes, MARK32 // page_bytes, num_pages)
    used = list(marks)
    reg = 0
    while len(used) < batch * pages_per_seq:
        p = rng.randrange(edges[reg], edges[reg + 1])
        if p not in used:
            used.append(p)
            reg = (reg + 1) % 3
    rng.shuffle(used)
    table = [used[b * pages_per_seq:(b + 1) * pages_per_seq] for b in range(batch)]
    rank = {p: i for i, p in enumerate(sorted(used))}
    ragged = (0, 13, 1, page_size - 1)
    lens = [pages_per_seq * page_size - ragged[b % 4] for b in range(batch)]
    rows = np.array([p * page_size + r for row in table for p in row for r in range(page_size)], dtype=np.int64)
    crow = np.array([rank[p] * page_size + r for row in table for p in row for r in range(page_size)], dtype=np.int64)
    nbytes, cbytes = num_pages * page_bytes, len(used) * page_bytes
    t = Tensor(nbytes, page_bytes // page_size, rows, crow, cbytes)
    return dict(kind="paged", name=f"paged{page_size}x{elem_bytes}", page_size=page_size, num_pages=num_pages, n_kv=n_kv, batch=batch,
                elem_bytes=elem_bytes, table=table, compact_table=[[rank[p] for p in row] for row in table], used=sorted(used),
                marks=marks, cache_seqlens=lens, shape=(num_pages, page_size, n_kv, D), compact_shape=(len(used), page_size, n_kv, D),
                strides=(page_size * n_kv * D, n_kv * D, D, 1), tensors={"k_cache": t, "v_cache": t},
                bytes={"k_cache": nbytes, "v_cache": nbytes, "compact": 2 * cbytes, "check": nbytes // 8})


def append_plan(lay, new=4):
    """What the append test writes into a paged or batch-stride layout: `before`, the lengths in front of the append, and the
    cache rows that `new` tokens per entry land on, large and compact (units of the layout's row).  On a paged pool every entry
    writes two rows on either side of a page boundary of its table, the boundary chosen entry by entry so that the written pages
    come from all three regions of the pool (the test on the CPU asserts that they do)."""
    t = lay["tensors"]["k_cache"]
    before, rows, crow = [], [], []
    if lay["kind"] == "batch":
        before = list(lay["cache_seqlens"])
        for b, n in enumerate(before):
            rows += [b * lay["seqlen_cache"] + n + i for i in range(new)]
            crow += [b * lay["compact_seqlen"] + n + i for i in range(new)]
    else:
        ps, covered = lay["page_size"], set()
        page_region = lambda p: int(region([p * ps * t.row_bytes])[0])   # noqa: E731
        for large_row, compact_row in zip(lay["table"], lay["compact_table"]):
            gain = [len({page_region(large_row[c - 1]), page_region(large_row[c])} - covered) for c in range(1, len(large_row))]
            c = max(range(1, len(large_row)), key=lambda c: (gain[c - 1], c))
            covered |= {page_region(large_row[c - 1]), page_region(large_row[c])}
            before.append(c * ps - new // 2)
            for i in range(new):
                pos = before[-1] + i
                rows.append(large_row[pos // ps] * ps + pos % ps)
                crow.append(compact_row[pos // ps] * ps + pos % ps)
    return dict(before=before, new=new, rows=np.array(rows, dtype=np.int64), compact_rows=np.array(crow, dtype=np.int64))


def batch_stride_cache(elem_bytes=2, n_kv=2, batch=42, compact_seqlen=256):
    """(batch, seqlen_cache, n_kv, 128) with batch * the batch stride past 4 GiB and short cache_seqlens; an entry is 128 MB,
    which divides neither mark, so one entry straddles each.  The compact form has a small seqlen_cache."""
    seqlen_cache = 128_000_000 // (n_kv * D * elem_bytes)
    row_bytes = n_kv * D * elem_bytes
    entry_bytes = seqlen_cache * row_bytes
    lens = [1 + (b * 37) % (compact_seqlen - 8) for b in range(batch)]
    lens[0], lens[-1] = compact_seqlen - 8, 200
    rows = np.array([b * seqlen_cache + j for b in range(batch) for j in range(lens[b])], dtype=np.int64)
    crow = np.array([b * compact_seqlen + j for b in range(batch) for j in range(lens[b])], dtype=np.int64)
    nbytes, cbytes = batch * entry_bytes, batch * compact_seqlen * row_bytes
    t = Tensor(nbytes, row_bytes, rows, crow, cbytes)
    return dict(kind="batch", name=f"batch{elem_bytes}", batch=batch, n_kv=n_kv, elem_bytes=elem_bytes, seqlen_cache=seqlen_cache,
                compact_seqlen=compact_seqlen, cache_seqlens=lens, marks=item_marks(batch, entry_bytes),
                shape=(batch, seqlen_cache, n_kv, D), compact_shape=(batch, compact_seqlen, n_kv, D),
                strides=(seqlen_cache * n_kv * D, n_kv * D, D, 1), tensors={"k_cache": t, "v_cache": t},
                bytes={"k_cache": nbytes, "v_cache": nbytes, "compact": 2 * cbytes, "check": nbytes // 8})


def long_entry_cache(elem_bytes=2, n_kv=2, keys=1_100_000):
    """One entry whose own keys pass 4 GiB: (1, keys, n_kv, 128) as a view with a 4 KiB row stride (a slice of a wider head
    axis).  The compact form is the contiguous copy."""
    row_elems = ROW_STRIDE_BYTES // elem_bytes
    rows = np.arange(keys, dtype=np.int64)
    nbytes, cbytes = keys * ROW_STRIDE_BYTES, keys * n_kv * D * elem_bytes
    t = Tensor(nbytes, ROW_STRIDE_BYTES, rows, rows, cbytes, n_kv * D * elem_bytes)
    return dict(kind="long", name=f"long{elem_bytes}", batch=1, n_kv=n_kv, elem_bytes=elem_bytes, keys=keys, cache_seqlens=[keys - 77],
                shape=(1, keys, n_kv, D), compact_shape=(1, keys, n_kv, D), strides=(keys * row_elems, row_elems, D, 1),
                tensors={"k_cache": t, "v_cache": t},
                bytes={"k_cache": nbytes, "v_cache": nbytes, "compact": 2 * cbytes, "staging": 4 * keys * n_kv * D})


# ---- packed sequences -------------------------------------------------------------------------------------------------------------

def _placed(total_rows, row_bytes, lens):
    """Start rows of seven sequences of `lens` rows at the marks of a (total_rows, row_bytes) tensor: the first rows; the last
    sequence wholly below 2 GiB and the first at or above it; a sequence that straddles 4 GiB with the last wholly below and the
    first wholly above it on either side; the last rows."""
    assert len(lens) == 7
    r31_lo, r31_hi = MARK31 // row_bytes, -(-MARK31 // row_bytes)
    s4 = MARK32 // row_bytes - max(lens[4] // 2, 1)
    starts = [0, r31_lo - lens[1], r31_hi, s4 - lens[3], s4, s4 + lens[4], total_rows - lens[6]]
    ends = [s + n for s, n in zip(starts, lens)]
    assert all(e <= s for e, s in zip(ends, starts[1:])) and ends[-1] == total_rows and (lens[4] < 2 or starts[4] * row_bytes < MARK32 < ends[4] * row_bytes)
    return starts


def packed(side, heads=(16, 2), max_filler=131072, strided_kv=None, placement=None, name=None):
    """Packed sequences with one side large.  side "q": q, o, dout, dq (total_q, H, 128) contiguous, past 4 GiB, the real sequences
    (PAIRS in turn) at the marks of Q and between them fillers of (len_q large, len_k = 0) -- rows that see no key; K / V hold
    the real keys only.  side "k": k, v, dk, dv as views with a 4 KiB token stride, the real sequences at the marks of K and
    fillers of (0, len_k large) -- keys no row sees; Q holds the real rows only.  side "one": one range for both sides, so a filler
    is a sequence of max_filler rows AND keys (its inputs are poison and its results are not compared) and a real one has PAIRS'
    len_q on both sides; K / V contiguous.
    The compact form keeps every sequence and both bounds (so the grids and the backward's dK / dV split agree) and gives the
    fillers length 0.  placement = (rows of the large side, the real pairs, their start rows) replaces the marks of the side's
    own tensor (packed_workspace: the marks of the backward's workspace)."""
    hq, hk = heads
    strided = side == "k" if strided_kv is None else strided_kv
    q_row, k_row = hq * D * 2, (ROW_STRIDE_BYTES if strided else hk * D * 2)
    real = [PAIRS[i % 4] for i in range(7)]
    if side == "one":   # (one range: a sequence's keys are its rows)
        real = [(lq, lq) for lq, _ in real]
    big_row = k_row if side == "k" else q_row
    total_big = (MARK32 + 64 * (1 << 20)) // big_row
    which = 1 if side == "k" else 0
    starts = _placed(total_big, big_row, [p[which] for p in real]) if placement is None else None
    if placement is not None:
        total_big, real, starts = placement
    seqs, pos = [], 0    # (len_q, len_k, real index or None)
    for i, (s, pair) in enumerate(zip(starts, real)):
        gap = s - pos
        while gap > 0:
            g = min(gap, max_filler)
            seqs.append({"q": (g, 0, None), "k": (0, g, None), "one": (g, g, None)}[side])
            gap -= g
        seqs.append((pair[0], pair[1], i))
        pos = s + pair[which]
    assert pos == total_big
    cu = {n: [0] for n in ("q", "k", "cq", "ck")}
    for lq, lk, i in seqs:
        cu["q"].append(cu["q"][-1] + lq)
        cu["k"].append(cu["k"][-1] + lk)
        cu["cq"].append(cu["cq"][-1] + (lq if i is not None else 0))
        cu["ck"].append(cu["ck"][-1] + (lk if i is not None else 0))
    idx = [j for j, s in enumerate(seqs) if s[2] is not None]

    def rows(c, lens_at):
        return np.concatenate([np.arange(c[j], c[j] + seqs[j][lens_at], dtype=np.int64) for j in idx])
    total_q, total_k, ctq, ctk = cu["q"][-1], cu["k"][-1], cu["cq"][-1], cu["ck"][-1]
    tq = Tensor(total_q * q_row, q_row, rows(cu["q"], 0), rows(cu["cq"], 0), ctq * q_row)
    tk = Tensor(total_k * k_row, k_row, rows(cu["k"], 1), rows(cu["ck"], 1), ctk * hk * D * 2, hk * D * 2)
    lse = 4 * hq * total_q
    nb = {"q": tq.nbytes, "o": tq.nbytes, "k": tk.nbytes, "v": tk.nbytes, "lse": lse, "compact": 4 * tq.compact_nbytes + 4 * tk.compact_nbytes}
    fwd_bytes = dict(nb, check=max(tq.nbytes, tk.nbytes) // 2)
    bwd_bytes = dict(nb, dout=tq.nbytes, dq=tq.nbytes, dk=tk.nbytes, dv=tk.nbytes, workspace=lse + (1 << 28), check=max(tq.nbytes, tk.nbytes) // 2)
    return dict(kind="packed", name=name or f"packed-{side}-{hq}x{hk}", side=side, heads=heads, seqs=seqs, real=idx, strided_kv=strided,
                cu_q=cu["q"], cu_k=cu["k"], compact_cu_q=cu["cq"], compact_cu_k=cu["ck"], total_q=total_q, total_k=total_k,
                compact_total_q=ctq, compact_total_k=ctk, max_q=max(max(s[0] for s in seqs), 1), max_k=max(max(s[1] for s in seqs), 1),
                q_strides=(hq * D, D, 1), k_strides=(k_row // 2, D, 1),
                tensors={"q": tq, "o": tq, "dout": tq, "dq": tq, "k": tk, "v": tk, "dk": tk, "dv": tk},
                bytes=bwd_bytes, forward_bytes=fwd_bytes)


def packed_workspace(heads=(37, 1), total_k=122_000, max_filler=1408):
    """The packed backward with its fp32 dK / dV partials past 4 GiB.  The split is the smallest divisor of the
    group that brings the key side's grid to 1024 workgroups under a causal mask, and the whole group where no divisor does: a
    prime group, (37, 1), with n_seqs * ceil(max_seqlen_k / 128) < 1024 runs with split 37, and the partials --
    n_kv_heads * split * total_k * 256 floats, part (hk * split + sp) of key row r at ((hk * split + sp) * total_k + r) * 1 KiB --
    pass 4 GiB at total_k = 122 000 while k, v, dk and dv stay 31 MB each.  The real sequences sit at the first and last key rows
    and straddle the rows whose part 17 / part 34 partials cross 2 GiB / 4 GiB; the fillers are keys no row sees."""
    hq, hk = heads
    real = [PAIRS[i] for i in range(4)]
    part_row = 2 * D * 4
    r31, r32 = (MARK31 // part_row) % total_k, (MARK32 // part_row) % total_k
    starts = [0, r31 - real[1][1] // 2, r32 - real[2][1] // 2, total_k - real[3][1]]
    lay = packed("k", heads, max_filler, strided_kv=False, placement=(total_k, real, starts), name=f"packed-workspace-{hq}x{hk}")
    split, tk = hq // hk, lay["tensors"]["k"]
    ctk = lay["compact_total_k"]
    ws = Tensor(hk * split * total_k * part_row, part_row,
                np.concatenate([sp * total_k + tk.rows for sp in range(hk * split)]),
                np.concatenate([sp * ctk + tk.compact_rows for sp in range(hk * split)]), hk * split * ctk * part_row)
    lay["tensors"] = dict(lay["tensors"], workspace=ws)
    lay["bytes"] = dict(lay["bytes"], workspace=ws.nbytes, delta=4 * hq * lay["total_q"] + 16, compact_workspace=ws.compact_nbytes)
    lay["split"] = split
    return lay


# ---- the dense and GQA backward ---------------------------------------------------------------------------------------------------

def dense_qkv(batch=800, seq_len=256, heads=(32, 32)):
    """q, k, v as slices of one packed (batch, seq_len, 3, H, 128) buffer of about 4.7 GiB; for GQA (heads (H, Hkv), Hkv < H) the
    K / V heads sit in a second (batch, seq_len, 2, Hkv, 128) buffer.  A sample is 6 MiB of the first buffer, which divides neither
    mark, so the samples at the marks include one straddling each.  o, dout and the gradients are contiguous.  The compact form
    is the marked samples gathered into one small batch."""
    hq, hk = heads
    sample = seq_len * 3 * hq * D * 2
    marks = item_marks(batch, sample)
    row_bytes = 3 * hq * D * 2
    rows = np.array([b * seq_len + r for b in marks for r in range(seq_len)], dtype=np.int64)
    crow = np.arange(len(marks) * seq_len, dtype=np.int64)
    t = Tensor(batch * sample, row_bytes, rows, crow, len(marks) * sample)
    out = batch * seq_len * hq * D * 2
    kv_out = batch * seq_len * hk * D * 2
    nb = {"qkv": t.nbytes, "o": out, "dout": out, "dq": out, "dk": kv_out, "dv": kv_out, "lse": 4 * batch * hq * seq_len,
          "workspace": 4 * batch * hq * seq_len + (1 << 28), "compact": 8 * t.compact_nbytes}
    if hk != hq:
        nb["kv"] = batch * seq_len * 2 * hk * D * 2
    return dict(kind="dense", name=f"dense-{hq}x{hk}", batch=batch, seq_len=seq_len, heads=heads, marks=marks,
                qkv_shape=(batch, seq_len, 3, hq, D), kv_shape=(batch, seq_len, 2, hk, D),
                qkv_strides=(seq_len * 3 * hq * D, 3 * hq * D, D, 1), kv_strides=(seq_len * 2 * hk * D, 2 * hk * D, D, 1),
                out_strides=(seq_len * hq * D, hq * D, D, 1), dkv_strides=(seq_len * hk * D, hk * D, D, 1),
                tensors={"qkv": t}, bytes=nb)


def all_layouts():
    """Every layout the GPU tests use, by name."""
    out = [paged_pool(64), paged_pool(256), paged_pool(64, 1), paged_pool(256, 1), batch_stride_cache(2), batch_stride_cache(1),
           long_entry_cache(2), long_entry_cache(1),
           packed("q"), packed("k"), packed("one", max_filler=1024), packed("q", (8, 2)), packed("k", (4, 4)),
           packed_workspace(), dense_qkv(), dense_qkv(heads=(32, 16))]
    return {lay["name"]: lay for lay in out}


def total_bytes(layout, which="bytes"):
    return sum(layout[which].values())
