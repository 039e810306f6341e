"""The layouts of tests/large_offset_layouts.py, from shapes, strides and tables alone (nothing is allocated, nothing launches):
the rows each large tensor names fall on every side of the 2 GiB and 4 GiB byte marks it reaches, a 32-bit slip in an offset --
unsigned or signed -- moves at least one named row, the compact form names the same rows in the same order, no test allocates
more than 24 GiB, and the library's own host-side rules accept every stride and length (its *_workspace_bytes / *_num_splits
queries with fake non-null pointers, which validate and never launch; for the entry points that have no such query -- the append,
the prefill and the packed forward -- the rules of include/fa_hip.h restated)."""
import ctypes

import numpy as np
import pytest

from flash_attention_from_scratch_amd import _capi
from tests import large_offset_layouts as lo

LAYOUTS = lo.all_layouts()
IDS = dict(ids=str)
FAKE = 16   # a non-null, 16-byte aligned pointer no query follows


@pytest.mark.parametrize("name", list(LAYOUTS), **IDS)
def test_named_rows_lie_on_every_side_of_the_marks_each_tensor_reaches(name):
    lay = LAYOUTS[name]
    large = 0
    for tname, t in lay["tensors"].items():
        off = t.offsets()
        assert off.min() >= 0 and off.max() + 256 <= t.nbytes, (name, tname)
        want = {0} | ({1} if t.nbytes > lo.MARK31 else set()) | ({2} if t.nbytes > lo.MARK32 else set())
        assert set(np.unique(lo.region(off)).tolist()) == want, (name, tname, want)
        if t.nbytes <= lo.MARK32:
            continue
        large += 1
        # the rows next to each mark, and the ends, are named
        assert off.min() == 0, (name, tname)
        if lay["kind"] == "batch":
            assert t.nbytes - off.max() <= lay["seqlen_cache"] * t.row_bytes, (name, tname, "the last entry")
        else:
            assert off.max() == t.nbytes - t.row_bytes, (name, tname, "the last row")
        for mark in (lo.MARK31, lo.MARK32):
            below, above = off[off < mark].max(), off[off >= mark].min()
            if lay["kind"] == "batch":       # (an entry's short length starts at the entry's base)
                entry = lay["seqlen_cache"] * t.row_bytes
                assert mark - below < entry and above - mark < entry, (name, tname, mark)
            else:
                assert below == (mark - 1) // t.row_bytes * t.row_bytes and above == -(-mark // t.row_bytes) * t.row_bytes, (name, tname, mark)
        # the proof that a 32-bit slip moves a named row: an unsigned one, and a signed one
        assert (lo.as_uint32(off) != off).any() and (lo.as_int32(off) != off).any(), (name, tname)
        assert ((lo.as_int32(off) != off) & (lo.as_uint32(off) == off)).any(), (name, tname, "a row only a signed slip moves")
    assert large >= 1, name


@pytest.mark.parametrize("name", list(LAYOUTS), **IDS)
def test_compact_and_large_name_the_same_rows_in_the_same_order(name):
    lay = LAYOUTS[name]
    for tname, t in lay["tensors"].items():
        assert t.rows.shape == t.compact_rows.shape and len(np.unique(t.rows)) == len(t.rows), (name, tname)
        order = np.argsort(t.rows, kind="stable")
        assert (np.diff(t.compact_rows[order]) > 0).all(), (name, tname, "the renumbering keeps the order")
        assert t.compact_rows.min() == 0 and (t.compact_rows.max() + 1) * (t.compact_row_bytes or t.row_bytes) <= t.compact_nbytes, (name, tname)
        assert t.compact_nbytes < lo.MARK31 // 2, (name, tname)
    if lay["kind"] == "paged":
        used = lay["used"]
        assert [[used[r] for r in row] for row in lay["compact_table"]] == lay["table"]
        assert sorted(p for row in lay["table"] for p in row) == used and set(lay["marks"]) <= set(used)
        edges = (0, lo.MARK31 // (lay["tensors"]["k_cache"].row_bytes * lay["page_size"]), lo.MARK32 // (lay["tensors"]["k_cache"].row_bytes * lay["page_size"]))
        fillers = [p for p in used if p not in lay["marks"]]
        assert {sum(p >= e for e in edges) for p in fillers} == {1, 2, 3}, "filler pages from all three regions"
    if lay["kind"] == "packed":
        for cu, ccu in ((lay["cu_q"], lay["compact_cu_q"]), (lay["cu_k"], lay["compact_cu_k"])):
            assert len(cu) == len(ccu) == len(lay["seqs"]) + 1
            for j, (lq, lk, real) in enumerate(lay["seqs"]):
                if real is not None:
                    assert (cu[j + 1] - cu[j]) == (ccu[j + 1] - ccu[j])
                else:
                    assert ccu[j + 1] == ccu[j] and (lq == 0 or lay["side"] != "k") and (lk == 0 or lay["side"] != "q")
        want = [lo.PAIRS[i % 4] for i in range(len(lay["real"]))]
        assert [lay["seqs"][j][:2] for j in lay["real"]] == ([(lq, lq) for lq, _ in want] if lay["side"] == "one" else want)
        if lay["side"] == "one":
            assert lay["cu_q"] == lay["cu_k"] and lay["compact_cu_q"] == lay["compact_cu_k"]


@pytest.mark.parametrize("name", list(LAYOUTS), **IDS)
def test_every_layout_stays_inside_the_byte_budget(name):
    lay = LAYOUTS[name]
    for which in ("bytes", "forward_bytes"):
        if which in lay:
            assert lo.total_bytes(lay, which) <= lo.BUDGET, (name, which, lo.total_bytes(lay, which) / lo.GIB)
    for tname, t in lay["tensors"].items():
        assert any(v == t.nbytes for v in lay["bytes"].values()), (name, tname, "a declared allocation")


def test_item_marks_names_the_six_positions_and_the_straddlers():
    assert lo.item_marks(163840, 32768) == [0, 65535, 65536, 131071, 131072, 163839]      # (a page divides both marks)
    got = lo.item_marks(800, 6291456)
    assert got == [0, 340, 341, 342, 681, 682, 683, 799]
    assert 341 * 6291456 < lo.MARK31 < 342 * 6291456 and 682 * 6291456 < lo.MARK32 < 683 * 6291456
    assert lo.item_marks(3, 1 << 20) == [0, 2]
    assert lo.as_int32([lo.MARK31, lo.MARK32 + 5, 7]).tolist() == [-lo.MARK31, 5, 7]
    assert lo.as_uint32([lo.MARK31, lo.MARK32 + 5, 7]).tolist() == [lo.MARK31, 5, 7]
    assert lo.region([0, lo.MARK31 - 1, lo.MARK31, lo.MARK32 - 1, lo.MARK32]).tolist() == [0, 0, 1, 1, 2]


# ---- the library's host-side rules ------------------------------------------------------------------------------------------

def _stride_rules(strides, unit):
    """include/fa_hip.h: every stride but the last a multiple of 16 bytes, the last one 1"""
    assert strides[-1] == 1 and all(s > 0 and s % unit == 0 for s in strides[:-1]), strides


def _packed_rule(seq_stride):
    """... and a packed tensor's token stride: 256 rows * seq_stride * 2 bytes fit 32 bits"""
    assert 0 < seq_stride <= 0xFFFFFFFF // (2 * 256) and seq_stride % 8 == 0, seq_stride


def _decode_struct(lay, compact, seqlen_q, num_splits, n_heads=8):
    fp8 = lay["elem_bytes"] == 1
    shape = lay["compact_shape"] if compact else lay["shape"]
    strides = lay["strides"]
    if compact:
        strides = (shape[1] * shape[2] * shape[3], shape[2] * shape[3], shape[3], 1)
    f = dict(dtype=15, causal=0, num_splits=num_splits, q=FAKE, k=FAKE, v=FAKE, o=FAKE, lse=FAKE, cache_seqlens=FAKE, workspace=FAKE,
             batch=lay["batch"], seqlen_q=seqlen_q, n_heads=n_heads, n_kv_heads=lay["n_kv"], q_batch_stride=seqlen_q * n_heads * 128,
             q_seq_stride=n_heads * 128, q_head_stride=128, o_batch_stride=seqlen_q * n_heads * 128, o_seq_stride=n_heads * 128,
             o_head_stride=128, kv_batch_stride=strides[0], kv_seq_stride=strides[1], kv_head_stride=strides[2],
             max_seqlen_k=max(lay["cache_seqlens"]))   # (as the GPU tests pass it: the split rule then reads the same bound in both forms)
    if lay["kind"] == "paged":
        width = len(lay["table"][0])
        f.update(block_table=FAKE, num_pages=shape[0], page_size=shape[1], max_pages_per_seq=width, block_table_stride=width)
    else:
        f.update(seqlen_cache=shape[1])
    if fp8:
        return _capi.make_decode_fp8_args(k_descale=FAKE, v_descale=FAKE, descale_batch_stride=lay["n_kv"], **f)
    return _capi.make_decode_args(**f)


KV_LAYOUTS = [n for n, lay in LAYOUTS.items() if lay["kind"] in ("paged", "batch", "long")]


@pytest.mark.parametrize("name", KV_LAYOUTS, **IDS)
def test_the_decode_queries_accept_every_cache_layout(name):
    lay, lib = LAYOUTS[name], _capi.load()
    fp8 = lay["elem_bytes"] == 1
    plain, windowed = ((lib.fa_decode_fp8_workspace_bytes, lib.fa_decode_fp8_window_workspace_bytes) if fp8 else
                       (lib.fa_decode_workspace_bytes, lib.fa_decode_window_workspace_bytes))
    splits, wsplits = ((lib.fa_decode_fp8_num_splits, lib.fa_decode_fp8_window_num_splits) if fp8 else
                       (lib.fa_decode_num_splits, lib.fa_decode_window_num_splits))
    served, wserved = ((lib.fa_decode_fp8_supported, lib.fa_decode_fp8_window_supported) if fp8 else
                       (lib.fa_decode_supported, lib.fa_decode_window_supported))
    w = _capi.make_window(100, 0)
    for seqlen_q in (1, 4):
        for num_splits in (0, 3):
            got = []
            for compact in (False, True):
                a = _decode_struct(lay, compact, seqlen_q, num_splits)
                assert plain(ctypes.byref(a)) >= 0, (name, compact, _capi.last_error())
                assert served(ctypes.byref(a)) == 1 and wserved(ctypes.byref(a), ctypes.byref(w)) == 1, (name, compact)
                assert windowed(ctypes.byref(a), ctypes.byref(w)) >= 0, (name, compact, _capi.last_error())
                got.append((splits(ctypes.byref(a)), wsplits(ctypes.byref(a), ctypes.byref(w))))
            assert got[0] == got[1] and got[0][0] >= 1, (name, seqlen_q, num_splits, got, "one split count in both forms")
    # the rules of the entry points without a query (the append and the prefill), restated
    _stride_rules(lay["strides"], 16 if fp8 else 8)
    if lay["kind"] == "paged":
        assert lay["page_size"] % 64 == 0 and lay["num_pages"] <= (2 ** 31 - 1) // 2
        assert lay["num_pages"] * len(lay["table"][0]) > 0 and len(lay["table"][0]) * lay["page_size"] <= (2 ** 31 - 1) // 2
    else:
        assert lay["shape"][1] <= 2 ** 30 - 128, "a contiguous cache's capacity under a window"
    if not fp8:
        _packed_rule(lay["strides"][1])   # (the prefill reads a 16-bit cache's token stride by the packed tensors' rule)
    assert all(0 < n <= (lay["shape"][1] if lay["kind"] != "paged" else len(lay["table"][0]) * lay["page_size"]) for n in lay["cache_seqlens"])


@pytest.mark.parametrize("name", [n for n in KV_LAYOUTS if LAYOUTS[n]["kind"] != "long"], **IDS)
def test_the_rows_the_append_stores_lie_in_all_three_regions(name):
    """The append writes a few rows only: they, not just the rows the table names, lie on every side of the marks, and a 32-bit
    slip -- unsigned or signed -- moves one of them.  Without this a seed or layout change could empty the stray-store test."""
    lay = LAYOUTS[name]
    plan, t = lo.append_plan(lay), lay["tensors"]["k_cache"]
    assert len(plan["before"]) == lay["batch"] and len(plan["rows"]) == lay["batch"] * plan["new"] == len(np.unique(plan["rows"]))
    assert np.isin(plan["rows"], t.rows).all() or lay["kind"] == "batch", "rows of pages the table names"
    off = plan["rows"] * t.row_bytes
    assert set(lo.region(off).tolist()) == {0, 1, 2}, name
    assert (lo.as_uint32(off) != off).any() and ((lo.as_int32(off) != off) & (lo.as_uint32(off) == off)).any(), name
    order = np.argsort(plan["rows"], kind="stable")
    assert (np.diff(plan["compact_rows"][order]) > 0).all() and (plan["compact_rows"] + 1).max() * t.row_bytes <= t.compact_nbytes
    capacity = lay["shape"][1] if lay["kind"] == "batch" else len(lay["table"][0]) * lay["page_size"]
    compact_capacity = lay["compact_shape"][1] if lay["kind"] == "batch" else capacity
    assert all(0 <= n and n + plan["new"] <= min(capacity, compact_capacity) for n in plan["before"]), "no token is dropped"
    if lay["kind"] == "paged":
        assert all(n % lay["page_size"] == lay["page_size"] - plan["new"] // 2 for n in plan["before"]), "every entry crosses a page boundary"


def _bwd_struct(lay, compact, one_range=False, causal=False):
    hq, hk = lay["heads"]
    tq, tk = (lay["compact_total_q"], lay["compact_total_k"]) if compact else (lay["total_q"], lay["total_k"])
    ks = (hk * 128, 128, 1) if compact else lay["k_strides"]
    fields = dict(q=FAKE, k=FAKE, v=FAKE, o=FAKE, dout=FAKE, lse=ctypes.cast(ctypes.c_void_p(FAKE), ctypes.POINTER(ctypes.c_float)),
                  dq=FAKE, dk=FAKE, dv=FAKE, workspace=FAKE, n_heads=hq, n_kv_heads=hk, d_head=128,
                  q_seq_stride=hq * 128, q_head_stride=128, out_seq_stride=hq * 128, out_head_stride=128,
                  kv_seq_stride=ks[0], kv_head_stride=ks[1], dkv_seq_stride=ks[0], dkv_head_stride=ks[1], dtype=15, causal=int(causal),
                  varlen=_capi.make_varlen_layout(FAKE, len(lay["seqs"]), tq, lay["max_q"]))
    if one_range:
        return _capi.FaBwdVarlenArgs(**fields)
    return _capi.FaBwdVarlenQKArgs(struct_size=ctypes.sizeof(_capi.FaBwdVarlenQKArgs),
                                   varlen_k=_capi.make_varlen_layout(FAKE, len(lay["seqs"]), tk, lay["max_k"]), **fields)


def bwd_split(lay, compact, one_range=False, causal=False):
    """The dK / dV split of a packed backward on `lay`, read back from the workspace query as tests/test_softcap_gpu.py does"""
    a = _bwd_struct(lay, compact, one_range, causal)
    lib = _capi.load()
    nbytes = (lib.fa_bwd_varlen_workspace_bytes if one_range else lib.fa_bwd_varlen_qk_workspace_bytes)(ctypes.byref(a))
    assert nbytes > 0, _capi.last_error()
    hq, hk = lay["heads"]
    tq, tk = (lay["compact_total_q"], lay["compact_total_k"]) if compact else (lay["total_q"], lay["total_k"])
    delta = (4 * hq * tq + 15) & ~15
    per_split = 4 * hk * tk * 2 * 128
    assert (nbytes - delta) % per_split == 0
    return (nbytes - delta) // per_split or 1, nbytes


PACKED = [n for n, lay in LAYOUTS.items() if lay["kind"] == "packed"]


@pytest.mark.parametrize("name", PACKED, **IDS)
def test_the_packed_backward_queries_accept_every_layout_and_the_split_agrees(name):
    lay = LAYOUTS[name]
    one = lay["side"] == "one"
    for causal in (False, True):
        large, nbytes = bwd_split(lay, False, one, causal)
        compact, _ = bwd_split(lay, True, one, causal)
        assert large == compact, (name, causal, large, compact)
        assert nbytes <= lay["bytes"]["workspace"] + lay["bytes"].get("delta", 0), (name, nbytes)
    lib = _capi.load()
    for dtype in (15, 5):   # the packed forward has no query that reads sizes: the configuration that serves it is served
        cfg = _capi.FaFwdConfig(dtype=dtype, d_head=128, B_r=128, B_c=64, n_warps=4, async_copy=1, eager_load_blocks=1, swizzled=1,
                                Q_mma_load_K_tiles=0, K_mma_load_K_tiles=0, V_mma_load_K_tiles=0, mma_double_buffer_loads=1, optimized_softmax=0)
        opts = _capi.make_opts()
        for query in (lib.fa_fwd_varlen_supported, lib.fa_fwd_varlen_qk_supported, lib.fa_fwd_varlen_qk_window_supported,
                      lib.fa_fwd_varlen_qk_softcap_supported, lib.fa_fwd_varlen_kvcache_supported, lib.fa_fwd_varlen_kvcache_fp8_supported,
                      lib.fa_fwd_varlen_kvcache_window_supported, lib.fa_fwd_varlen_kvcache_fp8_window_supported):
            assert query(ctypes.byref(cfg), ctypes.byref(opts)) == 1, dtype
    _packed_rule(lay["q_strides"][0])
    _packed_rule(lay["k_strides"][0])
    _stride_rules(lay["q_strides"], 8)
    _stride_rules(lay["k_strides"], 8)
    assert lay["max_q"] <= 2 ** 30 - 128 and lay["max_k"] <= 2 ** 30 - 128 and lay["total_q"] <= (2 ** 31 - 1) // 2 and lay["total_k"] <= (2 ** 31 - 1) // 2
    if lay["heads"] == (8, 2):
        assert bwd_split(lay, False)[0] > 1, "the GQA case runs the split partials and the reduce kernel"


def test_the_prime_group_layout_carries_the_partials_past_4_gib():
    """The split is the smallest divisor of the group that brings n_seqs * n_kv_heads * ceil(max_seqlen_k / 128) * split to 1024
    workgroups under a causal mask (256 without one), and the whole group where no divisor does.  Heads (37, 1) with 1012
    workgroups therefore run with split 37, in the large and in the compact form, and the fp32 partials -- n_kv_heads * split *
    total_k * 256 floats -- are 4.3 GiB at total_k = 122 000: the query returns delta and exactly the bytes the layout's workspace
    tensor describes.  With one K / V head per query head, (4, 4), the split is 1 and the workspace is delta alone."""
    lay = LAYOUTS["packed-workspace-37x1"]
    assert len(lay["seqs"]) * -(-lay["max_k"] // 128) < 1024
    ws = lay["tensors"]["workspace"]
    for compact, part in ((False, ws.nbytes), (True, ws.compact_nbytes)):
        split, nbytes = bwd_split(lay, compact, causal=True)
        tq = lay["compact_total_q"] if compact else lay["total_q"]
        assert split == lay["split"] == 37 and nbytes == ((4 * 37 * tq + 15) & ~15) + part, (compact, split, nbytes)
    assert ws.nbytes > lo.MARK32 and ws.row_bytes == 4 * 2 * 128
    # the rows of the workspace tensor are part (hk * split + sp) of every real key row
    k = lay["tensors"]["k"]
    assert (ws.rows.reshape(37, -1) == np.arange(37)[:, None] * lay["total_k"] + k.rows[None, :]).all()
    lay = LAYOUTS["packed-k-4x4"]
    split, nbytes = bwd_split(lay, False)
    assert split == 1 and nbytes == (4 * 4 * lay["total_q"] + 15) & ~15


@pytest.mark.parametrize("name", [n for n, lay in LAYOUTS.items() if lay["kind"] == "dense"], **IDS)
def test_the_dense_backward_queries_accept_the_packed_buffer_and_the_split_agrees(name):
    lay, lib = LAYOUTS[name], _capi.load()
    hq, hk = lay["heads"]
    got = []
    for batch in (lay["batch"], len(lay["marks"])):
        qs, os_, ks, ds = lay["qkv_strides"], lay["out_strides"], lay["kv_strides"], lay["dkv_strides"]
        base = _capi.FaBwdArgs(q=FAKE, k=FAKE, v=FAKE, o=FAKE, dout=FAKE, lse=ctypes.cast(ctypes.c_void_p(FAKE), ctypes.POINTER(ctypes.c_float)),
                               dq=FAKE, dk=FAKE, dv=FAKE, workspace=FAKE, batch=batch, seq_len=lay["seq_len"], n_heads=hq, d_head=128,
                               qkv_batch_stride=qs[0], qkv_seq_stride=qs[1], qkv_head_stride=qs[2],
                               out_batch_stride=os_[0], out_seq_stride=os_[1], out_head_stride=os_[2], dtype=15, causal=0)
        delta = 4 * batch * hq * lay["seq_len"]
        if hq == hk:
            nbytes = lib.fa_bwd_workspace_bytes(ctypes.byref(base))
        else:
            args = _capi.FaBwdGqaArgs(base=base, n_kv_heads=hk, kv_batch_stride=ks[0], kv_seq_stride=ks[1], kv_head_stride=ks[2],
                                      dkv_batch_stride=ds[0], dkv_seq_stride=ds[1], dkv_head_stride=ds[2])
            nbytes = lib.fa_bwd_gqa_workspace_bytes(ctypes.byref(args))
        assert nbytes >= delta, (name, batch, _capi.last_error())
        got.append((nbytes - delta) // (4 * batch * hk * lay["seq_len"] * 2 * 128))
    assert got[0] == got[1] == 0, (name, got, "no dK / dV split in either launch: the summation order agrees")
    assert lay["qkv_strides"][1] <= 0xFFFFFFFF // 512
