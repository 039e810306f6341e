"""The KV-cache, varlen and backward paths at byte offsets beyond 2 GiB and 4 GiB on the MI355X.

Every case places a small problem inside a large allocation by a layout of tests/large_offset_layouts.py -- the rows the launch
names lie on both sides of the 2^31 and 2^32 byte marks of each large tensor, everything else holds poison -- and asks that the
result equal, BIT FOR BIT, the same call on a compact copy of the same rows, renumbered.  The compact call is the small-offset
result the rest of the suite compares with fp32 eager, so no tolerance appears here; tests/test_large_offsets_cpu.py proves on
the CPU that a 32-bit slip in any of these offsets moves a named row.  A case builds the compact form first, allocates the large
one with torch.empty, poisons it in place, copies the named rows in, runs both, compares integer views and frees the large
tensors.  It skips only when the device has less free memory than the layout's declared bytes plus 2 GiB, and prints both
figures then; it prints the largest byte offset its layout names and its wall time."""
import ctypes
import functools
import time
import traceback

import pytest
import torch

import flash_attention
from flash_attention_from_scratch_amd import _capi
from tests import large_offset_layouts as lo

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
IDS = dict(ids=str)
INT_VIEW = {1: torch.uint8, 2: torch.int16, 4: torch.int32}
SENTINEL64 = {1: 0x7F7F7F7F7F7F7F7F, 2: 0x7FC07FC07FC07FC0}   # eight NAN8 bytes / four NAN16 words
LAYOUTS = lo.all_layouts()
N_HEADS = 8   # the decode and prefill queries' heads (the caches have 2: groups of 4)


@pytest.fixture(autouse=True)
def _release():
    yield
    torch.cuda.empty_cache()


def _frees(test):
    """A failing (or skipping) case drops its frames' locals at once: up to 21 GiB of tensors that the traceback would keep alive,
    so that the cases behind it would skip for lack of memory instead of running."""
    @functools.wraps(test)
    def run(*args, **kwargs):
        try:
            return test(*args, **kwargs)
        except BaseException as exc:
            traceback.clear_frames(exc.__traceback__)
            raise
    return run


class _Case:
    """The budget check in front of a case, and its report behind it."""

    def __init__(self, tag, lay, which="bytes"):
        self.tag, self.t0 = tag, time.perf_counter()
        self.need = lo.total_bytes(lay, which)
        assert self.need <= lo.BUDGET, (tag, self.need)
        torch.cuda.empty_cache()
        free, _ = torch.cuda.mem_get_info(0)
        if free < self.need + lo.HEADROOM:
            print(f"large offsets {tag}: skipped, {free} bytes free, {self.need} + {lo.HEADROOM} needed")
            pytest.skip(f"{free} bytes free, {self.need} + {lo.HEADROOM} needed")
        self.largest = max(int(t.offsets().max()) for t in lay["tensors"].values())

    def done(self):
        torch.cuda.synchronize()
        print(f"large offsets {self.tag}: the layout's largest named byte offset {self.largest} ({self.largest / lo.GIB:.2f} GiB), "
              f"{self.need / lo.GIB:.1f} GiB declared, {time.perf_counter() - self.t0:.2f} s")


def _bits(t):
    return t.view(INT_VIEW[t.element_size()])


def _same(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _nonzero_bits(t):
    """The elements of t that are not +0 (-0.0 and NaN count).  The real rows agree bit for bit, so two equal counts mean that
    every filler element is exactly +0."""
    return int(torch.count_nonzero(_bits(t)))


def _poisoned(numel, dtype):
    """numel elements of dtype, every one the NaN pattern of its width (written in place: no temporary)"""
    size = torch.empty((), dtype=dtype).element_size()
    return torch.empty(numel, dtype=INT_VIEW[size], device=DEV).fill_(lo.NAN16 if size == 2 else lo.NAN8).view(dtype)


def _randn(shape, dtype, gen):
    return torch.randn(shape, generator=gen, device=DEV, dtype=torch.float32).to(dtype)


def _finite_where_it_must_be(o, lse):
    """the compact call: o finite; lse finite, or -inf on a row that sees no key"""
    assert bool(torch.isfinite(o.float()).all()) and not bool(torch.isnan(lse).any()) and not bool((lse == float("inf")).any())


def _i32(values):
    return torch.tensor(values, dtype=torch.int32, device=DEV)


# ---- K / V caches: the two forms of a layout ------------------------------------------------------------------------------------

class _Caches:
    """k / v caches of a cache layout: .compact and .large (k, v, block_table or None), and the lengths"""

    def __init__(self, lay, dtype, seed, poison_compact=False):
        self.lay, self.fp8 = lay, lay["elem_bytes"] == 1
        self.cache_dtype = torch.float8_e4m3fn if self.fp8 else dtype
        gen = torch.Generator(device=DEV).manual_seed(seed)
        cshape, numel = lay["compact_shape"], lay["tensors"]["k_cache"].nbytes // lay["elem_bytes"]
        kv_c, kv_l, self.bases = [], [], []
        for _ in range(2):
            if poison_compact:
                c = _poisoned(cshape[0] * cshape[1] * cshape[2] * cshape[3], self.cache_dtype).view(cshape)
            else:
                c = _randn(cshape, self.cache_dtype, gen)
            base = _poisoned(numel, self.cache_dtype)
            large = base.as_strided(lay["shape"], lay["strides"])
            if not poison_compact:
                if lay["kind"] == "paged":
                    _bits(large).index_copy_(0, torch.tensor(lay["used"], device=DEV), _bits(c))
                elif lay["kind"] == "batch":
                    _bits(large)[:, :cshape[1]].copy_(_bits(c))
                else:
                    _bits(large).copy_(_bits(c))
            kv_c.append(c)
            kv_l.append(large)
            self.bases.append(base)
        paged = lay["kind"] == "paged"
        self.compact = (kv_c[0], kv_c[1], _i32(lay["compact_table"]) if paged else None)
        self.large = (kv_l[0], kv_l[1], _i32(lay["table"]) if paged else None)
        self.lens = _i32(lay["cache_seqlens"])
        self.descales = {}
        if self.fp8:
            self.descales = dict(k_descale=torch.rand((lay["batch"], lay["n_kv"]), generator=gen, device=DEV) + 0.5,
                                 v_descale=torch.rand((lay["batch"], lay["n_kv"]), generator=gen, device=DEV) + 0.5)

    def free(self):
        self.compact = self.large = self.bases = None


DECODE_LAYOUTS = {"paged64": "paged64x", "paged256": "paged256x", "batch": "batch", "long": "long"}
VARIANTS = {"bf16": (torch.bfloat16, 2, False), "fp16": (torch.float16, 2, False), "fp8": (torch.bfloat16, 1, False),
            "window": (torch.float16, 2, True), "fp8-window": (torch.float16, 1, True)}


@pytest.mark.parametrize("variant", list(VARIANTS), **IDS)
@pytest.mark.parametrize("layout", list(DECODE_LAYOUTS), **IDS)
@_frees
def test_decode_reads_caches_beyond_4_gib(layout, variant):
    """forward_kvcache on a paged pool (page sizes 64 and 256), a contiguous cache whose batch stride carries it past 4 GiB and one
    entry whose own 1.1 M keys pass 4 GiB (a 4 KiB row stride): o and lse of seqlen_q 1 with the rule's split count and of
    seqlen_q 4 with 3 splits.  The window of the long entry, (60000, 0), spans the 4 GiB mark."""
    dtype, elem, windowed = VARIANTS[variant]
    lay = LAYOUTS[DECODE_LAYOUTS[layout] + str(elem)]
    case = _Case(f"decode {layout} {variant}", lay)
    c = _Caches(lay, dtype, seed=1)
    gen = torch.Generator(device=DEV).manual_seed(2)
    window = ((60000, 0) if layout == "long" else (100, 0)) if windowed else (-1, -1)
    for seqlen_q, num_splits in ((1, 0), (4, 3)):
        q = _randn((lay["batch"], seqlen_q, N_HEADS, 128), dtype, gen)
        kw = dict(return_lse=True, max_seqlen_k=max(lay["cache_seqlens"]), num_splits=num_splits, window_size=window, **c.descales)
        o_c, lse_c = flash_attention.forward_kvcache(q, c.compact[0], c.compact[1], c.lens, block_table=c.compact[2], **kw)
        o_l, lse_l = flash_attention.forward_kvcache(q, c.large[0], c.large[1], c.lens, block_table=c.large[2], **kw)
        _finite_where_it_must_be(o_c, lse_c)
        assert _same(o_l, o_c), (layout, variant, seqlen_q, num_splits, "o")
        assert _same(lse_l, lse_c), (layout, variant, seqlen_q, num_splits, "lse")
    c.free()
    case.done()


APPEND = [("paged64", 2), ("paged256", 2), ("paged256", 1), ("batch", 2), ("batch", 1)]


@pytest.mark.parametrize("layout,elem", APPEND, **IDS)
@_frees
def test_append_writes_its_rows_beyond_4_gib_and_nothing_else(layout, elem):
    """append_kvcache with rotary (and q) into pools that hold the sentinel everywhere: the written rows, the rotated q and the
    new lengths equal the compact call's, and every other 8-byte word of both large pools still holds the sentinel -- which is
    what catches a store whose 32-bit offset wrapped."""
    lay = LAYOUTS[DECODE_LAYOUTS[layout] + str(elem)]
    dtype = torch.bfloat16 if elem == 2 else torch.float16
    case = _Case(f"append {layout} x{elem}", lay)
    c = _Caches(lay, dtype, seed=3, poison_compact=True)
    gen = torch.Generator(device=DEV).manual_seed(4)
    plan = lo.append_plan(lay)   # (tests/test_large_offsets_cpu.py: the rows it stores lie in all three regions of the pool)
    batch, n_kv, new, before, ps = lay["batch"], lay["n_kv"], plan["new"], plan["before"], lay.get("page_size")
    k, v = _randn((batch, new, n_kv, 128), dtype, gen), _randn((batch, new, n_kv, 128), dtype, gen)
    q = _randn((batch, new, N_HEADS, 128), dtype, gen)
    angle = torch.rand((2048, 32), generator=gen, device=DEV) * 6.28
    cos, sin = torch.cos(angle).to(dtype), torch.sin(angle).to(dtype)
    got = []
    for kc, vc, table in (c.compact, c.large):
        lens_out, q_rot = flash_attention.append_kvcache(kc, vc, k, v, _i32(before), block_table=table, q=q, rotary_cos=cos, rotary_sin=sin,
                                                         causal=True, **c.descales)
        first, second = [], []   # the written rows' indices into the cache's first two axes
        for b in range(batch):
            for t in range(new):
                pos = before[b] + t
                if lay["kind"] == "paged":
                    first.append(int(table[b, pos // ps]))
                    second.append(pos % ps)
                else:
                    first.append(b)
                    second.append(pos)
        named = plan["compact_rows"] if kc is c.compact[0] else plan["rows"]
        assert [f * kc.shape[1] + r for f, r in zip(first, second)] == named.tolist(), "the rows of the plan"
        first, second = torch.tensor(first, device=DEV), torch.tensor(second, device=DEV)
        got.append((lens_out, q_rot, _bits(kc)[first, second].contiguous(), _bits(vc)[first, second].contiguous()))
    (lens_c, q_c, k_rows_c, v_rows_c), (lens_l, q_l, k_rows_l, v_rows_l) = got
    assert lens_c.tolist() == [n + new for n in before] and torch.equal(lens_l, lens_c)
    assert bool(torch.isfinite(q_c.float()).all()) and _same(q_l, q_c)
    sentinel = SENTINEL64[elem]
    for name, rows_c, rows_l, base in (("k", k_rows_c, k_rows_l, c.bases[0]), ("v", v_rows_c, v_rows_l, c.bases[1])):
        assert not bool((rows_c.view(torch.int64) == sentinel).all(dim=-1).any()), (name, "a row the compact call did not write")
        assert torch.equal(rows_l, rows_c), (layout, elem, name, "the written rows")
        words = base.view(torch.int64)
        untouched = int((words == sentinel).sum())
        written = rows_c.view(torch.int64)
        assert untouched == words.numel() - written.numel() + int((written == sentinel).sum()), (layout, elem, name, "a stray store")
    c.free()
    case.done()


PREFILL = {"16-bit": (torch.bfloat16, 2, False), "fp8": (torch.float16, 1, False), "window": (torch.float16, 2, True),
           "fp8-window": (torch.bfloat16, 1, True)}


@pytest.mark.parametrize("variant", list(PREFILL), **IDS)
@pytest.mark.parametrize("layout", ["paged256", "batch"], **IDS)
@_frees
def test_prefill_reads_caches_beyond_4_gib(layout, variant):
    """forward_varlen_kvcache against the paged pool (page size 256) and the contiguous cache past 4 GiB: o and lse of a packed
    chunk per sequence, causal (bottom-right), plain or under the window (63, 0)."""
    dtype, elem, windowed = PREFILL[variant]
    lay = LAYOUTS[DECODE_LAYOUTS[layout] + str(elem)]
    case = _Case(f"prefill {layout} {variant}", lay)
    c = _Caches(lay, dtype, seed=5)
    gen = torch.Generator(device=DEV).manual_seed(6)
    len_q = [min(n, (129, 64, 1, 40, 257)[b % 5]) for b, n in enumerate(lay["cache_seqlens"])]
    cu_q = [0]
    for n in len_q:
        cu_q.append(cu_q[-1] + n)
    q = _randn((cu_q[-1], N_HEADS, 128), dtype, gen)
    kw = dict(causal=True, max_seqlen_k=max(lay["cache_seqlens"]), window_size=(63, 0) if windowed else (-1, -1), **c.descales)
    o_c, lse_c = flash_attention.forward_varlen_kvcache(q, c.compact[0], c.compact[1], _i32(cu_q), max(len_q), c.lens, block_table=c.compact[2], **kw)
    o_l, lse_l = flash_attention.forward_varlen_kvcache(q, c.large[0], c.large[1], _i32(cu_q), max(len_q), c.lens, block_table=c.large[2], **kw)
    _finite_where_it_must_be(o_c, lse_c)
    assert _same(o_l, o_c), (layout, variant, "o")
    assert _same(lse_l, lse_c), (layout, variant, "lse")
    c.free()
    case.done()


# ---- packed sequences -------------------------------------------------------------------------------------------------------------

FORMS = {"qk": {}, "causal": dict(causal=True), "window": dict(window_size=(63, 3)), "softcap": dict(softcap=4.0), "softcap-window": dict(softcap=4.0, window_size=(63, 3))}


class _Packed:
    """The two forms of a packed layout: .compact and .large hold (q, k, v, dout, cu_q, cu_k); on the large side the fillers' rows
    and the strided views' padding hold NaN."""

    def __init__(self, lay, dtype, seed, backward):
        self.lay, self.dtype = lay, dtype
        hq, hk = lay["heads"]
        gen = torch.Generator(device=DEV).manual_seed(seed)
        q, dout = (_randn((lay["compact_total_q"], hq, 128), dtype, gen) for _ in range(2))
        k, v = (_randn((lay["compact_total_k"], hk, 128), dtype, gen) for _ in range(2))
        self.compact = (q, k, v, dout if backward else None, _i32(lay["compact_cu_q"]), _i32(lay["compact_cu_k"]))
        side = lay["side"]
        ql = self.place(q, "q") if side in ("q", "one") else q
        dl = (self.place(dout, "q") if side in ("q", "one") else dout) if backward else None
        kl, vl = ((self.place(k, "k"), self.place(v, "k")) if side in ("k", "one") else (k, v))
        self.large = (ql, kl, vl, dl, _i32(lay["cu_q"]), _i32(lay["cu_k"]))

    def empty(self, which, large):
        """A NaN-filled tensor of the q side's ("q") or the key side's ("k") shape, in the large or the compact form -> (view, base)"""
        lay = self.lay
        hq, hk = lay["heads"]
        if which == "q":
            total = lay["total_q"] if large else lay["compact_total_q"]
            base = _poisoned(total * hq * 128, self.dtype)
            return base.view(total, hq, 128), base
        total = lay["total_k"] if large else lay["compact_total_k"]
        row = lay["k_strides"][0] if large else hk * 128
        base = _poisoned(total * row, self.dtype)
        return base.as_strided((total, hk, 128), (row, 128, 1)), base

    def slices(self, which):
        """(large rows, compact rows) of every real sequence on one side"""
        lay = self.lay
        cu, ccu = (lay["cu_q"], lay["compact_cu_q"]) if which == "q" else (lay["cu_k"], lay["compact_cu_k"])
        return [(slice(cu[j], cu[j + 1]), slice(ccu[j], ccu[j + 1])) for j in lay["real"]]

    def place(self, compact, which):
        large, _ = self.empty(which, True)
        for sl, sc in self.slices(which):
            large[sl] = compact[sc]
        return large

    def forward(self, form, large):
        lay = self.lay
        q, k, v, _, cu_q, cu_k = self.large if large else self.compact
        kw = dict(FORMS[form])
        if lay["side"] != "one":
            kw.update(cu_seqlens_k=cu_k, max_seqlen_k=lay["max_k"])
        return flash_attention.forward_varlen(q, k, v, cu_q, lay["max_q"], **kw)

    def backward(self, form, large, o, lse):
        """The C ABI call into NaN-filled outputs (dk and dv strided as k is) and a NaN-filled workspace -> (dq, dk, dv, the bases of
        dk and dv, the split); .workspace_bytes is what the query asked for"""
        lay, lib = self.lay, _capi.load()
        q, k, v, dout, cu_q, cu_k = self.large if large else self.compact
        big = lambda which: large and lay["side"] in (which, "one")   # noqa: E731
        dq, _ = self.empty("q", big("q"))
        (dk, dk_base), (dv, dv_base) = self.empty("k", big("k")), self.empty("k", big("k"))
        assert dk.stride() == k.stride() or not lay["strided_kv"]
        fields = dict(
            q=q.data_ptr(), k=k.data_ptr(), v=v.data_ptr(), o=o.data_ptr(), dout=dout.data_ptr(),
            lse=ctypes.cast(ctypes.c_void_p(lse.data_ptr()), ctypes.POINTER(ctypes.c_float)),
            dq=dq.data_ptr(), dk=dk.data_ptr(), dv=dv.data_ptr(), workspace=16, n_heads=q.shape[1], n_kv_heads=k.shape[1], d_head=128,
            q_seq_stride=q.stride(0), q_head_stride=q.stride(1), out_seq_stride=o.stride(0), out_head_stride=o.stride(1),
            kv_seq_stride=k.stride(0), kv_head_stride=k.stride(1), dkv_seq_stride=dk.stride(0), dkv_head_stride=dk.stride(1),
            dtype=15 if self.dtype == torch.bfloat16 else 5, causal=int(FORMS[form].get("causal", False)),
            varlen=_capi.make_varlen_layout(cu_q.data_ptr(), len(lay["seqs"]), q.shape[0], lay["max_q"]))
        assert o.is_contiguous() and dout.is_contiguous() and dq.stride() == o.stride() == dout.stride()
        one = lay["side"] == "one"
        if one:
            a, sized = _capi.FaBwdVarlenArgs(**fields), lib.fa_bwd_varlen_workspace_bytes
        else:
            a = _capi.FaBwdVarlenQKArgs(struct_size=ctypes.sizeof(_capi.FaBwdVarlenQKArgs),
                                        varlen_k=_capi.make_varlen_layout(cu_k.data_ptr(), len(lay["seqs"]), k.shape[0], lay["max_k"]), **fields)
            sized = lib.fa_bwd_varlen_qk_workspace_bytes
        nbytes = sized(ctypes.byref(a))
        assert nbytes > 0, _capi.last_error()
        delta = (4 * q.shape[1] * q.shape[0] + 15) & ~15
        per_split = 4 * k.shape[1] * k.shape[0] * 2 * 128
        assert (nbytes - delta) % per_split == 0
        split = (nbytes - delta) // per_split or 1
        ws = torch.empty(nbytes, dtype=torch.uint8, device=DEV).fill_(0xFF)   # (fp32 NaN: a partial or a delta the kernels do not write shows)
        a.workspace = ws.data_ptr()
        stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        opts = FORMS[form]
        w = _capi.make_window(*opts.get("window_size", (-1, -1)))
        if one:
            rc = lib.fa_bwd_launch_varlen(ctypes.byref(a), stream, None)
        elif "softcap" in opts:
            cap = _capi.make_softcap(opts["softcap"])
            rc = lib.fa_bwd_launch_varlen_qk_softcap(ctypes.byref(a), ctypes.byref(w), ctypes.byref(cap), stream, None)
        elif "window_size" in opts:
            rc = lib.fa_bwd_launch_varlen_qk_window(ctypes.byref(a), ctypes.byref(w), stream, None)
        else:
            rc = lib.fa_bwd_launch_varlen_qk(ctypes.byref(a), stream, None)
        _capi.check(rc)
        torch.cuda.synchronize()
        self.workspace_bytes = nbytes
        return dq, dk, dv, (dk_base, dv_base), split

    def same_real_rows(self, large, compact, which, tag, lse=False):
        for sl, sc in self.slices(which):
            got, want = (large[:, sl], compact[:, sc]) if lse else (large[sl], compact[sc])
            assert _same(got.contiguous(), want.contiguous()), (self.lay["name"], tag, sl)


def _check_forward(p, form, o_l, lse_l, o_c, lse_c):
    lay = p.lay
    _finite_where_it_must_be(o_c, lse_c)
    p.same_real_rows(o_l, o_c, "q", form + " o")
    p.same_real_rows(lse_l, lse_c, "q", form + " lse", lse=True)
    if lay["side"] == "q":   # the fillers' rows see no key: exactly 0 and -inf, written
        assert _nonzero_bits(o_l) == _nonzero_bits(o_c), (lay["name"], form, "o of a filler row")
        fillers = lay["total_q"] - lay["compact_total_q"]
        assert int((lse_l == float("-inf")).sum()) == fillers * lay["heads"][0] + int((lse_c == float("-inf")).sum()), (lay["name"], form, "lse")
    if lay["side"] == "k":   # (the query side is the compact one: the whole outputs agree)
        assert _same(o_l, o_c) and _same(lse_l, lse_c), (lay["name"], form)


@pytest.mark.parametrize("form", list(FORMS), **IDS)
@pytest.mark.parametrize("side", ["q", "k"], **IDS)
@_frees
def test_packed_forward_two_ranges_beyond_4_gib(side, form):
    """forward_varlen(cu_seqlens_k=) plain, under window_size=(63, 3), under softcap=4.0 and under both: with the query side
    large (q and o past 4 GiB; fillers of rows that see no key, o = 0 and lse = -inf exactly) and with the key side large (k and v
    as views with a 4 KiB token stride past 4 GiB; fillers of keys no row sees)."""
    lay = LAYOUTS[f"packed-{side}-16x2"]
    case = _Case(f"packed forward {side} {form}", lay, "forward_bytes")
    p = _Packed(lay, torch.float16 if form == "window" else torch.bfloat16, seed=7, backward=False)
    o_c, lse_c = p.forward(form, False)
    o_l, lse_l = p.forward(form, True)
    _check_forward(p, form, o_l, lse_l, o_c, lse_c)
    del p, o_l, lse_l
    case.done()


@_frees
def test_packed_forward_one_range_beyond_4_gib():
    """forward_varlen with one range for both sides: q and o past 4 GiB, the real sequences at the marks.  With one range a
    filler is a sequence of its own (rows and keys): its inputs are NaN and its results are not compared."""
    lay = LAYOUTS["packed-one-16x2"]
    case = _Case("packed forward one range", lay, "forward_bytes")
    p = _Packed(lay, torch.bfloat16, seed=8, backward=False)
    o_c, lse_c = p.forward("qk", False)
    o_l, lse_l = p.forward("qk", True)
    _check_forward(p, "one range", o_l, lse_l, o_c, lse_c)
    del p, o_l, lse_l
    case.done()


def _run_backward(lay, form, dtype, seed, tag):
    case = _Case(f"packed backward {tag}", lay)
    p = _Packed(lay, dtype, seed, backward=True)
    o_c, lse_c = p.forward(form, False)
    _finite_where_it_must_be(o_c, lse_c)
    dq_c, dk_c, dv_c, _, split_c = p.backward(form, False, o_c, lse_c)
    assert all(bool(torch.isfinite(g.float()).all()) for g in (dq_c, dk_c, dv_c)), (tag, "the compact launch wrote every gradient")
    o_l, lse_l = p.forward(form, True)
    dq_l, dk_l, dv_l, bases, split_l = p.backward(form, True, o_l, lse_l)
    assert split_l == split_c, (tag, split_l, split_c, "one summation order")
    p.same_real_rows(dq_l, dq_c, "q", tag + " dq")
    p.same_real_rows(dk_l, dk_c, "k", tag + " dk")
    p.same_real_rows(dv_l, dv_c, "k", tag + " dv")
    side = lay["side"]
    if side == "q":     # a filler's rows saw no key: dq = 0, written into the NaN
        assert _nonzero_bits(dq_l) == _nonzero_bits(dq_c), (tag, "dq of a filler row")
        assert _same(dk_l, dk_c) and _same(dv_l, dv_c), tag
    if side == "k":     # a filler's keys are seen by no row: dk = dv = 0, written; the views' padding still holds NaN
        assert _same(dq_l, dq_c), tag
        padding = lay["total_k"] * (lay["k_strides"][0] - lay["heads"][1] * 128)
        for name, g_l, g_c, base in (("dk", dk_l, dk_c, bases[0]), ("dv", dv_l, dv_c, bases[1])):
            assert _nonzero_bits(g_l) == _nonzero_bits(g_c), (tag, name, "of a filler key")
            assert int((_bits(base) == lo.NAN16).sum()) == padding, (tag, name, "a store outside the view")
    workspace_bytes = p.workspace_bytes
    del p, o_l, lse_l, dq_l, dk_l, dv_l, bases
    case.done()
    return split_l, workspace_bytes


@pytest.mark.parametrize("form", ["qk", "window", "softcap"], **IDS)
@pytest.mark.parametrize("side", ["q", "k"], **IDS)
@_frees
def test_packed_backward_two_ranges_beyond_4_gib(side, form):
    """fa_bwd_launch_varlen_qk, _window ((63, 3)) and _softcap (4.0) through the C ABI into NaN-filled outputs: with the query side
    large (q, o, dout and dq past 4 GiB; a filler row's dq = 0) and with the key side large (k, v, dk and dv as views with a 4 KiB
    token stride past 4 GiB; a filler key's dk = dv = 0, the views' padding untouched).  Both launches keep every sequence and both
    bounds, so the dK / dV split agrees (asserted) and the bits must."""
    _run_backward(LAYOUTS[f"packed-{side}-16x2"], form, torch.float16 if form == "window" else torch.bfloat16, 9, f"{side} {form}")


@_frees
def test_packed_backward_one_range_beyond_4_gib():
    """fa_bwd_launch_varlen (one range): q, o, dout and dq past 4 GiB; the fillers are sequences of their own, not compared."""
    _run_backward(LAYOUTS["packed-one-16x2"], "qk", torch.bfloat16, 10, "one range")


@_frees
def test_packed_backward_gqa_split_beyond_4_gib():
    """Heads (8, 2) with few enough key blocks that the dK / dV split is > 1 in both launches: the fp32 partials and the reduce
    kernel run beside a query side past 4 GiB."""
    assert _run_backward(LAYOUTS["packed-q-8x2"], "qk", torch.bfloat16, 11, "q 8x2 split")[0] > 1


@_frees
def test_packed_backward_one_kv_head_per_query_head_beyond_4_gib():
    """Heads (4, 4) on the large key side: with one K / V head per query head the split is 1 and the workspace is delta alone
    (the workspace past 4 GiB is test_packed_backward_workspace_beyond_4_gib's)."""
    assert _run_backward(LAYOUTS["packed-k-4x4"], "qk", torch.float16, 12, "k 4x4")[0] == 1


@_frees
def test_packed_backward_workspace_beyond_4_gib():
    """The fp32 dK / dV partials past 4 GiB: heads (37, 1), causal, 92 sequences of at most 11 key blocks -- 1012 workgroups, under
    the 1024 the split rule wants, and 37 has no divisor to reach them with, so the split is 37 in the large and in the compact
    launch (asserted) and the partials are 37 * 122 000 * 1 KiB = 4.3 GiB.  The real sequences hold the first and the last key
    row and the rows whose part 17 / part 34 partials straddle 2 GiB / 4 GiB; between them lie keys no row sees.  dk and dv of
    the real keys equal the compact launch's bits, the others are exactly 0, out of a workspace that held NaN."""
    lay = LAYOUTS["packed-workspace-37x1"]
    split, nbytes = _run_backward(lay, "causal", torch.bfloat16, 14, "workspace 37x1")
    assert split == lay["split"] == 37 and nbytes > lo.MARK32 and nbytes - lay["tensors"]["workspace"].nbytes == (4 * 37 * lay["total_q"] + 15) & ~15


# ---- the dense and GQA backward ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["dense-32x32", "dense-32x16"], **IDS)
@_frees
def test_dense_backward_reads_a_packed_buffer_beyond_4_gib(name):
    """backward with q, k, v as slices of one packed (800, 256, 3, 32, 128) buffer of 4.7 GiB (GQA: the K / V heads in a second
    buffer); o, dout and the gradients contiguous (1.6 GiB each).  The samples at the marks -- one straddles each -- equal the same
    samples gathered into a small batch.  (A deviation from "the same sample run alone": a batch of one would change the GQA
    launch's dK / dV split, and so its summation order; gathered, neither launch splits -- tests/test_large_offsets_cpu.py asserts
    it -- and a sample's work does not depend on its neighbours in either form.)  Outputs
    past 4 GiB are out of scope here: with five contiguous tensors of that size the case would not fit the memory budget."""
    lay = LAYOUTS[name]
    case = _Case(f"dense backward {name}", lay)
    hq, hk = lay["heads"]
    batch, seq_len = lay["batch"], lay["seq_len"]
    gen = torch.Generator(device=DEV).manual_seed(13)
    buf = torch.empty(lay["qkv_shape"], dtype=torch.bfloat16, device=DEV)
    for b in range(0, batch, 100):   # (by slices: no fp32 temporary of the whole buffer)
        buf[b:b + 100].normal_(generator=gen)
    assert buf.numel() * 2 > lo.MARK32 and buf.stride() == (seq_len * 3 * hq * 128, 3 * hq * 128, hq * 128, 128, 1)
    q, k, v = buf[:, :, 0], buf[:, :, 1], buf[:, :, 2]
    kvbuf = None
    if hk != hq:
        kvbuf = torch.empty(lay["kv_shape"], dtype=torch.bfloat16, device=DEV).normal_(generator=gen)
        k, v = kvbuf[:, :, 0], kvbuf[:, :, 1]
    assert q.stride() == lay["qkv_strides"]
    o, dout = (torch.empty((batch, seq_len, hq, 128), dtype=torch.bfloat16, device=DEV).normal_(generator=gen) for _ in range(2))
    # (any finite o and lse serve: the backward is a function of its six inputs; lse near ln 256 keeps exp(s - lse) in range)
    lse = torch.empty((batch, hq, seq_len), dtype=torch.float32, device=DEV).uniform_(5.0, 7.0, generator=gen)
    idx = torch.tensor(lay["marks"], device=DEV)
    small = buf[idx]
    q_c, k_c, v_c = small[:, :, 0], small[:, :, 1], small[:, :, 2]
    if kvbuf is not None:
        small_kv = kvbuf[idx]
        k_c, v_c = small_kv[:, :, 0], small_kv[:, :, 1]
    want = flash_attention.backward(q_c, k_c, v_c, o[idx], lse[idx], dout[idx])
    assert all(bool(torch.isfinite(g.float()).all()) for g in want)
    got = flash_attention.backward(q, k, v, o, lse, dout)
    for gname, g_l, g_c in zip(("dq", "dk", "dv"), got, want):
        assert _same(g_l[idx], g_c), (name, gname)
    del buf, kvbuf, o, dout, got
    case.done()
