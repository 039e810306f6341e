"""The host-side corpus of the KV-cache entry points (tests/test_host_corpus_cpu.py; recorded in tests/golden/host_corpus.json).

For every fa_decode* function, fa_kvcache_append_launch and the two cache prefills: valid base argument sets, every field of
every argument set to each value of VALUES, and every pair of fields set to a "bad" value each (pairs pin the ORDER of the
library's checks: an input that breaks two rules reports the first).  A case's record is (return value, fa_last_error(), the
returned ms where a launch succeeded).  Nothing here is random and nothing needs a device: the library validates before any HIP
call, and a call that passes every rule ends in the "no HIP device" status.  Because such a call WOULD launch on a machine that
has a device, with the fake pointers used here, run() refuses to start unless the library sees no device: the test runs this
module in a child process that hides them.

    python -m tests.host_corpus --record <parent commit>    # rewrites the golden file (from a build of that commit)
    python -m tests.host_corpus --dump                      # the current library's records, as JSON on stdout
"""
import base64
import ctypes
import itertools
import json
import os
import struct
import sys
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from flash_attention_from_scratch_amd import _capi   # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "host_corpus.json")
NO_DEVICE = (-7, "no HIP device available")
HIDE_DEVICES = {"HIP_VISIBLE_DEVICES": "-1", "ROCR_VISIBLE_DEVICES": "-1", "CUDA_VISIBLE_DEVICES": "-1"}

VALUES = (None, 0, -1, 1, 7, 8, 24, 32, 64, 96, 2 ** 30, 2 ** 31 - 1, 2 ** 31)   # None: a null pointer (0 for a number)
BAD_POINTER = (None, 7)       # the two "bad" values of a pair, by the kind of field: missing / misaligned,
BAD_NUMBER = (-1, 2 ** 31)    # negative / too large (a 32-bit field wraps it to its lowest value)
MS_SENTINEL = -1.0            # what a launch's ms holds before the call


def _varlen_cfg():
    """The configuration that serves packed sequences (flash_attention_kernels.varlen_config, without torch): bf16."""
    return _capi.FaFwdConfig(dtype=15, d_head=128, B_r=128, B_c=64, n_warps=4, async_copy=1, eager_load_blocks=1, swizzled=1,
                             Q_mma_load_K_tiles=0, K_mma_load_K_tiles=0, V_mma_load_K_tiles=0, mma_double_buffer_loads=1,
                             optimized_softmax=0)


# ---- base argument sets: name -> a function that builds fresh structures {struct name: ctypes structure} ----------------------

def _decode(paged, fp8=False, descales=True, causal=False, batch=2, Sq=1, H=8, Hkv=2, cache=4096):
    f = dict(dtype=15, causal=int(causal), q=16, k=16, v=16, o=16, lse=16, cache_seqlens=16, workspace=16, batch=batch, seqlen_q=Sq,
             n_heads=H, n_kv_heads=Hkv, q_batch_stride=Sq * H * 128, q_seq_stride=H * 128, q_head_stride=128,
             o_batch_stride=Sq * H * 128, o_seq_stride=H * 128, o_head_stride=128, kv_seq_stride=Hkv * 128, kv_head_stride=128)
    if paged:
        f.update(block_table=16, num_pages=100, page_size=256, max_pages_per_seq=16, block_table_stride=16, kv_batch_stride=256 * Hkv * 128)
    else:
        f.update(seqlen_cache=cache, kv_batch_stride=cache * Hkv * 128)
    if not fp8:
        return _capi.make_decode_args(**f)
    if descales:
        f.update(k_descale=16, v_descale=16, descale_batch_stride=Hkv)
    return _capi.make_decode_fp8_args(**f)


def _append(paged, fp8=False, descales=False, rotary=False, with_q=False, batch=3, Sn=1, Sq=1, H=8, Hkv=2, cache=256):
    f = dict(dtype=15, kv_dtype=1 if fp8 else 0, k_new=16, v_new=32, k=48, v=64, cache_seqlens=16, seqlens_out=16, batch=batch,
             seqlen_new=Sn, n_kv_heads=Hkv, new_batch_stride=Sn * Hkv * 128, new_seq_stride=Hkv * 128, new_head_stride=128,
             kv_seq_stride=Hkv * 128, kv_head_stride=128)
    if paged:
        f.update(block_table=16, num_pages=10, page_size=64, max_pages_per_seq=4, block_table_stride=4, kv_batch_stride=64 * Hkv * 128)
    else:
        f.update(seqlen_cache=cache, kv_batch_stride=cache * Hkv * 128)
    if rotary:
        f.update(rotary_cos=16, rotary_sin=16, rotary_dim=64, seqlen_ro=cache, rotary_seq_stride=32)
    if with_q:
        n = batch * Sq * H * 128 * 2
        f.update(q=1 << 20, q_out=(1 << 20) + n, seqlen_q=Sq, n_heads=H, q_batch_stride=Sq * H * 128, q_seq_stride=H * 128,
                 q_head_stride=128, qo_batch_stride=Sq * H * 128, qo_seq_stride=H * 128, qo_head_stride=128)
    if descales:
        f.update(k_descale=16, v_descale=16, descale_batch_stride=Hkv)
    return _capi.make_kvcache_append_args(**f)


def _prefill(paged, causal, fp8=False, T=1000, H=8, Hkv=2, n_seqs=3):
    s = {"args": _capi.FaFwdArgs(q=16, k=16, v=16, o=16, batch=1, seq_len=T, n_heads=H, d_head=128, batch_stride=0, seq_stride=H * 128,
                                 head_stride=128, cfg=_varlen_cfg()),
         "vq": _capi.make_varlen_layout(16, n_seqs, T, 512),
         "opts": _capi.make_opts(causal=causal, ms=ctypes.c_float(MS_SENTINEL))}
    if paged:
        s["kv"] = _capi.make_kv_layout(Hkv, 256 * Hkv * 128, Hkv * 128, 128)
        s["kc"] = _capi.make_kvcache_layout(cache_seqlens=16, block_table=16, num_pages=100, page_size=256, max_pages_per_seq=16,
                                            block_table_stride=16)
    else:
        s["kv"] = _capi.make_kv_layout(Hkv, 4096 * Hkv * 128, Hkv * 128, 128)
        s["kc"] = _capi.make_kvcache_layout(cache_seqlens=16, seqlen_cache=4096, batch=n_seqs)
    if fp8:
        s["sc"] = _capi.make_kvcache_fp8_scales(k_descale=16, v_descale=16, descale_batch_stride=Hkv)
    return s


WINDOWS = ((-1, -1), (0, 0), (128, -1), (128, 0))


def _window_bases(fp8):
    """Every window, plain and causal, on the contiguous cache; two of them paged; for fp8 two more without descales."""
    out = []
    for (left, right), causal in itertools.product(WINDOWS, (False, True)):
        out.append((f"contig,w=({left},{right}),causal={int(causal)}", dict(paged=False, causal=causal), (left, right)))
    out.append(("paged,w=(128,-1),causal=0", dict(paged=True, causal=False), (128, -1)))
    out.append(("paged,w=(0,0),causal=1", dict(paged=True, causal=True), (0, 0)))
    if fp8:
        out.append(("contig,nodescale,w=(128,0),causal=0", dict(paged=False, causal=False, descales=False), (128, 0)))
        out.append(("paged,nodescale,w=(-1,-1),causal=1", dict(paged=True, causal=True, descales=False), (-1, -1)))
    return out


def bases():
    """-> {family: [(base name, builder -> {struct name: structure})]}"""
    fam = {}
    fam["decode"] = [(n, (lambda p=p: {"a": _decode(p)})) for n, p in (("contig", False), ("paged", True))]
    fam["decode_fp8"] = [(f"{n},{'descale' if d else 'nodescale'}", (lambda p=p, d=d: {"a": _decode(p, fp8=True, descales=d)}))
                         for (n, p), d in itertools.product((("contig", False), ("paged", True)), (True, False))]
    for name, fp8 in (("decode_window", False), ("decode_fp8_window", True)):
        fam[name] = [(n, (lambda kw=kw, w=w, fp8=fp8: {"a": _decode(fp8=fp8, **kw), "w": _capi.make_window(*w)}))
                     for n, kw, w in _window_bases(fp8)]
    fam["append"] = []
    for (n, p), (kind, fp8, d), (rn, rot, wq) in itertools.product(
            (("contig", False), ("paged", True)), (("16bit", False, False), ("fp8", True, False), ("fp8+descale", True, True)),
            (("plain", False, False), ("rotary", True, False), ("rotary+q", True, True))):
        fam["append"].append((f"{n},{kind},{rn}", (lambda p=p, fp8=fp8, d=d, rot=rot, wq=wq: {"a": _append(p, fp8, d, rot, wq)})))
    for name, fp8 in (("prefill", False), ("prefill_fp8", True)):
        fam[name] = [(f"{n},causal={int(c)}", (lambda p=p, c=c, fp8=fp8: _prefill(p, c, fp8)))
                     for (n, p), c in itertools.product((("contig", False), ("paged", True)), (False, True))]
    return fam


# ---- entry points: (exported name, family, how it is called with the family's structures) -----------------------------------

def _ref(s):
    return ctypes.byref(s) if s is not None else None


def entries(lib):
    """-> [(exported function, family, is a launch, call(structs, extra) -> return value)].  `extra`: 'lse' (prefill) and
    'ms' (decode and append launches: a float pointer or None)."""
    out = []
    for fam, prefix, windowed in (("decode", "fa_decode", False), ("decode_fp8", "fa_decode_fp8", False),
                                  ("decode_window", "fa_decode_window", True), ("decode_fp8_window", "fa_decode_fp8_window", True)):
        for suffix in ("supported", "num_splits", "workspace_bytes", "launch"):
            fn = getattr(lib, f"{prefix}_{suffix}")
            launch = suffix == "launch"

            def call(s, extra, fn=fn, windowed=windowed, launch=launch):
                argv = [_ref(s["a"])] + ([_ref(s["w"])] if windowed else [])
                return fn(*argv, None, extra["ms"]) if launch else fn(*argv)
            out.append((f"{prefix}_{suffix}", fam, launch, call))
    out.append(("fa_kvcache_append_launch", "append", True, lambda s, extra: lib.fa_kvcache_append_launch(_ref(s["a"]), None, extra["ms"])))
    out.append(("fa_fwd_launch_varlen_kvcache", "prefill", False,
                lambda s, extra: lib.fa_fwd_launch_varlen_kvcache(_ref(s["args"]), _ref(s["kv"]), _ref(s["vq"]), _ref(s["kc"]), _ref(s["opts"]),
                                                                  extra["lse"], None)))
    out.append(("fa_fwd_launch_varlen_kvcache_fp8", "prefill_fp8", False,
                lambda s, extra: lib.fa_fwd_launch_varlen_kvcache_fp8(_ref(s["args"]), _ref(s["kv"]), _ref(s["vq"]), _ref(s["kc"]), _ref(s["sc"]),
                                                                      _ref(s["opts"]), extra["lse"], None)))
    return out


# ---- fields and mutations -------------------------------------------------------------------------------------------------------

def fields(structs, launch):
    """Every place a case can change: (struct name, field path, kind).  kind: 'ptr' / 'num' (all of VALUES), 'null' (only
    None: a whole structure, or a pointer the library writes through, which no fake value may stand for)."""
    out = []
    for sname in sorted(structs):
        out.append((sname, "", "null"))
        for fname, ftype in structs[sname]._fields_:
            if ftype is _capi.FaFwdConfig:
                out += [(sname, f"{fname}.{c}", "num") for c, _ in ftype._fields_]
            elif fname == "ms":
                out.append((sname, fname, "null"))
            else:
                out.append((sname, fname, "ptr" if ftype is ctypes.c_void_p else "num"))
    if "args" in structs:
        out.append(("@", "lse", "ptr"))
    if launch:
        out.append(("@", "ms", "null"))
    return out


def apply(structs, extra, place, value):
    sname, path, _ = place
    if sname == "@":
        extra[path] = None if value is None else ctypes.c_void_p(value)
    elif path == "":
        structs[sname] = None
    elif structs[sname] is not None:
        obj, parts = structs[sname], path.split(".")
        for p in parts[:-1]:
            obj = getattr(obj, p)
        if parts[-1] == "ms":
            obj.ms = None
        else:
            is_ptr = dict(type(obj)._fields_)[parts[-1]] is ctypes.c_void_p
            setattr(obj, parts[-1], value if is_ptr else (0 if value is None else value))


def mutations(places, pair_stride=1):
    """-> the cases of one (entry, base): [()] (unmutated), every single mutation, then the pairs (every pair_stride-th)."""
    out = [()]
    for pl in places:
        out += [((pl, v),) for v in (VALUES if pl[2] != "null" else (None,))]
    pairs = []
    for a, b in itertools.combinations(places, 2):
        bad_a, bad_b = ({"ptr": BAD_POINTER, "num": BAD_NUMBER, "null": (None, None)}[pl[2]] for pl in (a, b))
        pairs += [((a, bad_a[0]), (b, bad_b[0])), ((a, bad_a[1]), (b, bad_b[1]))]
    return out + pairs[::pair_stride]


PAIR_STRIDE = {"decode_window": 3, "decode_fp8_window": 3}   # (the window forms have the most bases: every third pair)


def describe(case):
    return ", ".join(f"{s}.{p or '*'}={v!r}" for (s, p, _), v in case) or "unmutated"


class _NoLibrary:
    def __getattr__(self, name):
        return None


def cases(lib=None):
    """Every case in order: (entry, base name, base builder, takes ms, call, case).  Without a library: for the labels only."""
    fam_bases = bases()
    for name, fam, launch, call in entries(lib or _NoLibrary()):
        for bname, build in fam_bases[fam]:
            for case in mutations(fields(build(), launch), PAIR_STRIDE.get(fam, 1)):
                yield name, bname, build, launch, call, case


def run(lib=None):
    """-> [(entry, base, case, (rc, message, ms or None))] in cases()' order.  Refuses to start where there is a device."""
    lib = lib or _capi.load()
    rc = lib.fa_init()
    if (rc, _capi.last_error()) != NO_DEVICE:
        raise RuntimeError(f"the host corpus runs only where the library sees no device (fa_init: {rc}, {_capi.last_error()!r}): "
                           "its passing cases would launch with fake pointers")
    out = []
    for name, bname, build, launch, call, case in cases(lib):
        structs = build()
        ms = ctypes.c_float(MS_SENTINEL)
        extra = {"lse": ctypes.c_void_p(16), "ms": ctypes.pointer(ms)}
        for place, value in case:
            apply(structs, extra, place, value)
        lib.fa_fwd_lds_bytes(None)   # (sets the thread's message to "null config": a call that sets none shows that)
        got = call(structs, extra)
        timed = None
        if got == 0 and launch and extra["ms"] is not None:
            timed = ms.value
        elif got == 0 and "opts" in structs and structs["opts"] is not None and structs["opts"].ms:
            timed = structs["opts"].ms.contents.value
        out.append((name, bname, case, (int(got), _capi.last_error(), timed)))
    return out


def pack(results, parent):
    """The golden file's content: the distinct records, and per entry point the cases' indices into them (unsigned 16-bit,
    little-endian, zlib, base64 -- a few hundred thousand small numbers)."""
    table, index, per_entry, base_ok = [], {}, {}, {}
    for name, bname, case, rec in results:
        if rec not in index:
            index[rec] = len(table)
            table.append(list(rec))
        per_entry.setdefault(name, []).append(index[rec])
        if not case:
            base_ok[f"{name}[{bname}]"] = list(rec[:2])
    assert len(table) < 65536
    return {"parent": parent, "n_cases": len(results), "records": table,
            "cases": {n: {"n": len(ix), "indices_u16le_zlib_b64": base64.b64encode(zlib.compress(struct.pack(f"<{len(ix)}H", *ix), 9)).decode()}
                      for n, ix in per_entry.items()},
            "unmutated": base_ok}


def unpack(golden):
    """-> {entry: [record (rc, message, ms)] in case order}"""
    out = {}
    for name, c in golden["cases"].items():
        raw = zlib.decompress(base64.b64decode(c["indices_u16le_zlib_b64"]))
        out[name] = [tuple(golden["records"][i]) for i in struct.unpack(f"<{c['n']}H", raw)]
    return out


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "--record":
        with open(GOLDEN, "w") as f:
            json.dump(pack(run(), sys.argv[2]), f, indent=0, separators=(",", ":"))
            f.write("\n")
    elif sys.argv[1:] == ["--dump"]:
        json.dump(pack(run(), "the library under test"), sys.stdout)
    else:
        sys.exit(__doc__)
