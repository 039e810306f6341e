"""Prefill against a KV cache without a device: the C ABI of fa_fwd_launch_varlen_kvcache (struct layout, exports
in both libraries, every refusal before any HIP call, total_q = 0), the ISA and the resource figures the build keeps for the new
slice, and the Python entry's own refusals."""
import ctypes
import os
import re
import subprocess
import tempfile

import pytest
import torch

import flash_attention
from flash_attention_from_scratch_amd import _capi
from flash_attention_from_scratch_amd import flash_attention_kernels as fak
from flash_helpers import kernel_configs as kc
from tests.conftest import ROOT

BUILD = os.path.join(ROOT, "flash_attention_from_scratch_amd", "csrc", "build")
NEW_SYMBOLS = ("fa_fwd_varlen_kvcache_supported", "fa_fwd_launch_varlen_kvcache")
JITTER = os.path.join(ROOT, "flash_attention_from_scratch_amd", "lib", "libfa_hip_jitter.so")


def test_kvcache_layout_mirror_matches_the_header():
    fields = [f[0] for f in _capi.FaKvcacheLayout._fields_]
    src = "#include <stdio.h>\n#include <stddef.h>\n#include \"fa_hip.h\"\nint main(void) {\n"
    src += "    printf(\"%zu\", sizeof(fa_kvcache_layout));\n"
    src += "".join(f"    printf(\" %zu\", offsetof(fa_kvcache_layout, {f}));\n" for f in fields)
    src += "    printf(\"\\n\");\n    return 0;\n}\n"
    with tempfile.TemporaryDirectory() as tmp:
        open(os.path.join(tmp, "t.c"), "w").write(src)
        subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), os.path.join(tmp, "t.c"), "-o", os.path.join(tmp, "t")], check=True)
        got = [int(x) for x in subprocess.run([os.path.join(tmp, "t")], capture_output=True, text=True, check=True).stdout.split()]
    assert got == [ctypes.sizeof(_capi.FaKvcacheLayout)] + [getattr(_capi.FaKvcacheLayout, f).offset for f in fields]
    assert fields[0] == "struct_size" and _capi.FaKvcacheLayout.struct_size.offset == 0
    assert fields[1:] == ["cache_seqlens", "block_table", "seqlen_cache", "num_pages", "page_size", "max_pages_per_seq",
                          "block_table_stride", "max_seqlen_k", "batch"]
    assert _capi.make_kvcache_layout().struct_size == ctypes.sizeof(_capi.FaKvcacheLayout) == 8 + 2 * 8 + 7 * 8


def test_kvcache_symbols_in_both_libraries_and_the_header():
    assert set(NEW_SYMBOLS) <= set(_capi.EXPORTED_SYMBOLS)
    for path in (_capi.LIB_PATH, JITTER):
        nm = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True)
        exported = set(re.findall(r" T (fa_[a-z_0-9]+)", nm.stdout))
        assert set(NEW_SYMBOLS) <= exported, (path, set(NEW_SYMBOLS) - exported)
        assert set(_capi.EXPORTED_SYMBOLS) <= exported, (path, set(_capi.EXPORTED_SYMBOLS) - exported)
    header = open(os.path.join(ROOT, "include", "fa_hip.h")).read()
    declared = set(re.findall(r"\b(fa_[a-z_0-9]+)\s*\(", re.sub(r"/\*.*?\*/", "", header, flags=re.S)))
    assert declared == set(_capi.EXPORTED_SYMBOLS), declared ^ set(_capi.EXPORTED_SYMBOLS)
    lib = _capi.load()
    assert lib.fa_abi_version() == 6 and _capi.FA_ABI_VERSION == 6
    twin = ctypes.CDLL(JITTER)   # the new kernels are outside the registry: the count is unchanged, and the twin's
    twin.fa_num_kernels.restype = ctypes.c_int
    assert lib.fa_num_kernels() == twin.fa_num_kernels() == len(_capi.kernels())


def _cfg(dtype=torch.bfloat16):
    return fak.varlen_config(dtype)


def _fwd(cfg=None, T=1000, H=8, **over):
    a = _capi.FaFwdArgs(q=16, k=16, v=16, o=16, batch=1, seq_len=T, n_heads=H, d_head=128, batch_stride=0, seq_stride=H * 128,
                        head_stride=128, cfg=_capi.make_config(cfg or _cfg()))
    for name, val in over.items():
        setattr(a, name, val)
    return a


def _kv(Hkv=2, bs=4096 * 2 * 128, **over):
    kv = _capi.make_kv_layout(Hkv, bs, Hkv * 128, 128)
    for name, val in over.items():
        setattr(kv, name, val)
    return kv


def _vl(n_seqs=3, T=1000, max_seqlen=512, cu=16, **over):
    vl = _capi.make_varlen_layout(cu, n_seqs, T, max_seqlen)
    for name, val in over.items():
        setattr(vl, name, val)
    return vl


def _contig(**over):
    fields = dict(cache_seqlens=16, seqlen_cache=4096, batch=3)
    fields.update(over)
    return _capi.make_kvcache_layout(**fields)


def _paged(**over):
    fields = dict(cache_seqlens=16, block_table=16, num_pages=100, page_size=256, max_pages_per_seq=16, block_table_stride=16)
    fields.update(over)
    return _capi.make_kvcache_layout(**fields)


def test_fwd_varlen_kvcache_supported_is_the_varlen_rule():
    lib = _capi.load()
    opts = [None, _capi.make_opts(), _capi.make_opts(causal=True), _capi.make_opts(speculative=True), _capi.make_opts(prescaled_q=True),
            _capi.make_opts(stats_ptr=16), _capi.make_opts(allow_ragged=True)]
    cfgs = [_cfg(torch.bfloat16), _cfg(torch.float16), kc.best_config(kc.DType.BF16), kc.best_config(kc.DType.FP16)]
    seen = set()
    for c in cfgs:
        cfg = ctypes.byref(_capi.make_config(c))
        for o in opts:
            op = ctypes.byref(o) if o is not None else None
            got = lib.fa_fwd_varlen_kvcache_supported(cfg, op)
            assert got == lib.fa_fwd_varlen_supported(cfg, op), (c, o)
            seen.add(got)
    assert seen == {0, 1}
    assert lib.fa_fwd_varlen_kvcache_supported(None, None) == 0


def test_fwd_launch_varlen_kvcache_refusals_without_a_device():
    lib = _capi.load()
    lse = ctypes.c_void_p(16)

    def launch(args=None, kv=None, vq=None, kc_=None, opts=None, lse=lse, no_kv=False, no_vq=False, no_kc=False):
        args, kv, vq, kc_ = args or _fwd(), kv or _kv(), vq or _vl(), kc_ or _contig()
        opts = opts or _capi.make_opts()
        rc = lib.fa_fwd_launch_varlen_kvcache(ctypes.byref(args), None if no_kv else ctypes.byref(kv), None if no_vq else ctypes.byref(vq),
                                              None if no_kc else ctypes.byref(kc_), ctypes.byref(opts), lse, None)
        return rc, _capi.last_error()

    page = 256 * 2 * 128
    cases = [
        # null pointers
        (dict(no_kv=True), -1, "null pointer"),
        (dict(no_vq=True), -1, "null pointer"),
        (dict(no_kc=True), -1, "null pointer"),
        (dict(args=_fwd(q=None)), -1, "null pointer"),
        (dict(args=_fwd(k=None)), -1, "null pointer"),
        (dict(lse=None), -1, "lse is null"),
        (dict(vq=_vl(cu=None)), -1, "cu_seqlens is null"),
        (dict(kc_=_contig(cache_seqlens=None)), -1, "cache_seqlens is null"),
        (dict(kc_=_paged(cache_seqlens=None), kv=_kv(bs=page)), -1, "cache_seqlens is null"),
        # the page size: no kernel
        (dict(kc_=_paged(page_size=96), kv=_kv(bs=96 * 256)), -3, "multiple of 64"),
        (dict(kc_=_paged(page_size=32), kv=_kv(bs=32 * 256)), -3, "multiple of 64"),
        # sizes that are not positive, and the bounds
        (dict(kc_=_contig(seqlen_cache=0)), -4, "seqlen_cache"),
        (dict(kc_=_contig(seqlen_cache=-64)), -4, "seqlen_cache"),
        (dict(kc_=_paged(page_size=0), kv=_kv(bs=page)), -4, "must be positive"),
        (dict(kc_=_paged(num_pages=0), kv=_kv(bs=page)), -4, "must be positive"),
        (dict(kc_=_paged(max_pages_per_seq=0), kv=_kv(bs=page)), -4, "must be positive"),
        (dict(kc_=_paged(block_table_stride=15), kv=_kv(bs=page)), -4, "block_table_stride"),
        (dict(kc_=_contig(max_seqlen_k=-1)), -4, "max_seqlen_k"),
        (dict(kc_=_contig(max_seqlen_k=4097)), -4, "max_seqlen_k"),
        (dict(kc_=_paged(max_seqlen_k=16 * 256 + 1), kv=_kv(bs=page)), -4, "max_seqlen_k"),
        (dict(kc_=_contig(seqlen_cache=1 << 31)), -4, "too large"),
        (dict(kc_=_paged(num_pages=1 << 31), kv=_kv(bs=page)), -4, "too large"),
        (dict(kc_=_contig(struct_size=8)), -4, "fa_kvcache_layout.struct_size"),
        # a contiguous cache: one batch entry per sequence
        (dict(kc_=_contig(batch=4)), -4, "must equal n_seqs"),
        (dict(kc_=_contig(batch=0)), -4, "must equal n_seqs"),
        # strides
        (dict(kv=_kv(bs=0)), -4, "positive"),
        (dict(kv=_kv(bs=-page)), -4, "positive"),
        (dict(kc_=_paged(), kv=_kv(bs=0)), -4, "positive"),
        (dict(kv=_kv(bs=page + 4)), -5, "multiples of 8"),
        (dict(kv=_kv(kv_seq_stride=2 * 128 + 4)), -5, "multiples of 8"),
        (dict(kv=_kv(kv_head_stride=-128)), -4, "positive"),
        (dict(args=_fwd(seq_stride=0)), -4, "positive"),
        (dict(args=_fwd(head_stride=132)), -5, "multiples of 8"),
        # alignment
        (dict(kc_=_contig(cache_seqlens=18)), -5, "4-byte aligned"),
        (dict(kc_=_paged(block_table=18), kv=_kv(bs=page)), -5, "4-byte aligned"),
        (dict(vq=_vl(cu=18)), -5, "cu_seqlens must be 4-byte"),
        (dict(lse=ctypes.c_void_p(18)), -5, "lse must be 4-byte"),
        (dict(args=_fwd(k=24)), -5, "16-byte aligned"),
        (dict(args=_fwd(v=24)), -5, "16-byte aligned"),
        # fa_fwd_launch_varlen's own: d_head, head counts, layouts, struct sizes, the grid
        (dict(args=_fwd(d_head=64)), -4, "d_head"),
        (dict(kv=_kv(Hkv=3)), -4, "divide"),
        (dict(args=_fwd(n_heads=0)), -4, "n_heads"),
        (dict(vq=_vl(struct_size=4)), -4, "struct_size"),
        (dict(kv=_kv(struct_size=4)), -4, "struct_size"),
        (dict(vq=_vl(n_seqs=0)), -4, "n_seqs"),
        (dict(vq=_vl(T=-1)), -4, "total_tokens"),
        (dict(vq=_vl(max_seqlen=0)), -4, "max_seqlen"),
        (dict(vq=_vl(n_seqs=1 << 20, max_seqlen=1 << 20), kc_=_contig(batch=1 << 20)), -4, "too large"),
        # configurations and options without a varlen form
        (dict(args=_fwd(cfg=kc.best_config(kc.DType.BF16))), -3, "variable-length"),
        (dict(opts=_capi.make_opts(speculative=True)), -3, "variable-length"),
        (dict(opts=_capi.make_opts(prescaled_q=True)), -3, "variable-length"),
        (dict(opts=_capi.make_opts(stats_ptr=16)), -3, "variable-length"),
    ]
    for over, status, text in cases:
        rc, msg = launch(**over)
        assert rc == status and text in msg, (over, rc, msg)
    bad = _fwd()
    bad.cfg.dtype = 7
    rc, msg = launch(args=bad)
    assert rc == -2 and "fp16 and bf16" in msg


def test_total_q_zero_returns_ok_without_a_device():
    lib = _capi.load()
    lse = ctypes.c_void_p(16)
    for kc_, kv in ((_contig(), _kv()), (_paged(), _kv(bs=256 * 2 * 128)), (_paged(page_size=64, max_seqlen_k=100), _kv(bs=64 * 2 * 128))):
        ms = ctypes.c_float(-1.0)
        opts = _capi.make_opts(causal=True, ms=ms)
        rc = lib.fa_fwd_launch_varlen_kvcache(ctypes.byref(_fwd(T=0)), ctypes.byref(kv), ctypes.byref(_vl(T=0)), ctypes.byref(kc_),
                                              ctypes.byref(opts), lse, None)
        assert rc == 0 and ms.value == 0.0, _capi.last_error()
    # ... but its arguments are still checked
    rc = lib.fa_fwd_launch_varlen_kvcache(ctypes.byref(_fwd(T=0)), ctypes.byref(_kv()), ctypes.byref(_vl(T=0)),
                                          ctypes.byref(_paged(page_size=96)), ctypes.byref(_capi.make_opts()), lse, None)
    assert rc == -3


def _isa(folder, unit):
    path = os.path.join(BUILD, folder, f"{unit}-hip-amdgcn-amd-amdhsa-gfx950.s")
    assert os.path.exists(path), "the build keeps the ISA of every slice under csrc/build (make -C flash_attention_from_scratch_amd/csrc)"
    return open(path).read()


def test_kvcache_slices_are_kept_with_no_scratch_and_no_vector_spill():
    """The figures the compiler writes beside each kernel of the kept ISA (the kernel-resource-usage remarks, as comments and as
    metadata): no scratch, no vector-register spill; scalars spilled to lanes are allowed and recorded in DESIGN.md 10.9."""
    for dt in (15, 5):
        text = _isa(f"varlen_kvcache_dt{dt}", "fa_inst_varlen")
        # the two forms (with and without the first-block skip) of the new kernel, and neither kernel it is built from
        assert len(re.findall(r"^_ZN2fa28fa_fwd_kernel_varlen_kvcacheI\w+:", text, flags=re.M)) == 2
        assert re.search(r"^_ZN2fa20fa_fwd_kernel_varlenI", text, flags=re.M) is None
        assert re.search(r"^_ZN2fa13fa_fwd_kernelI", text, flags=re.M) is None
        scratch = re.findall(r"; ScratchSize: (\d+)", text)
        assert scratch == ["0", "0"], scratch
        assert re.findall(r"\.private_segment_fixed_size:\s+(\d+)", text) == ["0", "0"]
        assert re.findall(r"\.vgpr_spill_count:\s+(\d+)", text) == ["0", "0"]
        assert re.findall(r"; Occupancy: (\d+)", text) == ["1", "1"]
        sgpr_spills = [int(x) for x in re.findall(r"\.sgpr_spill_count:\s+(\d+)", text)]
        figures = {name: re.findall(rf"; {name}: (\d+)", text) for name in ("NumVgprs", "NumAgprs", "TotalNumSgprs")}
        print(f"dt{dt}: sgpr_spill_count {sgpr_spills} {figures}")
        assert len(sgpr_spills) == 2
    # the packed kernel's slice is still there, with its two forms
    for dt in (15, 5):
        assert len(re.findall(r"^_ZN2fa20fa_fwd_kernel_varlenI\w+:", _isa(f"varlen_dt{dt}", "fa_inst_varlen"), flags=re.M)) == 2


def test_python_entry_is_exposed_and_refuses_before_the_device():
    from flash_attention_from_scratch_amd import flash_attention as inner

    assert flash_attention.forward_varlen_kvcache is inner.forward_varlen_kvcache and callable(fak.forward_varlen_kvcache)
    q = torch.zeros((4, 2, 128), dtype=torch.bfloat16)
    cache = torch.zeros((1, 64, 2, 128), dtype=torch.bfloat16)
    cu = torch.tensor([0, 4], dtype=torch.int32)
    lens = torch.tensor([4], dtype=torch.int32)
    for fn in (flash_attention.forward_varlen_kvcache, fak.forward_varlen_kvcache):
        with pytest.raises(RuntimeError, match="fp8 cache is not served"):
            fn(q, cache.to(torch.float8_e4m3fn), cache.to(torch.float8_e4m3fn), cu, 4, lens)
        with pytest.raises(RuntimeError, match="must be a CUDA tensor"):
            fn(q, cache, cache, cu, 4, lens)
        with pytest.raises(RuntimeError, match="must be a tensor"):
            fn(q, cache, cache, [0, 4], 4, lens)
