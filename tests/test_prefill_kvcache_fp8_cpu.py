"""Prefill against an fp8 KV cache without a device: the C ABI of fa_fwd_launch_varlen_kvcache_fp8 (struct
layout, exports in both libraries, every refusal it adds before any HIP call, total_q = 0), the resource figures the build keeps
for the new slice, and the Python entry's own refusals."""
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
from tests.conftest import ROOT

BUILD = os.path.join(ROOT, "flash_attention_from_scratch_amd", "csrc", "build")
NEW_SYMBOLS = ("fa_fwd_varlen_kvcache_fp8_supported", "fa_fwd_launch_varlen_kvcache_fp8")
JITTER = os.path.join(ROOT, "flash_attention_from_scratch_amd", "lib", "libfa_hip_jitter.so")


def test_fp8_scales_mirror_matches_the_header():
    fields = [f[0] for f in _capi.FaKvcacheFp8Scales._fields_]
    src = "#include <stdio.h>\n#include <stddef.h>\n#include \"fa_hip.h\"\nint main(void) {\n"
    src += "    printf(\"%zu\", sizeof(fa_kvcache_fp8_scales));\n"
    src += "".join(f"    printf(\" %zu\", offsetof(fa_kvcache_fp8_scales, {f}));\n" for f in fields)
    src += "    printf(\"\\n\");\n    return 0;\n}\n"
    with tempfile.TemporaryDirectory() as tmp:
        open(os.path.join(tmp, "t.c"), "w").write(src)
        subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), os.path.join(tmp, "t.c"), "-o", os.path.join(tmp, "t")], check=True)
        got = [int(x) for x in subprocess.run([os.path.join(tmp, "t")], capture_output=True, text=True, check=True).stdout.split()]
    assert got == [ctypes.sizeof(_capi.FaKvcacheFp8Scales)] + [getattr(_capi.FaKvcacheFp8Scales, f).offset for f in fields]
    assert fields == ["struct_size", "kv_dtype", "k_descale", "v_descale", "descale_batch_stride"]
    sc = _capi.make_kvcache_fp8_scales()
    assert sc.struct_size == ctypes.sizeof(_capi.FaKvcacheFp8Scales) == 4 + 4 + 3 * 8 and sc.kv_dtype == _capi.FA_KV_FP8_E4M3FN == 1
    # the 16-bit call's layout did not grow
    assert ctypes.sizeof(_capi.FaKvcacheLayout) == 8 + 2 * 8 + 7 * 8


def test_fp8_symbols_in_both_libraries_and_the_header():
    assert set(NEW_SYMBOLS) <= set(_capi.EXPORTED_SYMBOLS)
    for path in (_capi.LIB_PATH, JITTER):
        nm = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True)
        exported = set(re.findall(r" T (fa_[a-z_0-9]+)", nm.stdout))
        assert set(NEW_SYMBOLS) <= exported, (path, set(NEW_SYMBOLS) - exported)
    header = open(os.path.join(ROOT, "include", "fa_hip.h")).read()
    declared = set(re.findall(r"\b(fa_[a-z_0-9]+)\s*\(", re.sub(r"/\*.*?\*/", "", header, flags=re.S)))
    assert set(NEW_SYMBOLS) <= declared
    lib = _capi.load()
    assert lib.fa_abi_version() == 6 and _capi.FA_ABI_VERSION == 6
    twin = ctypes.CDLL(JITTER)   # outside the registry: the count is unchanged, and the twin's
    twin.fa_num_kernels.restype = ctypes.c_int
    assert lib.fa_num_kernels() == twin.fa_num_kernels() == len(_capi.kernels())


def _cfg(dtype=torch.bfloat16):
    return fak.varlen_config(dtype)


def _fwd(T=1000, H=8, **over):
    a = _capi.FaFwdArgs(q=16, k=16, v=16, o=16, batch=1, seq_len=T, n_heads=H, d_head=128, batch_stride=0, seq_stride=H * 128,
                        head_stride=128, cfg=_capi.make_config(_cfg()))
    for name, val in over.items():
        setattr(a, name, val)
    return a


def _kv(Hkv=2, bs=4096 * 2 * 128, **over):   # (an fp8 cache: the strides count bytes)
    kv = _capi.make_kv_layout(Hkv, bs, Hkv * 128, 128)
    for name, val in over.items():
        setattr(kv, name, val)
    return kv


def _vl(n_seqs=3, T=1000, max_seqlen=512, cu=16):
    return _capi.make_varlen_layout(cu, n_seqs, T, max_seqlen)


def _contig(**over):
    fields = dict(cache_seqlens=16, seqlen_cache=4096, batch=3)
    fields.update(over)
    return _capi.make_kvcache_layout(**fields)


def _paged(**over):
    fields = dict(cache_seqlens=16, block_table=16, num_pages=100, page_size=256, max_pages_per_seq=16, block_table_stride=16)
    fields.update(over)
    return _capi.make_kvcache_layout(**fields)


def _sc(**over):
    fields = dict(k_descale=16, v_descale=16, descale_batch_stride=2)
    fields.update(over)
    return _capi.make_kvcache_fp8_scales(**fields)


def test_fwd_varlen_kvcache_fp8_supported_is_the_varlen_rule():
    from flash_helpers import kernel_configs as kc

    lib = _capi.load()
    seen = set()
    for c in (_cfg(torch.bfloat16), _cfg(torch.float16), kc.best_config(kc.DType.BF16)):
        cfg = ctypes.byref(_capi.make_config(c))
        for o in (None, _capi.make_opts(causal=True), _capi.make_opts(speculative=True), _capi.make_opts(stats_ptr=16)):
            op = ctypes.byref(o) if o is not None else None
            got = lib.fa_fwd_varlen_kvcache_fp8_supported(cfg, op)
            assert got == lib.fa_fwd_varlen_supported(cfg, op), (c, o)
            seen.add(got)
    assert seen == {0, 1}
    assert lib.fa_fwd_varlen_kvcache_fp8_supported(None, None) == 0


def test_fwd_launch_varlen_kvcache_fp8_refusals_without_a_device():
    lib = _capi.load()
    lse = ctypes.c_void_p(16)

    def launch(args=None, kv=None, kc_=None, sc=None, no_sc=False, opts=None):
        args, kv, kc_, sc = args or _fwd(), kv or _kv(), kc_ or _contig(), sc or _sc()
        opts = opts or _capi.make_opts()
        rc = lib.fa_fwd_launch_varlen_kvcache_fp8(ctypes.byref(args), ctypes.byref(kv), ctypes.byref(_vl()), ctypes.byref(kc_),
                                                  None if no_sc else ctypes.byref(sc), ctypes.byref(opts), lse, None)
        return rc, _capi.last_error()

    page = 256 * 2 * 128
    cases = [
        # the fp8 side's own refusals
        (dict(no_sc=True), -1, "null pointer"),
        (dict(sc=_sc(kv_dtype=0)), -2, "kv_dtype"),
        (dict(sc=_sc(kv_dtype=2)), -2, "kv_dtype"),
        (dict(sc=_sc(struct_size=8)), -4, "fa_kvcache_fp8_scales.struct_size"),
        (dict(sc=_sc(descale_batch_stride=1)), -4, "descale_batch_stride"),
        (dict(sc=_sc(v_descale=None, descale_batch_stride=0)), -4, "descale_batch_stride"),
        (dict(sc=_sc(k_descale=18)), -5, "4-byte aligned"),
        (dict(sc=_sc(v_descale=18)), -5, "4-byte aligned"),
        (dict(kv=_kv(kv_seq_stride=2 * 128 + 8)), -5, "16 bytes"),
        (dict(kv=_kv(kv_head_stride=128 + 8, kv_seq_stride=2 * 128 + 16)), -5, "16 bytes"),
        (dict(kv=_kv(bs=page + 8)), -5, "16 bytes"),
        (dict(args=_fwd(k=24)), -5, "16-byte aligned"),
        (dict(args=_fwd(v=24)), -5, "16-byte aligned"),
        # ... and the 16-bit call's still hold
        (dict(kc_=_paged(page_size=96), kv=_kv(bs=96 * 256)), -3, "multiple of 64"),
        (dict(kc_=_contig(cache_seqlens=None)), -1, "cache_seqlens is null"),
        (dict(kc_=_contig(struct_size=8)), -4, "fa_kvcache_layout.struct_size"),
        (dict(kc_=_contig(batch=4)), -4, "must equal n_seqs"),
        (dict(kv=_kv(bs=0)), -4, "positive"),
        (dict(args=_fwd(d_head=64)), -4, "d_head"),
        (dict(opts=_capi.make_opts(speculative=True)), -3, "variable-length"),
    ]
    for over, status, text in cases:
        rc, msg = launch(**over)
        assert rc == status and text in msg, (over, rc, msg)
    # a descale that is not given needs no stride (null = 1)
    rc = lib.fa_fwd_launch_varlen_kvcache_fp8(ctypes.byref(_fwd(T=0)), ctypes.byref(_kv()), ctypes.byref(_capi.make_varlen_layout(16, 3, 0, 512)),
                                              ctypes.byref(_contig()), ctypes.byref(_sc(k_descale=None, v_descale=None, descale_batch_stride=0)),
                                              ctypes.byref(_capi.make_opts()), lse, None)
    assert rc == 0, _capi.last_error()


def test_total_q_zero_returns_ok_without_a_device():
    lib = _capi.load()
    lse = ctypes.c_void_p(16)
    for kc_, kv in ((_contig(), _kv()), (_paged(), _kv(bs=256 * 2 * 128)), (_paged(page_size=64, max_seqlen_k=100), _kv(bs=64 * 2 * 128))):
        ms = ctypes.c_float(-1.0)
        opts = _capi.make_opts(causal=True, ms=ms)
        rc = lib.fa_fwd_launch_varlen_kvcache_fp8(ctypes.byref(_fwd(T=0)), ctypes.byref(kv), ctypes.byref(_capi.make_varlen_layout(16, 3, 0, 512)),
                                                  ctypes.byref(kc_), ctypes.byref(_sc()), ctypes.byref(opts), lse, None)
        assert rc == 0 and ms.value == 0.0, _capi.last_error()
    # ... but its arguments are still checked
    rc = lib.fa_fwd_launch_varlen_kvcache_fp8(ctypes.byref(_fwd(T=0)), ctypes.byref(_kv()), ctypes.byref(_capi.make_varlen_layout(16, 3, 0, 512)),
                                              ctypes.byref(_contig()), ctypes.byref(_sc(kv_dtype=0)), ctypes.byref(_capi.make_opts()), lse, None)
    assert rc == -2


def test_fp8_slices_are_kept_with_no_scratch_and_no_vector_spill():
    """The figures the compiler writes beside each kernel of the kept ISA (the kernel-resource-usage remarks, as comments and as
    metadata): no scratch, no vector-register spill.  The register figures are printed; DESIGN.md 10.10 records them."""
    for dt in (15, 5):
        path = os.path.join(BUILD, f"varlen_kvcache_fp8_dt{dt}", "fa_inst_varlen-hip-amdgcn-amd-amdhsa-gfx950.s")
        assert os.path.exists(path), "the build keeps the ISA of every slice under csrc/build (make -C flash_attention_from_scratch_amd/csrc)"
        text = open(path).read()
        # the two forms (with and without the first-block skip) of the new kernel, and none of the kernels it is built from
        assert len(re.findall(r"^_ZN2fa32fa_fwd_kernel_varlen_kvcache_fp8I\w+:", text, flags=re.M)) == 2
        assert re.search(r"^_ZN2fa28fa_fwd_kernel_varlen_kvcacheI", text, flags=re.M) is None
        assert re.search(r"^_ZN2fa20fa_fwd_kernel_varlenI", text, flags=re.M) is None
        assert re.search(r"^_ZN2fa13fa_fwd_kernelI", text, flags=re.M) is None
        assert re.findall(r"; ScratchSize: (\d+)", text) == ["0", "0"]
        assert re.findall(r"\.private_segment_fixed_size:\s+(\d+)", text) == ["0", "0"]
        assert re.findall(r"\.vgpr_spill_count:\s+(\d+)", text) == ["0", "0"]
        sgpr_spills = [int(x) for x in re.findall(r"\.sgpr_spill_count:\s+(\d+)", text)]
        figures = {name: re.findall(rf"; {name}: (\d+)", text) for name in ("NumVgprs", "NumAgprs", "TotalNumSgprs", "Occupancy")}
        print(f"dt{dt}: sgpr_spill_count {sgpr_spills} {figures}")
        assert len(sgpr_spills) == 2
    # the 16-bit cache's slice keeps its two kernels
    for dt in (15, 5):
        text = open(os.path.join(BUILD, f"varlen_kvcache_dt{dt}", "fa_inst_varlen-hip-amdgcn-amd-amdhsa-gfx950.s")).read()
        assert len(re.findall(r"^_ZN2fa28fa_fwd_kernel_varlen_kvcacheI\w+:", text, flags=re.M)) == 2
        assert "kvcache_fp8" not in text


def test_python_entry_takes_descales_and_refuses_before_the_device():
    from flash_attention_from_scratch_amd import flash_attention as inner

    assert flash_attention.forward_varlen_kvcache is inner.forward_varlen_kvcache
    q = torch.zeros((4, 2, 128), dtype=torch.bfloat16)
    cache = torch.zeros((1, 64, 2, 128), dtype=torch.bfloat16)
    c8 = cache.to(torch.float8_e4m3fn)
    cu = torch.tensor([0, 4], dtype=torch.int32)
    lens = torch.tensor([4], dtype=torch.int32)
    ones = torch.ones((1, 2), dtype=torch.float32)
    for fn in (flash_attention.forward_varlen_kvcache, fak.forward_varlen_kvcache):
        # one descale only, or none: refused, and told to pass both
        for kw in (dict(k_descale=ones), dict(v_descale=ones), dict()):
            with pytest.raises(RuntimeError, match="fp8 cache is not served without both k_descale and v_descale"):
                fn(q, c8, c8, cu, 4, lens, **kw)
        # a descale with a 16-bit cache
        for kw in (dict(k_descale=ones), dict(v_descale=ones), dict(k_descale=ones, v_descale=ones)):
            with pytest.raises(RuntimeError, match="belong to an fp8"):
                fn(q, cache, cache, cu, 4, lens, **kw)
        # two cache dtypes, another fp8 encoding
        with pytest.raises(RuntimeError, match="one data type"):
            fn(q, c8, cache, cu, 4, lens, k_descale=ones, v_descale=ones)
        with pytest.raises(RuntimeError, match="one data type"):
            fn(q, cache, c8, cu, 4, lens, k_descale=ones, v_descale=ones)
        with pytest.raises(RuntimeError, match="must be torch.float8_e4m3fn"):
            fn(q, cache.to(torch.float8_e5m2), cache.to(torch.float8_e5m2), cu, 4, lens, k_descale=ones, v_descale=ones)
        with pytest.raises(RuntimeError, match="k_descale must be a tensor"):
            fn(q, c8, c8, cu, 4, lens, k_descale=1.0, v_descale=ones)
        # both given: the call goes on to the device checks (the descales among them)
        with pytest.raises(RuntimeError, match="must be a CUDA tensor"):
            fn(q, c8, c8, cu, 4, lens, k_descale=ones, v_descale=ones)


def test_python_entry_checks_the_descales_shape_and_dtype():
    """What the descales are (dtype, shape, a contiguous last dimension) is checked before where they are: reached without a GPU."""
    q = torch.zeros((4, 2, 128), dtype=torch.bfloat16)
    c8 = torch.zeros((1, 64, 2, 128), dtype=torch.bfloat16).to(torch.float8_e4m3fn)
    cu = torch.tensor([0, 4], dtype=torch.int32)
    lens = torch.tensor([4], dtype=torch.int32)
    ones = torch.ones((1, 2), dtype=torch.float32)
    bad = [ones.double(), ones.half(), torch.ones((2, 2)), torch.ones((1, 1)), torch.ones((2,)), torch.ones((1, 4))[:, ::2]]
    for fn in (flash_attention.forward_varlen_kvcache, fak.forward_varlen_kvcache):
        for t in bad:
            with pytest.raises(RuntimeError, match="k_descale must be an fp32"):
                fn(q, c8, c8, cu, 4, lens, k_descale=t, v_descale=ones)
            with pytest.raises(RuntimeError, match="v_descale must be an fp32"):
                fn(q, c8, c8, cu, 4, lens, k_descale=ones, v_descale=t)
        # a single row of any stride is a valid shape: the call goes on to the device checks
        with pytest.raises(RuntimeError, match="must be a CUDA tensor"):
            fn(q, c8, c8, cu, 4, lens, k_descale=torch.ones((2,))[None], v_descale=ones)
