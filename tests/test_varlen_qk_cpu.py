"""Packed sequences with separate Q and K / V lengths without a device: the C ABI of fa_fwd_launch_varlen_qk /
fa_bwd_launch_varlen_qk (struct layout, exports, validation before any HIP call, the backward's workspace and split rule), the
ISA the build keeps for the new slices, and the Python keyword pair."""
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
NEW_SYMBOLS = ("fa_fwd_varlen_qk_supported", "fa_fwd_launch_varlen_qk", "fa_bwd_varlen_qk_workspace_bytes", "fa_bwd_launch_varlen_qk")
JITTER = os.path.join(ROOT, "flash_attention_from_scratch_amd", "lib", "libfa_hip_jitter.so")


def _layout(struct, cname):
    """[sizeof, offsetof(field) ...] of `cname` from a C program compiled against include/fa_hip.h"""
    fields = [f[0] for f in struct._fields_]
    src = "#include <stdio.h>\n#include <stddef.h>\n#include \"fa_hip.h\"\nint main(void) {\n"
    src += f"    printf(\"%zu\", sizeof({cname}));\n"
    src += "".join(f"    printf(\" %zu\", offsetof({cname}, {f}));\n" for f in fields)
    src += "    printf(\"\\n\");\n    return 0;\n}\n"
    with tempfile.TemporaryDirectory() as tmp:
        open(os.path.join(tmp, "t.c"), "w").write(src)
        subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), os.path.join(tmp, "t.c"), "-o", os.path.join(tmp, "t")], check=True)
        got = [int(x) for x in subprocess.run([os.path.join(tmp, "t")], capture_output=True, text=True, check=True).stdout.split()]
    return got, [ctypes.sizeof(struct)] + [getattr(struct, f).offset for f in fields]


def test_varlen_qk_struct_mirror_matches_the_header():
    got, want = _layout(_capi.FaBwdVarlenQKArgs, "fa_bwd_varlen_qk_args")
    assert got == want
    # struct_size (padded to 8), the fields of fa_bwd_varlen_args, a second layout
    assert ctypes.sizeof(_capi.FaBwdVarlenQKArgs) == 8 + ctypes.sizeof(_capi.FaBwdVarlenArgs) + ctypes.sizeof(_capi.FaVarlenLayout)
    names = [f[0] for f in _capi.FaBwdVarlenQKArgs._fields_]
    assert names == ["struct_size"] + [f[0] for f in _capi.FaBwdVarlenArgs._fields_] + ["varlen_k"]
    # the existing structs keep their size (ABI 6)
    assert ctypes.sizeof(_capi.FaVarlenLayout) == 40 and ctypes.sizeof(_capi.FaBwdVarlenArgs) == 10 * 8 + 11 * 8 + 8 + 40


def test_varlen_qk_symbols_abi_version_and_registry():
    assert set(NEW_SYMBOLS) <= set(_capi.EXPORTED_SYMBOLS)
    for path in (_capi.LIB_PATH, JITTER):
        nm = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True)
        exported = set(re.findall(r" T (fa_[a-z_0-9]+)", nm.stdout))
        assert set(NEW_SYMBOLS) <= exported, (path, set(NEW_SYMBOLS) - exported)
    header = open(os.path.join(ROOT, "include", "fa_hip.h")).read()
    for sym in NEW_SYMBOLS:
        assert re.search(rf"\b{sym}\(", header), sym
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


def _kv(Hkv=2, **over):
    kv = _capi.make_kv_layout(Hkv, 0, Hkv * 128, 128)
    for name, val in over.items():
        setattr(kv, name, val)
    return kv


def _vl(n_seqs=3, T=1000, max_seqlen=512, cu=16, **over):
    vl = _capi.make_varlen_layout(cu, n_seqs, T, max_seqlen)
    for name, val in over.items():
        setattr(vl, name, val)
    return vl


def test_fwd_varlen_qk_supported_is_the_varlen_rule():
    lib = _capi.load()
    opts = [None, _capi.make_opts(), _capi.make_opts(causal=True), _capi.make_opts(speculative=True), _capi.make_opts(prescaled_q=True),
            _capi.make_opts(stats_ptr=16), _capi.make_opts(allow_ragged=True)]
    cfgs = [_cfg(torch.bfloat16), _cfg(torch.float16), kc.best_config(kc.DType.BF16), kc.best_config(kc.DType.FP16)]
    seen = set()
    for c in cfgs:
        cfg = ctypes.byref(_capi.make_config(c))
        for o in opts:
            op = ctypes.byref(o) if o is not None else None
            got = lib.fa_fwd_varlen_qk_supported(cfg, op)
            assert got == lib.fa_fwd_varlen_supported(cfg, op), (c, o)
            seen.add(got)
    assert seen == {0, 1}
    assert lib.fa_fwd_varlen_qk_supported(None, None) == 0
    assert lib.fa_fwd_varlen_qk_supported(ctypes.byref(_capi.make_config(_cfg())), ctypes.byref(_capi.make_opts(causal=True))) == 1


def test_fwd_launch_varlen_qk_refusals_without_a_device():
    lib = _capi.load()
    lse = ctypes.c_void_p(16)

    def launch(args=None, kv=None, vq=None, vk=None, opts=None, lse=lse, no_kv=False, no_vq=False, no_vk=False):
        args, kv, vq, vk = args or _fwd(), kv or _kv(), vq or _vl(), vk or _vl(T=5000, max_seqlen=4096)
        opts = opts or _capi.make_opts()
        rc = lib.fa_fwd_launch_varlen_qk(ctypes.byref(args), None if no_kv else ctypes.byref(kv), None if no_vq else ctypes.byref(vq),
                                         None if no_vk else ctypes.byref(vk), ctypes.byref(opts), lse, None)
        return rc, _capi.last_error()

    cases = [
        # null pointers
        (dict(no_kv=True), -1, "null pointer"),
        (dict(no_vq=True), -1, "null pointer"),
        (dict(no_vk=True), -1, "null pointer"),
        (dict(args=_fwd(q=None)), -1, "null pointer"),
        (dict(lse=None), -1, "lse is null"),
        (dict(vq=_vl(cu=None)), -1, "cu_seqlens is null"),
        (dict(vk=_vl(cu=None)), -1, "cu_seqlens is null"),
        # d_head, head counts
        (dict(args=_fwd(d_head=64)), -4, "d_head"),
        (dict(kv=_kv(Hkv=3)), -4, "divide"),
        (dict(kv=_kv(Hkv=0)), -4, "divide"),
        (dict(args=_fwd(n_heads=0)), -4, "n_heads"),
        # strides and alignment
        (dict(vq=_vl(cu=18)), -5, "cu_seqlens must be 4-byte"),
        (dict(vk=_vl(cu=18)), -5, "cu_seqlens must be 4-byte"),
        (dict(lse=ctypes.c_void_p(18)), -5, "lse must be 4-byte"),
        (dict(args=_fwd(k=24)), -5, "16-byte aligned"),
        (dict(kv=_kv(kv_seq_stride=2 * 128 + 4)), -5, "multiples of 8"),
        (dict(kv=_kv(kv_head_stride=-128)), -4, "positive"),
        (dict(args=_fwd(seq_stride=0)), -4, "positive"),
        (dict(args=_fwd(head_stride=132)), -5, "multiples of 8"),
        # struct_size
        (dict(vq=_vl(struct_size=4)), -4, "struct_size"),
        (dict(vk=_vl(struct_size=4)), -4, "struct_size"),
        (dict(kv=_kv(struct_size=4)), -4, "struct_size"),
        # the layouts: each side's bounds, one sequence count
        (dict(vq=_vl(n_seqs=0)), -4, "n_seqs"),
        (dict(vk=_vl(T=-1)), -4, "total_tokens"),
        (dict(vk=_vl(max_seqlen=0)), -4, "max_seqlen"),
        (dict(vq=_vl(n_seqs=3), vk=_vl(n_seqs=4)), -4, "n_seqs mismatch"),
        # the 32-bit stride bound, both sides
        (dict(args=_fwd(seq_stride=(1 << 23) + 8)), -4, "too large"),
        (dict(kv=_kv(kv_seq_stride=(1 << 23) + 8)), -4, "too large"),
        (dict(vq=_vl(n_seqs=1 << 20, max_seqlen=1 << 20), vk=_vl(n_seqs=1 << 20)), -4, "too large"),
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
    # total_q = 0: nothing to do, no device needed (whatever the key side holds)
    assert launch(vq=_vl(T=0))[0] == 0
    assert launch(vq=_vl(T=0), vk=_vl(T=0))[0] == 0


def _bwd(n_seqs=3, T=1000, max_seqlen=512, Tk=None, max_seqlen_k=None, H=8, Hkv=2, causal=0, k_over=None, **over):
    Tk = T if Tk is None else Tk
    max_seqlen_k = max_seqlen if max_seqlen_k is None else max_seqlen_k
    a = _capi.FaBwdVarlenQKArgs(struct_size=ctypes.sizeof(_capi.FaBwdVarlenQKArgs),
                                q=16, k=16, v=16, o=16, dout=16, lse=ctypes.cast(ctypes.c_void_p(16), ctypes.POINTER(ctypes.c_float)),
                                dq=16, dk=16, dv=16, workspace=16, n_heads=H, n_kv_heads=Hkv, d_head=128,
                                q_seq_stride=H * 128, q_head_stride=128, out_seq_stride=H * 128, out_head_stride=128,
                                kv_seq_stride=Hkv * 128, kv_head_stride=128, dkv_seq_stride=Hkv * 128, dkv_head_stride=128,
                                dtype=15, causal=causal, varlen=_capi.make_varlen_layout(16, n_seqs, T, max_seqlen),
                                varlen_k=_capi.make_varlen_layout(16, n_seqs, Tk, max_seqlen_k))
    for name, val in over.items():
        setattr(a, name, val)
    for name, val in (k_over or {}).items():
        setattr(a.varlen_k, name, val)
    return a


def _bwd_eq(n_seqs, T, max_seqlen, H, Hkv, causal):
    return _capi.FaBwdVarlenArgs(q=16, k=16, v=16, o=16, dout=16, lse=ctypes.cast(ctypes.c_void_p(16), ctypes.POINTER(ctypes.c_float)),
                                 dq=16, dk=16, dv=16, workspace=16, n_heads=H, n_kv_heads=Hkv, d_head=128,
                                 q_seq_stride=H * 128, q_head_stride=128, out_seq_stride=H * 128, out_head_stride=128,
                                 kv_seq_stride=Hkv * 128, kv_head_stride=128, dkv_seq_stride=Hkv * 128, dkv_head_stride=128,
                                 dtype=15, causal=causal, varlen=_capi.make_varlen_layout(16, n_seqs, T, max_seqlen))


def _expected_split(n_seqs, max_seqlen_k, H, Hkv, causal):
    """DESIGN 9.2's rule with max_seqlen_k: the smallest divisor of the group whose workgroup count reaches 256 (1024 causal)"""
    group, wgs = H // Hkv, n_seqs * Hkv * ((max_seqlen_k + 127) // 128)
    for s in range(1, group):
        if group % s == 0 and wgs * s >= (1024 if causal else 256):
            return s
    return group


SPLIT_TABLE = [   # (n_seqs, max_seqlen_k, H, Hkv, causal)
    (16, 4096, 16, 16, 0), (16, 4096, 16, 4, 0), (4, 4096, 16, 1, 0), (4, 4096, 16, 4, 1), (4, 4096, 16, 1, 1), (1, 1000, 8, 1, 0),
    (3, 1024, 8, 2, 0), (3, 8192, 8, 2, 0), (1, 4096, 16, 4, 0), (8, 32768, 32, 8, 1), (8, 8192, 32, 8, 1), (2, 300, 4, 1, 1),
]


@pytest.mark.parametrize("case", SPLIT_TABLE)
def test_bwd_varlen_qk_workspace_and_split_rule(case):
    n_seqs, max_k, H, Hkv, causal = case
    lib = _capi.load()
    # a short query side against the table's key side: delta over total_q, the partials over total_k, the split from the key side
    Tq, Tk = 7 * n_seqs + 1, max_k * n_seqs - 3
    a = _bwd(n_seqs=n_seqs, T=Tq, max_seqlen=64, Tk=Tk, max_seqlen_k=max_k, H=H, Hkv=Hkv, causal=causal)
    split = _expected_split(n_seqs, max_k, H, Hkv, causal)
    want = ((4 * H * Tq + 15) & ~15) + (4 * Hkv * split * Tk * 2 * 128 if split > 1 else 0)
    assert lib.fa_bwd_varlen_qk_workspace_bytes(ctypes.byref(a)) == want, (case, split)
    # the query side's max_seqlen does not enter the split
    a2 = _bwd(n_seqs=n_seqs, T=Tq, max_seqlen=1 << 16, Tk=Tk, max_seqlen_k=max_k, H=H, Hkv=Hkv, causal=causal)
    assert lib.fa_bwd_varlen_qk_workspace_bytes(ctypes.byref(a2)) == want
    # equal sides: the existing entry point's bytes (the same split)
    T = max_k * n_seqs - 3
    eq = _bwd(n_seqs=n_seqs, T=T, max_seqlen=max_k, H=H, Hkv=Hkv, causal=causal)
    assert lib.fa_bwd_varlen_qk_workspace_bytes(ctypes.byref(eq)) == \
        lib.fa_bwd_varlen_workspace_bytes(ctypes.byref(_bwd_eq(n_seqs, T, max_k, H, Hkv, causal)))


def test_bwd_varlen_qk_refusals_without_a_device():
    lib = _capi.load()
    assert lib.fa_bwd_varlen_qk_workspace_bytes(None) == -1
    assert lib.fa_bwd_varlen_qk_workspace_bytes(ctypes.byref(_bwd(Hkv=3))) == -4
    vl = lambda **kw: _capi.make_varlen_layout(kw.pop("cu", 16), kw.pop("n_seqs", 3), kw.pop("T", 1000), kw.pop("max_seqlen", 512))   # noqa: E731
    cases = [
        # null pointers
        (dict(lse=None), -1, "lse is null"),
        (dict(dk=None), -1, "null tensor pointer"),
        (dict(q=None), -1, "null tensor pointer"),
        (dict(workspace=None), -1, "workspace is null"),
        (dict(varlen=vl(cu=None)), -1, "cu_seqlens is null"),
        (dict(k_over=dict(cu_seqlens=None)), -1, "cu_seqlens is null"),
        # dtype, d_head, head counts
        (dict(dtype=7), -2, "fp16 and bf16"),
        (dict(d_head=64), -4, "d_head = 128"),
        (dict(Hkv=3), -4, "divide"),
        (dict(n_heads=0), -4, "n_heads"),
        # strides and alignment
        (dict(kv_seq_stride=2 * 128 + 4), -5, "multiples of 8"),
        (dict(dkv_head_stride=4), -5, "multiples of 8"),
        (dict(dkv_seq_stride=-256), -4, "positive"),
        (dict(out_seq_stride=0), -4, "positive"),
        (dict(workspace=20), -5, "workspace must be 16-byte"),
        (dict(q=24), -5, "16-byte aligned"),
        (dict(varlen=vl(cu=18)), -5, "cu_seqlens must be 4-byte"),
        (dict(k_over=dict(cu_seqlens=18)), -5, "cu_seqlens must be 4-byte"),
        # struct_size: the arguments' own, and either layout's
        (dict(struct_size=8), -4, "fa_bwd_varlen_qk_args.struct_size"),
        (dict(struct_size=ctypes.sizeof(_capi.FaBwdVarlenArgs)), -4, "fa_bwd_varlen_qk_args.struct_size"),
        (dict(k_over=dict(struct_size=8)), -4, "fa_varlen_layout.struct_size"),
        # the layouts
        (dict(varlen=vl(n_seqs=0)), -4, "n_seqs"),
        (dict(k_over=dict(total_tokens=-5)), -4, "total_tokens"),
        (dict(k_over=dict(max_seqlen=0)), -4, "max_seqlen"),
        (dict(k_over=dict(n_seqs=4)), -4, "n_seqs mismatch"),
        # the 32-bit stride bound, both sides
        (dict(q_seq_stride=(1 << 23) + 8), -4, "too large"),
        (dict(kv_seq_stride=(1 << 23) + 8), -4, "too large"),
        (dict(varlen=vl(n_seqs=1 << 20), k_over=dict(n_seqs=1 << 20, max_seqlen=1 << 20)), -4, "too large"),
    ]
    for over, status, text in cases:
        rc = lib.fa_bwd_launch_varlen_qk(ctypes.byref(_bwd(**over)), None, None)
        msg = _capi.last_error()
        assert rc == status and text in msg, (over, rc, msg)
    assert lib.fa_bwd_launch_varlen_qk(ctypes.byref(_bwd(T=0, Tk=0)), None, None) == 0


def _isa(folder, unit):
    path = os.path.join(BUILD, folder, f"{unit}-hip-amdgcn-amd-amdhsa-gfx950.s")
    assert os.path.exists(path), "the build keeps the ISA of every slice under csrc/build (make -C flash_attention_from_scratch_amd/csrc)"
    return open(path).read()


def _no_scratch_no_spills(text):
    assert "scratch_" not in text
    assert re.search(r"private_segment_fixed_size:\s+[1-9]", text) is None
    assert re.search(r"\.(s|v)gpr_spill_count:\s+[1-9]", text) is None
    assert re.search(r"; ScratchSize: [1-9]", text) is None


def test_varlen_qk_slices_have_mfma_and_no_scratch():
    """the forward comes from the varlen slice, which serves both entry-point families; the backward has a slice of its own"""
    for dt, mfma in ((15, "v_mfma_f32_32x32x16_bf16"), (5, "v_mfma_f32_32x32x16_f16")):
        text = _isa(f"varlen_dt{dt}", "fa_inst_varlen")
        assert mfma in text and "ds_read_b64_tr_b16" in text and "global_load_lds_dwordx4" in text
        # the two forms (with and without the first-block skip) of the varlen kernel, and not the kernel it is built from
        assert len(re.findall(r"^_ZN2fa20fa_fwd_kernel_varlenI\w+:", text, flags=re.M)) == 2
        assert re.search(r"^_ZN2fa13fa_fwd_kernelI", text, flags=re.M) is None
        _no_scratch_no_spills(text)
    text = _isa("bwd_varlen_qk", "fa_bwd_varlen_qk")
    assert "v_mfma_f32_32x32x16_bf16" in text and "v_mfma_f32_32x32x16_f16" in text
    assert "ds_read_b64_tr_b16" in text
    _no_scratch_no_spills(text)
    # one text per kernel (fa_bwd_varlen.hpp): this slice holds the two-range forms (delta comes from the one-range slice)
    names = set(re.findall(r"^\s+\.name:\s+(_Z\w+)$", text, re.M))
    want = {f"_ZN2fa32fa_bwd_dkdv_reduce_varlen_kernelINS_15BwdVarlenQKArgsELi{dt}EEEvT_" for dt in (15, 5)}
    for kernel in ("25fa_bwd_dkdv_varlen_kernel", "23fa_bwd_dq_varlen_kernel"):
        want |= {f"_ZN2fa{kernel}INS_15BwdVarlenQKArgsELi{dt}ELb{c}EEEvT_" for dt in (15, 5) for c in (0, 1)}
    assert names == want, names ^ want
    for name in want:
        assert re.search(rf"^{name}:", text, flags=re.M), name
    assert "atomic" not in text   # no float atomics: a fixed order of sums


def test_python_wants_both_key_side_arguments_or_neither():
    q = torch.zeros((4, 2, 128), dtype=torch.bfloat16)
    cu = torch.tensor([0, 4], dtype=torch.int32)
    for fn, args in ((flash_attention.forward_varlen, (q, q, q, cu, 4)),
                     (flash_attention.attention_varlen, (q, q, q, cu, 4)),
                     (flash_attention.backward_varlen, (q, q, q, q, torch.zeros((2, 4)), q, cu, 4)),
                     (fak.forward_varlen, (q, q, q, cu, 4)),
                     (fak.backward_varlen, (q, q, q, q, torch.zeros((2, 4)), q, cu, 4))):
        with pytest.raises(ValueError, match="cu_seqlens_k and max_seqlen_k"):
            fn(*args, cu_seqlens_k=cu)
        with pytest.raises(ValueError, match="cu_seqlens_k and max_seqlen_k"):
            fn(*args, max_seqlen_k=4)
