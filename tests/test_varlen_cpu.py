"""Packed variable-length sequences without a device: the C ABI of fa_fwd_launch_varlen / fa_bwd_launch_varlen (struct layout,
exports, validation before any HIP call, the backward's workspace and split rule) and the ISA the build keeps for the new slices."""
import ctypes
import os
import re
import subprocess
import tempfile

from flash_attention_from_scratch_amd import _capi
from flash_attention_from_scratch_amd import flash_attention_kernels as fak
from flash_helpers import kernel_configs as kc
from tests.conftest import ROOT

import torch

BUILD = os.path.join(ROOT, "flash_attention_from_scratch_amd", "csrc", "build")
NEW_SYMBOLS = ("fa_fwd_varlen_supported", "fa_fwd_launch_varlen", "fa_bwd_varlen_workspace_bytes", "fa_bwd_launch_varlen")
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


def test_varlen_struct_mirrors_match_the_header():
    got, want = _layout(_capi.FaVarlenLayout, "fa_varlen_layout")
    assert got == want
    assert ctypes.sizeof(_capi.FaVarlenLayout) == 8 + 8 + 3 * 8   # (4 bytes of padding behind struct_size)
    got, want = _layout(_capi.FaBwdVarlenArgs, "fa_bwd_varlen_args")
    assert got == want
    assert ctypes.sizeof(_capi.FaBwdVarlenArgs) == 10 * 8 + 11 * 8 + 8 + ctypes.sizeof(_capi.FaVarlenLayout)


def test_varlen_symbols_abi_version_and_registry():
    assert set(NEW_SYMBOLS) <= set(_capi.EXPORTED_SYMBOLS)
    for path in (_capi.LIB_PATH, JITTER):
        nm = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True)
        exported = set(re.findall(r" T (fa_[a-z_0-9]+)", nm.stdout))
        assert set(NEW_SYMBOLS) <= exported, (path, set(NEW_SYMBOLS) - exported)
    lib = _capi.load()
    assert lib.fa_abi_version() == 6
    twin = ctypes.CDLL(JITTER)   # the varlen kernels are outside the registry: the count is the twin's
    twin.fa_num_kernels.restype = ctypes.c_int
    assert lib.fa_num_kernels() == twin.fa_num_kernels()


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


def test_fwd_varlen_supported():
    lib = _capi.load()
    for dtype in (torch.bfloat16, torch.float16):
        cfg = ctypes.byref(_capi.make_config(_cfg(dtype)))
        for causal in (False, True):
            assert lib.fa_fwd_varlen_supported(cfg, ctypes.byref(_capi.make_opts(causal=causal))) == 1
        assert lib.fa_fwd_varlen_supported(cfg, None) == 1
        assert lib.fa_fwd_varlen_supported(cfg, ctypes.byref(_capi.make_opts(speculative=True))) == 0
        assert lib.fa_fwd_varlen_supported(cfg, ctypes.byref(_capi.make_opts(prescaled_q=True))) == 0
        assert lib.fa_fwd_varlen_supported(cfg, ctypes.byref(_capi.make_opts(stats_ptr=16))) == 0
    # the persistent 64-rows-per-wave configuration (the dense training path's) has no varlen form
    best = ctypes.byref(_capi.make_config(kc.best_config(kc.DType.BF16)))
    assert lib.fa_fwd_varlen_supported(best, None) == 0


def test_fwd_launch_varlen_refusals_without_a_device():
    lib = _capi.load()
    lse = ctypes.c_void_p(16)

    def launch(args=None, kv=None, vl=None, opts=None, lse=lse, no_kv=False, no_vl=False):
        args, kv, vl = args or _fwd(), kv or _kv(), vl or _vl()
        opts = opts or _capi.make_opts()
        rc = lib.fa_fwd_launch_varlen(ctypes.byref(args), None if no_kv else ctypes.byref(kv), None if no_vl else ctypes.byref(vl),
                                      ctypes.byref(opts), lse, None)
        return rc, _capi.last_error()

    cases = [
        (dict(no_kv=True), -1, "null pointer"),
        (dict(no_vl=True), -1, "null pointer"),
        (dict(args=_fwd(q=None)), -1, "null pointer"),
        (dict(lse=None), -1, "lse is null"),
        (dict(vl=_vl(cu=None)), -1, "cu_seqlens is null"),
        (dict(vl=_vl(cu=18)), -5, "cu_seqlens must be 4-byte"),
        (dict(lse=ctypes.c_void_p(18)), -5, "lse must be 4-byte"),
        (dict(args=_fwd(k=24)), -5, "16-byte aligned"),
        (dict(vl=_vl(n_seqs=0)), -4, "n_seqs"),
        (dict(vl=_vl(T=-1)), -4, "total_tokens"),
        (dict(vl=_vl(max_seqlen=0)), -4, "max_seqlen"),
        (dict(vl=_vl(struct_size=4)), -4, "struct_size"),
        (dict(kv=_kv(struct_size=4)), -4, "struct_size"),
        (dict(kv=_kv(Hkv=3)), -4, "divide"),
        (dict(kv=_kv(Hkv=0)), -4, "divide"),
        (dict(kv=_kv(kv_seq_stride=2 * 128 + 4)), -5, "multiples of 8"),
        (dict(kv=_kv(kv_head_stride=-128)), -4, "positive"),
        (dict(kv=_kv(kv_seq_stride=(1 << 23) + 8)), -4, "too large"),
        (dict(args=_fwd(seq_stride=0)), -4, "positive"),
        (dict(args=_fwd(head_stride=132)), -5, "multiples of 8"),
        (dict(args=_fwd(d_head=64)), -4, "d_head"),
        (dict(args=_fwd(cfg=kc.best_config(kc.DType.BF16))), -3, "variable-length"),
        (dict(opts=_capi.make_opts(speculative=True)), -3, "variable-length"),
        (dict(opts=_capi.make_opts(prescaled_q=True)), -3, "variable-length"),
        (dict(opts=_capi.make_opts(stats_ptr=16)), -3, "variable-length"),
        (dict(vl=_vl(n_seqs=1 << 20, max_seqlen=1 << 20)), -4, "too large"),
    ]
    for over, status, text in cases:
        rc, msg = launch(**over)
        assert rc == status and text in msg, (over, rc, msg)
    bad = _fwd()
    bad.cfg.dtype = 7
    rc, msg = launch(args=bad)
    assert rc == -2 and "fp16 and bf16" in msg
    # total_tokens = 0: nothing to do, no device needed
    assert launch(vl=_vl(T=0))[0] == 0


def _bwd(n_seqs=3, T=1000, max_seqlen=512, H=8, Hkv=2, causal=0, **over):
    a = _capi.FaBwdVarlenArgs(q=16, k=16, v=16, o=16, dout=16, lse=ctypes.cast(ctypes.c_void_p(16), ctypes.POINTER(ctypes.c_float)),
                              dq=16, dk=16, dv=16, workspace=16, n_heads=H, n_kv_heads=Hkv, d_head=128,
                              q_seq_stride=H * 128, q_head_stride=128, out_seq_stride=H * 128, out_head_stride=128,
                              kv_seq_stride=Hkv * 128, kv_head_stride=128, dkv_seq_stride=Hkv * 128, dkv_head_stride=128,
                              dtype=15, causal=causal, varlen=_capi.make_varlen_layout(16, n_seqs, T, max_seqlen))
    for name, val in over.items():
        if hasattr(a.varlen, name):
            setattr(a.varlen, name, val)
        else:
            setattr(a, name, val)
    return a


def _split(**kw):
    """the dK / dV split the workspace size implies: delta (rounded up to 16 bytes) first, then the fp32 partials"""
    a = _bwd(**kw)
    T = a.varlen.total_tokens
    extra = _capi.load().fa_bwd_varlen_workspace_bytes(ctypes.byref(a)) - ((4 * a.n_heads * T + 15) & ~15)
    per = 4 * a.n_kv_heads * T * 2 * 128
    assert extra % per == 0
    return 1 if extra == 0 else extra // per


def test_bwd_varlen_workspace_and_split_rule():
    # workgroups per split part: n_seqs * n_kv_heads * ceil(max_seqlen / 128); the split is the smallest divisor of the group that
    # reaches 256 of them (1024 causal), else the whole group -- a function of the host's arguments, not of cu_seqlens
    assert _split(n_seqs=16, T=65536, max_seqlen=4096, H=16, Hkv=16) == 1          # MHA: nothing to split
    assert _split(n_seqs=16, T=65536, max_seqlen=4096, H=16, Hkv=4) == 1           # 2048 workgroups
    assert _split(n_seqs=4, T=16384, max_seqlen=4096, H=16, Hkv=1) == 2            # 128 -> 256
    assert _split(n_seqs=4, T=16384, max_seqlen=4096, H=16, Hkv=4, causal=1) == 2
    assert _split(n_seqs=4, T=16384, max_seqlen=4096, H=16, Hkv=1, causal=1) == 8
    assert _split(n_seqs=1, T=1000, max_seqlen=1000, H=8, Hkv=1) == 8              # 8 workgroups: the whole group
    assert _split(n_seqs=3, T=1792, max_seqlen=1024, H=8, Hkv=2) == 4              # 48 -> 192: the whole group
    assert _split(n_seqs=3, T=1792, max_seqlen=8192, H=8, Hkv=2) == 1              # a loose bound counts: 3 * 2 * 64 = 384
    # the same total_tokens and bounds with another number of sequences: another grid, possibly another split
    assert _split(n_seqs=1, T=4096, max_seqlen=4096, H=16, Hkv=4) == 2             # 128 -> 256
    lib = _capi.load()
    assert lib.fa_bwd_varlen_workspace_bytes(ctypes.byref(_bwd(T=1001, H=3, Hkv=3))) == (4 * 3 * 1001 + 15) // 16 * 16
    assert lib.fa_bwd_varlen_workspace_bytes(ctypes.byref(_bwd(Hkv=3))) == -4
    assert lib.fa_bwd_varlen_workspace_bytes(None) == -1


def test_bwd_varlen_refusals_without_a_device():
    lib = _capi.load()
    cases = [
        (dict(Hkv=3), -4, "divide"),
        (dict(kv_seq_stride=2 * 128 + 4), -5, "multiples of 8"),
        (dict(dkv_head_stride=4), -5, "multiples of 8"),
        (dict(dkv_seq_stride=-256), -4, "positive"),
        (dict(q_seq_stride=(1 << 23) + 8), -4, "too large"),
        (dict(out_seq_stride=0), -4, "positive"),
        (dict(lse=None), -1, "lse is null"),
        (dict(dk=None), -1, "null tensor pointer"),
        (dict(workspace=None), -1, "workspace is null"),
        (dict(workspace=20), -5, "workspace must be 16-byte"),
        (dict(q=24), -5, "16-byte aligned"),
        (dict(d_head=64), -4, "d_head = 128"),
        (dict(dtype=7), -2, "fp16 and bf16"),
        (dict(cu_seqlens=None), -1, "cu_seqlens is null"),
        (dict(cu_seqlens=18), -5, "cu_seqlens must be 4-byte"),
        (dict(n_seqs=0), -4, "n_seqs"),
        (dict(total_tokens=-5), -4, "total_tokens"),
        (dict(max_seqlen=0), -4, "max_seqlen"),
        (dict(struct_size=8), -4, "struct_size"),
        (dict(n_seqs=1 << 20, max_seqlen=1 << 20), -4, "too large"),
    ]
    for over, status, text in cases:
        rc = lib.fa_bwd_launch_varlen(ctypes.byref(_bwd(**over)), None, None)
        msg = _capi.last_error()
        assert rc == status and text in msg, (over, rc, msg)
    assert lib.fa_bwd_launch_varlen(ctypes.byref(_bwd(T=0)), None, None) == 0


def _isa(folder, unit):
    path = os.path.join(BUILD, folder, f"{unit}-hip-amdgcn-amd-amdhsa-gfx950.s")
    assert os.path.exists(path), "the build keeps the ISA of every slice under csrc/build (make -C flash_attention_from_scratch_amd/csrc)"
    return open(path).read()


def test_varlen_slices_have_mfma_and_no_scratch():
    for dt, mfma in ((15, "v_mfma_f32_32x32x16_bf16"), (5, "v_mfma_f32_32x32x16_f16")):
        text = _isa(f"varlen_dt{dt}", "fa_inst_varlen")
        assert mfma in text and "ds_read_b64_tr_b16" in text
        assert len(re.findall(r"^_ZN2fa20fa_fwd_kernel_varlen\w+:", text, flags=re.M)) == 2
        assert "scratch_" not in text
        assert re.search(r"private_segment_fixed_size:\s+[1-9]", text) is None
    text = _isa("bwd_varlen", "fa_bwd_varlen")
    assert "v_mfma_f32_32x32x16_bf16" in text and "v_mfma_f32_32x32x16_f16" in text
    assert "ds_read_b64_tr_b16" in text
    assert "scratch_" not in text
    assert re.search(r"private_segment_fixed_size:\s+[1-9]", text) is None
    # one text per kernel (fa_bwd_varlen.hpp): this slice holds the one-range forms, and none of the two-range ones
    names = set(re.findall(r"^\s+\.name:\s+(_Z\w+)$", text, re.M))
    want = {f"_ZN2fa26fa_bwd_delta_varlen_kernelILi{dt}EEEvNS_13BwdVarlenArgsE" for dt in (15, 5)}
    want |= {f"_ZN2fa32fa_bwd_dkdv_reduce_varlen_kernelINS_13BwdVarlenArgsELi{dt}EEEvT_" for dt in (15, 5)}
    for kernel in ("25fa_bwd_dkdv_varlen_kernel", "23fa_bwd_dq_varlen_kernel"):
        want |= {f"_ZN2fa{kernel}INS_13BwdVarlenArgsELi{dt}ELb{c}EEEvT_" for dt in (15, 5) for c in (0, 1)}
    assert names == want, names ^ want


def test_dense_training_entry_points_still_refuse_ragged_lengths():
    """the varlen path is additive: the dense LSE / backward launches keep their seq_len % 256 rule"""
    lib = _capi.load()
    base = _capi.FaBwdArgs(q=16, k=16, v=16, o=16, dout=16, lse=ctypes.cast(ctypes.c_void_p(16), ctypes.POINTER(ctypes.c_float)),
                           dq=16, dk=16, dv=16, workspace=16, batch=1, seq_len=1000, n_heads=8, d_head=128,
                           qkv_batch_stride=1000 * 1024, qkv_seq_stride=1024, qkv_head_stride=128,
                           out_batch_stride=1000 * 1024, out_seq_stride=1024, out_head_stride=128, dtype=15, causal=0)
    assert lib.fa_bwd_launch(ctypes.byref(base), None, None) == -4 and "seq_len % 256" in _capi.last_error()
