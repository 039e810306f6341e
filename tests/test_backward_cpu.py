"""The training path without a device: the C ABI of the forward with LSE and of the backward (struct layout, exports,
validation before any HIP call) and the ISA the build keeps for both."""
import ctypes
import dataclasses
import os
import re
import subprocess
import tempfile

from flash_attention_from_scratch_amd import _capi
from flash_helpers import kernel_configs as kc
from tests.conftest import ROOT

BUILD = os.path.join(ROOT, "flash_attention_from_scratch_amd", "csrc", "build")
NEW_SYMBOLS = ("fa_fwd_lse_supported", "fa_fwd_launch_lse", "fa_bwd_workspace_bytes", "fa_bwd_launch")


def test_bwd_args_mirror_matches_the_header():
    fields = [f[0] for f in _capi.FaBwdArgs._fields_]
    src = "#include <stdio.h>\n#include <stddef.h>\n#include \"fa_hip.h\"\nint main(void) {\n    printf(\"%zu\", sizeof(fa_bwd_args));\n"
    src += "".join(f"    printf(\" %zu\", offsetof(fa_bwd_args, {f}));\n" for f in fields)
    src += "    printf(\"\\n\");\n    return 0;\n}\n"
    with tempfile.TemporaryDirectory() as tmp:
        open(os.path.join(tmp, "t.c"), "w").write(src)
        subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), os.path.join(tmp, "t.c"), "-o", os.path.join(tmp, "t")], check=True)
        got = [int(x) for x in subprocess.run([os.path.join(tmp, "t")], capture_output=True, text=True, check=True).stdout.split()]
    want = [ctypes.sizeof(_capi.FaBwdArgs)] + [getattr(_capi.FaBwdArgs, f).offset for f in fields]
    assert got == want
    assert ctypes.sizeof(_capi.FaBwdArgs) == 10 * 8 + 10 * 8 + 2 * 4


def test_new_symbols_are_exported_by_both_libraries():
    assert set(NEW_SYMBOLS) <= set(_capi.EXPORTED_SYMBOLS)
    jitter = os.path.join(ROOT, "flash_attention_from_scratch_amd", "lib", "libfa_hip_jitter.so")
    for path in (_capi.LIB_PATH, jitter):
        nm = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True)
        exported = set(re.findall(r" T (fa_[a-z_0-9]+)", nm.stdout))
        assert set(NEW_SYMBOLS) <= exported, (path, set(NEW_SYMBOLS) - exported)


def _bwd_args(**over):
    B, S, H, D = 2, 1024, 3, 128
    a = _capi.FaBwdArgs(q=16, k=16, v=16, o=16, dout=16, lse=ctypes.cast(ctypes.c_void_p(16), ctypes.POINTER(ctypes.c_float)),
                        dq=16, dk=16, dv=16, workspace=16, batch=B, seq_len=S, n_heads=H, d_head=D,
                        qkv_batch_stride=S * H * D, qkv_seq_stride=H * D, qkv_head_stride=D,
                        out_batch_stride=S * H * D, out_seq_stride=H * D, out_head_stride=D, dtype=15, causal=0)
    for name, val in over.items():
        setattr(a, name, val)
    return a


def _launch(a):
    lib = _capi.load()
    rc = lib.fa_bwd_launch(ctypes.byref(a), None, None)
    return rc, _capi.last_error()


def test_bwd_validation_without_a_device():
    lib = _capi.load()
    assert lib.fa_bwd_workspace_bytes(ctypes.byref(_bwd_args())) == 4 * 2 * 3 * 1024
    cases = [
        (dict(d_head=64), -4, "d_head = 128"),
        (dict(seq_len=1000), -4, "seq_len % 256"),
        (dict(dtype=6), -2, "fp16 and bf16"),
        (dict(lse=None), -1, "lse is null"),
        (dict(workspace=None), -1, "workspace is null"),
        (dict(q=None), -1, "null tensor pointer"),
        (dict(qkv_seq_stride=3 * 128 + 4), -5, "multiples of 8"),
        (dict(out_head_stride=-128), -4, "positive"),
        (dict(qkv_seq_stride=(1 << 23) + 8), -4, "too large"),
        (dict(lse=ctypes.cast(ctypes.c_void_p(18), ctypes.POINTER(ctypes.c_float))), -5, "4-byte aligned"),
        (dict(workspace=17), -5, "4-byte aligned"),
        (dict(dq=24), -5, "16-byte aligned"),
    ]
    for over, status, text in cases:
        rc, msg = _launch(_bwd_args(**over))
        assert rc == status and text in msg, (over, rc, msg)
    assert lib.fa_bwd_workspace_bytes(ctypes.byref(_bwd_args(d_head=64))) == -4
    assert lib.fa_bwd_workspace_bytes(None) == -1


def _persistent(dtype):
    return kc.best_config(dtype)


def test_fwd_lse_supported_matrix():
    lib = _capi.load()
    for dtype in (kc.DType.BF16, kc.DType.FP16):
        cfg = _persistent(dtype)
        for causal in (False, True):
            for spec in (False, True, "adaptive"):
                for ragged in (False, True):
                    o = _capi.make_opts(causal=causal, speculative=spec, allow_ragged=ragged)
                    assert lib.fa_fwd_lse_supported(ctypes.byref(_capi.make_config(cfg)), ctypes.byref(o)) == 1, (dtype, causal, spec)
        psq = dataclasses.replace(cfg, prescaled_q=True)
        o = _capi.make_opts(speculative=True, prescaled_q=True)
        assert lib.fa_fwd_lse_supported(ctypes.byref(_capi.make_config(psq)), ctypes.byref(o)) == 0
        # the 32-rows-per-wave configurations, among them (128, 64, 4) + buffer, whose long launches take the ring form
        others = [c for c in kc.get_all_supported_configs() if c.dtype == dtype and c.d_head == 128 and c.B_r // c.n_warps != 64]
        assert any(c.B_r == 128 and c.B_c == 64 and c.n_warps == 4 and c.mma_double_buffer_loads for c in others)
        for c in others:
            for spec in (False, True):
                o = _capi.make_opts(speculative=spec)
                assert lib.fa_fwd_lse_supported(ctypes.byref(_capi.make_config(c)), ctypes.byref(o)) == 0, c


def test_fwd_launch_lse_validation_without_a_device():
    lib = _capi.load()
    B, S, H = 1, 1024, 2
    cfg = _capi.make_config(_persistent(kc.DType.BF16))
    def args(seq_stride=H * 128, seq_len=S):
        return _capi.FaFwdArgs(q=16, k=16, v=16, o=16, batch=B, seq_len=seq_len, n_heads=H, d_head=128,
                               batch_stride=seq_len * seq_stride, seq_stride=seq_stride, head_stride=128, cfg=cfg)
    o = _capi.make_opts(speculative=True)
    lse = ctypes.c_void_p(16)
    assert lib.fa_fwd_launch_lse(ctypes.byref(args(seq_stride=136 * H)), ctypes.byref(o), lse, None) == -4
    assert "seq_stride % 128" in _capi.last_error()
    assert lib.fa_fwd_launch_lse(ctypes.byref(args(seq_len=1000)), ctypes.byref(_capi.make_opts(allow_ragged=True)), lse, None) == -4
    assert "seq_len % 256" in _capi.last_error()
    assert lib.fa_fwd_launch_lse(ctypes.byref(args()), ctypes.byref(o), None, None) == -1
    assert "lse is null" in _capi.last_error()
    psq = _capi.make_config(dataclasses.replace(_persistent(kc.DType.BF16), prescaled_q=True))
    a = args()
    a.cfg = psq
    assert lib.fa_fwd_launch_lse(ctypes.byref(a), ctypes.byref(_capi.make_opts(speculative=True, prescaled_q=True)), lse, None) == -3
    assert "log-sum-exp" in _capi.last_error()


def _isa(slice_dir, stem):
    path = os.path.join(BUILD, slice_dir, f"{stem}-hip-amdgcn-amd-amdhsa-gfx950.s")
    assert os.path.exists(path), "the build keeps the ISA of every slice under csrc/build (make -C flash_attention_from_scratch_amd/csrc)"
    return open(path).read()


def test_lse_forms_keep_the_visits_of_their_siblings():
    """The hot loop did not move: the visit histograms of the LSE forms' plain variants are those the committed digest
    (profiles/r06/toolchain.json) records for their non-LSE siblings.  The speculative forms match block for block.  In the
    lazy forms exactly one visit block differs: a general visit (64 MFMAs: the first group of an item, outside the hot loop)
    carries two more SGPR spill reloads (v_readlane_b32, +2 instructions) -- the register pressure of the epilogue's lse
    address -- and every other count of that block, and every other block, is the digest's."""
    import json

    from flash_attention_from_scratch_amd.tools import isa_digest

    ref = json.load(open(os.path.join(ROOT, "profiles", "r06", "toolchain.json")))["kernels"]
    names = {15: (("bf16 speculative (default)", "ILi15ELb0ELb1ELi0ELb0ELb0ELi2ELb0ELi4E"), ("bf16 lazy", "ILi15ELb0ELb0ELi0ELb0ELb0ELi2ELb0ELi4E")),
             5: (("fp16 speculative", "ILi5ELb0ELb1ELi0ELb0ELb0ELi2ELb0ELi4E"), ("fp16 lazy (default)", "ILi5ELb0ELb0ELi0ELb0ELb0ELi2ELb0ELi4E"))}
    for dt, pairs in names.items():
        text = _isa(f"lse_dt{dt}", "fa_inst_lse")
        for name, targs in pairs:
            got = isa_digest.visits_of(text, targs, prefix="_ZN2fa19fa_fwd_kernel64_lse", suffix="EEvNS_13KernelArgsLseE")
            want = ref[name]
            assert got is not None and len(got) == len(want), name
            if "speculative" in name:
                assert got == want, name
                continue
            differ = [(g, w) for g, w in zip(got, want) if g != w]
            assert len(differ) <= 1, (name, differ)
            for g, w in differ:
                assert g["mfma"] == 64, (name, g)   # a single (general) visit, not the merged hot block
                assert {**w, "v_readlane_b32": w["v_readlane_b32"] + 2, "instructions": w["instructions"] + 2} == g, (name, g, w)


def test_backward_slice_has_mfma_and_no_scratch():
    text = _isa("bwd", "fa_bwd")
    assert "v_mfma_f32_32x32x16_bf16" in text and "v_mfma_f32_32x32x16_f16" in text
    assert "ds_read_b64_tr_b16" in text
    assert "scratch_" not in text
    assert re.search(r"private_segment_fixed_size:\s+[1-9]", text) is None
    for kernel in ("fa_bwd_dkdv_kernel", "fa_bwd_dq_kernel", "fa_bwd_delta_kernel"):
        assert kernel in text, kernel
