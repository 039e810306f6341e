"""Grouped-query attention without a device: the C ABI of fa_fwd_launch_gqa / fa_bwd_launch_gqa (struct layout, exports,
validation before any HIP call, the backward's workspace and split) and the ISA the build keeps for the GQA forward forms."""
import ctypes
import dataclasses
import json
import os
import re
import subprocess
import sys
import tempfile

from flash_attention_from_scratch_amd import _capi
from flash_helpers import kernel_configs as kc
from tests.conftest import ROOT

BUILD = os.path.join(ROOT, "flash_attention_from_scratch_amd", "csrc", "build")
NEW_SYMBOLS = ("fa_fwd_gqa_supported", "fa_fwd_launch_gqa", "fa_bwd_gqa_workspace_bytes", "fa_bwd_launch_gqa")


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


def test_gqa_struct_mirrors_match_the_header():
    got, want = _layout(_capi.FaKvLayout, "fa_kv_layout")
    assert got == want
    assert ctypes.sizeof(_capi.FaKvLayout) == 8 + 4 * 8   # (4 bytes of padding behind struct_size)
    got, want = _layout(_capi.FaBwdGqaArgs, "fa_bwd_gqa_args")
    assert got == want
    assert ctypes.sizeof(_capi.FaBwdGqaArgs) == ctypes.sizeof(_capi.FaBwdArgs) + 7 * 8


def test_gqa_symbols_are_exported_by_both_libraries():
    assert set(NEW_SYMBOLS) <= set(_capi.EXPORTED_SYMBOLS)
    jitter = os.path.join(ROOT, "flash_attention_from_scratch_amd", "lib", "libfa_hip_jitter.so")
    for path in (_capi.LIB_PATH, jitter):
        nm = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True)
        exported = set(re.findall(r" T (fa_[a-z_0-9]+)", nm.stdout))
        assert set(NEW_SYMBOLS) <= exported, (path, set(NEW_SYMBOLS) - exported)


def _fwd(cfg, B=2, S=1024, H=8, seq_len=None):
    S = seq_len or S
    return _capi.FaFwdArgs(q=16, k=16, v=16, o=16, batch=B, seq_len=S, n_heads=H, d_head=128,
                           batch_stride=S * H * 128, seq_stride=H * 128, head_stride=128, cfg=_capi.make_config(cfg))


def _kv(Hkv=2, S=1024, **over):
    kv = _capi.make_kv_layout(Hkv, S * Hkv * 128, Hkv * 128, 128)
    for name, val in over.items():
        setattr(kv, name, val)
    return kv


def test_fwd_gqa_supported_is_the_lse_forms():
    lib = _capi.load()
    for c in kc.get_all_supported_configs():
        for causal in (False, True):
            for spec in (False, True):
                o = _capi.make_opts(causal=causal, speculative=spec)
                cfg = ctypes.byref(_capi.make_config(c))
                assert lib.fa_fwd_gqa_supported(cfg, ctypes.byref(o)) == lib.fa_fwd_lse_supported(cfg, ctypes.byref(o)), c
    assert lib.fa_fwd_gqa_supported(ctypes.byref(_capi.make_config(kc.best_config(kc.DType.BF16))),
                                    ctypes.byref(_capi.make_opts(speculative=True))) == 1


def test_fwd_launch_gqa_refusals_without_a_device():
    lib = _capi.load()
    cfg = kc.best_config(kc.DType.BF16)
    spec = _capi.make_opts(speculative=True)
    lse = ctypes.c_void_p(16)

    def launch(args, kv, opts=spec, lse=lse):
        rc = lib.fa_fwd_launch_gqa(ctypes.byref(args), ctypes.byref(kv) if kv is not None else None, ctypes.byref(opts), lse, None)
        return rc, _capi.last_error()

    cases = [
        (dict(kv=_kv(Hkv=3)), -4, "divide"),
        (dict(kv=_kv(Hkv=0)), -4, "divide"),
        (dict(lse=None), -1, "lse is null"),
        (dict(kv=None), -1, "null pointer"),
        (dict(kv=_kv(kv_seq_stride=2 * 128 + 4)), -5, "multiples of 8"),
        (dict(kv=_kv(kv_head_stride=-128)), -4, "positive"),
        (dict(kv=_kv(kv_seq_stride=(1 << 23) + 8)), -4, "too large"),
        (dict(kv=_kv(struct_size=4)), -4, "struct_size"),
        (dict(args=_fwd(cfg, seq_len=1000), opts=_capi.make_opts(allow_ragged=True, speculative=True)), -4, "seq_len % 256"),
    ]
    for over, status, text in cases:
        kw = dict(args=_fwd(cfg), kv=_kv())
        kw.update(over)
        rc, msg = launch(**kw)
        assert rc == status and text in msg, (over, rc, msg)
    # (a K / V seq stride that is not a multiple of 128 -- padded rows -- is accepted: tests/test_gqa_gpu.py runs one)
    psq = dataclasses.replace(cfg, prescaled_q=True)
    rc, msg = launch(_fwd(psq), _kv(), opts=_capi.make_opts(speculative=True, prescaled_q=True))
    assert rc == -3 and "grouped-query" in msg, (rc, msg)
    ring = [c for c in kc.get_all_supported_configs() if c.dtype == kc.DType.BF16 and c.d_head == 128 and c.B_r == 128
            and c.B_c == 64 and c.n_warps == 4 and c.mma_double_buffer_loads][0]
    rc, msg = launch(_fwd(ring), _kv(), opts=_capi.make_opts())
    assert rc == -3 and "grouped-query" in msg, (rc, msg)


def _bwd(B=2, S=1024, H=8, Hkv=2, causal=0, **over):
    base = _capi.FaBwdArgs(q=16, k=16, v=16, o=16, dout=16, lse=ctypes.cast(ctypes.c_void_p(16), ctypes.POINTER(ctypes.c_float)),
                           dq=16, dk=16, dv=16, workspace=16, batch=B, seq_len=S, n_heads=H, d_head=128,
                           qkv_batch_stride=S * H * 128, qkv_seq_stride=H * 128, qkv_head_stride=128,
                           out_batch_stride=S * H * 128, out_seq_stride=H * 128, out_head_stride=128, dtype=15, causal=causal)
    a = _capi.FaBwdGqaArgs(base=base, n_kv_heads=Hkv, kv_batch_stride=S * Hkv * 128, kv_seq_stride=Hkv * 128, kv_head_stride=128,
                           dkv_batch_stride=S * Hkv * 128, dkv_seq_stride=Hkv * 128, dkv_head_stride=128)
    for name, val in over.items():
        if hasattr(a.base, name) and name not in ("n_kv_heads",) and not name.startswith(("kv_", "dkv_")):
            setattr(a.base, name, val)
        else:
            setattr(a, name, val)
    return a


def _split(**kw):
    """the dK / dV split the workspace size implies (delta first, then the fp32 partials)"""
    lib = _capi.load()
    a = _bwd(**kw)
    b = a.base
    extra = lib.fa_bwd_gqa_workspace_bytes(ctypes.byref(a)) - 4 * b.batch * b.n_heads * b.seq_len
    per = 4 * b.batch * a.n_kv_heads * b.seq_len * 2 * 128
    return 1 if extra == 0 else extra // per


def test_bwd_gqa_workspace_and_split():
    # the grid is batch * n_kv_heads * seq_len / 128 workgroups per split part; the split is the smallest divisor of the group
    # that reaches 256 workgroups (1024 causal), else the whole group
    assert _split(B=4, S=4096, H=16, Hkv=4) == 1     # 512 workgroups
    assert _split(B=4, S=4096, H=16, Hkv=2) == 1     # 256
    assert _split(B=4, S=4096, H=16, Hkv=1) == 2     # MQA: 128 -> 256
    assert _split(B=4, S=4096, H=16, Hkv=4, causal=1) == 2
    assert _split(B=4, S=4096, H=16, Hkv=1, causal=1) == 8
    assert _split(B=1, S=1024, H=8, Hkv=1) == 8      # 8 workgroups: the whole group
    assert _split(B=2, S=1024, H=8, Hkv=8) == 1      # group 1: nothing to split


def test_bwd_gqa_refusals_without_a_device():
    lib = _capi.load()
    cases = [
        (dict(Hkv=3), -4, "divide"),
        (dict(kv_seq_stride=2 * 128 + 4), -5, "multiples of 8"),
        (dict(dkv_head_stride=4), -5, "multiples of 8"),
        (dict(dkv_seq_stride=-256), -4, "positive"),
        (dict(seq_len=1000), -4, "seq_len % 256"),
        (dict(lse=None), -1, "lse is null"),
        (dict(dk=None), -1, "null tensor pointer"),
        (dict(d_head=64), -4, "d_head = 128"),
    ]
    for over, status, text in cases:
        rc = lib.fa_bwd_launch_gqa(ctypes.byref(_bwd(**over)), None, None)
        msg = _capi.last_error()
        assert rc == status and text in msg, (over, rc, msg)
    # the split needs a 16-byte aligned workspace (its fp32 partials); without a split 4 bytes do
    rc = lib.fa_bwd_launch_gqa(ctypes.byref(_bwd(B=1, S=1024, H=8, Hkv=1, workspace=20)), None, None)
    assert rc == -5 and "16-byte" in _capi.last_error()
    assert lib.fa_bwd_gqa_workspace_bytes(ctypes.byref(_bwd(Hkv=3))) == -4
    assert lib.fa_bwd_gqa_workspace_bytes(None) == -1


def _isa(dt):
    path = os.path.join(BUILD, f"gqa_dt{dt}", "fa_inst_gqa-hip-amdgcn-amd-amdhsa-gfx950.s")
    assert os.path.exists(path), "the build keeps the ISA of every slice under csrc/build (make -C flash_attention_from_scratch_amd/csrc)"
    return path, open(path).read()


def test_gqa_slices_have_no_scratch_and_pass_the_lint():
    lint = os.path.join(ROOT, "flash_attention_from_scratch_amd", "tools", "isa_lint64.py")
    for dt in (15, 5):
        path, text = _isa(dt)
        assert len(re.findall(r"^_ZN2fa19fa_fwd_kernel64_gqa\w+:", text, flags=re.M)) == 4
        assert "scratch_" not in text
        assert re.search(r"private_segment_fixed_size:\s+[1-9]", text) is None
        assert re.search(r"\.vgpr_spill_count:\s+[1-9]", text) is None
        for opts in (["--window", "4", "--raw", "3", "--only", "fa_fwd_kernel64"], ["--window", "0", "--raw", "0"]):
            r = subprocess.run([sys.executable, lint, path] + opts, capture_output=True, text=True)
            assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]


def test_gqa_forms_keep_the_visits_of_their_siblings():
    """The hot loop did not move: the visit histograms of the GQA forms' plain variants against the committed digest
    (profiles/r06/toolchain.json).  The speculative forms match block for block.  In the lazy forms exactly two general
    visits (64 MFMAs each, outside the merged hot block) differ: the first carries four SGPR spill reloads where the digest
    has two (the LSE form's pinned +2, plus 2: v_readlane_b32 +2) and three more instructions in all; the second one
    instruction fewer.  Every other count of those blocks, and every other block, is the digest's."""
    from flash_attention_from_scratch_amd.tools import isa_digest

    ref = json.load(open(os.path.join(ROOT, "profiles", "r06", "toolchain.json")))["kernels"]
    names = {15: (("bf16 speculative (default)", "ILi15ELb0ELb1ELi0ELb0ELb0ELi2ELb0ELi4E"), ("bf16 lazy", "ILi15ELb0ELb0ELi0ELb0ELb0ELi2ELb0ELi4E")),
             5: (("fp16 speculative", "ILi5ELb0ELb1ELi0ELb0ELb0ELi2ELb0ELi4E"), ("fp16 lazy (default)", "ILi5ELb0ELb0ELi0ELb0ELb0ELi2ELb0ELi4E"))}
    for dt, pairs in names.items():
        _, text = _isa(dt)
        for name, targs in pairs:
            got = isa_digest.visits_of(text, targs, prefix="_ZN2fa19fa_fwd_kernel64_gqa", suffix="EEvNS_13KernelArgsGqaE")
            want = ref[name]
            assert got is not None and len(got) == len(want), name
            if "speculative" in name:
                assert got == want, name
                continue
            differ = [(i, g, w) for i, (g, w) in enumerate(zip(got, want)) if g != w]
            assert len(differ) == 2, (name, differ)
            (_, g1, w1), (_, g2, w2) = differ
            assert g1["mfma"] == 64 and g2["mfma"] == 64, name
            assert {**w1, "v_readlane_b32": w1["v_readlane_b32"] + 2, "instructions": w1["instructions"] + 3} == g1, (name, g1, w1)
            assert {**w2, "instructions": w2["instructions"] - 1} == g2, (name, g2, w2)
