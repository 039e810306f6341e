#!/usr/bin/env python3
"""Pin of kernels that one text instantiates in several forms: per kernel of a kept ISA file (csrc/build/<slice>/*.s) a
SHA-256 of its normalised body -- one instruction or label per line; comments, directives and blank lines dropped; the
function's number taken out of its .LBB<n>_<m> labels -- and a SHA-256 of its .amdhsa_* kernel-descriptor block.  An entry is
keyed by (slice, kernel family, argument form, template arguments) and not by the mangled name, so a fold that moves the form
from the kernel's name into a template argument keeps its keys: fa_decode_fp8_split_kernel<15, 1, false>(DecodeFp8Args) and
fa_decode_split_kernel<DecodeFp8Args, 15, 1, false> are both "decode_fp8/fa_decode_split_kernel/DecodeFp8Args/15,1,0".

    isa_bodies.py [--write tests/golden/folded_kernel_bodies.json]

tests/test_tools_cpu.py::test_folded_kernels_keep_their_recorded_bodies holds a build to the committed record (taken from the
last commit that kept two texts per family), under the hipcc that record names."""
import argparse
import hashlib
import json
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from flash_attention_from_scratch_amd.tools import isa_digest  # noqa: E402

# slice directory under csrc/build -> the translation unit whose ISA it keeps
SLICES = {"decode": "fa_decode", "decode_fp8": "fa_decode_fp8", "bwd_varlen": "fa_bwd_varlen", "bwd_varlen_qk": "fa_bwd_varlen_qk"}


def kernels(text):
    """{mangled name: (body text, descriptor text)} of a kept .s (the splitting of the tests' _kernels)"""
    out = {}
    for m in re.finditer(r"^(_Z\w+):(.*?)\n\s*\.amdhsa_kernel \1\n(.*?)\n\s*\.end_amdhsa_kernel", text, re.M | re.S):
        out[m.group(1)] = (m.group(2), m.group(3))
    return out


def key_of(slice_dir, name):
    m = re.match(r"_ZN2fa\d+(fa_\w+?_kernel)I(.*)EEv", name)
    family = re.sub(r"_(fp8|qk)(?=_)", "", m.group(1))   # (before the fold the kernel's name carried the form)
    form = re.search(r"NS_\d+(\w+?Args)E", name).group(1)
    targs = ",".join(re.findall(r"L[ib](\d+)E", m.group(2)))
    return f"{slice_dir}/{family}/{form}/{targs}"


def normalised(body):
    lines = []
    for line in body.split("\n"):
        s = line.split(";")[0].strip()
        if re.match(r"\.LBB\d+_\d+:", s) or (s and not s.startswith(".")):
            lines.append(re.sub(r"\.LBB\d+_", ".LBB_", " ".join(s.split())))
    return "\n".join(lines)


def sha(text):
    return hashlib.sha256(text.encode()).hexdigest()


def bodies(build=isa_digest.BUILD):
    """-> {"hipcc": version, "kernels": {key: {"body": sha256, "descriptor": sha256}}}, or None without a kept ISA file"""
    out = {"hipcc": isa_digest.hipcc_version(), "kernels": {}}
    for slice_dir, unit in SLICES.items():
        path = os.path.join(build, slice_dir, f"{unit}-hip-amdgcn-amd-amdhsa-gfx950.s")
        if not os.path.exists(path):
            return None
        for name, (body, desc) in kernels(open(path).read()).items():
            key = key_of(slice_dir, name)
            assert key not in out["kernels"], key
            out["kernels"][key] = {"body": sha(normalised(body)), "descriptor": sha(normalised(desc.replace(".amdhsa_", "amdhsa_")))}
    return out


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--build", default=isa_digest.BUILD, help="the build directory that holds the slices (default: csrc/build)")
    ap.add_argument("--write", default="", help="write the record to this JSON file")
    args = ap.parse_args(argv)
    d = bodies(args.build)
    if d is None:
        print("no kept ISA under csrc/build: run make -C flash_attention_from_scratch_amd/csrc first")
        return 1
    text = json.dumps(d, indent=1, sort_keys=True)
    if args.write:
        with open(args.write, "w") as f:
            f.write(text + "\n")
    print(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
