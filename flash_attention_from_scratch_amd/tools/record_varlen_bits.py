"""Records the bits of the equal-length varlen path: SHA-256 of the raw bytes of o, lse, dq, dk, dv from forward_varlen /
backward_varlen called WITHOUT the key side, for every (dtype, causal, heads, length set) of
tests/test_varlen_qk_gpu.py::test_varlen_qk_with_equal_sides_is_the_varlen_path_bit_for_bit, on that test's inputs (its own
builder and seed, imported).  tests/test_varlen_gpu.py::test_varlen_reproduces_the_recorded_bits holds both spellings of the
call (with and without cu_seqlens_k) to the recording.

The bits belong to one compiler: the file carries the `hipcc --version` string, and is regenerated on the MI355X whenever
profiles/r06/toolchain.json is.  Public Python API only.

    python flash_attention_from_scratch_amd/tools/record_varlen_bits.py [--out tests/golden/varlen_equal_sides_bits.json]
"""
import argparse
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402

import flash_attention  # noqa: E402

SEED = 3   # the seed of the test named above
NAMES = ("o", "lse", "dq", "dk", "dv")


def case_id(dtype, causal, heads, name):
    return f"{str(dtype).replace('torch.', '')}-{'causal' if causal else 'plain'}-{heads[0]}x{heads[1]}-{name}"


def sha256_of(x):
    """SHA-256 of a tensor's raw bytes, in its logical (row-major) order"""
    return hashlib.sha256(x.detach().contiguous().cpu().view(torch.uint8).numpy().tobytes()).hexdigest()


def record():
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import test_varlen_qk_gpu as t   # the test module: DTYPES, HEADS, LENGTH_SETS, _inputs, _cu
    from flash_attention_from_scratch_amd.tools.isa_digest import hipcc_version

    cases = {}
    for dtype in t.DTYPES:
        for causal in (False, True):
            for heads in t.HEADS:
                for name, (lengths, max_seqlen) in t.LENGTH_SETS.items():
                    max_seqlen = max_seqlen or max(lengths)
                    q, k, v, dout = t._inputs([(n, n) for n in lengths], heads[0], heads[1], dtype, seed=SEED)
                    cu, _ = t._cu(lengths)
                    o, lse = flash_attention.forward_varlen(q, k, v, cu, max_seqlen, causal=causal)
                    grads = flash_attention.backward_varlen(q, k, v, o, lse, dout, cu, max_seqlen, causal=causal)
                    torch.cuda.synchronize()
                    cases[case_id(dtype, causal, heads, name)] = {nm: sha256_of(x) for nm, x in zip(NAMES, (o, lse) + tuple(grads))}
    return {
        "what": "SHA-256 of the raw bits of o, lse, dq, dk, dv of forward_varlen / backward_varlen without cu_seqlens_k, on the "
                "inputs of tests/test_varlen_qk_gpu.py::test_varlen_qk_with_equal_sides_is_the_varlen_path_bit_for_bit",
        "regenerate": "with tools/record_varlen_bits.py on the MI355X, whenever profiles/r06/toolchain.json is regenerated",
        "hipcc": hipcc_version(),
        "seed": SEED,
        "cases": cases,
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "varlen_equal_sides_bits.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "record_varlen_bits.py needs the GPU"
    rec = record()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"{len(rec['cases'])} cases -> {a.out}")


if __name__ == "__main__":
    main()
