"""The Python wrapper's refusals on the KV-cache paths with real device tensors (the cases: tests/test_wrapper_refusals_cpu.py;
the record: tests/golden/wrapper_refusals.json): wrong dtype, dim, shape, device or contiguity, mismatched k / v strides, a
misaligned view, descales against the cache's type, the block table's shape, a max_seqlen_k that is no int -- and, per function and
cache kind, calls that go through, whose results must have the recorded bits (the structure the wrapper fills reached the
library unchanged).  A refusal launches nothing; the tensors are tiny.

    python -m tests.test_wrapper_refusals_gpu     # this tier's records as JSON
"""
import json
import sys

import pytest
import torch

from tests.test_wrapper_refusals_cpu import FUNCTIONS, RECORDED, collect

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def recorded():
    with open(RECORDED) as f:
        g = json.load(f)
    return dict(g, cpu={k: g["records"][i] for k, i in g["cpu"].items()}, gpu={k: g["records"][i] for k, i in g["gpu"].items()})


@pytest.fixture(scope="module")
def got():
    out = collect("gpu", "cuda:0")
    torch.cuda.synchronize()
    return out


def test_gpu_tier_every_case_as_recorded(recorded, got):
    assert len(got) == recorded["n_gpu"] == len(recorded["gpu"])
    wrong = [f"{cid}: recorded {recorded['gpu'].get(cid)}, now {rec}" for cid, rec in got.items() if recorded["gpu"].get(cid) != rec]
    assert not wrong, "\n".join(wrong[:20])


def test_gpu_tier_valid_calls_went_through_and_refusals_vary(recorded, got):
    for fn in FUNCTIONS:
        for kind in ("contig,16bit", "paged,16bit", "contig,fp8", "paged,fp8"):
            assert got[f"{fn}[{kind}] valid"][0] == "ok" == recorded["gpu"][f"{fn}[{kind}] valid"][0], (fn, kind)
        refusals = {tuple(rec) for cid, rec in got.items() if cid.startswith(fn + "[") and rec[0] not in ("ok", "n/a")}
        assert len(refusals) >= 15, (fn, len(refusals))


if __name__ == "__main__":
    json.dump(collect("gpu", "cuda:0"), sys.stdout, indent=0)
