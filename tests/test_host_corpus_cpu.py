"""The host layer of the KV-cache entry points against its recorded behaviour (tests/host_corpus.py; tests/golden/host_corpus.json,
recorded from a build of the commit the file names): every case's return value, message and returned ms, all of them, so that the
order of the library's checks cannot move unnoticed.  The corpus runs in a child process that sees no device: its passing cases
end in the "no HIP device" status there and would launch with fake pointers anywhere else."""
import json
import os
import subprocess
import sys

import pytest

from tests import host_corpus as hc
from tests.conftest import ROOT


@pytest.fixture(scope="module")
def recorded():
    with open(hc.GOLDEN) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def current():
    env = dict(os.environ, **hc.HIDE_DEVICES)
    run = subprocess.run([sys.executable, "-m", "tests.host_corpus", "--dump"], cwd=ROOT, env=env, capture_output=True, text=True)
    assert run.returncode == 0, run.stderr[-2000:]
    return json.loads(run.stdout)


def test_the_case_count_is_the_recorded_one(recorded, current):
    assert current["n_cases"] == recorded["n_cases"] == sum(c["n"] for c in recorded["cases"].values())
    assert {n: c["n"] for n, c in current["cases"].items()} == {n: c["n"] for n, c in recorded["cases"].items()}
    assert len(recorded["cases"]) == 16 + 3 and len(recorded["parent"]) == 40
    assert recorded["n_cases"] == sum(1 for _ in hc.cases())


def test_every_base_set_passes_every_rule_unmutated(recorded, current):
    for golden in (recorded, current):
        assert len(golden["unmutated"]) == 4 * (2 + 4 + 10 + 12) + 18 + 4 + 4
        for key, (rc, message) in golden["unmutated"].items():
            if "_launch" in key:
                assert (rc, message) == hc.NO_DEVICE, key
            elif "_supported" in key:
                assert rc == 1, key
            elif "_num_splits" in key:
                assert 1 <= rc <= 128, key
            else:
                assert rc >= 0 and "_workspace_bytes" in key, key


def test_every_case_gives_the_recorded_status_message_and_ms(recorded, current):
    want, got = hc.unpack(recorded), hc.unpack(current)
    assert list(want) == list(got)
    wrong = []
    labels = hc.cases()
    for name in want:
        for w, g in zip(want[name], got[name]):
            entry, base, _, _, _, case = next(labels)
            assert entry == name
            if w != g and len(wrong) < 20:
                wrong.append(f"{name}[{base}] {hc.describe(case)}: recorded {w}, now {g}")
    assert not wrong, "\n".join(wrong)
    # the records are not a handful of early refusals: each status occurs, and the timed empty launches
    statuses = {r[0] for r in recorded["records"]}
    assert {-1, -2, -3, -4, -5, -7, 0, 1} <= statuses
    assert any(r[0] == 0 and r[2] == 0.0 for r in recorded["records"])
