"""GPU tier: which autograd nodes and launches every model of fitgnn_amd.network runs, and the bits they give, against the record in
tests/golden/model_dispatch.json (tests/golden/make_model_dispatch_golden.py; cases and record: tests/model_dispatch_cases.py).
A change that is not meant to move a model onto other nodes, launches or bits leaves every record as it is."""
import json
import os

import pytest

from model_dispatch_cases import CASES, MODES, key, record

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def golden(golden_dir):
    with open(os.path.join(golden_dir, "model_dispatch.json")) as f:
        return json.load(f)


@pytest.mark.parametrize("name", sorted(CASES))
def test_model_runs_the_recorded_nodes_launches_and_bits(golden, name):
    for mode in MODES:
        want = golden["records"][key(name, mode)]
        got = record(name, mode)
        assert got["nodes"] == want["nodes"], mode
        assert got["kinds"] == want["kinds"], mode
        assert got["gemms"] == want["gemms"], mode
        for field in ("out", "grads"):   # (absent from a record whose bits did not reproduce when it was made)
            if field in want:
                assert got[field] == want[field], (mode, field)


def test_the_fixture_holds_exactly_the_parametrised_cases(golden):
    assert sorted(golden["records"]) == sorted(key(n, m) for n in CASES for m in MODES)
