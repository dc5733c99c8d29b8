"""`generate()` / `generate_inflight()` / `score()` issue the engine calls they issued before: every call the product class makes on a
(recorded) CPU oracle engine, with a summary of its arguments, and what the entry point returns, against
tests/golden/generate_engine_calls.json — written by tests/golden/make_generate_engine_calls.py on the commit BEFORE the host code was
refactored.  The engine calls decide the GPU launches; what this cannot see is device work outside the engine (`n_valid.clone()`, the D2H
synchronisations)."""
import json
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))

import make_generate_engine_calls as M  # noqa: E402

GOLD = json.load(open(os.path.join(HERE, "golden", "generate_engine_calls.json")))
# floats of a result (log-probabilities, logits, beam scores: O(1..10) in fp32 on the CPU; the recorded ones are rounded to 1e-6): the code
# on both sides runs the same oracle calls in the same order, so only the BLAS of the machine can differ — tests/test_score.py's PER_TOKEN
ATOL = 1e-4


def same(got, want, where):
    if isinstance(want, float) or isinstance(got, float):
        assert got is not None and want is not None and abs(got - want) <= ATOL, (where, got, want)
    elif isinstance(want, list):
        assert isinstance(got, list) and len(got) == len(want), (where, got, want)
        for i, (g, w) in enumerate(zip(got, want)):
            same(g, w, f"{where}[{i}]")
    elif isinstance(want, dict):
        assert isinstance(got, dict) and sorted(got) == sorted(want), (where, got, want)
        for k in want:
            same(got[k], want[k], f"{where}.{k}")
    else:
        assert got == want and type(got) is type(want), (where, got, want)           # ints (tokens, ranks), texts, None (-inf), bools


def test_the_cases_are_the_recorded_ones():
    assert list(M.CASES) == list(GOLD)


@pytest.mark.parametrize("name", list(M.CASES))
def test_engine_calls_and_results_are_those_of_the_parent(name):
    got, want = M.run_case(name), GOLD[name]
    assert [c["call"] for c in got["calls"]] == [c["call"] for c in want["calls"]]
    for i, (g, w) in enumerate(zip(got["calls"], want["calls"])):
        assert g == w, f"call {i}"
    same(got["result"], want["result"], name)
