"""The host route of the fused blocks launches what the recorded commit launched: for every case of block_trace_cases.py
(tiny STDiT and PixArt models behind each route switch, off and on) the ordered list of ops calls - function, shape / dtype
/ strides of every tensor argument, value of every scalar argument - equals tests/golden/fused_block_traces.json, and the
output's SHA-256 equals the recorded one wherever two runs of the recording commit agreed on it
(tests/golden/make_block_traces.py)."""
import json

import pytest

import block_trace_cases as bt

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def recorded():
    with open(bt.FIXTURE) as f:
        fx = json.load(f)
    assert sorted(fx["cases"]) == sorted(bt.NAMES), "the fixture and block_trace_cases.CASES name different cases"
    return [json.dumps(c, sort_keys=True) for c in fx["calls"]], fx["cases"]


@pytest.mark.parametrize("name", bt.NAMES)
def test_fused_route_makes_the_recorded_calls(ops, dev, recorded, name):
    table, cases = recorded
    want = [table[i] for i in cases[name]["trace"]]
    got, sha = bt.run_case(name, dev)
    for j, (a, b) in enumerate(zip(got, want)):
        assert a == b, "call %d of %d differs:\n  now      %s\n  recorded %s" % (j, len(want), a, b)
    unmatched = got[len(want):] or want[len(got):]
    assert not unmatched, "%d calls now, %d recorded; the first unmatched one: %s" % (len(got), len(want), unmatched[0])
    print("%s: %d calls equal; output digest %s" % (name, len(got), "recorded" if cases[name]["sha256"] else "not recorded"))
    if cases[name]["sha256"] is not None:
        assert sha == cases[name]["sha256"], "the output's bytes differ from the recorded run's"
