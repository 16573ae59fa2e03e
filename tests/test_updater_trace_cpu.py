"""FleetUpdater against a call trace recorded on the commit before its methods were split
(tests/golden/updater_traces.json, by tests/golden/make_updater_traces.py): in every scenario
of tests/updater_trace.py the updater makes the same calls with the same arguments in the same
order on everything it touches, returns or raises the same, and ends in the same public state."""
import json
import os

import pytest

import fleet_amd.updater
import updater_trace as T

with open(os.path.join(os.path.dirname(__file__), "golden", "updater_traces.json")) as f:
    GOLDEN = json.load(f)


def test_the_record_holds_the_scenario_list_and_names_its_commit():
    assert list(GOLDEN["scenarios"]) == [name for name, _, _ in T.scenarios()]
    assert len(GOLDEN["recorded_from"]) == 40


@pytest.mark.parametrize("name", [name for name, _, _ in T.scenarios()])
def test_scenario_reproduces_the_record(name):
    got, want = T.run_all(fleet_amd.updater, only=name)[name], GOLDEN["scenarios"][name]
    assert got["returns"] == want["returns"]
    for k, (a, b) in enumerate(zip(got["trace"], want["trace"])):
        assert a == b, f"call {k}"
    assert len(got["trace"]) == len(want["trace"])
    assert got["state"] == want["state"]
