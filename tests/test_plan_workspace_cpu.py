"""The sampling workspace of the score net is what it was before the forward plan moved into
csrc/net_graph.h: sdp_net_workspace_size for both shapes, B in {1,2,3,5} and split 0/1/2/4 against the
sizes recorded on the parent commit (tests/golden/scorenet_plan_parent.json, tools/plan_record.py).
Needs no GPU and no weights."""
import importlib.util
import json
import os

from conftest import GOLDEN, REPO


def plan_record():
    spec = importlib.util.spec_from_file_location("plan_record", os.path.join(REPO, "tools", "plan_record.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def parent():
    with open(os.path.join(GOLDEN, "scorenet_plan_parent.json")) as f:
        return json.load(f)


def test_sampling_workspace_sizes_equal_the_parents():
    want = parent()["sampling_workspace"]
    got = plan_record().sampling_workspace()
    assert len(want) == 2 * 4 * 4
    assert got == want
