"""The plan the graph walker (csrc/net_graph.h) launches is the plan of the parent commit, structurally:
per precision the set of launch classes of one profiled sampling forward, and per class the launch
count, FLOPs and bytes per launch, equal the table recorded on the parent
(tests/golden/scorenet_plan_parent.json, tools/plan_record.py); times are ignored.  B = 1 at 64x128, the
smallest shape there is -- exact fp32 at 64x256, the smallest it runs (its 256-channel kernel tiles the
dilation-4 sub-grid at half resolution 4 x 32; the parent rejects 64x128 just the same).  The training
workspace (every tensor the training runtime allocates through the same walker) has the parent's size."""
import pytest

from test_plan_workspace_cpu import parent, plan_record

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("precision", ["fp32", "fp32x3", "bf16"])
def test_launch_table_equals_the_parents(precision):
    want = {k: tuple(v) for k, v in parent()["launch_table"][precision].items()}
    got = {k: tuple(v) for k, v in plan_record().launch_table(precision).items()}
    assert set(got) == set(want)
    assert got == want
    # what the table pins: the ConvMeanPool block per mode, one pool-first shortcut, the eight CRP pools
    s2 = [k for k in got if k.startswith("conv4x4s2")]
    pool = [k for k in got if k.endswith(" pool")]
    assert (len(s2), len(pool)) == ((0, 1) if precision == "fp32" else (1, 0))
    assert sum(n for k, (n, _, _) in got.items() if k.startswith("avgpool2")) == 1
    assert sum(n for k, (n, _, _) in got.items() if k.startswith("maxpool5")) == 8


def test_training_workspace_sizes_equal_the_parents():
    want = parent()["train_workspace"]
    assert len(want) == 3 * 2
    assert plan_record().train_workspace() == want
