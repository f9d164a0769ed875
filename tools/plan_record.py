"""Record the structure of the score-net plan as the loaded libsdp runs it: the sampling workspace
sizes (no GPU needed), and on a GPU the training workspace sizes and the per-class launch table
of one profiled sampling forward.  tests/golden/scorenet_plan_parent.json is this script's output
on the commit before the forward plan moved into csrc/net_graph.h; the tests that read it
(tests/test_plan_workspace_cpu.py, tests/test_gpu_plan_table.py) use the functions below, so the
recording and the check cannot drift apart.

    python tools/plan_record.py OUT.json            (SDP_LIB=<libsdp.so> selects another build)
"""
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (REPO, os.path.join(REPO, "simultaneous-diffusion-for-pointclouds_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import torch  # noqa: E402

SHAPES = ((64, 128), (64, 1024))
BATCHES = (1, 2, 3, 5)
SPLITS = (0, 1, 2, 4)
PRECISIONS = ("fp32", "fp32x3", "bf16")
# (precision, bf16 tape) of the training workspace
TRAIN_TAPES = (("fp32x3", True), ("bf16", True), ("bf16", False))
TRAIN_BATCHES = (1, 2)
# the smallest shape each precision runs: 64x128 is the smallest sdp_net_create accepts, but the exact-fp32
# 256-channel kernel tiles the dilation-4 sub-grid at half resolution 4 x 32, which needs W >= 256
TABLE_SHAPE = {"fp32": (64, 256), "fp32x3": (64, 128), "bf16": (64, 128)}


def sampling_workspace():
    """{"HxW/B/split": bytes} of sdp_net_workspace_size (no weights, no GPU)."""
    from sdp import _lib
    from sdp.scorenet import ScoreNet
    out = {}
    for H, W in SHAPES:
        net = ScoreNet(H=H, W=W)
        for split in SPLITS:
            net.set_split(split)
            for B in BATCHES:
                n = _lib.SZ()
                _lib.check(_lib.lib().sdp_net_workspace_size(net._h, B, _lib.C.byref(n)), "workspace_size")
                out[f"{H}x{W}/B{B}/split{split}"] = n.value
    return out


def train_workspace():
    """{"precision/tape/B": bytes} of sdp_net_train_workspace_size at 64x128 (needs finalized weights)."""
    from sdp import _lib
    from sdp.scorenet import ScoreNet
    out = {}
    for prec, tape16 in TRAIN_TAPES:
        net = ScoreNet(H=64, W=128, precision=prec).load_synthetic()
        net.set_tape(tape16)
        for B in TRAIN_BATCHES:
            n = _lib.SZ()
            _lib.check(_lib.lib().sdp_net_train_workspace_size(net._h, B, _lib.C.byref(n)), "train_workspace_size")
            out[f"{prec}/{'bf16' if tape16 else 'fp32'}tape/B{B}"] = n.value
    return out


def launch_table(precision):
    """{class: [launches, flops per launch, bytes per launch]} of one profiled forward at TABLE_SHAPE, B=1."""
    from sdp.scorenet import ScoreNet
    H, W = TABLE_SHAPE[precision]
    net = ScoreNet(H=H, W=W, precision=precision).load_synthetic()
    g = torch.Generator().manual_seed(1)
    x = torch.rand(1, 2, H, W, generator=g).cuda()
    y = torch.tensor([7]).cuda()
    net.profile(True)
    net(x, y)
    torch.cuda.synchronize()
    return {cls: [n, fl, by] for cls, (n, _ms, fl, by) in net.profile_read().items()}


def main():
    doc = {"sampling_workspace": sampling_workspace()}
    if torch.cuda.is_available():
        doc["train_workspace"] = train_workspace()
        doc["launch_table"] = {p: launch_table(p) for p in PRECISIONS}
    with open(sys.argv[1], "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
