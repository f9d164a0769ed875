"""The ConvMeanPool 3x3 of res2 as one 4x4 stride-2 conv in the sampling forward (bf16 modes; MI355X only).

The 2x2 mean of the zero-padded 3x3 conv is a 4x4 stride-2 conv on merged weights (the "#pool4x4" packing), run on
8 x 16 tiles of the half-resolution output.  The net admits H = 64 and W >= 128; at 64x128 the half-resolution grid
has 4 x 4 tiles: corner, edge and interior ones (the zero padding differs per tile and per input phase).

Tolerances:
  * fp32x3 vs the torch-CPU oracle: the project's score-net bound, max|err| <= 1e-4 * max|ref| per image;
    a batch equals its single-image results bit for bit (B = 3: uneven part-batches under the two-stream split)
  * bf16: sampling forward vs the training forward on a float32 tape (conv-then-pool, untouched).  Both sides are one
    bf16 rounding pattern apart -- as they already were with the pool-first shortcut before the 4x4 form -- so the
    bound is 1.5x the value measured before the change on the same inputs (PARENT_BF16 below)
  * re-pack: weights overwritten in the bound arena + sdp_net_repack == a fresh net finalized with those weights,
    bit for bit (a stale merged packing fails it)
"""
import numpy as np
import pytest
import torch

from oracle import golden_inputs as GI
from oracle import scorenet_ref as R
from sdp import _lib
from sdp.scorenet import ScoreNet
from sdp.training import Trainer
from sdp.weights import synthetic_state_dict

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LABELS = [0, 57, 231]

# max|training fwd - sampling fwd| / max|sampling fwd|, bf16 mode, 64x128, B = 2, inputs of _bf16_case():
PARENT_BF16 = 8.370e-3     # before the change (conv-then-pool in both, pool-first shortcut in the sampling forward)
# measured with the 4x4 stride-2 form: 7.997e-3


def _net(W, precision="fp32x3"):
    return ScoreNet(H=64, W=W, precision=precision).load_synthetic()


@pytest.fixture(scope="module")
def nets():
    return {W: _net(W) for W in (128, 256)}


@pytest.fixture(scope="module")
def oracle():
    P = R.to_torch_params(synthetic_state_dict(128))
    cache = {}

    def get(B, W):
        if (B, W) not in cache:
            x = torch.from_numpy(GI.scorenet_input(f"pool4x4-{W}", 3, 64, W))[:B]
            y = torch.tensor(LABELS[:B])
            with torch.no_grad():
                cache[(B, W)] = (x, y, R.scorenet_forward(P, x, y).numpy())
        return cache[(B, W)]
    return get


@pytest.mark.parametrize("B,W", [(1, 128), (3, 128), (2, 256)])
def test_fp32x3_matches_oracle_on_border_and_mixed_tiles(nets, oracle, B, W):
    x, y, ref = oracle(B, W)
    net = nets[W]
    out = net(x.to(DEV), y.to(DEV)).cpu().numpy()
    assert np.isfinite(out).all()
    errs = [np.abs(out[b] - ref[b]).max() / np.abs(ref[b]).max() for b in range(B)]
    print(f"fp32x3 64x{W} B={B}: max err / max|ref| per image = {['%.3e' % e for e in errs]}")
    assert max(errs) <= 1e-4
    if B == 3:   # no cross-image coupling, whatever part-batch an image lands in
        for b in range(B):
            o1 = net(x[b:b + 1].to(DEV), y[b:b + 1].to(DEV)).cpu().numpy()
            np.testing.assert_array_equal(o1[0], out[b])


def _bf16_case():
    x = torch.from_numpy(GI.scorenet_input("pool4x4-bf16", 2, 64, 128))
    return x, torch.tensor([3, 200])


def test_bf16_sampling_forward_vs_float32_tape_training_forward():
    """Measured max|a - b| / max|b|: 8.370e-3 before the change (PARENT_BF16), 7.997e-3 with the 4x4 stride-2 form."""
    net = _net(128, "bf16")
    tr = Trainer(net, tape_bf16=False)
    x, y = _bf16_case()
    a = tr.forward(x.to(DEV), y.to(DEV))
    b = net(x.to(DEV), y.to(DEV))
    torch.cuda.synchronize()
    assert torch.isfinite(a).all() and torch.isfinite(b).all()
    err = ((a - b).abs().max() / b.abs().max()).item()
    print(f"bf16 training (float32 tape) vs sampling forward: max err / max|out| = {err:.3e} (before: {PARENT_BF16:.3e})")
    assert err <= 1.5 * PARENT_BF16


def test_repack_rebuilds_the_merged_weights(oracle):
    x, y, _ = oracle(1, 128)
    keys = ["res2.0.conv2.conv.weight", "res2.0.shortcut.conv.weight"]
    sd = synthetic_state_dict(128)
    r = GI.rng("pool4x4-repack")
    new = {k: (sd[k] * 0.5 + 0.02 * r.standard_normal(sd[k].shape)).astype(np.float32) for k in keys}

    net = _net(128)
    tr = Trainer(net)
    stale = net(x.to(DEV), y.to(DEV)).cpu().numpy()
    views = dict(tr.named_parameters())
    for k in keys:
        views[k].copy_(torch.from_numpy(new[k]))
    _lib.check(tr.L.sdp_net_repack(net._h, _lib.stream()), "repack")
    got = net(x.to(DEV), y.to(DEV)).cpu().numpy()

    sd.update(new)
    fresh = ScoreNet(H=64, W=128, precision="fp32x3").load_state_dict(sd)
    want = fresh(x.to(DEV), y.to(DEV)).cpu().numpy()
    assert np.abs(want - stale).max() > 1e-3 * np.abs(want).max()   # the new weights do change the output
    np.testing.assert_array_equal(got, want)
