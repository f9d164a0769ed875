"""Digests of what the score-net plan computes, for a one-time bit-identity check between two builds of
libsdp (SDP_LIB=<libsdp.so> selects the build): sampling at 64x128, the smallest shape (exact fp32: 64x256,
the smallest its 256-channel dilated layers tile), training at 64x256 (its data and weight gradients want
sub-grids 32 n wide), B=3 (the default two-way split runs parts of 1 and 2 images), fixed seeds, per
precision the SHA-256 of
  forward    the output of ScoreNet.forward
  langevin   x after one forward_langevin with Philox noise
  train_fwd  the scores of Trainer.forward              (fp32x3, bf16)
  grads      the gradient arena after one backward      (fp32x3, bf16)
--save DIR also writes the gradient arenas as DIR/grads_<precision>.npy; `--diff A B` prints, per
precision, max|A - B| / max|B| of two such directories (for weight gradients that are not
reproducible run to run).  The log of one comparison: profiles/experiments/plan_walker_identity.log.
"""
import argparse
import hashlib
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (REPO, os.path.join(REPO, "simultaneous-diffusion-for-pointclouds_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

H, B = 64, 3
WIDTH = {"fp32": 256, "fp32x3": 128, "bf16": 128}   # sampling
TRAIN_WIDTH = 256


def sha(t):
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


def digests(save):
    from sdp.scorenet import ScoreNet
    from sdp.training import Trainer
    dev = "cuda:0"
    y = torch.tensor([3, 100, 231]).to(dev)
    for prec in ("fp32", "fp32x3", "bf16"):
        W = WIDTH[prec]
        g = torch.Generator().manual_seed(20)
        x = torch.rand(B, 2, H, W, generator=g).to(dev)
        ref = torch.rand(B, 2, H, W, generator=g).to(dev)
        mask = (torch.rand(B, 2, H, W, generator=g) > 0.4).to(torch.int32).to(dev)
        net = ScoreNet(H=H, W=W, precision=prec).load_synthetic()
        print(f"{prec:7s} forward   {sha(net(x, y))}")
        xl = x.clone()
        net.forward_langevin(xl, y, ref, mask, None, 1234, 96, 1e-4, 0.014, 1.0, True, None, None)
        print(f"{prec:7s} langevin  {sha(xl)}")
        if prec == "fp32":
            continue
        x = torch.rand(B, 2, H, TRAIN_WIDTH, generator=g).to(dev)
        dscore = torch.randn(B, 2, H, TRAIN_WIDTH, generator=g).to(dev)
        tr = Trainer(ScoreNet(H=H, W=TRAIN_WIDTH, precision=prec).load_synthetic())
        print(f"{prec:7s} train_fwd {sha(tr.forward(x, y))}")
        tr.backward(dscore)
        print(f"{prec:7s} grads     {sha(tr.grads)}")
        if save:
            os.makedirs(save, exist_ok=True)
            np.save(os.path.join(save, f"grads_{prec}.npy"), tr.grads.cpu().numpy())


def diff(a, b):
    for prec in ("fp32x3", "bf16"):
        ga, gb = (np.load(os.path.join(d, f"grads_{prec}.npy")).astype(np.float64) for d in (a, b))
        print(f"{prec:7s} grads max|A-B|/max|B| = {np.abs(ga - gb).max() / np.abs(gb).max():.3e}")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--save", default=None)
    ap.add_argument("--diff", nargs=2, default=None)
    a = ap.parse_args()
    if a.diff:
        diff(*a.diff)
    else:
        digests(a.save)
    sys.stdout.flush()
