"""Every step of the samplers on the device, graded against the oracle from the device's own state (MI355X only).

The end-to-end tests of test_gpu_parity.py and test_gpu_runner.py compare a device trajectory with a
reference-generated one and therefore allow 0.1 % of the values to differ by any amount.  Here nothing
may: each sampler runs once over recording ops and a recording score net (tests/sampler_lockstep.py), and
every transition is then replayed on the CPU oracle from the recorded input of that step --

  * schedule: the kinds and levels of the calls are what (L, n_steps_each, min_step, denoise) dictates;
  * host scalars (step size, noise scale, cc ramp, allowance, sigma): bit-equal to the reference formulas;
  * scores: the fp32x3 gate of test_gpu_parity.py, max|err| <= 1e-4 * max|ref| per image;
  * Langevin update, lik, the absmax word, denoise, final data consistency: bit-equal;
  * merge: the SURVEY 8(c) rule (_assert_merge_exact) on x and on the new images -- exact zero pattern and
    rtol 1e-5 / atol 2e-6 outside the pixels the oracle flags, no mismatch fraction, flagged share <= 2e-3
    (along the oracle's own trajectories of these cases the flagged share per merge was 0, 0, 0 and at most
    8.14e-5);
  * the returned lists are the recorded buffers, bit for bit.
"""
import time

import numpy as np
import pytest
import torch

import sampler_lockstep as LS
from oracle import golden_inputs as GI
from oracle import scorenet_ref as R
from oracle.gen_golden import CIRCLE_MODS

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
H, W = 64, 128
STEP_LR, GRAD_REF, CC0 = 6.2e-6, 1, 0.01
# a merged image is non-trivial when both its zero pixels (cells no point lands in) and its filled pixels are at
# least 1 % of it (82 of a 64 x 128 view): five times the 2e-3 share the oracle may flag, so the exact zero-pattern
# comparison always has unflagged pixels of both kinds to grade
ZERO_SHARE = (0.01, 0.99)

CASES = [  # tag, sampler, B, aB, setting, min_step
    ("lock_k5", "kitti", 2, 2, 5, 1),         # constant cc, depth filter
    ("lock_k7", "kitti", 4, 2, 7, 1),         # two megabatches, cc ramp
    ("lock_a5", "allforone", 3, 3, 5, 0),     # cc ramp from level 0, shared image at level 0
    ("lock_a7", "allforone", 3, 3, 7, 1),     # controlled average
    ("lock_b", "baseline", 1, None, None, None),   # keep_all: no merge, no nan_to_num
]


@pytest.fixture(scope="module")
def net128():
    from sdp.scorenet import ScoreNet
    return ScoreNet(H=H, W=W, precision="fp32x3").load_synthetic()


@pytest.fixture(scope="module")
def oracle_score():
    from sdp.weights import synthetic_state_dict
    P = R.to_torch_params(synthetic_state_dict(128))

    def score(x, y):
        with torch.no_grad():
            return R.scorenet_forward(P, torch.from_numpy(x), torch.from_numpy(y)).numpy()
    return score


@pytest.mark.parametrize("tag,sampler,B,aB,setting,min_step", CASES, ids=[c[0] for c in CASES])
def test_sampler_steps_match_the_oracle_in_lockstep(net128, oracle_score, tag, sampler, B, aB, setting, min_step):
    from sdp import sampling
    from sdp.weights import get_sigmas_np
    sigmas = get_sigmas_np()[229:232]
    case = GI.merge_case(tag, B, H, W)
    x0 = GI.scorenet_input(tag, B, H, W)
    k = [0]

    def noise_fn(shape):
        k[0] += 1
        return torch.from_numpy(GI.noise(tag, k[0] - 1, shape))

    rec = LS.Recording()
    ops, net = rec.ops(), rec.net(net128)
    assert isinstance(ops, sampling.DeviceOps) and hasattr(net, "forward_langevin")
    t = lambda a: torch.from_numpy(a).to(DEV)
    kw = dict(n_steps_each=1, step_lr=STEP_LR, denoise=True, verbose=False, grad_ref=GRAD_REF, noise_fn=noise_fn, ops=ops)
    t0 = time.perf_counter()
    shared = []
    if sampler == "kitti":
        images, _, shared = sampling.anneal_Langevin_dynamics_inpainting_simultaneous_basic_kitti(
            t(x0), t(case["ref"]), t(case["mask"]), t(case["sky"]), None, min_step, setting, 10, net, sigmas,
            t(case["fromWorld"].reshape(B, 1, 4, 4)), t(case["toWorld"].reshape(B, 1, 4, 4)), aB,
            existMask=t(case["exist"]), correlation_coefficient=CC0, **kw)
    elif sampler == "allforone":
        images, _, shared = sampling.anneal_Langevin_dynamics_inpainting_simultaneous_basic(
            t(x0), t(case["ref"]), t(case["mask"]), t(case["sky"]), None, min_step, setting, net, sigmas,
            torch.tensor(CIRCLE_MODS[:B]), aB, existMask=t(case["exist"]), correlation_coefficient=CC0, **kw)
    else:
        images, _ = sampling.anneal_Langevin_dynamics_inpainting(t(x0), t(case["ref"]), t(case["mask"]), net, sigmas,
                                                                 keep_all=True, **kw)
    torch.cuda.synchronize()
    t_dev = time.perf_counter() - t0

    # the fused path ran: every Langevin step is a forward_langevin record, none the two-call form
    lang = [r for r in rec.records if r["kind"] == "langevin"]
    assert len(lang) == 3 and all(r["via"] == "forward_langevin" for r in lang)

    stats = LS.grade(rec.records, sampler=sampler, sigmas=sigmas, n_steps_each=1, step_lr=STEP_LR, grad_ref=GRAD_REF,
                     ref=case["ref"], mask=case["mask"], score=oracle_score, noise=lambda i: GI.noise(tag, i, x0.shape),
                     x0=x0, min_step=min_step or 0, setting=setting, cc0=CC0, allowance=10, aB=aB, sky=case["sky"],
                     exist=case["exist"], toWorld=case["toWorld"], fromWorld=case["fromWorld"],
                     mods=CIRCLE_MODS[:B], images=[i.numpy() for i in images], shared=[i.numpy() for i in shared],
                     keep_all=True)
    merges = [s for s in stats if s["kind"] == "merge"]
    assert len(merges) == (0 if sampler == "baseline" else 3 - min_step)
    for s in merges:
        # (without a new buffer of the sampler's the zero pattern is the oracle's, which the corrected x was graded on)
        print(f"{tag} step {s['k']}: zero share of the new images {s['zero_share']:.4f}, {s['changed']} values of x changed, "
              f"flagged share {s['flagged_share']:.2e}")
        assert s["changed"] > 0, f"step {s['k']}: the merge left x unchanged"
        assert ZERO_SHARE[0] <= s["zero_share"] <= ZERO_SHARE[1], f"step {s['k']}: zero share {s['zero_share']}"
        assert s["flagged_share"] <= 2e-3
    print(f"{tag}: {len(stats)} steps graded, device run {t_dev:.2f} s, with the oracle {time.perf_counter() - t0:.2f} s; "
          f"largest score error {max(s.get('score_err', 0.0) for s in stats):.3e}, "
          f"largest merge error outside the flagged pixels {max(s['max_err'] for s in stats):.3e}")
