"""The lockstep grader (tests/sampler_lockstep.py) shown to catch what it is for, on the CPU.

The kitti and AllForOne samplers run on OracleOps with the cheap deterministic score stand-in (the score oracle
is the same function), recorded and graded: clean runs must pass.  Then one run per mutant -- each applied by
wrapping the ops object, never by editing sdp -- must fail, and the failure must name the step:

  a merger that writes one valid cell one column off in one view .... the merge of that step
  cc taken from the previous level .................................. the first merge of a ramp setting
  the absmax word not zeroed between steps .......................... the second Langevin step
  denoise fed a freshly computed lik instead of the stale one ....... the denoise
  a merge skipped at c == min_step .................................. the schedule, at that merge
  allowance 10 where 5 is due (AllForOne, setting 8) ................ the first merge
"""
import numpy as np
import pytest
import torch

import sampler_lockstep as LS
from oracle import golden_inputs as GI
from oracle.gen_golden import CIRCLE_MODS

H, W = 64, 128
SIGMAS = np.array([0.9, 0.6, 0.3], np.float32)
STEP_LR, GRAD_REF, CC0 = 6.2e-6, 1, 0.01
CASES = {  # tag: (sampler, B, aB, setting, min_step)
    "k7": ("kitti", 2, 2, 7, 1),
    "a5": ("allforone", 3, 3, 5, 0),
    "a8": ("allforone", 3, 3, 8, 1),
}


def _score(x, y):
    return LS.fake_score(torch.from_numpy(x), torch.from_numpy(y)).numpy()


def _run(tag, mutate=None):
    """Run the sampler of a case over (mutated) recorded OracleOps and grade the log."""
    from sdp.sampling import anneal_Langevin_dynamics_inpainting_simultaneous_basic as samp_a
    from sdp.sampling import anneal_Langevin_dynamics_inpainting_simultaneous_basic_kitti as samp_k
    sampler, B, aB, setting, min_step = CASES[tag]
    case = GI.merge_case("lockcpu_" + tag, B, H, W)
    x0 = GI.scorenet_input("lockcpu_" + tag, B, H, W)
    noise = lambda k: GI.noise("lockcpu_" + tag, k, (B, 2, H, W))
    k = [0]

    def noise_fn(shape):
        k[0] += 1
        return torch.from_numpy(GI.noise("lockcpu_" + tag, k[0] - 1, shape))

    rec = LS.Recording()
    inner, outer = (mutate or (lambda: (None, None)))()
    ops = rec.ops(LS.OracleOps() if inner is None else inner(LS.OracleOps()))
    ops = ops if outer is None else outer(ops)
    t = lambda a: torch.from_numpy(a.copy())
    kw = dict(n_steps_each=1, step_lr=STEP_LR, existMask=t(case["exist"]), denoise=True, verbose=False,
              grad_ref=GRAD_REF, correlation_coefficient=CC0, noise_fn=noise_fn, ops=ops)
    net = rec.net(LS.fake_score)
    if sampler == "kitti":
        images, _, shared = samp_k(t(x0), t(case["ref"]), t(case["mask"]), t(case["sky"]), None, min_step, setting, 10,
                                   net, SIGMAS, t(case["fromWorld"]), t(case["toWorld"]), aB, **kw)
    else:
        images, _, shared = samp_a(t(x0), t(case["ref"]), t(case["mask"]), t(case["sky"]), None, min_step, setting, net,
                                   SIGMAS, torch.tensor(CIRCLE_MODS[:B]), aB, **kw)
    return LS.grade(rec.records, sampler=sampler, sigmas=SIGMAS, n_steps_each=1, step_lr=STEP_LR, grad_ref=GRAD_REF,
                    ref=case["ref"], mask=case["mask"], score=_score, noise=noise, x0=x0, min_step=min_step,
                    setting=setting, cc0=CC0, allowance=10, aB=aB, sky=case["sky"], exist=case["exist"],
                    toWorld=case["toWorld"], fromWorld=case["fromWorld"], mods=CIRCLE_MODS[:B],
                    images=[i.numpy() for i in images], shared=[i.numpy() for i in shared])


@pytest.mark.parametrize("tag", list(CASES))
def test_clean_run_grades_clean(tag):
    sampler, B, aB, setting, min_step = CASES[tag]
    stats = _run(tag)
    assert [s["kind"] for s in stats] == [k for k, _ in LS.expected_schedule(sampler, 3, 1, min_step, True)]
    merges = [s for s in stats if s["kind"] == "merge"]
    assert len(merges) == 3 - min_step
    for s in merges:
        assert s["changed"] > 0 and s["flagged_share"] <= 2e-3


def test_schedule_and_ramp_are_the_reference_formulas():
    assert LS.expected_schedule("kitti", 3, 2, 1, True) == [
        ("langevin", 0), ("langevin", 0), ("langevin", 1), ("merge", 1), ("langevin", 1), ("merge", 1),
        ("langevin", 2), ("merge", 2), ("langevin", 2), ("merge", 2), ("denoise", 2), ("final", None)]
    assert LS.expected_schedule("baseline", 2, 1, 0, False) == [("langevin", 0), ("langevin", 1), ("final", None)]
    assert [LS.reference_cc("kitti", 7, 0.01, c, 3) for c in range(3)] == [0.5 / 3, 0.5 / 1.5, 0.5]
    assert [LS.reference_cc("kitti", 6, 0.01, c, 4) for c in range(4)] == [0.25, 0.5, 1 / (4 / 3), 1.0]
    assert LS.reference_cc("kitti", 5, 0.01, 1, 3) == 0.01
    assert [LS.reference_cc("allforone", 5, 0.01, c, 3) for c in range(3)] == [1 / 3, 1 / 1.5, 1.0]
    assert LS.reference_cc("allforone", 6, 0.01, 0, 2) == 0.25 and LS.reference_cc("allforone", 7, 0.01, 0, 2) == 0.01


# ------------------------------------------------------------------------------- mutants
class _Wrap:
    """An ops object that forwards to another one; a mutant overrides what it breaks."""

    def __init__(self, ops):
        self.ops = ops

    def langevin(self, *a):
        return self.ops.langevin(*a)

    def axpy(self, *a):
        return self.ops.axpy(*a)

    def make_merger(self, *a, **kw):
        return self.ops.make_merger(*a, **kw)


class _WrapMerger:
    def __init__(self, inner):
        self.inner = inner
        self.n_out, self.o_begin = inner.n_out, inner.o_begin


class ColumnOff(_Wrap):
    """Device side (under the recorder): the first merge writes one corrected cell of view 1 a column to the right."""

    def make_merger(self, *a, **kw):
        class M(_WrapMerger):
            done = False

            def __call__(self, x_all, sigma, setting, allowance, cc, absmax, new):
                before = x_all.clone()
                self.inner(x_all, sigma, setting, allowance, cc, absmax, new)
                if not self.done:
                    self.done = True
                    moved = (x_all[1, 0] != before[1, 0])[:, :-1].nonzero()
                    r, c = (int(v) for v in moved[len(moved) // 2])
                    x_all[1, :, r, c + 1] = x_all[1, :, r, c]
                    x_all[1, :, r, c] = before[1, :, r, c]
        return M(self.ops.make_merger(*a, **kw))


class StaleCc(_Wrap):
    """Sampler side: each merge gets the cc of the level before (the ramp applied a level late)."""

    def make_merger(self, *a, **kw):
        class M(_WrapMerger):
            prev = CC0

            def __call__(self, x_all, sigma, setting, allowance, cc, absmax, new):
                self.inner(x_all, sigma, setting, allowance, self.prev, absmax, new)
                self.prev = cc
        return M(self.ops.make_merger(*a, **kw))


class AbsmaxKept(_Wrap):
    """Sampler side: the absmax word is not zeroed, so the device's atomic max starts from the last step's."""
    prev = None

    def langevin(self, x, grad, ref, mask, noise, seed, offset, step, nscale, grad_ref, n2n, lik, absmax):
        if self.prev is not None:
            absmax.copy_(self.prev)
        self.ops.langevin(x, grad, ref, mask, noise, seed, offset, step, nscale, grad_ref, n2n, lik, absmax)
        self.prev = absmax.clone()


class FreshLik(_Wrap):
    """Sampler side: the denoise gets lik recomputed on the current x, not the last Langevin step's."""

    def langevin(self, x, grad, ref, mask, *a):
        self.ref, self.mask = ref, mask
        self.ops.langevin(x, grad, ref, mask, *a)

    def axpy(self, x, g, a, lik, mask, ref, b):
        if g is not None:
            lik = (-self.mask).float() * (x - self.ref)
        self.ops.axpy(x, g, a, lik, mask, ref, b)


class SkipFirstMerge(_Wrap):
    """Sampler side: no merge at c == min_step (merging starts a level late)."""

    def make_merger(self, *a, **kw):
        class M(_WrapMerger):
            calls = 0

            def __call__(self, *args):
                self.calls += 1
                if self.calls > 1:
                    self.inner(*args)
        return M(self.ops.make_merger(*a, **kw))


class Allowance10(_Wrap):
    """Sampler side: allowance 10 whatever the setting."""

    def make_merger(self, *a, **kw):
        class M(_WrapMerger):
            def __call__(self, x_all, sigma, setting, allowance, cc, absmax, new):
                self.inner(x_all, sigma, setting, 10, cc, absmax, new)
        return M(self.ops.make_merger(*a, **kw))


MUTANTS = {  # name: (case, wrapper under the recorder, wrapper over it, what the failure must say)
    "column_off": ("k7", ColumnOff, None, r"step 2 \(merge, c=1\): merge differs from the oracle"),
    "stale_cc": ("k7", None, StaleCc, r"step 2 \(merge, c=1\): cc 0\.01, reference 0\.3333"),
    "absmax_kept": ("k7", None, AbsmaxKept, r"step 1 \(langevin, c=1\): the absmax word was not zeroed"),
    "fresh_lik": ("k7", None, FreshLik, r"step 5 \(denoise, c=2\): lik \(the reference's stale likelihood"),
    "skip_first_merge": ("k7", None, SkipFirstMerge, r"step 2: the schedule .* wants merge at c=1, recorded langevin at c=2"),
    "allowance_10": ("a8", None, Allowance10, r"step 2 \(merge, c=1\): allowance 10, reference 5"),
}


@pytest.mark.parametrize("name", list(MUTANTS))
def test_mutant_fails_and_names_the_step(name):
    tag, inner, outer, says = MUTANTS[name]
    with pytest.raises(LS.LockstepError, match=says):
        _run(tag, lambda: (inner, outer))
