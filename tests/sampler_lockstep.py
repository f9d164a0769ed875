"""Lockstep grading of the samplers (a helper module, like kernel_lib.py): record every device call of
a sampler run, then grade each transition against the CPU oracle from the run's OWN recorded state.

Comparing a device trajectory with an oracle trajectory needs a mismatch allowance: the score net
differs by ~1e-4 relative, which moves a point across a merge-bin edge that the oracle's flags (computed on
the oracle's state) do not cover.  Grading transition by transition does not: every oracle evaluation starts
from the recorded input of that step, so the gates are the exact ones -- bit equality for the elementwise
steps and the host scalars, the SURVEY 8(c) merge rule (``_assert_merge_exact``) for the merge, and
the score net's own tolerance for the scores.

  Recording ...... ``rec.ops(inner)`` (a DeviceOps subclass, so the fused forward_langevin path stays in use) and
                   ``rec.net(scorenet)``; pass both to a sampler of sdp/sampling.py; ``rec.records`` is the log
  grade ........... replays the log against oracle/sampling_ref.py and a score oracle
  OracleOps ....... the CPU stand-in for the device ops (the gloo tests and the grader's self-test)
"""
from __future__ import annotations

import numpy as np
import torch

from oracle import philox_ref
from oracle import sampling_ref as S
from sdp.sampling import DeviceOps

F32 = np.float32
SCORE_TOL = 1e-4          # fp32x3 score net: max|err| <= 1e-4 * max|ref| per image (tests/test_gpu_parity.py)
NEW_LEVELS = (0, 20, 110)  # the levels whose merged images the reference keeps, besides the last


# ------------------------------------------------------------------------------- CPU stand-ins
class OracleMerger:
    def __init__(self, n_all, aB, H, W, dev, exist, sky, refmask, toWorld=None, fromWorld=None, origins=None,
                 o_begin=0, n_out=None):
        self.aB, self.o_begin, self.n_out = aB, o_begin, n_out
        self.exist = np.asarray(exist)
        self.sky = np.asarray(sky).reshape(n_all, 1, H, W)
        self.refmask = np.asarray(refmask)
        # origin-offset variant: the origins are already 10*sign(m), which the oracle maps to themselves
        self.mods = None if origins is None else np.asarray(origins)
        if origins is None:
            self.toWorld = np.asarray(toWorld).reshape(n_all, 4, 4)
            self.fromWorld = np.asarray(fromWorld).reshape(n_all, 4, 4)

    def __call__(self, x_all, sigma, setting, allowance, cc, absmax, new):
        amax = absmax.view(torch.float32).item()
        if self.mods is not None:
            n, xc = S.allforone_merge(x_all.numpy(), self.refmask, self.sky, self.exist, self.mods, self.aB, sigma,
                                      setting, cc, absmax=amax)
        else:
            n, xc = S.kitti_merge(x_all.numpy(), self.refmask, self.sky, self.exist, self.toWorld, self.fromWorld,
                                  self.aB, sigma, setting, allowance, cc, absmax=amax)
        sl = slice(self.o_begin, self.o_begin + self.n_out)
        x_all[sl] = torch.from_numpy(xc[sl])
        if new is not None:
            new.copy_(torch.from_numpy(n[sl]))


class OracleOps:
    def langevin(self, x, grad, ref, mask, noise, seed, offset, step, nscale, grad_ref, nan_to_num, lik, absmax):
        g = S.nan_to_num(grad.numpy()) if nan_to_num else grad.numpy()
        if noise is None:   # the kernel's Philox stream (seed, counter = offset + element/4)
            noise = torch.from_numpy(philox_ref.normal(seed, offset, x.numel()).reshape(x.shape))
        lk = (-mask.numpy()).astype(np.float32) * (x.numpy() - ref.numpy())
        v = (((x.numpy() + np.float32(step) * g) + np.float32(grad_ref) * lk) + noise.numpy() * np.float32(nscale))
        x.copy_(torch.from_numpy(v.astype(np.float32)))
        lik.copy_(torch.from_numpy(lk))
        absmax.copy_(torch.tensor([np.abs(v[:, 0]).max()], dtype=torch.float32).view(torch.int32))

    def axpy(self, x, g, a, lik, mask, ref, b):
        if g is not None:
            x.copy_(((x + np.float32(a) * g) + np.float32(b) * lik))
        else:
            x.copy_(x + np.float32(b) * ((-mask).float() * (x - ref)))

    def make_merger(self, *a, **kw):
        return OracleMerger(*a, **kw)


def fake_score(x, y):
    """Deterministic stand-in for the score net (depends on x and on the label)."""
    return -(x - 0.5) * (1.0 + 0.01 * y.view(-1, 1, 1, 1).float()) + 0.05 * torch.sin(7 * x)


# ------------------------------------------------------------------------------- the recorder
def _cpu(t):
    """A CPU numpy copy of a tensor as it is now (None stays None)."""
    return None if t is None else t.detach().to("cpu", copy=True).numpy()


def _word(absmax):
    """The absmax word (float bits of max|x[:, 0]|) as an unsigned int."""
    return None if absmax is None else int(absmax.detach().cpu().view(torch.int32).reshape(-1)[0].item()) & 0xFFFFFFFF


class Recording:
    """The log of one sampler run.  Each record is a dict: ``kind`` (langevin / merge / denoise / final), ``c``
    (the level label), CPU copies of the call's inputs taken before it, its scalar arguments, and CPU copies of
    its outputs taken after it."""

    def __init__(self):
        self.records = []
        self.score_call = None      # the last plain scorenet(x, y) call, until the ops call that consumes it

    def ops(self, inner=None):
        return RecordingOps(self, DeviceOps() if inner is None else inner)

    def net(self, inner):
        return (RecordingNet if hasattr(inner, "forward_langevin") else RecordingScore)(self, inner)

    def take_score(self):
        sc, self.score_call = self.score_call, None
        return sc or dict(x=None, y=None, scores=None)

    def last_level(self):
        for r in reversed(self.records):
            if r["kind"] == "langevin":
                return r["c"]
        return None


class RecordingScore:
    """scorenet(x, y) with its input and output noted for the ops call that follows (the two-call path, and
    the denoise step of every path)."""

    def __init__(self, rec, inner):
        self._rec, self._inner = rec, inner

    def __call__(self, x, y):
        xb, yb = _cpu(x), _cpu(y)
        out = self._inner(x, y)
        self._rec.score_call = dict(x=xb, y=yb, scores=_cpu(out))
        return out


class RecordingNet(RecordingScore):
    """A score net with the fused step: forward_langevin is forwarded, always with a grad_out buffer."""

    def forward_langevin(self, x, y, ref, mask, noise, seed, offset, step, nscale, grad_ref, nan_to_num, lik, absmax,
                         grad_out=None):
        r = dict(kind="langevin", via="forward_langevin", c=int(y.reshape(-1)[0].item()), y=_cpu(y), x_before=_cpu(x),
                 score_x=None, ref=_cpu(ref), mask=_cpu(mask), noise=_cpu(noise), seed=seed, offset=offset, step=step,
                 nscale=nscale, grad_ref=grad_ref, nan_to_num=bool(nan_to_num), absmax_in=_word(absmax))
        if grad_out is None:
            grad_out = torch.empty_like(x)
        self._inner.forward_langevin(x, y, ref, mask, noise, seed, offset, step, nscale, grad_ref, nan_to_num, lik,
                                     absmax, grad_out)
        r.update(scores=_cpu(grad_out), x_after=_cpu(x), lik=_cpu(lik), absmax=_word(absmax))
        self._rec.records.append(r)


class RecordingMerger:
    def __init__(self, rec, inner):
        self._rec, self._inner = rec, inner
        self.n_out, self.o_begin = inner.n_out, inner.o_begin

    def __call__(self, x_all, sigma, setting, allowance, cc, absmax, new=None, **kw):
        r = dict(kind="merge", c=self._rec.last_level(), x_before=_cpu(x_all), sigma=sigma, setting=setting,
                 allowance=allowance, cc=cc, absmax=_word(absmax), o_begin=self.o_begin, n_out=self.n_out)
        self._inner(x_all, sigma, setting, allowance, cc, absmax, new, **kw)
        r.update(x_after=_cpu(x_all), new=_cpu(new))
        self._rec.records.append(r)


class RecordingOps(DeviceOps):
    """DeviceOps that logs each call around ``inner`` (DeviceOps, or OracleOps on the CPU)."""

    def __init__(self, rec, inner):
        self._rec, self._inner = rec, inner

    def langevin(self, x, grad, ref, mask, noise, seed, offset, step, nscale, grad_ref, nan_to_num, lik, absmax):
        sc = self._rec.take_score()
        r = dict(kind="langevin", via="langevin", c=None if sc["y"] is None else int(sc["y"].reshape(-1)[0]), y=sc["y"],
                 x_before=_cpu(x), score_x=sc["x"], scores=_cpu(grad), ref=_cpu(ref), mask=_cpu(mask),
                 noise=_cpu(noise), seed=seed, offset=offset, step=step, nscale=nscale, grad_ref=grad_ref,
                 nan_to_num=bool(nan_to_num), absmax_in=_word(absmax))
        self._inner.langevin(x, grad, ref, mask, noise, seed, offset, step, nscale, grad_ref, nan_to_num, lik, absmax)
        r.update(x_after=_cpu(x), lik=_cpu(lik), absmax=_word(absmax))
        self._rec.records.append(r)

    def axpy(self, x, g, a, lik, mask, ref, b):
        if g is not None:
            sc = self._rec.take_score()
            r = dict(kind="denoise", c=None if sc["y"] is None else int(sc["y"].reshape(-1)[0]), y=sc["y"],
                     x_before=_cpu(x), score_x=sc["x"], scores=_cpu(g), a=a, b=b, lik=_cpu(lik))
        else:
            r = dict(kind="final", c=None, x_before=_cpu(x), mask=_cpu(mask), ref=_cpu(ref), b=b)
        self._inner.axpy(x, g, a, lik, mask, ref, b)
        r["x_after"] = _cpu(x)
        self._rec.records.append(r)

    def make_merger(self, *args, **kw):
        return RecordingMerger(self._rec, self._inner.make_merger(*args, **kw))


# ------------------------------------------------------------------------------- the merge gate
def _assert_merge_exact(got_new, want_new, got_x, want_x, flagged, what=""):
    """SURVEY 8(c) merge gate: outside the pixels the oracle flags (oracle/sampling_ref.py flag_cells:
    a point within float rounding of a bin edge or of the depth filter, a nearest-depth tie, a
    controlled-average branch on its edge) the zero pattern (mask / bins) must agree exactly and every
    value within float rounding (rtol 1e-5, atol 2e-6: float64 sums in another order, the device's float32
    exp2); no fraction of mismatches is allowed.  Prints the flagged count."""
    fl = np.broadcast_to(np.asarray(flagged)[:, None], got_new.shape)
    ok = ~fl
    bad_new = (np.abs(got_new - want_new) > 2e-6 + 1e-5 * np.abs(want_new)) & ok
    bad_zero = ((got_new != 0) != (want_new != 0)) & ok
    bad_x = (np.abs(got_x - want_x) > 2e-6 + 1e-5 * np.abs(want_x)) & ok
    print(f"merge {what}: {int(np.asarray(flagged).sum())} of {np.asarray(flagged).size} pixels flagged, "
          f"mismatches outside them: values {int(bad_new.sum())}, zero pattern {int(bad_zero.sum())}, x {int(bad_x.sum())}")
    assert np.asarray(flagged).mean() <= 2e-3, "the oracle flags too much to grade"
    assert not bad_zero.any(), np.argwhere(bad_zero)[:8]
    assert not bad_new.any(), np.argwhere(bad_new)[:8]
    assert not bad_x.any(), np.argwhere(bad_x)[:8]


# ------------------------------------------------------------------------------- the grader
class LockstepError(AssertionError):
    pass


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=F32)).view(np.uint32)


def _f32_bits(v):
    return int(np.asarray(v, dtype=F32).reshape(1).view(np.uint32)[0])


def _need(cond, where, msg):
    if not cond:
        raise LockstepError(f"{where}: {msg}")


def _need_bits(got, want, where, what):
    """got and want are the same float32 values bit for bit."""
    _need(got is not None, where, f"{what} was not passed")
    got, want = np.asarray(got), np.asarray(want)
    _need(got.shape == want.shape, where, f"{what} has shape {got.shape}, not {want.shape}")
    bad = _bits(got) != _bits(want)
    if bad.any():
        i = tuple(np.argwhere(bad)[0])
        raise LockstepError(f"{where}: {what} is not bit-equal in {int(bad.sum())} of {bad.size} values, first at {i}: "
                            f"{got[i]!r} instead of {want[i]!r}")


def _rel_err(out, ref):
    return max(np.abs(out[b] - ref[b]).max() / np.abs(ref[b]).max() for b in range(ref.shape[0]))


def _absmax_ok(word, x_after):
    """word == the float bits of numpy's max|x[:, 0]| (any NaN bits when that is NaN)."""
    want = F32(np.abs(x_after[:, 0]).max())
    if np.isnan(want):
        return bool(np.isnan(np.array([word], np.uint32).view(F32)[0])), want
    return word == _f32_bits(want), want


def expected_schedule(sampler, L, n_steps_each, min_step, denoise):
    """[(kind, c)] of a run: a Langevin step per (level, repeat), for the simultaneous samplers a merge after
    every step with c >= min_step and after none before, then the denoise at the last level and the final
    data consistency."""
    out = []
    for c in range(L):
        for _ in range(n_steps_each):
            out.append(("langevin", c))
            if sampler != "baseline" and c >= min_step:
                out.append(("merge", c))
    if denoise:
        out.append(("denoise", L - 1))
    out.append(("final", None))
    return out


def reference_cc(sampler, setting, cc0, c, L):
    """The correlation ramp of the reference, written out from its formulas (KITTISampling.py:108-111: settings 6 / 7;
    models/__init__.py:209-212: settings 5 / 6); any other setting keeps the constant."""
    full, half = {"kitti": (6, 7), "allforone": (5, 6)}[sampler]
    if setting == full:
        return 1 / (L / (c + 1))
    if setting == half:
        return 0.5 / (L / (c + 1))
    return cc0


def _label(k, r):
    return f"step {k} ({r['kind']}" + ("" if r["c"] is None else f", c={r['c']}") + ")"


def grade(records, *, sampler, sigmas, n_steps_each, step_lr, grad_ref, ref, mask, score, noise, denoise=True, x0=None,
          min_step=0, setting=None, cc0=None, allowance=None, aB=None, sky=None, exist=None, toWorld=None,
          fromWorld=None, mods=None, images=None, shared=None, keep_all=False):
    """Grade the log of one run.  ``sampler``: kitti / allforone / baseline; ``score(x, y) -> scores`` is the score
    oracle (numpy in and out); ``noise(k)`` the noise injected at Langevin step k; the other arguments are what the
    test handed the sampler.  Raises LockstepError naming the first step that breaks a rule; prints one line per
    record and returns the per-record figures (dicts)."""
    sigmas = np.asarray(sigmas, dtype=F32)
    L = len(sigmas)
    ref, mask = np.asarray(ref, dtype=F32), np.asarray(mask)
    simultaneous = sampler != "baseline"

    # ---- schedule
    want = expected_schedule(sampler, L, n_steps_each, min_step, denoise)
    got = [(r["kind"], r["c"]) for r in records]
    for k, w in enumerate(want):
        g = got[k] if k < len(got) else ("nothing", None)
        if g != w:
            at = lambda e: e[0] + ("" if e[1] is None else f" at c={e[1]}")
            raise LockstepError(f"step {k}: the schedule (L={L}, n_steps_each={n_steps_each}, min_step={min_step}, "
                                f"denoise={denoise}) wants {at(w)}, recorded {at(g)}")
    _need(len(got) == len(want), f"step {len(want)}", f"{len(got) - len(want)} records past the end of the schedule")

    stats = []
    prev_x = None if x0 is None else np.asarray(x0, dtype=F32)
    last_lang = None
    n_lang = 0
    for k, r in enumerate(records):
        at = _label(k, r)
        st = dict(k=k, kind=r["kind"], c=r["c"], flagged=0, flagged_share=0.0, max_err=0.0)
        xb = r["x_before"]
        if r["kind"] == "merge":
            own = slice(r["o_begin"], r["o_begin"] + r["n_out"])
            if prev_x is not None:
                _need_bits(xb[own], prev_x, at, "x handed to the merge (against the step before)")
        elif prev_x is not None:
            _need_bits(xb, prev_x, at, "x handed to the step (against the step before)")

        if r["kind"] == "langevin":
            c = r["c"]
            want_step = S.step_size_of(step_lr, sigmas[c], sigmas[-1])
            _need(_f32_bits(r["step"]) == _f32_bits(want_step), at, f"step size {r['step']!r}, reference {want_step!r}")
            want_ns = F32(np.sqrt(F32(want_step * F32(2))))
            _need(_f32_bits(r["nscale"]) == _f32_bits(want_ns), at, f"noise scale {r['nscale']!r}, reference {want_ns!r}")
            _need(_f32_bits(r["grad_ref"]) == _f32_bits(grad_ref), at, f"grad_ref {r['grad_ref']!r}")
            _need(r["nan_to_num"] == simultaneous, at, f"nan_to_num {r['nan_to_num']}")
            _need(r["y"] is not None and (r["y"] == c).all(), at, "labels differ from the level")
            _need(r["absmax_in"] == 0, at, f"the absmax word was not zeroed before the step (0x{r['absmax_in']:08x}): "
                  "the device takes an atomic max into it")
            _need_bits(r["ref"], ref, at, "ref")
            _need(np.array_equal(r["mask"], mask), at, "mask differs")
            nz = np.asarray(noise(n_lang), dtype=F32)
            _need_bits(r["noise"], nz, at, f"noise (injected draw {n_lang})")
            if r["score_x"] is not None:
                _need_bits(r["score_x"], xb, at, "x the scores were computed on")
            ws = np.asarray(score(xb, r["y"]), dtype=F32)
            st["score_err"] = float(_rel_err(r["scores"], ws))
            _need(st["score_err"] <= SCORE_TOL, at, f"scores off by {st['score_err']:.3e} of max|ref| (> {SCORE_TOL})")
            g = S.nan_to_num(r["scores"]) if simultaneous else r["scores"]
            wx, wl = S.langevin_update(xb, g, ref, mask, nz, want_step, grad_ref)
            _need_bits(r["x_after"], wx, at, "x after the update")
            _need_bits(r["lik"], wl, at, "lik")
            ok, wa = _absmax_ok(r["absmax"], r["x_after"])
            _need(ok, at, f"absmax word 0x{r['absmax']:08x}, max|x[:, 0]| = {wa!r} (0x{_f32_bits(wa):08x})")
            last_lang = r
            n_lang += 1

        elif r["kind"] == "merge":
            c = r["c"]
            _need(_f32_bits(r["sigma"]) == _f32_bits(sigmas[c]), at, f"sigma {r['sigma']!r}, level's {sigmas[c]!r}")
            _need(r["setting"] == setting, at, f"setting {r['setting']}")
            want_al = allowance if sampler == "kitti" else (5 if setting >= 8 else 10)
            _need(r["allowance"] == want_al, at, f"allowance {r['allowance']}, reference {want_al}")
            want_cc = reference_cc(sampler, setting, cc0, c, L)
            _need(float(r["cc"]) == float(want_cc), at, f"cc {r['cc']!r}, reference {want_cc!r}")
            _need(r["absmax"] == last_lang["absmax"], at, f"absmax word 0x{r['absmax']:08x}, the Langevin step left "
                  f"0x{last_lang['absmax']:08x}")
            keeps = c in NEW_LEVELS or c == L - 1
            _need((r["new"] is not None) == keeps, at, f"new images {'missing' if keeps else 'passed'}")
            amax = np.array([r["absmax"]], np.uint32).view(F32)[0]
            if sampler == "kitti":
                wn, wx, fl = S.kitti_merge(xb, mask, sky, exist, toWorld, fromWorld, aB, r["sigma"], setting,
                                           r["allowance"], r["cc"], absmax=amax, flags=True)
            else:
                wn, wx, fl = S.allforone_merge(xb, mask, sky, exist, mods, aB, r["sigma"], setting, r["cc"],
                                               absmax=amax, flags=True)
            gn = wn[own] if r["new"] is None else r["new"]
            _need(gn.shape == wn[own].shape, at, f"new images have shape {gn.shape}")
            ok_px = ~np.broadcast_to(fl[own][:, None], wn[own].shape)
            st.update(flagged=int(fl[own].sum()), flagged_share=float(fl[own].mean()),
                      max_err=float(max(np.abs(r["x_after"][own] - wx[own])[ok_px].max(),
                                        np.abs(gn - wn[own])[ok_px].max())),
                      changed=int((_bits(r["x_after"]) != _bits(xb)).sum()),
                      zero_share=float((gn == 0).mean()), has_new=r["new"] is not None)
            try:
                _assert_merge_exact(gn, wn[own], r["x_after"][own], wx[own], fl[own], at)
            except LockstepError:
                raise
            except AssertionError as e:
                raise LockstepError(f"{at}: merge differs from the oracle outside the flagged pixels: {e}") from e
            rest = np.ones(xb.shape[0], bool)
            rest[own] = False
            _need_bits(r["x_after"][rest], xb[rest], at, "views outside the output range")

        elif r["kind"] == "denoise":
            _need(r["c"] == L - 1 and (r["y"] == L - 1).all(), at, "labels differ from the last level")
            _need_bits(r["score_x"], xb, at, "x the scores were computed on")
            _need_bits(r["lik"], last_lang["lik"], at, "lik (the reference's stale likelihood: the last Langevin step's)")
            want_a = F32(sigmas[-1]) ** 2
            _need(_f32_bits(r["a"]) == _f32_bits(want_a), at, f"a {r['a']!r}, reference {want_a!r}")
            _need(_f32_bits(r["b"]) == _f32_bits(grad_ref), at, f"b {r['b']!r}")
            ws = np.asarray(score(xb, r["y"]), dtype=F32)
            st["score_err"] = float(_rel_err(r["scores"], ws))
            _need(st["score_err"] <= SCORE_TOL, at, f"scores off by {st['score_err']:.3e} of max|ref| (> {SCORE_TOL})")
            wx = ((xb + want_a * r["scores"]) + F32(grad_ref) * r["lik"]).astype(F32)
            _need_bits(r["x_after"], wx, at, "x after the denoise")

        else:   # final
            _need_bits(r["ref"], ref, at, "ref")
            _need(np.array_equal(r["mask"], mask), at, "mask differs")
            _need(_f32_bits(r["b"]) == _f32_bits(grad_ref), at, f"b {r['b']!r}")
            wx = (xb + F32(grad_ref) * ((-mask).astype(F32) * (xb - ref))).astype(F32)
            _need_bits(r["x_after"], wx, at, "x after the final data consistency")

        prev_x = r["x_after"][own] if r["kind"] == "merge" else r["x_after"]
        print(f"lockstep {at}: " + ", ".join(f"{n} {st[n]:.3e}" if isinstance(st[n], float) else f"{n} {st[n]}"
                                             for n in st if n not in ("k", "kind", "c")))
        stats.append(st)

    # ---- returned lists
    if images is not None:
        imgs = [np.asarray(i) for i in images]
        if simultaneous:
            kept = [r for r in records if r["kind"] == "merge" and r["c"] == L - 1]
            sh = [r for r in records if r["kind"] == "merge" and r["c"] in NEW_LEVELS]
            _need(len(imgs) == len(kept) + 1, "returned images", f"{len(imgs)} images for {len(kept)} last-level merges")
            for i, r in enumerate(kept):
                _need_bits(imgs[i], r["new"], f"returned images[{i}]", "the new images of its merge")
            shl = [np.asarray(i) for i in (shared or [])]
            _need(len(shl) == len(sh), "returned shared images", f"{len(shl)} images for {len(sh)} kept merges")
            for i, r in enumerate(sh):
                _need_bits(shl[i], r["new"], f"returned shared[{i}]", "the new images of its merge")
        else:
            steps = [r for r in records if r["kind"] != "final"] if keep_all else \
                [r for r in records if r["kind"] == "denoise" or r is last_lang]
            _need(len(imgs) == len(steps) + 1, "returned images", f"{len(imgs)} images for {len(steps)} kept steps")
            for i, r in enumerate(steps):
                _need_bits(imgs[i], r["x_after"], f"returned images[{i}]", "x after its step")
        _need_bits(imgs[-1], records[-1]["x_after"], "returned images[-1]", "the last recorded x")
    return stats
