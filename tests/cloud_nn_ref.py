"""numpy brute force of the semantics of sdp_cloud_nn / sdp_cloud_nn_stats (include/sdp.h): the reference the
GPU tests compare bit for bit.

  d2(i,j) = ((qx-tx)*(qx-tx) + (qy-ty)*(qy-ty)) + (qz-tz)*(qz-tz) in float64, one rounding per operation
            (numpy evaluates elementwise, so nothing is fused);
  a target with a non-finite coordinate is never a neighbour; a query with one is unmatched;
  query i matches argmin_j d2(i,j) over d2 <= R*R (the rounded product), np.argmin's first minimum = the
  lowest index among equals; unmatched: d2 = +inf, index = -1.
"""
import math

import numpy as np


def _brute(qq, tt, r2):
    """All pairs of finite queries qq [a,3] and finite targets tt [b,3]: (best d2 or +inf, position in tt)."""
    with np.errstate(over="ignore", invalid="ignore"):
        dx = qq[:, 0:1] - tt[None, :, 0]
        dy = qq[:, 1:2] - tt[None, :, 1]
        dz = qq[:, 2:3] - tt[None, :, 2]
        d2 = (dx * dx + dy * dy) + dz * dz
        d2 = np.where(d2 <= r2, d2, np.inf)
    j = np.argmin(d2, axis=1)
    return d2[np.arange(len(j)), j], j


def nearest(q, t, max_dist, chunk=32, slab=True):
    """q [nq,>=3], t [nt,>=3] float64 -> (d2 float64 [nq], index int32 [nq]).

    Brute force over all pairs, chunked over the queries.  With slab=True the queries are taken in order of
    their x and a chunk is compared only with the targets whose x lies within 1.001 * max_dist of the chunk's
    x-range -- every other target has |dx| > max_dist and cannot match -- kept in ascending target index so
    that argmin's first minimum is still the lowest index.  slab=False compares every chunk with every target;
    tests/test_cloud_nn_ref_cpu.py holds the two equal."""
    q = np.asarray(q, dtype=np.float64)[:, :3]
    t = np.asarray(t, dtype=np.float64)[:, :3]
    nq, nt = len(q), len(t)
    d2o = np.full(nq, np.inf)
    ido = np.full(nq, -1, dtype=np.int32)
    if nq == 0 or nt == 0:
        return d2o, ido
    r2 = np.float64(max_dist) * np.float64(max_dist)
    tf = np.nonzero(np.isfinite(t).all(1))[0]
    qi = np.nonzero(np.isfinite(q).all(1))[0]
    if slab:
        qi = qi[np.argsort(q[qi, 0], kind="stable")]
    tx = t[tf, 0]
    margin = 1.001 * float(max_dist)
    for s in range(0, len(qi), chunk):
        rows = qi[s:s + chunk]
        cand = tf
        if slab:
            cand = tf[(tx >= q[rows, 0].min() - margin) & (tx <= q[rows, 0].max() + margin)]
        if len(cand) == 0:
            continue
        tt = t[cand]
        step = max(1, (1 << 23) // len(cand))
        for u in range(0, len(rows), step):
            best, j = _brute(q[rows[u:u + step]], tt, r2)
            ok = np.isfinite(best)
            d2o[rows[u:u + step]] = best
            ido[rows[u:u + step]] = np.where(ok, cand[j], -1)
    return d2o, ido


def stats(d2, q, thresholds):
    """[n_finite, n_matched, sum_d, sum_d2, max_d, cnt_k...] of one direction; the sums with math.fsum."""
    d2 = np.asarray(d2, dtype=np.float64)
    q = np.asarray(q, dtype=np.float64)[:, :3]
    m = d2[d2 < np.inf]
    d = np.sqrt(m)
    out = [float(np.isfinite(q).all(1).sum()), float(len(m)), math.fsum(d), math.fsum(m), float(d.max()) if len(m) else 0.0]
    for tau in thresholds:
        tau = np.float64(tau)
        out.append(float((m <= tau * tau).sum()))
    return np.array(out, dtype=np.float64)


def sum_bound(n, fsum):
    """The worst case of any float64 summation order of n non-negative addends against their exact sum
    (n - 1 additions, each within 2^-53 relative of a partial sum <= the total; the last unit covers fsum's own
    rounding): n * 2^-53 * fsum."""
    return n * 2.0 ** -53 * fsum


def metrics(ab, ba, thresholds):
    """The formulae of sdp.pointcloud.cloud_metrics on two stat rows, written out independently."""
    out = {}
    for name, r in (("ab", ab), ("ba", ba)):
        n, k = r[0], r[1]
        out[name] = {"n": int(n), "matched": int(k), "mean": r[2] / k if k else float("nan"),
                     "rms": math.sqrt(r[3] / k) if k else float("nan"), "max": float(r[4]),
                     "within": [int(v) for v in r[5:]]}
    out["chamfer"] = out["ab"]["mean"] + out["ba"]["mean"]
    out["precision"] = [w / ab[0] if ab[0] else 0.0 for w in ab[5:]]
    out["recall"] = [w / ba[0] if ba[0] else 0.0 for w in ba[5:]]
    out["fscore"] = [2 * p * r / (p + r) if p + r > 0 else 0.0 for p, r in zip(out["precision"], out["recall"])]
    return out
