"""tests/cloud_nn_ref.py, the brute force the GPU tests trust, against an independent implementation
(scipy.spatial.cKDTree) on random clouds, and against literal values on hand-made tie / duplicate / NaN cases."""
import numpy as np
import pytest
from scipy.spatial import cKDTree

import cloud_nn_ref as NR

INF = np.inf


@pytest.mark.parametrize("nq,nt,R,seed", [(500, 700, 0.5, 0), (1000, 300, 0.2, 1), (64, 2000, 1.0, 2)])
def test_reference_equals_kdtree(nq, nt, R, seed):
    rng = np.random.default_rng(seed)
    q = rng.uniform(-2, 2, (nq, 3))
    t = rng.uniform(-2, 2, (nt, 3))
    d2, idx = NR.nearest(q, t, R, chunk=97, slab=bool(seed % 2))
    # guard, from the reference alone: no d2 of any pair within 1e-12 relative of R*R, so the matched sets of two
    # arithmetic orders cannot differ; and no ties (random doubles)
    r2 = np.float64(R) * np.float64(R)
    diff = q[:, None, :] - t[None, :, :]
    alld2 = (diff[..., 0] * diff[..., 0] + diff[..., 1] * diff[..., 1]) + diff[..., 2] * diff[..., 2]
    assert not (np.abs(alld2 - r2) <= 1e-12 * r2).any()
    dist, j = cKDTree(t).query(q, k=1, distance_upper_bound=R)
    matched = np.isfinite(dist)
    assert 0 < matched.sum() < nq or nq < 100
    np.testing.assert_array_equal(idx >= 0, matched)
    np.testing.assert_array_equal(idx[matched], j[matched])
    assert (j[~matched] == nt).all() and (d2[~matched] == INF).all()
    d = np.sqrt(d2[matched])
    assert (np.abs(d - dist[matched]) <= 4 * np.spacing(d)).all()
    # d2 is the written-out expression on the chosen pair
    e = q[matched] - t[idx[matched]]
    np.testing.assert_array_equal(d2[matched], (e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1]) + e[:, 2] * e[:, 2])


def test_ties_duplicates_and_non_finite():
    t = np.array([[1.0, 0, 0], [-1.0, 0, 0], [1.0, 0, 0], [np.nan, 0, 0], [0, INF, 0], [0, 0, 0.25], [0, 0, 0.25]])
    q = np.array([[0.0, 0, 0],        # nearest: the duplicates 5, 6 -> 5
                  [0.0, 0, -5.0],     # nothing within 2
                  [0.0, 2.0, 0],      # 0, 1, 2 at d2 = 5 > 4; 5 at 4 + 1/16 > 4: unmatched
                  [3.0, 0, 0],        # 0 and 2 at exactly R: tie -> 0
                  [np.nan, 0, 0], [0, -INF, 0],
                  [0.0, 0.0, -1.0]])  # 0, 1, 2 at d2 = 2; 5 at 1.5625 -> 5
    d2, idx = NR.nearest(q, t, 2.0)
    np.testing.assert_array_equal(idx, np.array([5, -1, -1, 0, -1, -1, 5], dtype=np.int32))
    np.testing.assert_array_equal(d2, np.array([0.0625, INF, INF, 4.0, INF, INF, 1.5625]))
    assert idx.dtype == np.int32 and d2.dtype == np.float64
    # equal d2 from different points: the lowest index
    d2, idx = NR.nearest(np.zeros((1, 3)), np.array([[0, 1.0, 0], [1.0, 0, 0], [0, 0, -1.0]]), 1.0)
    assert idx[0] == 0 and d2[0] == 1.0
    # the radius edge is the rounded product R*R
    R = 0.1
    x = np.sqrt(np.float64(R) * np.float64(R))
    for xx, hit in ((x, True), (np.nextafter(x, 1.0) + 1e-17, False)):
        d2, idx = NR.nearest(np.array([[xx, 0.0, 0.0]]), np.zeros((1, 3)), R)
        assert (idx[0] == 0) == (xx * xx <= np.float64(R) * np.float64(R)) == hit


def test_slab_pruning_changes_nothing():
    rng = np.random.default_rng(7)
    t = np.round(rng.uniform(-3, 3, (3000, 3)) * 4) / 4          # a lattice: many exact ties and duplicates
    q = np.round(rng.uniform(-4, 4, (1500, 3)) * 4) / 4
    q[5] = [np.nan, 0, 0]
    q[6] = [1e30, 0, 0]
    t[7] = [0, np.inf, 0]
    for R in (0.25, 0.5, 1.0):
        a, b = NR.nearest(q, t, R), NR.nearest(q, t, R, chunk=200, slab=False)
        np.testing.assert_array_equal(a[0], b[0])
        np.testing.assert_array_equal(a[1], b[1])
        assert (a[1] >= 0).sum() > 100


def test_empty_and_stride():
    d2, idx = NR.nearest(np.zeros((3, 4)), np.zeros((0, 3)), 1.0)
    assert (d2 == INF).all() and (idx == -1).all()
    d2, idx = NR.nearest(np.zeros((0, 3)), np.zeros((5, 4)), 1.0)
    assert d2.shape == (0,) and idx.shape == (0,)
    t = np.array([[0, 0, 0, 99.0], [1, 1, 1, -99.0]])
    d2, idx = NR.nearest(np.array([[0.9, 1, 1, 1e9]]), t, 1.0)
    assert idx[0] == 1 and d2[0] == (1 - 0.9) * (1 - 0.9)


def test_stats_literal():
    q = np.array([[0.0, 0, 0], [1, 1, 1], [np.nan, 0, 0], [2, 2, 2], [3, 3, 3]])
    d2 = np.array([0.25, INF, INF, 0.04, 0.0])
    s = NR.stats(d2, q, (0.1, 0.2, 0.5))
    np.testing.assert_array_equal(s[[0, 1]], [4.0, 3.0])
    assert s[2] == 0.5 + np.sqrt(0.04) and s[3] == 0.25 + 0.04 and s[4] == 0.5
    np.testing.assert_array_equal(s[5:], [1.0, 1.0 + (0.04 <= np.float64(0.2) * np.float64(0.2)), 3.0])
    s = NR.stats(np.array([INF]), q[:1], (0.5,))
    np.testing.assert_array_equal(s, [1.0, 0.0, 0.0, 0.0, 0.0, 0.0])
    m = NR.metrics(NR.stats(d2, q, (0.5,)), NR.stats(np.array([0.0, 0.0]), q[:2], (0.5,)), (0.5,))
    assert m["precision"] == [0.75] and m["recall"] == [1.0] and m["fscore"] == [2 * 0.75 / 1.75]
    assert m["chamfer"] == (0.5 + 0.2 + 0.0) / 3 + 0.0
