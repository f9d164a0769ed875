"""tests/voxel_ref.py, the restatement the device voxel grid is graded against (tests/test_gpu_voxel_grid.py),
pinned on the CPU to the host C++ (sdp.grid_subsampling.compute, itself bit-equal to the reference's
build) and to oracle.grid_subsampling_ref.subsample.

The host returns its voxels in hash order, voxel_ref in ascending key, so the rows are matched by
lexsorted barycentre after asserting that the barycentres of a side are distinct.  Points and features
are then bit-equal; on an untied voxel the labels are equal, on a tied one the host's label (first
maximum in hash order) is one of the labels with the most votes while voxel_ref gives the smallest of
them; both kinds of voxel must occur, and no voxel is left out."""
import numpy as np
import pytest

import voxel_ref as VR
from oracle import grid_subsampling_ref as G
from sdp import grid_subsampling as GS


def _cloud(seed, n, fdim, ldim):
    r = np.random.default_rng(seed)
    p = np.concatenate([r.uniform(-4, 4, (n // 2, 3)), r.normal(0, 0.03, (n - n // 2, 3)) + r.uniform(-4, 4, (40, 3))[
        r.integers(0, 40, n - n // 2)]]).astype(np.float32)
    p = p[r.permutation(n)]
    f = r.normal(0, 1, (n, fdim)).astype(np.float32) if fdim else None
    c = None
    if ldim:
        c = np.stack([r.integers(0, 4, n), r.integers(-3, 3, n)][:ldim], 1).astype(np.int32)
    return p, f, c


def _rows(pts):
    order = np.lexsort((pts[:, 2], pts[:, 1], pts[:, 0]))
    s = pts[order]
    assert (np.abs(np.diff(s, axis=0)).max(1) > 0).all(), "two voxels share a barycentre: rows cannot be matched"
    return order


CASES = [(1, 6000, 3, 2, 0.5), (2, 6000, 1, 1, 0.05), (3, 4000, 0, 2, 1.0), (4, 4000, 3, 0, 0.25), (5, 3000, 0, 0, 0.1),
         (6, 1, 1, 1, 0.1), (7, 500, 1, 1, 100.0)]


@pytest.mark.parametrize("seed,n,fdim,ldim,dl", CASES)
def test_matches_the_host_implementation(seed, n, fdim, ldim, dl):
    p, f, c = _cloud(seed, n, fdim, ldim)
    got = GS.compute(p, features=f, classes=c, sampleDl=dl)
    got = list(got if isinstance(got, tuple) else (got,))
    hp = got.pop(0)
    hf = got.pop(0) if fdim else None
    hc = got.pop(0) if ldim else None
    r = VR.subsample(p, f, c, dl)
    m = int(r["info"][0])
    assert m == len(hp) == len(r["points"]) and r["info"][4] == n
    assert (np.diff(r["keys"]) > 0).all() and r["counts"].sum() == n
    a, b = _rows(hp), _rows(r["points"])
    np.testing.assert_array_equal(hp[a].view(np.int32), r["points"][b].view(np.int32))
    if fdim:
        np.testing.assert_array_equal(hf[a].view(np.int32), r["features"][b].view(np.int32))
    if ldim:
        assert hc.shape == r["classes"].shape == (m, ldim)
        tied = r["tied"][b]
        np.testing.assert_array_equal(hc[a][~tied], r["classes"][b][~tied])
        for j in range(ldim):
            t = np.flatnonzero(tied[:, j])
            assert np.isin(VR.label_code(b[t], hc[a][t, j]), r["max_codes"][j]).all(), "host label is not a maximum"
            assert (r["classes"][b][t, j] <= hc[a][t, j]).all(), "the restatement keeps the smallest maximum"
        if n >= 3000:
            assert tied.any() and (~tied).any()


@pytest.mark.parametrize("seed,n,fdim,ldim,dl", [(11, 1500, 2, 2, 0.5), (12, 1200, 1, 1, 0.07)])
def test_matches_the_oracle(seed, n, fdim, ldim, dl):
    p, f, c = _cloud(seed, n, fdim, ldim)
    cells = G.subsample(p, f, c, dl)
    r = VR.subsample(p, f, c, dl)
    assert sorted(cells) == r["keys"].tolist()
    n_tied = 0
    for i, k in enumerate(r["keys"].tolist()):
        pt, ff, hist, votes = cells[k]
        assert np.array_equal(pt.view(np.int32), r["points"][i].view(np.int32))
        assert np.array_equal(ff.view(np.int32), r["features"][i].view(np.int32))
        assert sum(hist[0].values()) == r["counts"][i]
        for j in range(ldim):
            top = sorted(lab for lab, v in hist[j].items() if v == votes[j])
            assert r["classes"][i, j] == top[0] and r["tied"][i, j] == (len(top) > 1)
            n_tied += len(top) > 1
    assert n_tied > 0


def test_non_finite_points_are_skipped_and_rows_map_back():
    p, f, c = _cloud(21, 2000, 2, 1)
    bad = [0, 7, 1000, 1999]
    p[bad] = [[np.nan, 0, 0], [0, np.inf, 0], [0, 0, -np.inf], [np.nan, np.nan, np.nan]]
    keep = np.setdiff1d(np.arange(2000), bad)
    r = VR.subsample(p, f, c, 0.3)
    q = VR.subsample(p[keep], f[keep], c[keep], 0.3)
    for name in ("points", "features", "classes", "keys", "counts"):
        np.testing.assert_array_equal(r[name], q[name])
    assert (r["inverse"][bad] == -1).all() and r["info"][4] == 1996
    np.testing.assert_array_equal(r["inverse"][keep], q["inverse"])
    np.testing.assert_array_equal(r["order"], keep[q["order"]])
    np.testing.assert_array_equal(np.bincount(r["inverse"][keep], minlength=len(r["keys"])), r["counts"])
    assert VR.subsample(np.full((3, 3), np.nan, np.float32), dl=0.1)["info"].tolist() == [0, 0, 0, 0, 0]


def test_key_bits_and_the_cell_limit():
    p = np.array([[-50, -50, -3], [50, 50, 17]], np.float32)
    assert VR.subsample(p, dl=50)["key_bits"] == 5
    r = VR.subsample(p, dl=0.001)
    assert r["key_bits"] == 48 and r["info"][0] == -1 and "points" not in r
