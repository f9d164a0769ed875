"""sdp_cloud_nn / sdp_cloud_nn_stats and their Python surface (sdp.pointcloud.nearest_neighbours, cloud_metrics)
against tests/cloud_nn_ref.py, the numpy brute force: nn_idx exactly equal and nn_d2 bit-equal on EVERY query,
at the smallest sizes where the kernels can still go wrong.  The sums of the stats are compared with the bound
of cloud_nn_ref.sum_bound (the worst case of any summation order; the addends themselves are bit-equal), the
counts and the maximum exactly.
"""
import numpy as np
import pytest
import torch

import cloud_nn_ref as NR

pytestmark = pytest.mark.gpu
DEV = "cuda"
INF = np.inf
_CACHE = {}


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a)).to(DEV)


def raw(q, t, R, cell, center=None):
    """The C entry on sentinel-filled outputs: (rc, d2, idx, info) as numpy after a sync."""
    from sdp import _lib
    L = _lib.lib()
    q, t = dev(np.asarray(q, dtype=np.float64)), dev(np.asarray(t, dtype=np.float64))
    nq, nt = q.shape[0], t.shape[0]
    nb = _lib.SZ()
    assert L.sdp_cloud_nn_workspace_size(nq, nt, _lib.C.byref(nb)) == 0
    ws = torch.empty(nb.value, dtype=torch.uint8, device=DEV)
    d2 = torch.full((max(nq, 1),), -7.0, dtype=torch.float64, device=DEV)
    idx = torch.full((max(nq, 1),), -7, dtype=torch.int32, device=DEV)
    info = torch.full((8,), -7, dtype=torch.int64, device=DEV)
    c = None if center is None else dev(np.asarray(center, dtype=np.float64))
    rc = L.sdp_cloud_nn(q.data_ptr() if nq else None, nq, q.shape[1], t.data_ptr() if nt else None, nt, t.shape[1],
                        float(R), float(cell), _lib.ptr(c), d2.data_ptr(), idx.data_ptr(), info.data_ptr(),
                        ws.data_ptr(), ws.numel(), _lib.stream())
    torch.cuda.synchronize()
    return rc, d2.cpu().numpy()[:nq], idx.cpu().numpy()[:nq], info.cpu().numpy()


def same_bits(d2, idx, ref):
    assert d2.dtype == np.float64 and idx.dtype == np.int32
    np.testing.assert_array_equal(idx, ref[1])
    np.testing.assert_array_equal(d2.view(np.int64), ref[0].view(np.int64))


def check(q, t, R, cell=None, center=None, ref=None, some=True):
    """nearest_neighbours against the brute force on every query; returns the reference."""
    from sdp.pointcloud import nearest_neighbours
    ref = NR.nearest(q, t, R) if ref is None else ref
    d2, idx = nearest_neighbours(dev(q), dev(t), R, cell=cell, center=None if center is None else dev(center))
    same_bits(d2.cpu().numpy(), idx.cpu().numpy(), ref)
    if some:   # the case means something: matched and unmatched queries both occur
        assert 0 < (ref[1] >= 0).sum() < len(ref[1])
    return ref


def cloud(n, seed, lo=-1.0, hi=1.0, stride=3):
    r = np.random.default_rng(seed)
    p = r.uniform(lo, hi, (n, stride))
    if stride == 4:
        p[:, 3] = r.uniform(0, 1e6, n)      # the fourth column is not a coordinate
    return p


@pytest.mark.parametrize("nq,nt,qs,ts", [(1, 63, 3, 3), (63, 1, 4, 3), (64, 65, 3, 4), (65, 257, 4, 4), (257, 64, 3, 3),
                                         (3 * 1024 + 17, 1, 3, 4), (1, 3 * 1024 + 17, 4, 3), (3 * 1024 + 17, 257, 3, 3),
                                         (257, 3 * 1024 + 17, 4, 4)])
def test_small_sizes_and_strides(nq, nt, qs, ts):
    q, t = cloud(nq, 10 + nq, -1.5, 1.5, stride=qs), cloud(nt, 20 + nt, stride=ts)
    R = 0.3 if nt > 1 else 1.2
    if nq == 1:
        q[0, :3] = t[nt // 2, :3] + 0.01
    ref = check(q, t, R, some=nq > 1)
    assert (ref[1] >= 0).any()
    rc, d2, idx, info = raw(q, t, R, R)
    assert rc == 0 and info[4] == nt and info[0] > 0 and info[6] == 0
    same_bits(d2, idx, ref)


def test_empty_clouds():
    from sdp.pointcloud import nearest_neighbours
    q, t = cloud(70, 1), cloud(5, 2)
    rc, d2, idx, info = raw(q, np.zeros((0, 3)), 0.5, 0.5)
    assert rc == 0 and (d2 == INF).all() and (idx == -1).all() and (info == 0).all()
    rc, d2, idx, info = raw(np.zeros((0, 4)), t, 0.5, 0.5)
    assert rc == 0 and len(d2) == 0 and (info == 0).all()
    d2, idx = nearest_neighbours(dev(q), dev(np.zeros((0, 3))), 0.5)
    assert d2.shape == (70,) and bool((d2 == INF).all()) and bool((idx == -1).all())
    d2, idx = nearest_neighbours(dev(np.zeros((0, 3))), dev(t), 0.5)
    assert d2.shape == (0,) and idx.shape == (0,) and idx.dtype == torch.int32
    # targets, but none of them finite
    t[:, 1] = np.nan
    rc, d2, idx, info = raw(q, t, 0.5, 0.5)
    assert rc == 0 and (d2 == INF).all() and (idx == -1).all() and info[0] == 0 and info[4] == 0


def test_all_targets_in_one_cell():
    r = np.random.default_rng(3)
    t = np.array([0.2, 0.2, 0.2]) + r.uniform(0, 0.1, (3000, 3))      # several sort tiles, one cell of 0.5
    q = r.uniform(-0.6, 1.0, (300, 3))
    check(q, t, 0.5)
    rc, _, _, info = raw(q, t, 0.5, 0.5, center=np.zeros(3))
    assert rc == 0 and info[0] == 1 and info[4] == 3000


def test_one_target_per_cell():
    r = np.random.default_rng(4)
    g = np.arange(-6, 6) * 0.25 + 0.125
    t = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3) + r.uniform(-0.1, 0.1, (12 ** 3, 3))
    t = t[r.permutation(len(t))]
    q = r.uniform(-1.9, 1.9, (500, 3))
    check(q, t, 0.25, some=False)
    rc, _, _, info = raw(q, t, 0.25, 0.25, center=np.zeros(3))
    assert rc == 0 and info[0] == 12 ** 3


def test_identical_points_and_duplicated_targets():
    r = np.random.default_rng(5)
    base = r.uniform(-1, 1, (200, 3))
    t = np.concatenate([base, base[::-1], base[50:70]])          # every point twice or three times
    ref = check(np.concatenate([base, r.uniform(-3, 3, (100, 3))]), t, 0.2)
    assert (ref[1][:200] == np.arange(200)).all() and (ref[0][:200] == 0).all()   # the lowest of the equal indices
    same = np.tile(np.array([[0.3, -0.2, 0.1]]), (1500, 1))
    ref = check(np.array([[0.3, -0.2, 0.1], [0.3, -0.2, 0.2], [5.0, 5, 5]]), same, 0.5)
    assert ref[1].tolist() == [0, 0, -1]


@pytest.mark.parametrize("R,cell,offs", [(0.5, 0.5, None), (0.5, 0.25, None), (0.625, 0.125, (0.375, 0.5)),
                                         (0.625, 0.625, (0.375, 0.5))])
def test_lattice_cell_faces_and_radius_edge(R, cell, offs):
    """Targets and queries on exact multiples of `cell` (R is one too: every one on a cell face), queries at distance exactly R,
    sqrt(2) R and R (1 +- 2^-52) along the axes, and on diagonals: (3/8, 4/8, 0) has length exactly 5/8."""
    k = np.arange(-2, 3) * 4.0
    t = np.stack(np.meshgrid(k, k, k, indexing="ij"), -1).reshape(-1, 3) * R          # isolated lattice points
    eye = np.concatenate([np.eye(3), -np.eye(3)])
    steps = [eye * R, eye * (R * (1 + 2.0 ** -52)), eye * (R * (1 - 2.0 ** -52)), eye * cell, np.zeros((1, 3))]
    diag = np.array([[1, 1, 0], [1, -1, 0], [0, 1, 1], [-1, 0, 1], [1, 0, -1], [1, 1, 1], [-1, -1, -1]], dtype=np.float64)
    steps += [diag * R, diag * (R / np.sqrt(2.0)), diag * (R / np.sqrt(3.0)), diag * (R / 2)]
    if offs:
        a, b = offs
        steps.append(np.array([[a, b, 0], [-a, b, 0], [0, a, -b], [b, 0, a], [-b, -a, 0], [0, -b, -a]]))
    d = np.concatenate(steps)
    q = (t[:, None, :] + d[None, :, :]).reshape(-1, 3)
    ref = check(q, t, R, cell=cell, center=np.zeros(3))
    r2 = np.float64(R) * np.float64(R)
    assert (ref[0] == r2).sum() >= 6 * len(t)            # the radius edge itself is hit, and counts as a match
    check(q, t, R, cell=cell, ref=ref)


def test_queries_outside_the_targets_box():
    r = np.random.default_rng(6)
    t = r.uniform(-1, 1, (800, 3))
    face = r.uniform(-1, 1, (300, 3))
    face[np.arange(300), r.integers(0, 3, 300)] = r.choice([-1.0, 1.0], 300) * r.uniform(1.0, 1.6, 300)
    far = r.uniform(-1, 1, (60, 3)) + r.choice([-1.0, 1.0], (60, 3)) * r.choice([3.0, 1e3, 1e9], (60, 1))
    huge = np.array([[1e30, 0, 0], [0, -1e30, 0], [1e30, 1e30, -1e30], [-1e30, 0.5, 0.5], [1e300, 0, 0], [0, 0, -1e300]])
    ref = check(np.concatenate([face, far, huge]), t, 0.5, cell=0.25)
    assert (ref[1][:300] >= 0).sum() > 30 and (ref[1][300:] == -1).all()
    # and targets that far apart: a coordinate beyond float32 must not drop out silently
    rc, d2, idx, info = raw(face, np.concatenate([t, [[1e300, 0, 0]]]), 0.5, 0.5)
    assert rc == 0 and info[0] == -1 and (d2 == -7).all() and (idx == -7).all()     # reported, nothing written


def test_non_finite_queries_and_targets():
    r = np.random.default_rng(7)
    q, t = r.uniform(-1, 1, (600, 4)), r.uniform(-1, 1, (700, 4))
    bad = [np.nan, INF, -INF]
    for k in range(60):
        q[r.integers(0, 600), r.integers(0, 3)] = bad[k % 3]
        t[r.integers(0, 700), r.integers(0, 3)] = bad[(k + 1) % 3]
    q[:, 3] = np.nan                                        # not a coordinate
    q[100, :3] = t[5, :3] = [0.1, 0.2, np.nan]              # NaN never equals NaN
    tfin = np.isfinite(t[:, :3]).all(1)
    q[101, :3] = t[np.nonzero(~tfin)[0][0], :3]
    ref = check(q, t, 0.3)
    assert (ref[1][~np.isfinite(q[:, :3]).all(1)] == -1).all() and tfin[ref[1][ref[1] >= 0]].all()
    rc, _, _, info = raw(q, t, 0.3, 0.3)
    assert rc == 0 and info[4] == tfin.sum()


def test_cell_sizes_give_identical_bits():
    q, t = cloud(1500, 8, -2.6, 2.6), cloud(4000, 9, -2, 2)
    R = 0.4
    ref = check(q, t, R)
    for cell in (R / 2, R / 3, R / 8):
        check(q, t, R, cell=cell, ref=ref)
        check(q, t, R, cell=cell, center=np.array([0.37, -1.91, 5.5]), ref=ref)
    rc, _, _, info = raw(q, t, R, R / 8)
    assert rc == 0 and info[5] == 9          # eight rings from cell = R / 8 and the one the slack adds


def test_cell_too_small_raises():
    from sdp.pointcloud import nearest_neighbours
    q, t = dev(cloud(10, 1)), dev(cloud(10, 2))
    with pytest.raises(RuntimeError, match="cell too small for max_dist"):
        nearest_neighbours(q, t, 0.9, cell=0.0999)
    with pytest.raises(ValueError):
        nearest_neighbours(q, t, 0.5, cell=0.6)
    with pytest.raises(ValueError):
        nearest_neighbours(q, t, 0.0)
    with pytest.raises(ValueError):
        nearest_neighbours(q.cpu(), t, 0.5)
    with pytest.raises(ValueError):
        nearest_neighbours(q[:, :2], t, 0.5)
    # float32 clouds are widened
    d2, idx = nearest_neighbours(q.float(), t.float(), 0.5)
    same_bits(d2.cpu().numpy(), idx.cpu().numpy(), NR.nearest(q.float().cpu().numpy(), t.float().cpu().numpy(), 0.5))


def test_shifted_cloud_exercises_the_slack():
    """At (1e5, -2e5, 3e3) the float32 ulp is 0.016 m: with center = zeros the float32 cell of a point is off by
    up to that, and the slack (0.14 m here) must cover it."""
    r = np.random.default_rng(11)
    shift = np.array([1e5, -2e5, 3e3])
    t = r.uniform(-5, 5, (6000, 3)) + shift
    q = r.uniform(-5.5, 5.5, (3000, 3)) + shift
    ref = check(q, t, 0.5, cell=0.25)                       # center=None: the midpoint of the targets
    check(q, t, 0.5, cell=0.25, center=np.zeros(3), ref=ref)
    # K = ceil((R + slack) / cell): 0.5 + 0.143 at the far centre, 0.5 + 4e-6 at the near one
    ref2 = NR.nearest(q[:500], t, 0.5)
    for center, rings in ((np.zeros(3), 4), (shift, 3)):
        rc, d2, idx, info = raw(q[:500], t, 0.5, 0.2, center=center)
        assert rc == 0 and info[5] == rings
        same_bits(d2, idx, ref2)
    # the same cloud with cell = R / 8 at that distance from the centre: the slack is beyond one ring
    from sdp.pointcloud import nearest_neighbours
    with pytest.raises(RuntimeError, match="too small for max_dist"):
        nearest_neighbours(dev(q), dev(t), 0.5, cell=0.0625, center=dev(np.zeros(3)))


def test_origin_above_the_lower_bound_scans_all_targets():
    """org = floor(lo * fl(1/c)) * c in float32 can land one rounding above lo; then the lowest cell index of the
    grid wraps, the keys are useless, and the entry falls back to scanning every target (info[6] = 1): the same bits."""
    from sdp.pointcloud import nearest_neighbours
    F = np.float32
    c, lo = F(0.2), F(458.19998)
    assert F(np.floor(lo * (F(1) / c))) * c > lo           # the premise, in the grid's own arithmetic
    r = np.random.default_rng(21)
    t = np.array([float(lo), 0.0, 0.0]) + r.uniform(0, 3, (700, 3))
    t[0] = [float(lo), 1.0, 1.0]
    q = np.array([float(lo) - 0.2, -0.2, -0.2]) + r.uniform(0, 3.4, (400, 3))
    ref = NR.nearest(q, t, 0.4)
    assert 0 < (ref[1] >= 0).sum() < 400
    rc, d2, idx, info = raw(q, t, 0.4, 0.2, center=np.zeros(3))
    assert rc == 0 and info[6] == 1 and info[4] == 700
    same_bits(d2, idx, ref)
    with pytest.warns(RuntimeWarning, match="scanned all targets"):
        d2, idx = nearest_neighbours(dev(q), dev(t), 0.4, cell=0.2, center=dev(np.zeros(3)))
    same_bits(d2.cpu().numpy(), idx.cpu().numpy(), ref)
    rc, d2, idx, info = raw(q, t, 0.4, 0.25, center=np.zeros(3))      # a power-of-two cell: no such rounding
    assert rc == 0 and info[6] == 0
    same_bits(d2, idx, ref)


def test_non_finite_center_raises():
    from sdp.pointcloud import nearest_neighbours
    q, t = dev(cloud(50, 1)), dev(cloud(60, 2))
    for bad in ([0.0, np.nan, 0.0], [np.inf, 0.0, 0.0]):
        with pytest.raises(ValueError, match="center must be finite"):
            nearest_neighbours(q, t, 0.5, center=bad)


def test_grid_too_large_raises():
    from sdp.pointcloud import nearest_neighbours
    t = np.array([[0.0, 0, 0], [1e6, 1e6, 1e6]])
    q = cloud(100, 3)
    with pytest.raises(RuntimeError, match=r"exceeds 2\^40 cells"):
        nearest_neighbours(dev(q), dev(t), 0.5, cell=0.0625)
    rc, d2, idx, info = raw(q, t, 0.5, 0.0625)
    assert rc == 0 and info[0] == -1 and (info[1:4] > 9e6).all() and (d2 == -7).all() and (idx == -7).all()


def realistic():
    """Two fused clouds of 3 procedural views of 64 x 256: the scene, and the scene with range noise."""
    if "real" not in _CACHE:
        from sdp import synthetic
        from sdp.pointcloud import fuse_views
        sc = synthetic.scene_views(3, 64, 256, seed=77)
        x = torch.from_numpy(sc["ref"]).to(DEV)
        keep = torch.from_numpy(sc["sky"]).reshape(3, 64, 256).to(DEV)
        poses = torch.from_numpy(sc["toWorld"]).to(DEV)
        g = torch.Generator(device="cpu").manual_seed(5)
        noise = (torch.rand(x.shape, generator=g) - 0.5).to(DEV) * 0.01
        a = fuse_views((x + noise).clamp(0, 1), poses=poses, keep=keep).cpu().numpy()
        b = fuse_views(x, poses=poses, keep=keep).cpu().numpy()
        ab, ba = NR.nearest(a, b, 0.5), NR.nearest(b, a, 0.5)
        _CACHE["real"] = (a, b, ab, ba)
    return _CACHE["real"]


def test_realistic_pair():
    a, b, ab, ba = realistic()
    assert len(a) > 10000 and len(b) > 10000 and a.shape[1] == 4
    check(a, b, 0.5, ref=ab, some=False)
    check(b, a, 0.5, cell=0.125, ref=ba, some=False)
    assert (ab[1] >= 0).sum() > 5000 and (ba[1] >= 0).sum() > 5000


def test_second_scan_iteration():
    """1,048,876 targets: 4,098 chunks, 262,400 digit counts and the segment heads each exceed one iteration of
    the sort's single-workgroup scans."""
    r = np.random.default_rng(12)
    n = 1_048_876
    t = r.uniform([-20, -20, -5], [20, 20, 5], (n, 3))
    q = r.uniform([-20.2, -20.2, -5.2], [20.2, 20.2, 5.2], (256, 3))
    q[:8] = t[::131101][:8]
    ref = check(q, t, 0.25, some=False)
    assert (ref[1][:8] == np.arange(8) * 131101).all() and (ref[1] >= 0).sum() > 200


def test_two_calls_are_bit_identical():
    a, b, _, _ = realistic()
    r1, r2 = raw(a, b, 0.5, 0.25), raw(a, b, 0.5, 0.25)
    assert r1[0] == 0 and r2[0] == 0
    for x, y in zip(r1[1:], r2[1:]):
        assert x.tobytes() == y.tobytes()
    from sdp.pointcloud import nearest_neighbour_stats
    d2 = dev(r1[1])
    s1 = nearest_neighbour_stats(d2, dev(a), (0.1, 0.2, 0.5), 0.5).cpu().numpy()
    s2 = nearest_neighbour_stats(d2, dev(a), (0.1, 0.2, 0.5), 0.5).cpu().numpy()
    assert s1.tobytes() == s2.tobytes()


def check_stats(d2, q, thr, R):
    from sdp.pointcloud import nearest_neighbour_stats
    got = nearest_neighbour_stats(dev(d2), dev(q), thr, R).cpu().numpy()
    ref = NR.stats(d2, q, thr)
    assert got.dtype == np.float64 and got.shape == (5 + len(thr),)
    np.testing.assert_array_equal(got[[0, 1, 4]], ref[[0, 1, 4]])
    np.testing.assert_array_equal(got[5:], ref[5:])
    n = int(ref[1])
    for k in (2, 3):
        assert abs(got[k] - ref[k]) <= NR.sum_bound(n, ref[k])
    return got, ref


@pytest.mark.parametrize("n", [1, 255, 256, 257, 3 * 1024 + 17, 70001])
def test_stats_sizes(n):
    r = np.random.default_rng(n)
    q = r.uniform(-1, 1, (n, 3 + n % 2))
    d2 = r.uniform(0, 0.25, n)
    d2[r.uniform(size=n) < 0.2] = INF
    d2[r.integers(0, n, 3)] = [0.01, 0.04, 0.25]               # on the thresholds' squares
    bad = r.uniform(size=n) < 0.1
    q[bad, 1] = np.nan
    d2[bad] = INF
    got, ref = check_stats(d2, q, (0.1, 0.2, 0.5), 0.5)
    assert ref[0] == (~bad).sum()
    check_stats(d2, q, (), 0.5)
    check_stats(d2, q, (0.5, 0.4, 0.3, 0.2, 0.1, 0.05, 0.01, 0.0), 0.5)


def test_stats_edge_cases():
    from sdp.pointcloud import nearest_neighbour_stats
    q = cloud(300, 1)
    got, _ = check_stats(np.full(300, INF), q, (0.1,), 0.5)
    assert got.tolist() == [300.0, 0.0, 0.0, 0.0, 0.0, 0.0]
    got = nearest_neighbour_stats(dev(np.zeros(0)), dev(np.zeros((0, 3))), (0.1, 0.2), 0.5).cpu().numpy()
    assert got.tolist() == [0.0] * 7
    with pytest.raises(RuntimeError, match="threshold"):
        nearest_neighbour_stats(dev(np.zeros(300)), dev(q), (0.1, 0.5000001), 0.5)
    with pytest.raises(RuntimeError):
        nearest_neighbour_stats(dev(np.zeros(300)), dev(q), [0.1] * 9, 0.5)


def test_cloud_metrics_of_a_cloud_with_itself():
    from sdp.pointcloud import cloud_metrics, nearest_neighbours
    a = dev(cloud(5000, 13, -3, 3, stride=4))
    d2, idx = nearest_neighbours(a, a, 0.5)
    assert torch.equal(idx, torch.arange(5000, dtype=torch.int32, device=DEV)) and bool((d2 == 0).all())
    m = cloud_metrics(a, a, 0.5)
    assert m["chamfer"] == 0.0 and m["precision"] == m["recall"] == m["fscore"] == [1.0, 1.0, 1.0]
    assert m["ab"] == m["ba"] == {"n": 5000, "matched": 5000, "mean": 0.0, "rms": 0.0, "max": 0.0, "within": [5000] * 3}


def test_cloud_metrics_on_the_realistic_pair():
    from sdp.pointcloud import cloud_metrics
    a, b, ab, ba = realistic()
    thr = (0.05, 0.2, 0.5)
    m = cloud_metrics(dev(a), dev(b), 0.5, thresholds=thr, cell=0.25)
    ref = NR.metrics(NR.stats(ab[0], a, thr), NR.stats(ba[0], b, thr), thr)
    for d in ("ab", "ba"):
        for k in ("n", "matched", "max", "within"):
            assert m[d][k] == ref[d][k]
        rel = (ref[d]["matched"] + 4) * 2.0 ** -53       # the sum's bound, and the division and square root
        assert m[d]["mean"] == pytest.approx(ref[d]["mean"], rel=rel, abs=0)
        assert m[d]["rms"] == pytest.approx(ref[d]["rms"], rel=rel, abs=0)
        assert 0 < ref[d]["matched"] <= ref[d]["n"] and ref[d]["within"][0] < ref[d]["within"][2]
    assert m["chamfer"] == pytest.approx(ref["chamfer"], rel=(max(len(a), len(b)) + 4) * 2.0 ** -53, abs=0)
    assert m["precision"] == ref["precision"] and m["recall"] == ref["recall"] and m["fscore"] == ref["fscore"]
    assert 0 < m["fscore"][0] < m["fscore"][2] <= 1
    with pytest.raises(ValueError):
        cloud_metrics(dev(a), dev(b), 0.5, thresholds=(0.6,))
    empty = cloud_metrics(dev(a), dev(np.zeros((0, 3))), 0.5)
    assert np.isnan(empty["chamfer"]) and empty["fscore"] == [0.0] * 3 and empty["ab"]["matched"] == 0


def test_stage_events_hook():
    from sdp import _lib
    L = _lib.lib()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
    for e in ev:
        e.record()
    torch.cuda.synchronize()
    assert L.sdp_cloud_nn_stage_events((_lib.P * 3)(*[e.cuda_event for e in ev])) == 0
    try:
        a, b, ab, _ = realistic()
        rc, d2, idx, _ = raw(a, b, 0.5, 0.5)
    finally:
        assert L.sdp_cloud_nn_stage_events(None) == 0
    assert rc == 0
    same_bits(d2, idx, ab)
    dt = [ev[i].elapsed_time(ev[i + 1]) for i in range(2)]
    assert all(t >= 0 for t in dt) and sum(dt) > 0
    assert L.sdp_cloud_nn_stage_events((_lib.P * 3)(ev[0].cuda_event, None, ev[1].cuda_event)) < 0
