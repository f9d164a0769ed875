"""sdp_voxel_grid (csrc/voxel_grid.hip) on the GPU against tests/voxel_ref.py (pinned on the CPU to the host
C++ in tests/test_voxel_ref_cpu.py): every row and every bit.  Points and features are compared as int32
views; keys, counts, classes, inverse and info are exact; `order` is exactly the stable argsort.  Every
raw call fills its outputs with sentinels first and checks that rows past m were left alone.

Small cases: n = 1, 2, 63, 64, 65, TILE-1, TILE, TILE+1, 3*TILE+17 (TILE = VOXEL_SORT_TILE, read from the
kernel source) with no features / classes, with fdim 1 and ldim 1, and with fdim 3 and ldim 2 (negative
labels); all points in one voxel; all points identical; every point in a voxel of its own; stride 4; planted
NaN and +-inf points (the first and the last among them); a cloud whose only finite point is one point.

The scene: n = 200,000 from a fixed seed -- 55 % uniform in [-50,50]^2 x [-3,17], 40 % in 2000 Gaussian
clusters of sigma 0.03, 5000 points inside one 0.01 m voxel, the rest exact duplicates, the two box
corners planted, shuffled; labels uniform in [0,20) and [-3,3).  dl = 50, 5, 0.5, 0.05, 0.01 give keys of
5, 12, 21, 31, 38 bits, i.e. 1 to 5 active sort passes (asserted from voxel_ref alone); dl = 0.001 (48 bits)
must report info[0] = -1 and write nothing else.

The scan case takes its size from the kernel's constants so that every single-workgroup scan (digit counts,
finite-point chunks, segment-head chunks) needs a second iteration: n = VOXEL_CHUNK * (scan iteration) + 300,
1.05 M points, under 60 MB of inputs and workspace.
"""
import os
import re

import numpy as np
import pytest
import torch

import voxel_ref as VR
from conftest import PKG_DIR

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _constants():
    src = open(os.path.join(PKG_DIR, "csrc", "voxel_grid.hip")).read()
    get = lambda name: int(re.search(r"constexpr int %s = (\d+);" % name, src).group(1))
    return get("VOXEL_SORT_TILE"), get("VOXEL_CHUNK"), get("VOXEL_SCAN_THREADS") * get("VOXEL_SCAN_PER_THREAD")


TILE, CHUNK, SCAN = _constants()
N_SCAN = CHUNK * SCAN + 300          # the first sizes whose chunk counts exceed one scan iteration
assert -(-N_SCAN // CHUNK) > SCAN and 256 * -(-N_SCAN // TILE) > SCAN and N_SCAN * (20 + 34) < 150e6
SIZES = [1, 2, 63, 64, 65, TILE - 1, TILE, TILE + 1, 3 * TILE + 17]
SCENE_DL = {50.0: 5, 5.0: 12, 0.5: 21, 0.05: 31, 0.01: 38}
_CACHE = {}


def dev(a, dtype=None):
    return None if a is None else torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).to(DEV)


def attrs(r, n, fdim, ldim):
    """Features [n,fdim] and labels [n,ldim] (column 0 in [0,4) or [0,20), column 1 negative too)."""
    f = r.normal(0, 1, (n, fdim)).astype(np.float32) if fdim else None
    c = np.stack([r.integers(0, 4, n), r.integers(-3, 3, n)][:ldim], 1).astype(np.int32) if ldim else None
    return f, c


def small_cloud(n, seed=0):
    r = np.random.default_rng(1000 + n + seed)
    p = r.uniform(-1, 1, (n, 3)).astype(np.float32)
    if n > 4:
        p[n // 2] = p[1]                     # an exact duplicate
    return p


def scene():
    if "scene" in _CACHE:
        return _CACHE["scene"]
    n = 200_000
    r = np.random.default_rng(20240)
    lo, hi = np.array([-50.0, -50.0, -3.0]), np.array([50.0, 50.0, 17.0])
    n_uni, n_clu, n_one = int(0.55 * n), int(0.40 * n), 5000
    uni = r.uniform(lo, hi, (n_uni, 3))
    centres = r.uniform(lo + 1, hi - 1, (2000, 3))
    clu = centres[r.integers(0, 2000, n_clu)] + r.normal(0, 0.03, (n_clu, 3))
    one = np.array([12.345, -7.885, 4.565]) + r.uniform(-0.004, 0.004, (n_one, 3))   # inside one 0.01 m voxel
    n_dup = n - n_uni - n_clu - n_one - 2
    base = np.concatenate([uni, clu, one]).astype(np.float32)
    dup = base[r.integers(0, len(base), n_dup)]
    p = np.concatenate([base, dup, lo[None].astype(np.float32), hi[None].astype(np.float32)])
    p = np.clip(p, lo.astype(np.float32), hi.astype(np.float32))[r.permutation(n)]
    f = r.normal(0, 1, (n, 3)).astype(np.float32)
    c = np.stack([r.integers(0, 20, n), r.integers(-3, 3, n)], 1).astype(np.int32)
    _CACHE["scene"] = (np.ascontiguousarray(p), f, c)
    return _CACHE["scene"]


def scene_ref(dl):
    if ("ref", dl) not in _CACHE:
        _CACHE[("ref", dl)] = VR.subsample(*scene(), dl)
    return _CACHE[("ref", dl)]


def raw(p, f, c, dl, n=None, stride=None, ws_short=0, sp=-7.0):
    """The C entry on sentinel-filled outputs; returns (rc, dict of device tensors) after a sync."""
    from sdp import _lib
    L = _lib.lib()
    n = len(p) if n is None else n
    cap = len(p)
    stride = p.shape[1] if stride is None else stride
    fdim, ldim = (0 if f is None else f.shape[1]), (0 if c is None else c.shape[1])
    nb = _lib.SZ()
    _lib.check(L.sdp_voxel_grid_workspace_size(cap, _lib.C.byref(nb)), "ws")
    ws = torch.zeros(nb.value, dtype=torch.uint8, device=DEV)
    tp, tf, tc = dev(p), dev(f), dev(c)
    o = dict(points=torch.full((cap, 3), sp, dtype=torch.float32, device=DEV),
             features=torch.full((cap, max(fdim, 1)), sp, dtype=torch.float32, device=DEV),
             classes=torch.full((cap, max(ldim, 1)), -7, dtype=torch.int32, device=DEV),
             keys=torch.full((cap,), -7, dtype=torch.int64, device=DEV),
             counts=torch.full((cap,), -7, dtype=torch.int32, device=DEV),
             order=torch.full((cap,), -7, dtype=torch.int32, device=DEV),
             inverse=torch.full((cap,), -7, dtype=torch.int32, device=DEV),
             info=torch.full((5,), -7, dtype=torch.int64, device=DEV))
    rc = L.sdp_voxel_grid(tp.data_ptr(), n, stride, _lib.ptr(tf), fdim, _lib.ptr(tc), ldim, float(np.float32(dl)),
                          o["points"].data_ptr(), o["features"].data_ptr() if fdim else None,
                          o["classes"].data_ptr() if ldim else None, o["keys"].data_ptr(), o["counts"].data_ptr(),
                          o["order"].data_ptr(), o["inverse"].data_ptr(), o["info"].data_ptr(), ws.data_ptr(),
                          nb.value - ws_short, _lib.stream())
    torch.cuda.synchronize()
    return rc, o


def untouched(o, names=("points", "features", "classes", "keys", "counts", "order", "inverse", "info"), start=0):
    return all(bool((o[k][start:] == -7).all()) for k in names)


def check(p, f, c, dl, ref=None):
    """One raw call against voxel_ref: every output, every row, and the sentinels past m."""
    r = VR.subsample(p, f, c, dl) if ref is None else ref
    rc, o = raw(p, f, c, dl)
    assert rc == 0
    n = len(p)
    np.testing.assert_array_equal(o["info"].cpu().numpy(), r["info"])
    m, used = int(r["info"][0]), int(r["info"][4])
    np.testing.assert_array_equal(o["inverse"].cpu().numpy(), r["inverse"])
    if m == 0:
        assert untouched(o, ("points", "features", "classes", "keys", "counts", "order"))
        return r
    np.testing.assert_array_equal(o["order"][:used].cpu().numpy(), r["order"])
    np.testing.assert_array_equal(o["keys"][:m].cpu().numpy(), r["keys"])
    np.testing.assert_array_equal(o["counts"][:m].cpu().numpy(), r["counts"])
    np.testing.assert_array_equal(o["points"][:m].cpu().numpy().view(np.int32), r["points"].view(np.int32))
    if f is not None:
        np.testing.assert_array_equal(o["features"][:m].cpu().numpy().view(np.int32), r["features"].view(np.int32))
    if c is not None:
        np.testing.assert_array_equal(o["classes"][:m].cpu().numpy(), r["classes"])
    assert untouched(o, ("points", "keys", "counts") + (("features",) if f is not None else ()) +
                     (("classes",) if c is not None else ()), start=m)
    assert untouched(o, ("order",), start=used)
    if f is None:
        assert untouched(o, ("features",))
    if c is None:
        assert untouched(o, ("classes",))
    assert n >= used >= m
    return r


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("fdim,ldim", [(0, 0), (1, 1), (3, 2)])
def test_small_sizes(n, fdim, ldim):
    p = small_cloud(n)
    f, c = attrs(np.random.default_rng(n), n, fdim, ldim)
    r = check(p, f, c, 0.3)
    if n >= 63:
        assert 1 < r["info"][0] < n


@pytest.mark.parametrize("what", ["one_voxel", "identical", "own_voxel", "stride4", "non_finite", "one_finite",
                                  "none_finite"])
def test_shapes_of_clouds(what):
    n = 2 * TILE + 77
    r = np.random.default_rng(77)
    f, c = attrs(r, n, 3, 2)
    dl = 0.3
    p = small_cloud(n, seed=1)
    if what == "one_voxel":
        p, dl = (p * 0.5 + 1.5).astype(np.float32), 100.0
    elif what == "identical":
        p = np.tile(np.array([[0.7, -1.3, 2.9]], np.float32), (n, 1))
    elif what == "own_voxel":
        g = np.stack(np.meshgrid(np.arange(13), np.arange(13), np.arange(13), indexing="ij"), -1).reshape(-1, 3)
        p, dl = g[r.permutation(len(g))[:n]].astype(np.float32) + np.float32(0.25), 0.5
    elif what == "stride4":
        p = np.concatenate([p, r.normal(0, 1, (n, 1)).astype(np.float32)], 1)
        p[5, 3] = np.nan                      # the fourth float is not a coordinate
    elif what == "non_finite":
        bad = np.r_[0, n - 1, r.integers(1, n - 1, 40)]
        p[bad] = np.array([[np.nan, 0, 0], [0, np.inf, 0], [0, 0, -np.inf], [np.inf, np.nan, 1]], np.float32)[np.arange(len(bad)) % 4]
    elif what == "one_finite":
        p[:] = np.nan
        p[n // 3] = [1.0, 2.0, 3.0]
    elif what == "none_finite":
        p[:] = np.inf
    ref = check(p, f, c, dl)
    m = int(ref["info"][0])
    assert m == dict(one_voxel=1, identical=1, own_voxel=n, one_finite=1, none_finite=0).get(what, m)
    if what == "non_finite":
        assert ref["info"][4] < n - 2 and ref["inverse"][0] == -1 and ref["inverse"][-1] == -1
    if what == "stride4":
        assert ref["info"][4] == n


@pytest.mark.parametrize("dl", list(SCENE_DL))
def test_scene(dl):
    p, f, c = scene()
    ref = scene_ref(dl)
    assert ref["key_bits"] == SCENE_DL[dl], "the case no longer exercises the number of sort passes it claims"
    check(p, f, c, dl, ref=ref)
    tied = ref["tied"]
    print(f"voxel grid scene dl={dl}: bits={ref['key_bits']} m={ref['info'][0]} longest run={ref['counts'].max()} "
          f"tied voxels col0={tied[:, 0].mean():.3f} col1={tied[:, 1].mean():.3f}")
    assert ref["counts"].max() >= 5000 > 3 * TILE and (~tied).any()
    if dl <= 5.0:                 # nine voxels of 20,000 points have no tied labels; every finer grid does
        assert tied[:, 0].any() and tied[:, 1].any()


def test_scene_grid_too_large():
    from sdp.pointcloud import voxel_grid_subsample
    p, f, c = scene()
    ref = VR.subsample(p, f, c, 0.001)
    assert ref["key_bits"] == 48 and ref["info"][0] == -1
    rc, o = raw(p, f, c, 0.001)
    assert rc == 0
    np.testing.assert_array_equal(o["info"].cpu().numpy(), ref["info"])
    assert untouched(o, ("points", "features", "classes", "keys", "counts", "order", "inverse"))
    with pytest.raises(RuntimeError, match="100000 x 100000 x 20001"):
        voxel_grid_subsample(dev(p), sampleDl=0.001)


def test_second_scan_iteration():
    r = np.random.default_rng(5)
    n = N_SCAN
    p = r.uniform(0, 100, (n, 3)).astype(np.float32)
    p[r.integers(0, n, 50)] = np.nan
    f, c = attrs(r, n, 1, 1)
    ref = check(p, f, c, 1.0)
    assert ref["info"][0] > CHUNK * SCAN // 2 and ref["info"][4] > CHUNK * SCAN


def test_two_calls_are_bit_identical():
    p, f, c = scene()
    _, a = raw(p, f, c, 0.05)
    _, b = raw(p, f, c, 0.05)
    for k in a:
        assert torch.equal(a[k].view(torch.int32) if a[k].dtype == torch.float32 else a[k],
                           b[k].view(torch.int32) if b[k].dtype == torch.float32 else b[k]), k


@pytest.mark.parametrize("what", ["n0", "n_huge", "dl0", "dl_nan", "dl_neg", "stride5", "short_workspace"])
def test_errors_are_reported_and_nothing_is_enqueued(what):
    from sdp import _lib
    p = small_cloud(300)
    f, c = attrs(np.random.default_rng(3), 300, 1, 1)
    kw = dict(n0=dict(n=0), n_huge=dict(n=(1 << 30) + 1), dl0=dict(dl=0.0), dl_nan=dict(dl=float("nan")),
              dl_neg=dict(dl=-0.1), stride5=dict(stride=5), short_workspace=dict(ws_short=1))[what]
    rc, o = raw(p, f, c, kw.pop("dl", 0.3), **kw)
    assert rc < 0 and len(_lib.lib().sdp_last_error()) > 0
    assert untouched(o)
    nb = _lib.SZ()
    assert _lib.lib().sdp_voxel_grid_workspace_size(0, _lib.C.byref(nb)) < 0


def test_python_wrapper_return_convention():
    from sdp.pointcloud import voxel_grid_subsample
    p, f, c = scene()
    ref = scene_ref(0.5)
    tp, tf, tc = dev(p), dev(f), dev(c)
    only = voxel_grid_subsample(tp, sampleDl=0.5)
    assert torch.is_tensor(only) and only.dtype == torch.float32
    np.testing.assert_array_equal(only.cpu().numpy().view(np.int32), ref["points"].view(np.int32))
    pts, cls = voxel_grid_subsample(tp, classes=tc[:, 0], sampleDl=0.5)
    np.testing.assert_array_equal(cls.cpu().numpy(), ref["classes"][:, :1])
    pts, ft, cls, keys, counts, inv = voxel_grid_subsample(tp, tf, tc, 0.5, return_keys=True, return_counts=True,
                                                           return_inverse=True)
    np.testing.assert_array_equal(pts.cpu().numpy().view(np.int32), ref["points"].view(np.int32))
    np.testing.assert_array_equal(ft.cpu().numpy().view(np.int32), ref["features"].view(np.int32))
    np.testing.assert_array_equal(cls.cpu().numpy(), ref["classes"])
    np.testing.assert_array_equal(keys.cpu().numpy(), ref["keys"])
    np.testing.assert_array_equal(counts.cpu().numpy(), ref["counts"])
    np.testing.assert_array_equal(inv.cpu().numpy(), ref["inverse"])
    pts, ft, counts = voxel_grid_subsample(tp, tf, sampleDl=0.5, return_counts=True)
    np.testing.assert_array_equal(counts.cpu().numpy(), ref["counts"])


def test_float64_points_with_a_center():
    from sdp.pointcloud import voxel_grid_subsample
    r = np.random.default_rng(9)
    center = np.array([431234.567, -5812345.25, 112.125])
    p64 = center + r.uniform(-20, 20, (30000, 3))
    f = r.random((30000, 1)).astype(np.float32)
    q = (p64 - center).astype(np.float32)
    ref = VR.subsample(q, f, None, 0.2)
    pts, ft = voxel_grid_subsample(dev(p64), dev(f), sampleDl=0.2, center=dev(center))
    assert pts.dtype == torch.float64
    np.testing.assert_array_equal(pts.cpu().numpy(), ref["points"].astype(np.float64) + center)
    np.testing.assert_array_equal(ft.cpu().numpy().view(np.int32), ref["features"].view(np.int32))
    zero = voxel_grid_subsample(dev(p64 - center), sampleDl=0.2)          # center defaults to zeros
    np.testing.assert_array_equal(zero.cpu().numpy(), ref["points"].astype(np.float64))


def test_fuse_views_on_a_grid():
    from sdp.pointcloud import fuse_views, voxel_grid_subsample
    r = np.random.default_rng(4)
    x = dev(r.uniform(0.05, 1.0, (3, 2, 16, 128)).astype(np.float32))
    origins = dev(r.uniform(-3.0, 3.0, (3, 3)))
    cloud = fuse_views(x, origins=origins)
    grid = fuse_views(x, origins=origins, grid=0.4)
    pts, it = voxel_grid_subsample(cloud[:, :3], features=cloud[:, 3:4], sampleDl=0.4)
    assert grid.dtype == torch.float64 and grid.shape[1] == 4 and 0 < grid.shape[0] < cloud.shape[0]
    assert torch.equal(grid, torch.cat((pts, it.double()), 1))
    c = cloud.cpu().numpy()
    ref = VR.subsample(c[:, :3].astype(np.float32), c[:, 3:4].astype(np.float32), None, 0.4)
    np.testing.assert_array_equal(grid.cpu().numpy(), np.concatenate([ref["points"], ref["features"]], 1).astype(np.float64))
    assert torch.equal(fuse_views(x, origins=origins, grid=None), cloud)


def test_stage_events_hook():
    """sdp_voxel_grid_stage_events: seven events recorded in stream order by every later call, until switched off."""
    from sdp import _lib
    L = _lib.lib()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(7)]
    for e in ev:
        e.record()
    torch.cuda.synchronize()
    arr = (_lib.P * 7)(*[e.cuda_event for e in ev])
    assert L.sdp_voxel_grid_stage_events(arr) == 0
    try:
        p, f, c = scene()
        rc, o = raw(p, f, c, 0.5)
    finally:
        assert L.sdp_voxel_grid_stage_events(None) == 0
    assert rc == 0 and int(o["info"][0]) == scene_ref(0.5)["info"][0]
    dt = [ev[i].elapsed_time(ev[i + 1]) for i in range(6)]
    assert all(t >= 0 for t in dt) and sum(dt) > 0
    bad = (_lib.P * 7)(*([ev[0].cuda_event] * 6 + [None]))
    assert L.sdp_voxel_grid_stage_events(bad) < 0
