"""sdp_voxel_iou (csrc/voxel_iou.hip) on the GPU against tests/voxel_iou_ref.py (pinned on the CPU in
tests/test_voxel_iou_ref_cpu.py): exact integer equality of the confusion matrix, info [8] and the optional
cells / labels / counts of both sides.  Every raw call fills its outputs with sentinels first and checks that the
rows past m were left alone.

Sizes come from the kernel's constants (read from the sources): na, nb in 1, 63, 64, 65, CHUNK - 1, CHUNK + 1,
TILE - 1, TILE, TILE + 1, 3 TILE + 17; SCAN - 1, SCAN, SCAN + 1 unique cells (SCAN = the counts of one scan
iteration); one case of CHUNK * SCAN + 300 points per side, so that every single-workgroup scan (used-point
chunks, digit counts, segment-head chunks) takes a second iteration.  Shapes: empty clouds, all points in one
voxel (5,000: a segment across several sort tiles), one voxel per point, every point out of bounds, planted NaN /
+-inf / +-1e300 and labels -1 and C, lattice points on the cell faces for voxel = 0.25 (exact) and 0.2 (not exact:
the device must land where numpy lands, one ulp on either side of a face too), label ties, C = 1, 20, 64, identical
and disjoint clouds, a valid mask, stride 4, the SSC grid, a grid of 2^40 cells (all six sort passes move keys)
and one of 2^41, which must fail at the call like every other bad argument.
"""
import os
import re

import numpy as np
import pytest
import torch

import voxel_iou_ref as IR
from conftest import PKG_DIR

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENT = -7


def _constants():
    src = open(os.path.join(PKG_DIR, "csrc", "voxel_iou.hip")).read()
    get = lambda name: int(re.search(r"constexpr int %s = (\d+);" % name, src).group(1))
    return get("VIOU_SORT_TILE"), get("VIOU_CHUNK"), get("VIOU_SCAN_THREADS") * get("VIOU_SCAN_PER_THREAD")


TILE, CHUNK, SCAN = _constants()
N_SCAN = CHUNK * SCAN + 300
assert -(-N_SCAN // CHUNK) > SCAN and 256 * -(-N_SCAN // TILE) > SCAN
SIZES = [1, 63, 64, 65, CHUNK - 1, CHUNK + 1, TILE - 1, TILE, TILE + 1, 3 * TILE + 17]
SSC = dict(origin=(0.0, -25.6, -2.0), voxel=0.2, dims=(256, 256, 32))


def dev(a, dtype=None):
    return None if a is None else torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).to(DEV)


def raw(a, la, b, lb, origin, voxel, dims, C, valid=None, conf_cap=None):
    """The C entry on sentinel-filled outputs; returns (rc, dict of device tensors) after a sync."""
    from sdp import _lib
    L = _lib.lib()
    na, nb = len(a), len(b)
    nbytes = _lib.SZ()
    _lib.check(L.sdp_voxel_iou_workspace_size(na, nb, min(max(C, 1), 64), _lib.C.byref(nbytes)), "ws")
    ws = torch.zeros(nbytes.value, dtype=torch.uint8, device=DEV)
    ta, tb = dev(a, torch.float64), dev(b, torch.float64)
    tla, tlb = dev(la, torch.int32), dev(lb, torch.int32)
    tv = dev(valid, torch.uint8)
    S = (C + 1) if conf_cap is None else conf_cap
    full = lambda n, dt: torch.full((max(n, 1),), SENT, dtype=dt, device=DEV)
    o = dict(confusion=full(S * S, torch.int64), info=full(8, torch.int64),
             a_cells=full(na, torch.int64), a_labels=full(na, torch.int32), a_counts=full(na, torch.int32),
             b_cells=full(nb, torch.int64), b_labels=full(nb, torch.int32), b_counts=full(nb, torch.int32))
    ptr = lambda t: t.data_ptr() if t is not None and t.numel() else None
    rc = L.sdp_voxel_iou(ptr(ta), na, a.shape[1] if na else 3, ptr(tla), ptr(tb), nb, b.shape[1] if nb else 3, ptr(tlb),
                         (_lib.D * 3)(*[float(v) for v in origin]), float(voxel),
                         (_lib.C.c_int64 * 3)(*[int(v) for v in dims]), C, ptr(tv), o["confusion"].data_ptr(),
                         o["a_cells"].data_ptr(), o["a_labels"].data_ptr(), o["a_counts"].data_ptr(),
                         o["b_cells"].data_ptr(), o["b_labels"].data_ptr(), o["b_counts"].data_ptr(),
                         o["info"].data_ptr(), ws.data_ptr(), nbytes.value, _lib.stream())
    torch.cuda.synchronize()
    return rc, {k: v.cpu().numpy() for k, v in o.items()}


def check(a, la, b, lb, origin, voxel, dims, C, valid=None, twice=False):
    """One raw call against voxel_iou_ref: every output, every row, and the sentinels past m."""
    r = IR.confusion(a, la, b, lb, origin, voxel, dims, C, valid)
    rc, o = raw(a, la, b, lb, origin, voxel, dims, C, valid)
    assert rc == 0
    np.testing.assert_array_equal(o["info"], r["info"])
    np.testing.assert_array_equal(o["confusion"].reshape(C + 1, C + 1), r["confusion"])
    for side in "ab":
        m = len(r[side]["cells"])
        np.testing.assert_array_equal(o[f"{side}_cells"][:m], r[side]["cells"])
        np.testing.assert_array_equal(o[f"{side}_labels"][:m], r[side]["labels"])
        np.testing.assert_array_equal(o[f"{side}_counts"][:m], r[side]["counts"])
        for k in ("cells", "labels", "counts"):
            assert (o[f"{side}_{k}"][m:] == SENT).all()
    nvalid = int(np.prod([int(v) for v in dims])) if valid is None else int(np.count_nonzero(valid))
    assert o["confusion"].sum() == nvalid
    if twice:
        rc2, o2 = raw(a, la, b, lb, origin, voxel, dims, C, valid)
        assert rc2 == 0
        for k in o:
            assert o[k].tobytes() == o2[k].tobytes(), k
    return r


def cloud(n, seed, C, lo=-0.3, hi=4.3):
    """n points around a 4 m cube (some outside), labels in [0, C); an exact duplicate when there is room."""
    r = np.random.default_rng(1000 + 7 * n + seed)
    p = r.uniform(lo, hi, (n, 3))
    if n > 4:
        p[n // 2] = p[1]
    return p, r.integers(0, C, n).astype(np.int32)


@pytest.mark.parametrize("k", range(len(SIZES)))
def test_sizes(k):
    na, nb = SIZES[k], SIZES[len(SIZES) - 1 - k]
    C = 5
    a, la = cloud(na, 0, C)
    b, lb = cloud(nb, 1, C)
    r = check(a, la, b, lb, (0, 0, 0), 0.5, (8, 8, 8), C)
    if min(na, nb) >= 63:
        assert r["info"][6] > 0 and r["confusion"][1:, 0].sum() + r["confusion"][0, 1:].sum() > 0


@pytest.mark.parametrize("m", [SCAN - 1, SCAN, SCAN + 1])
def test_unique_cells_around_one_scan_iteration(m):
    r = np.random.default_rng(m)
    dims = (32, 32, 8)
    cells = r.permutation(32 * 32 * 8)[:m]
    centre = lambda c: np.stack([c % 32, c // 32 % 32, c // 1024], 1) + 0.5
    a = np.concatenate([centre(cells), centre(cells[r.integers(0, m, 500)])])[r.permutation(m + 500)]
    b = centre((cells + 1) % (32 * 32 * 8))
    la, lb = r.integers(0, 3, len(a)).astype(np.int32), r.integers(0, 3, len(b)).astype(np.int32)
    ref = check(a, la, b, lb, (0, 0, 0), 1.0, dims, 3)
    assert ref["info"][0] == m and ref["info"][1] == m


@pytest.mark.parametrize("na,nb", [(0, 700), (700, 0), (0, 0)])
def test_empty_clouds(na, nb):
    a, la = cloud(na, 2, 3)
    b, lb = cloud(nb, 3, 3)
    r = check(a, la, b, lb, (0, 0, 0), 0.5, (8, 8, 8), 3)
    assert r["info"][6] == 0 and r["confusion"][1:, 1:].sum() == 0


@pytest.mark.parametrize("what", ["one_voxel", "own_voxel", "out_of_bounds", "bad_points", "ties", "identical",
                                  "disjoint", "stride4", "no_labels"])
def test_shapes_of_clouds(what):
    r = np.random.default_rng(77)
    C, n = 4, 2 * TILE + 77
    origin, voxel, dims = (0.0, 0.0, 0.0), 0.5, (8, 8, 8)
    a, la = cloud(n, 4, C)
    b, lb = cloud(n - 100, 5, C)
    if what == "one_voxel":
        a, la = r.uniform(1.01, 1.49, (5000, 3)), r.integers(0, C, 5000).astype(np.int32)
    elif what == "own_voxel":
        g = np.stack(np.meshgrid(np.arange(13), np.arange(13), np.arange(13), indexing="ij"), -1).reshape(-1, 3)
        a, dims = (g[r.permutation(len(g))[:n]] + 0.25) * voxel, (13, 13, 13)
    elif what == "out_of_bounds":
        a = np.concatenate([a[: n // 2] + 4.5, -np.abs(a[n // 2:]) - 0.01])
    elif what == "bad_points":
        bad = np.r_[0, n - 1, r.integers(1, n - 1, 60)]
        a[bad] = np.array([[np.nan, 1, 1], [1, np.inf, 1], [1, 1, -np.inf], [1e300, 1, 1], [1, -1e300, 1],
                           [np.inf, np.nan, 1]])[np.arange(len(bad)) % 6]
        la[r.integers(0, n, 50)] = -1
        la[r.integers(0, n, 50)] = C
        lb[r.permutation(len(lb))[:50]] = np.array([-2 ** 31, 2 ** 31 - 1, 64, C + 1, -1], np.int32)[np.arange(50) % 5]
    elif what == "ties":
        a = np.repeat(r.uniform(0.01, 3.99, (n // 4, 3)), 4, 0)               # four points per spot ...
        la = np.tile(np.array([3, 1, 3, 1], np.int32), n // 4)                   # ... two votes for 3, two for 1
    elif what == "identical":
        b, lb = a.copy(), la.copy()
    elif what == "disjoint":
        a[:, 0] = a[:, 0] * 0.3            # x below 1.29: cells 0 to 2 ...
        b[:, 0] = 2.0 + b[:, 0] * 0.4      # ... and above 1.88: cells 3 to 7
    elif what == "stride4":
        a = np.concatenate([a, r.normal(0, 1, (n, 1))], 1)
        a[5, 3] = np.nan                   # the fourth double is not a coordinate
        b = np.concatenate([b, np.full((len(b), 1), np.inf)], 1)
    elif what == "no_labels":
        la = lb = None
    ref = check(a, la, b, lb, origin, voxel, dims, C, twice=what in ("one_voxel", "ties"))
    conf, info = ref["confusion"], ref["info"]
    if what == "one_voxel":
        assert info[0] == 1 and ref["a"]["counts"][0] == 5000
    elif what == "own_voxel":
        assert info[0] == n == info[2]
    elif what == "out_of_bounds":
        assert info[0] == 0 and info[2] == 0 and conf[1:].sum() == 0
    elif what == "bad_points":
        assert info[4] > 90 and info[5] == 50 and info[2] < n - 60
    elif what == "ties":
        assert ref["a"]["tied"].all() and info[0] > 100 and set(ref["a"]["labels"]) == {1}
    elif what == "identical":
        assert (conf - np.diag(np.diagonal(conf))).sum() == 0 and info[6] == info[0] == info[1]
    elif what == "disjoint":
        assert info[6] == 0 and conf[1:, 1:].sum() == 0 and conf[1:, 0].sum() == info[0] and conf[0, 1:].sum() == info[1]


@pytest.mark.parametrize("C", [1, 20, 64])
def test_number_of_classes(C):
    n = TILE + 300
    a, la = cloud(n, 6, C)
    b, lb = cloud(n, 7, C)
    ref = check(a, la, b, lb, (0, 0, 0), 1.0, (4, 4, 4), C)      # 64 cells: long segments, many labels per cell
    assert ref["info"][6] >= 60
    if C > 1:
        assert len(set(ref["a"]["labels"])) > 1


@pytest.mark.parametrize("voxel", [0.25, 0.2])
def test_points_on_cell_faces(voxel):
    """Lattice points origin + k * voxel, and their neighbours one ulp below and above: 0.25 is exact in float64,
    0.2 is not -- (k * 0.2 - origin) / 0.2 may floor to k or to k - 1, and the device must agree with numpy."""
    dims = (40, 30, 20)
    origin = np.array([0.0, -3.0, 1.7]) if voxel == 0.2 else np.array([0.0, -3.0, 1.75])
    k = np.stack(np.meshgrid(np.arange(-1, 42), np.arange(-1, 32, 3), np.arange(-1, 22, 4), indexing="ij"), -1).reshape(-1, 3)
    face = origin + k * np.float64(voxel)
    a = np.concatenate([face, np.nextafter(face, -np.inf), np.nextafter(face, np.inf)])
    b = np.concatenate([origin + (k + 0.5) * np.float64(voxel), face[::3]])
    ref = check(a, None, b, None, origin, voxel, dims, 1)
    assert ref["info"][0] > 1000
    if voxel == 0.2:
        # the inexact case really splits: lattice points that do not land in "their" cell k exist
        inside, key = IR.cell_keys(face, origin, voxel, dims)
        kk = k[:, 0] + 40 * k[:, 1] + 1200 * k[:, 2]
        ok = ((k >= 0) & (k < np.array(dims))).all(1)
        assert (key[ok & inside] != kk[ok & inside]).any() or (~inside[ok]).any()


def test_valid_mask_removes_occupied_and_empty_cells():
    r = np.random.default_rng(11)
    C, n, dims = 6, 3 * TILE + 17, (19, 17, 11)            # 3553 cells for 3089 points: empty cells in both clouds
    a = np.concatenate([r.uniform(-0.2, 1.0, (n, 3)) * (np.array(dims) * 0.3), r.normal(0, 1, (n, 1))], 1)   # stride 4
    b = r.uniform(-0.2, 1.0, (n - 50, 3)) * (np.array(dims) * 0.3) * [1.0, 0.6, 1.0]      # leaves empty cells
    la, lb = r.integers(0, C, n).astype(np.int32), r.integers(0, C, n - 50).astype(np.int32)
    valid = (r.random((dims[2], dims[1], dims[0])) > 0.4).astype(np.uint8) * r.integers(1, 255, (dims[2], dims[1], dims[0])).astype(np.uint8)
    ref = check(a, la, b, lb, (0, 0, 0), 0.3, dims, C, valid, twice=True)
    full = IR.confusion(a, la, b, lb, (0, 0, 0), 0.3, dims, C)
    assert ref["info"][0] < full["info"][0] and ref["info"][7] == np.count_nonzero(valid) < 19 * 17 * 11
    assert 0 < ref["confusion"][0, 0] < full["confusion"][0, 0]      # the mask took away empty cells too
    # an unaligned mask pointer and a size that is no multiple of 16 take the byte-wise ends of the count
    pad = np.concatenate([np.zeros(3, np.uint8), valid.reshape(-1)])
    tv = dev(pad)[3:]
    assert tv.data_ptr() % 16 == 3
    conf, info = _call_with_mask_tensor(a, la, b, lb, (0, 0, 0), 0.3, dims, C, tv)
    np.testing.assert_array_equal(conf, ref["confusion"])
    np.testing.assert_array_equal(info, ref["info"])


def _call_with_mask_tensor(a, la, b, lb, origin, voxel, dims, C, tv):
    from sdp import _lib
    L = _lib.lib()
    nbytes = _lib.SZ()
    _lib.check(L.sdp_voxel_iou_workspace_size(len(a), len(b), C, _lib.C.byref(nbytes)), "ws")
    ws = torch.zeros(nbytes.value, dtype=torch.uint8, device=DEV)
    ta, tb, tla, tlb = dev(a, torch.float64), dev(b, torch.float64), dev(la, torch.int32), dev(lb, torch.int32)
    conf = torch.zeros((C + 1) ** 2, dtype=torch.int64, device=DEV)
    info = torch.zeros(8, dtype=torch.int64, device=DEV)
    _lib.check(L.sdp_voxel_iou(ta.data_ptr(), len(a), a.shape[1], tla.data_ptr(), tb.data_ptr(), len(b), b.shape[1],
                               tlb.data_ptr(), (_lib.D * 3)(*origin), float(voxel), (_lib.C.c_int64 * 3)(*dims), C,
                               tv.data_ptr(), conf.data_ptr(), None, None, None, None, None, None, info.data_ptr(),
                               ws.data_ptr(), nbytes.value, _lib.stream()), "voxel_iou")
    torch.cuda.synchronize()
    return conf.cpu().numpy().reshape(C + 1, C + 1), info.cpu().numpy()


def test_ssc_grid_with_mask():
    r = np.random.default_rng(12)
    C, n = 20, 40_000
    lo, ext = np.array(SSC["origin"]), np.array(SSC["dims"]) * SSC["voxel"]
    centres = lo + r.uniform(0, 1, (300, 3)) * ext
    a = np.concatenate([lo + r.uniform(-0.02, 1.02, (n // 2, 3)) * ext, centres[r.integers(0, 300, n // 2)] + r.normal(0, 0.3, (n // 2, 3))])
    b = a[r.permutation(n)[: n - 5000]] + r.normal(0, 0.05, (n - 5000, 3))
    la, lb = r.integers(0, C, n).astype(np.int32), r.integers(0, C, n - 5000).astype(np.int32)
    nx, ny, nz = SSC["dims"]
    valid = (r.random((nz, ny, nx)) > 0.1).astype(np.uint8)
    ref = check(a, la, b, lb, SSC["origin"], SSC["voxel"], SSC["dims"], C, valid)
    assert ref["info"][6] > 1000 and ref["info"][7] == valid.sum()


def test_grid_of_2_to_the_40_cells_and_beyond():
    r = np.random.default_rng(13)
    dims = (1 << 14, 1 << 14, 1 << 12)
    C, n, voxel = 64, 2 * TILE + 5, 0.01
    ext = np.array(dims) * voxel
    a = r.uniform(0, 1, (n, 3)) * ext
    a[0], a[1] = [0.001, 0.001, 0.001], ext - 0.001                    # the first and the last cell
    b = np.concatenate([a[: n // 2] + r.normal(0, 0.002, (n // 2, 3)), r.uniform(0, 1, (n // 2, 3)) * ext])
    la, lb = r.integers(0, C, n).astype(np.int32), r.integers(0, C, len(b)).astype(np.int32)
    ref = check(a, la, b, lb, (0, 0, 0), voxel, dims, C)
    assert ref["a"]["cells"][0] == 0 and ref["a"]["cells"][-1] == (1 << 40) - 1
    comp = (ref["a"]["cells"] << 6) | ref["a"]["labels"]
    for p in range(6):                                                 # every sort pass has digits to move
        assert len(np.unique((comp >> (8 * p)) & 255)) > 1
    rc, o = raw(a, la, b, lb, (0, 0, 0), voxel, (1 << 14, 1 << 14, 1 << 13), C)
    assert rc != 0 and all((v == SENT).all() for v in o.values())
    from sdp import _lib
    assert b"2^40" in _lib.lib().sdp_last_error()


@pytest.mark.parametrize("what,msg", [("dims0", b"dim"), ("dims_neg", b"dim"), ("voxel0", b"voxel"), ("voxel_nan", b"voxel"),
                                      ("voxel_inf", b"voxel"), ("origin_nan", b"origin"), ("origin_inf", b"origin"),
                                      ("C0", b"num_classes"), ("C65", b"num_classes"), ("mask_cells", b"2^31")])
def test_bad_arguments_fail_the_call_and_write_nothing(what, msg):
    from sdp import _lib
    a, la = cloud(100, 8, 1)
    b, lb = cloud(90, 9, 1)
    kw = dict(origin=(0.0, 0.0, 0.0), voxel=0.5, dims=(8, 8, 8), C=1, valid=None)
    kw.update(dict(dims0=dict(dims=(8, 0, 8)), dims_neg=dict(dims=(8, 8, -1)), voxel0=dict(voxel=0.0),
                   voxel_nan=dict(voxel=float("nan")), voxel_inf=dict(voxel=float("inf")),
                   origin_nan=dict(origin=(0.0, float("nan"), 0.0)), origin_inf=dict(origin=(float("-inf"), 0.0, 0.0)),
                   C0=dict(C=0), C65=dict(C=65),
                   mask_cells=dict(dims=(1 << 11, 1 << 11, (1 << 9) + 1), valid=np.ones(16, np.uint8)))[what])
    rc, o = raw(a, la, b, lb, kw["origin"], kw["voxel"], kw["dims"], kw["C"], kw["valid"], conf_cap=66)
    assert rc != 0 and all((v == SENT).all() for v in o.values())
    assert msg in _lib.lib().sdp_last_error()


def test_every_scan_takes_a_second_iteration():
    r = np.random.default_rng(14)
    C, n = 20, N_SCAN
    lo, ext = np.array(SSC["origin"]), np.array(SSC["dims"]) * SSC["voxel"]
    a = lo + r.uniform(0.001, 0.999, (n, 3)) * ext
    b = a[r.permutation(n)] + r.normal(0, 0.08, (n, 3))
    la, lb = r.integers(0, C, n).astype(np.int32), r.integers(-1, C, n).astype(np.int32)
    ref = check(a, la, b, lb, SSC["origin"], SSC["voxel"], SSC["dims"], C)
    assert ref["info"][2] == n > CHUNK * SCAN and ref["info"][0] > 100_000 and ref["info"][5] > 0


def test_python_interface():
    from sdp import pointcloud as PC
    C = 5
    a, la = cloud(3000, 10, C)
    b, lb = cloud(2500, 11, C)
    grid = dict(origin=(0.0, 0.0, 0.0), voxel=0.5, dims=(8, 8, 8))
    ref = IR.confusion(a, la, b, lb, num_classes=C, **grid)
    ta, tb = dev(a, torch.float64), dev(b, torch.float64)
    conf, info, ca, cb = PC.voxel_confusion(ta, tb, truth_labels=dev(la).long(), pred_labels=dev(lb), num_classes=C,
                                            return_cells=True, **grid)
    assert conf.dtype == torch.int64 and conf.shape == (C + 1, C + 1) and conf.is_cuda and info.shape == (8,)
    np.testing.assert_array_equal(conf.cpu().numpy(), ref["confusion"])
    np.testing.assert_array_equal(info.cpu().numpy(), ref["info"])
    for got, side in ((ca, "a"), (cb, "b")):
        for t, k in zip(got, ("cells", "labels", "counts")):
            np.testing.assert_array_equal(t.cpu().numpy(), ref[side][k])
    # float32 clouds are widened: the reference on the widened values
    a32, b32 = a.astype(np.float32), b.astype(np.float32)
    out = PC.voxel_iou(dev(a32), dev(b32), truth_labels=dev(la), pred_labels=dev(lb), num_classes=C, ignore=(1,), **grid)
    ref32 = IR.confusion(a32.astype(np.float64), la, b32.astype(np.float64), lb, num_classes=C, **grid)
    np.testing.assert_array_equal(out["confusion"], ref32["confusion"])
    np.testing.assert_array_equal(out["info"], ref32["info"])
    want = PC.iou_from_confusion(ref32["confusion"], ignore=(1,))
    assert out["iou"] == want["iou"] and out["miou"] == want["miou"] and 0 < out["iou"] < 1
    np.testing.assert_array_equal(out["class_iou"], want["class_iou"])
    # occupancy only, a mask, and a dense ground-truth volume as the truth
    nx, ny, nz = grid["dims"]
    vol = np.random.default_rng(3).integers(0, C + 1, (nz, ny, nx))
    pts, lab = PC.volume_to_cloud(dev(vol), grid["origin"], grid["voxel"], empty=0)
    mask = dev((vol != 2).astype(np.uint8))
    got = PC.voxel_iou(pts, tb, truth_labels=lab - 1, pred_labels=dev(lb), num_classes=C, valid=mask, **grid)
    refv = IR.confusion(pts.cpu().numpy(), (lab - 1).cpu().numpy(), b, lb, num_classes=C, valid=(vol != 2), **grid)
    np.testing.assert_array_equal(got["confusion"], refv["confusion"])
    assert got["info"][0] == ((vol != 0) & (vol != 2)).sum() and got["confusion"].sum() == (vol != 2).sum()
    for bad in (dict(voxel=0.0), dict(dims=(8, 8)), dict(dims=(8, 0, 8)), dict(origin=(0.0, np.nan, 0.0)),
                dict(num_classes=0), dict(num_classes=65), dict(dims=(1 << 14, 1 << 14, 1 << 13)),
                dict(truth_labels=dev(la)[:-1]), dict(valid=mask[:-1]), dict(truth_labels=dev(la).float())):
        with pytest.raises(ValueError):
            PC.voxel_confusion(ta, tb, **{**grid, "num_classes": C, **bad})
    with pytest.raises(ValueError):
        PC.voxel_confusion(ta.cpu(), tb, **grid)
