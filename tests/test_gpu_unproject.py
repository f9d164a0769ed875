"""sdp_range_unproject (csrc/unproject.hip) on the GPU against the float64 restatement
tests/pointcloud_ref.py (pinned to the projection oracle in tests/test_pointcloud_cpu.py).

Shapes: (1,3,7); (3,5,48), no multiple of a wave or of a chunk; (2,64,1024) and (3,64,1024); and B
views of 64x1024 with B taken from the kernel's constants so that the chunk counts need a second iteration of the scan
kernel (B = 17: 4352 chunks of 256 pixels against 4096 per iteration, 36 MB of rows).  View 0 of every
multi-view case keeps nothing (codes with rd < 1.5), view 1 keeps everything (every code far enough, its
own mask all ones: all pixels without masks, all the shared mask allows with them), the others ~70 %
(59 % under the masks); the 2-view case can hold only the first two kinds, so (3,64,1024) stands beside it.
Codes are uniform in [0.05, 1] plus planted negatives, NaNs, zeros and values with rd <= 1.5, some of
them just below and just above the threshold; a guard on the restatement alone asserts no pixel has
|rd - 1.5| < 1e-5, so the float32 keep compare cannot differ between the two sides.

Gates: offsets and pixel exactly equal, intensity bit-equal, coordinates within
1e-12 * max(1, max|coordinate| of the case): three float64 factors within 2 ulp each and their
roundings bound the error near 1e-15 relative, one bin of angle error is 6e-3 rad.
Measured worst on an MI355X: 2.8e-14 absolute, 2.6e-16 of the case's largest coordinate.
"""
import os
import re

import numpy as np
import pytest
import torch

import pointcloud_ref as PR
from conftest import PKG_DIR

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _constants():
    src = open(os.path.join(PKG_DIR, "csrc", "unproject.hip")).read()
    chunk = int(re.search(r"constexpr int UNPROJ_CHUNK = (\d+);", src).group(1))
    scan = int(re.search(r"constexpr int UNPROJ_SCAN_THREADS = (\d+);", src).group(1))
    per = int(re.search(r"constexpr int UNPROJ_SCAN_PER_THREAD = (\d+);", src).group(1))
    return chunk, scan * per


CHUNK, SCAN = _constants()
B_SCAN = SCAN // (-(-64 * 1024 // CHUNK)) + 1          # the first B whose chunk count exceeds one scan iteration
assert B_SCAN * 64 * 1024 * 32 < 150e6
SMALL = [(1, 3, 7), (3, 5, 48)]
BIG = [(2, 64, 1024), (3, 64, 1024), (B_SCAN, 64, 1024)]
_CASES = {}


def case(B, H, W):
    """Inputs of one shape, built once and never modified: x [B,2,H,W], keep [B,H,W], exist [H,W],
    origins [B,3], poses [B,4,4] (general, non-symmetric)."""
    key = (B, H, W)
    if key in _CASES:
        return _CASES[key]
    r = np.random.default_rng(B * 1000003 + H * 1009 + W)
    x = r.uniform(0.05, 1.0, (B, 2, H, W)).astype(np.float32)
    d = x[:, 0]
    u = r.random((B, H, W))
    d[u < 0.10] = r.uniform(0.05, 0.2, (B, H, W)).astype(np.float32)[u < 0.10]   # rd <= 1.3: dropped
    d[(u >= 0.10) & (u < 0.12)] = np.nan
    d[(u >= 0.12) & (u < 0.14)] = 0.0
    d[(u >= 0.14) & (u < 0.20)] *= -1                                            # kept by their magnitude
    keep = r.random((B, H, W)) < 0.92
    if B > 1:
        x[0, 0] = r.uniform(0.05, 0.2, (H, W)).astype(np.float32)                # view 0: nothing kept
        x[1, 0] = r.uniform(0.3, 1.0, (H, W)).astype(np.float32)                 # view 1: everything kept
        keep[1] = True
    exist = r.random((H, W)) < 0.9
    origins = r.uniform(-30.0, 30.0, (B, 3))
    poses = r.uniform(-1.0, 1.0, (B, 4, 4))
    poses[:, :3, 3] = r.uniform(-100.0, 100.0, (B, 3))
    poses[:, 3] = r.uniform(-1.0, 1.0, (B, 4))           # the last row must not enter the result
    # codes closer than 1e-4 to the threshold (a handful per million) become planted values just below
    # and just above it: rd = 1.4987 and 1.5008
    with np.errstate(invalid="ignore"):
        near = np.abs(PR.distance(d).astype(np.float64) - 1.5) < 1e-4
    d[near] = np.where(np.arange(int(near.sum())) % 2 == 0, np.float32(0.2202), np.float32(0.2204))
    if B > 1:
        d[1][near[1]] = np.float32(0.2204)                                           # view 1 still keeps everything
    d[0, 0, :2] = (0.2202, 0.2204) if B == 1 else (0.2202, 0.2202)
    rd = PR.distance(d)
    with np.errstate(invalid="ignore"):
        assert not (np.abs(rd.astype(np.float64) - 1.5) < 1e-5).any(), "a code sits on the min-range threshold"
    _CASES[key] = dict(x=x, keep=keep, exist=exist, origins=origins, poses=poses)
    return _CASES[key]


def dev(a, dtype=None):
    return None if a is None else torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).to(DEV)


def run(c, C, place, masks, geometry, return_pixel=True):
    from sdp.pointcloud import range_image_to_point_cloud
    kw = dict(origins=dev(c["origins"]) if place == "origins" else None,
              poses=dev(c["poses"]) if place == "poses" else None,
              keep=dev(c["keep"]) if masks else None, exist=dev(c["exist"]) if masks else None)
    return range_image_to_point_cloud(dev(c["x"][:, :C]), geometry=geometry, return_pixel=return_pixel, **kw)


def ref(c, C, place, masks, geometry):
    return PR.unproject(c["x"][:, :C], origins=c["origins"] if place == "origins" else None,
                        poses=c["poses"] if place == "poses" else None, keep=c["keep"] if masks else None,
                        exist=c["exist"] if masks else None, geometry=geometry)


def check_parity(shape, C, place, masks, geometry):
    c = case(*shape)
    pts, off, pix = (t.cpu().numpy() for t in run(c, C, place, masks, geometry))
    rp, ro, rpix, _ = ref(c, C, place, masks, geometry)
    np.testing.assert_array_equal(off, ro)
    np.testing.assert_array_equal(pix, rpix)
    assert pts.shape == rp.shape and pts.dtype == np.float64
    B = shape[0]
    if B > 1:
        n = shape[1] * shape[2]
        assert off[1] == 0, "view 0 keeps nothing"
        # view 1: every code is far enough and its own mask is all ones, so only the shared mask can drop
        assert off[2] - off[1] == (int(c["exist"].sum()) if masks else n), "view 1 keeps everything"
        if B > 2:
            assert 0.5 * n < off[3] - off[2] < 0.8 * n, "view 2 keeps roughly 60-70 %"
    scale = max(1.0, float(np.abs(rp[:, :3]).max())) if len(rp) else 1.0
    err = float(np.abs(pts[:, :3] - rp[:, :3]).max()) if len(rp) else 0.0
    print(f"unproject {shape} C={C} {place} masks={masks} {geometry}: n={len(rp)} kept={len(rp) / (B * shape[1] * shape[2]):.2f} "
          f"worst |err|={err:.3e} scale={scale:.1f} ratio={err / scale:.2e}")
    assert err <= 1e-12 * scale
    assert np.array_equal(pts[:, 3].view(np.int64), rp[:, 3].view(np.int64)), "intensity must be bit-equal"


@pytest.mark.parametrize("shape", SMALL)
@pytest.mark.parametrize("C", [1, 2])
@pytest.mark.parametrize("geometry", ["dataset", "sampler"])
@pytest.mark.parametrize("place,masks", [("none", False), ("origins", True), ("poses", True)])
def test_parity_small(shape, C, geometry, place, masks):
    check_parity(shape, C, place, masks, geometry)


@pytest.mark.parametrize("shape", BIG)
@pytest.mark.parametrize("C,geometry,place,masks", [(2, "dataset", "origins", True), (1, "sampler", "poses", True),
                                                    (2, "sampler", "none", False), (1, "dataset", "poses", False)])
def test_parity_big(shape, C, geometry, place, masks):
    check_parity(shape, C, place, masks, geometry)


def raw_call(c, C=2, origins=None, poses=None, ws_short=0, sentinel=-7.0):
    """The C entry on caller-filled buffers: returns (rc, points, pixel, offsets) after a sync."""
    from sdp import _lib
    L = _lib.lib()
    x = dev(c["x"][:, :C] if C <= 2 else np.repeat(c["x"][:, :1], C, 1))
    B, _, H, W = x.shape
    n = _lib.SZ()
    _lib.check(L.sdp_range_unproject_workspace_size(B, H, W, _lib.C.byref(n)), "ws")
    ws = torch.zeros(n.value, dtype=torch.uint8, device=DEV)
    points = torch.full((B * H * W, 4), sentinel, dtype=torch.float64, device=DEV)
    pixel = torch.full((B * H * W,), -7, dtype=torch.int32, device=DEV)
    offsets = torch.full((B + 1,), -7, dtype=torch.int64, device=DEV)
    keep, exist = dev(c["keep"]).to(torch.uint8), dev(c["exist"]).to(torch.uint8)
    rc = L.sdp_range_unproject(x.data_ptr(), B, C, H, W, 0, _lib.ptr(origins), _lib.ptr(poses), keep.data_ptr(),
                               exist.data_ptr(), 1.5, points.data_ptr(), pixel.data_ptr(), offsets.data_ptr(),
                               ws.data_ptr(), n.value - ws_short, _lib.stream())
    torch.cuda.synchronize()
    return rc, points, pixel, offsets


@pytest.mark.parametrize("shape", [(3, 5, 48), (2, 64, 1024)])
def test_rows_past_the_total_are_not_written(shape):
    c = case(*shape)
    rc, points, pixel, offsets = raw_call(c, origins=dev(c["origins"]))
    assert rc == 0
    n = int(offsets[-1])
    assert 0 < n < points.shape[0]
    assert (points[n:] == -7.0).all() and (pixel[n:] == -7).all()
    assert (pixel[:n] >= 0).all() and (points[:n, 3] != -7.0).all()


@pytest.mark.parametrize("shape", [(3, 5, 48), (2, 64, 1024)])
def test_round_trip_through_the_device_projection(shape):
    """sdp_range_project of each view's slice at its origin gives index == rank and depth == rd
    (1e-13 relative); image row H-1 / column W-1 (inGrid) and dropped pixels come back empty."""
    from sdp.projection import project_device
    c = case(*shape)
    B, H, W = shape
    pts, off, pix = run(c, 2, "origins", True, "dataset")
    off = off.cpu().numpy()
    _, _, _, rd = ref(c, 2, "origins", True, "dataset")
    for b in range(B):
        r = project_device(pts[int(off[b]):int(off[b + 1])], c["origins"][b], H, W, with_intensity=True)
        idx, depth = r["index"].cpu().numpy().reshape(-1), r["depth"].cpu().numpy().reshape(-1)
        with np.errstate(invalid="ignore"):
            kept = ((rd[b] > np.float32(1.5)) & c["keep"][b] & c["exist"]).reshape(-1)
        ii, jj = np.divmod(np.arange(H * W), W)
        seen = kept & (ii != H - 1) & (jj != W - 1)
        np.testing.assert_array_equal(idx, np.where(seen, np.cumsum(kept) - 1, -1))
        want = np.where(seen, rd[b].reshape(-1).astype(np.float64), 2057.701)
        assert (np.abs(depth - want) <= 1e-13 * want).all()


def test_two_calls_are_bit_identical():
    c = case(*BIG[0])
    a = run(c, 2, "poses", True, "dataset")
    b = run(c, 2, "poses", True, "dataset")
    assert torch.equal(a[0].view(torch.int64), b[0].view(torch.int64))
    assert torch.equal(a[1], b[1]) and torch.equal(a[2], b[2])


@pytest.mark.parametrize("what", ["both_transforms", "C3", "short_workspace"])
def test_errors_are_reported_and_nothing_is_written(what):
    from sdp import _lib
    c = case(3, 5, 48)
    kw = dict(both_transforms=dict(origins=dev(c["origins"]), poses=dev(c["poses"])), C3=dict(C=3),
              short_workspace=dict(ws_short=1))[what]
    rc, points, pixel, offsets = raw_call(c, **kw)
    assert rc != 0 and len(_lib.lib().sdp_last_error()) > 0
    assert (points == -7.0).all() and (pixel == -7).all() and (offsets == -7).all()


def test_python_wrapper_rejects_both_transforms():
    from sdp.pointcloud import range_image_to_point_cloud
    c = case(3, 5, 48)
    with pytest.raises(RuntimeError, match="exclusive"):
        range_image_to_point_cloud(dev(c["x"]), origins=dev(c["origins"]), poses=dev(c["poses"]))


def test_fuse_views_and_write_bin(tmp_path):
    from sdp.pointcloud import fuse_views, write_bin
    c = case(3, 5, 48)
    cloud = fuse_views(dev(c["x"]), origins=dev(c["origins"]), keep=dev(c["keep"]), exist=dev(c["exist"]))
    rp = ref(c, 2, "origins", True, "dataset")[0]
    assert cloud.shape == rp.shape
    write_bin(str(tmp_path / "c.bin"), cloud)
    back = np.fromfile(str(tmp_path / "c.bin"), dtype=np.float32).reshape(-1, 4)
    np.testing.assert_array_equal(back, cloud.cpu().numpy().astype(np.float32))
