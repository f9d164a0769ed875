"""CPU checks of the range image -> point cloud path: the C ABI is declared, exported and bound, and
the float64 restatement that grades the kernel (tests/pointcloud_ref.py) inverts the projection
oracle, which is itself pinned to the reference's own outputs (tests/golden/projection_*.npz).

Round trip: unproject a random code image with the dataset geometry and per-view origins, feed each
view's kept points to ``oracle.projection_ref.point_cloud_to_range_image`` at the same origin.  Then
  * the index image equals each kept pixel's compaction rank inside its view;
  * image row H-1, column W-1 (``inGrid`` excludes pre-flip row and column 0) and dropped pixels come
    back -1 / MAX_RANGE;
  * the depth equals rd within 1e-14 relative (worst seen: 4.8e-16);
  * every point lies on the centre of its bin: |fractional bin| <= 1e-9 in both axes.  atan2 is good
    to a few ulp of pi (~1e-15 rad) and the smallest bin here is 6e-3 rad, so an exact inverse stays
    below ~1e-12 bin.  This is what sees the sampler's vertical origin: it sits 0.04 - 0.36 bin from the
    dataset's at these heights, which np.round alone would absorb.
Each mutant of the restatement (no flip, sampler vMin, arange(W) columns, view-minor order) must fail it.
"""
import os
import re
import subprocess

import numpy as np
import pytest

import pointcloud_ref as PR
from conftest import PKG_DIR, REPO
from oracle import projection_ref as P

HEADER = os.path.join(REPO, "include", "sdp.h")
LIB = os.path.join(PKG_DIR, "sdp", "_lib", "libsdp.so")
SYMBOLS = ("sdp_range_unproject_workspace_size", "sdp_range_unproject")
SHAPES = [(2, 64, 1024), (2, 16, 1000), (3, 5, 48), (2, 3, 7)]


def test_header_declares_the_unprojection():
    src = open(HEADER).read()
    for s in SYMBOLS:
        assert re.search(r"^\s*int\s+" + s + r"\s*\(", src, re.M), s
    assert re.search(r"SDP_GEOM_DATASET\s*=\s*0\s*,\s*SDP_GEOM_SAMPLER\s*=\s*1", src)


def test_library_exports_the_unprojection():
    assert os.path.exists(LIB), "build libsdp.so first (python __graft_entry__.py build)"
    out = subprocess.run(["nm", "-D", "--defined-only", LIB], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r" T (sdp_\w+)", out))
    assert set(SYMBOLS) <= exported


def test_ctypes_table_binds_the_unprojection():
    from sdp import _lib
    L = _lib.lib()
    for s in SYMBOLS:
        assert s in _lib.exported_symbols()
        assert getattr(L, s).restype is _lib.I
    assert len(L.sdp_range_unproject.argtypes) == 17 and len(L.sdp_range_unproject_workspace_size.argtypes) == 4


def test_argument_errors_need_no_device():
    """The argument checks run before anything is launched, so they answer on a machine without a GPU."""
    from sdp import _lib
    L = _lib.lib()
    n = _lib.SZ()
    assert L.sdp_range_unproject_workspace_size(0, 64, 1024, _lib.C.byref(n)) != 0
    # every view padded to whole 256-pixel chunks, B of them, must stay below 2^31 (int32 pixel ids)
    assert L.sdp_range_unproject_workspace_size(1, 1, 2 ** 31 - 100, _lib.C.byref(n)) != 0
    assert L.sdp_range_unproject_workspace_size(32768, 256, 256, _lib.C.byref(n)) != 0
    assert L.sdp_range_unproject_workspace_size(32767, 256, 256, _lib.C.byref(n)) == 0
    assert L.sdp_range_unproject_workspace_size(2, 64, 1024, _lib.C.byref(n)) == 0 and n.value > 0
    dummy = _lib.C.create_string_buffer(64)
    p = _lib.C.addressof(dummy)
    common = (None, None, 1.5, p, None, p, p)
    assert L.sdp_range_unproject(p, 1, 3, 3, 7, 0, None, None, *common, n.value, None) != 0
    assert b"C must be 1 or 2" in L.sdp_last_error()
    assert L.sdp_range_unproject(p, 1, 2, 3, 7, 0, p, p, *common, n.value, None) != 0
    assert b"exclusive" in L.sdp_last_error()
    assert L.sdp_range_unproject(p, 1, 2, 0, 7, 0, None, None, *common, n.value, None) != 0
    assert L.sdp_range_unproject(p, 2, 2, 64, 1024, 0, None, None, *common, n.value - 1, None) != 0
    assert b"workspace" in L.sdp_last_error()


def _case(B, H, W):
    r = np.random.default_rng(B * 1000003 + H * 1009 + W)
    x = r.uniform(0.05, 1.0, (B, 2, H, W)).astype(np.float32)
    x[:, 0][r.random((B, H, W)) < 0.15] = 0.1          # rd = 0.52 <= 1.5: dropped
    x[:, 0][r.random((B, H, W)) < 0.05] *= -1          # negative codes count by their magnitude
    keep = r.random((B, H, W)) < 0.8
    exist = r.random((H, W)) < 0.9
    origins = r.uniform(-2.0, 2.0, (B, 3))
    return x, keep, exist, origins


def _round_trip(x, keep, exist, origins, geometry="dataset", mutant=None):
    """Returns the list of failed properties (empty = the restatement inverts the projection)."""
    B, C, H, W = x.shape
    pts, off, pixel, rd = PR.unproject(x, origins=origins, keep=keep, exist=exist, geometry=geometry, mutant=mutant)
    hA, vA, hMin, vMin = P.geometry(H, W)
    failed = set()
    worst = 0.0
    for b in range(B):
        cloud = pts[int(off[b]):int(off[b + 1])]              # a consumer's view slice
        depth, _, _, _, _, idx = P.point_cloud_to_range_image(cloud, origins[b], return_remission=True, rowMax=H,
                                                              colMax=W)
        # what must come back, from the codes and the masks alone
        rdb = PR.distance(x[b, 0])
        kept = ((rdb > np.float32(1.5)) & keep[b] & exist).reshape(-1)
        rank = np.cumsum(kept) - 1                            # row-major compaction rank
        ii, jj = np.divmod(np.arange(H * W), W)
        seen = kept & (ii != H - 1) & (jj != W - 1)           # inGrid drops pre-flip row 0 / column 0
        want_idx = np.where(seen, rank, -1).astype(np.float64)
        want_depth = np.where(seen, rdb.reshape(-1).astype(np.float64), P.MAX_RANGE)
        if not np.array_equal(idx.reshape(-1), want_idx):
            failed.add("index")
        rel = np.abs(depth.reshape(-1) - want_depth) / want_depth
        worst = max(worst, float(rel.max()))
        if rel.max() > 1e-14:
            failed.add("depth")
        q = cloud[:, :3] - origins[b]
        fc = (np.arctan2(q[:, 1], q[:, 0]) - hMin) / hA
        fr = (np.arctan2(q[:, 2], np.hypot(q[:, 0], q[:, 1])) - vMin) / vA
        if len(q) and max(np.abs(fc - np.rint(fc)).max(), np.abs(fr - np.rint(fr)).max()) > 1e-9:
            failed.add("centre")
    return failed, worst


@pytest.mark.parametrize("B,H,W", SHAPES)
def test_restatement_inverts_the_pinned_projection(B, H, W):
    failed, worst = _round_trip(*_case(B, H, W))
    print(f"round trip {B}x{H}x{W}: worst relative depth error {worst:.2e}")
    assert not failed, failed


@pytest.mark.parametrize("B,H,W", SHAPES[1:])
@pytest.mark.parametrize("mutant", ["no_flip", "sampler_vmin", "arange_cols", "view_minor"])
def test_round_trip_sees_each_mutant(B, H, W, mutant):
    case = _case(B, H, W)
    if mutant == "sampler_vmin":
        failed, _ = _round_trip(*case, geometry="sampler")
    else:
        failed, _ = _round_trip(*case, mutant=mutant)
    assert failed, f"the round trip accepted the {mutant} mutant"


def test_sampler_geometry_is_the_merge_tables():
    """geometry="sampler" restates KITTISampling.py:29-102 through the merge oracle's own tables."""
    from oracle.sampling_ref import merge_geometry
    for H, W in ((64, 1024), (5, 48), (3, 7)):
        az, el = PR.angles(H, W, "sampler")
        g = merge_geometry(H, W)
        np.testing.assert_array_equal(az, g["az"])
        np.testing.assert_allclose(el, g["el"], rtol=0, atol=1e-15)
        az_d, el_d = PR.angles(H, W, "dataset")
        np.testing.assert_array_equal(az_d, az)                # the two differ in the vertical origin only
        assert np.abs(el_d - el).max() > 0.03 * g["vA"]


def test_write_bin_round_trips_through_the_kitti_reader(tmp_path):
    from sdp import kitti360
    from sdp.pointcloud import write_bin
    pts = np.random.default_rng(3).normal(size=(17, 4))
    write_bin(str(tmp_path / "a.bin"), pts)
    back = np.fromfile(str(tmp_path / "a.bin"), dtype=np.float32).reshape(-1, 4)
    np.testing.assert_array_equal(back, pts.astype(np.float32))
    np.testing.assert_array_equal(kitti360.load_velodyne(str(tmp_path / "a.bin")), back)


def test_cloud_poses_place_allforone_views_at_their_modifications():
    """Views of the AllForOne / densification datasets from a KITTI tree share one pose frame and are
    rendered from data.modifications[j] inside it (sdp/kitti360.py): their sensor origin in the world is
    toWorld @ [modifications[j], 1].  The 8batch views and the procedural source use toWorld alone."""
    import argparse
    import torch
    from sdp.runner import Runner
    mods = [[0, 0, 0], [5, -5, 0], [-5, -5, 0]]
    th = 0.3
    T = np.array([[np.cos(th), -np.sin(th), 0, 100.0], [np.sin(th), np.cos(th), 0, 50.0], [0, 0, 1, 110.0], [0, 0, 0, 1]])
    to_world = torch.from_numpy(np.tile(T, (4, 1, 1)))            # 2 megabatches, k = 2 views kept of each
    cfg = argparse.Namespace(device=torch.device("cpu"),
                             data=argparse.Namespace(dataset="KITTI360_im_AllForOne", modifications=mods))
    r = Runner(argparse.Namespace(kitti_root="/some/tree"), cfg)
    poses = r._cloud_poses(to_world, 2, kitti=False).numpy()
    for v in range(4):
        np.testing.assert_allclose(poses[v] @ [0, 0, 0, 1], T @ np.array(mods[v % 2] + [1.0]), rtol=0, atol=1e-12)
        np.testing.assert_array_equal(poses[v][:3, :3], T[:3, :3])
    np.testing.assert_array_equal(r._cloud_poses(to_world, 2, kitti=True).numpy(), to_world.numpy())
    r2 = Runner(argparse.Namespace(kitti_root=None), cfg)
    np.testing.assert_array_equal(r2._cloud_poses(to_world, 2, kitti=False).numpy(), to_world.numpy())
