"""KITTI-360 view rendering on the GPU (sdp/kitti360.py over sdp_view_transform /
sdp_range_project / sdp_view_gather / sdp_view_finalize) against the numpy restatement of the
datasets' __getitem__ (oracle/kitti_ref.py, projection pinned to the reference's outputs).

Bar: masks, sky, index and the pose matrices bit-exact on every pixel; the float64 images to 1e-13
relative (device log2 vs the host libm).  The point transform sums the 4 products left to right
where numpy's matmul goes through BLAS, so coordinates may differ in the last bit, and the device
atan2 from libm's by a few ulp: together below 1e-12 bins.  A pixel assignment could only change
for a point that close to a bin edge, and every cloud the oracle projects here first passes
kernel_ref.bin_edge_guard (no point within 1e-9 bins of an edge that decides its pixel), computed
from the reference's arithmetic alone."""
import numpy as np
import pytest
import torch

import kernel_ref as KR
from kitti_tree import config, write_tree
from oracle import kitti_ref
from sdp import kitti360

pytestmark = pytest.mark.gpu
H, W = 64, 1024


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    root = str(tmp_path_factory.mktemp("kitti360"))
    write_tree(root, n_poses=24, n_points=40000)
    return root


@pytest.fixture(autouse=True)
def guarded_oracle(monkeypatch):
    """Every cloud the oracle projects (the view, the goal scan, the densification input) passes the bin-edge guard."""
    project = kitti_ref.point_cloud_to_range_image

    def guarded(pc, origin, return_remission=False, rowMax=64, colMax=1024):
        assert KR.bin_edge_guard(pc, origin, rowMax, colMax) > KR.BIN_EDGE_EPS
        return project(pc, origin, return_remission, rowMax=rowMax, colMax=colMax)
    monkeypatch.setattr(kitti_ref, "point_cloud_to_range_image", guarded)


def _check(got, want):
    names = ["real", "notmask", "notsky", "index", "toWorld", "fromWorld", "goal", "toOGView", "initialScan"]
    for n, g, w in zip(names, got, want):
        if n in ("real", "goal"):
            assert g.shape == w.shape and g.dtype == w.dtype, n
            np.testing.assert_allclose(g, w, rtol=1e-13, atol=0, err_msg=n)
        elif n == "initialScan":
            assert g == w
        else:
            assert g.shape == w.shape, (n, g.shape, w.shape)
            assert np.array_equal(g, w), (n, int(np.sum(g != w)))


CLASSES = {0: kitti360.KITTI360_im_8batch, 1: kitti360.KITTI360_im_AllForOne,
           2: kitti360.KITTI360_im_simultaneous_densification}


@pytest.mark.parametrize("variant", [0, 1, 2])
@pytest.mark.parametrize("idx", [0, 1, 3, 22])
def test_item_matches_oracle(tree, variant, idx):
    cfg = config(4)
    ds = CLASSES[variant]("unused", cfg, split="test", root=tree, device="cuda")
    np.random.seed(11)
    got = ds[idx]
    np.random.seed(11)
    want = kitti_ref.item(tree, variant, idx, 4, cfg.data.modifications, H, W)
    _check(got, want)


@pytest.mark.parametrize("variant", [0, 2])
def test_item_with_random_roll(tree, variant):
    cfg = config(4, random_roll=True)
    ds = CLASSES[variant]("unused", cfg, split="test", root=tree, device="cuda")
    np.random.seed(7)
    got = ds[5]
    np.random.seed(7)
    want = kitti_ref.item(tree, variant, 5, 4, cfg.data.modifications, H, W, random_roll=True)
    _check(got, want)


def test_transform_matches_numpy(tree):
    ds = kitti360.KITTI360_im_8batch("unused", config(4), split="test", root=tree, device="cuda")
    scan = kitti360.load_velodyne(ds._scan_name(ds.frames[2]))
    m1 = ds.Tr_pose_world[ds.frames[2]]
    m2 = np.linalg.inv(ds.Tr_pose_world[ds.frames[7]])
    _, out = ds._to_view(scan, m1, m2)
    pv = np.concatenate((scan[:, :3].T, np.ones((1, len(scan)), np.float32)), 0)
    ref = np.matmul(m2, np.matmul(m1, pv))
    got = out.cpu().numpy()
    np.testing.assert_allclose(got[:, :3], ref[:3].T, rtol=1e-14, atol=1e-12)
    assert np.array_equal(got[:, 3], scan[:, 3].astype(np.float64))


def test_gather_keeps_row_major_order(tree):
    ds = kitti360.KITTI360_im_simultaneous_densification("unused", config(4), split="test", root=tree, device="cuda")
    ds.device = torch.device("cuda")
    scan = kitti360.load_velodyne(ds._scan_name(ds.frames[0]))
    raw, p64 = ds._to_view(scan)
    _, _, _, _, idx = ds._project(p64, [0, 0, 0])
    from sdp import _lib
    sub = torch.empty(H * W, 4, dtype=torch.float64, device="cuda")
    cnt = torch.zeros(1, dtype=torch.int32, device="cuda")
    _lib.check(_lib.lib().sdp_view_gather(idx.data_ptr(), H, W, W // 4, raw.data_ptr(), sub.data_ptr(), cnt.data_ptr(),
                                          _lib.stream()), "gather")
    ind = idx.cpu().numpy().copy()
    ind[:, :W // 4] = -2
    want = scan[ind[ind >= 0].astype(int)].astype(np.float64)
    n = int(cnt.item())
    assert n == len(want)
    assert np.array_equal(sub[:n].cpu().numpy(), want)
