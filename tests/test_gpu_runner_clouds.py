"""main.py --sample --save_clouds end to end on the GPU: the fused clouds the runners write are
the inverse of the projection the saved range images came from.

Setups: the reduced Line config of tests/test_gpu_runner.py (6 procedural views of 64x256 in
megabatches of 3) and the scene-completion setup of tests/test_gpu_completion.py (one synthetic SSC
scan, 5 views); both with 4 sigma levels, which keeps a run to a few seconds and still reaches the
merge (it starts at level 2).  For every sampled doThis the two files exist, the offsets are monotone
and end at the row count, and re-projecting each view's slice on the CPU projection oracle -- at the
view's origin (completion) or after fromWorld = inv(toWorld) (kitti) -- hits exactly the pixels that
are in the exist mask, not sky and farther than 1.5 m, with the un-logged depth of the saved
Masked_completion image (1e-10 relative: the clouds are float64 and the poses rigid motions of tens
to hundreds of metres).  Image row H-1 and column W-1 are outside the projection's inGrid and come
back empty.

The same check runs on views rendered from a KITTI-360 tree (tests/kitti_tree.py: rotated poses
hundreds of metres from the world origin) for the Line config and for the Circle (AllForOne) config,
whose views share one pose frame and are rendered from data.modifications[j] inside it: each slice
is re-projected at modifications[j] after inv(toWorld).  The projection clears its sky mask
(lidar_utils.py:304), so no saved SKY file ever drops a pixel; the polarity of the not-sky mask is
therefore checked on ``Runner._save_clouds`` directly, with a hand-made mask.
"""
import os

import numpy as np
import pytest
import yaml

import main as sdp_main
import pointcloud_ref as PR
from oracle import projection_ref as P

pytestmark = pytest.mark.gpu
CFG_DIR = os.path.join(os.path.dirname(sdp_main.__file__), "configs")
H, W = 64, 256


def _line_cfg(tmp_path):
    with open(os.path.join(CFG_DIR, "HDVMine_Line.yml")) as f:
        c = yaml.safe_load(f)
    c["sampling"].update(batch_size=6, actualBatchSize=3, n_steps_each=1)
    c["data"].update(image_width=W, modifications=c["data"]["modifications"][:3])
    c["model"]["num_classes"] = 4
    cfg = tmp_path / "small.yml"
    cfg.write_text(yaml.safe_dump(c))
    return cfg


def _check_view(cloud, code, keep, origin=None, from_world=None):
    """cloud [n,4] of one view, code [H,W] its saved depth code, keep [H,W] exist & not sky."""
    pts = cloud.copy()
    if from_world is not None:
        pts[:, :3] = (from_world[:3, :3] @ cloud[:, :3].T).T + from_world[:3, 3]
    depth, _, _, _, _, idx = P.point_cloud_to_range_image(pts, np.zeros(3) if origin is None else origin,
                                                          return_remission=True, rowMax=H, colMax=W)
    rd = PR.distance(code)
    kept = (keep & (rd > np.float32(1.5))).reshape(-1)
    assert kept.sum() == len(cloud)
    ii, jj = np.divmod(np.arange(H * W), W)
    seen = kept & (ii != H - 1) & (jj != W - 1)
    np.testing.assert_array_equal(idx.reshape(-1), np.where(seen, np.cumsum(kept) - 1, -1))
    want = rd.reshape(-1).astype(np.float64)[seen]
    assert seen.sum() > 0
    assert (np.abs(depth.reshape(-1)[seen] - want) <= 1e-10 * want).all()


def _check_offsets(off, cloud, n_views):
    assert off.dtype == np.int64 and off.shape == (n_views + 1,) and off[0] == 0
    assert (np.diff(off) >= 0).all() and off[-1] == len(cloud)
    assert cloud.dtype == np.float64 and cloud.ndim == 2 and cloud.shape[1] == 4


def test_line_clouds_invert_the_saved_images(tmp_path):
    from sdp import synthetic
    cfg = _line_cfg(tmp_path)
    assert sdp_main.main(["--config", str(cfg), "--sample", "--save_clouds", "--ni", "--exp", str(tmp_path / "exp"),
                          "--verbose", "warning"]) == 0
    out = tmp_path / "exp" / "image_samples" / "images"
    exist = synthetic.exist_mask(H, W)
    to_world = np.load(out / "toWorld_0_3_.npy").reshape(6, 4, 4)
    notsky = np.load(out / "0_0_3__SKY_897.pth.npy").reshape(6, H, W).astype(bool)
    for do, k in enumerate([2, 3, 3]):           # views of every megabatch of 3 that doThis samples
        views = [m * 3 + v for m in range(2) for v in range(k)]
        cloud = np.load(out / f"{do}_0_3__Cloud_897.npy")
        off = np.load(out / f"{do}_0_3__CloudOffsets_897.npy")
        _check_offsets(off, cloud, len(views))
        masked = np.load(out / f"{do}_0_3__Masked_completion_897.pth.npy")
        assert masked.shape[0] == 2 * len(views)
        for i, v in enumerate(views):
            sl = cloud[off[i]:off[i + 1]]
            _check_view(sl, masked[i, 0], exist & notsky[v], from_world=np.linalg.inv(to_world[v]))
            np.testing.assert_array_equal(sl[:, 3], masked[len(views) + i, 0].astype(np.float64).reshape(-1)[
                (exist & notsky[v] & (PR.distance(masked[i, 0]) > np.float32(1.5))).reshape(-1)])


def test_completion_clouds_invert_the_saved_images(tmp_path):
    from sdp import synthetic
    from ssc_tree import write_ssc_tree
    root = tmp_path / "KITTI-360"
    write_ssc_tree(str(root), n_scans=1)
    with open(os.path.join(CFG_DIR, "HDVMineCompletion.yml")) as f:
        c = yaml.safe_load(f)
    c["data"]["image_width"] = W
    c["sampling"]["n_steps_each"] = 1
    c["model"]["num_classes"] = 4
    cfg = tmp_path / "completion.yml"
    cfg.write_text(yaml.safe_dump(c))
    assert sdp_main.main(["--config", str(cfg), "--sample", "--save_clouds", "--ni", "--exp", str(tmp_path / "exp"),
                          "--verbose", "warning", "--kitti_root", str(root)]) == 0
    out = tmp_path / "exp" / "image_samples" / "images"
    assert not list(out.glob("0_*Cloud*")), "doThis 0 samples nothing"
    exist = synthetic.exist_mask(H, W)
    origins = np.load(out / "0_000000_ORIGINS_897.pth.npy").reshape(5, 3)
    notsky = np.load(out / "0_000000_SKY_897.pth.npy").reshape(5, H, W).astype(bool)
    cloud = np.load(out / "1_000000_Cloud_897.npy")
    off = np.load(out / "1_000000_CloudOffsets_897.npy")
    _check_offsets(off, cloud, 5)
    masked = np.load(out / "1_000000_Masked_completion_897.pth.npy")
    for v in range(5):
        _check_view(cloud[off[v]:off[v + 1]], masked[v, 0], exist & notsky[v], origin=origins[v])


def test_without_the_flag_no_cloud_is_written(tmp_path):
    cfg = _line_cfg(tmp_path)
    assert sdp_main.main(["--config", str(cfg), "--sample", "--ni", "--exp", str(tmp_path / "exp"),
                          "--verbose", "warning"]) == 0
    out = tmp_path / "exp" / "image_samples" / "images"
    names = sorted(p.name for p in out.iterdir())
    assert any("Masked_completion" in n for n in names)
    assert not [n for n in names if "Cloud" in n], names


@pytest.mark.parametrize("name", ["HDVMine_Line.yml", "HDVMine_Circle.yml"])
def test_kitti_tree_clouds_invert_the_saved_images(tmp_path, name):
    from kitti_tree import write_tree
    from sdp import synthetic
    root = tmp_path / "KITTI-360"
    write_tree(str(root), n_poses=40, n_points=20000)
    with open(os.path.join(CFG_DIR, name)) as f:
        c = yaml.safe_load(f)
    c["sampling"].update(batch_size=3, actualBatchSize=3, n_steps_each=1)
    c["data"].update(image_width=W, modifications=c["data"]["modifications"][:3])
    c["model"]["num_classes"] = 4
    cfg = tmp_path / "small.yml"
    cfg.write_text(yaml.safe_dump(c))
    assert sdp_main.main(["--config", str(cfg), "--sample", "--save_clouds", "--ni", "--exp", str(tmp_path / "exp"),
                          "--verbose", "warning", "--kitti_root", str(root)]) == 0
    out = tmp_path / "exp" / "image_samples" / "images"
    (tw,) = list(out.glob("toWorld_*.npy"))
    save_num = tw.name[len("toWorld_"):-len(".npy")]
    to_world = np.load(tw).reshape(3, 4, 4)
    kitti = "Line" in name
    mods = np.asarray(c["data"]["modifications"], dtype=np.float64)
    if not kitti:
        assert np.abs(mods).max() >= 5 and np.array_equal(to_world[0], to_world[1])   # one pose frame, distinct origins
    exist = synthetic.exist_mask(H, W)
    notsky = np.load(out / f"0_{save_num}_SKY_897.pth.npy").reshape(3, H, W).astype(bool)
    for do, k in enumerate([2, 3, 3] if kitti else [2, 3, 1]):
        cloud = np.load(out / f"{do}_{save_num}_Cloud_897.npy")
        off = np.load(out / f"{do}_{save_num}_CloudOffsets_897.npy")
        _check_offsets(off, cloud, k)
        masked = np.load(out / f"{do}_{save_num}_Masked_completion_897.pth.npy")
        assert masked.shape[0] == 2 * k
        for v in range(k):
            _check_view(cloud[off[v]:off[v + 1]], masked[v, 0], exist & notsky[v],
                        origin=None if kitti else mods[v], from_world=np.linalg.inv(to_world[v]))


def test_save_clouds_drops_sky_pixels(tmp_path):
    """notsky is True where a pixel is NOT sky: a hand-made mask with a block of sky in view 1 only."""
    import argparse
    import torch
    from sdp import synthetic
    from sdp.runner import Runner
    with open(os.path.join(CFG_DIR, "HDVMine_Line.yml")) as f:
        cfg = sdp_main.dict2namespace(yaml.safe_load(f))
    cfg.device = torch.device("cuda")
    r = Runner(argparse.Namespace(image_folder=str(tmp_path), save_clouds=True, kitti_root=None), cfg)
    g = np.random.default_rng(11)
    sample = torch.from_numpy(g.uniform(0.3, 1.0, (2, 2, H, W)).astype(np.float32))      # every rd > 1.5
    notsky = np.ones((2, 1, H, W), bool)
    notsky[1, 0, 10:20, 30:200] = False
    r._save_clouds("t", 897, sample, torch.from_numpy(notsky))
    cloud, off = np.load(tmp_path / "t_Cloud_897.npy"), np.load(tmp_path / "t_CloudOffsets_897.npy")
    exist = synthetic.exist_mask(H, W)
    assert exist[10:20, 30:200].sum() > 0
    np.testing.assert_array_equal(np.diff(off), [exist.sum(), (exist & notsky[1, 0]).sum()])
    for v in range(2):
        _check_view(cloud[off[v]:off[v + 1]], sample[v, 0].numpy(), exist & notsky[v, 0])
