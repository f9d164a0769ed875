"""main.py --sample --save_clouds --cloud_grid DL end to end on the GPU (modelled on tests/test_gpu_runner_clouds.py,
same reduced configs): besides the unchanged _Cloud_ / _CloudOffsets_ files every sampled doThis writes
{stem}_CloudGrid_{ckpt}.npy, which must equal tests/voxel_ref.py applied to the _Cloud_ file of the same run
-- on float32(cloud - center), the barycentres added back to center in float64, the intensity as the one
feature -- with center the translation of the first view's pose (Line) or its origin (completion).  The
_Cloud_ and _CloudOffsets_ files equal those of a run without the flag, which writes no _CloudGrid_ file.
"""
import os

import numpy as np
import pytest
import yaml

import main as sdp_main
import voxel_ref as VR

pytestmark = pytest.mark.gpu
CFG_DIR = os.path.join(os.path.dirname(sdp_main.__file__), "configs")
H, W = 64, 256
DL = 0.2


def _expected(cloud, center):
    q = (cloud[:, :3] - center).astype(np.float32)
    r = VR.subsample(q, cloud[:, 3:4].astype(np.float32), None, DL)
    return np.concatenate([r["points"].astype(np.float64) + center, r["features"].astype(np.float64)], 1)


def _check_grid(out, stem, center):
    cloud = np.load(out / f"{stem}_Cloud_897.npy")
    grid = np.load(out / f"{stem}_CloudGrid_897.npy")
    assert grid.dtype == np.float64 and grid.ndim == 2 and grid.shape[1] == 4
    assert 0 < len(grid) < len(cloud)
    np.testing.assert_array_equal(grid, _expected(cloud, center))


def test_line_cloud_grid(tmp_path):
    with open(os.path.join(CFG_DIR, "HDVMine_Line.yml")) as f:
        c = yaml.safe_load(f)
    c["sampling"].update(batch_size=6, actualBatchSize=3, n_steps_each=1)
    c["data"].update(image_width=W, modifications=c["data"]["modifications"][:3])
    c["model"]["num_classes"] = 4
    cfg = tmp_path / "small.yml"
    cfg.write_text(yaml.safe_dump(c))
    base = ["--config", str(cfg), "--sample", "--save_clouds", "--ni", "--verbose", "warning"]
    assert sdp_main.main(base + ["--exp", str(tmp_path / "grid"), "--cloud_grid", str(DL)]) == 0
    assert sdp_main.main(base + ["--exp", str(tmp_path / "plain")]) == 0
    out = tmp_path / "grid" / "image_samples" / "images"
    plain = tmp_path / "plain" / "image_samples" / "images"
    assert not list(plain.glob("*CloudGrid*"))
    to_world = np.load(out / "toWorld_0_3_.npy").reshape(6, 4, 4)
    for do in range(3):
        stem = f"{do}_0_3_"
        _check_grid(out, stem, to_world[0][:3, 3].astype(np.float64))
        for kind in ("Cloud", "CloudOffsets"):
            a, b = np.load(out / f"{stem}_{kind}_897.npy"), np.load(plain / f"{stem}_{kind}_897.npy")
            assert a.dtype == b.dtype and np.array_equal(a, b)


def test_completion_cloud_grid(tmp_path):
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
    assert sdp_main.main(["--config", str(cfg), "--sample", "--save_clouds", "--cloud_grid", str(DL), "--ni", "--exp",
                          str(tmp_path / "exp"), "--verbose", "warning", "--kitti_root", str(root)]) == 0
    out = tmp_path / "exp" / "image_samples" / "images"
    origins = np.load(out / "0_000000_ORIGINS_897.pth.npy").reshape(5, 3).astype(np.float64)
    _check_grid(out, "1_000000", origins[0])
