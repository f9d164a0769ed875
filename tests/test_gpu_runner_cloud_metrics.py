"""main.py --sample --save_clouds --cloud_metrics R end to end on the GPU (modelled on tests/test_gpu_runner_cloud_grid.py,
same reduced configs).  Besides the unchanged files every sampled doThis writes
  {stem}_CloudRef_ / _CloudRefOffsets_  the run's reference images (GT_completion for the Line config -- the masked
                                        input, the reference's quirk; the masked input for scene completion) of the
                                        sampled views, fused like _Cloud_: equal to tests/pointcloud_ref.py on the saved
                                        images within the gate of tests/test_gpu_unproject.py;
  {stem}_CloudDist_                     sqrt(nn_d2) sampled -> reference: bit-equal to tests/cloud_nn_ref.py applied to
                                        the saved _Cloud_ and _CloudRef_ files;
  {stem}_CloudMetrics_                  rows 0-1 the reference's stats of both directions (counts and maximum exact, sums
                                        within cloud_nn_ref.sum_bound), row 2 the arguments.
The _Cloud_, _CloudOffsets_ and Masked_completion files equal those of a run without the flag byte for byte, and that
run writes none of the four files.  --cloud_metrics without --save_clouds is an argparse error.
"""
import os

import numpy as np
import pytest
import yaml

import cloud_nn_ref as NR
import main as sdp_main
import pointcloud_ref as PR

pytestmark = pytest.mark.gpu
CFG_DIR = os.path.join(os.path.dirname(sdp_main.__file__), "configs")
H, W = 64, 256
R = 0.5
THR = (0.1, 0.2, 0.5)
NEW = ("CloudRef", "CloudRefOffsets", "CloudDist", "CloudMetrics")


def _check_metrics(out, stem, R=R, cell=R, thr=THR):
    cloud = np.load(out / f"{stem}_Cloud_897.npy")
    ref = np.load(out / f"{stem}_CloudRef_897.npy")
    dist = np.load(out / f"{stem}_CloudDist_897.npy")
    met = np.load(out / f"{stem}_CloudMetrics_897.npy")
    assert ref.dtype == np.float64 and ref.ndim == 2 and ref.shape[1] == 4 and len(ref) > 1000 and len(cloud) > 1000
    ab, ba = NR.nearest(cloud, ref, R), NR.nearest(ref, cloud, R)
    assert dist.dtype == np.float64 and dist.shape == (len(cloud),)
    np.testing.assert_array_equal(dist.view(np.int64), np.sqrt(ab[0]).view(np.int64))
    assert met.dtype == np.float64 and met.shape == (3, 5 + len(thr))
    for row, d2, q in ((0, ab[0], cloud), (1, ba[0], ref)):
        want = NR.stats(d2, q, thr)
        np.testing.assert_array_equal(met[row][[0, 1, 4]], want[[0, 1, 4]])
        np.testing.assert_array_equal(met[row][5:], want[5:])
        for k in (2, 3):
            assert abs(met[row][k] - want[k]) <= NR.sum_bound(int(want[1]), want[k])
        assert want[0] == len(q) and 0 < want[1]
    np.testing.assert_array_equal(met[2], np.array([R, cell, len(thr), 0, 0] + list(thr)))
    return cloud, ref


def _check_reference_cloud(out, stem, images, n_all, views, keep, **place):
    """_CloudRef_ against pointcloud_ref on the saved reference images (grid layout [2 n_all, 3, H, W])."""
    x = np.stack([np.stack([images[v, 0], images[n_all + v, 0]]) for v in views]).astype(np.float32)
    rd = PR.distance(x[:, 0])
    assert not (np.abs(rd - np.float32(1.5)) < 1e-5).any()       # the float32 keep compare cannot differ
    rp, ro, _, _ = PR.unproject(x, keep=keep, exist=None, min_range=1.5, geometry="dataset", **place)
    ref = np.load(out / f"{stem}_CloudRef_897.npy")
    off = np.load(out / f"{stem}_CloudRefOffsets_897.npy")
    assert off.dtype == np.int64
    np.testing.assert_array_equal(off, ro)
    assert ref.shape == rp.shape
    scale = max(1.0, float(np.abs(rp[:, :3]).max()))
    assert float(np.abs(ref[:, :3] - rp[:, :3]).max()) <= 1e-12 * scale
    assert np.array_equal(ref[:, 3].view(np.int64), rp[:, 3].view(np.int64))


def _same_files(a, b, names):
    for name in names:
        x, y = np.load(a / name), np.load(b / name)
        assert x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes(), name


def _line_cfg(tmp_path):
    with open(os.path.join(CFG_DIR, "HDVMine_Line.yml")) as f:
        c = yaml.safe_load(f)
    c["sampling"].update(batch_size=6, actualBatchSize=3, n_steps_each=1)
    c["data"].update(image_width=W, modifications=c["data"]["modifications"][:3])
    c["model"]["num_classes"] = 4
    cfg = tmp_path / "small.yml"
    cfg.write_text(yaml.safe_dump(c))
    return cfg


def test_line_cloud_metrics(tmp_path):
    from sdp import synthetic
    cfg = _line_cfg(tmp_path)
    base = ["--config", str(cfg), "--sample", "--save_clouds", "--ni", "--verbose", "warning"]
    assert sdp_main.main(base + ["--exp", str(tmp_path / "met"), "--cloud_metrics", str(R)]) == 0
    assert sdp_main.main(base + ["--exp", str(tmp_path / "plain")]) == 0
    out = tmp_path / "met" / "image_samples" / "images"
    plain = tmp_path / "plain" / "image_samples" / "images"
    for kind in NEW:
        assert not list(plain.glob(f"*_{kind}_*"))
    exist = synthetic.exist_mask(H, W)
    to_world = np.load(out / "toWorld_0_3_.npy").reshape(6, 4, 4)
    notsky = np.load(out / "0_0_3__SKY_897.pth.npy").reshape(6, H, W).astype(bool)
    gt = np.load(out / "0_0_3__GT_completion_897.pth.npy")
    for do, k in enumerate([2, 3, 3]):
        stem = f"{do}_0_3_"
        views = [m * 3 + v for m in range(2) for v in range(k)]
        _check_metrics(out, stem)
        _check_reference_cloud(out, stem, gt, 6, views, np.stack([exist & notsky[v] for v in views]),
                               poses=to_world[views])
        _same_files(out, plain, [f"{stem}_Cloud_897.npy", f"{stem}_CloudOffsets_897.npy",
                                 f"{stem}_Masked_completion_897.pth.npy"])


def test_line_cloud_metrics_cell_and_small_radius(tmp_path):
    cfg = _line_cfg(tmp_path)
    assert sdp_main.main(["--config", str(cfg), "--sample", "--save_clouds", "--ni", "--verbose", "warning", "--exp",
                          str(tmp_path / "exp"), "--cloud_metrics", "0.25", "--cloud_metrics_cell", "0.125"]) == 0
    out = tmp_path / "exp" / "image_samples" / "images"
    _check_metrics(out, "0_0_3_", R=0.25, cell=0.125, thr=tuple(t * 0.5 for t in THR))


def test_completion_cloud_metrics(tmp_path):
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
    base = ["--config", str(cfg), "--sample", "--save_clouds", "--ni", "--verbose", "warning", "--kitti_root", str(root)]
    assert sdp_main.main(base + ["--exp", str(tmp_path / "met"), "--cloud_metrics", str(R)]) == 0
    assert sdp_main.main(base + ["--exp", str(tmp_path / "plain")]) == 0
    out = tmp_path / "met" / "image_samples" / "images"
    plain = tmp_path / "plain" / "image_samples" / "images"
    for kind in NEW:
        assert not list(plain.glob(f"*_{kind}_*")) and not list(out.glob(f"0_*_{kind}_*"))
    exist = synthetic.exist_mask(H, W)
    origins = np.load(out / "0_000000_ORIGINS_897.pth.npy").reshape(5, 3).astype(np.float64)
    notsky = np.load(out / "0_000000_SKY_897.pth.npy").reshape(5, H, W).astype(bool)
    inp = np.load(out / "0_000000_Input_completion_897.pth.npy")
    _check_metrics(out, "1_000000")
    _check_reference_cloud(out, "1_000000", inp, 5, list(range(5)), exist[None] & notsky, origins=origins)
    _same_files(out, plain, ["1_000000_Cloud_897.npy", "1_000000_CloudOffsets_897.npy",
                             "1_000000_Masked_completion_897.pth.npy"])


def test_cloud_metrics_needs_save_clouds(tmp_path, capsys):
    cfg = _line_cfg(tmp_path)
    base = ["--config", str(cfg), "--sample", "--ni", "--exp", str(tmp_path / "exp")]
    for extra in (["--cloud_metrics", "0.5"], ["--save_clouds", "--cloud_metrics_cell", "0.5"],
                  ["--save_clouds", "--cloud_metrics", "0.5", "--cloud_metrics_cell", "0.6"]):
        with pytest.raises(SystemExit) as e:
            sdp_main.main(base + extra)
        assert e.value.code == 2
    assert "--cloud_metrics needs --save_clouds" in capsys.readouterr().err
