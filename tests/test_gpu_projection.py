"""GPU parity of the point cloud -> range image front end (csrc/projection.hip) against the
reference's own outputs (tests/golden/projection_*.npz, datasets/lidar_utils.py:54-347) and
the oracle.  Float64 geometry without contraction: bins, depths, intensities, indices and the
obfuscation mask are graded bit-exact on EVERY pixel.  The device atan2 may differ from the host
libm by a few ulp, which can move a point to another bin only within ~1e-12 bins of a bin edge;
kernel_ref.bin_edge_guard asserts from the reference's arithmetic alone that no point of these
golden clouds comes within 1e-9 bins of an edge that decides its pixel (the nearest is 1e-5 bins
away), and no two of their points have equal depth, so nothing is left to a tie or to rounding.
The four points of the edge-case test lie on the axes on purpose: their azimuths are the values
atan2 is defined to return there (0, pi/2), not computed ones."""
import numpy as np
import pytest
import torch

import kernel_ref as KR
from oracle import golden_inputs as GI
from oracle import projection_ref as PR
from sdp.projection import point_cloud_to_range_image, project_device

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("tag", sorted(GI.PROJECTION_CASES))
def test_projection_matches_reference_golden(tag):
    n, origin = GI.PROJECTION_CASES[tag]
    f = np.load(f"{GI.GOLDEN_DIR}/projection_{tag}.npz")
    cloud = GI.projection_cloud(tag, n)
    assert KR.bin_edge_guard(cloud, origin, 64, 1024) > KR.BIN_EDGE_EPS
    d, inten, obf, save_num, sky, idx = point_cloud_to_range_image(cloud, np.array(origin), True)
    assert save_num == 0 and d.dtype == np.float64 and d.shape == (64, 1024)
    assert np.array_equal(idx.astype(np.int32), f["index"]), int(np.sum(idx.astype(np.int32) != f["index"]))
    assert np.array_equal(d, f["depth"]), int(np.sum(d != f["depth"]))
    assert np.array_equal(inten.astype(np.float32), f["intensity"])
    assert np.array_equal(obf, f["obf"]), int(np.sum(obf != f["obf"]))
    assert not sky.any()


def test_projection_edge_cases():
    """Empty cloud, points on row/col 0 (excluded), a point at the origin (depth 0 -> empty),
    exact duplicates (lowest index wins), no remission."""
    pts = np.array([[0.0, 0.0, 0.0, 0.9],          # at the origin: nearest depth 0 -> stays empty
                    [0.0, 10.0, 0.0, 0.5],
                    [0.0, 10.0, 0.0, 0.7],         # duplicate of point 1: index 1 wins
                    [5.0, 0.0, -30.0, 0.1]], np.float64)   # far below the vertical scope -> row 0 -> excluded
    d, obf, _, sky, idx = point_cloud_to_range_image(pts, np.zeros(3), False)
    rd, robf, _, rsky, ridx = PR.point_cloud_to_range_image(pts, np.zeros(3), False)
    assert np.array_equal(d, rd) and np.array_equal(idx, ridx) and np.array_equal(obf, robf)
    assert (idx == 1).sum() == 1 and (idx == 2).sum() == 0 and (idx == 3).sum() == 0
    e = project_device(torch.zeros(0, 4, dtype=torch.float64, device="cuda"), np.zeros(3))
    assert (e["depth"] == 2057.701).all() and (e["index"] == -1).all()
