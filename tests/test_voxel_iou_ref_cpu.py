"""Pins tests/voxel_iou_ref.py (the numpy restatement the GPU tests of sdp_voxel_iou compare against) on the CPU:
hand-written cases of a few points; an independent DENSE formulation on small grids (a [cells][C] vote table by
np.add.at, argmax -- whose first maximum is the smallest label --, a dense state volume per cloud, a 2-D
bincount); the matrix sums to the valid-cell count; volume_to_cloud round-trips a random SSC-grid label volume
(every centre of the 256 x 256 x 32 grid of 0.2 m falls back into its own cell under the contract's three float64
operations); iou_from_confusion on matrices with known answers.
"""
import numpy as np
import pytest
import torch

import voxel_iou_ref as IR
from sdp import pointcloud as PC

ORG = (0.0, 0.0, 0.0)


def dense_confusion(a, la, b, lb, origin, voxel, dims, C, valid=None):
    """The independent formulation: loops over axes in plain numpy, a dense vote table and state volume."""
    nx, ny, nz = dims
    ncells = nx * ny * nz
    vmask = np.ones(ncells, bool) if valid is None else (np.asarray(valid).reshape(-1) != 0)
    states = []
    for p, l in ((a, la), (b, lb)):
        p = np.asarray(p, np.float64).reshape(len(p), -1)
        l = np.zeros(len(p), np.int64) if l is None else np.asarray(l, np.int64)
        votes = np.zeros((ncells, C), np.int64)
        for row in range(len(p)):
            x = p[row, :3]
            if not np.isfinite(x).all() or not 0 <= l[row] < C:
                continue
            with np.errstate(over="ignore"):
                f = [np.floor((x[k] - np.float64(origin[k])) / np.float64(voxel)) for k in range(3)]
            if not all(0 <= f[k] < dims[k] for k in range(3)):
                continue
            cell = int(f[0]) + nx * int(f[1]) + nx * ny * int(f[2])
            if vmask[cell]:
                np.add.at(votes, (cell, l[row]), 1)
        states.append(np.where(votes.sum(1) > 0, 1 + votes.argmax(1), 0))
    sa, sb = states[0][vmask], states[1][vmask]
    return np.bincount(sa * (C + 1) + sb, minlength=(C + 1) ** 2).reshape(C + 1, C + 1)


def test_hand_written_occupancy():
    a = np.array([[0.1, 0.1, 0.1], [0.9, 0.1, 0.1], [1.1, 0.1, 0.1], [5.0, 0.0, 0.0], [-0.1, 0.0, 0.0]])
    b = np.array([[0.5, 0.5, 0.5], [0.5, 1.5, 0.5], [np.nan, 0.0, 0.0], [1e300, 0.0, 0.0], [0.0, 0.0, np.inf]])
    r = IR.confusion(a, None, b, None, ORG, 1.0, (2, 2, 1), 1)
    # A occupies cells 0 (two points) and 1; B cells 0 and 2; cell 3 is empty in both
    np.testing.assert_array_equal(r["a"]["cells"], [0, 1])
    np.testing.assert_array_equal(r["a"]["counts"], [2, 1])
    np.testing.assert_array_equal(r["b"]["cells"], [0, 2])
    np.testing.assert_array_equal(r["confusion"], [[1, 1], [1, 1]])
    np.testing.assert_array_equal(r["info"], [2, 2, 3, 2, 0, 0, 1, 4])


def test_hand_written_labels_ties_and_bad_labels():
    # cell 0 of A: labels 2, 2, 1, 1, 3 -> tie between 1 and 2 -> 1; cell 1 of A: label 0; labels -1 and 3 (= C) are bad
    a = np.array([[0.1, 0.1, 0.1]] * 5 + [[1.5, 0.5, 0.5]] + [[0.5, 1.5, 0.5]] * 2)
    la = np.array([2, 2, 1, 1, 0, 0, -1, 3])
    b = np.array([[0.2, 0.2, 0.2], [0.5, 1.5, 0.5]])
    lb = np.array([2, 1])
    r = IR.confusion(a, la, b, lb, ORG, 1.0, (2, 2, 1), 3)
    np.testing.assert_array_equal(r["a"]["cells"], [0, 1])
    np.testing.assert_array_equal(r["a"]["labels"], [1, 0])
    np.testing.assert_array_equal(r["a"]["tied"], [True, False])
    want = np.zeros((4, 4), np.int64)
    want[2, 3] = 1      # cell 0: truth 1, prediction 2
    want[1, 0] = 1      # cell 1: truth 0, prediction empty
    want[0, 2] = 1      # cell 2: truth empty (both points bad), prediction 1
    want[0, 0] = 1      # cell 3
    np.testing.assert_array_equal(r["confusion"], want)
    np.testing.assert_array_equal(r["info"], [2, 2, 6, 2, 2, 0, 1, 4])


def test_hand_written_valid_mask():
    a = np.array([[0.5, 0.5, 0.5], [1.5, 0.5, 0.5]])
    b = np.array([[0.5, 0.5, 0.5], [0.5, 1.5, 0.5]])
    valid = np.array([[[1, 0], [0, 1]]], np.uint8)          # [nz][ny][nx]: cells 0 and 3
    r = IR.confusion(a, None, b, None, ORG, 1.0, (2, 2, 1), 1, valid)
    np.testing.assert_array_equal(r["confusion"], [[1, 0], [0, 1]])
    np.testing.assert_array_equal(r["info"], [1, 1, 1, 1, 0, 0, 1, 2])


@pytest.mark.parametrize("C,dims,voxel,masked", [(1, (5, 4, 3), 0.5, False), (4, (7, 3, 2), 0.2, True),
                                                 (20, (3, 3, 3), 0.25, True), (64, (2, 5, 1), 0.3, False)])
def test_against_the_dense_formulation(C, dims, voxel, masked):
    r = np.random.default_rng(C * 100 + dims[0])
    ext = np.array(dims) * voxel
    org = np.array([-1.0, 0.3, 2.0])
    clouds = []
    for n in (400, 300):
        p = org + r.uniform(-0.1, 1.1, (n, 3)) * ext
        p[::50] = org + r.integers(0, np.array(dims) + 1, (len(p[::50]), 3)) * voxel     # on cell faces
        p[7] = [np.nan, 0, 0]
        p[8] = [1e300, 0, 0]
        l = r.integers(-1, C + 1, n)
        clouds += [p, l]
    valid = (r.random((dims[2], dims[1], dims[0])) > 0.3).astype(np.uint8) if masked else None
    got = IR.confusion(clouds[0], clouds[1], clouds[2], clouds[3], org, voxel, dims, C, valid)
    want = dense_confusion(clouds[0], clouds[1], clouds[2], clouds[3], org, voxel, dims, C, valid)
    np.testing.assert_array_equal(got["confusion"], want)
    nvalid = int(np.prod(dims)) if valid is None else int(valid.sum())
    assert got["confusion"].sum() == nvalid == got["info"][7]
    assert got["info"][6] == want[1:, 1:].sum()
    if C > 1:
        assert got["a"]["tied"].any()       # the tie rule was exercised


def test_volume_to_cloud_round_trips_the_ssc_grid():
    g = PC.SSC_GRID
    assert g["origin"] == (0.0, -25.6, -2.0) and g["voxel"] == 0.2 and g["dims"] == (256, 256, 32)
    nx, ny, nz = g["dims"]
    # every centre of the grid falls into its own cell under the contract's arithmetic
    inside, key = IR.cell_keys(IR.cell_centres(g["dims"], g["origin"], g["voxel"]), g["origin"], g["voxel"], g["dims"])
    assert inside.all()
    np.testing.assert_array_equal(key, np.arange(nx * ny * nz))
    r = np.random.default_rng(5)
    vol = (r.integers(0, 20, (nz, ny, nx)) * (r.random((nz, ny, nx)) < 0.1)).astype(np.int64)
    pts, lab = PC.volume_to_cloud(torch.from_numpy(vol), g["origin"], g["voxel"], empty=0)
    assert pts.dtype == torch.float64 and lab.dtype == torch.int32 and pts.shape == (int((vol != 0).sum()), 3)
    occ = IR.occupied(pts.numpy(), lab.numpy(), g["origin"], g["voxel"], g["dims"], 20)
    back = np.zeros(nx * ny * nz, np.int64)
    back[occ["cells"]] = occ["labels"]
    np.testing.assert_array_equal(back.reshape(nz, ny, nx), vol)
    assert (occ["counts"] == 1).all() and occ["used"] == len(pts)
    # a volume graded against itself: nothing off the diagonal
    conf = IR.confusion(pts.numpy(), lab.numpy(), pts.numpy(), lab.numpy(), g["origin"], g["voxel"], g["dims"], 20)
    assert conf["confusion"].sum() == nx * ny * nz
    assert (conf["confusion"] - np.diag(np.diagonal(conf["confusion"]))).sum() == 0


def test_iou_identical_and_disjoint():
    same = PC.iou_from_confusion(np.array([[90, 0], [0, 10]]))
    assert same["iou"] == 1.0 and same["precision"] == 1.0 and same["recall"] == 1.0 and same["miou"] == 1.0
    apart = PC.iou_from_confusion(torch.tensor([[80, 10], [10, 0]]))
    assert apart["iou"] == 0.0 and apart["precision"] == 0.0 and apart["recall"] == 0.0 and apart["class_iou"][0] == 0.0
    assert (apart["tp"], apart["fp"], apart["fn"]) == (0, 10, 10)
    empty = PC.iou_from_confusion(np.array([[100, 0], [0, 0]]))
    assert np.isnan(empty["iou"]) and np.isnan(empty["miou"]) and np.isnan(empty["class_iou"][0])


def test_iou_classes_absent_and_ignored():
    #            pred: empty  c0  c1  c2
    conf = np.array([[50, 2, 0, 1],      # truth empty
                     [3, 6, 0, 1],       # truth c0
                     [0, 0, 0, 0],       # truth c1: absent from both
                     [1, 2, 0, 4]])      # truth c2
    r = PC.iou_from_confusion(conf)
    assert r["tp"] == 13 and r["fp"] == 3 and r["fn"] == 4
    assert r["iou"] == 13 / 20 and r["precision"] == 13 / 16 and r["recall"] == 13 / 17
    np.testing.assert_array_equal(r["class_iou"], [6 / (10 + 10 - 6), np.nan, 4 / (7 + 6 - 4)])
    assert r["miou"] == np.mean([6 / 14, 4 / 9])
    assert PC.iou_from_confusion(conf, ignore=(0,))["miou"] == 4 / 9
    assert np.isnan(PC.iou_from_confusion(conf, ignore=(0, 2))["miou"])
    with pytest.raises(ValueError):
        PC.iou_from_confusion(conf, ignore=(3,))
    with pytest.raises(ValueError):
        PC.iou_from_confusion(np.zeros((2, 3)))
