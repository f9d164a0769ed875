"""Float64 numpy restatement of the range image -> point cloud step (test infrastructure only):
MeasureResults/SceneCompleter.py:43-70 (azimuth / elevation tables), :105-121 (un-log, placement)
and :259-264 (mask and concatenation over views).  Checker for ``sdp_range_unproject``
(csrc/unproject.hip); pinned in tests/test_pointcloud_cpu.py through the projection oracle, itself
pinned to the reference's own outputs.

Distance: ``oracle.sampling_ref.real_distance`` with smod = 1 (float32, 2^v correctly rounded),
the merge's convention, not SceneCompleter's float32 ``np.power`` (not correctly rounded).

The keyword-only ``mutant`` argument builds deliberately wrong variants; the CPU tests assert that
each of them fails the round trip, so the round trip is known to see those mistakes.
"""
from __future__ import annotations

import numpy as np

from oracle.projection_ref import geometry as dataset_geometry
from oracle.sampling_ref import merge_geometry, real_distance

F32 = np.float32
MUTANTS = ("no_flip", "arange_cols", "view_minor")


def angles(H, W, geometry="dataset", mutant=None):
    """(azimuth [W], elevation [H]) of the image's columns and rows."""
    if geometry == "dataset":
        hA, vA, hMin, vMin = dataset_geometry(H, W)
    elif geometry == "sampler":
        g = merge_geometry(H, W)
        hA, vA, hMin = g["hA"], g["vA"], g["hMin"]
        vMin = g["el"][-1]                       # el = arange(H-1,-1,-1)*vA + vMin: its last entry is vMin
    else:
        raise ValueError(geometry)
    cols = np.arange(W - 1, -1, -1)
    rows = np.arange(H - 1, -1, -1)
    if mutant == "arange_cols":
        cols = np.arange(W)
    if mutant == "no_flip":
        cols, rows = np.arange(W), np.arange(H)
    return cols * hA + hMin, rows * vA + vMin


def distance(code):
    """rd = f32(2^f32(|code|*6)) - 1, float32 (negative codes count by their magnitude)."""
    return real_distance(np.abs(np.asarray(code, dtype=F32)), 1)


def unproject(x, origins=None, poses=None, keep=None, exist=None, min_range=1.5, geometry="dataset", mutant=None):
    """x [B,C,H,W] float32 -> (points [n,4] f64, offsets [B+1] i64, pixel [n] i32, rd [B,H,W] f32)."""
    x = np.asarray(x, dtype=F32)
    B, C, H, W = x.shape
    assert origins is None or poses is None
    az, el = angles(H, W, geometry, mutant)
    az, el = az.reshape(1, W), el.reshape(H, 1)
    clouds, pix, offsets = [], [], [0]
    rd_all = np.empty((B, H, W), F32)
    for b in range(B):
        rd = distance(x[b, 0])
        rd_all[b] = rd
        rdd = rd.astype(np.float64)
        px = rdd * np.cos(az) * np.cos(el)
        py = rdd * np.sin(az) * np.cos(el)
        pz = rdd * np.sin(el) + np.zeros((1, W))
        if origins is not None:
            px, py, pz = px + origins[b][0], py + origins[b][1], pz + origins[b][2]
        elif poses is not None:
            T = np.asarray(poses[b], dtype=np.float64)
            px, py, pz = (((T[r, 0] * px + T[r, 1] * py) + T[r, 2] * pz) + T[r, 3] * 1.0 for r in range(3))
        inten = x[b, 1].astype(np.float64) if C == 2 else np.zeros((H, W))
        with np.errstate(invalid="ignore"):
            mask = rd > F32(min_range)
        if keep is not None:
            mask = mask & (np.asarray(keep[b]) != 0)
        if exist is not None:
            mask = mask & (np.asarray(exist) != 0)
        clouds.append(np.stack((px[mask], py[mask], pz[mask], inten[mask]), 1))
        pix.append((b * H * W + np.nonzero(mask.reshape(-1))[0]).astype(np.int32))
        offsets.append(offsets[-1] + int(mask.sum()))
    points, pixel = np.concatenate(clouds, 0), np.concatenate(pix, 0)
    if mutant == "view_minor":      # pixel-major, view-minor: rows of all views interleaved by pixel
        order = np.lexsort((pixel // (H * W), pixel % (H * W)))
        points, pixel = points[order], pixel[order]
    return points, np.asarray(offsets, dtype=np.int64), pixel, rd_all
