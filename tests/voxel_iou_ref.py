"""TEST INFRASTRUCTURE ONLY: numpy restatement of the device voxel IoU (csrc/voxel_iou.hip, contract in
include/sdp.h at sdp_voxel_iou).

Cells by the contract's three float64 operations per axis, floor((p - origin) / voxel) -- numpy's float64
subtract and divide round once each, like the device's -- with the bounds test on the floored double; np.unique
over the composite keys cell * 64 + label; majority labels by sorted runs (the first longest run of a voxel's
ascending (label, count) rows is the smallest label among equal counts); the confusion matrix by np.add.at.
tests/test_voxel_iou_ref_cpu.py pins this file to hand-written cases and to an independent dense formulation.
"""
import numpy as np

LABEL_BITS = 6


def cell_keys(points, origin, voxel, dims):
    """(inside bool [n], key int64 [n], garbage where not inside): finite, 0 <= floor(...) < n per axis."""
    p = np.asarray(points, np.float64)[:, :3]
    org = np.asarray(origin, np.float64).reshape(3)
    d = [int(v) for v in dims]
    with np.errstate(over="ignore", invalid="ignore"):
        f = np.floor((p - org) / np.float64(voxel))
        inside = np.isfinite(p).all(1) & (f >= 0).all(1) & (f < np.array(d, np.float64)).all(1)
    i = np.where(inside[:, None], f, 0.0).astype(np.int64)
    return inside, i[:, 0] + d[0] * i[:, 1] + d[0] * d[1] * i[:, 2]


def occupied(points, labels, origin, voxel, dims, num_classes, valid=None):
    """One cloud on the grid: dict(cells int64 [m] ascending, labels int32 [m], counts int32 [m], used, bad,
    tied bool [m])."""
    n = len(points)
    lab = np.zeros(n, np.int64) if labels is None else np.asarray(labels).astype(np.int64)
    bad = (lab < 0) | (lab >= num_classes)
    inside, key = cell_keys(points, origin, voxel, dims)
    use = inside & ~bad
    if valid is not None:
        v = np.asarray(valid).reshape(-1)
        use &= v[np.where(use, key, 0)] != 0
    comp = (key[use] << LABEL_BITS) | lab[use]
    rows, votes = np.unique(comp, return_counts=True)            # ascending (cell, label) with their votes
    cell_of = rows >> LABEL_BITS
    cells, first, nrows = np.unique(cell_of, return_index=True, return_counts=True)
    m = len(cells)
    best = np.zeros(m, np.int64)
    tied = np.zeros(m, bool)
    counts = np.zeros(m, np.int64)
    if m:
        top = np.maximum.reduceat(votes, first)
        counts = np.add.reduceat(votes, first)
        seg = np.repeat(np.arange(m), nrows)
        is_top = votes == top[seg]
        tied = np.add.reduceat(is_top.astype(np.int64), first) > 1
        # the first row of each segment that reaches the top: rows are ascending in the label
        pos = np.where(is_top, np.arange(len(rows)), len(rows))
        best = rows[np.minimum.reduceat(pos, first)] & ((1 << LABEL_BITS) - 1)
    return dict(cells=cells.astype(np.int64), labels=best.astype(np.int32), counts=counts.astype(np.int32),
                used=int(use.sum()), bad=int(bad.sum()), tied=tied)


def confusion(a, a_labels, b, b_labels, origin, voxel, dims, num_classes, valid=None):
    """dict(confusion int64 [C+1, C+1], info int64 [8], a=occupied(a), b=occupied(b))."""
    C = int(num_classes)
    A = occupied(a, a_labels, origin, voxel, dims, C, valid)
    B = occupied(b, b_labels, origin, voxel, dims, C, valid)
    conf = np.zeros((C + 1, C + 1), np.int64)
    in_b = np.isin(A["cells"], B["cells"], assume_unique=True)
    in_a = np.isin(B["cells"], A["cells"], assume_unique=True)
    np.add.at(conf, (1 + A["labels"][in_b].astype(np.int64), 1 + B["labels"][in_a].astype(np.int64)), 1)
    np.add.at(conf, (1 + A["labels"][~in_b].astype(np.int64), 0), 1)
    np.add.at(conf, (0, 1 + B["labels"][~in_a].astype(np.int64)), 1)
    inter = int(in_b.sum())
    ncells = int(dims[0]) * int(dims[1]) * int(dims[2])
    nvalid = ncells if valid is None else int(np.count_nonzero(np.asarray(valid)))
    conf[0, 0] = nvalid - (len(A["cells"]) + len(B["cells"]) - inter)
    info = np.array([len(A["cells"]), len(B["cells"]), A["used"], B["used"], A["bad"], B["bad"], inter, nvalid], np.int64)
    return dict(confusion=conf, info=info, a=A, b=B)


def cell_centres(dims, origin, voxel):
    """Centres origin + (i + 0.5) * voxel of every cell, float64 [nz*ny*nx, 3] in key order (volume_to_cloud's formula)."""
    nx, ny, nz = (int(v) for v in dims)
    iz, iy, ix = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    idx = np.stack([ix.ravel(), iy.ravel(), iz.ravel()], 1).astype(np.float64)
    return np.asarray(origin, np.float64).reshape(3) + (idx + 0.5) * np.float64(voxel)
