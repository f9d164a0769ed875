"""TEST INFRASTRUCTURE ONLY: vectorised numpy restatement of the device voxel grid (csrc/voxel_grid.hip).

Method "barycenters" of the reference's grid_subsampling.cpp:46-102 with the device's conventions:
rows in ascending voxel key, points with a non-finite coordinate skipped, majority labels with equal
votes resolved to the smallest label.  Keys come from oracle.grid_subsampling_ref.voxel_keys on the
finite points; the per-voxel float32 sums run sequentially in point order (a loop over the position
inside the segment, vectorised over the voxels -- np.add.reduceat sums pairwise and is not used); the
barycentre is sum * float32(1.0 / count) and the features are sum / float32(count), the host's two
forms.  tests/test_voxel_ref_cpu.py pins this file to the host C++ and to the oracle.
"""
import numpy as np

from oracle import grid_subsampling_ref as G

F32 = np.float32
LIMIT = 1 << 40


def grid_dims(q, dl):
    """(nx, ny, nz) as Python ints: grid_subsampling.cpp:24-44 in float32 (nz by the same formula)."""
    dl = F32(dl)
    lo, hi = q.min(0), q.max(0)
    org = np.floor(lo * (F32(1) / dl)).astype(np.float32) * dl
    with np.errstate(over="ignore", invalid="ignore"):
        f = np.floor((hi - org) / dl).astype(np.float32)
    return tuple(int(v) + 1 for v in f.astype(np.float64))


def subsample(points, features=None, classes=None, dl=0.1):
    """points [n,>=3] (xyz first), features [n,d] or None, classes [n] / [n,l] or None.  Returns a dict:
    info int64 [5] = (m, nx, ny, nz, used) with m = -1 for a grid of more than 2^40 cells (nothing
    else is then set but key_bits), key_bits, points f32 [m,3], features f32 [m,d], classes i32 [m,l],
    tied bool [m,l] (more than one label has the most votes), max_codes (per label column the sorted
    uint64 codes (row << 32) | (label ^ 2^31) of every label with the most votes of its voxel),
    keys i64 [m], counts i32 [m], order i32 [used] (stable argsort), inverse i32 [n] (-1 = skipped)."""
    p = np.ascontiguousarray(np.asarray(points, np.float32)[:, :3])
    n = len(p)
    used = np.flatnonzero(np.isfinite(p).all(1))
    out = dict(key_bits=0)
    if len(used) == 0:
        out.update(info=np.array([0, 0, 0, 0, 0], np.int64), inverse=np.full(n, -1, np.int32))
        return out
    q = p[used]
    nx, ny, nz = grid_dims(q, dl)
    cells = nx * ny * nz
    out["key_bits"] = 0 if cells <= 1 else (cells - 1).bit_length()
    if cells > LIMIT:
        out["info"] = np.array([-1, nx, ny, nz, len(used)], np.int64)
        return out
    keys = G.voxel_keys(q, dl)
    o = np.argsort(keys, kind="stable")
    ks = keys[o]
    order = used[o]
    head = np.r_[True, ks[1:] != ks[:-1]]
    first = np.flatnonzero(head)
    m = len(first)
    counts = np.diff(np.r_[first, len(ks)])
    row = np.cumsum(head) - 1
    inverse = np.full(n, -1, np.int32)
    inverse[order] = row
    cols = [p]
    if features is not None:
        cols.append(np.asarray(features, np.float32).reshape(n, -1))
    data = np.ascontiguousarray(np.concatenate(cols, 1)[order])
    # sequential float32 sums: step j adds the j-th point of every voxel that has one (voxels by falling count)
    by = np.argsort(-counts, kind="stable")
    cs, fs = counts[by], first[by]
    acc = np.zeros((m, data.shape[1]), np.float32)
    for j in range(int(cs[0])):
        k = int(np.searchsorted(-cs, -j, side="left"))      # voxels with more than j points
        acc[:k] = acc[:k] + data[fs[:k] + j]
    sums = np.empty_like(acc)
    sums[by] = acc
    scale = (1.0 / counts.astype(np.float64)).astype(np.float32)
    out.update(info=np.array([m, nx, ny, nz, len(used)], np.int64), keys=ks[first].astype(np.int64),
               counts=counts.astype(np.int32), order=order.astype(np.int32), inverse=inverse,
               points=(sums[:, :3] * scale[:, None]).astype(np.float32))
    if features is not None:
        out["features"] = (sums[:, 3:] / counts.astype(np.float32)[:, None]).astype(np.float32)
    if classes is not None:
        c = np.asarray(classes, np.int32).reshape(n, -1)[order]
        lab = np.empty((m, c.shape[1]), np.int32)
        tied = np.empty((m, c.shape[1]), bool)
        max_codes = []
        for j in range(c.shape[1]):
            code = np.sort((row.astype(np.uint64) << np.uint64(32)) |
                           (c[:, j].view(np.uint32) ^ np.uint32(0x80000000)).astype(np.uint64))
            rh = np.flatnonzero(np.r_[True, code[1:] != code[:-1]])
            rlen = np.diff(np.r_[rh, len(code)])
            rcode = code[rh]
            rrow = (rcode >> np.uint64(32)).astype(np.int64)
            best = np.zeros(m, np.int64)
            np.maximum.at(best, rrow, rlen)
            top = rlen == best[rrow]
            tied[:, j] = np.bincount(rrow[top], minlength=m) > 1
            rows, at = np.unique(rrow[top], return_index=True)          # the first maximum of every voxel
            assert len(rows) == m
            lab[:, j] = ((rcode[top][at] & np.uint64(0xffffffff)).astype(np.uint32) ^ np.uint32(0x80000000)).view(np.int32)
            max_codes.append(rcode[top])
        out.update(classes=lab, tied=tied, max_codes=max_codes)
    return out


def label_code(rows, labels):
    """The codes of max_codes for (voxel row, label) pairs."""
    return (np.asarray(rows).astype(np.uint64) << np.uint64(32)) | \
        (np.asarray(labels, np.int32).view(np.uint32) ^ np.uint32(0x80000000)).astype(np.uint64)
