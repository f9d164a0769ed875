"""Range images -> fused point clouds on the GPU: the way back out of the samplers.

``range_image_to_point_cloud`` turns the [B,C,H,W] log-depth codes that ``Runner.sample()`` /
``Runner.sample_completion()`` produce into one compacted float64 cloud, the offline step of
MeasureResults/SceneCompleter.py:43-70 (azimuth / elevation tables), :105-121 (un-log and
placement) and :259-264 (exist / min-range / sky mask, concatenation over views).  The work runs
in ``sdp_range_unproject`` (csrc/unproject.hip); tensors stay on the device.

Distance convention: rd = float32(2^float32(|code|*6)) - 1 with 2^v correctly rounded, the
merge's (KITTISampling.py:164-166, oracle ``real_distance`` with smod = 1).  SceneCompleter's own
``np.power(2, float32)`` is not correctly rounded and differs from it in the last float32 bit of
2^v for about a fifth of random codes.

Two vertical origins exist in the reference and they are NOT interchangeable:
  geometry="dataset"  vMin = radians(3 - 28)            lidar_utils.py / SceneCompleter.py -- the
                      images the datasets render and the runners save (``sdp_range_project``);
  geometry="sampler"  vMin = ((H*-25)//28)*vA + vA/2    KITTISampling.py:29-102 -- the grid the
                      consistency merge reprojects in, 0.36 bin (0.16 degrees) above the dataset's.

``voxel_grid_subsample`` puts such a cloud on a voxel grid without leaving the device
(``sdp_voxel_grid``, csrc/voxel_grid.hip): the barycentre, the mean features and the majority labels
of every occupied voxel, bit for bit what ``sdp.grid_subsampling.compute`` gives on the host, in
ascending voxel key.

``nearest_neighbours`` / ``cloud_metrics`` score one such cloud against another on the device
(``sdp_cloud_nn`` / ``sdp_cloud_nn_stats``, csrc/cloud_nn.hip): the exact nearest target within a radius
for every point, and from it Chamfer distance, accuracy / completeness and precision / recall / F-score.

``voxel_confusion`` / ``voxel_iou`` grade a cloud the way scene completion is graded (``sdp_voxel_iou``,
csrc/voxel_iou.hip): both clouds on one fixed grid (``SSC_GRID``: SemanticKITTI-SSC's 256 x 256 x 32 voxels of
0.2 m), the majority label of every occupied voxel, the confusion matrix of the voxel states, and from it
(``iou_from_confusion``) the completion IoU and the per-class IoU / mIoU.  ``volume_to_cloud`` turns a dense
ground-truth label volume into the labelled cloud these take.
"""
from __future__ import annotations

import warnings

import numpy as np
import torch

from . import _lib

GEOMETRY = {"dataset": 0, "sampler": 1}


def _workspace(entry, *args, device):
    """The uint8 workspace tensor whose size the ``sdp_<entry>_workspace_size`` entry reports for ``args``."""
    n = _lib.SZ()
    _lib.check(getattr(_lib.lib(), f"sdp_{entry}_workspace_size")(*args, _lib.C.byref(n)), f"{entry}_ws")
    return torch.empty(n.value, dtype=torch.uint8, device=device)


def _mask_u8(m, shape, what):
    if m is None:
        return None
    if not m.is_cuda or tuple(m.shape) != tuple(shape):
        raise ValueError(f"{what} must be a cuda tensor of shape {tuple(shape)}, got {tuple(m.shape)}")
    return (m != 0).to(torch.uint8).contiguous() if m.dtype != torch.uint8 else m.contiguous()


def range_image_to_point_cloud(x, origins=None, poses=None, keep=None, exist=None, min_range=1.5,
                               geometry="dataset", return_pixel=False):
    """x: cuda float32 [B,C,H,W], C in {1, 2} (code, intensity).  origins: cuda float64 [B,3] added to
    each view's points, OR poses: cuda float64 [B,4,4] applied as (pose @ [x y z 1])[:3]; neither =
    the sensor frame.  keep: per-view mask [B,H,W], exist: shared mask [H,W] (non-zero = keep);
    a pixel is kept iff rd > min_range (float32) and both masks allow it.

    Returns (points [n,4] float64 (x, y, z, intensity), offsets [B+1] int64) -- view b owns rows
    offsets[b]:offsets[b+1], pixels row-major inside a view -- and, with return_pixel, the int32
    flat pixel index b*H*W + i*W + j of every row (to gather per-pixel labels).  All on x's device;
    one host sync, to read the total row count for the slice."""
    if not x.is_cuda or x.dtype != torch.float32 or x.dim() != 4:
        raise ValueError("range_image_to_point_cloud expects a cuda float32 [B,C,H,W] tensor")
    if geometry not in GEOMETRY:
        raise ValueError(f"geometry must be one of {sorted(GEOMETRY)}, got {geometry!r}")
    x = x.contiguous()
    B, C, H, W = x.shape
    dev = x.device
    for t, shape, what in ((origins, (B, 3), "origins"), (poses, (B, 4, 4), "poses")):
        if t is not None and (not t.is_cuda or t.dtype != torch.float64 or tuple(t.shape) != shape):
            raise ValueError(f"{what} must be a cuda float64 tensor of shape {shape}")
    origins = None if origins is None else origins.contiguous()
    poses = None if poses is None else poses.contiguous()
    keep = _mask_u8(keep, (B, H, W), "keep")
    exist = _mask_u8(exist, (H, W), "exist")
    L = _lib.lib()
    ws = _workspace("range_unproject", B, H, W, device=dev)
    with torch.cuda.device(dev):
        points = torch.empty(B * H * W, 4, dtype=torch.float64, device=dev)
        pixel = torch.empty(B * H * W, dtype=torch.int32, device=dev) if return_pixel else None
        offsets = torch.empty(B + 1, dtype=torch.int64, device=dev)
        _lib.check(L.sdp_range_unproject(x.data_ptr(), B, C, H, W, GEOMETRY[geometry], _lib.ptr(origins),
                                         _lib.ptr(poses), _lib.ptr(keep), _lib.ptr(exist), float(min_range),
                                         points.data_ptr(), _lib.ptr(pixel), offsets.data_ptr(), ws.data_ptr(),
                                         ws.numel(), _lib.stream()), "range_unproject")
        total = int(offsets[B].item())
    if return_pixel:
        return points[:total], offsets, pixel[:total]
    return points[:total], offsets


def voxel_grid_subsample(points, features=None, classes=None, sampleDl=0.1, center=None,
                         return_keys=False, return_counts=False, return_inverse=False):
    """Voxel-grid subsampling on the device (method "barycenters" of grid_subsampling.compute).

    points: cuda [n,3] or [n,4] (xyz first), float32 or float64; features: cuda float [n,d] or None;
    classes: cuda integer [n] or [n,l] or None.  With float32 points the result is float32, bit-equal to
    ``sdp.grid_subsampling.compute`` on the same arrays.  With float64 points the grid runs on
    q = float32(p - center) and the barycentres come back as float64(barycentre) + center; center is
    float64 [3] and defaults to zeros.  A point with a non-finite coordinate is skipped.

    Returns the points [m,3] alone, or a tuple in the order points, features [m,d], classes [m,l], then
    the requested extras: keys int64 [m] (ascending: the row order), counts int32 [m], inverse int32 [n]
    (the row of every point, -1 for a skipped one).  One host sync, to read m.  Labels with equal votes
    resolve to the smallest label value.  Raises RuntimeError when the grid exceeds 2^40 cells."""
    if not torch.is_tensor(points) or not points.is_cuda or points.dim() != 2 or points.shape[1] not in (3, 4):
        raise ValueError("voxel_grid_subsample expects a cuda [n,3] or [n,4] tensor of points")
    if points.dtype not in (torch.float32, torch.float64):
        raise ValueError("points must be float32 or float64")
    dev = points.device
    n = points.shape[0]
    wide = points.dtype == torch.float64
    if center is not None and not wide:
        raise ValueError("center applies to float64 points only")
    if wide:
        c64 = torch.zeros(3, dtype=torch.float64, device=dev) if center is None else \
            torch.as_tensor(center, dtype=torch.float64).to(dev).reshape(3)
        pts = (points[:, :3] - c64).to(torch.float32).contiguous()
    else:
        pts = points.contiguous()
    f = c = None
    fdim = ldim = 0
    if features is not None:
        if not features.is_cuda or features.dim() != 2 or features.shape[0] != n or features.shape[1] < 1:
            raise ValueError("features must be a cuda [n,d] tensor")
        f = features.to(torch.float32).contiguous()
        fdim = f.shape[1]
    if classes is not None:
        if not classes.is_cuda or classes.dim() not in (1, 2) or classes.shape[0] != n:
            raise ValueError("classes must be a cuda [n] or [n,l] tensor")
        c = classes.reshape(n, -1).to(torch.int32).contiguous()
        ldim = c.shape[1]
    L = _lib.lib()
    ws = _workspace("voxel_grid", n, device=dev)
    with torch.cuda.device(dev):
        op = torch.empty(n, 3, dtype=torch.float32, device=dev)
        of = torch.empty(n, fdim, dtype=torch.float32, device=dev) if f is not None else None
        oc = torch.empty(n, ldim, dtype=torch.int32, device=dev) if c is not None else None
        keys = torch.empty(n, dtype=torch.int64, device=dev) if return_keys else None
        counts = torch.empty(n, dtype=torch.int32, device=dev) if return_counts else None
        inverse = torch.empty(n, dtype=torch.int32, device=dev) if return_inverse else None
        info = torch.empty(5, dtype=torch.int64, device=dev)
        _lib.check(L.sdp_voxel_grid(pts.data_ptr(), n, pts.shape[1], _lib.ptr(f), fdim, _lib.ptr(c), ldim,
                                    float(np.float32(sampleDl)), op.data_ptr(), _lib.ptr(of), _lib.ptr(oc),
                                    _lib.ptr(keys), _lib.ptr(counts), None, _lib.ptr(inverse), info.data_ptr(),
                                    ws.data_ptr(), ws.numel(), _lib.stream()), "voxel_grid")
        m, nx, ny, nz, _ = (int(v) for v in info.tolist())
    if m < 0:
        raise RuntimeError(f"voxel_grid_subsample: a grid of {nx} x {ny} x {nz} cells at sampleDl = {sampleDl} "
                           "exceeds 2^40 cells")
    out = [op[:m].to(torch.float64) + c64 if wide else op[:m]]
    if of is not None:
        out.append(of[:m])
    if oc is not None:
        out.append(oc[:m])
    if return_keys:
        out.append(keys[:m])
    if return_counts:
        out.append(counts[:m])
    if return_inverse:
        out.append(inverse)
    return out[0] if len(out) == 1 else tuple(out)


def _xyz64(t, what):
    if not torch.is_tensor(t) or not t.is_cuda or t.dim() != 2 or t.shape[1] not in (3, 4):
        raise ValueError(f"{what} must be a cuda [n,3] or [n,4] tensor of points")
    if t.dtype not in (torch.float32, torch.float64):
        raise ValueError(f"{what} must be float32 or float64")
    return t.to(torch.float64).contiguous()


def _nn_launch(q, t, max_dist, cell, center):
    """sdp_cloud_nn on prepared float64 tensors; no host sync.  Returns (d2, index, info [9]): the entry's
    info [8] and, last, whether the centre is finite (a non-finite one would empty the grid silently)."""
    dev = q.device
    if center is None:
        # the midpoint of the target's finite bounds (zeros when it has no finite point), on the device
        xyz = t[:, :3]
        fin = torch.isfinite(xyz).all(1, keepdim=True)
        inf = torch.full((1, 3), float("inf"), dtype=torch.float64, device=dev)
        lo = torch.cat((torch.where(fin, xyz, inf), inf)).amin(0)
        hi = torch.cat((torch.where(fin, xyz, -inf), -inf)).amax(0)
        c64 = torch.nan_to_num(lo * 0.5 + hi * 0.5, nan=0.0, posinf=0.0, neginf=0.0)
    else:
        c64 = torch.as_tensor(center, dtype=torch.float64).to(dev).reshape(3).contiguous()
    L = _lib.lib()
    nq, nt = q.shape[0], t.shape[0]
    ws = _workspace("cloud_nn", nq, nt, device=dev)
    with torch.cuda.device(dev):
        d2 = torch.empty(nq, dtype=torch.float64, device=dev)
        idx = torch.empty(nq, dtype=torch.int32, device=dev)
        info = torch.empty(8, dtype=torch.int64, device=dev)
        _lib.check(L.sdp_cloud_nn(_lib.ptr(q) if nq else None, nq, q.shape[1], _lib.ptr(t) if nt else None, nt,
                                  t.shape[1], float(max_dist), float(cell), c64.data_ptr(), _lib.ptr(d2) if nq else None,
                                  _lib.ptr(idx) if nq else None, info.data_ptr(), ws.data_ptr(), ws.numel(),
                                  _lib.stream()), "cloud_nn")
    return d2, idx, torch.cat((info, torch.isfinite(c64).all().to(torch.int64).reshape(1)))


def _nn_check(info, max_dist, cell, what):
    """Raise / warn from the host copy of ``_nn_launch``'s info."""
    st, nx, ny, nz = (int(v) for v in info[:4])
    if not int(info[8]):
        raise ValueError(f"{what}: center must be finite")
    if int(info[6]):
        warnings.warn(f"{what}: the float32 grid origin rounded above the targets' lower bound at cell = {cell}; "
                      "every query scanned all targets (exact, but slow): change cell or center slightly",
                      RuntimeWarning, stacklevel=3)
    if st == -1:
        raise RuntimeError(f"{what}: a grid of {nx} x {ny} x {nz} cells at cell = {cell} exceeds 2^40 cells")
    if st == -2:
        raise RuntimeError(f"{what}: cell = {cell} too small for max_dist = {max_dist} on a float32 grid of "
                           f"{nx} x {ny} x {nz} cells ({int(info[5])} rings needed, 9 allowed): use a larger "
                           "cell or a center near the cloud")


def _nn_args(max_dist, cell, what):
    if not max_dist > 0 or not np.isfinite(max_dist):
        raise ValueError(f"{what}: max_dist must be > 0 and finite")
    cell = max_dist if cell is None else cell
    if not 0 < cell <= max_dist:
        raise ValueError(f"{what}: cell must be in (0, max_dist]")
    return float(max_dist), float(cell)


def nearest_neighbours(query, target, max_dist, cell=None, center=None):
    """For every point of ``query`` the exact nearest point of ``target`` within ``max_dist``, on the device.

    query, target: cuda [n,3] or [n,4] (xyz first), float64 (float32 is widened).  Returns (d2 float64 [nq],
    index int32 [nq]): d2 = ((dx*dx + dy*dy) + dz*dz) in float64 from the given coordinates, the target of
    smallest d2 <= max_dist*max_dist, among equals the smallest index; +inf and -1 for a query without one or
    with a non-finite coordinate.  A target with a non-finite coordinate is never a neighbour.  ``cell``
    (default max_dist, at least max_dist / 8) and ``center`` (float64 [3], default the midpoint of the target's
    finite bounds) only steer the float32 acceleration grid; the result does not depend on them.  One host
    sync, to read the grid's status.  Raises RuntimeError when the grid exceeds 2^40 cells or the cell is too
    small for max_dist."""
    what = "nearest_neighbours"
    q, t = _xyz64(query, "query"), _xyz64(target, "target")
    if q.device != t.device:
        raise ValueError("query and target must be on the same device")
    max_dist, cell = _nn_args(max_dist, cell, what)
    d2, idx, info = _nn_launch(q, t, max_dist, cell, center)
    _nn_check(info.tolist(), max_dist, cell, what)
    return d2, idx


def _nn_stats_launch(d2, q, thresholds, max_dist):
    L = _lib.lib()
    n, T = q.shape[0], len(thresholds)
    ws = _workspace("cloud_nn_stats", n, device=q.device)
    with torch.cuda.device(q.device):
        out = torch.empty(5 + T, dtype=torch.float64, device=q.device)
        thr = (_lib.D * max(T, 1))(*thresholds)
        _lib.check(L.sdp_cloud_nn_stats(_lib.ptr(d2) if n else None, _lib.ptr(q) if n else None, q.shape[1], n, thr, T,
                                        float(max_dist), out.data_ptr(), ws.data_ptr(), ws.numel(), _lib.stream()),
                   "cloud_nn_stats")
    return out


def nearest_neighbour_stats(d2, query, thresholds, max_dist):
    """The sums of one direction (``sdp_cloud_nn_stats``): cuda float64 [5 + T] = n_finite, n_matched,
    sum of distances, sum of squared distances, largest distance, then per threshold tau the number of points
    with d2 <= tau*tau.  ``d2`` from ``nearest_neighbours(query, ...)``; thresholds above max_dist raise."""
    q = _xyz64(query, "query")
    if not d2.is_cuda or d2.dtype != torch.float64 or tuple(d2.shape) != (q.shape[0],):
        raise ValueError("d2 must be the cuda float64 [n] result of nearest_neighbours on this query")
    return _nn_stats_launch(d2.contiguous(), q, [float(v) for v in thresholds], max_dist)


def cloud_distance_stats(a, b, max_dist, thresholds=(0.1, 0.2, 0.5), cell=None):
    """Both directions between clouds ``a`` and ``b`` on the device: (d2 float64 [n_a], the squared distance of
    every point of ``a`` to its nearest point of ``b`` within max_dist, +inf without one; rows float64
    [2, 5 + T], the sums of ``nearest_neighbour_stats`` for a -> b and b -> a).  One host sync, to read the
    grids' status: raises like ``nearest_neighbours``."""
    what = "cloud_distance_stats"
    a64, b64 = _xyz64(a, "a"), _xyz64(b, "b")
    if a64.device != b64.device:
        raise ValueError("a and b must be on the same device")
    max_dist, cell = _nn_args(max_dist, cell, what)
    thr = [float(v) for v in thresholds]
    if len(thr) > 8 or any(not 0 <= v <= max_dist for v in thr):
        raise ValueError(f"{what}: at most 8 thresholds, each in [0, max_dist]")
    rows, infos, fwd = [], [], None
    for q, t in ((a64, b64), (b64, a64)):
        d2, _, info = _nn_launch(q, t, max_dist, cell, None)
        rows.append(_nn_stats_launch(d2, q, thr, max_dist))
        infos.append(info)
        fwd = d2 if fwd is None else fwd
    for info in torch.stack(infos).tolist():
        _nn_check(info, max_dist, cell, what)
    return fwd, torch.stack(rows)


def metrics_from_stats(ab, ba, thresholds):
    """The dict of ``cloud_metrics`` from the two [5 + T] stat rows (host numbers)."""
    out = {}
    for name, r in (("ab", ab), ("ba", ba)):
        n, matched = float(r[0]), float(r[1])
        out[name] = {"n": int(n), "matched": int(matched),
                     "mean": float(r[2]) / matched if matched else float("nan"),
                     "rms": float(np.sqrt(float(r[3]) / matched)) if matched else float("nan"),
                     "max": float(r[4]), "within": [int(v) for v in r[5:]]}
    out["chamfer"] = out["ab"]["mean"] + out["ba"]["mean"]
    out["thresholds"] = [float(v) for v in thresholds]
    pr = [w / out["ab"]["n"] if out["ab"]["n"] else 0.0 for w in out["ab"]["within"]]
    rc = [w / out["ba"]["n"] if out["ba"]["n"] else 0.0 for w in out["ba"]["within"]]
    out["precision"], out["recall"] = pr, rc
    out["fscore"] = [2 * p * r / (p + r) if p + r > 0 else 0.0 for p, r in zip(pr, rc)]
    return out


def cloud_metrics(a, b, max_dist, thresholds=(0.1, 0.2, 0.5), cell=None):
    """Chamfer distance and precision / recall / F-score between clouds ``a`` (e.g. a completion) and ``b``
    (e.g. its reference), from the exact nearest neighbours within ``max_dist`` in both directions.

    Returns {"ab": {n, matched, mean, rms, max, within[k]}, "ba": {...}, "chamfer": mean_ab + mean_ba,
    "thresholds", "precision"[k] = within_ab[k] / n_a, "recall"[k] = within_ba[k] / n_b, "fscore"[k] =
    2PR / (P + R) or 0}.  n counts the points with finite coordinates, matched those with a neighbour within
    max_dist; mean / rms / max run over the matched (NaN when none), so a point farther than max_dist from
    the other cloud lowers precision / recall but not the means.  Thresholds must not exceed max_dist.
    Everything runs on the device (``cloud_distance_stats``); the host reads the grids' status and the two rows of sums at the end."""
    thr = [float(v) for v in thresholds]
    _, rows = cloud_distance_stats(a, b, max_dist, thr, cell)
    ab, ba = rows.tolist()
    return metrics_from_stats(ab, ba, thr)


SSC_GRID = {"origin": (0.0, -25.6, -2.0), "voxel": 0.2, "dims": (256, 256, 32)}   # SemanticKITTI-SSC, 51.2 x 51.2 x 6.4 m


def _grid_args(origin, voxel, dims, num_classes, what):
    org = [float(v) for v in np.asarray(origin, dtype=np.float64).reshape(-1)]
    if len(org) != 3 or not all(np.isfinite(org)):
        raise ValueError(f"{what}: origin must be three finite numbers")
    voxel = float(voxel)
    if not voxel > 0 or not np.isfinite(voxel):
        raise ValueError(f"{what}: voxel must be > 0 and finite")
    d = [int(v) for v in dims]
    if len(d) != 3 or any(v < 1 for v in d) or any(int(v) != v for v in dims):
        raise ValueError(f"{what}: dims must be three integers >= 1")
    if d[0] * d[1] * d[2] > 2 ** 40:
        raise ValueError(f"{what}: a grid of {d[0]} x {d[1]} x {d[2]} cells exceeds 2^40 cells")
    if not 1 <= int(num_classes) <= 64:
        raise ValueError(f"{what}: num_classes must be in [1, 64]")
    return org, voxel, d, int(num_classes)


def _labels_i32(t, n, dev, what):
    if t is None:
        return None
    if not torch.is_tensor(t) or not t.is_cuda or t.device != dev or tuple(t.shape) != (n,) or \
            t.dtype.is_floating_point or t.dtype == torch.bool:
        raise ValueError(f"{what} must be a cuda integer [{n}] tensor on the clouds' device")
    return t.to(torch.int32).contiguous()


def voxel_confusion(truth, pred, origin, voxel, dims, truth_labels=None, pred_labels=None, num_classes=1,
                    valid=None, return_cells=False):
    """The confusion matrix of voxel states between clouds ``truth`` and ``pred`` on one fixed grid, on the device
    (``sdp_voxel_iou``, csrc/voxel_iou.hip; the contract stands in include/sdp.h).

    truth, pred: cuda [n,3] or [n,4] (xyz first), float64 (float32 is widened).  origin: the grid's low corner [3],
    voxel: its cell size, dims = (nx, ny, nz).  A point lies in cell floor((p - origin) / voxel) per axis, in float64;
    points outside the grid, with a non-finite coordinate, with a label outside [0, num_classes) or in a cell where
    ``valid`` is 0 are not used.  *_labels: cuda integer [n] or None (every label 0); valid: cuda [nz,ny,nx] or None.

    Returns (confusion int64 [C+1, C+1] -- row = state of the voxel in truth, column = in pred, state 0 = empty,
    1 + c = occupied with majority label c (smallest label among equal votes); it sums to the number of valid cells
    -- and info int64 [8] = m_truth, m_pred, points used of truth, of pred, bad labels of truth, of pred,
    |truth n pred|, valid cells), both on the device: no host sync.  With return_cells also two tuples (cells int64
    [m], labels int32 [m], counts int32 [m]), the occupied voxels of truth and of pred in ascending cell key
    (ix + nx*iy + nx*ny*iz); that costs the one host sync that reads m."""
    what = "voxel_confusion"
    a, b = _xyz64(truth, "truth"), _xyz64(pred, "pred")
    if a.device != b.device:
        raise ValueError("truth and pred must be on the same device")
    dev = a.device
    org, voxel, d, C = _grid_args(origin, voxel, dims, num_classes, what)
    na, nb = a.shape[0], b.shape[0]
    la, lb = _labels_i32(truth_labels, na, dev, "truth_labels"), _labels_i32(pred_labels, nb, dev, "pred_labels")
    if valid is not None:
        if d[0] * d[1] * d[2] > 2 ** 31:
            raise ValueError(f"{what}: a valid mask needs a grid of at most 2^31 cells")
        valid = _mask_u8(valid, (d[2], d[1], d[0]), "valid")
        if valid.device != dev:
            raise ValueError("valid must be on the clouds' device")
    L = _lib.lib()
    ws = _workspace("voxel_iou", na, nb, C, device=dev)
    with torch.cuda.device(dev):
        conf = torch.empty(C + 1, C + 1, dtype=torch.int64, device=dev)
        info = torch.empty(8, dtype=torch.int64, device=dev)
        cells = [None] * 6
        if return_cells:
            cells = [torch.empty(n, dtype=dt, device=dev) for n in (na, nb)
                     for dt in (torch.int64, torch.int32, torch.int32)]
        opt = lambda t: _lib.ptr(t) if t is not None and t.numel() else None
        _lib.check(L.sdp_voxel_iou(opt(a), na, a.shape[1], opt(la), opt(b), nb, b.shape[1], opt(lb),
                                   (_lib.D * 3)(*org), voxel, (_lib.C.c_int64 * 3)(*d), C, _lib.ptr(valid),
                                   conf.data_ptr(), *(opt(t) for t in cells), info.data_ptr(), ws.data_ptr(),
                                   ws.numel(), _lib.stream()), "voxel_iou")
        if return_cells:
            ma, mb = (int(v) for v in info[:2].tolist())
            return conf, info, tuple(t[:ma] for t in cells[:3]), tuple(t[:mb] for t in cells[3:])
    return conf, info


def iou_from_confusion(conf, ignore=()):
    """Completion and semantic IoU from a ``voxel_confusion`` matrix [C+1, C+1] (tensor or array), on the host.

    Occupancy over the states > 0: TP = voxels occupied in both, FP = only in the prediction (row 0), FN = only
    in the truth (column 0); iou = TP / (TP + FP + FN), precision = TP / (TP + FP), recall = TP / (TP + FN), NaN
    where the denominator is 0.  class_iou[c] = conf[1+c][1+c] / (row + column - diagonal) over the full matrix, NaN
    where that union is 0; miou = the mean over the classes not in ``ignore`` whose union is non-zero, NaN if there
    are none.  Returns a dict with these and the integers tp, fp, fn."""
    m = conf.detach().cpu().numpy() if torch.is_tensor(conf) else np.asarray(conf)
    if m.ndim != 2 or m.shape[0] != m.shape[1] or m.shape[0] < 2:
        raise ValueError(f"iou_from_confusion expects a [C+1, C+1] matrix, got {m.shape}")
    m = m.astype(np.int64)
    C = m.shape[0] - 1
    ignore = {int(c) for c in ignore}
    if any(not 0 <= c < C for c in ignore):
        raise ValueError(f"ignore must name classes in [0, {C})")
    tp, fp, fn = int(m[1:, 1:].sum()), int(m[0, 1:].sum()), int(m[1:, 0].sum())
    ratio = lambda num, den: num / den if den else float("nan")
    diag = np.diagonal(m)[1:]
    union = m.sum(1)[1:] + m.sum(0)[1:] - diag
    class_iou = np.full(C, np.nan)
    np.divide(diag, union, out=class_iou, where=union > 0)
    keep = [c for c in range(C) if c not in ignore and union[c] > 0]
    return {"iou": ratio(tp, tp + fp + fn), "precision": ratio(tp, tp + fp), "recall": ratio(tp, tp + fn),
            "tp": tp, "fp": fp, "fn": fn, "class_iou": class_iou,
            "miou": float(np.mean(class_iou[keep])) if keep else float("nan")}


def voxel_iou(truth, pred, origin, voxel, dims, truth_labels=None, pred_labels=None, num_classes=1, valid=None,
              ignore=()):
    """``iou_from_confusion`` of ``voxel_confusion``: the completion IoU (and, with labels, per-class IoU / mIoU)
    of ``pred`` against ``truth`` on the given grid.  The dict also holds "confusion" and "info" as host arrays.
    One host sync, to read the matrix."""
    conf, info = voxel_confusion(truth, pred, origin, voxel, dims, truth_labels, pred_labels, num_classes, valid)
    host = torch.cat((conf.reshape(-1), info)).cpu().numpy()
    out = iou_from_confusion(host[:-8].reshape(conf.shape), ignore)
    out["confusion"], out["info"] = host[:-8].reshape(conf.shape), host[-8:]
    return out


def volume_to_cloud(labels_volume, origin, voxel, empty=0):
    """A dense label volume [nz,ny,nx] (the SSC ground-truth form; tensor or array, any device) as a labelled
    cloud: for every voxel whose label differs from ``empty`` its centre origin + (i + 0.5) * voxel (float64
    [m,3], in ascending cell key) and its label (int32 [m]), on the volume's device.  On the SSC grid every centre
    falls back into its own cell under ``voxel_confusion``'s arithmetic (tests/test_voxel_iou_ref_cpu.py)."""
    vol = torch.as_tensor(labels_volume)
    if vol.dim() != 3:
        raise ValueError(f"volume_to_cloud expects a [nz,ny,nx] volume, got {tuple(vol.shape)}")
    org = torch.as_tensor(np.asarray(origin, dtype=np.float64).reshape(3), device=vol.device)
    idx = torch.nonzero(vol != empty)                      # [m,3] (iz, iy, ix), row-major = ascending key
    pts = org + (idx.flip(1).to(torch.float64) + 0.5) * float(voxel)
    return pts, vol[idx[:, 0], idx[:, 1], idx[:, 2]].to(torch.int32)


def fuse_views(x, origins=None, poses=None, keep=None, exist=None, min_range=1.5, geometry="dataset",
               grid=None, center=None):
    """The views of one scan as a single cloud [n,4] (SceneCompleter.py:261-264).  With grid=dl the cloud
    is put on a voxel grid of that size (``voxel_grid_subsample`` around ``center``): [m,4] float64, the
    barycentre and the mean intensity of every occupied voxel."""
    cloud = range_image_to_point_cloud(x, origins, poses, keep, exist, min_range, geometry)[0]
    if grid is None:
        return cloud
    if cloud.shape[0] == 0:
        return cloud
    pts, inten = voxel_grid_subsample(cloud[:, :3], features=cloud[:, 3:4], sampleDl=grid, center=center)
    return torch.cat((pts, inten.to(torch.float64)), 1)


def write_bin(path, points) -> None:
    """Write a cloud as float32 [n][4] (x, y, z, intensity): the KITTI .bin layout sdp.kitti360 reads."""
    p = points.detach().cpu().numpy() if torch.is_tensor(points) else np.asarray(points)
    if p.ndim != 2 or p.shape[1] != 4:
        raise ValueError(f"write_bin expects [n,4] points, got {p.shape}")
    np.ascontiguousarray(p, dtype=np.float32).tofile(path)
