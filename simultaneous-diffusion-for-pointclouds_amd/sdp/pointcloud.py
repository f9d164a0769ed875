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
"""
from __future__ import annotations

import numpy as np
import torch

from . import _lib

GEOMETRY = {"dataset": 0, "sampler": 1}


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
    n = _lib.SZ()
    _lib.check(L.sdp_range_unproject_workspace_size(B, H, W, _lib.C.byref(n)), "range_unproject_ws")
    with torch.cuda.device(dev):
        ws = torch.empty(n.value, dtype=torch.uint8, device=dev)
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


def fuse_views(x, origins=None, poses=None, keep=None, exist=None, min_range=1.5, geometry="dataset"):
    """The views of one scan as a single cloud [n,4] (SceneCompleter.py:261-264)."""
    return range_image_to_point_cloud(x, origins, poses, keep, exist, min_range, geometry)[0]


def write_bin(path, points) -> None:
    """Write a cloud as float32 [n][4] (x, y, z, intensity): the KITTI .bin layout sdp.kitti360 reads."""
    p = points.detach().cpu().numpy() if torch.is_tensor(points) else np.asarray(points)
    if p.ndim != 2 or p.shape[1] != 4:
        raise ValueError(f"write_bin expects [n,4] points, got {p.shape}")
    np.ascontiguousarray(p, dtype=np.float32).tofile(path)
