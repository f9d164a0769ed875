"""Time sdp_range_unproject (csrc/unproject.hip) against the same cloud built from torch ops.

    python tools/unproject_bench.py [--views 8 42] [--iters 50] [--out FILE.json]

Both formulations run in one process on the same seeded inputs (64x1024 views, origins placement,
the per-view and the shared keep mask, ~70 % of the pixels kept) and are timed with stream events
around `iters` back-to-back calls after a warm-up:
  hip    the three launches of sdp_range_unproject on preallocated outputs (the C entry, no host sync);
  torch  float64 tensor ops (exp2, cos / sin tables, broadcast multiply-add, stack) followed by boolean
         indexing -- the formulation a user without this kernel would write; its nonzero syncs the host,
         which is part of what it costs.
The two clouds are compared before anything is timed.  The fraction of the HBM roofline uses the
algorithmic bytes of DESIGN section 4 -- 8 B per pixel (the code twice: count and scatter), 1 B per mask
read per pass and 32 B of row per kept point, 4 B more with `pixel` -- over the
measured copy bandwidth (6.29 TB/s).  Nothing here is a gate: the figures are printed and, with --out,
written as JSON.
"""
import argparse
import json
import math
import os
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "simultaneous-diffusion-for-pointclouds_amd"))

HBM_BYTES_PER_S = 6.29e12   # measured float4 copy on one MI355X
H, W = 64, 1024


def torch_formulation(x, origins, keep, exist, min_range=1.5):
    B = x.shape[0]
    hA, vA = math.radians(360) / W, math.radians(28) / H
    hMin, vMin = W // (-2) * hA + hA / 2, math.radians(3 - 28)
    az = (torch.arange(W - 1, -1, -1, device=x.device, dtype=torch.float64) * hA + hMin).view(1, 1, W)
    el = (torch.arange(H - 1, -1, -1, device=x.device, dtype=torch.float64) * vA + vMin).view(1, H, 1)
    v = x[:, 0].abs() * 6.0
    rd = torch.exp2(v.double()).float() - 1.0
    rdd = rd.double()
    o = origins.view(B, 3, 1, 1)
    px = rdd * torch.cos(az) * torch.cos(el) + o[:, 0]
    py = rdd * torch.sin(az) * torch.cos(el) + o[:, 1]
    pz = rdd * torch.sin(el) + o[:, 2]
    mask = (rd > min_range) & keep.bool() & exist.bool().unsqueeze(0)
    cloud = torch.stack((px, py, pz, x[:, 1].double()), -1)[mask]
    offsets = torch.cat((mask.new_zeros(1, dtype=torch.int64), mask.view(B, -1).sum(1).cumsum(0)))
    return cloud, offsets


def event_time_ms(fn, iters, warmup=5):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(iters):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / iters


def bench(B, iters):
    from sdp import _lib
    from sdp.pointcloud import range_image_to_point_cloud
    dev = torch.device("cuda")
    g = torch.Generator(device="cpu").manual_seed(1234 + B)
    x = (torch.rand(B, 2, H, W, generator=g) * 0.95 + 0.05).to(dev)
    low = torch.rand(B, H, W, generator=g) < 0.1
    x[:, 0][low.to(dev)] = 0.1                                   # rd = 0.52: dropped
    keep = (torch.rand(B, H, W, generator=g) < 0.88).to(dev).to(torch.uint8)
    exist = (torch.rand(H, W, generator=g) < 0.9).to(dev).to(torch.uint8)
    origins = (torch.rand(B, 3, generator=g, dtype=torch.float64) * 10).to(dev)

    pts, off, pix = range_image_to_point_cloud(x, origins=origins, keep=keep, exist=exist, return_pixel=True)
    tc, toff = torch_formulation(x, origins, keep, exist)
    assert torch.equal(off, toff), "the two formulations disagree on the kept set"
    err = float((pts - tc).abs().max())
    assert err <= 1e-12 * max(1.0, float(tc[:, :3].abs().max())), err

    L = _lib.lib()
    n = _lib.SZ()
    _lib.check(L.sdp_range_unproject_workspace_size(B, H, W, _lib.C.byref(n)), "ws")
    ws = torch.empty(n.value, dtype=torch.uint8, device=dev)
    points = torch.empty(B * H * W, 4, dtype=torch.float64, device=dev)
    pixel = torch.empty(B * H * W, dtype=torch.int32, device=dev)
    offsets = torch.empty(B + 1, dtype=torch.int64, device=dev)

    def hip(with_pixel):
        _lib.check(L.sdp_range_unproject(x.data_ptr(), B, 2, H, W, 0, origins.data_ptr(), None, keep.data_ptr(),
                                         exist.data_ptr(), 1.5, points.data_ptr(),
                                         pixel.data_ptr() if with_pixel else None, offsets.data_ptr(), ws.data_ptr(),
                                         n.value, _lib.stream()), "range_unproject")

    t_hip = event_time_ms(lambda: hip(False), iters)
    t_hip_pix = event_time_ms(lambda: hip(True), iters)
    t_torch = event_time_ms(lambda: torch_formulation(x, origins, keep, exist), max(3, iters // 5), warmup=2)
    n_pix, n_kept = B * H * W, int(off[-1])
    algo = n_pix * (8 + 2 * 2) + n_kept * 32                # two masks, each read by both passes
    floor_ms = algo / HBM_BYTES_PER_S * 1e3
    return dict(views=B, pixels=n_pix, kept=n_kept, kept_fraction=n_kept / n_pix, max_abs_diff_vs_torch=err,
                hip_ms=t_hip, hip_with_pixel_ms=t_hip_pix, torch_ms=t_torch, algorithmic_bytes=algo,
                hbm_floor_ms=floor_ms, hbm_roofline_fraction=floor_ms / t_hip, speedup_vs_torch=t_torch / t_hip)


def main(argv=None):
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--views", type=int, nargs="+", default=[8, 42])
    p.add_argument("--iters", type=int, default=50)
    p.add_argument("--out", type=str, default=None)
    a = p.parse_args(argv)
    if not torch.cuda.is_available():
        raise RuntimeError("an MI355X (HIP device) is required: there is no CPU timing path")
    rows = [bench(B, a.iters) for B in a.views]
    for r in rows:
        print(json.dumps(r))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
