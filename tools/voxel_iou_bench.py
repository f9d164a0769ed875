"""Time sdp_voxel_iou (csrc/voxel_iou.hip) per stage and in total against the same question asked of the host.

    python tools/voxel_iou_bench.py [--views 32] [--voxel 0.2 0.05] [--classes 1 20] [--iters 20] [--host-iters 3]
                                    [--out FILE.json]

Input: the fused cloud of `views` procedural views of 64x1024 (sdp.synthetic.scene_views, poses 5 m apart, every
pixel kept: 32 views = 2,097,152 rows) as the truth, and as the prediction the same views with range noise (codes
+- 0.005, i.e. +- 2 % of the range), float64 [n,4] both.  The grid covers the truth's bounds: origin =
floor(min / V) * V, dims = ceil((max - origin) / V) + 1.  With C = 1 there are no labels; with C > 1 both clouds carry
random labels in [0, C).
  device  sdp_voxel_iou on preallocated buffers (the C entry, no host sync).  Total: stream events around `iters`
          single calls after a warm-up, the median.  Stages: the events of sdp_voxel_iou_stage_events inside each of
          those calls (keys, sort, heads, votes, compare), the median of each.
  host    what a caller does without the entry: copy both clouds (and labels) to the host, tests/voxel_iou_ref.py
          (np.unique over the composite keys of each cloud, on one core), copy the matrix back; wall clock with a device
          sync at both ends, the median of `host-iters` runs, each step also on its own.
The two matrices and info vectors are compared for equality before anything is timed.  Nothing here is a gate: the
figures are printed and, with --out, written as JSON.
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "simultaneous-diffusion-for-pointclouds_amd"))
sys.path.insert(0, os.path.join(REPO, "tests"))

H, W = 64, 1024
STAGES = ("keys", "sort", "heads", "votes", "compare")


def clouds(views):
    from sdp import synthetic
    from sdp.pointcloud import fuse_views
    sv = synthetic.scene_views(views, H, W)
    x = torch.from_numpy(np.ascontiguousarray(sv["ref"], dtype=np.float32)).cuda()
    poses = torch.from_numpy(np.ascontiguousarray(sv["toWorld"], dtype=np.float64)).cuda()
    g = torch.Generator(device="cpu").manual_seed(1)
    noise = ((torch.rand(x.shape, generator=g) - 0.5) * 0.01).cuda()
    truth = fuse_views(x, poses=poses, min_range=-1.0).contiguous()
    pred = fuse_views((x + noise).clamp(0, 1), poses=poses, min_range=-1.0).contiguous()
    return truth, pred


def host_path(truth, tl, pred, pl, origin, V, dims, nc):
    """D2H, the numpy reference, H2D; returns (confusion, info, seconds of each step)."""
    import voxel_iou_ref as IR
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    ht, hp = truth.cpu().numpy(), pred.cpu().numpy()
    htl, hpl = (None if tl is None else tl.cpu().numpy()), (None if pl is None else pl.cpu().numpy())
    t1 = time.perf_counter()
    r = IR.confusion(ht, htl, hp, hpl, origin, V, dims, nc)
    t2 = time.perf_counter()
    dc = torch.from_numpy(r["confusion"]).cuda()
    torch.cuda.synchronize()
    t3 = time.perf_counter()
    return dc, r["info"], (t1 - t0, t2 - t1, t3 - t2)


def bench(truth, pred, V, nc, iters, host_iters):
    from sdp import _lib
    L = _lib.lib()
    dev = truth.device
    na, nb = truth.shape[0], pred.shape[0]
    xyz = truth[:, :3]
    lo, hi = xyz.amin(0).cpu().numpy(), xyz.amax(0).cpu().numpy()
    origin = np.floor(lo / V) * V
    dims = [int(v) for v in np.ceil((hi - origin) / V) + 1]
    tl = pl = None
    if nc > 1:
        g = torch.Generator(device="cpu").manual_seed(2)
        tl = torch.randint(0, nc, (na,), generator=g, dtype=torch.int32).cuda()
        pl = torch.randint(0, nc, (nb,), generator=g, dtype=torch.int32).cuda()
    nbytes = _lib.SZ()
    _lib.check(L.sdp_voxel_iou_workspace_size(na, nb, nc, C.byref(nbytes)), "ws")
    ws = torch.empty(nbytes.value, dtype=torch.uint8, device=dev)
    conf = torch.empty(nc + 1, nc + 1, dtype=torch.int64, device=dev)
    info = torch.empty(8, dtype=torch.int64, device=dev)
    org_c, dims_c = (_lib.D * 3)(*origin), (C.c_int64 * 3)(*dims)

    def call():
        _lib.check(L.sdp_voxel_iou(truth.data_ptr(), na, truth.shape[1], _lib.ptr(tl), pred.data_ptr(), nb, pred.shape[1],
                                   _lib.ptr(pl), org_c, float(V), dims_c, nc, None, conf.data_ptr(), None, None, None,
                                   None, None, None, info.data_ptr(), ws.data_ptr(), nbytes.value, _lib.stream()),
                   "voxel_iou")

    call()
    hc, hinfo, _ = host_path(truth, tl, pred, pl, origin, V, dims, nc)
    assert torch.equal(conf, hc), "device and host confusion matrices differ"
    assert np.array_equal(info.cpu().numpy(), hinfo), "device and host info differ"

    for _ in range(3):
        call()
    torch.cuda.synchronize()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(6)]
    for e in ev:
        e.record()
    torch.cuda.synchronize()
    arr = (_lib.P * 6)(*[e.cuda_event for e in ev])
    _lib.check(L.sdp_voxel_iou_stage_events(arr), "stage_events")
    totals, stages = [], []
    try:
        for _ in range(iters):
            call()
            torch.cuda.synchronize()
            totals.append(ev[0].elapsed_time(ev[5]))
            stages.append([ev[i].elapsed_time(ev[i + 1]) for i in range(5)])
    finally:
        _lib.check(L.sdp_voxel_iou_stage_events(None), "stage_events")
    host = [host_path(truth, tl, pred, pl, origin, V, dims, nc)[2] for _ in range(host_iters)]
    host_total = statistics.median(sum(h) for h in host) * 1e3
    dev_total = statistics.median(totals)
    m = conf.cpu().numpy()
    tp, fp, fn = int(m[1:, 1:].sum()), int(m[0, 1:].sum()), int(m[1:, 0].sum())
    return dict(points=[na, nb], voxel=V, classes=nc, dims=dims, info=info.tolist(), iou=tp / max(tp + fp + fn, 1),
                device_ms=dev_total,
                device_stage_ms={s: statistics.median(r[i] for r in stages) for i, s in enumerate(STAGES)},
                host_ms=host_total, host_d2h_ms=statistics.median(h[0] for h in host) * 1e3,
                host_numpy_ms=statistics.median(h[1] for h in host) * 1e3,
                host_h2d_ms=statistics.median(h[2] for h in host) * 1e3, host_over_device=host_total / dev_total)


def main(argv=None):
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--views", type=int, default=32)
    p.add_argument("--voxel", type=float, nargs="+", default=[0.2, 0.05])
    p.add_argument("--classes", type=int, nargs="+", default=[1, 20])
    p.add_argument("--iters", type=int, default=20)
    p.add_argument("--host-iters", type=int, default=3)
    p.add_argument("--out", type=str, default=None)
    a = p.parse_args(argv)
    if not torch.cuda.is_available():
        raise RuntimeError("an MI355X (HIP device) is required: there is no CPU timing path")
    truth, pred = clouds(a.views)
    rows = []
    for V in a.voxel:
        for nc in a.classes:
            rows.append(bench(truth, pred, V, nc, a.iters, a.host_iters))
            print(json.dumps(rows[-1]), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
