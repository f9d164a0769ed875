"""Time sdp_cloud_nn + sdp_cloud_nn_stats (csrc/cloud_nn.hip) per stage and in total against the same question
asked of the host.

    python tools/cloud_nn_bench.py [--views 32] [--max-dist 0.5] [--cell 0.5 0.125] [--iters 20] [--host-iters 3]
                                   [--out FILE.json]

Input: the fused cloud of `views` procedural views of 64x1024 (sdp.synthetic.scene_views, poses 5 m apart, every
pixel kept: 32 views = 2,097,152 rows) as the targets, and as the queries the same views with range noise (codes
+- 0.005, i.e. +- 2 % of the range), float64 [n,4] both -- a completion scored against its reference.
  device  sdp_cloud_nn and sdp_cloud_nn_stats on preallocated buffers (the C entries, no host sync).  Total: stream
          events around `iters` single pairs of calls after a warm-up, the median.  Stages: the events of
          sdp_cloud_nn_stage_events inside each call (grid build, query) and one more after the stats.
  host    copy both clouds to the host, scipy.spatial.cKDTree(targets).query(queries, distance_upper_bound=R) on
          one core, copy distances and indices back; wall clock with a device sync at both ends, the median of
          `host-iters` runs, each step also on its own.
The two results are compared before anything is timed: the same queries matched, distances within 4 float64 ulps
(the tree's arithmetic order differs), and the number of differing indices (equal distances only) is reported.
Nothing here is a gate: the figures are printed and, with --out, written as JSON.
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

H, W = 64, 1024
THR = (0.1, 0.2, 0.5)


def clouds(views):
    from sdp import synthetic
    from sdp.pointcloud import fuse_views
    sv = synthetic.scene_views(views, H, W)
    x = torch.from_numpy(np.ascontiguousarray(sv["ref"], dtype=np.float32)).cuda()
    poses = torch.from_numpy(np.ascontiguousarray(sv["toWorld"], dtype=np.float64)).cuda()
    g = torch.Generator(device="cpu").manual_seed(1)
    noise = ((torch.rand(x.shape, generator=g) - 0.5) * 0.01).cuda()
    target = fuse_views(x, poses=poses, min_range=-1.0).contiguous()
    query = fuse_views((x + noise).clamp(0, 1), poses=poses, min_range=-1.0).contiguous()
    return query, target, poses[0, :3, 3].contiguous()


def host_path(q, t, R):
    """D2H, cKDTree build + query, H2D; returns (distance, index, seconds of each step)."""
    from scipy.spatial import cKDTree
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    hq, ht = q.cpu().numpy()[:, :3], t.cpu().numpy()[:, :3]
    t1 = time.perf_counter()
    dist, idx = cKDTree(ht).query(hq, k=1, distance_upper_bound=R)
    t2 = time.perf_counter()
    dd, di = torch.from_numpy(dist).cuda(), torch.from_numpy(idx).cuda()
    torch.cuda.synchronize()
    t3 = time.perf_counter()
    return dist, idx, (t1 - t0, t2 - t1, t3 - t2), (dd, di)


def bench(q, t, center, R, cell, iters, host_iters):
    from sdp import _lib
    L = _lib.lib()
    nq, nt = q.shape[0], t.shape[0]
    dev = q.device
    nb, sb = _lib.SZ(), _lib.SZ()
    _lib.check(L.sdp_cloud_nn_workspace_size(nq, nt, C.byref(nb)), "ws")
    _lib.check(L.sdp_cloud_nn_stats_workspace_size(nq, C.byref(sb)), "stats_ws")
    ws = torch.empty(nb.value, dtype=torch.uint8, device=dev)
    sws = torch.empty(sb.value, dtype=torch.uint8, device=dev)
    d2 = torch.empty(nq, dtype=torch.float64, device=dev)
    idx = torch.empty(nq, dtype=torch.int32, device=dev)
    info = torch.empty(8, dtype=torch.int64, device=dev)
    stats = torch.empty(5 + len(THR), dtype=torch.float64, device=dev)
    thr = (_lib.D * len(THR))(*[v * min(1.0, R / 0.5) for v in THR])
    after = torch.cuda.Event(enable_timing=True)

    def call():
        _lib.check(L.sdp_cloud_nn(q.data_ptr(), nq, 4, t.data_ptr(), nt, 4, R, cell, center.data_ptr(), d2.data_ptr(),
                                  idx.data_ptr(), info.data_ptr(), ws.data_ptr(), nb.value, _lib.stream()), "cloud_nn")
        _lib.check(L.sdp_cloud_nn_stats(d2.data_ptr(), q.data_ptr(), 4, nq, thr, len(THR), R, stats.data_ptr(),
                                        sws.data_ptr(), sb.value, _lib.stream()), "cloud_nn_stats")
        after.record()

    call()
    torch.cuda.synchronize()
    assert int(info[0]) > 0, info.tolist()
    hd, hi, _, _ = host_path(q, t, R)
    gd, gi = np.sqrt(d2.cpu().numpy()), idx.cpu().numpy()
    matched = np.isfinite(hd)
    assert np.array_equal(matched, gi >= 0), "device and host match different queries"
    assert (np.abs(gd[matched] - hd[matched]) <= 4 * np.spacing(hd[matched])).all(), "device and host distances differ"
    idx_differ = int((gi[matched] != hi[matched]).sum())

    for _ in range(2):
        call()
    torch.cuda.synchronize()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
    for e in ev:
        e.record()
    torch.cuda.synchronize()
    _lib.check(L.sdp_cloud_nn_stage_events((_lib.P * 3)(*[e.cuda_event for e in ev])), "stage_events")
    rows = []
    try:
        for _ in range(iters):
            call()
            torch.cuda.synchronize()
            rows.append([ev[0].elapsed_time(after), ev[0].elapsed_time(ev[1]), ev[1].elapsed_time(ev[2]),
                         ev[2].elapsed_time(after)])
    finally:
        _lib.check(L.sdp_cloud_nn_stage_events(None), "stage_events")
    host = [host_path(q, t, R)[2] for _ in range(host_iters)]
    med = lambda k: statistics.median(r[k] for r in rows)
    host_total = statistics.median(sum(h) for h in host) * 1e3
    return dict(queries=nq, targets=nt, max_dist=R, cell=cell, info=info.tolist(), matched=int(matched.sum()),
                index_differs=idx_differ, stats=stats.tolist(), device_ms=med(0),
                device_stage_ms=dict(grid=med(1), query=med(2), stats=med(3)), host_ms=host_total,
                host_d2h_ms=statistics.median(h[0] for h in host) * 1e3,
                host_kdtree_ms=statistics.median(h[1] for h in host) * 1e3,
                host_h2d_ms=statistics.median(h[2] for h in host) * 1e3, host_over_device=host_total / med(0))


def main(argv=None):
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--views", type=int, default=32)
    p.add_argument("--max-dist", type=float, default=0.5)
    p.add_argument("--cell", type=float, nargs="+", default=[0.5, 0.125])
    p.add_argument("--iters", type=int, default=20)
    p.add_argument("--host-iters", type=int, default=3)
    p.add_argument("--out", type=str, default=None)
    a = p.parse_args(argv)
    if not torch.cuda.is_available():
        raise RuntimeError("an MI355X (HIP device) is required: there is no CPU timing path")
    q, t, center = clouds(a.views)
    rows = []
    for cell in a.cell:
        rows.append(bench(q, t, center, a.max_dist, cell, a.iters, a.host_iters))
        print(json.dumps(rows[-1]), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
