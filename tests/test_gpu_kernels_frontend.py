"""Per-kernel parity of the data front end -- csrc/projection.hip (sdp_range_project and its sky / obfuscation scan,
the latter also alone through sdpk_range_sky_scan) and csrc/kitti_view.hip (sdp_view_transform, sdp_view_gather,
sdp_view_finalize) -- against float64 numpy references of the same operations, EVERY element, no mismatch fraction.

Why exact: all four are float64 without contraction, in the reference's evaluation order.  The only device functions
that may differ from the host's libm are atan2 (projection: it only feeds a round-to-bin) and log2 (finalize: the depth
code, graded to rtol 1e-13, the bar tests/test_gpu_kitti_view.py sets).  A bin can only differ for a point within the
atan2 error of a bin edge, and KR.bin_edge_guard asserts -- from the reference's arithmetic alone, before anything runs
on the device -- that no finite point of a cloud is within 1e-9 bins of an edge that decides anything (derivation in its
docstring).  One kind of point is outside the guard by construction: a point AT the view origin has the azimuth
atan2(+-0, +-0), which IEEE 754 / C Annex F fix at exactly 0 or +-pi, so its column (W/2 - 1/2, rounded half to even)
is the same correctly rounded subtraction and division on both sides; the guard checks its row only.  Non-finite points
have no bin: NaN angles clamp to row / column 0 on both sides and are excluded.

Every output buffer is prefilled with a sentinel (NaN for float64, 0xFF for uint8, -7 for int64 / int32), so an element
a kernel fails to write shows up; a rejected call must leave the sentinels in place.

What the inputs reach that the 64x1024 goldens and the seeded KITTI scans do not (each asserted below from the
reference alone, so a reseed cannot empty a test):
  proj_sky_kernel        the still-sky chain alive for >= 8 rows, x == min_depth + 5 (the strict compare), H = 3 (loop
                         body never run), one row, (H - 3) % 16 in {15, 0, 1} (full / partial register batches), odd W,
                         W no multiple of 64, W = 65 (one lane past a wave), the 1024-thread block;
  proj_depth / _index    a second grid-stride pass (N > 4096 * 256) with >= 100 pixels won through an equal-depth tie
                         whose two indices lie in different passes; ties and z-buffer losers in every lattice cloud;
  proj_pixel_kernel      depth-0 winner over a farther point, +inf depth, every optional output absent, strides 3 / 6;
  view_finalize_kernel   set sky bits (rows 0-2 and the last three included) under the 3-row shift and the roll,
                         intensity >= 1 against the rolled mask, inten_code's cut, channels 1, H * W no multiple of 256,
                         variant 3 with and without goal;
  view_gather_kernel     HW < 1024, HW no multiple of 1024, blank_cols 0 / W / > W, count 0;
  view_transform_kernel  n = 1, partial blocks, m1 only, no matrix.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import kernel_lib as KL
import kernel_ref as KR
from oracle import projection_ref as PR
from sdp import _lib

pytestmark = pytest.mark.gpu
MAXR = PR.MAX_RANGE
GRID_CAP = 4096 * 256            # threads of one grid-stride pass of proj_depth_kernel / proj_index_kernel


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def filled(shape, dtype):
    """A device buffer of sentinels: NaN / 0xFF / -7."""
    v = {torch.float64: float("nan"), torch.uint8: 0xFF, torch.int64: -7, torch.int32: -7}[dtype]
    return torch.full(shape, v, dtype=dtype, device="cuda")


def untouched(t):
    if t.dtype == torch.float64:
        return bool(torch.isnan(t).all())
    return bool((t == (0xFF if t.dtype == torch.uint8 else -7)).all())


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def last_error():
    return _lib.lib().sdp_last_error().decode()


# ---- the sky / obfuscation scan, one launch --------------------------------------------------------------------------

SKY_SHAPES = [(3, 64), (4, 7), (18, 100), (19, 100), (20, 100), (35, 1024), (64, 1024), (64, 65)]


def sky_image(H, W):
    r = KR.rng_for(f"sky-scan-{H}x{W}")
    xy = r.choice([MAXR, 3.0, 8.0, 13.0, 18.0, 40.0], size=(H, W), p=(.55, .09, .09, .09, .09, .09))
    top = xy[:H // 2]
    top[r.random(top.shape) < 0.8] = MAXR
    return xy


def sky_scan_stats(xy):
    """oracle.projection_ref.sky_scan's recurrence again, only to count what it meets: the last row at which the
    still-sky chain is alive in some column, and how often the strict compare sees x == min_depth + 5."""
    H, W = xy.shape
    md = np.zeros(W) + MAXR
    prev = np.ones(W, bool)
    last_alive, equal = 1, 0
    obf = np.zeros((H, W), bool)
    for row in range(2, H - 1):
        obf[row] = xy[row] > md + 5
        equal += int((xy[row] == md + 5).sum())
        e = (xy[row] != md).astype(int) + (xy[row - 1] != md).astype(int) + (xy[row + 1] != md).astype(int)
        e = np.concatenate(([0], e, [0]))
        cur = (e[1:-1] + e[:-2] + e[2:] <= 1) & prev
        if cur.any():
            last_alive = row
        md = np.where(cur, md, np.minimum(xy[row], md))
        prev = cur
    obf[-1] = xy[-1] > md + 5
    equal += int((xy[-1] == md + 5).sum())
    assert np.array_equal(obf, PR.sky_scan(xy)[0])          # the counts belong to the reference's own computation
    return last_alive, equal


def run_sky_scan(xy):
    H, W = xy.shape
    obf, sky = filled((H, W), torch.uint8), filled((H, W), torch.uint8)
    KL.check(KL.lib().sdpk_range_sky_scan(KL.ptr(dev(xy)), H, W, KL.ptr(obf), KL.ptr(sky), KL.stream()), "sky_scan")
    torch.cuda.synchronize()
    return obf.cpu().numpy(), sky.cpu().numpy()


@pytest.mark.parametrize("H,W", SKY_SHAPES)
def test_sky_scan_equals_the_reference(H, W):
    xy = sky_image(H, W)
    want, _ = PR.sky_scan(xy)
    last_alive, equal = sky_scan_stats(xy)
    print(f"sky {H}x{W}: chain alive up to row {last_alive}, x == md + 5 met {equal} times, {int(want.sum())} obf set")
    if H >= 18:
        assert last_alive >= 9, last_alive        # rows 2..9: alive for 8 rows
        assert equal >= 10 and want.sum() >= 100
    obf, sky = run_sky_scan(xy)
    assert np.array_equal(obf, want.astype(np.uint8)), int((obf != want).sum())
    assert not sky.any()


@pytest.mark.parametrize("value", [MAXR, 8.0])
@pytest.mark.parametrize("H,W", [(3, 64), (20, 100)])
def test_sky_scan_of_an_empty_and_of_a_constant_image(H, W, value):
    xy = np.full((H, W), value)
    obf, sky = run_sky_scan(xy)
    assert np.array_equal(obf, PR.sky_scan(xy)[0].astype(np.uint8)) and not sky.any()


@pytest.mark.parametrize("H,W", [(2, 64), (20, 0), (20, 1025), (0, 64)])
def test_sky_scan_rejects_a_shape_it_cannot_run(H, W):
    xy = dev(np.full((32, 1025), 8.0))
    obf, sky = filled((32, 1025), torch.uint8), filled((32, 1025), torch.uint8)
    rc = KL.lib().sdpk_range_sky_scan(KL.ptr(xy), H, W, KL.ptr(obf), KL.ptr(sky), KL.stream())
    torch.cuda.synchronize()
    assert rc != 0 and "sdpk_range_sky_scan" in last_error()
    assert untouched(obf) and untouched(sky)


# ---- sdp_range_project -----------------------------------------------------------------------------------------------

def ws_bytes(H, W):
    n = _lib.SZ()
    _lib.check(_lib.lib().sdp_range_project_workspace_size(H, W, C.byref(n)), "ws")
    return n.value


def project(pts, origin, H, W, N=None, stride=None, has_int=1, intensity=True, index=True, scan=True, obf_only=False,
            ws_short=0, ws_size=None):
    """One sdp_range_project call over sentinel-filled outputs -> (rc, {name: numpy array of each output given})."""
    pts = np.ascontiguousarray(pts, np.float64)
    N = len(pts) if N is None else N
    stride = pts.shape[1] if stride is None else stride
    out = {"depth": filled((H, W), torch.float64)}
    if intensity:
        out["intensity"] = filled((H, W), torch.float64)
    if scan or obf_only:
        out["obf"] = filled((H, W), torch.uint8)
    if scan:
        out["sky"] = filled((H, W), torch.uint8)
    if index:
        out["index"] = filled((H, W), torch.int64)
    if ws_size is None:       # a shape the library sizes no workspace for still gets one that would hold its layout
        ws_size = ws_bytes(H, W) if H >= 3 and 1 <= W <= 1024 else H * W * 20 + 8
    size = ws_size
    ws = torch.empty(max(size, 8), dtype=torch.uint8, device="cuda")
    p = dev(pts) if pts.size else None
    o = np.ascontiguousarray(np.asarray(origin, np.float64).reshape(3))
    rc = _lib.lib().sdp_range_project(KL.ptr(p), N, stride, has_int, o.ctypes.data, H, W, KL.ptr(out["depth"]),
                                      KL.ptr(out.get("intensity")), KL.ptr(out.get("obf")), KL.ptr(out.get("sky")),
                                      KL.ptr(out.get("index")), KL.ptr(ws), size - ws_short, _lib.stream())
    torch.cuda.synchronize()
    return rc, out


def reference(pts, origin, H, W):
    with np.errstate(all="ignore"):
        d, it, obf, _, sky, idx = PR.point_cloud_to_range_image(np.asarray(pts, np.float64)[:, :4], origin, True, H, W)
    return {"depth": d, "intensity": it, "obf": obf.astype(np.uint8), "sky": sky.astype(np.uint8),
            "index": idx.astype(np.int64)}


def assert_equal_images(out, ref, what=""):
    """Every pixel of every output present: floats by bit pattern, the rest by value."""
    for k, t in out.items():
        g = t.cpu().numpy() if isinstance(t, torch.Tensor) else t
        w = ref[k].cpu().numpy() if isinstance(ref[k], torch.Tensor) else ref[k]
        if g.dtype == np.float64:
            n = int((bits(g) != bits(w)).sum())
        else:
            n = int((g != w).sum())
        assert n == 0, f"{what} {k}: {n} of {g.size} pixels differ"


def check_projection(pts, origin, H, W, what):
    KR.bin_edge_guard(pts, origin, H, W)
    ref = reference(pts, origin, H, W)
    rc, out = project(pts, origin, H, W)
    assert rc == 0, last_error()
    assert not ref["sky"].any()
    assert_equal_images(out, ref, what)
    return ref


def bin_centre_points(rows, cols, rng_xy, H, W):
    """Points at the centres of the (pre-flip) bins (rows, cols), planar range rng_xy."""
    hA, vA, hMin, vMin = PR.geometry(H, W)
    h, v = hMin + cols * hA, vMin + rows * vA
    return np.stack([rng_xy * np.cos(h), rng_xy * np.sin(h), rng_xy * np.tan(v)], axis=1)


def lattice_cloud(H, W):
    """One point at the bin centre of a random 45 % of the pixels (row 0 and column 0, which the projection excludes,
    among them), a second, farther one in a third of those, and in a tenth an exact duplicate of the nearer one with
    another intensity; the cloud shuffled, so which of a tie's two indices is lower -- the winner -- is the seed's."""
    r = KR.rng_for(f"lattice-cloud-{H}x{W}")
    pix = np.flatnonzero(r.random(H * W) < 0.45)
    rows, cols = pix // W, pix % W
    rng_xy = r.uniform(2.0, 60.0, len(pix))
    near = bin_centre_points(rows, cols, rng_xy, H, W)
    far_sel = r.random(len(pix)) < 1 / 3
    far = bin_centre_points(rows[far_sel], cols[far_sel], rng_xy[far_sel] * r.uniform(1.2, 3.0, far_sel.sum()), H, W)
    dup = near[r.random(len(pix)) < 0.1]
    xyz = np.concatenate([near, far, dup])
    pts = np.concatenate([xyz, r.uniform(0.0, 1.0, (len(xyz), 1))], axis=1)
    return pts[r.permutation(len(pts))]


def tie_pixels(pts, ref):
    """Pixels whose winner has an exact duplicate (x, y, z) at a higher index: won through the tie rule."""
    win = ref["index"][ref["index"] >= 0]
    _, inv, cnt = np.unique(pts[:, :3], axis=0, return_inverse=True, return_counts=True)
    return int((cnt[inv.reshape(-1)[win]] > 1).sum())


@pytest.mark.parametrize("H,W", [(3, 64), (20, 100), (16, 128), (64, 1024), (5, 7)])     # 5 x 7: an odd pixel count
def test_projection_of_a_lattice_cloud_is_exact(H, W):
    pts = lattice_cloud(H, W)
    ref = check_projection(pts, np.zeros(3), H, W, f"lattice {H}x{W}")
    filled_px, ties = int((ref["index"] >= 0).sum()), tie_pixels(pts, ref)
    losers = len(pts) - filled_px
    print(f"lattice {H}x{W}: {len(pts)} points, {filled_px} pixels filled, {ties} through a tie, {losers} points lose, "
          f"{int(ref['obf'].sum())} obf set")
    assert ties >= (1 if H * W < 200 else 10) and losers > ties and filled_px > 0.3 * (H - 1) * (W - 1)
    if H > 5:
        assert ref["obf"].any()


def two_pass_cloud():
    """N = 2^20 + 5000 uniform points at 16x128 (planar range >= 2) and 600 nearer bin-centre points (range < 1), each
    the nearest of a pixel of its own, in exact pairs: 300 pairs with one index in the first grid-stride pass
    (i < 4096 * 256) and one in the second, which the first-pass index must win, and 150 pairs with both indices in the
    first and 150 with both in the second pass, whose pixels a second-pass index wins over farther first-pass points."""
    H, W = 16, 128
    N = 2 ** 20 + 5000
    assert N > GRID_CAP
    r = KR.rng_for("two-pass-cloud")
    hA, vA, hMin, vMin = PR.geometry(H, W)
    h = r.uniform(-np.pi, np.pi, N)
    v = r.uniform(vMin - 2 * vA, vMin + (H + 1) * vA, N)
    rr = r.uniform(2.0, 60.0, N)
    pts = np.stack([rr * np.cos(h), rr * np.sin(h), rr * np.tan(v), r.uniform(0.0, 1.0, N)], axis=1)
    pix = r.permutation((H - 1) * (W - 1))[:600]
    rows, cols = 1 + pix // (W - 1), 1 + pix % (W - 1)
    near = bin_centre_points(rows, cols, r.uniform(0.5, 1.0, 600), H, W)
    first = r.permutation(GRID_CAP)[:750]                   # slots in the first pass
    second = GRID_CAP + r.permutation(N - GRID_CAP)[:750]   # slots in the second
    a = np.concatenate([first[:300], first[300:450], second[300:450]])      # 300 cross, 150 first-first, 150 second-second
    b = np.concatenate([second[:300], first[450:600], second[450:600]])
    pts[a, :3] = near
    pts[b, :3] = near
    cross = np.zeros(N, bool)
    cross[a[:300]] = cross[b[:300]] = True
    return pts, H, W, cross


def test_projection_past_the_grid_cap_keeps_the_lowest_index_across_passes():
    pts, H, W, cross = two_pass_cloud()
    ref = check_projection(pts, np.zeros(3), H, W, "two-pass")
    win = ref["index"][ref["index"] >= 0]
    n_cross = int(cross[win].sum())
    print(f"two-pass: N = {len(pts)}, {n_cross} pixels won through a tie across the passes, {tie_pixels(pts, ref)} ties")
    assert n_cross >= 100 and (win[cross[win]] < GRID_CAP).all()
    assert tie_pixels(pts, ref) >= n_cross + 200
    assert (win >= GRID_CAP).sum() >= 100                   # and second-pass points win pixels at all


def edge_cloud(with_origin_point=True):
    """About 300 uniform points, none in ORIGIN_PIXEL, and, from index 150 on, the special ones.  ORIGIN_PIXEL is where the oracle's arithmetic puts a
    point at the origin (azimuth and elevation 0); x = +inf has both angles 0 as well, so it shares that pixel and shows
    only in the cloud without the origin point and its farther companion."""
    H, W = 20, 100
    hA, vA, hMin, vMin = PR.geometry(H, W)
    r = KR.rng_for("edge-cloud")
    n = 300
    h, v, rr = r.uniform(-np.pi, np.pi, n), r.uniform(vMin - vA, vMin + (H + 1) * vA, n), r.uniform(2.0, 60.0, n)
    row0, col0 = int(np.round((0 - vMin) / vA)), int(np.round((0 - hMin) / hA))
    in_origin_pixel = (np.round((h - hMin) / hA) == col0) & (np.round((v - vMin) / vA) == row0)
    fill = np.stack([rr * np.cos(h), rr * np.sin(h), rr * np.tan(v)], axis=1)[~in_origin_pixel]
    nan, inf = float("nan"), float("inf")
    special = [
        [-5.0, +0.0, 0.0],                                   # 0: azimuth +pi: column W - 1/2, clamped to W - 1, kept
        [-5.0, -0.0, 0.0],                                   # 1: azimuth -pi: column -1/2, clamped to 0, excluded
        [0.4, 0.3, 0.5 * np.tan(vMin + (H + 3) * vA)],       # 2: above the vertical scope: clamped into row H - 1, kept
        [3.0, -4.0, 5.0 * np.tan(vMin - 4 * vA)],            # 3: below it: row 0, excluded
        [nan, 1.0, 0.0],                                     # 4
        [2.0, 1.0, nan],                                     # 5
        [inf, 1.0, 0.0],                                     # 6: depth +inf in the origin's pixel
    ]
    if with_origin_point:
        special += [[0.0, 0.0, 0.0],                         # 7: depth 0 wins its pixel, which stays empty ...
                    *bin_centre_points(np.array([row0]), np.array([col0]), np.array([1.0]), H, W)]   # 8: ... over this
    pts = np.concatenate([fill[:150], np.array(special), fill[150:]])
    return np.concatenate([pts, r.uniform(0.0, 1.0, (len(pts), 1))], axis=1), 150, H, W, (row0, col0)


def test_projection_edge_points():
    pts, s, H, W, (row0, col0) = edge_cloud()
    ref = check_projection(pts, np.zeros(3), H, W, "edge points")
    idx = ref["index"]
    origin_px = (H - 1 - row0, W - 1 - col0)                            # the outputs are flipped in both axes
    assert idx[H - 1 - row0, 0] == s                                    # (-5, +0, 0): column W - 1
    assert not (idx == s + 1).any()                                     # (-5, -0, 0): column 0
    assert (idx[0] == s + 2).sum() == 1 and (idx == s + 2).sum() == 1   # clamped into row H - 1
    assert not np.isin(idx, [s + 3, s + 4, s + 5, s + 6, s + 7, s + 8]).any()
    assert idx[origin_px] == -1 and ref["depth"][origin_px] == MAXR     # the origin point empties its pixel
    # without the origin point and its companion, x = +inf is alone in that pixel
    pts2, s, H, W, _ = edge_cloud(with_origin_point=False)
    ref2 = check_projection(pts2, np.zeros(3), H, W, "edge points, +inf visible")
    assert ref2["index"][origin_px] == s + 6 and np.isinf(ref2["depth"][origin_px])
    # the first cloud seen from a nonzero origin (the signed zero of the seam points does not survive the shift)
    origin = np.array([1.5, -2.0, 0.5])
    moved = pts.copy()
    moved[:, :3] += origin
    ref3 = check_projection(moved, origin, H, W, "edge points, moved origin")
    assert ref3["index"][origin_px] == -1 and (ref3["index"] >= 0).sum() > 100


def test_projection_argument_forms_agree_with_the_default_form():
    H, W = 20, 100
    pts = lattice_cloud(H, W)
    KR.bin_edge_guard(pts, np.zeros(3), H, W)
    ref = reference(pts, np.zeros(3), H, W)
    rc, base = project(pts, np.zeros(3), H, W)
    assert rc == 0, last_error()
    assert_equal_images(base, ref, "default form")
    wide = np.concatenate([pts, np.full((len(pts), 2), np.nan)], axis=1)
    forms = {
        "stride 3, no intensity": dict(pts=pts[:, :3], has_int=0, intensity=False),
        "stride 4, has_intensity 0": dict(pts=pts, has_int=0, intensity=False),
        "stride 6 with intensity": dict(pts=wide),
        "index null": dict(pts=pts, index=False),
        "intensity null": dict(pts=pts, intensity=False),
        "obfuscation and sky null": dict(pts=pts, scan=False),
    }
    for name, kw in forms.items():
        rc, out = project(kw.pop("pts"), np.zeros(3), H, W, **kw)
        assert rc == 0, (name, last_error())
        assert len(out) >= 3
        assert_equal_images(out, base, name)
    # an empty cloud: every pixel empty, the scan still runs
    rc, out = project(np.zeros((0, 4)), np.zeros(3), H, W)
    assert rc == 0, last_error()
    e = {k: t.cpu().numpy() for k, t in out.items()}
    assert (e["depth"] == MAXR).all() and (e["intensity"] == 0).all() and (e["index"] == -1).all()
    assert not e["obf"].any() and not e["sky"].any()


@pytest.mark.parametrize("name,kw", [
    ("W = 1025", dict(W=1025)),
    ("H = 2", dict(H=2)),
    ("stride = 2", dict(stride=2)),
    ("has_intensity with stride 3", dict(stride=3, has_int=1)),
    ("workspace one byte short", dict(ws_short=1)),
    ("obfuscation without sky", dict(scan=False, obf_only=True)),
    ("N < 0", dict(N=-1)),
])
def test_projection_rejects(name, kw):
    kw = dict(kw)
    H, W = kw.pop("H", 20), kw.pop("W", 100)
    pts = lattice_cloud(20, 100)
    rc, out = project(pts, np.zeros(3), H, W, **kw)
    assert rc != 0 and last_error().startswith("sdp_range_project"), (name, rc, last_error())
    for k, t in out.items():
        assert untouched(t), (name, k)


# ---- sdp_view_finalize -----------------------------------------------------------------------------------------------

def finalize(a, H, W, channels, roll, variant, first_view, goal=True, null_inten=False):
    real, notmask = filled((channels, H, W), torch.float64), filled((channels, H, W), torch.uint8)
    notsky = filled((H, W), torch.uint8)
    g = filled((channels, H, W), torch.float64) if goal else None
    two = channels == 2
    t = {k: dev(v) for k, v in a.items()}
    rc = _lib.lib().sdp_view_finalize(
        KL.ptr(t["depth"]), KL.ptr(t["inten"]) if two and not null_inten else None, KL.ptr(t["obf"]), KL.ptr(t["sky"]),
        KL.ptr(t["goal_depth"]) if goal else None, KL.ptr(t["goal_inten"]) if goal and two else None, H, W, channels,
        roll, variant, first_view, KL.ptr(real), KL.ptr(notmask), KL.ptr(notsky), KL.ptr(g), _lib.stream())
    torch.cuda.synchronize()
    return rc, real, notmask, notsky, g


def assert_depth_code(got, want, what):
    assert not np.isnan(got).any(), what
    np.testing.assert_allclose(got, want, rtol=1e-13, atol=0, err_msg=what)
    clipped = (want == 0.0) | (want == 1.0)
    assert np.array_equal(bits(got[clipped]), bits(want[clipped])), what


@pytest.mark.parametrize("variant", [0, 1, 2, 3])
@pytest.mark.parametrize("H,W", [(5, 7), (8, 100), (64, 256)])
def test_view_finalize_equals_the_reference(H, W, variant):
    a = KR.view_finalize_inputs(f"{H}x{W}", H, W)
    assert (H * W) % 256 != 0 or (H, W) == (64, 256)
    for channels in (1, 2):
        for first_view in (0, 1):
            for roll in (-1, 0, 1, W - 1):
                for goal in ((True, False) if variant == 3 else (True,)):
                    what = f"{H}x{W} variant {variant} C {channels} first {first_view} roll {roll} goal {goal}"
                    rc, real, notmask, notsky, g = finalize(a, H, W, channels, roll, variant, first_view, goal)
                    assert rc == 0, (what, last_error())
                    w_real, w_notmask, w_notsky, w_goal = KR.view_finalize_ref(
                        a["depth"], a["inten"] if channels == 2 else None, a["obf"], a["sky"],
                        a["goal_depth"] if goal else None, a["goal_inten"] if goal and channels == 2 else None,
                        channels, roll, variant, first_view)
                    assert np.array_equal(notmask.cpu().numpy(), w_notmask.astype(np.uint8)), what
                    assert np.array_equal(notsky.cpu().numpy(), w_notsky.astype(np.uint8)), what
                    real = real.cpu().numpy()
                    assert_depth_code(real[0], w_real[0], what)
                    if channels == 2 and variant == 3:
                        assert np.array_equal(bits(real[1]), bits(real[0])), what
                    elif channels == 2:
                        assert np.array_equal(bits(real[1]), bits(w_real[1])), what
                    if goal:
                        g = g.cpu().numpy()
                        assert_depth_code(g[0], w_goal[0], what)
                        if channels == 2:
                            assert np.array_equal(bits(g[1]), bits(w_goal[1])), what


@pytest.mark.parametrize("name,kw", [
    ("roll = W", dict(roll=100)),
    ("channels = 3", dict(channels=3)),
    ("variant = 4", dict(variant=4)),
    ("variant 0 with a null goal", dict(goal=False)),
    ("channels = 2 with null intensity", dict(null_inten=True)),
])
def test_view_finalize_rejects(name, kw):
    H, W = 8, 100
    a = KR.view_finalize_inputs("reject", H, W)
    args = dict(channels=2, roll=1, variant=0, first_view=0)
    args.update(kw)
    rc, *outs = finalize(a, H, W, **args)
    assert rc != 0 and last_error().startswith("sdp_view_finalize"), (name, last_error())
    for t in outs:
        assert t is None or untouched(t), name


# ---- sdp_view_gather -------------------------------------------------------------------------------------------------

def index_image(H, W, valid, n_pts):
    r = KR.rng_for(f"gather-{H}x{W}-{valid}")
    ind = np.where(r.random((H, W)) < 0.5, -1, -2).astype(np.int64)
    sel = r.random((H, W)) < valid
    ind[sel] = r.integers(0, n_pts, int(sel.sum()))
    return ind


@pytest.mark.parametrize("valid", [0.4, 0.0])
@pytest.mark.parametrize("H,W", [(3, 5), (7, 150), (64, 1024)])
def test_view_gather_equals_the_reference(H, W, valid):
    n_pts = 5000
    pts = KR.rng_for("gather-points").standard_normal((n_pts, 4)).astype(np.float32) * 30
    ind = index_image(H, W, valid, n_pts)
    assert (ind == -1).any() and (ind == -2).any() and (valid == 0) == (not (ind >= 0).any())
    p, i = dev(pts), dev(ind)
    for blank in (0, W // 4, W, W + 3):
        out, cnt = filled((H * W, 4), torch.float64), filled((1,), torch.int32)
        rc = _lib.lib().sdp_view_gather(KL.ptr(i), H, W, blank, KL.ptr(p), KL.ptr(out), KL.ptr(cnt), _lib.stream())
        torch.cuda.synchronize()
        assert rc == 0, last_error()
        w = ind.copy()
        w[:, :blank] = -2
        want = pts[w[w >= 0]].astype(np.float64)
        n = int(cnt.item())
        assert n == len(want), (blank, n, len(want))
        assert (n == 0) == (valid == 0 or blank >= W)
        assert np.array_equal(bits(out[:n].cpu().numpy()), bits(want)), blank
        assert untouched(out[n:]), blank


# ---- sdp_view_transform ----------------------------------------------------------------------------------------------

def pose(r):
    """A KITTI-like vehicle pose: yaw anywhere, a few degrees of pitch and roll, a translation of order 100."""
    yaw, pitch, roll = r.uniform(-np.pi, np.pi), r.uniform(-0.05, 0.05), r.uniform(-0.05, 0.05)
    cz, sz, cy, sy, cx, sx = np.cos(yaw), np.sin(yaw), np.cos(pitch), np.sin(pitch), np.cos(roll), np.sin(roll)
    R = (np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]]) @ np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
         @ np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]]))
    M = np.eye(4)
    M[:3, :3] = R
    M[:3, 3] = r.choice([-1.0, 1.0], 3) * r.uniform(100, 300, 3) * (1.0, 1.0, 0.05)
    return M


def apply_in_kernel_order(M, v):
    """M @ v per point, the four products summed left to right: ((a0*v0 + a1*v1) + a2*v2) + a3*v3 (float64, unfused)."""
    return np.stack([((M[i, 0] * v[0] + M[i, 1] * v[1]) + M[i, 2] * v[2]) + M[i, 3] * v[3] for i in range(4)])


@pytest.mark.parametrize("n", [1, 255, 257, 70001])
def test_view_transform_equals_the_reference(n):
    r = KR.rng_for(f"transform-{n}")
    pts = (r.standard_normal((n, 4)) * (30, 30, 3, 0.3)).astype(np.float32)
    m1, m2 = pose(r), np.linalg.inv(pose(r))
    assert np.abs(m1[:3, 3]).max() > 50 and np.abs(m2[:3, 3]).max() > 50
    v = np.concatenate([pts[:, :3].T.astype(np.float64), np.ones((1, n))])
    wants = {"both": apply_in_kernel_order(m2, apply_in_kernel_order(m1, v)), "m1 only": apply_in_kernel_order(m1, v),
             "neither": v}
    p = dev(pts)
    for name, (a, b) in {"both": (m1, m2), "m1 only": (m1, None), "neither": (None, None)}.items():
        out = filled((n, 4), torch.float64)
        a = None if a is None else np.ascontiguousarray(a)
        b = None if b is None else np.ascontiguousarray(b)
        rc = _lib.lib().sdp_view_transform(KL.ptr(p), n, None if a is None else a.ctypes.data,
                                           None if b is None else b.ctypes.data, KL.ptr(out), _lib.stream())
        torch.cuda.synchronize()
        assert rc == 0, last_error()
        got = out.cpu().numpy()
        assert np.array_equal(bits(got[:, :3]), bits(wants[name][:3].T)), (name, n)
        assert np.array_equal(bits(got[:, 3]), bits(pts[:, 3].astype(np.float64))), (name, n)


def test_view_transform_rejects_m2_alone_and_skips_an_empty_scan():
    pts = dev(np.ones((4, 4), np.float32))
    out = filled((4, 4), torch.float64)
    m = np.ascontiguousarray(np.eye(4))
    rc = _lib.lib().sdp_view_transform(KL.ptr(pts), 4, None, m.ctypes.data, KL.ptr(out), _lib.stream())
    assert rc != 0 and last_error().startswith("sdp_view_transform")
    assert _lib.lib().sdp_view_transform(None, 0, m.ctypes.data, m.ctypes.data, None, _lib.stream()) == 0
    assert _lib.lib().sdp_view_transform(KL.ptr(pts), 0, m.ctypes.data, None, KL.ptr(out), _lib.stream()) == 0
    torch.cuda.synchronize()
    assert untouched(out)
