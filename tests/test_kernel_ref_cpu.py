"""The per-kernel references and gates themselves (CPU only; tests/kernel_ref.py).

* every lattice case of the GPU modules' tables keeps its largest partial sum below 2^24 lattice units, and a float32
  torch-CPU evaluation of it EQUALS the float64 reference (the exactness the GPU equality gate rests on);
* a float32 torch-CPU evaluation of every real-valued case passes the fp32 gate;
* for each conv direction, a reference with ONE misplaced term -- a border pixel read one lattice unit off, the wrap
  column of one row taken as zero, one channel pair swapped in one tile -- fails the gate of every mode, on the
  smallest case of each class: the gates see a single-term error;
* the same for the head and tail kernels (begin / end conv, their backward kernels, the DSM loss): lattice cases exact
  in float32 and below 2^24 units, real cases within the fp32 gate, the written-out references equal to autograd and to
  the oracle's own functions, and single-term mutants -- zero padding replaced by the clamped border value in one border
  row or column, the coordinate channels swapped, one tap one pixel off, image 1 divided by image 0's sigma, the
  per-image mask count instead of the batch's -- failing the gate of every mode;
* the data front end (tests/test_gpu_kernels_frontend.py): ``view_finalize_ref`` bit-equal to the oracle's own dataset
  tails, the bin-edge guard, the projection's workspace size against its layout, and the GPU module's inputs telling
  single-term mutants of the references apart (a non-strict compare, a stale column sum, a dropped chain term or a
  misread batch row in the sky scan; the higher index of a tie, a single grid-stride pass; a rolled intensity test, a
  2- or 4-row sky shift, an unrolled sky).
"""
import dataclasses

import numpy as np
import pytest
import torch

import kernel_ref as KR
import test_gpu_kernels_aux as TA
import test_gpu_kernels_conv as TC
import test_gpu_kernels_frontend as TF
import test_gpu_kernels_head as TH
from kernel_ref import Head

CASES = [c for c, _ in TC.CASES]
SMALL = [c for c in CASES if c.name.endswith("-a")]
# the smallest case of each (class, direction), lattice and real: the first of its table
FIRST = list({(c.name.split("-")[0], c.kind, c.real): c for c in reversed(SMALL)}.values())


def test_every_weight_gradient_kernel_class_has_interior_and_multi_tile_cases():
    """The weight-gradient kernels load interior tiles (no border in the 3x3 patch) through a path of their own and
    walk several tiles per workgroup when there are more tiles than splits: each class needs a case of either."""
    seen = {}
    for c, modes in TC.WGRAD:
        for m in modes:
            name, interior, multi = TC.wgrad_kernel(c, m)
            s = seen.setdefault(name, [0, 0, 0, 0])
            s[0] += 1
            s[1] += interior and not c.real
            s[2] += multi and not c.real
            s[3] += interior and multi
    assert set(seen) == {"<64,3,OCC1>", "<32,3,OCC1>", "<64,1,OCC1>", "<64,1,OCC3>", "<32,3,OCC3>", "<64,3,OCC2>",
                         "h16<32,3>", "h16<64,1>"}, sorted(seen)
    for name, (n, interior, multi, both) in seen.items():
        assert interior >= 1 and multi >= 1 and both >= 1, (name, n, interior, multi, both)


def _f32(o):
    return {k: v.to(torch.float32) for k, v in o.items()}


def test_lattice_bound_holds_for_every_case_of_the_gpu_tables():
    for c in CASES:
        if not c.real:
            assert c.lattice_bound() < 2 ** 24, c.name
    for shape in TA.LATTICE_SHAPES:
        assert TA.lattice_bound(*shape) < 2 ** 24, shape


@pytest.mark.parametrize("c", SMALL, ids=lambda c: c.name)
def test_float32_cpu_evaluation_passes_the_gate(c):
    """Lattice: float32 == float64 (equality).  Real: |float32 - float64| within the fp32 gate."""
    o = KR.make_operands(c)
    ref = KR.reference(c, o, "fp32")
    gate = KR.gate(c, o, "fp32", ref)
    got = KR.REFS[c.kind](c, _f32(o))
    for k in ref:
        g = got[k].to(torch.float64)
        if c.real or gate[k].max() > 0:
            assert ((g - ref[k]).abs() <= gate[k]).all(), (c.name, k, float((g - ref[k]).abs().max()))
        else:
            assert torch.equal(g, ref[k]), (c.name, k)


@pytest.mark.parametrize("mutant", sorted(KR.MUTANTS))
@pytest.mark.parametrize("c", FIRST, ids=lambda c: c.name)
def test_a_single_misplaced_term_fails_every_gate(c, mutant):
    o = KR.make_operands(c)
    for mode in ("fp32x3", "bf16") if c.kind != "fwd" else ("fp32", "fp32x3", "bf16"):
        ref = KR.reference(c, o, mode)
        gate = KR.gate(c, o, mode, ref)
        bad = KR.REFS[c.kind](c, o, bf16=(mode == "bf16" and c.real), mutate=KR.MUTANTS[mutant](c))
        key = "dw" if c.kind == "wgrad" else "out"
        over = (bad[key] - ref[key]).abs() > gate[key]
        assert over.any(), f"{c.name} {mode}: the {mutant} mutant passes the gate"


def test_statistics_gate_sees_one_wrong_pixel():
    c = next(c for c in SMALL if c.stats and not c.real)
    o = KR.make_operands(c)
    y = KR.reference(c, o)["out"]
    gm, gv = KR.stats_gate(y)
    y2 = y.clone()
    y2[0, 0, 0, 0] += 0.25
    assert ((y2.mean(dim=(2, 3)) - y.mean(dim=(2, 3))).abs() > gm).any()


# ------------------------------------------------------------------------------------------------ the small ops
F32 = torch.float32


def test_float32_cpu_evaluation_of_the_small_ops_passes_their_gates():
    r = KR.rng_for("small-ops")
    shape = (3, 36, 6, 10)
    x, g, lo0, res = (KR.normal(r, s) for s in (shape, shape, (3, 36, 3, 5), shape))
    y = KR.R.elu(KR.normal(r, shape)).to(F32).to(torch.float64)
    assert ((KR.R.mean_pool2(x.to(F32)).double() - KR.R.mean_pool2(x)).abs() <= KR.avgpool2_gate(x)).all()
    ref = KR.upsample_backward(g) + lo0
    got = (KR.upsample_backward(g.to(F32)) + lo0.to(F32)).double()
    assert ((got - ref).abs() <= KR.upsample_backward_gate(g, lo0, ref)).all()
    ref = g * KR.elu_grad(y, 2) + res
    got = (g.to(F32) * KR.elu_grad(y.to(F32), 2) + res.to(F32)).double()
    assert ((got - ref).abs() <= KR.elu_post_gate(g, y, res, ref)).all()
    assert (((g.to(F32) + res.to(F32)).double() - (g + res)).abs() <= KR.add_gate(g, res)).all()
    # a single misplaced element: one output takes its neighbour's value
    bad = ref.clone()
    bad[0, 0, 0, 0] = ref[0, 0, 0, 1]
    assert ((bad - ref).abs() > KR.elu_post_gate(g, y, res, ref)).any()


def test_lattice_small_ops_are_exact_in_float32_and_the_index_helpers_agree_with_autograd():
    r = KR.rng_for("small-lattice")
    shape = (2, 8, 12, 16)
    x, dp = KR.lattice(r, shape, -4, 4, 4), KR.lattice(r, shape, -4, 4, 4)
    assert torch.equal(KR.maxpool5(x.to(F32)).double(), KR.maxpool5(x))
    assert torch.equal(KR.R.mean_pool2(x.to(F32)).double(), KR.R.mean_pool2(x))
    assert torch.equal(KR.unpool(dp.to(F32)).double(), KR.unpool(dp))
    # torch's own argmax, as window positions 5 r + s, through the scatter helper == autograd (ties included)
    _, ti = torch.nn.functional.max_pool2d(x, 5, 1, 2, return_indices=True)
    H, W = shape[2:]
    i = (ti // W - torch.arange(H).view(1, 1, H, 1) + 2) * 5 + (ti % W - torch.arange(W).view(1, 1, 1, W) + 2)
    assert torch.equal(KR.window_values(x).gather(-1, i.unsqueeze(-1)).squeeze(-1), KR.maxpool5(x))
    assert torch.equal(KR.pick_by_idx(x, i), KR.maxpool5(x))
    assert torch.equal(KR.scatter_by_idx(i, dp), KR.maxpool5_backward(x, dp))
    y = TA.tie_free(2, 8, 12, 16, r)
    w = KR.window_values(y)
    assert (w.isfinite().sum(-1) == (w.unsqueeze(-1) == w.unsqueeze(-2)).logical_and(w.isfinite().unsqueeze(-1)).sum((-1, -2))).all()


def test_inpp_scale_shift_restates_instance_norm_pp():
    r = KR.rng_for("inpp-ss")
    x = KR.normal(r, (2, 64, 8, 16))
    x[:, 5] = 3.0
    alpha, gamma, beta = TA._norm_params(64, r)
    scale, shift = KR.inpp_scale_shift(x, alpha, gamma, beta)
    want = KR.R.instance_norm_pp(x, KR.inpp_params(alpha, gamma, beta), "n")
    assert torch.allclose(x * scale[:, :, None, None] + shift[:, :, None, None], want, rtol=0, atol=1e-11)
    mean, var = KR.combine_stats(TA._groups(x, 64), 64)
    gm, gv = KR.stats_gate(x)
    assert ((mean - x.mean(dim=(2, 3))).abs() <= gm).all() and ((var - x.var(dim=(2, 3), unbiased=False)).abs() <= gv).all()


# ------------------------------------------------------------------------------------------------ head and tail kernels
R = KR.R
F64 = torch.float64
HEAD = TH.BEGIN + [TH.BEGIN_Q] + [c for c, _ in TH.END] + TH.BACKWARD
_hid = lambda c: c.name + ("-h16" if c.h16 else "")


def _h32(o):
    return {k: (v.to(F32) if v.dtype == F64 else v) for k, v in o.items()}


def test_head_tables_hold_the_cases_the_kernels_need():
    names = {_hid(c) for c in HEAD}
    assert len(names) == len(HEAD)
    for op in KR.HEAD_OPS:
        mine = [c for c in HEAD if c.op == op]
        assert any(c.real for c in mine) and any(not c.real for c in mine) and any(c.B > 1 for c in mine), op
    assert {f for _, forms in TH.END for f in forms} == set(TH.FORMS)
    assert {c.h16 for c in TH.BACKWARD} == {False, True}
    for c in HEAD:      # different sigmas per image, out of order
        assert len(set(c.labels())) == c.B and (c.B < 2 or c.labels() != sorted(c.labels()))


@pytest.mark.parametrize("c", HEAD, ids=_hid)
def test_head_float32_cpu_evaluation_passes_the_gate(c):
    """Lattice: the bound holds and float32 == float64 (begin_wgrad's coordinate channels: the fp32 gate).  Real:
    |float32 - float64| within the fp32 gate."""
    if not c.real:
        assert c.lattice_bound() < 2 ** 24, c.name
    o = KR.head_operands(c)
    ref = KR.head_reference(c, o)
    gate = KR.head_gate(dataclasses.replace(c, h16=False), o, "fp32", ref)
    got = KR.head_reference(c, _h32(o))
    for k in ref:
        g = got[k].to(F64)
        exact = gate[k] == 0
        assert c.real or exact.any()
        assert torch.equal(g[exact], ref[k][exact]), (c.name, k)
        assert ((g - ref[k]).abs() <= gate[k]).all(), (c.name, k, float((g - ref[k]).abs().max()))
    if not c.real and c.op == "begin_wgrad":
        assert (gate["dw"][:, :2] == 0).all() and (gate["db"] == 0).all() and (gate["dw"][:, 2:] > 0).all()
    if not c.real and c.h16:      # every operand the bf16 tape holds is bf16-representable
        for k in ("x", "dy"):
            if k in o:
                assert torch.equal(KR.bf16_round(o[k]), o[k])


def test_head_references_restate_the_oracle_and_autograd():
    close = lambda a, b: torch.allclose(a, b, rtol=0, atol=1e-11 * float(b.abs().max()))
    # begin conv and its weight gradient
    c = Head("restate-begin", "begin", 2, 5, 128, real=True)
    o = KR.head_operands(c)
    w, b = o["w"].clone().requires_grad_(True), o["bias"].clone().requires_grad_(True)
    y = R.conv2d(R.input_prep(o["x"]), w, b, circular=False)
    assert close(KR.head_reference(c, o)["out"], y.detach())
    cw = Head("restate-begin", "begin_wgrad", 2, 8, 64, real=True)
    ow = KR.head_operands(cw)
    dw, db = torch.autograd.grad(R.conv2d(R.input_prep(ow["x"]), w, b, circular=False), [w, b], ow["dy"])
    got = KR.head_reference(cw, ow)
    assert close(got["dw"], dw) and close(got["db"], db)
    # end conv: conv_forward on the affine + ELU case, / sigma; its backward: autograd of exactly that
    c = Head("restate-end", "end_bwd", 3, 16, 64, real=True)
    o = KR.head_operands(c)
    o["bias"] = torch.tensor([0.25, -0.5], dtype=F64)
    sig = o["sigmas"][o["labels"]][:, None, None, None]
    fwd = KR.head_reference(dataclasses.replace(c, op="end"), o)["out"]
    assert close(fwd, KR.conv_forward(c.end_case(), o)["out"] / sig)
    h = (o["x"] * o["scale"][:, :, None, None] + o["shift"][:, :, None, None]).requires_grad_(True)
    w, b = o["w"].clone().requires_grad_(True), o["bias"].clone().requires_grad_(True)
    out = R.conv2d(R.elu(h), w, b, circular=False) / sig
    assert close(fwd, out.detach())
    g, dw, db = torch.autograd.grad(out, [h, w, b], o["dscore"])
    got = KR.head_reference(c, o)
    assert close(got["g"], g) and close(got["dw"], dw) and close(got["db"], db)
    assert (h < 0).any() and (h > 0).any()          # both ELU branches
    # DSM loss
    o = KR.dsm_operands("restate-dsm", 3, 1600, zero_image=1)
    for p in (0, 2):
        ref = KR.dsm_reference(o, p)
        want = R.dsm_loss(o["score"], o["sigma"][:, None], o["noise"], o["mask"], p)
        assert abs(ref["loss"] - want) <= 1e-13 * want and ref["loss_per"][1] == 0 and (ref["dscore"][1] == 0).all()


def _mutant_rows():
    bwd = [("fp32", False), ("fp32", True)]
    pads = ("pad_row", "pad_col", "tap")
    rows = []
    for real in (False, True):
        t = dict(real=real)
        rows += [
            (Head("begin-a", "begin", *TH.BEGIN_SHAPES["a"], **t), TH.FORMS, pads + ("coord_swap",), ("out",)),
            (Head("end-mfma-a", "end", *TH.END_MFMA["a"], **t), TH.FORMS[1:], pads, ("out",)),
            (Head("end-direct-a", "end", *TH.END_DIRECT["a"], **t), TH.FORMS[:1], pads, ("out",)),
            (Head("end-mfma-b", "end", *TH.END_MFMA["b"], **t), TH.FORMS[1:], ("sigma",), ("out",)),
            (Head("begin_wgrad-a", "begin_wgrad", *TH.BWG["a"], **t), bwd, pads + ("coord_swap",), ("dw",)),
            (Head("end_bwd-a", "end_bwd", *TH.EBW["a"], **t), bwd, pads, ("g", "dw")),
            (Head("end_bwd-b", "end_bwd", *TH.EBW["b"], **t), bwd, ("sigma",), ("g", "dw", "db")),
        ]
    return [pytest.param(c, forms, m, keys, id=f"{c.name}{'-real' if c.real else ''}-{m}") for c, forms, ms, keys in rows for m in ms]


@pytest.mark.parametrize("c,forms,mutant,keys", _mutant_rows())
def test_a_single_wrong_term_fails_every_gate_of_the_head_kernels(c, forms, mutant, keys):
    for mode, h16 in forms:
        cc = dataclasses.replace(c, h16=h16)
        o = KR.head_operands(cc)
        ref = KR.head_finish(cc, KR.head_reference(cc, o, mode))
        gate = KR.head_gate(cc, o, mode, ref)
        bad = KR.head_finish(cc, KR.head_reference(cc, o, mode, mutate=KR.HEAD_MUTANTS[mutant](cc)))
        for k in keys:
            assert ((bad[k] - ref[k]).abs() > gate[k]).any(), f"{c.name} {mode} h16={h16} {k}: the {mutant} mutant passes the gate"


def dsm_float32(o, power):
    """The DSM loss in float32 elementwise arithmetic with the sums in double (the order train_aux.hip documents)."""
    s, z, m, sg = (o[k].to(F32) for k in ("score", "noise", "mask", "sigma"))
    B, n = s.shape
    inv2 = 1.0 / (sg * sg)
    r = m * (s - (-inv2[:, None] * z))
    count = m.double().sum()
    scale = n / count * sg.double() ** power / B
    per = 0.5 * (r.double() ** 2).sum(dim=-1).to(F32).double() * n / count * sg.double() ** power
    return {"dscore": (scale[:, None] * (m * r).double()).to(F32).double(), "loss_per": per.to(F32).double(),
            "loss": per.mean().to(F32).double()}


def test_dsm_loss_reference_gates_and_mutant():
    for B, n_img, power in ((1, 1600, 2), (3, 2 * 7 * 1171, 0), (3, 1600, 2)):
        o = KR.dsm_operands(f"dsm-cpu-{B}-{n_img}", B, n_img, zero_image=1 if B == 3 else None)
        ref, gate, got = KR.dsm_reference(o, power), KR.dsm_gate(o, power), dsm_float32(o, power)
        assert ((got["dscore"] - ref["dscore"]).abs() <= gate).all()
        assert abs(got["loss"] - ref["loss"]) <= 2.0 ** -22 * ref["loss"]
        assert ((got["loss_per"] - ref["loss_per"]).abs() <= 2.0 ** -22 * ref["loss_per"]).all()
    assert all(float(torch.tensor(v, dtype=F32) ** 2) == v * v for v in KR.DSM_SIGMAS)      # exact float32 squares
    # the lattice case: exact
    assert KR.dsm_lattice_bound(1600) < 2 ** 24
    o = KR.dsm_operands("dsm-lattice", 2, 1600, lattice_case=True)
    ref, got = KR.dsm_reference(o, 2), dsm_float32(o, 2)
    assert torch.equal(got["dscore"], ref["dscore"]) and torch.equal(got["loss_per"], ref["loss_per"].to(F32).double())
    assert got["loss"] == ref["loss"].to(F32).double()
    # the mutant: each image divided by its own mask count instead of the batch's
    o = KR.dsm_operands("dsm-mutant", 3, 1600)
    ref, gate, bad = KR.dsm_reference(o, 2), KR.dsm_gate(o, 2), KR.dsm_reference(o, 2, per_image_count=True)
    assert ((bad["dscore"] - ref["dscore"]).abs() > gate).any()
    assert abs(bad["loss"] - ref["loss"]) > 2.0 ** -22 * ref["loss"]
    assert ((bad["loss_per"] - ref["loss_per"]).abs() > 2.0 ** -22 * ref["loss_per"]).any()


# ---- the view post-processing reference (KR.view_finalize_ref) against the oracle's own dataset tails -------------

def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def test_view_finalize_inputs_reach_every_branch():
    for H, W in ((5, 7), (8, 100), (64, 256)):
        a = KR.view_finalize_inputs(f"{H}x{W}", H, W)
        assert a["sky"][:3].any() and a["sky"][-3:].any() and 0.05 < a["sky"].mean() < 0.25    # 5x7: 6 forced bits
        assert (a["depth"] == KR.VIEW_MAX_RANGE).any() and (a["depth"] > KR.VIEW_MAX_RANGE).any()
        assert ((a["depth"] > 63) & (a["depth"] < KR.VIEW_MAX_RANGE)).any()        # the upper clip of the depth code
        for v in (1.0, 1.5, 0.0, 1.0 - 2.0 ** -24):
            assert (a["inten"] == v).any(), v
        # the "unrolled intensity against rolled mask" rule decides pixels under a roll by one column
        hit = (a["inten"] >= 1) & ~((np.roll(a["inten"], 1, axis=1) >= 1))
        assert hit.any()


@pytest.mark.parametrize("variant", [0, 1, 2])
@pytest.mark.parametrize("roll", [None, 0, 1, 99])
@pytest.mark.parametrize("first_view", [0, 1])
def test_view_finalize_ref_equals_the_kitti_oracle_tail(variant, roll, first_view):
    from oracle import kitti_ref
    H, W = 8, 100
    a = KR.view_finalize_inputs("pin", H, W)
    want = kitti_ref._post(a["depth"], a["inten"], a["obf"].astype(bool), a["sky"].astype(bool), a["goal_depth"],
                           a["goal_inten"], H, W, roll, variant, 0 if first_view else 1)
    got = KR.view_finalize_ref(a["depth"], a["inten"], a["obf"], a["sky"], a["goal_depth"], a["goal_inten"], 2,
                               -1 if roll is None else roll, variant, first_view)
    real, notmask, notsky, goal = got
    assert real.shape == want[0].shape == (2, H, W) and np.array_equal(_bits(real), _bits(want[0]))
    assert notmask.shape == (2, H, W) and np.array_equal(notmask, want[1])
    assert np.array_equal(notsky[None], want[2])
    assert np.array_equal(_bits(goal), _bits(want[3]))
    assert not notsky.all() and not notmask.all() and notmask.any()


@pytest.mark.parametrize("roll", [None, 0, 1, 99])
def test_view_finalize_ref_equals_the_completion_oracle_tail(roll, tmp_path, monkeypatch):
    """oracle/completion_ref.item with its loading, subsampling, origin and projection replaced by the seeded arrays:
    what remains is its post-processing tail, unchanged."""
    from oracle import completion_ref as CR
    H, W = 8, 100
    a = KR.view_finalize_inputs("pin3", H, W)
    np.save(tmp_path / "scan.npy", np.zeros((4, 3)))
    np.save(tmp_path / "final.npy", np.zeros((2, 4)))
    monkeypatch.setattr(CR, "grid_sub_sampling_ref", lambda p, dl=0.05: p)
    monkeypatch.setattr(CR, "view_origin", lambda scan, nib, mods: np.zeros(3))
    monkeypatch.setattr(CR, "point_cloud_to_range_image", lambda *_: (
        a["depth"].copy(), a["inten"].copy(), a["obf"].astype(bool), 0, a["sky"].astype(bool), np.zeros((H, W))))
    want = CR.item(str(tmp_path / "scan.npy"), str(tmp_path / "final.npy"), 0, np.zeros((1, 3)), H, W, roll)
    real, notmask, notsky, goal = KR.view_finalize_ref(a["depth"], a["inten"], a["obf"], a["sky"], None, None, 2,
                                                       -1 if roll is None else roll, 3, 0)
    assert goal is None
    assert real.shape == want[0].shape and np.array_equal(_bits(real), _bits(want[0]))
    assert np.array_equal(_bits(real[0]), _bits(real[1]))
    assert notmask.shape == want[1].shape and np.array_equal(notmask, want[1]) and not notmask[1].any()
    assert np.array_equal(notsky[None], want[2])


def test_view_finalize_ref_one_channel_is_the_depth_path_alone():
    """channels == 1 is return_remission off: no intensity test, one channel (8Batch:268-291 skipped)."""
    H, W = 8, 100
    a = KR.view_finalize_inputs("pin1", H, W)
    for variant in range(4):
        r1 = KR.view_finalize_ref(a["depth"], None, a["obf"], a["sky"], a["goal_depth"], None, 1, 3, variant, 0)
        r2 = KR.view_finalize_ref(a["depth"], np.zeros((H, W)), a["obf"], a["sky"], a["goal_depth"], np.zeros((H, W)),
                                  2, 3, variant, 0)
        assert r1[0].shape == r1[1].shape == r1[3].shape == (1, H, W)
        assert np.array_equal(_bits(r1[0][0]), _bits(r2[0][0])) and np.array_equal(r1[1][0], r2[1][0])
        assert np.array_equal(r1[2], r2[2]) and np.array_equal(_bits(r1[3][0]), _bits(r2[3][0]))


def test_bin_edge_guard_passes_the_goldens_and_sees_an_edge_point():
    from oracle import golden_inputs as GI
    from oracle import projection_ref as PR
    for tag, (n, origin) in GI.PROJECTION_CASES.items():
        assert KR.bin_edge_guard(GI.projection_cloud(tag, n), origin, 64, 1024) > KR.BIN_EDGE_EPS
    hA, vA, hMin, vMin = PR.geometry(20, 100)
    for dc, dr in ((0.5 + 1e-11, 0.0), (0.0, 0.5 - 1e-11)):          # 1e-11 bins off a column / a row edge
        h, v = hMin + (40 + dc) * hA, vMin + (7 + dr) * vA
        p = np.array([[10 * np.cos(h), 10 * np.sin(h), 10 * np.tan(v)]])
        with pytest.raises(AssertionError):
            KR.bin_edge_guard(p, np.zeros(3), 20, 100)
    # the clamp absorbs the last half bin: a point on the seam (column W - 1/2) decides nothing
    assert KR.bin_edge_guard(np.array([[-5.0, 0.0, 0.0], [-5.0, -0.0, 0.0]]), np.zeros(3), 20, 100) > 0.1


def test_projection_workspace_holds_its_layout_at_odd_pixel_counts():
    """sdp_range_project lays out 8 n bytes of depth bits, 4 n of winner indices padded to 8-byte alignment, and 8 n of
    planar ranges: at an odd n = H * W the padding is 4 bytes that n * 20 does not have."""
    import ctypes as C

    from sdp import _lib
    for H, W in ((5, 7), (3, 1), (64, 1023), (64, 1024), (20, 100)):
        n, got = H * W, _lib.SZ()
        _lib.check(_lib.lib().sdp_range_project_workspace_size(H, W, C.byref(got)), "ws")
        assert got.value >= 8 * n + 8 * ((4 * n + 7) // 8) + 8 * n, (H, W, got.value)


# ---- the front-end inputs tell single-term mutants of the references apart (tests/test_gpu_kernels_frontend.py) ----

def _sky_scan_mutant(xy, kind):
    """oracle.projection_ref.sky_scan with ONE change: 'ge' compares x >= md + 5; 'stale' takes the left neighbour's
    count from the previous row (a 3-column sum read before the row buffer is rewritten); 'nochain' drops the
    `and sky[row - 1]` of the still-sky chain; 'batch' reads row 2 + 16 + 1, the first of the second 16-row batch, as 0."""
    H, W = xy.shape
    md = np.zeros(W) + TF.MAXR
    prev, e_prev = np.ones(W, bool), np.zeros(W + 2, int)
    obf = np.zeros((H, W), bool)
    over = (lambda x, m: x >= m + 5) if kind == "ge" else (lambda x, m: x > m + 5)
    for row in range(2, H - 1):
        obf[row] = over(xy[row], md)
        nxt = np.zeros(W) if kind == "batch" and row + 1 == 19 else xy[row + 1]
        e = np.concatenate(([0], (xy[row] != md).astype(int) + (xy[row - 1] != md) + (nxt != md), [0]))
        left = e_prev[:-2] if kind == "stale" else e[:-2]
        cur = (e[1:-1] + left + e[2:] <= 1) & (True if kind == "nochain" else prev)
        md = np.where(cur, md, np.minimum(xy[row], md))
        prev, e_prev = cur, e
    obf[-1] = over(xy[-1], md)
    return obf


@pytest.mark.parametrize("H,W", [s for s in TF.SKY_SHAPES if s[0] >= 20])
def test_the_sky_scan_images_tell_single_term_mutants_apart(H, W):
    xy = TF.sky_image(H, W)
    want = TF.PR.sky_scan(xy)[0]
    assert np.array_equal(_sky_scan_mutant(xy, None), want)
    for kind in ("ge", "stale", "nochain") + (("batch",) if H > 20 else ()):      # H = 20: row 19 is the last row
        assert (_sky_scan_mutant(xy, kind) != want).any(), kind


def test_the_lattice_clouds_tell_the_tie_rule_and_the_z_buffer_apart():
    for H, W in ((20, 100), (16, 128)):
        pts = TF.lattice_cloud(H, W)
        ref = TF.reference(pts, np.zeros(3), H, W)
        # the highest index of a tie instead of the lowest: the oracle on the reversed cloud, indices mapped back
        rev = TF.reference(pts[::-1], np.zeros(3), H, W)["index"]
        rev = np.where(rev >= 0, len(pts) - 1 - rev, rev)
        assert int((rev != ref["index"]).sum()) == TF.tie_pixels(pts, ref) >= 10
        # the farther point of a pixel instead of the nearer: depth negated in the sort is not expressible through the
        # oracle, but dropping the winners must bring the losers up -- the cloud has pixels with more than one point
        win = ref["index"][ref["index"] >= 0]
        rest = TF.reference(np.delete(pts, win, axis=0), np.zeros(3), H, W)
        assert (rest["index"] >= 0).sum() >= 100


def test_the_two_pass_cloud_needs_its_second_pass():
    pts, H, W, cross = TF.two_pass_cloud()
    assert len(pts) > TF.GRID_CAP and cross.sum() == 600
    ref = TF.reference(pts, np.zeros(3), H, W)
    first_only = TF.reference(pts[:TF.GRID_CAP], np.zeros(3), H, W)     # a loop that stops after one pass
    assert (first_only["index"] != ref["index"]).sum() >= 150
    rev = TF.reference(pts[::-1], np.zeros(3), H, W)["index"]            # the higher index of each tie
    rev = np.where(rev >= 0, len(pts) - 1 - rev, rev)
    assert (rev != ref["index"]).sum() == 600 and (rev[rev != ref["index"]] >= TF.GRID_CAP).sum() >= 300


def test_the_finalize_inputs_tell_single_term_mutants_apart():
    for H, W in ((5, 7), (8, 100), (64, 256)):
        a = KR.view_finalize_inputs(f"{H}x{W}", H, W)
        args = (a["obf"], a["sky"], a["goal_depth"], a["goal_inten"], 2)
        real, notmask, notsky, _ = KR.view_finalize_ref(a["depth"], a["inten"], *args, 1, 0, 0)
        # the intensity test on the ROLLED intensity
        assert (KR.view_finalize_ref(a["depth"], np.roll(a["inten"], 1, axis=1), *args, 1, 0, 0)[1] != notmask).any()
        # no intensity test at all (channels 1), and the intensity cut left out of channel 2
        one = KR.view_finalize_ref(a["depth"], None, a["obf"], a["sky"], a["goal_depth"], None, 1, 1, 0, 0)
        assert (one[1][0] != notmask[0]).any()
        assert (real[1] == 0.0001).sum() >= 3 and (np.roll(a["inten"], 1, axis=1) >= 1)[real[1] == 0.0001].any()
        # the sky: unrolled, or shifted by 2 or by 4 rows instead of 3
        sky = np.roll(a["sky"].astype(bool), 1, axis=1)
        shift = lambda s, k: np.concatenate([np.repeat(s[:1], k, axis=0), s[:-k]])
        assert np.array_equal(notsky, ~shift(sky, 3))
        for bad in (~shift(a["sky"].astype(bool), 3), ~shift(sky, 2), ~shift(sky, 4)):
            assert (bad != notsky).any()
        # the first-view mask of the densification variant, and the all-masked second channel of the completion one
        dens = KR.view_finalize_ref(a["depth"], a["inten"], *args, 1, 2, 1)[1]
        assert (dens != notmask).any() and dens[0, :, :W // 4].sum() == 0 and dens[0, :, W // 4:].all()
        assert not KR.view_finalize_ref(a["depth"], a["inten"], a["obf"], a["sky"], None, None, 2, 1, 3, 0)[1][1].any()
