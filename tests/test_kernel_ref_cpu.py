"""The per-kernel references and gates themselves (CPU only; tests/kernel_ref.py).

* every lattice case of the GPU modules' tables keeps its largest partial sum below 2^24 lattice units, and a float32
  torch-CPU evaluation of it EQUALS the float64 reference (the exactness the GPU equality gate rests on);
* a float32 torch-CPU evaluation of every real-valued case passes the fp32 gate;
* for each conv direction, a reference with ONE misplaced term -- a border pixel read one lattice unit off, the wrap
  column of one row taken as zero, one channel pair swapped in one tile -- fails the gate of every mode, on the
  smallest case of each class: the gates see a single-term error.
"""
import pytest
import torch

import kernel_ref as KR
import test_gpu_kernels_aux as TA
import test_gpu_kernels_conv as TC

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
