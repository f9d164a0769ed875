"""Per-kernel parity of the pooling, adjoint and InstanceNorm++ kernels (MI355X only; through the sdpk_* entries).

  kernel (float32 and, where it exists, the bf16 tape "h16")      reference (float64)                gate
  maxpool5 + idx               lattice, with and without ties     F.max_pool2d                       equality; idx -> a maximum
                               (also past the rows-per-block thresholds of both launchers)
  maxpool5_backward            lattice dp on tie-free data        autograd of F.max_pool2d           equality
                               tied data                          scatter by the kernel's own idx    equality, sum conserved
  avgpool2 (float32 only)      lattice / real                     mean_pool2                         equality / 4 ulp of sum|.|
  unpool                       lattice                            repeat / 4                         equality
  upsample_backward acc 0 / 1  real                               autograd of F.interpolate          kernel_ref.upsample_backward_gate
  elu_backward_post (+ res)    lattice (y >= 0) / real            dy * elu'(y) + res                 equality / 4 ulp
  add_tensors                  lattice / real                     a + b                              equality / 1 ulp
  conv stats -> inpp_finalize  groups of 128 / 32 / 64 values     instance_norm_pp's scale, shift    kernel_ref.stats_gate, propagated
  inpp_backward (+ r1, r2)     real                               autograd of instance_norm_pp       4 x the float32 torch-CPU error
A bf16 output is the reference rounded once (lattice) or carries one more 2^-8 |ref| (real).  Shapes: odd tile / block
counts, more than one block, a partial last row block.
"""
import math

import numpy as np
import pytest
import torch

import kernel_lib as KL
import kernel_ref as KR
from oracle import scorenet_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F64 = torch.float64
H16 = [False, True]

# (B, C, H, W) of the lattice cases: sums of at most 25 values of at most 4 units
LATTICE_SHAPES = [(1, 128, 12, 96), (3, 256, 40, 32)]


def lattice_bound(B, C, H, W):
    return 25 * 4 + 4


def _dt(h16):
    return torch.bfloat16 if h16 else torch.float32


def up(t, h16=False):
    return KR.nhwc(t).to(_dt(h16)).to(DEV)


def back(t):
    return KR.nchw(t.to(F64).cpu())


def rounded(t, h16):
    return KR.bf16_round(t) if h16 else t


def tie_free(B, C, H, W, rng):
    """Integers in [-12, 12], distinct inside every 5x5 window: position (y % 5, x % 5) through a per-channel permutation."""
    perm = torch.from_numpy(np.stack([rng.permutation(25) for _ in range(C)]))           # [C, 25]
    pos = (torch.arange(H).view(H, 1) % 5) * 5 + torch.arange(W).view(1, W) % 5           # [H, W]
    return (perm[:, pos] - 12).to(F64).unsqueeze(0).repeat(B, 1, 1, 1).contiguous()


def run_maxpool(x, h16):
    B, C, H, W = x.shape
    xin = up(x, h16)
    out = torch.full_like(xin, float("nan"))
    idx = torch.full((B, H, W, C), 255, dtype=torch.uint8, device=DEV)
    KL.check(KL.lib().sdpk_maxpool5(xin.data_ptr(), out.data_ptr(), idx.data_ptr(), B, H, W, C, int(h16), KL.stream()), "maxpool5")
    torch.cuda.synchronize()
    return back(out), idx


@pytest.mark.parametrize("h16", H16)
@pytest.mark.parametrize("shape", LATTICE_SHAPES)
def test_maxpool5_values_and_indices_with_ties(shape, h16):
    """Lattice data in {-4..4}/4: nine values, so nearly every window has ties (as ELU's saturation at -1 gives in
    production).  Values: equality.  idx: every window's index points at a maximal element."""
    B, C, H, W = shape
    x = KR.lattice(KR.rng_for(f"mp{shape}"), shape, -4, 4, 4)
    out, idx = run_maxpool(x, h16)
    ref = KR.maxpool5(x)
    assert torch.equal(out, ref)
    if not h16:      # the forward plan's variant without indices
        xin = up(x)
        o2 = torch.full_like(xin, float("nan"))
        KL.check(KL.lib().sdpk_maxpool5(xin.data_ptr(), o2.data_ptr(), None, B, H, W, C, 0, KL.stream()), "maxpool5")
        assert torch.equal(back(o2), ref)
    i = KR.nchw(idx.cpu().to(torch.int64))
    assert int(i.max()) < 25
    assert torch.equal(KR.pick_by_idx(x, i), ref)
    _, ti = torch.nn.functional.max_pool2d(x, 5, 1, 2, return_indices=True)
    ty, tx = ti // W, ti % W
    same = (ty == torch.arange(H).view(1, 1, H, 1) + i // 5 - 2) & (tx == torch.arange(W).view(1, 1, 1, W) + i % 5 - 2)
    print(f"maxpool5 {shape} h16={h16}: tie choice equals torch-CPU's in {same.float().mean().item():.4f} of the windows")


# (B, C, H, W), h16: the smallest shapes past the launchers' rows-per-block thresholds (aux.hip maxpool5: 32 rows once
# the grid has 512 blocks of 32 rows x 8 columns x 128 channels; the bf16 kernel 16 / 32 rows once it has 1024 of
# 16 / 32 rows x 16 columns), with a partial last row block.  The small shapes above run 16 (float32) and 8 (bf16) rows.
THRESHOLD_SHAPES = [((4, 128, 36, 512), False), ((4, 128, 17, 2048), True), ((4, 128, 33, 2048), True)]


@pytest.mark.parametrize("shape,h16", THRESHOLD_SHAPES)
def test_maxpool5_rows_per_block_thresholds(shape, h16):
    """Lattice data with ties: values equal, idx points at a maximal element -- on the 32-row (float32) and 16- and
    32-row (bf16) launches that the production shapes take."""
    B, C, H, W = shape
    strips = B * (W // (16 if h16 else 8)) * (C // 128)
    blocks = lambda rows: strips * ((H + rows - 1) // rows)
    rows = (32 if blocks(32) >= 1024 else 16 if blocks(16) >= 1024 else 8) if h16 else (32 if blocks(32) >= 512 else 16)
    assert rows == (32 if (not h16 or H == 33) else 16)
    x = KR.lattice(KR.rng_for(f"mpt{shape}"), shape, -4, 4, 4)
    out, idx = run_maxpool(x, h16)
    ref = KR.maxpool5(x)
    assert torch.equal(out, ref)
    assert torch.equal(KR.pick_by_idx(x, KR.nchw(idx.cpu().to(torch.int64))), ref)


@pytest.mark.parametrize("with_res", [False, True])
@pytest.mark.parametrize("h16", H16)
@pytest.mark.parametrize("shape", LATTICE_SHAPES)
def test_maxpool5_backward(shape, h16, with_res):
    """Tie-free data: equality with float64 autograd.  Tied data: the gradient lands where the kernel's own idx points
    (maximal elements, checked above) and its sum is conserved; whether the choice is torch-CPU's is printed only."""
    B, C, H, W = shape
    rng = KR.rng_for(f"mpb{shape}{h16}{with_res}")
    dp = KR.lattice(rng, shape, -4, 4, 4)
    res = KR.lattice(rng, shape, -4, 4, 4) if with_res else None
    for tied in (False, True):
        x = KR.lattice(rng, shape, -4, 4, 4) if tied else tie_free(B, C, H, W, rng)
        _, idx = run_maxpool(x, h16)
        d, r = up(dp, h16), (up(res, h16) if with_res else None)
        dst = torch.full_like(d, float("nan"))
        KL.check(KL.lib().sdpk_maxpool5_backward(idx.data_ptr(), d.data_ptr(), KL.ptr(r), dst.data_ptr(), B, H, W, C, int(h16),
                                                 KL.stream()), "maxpool5_backward")
        got = back(dst)
        i = KR.nchw(idx.cpu().to(torch.int64))
        assert torch.equal(KR.pick_by_idx(x, i), KR.maxpool5(x))        # this x's idx points at maximal elements
        own = KR.scatter_by_idx(i, dp) + (res if with_res else 0.0)
        assert torch.equal(got, own)
        assert got.sum().item() == dp.sum().item() + (res.sum().item() if with_res else 0.0)
        auto = KR.maxpool5_backward(x, dp) + (res if with_res else 0.0)
        if tied:
            print(f"maxpool5_backward {shape} h16={h16}: equals torch-CPU's tie choice: {torch.equal(got, auto)}")
        else:
            assert torch.equal(got, auto)


# odd tile counts: (B, C, H, W) with B * H * W * C / 4 no multiple of the 256-thread block
SMALL = [(3, 36, 6, 10), (1, 128, 2, 6)]


@pytest.mark.parametrize("shape", SMALL)
def test_avgpool2(shape):
    B, C, H, W = shape
    L = KL.lib()
    for real in (False, True):
        r = KR.rng_for(f"avg{shape}{real}")
        x = KR.normal(r, shape) if real else KR.lattice(r, shape, -4, 4, 4)
        xin = up(x)
        out = torch.full((B, H // 2, W // 2, C), float("nan"), device=DEV)
        KL.check(L.sdpk_avgpool2(xin.data_ptr(), out.data_ptr(), B, H, W, C, KL.stream()), "avgpool2")
        got, ref = back(out), R.mean_pool2(x)
        if real:   # three adds and a division: <= 4 roundings of the sum of magnitudes
            assert ((got - ref).abs() <= KR.avgpool2_gate(x)).all()
        else:
            assert torch.equal(got, ref)
    with pytest.raises(KL.KernelError):
        KL.check(L.sdpk_avgpool2(xin.data_ptr(), out.data_ptr(), B, H + 1, W, C, KL.stream()), "avgpool2")


@pytest.mark.parametrize("h16", H16)
@pytest.mark.parametrize("shape", SMALL)
def test_unpool(shape, h16):
    B, C, H, W = shape
    L = KL.lib()
    d = KR.lattice(KR.rng_for(f"unpool{shape}"), (B, C, H // 2, W // 2), -4, 4, 4)
    din = up(d, h16)
    dst = torch.full((B, H, W, C), float("nan"), dtype=_dt(h16), device=DEV)
    KL.check(L.sdpk_unpool(din.data_ptr(), dst.data_ptr(), B, H, W, C, int(h16), KL.stream()), "unpool")
    assert torch.equal(back(dst), KR.unpool(d))
    for bad in ((B, H + 1, W, C), (B, H, W + 1, C), (B, H, W, C + 2)):   # odd sizes: rejected, not indexed
        with pytest.raises(KL.KernelError):
            KL.check(L.sdpk_unpool(din.data_ptr(), dst.data_ptr(), *bad, int(h16), KL.stream()), "unpool")


@pytest.mark.parametrize("accumulate", [0, 1])
@pytest.mark.parametrize("h16", H16)
@pytest.mark.parametrize("shape", [(3, 36, 6, 10), (1, 128, 4, 6), (2, 128, 16, 64)])
def test_upsample_backward(shape, h16, accumulate):
    """Real operands; the gate is kernel_ref.upsample_backward_gate (its docstring has the derivation)."""
    B, C, H, W = shape
    r = KR.rng_for(f"upb{shape}{h16}")
    g = rounded(KR.normal(r, shape), h16)
    lo0 = rounded(KR.normal(r, (B, C, H // 2, W // 2)), h16)
    gin, dlow = up(g, h16), up(lo0, h16)
    L = KL.lib()
    KL.check(L.sdpk_upsample_backward(gin.data_ptr(), dlow.data_ptr(), B, H, W, C, accumulate, int(h16), KL.stream()), "upsample_backward")
    ref = KR.upsample_backward(g) + (lo0 if accumulate else 0.0)
    gate = KR.upsample_backward_gate(g, lo0 if accumulate else None, ref, h16)
    err = (back(dlow) - ref).abs()
    print(f"upsample_backward {shape} h16={h16} acc={accumulate}: max err {err.max().item():.3e}, max gate {gate.max().item():.3e}")
    assert (err <= gate).all()
    for bad in ((H + 1, W), (2, W), (H, 2)):     # odd, or a one-pixel dlow (scale 0): rejected, not indexed
        with pytest.raises(KL.KernelError):
            KL.check(L.sdpk_upsample_backward(gin.data_ptr(), dlow.data_ptr(), B, *bad, C, 0, int(h16), KL.stream()), "upsample_backward")


@pytest.mark.parametrize("h16", H16)
@pytest.mark.parametrize("shape", SMALL)
def test_elu_backward_post_and_add_tensors(shape, h16):
    """Lattice (y >= 0, so elu' = 1): equality.  Real: dy * (y + 1) + res is three roundings, a + b one: 4 (1) ulp of the
    sum of magnitudes; bf16 output: + 2^-8 |ref|."""
    n = math.prod(shape)
    L = KL.lib()
    for real in (False, True):
        r = KR.rng_for(f"elub{shape}{real}")
        if real:
            dy, res = rounded(KR.normal(r, shape), h16), rounded(KR.normal(r, shape), h16)
            y = rounded(R.elu(KR.normal(r, shape)).to(torch.float32).to(F64), h16)
        else:
            dy, res, y = (KR.lattice(r, shape, -4, 4, 4), KR.lattice(r, shape, -4, 4, 4), KR.lattice(r, shape, 0, 4, 4))
        for with_res in (False, True):
            a, b, c = up(dy, h16), up(y, h16), up(res, h16)
            dst = torch.full_like(a, float("nan"))
            KL.check(L.sdpk_elu_backward_post(a.data_ptr(), b.data_ptr(), c.data_ptr() if with_res else None, dst.data_ptr(), n,
                                              int(h16), KL.stream()), "elu_backward_post")
            ref = dy * KR.elu_grad(y, 2) + (res if with_res else 0.0)
            if real:
                gate = KR.elu_post_gate(dy, y, res if with_res else None, ref, h16)
                assert ((back(dst) - ref).abs() <= gate).all()
            else:
                assert torch.equal(back(dst), rounded(ref, h16))
        a, c = up(dy, h16), up(res, h16)
        dst = torch.full_like(a, float("nan"))
        KL.check(L.sdpk_add_tensors(a.data_ptr(), c.data_ptr(), dst.data_ptr(), n, int(h16), KL.stream()), "add_tensors")
        if real:
            assert ((back(dst) - (dy + res)).abs() <= KR.add_gate(dy, res, h16)).all()
        else:
            assert torch.equal(back(dst), rounded(dy + res, h16))
    for fn, args in ((L.sdpk_elu_backward_post, (a.data_ptr(), a.data_ptr(), None, dst.data_ptr(), n - 2)),
                     (L.sdpk_add_tensors, (a.data_ptr(), c.data_ptr(), dst.data_ptr(), n - 2))):
        with pytest.raises(KL.KernelError):    # a tail of 2 elements would be left unwritten
            KL.check(fn(*args, int(h16), KL.stream()), "tail")


# ------------------------------------------------------------------------------------------------ InstanceNorm++
def _groups(y, cnt):
    """Host (mean, M2) groups of cnt consecutive NHWC pixels: [B][T][C][2] float32 (as begin_conv's 64-pixel tiles)."""
    B, C, H, W = y.shape
    v = KR.nhwc(y).reshape(B, H * W // cnt, cnt, C)
    m = v.mean(dim=2)
    return torch.stack([m, ((v - m[:, :, None, :]) ** 2).sum(dim=2)], dim=-1).to(torch.float32)


def _finalize(stats, cnt, alpha, gamma, beta):
    B, T, C, _ = stats.shape
    f = lambda t: t.to(torch.float32).contiguous().to(DEV)
    st, al, ga, be = f(stats), f(alpha), f(gamma), f(beta)
    ss = torch.full((B, C, 2), float("nan"), device=DEV)
    nst = torch.full((B, C, 4), float("nan"), device=DEV)
    scratch = torch.empty(B * C * 2, dtype=F64, device=DEV)
    KL.check(KL.lib().sdpk_inpp_finalize(st.data_ptr(), B, T, float(cnt), C, al.data_ptr(), ga.data_ptr(), be.data_ptr(),
                                         ss.data_ptr(), nst.data_ptr(), scratch.data_ptr(), KL.stream()), "inpp_finalize")
    torch.cuda.synchronize()
    return ss, nst


def _norm_params(C, rng):
    f = lambda t: t.to(torch.float32).to(F64)
    return f(1.0 + 0.1 * KR.normal(rng, (C,))), f(1.0 + 0.1 * KR.normal(rng, (C,))), f(0.1 * KR.normal(rng, (C,)))


def check_scale_shift(ss, y, alpha, gamma, beta, gmax=0.0):
    """ss against the (scale, shift) implied by instance_norm_pp on y in float64, with kernel_ref.stats_gate's bounds
    on mean and variance carried through scale = gamma (var + eps)^-1/2 and shift = gamma (-mean inv + mhat alpha) +
    beta to first order (x 1.5 for the second), plus 4 float32 roundings of the results."""
    scale, shift = KR.inpp_scale_shift(y, alpha, gamma, beta)
    mean, var = y.mean(dim=(2, 3)), y.var(dim=(2, 3), unbiased=False)
    gm, gv = KR.stats_gate(y, gmax)
    inv = (var + 1e-5) ** -0.5
    dinv = 1.5 * 0.5 * (var + 1e-5) ** -1.5 * gv
    dev = mean - mean.mean(dim=-1, keepdim=True)
    v = mean.var(dim=-1, keepdim=True)
    tinv = (v + 1e-5) ** -0.5
    ddev, G = gm + gm.mean(dim=-1, keepdim=True), gm.amax(dim=-1, keepdim=True)
    dv = 2 * torch.sqrt(v) * 1.1 * G + G * G            # var over the channels of means each off by <= G
    dmn = 1.5 * (tinv * ddev + dev.abs() * 0.5 * tinv ** 3 * dv)
    g_scale = gamma.abs() * dinv + 4 * KR.EPS24 * scale.abs()
    g_shift = gamma.abs() * (mean.abs() * dinv + inv * gm + alpha.abs() * dmn) + \
        4 * KR.EPS24 * (shift.abs() + (gamma * mean * inv).abs() + beta.abs())
    got = ss.to(F64).cpu()
    es, eh = (got[..., 0] - scale).abs(), (got[..., 1] - shift).abs()
    print(f"  scale err / gate max {(es / g_scale).max().item():.3f}, shift err / gate max {(eh / g_shift).max().item():.3f}; "
          f"min var {var.min().item():.3e}, max |mean|/std {(mean.abs() / torch.sqrt(var + 1e-30)).clamp(max=1e9).max().item():.3e}")
    assert (es <= g_scale).all() and (eh <= g_shift).all()


def _special_channels(w, bias, x, c):
    """Channel 5 constant (variance 0), channel 7 with |mean| >= 1e3 std: through the conv's weights and bias."""
    w[5] = 0.0
    bias[5] = 3.0
    y7 = KR.conv_forward(c, {"x": x, "w": w, "bias": torch.zeros_like(bias)})["out"][:, 7]
    bias[7] = float(torch.tensor(1500.0 * y7.std().item(), dtype=torch.float32))
    return w, bias


@pytest.mark.parametrize("kind", ["conv128", "pooled32"])
def test_conv_statistics_then_inpp_finalize(kind):
    """The conv's stats epilogue (groups of 128 values; of 32 pooled values for the ConvMeanPool) -> inpp_finalize."""
    import test_gpu_kernels_conv as TC
    if kind == "conv128":      # 3 images x 3 tiles: an odd group count per image
        c = KR.Case("stats-conv128", "fwd", 3, 8, 48, 128, 128, bias=True, stats=True, real=True)
    else:
        c = KR.Case("stats-pooled32", "fwd", 3, 4, 192, 128, 256, circular=False, pool=True, pro=KR.PRO_ELU, bias=True,
                    stats=True, real=True)
    o = KR.make_operands(c)
    o["w"], o["bias"] = _special_channels(o["w"], o["bias"], o["x"], c)
    got = TC.run_case(c, "fp32x3", o)
    y = got["out"]                                  # the statistics are those of the GPU's own output
    alpha, gamma, beta = _norm_params(c.Cout, KR.rng_for(kind))
    ss, _ = _finalize(got["stats"], got["cnt"], alpha, gamma, beta)
    assert (got["stats"].shape[1], got["cnt"]) in ((3, 128), (6, 32))
    check_scale_shift(ss, y, alpha, gamma, beta)


def test_inpp_finalize_on_64_value_groups():
    """Groups of 64 values (begin_conv's tiles), made on the host in float64: only the finalize is under test, so the
    bound is the float32 rounding of the groups handed over."""
    r = KR.rng_for("fin64")
    y = KR.normal(r, (3, 128, 8, 40))
    y[:, 5] = 3.0
    y[:, 7] = y[:, 7] * 1e-3 + 2.0
    alpha, gamma, beta = _norm_params(128, r)
    ss, nst = _finalize(_groups(y, 64), 64, alpha, gamma, beta)
    check_scale_shift(ss, y, alpha, gamma, beta)
    mean, var = y.mean(dim=(2, 3)), y.var(dim=(2, 3), unbiased=False)
    n = nst.to(F64).cpu()
    assert ((n[..., 0] - mean).abs() <= 64 * KR.EPS24 * y.abs().amax(dim=(2, 3))).all()
    assert torch.isfinite(n).all()


@pytest.mark.parametrize("with_r", [False, True])
@pytest.mark.parametrize("h16", H16)
@pytest.mark.parametrize("shape", [(3, 128, 16, 96), (2, 256, 8, 64)])
def test_inpp_backward(shape, h16, with_r):
    """Against float64 autograd of instance_norm_pp.  Gate: 4 x the error of the same backward evaluated by torch-CPU
    in float32 (max |.| per tensor; the factor is for the kernel's different reduction tree); bf16 output: + 2^-8 |ref|."""
    B, C, H, W = shape
    r = KR.rng_for(f"inppb{shape}{h16}{with_r}")
    h, g = rounded(KR.normal(r, shape), h16), rounded(KR.normal(r, shape), h16)
    h[:, 3] += 4.0
    h = rounded(h.to(torch.float32).to(F64), h16)
    r1, r2 = rounded(KR.normal(r, shape), h16), rounded(KR.normal(r, shape), h16)
    alpha, gamma, beta = _norm_params(C, r)
    _, nst = _finalize(_groups(h, 128), 128, alpha, gamma, beta)
    f = lambda t: t.to(torch.float32).contiguous().to(DEV)
    al, ga = f(alpha), f(gamma)
    part = torch.empty(B * (H * W // 512) * C * 2, device=DEV)
    coef, ppart = torch.empty(B * C * 4, device=DEV), torch.empty(B * C * 3, device=DEV)
    dal, dga, dbe = (torch.full((C,), float("nan"), device=DEV) for _ in range(3))
    gi, hi = up(g, h16), up(h, h16)
    r1i, r2i = (up(r1, h16), up(r2, h16)) if with_r else (None, None)
    out = torch.full_like(gi, float("nan"))
    KL.check(KL.lib().sdpk_inpp_backward(gi.data_ptr(), hi.data_ptr(), nst.data_ptr(), al.data_ptr(), ga.data_ptr(), B, H * W, C,
                                         part.data_ptr(), coef.data_ptr(), ppart.data_ptr(), dal.data_ptr(), dga.data_ptr(),
                                         dbe.data_ptr(), KL.ptr(r1i), KL.ptr(r2i), out.data_ptr(), int(h16), KL.stream()),
             "inpp_backward")
    torch.cuda.synchronize()
    ref = list(KR.inpp_backward(h, g, alpha, gamma, beta))
    f32 = [t.to(F64) for t in KR.inpp_backward(h, g, alpha, gamma, beta, torch.float32)]
    if with_r:
        ref[0] = ref[0] + r1 + r2
        f32[0] = (f32[0].to(torch.float32) + r1.to(torch.float32) + r2.to(torch.float32)).to(F64)
    got = [back(out)] + [t.to(F64).cpu() for t in (dal, dga, dbe)]
    for name, a, b, c32 in zip(("dh", "dalpha", "dgamma", "dbeta"), got, ref, f32):
        e32, e = (c32 - b).abs().max().item(), (a - b).abs().max().item()
        gate = 4 * e32 + (2.0 ** -8 * b.abs().max().item() if (h16 and name == "dh") else 0.0)
        print(f"inpp_backward {shape} h16={h16} r={with_r} {name}: gpu err {e:.3e}, float32 torch-CPU err {e32:.3e}, gate {gate:.3e}")
        assert e <= gate, name
