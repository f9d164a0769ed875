"""Float64 references, operand generators and gates for the per-kernel parity tests (pure CPU).

The score net's kernels -- begin_conv and end_conv, their backward kernels and the DSM loss included (the "head"
section below) -- are compared one launch at a time (tests/test_gpu_kernels_*.py, through the sdpk_* entries of
include/sdp_kernels.h) with float64 torch restatements of the same operation.  Tensors are NCHW float64 in here; the
GPU modules convert to NHWC at the boundary.

Two kinds of operands:

* LATTICE operands -- small integers times a power of two: activations and output gradients in {-4..4}/4 (non-negative
  where an ELU prologue or an ELU' epilogue touches them, so that ELU is the identity and ELU' is 1), weights and
  biases in {-4..4}/8, prologue scales in {1, 2} and shifts in {0, 1, 2}/4.  Every value is bf16-representable (the
  fp32x3 lo parts are zero, bf16 mode rounds nothing) and every product and partial sum of the largest reduction of a
  case is an integer number of lattice units below 2^24 (``Case.lattice_bound()`` checks it per case), hence exact in
  float32 whatever the accumulation order, split count or MFMA shape.  THE GATE IS EQUALITY with the float64
  reference, in all three modes; a bf16 output tensor equals the reference rounded once to bf16.
* REAL operands (standard normal) only where the function itself is inexact -- ELU on negatives, elu_grad, the
  bilinear upsample-add, the statistics, the fp32x3 split.  The gates are elementwise and derived, not measured.
  With K the reduction length and S the same operation evaluated on absolute values (|ELU(h)| taken as e^h + 1
  for h < 0: the two terms the kernel subtracts):
      fp32    |gpu - ref64| <= K * 2^-24 * S
      fp32x3  |gpu - ref64| <= (2^-15 + K * 2^-24) * S
      bf16    the fp32 gate against a reference that rounds the prologue output and the weights to bf16, plus
              2^-8 * max|a| * max|w| for ONE bf16 rounding flip per output element
      bf16 output tensors: one more 2^-8 * |ref|
"""
from __future__ import annotations

import dataclasses
import math

import numpy as np
import torch
import torch.nn.functional as F

from oracle import scorenet_ref as R

F64 = torch.float64
EPS24 = 2.0 ** -24
MODES = {"fp32": 0, "fp32x3": 1, "bf16": 2}
PRO_NONE, PRO_ELU, PRO_AFFINE_ELU = 0, 1, 2


def nhwc(x):
    return x.permute(0, 2, 3, 1).contiguous()


def nchw(x):
    return x.permute(0, 3, 1, 2).contiguous()


def bf16_round(x):
    """Round-to-nearest-even to bf16, returned in x's dtype (float64 values go through float32 first: exact for
    every lattice value; for real values a double rounding is one of the flips the bf16 gate allows)."""
    return x.to(torch.float32).to(torch.bfloat16).to(x.dtype)


def rng_for(name):
    return np.random.default_rng(int.from_bytes(name.encode(), "little") % (2 ** 63))


def lattice(rng, shape, lo, hi, denom):
    return torch.from_numpy(rng.integers(lo, hi + 1, size=shape)).to(F64) / denom


def normal(rng, shape, scale=1.0):
    """Standard normal values, rounded to float32 (what the GPU is given)."""
    return torch.from_numpy(rng.standard_normal(shape).astype(np.float32)).to(F64) * scale


# ---------------------------------------------------------------------------------------------- conv cases
@dataclasses.dataclass(frozen=True)
class Case:
    """One conv launch.  kind: fwd | dgrad | wgrad.  For dgrad, Cin / Cout are the FORWARD conv's (dy has Cout
    channels, dx has Cin); pro / ss describe the forward prologue (wgrad) and dact / res the backward epilogue."""
    name: str
    kind: str
    B: int
    H: int
    W: int
    Cin: int
    Cout: int
    ks: int = 3
    dil: int = 1
    circular: bool = True
    pool: bool = False
    s2: bool = False
    pro: int = PRO_NONE
    bias: bool = False
    res: bool = False
    out2: bool = False
    up: bool = False
    epi_elu: bool = False
    stats: bool = False
    dact: int = 0
    accumulate: bool = False
    io16: bool = False
    real: bool = False          # real-valued operands (derived gates) instead of lattice ones (equality)

    @property
    def id(self):
        return self.name

    def out_hw(self):
        return (self.H // 2, self.W // 2) if (self.pool or self.s2) else (self.H, self.W)

    def K(self):
        """Reduction length of one output element (terms of the longest sum, bias and addends included)."""
        if self.kind == "wgrad":
            return self.B * self.H * self.W + (1 if self.accumulate else 0)
        cin = self.Cout if self.kind == "dgrad" else self.Cin
        k = self.ks * self.ks * cin
        if self.pool or self.s2:
            k *= 4
        return k + 4

    def lattice_bound(self):
        """Largest partial sum of the case in lattice units; must stay below 2^24 (then float32 is exact).
        Units: 1/4 for activations, gradients and addends, 1/8 for weights and biases -> products in 1/32
        (wgrad: 1/4 * 1/4 -> 1/16), the 2x2 mean two more bits."""
        amax = 4 * (2 if self.pro == PRO_AFFINE_ELU else 1) + (2 if self.pro == PRO_AFFINE_ELU else 0)
        if self.kind == "wgrad":
            return self.B * self.H * self.W * amax * 4 + 64
        if self.kind == "dgrad":
            return self.ks * self.ks * self.Cout * 4 * 4 + 8 * 4 + 64
        k = self.ks * self.ks * self.Cin * amax * 4 + 4 * 4
        if self.pool or self.s2:
            k *= 16          # four convs summed, and units of 1/128 after the division by 4
        return k + 3 * 8 * 4


def make_operands(c: Case):
    """The tensors of case c (NCHW float64; every value float32- and, on the lattice, bf16-representable)."""
    r = rng_for(c.name)
    o = {}
    pelu = c.pro != PRO_NONE and c.kind != "dgrad"
    Ho, Wo = c.out_hw()
    if c.real:
        act = lambda shape: normal(r, shape)
        wgt = lambda shape: normal(r, shape, 0.25)
    else:
        act = lambda shape, nonneg=False: lattice(r, shape, 0 if nonneg else -4, 4, 4)
        wgt = lambda shape: lattice(r, shape, -4, 4, 8)
    o["w"] = wgt((c.Cout, c.Cin, c.ks, c.ks))
    if c.kind in ("fwd", "wgrad"):
        o["x"] = act((c.B, c.Cin, c.H, c.W)) if c.real else act((c.B, c.Cin, c.H, c.W), pelu)
        if c.pro == PRO_AFFINE_ELU:
            if c.real:
                o["scale"] = 0.5 + torch.from_numpy(r.random((c.B, c.Cin)).astype(np.float32)).to(F64)
                o["shift"] = normal(r, (c.B, c.Cin), 0.5)
            else:
                o["scale"] = 2.0 ** lattice(r, (c.B, c.Cin), 0, 1, 1)
                o["shift"] = lattice(r, (c.B, c.Cin), 0, 2, 4)
    if c.kind == "fwd":
        if c.bias:
            o["bias"] = wgt((c.Cout,))
        if c.res:
            o["res"] = act((c.B, c.Cout, Ho, Wo))
        if c.out2:
            o["res2"] = act((c.B, c.Cout, Ho, Wo))
        if c.up:
            o["up"] = normal(r, (c.B, c.Cout, c.H // 2, c.W // 2))
    elif c.kind == "dgrad":
        o["dy"] = act((c.B, c.Cout, c.H, c.W))
        if c.res:
            o["res"] = act((c.B, c.Cin, c.H, c.W))
        if c.dact:
            o["aux"] = act((c.B, c.Cin, c.H, c.W)) if c.real else act((c.B, c.Cin, c.H, c.W), True)
            if c.dact == 3:
                if c.real:
                    o["escale"] = 0.5 + torch.from_numpy(r.random((c.B, c.Cin)).astype(np.float32)).to(F64)
                    o["eshift"] = normal(r, (c.B, c.Cin), 0.5)
                else:
                    o["escale"] = 2.0 ** lattice(r, (c.B, c.Cin), 0, 1, 1)
                    o["eshift"] = lattice(r, (c.B, c.Cin), 0, 2, 4)
    else:
        o["dy"] = act((c.B, c.Cout, c.H, c.W))
        if c.accumulate:
            o["w0"] = act((c.Cout, c.Cin, c.ks, c.ks))
            o["b0"] = act((c.Cout,))
    if c.real and c.dact == 2:      # form 2 takes the ELU's OUTPUT (> -1)
        o["aux"] = R.elu(o["aux"]).to(torch.float32).to(F64)
    if c.real and c.io16:           # the bf16 tape holds bf16 values
        for k in ("x", "res", "res2", "up", "dy", "aux"):
            if k in o:
                o[k] = bf16_round(o[k])
    return o


def prologue(c: Case, o, absval=False, bf16=False):
    """The conv's input after its prologue.  absval: the S evaluation (every term by its magnitude)."""
    x = o["x"]
    if c.pro == PRO_AFFINE_ELU:
        s, t = o["scale"][:, :, None, None], o["shift"][:, :, None, None]
        h = x * s + t
        habs = x.abs() * s.abs() + t.abs()
    else:
        h, habs = x, x.abs()
    if c.pro == PRO_NONE:
        a = habs if absval else h
    elif absval:
        a = torch.where(h > 0, habs, torch.exp(torch.clamp(h, max=0.0)) + 1.0)
    else:
        a = R.elu(h)
    return bf16_round(a) if bf16 else a


def elu_grad(t, form):
    """d ELU / d h from the pre-activation (forms 1, 3) or from the ELU's output (form 2)."""
    if form == 2:
        return torch.where(t > 0, torch.ones_like(t), t + 1.0)
    return torch.where(t > 0, torch.ones_like(t), torch.exp(torch.clamp(t, max=0.0)))


def _conv(c: Case, a, w, b=None):
    return R.conv2d(a, w, b, dilation=c.dil, circular=c.circular)


def conv_forward(c: Case, o, absval=False, bf16=False, mutate=None):
    """{'out', 'out2'} of the forward launch.  mutate(a, w) -> (a, w): a deliberately wrong operand pair
    (tests/test_kernel_ref_cpu.py), applied after the prologue."""
    A = (lambda t: t.abs()) if absval else (lambda t: t)
    a = prologue(c, o, absval, bf16)
    w = A(bf16_round(o["w"]) if bf16 else o["w"])
    if mutate:
        a, w = mutate(a, w)
    y = _conv(c, a, w, A(o["bias"]) if c.bias else None)
    if c.pool or c.s2:
        y = R.mean_pool2(y)
    if c.up:
        y = y + F.interpolate(A(o["up"]), size=y.shape[2:], mode="bilinear", align_corners=True)
    if c.res:
        y = y + A(o["res"])
    out = {}
    if c.out2:
        out["out2"] = y + A(o["res2"])
    if c.epi_elu:
        y = torch.where(y > 0, y, torch.exp(torch.clamp(y, max=0.0)) + 1.0) if absval else R.elu(y)
    out["out"] = y
    return out


def conv_dgrad(c: Case, o, absval=False, bf16=False, mutate=None):
    """{'out'}: d loss / d conv input = autograd of the forward conv, * elu'(aux), + res."""
    A = (lambda t: t.abs()) if absval else (lambda t: t)
    w = A(bf16_round(o["w"]) if bf16 else o["w"])
    dy = A(bf16_round(o["dy"]) if bf16 else o["dy"])
    if mutate:
        dy, w = mutate(dy, w)
    x = torch.zeros(c.B, c.Cin, c.H, c.W, dtype=dy.dtype, requires_grad=True)
    (dx,) = torch.autograd.grad(_conv(c, x, w), x, dy)
    if c.dact:
        h = o["aux"]
        if c.dact == 3:
            h = h * o["escale"][:, :, None, None] + o["eshift"][:, :, None, None]
        dx = dx * elu_grad(h, c.dact)
    if c.res:
        dx = dx + A(o["res"])
    return {"out": dx}


def conv_wgrad(c: Case, o, absval=False, bf16=False, mutate=None):
    """{'dw', 'db'}: autograd of the forward conv (prologue included) with respect to weight and bias."""
    A = (lambda t: t.abs()) if absval else (lambda t: t)
    a = prologue(c, o, absval, bf16)
    dy = A(bf16_round(o["dy"]) if bf16 else o["dy"])
    if mutate:
        a, dy = mutate(a, dy)
    w = torch.zeros(c.Cout, c.Cin, c.ks, c.ks, dtype=dy.dtype, requires_grad=True)
    (dw,) = torch.autograd.grad(_conv(c, a, w), w, dy)
    db = A(o["dy"]).sum(dim=(0, 2, 3))     # the bias gradient sums the gradient as stored, before any rounding
    if c.accumulate:
        dw, db = dw + A(o["w0"]), db + A(o["b0"])
    return {"dw": dw, "db": db}


REFS = {"fwd": conv_forward, "dgrad": conv_dgrad, "wgrad": conv_wgrad}


def reference(c: Case, o, mode="fp32"):
    """The float64 reference of mode `mode` (bf16: prologue output, gradient and weights rounded to bf16)."""
    return REFS[c.kind](c, o, bf16=(mode == "bf16" and c.real))


def gate(c: Case, o, mode, ref):
    """Elementwise bound on |gpu - ref| per output tensor: zeros on lattice operands (equality), the module
    docstring's table on real ones.  ELU epilogues on lattice operands: exact where the pre-activation is
    non-negative, 4 * 2^-23 (the error of e^h - 1 in float32, |ELU| < 1) elsewhere."""
    if not c.real:
        g = {k: torch.zeros_like(v) for k, v in ref.items()}
        if c.epi_elu:
            g["out"] = torch.where(ref["out"] >= 0, 0.0, 4 * 2.0 ** -23).to(F64)
            # (the second output is taken before the ELU: exact)
        return g
    S = REFS[c.kind](c, o, absval=True)
    K = c.K()
    rel = K * EPS24 + (2.0 ** -15 if mode == "fp32x3" else 0.0)
    flip = 0.0
    if mode == "bf16":
        if c.kind == "fwd":
            amax, wmax = prologue(c, o).abs().max(), o["w"].abs().max()
        elif c.kind == "dgrad":
            amax, wmax = o["dy"].abs().max(), o["w"].abs().max()
        else:
            amax, wmax = prologue(c, o).abs().max(), o["dy"].abs().max()
        flip = float(2.0 ** -8 * amax * wmax)
    g = {k: rel * S[k] + flip for k in ref}
    if c.io16:
        g = {k: g[k] + 2.0 ** -8 * ref[k].abs() for k in g}
    return g


def finish_io16(c: Case, ref):
    """A bf16 output tensor of an exact (lattice) result is that result rounded once."""
    if c.io16 and not c.real and c.kind != "wgrad":
        return {k: bf16_round(v) for k, v in ref.items()}
    return ref


def stats_gate(y, gmax=0.0):
    """Bounds on the per-(b, c) mean and biased variance recombined from the kernel's (mean, M2) groups, against the
    float64 mean / variance of the output y.  A group mean is <= 32 float32 adds and a scale: off by d <= 64 * 2^-24
    max|y|.  The deviations v - mean_group are then exact up to d, so a sum of squares (and each Chan merge's
    n dm^2 / 2, |dm| ~ std) is off by <= 2 std d + d^2 per value, plus 64 roundings of the sum itself:
        |mean err| <= d,   |var err| <= 64 * 2^-24 var + 2 std d + d^2
    -- relative to the variance, NOT to E[y^2]: a channel with |mean| >> std keeps a meaningful bound.  gmax: the
    output's own gate (real operands: y is the reference, not the GPU's output), which moves the mean by as much
    and the variance by 2 std gmax + gmax^2."""
    var = y.var(dim=(2, 3), unbiased=False)
    std = torch.sqrt(var)
    d = 64 * EPS24 * y.abs().amax(dim=(2, 3)) + gmax
    return d, 64 * EPS24 * var + 2 * std * d + d * d


def combine_stats(stats, cnt):
    """[B][T][C][2] (mean, M2) groups of cnt values each -> per-(b, c) mean and biased variance, in float64."""
    m, q = stats[..., 0].to(F64), stats[..., 1].to(F64)
    mean = m.mean(dim=1)
    m2 = (q + cnt * (m - mean[:, None, :]) ** 2).sum(dim=1)
    return mean, m2 / (stats.shape[1] * cnt)


# ---------------------------------------------------------------------------------------------- mutants
# Each mutant misplaces what ONE pixel position contributes, so every output element it reaches has one wrong term
# per input channel touched (a single term for tap_shift) among its K: the smallest index error a kernel can make.
def mutant_tap_shift(c: Case):
    """One tap at one border pixel reads its neighbour: ONE channel of pixel (0, 0) of image 0 takes the value of
    pixel (0, 1) -- the channel where the two differ most; on the lattice it is channel 0, off by one unit (1/4).
    ONE of the K terms of each output element that reaches it is wrong."""
    def mut(a, w):
        a = a.clone()
        if c.real:
            ch = int((a[0, :, 0, 1] - a[0, :, 0, 0]).abs().argmax())
            a[0, ch, 0, 0] = a[0, ch, 0, 1]
        else:
            a[0, 0, 0, 0] += 0.25
        return a, w
    return mut


def mutant_wrap_zero(c: Case):
    """The wrap column taken as zero for one row: the last column of row 0 of image 0 reads as 0."""
    def mut(a, w):
        a = a.clone()
        a[0, :, 0, -1] = 0.0
        return a, w
    return mut


def mutant_channel_swap(c: Case):
    """One channel pair (0, 1) swapped inside one 8 x 16 tile of image 0."""
    def mut(a, w):
        a = a.clone()
        t = a[0, 0, :8, :16].clone()
        a[0, 0, :8, :16] = a[0, 1, :8, :16]
        a[0, 1, :8, :16] = t
        return a, w
    return mut


MUTANTS = {"tap_shift": mutant_tap_shift, "wrap_zero": mutant_wrap_zero, "channel_swap": mutant_channel_swap}


# ---------------------------------------------------------------------------------------------- small ops
def maxpool5(x):
    return F.max_pool2d(x, kernel_size=5, stride=1, padding=2)


def maxpool5_backward(x, dp):
    """torch's adjoint of MaxPool2d(5, 1, 2) at x applied to dp (first maximum in window order on ties)."""
    x = x.clone().requires_grad_(True)
    (g,) = torch.autograd.grad(maxpool5(x), x, dp)
    return g


def window_values(x):
    """[B, C, H, W, 25]: the 5x5 window of every pixel in row-major window order, -inf outside the image."""
    B, C, H, W = x.shape
    p = F.pad(x, (2, 2, 2, 2), value=-math.inf)
    return torch.stack([p[:, :, r:r + H, s:s + W] for r in range(5) for s in range(5)], dim=-1)


def pick_by_idx(x, idx):
    """The element each window's idx (window position 5 r + s, [B, C, H, W]) points at; -inf outside the image."""
    B, C, H, W = x.shape
    p = F.pad(x, (2, 2, 2, 2), value=-math.inf)
    ys = torch.arange(H).view(1, 1, H, 1) + idx // 5
    xs = torch.arange(W).view(1, 1, 1, W) + idx % 5
    return p.view(B, C, -1).gather(2, (ys * (W + 4) + xs).view(B, C, -1)).view(B, C, H, W)


def scatter_by_idx(idx, dp):
    """Adjoint of the pooling described by idx ([B, C, H, W] window positions 5 r + s) applied to dp."""
    B, C, H, W = dp.shape
    out = torch.zeros(B, C, H + 4, W + 4, dtype=dp.dtype)
    ys = torch.arange(H).view(1, 1, H, 1) + idx // 5
    xs = torch.arange(W).view(1, 1, 1, W) + idx % 5
    flat = (ys * (W + 4) + xs).view(B, C, -1)
    out.view(B, C, -1).scatter_add_(2, flat, dp.reshape(B, C, -1))
    return out[:, :, 2:-2, 2:-2]


def upsample2(x):
    return F.interpolate(x, scale_factor=2, mode="bilinear", align_corners=True)


def upsample_backward(g):
    B, C, H, W = g.shape
    lo = torch.zeros(B, C, H // 2, W // 2, dtype=g.dtype, requires_grad=True)
    (d,) = torch.autograd.grad(upsample2(lo), lo, g)
    return d


def unpool(dout):
    return dout.repeat_interleave(2, dim=2).repeat_interleave(2, dim=3) / 4.0


def inpp_params(alpha, gamma, beta):
    return {"n.alpha": alpha, "n.gamma": gamma, "n.beta": beta}


def inpp_scale_shift(x, alpha, gamma, beta):
    """(scale, shift) [B, C] with instance_norm_pp(x) == x * scale + shift (normalization.py:163-176)."""
    mean = x.mean(dim=(2, 3))
    var = x.var(dim=(2, 3), unbiased=False)
    m = mean.mean(dim=-1, keepdim=True)
    v = mean.var(dim=-1, keepdim=True)
    mn = (mean - m) / torch.sqrt(v + 1e-5)
    inv = 1.0 / torch.sqrt(var + 1e-5)
    return gamma * inv, gamma * (-mean * inv + mn * alpha) + beta


def inpp_backward(h, g, alpha, gamma, beta, dtype=F64):
    """(dh, dalpha, dgamma, dbeta) of instance_norm_pp at h for the output gradient g, by autograd in `dtype`."""
    h = h.to(dtype).clone().requires_grad_(True)
    P = {k: v.to(dtype).clone().requires_grad_(True) for k, v in inpp_params(alpha, gamma, beta).items()}
    y = R.instance_norm_pp(h, P, "n")
    return torch.autograd.grad(y, [h, P["n.alpha"], P["n.gamma"], P["n.beta"]], g.to(dtype))


# ---------------------------------------------------------------------------------------------- gates of the small ops
def avgpool2_gate(x):
    """((a + b) + c + d) / 4: three adds and a division, <= 4 roundings of the sum of magnitudes."""
    return 4 * EPS24 * 4 * R.mean_pool2(x.abs())


def upsample_backward_gate(g, lo0, ref, h16=False):
    """dlow(i, j) = sum of wy wx g over the <= 5 x 5 high-resolution pixels whose source rows / columns include (i, j).
    A source coordinate is f = float32(scale) * index: two roundings, |df| <= 2 * 2^-24 f, and f < i + 1 for a pixel
    that reaches row i -- so a row weight is off by <= 2 (i + 1) 2^-24 and a product wy wx by <= 2 (i + j + 2) 2^-24,
    ABSOLUTE (not relative to the weight).  With S = the adjoint of |g| (+ |dlow| when accumulating into lo0) and
    G = the sum of |g| over the 6 x 6 block of rows 2i - 2 .. 2i + 3 that holds every contributing pixel:
        |err| <= 2^-24 (16 S + 2 (i + j + 2) G)        (16: the product, the fused adds of <= 16 nonzero terms)
    a bf16 output: + 2^-8 |ref|."""
    H, W = g.shape[2:]
    S = upsample_backward(g.abs()) + (lo0.abs() if lo0 is not None else 0.0)
    G = 36 * F.avg_pool2d(g.abs(), 6, 2, 2, count_include_pad=True)
    ij = torch.arange(H // 2, dtype=F64).view(1, 1, -1, 1) + torch.arange(W // 2, dtype=F64).view(1, 1, 1, -1) + 2
    return EPS24 * (16 * S + 2 * ij * G) + (2.0 ** -8 * ref.abs() if h16 else 0.0)


def elu_post_gate(dy, y, res, ref, h16=False):
    """dy * (y + 1) + res: three roundings of the sum of magnitudes (4 allowed); a bf16 output: + 2^-8 |ref|."""
    return 4 * EPS24 * (dy.abs() * (y.abs() + 1) + (res.abs() if res is not None else 0.0)) + (2.0 ** -8 * ref.abs() if h16 else 0.0)


def add_gate(a, b, h16=False):
    return EPS24 * (a.abs() + b.abs()) + (2.0 ** -8 * (a + b).abs() if h16 else 0.0)


# ---------------------------------------------------------------------------------------------- head and tail kernels
# begin_conv (input prep + zero-padded 4 -> 128 conv + statistics), end_conv (IN++ affine + ELU + zero-padded
# 128 -> 2 conv, / sigmas[labels[b]]), their backward kernels and the DSM loss.  Operands as above, with
#   begin conv     image x in {0..8}/8 (2x - 1 on the 1/4 lattice); the y-coordinate channel is exact in float32 and
#                  bf16 when H = 2^k + 1 (step 1/2^k, k <= 7); the x-coordinate channel never is (W is a multiple of
#                  128), so the forward lattice cases give that input channel zero weights
#   end conv       the test's OWN table of power-of-two sigmas, picked out of order by the labels: the division is exact
# K (the reduction length of the gates): 37 begin conv, 9 * 128 + 1 end conv, 18 end data gradient, B * H * W the
# head weight gradients.  The backward kernels are plain float32 in every mode: the fp32 row of the table.
SIGMA_ORDER = (2, 0, 3, 1)      # labels of images 0, 1, 2, ...: a different table entry each, out of order
HEAD_OPS = ("begin", "end", "begin_wgrad", "end_bwd")


@dataclasses.dataclass(frozen=True)
class Head:
    """One launch of a head / tail kernel.  op: begin | end | begin_wgrad | end_bwd.  h16: the bf16 tape's tensor of the
    call (begin: out; end: in; begin_wgrad: dy; end_bwd: o and g)."""
    name: str
    op: str
    B: int
    H: int
    W: int
    real: bool = False
    h16: bool = False
    sigmas: tuple = (0.5, 1.0, 2.0, 4.0)

    @property
    def id(self):
        return self.name

    def labels(self):
        return [SIGMA_ORDER[b % 4] for b in range(self.B)]

    def K(self, key="out"):
        if self.op == "begin":
            return 37
        if self.op == "end":
            return 9 * 128 + 1
        if self.op == "end_bwd" and key == "g":
            return 18
        return self.B * self.H * self.W

    def end_case(self):
        return Case(self.name, "fwd", self.B, self.H, self.W, 128, 2, circular=False, pro=PRO_AFFINE_ELU, bias=True,
                    real=self.real, io16=self.h16)

    def lattice_bound(self):
        """Largest partial sum in lattice units; below 2^24 float32 is exact.
        begin: activations in 1/128 (the y coordinate's step is >= 1/128; H - 1 must be a power of two <= 128),
        weights in 1/8: 37 terms of <= 128 * 4 units.  end: the conv's own bound (the division by a power of two is
        exact).  begin_wgrad: B H W terms of 4 * 4 units of 1/16 (image channels and bias).  end_bwd: dscore / sigma
        in units of 1 / (4 max sigma), <= 4 max / min of them; times 4 weight units over 18 terms (g), times
        10 activation units over B H W terms (dw)."""
        n = self.B * self.H * self.W
        if self.op == "begin":
            k = self.H - 1
            return 37 * 128 * 4 if (k & (k - 1)) == 0 and 1 <= k <= 128 else 2 ** 24
        if self.op == "end":
            return self.end_case().lattice_bound()
        if self.op == "begin_wgrad":
            return n * 4 * 4
        d = int(4 * max(self.sigmas) / min(self.sigmas))
        return max(18 * d * 4, n * d * 10)


def head_operands(c: Head):
    """The tensors of case c (NCHW float64, float32-representable; bf16-representable on the lattice and, for real
    operands, where the bf16 tape holds them)."""
    r = rng_for(c.name)
    o = {"sigmas": torch.tensor(c.sigmas, dtype=F64), "labels": torch.tensor(c.labels(), dtype=torch.int64)}
    act = (lambda s: normal(r, s)) if c.real else (lambda s: lattice(r, s, -4, 4, 4))
    wgt = (lambda s: normal(r, s, 0.25)) if c.real else (lambda s: lattice(r, s, -4, 4, 8))
    if c.op in ("begin", "begin_wgrad"):
        o["x"] = normal(r, (c.B, 2, c.H, c.W)) if c.real else lattice(r, (c.B, 2, c.H, c.W), 0, 8, 8)
        if c.op == "begin":
            o["w"], o["bias"] = wgt((128, 4, 3, 3)), wgt((128,))
            if not c.real:
                o["w"][:, 2] = 0.0          # the x coordinate is not on a lattice
        else:
            o["dy"] = act((c.B, 128, c.H, c.W))
            if c.real and c.h16:
                o["dy"] = bf16_round(o["dy"])
        return o
    o["w"] = wgt((2, 128, 3, 3))
    if c.real:
        o["x"] = normal(r, (c.B, 128, c.H, c.W))
        o["scale"] = 0.5 + torch.from_numpy(r.random((c.B, 128)).astype(np.float32)).to(F64)
        o["shift"] = normal(r, (c.B, 128), 0.5)
        if c.h16:
            o["x"] = bf16_round(o["x"])
    else:
        o["x"] = lattice(r, (c.B, 128, c.H, c.W), 0, 4, 4)
        o["scale"] = 2.0 ** lattice(r, (c.B, 128), 0, 1, 1)
        o["shift"] = lattice(r, (c.B, 128), 0, 2, 4)
    if c.op == "end":
        o["bias"] = wgt((2,))
    else:
        o["dscore"] = act((c.B, 2, c.H, c.W))
    return o


def begin_prep(x, absval=False, bf16=False):
    """The begin conv's 4-channel input: R.input_prep (float32 torch.linspace) on the float64 image."""
    p = R.input_prep(x)          # (a float64 image promotes the float32 coordinates on concatenation)
    if absval:
        p = p.abs()
    return bf16_round(p) if bf16 else p


def _pad1(t):
    return F.pad(t, (1, 1, 1, 1))


def head_reference(c: Head, o, mode="fp32", absval=False, mutate=None):
    """{'out'} (begin, end), {'dw', 'db'} (begin_wgrad) or {'g', 'dw', 'db'} (end_bwd) in float64.  mode 'bf16' on real
    operands of the forward kernels: conv input and weights rounded to bf16.  absval: the S of the gates.
    mutate(name, tensor) -> tensor, a deliberately wrong operand (tests/test_kernel_ref_cpu.py), is offered 'prep' (the
    begin conv's 4-channel input), 'pad' (the zero-padded conv input), 'pad_d' (the zero-padded dscore / sigma of the
    end data gradient) and 'sigma' (the [B] sigmas of the images)."""
    A = (lambda t: t.abs()) if absval else (lambda t: t)
    M = (lambda n, t: mutate(n, t)) if mutate else (lambda n, t: t)
    bf16 = mode == "bf16" and c.real and c.op in ("begin", "end")
    rw = lambda t: A(bf16_round(t) if bf16 else t)
    if c.op == "begin":
        a = M("pad", _pad1(M("prep", begin_prep(o["x"], absval, bf16))))
        return {"out": F.conv2d(a, rw(o["w"]), A(o["bias"]))}
    if c.op == "begin_wgrad":
        a = M("pad", _pad1(M("prep", begin_prep(o["x"], absval))))
        dy = A(o["dy"])
        w = torch.zeros(128, 4, 3, 3, dtype=dy.dtype, requires_grad=True)
        (dw,) = torch.autograd.grad(F.conv2d(a, w), w, dy)
        return {"dw": dw, "db": dy.sum(dim=(0, 2, 3))}
    sig = M("sigma", o["sigmas"][o["labels"]].clone())[:, None, None, None]
    ec = c.end_case()
    a = M("pad", _pad1(prologue(ec, o, absval, bf16)))
    if c.op == "end":
        return {"out": F.conv2d(a, rw(o["w"]), A(o["bias"])) / sig}
    dend = A(o["dscore"]) / sig
    w = torch.zeros(2, 128, 3, 3, dtype=dend.dtype, requires_grad=True)
    (dw,) = torch.autograd.grad(F.conv2d(a, w), w, dend)
    # the adjoint of the zero-padded conv, written out (so that the padding can be mutated): a correlation of the
    # padded gradient with the flipped, transposed weights; test_kernel_ref_cpu.py checks it against autograd
    da = F.conv2d(M("pad_d", _pad1(dend)), A(o["w"]).flip(2, 3).transpose(0, 1).contiguous())
    h = o["x"] * o["scale"][:, :, None, None] + o["shift"][:, :, None, None]
    return {"g": da * elu_grad(h, 1), "dw": dw, "db": dend.sum(dim=(0, 2, 3))}


def head_finish(c: Head, ref):
    """A bf16 output tensor of an exact (lattice) result is that result rounded once."""
    if c.h16 and not c.real:
        key = {"begin": "out", "end_bwd": "g"}.get(c.op)
        if key:
            ref = dict(ref)
            ref[key] = bf16_round(ref[key])
    return ref


def head_gate(c: Head, o, mode, ref):
    """Elementwise bound on |gpu - ref| per output tensor: zero (equality) on lattice operands -- but the coordinate
    channels of begin_wgrad's dw, which take the fp32 gate -- and the module docstring's table on real ones."""
    g = {k: torch.zeros_like(v) for k, v in ref.items()}
    if not c.real and c.op != "begin_wgrad":
        return g
    S = head_reference(c, o, absval=True)
    fwd = c.op in ("begin", "end")
    for k in ref:
        rel = c.K(k) * EPS24 + (2.0 ** -15 if (mode == "fp32x3" and fwd) else 0.0)
        g[k] = rel * S[k]
    if not c.real:
        g["dw"][:, :2] = 0.0
        g["db"] = torch.zeros_like(ref["db"])
        return g
    if mode == "bf16" and fwd:
        if c.op == "begin":
            flip = 2.0 ** -8 * begin_prep(o["x"]).abs().max() * o["w"].abs().max()
        else:
            flip = 2.0 ** -8 * prologue(c.end_case(), o).abs().max() * o["w"].abs().max() / \
                o["sigmas"][o["labels"]][:, None, None, None]
        g["out"] = g["out"] + flip
    key = {"begin": "out", "end_bwd": "g"}.get(c.op)
    if c.h16 and key:
        g[key] = g[key] + 2.0 ** -8 * ref[key].abs()
    return g


# ---- single-term mutants of the head kernels (each a mutate(name, tensor) of head_reference)
def head_mutant_pad_row(c: Head):
    """The zero padding above image 0 replaced by the clamped border value (what an unselected clamped load gives)."""
    def mut(name, t):
        if name in ("pad", "pad_d"):
            t = t.clone()
            t[0, :, 0, 1:-1] = t[0, :, 1, 1:-1]
        return t
    return mut


def head_mutant_pad_col(c: Head):
    """The zero padding left of image 0 replaced by the clamped border value."""
    def mut(name, t):
        if name in ("pad", "pad_d"):
            t = t.clone()
            t[0, :, 1:-1, 0] = t[0, :, 1:-1, 1]
        return t
    return mut


def head_mutant_coord_swap(c: Head):
    """The two coordinate channels of the begin conv's input swapped."""
    def mut(name, t):
        return t[:, [0, 1, 3, 2]].contiguous() if name == "prep" else t
    return mut


def head_mutant_tap(c: Head):
    """One tap read one pixel off: one channel of pixel (0, 0) of image 0 takes the value of pixel (0, 1) -- the
    channel where the two differ most; on the lattice channel 0, one unit (1/4) off."""
    def mut(name, t):
        if name in ("pad", "pad_d"):
            t = t.clone()
            if c.real:
                ch = int((t[0, :, 1, 2] - t[0, :, 1, 1]).abs().argmax())
                t[0, ch, 1, 1] = t[0, ch, 1, 2]
            else:
                t[0, 0, 1, 1] += 0.25
        return t
    return mut


def head_mutant_sigma(c: Head):
    """Image 1 divided by image 0's sigma."""
    def mut(name, t):
        if name == "sigma":
            t = t.clone()
            t[1] = t[0]
        return t
    return mut


HEAD_MUTANTS = {"pad_row": head_mutant_pad_row, "pad_col": head_mutant_pad_col, "coord_swap": head_mutant_coord_swap,
                "tap": head_mutant_tap, "sigma": head_mutant_sigma}


# ---- DSM loss (losses/dsm.py:67-119): score, noise, mask [B][n_img]; sigma [B]
# real sigmas with an exact float32 square, so that 1 / sigma^2 carries ONE rounding (the dscore gate counts it)
DSM_SIGMAS = (0.75, 13.0, 1.625)


def dsm_operands(name, B, n_img, lattice_case=False, zero_image=None):
    r = rng_for(name)
    if lattice_case:        # exactly n_img ones over the batch: scale = n_img / count * sigma^p / B = sigma^p / 2 at B = 2
        assert B == 2
        mask = np.zeros(B * n_img)
        mask[r.permutation(B * n_img)[:n_img]] = 1.0
        return {"score": lattice(r, (B, n_img), -4, 4, 4), "noise": lattice(r, (B, n_img), -4, 4, 4),
                "mask": torch.from_numpy(mask.reshape(B, n_img)).to(F64), "sigma": torch.tensor((0.5, 2.0), dtype=F64)}
    sigma = torch.tensor(DSM_SIGMAS[:B], dtype=F64)
    noise = (normal(r, (B, n_img)) * sigma[:, None]).to(torch.float32).to(F64)
    mask = torch.from_numpy((r.random((B, n_img)) > 0.3).astype(np.float64))
    if zero_image is not None:
        mask[zero_image] = 0.0
    return {"score": normal(r, (B, n_img)), "noise": noise, "mask": mask, "sigma": sigma}


def dsm_reference(o, power, per_image_count=False):
    """{'loss', 'loss_per', 'dscore'} in float64: R.dsm_loss with its per-image terms kept, and its autograd.
    per_image_count: the mutant that divides each image by its own mask count instead of the batch's."""
    s = o["score"].clone().requires_grad_(True)
    sig, m = o["sigma"][:, None], o["mask"]
    target = -1 / (sig ** 2) * o["noise"]
    count = m.sum(dim=-1) * m.shape[0] if per_image_count else m.sum()
    per = 1 / 2. * (((m * (s - target)) ** 2).sum(dim=-1) * m.shape[-1] / count) * o["sigma"] ** power
    loss = per.mean(dim=0)
    (d,) = torch.autograd.grad(loss, s)
    return {"loss": loss.detach(), "loss_per": per.detach(), "dscore": d}


def dsm_gate(o, power):
    """dscore = scale * mask * mask * (score - target), scale = n_img / count * sigma^p / B taken in double: the
    reciprocal 1 / sigma^2, the product with the noise, the subtraction and the final rounding -- 4 float32 roundings
    of (|score| + |target|) * scale.  loss, loss_per: relative 2^-22 (sums of non-negative terms in double; only the
    per-block partials and the result are rounded to float32)."""
    sig, m = o["sigma"][:, None], o["mask"]
    scale = m.shape[-1] / m.sum() * sig ** power / m.shape[0]
    return 4 * EPS24 * (o["score"].abs() + (o["noise"] / sig ** 2).abs()) * scale * m


def dsm_lattice_bound(n_img):
    """r = score + noise / sigma^2 in units of 1/16, |r| <= 5: r^2 <= 6400 units of 1/256, at most ceil(n_img / 64 / 256)
    * 256 of them in one block's partial."""
    return 6400 * 256 * -(-n_img // (64 * 256))


# ---- the data front end (projection.hip, kitti_view.hip): float64 numpy --------------------------------------------

VIEW_MAX_RANGE = 2057.701
BIN_EDGE_EPS = 1e-9


def bin_edge_guard(points, origin, H, W, eps=BIN_EDGE_EPS):
    """The precondition of every exact comparison with sdp_range_project, from the reference's arithmetic alone: no
    finite point's fractional column or row, moved by +-eps bins, changes its decision (the clamped pixel together
    with in-grid or excluded).  The device's atan2 may differ from libm by a few ulp of at most pi, ~1e-15 rad, i.e.
    ~3e-13 bins at the finest step used (W = 1024); the subtraction and the division add about as much again; 1e-9
    leaves three orders of margin.  A point AT the origin (x = y = 0 after the subtraction) is checked for its row only:
    its azimuth atan2(+-0, +-0) is not computed but fixed by IEEE 754 / C Annex F at exactly 0 or +-pi, and the column
    W/2 - 1/2 it gives (a bin edge, always) is then the same correctly rounded subtraction and division, rounded half
    to even, on every conforming implementation.
    Returns the smallest distance to a deciding bin edge (inf: no such edge)."""
    from oracle import projection_ref as PR
    p = np.asarray(points, np.float64)[:, :3] - np.asarray(origin, np.float64)
    p = p[np.isfinite(p).all(axis=1)]
    hA, vA, hMin, vMin = PR.geometry(H, W)
    at_origin = (p[:, 0] == 0) & (p[:, 1] == 0)
    cf = ((np.arctan2(p[:, 1], p[:, 0]) - hMin) / hA)[~at_origin]
    rf = (np.arctan2(p[:, 2], np.sqrt(np.square(p[:, 0]) + np.square(p[:, 1]))) - vMin) / vA

    def decide(f, n):
        b = np.clip(np.round(f), 0, n - 1)
        return b, b > 0

    margin = np.inf
    for f, n, what in ((cf, W, "column"), (rf, H, "row")):
        b0, in0 = decide(f, n)
        for s in (-eps, eps):
            b, ing = decide(f + s, n)
            bad = (b != b0) | (ing != in0)
            assert not bad.any(), f"{int(bad.sum())} points within {eps} bins of a {what} edge at {H}x{W}: reseed"
        # distance to the nearest half-integer that separates two different clamped bins
        edge = np.floor(f) + 0.5
        deciding = (edge > 0) & (edge < n - 1)
        if deciding.any():
            margin = min(margin, float(np.abs(f - edge)[deciding].min()))
    return margin


def view_finalize_ref(depth, inten, obf, sky, goal_depth, goal_inten, channels, roll, variant, first_view):
    """The post-processing the datasets' __getitem__ apply to the projection's outputs, statement by statement from
    kitti360_im_8Batch.py:221-304 (variant 0), kitti360_im_AllForOne.py:253-353 (1),
    kitti360_im_simultenous_densification.py:230-339 (2, first_view = numberInBatch == 0) and
    kitti360_im_SceneCompletion.py:388-513 (3; goal_depth may be None).  channels == 2 is return_remission;
    roll >= 0 is random_roll with that draw, roll < 0 is random_roll off.  All inputs [H][W].
    Returns (real [C][H][W] float64, notmask [C][H][W] bool, notsky [H][W] bool, goal [C][H][W] float64 or None)."""
    maxRange = VIEW_MAX_RANGE
    real = np.array(depth, np.float64)
    mask = np.array(obf).astype(bool)
    sky = np.array(sky).astype(bool)
    colMax = real.shape[1]
    has_goal = goal_depth is not None
    mask = np.where(real >= maxRange, 1, mask)
    real = np.where(real >= maxRange, 0, real) + 0.0001
    real = np.log2(real + 1) / 6
    real = np.clip(real, 0, 1)
    if has_goal:
        goalDepth = np.where(goal_depth >= maxRange, 0, goal_depth) + 0.0001
        goalDepth = np.clip(np.log2(goalDepth + 1) / 6, 0, 1)
        goalDepth = np.expand_dims(goalDepth, axis=0)
    if roll >= 0:
        real = np.roll(real, roll, axis=1)
        mask = np.roll(mask, roll, axis=1)
        sky = np.roll(sky, roll, axis=1)
    if channels == 2:
        # 8Batch:272 and SceneCompletion:472 run this after the sky shift, AllForOne:276-279 and densification:257-258
        # right here; nothing in between touches the mask except the first-view override below, which comes later in
        # the only variant that has it
        mask = np.where(inten >= 1, 1, mask)      # the intensity is NOT rolled yet
    real = np.expand_dims(real, axis=0)
    mask = np.expand_dims(mask, axis=0)
    if variant == 2 and first_view:
        maskThree = np.zeros_like(real).astype(int)
        maskThree[:, :, :(colMax // 4)] = 1
        mask = np.zeros_like(mask)
        mask = np.logical_or(mask, maskThree)
    sky[1:] = sky[:-1]
    sky[1:] = sky[:-1]
    sky[1:] = sky[:-1]
    if channels == 2:
        intensity = np.where(inten >= 1, 0, inten) + 0.0001
        intensity = np.clip(intensity, 0, 1.0)
        if roll >= 0:
            intensity = np.roll(intensity, roll, axis=1)
        intensity = np.expand_dims(intensity, axis=0)
        if variant == 3:
            real = np.concatenate((real, real), axis=0)
            mask = np.concatenate((mask, np.ones_like(mask)), axis=0)
        else:
            real = np.concatenate((real, intensity), axis=0)
            mask = np.concatenate((mask, mask), axis=0)
        if has_goal:
            goalIntensity = np.where(goal_inten >= 1, 0, goal_inten) + 0.0001
            goalIntensity = np.clip(goalIntensity, 0, 1.0)
            goalDepth = np.concatenate((goalDepth, np.expand_dims(goalIntensity, axis=0)), axis=0)
    return real, np.logical_not(mask), np.logical_not(sky), (goalDepth if has_goal else None)


def view_finalize_inputs(name, H, W):
    """Projection-like inputs that reach every branch of the post-processing: ~10 % set sky bits with rows 0-2 and the
    last three rows among them, a random obf, a third of the depths exactly 2057.701 and some above it, intensities
    with exactly 1.0, 1.5, 0 and 1 - 2^-24 among uniform(0, 1.2) draws."""
    r = rng_for("view_finalize-" + name)
    depth = r.uniform(0.0, 80.0, (H, W))                    # log2(d + 1) / 6 clips to 1 past d = 63
    depth[r.random((H, W)) < 1 / 3] = VIEW_MAX_RANGE
    depth[r.random((H, W)) < 0.04] = VIEW_MAX_RANGE + 1.0
    depth[r.random((H, W)) < 0.02] = 5000.0
    depth[r.random((H, W)) < 0.02] = 0.0
    inten = r.uniform(0.0, 1.2, (H, W))
    for v in (1.0, 1.5, 0.0, 1.0 - 2.0 ** -24):
        inten[r.random((H, W)) < 0.06] = v
    pos = r.permutation(H * W)[:7]                          # each special value at least once, whatever the size
    for k, v in enumerate((1.0, 1.5, 0.0, 1.0 - 2.0 ** -24)):
        inten.flat[pos[k]] = v
    for k, v in enumerate((VIEW_MAX_RANGE, VIEW_MAX_RANGE + 1.0, 70.0)):
        depth.flat[pos[4 + k]] = v
    obf = (r.random((H, W)) < 0.3).astype(np.uint8)
    sky = (r.random((H, W)) < 0.1).astype(np.uint8)
    for row in (0, 1, 2, H - 3, H - 2, H - 1):
        sky[row, r.integers(0, W)] = 1
    gd = r.uniform(0.0, 80.0, (H, W))
    gd[r.random((H, W)) < 0.3] = VIEW_MAX_RANGE
    gi = r.uniform(0.0, 1.2, (H, W))
    gi[r.random((H, W)) < 0.1] = 1.0
    return dict(depth=depth, inten=inten, obf=obf, sky=sky, goal_depth=gd, goal_inten=gi)
