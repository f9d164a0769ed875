"""Per-kernel parity of the implicit-GEMM convolutions: forward, data gradient, weight gradient (MI355X only).

Every launch goes through the sdpk_* test entries (include/sdp_kernels.h) and is compared with the float64 reference
of the same operation (tests/kernel_ref.py).  Lattice operands: EQUALITY, in every mode, whatever the accumulation
order, split count or MFMA shape (a bf16 output tensor: the reference rounded once).  Real operands (only where the
function is inexact: ELU on negatives, elu_grad, bilinear upsample-add, statistics, the fp32x3 split): the derived
elementwise gates of kernel_ref's docstring.  Statistics: kernel_ref.stats_gate.

Dispatch classes the forward plan (net.hip) and the training plan (train.hip) launch at H = 64, W in {128, 256, 384,
1024} (the training plan's data and weight gradients admit W in {256, 1024} only: at 128 / 384 the dilation-4
sub-grid is 16 / 48 wide and conv_dgrad / conv_wgrad reject it).  Channels 128 / 256; tile = rows x columns of a
polyphase sub-grid.

  forward (conv.hip)                      modes            tile     reached by
  F1 conv_launch<2,32,3>                  fp32             8 x 32   every 3x3 with 128 Cout
  F2 conv_launch<1,32,3>                  fp32             4 x 32   every 3x3 with 256 Cout, d = 1 / 2 / 4
  F3 conv_launch<1,64,3,pool>   PELU      fp32|fp32x3|bf16 2 x 64   res2.0 conv2 (fp32 sampling; training)
  F4 conv_launch<1,64,1,pool>   no PELU   fp32x3|bf16      2 x 64   res2.0 shortcut (training)
  F5 conv_launch<1,64,1>        no PELU   all              2 x 64   res2.0 shortcut on the pre-pooled input (sampling)
  F6 conv_launch_nj2<4> 128 Cout          fp32x3|bf16      8 x 16   every 3x3 with 128 Cout
  F7 conv_launch_nj2<4> cpair 256 Cout    fp32x3           8 x 16   every 3x3 with 256 Cout, d = 1 / 2 / 4
  F8 conv_launch_nj2<8> 256 Cout          bf16             8 x 16   the same layers in bf16
  F9 conv_launch_s2 (4x4 stride 2)        fp32x3|bf16      8 x 16o  res2.0 conv2 (sampling)
  F10 IO16 conv_launch<1,64,1,pool> / <1,64,3,pool,PELU> / nj2<4,IO16> (PELU and not; 128 and, as a cpair, 256 Cout)
  prologue / epilogue combinations, as the plans set them: res conv1 (affine+ELU, bias, stats), res conv2 (+ res),
  dilated shortcut (bias), RCU (ELU; + res, epi_elu or stats), CRP (out2 + res2; res), MSF (bias; + res, epi_elu;
  + up, epi_elu; 256 -> 128).
  F7 against F8 (the fp32x3 paired-Cout launch against the bf16 8-wave one): equal on lattice operands.

  data gradient (conv_bwd.hip)            modes            tile     reached by
  D1 dgrad_launch<2,32,1>                 fp32x3|bf16      8 x 32   res2.0 shortcut (1x1)
  D2 dgrad_launch<2,32,3,ZP>              fp32x3|bf16      8 x 32   res2.0 conv2 (zero-padded), dact 3
  D3 dgrad_launch_nj2<4>                  fp32x3|bf16      8 x 16   every circular 3x3 with 128 input channels
  D4 dgrad_launch<1,16,3> (transposed)    fp32x3           8 x 16   every circular 3x3 with 256 input channels
  D5 dgrad_launch_nj2<8>                  bf16             8 x 16   the same layers in bf16
  D6 IO16 dgrad_launch<2,32,1> / <2,32,3,ZP> / nj2<4,IO16> (128 and 256 input channels)
  dact 0 / 1 / 2 / 3, each with and without res (the plans use 0, 1, 1 + res, 3; 2 is the ELU-output form).

  weight gradient (wgrad.hip)             modes            tile     reached by
  W1 conv_wgrad_kernel<64,3,OCC1>         fp32x3           2 x 64   sub-grids 64 n wide
  W2 conv_wgrad_kernel<32,3,OCC1>         fp32x3           4 x 32   the dilation-4 sub-grid at W = 256 (32 wide)
  W3 conv_wgrad_kernel<64,1,OCC1|OCC3>    fp32x3|bf16      2 x 64   res2.0 shortcut
  W4 conv_wgrad_kernel<32,3,OCC3>         bf16             4 x 32   every 3x3
  W5 conv_wgrad_kernel<64,3,OCC2>         bf16             2 x 64   the fallback: sub-grid rows not a multiple of 4
                                                                    (no net shape; kept because it is dispatched)
  W6 conv_wgrad_h16_kernel<32,3> / <64,1> bf16             4 x 32 / 2 x 64   the bf16 tape
  circular and zero-padded, d = 1 / 2 / 4, each prologue, bias gradient, accumulate 0 / 1.

Launch shapes, per class: (a) B = 1 on 2 x 2 tiles -- the grid is no multiple of 8 (conv_kernel.h's plain-blockIdx
branch) and every tile is a corner; where 2 x 2 tiles do give a multiple of 8 (paired Cout blocks, dilation 2) the
sub-grid is 1 x 3 tiles instead; at dilation 4 every grid is a multiple of 16 and the branch cannot be taken.
(b) B = 4 on 2 x 3 tiles (dilation 4: B = 3 on 1 x 3) -- conv_strip_w stops at 1 because 3 is odd, there are edge
and interior columns, the grid is a multiple of 8; F7 / F8 also on 2 x 6 tiles (strip width 2 of 6 columns), and
the 16-wide data gradients only there: conv_dgrad asks for a sub-grid 32 n wide, as the weight gradient does, so it
admits 16-wide tiles in pairs only (which is also why the training plan rejects W = 128 and 384).  Real
operands run on (a) only.  Weight gradient: (b) has at least 3 x 3 tiles of the kernel's own tile shape, so interior
tiles (their own load path in wgrad.hip) beside edge and corner ones -- dilation 4: a third shape, B = 1 on 3 x 3; (a)
and (b) give different wgrad_splits (asserted through the query); "multi" shapes have more tiles than splits, unevenly
(a workgroup walks several tiles); B = 1 on 1 x 3 tiles makes the 128 -> 128 grid 3 x 4 workgroups, no multiple of 8
(the 1x1 and 256-channel grids are multiples of 8 whatever the shape).  tests/test_kernel_ref_cpu.py asserts on this
table that every weight-gradient kernel class has a case with an interior tile and one with several tiles per
workgroup.  The forward and data-gradient (b) shapes have edge and corner tiles and interior COLUMNS only (2 tile
rows: those kernels have one load path, wrap or clamp, for every tile).

Not covered, on purpose: the weight-gradient instantiations that no admitted net shape reaches (wgrad OCC 2 <64,1>
and <32,3>).  Every forward and data-gradient kernel that is built is a row of conv_inst.hip's table, and every row is
one of the classes F1 - F10 / D1 - D6 above.

Rejected (the REJECTED table: a non-zero return, the condition in sdp_last_error(), the output untouched): what used
to reach kernels outside those classes, or no fitting kernel at all.  A NON-pooled zero-padded 3x3 (circular = 0,
pool = 0, s2 = 0; only the pooled and 4x4 stride-2 kernels are built with zero padding, the others clamp at the
border); in the bf16 modes a non-pooled 3x3, and any circular 3x3 data gradient, whose sub-grid does not tile into
8 x 16; a pooled 3x3 without a prologue; a pooled 1x1 with a prologue or in fp32; a non-pooled 1x1 with a prologue.
"""
import functools

import pytest
import torch

import kernel_lib as KL
import kernel_ref as KR
from kernel_ref import PRO_AFFINE_ELU as AFF
from kernel_ref import PRO_ELU as ELU
from kernel_ref import PRO_NONE as NONE
from kernel_ref import Case

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


# ------------------------------------------------------------------------------------------------ case tables
def _grid_a(d, wg_per_tile):
    """Tile rows x columns of launch shape (a): the first whose grid.x is no multiple of 8."""
    for r, c in ((2, 2), (1, 3), (3, 3)):
        if (r * c * d * d * wg_per_tile) % 8:
            return r, c
    return 2, 2


def _shapes(tr, tc, d=1, wg_per_tile=1, six=False):
    """(tag, B, H, W) of the launch shapes of a class with tr x tc tiles of its dilation-d sub-grid."""
    r, c = _grid_a(d, wg_per_tile)
    out = [("a", 1, r * tr * d, c * tc * d), ("b", 4, 2 * tr * d, 3 * tc * d)]
    if d == 4:      # 16 phases: one tile row and B = 3 keep the float64 reference of (b) to a few GFLOP
        out[1] = ("b", 3, tr * d, 3 * tc * d)
    if six:
        out.append(("b6", 4, 2 * tr * d, 6 * tc * d))
    return out


# prologue / epilogue combinations of the plans (forward)
RES1 = dict(pro=AFF, bias=True, stats=True)
RES2 = dict(pro=AFF, bias=True, res=True, stats=True)
SHORT = dict(pro=NONE, bias=True)
RCU1 = dict(pro=ELU)
RCU2E = dict(pro=ELU, res=True, epi_elu=True)
RCU2S = dict(pro=ELU, res=True, stats=True)
CRP0 = dict(pro=NONE, out2=True)
CRP1 = dict(pro=NONE, res=True)
MSFE = dict(pro=NONE, bias=True, res=True, epi_elu=True)
MSFU = dict(pro=NONE, bias=True, up=True, epi_elu=True, real=True)
REAL = dict(real=True)


def _fwd(cls, modes, tr, tc, cin, cout, opts, d=1, wg=1, six=False, **kw):
    out = []
    for oname, o in opts.items():
        for tag, B, H, W in _shapes(tr, tc, d, wg, six):
            if o.get("real") and tag != "a":
                continue
            name = f"{cls}-{cin}to{cout}-d{d}-{oname}-{tag}"
            out.append((Case(name, "fwd", B, H, W, cin, cout, dil=d, **{**kw, **o}), modes))
    return out


ALL3 = ("fp32", "fp32x3", "bf16")
B16 = ("fp32x3", "bf16")
O128 = dict(res1=RES1, res2=RES2, rcu1=RCU1, rcu2e=RCU2E, rcu2s=RCU2S, crp0=CRP0, crp1=CRP1, msf=SHORT, msfe=MSFE,
            msfu=MSFU, res2_real={**RES2, **REAL}, rcu2e_real={**RCU2E, **REAL})
O256 = dict(res1=RES1, res2=RES2, rcu1=RCU1, rcu2e=RCU2E, crp0=CRP0, crp1=CRP1, msfe=MSFE,
            res2_real={**RES2, **REAL}, rcu2e_real={**RCU2E, **REAL})
ODIL = dict(res1=RES1, res2=RES2, short=SHORT, res2_real={**RES2, **REAL})
POOL3 = dict(res2=RES2, res2_real={**RES2, **REAL})

FWD = (
    _fwd("F1", ("fp32",), 8, 32, 128, 128, O128)
    + _fwd("F1", ("fp32",), 8, 32, 256, 128, dict(msf=SHORT, msfe=MSFE))
    + _fwd("F2", ("fp32",), 4, 32, 256, 256, O256)
    + _fwd("F2", ("fp32",), 4, 32, 256, 256, ODIL, d=2)
    + _fwd("F2", ("fp32",), 4, 32, 256, 256, ODIL, d=4)
    + _fwd("F3", ALL3, 2, 64, 128, 256, POOL3, circular=False, pool=True)
    + _fwd("F4", B16, 2, 64, 128, 256, dict(short=SHORT), ks=1, circular=False, pool=True)
    + _fwd("F5", ALL3, 2, 64, 128, 256, dict(short=SHORT), ks=1, circular=False)
    + _fwd("F6", B16, 8, 16, 128, 128, O128)
    + _fwd("F6", B16, 8, 16, 256, 128, dict(msf=SHORT, msfe=MSFE))
    # F7 (fp32x3: two workgroups per tile) and F8 (bf16: one 8-wave workgroup) share their cases
    + _fwd("F78", B16, 8, 16, 256, 256, O256, wg=2, six=True)
    + _fwd("F78", B16, 8, 16, 256, 256, ODIL, d=2)     # (a) 1 x 3 tiles: 12 workgroups in bf16, 24 in fp32x3
    + _fwd("F78", B16, 8, 16, 256, 256, ODIL, d=4, wg=2)
    + _fwd("F9", B16, 16, 32, 128, 256, POOL3, wg=2, circular=False, s2=True)
    + _fwd("F10", ("bf16",), 2, 64, 128, 256, dict(short=SHORT), ks=1, circular=False, pool=True, io16=True)
    + _fwd("F10", ("bf16",), 2, 64, 128, 256, POOL3, circular=False, pool=True, io16=True)
    + _fwd("F10", ("bf16",), 8, 16, 128, 128, dict(res2=RES2, rcu2e=RCU2E, crp0=CRP0, msfu=MSFU, res2_real={**RES2, **REAL}),
           io16=True)
    + _fwd("F10", ("bf16",), 8, 16, 256, 256, dict(res2=RES2, crp0=CRP0, msfe=MSFE), wg=2, io16=True)
    + _fwd("F10", ("bf16",), 8, 16, 256, 256, dict(res2=RES2, short=SHORT), d=2, wg=2, io16=True)
)


def _dgrad(cls, modes, tr, tc, cin, cout, opts, d=1, **kw):
    """cin / cout: the FORWARD conv's (dx has cin channels)."""
    out = []
    for oname, o in opts.items():
        shapes = _shapes(tr, tc, d)
        if tc == 16:
            # conv_dgrad asks for a sub-grid 32 n wide (as the weight gradient), so 16-wide tiles come in pairs: (b) has
            # six tile columns (strip width 2), (a) 2 x 2 tiles also under a dilation (no grid off a multiple of 8 then)
            shapes = [("a", 1, 2 * tr * d, 2 * tc * d), ("b", 4 if d < 4 else 3, (2 if d == 1 else 1) * tr * d, 6 * tc * d)]
        for tag, B, H, W in shapes:
            if (o.get("real") and tag != "a") or (d == 4 and tag == "b" and oname != "dact3"):
                continue      # (dilation 4, (b): 43 GFLOP of float64 reference, once)
            name = f"{cls}-{cin}to{cout}-d{d}-{oname}-{tag}"
            out.append((Case(name, "dgrad", B, H, W, cin, cout, dil=d, **{**kw, **o}), modes))
    return out


DACT = {f"dact{k}{'res' if r else ''}{'_real' if real else ''}": dict(dact=k, res=r, real=real)
        for k in (0, 1, 2, 3) for r in (False, True) for real in (False, True) if not (real and (k == 0 or not r))}
DACT["dact3_real"] = dict(dact=3, res=False, real=True)
DPLAN = {k: DACT[k] for k in ("dact0", "dact1res", "dact3", "dact3_real", "dact1res_real")}

DGRAD = (
    _dgrad("D1", B16, 8, 32, 128, 256, dict(dact0=DACT["dact0"], dact0res=DACT["dact0res"]), ks=1, circular=False)
    + _dgrad("D2", B16, 8, 32, 128, 256, dict(dact3=DACT["dact3"], dact3_real=DACT["dact3_real"]), circular=False)
    + _dgrad("D3", B16, 8, 16, 128, 128, DACT)
    + _dgrad("D45", B16, 8, 16, 256, 256, DACT)
    + _dgrad("D45", B16, 8, 16, 256, 128, dict(dact0=DACT["dact0"]))
    + _dgrad("D45", B16, 8, 16, 256, 256, DPLAN, d=2)
    + _dgrad("D45", B16, 8, 16, 256, 256, DPLAN, d=4)
    + _dgrad("D6", ("bf16",), 8, 32, 128, 256, dict(dact0=DACT["dact0"]), ks=1, circular=False, io16=True)
    + _dgrad("D6", ("bf16",), 8, 32, 128, 256, dict(dact3=DACT["dact3"]), circular=False, io16=True)
    + _dgrad("D6", ("bf16",), 8, 16, 128, 128, DPLAN, io16=True)
    + _dgrad("D6", ("bf16",), 8, 16, 256, 256, DPLAN, io16=True)
    + _dgrad("D6", ("bf16",), 8, 16, 256, 256, dict(dact3=DACT["dact3"]), d=4, io16=True)
)


def _wgrad(cls, modes, tr, tc, cin, cout, opts, d=1, odd=False, rows_a=2, rows_b=None, multi=None, **kw):
    """Shapes: (a) B = 1 on corner tiles only; (b) B = 4 on at least 3 x 3 tiles of the kernel's own tile shape (64-wide
    classes: 4 x 3 unless rows_b says otherwise), so that it has interior tiles -- the weight-gradient kernels load
    those through a path of their own (wgrad.hip `interior`); dilation 4: (b) B = 3 on 1 x 3 tiles and "int" B = 1 on
    3 x 3; "odd": B = 1 on 1 x 3 tiles (a grid off a multiple of 8 for 128 -> 128); "multi" = (B, H, W): more tiles than
    wgrad_splits, unevenly, so a workgroup accumulates over several tiles and stages the next one."""
    out = []
    if rows_b is None:
        rows_b = 4 if tc == 64 else 3
    # 64-wide tiles need a sub-grid 64 n wide, 32-wide ones 32 n with n odd (conv_wgrad picks 64 where it divides)
    shapes = [("a", 1, rows_a * tr * d, (2 if tc == 64 else 3) * tc * d), ("b", 4, rows_b * tr * d, 3 * tc * d)]
    if d == 4:
        shapes = [("a", 1, tr * d, tc * d), ("b", 3, tr * d, 3 * tc * d), ("int", 1, 3 * tr * d, 3 * tc * d)]
    if odd:
        shapes.append(("odd", 1, tr * d, 3 * tc * d))
    if multi:
        shapes.append(("multi",) + tuple(multi))
    for oname, o in opts.items():
        for tag, B, H, W in shapes:
            if (o.get("real") and tag != "a") or (tag in ("int", "multi") and oname != next(iter(opts))):
                continue      # ("int" and "multi": the first option set only)
            name = f"{cls}-{cin}to{cout}-d{d}-{oname}-{tag}"
            out.append((Case(name, "wgrad", B, H, W, cin, cout, dil=d, **{**kw, **o}), modes))
    return out


def wgrad_kernel(c: Case, mode):
    """(kernel class, has an interior tile, a workgroup walks several tiles) of a weight-gradient case: conv_wgrad's
    dispatch and wgrad_splits restated (the GPU test asserts the split count against the library's)."""
    d, Hs, Ws = c.dil, c.H // c.dil, c.W // c.dil
    if c.io16:
        name, tr, tc = ("h16<64,1>", 2, 64) if c.ks == 1 else ("h16<32,3>", 4, 32)
    elif c.ks == 1:
        name, tr, tc = f"<64,1,OCC{1 if mode == 'fp32x3' else 3}>", 2, 64
    elif mode == "bf16":
        name, tr, tc = ("<32,3,OCC3>", 4, 32) if (Ws % 32 == 0 and Hs % 4 == 0) else ("<64,3,OCC2>", 2, 64)
    else:
        name, tr, tc = ("<64,3,OCC1>", 2, 64) if Ws % 64 == 0 else ("<32,3,OCC1>", 4, 32)
    interior = c.ks == 1 or (Hs // tr >= 3 and Ws // tc >= 3)
    return name, interior, wgrad_total(c) > wgrad_splits(c)


def wgrad_total(c: Case):
    return c.B * c.H * c.W // 128


def wgrad_splits(c: Case):
    blocks = (c.Cin // 32) * (c.Cout // 128)
    return max(1, min((512 + blocks - 1) // blocks, wgrad_total(c)))


WRES = dict(pro=AFF, bias=True)
WOPT = dict(res=WRES, res_acc={**WRES, "accumulate": True}, rcu=dict(pro=ELU), crp=dict(pro=NONE),
            msf=dict(pro=NONE, bias=True), res_real={**WRES, **REAL}, rcu_real=dict(pro=ELU, real=True))
WDIL = dict(res=WRES, short=dict(pro=NONE, bias=True), res_real={**WRES, **REAL})

WGRAD = (
    # 2 x 64 tiles in fp32x3 (W1); the bf16 mode takes 4 x 32 tiles on the same shapes (W4: H a multiple of 4)
    _wgrad("W14", B16, 2, 64, 128, 128, WOPT, odd=True, multi=(4, 24, 192))
    + _wgrad("W14", B16, 2, 64, 256, 256, dict(res=WRES, crp=dict(pro=NONE)))
    + _wgrad("W14", B16, 2, 64, 256, 128, dict(msf=dict(pro=NONE, bias=True)))
    + _wgrad("W14", B16, 2, 64, 256, 256, WDIL, d=2, rows_b=2)
    + _wgrad("W14", B16, 2, 64, 128, 256, dict(res=WRES, res_real={**WRES, **REAL}), circular=False)
    # 4 x 32 tiles in both modes (W2, W4): sub-grids 32 n wide, n odd
    + _wgrad("W24", B16, 4, 32, 128, 128, dict(res=WRES, rcu=dict(pro=ELU)), odd=True)
    + _wgrad("W24", B16, 4, 32, 128, 256, dict(res=WRES), circular=False)
    + _wgrad("W24", B16, 4, 32, 256, 256, WDIL, d=4)
    + _wgrad("W3", B16, 2, 64, 128, 256, dict(short=dict(pro=NONE, bias=True), short_acc=dict(pro=NONE, bias=True, accumulate=True),
                                              short_real=dict(pro=NONE, bias=True, real=True)), ks=1, circular=False,
             multi=(4, 16, 192))
    # sub-grid rows 6 = 2 mod 4: the bf16 mode falls back to OCC 2 on 2 x 64 tiles (fp32x3: W1 again)
    + _wgrad("W5", B16, 2, 64, 128, 128, dict(res=WRES, crp=dict(pro=NONE), res_real={**WRES, **REAL}), rows_a=3, rows_b=3)
    + _wgrad("W5", B16, 2, 64, 256, 256, dict(res=WRES), rows_a=3, rows_b=3)
    + _wgrad("W6", ("bf16",), 4, 32, 128, 128, dict(res=WRES, res_acc={**WRES, "accumulate": True}, rcu=dict(pro=ELU),
                                                    crp=dict(pro=NONE), res_real={**WRES, **REAL}), odd=True, io16=True,
             multi=(4, 24, 192))
    + _wgrad("W6", ("bf16",), 4, 32, 256, 256, WDIL, d=2, io16=True)
    + _wgrad("W6", ("bf16",), 4, 32, 128, 256, dict(res=WRES), circular=False, io16=True)
    + _wgrad("W6", ("bf16",), 2, 64, 128, 256, dict(short=dict(pro=NONE, bias=True)), ks=1, circular=False, io16=True,
             multi=(4, 16, 192))
)

CASES = FWD + DGRAD + WGRAD
PARAMS = [pytest.param(c, m, id=f"{c.name}-{m}") for c, modes in CASES for m in modes]


# ------------------------------------------------------------------------------------------------ GPU runner
@functools.lru_cache(maxsize=4)
def _operands(c: Case):
    return KR.make_operands(c)


@functools.lru_cache(maxsize=8)
def _reference(c: Case, mode_key):
    o = _operands(c)
    ref = KR.reference(c, o, mode_key)
    return KR.finish_io16(c, ref), KR.gate(c, o, mode_key, ref)


def _act(c, t):
    """NCHW float64 -> the NHWC CUDA tensor of the launch (bf16 on the bf16 tape)."""
    return KR.nhwc(t).to(torch.bfloat16 if c.io16 else torch.float32).to(DEV)


def _back(t):
    return KR.nchw(t.to(torch.float64).cpu())


def _ss(scale, shift):
    return torch.stack([scale, shift], dim=-1).to(torch.float32).contiguous().to(DEV)   # [B][C][2]


def _new(c, B, H, W, C):
    return torch.full((B, H, W, C), float("nan"), dtype=torch.bfloat16 if c.io16 else torch.float32, device=DEV)


def run_case(c: Case, mode, o=None, outputs=None):
    """Launch case c in mode `mode` (on the operands o, else the case's own); returns {name: NCHW float64 CPU
    tensor} (+ 'stats': [B][T][C][2], 'cnt').  outputs: a list that receives the NaN-filled forward / data-gradient
    output tensor before the launch (for the callers that expect the launch to be refused)."""
    o = _operands(c) if o is None else o
    L, m = KL.lib(), KR.MODES[mode]
    f32 = lambda t: t.to(torch.float32).contiguous().to(DEV)
    w = f32(o["w"])
    keep, res = [w], {}
    if c.kind == "wgrad":
        g = KL.Wgrad()
        x, dy = _act(c, o["x"]), _act(c, o["dy"])
        ss = _ss(o["scale"], o["shift"]) if c.pro == AFF else KL.ident_ss(DEV)
        S = L.sdpk_wgrad_splits(c.B, c.H, c.W, c.dil, c.Cin, c.Cout, c.ks)
        n = L.sdpk_wgrad_part_floats(S, c.Cin, c.Cout, c.ks)
        part = torch.empty(n, dtype=torch.float32, device=DEV)
        bpart = torch.empty(S * c.Cout, dtype=torch.float32, device=DEV)
        dw = f32(o["w0"]) if c.accumulate else torch.full(tuple(o["w"].shape), float("nan"), device=DEV)
        db = f32(o["b0"]) if c.accumulate else torch.full((c.Cout,), float("nan"), device=DEV)
        g.in_, g.pro_ss, g.ss_bstride, g.pro_mode, g.dy = x.data_ptr(), ss.data_ptr(), 2 * c.Cin if c.pro == AFF else 0, c.pro, dy.data_ptr()
        g.part, g.part_floats, g.bpart = part.data_ptr(), n, bpart.data_ptr()
        g.B, g.H, g.W, g.Cin, g.Cout, g.dil, g.circular = c.B, c.H, c.W, c.Cin, c.Cout, c.dil, int(c.circular)
        KL.check(L.sdpk_conv_wgrad(m, g, c.ks, dw.data_ptr(), db.data_ptr() if c.bias else None, int(c.accumulate),
                                   int(c.io16), KL.stream()), c.name)
        torch.cuda.synchronize()
        res["dw"] = dw.to(torch.float64).cpu()
        if c.bias:
            res["db"] = db.to(torch.float64).cpu()
        res["splits"] = S
        return res
    a = KL.Conv()
    if c.kind == "fwd":
        packing = KL.PACK_POOL4X4 if c.s2 else (KL.PACK_FRAG if mode == "fp32" else KL.PACK_FRAG16)
        cin, cout, x = c.Cin, c.Cout, _act(c, o["x"])
        ss = _ss(o["scale"], o["shift"]) if c.pro == AFF else KL.ident_ss(DEV)
        a.ss_bstride, a.pro_mode = (2 * c.Cin if c.pro == AFF else 0), c.pro
    else:
        packing, cin, cout, x, ss = KL.PACK_DFRAG16, c.Cout, c.Cin, _act(c, o["dy"]), KL.ident_ss(DEV)
    pk = KL.pack_weights(w, m, packing)
    Ho, Wo = c.out_hw()
    out = _new(c, c.B, Ho, Wo, cout)
    if outputs is not None:
        outputs.append(out)
    keep += [x, ss, pk, out]
    a.in_, a.out, a.pro_ss = x.data_ptr(), out.data_ptr(), ss.data_ptr()
    if packing == KL.PACK_FRAG:
        a.wf = pk.data_ptr()
    else:
        a.wf16 = pk.data_ptr()
    for key, field in (("res", "res"), ("res2", "res2"), ("up", "up"), ("aux", "aux")):
        if key in o:
            t = _act(c, o[key])
            keep.append(t)
            setattr(a, field, t.data_ptr())
    if c.kind == "fwd" and c.bias:
        b = f32(o["bias"])
        keep.append(b)
        a.bias = b.data_ptr()
    out2 = None
    if c.out2:
        out2 = _new(c, c.B, Ho, Wo, cout)
        a.out2 = out2.data_ptr()
    if c.dact == 3:
        es = _ss(o["escale"], o["eshift"])
        keep.append(es)
        a.epi_ss = es.data_ptr()
    stats = None
    if c.stats:
        T, cnt = (Ho * Wo // 128, 128) if not c.pool else (c.H * c.W // 128, 32)
        stats = torch.full((c.B, T, cout, 2), float("nan"), device=DEV)
        a.stats = stats.data_ptr()
    a.B, a.H, a.W, a.Cin, a.Cout = c.B, c.H, c.W, cin, cout
    a.dil, a.circular, a.epi_elu, a.dact, a.io16, a.s2 = c.dil, int(c.circular), int(c.epi_elu), c.dact, int(c.io16), int(c.s2)
    if c.kind == "fwd":
        KL.check(L.sdpk_conv_mfma(m, a, c.ks, int(c.pool), KL.stream()), c.name)
    else:
        KL.check(L.sdpk_conv_dgrad(m, a, c.ks, KL.stream()), c.name)
    torch.cuda.synchronize()
    res["out"] = _back(out)
    if out2 is not None:
        res["out2"] = _back(out2)
    if stats is not None:
        res["stats"], res["cnt"] = stats.cpu(), cnt
    return res


def compare(c: Case, mode, got, ref, gate):
    for k, r in ref.items():
        if k == "db" and not c.bias:
            continue
        g = got[k]
        assert torch.isfinite(g).all(), f"{c.name} {mode} {k}: unwritten or non-finite elements"
        err = (g - r).abs()
        print(f"{c.name} {mode} {k}: max|gpu - ref| = {err.max().item():.3e}, max gate = {gate[k].max().item():.3e}, "
              f"max|ref| = {r.abs().max().item():.3e}")
        if not c.real and gate[k].max().item() == 0.0:
            assert torch.equal(g, r), f"{c.name} {mode} {k}: {int((g != r).sum())} of {r.numel()} elements differ"
        else:
            bad = err > gate[k]
            assert not bad.any(), f"{c.name} {mode} {k}: {int(bad.sum())} elements over the gate, worst {err.max().item():.3e}"
    if "stats" in got:
        mean, var = KR.combine_stats(got["stats"], got["cnt"])
        y = ref["out"]
        gm, gv = KR.stats_gate(y, float(gate["out"].max()) + (2.0 ** -8 * float(y.abs().max()) if c.io16 else 0.0))
        em, ev = (mean - y.mean(dim=(2, 3))).abs(), (var - y.var(dim=(2, 3), unbiased=False)).abs()
        print(f"{c.name} {mode} stats: mean err {em.max().item():.3e} (gate {gm.max().item():.3e}), "
              f"var err {ev.max().item():.3e} (gate {gv.max().item():.3e})")
        assert (em <= gm).all() and (ev <= gv).all()


@pytest.mark.parametrize("c,mode", PARAMS)
def test_conv_kernel_matches_float64_reference(c, mode):
    """Lattice cases: equality.  Real cases: the derived elementwise gate (kernel_ref docstring)."""
    assert c.real or c.lattice_bound() < 2 ** 24
    ref, gate = _reference(c, mode if c.real else "exact")
    compare(c, mode, run_case(c, mode), ref, gate)


def test_paired_cout_launch_equals_the_8_wave_one():
    """F7 (fp32x3: two 4-wave 128-Cout workgroups per tile, dealt as pairs) against F8 (bf16: one 8-wave workgroup):
    the same lattice case, so the two outputs are equal element for element.  The statistics are float32 means and
    sums of squares, exact in neither: each within kernel_ref.stats_gate of the reference, so within twice that of
    each other."""
    c = next(c for c, _ in FWD if c.name == "F78-256to256-d1-res2-b6")
    a, b = run_case(c, "fp32x3"), run_case(c, "bf16")
    assert torch.equal(a["out"], b["out"])
    (ma, va), (mb, vb) = KR.combine_stats(a["stats"], a["cnt"]), KR.combine_stats(b["stats"], b["cnt"])
    gm, gv = KR.stats_gate(a["out"])
    assert ((ma - mb).abs() <= 2 * gm).all() and ((va - vb).abs() <= 2 * gv).all()


def test_weight_gradient_split_counts_differ_between_the_launch_shapes():
    L = KL.lib()
    by = {}
    for c, _ in WGRAD:
        by.setdefault(c.name.rsplit("-", 1)[0], {})[c.name.rsplit("-", 1)[1]] = L.sdpk_wgrad_splits(
            c.B, c.H, c.W, c.dil, c.Cin, c.Cout, c.ks)
    for c, _ in WGRAD:
        assert L.sdpk_wgrad_splits(c.B, c.H, c.W, c.dil, c.Cin, c.Cout, c.ks) == wgrad_splits(c), c.name
    pairs = [v for v in by.values() if "a" in v and "b" in v]
    assert pairs and all(v["a"] != v["b"] for v in pairs), by


# ------------------------------------------------------------------------------------------------ error paths
def _launch_error(c: Case, mode, needle):
    with pytest.raises(KL.KernelError) as e:
        run_case(c, mode)
    assert needle in str(e.value), str(e.value)


# Combinations no kernel is built for (conv_inst.hip's table): the launch is refused, with the unmet condition in
# sdp_last_error(), and nothing is written.  Smallest shapes that pass every earlier check; buffers at full size and
# valid packed weights, so a launch that wrongly went ahead would stay inside them.
REJECTED = (
    # a non-pooled zero-padded 3x3: the non-pooled kernels clamp at the border
    (Case("rej-fwd-zp", "fwd", 1, 16, 32, 128, 128, circular=False), ALL3, "needs circular padding"),
    # tiles 4 x 32 but not 8 x 16: ran on the retired 32-wide tiles of the bf16 modes (data gradient: 64-wide)
    (Case("rej-fwd-4x32", "fwd", 1, 4, 32, 256, 256), B16, "8 x 16 pixel tile"),
    (Case("rej-dgrad-4x64", "dgrad", 1, 4, 64, 256, 256), B16, "8 x 16 tiles of a circular 3x3"),
    # prologues the pooled and 1x1 kernels are not built with
    (Case("rej-pool3-none", "fwd", 1, 4, 64, 128, 256, circular=False, pool=True, pro=NONE), ALL3, "pooled 3x3 needs an ELU prologue"),
    (Case("rej-pool1-elu", "fwd", 1, 4, 64, 128, 256, ks=1, circular=False, pool=True, pro=ELU), B16, "pooled 1x1 needs"),
    (Case("rej-pool1-fp32", "fwd", 1, 4, 64, 128, 256, ks=1, circular=False, pool=True), ("fp32",), "pooled 1x1 needs"),
    (Case("rej-1x1-elu", "fwd", 1, 2, 64, 128, 256, ks=1, circular=False, pro=ELU), ALL3, "non-pooled 1x1 takes no prologue"),
)


@pytest.mark.parametrize("c,mode,needle", [pytest.param(c, m, needle, id=f"{c.name}-{m}")
                                           for c, modes, needle in REJECTED for m in modes])
def test_unbuilt_combinations_are_rejected(c, mode, needle):
    outputs = []
    with pytest.raises(KL.KernelError) as e:      # raised on a non-zero return, with sdp_last_error()
        run_case(c, mode, outputs=outputs)
    assert needle in str(e.value), str(e.value)
    torch.cuda.synchronize()
    assert len(outputs) == 1 and torch.isnan(outputs[0]).all(), f"{c.name} {mode}: the output was written"


def test_launchers_reject_what_their_kernels_cannot_index():
    # a sub-grid that does not tile: 8 x 24 (16-wide tiles need a multiple of 16, 32-wide ones of 32)
    _launch_error(Case("err-fwd-tile", "fwd", 1, 8, 24, 128, 128), "fp32x3", "not divisible")
    _launch_error(Case("err-dgrad-tile", "dgrad", 1, 8, 24, 128, 128), "bf16", "not divisible")
    _launch_error(Case("err-wgrad-tile", "wgrad", 1, 8, 48, 128, 128), "bf16", "not divisible")
    # zero padding with a dilation, channels off the block size, the bf16 tape outside bf16 mode
    _launch_error(Case("err-fwd-zp-dil", "fwd", 1, 16, 32, 128, 128, dil=2, circular=False), "bf16", "zero padding")
    _launch_error(Case("err-fwd-cout", "fwd", 1, 8, 16, 128, 64), "bf16", "Cout%128")
    _launch_error(Case("err-fwd-io16", "fwd", 1, 8, 16, 128, 128, io16=True), "fp32x3", "io16")
    _launch_error(Case("err-wgrad-h16", "wgrad", 1, 2, 64, 128, 128, io16=True), "bf16", "4 x 32")
