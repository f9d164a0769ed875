"""Per-kernel parity of the kernels at the two ends of the score net (MI355X only; through the sdpk_* entries and, for
the DSM loss and the stand-alone Langevin step, the stable sdp_* ones).

  kernel                                           forms                              reference (float64, kernel_ref)
  begin_conv_kernel / begin_conv_mfma_kernel       fp32 | fp32x3 | bf16 | bf16 + bf16 out   input_prep + zero-padded conv
  end_conv_kernel / end_conv_mfma_kernel           fp32 | fp32x3 | bf16 | bf16 + bf16 in    IN++ affine + ELU + conv, / sigma
  end conv + fused Langevin update                 fp32 | fp32x3 | bf16               the plain launch, then sdp_langevin_step
  begin_wgrad_kernel + sum_rows                    float | bf16 dy                    autograd of the begin conv
  end_dgrad_kernel, end_wgrad_kernel + sum_rows    float | bf16 o, g                  autograd of the end conv
  dsm_mask_sum / dsm_grad / dsm_final              --                                 R.dsm_loss and its autograd

Lattice operands: EQUALITY with the float64 reference in every form (a bf16 output: the reference rounded once).  Real
operands: kernel_ref's derived gates (K = 37, 9 * 128 + 1, 18, B H W).  Every output buffer is NaN-filled before the
launch and must be finite everywhere after it.

Shapes: the smallest at which each kernel can still go wrong.
  begin conv (tile 1 row x 128 px; persistent, grid = min(tiles, 768) fp32 / min(tiles, 512) MFMA):
    a 1 x 3 x 128     top, middle and bottom rows; the one tile of a row holds both side borders
    b 3 x 5 x 384     an interior tile column; more than one image
    p 3 x 33 x 1536   1188 tiles: more than 768 and than 2 x 512, a multiple of neither -- fp32 workgroups walk 1 - 2
                      tiles, MFMA ones 2 - 3, successive tiles of a workgroup lie in different images (the prefetch
                      hand-off, the vmcnt(17) wait, the clamp past the last tile)
    q 4 x 33 x 1536   1584 tiles, more than 2 x 768: every fp32 workgroup walks 2 - 3 tiles (fp32 form only)
  end conv: MFMA (16 x 32 tiles) a 1 x 16 x 64 (corner tiles only), b 3 x 48 x 96 (3 x 3 tiles: an interior one; W no
    multiple of 64); direct (4 x 64 tiles) a 1 x 4 x 64, b 3 x 12 x 192 (3 x 3 tiles); fp32x3 at 3 x 12 x 192 falls
    back to the direct kernel (H % 16 != 0): bit-identical to the fp32 call
  begin_wgrad (block 8 rows x 64 px): a 1 x 8 x 64, b 3 x 24 x 192 (an interior block, 27 partials)
  end_conv_backward (data gradient: 1 row x 64 px; weight gradient: 16 rows x 32 px, 3-slot row ring):
    a 1 x 16 x 64, b 3 x 48 x 192 (the ring crosses block boundaries above and below, 3 x 6 blocks)
  dsm_loss: n_img 1600 (below one pass of the 64 x 256 threads), 32768 (exactly two), 2 * 7 * 1171 (a ragged tail)
"""
import dataclasses
import functools

import pytest
import torch

import kernel_lib as KL
import kernel_ref as KR
import test_gpu_kernels_aux as TA
from kernel_ref import Head

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F64 = torch.float64
NAN = float("nan")

# the launchers' grid caps (aux.hip begin_conv): 256 CUs x BC_WG_PER_CU = 3 / SDP_BM_WG = 2 workgroups
BEGIN_CAP_FP32, BEGIN_CAP_MFMA = 256 * 3, 256 * 2
BEGIN_SHAPES = {"a": (1, 3, 128), "b": (3, 5, 384), "p": (3, 33, 1536), "q": (4, 33, 1536)}
_tiles = lambda s: s[0] * s[1] * (s[2] // 128)
# a retuned cap must fail here, loudly, instead of silently losing the multi-tile coverage
assert _tiles(BEGIN_SHAPES["p"]) > BEGIN_CAP_FP32 and _tiles(BEGIN_SHAPES["p"]) > 2 * BEGIN_CAP_MFMA
assert _tiles(BEGIN_SHAPES["q"]) > 2 * max(BEGIN_CAP_FP32, BEGIN_CAP_MFMA)
assert all(_tiles(BEGIN_SHAPES[k]) % cap for k in "pq" for cap in (BEGIN_CAP_FP32, BEGIN_CAP_MFMA))
# an image has no more tiles than a workgroup's stride: its successive tiles lie in different images
assert all(_tiles(BEGIN_SHAPES[k]) // BEGIN_SHAPES[k][0] <= BEGIN_CAP_MFMA for k in "pq")

FORMS = [("fp32", False), ("fp32x3", False), ("bf16", False), ("bf16", True)]      # (mode, h16)
FORM_ID = lambda f: f[0] + ("-h16" if f[1] else "")


def f32(t):
    return t.to(torch.float32).contiguous().to(DEV)


def act(t, h16=False):
    """NCHW float64 -> the NHWC CUDA tensor of the launch (bf16 on the bf16 tape)."""
    return KR.nhwc(t).to(torch.bfloat16 if h16 else torch.float32).to(DEV)


def back(t):
    return KR.nchw(t.to(F64).cpu())


def ss_of(o):
    return torch.stack([o["scale"], o["shift"]], dim=-1).to(torch.float32).contiguous().to(DEV)      # [B][C][2]


@functools.lru_cache(maxsize=4)
def _operands(c: Head):
    return KR.head_operands(c)


@functools.lru_cache(maxsize=4)
def _reference(c: Head, mode_key):
    """The float64 reference, shared by the forms of a case (ref_and_gate picks the key: the operands of a real case on
    the bf16 tape are rounded, so it keeps its own)."""
    return KR.head_reference(c, _operands(c), mode_key)


def ref_and_gate(c: Head, mode):
    key = c if (c.real and c.op != "begin") else dataclasses.replace(c, h16=False)   # begin: h16 is the OUTPUT only
    o = _operands(key)
    ref = KR.head_finish(c, _reference(key, mode if c.real else "exact"))
    return o, ref, KR.head_gate(c, o, mode, ref)


def compare(c: Head, form, got, ref, gate):
    for k, r in ref.items():
        g = got[k]
        assert torch.isfinite(g).all(), f"{c.name} {form} {k}: unwritten or non-finite elements"
        err = (g - r).abs()
        print(f"{c.name} {form} {k}: max|gpu - ref| = {err.max().item():.3e}, max gate = {gate[k].max().item():.3e}, "
              f"max|ref| = {r.abs().max().item():.3e}")
        bad = err > gate[k]                              # a zero gate: equality
        assert not bad.any(), f"{c.name} {form} {k}: {int(bad.sum())} of {r.numel()} elements over the gate, worst {err.max().item():.3e}"


# ------------------------------------------------------------------------------------------------ begin conv
def run_begin(c: Head, mode, o, h16=False, outputs=None):
    x, w, b = f32(o["x"]), f32(o["w"]), f32(o["bias"])
    out = torch.full((c.B, c.H, c.W, 128), NAN, dtype=torch.bfloat16 if h16 else torch.float32, device=DEV)
    stats = torch.full((c.B, c.H * c.W // 64, 128, 2), NAN, device=DEV)
    if outputs is not None:
        outputs += [out, stats]
    KL.check(KL.lib().sdpk_begin_conv(x.data_ptr(), w.data_ptr(), b.data_ptr(), out.data_ptr(), stats.data_ptr(), c.B, c.H, c.W,
                                      KR.MODES[mode], int(h16), KL.stream()), c.name)
    torch.cuda.synchronize()
    return {"out": back(out), "stats": stats.cpu()}


BEGIN = [Head(f"begin-{k}", "begin", *BEGIN_SHAPES[k]) for k in "abp"] + \
        [Head(f"begin-{k}-real", "begin", *BEGIN_SHAPES[k], real=True) for k in "ab"]
BEGIN_Q = Head("begin-q", "begin", *BEGIN_SHAPES["q"])
BEGIN_PARAMS = [pytest.param(c, f, id=f"{c.name}-{FORM_ID(f)}") for c in BEGIN for f in FORMS] + \
               [pytest.param(BEGIN_Q, FORMS[0], id="begin-q-fp32")]


@pytest.mark.parametrize("c,form", BEGIN_PARAMS)
def test_begin_conv(c, form):
    """The conv output against input_prep + zero-padded conv; the 64-pixel (mean, M2) groups against the GPU's own
    output (kernel_ref.stats_gate), then through inpp_finalize against instance_norm_pp's scale and shift."""
    mode, h16 = form
    c = dataclasses.replace(c, h16=h16)
    assert c.real or c.lattice_bound() < 2 ** 24
    o, ref, gate = ref_and_gate(c, mode)
    got = run_begin(c, mode, o, h16)
    compare(c, FORM_ID(form), got, ref, gate)
    stats, y = got["stats"], got["out"]
    assert torch.isfinite(stats).all(), "unwritten statistics groups"
    gmax = 2.0 ** -8 * float(y.abs().max()) if h16 else 0.0     # the statistics are those of the unrounded values
    mean, var = KR.combine_stats(stats, 64)
    gm, gv = KR.stats_gate(y, gmax)
    em, ev = (mean - y.mean(dim=(2, 3))).abs(), (var - y.var(dim=(2, 3), unbiased=False)).abs()
    print(f"{c.name} {FORM_ID(form)} stats: mean err {em.max().item():.3e} (gate {gm.max().item():.3e}), "
          f"var err {ev.max().item():.3e} (gate {gv.max().item():.3e})")
    assert (em <= gm).all() and (ev <= gv).all()
    alpha, gamma, beta = TA._norm_params(128, KR.rng_for(c.name + "norm"))
    ss, _ = TA._finalize(stats, 64, alpha, gamma, beta)
    TA.check_scale_shift(ss, y, alpha, gamma, beta, gmax)


# ------------------------------------------------------------------------------------------------ end conv
def run_end(c: Head, mode, o, h16=False, lg=None, store=True, Cin=128, outputs=None):
    """One end conv launch; lg: a KL.Langevin (fused update).  Returns the scores [B][2][H][W] (float32, CUDA)."""
    x, ss, w, b = act(o["x"], h16), ss_of(o), f32(o["w"]), f32(o["bias"])
    sig, lab = f32(o["sigmas"]), o["labels"].to(DEV)
    out = torch.full((c.B, 2, c.H, c.W), NAN, device=DEV)
    if outputs is not None:
        outputs.append(out)
    KL.check(KL.lib().sdpk_end_conv(x.data_ptr(), ss.data_ptr(), w.data_ptr(), b.data_ptr(), sig.data_ptr(), lab.data_ptr(),
                                    out.data_ptr() if store else None, c.B, c.H, c.W, Cin, KR.MODES[mode], int(h16), lg,
                                    KL.stream()), c.name)
    torch.cuda.synchronize()
    return out


END_MFMA = {"a": (1, 16, 64), "b": (3, 48, 96)}
END_DIRECT = {"a": (1, 4, 64), "b": (3, 12, 192)}
END = [(Head(f"end-mfma-{k}", "end", *s), FORMS[1:]) for k, s in END_MFMA.items()] + \
      [(Head("end-mfma-a-real", "end", *END_MFMA["a"], real=True), FORMS[1:])] + \
      [(Head(f"end-direct-{k}", "end", *s), FORMS[:1]) for k, s in END_DIRECT.items()] + \
      [(Head("end-direct-a-real", "end", *END_DIRECT["a"], real=True), FORMS[:1])]
END_PARAMS = [pytest.param(c, f, id=f"{c.name}-{FORM_ID(f)}") for c, forms in END for f in forms]


@pytest.mark.parametrize("c,form", END_PARAMS)
def test_end_conv(c, form):
    mode, h16 = form
    c = dataclasses.replace(c, h16=h16)
    assert c.real or c.lattice_bound() < 2 ** 24
    assert len(set(c.labels())) == c.B and (c.B < 2 or c.labels() != sorted(c.labels()))
    o, ref, gate = ref_and_gate(c, mode)
    compare(c, FORM_ID(form), {"out": run_end(c, mode, o, h16).to(F64).cpu()}, ref, gate)


def test_end_conv_fp32x3_falls_back_to_the_direct_kernel_off_the_mfma_tiling():
    """H = 12 is no multiple of the MFMA kernel's 16 rows: the fp32x3 call runs the direct fp32 kernel, bit for bit."""
    c = Head("end-fallback", "end", *END_DIRECT["b"], real=True)
    o = _operands(c)
    a, b = run_end(c, "fp32", o), run_end(c, "fp32x3", o)
    assert torch.isfinite(a).all() and torch.equal(a, b)


# ---- the fused Langevin update
LGV = [("fp32", (2, 8, 192)), ("fp32x3", (2, 32, 96)), ("bf16", (2, 32, 96))]


def _langevin_step(x, grad, ref, mask, noise, seed, offset, step, nscale, gref, n2n):
    from sdp import _lib
    B, C, H, W = x.shape
    lik = torch.full_like(x, NAN)
    am = torch.zeros(1, dtype=torch.int32, device=DEV)
    _lib.check(_lib.lib().sdp_langevin_step(x.data_ptr(), grad.data_ptr(), ref.data_ptr(), mask.data_ptr(), KL.ptr(noise), seed,
                                            offset, step, nscale, gref, n2n, B, C, H * W, lik.data_ptr(), am.data_ptr(),
                                            KL.stream()), "langevin_step")
    torch.cuda.synchronize()
    return lik, am


@pytest.mark.parametrize("variant", ["philox", "injected", "inf"])
@pytest.mark.parametrize("mode,shape", LGV, ids=[m for m, _ in LGV])
def test_end_conv_with_fused_langevin_update(mode, shape, variant):
    """The fused launch against the plain launch followed by sdp_langevin_step on its scores, bit for bit: x, lik,
    max|x[:, 0]| and the stored scores; Philox at a non-zero counter or an injected noise buffer; out, lik and absmax
    each null; nan_to_num of an infinite score (bias[1] = +inf)."""
    c = Head(f"end-lgv-{mode}", "end", *shape, real=True)
    o = dict(_operands(c))
    n2n = int(variant == "inf")
    if n2n:
        o["bias"] = torch.tensor([float(o["bias"][0]), float("inf")], dtype=F64)
    r = KR.rng_for(c.name + variant)
    dims = (c.B, 2, c.H, c.W)
    x0, ref = f32(KR.normal(r, dims)), f32(KR.normal(r, dims))
    mask = torch.from_numpy(r.integers(0, 2, size=dims).astype("int32")).to(DEV)
    noise = f32(KR.normal(r, dims)) if variant == "injected" else None
    seed, offset = 20240607, 3 * (c.B * 2 * c.H * c.W // 4) + 17
    step, gref = 1e-3, 0.7
    nscale = float(torch.tensor(2 * step, dtype=torch.float32).sqrt())

    scores = run_end(c, mode, o)
    x_a = x0.clone()
    lik_a, am_a = _langevin_step(x_a, scores, ref, mask, noise, seed, offset, step, nscale, gref, n2n)

    def fused(store=True, with_lik=True, with_am=True):
        x = x0.clone()
        lik = torch.full_like(x, NAN) if with_lik else None
        am = torch.zeros(1, dtype=torch.int32, device=DEV) if with_am else None
        lg = KL.Langevin(x.data_ptr(), ref.data_ptr(), mask.data_ptr(), KL.ptr(noise), seed, offset, step, nscale, gref, n2n,
                         KL.ptr(lik), KL.ptr(am))
        return x, lik, am, run_end(c, mode, o, lg=lg, store=store)

    bits = lambda t: t.view(torch.int32)
    x_b, lik_b, am_b, g_b = fused()
    assert torch.isfinite(x_b).all() and torch.isfinite(lik_b).all()
    assert torch.equal(bits(g_b), bits(scores)) and (n2n or torch.isfinite(g_b).all())
    assert torch.equal(bits(x_b), bits(x_a)) and torch.equal(bits(lik_b), bits(lik_a)) and torch.equal(am_b, am_a)
    assert not torch.equal(x_b, x0)
    if n2n:
        assert torch.isinf(g_b[:, 1]).all() and torch.isfinite(g_b[:, 0]).all()
    host = x_b.cpu()[:, 0].abs().max().item()                     # max|x_new[:, 0]| on the host (finite, asserted above)
    assert am_b.view(torch.float32).item() == host
    for kw in (dict(store=False), dict(with_lik=False), dict(with_am=False)):
        x_c, lik_c, am_c, g_c = fused(**kw)
        assert torch.equal(bits(x_c), bits(x_a)), kw
        if kw.get("store", True) is False:
            assert torch.isnan(g_c).all()                     # scores not stored
        else:
            assert torch.equal(bits(g_c), bits(scores))
        if lik_c is not None:
            assert torch.equal(bits(lik_c), bits(lik_a))
        if am_c is not None:
            assert torch.equal(am_c, am_a)


# ------------------------------------------------------------------------------------------------ head weight gradients
GUARD = 4096


def _part(c: Head, written):
    """The partial-sum scratch at exactly sdpk_head_wgrad_part_floats, NaN-filled, with a NaN guard region behind."""
    n = KL.lib().sdpk_head_wgrad_part_floats(c.B, c.H, c.W)
    assert n >= written, (n, written)
    return torch.full((n + GUARD,), NAN, device=DEV), n


def _check_part(buf, n, written):
    assert torch.isfinite(buf[:written]).all(), "partials left unwritten"
    assert torch.isnan(buf[n:]).all(), "the launch wrote past sdpk_head_wgrad_part_floats"


def run_begin_wgrad(c: Head, o, outputs=None):
    x, dy = f32(o["x"]), act(o["dy"], c.h16)
    written = c.B * (c.H // 8) * (c.W // 64) * 128 * 37
    part, n = _part(c, written)
    dw, db = torch.full((128, 4, 3, 3), NAN, device=DEV), torch.full((128,), NAN, device=DEV)
    if outputs is not None:
        outputs += [dw, db]
    KL.check(KL.lib().sdpk_begin_conv_wgrad(x.data_ptr(), dy.data_ptr(), part.data_ptr(), dw.data_ptr(), db.data_ptr(), c.B, c.H,
                                            c.W, int(c.h16), KL.stream()), c.name)
    torch.cuda.synchronize()
    _check_part(part, n, written)
    return {"dw": dw.to(F64).cpu(), "db": db.to(F64).cpu()}


def run_end_bwd(c: Head, o, outputs=None):
    ds, sig, lab, w = f32(o["dscore"]), f32(o["sigmas"]), o["labels"].to(DEV), f32(o["w"])
    x, ss = act(o["x"], c.h16), ss_of(o)
    written = c.B * (c.H // 16) * (c.W // 32) * (2 * 128 * 9 + 2)
    part, n = _part(c, written)
    g = torch.full_like(x, NAN)
    dw, db = torch.full((2, 128, 3, 3), NAN, device=DEV), torch.full((2,), NAN, device=DEV)
    if outputs is not None:
        outputs += [g, dw, db]
    KL.check(KL.lib().sdpk_end_conv_backward(ds.data_ptr(), sig.data_ptr(), lab.data_ptr(), w.data_ptr(), x.data_ptr(),
                                             ss.data_ptr(), g.data_ptr(), part.data_ptr(), dw.data_ptr(), db.data_ptr(), c.B, c.H,
                                             c.W, int(c.h16), KL.stream()), c.name)
    torch.cuda.synchronize()
    _check_part(part, n, written)
    return {"g": back(g), "dw": dw.to(F64).cpu(), "db": db.to(F64).cpu()}


BWG = {"a": (1, 8, 64), "b": (3, 24, 192)}
EBW = {"a": (1, 16, 64), "b": (3, 48, 192)}
BACKWARD = [Head(f"{op}-{k}{'-real' if real else ''}", op, *s, real=real, h16=h16)
            for op, shapes in (("begin_wgrad", BWG), ("end_bwd", EBW)) for k, s in shapes.items()
            for real in (False, True) for h16 in (False, True)]


@pytest.mark.parametrize("c", BACKWARD, ids=lambda c: c.name + ("-h16" if c.h16 else ""))
def test_head_backward_kernels(c):
    """begin_wgrad: db and the image channels of dw equal on the lattice, the coordinate channels within the fp32 gate.
    end_conv_backward: g, dw and db, with a different sigma per image."""
    assert c.real or c.lattice_bound() < 2 ** 24
    o, ref, gate = ref_and_gate(c, "fp32")
    got = (run_begin_wgrad if c.op == "begin_wgrad" else run_end_bwd)(c, o)
    compare(c, "h16" if c.h16 else "float", got, ref, gate)
    if c.op == "begin_wgrad" and not c.real:
        assert torch.equal(got["dw"][:, :2], ref["dw"][:, :2]) and torch.equal(got["db"], ref["db"])


# ------------------------------------------------------------------------------------------------ DSM loss
def run_dsm(o, power, with_per=True):
    from sdp import _lib
    B, n = o["score"].shape
    s, z, m, sg = f32(o["score"]), f32(o["noise"]), f32(o["mask"]), f32(o["sigma"])
    d = torch.full((B, n), NAN, device=DEV)
    loss, per = torch.full((1,), NAN, device=DEV), torch.full((B,), NAN, device=DEV)
    part = torch.full((2 * B * 64,), NAN, device=DEV)
    _lib.check(_lib.lib().sdp_dsm_loss(s.data_ptr(), z.data_ptr(), m.data_ptr(), sg.data_ptr(), B, n, float(power), d.data_ptr(),
                                       loss.data_ptr(), per.data_ptr() if with_per else None, part.data_ptr(), KL.stream()),
               "dsm_loss")
    torch.cuda.synchronize()
    return {"dscore": d.to(F64).cpu(), "loss": loss.to(F64).cpu()[0], "loss_per": per.to(F64).cpu()}


DSM_N = [1600, 32768, 2 * 7 * 1171]


@pytest.mark.parametrize("power", [0, 2])
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("n_img", DSM_N)
def test_dsm_loss(n_img, B, power):
    zero = 1 if B == 3 else None
    o = KR.dsm_operands(f"dsm-{n_img}-{B}", B, n_img, zero_image=zero)
    ref, gate = KR.dsm_reference(o, power), KR.dsm_gate(o, power)
    got = run_dsm(o, power)
    for k in ("dscore", "loss", "loss_per"):
        assert torch.isfinite(got[k]).all(), k
    err = (got["dscore"] - ref["dscore"]).abs()
    rl = abs(got["loss"] - ref["loss"]) / ref["loss"]
    rp = ((got["loss_per"] - ref["loss_per"]).abs() / ref["loss_per"].clamp(min=1e-300)).max()
    print(f"dsm n_img={n_img} B={B} p={power}: dscore max err / gate {(err / gate.clamp(min=1e-300)).max().item():.3f}, "
          f"loss rel err {rl.item():.3e}, loss_per rel err {rp.item():.3e} (gate {2.0 ** -22:.3e})")
    assert (err <= gate).all()
    assert rl <= 2.0 ** -22 and rp <= 2.0 ** -22
    if zero is not None:
        assert got["loss_per"][zero] == 0.0 and (got["dscore"][zero] == 0.0).all()
    without = run_dsm(o, power, with_per=False)
    assert torch.equal(without["dscore"], got["dscore"]) and without["loss"] == got["loss"]
    assert torch.isnan(without["loss_per"]).all()


def test_dsm_loss_on_the_lattice():
    """B = 2, sigmas (0.5, 2), power 2, a 0 / 1 mask with exactly n_img ones: scale = sigma^2 / 2, every term exact."""
    n_img = 1600
    assert KR.dsm_lattice_bound(n_img) < 2 ** 24
    o = KR.dsm_operands("dsm-lattice", 2, n_img, lattice_case=True)
    assert o["mask"].sum().item() == n_img
    ref, got = KR.dsm_reference(o, 2), run_dsm(o, 2)
    once = lambda t: t.to(torch.float32).to(F64)
    assert torch.equal(got["dscore"], ref["dscore"])
    assert got["loss"] == once(ref["loss"]) and torch.equal(got["loss_per"], once(ref["loss_per"]))


# ------------------------------------------------------------------------------------------------ rejected launches
def _rejected(run, outputs):
    with pytest.raises(KL.KernelError):
        run()
    torch.cuda.synchronize()
    assert outputs and all(torch.isnan(t).all() for t in outputs), "a rejected launch wrote its output"


def test_begin_conv_rejects_what_it_cannot_tile():
    for name, shape, mode, h16 in (("w192", (1, 3, 192), "fp32", False), ("w192", (1, 3, 192), "bf16", False),
                                   ("h16-fp32x3", (1, 3, 128), "fp32x3", True), ("h16-fp32", (1, 3, 128), "fp32", True)):
        c, outs = Head("rej-begin-" + name, "begin", *shape), []
        _rejected(lambda: run_begin(c, mode, _operands(c), h16, outputs=outs), outs)


def test_end_conv_rejects_what_it_cannot_tile():
    def rej(name, shape, mode, h16=False, Cin=128, lgv=False):
        c, outs = Head("rej-end-" + name, "end", *shape, h16=h16), []
        lg = None
        if lgv:
            x = torch.full((c.B, 2, c.H, c.W), NAN, device=DEV)
            ref, mask = torch.zeros_like(x), torch.zeros(x.shape, dtype=torch.int32, device=DEV)
            outs.append(x)
            lg = KL.Langevin(x.data_ptr(), ref.data_ptr(), mask.data_ptr(), None, 1, 0, 0.1, 0.1, 1.0, 0, None, None)
        _rejected(lambda: run_end(c, mode, _operands(c), h16, lg=lg, Cin=Cin, outputs=outs), outs)
    rej("cin64", (1, 16, 64), "fp32", Cin=64)
    rej("cin64", (1, 16, 64), "bf16", Cin=64)
    rej("h16-fp32x3", (1, 16, 64), "fp32x3", h16=True)
    rej("h16-fp32", (1, 16, 64), "fp32", h16=True)
    rej("h16-lgv", (1, 16, 64), "bf16", h16=True, lgv=True)
    rej("h16-h8", (1, 8, 64), "bf16", h16=True)
    rej("fp32-h6", (1, 6, 64), "fp32")
    rej("fp32-w96", (1, 4, 96), "fp32")


def test_head_backward_kernels_reject_what_they_cannot_tile():
    for op, shape in (("begin_wgrad", (1, 12, 64)), ("begin_wgrad", (1, 8, 96)), ("end_bwd", (1, 8, 64)), ("end_bwd", (1, 16, 96))):
        for h16 in (False, True):
            c, outs = Head(f"rej-{op}-{shape[1]}x{shape[2]}", op, *shape, h16=h16), []
            run = run_begin_wgrad if op == "begin_wgrad" else run_end_bwd
            _rejected(lambda: run(c, _operands(c), outputs=outs), outs)
