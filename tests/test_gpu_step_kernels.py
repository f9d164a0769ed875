"""sdp_langevin_step and sdp_axpy_step against numpy float32 in the reference order (MI355X only).

csrc/langevin.hip promises "reference evaluation order, no FMA contraction"; the oracle is
oracle/sampling_ref.py (langevin_update, nan_to_num) and the two axpy forms written out below.  With an injected
noise buffer everything is bit-equal: x, lik and the absmax word (the float bits of max|x_new[:, 0]|, which the
merge's tooHigh test consumes).

Launch geometry these shapes are chosen against (langevin.hip): one thread per float4 group, 256 threads a block;
with the absmax word at most 256 blocks (65 536 groups a pass of the grid-stride loop), without it at most 2048
blocks (524 288 groups a pass); axpy: one thread per element, at most 2048 blocks (524 288 elements a pass).
"""
import numpy as np
import pytest
import torch

from oracle import golden_inputs as GI
from oracle import philox_ref
from oracle import sampling_ref as S

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32 = np.float32
PASS4 = 256 * 256           # float4 groups per pass with the absmax word


def _t(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _bits(a):
    return np.ascontiguousarray(a, dtype=F32).view(np.uint32)


def _word_of(v):
    """The float32 bits of a scalar, as an unsigned int."""
    return int(np.asarray(v, dtype=F32).reshape(1).view(np.uint32)[0])


def _step_scalars():
    sig = __import__("sdp").get_sigmas_np()
    s = S.step_size_of(6.2e-6, sig[100], sig[-1])
    return s, F32(np.sqrt(F32(s * F32(2))))


def _langevin(x, g, ref, mask, noise, B, C, HW, *, seed=0, offset=0, step=0.0, nscale=1.0, gref=1.0, n2n=0, lik=True,
              absmax=True, check=True):
    """One sdp_langevin_step call; returns (rc or None, x, lik, absmax word) as numpy / int."""
    from sdp import _lib
    xd, gd, rd, md, nd = _t(x), _t(g), _t(ref), _t(mask), _t(noise)
    ld = torch.full_like(xd, float("nan")) if lik else None
    ad = torch.zeros(1, dtype=torch.int32, device=DEV) if absmax else None
    rc = _lib.lib().sdp_langevin_step(xd.data_ptr(), gd.data_ptr(), rd.data_ptr(), md.data_ptr(), _lib.ptr(nd), seed,
                                      offset, float(step), float(nscale), float(gref), n2n, B, C, HW, _lib.ptr(ld),
                                      _lib.ptr(ad), _lib.stream())
    if check:
        _lib.check(rc, "langevin_step")
    torch.cuda.synchronize()
    return (rc, xd.cpu().numpy(), None if ld is None else ld.cpu().numpy(),
            None if ad is None else int(ad.cpu().item()) & 0xFFFFFFFF)


def _inputs(tag, B, C, HW):
    r = GI.rng("step-kernels-" + tag)
    shape = (B, C, HW)
    x = r.random(shape, dtype=np.float32)
    g = (r.standard_normal(shape) * 3.0).astype(F32)
    ref = r.random(shape, dtype=np.float32)
    mask = (r.random(shape) > 0.4).astype(np.int32)
    noise = r.standard_normal(shape).astype(F32)
    return x, g, ref, mask, noise


def _plant(x, g, mask, noise, where):
    """Make max|x_new| of channel 0 fall in float4 group ``where`` of the channel-0 groups' flat order, and put a
    larger value into every other channel (it must be ignored).  The planted elements are unknown pixels
    (mask 0) with a zero score and zero noise, so x_new there is the planted value itself; every other |x_new| stays
    well below 7 (the test asserts the oracle's maxima)."""
    B, C, HW = x.shape
    n4_plane = HW // 4
    groups = [i for i in range(B * C * n4_plane) if (i // n4_plane) % C == 0]
    i = {"second_pass": next((j for j in groups if j >= PASS4), groups[len(groups) // 2]), "last": groups[-1]}[where]
    flat = lambda a: a.reshape(-1)
    e = 4 * i + 2
    for a, v in ((x, -7.0), (g, 0.0), (mask, 0), (noise, 0.0)):
        flat(a)[e] = v
    for c in range(1, C):           # channel c of the last image, its very last element: the tensor's last group for c = C-1
        x[B - 1, c, HW - 1], g[B - 1, c, HW - 1], mask[B - 1, c, HW - 1], noise[B - 1, c, HW - 1] = 9.0, 0.0, 0, 0.0
        x[0, c, 1], g[0, c, 1], mask[0, c, 1], noise[0, c, 1] = -9.5, 0.0, 0, 0.0
    return i


SHAPES = [(1, 1, 4), (2, 3, 1028), (3, 2, 65536), (5, 2, 65536)]


@pytest.mark.parametrize("where", ["second_pass", "last"])
@pytest.mark.parametrize("B,C,HW", SHAPES, ids=["x".join(map(str, s)) for s in SHAPES])
def test_langevin_injected_noise_bit_exact_with_absmax(B, C, HW, where):
    """One float4 group; C = 3 with channel boundaries inside a block (HW / 4 = 257); 1.5 and 2.5 passes of the
    grid-stride loop.  The winning |x_new| of channel 0 sits in the second pass (``second_pass``; the middle where
    there is one pass only) or in the last channel-0 group (``last``); larger values sit in the other channels, one
    of them in the last group of the tensor."""
    x, g, ref, mask, noise = _inputs(f"{B}-{C}-{HW}", B, C, HW)
    i = _plant(x, g, mask, noise, where)
    if B * C * HW // 4 > PASS4:
        assert i >= PASS4, "the planted maximum must lie past the first pass"
    s, ns = _step_scalars()
    want_x, want_lik = S.langevin_update(x, g, ref, mask, noise, s, 0.7)
    want_max = F32(np.abs(want_x[:, 0]).max())
    assert want_max == F32(7.0) and (C == 1 or np.abs(want_x[:, 1:]).max() == F32(9.5))
    _, got_x, got_lik, word = _langevin(x, g, ref, mask, noise, B, C, HW, step=s, nscale=ns, gref=0.7)
    np.testing.assert_array_equal(_bits(got_x), _bits(want_x))
    np.testing.assert_array_equal(_bits(got_lik), _bits(want_lik))
    assert word == _word_of(want_max), f"absmax word 0x{word:08x}, max|x[:, 0]| = {want_max}"


def test_langevin_past_the_block_cap_without_absmax_and_lik():
    """(17, 2, 65536): 557 056 groups, past the 2048-block cap of the launch without the absmax word."""
    B, C, HW = 17, 2, 65536
    assert B * C * HW // 4 > 2048 * 256
    x, g, ref, mask, noise = _inputs("cap", B, C, HW)
    s, ns = _step_scalars()
    want_x, _ = S.langevin_update(x, S.nan_to_num(g), ref, mask, noise, s, 1.0)
    _, got_x, _, _ = _langevin(x, g, ref, mask, noise, B, C, HW, step=s, nscale=ns, n2n=1, lik=False, absmax=False)
    np.testing.assert_array_equal(_bits(got_x), _bits(want_x))


@pytest.mark.parametrize("n2n", [0, 1])
@pytest.mark.parametrize("nan_channel", [0, 1])
def test_langevin_non_finite_gradients(nan_channel, n2n):
    """NaN, +inf and -inf at each of the four lanes of a group.  With nan_to_num the update is the oracle's bit for
    bit; without, the NaN pattern is numpy's (and every other value bit-equal).  The absmax word follows numpy's
    max|x[:, 0]|: a NaN in channel 0 makes it a NaN, otherwise +-inf makes it inf."""
    B, C, HW = 2, 2, 1024
    x, g, ref, mask, noise = _inputs("nonfinite", B, C, HW)
    for lane in range(4):
        g[1, nan_channel, 4 * (10 + lane) + lane] = np.nan      # 4 groups, the NaN at a different lane in each
        g[0, 0, 4 * (40 + lane) + lane] = np.inf
        g[1, 0, 4 * (80 + lane) + lane] = -np.inf
        g[0, 1, 4 * (90 + lane) + lane] = np.inf
    s, ns = _step_scalars()
    with np.errstate(invalid="ignore", over="ignore"):
        want_x, want_lik = S.langevin_update(x, S.nan_to_num(g) if n2n else g, ref, mask, noise, s, 1.0)
        want_max = F32(np.abs(want_x[:, 0]).max())
    _, got_x, got_lik, word = _langevin(x, g, ref, mask, noise, B, C, HW, step=s, nscale=ns, n2n=n2n)
    got_max = np.array([word], np.uint32).view(F32)[0]
    nan = np.isnan(want_x)
    if n2n:
        assert not nan.any() and np.isfinite(want_x).all()
    else:
        assert nan.sum() == 4 and np.isinf(want_x).sum() == 12
        assert np.isnan(want_max) == (nan_channel == 0) and (nan_channel == 0 or np.isinf(want_max))
    np.testing.assert_array_equal(np.isnan(got_x), nan)
    np.testing.assert_array_equal(_bits(got_x)[~nan], _bits(want_x)[~nan])
    np.testing.assert_array_equal(_bits(got_lik), _bits(want_lik))
    if np.isnan(want_max):
        assert np.isnan(got_max), f"absmax word 0x{word:08x} with a NaN in channel 0"
    else:
        assert word == _word_of(want_max), f"absmax word 0x{word:08x}, max|x[:, 0]| = {want_max}"


@pytest.mark.parametrize("offset", [0, 2 ** 32 - 1000, 2 ** 40 + 7], ids=["0", "2^32-1000", "2^40+7"])
def test_langevin_philox_counter_is_64_bit_and_strides_with_the_grid(offset):
    """No noise buffer: x = 0 + 1 * N(0, 1) of Philox counter offset + group, 1.5 passes of the grid-stride loop.
    2^32 - 1000 carries into the counter's high word inside the call; 2^40 + 7 starts there.  Against
    oracle/philox_ref.py within the project's gate for the device's log / sincos intrinsics, 2e-5 * max|want|."""
    B, C, HW = 3, 2, 65536
    z = np.zeros((B, C, HW), F32)
    _, got, _, word = _langevin(z, z, z, np.zeros((B, C, HW), np.int32), None, B, C, HW, seed=0x1234567887654321,
                                offset=offset, step=0.0, nscale=1.0, n2n=1)
    want = philox_ref.normal(0x1234567887654321, offset, B * C * HW).reshape(B, C, HW)
    err = np.abs(got - want).max()
    print(f"philox offset {offset}: max|err| {err:.3e}, gate {2e-5 * np.abs(want).max():.3e}")
    assert err <= 2e-5 * np.abs(want).max()
    assert word == _word_of(np.abs(got[:, 0]).max())     # the block reduction, on the device's own values


def test_langevin_rejects_hw_not_a_multiple_of_4():
    B, C, HW = 1, 2, 6
    x, g, ref, mask, noise = _inputs("rej", B, C, HW)
    rc, got_x, got_lik, word = _langevin(x, g, ref, mask, noise, B, C, HW, step=1.0, check=False)
    assert rc != 0
    np.testing.assert_array_equal(_bits(got_x), _bits(x))
    assert np.isnan(got_lik).all() and word == 0


# ------------------------------------------------------------------------------- axpy
def _axpy(x, g, a, lik, mask, ref, b, check=True):
    from sdp import _lib
    xd, gd, ld, md, rd = _t(x), _t(g), _t(lik), _t(mask), _t(ref)
    rc = _lib.lib().sdp_axpy_step(xd.data_ptr(), _lib.ptr(gd), float(a), _lib.ptr(ld), _lib.ptr(md), _lib.ptr(rd),
                                  float(b), x.size, _lib.stream())
    if check:
        _lib.check(rc, "axpy")
    torch.cuda.synchronize()
    return rc, xd.cpu().numpy()


def _fma(a, b, c):
    """round_f32(a * b + c) evaluated once in float64 (the product of two float32 is exact there): what a contracted
    a * b + c gives."""
    return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(F32)


def _first_to_front(arrays, good):
    """Swap the first element at which ``good`` holds to index 0 of every array (n = 1 then keeps it)."""
    j = int(np.flatnonzero(good)[0])
    for arr in arrays:
        arr[[0, j]] = arr[[j, 0]]


AXPY_N = [1, 255, 4096, 524288 + 3]
A, Bc = F32(0.37), F32(0.7)


@pytest.mark.parametrize("n", AXPY_N)
def test_axpy_denoise_form_bit_exact_and_not_contracted(n):
    """x <- (x + a*g) + b*lik.  The operands are chosen so that every contracted evaluation -- either product or
    both fused into its addition -- differs from the reference order in at least one element (asserted), so a build
    that contracts cannot pass."""
    r = GI.rng(f"axpy-denoise-{n}")
    m = max(n, 64)
    x, g, lik = (r.standard_normal(m).astype(F32) for _ in range(3))

    def forms(x, g, lik):
        ref = ((x + A * g) + Bc * lik).astype(F32)
        t_f, t_r = _fma(A, g, x), (x + A * g).astype(F32)
        return ref, [_fma(Bc, lik, t_f), (t_f + Bc * lik).astype(F32), _fma(Bc, lik, t_r)]
    ref, alts = forms(x, g, lik)
    _first_to_front((x, g, lik), np.logical_and.reduce([_bits(a) != _bits(ref) for a in alts]))
    x, g, lik = x[:n].copy(), g[:n].copy(), lik[:n].copy()
    want, alts = forms(x, g, lik)
    for a in alts:
        assert (_bits(a) != _bits(want)).any(), "the operands do not tell the contracted form from the reference order"
    _, got = _axpy(x, g, A, lik, None, None, Bc)
    np.testing.assert_array_equal(_bits(got), _bits(want))


@pytest.mark.parametrize("n", AXPY_N)
def test_axpy_data_consistency_form_bit_exact_and_not_contracted(n):
    """x <- x + b*(-mask*(x - ref)), with b != 1 so that fusing b*l into the addition changes a result (asserted)."""
    r = GI.rng(f"axpy-final-{n}")
    m = max(n, 64)
    x, ref = r.standard_normal(m).astype(F32), r.standard_normal(m).astype(F32)
    mask = np.ones(m, np.int32)
    mask[1::5] = 0

    def forms(x, ref, mask):
        l = (-mask).astype(F32) * (x - ref)
        return (x + Bc * l).astype(F32), _fma(Bc, l, x)
    want, alt = forms(x, ref, mask)
    _first_to_front((x, ref, mask), _bits(alt) != _bits(want))
    x, ref, mask = x[:n].copy(), ref[:n].copy(), mask[:n].copy()
    want, alt = forms(x, ref, mask)
    assert (_bits(alt) != _bits(want)).any(), "the operands do not tell the contracted form from the reference order"
    if n > 1:
        assert (mask == 0).any() and (_bits(want)[mask == 0] == _bits(x)[mask == 0]).all()
    _, got = _axpy(x, None, 0.0, None, mask, ref, Bc)
    np.testing.assert_array_equal(_bits(got), _bits(want))


@pytest.mark.parametrize("what", ["g_without_lik", "neither_g_nor_mask_ref", "mask_without_ref"])
def test_axpy_rejects_incomplete_operands(what):
    r = GI.rng("axpy-rej")
    x, g, ref = (r.standard_normal(64).astype(F32) for _ in range(3))
    mask = np.ones(64, np.int32)
    args = {"g_without_lik": (g, 0.5, None, None, None), "neither_g_nor_mask_ref": (None, 0.5, None, None, None),
            "mask_without_ref": (None, 0.5, None, mask, None)}[what]
    rc, got = _axpy(x, *args, 0.5, check=False)
    assert rc != 0
    np.testing.assert_array_equal(_bits(got), _bits(x))
