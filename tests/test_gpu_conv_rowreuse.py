"""One-hot taps through the 8 x 16 forward 3x3 kernels: every tap must move the input by exactly its offset.

The 8 x 16 tiles' tap schedule (conv_kernel.h ROWS) keeps the A fragments of a chunk in a ring of patch rows: a tap
takes its eight fragments out of the ring by (tile row + kh), a column offset kw is one generation of the ring, and a
slot is refilled for the next kw as soon as its last use has issued.  With the weights one-hot per tap,
w[co][ci][kh][kw] = [co == ci][(kh, kw) == t], the output IS the input moved circularly by ((kh - 1) d, (kw - 1) d),
and with an input of small integers that code (row, column, channel) -- exact in bf16, so every product and every sum
(one non-zero term) is exact in both bf16 modes -- the output must EQUAL the shifted input: a fragment taken from the
wrong patch row or column offset, a slot refilled before its last use, a weight fragment of another tap or chunk, all
change integers.  Launched through the sdpk_* entries (tests/kernel_lib.py) by test_gpu_kernels_conv.run_case.

Shapes (B = 1): 16 x 32 at d = 1 (2 x 2 tiles), 8 x 16 at d = 1 (one tile that wraps onto itself), 32 x 64 at d = 2,
64 x 64 at d = 4; 128 channels (class F6) and 256 (F7 in fp32x3, F8 in bf16); the ELU prologue on 16 x 32 (the input
is non-negative, and ELU is the identity there).  Beyond those: the bf16 tape (class F10, the same schedule on 16-B
copies) on 16 x 32, and in fp32x3 an input of 16-bit integers, whose lo halves are non-zero -- the small integers
leave the lo half of the ring all zeros.  The 4x4 stride-2 kernel (F9) keeps its tap order and fragments: no case.
"""
import functools

import pytest
import torch

import kernel_ref as KR
from kernel_ref import Case

SHAPES = ((16, 32, 1), (8, 16, 1), (32, 64, 2), (64, 64, 4))
TAPS = tuple(range(9))


def coded_input(H, W, C, wide=False):
    """NCHW float64 [1][C][H][W] of integers coding (row, column, channel): 0 .. 255 (exact in bf16), or `wide`
    0 .. 65535 (exact as bf16 hi + bf16 lo, the lo half non-zero).  The multipliers are odd, so the code differs between
    any two rows, any two columns (fewer than 256 apart) and any two channels."""
    r = torch.arange(H, dtype=torch.int64).view(1, 1, H, 1)
    c = torch.arange(W, dtype=torch.int64).view(1, 1, 1, W)
    ch = torch.arange(C, dtype=torch.int64).view(1, C, 1, 1)
    if wide:
        return ((r * 9973 + c * 331 + ch * 77) % 65536).to(torch.float64)
    return ((r * 37 + c * 5 + ch * 11) % 256).to(torch.float64)


def one_hot_weights(C, t):
    w = torch.zeros(C, C, 3, 3, dtype=torch.float64)
    w[torch.arange(C), torch.arange(C), t // 3, t % 3] = 1.0
    return w


def shifted(x, t, d):
    """out[y][x] = in[y + (kh - 1) d][x + (kw - 1) d], circular."""
    return torch.roll(x, shifts=(-(t // 3 - 1) * d, -(t % 3 - 1) * d), dims=(2, 3))


@functools.lru_cache(maxsize=None)
def _input(H, W, C, wide=False):
    return coded_input(H, W, C, wide)


def test_shifted_input_is_the_reference_conv_of_a_one_hot_tap():
    """The expectation itself, against the float64 reference conv (tests/kernel_ref.py), dilated and not."""
    for H, W, d in ((8, 16, 1), (8, 16, 2)):
        c = Case(f"onehot-ref-d{d}", "fwd", 1, H, W, 32, 32, dil=d)
        x = coded_input(H, W, 32)
        for t in TAPS:
            ref = KR.conv_forward(c, {"x": x, "w": one_hot_weights(32, t)})["out"]
            assert torch.equal(ref, shifted(x, t, d)), (d, t)
    assert float(coded_input(64, 64, 256).max()) <= 255 and float(coded_input(64, 64, 256, True).max()) <= 65535
    assert torch.equal(KR.bf16_round(coded_input(64, 64, 256)), coded_input(64, 64, 256))


def _check(H, W, d, C, mode, t, wide=False, **kw):
    from test_gpu_kernels_conv import run_case
    c = Case(f"onehot-{H}x{W}-d{d}-{C}-t{t}", "fwd", 1, H, W, C, C, dil=d, **kw)
    x = _input(H, W, C, wide)
    got = run_case(c, mode, {"x": x, "w": one_hot_weights(C, t)})["out"]
    want = shifted(x, t, d)
    bad = got != want
    assert not bad.any(), (f"{c.name} {mode}: {int(bad.sum())} of {bad.numel()} elements differ, first at "
                           f"(b, c, y, x) = {tuple(bad.nonzero()[0].tolist())}")


@pytest.mark.gpu
@pytest.mark.parametrize("t", TAPS)
@pytest.mark.parametrize("mode", ("fp32x3", "bf16"))
@pytest.mark.parametrize("C", (128, 256))
@pytest.mark.parametrize("H,W,d", SHAPES, ids=[f"{h}x{w}-d{d}" for h, w, d in SHAPES])
def test_one_hot_tap_shifts_the_input(H, W, d, C, mode, t):
    _check(H, W, d, C, mode, t)


@pytest.mark.gpu
@pytest.mark.parametrize("t", TAPS)
@pytest.mark.parametrize("mode", ("fp32x3", "bf16"))
@pytest.mark.parametrize("C", (128, 256))
def test_one_hot_tap_behind_the_elu_prologue(C, mode, t):
    _check(16, 32, 1, C, mode, t, pro=KR.PRO_ELU)


@pytest.mark.gpu
@pytest.mark.parametrize("t", TAPS)
@pytest.mark.parametrize("pro", (KR.PRO_NONE, KR.PRO_ELU), ids=("none", "elu"))
def test_one_hot_tap_on_the_bf16_tape(pro, t):
    _check(16, 32, 1, 128, "bf16", t, pro=pro, io16=True)


@pytest.mark.gpu
@pytest.mark.parametrize("t", TAPS)
@pytest.mark.parametrize("C", (128, 256))
def test_one_hot_tap_moves_the_lo_halves_too(C, t):
    _check(16, 32, 1, C, "fp32x3", t, wide=True)
