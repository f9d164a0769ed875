"""One-hot taps PER CHUNK through the tap-scheduled forward 3x3 kernels: the K loop's peeled tail must compute what
the steady body computes.

The tap schedule (conv_kernel.h do_chunk9) ends its K loop in a peeled pair of 32-channel chunks: the second-to-last
issues no LDS-DMA and loads no (scale, shift) rows, the last runs no transform and loads no weights of a next chunk
(its taps 7 and 8 sit beside the removed loads) and no barrier closes it.  With the weights one-hot per chunk and tap,
w[co][ci][kh][kw] = [ci == 32 k + co % 32][(kh, kw) == t], output channel co IS input channel 32 k + co % 32 moved by
tap t, and with an input of small integers that code (image, row, column, channel) -- exact in bf16, one non-zero
term per sum -- the output must EQUAL it: a chunk staged from the wrong channels or the wrong image, a weight
fragment of another chunk or tap, a (scale, shift) row of another chunk, a patch buffer read before it is complete,
all change integers.

Shapes: 8 x 16 (one tile per image) and 16 x 32 (2 x 2 tiles), B = 2 -- a tile ends at the end of image 0 with
image 1 behind it.  Cin in {64, 128, 192, 256} -> 128 Cout and 256 -> 256 (the paired fp32x3 launch, the 8-wave
bf16 one); Cin = 64 is two chunks: the steady loop runs zero times.  Per case all 9 taps for the first chunk and the
last two, the centre tap for the chunks between.  fp32x3 and bf16; fp32x3 also on 16-bit integers (non-zero lo
halves); behind the ELU prologue (the identity on the non-negative input); behind the affine + ELU prologue with a
per-channel scale in {1, 2}, shift 0 and inputs <= 127; the bf16 tape (IO16) 128 -> 128.  The 4x4 stride-2 kernel
(128 -> 256 on 16 x 32): one-hot 3x3 weights merge into 4x4 weights that are multiples of 1/4, and the output must
equal the 2x2 mean of the zero-padded shifted channel, for k in the first and last channel chunks.
Launched through the sdpk_* entries by test_gpu_kernels_conv.run_case.
"""
import functools

import pytest
import torch
import torch.nn.functional as F

import kernel_ref as KR
from kernel_ref import Case

B = 2
SHAPES = ((8, 16), (16, 32))
CHANNELS = ((64, 128), (128, 128), (192, 128), (256, 128), (256, 256))
CH_IDS = [f"{a}to{b}" for a, b in CHANNELS]
MODES = ("fp32x3", "bf16")
CENTRE = 4


def coded_batch(H, W, C, wide=False, top=256):
    """NCHW float64 [B][C][H][W] of integers coding (image, row, column, channel): 0 .. top - 1 (top <= 256: exact in
    bf16), or `wide` 0 .. 65535 (exact as bf16 hi + bf16 lo, the lo half non-zero).  Odd multipliers: the code differs
    between the two images, any two rows, any two columns and any two channels (fewer than `top` apart)."""
    b = torch.arange(B, dtype=torch.int64).view(B, 1, 1, 1)
    r = torch.arange(H, dtype=torch.int64).view(1, 1, H, 1)
    c = torch.arange(W, dtype=torch.int64).view(1, 1, 1, W)
    ch = torch.arange(C, dtype=torch.int64).view(1, C, 1, 1)
    if wide:
        return ((b * 30011 + r * 9973 + c * 331 + ch * 77) % 65536).to(torch.float64)
    return ((b * 101 + r * 37 + c * 5 + ch * 11) % top).to(torch.float64)


def chunk_taps(cin):
    """(k, t) of a case: every tap for the first chunk and the last two, the centre tap for the others."""
    n = cin // 32
    return [(k, t) for k in range(n) for t in (range(9) if k == 0 or k >= n - 2 else (CENTRE,))]


def selected(cout, k):
    """Input channel of output channel co: 32 k + co % 32."""
    return 32 * k + torch.arange(cout) % 32


def one_hot_weights(cin, cout, k, t):
    w = torch.zeros(cout, cin, 3, 3, dtype=torch.float32)
    w[torch.arange(cout), selected(cout, k), t // 3, t % 3] = 1.0
    return w


def shifted(x, t):
    """out[y][x] = in[y + kh - 1][x + kw - 1], circular."""
    return torch.roll(x, shifts=(-(t // 3 - 1), -(t % 3 - 1)), dims=(2, 3))


def shifted_zero_padded(x, t):
    """out[y][x] = in[y + kh - 1][x + kw - 1], zero outside the image."""
    H, W = x.shape[2:]
    return F.pad(x, (1, 1, 1, 1))[:, :, t // 3:t // 3 + H, t % 3:t % 3 + W]


def mean2x2(y):
    return (y[:, :, 0::2, 0::2] + y[:, :, 1::2, 0::2] + y[:, :, 0::2, 1::2] + y[:, :, 1::2, 1::2]) / 4.0


def scales(cin):
    """[B][cin] in {1, 2}, drawn once: any two chunks differ at about half of their 32 channel positions."""
    return 1.0 + torch.from_numpy(KR.rng_for("conv-tail-scale").integers(0, 2, size=(B, cin))).to(torch.float64)


def expected(x, cout, k, t, scale=None, s2=False):
    sel = selected(cout, k)
    a = x if scale is None else x * scale[:, :, None, None]
    if s2:
        return mean2x2(shifted_zero_padded(a[:, sel], t))
    return shifted(a[:, sel], t)


@functools.lru_cache(maxsize=None)
def _input(H, W, C, wide=False, top=256):
    return coded_batch(H, W, C, wide, top)


def test_the_expectation_is_the_reference_conv_of_a_one_hot_chunk_and_tap():
    """The expectation itself, against the float64 reference conv (tests/kernel_ref.py): plain, behind the affine +
    ELU prologue, and the 2x2 mean of the zero-padded conv that the 4x4 stride-2 kernel computes."""
    H, W, cin, cout = 8, 16, 64, 128
    x = coded_batch(H, W, cin)
    xs = coded_batch(H, W, cin, top=128)
    sc = scales(cin)
    assert set(sc.unique().tolist()) == {1.0, 2.0} and not torch.equal(sc[:, :32], sc[:, 32:])
    for k, t in chunk_taps(cin):
        w = one_hot_weights(cin, cout, k, t).to(torch.float64)
        c = Case("tail-ref", "fwd", B, H, W, cin, cout)
        assert torch.equal(KR.conv_forward(c, {"x": x, "w": w})["out"], expected(x, cout, k, t)), (k, t)
        c = Case("tail-ref-aff", "fwd", B, H, W, cin, cout, pro=KR.PRO_AFFINE_ELU)
        o = {"x": xs, "w": w, "scale": sc, "shift": torch.zeros(B, cin, dtype=torch.float64)}
        assert torch.equal(KR.conv_forward(c, o)["out"], expected(xs, cout, k, t, scale=sc)), (k, t)
        c = Case("tail-ref-s2", "fwd", B, H, W, cin, cout, circular=False, s2=True, pro=KR.PRO_ELU)
        assert torch.equal(KR.conv_forward(c, {"x": x, "w": w})["out"], expected(x, cout, k, t, s2=True)), (k, t)
    assert [len(chunk_taps(c)) for c in (64, 128, 192, 256)] == [18, 28, 30, 32]
    for C in (128, 256):   # exact in the number formats: bf16, bf16 hi + bf16 lo, and the scaled values in bf16
        assert torch.equal(KR.bf16_round(coded_batch(16, 32, C)), coded_batch(16, 32, C))
        wide = coded_batch(16, 32, C, wide=True)
        hi = KR.bf16_round(wide)
        assert torch.equal(hi + KR.bf16_round(wide - hi), wide) and bool((wide != hi).any())
        assert float(coded_batch(16, 32, C, top=128).max()) == 127
    assert not torch.equal(coded_batch(8, 16, 64)[0], coded_batch(8, 16, 64)[1])


def _check(H, W, cin, cout, mode, pairs=None, wide=False, top=256, scale=None, **kw):
    from test_gpu_kernels_conv import run_case
    x = _input(H, W, cin, wide, top)
    s2 = kw.get("s2", False)
    o = {"x": x}
    if scale is not None:
        o["scale"], o["shift"] = scale, torch.zeros(B, cin, dtype=torch.float64)
    for k, t in (chunk_taps(cin) if pairs is None else pairs):
        c = Case(f"tail-{H}x{W}-{cin}to{cout}-k{k}-t{t}", "fwd", B, H, W, cin, cout, **kw)
        got = run_case(c, mode, {**o, "w": one_hot_weights(cin, cout, k, t)})["out"]
        want = expected(x, cout, k, t, scale=scale, s2=s2)
        bad = got != want
        assert not bad.any(), (f"{c.name} {mode}: {int(bad.sum())} of {bad.numel()} elements differ, first at "
                               f"(b, c, y, x) = {tuple(bad.nonzero()[0].tolist())}")


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("cin,cout", CHANNELS, ids=CH_IDS)
@pytest.mark.parametrize("H,W", SHAPES, ids=[f"{h}x{w}" for h, w in SHAPES])
def test_one_hot_chunk_and_tap_selects_and_shifts_the_channel(H, W, cin, cout, mode):
    _check(H, W, cin, cout, mode)


@pytest.mark.gpu
@pytest.mark.parametrize("cin,cout", CHANNELS, ids=CH_IDS)
def test_one_hot_chunk_and_tap_moves_the_lo_halves_too(cin, cout):
    _check(16, 32, cin, cout, "fp32x3", wide=True)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("cin,cout", CHANNELS, ids=CH_IDS)
def test_one_hot_chunk_and_tap_behind_the_elu_prologue(cin, cout, mode):
    _check(16, 32, cin, cout, mode, pro=KR.PRO_ELU)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("cin,cout", CHANNELS, ids=CH_IDS)
def test_one_hot_chunk_and_tap_takes_its_own_chunks_scale_rows(cin, cout, mode):
    _check(16, 32, cin, cout, mode, top=128, scale=scales(cin), pro=KR.PRO_AFFINE_ELU)


@pytest.mark.gpu
@pytest.mark.parametrize("pro", (KR.PRO_NONE, KR.PRO_ELU), ids=("none", "elu"))
@pytest.mark.parametrize("H,W", SHAPES, ids=[f"{h}x{w}" for h, w in SHAPES])
def test_one_hot_chunk_and_tap_on_the_bf16_tape(H, W, pro):
    _check(H, W, 128, 128, "bf16", pro=pro, io16=True)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
def test_one_hot_chunk_and_tap_through_the_4x4_stride_2_conv(mode):
    pairs = [(k, t) for k in (0, 3) for t in range(9)]
    _check(16, 32, 128, 256, mode, pairs=pairs, circular=False, s2=True, pro=KR.PRO_ELU)
