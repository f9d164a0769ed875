// Data gradient of the score network's convolutions (DSM training, LiDARGen/losses/dsm.py:67-119
// through NCSN_LiDAR_small).  A stride-1 conv with circular or zero padding is adjoint to the
// same conv over the output gradient with the kernel flipped in both taps and transposed in
// (Cin, Cout) -- circular padding stays circular, zero padding stays zero, a dilation stays
// the same dilation -- so the data gradient is the forward implicit-GEMM kernel
// (conv_kernel.h) run on dy with the "dgrad" weight packing (train_aux.hip pack kernel),
// without prologue, and with the backward epilogue: *elu'(...) of the forward activation
// (ConvArgs::dact) and the residual add of the gradient already accumulated for its input.
#include "conv_launch.h"

// The 8 x 16 circular data gradients run on 32-Cout waves, two per SIMD (dgrad_launch_nj2), as the forward:
// the 128-Cout layers in both modes, the 256-Cout layers in bf16 (bf16 training step 151.2-151.8 ->
// 151.7-152.5 image-steps/s against the 64-Cout waves, profiles/experiments/r05_dgrad_nj2_ab.log; those
// kernels, and the build switch that restored them, were retired with the table of conv_inst.hip).
// The bf16 256-Cout data gradients on one 8-wave workgroup per tile: training 159.3-159.8 against
// 157.8-158.5 image-steps/s for two 4-wave 128-Cout ones (SDP_DGRAD_NJ2_BF16_W8=0, build-time A/B only;
// profiles/experiments/r05_dgrad_w8_vs_w4_ab.log); both arms are rows of the table
#ifndef SDP_DGRAD_NJ2_BF16_W8
#define SDP_DGRAD_NJ2_BF16_W8 1
#endif

namespace sdp {

// 8 x 16 pixel tiles (the forward's: a 10 x 18 patch, 1.41x the pixels, against 4 x 66 = 2.06x for
// 2 x 64 tiles) with the transposed direct 16x16 epilogue (conv_kernel.h TRN: 16-B elu' operand,
// residual and output accesses) for every circular 3x3 layer: bf16 training step 132.8 -> 137.0
// image-steps/s against 2 x 64 tiles (profiles/experiments/r03_dgrad16_train_ab.log, r03_trans_ab.log;
// the 32- and 64-wide tiles and the build switch for their preferred width were retired in round 8).  The
// zero-padded and 1x1 layers run on 8 x 32 tiles with the LDS-staged epilogue.

// a validated launch outside the bf16 tape (conv_inst.hip rows D1 - D5)
template <int MODE>
static hipError_t launch_dgrad_mode(const ConvArgs& a, int ks, hipStream_t st) {
  if (ks == 1) return dgrad_launch<MODE, 2, 32, 1, false>(a, st);
  if (!a.circular) return dgrad_launch<MODE, 2, 32, 3, true>(a, st);
  if (a.Cout % 256) return dgrad_launch_nj2<MODE, 4>(a, st);
  if constexpr (MODE == MODE_BF16) {
    return SDP_DGRAD_NJ2_BF16_W8 ? dgrad_launch_nj2<MODE, 8>(a, st) : dgrad_launch_nj2<MODE, 4>(a, st);
  } else {
    return dgrad_launch<MODE, 1, 16, 3, false>(a, st);
  }
}

// a.in = dy [B][H][W][Cin = forward Cout], a.wf = dgrad-packed weights, a.out = dx
// [B][H][W][Cout = forward Cin].  No pooling, no prologue.  Every path ends in a row of conv_inst.hip's
// table (D1 - D6) or in hipErrorInvalidValue with *why naming the unmet condition.
hipError_t conv_dgrad(int mode, ConvArgs a, int ks, hipStream_t st, const char** why) {
  const int d = a.dil;
  if (ks != 1 && ks != 3) { *why = "dgrad: 1x1 and 3x3 kernels only"; return hipErrorInvalidValue; }
  if (a.Cin % 64 || a.Cout % 128) { *why = "dgrad: Cin%64 and Cout%128 required"; return hipErrorInvalidValue; }
  if (a.H % d || a.W % d) { *why = "dgrad: H,W must be multiples of the dilation"; return hipErrorInvalidValue; }
  if (a.pro_mode != PRO_NONE || a.up || a.out2 || a.stats) { *why = "dgrad: plain input, no fused extras"; return hipErrorInvalidValue; }
  const int Hs = a.H / d, Ws = a.W / d;
  // one precondition for every layer: the 1x1 and zero-padded layers run on 8 x 32 tiles; a circular 3x3 runs on
  // 8 x 16 tiles and takes them in pairs, because the weight gradient of the same layer needs a 32-multiple width
  // (the training plan's admitted widths follow from this check)
  if (Ws % 32 || Hs % 8) {
    *why = "dgrad: sub-grid not divisible by 8 x 32 (8 x 32 pixel tiles; the 8 x 16 tiles of a circular 3x3 in pairs)";
    return hipErrorInvalidValue;
  }
  if (!a.circular && d != 1) { *why = "dgrad: zero padding only for d=1"; return hipErrorInvalidValue; }
  if (a.dact && !a.aux) { *why = "dgrad: dact needs aux"; return hipErrorInvalidValue; }
  if (a.dact == 3 && !a.epi_ss) { *why = "dgrad: dact 3 needs epi_ss"; return hipErrorInvalidValue; }
  if (!a.pro_ss) { *why = "dgrad: prologue identity table missing"; return hipErrorInvalidValue; }
  if (!a.wf16) { *why = "dgrad: weights in wf16 (the #dfrag16 packing)"; return hipErrorInvalidValue; }
  if (a.io16) {   // the bf16 training tape: the shapes the training plan launches (rows D6)
    if (mode != MODE_BF16) { *why = "dgrad: bf16 tensors (io16) need bf16 mode"; return hipErrorInvalidValue; }
    if (ks == 1) return dgrad_launch<MODE_BF16, 2, 32, 1, false, true>(a, st);
    if (!a.circular) return dgrad_launch<MODE_BF16, 2, 32, 3, true, true>(a, st);
    return dgrad_launch_nj2<MODE_BF16, 4, true>(a, st);   // 128-Cout workgroups (see conv.hip's io16 forward)
  }
  switch (mode) {
    case MODE_F32X3: return launch_dgrad_mode<MODE_F32X3>(a, ks, st);
    case MODE_BF16: return launch_dgrad_mode<MODE_BF16>(a, ks, st);
    default: *why = "dgrad: training runs in fp32x3 or bf16"; return hipErrorInvalidValue;
  }
}

}  // namespace sdp
