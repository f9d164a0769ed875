// Shape dispatch of the forward convolutions of NCSN_LiDAR_small (kernel: conv_kernel.h;
// launchers: conv_launch.h; what is built: the table in conv_inst.hip, rows F1 - F10).
#include "conv_launch.h"

namespace sdp {

// The 8 x 16 3x3 forward tiles run on 32-Cout waves, two per SIMD (conv_launch_nj2): the 128-Cout layers
// in both bf16 modes (4-wave workgroups, two per CU: 128->128 @64x1024 203.7 -> 184.4 us per fp32x3 B=4
// launch in the network, line 333.7-336.1 -> 345.0-345.1 image-steps/s, against 2-wave workgroups of
// 64-Cout waves), the 256-Cout layers in bf16 (8-wave workgroups: 87.4 -> 80.8-85.4 us per B=4 launch; in
// fp32x3 the 8-wave workgroup measured slower than one 64-Cout wave per SIMD, 163.0 -> 165.8 us)
// -- profiles/experiments/r05_nj2_ab.log.
// The fp32x3 256-Cout layers run as two of those 128-Cout workgroups per tile (the patch is staged
// twice, and 8 waves per CU hide each other's phases): line 348.6-348.9 -> 356.6-357.5
// image-steps/s, 256->256 160.9-162.4 -> 159.7-161.5 us per launch (profiles/experiments/
// r05_pair256_ab.log).  The 64-Cout-wave kernels those runs compared against, and the build switch that
// restored them, were retired with the table of conv_inst.hip; SDP_CONV_NJ2_BF16_W8 (build-time A/B only,
// tools/lib_variant.sh) picks the 8-wave workgroups for the bf16 256-Cout layers, and both arms are rows.
#ifndef SDP_CONV_NJ2_BF16_W8
#define SDP_CONV_NJ2_BF16_W8 1
#endif

// the 8 x 16 tiles of a non-pooled 3x3 in a bf16 mode (rows F6 - F8)
template <int MODE, bool PELU>
static hipError_t launch_nj2(const ConvArgs& a, hipStream_t st) {
  if constexpr (MODE == MODE_BF16 && SDP_CONV_NJ2_BF16_W8) {
    if (a.Cout % 256 == 0) return conv_launch_nj2<MODE, PELU, 8>(a, st);
  }
  return conv_launch_nj2<MODE, PELU, 4>(a, st);   // 256 Cout (fp32x3): two workgroups per tile
}

// a validated launch outside the bf16 tape and the 4x4 stride-2 form (rows F1 - F8)
template <int MODE>
static hipError_t launch_mode(const ConvArgs& a, int ks, bool pool, hipStream_t st) {
  const bool pe = a.pro_mode != PRO_NONE;
  if (ks == 1) {   // the ConvMeanPool 1x1 shortcut: pooled epilogue (training), or on pre-pooled input (forward)
    if (!pool) return conv_launch<MODE, 1, 64, 1, false, false>(a, st);
    if constexpr (MODE != MODE_F32) return conv_launch<MODE, 1, 64, 1, true, false>(a, st);
    return hipErrorInvalidValue;   // (not reached: conv_mfma rejects the pooled 1x1 in fp32)
  }
  if (pool) return conv_launch<MODE, 1, 64, 3, true, true>(a, st);
  if constexpr (MODE != MODE_F32) {
    return pe ? launch_nj2<MODE, true>(a, st) : launch_nj2<MODE, false>(a, st);
  } else if (a.Cout % 256) {
    return pe ? conv_launch<MODE, 2, 32, 3, false, true>(a, st) : conv_launch<MODE, 2, 32, 3, false, false>(a, st);
  } else {
    return pe ? conv_launch<MODE, 1, 32, 3, false, true>(a, st) : conv_launch<MODE, 1, 32, 3, false, false>(a, st);
  }
}

// Host entry: validates the shape contract the kernel's indexing assumes, then launches.  Every path ends
// in a row of conv_inst.hip's table or in hipErrorInvalidValue with *why naming the unmet condition.
//
// Workgroup shapes (conv_kernel.h ConvTile), tiles = rows x columns of the dilation's sub-grid:
//   bf16 modes (fp32x3, bf16; 16x16 MFMAs), non-pooled 3x3 layers: 8 x 16 pixel tiles (a 10 x 18 patch,
//     1.41x the pixels; 171.4 -> 167.0 -> ~164 us per 256->256 @32x512 launch against 4 x 32 / 2 x 64
//     tiles, profiles/experiments/r02_tile_width_ab.log) of 128 px x 128 Cout on 4 waves, two workgroups
//     per CU (one's prologue and epilogue run under the other's MFMAs), or 128 px x 256 Cout on 8 waves;
//   exact fp32 (32x32 MFMAs, 32-pixel fragment rows): 4 x 32 tiles of 128 px x 256 Cout, or 8 x 32 tiles
//     of 256 px x 128 Cout;
//   pooled (ConvMeanPool) and 1x1 layers: 2 x 64 tiles of 128 px x 256 Cout.
hipError_t conv_mfma(int mode, ConvArgs a, int ks, bool pool, hipStream_t st, const char** why) {
  const int d = a.dil;
  if (ks != 1 && ks != 3) { *why = "conv: 1x1 and 3x3 kernels only"; return hipErrorInvalidValue; }
  if (a.Cin % 64 || a.Cout % 128) { *why = "conv: Cin%64 and Cout%128 required"; return hipErrorInvalidValue; }
  if (a.H % d || a.W % d) { *why = "conv: H,W must be multiples of the dilation"; return hipErrorInvalidValue; }
  const int Hs = a.H / d, Ws = a.W / d;
  const int wm = (a.Cout % 256 == 0) ? 1 : 2;
  const bool sh16 = mode != MODE_F32;
  if (ks == 1 || pool) {
    if (Ws % 64 || Hs % 2) { *why = "conv: sub-grid not divisible by the 2 x 64 pixel tile"; return hipErrorInvalidValue; }
  } else if (sh16) {
    if (Ws % 16 || Hs % 8) {
      *why = "conv: sub-grid not divisible by the 8 x 16 pixel tile of the bf16 modes";
      return hipErrorInvalidValue;
    }
  } else if (wm == 2) {
    if (Ws % 32 || Hs % 8) { *why = "conv: sub-grid not divisible by the 8 x 32 pixel tile"; return hipErrorInvalidValue; }
  } else if (Ws % 32 || Hs % 4) {
    *why = "conv: sub-grid not divisible by the 4 x 32 pixel tile of the fp32 256-Cout layers";
    return hipErrorInvalidValue;
  }
  if (sh16 && !a.wf16) { *why = "conv: bf16 modes need the 16x16 weight packing (#frag16)"; return hipErrorInvalidValue; }
  if (!sh16 && !a.wf) { *why = "conv: exact fp32 needs the 32x32 weight packing (#frag)"; return hipErrorInvalidValue; }
  if (ks == 1 && !pool && (d != 1 || wm != 1)) { *why = "conv: 1x1 needs d=1 and 256-multiple Cout"; return hipErrorInvalidValue; }
  if (pool && (d != 1 || wm != 1 || (a.H & 1) || (a.W & 1))) {
    *why = "conv: pooling needs d=1, even H,W and 256-multiple Cout";
    return hipErrorInvalidValue;
  }
  if (a.up && ((a.H & 1) || (a.W & 1) || a.H < 2 || a.W < 2)) { *why = "conv: upsample needs even H,W"; return hipErrorInvalidValue; }
  if (!a.circular && d != 1) { *why = "conv: zero padding only for d=1"; return hipErrorInvalidValue; }
  if (!a.pro_ss) { *why = "conv: prologue scale/shift table missing"; return hipErrorInvalidValue; }
  if (a.Cin > 1024 && a.ss_bstride == 0) { *why = "conv: identity table holds 1024 channels"; return hipErrorInvalidValue; }
  const bool pe = a.pro_mode != PRO_NONE;
  if (a.s2) {   // the ConvMeanPool 3x3 as a 4x4 stride-2 conv (conv_kernel.h S2): 8 x 16 tiles of the half-resolution output
    if (!sh16 || a.io16 || ks != 3 || pool || d != 1 || a.circular || a.up || !pe || a.dact || (a.H % 16) || (a.W % 32)) {
      *why = "conv: the 4x4 stride-2 form needs a bf16 mode, a zero-padded 3x3 with an ELU prologue, H%16 and W%32";
      return hipErrorInvalidValue;
    }
    return mode == MODE_F32X3 ? conv_launch_s2<MODE_F32X3>(a, st) : conv_launch_s2<MODE_BF16>(a, st);
  }
  // combinations no kernel is built for (the non-pooled kernels clamp at the border: ZP = POOL in conv_inst.hip)
  if (ks == 3 && !pool && !a.circular) {
    *why = "conv: a non-pooled 3x3 needs circular padding (zero padding: the pooled and the 4x4 stride-2 form only)";
    return hipErrorInvalidValue;
  }
  if (ks == 3 && pool && !pe) { *why = "conv: the pooled 3x3 needs an ELU prologue"; return hipErrorInvalidValue; }
  if (ks == 1 && pool && (pe || !sh16)) {
    *why = "conv: the pooled 1x1 needs a bf16 mode and no prologue";
    return hipErrorInvalidValue;
  }
  if (ks == 1 && !pool && pe) { *why = "conv: the non-pooled 1x1 takes no prologue"; return hipErrorInvalidValue; }
  if (a.io16) {   // the bf16 training tape: the shapes the training plan launches (rows F10)
    if (mode != MODE_BF16) { *why = "conv: bf16 tensors (io16) need bf16 mode"; return hipErrorInvalidValue; }
    if (pool) return ks == 1 ? conv_launch<MODE_BF16, 1, 64, 1, true, false, true>(a, st)
                             : conv_launch<MODE_BF16, 1, 64, 3, true, true, true>(a, st);
    if (ks == 1) { *why = "conv: no bf16-tensor (io16) kernel for the non-pooled 1x1"; return hipErrorInvalidValue; }
    // 8 x 16 tiles: 4-wave 128-Cout workgroups for both Cout widths (the 256-Cout layers as a pair per
    // tile): with 8-channel staging units an 8-wave workgroup leaves 29 % of its units empty (720 for 1024
    // slots) and ran the 256-class slower than the float32 tape (181 vs 168.5 us per B=8 launch)
    return pe ? conv_launch_nj2<MODE_BF16, true, 4, true>(a, st) : conv_launch_nj2<MODE_BF16, false, 4, true>(a, st);
  }
  switch (mode) {
    case MODE_F32: return launch_mode<MODE_F32>(a, ks, pool, st);
    case MODE_F32X3: return launch_mode<MODE_F32X3>(a, ks, pool, st);
    default: return launch_mode<MODE_BF16>(a, ks, pool, st);
  }
}

}  // namespace sdp
