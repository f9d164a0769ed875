// Definitions of the conv launchers (conv_launch.h) and the table of what is built.
//
// Built once per row of the table at the end of this file (Makefile: conv_i_<id>.o with -DSDP_INST=<id>; the
// Makefile reads the row ids from this file).  A row is one explicit instantiation, written out, with the class
// label of the parity tests (tests/test_gpu_kernels_conv.py: F1 - F10 forward, D1 - D6 data gradient).  conv.hip and
// conv_bwd.hip dispatch to these rows only; an id without a row is an #error, a dispatched launcher without a row a
// link error (-z defs).
#include "conv_kernel.h"
#include "conv_launch.h"

namespace sdp {

// MFMA shapes: the bf16 modes (fp32x3, bf16) run every launch on v_mfma_f32_16x16x32_bf16 (SH = 16);
// exact fp32 on v_mfma_f32_32x32x2_f32 (SH = 32).  The 16x16 shape holds a higher clock under this
// power-limited load at the same cycles per FLOP (256->256 185 -> 171 us,
// 128->128 @64x1024 227 -> 214 us).

// SDP_CONV_CPAIR=0 (build-time A/B only): the two Cout blocks of a tile on grid.y (dispatched a whole
// grid row apart, the second patch read from HBM)
#ifndef SDP_CONV_CPAIR
#define SDP_CONV_CPAIR 1
#endif

// SDP_NJ2_STRIP (build-time A/B): strip tile order (conv_strip_w) for the 4-wave 32-Cout-wave launches too --
// 1 = the paired 256-Cout layers, 2 = every 4-wave launch (the 128-channel layers as well)
#ifndef SDP_NJ2_STRIP
#define SDP_NJ2_STRIP 1
#endif

template <int MODE, int WM, int TC, int KS, bool POOL, bool PELU, bool IO16>
hipError_t conv_launch(ConvArgs a, hipStream_t st) {
  using T = ConvTile<WM, TC, KS, 4, 4, IO16>;
  a.tiles_per_img = a.H * a.W / (T::TR * TC);
  a.groups_per_img = a.H * a.W / 128;
  a.strip_w = conv_strip_w(a.H / a.dil / T::TR, a.W / a.dil / TC);
  dim3 grid(a.B * a.tiles_per_img, a.Cout / T::NTILE);
  if constexpr (MODE != MODE_F32) {
    hipLaunchKernelGGL((conv_mfma_kernel<MODE, WM, TC, KS, POOL, POOL, PELU, 16, 4, false, 4, IO16>),
                       grid, dim3(256), 0, st, a);
    return hipGetLastError();
  } else if constexpr (TC >= 32) {   // the 32x32 shape tiles rows in 32-pixel fragments
    hipLaunchKernelGGL((conv_mfma_kernel<MODE, WM, TC, KS, POOL, POOL, PELU>), grid, dim3(256), 0, st, a);
    return hipGetLastError();
  }
  return hipErrorInvalidValue;   // (not reached: conv.hip picks 16-wide tiles for the bf16 modes only)
}

// 32-Cout waves, two per SIMD (conv_kernel.h ConvTile NJ = 2): 128 px x 128 Cout on 4 waves, two
// workgroups per CU (pair), or 128 px x 256 Cout on 8 waves, one per CU (oct)
template <int MODE, bool PELU, int NW, bool IO16>
hipError_t conv_launch_nj2(ConvArgs a, hipStream_t st) {
  using T = ConvTile<1, 16, 3, NW, 2, IO16>;
  a.tiles_per_img = a.H * a.W / (T::TR * 16);
  a.groups_per_img = a.H * a.W / 128;
  // two Cout blocks per tile (the fp32x3 256-Cout layers on 4-wave workgroups): dealt as adjacent pairs
  // of the XCD-ordered index, so a tile's second patch read comes from that XCD's L2
  a.cpair = (SDP_CONV_CPAIR && a.Cout == 2 * T::NTILE) ? 1 : 0;
  const bool strip = NW == 8 || SDP_NJ2_STRIP == 2 || (SDP_NJ2_STRIP == 1 && a.cpair);
  a.strip_w = strip ? conv_strip_w(a.H / a.dil / T::TR, a.W / a.dil / 16) : 0;
  dim3 grid(a.B * a.tiles_per_img * (a.cpair ? 2 : 1), a.cpair ? 1 : a.Cout / T::NTILE);
  hipLaunchKernelGGL((conv_mfma_kernel<MODE, 1, 16, 3, false, false, PELU, 16, NW, false, 2, IO16>), grid, dim3(T::NTH), 0,
                     st, a);
  return hipGetLastError();
}

// the ConvMeanPool 3x3 as a 4x4 stride-2 conv: tiles of 8 x 16 output pixels, the grid and the statistics groups
// are those of the half-resolution output
template <int MODE>
hipError_t conv_launch_s2(ConvArgs a, hipStream_t st) {
  using T = ConvTile<1, 16, 3, 4, 2>;
  const int Ho = a.H / 2, Wo = a.W / 2;
  a.tiles_per_img = Ho * Wo / (T::TR * 16);
  a.groups_per_img = Ho * Wo / 128;
  a.cpair = (SDP_CONV_CPAIR && a.Cout == 2 * T::NTILE) ? 1 : 0;
  a.strip_w = a.cpair ? conv_strip_w(Ho / T::TR, Wo / 16) : 0;
  dim3 grid(a.B * a.tiles_per_img * (a.cpair ? 2 : 1), a.cpair ? 1 : a.Cout / T::NTILE);
  hipLaunchKernelGGL((conv_mfma_kernel<MODE, 1, 16, 3, false, true, true, 16, 4, false, 2, false, true>), grid, dim3(T::NTH),
                     0, st, a);
  return hipGetLastError();
}

template <int MODE, int WM, int TC, int KS, bool ZP, bool IO16>
hipError_t dgrad_launch(ConvArgs a, hipStream_t st) {
  using T = ConvTile<WM, TC, KS, 4, 4, IO16>;
  a.tiles_per_img = a.H * a.W / (T::TR * TC);
  a.groups_per_img = a.H * a.W / 128;
  dim3 grid(a.B * a.tiles_per_img, a.Cout / T::NTILE);
  if constexpr (TC < 32) {   // 8 x 16 tiles: the transposed direct epilogue (conv_kernel.h TRN)
    hipLaunchKernelGGL((conv_mfma_kernel<MODE, WM, TC, KS, false, ZP, false, 16, 4, true, 4, IO16>), grid, dim3(256), 0, st, a);
  } else {
    hipLaunchKernelGGL((conv_mfma_kernel<MODE, WM, TC, KS, false, ZP, false, 16, 4, false, 4, IO16>), grid, dim3(256), 0, st, a);
  }
  return hipGetLastError();
}

// data gradient on 32-Cout waves, two per SIMD (conv_kernel.h ConvTile NJ = 2, transposed epilogue):
// 4 waves = 128 Cout per workgroup, two per CU; 8 waves = 256 Cout, one per CU
template <int MODE, int NW, bool IO16>
hipError_t dgrad_launch_nj2(ConvArgs a, hipStream_t st) {
  using T = ConvTile<1, 16, 3, NW, 2, IO16>;
  a.tiles_per_img = a.H * a.W / (T::TR * 16);
  a.groups_per_img = a.H * a.W / 128;
  dim3 grid(a.B * a.tiles_per_img, a.Cout / T::NTILE);
  hipLaunchKernelGGL((conv_mfma_kernel<MODE, 1, 16, 3, false, false, false, 16, NW, true, 2, IO16>), grid, dim3(T::NTH), 0,
                     st, a);
  return hipGetLastError();
}

// ---- the table: one row per built class, selected by -DSDP_INST=<row id> ----
#ifndef SDP_INST
#error "conv_inst.hip: build with -DSDP_INST=<row id> (Makefile)"
#elif SDP_INST == 1   // F1: the 8 x 32 tiles of the 128-Cout layers, exact fp32
template hipError_t conv_launch<MODE_F32, 2, 32, 3, false, false>(ConvArgs, hipStream_t);
#elif SDP_INST == 2   // F1
template hipError_t conv_launch<MODE_F32, 2, 32, 3, false, true>(ConvArgs, hipStream_t);
#elif SDP_INST == 3   // F2: the 4 x 32 tiles of the 256-Cout layers, exact fp32
template hipError_t conv_launch<MODE_F32, 1, 32, 3, false, false>(ConvArgs, hipStream_t);
#elif SDP_INST == 4   // F2
template hipError_t conv_launch<MODE_F32, 1, 32, 3, false, true>(ConvArgs, hipStream_t);
#elif SDP_INST == 5   // F3: the pooled (ConvMeanPool) 3x3, ELU prologue
template hipError_t conv_launch<MODE_F32, 1, 64, 3, true, true>(ConvArgs, hipStream_t);
#elif SDP_INST == 6   // F3
template hipError_t conv_launch<MODE_F32X3, 1, 64, 3, true, true>(ConvArgs, hipStream_t);
#elif SDP_INST == 7   // F3
template hipError_t conv_launch<MODE_BF16, 1, 64, 3, true, true>(ConvArgs, hipStream_t);
#elif SDP_INST == 8   // F4: the pooled 1x1 shortcut (training)
template hipError_t conv_launch<MODE_F32X3, 1, 64, 1, true, false>(ConvArgs, hipStream_t);
#elif SDP_INST == 9   // F4
template hipError_t conv_launch<MODE_BF16, 1, 64, 1, true, false>(ConvArgs, hipStream_t);
#elif SDP_INST == 10   // F5: the 1x1 shortcut on the pre-pooled input (sampling)
template hipError_t conv_launch<MODE_F32, 1, 64, 1, false, false>(ConvArgs, hipStream_t);
#elif SDP_INST == 11   // F5
template hipError_t conv_launch<MODE_F32X3, 1, 64, 1, false, false>(ConvArgs, hipStream_t);
#elif SDP_INST == 12   // F5
template hipError_t conv_launch<MODE_BF16, 1, 64, 1, false, false>(ConvArgs, hipStream_t);
#elif SDP_INST == 13   // F6/F7: 8 x 16 tiles on 4-wave 128-Cout workgroups (256 Cout: a pair per tile)
template hipError_t conv_launch_nj2<MODE_F32X3, false, 4>(ConvArgs, hipStream_t);
#elif SDP_INST == 14   // F6/F7
template hipError_t conv_launch_nj2<MODE_F32X3, true, 4>(ConvArgs, hipStream_t);
#elif SDP_INST == 15   // F6/F7
template hipError_t conv_launch_nj2<MODE_BF16, false, 4>(ConvArgs, hipStream_t);
#elif SDP_INST == 16   // F6/F7
template hipError_t conv_launch_nj2<MODE_BF16, true, 4>(ConvArgs, hipStream_t);
#elif SDP_INST == 17   // F8: 8 x 16 tiles on 8-wave 256-Cout workgroups
template hipError_t conv_launch_nj2<MODE_BF16, false, 8>(ConvArgs, hipStream_t);
#elif SDP_INST == 18   // F8
template hipError_t conv_launch_nj2<MODE_BF16, true, 8>(ConvArgs, hipStream_t);
#elif SDP_INST == 19   // F9: the ConvMeanPool 3x3 as a 4x4 stride-2 conv
template hipError_t conv_launch_s2<MODE_F32X3>(ConvArgs, hipStream_t);
#elif SDP_INST == 20   // F9
template hipError_t conv_launch_s2<MODE_BF16>(ConvArgs, hipStream_t);
#elif SDP_INST == 21   // F10: the bf16 tape (IO16)
template hipError_t conv_launch<MODE_BF16, 1, 64, 1, true, false, true>(ConvArgs, hipStream_t);
#elif SDP_INST == 22   // F10
template hipError_t conv_launch<MODE_BF16, 1, 64, 3, true, true, true>(ConvArgs, hipStream_t);
#elif SDP_INST == 23   // F10
template hipError_t conv_launch_nj2<MODE_BF16, false, 4, true>(ConvArgs, hipStream_t);
#elif SDP_INST == 24   // F10
template hipError_t conv_launch_nj2<MODE_BF16, true, 4, true>(ConvArgs, hipStream_t);
#elif SDP_INST == 25   // D1: the 1x1 shortcut
template hipError_t dgrad_launch<MODE_F32X3, 2, 32, 1, false>(ConvArgs, hipStream_t);
#elif SDP_INST == 26   // D1
template hipError_t dgrad_launch<MODE_BF16, 2, 32, 1, false>(ConvArgs, hipStream_t);
#elif SDP_INST == 27   // D2: the zero-padded 3x3
template hipError_t dgrad_launch<MODE_F32X3, 2, 32, 3, true>(ConvArgs, hipStream_t);
#elif SDP_INST == 28   // D2
template hipError_t dgrad_launch<MODE_BF16, 2, 32, 3, true>(ConvArgs, hipStream_t);
#elif SDP_INST == 29   // D3: circular 3x3, 128 input channels
template hipError_t dgrad_launch_nj2<MODE_F32X3, 4>(ConvArgs, hipStream_t);
#elif SDP_INST == 30   // D3
template hipError_t dgrad_launch_nj2<MODE_BF16, 4>(ConvArgs, hipStream_t);
#elif SDP_INST == 31   // D4: circular 3x3, 256 input channels, fp32x3 (transposed epilogue)
template hipError_t dgrad_launch<MODE_F32X3, 1, 16, 3, false>(ConvArgs, hipStream_t);
#elif SDP_INST == 32   // D5: circular 3x3, 256 input channels, bf16
template hipError_t dgrad_launch_nj2<MODE_BF16, 8>(ConvArgs, hipStream_t);
#elif SDP_INST == 33   // D6: the bf16 tape (IO16)
template hipError_t dgrad_launch<MODE_BF16, 2, 32, 1, false, true>(ConvArgs, hipStream_t);
#elif SDP_INST == 34   // D6
template hipError_t dgrad_launch<MODE_BF16, 2, 32, 3, true, true>(ConvArgs, hipStream_t);
#elif SDP_INST == 35   // D6
template hipError_t dgrad_launch_nj2<MODE_BF16, 4, true>(ConvArgs, hipStream_t);
#else
#error "conv_inst.hip: SDP_INST names no row of the table"
#endif

}  // namespace sdp
