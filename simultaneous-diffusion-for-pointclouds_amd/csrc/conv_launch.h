// Launchers of conv_mfma_kernel, one per kernel shape.  Declared here, defined in conv_inst.hip, which also
// holds the table of what is built: one explicit instantiation per row, one object per row (Makefile:
// -DSDP_INST=<row id>), so `make -j` builds the kernels in parallel instead of in two translation units.
// conv.hip and conv_bwd.hip dispatch to the rows of that table only; the library links with -z defs, so a
// dispatched launcher without a row is a link error.
#pragma once
#include "common.h"

namespace sdp {

// forward conv (conv.hip dispatch) on 64-Cout waves: 8 x 32 / 4 x 32 tiles in exact fp32, the 2 x 64 tiles of the
// pooled and 1x1 layers in every mode (conv_inst.hip F1 - F5, F10)
template <int MODE, int WM, int TC, int KS, bool POOL, bool PELU, bool IO16 = false>
hipError_t conv_launch(ConvArgs a, hipStream_t st);

// forward of the 8 x 16 3x3 tiles on 32-Cout waves, two per SIMD (conv_inst.hip F6 - F8, F10): NW = 4
// (128 Cout per workgroup, two per CU) or 8 (256 Cout, one per CU)
template <int MODE, bool PELU, int NW, bool IO16 = false>
hipError_t conv_launch_nj2(ConvArgs a, hipStream_t st);

// forward of the ConvMeanPool 3x3 as a 4x4 stride-2 conv (conv_kernel.h S2; ConvArgs::s2) on 8 x 16 output tiles and
// 32-Cout waves: 4-wave 128-Cout workgroups, the 256 Couts as a pair per tile (conv_inst.hip F9)
template <int MODE>
hipError_t conv_launch_s2(ConvArgs a, hipStream_t st);

// data gradient of the 8 x 16 circular 3x3 tiles on 32-Cout waves, two per SIMD (conv_inst.hip D3, D5, D6)
template <int MODE, int NW, bool IO16 = false>
hipError_t dgrad_launch_nj2(ConvArgs a, hipStream_t st);

// data gradient (conv_bwd.hip dispatch) on 64-Cout waves: the 8 x 32 tiles of the 1x1 and zero-padded layers, the
// 8 x 16 tiles of the fp32x3 256-channel layers (conv_inst.hip D1, D2, D4, D6)
template <int MODE, int WM, int TC, int KS, bool ZP, bool IO16 = false>
hipError_t dgrad_launch(ConvArgs a, hipStream_t st);

// IO16 (the bf16 training tape) launchers exist for MODE_BF16 and the rows F10 / D6 only

}  // namespace sdp
