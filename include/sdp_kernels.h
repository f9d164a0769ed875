/*
 * sdp_kernels.h -- per-kernel TEST AND DIAGNOSTIC entries of libsdp.so.
 *
 * NOT part of the stable ABI (that is sdp.h, prefix sdp_): these sdpk_* entries expose the library's
 * internal kernel launchers (csrc/kernels.h) one at a time, so that a test can compare one kernel with a
 * reference of the same operation.  They may change or disappear with the kernels they wrap.
 *
 * Conventions (those of sdp.h): every pointer is a DEVICE pointer owned by the caller, every call is
 * enqueued on the given hipStream_t (passed as void*) and never synchronises, the return value is 0 = OK or
 * < 0 = error with the message in sdp_last_error().  The wrappers only copy their flat arguments into the
 * launcher's argument struct: the launcher's own validation is the only shape check, and a shape it
 * rejects comes back as an error, never as a launch.
 *
 * Tensors are NHWC.  "h16" / "io16": the activation and gradient tensors of the call hold bf16 elements
 * (the bf16 training tape); parameters, statistics and coefficient tables stay float32.
 */
#ifndef SDP_KERNELS_H
#define SDP_KERNELS_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* weight packings of sdpk_pack_weights (out: Cout * Cin * k * k 32-bit slots; SDPK_PACK_POOL4X4: Cout * Cin * 16) */
enum sdpk_packing {
  SDPK_PACK_FRAG = 0,     /* "#frag":    32x32 fragment order, the exact-fp32 forward                  */
  SDPK_PACK_FRAG16 = 3,   /* "#frag16":  16x16 fragment order, the forward of the bf16 modes           */
  SDPK_PACK_DFRAG16 = 4,  /* "#dfrag16": flipped + transposed, 16x16 order, the data gradient          */
  SDPK_PACK_POOL4X4 = 5   /* "#pool4x4": zero-padded 3x3 + 2x2 mean merged into a 4x4 stride-2 conv    */
};
/* w: float32 [Cout][Cin][k][k]; mode: enum sdp_precision; desc_scratch: 64 bytes of device memory that must
 * stay untouched until the stream has run the call (it receives the launch descriptor) */
int sdpk_pack_weights(const float* w, uint32_t* out, int Cout, int Cin, int k, int mode, int packing,
                      void* desc_scratch, void* stream);

/* one forward or data-gradient convolution launch: the fields of csrc/common.h ConvArgs that a caller sets
 * (the launcher fills the tile bookkeeping) */
typedef struct sdpk_conv {
  const void* in;        /* [B][H][W][Cin]                                                              */
  const void* wf;        /* SDPK_PACK_FRAG weights (exact fp32) or null                                 */
  const void* wf16;      /* SDPK_PACK_FRAG16 / DFRAG16 / POOL4X4 weights (bf16 modes) or null           */
  const float* bias;     /* [Cout] or null                                                              */
  void* out;             /* [B][Ho][Wo][Cout]; Ho, Wo = H, W, or H/2, W/2 when pooled or s2             */
  const void* res;       /* residual, layout of out, or null                                            */
  void* out2;            /* second output = value + res2, or null                                       */
  const void* res2;
  const void* up;        /* [B][H/2][W/2][Cout]: bilinear (align_corners) upsample-add, or null         */
  const float* pro_ss;   /* [B][Cin][2] prologue (scale, shift), or the identity table with stride 0   */
  int ss_bstride;        /* floats between the rows of consecutive images                               */
  float* stats;          /* [B][groups][Cout][2] per-group (mean, M2) of the output, or null           */
  int B, H, W, Cin, Cout;
  int dil, circular, pro_mode, epi_elu;   /* pro_mode: 0 none, 1 ELU, 2 affine + ELU                    */
  const void* aux;       /* data gradient: the operand of elu' (layout of out)                          */
  const float* epi_ss;   /* dact 3: [B][Cout][2] (scale, shift) applied to aux first                    */
  int dact;              /* 0 off, 1 aux = pre-activation, 2 aux = ELU output, 3 aux = IN++ input       */
  int io16;
  int s2;                /* 1: the 4x4 stride-2 form (wf16 = SDPK_PACK_POOL4X4)                          */
} sdpk_conv;
int sdpk_conv_mfma(int mode, const sdpk_conv* c, int ks, int pool, void* stream);
/* in = dy [B][H][W][Cin = forward Cout], wf16 = SDPK_PACK_DFRAG16, out = dx [B][H][W][Cout = forward Cin] */
int sdpk_conv_dgrad(int mode, const sdpk_conv* c, int ks, void* stream);

/* one weight-gradient launch (csrc/common.h WgradArgs) + its split reduction */
typedef struct sdpk_wgrad {
  const void* in;        /* forward input [B][H][W][Cin], before the prologue                           */
  const float* pro_ss;
  int ss_bstride;
  int pro_mode;
  const void* dy;        /* [B][H][W][Cout]                                                             */
  float* part;           /* split partials, sdpk_wgrad_part_floats(sdpk_wgrad_splits(...), ...) floats  */
  size_t part_floats;
  float* bpart;          /* bias partials [splits][Cout], or null                                       */
  int B, H, W, Cin, Cout, dil, circular;
} sdpk_wgrad;
/* out: float32 [Cout][Cin][ks][ks]; bias_out: [Cout] or null; accumulate: add to out / bias_out */
int sdpk_conv_wgrad(int mode, const sdpk_wgrad* g, int ks, float* out, float* bias_out, int accumulate, int h16,
                    void* stream);
int sdpk_wgrad_splits(int B, int H, int W, int dil, int Cin, int Cout, int ks);
size_t sdpk_wgrad_part_floats(int splits, int Cin, int Cout, int ks);

/* MaxPool2d(5, 1, 2); idx (or null): one byte per element, the window position 5 * row + column of the maximum */
int sdpk_maxpool5(const void* in, void* out, uint8_t* idx, int B, int H, int W, int C, int h16, void* stream);
/* dst = (res or 0) + the adjoint of the pooling that wrote idx, applied to dp */
int sdpk_maxpool5_backward(const uint8_t* idx, const void* dp, const void* res, void* dst, int B, int H, int W, int C,
                           int h16, void* stream);
/* 2x2 mean: out [B][H/2][W/2][C] (float32 only) */
int sdpk_avgpool2(const float* in, float* out, int B, int H, int W, int C, void* stream);
/* adjoint of the 2x2 mean: dst [B][H][W][C] = dout [B][H/2][W/2][C] / 4 */
int sdpk_unpool(const void* dout, void* dst, int B, int H, int W, int C, int h16, void* stream);
/* adjoint of the bilinear (align_corners) 2x upsampling: g [B][H][W][C] -> dlow [B][H/2][W/2][C] */
int sdpk_upsample_backward(const void* g, void* dlow, int B, int H, int W, int C, int accumulate, int h16, void* stream);
/* dst = dy * elu'(y) (+ res), y = the ELU's output; n elements, a multiple of 4 */
int sdpk_elu_backward_post(const void* dy, const void* y, const void* res, void* dst, size_t n, int h16, void* stream);
int sdpk_add_tensors(const void* a, const void* b, void* dst, size_t n, int h16, void* stream);

/* InstanceNorm++: stats [B][T][C][2] of (mean, M2) over cnt values each -> ss [B][C][2] (scale, shift) and, when
 * nst is given, [B][C][4] (mean, rstd, normalised channel mean, 1 / sqrt(var of the means + eps));
 * scratch: B * C * 16 bytes */
int sdpk_inpp_finalize(const float* stats, int B, int T, float cnt, int C, const float* alpha, const float* gamma,
                       const float* beta, float* ss, float* nst, void* scratch, void* stream);
/* out = (r1 or 0) + (r2 or 0) + d IN++(h) applied to g; part: B * (HW / 512) * C * 2 floats, coef: B * C * 4,
 * ppart: B * C * 3; dalpha, dgamma, dbeta: [C], overwritten */
int sdpk_inpp_backward(const void* g, const void* h, const float* nst, const float* alpha, const float* gamma, int B,
                       int HW, int C, float* part, float* coef, float* ppart, float* dalpha, float* dgamma, float* dbeta,
                       const void* r1, const void* r2, void* out, int h16, void* stream);

/* ---- the head and the tail of the score net (aux.hip, train_aux.hip).  mode: enum sdp_precision */
/* x: [B][2][H][W] image (NCHW float32); w: [128][4][3][3]; bias: [128]; out: [B][H][W][128] (bf16 elements when
 * h16); stats: [B][H*W/64][128][2] (mean, M2) of groups of 64 pixels.  W a multiple of 128; h16 in bf16 mode only */
int sdpk_begin_conv(const float* x, const float* w, const float* bias, void* out, float* stats, int B, int H, int W,
                    int mode, int h16, void* stream);
/* the fused Langevin update of sdpk_end_conv: csrc/langevin.h LangevinArgs */
typedef struct sdpk_langevin {
  float* x;              /* [B][2][H][W], updated in place                                              */
  const float* ref;      /* [B][2][H][W]                                                                */
  const int32_t* mask;   /* [B][2][H][W]                                                                */
  const float* noise;    /* nullable: Philox4x32-10(seed, offset + i / 4)                               */
  uint64_t seed, offset;
  float step_size, noise_scale, grad_ref;
  int nan_to_num;
  float* lik_out;        /* nullable                                                                    */
  uint32_t* absmax_bits; /* nullable: atomicMax of the float bits of |x_new[:, 0]|                      */
} sdpk_langevin;
/* in: [B][H][W][Cin] (bf16 elements when h16); ss: [B][Cin][2] (scale, shift); w: [2][Cin][3][3]; bias: [2];
 * out: [B][2][H][W] = (conv3x3_zero(ELU(in * scale + shift), w) + bias) / sigmas[labels[b]] (nullable with lg);
 * labels: int64 [B].  Cin = 128; bf16 modes: 16 x 32 tiles, else (and fp32) the direct kernel on 4 x 64 tiles */
int sdpk_end_conv(const void* in, const float* ss, const float* w, const float* bias, const float* sigmas,
                  const int64_t* labels, float* out, int B, int H, int W, int Cin, int mode, int h16,
                  const sdpk_langevin* lg_or_null, void* stream);
/* dw [128][4][3][3], db [128]: gradients of the begin conv for dy [B][H][W][128] (bf16 elements when h16);
 * part: sdpk_head_wgrad_part_floats(B, H, W) floats.  H a multiple of 8, W of 64 */
int sdpk_begin_conv_wgrad(const float* x, const void* dy, float* part, float* dw, float* db, int B, int H, int W, int h16,
                          void* stream);
/* dscore [B][2][H][W]; o, ss: the forward's in, ss; g [B][H][W][128] = d loss / d (o * scale + shift) (o, g: bf16
 * elements when h16); dw [2][128][3][3], db [2]; part as above.  H a multiple of 16, W of 64 */
int sdpk_end_conv_backward(const float* dscore, const float* sigmas, const int64_t* labels, const float* w, const void* o,
                           const float* ss, void* g, float* part, float* dw, float* db, int B, int H, int W, int h16,
                           void* stream);
size_t sdpk_head_wgrad_part_floats(int B, int H, int W);

/* ---- the data front end (projection.hip) */
/* the row-sequential sky / obfuscation scan of sdp_range_project (datasets/lidar_utils.py:283-306), one launch:
 * xy: float64 [H][W], the flipped planar-range image (2057.701 where empty); obf, sky: u8 [H][W], sky all 0 as the
 * reference clears it.  3 <= H, 1 <= W <= 1024 */
int sdpk_range_sky_scan(const double* xy, int H, int W, uint8_t* obf, uint8_t* sky, void* stream);

/* ---- the shared primitives of the point-cloud back end (csrc/device_prims.h, csrc/radix_sort.hip) */
/* one workgroup: exclusive scan of data[0..n) in place, the sum to *total; 4096 counts per iteration.  n >= 0 */
int sdpk_block_scan(int32_t* data, int n, int32_t* total, void* stream);
/* Stable LSD radix sort, 8-bit digits 0 .. passes-1, tiles of 1024 elements, of the keys in key0 (with the values
 * in val0; val0 = val1 = null: keys only) between the ping/pong buffers of `capacity` elements each.
 * tile_cnt: 256 * ceil(capacity / 1024) int32 of scratch.  params: DEVICE int32 [3] = the element count
 * (0 <= n <= capacity, the caller's duty), the key width in bits (a pass at or beyond it moves nothing) and a
 * flag, non-zero = do nothing.  state: DEVICE int32 [SDPK_RADIX_STATE_INTS], zeroed by the caller (csrc/radix_sort.h
 * RadixState); afterwards state[SDPK_RADIX_STATE_RESULT] tells which buffer (0 | 1) holds the sorted elements */
#define SDPK_RADIX_STATE_INTS 18
#define SDPK_RADIX_STATE_RESULT 17
int sdpk_radix_sort(uint64_t* key0, uint64_t* key1, uint32_t* val0, uint32_t* val1, int32_t* tile_cnt, int64_t capacity,
                    const int32_t* params, int32_t* state, int passes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SDP_KERNELS_H */
