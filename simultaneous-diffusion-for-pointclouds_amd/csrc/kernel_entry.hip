// Test and diagnostic entries over the kernel launchers of kernels.h (include/sdp_kernels.h, prefix
// sdpk_): one C wrapper per launcher, outside the stable sdp_* ABI.  A wrapper copies its flat
// arguments into the launcher's struct and calls it -- the launcher's validation is the only shape
// check -- and reports a failure through sdp_last_error().
#include <string>

#include "../../include/sdp_kernels.h"
#include "capi.h"
#include "kernels.h"
#include "radix_sort.h"

using namespace sdp;

namespace {

hipStream_t S(void* stream) { return reinterpret_cast<hipStream_t>(stream); }
const float* F(const void* p) { return reinterpret_cast<const float*>(p); }
float* F(void* p) { return reinterpret_cast<float*>(p); }

int done(hipError_t e, const char* what, const char* why = nullptr) {
  if (e == hipSuccess) return 0;
  return sdp_fail(std::string(what) + ": " + (why ? why : hipGetErrorString(e)));
}

ConvArgs conv_args(const sdpk_conv& c) {
  ConvArgs a{};
  a.in = F(c.in);
  a.wf = reinterpret_cast<const uint4*>(c.wf);
  a.wf16 = reinterpret_cast<const uint4*>(c.wf16);
  a.bias = c.bias;
  a.out = F(c.out);
  a.res = F(c.res);
  a.out2 = F(c.out2);
  a.res2 = F(c.res2);
  a.up = F(c.up);
  a.pro_ss = c.pro_ss;
  a.ss_bstride = c.ss_bstride;
  a.stats = c.stats;
  a.B = c.B;
  a.H = c.H;
  a.W = c.W;
  a.Cin = c.Cin;
  a.Cout = c.Cout;
  a.dil = c.dil;
  a.circular = c.circular;
  a.pro_mode = c.pro_mode;
  a.epi_elu = c.epi_elu;
  a.aux = F(c.aux);
  a.epi_ss = c.epi_ss;
  a.dact = c.dact;
  a.io16 = c.io16;
  a.s2 = c.s2;
  return a;
}

}  // namespace

extern "C" {

int sdpk_pack_weights(const float* w, uint32_t* out, int Cout, int Cin, int k, int mode, int packing, void* desc_scratch,
                      void* stream) {
  if (!w || !out || !desc_scratch) return sdp_fail("sdpk_pack_weights: null argument");
  if (packing != SDPK_PACK_FRAG && packing != SDPK_PACK_FRAG16 && packing != SDPK_PACK_DFRAG16 &&
      packing != SDPK_PACK_POOL4X4)
    return sdp_fail("sdpk_pack_weights: unknown packing");
  if (packing == SDPK_PACK_POOL4X4 && k != 3) return sdp_fail("sdpk_pack_weights: the 4x4 stride-2 packing merges a 3x3");
  const int nt = packing == SDPK_PACK_POOL4X4 ? 16 : k * k;
  const PackDesc d{w, out, Cout, Cin, nt, packing, 0};
  static_assert(sizeof(PackDesc) <= 64, "sdpk_pack_weights: desc_scratch holds one descriptor");
  // (a pageable source: the copy is staged before the call returns, so `d` may go out of scope)
  hipError_t e = hipMemcpyAsync(desc_scratch, &d, sizeof d, hipMemcpyHostToDevice, S(stream));
  if (e != hipSuccess) return done(e, "sdpk_pack_weights");
  return done(pack_weights_multi(reinterpret_cast<const PackDesc*>(desc_scratch), 1, (size_t)Cout * Cin * nt, mode,
                                 S(stream)),
              "sdpk_pack_weights");
}

int sdpk_conv_mfma(int mode, const sdpk_conv* c, int ks, int pool, void* stream) {
  if (!c) return sdp_fail("sdpk_conv_mfma: null argument");
  const char* why = nullptr;
  return done(conv_mfma(mode, conv_args(*c), ks, pool != 0, S(stream), &why), "sdpk_conv_mfma", why);
}

int sdpk_conv_dgrad(int mode, const sdpk_conv* c, int ks, void* stream) {
  if (!c) return sdp_fail("sdpk_conv_dgrad: null argument");
  const char* why = nullptr;
  return done(conv_dgrad(mode, conv_args(*c), ks, S(stream), &why), "sdpk_conv_dgrad", why);
}

int sdpk_conv_wgrad(int mode, const sdpk_wgrad* g, int ks, float* out, float* bias_out, int accumulate, int h16,
                    void* stream) {
  if (!g) return sdp_fail("sdpk_conv_wgrad: null argument");
  WgradArgs a{};
  a.in = F(g->in);
  a.pro_ss = g->pro_ss;
  a.ss_bstride = g->ss_bstride;
  a.pro_mode = g->pro_mode;
  a.dy = F(g->dy);
  a.part = g->part;
  a.part_floats = g->part_floats;
  a.bpart = g->bpart;
  a.B = g->B;
  a.H = g->H;
  a.W = g->W;
  a.Cin = g->Cin;
  a.Cout = g->Cout;
  a.dil = g->dil;
  a.circular = g->circular;
  const char* why = nullptr;
  return done(conv_wgrad(mode, a, ks, out, bias_out, accumulate, S(stream), &why, h16 != 0), "sdpk_conv_wgrad", why);
}

int sdpk_wgrad_splits(int B, int H, int W, int dil, int Cin, int Cout, int ks) {
  return wgrad_splits(B, H, W, dil, Cin, Cout, ks);
}

size_t sdpk_wgrad_part_floats(int splits, int Cin, int Cout, int ks) { return wgrad_part_floats(splits, Cin, Cout, ks); }

int sdpk_maxpool5(const void* in, void* out, uint8_t* idx, int B, int H, int W, int C, int h16, void* stream) {
  return done(maxpool5(F(in), F(out), B, H, W, C, S(stream), idx, h16 != 0), "sdpk_maxpool5");
}

int sdpk_maxpool5_backward(const uint8_t* idx, const void* dp, const void* res, void* dst, int B, int H, int W, int C,
                           int h16, void* stream) {
  return done(maxpool5_backward(idx, F(dp), F(res), F(dst), B, H, W, C, S(stream), h16 != 0), "sdpk_maxpool5_backward");
}

int sdpk_avgpool2(const float* in, float* out, int B, int H, int W, int C, void* stream) {
  return done(avgpool2(in, out, B, H, W, C, S(stream)), "sdpk_avgpool2");
}

int sdpk_unpool(const void* dout, void* dst, int B, int H, int W, int C, int h16, void* stream) {
  return done(unpool(F(dout), F(dst), B, H, W, C, S(stream), h16 != 0), "sdpk_unpool");
}

int sdpk_upsample_backward(const void* g, void* dlow, int B, int H, int W, int C, int accumulate, int h16, void* stream) {
  return done(upsample_backward(F(g), F(dlow), B, H, W, C, accumulate, S(stream), h16 != 0), "sdpk_upsample_backward");
}

int sdpk_elu_backward_post(const void* dy, const void* y, const void* res, void* dst, size_t n, int h16, void* stream) {
  return done(elu_backward_post(F(dy), F(y), F(res), F(dst), n, S(stream), h16 != 0), "sdpk_elu_backward_post");
}

int sdpk_add_tensors(const void* a, const void* b, void* dst, size_t n, int h16, void* stream) {
  return done(add_tensors(F(a), F(b), F(dst), n, S(stream), h16 != 0), "sdpk_add_tensors");
}

int sdpk_inpp_finalize(const float* stats, int B, int T, float cnt, int C, const float* alpha, const float* gamma,
                       const float* beta, float* ss, float* nst, void* scratch, void* stream) {
  return done(inpp_finalize(stats, B, T, cnt, C, alpha, gamma, beta, ss, S(stream), nst, scratch), "sdpk_inpp_finalize");
}

int sdpk_inpp_backward(const void* g, const void* h, const float* nst, const float* alpha, const float* gamma, int B,
                       int HW, int C, float* part, float* coef, float* ppart, float* dalpha, float* dgamma, float* dbeta,
                       const void* r1, const void* r2, void* out, int h16, void* stream) {
  return done(inpp_backward(F(g), F(h), nst, alpha, gamma, B, HW, C, part, coef, ppart, dalpha, dgamma, dbeta, F(r1), F(r2),
                            F(out), S(stream), h16 != 0),
              "sdpk_inpp_backward");
}

int sdpk_begin_conv(const float* x, const float* w, const float* bias, void* out, float* stats, int B, int H, int W,
                    int mode, int h16, void* stream) {
  return done(begin_conv(x, w, bias, F(out), stats, B, H, W, S(stream), mode, h16 != 0), "sdpk_begin_conv");
}

int sdpk_end_conv(const void* in, const float* ss, const float* w, const float* bias, const float* sigmas,
                  const int64_t* labels, float* out, int B, int H, int W, int Cin, int mode, int h16,
                  const sdpk_langevin* lg, void* stream) {
  LangevinArgs la{};
  if (lg) {
    la.x = lg->x;
    la.ref = lg->ref;
    la.mask = lg->mask;
    la.noise = lg->noise;
    la.seed = lg->seed;
    la.offset = lg->offset;
    la.step = lg->step_size;
    la.nscale = lg->noise_scale;
    la.gref = lg->grad_ref;
    la.n2n = lg->nan_to_num;
    la.lik = lg->lik_out;
    la.absmax = lg->absmax_bits;
  }
  return done(end_conv(F(in), ss, w, bias, sigmas, labels, out, B, H, W, Cin, S(stream), lg ? &la : nullptr, mode, h16 != 0),
              "sdpk_end_conv");
}

int sdpk_begin_conv_wgrad(const float* x, const void* dy, float* part, float* dw, float* db, int B, int H, int W, int h16,
                          void* stream) {
  return done(begin_conv_wgrad(x, F(dy), part, dw, db, B, H, W, S(stream), h16 != 0), "sdpk_begin_conv_wgrad");
}

int sdpk_end_conv_backward(const float* dscore, const float* sigmas, const int64_t* labels, const float* w, const void* o,
                           const float* ss, void* g, float* part, float* dw, float* db, int B, int H, int W, int h16,
                           void* stream) {
  return done(end_conv_backward(dscore, sigmas, labels, w, F(o), ss, F(g), part, dw, db, B, H, W, S(stream), h16 != 0),
              "sdpk_end_conv_backward");
}

size_t sdpk_head_wgrad_part_floats(int B, int H, int W) { return head_wgrad_part_floats(B, H, W); }

int sdpk_range_sky_scan(const double* xy, int H, int W, uint8_t* obf, uint8_t* sky, void* stream) {
  return done(range_sky_scan(xy, H, W, obf, sky, S(stream)), "sdpk_range_sky_scan");
}

int sdpk_block_scan(int32_t* data, int n, int32_t* total, void* stream) {
  if (!data || !total || n < 0) return sdp_fail("sdpk_block_scan: null argument or n < 0");
  return done(block_scan(data, n, total, S(stream)), "sdpk_block_scan");
}

int sdpk_radix_sort(uint64_t* key0, uint64_t* key1, uint32_t* val0, uint32_t* val1, int32_t* tile_cnt, int64_t capacity,
                    const int32_t* params, int32_t* state, int passes, void* stream) {
  static_assert(sizeof(RadixState) == SDPK_RADIX_STATE_INTS * sizeof(int32_t) &&
                    offsetof(RadixState, result) == SDPK_RADIX_STATE_RESULT * sizeof(int32_t),
                "sdp_kernels.h describes RadixState");
  if (!key0 || !key1 || !tile_cnt || !params || !state || (val0 == nullptr) != (val1 == nullptr))
    return sdp_fail("sdpk_radix_sort: null argument");
  if (capacity < 1 || capacity > (1 << 30) || passes < 0 || passes > RADIX_MAX_PASSES)
    return sdp_fail("sdpk_radix_sort: capacity must be in [1, 2^30] and passes in [0, 8]");
  RadixArgs a{};
  a.key0 = key0;
  a.key1 = key1;
  a.val0 = val0;
  a.val1 = val1;
  a.tile_cnt = tile_cnt;
  a.ntiles = (int)((capacity + RADIX_TILE - 1) / RADIX_TILE);
  a.n = params;
  a.bits = params + 1;
  a.skip = params + 2;
  a.state = reinterpret_cast<RadixState*>(state);
  radix_sort(a, passes, S(stream));
  return launch_status("sdpk_radix_sort");
}

}  // extern "C"
