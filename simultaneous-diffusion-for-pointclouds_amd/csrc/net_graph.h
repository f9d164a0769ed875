// The forward of NCSN_LiDAR_small (LiDARGen/models/ncsnv2.py:420-518) over the libsdp kernels, written
// once: the ConvArgs of a forward conv, the ResidualBlock / RCU / CRP / RefineBlock wiring, the per-norm
// tile counts and the layer order.  The sampling forward (net.hip, Fwd) and the training forward that
// keeps its tape (train.hip, TrainPlan) are the two runtimes RT this walker runs on.  A runtime provides
//   net, B, st, stats, mv   the handle, batch, stream, statistics tiles and inpp_finalize scratch
//   kTraining, dry, h16     which of the two it is; launch nothing (training's sizing run); bf16 tape
//   alloc / release         activation memory (below)
//   keep, norm_out, argmax_out   the tape (training; sampling keeps nothing and shares one ss table)
//   launch, launch_conv     enqueue (sampling: under the event-pair profiler; training: not when dry)
//
// Where the two forwards differ the walker branches on RT::kTraining, each place marked "training:" /
// "sampling:" (DESIGN.md lists them): the ConvMeanPool block, the statistics tiles of res2.1.normalize1,
// the statistics of res4.1's conv2, the maxpool argmax, the per-norm tables, io16 / h16 and the fused
// Langevin update.  Everything else is the graph.
//
// Ownership of activations: a block releases every temporary it allocated and returns its output
// unreleased; the caller releases a block's inputs after their last reader.  Training never reuses
// memory (its release is a no-op: the backward reads the tape); sampling recycles a fixed pool of slots,
// so how many it needs depends on this file alone, not on the shape.
#pragma once
#include <string>

#include "net_internal.h"

namespace sdp {

// an NHWC activation: float32, or bf16 elements on the bf16 training tape
struct Act {
  float* p;
  int H, W, C;
};

struct NormOut {
  float* ss;    // (scale, shift) per (image, channel): the consuming conv's prologue
  float* nst;   // statistics the IN++ backward reads (training), else null
};

struct ConvOpt {
  int pro = PRO_NONE;          // prologue
  const float* ss = nullptr;   // PRO_AFFINE_ELU: the norm's (scale, shift)
  bool bias = true;
  const float* res = nullptr;
  const float* up = nullptr;
  float* out2 = nullptr;
  const float* res2 = nullptr;
  bool epi_elu = false;
  bool stats = false;
  int dil = 1;
  bool circular = true;
  bool pool = false;
  bool s2 = false;             // the ConvMeanPool 3x3 as one 4x4 stride-2 conv on the merged weights
};

template <class RT>
struct NetGraph {
  RT& rt;

  static int tiles(const Act& t) { return t.H * t.W / 128; }
  Act like(const Act& t) { return rt.alloc(t.H, t.W, t.C); }
  static std::string at(const Act& t) { return " @" + std::to_string(t.H) + "x" + std::to_string(t.W); }

  void conv(const Act& in, const std::string& wkey, const Act& out, const ConvOpt& o) {
    const sdp_net* net = rt.net;
    const auto& hp = net->host.at(wkey + ".weight");
    if ((int)hp.shape[1] != in.C || (int)hp.shape[0] != out.C) throw std::runtime_error("conv shape mismatch " + wkey);
    if (rt.dry) return;
    const bool f32 = net->mode == MODE_F32;
    ConvArgs a{};
    a.in = in.p;
    // forward weights: "#frag16" in the bf16 modes (16x16 MFMAs), "#frag" for exact fp32 (32x32)
    a.wf = f32 ? reinterpret_cast<const uint4*>(net->P(wkey + ".weight#frag")) : nullptr;
    a.wf16 = f32 ? nullptr : reinterpret_cast<const uint4*>(net->P(wkey + (o.s2 ? ".weight#pool4x4" : ".weight#frag16")));
    a.s2 = o.s2 ? 1 : 0;
    a.bias = o.bias ? net->P(wkey + ".bias") : nullptr;
    a.out = out.p;
    a.res = o.res;
    a.out2 = o.out2;
    a.res2 = o.res2;
    a.up = o.up;
    a.pro_ss = o.pro == PRO_AFFINE_ELU ? o.ss : net->P("#ident_ss");
    a.ss_bstride = o.pro == PRO_AFFINE_ELU ? 2 * in.C : 0;
    a.stats = o.stats ? rt.stats : nullptr;
    a.B = rt.B;
    a.H = in.H;
    a.W = in.W;
    a.Cin = in.C;
    a.Cout = out.C;
    a.dil = o.dil;
    a.circular = o.circular ? 1 : 0;
    a.pro_mode = o.pro;
    a.epi_elu = o.epi_elu ? 1 : 0;
    a.io16 = rt.h16 ? 1 : 0;   // training: the bf16 tape
    rt.launch_conv(a, (int)hp.shape[2], o, wkey, in, out);
  }

  // statistics of the last stats-writing conv (T tiles of cnt pixels) -> (scale, shift) of InstanceNorm2dPlus `nkey`
  const float* norm(const std::string& nkey, int T, float cnt, int C) {
    // training: a fresh ss and nst per norm, kept as "<nkey>#ss" / "<nkey>#nst"; sampling: one shared ss, no nst
    const NormOut n = rt.norm_out(nkey, C);
    const int B = rt.B;
    rt.launch("inpp_finalize", "inpp_finalize C" + std::to_string(C), (double)B * T * C * 8 + (double)B * C * 8, [&] {
      const sdp_net* net = rt.net;
      return inpp_finalize(rt.stats, B, T, cnt, C, net->P(nkey + ".alpha"), net->P(nkey + ".gamma"), net->P(nkey + ".beta"),
                           n.ss, rt.st, n.nst, rt.mv);
    });
    return n.ss;
  }

  // ResidualBlock.forward (layers.py:443-456) on x, whose statistics lie in x_tiles tiles of x_cnt pixels;
  // its conv2 writes the statistics of the output when want_stats
  Act resblock(const std::string& k, const Act& x, bool down, int dil, bool want_stats, int x_tiles, float x_cnt) {
    if constexpr (RT::kTraining) rt.keep(k + ".x", x);
    ConvOpt o1;
    o1.pro = PRO_AFFINE_ELU;
    o1.ss = norm(k + ".normalize1", x_tiles, x_cnt, x.C);
    o1.stats = true;
    o1.dil = dil;
    Act h1 = like(x);
    conv(x, k + ".conv1", h1, o1);
    if constexpr (RT::kTraining) rt.keep(k + ".h1", h1);
    ConvOpt o2;
    o2.pro = PRO_AFFINE_ELU;
    o2.ss = norm(k + ".normalize2", tiles(h1), 128.f, h1.C);
    o2.stats = want_stats;
    o2.dil = dil;
    Act out;
    if (down && dil == 1) {   // ConvMeanPool conv2 + ConvMeanPool 1x1 shortcut (layers.py:417-420)
      Act s = rt.alloc(x.H / 2, x.W / 2, 2 * x.C);
      ConvOpt os;
      os.circular = false;
      if constexpr (RT::kTraining) {
        // training: the shortcut as conv-then-pool at full resolution
        os.pool = true;
        conv(x, k + ".shortcut.conv", s, os);
      } else {
        // sampling: pool-first -- the 2x2 mean of the raw input, then the 1x1 conv at half resolution (a quarter
        // of the FLOPs; the same linear map, float rounding aside)
        Act xp = rt.alloc(x.H / 2, x.W / 2, x.C);
        rt.launch("avgpool2", "avgpool2 " + std::to_string(x.C) + at(x), 1.25 * rt.B * x.H * x.W * x.C * 4,
                  [&] { return avgpool2(x.p, xp.p, rt.B, x.H, x.W, x.C, rt.st); });
        conv(xp, k + ".shortcut.conv", s, os);
        rt.release(xp);
      }
      out = like(s);
      // sampling, bf16 modes: conv2 and its 2x2 mean as one 4x4 stride-2 conv on the "#pool4x4" weights
      // (conv_kernel.h S2); training and exact fp32: conv-then-pool
      o2.s2 = !RT::kTraining && rt.net->mode != MODE_F32;
      o2.pool = !o2.s2;
      o2.circular = false;
      o2.res = s.p;
      conv(h1, k + ".conv2.conv", out, o2);
      rt.release(s);
    } else if (down) {        // dilated: no resampling, dilated shortcut (layers.py:411-415)
      Act s = like(x);
      ConvOpt os;
      os.dil = dil;
      conv(x, k + ".shortcut", s, os);
      out = like(x);
      o2.res = s.p;
      conv(h1, k + ".conv2", out, o2);
      rt.release(s);
    } else {
      out = like(x);
      o2.res = x.p;
      conv(h1, k + ".conv2", out, o2);
    }
    rt.release(h1);
    return out;
  }

  // RCUBlock (layers.py:126-134): nb blocks of [ELU -> conv -> ELU -> conv] + residual; the last conv applies
  // the following CRP's ELU (final_elu) or writes the head norm's statistics (final_stats)
  Act rcu(const std::string& k, const Act& x0, int nb, bool final_elu, bool final_stats) {
    Act x = x0;
    for (int i = 0; i < nb; ++i) {
      const std::string c = k + "." + std::to_string(i + 1);
      if constexpr (RT::kTraining) rt.keep(k + ".x" + std::to_string(i), x);
      Act t = like(x);
      ConvOpt a;
      a.pro = PRO_ELU;
      a.bias = false;
      conv(x, c + "_1_conv", t, a);
      if constexpr (RT::kTraining) rt.keep(k + ".t" + std::to_string(i), t);
      Act y = like(x);
      ConvOpt b;
      b.pro = PRO_ELU;
      b.bias = false;
      b.res = x.p;
      b.epi_elu = final_elu && i == nb - 1;
      b.stats = final_stats && i == nb - 1;
      conv(t, c + "_2_conv", y, b);
      rt.release(t);
      if (i) rt.release(x);   // the previous block's output; x0 is the caller's
      x = y;
    }
    if constexpr (RT::kTraining) rt.keep(k + ".out", x);
    return x;
  }

  void maxpool(const std::string& ikey, const Act& X, const Act& P) {
    const int B = rt.B;
    // training: the argmax of every window, kept as `ikey` for the backward, and the bf16 tape; sampling: neither
    uint8_t* idx = rt.argmax_out(ikey, (size_t)B * X.H * X.W * X.C);
    rt.launch("maxpool5", "maxpool5 " + std::to_string(X.C) + at(X), 2.0 * B * X.H * X.W * X.C * 4,
              [&] { return maxpool5(X.p, P.p, B, X.H, X.W, X.C, rt.st, idx, rt.h16); });
  }

  // CRPBlock (layers.py:76-83) on X = ELU(h), the ELU already applied by X's producer
  Act crp(const std::string& k, const Act& X) {
    if constexpr (RT::kTraining) rt.keep(k + ".X", X);
    Act p1 = like(X), path1 = like(X), x1 = like(X);
    maxpool(k + ".i1", X, p1);
    ConvOpt a;
    a.bias = false;
    a.out2 = x1.p;
    a.res2 = X.p;
    conv(p1, k + ".convs.0", path1, a);   // path1 ; x1 = path1 + X
    rt.release(p1);
    Act p2 = like(X);
    maxpool(k + ".i2", path1, p2);
    rt.release(path1);
    Act x2 = like(X);
    ConvOpt b;
    b.bias = false;
    b.res = x1.p;
    conv(p2, k + ".convs.1", x2, b);      // x2 = path2 + x1
    if constexpr (RT::kTraining) {
      rt.keep(k + ".p1", p1);
      rt.keep(k + ".path1", path1);
      rt.keep(k + ".p2", p2);
    }
    rt.release(p2);
    rt.release(x1);
    return x2;
  }

  // RefineBlock (layers.py:234-249) of a and, from refine2 on, the previous refine block's output b;
  // MSF (layers.py:179-184) fused with the CRP's input ELU
  Act refine(const std::string& k, const Act& a, const Act* b, int cout, int n_out, bool final_stats) {
    Act X;
    if (!b) {
      X = rcu(k + ".adapt_convs.0", a, 2, true, false);
    } else {
      Act hA = rcu(k + ".adapt_convs.0", a, 2, false, false);
      Act hB = rcu(k + ".adapt_convs.1", *b, 2, false, false);
      Act m;
      ConvOpt o;
      o.epi_elu = true;
      if (hA.H == hB.H) {
        m = rt.alloc(hA.H, hA.W, cout);
        conv(hA, k + ".msf.convs.0", m, ConvOpt{});
        X = like(m);
        o.res = m.p;
        conv(hB, k + ".msf.convs.1", X, o);   // ELU(m0 + m1)
      } else {                                // b at half of a's resolution (refine4)
        m = rt.alloc(hB.H, hB.W, cout);
        conv(hB, k + ".msf.convs.1", m, ConvOpt{});
        X = rt.alloc(hA.H, hA.W, cout);
        o.up = m.p;
        conv(hA, k + ".msf.convs.0", X, o);   // ELU(m0 + up(m1))
      }
      rt.release(m);
      rt.release(hA);
      rt.release(hB);
      if constexpr (RT::kTraining) rt.keep(k + ".msf.X", X);
    }
    Act x2 = crp(k + ".crp", X);
    rt.release(X);
    Act out = rcu(k + ".output_convs", x2, n_out, false, final_stats);
    rt.release(x2);
    return out;
  }

  // scores (or, with lg, the fused Langevin update of lg->x) of x [B,2,H,W] at noise levels `labels`
  void forward(const float* x, const int64_t* labels, float* out, const LangevinArgs* lg) {
    const sdp_net* net = rt.net;
    const int B = rt.B, H = net->d.H, W = net->d.W, C = net->d.ngf;
    const std::string hw = " @" + std::to_string(H) + "x" + std::to_string(W);
    // begin_conv + input prep, statistics over 64-pixel tiles
    Act x0 = rt.alloc(H, W, C);
    rt.launch("begin_conv", "begin_conv 4->128" + hw, (double)B * H * W * (2 * 4 + C * 4) + (double)B * (H * W / 64) * C * 8,
              [&] {
                return begin_conv(x, net->P("begin_conv.weight"), net->P("begin_conv.bias"), x0.p, rt.stats, B, H, W, rt.st,
                                  net->mode, rt.h16);
              });
    Act r = resblock("res1.0", x0, false, 1, true, H * W / 64, 64.f);
    rt.release(x0);
    Act l1 = resblock("res1.1", r, false, 1, true, tiles(r), 128.f);
    rt.release(r);
    // res2 (down: ConvMeanPool).  Its conv2 as conv-then-pool writes statistics per 128-pixel tile of its INPUT
    // (32 pooled pixels each); as one 4x4 stride-2 conv (sampling, bf16 modes) per 128-pixel tile of its output
    r = resblock("res2.0", l1, true, 1, true, tiles(l1), 128.f);
    const bool s2 = !RT::kTraining && net->mode != MODE_F32;
    Act l2 = resblock("res2.1", r, false, 1, true, s2 ? tiles(r) : tiles(l1), s2 ? 128.f : 32.f);
    rt.release(r);
    // res3 (dilation 2), res4 (dilation 4)
    r = resblock("res3.0", l2, true, 2, true, tiles(l2), 128.f);
    Act l3 = resblock("res3.1", r, false, 2, true, tiles(r), 128.f);
    rt.release(r);
    r = resblock("res4.0", l3, true, 4, true, tiles(l3), 128.f);
    // nothing reads the statistics of res4.1's output (refine1 starts with an RCU); training: written all the same
    Act l4 = resblock("res4.1", r, false, 4, RT::kTraining, tiles(r), 128.f);
    rt.release(r);
    Act r1 = refine("refine1", l4, nullptr, 2 * C, 1, false);
    rt.release(l4);
    Act r2 = refine("refine2", l3, &r1, 2 * C, 1, false);
    rt.release(l3);
    rt.release(r1);
    Act r3 = refine("refine3", l2, &r2, C, 1, false);   // 128 channels at half resolution
    rt.release(l2);
    rt.release(r2);
    Act o = refine("refine4", l1, &r3, C, 3, true);     // full resolution, + the head norm's statistics
    rt.release(l1);
    rt.release(r3);
    // head: IN++ -> ELU -> end_conv -> / sigmas[y]
    const float* ss = norm("normalizer", tiles(o), 128.f, C);
    // sampling, with lg: + the fused Langevin update (x read + written, ref, mask, lik: 20 B per element; the
    // scores only when out is given); training: lg is null
    const double lg_bytes = lg ? (double)B * 2 * H * W * (20 + (out ? 4 : 0) + (lg->noise ? 4 : 0)) : B * 2.0 * H * W * 4;
    rt.launch("end_conv", std::string(lg ? "end_conv+langevin" : "end_conv") + " 128->2" + hw,
              (double)B * H * W * C * 4 + lg_bytes, [&] {
                return end_conv(o.p, ss, net->P("end_conv.weight"), net->P("end_conv.bias"), net->P("sigmas"), labels, out, B,
                                H, W, C, rt.st, lg, net->mode, rt.h16);
              });
    rt.release(o);
  }
};

}  // namespace sdp
