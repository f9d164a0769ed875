// DSM training runtime of NCSN_LiDAR_small (BASELINE config 5):
//   sdp_net_forward_train : the score-net forward of ncsnv2.py:484-518 with every tensor the
//                           backward needs kept in the caller's workspace (the "tape")
//   sdp_net_backward      : d loss / d parameters for a given d loss / d score -- loss.backward()
//                           of runners/ncsn_runner_kitti_simultaneous.py:229-232 -- written into a
//                           caller-owned gradient arena laid out like the parameter arena
//   sdp_dsm_loss          : anneal_dsm_score_estimation_with_mask (losses/dsm.py:67-119)
//   sdp_adam_ema_step     : optimizer.step() of torch.optim.Adam + EMAHelper.update (ema.py:16-21)
//
// The forward is the fused plan of net_graph.h (InstanceNorm++ statistics in conv epilogues, its
// affine + ELU in the consumer's prologue, residual / upsample / CRP sums as epilogues), the same
// walker the sampling forward runs, on a runtime that keeps its tensors.  The backward walks the
// graph in reverse with
//   data gradients  : conv_mfma_kernel on dy with flipped/transposed weights (conv_bwd.hip),
//                     fusing elu' and residual gradients into its epilogue,
//   weight gradients: conv_wgrad_kernel (wgrad.hip, MFMA with LDS transpose reads),
//   the rest        : train_aux.hip (IN++ backward, pooling / upsampling adjoints, biases).
// Workspace = forward tape + backward buffers, bump-allocated in a fixed order; a dry run of
// the same code computes its size (sdp_net_train_workspace_size).
#include <cmath>
#include <set>
#include <string>

#include "net_graph.h"

namespace sdp {

// an NHWC activation / gradient tensor of the tape: float32, or bf16 elements when the plan's h16 is set
// (p is then reinterpreted by the kernels: every launch below passes h16 along)
using T4 = Act;

struct TrainPlan {
  sdp_net* net = nullptr;
  int B = 0, H = 0, W = 0, C = 0;
  hipStream_t st = nullptr;
  bool dry = true;
  // the bf16 tape (bf16 mode, sdp_net_set_tape): every activation and output gradient is stored once in
  // bf16 -- half the bytes of every conv's patch DMA and epilogue, of the weight gradient's two operand
  // streams and of the memory-bound adjoints; parameters, the gradient arena, statistics and the head's
  // scores stay float32
  bool h16 = false;
  char* base = nullptr;
  size_t cap = 0, used = 0;
  std::map<std::string, T4> saved;
  std::map<std::string, float*> fl;   // saved per-norm tables: "<key>#ss", "<key>#nst"
  std::map<std::string, uint8_t*> idxs;  // saved maxpool argmax indices
  float* stats = nullptr;
  float* mv = nullptr;                // inpp_finalize scratch
  float* xin = nullptr;               // copy of the forward input [B,2,H,W]
  int64_t* lab = nullptr;             // copy of the labels
  // backward scratch
  float *wpart = nullptr, *bpart = nullptr, *spart = nullptr, *coef = nullptr, *ppart = nullptr, *epart = nullptr;
  size_t wpart_n = 0;
  float* grads = nullptr;
  // gradient completion: the parameters whose gradient each producer finishes, in backward order
  // (grad_order, recorded by every run, dry or not); with bucket events, events[i] is recorded on
  // the stream once the finished parameters cover the arena prefix [0, bucket_end[i])
  std::vector<std::string> grad_order;
  int n_buckets = 0, next_bucket = 0;
  const size_t* bucket_end = nullptr;
  hipEvent_t const* bucket_ev = nullptr;
  size_t done_prefix = 0;             // floats of the arena prefix whose gradients are final
  std::set<std::string> done_keys;    // parameters whose gradients are final
  size_t layout_pos = 0;              // net->layout entries [0, layout_pos) are all in done_keys
  size_t fwd_bytes = 0;
  size_t ws_need = 0;                 // forward + backward bytes (dry run), 0 = unknown

  // ------------------------------------------------------------------ allocation
  float* takeb(size_t nbytes) {
    const size_t bytes = (nbytes + 255) / 256 * 256;
    float* p = dry ? nullptr : reinterpret_cast<float*>(base + used);
    used += bytes;
    if (!dry && used > cap) throw std::runtime_error("training workspace too small");
    return p;
  }
  float* take(size_t nfloats) { return takeb(nfloats * 4); }
  T4 mk(int h, int w, int c) { return T4{takeb((size_t)B * h * w * c * (h16 ? 2 : 4)), h, w, c}; }
  T4 like(const T4& t) { return mk(t.H, t.W, t.C); }
  size_t n(const T4& t) const { return (size_t)B * t.H * t.W * t.C; }
  void ok(hipError_t e, const std::string& what) {
    if (e != hipSuccess) throw std::runtime_error(what + ": " + hipGetErrorString(e));
  }
  const float* P(const std::string& k) const { return net->P(k); }
  float* G(const std::string& k) const { return dry ? nullptr : net->grad_of(grads, k); }
  const T4& S(const std::string& k) const {
    auto it = saved.find(k);
    if (it == saved.end()) throw std::runtime_error("tape: missing " + k);
    return it->second;
  }
  float* F(const std::string& k) const {
    auto it = fl.find(k);
    if (it == fl.end()) throw std::runtime_error("tape: missing " + k);
    return it->second;
  }
  // the gradients of `keys` are final once the launches enqueued so far have run.  The final prefix
  // advances only over layout entries that are ALL finished, in arena order: a parameter finished
  // out of layout order (e.g. a key-ordered fallback layout) never lets a bucket event fire over a
  // gradient that is still being written.  Invariant the bucket reducer relies on
  // (sdp/gradreduce.py): no launch writes a parameter's gradient range after finished() named it.
  void finished(std::initializer_list<std::string> keys) {
    for (const auto& k : keys) {
      grad_order.push_back(k);
      done_keys.insert(k);
    }
    if (dry) return;
    const auto& lay = net->layout;
    while (layout_pos < lay.size() && done_keys.count(lay[layout_pos].key)) {
      done_prefix = std::max(done_prefix, lay[layout_pos].offset + (lay[layout_pos].numel + 63) / 64 * 64);
      ++layout_pos;
    }
    while (next_bucket < n_buckets && done_prefix >= bucket_end[next_bucket])
      ok(hipEventRecord(bucket_ev[next_bucket++], st), "hipEventRecord (gradient bucket)");
  }

  // ------------------------------------------------------------------ forward: the runtime of the graph walker
  // (net_graph.h).  Bump allocation in walker order, nothing reused; what the backward reads is kept
  // under string keys in saved / fl / idxs; a dry run launches nothing
  static constexpr bool kTraining = true;
  Act alloc(int h, int w, int c) { return mk(h, w, c); }
  void release(const Act&) {}
  void keep(const std::string& key, const Act& t) { saved[key] = t; }
  NormOut norm_out(const std::string& nkey, int c) {
    float* ss = take((size_t)B * c * 2);
    float* nst = take((size_t)B * c * 4);
    fl[nkey + "#ss"] = ss;
    fl[nkey + "#nst"] = nst;
    return {ss, nst};
  }
  uint8_t* argmax_out(const std::string& key, size_t n) {
    return idxs[key] = reinterpret_cast<uint8_t*>(take((n + 3) / 4));   // argmax bytes, in floats
  }
  template <class F>
  void launch(const char* what, const std::string&, double, F&& f) {
    if (!dry) ok(f(), what);
  }
  void launch_conv(const ConvArgs& a, int ks, const ConvOpt& o, const std::string& wkey, const Act&, const Act&) {
    const char* why = "conv launch";
    ok(conv_mfma(net->mode, a, ks, o.pool, st, &why), std::string(why) + " (" + wkey + ")");
  }

  void forward(const float* x, const int64_t* labels, float* out) {
    used = 0;
    saved.clear();
    fl.clear();
    idxs.clear();
    xin = take((size_t)B * 2 * H * W);
    lab = reinterpret_cast<int64_t*>(take((size_t)B * 2));
    if (!dry) {
      ok(hipMemcpyAsync(xin, x, (size_t)B * 2 * H * W * 4, hipMemcpyDeviceToDevice, st), "copy x");
      ok(hipMemcpyAsync(lab, labels, (size_t)B * 8, hipMemcpyDeviceToDevice, st), "copy labels");
    }
    stats = take((size_t)B * (H * W / 64) * 2 * C * 2);
    mv = take((size_t)B * 2 * C * 4);
    NetGraph<TrainPlan>{*this}.forward(xin, lab, out, nullptr);
    fwd_bytes = used;
  }

  // ------------------------------------------------------------------ backward pieces
  void wgrad(const std::string& k, const T4& in, int pro, const float* ss, const T4& dy, int dil, bool circular, int ks,
             bool with_bias) {
    if (!dry) wgrad_launch(k, in, pro, ss, dy, dil, circular, ks, with_bias);
    if (with_bias) finished({k + ".weight", k + ".bias"});
    else finished({k + ".weight"});
  }
  void wgrad_launch(const std::string& k, const T4& in, int pro, const float* ss, const T4& dy, int dil, bool circular,
                    int ks, bool with_bias) {
    WgradArgs a{};
    a.in = in.p;
    a.pro_ss = pro == PRO_AFFINE_ELU ? ss : P("#ident_ss");
    a.ss_bstride = pro == PRO_AFFINE_ELU ? 2 * in.C : 0;
    a.pro_mode = pro;
    a.dy = dy.p;
    a.part = wpart;
    a.part_floats = wpart_n;
    a.bpart = bpart;
    a.B = B;
    a.H = in.H;
    a.W = in.W;
    a.Cin = in.C;
    a.Cout = dy.C;
    a.dil = dil;
    a.circular = circular ? 1 : 0;
    const char* why = "wgrad launch";
    ok(conv_wgrad(net->mode, a, ks, G(k + ".weight"), with_bias ? G(k + ".bias") : nullptr, 0, st, &why, h16),
       std::string(why) + " (" + k + ")");
  }
  void dgrad(const std::string& k, const T4& dy, const T4& dx, int dil, bool circular, int ks, int dact,
             const float* aux, const float* epi_ss, const float* res) {
    if (dry) return;
    ConvArgs a{};
    a.in = dy.p;
    a.wf16 = reinterpret_cast<const uint4*>(P(k + ".weight#dfrag16"));   // coalesced 16x16 order (train_aux.hip pack_slot16)
    a.out = dx.p;
    a.res = res;
    a.pro_ss = P("#ident_ss");
    a.B = B;
    a.H = dy.H;
    a.W = dy.W;
    a.Cin = dy.C;
    a.Cout = dx.C;
    a.dil = dil;
    a.circular = circular ? 1 : 0;
    a.pro_mode = PRO_NONE;
    a.aux = aux;
    a.epi_ss = epi_ss;
    a.dact = dact;
    a.io16 = h16 ? 1 : 0;
    const char* why = "dgrad launch";
    ok(conv_dgrad(net->mode, a, ks, st, &why), std::string(why) + " (" + k + ")");
  }
  void inpp_back(const std::string& nkey, const T4& g, const T4& h, const float* r1, const float* r2, const T4& out) {
    if (!dry)
      ok(inpp_backward(g.p, h.p, F(nkey + "#nst"), P(nkey + ".alpha"), P(nkey + ".gamma"), B, h.H * h.W, h.C, spart,
                       coef, ppart, G(nkey + ".alpha"), G(nkey + ".gamma"), G(nkey + ".beta"), r1, r2, out.p, st, h16),
         "inpp_backward " + nkey);
    finished({nkey + ".alpha", nkey + ".gamma", nkey + ".beta"});
  }

  T4 resb(const std::string& k, const T4& dout, bool down, int dil, const float* extra) {
    const T4 &x = S(k + ".x"), &h1 = S(k + ".h1");
    float *ss1 = F(k + ".normalize1#ss"), *ss2 = F(k + ".normalize2#ss");
    T4 g2 = like(h1);
    const float* sg;
    if (down && dil == 1) {
      T4 dyf = mk(x.H, x.W, dout.C);
      if (!dry) ok(unpool(dout.p, dyf.p, B, x.H, x.W, dout.C, st, h16), "unpool");
      wgrad(k + ".conv2.conv", h1, PRO_AFFINE_ELU, ss2, dyf, 1, false, 3, true);
      dgrad(k + ".conv2.conv", dyf, g2, 1, false, 3, 3, h1.p, ss2, nullptr);
      wgrad(k + ".shortcut.conv", x, PRO_NONE, nullptr, dyf, 1, false, 1, true);
      T4 sgb = like(x);
      dgrad(k + ".shortcut.conv", dyf, sgb, 1, false, 1, 0, nullptr, nullptr, nullptr);
      sg = sgb.p;
    } else {
      wgrad(k + ".conv2", h1, PRO_AFFINE_ELU, ss2, dout, dil, true, 3, true);
      dgrad(k + ".conv2", dout, g2, dil, true, 3, 3, h1.p, ss2, nullptr);
      if (down) {
        wgrad(k + ".shortcut", x, PRO_NONE, nullptr, dout, dil, true, 3, true);
        T4 sgb = like(x);
        dgrad(k + ".shortcut", dout, sgb, dil, true, 3, 0, nullptr, nullptr, nullptr);
        sg = sgb.p;
      } else {
        sg = dout.p;
      }
    }
    T4 dh1 = like(h1);
    inpp_back(k + ".normalize2", g2, h1, nullptr, nullptr, dh1);
    wgrad(k + ".conv1", x, PRO_AFFINE_ELU, ss1, dh1, dil, true, 3, true);
    T4 g1 = like(x);
    dgrad(k + ".conv1", dh1, g1, dil, true, 3, 3, x.p, ss1, nullptr);
    T4 dx = like(x);
    inpp_back(k + ".normalize1", g1, x, sg, extra, dx);
    return dx;
  }
  T4 rcub(const std::string& k, const T4& dxn, int nb, bool final_elu) {
    T4 d = dxn;
    if (final_elu) {
      T4 d2 = like(dxn);
      if (!dry) ok(elu_backward_post(dxn.p, S(k + ".out").p, nullptr, d2.p, n(d2), st, h16), "elu_backward");
      d = d2;
    }
    for (int i = nb - 1; i >= 0; --i) {
      const std::string c1 = k + "." + std::to_string(i + 1) + "_1_conv", c2 = k + "." + std::to_string(i + 1) + "_2_conv";
      const T4 &xi = S(k + ".x" + std::to_string(i)), &ti = S(k + ".t" + std::to_string(i));
      wgrad(c2, ti, PRO_ELU, nullptr, d, 1, true, 3, false);
      T4 dt = like(ti);
      dgrad(c2, d, dt, 1, true, 3, 1, ti.p, nullptr, nullptr);
      wgrad(c1, xi, PRO_ELU, nullptr, dt, 1, true, 3, false);
      T4 dn = like(xi);
      dgrad(c1, dt, dn, 1, true, 3, 1, xi.p, nullptr, d.p);
      d = dn;
    }
    return d;
  }
  T4 crpb(const std::string& k, const T4& dx2) {
    const T4 &X = S(k + ".X"), &p1 = S(k + ".p1"), &p2 = S(k + ".p2");
    wgrad(k + ".convs.1", p2, PRO_NONE, nullptr, dx2, 1, true, 3, false);
    T4 dp2 = like(X);
    dgrad(k + ".convs.1", dx2, dp2, 1, true, 3, 0, nullptr, nullptr, nullptr);
    T4 dpath1 = like(X);
    if (!dry)
      ok(maxpool5_backward(idxs.at(k + ".i2"), dp2.p, dx2.p, dpath1.p, B, X.H, X.W, X.C, st, h16), "maxpool5_backward");
    wgrad(k + ".convs.0", p1, PRO_NONE, nullptr, dpath1, 1, true, 3, false);
    T4 dp1 = like(X);
    dgrad(k + ".convs.0", dpath1, dp1, 1, true, 3, 0, nullptr, nullptr, nullptr);
    T4 dX = like(X);
    if (!dry) ok(maxpool5_backward(idxs.at(k + ".i1"), dp1.p, dx2.p, dX.p, B, X.H, X.W, X.C, st, h16), "maxpool5_backward");
    return dX;
  }
  // returns the gradients of the refine block's inputs (second one empty for refine1)
  std::pair<T4, T4> refineb(const std::string& k, const T4& dout, bool two, int n_out) {
    T4 dx2 = rcub(k + ".output_convs", dout, n_out, false);
    T4 dX = crpb(k + ".crp", dx2);
    if (!two) return {rcub(k + ".adapt_convs.0", dX, 2, true), T4{}};
    const T4 &X = S(k + ".msf.X"), &hA = S(k + ".adapt_convs.0.out"), &hB = S(k + ".adapt_convs.1.out");
    T4 dm = like(X);
    if (!dry) ok(elu_backward_post(dX.p, X.p, nullptr, dm.p, n(dm), st, h16), "elu_backward");
    T4 dm1 = dm;
    if (hB.H != hA.H) {
      dm1 = mk(hB.H, hB.W, X.C);
      if (!dry) ok(upsample_backward(dm.p, dm1.p, B, X.H, X.W, X.C, 0, st, h16), "upsample_backward");
    }
    wgrad(k + ".msf.convs.0", hA, PRO_NONE, nullptr, dm, 1, true, 3, true);
    T4 dhA = like(hA);
    dgrad(k + ".msf.convs.0", dm, dhA, 1, true, 3, 0, nullptr, nullptr, nullptr);
    wgrad(k + ".msf.convs.1", hB, PRO_NONE, nullptr, dm1, 1, true, 3, true);
    T4 dhB = like(hB);
    dgrad(k + ".msf.convs.1", dm1, dhB, 1, true, 3, 0, nullptr, nullptr, nullptr);
    return {rcub(k + ".adapt_convs.0", dhA, 2, false), rcub(k + ".adapt_convs.1", dhB, 2, false)};
  }

  void backward(const float* dscore, float* grad_arena) {
    used = fwd_bytes;
    grads = grad_arena;
    grad_order.clear();
    next_bucket = 0;
    done_prefix = 0;
    done_keys.clear();
    layout_pos = 0;
    // scratch (upper bounds over every layer of the network)
    wpart_n = (size_t)(WGRAD_TARGET_BLOCKS + 64) * 9 * 128 * 32;   // >= splits x 9 x Cin x Cout for every conv
    wpart = take(wpart_n);
    spart = take((size_t)B * (H * W / 512) * 256 * 2);   // inpp_backward: 512-pixel groups (train_aux.hip INPP_GRP)
    coef = take((size_t)B * 256 * 4);
    bpart = take(1024 * 256);
    ppart = take((size_t)B * 256 * 3);
    epart = take(head_wgrad_part_floats(B, H, W));
    if (!dry) ok(hipMemsetAsync(grads, 0, net->arena_floats * 4, st), "zero grads");

    // head: IN++ -> ELU -> end_conv -> / sigma
    const T4& o = S("refine4.output_convs.out");
    T4 g = like(o);
    if (!dry)
      ok(end_conv_backward(dscore, P("sigmas"), lab, P("end_conv.weight"), o.p, F("normalizer#ss"), g.p, epart,
                           G("end_conv.weight"), G("end_conv.bias"), B, H, W, st, h16),
         "end_conv_backward");
    finished({"end_conv.weight", "end_conv.bias"});
    T4 d_o = like(o);
    inpp_back("normalizer", g, o, nullptr, nullptr, d_o);
    auto r4 = refineb("refine4", d_o, true, 3);      // -> d L1 (part), d ref3
    auto r3 = refineb("refine3", r4.second, true, 1);  // -> d L2 (part), d ref2
    auto r2 = refineb("refine2", r3.second, true, 1);  // -> d L3 (part), d ref1
    auto r1 = refineb("refine1", r2.second, false, 1); // -> d L4
    T4 d = resb("res4.1", r1.first, false, 4, nullptr);
    d = resb("res4.0", d, true, 4, r2.first.p);        // + d L3 from refine2
    d = resb("res3.1", d, false, 2, nullptr);
    d = resb("res3.0", d, true, 2, r3.first.p);        // + d L2 from refine3
    d = resb("res2.1", d, false, 1, nullptr);
    d = resb("res2.0", d, true, 1, r4.first.p);        // + d L1 from refine4
    d = resb("res1.1", d, false, 1, nullptr);
    d = resb("res1.0", d, false, 1, nullptr);
    if (!dry)
      ok(begin_conv_wgrad(xin, d.p, epart, G("begin_conv.weight"), G("begin_conv.bias"), B, H, W, st, h16),
         "begin_conv_wgrad");
    finished({"begin_conv.weight", "begin_conv.bias"});
    done_prefix = net->arena_floats;   // every gradient is final: the remaining buckets complete here
    finished({});
  }
};

void destroy_plan(TrainPlan* p) { delete p; }

// The parameters in the order the backward finishes their gradients (a dry run of the plan: host
// bookkeeping only).  sdp_net_finalize lays the parameter arena out in this order, so the arena
// prefix whose gradients are final grows monotonically during sdp_net_backward -- the gradient
// buckets of sdp_net_backward_buckets are contiguous ranges that complete one after another.
std::vector<std::string> grad_completion_order(sdp_net* net) {
  TrainPlan p;
  p.net = net;
  p.B = 1;
  p.H = net->d.H;
  p.W = net->d.W;
  p.C = net->d.ngf;
  p.dry = true;
  p.forward(nullptr, nullptr, nullptr);
  p.backward(nullptr, nullptr);
  return p.grad_order;
}

static TrainPlan* plan_for(sdp_net* net, int B) {
  const bool h16 = net->mode == MODE_BF16 && net->tape16;
  if (net->plan && net->plan->B == B && net->plan->h16 == h16) return net->plan;
  if (net->plan) destroy_plan(net->plan);
  TrainPlan* p = new TrainPlan();
  p->net = net;
  p->B = B;
  p->h16 = h16;
  p->H = net->d.H;
  p->W = net->d.W;
  p->C = net->d.ngf;
  net->plan = p;
  return p;
}

static size_t train_ws_bytes(sdp_net* net, int B) {
  TrainPlan* p = plan_for(net, B);
  if (p->ws_need) return p->ws_need;
  p->dry = true;
  p->forward(nullptr, nullptr, nullptr);
  p->backward(nullptr, nullptr);
  p->ws_need = p->used;
  p->saved.clear();
  p->fl.clear();
  return p->ws_need;
}

}  // namespace sdp

using namespace sdp;

static void enable_training(sdp_net* net, hipStream_t st) {
  if (net->mode != MODE_F32X3 && net->mode != MODE_BF16) throw std::runtime_error("training needs fp32x3 or bf16");
  if (!net->train_packs) {
    net->train_packs = true;
    net->repack(st);
  }
}

// sdp_net_backward is sdp_net_backward_buckets with no buckets; `who` prefixes the errors of either
static int backward_entry(const std::string& who, sdp_net* net, const float* dscore, int B, void* ws, size_t ws_bytes,
                          float* grads, int n_buckets, const size_t* bucket_end, void* const* events, void* stream) {
  if (!net || !dscore || !ws || !grads || B <= 0 || n_buckets < 0 || (n_buckets && (!bucket_end || !events)))
    return sdp_fail(who + "bad argument");
  for (int i = 0; i < n_buckets; ++i)
    if (!events[i] || (i && bucket_end[i] <= bucket_end[i - 1]) || bucket_end[i] > net->arena_floats)
      return sdp_fail(who + "bucket ends must increase within the arena, events non-null");
  TrainPlan* p = net->plan;
  if (!p || p->dry || p->B != B || p->base != ws || p->saved.empty())
    return sdp_fail(who + "no tape -- call sdp_net_forward_train with this workspace and batch first");
  try {
    p->st = reinterpret_cast<hipStream_t>(stream);
    p->cap = ws_bytes;
    p->n_buckets = n_buckets;
    p->bucket_end = bucket_end;
    p->bucket_ev = reinterpret_cast<hipEvent_t const*>(events);
    p->backward(dscore, grads);
    p->n_buckets = 0;
  } catch (const std::exception& e) {
    p->n_buckets = 0;
    return sdp_fail(who + e.what());
  }
  return 0;
}

extern "C" {

int sdp_net_set_tape(sdp_net* net, int bf16) {
  if (!net || bf16 < 0 || bf16 > 1) return sdp_fail("sdp_net_set_tape: bad argument");
  net->tape16 = bf16 != 0;
  return 0;
}

int sdp_net_train_workspace_size(sdp_net* net, int B, size_t* bytes) {
  if (!net || !bytes || B <= 0 || !net->finalized) return sdp_fail("sdp_net_train_workspace_size: bad argument");
  try {
    *bytes = train_ws_bytes(net, B);
  } catch (const std::exception& e) {
    return sdp_fail(std::string("sdp_net_train_workspace_size: ") + e.what());
  }
  return 0;
}

int sdp_net_forward_train(sdp_net* net, const float* x, const int64_t* labels, float* out, int B, void* ws,
                          size_t ws_bytes, void* stream) {
  if (!net || !x || !labels || !out || !ws || B <= 0) return sdp_fail("sdp_net_forward_train: bad argument");
  if (!net->finalized) return sdp_fail("sdp_net_forward_train: call sdp_net_finalize first");
  try {
    const size_t need = train_ws_bytes(net, B);
    if (ws_bytes < need) return sdp_fail("sdp_net_forward_train: workspace too small");
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    enable_training(net, st);
    TrainPlan* p = plan_for(net, B);
    p->dry = false;
    p->st = st;
    p->base = reinterpret_cast<char*>(ws);
    p->cap = ws_bytes;
    p->forward(x, labels, out);
  } catch (const std::exception& e) {
    return sdp_fail(std::string("sdp_net_forward_train: ") + e.what());
  }
  return 0;
}

int sdp_net_backward(sdp_net* net, const float* dscore, int B, void* ws, size_t ws_bytes, float* grads, void* stream) {
  return backward_entry("sdp_net_backward: ", net, dscore, B, ws, ws_bytes, grads, 0, nullptr, nullptr, stream);
}

int sdp_net_backward_buckets(sdp_net* net, const float* dscore, int B, void* ws, size_t ws_bytes, float* grads,
                             int n_buckets, const size_t* bucket_end, void* const* events, void* stream) {
  return backward_entry("sdp_net_backward_buckets: ", net, dscore, B, ws, ws_bytes, grads, n_buckets, bucket_end, events,
                        stream);
}

int sdp_dsm_loss(const float* score, const float* noise, const float* mask, const float* used_sigma, int B, int n_img,
                 float anneal_power, float* dscore, float* loss, float* loss_per, float* part, void* stream) {
  if (!score || !noise || !mask || !used_sigma || !dscore || !loss || !part || B <= 0 || n_img <= 0)
    return sdp_fail("sdp_dsm_loss: bad argument");
  hipError_t e = dsm_loss(score, noise, mask, used_sigma, B, n_img, anneal_power, dscore, loss, loss_per, part,
                          reinterpret_cast<hipStream_t>(stream));
  return e == hipSuccess ? 0 : sdp_fail(std::string("sdp_dsm_loss: ") + hipGetErrorString(e));
}

int sdp_adam_ema_step(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, float* ema_shadow, size_t n,
                      double lr, double beta1, double beta2, double eps, int step, double ema_mu, void* stream) {
  if (!params || !grads || !exp_avg || !exp_avg_sq || n == 0 || step < 1) return sdp_fail("sdp_adam_ema_step: bad argument");
  return sdp_optim_ema_step(SDP_OPTIM_ADAM, params, grads, exp_avg, exp_avg_sq, nullptr, ema_shadow, n, lr, beta1, beta2,
                            eps, 0.0, step, ema_mu, stream);
}

int sdp_optim_ema_step(int kind, float* params, const float* grads, float* state0, float* state1, float* state2,
                       float* ema_shadow, size_t n, double lr, double beta1, double beta2, double eps,
                       double weight_decay, int step, double ema_mu, void* stream) {
  if (!params || !grads || !state0 || n == 0 || step < 1 || kind < SDP_OPTIM_ADAM || kind > SDP_OPTIM_SGD ||
      (kind == SDP_OPTIM_ADAM && !state1))
    return sdp_fail("sdp_optim_ema_step: bad argument");
  OptimHyper h{};
  h.b1 = (float)beta1;
  h.b2 = (float)beta2;
  h.eps = (float)eps;
  h.weight_decay = (float)weight_decay;
  h.mu = (float)ema_mu;
  h.omb1 = (float)(1.0 - beta1);
  h.omb2 = (float)(1.0 - beta2);
  h.ommu = (float)(1.0 - ema_mu);
  h.first = step == 1;
  h.step_size = (float)lr;
  h.bc2_sqrt = 1.f;
  if (kind == SDP_OPTIM_ADAM) {   // torch: bias corrections in Python float (double), then lr / bc1, bc2 ** 0.5
    const double bc1 = 1.0 - std::pow(beta1, step), bc2 = 1.0 - std::pow(beta2, step);
    h.step_size = (float)(lr / bc1);
    h.bc2_sqrt = (float)std::sqrt(bc2);
  }
  hipError_t e = optim_ema(kind, params, grads, state0, kind == SDP_OPTIM_ADAM ? state1 : nullptr,
                           kind == SDP_OPTIM_ADAM ? state2 : nullptr, ema_shadow, n, h,
                           reinterpret_cast<hipStream_t>(stream));
  return e == hipSuccess ? 0 : sdp_fail(std::string("sdp_optim_ema_step: ") + hipGetErrorString(e));
}

}  // extern "C"
