// Score-network runtime: parameter store, weight packing and the sampling forward of
// NCSN_LiDAR_small (LiDARGen/models/ncsnv2.py:420-518) over the libsdp kernels.  The plan itself
// is net_graph.h; this file runs it with recycled activation slots and the launch profiler.
//
// Activations live in HBM as NHWC float32 carved from the caller's workspace; every
// InstanceNorm++ is split into per-tile statistics written by the producing conv's
// epilogue + a tiny finalize kernel + an affine/ELU prologue in the consuming conv, so no
// activation is ever re-read just for normalisation.
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <map>
#include <stdexcept>
#include <string>
#include <vector>


#include "net_graph.h"

using namespace sdp;

namespace {

// the activation slots of one sampling forward (the closed form of workspace_bytes_one and the recycler of Fwd):
// full resolution [H, W, C], and half resolution [H/2, W/2, 2C] -- a [H/2, W/2, C] tensor takes a half slot too
constexpr int kFullSlots = 6, kHalfSlots = 8;

size_t round256(size_t floats) { return ((floats * 4 + 255) / 256) * 256; }

// the sampling runtime of the graph walker (net_graph.h): no tape, every launch under the event-pair profiler,
// activations in a fixed pool of slots that the walker's release() hands out again
struct Fwd {
  static constexpr bool kTraining = false, dry = false, h16 = false;
  sdp_net* net;
  int B;
  hipStream_t st;
  float* stats;
  float* ss;     // the one (scale, shift) table: every norm is consumed by the next conv
  float* mv;     // inpp_finalize scratch
  struct Slots {
    char* base;
    size_t stride;   // bytes
    int n;
    unsigned busy;
  } full, half;

  Fwd(sdp_net* net_, int B_, void* ws, size_t ws_bytes, hipStream_t st_) : net(net_), B(B_), st(st_) {
    const int H = net->d.H, W = net->d.W, C2 = 2 * net->d.ngf;
    char* p = reinterpret_cast<char*>(ws);
    char* end = p + ws_bytes;
    auto take = [&](size_t bytes) {
      char* q = p;
      p += bytes;
      if (p > end) throw std::runtime_error("workspace too small");
      return q;
    };
    stats = reinterpret_cast<float*>(take(round256((size_t)B * (H * W / 64) * C2 * 2)));
    ss = reinterpret_cast<float*>(take(round256((size_t)B * C2 * 2)));
    mv = reinterpret_cast<float*>(take(round256((size_t)B * C2 * 4)));
    full = {nullptr, round256((size_t)B * H * W * (C2 / 2)), kFullSlots, 0};
    full.base = take(full.n * full.stride);
    half = {nullptr, round256((size_t)B * (H / 2) * (W / 2) * C2), kHalfSlots, 0};
    half.base = take(half.n * half.stride);
  }

  Slots& slots_of(int H) { return H == net->d.H ? full : half; }
  Act alloc(int H, int W, int C) {
    Slots& s = slots_of(H);
    for (int i = 0; i < s.n; ++i)
      if (!(s.busy >> i & 1)) {
        s.busy |= 1u << i;
        return Act{reinterpret_cast<float*>(s.base + i * s.stride), H, W, C};
      }
    throw std::runtime_error("activation slots exhausted");
  }
  void release(const Act& t) {
    Slots& s = slots_of(t.H);
    s.busy &= ~(1u << ((reinterpret_cast<char*>(t.p) - s.base) / s.stride));
  }
  NormOut norm_out(const std::string&, int) { return {ss, nullptr}; }
  uint8_t* argmax_out(const std::string&, size_t) { return nullptr; }

  // a launch under the profiler: class name + FLOPs + algorithmic bytes (HBM roofline) between two events
  template <class Rec, class F>
  void profiled(Rec&& describe, F&& launch) {
    sdp_net::ProfRec rec;
    if (net->profile) {
      describe(rec);
      rec.a = net->event();
      rec.b = net->event();
      chk(hipEventRecord(rec.a, st), "hipEventRecord");
    }
    launch();
    if (net->profile) {
      chk(hipEventRecord(rec.b, st), "hipEventRecord");
      net->prof.push_back(rec);
    }
  }
  template <class F>
  void launch(const char* what, const std::string& cls, double bytes, F&& f) {
    profiled(
        [&](sdp_net::ProfRec& rec) {
          rec.cls = cls;
          rec.flops = 0;
          rec.bytes = bytes;
        },
        [&] { chk(f(), what); });
  }
  void launch_conv(const ConvArgs& a, int ks, const ConvOpt& o, const std::string& wkey, const Act& in, const Act& out) {
    profiled(
        [&](sdp_net::ProfRec& rec) {
          rec.cls = "conv" + std::to_string(ks) + "x" + std::to_string(ks) + " " + std::to_string(in.C) + "->" +
                    std::to_string(out.C) + " @" + std::to_string(in.H) + "x" + std::to_string(in.W) + " d" +
                    std::to_string(o.dil) + (o.pool ? " pool" : "");
          rec.flops = 2.0 * B * in.H * in.W * (double)in.C * out.C * ks * ks;
          if (o.s2) {   // the FLOPs it executes: 16 taps per output pixel (conv-then-pool, the algorithmic form: 36)
            rec.cls = "conv4x4s2 " + std::to_string(in.C) + "->" + std::to_string(out.C) + " @" + std::to_string(in.H) +
                      "x" + std::to_string(in.W);
            rec.flops = 2.0 * B * out.H * out.W * (double)in.C * out.C * 16;
          }
          rec.bytes = 4.0 * B * ((double)in.H * in.W * in.C + (double)out.H * out.W * out.C) + 4.0 * out.C * in.C * ks * ks;
        },
        [&] {
          const char* why = "conv launch";
          if (conv_mfma(net->mode, a, ks, o.pool, st, &why) != hipSuccess)
            throw std::runtime_error(std::string(why) + " (" + wkey + ")");
        });
  }
};

}  // namespace

// ------------------------------------------------------------------------------ forward
static void forward_impl(sdp_net* net, const float* x, const int64_t* labels, float* out, int B, void* ws,
                         size_t ws_bytes, hipStream_t st, const LangevinArgs* lg = nullptr) {
  Fwd f(net, B, ws, ws_bytes, st);
  NetGraph<Fwd>{f}.forward(x, labels, out, lg);
}

static size_t workspace_bytes_one(const sdp_net* net, int B) {
  const int H = net->d.H, W = net->d.W, C = net->d.ngf, C2 = 2 * C;
  const size_t F = (size_t)B * H * W * C, Q = (size_t)B * (H / 2) * (W / 2) * C2;
  return round256((size_t)B * (H * W / 64) * C2 * 2) + round256((size_t)B * C2 * 2) + round256((size_t)B * C2 * 4) +
         kFullSlots * round256(F) + kHalfSlots * round256(Q);
}

// default of sdp_net::split: two part-batch forwards on two streams (forward_split; the A/B that
// set it: profiles/experiments/r02_split_streams_ab.log)
constexpr int kSplitDefault = 2;
static int split_ways(const sdp_net* net) { return net->split > 0 ? net->split : kSplitDefault; }

// part p of B images split k ways: [first, first + count)
static void split_part(int B, int k, int p, int& first, int& count) {
  first = (int)((long)B * p / k);
  count = (int)((long)B * (p + 1) / k) - first;
}

// room for one B-image forward, or for the part-batch forwards side by side (forward_split)
static size_t workspace_bytes(const sdp_net* net, int B) {
  size_t need = workspace_bytes_one(net, B);
  const int k = std::min(B, split_ways(net));
  if (k > 1) {
    size_t sum = 0;
    for (int p = 0; p < k; ++p) {
      int f, c;
      split_part(B, k, p, f, c);
      sum += workspace_bytes_one(net, c);
    }
    need = std::max(need, sum);
  }
  return need;
}

// The forward as k part-batch forwards on k streams (the caller's and the handle's own), joined by
// events.  Every conv launch of one forward is a lock-step grid: each workgroup owns a CU (LDS),
// so all of them stage their first chunks together and store their outputs together, and those
// bursts leave the matrix cores idle chip-wide; a grid that is not a whole number of rounds also
// idles CUs in its last one.  Concurrent part-size launches de-phase the bursts of one against the
// main loops of another and fill each other's last rounds.  Per-image results are unchanged: no op
// couples images (batch invariance), and the Langevin update of a part uses its own Philox counters
// (offset + first image * per-image counters).
static void forward_split(sdp_net* net, const float* x, const int64_t* labels, float* out, int B, void* ws,
                          size_t ws_bytes, hipStream_t st, const LangevinArgs* lg) {
  const int k = std::min(B, split_ways(net));
  if (k < 2 || net->profile) {
    forward_impl(net, x, labels, out, B, ws, ws_bytes, st, lg);
    return;
  }
  for (int p = 0; p + 1 < k; ++p) {
    if (!net->aux_stream[p])
      chk(hipStreamCreateWithFlags(&net->aux_stream[p], hipStreamNonBlocking), "hipStreamCreate");
    if (!net->ev_join[p]) chk(hipEventCreateWithFlags(&net->ev_join[p], hipEventDisableTiming), "hipEventCreate");
  }
  if (!net->ev_fork) chk(hipEventCreateWithFlags(&net->ev_fork, hipEventDisableTiming), "hipEventCreate");
  const size_t per = (size_t)2 * net->d.H * net->d.W;        // floats of one image (2 channels)
  char* w = reinterpret_cast<char*>(ws);
  chk(hipEventRecord(net->ev_fork, st), "hipEventRecord");
  for (int p = k - 1; p >= 0; --p) {                        // the caller's stream takes part 0, last
    int f, c;
    split_part(B, k, p, f, c);
    const size_t wb = workspace_bytes_one(net, c);
    hipStream_t s = p ? net->aux_stream[p - 1] : st;
    if (p) chk(hipStreamWaitEvent(s, net->ev_fork, 0), "hipStreamWaitEvent");
    LangevinArgs l{};
    if (lg) {
      l = *lg;
      l.x = lg->x + f * per;
      l.ref = lg->ref + f * per;
      l.mask = lg->mask + f * per;
      if (lg->noise) l.noise = lg->noise + f * per;
      if (lg->lik) l.lik = lg->lik + f * per;
      l.offset = lg->offset + f * per / 4;
    }
    forward_impl(net, x + f * per, labels + f, out ? out + f * per : nullptr, c, w, wb, s, lg ? &l : nullptr);
    w += wb;
    if (p) chk(hipEventRecord(net->ev_join[p - 1], s), "hipEventRecord");
  }
  for (int p = 0; p + 1 < k; ++p) chk(hipStreamWaitEvent(st, net->ev_join[p], 0), "hipStreamWaitEvent");
}

// ------------------------------------------------------------------------------ C ABI
static thread_local std::string g_err;

int sdp_fail(const std::string& m) {
  g_err = m;
  return -1;
}

extern "C" {

int sdp_version(void) { return SDP_VERSION; }
const char* sdp_last_error(void) { return g_err.c_str(); }

int sdp_net_create(const sdp_net_desc* desc, sdp_net** out) {
  if (!desc || !out) return sdp_fail("sdp_net_create: null argument");
  if (desc->ngf != 128 || desc->channels != 2) return sdp_fail("sdp_net_create: only ngf=128, channels=2 are built");
  // H % 64: every sub-grid of the plan, down to the dilation-4 one at half resolution, tiles into 8 x 16
  if (desc->H % 64 || desc->W % 128) return sdp_fail("sdp_net_create: H must be a multiple of 64 and W of 128");
  if (desc->precision < 0 || desc->precision > 2) return sdp_fail("sdp_net_create: bad precision");
  sdp_net* n = new sdp_net();
  n->d = *desc;
  n->mode = desc->precision;
  *out = n;
  return 0;
}

int sdp_net_set_param(sdp_net* net, const char* key, const float* data, const int64_t* shape, int ndim) {
  if (!net || !key || !data || (ndim > 0 && !shape)) return sdp_fail("sdp_net_set_param: null argument");
  HostParam hp;
  size_t n = 1;
  for (int i = 0; i < ndim; ++i) {
    hp.shape.push_back(shape[i]);
    n *= (size_t)shape[i];
  }
  hp.data.assign(data, data + n);
  net->host[key] = std::move(hp);
  net->finalized = false;
  return 0;
}

int sdp_net_finalize(sdp_net* net) {
  if (!net) return sdp_fail("sdp_net_finalize: null net");
  try {
    net->release();
    if (!net->host.count("sigmas")) return sdp_fail("sdp_net_finalize: missing sigmas");
    auto upload = [&](const std::string& k, const void* src, size_t bytes) {
      void* d = nullptr;
      chk(hipMalloc(&d, bytes), "hipMalloc");
      chk(hipMemcpy(d, src, bytes, hipMemcpyHostToDevice), "hipMemcpy");
      net->dev[k] = d;
    };
    // every learnable parameter in one arena, 64-float aligned (sdp_net_param_info), in the order
    // the backward finishes their gradients (train.hip grad_completion_order; the parameters it
    // does not name, in key order after them): gradient buckets are then contiguous arena ranges
    net->layout.clear();
    size_t off = 0;
    std::vector<std::string> order;
    try {
      order = grad_completion_order(net);
    } catch (const std::exception&) {   // an incomplete parameter set: key order (its forward fails anyway)
      order.clear();
    }
    std::map<std::string, bool> placed;
    for (auto& kv : net->host)
      if (kv.first != "sigmas") order.push_back(kv.first);   // (duplicates skipped below)
    for (const auto& k : order) {
      auto it = net->host.find(k);
      if (it == net->host.end() || k == "sigmas" || placed[k]) continue;
      placed[k] = true;
      net->layout.push_back({k, off, it->second.data.size()});
      off += (it->second.data.size() + 63) / 64 * 64;
    }
    net->arena_floats = off;
    chk(hipMalloc(&net->arena, off * 4), "hipMalloc");
    net->arena_owned = true;
    for (auto& e : net->layout) {
      chk(hipMemcpy(net->arena + e.offset, net->host[e.key].data.data(), e.numel * 4, hipMemcpyHostToDevice), "hipMemcpy");
      net->dev[e.key] = net->arena + e.offset;
    }
    upload("sigmas", net->host["sigmas"].data.data(), net->host["sigmas"].data.size() * 4);
    for (auto& kv : net->host) {
      const HostParam& hp = kv.second;
      if (net->is_conv_w(kv.first) && (hp.shape[0] % 32 || hp.shape[1] % 32))
        return sdp_fail("sdp_net_finalize: conv channels must be /32: " + kv.first);
    }
    // identity (scale, shift) = (1, 0) rows for convs without an InstanceNorm++ prologue
    std::vector<float> ident(2 * 1024);
    for (size_t i = 0; i < ident.size(); i += 2) ident[i] = 1.f;
    upload("#ident_ss", ident.data(), ident.size() * 4);
    hipStream_t st;
    chk(hipStreamCreateWithFlags(&st, hipStreamNonBlocking), "hipStreamCreate");
    net->repack(st);
    chk(hipStreamSynchronize(st), "hipStreamSynchronize");
    chk(hipStreamDestroy(st), "hipStreamDestroy");
    net->finalized = true;
  } catch (const std::exception& e) {
    return sdp_fail(std::string("sdp_net_finalize: ") + e.what());
  }
  return 0;
}

int sdp_net_param_arena_floats(const sdp_net* net, size_t* n) {
  if (!net || !n || !net->finalized) return sdp_fail("sdp_net_param_arena_floats: finalize first");
  *n = net->arena_floats;
  return 0;
}

int sdp_net_param_count(const sdp_net* net, int* n) {
  if (!net || !n || !net->finalized) return sdp_fail("sdp_net_param_count: finalize first");
  *n = (int)net->layout.size();
  return 0;
}

int sdp_net_param_info(const sdp_net* net, int i, char* key, size_t cap, size_t* offset, size_t* numel) {
  if (!net || !net->finalized || i < 0 || i >= (int)net->layout.size() || !key || cap == 0)
    return sdp_fail("sdp_net_param_info: bad argument");
  const auto& e = net->layout[i];
  std::strncpy(key, e.key.c_str(), cap - 1);
  key[cap - 1] = 0;
  if (offset) *offset = e.offset;
  if (numel) *numel = e.numel;
  return 0;
}

int sdp_net_bind_params(sdp_net* net, float* arena, void* stream) {
  if (!net || !arena || !net->finalized) return sdp_fail("sdp_net_bind_params: bad argument");
  try {
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    if (arena != net->arena)
      chk(hipMemcpyAsync(arena, net->arena, net->arena_floats * 4, hipMemcpyDeviceToDevice, st), "hipMemcpyAsync");
    chk(hipStreamSynchronize(st), "hipStreamSynchronize");
    if (net->arena_owned) chk(hipFree(net->arena), "hipFree");
    net->arena = arena;
    net->arena_owned = false;
    for (auto& e : net->layout) net->dev[e.key] = arena + e.offset;
  } catch (const std::exception& e) {
    return sdp_fail(std::string("sdp_net_bind_params: ") + e.what());
  }
  return 0;
}

int sdp_net_repack(sdp_net* net, void* stream) {
  if (!net || !net->finalized) return sdp_fail("sdp_net_repack: finalize first");
  try {
    net->repack(reinterpret_cast<hipStream_t>(stream));
  } catch (const std::exception& e) {
    return sdp_fail(std::string("sdp_net_repack: ") + e.what());
  }
  return 0;
}

int sdp_net_workspace_size(const sdp_net* net, int B, size_t* bytes) {
  if (!net || !bytes || B <= 0) return sdp_fail("sdp_net_workspace_size: bad argument");
  *bytes = workspace_bytes(net, B);
  return 0;
}

int sdp_net_forward(sdp_net* net, const float* x, const int64_t* labels, float* out, int B, void* ws, size_t ws_bytes,
                    void* stream) {
  if (!net || !x || !labels || !out || !ws || B <= 0) return sdp_fail("sdp_net_forward: bad argument");
  if (!net->finalized) return sdp_fail("sdp_net_forward: call sdp_net_finalize first");
  if (ws_bytes < workspace_bytes(net, B)) return sdp_fail("sdp_net_forward: workspace too small");
  const hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  try {
    forward_split(net, x, labels, out, B, ws, ws_bytes, st, nullptr);
  } catch (const std::exception& e) {
    return sdp_fail(std::string("sdp_net_forward: ") + e.what());
  }
  return 0;
}

int sdp_net_forward_langevin(sdp_net* net, float* x, const int64_t* labels, int B, const sdp_langevin_params* lp,
                             void* ws, size_t ws_bytes, void* stream) {
  if (!net || !x || !labels || !lp || !lp->ref || !lp->mask || !ws || B <= 0)
    return sdp_fail("sdp_net_forward_langevin: bad argument");
  if (!net->finalized) return sdp_fail("sdp_net_forward_langevin: call sdp_net_finalize first");
  if (ws_bytes < workspace_bytes(net, B)) return sdp_fail("sdp_net_forward_langevin: workspace too small");
  const LangevinArgs lg{x,         lp->ref,          lp->mask,  lp->noise,    lp->seed,         lp->offset, lp->step_size,
                        lp->noise_scale, lp->grad_ref, lp->nan_to_num, lp->lik_out, lp->absmax_bits};
  try {
    forward_split(net, x, labels, lp->grad_out, B, ws, ws_bytes, reinterpret_cast<hipStream_t>(stream), &lg);
  } catch (const std::exception& e) {
    return sdp_fail(std::string("sdp_net_forward_langevin: ") + e.what());
  }
  return 0;
}

int sdp_net_set_split(sdp_net* net, int ways) {
  if (!net || ways < 0 || ways > SDP_MAX_SPLIT) return sdp_fail("sdp_net_set_split: ways must be 0 (default) .. 4");
  net->split = ways;
  return 0;
}

int sdp_net_profile_enable(sdp_net* net, int enable) {
  if (!net) return sdp_fail("sdp_net_profile_enable: null net");
  net->profile = enable != 0;
  return 0;
}

// Synchronise on the recorded events and aggregate them per conv class.  Writes up to
// `cap` rows of "class\tlaunches\ttotal_ms\tflops_per_launch\tbytes_per_launch\n" into buf (NUL-terminated)
// and releases the events.  Returns 0; *n_launches receives the number of launches read.
int sdp_net_profile_read(sdp_net* net, char* buf, size_t cap, int* n_launches) {
  if (!net || !buf || cap == 0) return sdp_fail("sdp_net_profile_read: bad argument");
  struct Agg { int n = 0; double ms = 0, flops = 0, bytes = 0; };
  std::map<std::string, Agg> agg;
  try {
    for (auto& r : net->prof) {
      chk(hipEventSynchronize(r.b), "hipEventSynchronize");
      float ms = 0.f;
      chk(hipEventElapsedTime(&ms, r.a, r.b), "hipEventElapsedTime");
      Agg& g = agg[r.cls];
      g.n += 1;
      g.ms += ms;
      g.flops = r.flops;
      g.bytes = r.bytes;
      net->ev_pool.push_back(r.a);
      net->ev_pool.push_back(r.b);
    }
  } catch (const std::exception& e) {
    return sdp_fail(std::string("sdp_net_profile_read: ") + e.what());
  }
  if (n_launches) *n_launches = (int)net->prof.size();
  net->prof.clear();
  std::string out;
  for (auto& kv : agg)
    out += kv.first + "\t" + std::to_string(kv.second.n) + "\t" + std::to_string(kv.second.ms) + "\t" +
           std::to_string(kv.second.flops) + "\t" + std::to_string(kv.second.bytes) + "\n";
  std::strncpy(buf, out.c_str(), cap - 1);
  buf[cap - 1] = 0;
  return 0;
}

int sdp_net_destroy(sdp_net* net) {
  delete net;
  return 0;
}

int sdp_langevin_step(float* x, const float* grad, const float* ref, const int32_t* mask, const float* noise,
                      uint64_t seed, uint64_t offset, float step_size, float noise_scale, float grad_ref, int nan_to_num,
                      int B, int C, int HW, float* lik_out, uint32_t* absmax_bits, void* stream) {
  if (!x || !grad || !ref || !mask || B <= 0 || C <= 0 || HW <= 0) return sdp_fail("sdp_langevin_step: bad argument");
  if (HW % 4) return sdp_fail("sdp_langevin_step: H*W must be a multiple of 4");
  hipError_t e = langevin_step(x, grad, ref, mask, noise, seed, offset, step_size, noise_scale, grad_ref, nan_to_num, B,
                               C, HW, lik_out, absmax_bits, reinterpret_cast<hipStream_t>(stream));
  return e == hipSuccess ? 0 : sdp_fail(std::string("sdp_langevin_step: ") + hipGetErrorString(e));
}

int sdp_axpy_step(float* x, const float* g, float a, const float* lik, const int32_t* mask, const float* ref, float b,
                  int n, void* stream) {
  if (!x || n <= 0 || (g && !lik) || (!g && (!mask || !ref))) return sdp_fail("sdp_axpy_step: bad argument");
  hipError_t e = axpy_step(x, g, a, lik, mask, ref, b, (size_t)n, reinterpret_cast<hipStream_t>(stream));
  return e == hipSuccess ? 0 : sdp_fail(std::string("sdp_axpy_step: ") + hipGetErrorString(e));
}

}  // extern "C"
