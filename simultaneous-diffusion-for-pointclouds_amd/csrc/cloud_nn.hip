// Exact fixed-radius nearest neighbour between two float64 point clouds on the DEVICE, and the metric sums
// on top of it (Chamfer distance, accuracy / completeness, precision / recall / F-score at thresholds).
//   sdp_cloud_nn        for every query the nearest target within max_dist: nn_d2 [nq], nn_idx [nq]
//   sdp_cloud_nn_stats  n_finite, n_matched, sum sqrt(d2), sum d2, max sqrt(d2), #{d2 <= tau_k^2} of one direction
// Every kernel runs on the caller's stream, no workgroup waits for another, there is no floating-point atomic
// and nothing depends on the order in which atomics land (the only ones are the integer LDS digit counts of the
// sort's histogram), so two calls give the same bits.
//   nn_center_kernel    pf = float32(t - center) of every target, a coordinate beyond float32 clamped to
//                       +-FLT_MAX (a target that is finite in float64 must not drop out of the grid)
//   vox_build_cells     voxel_grid.hip's front on pf with cell size float32(cell): bounds, org, nx, ny, nz,
//                       key = ix + nx*iy + nx*ny*iz, the stable sort of (key, target index) (radix_sort.hip), heads
//                       -> sorted unique keys [m], the first sorted row of every cell, the permutation
//   nn_plan_kernel      ONE thread: slack, K, the status and info[8]
//   nn_query_kernel     one query per lane: its own signed cell from the same float32 arithmetic, then the rings
//                       r = 0..K of cells at Chebyshev distance r; per (iy, iz) row one lower-bound search in
//                       the unique keys (the x-neighbours have consecutive keys); the points of a cell through
//                       the permutation; d2 from the ORIGINAL float64 coordinates, ((dx*dx + dy*dy) + dz*dz)
//                       with every operation rounded once; (min d2, then min index) kept
//
// Why the result is exact although a point's cell comes from rounded float32 arithmetic.  Per axis let u be the
// real centred coordinate of a point, x = float32(float64(u)) its float32 image and
//   g(x) = fl32(fl32(x - org) / c),   cell(x) = floor(g(x)),
// the arithmetic of vox_cell, which targets and queries share.  Rounding is monotone, so g is non-decreasing.
// With eps = 2^-24:  g(x) c = (x - org)(1 + d), |d| <= 2 eps + eps^2, and |x - u| <= eps |x| (1 + 2^-28).
// Take a target t and a query q whose cells differ by r >= 1 on this axis, cell(x_t) >= cell(x_q) + r (the
// other sign is symmetric).  Then g(x_t) >= cell(x_t) >= cell(x_q) + r > g(x_q) + r - 1, hence
//   x_t - x_q > (r - 1) c - |d| (|x_t - org| + |x_q - org|)
//   u_t - u_q > (r - 1) c - 2.0001 eps (|x_t - org| + |x_q - org|) - 1.0001 eps (|x_t| + |x_q|).
// Let A bound |x_t|, |x_q| and |org|.  |x_t| <= M, the largest |float32 coordinate| of the targets; |org| <=
// M + c(1 + ...) because org = floor(lo / c) c in float32; and a query is only searched when its float64
// centred coordinate lies within reach = R + slack of the targets' float32 bounds on every axis (otherwise every
// target is farther than R and it is unmatched), so |x_q| <= M + R + slack <= A (1 + 2^-20).  With A = M + R + 2c:
//   u_t - u_q > (r - 1) c - 2.0001 eps 4A - 1.0001 eps 2A = (r - 1) c - 5.0003 * 2^-23 A.
//   slack = 6 * 2^-23 * A,                A = max |float32 target coordinate| + R + 2c
// is therefore a strict bound with a fifth to spare, which also covers the rounding of slack, K and the bounds
// below themselves.  A cell at Chebyshev distance r' differs by r' on some axis, so all its points are farther
// than (r' - 1) c - slack from the query.  Consequences:
//   * rings beyond K = ceil((R + slack) / c) hold only points farther than K c - slack >= R: never a match;
//   * after ring r the unvisited rings (r + 1 ...) hold only points farther than lb = r c - slack, so the search
//     stops once best d2 < lb^2 (1 - 2^-40): an unvisited point can neither beat nor tie the best.
// cell >= R / 8 is required by the entry (K = 8 before the slack); the slack may add ONE ring (cell = R / 8 needs
// K = 9 for any slack > 0).  A slack beyond that -- the float32 grid is too coarse for this cell at these
// coordinates -- gives info[0] = -2 and writes nothing else, like a grid beyond 2^40 cells (info[0] = -1).
// If org lands above the lower bound on an axis (floor(lo * (1/c)) * c can, by one rounding), the lowest cell
// index of voxel_grid.hip wraps and its keys are not ordered; the plan then sets the brute flag and every query
// scans all targets with the same candidate rule: exact but O(nq nt).  It takes a cell that is no power of two
// and a lower bound a rounding away from a multiple of it (about 1e-5 per axis at coordinates of hundreds of
// metres); info[6] reports it, the Python wrappers warn, tests/test_gpu_cloud_nn.py forces it.
#include <cfloat>
#include <cmath>

#include "../../include/sdp.h"
#include "capi.h"
#include "common.h"
#include "voxel_grid.h"

namespace sdp {

constexpr int NN_THREADS = 256;
constexpr int NN_MAX_RINGS = 9;        // 8 from cell >= max_dist / 8, one more for the slack
constexpr int NN_MAX_THRESHOLDS = 8;
constexpr int NN_STAT_COLS = 5 + NN_MAX_THRESHOLDS;
constexpr int64_t NN_MAX_N = 1 << 30;

struct NnPlan {
  double slack, reach;   // metres; reach = R + slack
  int rings, status, brute, pad;
};

struct NnArgs {
  const double* q;
  const double* t;
  const double* center;   // or nullptr
  int nq, nt, qstride, tstride;
  double R, R2;
  double* nn_d2;
  int32_t* nn_idx;
  int64_t* info;
  float* pf;              // [nt][3]
  int64_t* keys;          // [m] sorted unique keys
  int32_t* order;         // [used] sorted permutation
  NnPlan* plan;
  VoxArgs vox;
};

SDP_DEV bool nn_finite3(double x, double y, double z) { return isfinite(x) && isfinite(y) && isfinite(z); }

SDP_DEV double nn_center(const double* c, int k) { return c ? c[k] : 0.0; }

__global__ __launch_bounds__(NN_THREADS) void nn_center_kernel(NnArgs a) {
  const int i = blockIdx.x * NN_THREADS + threadIdx.x;
  if (i >= a.nt) return;
  const double* p = a.t + (size_t)i * a.tstride;
  const double x = p[0], y = p[1], z = p[2];
  const bool fin = nn_finite3(x, y, z);
  const float nan = __builtin_nanf("");
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    double d = __dsub_rn(k == 0 ? x : k == 1 ? y : z, nn_center(a.center, k));
    if (d > (double)FLT_MAX) d = (double)FLT_MAX;
    if (d < -(double)FLT_MAX) d = -(double)FLT_MAX;
    // a non-finite target is no cell's point; a NaN from inf - inf or a NaN centre drops the point too
    a.pf[(size_t)i * 3 + k] = fin ? (float)d : nan;
  }
}

__global__ void nn_plan_kernel(NnArgs a) {
  const VoxHdr* h = a.vox.hdr;
  NnPlan* p = a.plan;
  const double c = (double)a.vox.dl;
  double M = 0.0;
  int brute = 0;
  if (h->used > 0) {
    for (int k = 0; k < 3; ++k) {
      M = fmax(M, fmax(fabs((double)h->lo[k]), fabs((double)h->hi[k])));
      if (!(h->lo[k] >= h->org[k])) brute = 1;
    }
  }
  const double A = M + a.R + 2.0 * c;
  const double slack = 6.0 * 1.1920928955078125e-07 * A;   // 6 * 2^-23 * A
  const double rings = ceil((a.R + slack) / c);
  int status = 0;
  if (h->too_large) status = -1;
  else if (!(rings <= (double)NN_MAX_RINGS)) status = -2;
  p->slack = slack;
  p->reach = a.R + slack;
  p->rings = status == 0 ? (int)rings : 0;
  p->status = status;
  p->brute = brute;
  p->pad = 0;
  a.info[0] = status < 0 ? status : h->m;
  a.info[1] = h->dims[0];
  a.info[2] = h->dims[1];
  a.info[3] = h->dims[2];
  a.info[4] = h->used;
  a.info[5] = rings < 1e18 ? (int64_t)rings : (int64_t)1e18;
  a.info[6] = brute;
  a.info[7] = 0;
}

// nq > 0 and nt == 0: nothing to search
__global__ __launch_bounds__(NN_THREADS) void nn_empty_kernel(NnArgs a) {
  const int i = blockIdx.x * NN_THREADS + threadIdx.x;
  if (i < a.nq) {
    a.nn_d2[i] = __builtin_huge_val();
    a.nn_idx[i] = -1;
  }
  if (i == 0)
    for (int k = 0; k < 8; ++k) a.info[k] = 0;
}

__global__ void nn_info_zero_kernel(NnArgs a) {
  for (int k = 0; k < 8; ++k) a.info[k] = 0;
}

// target j as a candidate for the query (qx, qy, qz): d2 with every operation rounded once, in this order
SDP_DEV void nn_candidate(const NnArgs& a, int j, double qx, double qy, double qz, double& best, int& bj) {
  const double* p = a.t + (size_t)j * a.tstride;
  const double tx = p[0], ty = p[1], tz = p[2];
  if (!nn_finite3(tx, ty, tz)) return;
  const double dx = __dsub_rn(qx, tx), dy = __dsub_rn(qy, ty), dz = __dsub_rn(qz, tz);
  const double d2 = __dadd_rn(__dadd_rn(__dmul_rn(dx, dx), __dmul_rn(dy, dy)), __dmul_rn(dz, dz));
  if (d2 <= a.R2 && (d2 < best || (d2 == best && j < bj))) {
    best = d2;
    bj = j;
  }
}

__global__ __launch_bounds__(NN_THREADS) void nn_query_kernel(NnArgs a) {
  const NnPlan* pl = a.plan;
  if (pl->status < 0) return;
  const int i = blockIdx.x * NN_THREADS + threadIdx.x;
  if (i >= a.nq) return;
  const VoxHdr* h = a.vox.hdr;
  const double* qp = a.q + (size_t)i * a.qstride;
  const double qx = qp[0], qy = qp[1], qz = qp[2];
  double best = __builtin_huge_val();
  int bj = -1;
  const int used = h->used, m = h->m;
  if (nn_finite3(qx, qy, qz) && used > 0) {
    if (pl->brute) {
      for (int j = 0; j < a.nt; ++j) nn_candidate(a, j, qx, qy, qz, best, bj);
    } else {
      const double reach = pl->reach;
      const float c = a.vox.dl;
      long long cq[3];
      bool near = true;
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        const double u = __dsub_rn(k == 0 ? qx : k == 1 ? qy : qz, nn_center(a.center, k));
        // farther than reach from the targets' bounds on one axis (or no number at all): no target within R
        if (!(u >= (double)h->lo[k] - reach && u <= (double)h->hi[k] + reach)) near = false;
        // |u| <= max |target| + reach and fewer than 2^40 cells per axis: the cell fits an int64 with room
        const float f = floorf(__fdiv_rn(__fsub_rn((float)u, h->org[k]), c));
        cq[k] = near ? (long long)f : 0;
      }
      if (near) {
        const long long nx = (long long)h->nx, ny = (long long)h->ny, nz = h->dims[2];
        const int32_t* first = a.vox.first;
        const int rings = pl->rings;
        for (int r = 0; r <= rings; ++r) {
          const long long x0 = cq[0] - r < 0 ? 0 : cq[0] - r, x1 = cq[0] + r > nx - 1 ? nx - 1 : cq[0] + r;
          if (x0 <= x1) {
            for (int dz = -r; dz <= r; ++dz) {
              const long long iz = cq[2] + dz;
              if (iz < 0 || iz >= nz) continue;
              for (int dy = -r; dy <= r; ++dy) {
                const long long iy = cq[1] + dy;
                if (iy < 0 || iy >= ny) continue;
                const bool shell = dz == -r || dz == r || dy == -r || dy == r;   // else only x = cq +- r
                const long long row = nx * iy + nx * ny * iz, khi = row + x1;
                int lo = 0, hi = m;   // lower bound of row + x0 in the unique keys
                while (lo < hi) {
                  const int mid = (int)(((unsigned)lo + (unsigned)hi) >> 1);
                  if (a.keys[mid] < row + x0) lo = mid + 1;
                  else hi = mid;
                }
                for (int v = lo; v < m; ++v) {
                  const long long key = a.keys[v];
                  if (key > khi) break;
                  const long long ddx = key - row - cq[0];
                  if (!shell && ddx != -r && ddx != r) continue;
                  const int b = first[v], e = v + 1 < m ? first[v + 1] : used;
                  for (int s = b; s < e; ++s) nn_candidate(a, a.order[s], qx, qy, qz, best, bj);
                }
              }
            }
          }
          const double lb = (double)r * (double)c - pl->slack;
          if (lb > 0.0 && best < lb * lb * (1.0 - 9.094947017729282e-13)) break;   // 1 - 2^-40
        }
      }
    }
  }
  a.nn_d2[i] = best;
  a.nn_idx[i] = bj;
}

// ---- stats: per-256-point partials in a fixed tree, then one workgroup over the partials in a fixed order ----
struct NnStatArgs {
  const double* d2;
  const double* q;
  int n, qstride, nthr, nblocks;
  double tau2[NN_MAX_THRESHOLDS];
  double* partial;   // [nblocks][NN_STAT_COLS]
  double* out;       // [5 + nthr]
};

// columns 0-3 and 5.. are sums, column 4 a maximum; the tree is the same for every call
SDP_DEV void nn_stat_tree(double (*sh)[NN_THREADS], double* v, int ncol) {
  const int tid = threadIdx.x;
  for (int c = 0; c < ncol; ++c) sh[c][tid] = v[c];
  __syncthreads();
  for (int o = NN_THREADS / 2; o > 0; o >>= 1) {
    if (tid < o) {
      for (int c = 0; c < ncol; ++c)
        sh[c][tid] = c == 4 ? fmax(sh[c][tid], sh[c][tid + o]) : __dadd_rn(sh[c][tid], sh[c][tid + o]);
    }
    __syncthreads();
  }
}

__global__ __launch_bounds__(NN_THREADS) void nn_stat_partial_kernel(NnStatArgs a) {
  __shared__ double sh[NN_STAT_COLS][NN_THREADS];
  const int i = blockIdx.x * NN_THREADS + threadIdx.x, ncol = 5 + a.nthr;
  double v[NN_STAT_COLS];
  for (int c = 0; c < NN_STAT_COLS; ++c) v[c] = 0.0;
  if (i < a.n) {
    const double* p = a.q + (size_t)i * a.qstride;
    const double d2 = a.d2[i];
    v[0] = nn_finite3(p[0], p[1], p[2]) ? 1.0 : 0.0;
    if (d2 < __builtin_huge_val()) {   // matched
      const double d = __dsqrt_rn(d2);
      v[1] = 1.0;
      v[2] = d;
      v[3] = d2;
      v[4] = d;
      for (int k = 0; k < a.nthr; ++k) v[5 + k] = d2 <= a.tau2[k] ? 1.0 : 0.0;
    }
  }
  nn_stat_tree(sh, v, ncol);
  if (threadIdx.x < ncol) a.partial[(size_t)blockIdx.x * NN_STAT_COLS + threadIdx.x] = sh[threadIdx.x][0];
}

__global__ __launch_bounds__(NN_THREADS) void nn_stat_final_kernel(NnStatArgs a) {
  __shared__ double sh[NN_STAT_COLS][NN_THREADS];
  const int ncol = 5 + a.nthr;
  double v[NN_STAT_COLS];
  for (int c = 0; c < NN_STAT_COLS; ++c) v[c] = 0.0;
  for (int b = threadIdx.x; b < a.nblocks; b += NN_THREADS) {
    const double* p = a.partial + (size_t)b * NN_STAT_COLS;
    for (int c = 0; c < ncol; ++c) v[c] = c == 4 ? fmax(v[c], p[c]) : __dadd_rn(v[c], p[c]);
  }
  nn_stat_tree(sh, v, ncol);
  if (threadIdx.x < ncol) a.out[threadIdx.x] = sh[threadIdx.x][0];
}

// measurement hook (sdp_cloud_nn_stage_events): start, after the grid build, after the queries
static thread_local StageEvents<3> nn_events;

// points a.plan .. a.order and vox_ws into the workspace at `w` (0: only count); returns the bytes
static size_t nn_place(NnArgs& a, char*& vox_ws, int64_t nt, uintptr_t w) {
  Layout l{w};
  l.take(a.plan, sizeof(NnPlan));
  if (nt > 0) {
    l.take(a.pf, (size_t)nt * 12);
    l.take(a.keys, (size_t)nt * 8);
    l.take(a.order, (size_t)nt * 4);
    l.take(vox_ws, vox_workspace_bytes(nt));
  }
  return l.bytes;
}

}  // namespace sdp

extern "C" {

int sdp_cloud_nn_workspace_size(int64_t nq, int64_t nt, size_t* bytes) {
  if (!bytes || nq < 0 || nt < 0 || nq > sdp::NN_MAX_N || nt > sdp::NN_MAX_N)
    return sdp_fail("sdp_cloud_nn_workspace_size: nq and nt must be in [0, 2^30]");
  sdp::NnArgs a{};
  char* vox_ws = nullptr;
  *bytes = sdp::nn_place(a, vox_ws, nt, 0);
  return 0;
}

int sdp_cloud_nn_stage_events(void* const* events) { return sdp::nn_events.set(events, "sdp_cloud_nn_stage_events"); }

int sdp_cloud_nn(const double* q, int64_t nq, int qstride, const double* t, int64_t nt, int tstride, double max_dist,
                 double cell, const double* center, double* nn_d2, int32_t* nn_idx, int64_t* info, void* workspace,
                 size_t workspace_bytes, void* stream) {
  using namespace sdp;
  if (nq < 0 || nt < 0 || nq > NN_MAX_N || nt > NN_MAX_N)
    return sdp_fail("sdp_cloud_nn: nq and nt must be in [0, 2^30] (point indices are int32)");
  if (!(max_dist > 0.0) || !std::isfinite(max_dist)) return sdp_fail("sdp_cloud_nn: max_dist must be > 0 and finite");
  if (!(cell > 0.0) || !(cell <= max_dist)) return sdp_fail("sdp_cloud_nn: cell must be in (0, max_dist]");
  if (max_dist / cell > 8.0 || !((float)cell > 0.f))
    return sdp_fail("sdp_cloud_nn: cell too small for max_dist (max_dist / cell must be <= 8)");
  if ((qstride != 3 && qstride != 4) || (tstride != 3 && tstride != 4)) return sdp_fail("sdp_cloud_nn: stride must be 3 or 4");
  if (!info || !workspace || (nq > 0 && (!q || !nn_d2 || !nn_idx)) || (nt > 0 && !t)) return sdp_fail("sdp_cloud_nn: null argument");
  NnArgs a{};
  char* vox_ws = nullptr;
  if (workspace_bytes < nn_place(a, vox_ws, nt, reinterpret_cast<uintptr_t>(workspace)))
    return sdp_fail("sdp_cloud_nn: workspace too small");
  if (reinterpret_cast<uintptr_t>(workspace) % 16) return sdp_fail("sdp_cloud_nn: workspace must be 16-byte aligned");
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  a.q = q;
  a.t = t;
  a.center = center;
  a.nq = (int)nq;
  a.nt = (int)nt;
  a.qstride = qstride;
  a.tstride = tstride;
  a.R = max_dist;
  a.R2 = max_dist * max_dist;
  a.nn_d2 = nn_d2;
  a.nn_idx = nn_idx;
  a.info = info;
  auto mark = [&](int i) { nn_events.mark(i, st); };
  const dim3 one(1), threads(NN_THREADS), qblocks((unsigned)((nq + NN_THREADS - 1) / NN_THREADS));
  mark(0);
  if (nt == 0 || nq == 0) {
    if (nq > 0) hipLaunchKernelGGL(nn_empty_kernel, qblocks, threads, 0, st, a);
    else hipLaunchKernelGGL(nn_info_zero_kernel, one, one, 0, st, a);
    mark(1);
    mark(2);
  } else {
    a.vox.points = a.pf;
    a.vox.n = (int)nt;
    a.vox.stride = 3;
    a.vox.dl = (float)cell;
    a.vox.out_keys = a.keys;
    a.vox.out_order = a.order;
    hipLaunchKernelGGL(nn_center_kernel, dim3((unsigned)((nt + NN_THREADS - 1) / NN_THREADS)), threads, 0, st, a);
    vox_build_cells(a.vox, vox_ws, st);
    hipLaunchKernelGGL(nn_plan_kernel, one, one, 0, st, a);
    mark(1);
    hipLaunchKernelGGL(nn_query_kernel, qblocks, threads, 0, st, a);
    mark(2);
  }
  return launch_status("sdp_cloud_nn");
}

int sdp_cloud_nn_stats_workspace_size(int64_t n, size_t* bytes) {
  if (!bytes || n < 0 || n > sdp::NN_MAX_N) return sdp_fail("sdp_cloud_nn_stats_workspace_size: n must be in [0, 2^30]");
  *bytes = sdp::align256((size_t)((n + sdp::NN_THREADS - 1) / sdp::NN_THREADS) * sdp::NN_STAT_COLS * 8) + 256;
  return 0;
}

int sdp_cloud_nn_stats(const double* nn_d2, const double* q, int qstride, int64_t n, const double* thresholds, int nthr,
                       double max_dist, double* out, void* workspace, size_t workspace_bytes, void* stream) {
  using namespace sdp;
  if (n < 0 || n > NN_MAX_N) return sdp_fail("sdp_cloud_nn_stats: n must be in [0, 2^30]");
  if (nthr < 0 || nthr > NN_MAX_THRESHOLDS || (nthr > 0 && !thresholds)) return sdp_fail("sdp_cloud_nn_stats: 0 to 8 thresholds");
  if (!(max_dist > 0.0)) return sdp_fail("sdp_cloud_nn_stats: max_dist must be > 0");
  if (qstride != 3 && qstride != 4) return sdp_fail("sdp_cloud_nn_stats: stride must be 3 or 4");
  if (!out || !workspace || (n > 0 && (!nn_d2 || !q))) return sdp_fail("sdp_cloud_nn_stats: null argument");
  size_t need = 0;
  sdp_cloud_nn_stats_workspace_size(n, &need);
  if (workspace_bytes < need) return sdp_fail("sdp_cloud_nn_stats: workspace too small");
  if (reinterpret_cast<uintptr_t>(workspace) % 16) return sdp_fail("sdp_cloud_nn_stats: workspace must be 16-byte aligned");
  NnStatArgs a{};
  for (int k = 0; k < nthr; ++k) {
    if (!(thresholds[k] >= 0.0) || thresholds[k] > max_dist)
      return sdp_fail("sdp_cloud_nn_stats: a threshold must lie in [0, max_dist] (nothing beyond max_dist was searched)");
    a.tau2[k] = thresholds[k] * thresholds[k];
  }
  a.d2 = nn_d2;
  a.q = q;
  a.n = (int)n;
  a.qstride = qstride;
  a.nthr = nthr;
  a.nblocks = (int)((n + NN_THREADS - 1) / NN_THREADS);
  a.partial = reinterpret_cast<double*>(workspace);
  a.out = out;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (a.nblocks > 0) hipLaunchKernelGGL(nn_stat_partial_kernel, dim3(a.nblocks), dim3(NN_THREADS), 0, st, a);
  hipLaunchKernelGGL(nn_stat_final_kernel, dim3(1), dim3(NN_THREADS), 0, st, a);
  return launch_status("sdp_cloud_nn_stats");
}

}  // extern "C"
