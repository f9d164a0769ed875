// Range image -> point cloud (the way back out of the samplers): the offline step of
// MeasureResults/SceneCompleter.py:43-70 (azimuth / elevation tables), :105-121 (un-log and
// placement) and :259-264 (exist / min-range / sky mask, concatenation over the views of a scan).
//   x [B][C][H][W] float32 log-depth codes (+ intensity)  ->  float64 [n][4] rows (x, y, z, intensity),
//   views in order, pixels row-major inside a view: numpy's cloud[mask] per view, concatenated.
// Three launches on the caller's stream, no workgroup ever waits for another:
//   unproj_count_kernel   : one workgroup per chunk of UNPROJ_CHUNK pixels of one view; its keep count,
//                           and (spread over the workgroups) the (cos, sin) table of the W azimuths and
//                           H elevations
//   unproj_scan_kernel    : ONE workgroup; exclusive scan of the chunk counts in place and offsets[B+1]
//   unproj_scatter_kernel : the predicate again and its in-chunk rank, one 32-byte row per kept pixel at
//                           base[chunk] + rank
// so the row order is fixed by the pixel order alone and the result is bit-identical from run to run.
// The scan and the chunk count / rank: device_prims.h ("Shared device primitives").
// Distance as oracle/sampling_ref.real_distance with smod = 1: v = f32(|code|*6),
// rd = f32(2^v) - 1 in float32 with 2^v rounded once from its float64 value (numpy's float32 power,
// which SceneCompleter calls, is not correctly rounded); everything after that is float64, no contraction.
#include "../../include/sdp.h"
#include "capi.h"
#include "device_prims.h"

namespace sdp {

constexpr int UNPROJ_CHUNK = 256;           // pixels per workgroup = threads per workgroup (4 waves)
constexpr int UNPROJ_SCAN_THREADS = 1024;   // the scan kernel's one workgroup ...
constexpr int UNPROJ_SCAN_PER_THREAD = 4;   // ... and chunks per thread (the tests size their scan case by the two)
static_assert(UNPROJ_CHUNK == CHUNK_THREADS && UNPROJ_SCAN_THREADS == SCAN_THREADS &&
                  UNPROJ_SCAN_PER_THREAD == SCAN_PER_THREAD, "the primitives of device_prims.h");

struct UnprojArgs {
  const float* x;               // [B][C][H][W]
  const double* origins;        // [B][3] or null
  const double* poses;          // [B][4][4] row-major or null
  const uint8_t* keep_view;     // [B][H][W] or null
  const uint8_t* keep_shared;   // [H][W] or null
  double* points;               // [<= B*H*W][4]
  int32_t* pixel;               // [<= B*H*W] or null
  int64_t* offsets;             // [B+1]
  int32_t* chunk;               // [B * cpv]: keep counts, after the scan the chunks' first rows
  double2* trig;                // [W] (cos, sin) of the azimuths, then [H] of the elevations
  int B, C, H, W, HW, cpv;      // cpv = chunks per view
  float min_range;
  double hA, vA, hMin, vMin;
};

// realDistance of SceneCompleter.py:116 in the merge's float32 convention
SDP_DEV float unproj_distance(float code) {
  const float v = __fmul_rn(fabsf(code), 6.0f);
  return __fsub_rn((float)exp2((double)v), 1.0f);
}

// SceneCompleter.py:259-260: existVals & realDistance > 1.5 & not sky (a NaN code fails the compare)
// (the mask bytes are loaded whatever the compare says, so the three loads of a pixel are in flight together)
SDP_DEV bool unproj_keep(const UnprojArgs& a, int b, int p, float code) {
  const uint8_t kv = a.keep_view ? a.keep_view[(size_t)b * a.HW + p] : 1;
  const uint8_t ks = a.keep_shared ? a.keep_shared[p] : 1;
  return (unproj_distance(code) > a.min_range) & (kv != 0) & (ks != 0);
}

__global__ __launch_bounds__(UNPROJ_CHUNK) void unproj_count_kernel(UnprojArgs a) {
  __shared__ int wcnt[UNPROJ_CHUNK / 64];
  const int c = blockIdx.x, b = c / a.cpv, p = (c - b * a.cpv) * UNPROJ_CHUNK + threadIdx.x;
  // azimuth = arange(W-1,-1,-1)*hA + hMin, elevation = arange(H-1,-1,-1)*vA + vMin (SceneCompleter.py:69-70)
  for (long long i = (long long)c * UNPROJ_CHUNK + threadIdx.x; i < (long long)a.W + a.H;
       i += (long long)gridDim.x * UNPROJ_CHUNK) {
    const double ang = i < a.W ? (double)(a.W - 1 - i) * a.hA + a.hMin : (double)(a.H - 1 - (i - a.W)) * a.vA + a.vMin;
    a.trig[i] = make_double2(cos(ang), sin(ang));
  }
  bool keep = false;
  if (p < a.HW) keep = unproj_keep(a, b, p, a.x[((size_t)b * a.C) * a.HW + p]);
  chunk_post(keep, wcnt);
  __syncthreads();
  if (threadIdx.x == 0) a.chunk[c] = chunk_total(wcnt);
}

__global__ __launch_bounds__(UNPROJ_SCAN_THREADS) void unproj_scan_kernel(UnprojArgs a) {
  // unproj_shape_ok keeps every base and the total below 2^31, so the scan's int carry needs no widening
  const int total = block_exclusive_scan(a.chunk, a.B * a.cpv);   // its last barrier: the bases are visible
  for (int b = threadIdx.x; b < a.B; b += UNPROJ_SCAN_THREADS) a.offsets[b] = a.chunk[(size_t)b * a.cpv];
  if (threadIdx.x == 0) a.offsets[a.B] = total;
}

__global__ __launch_bounds__(UNPROJ_CHUNK) void unproj_scatter_kernel(UnprojArgs a) {
  __shared__ int wcnt[UNPROJ_CHUNK / 64];
  const int c = blockIdx.x, b = c / a.cpv, p = (c - b * a.cpv) * UNPROJ_CHUNK + threadIdx.x;
  const float* xb = a.x + ((size_t)b * a.C) * a.HW;
  float code = 0.f;
  bool keep = false;
  if (p < a.HW) {
    code = xb[p];
    keep = unproj_keep(a, b, p, code);
  }
  const unsigned long long m = chunk_post(keep, wcnt);
  __syncthreads();
  if (!keep) return;
  const float rd = unproj_distance(code);
  const size_t row = (size_t)a.chunk[c] + chunk_rank(m, wcnt);
  const int i = p / a.W, j = p - i * a.W;
  const double2 tz = a.trig[j], te = a.trig[(size_t)a.W + i];
  const double rdd = (double)rd;
  // pointX = realDistance*cos(azimuth)*cos(elevation), ... (SceneCompleter.py:119-121)
  double px = (rdd * tz.x) * te.x, py = (rdd * tz.y) * te.x, pz = rdd * te.y;
  if (a.origins) {
    const double* o = a.origins + (size_t)b * 3;
    px = px + o[0];
    py = py + o[1];
    pz = pz + o[2];
  } else if (a.poses) {   // (pose @ [x y z 1])[:3], products summed left to right (view_transform_kernel)
    const double* T = a.poses + (size_t)b * 16;
    const double qx = ((T[0] * px + T[1] * py) + T[2] * pz) + T[3] * 1.0;
    const double qy = ((T[4] * px + T[5] * py) + T[6] * pz) + T[7] * 1.0;
    const double qz = ((T[8] * px + T[9] * py) + T[10] * pz) + T[11] * 1.0;
    px = qx;
    py = qy;
    pz = qz;
  }
  const double it = a.C == 2 ? (double)xb[(size_t)a.HW + p] : 0.0;
  reinterpret_cast<double4*>(a.points)[row] = make_double4(px, py, pz, it);
  if (a.pixel) a.pixel[row] = b * a.HW + p;
}

static size_t unproj_chunk_bytes(int B, int H, int W) {
  const size_t cpv = ((size_t)H * W + UNPROJ_CHUNK - 1) / UNPROJ_CHUNK;
  return ((size_t)B * cpv * sizeof(int32_t) + 15) / 16 * 16;   // the trig table behind it is 16-byte aligned
}

// pixel ids, in-view pixel offsets and chunk bases are int32: every view padded to whole chunks, B views of
// them, must stay below 2^31 (which also keeps H*W + UNPROJ_CHUNK and the chunk count far inside an int)
static bool unproj_shape_ok(int B, int H, int W) {
  if (B < 1 || H < 1 || W < 1) return false;
  const long long hw = (long long)H * W;
  if (hw > 0x7fffffffll - UNPROJ_CHUNK) return false;
  const long long cpv = (hw + UNPROJ_CHUNK - 1) / UNPROJ_CHUNK;
  return (long long)B * cpv * UNPROJ_CHUNK <= 0x7fffffffll;
}

static size_t unproj_ws_bytes(int B, int H, int W) {
  return unproj_chunk_bytes(B, H, W) + ((size_t)W + H) * sizeof(double2);
}

}  // namespace sdp

extern "C" {

int sdp_range_unproject_workspace_size(int B, int H, int W, size_t* bytes) {
  if (!bytes || !sdp::unproj_shape_ok(B, H, W)) return sdp_fail("sdp_range_unproject_workspace_size: bad argument");
  *bytes = sdp::unproj_ws_bytes(B, H, W);
  return 0;
}

int sdp_range_unproject(const float* x, int B, int C, int H, int W, int geometry, const double* origins,
                        const double* poses, const uint8_t* keep_view, const uint8_t* keep_shared, float min_range,
                        double* points, int32_t* pixel, int64_t* offsets, void* workspace, size_t workspace_bytes,
                        void* stream) {
  if (!sdp::unproj_shape_ok(B, H, W))
    return sdp_fail("sdp_range_unproject: B, H, W must be >= 1 and B * (H*W rounded up to 256) < 2^31");
  if (C != 1 && C != 2) return sdp_fail("sdp_range_unproject: C must be 1 or 2");
  if (origins && poses) return sdp_fail("sdp_range_unproject: origins and poses are exclusive");
  if (geometry != SDP_GEOM_DATASET && geometry != SDP_GEOM_SAMPLER)
    return sdp_fail("sdp_range_unproject: unknown geometry");
  if (!x || !points || !offsets || !workspace) return sdp_fail("sdp_range_unproject: null argument");
  if (workspace_bytes < sdp::unproj_ws_bytes(B, H, W)) return sdp_fail("sdp_range_unproject: workspace too small");
  sdp::UnprojArgs a{};
  a.x = x;
  a.origins = origins;
  a.poses = poses;
  a.keep_view = keep_view;
  a.keep_shared = keep_shared;
  a.points = points;
  a.pixel = pixel;
  a.offsets = offsets;
  a.chunk = reinterpret_cast<int32_t*>(workspace);
  a.trig = reinterpret_cast<double2*>(reinterpret_cast<char*>(workspace) + sdp::unproj_chunk_bytes(B, H, W));
  a.B = B;
  a.C = C;
  a.H = H;
  a.W = W;
  a.HW = H * W;
  a.cpv = (a.HW + sdp::UNPROJ_CHUNK - 1) / sdp::UNPROJ_CHUNK;
  a.min_range = min_range;
  const double deg = 3.14159265358979323846 / 180.0;   // math.radians(x) = x * (pi / 180)
  a.hA = (360.0 * deg) / W;
  a.vA = (28.0 * deg) / H;
  // colCount // (-2) == (W * -180) // 360: the two geometries share the azimuths
  a.hMin = (double)(-(W / 2) - (W % 2)) * a.hA + a.hA / 2;
  if (geometry == SDP_GEOM_DATASET) {
    a.vMin = (3.0 - 28.0) * deg;                       // math.radians(verticalPositive - verticalScope)
  } else {
    const long q = (long)H * -25;                      // (H * -25) // 28, floor division
    a.vMin = (double)(q / 28 - (q % 28 != 0 ? 1 : 0)) * a.vA + a.vA / 2;
  }
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const int n_chunks = B * a.cpv;
  hipLaunchKernelGGL(sdp::unproj_count_kernel, dim3(n_chunks), dim3(sdp::UNPROJ_CHUNK), 0, st, a);
  hipLaunchKernelGGL(sdp::unproj_scan_kernel, dim3(1), dim3(sdp::UNPROJ_SCAN_THREADS), 0, st, a);
  hipLaunchKernelGGL(sdp::unproj_scatter_kernel, dim3(n_chunks), dim3(sdp::UNPROJ_CHUNK), 0, st, a);
  return sdp::launch_status("sdp_range_unproject");
}

}  // extern "C"
