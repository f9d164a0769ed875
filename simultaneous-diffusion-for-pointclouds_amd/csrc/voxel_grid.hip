// Voxel-grid subsampling of a point cloud on the DEVICE: method 0 ("barycenters") of the reference's
// cpp_subsampling/grid_subsampling/grid_subsampling.cpp:46-102, which csrc/grid_subsampling.cpp keeps on
// the host.  Same float32 arithmetic in the same order, so every output bit equals the host's; only the
// row order differs (ascending voxel key here, std::unordered_map order there) and the tie rule of the
// majority labels (smallest label here, hash order there).
//   points [n][stride] (+ features [n][fdim], classes [n][ldim])  ->  [m] barycentres, mean features,
//   majority labels, and optionally keys, counts, the sorted permutation and the point -> voxel map.
// Every kernel runs on the caller's stream, no workgroup ever waits for another, and there is no
// floating-point atomic anywhere (integer LDS atomics count the digits of a tile):
//   vox_finite_kernel   per chunk of VOXEL_CHUNK points: how many are finite, and their min / max
//   vox_grid_kernel     ONE workgroup: exclusive scan of the chunk counts (-> points used), min / max of
//                       the chunks, then org, nx, ny, nz, the key bits and the too-large flag (VoxHdr)
//   vox_keys_kernel     (key, point index) of every finite point, compacted in point order
//   radix_sort, 5 passes  the stable sort of radix_sort.hip on (key, point index)
//   vox_head_count_kernel, vox_scan_heads_kernel, vox_head_scatter_kernel
//                       key[i] != key[i-1] -> m, the first sorted row of every voxel, keys, order, inverse
//   vox_reduce_kernel   one thread per (voxel, column): float32 sum in ascending point index, one addend
//                       at a time, then sum * (float)(1.0 / count) (points) or sum / (float)count (features)
//   per label column: vox_label_keys_kernel, radix_sort with 8 passes and no values on
//                       (voxel row << 32) | (label ^ 2^31), vox_vote_kernel: the longest run of every voxel,
//                       the first one among equals
//   vox_info_kernel     info[5]
// The scan, the chunk count / rank and the min / max butterfly: device_prims.h ("Shared device
// primitives").  The sort is stable: a voxel's points stay in ascending index, the sums are the host loop's.
#include "../../include/sdp.h"
#include "capi.h"
#include "device_prims.h"
#include "voxel_grid.h"

namespace sdp {

constexpr int VOXEL_CHUNK = 256;            // points per workgroup of the compaction kernels (4 waves)
constexpr int VOXEL_SORT_TILE = 1024;       // elements per sort workgroup ...
constexpr int VOXEL_SCAN_THREADS = 1024;    // ... the one workgroup of every scan kernel ...
constexpr int VOXEL_SCAN_PER_THREAD = 4;    // ... and its counts per thread (the tests size their cases by the three)
constexpr int VOXEL_KEY_PASSES = 5;         // keys below 2^40
constexpr int VOXEL_LABEL_PASSES = 8;       // (voxel row, label) keys of 64 bits
static_assert(VOXEL_CHUNK == CHUNK_THREADS && VOXEL_SORT_TILE == RADIX_TILE && VOXEL_SCAN_THREADS == SCAN_THREADS &&
                  VOXEL_SCAN_PER_THREAD == SCAN_PER_THREAD && VOXEL_LABEL_PASSES <= RADIX_MAX_PASSES,
              "the primitives of device_prims.h and radix_sort.h");
constexpr int VOXEL_MAX_N = 1 << 30;

// point i and whether it counts: inside the cloud, all three coordinates finite
SDP_DEV bool vox_point(const VoxArgs& a, int i, float& x, float& y, float& z) {
  if (i >= a.n) return false;
  const float* p = a.points + (size_t)i * a.stride;
  x = p[0];
  y = p[1];
  z = p[2];
  return isfinite(x) && isfinite(y) && isfinite(z);
}

// grid_subsampling.cpp:57-61: (size_t)floor((p - org) / dl), in float32 with an IEEE divide
SDP_DEV unsigned long long vox_cell(float p, float org, float dl) {
  return (unsigned long long)(long long)floorf(__fdiv_rn(__fsub_rn(p, org), dl));
}

__global__ __launch_bounds__(VOXEL_CHUNK) void vox_finite_kernel(VoxArgs a) {
  __shared__ int wcnt[VOXEL_CHUNK / 64];
  __shared__ float wmm[VOXEL_CHUNK / 64][6];
  const int c = blockIdx.x, i = c * VOXEL_CHUNK + threadIdx.x;
  float x = 0.f, y = 0.f, z = 0.f;
  const bool fin = vox_point(a, i, x, y, z);
  const float inf = __builtin_huge_valf();
  float v[6] = {fin ? x : inf, fin ? y : inf, fin ? z : inf, fin ? x : -inf, fin ? y : -inf, fin ? z : -inf};
  wave_minmax3(v, wmm[threadIdx.x >> 6]);
  chunk_post(fin, wcnt);
  __syncthreads();   // the one barrier for the counts and the bounds
  if (threadIdx.x == 0) a.chunk_fin[c] = chunk_total(wcnt);
  if (threadIdx.x < 6) {
    const int k = threadIdx.x;
    const float r = k < 3 ? fminf(fminf(wmm[0][k], wmm[1][k]), fminf(wmm[2][k], wmm[3][k]))
                          : fmaxf(fmaxf(wmm[0][k], wmm[1][k]), fmaxf(wmm[2][k], wmm[3][k]));
    a.chunk_mm[(size_t)c * 6 + k] = r;
  }
}

__global__ __launch_bounds__(SCAN_THREADS) void vox_grid_kernel(VoxArgs a) {
  __shared__ float wmm[SCAN_THREADS / 64][6];
  const int tid = threadIdx.x;
  const int used = block_exclusive_scan(a.chunk_fin, a.nchunks);
  const float inf = __builtin_huge_valf();
  float v[6] = {inf, inf, inf, -inf, -inf, -inf};
  for (int c = tid; c < a.nchunks; c += SCAN_THREADS) {
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      v[k] = fminf(v[k], a.chunk_mm[(size_t)c * 6 + k]);
      v[k + 3] = fmaxf(v[k + 3], a.chunk_mm[(size_t)c * 6 + k + 3]);
    }
  }
  wave_minmax3(v, wmm[tid >> 6]);
  __syncthreads();
  if (tid != 0) return;
  VoxHdr* h = a.hdr;
  for (int w = 1; w < SCAN_THREADS / 64; ++w) {
    for (int k = 0; k < 3; ++k) {
      v[k] = fminf(v[k], wmm[w][k]);
      v[k + 3] = fmaxf(v[k + 3], wmm[w][k + 3]);
    }
  }
  *h = VoxHdr{};   // m, the grid, the key widths, the flag and both sort states start at zero
  h->used = used;
  for (int k = 0; k < 3; ++k) {
    h->lo[k] = v[k];
    h->hi[k] = v[k + 3];
  }
  if (used == 0) return;
  // grid_subsampling.cpp:24-44 in float32: inv = 1/dl, org = floor(lo*inv)*dl, nx = (size_t)floor((hi-org)/dl) + 1
  const float dl = a.dl, inv = __fdiv_rn(1.0f, dl);
  const unsigned long long LIM = 1ull << 40;
  bool big = false;
  unsigned long long d[3];
  for (int k = 0; k < 3; ++k) {
    const float org = __fmul_rn(floorf(__fmul_rn(v[k], inv)), dl);
    h->org[k] = org;
    const float f = floorf(__fdiv_rn(__fsub_rn(v[k + 3], org), dl));
    if (!(f < 1099511627776.0f)) {   // 2^40; a NaN or infinite extent fails the compare too
      big = true;
      d[k] = f < 4611686018427387904.0f ? (unsigned long long)f + 1 : (1ull << 62);
    } else {
      d[k] = (unsigned long long)(long long)f + 1;
    }
    h->dims[k] = (long long)d[k];
  }
  if (!big) {
    const unsigned long long nxy = d[0] * d[1];   // below 2^81 only in theory: each factor is <= 2^40 + 1
    if (d[0] > LIM || d[1] > LIM || d[0] > LIM / (d[1] ? d[1] : 1) || d[2] > LIM / (nxy ? nxy : 1)) big = true;
    if (!big) {
      const unsigned long long cells = nxy * d[2];
      h->nx = d[0];
      h->ny = d[1];
      h->key_bits = cells <= 1 ? 0 : 64 - __clzll((long long)(cells - 1));
    }
  }
  h->too_large = big ? 1 : 0;
}

__global__ __launch_bounds__(VOXEL_CHUNK) void vox_keys_kernel(VoxArgs a) {
  __shared__ int wcnt[VOXEL_CHUNK / 64];
  const VoxHdr* h = a.hdr;
  if (h->too_large) return;
  const int c = blockIdx.x, i = c * VOXEL_CHUNK + threadIdx.x;
  float x = 0.f, y = 0.f, z = 0.f;
  const bool fin = vox_point(a, i, x, y, z);
  if (i < a.n && !fin && a.out_inverse) a.out_inverse[i] = -1;
  const unsigned long long m = chunk_post(fin, wcnt);
  __syncthreads();
  if (!fin) return;
  const size_t row = (size_t)a.chunk_fin[c] + chunk_rank(m, wcnt);
  const float dl = a.dl;
  a.key0[row] = vox_cell(x, h->org[0], dl) + h->nx * vox_cell(y, h->org[1], dl) + h->nx * h->ny * vox_cell(z, h->org[2], dl);
  a.idx0[row] = (uint32_t)i;
}

// ---- segment heads of the sorted keys ----
__global__ __launch_bounds__(VOXEL_CHUNK) void vox_head_count_kernel(VoxArgs a) {
  __shared__ int wcnt[VOXEL_CHUNK / 64];
  const VoxHdr* h = a.hdr;
  if (h->too_large) return;
  const uint64_t* k = radix_result(h->sort[0]) ? a.key1 : a.key0;
  const int c = blockIdx.x, i = c * VOXEL_CHUNK + threadIdx.x;
  const bool head = i < h->used && (i == 0 || k[i] != k[i - 1]);
  chunk_post(head, wcnt);
  __syncthreads();
  if (threadIdx.x == 0) a.chunk_head[c] = chunk_total(wcnt);
}

__global__ __launch_bounds__(SCAN_THREADS) void vox_scan_heads_kernel(VoxArgs a) {
  VoxHdr* h = a.hdr;
  if (h->too_large) return;
  const int m = block_exclusive_scan(a.chunk_head, a.nchunks);
  if (threadIdx.x == 0) {
    h->m = m;
    h->label_bits = 32 + (m <= 1 ? 0 : 32 - __clz(m - 1));   // (voxel row << 32) | label: the rows are below m
  }
}

__global__ __launch_bounds__(VOXEL_CHUNK) void vox_head_scatter_kernel(VoxArgs a) {
  __shared__ int wcnt[VOXEL_CHUNK / 64];
  const VoxHdr* h = a.hdr;
  if (h->too_large) return;
  const int s = radix_result(h->sort[0]);
  const uint64_t* k = s ? a.key1 : a.key0;
  const uint32_t* idx = s ? a.idx1 : a.idx0;
  const int c = blockIdx.x, i = c * VOXEL_CHUNK + threadIdx.x;
  const bool in = i < h->used;
  uint64_t key = 0;
  bool head = false;
  if (in) {
    key = k[i];
    head = i == 0 || key != k[i - 1];
  }
  const unsigned long long m = chunk_post(head, wcnt);
  __syncthreads();
  if (!in) return;
  const int heads = chunk_rank(m, wcnt) + (head ? 1 : 0);   // heads up to and including this row
  const int row = a.chunk_head[c] + heads - 1;
  const int p = (int)idx[i];
  a.rowof[i] = row;
  if (a.out_order) a.out_order[i] = p;
  if (a.out_inverse) a.out_inverse[p] = row;
  if (head) {
    a.first[row] = i;
    if (a.out_keys) a.out_keys[row] = (int64_t)key;
  }
}

// one thread per (voxel, column): columns 0-2 the point, 3.. the features
__global__ __launch_bounds__(256) void vox_reduce_kernel(VoxArgs a) {
  const VoxHdr* h = a.hdr;
  if (h->too_large) return;
  const uint32_t* idx = radix_result(h->sort[0]) ? a.idx1 : a.idx0;
  const int m = h->m, used = h->used, ncol = 3 + a.fdim;
  const long long total = (long long)m * ncol;
  for (long long g = (long long)blockIdx.x * 256 + threadIdx.x; g < total; g += (long long)gridDim.x * 256) {
    const int v = (int)(g / ncol), col = (int)(g - (long long)v * ncol);
    const int b = a.first[v], e = v + 1 < m ? a.first[v + 1] : used, cnt = e - b;
    const float* src = col < 3 ? a.points + col : a.features + (col - 3);
    const size_t st = col < 3 ? (size_t)a.stride : (size_t)a.fdim;
    float sum = 0.f;
    int j = b;
    for (; j + 8 <= e; j += 8) {   // eight gathers in flight, added one at a time in point order
      float t[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) t[u] = src[(size_t)idx[j + u] * st];
#pragma unroll
      for (int u = 0; u < 8; ++u) sum = __fadd_rn(sum, t[u]);
    }
    for (; j < e; ++j) sum = __fadd_rn(sum, src[(size_t)idx[j] * st]);
    // grid_subsampling.cpp:92-101: the point times float(1.0 / count), the features divided by float(count)
    if (col < 3) {
      a.out_points[(size_t)v * 3 + col] = __fmul_rn(sum, (float)(1.0 / (double)cnt));
    } else {
      a.out_features[(size_t)v * a.fdim + (col - 3)] = __fdiv_rn(sum, (float)cnt);
    }
    if (col == 0 && a.out_counts) a.out_counts[v] = cnt;
  }
}

// ---- majority label of column `col`: (voxel row << 32) | (label ^ 2^31) sorted, longest run per voxel ----
__global__ __launch_bounds__(VOXEL_CHUNK) void vox_label_keys_kernel(VoxArgs a, int col) {
  const VoxHdr* h = a.hdr;
  if (h->too_large) return;
  const uint32_t* idx = radix_result(h->sort[0]) ? a.idx1 : a.idx0;
  const int i = blockIdx.x * VOXEL_CHUNK + threadIdx.x;
  if (i >= h->used) return;
  const uint32_t lab = (uint32_t)a.classes[(size_t)idx[i] * a.ldim + col] ^ 0x80000000u;
  a.key0[i] = ((uint64_t)(uint32_t)a.rowof[i] << 32) | lab;   // a sort reads its input from buffer 0
}

__global__ __launch_bounds__(256) void vox_vote_kernel(VoxArgs a, int col) {
  const VoxHdr* h = a.hdr;
  if (h->too_large) return;
  const uint64_t* k = radix_result(h->sort[1]) ? a.key1 : a.key0;
  const int m = h->m, used = h->used;
  for (long long g = (long long)blockIdx.x * 256 + threadIdx.x; g < m; g += (long long)gridDim.x * 256) {
    const int v = (int)g, b = a.first[v], e = v + 1 < m ? a.first[v + 1] : used;
    uint64_t cur = k[b], best = cur;
    int len = 1, best_len = 0;
    for (int j = b + 1; j < e; ++j) {
      const uint64_t x = k[j];
      if (x == cur) {
        ++len;
      } else {
        if (len > best_len) {   // strictly longer: among equals the first, i.e. the smallest label, stays
          best_len = len;
          best = cur;
        }
        cur = x;
        len = 1;
      }
    }
    if (len > best_len) best = cur;
    a.out_classes[(size_t)v * a.ldim + col] = (int32_t)((uint32_t)best ^ 0x80000000u);
  }
}

__global__ void vox_info_kernel(VoxArgs a) {
  const VoxHdr* h = a.hdr;
  a.info[0] = h->too_large ? -1 : h->m;
  a.info[1] = h->dims[0];
  a.info[2] = h->dims[1];
  a.info[3] = h->dims[2];
  a.info[4] = h->used;
}

// measurement hook (sdp_voxel_grid_stage_events): events recorded on the stream between the stages
static thread_local StageEvents<7> vox_events;

// points a.hdr .. a.rowof into the workspace at `w` (0: only count) and sets a.nchunks, a.ntiles; returns the bytes
static size_t vox_place(VoxArgs& a, int64_t n, uintptr_t w) {
  a.nchunks = (int)((n + VOXEL_CHUNK - 1) / VOXEL_CHUNK);
  a.ntiles = (int)((n + VOXEL_SORT_TILE - 1) / VOXEL_SORT_TILE);
  Layout l{w};
  l.take(a.hdr, sizeof(VoxHdr));
  l.take(a.chunk_fin, (size_t)a.nchunks * 4);
  l.take(a.chunk_mm, (size_t)a.nchunks * 24);
  l.take(a.chunk_head, (size_t)a.nchunks * 4);
  l.take(a.tile_cnt, (size_t)a.ntiles * 256 * 4);
  l.take(a.key0, (size_t)n * 8);
  l.take(a.key1, (size_t)n * 8);
  l.take(a.idx0, (size_t)n * 4);
  l.take(a.idx1, (size_t)n * 4);
  l.take(a.first, (size_t)n * 4);
  l.take(a.rowof, (size_t)n * 4);
  return l.bytes;
}

// the sort of the (voxel key, point index) pairs, or of the (voxel row, label) keys alone
static void vox_sort(const VoxArgs& a, bool labels, hipStream_t st) {
  VoxHdr* h = a.hdr;   // a device pointer: only addresses are taken here
  const RadixArgs s{a.key0, a.key1, labels ? nullptr : a.idx0, labels ? nullptr : a.idx1, a.tile_cnt, a.ntiles,
                    &h->used, labels ? &h->label_bits : &h->key_bits, &h->too_large, &h->sort[labels ? 1 : 0]};
  radix_sort(s, labels ? VOXEL_LABEL_PASSES : VOXEL_KEY_PASSES, st);
}

size_t vox_workspace_bytes(int64_t n) {
  VoxArgs a{};
  return vox_place(a, n, 0);
}

void vox_build_cells(VoxArgs& a, void* workspace, hipStream_t st) {
  vox_place(a, a.n, reinterpret_cast<uintptr_t>(workspace));
  const dim3 chunks(a.nchunks), one(1);
  vox_events.mark(0, st);
  hipLaunchKernelGGL(vox_finite_kernel, chunks, dim3(VOXEL_CHUNK), 0, st, a);
  hipLaunchKernelGGL(vox_grid_kernel, one, dim3(SCAN_THREADS), 0, st, a);
  vox_events.mark(1, st);
  hipLaunchKernelGGL(vox_keys_kernel, chunks, dim3(VOXEL_CHUNK), 0, st, a);
  vox_events.mark(2, st);
  vox_sort(a, false, st);
  vox_events.mark(3, st);
  hipLaunchKernelGGL(vox_head_count_kernel, chunks, dim3(VOXEL_CHUNK), 0, st, a);
  hipLaunchKernelGGL(vox_scan_heads_kernel, one, dim3(SCAN_THREADS), 0, st, a);
  hipLaunchKernelGGL(vox_head_scatter_kernel, chunks, dim3(VOXEL_CHUNK), 0, st, a);
}

}  // namespace sdp

extern "C" {

int sdp_voxel_grid_workspace_size(int64_t n, size_t* bytes) {
  if (!bytes || n < 1 || n > sdp::VOXEL_MAX_N) return sdp_fail("sdp_voxel_grid_workspace_size: n must be in [1, 2^30]");
  *bytes = sdp::vox_workspace_bytes(n);
  return 0;
}

int sdp_voxel_grid_stage_events(void* const* events) { return sdp::vox_events.set(events, "sdp_voxel_grid_stage_events"); }

int sdp_voxel_grid(const float* points, int64_t n, int stride, const float* features, int fdim, const int32_t* classes,
                   int ldim, float sample_dl, float* out_points, float* out_features, int32_t* out_classes,
                   int64_t* out_keys, int32_t* out_counts, int32_t* out_order, int32_t* out_inverse, int64_t* info,
                   void* workspace, size_t workspace_bytes, void* stream) {
  using namespace sdp;
  if (n < 1 || n > VOXEL_MAX_N) return sdp_fail("sdp_voxel_grid: n must be in [1, 2^30] (point indices and rows are int32)");
  if (!(sample_dl > 0.f)) return sdp_fail("sdp_voxel_grid: sample_dl must be > 0");
  if (stride != 3 && stride != 4) return sdp_fail("sdp_voxel_grid: stride must be 3 or 4");
  if (!points || !out_points || !info || !workspace) return sdp_fail("sdp_voxel_grid: null argument");
  if (features && (fdim < 1 || fdim > 4096 || !out_features)) return sdp_fail("sdp_voxel_grid: features need 1 <= fdim <= 4096 and out_features");
  if (classes && (ldim < 1 || ldim > 4096 || !out_classes)) return sdp_fail("sdp_voxel_grid: classes need 1 <= ldim <= 4096 and out_classes");
  if (workspace_bytes < vox_workspace_bytes(n)) return sdp_fail("sdp_voxel_grid: workspace too small");
  if (reinterpret_cast<uintptr_t>(workspace) % 16) return sdp_fail("sdp_voxel_grid: workspace must be 16-byte aligned");
  VoxArgs a{};
  a.points = points;
  a.features = features;
  a.classes = classes;
  a.n = (int)n;
  a.stride = stride;
  a.fdim = features ? fdim : 0;
  a.ldim = classes ? ldim : 0;
  a.dl = sample_dl;
  a.out_points = out_points;
  a.out_features = out_features;
  a.out_classes = out_classes;
  a.out_keys = out_keys;
  a.out_counts = out_counts;
  a.out_order = out_order;
  a.out_inverse = out_inverse;
  a.info = info;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  vox_build_cells(a, workspace, st);
  const dim3 chunks(a.nchunks), one(1);
  vox_events.mark(4, st);
  const long long work = (long long)n * (3 + a.fdim);
  const int rblocks = (int)((work + 255) / 256 < 262144 ? (work + 255) / 256 : 262144);
  hipLaunchKernelGGL(vox_reduce_kernel, dim3(rblocks), dim3(256), 0, st, a);
  vox_events.mark(5, st);
  for (int c = 0; c < a.ldim; ++c) {
    hipLaunchKernelGGL(vox_label_keys_kernel, chunks, dim3(VOXEL_CHUNK), 0, st, a, c);
    vox_sort(a, true, st);
    hipLaunchKernelGGL(vox_vote_kernel, dim3(a.nchunks < 262144 ? a.nchunks : 262144), dim3(256), 0, st, a, c);
  }
  hipLaunchKernelGGL(vox_info_kernel, one, one, 0, st, a);
  vox_events.mark(6, st);
  return launch_status("sdp_voxel_grid");
}

}  // extern "C"
