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
//   5 x { vox_hist_kernel, vox_scan_digits_kernel, vox_scatter_kernel }
//                       stable LSD radix sort, 8-bit digits, tiles of VOXEL_SORT_TILE; a pass at or beyond
//                       the key bits, or one whose digit is the same for every key, moves nothing and
//                       leaves the ping/pong index (VoxHdr::src) where it was
//   vox_head_count_kernel, vox_scan_heads_kernel, vox_head_scatter_kernel
//                       key[i] != key[i-1] -> m, the first sorted row of every voxel, keys, order, inverse
//   vox_reduce_kernel   one thread per (voxel, column): float32 sum in ascending point index, one addend
//                       at a time, then sum * (float)(1.0 / count) (points) or sum / (float)count (features)
//   per label column: vox_label_keys_kernel, 8 x the sort passes on (voxel row << 32) | (label ^ 2^31),
//                       vox_vote_kernel: the longest run of every voxel, the first one among equals
//   vox_info_kernel     info[5]
// The rank of an element inside its tile and digit is a wave ballot (lanes below with the same digit) plus
// an LDS prefix over the (round, wave) slots of the tile in element order -- never the order in which
// atomics land -- so the sort is stable, each voxel's points stay in ascending index, and the sums are
// those of the host's loop over the points.
#include <string>

#include "../../include/sdp.h"
#include "common.h"
#include "voxel_grid.h"

int sdp_fail(const std::string& m);

namespace sdp {

constexpr int VOXEL_CHUNK = 256;            // points per workgroup of the compaction kernels (4 waves)
constexpr int VOXEL_SORT_THREADS = 256;     // threads of a sort workgroup
constexpr int VOXEL_SORT_ROUNDS = 4;        // elements per thread
constexpr int VOXEL_SORT_TILE = 1024;       // elements per sort workgroup
static_assert(VOXEL_SORT_TILE == VOXEL_SORT_THREADS * VOXEL_SORT_ROUNDS, "tile = threads x rounds");
static_assert(VOXEL_SORT_THREADS == 256 && VOXEL_CHUNK == 256, "one thread per digit, four waves");
constexpr int VOXEL_SCAN_THREADS = 1024;    // the one workgroup of every scan kernel
constexpr int VOXEL_SCAN_PER_THREAD = 4;    // consecutive counts per thread: 4096 counts per iteration
constexpr int VOXEL_KEY_PASSES = 5;         // keys below 2^40
constexpr int VOXEL_LABEL_PASSES = 8;       // (voxel row, label) keys of 64 bits
constexpr int VOXEL_SLOTS = VOXEL_SORT_ROUNDS * (VOXEL_SORT_THREADS / 64);
constexpr int VOXEL_MAX_N = 1 << 30;
static_assert(VOXEL_LABEL_PASSES == VOX_HDR_PASSES, "VoxHdr holds the sort state of the longer sort");

SDP_DEV bool vox_finite(float x, float y, float z) { return isfinite(x) && isfinite(y) && isfinite(z); }

// grid_subsampling.cpp:57-61: (size_t)floor((p - org) / dl), in float32 with an IEEE divide
SDP_DEV unsigned long long vox_cell(float p, float org, float dl) {
  return (unsigned long long)(long long)floorf(__fdiv_rn(__fsub_rn(p, org), dl));
}

SDP_DEV int vox_sort_bits(const VoxHdr* h, int mode) {
  if (mode == 0) return h->key_bits;
  return 32 + (h->m <= 1 ? 0 : 32 - __clz(h->m - 1));
}

// exclusive scan of data[0..n) in place by the whole (one) workgroup; returns the total
SDP_DEV int vox_block_scan(int32_t* data, int n) {
  __shared__ int wsum[VOXEL_SCAN_THREADS / 64];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  int carry = 0;
  for (int t0 = 0; t0 < n; t0 += VOXEL_SCAN_THREADS * VOXEL_SCAN_PER_THREAD) {
    const int i0 = t0 + tid * VOXEL_SCAN_PER_THREAD;
    int c[VOXEL_SCAN_PER_THREAD], cnt = 0;
#pragma unroll
    for (int k = 0; k < VOXEL_SCAN_PER_THREAD; ++k) {
      c[k] = i0 + k < n ? data[i0 + k] : 0;
      cnt += c[k];
    }
    int inc = cnt;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const int v = __shfl_up(inc, o, 64);
      if (lane >= o) inc += v;
    }
    if (lane == 63) wsum[wv] = inc;
    __syncthreads();
    int before = 0, total = 0;
    for (int k = 0; k < VOXEL_SCAN_THREADS / 64; ++k) {
      before += k < wv ? wsum[k] : 0;
      total += wsum[k];
    }
    int base = carry + before + (inc - cnt);
#pragma unroll
    for (int k = 0; k < VOXEL_SCAN_PER_THREAD; ++k) {
      if (i0 + k < n) data[i0 + k] = base;
      base += c[k];
    }
    carry += total;
    __syncthreads();   // wsum is rewritten by the next iteration; the stores are visible to the workgroup
  }
  return carry;
}

__global__ __launch_bounds__(VOXEL_CHUNK) void vox_finite_kernel(VoxArgs a) {
  __shared__ int wcnt[VOXEL_CHUNK / 64];
  __shared__ float wmm[VOXEL_CHUNK / 64][6];
  const int c = blockIdx.x, i = c * VOXEL_CHUNK + threadIdx.x, lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  bool fin = false;
  float x = 0.f, y = 0.f, z = 0.f;
  if (i < a.n) {
    const float* p = a.points + (size_t)i * a.stride;
    x = p[0];
    y = p[1];
    z = p[2];
    fin = vox_finite(x, y, z);
  }
  const float inf = __builtin_huge_valf();
  float v[6] = {fin ? x : inf, fin ? y : inf, fin ? z : inf, fin ? x : -inf, fin ? y : -inf, fin ? z : -inf};
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      v[k] = fminf(v[k], __shfl_xor(v[k], o, 64));
      v[k + 3] = fmaxf(v[k + 3], __shfl_xor(v[k + 3], o, 64));
    }
  }
  const unsigned long long m = __ballot(fin);
  if (lane == 0) {
    wcnt[wv] = __popcll(m);
#pragma unroll
    for (int k = 0; k < 6; ++k) wmm[wv][k] = v[k];
  }
  __syncthreads();
  if (threadIdx.x == 0) a.chunk_fin[c] = wcnt[0] + wcnt[1] + wcnt[2] + wcnt[3];
  if (threadIdx.x < 6) {
    const int k = threadIdx.x;
    const float r = k < 3 ? fminf(fminf(wmm[0][k], wmm[1][k]), fminf(wmm[2][k], wmm[3][k]))
                          : fmaxf(fmaxf(wmm[0][k], wmm[1][k]), fmaxf(wmm[2][k], wmm[3][k]));
    a.chunk_mm[(size_t)c * 6 + k] = r;
  }
}

__global__ __launch_bounds__(VOXEL_SCAN_THREADS) void vox_grid_kernel(VoxArgs a) {
  __shared__ float wmm[VOXEL_SCAN_THREADS / 64][6];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int used = vox_block_scan(a.chunk_fin, a.nchunks);
  const float inf = __builtin_huge_valf();
  float v[6] = {inf, inf, inf, -inf, -inf, -inf};
  for (int c = tid; c < a.nchunks; c += VOXEL_SCAN_THREADS) {
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      v[k] = fminf(v[k], a.chunk_mm[(size_t)c * 6 + k]);
      v[k + 3] = fmaxf(v[k + 3], a.chunk_mm[(size_t)c * 6 + k + 3]);
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      v[k] = fminf(v[k], __shfl_xor(v[k], o, 64));
      v[k + 3] = fmaxf(v[k + 3], __shfl_xor(v[k + 3], o, 64));
    }
  }
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < 6; ++k) wmm[wv][k] = v[k];
  }
  __syncthreads();
  if (tid != 0) return;
  VoxHdr* h = a.hdr;
  for (int w = 1; w < VOXEL_SCAN_THREADS / 64; ++w) {
    for (int k = 0; k < 3; ++k) {
      v[k] = fminf(v[k], wmm[w][k]);
      v[k + 3] = fmaxf(v[k + 3], wmm[w][k + 3]);
    }
  }
  h->used = used;
  for (int k = 0; k < 3; ++k) {
    h->lo[k] = v[k];
    h->hi[k] = v[k + 3];
  }
  h->m = 0;
  h->too_large = 0;
  h->key_bits = 0;
  h->nx = h->ny = 0;
  h->pad = 0.f;
  for (int k = 0; k < 3; ++k) {
    h->org[k] = 0.f;
    h->dims[k] = 0;
  }
  for (int md = 0; md < 2; ++md) {
    for (int p = 0; p <= VOXEL_LABEL_PASSES; ++p) h->src[md][p] = 0;
    for (int p = 0; p < VOXEL_LABEL_PASSES; ++p) h->active[md][p] = 0;
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
  const int c = blockIdx.x, i = c * VOXEL_CHUNK + threadIdx.x, lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  bool fin = false;
  float x = 0.f, y = 0.f, z = 0.f;
  if (i < a.n) {
    const float* p = a.points + (size_t)i * a.stride;
    x = p[0];
    y = p[1];
    z = p[2];
    fin = vox_finite(x, y, z);
    if (!fin && a.out_inverse) a.out_inverse[i] = -1;
  }
  const unsigned long long m = __ballot(fin);
  if (lane == 0) wcnt[wv] = __popcll(m);
  __syncthreads();
  if (!fin) return;
  int rank = __popcll(m & ((1ull << lane) - 1ull));
  for (int k = 0; k < wv; ++k) rank += wcnt[k];
  const size_t row = (size_t)a.chunk_fin[c] + rank;
  const float dl = a.dl;
  a.key0[row] = vox_cell(x, h->org[0], dl) + h->nx * vox_cell(y, h->org[1], dl) + h->nx * h->ny * vox_cell(z, h->org[2], dl);
  a.idx0[row] = (uint32_t)i;
}

// ---- one pass of the radix sort: digit `pass` of the keys in buffer src[mode][pass] ----
__global__ __launch_bounds__(VOXEL_SORT_THREADS) void vox_hist_kernel(VoxArgs a, int pass, int mode) {
  __shared__ int hist[256];
  const VoxHdr* h = a.hdr;
  if (h->too_large || pass * 8 >= vox_sort_bits(h, mode)) return;
  const int used = h->used, tid = threadIdx.x, tile = blockIdx.x;
  const uint64_t* k = h->src[mode][pass] ? a.key1 : a.key0;
  hist[tid] = 0;
  __syncthreads();
#pragma unroll
  for (int r = 0; r < VOXEL_SORT_ROUNDS; ++r) {
    const int e = tile * VOXEL_SORT_TILE + r * VOXEL_SORT_THREADS + tid;
    if (e < used) atomicAdd(&hist[(int)((k[e] >> (8 * pass)) & 255)], 1);
  }
  __syncthreads();
  a.tile_cnt[(size_t)tid * a.ntiles + tile] = hist[tid];
}

__global__ __launch_bounds__(VOXEL_SCAN_THREADS) void vox_scan_digits_kernel(VoxArgs a, int pass, int mode) {
  __shared__ int same;
  VoxHdr* h = a.hdr;
  if (h->too_large) return;
  const int tid = threadIdx.x, s = h->src[mode][pass];
  if (pass * 8 >= vox_sort_bits(h, mode)) {
    if (tid == 0) {
      h->active[mode][pass] = 0;
      h->src[mode][pass + 1] = s;
    }
    return;
  }
  if (tid == 0) same = 0;
  const int total = vox_block_scan(a.tile_cnt, 256 * a.ntiles);
  // one digit holds every key: the pass would be the identity, so it is skipped like one beyond the key bits
  if (tid < 256) {
    const int end = tid == 255 ? total : a.tile_cnt[(size_t)(tid + 1) * a.ntiles];
    if (end - a.tile_cnt[(size_t)tid * a.ntiles] == total) same = 1;
  }
  __syncthreads();
  if (tid == 0) {
    const int act = (same || total == 0) ? 0 : 1;
    h->active[mode][pass] = act;
    h->src[mode][pass + 1] = s ^ act;
  }
}

__global__ __launch_bounds__(VOXEL_SORT_THREADS) void vox_scatter_kernel(VoxArgs a, int pass, int mode) {
  __shared__ int wh[VOXEL_SLOTS][256];   // per (round, wave) slot, in element order: count, then first output row
  const VoxHdr* h = a.hdr;
  if (h->too_large || !h->active[mode][pass]) return;
  const int used = h->used, tid = threadIdx.x, tile = blockIdx.x, lane = tid & 63, wv = tid >> 6;
  const int s = h->src[mode][pass];
  const uint64_t* kin = s ? a.key1 : a.key0;
  uint64_t* kout = s ? a.key0 : a.key1;
  const uint32_t* iin = s ? a.idx1 : a.idx0;
  uint32_t* iout = s ? a.idx0 : a.idx1;
  for (int j = tid; j < VOXEL_SLOTS * 256; j += VOXEL_SORT_THREADS) (&wh[0][0])[j] = 0;
  __syncthreads();
  uint64_t kk[VOXEL_SORT_ROUNDS];
  uint32_t vv[VOXEL_SORT_ROUNDS];
  int rk[VOXEL_SORT_ROUNDS], dg[VOXEL_SORT_ROUNDS];
#pragma unroll
  for (int r = 0; r < VOXEL_SORT_ROUNDS; ++r) {
    const int e = tile * VOXEL_SORT_TILE + r * VOXEL_SORT_THREADS + tid;
    const bool valid = e < used;
    kk[r] = valid ? kin[e] : 0;
    vv[r] = (valid && mode == 0) ? iin[e] : 0;
    const int d = (int)((kk[r] >> (8 * pass)) & 255);
    dg[r] = d;
    unsigned long long peers = __ballot(valid);   // the valid lanes of this wave with my digit
#pragma unroll
    for (int b = 0; b < 8; ++b) {
      const bool bit = (d >> b) & 1;
      const unsigned long long bal = __ballot(bit);
      peers &= bit ? bal : ~bal;
    }
    rk[r] = __popcll(peers & ((1ull << lane) - 1ull));
    if (valid && rk[r] == 0) wh[r * (VOXEL_SORT_THREADS / 64) + wv][d] = __popcll(peers);
  }
  __syncthreads();
  {
    int run = a.tile_cnt[(size_t)tid * a.ntiles + tile];   // first output row of (digit tid, this tile)
#pragma unroll
    for (int q = 0; q < VOXEL_SLOTS; ++q) {
      const int t = wh[q][tid];
      wh[q][tid] = run;
      run += t;
    }
  }
  __syncthreads();
#pragma unroll
  for (int r = 0; r < VOXEL_SORT_ROUNDS; ++r) {
    const int e = tile * VOXEL_SORT_TILE + r * VOXEL_SORT_THREADS + tid;
    if (e < used) {
      const int pos = wh[r * (VOXEL_SORT_THREADS / 64) + wv][dg[r]] + rk[r];
      kout[pos] = kk[r];
      if (mode == 0) iout[pos] = vv[r];
    }
  }
}

// ---- segment heads of the sorted keys ----
__global__ __launch_bounds__(VOXEL_CHUNK) void vox_head_count_kernel(VoxArgs a) {
  __shared__ int wcnt[VOXEL_CHUNK / 64];
  const VoxHdr* h = a.hdr;
  if (h->too_large) return;
  const uint64_t* k = h->src[0][VOXEL_KEY_PASSES] ? a.key1 : a.key0;
  const int c = blockIdx.x, i = c * VOXEL_CHUNK + threadIdx.x;
  const bool head = i < h->used && (i == 0 || k[i] != k[i - 1]);
  const unsigned long long m = __ballot(head);
  if ((threadIdx.x & 63) == 0) wcnt[threadIdx.x >> 6] = __popcll(m);
  __syncthreads();
  if (threadIdx.x == 0) a.chunk_head[c] = wcnt[0] + wcnt[1] + wcnt[2] + wcnt[3];
}

__global__ __launch_bounds__(VOXEL_SCAN_THREADS) void vox_scan_heads_kernel(VoxArgs a) {
  VoxHdr* h = a.hdr;
  if (h->too_large) return;
  const int m = vox_block_scan(a.chunk_head, a.nchunks);
  if (threadIdx.x == 0) h->m = m;
}

__global__ __launch_bounds__(VOXEL_CHUNK) void vox_head_scatter_kernel(VoxArgs a) {
  __shared__ int wcnt[VOXEL_CHUNK / 64];
  const VoxHdr* h = a.hdr;
  if (h->too_large) return;
  const int s = h->src[0][VOXEL_KEY_PASSES];
  const uint64_t* k = s ? a.key1 : a.key0;
  const uint32_t* idx = s ? a.idx1 : a.idx0;
  const int c = blockIdx.x, i = c * VOXEL_CHUNK + threadIdx.x, lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const bool in = i < h->used;
  uint64_t key = 0;
  bool head = false;
  if (in) {
    key = k[i];
    head = i == 0 || key != k[i - 1];
  }
  const unsigned long long m = __ballot(head);
  if (lane == 0) wcnt[wv] = __popcll(m);
  __syncthreads();
  if (!in) return;
  int heads = __popcll(m & ((2ull << lane) - 1ull));   // heads up to and including this row
  for (int q = 0; q < wv; ++q) heads += wcnt[q];
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
  const uint32_t* idx = h->src[0][VOXEL_KEY_PASSES] ? a.idx1 : a.idx0;
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
  const uint32_t* idx = h->src[0][VOXEL_KEY_PASSES] ? a.idx1 : a.idx0;
  const int i = blockIdx.x * VOXEL_CHUNK + threadIdx.x;
  if (i >= h->used) return;
  const uint32_t lab = (uint32_t)a.classes[(size_t)idx[i] * a.ldim + col] ^ 0x80000000u;
  a.key0[i] = ((uint64_t)(uint32_t)a.rowof[i] << 32) | lab;   // src[1][0] is 0
}

__global__ __launch_bounds__(256) void vox_vote_kernel(VoxArgs a, int col) {
  const VoxHdr* h = a.hdr;
  if (h->too_large) return;
  const uint64_t* k = h->src[1][VOXEL_LABEL_PASSES] ? a.key1 : a.key0;
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
constexpr int VOXEL_STAGE_EVENTS = 7;
static thread_local void* vox_events[VOXEL_STAGE_EVENTS];
static thread_local bool vox_events_on = false;

static size_t vox_align(size_t b) { return (b + 255) / 256 * 256; }

struct VoxLayout {
  size_t hdr, chunk_fin, chunk_mm, chunk_head, tile_cnt, key0, key1, idx0, idx1, first, rowof, total;
  int nchunks, ntiles;
};

static VoxLayout vox_layout(int64_t n) {
  VoxLayout l{};
  l.nchunks = (int)((n + VOXEL_CHUNK - 1) / VOXEL_CHUNK);
  l.ntiles = (int)((n + VOXEL_SORT_TILE - 1) / VOXEL_SORT_TILE);
  size_t o = 0;
  auto take = [&o](size_t bytes) {
    const size_t at = o;
    o += vox_align(bytes);
    return at;
  };
  l.hdr = take(sizeof(VoxHdr));
  l.chunk_fin = take((size_t)l.nchunks * 4);
  l.chunk_mm = take((size_t)l.nchunks * 24);
  l.chunk_head = take((size_t)l.nchunks * 4);
  l.tile_cnt = take((size_t)l.ntiles * 256 * 4);
  l.key0 = take((size_t)n * 8);
  l.key1 = take((size_t)n * 8);
  l.idx0 = take((size_t)n * 4);
  l.idx1 = take((size_t)n * 4);
  l.first = take((size_t)n * 4);
  l.rowof = take((size_t)n * 4);
  l.total = o;
  return l;
}

static void vox_mark(int i, hipStream_t st) {
  if (vox_events_on) (void)hipEventRecord(reinterpret_cast<hipEvent_t>(vox_events[i]), st);
}

static void vox_sort(const VoxArgs& a, int passes, int mode, hipStream_t st) {
  const dim3 tiles(a.ntiles), one(1);
  for (int p = 0; p < passes; ++p) {
    hipLaunchKernelGGL(vox_hist_kernel, tiles, dim3(VOXEL_SORT_THREADS), 0, st, a, p, mode);
    hipLaunchKernelGGL(vox_scan_digits_kernel, one, dim3(VOXEL_SCAN_THREADS), 0, st, a, p, mode);
    hipLaunchKernelGGL(vox_scatter_kernel, tiles, dim3(VOXEL_SORT_THREADS), 0, st, a, p, mode);
  }
}

size_t vox_workspace_bytes(int64_t n) { return vox_layout(n).total; }

void vox_build_cells(VoxArgs& a, void* workspace, hipStream_t st) {
  const VoxLayout l = vox_layout(a.n);
  char* w = reinterpret_cast<char*>(workspace);
  a.nchunks = l.nchunks;
  a.ntiles = l.ntiles;
  a.hdr = reinterpret_cast<VoxHdr*>(w + l.hdr);
  a.chunk_fin = reinterpret_cast<int32_t*>(w + l.chunk_fin);
  a.chunk_mm = reinterpret_cast<float*>(w + l.chunk_mm);
  a.chunk_head = reinterpret_cast<int32_t*>(w + l.chunk_head);
  a.tile_cnt = reinterpret_cast<int32_t*>(w + l.tile_cnt);
  a.key0 = reinterpret_cast<uint64_t*>(w + l.key0);
  a.key1 = reinterpret_cast<uint64_t*>(w + l.key1);
  a.idx0 = reinterpret_cast<uint32_t*>(w + l.idx0);
  a.idx1 = reinterpret_cast<uint32_t*>(w + l.idx1);
  a.first = reinterpret_cast<int32_t*>(w + l.first);
  a.rowof = reinterpret_cast<int32_t*>(w + l.rowof);
  const dim3 chunks(l.nchunks), one(1);
  vox_mark(0, st);
  hipLaunchKernelGGL(vox_finite_kernel, chunks, dim3(VOXEL_CHUNK), 0, st, a);
  hipLaunchKernelGGL(vox_grid_kernel, one, dim3(VOXEL_SCAN_THREADS), 0, st, a);
  vox_mark(1, st);
  hipLaunchKernelGGL(vox_keys_kernel, chunks, dim3(VOXEL_CHUNK), 0, st, a);
  vox_mark(2, st);
  vox_sort(a, VOXEL_KEY_PASSES, 0, st);
  vox_mark(3, st);
  hipLaunchKernelGGL(vox_head_count_kernel, chunks, dim3(VOXEL_CHUNK), 0, st, a);
  hipLaunchKernelGGL(vox_scan_heads_kernel, one, dim3(VOXEL_SCAN_THREADS), 0, st, a);
  hipLaunchKernelGGL(vox_head_scatter_kernel, chunks, dim3(VOXEL_CHUNK), 0, st, a);
}

}  // namespace sdp

extern "C" {

int sdp_voxel_grid_workspace_size(int64_t n, size_t* bytes) {
  if (!bytes || n < 1 || n > sdp::VOXEL_MAX_N) return sdp_fail("sdp_voxel_grid_workspace_size: n must be in [1, 2^30]");
  *bytes = sdp::vox_layout(n).total;
  return 0;
}

int sdp_voxel_grid_stage_events(void* const* events) {
  sdp::vox_events_on = events != nullptr;
  for (int i = 0; i < sdp::VOXEL_STAGE_EVENTS; ++i) sdp::vox_events[i] = events ? events[i] : nullptr;
  if (events)
    for (int i = 0; i < sdp::VOXEL_STAGE_EVENTS; ++i)
      if (!events[i]) {
        sdp::vox_events_on = false;
        return sdp_fail("sdp_voxel_grid_stage_events: null event");
      }
  return 0;
}

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
  auto sort = [&](int passes, int mode) { vox_sort(a, passes, mode, st); };
  auto mark = [&](int i) { vox_mark(i, st); };
  mark(4);
  const long long work = (long long)n * (3 + a.fdim);
  const int rblocks = (int)((work + 255) / 256 < 262144 ? (work + 255) / 256 : 262144);
  hipLaunchKernelGGL(vox_reduce_kernel, dim3(rblocks), dim3(256), 0, st, a);
  mark(5);
  for (int c = 0; c < a.ldim; ++c) {
    hipLaunchKernelGGL(vox_label_keys_kernel, chunks, dim3(VOXEL_CHUNK), 0, st, a, c);
    sort(VOXEL_LABEL_PASSES, 1);
    hipLaunchKernelGGL(vox_vote_kernel, dim3(a.nchunks < 262144 ? a.nchunks : 262144), dim3(256), 0, st, a, c);
  }
  hipLaunchKernelGGL(vox_info_kernel, one, one, 0, st, a);
  mark(6);
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? 0 : sdp_fail(std::string("sdp_voxel_grid: ") + hipGetErrorString(e));
}

}  // extern "C"
