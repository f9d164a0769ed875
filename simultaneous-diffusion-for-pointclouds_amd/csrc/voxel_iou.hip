// Voxel occupancy and semantic IoU between two float64 point clouds on the DEVICE: both clouds on ONE fixed
// grid (origin, voxel, dims from the caller), the majority label of every occupied voxel, and the confusion
// matrix of the voxels' states (contract: include/sdp.h, sdp_voxel_iou; DESIGN.md section 4, "Voxel IoU").
// Per cloud (cloud A = the truth, cloud B = the prediction):
//   viou_count_kernel       per chunk of CHUNK_THREADS points: how many are used, how many carry a bad label
//   viou_hdr_kernel         ONE workgroup per cloud: exclusive scan of the used counts (-> points used, the
//                           chunks' first rows), the bad-label total, the zeroed sort state
//   viou_keys_kernel        cell * 64 + label of every used point, compacted in point order
//   radix_sort              ceil(key bits / 8) passes of radix_sort.hip, keys only; the count stays on the device
//   viou_head_count_kernel, viou_scan_heads_kernel, viou_head_scatter_kernel
//                           (key >> 6)[i] != (key >> 6)[i-1] -> m, the unique cells [m], their first sorted rows
//   viou_vote_kernel        one thread per voxel: the longest label run of its segment, the first among equals
//                           (the keys are sorted, so that is the smallest label), the point count
// Comparison:
//   viou_valid_kernel       with a valid mask: VIOU_BLOCKS partial counts of its non-zero bytes
//   viou_compare_kernel     every cell of A searches B's unique cells (lower bound): (1 + la, 1 + lb) or
//                           (1 + la, 0); every cell of B searches A's: (0, 1 + lb) when absent.  Each workgroup
//                           counts its pairs in an LDS integer histogram and writes it as its partial
//   viou_final_kernel       ONE workgroup: the partials added in block order, |A n B|, [0][0] and info[8]
// Every kernel runs on the caller's stream and no workgroup waits for another.  The only atomics are integer
// LDS adds (the sort's digit counts, the pair histogram, the intersection count), whose sums do not depend on
// the order they land in: every output is an exact integer, the same bits on every call.
// A point's cell is floor((p - origin) / voxel) per axis in float64: one subtraction, one IEEE division, one
// floor -- no reciprocal, no FMA (the file is built with -ffp-contract=off).  The bounds test runs on the floored
// double, so a NaN, an infinite or a huge quotient never reaches an integer conversion.
#include <cmath>

#include "../../include/sdp.h"
#include "capi.h"
#include "device_prims.h"
#include "radix_sort.h"

namespace sdp {

constexpr int VIOU_CHUNK = 256;             // points (or sorted rows) per workgroup of the compaction kernels
constexpr int VIOU_SORT_TILE = 1024;        // elements per sort workgroup ...
constexpr int VIOU_SCAN_THREADS = 1024;     // ... the one workgroup of every scan kernel ...
constexpr int VIOU_SCAN_PER_THREAD = 4;     // ... and its counts per thread (the tests size their cases by these)
constexpr int VIOU_LABEL_BITS = 6;          // composite key = cell * 64 + label
constexpr int VIOU_MAX_CLASSES = 64;
constexpr int VIOU_BLOCKS = 256;            // workgroups (and partials) of the comparison and of the mask count
constexpr int VIOU_THREADS = 256;
constexpr int VIOU_MAX_STATES = VIOU_MAX_CLASSES + 1;
constexpr int64_t VIOU_MAX_N = 1 << 30;
constexpr int64_t VIOU_MAX_CELLS = 1ll << 40;
constexpr int64_t VIOU_MAX_MASK_CELLS = 1ll << 31;
static_assert(VIOU_CHUNK == CHUNK_THREADS && VIOU_SORT_TILE == RADIX_TILE && VIOU_SCAN_THREADS == SCAN_THREADS &&
                  VIOU_SCAN_PER_THREAD == SCAN_PER_THREAD && (1 << VIOU_LABEL_BITS) == VIOU_MAX_CLASSES,
              "the primitives of device_prims.h and radix_sort.h");
static_assert(VIOU_MAX_STATES * VIOU_MAX_STATES * 4 <= 17 * 1024, "the pair histogram stays under 17 KB of LDS");

struct ViouHdr {
  int used, m, bad, key_bits, skip, pad;
  RadixState sort;
};

struct ViouCloud {
  const double* p;
  const int32_t* labels;    // or nullptr: every label 0
  int n, stride, nchunks, ntiles;
  ViouHdr* hdr;
  int32_t* chunk_cnt;       // [nchunks] used points per chunk, after the scan the chunks' first rows
  int32_t* chunk_bad;       // [nchunks] points with a label outside [0, C), after the scan their prefix
  int32_t* chunk_head;      // [nchunks] segment heads per chunk of sorted rows, then their first voxel rows
  int32_t* tile_cnt;        // [256][ntiles]
  uint64_t* key0;
  uint64_t* key1;
  int32_t* first;           // [m] first sorted row of each voxel
  int64_t* cells;           // [m] sorted unique cell keys
  int32_t* state;           // [m] majority label
  int64_t* out_cells;       // the caller's optional outputs
  int32_t* out_labels;
  int32_t* out_counts;
};

struct ViouArgs {
  ViouCloud c[2];
  double org[3];
  double voxel;
  long long nx, ny, nz, ncells;
  int C, key_bits;
  const uint8_t* valid;     // or nullptr
  int64_t* confusion;
  int64_t* info;
  uint32_t* partial;        // [VIOU_BLOCKS][(C+1)*(C+1)]
  int64_t* valid_partial;   // [VIOU_BLOCKS]
};

// one axis: i = floor((p - org) / voxel), tested against [0, n) as a double
SDP_DEV bool viou_axis(double p, double org, double voxel, long long n, long long& i) {
  const double f = floor(__ddiv_rn(__dsub_rn(p, org), voxel));
  if (!(f >= 0.0 && f < (double)n)) return false;   // a NaN fails both compares
  i = (long long)f;
  return true;
}

// point i of cloud c: whether it is used, its composite key, and whether its label is outside [0, C)
SDP_DEV bool viou_point(const ViouArgs& a, const ViouCloud& c, int i, uint64_t& key, bool& bad) {
  bad = false;
  if (i >= c.n) return false;
  const int lab = c.labels ? c.labels[i] : 0;
  bad = lab < 0 || lab >= a.C;
  const double* p = c.p + (size_t)i * c.stride;
  const double x = p[0], y = p[1], z = p[2];
  if (bad || !(isfinite(x) && isfinite(y) && isfinite(z))) return false;
  long long ix, iy, iz;
  if (!viou_axis(x, a.org[0], a.voxel, a.nx, ix) || !viou_axis(y, a.org[1], a.voxel, a.ny, iy) ||
      !viou_axis(z, a.org[2], a.voxel, a.nz, iz))
    return false;
  const long long cell = ix + a.nx * iy + a.nx * a.ny * iz;
  if (a.valid && a.valid[cell] == 0) return false;
  key = ((uint64_t)cell << VIOU_LABEL_BITS) | (uint64_t)lab;
  return true;
}

__global__ __launch_bounds__(VIOU_CHUNK) void viou_count_kernel(ViouArgs a, int side) {
  __shared__ int wcnt[VIOU_CHUNK / 64], wbad[VIOU_CHUNK / 64];
  const ViouCloud& c = a.c[side];
  const int ch = blockIdx.x, i = ch * VIOU_CHUNK + threadIdx.x;
  uint64_t key = 0;
  bool bad = false;
  const bool use = viou_point(a, c, i, key, bad);
  chunk_post(use, wcnt);
  chunk_post(bad, wbad);
  __syncthreads();
  if (threadIdx.x == 0) {
    c.chunk_cnt[ch] = chunk_total(wcnt);
    c.chunk_bad[ch] = chunk_total(wbad);
  }
}

__global__ __launch_bounds__(SCAN_THREADS) void viou_hdr_kernel(ViouArgs a) {
  const ViouCloud& c = a.c[blockIdx.x];
  const int used = block_exclusive_scan(c.chunk_cnt, c.nchunks);
  const int bad = block_exclusive_scan(c.chunk_bad, c.nchunks);
  if (threadIdx.x != 0) return;
  ViouHdr* h = c.hdr;
  *h = ViouHdr{};   // m, skip and the sort state start at zero
  h->used = used;
  h->bad = bad;
  h->key_bits = a.key_bits;
}

__global__ __launch_bounds__(VIOU_CHUNK) void viou_keys_kernel(ViouArgs a, int side) {
  __shared__ int wcnt[VIOU_CHUNK / 64];
  const ViouCloud& c = a.c[side];
  const int ch = blockIdx.x, i = ch * VIOU_CHUNK + threadIdx.x;
  uint64_t key = 0;
  bool bad = false;
  const bool use = viou_point(a, c, i, key, bad);
  const unsigned long long m = chunk_post(use, wcnt);
  __syncthreads();
  if (!use) return;
  c.key0[(size_t)c.chunk_cnt[ch] + chunk_rank(m, wcnt)] = key;
}

// ---- segment heads of the sorted composite keys, by cell ----
SDP_DEV const uint64_t* viou_sorted(const ViouCloud& c) { return radix_result(c.hdr->sort) ? c.key1 : c.key0; }

__global__ __launch_bounds__(VIOU_CHUNK) void viou_head_count_kernel(ViouArgs a, int side) {
  __shared__ int wcnt[VIOU_CHUNK / 64];
  const ViouCloud& c = a.c[side];
  const uint64_t* k = viou_sorted(c);
  const int ch = blockIdx.x, i = ch * VIOU_CHUNK + threadIdx.x;
  const bool head = i < c.hdr->used && (i == 0 || (k[i] >> VIOU_LABEL_BITS) != (k[i - 1] >> VIOU_LABEL_BITS));
  chunk_post(head, wcnt);
  __syncthreads();
  if (threadIdx.x == 0) c.chunk_head[ch] = chunk_total(wcnt);
}

__global__ __launch_bounds__(SCAN_THREADS) void viou_scan_heads_kernel(ViouArgs a) {
  const ViouCloud& c = a.c[blockIdx.x];
  const int m = block_exclusive_scan(c.chunk_head, c.nchunks);
  if (threadIdx.x == 0) c.hdr->m = m;
}

__global__ __launch_bounds__(VIOU_CHUNK) void viou_head_scatter_kernel(ViouArgs a, int side) {
  __shared__ int wcnt[VIOU_CHUNK / 64];
  const ViouCloud& c = a.c[side];
  const uint64_t* k = viou_sorted(c);
  const int ch = blockIdx.x, i = ch * VIOU_CHUNK + threadIdx.x;
  uint64_t cell = 0;
  bool head = false;
  if (i < c.hdr->used) {
    cell = k[i] >> VIOU_LABEL_BITS;
    head = i == 0 || cell != (k[i - 1] >> VIOU_LABEL_BITS);
  }
  const unsigned long long m = chunk_post(head, wcnt);
  __syncthreads();
  if (!head) return;
  const int row = c.chunk_head[ch] + chunk_rank(m, wcnt);
  c.first[row] = i;
  c.cells[row] = (int64_t)cell;
  if (c.out_cells) c.out_cells[row] = (int64_t)cell;
}

// one thread per voxel: its segment of sorted keys is ascending in the label, so the first longest run is the
// smallest label among those with the most points
__global__ __launch_bounds__(VIOU_THREADS) void viou_vote_kernel(ViouArgs a, int side) {
  const ViouCloud& c = a.c[side];
  const uint64_t* k = viou_sorted(c);
  const int m = c.hdr->m, used = c.hdr->used;
  for (long long g = (long long)blockIdx.x * VIOU_THREADS + threadIdx.x; g < m; g += (long long)gridDim.x * VIOU_THREADS) {
    const int v = (int)g, b = c.first[v], e = v + 1 < m ? c.first[v + 1] : used;
    uint64_t cur = k[b], best = cur;
    int len = 1, best_len = 0;
    for (int j = b + 1; j < e; ++j) {
      const uint64_t x = k[j];
      if (x == cur) {
        ++len;
      } else {
        if (len > best_len) {   // strictly longer: among equals the first stays
          best_len = len;
          best = cur;
        }
        cur = x;
        len = 1;
      }
    }
    if (len > best_len) best = cur;
    const int lab = (int)(best & (uint64_t)(VIOU_MAX_CLASSES - 1));
    c.state[v] = lab;
    if (c.out_labels) c.out_labels[v] = lab;
    if (c.out_counts) c.out_counts[v] = e - b;
  }
}

// ---- the valid mask: non-zero bytes, 16 at a time over the aligned body ----
SDP_DEV int viou_nonzero_bytes(uint32_t w) {
  return __popc((((w & 0x7f7f7f7fu) + 0x7f7f7f7fu) | w) & 0x80808080u);
}

__global__ __launch_bounds__(VIOU_THREADS) void viou_valid_kernel(ViouArgs a) {
  __shared__ unsigned long long total;
  if (threadIdx.x == 0) total = 0;
  __syncthreads();
  const uint8_t* v = a.valid;
  const long long n = a.ncells;
  long long head = (long long)((16 - (reinterpret_cast<uintptr_t>(v) & 15)) & 15);
  if (head > n) head = n;
  const long long nvec = (n - head) / 16, tail0 = head + nvec * 16;
  const uint4* body = reinterpret_cast<const uint4*>(v + head);
  unsigned long long cnt = 0;
  for (long long j = (long long)blockIdx.x * VIOU_THREADS + threadIdx.x; j < nvec; j += (long long)gridDim.x * VIOU_THREADS) {
    const uint4 q = body[j];
    cnt += viou_nonzero_bytes(q.x) + viou_nonzero_bytes(q.y) + viou_nonzero_bytes(q.z) + viou_nonzero_bytes(q.w);
  }
  if (blockIdx.x == 0) {   // the unaligned ends: fewer than 16 bytes each
    for (long long j = threadIdx.x; j < head; j += VIOU_THREADS) cnt += v[j] != 0;
    for (long long j = tail0 + threadIdx.x; j < n; j += VIOU_THREADS) cnt += v[j] != 0;
  }
  atomicAdd(&total, cnt);
  __syncthreads();
  if (threadIdx.x == 0) a.valid_partial[blockIdx.x] = (int64_t)total;
}

// row of `cell` in the sorted unique cells[0..m), or -1
SDP_DEV int viou_find(const int64_t* cells, int m, int64_t cell) {
  int lo = 0, hi = m;
  while (lo < hi) {
    const int mid = (int)(((unsigned)lo + (unsigned)hi) >> 1);
    if (cells[mid] < cell) lo = mid + 1;
    else hi = mid;
  }
  return lo < m && cells[lo] == cell ? lo : -1;
}

__global__ __launch_bounds__(VIOU_THREADS) void viou_compare_kernel(ViouArgs a) {
  __shared__ unsigned int hist[VIOU_MAX_STATES * VIOU_MAX_STATES];   // a count is at most na + nb <= 2^31
  const int S = a.C + 1, SS = S * S;
  for (int j = threadIdx.x; j < SS; j += VIOU_THREADS) hist[j] = 0;
  __syncthreads();
  const ViouCloud& A = a.c[0];
  const ViouCloud& B = a.c[1];
  const int ma = A.hdr->m, mb = B.hdr->m;
  const long long stride = (long long)gridDim.x * VIOU_THREADS, t0 = (long long)blockIdx.x * VIOU_THREADS + threadIdx.x;
  for (long long g = t0; g < ma; g += stride) {
    const int r = viou_find(B.cells, mb, A.cells[g]);
    atomicAdd(&hist[(1 + A.state[g]) * S + (r < 0 ? 0 : 1 + B.state[r])], 1u);
  }
  for (long long g = t0; g < mb; g += stride) {
    if (viou_find(A.cells, ma, B.cells[g]) < 0) atomicAdd(&hist[1 + B.state[g]], 1u);
  }
  __syncthreads();
  for (int j = threadIdx.x; j < SS; j += VIOU_THREADS) a.partial[(size_t)blockIdx.x * SS + j] = hist[j];
}

__global__ __launch_bounds__(SCAN_THREADS) void viou_final_kernel(ViouArgs a, int nblocks) {
  __shared__ unsigned long long inter;
  if (threadIdx.x == 0) inter = 0;
  __syncthreads();
  const int S = a.C + 1, SS = S * S;
  unsigned long long mine = 0;
  for (int j = threadIdx.x; j < SS; j += SCAN_THREADS) {
    long long sum = 0;
    for (int b = 0; b < nblocks; ++b) sum += a.partial[(size_t)b * SS + j];
    if (j != 0) a.confusion[j] = sum;
    if (j / S > 0 && j % S > 0) mine += (unsigned long long)sum;
  }
  atomicAdd(&inter, mine);
  __syncthreads();
  if (threadIdx.x != 0) return;
  long long valid = a.ncells;
  if (a.valid) {
    valid = 0;
    for (int b = 0; b < VIOU_BLOCKS; ++b) valid += a.valid_partial[b];
  }
  const ViouHdr* ha = a.c[0].hdr;
  const ViouHdr* hb = a.c[1].hdr;
  a.confusion[0] = valid - ((long long)ha->m + hb->m - (long long)inter);
  a.info[0] = ha->m;
  a.info[1] = hb->m;
  a.info[2] = ha->used;
  a.info[3] = hb->used;
  a.info[4] = ha->bad;
  a.info[5] = hb->bad;
  a.info[6] = (long long)inter;
  a.info[7] = valid;
}

// measurement hook (sdp_voxel_iou_stage_events): start, after the keys, the sorts, the heads, the votes, the end
static thread_local StageEvents<6> viou_events;

// points the workspace arrays of both clouds into `w` (0: only count) and sets nchunks / ntiles; returns the bytes
static size_t viou_place(ViouArgs& a, int64_t na, int64_t nb, int num_classes, uintptr_t w) {
  Layout l{w};
  l.take(a.partial, (size_t)VIOU_BLOCKS * (num_classes + 1) * (num_classes + 1) * 4);
  l.take(a.valid_partial, (size_t)VIOU_BLOCKS * 8);
  for (int s = 0; s < 2; ++s) {
    ViouCloud& c = a.c[s];
    const int64_t n = s == 0 ? na : nb, cap = n > 0 ? n : 1;   // an empty cloud still launches one workgroup
    c.nchunks = (int)((cap + VIOU_CHUNK - 1) / VIOU_CHUNK);
    c.ntiles = (int)((cap + VIOU_SORT_TILE - 1) / VIOU_SORT_TILE);
    l.take(c.hdr, sizeof(ViouHdr));
    l.take(c.chunk_cnt, (size_t)c.nchunks * 4);
    l.take(c.chunk_bad, (size_t)c.nchunks * 4);
    l.take(c.chunk_head, (size_t)c.nchunks * 4);
    l.take(c.tile_cnt, (size_t)c.ntiles * 256 * 4);
    l.take(c.key0, (size_t)cap * 8);
    l.take(c.key1, (size_t)cap * 8);
    l.take(c.first, (size_t)cap * 4);
    l.take(c.cells, (size_t)cap * 8);
    l.take(c.state, (size_t)cap * 4);
  }
  return l.bytes;
}

static int viou_blocks(int64_t work) {
  const int64_t b = (work + VIOU_THREADS - 1) / VIOU_THREADS;
  return (int)(b < 1 ? 1 : b > VIOU_BLOCKS ? VIOU_BLOCKS : b);
}

}  // namespace sdp

extern "C" {

int sdp_voxel_iou_workspace_size(int64_t na, int64_t nb, int num_classes, size_t* bytes) {
  using namespace sdp;
  if (!bytes || na < 0 || nb < 0 || na > VIOU_MAX_N || nb > VIOU_MAX_N)
    return sdp_fail("sdp_voxel_iou_workspace_size: na and nb must be in [0, 2^30]");
  if (num_classes < 1 || num_classes > VIOU_MAX_CLASSES) return sdp_fail("sdp_voxel_iou_workspace_size: num_classes must be in [1, 64]");
  ViouArgs a{};
  *bytes = viou_place(a, na, nb, num_classes, 0);
  return 0;
}

int sdp_voxel_iou_stage_events(void* const* events) { return sdp::viou_events.set(events, "sdp_voxel_iou_stage_events"); }

int sdp_voxel_iou(const double* pa, int64_t na, int astride, const int32_t* a_labels, const double* pb, int64_t nb,
                  int bstride, const int32_t* b_labels, const double* origin, double voxel, const int64_t* dims,
                  int num_classes, const uint8_t* valid, int64_t* confusion, int64_t* a_cells, int32_t* a_cell_labels,
                  int32_t* a_cell_counts, int64_t* b_cells, int32_t* b_cell_labels, int32_t* b_cell_counts, int64_t* info,
                  void* workspace, size_t workspace_bytes, void* stream) {
  using namespace sdp;
  if (na < 0 || nb < 0 || na > VIOU_MAX_N || nb > VIOU_MAX_N)
    return sdp_fail("sdp_voxel_iou: na and nb must be in [0, 2^30] (rows are int32)");
  if ((astride != 3 && astride != 4) || (bstride != 3 && bstride != 4)) return sdp_fail("sdp_voxel_iou: stride must be 3 or 4");
  if (!origin || !dims || !confusion || !info || !workspace || (na > 0 && !pa) || (nb > 0 && !pb))
    return sdp_fail("sdp_voxel_iou: null argument");
  if (!(voxel > 0.0) || !std::isfinite(voxel)) return sdp_fail("sdp_voxel_iou: voxel must be > 0 and finite");
  if (!std::isfinite(origin[0]) || !std::isfinite(origin[1]) || !std::isfinite(origin[2]))
    return sdp_fail("sdp_voxel_iou: origin must be finite");
  if (num_classes < 1 || num_classes > VIOU_MAX_CLASSES) return sdp_fail("sdp_voxel_iou: num_classes must be in [1, 64]");
  if (dims[0] < 1 || dims[1] < 1 || dims[2] < 1) return sdp_fail("sdp_voxel_iou: every dim must be >= 1");
  if (dims[0] > VIOU_MAX_CELLS || dims[1] > VIOU_MAX_CELLS / dims[0] || dims[2] > VIOU_MAX_CELLS / (dims[0] * dims[1]))
    return sdp_fail("sdp_voxel_iou: the grid must not exceed 2^40 cells");
  const int64_t ncells = dims[0] * dims[1] * dims[2];
  if (valid && ncells > VIOU_MAX_MASK_CELLS) return sdp_fail("sdp_voxel_iou: a valid mask needs a grid of at most 2^31 cells");
  ViouArgs a{};
  if (workspace_bytes < viou_place(a, na, nb, num_classes, reinterpret_cast<uintptr_t>(workspace)))
    return sdp_fail("sdp_voxel_iou: workspace too small");
  if (reinterpret_cast<uintptr_t>(workspace) % 16) return sdp_fail("sdp_voxel_iou: workspace must be 16-byte aligned");
  a.c[0].p = pa;
  a.c[0].labels = a_labels;
  a.c[0].n = (int)na;
  a.c[0].stride = astride;
  a.c[0].out_cells = a_cells;
  a.c[0].out_labels = a_cell_labels;
  a.c[0].out_counts = a_cell_counts;
  a.c[1].p = pb;
  a.c[1].labels = b_labels;
  a.c[1].n = (int)nb;
  a.c[1].stride = bstride;
  a.c[1].out_cells = b_cells;
  a.c[1].out_labels = b_cell_labels;
  a.c[1].out_counts = b_cell_counts;
  for (int k = 0; k < 3; ++k) a.org[k] = origin[k];
  a.voxel = voxel;
  a.nx = dims[0];
  a.ny = dims[1];
  a.nz = dims[2];
  a.ncells = ncells;
  a.C = num_classes;
  int cell_bits = 0;
  while (cell_bits < 40 && (1ll << cell_bits) < ncells) ++cell_bits;
  a.key_bits = cell_bits + VIOU_LABEL_BITS;
  const int passes = (a.key_bits + 7) / 8;   // 6 at most
  a.valid = valid;
  a.confusion = confusion;
  a.info = info;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const dim3 one(1), two(2), chunk(VIOU_CHUNK), scan(SCAN_THREADS), threads(VIOU_THREADS);
  viou_events.mark(0, st);
  for (int s = 0; s < 2; ++s) hipLaunchKernelGGL(viou_count_kernel, dim3(a.c[s].nchunks), chunk, 0, st, a, s);
  hipLaunchKernelGGL(viou_hdr_kernel, two, scan, 0, st, a);
  for (int s = 0; s < 2; ++s) hipLaunchKernelGGL(viou_keys_kernel, dim3(a.c[s].nchunks), chunk, 0, st, a, s);
  viou_events.mark(1, st);
  for (int s = 0; s < 2; ++s) {
    const ViouCloud& c = a.c[s];
    ViouHdr* h = c.hdr;   // a device pointer: only addresses are taken here
    const RadixArgs r{c.key0, c.key1, nullptr, nullptr, c.tile_cnt, c.ntiles, &h->used, &h->key_bits, &h->skip, &h->sort};
    radix_sort(r, passes, st);
  }
  viou_events.mark(2, st);
  for (int s = 0; s < 2; ++s) hipLaunchKernelGGL(viou_head_count_kernel, dim3(a.c[s].nchunks), chunk, 0, st, a, s);
  hipLaunchKernelGGL(viou_scan_heads_kernel, two, scan, 0, st, a);
  for (int s = 0; s < 2; ++s) hipLaunchKernelGGL(viou_head_scatter_kernel, dim3(a.c[s].nchunks), chunk, 0, st, a, s);
  viou_events.mark(3, st);
  for (int s = 0; s < 2; ++s) {
    const int64_t blocks = ((int64_t)a.c[s].n + VIOU_THREADS - 1) / VIOU_THREADS;
    hipLaunchKernelGGL(viou_vote_kernel, dim3((unsigned)(blocks < 1 ? 1 : blocks > 262144 ? 262144 : blocks)), threads, 0, st, a, s);
  }
  viou_events.mark(4, st);
  if (valid) hipLaunchKernelGGL(viou_valid_kernel, dim3(VIOU_BLOCKS), threads, 0, st, a);
  const int cblocks = viou_blocks(na > nb ? na : nb);
  hipLaunchKernelGGL(viou_compare_kernel, dim3(cblocks), threads, 0, st, a);
  hipLaunchKernelGGL(viou_final_kernel, one, scan, 0, st, a, cblocks);
  viou_events.mark(5, st);
  return launch_status("sdp_voxel_iou");
}

}  // extern "C"
