// Stable LSD radix sort on the device (radix_sort.h): per 8-bit digit
//   radix_hist_kernel     per tile of RADIX_TILE elements: the count of every digit (integer LDS atomics)
//   radix_scan_kernel     ONE workgroup: exclusive scan of the digit-major counts [256][ntiles] -> first output
//                         rows; decides whether the pass moves anything and where the next one reads
//   radix_scatter_kernel  every element to its row
// The rank of an element inside its tile and digit is a wave ballot (lanes below with the same digit) plus an LDS
// prefix over the (round, wave) slots of the tile in element order -- never the order in which atomics land -- so
// the sort is stable.  A pass at or beyond the key bits, or one whose digit is the same for every key, moves
// nothing and leaves the ping/pong index (RadixState::src) where it was.  No workgroup waits for another.
#include "device_prims.h"
#include "radix_sort.h"

namespace sdp {

constexpr int RADIX_SLOTS = RADIX_ROUNDS * (RADIX_THREADS / 64);

__global__ __launch_bounds__(RADIX_THREADS) void radix_hist_kernel(RadixArgs a, int pass) {
  __shared__ int hist[256];
  if (*a.skip || pass * 8 >= *a.bits) return;
  const int n = *a.n, tid = threadIdx.x, tile = blockIdx.x;
  const uint64_t* k = a.state->src[pass] ? a.key1 : a.key0;
  hist[tid] = 0;
  __syncthreads();
#pragma unroll
  for (int r = 0; r < RADIX_ROUNDS; ++r) {
    const int e = tile * RADIX_TILE + r * RADIX_THREADS + tid;
    if (e < n) atomicAdd(&hist[(int)((k[e] >> (8 * pass)) & 255)], 1);
  }
  __syncthreads();
  a.tile_cnt[(size_t)tid * a.ntiles + tile] = hist[tid];
}

__global__ __launch_bounds__(SCAN_THREADS) void radix_scan_kernel(RadixArgs a, int pass) {
  __shared__ int same;
  if (*a.skip) return;
  RadixState* st = a.state;
  const int tid = threadIdx.x, s = st->src[pass];
  auto decide = [&](int act) {   // by one thread: does the pass move anything, and where the next one reads
    st->active[pass] = act;
    st->src[pass + 1] = st->result = s ^ act;
  };
  if (pass * 8 >= *a.bits) {
    if (tid == 0) decide(0);
    return;
  }
  if (tid == 0) same = 0;
  const int total = block_exclusive_scan(a.tile_cnt, 256 * a.ntiles);
  // one digit holds every key: the pass would be the identity, so it is skipped like one beyond the key bits
  if (tid < 256) {
    const int end = tid == 255 ? total : a.tile_cnt[(size_t)(tid + 1) * a.ntiles];
    if (end - a.tile_cnt[(size_t)tid * a.ntiles] == total) same = 1;
  }
  __syncthreads();
  if (tid == 0) decide((same || total == 0) ? 0 : 1);
}

__global__ __launch_bounds__(RADIX_THREADS) void radix_scatter_kernel(RadixArgs a, int pass) {
  __shared__ int wh[RADIX_SLOTS][256];   // per (round, wave) slot, in element order: count, then first output row
  const RadixState* st = a.state;
  if (*a.skip || !st->active[pass]) return;
  const int n = *a.n, tid = threadIdx.x, tile = blockIdx.x, lane = tid & 63, wv = tid >> 6;
  const int s = st->src[pass];
  const bool vals = a.val0 != nullptr;
  const uint64_t* kin = s ? a.key1 : a.key0;
  uint64_t* kout = s ? a.key0 : a.key1;
  const uint32_t* vin = s ? a.val1 : a.val0;
  uint32_t* vout = s ? a.val0 : a.val1;
  for (int j = tid; j < RADIX_SLOTS * 256; j += RADIX_THREADS) (&wh[0][0])[j] = 0;
  __syncthreads();
  uint64_t kk[RADIX_ROUNDS];
  uint32_t vv[RADIX_ROUNDS];
  int rk[RADIX_ROUNDS], dg[RADIX_ROUNDS];
#pragma unroll
  for (int r = 0; r < RADIX_ROUNDS; ++r) {
    const int e = tile * RADIX_TILE + r * RADIX_THREADS + tid;
    const bool valid = e < n;
    kk[r] = valid ? kin[e] : 0;
    vv[r] = (valid && vals) ? vin[e] : 0;
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
    if (valid && rk[r] == 0) wh[r * (RADIX_THREADS / 64) + wv][d] = __popcll(peers);
  }
  __syncthreads();
  int run = a.tile_cnt[(size_t)tid * a.ntiles + tile];   // first output row of (digit tid, this tile)
#pragma unroll
  for (int q = 0; q < RADIX_SLOTS; ++q) {
    const int t = wh[q][tid];
    wh[q][tid] = run;
    run += t;
  }
  __syncthreads();
#pragma unroll
  for (int r = 0; r < RADIX_ROUNDS; ++r) {
    const int e = tile * RADIX_TILE + r * RADIX_THREADS + tid;
    if (e < n) {
      const int pos = wh[r * (RADIX_THREADS / 64) + wv][dg[r]] + rk[r];
      kout[pos] = kk[r];
      if (vals) vout[pos] = vv[r];
    }
  }
}

void radix_sort(const RadixArgs& a, int passes, hipStream_t st) {
  const dim3 tiles(a.ntiles), one(1);
  for (int p = 0; p < passes; ++p) {
    hipLaunchKernelGGL(radix_hist_kernel, tiles, dim3(RADIX_THREADS), 0, st, a, p);
    hipLaunchKernelGGL(radix_scan_kernel, one, dim3(SCAN_THREADS), 0, st, a, p);
    hipLaunchKernelGGL(radix_scatter_kernel, tiles, dim3(RADIX_THREADS), 0, st, a, p);
  }
}

__global__ __launch_bounds__(SCAN_THREADS) void block_scan_kernel(int32_t* data, int n, int32_t* total) {
  const int t = block_exclusive_scan(data, n);
  if (threadIdx.x == 0) *total = t;
}

hipError_t block_scan(int32_t* data, int n, int32_t* total, hipStream_t st) {
  hipLaunchKernelGGL(block_scan_kernel, dim3(1), dim3(SCAN_THREADS), 0, st, data, n, total);
  return hipGetLastError();
}

}  // namespace sdp
