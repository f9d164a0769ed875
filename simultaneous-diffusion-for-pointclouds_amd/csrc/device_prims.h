// In-kernel building blocks of the point-cloud back end (unproject.hip, voxel_grid.hip, radix_sort.hip; DESIGN.md
// section 4, "Shared device primitives"): each exists once, here.  Integer arithmetic and fminf / fmaxf only, so
// the results do not depend on the order of anything; every file that includes this is built with -ffp-contract=off.
#pragma once
#include "common.h"

namespace sdp {

constexpr int SCAN_THREADS = 1024;    // the one workgroup of every scan kernel
constexpr int SCAN_PER_THREAD = 4;    // consecutive counts per thread: 4096 counts per iteration
constexpr int CHUNK_THREADS = 256;    // a compaction workgroup: one element per thread, four waves

// Exclusive scan of data[0..n) in place by the whole (one) workgroup of SCAN_THREADS; every thread gets the total,
// which the caller keeps below 2^31.  Per iteration: a __shfl_up scan inside each wave, an LDS prefix over the
// waves, a running carry.  After the last barrier the caller may read data[].
SDP_DEV int block_exclusive_scan(int32_t* data, int n) {
  __shared__ int wsum[SCAN_THREADS / 64];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  int carry = 0;
  for (int t0 = 0; t0 < n; t0 += SCAN_THREADS * SCAN_PER_THREAD) {
    const int i0 = t0 + tid * SCAN_PER_THREAD;
    int c[SCAN_PER_THREAD], cnt = 0;
#pragma unroll
    for (int k = 0; k < SCAN_PER_THREAD; ++k) {
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
    for (int k = 0; k < SCAN_THREADS / 64; ++k) {
      before += k < wv ? wsum[k] : 0;
      total += wsum[k];
    }
    int base = carry + before + (inc - cnt);
#pragma unroll
    for (int k = 0; k < SCAN_PER_THREAD; ++k) {
      if (i0 + k < n) data[i0 + k] = base;
      base += c[k];
    }
    carry += total;
    __syncthreads();   // wsum is rewritten by the next iteration; the stores are visible to the workgroup
  }
  return carry;
}

// Count and rank of a per-thread flag over a workgroup of CHUNK_THREADS, in two halves around ONE barrier that the
// caller owns (and shares with whatever else it posts to LDS); wcnt is its __shared__ int[CHUNK_THREADS / 64]:
//   m = chunk_post(flag, wcnt) by every thread;  __syncthreads();  chunk_total(wcnt)  /  chunk_rank(m, wcnt)
SDP_DEV unsigned long long chunk_post(bool flag, int* wcnt) {
  const unsigned long long m = __ballot(flag);
  if ((threadIdx.x & 63) == 0) wcnt[threadIdx.x >> 6] = __popcll(m);
  return m;
}

static_assert(CHUNK_THREADS / 64 == 4, "chunk_total adds four waves");
SDP_DEV int chunk_total(const int* wcnt) { return wcnt[0] + wcnt[1] + wcnt[2] + wcnt[3]; }

// flagged threads before this one in the workgroup (the inclusive rank is this plus the thread's own flag)
SDP_DEV int chunk_rank(unsigned long long m, const int* wcnt) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  int rank = __popcll(m & ((1ull << lane) - 1ull));
  for (int k = 0; k < wv; ++k) rank += wcnt[k];
  return rank;
}

// v[0..3) minima, v[3..6) maxima: reduced over the wave, the result in every lane and, by lane 0, in post[0..6)
SDP_DEV void wave_minmax3(float (&v)[6], float* post) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      v[k] = fminf(v[k], __shfl_xor(v[k], o, 64));
      v[k + 3] = fmaxf(v[k + 3], __shfl_xor(v[k + 3], o, 64));
    }
  }
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int k = 0; k < 6; ++k) post[k] = v[k];
  }
}

}  // namespace sdp
