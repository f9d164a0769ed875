// Stable LSD radix sort of 64-bit keys (with optional 32-bit values) on the device, 8-bit digits, between two
// ping/pong buffers (radix_sort.hip; DESIGN.md section 4, "Shared device primitives").  The element count, the key
// width and whether to sort at all are read from device memory: a sort is enqueued before they are known.
#pragma once
#include <cstdint>

#include <hip/hip_runtime.h>

namespace sdp {

constexpr int RADIX_THREADS = 256;     // threads of a sort workgroup: one per digit, four waves
constexpr int RADIX_ROUNDS = 4;        // elements per thread
constexpr int RADIX_TILE = 1024;       // elements per sort workgroup
constexpr int RADIX_MAX_PASSES = 8;    // 64-bit keys
static_assert(RADIX_THREADS == 256 && RADIX_TILE == RADIX_THREADS * RADIX_ROUNDS, "thread = digit, tile");

// Device state of one sort.  The owner zeroes it before the first pass; src[0] stays 0, so the input is always in
// buffer 0 and a state may be reused for one sort after another.
struct RadixState {
  int src[RADIX_MAX_PASSES + 1];   // the buffer (0 | 1) pass p reads
  int active[RADIX_MAX_PASSES];    // 0: pass p is at or beyond the key bits, or its digit is the same for every key
  int result;                      // the buffer that holds the sorted elements after the last pass that ran
};

// the buffer the consumers of a finished sort read
__host__ __device__ inline int radix_result(const RadixState& s) { return s.result; }

struct RadixArgs {
  uint64_t* key0;
  uint64_t* key1;
  uint32_t* val0;        // both null: keys only
  uint32_t* val1;
  int32_t* tile_cnt;     // [256][ntiles] digit-major counts, after the scan the first output rows
  int ntiles;            // >= ceil(*n / RADIX_TILE)
  const int* n;          // device: elements
  const int* bits;       // device: key width; passes at or beyond it move nothing
  const int* skip;       // device: non-zero = do nothing at all (buffers and state stay as they are)
  RadixState* state;
};

// `passes` x { histogram, digit scan, scatter } on `st`: digits 0 .. passes-1 of the keys in buffer 0
void radix_sort(const RadixArgs& a, int passes, hipStream_t st);

// one workgroup: block_exclusive_scan (device_prims.h) of data[0..n) in place, the total to *total (the kernel test)
hipError_t block_scan(int32_t* data, int n, int32_t* total, hipStream_t st);

}  // namespace sdp
