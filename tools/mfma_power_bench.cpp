// Full-chip bare MFMA loop: v_mfma_f32_32x32x16_bf16 vs v_mfma_f32_16x16x32_bf16 at equal
// FLOPs per wave, operands re-read from LDS every step (as a conv main loop does), one wave
// per SIMD, every CU busy for ~0.2 s -- does the smaller instruction run at a higher clock
// when the chip is power-limited?  Usage: mfma_power_bench [iters]
//
// mfma_power_bench reads [iters [rounds]]: the A-read knob of the 16x16x32 loop (kr<RD> below) -- the conv's 8 x 16
// tile (32-Cout waves, two per SIMD, fp32x3: 3 MFMAs per block, 16 blocks per tap) with RD ds_read_b128 per three
// taps = 144 MFMAs: 48 = a tap reads its 8 fragments hi and lo (16 per 48 MFMAs), 20 = each patch row once per
// column offset (60 per 9 taps = 6.7 per 48 MFMAs), 0 = none.  Random operands, variants interleaved over the rounds
// in one process; per run the wall time and the in-kernel clock (s_memtime ticks over s_memrealtime's 100 MHz).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(16))) float f32x16;
typedef __attribute__((ext_vector_type(4))) float f32x4;

#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("HIP %s @%d\n", hipGetErrorString(e_), __LINE__); exit(1); } } while (0)

// 32x32x16: 8 accumulators (128 regs), per step 4 A reads + 2 B reads -> 8 MFMAs (like the conv)
__global__ __launch_bounds__(256, 1) void k32(float* out, int iters, unsigned long long* clk) {
  __shared__ __attribute__((aligned(16))) char lds[64 * 1024];
  const int lane = threadIdx.x & 63;
  for (int i = threadIdx.x; i < 64 * 1024 / 4; i += 256) reinterpret_cast<float*>(lds)[i] = (float)(i % 7) * 0.01f;
  __syncthreads();
  f32x16 acc[4][2] = {};
  const unsigned long long t0 = __builtin_amdgcn_s_memtime();
  for (int it = 0; it < iters; ++it) {
    bf16x8 a[4], b[2];
#pragma unroll
    for (int m = 0; m < 4; ++m) a[m] = *reinterpret_cast<const bf16x8*>(lds + ((it * 4 + m) & 63) * 1024 + lane * 16);
#pragma unroll
    for (int n = 0; n < 2; ++n) b[n] = *reinterpret_cast<const bf16x8*>(lds + ((it * 2 + n + 32) & 63) * 1024 + lane * 16);
#pragma unroll
    for (int m = 0; m < 4; ++m)
#pragma unroll
      for (int n = 0; n < 2; ++n) acc[m][n] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[m], b[n], acc[m][n], 0, 0, 0);
  }
  const unsigned long long t1 = __builtin_amdgcn_s_memtime();
  float s = 0.f;
#pragma unroll
  for (int m = 0; m < 4; ++m)
#pragma unroll
    for (int n = 0; n < 2; ++n)
#pragma unroll
      for (int r = 0; r < 16; ++r) s += acc[m][n][r];
  out[blockIdx.x * 256 + threadIdx.x] = s;
  if (threadIdx.x == 0) clk[blockIdx.x] = t1 - t0;
}

// 16x16x32: 32 accumulators (128 regs), per step 8 A reads + 4 B reads -> 32 MFMAs = same FLOPs
__global__ __launch_bounds__(256, 1) void k16(float* out, int iters, unsigned long long* clk) {
  __shared__ __attribute__((aligned(16))) char lds[64 * 1024];
  const int lane = threadIdx.x & 63;
  for (int i = threadIdx.x; i < 64 * 1024 / 4; i += 256) reinterpret_cast<float*>(lds)[i] = (float)(i % 7) * 0.01f;
  __syncthreads();
  f32x4 acc[8][4] = {};
  const unsigned long long t0 = __builtin_amdgcn_s_memtime();
  for (int it = 0; it < iters; ++it) {
    bf16x8 a[8], b[4];
#pragma unroll
    for (int m = 0; m < 8; ++m) a[m] = *reinterpret_cast<const bf16x8*>(lds + ((it * 8 + m) & 63) * 1024 + lane * 16);
#pragma unroll
    for (int n = 0; n < 4; ++n) b[n] = *reinterpret_cast<const bf16x8*>(lds + ((it * 4 + n + 32) & 63) * 1024 + lane * 16);
#pragma unroll
    for (int m = 0; m < 8; ++m)
#pragma unroll
      for (int n = 0; n < 4; ++n) acc[m][n] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[m], b[n], acc[m][n], 0, 0, 0);
  }
  const unsigned long long t1 = __builtin_amdgcn_s_memtime();
  float s = 0.f;
#pragma unroll
  for (int m = 0; m < 8; ++m)
#pragma unroll
    for (int n = 0; n < 4; ++n)
#pragma unroll
      for (int r = 0; r < 4; ++r) s += acc[m][n][r];
  out[blockIdx.x * 256 + threadIdx.x] = s;
  if (threadIdx.x == 0) clk[blockIdx.x] = t1 - t0;
}

// Block (tap, s, nj, i) multiplies the A fragment (hi, lo) of the 16-px group mb = 4 s + i by the two weight fragments.
// RD 48: the fragments of the group, a[.][mb]; blocks 0 .. 7 read the tap's groups 4 .. 7, blocks 8 .. 15 the next
// tap's 0 .. 3 (one read per block, hi / lo alternating).  RD 20 (and 0): patch row mb + tap of a 10-row ring;
// rows 8 and 9 come under tap 0, and the next three taps' rows under this one's as their registers retire (row 0
// in tap 0, row 1 in tap 1, rows 2 .. 7 in tap 2).  Every read is used; the conv's lane pattern (16 pixels of 144 B x 4
// channel groups), at an address that moves every iteration.
template <int RD>
__global__ __launch_bounds__(256, 2) void kr(float* out, const uint4* rnd, int iters, unsigned long long* clk) {
  __shared__ __attribute__((aligned(16))) char lds[64 * 1024];
  const int lane = threadIdx.x & 63;
  for (int i = threadIdx.x; i < 64 * 1024 / 16; i += 256) reinterpret_cast<uint4*>(lds)[i] = rnd[i];
  __syncthreads();
  const char* base = lds + (lane & 15) * 144 + (lane >> 4) * 16;
  bf16x8 a[2][10], b[4];
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    a[0][r] = *reinterpret_cast<const bf16x8*>(base + r * 2592);
    a[1][r] = *reinterpret_cast<const bf16x8*>(base + r * 2592 + 64);
  }
#pragma unroll
  for (int n = 0; n < 4; ++n) {
    const uint4 v = rnd[4096 + n * 64 + lane];
    b[n] = *reinterpret_cast<const bf16x8*>(&v);
  }
  f32x4 acc[8][2] = {};
  const unsigned long long t0 = __builtin_amdgcn_s_memtime(), r0 = __builtin_amdgcn_s_memrealtime();
  for (int it = 0; it < iters; ++it) {
    const char* p = base + (it % 12) * 2592;
#pragma unroll
    for (int blk = 0; blk < 48; ++blk) {
      const int tap = blk / 16, bb = blk % 16, mb = 4 * (bb / 8) + (bb & 3), nj = (bb / 4) % 2;
      const int row = RD == 48 ? mb : mb + tap;
      acc[mb][nj] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[1][row], b[2 * nj], acc[mb][nj], 0, 0, 0);
      acc[mb][nj] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[0][row], b[2 * nj + 1], acc[mb][nj], 0, 0, 0);
      acc[mb][nj] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[0][row], b[2 * nj], acc[mb][nj], 0, 0, 0);
      int dst = -1, part = bb & 1;
      if (RD == 48) dst = bb < 8 ? 4 + bb / 2 : (bb - 8) / 2;
      if (RD == 20) {
        if (tap == 0 && bb < 4) dst = 8 + bb / 2;
        if (tap == 0 && (bb == 12 || bb == 13)) dst = 0;
        if (tap == 1 && (bb == 8 || bb == 10)) dst = 1, part = bb == 10;
        if (tap == 2 && bb >= 4) dst = 2 + (bb - 4) / 2;
      }
      if (dst >= 0)
        a[part][dst] = *reinterpret_cast<const bf16x8*>(p + ((blk / 2) % 12) * 2592 + (blk % 3) * 144 + part * 64);
      __builtin_amdgcn_sched_barrier(0);
    }
  }
  const unsigned long long t1 = __builtin_amdgcn_s_memtime(), r1 = __builtin_amdgcn_s_memrealtime();
  float s = 0.f;
#pragma unroll
  for (int m = 0; m < 8; ++m)
#pragma unroll
    for (int n = 0; n < 2; ++n)
#pragma unroll
      for (int r = 0; r < 4; ++r) s += acc[m][n][r];
  out[blockIdx.x * 256 + threadIdx.x] = s;
  if (threadIdx.x == 0) {
    clk[2 * blockIdx.x] = t1 - t0;
    clk[2 * blockIdx.x + 1] = r1 - r0;
  }
}

static int reads_bench(int iters, int rounds) {
  const int nwg = 256 * 2 * 2;   // two workgroups per CU = two waves per SIMD, two rounds of them
  float* out;
  unsigned long long* clk;
  uint4* rnd;
  CK(hipMalloc(&out, nwg * 256 * 4));
  CK(hipMalloc(&clk, nwg * 16));
  CK(hipMalloc(&rnd, (4096 + 256) * 16));
  std::vector<unsigned short> h((4096 + 256) * 8);
  unsigned long long st = 0x9E3779B97F4A7C15ull;
  for (auto& v : h) {   // random bf16 in (-2, 2): top 16 bits of a float with a random sign, mantissa and 0 - 7 exponent steps down
    st = st * 6364136223846793005ull + 1442695040888963407ull;
    const unsigned r = (unsigned)(st >> 33);
    v = (unsigned short)(((r & 1u) << 15) | ((127u - ((r >> 1) & 7u)) << 7) | ((r >> 4) & 0x7fu));
  }
  CK(hipMemcpy(rnd, h.data(), h.size() * 2, hipMemcpyHostToDevice));
  std::vector<unsigned long long> hc(2 * nwg);
  const int RDS[3] = {48, 20, 0};
  for (int round = -1; round < rounds; ++round) {   // round -1: warm-up (not printed)
    for (int v = 0; v < 3; ++v) {
      hipEvent_t e0, e1;
      CK(hipEventCreate(&e0));
      CK(hipEventCreate(&e1));
      CK(hipEventRecord(e0, 0));
      if (v == 0) hipLaunchKernelGGL(kr<48>, dim3(nwg), dim3(256), 0, 0, out, rnd, iters, clk);
      else if (v == 1) hipLaunchKernelGGL(kr<20>, dim3(nwg), dim3(256), 0, 0, out, rnd, iters, clk);
      else hipLaunchKernelGGL(kr<0>, dim3(nwg), dim3(256), 0, 0, out, rnd, iters, clk);
      CK(hipEventRecord(e1, 0));
      CK(hipEventSynchronize(e1));
      float ms;
      CK(hipEventElapsedTime(&ms, e0, e1));
      CK(hipMemcpy(hc.data(), clk, nwg * 16, hipMemcpyDeviceToHost));
      CK(hipEventDestroy(e0));
      CK(hipEventDestroy(e1));
      std::vector<double> ghz(nwg), tk(nwg);
      for (int i = 0; i < nwg; ++i) {
        tk[i] = (double)hc[2 * i];
        ghz[i] = (double)hc[2 * i] / (double)(hc[2 * i + 1] ? hc[2 * i + 1] : 1) * 0.1;
      }
      std::sort(ghz.begin(), ghz.end());
      std::sort(tk.begin(), tk.end());
      if (round < 0) continue;
      printf("reads/144 MFMA %2d (%.1f per 48) round %d: %8.2f ms  ticks per MFMA (median WG) %.2f  in-kernel clock %.3f GHz\n",
             RDS[v], RDS[v] / 3.0, round, ms, tk[nwg / 2] / (144.0 * iters), ghz[nwg / 2]);
    }
  }
  return 0;
}

int main(int argc, char** argv) {
  if (argc > 1 && !strcmp(argv[1], "reads")) return reads_bench(argc > 2 ? atoi(argv[2]) : 20000, argc > 3 ? atoi(argv[3]) : 4);
  const int iters = argc > 1 ? atoi(argv[1]) : 20000;
  const int nwg = 256 * 2;
  float* out;
  unsigned long long* clk;
  CK(hipMalloc(&out, nwg * 256 * 4));
  CK(hipMalloc(&clk, nwg * 8));
  unsigned long long hc[512];
  for (int v = 0; v < 2; ++v) {
    for (int rep = 0; rep < 3; ++rep) {
      hipEvent_t e0, e1;
      CK(hipEventCreate(&e0));
      CK(hipEventCreate(&e1));
      CK(hipEventRecord(e0, 0));
      if (v == 0) hipLaunchKernelGGL(k32, dim3(nwg), dim3(256), 0, 0, out, iters, clk);
      else hipLaunchKernelGGL(k16, dim3(nwg), dim3(256), 0, 0, out, iters, clk);
      CK(hipEventRecord(e1, 0));
      CK(hipEventSynchronize(e1));
      float ms;
      CK(hipEventElapsedTime(&ms, e0, e1));
      CK(hipMemcpy(hc, clk, nwg * 8, hipMemcpyDeviceToHost));
      double avg = 0;
      for (int i = 0; i < nwg; ++i) avg += (double)hc[i];
      avg /= nwg;
      // FLOPs: per wave per iter 8 x (32*32*16*2) = 262144 (both variants)
      const double fl = (double)nwg * 4 * iters * 262144.0;
      const double mf = (v == 0 ? 8.0 : 32.0) * iters;
      printf("%s rep %d: %.2f ms  %.0f TFLOP/s  ticks/WG %.0f  ticks per MFMA %.2f  implied clock %.2f GHz\n",
             v == 0 ? "32x32x16" : "16x16x32", rep, ms, fl / ms * 1e-9, avg, avg / mf, avg / (ms * 1e-3 / 2) * 1e-9);
    }
  }
  return 0;
}
