// devutil.h -- the leaf helpers of the gfx950 kernels (wave64): index arithmetic, wave primitives, unaligned loads, the counter-based mixer.  One definition each;
// common.h includes this header, so every translation unit has them.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

__host__ __device__ static inline int div_up(int a, int b) { return (a + b - 1) / b; }

// Workgroup b of a launch is observed on XCD b % 8 (nothing promises it: speed only, never correctness).  Kernels whose neighbouring tiles share cache lines take their tile from
// this bijective remap of the linear workgroup index instead: XCD x works through the contiguous range [x * n / 8, (x + 1) * n / 8) in dispatch order, so the lines two neighbours
// share arrive in ONE L2 (any n, also n % 8 != 0).
__device__ __forceinline__ unsigned xcd_contiguous(unsigned id, unsigned n) {
  const unsigned q = n >> 3, r = n & 7u, x = id & 7u, k = id >> 3;
  return (x < r ? x * (q + 1) : r * (q + 1) + (x - r) * q) + k;
}

__device__ __forceinline__ int lane_id() { return threadIdx.x & 63; }

// wave64 reduction (DPP/bpermute via __shfl; no LDS, no volatile warp idioms): every lane returns the sum.  T: int, float, double, unsigned long long
template <class T>
__device__ __forceinline__ T wave_sum(T v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// value of lane `lane` of a 64-bit quantity: a readlane of each half (lane is wave-uniform; a compile-time constant after unrolling where that matters)
__device__ __forceinline__ double lane_bcast(double v, int lane) {
  const int lo = __builtin_amdgcn_readlane(__double2loint(v), lane), hi = __builtin_amdgcn_readlane(__double2hiint(v), lane);
  return __hiloint2double(hi, lo);
}
__device__ __forceinline__ unsigned long long lane_bcast(unsigned long long v, int lane) {
  const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)v, lane), hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(v >> 32), lane);
  return ((unsigned long long)hi << 32) | lo;
}

// orders the LDS traffic of one wave's lanes: what a lane wrote before is readable by the other lanes behind it (lgkmcnt(0) between two wave barriers)
__device__ __forceinline__ void wave_lds_sync() { __builtin_amdgcn_wave_barrier(); __builtin_amdgcn_s_waitcnt(0xc07f); __builtin_amdgcn_wave_barrier(); }

// a T from any byte address (one load instruction where the hardware takes unaligned addresses, as global memory does)
template <class T>
__device__ __forceinline__ T ld_unaligned(const uint8_t *p) { T v; __builtin_memcpy(&v, p, sizeof(T)); return v; }

// index i of an axis of n samples under cv::BORDER_REFLECT_101
__device__ __forceinline__ int reflect101(int i, int n) {
  if (n == 1) return 0;
  while (i < 0 || i >= n) { i = i < 0 ? -i : 2 * n - 2 - i; }
  return i;
}

// the mixer of every counter-based draw (point seeding, loop closure, vocabulary training); each seeding scheme is pinned to its CPU model in tests/
__host__ __device__ __forceinline__ uint64_t splitmix64(uint64_t z) {
  z += 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
