// devutil.h -- the leaf helpers of the gfx950 kernels (wave64): index arithmetic, wave primitives, unaligned loads, the counter-based mixer.  One definition each;
// common.h includes this header, so every translation unit has them.
#pragma once
#include <stdint.h>
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define SVS_HD __host__ __device__ __forceinline__
#else
#include <math.h>
#define SVS_HD static inline      // the exact quotients below also compile for the host alone (tests/cpp/quotient_host.cpp holds them to a / b)
#endif

// ---- exact quotients that share a denominator -------------------------------------------------------------------------------------------------------
// x / z and y / z share their denominator, and the Jacobian needs 1 / z again: one refined reciprocal serves all three.
// r = RN(1 / b) after two Newton steps on v_rcp_f64 (what the compiler's own division expansion does per quotient), then
// q = a r, e = a - q b (exact in an FMA), q + e r is the correctly rounded a / b by Markstein's theorem whenever r is the
// correctly rounded reciprocal -- 3 f64 instructions per quotient instead of 11.  The tracker's pass is f64-issue bound
// (~200 VALU instructions per sample, profiles/r1_notes.md), so this is ~10 % of its time.  Non-finite / zero b give
// NaN or inf exactly where the IEEE quotient would be inf or NaN: the tracker's samples fail the |uv| < 1e9 gate either way.
// (the seed: v_rcp_f64 on the device, 2^29 ulp; the host takes 1 / b cut to 24 significant bits -- what follows must not depend on which)
SVS_HD double rcp_seed(double b) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __builtin_amdgcn_rcp(b);
#else
  double r = 1.0 / b;
  uint64_t u;
  __builtin_memcpy(&u, &r, 8);
  u &= ~((1ull << 29) - 1ull);
  __builtin_memcpy(&r, &u, 8);
  return r;
#endif
}
SVS_HD double rcp_rn(double b) {
  double r = rcp_seed(b);
  double e = __builtin_fma(-b, r, 1.0);
  r = __builtin_fma(e, r, r);
  e = __builtin_fma(-b, r, 1.0);
  return __builtin_fma(e, r, r);
}
SVS_HD double div_rn(double a, double b, double r) {
  const double q = a * r;
  return __builtin_fma(__builtin_fma(-q, b, a), r, q);
}
// The guarded forms: a / b bit for bit for EVERY pair of doubles, for the callers whose results are held to the plain division (motion.hip's clouds, gate.h).
// Markstein's theorem wants (1) r = RN(1 / b) and (2) no overflow, underflow or subnormal in r, q, e and the result.
// (2) the exponent window: |a| and |b| in [2^-500, 2^501).  Then r and q = a r lie in (2^-1002, 2^1002) -- normal, with room for the one ulp q may be off --
//     and e = a - q b, a multiple of ulp(q) ulp(b) >= 2^(-500 - 105) of magnitude <= ulp(q) |b|, is a normal double or zero: the inner FMA is exact.  Zero, subnormal,
//     infinite and NaN operands have the exponent fields 0 / 2047 and are outside (a = -0 would lose its sign in q + e r).  One integer range test on the high word each.
// (1) two Newton steps do not reach RN(1 / b) for every b: r (1 + e) is rounded from a value that lies below 1 / b by up to e1^2 ~ 2^-92 relative, so a b whose reciprocal
//     lies that close above a rounding midpoint gets the neighbour below -- b = 2 - 2^-52 (mantissa of all ones: 1 / b = 1/2 + 2^-54 + 2^-107) is the known one.
//     rcp_rn_checked tests what the theorem needs instead of assuming it: e' = 1 - b r is exact in an FMA, and r = RN(1 / b) <=> |1 / b - r| <= ulp(r) / 2 <=>
//     |e'| m <= (1 - e') 2^-53 with m = |r| / 2^exponent(r) in [1, 2).  The test asks for |e'| m < 2^-53 (1 - 2^-20): the margin covers 1 - e' (|e'| <= 2^-52) and the
//     rounding of the product, and sends a b within 2^-20 ulp of a midpoint (one in a million) to the plain division.  (Below a power of two the doubles lie twice as
//     close, so there half of ulp(r) would be too wide a bound -- but a reciprocal just below 2^k belongs to b = 2^-k (1 + j 2^-52), j >= 1, and lies a whole ulp(r) away.)
SVS_HD uint32_t quot_exp_field(double x) {      // the exponent field, in place (bits 20..30 of the high word)
  uint64_t u;
  __builtin_memcpy(&u, &x, 8);
  return (uint32_t)(u >> 32) & 0x7ff00000u;
}
SVS_HD bool quot_exp_field_ok(uint32_t f) { return f - ((1023u - 500u) << 20) <= (1000u << 20); }
SVS_HD bool quot_exp_ok(double x) { return quot_exp_field_ok(quot_exp_field(x)); }
SVS_HD double rcp_rn_checked(double b, bool &ok) {      // ok: the returned r is RN(1 / b) and b is inside the window (otherwise r is not to be used)
  const double r = rcp_rn(b);
  const double e = __builtin_fma(-b, r, 1.0);
#if defined(__HIP_DEVICE_COMPILE__)
  const double m = __builtin_amdgcn_frexp_mant(r);        // |m| in [0.5, 1)
#else
  int ex;
  const double m = frexp(r, &ex);
#endif
  ok = quot_exp_ok(b) & (fabs(e * m) < 0x1p-54 * (1.0 - 0x1p-20));      // (&: no branch; a NaN product compares false)
  return r;
}
SVS_HD double div_rn_guarded(double a, double b, double r, bool r_ok) {
  if (__builtin_expect(r_ok & quot_exp_ok(a), 1)) return div_rn(a, b, r);
  return a / b;
}
// q[k] = a[k] / b, N quotients by one denominator behind ONE test (a wave leaves the short path only where a lane holds an operand outside the window): the window
// is tested on the smallest and the largest of the numerators' exponent fields
template <int N>
SVS_HD void div_rn_guarded(const double (&a)[N], double b, double (&q)[N]) {
  bool ok;
  const double r = rcp_rn_checked(b, ok);
  uint32_t lo = quot_exp_field(a[0]), hi = lo;
  for (int k = 1; k < N; ++k) { const uint32_t f = quot_exp_field(a[k]); lo = f < lo ? f : lo; hi = f > hi ? f : hi; }
  ok = ok & quot_exp_field_ok(lo) & quot_exp_field_ok(hi);
  if (__builtin_expect(ok, 1)) {
    for (int k = 0; k < N; ++k) q[k] = div_rn(a[k], b, r);
  } else {
    for (int k = 0; k < N; ++k) q[k] = a[k] / b;
  }
}

#if defined(__HIPCC__)
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
// wave64 inclusive prefix sum: lane l returns v of lanes 0 .. l
__device__ __forceinline__ int wave_incl_scan(int v) {
  const int lane = lane_id();
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) { const int t = __shfl_up(v, o, 64); if (lane >= o) v += t; }
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

// A pointer with its address space spelled out: SVS_AS1 global memory, SVS_AS3 the LDS.  A pointer that has been through memory, the LDS or an asm statement is a
// flat pointer to the compiler -- every access a flat_load that also probes the LDS aperture and counts on BOTH wait counters, so that a wait for the LDS waits for the
// memory requests in flight as well.  With the address space in the type the access is a global_load (vmcnt alone) or a ds_read (lgkmcnt alone) whatever the pointer
// has been through.
#define SVS_AS1 __attribute__((address_space(1)))
#define SVS_AS3 __attribute__((address_space(3)))
template <class T>
__device__ __forceinline__ T ld_unaligned(const SVS_AS1 uint8_t *p) {
  typedef T unaligned_t __attribute__((aligned(1)));
  return *(const SVS_AS1 unaligned_t *)p;
}

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
#endif      // __HIPCC__
