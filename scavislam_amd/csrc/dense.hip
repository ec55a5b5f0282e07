// dense.hip -- dense (direct) SE3 tracking for gfx950.
// Replaces DenseTracker::denseTrackingCpu (dense_tracking.cpp:222-391; the parity target, SURVEY.md section 0
// last row).  The CUDA build's full-resolution tracker (GpuTracker, denseTrackingGpu) lives in dense_full.hip,
// computeDensePointCloudCpu (the clouds this tracker reads) in motion.hip, the 6x6 LM step in lm6.h.
//
// MI355X-first design:
//  * per-sample work is a gather (cloud, 4-tap bilinear of cur/dx/dy) + 27 accumulators; the
//    reduction is wave64 shuffles -> LDS across waves -> one partial per workgroup, summed by a
//    fixed-order finalize kernel (deterministic, no float atomics, no host-side summation of
//    block partials as in the reference's .cu:343-355);
//  * svs_dense_track_cpu_sem keeps the WHOLE coarse-to-fine LM loop on the device: one 1024-lane
//    workgroup per camera stream iterates chi2 / H,b / 6x6 solve / SE3 exp / accept-reject with
//    LDS broadcasts, so a frame costs one launch instead of ~90 launch+sync+D2H round trips.
#include "common.h"
#include "lm6.h"
#include "pose.h"
#include "seqsum.h"
#include <algorithm>
#include <climits>

namespace {

constexpr int NSUM = 28;   // 21 H + 6 b + chi2 ; n_valid kept separately

struct Acc {
  double v[NSUM];
  int n;      // samples that contributed (a lane sees a few dozen per sweep; block_reduce widens it)
  __device__ __forceinline__ void zero() {
#pragma unroll
    for (int i = 0; i < NSUM; ++i) v[i] = 0;
    n = 0;
  }
};

// (P: `const float *`, or the same pointer with its address space spelled out -- see LevelArgsG)
template <class P>
__device__ __forceinline__ float interp32f(P m, int stride, float u, float v) {
  float x = floorf(u), y = floorf(v);
  float sx = u - x, sy = v - y;
  float wx0 = 1 - sx, wx1 = sx, wy0 = 1 - sy, wy1 = sy;
  int xi = (int)x, yi = (int)y;
  const P p = m + (unsigned)(yi * stride + xi);      // (in-frame samples: non-negative, below 2^31)
  float v00 = p[0], v10 = p[1], v01 = p[stride], v11 = p[stride + 1];
  return (wx0 * wy0) * v00 + (wx0 * wy1) * v01 + (wx1 * wy0) * v10 + (wx1 * wy1) * v11;
}

struct LevelArgs {
  const float *cloud; const uint8_t *prev; const float *cur, *dx, *dy;
  int pstride, fstride;
  svs_cam cam;
  const uint8_t *cur8;   // optional: current u8 level image; f32 image and Sobel taps are then formed on the fly
  int c8stride;
};

// The same with the address space of every pointer spelled out (global memory).  The flat tracker kernel's sweep takes its operands out of LDS
// (track_pass_from_lds), and a pointer that has been through memory is a flat pointer to the compiler -- every access a flat_load that also probes the LDS
// aperture and counts on both wait counters (SVS_AS1: devutil.h).
typedef float svs_f4 __attribute__((ext_vector_type(4)));
struct LevelArgsG {
  const SVS_AS1 float *cloud; const SVS_AS1 uint8_t *prev; const SVS_AS1 float *cur, *dx, *dy;
  int pstride, fstride;
  svs_cam cam;
  const SVS_AS1 uint8_t *cur8;
  int c8stride;
};
__device__ __forceinline__ float4 load_f4(const float *p) { return *reinterpret_cast<const float4 *>(p); }
__device__ __forceinline__ float4 load_f4(const SVS_AS1 float *p) { const svs_f4 v = *(const SVS_AS1 svs_f4 *)p; return make_float4(v.x, v.y, v.z, v.w); }
__device__ __forceinline__ uint32_t load_u32_unaligned(const uint8_t *p) { return ld_unaligned<uint32_t>(p); }      // (the pair exists for taps_u8_issue, which takes either pointer)
__device__ __forceinline__ uint32_t load_u32_unaligned(const SVS_AS1 uint8_t *p) {
  typedef uint32_t u32_unaligned __attribute__((aligned(1)));
  return *(const SVS_AS1 u32_unaligned *)p;
}

// Bilinear taps of I, dx, dy straight from the u8 level image.  (float)u8 * float(1/255.) and the
// centred differences are exactly the values frame_grabber.cpp:315-333 would have materialised, so
// the results are bit-identical to reading the f32 pyramids -- at 1/8 of the HBM traffic (the f32
// path touches ~half of three 4 B/px images per pass for a 1/16 sampling grid).  In-frame samples
// (border 2) never need the REFLECT_101 border rule.
// The four rows of a sample's 4 x 4 neighbourhood, one dword each, in two steps: taps_u8_issue puts the four requests in flight, taps_u8_wait makes them usable.
// What the caller places between the two runs under ONE memory round trip.  TapRows::w must not be touched in between (tools/tracker_loop_isa.py checks the ISA).
struct TapRows { uint32_t w[4]; };
constexpr bool TRK_TAPS_ASM = true;
// ASM: the loads as one inline-asm statement and the wait as a second one that names all four destinations (the form seq_load_run uses for its ten loads).  Left to
// the compiler, the flat tracker kernel at its 128-register limit waited for row 0 -- and with it for the store and the prefetch in front of it -- before it issued
// rows 1..3 into row 0's register: two dependent round trips per sample (profiles/tracker_taps.md).  The base comes from scalar registers (the stream's image, and
// the same moved down by one, two and three rows), the one vector operand is the 32-bit offset of row 0: no destination can alias an address still to be read.
template <bool ASM, class P>
__device__ __forceinline__ void taps_u8_issue(P img, int stride, float u, float v, TapRows &t) {
  const int xi = (int)floorf(u), yi = (int)floorf(v);
  // 32-bit offsets from the stream's (scalar) image pointer: the tap loads take the base from scalar registers and the sweep spends no 64-bit multiply-adds
  // (quarter rate) on addresses.  In-frame samples (border 2) keep yi - 1 >= 1 and xi - 1 >= 1: the offsets are non-negative and far below 2^31; rows and
  // strides are below 2^24 (offsets_fit_24: the host refuses anything else), so the product is a 24-bit multiply (full rate; v_mul_lo_u32 is quarter rate)
  const unsigned o0 = __umul24(yi - 1, stride) + (unsigned)(xi - 1);
  __builtin_amdgcn_sched_barrier(0);
  if constexpr (ASM) {
    // (image and stride are the stream's: the same in every lane.  Where the compiler cannot see that -- the level came through memory -- they are read from lane 0)
    const unsigned long long bv = (unsigned long long)img;
    const unsigned long long b0 = ((unsigned long long)(unsigned)__builtin_amdgcn_readfirstlane((int)(bv >> 32)) << 32) | (unsigned)__builtin_amdgcn_readfirstlane((int)bv);
    const unsigned long long rs = (unsigned long long)(unsigned)__builtin_amdgcn_readfirstlane(stride);
    asm("global_load_dword %0, %4, %5\n\t"
        "global_load_dword %1, %4, %6\n\t"
        "global_load_dword %2, %4, %7\n\t"
        "global_load_dword %3, %4, %8"
        : "=&v"(t.w[0]), "=&v"(t.w[1]), "=&v"(t.w[2]), "=&v"(t.w[3])
        : "v"(o0), "s"(b0), "s"(b0 + rs), "s"(b0 + 2 * rs), "s"(b0 + 3 * rs));
    // (neither volatile nor a "memory" clobber: nothing writes the image while the tracker runs, the wait below is tied to the loads through their registers, and the
    // scheduling fences keep both where they are written)
  } else {
#pragma unroll
    for (int r = 0; r < 4; ++r) t.w[r] = load_u32_unaligned(img + (o0 + (unsigned)(r * stride)));
  }
  __builtin_amdgcn_sched_barrier(0);
}
template <bool ASM>
__device__ __forceinline__ void taps_u8_wait(TapRows &t) {
  __builtin_amdgcn_sched_barrier(0);
  if constexpr (ASM) {
    // (the four are the youngest requests of the lane, so the count that covers them is zero.  The compiler does not count them: a wait of its own in between
    // would be for something older and only wait longer -- the caller puts nothing there that reads memory)
    // The wait is the BUILTIN, not a line of inline asm: the compiler's wait-count bookkeeping sees a builtin and knows that every request of its own -- the sweep's
    // deferred term store and the prefetch of the next sample -- is complete behind it.  With the wait hidden in asm it carried the prefetched previous-frame byte
    // of the peeled first trip as "still in flight" into the sample loop and waited vmcnt(1) for it in front of every trip's taps: behind the trip's own store and
    // prefetch loads that made two of them complete before the taps were issued -- two memory round trips per sample, one after the other (profiles/tracker_prefetch.md;
    // tools/tracker_loop_isa.py checks the ISA).  The empty asm statement keeps the four registers defined HERE, not at the loads.
    __builtin_amdgcn_s_waitcnt(0x0f70);      // vmcnt(0) (bits 3:0 and 15:14), expcnt and lgkmcnt left open
    asm volatile("" : "+v"(t.w[0]), "+v"(t.w[1]), "+v"(t.w[2]), "+v"(t.w[3]));
    __builtin_amdgcn_sched_barrier(0);
  }
}
__device__ __forceinline__ void taps_u8_finish(const TapRows &t, float u, float v, float &ic, float &gx, float &gy) {
  const float sc = (float)(1. / 255.);
  const float x = floorf(u), y = floorf(v);
  const float sx = u - x, sy = v - y;
  const float wx0 = 1 - sx, wx1 = sx, wy0 = 1 - sy, wy1 = sy;
  float f[4][4];
#pragma unroll
  for (int r = 0; r < 4; ++r)
#pragma unroll
    for (int c = 0; c < 4; ++c) f[r][c] = (float)((t.w[r] >> (8 * c)) & 0xff) * sc;
  const float w00 = wx0 * wy0, w01 = wx0 * wy1, w10 = wx1 * wy0, w11 = wx1 * wy1;   // v00=(x,y) v01=(x,y+1) v10=(x+1,y) v11
  ic = w00 * f[1][1] + w01 * f[2][1] + w10 * f[1][2] + w11 * f[2][2];
  gx = w00 * (f[1][2] - f[1][0]) + w01 * (f[2][2] - f[2][0]) + w10 * (f[1][3] - f[1][1]) + w11 * (f[2][3] - f[2][1]);
  gy = w00 * (f[2][1] - f[0][1]) + w01 * (f[3][1] - f[1][1]) + w10 * (f[2][2] - f[0][2]) + w11 * (f[3][2] - f[1][2]);
}
template <class P>
__device__ __forceinline__ void taps_u8(P img, int stride, float u, float v, float &ic, float &gx, float &gy) {
  TapRows t;
  taps_u8_issue<false>(img, stride, u, v, t);
  taps_u8_finish(t, u, v, ic, gx, gy);
}

// loop body of dense_tracking.cpp:229-261 (chi2) / :278-331 (H, b), one sample.
// Every load is unconditional (an invalid sample taps a safe address) so that the caller can keep the cloud
// load and the bilinear taps of several samples in flight: the pass is bound by gather latency, not by bytes.
// What an invalid sample would add to the sums is skipped under one `if (ok)` behind the taps.
// the two T-independent loads of a sample (stored 3D point, previous-frame intensity): issued one trip ahead by track_pass
struct SampleIn { float4 c4; uint8_t prev; };
// A grid position past the level's end (the prefetch of a lane's last trip) reads the level's FIRST sample instead: an address that is always there, and no
// constants to materialise per trip.  What comes back is then some other sample's data, c4.w included -- whoever may consume such a sample masks it with its own
// in_range (sample_cpu_sem starts `ok` from it: the TM == 0 sweep); the TM != 0 sweeps run a trip only for i < n and never consume one.
template <class LA>
__device__ __forceinline__ SampleIn sample_load(const LA &L, int u, int v, int cw, bool in_range) {
  SampleIn s;
  const int us = in_range ? u : 0, vs = in_range ? v : 0;
  s.c4 = load_f4(L.cloud + 4u * (__umul24(vs, cw) + (unsigned)us));
  s.prev = L.prev[__umul24(vs * 4, L.pstride) + (unsigned)(us * 4)];
  return s;
}
// (rcp_rn / div_rn, one refined reciprocal for x / z, y / z and the Jacobian: devutil.h)

// TM (term mode): what happens to the sample's float term res * res of the reference's `chi2 += res * res` -- 0: nothing; 1: stored at t_out (if not null);
// 2: stored past the caches (sibling workgroups of the stream will read it: MULTI)
template <bool JAC, bool U8SRC = false, int TM = 0, class LA = LevelArgs>
__device__ __forceinline__ void sample_cpu_sem(const LA &L, const double *T, const SampleIn &in, bool in_range, Acc &a,
                                               const float *ip_lut = nullptr, float *term_out = nullptr) {      // term_out (TM != 0): where the caller wants the sample's term
  const float4 c4 = in.c4;
  bool ok = in_range && (c4.w > 0);
  const double xp0 = c4.x, xp1 = c4.y, xp2 = c4.z;
  double x, y, z;
  pose_act(T, xp0, xp1, xp2, x, y, z);
  const double rz = rcp_rn(z);
  float uvx = (float)(L.cam.f * div_rn(x, z, rz) + L.cam.cx);
  float uvy = (float)(L.cam.f * div_rn(y, z, rz) + L.cam.cy);
  ok = ok && (fabsf(uvx) < 1e9f && fabsf(uvy) < 1e9f);
  const int ui = ok ? (int)uvx : 0, vi = ok ? (int)uvy : 0;
  ok = ok && (ui >= 2 && vi >= 2 && ui < L.cam.w - 2 && vi < L.cam.h - 2);
  if (!ok) { uvx = 2.f; uvy = 2.f; }                       // safe tap position, contribution masked below
  // (float)((1./255.) * u8): a double product rounded once (dense_tracking.cpp:290-293), NOT the f32 product convertTo
  // uses for the current image -- the tracker kernel keeps the 256 possible values in LDS (3 f64-rate instructions less)
  // u8 source: the four row loads go out here, all of them before anything waits; what follows down to taps_u8_wait needs none of them and runs under their
  // round trip -- the look-up of ip and the part of the Jacobian that depends on the pose alone (~25 f64 instructions)
  const float ip = ip_lut ? ip_lut[in.prev] : (float)((1. / 255.) * in.prev);
  TapRows taps;
  if constexpr (U8SRC) taps_u8_issue<TRK_TAPS_ASM>(L.cur8, L.c8stride, uvx, uvy, taps);
  // (x, y, rz as they are, valid sample or not: what an invalid lane forms from them below is garbage that nothing reads -- see `if (ok)`)
  const double xs = x, ys = y;
  // transformations.h:117-139 frame_jac_xyz2uv.  One reciprocal instead of eight f64 divisions and
  // fused multiply-adds in the 27 accumulations: the pass is f64-issue bound on its CU, and H/b only
  // need 1e-9 relative agreement with the serial oracle (uv above stays division-exact because the
  // in-frame test and the tap addresses must match bit for bit).
  // (every fused multiply-add written out: left to the compiler's contraction the two instantiations of this function -- f32 pyramids / u8 source -- fused
  // different pairs, and their sums, which the tests hold bit-identical, drifted apart with every unrelated change to the kernel)
  double f = L.cam.f, iz = rz, iz2 = iz * iz, fx = f * iz, xz = xs * iz2 * f, yz = ys * iz2 * f;
  // (only the accumulation under `if (ok)` reads these three, and the optimiser would sink them in there, behind the wait: the empty statement keeps them here,
  // under the taps' round trip)
  if constexpr (U8SRC && JAC) asm volatile("" : "+v"(fx), "+v"(xz), "+v"(yz));
  float ic, g8x = 0.f, g8y = 0.f;     // (the bilinear dx, dy of either source; the loads of the f32 pyramids unconditional like the u8 taps)
  if constexpr (U8SRC) { taps_u8_wait<TRK_TAPS_ASM>(taps); taps_u8_finish(taps, uvx, uvy, ic, g8x, g8y); }
  else {
    ic = interp32f(L.cur, L.fstride, uvx, uvy);
    if (JAC) { g8x = interp32f(L.dx, L.fstride, uvx, uvy); g8y = interp32f(L.dy, L.fstride, uvx, uvy); }
  }
  float res = ip - ic;
  // dense_tracking.cpp:299-300 `if (res > 0.1) res = 0.1; if (res < -0.1) res = -0.1;` on a float res: the comparisons are made in double against the double 0.1,
  // which lies between 0.1f and the float below it, so `res > 0.1` is `res >= 0.1f` and the assignment stores 0.1f -- min / max with +-0.1f, bit for bit
  // (res is never NaN: both images are finite), two instructions instead of two conversions and two f64 compares
  res = fminf(fmaxf(res, -0.1f), 0.1f);
  // the term of the reference's `float chi2 += res*res` (0 where the reference skips the sample: x + 0 is exact)
  if constexpr (TM != 0) *term_out = ok ? res * res : 0.f;
  a.n += ok ? 1 : 0;
  // An invalid sample is SKIPPED, not added as zeros (one exec mask instead of a select per operand).  The sums keep their bits: the masked form added
  // fma(+-0, +-0, acc) to H and b and acc + 0.0 to chi2, which leaves every acc but -0 as it is, and no accumulator is ever -0 -- each starts at +0, x + y
  // of opposite signs that cancel exactly rounds to +0, and a product small enough to round to -0 would need |J| < 1e-150 (J is a half u8 gradient, >= 1e-17
  // where it is not 0, times a camera-geometry factor).  (The tap loads above stay unconditional, at the safe position.)
  if (ok) {
    a.v[27] += (double)(res * res);
    if (JAC) {
      const double r0[6] = {-fx, 0, xz, xz * ys, -__builtin_fma(xz, xs, f), ys * fx};
      const double r1[6] = {0, -fx, yz, __builtin_fma(yz, ys, f), -(yz * xs), -(xs * fx)};
      const float gx = (float)(0.5 * g8x);
      const float gy = (float)(0.5 * g8y);
      double J[6];
      J[0] = gx * r0[0];
      J[1] = gy * r1[1];
#pragma unroll
      for (int k = 2; k < 6; ++k) J[k] = __builtin_fma(gx, r0[k], gy * r1[k]);
      int k = 0;
#pragma unroll
      for (int c = 0; c < 6; ++c)
#pragma unroll
        for (int r = 0; r <= c; ++r) { a.v[k] = __builtin_fma(J[r], J[c], a.v[k]); ++k; }
#pragma unroll
      for (int i = 0; i < 6; ++i) a.v[21 + i] = __builtin_fma(J[i], (double)res, a.v[21 + i]);
    }
  }
}

// block reduction; result valid in threads [0, NSUM] (index = value id).  Inside a wave the 29 sums are reduced by
// recursive halving: in step s a lane keeps one half of its partial vector and hands the other half to its partner
// (lane ^ 2^s), so 16+8+4+2+1(+1) = 32 f64 exchanges replace 29 x 6 butterflies -- the pass is short, this tail is not.
template <int NWAVES>
__device__ __forceinline__ void block_reduce(Acc &a, double (*s_part)[NSUM + 1], double *out_vals /* NSUM+1 in LDS */) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  double x[32];
#pragma unroll
  for (int i = 0; i < NSUM; ++i) x[i] = a.v[i];
  x[NSUM] = (double)a.n;
#pragma unroll
  for (int i = NSUM + 1; i < 32; ++i) x[i] = 0.0;
#pragma unroll
  for (int step = 0; step < 5; ++step) {
    const int half = 16 >> step, bit = 1 << step;
    const bool up = (lane & bit) != 0;
#pragma unroll
    for (int k = 0; k < half; ++k) {
      const double send = up ? x[k] : x[k + half];
      const double keep = up ? x[k + half] : x[k];
      x[k] = keep + __shfl_xor(send, bit, 64);
    }
  }
  x[0] += __shfl_xor(x[0], 32, 64);
  // lanes 0..31 now hold the wave sum of value id = bit-reversed lane index (5 bits)
  const int idx = ((lane & 1) << 4) | ((lane & 2) << 2) | (lane & 4) | ((lane & 8) >> 2) | ((lane & 16) >> 4);
  if (lane < 32 && idx <= NSUM) s_part[wave][idx] = x[0];
  __syncthreads();
  if (threadIdx.x <= NSUM) {
    double s = 0;
    for (int w = 0; w < NWAVES; ++w) s += s_part[w][threadIdx.x];
    out_vals[threadIdx.x] = s;
  }
  __syncthreads();
}

// ---- multi-workgroup single pass (GpuTracker-style API) --------------------------------------
template <bool JAC>
__global__ __launch_bounds__(256) void dense_pass_cpu_sem_kernel(LevelArgs L, size_t cloud_b, size_t prev_b, size_t f_b,
                                                                 const double *__restrict__ Tarr, double *__restrict__ partials) {
  __shared__ double s_part[4][NSUM + 1];
  __shared__ double s_out[NSUM + 1];
  const int slot = blockIdx.y;
  L.cloud += slot * cloud_b; L.prev += slot * prev_b; L.cur += slot * f_b; L.dx += slot * f_b; L.dy += slot * f_b;
  double T[12];
#pragma unroll
  for (int i = 0; i < 12; ++i) T[i] = Tarr[(size_t)slot * 12 + i];
  const int cw = L.cam.w / 4, ch = L.cam.h / 4, n = cw * ch;
  Acc a;
  a.zero();
  for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) sample_cpu_sem<JAC>(L, T, sample_load(L, i % cw, i / cw, cw, true), true, a);
  block_reduce<4>(a, s_part, s_out);
  if (threadIdx.x <= NSUM) partials[((size_t)slot * gridDim.x + blockIdx.x) * (NSUM + 1) + threadIdx.x] = s_out[threadIdx.x];
}

__global__ void dense_finalize_kernel(const double *__restrict__ partials, int nblocks, svs_dense_sums *__restrict__ out) {
  const int slot = blockIdx.x, t = threadIdx.x;
  if (t > NSUM) return;
  double s = 0;
  for (int b = 0; b < nblocks; ++b) s += partials[((size_t)slot * nblocks + b) * (NSUM + 1) + t];
  svs_dense_sums *o = &out[slot];
  if (t < 21) o->H[t] = s;
  else if (t < 27) o->b[t - 21] = s;
  else if (t == 27) o->chi2 = (double)(float)s;     // reference keeps chi2 in a float
  else o->n_valid = (long long)s;
}

// ---- device-resident LM (whole denseTrackingCpu) ---------------------------------------------
struct TrackArgs {
  LevelArgs lv[3];
  size_t cloud_b[3], prev_b[3], f_b[3], c8_b[3];
  double *T_jac;     // optional [batch][3][12]: pose of the last H,b pass of each level (what residual_img[level] shows)
  svs_dense_lm_record *rec; int rec_cap; int32_t *n_rec;      // optional accept / reject record of the loop
};

// tuning constants, as measured (profiles/r3_notes.md, r5_notes.md)
constexpr int TRK_THREADS = 512;      // lanes per workgroup
constexpr int TRK_UNROLL = 1;         // samples per lane and trip of the sweep (2: the 128-register build spills 126 registers)
constexpr bool TRK_T_SCALAR = true;   // the pose of a sweep in scalar registers instead of 24 vector registers

template <bool JAC, bool U8SRC, int TM = 0, class LA = LevelArgs>
__device__ __forceinline__ void track_pass(const LA &L_in, const double *T_in, double (*s_part)[NSUM + 1], double *s_out, const float *ip_lut,
                                           int first, int nwg, float *t_buf = nullptr) {      // first = wg * TRK_THREADS + tid; nwg workgroups share the sweep; t_buf: the pass's terms (TM), or null
  // a copy of the sweep's own: where the caller's level lives in memory (the latency-mode kernel hands it to a lambda by reference) the scheduling fences around the
  // tap loads would make every trip read it again
  const LA L = L_in;
  const int cw = L.cam.w / 4, ch = L.cam.h / 4, n = cw * ch;
  // the pose of a sweep is the same in every lane: kept in scalar registers (24 vector registers less over the whole sweep -- the kernel is built for 128)
  double T[12];
#pragma unroll
  for (int i = 0; i < 12; ++i)
    T[i] = TRK_T_SCALAR ? __hiloint2double(__builtin_amdgcn_readfirstlane(__double2hiint(T_in[i])), __builtin_amdgcn_readfirstlane(__double2loint(T_in[i]))) : T_in[i];
  Acc a;
  a.zero();
  // TRK_UNROLL samples per lane per trip (independent gather chains in flight); the next trip's stored points and
  // previous-frame intensities (independent of T) are loaded before this trip's arithmetic, so only the bilinear
  // taps -- whose addresses depend on the projection -- are exposed.  The grid position of the prefetched sample is
  // carried incrementally (one division per pass instead of one per sample: the pass is VALU-issue bound).
  const int STEP = TRK_UNROLL * TRK_THREADS * nwg;
  const int su = STEP % cw, sv = STEP / cw;
  SampleIn nxt[TRK_UNROLL];
  int pu[TRK_UNROLL], pv[TRK_UNROLL];
#pragma unroll
  for (int q = 0; q < TRK_UNROLL; ++q) {
    const int j = first + q * TRK_THREADS * nwg;
    pu[q] = j % cw; pv[q] = j / cw;
    const bool in = pv[q] < ch;
    nxt[q] = sample_load(L, in ? pu[q] : 0, in ? pv[q] : 0, cw, in);
  }
  // TM: the term of a sample is stored one trip LATE, in front of the next trip's loads.  vmcnt counts loads and stores in one queue: a store issued at the end of a
  // trip would be the youngest entry when the next trip waits for its prefetched operands at the top of the loop -- a full write round trip exposed per trip
  // (measured: + 18 % on the sweep); issued here it retires under the projection arithmetic and the tap loads that follow.
  // (the buffer's address space spelled out: the pointer comes out of a two-entry array indexed by the LM loop, and a flat store would tie the loop's LDS waits to memory)
  // Its address is the buffer (uniform: a scalar base, moved back by one trip) plus a 32-bit byte offset formed from the sample index the loop carries anyway --
  // no 64-bit pointer per lane to keep and advance (terms of a pass: far below 2^30)
  typedef __attribute__((address_space(1))) float *gptr_t;
  typedef __attribute__((address_space(1))) char *gptr_c;
  static_assert(TM == 0 || TRK_UNROLL == 1, "the deferred term store keeps one term per lane");
  float pend_t = 0.f;
  const gptr_c pend_base = (gptr_c)(gptr_t)t_buf - 4 * (long)STEP;
  bool pend = false;
  int i = first;
  auto flush = [&]() {      // the term of sample i - STEP
    const gptr_t pend_p = (gptr_t)(pend_base + 4u * (unsigned)i);
    if constexpr (TM == 1) { if (pend) *pend_p = pend_t; }
    if constexpr (TM == 2) { if (pend) __hip_atomic_store(pend_p, pend_t, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
  };
  // one trip: the term store of the trip before, the prefetch of the next sample into `nxt`, the sample in `cur`
  auto trip = [&](const SampleIn (&cur)[TRK_UNROLL], SampleIn (&nxt)[TRK_UNROLL]) {
    if constexpr (TM != 0) { flush(); pend = t_buf != nullptr; }
#pragma unroll
    for (int q = 0; q < TRK_UNROLL; ++q) {
      pu[q] += su; pv[q] += sv;
      if (pu[q] >= cw) { pu[q] -= cw; ++pv[q]; }
      const bool in = pv[q] < ch;
      nxt[q] = sample_load(L, in ? pu[q] : 0, in ? pv[q] : 0, cw, in);
    }
#pragma unroll
    for (int q = 0; q < TRK_UNROLL; ++q) {
      if constexpr (TM != 0) sample_cpu_sem<JAC, U8SRC, TM, LA>(L, T, cur[q], true, a, ip_lut, &pend_t);      // (i < n: in range)
      else sample_cpu_sem<JAC, U8SRC, 0, LA>(L, T, cur[q], i + q * TRK_THREADS * nwg < n, a, ip_lut);
    }
    i += STEP;
  };
  // Two trips per iteration on two register sets -- `nxt` consumed while `alt` is in flight, then the reverse --, so that no trip copies its prefetched sample
  // into a "current" one (five moves per sample); one more trip behind the loop for a lane with an odd count.  Same samples, same order, in every lane.
  SampleIn alt[TRK_UNROLL];
  // (the first sample's own operands, which its projection needs at once, waited for HERE, in the builtin form the compiler's bookkeeping reads: entered with
  // them "in flight" the loop would wait for them behind the trip's store and prefetch -- vmcnt(2) in every trip, which completes the trip's own store in front of
  // its taps; see taps_u8_wait)
  if constexpr (U8SRC) __builtin_amdgcn_s_waitcnt(0x0f70);
  while (i + STEP < n) { trip(nxt, alt); trip(alt, nxt); }      // (both trips in range; i + STEP is far below 2^31)
  if (i < n) trip(nxt, alt);
  if constexpr (TM != 0) flush();
  block_reduce<TRK_THREADS / 64>(a, s_part, s_out);
}

// ---- the sweep with its operands in LDS --------------------------------------------------------------------------------------------------------------------
// The big-batch kernel (dense_track_batch_kernel) is built for 128 vector registers (two 512-lane workgroups per CU) and the sweep alone fills them: 28 f64
// accumulators, the sample in flight, the prefetched next one.  Whatever else is alive across the sweep shares that allocation and spills inside the loop over
// the samples.  So one lane leaves the sweep's operands in LDS (g_pa), and the sweep reads them back into scalar registers (they are uniform): nothing of the
// LM loop is live inside.  Results in g_s_out.
struct PassArgs { LevelArgs L; double T[12]; float *t_buf; int wg, nwg; };
__shared__ PassArgs g_pa;
__shared__ double g_s_part[TRK_THREADS / 64][NSUM + 1];
__shared__ double g_s_out[NSUM + 1];
__shared__ float g_iplut[256];
__device__ __forceinline__ int uni_i32(int v) { return __builtin_amdgcn_readfirstlane(v); }
__device__ __forceinline__ double uni_f64(double v) { return __hiloint2double(__builtin_amdgcn_readfirstlane(__double2hiint(v)), __builtin_amdgcn_readfirstlane(__double2loint(v))); }
template <class T>
__device__ __forceinline__ T *uni_ptr(T *p) {
  const unsigned long long u = (unsigned long long)p;
  const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)u), hi = __builtin_amdgcn_readfirstlane((unsigned)(u >> 32));
  return (T *)(((unsigned long long)hi << 32) | lo);
}
template <bool U8SRC, int TM>
__device__ __forceinline__ void track_pass_from_lds() {      // a sweep with its operands out of g_pa, into scalar registers
  LevelArgsG L;
  L.cloud = (const SVS_AS1 float *)uni_ptr(g_pa.L.cloud); L.prev = (const SVS_AS1 uint8_t *)uni_ptr(g_pa.L.prev);
  L.cur = (const SVS_AS1 float *)uni_ptr(g_pa.L.cur); L.dx = (const SVS_AS1 float *)uni_ptr(g_pa.L.dx); L.dy = (const SVS_AS1 float *)uni_ptr(g_pa.L.dy);
  L.cur8 = (const SVS_AS1 uint8_t *)uni_ptr(g_pa.L.cur8);
  L.pstride = uni_i32(g_pa.L.pstride); L.fstride = uni_i32(g_pa.L.fstride); L.c8stride = uni_i32(g_pa.L.c8stride);
  L.cam.f = uni_f64(g_pa.L.cam.f); L.cam.cx = uni_f64(g_pa.L.cam.cx); L.cam.cy = uni_f64(g_pa.L.cam.cy); L.cam.b = 0;
  L.cam.w = uni_i32(g_pa.L.cam.w); L.cam.h = uni_i32(g_pa.L.cam.h);
  const int nwg = uni_i32(g_pa.nwg), first = uni_i32(g_pa.wg) * TRK_THREADS + (int)threadIdx.x;
  track_pass<true, U8SRC, TM, LevelArgsG>(L, g_pa.T, g_s_part, g_s_out, g_iplut, first, nwg, uni_ptr(g_pa.t_buf));
}

// "trk_seq_chi2": the reference's `float chi2`, summed the way the reference sums it -- one f32 accumulator, samples in row-major order (dense_tracking.cpp:229-262,
// 341-367).  Near convergence chi2 - new_chi2 is below the rounding noise of these 19 200-term sums, so the accept test of the last LM steps of a level is decided by
// the summation order; with this option the loop takes exactly the reference's decisions (the default compares the f64 sums, narrowed).  Wave 0 walks the terms the
// pass left in t_buf: 64 loads at a time, then 64 dependent adds on values broadcast from the lanes in order.  Slow (~0.1 ms per sum) -- parity runs only.
// a pointer into GLOBAL memory, told to the compiler: exact_seq_sum_f32 is a real call (it must not take part in the register allocation of the tracker's sweeps), and
// behind a call boundary a plain `const float *` is a flat pointer -- every access a flat_load that also probes the LDS aperture
typedef const __attribute__((address_space(1))) float *svs_gptr_f32;
typedef const __attribute__((address_space(1))) svs_f4 *svs_gptr_f4;
template <bool COH, typename P>      // COH: the terms were stored past the caches by sibling workgroups (MULTI) and are read the same way
__device__ __forceinline__ float seq_term_load(P p) {
  if constexpr (COH) return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); else return *p;
}
template <bool COH = false, typename P = const float *>
__device__ __forceinline__ float seq_sum_f32(P t, int n) {
  float acc = 0.f;
  const int lane = threadIdx.x & 63;
  for (int base = 0; base < n; base += 64) {
    const float v = base + lane < n ? seq_term_load<COH, P>(t + base + lane) : 0.f;      // (written by this workgroup before a barrier: workgroup-scope visibility is enough)
#pragma unroll
    for (int l = 0; l < 64; ++l) acc = acc + __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), l));
  }
  return acc;
}
// every lane of the workgroup gets the sequential sum (wave 0 computes it between two barriers)
__device__ __forceinline__ float seq_chi2_f32(const float *t, int n) {
  __shared__ float s_seq;
  __syncthreads();
  if (threadIdx.x < 64) { const float v = seq_sum_f32(t, n); if (threadIdx.x == 0) s_seq = v; }
  __syncthreads();
  return s_seq;
}

// ---- the same bits without the chain (seqsum.h): the default accept test ------------------------------------------------------------------------------
// The tracker decides on its f64 sums wherever their difference is outside the rigorous error bound of the reference's float sums; inside the bound (most trials of
// level 0: the bound is 1.1e-3 of chi2 at 19 200 samples, the last LM steps of a level change chi2 by less) it needs the reference's float sums themselves.
// exact_seq_sum_f32 forms one from the terms a pass left in its buffer, all lanes of the workgroup at work: lane k owns the k-th run of S consecutive terms
// (f64 sum + count -> workgroup scan -> is my run certainly inside one binade? -> its integer map), a wave-level segmented scan composes the maps of neighbouring
// safe runs, and wave 0 walks the result: one table look-up per group of safe runs, a readlane chain over the ~10 runs that may straddle a power of two (staged in
// LDS by their lanes).  ~400 dependent float adds instead of 19 200.  Any failed check -> the plain chain over all terms (never seen; counted by the tests' hook).
constexpr int SEQ_Q = TRK_THREADS >= 512 ? 10 : 13;  // a lane's run of terms lives in SEQ_Q float4 registers: runs of up to 40 terms, i.e. up to 20 480 terms per sum (a 640 x 512 image)
constexpr int SEQ_RUN_MAX = 4 * SEQ_Q;
constexpr int SEQ_STAGE_FLOATS = 48 * SEQ_RUN_MAX;   // the runs the walker adds the slow way (typically ~10)
struct SeqShared {
  SvsSeqMap pref[TRK_THREADS];                       // composition of the safe runs from the start of my group (wave-local) through me
  unsigned char eb[TRK_THREADS];                     // biased exponent of my run's binade (0: not safe)
  short slot[TRK_THREADS];                           // my place in `stage` (unsafe runs), -1: none (the walker reads global memory)
  unsigned long long unsafe[TRK_THREADS / 64];
  double wave_P[TRK_THREADS / 64];
  int wave_c[TRK_THREADS / 64], wave_u[TRK_THREADS / 64];
  float stage[SEQ_STAGE_FLOATS];
  float result;
  int fell_back;
};
// the terms [j0, j0 + 4 nq) of a pass as nq float4 (16-byte aligned: the buffers are, and runs are multiples of four terms long); reads up to SEQ_RUN_MAX terms
// past the last one the caller will use (the buffers are padded by that much)
template <bool COH>
__device__ __forceinline__ void seq_load_run(svs_gptr_f32 p, int nq, svs_f4 (&v)[SEQ_Q]) {
  if constexpr (COH) {
    // past the caches, as the sibling workgroups stored them (sc1 = agent scope on gfx950, what an agent-scope atomic load compiles to); all ten requests in
    // flight before the one wait -- ten atomic dword loads in a row would be forty round trips
    static_assert(SEQ_Q == 10 || SEQ_Q == 13, "the blocks below issue ten (+ three) loads");
    asm volatile("global_load_dwordx4 %0, %10, off sc1\n\t"
                 "global_load_dwordx4 %1, %10, off offset:16 sc1\n\t"
                 "global_load_dwordx4 %2, %10, off offset:32 sc1\n\t"
                 "global_load_dwordx4 %3, %10, off offset:48 sc1\n\t"
                 "global_load_dwordx4 %4, %10, off offset:64 sc1\n\t"
                 "global_load_dwordx4 %5, %10, off offset:80 sc1\n\t"
                 "global_load_dwordx4 %6, %10, off offset:96 sc1\n\t"
                 "global_load_dwordx4 %7, %10, off offset:112 sc1\n\t"
                 "global_load_dwordx4 %8, %10, off offset:128 sc1\n\t"
                 "global_load_dwordx4 %9, %10, off offset:144 sc1\n\t"
                 "s_waitcnt vmcnt(0)"
                 : "=&v"(v[0]), "=&v"(v[1]), "=&v"(v[2]), "=&v"(v[3]), "=&v"(v[4]), "=&v"(v[5]), "=&v"(v[6]), "=&v"(v[7]), "=&v"(v[8]), "=&v"(v[9])
                 : "v"(p)
                 : "memory");
    if constexpr (SEQ_Q == 13)
      asm volatile("global_load_dwordx4 %0, %3, off offset:160 sc1\n\t"
                   "global_load_dwordx4 %1, %3, off offset:176 sc1\n\t"
                   "global_load_dwordx4 %2, %3, off offset:192 sc1\n\t"
                   "s_waitcnt vmcnt(0)"
                   : "=&v"(v[SEQ_Q - 3]), "=&v"(v[SEQ_Q - 2]), "=&v"(v[SEQ_Q - 1])
                   : "v"(p)
                   : "memory");
  } else {
#pragma unroll
    for (int q = 0; q < SEQ_Q; ++q) v[q] = q < nq ? *reinterpret_cast<svs_gptr_f4>(p + 4 * q) : svs_f4{0.f, 0.f, 0.f, 0.f};
  }
}
__shared__ SeqShared g_seq_sh;      // file scope: the routine below is a real call, and a reference handed through a call would be a flat pointer too
template <bool COH>
__device__ __noinline__ float exact_seq_sum_f32(const float *t_flat, int n) {
  SeqShared &sh = g_seq_sh;
  svs_gptr_f32 t = (svs_gptr_f32)t_flat;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int S = max(4, (div_up(n, TRK_THREADS) + 3) & ~3);      // terms per lane: a multiple of four
  if (S > SEQ_RUN_MAX) {                                         // images beyond 640 x 512: the chain (never with the reference's cameras)
    __syncthreads();
    if (wave == 0) { const float v = seq_sum_f32<COH, svs_gptr_f32>(t, n); if (lane == 0) { sh.result = v; sh.fell_back = 1; } }
    __syncthreads();
    return sh.result;
  }
  const int nq = S / 4;
  const int j0 = min(n, tid * S), j1 = min(n, j0 + S);
  const bool empty = j0 >= j1;
  svs_f4 v[SEQ_Q];
  seq_load_run<COH>(t + (empty ? 0 : j0), nq, v);
  double ps = 0;
  int cnt = 0;
#pragma unroll
  for (int q = 0; q < SEQ_Q; ++q)
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      if (!(q < nq && j0 + 4 * q + c < j1)) v[q][c] = 0.f;      // past my run / past the last term: zeros add nothing anywhere below
      ps += (double)v[q][c];
      cnt += v[q][c] != 0.f ? 1 : 0;
    }
  double incl = ps;
  int cincl = cnt;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const double o = __shfl_up(incl, d, 64);
    const int oc = __shfl_up(cincl, d, 64);
    if (lane >= d) { incl += o; cincl += oc; }
  }
  __syncthreads();                                   // (sh may still be read by the walker of the previous call)
  if (lane == 63) { sh.wave_P[wave] = incl; sh.wave_c[wave] = cincl; }
  __syncthreads();
  double base = 0;
  int cbase = 0;
  for (int w = 0; w < wave; ++w) { base += sh.wave_P[w]; cbase += sh.wave_c[w]; }
  // exclusive prefix as a sum of the earlier runs (never a difference: the bound in svs_seq_safe covers f64 sums of non-negative terms only)
  const double excl = __shfl_up(incl, 1, 64);
  const int cexcl = __shfl_up(cincl, 1, 64);
  const double P_s = base + (lane ? excl : 0.0), P_e = P_s + ps;
  const int c_s = cbase + (lane ? cexcl : 0), c_e = c_s + cnt;
  int eb = 0;
  bool safe = empty || svs_seq_safe(P_s, P_e, c_s, c_e, &eb);
  sh.eb[tid] = (safe && !empty) ? (unsigned char)eb : (unsigned char)0;
  __syncthreads();
  // two neighbouring safe runs share their binade (P_s of one is P_e of the other); nothing below relies on that proof: a change of binade ends the group
  if (safe && !empty && tid > 0) { const int pe = sh.eb[tid - 1]; if (pe != 0 && pe != eb) safe = false; }
  const unsigned long long um = __ballot(!safe);
  if (lane == 0) { sh.unsafe[wave] = um; sh.wave_u[wave] = __popcll(um); }
  __syncthreads();
  int ubase = 0;
  for (int w = 0; w < wave; ++w) ubase += sh.wave_u[w];
  const int uidx = ubase + __popcll(um & ((1ull << lane) - 1ull));
  const int slot = (!safe && (uidx + 1) * S <= SEQ_STAGE_FLOATS) ? uidx : -1;
  sh.slot[tid] = (short)slot;
  if (!safe) sh.eb[tid] = 0;
  SvsSeqMap m{0, 0};
  if (safe) {
#pragma unroll
    for (int q = 0; q < SEQ_Q; ++q)
#pragma unroll
      for (int c = 0; c < 4; ++c) svs_seq_add_term_fast(m, v[q][c], eb);      // (zeros past the run add nothing)
  } else if (slot >= 0) {
#pragma unroll
    for (int q = 0; q < SEQ_Q; ++q)
      if (q < nq) *reinterpret_cast<svs_f4 *>(&sh.stage[slot * S + 4 * q]) = v[q];
  }
  bool flag = !safe || lane == 0;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const int o0 = __shfl_up(m.d0, d, 64), o1 = __shfl_up(m.dd, d, 64), of = __shfl_up((int)flag, d, 64);
    if (lane >= d && !flag) { m = svs_seq_compose(SvsSeqMap{o0, o1}, m); flag = of != 0; }
  }
  sh.pref[tid] = m;
  __syncthreads();
  if (wave == 0) {
    float acc = 0.f;
    bool ok = true;
    const int nseg = div_up(n, S);
    for (int chunk = 0; chunk * 64 < nseg && ok; ++chunk) {
      const int limit = min(64, nseg - chunk * 64);
      const unsigned long long mask = sh.unsafe[chunk];
      // this chunk's 64 runs, one per lane, in registers: the walk below is a dependent chain, and a readlane is a tenth of an LDS round trip
      const SvsSeqMap my = sh.pref[chunk * 64 + lane];
      const int my_eb = sh.eb[chunk * 64 + lane], my_sl = sh.slot[chunk * 64 + lane];
      // the terms of an unsafe run, one per lane (staged in LDS by the run's own lane, else from global memory); the NEXT unsafe run's terms are requested
      // before this one's chain of adds starts, so that only the first LDS round trip of a chunk is exposed
      auto run_terms = [&](int idx) {
        const int seg = chunk * 64 + idx, sj0 = seg * S, len = min(S, n - sj0), sl = __builtin_amdgcn_readlane(my_sl, idx);      // len <= SEQ_RUN_MAX <= 64
        // (two loads and a select of VALUES: a select of the two addresses would make a flat pointer out of an LDS and a global one)
        float x = sh.stage[(sl >= 0 && lane < len) ? sl * S + lane : 0];
        if (sl < 0) x = seq_term_load<COH, svs_gptr_f32>(t + sj0 + (lane < len ? lane : 0));
        return lane < len ? x : 0.f;
      };
      unsigned long long m = limit < 64 ? mask & ((1ull << limit) - 1ull) : mask;
      float x_next = m ? run_terms((int)__builtin_ctzll(m)) : 0.f;
      int pos = 0;
      while (ok) {
        const int nxt = m ? (int)__builtin_ctzll(m) : limit;
        if (nxt > pos) {
          const SvsSeqMap g{__builtin_amdgcn_readlane(my.d0, nxt - 1), __builtin_amdgcn_readlane(my.dd, nxt - 1)};
          ok = svs_seq_apply(&acc, g, __builtin_amdgcn_readlane(my_eb, nxt - 1));
        }
        if (nxt >= limit || !ok) break;
        m &= m - 1ull;
        const float x = x_next;
        if (m) x_next = run_terms((int)__builtin_ctzll(m));
#pragma unroll
        for (int l = 0; l < SEQ_RUN_MAX; ++l) acc = acc + __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, x), l));      // (+ 0 past the run: exact)
        pos = nxt + 1;
      }
    }
    if (!ok) acc = seq_sum_f32<COH, svs_gptr_f32>(t, n);
    if (lane == 0) { sh.result = acc; if (!ok) sh.fell_back = 1; }
  }
  __syncthreads();
  return sh.result;
}

// The exact float sums of a near-tie when several workgroups share a stream (latency mode, continuation launch).  Every workgroup must take the same decision, the
// sums must be formed ONCE (round 5 formed them in all eight workgroups), and nobody may start the next sweep -- which overwrites one of the two term buffers -- before
// the readers are done.  Workgroup 0 forms the trial pass's sum; when the accepted pass's sum is not known either (the level's first near-tie, or the
// first after an accepted step that needed no sums) workgroup 1 forms it AT THE SAME TIME on its own CU.  Each publishes ONE 8-byte word (count of such events << 32 | the
// float's bits: value and flag in one atomic store, no fence, no second store) in the stream's hand-over block (bc[13]: trial sum, bc[15]: accepted sum), and every
// workgroup waits for the word(s) it did not form itself.  n_dec / n_old: how many trial / accepted sums this stream has needed so far, this one included (all workgroups count alike).
struct NearSums { float seq_old, seq_new; bool failed; };
template <bool COH>
__device__ __forceinline__ NearSums shared_near_sums(const float *t_old, const float *t_new, int n, int wg, int nwg, bool need_old, float seq_old_in, unsigned n_dec, unsigned n_old,
                                                     double *bc, unsigned *fail_word, unsigned &n_exact) {
  __shared__ unsigned long long s_words[2];
  __shared__ int s_nf;
  NearSums R{seq_old_in, 0.f, false};
  if (nwg <= 1) {                                    // one workgroup: both sums here, nothing to hand over
    if (need_old) { R.seq_old = exact_seq_sum_f32<COH>(t_old, n); ++n_exact; }
    R.seq_new = exact_seq_sum_f32<COH>(t_new, n); ++n_exact;
    return R;
  }
  unsigned long long *w_new = reinterpret_cast<unsigned long long *>(bc + 13), *w_old = reinterpret_cast<unsigned long long *>(bc + 15);
  if (wg == 0) {
    R.seq_new = exact_seq_sum_f32<COH>(t_new, n); ++n_exact;
    if (threadIdx.x == 0) __hip_atomic_store(w_new, ((unsigned long long)n_dec << 32) | (unsigned long long)__float_as_uint(R.seq_new), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  } else if (wg == 1 && need_old) {
    R.seq_old = exact_seq_sum_f32<COH>(t_old, n); ++n_exact;
    if (threadIdx.x == 0) __hip_atomic_store(w_old, ((unsigned long long)n_old << 32) | (unsigned long long)__float_as_uint(R.seq_old), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  if (threadIdx.x == 0) {
    int nf = 0;
    auto wait_word = [&](const unsigned long long *w, unsigned want) {
      unsigned long long v = 0;
      long spin = 0;
      for (; spin < (1l << 24); ++spin) { v = __hip_atomic_load(w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); if ((unsigned)(v >> 32) >= want) break; __builtin_amdgcn_s_sleep(1); }
      if (spin >= (1l << 24)) nf = 1;
      return v;
    };
    s_words[0] = wg == 0 ? 0ull : wait_word(w_new, n_dec);
    s_words[1] = (need_old && wg != 1) ? wait_word(w_old, n_old) : 0ull;
    if (nf) __hip_atomic_store(fail_word, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    s_nf = nf;
  }
  __syncthreads();
  if (wg != 0) R.seq_new = __uint_as_float((unsigned)s_words[0]);
  if (need_old && wg != 1) R.seq_old = __uint_as_float((unsigned)s_words[1]);
  R.failed = s_nf != 0;
  __syncthreads();                                   // (s_words is rewritten at the next near-tie)
  return R;
}

// MULTI: a few streams only (latency mode) -- gridDim.x workgroups share every sweep of one stream.  Each leaves its 29 partial
// sums in global memory, a device-scope counter barrier (all workgroups of the launch are resident: NW * batch <= #CUs) lets
// every workgroup add the partials up in the same fixed order, and each then runs the identical LM bookkeeping redundantly,
// so no pose has to be broadcast.  Partials are double-buffered by pass parity: a workgroup can only overwrite a buffer after
// everyone has passed the barrier of the pass in between, i.e. after everyone has read it.
// The cross-workgroup exchange below (partials, arrival counter, hand-over of the coarse level's pose) uses RELAXED agent-scope atomics plus a raw
// `s_waitcnt vmcnt(0)` instead of release / acquire fences: on gfx950 (and gfx942) vmcnt counts stores as well as loads and sc1 atomics write through /
// bypass the non-coherent per-XCD L2, so "all my stores have left" + "flag store" is a release in practice.  This is OUTSIDE the HIP memory model and wrong on
// any target that counts stores separately (vscnt: gfx10 and later) -- hence the hard stop.
#if defined(__HIP_DEVICE_COMPILE__) && !defined(__gfx950__) && !defined(__gfx942__)
#error "dense.hip: the relaxed-atomic + s_waitcnt vmcnt(0) hand-off is only valid on gfx950 / gfx942"
#endif
struct TrackMulti {
  double *part;                                   // [batch][2][nwg][32] partial sums of the shared sweeps, by sweep parity (latency mode: [batch][2][nwg][64] flagged words)
  unsigned *bar; int fail_off;                    // [batch] arrival counters + [batch] failure flags at bar + fail_off (zeroed before the launch)
  double *bcast;                                  // [batch][16]: the pose after the coarsest level + a ready word (zeroed before the launch)
  const int *map;                                 // the ordered launch of a big batch: workgroup -> (stream << 4)
  float *terms; size_t terms_b;                   // the float terms of the accepted and of the trial pass, [batch][2][terms_b] (null: accept test on the f64 sums alone)
  unsigned *seq_stats;                            // [0] exact sums formed, [1] fallbacks to the chain
  int terms_only;                                 // kernel A/B: the stores of the terms without the sums
  int *work16;                                    // (optional, flat kernel): [batch] the stream's passes counted as 16 / 4 / 1 per sweep of level 0 / 1 / 2
};

// ---- the LM step, written once: both tracker kernels below (the nested-loop kernel, the flat kernel of big batches) inline these ---------------------------------
// the operands of a stream's sweeps of one level: the level's cloud and images at the stream's batch offsets
template <bool U8SRC>
__device__ __forceinline__ LevelArgs stream_level(const TrackArgs &A, int level, int slot) {
  LevelArgs L = A.lv[level];
  L.cloud += slot * A.cloud_b[level]; L.prev += slot * A.prev_b[level];
  if (U8SRC) L.cur8 += slot * A.c8_b[level];
  else { L.cur += slot * A.f_b[level]; L.dx += slot * A.f_b[level]; L.dy += slot * A.f_b[level]; }
  return L;
}
// the solve of an iteration, on seven lanes of wave 0 (called with threadIdx.x < 64): H.ldlt().solve(-Jres), undamped (dense_tracking.cpp:332) + exp(x) * T.
// All four in LDS: sH = H (packed upper by column) and b of the accepted pass, sT = the accepted pose -> sTn = the trial pose, sx = the step
__device__ __forceinline__ void track_solve(const double (&sH)[27], const double (&sT)[12], double (&sTn)[12], double (&sx)[6]) {
  const int lane = threadIdx.x;
  double col[6], x[6], Tc[12], Tn[12];
#pragma unroll
  for (int r = 0; r < 6; ++r) {
    const int lo = r < lane ? r : lane, hi = r < lane ? lane : r;      // packed upper by column: (lo, hi) at hi (hi + 1) / 2 + lo
    col[r] = lane < 6 ? sH[hi * (hi + 1) / 2 + lo] : (lane == 6 ? -sH[21 + r] : (r == 0 ? 1.0 : 0.0));
  }
  wave_solve6(col, x);
#pragma unroll
  for (int i = 0; i < 12; ++i) Tc[i] = sT[i];
  mo2_exp_mul(x, Tc, Tn);
  if (lane < 12) {
    double v = Tn[0];
#pragma unroll
    for (int i = 1; i < 12; ++i) v = lane == i ? Tn[i] : v;
    sTn[lane] = v;
  }
  if (lane < 6) {
    double v = x[0];
#pragma unroll
    for (int i = 1; i < 6; ++i) v = lane == i ? x[i] : v;
    sx[lane] = v;
  }
}
// g_s_out[0..NSUM] <- the sums of all nwg workgroups of a stream, added in workgroup order.  buf: the [nwg][32] partials of this sweep's parity; sweep: the sweeps the
// stream has shared so far (target of its arrival counter); s_failed (LDS): a sibling never arrived.  Write-through 8-byte words + one arrival counter (relaxed, agent
// scope) + vmcnt(0): no fence that would write an XCD's whole L2 back -- valid on gfx950 / gfx942 only, see the #error above
__device__ __forceinline__ void sum_workgroups(const TrackMulti &G, int slot, double *buf, int wg, int nwg, int &sweep, bool &s_failed) {
  if (threadIdx.x <= NSUM) __hip_atomic_store(buf + wg * 32 + threadIdx.x, g_s_out[threadIdx.x], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  ++sweep;
  if (threadIdx.x == 0) {
    __hip_atomic_fetch_add(G.bar + slot, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const unsigned target = (unsigned)sweep * (unsigned)nwg;
    long spin = 0;
    for (; spin < (1l << 24) && __hip_atomic_load(G.bar + slot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < target; ++spin) __builtin_amdgcn_s_sleep(1);
    // a sibling workgroup never arrived (they are not all resident: the device is shared with other work).  Summing what is
    // there would let the replicated LM bookkeeping diverge silently: raise the stream's failure flag instead -- every
    // workgroup sees it at its next barrier at the latest, the pose is left as it came in and passes_out reports -1.
    if (spin >= (1l << 24)) __hip_atomic_store(G.bar + G.fail_off + slot, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    s_failed = __hip_atomic_load(G.bar + G.fail_off + slot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0;
  }
  __syncthreads();
  if (threadIdx.x <= NSUM) {
    double acc = 0;
    for (int w = 0; w < nwg; ++w) acc += __hip_atomic_load(buf + w * 32 + threadIdx.x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    g_s_out[threadIdx.x] = acc;
  }
  __syncthreads();
}
// The accept test of a trial: S_old / S_new = the f64 sums of the float terms of the accepted / the trial pass (nv_*: samples that contributed one), tb0 = the stream's two
// term buffers (null: none; the accepted pass's is number cur, the trial's the other one), chi2 = the accepted pass's chi2 as the loop carries it.  The reference compares two float sums of n terms each:
// |sum_float - sum_exact| <= ((1 + 2^-24)^(n - 1) - 1) sum_exact.  Outside that band the f64 sums decide as the float sums would; inside it (a near-tie) the float sums
// are formed, bit for bit (exact_seq_sum_f32): the trial's, and the accepted pass's unless the loop carries it (seq_old, seq_old_ok).  counted: the near-tie takes part
// in the stream's count of such events (n_decisions, n_old_sums: what the workgroups that share the sums wait for, shared_near_sums).  failed: a sibling never published
struct TrkVerdict { bool accept, failed; float chi2, new_chi2; };
template <bool MULTI>
__device__ __forceinline__ TrkVerdict track_accept(const TrackMulti &G, int slot, double S_old, double S_new, int nv_old, int nv_new, const float *tb0, int cur,
                                                   int n_lvl, bool counted, int wg, int nwg, float chi2, float &seq_old, bool &seq_old_ok,
                                                   unsigned &n_decisions, unsigned &n_old_sums, unsigned &n_exact) {
  TrkVerdict V{false, false, chi2, 0.f};
  const double gam = 1.0001 * (double)max(nv_old, nv_new) * 5.9604644775390625e-08 + 1e-12;
  const bool near = tb0 && !G.terms_only && !(fabs(S_old - S_new) > gam * (S_old + S_new));      // (terms_only: kernel A/B -- the stores without the sums)
  if (near) {
    if (counted) { ++n_decisions; if (!seq_old_ok) ++n_old_sums; }
    const NearSums ns = shared_near_sums<MULTI>(tb0 + (size_t)cur * G.terms_b, tb0 + (size_t)(cur ^ 1) * G.terms_b, n_lvl, wg, nwg, !seq_old_ok, seq_old, n_decisions, n_old_sums,
                                                MULTI ? G.bcast + (size_t)slot * 16 : nullptr, MULTI ? G.bar + G.fail_off + slot : nullptr, n_exact);
    if (ns.failed) { V.failed = true; return V; }
    seq_old = ns.seq_old;
    seq_old_ok = true;
    V.chi2 = seq_old; V.new_chi2 = ns.seq_new;
    V.accept = (double)V.chi2 - (double)V.new_chi2 > 0;
    if (V.accept) seq_old = ns.seq_new;
  } else {
    V.new_chi2 = (float)S_new;
    V.accept = S_old > S_new;
    if (V.accept) seq_old_ok = false;
  }
  return V;
}

// ---- the nested-loop kernel: latency mode (MULTI), at most one stream per CU, "trk_seq_chi2" (SEQ) -----------------------------------------------------------
// Built for two waves per SIMD (<= 256 VGPRs; the kernel takes 147: one 8-wave workgroup per CU): room for the sweep inline in the level / iteration loops
// beside everything those loops keep alive.  Batches of more than one stream per CU run dense_track_batch_kernel below, which is held to this one bit for bit.
template <bool U8SRC, bool MULTI, bool SEQ = false>      // SEQ: "trk_seq_chi2" (its own instantiation: the hot ones keep their register budget)
__global__ __launch_bounds__(TRK_THREADS, 2) void dense_track_cpu_sem_kernel(TrackArgs A, double *__restrict__ T_io, int *__restrict__ passes_out, TrackMulti G) {
  double (&s_out)[NSUM + 1] = g_s_out;
  float (&s_iplut)[256] = g_iplut;
  __shared__ double s_T[12], s_Tn[12], s_x[6], s_H[27], s_Tj[3][12];
  __shared__ bool s_failed;
  if (threadIdx.x == 0) { s_failed = false; if (!SEQ) g_seq_sh.fell_back = 0; }
  constexpr int TM = SEQ ? 1 : (MULTI ? 2 : 1);      // the terms of a pass: plain stores, or past the caches when sibling workgroups read them
  unsigned n_exact = 0, n_decisions = 0, n_old_sums = 0;      // exact float sums formed by this workgroup; near-ties of this stream so far / those of them that needed the accepted pass's sum as well (shared_near_sums)
  const int slot = MULTI ? blockIdx.y : blockIdx.x, wg = MULTI ? blockIdx.x : 0;
  const int nwg = MULTI ? (int)gridDim.x : 1;
  const int first = wg * TRK_THREADS + threadIdx.x;
  int sweep = 0;
  auto all_workgroups = [&]() {      // s_out[0..NSUM] <- sum over the workgroups of this stream
    if (!MULTI) return;
    // Round 6: every 8-byte word carries its own flag (4 bytes of data + the sweep number: what NCCL calls the LL protocol).  A workgroup publishes its 29 sums as 58
    // such words and reads the others' the moment they carry this sweep's number: ONE store-to-load hop between workgroups -- no drain of the store queue, no arrival
    // counter (a device-scope read-modify-write), no second wait.  Rounds 2-5: stores, s_waitcnt vmcnt(0), barrier, counter += 1, poll the counter, barrier, loads --
    // 4-5 us of a 10 us pass in latency mode.  Two parities of buffers: a word is overwritten two sweeps later, which its writer can only reach after every sibling has
    // consumed this sweep (it needs their next sweep's words to get there).  The buffers are zeroed before the launch (sweep numbers start at 1).
    const unsigned ep = (unsigned)(++sweep);
    unsigned long long *buf = reinterpret_cast<unsigned long long *>(G.part) + ((size_t)slot * 2 + (ep & 1u)) * (size_t)nwg * 64;
    bool timed_out = false;
    if (threadIdx.x < 2 * (NSUM + 1)) {
      const int k = threadIdx.x;
      const double mine = s_out[k >> 1];
      const unsigned my_half = (k & 1) ? (unsigned)__double2hiint(mine) : (unsigned)__double2loint(mine);
      __hip_atomic_store(buf + (size_t)wg * 64 + k, ((unsigned long long)ep << 32) | my_half, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      double acc = 0;
      long budget = 1l << 24;
      for (int w = 0; w < nwg; ++w) {                      // workgroup order: the same sum in every workgroup
        unsigned h = my_half;
        if (w != wg) {
          unsigned long long v = __hip_atomic_load(buf + (size_t)w * 64 + k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          while ((unsigned)(v >> 32) != ep && budget > 0) { __builtin_amdgcn_s_sleep(1); --budget; v = __hip_atomic_load(buf + (size_t)w * 64 + k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
          if ((unsigned)(v >> 32) != ep) timed_out = true;
          h = (unsigned)v;
        }
        const unsigned other = (unsigned)__shfl_xor((int)h, 1, 64);      // even lane: the low half is mine, the high half my neighbour's
        acc += __hiloint2double((int)((k & 1) ? h : other), (int)((k & 1) ? other : h));
      }
      if (!(k & 1)) s_out[k >> 1] = acc;                     // (this wave published from s_out before any lane of it writes here)
    }
    // a sibling never published (not resident: the device is shared with other work): raise the stream's failure flag -- the pose is left as it came in, passes_out reports -1
    if (__syncthreads_or(timed_out ? 1 : 0)) {
      if (threadIdx.x == 0) { __hip_atomic_store(G.bar + G.fail_off + slot, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); s_failed = true; }
      __syncthreads();
    }
  };
  if (threadIdx.x < 12) s_T[threadIdx.x] = T_io[(size_t)slot * 12 + threadIdx.x];
  for (int i = threadIdx.x; i < 256; i += TRK_THREADS) s_iplut[i] = (float)((1. / 255.) * i);
  __syncthreads();
  int passes = 0, n_rec = 0;
  bool failed = false;
  // One fused pass per LM iteration.  The reference runs, per iteration, an H,b pass at T and a
  // chi2 pass at T_new, and after an accepted step starts the next iteration with an H,b pass at
  // that same T_new.  Evaluating chi2 AND H,b together at T_new therefore serves both (identical
  // sums, one gather sweep instead of two).  A rejected step makes the reference repeat the same
  // undamped solve at the unchanged T (mu is never applied, dense_tracking.cpp:332), reject again and
  // stop (trial == 2, :379-384): that is "stop on the first rejection" here.
  for (int level = 2; level >= 0; --level) {
    // MULTI: the coarsest level (1/16 of the samples: less than one per lane and workgroup) is run by workgroup 0 ALONE -- a sweep of it is
    // shorter than the cross-workgroup exchange that sharing it would cost -- and the others pick the pose up when it is done
    const bool solo = MULTI && level == 2;
    if (solo && wg != 0) {
      if (threadIdx.x == 0) {
        long spin = 0;
        for (; spin < (1l << 24) && __hip_atomic_load(reinterpret_cast<unsigned *>(G.bcast + (size_t)slot * 16 + 12), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 0u; ++spin)
          __builtin_amdgcn_s_sleep(2);
        if (spin >= (1l << 24)) s_failed = true;
      }
      __syncthreads();
      if (s_failed) { failed = true; break; }
      if (threadIdx.x < 12) s_T[threadIdx.x] = __hip_atomic_load(G.bcast + (size_t)slot * 16 + threadIdx.x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      __syncthreads();
      continue;
    }
    const int lnwg = solo ? 1 : nwg;
    const LevelArgs L = stream_level<U8SRC>(A, level, slot);
    const int n_lvl = (L.cam.w / 4) * (L.cam.h / 4);
    __syncthreads();      // (between the levels: everybody is through with the last trial's sums and state)
    auto sweep_at = [&](const double *s_pose, float *t_buf) {      // s_pose: 12 doubles in LDS
      track_pass<true, U8SRC, TM>(L, s_pose, g_s_part, g_s_out, g_iplut, solo ? (int)threadIdx.x : first, lnwg, t_buf);
    };
    // SEQ: one term buffer, every sum by the chain ("trk_seq_chi2"; never MULTI: G.part carries the buffer and fail_off its stream stride).
    // Default: two buffers -- the terms of the accepted pass (tb[cur]) and of the trial -- for the sums the accept test cannot decide in f64 (seqsum.h)
    float *tb[2];
    tb[0] = SEQ ? reinterpret_cast<float *>(G.part) + (size_t)slot * G.fail_off : (G.terms ? G.terms + (size_t)slot * 2 * G.terms_b : nullptr);
    tb[1] = SEQ ? tb[0] : (G.terms ? tb[0] + G.terms_b : nullptr);
    int cur = 0;
    // (inlined by hand -- and with it the trial sweep below, then the lambda's one remaining use: with two trips per iteration the sweep is past the inliner's
    // own threshold, and left alone both sweeps of this kernel became calls of one out-of-line copy built for 246 / 214 registers)
    [[clang::always_inline]] sweep_at(s_T, tb[cur]);        // chi2 (dense_tracking.cpp:229-261) + H,b of iteration 0
    if (!solo) all_workgroups();
    if (MULTI && s_failed) { failed = true; break; }
    ++passes;
    float chi2;
    double S_old = s_out[27];                  // the f64 sum of the same float terms: exact to 1e-13
    int nv_old = (int)s_out[NSUM];             // samples that contributed a term (adding the zero of a skipped sample is exact)
    float seq_old = 0.f;
    bool seq_old_ok = false;
    if constexpr (SEQ) chi2 = seq_chi2_f32(tb[0], n_lvl); else chi2 = (float)S_old;
    if (threadIdx.x < 27) s_H[threadIdx.x] = s_out[threadIdx.x];
    if (A.rec && wg == 0 && threadIdx.x == 0 && n_rec < A.rec_cap) A.rec[(size_t)slot * A.rec_cap + n_rec] = svs_dense_lm_record{level, 2, chi2, chi2};
    ++n_rec;
    __syncthreads();
    bool stop = false;
    for (int it = 0; it < 15 && !stop; ++it) {
      if (threadIdx.x >= 64 && threadIdx.x < 76) s_Tj[level][threadIdx.x - 64] = s_T[threadIdx.x - 64];   // the reference's H,b pass of this iteration ran at s_T
      if (threadIdx.x < 64) track_solve(s_H, s_T, s_Tn, s_x);
      __syncthreads();
      sweep_at(s_Tn, tb[cur ^ 1]);      // new_chi2 (:335-367) + H,b for the next iteration
      if (!solo) all_workgroups();
      if (MULTI && s_failed) { failed = true; break; }
      ++passes;
      float new_chi2;
      bool accept;
      const double S_new = s_out[27];
      const int nv_new = (int)s_out[NSUM];
      if constexpr (SEQ) {
        new_chi2 = seq_chi2_f32(tb[0], n_lvl);
        accept = (double)chi2 - (double)new_chi2 > 0;
      } else {
        const bool shared = MULTI && !solo;      // (the coarsest level of a shared stream is run by its leader alone: its near-ties are not counted, the siblings never see them)
        const TrkVerdict V = track_accept<MULTI>(G, slot, S_old, S_new, nv_old, nv_new, tb[0], cur, n_lvl, shared, shared ? wg : 0, shared ? nwg : 1,
                                                 chi2, seq_old, seq_old_ok, n_decisions, n_old_sums, n_exact);
        if (V.failed) { s_failed = true; failed = true; break; }
        accept = V.accept; chi2 = V.chi2; new_chi2 = V.new_chi2;
        if (accept) { S_old = S_new; nv_old = nv_new; cur ^= 1; }
      }
      if (A.rec && wg == 0 && threadIdx.x == 0 && n_rec < A.rec_cap) A.rec[(size_t)slot * A.rec_cap + n_rec] = svs_dense_lm_record{level, accept ? 1 : 0, chi2, new_chi2};
      ++n_rec;
      if (accept) {
        chi2 = new_chi2;
        double mx = -1;
        for (int q = 0; q < 6; ++q) mx = fmax(mx, fabs(s_x[q]));
        stop = mx <= 1e-10;
        if (threadIdx.x < 12) s_T[threadIdx.x] = s_Tn[threadIdx.x];
        if (threadIdx.x < 27) s_H[threadIdx.x] = s_out[threadIdx.x];
        __syncthreads();
      } else {
        stop = true;
      }
    }
    if (failed) break;
    if (solo) {                                      // workgroup 0 hands the pose of the coarsest level to its siblings
      __syncthreads();
      if (threadIdx.x < 12) __hip_atomic_store(G.bcast + (size_t)slot * 16 + threadIdx.x, s_T[threadIdx.x], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __syncthreads();
      if (threadIdx.x == 0) __hip_atomic_store(reinterpret_cast<unsigned *>(G.bcast + (size_t)slot * 16 + 12), 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
  __syncthreads();
  if (wg != 0) return;
  if (failed) { if (threadIdx.x == 0 && passes_out) passes_out[slot] = -1; return; }      // pose left as it came in
  if (threadIdx.x < 12) T_io[(size_t)slot * 12 + threadIdx.x] = s_T[threadIdx.x];
  if (threadIdx.x == 0 && passes_out) passes_out[slot] = passes;
  if (threadIdx.x == 0 && A.n_rec) A.n_rec[slot] = n_rec;
  if (A.T_jac && threadIdx.x < 36) A.T_jac[(size_t)slot * 36 + threadIdx.x] = s_Tj[threadIdx.x / 12][threadIdx.x % 12];
  if (threadIdx.x == 0 && G.seq_stats && n_exact) {
    atomicAdd(G.seq_stats, n_exact);
    if (g_seq_sh.fell_back) atomicAdd(G.seq_stats + 1, 1u);
  }
}

// ---- big batches: the LM loop as a flat state machine around ONE inlined sweep ---------------------------------------------------------------------------------
// Two 512-lane workgroups per CU (the second one hides the first one's dependent chains: 0.55 -> 0.45 ms per 256 streams) leave 128 vector registers, and the sweep
// fills them by itself.  Inlined into level / iteration loops like the kernel above's, everything those loops keep alive (sums, flags, buffers: uniform values the
// compiler cannot prove uniform) shares the sweep's allocation and spills inside the loop over the samples; as a callee the sweep saves and restores every callee-saved
// register it touches, 29 dwords per lane and call.  So the LM state of the stream lives in LDS (TrkState: one lane writes it, everybody reads what it needs), the kernel
// is ONE loop { sweep; step }, and nothing of the step is alive while the sweep runs: no call on the hot path, no callee-saved traffic, no spills in the sweep.  Same
// sweep, same sums, same solve, same decisions as the kernel above: bit-identical results (tests/test_gpu_frontend_batch.py::test_tracker_grid_order_does_not_change_results).
struct TrkState {
  double S_old; float chi2, seq_old;
  int work16;                                                        // passes so far, weighted 16 / 4 / 1 by level (what trk_assign_kernel orders the next frame's grid by)
  int level, it, cur, passes, n_rec, nv_old, seq_old_ok, phase;      // phase 0: the sweep just run was the level's first (chi2 + H,b at the accepted pose); 1: a trial
  unsigned n_exact;
};
__shared__ TrkState g_ts;
// the solve of an iteration (track_solve) as a function of its own, called by ONE wave: its 70-odd live doubles are not part of the kernel's allocation, and whatever it
// saves on entry it saves for 64 lanes, not 512.
__shared__ double g_sT[12], g_sTn[12], g_sx[6], g_sH[27], g_sTj[3][12];
__device__ __noinline__ void track_solve_call() { track_solve(g_sH, g_sT, g_sTn, g_sx); }
// ---- the tail of a big batch: the CONTINUATION launch ("trk_split", VERDICT round 5 item 2 iii) ------------------------------------------------------------------
// All streams of a big batch are resident at once (two workgroups per CU) and the launch lasts as long as its longest stream: 16.75 level-0 sweeps in the bench's batch
// against a mean of 8.7 -- and the last sweeps of a stream are the ones whose accept test needs the exact float sums, one after the other on the critical path.  Predicting
// the long streams from the last frame does not work (correlation -0.18 in the bench).  So the first launch (CONT = 0) runs every stream with one workgroup as before, but a
// stream that has taken K trials on level 0 and is still not done PARKS: its LM state -- the accepted pose, H,b of the accepted pass, the sums the accept test carries,
// the term buffers (they are in global memory already) -- goes to global memory, its index to a list, and the workgroup exits.  The second launch (CONT = 1) takes the list:
// every parked stream is resumed by CONT_MAX_NWG = 8 workgroups that share each sweep exactly like the latency mode does (partial sums through write-through words + one
// arrival counter, the leader forms the exact float sums and publishes the decision).  A trial of a parked stream then takes ~30 us instead of ~170.  The launch has
// slots / 8 groups of eight siblings; a group resumes the parked streams y, y + groups, ... one after the other, so more parked streams than fit at once wait for a
// group instead of getting fewer workgroups.  K and the eight are constants, so which sweeps run in which form, and the order every partial sum is added in, are a
// function of the stream's own data alone: its result does not depend on the other streams of the batch, the batch size, "trk_cont_slots" or the device's CU count.
// The partial sums of a shared sweep are added in another order than the one-workgroup sweep's, so H,b differ from the unsplit run in their last bits (pose 1e-12),
// while the accept decisions are the reference's either way (exact float sums of the terms).
struct TrkPark { TrkState ts; double T[12], H[27], Tj[36]; };
struct TrackCont { TrkPark *park; int *list; unsigned *count; int K; int slots; };      // K < 0: no parking; slots: resident workgroup slots of the device for the second launch (its concurrency, not its results)
constexpr int CONT_MAX_NWG = 8;
// one stream of a big batch: the whole LM loop (MULTI = false: first launch, one workgroup) or the rest of a parked stream (MULTI: workgroup wg of the stream's
// CONT_MAX_NWG).  Every word the siblings of a stream exchange -- partials, arrival counter, failure flag, hand-over words -- belongs to the STREAM (slot), and each
// parked stream is resumed exactly once, so nothing needs resetting between the streams one group of siblings resumes in turn.
template <bool U8SRC, bool MULTI>
__device__ __forceinline__ void track_batch_stream(const TrackArgs &A, double *__restrict__ T_io, int *__restrict__ passes_out, const TrackMulti &G, const TrackCont &C,
                                                   const int slot, const int wg, const int nwg) {
  constexpr int TM = MULTI ? 2 : 1;
  const int tid = threadIdx.x;
  __shared__ bool s_failed;
  float *const tb0 = G.terms ? G.terms + (size_t)slot * 2 * G.terms_b : nullptr;
  // level set-up (one lane): the operands of the level's sweeps
  auto set_level = [&](int level) { g_pa.L = stream_level<U8SRC>(A, level, slot); g_pa.wg = wg; g_pa.nwg = nwg; };
  auto enter_level = [&](int level) {          // ... the first sweep of the level at the accepted pose into term buffer 0
    set_level(level);
    g_pa.t_buf = tb0;
    g_ts.level = level; g_ts.phase = 0; g_ts.cur = 0; g_ts.it = 0;
  };
  for (int i = tid; i < 256; i += TRK_THREADS) g_iplut[i] = (float)((1. / 255.) * i);
  if (tid == 0) { g_seq_sh.fell_back = 0; s_failed = false; }
  int sweep = 0;                                   // MULTI: sweeps shared so far (parity of the partials' buffer, target of the arrival counter)
  unsigned n_decisions = 0, n_old_sums = 0;          // near-ties of this stream so far / those that needed the accepted pass's sum too (shared_near_sums)
  if constexpr (!MULTI) {
    if (tid < 12) { const double v = T_io[(size_t)slot * 12 + tid]; g_sT[tid] = v; g_pa.T[tid] = v; }
    if (tid == 0) {
      g_ts.passes = 0; g_ts.n_rec = 0; g_ts.n_exact = 0; g_ts.work16 = 0;
      enter_level(2);
    }
    __syncthreads();
  } else {
    // resume: the state as the first launch left it (behind a trial step that did not end the level); every workgroup of the stream loads it and goes on with the solve
    const TrkPark &P = C.park[slot];
    if (tid == 0) { g_ts = P.ts; if (wg != 0) g_ts.n_exact = 0; }
    if (tid < 12) g_sT[tid] = P.T[tid];
    if (tid >= 64 && tid < 64 + 27) g_sH[tid - 64] = P.H[tid - 64];
    if (tid >= 128 && tid < 128 + 36) g_sTj[(tid - 128) / 12][(tid - 128) % 12] = P.Tj[tid - 128];
    __syncthreads();
    if (tid == 0) set_level(g_ts.level);
    __syncthreads();
  }
  // MULTI: g_s_out <- the sums of all workgroups of the stream, added in workgroup order
  auto all_workgroups = [&]() {
    if (nwg == 1) return;
    sum_workgroups(G, slot, G.part + ((size_t)slot * 2 + (sweep & 1)) * CONT_MAX_NWG * 32, wg, nwg, sweep, s_failed);
  };
  bool failed = false, parked = false;
  bool resume = MULTI;                             // the continuation enters the loop behind a step: solve first
#pragma nounroll
  for (;;) {
    bool level_done = false;
    int level;
    if (!resume) {
      track_pass_from_lds<U8SRC, TM>();            // (ends in a barrier: g_s_out is complete)
      if constexpr (MULTI) { all_workgroups(); if (s_failed) { failed = true; break; } }
      // ---- the LM step: every lane reads the state, one lane writes it back
      level = g_ts.level;
      const int phase = g_ts.phase, cur = g_ts.cur, n_rec = g_ts.n_rec;
      const int n_lvl = (A.lv[level].cam.w / 4) * (A.lv[level].cam.h / 4);
      if (phase == 0) {                              // chi2 (dense_tracking.cpp:229-261) + H,b of iteration 0
        const double S = g_s_out[27];
        const float chi2 = (float)S;
        __syncthreads();                             // (everybody has read g_s_out / the state)
        if (tid < 27) g_sH[tid] = g_s_out[tid];
        if (tid == 0) {
          g_ts.S_old = S; g_ts.nv_old = (int)g_s_out[NSUM]; g_ts.chi2 = chi2; g_ts.seq_old_ok = 0; g_ts.seq_old = 0.f;
          ++g_ts.passes; ++g_ts.n_rec; g_ts.work16 += 16 >> (2 * level);
          if (A.rec && wg == 0 && n_rec < A.rec_cap) A.rec[(size_t)slot * A.rec_cap + n_rec] = svs_dense_lm_record{level, 2, chi2, chi2};
        }
      } else {                                       // new_chi2 (:335-367) + H,b for the next iteration
        const double S_old = g_ts.S_old, S_new = g_s_out[27];
        const int nv_old = g_ts.nv_old, nv_new = (int)g_s_out[NSUM];
        float seq_old = g_ts.seq_old;
        bool seq_old_ok = g_ts.seq_old_ok != 0;
        unsigned n_exact = 0;
        const TrkVerdict V = track_accept<MULTI>(G, slot, S_old, S_new, nv_old, nv_new, tb0, cur, n_lvl, true, wg, nwg, g_ts.chi2, seq_old, seq_old_ok, n_decisions, n_old_sums, n_exact);
        if (V.failed) { if (tid == 0) s_failed = true; failed = true; break; }
        const bool accept = V.accept;
        const float chi2 = V.chi2, new_chi2 = V.new_chi2;
        double mx = -1;
        for (int q = 0; q < 6; ++q) mx = fmax(mx, fabs(g_sx[q]));
        const int it = g_ts.it + 1;
        level_done = !accept || mx <= 1e-10 || it >= 15;
        __syncthreads();                             // (everybody has read g_s_out / the state / g_sx / s_word)
        if (accept) {
          if (tid < 12) g_sT[tid] = g_sTn[tid];
          if (tid < 27) g_sH[tid] = g_s_out[tid];
        }
        if (tid == 0) {
          if (accept) { g_ts.S_old = S_new; g_ts.nv_old = nv_new; g_ts.cur = cur ^ 1; g_ts.chi2 = new_chi2; }
          g_ts.seq_old = seq_old; g_ts.seq_old_ok = seq_old_ok ? 1 : 0; g_ts.it = it; g_ts.n_exact += n_exact;
          ++g_ts.passes; ++g_ts.n_rec; g_ts.work16 += 16 >> (2 * level);
          if (A.rec && wg == 0 && n_rec < A.rec_cap) A.rec[(size_t)slot * A.rec_cap + n_rec] = svs_dense_lm_record{level, accept ? 1 : 0, chi2, new_chi2};
        }
        // first launch: a stream that is still going after K trials on the finest level parks here (state of the accepted pass, before the solve)
        if constexpr (!MULTI) {
          if (!level_done && level == 0 && C.K >= 0 && it >= C.K) parked = true;
        }
      }
      __syncthreads();                               // the state, g_sT and g_sH are those of the accepted pass
      if (parked) break;
    } else {
      resume = false;
      level = g_ts.level;
    }
    if (level_done) {
      if (level == 0) break;
      if (tid == 0) enter_level(level - 1);
      if (tid >= 64 && tid < 76) g_pa.T[tid - 64] = g_sT[tid - 64];
    } else {                                       // the next trial: solve at the accepted pose, sweep at the trial pose into the other term buffer
      if (tid >= 64 && tid < 76) g_sTj[level][tid - 64] = g_sT[tid - 64];      // the reference's H,b pass of this iteration ran at the accepted pose
      if (tid < 64) track_solve_call();
      __syncthreads();
      if (tid < 12) g_pa.T[tid] = g_sTn[tid];
      if (tid == 12) { g_pa.t_buf = tb0 ? tb0 + (size_t)(g_ts.cur ^ 1) * G.terms_b : nullptr; g_ts.phase = 1; }
    }
    __syncthreads();
  }
  if constexpr (!MULTI) {
    if (parked) {
      TrkPark &P = C.park[slot];
      if (tid == 0) { P.ts = g_ts; C.list[atomicAdd(C.count, 1u)] = slot; }
      if (tid < 12) P.T[tid] = g_sT[tid];
      if (tid >= 64 && tid < 64 + 27) P.H[tid - 64] = g_sH[tid - 64];
      if (tid >= 128 && tid < 128 + 36) P.Tj[tid - 128] = g_sTj[(tid - 128) / 12][(tid - 128) % 12];
      return;
    }
  }
  if (wg != 0) return;
  if (failed) { if (tid == 0 && passes_out) passes_out[slot] = -1; return; }      // (MULTI: a sibling never arrived) pose left as it came in
  if (tid < 12) T_io[(size_t)slot * 12 + tid] = g_sT[tid];
  if (tid == 0 && passes_out) passes_out[slot] = g_ts.passes;
  if (tid == 0 && A.n_rec) A.n_rec[slot] = g_ts.n_rec;
  if (tid == 0 && G.work16) G.work16[slot] = g_ts.work16;
  if (A.T_jac && tid < 36) A.T_jac[(size_t)slot * 36 + tid] = g_sTj[tid / 12][tid % 12];
  if (tid == 0 && G.seq_stats && g_ts.n_exact) {
    atomicAdd(G.seq_stats, g_ts.n_exact);
    if (g_seq_sh.fell_back) atomicAdd(G.seq_stats + 1, 1u);
  }
}
// (four waves per SIMD: 128 VGPRs, two 512-lane workgroups per CU)
template <bool U8SRC, bool BAL, int CONT>      // CONT 0: first launch (BAL: grid order from the table); 1: the continuation (grid = CONT_MAX_NWG x groups: launch_batch_tracker)
__global__ __launch_bounds__(TRK_THREADS, 4) void dense_track_batch_kernel(TrackArgs A, double *__restrict__ T_io, int *__restrict__ passes_out, TrackMulti G, TrackCont C) {
  if constexpr (CONT == 0) {
    int slot = blockIdx.x;
    if constexpr (BAL) {
      const int e = G.map[blockIdx.x];
      if (e < 0) return;      // (the table is device memory this kernel does not own)
      slot = e >> 4;
    }
    track_batch_stream<U8SRC, false>(A, T_io, passes_out, G, C, slot, 0, 1);
  } else {
    // every parked stream gets CONT_MAX_NWG workgroups, whatever else parked: the split of its sweeps, and so the order its partial sums are added in, is that of the
    // stream alone.  Group y of siblings (the CONT_MAX_NWG workgroups of grid row y, neighbours in the dispatch order) resumes list entries y, y + groups, ...
    const int n_parked = (int)*C.count;
    for (int p = blockIdx.y; p < n_parked; p += gridDim.y) {
      track_batch_stream<U8SRC, true>(A, T_io, passes_out, G, C, C.list[p], blockIdx.x, CONT_MAX_NWG);
      __syncthreads();                             // (the next stream's state overwrites this one's in LDS)
    }
  }
}

// DenseTracker::residual_img[level] (dense_tracking.cpp:279-329): the GUI image an H,b pass at pose T leaves behind.
// Green = no depth, red = projects out of frame, grey = 1 - 50 res^2 of the clamped residual.
template <bool U8SRC>
__global__ __launch_bounds__(256) void residual_image_cpu_sem_kernel(LevelArgs L, size_t cloud_b, size_t prev_b, size_t f_b, size_t c8_b,
                                                                     const double *__restrict__ Tarr, size_t T_b,
                                                                     float *__restrict__ rimg, size_t rimg_b) {
  const int slot = blockIdx.y;
  const int cw = L.cam.w / 4, ch = L.cam.h / 4;
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= cw * ch) return;
  L.cloud += slot * cloud_b; L.prev += slot * prev_b;
  if (U8SRC) L.cur8 += slot * c8_b; else L.cur += slot * f_b;
  double T[12];
#pragma unroll
  for (int k = 0; k < 12; ++k) T[k] = Tarr[(size_t)slot * T_b + k];
  const int u = i % cw, v = i / cw;
  const float4 c4 = reinterpret_cast<const float4 *>(L.cloud)[i];
  float4 o = make_float4(0.f, 1.f, 0.f, 1.f);
  if (c4.w > 0) {
    const double xp0 = c4.x, xp1 = c4.y, xp2 = c4.z;
    double x, y, z;
    pose_act(T, xp0, xp1, xp2, x, y, z);
    const float uvx = (float)(L.cam.f * (x / z) + L.cam.cx);
    const float uvy = (float)(L.cam.f * (y / z) + L.cam.cy);
    bool ok = fabsf(uvx) < 1e9f && fabsf(uvy) < 1e9f;
    const int ui = ok ? (int)uvx : 0, vi = ok ? (int)uvy : 0;
    ok = ok && (ui >= 2 && vi >= 2 && ui < L.cam.w - 2 && vi < L.cam.h - 2);
    o = make_float4(1.f, 0.f, 0.f, 1.f);
    if (ok) {
      const float ip = (float)((1. / 255.) * L.prev[(size_t)(v * 4) * L.pstride + u * 4]);
      float ic, gx, gy;
      if (U8SRC) taps_u8(L.cur8, L.c8stride, uvx, uvy, ic, gx, gy);
      else ic = interp32f(L.cur, L.fstride, uvx, uvy);
      float res = ip - ic;
      if (res > 0.1) res = 0.1;
      if (res < -0.1) res = -0.1;
      float g = 1 - 50.f * res * res;
      if (g < 0.f) g = 0.f;
      o = make_float4(g, g, g, 1.f);
    }
  }
  reinterpret_cast<float4 *>(rimg + slot * rimg_b)[i] = o;
}


}  // namespace


// the sample offsets are formed with 24-bit multiplies (sample_load, taps_u8_issue): rows, columns and row strides of a level stay below 2^24
static bool offsets_fit_24(const svs_cam &cam, int pstride, int c8stride) {
  const int lim = 1 << 24;
  return cam.w > 0 && cam.h > 0 && cam.w < lim && cam.h < lim && pstride >= 0 && pstride < lim && c8stride >= 0 && c8stride < lim;
}
static int ensure_scratch(svs_ctx *ctx, double **p, size_t count) {      // ctx-owned (common.h)
  void *v = nullptr;
  const int rc = svs_ctx_scratch(ctx, count * sizeof(double), &v);
  *p = static_cast<double *>(v);
  return rc;
}


extern "C" int svs_dense_pass_cpu_sem(svs_ctx *ctx, const float *d_cloud, size_t cloud_bstride, const uint8_t *d_prev_u8,
                                      int pstride, size_t p_bstride, const float *d_cur, const float *d_dx,
                                      const float *d_dy, int fstride, size_t f_bstride, const svs_cam *cam,
                                      const double *d_T, int do_jac, svs_dense_sums *d_out, int batch) {
  SVS_REQUIRE(ctx, ctx && d_cloud && d_prev_u8 && d_cur && cam && d_T && d_out && batch >= 1);
  SVS_DEVICE(ctx);
  SVS_REQUIRE(ctx, !do_jac || (d_dx && d_dy));
  SVS_REQUIRE(ctx, cam->w % 4 == 0 && cam->h % 4 == 0);
  SVS_REQUIRE(ctx, offsets_fit_24(*cam, pstride, 0));
  LevelArgs L{d_cloud, d_prev_u8, d_cur, d_dx, d_dy, pstride, fstride, *cam, nullptr, 0};
  int n = (cam->w / 4) * (cam->h / 4);
  int nblocks = std::min(div_up(n, 256), 256);
  double *part = nullptr;
  int rc = ensure_scratch(ctx, &part, (size_t)batch * nblocks * (NSUM + 1));
  if (rc) return rc;
  if (do_jac)
    hipLaunchKernelGGL(dense_pass_cpu_sem_kernel<true>, dim3(nblocks, batch), dim3(256), 0, ctx->stream, L, cloud_bstride, p_bstride, f_bstride, d_T, part);
  else
    hipLaunchKernelGGL(dense_pass_cpu_sem_kernel<false>, dim3(nblocks, batch), dim3(256), 0, ctx->stream, L, cloud_bstride, p_bstride, f_bstride, d_T, part);
  SVS_LAUNCH_CHECK(ctx);
  hipLaunchKernelGGL(dense_finalize_kernel, dim3(batch), dim3(64), 0, ctx->stream, part, nblocks, d_out);
  SVS_LAUNCH_CHECK(ctx);
  return SVS_OK;
}

namespace {
// "trk_balance": the grid order of the next frame's ordered launch (one workgroup, B <= 4096 streams): the streams by decreasing LM work of this frame, ties by
// index.  All streams of a big batch are resident at once (two workgroups per CU) and the launch lasts as long as its longest stream; the shortest streams start
// last, in the slots the first finishers leave.  work16 [B]: each stream's work in 1/16 level-0 sweeps, left by the flat tracker kernel (all zero: stream order).
// map [B]: position in the grid -> (stream << 4), the encoding motion.hip's tail and svs_dense_track_balance_order read
constexpr int BAL_MAX_STREAMS = 4096;
constexpr int ASSIGN_THREADS = 1024;
__global__ __launch_bounds__(ASSIGN_THREADS) void trk_assign_kernel(const int *__restrict__ work16, int B, int *__restrict__ map) {
  // the position of a stream = its rank by (work descending, index ascending) = the number of keys greater than its own; keys = work << 12 | (4095 - index),
  // packed in LDS and compared four per read (the padding is below every key, so a position stays below B whatever the words hold)
  __shared__ __attribute__((aligned(16))) int s_key[BAL_MAX_STREAMS];
  const int tid = threadIdx.x;
  const int Bp = (B + 3) & ~3;
  for (int b = tid; b < Bp; b += ASSIGN_THREADS) s_key[b] = b < B ? (work16[b] << 12) | (4095 - b) : INT_MIN;
  __syncthreads();
  for (int b = tid; b < B; b += ASSIGN_THREADS) {
    const int mine = s_key[b];
    int pos = 0;
    for (int k = 0; k < Bp; k += 4) {
      const int4 q = *reinterpret_cast<const int4 *>(s_key + k);
      pos += (q.x > mine) + (q.y > mine) + (q.z > mine) + (q.w > mine);
    }
    map[pos] = b << 4;
  }
}

// scratch of the continuation launch (dense_track_batch_kernel<., ., 1>): partial sums of the shared sweeps, arrival counters + failure flags, decision words, the
// parked states and their list.  Returns G / C filled in; enqueues the memset of the words that must start at zero.
static int cont_setup(svs_ctx *ctx, int batch, TrackMulti &G, TrackCont &C) {
  const size_t n_part = (size_t)batch * 2 * CONT_MAX_NWG * 32, n_bar = (size_t)batch, n_bc = (size_t)batch * 16, n_cnt = 2, n_list = (size_t)batch / 2 + 1;
  const size_t n_park = ((size_t)batch * sizeof(TrkPark) + 7) / 8;
  double *scr = nullptr;
  const int rc = ensure_scratch(ctx, &scr, n_part + n_bar + n_bc + n_cnt + n_list + n_park);
  if (rc) return rc;
  G.part = scr;
  G.bar = reinterpret_cast<unsigned *>(scr + n_part);
  G.fail_off = batch;
  G.bcast = scr + n_part + n_bar;
  C.count = reinterpret_cast<unsigned *>(scr + n_part + n_bar + n_bc);
  C.list = reinterpret_cast<int *>(scr + n_part + n_bar + n_bc + n_cnt);
  C.park = reinterpret_cast<TrkPark *>(scr + n_part + n_bar + n_bc + n_cnt + n_list);
  C.K = ctx->trk_split; C.slots = ctx->trk_cont_slots > 0 ? ctx->trk_cont_slots : 2 * ctx->n_cu;
  SVS_HIP(ctx, hipMemsetAsync(G.bar, 0, sizeof(double) * (n_bar + n_bc + n_cnt), ctx->stream));
  return SVS_OK;
}
// a tracker kernel for the source of the current image (u8src: the u8 level images, else the f32 pyramids): K<true, ...> or K<false, ...>, both from ONE list of the
// remaining template arguments (in parentheses) and ONE argument list; TRK_THREADS lanes per workgroup, on the context's stream
#define TRK_ARGS(...) __VA_ARGS__
#define TRK_LAUNCH(u8src, K, TAIL, grid, ...)                                                                              \
  do {                                                                                                                     \
    if (u8src) hipLaunchKernelGGL((K<true, TRK_ARGS TAIL>), grid, dim3(TRK_THREADS), 0, ctx->stream, __VA_ARGS__);         \
    else hipLaunchKernelGGL((K<false, TRK_ARGS TAIL>), grid, dim3(TRK_THREADS), 0, ctx->stream, __VA_ARGS__);              \
  } while (0)
// the first launch of a big batch (one workgroup per stream; BAL: in the order of G.map) and, with "trk_split", its continuation
template <bool BAL>
static int launch_batch_tracker(svs_ctx *ctx, const TrackArgs &A, bool u8src, double *d_T_io, int32_t *d_passes_out, int batch, TrackMulti G) {
  TrackCont C{nullptr, nullptr, nullptr, -1, 0};
  if (ctx->trk_split > 0) { const int rc = cont_setup(ctx, batch, G, C); if (rc) return rc; }
  TRK_LAUNCH(u8src, dense_track_batch_kernel, (BAL, 0), dim3(batch), A, d_T_io, d_passes_out, G, C);
  SVS_LAUNCH_CHECK(ctx);
  if (C.K < 0) return SVS_OK;
  // the parked streams, CONT_MAX_NWG workgroups each: they wait for each other inside the launch -- through the spin gate like every launch of that kind (common.h).
  // groups x CONT_MAX_NWG <= slots workgroups: all resident together, so every sibling a workgroup waits for is running (and a wait is only ever on a sibling)
  const int groups = std::max(1, std::min(batch, C.slots / CONT_MAX_NWG));
  SvsSpinScope gate(ctx);
  if (gate.rc) return gate.rc;
  TRK_LAUNCH(u8src, dense_track_batch_kernel, (false, 1), dim3(CONT_MAX_NWG, groups), A, d_T_io, d_passes_out, G, C);
  SVS_LAUNCH_CHECK(ctx);
  return gate.leave();
}
// the ordered launch of a big batch.  State (owned by the caller, frontend.hip; persistent from frame to frame): the grid order [batch] i32 | each stream's LM work
// of the last frame [batch] i32 (written by the flat tracker kernel), each padded to 256 bytes.  The order for the NEXT frame is made right behind this frame's
// tracker, so that nothing small sits between the fork of the side stream and the tracker's launch.
struct BalState { int *map, *work16; };
size_t bal_row_bytes(int batch) { return (sizeof(int) * (size_t)batch + 255) & ~(size_t)255; }
BalState bal_state(void *state, int batch) {
  char *p = static_cast<char *>(state);
  return BalState{reinterpret_cast<int *>(p), reinterpret_cast<int *>(p + bal_row_bytes(batch))};
}
int bal_assign(svs_ctx *ctx, const BalState &S, int batch) {
  hipLaunchKernelGGL(trk_assign_kernel, dim3(1), dim3(ASSIGN_THREADS), 0, ctx->stream, S.work16, batch, S.map);
  SVS_LAUNCH_CHECK(ctx);
  return SVS_OK;
}
int svs_dense_track_cpu_sem_balanced(svs_ctx *ctx, const TrackArgs &A, bool u8src, double *d_T_io, int32_t *d_passes_out, int batch, void *state, TrackMulti G) {
  const BalState S = bal_state(state, batch);
  G.map = S.map; G.work16 = S.work16;
  if (int rc = launch_batch_tracker<true>(ctx, A, u8src, d_T_io, d_passes_out, batch, G)) return rc;
  return bal_assign(ctx, S, batch);
}
}  // namespace
// the grid order the ordered launch will use for the next tracker launch, as (stream << 4) entries: a permutation of the streams
const int *svs_dense_track_balance_order(svs_ctx *ctx, void *state, int batch) {
  return state && ctx->trk_balance ? bal_state(state, batch).map : nullptr;
}
size_t svs_dense_track_balance_bytes(int batch) { return 2 * bal_row_bytes(batch); }
// zero history: streams in index order
int svs_dense_track_balance_init(svs_ctx *ctx, void *state, int batch) {
  SVS_REQUIRE(ctx, ctx && state && batch >= 1 && batch <= BAL_MAX_STREAMS);
  SVS_DEVICE(ctx);
  SVS_HIP(ctx, hipMemsetAsync(state, 0, svs_dense_track_balance_bytes(batch), ctx->stream));
  return bal_assign(ctx, bal_state(state, batch), batch);
}
extern "C" int svs_dense_track_cpu_sem(svs_ctx *ctx, const svs_dense_track_args *a, double *d_T_io, int32_t *d_passes_out,
                                       int batch) {
  return svs_dense_track_cpu_sem_work(ctx, a, d_T_io, d_passes_out, batch, nullptr);
}
// d_bal_state != NULL (frontend.hip; svs_dense_track_balance_bytes / _init): the balanced launch of big batches
int svs_dense_track_cpu_sem_work(svs_ctx *ctx, const svs_dense_track_args *a, double *d_T_io, int32_t *d_passes_out, int batch, void *d_bal_state) {
  SVS_REQUIRE(ctx, ctx && a && d_T_io && batch >= 1);
  SVS_DEVICE(ctx);
  TrackArgs A;
  const bool u8src = a->d_cur_u8[0] != nullptr;
  for (int l = 0; l < 3; ++l) {
    SVS_REQUIRE(ctx, a->d_cloud[l] && a->d_prev_u8[l]);
    SVS_REQUIRE(ctx, u8src ? a->d_cur_u8[l] != nullptr : (a->d_cur[l] && a->d_dx[l] && a->d_dy[l]));
    SVS_REQUIRE(ctx, a->cam_vec[l].w % 4 == 0 && a->cam_vec[l].h % 4 == 0);
    SVS_REQUIRE(ctx, offsets_fit_24(a->cam_vec[l], a->pstride[l], u8src ? a->c8stride[l] : 0));
    A.lv[l] = LevelArgs{a->d_cloud[l], a->d_prev_u8[l], a->d_cur[l], a->d_dx[l], a->d_dy[l], a->pstride[l], a->fstride[l], a->cam_vec[l],
                        a->d_cur_u8[l], a->c8stride[l]};
    A.cloud_b[l] = a->cloud_bstride[l]; A.prev_b[l] = a->p_bstride[l]; A.f_b[l] = a->f_bstride[l]; A.c8_b[l] = a->c8_bstride[l];
  }
  A.T_jac = a->d_T_jac_out;
  A.rec = a->d_record_out; A.rec_cap = a->d_record_out ? a->record_cap : 0; A.n_rec = a->d_n_record_out;
  SVS_REQUIRE(ctx, !a->d_record_out || a->record_cap > 0);
  // latency mode: with few streams, NW workgroups share each stream's sweeps (they must all be resident: NW * batch <= 128 CUs)
  // workgroups per stream in latency mode.  Round 3 (exchange without a device-wide fence, coarsest level on one workgroup), B = 1:
  // 2 -> 0.211, 4 -> 0.165, 8 -> 0.160, 16 -> 0.184 ms per frame; round 2 (fence per sweep): 4 -> 0.26, 8 -> 0.26, 16 -> 0.28, 1 -> 0.34 ms
  int nwg = batch <= 16 ? 8 : (batch <= 32 ? 4 : 1);
  if (ctx->trk_nwg) nwg = ctx->trk_nwg;
  float *t_buf = nullptr; size_t t_b = 0;
  // the float terms of the passes (dense_tracking.cpp:229-262: `chi2 += res * res`).  "trk_seq_chi2": one buffer per stream, every sum by the sequential chain, one
  // workgroup per stream.  Default ("trk_lazy_chi2"): two buffers per stream, read only where the f64 sums cannot decide the accept test (seqsum.h)
  const bool seq_all = ctx->trk_seq_chi2 != 0, lazy = !seq_all && ctx->trk_lazy_chi2 != 0;
  float *terms = nullptr;
  if (seq_all || lazy) {
    if (seq_all) nwg = 1;
    t_b = (size_t)(a->cam_vec[0].w / 4) * (a->cam_vec[0].h / 4);
    if (lazy) t_b = ((t_b + 3) & ~(size_t)3) + 64;      // 16-byte aligned buffers, padded by more than the longest run a lane reads in one go (SEQ_RUN_MAX)
    const size_t want = (size_t)batch * t_b * sizeof(float) * (lazy ? 2 : 1) + 256;
    if (ctx->seq_buf.bytes() < want) {
      if (ctx->seq_buf) SVS_HIP(ctx, hipStreamSynchronize(ctx->stream));
      SVS_HIP(ctx, ctx->seq_buf.reserve(want, want));
    }
    if (seq_all) t_buf = static_cast<float *>(ctx->seq_buf.get()); else terms = static_cast<float *>(ctx->seq_buf.get());
    if (!ctx->seq_stats) {
      SVS_HIP(ctx, ctx->seq_stats.alloc_bytes(256));
      SVS_HIP(ctx, hipMemsetAsync(ctx->seq_stats, 0, 256, ctx->stream));
    }
  }
  TrackMulti G{};
  G.terms = terms; G.terms_b = t_b; G.seq_stats = ctx->seq_stats; G.terms_only = ctx->trk_lazy_chi2 == 2;
  // the form of the launch.  SeqChain: "trk_seq_chi2"; Latency: nwg workgroups share each stream's sweeps; BigOrdered / Big: the flat kernel, two workgroups
  // per CU, in the order of the last frame's LM work where the front end keeps that state and records ("trk_regs" = 2 asks for the flat kernel at any batch
  // size, 1 for the nested-loop kernel: tests / experiments); OnePerCu: the nested-loop kernel, one workgroup per stream
  enum class Form { SeqChain, Latency, BigOrdered, Big, OnePerCu };
  const bool ordered = d_bal_state && ctx->trk_balance && batch >= 2 * ctx->n_cu && batch <= BAL_MAX_STREAMS && A.rec && A.n_rec;
  const bool big = (batch > ctx->n_cu && ctx->trk_regs != 1) || ctx->trk_regs == 2;
  const Form form = t_buf ? Form::SeqChain : nwg >= 2 ? Form::Latency : ordered ? Form::BigOrdered : big ? Form::Big : Form::OnePerCu;
  switch (form) {
    case Form::SeqChain:
      G.part = reinterpret_cast<double *>(t_buf); G.fail_off = (int)t_b;
      TRK_LAUNCH(u8src, dense_track_cpu_sem_kernel, (false, true), dim3(batch), A, d_T_io, d_passes_out, G);
      break;
    case Form::Latency: {
      double *scratch = nullptr;
      const size_t n_part = (size_t)batch * 2 * nwg * 64;      // per stream, parity and workgroup: 58 (+ 6) flagged 8-byte words (all_workgroups)
      // (the cleared size rounded up to 64 bytes: a clear whose size is no multiple of 16 bytes is TWO fill kernels in the runtime -- an aligned bulk and a tail --
      //  and in latency mode every launch in front of the tracker is on the frame's critical path)
      const size_t n_clear = (n_part + (size_t)batch + (size_t)batch * 16 + 7) & ~(size_t)7;
      int rc = ensure_scratch(ctx, &scratch, n_clear);      // + one counter word and one failure flag (4 + 4 bytes) per stream + the hand-over words
      if (rc) return rc;
      G.part = scratch;
      G.bar = reinterpret_cast<unsigned *>(scratch + n_part);
      G.fail_off = batch;
      G.bcast = scratch + n_part + (size_t)batch;
      SVS_HIP(ctx, hipMemsetAsync(scratch, 0, sizeof(double) * n_clear, ctx->stream));      // flagged words, failure flags, hand-over words: one clear
      SvsSpinScope gate(ctx, nwg * batch);      // the workgroups of a stream wait for each other: one such launch on the device at a time (common.h); one stream: priority lane
      if (gate.rc) return gate.rc;
      TRK_LAUNCH(u8src, dense_track_cpu_sem_kernel, (true), dim3(nwg, batch), A, d_T_io, d_passes_out, G);
      SVS_LAUNCH_CHECK(ctx);
      if (int grc = gate.leave()) return grc;
      break;
    }
    case Form::BigOrdered: return svs_dense_track_cpu_sem_balanced(ctx, A, u8src, d_T_io, d_passes_out, batch, d_bal_state, G);
    case Form::Big: return launch_batch_tracker<false>(ctx, A, u8src, d_T_io, d_passes_out, batch, G);
    case Form::OnePerCu:
      TRK_LAUNCH(u8src, dense_track_cpu_sem_kernel, (false), dim3(batch), A, d_T_io, d_passes_out, G);
      break;
  }
  SVS_LAUNCH_CHECK(ctx);
  return SVS_OK;
}

// diagnostic: the sum of the reference's `float chi2 += t[i]` over batch rows of n terms, formed (how = 0) as the tracker's accept test forms it (exact_seq_sum_f32),
// (how = 1) the same with the terms read past the caches as the latency-mode tracker reads them, (how = 2) by the literal sequential chain
namespace {
template <int HOW>
__global__ __launch_bounds__(TRK_THREADS) void seq_sum_probe_kernel(const float *__restrict__ t, int n, size_t bstride, float *__restrict__ out, int *__restrict__ fell_back) {
  if (threadIdx.x == 0) g_seq_sh.fell_back = 0;
  __syncthreads();
  const float *row = t + (size_t)blockIdx.x * bstride;
  float v;
  if constexpr (HOW == 2) v = seq_chi2_f32(row, n); else v = exact_seq_sum_f32<HOW == 1>(row, n);
  if (threadIdx.x == 0) { out[blockIdx.x] = v; if (fell_back) fell_back[blockIdx.x] = HOW == 2 ? 1 : g_seq_sh.fell_back; }
}
}  // namespace
extern "C" int svs_dense_seq_sum_f32(svs_ctx *ctx, const float *d_terms, int n, size_t bstride, int batch, int how, float *d_out, int32_t *d_fell_back) {
  SVS_REQUIRE(ctx, ctx && d_terms && d_out && n >= 0 && batch >= 1 && how >= 0 && how <= 2);
  SVS_DEVICE(ctx);
  if (how == 0) hipLaunchKernelGGL(seq_sum_probe_kernel<0>, dim3(batch), dim3(TRK_THREADS), 0, ctx->stream, d_terms, n, bstride, d_out, d_fell_back);
  else if (how == 1) hipLaunchKernelGGL(seq_sum_probe_kernel<1>, dim3(batch), dim3(TRK_THREADS), 0, ctx->stream, d_terms, n, bstride, d_out, d_fell_back);
  else hipLaunchKernelGGL(seq_sum_probe_kernel<2>, dim3(batch), dim3(TRK_THREADS), 0, ctx->stream, d_terms, n, bstride, d_out, d_fell_back);
  SVS_LAUNCH_CHECK(ctx);
  return SVS_OK;
}

extern "C" int svs_dense_residual_image_cpu_sem(svs_ctx *ctx, const float *d_cloud, size_t cloud_bstride, const uint8_t *d_prev_u8,
                                                int pstride, size_t p_bstride, const float *d_cur, int fstride, size_t f_bstride,
                                                const uint8_t *d_cur_u8, int c8stride, size_t c8_bstride, const svs_cam *cam,
                                                const double *d_T, size_t T_bstride, float *d_res_img4, size_t res_bstride, int batch) {
  SVS_REQUIRE(ctx, ctx && d_cloud && d_prev_u8 && (d_cur || d_cur_u8) && cam && d_T && d_res_img4 && batch >= 1);
  SVS_DEVICE(ctx);
  SVS_REQUIRE(ctx, cam->w % 4 == 0 && cam->h % 4 == 0);
  SVS_REQUIRE(ctx, offsets_fit_24(*cam, pstride, d_cur_u8 ? c8stride : 0));
  LevelArgs L{d_cloud, d_prev_u8, d_cur, nullptr, nullptr, pstride, fstride, *cam, d_cur_u8, c8stride};
  const int n = (cam->w / 4) * (cam->h / 4);
  if (d_cur_u8)
    hipLaunchKernelGGL(residual_image_cpu_sem_kernel<true>, dim3(div_up(n, 256), batch), dim3(256), 0, ctx->stream, L, cloud_bstride, p_bstride,
                       f_bstride, c8_bstride, d_T, T_bstride, d_res_img4, res_bstride);
  else
    hipLaunchKernelGGL(residual_image_cpu_sem_kernel<false>, dim3(div_up(n, 256), batch), dim3(256), 0, ctx->stream, L, cloud_bstride, p_bstride,
                       f_bstride, c8_bstride, d_T, T_bstride, d_res_img4, res_bstride);
  SVS_LAUNCH_CHECK(ctx);
  return SVS_OK;
}
