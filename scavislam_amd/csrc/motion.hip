// motion.hip -- what the front end does to a frame behind the guided matcher, for gfx950: motion-only pose refinement
// (PoseOptimizer::calcFastMotionOnly), the reprojection gate of StereoFrontend::processMatchedPoints and the dense point clouds of the
// new pose (DenseTracker::computeDensePointCloudCpu, dense_tracking.cpp:393-423) -- each as a launch of its own, and all three fused in
// ONE launch per frame batch (motion_only_fused_kernel<true>: gate and clouds as the tail of a stream's refinement workgroup).
// The fused tail and the stand-alone kernels share their device functions (gate_stream, cloud_TQ, cloud_disp, cloud_point): identical bits.
#include "common.h"
#include "gate.h"
#include "lm6.h"
#include "pose.h"
#include <algorithm>

namespace {

// ---- the dense point cloud ------------------------------------------------------------------------------------
// computeDensePointCloudCpu (dense_tracking.cpp:393-423)
// TQ = [Ti;0 0 0 1] * Q, Ti = inverse of the pose, Q = [1 0 0 -cx; 0 1 0 -cy; 0 0 0 f; 0 0 1/b 0] (stereo_camera.cpp:24-34), evaluated with the same term order
// as a dense 4x4 product
__device__ __forceinline__ void cloud_TQ(const double (&T)[12], const svs_cam &cam, double (&TQ)[16]) {
  double Ti[12];
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int c = 0; c < 3; ++c) Ti[4 * r + c] = T[4 * c + r];
#pragma unroll
  for (int r = 0; r < 3; ++r) Ti[4 * r + 3] = -(Ti[4 * r] * T[3] + Ti[4 * r + 1] * T[7] + Ti[4 * r + 2] * T[11]);
  const double Q[16] = {1, 0, 0, -cam.cx, 0, 1, 0, -cam.cy, 0, 0, 0, cam.f, 0, 0, 1.0 / cam.b, 0};
#pragma unroll
  for (int r = 0; r < 4; ++r)
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      double s = 0;
#pragma unroll
      for (int k = 0; k < 4; ++k) { double tik = r < 3 ? Ti[4 * r + k] : (k == 3 ? 1.0 : 0.0); s += tik * Q[4 * k + c]; }
      TQ[4 * r + c] = s;
    }
}
// quarter-grid sample (u, v) of one stream's level: disp = the stream's level-0 disparity image.  The load and the arithmetic are two functions so that the fused
// tail can request the disparities of later samples before it works on this one; every caller runs these two: identical bits.
__device__ __forceinline__ float cloud_disp(const float *__restrict__ disp, int ds, int level, int u, int v) {
  return disp[(size_t)((v * 4) << level) * ds + ((u * 4) << level)];
}
__device__ __forceinline__ float4 cloud_point(float disp_uv, int level, const double (&TQ)[16], int u, int v) {
  const double inv_factor = 1.0 / (double)(1 << level);
  const float d = (float)(disp_uv * inv_factor);
  if (d <= 0) return make_float4(0.f, 0.f, 0.f, -1.f);
  const double q[4] = {(double)(u * 4), (double)(v * 4), (double)d, 1.0};
  double r[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) r[k] = TQ[4 * k] * q[0] + TQ[4 * k + 1] * q[1] + TQ[4 * k + 2] * q[2] + TQ[4 * k + 3] * q[3];
  // r[0] / r[3], r[1] / r[3], r[2] / r[3]: one reciprocal and three exact quotients (devutil.h: the bits of the three divisions, 19 f64 instructions instead of 3 x 13)
  const double num[3] = {r[0], r[1], r[2]};
  double p[3];
  div_rn_guarded(num, r[3], p);
  return make_float4((float)p[0], (float)p[1], (float)p[2], 1.f);
}
// sample i = v cw + u of the level (the stand-alone kernels: one sample per lane, one division per lane)
__device__ __forceinline__ void cloud_sample(const float *__restrict__ disp, int ds, int cw, int level, const double (&TQ)[16], int i, float *__restrict__ cloud) {
  const int v = i / cw, u = i - v * cw;
  reinterpret_cast<float4 *>(cloud)[i] = cloud_point(cloud_disp(disp, ds, level, u, v), level, TQ, u, v);
}
// One level of one stream's cloud by the NT lanes of its workgroup (the fused tail).  A lane's samples are NT apart: their grid position is carried from trip to trip
// (one division per lane and level), and the disparities of the next PF samples are in flight while this one's point is formed -- the stream's disparity image
// is in no cache, and with one load per trip and nothing beside it every trip waited a whole memory round trip.
constexpr int CLOUD_PF = 4;      // as measured (profiles/refinement_tail.md: 2, 4 and 8 are within each other's spread; the tail is then bound by the device's memory traffic)
template <int NT, int PF>
__device__ __forceinline__ void cloud_level_sweep(const float *__restrict__ disp, int ds, const svs_cam &cam, int level, const double (&TQ)[16], float *__restrict__ cloud,
                                                  int tid) {
  const int cw = cam.w / 4, n_px = cw * (cam.h / 4);
  const int sv = NT / cw, su = NT - sv * cw;                 // one trip further: (u + su, v + sv), one carry at most (su < cw)
  int v = tid / cw, u = tid - v * cw;                        // the sample this trip works on
  int pv = v, pu = u, pi = tid;                              // the sample whose disparity is requested next: PF trips ahead
  float ahead[PF];
#pragma unroll
  for (int k = 0; k < PF; ++k) {
    const bool in = pi < n_px;
    ahead[k] = cloud_disp(disp, ds, level, in ? pu : 0, in ? pv : 0);
    pu += su; pv += sv; pi += NT;
    if (pu >= cw) { pu -= cw; ++pv; }
  }
  for (int i = tid; i < n_px; i += PF * NT) {
#pragma unroll
    for (int k = 0; k < PF; ++k) {
      const float d = ahead[k];
      const bool in = pi < n_px;
      ahead[k] = cloud_disp(disp, ds, level, in ? pu : 0, in ? pv : 0);      // (past the end: the image's first sample, never used)
      pu += su; pv += sv; pi += NT;
      if (pu >= cw) { pu -= cw; ++pv; }
      if (i + k * NT < n_px) reinterpret_cast<float4 *>(cloud)[i + k * NT] = cloud_point(d, level, TQ, u, v);
      u += su; v += sv;
      if (u >= cw) { u -= cw; ++v; }
    }
  }
}
__global__ __launch_bounds__(256) void pointcloud_cpu_sem_kernel(const float *__restrict__ disp, int ds, size_t disp_b, svs_cam cam,
                                                                 int level, const double *__restrict__ Tarr,
                                                                 float *__restrict__ cloud, size_t cloud_b) {
  const int slot = blockIdx.y;
  const int cw = cam.w / 4, ch = cam.h / 4;
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= cw * ch) return;
  double T[12], TQ[16];
#pragma unroll
  for (int k = 0; k < 12; ++k) T[k] = Tarr[(size_t)slot * 12 + k];
  cloud_TQ(T, cam, TQ);
  cloud_sample(disp + slot * disp_b, ds, cw, level, TQ, i, cloud + slot * cloud_b);
}

// the three levels' clouds of a frame in ONE launch (latency mode: three launches of 75 / 19 / 5 blocks each paid a launch gap); the same per-sample function: identical bits
struct CloudLevels { svs_cam cam[3]; float *cloud[3]; size_t cloud_b[3]; int blocks[3]; };
__global__ __launch_bounds__(256) void pointcloud_cpu_sem_levels_kernel(const float *__restrict__ disp, int ds, size_t disp_b, CloudLevels Q, const double *__restrict__ Tarr) {
  const int slot = blockIdx.y;
  int bx = blockIdx.x, level = 0;
  if (bx >= Q.blocks[0]) { bx -= Q.blocks[0]; level = 1; if (bx >= Q.blocks[1]) { bx -= Q.blocks[1]; level = 2; } }
  const svs_cam cam = level == 0 ? Q.cam[0] : (level == 1 ? Q.cam[1] : Q.cam[2]);
  float *cloud = level == 0 ? Q.cloud[0] : (level == 1 ? Q.cloud[1] : Q.cloud[2]);
  const size_t cloud_b = level == 0 ? Q.cloud_b[0] : (level == 1 ? Q.cloud_b[1] : Q.cloud_b[2]);
  const int cw = cam.w / 4, ch = cam.h / 4;
  const int i = bx * 256 + threadIdx.x;
  if (i >= cw * ch) return;
  double T[12], TQ[16];
#pragma unroll
  for (int k = 0; k < 12; ++k) T[k] = Tarr[(size_t)slot * 12 + k];
  cloud_TQ(T, cam, TQ);
  cloud_sample(disp + slot * disp_b, ds, cw, level, TQ, i, cloud + slot * cloud_b);
}

}  // namespace

// internal (frontend.hip): computeDensePointCloudCpu of all three levels, one launch
int svs_pointcloud_cpu_sem_levels(svs_ctx *ctx, const float *d_disp, int disp_stride, size_t disp_bstride, const svs_cam *cams, const double *d_T, float *const *d_cloud,
                                  const size_t *cloud_bstride, int batch) {
  SVS_REQUIRE(ctx, ctx && d_disp && cams && d_T && d_cloud && cloud_bstride && batch >= 1);
  SVS_DEVICE(ctx);
  CloudLevels Q;
  int total = 0;
  for (int l = 0; l < 3; ++l) {
    SVS_REQUIRE(ctx, cams[l].w % 4 == 0 && cams[l].h % 4 == 0 && d_cloud[l]);
    Q.cam[l] = cams[l]; Q.cloud[l] = d_cloud[l]; Q.cloud_b[l] = cloud_bstride[l];
    Q.blocks[l] = div_up((cams[l].w / 4) * (cams[l].h / 4), 256);
    total += Q.blocks[l];
  }
  hipLaunchKernelGGL(pointcloud_cpu_sem_levels_kernel, dim3(total, batch), dim3(256), 0, ctx->stream, d_disp, disp_stride, disp_bstride, Q, d_T);
  SVS_LAUNCH_CHECK(ctx);
  return SVS_OK;
}

extern "C" int svs_pointcloud_cpu_sem(svs_ctx *ctx, const float *d_disp, int disp_stride, size_t disp_bstride,
                                      const svs_cam *cam, int level, const double *d_T, float *d_cloud,
                                      size_t cloud_bstride, int batch) {
  SVS_REQUIRE(ctx, ctx && d_disp && cam && d_T && d_cloud && level >= 0 && level < 3 && batch >= 1);
  SVS_DEVICE(ctx);
  SVS_REQUIRE(ctx, cam->w % 4 == 0 && cam->h % 4 == 0);            // dense_tracking.cpp:45-46 asserts
  int n = (cam->w / 4) * (cam->h / 4);
  hipLaunchKernelGGL(pointcloud_cpu_sem_kernel, dim3(div_up(n, 256), batch), dim3(256), 0, ctx->stream, d_disp, disp_stride,
                     disp_bstride, *cam, level, d_T, d_cloud, cloud_bstride);
  SVS_LAUNCH_CHECK(ctx);
  return SVS_OK;
}

// ---- motion-only pose refinement: PoseOptimizer<SE3,6,IdObs<3>,3>::calcFastMotionOnly ---------------------------
// (pose_optimizer.h:134-298, called at stereo_frontend.cpp:1058-1063 right behind the guided matcher).  One workgroup
// per camera stream runs the whole LM loop on the device: observations are the status-OK entries of the matcher's
// result array (= TrackData::obs_list / point_list, in list order); every pass is a strided sweep over them with a
// wave-shuffle + LDS reduction of the 21 + 6 normal-equation sums (or chi2 / max error); one lane solves the 6x6 system.
namespace {

__device__ __forceinline__ double mo_kernel(double delta, double b) {      // pseudo-Huber cost, pose_optimizer.h:426-435
  const double a = fabs(delta);
  return a < b ? delta * delta : 2 * b * a - b * b;
}
// (mo_residual: gate.h)
__device__ __forceinline__ double mo_weighted_sq(double *f, int robust, double b) {
  if (robust) {
    const double nrm = fmax(1e-10, sqrt(f[0] * f[0] + f[1] * f[1] + f[2] * f[2]));
    const double w = sqrt(mo_kernel(nrm, b)) / nrm;
    f[0] *= w; f[1] *= w; f[2] *= w;
  }
  return f[0] * f[0] + f[1] * f[1] + f[2] * f[2];
}

constexpr int MO_THREADS = 256;
// block reduction of N doubles per thread: sums for k < n_sum, maxima for the rest.  Result in s_red[0..N) (all threads may read)
template <int N>
__device__ __forceinline__ void mo_reduce(double (&v)[N], int n_sum, double *s_red) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int k = 0; k < N; ++k) {
    double x = v[k];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { const double y = __shfl_xor(x, o, 64); x = k < n_sum ? x + y : fmax(x, y); }
    if (lane == 0) s_red[wave * N + k] = x;
  }
  __syncthreads();
  if (threadIdx.x < N) {
    const int k = threadIdx.x;
    double x = s_red[k];
    for (int w = 1; w < MO_THREADS / 64; ++w) x = k < n_sum ? x + s_red[w * N + k] : fmax(x, s_red[w * N + k]);
    s_red[(MO_THREADS / 64) * N + k] = x;
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < N; ++k) v[k] = s_red[(MO_THREADS / 64) * N + k];
  __syncthreads();
}

__global__ __launch_bounds__(MO_THREADS) void motion_only_kernel(const svs_match_result *__restrict__ res, int n, size_t res_bstride, svs_cam cam,
                                                                 svs_pose_opt_params prm, double *__restrict__ T_io, svs_pose_opt_stats *__restrict__ stats) {
  __shared__ double s_red[(MO_THREADS / 64 + 1) * 28];
  __shared__ double s_T[12], s_Tn[12], s_B[6];
  const int tid = threadIdx.x, slot = blockIdx.x;
  res += (size_t)slot * res_bstride;
  if (tid < 12) s_T[tid] = T_io[12 * slot + tid];
  __syncthreads();
  // initial residuals: chi2, max error, number of observations, max diag(J^T J)
  double chi2, max_err, mu, nu = 2;
  int num_obs;
  {
    double v[4] = {0, 0, 0, 0};      // chi2, num_obs | max_err, norm_max_A
    for (int i = tid; i < n; i += MO_THREADS) {
      if (res[i].status != 0) continue;
      double f[3], J[18];
      mo_residual<true>(s_T, res[i], cam, f, J);
#pragma unroll
      for (int c = 0; c < 6; ++c) v[3] = fmax(v[3], fabs(J[c] * J[c] + J[6 + c] * J[6 + c] + J[12 + c] * J[12 + c]));
      v[0] += mo_weighted_sq(f, prm.robust_kernel, prm.kernel_param);
      v[1] += 1.0;
      v[2] = fmax(v[2], fmax(fabs(f[0]), fmax(fabs(f[1]), fabs(f[2]))));
    }
    mo_reduce<4>(v, 2, s_red);
    chi2 = v[0]; num_obs = (int)v[1]; max_err = v[2];
    mu = prm.initial_mu == -1 ? prm.tau * v[3] : prm.initial_mu;
  }
  const double initial_chi2 = chi2;
  int status = num_obs == 0 ? 1 : (num_obs < prm.min_obs ? 3 : 0), trial = 0;
  bool stop = status != 0;
  for (int ig = 0; ig < prm.num_iter && !stop; ++ig) {
    double rho = 0;
    do {
      double v[27];      // 21 unique of sum J^T J (upper, row-major), 6 of sum J^T (w f)
#pragma unroll
      for (int k = 0; k < 27; ++k) v[k] = 0;
      for (int i = tid; i < n; i += MO_THREADS) {
        if (res[i].status != 0) continue;
        double f[3], J[18];
        mo_residual<true>(s_T, res[i], cam, f, J);
        mo_weighted_sq(f, prm.robust_kernel, prm.kernel_param);
        int k = 0;
#pragma unroll
        for (int r = 0; r < 6; ++r) {
#pragma unroll
          for (int c = r; c < 6; ++c) v[k++] += J[r] * J[c] + J[6 + r] * J[6 + c] + J[12 + r] * J[12 + c];
          v[21 + r] += J[r] * f[0] + J[6 + r] * f[1] + J[12 + r] * f[2];
        }
      }
      mo_reduce<27>(v, 27, s_red);
      if (tid == 0) {
        double A[36], B[6], delta[6];
        int k = 0;
        for (int r = 0; r < 6; ++r)
          for (int c = r; c < 6; ++c) { A[6 * r + c] = A[6 * c + r] = v[k++]; }
        for (int r = 0; r < 6; ++r) { A[7 * r] += mu; B[r] = -v[21 + r]; s_B[r] = B[r]; }
        d_solve6(A, B, delta);                                 // A.ldlt().solve(B)
        double Tn[12];
        d_se3_exp_mul(delta, s_T, Tn);                         // prediction.add: exp(delta) * T
        for (int i = 0; i < 12; ++i) s_Tn[i] = Tn[i];
      }
      __syncthreads();
      double w[2] = {0, 0};      // new chi2 | new max error
      for (int i = tid; i < n; i += MO_THREADS) {
        if (res[i].status != 0) continue;
        double f[3];
        mo_residual<false>(s_Tn, res[i], cam, f, nullptr);
        w[0] += mo_weighted_sq(f, prm.robust_kernel, prm.kernel_param);
        w[1] = fmax(w[1], fmax(fabs(f[0]), fmax(fabs(f[1]), fabs(f[2]))));
      }
      mo_reduce<2>(w, 1, s_red);
      const double new_chi2 = w[0];
      if (isnan(new_chi2)) { status = 2; stop = true; break; }      // the reference throws here
      rho = chi2 - new_chi2;
      if (rho > 0) {
        if (tid < 12) s_T[tid] = s_Tn[tid];
        chi2 = new_chi2; max_err = w[1];
        double bm = -1;
        for (int c = 0; c < 6; ++c) bm = fmax(bm, fabs(s_B[c]));
        stop = bm <= 1e-10;
        const double q = 2 * rho - 1, sc = 1 - q * q * q;
        mu *= fmax(1. / 3., sc);
        nu = 2.; trial = 0;
      } else {
        mu *= nu; nu *= 2.; ++trial;
        if (trial == 5) stop = true;
      }
      __syncthreads();
    } while (!(rho > 0 || stop));
  }
  if (tid < 12) T_io[12 * slot + tid] = s_T[tid];
  if (tid == 0) {
    svs_pose_opt_stats st;
    st.initial_chi2 = initial_chi2; st.chi2 = chi2; st.max_err = max_err; st.num_obs = num_obs; st.status = status;
    stats[slot] = st;
  }
}

// ---- the same loop, restructured for latency (round 3) ---------------------------------------------------------------------------
// The kernel above walks the matcher's record array (status test + 64-byte record from global memory per observation) twice per LM
// trial and solves on one lane: 202 us for ~850 observations at B = 1.  Here:
//  * the status-OK records are compacted ONCE (order-preserving: ballots + a wave prefix) into an index list in LDS, and every thread keeps
//    up to MO2_RC observations in registers for the whole loop (observations beyond MO2_RC * MO2_THREADS are re-read through the list);
//  * ONE sweep per LM trial: chi2 / max error at the trial pose and the normal equations at the same pose share their residuals, so the
//    reference's "new chi2" pass and the next iteration's J^T J pass are one (a rejected trial keeps the stored system and only re-damps);
//  * 28 sums per wave by recursive halving (32 exchanges instead of 168 butterflies), two block barriers per trial;
//  * the 6x6 solve runs on seven lanes of wave 0 (lane = column of [A + mu I | B], Gauss-Jordan with readlane broadcasts; the matrix is
//    symmetric positive definite, so no pivoting is needed where the reference's ldlt() pivots), exp(delta) * T on the same wave.
// Same LM schedule and stopping rules as pose_optimizer.h:134-298; sums in a different order and one reciprocal instead of five divisions
// per residual => the pose agrees with the oracle to ~1e-12 (test bar 1e-9).
// Round 5: 256 lanes and six observations per lane in registers (rounds 3-4: 512 and four).  The kernel needs ~235 vector registers whatever its width, i.e. two
// waves per SIMD: a 512-lane workgroup had a CU to itself and a batch of 512 streams ran as two rounds of a latency-bound loop (<= 15 dependent LM iterations, two
// barriers and a 6 x 6 solve on one wave each); two 256-lane workgroups share a CU and the serial parts of one stream hide behind the sweeps of the other:
// 0.32 -> 0.22 ms per 512 streams.
constexpr int MO2_THREADS = 256, MO2_RC = 6, MO2_WAVES = MO2_THREADS / 64;      // lanes per workgroup, observations per lane in registers: as measured in round 5 (above)
struct MoObs { double o[3], q[3]; };

template <bool FIRST, bool JAC = true>      // JAC = false: chi2 and max error only (the sweep of a trial that is expected to be rejected)
__device__ __forceinline__ void mo2_terms(const double (&T)[12], const MoObs &ob, const svs_cam &cam, int robust, double kb, double (&x)[32], double &max_err,
                                          double &max_diag) {
  static_assert(JAC || !FIRST, "the first sweep needs the Jacobian");
  const double *q = ob.q;
  double X, Y, Z;
  pose_act(T, q[0], q[1], q[2], X, Y, Z);
  const double fl = cam.f, iz = 1.0 / Z, fiz = fl * iz, Xb = X - cam.b;
  double f0 = ob.o[0] - (X * fiz + cam.cx), f1 = ob.o[1] - (Y * fiz + cam.cy), f2 = ob.o[2] - (Xb * fiz + cam.cx);
  // frameJac (transformations.h:424-447): rows (A 0 C yC zA-xC -yA), (0 A D -zA+yD -xD xA), (A 0 E yE zA-xE -yA) with A = -f/z, C = f x/z^2, ...
  const double A = -fiz, C = fiz * X * iz, D = fiz * Y * iz, E = fiz * Xb * iz;
  const double a3 = Y * C, a4 = Z * A - X * C, a5 = -Y * A;      // row 0, columns 3..5
  const double b3 = Y * D - Z * A, b4 = -X * D, b5 = X * A;      // row 1
  const double c3 = Y * E, c4 = Z * A - X * E;                   // row 2 (column 5 = a5)
  if (FIRST) {
    const double AA = A * A;
    double m = fmax(AA + AA, AA);
    m = fmax(m, C * C + D * D + E * E);
    m = fmax(m, a3 * a3 + b3 * b3 + c3 * c3);
    m = fmax(m, a4 * a4 + b4 * b4 + c4 * c4);
    m = fmax(m, a5 * a5 + b5 * b5 + a5 * a5);
    max_diag = fmax(max_diag, m);
  }
  // pseudo-Huber weight (pose_optimizer.h:169-175,426-435): f *= sqrt(k(|f|)) / |f|, chi2 += |w f|^2 = k(|f|)
  const double ss = f0 * f0 + f1 * f1 + f2 * f2;
  double chi = ss;
  if (robust) {
    const double nrm = fmax(1e-10, sqrt(ss));
    if (nrm >= kb) {                                             // outliers only: inside the kernel width the weight is sqrt(n^2) / n = 1
      const double k = 2 * kb * nrm - kb * kb, w = sqrt(k) / nrm;
      f0 *= w; f1 *= w; f2 *= w;
      chi = f0 * f0 + f1 * f1 + f2 * f2;
    }
  }
  x[27] += chi;
  max_err = fmax(max_err, fmax(fabs(f0), fmax(fabs(f1), fabs(f2))));
  if constexpr (!JAC) return;
  // J^T J, upper triangle row-major (21) -- the structural zeros of frameJac are not multiplied out -- and J^T (w f) (6)
  x[0] += A * A + A * A;          x[1] += 0.0;                     x[2] += A * C + A * E;
  x[3] += A * a3 + A * c3;        x[4] += A * a4 + A * c4;         x[5] += A * a5 + A * a5;
  x[6] += A * A;                  x[7] += A * D;                   x[8] += A * b3;
  x[9] += A * b4;                 x[10] += A * b5;
  x[11] += C * C + D * D + E * E; x[12] += C * a3 + D * b3 + E * c3; x[13] += C * a4 + D * b4 + E * c4;
  x[14] += C * a5 + D * b5 + E * a5;
  x[15] += a3 * a3 + b3 * b3 + c3 * c3; x[16] += a3 * a4 + b3 * b4 + c3 * c4; x[17] += a3 * a5 + b3 * b5 + c3 * a5;
  x[18] += a4 * a4 + b4 * b4 + c4 * c4; x[19] += a4 * a5 + b4 * b5 + c4 * a5;
  x[20] += a5 * a5 + b5 * b5 + a5 * a5;
  x[21] += A * f0 + A * f2;       x[22] += A * f1;                 x[23] += C * f0 + D * f1 + E * f2;
  x[24] += a3 * f0 + b3 * f1 + c3 * f2; x[25] += a4 * f0 + b4 * f1 + c4 * f2; x[26] += a5 * f0 + b5 * f1 + a5 * f2;
}
// value id held by lane `lane` (< 32) after the recursive halving of mo2_wave_reduce
__device__ __forceinline__ int mo2_id(int lane) { return ((lane & 1) << 4) | ((lane & 2) << 2) | (lane & 4) | ((lane & 8) >> 2) | ((lane & 16) >> 4); }
__device__ __forceinline__ double mo2_wave_reduce(double (&x)[32]) {
  const int lane = threadIdx.x & 63;
#pragma unroll
  for (int step = 0; step < 5; ++step) {
    const int half = 16 >> step, bit = 1 << step;
    const bool up = (lane & bit) != 0;
#pragma unroll
    for (int k = 0; k < half; ++k) {
      // the two candidates are pinned as VALUES: left alone, the optimiser turns "select of two array elements" into one load at a selected address
      // before the loops are unrolled -- and the accumulator array then lives (and is stored after every observation) in scratch memory
      double lo = x[k], hi = x[k + half];
      asm volatile("" : "+v"(lo), "+v"(hi));
      const double send = up ? lo : hi;
      const double keep = up ? hi : lo;
      x[k] = keep + __shfl_xor(send, bit, 64);
    }
  }
  return x[0] + __shfl_xor(x[0], 32, 64);
}

// one sweep over the observations at pose T: per-wave sums -> s_part[wave]
template <bool FIRST>
__device__ __forceinline__ void mo2_sweep(const double (&T)[12], const MoObs (&ob)[MO2_RC], int n_ok, const int *s_idx, const svs_match_result *__restrict__ res,
                                          const svs_cam &cam, int robust, double kb, double (*s_part)[32]) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  double x[32];
#pragma unroll
  for (int i = 0; i < 32; ++i) x[i] = 0.0;
  double me = 0.0, md = 0.0;
#pragma unroll
  for (int k = 0; k < MO2_RC; ++k)
    if (tid + k * MO2_THREADS < n_ok) mo2_terms<FIRST>(T, ob[k], cam, robust, kb, x, me, md);
  for (int j = tid + MO2_RC * MO2_THREADS; j < n_ok; j += MO2_THREADS) {
    const svs_match_result &r = res[s_idx[j]];
    MoObs t;
#pragma unroll
    for (int c = 0; c < 3; ++c) { t.o[c] = r.obs[c]; t.q[c] = r.xyz_actkey[c]; }
    mo2_terms<FIRST>(T, t, cam, robust, kb, x, me, md);
  }
  const double v = mo2_wave_reduce(x);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) { me = fmax(me, __shfl_xor(me, o, 64)); if (FIRST) md = fmax(md, __shfl_xor(md, o, 64)); }
  const int id = mo2_id(lane);
  if (lane < 32 && id < 28) s_part[wave][id] = v;
  if (lane == 0) { s_part[wave][28] = me; s_part[wave][29] = md; }
}

// chi2 (and the largest residual) at pose T only -> s_part[wave][27], [28].  Bit-identical to what mo2_sweep leaves there: the same per-lane terms in the same
// order, and the butterfly below adds them in the association mo2_wave_reduce's halving gives element 27 (own + partner over lane distances 1, 2, 4, 8, 16, 32).
__device__ __forceinline__ void mo2_sweep_chi2(const double (&T)[12], const MoObs (&ob)[MO2_RC], int n_ok, const int *s_idx, const svs_match_result *__restrict__ res,
                                               const svs_cam &cam, int robust, double kb, double (*s_part)[32]) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  double x[32];
  x[27] = 0.0;
  double me = 0.0, md = 0.0;
#pragma unroll
  for (int k = 0; k < MO2_RC; ++k)
    if (tid + k * MO2_THREADS < n_ok) mo2_terms<false, false>(T, ob[k], cam, robust, kb, x, me, md);
  for (int j = tid + MO2_RC * MO2_THREADS; j < n_ok; j += MO2_THREADS) {
    const svs_match_result &r = res[s_idx[j]];
    MoObs t;
#pragma unroll
    for (int c = 0; c < 3; ++c) { t.o[c] = r.obs[c]; t.q[c] = r.xyz_actkey[c]; }
    mo2_terms<false, false>(T, t, cam, robust, kb, x, me, md);
  }
  double v = x[27];
#pragma unroll
  for (int o = 1; o <= 32; o <<= 1) v += __shfl_xor(v, o, 64);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) me = fmax(me, __shfl_xor(me, o, 64));
  if (lane == 0) { s_part[wave][27] = v; s_part[wave][28] = me; }
}

// the gate of one stream, run by 256 lanes (tid < 256) of a workgroup: s_cnt [18], s_sum [4] in LDS; the caller has a barrier in front of it
__device__ __forceinline__ void gate_stream(const svs_match_result *__restrict__ res, const svs_candidate_point *__restrict__ pts, int n, int n_new, const svs_cam &cam,
                                            const double (&T)[12], float mre, svs_gated_point *__restrict__ out, svs_point_stats *__restrict__ st, int tid, int *s_cnt,
                                            double *s_sum) {
  if (tid < 18) s_cnt[tid] = 0;
  __syncthreads();
  const int half_w = (int)(cam.w * 0.5), half_h = (int)(cam.h * 0.5);
  const float third = (float)(1. / 3.);
  const int third_w = (int)(cam.w * third), third_h = (int)(cam.h * third);
  const int tt_w = (int)(cam.w * 2 * third), tt_h = (int)(cam.h * 2 * third);
  double len = 0;
  // a lane's records are 256 apart; the next one (the matcher's record and the point's anchor level: two round trips to memory that depend on nothing here) is
  // requested before this one's arithmetic
  struct GateIn { svs_match_result r; int level; };
  auto gate_load = [&](int i) {
    GateIn in;
    const int j = i < n ? i : 0;                                 // (past the end: record 0, marked as no match)
    in.r = res[j];
    in.level = pts[j].anchor_level;
    if (i >= n) in.r.status = 1;
    return in;
  };
  GateIn nxt{};
  if (n > 0 && tid < 256) nxt = gate_load(tid);
  for (int i = tid; i < n && tid < 256; i += 256) {
    svs_gated_point g{};
    const GateIn cur = nxt;
    nxt = gate_load(i + 256);
    if (cur.r.status == 0) {
      atomicAdd(&s_cnt[17], 1);
      double d[3];
      mo_residual<false>(T, cur.r, cam, d, nullptr);           // uvu - se3xyz_stereo_.map(T_cur_from_actkey_, point)
      const int level = cur.level;
      const int factor = 1 << level;                             // zeroFromPyr_i(1, anchor_level)
      if (SVS_GATE_PASSES(d, factor, mre)) {
        const double *uvu = cur.r.obs, *q = cur.r.xyz_actkey;
        const int i2 = uvu[0] < half_w ? 0 : 1, j2 = uvu[1] < half_h ? 0 : 1;
        const int i3 = uvu[0] < third_w ? 0 : (uvu[0] < tt_w ? 1 : 2), j3 = uvu[1] < third_h ? 0 : (uvu[1] < tt_h ? 1 : 2);
        atomicAdd(&s_cnt[i2 * 2 + j2], 1);
        atomicAdd(&s_cnt[4 + i3 * 3 + j3], 1);
        atomicAdd(&s_cnt[13 + level], 1);
        atomicAdd(&s_cnt[16], 1);
        const double inv = 1.0 / (double)factor;                 // exact power of two: x * inv == x / factor
        g.accepted = 1;
        g.is_new = i < n_new ? 1 : 0;
        g.uv_pyr[0] = uvu[0] * inv; g.uv_pyr[1] = uvu[1] * inv;
        const double num[2] = {q[0], q[1]};
        double p[2];
        div_rn_guarded(num, q[2], p);                            // q[0] / q[2], q[1] / q[2]
        g.curkey_uv_pyr[0] = (p[0] * cam.f + cam.cx) * inv;
        g.curkey_uv_pyr[1] = (p[1] * cam.f + cam.cy) * inv;
        const double dx = g.uv_pyr[0] - g.curkey_uv_pyr[0], dy = g.uv_pyr[1] - g.curkey_uv_pyr[1];
        len += sqrt(dx * dx + dy * dy);
      }
    }
    out[i] = g;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) len += __shfl_xor(len, o, 64);
  if ((tid & 63) == 0 && tid < 256) s_sum[tid >> 6] = len;
  __syncthreads();
  if (tid < 4) st->num_points_grid2x2[tid] = s_cnt[tid];
  else if (tid < 13) st->num_points_grid3x3[tid - 4] = s_cnt[tid];
  else if (tid < 16) st->num_matched_points[tid - 13] = s_cnt[tid];
  else if (tid == 16) st->num_track_points = s_cnt[16];
  else if (tid == 17) st->num_obs = s_cnt[17];
  else if (tid == 18) { st->pad_[0] = st->pad_[1] = 0; st->sum_track_length = (s_sum[0] + s_sum[1]) + (s_sum[2] + s_sum[3]); }
}
// TAIL: processMatchedPoints' gate and the three dense clouds of a stream run at the end of its refinement workgroup instead of in four launches of their own --
// the streams that converge early do that work while the slow ones still iterate (the stage lasts as long as its slowest stream: <= 15 dependent iterations),
// and four launches per frame disappear.  Same device functions as the stand-alone kernels, the gate on the same 256 lanes: identical bits.
using MoTail = svs_mo_tail;      // common.h
template <bool TAIL>
__global__ __launch_bounds__(MO2_THREADS) void motion_only_fused_kernel(const svs_match_result *__restrict__ res, int n, size_t res_bstride, svs_cam cam,
                                                                        svs_pose_opt_params prm, double *__restrict__ T_io,
                                                                        svs_pose_opt_stats *__restrict__ stats, MoTail Q, int spec) {
  extern __shared__ int s_idx[];                   // [n]: indices of the status-OK records, in list order
  __shared__ double s_part[MO2_WAVES][32];         // per wave: 28 sums (21 of J^T J, 6 of J^T w f, chi2), max error, max diag
  __shared__ double s_Tn[12], s_Tc[12];        // trial pose / accepted pose (the latter is wave 0's)
  __shared__ int s_wcnt[8][MO2_WAVES];
  __shared__ int s_conv;                           // |B|_inf <= 1e-10 at the pose the pending step was taken from
  // TAIL (batches): the streams in the grid order of the tracker (by the last frame's LM work: replicas / neighbours of the caller's order dealt evenly over the XCDs)
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, slot = TAIL && Q.order ? (Q.order[blockIdx.x] >> 4) : (int)blockIdx.x;
  res += (size_t)slot * res_bstride;
  // ---- compaction of obs_list / point_list (the OK records, in order).  Eight chunks per round: their status words are requested together
  // (one memory round trip instead of eight), one barrier per round
  int n_ok = 0;
  for (int base = 0; base < n; base += 8 * MO2_THREADS) {
    int st[8];
#pragma unroll
    for (int c = 0; c < 8; ++c) { const int i = base + c * MO2_THREADS + tid; st[c] = i < n ? res[i].status : 1; }
    unsigned long long m[8];
#pragma unroll
    for (int c = 0; c < 8; ++c) { m[c] = __ballot(st[c] == 0); if (lane == 0) s_wcnt[c][wave] = __popcll(m[c]); }
    __syncthreads();
#pragma unroll
    for (int c = 0; c < 8; ++c) {
      int off = n_ok, tot = 0;
#pragma unroll
      for (int w = 0; w < MO2_WAVES; ++w) { const int k = s_wcnt[c][w]; off += w < wave ? k : 0; tot += k; }
      if (st[c] == 0) s_idx[off + __popcll(m[c] & ((1ull << lane) - 1ull))] = base + c * MO2_THREADS + tid;
      n_ok += tot;
    }
    __syncthreads();
  }
  MoObs ob[MO2_RC];
#pragma unroll
  for (int k = 0; k < MO2_RC; ++k) {
    const int j = tid + k * MO2_THREADS;
    if (j < n_ok) {
      const svs_match_result &r = res[s_idx[j]];
#pragma unroll
      for (int c = 0; c < 3; ++c) { ob[k].o[c] = r.obs[c]; ob[k].q[c] = r.xyz_actkey[c]; }
    }
  }
  auto total = [&](int id) { double s = s_part[0][id]; for (int w = 1; w < MO2_WAVES; ++w) s += s_part[w][id]; return s; };
  auto total_max = [&](int id) { double s = s_part[0][id]; for (int w = 1; w < MO2_WAVES; ++w) s = fmax(s, s_part[w][id]); return s; };
  // the pose of a sweep is wave-uniform: read once, moved to scalar registers (24 SGPRs instead of 24 VGPRs per lane)
  auto uniform_pose = [&](const double *p, double (&T)[12]) {
#pragma unroll
    for (int i = 0; i < 12; ++i) {
      const double v = p[i];
      T[i] = __hiloint2double(__builtin_amdgcn_readfirstlane(__double2hiint(v)), __builtin_amdgcn_readfirstlane(__double2loint(v)));
    }
  };
  double Tn[12];
  uniform_pose(T_io + 12 * slot, Tn);
  if (tid < 12) s_Tc[tid] = T_io[12 * slot + tid];
  mo2_sweep<true>(Tn, ob, n_ok, s_idx, res, cam, prm.robust_kernel, prm.kernel_param, s_part);
  __syncthreads();                                 // (A) sums of the sweep are in s_part
  const int num_obs = n_ok;
  double chi2 = total(27), max_err = total_max(28), mu = prm.initial_mu == -1 ? prm.tau * total_max(29) : prm.initial_mu, nu = 2;
  const double initial_chi2 = chi2;
  int status = num_obs == 0 ? 1 : (num_obs < prm.min_obs ? 3 : 0), trial = 0;
  bool stop = status != 0;
  // wave 0, lane c < 6: column c of the stored J^T J; lane 6: -J^T w f
  double col[6] = {0, 0, 0, 0, 0, 0};
  auto load_system = [&]() {
    if (wave == 0 && lane < 7) {
#pragma unroll
      for (int r = 0; r < 6; ++r) {
        const int a = r < lane ? r : lane, b = r < lane ? lane : r;      // upper-triangular index of (r, lane)
        col[r] = lane < 6 ? total(a * (13 - a) / 2 + (b - a)) : -total(21 + r);
      }
    }
  };
  load_system();
  // Two barriers per LM trial: (B) the trial pose is in s_Tn and every wave has read the sums of the sweep before; (A) the new sums are in s_part.
  for (int ig = 0; ig < prm.num_iter && !stop; ++ig) {
    double rho = 0;
    do {
      if (wave == 0) {
        // (A + mu I) delta = B on lanes 0..6 (wave_solve6)
        double a[6], bmax = 0, delta[6];
#pragma unroll
        for (int r = 0; r < 6; ++r) a[r] = col[r] + (r == lane ? mu : 0.0);
#pragma unroll
        for (int r = 0; r < 6; ++r) bmax = fmax(bmax, fabs(lane_bcast(col[r], 6)));
        wave_solve6(a, delta);
        double Tc[12], Tx[12];
#pragma unroll
        for (int i = 0; i < 12; ++i) Tc[i] = s_Tc[i];
        mo2_exp_mul(delta, Tc, Tx);                  // prediction.add: exp(delta) * T (every lane of the wave, same values)
        if (lane < 12) {
          double v = Tx[0];
#pragma unroll
          for (int i = 1; i < 12; ++i) v = lane == i ? Tx[i] : v;
          s_Tn[lane] = v;
        }
        if (lane == 0) s_conv = bmax <= 1e-10 ? 1 : 0;
      }
      __syncthreads();                               // (B)
      uniform_pose(s_Tn, Tn);
      const int conv = s_conv;
      // A trial that follows a rejection is almost always rejected too (every refinement ends in five rejections in a row at the noise floor of its chi2: a third
      // of all sweeps), and a rejected trial's Jacobian sums are never used: such a trial gets a chi2-only sweep ("mo_spec"); should it be accepted after all, the
      // full sweep at the same pose follows.  Either way the sums the loop goes on with are those of the full sweep: identical bits.
      const bool lean = spec != 0 && trial >= 1;
      if (lean) mo2_sweep_chi2(Tn, ob, n_ok, s_idx, res, cam, prm.robust_kernel, prm.kernel_param, s_part);
      else mo2_sweep<false>(Tn, ob, n_ok, s_idx, res, cam, prm.robust_kernel, prm.kernel_param, s_part);
      __syncthreads();                               // (A)
      const double new_chi2 = total(27), new_max = total_max(28);
      if (isnan(new_chi2)) { status = 2; stop = true; break; }      // the reference throws here
      rho = chi2 - new_chi2;
      if (rho > 0 && lean) {
        __syncthreads();                             // every lane has read the totals
        mo2_sweep<false>(Tn, ob, n_ok, s_idx, res, cam, prm.robust_kernel, prm.kernel_param, s_part);
        __syncthreads();
      }
      if (rho > 0) {
        if (tid < 12) s_Tc[tid] = s_Tn[tid];         // wave 0 only: it is the one that reads s_Tc (next solve) and rewrites s_Tn (after it)
        chi2 = new_chi2; max_err = new_max;
        load_system();
        stop = conv != 0;                            // |B|_inf <= 1e-10 at the pose the accepted step started from
        const double q = 2 * rho - 1, sc = 1 - q * q * q;
        mu *= fmax(1. / 3., sc);
        nu = 2.; trial = 0;
      } else {
        mu *= nu; nu *= 2.; ++trial;
        if (trial == 5) stop = true;
      }
    } while (!(rho > 0 || stop));
  }
  if (tid < 12) T_io[12 * slot + tid] = s_Tc[tid];
  if (tid == 0) {
    svs_pose_opt_stats st;
    st.initial_chi2 = initial_chi2; st.chi2 = chi2; st.max_err = max_err; st.num_obs = num_obs; st.status = status;
    stats[slot] = st;
  }
  if constexpr (TAIL) {
    __shared__ int s_gcnt[18];
    __shared__ double s_gsum[4];
    __syncthreads();                                 // s_Tc is final
    double T[12];
#pragma unroll
    for (int i = 0; i < 12; ++i) T[i] = s_Tc[i];
    gate_stream(res, Q.pts + slot * Q.pts_b, n, Q.n_new[slot], cam, T, Q.mre, Q.gated + slot * Q.gated_b, Q.ptstats + slot, tid, s_gcnt, s_gsum);
#pragma unroll 1
    for (int l = 0; l < 3; ++l) {
      double TQ[16];
      cloud_TQ(T, Q.cams[l], TQ);
      const float *disp = Q.disp + slot * Q.disp_b;
      float *cloud = Q.cloud[l] + slot * Q.cloud_b[l];
      cloud_level_sweep<MO2_THREADS, CLOUD_PF>(disp, Q.ds, Q.cams[l], l, TQ, cloud, tid);
    }
  }
}

}  // namespace
// ---- StereoFrontend::processMatchedPoints (stereo_frontend.cpp:834-974), data-parallel part ---------------------------
// One workgroup per stream sweeps the matcher records: reprojection gate at the refined pose, the 2x2 / 3x3 / per-level
// counters (LDS atomics), the pyramid-level positions the host needs for point_tree and the draw lists, and the
// track-length sum.  The host-side remainder (building new_point_list / track_point_list) walks the flags.
namespace {
__global__ __launch_bounds__(256) void gate_matched_kernel(const svs_match_result *__restrict__ res, const svs_candidate_point *__restrict__ pts, int n,
                                                           size_t res_b, size_t pts_b, int n_new, const int32_t *__restrict__ n_new_arr, svs_cam cam,
                                                           const double *__restrict__ Tarr, float mre, svs_gated_point *__restrict__ out, size_t out_b,
                                                           svs_point_stats *__restrict__ stats) {
  __shared__ int s_cnt[18];          // 4 + 9 + 3 + num_track + num_obs
  __shared__ double s_sum[4];
  const int tid = threadIdx.x, slot = blockIdx.x;
  if (n_new_arr) n_new = n_new_arr[slot];
  double T[12];
#pragma unroll
  for (int k = 0; k < 12; ++k) T[k] = Tarr[12 * slot + k];
  gate_stream(res + slot * res_b, pts + slot * pts_b, n, n_new, cam, T, mre, out + slot * out_b, stats + slot, tid, s_cnt, s_sum);
}
}  // namespace

extern "C" int svs_process_matched_points(svs_ctx *ctx, const svs_match_result *d_results, const svs_candidate_point *d_pts, int n,
                                          size_t res_bstride, size_t pts_bstride, int n_new_records, const svs_cam *cam, const double *d_T,
                                          float max_reproj_error, svs_gated_point *d_gated, size_t gated_bstride, svs_point_stats *d_stats,
                                          int batch) {
  SVS_REQUIRE(ctx, ctx && cam && d_T && d_stats && batch >= 1 && n >= 0 && (n == 0 || (d_results && d_pts && d_gated)));
  SVS_DEVICE(ctx);
  hipLaunchKernelGGL(gate_matched_kernel, dim3(batch), dim3(256), 0, ctx->stream, d_results, d_pts, n, res_bstride, pts_bstride, n_new_records,
                     (const int32_t *)nullptr, *cam, d_T, max_reproj_error, d_gated, gated_bstride, d_stats);
  SVS_LAUNCH_CHECK(ctx);
  return SVS_OK;
}
// the same with one record count of the new-feature lists PER STREAM, on the device (frontend.hip: streams carry different candidate lists)
int svs_process_matched_points_dev(svs_ctx *ctx, const svs_match_result *d_results, const svs_candidate_point *d_pts, int n, size_t res_bstride,
                                   size_t pts_bstride, const int32_t *d_n_new_records, const svs_cam *cam, const double *d_T, float max_reproj_error,
                                   svs_gated_point *d_gated, size_t gated_bstride, svs_point_stats *d_stats, int batch) {
  SVS_REQUIRE(ctx, ctx && cam && d_T && d_stats && d_n_new_records && batch >= 1 && n >= 0 && (n == 0 || (d_results && d_pts && d_gated)));
  SVS_DEVICE(ctx);
  hipLaunchKernelGGL(gate_matched_kernel, dim3(batch), dim3(256), 0, ctx->stream, d_results, d_pts, n, res_bstride, pts_bstride, 0, d_n_new_records, *cam, d_T,
                     max_reproj_error, d_gated, gated_bstride, d_stats);
  SVS_LAUNCH_CHECK(ctx);
  return SVS_OK;
}

// calcFastMotionOnly + processMatchedPoints' gate + the three dense clouds of every stream in ONE launch (frontend.hip; see MoTail).  Returns SVS_ERR_UNSUPPORTED
// when the fused refinement kernel does not apply (the caller then takes the separate launches).
int svs_motion_only_gate_cloud(svs_ctx *ctx, const svs_match_result *d_results, int n, size_t res_bstride, const svs_cam *cam, const svs_pose_opt_params *prm,
                               double *d_T_io, svs_pose_opt_stats *d_stats, const svs_mo_tail *tail, int batch) {
  SVS_REQUIRE(ctx, ctx && cam && prm && d_T_io && d_stats && tail && batch >= 1 && n >= 1 && d_results);
  SVS_DEVICE(ctx);
  if ((size_t)n * sizeof(int) > 48 * 1024 || ctx->mo_legacy) return SVS_ERR_UNSUPPORTED;
  for (int l = 0; l < 3; ++l) SVS_REQUIRE(ctx, tail->cams[l].w % 4 == 0 && tail->cams[l].h % 4 == 0 && tail->cloud[l]);
  hipLaunchKernelGGL(motion_only_fused_kernel<true>, dim3(batch), dim3(MO2_THREADS), (size_t)n * sizeof(int), ctx->stream, d_results, n, res_bstride, *cam, *prm, d_T_io,
                     d_stats, *tail, ctx->mo_spec);
  SVS_LAUNCH_CHECK(ctx);
  return SVS_OK;
}

extern "C" int svs_motion_only(svs_ctx *ctx, const svs_match_result *d_results, int n, size_t res_bstride, const svs_cam *cam,
                               const svs_pose_opt_params *prm, double *d_T_io, svs_pose_opt_stats *d_stats, int batch) {
  SVS_REQUIRE(ctx, ctx && cam && prm && d_T_io && d_stats && batch >= 1 && n >= 0 && (n == 0 || d_results));
  SVS_DEVICE(ctx);
  // the record-walking kernel stays for candidate lists whose index list does not fit LDS, and as the A/B partner ("mo_legacy")
  if ((size_t)n * sizeof(int) <= 48 * 1024 && !ctx->mo_legacy)
    hipLaunchKernelGGL(motion_only_fused_kernel<false>, dim3(batch), dim3(MO2_THREADS), (size_t)std::max(n, 1) * sizeof(int), ctx->stream, d_results, n, res_bstride, *cam,
                       *prm, d_T_io, d_stats, MoTail{}, ctx->mo_spec);
  else
    hipLaunchKernelGGL(motion_only_kernel, dim3(batch), dim3(MO_THREADS), 0, ctx->stream, d_results, n, res_bstride, *cam, *prm, d_T_io, d_stats);
  SVS_LAUNCH_CHECK(ctx);
  return SVS_OK;
}
