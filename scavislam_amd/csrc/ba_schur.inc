// ba_schur.inc -- part of ba.hip (one translation unit): f64 helpers, edge algebra, the device view of a problem (BaDev), the pose-pose constraint
// kernel and the Schur-complement kernels (one lane per edge; landmarks with more than 64 observations on 256-lane workgroups).
// ---- small f64 helpers ---------------------------------------------------------------------
__device__ __forceinline__ void atomic_add_f64(double *p, double v) { unsafeAtomicAdd(p, v); }
// LDS f64 atomic (ds_add_f64): workgroup-scope relaxed add on a __shared__ double
__device__ __forceinline__ void lds_add_f64(double *p, double v) {
  __hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}
// Per-workgroup accumulation window over WIN consecutive poses: the packed upper block triangle
// of the WIN x WIN pose window (plus b_p / b_s rows) lives in LDS; contributions whose poses fall
// outside the window go straight to global atomics.  Landmarks are processed sorted by anchor,
// so a workgroup's landmarks touch a narrow band of poses and nearly everything lands in LDS.
// Trial scalars (d_scal): [2] scale_p [3] fail [4] chi2_cur copy [5..11] solve phase times; the sums every workgroup contributes to --
// chi2 at the trial state and x_l (lambda x_l + b_l) -- are spread over SC_SLOTS words each (a workgroup adds to slot blockIdx % 16:
// hundreds of same-address f64 atomics serialise at the memory side) and folded by their readers
constexpr int SC_SLOTS = 16, SC_CHI = 16, SC_SCL = 32, SC_N = 48;
constexpr int DBG_N = 10;   // phase stamps per wave of the Schur kernel timeline (SVS_BA_DEBUG=2)
constexpr int DBG_X = 8;    // + per-wave structure words: landmarks, same-address multiplicity of the observer / anchor adds, pair rounds
constexpr int DBG_W = DBG_N + DBG_X;
constexpr int WIN = 16;               // widest window of the small pool (two workgroups per CU); the host lays out anchor groups against it
constexpr int WIN_BIG = 22;           // widest window of the big pool (one workgroup per CU)
constexpr int WIN_BLOCKS_MAX = WIN_BIG * (WIN_BIG + 1) / 2;
// LDS stride of one 6x6 window block in doubles: 37 (not 36) spreads the same element of different
// blocks over all banks -- measured 11 vs 32 cycles per ds_add_f64 wave instruction (tools/ubench.hip)
constexpr int WBLK = 37;
// The window is sized PER WORKGROUP: win = the pose span its edges actually touch (pmin .. pmax, at most WIN / WIN_BIG), and the pool
// holds as many COPIES of that window as fit (at most WCOPIES_MAX).  The cost of a ds_add_f64 wave instruction is set by the number of
// lanes that hit the SAME address (~3.6 cycles each: 13 lanes 47 cycles, <= 3 lanes 11 = the floor, tools/ubench.hip) -- lanes of
// different landmarks seen from the same keyframe.  A lane adds into copy (ordinal of its landmark in the wave) % copies, so with c
// copies at most ceil(landmarks per wave / c) lanes collide; a one-anchor workgroup spans ~9 poses = 45 blocks = 6 copies.  The
// flush adds the copies.
constexpr int WCOPIES_MAX = 8;
constexpr int SEG_DPP_MAX = 12;      // longest landmark of a wave for which the segmented sums use DPP shifts (seg_allreduce)
__device__ __host__ constexpr int win_pool_doubles(int nw, int wc) { return wc == 2 ? (163840 - nw * 64 * 18 * 8 - 4096) / 8 : 5226; }      // small pool: one 16-pose window (136 * 37 + 192 doubles, odd stride)
__device__ __forceinline__ int win_blk(int wi, int wj, int win) { return wi * win - wi * (wi - 1) / 2 + (wj - wi); }

// value of the lane below (wave_shr:1 reaches across the 16-lane DPP rows on gfx9), 0 in lane 0 and wherever `keep` is 0: one
// v_and_b32_dpp per word, no LDS-pipeline slot (a __shfl is two ds_bpermute_b32 that queue behind the kernel's LDS atomics)
__device__ __forceinline__ double shr1_keep(double x, unsigned keep) {
  int lo = __double2loint(x), hi = __double2hiint(x);
  lo = __builtin_amdgcn_update_dpp(0, lo, 0x138, 0xf, 0xf, true) & keep;
  hi = __builtin_amdgcn_update_dpp(0, hi, 0x138, 0xf, 0xf, true) & keep;
  return __hiloint2double(hi, lo);
}
// Sum of v over the lanes of each segment (= landmark).  The total is formed in the segment's LAST lane; its first NB values are
// handed to every lane of the segment, the remaining N - NB stay valid in the last lane only (the per-landmark anchor terms, which
// one lane consumes).  Short segments (the common case: a landmark has 3..9 observations) run a sliding sum with DPP shifts: after
// step k a lane holds v[lane] + ... + v[lane - k], cut at its segment head -- maxlen - 1 steps of 3 VALU instructions per value and
// no LDS-pipeline slot.  The recursive-doubling form (long segments) needs fewer steps, but each is two bpermutes per value on the
// LDS pipeline, which the Schur kernel's atomics already saturate (27 values x 4 x 2 = 216 per wave were 5 us of its 40,
// SVS_BA_DEBUG=2 timeline).  The hand-over goes through `slot` (SEG_SLOT doubles of LDS per lane, 16-byte aligned): 9 wide
// writes by the tail lanes + 9 wide reads instead of 54 bpermutes.
// (Measured alternatives at 50 KF / 20k, against 2.7 us per wave for this form: a column sum through LDS -- every lane parks its values,
// one lane per column walks the segment's rows -- 4.3 us, ~40 dependent read groups per lane; ds_add_f64 of the 27 values into the
// segment's first slot -- 4.1 us, the seven waves of a workgroup queue on the LDS pipeline.)
constexpr int SEG_SLOT = 18;
template <int N, int NB>
__device__ __forceinline__ void seg_allreduce(double (&v)[N], int lane, int seg_begin, int seg_end, int maxlen, double *wave_slots) {
  static_assert(NB <= SEG_SLOT && NB <= N, "");
  if (maxlen <= SEG_DPP_MAX) {
    const unsigned keep = lane == seg_begin ? 0u : 0xffffffffu;      // a head lane takes nothing from below
    double s[N];
#pragma unroll
    for (int i = 0; i < N; ++i) s[i] = v[i];
    for (int k = 1; k < maxlen; ++k) {
#pragma unroll
      for (int i = 0; i < N; ++i) { s[i] = shr1_keep(s[i], keep); v[i] += s[i]; }
    }
  } else {
    for (int o = 1; o < maxlen; o <<= 1) {
      const bool take = (lane - o) >= seg_begin;
#pragma unroll
      for (int i = 0; i < N; ++i) { double up = __shfl_up(v[i], o, 64); if (take) v[i] += up; }
    }
  }
  double *slot = wave_slots + seg_end * SEG_SLOT;
  if (lane == seg_end) {
#pragma unroll
    for (int i = 0; i < NB; ++i) slot[i] = v[i];
  }
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
#pragma unroll
  for (int i = 0; i < NB; ++i) v[i] = slot[i];
}

__device__ __forceinline__ long blk_index(int i, int j, int P) {   // i <= j, packed upper block row-major
  return (long)i * P - (long)i * (i - 1) / 2 + (j - i);
}

__device__ __forceinline__ void huber(double e2, double delta, int robust, double &rho0, double &rho1) {
  if (!robust) { rho0 = e2; rho1 = 1; return; }
  const double dsqr = delta * delta;
  if (e2 <= dsqr) { rho0 = e2; rho1 = 1.; }
  else { const double s = sqrt(e2); rho0 = 2 * s * delta - dsqr; rho1 = delta / s; }
}

// Compact linearisation of one G2oEdgeProjectPSI2UVU (anchored_points.cpp:148-189).  With
//   Jc = d_stereoproj_d_y(y),  D = d_Tinvpsi_d_psi,  Eo = [I | -hat(y)],  Ea = [I | -hat(x_a)]
// the three Jacobians are  J_psi = -Jc D,  J_obs = -Jc Eo,  J_anc = Jc R Ea  (transformations.h:62-95),
// so every block of the normal equations derives from the 3x3 matrix  A = Jc^T (rho1 Lambda) Jc  and
// g = Jc^T (-rho1 Lambda e):
//   H_ll = D^T A D        b_l = -D^T g        W_obs = Eo^T (A D)        W_anc = -Ea^T R^T (A D)
//   M_oo = Eo^T A Eo      M_aa = Ea^T (R^T A R) Ea      M_oa = -Eo^T (A R) Ea
//   b_obs = -Eo^T g       b_anc = Ea^T R^T g
// and E^T X = [X ; v x X(:,c)],  X E = [X | v x X(r,:)]: cross products instead of 3x6 / 6x6 products
// (~350 f64 operations per edge instead of ~1400 for the explicit J^T Omega J forms).
struct EdgeCore {
  double R[9], xa[3], y[3];
  double A[9];             // symmetric 3x3, stored full
  double g[3];
  double D[9];
  double rho0;
};
__device__ __forceinline__ void cross3(const double *v, double x0, double x1, double x2, double &o0, double &o1, double &o2) {
  o0 = v[1] * x2 - v[2] * x1; o1 = v[2] * x0 - v[0] * x2; o2 = v[0] * x1 - v[1] * x0;
}
// M = E^T X E (6x6, full) for symmetric 3x3 X and E = [I | -hat(v)]
__device__ __forceinline__ void sym_block(const double *X, const double *v, double *M) {
#pragma unroll
  for (int r = 0; r < 3; ++r) {
#pragma unroll
    for (int c = 0; c < 3; ++c) M[6 * r + c] = X[3 * r + c];
    cross3(v, X[3 * r], X[3 * r + 1], X[3 * r + 2], M[6 * r + 3], M[6 * r + 4], M[6 * r + 5]);       // top-right rows
  }
#pragma unroll
  for (int c = 0; c < 3; ++c) cross3(v, M[3 + c], M[6 + 3 + c], M[12 + 3 + c], M[18 + 3 + c], M[24 + 3 + c], M[30 + 3 + c]);   // bottom-right cols
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int c = 0; c < 3; ++c) M[6 * (3 + i) + c] = M[6 * c + 3 + i];
}
// N = Eo^T X Ea (6x6, full) for general 3x3 X, Eo = [I | -hat(y)], Ea = [I | -hat(xa)]
__device__ __forceinline__ void cross_block(const double *X, const double *y, const double *xa, double *N) {
#pragma unroll
  for (int r = 0; r < 3; ++r) {
#pragma unroll
    for (int c = 0; c < 3; ++c) N[6 * r + c] = X[3 * r + c];
    cross3(xa, X[3 * r], X[3 * r + 1], X[3 * r + 2], N[6 * r + 3], N[6 * r + 4], N[6 * r + 5]);
  }
#pragma unroll
  for (int c = 0; c < 6; ++c) cross3(y, N[c], N[6 + c], N[12 + c], N[18 + c], N[24 + c], N[30 + c]);
}

__device__ __forceinline__ void rel_pose(const double *To, const double *Ta, double *R, double *t) {
  // T_ca = T_obs * T_anc^-1
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) R[3 * i + j] = To[4 * i] * Ta[4 * j] + To[4 * i + 1] * Ta[4 * j + 1] + To[4 * i + 2] * Ta[4 * j + 2];
#pragma unroll
  for (int i = 0; i < 3; ++i) t[i] = To[4 * i + 3] - (R[3 * i] * Ta[3] + R[3 * i + 1] * Ta[7] + R[3 * i + 2] * Ta[11]);
}

__device__ __forceinline__ double edge_chi2(const double *psi, const double *To, const double *Ta, const svs_ba_edge &ed,
                                            const svs_cam &cam, double delta, int robust) {
  double R[9], t[3];
  rel_pose(To, Ta, R, t);
  const double xa[3] = {psi[0] / psi[2], psi[1] / psi[2], 1. / psi[2]};
  double y[3];
#pragma unroll
  for (int i = 0; i < 3; ++i) y[i] = R[3 * i] * xa[0] + R[3 * i + 1] * xa[1] + R[3 * i + 2] * xa[2] + t[i];
  const double e0 = ed.obs[0] - ((y[0] / y[2]) * cam.f + cam.cx);
  const double e1 = ed.obs[1] - ((y[1] / y[2]) * cam.f + cam.cy);
  const double e2_ = ed.obs[2] - (((y[0] - cam.b) / y[2]) * cam.f + cam.cx);
  const double e2 = e0 * e0 * ed.info[0] + e1 * e1 * ed.info[1] + e2_ * e2_ * ed.info[2];
  double r0, r1;
  huber(e2, delta, robust, r0, r1);
  return r0;
}

__device__ __forceinline__ void linearize_edge(const double *psi, const double *To, const double *Ta, const svs_ba_edge &ed,
                                               const svs_cam &cam, double delta, int robust, EdgeCore &o) {
  double t[3];
  rel_pose(To, Ta, o.R, t);
  const double ipz = 1. / psi[2];
  o.xa[0] = psi[0] * ipz; o.xa[1] = psi[1] * ipz; o.xa[2] = ipz;        // invert_depth, maths_utils.h:66-69
  double Rx[3];
#pragma unroll
  for (int i = 0; i < 3; ++i) { Rx[i] = o.R[3 * i] * o.xa[0] + o.R[3 * i + 1] * o.xa[1] + o.R[3 * i + 2] * o.xa[2]; o.y[i] = Rx[i] + t[i]; }
  const double iz = 1. / o.y[2], fz = cam.f * iz;
  double err[3];
  err[0] = ed.obs[0] - (o.y[0] * fz + cam.cx);
  err[1] = ed.obs[1] - (o.y[1] * fz + cam.cy);
  err[2] = ed.obs[2] - ((o.y[0] - cam.b) * fz + cam.cx);
  const double e2 = err[0] * err[0] * ed.info[0] + err[1] * err[1] * ed.info[1] + err[2] * err[2] * ed.info[2];
  double rho1;
  huber(e2, delta, robust, o.rho0, rho1);
  const double om0 = rho1 * ed.info[0], om1 = rho1 * ed.info[1], om2 = rho1 * ed.info[2];
  const double w0 = -om0 * err[0], w1 = -om1 * err[1], w2 = -om2 * err[2];
  // Jc = [a 0 c0; 0 a c1; a 0 c2]  (d_stereoproj_d_y, transformations.h:62-71)
  const double a = fz, c0 = -fz * o.y[0] * iz, c1 = -fz * o.y[1] * iz, c2 = -fz * (o.y[0] - cam.b) * iz;
  o.A[0] = a * a * (om0 + om2); o.A[1] = 0.0; o.A[2] = a * (om0 * c0 + om2 * c2);
  o.A[4] = a * a * om1; o.A[5] = a * om1 * c1;
  o.A[8] = om0 * c0 * c0 + om1 * c1 * c1 + om2 * c2 * c2;
  o.A[3] = o.A[1]; o.A[6] = o.A[2]; o.A[7] = o.A[5];
  o.g[0] = a * (w0 + w2); o.g[1] = a * w1; o.g[2] = c0 * w0 + c1 * w1 + c2 * w2;
  // D = [r1 r2 -R x_a] / psi_z  (d_Tinvpsi_d_psi, transformations.h:82-95)
#pragma unroll
  for (int i = 0; i < 3; ++i) { o.D[3 * i] = o.R[3 * i] * ipz; o.D[3 * i + 1] = o.R[3 * i + 1] * ipz; o.D[3 * i + 2] = -Rx[i] * ipz; }
}

struct BaDev {
  int P, L, E, C, n_chunks;
  const double *poses, *psi;            // current state
  double *poses_trial, *psi_trial;      // trial state
  const svs_ba_edge *edges;
  const int *chunk_start, *chunk_len;
  const svs_ba_constraint *cons;
  double *H;                            // packed upper blocks [nblk][36]
  double *bp, *bs;                      // [6P] pure b, Schur correction
  double *chi2_cur;                     // [SC_SLOTS] partial sums of chi2 at the current state (a workgroup adds to slot blockIdx % SC_SLOTS)
  const double *x;                      // [6P] pose solution
  double *scal;                         // [0]=chi2_trial [1]=scale_l [2]=scale_p [3]=fail [4]=chi2_cur copy
  svs_cam cam;
  double delta, lambda;
  int robust, self_mode;
  long long *dbg;                       // SVS_BA_DEBUG=2: per-wave phase stamps (100 MHz ticks), DBG_N per chunk
  double *ctl;                          // device-side LM control (speculative trials): [0] lambda, [1] abort flag, [8 + 8 it ..] trial records
  int fuse_cons;                        // constraints ride in extra workgroups of the landmark kernels
  int n_wide;                           // landmarks with more than 64 observations: one workgroup each (ba_wide_landmark_kernel)
  const int *wide_start, *wide_len;     // their edge ranges (behind the chunked edges)
  int wide_split;                       // workgroups per wide landmark in the Schur pass (they share its pair rounds)
};
__device__ __forceinline__ double chi2_cur_sum(const BaDev &B) { double t = 0; for (int i = 0; i < SC_SLOTS; ++i) t += B.chi2_cur[i]; return t; }

// ---- pose-pose constraints: G2oEdgeSE3 (anchored_points.cpp:207-235) -------------------------
__device__ void d_so3_log(const double *R, double *w, double &theta) {
  double q[4];
  const double tr = R[0] + R[4] + R[8];
  if (tr > 0) { double s = sqrt(tr + 1.0) * 2; q[0] = 0.25 * s; q[1] = (R[7] - R[5]) / s; q[2] = (R[2] - R[6]) / s; q[3] = (R[3] - R[1]) / s; }
  else if (R[0] > R[4] && R[0] > R[8]) { double s = sqrt(1.0 + R[0] - R[4] - R[8]) * 2; q[0] = (R[7] - R[5]) / s; q[1] = 0.25 * s; q[2] = (R[1] + R[3]) / s; q[3] = (R[2] + R[6]) / s; }
  else if (R[4] > R[8]) { double s = sqrt(1.0 + R[4] - R[0] - R[8]) * 2; q[0] = (R[2] - R[6]) / s; q[1] = (R[1] + R[3]) / s; q[2] = 0.25 * s; q[3] = (R[5] + R[7]) / s; }
  else { double s = sqrt(1.0 + R[8] - R[0] - R[4]) * 2; q[0] = (R[3] - R[1]) / s; q[1] = (R[2] + R[6]) / s; q[2] = (R[5] + R[7]) / s; q[3] = 0.25 * s; }
  const double n = sqrt(q[1] * q[1] + q[2] * q[2] + q[3] * q[3]), ww = q[0];
  double two_atan;
  if (n < 1e-10) two_atan = 2.0 / ww - 2.0 * (n * n) / (ww * ww * ww);
  else if (fabs(ww) < 1e-10) two_atan = (ww > 0 ? M_PI : -M_PI) / n;
  else two_atan = 2.0 * atan(n / ww) / n;
  w[0] = two_atan * q[1]; w[1] = two_atan * q[2]; w[2] = two_atan * q[3];
  theta = two_atan * n;
}
__device__ void d_se3_log(const double *T, double *x) {
  double R[9], W[9], W2[9], Vi[9], th;
  for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) R[3 * i + j] = T[4 * i + j];
  d_so3_log(R, x + 3, th);
  const double *w = x + 3;
  W[0] = 0; W[1] = -w[2]; W[2] = w[1]; W[3] = w[2]; W[4] = 0; W[5] = -w[0]; W[6] = -w[1]; W[7] = w[0]; W[8] = 0;
  for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) W2[3 * i + j] = W[3 * i] * W[j] + W[3 * i + 1] * W[3 + j] + W[3 * i + 2] * W[6 + j];
  const double c = fabs(th) < 1e-10 ? 1.0 / 12.0 : (1.0 - th / (2.0 * tan(th / 2.0))) / (th * th);
  for (int i = 0; i < 9; ++i) Vi[i] = -0.5 * W[i] + c * W2[i];
  Vi[0] += 1; Vi[4] += 1; Vi[8] += 1;
  for (int i = 0; i < 3; ++i) x[i] = Vi[3 * i] * T[3] + Vi[3 * i + 1] * T[7] + Vi[3 * i + 2] * T[11];
}
// One wavefront per constraint; lane (i,j) = element of the 6x6 products, operands staged in LDS.
// (A one-thread-per-constraint version spent 60 us in scratch-spilled serial 6x6x6 products.)

// one wave per constraint (lanes 0..63 of the calling workgroup); s_m: 8 x 36 doubles of LDS
// 0 Adj(T21) 1 dl(e) 2 t1 3 J1 4 dl(-e) 5 J2 6 O*J1 7 O*J2
template <int MODE>
__device__ __forceinline__ void ba_constraint_body(const BaDev &B, int c, double (*s_m)[36]) {
  const int lane = threadIdx.x;
  const svs_ba_constraint &cc = B.cons[c];
  const double *poses = MODE == 0 ? B.poses : B.poses_trial;
  double T2i[12], t[12], err[6];
  pose_inv(poses + 12 * cc.pose2, T2i);
  pose_mul(cc.T_21, poses + 12 * cc.pose1, t);
  pose_mul(t, T2i, t);
  d_se3_log(t, err);                                    // redundant per lane: ~300 flop
  double oe[6], e2 = 0;
#pragma unroll
  for (int i = 0; i < 6; ++i) { oe[i] = 0; for (int j = 0; j < 6; ++j) oe[i] += cc.info[6 * i + j] * err[j]; e2 += err[i] * oe[i]; }
  if (MODE == 1) { if (lane == 0) atomic_add_f64(&B.scal[SC_CHI + (c & (SC_SLOTS - 1))], e2); return; }
  if (lane == 0) atomic_add_f64(B.chi2_cur + (c & (SC_SLOTS - 1)), e2);
  const int i = lane / 6, j = lane - 6 * i;             // lanes 0..35 own element (i,j)
  const bool on = lane < 36;
  // Adj(T21) = [[R, t^R],[0, R]];  d_lieBracketab_by_d_a(d) = -ad_d   (SURVEY.md A.4)
  if (on) {
    const double *A = cc.T_21;
    const double tt[3] = {A[3], A[7], A[11]};
    const int bi = i % 3, bj = j % 3;
    const double Rij = A[4 * bi + bj];
    // element (r, c) of hat(v) = [[0, -v2, v1], [v2, 0, -v0], [-v1, v0, 0]] by arithmetic on the indices: the three 3 x 3 tables this used to index with (bi, bj)
    // were private arrays under a per-lane index, i.e. 224 bytes of scratch memory per lane of EVERY workgroup of the landmark kernel
    auto hat = [](double v0, double v1, double v2, int r, int c) {
      const int k = 3 - r - c;
      const double v = k == 0 ? v0 : (k == 1 ? v1 : v2);
      return r == c ? 0.0 : (((c - r + 3) % 3 == 1) ? -v : v);
    };
    // (t^ R)[bi][bj]
    const double tR = hat(tt[0], tt[1], tt[2], bi, 0) * A[bj] + hat(tt[0], tt[1], tt[2], bi, 1) * A[4 + bj] + hat(tt[0], tt[1], tt[2], bi, 2) * A[8 + bj];
    double adj = 0, dlp = 0, dlm = 0;
    const double hu_ij = hat(err[0], err[1], err[2], bi, bj), hw_ij = hat(err[3], err[4], err[5], bi, bj);
    if (i < 3 && j < 3) { adj = Rij; dlp = -hw_ij; }
    else if (i < 3 && j >= 3) { adj = tR; dlp = -hu_ij; }
    else if (i >= 3 && j >= 3) { adj = Rij; dlp = -hw_ij; }
    dlm = -dlp;                                         // dl(-e)
    s_m[0][lane] = adj; s_m[1][lane] = dlp; s_m[4][lane] = dlm;
  }
  wave_lds_sync();
  auto mm = [&](int a, int b) { double s = 0; for (int k = 0; k < 6; ++k) s += s_m[a][6 * i + k] * s_m[b][6 * k + j]; return s; };
  // J1 = third(T21, e) = Adj + 1/2 dl Adj + 1/12 dl dl Adj
  double t1 = on ? mm(1, 0) : 0.0;
  if (on) s_m[2][lane] = t1;
  wave_lds_sync();
  double t2 = on ? mm(1, 2) : 0.0;
  const double J1 = on ? s_m[0][lane] + 0.5 * t1 + (1. / 12.) * t2 : 0.0;
  // J2 = -third(I, -e) = -(I + 1/2 dl(-e) + 1/12 dl(-e)^2)
  double u2 = on ? mm(4, 4) : 0.0;
  const double J2 = on ? -((i == j ? 1.0 : 0.0) + 0.5 * s_m[4][lane] + (1. / 12.) * u2) : 0.0;
  wave_lds_sync();
  if (on) { s_m[3][lane] = J1; s_m[5][lane] = J2; }
  wave_lds_sync();
  // O*J1, O*J2
  if (on) {
    double a1 = 0, a2 = 0;
    for (int k = 0; k < 6; ++k) { a1 += cc.info[6 * i + k] * s_m[3][6 * k + j]; a2 += cc.info[6 * i + k] * s_m[5][6 * k + j]; }
    s_m[6][lane] = a1; s_m[7][lane] = a2;
  }
  wave_lds_sync();
  const int p1 = cc.pose1, p2 = cc.pose2, P = B.P;
  if (on) {
    double s11 = 0, s22 = 0, s12 = 0;
    for (int k = 0; k < 6; ++k) { s11 += s_m[3][6 * k + i] * s_m[6][6 * k + j]; s22 += s_m[5][6 * k + i] * s_m[7][6 * k + j]; s12 += s_m[3][6 * k + i] * s_m[7][6 * k + j]; }
    if (j >= i) { atomic_add_f64(&B.H[blk_index(p1, p1, P) * 36 + lane], s11); atomic_add_f64(&B.H[blk_index(p2, p2, P) * 36 + lane], s22); }
    if (p1 != p2) {
      const bool up = p1 < p2;
      atomic_add_f64(&B.H[(up ? blk_index(p1, p2, P) : blk_index(p2, p1, P)) * 36 + (up ? 6 * i + j : 6 * j + i)], s12);
    }
  }
  if (lane < 6) {
    double s1 = 0, s2 = 0;
    for (int k = 0; k < 6; ++k) { s1 += s_m[3][6 * k + lane] * oe[k]; s2 += s_m[5][6 * k + lane] * oe[k]; }
    atomic_add_f64(&B.bp[6 * p1 + lane], -s1);
    atomic_add_f64(&B.bp[6 * p2 + lane], -s2);
  }
}
// stand-alone launch (windows without landmarks on this rank; otherwise the constraints ride in extra workgroups of
// the landmark kernels)
template <int MODE>
__global__ __launch_bounds__(64) void ba_constraint_kernel(BaDev B) {
  if (B.ctl) { if (B.ctl[1] != 0.0) return; B.lambda = B.ctl[0]; }      // speculative trial: lambda decided on the device, skipped after a rejection
  __shared__ double s_m[8][36];
  ba_constraint_body<MODE>(B, blockIdx.x, s_m);
}

// Levenberg accept / reject of one speculative trial (OptimizationAlgorithmLevenberg::solve, SURVEY.md A.3), on one lane
__device__ __forceinline__ void ba_lm_decide(const BaDev &B, int it) {
  double *rec = B.ctl + 8 + 8 * it;
  const double chi_cur = B.scal[4], fail = B.scal[3];
  double chi_t = 0, scale_l = 0;
  for (int i = 0; i < SC_SLOTS; ++i) { chi_t += B.scal[SC_CHI + i]; scale_l += B.scal[SC_SCL + i]; }
  const double tempChi = fail != 0.0 ? 1.7976931348623157e308 : chi_t;
  const double scale = scale_l + B.scal[2] + 1e-3;
  const double rho = (chi_cur - tempChi) / scale;
  double lambda = B.ctl[0];
  const bool accept = rho > 0 && isfinite(tempChi);
  if (accept) {
    const double q = 2 * rho - 1;
    double alpha = 1. - q * q * q;
    alpha = fmin(alpha, 2. / 3.);
    lambda *= fmax(1. / 3., alpha);
    B.ctl[0] = lambda;
  } else {
    B.ctl[1] = 1.0;
  }
  rec[0] = chi_cur; rec[1] = tempChi; rec[2] = scale; rec[3] = rho; rec[4] = accept ? 1.0 : 0.0; rec[5] = lambda; rec[6] = fail; rec[7] = 1.0;
}

// MODE 0: accumulate reduced system + chi2 at the current state.
// MODE 1: back-substitute landmarks (psi_trial = psi + x_l), scale_l, chi2 at the trial state.
// NW waves (chunks) per workgroup: 4 by default; the host picks more when that brings the number of workgroups down to
// one per CU (at 50 KF / 20k: 1 612 chunks -> 231 workgroups of 7 waves instead of 403 of 4 that load the CUs unevenly).
template <int MODE, int NW, int WC = 1>
__global__ __launch_bounds__(NW * 64, (NW <= 4 && WC == 1) ? 2 : 1) void ba_landmark_kernel(BaDev B) {
  constexpr int NT = NW * 64;
  constexpr int POOL = win_pool_doubles(NW, WC), WMAX = WC == 2 ? WIN_BIG : WIN;
  if (B.ctl) { if (B.ctl[1] != 0.0) return; B.lambda = B.ctl[0]; }      // speculative trial: lambda decided on the device, skipped after a rejection
  const int lane = threadIdx.x & 63;
  __shared__ double s_cons[8][36];
  const int n_lm_blocks = (B.n_chunks + NW - 1) / NW;
  if (B.fuse_cons && (int)blockIdx.x >= n_lm_blocks) {                      // pose-pose constraints: one wave each
    if (threadIdx.x < 64) ba_constraint_body<MODE>(B, blockIdx.x - n_lm_blocks, s_cons);
    return;
  }
  const int chunk = blockIdx.x * NW + (threadIdx.x >> 6);
  const bool wave_valid = chunk < B.n_chunks;                        // wave-uniform
  const int e0 = wave_valid ? B.chunk_start[chunk] : 0, len = wave_valid ? B.chunk_len[chunk] : 0;
  const bool active = lane < len;
#define SVS_STAMP(k) do { if (B.dbg && lane == 0 && wave_valid) B.dbg[DBG_W * (size_t)chunk + (k)] = (long long)wall_clock64(); } while (0)
  SVS_STAMP(0);
  svs_ba_edge ed;
  if (active) ed = B.edges[e0 + lane];
  else { ed.point = -1 - lane; ed.pose = 0; ed.anchor = 0; }
  __shared__ __attribute__((aligned(16))) double s_win[MODE == 0 ? POOL : 1];      // `copies` x [window blocks (stride WBLK) | b_p rows | b_s rows]
  __shared__ __attribute__((aligned(16))) double s_wo[NW * 64 * 18];   // W_obs of every edge lane (MODE 0); before that, hand-over slots of the segmented sums
  __shared__ int s_wmin[NW], s_wmax[NW];
  __shared__ unsigned char s_wrow[MODE == 0 ? WIN_BLOCKS_MAX : 1];
  __shared__ double s_scal[2];      // per-workgroup chi2 (MODE 0) / trial chi2 and scale (MODE 1)
  if (threadIdx.x < 2) s_scal[threadIdx.x] = 0.0;
  if (MODE == 0 && blockIdx.x == 0 && threadIdx.x < SC_N) B.scal[threadIdx.x] = 0.0;      // trial scalars: zeroed here instead of by a memset launch
  if (MODE == 0) {      // the whole pool is zeroed while the edge records are on their way (how much of it the window uses is known after them)
    double2 *w2 = reinterpret_cast<double2 *>(s_win);
    const double2 z2 = {0.0, 0.0};
    for (int i = threadIdx.x; i < POOL / 2; i += NT) w2[i] = z2;
  }
#define SVS_SUBSTAMP(k) do { if (B.dbg) { __builtin_amdgcn_s_waitcnt(0x0F70); if (lane == 0 && wave_valid) B.dbg[DBG_W * (size_t)chunk + DBG_N + (k)] = (long long)wall_clock64(); } } while (0)
  SVS_SUBSTAMP(4);
  // the state gathers depend on the record alone: in flight while the window is set up (three barriers further down)
  double psi[3] = {1, 1, 1}, To[12], Ta[12];
  if (active) {
#pragma unroll
    for (int i = 0; i < 3; ++i) psi[i] = B.psi[3 * (size_t)ed.point + i];
#pragma unroll
    for (int i = 0; i < 12; ++i) { To[i] = B.poses[12 * (size_t)ed.pose + i]; Ta[i] = B.poses[12 * (size_t)ed.anchor + i]; }
  }
  SVS_SUBSTAMP(5);
  int pmin = 0, win = 1, nblk = 1, cstride = 1, copies = 1;
  if (MODE == 0) {
    int mn = active ? min(ed.pose, ed.anchor) : 0x7fffffff, mx = active ? max(ed.pose, ed.anchor) : -1;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { mn = min(mn, __shfl_xor(mn, o, 64)); mx = max(mx, __shfl_xor(mx, o, 64)); }
    if (lane == 0) { s_wmin[threadIdx.x >> 6] = mn; s_wmax[threadIdx.x >> 6] = mx; }
    __syncthreads();
    SVS_SUBSTAMP(6);
    pmin = s_wmin[0];
    int pmax = s_wmax[0];
#pragma unroll
    for (int k = 1; k < NW; ++k) { pmin = min(pmin, s_wmin[k]); pmax = max(pmax, s_wmax[k]); }
    if (pmin != 0x7fffffff) {
      win = min(pmax - pmin + 1, WMAX) + 1;
      do {                                                  // (WMAX fits the pool once; the loop is the guarantee, not the rule)
        --win;
        nblk = win * (win + 1) / 2;
        cstride = (nblk * WBLK + 12 * win) | 1;             // odd: the copies start in different banks
      } while (cstride > POOL && win > 1);
      copies = max(1, min(WCOPIES_MAX, POOL / cstride));
    }
    if (threadIdx.x < nblk) {                               // block row of every packed window block (for the flush, behind the next barrier)
      int wi = 0, rem = threadIdx.x;
      while (rem >= win - wi) { rem -= win - wi; ++wi; }
      s_wrow[threadIdx.x] = (unsigned char)wi;
    }
  }
  SVS_SUBSTAMP(7);
  // segment (= landmark) bounds inside the wave
  const int prev_point = __shfl_up(ed.point, 1, 64);
  const bool head = lane == 0 || prev_point != ed.point;
  const unsigned long long heads = __ballot(head);
  const unsigned long long le_mask = (lane == 63) ? ~0ull : ((1ull << (lane + 1)) - 1ull);
  const int seg_begin = 63 - __clzll((long long)(heads & le_mask));
  const unsigned long long gt = (lane == 63) ? 0ull : (heads & ~le_mask);
  const int seg_end = gt ? (__ffsll((long long)gt) - 2) : 63;
  int maxlen = seg_end - seg_begin + 1;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) maxlen = max(maxlen, __shfl_xor(maxlen, o, 64));
  // The waves of a workgroup share the CU's LDS pipeline and meet at the flush barrier: the ones holding the largest landmarks (most
  // pair rounds) are the critical path, so they get the higher issue priority
  if (MODE == 0) {
    const int ml = __builtin_amdgcn_readfirstlane(maxlen);
    if (ml >= 7) __builtin_amdgcn_s_setprio(3);
    else if (ml >= 5) __builtin_amdgcn_s_setprio(2);
    else if (ml >= 4) __builtin_amdgcn_s_setprio(1);
  }

  const int P = B.P;
  EdgeCore lin;
  const bool self = active && ed.pose == ed.anchor;
  if (active) {
    linearize_edge(psi, To, Ta, ed, B.cam, B.delta, B.robust, lin);
  } else {
#pragma unroll
    for (int i = 0; i < 9; ++i) { lin.R[i] = 0; lin.A[i] = 0; lin.D[i] = 0; }
#pragma unroll
    for (int i = 0; i < 3; ++i) { lin.xa[i] = 0; lin.y[i] = 0; lin.g[i] = 0; }
    lin.rho0 = 0;
  }
  SVS_STAMP(1);
  // one global atomic per WORKGROUP for the scalar sums: same-address f64 atomics serialise in L2 (~20 ns each), and one
  // per wave cost more than the rest of the back-substitution kernel
  if (MODE == 0) {
    const double c = wave_sum(lin.rho0);
    if (lane == 0 && c != 0.0) lds_add_f64(&s_scal[0], c);      // window init barrier above ordered the zeroing
  }
  // observer role: this lane owns pose ed.pose of its landmark.  A self edge (observer == anchor: R = I, y = x_a up to
  // rounding) has J_obs + J_anc = 0: it contributes to H_ll / b_l only, plus -- in G2O_LITERAL mode, SURVEY.md B-7 --
  // the slot terms M_oo + M_aa + sym(M_oa) on the anchor's diagonal block, which collapse to M_aa = Ea^T A Ea
  // (differences are O(eps |M|)); its b and W slot terms cancel.
  const bool obs_role = active && !self;
  const bool self_lit = self && B.self_mode == 0;

  // ---- per landmark sums, one segmented reduction: H_ll = sum D^T A D, b_l = -sum D^T g, and -- because x_a is common
  //      to all edges of a landmark -- W_anc = -Ea^T (sum R^T A D), M_aa = Ea^T (sum R^T A R) Ea, b_anc = Ea^T (sum R^T g)
  double Bm[9];
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) Bm[3 * i + j] = lin.A[3 * i] * lin.D[j] + lin.A[3 * i + 1] * lin.D[3 + j] + lin.A[3 * i + 2] * lin.D[6 + j];
  constexpr int NRED = MODE == 0 ? 27 : 18;
  double red[NRED];      // [0..5] H_ll upper, [6..8] b_l, [9..17] S_RB = sum R^T Bm, (MODE 0:) [18..23] S_RAR upper, [24..26] S_Rg
  {
    int k = 0;
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
      for (int j = i; j < 3; ++j) red[k++] = lin.D[i] * Bm[j] + lin.D[3 + i] * Bm[3 + j] + lin.D[6 + i] * Bm[6 + j];
#pragma unroll
    for (int i = 0; i < 3; ++i) red[6 + i] = -(lin.D[i] * lin.g[0] + lin.D[3 + i] * lin.g[1] + lin.D[6 + i] * lin.g[2]);
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
      for (int j = 0; j < 3; ++j) red[9 + 3 * i + j] = obs_role ? lin.R[i] * Bm[j] + lin.R[3 + i] * Bm[3 + j] + lin.R[6 + i] * Bm[6 + j] : 0.0;
    if (MODE == 0) {
      double AR[9];
#pragma unroll
      for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) AR[3 * i + j] = lin.A[3 * i] * lin.R[j] + lin.A[3 * i + 1] * lin.R[3 + j] + lin.A[3 * i + 2] * lin.R[6 + j];
      const bool in_maa = obs_role || self_lit;
      k = 18;
#pragma unroll
      for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = i; j < 3; ++j) red[k++] = in_maa ? lin.R[i] * AR[j] + lin.R[3 + i] * AR[3 + j] + lin.R[6 + i] * AR[6 + j] : 0.0;
#pragma unroll
      for (int i = 0; i < 3; ++i) red[24 + i] = obs_role ? lin.R[i] * lin.g[0] + lin.R[3 + i] * lin.g[1] + lin.R[6 + i] * lin.g[2] : 0.0;
    }
  }
  SVS_STAMP(2);
  seg_allreduce<NRED, 18>(red, lane, seg_begin, seg_end, maxlen, s_wo + (threadIdx.x >> 6) * 64 * 18);
  SVS_STAMP(3);
  double Di[9], bl[3] = {red[6], red[7], red[8]};
  {
    const double a00 = red[0] + B.lambda, a01 = red[1], a02 = red[2], a11 = red[3] + B.lambda, a12 = red[4], a22 = red[5] + B.lambda;
    // closed-form inverse of the symmetric 3x3 (Eigen fixed-size inverse = cofactors / det)
    const double c00 = a11 * a22 - a12 * a12, c01 = a12 * a02 - a01 * a22, c02 = a01 * a12 - a11 * a02;
    const double id = 1.0 / (a00 * c00 + a01 * c01 + a02 * c02);
    Di[0] = c00 * id; Di[1] = c01 * id; Di[2] = c02 * id;
    Di[3] = Di[1]; Di[4] = (a00 * a22 - a02 * a02) * id; Di[5] = (a02 * a01 - a00 * a12) * id;
    Di[6] = Di[2]; Di[7] = Di[5]; Di[8] = (a00 * a11 - a01 * a01) * id;
  }
  double Db[3];
#pragma unroll
  for (int i = 0; i < 3; ++i) Db[i] = Di[3 * i] * bl[0] + Di[3 * i + 1] * bl[1] + Di[3 * i + 2] * bl[2];
  // W_obs = Eo^T Bm = [Bm ; y x Bm(:,c)]  (0 for a self edge);  W_anc = -Ea^T S_RB = -[S_RB ; x_a x S_RB(:,c)], rebuilt where needed
  double Wo[18];
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    double t0, t1, t2;
    cross3(lin.y, Bm[c], Bm[3 + c], Bm[6 + c], t0, t1, t2);
    Wo[c] = obs_role ? Bm[c] : 0.0; Wo[3 + c] = obs_role ? Bm[3 + c] : 0.0; Wo[6 + c] = obs_role ? Bm[6 + c] : 0.0;
    Wo[9 + c] = obs_role ? t0 : 0.0; Wo[12 + c] = obs_role ? t1 : 0.0; Wo[15 + c] = obs_role ? t2 : 0.0;
  }
  auto make_WA = [&](double (&WA)[18]) {
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      double t0, t1, t2;
      cross3(lin.xa, red[9 + c], red[12 + c], red[15 + c], t0, t1, t2);
      WA[c] = -red[9 + c]; WA[3 + c] = -red[12 + c]; WA[6 + c] = -red[15 + c];
      WA[9 + c] = -t0; WA[12 + c] = -t1; WA[15 + c] = -t2;
    }
  };
  SVS_STAMP(4);
  const int anchor = ed.anchor;

  if (MODE == 1) {
    // x_l = D^-1 (b_l - sum_i W_i^T x_i - W_A^T x_A)
    double c[3] = {0, 0, 0};
    if (obs_role) {
#pragma unroll
      for (int j = 0; j < 3; ++j)
#pragma unroll
        for (int i = 0; i < 6; ++i) c[j] += Wo[3 * i + j] * B.x[6 * ed.pose + i];
    }
    __builtin_amdgcn_wave_barrier();      // every lane has read its slot of the first hand-over
    seg_allreduce<3, 3>(c, lane, seg_begin, seg_end, maxlen, s_wo + (threadIdx.x >> 6) * 64 * 18);
    double xl[3] = {0, 0, 0};
    if (active) {
      double WA[18];
      make_WA(WA);
#pragma unroll
      for (int j = 0; j < 3; ++j) {
        double s = bl[j] - c[j];
#pragma unroll
        for (int i = 0; i < 6; ++i) s -= WA[3 * i + j] * B.x[6 * anchor + i];
        c[j] = s;
      }
#pragma unroll
      for (int i = 0; i < 3; ++i) xl[i] = Di[3 * i] * c[0] + Di[3 * i + 1] * c[1] + Di[3 * i + 2] * c[2];
    }
    double npsi[3] = {psi[0] + xl[0], psi[1] + xl[1], psi[2] + xl[2]};   // G2oVertexPointXYZ::oplusImpl
    double sc = 0, chi = 0;
    if (active) {
      if (head) {
#pragma unroll
        for (int i = 0; i < 3; ++i) { B.psi_trial[3 * (size_t)ed.point + i] = npsi[i]; sc += xl[i] * (B.lambda * xl[i] + bl[i]); }
      }
      double Tno[12], Tna[12];
#pragma unroll
      for (int i = 0; i < 12; ++i) { Tno[i] = B.poses_trial[12 * (size_t)ed.pose + i]; Tna[i] = B.poses_trial[12 * (size_t)anchor + i]; }
      chi = edge_chi2(npsi, Tno, Tna, ed, B.cam, B.delta, B.robust);
    }
    sc = wave_sum(sc);
    chi = wave_sum(chi);
    __syncthreads();                                   // s_scal zeroed
    if (lane == 0) { lds_add_f64(&s_scal[0], chi); lds_add_f64(&s_scal[1], sc); }
    __syncthreads();
    if (threadIdx.x == 0) { atomic_add_f64(&B.scal[SC_CHI + (blockIdx.x & (SC_SLOTS - 1))], s_scal[0]); atomic_add_f64(&B.scal[SC_SCL + (blockIdx.x & (SC_SLOTS - 1))], s_scal[1]); }
    return;
  }

  // ---- MODE 0: reduced camera system -------------------------------------------------------
  // A block (pi <= pj) of the reduced system lives either in the workgroup's LDS window or (out of window) in global memory.  The
  // test is made ONCE per block and the six values of a block row are added under one branch: the per-element form of this
  // (a divergent `if` around every one of the ~270 adds of a lane) cost as many scalar instructions as the kernel has vector ones
  // (PMC: 2440 SALU vs 2490 VALU per wave, profiles/r2_notes.md).
  // (destinations are kept as INDICES into s_win / B.H, not as pointers: a pointer that may point to either would be a flat pointer and
  //  every add a flat atomic)
  const int lm_ord = __popcll(heads & le_mask) - 1;                            // ordinal of this lane's landmark in the wave
  const int my_copy = lm_ord % copies, my_base = my_copy * cstride, vec_base = my_base + nblk * WBLK;
  struct Dst { bool in_lds; int lds; long glb; };
  auto blk_dst = [&](int pi, int pj) __attribute__((always_inline)) {
    const int wi = pi - pmin, wj = pj - pmin;
    Dst d;
    d.in_lds = wj < win;
    d.lds = d.in_lds ? my_base + win_blk(wi, wj, win) * WBLK : 0;
    d.glb = d.in_lds ? 0 : blk_index(pi, pj, B.P) * 36;
    return d;
  };
  // v[c] -> element (r, c) of the block (stride 1), or -- transposed store -- element (c, r) (stride 6)
  auto add_row6 = [&](const Dst &d, int first, int stride, const double (&v)[6], int c0) __attribute__((always_inline)) {
    if (d.in_lds) {
#pragma unroll
      for (int c = 0; c < 6; ++c) if (c >= c0) lds_add_f64(&s_win[d.lds + first + stride * c], v[c]);
    } else {
#pragma unroll
      for (int c = 0; c < 6; ++c) if (c >= c0) atomic_add_f64(&B.H[d.glb + first + stride * c], v[c]);
    }
  };
  auto add_vec6 = [&](int which, int p, const double (&v)[6]) __attribute__((always_inline)) {      // which: 0 = b_p, 1 = b_s
    const int wp = p - pmin;
    if (wp < win) {
#pragma unroll
      for (int c = 0; c < 6; ++c) lds_add_f64(&s_win[vec_base + (which * win + wp) * 6 + c], v[c]);
    } else {
      double *g = (which ? B.bs : B.bp) + 6 * p;
#pragma unroll
      for (int c = 0; c < 6; ++c) atomic_add_f64(g + c, v[c]);
    }
  };
  // (1) anchor block, once per landmark: Ea^T S_RAR Ea - (W_A D^-1) W_A^T,  b_anc = Ea^T S_Rg,  Schur rhs W_A D^-1 b_l
  if (active && lane == seg_end) {      // the lane that holds the landmark's complete sums
    double WA[18], WAD[18], SR[9], Maa[36];
    make_WA(WA);
    SR[0] = red[18]; SR[1] = red[19]; SR[2] = red[20]; SR[3] = red[19]; SR[4] = red[21]; SR[5] = red[22]; SR[6] = red[20]; SR[7] = red[22]; SR[8] = red[23];
    sym_block(SR, lin.xa, Maa);
#pragma unroll
    for (int i = 0; i < 6; ++i)
#pragma unroll
      for (int j = 0; j < 3; ++j) WAD[3 * i + j] = WA[3 * i] * Di[j] + WA[3 * i + 1] * Di[3 + j] + WA[3 * i + 2] * Di[6 + j];
    const Dst dst = blk_dst(anchor, anchor);
#pragma unroll
    for (int r = 0; r < 6; ++r) {
      double v[6];
#pragma unroll
      for (int c = 0; c < 6; ++c) v[c] = c >= r ? Maa[6 * r + c] - (WAD[3 * r] * WA[3 * c] + WAD[3 * r + 1] * WA[3 * c + 1] + WAD[3 * r + 2] * WA[3 * c + 2]) : 0.0;
      add_row6(dst, 6 * r, 1, v, r);
    }
    double t0, t1, t2;
    cross3(lin.xa, red[24], red[25], red[26], t0, t1, t2);
    const double ba[6] = {red[24], red[25], red[26], t0, t1, t2};
    double bsv[6];
#pragma unroll
    for (int r = 0; r < 6; ++r) bsv[r] = WA[3 * r] * Db[0] + WA[3 * r + 1] * Db[1] + WA[3 * r + 2] * Db[2];
    add_vec6(0, anchor, ba);
    add_vec6(1, anchor, bsv);
  }
  SVS_STAMP(5);
  // (2) observer part: blocks (i,i), (i,A), b_i;  W_obs is parked in LDS for the pair phase
  double *my_wo = s_wo + ((threadIdx.x >> 6) * 64 + lane) * 18;
#pragma unroll
  for (int i = 0; i < 18; ++i) my_wo[i] = Wo[i];
  double WoD[18];
#pragma unroll
  for (int i = 0; i < 6; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) WoD[3 * i + j] = Wo[3 * i] * Di[j] + Wo[3 * i + 1] * Di[3 + j] + Wo[3 * i + 2] * Di[6 + j];
  if (obs_role) {
    const int pi = ed.pose;
    {
      double Moo[36];
      sym_block(lin.A, lin.y, Moo);                           // M_oo = Eo^T A Eo
      const Dst dst = blk_dst(pi, pi);
#pragma unroll
      for (int r = 0; r < 6; ++r) {
        double v[6];
#pragma unroll
        for (int c = 0; c < 6; ++c) v[c] = c >= r ? Moo[6 * r + c] - (WoD[3 * r] * Wo[3 * c] + WoD[3 * r + 1] * Wo[3 * c + 1] + WoD[3 * r + 2] * Wo[3 * c + 2]) : 0.0;
        add_row6(dst, 6 * r, 1, v, r);
      }
    }
    {
      double AR[9], Noa[36], WA[18];
      make_WA(WA);
#pragma unroll
      for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) AR[3 * i + j] = lin.A[3 * i] * lin.R[j] + lin.A[3 * i + 1] * lin.R[3 + j] + lin.A[3 * i + 2] * lin.R[6 + j];
      cross_block(AR, lin.y, lin.xa, Noa);                    // M_oa = -Eo^T (A R) Ea
      const bool up = pi < anchor;
      const Dst dst = blk_dst(up ? pi : anchor, up ? anchor : pi);
      const int rs = up ? 6 : 1, cstr = up ? 1 : 6;           // element (r, c) of M goes to (r, c) of block (pi, anchor) or to (c, r) of block (anchor, pi)
#pragma unroll
      for (int r = 0; r < 6; ++r) {
        double v[6];
#pragma unroll
        for (int c = 0; c < 6; ++c) v[c] = -Noa[6 * r + c] - (WoD[3 * r] * WA[3 * c] + WoD[3 * r + 1] * WA[3 * c + 1] + WoD[3 * r + 2] * WA[3 * c + 2]);
        add_row6(dst, rs * r, cstr, v, 0);
      }
    }
    double u0, u1, u2;
    cross3(lin.y, lin.g[0], lin.g[1], lin.g[2], u0, u1, u2);
    const double bo[6] = {-lin.g[0], -lin.g[1], -lin.g[2], -u0, -u1, -u2};    // b_obs = -Eo^T g
    double bsv[6];
#pragma unroll
    for (int r = 0; r < 6; ++r) bsv[r] = Wo[3 * r] * Db[0] + Wo[3 * r + 1] * Db[1] + Wo[3 * r + 2] * Db[2];
    add_vec6(0, pi, bo);
    add_vec6(1, pi, bsv);
  }
  SVS_STAMP(6);
  // (3) observer-observer pairs of a landmark, circulant schedule: in round r the edge with local index a
  //     pairs with (a + r) mod m, so all m lanes of a landmark work for floor(m/2) rounds (instead of one
  //     lane-partner distance per round over m-1 rounds).  -(W_a D^-1) W_b^T goes to block (min, max).
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  {
    // The circulant runs over the landmark's OBSERVERS only: its self edge (observer == anchor, at most one per landmark: one edge
    // per (point, keyframe)) has no W_obs and would only lengthen the schedule -- a landmark seen from its anchor and four more
    // keyframes takes 2 rounds instead of 2.5 -> 3, and the wave runs as many rounds as its largest landmark needs.
    const unsigned long long seg_mask = (seg_end == 63 ? ~0ull : ((1ull << (seg_end + 1)) - 1ull)) & ~((1ull << seg_begin) - 1ull);
    const unsigned long long self_in_seg = __ballot(active && !obs_role) & seg_mask;      // (a non-literal self edge included: it pairs with nobody)
    const int self_pos = self_in_seg ? (__ffsll((long long)self_in_seg) - 1) - seg_begin : 64;
    const int m = (seg_end - seg_begin + 1) - (self_in_seg ? 1 : 0);
    const int a_loc = (lane - seg_begin) - ((lane - seg_begin) > self_pos ? 1 : 0);
    int rounds = active ? (m >> 1) : 0;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) rounds = max(rounds, __shfl_xor(rounds, o, 64));
    const double *wave_wo = s_wo + (threadIdx.x >> 6) * 64 * 18;
    if (B.dbg && wave_valid && lane == 0) B.dbg[DBG_W * (size_t)chunk + DBG_N + 3] = rounds;
    // LDS operations of a wave complete in order: a partner fetch issued right behind the 36 adds of the previous round would wait for
    // all of them.  So the partner of round r+1 (its pose, role and W_obs) is fetched BEFORE the adds of round r are issued, and the
    // products of round r are formed while that fetch (and the adds of round r-1 in front of it) drain.
    auto partner = [&](int r, int &pj, bool &on, double (&Wj)[18]) __attribute__((always_inline)) {
      int b_loc = a_loc + r;
      if (b_loc >= m) b_loc -= m;
      const int lane_b = min(seg_begin + b_loc + (b_loc >= self_pos ? 1 : 0), 63);
      pj = __shfl(ed.pose, lane_b, 64);
      on = obs_role && 2 * r <= m && !(2 * r == m && a_loc >= r);
      const double *wj = wave_wo + lane_b * 18;
#pragma unroll
      for (int i = 0; i < 18; ++i) Wj[i] = wj[i];
    };
    int pj_n = 0; bool on_n = false; double W_n[18];
    if (rounds >= 1) partner(1, pj_n, on_n, W_n);
    for (int r = 1; r <= rounds; ++r) {
      const int pj = pj_n; const bool on = on_n;
      double Wj[18];
#pragma unroll
      for (int i = 0; i < 18; ++i) Wj[i] = W_n[i];
      if (r < rounds) partner(r + 1, pj_n, on_n, W_n);
      if (on) {
        const bool up = ed.pose < pj;
        const Dst dst = blk_dst(up ? ed.pose : pj, up ? pj : ed.pose);
        const int rs = up ? 6 : 1, cstr = up ? 1 : 6;
#pragma unroll
        for (int rr = 0; rr < 6; ++rr) {
          double v[6];
#pragma unroll
          for (int c = 0; c < 6; ++c) v[c] = -(WoD[3 * rr] * Wj[3 * c] + WoD[3 * rr + 1] * Wj[3 * c + 1] + WoD[3 * rr + 2] * Wj[3 * c + 2]);
          add_row6(dst, rs * rr, cstr, v, 0);
        }
      }
    }
  }
  SVS_STAMP(7);
  // flush the LDS window: one global atomic per touched element per workgroup
  __syncthreads();
  SVS_STAMP(8);
  if (threadIdx.x == 0 && s_scal[0] != 0.0) atomic_add_f64(B.chi2_cur + (blockIdx.x & (SC_SLOTS - 1)), s_scal[0]);
  if (pmin != 0x7fffffff) {
    for (int i = threadIdx.x; i < nblk * 36; i += NT) {
      const int wb = i / 36, rc = i - wb * 36;
      double v = s_win[wb * WBLK + rc];
      for (int k = 1; k < copies; ++k) v += s_win[k * cstride + wb * WBLK + rc];
      if (v != 0.0) {
        const int wi = s_wrow[wb], pi = pmin + wi, pj = pmin + wi + (wb - win_blk(wi, wi, win));
        if (pj < P) atomic_add_f64(&B.H[blk_index(pi, pj, P) * 36 + rc], v);
      }
    }
    for (int i = threadIdx.x; i < 2 * win * 6; i += NT) {
      double v = s_win[nblk * WBLK + i];
      for (int k = 1; k < copies; ++k) v += s_win[k * cstride + nblk * WBLK + i];
      if (v != 0.0) {
        const int which = i / (win * 6), rest = i - which * win * 6, wp = rest / 6, r = rest - wp * 6;
        if (pmin + wp < P) atomic_add_f64((which ? B.bs : B.bp) + 6 * (pmin + wp) + r, v);
      }
    }
  }
  SVS_STAMP(DBG_N - 1);
  if (B.dbg && wave_valid) {      // structure words of the timeline (debug only)
    const bool tail = active && lane == seg_end;
    int m_obs = 0, m_anc = 0;
    for (int j = 0; j < 64; ++j) {
      const int pj = __shfl(ed.pose, j, 64), aj = __shfl(ed.anchor, j, 64), cj = __shfl(my_copy, j, 64);
      const int oj = __shfl((int)obs_role, j, 64), tj = __shfl((int)tail, j, 64);
      if (obs_role && oj && pj == ed.pose && cj == my_copy) ++m_obs;
      if (tail && tj && aj == ed.anchor && cj == my_copy) ++m_anc;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { m_obs = max(m_obs, __shfl_xor(m_obs, o, 64)); m_anc = max(m_anc, __shfl_xor(m_anc, o, 64)); }
    const unsigned long long act_mask = __ballot(active);
    if (lane == 0) {
      B.dbg[DBG_W * (size_t)chunk + DBG_N + 0] = __popcll(heads & act_mask) * 100 + copies;      // landmarks * 100 + window copies
      B.dbg[DBG_W * (size_t)chunk + DBG_N + 1] = m_obs;
      B.dbg[DBG_W * (size_t)chunk + DBG_N + 2] = m_anc;
    }
  }
}

// ---- landmarks with more than 64 observations -------------------------------------------------------------------
// The reference adds an observation edge for every window pose in a point's vis_set, without a cap (slam_graph.cpp:1001-1027):
// in a loop a point is easily seen from more than 64 of the 230 window poses.  Such a landmark does not fit the
// one-wave-per-chunk kernel above; it gets ONE WORKGROUP of WIDE_THREADS lanes (lane = edge, up to WIDE_THREADS observations =
// more than the 256 poses a window can hold).  Same algebra as ba_landmark_kernel (compact edge blocks, per-landmark sums of
// 27 values, 3x3 closed-form inverse, circulant observer pairs with W_obs parked in LDS); sums go through the workgroup,
// blocks straight to global atomics -- these landmarks are few.
constexpr int WIDE_THREADS = 256;
template <int N>
__device__ __forceinline__ void wide_block_sum(double (&v)[N], double *s_red /* [WIDE_THREADS / 64][N] */) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int i = 0; i < N; ++i) {
    const double w = wave_sum(v[i]);
    if (lane == 0) s_red[wave * N + i] = w;
  }
  __syncthreads();
#pragma unroll
  for (int i = 0; i < N; ++i) {
    double t = 0;
#pragma unroll
    for (int w = 0; w < WIDE_THREADS / 64; ++w) t += s_red[w * N + i];
    v[i] = t;
  }
  __syncthreads();
}
template <int MODE>
__global__ __launch_bounds__(WIDE_THREADS) void ba_wide_landmark_kernel(BaDev B) {
  if (B.ctl) { if (B.ctl[1] != 0.0) return; B.lambda = B.ctl[0]; }
  __shared__ double s_red[(WIDE_THREADS / 64) * 27];
  __shared__ __attribute__((aligned(16))) double s_wo[MODE == 0 ? WIDE_THREADS * 18 : 1];
  __shared__ int s_pose[WIDE_THREADS], s_role[WIDE_THREADS];
  const int tid = threadIdx.x;
  // MODE 0: WIDE_SPLIT workgroups per landmark.  Every one of them forms the landmark's sums, D^-1 and the W blocks (cheap); the
  // landmark's own blocks (chi2, anchor, observer diagonal / anchor coupling, b) are added by part 0, the m (m - 1) / 2 observer pairs
  // -- 16 000 blocks of 36 global atomics at m = 180, 0.9 ms when one workgroup walked them -- are dealt round by round to the parts
  const int split = MODE == 0 ? B.wide_split : 1, lmi = blockIdx.x / split, part = blockIdx.x - lmi * split;
  const int e0 = B.wide_start[lmi], m = B.wide_len[lmi];
  const bool active = tid < m;
  svs_ba_edge ed;
  if (active) ed = B.edges[e0 + tid];
  else { ed.point = -1; ed.pose = 0; ed.anchor = 0; }
  {                                                     // every edge of the landmark has the same anchor / point: inactive lanes take
    __shared__ int s_ap[2];                             // them from the first edge
    if (tid == 0) { s_ap[0] = ed.anchor; s_ap[1] = ed.point; }
    __syncthreads();
    ed.anchor = s_ap[0]; if (!active) ed.point = s_ap[1];
  }
  const int anchor = ed.anchor;
  double psi[3], To[12], Ta[12];
  EdgeCore lin;
#pragma unroll
  for (int i = 0; i < 3; ++i) psi[i] = B.psi[3 * (size_t)ed.point + i];
#pragma unroll
  for (int i = 0; i < 12; ++i) { To[i] = B.poses[12 * (size_t)ed.pose + i]; Ta[i] = B.poses[12 * (size_t)anchor + i]; }
  linearize_edge(psi, To, Ta, ed, B.cam, B.delta, B.robust, lin);       // inactive lanes: a copy of a valid geometry, masked below
  const bool self = active && ed.pose == anchor;
  const bool obs_role = active && !self;
  const bool self_lit = self && B.self_mode == 0;
  if (!active) {
#pragma unroll
    for (int i = 0; i < 9; ++i) { lin.A[i] = 0; }
#pragma unroll
    for (int i = 0; i < 3; ++i) lin.g[i] = 0;
    lin.rho0 = 0;
  }
  double Bm[9];
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) Bm[3 * i + j] = lin.A[3 * i] * lin.D[j] + lin.A[3 * i + 1] * lin.D[3 + j] + lin.A[3 * i + 2] * lin.D[6 + j];
  constexpr int NRED = MODE == 0 ? 27 : 18;
  double red[27];
  {
    int k = 0;
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
      for (int j = i; j < 3; ++j) red[k++] = lin.D[i] * Bm[j] + lin.D[3 + i] * Bm[3 + j] + lin.D[6 + i] * Bm[6 + j];
#pragma unroll
    for (int i = 0; i < 3; ++i) red[6 + i] = -(lin.D[i] * lin.g[0] + lin.D[3 + i] * lin.g[1] + lin.D[6 + i] * lin.g[2]);
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
      for (int j = 0; j < 3; ++j) red[9 + 3 * i + j] = obs_role ? lin.R[i] * Bm[j] + lin.R[3 + i] * Bm[3 + j] + lin.R[6 + i] * Bm[6 + j] : 0.0;
    double AR[9];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
      for (int j = 0; j < 3; ++j) AR[3 * i + j] = lin.A[3 * i] * lin.R[j] + lin.A[3 * i + 1] * lin.R[3 + j] + lin.A[3 * i + 2] * lin.R[6 + j];
    const bool in_maa = obs_role || self_lit;
    k = 18;
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
      for (int j = i; j < 3; ++j) red[k++] = in_maa ? lin.R[i] * AR[j] + lin.R[3 + i] * AR[3 + j] + lin.R[6 + i] * AR[6 + j] : 0.0;
#pragma unroll
    for (int i = 0; i < 3; ++i) red[24 + i] = obs_role ? lin.R[i] * lin.g[0] + lin.R[3 + i] * lin.g[1] + lin.R[6 + i] * lin.g[2] : 0.0;
  }
  (void)NRED;
  wide_block_sum<27>(red, s_red);
  double Di[9], bl[3] = {red[6], red[7], red[8]};
  {
    const double a00 = red[0] + B.lambda, a01 = red[1], a02 = red[2], a11 = red[3] + B.lambda, a12 = red[4], a22 = red[5] + B.lambda;
    const double c00 = a11 * a22 - a12 * a12, c01 = a12 * a02 - a01 * a22, c02 = a01 * a12 - a11 * a02;
    const double id = 1.0 / (a00 * c00 + a01 * c01 + a02 * c02);
    Di[0] = c00 * id; Di[1] = c01 * id; Di[2] = c02 * id;
    Di[3] = Di[1]; Di[4] = (a00 * a22 - a02 * a02) * id; Di[5] = (a02 * a01 - a00 * a12) * id;
    Di[6] = Di[2]; Di[7] = Di[5]; Di[8] = (a00 * a11 - a01 * a01) * id;
  }
  double Db[3];
#pragma unroll
  for (int i = 0; i < 3; ++i) Db[i] = Di[3 * i] * bl[0] + Di[3 * i + 1] * bl[1] + Di[3 * i + 2] * bl[2];
  double Wo[18];
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    double t0, t1, t2;
    cross3(lin.y, Bm[c], Bm[3 + c], Bm[6 + c], t0, t1, t2);
    Wo[c] = obs_role ? Bm[c] : 0.0; Wo[3 + c] = obs_role ? Bm[3 + c] : 0.0; Wo[6 + c] = obs_role ? Bm[6 + c] : 0.0;
    Wo[9 + c] = obs_role ? t0 : 0.0; Wo[12 + c] = obs_role ? t1 : 0.0; Wo[15 + c] = obs_role ? t2 : 0.0;
  }
  double WA[18];
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    double t0, t1, t2;
    cross3(lin.xa, red[9 + c], red[12 + c], red[15 + c], t0, t1, t2);
    WA[c] = -red[9 + c]; WA[3 + c] = -red[12 + c]; WA[6 + c] = -red[15 + c];
    WA[9 + c] = -t0; WA[12 + c] = -t1; WA[15 + c] = -t2;
  }
  if (MODE == 1) {
    double c[3] = {0, 0, 0};
    if (obs_role) {
#pragma unroll
      for (int j = 0; j < 3; ++j)
#pragma unroll
        for (int i = 0; i < 6; ++i) c[j] += Wo[3 * i + j] * B.x[6 * ed.pose + i];
    }
    wide_block_sum<3>(c, s_red);
    double xl[3];
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      double sj = bl[j] - c[j];
#pragma unroll
      for (int i = 0; i < 6; ++i) sj -= WA[3 * i + j] * B.x[6 * anchor + i];
      c[j] = sj;
    }
#pragma unroll
    for (int i = 0; i < 3; ++i) xl[i] = Di[3 * i] * c[0] + Di[3 * i + 1] * c[1] + Di[3 * i + 2] * c[2];
    const double npsi[3] = {psi[0] + xl[0], psi[1] + xl[1], psi[2] + xl[2]};
    double sc[2] = {0, 0};      // chi2 at the trial state, x_l (lambda x_l + b_l)
    if (tid == 0) {
#pragma unroll
      for (int i = 0; i < 3; ++i) { B.psi_trial[3 * (size_t)ed.point + i] = npsi[i]; sc[1] += xl[i] * (B.lambda * xl[i] + bl[i]); }
    }
    if (active) {
      double Tno[12], Tna[12];
#pragma unroll
      for (int i = 0; i < 12; ++i) { Tno[i] = B.poses_trial[12 * (size_t)ed.pose + i]; Tna[i] = B.poses_trial[12 * (size_t)anchor + i]; }
      sc[0] = edge_chi2(npsi, Tno, Tna, ed, B.cam, B.delta, B.robust);
    }
    wide_block_sum<2>(sc, s_red);
    if (tid == 0) { atomic_add_f64(&B.scal[SC_CHI + (blockIdx.x & (SC_SLOTS - 1))], sc[0]); atomic_add_f64(&B.scal[SC_SCL + (blockIdx.x & (SC_SLOTS - 1))], sc[1]); }
    return;
  }
  // ---- MODE 0 ----
  if (part == 0) {            // (workgroup-uniform)
    double c1[1] = {lin.rho0};
    wide_block_sum<1>(c1, s_red);
    if (tid == 0 && c1[0] != 0.0) atomic_add_f64(B.chi2_cur + (blockIdx.x & (SC_SLOTS - 1)), c1[0]);
  }
  auto add_blk = [&](int pi, int pj, int rc, double v) { atomic_add_f64(&B.H[blk_index(pi, pj, B.P) * 36 + rc], v); };
  if (tid == 0 && part == 0) {             // anchor block, once: Ea^T S_RAR Ea - (W_A D^-1) W_A^T, b_anc, Schur rhs
    double WAD[18], SR[9], Maa[36];
    SR[0] = red[18]; SR[1] = red[19]; SR[2] = red[20]; SR[3] = red[19]; SR[4] = red[21]; SR[5] = red[22]; SR[6] = red[20]; SR[7] = red[22]; SR[8] = red[23];
    sym_block(SR, lin.xa, Maa);
#pragma unroll
    for (int i = 0; i < 6; ++i)
#pragma unroll
      for (int j = 0; j < 3; ++j) WAD[3 * i + j] = WA[3 * i] * Di[j] + WA[3 * i + 1] * Di[3 + j] + WA[3 * i + 2] * Di[6 + j];
#pragma unroll
    for (int r = 0; r < 6; ++r)
#pragma unroll
      for (int c = r; c < 6; ++c)
        add_blk(anchor, anchor, 6 * r + c, Maa[6 * r + c] - (WAD[3 * r] * WA[3 * c] + WAD[3 * r + 1] * WA[3 * c + 1] + WAD[3 * r + 2] * WA[3 * c + 2]));
    double t0, t1, t2;
    cross3(lin.xa, red[24], red[25], red[26], t0, t1, t2);
    const double ba[6] = {red[24], red[25], red[26], t0, t1, t2};
#pragma unroll
    for (int r = 0; r < 6; ++r) {
      atomic_add_f64(B.bp + 6 * anchor + r, ba[r]);
      atomic_add_f64(B.bs + 6 * anchor + r, WA[3 * r] * Db[0] + WA[3 * r + 1] * Db[1] + WA[3 * r + 2] * Db[2]);
    }
  }
  double *my_wo = s_wo + tid * 18;
#pragma unroll
  for (int i = 0; i < 18; ++i) my_wo[i] = Wo[i];
  s_pose[tid] = ed.pose; s_role[tid] = obs_role ? 1 : 0;
  double WoD[18];
#pragma unroll
  for (int i = 0; i < 6; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) WoD[3 * i + j] = Wo[3 * i] * Di[j] + Wo[3 * i + 1] * Di[3 + j] + Wo[3 * i + 2] * Di[6 + j];
  if (obs_role && part == 0) {
    const int pi = ed.pose;
    {
      double Moo[36];
      sym_block(lin.A, lin.y, Moo);
#pragma unroll
      for (int r = 0; r < 6; ++r)
#pragma unroll
        for (int c = r; c < 6; ++c)
          add_blk(pi, pi, 6 * r + c, Moo[6 * r + c] - (WoD[3 * r] * Wo[3 * c] + WoD[3 * r + 1] * Wo[3 * c + 1] + WoD[3 * r + 2] * Wo[3 * c + 2]));
    }
    {
      double AR[9], Noa[36];
#pragma unroll
      for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) AR[3 * i + j] = lin.A[3 * i] * lin.R[j] + lin.A[3 * i + 1] * lin.R[3 + j] + lin.A[3 * i + 2] * lin.R[6 + j];
      cross_block(AR, lin.y, lin.xa, Noa);
      const bool up = pi < anchor;
#pragma unroll
      for (int r = 0; r < 6; ++r)
#pragma unroll
        for (int c = 0; c < 6; ++c) {
          const double mm = -Noa[6 * r + c] - (WoD[3 * r] * WA[3 * c] + WoD[3 * r + 1] * WA[3 * c + 1] + WoD[3 * r + 2] * WA[3 * c + 2]);
          if (up) add_blk(pi, anchor, 6 * r + c, mm); else add_blk(anchor, pi, 6 * c + r, mm);
        }
    }
    double u0, u1, u2;
    cross3(lin.y, lin.g[0], lin.g[1], lin.g[2], u0, u1, u2);
    const double bo[6] = {-lin.g[0], -lin.g[1], -lin.g[2], -u0, -u1, -u2};
#pragma unroll
    for (int r = 0; r < 6; ++r) {
      atomic_add_f64(B.bp + 6 * pi + r, bo[r]);
      atomic_add_f64(B.bs + 6 * pi + r, Wo[3 * r] * Db[0] + Wo[3 * r + 1] * Db[1] + Wo[3 * r + 2] * Db[2]);
    }
  }
  __syncthreads();
  // observer-observer pairs, circulant schedule over the m edges of the landmark (partners may sit in other waves: pose / role /
  // W_obs come from LDS)
  for (int r = 1 + part; r <= (m >> 1); r += split) {
    int b = tid + r;
    if (b >= m) b -= m;
    const bool on = obs_role && 2 * r <= m && !(2 * r == m && tid >= r) && s_role[b] != 0;
    if (on) {
      const int pj = s_pose[b];
      const double *wj = s_wo + b * 18;
      double Wj[18];
#pragma unroll
      for (int i = 0; i < 18; ++i) Wj[i] = wj[i];
      const bool up = ed.pose < pj;
#pragma unroll
      for (int rr = 0; rr < 6; ++rr)
#pragma unroll
        for (int c = 0; c < 6; ++c) {
          const double v = -(WoD[3 * rr] * Wj[3 * c] + WoD[3 * rr + 1] * Wj[3 * c + 1] + WoD[3 * rr + 2] * Wj[3 * c + 2]);
          if (up) add_blk(ed.pose, pj, 6 * rr + c, v); else add_blk(pj, ed.pose, 6 * c + rr, v);
        }
    }
  }
}

