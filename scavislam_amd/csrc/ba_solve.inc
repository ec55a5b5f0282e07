// ba_solve.inc -- part of ba.hip (one translation unit): the reduced-system solves -- global-memory blocked Cholesky, multi-workgroup Cholesky for wide
// envelopes, LDS-window pipeline, register-resident fused elimination (one or two fronts).
// ---- reduced-system solve: blocked right-looking Cholesky on the packed upper 6x6 blocks -------
// One workgroup (1024 lanes); the factor overwrites H in L2-resident global memory, the current
// panel row and the rhs live in LDS.  A = U^T U, U upper.  Fused forward substitution; column
// oriented back substitution.  Then T_trial = exp(x_p) T, scale_p, bookkeeping scalars.
constexpr int SOLVE_THREADS = 256;
constexpr int GRID_NBAR = 16;        // arrival counters of the multi-workgroup solve (bar[32 i], failure flag at bar[32 GRID_NBAR])
constexpr int SOLVE_MAX_P = 256;

__device__ void d_se3_exp_mul(const double *x, const double *T, double *Tn) {   // exp(x) * T  (G2oVertexSE3::oplusImpl)
  const double *w = x + 3;
  const double th2 = w[0] * w[0] + w[1] * w[1] + w[2] * w[2];
  double W[9] = {0, -w[2], w[1], w[2], 0, -w[0], -w[1], w[0], 0}, W2[9], R[9], V[9];
  for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) W2[3 * i + j] = W[3 * i] * W[j] + W[3 * i + 1] * W[3 + j] + W[3 * i + 2] * W[6 + j];
  // a = sin(th) / th, b = (1 - cos th) / th^2, d = (th - sin th) / th^3.  An LM step rotates by far less than half a radian: there the three are even power series in
  // th^2 (remainder < 1e-22) -- no square root, no division, no sin / cos call at the tail of the solve kernel, where ONE lane per pose runs this (round 6; the same
  // series as the trackers' mo2_exp_mul); beyond it, the closed forms
  double a, b, d;
  if (th2 < 0.25) {
#define SVS_IF(k) (1.0 / k)
    const double t = th2;
    a = 1.0 - t * (SVS_IF(6.) - t * (SVS_IF(120.) - t * (SVS_IF(5040.) - t * (SVS_IF(362880.) - t * (SVS_IF(39916800.) - t * (SVS_IF(6227020800.) - t * (SVS_IF(1307674368000.) -
        t * (SVS_IF(355687428096000.) - t * SVS_IF(121645100408832000.)))))))));
    b = SVS_IF(2.) - t * (SVS_IF(24.) - t * (SVS_IF(720.) - t * (SVS_IF(40320.) - t * (SVS_IF(3628800.) - t * (SVS_IF(479001600.) - t * (SVS_IF(87178291200.) -
        t * (SVS_IF(20922789888000.) - t * (SVS_IF(6402373705728000.) - t * SVS_IF(2432902008176640000.)))))))));
    d = SVS_IF(6.) - t * (SVS_IF(120.) - t * (SVS_IF(5040.) - t * (SVS_IF(362880.) - t * (SVS_IF(39916800.) - t * (SVS_IF(6227020800.) - t * (SVS_IF(1307674368000.) -
        t * (SVS_IF(355687428096000.) - t * (SVS_IF(121645100408832000.) - t * SVS_IF(51090942171709440000.)))))))));
#undef SVS_IF
  } else {
    const double th = sqrt(th2);
    a = sin(th) / th; b = (1.0 - cos(th)) / th2; d = (th - sin(th)) / (th2 * th);
  }
  for (int i = 0; i < 9; ++i) { R[i] = a * W[i] + b * W2[i]; V[i] = b * W[i] + d * W2[i]; }
  R[0] += 1; R[4] += 1; R[8] += 1;
  V[0] += 1; V[4] += 1; V[8] += 1;
  double t[3];
  for (int i = 0; i < 3; ++i) t[i] = V[3 * i] * x[0] + V[3 * i + 1] * x[1] + V[3 * i + 2] * x[2];
  for (int i = 0; i < 3; ++i) {
    for (int j = 0; j < 4; ++j) Tn[4 * i + j] = R[3 * i] * T[j] + R[3 * i + 1] * T[4 + j] + R[3 * i + 2] * T[8 + j];
    Tn[4 * i + 3] += t[i];
  }
}

// rowmax[k] = last block column of row k inside the (filled) block envelope of the reduced system:
// structurally H_kj == 0 and stays 0 during elimination for j > rowmax[k].  For a dense window
// rowmax[k] = P-1 and this is a plain blocked Cholesky; for the banded co-visibility structure of a
// sliding window it skips almost all of the P^3/6 block updates (what CSparse's sparse Cholesky
// does for the reference).  colmin[k] = first row whose envelope reaches column k.
__global__ __launch_bounds__(SOLVE_THREADS) void ba_solve_kernel(BaDev B, double *__restrict__ x_out, double *__restrict__ linv_ws,
                                                                 const int *__restrict__ rowmax, const int *__restrict__ colmin) {
  extern __shared__ double smem[];
  if (B.ctl) { if (B.ctl[1] != 0.0) return; B.lambda = B.ctl[0]; }      // speculative trial: lambda decided on the device, skipped after a rejection
  const int P = B.P, n = 6 * P, tid = threadIdx.x;
  double *s_b = smem;                 // [n] rhs -> y -> x
  double *s_panel = smem + n;         // [P*36] current panel row U_kj, j>k
  double *s_linv = s_panel + (size_t)P * 36;   // [36] (U_kk^T)^-1, lower
  __shared__ int s_fail;
  if (tid == 0) s_fail = 0;
  for (int i = tid; i < n; i += SOLVE_THREADS) s_b[i] = B.bp[i] - B.bs[i];
  __syncthreads();
  for (int k = 0; k < P; ++k) {
    const long kk = blk_index(k, k, P);
    if (tid == 0) {
      // 6x6 Cholesky of A_kk (+lambda), upper stored; fully unrolled so A/U/Li stay in registers
      double A[36], U[36], Li[36];
      const double *Akk = B.H + kk * 36;
#pragma unroll
      for (int r = 0; r < 6; ++r)
#pragma unroll
        for (int c = r; c < 6; ++c) { double v = Akk[6 * r + c]; if (r == c) v += B.lambda; A[6 * r + c] = v; }
      int fail = 0;
#pragma unroll
      for (int i = 0; i < 36; ++i) { U[i] = 0; Li[i] = 0; }
      double rd[6];
#pragma unroll
      for (int j = 0; j < 6; ++j) {
        double d = A[6 * j + j];
#pragma unroll
        for (int q = 0; q < j; ++q) d -= U[6 * q + j] * U[6 * q + j];
        if (!(d > 0) || !isfinite(d)) { fail = 1; d = 1; }
        d = sqrt(d);
        U[6 * j + j] = d;
        rd[j] = 1.0 / d;
#pragma unroll
        for (int c = j + 1; c < 6; ++c) {
          double s = A[6 * j + c];
#pragma unroll
          for (int q = 0; q < j; ++q) s -= U[6 * q + j] * U[6 * q + c];
          U[6 * j + c] = s * rd[j];
        }
      }
      // Li = (U^T)^-1 (lower triangular): forward substitution on identity
#pragma unroll
      for (int c = 0; c < 6; ++c)
#pragma unroll
        for (int r = c; r < 6; ++r) {
          double s = (r == c) ? 1.0 : 0.0;
#pragma unroll
          for (int q = c; q < r; ++q) s -= U[6 * q + r] * Li[6 * q + c];
          Li[6 * r + c] = s * rd[r];
        }
#pragma unroll
      for (int i = 0; i < 36; ++i) { s_linv[i] = Li[i]; linv_ws[(size_t)k * 36 + i] = Li[i]; }
      if (fail) s_fail = 1;
    }
    __syncthreads();
    if (s_fail) break;
    // y_k = Li * b_k (forward substitution, fused)
    double yk[6];
#pragma unroll
    for (int r = 0; r < 6; ++r) { double s = 0; for (int q = 0; q <= r; ++q) s += s_linv[6 * r + q] * s_b[6 * k + q]; yk[r] = s; }
    // panel: U_kj = Li * A_kj, k < j <= rowmax[k]; one thread per (block, column)
    const int nj = rowmax[k] - k;
    for (int e = tid; e < nj * 6; e += SOLVE_THREADS) {
      const int jj = e / 6, c = e - jj * 6;
      const double *Akj = B.H + (kk + 1 + jj) * 36;
      double a[6];
#pragma unroll
      for (int q = 0; q < 6; ++q) a[q] = Akj[6 * q + c];
#pragma unroll
      for (int r = 0; r < 6; ++r) {
        double s = 0;
#pragma unroll
        for (int q = 0; q <= r; ++q) s += s_linv[6 * r + q] * a[q];
        s_panel[(size_t)jj * 36 + 6 * r + c] = s;
      }
    }
    __syncthreads();
    if (tid < 6) s_b[6 * k + tid] = yk[tid];
    for (int e = tid; e < nj * 36; e += SOLVE_THREADS) B.H[(kk + 1) * 36 + e] = s_panel[e];   // keep U for back substitution
    // rhs update: b_j -= U_kj^T y_k
    for (int e = tid; e < nj * 6; e += SOLVE_THREADS) {
      const int jj = e / 6, c = e - jj * 6;
      double s = 0;
#pragma unroll
      for (int q = 0; q < 6; ++q) s += s_panel[(size_t)jj * 36 + 6 * q + c] * yk[q];
      s_b[6 * (k + 1 + jj) + c] -= s;
    }
    // trailing update inside the envelope: A_ij -= U_ki^T U_kj, k < i <= j <= rowmax[k];
    // one thread per (block, row): 6 outputs from 6 + 36 LDS operands
    const long nblk = (long)nj * (nj + 1) / 2;
    for (long e = tid; e < nblk * 6; e += SOLVE_THREADS) {
      const long bidx = e / 6;
      const int r = (int)(e - bidx * 6);
      int ii = (int)((2.0 * nj + 1.0 - sqrt((2.0 * nj + 1.0) * (2.0 * nj + 1.0) - 8.0 * (double)bidx)) * 0.5);
      while ((long)ii * nj - (long)ii * (ii - 1) / 2 > bidx) --ii;
      while ((long)(ii + 1) * nj - (long)(ii + 1) * ii / 2 <= bidx) ++ii;
      const int jj = ii + (int)(bidx - ((long)ii * nj - (long)ii * (ii - 1) / 2));
      double xi[6];
#pragma unroll
      for (int q = 0; q < 6; ++q) xi[q] = s_panel[(size_t)ii * 36 + 6 * q + r];
      double *Aij = B.H + blk_index(k + 1 + ii, k + 1 + jj, P) * 36 + 6 * r;
#pragma unroll
      for (int c = 0; c < 6; ++c) {
        double s = 0;
#pragma unroll
        for (int q = 0; q < 6; ++q) s += xi[q] * s_panel[(size_t)jj * 36 + 6 * q + c];
        Aij[c] -= s;
      }
    }
    __syncthreads();
  }
  const int fail = s_fail;
  __syncthreads();
  if (!fail) {
    // back substitution (column oriented): x_k = Li_k^T y_k ; y_i -= U_ik x_k for colmin[k] <= i < k
    for (int k = P - 1; k >= 0; --k) {
      if (tid < 6) {
        double s = 0;
        for (int q = tid; q < 6; ++q) s += linv_ws[(size_t)k * 36 + 6 * q + tid] * s_b[6 * k + q];
        s_linv[tid] = s;
      }
      __syncthreads();
      if (tid < 6) s_b[6 * k + tid] = s_linv[tid];
      const int i0 = colmin[k];
      for (int e = tid; e < (k - i0) * 6; e += SOLVE_THREADS) {
        const int i = i0 + e / 6, r = e % 6;
        if (rowmax[i] >= k) {
          const double *Uik = B.H + blk_index(i, k, P) * 36;
          double s = 0;
#pragma unroll
          for (int q = 0; q < 6; ++q) s += Uik[6 * r + q] * s_linv[q];
          s_b[6 * i + r] -= s;
        }
      }
      __syncthreads();
    }
  } else {
    for (int i = tid; i < n; i += SOLVE_THREADS) s_b[i] = 0;
    __syncthreads();
  }
  // outputs: x, scale_p = sum x (lambda x + b_p), trial poses
  double sc = 0;
  for (int i = tid; i < n; i += SOLVE_THREADS) { const double xv = s_b[i]; x_out[i] = xv; sc += xv * (B.lambda * xv + B.bp[i]); }
  sc = wave_sum(sc);
  if ((tid & 63) == 0 && sc != 0.0) atomic_add_f64(&B.scal[2], sc);
  for (int p = tid; p < P; p += SOLVE_THREADS) {
    double Tn[12];
    d_se3_exp_mul(s_b + 6 * p, B.poses + 12 * (size_t)p, Tn);
    for (int i = 0; i < 12; ++i) B.poses_trial[12 * (size_t)p + i] = Tn[i];
  }
  if (tid == 0) { B.scal[3] = (double)fail; B.scal[4] = chi2_cur_sum(B); }
}

// The FULL structural pattern of the reduced system (every pair of poses that share a landmark, anchors included): what an ordering needs.  (h_pattern, built
// while marshalling, only marks each pose's farthest partners -- enough for the envelope of the caller's order, not for any other.)  One wave per chunk of whole
// landmarks (<= 64 edges): a lane holds one edge and walks the others of its landmark; wide landmarks (65 .. 256 edges) one workgroup each.
__global__ __launch_bounds__(64) void ba_full_pattern_kernel(BaDev B, double *__restrict__ pat) {
  const int c = blockIdx.x, lane = threadIdx.x, P = B.P;
  const int start = B.chunk_start[c], len = B.chunk_len[c];
  const bool live = lane < len;
  const svs_ba_edge e = B.edges[start + (live ? lane : 0)];
  const int lm = live ? e.point : -1, pose = e.pose, anc = e.anchor;
  if (live) { pat[(size_t)pose * P + anc] = 1.0; pat[(size_t)anc * P + pose] = 1.0; }
  for (int o = 0; o < len; ++o) {
    const int lm_o = __shfl(lm, o, 64), pose_o = __shfl(pose, o, 64);
    if (live && lm_o == lm && pose_o != pose) pat[(size_t)pose * P + pose_o] = 1.0;
  }
}
__global__ __launch_bounds__(256) void ba_full_pattern_wide_kernel(BaDev B, double *__restrict__ pat) {
  __shared__ int s_pose[256];
  const int w = blockIdx.x, tid = threadIdx.x, P = B.P;
  const int start = B.wide_start[w], len = B.wide_len[w];
  if (tid < len) s_pose[tid] = B.edges[start + tid].pose;
  __syncthreads();
  if (tid < len) {
    const int pose = s_pose[tid], anc = B.edges[start + tid].anchor;
    pat[(size_t)pose * P + anc] = 1.0; pat[(size_t)anc * P + pose] = 1.0;
    for (int o = 0; o < len; ++o) if (s_pose[o] != pose) pat[(size_t)pose * P + s_pose[o]] = 1.0;
  }
}
// ---- the solve's own pose order (ensure_profile: reverse Cuthill-McKee when it narrows the filled envelope) -------------------------------------------------
// H'(i, j) = H(perm[i], perm[j]) for i <= j on the packed upper storage: a block whose natural position lies below the diagonal is the transpose of the stored
// one.  One workgroup per block (grid-stride), 36 lanes busy; b_p, b_s and the current poses are gathered alongside.  Skipped trials (ctl abort) copy nothing.
__global__ __launch_bounds__(256) void ba_permute_system_kernel(BaDev B, const int *__restrict__ perm, double *__restrict__ Hp, double *__restrict__ bpp,
                                                                double *__restrict__ bsp, double *__restrict__ poses_p) {
  if (B.ctl && B.ctl[1] != 0.0) return;
  const int P = B.P, tid = threadIdx.x;
  const long nblk = (long)P * (P + 1) / 2;
  // 7 blocks per 256-lane workgroup pass: lane = (block slot, element)
  const int slot = tid / 36, e = tid - slot * 36;
  if (slot < 7) {
    for (long blk = (long)blockIdx.x * 7 + slot; blk < nblk; blk += (long)gridDim.x * 7) {
      // invert blk -> (i, j), i <= j, row-major packed upper: row i starts at i P - i (i - 1) / 2
      int i = (int)((2.0 * P + 1.0 - sqrt((2.0 * P + 1.0) * (2.0 * P + 1.0) - 8.0 * (double)blk)) * 0.5);
      while ((long)i * P - (long)i * (i - 1) / 2 > blk) --i;
      while ((long)(i + 1) * P - (long)(i + 1) * i / 2 <= blk) ++i;
      const int j = i + (int)(blk - ((long)i * P - (long)i * (i - 1) / 2));
      const int a = perm[i], b = perm[j];
      const int r = e / 6, c = e - 6 * r;
      Hp[blk * 36 + e] = a <= b ? B.H[blk_index(a, b, P) * 36 + e] : B.H[blk_index(b, a, P) * 36 + 6 * c + r];
    }
  }
  if (blockIdx.x == 0) {
    for (int q = tid; q < 6 * P; q += 256) { const int k = q / 6, c = q - 6 * k; bpp[q] = B.bp[6 * perm[k] + c]; bsp[q] = B.bs[6 * perm[k] + c]; }
    for (int q = tid; q < 12 * P; q += 256) { const int k = q / 12, c = q - 12 * k; poses_p[q] = B.poses[12 * (size_t)perm[k] + c]; }
  }
}
// x and the trial poses back into the caller's pose order
__global__ __launch_bounds__(64) void ba_unpermute_kernel(BaDev B, const int *__restrict__ perm, const double *__restrict__ x_p, const double *__restrict__ trial_p,
                                                          double *__restrict__ x_out) {
  if (B.ctl && B.ctl[1] != 0.0) return;
  const int k = blockIdx.x * 64 + threadIdx.x;
  if (k >= B.P) return;
  const int g = perm[k];
  for (int c = 0; c < 6; ++c) x_out[6 * g + c] = x_p[6 * k + c];
  for (int c = 0; c < 12; ++c) B.poses_trial[12 * (size_t)g + c] = trial_p[12 * k + c];
}

// ---- multi-workgroup variant for wide envelopes -------------------------------------------------------------------------
// The reference's real window is 30 inner + 200 outer poses (data/newcollege.cfg:21-22), and a loop closure or a landmark seen from
// 180 keyframes couples poses far apart: the filled envelope then spans most of the 230 block rows and the one-workgroup kernel
// above spends 0.26 ms per elimination step on its trailing update (60 ms per solve).  Here the trailing update of every step is
// spread over G workgroups (one per CU):
//   * every workgroup factorises the 6x6 pivot block and forms the WHOLE panel row U_k* = L_kk^-1 A_k* itself (<= 255 blocks,
//     50 kFLOP: cheaper than handing it around), into LDS;
//   * the trailing tiles A_ij -= U_ki^T U_kj of the step are dealt to all lanes of all workgroups (one lane per tile row);
//   * ONE device-scope arrival counter per step (monotonic, relaxed polls) makes row k+1 final before anybody reads it.  All
//     traffic on H goes through write-through stores / L1-bypassing loads (agent scope), so no cache has to be flushed or
//     invalidated and workgroups on different XCDs see each other's tiles (MI355X_MICROARCH.md, inter-workgroup visibility);
//   * workgroup 0 keeps the right-hand side (forward substitution rides along), stores U for the back substitution and finishes
//     alone: row-oriented back substitution, trial poses, scale.
// The G workgroups must be resident together (G <= #CUs, one 256-lane workgroup each); a bounded wait turns a missing sibling into
// the solve's failure path (the LM trial is then rejected like a non-positive pivot).
__device__ __forceinline__ void g_st(double *p, double v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ double g_ld(const double *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__global__ __launch_bounds__(SOLVE_THREADS) void ba_solve_grid_kernel(BaDev B, double *__restrict__ x_out, double *__restrict__ linv_ws,
                                                                      const int *__restrict__ rowmax, unsigned *__restrict__ bar, unsigned epoch0) {
  extern __shared__ double smem[];
  if (B.ctl) { if (B.ctl[1] != 0.0) return; B.lambda = B.ctl[0]; }
  const int P = B.P, n = 6 * P, tid = threadIdx.x, wg = blockIdx.x, G = gridDim.x;
  double *s_panel = smem;                          // [P*36] panel row U_kj, j > k
  double *s_linv = s_panel + (size_t)P * 36;       // [36] (U_kk^T)^-1, lower
  double *s_b = s_linv + 36;                       // [n] rhs -> y -> x (workgroup 0 only)
  __shared__ int s_fail;
  if (tid == 0) s_fail = 0;
  if (wg == 0) for (int i = tid; i < n; i += SOLVE_THREADS) s_b[i] = B.bp[i] - B.bs[i];
  __syncthreads();
  // Everything a step reads from H -- the pivot block, the panel row, this lane's trailing tiles -- was completed by the previous step's
  // arrival, and every such load bypasses the caches (other workgroups wrote the data) at the price of a memory round trip of ~2 us.
  // So a step issues ALL of its loads first and works from registers: one round trip per step instead of three dependent ones
  // (pivot block -> panel row -> trailing tiles; 13.5 -> 9 us per block row at 224 block columns).
  constexpr int NIT = (SOLVE_MAX_P * 6 + SOLVE_THREADS - 1) / SOLVE_THREADS;       // panel columns per lane
  long long acc_t[6] = {0, 0, 0, 0, 0, 0};      // workgroup 0, lane 0: where the time of a step goes (SVS_BA_DEBUG=1)
  for (int k = 0; k < P; ++k) {
    long long ts = wall_clock64();
#define GRID_LAP(i) do { const long long tn = wall_clock64(); acc_t[i] += tn - ts; ts = tn; } while (0)
    const long kk = blk_index(k, k, P);
    const int nj = rowmax[k] - k;
    const long nblk = (long)nj * (nj + 1) / 2, stride = (long)G * SOLVE_THREADS;
    // ---- loads: pivot block (lane 0), panel columns, the first three trailing tile rows of this lane
    double Acol[6] = {0, 0, 0, 0, 0, 0};         // lane c < 6: column c of the pivot block's upper triangle
    if (tid < 6) {
      const double *Akk = B.H + kk * 36;
#pragma unroll
      for (int r = 0; r < 6; ++r)
        if (r <= tid) { double v = g_ld(Akk + 6 * r + tid); if (r == tid) v += B.lambda; Acol[r] = v; }
    }
    double a[NIT][6];
#pragma unroll
    for (int it = 0; it < NIT; ++it) {
      const int e = tid + it * SOLVE_THREADS;
      if (e < nj * 6) {
        const int jj = e / 6, c = e - jj * 6;
        const double *Akj = B.H + (kk + 1 + jj) * 36;
#pragma unroll
        for (int q = 0; q < 6; ++q) a[it][q] = g_ld(Akj + 6 * q + c);
      }
    }
    double *Aij[3];
    int ti[3], tj[3], tr[3];
    double acc[3][6];
    auto tile_of = [&](long e, int u) {      // tile row e = (block (ii, jj) of the trailing triangle, row r): index + loads
      Aij[u] = nullptr;
      if (e < nblk * 6) {
        const long bidx = e / 6;
        tr[u] = (int)(e - bidx * 6);
        int i_ = (int)((2.0 * nj + 1.0 - sqrt((2.0 * nj + 1.0) * (2.0 * nj + 1.0) - 8.0 * (double)bidx)) * 0.5);
        while ((long)i_ * nj - (long)i_ * (i_ - 1) / 2 > bidx) --i_;
        while ((long)(i_ + 1) * nj - (long)(i_ + 1) * i_ / 2 <= bidx) ++i_;
        ti[u] = i_;
        tj[u] = i_ + (int)(bidx - ((long)i_ * nj - (long)i_ * (i_ - 1) / 2));
        Aij[u] = B.H + blk_index(k + 1 + ti[u], k + 1 + tj[u], P) * 36 + 6 * tr[u];
#pragma unroll
        for (int c = 0; c < 6; ++c) acc[u][c] = g_ld(Aij[u] + c);
      }
    };
    const long e_first = (long)wg * SOLVE_THREADS + tid;
#pragma unroll
    for (int u = 0; u < 3; ++u) tile_of(e_first + u * stride, u);
    // ---- pivot block: U_kk and (U_kk^T)^-1 in every workgroup (cheaper than handing them around), lane c of wave 0 = column c,
    //      the elements of other columns by readlane: six short steps instead of ~600 dependent instructions on one lane
    if (tid < 64) {
      const int c = tid;
      double Ucol[6] = {0, 0, 0, 0, 0, 0}, rdv[6];      // U[q][c], q <= c
      int fail = 0;
#pragma unroll
      for (int j = 0; j < 6; ++j) {
        double sv = Acol[j];                              // A[j][c], meaningful for c >= j
#pragma unroll
        for (int q = 0; q < j; ++q) sv -= lane_bcast(Ucol[q], j) * Ucol[q];      // U[q][j] U[q][c]
        double d = lane_bcast(sv, j);
        if (!(d > 0) || !isfinite(d)) { fail = 1; d = 1; }
        d = sqrt(d);
        rdv[j] = 1.0 / d;
        Ucol[j] = c == j ? d : (c > j ? sv * rdv[j] : 0.0);
      }
      double Lic[6];                                      // (U^T)^-1 [r][c], r >= c
#pragma unroll
      for (int r = 0; r < 6; ++r) {
        double sv = (r == c) ? 1.0 : 0.0;
#pragma unroll
        for (int q = 0; q < r; ++q) sv -= lane_bcast(Ucol[q], r) * Lic[q];      // U[q][r] Li[q][c] (Li[q][c] = 0 for q < c)
        Lic[r] = r >= c ? sv * rdv[r] : 0.0;
      }
      if (c < 6) {
#pragma unroll
        for (int r = 0; r < 6; ++r) s_linv[6 * r + c] = Lic[r];
        if (wg == 0) {
#pragma unroll
          for (int r = 0; r < 6; ++r) linv_ws[(size_t)k * 36 + 6 * r + c] = Lic[r];
        }
      }
      if (fail && c == 0) s_fail = 1;
    }
    __syncthreads();
    GRID_LAP(0);
    if (s_fail) break;                             // every workgroup takes the same decision from the same pivot block
    // ---- panel: U_kj = Li * A_kj, one lane per (block, column)
#pragma unroll
    for (int it = 0; it < NIT; ++it) {
      const int e = tid + it * SOLVE_THREADS;
      if (e < nj * 6) {
        const int jj = e / 6, c = e - jj * 6;
#pragma unroll
        for (int r = 0; r < 6; ++r) {
          double sv = 0;
#pragma unroll
          for (int q = 0; q <= r; ++q) sv += s_linv[6 * r + q] * a[it][q];
          s_panel[(size_t)jj * 36 + 6 * r + c] = sv;
        }
      }
    }
    __syncthreads();
    if (wg == 0) {
      double yk[6];
#pragma unroll
      for (int r = 0; r < 6; ++r) { double sv = 0; for (int q = 0; q <= r; ++q) sv += s_linv[6 * r + q] * s_b[6 * k + q]; yk[r] = sv; }
      __syncthreads();
      if (tid < 6) s_b[6 * k + tid] = yk[tid];
      for (int e = tid; e < nj * 6; e += SOLVE_THREADS) {
        const int jj = e / 6, c = e - jj * 6;
        double sv = 0;
#pragma unroll
        for (int q = 0; q < 6; ++q) sv += s_panel[(size_t)jj * 36 + 6 * q + c] * yk[q];
        s_b[6 * (k + 1 + jj) + c] -= sv;
      }
    }
    GRID_LAP(1);
    // ---- trailing update inside the envelope, dealt to all lanes of all workgroups: one lane per (tile, row), three per trip
    for (long e0 = e_first;; e0 += 3 * stride) {
#pragma unroll
      for (int u = 0; u < 3; ++u) {
        if (Aij[u]) {
          double xi[6];
#pragma unroll
          for (int q = 0; q < 6; ++q) xi[q] = s_panel[(size_t)ti[u] * 36 + 6 * q + tr[u]];
#pragma unroll
          for (int c = 0; c < 6; ++c) {
            double sv = 0;
#pragma unroll
            for (int q = 0; q < 6; ++q) sv += xi[q] * s_panel[(size_t)tj[u] * 36 + 6 * q + c];
            g_st(Aij[u] + c, acc[u][c] - sv);
          }
        }
      }
      if (e0 + 3 * stride >= nblk * 6) break;
#pragma unroll
      for (int u = 0; u < 3; ++u) tile_of(e0 + (3 + u) * stride, u);      // (only windows with few workgroups get here)
    }
    // arrival: this workgroup's tiles of step k are on their way; wait until everybody's are
    GRID_LAP(2);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    GRID_LAP(3);
    // GRID_NBAR counters, 128 bytes apart, workgroup w arrives on counter w % GRID_NBAR: 256 same-address device-scope atomics per step
    // serialise at the memory side (3 of the 16 us a step took); 16 per counter do not.  Wave 0 polls, one counter per lane.
    if (tid < 64 && k + 1 < P) {
      if (tid == 0) __hip_atomic_fetch_add(bar + 32 * (wg % GRID_NBAR), 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      const bool mine = tid < GRID_NBAR && tid < G;
      const unsigned n_here = mine ? (unsigned)((G - tid + GRID_NBAR - 1) / GRID_NBAR) : 0u;      // workgroups that arrive on this lane's counter
      const unsigned want = epoch0 + n_here * (unsigned)(k + 1);
      long spin = 0;
      bool late = false;
      for (;;) {
        const unsigned v = mine ? __hip_atomic_load(bar + 32 * tid, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : want;
        if (__all((int)(v - want) >= 0)) break;
        if (++spin >= (1l << 22)) { late = true; break; }
        __builtin_amdgcn_s_sleep(1);
      }
      if (tid == 0) {
        if (late) __hip_atomic_store(bar + 32 * GRID_NBAR, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (__hip_atomic_load(bar + 32 * GRID_NBAR, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0) s_fail = 2;
      }
    }
    __syncthreads();
    GRID_LAP(4);
    if (s_fail) break;
    // U_k* for the back substitution replaces A_k* only now: before the arrival above a slower workgroup could still be reading A_k*
    // for its own copy of the panel row
    if (wg == 0) {
      for (int e = tid; e < nj * 36; e += SOLVE_THREADS) g_st(B.H + (kk + 1) * 36 + e, s_panel[e]);
      __syncthreads();                              // s_panel is overwritten by the next step's panel
    }
    GRID_LAP(5);
  }
  if (wg != 0) return;
  const int fail = s_fail;
  __syncthreads();
  if (!fail) {
    // back substitution, column oriented (round 3; it was row oriented: a reduction over the row + three barriers per block row, 3 us each):
    // x_k = Li_k^T y_k, then y_i -= U_ik x_k for every row i < k whose envelope reaches column k.  A lane owns the same (row i, component r)
    // pairs in every step, so its part of column k-1 (and the pivot's inverse) is requested while step k is worked on: no memory round trip and
    // no reduction on the chain, two barriers per block row.
    constexpr int NBK = (SOLVE_MAX_P * 6 + SOLVE_THREADS - 1) / SOLVE_THREADS;
    __shared__ double s_xk[6];
    int my_i[NBK], my_r[NBK], my_rowmax[NBK];
#pragma unroll
    for (int it = 0; it < NBK; ++it) {
      const int e = tid + it * SOLVE_THREADS;
      my_i[it] = e / 6; my_r[it] = e - 6 * my_i[it];
      my_rowmax[it] = my_i[it] < P ? rowmax[my_i[it]] : -1;
    }
    auto load_col = [&](int k, double (&u)[NBK][6], double (&li)[6]) {      // plain loads: every U row was written by THIS workgroup (write-through)
      if (k < 0) return;
#pragma unroll
      for (int it = 0; it < NBK; ++it) {
        const bool on = my_i[it] < k && my_rowmax[it] >= k;
        const double *Uik = B.H + blk_index(on ? my_i[it] : 0, on ? k : 0, P) * 36 + 6 * my_r[it];
#pragma unroll
        for (int q = 0; q < 6; ++q) u[it][q] = on ? Uik[q] : 0.0;
      }
      if (tid < 6) {
#pragma unroll
        for (int q = 0; q < 6; ++q) li[q] = linv_ws[(size_t)k * 36 + 6 * q + tid];      // column tid of Li_k = row tid of Li_k^T (zero above the diagonal)
      }
    };
    double ua[NBK][6], ub[NBK][6], la[6] = {0, 0, 0, 0, 0, 0}, lb[6] = {0, 0, 0, 0, 0, 0};
    load_col(P - 1, ua, la);
    for (int k = P - 1; k >= 0; --k) {
      load_col(k - 1, ub, lb);                       // in flight during this step
      if (tid < 6) {
        double sv = 0;
#pragma unroll
        for (int q = 0; q < 6; ++q) sv += (q >= tid ? la[q] : 0.0) * s_b[6 * k + q];
        s_xk[tid] = sv;
      }
      __syncthreads();
      double xk[6];
#pragma unroll
      for (int q = 0; q < 6; ++q) xk[q] = s_xk[q];
      if (tid < 6) s_b[6 * k + tid] = xk[tid];
#pragma unroll
      for (int it = 0; it < NBK; ++it) {
        if (my_i[it] < k && my_rowmax[it] >= k) {
          double sv = 0;
#pragma unroll
          for (int q = 0; q < 6; ++q) sv += ua[it][q] * xk[q];
          s_b[6 * my_i[it] + my_r[it]] -= sv;
        }
      }
      __syncthreads();
#pragma unroll
      for (int it = 0; it < NBK; ++it)
#pragma unroll
        for (int q = 0; q < 6; ++q) ua[it][q] = ub[it][q];
#pragma unroll
      for (int q = 0; q < 6; ++q) la[q] = lb[q];
    }
  } else {
    for (int i = tid; i < n; i += SOLVE_THREADS) s_b[i] = 0;
    __syncthreads();
  }
  double sc = 0;
  for (int i = tid; i < n; i += SOLVE_THREADS) { const double xv = s_b[i]; x_out[i] = xv; sc += xv * (B.lambda * xv + B.bp[i]); }
  sc = wave_sum(sc);
  if ((tid & 63) == 0 && sc != 0.0) atomic_add_f64(&B.scal[2], sc);
  for (int p = tid; p < P; p += SOLVE_THREADS) {
    double Tn[12];
    d_se3_exp_mul(s_b + 6 * p, B.poses + 12 * (size_t)p, Tn);
    for (int i = 0; i < 12; ++i) B.poses_trial[12 * (size_t)p + i] = Tn[i];
  }
  if (tid == 0) {
    B.scal[3] = (double)fail; B.scal[4] = chi2_cur_sum(B);
    // loads + pivot | panel + rhs | trailing issue | store drain | arrival | write-back  (read as: init, forward, load+row update, eliminate, -, barrier wait)
    B.scal[5] = acc_t[0] * 0.01; B.scal[6] = acc_t[1] * 0.01; B.scal[8] = acc_t[2] * 0.01; B.scal[9] = acc_t[3] * 0.01; B.scal[10] = acc_t[5] * 0.01; B.scal[11] = acc_t[4] * 0.01; B.scal[7] = 0;
  }
}

// ---- LDS-window variant of the solve -------------------------------------------------------------
// When the filled block envelope is narrow (R = max_k(rowmax[k]-k)+1 rows fit in LDS) the active
// R x R block window of the elimination lives entirely in LDS as a ring of envelope rows, and the
// P-step elimination runs as a software pipeline with ONE workgroup barrier per step:
//   wave 0 (pivot wave)   stage k: applies panel k to block row k+1 and to b_{k+1}, then factors the
//                         pivot block k+1 and forms panel k+1 (Z, Y; fused forward substitution)
//   waves 1-4 (update)    stage k: applies panel k to block rows k+2.. and to the rest of b
//   wave 5 (loader)       stage k: drops envelope row k+R (loaded two stages earlier) into the ring
//                         slot row k vacated, issues the loads of row k+R+2
// Panels are double-buffered, so panel k+1 is written while panel k is still being applied.  The
// panel rows Y_kj also go to a global buffer (written once, read once by the back substitution).
// The back substitution is run by wave 0 alone -- no workgroup barriers on its P-step chain.
// Measured (tools/ubench.hip): an f64 FMA issues every ~5 cycles per wave, dependent or not; what is
// expensive on the critical path is LDS round trips and workgroup barriers, so those are minimised.

// Workgroup barrier that orders LDS traffic only.  __syncthreads() also drains vmcnt, which would put
// the latency of the loader's global loads (~1 us) back on the critical path of every step.
__device__ __forceinline__ void lds_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }
// orders LDS traffic between the lanes of one wave (LDS executes a wave's operations in order)
__device__ __forceinline__ void wave_lds_fence() { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); }
constexpr int PIPE_THREADS = 384;
constexpr int PIPE_LD = 16;     // loader registers per lane and buffer: R*36 <= 64*PIPE_LD  => R <= 28

// reciprocal by hardware estimate + 2 Newton steps.  The value of devutil.h's rcp_rn with the factors of the two correction products the other way round: the
// compiler keeps that order in the v_fmac_f64 operands of the solve kernels, which were measured with this one (profiles/shared_helpers.md)
__device__ __forceinline__ double rcp_nr(double d) {
  double x = __builtin_amdgcn_rcp(d);
  double e = __builtin_fma(-d, x, 1.0);
  x = __builtin_fma(x, e, x);
  e = __builtin_fma(-d, x, 1.0);
  return __builtin_fma(x, e, x);
}
// (Round 5 tried ONE Newton step on the pivot chain of the fused solve -- two FMAs of 8 issue cycles less per pivot, 70.5 -> 68.6 us -- on the assumption that
// v_rcp_f64 delivers single-precision accuracy.  It does not: the landmark update of the recorded-graph test moved from ~1e-10 to 1.07e-6 of its size, which puts the
// estimate near 2^-13.  Two steps stay.)

// H + lambda I = U^T D U (U unit upper, D diagonal), organised in 6x6 block rows inside the envelope.
//   row k:  U_kk (unit upper), Y_kj = D_k^-1 U_kk^-T A~_kj  (j > k);   Z_kj = D_k Y_kj
//   trailing: A~_ij -= Z_ki^T Y_kj;  forward: z_k = U_kk^-T b~_k, b~_j -= Y_kj^T z_k;  w = D^-1 z
//   backward: x_k = U_kk^-1 (w_k - sum_j Y_kj x_j)
__global__ __launch_bounds__(PIPE_THREADS) void ba_solve_lds_kernel(BaDev B, double *__restrict__ x_out, double *__restrict__ upanel,
                                                                    const int *__restrict__ rowmax_g, int R, double *__restrict__ ukk) {
  extern __shared__ double smem[];
  if (B.ctl) { if (B.ctl[1] != 0.0) return; B.lambda = B.ctl[0]; }      // speculative trial: lambda decided on the device, skipped after a rejection
  const int P = B.P, n = 6 * P, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  double *s_b = smem;                          // [n]
  double *s_win = s_b + n;                     // [R][R][36] ring of envelope rows
  double *s_pz = s_win + (size_t)R * R * 36;   // [2][R][36] Z_kj
  double *s_py = s_pz + 2 * (size_t)R * 36;    // [2][R][36] Y_kj
  // (round 5: U_kk and 1/D_k of the CURRENT row only -- the back substitution reads the U_kk of all rows from the global array `ukk`, which the pivot wave
  //  fills as it goes; [P][42] doubles in LDS were 77 KB at 230 poses and kept envelopes of 11..19 block rows out of this kernel)
  double *s_ud = s_py + 2 * (size_t)R * 36;    // [36] U_kk of the row being factored (unit upper; strict upper part used)
  double *s_rd = s_ud + 36;                    // [6]  1/D_k of that row
  double *s_y = s_rd + 8;                      // [2][8]  z_k
  double *s_part = s_y + 16;                   // [R][6]
  int *rowmax = reinterpret_cast<int *>(s_part + (size_t)R * 6);         // [P] envelope
  unsigned char *lut = reinterpret_cast<unsigned char *>(rowmax + P);     // [(R-1)(R-2)/2 + ..][2] (ii, jj) of trailing block t, 1 <= ii <= jj
  __shared__ int s_fail;
  const long long t_begin = wall_clock64();
  if (tid == 0) s_fail = 0;
  for (int i = tid; i < P; i += PIPE_THREADS) rowmax[i] = rowmax_g[i];
  for (int i = tid; i < n; i += PIPE_THREADS) s_b[i] = B.bp[i] - B.bs[i];
  for (int t = tid; t < R * (R - 1) / 2; t += PIPE_THREADS) {   // t = jj (jj - 1) / 2 + (ii - 1)
    int jj = 1;
    while ((jj + 1) * jj / 2 <= t) ++jj;
    lut[2 * t] = (unsigned char)(t - jj * (jj - 1) / 2 + 1);
    lut[2 * t + 1] = (unsigned char)jj;
  }
  for (int r = 0; r < R && r < P; ++r) {
    const long rb = blk_index(r, r, P);
    for (int e = tid; e < R * 36; e += PIPE_THREADS) {
      const int c = e / 36;
      s_win[((size_t)(r % R) * R) * 36 + e] = (r + c < P) ? B.H[(rb + c) * 36 + (e - c * 36)] : 0.0;
    }
  }
  // loader wave: envelope rows R and R+1 are in flight before the pipeline starts
  double ra[PIPE_LD], rb_[PIPE_LD];
  auto load_row = [&](double (&reg)[PIPE_LD], int rn) {
    if (rn < P) {
      const long rb = blk_index(rn, rn, P);
#pragma unroll
      for (int i = 0; i < PIPE_LD; ++i) {
        const int e = lane + 64 * i;
        const int c = e / 36;
        reg[i] = (e < R * 36 && rn + c < P) ? B.H[(rb + c) * 36 + (e - c * 36)] : 0.0;
      }
    }
  };
  auto store_row = [&](const double (&reg)[PIPE_LD], int k) {
    if (k + R < P) {
      double *row = s_win + ((size_t)(k % R) * R) * 36;
#pragma unroll
      for (int i = 0; i < PIPE_LD; ++i) { const int e = lane + 64 * i; if (e < R * 36) row[e] = reg[i]; }
    }
  };
  if (wave == 5) { load_row(ra, R); load_row(rb_, R + 1); }
  __syncthreads();
  // pivot block k -> U_kk, 1/D_k; panel k -> Z, Y (buffer k & 1), z_k, w_k.  Run by wave 0.
  long long t_mid = 0;
  auto factor_panel = [&](int k) {
    double *row = s_win + ((size_t)(k % R) * R) * 36;
    if (lane == 0) {
      // right-looking LDL^T of the 6x6 pivot block, in registers
      double A[36];
#pragma unroll
      for (int r = 0; r < 6; ++r)
#pragma unroll
        for (int c = r; c < 6; ++c) { double v = row[6 * r + c]; if (r == c) v += B.lambda; A[6 * r + c] = v; }
      int fail = 0;
#pragma unroll
      for (int j = 0; j < 6; ++j) {
        double d = A[6 * j + j];
        if (!(d > 0) || !isfinite(d)) { fail = 1; d = 1.0; }      // keep going (uniform control flow); x is zeroed at the end
        const double rj = rcp_nr(d);
        s_rd[j] = rj;
        double u[6];
#pragma unroll
        for (int c = j + 1; c < 6; ++c) { u[c] = A[6 * j + c] * rj; s_ud[6 * j + c] = u[c]; ukk[(size_t)k * 36 + 6 * j + c] = u[c]; }
#pragma unroll
        for (int r = j + 1; r < 6; ++r)
#pragma unroll
          for (int c = r; c < 6; ++c) A[6 * r + c] = __builtin_fma(-u[r], A[6 * j + c], A[6 * r + c]);
      }
      if (fail) s_fail = 1;
    }
    wave_lds_fence();
    t_mid = wall_clock64();
    const int nj = rowmax[k] - k;
    const double *U = s_ud, *rd = s_rd;
    double *pz = s_pz + (size_t)(k & 1) * R * 36, *py = s_py + (size_t)(k & 1) * R * 36, *zk = s_y + (k & 1) * 8;
    // panel columns (+ the rhs as one more column): unit-lower forward substitution
    for (int e = lane; e <= nj * 6; e += 64) {
      double a[6];
      const bool is_rhs = e == nj * 6;
      const int jj = e / 6, c = e - jj * 6;
#pragma unroll
      for (int q = 0; q < 6; ++q) a[q] = is_rhs ? s_b[6 * k + q] : row[(size_t)(1 + jj) * 36 + 6 * q + c];
#pragma unroll
      for (int q = 0; q < 5; ++q)
#pragma unroll
        for (int r = q + 1; r < 6; ++r) a[r] = __builtin_fma(-U[6 * q + r], a[q], a[r]);
      if (is_rhs) {
#pragma unroll
        for (int q = 0; q < 6; ++q) { zk[q] = a[q]; s_b[6 * k + q] = a[q] * rd[q]; }      // z_k, w_k
      } else {
#pragma unroll
        for (int q = 0; q < 6; ++q) {
          const double y = a[q] * rd[q];
          pz[(size_t)jj * 36 + 6 * q + c] = a[q];
          py[(size_t)jj * 36 + 6 * q + c] = y;
          upanel[((size_t)k * R + jj) * 36 + 6 * q + c] = y;
        }
      }
    }
    wave_lds_fence();
  };
  // A~_(k+1+ii),(k+1+jj) row r -= Z_k,ii(:,r)^T Y_k,jj
  auto update_block_row = [&](int k, const double *pz, const double *py, int ii, int jj, int r) {
    double zi[6];
#pragma unroll
    for (int q = 0; q < 6; ++q) zi[q] = pz[(size_t)ii * 36 + 6 * q + r];
    double *Aij = s_win + (((size_t)((k + 1 + ii) % R) * R) + (jj - ii)) * 36 + 6 * r;
#pragma unroll
    for (int c = 0; c < 6; ++c) {
      double s0 = 0, s1 = 0;
#pragma unroll
      for (int q = 0; q < 6; q += 2) {
        s0 = __builtin_fma(zi[q], py[(size_t)jj * 36 + 6 * q + c], s0);
        s1 = __builtin_fma(zi[q + 1], py[(size_t)jj * 36 + 6 * (q + 1) + c], s1);
      }
      Aij[c] -= s0 + s1;
    }
  };
  auto update_rhs = [&](int k, const double *py, const double *zk, int jj, int c) {     // b~_(k+1+jj)[c] -= Y_k,jj(:,c)^T z_k
    double s0 = 0, s1 = 0;
#pragma unroll
    for (int q = 0; q < 6; q += 2) {
      s0 = __builtin_fma(py[(size_t)jj * 36 + 6 * q + c], zk[q], s0);
      s1 = __builtin_fma(py[(size_t)jj * 36 + 6 * (q + 1) + c], zk[q + 1], s1);
    }
    s_b[6 * (k + 1 + jj) + c] -= s0 + s1;
  };
  if (wave == 0) factor_panel(0);
  lds_barrier();
  const long long t_loop = wall_clock64();
  long long acc_upd = 0, acc_piv = 0, acc_pan = 0, acc_bar = 0;      // pivot-wave stage breakdown (debug)
  for (int k = 0; k < P; ++k) {
    const int nj = rowmax[k] - k;
    const long long ts0 = wall_clock64();
    const double *pz = s_pz + (size_t)(k & 1) * R * 36, *py = s_py + (size_t)(k & 1) * R * 36, *zk = s_y + (k & 1) * 8;
    if (wave == 0) {
      for (int e = lane; e < nj * 6; e += 64) update_block_row(k, pz, py, 0, e / 6, e % 6);
      if (lane < 6 && nj > 0) update_rhs(k, py, zk, 0, lane);
      wave_lds_fence();
      const long long ts1 = wall_clock64();
      if (k + 1 < P) factor_panel(k + 1);
      const long long ts2 = wall_clock64();
      acc_upd += ts1 - ts0; acc_piv += t_mid - ts1; acc_pan += ts2 - t_mid;
    } else if (wave <= 4) {
      const int ul = tid - 64;
      for (int e = ul; e < (nj - 1) * 6; e += 256) update_rhs(k, py, zk, 1 + e / 6, e % 6);
      const int nb = nj * (nj - 1) / 2;
      for (int e = ul; e < nb * 6; e += 256) {
        const int t = e / 6;
        update_block_row(k, pz, py, lut[2 * t], lut[2 * t + 1], e - t * 6);
      }
    } else {
      if (k & 1) { store_row(rb_, k); load_row(rb_, k + R + 2); }
      else { store_row(ra, k); load_row(ra, k + R + 2); }
    }
    const long long ts3 = wall_clock64();
    lds_barrier();
    acc_bar += (long long)wall_clock64() - ts3;
  }
  const int fail = s_fail;
  const long long t_fwd = wall_clock64();
  if (wave == 0) {
    if (!fail) {
      double un[6], ucn[6] = {0, 0, 0, 0, 0, 0};      // the next row's panel values / row `lane` of its U_kk: requested one step ahead
      int njn = rowmax[P - 1] - (P - 1);
      if (lane < njn * 6) {
#pragma unroll
        for (int c = 0; c < 6; ++c) un[c] = upanel[((size_t)(P - 1) * R + lane / 6) * 36 + 6 * (lane % 6) + c];
      }
      if (lane < 6) {
#pragma unroll
        for (int r = 1; r < 6; ++r) ucn[r] = r > lane ? ukk[(size_t)(P - 1) * 36 + 6 * lane + r] : 0.0;      // (only the strict upper part was written)
      }
      for (int k = P - 1; k >= 0; --k) {
        const int nj = njn;
        double u[6], ucol[6];
#pragma unroll
        for (int c = 0; c < 6; ++c) { u[c] = un[c]; ucol[c] = ucn[c]; }
        if (k > 0) {
          njn = rowmax[k - 1] - (k - 1);
          if (lane < njn * 6) {
#pragma unroll
            for (int c = 0; c < 6; ++c) un[c] = upanel[((size_t)(k - 1) * R + lane / 6) * 36 + 6 * (lane % 6) + c];
          }
          if (lane < 6) {
#pragma unroll
            for (int r = 1; r < 6; ++r) ucn[r] = r > lane ? ukk[(size_t)(k - 1) * 36 + 6 * lane + r] : 0.0;
          }
        }
        for (int e = lane; e < nj * 6; e += 64) {
          const int jj = e / 6, r = e - jj * 6;
          if (e >= 64) {
#pragma unroll
            for (int c = 0; c < 6; ++c) u[c] = upanel[((size_t)k * R + jj) * 36 + 6 * r + c];
          }
          double s0 = 0, s1 = 0;
#pragma unroll
          for (int c = 0; c < 6; c += 2) {
            s0 = __builtin_fma(u[c], s_b[6 * (k + 1 + jj) + c], s0);
            s1 = __builtin_fma(u[c + 1], s_b[6 * (k + 1 + jj) + c + 1], s1);
          }
          s_part[jj * 6 + r] = s0 + s1;
        }
        wave_lds_fence();
        double x = 0;
        if (lane < 6) {
          double p0 = 0, p1 = 0;
          int jj = 0;
          for (; jj + 1 < nj; jj += 2) { p0 += s_part[jj * 6 + lane]; p1 += s_part[(jj + 1) * 6 + lane]; }
          if (jj < nj) p0 += s_part[jj * 6 + lane];
          x = s_b[6 * k + lane] - (p0 + p1);
        }
        // unit-upper back substitution across lanes 0..5 (ucol: row `lane` of U_kk, prefetched above)
#pragma unroll
        for (int r = 5; r >= 1; --r) {
          const double xr = lane_bcast(x, r);
          if (lane < r) x = __builtin_fma(-ucol[r], xr, x);
        }
        if (lane < 6) s_b[6 * k + lane] = x;
        wave_lds_fence();
      }
    } else {
      for (int i = lane; i < n; i += 64) s_b[i] = 0;
    }
  }
  __syncthreads();
  const long long t_back = wall_clock64();
  double sc = 0;
  for (int i = tid; i < n; i += PIPE_THREADS) { const double xv = s_b[i]; x_out[i] = xv; sc += xv * (B.lambda * xv + B.bp[i]); }
  sc = wave_sum(sc);
  if ((tid & 63) == 0 && sc != 0.0) atomic_add_f64(&B.scal[2], sc);
  for (int p = tid; p < P; p += PIPE_THREADS) {
    double Tn[12];
    d_se3_exp_mul(s_b + 6 * p, B.poses + 12 * (size_t)p, Tn);
    for (int i = 0; i < 12; ++i) B.poses_trial[12 * (size_t)p + i] = Tn[i];
  }
  if (tid == 0) {
    B.scal[3] = (double)fail; B.scal[4] = chi2_cur_sum(B);
    // phase timing (100 MHz wall clock ticks -> us), read by SVS_BA_DEBUG=1
    B.scal[5] = (double)(t_loop - t_begin) * 0.01; B.scal[6] = (double)(t_fwd - t_loop) * 0.01; B.scal[7] = (double)(t_back - t_fwd) * 0.01;
    B.scal[8] = acc_upd * 0.01; B.scal[9] = acc_piv * 0.01; B.scal[10] = acc_pan * 0.01; B.scal[11] = acc_bar * 0.01;
  }
}

// ---- register-resident variant for narrow envelopes (R <= 10 block rows) ------------------------------
// Same U^T D U elimination and the same pipeline as ba_solve_lds_kernel, but the pivot wave never
// round-trips through LDS inside a stage: lane (slot, c) of wave 0 owns column c of the block column
// j with j % 10 == slot for as long as j is inside the sliding window.  It keeps that column of the
// current panel (Y_k) in registers, applies panel k to its column of block row k+1, and the 6 pivots
// of block k+1 are eliminated on ALL columns of the row at once (panel columns and the rhs ride along
// as extra columns, multipliers broadcast with v_readlane) -- factorisation, panel and forward
// substitution are one pass.  Trailing blocks are updated by waves 1-3 (two block columns per lane,
// 128-bit LDS accesses), wave 4 streams envelope rows into the LDS ring.
// The back substitution is column-oriented: lane (slot, r) carries the running value of component r of
// one row, every solved x_k is broadcast from the pivot lanes and applied with 6 FMAs, panel rows are
// prefetched FUSE_PRE steps ahead into registers -- no LDS access and no barrier on its chain.
constexpr int FUSE_THREADS = 320;
constexpr int FUSE_SLOTS = 10;
constexpr int FUSE_PRE = 8;
// Two fronts ("burn at both ends"): with P1 > 0 the kernel runs as TWO workgroups.  Front 0 eliminates the block rows
// 0 .. P_top-1 in natural order; front 1 eliminates the last P1 rows (P_top = P - P1) in REVERSED block order -- the same
// code on the block-reversed matrix (blocks fetched transposed from the packed upper storage, envelope = the reversed
// profile).  The band structure decouples the two eliminations except for the R-1 rows just above front 1's set: front 1
// leaves their Schur-complement deltas (matrix corner + rhs) in `xfer`, raises flag 0, and front 0 adds them to its LDS
// window right before it consumes the first of those rows.  Back substitution mirrors it: front 0 publishes x of those
// R-1 rows as soon as they are solved (flag 1), front 1 treats them as known rows of its own (reversed) system.
// Flags hold the launch epoch (no reset needed); waits are bounded and fall into the solve's failure path.
struct FuseFronts { int P_top, P1; double *xfer; unsigned *flags; int lds_panel; };      // lds_panel: the panel rows of the back substitution stay in LDS (round 6)
__device__ __forceinline__ bool fuse_wait_flag(const unsigned *flag, unsigned epoch) {
  for (int spin = 0; spin < (1 << 22); ++spin) {
    if (__hip_atomic_load(flag, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT) == epoch) return true;
    __builtin_amdgcn_s_sleep(2);
  }
  return false;
}
// LDSP: the panel rows of the back substitution live in LDS (F.lds_panel, decided by the host); DBG: the per-stage clocks of SVS_BA_DEBUG.  Rounds 3-5 read the
// clock four times per stage on the pivot wave unconditionally: s_memrealtime is a scalar MEMORY instruction (a round trip, and its out-of-order return forces
// lgkmcnt(0) on the wave's LDS traffic) -- on the critical path of all 30 stages.
template <bool LDSP, bool DBG>
__global__ __launch_bounds__(FUSE_THREADS) void ba_solve_fused_kernel(BaDev B, double *__restrict__ x_out, double *__restrict__ upanel,
                                                                      const int *__restrict__ rowmax_g, int R, FuseFronts F) {
  extern __shared__ double smem[];
  if (B.ctl) { if (B.ctl[1] != 0.0) return; B.lambda = B.ctl[0]; }      // speculative trial: lambda decided on the device, skipped after a rejection
  const int front = blockIdx.x, PN = B.P;                                // PN: poses of the whole (natural) system
  const int Pe = front ? F.P1 : F.P_top;                                 // block rows this front eliminates
  const int P = front ? F.P1 + R - 1 : F.P_top;                          // block rows in its view (front 1: + the R-1 shared rows, kept symbolic)
  const int m0 = F.P_top - (R - 1);                                      // first shared row (natural index); shared rows = m0 .. P_top-1
  const bool two = F.P1 > 0;
  // The hand-over flags of the two fronts hold the launch EPOCH.  It lives on the device (flags[2]; front 0 advances it as its last act, when front 1 has long read it): a
  // recorded launch (HIP graph replay, svs_ba_graph_stats) runs with the same arguments every time, and a host-side launch counter would need a flag reset in front of
  // every solve (a 4 us fill kernel on the critical path of every trial).
  const unsigned epoch = two ? __hip_atomic_load(F.flags + 2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) + 1u : 0u;
  rowmax_g += front * PN;
  upanel += (size_t)front * ((size_t)PN * FUSE_SLOTS * 36 + 128);
  const int n = 6 * P, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  // element e = 6 r + c of local block (rl, rl + cb) of this front's matrix
  auto hval = [&](int rl, int cb, int e) -> double {
    if (!front) return B.H[(blk_index(rl, rl, PN) + cb) * 36 + e];
    if (rl >= Pe) return 0.0;                                            // shared rows start from zero: they end up holding the deltas
    const int i = PN - 1 - rl, j = i - cb;                               // natural block (j, i), j <= i; off-diagonal blocks transposed
    const int r = e / 6, c = e - 6 * r;
    return B.H[blk_index(j, i, PN) * 36 + (cb == 0 ? e : 6 * c + r)];
  };
  auto nat = [&](int rl) { return front ? PN - 1 - rl : rl; };
  double *s_b = smem;                          // [n]
  double *s_win = s_b + n;                     // [R][R][36] ring of envelope rows
  double *s_pz = s_win + (size_t)R * R * 36;   // [2][R][36] Z_kj
  double *s_py = s_pz + 2 * (size_t)R * 36;    // [2][R][36] Y_kj
  double *s_ud = s_py + 2 * (size_t)R * 36;    // [P][36] U_kk (strict upper part)
  double *s_y = s_ud + (size_t)P * 36;         // [2][8]  z_k
  double *s_trash = s_y + 16;                  // [48] sink of the Z stores of the pivot block lanes
  double *s_zero = s_trash + 48;               // [48] zeros: source of the lanes outside the envelope (keeps the LDS loads unconditional)
  int *rowmax = reinterpret_cast<int *>(s_zero + 48);                     // [P] envelope
  unsigned char *lut = reinterpret_cast<unsigned char *>(rowmax + P);     // (ii, jj) of trailing block t, 1 <= ii <= jj
  // Round 6: the panel rows Y the back substitution walks -- [P][10][36], 86 KB for a 30-row front -- stay in LDS where they fit (F.lds_panel, decided by the host: 160 KB
  // per workgroup on gfx950).  Rounds 3-5 sent them through global memory: eleven global stores per stage on the pivot wave, and a global load on every step of
  // the backward chain (12.9 us for 30 rows = 1 000 cycles per row where its dependent readlane / FMA chain is ~250).
  // s_gp: [P][10][36] panel rows, then [400] zeros (what the lanes without a row read)
  // (offset arithmetic from the LDS base: a pointer that has been through an integer cast is a FLAT pointer to the compiler -- flat_load instead of ds_read)
  const int gp_off = (int)((sizeof(double) * (size_t)(s_zero + 48 - smem) + sizeof(int) * (size_t)P + (size_t)R * (R - 1) + 15) / 16) * 2;
  double *const s_gp = smem + gp_off;
  double *const s_gz = s_gp + (size_t)P * FUSE_SLOTS * 36;
  if constexpr (LDSP) { for (int e = tid; e < 400; e += FUSE_THREADS) s_gz[e] = 0.0; }
  __shared__ int s_fail;
  const long long t_begin = DBG ? wall_clock64() : 0;
  if (tid == 0) s_fail = 0;
  if (tid < 48) s_zero[tid] = 0.0;
  for (int i = tid; i < P; i += FUSE_THREADS) rowmax[i] = rowmax_g[i];
  for (int i = tid; i < n; i += FUSE_THREADS) {
    const int rl = i / 6, g = 6 * nat(rl) + (i - 6 * rl);
    s_b[i] = rl < Pe ? B.bp[g] - B.bs[g] : 0.0;
  }
  if (front) {      // shared rows take no part in the elimination: identity U_kk and zero panel rows for the back substitution
    for (int e = tid; e < (P - Pe) * 36; e += FUSE_THREADS) s_ud[(size_t)Pe * 36 + e] = 0.0;
    for (int e = tid; e < (P - Pe) * FUSE_SLOTS * 36; e += FUSE_THREADS) { if constexpr (LDSP) s_gp[(size_t)Pe * FUSE_SLOTS * 36 + e] = 0.0; else upanel[(size_t)Pe * FUSE_SLOTS * 36 + e] = 0.0; }
  }
  for (int t = tid; t < R * (R - 1) / 2; t += FUSE_THREADS) {   // t = jj (jj - 1) / 2 + (ii - 1)
    int jj = 1;
    while ((jj + 1) * jj / 2 <= t) ++jj;
    lut[2 * t] = (unsigned char)(t - jj * (jj - 1) / 2 + 1);
    lut[2 * t + 1] = (unsigned char)jj;
  }
  {   // the first R envelope rows: all loads of a lane in flight together (one global round trip, not one per row)
    constexpr int NI = (FUSE_SLOTS * FUSE_SLOTS * 36 + FUSE_THREADS - 1) / FUSE_THREADS;
    const int rows0 = min(R, P), total = rows0 * R * 36;
    double v[NI];
#pragma unroll
    for (int u = 0; u < NI; ++u) {
      const int e = tid + u * FUSE_THREADS, r = e / (R * 36), rem = e - r * R * 36, c = rem / 36;
      v[u] = (e < total && r + c < P) ? hval(r, c, rem - c * 36) : 0.0;
    }
#pragma unroll
    for (int u = 0; u < NI; ++u) { const int e = tid + u * FUSE_THREADS; if (e < total) s_win[e] = v[u]; }      // row r of the ring = slot r % R = r
  }
  constexpr int LDN = (FUSE_SLOTS * 36 + 63) / 64;     // loader registers per lane and buffer
  double ra[LDN], rb_[LDN];
  auto load_row = [&](double (&reg)[LDN], int rn) {
    if (rn < P) {
#pragma unroll
      for (int i = 0; i < LDN; ++i) {
        const int e = lane + 64 * i;
        const int c = e / 36;
        reg[i] = (e < R * 36 && rn + c < P) ? hval(rn, c, e - c * 36) : 0.0;
      }
    }
  };
  auto store_row = [&](const double (&reg)[LDN], int k, int ringk) {      // ringk = k % R
    if (k + R < P) {
      double *row = s_win + (ringk * R) * 36;
#pragma unroll
      for (int i = 0; i < LDN; ++i) { const int e = lane + 64 * i; if (e < R * 36) row[e] = reg[i]; }
    }
  };
  if (wave == 4) { load_row(ra, R); load_row(rb_, R + 1); }
  __syncthreads();

  // ---- pivot wave state: lane (slot, c) <-> column c of block column j, j % 10 == slot; lane 60 <-> rhs
  const int slot = lane / 6, cc = lane - slot * 6;
  const bool col_lane = lane < 6 * FUSE_SLOTS, rhs_lane = lane == 6 * FUSE_SLOTS;
  double ycol[6] = {0, 0, 0, 0, 0, 0};          // this lane's column of Y_k (rhs lane: w_k); 0 outside panel k
  int failed = 0;
  long long t_ld = 0;
  double *const g_trash = upanel + (size_t)PN * FUSE_SLOTS * 36;     // 64 spare doubles behind this front's panel rows (write sink)
  const double *const g_zero = g_trash + 64;                         // 64 zeros (never written)
  // stage for pivot row p: apply panel p-1 (nj_prev blocks), eliminate, emit panel p
  auto pivot_stage = [&](int p, int nj_prev, int njp, int jp, int ringp, bool apply_only = false) {      // jp = p % 10, ringp = p % R (kept as counters)
    const int pl = jp * 6;
    int off = slot - jp;                                            // block column j = p + off
    off += off < 0 ? FUSE_SLOTS : 0;
    const bool in_env = col_lane && off <= njp, act = in_env || rhs_lane;
    double a[6];
    {
      const double *src = rhs_lane ? (s_b + 6 * p) : in_env ? (s_win + ((ringp * R) + off) * 36 + cc) : s_zero;
      const int stride = rhs_lane ? 1 : 6;
#pragma unroll
      for (int r = 0; r < 6; ++r) a[r] = src[stride * r];
    }
#pragma unroll
    for (int r = 0; r < 6; ++r) a[r] += (in_env && off == 0 && r == cc && !apply_only) ? B.lambda : 0.0;
    if (nj_prev > 0) {
      // block row p gets panel p-1:  a[r] -= sum_q Z_(p-1),p [q][r] * Y_(p-1),j [q][c]
      const double *z0 = s_pz + (size_t)((p - 1) & 1) * R * 36;      // block 0 of panel p-1 is block column p
      double z[36];
#pragma unroll
      for (int i = 0; i < 36; ++i) z[i] = z0[i];
      __builtin_amdgcn_sched_barrier(0);                            // all 18 LDS loads in flight before the first FMA waits
#pragma unroll
      for (int q = 0; q < 6; ++q)
#pragma unroll
        for (int r = 0; r < 6; ++r) a[r] = __builtin_fma(-z[6 * q + r], ycol[q], a[r]);
    }
    if (apply_only) {      // first shared row of front 1: it only receives panel p-1 (the update waves cover rows >= p+1), then rests
      if (rhs_lane) {
#pragma unroll
        for (int r = 0; r < 6; ++r) s_b[6 * p + r] = a[r];
      } else if (in_env) {
#pragma unroll
        for (int r = 0; r < 6; ++r) s_win[((ringp * R) + off) * 36 + 6 * r + cc] = a[r];
      }
      wave_lds_fence();
      return;
    }
    if constexpr (DBG) t_ld = wall_clock64();
    // eliminate the 6 pivots of block (p,p) on every column of the row (multipliers broadcast from the pivot lanes)
    double rd[6];
#pragma unroll
    for (int q = 0; q < 6; ++q) {
      const double rj = rcp_nr(lane_bcast(a[q], pl + q));
      rd[q] = rj;
#pragma unroll
      for (int r = q + 1; r < 6; ++r) {
        const double u = lane_bcast(a[q], pl + r) * rj;            // U_pp[q][r]
        a[r] = __builtin_fma(-u, a[q], a[r]);
      }
    }
    // a non-positive / non-finite pivot shows in its reciprocal; elimination continues (uniform control flow), x is zeroed at the end
#pragma unroll
    for (int q = 0; q < 6; ++q) failed |= !(rd[q] > 0.0 && rd[q] < 1.7976931348623157e308);
    // emit: Z = a, Y = D^-1 a.  Panel columns -> panel buffers + global row; pivot block columns -> U_pp = D^-1 (D U);
    // rhs -> z_p, w_p.  One exec mask for all 18 stores: every lane gets its own destinations and strides.
    const bool in_panel = in_env && off >= 1;
    double *dZ, *dY, *dG = (LDSP ? s_trash : g_trash) + lane % 6;
    int sZ = 6, sY = 6;
    if (rhs_lane) { dZ = s_y + (p & 1) * 8; dY = s_b + 6 * p; sZ = 1; sY = 1; }
    else if (off == 0) { dZ = s_trash + cc; dY = s_ud + (size_t)p * 36 + cc; }
    else {
      dZ = s_pz + ((size_t)(p & 1) * R + (off - 1)) * 36 + cc;
      dY = s_py + ((size_t)(p & 1) * R + (off - 1)) * 36 + cc;
      dG = (LDSP ? s_gp : upanel) + ((size_t)p * FUSE_SLOTS + (off - 1)) * 36 + cc;
    }
    if (act) {
#pragma unroll
      for (int q = 0; q < 6; ++q) {
        const double y = a[q] * rd[q];
        ycol[q] = y;
        dZ[sZ * q] = a[q];
        dY[sY * q] = y;
        dG[6 * q] = y;
      }
    } else if (col_lane) {      // outside the envelope of row p: zero block for the unconditional loads of the back substitution
#pragma unroll
      for (int q = 0; q < 6; ++q) dG[6 * q] = 0.0;
    }
#pragma unroll
    for (int q = 0; q < 6; ++q) ycol[q] = (in_panel || rhs_lane) ? ycol[q] : 0.0;
    wave_lds_fence();
  };
  auto env_len = [&](int k) { return k < P ? rowmax[k] - k : 0; };
  if (wave == 0) __builtin_amdgcn_s_setprio(3);      // the pivot wave is the critical path of every stage
  if (wave == 0) pivot_stage(0, 0, env_len(0), 0, 0);
  lds_barrier();
  const long long t_loop = DBG ? wall_clock64() : 0;
  long long acc_piv = 0, acc_bar = 0, acc_ld = 0;      // pivot-wave stage breakdown (SVS_BA_DEBUG)
  // One loop per role (P stages, one lds_barrier each).  Separate loops keep the compiler's wait-count
  // bookkeeping apart: in a shared loop body the pivot wave waited every stage for vmcnt(0) -- the round
  // trip of its own panel stores -- because the loader's loads were pending on the merged path.
  // front 0, entering stage inj_k: the shared rows m0 .. P_top-1 are all inside the LDS window and none has been consumed
  // yet -- wait for front 1, add its deltas (update waves), one extra barrier for every role
  const int inj_k = (two && !front) ? m0 - 1 : -1;
  bool wait_failed = false;
  auto inject = [&]() {
    if (wave >= 1 && wave <= 3) {
      if (!fuse_wait_flag(F.flags, epoch)) wait_failed = true;
      const int ul = tid - 64, nsh = R - 1;
      // front 1's local block (P1 + a, P1 + a + d) is natural block (j, i), i = P_top-1-a, j = i-d, transposed
      for (int e = ul; e < nsh * R * 36; e += 192) {
        const int a = e / (R * 36), rem = e - a * R * 36, d = rem / 36, q = rem - d * 36, r = q / 6, c = q - 6 * r;
        if (a + d < nsh) {
          const int i = F.P_top - 1 - a, j = i - d;
          s_win[(((j % R) * R) + d) * 36 + 6 * c + r] += F.xfer[e];
        }
      }
      for (int e = ul; e < nsh * 6; e += 192) { const int a = e / 6; s_b[6 * (F.P_top - 1 - a) + (e - 6 * a)] += F.xfer[nsh * R * 36 + e]; }
    }
    lds_barrier();
  };
  if (wave == 0) {
    int nj_a = env_len(0), nj_b = env_len(1), nj_c = env_len(2);      // envelope lengths of rows k, k+1, k+2 (read ahead of use)
    int ring1 = 1 % R, slot1 = 1 % FUSE_SLOTS;                         // (k + 1) % R and (k + 1) % 10
    for (int k = 0; k < Pe; ++k) {
      if (k == inj_k) inject();
      const int nj = nj_a, nj_nx = nj_b;
      nj_a = nj_b; nj_b = nj_c; nj_c = env_len(k + 3);
      long long ts0 = 0, ts3 = 0;
      if constexpr (DBG) ts0 = wall_clock64();
      if (k + 1 < Pe) pivot_stage(k + 1, nj, nj_nx, slot1, ring1);
      else if (k + 1 < P) pivot_stage(k + 1, nj, nj_nx, slot1, ring1, true);
      ring1 = ring1 + 1 == R ? 0 : ring1 + 1;
      slot1 = slot1 + 1 == FUSE_SLOTS ? 0 : slot1 + 1;
      if constexpr (DBG) ts3 = wall_clock64();
      lds_barrier();
      if constexpr (DBG) { acc_piv += ts3 - ts0; acc_bar += (long long)wall_clock64() - ts3; acc_ld += t_ld - ts0; }
    }
  } else if (wave <= 3) {
    const int ul = tid - 64;
    int nj_a = env_len(0), nj_b = env_len(1);
    int ring1 = 1 % R;
    for (int k = 0; k < Pe; ++k) {
      if (k == inj_k) inject();
      const int nj = nj_a;
      nj_a = nj_b; nj_b = env_len(k + 2);
      const double *pz = s_pz + (size_t)(k & 1) * R * 36, *py = s_py + (size_t)(k & 1) * R * 36, *zk = s_y + (k & 1) * 8;
      // trailing blocks (ii >= 1): lane = (block, column pair)
      const int nb = nj * (nj - 1) / 2;
      for (int e = ul; e < nb * 3; e += 192) {
        const int t = e / 3, c2 = 2 * (e - t * 3);
        const int ii = lut[2 * t], jj = lut[2 * t + 1];
        double y0[6], y1[6];
#pragma unroll
        for (int q = 0; q < 6; ++q) { y0[q] = py[(size_t)jj * 36 + 6 * q + c2]; y1[q] = py[(size_t)jj * 36 + 6 * q + c2 + 1]; }
        int ring = ring1 + ii;
        ring -= ring >= R ? R : 0;
        double *Aij = s_win + ((ring * R) + (jj - ii)) * 36 + c2;
        const double *zi = pz + (size_t)ii * 36;
#pragma unroll
        for (int r = 0; r < 6; ++r) {
          double s0 = 0, s1 = 0;
#pragma unroll
          for (int q = 0; q < 6; ++q) { s0 = __builtin_fma(zi[6 * q + r], y0[q], s0); s1 = __builtin_fma(zi[6 * q + r], y1[q], s1); }
          Aij[6 * r] -= s0; Aij[6 * r + 1] -= s1;
        }
      }
      // b~_(k+1+jj) -= Y_k,jj^T z_k  for jj >= 1 (block row k+1 is the pivot wave's)
      for (int e = ul; e < (nj - 1) * 6; e += 192) {
        const int jj = 1 + e / 6, c = e % 6;
        double s0 = 0, s1 = 0;
#pragma unroll
        for (int q = 0; q < 6; q += 2) {
          s0 = __builtin_fma(py[(size_t)jj * 36 + 6 * q + c], zk[q], s0);
          s1 = __builtin_fma(py[(size_t)jj * 36 + 6 * (q + 1) + c], zk[q + 1], s1);
        }
        s_b[6 * (k + 1 + jj) + c] -= s0 + s1;
      }
      ring1 = ring1 + 1 == R ? 0 : ring1 + 1;
      lds_barrier();
    }
  } else {
    int ringk = 0;
    for (int k = 0; k < Pe; ++k) {
      if (k == inj_k) inject();
      if (k & 1) { store_row(rb_, k, ringk); load_row(rb_, k + R + 2); }
      else { store_row(ra, k, ringk); load_row(ra, k + R + 2); }
      ringk = ringk + 1 == R ? 0 : ringk + 1;
      lds_barrier();
    }
  }
  if (wave == 0 && __any(failed)) s_fail = 1;
  if (__any(wait_failed) && lane == 0) s_fail = 1;
  __syncthreads();
  if (front) {
    // hand the deltas of the shared rows to front 0, then wait for their solution
    const int nsh = R - 1;
    for (int e = tid; e < nsh * R * 36; e += FUSE_THREADS) {
      const int a = e / (R * 36), rem = e - a * R * 36;
      F.xfer[e] = s_win[(((Pe + a) % R) * R) * 36 + rem];
    }
    for (int e = tid; e < nsh * 6; e += FUSE_THREADS) F.xfer[nsh * R * 36 + e] = s_b[6 * Pe + e];
    __threadfence();
    __syncthreads();
    if (tid == 0) __hip_atomic_store(F.flags, epoch, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
    if (wave == 0) {
      if (!fuse_wait_flag(F.flags + 1, epoch)) { if (lane == 0) s_fail = 1; }
      const double *xs = F.xfer + nsh * R * 36 + nsh * 6;              // x of natural rows m0 .. P_top-1
      for (int e = lane; e < nsh * 6; e += 64) { const int a = e / 6; s_b[6 * (Pe + a) + (e - 6 * a)] = xs[6 * (nsh - 1 - a) + (e - 6 * a)]; }
    }
    __syncthreads();
  }
  const int fail = s_fail;
  const long long t_fwd = DBG ? wall_clock64() : 0;
  const bool publish = two && !front;
  double *const xpub = F.xfer + (R - 1) * R * 36 + (R - 1) * 6;
  if (wave == 0) {
    if (!fail) {
      if constexpr (LDSP) {
      // ---- back substitution, round 6.  Lane (g, r), g = lane / 6 < 10, carries component r of ONE row at a time: the rows i with (P-1-i) % 10 == g, one after the
      // other.  Step t solves x_k, k = P-1-t: the pivot group of step t is t % 10, so with the loop unrolled ten times every lane index of a broadcast, every role and
      // every register of the prefetch ring is STATIC (rounds 3-5: the roles rotated at run time -- 270 instructions per step under ten exec-mask regions, 1 000 cycles
      // where the dependent readlane / FMA chain of a step is ~250).  Per step: 12 readlanes + 5 FMAs on the pivot lanes (U_kk), 6 FMAs on every lane (its row's block
      // Y_(i,k) times x_k), the pivot lanes store x_k and move on to their next row (state loaded one body ahead), and the block for the step four ahead is requested
      // from the LDS panel (three 16-byte reads from an address that is linear in (row, k): row * 324 + 36 (k - 1) + 6 r doubles).
      const int g = slot, r = cc;
      constexpr int PF = 4;                                          // steps between the request of a block and its use
      auto row_state = [&](int i, double &w, double (&u)[6]) {      // w_i[r], U_ii[r][r+1..5]; zeros for a lane without a row
        const bool ok = i >= 0 && col_lane;
        w = ok ? s_b[6 * i + r] : 0.0;
#pragma unroll
        for (int rr = 1; rr < 6; ++rr) u[rr] = (ok && rr > r) ? s_ud[(size_t)i * 36 + 6 * r + rr] : 0.0;
      };
      int irow = col_lane ? P - 1 - g : -1;                          // the row this lane carries (negative: none)
      int lrow = irow;                                               // ... as seen by the load stream, which runs PF steps ahead
      const int zoff = (int)(s_gz - s_gp);                           // the zero region behind the panel rows
      double acc, ucol[6], wn, un[6], wn2 = 0, un2[6] = {0, 0, 0, 0, 0, 0};
      row_state(irow, acc, ucol);
      row_state(irow - FUSE_SLOTS, wn, un);
      double yq[FUSE_SLOTS][6];
      // the block of step t' (k' = P-1-t'): row lrow's block against column k'
      auto request = [&](double (&y)[6], int kq, int dq) {           // dq = t' % 10 (static)
        // a lane has moved on to its next row once its pivot step is behind it
        if (dq > 0) { if (g == dq - 1) lrow -= FUSE_SLOTS; } else { if (g == FUSE_SLOTS - 1 && kq != P - 1) lrow -= FUSE_SLOTS; }
        const int e = (lrow >= 0 && kq >= 0) ? lrow * 324 + 36 * (kq - 1) + 6 * r : zoff + 36;      // (the pivot lanes of the step read the block before theirs: ignored)
        const double *src = s_gp + e;
#pragma unroll
        for (int c = 0; c < 6; ++c) y[c] = src[c];
      };
#pragma unroll
      for (int d = 0; d < PF; ++d) request(yq[d], P - 1 - d, d);
      for (int kb = P - 1; kb >= 0; kb -= FUSE_SLOTS) {
        row_state(irow - 2 * FUSE_SLOTS - (false ? 0 : 0), wn2, un2);      // (every lane carries its row of this body here: nobody has been pivot yet)
#pragma unroll
        for (int d = 0; d < FUSE_SLOTS; ++d) {
          const int k = kb - d;
          if (k >= 0) {
            const int pl = 6 * d;
            const bool piv = g == d && col_lane;
            double xs[6];
#pragma unroll
            for (int rr = 5; rr >= 1; --rr) {
              xs[rr] = lane_bcast(acc, pl + rr);
              acc = __builtin_fma(piv ? -ucol[rr] : 0.0, xs[rr], acc);
            }
            xs[0] = lane_bcast(acc, pl);
            if (piv) {
              s_b[6 * k + r] = acc;                                   // x_k
              if (publish && k >= m0) xpub[6 * (k - m0) + r] = acc;
            }
            double s0 = 0, s1 = 0;
#pragma unroll
            for (int c = 0; c < 6; c += 2) { s0 = __builtin_fma(yq[d][c], xs[c], s0); s1 = __builtin_fma(yq[d][c + 1], xs[c + 1], s1); }
            acc = piv ? wn : acc - (s0 + s1);
            irow = piv ? irow - FUSE_SLOTS : irow;
            if (publish && k == m0) {                                 // the shared rows are solved: release front 1
              __threadfence();
              if (lane == 0) __hip_atomic_store(F.flags + 1, epoch, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
            }
            request(yq[(d + PF) % FUSE_SLOTS], k - PF, (d + PF) % FUSE_SLOTS);
          }
        }
        // every lane has been pivot once: the state loaded during this body becomes the next row's
        wn = wn2;
#pragma unroll
        for (int rr = 1; rr < 6; ++rr) { ucol[rr] = un[rr]; un[rr] = un2[rr]; }
      }
      } else {
      // ---- back substitution: lane (slot, r) carries component r of row i, i % 10 == slot
      const int r = cc;
      // lane state: dist = (k - slot) mod 10 for the step being prefetched (row i = k - dist; dist == 0: pivot lane)
      auto load_row_state = [&](int i, double &w, double (&u)[6]) {      // w_i[r], U_ii[r][r+1..5]
        const bool ok = i >= 0 && col_lane;
        w = ok ? s_b[6 * i + r] : 0.0;
#pragma unroll
        for (int rr = 1; rr < 6; ++rr) u[rr] = (ok && rr > r) ? s_ud[(size_t)i * 36 + 6 * r + rr] : 0.0;
      };
      int kp = P - 1;                                              // step whose panel row is fetched next
      int distp = (kp % FUSE_SLOTS) - slot;
      distp += distp < 0 ? FUSE_SLOTS : 0;
      auto load_y = [&](double (&y)[6]) {                          // Y_(i,kp)[r][:], i = kp - distp;  0 on the pivot lanes
        const int i = kp - distp;
        const bool ok = col_lane && distp > 0 && i >= 0;
        // unconditional loads (lanes without a block read a zero block): predicated loads would make the compiler drain
        // vmcnt to 0 every step and put a full global round trip on the chain
        const double *src = ok ? upanel + ((size_t)i * FUSE_SLOTS + (distp - 1)) * 36 + 6 * r : g_zero;
#pragma unroll
        for (int c = 0; c < 6; ++c) y[c] = src[c];
        --kp;
        distp = distp == 0 ? FUSE_SLOTS - 1 : distp - 1;
      };
      double yq[FUSE_PRE][6];
#pragma unroll
      for (int d = 0; d < FUSE_PRE; ++d) load_y(yq[d]);
      double acc, wnext, ucol[6], ucolnext[6];
      int dist = ((P - 1) % FUSE_SLOTS) - slot;
      dist += dist < 0 ? FUSE_SLOTS : 0;
      load_row_state(P - 1 - dist, acc, ucol);
      load_row_state(P - 1 - dist - FUSE_SLOTS, wnext, ucolnext);
      int sk = (P - 1) % FUSE_SLOTS;
      for (int kb = P - 1; kb >= 0; kb -= FUSE_PRE) {
#pragma unroll
        for (int d = 0; d < FUSE_PRE; ++d) {
          const int k = kb - d;
          if (k >= 0) {
            const int pl = sk * 6;
            const bool piv = col_lane && dist == 0;
            double cm[6], xs[6];
#pragma unroll
            for (int rr = 1; rr < 6; ++rr) cm[rr] = piv ? ucol[rr] : 0.0;
#pragma unroll
            for (int rr = 5; rr >= 1; --rr) {
              xs[rr] = lane_bcast(acc, pl + rr);
              acc = __builtin_fma(-cm[rr], xs[rr], acc);
            }
            xs[0] = lane_bcast(acc, pl);
            if (piv) {
              s_b[6 * k + r] = acc;                                   // x_k
              if (publish && k >= m0) xpub[6 * (k - m0) + r] = acc;
              acc = wnext;
#pragma unroll
              for (int rr = 1; rr < 6; ++rr) ucol[rr] = ucolnext[rr];
              load_row_state(k - 2 * FUSE_SLOTS, wnext, ucolnext);
            }
            double s0 = 0, s1 = 0;
#pragma unroll
            for (int c = 0; c < 6; c += 2) { s0 = __builtin_fma(yq[d][c], xs[c], s0); s1 = __builtin_fma(yq[d][c + 1], xs[c + 1], s1); }
            acc -= s0 + s1;
            if (publish && k == m0) {                                 // the shared rows are solved: release front 1
              __threadfence();
              if (lane == 0) __hip_atomic_store(F.flags + 1, epoch, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
            }
            load_y(yq[d]);
            sk = sk == 0 ? FUSE_SLOTS - 1 : sk - 1;
            dist = dist == 0 ? FUSE_SLOTS - 1 : dist - 1;
          }
        }
      }
      }
    } else {
      for (int i = lane; i < n; i += 64) s_b[i] = 0;
      if (publish) {                                                   // a failed factorisation still releases front 1 (the step is rejected anyway)
        for (int i = lane; i < (R - 1) * 6; i += 64) xpub[i] = 0.0;
        __threadfence();
        if (lane == 0) __hip_atomic_store(F.flags + 1, epoch, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
      }
    }
  }
  __syncthreads();
  const long long t_back = DBG ? wall_clock64() : 0;
  double sc = 0;
  for (int i = tid; i < 6 * Pe; i += FUSE_THREADS) {
    const int rl = i / 6, g = 6 * nat(rl) + (i - 6 * rl);
    const double xv = s_b[i];
    x_out[g] = xv;
    sc += xv * (B.lambda * xv + B.bp[g]);
  }
  sc = wave_sum(sc);
  if ((tid & 63) == 0 && sc != 0.0) atomic_add_f64(&B.scal[2], sc);
  for (int p = tid; p < Pe; p += FUSE_THREADS) {
    double Tn[12];
    const int g = nat(p);
    d_se3_exp_mul(s_b + 6 * p, B.poses + 12 * (size_t)g, Tn);
    for (int i = 0; i < 12; ++i) B.poses_trial[12 * (size_t)g + i] = Tn[i];
  }
  if (tid == 0 && fail) B.scal[3] = 1.0;                               // zeroed before every trial by the Schur kernel / the host memset
  if (tid == 0 && !front && two) __hip_atomic_store(F.flags + 2, epoch, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  if (tid == 0 && !front) {
    B.scal[4] = chi2_cur_sum(B);
    B.scal[5] = (double)(t_loop - t_begin) * 0.01; B.scal[6] = (double)(t_fwd - t_loop) * 0.01; B.scal[7] = (double)(t_back - t_fwd) * 0.01;
    B.scal[8] = acc_ld * 0.01; B.scal[9] = (acc_piv - acc_ld) * 0.01; B.scal[10] = 0; B.scal[11] = acc_bar * 0.01;
  }
}

