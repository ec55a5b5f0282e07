// ba_solve_tiles.inc -- the reduced pose system of a WIDE envelope (double window with loop closures / long tracks: a near-dense
// 1 380 x 1 380 system at 230 poses) as a tile-resident blocked Cholesky over three quarters of the CUs.  Replaces ba_solve_grid_kernel's scheme
// (one 6 x 6 block row per step, the whole trailing matrix read and written through global memory every step: O(n^3) bytes, 2.1 GB
// written per launch) where it is selected (ba.hip).  Same role as the other solve kernels: g2o's LinearSolver on the Schur
// complement (BlockSolver::solve, external; SlamGraph::optimize -> optimizer.optimize, slam_graph.cpp:259-303).
//
//   * the matrix is cut into 24 x 24 tiles (4 x 4 pose blocks); tile (I, J), I <= J, belongs to workgroup (I mod g, J mod g) of a g x g grid (g = 14 on 256 CUs) and
//     lives in that workgroup's LDS from the first to the last step -- no tile ever travels to global memory and back;
//   * step s: the finished tile row s (published by its owners at the end of step s-1: 24 rows of the matrix, once) is read by whoever
//     needs it: every workgroup factors the 24 x 24 pivot tile itself (cheaper than handing the factor around), solves U(s,c) =
//     U_ss^-T A(s,c) for the <= 2 ceil(S / g) columns c its tiles need, and applies A(I,J) -= U(s,I)^T U(s,J) to its tiles in LDS
//     (4 x 6 register blocks);  the right-hand side rides along as one more column (forward substitution);
//   * ONE device-scope arrival per step (same counters as the grid kernel); global traffic per step = the published row (written once,
//     read by the workgroups that need a column of it) -- the matrix is written once in total, plus the factor for the back substitution;
//   * the owners of row s store U(s,c) transposed into a tile-packed factor buffer; workgroup 0 runs the back substitution from it.
constexpr int TS_M = 4, TS_N = 6 * TS_M, TS_T = TS_N * TS_N;      // pose blocks per tile edge, scalars per tile edge, doubles per tile
constexpr int TS_THREADS = 256;
constexpr int TS_MAXT = 16;                                       // own tiles per workgroup at most
// the workgroup's tile table in LDS (ints): I and J of the own tiles, the panel cache slots of their columns I / J, the column list, the step's job list
constexpr int TM_I = 0, TM_J = TS_MAXT, TM_CI = 2 * TS_MAXT, TM_CJ = 3 * TS_MAXT, TM_NCOL = 4 * TS_MAXT, TM_COL = TM_NCOL + 1, TM_NCJ = TM_COL + 2 * TS_MAXT, TM_NJOB = TM_NCJ + 1,
              TM_JOB = TM_NJOB + 1, TM_INTS = TM_JOB + 3 * TS_MAXT;


struct TilesArgs {
  int S, tpw, gq, ncm;        // tile rows (= ceil(P / 4)), own tiles per workgroup at most, edge of the square workgroup grid (gq * gq workgroups), panel columns per workgroup at most
  double *rowbuf;             // [2][S][TS_T]  published tile row of a step (by step parity) ...
  double *bbuf;               // [2][TS_N]     ... and its piece of the right-hand side
  double *ufac;               // [#tiles][TS_T] U(s,c) TRANSPOSED ([column][row]), by linear tile index
  double *ybuf;               // [S][2 TS_N]   y_s, then 1 / diag(U_ss)
  unsigned *bar;              // arrival counters (bar[32 i], i < GRID_NBAR) + failure flag (bar[32 GRID_NBAR])
};
__host__ __device__ inline long ts_tile_index(int I, int J, int S) { return (long)I * S - (long)I * (I - 1) / 2 + (J - I); }
__host__ inline size_t ts_ws_doubles(int S) { return 2 * (size_t)S * TS_T + 2 * TS_N + (size_t)S * (S + 1) / 2 * TS_T + 2 * (size_t)S * TS_N; }
__host__ inline size_t ts_lds_bytes(int tpw, int ncm) { return sizeof(double) * ((size_t)(tpw + ncm + 1) * TS_T + (size_t)tpw * TS_N + 2 * TS_N) + (size_t)TM_INTS * sizeof(int); }

// forward substitution with the factored pivot tile: u = U_ss^-T a for one column held in registers (a -> u in place), right-looking: as soon as u[q] is
// final it leaves every later row -- the updates of a step are independent of each other and read ROW q of U (contiguous in LDS, the same address in every
// lane: broadcast, two values per read).  rd = 1 / diag(U)
__device__ __forceinline__ void ts_fwd_col(const double *s_piv, const double *s_rd, double (&a)[TS_N]) {
#pragma unroll
  for (int q = 0; q < TS_N; ++q) {
    const double u = a[q] * s_rd[q];
    a[q] = u;
#pragma unroll
    for (int r = q + 1; r < TS_N; ++r) a[r] = __builtin_fma(-s_piv[q * TS_N + r], u, a[r]);
  }
}

__global__ __launch_bounds__(TS_THREADS) void ba_solve_tiles_kernel(BaDev B, double *__restrict__ x_out, TilesArgs A) {
  extern __shared__ double smem[];
  if (B.ctl) { if (B.ctl[1] != 0.0) return; B.lambda = B.ctl[0]; }
  const int P = B.P, n = 6 * P, S = A.S, tpw = A.tpw, tid = threadIdx.x, wg = blockIdx.x, G = gridDim.x, lane = tid & 63;
  double *s_tile = smem;                                   // [tpw][TS_T] own tiles
  double *s_cache = s_tile + (size_t)tpw * TS_T;           // [ncm][TS_T] U(s,c) of the columns the own tiles need
  double *s_piv = s_cache + (size_t)A.ncm * TS_T;          // [TS_T] pivot tile -> U_ss (upper)
  double *s_bown = s_piv + TS_T;                           // [tpw][TS_N] right-hand side pieces of the own diagonal tiles
  double *s_rd = s_bown + (size_t)tpw * TS_N;              // [TS_N] 1 / diag(U_ss)
  double *s_y = s_rd + TS_N;                               // [TS_N] b_s -> y_s
  int *s_meta = reinterpret_cast<int *>(s_y + TS_N);   // the workgroup's tile table (TM_* above)
  __shared__ int s_fail;
  if (tid == 0) {
    s_fail = 0;
    // own tiles: (I, J), I <= J, with I = a and J = b modulo the edge of the square workgroup grid, wg = a * GQ + b -- the tiles of one workgroup share their
    // rows and columns, so it needs <= 2 ceil(S / GQ) columns of a step's panel row (a linear deal needed two per tile: 1.7 x the traffic and the panel work)
    const int GQ = A.gq, ga = wg / GQ, gb = wg - ga * GQ;
    int ncol = 0, nt = 0;
    for (int t = 0; t < tpw; ++t) { s_meta[TM_I + t] = -1; s_meta[TM_J + t] = -1; s_meta[TM_CI + t] = -1; s_meta[TM_CJ + t] = -1; }
    for (int I = ga; I < S; I += GQ)
      for (int J = gb; J < S; J += GQ) {
        if (I > J || nt >= tpw) continue;
        s_meta[TM_I + nt] = I; s_meta[TM_J + nt] = J;
        for (int side = 0; side < 2; ++side) {
          const int c = side ? J : I;
          int slot = -1;
          for (int k = 0; k < ncol; ++k) if (s_meta[TM_COL + k] == c) slot = k;
          if (slot < 0 && ncol < A.ncm) { slot = ncol; s_meta[TM_COL + ncol++] = c; }
          s_meta[TM_CI + TS_MAXT * side + nt] = slot;
        }
        ++nt;
      }
    s_meta[TM_NCOL] = ncol;
  }
  __syncthreads();
  const int ncol = s_meta[TM_NCOL];
  // ---- own tiles from the packed block storage (upper block triangle; diagonal blocks: their upper triangle), lambda on the diagonal, identity padding
  auto h_elem = [&](int gi, int gj) -> double {
    if (gi >= n || gj >= n) return gi == gj ? 1.0 : 0.0;
    int bi = gi / 6, bj = gj / 6, ri = gi - 6 * bi, rj = gj - 6 * bj;
    if (bi > bj || (bi == bj && ri > rj)) { int t = bi; bi = bj; bj = t; t = ri; ri = rj; rj = t; }
    const double v = B.H[blk_index(bi, bj, P) * 36 + 6 * ri + rj];
    return gi == gj ? v + B.lambda : v;
  };
  for (int t = 0; t < tpw; ++t) {
    const int I = s_meta[TM_I + t], J = s_meta[TM_J + t];
    if (I < 0) continue;
    for (int e = tid; e < TS_T; e += TS_THREADS) { const int r = e / TS_N, c = e - r * TS_N; s_tile[(size_t)t * TS_T + e] = h_elem(TS_N * I + r, TS_N * J + c); }
    if (I == J && tid < TS_N) { const int g = TS_N * I + tid; s_bown[t * TS_N + tid] = g < n ? B.bp[g] - B.bs[g] : 0.0; }
  }
  __syncthreads();
  auto publish_row = [&](int row) {      // own tiles of tile row `row` (final) -> the row buffer of that step's parity
    for (int t = 0; t < tpw; ++t) {
      if (s_meta[TM_I + t] != row) continue;
      const int J = s_meta[TM_J + t];
      double *dst = A.rowbuf + ((size_t)(row & 1) * S + J) * TS_T;
      for (int e = tid; e < TS_T; e += TS_THREADS) g_st(dst + e, s_tile[(size_t)t * TS_T + e]);
      if (J == row && tid < TS_N) g_st(A.bbuf + (row & 1) * TS_N + tid, s_bown[t * TS_N + tid]);
    }
  };
  unsigned arrivals = 0;
  auto arrive_and_wait = [&]() {         // every workgroup's stores of this step are on their way; wait until everybody's are (as in ba_solve_grid_kernel)
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    ++arrivals;
    if (tid < 64) {
      if (tid == 0) __hip_atomic_fetch_add(A.bar + 32 * (wg % GRID_NBAR), 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      const bool mine = tid < GRID_NBAR && tid < G;
      const unsigned n_here = mine ? (unsigned)((G - tid + GRID_NBAR - 1) / GRID_NBAR) : 0u;
      const unsigned want = n_here * arrivals;
      long spin = 0;
      bool late = false;
      for (;;) {
        const unsigned v = mine ? __hip_atomic_load(A.bar + 32 * tid, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : want;
        if (__all((int)(v - want) >= 0)) break;
        if (++spin >= (1l << 22)) { late = true; break; }
        __builtin_amdgcn_s_sleep(1);
      }
      if (tid == 0) {
        if (late) __hip_atomic_store(A.bar + 32 * GRID_NBAR, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (__hip_atomic_load(A.bar + 32 * GRID_NBAR, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0) s_fail = 2;
      }
    }
    __syncthreads();
  };
  const long long t_begin = wall_clock64();
  long long acc_t[5] = {0, 0, 0, 0, 0}, ts = 0;      // workgroup 0: where the time of a step goes (SVS_BA_DEBUG): loads | pivot | panel | update + publish | arrival
#define TS_LAP(i) do { const long long tn = wall_clock64(); acc_t[i] += tn - ts; ts = tn; } while (0)
  auto build_jobs = [&](int step) {      // lane 0: the cache slots whose column lies right of `step` (they are loaded and solved in that step), then the own tiles of row `step`
    int nj = 0;
    for (int k = 0; k < ncol; ++k) if (s_meta[TM_COL + k] > step) s_meta[TM_JOB + nj++] = k;
    s_meta[TM_NCJ] = nj;
    for (int t = 0; t < tpw; ++t) if (s_meta[TM_I + t] == step) s_meta[TM_JOB + nj++] = ~t;
    s_meta[TM_NJOB] = nj;
  };
  publish_row(0);
  if (tid == 0) build_jobs(0);
  arrive_and_wait();
  const long long t_loop = wall_clock64();
  for (int s = 0; s < S && !s_fail; ++s) {
    ts = wall_clock64();
    const double *row = A.rowbuf + (size_t)(s & 1) * S * TS_T;
    // ---- loads of the step: pivot tile, b_s, the columns c > s of the own tiles (raw A(s,c) into the cache); other workgroups wrote them: agent-scope loads.
    //      (Measured and dropped: an agent-scope acquire after the arrival + ordinary 16-byte loads -- the L1 invalidate cost more than the wider requests saved:
    //      8.0 against 5.8 us per step; the phase moves (1 + columns) x 4.6 KB per workgroup and step from the other XCDs and is bound by that traffic.)
    for (int e = tid; e < TS_T; e += TS_THREADS) s_piv[e] = g_ld(row + (size_t)s * TS_T + e);
    if (tid < TS_N) s_y[tid] = g_ld(A.bbuf + (s & 1) * TS_N + tid);
    {
      const int n_colj = s_meta[TM_NCJ];
      for (int e = tid; e < n_colj * TS_T; e += TS_THREADS) {
        const int jb = e / TS_T, w = e - jb * TS_T, slot = s_meta[TM_JOB + jb];
        s_cache[(size_t)slot * TS_T + w] = g_ld(row + (size_t)s_meta[TM_COL + slot] * TS_T + w);
      }
    }
    __syncthreads();
    TS_LAP(0);
    // ---- pivot tile: U_ss (upper) by the lanes of wave 0, lane c = column c, the elements of other columns by readlane
    if (tid < 64) {
      const int c = tid < TS_N ? tid : 0;
      double Ucol[TS_N], acol[TS_N];
#pragma unroll
      for (int j = 0; j < TS_N; ++j) { acol[j] = s_piv[j * TS_N + c]; Ucol[j] = 0.0; }
      int fail = 0;
      double rdv = 0.0;
#pragma unroll
      for (int j = 0; j < TS_N; ++j) {
        double s0 = acol[j], s1 = 0.0, s2 = 0.0, s3 = 0.0;      // A[j][c] - sum_q U[q][j] U[q][c] (meaningful for c >= j), four chains
#pragma unroll
        for (int q = 0; q < j; ++q) {
          const double m = -lane_bcast(Ucol[q], j);
          if ((q & 3) == 0) s0 = __builtin_fma(m, Ucol[q], s0);
          else if ((q & 3) == 1) s1 = __builtin_fma(m, Ucol[q], s1);
          else if ((q & 3) == 2) s2 = __builtin_fma(m, Ucol[q], s2);
          else s3 = __builtin_fma(m, Ucol[q], s3);
        }
        const double sv = (s0 + s1) + (s2 + s3);
        double d = lane_bcast(sv, j);
        if (!(d > 0) || !(d < 1.7976931348623157e308)) { fail = 1; d = 1; }
        // 1 / sqrt(d) from the hardware estimate and two Newton steps (sqrt and a division in IEEE form are ~50 dependent instructions each, 24 times on this chain)
        double y = __builtin_amdgcn_rsq(d);
        const double h = 0.5 * d;
        y = __builtin_fma(__builtin_fma(-h * y, y, 0.5), y, y);
        y = __builtin_fma(__builtin_fma(-h * y, y, 0.5), y, y);
        const double rj = y;
        if (c == j) rdv = rj;
        Ucol[j] = c == j ? d * rj : (c > j ? sv * rj : 0.0);
      }
      if (tid < TS_N) {
#pragma unroll
        for (int j = 0; j < TS_N; ++j) s_piv[j * TS_N + c] = Ucol[j];
        s_rd[c] = rdv;
      }
      if (fail && tid == 0) s_fail = 1;
    }
    __syncthreads();
    TS_LAP(1);
    if (s_fail) break;                                   // every workgroup takes the same decision from the same pivot tile
    // ---- panel: U(s,c) = U_ss^-T A(s,c), one lane per column of a tile.  Jobs: the cached columns c > s (in place in the cache), the own tiles of row s
    //      (in place in the tile; stored transposed into the factor buffer), and the right-hand side piece (one lane)
    {
      const int n_jobs = s_meta[TM_NJOB];                       // (list written by lane 0 before the barrier above) >= 0: cache slot k; < 0: own tile ~t
      for (int e = tid; e < n_jobs * TS_N; e += TS_THREADS) {
        const int jb = e / TS_N, j = e - jb * TS_N, src = s_meta[TM_JOB + jb];
        double *tile = src >= 0 ? s_cache + (size_t)src * TS_T : s_tile + (size_t)(~src) * TS_T;
        double a[TS_N];
#pragma unroll
        for (int r = 0; r < TS_N; ++r) a[r] = tile[r * TS_N + j];
        if (src < 0 && s_meta[TM_J + ~src] == s) {          // the pivot tile itself: its factor is U_ss (column j, zero below the diagonal)
#pragma unroll
          for (int r = 0; r < TS_N; ++r) a[r] = s_piv[r * TS_N + j];
        } else ts_fwd_col(s_piv, s_rd, a);
        if (src >= 0) {
#pragma unroll
          for (int r = 0; r < TS_N; ++r) tile[r * TS_N + j] = a[r];
        } else {
          double *dst = A.ufac + (size_t)ts_tile_index(s, s_meta[TM_J + ~src], S) * TS_T + (size_t)j * TS_N;
#pragma unroll
          for (int r = 0; r < TS_N; ++r) g_st(dst + r, a[r]);
        }
      }
      if (tid == TS_THREADS - 1) {                        // y_s = U_ss^-T b_s
        double a[TS_N];
#pragma unroll
        for (int r = 0; r < TS_N; ++r) a[r] = s_y[r];
        ts_fwd_col(s_piv, s_rd, a);
#pragma unroll
        for (int r = 0; r < TS_N; ++r) s_y[r] = a[r];
        bool owner = false;
        for (int t = 0; t < tpw; ++t) owner = owner || (s_meta[TM_I + t] == s && s_meta[TM_J + t] == s);
        if (owner) {
#pragma unroll
          for (int r = 0; r < TS_N; ++r) { g_st(A.ybuf + (size_t)s * 2 * TS_N + r, a[r]); g_st(A.ybuf + (size_t)s * 2 * TS_N + TS_N + r, s_rd[r]); }
        }
      }
    }
    __syncthreads();
    TS_LAP(2);
    // ---- trailing update of the own tiles below row s: A(I,J) -= U(s,I)^T U(s,J), a 4 x 6 block of the tile per lane (24 lanes per tile, ten tiles at a time;
    //      the pass is bound by LDS bandwidth: 80 bytes of panel per 24 multiply-adds -- 6 x 6 blocks, one round for 15 tiles, measured slower)
    {
      constexpr int UR = 4, UC = 6, LPT = (TS_N / UR) * (TS_N / UC), TPR = TS_THREADS / LPT;      // block rows / columns, lanes per tile, tiles per round
      const int sub = tid % LPT, tsel = tid / LPT;
      const int rb = sub / (TS_N / UC), cb = sub - (TS_N / UC) * rb;                      // rows UR rb .. , columns UC cb ..
      for (int t0 = 0; t0 < tpw; t0 += TPR) {
        const int t = t0 + tsel;
        if (tsel < TPR && t < tpw && s_meta[TM_I + t] > s) {
          const double *Ui = s_cache + (size_t)s_meta[TM_CI + t] * TS_T + UR * rb, *Uj = s_cache + (size_t)s_meta[TM_CJ + t] * TS_T + UC * cb;
          double acc[UR][UC];
#pragma unroll
          for (int r = 0; r < UR; ++r)
#pragma unroll
            for (int c = 0; c < UC; ++c) acc[r][c] = 0.0;
#pragma unroll 4
          for (int q = 0; q < TS_N; ++q) {
            double ui[UR], uj[UC];
#pragma unroll
            for (int r = 0; r < UR; ++r) ui[r] = Ui[q * TS_N + r];
#pragma unroll
            for (int c = 0; c < UC; ++c) uj[c] = Uj[q * TS_N + c];
#pragma unroll
            for (int r = 0; r < UR; ++r)
#pragma unroll
              for (int c = 0; c < UC; ++c) acc[r][c] = __builtin_fma(ui[r], uj[c], acc[r][c]);
          }
          double *T = s_tile + (size_t)t * TS_T + (UR * rb) * TS_N + UC * cb;
#pragma unroll
          for (int r = 0; r < UR; ++r)
#pragma unroll
            for (int c = 0; c < UC; ++c) T[r * TS_N + c] -= acc[r][c];
        }
      }
      // right-hand side pieces of the own diagonal tiles: b_I -= U(s,I)^T y_s
      for (int e = tid; e < tpw * TS_N; e += TS_THREADS) {
        const int t = e / TS_N, r = e - t * TS_N;
        if (s_meta[TM_I + t] > s && s_meta[TM_I + t] == s_meta[TM_J + t]) {
          const double *Ui = s_cache + (size_t)s_meta[TM_CI + t] * TS_T;
          double sv = 0.0;
#pragma unroll
          for (int q = 0; q < TS_N; ++q) sv = __builtin_fma(Ui[q * TS_N + r], s_y[q], sv);
          s_bown[t * TS_N + r] -= sv;
        }
      }
    }
    __syncthreads();
    if (s + 1 < S) publish_row(s + 1);
    if (tid == 0) build_jobs(s + 1);                     // (the panel jobs of this step were read before the barrier above)
    TS_LAP(3);
    arrive_and_wait();
    TS_LAP(4);                                   // (after the last step: the factor is complete for workgroup 0)
  }
  if (wg != 0) return;
  const long long t_fwd = wall_clock64();
  const int fail = s_fail;
  __syncthreads();
  double *s_sol = s_tile;                                  // [S * TS_N] the solution (the own tiles are done with)
  if (!fail) {
    // back substitution, row oriented: x_s = U_ss^-1 (y_s - sum_{c > s} U(s,c) x_c).  The factor was stored by the other workgroups before their last
    // arrival: ONE agent-scope acquire, then ordinary 16-byte loads -- lane (row pair, k) sums the tiles c = s + 1 + k, s + 1 + k + 20, ... of its two rows
    // from the transposed factor (coalesced across the rows), all requests of a step in flight together; the twenty partial sums meet in LDS.
    // (The first version read the factor with 8-byte agent-scope atomic loads: 5.9 us per step.)
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    typedef double ts_d2 __attribute__((ext_vector_type(2)));
    constexpr int NK = 20, NRP = TS_N / 2;
    double *s_part = s_cache;                              // [NK][TS_N]
    for (int s = S - 1; s >= 0; --s) {
      const int rp = tid % NRP, k = tid / NRP;
      if (k < NK) {
        double sv0 = 0.0, sv1 = 0.0;
        for (int c = s + 1 + k; c < S; c += NK) {
          const ts_d2 *Ut = reinterpret_cast<const ts_d2 *>(A.ufac + (size_t)ts_tile_index(s, c, S) * TS_T) + rp;
          const double *xc = s_sol + (size_t)c * TS_N;
          ts_d2 u[TS_N];
#pragma unroll
          for (int j = 0; j < TS_N; ++j) u[j] = Ut[j * NRP];
#pragma unroll
          for (int j = 0; j < TS_N; ++j) { sv0 = __builtin_fma(u[j].x, xc[j], sv0); sv1 = __builtin_fma(u[j].y, xc[j], sv1); }
        }
        s_part[k * TS_N + 2 * rp] = sv0; s_part[k * TS_N + 2 * rp + 1] = sv1;
      }
      {                                                    // U_ss back from [column][row]
        const ts_d2 *Ud = reinterpret_cast<const ts_d2 *>(A.ufac + (size_t)ts_tile_index(s, s, S) * TS_T);
        for (int e = tid; e < TS_T / 2; e += TS_THREADS) { const ts_d2 v = Ud[e]; const int j = e / NRP, rr = 2 * (e - j * NRP); s_piv[rr * TS_N + j] = v.x; s_piv[(rr + 1) * TS_N + j] = v.y; }
      }
      __syncthreads();
      if (tid < 64) {                                      // U_ss x = rhs, column oriented on the lanes of wave 0 (lane = row)
        const int rr = tid < TS_N ? tid : 0;
        double rhs = A.ybuf[(size_t)s * 2 * TS_N + rr];
        const double rdr = A.ybuf[(size_t)s * 2 * TS_N + TS_N + rr];
#pragma unroll
        for (int kk = 0; kk < NK; ++kk) rhs -= s_part[kk * TS_N + rr];
        double xs = 0.0;
#pragma unroll
        for (int j = TS_N - 1; j >= 0; --j) {
          const double xj = lane_bcast(rhs * rdr, j);
          if (rr == j) xs = xj;
          rhs = __builtin_fma(-s_piv[rr * TS_N + j], xj, rhs);      // (rows below j get zeros of the upper factor: harmless)
        }
        if (tid < TS_N) s_sol[(size_t)s * TS_N + tid] = xs;
      }
      __syncthreads();
    }
  } else {
    for (int i = tid; i < S * TS_N; i += TS_THREADS) s_sol[i] = 0;
    __syncthreads();
  }
  double sc = 0;
  for (int i = tid; i < n; i += TS_THREADS) { const double xv = s_sol[i]; x_out[i] = xv; sc += xv * (B.lambda * xv + B.bp[i]); }
  sc = wave_sum(sc);
  if (lane == 0 && sc != 0.0) atomic_add_f64(&B.scal[2], sc);
  for (int p = tid; p < P; p += TS_THREADS) {
    double Tn[12];
    d_se3_exp_mul(s_sol + 6 * p, B.poses + 12 * (size_t)p, Tn);
    for (int i = 0; i < 12; ++i) B.poses_trial[12 * (size_t)p + i] = Tn[i];
  }
  if (tid == 0) {
    B.scal[3] = (double)fail; B.scal[4] = chi2_cur_sum(B);
    // read as: init, forward, loads, pivot, panel + update (+ publish), arrival wait, backward
    B.scal[5] = (t_loop - t_begin) * 0.01; B.scal[6] = (t_fwd - t_loop) * 0.01; B.scal[8] = acc_t[0] * 0.01; B.scal[9] = acc_t[1] * 0.01; B.scal[10] = (acc_t[2] + acc_t[3]) * 0.01;
    B.scal[11] = acc_t[4] * 0.01; B.scal[7] = ((long long)wall_clock64() - t_fwd) * 0.01;
  }
#undef TS_LAP
}
