// map_edges.inc -- the pose graph's edge table and computeConstraint on the resident map; included by map.hip behind map_csr.inc.
namespace {
// ---- the pose graph's edges (EdgeTable, slam_graph.hpp:197-363): one 408-byte record per slot, 51 eight-byte words -----------------------------------------------
constexpr int EDGE_WORDS = sizeof(svs_map_edge) / 8;
static_assert(sizeof(svs_map_edge) == 408 && sizeof(svs_ba_constraint) == 392 && sizeof(svs_map_constraint_result) == 416, "record copies below");
struct edge_up { int32_t slot, lo, hi, strength, type, pad_; };

// insertEdge: 64 lanes per staged record; T and info zero, not marginalised
__global__ __launch_bounds__(256) void map_edge_add_kernel(svs_map_edge *__restrict__ E, const edge_up *__restrict__ up, int n) {
  const int i = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (i >= n || lane >= EDGE_WORDS) return;
  const edge_up u = up[i];
  int2 w = make_int2(0, 0);
  if (lane == 0) w = make_int2(u.lo, u.hi);
  if (lane == 1) w = make_int2(u.strength, u.type);
  reinterpret_cast<int2 *>(E + u.slot)[lane] = w;
}

// setConstraint with the caller's values: 64 lanes per record.  slot_inv[i] = (slot, T_21 has to be inverted to become T_lo_from_hi)
__global__ __launch_bounds__(256) void map_edge_set_kernel(svs_map_edge *__restrict__ E, const svs_ba_constraint *__restrict__ up, const int2 *__restrict__ slot_inv, int n) {
  const int i = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (i >= n) return;
  const int2 si = slot_inv[i];
  svs_map_edge &e = E[si.x];
  if (lane < 36) e.info[lane] = up[i].info[lane];
  if (lane == 36) {
    double T[12];
#pragma unroll
    for (int k = 0; k < 12; ++k) T[k] = up[i].T_21[k];
    if (si.y) pose_inv(T, T);
#pragma unroll
    for (int k = 0; k < 12; ++k) e.T_lo_from_hi[k] = T[k];
    e.is_marginalized = 1;
  }
}

__global__ __launch_bounds__(256) void map_edge_unmarg_kernel(svs_map_edge *__restrict__ E, const int32_t *__restrict__ slots, int n) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < n) E[slots[i]].is_marginalized = 0;
}

__global__ __launch_bounds__(256) void map_edge_get_kernel(const svs_map_edge *__restrict__ E, const int32_t *__restrict__ slots, int n, svs_map_edge *__restrict__ out) {
  const int i = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (i >= n || lane >= EDGE_WORDS) return;
  reinterpret_cast<long long *>(out + i)[lane] = reinterpret_cast<const long long *>(E + slots[i])[lane];
}

// copyContraintsToG2o's records for the optimizer (ba_map.h): 64 lanes per list entry (i, j, slot, invert)
__global__ __launch_bounds__(256) void map_edge_gather_kernel(const svs_map_edge *__restrict__ E, const int4 *__restrict__ list, int n, svs_ba_constraint *__restrict__ out) {
  const int i = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (i >= n) return;
  const int4 q = list[i];
  const svs_map_edge &e = E[q.z];
  if (lane < 36) out[i].info[lane] = e.info[lane];
  if (lane == 36) {
    double T[12];
#pragma unroll
    for (int k = 0; k < 12; ++k) T[k] = e.T_lo_from_hi[k];
    if (q.w) pose_inv(T, T);
#pragma unroll
    for (int k = 0; k < 12; ++k) out[i].T_21[k] = T[k];
    out[i].pose1 = q.x; out[i].pose2 = q.y;
  }
}

// ---- computeConstraint (slam_graph.cpp:787-846) for a batch of keyframe pairs: one workgroup per request --------------------------------------------------------
// The common points are a bitmap in the request's row of M.mark (kf1's feature_table row is walked, kf2 searched in each point's sorted observer row), turned into
// ascending ids by popcount prefixes; a lane then owns whole points -- record, anchor pose, arithmetic -- and leaves the depth in the request's scratch row.  The
// median is a radix select over the depths' bit patterns (non-negative doubles order as their bits), eight passes of eight bits with LDS histograms that re-read
// the scratch row: both middle ranks are followed at once, nothing is sorted, and the row may be of any length.  No atomic decides a value or an order.
struct cons_req {
  int32_t kf1, kf2, slot, slot_inv;    // slot < 0: do not store; slot_inv: T_12 is the inverse of T_lo_from_hi (kf1 > kf2)
  int32_t n_override, override_id[2], n_cached;
  int32_t cached_off, pad_;            // into the staged cached ids / poses
  long long row_off;                   // into the scratch rows (depths, common point ids)
  double override_T[2][12];
};
static_assert(sizeof(cons_req) % 8 == 0, "staged as an array");
struct MapConsK {
  const cons_req *req; const int32_t *cached_ids; const double *cached_T;
  svs_map_constraint_result *res; int32_t *missing; int missing_cap;
  double *depth; int32_t *common; svs_map_edge *edges;
};
constexpr int CONS_UNROLL = 4;         // points of a lane whose loads are requested together

// the request's pose of keyframe `id`: an override, else the map's
__device__ __forceinline__ const double *cons_pose_of(const MapK &M, const cons_req &Q, int id) {
  if (Q.n_override > 0 && id == Q.override_id[0]) return Q.override_T[0];
  if (Q.n_override > 1 && id == Q.override_id[1]) return Q.override_T[1];
  return M.kf[id].T_anchor_from_w;
}

__global__ __launch_bounds__(MB_THREADS) void map_cons_kernel(MapK M, MapConsK A) {
  __shared__ uint32_t s_miss[MAP_KF_WORDS];
  __shared__ int s_hist[2 * 256];
  __shared__ int s_w[MB_THREADS / 64];
  __shared__ unsigned long long s_pref[2];
  __shared__ int s_rank[2];
  __shared__ double s_T[3][12];                                   // T1, T2, then T_12
  __shared__ double s_diag[2];
  const int r = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const cons_req &Q = A.req[r];
  const int kf1 = Q.kf1, kf2 = Q.kf2;
  uint32_t *mark = M.mark + (size_t)r * M.mark_b;
  double *depth = A.depth + Q.row_off;
  int32_t *common = A.common + Q.row_off;
  const int n_words = (M.pt_hi + 31) >> 5;                        // <= mark_b
  // a. empty sets; the two poses (ids the host has checked: in the map, so below kf_hi <= MAP_MAX_KF)
  s_miss[tid] = 0;
  for (int i = tid; i < n_words; i += MB_THREADS) mark[i] = 0;
  if (tid < 24) s_T[tid / 12][tid % 12] = cons_pose_of(M, Q, tid < 12 ? kf1 : kf2)[tid % 12];
  __syncthreads();
  // b. the common points: CONS_UNROLL entries of kf1's row per lane and step, their row bounds requested together, then the searches
  const int row_b = M.kf_begin[kf1], row_e = M.kf_begin[kf1 + 1];
  for (int e0 = row_b; e0 < row_e; e0 += MB_THREADS * CONS_UNROLL) {      // block-uniform
    int p[CONS_UNROLL], ob[CONS_UNROLL], oe[CONS_UNROLL];
#pragma unroll
    for (int k = 0; k < CONS_UNROLL; ++k) { const int e = e0 + k * MB_THREADS + tid; p[k] = e < row_e ? M.kf_rows[e] : -1; }
#pragma unroll
    for (int k = 0; k < CONS_UNROLL; ++k) {
      const bool have = (unsigned)p[k] < (unsigned)M.pt_hi;
      ob[k] = have ? M.pt_begin[p[k]] : 0; oe[k] = have ? M.pt_begin[p[k] + 1] : 0;
    }
#pragma unroll
    for (int k = 0; k < CONS_UNROLL; ++k) {
      wave_or_by_word(mark, p[k] >> 5, 1u << (p[k] & 31), row_has(M.pt_rows, ob[k], oe[k], kf2));
    }
  }
  __syncthreads();
  // c. ascending ids (the capacity always holds: the common points are entries of kf1's row)
  const int n = min(list_marked(mark, n_words, common, 0, row_e - row_b, s_w), row_e - row_b);
  __syncthreads();
  // d. the depths: record, anchor, pose source and pose of CONS_UNROLL points requested before their arithmetic
  for (int i0 = 0; i0 < n; i0 += MB_THREADS * CONS_UNROLL) {
    int a[CONS_UNROLL];
    double x[CONS_UNROLL][3];
    const double *Ta[CONS_UNROLL];
#pragma unroll
    for (int k = 0; k < CONS_UNROLL; ++k) {
      const int i = i0 + k * MB_THREADS + tid;
      a[k] = -1;
      if (i < n) {
        const svs_candidate_point &q = M.pt[common[i]];
        x[k][0] = q.xyz_anchor[0]; x[k][1] = q.xyz_anchor[1]; x[k][2] = q.xyz_anchor[2];
        a[k] = q.kf_index;
      }
    }
#pragma unroll
    for (int k = 0; k < CONS_UNROLL; ++k) {
      Ta[k] = nullptr;
      if ((unsigned)a[k] >= (unsigned)MAP_MAX_KF) continue;
      if ((Q.n_override > 0 && a[k] == Q.override_id[0]) || (Q.n_override > 1 && a[k] == Q.override_id[1]) || (M.kf_flags[a[k]] & SVS_REG_KF_IN_WINDOW)) {
        Ta[k] = cons_pose_of(M, Q, a[k]);
      } else {
        int lo = 0, hi = Q.n_cached;                               // the cached list is ascending
        const int32_t *ids = A.cached_ids + Q.cached_off;
        while (lo < hi) { const int mid = (lo + hi) >> 1; if (ids[mid] < a[k]) lo = mid + 1; else hi = mid; }
        if (lo < Q.n_cached && ids[lo] == a[k]) Ta[k] = A.cached_T + 12 * (size_t)(Q.cached_off + lo);
        else bit_set(s_miss, a[k]);
      }
    }
#pragma unroll
    for (int k = 0; k < CONS_UNROLL; ++k) {
      const int i = i0 + k * MB_THREADS + tid;
      if (i >= n) continue;
      double d = 0.0;
      if (Ta[k]) {
        double T[12], y[3], z[3];
#pragma unroll
        for (int q = 0; q < 12; ++q) T[q] = Ta[k][q];
        pose_inv(T, T);
        pose_act(T, x[k], y);
        pose_act(s_T[0], y, z);
        d = sqrt((z[0] * z[0] + z[1] * z[1]) + z[2] * z[2]);
      }
      depth[i] = d;
    }
  }
  // e. T_12 = T1 * inv(T2); the missing anchors, ascending
  if (tid == 0) {
    double Ti[12], T12[12];
    pose_inv(s_T[1], Ti);
    pose_mul(s_T[0], Ti, T12);
#pragma unroll
    for (int k = 0; k < 12; ++k) s_T[2][k] = T12[k];
  }
  __syncthreads();                                                 // (completes s_miss, the scratch row and s_T[2])
  svs_map_constraint_result &R = A.res[r];
  int32_t *missing = A.missing + (size_t)r * A.missing_cap;
  const int n_missing = list_words(s_miss[tid], tid << 5, 0, s_w, [&](int id, int pos) { if (pos < A.missing_cap) missing[pos] = id; });
  for (int k = n_missing + tid; k < A.missing_cap; k += MB_THREADS) missing[k] = -1;
  if (tid < 12) R.T_12[tid] = s_T[2][tid];
  if (n_missing > 0 || n == 0) {                                   // block-uniform
    if (tid < 36) R.info[tid] = 0.0;
    if (tid == 0) { R.status = n_missing > 0 ? SVS_CONS_MISSING_ANCHOR : SVS_CONS_EMPTY; R.strength = n; R.n_missing = n_missing; R.pad_ = 0; R.median = 0.0; R.norm_dist = 0.0; }
    return;
  }
  // f. the median (maths_utils.h:114-136): ranks (n - 1) / 2 and n / 2 of the multiset, one and the same for an odd count
  if (tid < 2) { s_pref[tid] = 0ull; s_rank[tid] = tid == 0 ? (n - 1) / 2 : n / 2; }
  __syncthreads();
  for (int shift = 56; shift >= 0; shift -= 8) {
    const unsigned long long pref0 = s_pref[0], pref1 = s_pref[1];
    const int my = tid >> 8, bin = tid & 255, rank = s_rank[my];
    s_hist[tid] = 0;
    __syncthreads();
    for (int i = tid; i < n; i += MB_THREADS) {
      const unsigned long long u = (unsigned long long)__double_as_longlong(depth[i]);
      const unsigned long long hi = shift == 56 ? 0ull : u >> (shift + 8);
      const int b = (int)(u >> shift) & 255;
      if (hi == pref0) atomicAdd(&s_hist[b], 1);
      if (hi == pref1) atomicAdd(&s_hist[256 + b], 1);
    }
    __syncthreads();
    // the prefix of each half's 256 bins over its own four waves, behind ONE barrier: block_excl_scan would sum over all eight waves and add a barrier per pass
    const int v = s_hist[tid];
    const int inc = wave_incl_scan(v);
    if (lane == 63) s_w[wave] = inc;
    __syncthreads();
    int off = 0;
#pragma unroll
    for (int w = 0; w < MB_THREADS / 64; ++w) off += ((w >> 2) == my && w < wave) ? s_w[w] : 0;
    const int excl = off + inc - v;
    if (v > 0 && excl <= rank && rank < excl + v) {                // exactly one bin per rank
      s_pref[my] = ((my == 0 ? pref0 : pref1) << 8) | (unsigned long long)bin;
      s_rank[my] = rank - excl;
    }
    __syncthreads();
  }
  // g. norm_dist, Lambda; the record, and setConstraint where the request stores
  if (tid == 0) {
    const double lo = __longlong_as_double((long long)s_pref[0]), hi = __longlong_as_double((long long)s_pref[1]);
    double val = lo;
    if ((n & 1) == 0) { val += hi; val = 0.5 * val; }
    const double tx = s_T[2][3], ty = s_T[2][7], tz = s_T[2][11];
    const double norm_dist = sqrt((tx * tx + ty * ty) + tz * tz) / val;
    const double s = (double)n, v350 = (350 * 1.0) * norm_dist, v100 = 100 * 1.0;
    s_diag[0] = s * (v350 * v350); s_diag[1] = s * (v100 * v100);
    R.status = SVS_CONS_OK; R.strength = n; R.n_missing = 0; R.pad_ = 0; R.median = val; R.norm_dist = norm_dist;
  }
  __syncthreads();
  const double lam = tid < 36 ? (tid % 7 == 0 ? s_diag[tid >= 21 ? 1 : 0] : 0.0) : 0.0;
  if (tid < 36) R.info[tid] = lam;
  if (Q.slot >= 0) {
    svs_map_edge &E = A.edges[Q.slot];
    if (tid < 36) E.info[tid] = lam;
    if (tid == 36) {
      double T[12];
#pragma unroll
      for (int k = 0; k < 12; ++k) T[k] = s_T[2][k];
      if (Q.slot_inv) pose_inv(T, T);
#pragma unroll
      for (int k = 0; k < 12; ++k) E.T_lo_from_hi[k] = T[k];
      E.is_marginalized = 1;
    }
  }
}
}  // namespace

// ---- the pose graph's edges ---------------------------------------------------------------------------------------------------------------------------------
static uint64_t edge_key(int a, int b) { return ((uint64_t)(uint32_t)std::min(a, b) << 32) | (uint32_t)std::max(a, b); }

// the slots of n named edges (either orientation): every edge exists; `distinct`: none twice
static int map_edge_slots(svs_map *m, int n, const int32_t *a, const int32_t *b, int stride, bool distinct, std::vector<int32_t> *slots) {
  svs_ctx *ctx = m->ctx;
  std::unordered_set<int> seen;
  slots->resize((size_t)n);
  for (int i = 0; i < n; ++i) {
    const int x = a[(size_t)i * stride], y = b[(size_t)i * stride];
    SVS_REQUIRE(ctx, x != y && svs_map_has_keyframe(m, x) && svs_map_has_keyframe(m, y));
    const auto it = m->edge_slot.find(edge_key(x, y));
    SVS_REQUIRE(ctx, it != m->edge_slot.end());
    SVS_REQUIRE(ctx, !distinct || seen.insert(it->second).second);
    (*slots)[i] = it->second;
  }
  return SVS_OK;
}

extern "C" int svs_map_reserve_edges(svs_map *m, int max_edges) {
  svs_ctx *ctx = m ? m->ctx : nullptr;
  SVS_REQUIRE(ctx, m && max_edges >= 1 && max_edges < (1 << 24) && m->max_edges == 0);
  SVS_DEVICE(ctx);
  SVS_HIP(ctx, m->d_edges.alloc((size_t)max_edges));
  m->edge_marg.assign((size_t)max_edges, 0);
  m->max_edges = max_edges;
  return SVS_OK;
}

extern "C" int svs_map_add_edges(svs_map *m, int n, const int32_t *h_pairs, const int32_t *h_strength, const int32_t *h_type) {
  svs_ctx *ctx = m ? m->ctx : nullptr;
  SVS_REQUIRE(ctx, m && n >= 0 && (n == 0 || (h_pairs && h_strength && h_type)));
  MAP_CAPACITY(ctx, (size_t)m->n_edges + (size_t)n <= (size_t)m->max_edges);
  if (n == 0) return SVS_OK;
  std::unordered_set<uint64_t> seen;
  for (int i = 0; i < n; ++i) {
    const int a = h_pairs[2 * i], b = h_pairs[2 * i + 1];
    SVS_REQUIRE(ctx, a != b && svs_map_has_keyframe(m, a) && svs_map_has_keyframe(m, b) && h_type[i] >= 0 && h_type[i] <= 2);
    SVS_REQUIRE(ctx, !m->edge_slot.count(edge_key(a, b)) && seen.insert(edge_key(a, b)).second);
  }
  SVS_DEVICE(ctx);
  MapUp up(m);
  const auto recs = up.piece<edge_up>(n);
  if (int rc = up.reserve()) return rc;
  edge_up *u = up.host(recs);
  for (int i = 0; i < n; ++i) {
    const int a = h_pairs[2 * i], b = h_pairs[2 * i + 1];
    u[i].slot = m->n_edges + i; u[i].lo = std::min(a, b); u[i].hi = std::max(a, b); u[i].strength = h_strength[i]; u[i].type = h_type[i]; u[i].pad_ = 0;
  }
  if (int rc = up.upload()) return rc;
  hipLaunchKernelGGL(map_edge_add_kernel, dim3(div_up(n, 4)), dim3(256), 0, ctx->stream, m->d_edges.get(), up.dev(recs), n);
  SVS_LAUNCH_CHECK(ctx);
  for (int i = 0; i < n; ++i) { m->edge_slot[edge_key(h_pairs[2 * i], h_pairs[2 * i + 1])] = m->n_edges + i; m->edge_marg[(size_t)m->n_edges + i] = 0; }
  m->n_edges += n;
  return SVS_OK;
}

extern "C" int svs_map_set_constraints(svs_map *m, int n, const svs_ba_constraint *h_cons) {
  svs_ctx *ctx = m ? m->ctx : nullptr;
  SVS_REQUIRE(ctx, m && n >= 0 && (n == 0 || h_cons));
  MAP_CAPACITY(ctx, n == 0 || m->max_edges > 0);
  if (n == 0) return SVS_OK;
  std::vector<int32_t> slots;
  if (int rc = map_edge_slots(m, n, &h_cons[0].pose1, &h_cons[0].pose2, (int)(sizeof(svs_ba_constraint) / sizeof(int32_t)), true, &slots)) return rc;
  SVS_DEVICE(ctx);
  MapUp up(m);
  const auto cons = up.piece<svs_ba_constraint>(n);
  const auto slot_inv = up.piece<int2>(n);
  if (int rc = up.reserve()) return rc;
  up.put(cons, h_cons);
  // T_21 = T_pose2_from_pose1: T_lo_from_hi as it stands where pose2 is the smaller id, its inverse otherwise (slam_graph.hpp:327)
  for (int i = 0; i < n; ++i) up.host(slot_inv)[i] = make_int2(slots[i], h_cons[i].pose1 < h_cons[i].pose2 ? 1 : 0);
  if (int rc = up.upload()) return rc;
  hipLaunchKernelGGL(map_edge_set_kernel, dim3(div_up(n, 4)), dim3(256), 0, ctx->stream, m->d_edges.get(), up.dev(cons), up.dev(slot_inv), n);
  SVS_LAUNCH_CHECK(ctx);
  for (int s : slots) { m->n_marg += m->edge_marg[s] ? 0 : 1; m->edge_marg[s] = 1; }
  return SVS_OK;
}

extern "C" int svs_map_unmarginalize(svs_map *m, int n, const int32_t *h_pairs) {
  svs_ctx *ctx = m ? m->ctx : nullptr;
  SVS_REQUIRE(ctx, m && n >= 0 && (n == 0 || h_pairs));
  MAP_CAPACITY(ctx, n == 0 || m->max_edges > 0);
  if (n == 0) return SVS_OK;
  std::vector<int32_t> slots;
  if (int rc = map_edge_slots(m, n, h_pairs, h_pairs + 1, 2, true, &slots)) return rc;
  SVS_DEVICE(ctx);
  MapUp up(m);
  const auto p_slots = up.piece<int32_t>(n);
  if (int rc = up.reserve()) return rc;
  up.put(p_slots, slots.data());
  if (int rc = up.upload()) return rc;
  hipLaunchKernelGGL(map_edge_unmarg_kernel, dim3(div_up(n, 256)), dim3(256), 0, ctx->stream, m->d_edges.get(), up.dev(p_slots), n);
  SVS_LAUNCH_CHECK(ctx);
  for (int s : slots) { m->n_marg -= m->edge_marg[s] ? 1 : 0; m->edge_marg[s] = 0; }
  return SVS_OK;
}

extern "C" int svs_map_get_edges(svs_map *m, int n, const int32_t *h_pairs, svs_map_edge *h_out) {
  svs_ctx *ctx = m ? m->ctx : nullptr;
  SVS_REQUIRE(ctx, m && n >= 0 && (n == 0 || (h_pairs && h_out)));
  MAP_CAPACITY(ctx, n == 0 || m->max_edges > 0);
  if (n == 0) return SVS_OK;
  std::vector<int32_t> slots;
  if (int rc = map_edge_slots(m, n, h_pairs, h_pairs + 1, 2, false, &slots)) return rc;
  return map_read_back(m, n, slots.data(), 1, h_out, [&](const int32_t *d_slots, svs_map_edge *out) {
    hipLaunchKernelGGL(map_edge_get_kernel, dim3(div_up(n, 4)), dim3(256), 0, ctx->stream, m->d_edges.get(), d_slots, n, out);
  });
}

extern "C" int svs_map_edge_info(svs_map *map, int32_t *n_edges, int32_t *n_marginalized) {
  if (!map) return SVS_ERR_INVALID;
  if (n_edges) *n_edges = map->n_edges;
  if (n_marginalized) *n_marginalized = map->n_marg;
  return SVS_OK;
}

int svs_map_window_constraint_list(svs_map *m, std::vector<int4> *out) {
  svs_ctx *ctx = m->ctx;
  SVS_REQUIRE(ctx, m->win_valid);
  out->clear();
  const int P = m->win_P;
  for (int i = 0; i < P; ++i)
    for (int j = 0; j < P; ++j) {
      if (j == i || (m->win_types[i] != 1 && m->win_types[j] != 1)) continue;
      const int a = m->win_ids[i], b = m->win_ids[j];
      const auto it = m->edge_slot.find(edge_key(a, b));
      if (it == m->edge_slot.end()) continue;
      if (!m->edge_marg[it->second]) { ctx->err = "svs_ba_window_from_map_edges: an edge with an OUTER end is not marginalised (slam_graph.cpp:972)"; return SVS_ERR_INVALID; }
      out->push_back(make_int4(i, j, it->second, a < b ? 1 : 0));      // T_21 = T_j_from_i: the stored T_lo_from_hi where id_j is the smaller
    }
  return SVS_OK;
}

int svs_map_gather_constraints(svs_map *m, const int4 *d_list, int C, svs_ba_constraint *d_out) {
  svs_ctx *ctx = m->ctx;
  SVS_REQUIRE(ctx, C >= 1 && m->max_edges > 0 && d_list && d_out);
  hipLaunchKernelGGL(map_edge_gather_kernel, dim3(div_up(C, 4)), dim3(256), 0, ctx->stream, m->d_edges.get(), d_list, C, d_out);
  SVS_LAUNCH_CHECK(ctx);
  return SVS_OK;
}

extern "C" int svs_map_compute_constraints(svs_map *m, int n, const svs_map_constraint_request *req, int missing_cap, svs_map_constraint_result *h_res,
                                           int32_t *h_missing, int depth_cap, double *h_depths) {
  svs_ctx *ctx = m ? m->ctx : nullptr;
  SVS_REQUIRE(ctx, m && n >= 0 && (n == 0 || (req && h_res)) && missing_cap >= 0 && (missing_cap == 0 || h_missing) && depth_cap >= 0 && (depth_cap == 0 || h_depths));
  if (n == 0) return SVS_OK;
  MAP_CAPACITY(ctx, n <= SVS_MAP_CONS_MAX_REQUESTS);
  // ---- every refusal: before anything is uploaded -------------------------------------------------------------------------------------------------------
  size_t n_cached = 0, n_rows = 0;
  std::vector<int32_t> slot((size_t)n, -1);
  {
    std::unordered_set<int> storing;
    for (int i = 0; i < n; ++i) {
      const svs_map_constraint_request &q = req[i];
      SVS_REQUIRE(ctx, q.kf1 != q.kf2 && svs_map_has_keyframe(m, q.kf1) && svs_map_has_keyframe(m, q.kf2));
      SVS_REQUIRE(ctx, q.n_override >= 0 && q.n_override <= 2 && q.n_cached >= 0 && (q.n_cached == 0 || (q.cached_ids && q.cached_T)));
      for (int k = 0; k < q.n_override; ++k) SVS_REQUIRE(ctx, q.override_id[k] >= 0 && q.override_id[k] < m->max_kf);
      SVS_REQUIRE(ctx, q.n_override < 2 || q.override_id[0] != q.override_id[1]);
      MAP_CAPACITY(ctx, q.n_cached <= m->max_kf);
      for (int k = 0; k < q.n_cached; ++k) SVS_REQUIRE(ctx, q.cached_ids[k] >= 0 && q.cached_ids[k] < m->max_kf && (k == 0 || q.cached_ids[k - 1] < q.cached_ids[k]));
      if (h_depths) MAP_CAPACITY(ctx, m->kf_nobs[q.kf1] <= depth_cap);
      if (q.store) {
        MAP_CAPACITY(ctx, m->max_edges > 0);
        const auto it = m->edge_slot.find(edge_key(q.kf1, q.kf2));
        SVS_REQUIRE(ctx, it != m->edge_slot.end());
        SVS_REQUIRE(ctx, storing.insert(it->second).second);
        slot[i] = it->second;
      }
      n_cached += (size_t)q.n_cached; n_rows += (size_t)m->kf_nobs[q.kf1];
    }
  }
  SVS_DEVICE(ctx);
  // ---- room: the scratch rows, the download block, a bitmap row per request, current CSR views ----------------------------------------------------------------
  if (m->d_depth.bytes() < std::max<size_t>(n_rows, 1) * sizeof(double)) {
    SVS_HIP(ctx, hipStreamSynchronize(ctx->stream));
    const size_t want = std::max<size_t>(n_rows * 2, 4096);
    SVS_HIP(ctx, m->d_depth.alloc(want));
    SVS_HIP(ctx, m->d_common.alloc(want));
  }
  MapDn dn(m);
  const auto res = dn.piece<svs_map_constraint_result>(n);
  const auto missing = dn.piece<int32_t>((size_t)n * missing_cap);
  const auto depths = dn.piece<double>(h_depths ? n_rows : 0);
  if (int rc = dn.reserve()) return rc;
  if (int rc = map_prepare_walk(m, n)) return rc;
  // ---- one staged upload: the requests | cached ids | cached poses -------------------------------------------------------------------------------------------
  MapUp up(m);
  const auto reqs = up.piece<cons_req>(n);
  const auto cached_ids = up.piece<int32_t>(n_cached);
  const auto cached_T = up.piece<double>(12 * n_cached);
  if (int rc = up.reserve()) return rc;
  {
    int32_t *ids = up.host(cached_ids);
    double *T = up.host(cached_T);
    size_t c = 0, row = 0;
    for (int i = 0; i < n; ++i) {
      const svs_map_constraint_request &q = req[i];
      cons_req u{};
      u.kf1 = q.kf1; u.kf2 = q.kf2; u.slot = slot[i]; u.slot_inv = q.kf1 > q.kf2 ? 1 : 0;
      u.n_override = q.n_override; u.n_cached = q.n_cached; u.cached_off = (int32_t)c; u.row_off = (long long)row;
      for (int k = 0; k < q.n_override; ++k) { u.override_id[k] = q.override_id[k]; memcpy(u.override_T[k], q.override_T[k], sizeof u.override_T[k]); }
      up.host(reqs)[i] = u;
      if (q.n_cached) { memcpy(ids + c, q.cached_ids, (size_t)q.n_cached * sizeof(int32_t)); memcpy(T + 12 * c, q.cached_T, (size_t)q.n_cached * 12 * sizeof(double)); }
      c += (size_t)q.n_cached; row += (size_t)m->kf_nobs[q.kf1];
    }
  }
  if (int rc = up.upload()) return rc;
  MapConsK A{};
  A.req = up.dev(reqs); A.cached_ids = up.dev(cached_ids); A.cached_T = up.dev(cached_T);
  A.res = dn.dev(res); A.missing = dn.dev(missing); A.missing_cap = missing_cap;
  A.depth = m->d_depth; A.common = m->d_common; A.edges = m->d_edges;
  hipLaunchKernelGGL(map_cons_kernel, dim3(n), dim3(MB_THREADS), 0, ctx->stream, m->view(), A);
  SVS_LAUNCH_CHECK(ctx);
  if (depths.n) SVS_HIP(ctx, hipMemcpyAsync(dn.dev(depths), m->d_depth, depths.bytes(), hipMemcpyDeviceToDevice, ctx->stream));
  if (int rc = dn.download()) return rc;
  dn.get(res, h_res);
  dn.get(missing, h_missing);
  size_t row = 0;
  for (int i = 0; i < n; ++i) {
    if (h_depths) {
      double *d = h_depths + (size_t)i * depth_cap;
      const int k = h_res[i].status == SVS_CONS_OK ? h_res[i].strength : 0;
      memcpy(d, dn.host(depths) + row, (size_t)k * sizeof(double));
      std::fill(d + k, d + depth_cap, 0.0);
    }
    row += (size_t)m->kf_nobs[req[i].kf1];
    if (slot[i] >= 0 && h_res[i].status == SVS_CONS_OK) { m->n_marg += m->edge_marg[slot[i]] ? 0 : 1; m->edge_marg[slot[i]] = 1; }
  }
  return SVS_OK;
}
