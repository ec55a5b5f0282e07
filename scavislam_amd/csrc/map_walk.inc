// map_walk.inc -- the pose graph's breadth-first walks on the device-resident map (included by map.hip behind map_edges.inc): computeInitialDoubleWin
// (slam_graph.cpp:555-596), framesInNeighborhood (:105-140), shortestPathToWindow + computeAbsolutePose (:64-103, :762-782) and reinitializePoses (:665-725).
//   walk_adj_*        the strength-ordered adjacency: a CSR over keyframe ids built from the edge records -- count, scan, fill, then a rank sort of every row by
//                     descending (strength, edge slot).  The reference pushes a vertex's neighbours in neighbor_ids_ordered_by_strength.rbegin() .. rend() order;
//                     every insertion into that multimap is paired with an insertEdge of the same strength (:222-227, :442-447), the strength is never updated and
//                     a multimap keeps equal keys in insertion order, so the reverse walk is the row of edges in descending (strength, slot)
//   map_walk_kernel   one workgroup per request, level-synchronous.  The reference drops duplicates at pop; with a FIFO queue the order of first pops is the order
//                     of first pushes and the processed copy is the first pusher's, so the visit order is "frontier in order, each frontier vertex's row in order,
//                     first claim wins": an unclaimed neighbour takes atomicMin(((visit index of the claimer + 1) << 14) | rank in its row), a minimum that no
//                     arrival order changes; the winners of a row are counted, the counts prefixed over the level, and every winner lands at prefix + its rank among
//                     the row's winners.  Visit indices grow over the whole walk, so a key once won is never beaten and doubles as the visited mark
// Poses are chained with pose.h in f64 without contraction, one lane per chain or per keyframe of a level, in the order map_cons_kernel uses.
namespace {
constexpr int WALK_RANK_BITS = 14;
static_assert(MAP_MAX_KF <= (1 << WALK_RANK_BITS) && MAP_MAX_KF < (1 << (31 - WALK_RANK_BITS)), "a claim is (visit index + 1, rank in row) in 32 bits");
constexpr int WALK_INF = 0x7fffffff;

struct WalkAdjK {
  int32_t *begin, *cur, *nb, *slot, *tmp_nb; unsigned long long *tmp_key;
  const svs_map_edge *edges; int n_edges, kf_hi;
};

__global__ __launch_bounds__(256) void walk_adj_count_kernel(WalkAdjK A) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= A.n_edges) return;
  atomicAdd(&A.begin[A.edges[e].lo], 1);      // (ids the host has checked: below kf_hi)
  atomicAdd(&A.begin[A.edges[e].hi], 1);
}

// one workgroup (a keyframe has a handful of edges: one entry per lane and step)
__global__ __launch_bounds__(MB_THREADS) void walk_adj_scan_kernel(WalkAdjK A) {
  __shared__ int s_w[MB_THREADS / 64];
  counts_to_begin<1>(A.begin, A.cur, A.kf_hi, s_w);
}

// the position inside a row is whatever the atomics give: the sort below puts every entry at its rank
__global__ __launch_bounds__(256) void walk_adj_fill_kernel(WalkAdjK A) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= A.n_edges) return;
  const svs_map_edge &E = A.edges[e];
  const int lo = E.lo, hi = E.hi;
  const unsigned long long key = ((unsigned long long)((uint32_t)E.strength ^ 0x80000000u) << 32) | (uint32_t)e;      // orders as (strength, slot)
  const int a = atomicAdd(&A.cur[lo], 1), b = atomicAdd(&A.cur[hi], 1);      // < begin of the next row <= 2 n_edges
  A.tmp_key[a] = key; A.tmp_nb[a] = hi;
  A.tmp_key[b] = key; A.tmp_nb[b] = lo;
}

// one wave per row: an entry's place is the number of entries of its row with a greater key (the keys of a row are distinct: a slot is in a row once).  Any
// row length; the work is quadratic in it
__global__ __launch_bounds__(256) void walk_adj_sort_kernel(WalkAdjK A) {
  const int v = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (v >= A.kf_hi) return;
  const int b = A.begin[v], e = A.begin[v + 1];
  for (int k = b + lane; k < e; k += 64) {
    const unsigned long long mine = A.tmp_key[k];
    int rank = 0;
    for (int j = b; j < e; ++j) rank += A.tmp_key[j] > mine ? 1 : 0;
    A.nb[b + rank] = A.tmp_nb[k];
    A.slot[b + rank] = (int32_t)(uint32_t)mine;
  }
}

struct MapWalkK {
  const int32_t *begin, *nb, *slot; const svs_map_edge *edges;
  const int32_t *roots;                // [requests]
  int mode, limit, inner, out_cap;     // limit: double_size / size_of_neighborhood; out_cap: row length of out_ids (path_cap with WALK_ABSOLUTE)
  int loop_id, n_old; const int32_t *old_ids;      // WALK_REINIT
  int32_t *work; int stride;
  int4 *hdr;                           // [requests]: WINDOW / NEIGHBORHOOD (count, pairs, INNER, 0); ABSOLUTE (status, path length, 0, 0); REINIT (changed, visited, 0, 0)
  double *T;                           // [requests][12], WALK_ABSOLUTE
  int32_t *out_ids, *out_type;         // [requests][out_cap]
  int32_t *win; int win_cap;           // svs_map_prepare_window_from_root: ids [win_cap] | types [win_cap] | INNER ids [win_cap] | pairs
};

__device__ __forceinline__ uint32_t walk_claim(int visit, int rank) { return ((uint32_t)(visit + 1) << WALK_RANK_BITS) | (uint32_t)rank; }

// T_1_from_2 of getRelativePose_1_from_2 (:271-286) across edge E with the poses the map holds now
__device__ __forceinline__ void walk_rel(const MapK &M, const svs_map_edge &E, int id1, int id2, double *R) {
  if (E.is_marginalized) {
#pragma unroll
    for (int k = 0; k < 12; ++k) R[k] = E.T_lo_from_hi[k];
    if (id1 != E.lo) pose_inv(R, R);
  } else {
    double T1[12], T2[12];
#pragma unroll
    for (int k = 0; k < 12; ++k) { T1[k] = M.kf[id1].T_anchor_from_w[k]; T2[k] = M.kf[id2].T_anchor_from_w[k]; }
    pose_inv(T2, T2);
    pose_mul(T1, T2, R);
  }
}

// one search by the whole workgroup: request r (the row of every output) from `root` in work space `work_row`.  The kernels below call it; a workgroup that
// calls it again puts a barrier between the calls
__device__ __forceinline__ void map_walk_search(const MapK &M, const MapWalkK &W, int r, int root, int work_row, int *s_w, uint32_t *s_old, int &s_first) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, mode = W.mode;
  int32_t *work = W.work + (size_t)work_row * WALK_ROWS * W.stride;      // stride >= kf_hi
  uint32_t *key = reinterpret_cast<uint32_t *>(work + (size_t)WALK_ROW_KEY * W.stride);
  int32_t *order = work + (size_t)WALK_ROW_ORDER * W.stride, *parent = work + (size_t)WALK_ROW_PARENT * W.stride, *pedge = work + (size_t)WALK_ROW_PEDGE * W.stride,
          *cnt = work + (size_t)WALK_ROW_CNT * W.stride, *flag = work + (size_t)WALK_ROW_FLAG * W.stride;
  const bool restricted = mode == WALK_NEIGHBORHOOD || mode == WALK_REINIT;      // keyframes outside the window are skipped and not expanded (:124, :690)
  // a. nothing claimed; the old window
  for (int i = tid; i < M.kf_hi; i += MB_THREADS) __hip_atomic_store(&key[i], 0xffffffffu, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  s_old[tid] = 0;
  if (tid == 0) s_first = WALK_INF;
  __syncthreads();
  if (mode == WALK_REINIT)
    for (int i = tid; i < W.n_old; i += MB_THREADS) bit_set(s_old, W.old_ids[i]);
  const bool root_in = (M.kf_flags[root] & SVS_REG_KF_IN_WINDOW) != 0;
  int n = 0, target = -1, depth = 0;                              // visited so far; WALK_ABSOLUTE: the visit index the path ends at, and its level
  if (!restricted || root_in) {
    if (tid == 0) {
      __hip_atomic_store(&key[root], 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      order[0] = root; parent[root] = -1; pedge[root] = -1; flag[root] = root == W.loop_id ? 1 : 0;
    }
    n = 1;
    if (mode == WALK_ABSOLUTE && root_in) target = 0;             // a window vertex is recognised before it would be expanded (:79)
  }
  __syncthreads();
  // b. level by level
  int lvl_b = 0;
  while (lvl_b < n && n < W.limit && target < 0) {                // block-uniform
    const int lvl_e = n, m = lvl_e - lvl_b;
    // claims: a wave per frontier vertex, its lanes along the row
    for (int i = lvl_b + wave; i < lvl_e; i += MB_THREADS / 64) {
      const int f = order[i], b = W.begin[f], e = W.begin[f + 1];
      for (int k = b + lane; k < e; k += 64) {
        const int u = W.nb[k];
        if (restricted && !(M.kf_flags[u] & SVS_REG_KF_IN_WINDOW)) continue;
        atomicMin(&key[u], walk_claim(i, k - b));
      }
    }
    __syncthreads();
    // the winners of every row
    for (int i = lvl_b + wave; i < lvl_e; i += MB_THREADS / 64) {
      const int f = order[i], b = W.begin[f], e = W.begin[f + 1];
      int c = 0;
      for (int k0 = b; k0 < e; k0 += 64) {                         // wave-uniform
        const int k = k0 + lane;
        const bool win = k < e && __hip_atomic_load(&key[W.nb[k]], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == walk_claim(i, k - b);
        c += __popcll(__ballot(win));
      }
      if (lane == 0) cnt[i - lvl_b] = c;
    }
    __syncthreads();
    int run = 0;
    for (int base = 0; base < m; base += MB_THREADS) {            // block-uniform
      const int idx = base + tid;
      const int v = idx < m ? cnt[idx] : 0;
      int tot;
      const int off = run + block_excl_scan(v, s_w, tot);
      if (idx < m) cnt[idx] = off;
      run += tot;
    }
    __syncthreads();
    // the next level in visit order (lvl_e + run <= kf_hi: a keyframe wins once)
    for (int i = lvl_b + wave; i < lvl_e; i += MB_THREADS / 64) {
      const int f = order[i], b = W.begin[f], e = W.begin[f + 1];
      int pos = lvl_e + cnt[i - lvl_b];
      for (int k0 = b; k0 < e; k0 += 64) {
        const int k = k0 + lane;
        const int u = k < e ? W.nb[k] : -1;
        const bool win = k < e && __hip_atomic_load(&key[u], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == walk_claim(i, k - b);
        const unsigned long long mask = __ballot(win);
        if (win) {
          const int p = pos + __popcll(mask & ((1ull << lane) - 1ull));
          order[p] = u; parent[u] = f; pedge[u] = W.slot[k];
        }
        pos += __popcll(mask);
      }
    }
    n = lvl_e + run; lvl_b = lvl_e; ++depth;
    __syncthreads();
    if (mode == WALK_ABSOLUTE) {                                   // the first window vertex of the level, if any
      int best = WALK_INF;
      for (int p = lvl_e + tid; p < n; p += MB_THREADS)
        if (M.kf_flags[order[p]] & SVS_REG_KF_IN_WINDOW) { best = p; break; }
      if (best != WALK_INF) atomicMin(&s_first, best);
      __syncthreads();
      if (s_first != WALK_INF) target = s_first;
    }
    if (mode == WALK_REINIT) {                                     // a lane per keyframe of the level: its parent's pose is final (:699-712)
      for (int p = lvl_e + tid; p < n; p += MB_THREADS) {
        const int v = order[p], par = parent[v];
        const int mark = ((flag[par] & 1) || v == W.loop_id) ? 1 : 0;
        int changed = 0;
        if (mark || !bit_of(s_old, v)) {
          double R[12], Tp[12];
          walk_rel(M, W.edges[pedge[v]], v, par, R);
#pragma unroll
          for (int k = 0; k < 12; ++k) Tp[k] = M.kf[par].T_anchor_from_w[k];
          pose_mul(R, Tp, R);
#pragma unroll
          for (int k = 0; k < 12; ++k) M.kf[v].T_anchor_from_w[k] = R[k];
          changed = 2;
        }
        flag[v] = mark | changed;
      }
      __syncthreads();
    }
  }
  // c. the outputs
  if (mode == WALK_WINDOW || mode == WALK_NEIGHBORHOOD) {
    const int count = min(n, W.limit), n_inner = min(count, W.inner);
    for (int i = tid; i < W.out_cap; i += MB_THREADS) {
      W.out_ids[(size_t)r * W.out_cap + i] = i < count ? order[i] : -1;
      if (W.out_type) W.out_type[(size_t)r * W.out_cap + i] = i < count ? (i < W.inner ? 0 : 1) : -1;
    }
    int n_pairs = 0;
    if (W.win) {                                                   // one request, count <= win_cap <= MB_THREADS: what svs_map_prepare_window is given
      int32_t *ids = W.win, *types = ids + W.win_cap, *inner = types + W.win_cap, *pairs = inner + W.win_cap;
      if (tid < count) { ids[tid] = order[tid]; types[tid] = tid < W.inner ? 0 : 1; }
      if (tid < n_inner) inner[tid] = order[tid];
      const int deg = tid < n_inner ? W.begin[order[tid] + 1] - W.begin[order[tid]] : 0;
      const int off = block_excl_scan(deg, s_w, n_pairs);
      if (tid < n_inner) cnt[tid] = off;
      __syncthreads();
      for (int i = wave; i < n_inner; i += MB_THREADS / 64) {      // the adjacency rows of the INNER keyframes: every edge with an end in one of them
        const int f = order[i], b = W.begin[f], e = W.begin[f + 1];
        for (int k = b + lane; k < e; k += 64) { pairs[2 * (size_t)(cnt[i] + k - b)] = f; pairs[2 * (size_t)(cnt[i] + k - b) + 1] = W.nb[k]; }
      }
    }
    if (tid == 0) W.hdr[r] = make_int4(count, n_pairs, n_inner, 0);
  } else if (mode == WALK_ABSOLUTE) {
    const int len = target >= 0 ? depth + 1 : 0;
    for (int i = len + tid; i < W.out_cap; i += MB_THREADS) W.out_ids[(size_t)r * W.out_cap + i] = -1;
    if (tid == 0) {                                                // the chain (:769-781), from the window end of the path back to the root
      double T[12];
#pragma unroll
      for (int k = 0; k < 12; ++k) T[k] = 0.0;
      if (target >= 0) {
        int cur = order[target], pos = len - 1;
#pragma unroll
        for (int k = 0; k < 12; ++k) T[k] = M.kf[cur].T_anchor_from_w[k];
        if (pos < W.out_cap) W.out_ids[(size_t)r * W.out_cap + pos] = cur;
        for (int nw = parent[cur]; nw >= 0; nw = parent[cur]) {
          double R[12];
          walk_rel(M, W.edges[pedge[cur]], nw, cur, R);
          pose_mul(R, T, T);
          cur = nw; --pos;
          if (pos < W.out_cap) W.out_ids[(size_t)r * W.out_cap + pos] = cur;
        }
      }
#pragma unroll
      for (int k = 0; k < 12; ++k) W.T[(size_t)r * 12 + k] = T[k];
      W.hdr[r] = make_int4(target >= 0 ? SVS_WALK_OK : SVS_WALK_NO_PATH, len, 0, 0);
    }
  } else {                                                         // WALK_REINIT: the changed keyframes in visit order
    int n_changed = 0;
    for (int base = 0; base < n; base += MB_THREADS) {            // block-uniform
      const int p = base + tid;
      const int c = p < n && (flag[order[p]] & 2) ? 1 : 0;
      int tot;
      const int pos = n_changed + block_excl_scan(c, s_w, tot);
      if (c && pos < W.out_cap) W.out_ids[(size_t)r * W.out_cap + pos] = order[p];
      n_changed += tot;
    }
    for (int i = n_changed + tid; i < W.out_cap; i += MB_THREADS) W.out_ids[(size_t)r * W.out_cap + i] = -1;
    if (tid == 0) W.hdr[r] = make_int4(n_changed, n, 0, 0);
  }
}

__global__ __launch_bounds__(MB_THREADS) void map_walk_kernel(MapK M, MapWalkK W) {
  __shared__ int s_w[MB_THREADS / 64];
  __shared__ uint32_t s_old[MAP_KF_WORDS];
  __shared__ int s_first;
  const int r = blockIdx.x;
  map_walk_search(M, W, r, W.roots[r], r, s_w, s_old, s_first);      // (an id the host has checked: in the map, so below kf_hi <= MAP_MAX_KF)
}
}  // namespace

// what every walk needs before its launch: current adjacency rows and a work space per request
static int map_walk_prepare(svs_map *m, int n_requests) {
  svs_ctx *ctx = m->ctx;
  MapWalkState &S = m->walk;
  const size_t rows = 2 * (size_t)std::max(m->max_edges, 1);
  if (!S.d_begin) {
    SVS_HIP(ctx, S.d_begin.alloc((size_t)m->max_kf + 1));
    SVS_HIP(ctx, S.d_cur.alloc((size_t)m->max_kf + 1));
  }
  if (S.d_nb.bytes() < rows * sizeof(int32_t)) {                   // (the edge table is reserved once)
    SVS_HIP(ctx, hipStreamSynchronize(ctx->stream));
    SVS_HIP(ctx, S.d_nb.alloc(rows)); SVS_HIP(ctx, S.d_slot.alloc(rows)); SVS_HIP(ctx, S.d_tmp_nb.alloc(rows)); SVS_HIP(ctx, S.d_tmp_key.alloc(rows));
    S.built_edges = -1;
  }
  if (S.built_edges != m->n_edges || S.built_kf_hi != m->kf_hi) {
    WalkAdjK A{};
    A.begin = S.d_begin; A.cur = S.d_cur; A.nb = S.d_nb; A.slot = S.d_slot; A.tmp_nb = S.d_tmp_nb; A.tmp_key = S.d_tmp_key;
    A.edges = m->d_edges; A.n_edges = m->n_edges; A.kf_hi = m->kf_hi;
    SVS_HIP(ctx, hipMemsetAsync(S.d_begin, 0, ((size_t)m->kf_hi + 1) * sizeof(int32_t), ctx->stream));
    if (m->n_edges) hipLaunchKernelGGL(walk_adj_count_kernel, dim3(div_up(m->n_edges, 256)), dim3(256), 0, ctx->stream, A);
    hipLaunchKernelGGL(walk_adj_scan_kernel, dim3(1), dim3(MB_THREADS), 0, ctx->stream, A);
    if (m->n_edges) {
      hipLaunchKernelGGL(walk_adj_fill_kernel, dim3(div_up(m->n_edges, 256)), dim3(256), 0, ctx->stream, A);
      hipLaunchKernelGGL(walk_adj_sort_kernel, dim3(div_up(m->kf_hi, 4)), dim3(256), 0, ctx->stream, A);
    }
    SVS_LAUNCH_CHECK(ctx);
    S.built_edges = m->n_edges; S.built_kf_hi = m->kf_hi;
  }
  if (S.work_rows < n_requests || S.work_stride < m->kf_hi) {      // grow-only; a new block needs the stream drained of the walks that use the old one
    SVS_HIP(ctx, hipStreamSynchronize(ctx->stream));
    const int stride = std::max(S.work_stride, (m->kf_hi + 63) & ~63), n = std::max(S.work_rows, n_requests);
    SVS_HIP(ctx, S.d_work.alloc((size_t)n * WALK_ROWS * stride));
    S.work_rows = n; S.work_stride = stride;
  }
  return SVS_OK;
}

// a walk's download: hdr | T | ids | types (the latter three as the mode has them)
struct WalkDn : MapDn {
  MapPiece<int4> hdr; MapPiece<double> T; MapPiece<int32_t> ids, type;
  WalkDn(svs_map *map, int n, int out_cap, bool with_T, bool with_type) : MapDn(map) {
    hdr = piece<int4>(n); T = piece<double>(with_T ? (size_t)n * 12 : 0); ids = piece<int32_t>((size_t)n * out_cap); type = piece<int32_t>(with_type ? (size_t)n * out_cap : 0);
  }
};

// stages `n_up` int32, launches the walk, downloads `dn` and waits
static int map_walk_run(svs_map *m, int n, MapWalkK W, const int32_t *h_up, int n_up, WalkDn &dn) {
  svs_ctx *ctx = m->ctx;
  SVS_DEVICE(ctx);
  if (int rc = dn.reserve()) return rc;
  if (int rc = map_walk_prepare(m, n)) return rc;
  MapUp up(m);
  const auto staged = up.piece<int32_t>(n_up);
  if (int rc = up.reserve()) return rc;
  up.put(staged, h_up);
  if (int rc = up.upload()) return rc;
  const MapWalkState &S = m->walk;
  W.begin = S.d_begin; W.nb = S.d_nb; W.slot = S.d_slot; W.edges = m->d_edges;
  W.roots = up.dev(staged); W.old_ids = W.roots + n;
  W.work = S.d_work; W.stride = S.work_stride;
  W.hdr = dn.dev(dn.hdr); W.T = dn.T.n ? dn.dev(dn.T) : nullptr;
  W.out_ids = dn.dev(dn.ids); W.out_type = dn.type.n ? dn.dev(dn.type) : nullptr;
  hipLaunchKernelGGL(map_walk_kernel, dim3(n), dim3(MB_THREADS), 0, ctx->stream, m->view(), W);
  SVS_LAUNCH_CHECK(ctx);
  return dn.download();
}

extern "C" int svs_map_initial_windows(svs_map *m, int n, const int32_t *h_root, int inner_size, int double_size, int window_cap, int32_t *h_count, int32_t *h_ids,
                                       int32_t *h_type) {
  svs_ctx *ctx = m ? m->ctx : nullptr;
  SVS_REQUIRE(ctx, m && n >= 0 && (n == 0 || (h_root && h_count && h_ids && h_type)) && inner_size >= 1 && inner_size < double_size);
  MAP_CAPACITY(ctx, n <= SVS_MAP_WALK_MAX_REQUESTS && double_size <= window_cap && window_cap <= MAP_MAX_KF);
  for (int i = 0; i < n; ++i) SVS_REQUIRE(ctx, svs_map_has_keyframe(m, h_root[i]));
  if (n == 0) return SVS_OK;
  MapWalkK W{};
  W.mode = WALK_WINDOW; W.limit = double_size; W.inner = inner_size; W.out_cap = window_cap; W.loop_id = -1;
  WalkDn dn(m, n, window_cap, false, true);
  if (int rc = map_walk_run(m, n, W, h_root, n, dn)) return rc;
  for (int i = 0; i < n; ++i) h_count[i] = dn.host(dn.hdr)[i].x;
  dn.get(dn.ids, h_ids);
  dn.get(dn.type, h_type);
  return SVS_OK;
}

extern "C" int svs_map_frames_in_neighborhood(svs_map *m, int n, const int32_t *h_root, int size, int32_t *h_count, int32_t *h_ids) {
  svs_ctx *ctx = m ? m->ctx : nullptr;
  SVS_REQUIRE(ctx, m && n >= 0 && (n == 0 || (h_root && h_count && h_ids)) && size >= 1);
  MAP_CAPACITY(ctx, n <= SVS_MAP_WALK_MAX_REQUESTS && size <= MAP_MAX_KF);
  for (int i = 0; i < n; ++i) SVS_REQUIRE(ctx, svs_map_has_keyframe(m, h_root[i]));
  if (n == 0) return SVS_OK;
  MapWalkK W{};
  W.mode = WALK_NEIGHBORHOOD; W.limit = size; W.inner = size; W.out_cap = size; W.loop_id = -1;
  WalkDn dn(m, n, size, false, false);
  if (int rc = map_walk_run(m, n, W, h_root, n, dn)) return rc;
  for (int i = 0; i < n; ++i) h_count[i] = dn.host(dn.hdr)[i].x;
  dn.get(dn.ids, h_ids);
  return SVS_OK;
}

extern "C" int svs_map_absolute_poses(svs_map *m, int n, const int32_t *h_kf_ids, int path_cap, int32_t *h_status, int32_t *h_path_len, double *h_T, int32_t *h_path) {
  svs_ctx *ctx = m ? m->ctx : nullptr;
  SVS_REQUIRE(ctx, m && n >= 0 && (n == 0 || (h_kf_ids && h_status && h_T)) && path_cap >= 0 && (path_cap == 0 || h_path));
  MAP_CAPACITY(ctx, n <= SVS_MAP_WALK_MAX_REQUESTS && path_cap <= MAP_MAX_KF);
  for (int i = 0; i < n; ++i) SVS_REQUIRE(ctx, svs_map_has_keyframe(m, h_kf_ids[i]));
  if (n == 0) return SVS_OK;
  MapWalkK W{};
  W.mode = WALK_ABSOLUTE; W.limit = WALK_INF; W.out_cap = path_cap; W.loop_id = -1;
  WalkDn dn(m, n, path_cap, true, false);
  if (int rc = map_walk_run(m, n, W, h_kf_ids, n, dn)) return rc;
  const int4 *hdr = dn.host(dn.hdr);
  for (int i = 0; i < n; ++i) { h_status[i] = hdr[i].x; if (h_path_len) h_path_len[i] = hdr[i].y; }
  dn.get(dn.T, h_T);
  dn.get(dn.ids, h_path);
  return SVS_OK;
}

extern "C" int svs_map_reinitialize_poses(svs_map *m, int32_t root_id, int32_t loop_id, int n_old, const int32_t *h_old_window, int changed_cap, int32_t *h_n_changed,
                                          int32_t *h_changed) {
  svs_ctx *ctx = m ? m->ctx : nullptr;
  SVS_REQUIRE(ctx, m && n_old >= 0 && (n_old == 0 || h_old_window) && changed_cap >= 0 && (changed_cap == 0 || h_changed) && h_n_changed);
  SVS_REQUIRE(ctx, svs_map_has_keyframe(m, root_id) && (loop_id == -1 || svs_map_has_keyframe(m, loop_id)));
  MAP_CAPACITY(ctx, changed_cap <= MAP_MAX_KF);
  if (int rc = map_check_ids(m, n_old, h_old_window, m->kf_in, m->max_kf, true)) return rc;
  std::vector<int32_t> up((size_t)n_old + 1);
  up[0] = root_id;
  if (n_old) memcpy(up.data() + 1, h_old_window, (size_t)n_old * sizeof(int32_t));
  MapWalkK W{};
  W.mode = WALK_REINIT; W.limit = WALK_INF; W.out_cap = changed_cap; W.loop_id = loop_id; W.n_old = n_old;
  WalkDn dn(m, 1, changed_cap, false, false);
  if (int rc = map_walk_run(m, 1, W, up.data(), n_old + 1, dn)) return rc;
  *h_n_changed = dn.host(dn.hdr)->x;
  dn.get(dn.ids, h_changed);
  return SVS_OK;
}
