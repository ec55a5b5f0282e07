// map_walk.inc -- the pose graph's breadth-first walks on the device-resident map (included by map.hip behind its own exports): computeInitialDoubleWin
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

// counts [n] -> begin [n + 1] in place, and a copy as the fill cursors; one workgroup
__global__ __launch_bounds__(MB_THREADS) void walk_adj_scan_kernel(WalkAdjK A) {
  __shared__ int s_w[MB_THREADS / 64];
  const int n = A.kf_hi;
  int run = 0;
  for (int base = 0; base <= n; base += MB_THREADS) {      // block-uniform; entry n becomes the total
    const int i = base + threadIdx.x;
    const int v = i < n ? A.begin[i] : 0;
    int tot;
    const int off = run + block_excl_scan(v, s_w, tot);
    if (i <= n) { A.begin[i] = off; A.cur[i] = off; }
    run += tot;
  }
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
    for (int i = tid; i < W.n_old; i += MB_THREADS) { const int id = W.old_ids[i]; atomicOr(&s_old[id >> 5], 1u << (id & 31)); }
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

// ---- a stream's whole neighbourhood from a root id (nbr_map.h; the contract is in the header under svs_frontend_set_neighborhood_from_root) -------------------
//   map_nbr_collect_kernel   one workgroup per request: findNeighborsOfRoot (backend.cpp:287-309) on the root's adjacency row walked backwards, compacted by a
//                            workgroup prefix; nbh_collect's point / anchor walk on that list; the vertex set's ids and the vertices outside the window
//   map_nbr_list_kernel      one workgroup: the prefix of those counts over the requests, the flat list (request, vertex) and its length -- on the device
//   map_nbr_walk_kernel      WALK_ABSOLUTE's search for every entry of that list: the grid is sized to an upper bound, workgroup g takes the entries g, g + grid, ..
//                            and leaves at once when there is none; T goes straight into the request's row of vertex poses
//   map_nbr_finish_kernel    one workgroup per request: the poses, the active keyframe's neighbours as a rank sort over (strength, id), the strength matrix, the
//                            head's groups in that order, then everything map_nbh_kernel writes and the stream's resident vertex table
__global__ __launch_bounds__(MB_THREADS) void map_nbr_collect_kernel(MapK M, MapWalkK W, MapNbrDst D) {
  __shared__ uint32_t s_vert[MAP_KF_WORDS], s_anch[MAP_KF_WORDS];
  __shared__ int16_t s_slot[MAP_MAX_KF];
  __shared__ int s_w[MB_THREADS / 64];
  const int r = blockIdx.x, tid = threadIdx.x, VB = D.VB, MP = D.max_points;
  const nbr_req &Q = D.req[r];
  const int root = Q.root, max_nn = Q.max_nn;
  int32_t *vid = D.vertex_id + (size_t)r * VB;
  nbr_mid &Mid = D.mid[r];
  if (!(M.kf_flags[root] & SVS_REG_KF_IN_WINDOW)) {                // block-uniform
    if (tid == 0) { nbr_mid m{}; m.status = NBR_ROOT_OUTSIDE; Mid = m; }
    return;
  }
  // rule 1: the row from its back; entry k of the in-window ones is taken while k <= max_nn
  const int b = W.begin[root], e = W.begin[root + 1];
  int n_in = 0;
  for (int base = 0; base < e - b; base += MB_THREADS) {           // block-uniform
    const int k = e - 1 - (base + tid);
    const int u = k >= b ? W.nb[k] : -1;
    const int in = u >= 0 && (M.kf_flags[u] & SVS_REG_KF_IN_WINDOW) ? 1 : 0;
    int tot;
    const int pos = n_in + block_excl_scan(in, s_w, tot);
    if (in && pos <= max_nn && 1 + pos < VB) vid[1 + pos] = u;
    n_in += tot;
  }
  const int n_nb = max_nn < n_in ? max_nn + 1 : n_in;            // (max_nn + 1 is formed only where it is at most n_in)
  const int n_given = 1 + n_nb;
  if (tid == 0) vid[0] = root;                                     // VB >= 1
  const int n_fixed_rec = Q.group_end[Q.n_fixed - 1];
  if (n_given > VB) {                                              // block-uniform, rule 9 (a)
    if (tid == 0) { nbr_mid m{}; m.status = NBR_OVER; m.n_given = n_given; m.n_vert = n_given; Mid = m; }
    return;
  }
  __syncthreads();                                                 // the list is read by every lane
  const NbhSets S = nbh_collect(M, M.mark + (size_t)r * M.mark_b, D.map_pid + (size_t)r * MP, 0, MP - n_fixed_rec, vid, n_given, D.ids + Q.slot_off, D.max_keyframes,
                                s_vert, s_anch, s_slot, s_w);
  const int n_vert = S.over_points ? 0 : n_given + S.n_extra;
  if (S.over_points || n_vert > VB) {                              // block-uniform, rule 9 (b), (c)
    if (tid == 0) { nbr_mid m{}; m.status = NBR_OVER; m.n_given = n_given; m.n_vert = n_vert; m.n_map = S.n_map; m.n_no_slot = S.over_points ? 0 : S.n_no_slot; Mid = m; }
    return;
  }
  uint32_t extra = S.extra;
  for (int at = n_given + S.rank; extra; ++at) {                   // at < n_vert <= VB
    vid[at] = (tid << 5) + __ffs((int)extra) - 1;
    extra &= extra - 1;
  }
  for (int i = n_vert + tid; i < VB; i += MB_THREADS) vid[i] = -1;
  __syncthreads();
  // the vertices outside the window, ascending index: one wave's ballot (VB <= 64)
  if (tid < 64) {
    const bool out = tid < n_vert && !(M.kf_flags[vid[tid]] & SVS_REG_KF_IN_WINDOW);
    const unsigned long long mask = __ballot(out);
    if (out) D.walk_v[(size_t)r * VB + __popcll(mask & ((1ull << tid) - 1ull))] = tid;
    if (tid == 0) {
      nbr_mid m{};
      m.status = NBR_OK; m.n_given = n_given; m.n_vert = n_vert; m.n_map = S.n_map; m.n_no_slot = S.n_no_slot; m.n_walk = __popcll(mask);
      Mid = m;
    }
  }
}

__global__ __launch_bounds__(MB_THREADS) void map_nbr_list_kernel(MapNbrDst D) {
  __shared__ int s_w[MB_THREADS / 64];
  const int tid = threadIdx.x, R = D.R, VB = D.VB;
  int run = 0;
  for (int base = 0; base <= R; base += MB_THREADS) {              // block-uniform; entry R becomes the total
    const int i = base + tid;
    const int v = i < R ? D.mid[i].n_walk : 0;
    int tot;
    const int off = run + block_excl_scan(v, s_w, tot);
    if (i <= R) D.walk_off[i] = off;
    run += tot;
  }
  __syncthreads();
  for (int i = tid; i < R * VB; i += MB_THREADS) {
    const int r = i / VB, k = i % VB;
    if (k < D.mid[r].n_walk) D.walk_list[D.walk_off[r] + k] = make_int2(r, D.walk_v[i]);      // < walk_off[R] <= R * VB
  }
}

__global__ __launch_bounds__(MB_THREADS) void map_nbr_walk_kernel(MapK M, MapWalkK W, MapNbrDst D) {
  __shared__ int s_w[MB_THREADS / 64];
  __shared__ uint32_t s_old[MAP_KF_WORDS];
  __shared__ int s_first;
  const int n = D.walk_off[D.R];
  for (int j = blockIdx.x; j < n; j += gridDim.x) {                // block-uniform
    const int2 q = D.walk_list[j];
    const int row = q.x * D.VB + q.y;
    map_walk_search(M, W, row, D.vertex_id[row], blockIdx.x, s_w, s_old, s_first);
    __syncthreads();
  }
}

constexpr int NBR_NO_VERTEX = 0xff;
static_assert(SVS_KF_MAX_VERTICES <= 64 && SVS_KF_MAX_VERTICES < NBR_NO_VERTEX, "a vertex index is a byte, the vertex set one wave's ballot");
static_assert(sizeof(svs_kf_vertex) == 112 && sizeof(svs_kf_table) == 16 + 4 * SVS_KF_MAX_VERTICES, "written word by word below");

__global__ __launch_bounds__(MB_THREADS) void map_nbr_finish_kernel(MapK M, MapWalkK W, MapNbrDst D) {
  __shared__ int16_t s_slot[MAP_MAX_KF];                           // -1: no slot of the stream holds the keyframe
  __shared__ uint8_t s_vidx[MAP_MAX_KF];                           // the place of a keyframe in the vertex set, NBR_NO_VERTEX: not in it
  __shared__ double s_T[SVS_KF_MAX_VERTICES][12];
  __shared__ int s_actn[SVS_KF_MAX_VERTICES];                      // rule 4: vertex indices in order
  __shared__ int s_gsrc[NBH_MAX_GROUPS], s_gend[NBH_MAX_GROUPS];   // rule 6, by group of the written head: where its records were staged, one past its last record
  __shared__ int s_cnt[4];                                         // n_no_path, n_actn, groups of the written head, its records
  const int r = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, VB = D.VB, MP = D.max_points, K = D.max_keyframes;
  const nbr_req &Q = D.req[r];
  const nbr_mid mid = D.mid[r];
  svs_nbr_result R{};
  if (mid.status != NBR_OK) {                                      // block-uniform: nothing of the stream is touched
    if (tid == 0) {
      if (mid.status == NBR_ROOT_OUTSIDE) R.root_outside_window = 1;
      else {
        R.over_capacity = 1; R.n_map_points = mid.n_map; R.n_points = Q.group_end[Q.n_fixed - 1] + mid.n_map; R.n_vertex = mid.n_vert; R.n_no_slot = mid.n_no_slot;
        R.n_root_neighbors = mid.n_given - 1;
      }
      D.res[r] = R;
    }
    return;
  }
  const int b = Q.stream, n_vert = mid.n_vert, n_map = mid.n_map, n_head = Q.n_head, G = Q.n_groups, n_fixed = Q.n_fixed;
  const int32_t *slot_kf = D.ids + Q.slot_off, *slot_raw = D.ids + Q.slot_raw_off;
  int32_t *vid = D.vertex_id + (size_t)r * VB;
  double *vT = D.vertex_T + (size_t)r * VB * 12;
  // a. id -> slot, id -> vertex index
  for (int i = tid; i < MAP_MAX_KF; i += MB_THREADS) { s_slot[i] = -1; s_vidx[i] = NBR_NO_VERTEX; }
  __syncthreads();
  for (int s = tid; s < K; s += MB_THREADS) { const int id = slot_kf[s]; if ((unsigned)id < (unsigned)MAP_MAX_KF) s_slot[id] = (int16_t)s; }
  if (tid < n_vert) s_vidx[vid[tid]] = (uint8_t)tid;
  // b. rule 3: the stored pose inside the window and without a path, else the search's
  for (int i = tid; i < VB * 12; i += MB_THREADS) {
    const int v = i / 12, k = i % 12;
    double t = 0.0;
    if (v < n_vert) {
      const int id = vid[v];
      const bool walked = !(M.kf_flags[id] & SVS_REG_KF_IN_WINDOW) && D.walk_hdr[(size_t)r * VB + v].x == SVS_WALK_OK;
      t = walked ? vT[i] : M.kf[id].T_anchor_from_w[k];
      s_T[v][k] = t;
    }
    vT[i] = t;
  }
  if (tid < 64) {
    const bool lost = tid < n_vert && !(M.kf_flags[vid[tid]] & SVS_REG_KF_IN_WINDOW) && D.walk_hdr[(size_t)r * VB + tid].x != SVS_WALK_OK;
    const unsigned long long mask = __ballot(lost);
    if (tid == 0) s_cnt[0] = __popcll(mask);
  }
  __syncthreads();
  // c. rule 4: lane v of the first wave looks for v in act's row; the list is those found at their rank by (strength, id)
  const int act = s_vidx[Q.act] == NBR_NO_VERTEX ? -1 : (int)s_vidx[Q.act];
  if (wave == 0) {
    bool has = false;
    unsigned long long key = 0;
    if (act >= 0 && lane < n_vert && lane != act) {
      const int id = vid[lane], rb = W.begin[Q.act], re = W.begin[Q.act + 1];
      for (int k = rb; k < re; ++k)
        if (W.nb[k] == id) {                                       // (at most once: an edge is in the table once)
          has = true;
          key = ((unsigned long long)((uint32_t)W.edges[W.slot[k]].strength ^ 0x80000000u) << 32) | (uint32_t)id;
          break;
        }
    }
    int rank = 0;
    for (int u = 0; u < 64; ++u) {
      const unsigned long long ku = __shfl((long long)key, u, 64);
      const int hu = __shfl(has ? 1 : 0, u, 64);
      rank += hu && ku < key ? 1 : 0;
    }
    if (has) s_actn[rank] = lane;
    const int n_actn = __popcll(__ballot(has));
    if (lane == 0) s_cnt[1] = n_actn;
    // d. rule 6: lane g is head group g.  Fixed groups stay; a keyed group goes behind them at the place of its key in rule 4's list, which is the rank
    // lane j of this wave has just found for vertex j
    int place = -1;                                                // among the written groups: fixed g -> g, keyed -> n_fixed + its rank among the kept
    const int j = lane >= n_fixed && lane < G ? (int)s_vidx[Q.group_kf[lane]] : NBR_NO_VERTEX;
    const int rank_j = __shfl(has ? rank : -1, j & 63, 64);
    const int where = lane >= G ? -1 : lane < n_fixed ? -2 : j != NBR_NO_VERTEX ? rank_j : -1;
    const bool keyed_kept = where >= 0;
    int before = 0;
    for (int u = 0; u < 64; ++u) {
      const int wu = __shfl(where, u, 64);
      before += wu >= 0 && wu < where ? 1 : 0;
    }
    if (where == -2) place = lane; else if (keyed_kept) place = n_fixed + before;
    const int n_out = n_fixed + __popcll(__ballot(keyed_kept));
    const int gb = lane < G && lane > 0 ? Q.group_end[lane - 1] : 0, sz = lane < G ? Q.group_end[lane] - gb : 0;
    // sizes by place, their inclusive prefix: one wave
    int mine_src = 0, mine_sz = 0;
    for (int u = 0; u < 64; ++u) {
      const int pu = __shfl(place, u, 64), su = __shfl(gb, u, 64), zu = __shfl(sz, u, 64);
      if (pu == lane) { mine_src = su; mine_sz = zu; }
    }
    const int end = wave_incl_scan(lane < n_out ? mine_sz : 0);
    if (lane < n_out) { s_gsrc[lane] = mine_src; s_gend[lane] = end; }
    const int kept = __shfl(end, 63, 64);
    if (lane == 0) { s_cnt[2] = n_out; s_cnt[3] = kept; }
  }
  __syncthreads();
  const int n_no_path = s_cnt[0], n_actn = s_cnt[1], n_out = s_cnt[2], n_kept = s_cnt[3], total = n_kept + n_map;
  R.n_points = total; R.n_map_points = n_map; R.n_vertex = n_vert; R.n_no_slot = mid.n_no_slot; R.n_root_neighbors = mid.n_given - 1; R.n_no_path = n_no_path;
  R.act_index = act; R.n_act_neighbors = n_actn; R.n_head_kept = n_kept; R.n_head_dropped = n_head - n_kept; R.n_groups = n_out + 1;
  // e. rules 4 and 5 as outputs (not state of the stream: written also for a request that turns out over capacity in f)
  for (int i = tid; i < VB; i += MB_THREADS) D.act_nb[(size_t)r * VB + i] = i < n_actn ? s_actn[i] : -1;
  int32_t *st = D.strength + (size_t)r * VB * VB;
  for (int i = tid; i < VB * VB; i += MB_THREADS) st[i] = -1;
  __syncthreads();
  for (int i = wave; i < n_vert; i += MB_THREADS / 64) {           // a wave per vertex, its lanes along the row
    const int id = vid[i], rb = W.begin[id], re = W.begin[id + 1];
    for (int k = rb + lane; k < re; k += 64) {
      const int j = s_vidx[W.nb[k]];
      if (j != NBR_NO_VERTEX) st[i * VB + j] = W.edges[W.slot[k]].strength;
    }
  }
  // f. rule 9 (d)
  if (total > MP) {                                                // block-uniform
    if (tid == 0) { R.over_capacity = 1; D.res[r] = R; }
    return;
  }
  // g. the stream's list: the head's groups at their places, the map's records with the anchor's slot, 0xff up to the previous length
  svs_candidate_point *pts = D.pts + (size_t)b * MP;
  int4 *d4 = reinterpret_cast<int4 *>(pts);
  const svs_candidate_point *head = D.head + Q.head_off;
  const int4 *h4 = reinterpret_cast<const int4 *>(head);
  int32_t *point_id = D.point_id + (size_t)r * MP;
  const int32_t *map_pid = D.map_pid + (size_t)r * MP;
  for (int i = tid; i < n_kept * 4; i += MB_THREADS) {
    const int rec = i >> 2;
    int g = 0;
    while (s_gend[g] <= rec) ++g;                                  // rec < n_kept = s_gend[n_out - 1]
    const int src = s_gsrc[g] + rec - (g ? s_gend[g - 1] : 0);
    d4[i] = h4[(size_t)src * 4 + (i & 3)];
    if ((i & 3) == 0) point_id[rec] = head[src].point_id;
  }
  for (int i = tid; i < n_map; i += MB_THREADS) {
    const int p = map_pid[i];
    const int4 *s4 = reinterpret_cast<const int4 *>(M.pt + p);
    int4 q = s4[3];                                                // anchor_level, the anchor's id, point_id, pad_
    q.y = (unsigned)q.y < (unsigned)MAP_MAX_KF ? (int)s_slot[q.y] : -1;
    int4 *o4 = d4 + (size_t)(n_kept + i) * 4;
    o4[0] = s4[0]; o4[1] = s4[1]; o4[2] = s4[2]; o4[3] = q;
    point_id[n_kept + i] = p;
  }
  for (int i = total * 4 + tid; i < Q.prev_len * 4; i += MB_THREADS) d4[i] = make_int4(-1, -1, -1, -1);
  for (int i = total + tid; i < MP; i += MB_THREADS) point_id[i] = -1;
  if (tid < NBH_MAX_GROUPS) D.group_end[(size_t)b * NBH_MAX_GROUPS + tid] = tid < n_out ? s_gend[tid] : tid == n_out ? total : 0;
  if (tid == 0) { D.n_groups[b] = n_out + 1; D.n_new[b] = n_kept; }
  // h. rule 7
  svs_keyframe *kfs = D.kfs + (size_t)b * K;
  double *sT = D.slot_T + (size_t)r * K * 12;
  for (int i = tid; i < K * 12; i += MB_THREADS) {
    const int s = i / 12, k = i % 12, id = slot_kf[s];
    double v = 0.0;
    if (D.refresh && (unsigned)id < (unsigned)MAP_MAX_KF) {
      v = s_vidx[id] != NBR_NO_VERTEX ? s_T[s_vidx[id]][k] : M.kf[id].T_anchor_from_w[k];
      kfs[s].T_anchor_from_w[k] = v;
    }
    sT[i] = v;
  }
  // i. rule 8: the words svs_frontend_set_vertex_table's staging holds
  int32_t *tab = reinterpret_cast<int32_t *>(D.vt_tab + b);
  for (int i = tid; i < 4 + SVS_KF_MAX_VERTICES; i += MB_THREADS)
    tab[i] = i == 0 ? n_vert : i == 1 ? act : i == 2 ? (act >= 0 ? n_actn : 0) : i == 3 ? 0 : (i - 4 < n_actn ? s_actn[i - 4] : 0);
  svs_kf_vertex *vtx = D.vt_vtx + (size_t)b * SVS_KF_MAX_VERTICES;
  for (int i = tid; i < SVS_KF_MAX_VERTICES * 14; i += MB_THREADS) {
    const int v = i / 14, k = i % 14;
    long long word = 0;
    if (v < n_vert) {
      if (k < 12) word = __double_as_longlong(s_T[v][k]);
      else if (k == 12) word = (long long)(((unsigned long long)(uint32_t)SVS_KF_SET_MAP << 32) | (uint32_t)vid[v]);      // kf_id | set_begin
    }
    reinterpret_cast<long long *>(vtx + v)[k] = word;              // k == 13: set_count, pad_
  }
  for (int s = tid; s < K; s += MB_THREADS) D.vt_slot[(size_t)b * K + s] = slot_raw[s];
  if (tid == 0) D.res[r] = R;
}

__global__ __launch_bounds__(256) void map_get_poses_kernel(MapK M, const int32_t *ids, int n, double *out) {
  const int t = blockIdx.x * 256 + threadIdx.x, i = t / 12, k = t % 12;
  if (i < n) out[t] = M.kf[ids[i]].T_anchor_from_w[k];
}

size_t walk_align(size_t v) { return (v + 15) & ~(size_t)15; }
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

// stages `n_up` int32, launches the walk, downloads hdr | T | ids | types (the latter three as the mode has them) and waits
static int map_walk_run(svs_map *m, int n, MapWalkK W, const int32_t *h_up, int n_up, bool with_T, bool with_type) {
  svs_ctx *ctx = m->ctx;
  SVS_DEVICE(ctx);
  const size_t o_T = walk_align((size_t)n * sizeof(int4)), o_ids = o_T + (with_T ? (size_t)n * 12 * sizeof(double) : 0),
               o_type = walk_align(o_ids + (size_t)n * W.out_cap * sizeof(int32_t)), bytes = o_type + (with_type ? (size_t)n * W.out_cap * sizeof(int32_t) : 0);
  if (int rc = map_dn_reserve(m, bytes)) return rc;
  if (int rc = map_walk_prepare(m, n)) return rc;
  uint8_t *hs;
  if (int rc = map_stage(m, (size_t)n_up * sizeof(int32_t), &hs)) return rc;
  memcpy(hs, h_up, (size_t)n_up * sizeof(int32_t));
  if (int rc = map_upload(m, m->d_up, (size_t)n_up * sizeof(int32_t))) return rc;
  const MapWalkState &S = m->walk;
  W.begin = S.d_begin; W.nb = S.d_nb; W.slot = S.d_slot; W.edges = m->d_edges;
  W.roots = reinterpret_cast<const int32_t *>(m->d_up.get()); W.old_ids = W.roots + n;
  W.work = S.d_work; W.stride = S.work_stride;
  W.hdr = reinterpret_cast<int4 *>(m->d_dn.get()); W.T = with_T ? reinterpret_cast<double *>(m->d_dn.get() + o_T) : nullptr;
  W.out_ids = reinterpret_cast<int32_t *>(m->d_dn.get() + o_ids); W.out_type = with_type ? reinterpret_cast<int32_t *>(m->d_dn.get() + o_type) : nullptr;
  hipLaunchKernelGGL(map_walk_kernel, dim3(n), dim3(MB_THREADS), 0, ctx->stream, m->view(), W);
  SVS_LAUNCH_CHECK(ctx);
  SVS_HIP(ctx, hipMemcpyAsync(m->h_dn, m->d_dn, bytes, hipMemcpyDeviceToHost, ctx->stream));
  SVS_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return SVS_OK;
}

// nbr_map.h: the four launches of svs_frontend_set_neighborhood_from_root behind the front end's staged upload
int svs_map_build_root_neighborhoods(svs_map *m, const MapNbrDst &dst) {
  svs_ctx *ctx = m->ctx;
  const int R = dst.R, grid = std::min(R * dst.VB, (int)SVS_MAP_WALK_MAX_REQUESTS);      // the searches' upper bound; one work space per workgroup
  if (int rc = map_prepare_walk(m, R)) return rc;
  if (int rc = map_walk_prepare(m, grid)) return rc;
  const MapWalkState &S = m->walk;
  MapWalkK W{};
  W.begin = S.d_begin; W.nb = S.d_nb; W.slot = S.d_slot; W.edges = m->d_edges;
  W.mode = WALK_ABSOLUTE; W.limit = WALK_INF; W.out_cap = 0; W.loop_id = -1;
  W.work = S.d_work; W.stride = S.work_stride;
  W.hdr = dst.walk_hdr; W.T = dst.vertex_T;
  const MapK M = m->view();
  hipLaunchKernelGGL(map_nbr_collect_kernel, dim3(R), dim3(MB_THREADS), 0, ctx->stream, M, W, dst);
  hipLaunchKernelGGL(map_nbr_list_kernel, dim3(1), dim3(MB_THREADS), 0, ctx->stream, dst);
  hipLaunchKernelGGL(map_nbr_walk_kernel, dim3(grid), dim3(MB_THREADS), 0, ctx->stream, M, W, dst);
  hipLaunchKernelGGL(map_nbr_finish_kernel, dim3(R), dim3(MB_THREADS), 0, ctx->stream, M, W, dst);
  SVS_LAUNCH_CHECK(ctx);
  return SVS_OK;
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
  if (int rc = map_walk_run(m, n, W, h_root, n, false, true)) return rc;
  const size_t o_ids = walk_align((size_t)n * sizeof(int4)), o_type = walk_align(o_ids + (size_t)n * window_cap * sizeof(int32_t));
  const int4 *hdr = reinterpret_cast<const int4 *>(m->h_dn.get());
  for (int i = 0; i < n; ++i) h_count[i] = hdr[i].x;
  memcpy(h_ids, m->h_dn.get() + o_ids, (size_t)n * window_cap * sizeof(int32_t));
  memcpy(h_type, m->h_dn.get() + o_type, (size_t)n * window_cap * sizeof(int32_t));
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
  if (int rc = map_walk_run(m, n, W, h_root, n, false, false)) return rc;
  const int4 *hdr = reinterpret_cast<const int4 *>(m->h_dn.get());
  for (int i = 0; i < n; ++i) h_count[i] = hdr[i].x;
  memcpy(h_ids, m->h_dn.get() + walk_align((size_t)n * sizeof(int4)), (size_t)n * size * sizeof(int32_t));
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
  if (int rc = map_walk_run(m, n, W, h_kf_ids, n, true, false)) return rc;
  const size_t o_T = walk_align((size_t)n * sizeof(int4)), o_ids = o_T + (size_t)n * 12 * sizeof(double);
  const int4 *hdr = reinterpret_cast<const int4 *>(m->h_dn.get());
  for (int i = 0; i < n; ++i) { h_status[i] = hdr[i].x; if (h_path_len) h_path_len[i] = hdr[i].y; }
  memcpy(h_T, m->h_dn.get() + o_T, (size_t)n * 12 * sizeof(double));
  if (path_cap) memcpy(h_path, m->h_dn.get() + o_ids, (size_t)n * path_cap * sizeof(int32_t));
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
  if (int rc = map_walk_run(m, 1, W, up.data(), n_old + 1, false, false)) return rc;
  *h_n_changed = reinterpret_cast<const int4 *>(m->h_dn.get())->x;
  if (changed_cap) memcpy(h_changed, m->h_dn.get() + walk_align(sizeof(int4)), (size_t)changed_cap * sizeof(int32_t));
  return SVS_OK;
}

extern "C" int svs_map_get_poses(svs_map *m, int n, const int32_t *h_kf_ids, double *h_poses) {
  svs_ctx *ctx = m ? m->ctx : nullptr;
  SVS_REQUIRE(ctx, m && n >= 0 && (n == 0 || (h_kf_ids && h_poses)));
  for (int i = 0; i < n; ++i) SVS_REQUIRE(ctx, svs_map_has_keyframe(m, h_kf_ids[i]));
  if (n == 0) return SVS_OK;
  SVS_DEVICE(ctx);
  const size_t bytes = (size_t)n * 12 * sizeof(double);
  if (int rc = map_dn_reserve(m, bytes)) return rc;
  uint8_t *hs;
  if (int rc = map_stage(m, (size_t)n * sizeof(int32_t), &hs)) return rc;
  memcpy(hs, h_kf_ids, (size_t)n * sizeof(int32_t));
  if (int rc = map_upload(m, m->d_up, (size_t)n * sizeof(int32_t))) return rc;
  hipLaunchKernelGGL(map_get_poses_kernel, dim3(div_up(n * 12, 256)), dim3(256), 0, ctx->stream, m->view(), reinterpret_cast<const int32_t *>(m->d_up.get()), n,
                     reinterpret_cast<double *>(m->d_dn.get()));
  SVS_LAUNCH_CHECK(ctx);
  SVS_HIP(ctx, hipMemcpyAsync(m->h_dn, m->d_dn, bytes, hipMemcpyDeviceToHost, ctx->stream));
  SVS_HIP(ctx, hipStreamSynchronize(ctx->stream));
  memcpy(h_poses, m->h_dn.get(), bytes);
  return SVS_OK;
}

extern "C" int svs_map_prepare_window_from_root(svs_map *m, int32_t root_id, int inner_size, int double_size, int set_window_flags, int window_cap,
                                                svs_map_window_result *h_res, int32_t *h_window_ids, int32_t *h_window_type) {
  svs_ctx *ctx = m ? m->ctx : nullptr;
  SVS_REQUIRE(ctx, m && h_res && inner_size >= 1 && inner_size < double_size && svs_map_has_keyframe(m, root_id));
  MAP_CAPACITY(ctx, double_size <= window_cap && window_cap <= MAP_WIN_MAX);
  if (m->n_unmeasured > 0) { ctx->err = "svs_map_prepare_window_from_root: the map holds observations without a measurement (svs_map_add_observations)"; return SVS_ERR_INVALID; }
  SVS_DEVICE(ctx);
  if (int rc = map_win_reserve(m)) return rc;
  if (int rc = map_prepare_walk(m, 1)) return rc;
  MapWalkState &S = m->walk;
  const size_t need = (3 * (size_t)MAP_WIN_MAX + 4 * (size_t)std::max(m->n_edges, 1)) * sizeof(int32_t);
  if (S.d_pairs.bytes() < need) {
    SVS_HIP(ctx, hipStreamSynchronize(ctx->stream));
    SVS_HIP(ctx, S.d_pairs.alloc_bytes(need * 2));
  }
  // the initial window and the pairs, left on the device
  MapWalkK W{};
  W.mode = WALK_WINDOW; W.limit = double_size; W.inner = inner_size; W.out_cap = double_size; W.loop_id = -1; W.win = S.d_pairs; W.win_cap = MAP_WIN_MAX;
  if (int rc = map_walk_run(m, 1, W, &root_id, 1, false, true)) return rc;
  const int4 hdr = *reinterpret_cast<const int4 *>(m->h_dn.get());
  MapWinK A = map_win_pieces(m);
  A.ids = S.d_pairs.get(); A.types = A.ids + MAP_WIN_MAX; A.inner = A.types + MAP_WIN_MAX; A.pairs = A.inner + MAP_WIN_MAX;
  A.n0 = hdr.x; A.n_pairs = hdr.y; A.window_cap = window_cap; A.set_flags = set_window_flags != 0;
  return map_win_finish(m, A, hdr.z, window_cap, h_res, h_window_ids, h_window_type);
}
