// map_nbh.inc -- the neighbourhood of a front-end stream from the resident map: from a vertex list (nbh_map.h) and from a root id (nbr_map.h); included by
// map.hip behind map_walk.inc, whose map_walk_search it calls.
namespace {
// ---- the neighbourhood of a front-end stream (Backend::computeNeighborhood from the vertex list onwards, backend.cpp:311-386): one workgroup per request.
// The same sets as above -- the given vertices and the anchors as LDS bitmaps over keyframe ids, the points as the request's row of M.mark, ascending ids by
// popcounts and prefixes -- and a table id -> slot of the stream in LDS.  Everything that decides whether the request fits (the point count, the vertex count) is
// known before the first write into the front end's tables: a request over capacity returns with those untouched.
// steps a-f of the neighbourhood of a vertex list, shared by map_nbh_kernel and map_nbr_collect_kernel (below): the points observed by the list's keyframes
// as ascending ids in ids_row[id_off ..] (what lies at or behind ids_row[cap] is only counted), their anchors, and the anchors that are not in the list ("extra":
// this lane's word of that bitmap, `rank` the set bits in the words before it).  Every lane of the workgroup calls it (barriers inside)
struct NbhSets { int n_map, n_no_slot, n_extra, rank; uint32_t extra; bool over_points; };
__device__ __forceinline__ NbhSets nbh_collect(const MapK &M, uint32_t *mark, int32_t *ids_row, int id_off, int cap, const int32_t *vertex, int n_vertex,
                                               const int32_t *slot_kf, int K, uint32_t *s_vert, uint32_t *s_anch, int16_t *s_slot, int *s_w) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int n_words = (M.pt_hi + 31) >> 5;                      // <= mark_b
  // a. empty sets
  s_vert[tid] = 0; s_anch[tid] = 0;
  for (int i = tid; i < MAP_MAX_KF; i += MB_THREADS) s_slot[i] = -1;
  for (int i = tid; i < n_words; i += MB_THREADS) mark[i] = 0;
  __syncthreads();
  // b. the given vertices (ids the host has checked: in the map, so below kf_hi <= MAP_MAX_KF); the slots (an id in at most one slot)
  for (int i = tid; i < n_vertex; i += MB_THREADS) bit_set(s_vert, vertex[i]);
  for (int s = tid; s < K; s += MB_THREADS) { const int id = slot_kf[s]; if ((unsigned)id < (unsigned)MAP_MAX_KF) s_slot[id] = (int16_t)s; }
  __syncthreads();
  // c. mark the points: a wave per feature_table (:316-331)
  for (int i = wave; i < n_vertex; i += MB_THREADS / 64) {
    const int kf = vertex[i];
    const int e1 = M.kf_begin[kf + 1];
    for (int e0 = M.kf_begin[kf]; e0 < e1; e0 += 64) {          // wave-uniform
      const int p = e0 + lane < e1 ? M.kf_rows[e0 + lane] : -1;
      wave_or_by_word(mark, p >> 5, 1u << (p & 31), (unsigned)p < (unsigned)M.pt_hi);
    }
  }
  __syncthreads();
  // d. the set bits in ascending order; what does not fit is only counted
  NbhSets S;
  const int n_map = list_marked(mark, n_words, ids_row, id_off, cap, s_w);
  S.n_map = n_map;
  S.over_points = id_off + n_map > cap;
  __syncthreads();
  // e. their anchors (:374-384), and how many of them the stream holds no slot for
  int c = 0;
  if (!S.over_points)
    for (int i = tid; i < n_map; i += MB_THREADS) {
      const int a = M.pt[ids_row[id_off + i]].kf_index;
      if ((unsigned)a < (unsigned)MAP_MAX_KF) bit_set(s_anch, a);
      if ((unsigned)a >= (unsigned)MAP_MAX_KF || s_slot[a] < 0) ++c;
    }
  (void)block_excl_scan(c, s_w, S.n_no_slot);                    // (its barriers also complete s_anch)
  // f. the anchors that are not among the given vertices, ascending
  S.extra = s_anch[tid] & ~s_vert[tid];
  S.rank = block_excl_scan(__popc(S.extra), s_w, S.n_extra);
  return S;
}

__global__ __launch_bounds__(MB_THREADS) void map_nbh_kernel(MapK M, MapNbhDst D) {
  __shared__ uint32_t s_vert[MAP_KF_WORDS], s_anch[MAP_KF_WORDS];
  __shared__ int16_t s_slot[MAP_MAX_KF];                           // -1: no slot of the stream holds the keyframe
  __shared__ int s_w[MB_THREADS / 64];
  const int r = blockIdx.x, tid = threadIdx.x;
  const nbh_req &Q = D.req[r];
  const int b = Q.stream, n_vertex = Q.n_vertex, n_head = Q.n_head, G = Q.n_groups, MP = D.max_points, K = D.max_keyframes;
  const int32_t *vertex = D.ids + Q.vertex_off, *slot_kf = D.ids + Q.slot_off;
  int32_t *point_id = D.point_id + (size_t)r * MP;
  const NbhSets S = nbh_collect(M, M.mark + (size_t)r * M.mark_b, point_id, n_head, MP, vertex, n_vertex, slot_kf, K, s_vert, s_anch, s_slot, s_w);
  const int n_map = S.n_map, total = n_head + n_map, n_no_slot = S.n_no_slot, rank = S.rank;
  const bool over_points = S.over_points;
  // f. the vertex set: the given ids, behind them the anchors that are not among them, ascending
  const int n_vert = over_points ? 0 : n_vertex + S.n_extra;
  if (over_points || n_vert > D.VB) {                            // block-uniform: nothing of the stream has been touched
    if (tid == 0) {
      svs_nbh_result R{};
      R.n_points = total; R.n_map_points = n_map; R.n_vertex = n_vert; R.n_no_slot = n_no_slot; R.over_capacity = 1;
      D.res[r] = R;
    }
    return;
  }
  // g. the stream's list: the head as it was staged, the map's records (four 16-byte loads each) with the anchor's slot, 0xff up to the previous length
  svs_candidate_point *pts = D.pts + (size_t)b * MP;
  int4 *d4 = reinterpret_cast<int4 *>(pts);
  const svs_candidate_point *head = D.head + Q.head_off;
  const int4 *h4 = reinterpret_cast<const int4 *>(head);
  for (int i = tid; i < n_head * 4; i += MB_THREADS) d4[i] = h4[i];
  for (int i = tid; i < n_map; i += MB_THREADS) {
    // the fourth word: anchor_level, the anchor's id, point_id, pad_
    copy_rec64(pts + n_head + i, M.pt + point_id[n_head + i], [&](int4 &q) { q.y = (unsigned)q.y < (unsigned)MAP_MAX_KF ? (int)s_slot[q.y] : -1; });
  }
  for (int i = total * 4 + tid; i < Q.prev_len * 4; i += MB_THREADS) d4[i] = make_int4(-1, -1, -1, -1);
  for (int i = tid; i < n_head; i += MB_THREADS) point_id[i] = head[i].point_id;
  for (int i = total + tid; i < MP; i += MB_THREADS) point_id[i] = -1;
  if (tid < NBH_MAX_GROUPS) D.group_end[(size_t)b * NBH_MAX_GROUPS + tid] = tid < G - 1 ? Q.group_end[tid] : tid == G - 1 ? total : 0;
  if (tid == 0) { D.n_groups[b] = G; D.n_new[b] = n_head; }
  // h. the vertex set with the poses the map stores
  int32_t *vid = D.vertex_id + (size_t)r * D.VB;
  double *vT = D.vertex_T + (size_t)r * D.VB * 12;
  for (int i = tid; i < n_vertex * 12; i += MB_THREADS) {
    const int v = i / 12, k = i % 12, id = vertex[v];
    vT[i] = M.kf[id].T_anchor_from_w[k];
    if (k == 0) vid[v] = id;
  }
  for_each_set_bit(S.extra, tid << 5, n_vertex + rank, [&](int id, int e) {      // e < n_vert <= VB
    vid[e] = id;
    for (int k = 0; k < 12; ++k) vT[(size_t)e * 12 + k] = M.kf[id].T_anchor_from_w[k];
  });
  for (int i = n_vert * 12 + tid; i < D.VB * 12; i += MB_THREADS) {
    vT[i] = 0.0;
    if (i % 12 == 0) vid[i / 12] = -1;
  }
  // i. the slots that hold a keyframe of the map take its pose (the pyramid pointers and strides stay)
  svs_keyframe *kfs = D.kfs + (size_t)b * K;
  double *sT = D.slot_T + (size_t)r * K * 12;
  for (int i = tid; i < K * 12; i += MB_THREADS) {
    const int s = i / 12, k = i % 12, id = slot_kf[s];
    double v = 0.0;
    if (D.refresh && (unsigned)id < (unsigned)MAP_MAX_KF) { v = M.kf[id].T_anchor_from_w[k]; kfs[s].T_anchor_from_w[k] = v; }
    sT[i] = v;
  }
  if (tid == 0) {
    svs_nbh_result R{};
    R.n_points = total; R.n_map_points = n_map; R.n_vertex = n_vert; R.n_no_slot = n_no_slot; R.over_capacity = 0;
    D.res[r] = R;
  }
}

// ---- a stream's whole neighbourhood from a root id (nbr_map.h; the contract is in the header under svs_frontend_set_neighborhood_from_root) -------------------
//   map_nbr_collect_kernel   one workgroup per request: findNeighborsOfRoot (backend.cpp:287-309) on the root's adjacency row walked backwards, compacted by a
//                            workgroup prefix; nbh_collect's point / anchor walk on that list; the vertex set's ids and the vertices outside the window
//   map_nbr_list_kernel      one workgroup: the prefix of those counts over the requests, the flat list (request, vertex) and its length -- on the device
//   map_nbr_walk_kernel      WALK_ABSOLUTE's search for every entry of that list: the grid is sized to an upper bound, workgroup g takes the entries g, g + grid, ..
//                            and leaves at once when there is none; T goes straight into the request's row of vertex poses
//   map_nbr_finish_kernel    one workgroup per request: the poses, the active keyframe's neighbours as a rank sort over (strength, id), the strength matrix, the
//                            head's groups in that order, then everything map_nbh_kernel writes and the stream's resident vertex table
// the records of a request's fixed groups: the leading n_fixed groups, or group fixed_at - 1 alone
__device__ __forceinline__ int nbr_fixed_records(const nbr_req &Q) {
  if (Q.fixed_at == 0) return Q.group_end[Q.n_fixed - 1];
  const int f = Q.fixed_at - 1;
  return Q.group_end[f] - (f ? Q.group_end[f - 1] : 0);
}

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
  const int n_fixed_rec = nbr_fixed_records(Q);
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
  for_each_set_bit(S.extra, tid << 5, n_given + S.rank, [&](int id, int at) { vid[at] = id; });      // at < n_vert <= VB
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
  __shared__ int s_gkey[NBH_MAX_GROUPS];                           // ... and its key (read for a head that comes from the store)
  __shared__ int s_cnt[4];                                         // n_no_path, n_actn, groups of the written head, its records
  const int r = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, VB = D.VB, MP = D.max_points, K = D.max_keyframes;
  const nbr_req &Q = D.req[r];
  const nbr_mid mid = D.mid[r];
  svs_nbr_result R{};
  if (mid.status != NBR_OK) {                                      // block-uniform: nothing of the stream is touched
    if (tid == 0) {
      if (mid.status == NBR_ROOT_OUTSIDE) R.root_outside_window = 1;
      else {
        R.over_capacity = 1; R.n_map_points = mid.n_map; R.n_points = nbr_fixed_records(Q) + mid.n_map; R.n_vertex = mid.n_vert; R.n_no_slot = mid.n_no_slot;
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
    const int fx = Q.fixed_at - 1;                                 // >= 0: the head is the stream's store, group fx (the active keyframe's) is the fixed one
    const bool is_fixed = fx >= 0 ? lane == fx : lane < n_fixed;
    const int gkey = lane < G ? Q.group_kf[lane] : -1;             // (a store's key need not be a keyframe of the map: such a group is left out)
    const int j = lane < G && !is_fixed && (unsigned)gkey < (unsigned)MAP_MAX_KF ? (int)s_vidx[gkey] : NBR_NO_VERTEX;
    const int rank_j = __shfl(has ? rank : -1, j & 63, 64);
    const int where = lane >= G ? -1 : is_fixed ? -2 : j != NBR_NO_VERTEX ? rank_j : -1;
    const bool keyed_kept = where >= 0;
    int before = 0;
    for (int u = 0; u < 64; ++u) {
      const int wu = __shfl(where, u, 64);
      before += wu >= 0 && wu < where ? 1 : 0;
    }
    if (where == -2) place = fx >= 0 ? 0 : lane; else if (keyed_kept) place = n_fixed + before;
    const int n_out = n_fixed + __popcll(__ballot(keyed_kept));
    const int gb = lane < G && lane > 0 ? Q.group_end[lane - 1] : 0, sz = lane < G ? Q.group_end[lane] - gb : 0;
    // sizes by place, their inclusive prefix: one wave
    int mine_src = 0, mine_sz = 0, mine_key = -1;
    for (int u = 0; u < 64; ++u) {
      const int pu = __shfl(place, u, 64), su = __shfl(gb, u, 64), zu = __shfl(sz, u, 64), ku = __shfl(gkey, u, 64);
      if (pu == lane) { mine_src = su; mine_sz = zu; mine_key = ku; }
    }
    const int end = wave_incl_scan(lane < n_out ? mine_sz : 0);
    if (lane < n_out) { s_gsrc[lane] = mine_src; s_gend[lane] = end; s_gkey[lane] = mine_key; }
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
  const svs_candidate_point *head = D.head + (size_t)Q.stream * D.head_stride + Q.head_off;
  const int4 *h4 = reinterpret_cast<const int4 *>(head);
  int32_t *point_id = D.point_id + (size_t)r * MP;
  const int32_t *map_pid = D.map_pid + (size_t)r * MP;
  for (int i = tid; i < n_kept * 4; i += MB_THREADS) {
    const int rec = i >> 2;
    int g = 0;
    while (s_gend[g] <= rec) ++g;                                  // rec < n_kept = s_gend[n_out - 1]
    const int src = s_gsrc[g] + rec - (g ? s_gend[g - 1] : 0);
    int4 q = h4[(size_t)src * 4 + (i & 3)];
    if (D.from_store && (i & 3) == 3) q.y = (unsigned)s_gkey[g] < (unsigned)MAP_MAX_KF ? (int)s_slot[s_gkey[g]] : -1;      // kf_index: the slot that holds the group's keyframe
    d4[i] = q;
    if ((i & 3) == 0) point_id[rec] = head[src].point_id;
  }
  for (int i = tid; i < n_map; i += MB_THREADS) {
    const int p = map_pid[i];
    // the fourth word: anchor_level, the anchor's id, point_id, pad_
    copy_rec64(pts + n_kept + i, M.pt + p, [&](int4 &q) { q.y = (unsigned)q.y < (unsigned)MAP_MAX_KF ? (int)s_slot[q.y] : -1; });
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
}  // namespace

int svs_map_build_neighborhoods(svs_map *m, int n_requests, const MapNbhDst &dst) {
  svs_ctx *ctx = m->ctx;
  if (int rc = map_prepare_walk(m, n_requests)) return rc;
  hipLaunchKernelGGL(map_nbh_kernel, dim3(n_requests), dim3(MB_THREADS), 0, ctx->stream, m->view(), dst);
  SVS_LAUNCH_CHECK(ctx);
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
