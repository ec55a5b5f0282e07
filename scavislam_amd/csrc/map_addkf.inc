// map_addkf.inc -- inserting a keyframe into the resident map (SlamGraph::addKeyframe, slam_graph.cpp:143-186), included by map.hip behind map_walk.inc.
//   map_strength_kernel      computeStrength (:467-552) as the closed form of include/scavislam_hip.h, one workgroup per call: the keys are an LDS bitmap over
//                            keyframe ids (new points' anchors, observer rows of the track points), popcount prefixes give the ascending key list and id -> rank,
//                            everything per key is an LDS table of 1024 entries.  t_q(f), "the index of the h-th track entry f observes in class q", is found by
//                            COUNTING, never by arrival order: x = the largest list index with fewer than h such entries in front of it, built bit by bit from the
//                            top -- one pass of integer LDS adds per bit over "entries in front of x | bit".  ceil(log2(n_track + 1)) passes whatever h is; the
//                            counts are sums of integers, so every value is a function of the input alone.
//   map_addkf_apply_kernel   addNewPointsToMap / addNewObsToOldPoints (:358-420) from the block the strength kernel read: the kept points and the kept measurement
//                            records are compacted by prefix sums into the point store, the pair log and the measured store in the order the twin calls would
//                            give them; the new keyframe's pose is pose_mul(T_newkey_from_oldkey, T_oldkey_from_world) formed here.
//   map_get_points_kernel / map_feature_table_kernel      the two read-backs.
// The edges go through map_edge_add_kernel and their constraints through map_cons_kernel, both unchanged.
namespace {
constexpr int AK_MAX_KEYS = SVS_MAP_ADDKF_MAX_NEIGHBORS;
constexpr int AK_UNROLL = 4;           // track entries of a lane whose row bounds are requested together
static_assert(sizeof(svs_map_new_point) == 96 && sizeof(svs_map_track_point) == 32 && sizeof(svs_map_key) == 32 && sizeof(svs_map_strength_result) == 16, "staged as arrays");
static_assert(AK_MAX_KEYS == 2 * MB_THREADS, "a lane owns two keys");

struct MapStrK {
  const svs_map_new_point *np; const svs_map_track_point *tp; const int32_t *tflag;      // tflag bit 0: the entry is in E; bit 1: it adds its pair (first occurrence)
  int n_new, n_track, thr, half_w, half_h, oldkey, clamp;
  svs_map_strength_result *res; svs_map_key *keys; int32_t *kept;
};

// f(list index, left / right class 0 / 1, top / bottom class 2 / 3, observer keyframe) for every observer of every entry of E: AK_UNROLL entries per lane and
// step, their row bounds requested together, then the rows four loads at a time (map_cons_kernel's pattern)
template <class F>
__device__ __forceinline__ void ak_for_each(const MapK &M, const MapStrK &A, F f) {
  const int tid = threadIdx.x;
  for (int i0 = 0; i0 < A.n_track; i0 += MB_THREADS * AK_UNROLL) {
    int g[AK_UNROLL], lr[AK_UNROLL], tb[AK_UNROLL], ob[AK_UNROLL], oe[AK_UNROLL];
#pragma unroll
    for (int k = 0; k < AK_UNROLL; ++k) {
      const int i = i0 + k * MB_THREADS + tid;
      g[k] = -1; lr[k] = 0; tb[k] = 2;
      if (i < A.n_track && (A.tflag[i] & 1)) {
        const svs_map_track_point &t = A.tp[i];
        g[k] = t.global_id;
        lr[k] = t.center[0] < (double)A.half_w ? 0 : 1;
        tb[k] = t.center[1] < (double)A.half_h ? 2 : 3;
      }
    }
#pragma unroll
    for (int k = 0; k < AK_UNROLL; ++k) {
      const bool have = (unsigned)g[k] < (unsigned)M.pt_hi;
      ob[k] = have ? M.pt_begin[g[k]] : 0; oe[k] = have ? M.pt_begin[g[k] + 1] : 0;
    }
#pragma unroll
    for (int k = 0; k < AK_UNROLL; ++k) {
      const int i = i0 + k * MB_THREADS + tid;
      for (int e = ob[k]; e < oe[k]; e += 4) {
        int kf[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) kf[q] = e + q < oe[k] ? M.pt_rows[e + q] : -1;
#pragma unroll
        for (int q = 0; q < 4; ++q)
          if ((unsigned)kf[q] < (unsigned)MAP_MAX_KF) f(i, lr[k], tb[k], kf[q]);
      }
    }
  }
}

__global__ __launch_bounds__(MB_THREADS) void map_strength_kernel(MapK M, MapStrK A) {
  __shared__ uint32_t s_bm[MAP_KF_WORDS];
  __shared__ int s_rank[MAP_KF_WORDS];
  __shared__ int s_cnt[4][AK_MAX_KEYS], s_x[4][AK_MAX_KEYS];
  __shared__ int s_str[AK_MAX_KEYS], s_tstar[AK_MAX_KEYS];
  __shared__ int s_w[MB_THREADS / 64];
  const int tid = threadIdx.x;
  auto rank_of = [&](int id) { return s_rank[id >> 5] + __popc(s_bm[id >> 5] & ((1u << (id & 31)) - 1u)); };
  // a. empty tables
  s_bm[tid] = 0;
  for (int r = tid; r < AK_MAX_KEYS; r += MB_THREADS) {
#pragma unroll
    for (int q = 0; q < 4; ++q) { s_cnt[q][r] = 0; s_x[q][r] = 0; }
    s_str[r] = 0; s_tstar[r] = 0;
  }
  __syncthreads();
  // b. the keys: anchors of the new points (ids the host has checked), observers of E; m = |E|
  for (int i = tid; i < A.n_new; i += MB_THREADS) { const int a = A.np[i].anchor_id; if ((unsigned)a < (unsigned)MAP_MAX_KF) atomicOr(&s_bm[a >> 5], 1u << (a & 31)); }
  ak_for_each(M, A, [&](int, int, int, int kf) { atomicOr(&s_bm[kf >> 5], 1u << (kf & 31)); });
  int mine = 0;
  for (int i = tid; i < A.n_track; i += MB_THREADS) mine += A.tflag[i] & 1;
  int m;
  (void)block_excl_scan(mine, s_w, m);                            // (its barriers also complete s_bm)
  const uint32_t bits = s_bm[tid];
  int n_keys;
  const int rank = block_excl_scan(__popc(bits), s_w, n_keys);
  s_rank[tid] = rank;
  if (n_keys > AK_MAX_KEYS) {                                     // block-uniform: the count and the mark, nothing else
    if (tid == 0) { svs_map_strength_result R; R.n_keys = n_keys; R.m = 0; R.over_capacity = 1; R.n_edges = 0; *A.res = R; }
    return;
  }
  __syncthreads();
  const int h = max(A.thr / 2, 1);
  if (m == 0) {
    // c. no track point of the map: the new points' counts stand
    for (int i = tid; i < A.n_new; i += MB_THREADS) { const int a = A.np[i].anchor_id; if ((unsigned)a < (unsigned)MAP_MAX_KF) atomicAdd(&s_str[rank_of(a)], 1); }
  } else {
    // d. the four class totals
    ak_for_each(M, A, [&](int, int lr, int tb, int kf) { const int r = rank_of(kf); atomicAdd(&s_cnt[lr][r], 1); atomicAdd(&s_cnt[tb][r], 1); });
  }
  __syncthreads();
  for (int r = tid; r < AK_MAX_KEYS; r += MB_THREADS) {
    if (r < n_keys) { svs_map_key &K = A.keys[r]; K.n_left = s_cnt[0][r]; K.n_right = s_cnt[1][r]; K.n_top = s_cnt[2][r]; K.n_bottom = s_cnt[3][r]; }
    // a key that lacks the h-th entry of a class never keeps a count
    s_tstar[r] = (s_cnt[0][r] >= h && s_cnt[1][r] >= h && s_cnt[2][r] >= h && s_cnt[3][r] >= h) ? 0 : 0x7fffffff;
  }
  if (m > 0) {                                                    // block-uniform
    // e. x[q][f] = the largest index with fewer than h entries of class q that f observes in front of it = the index of the h-th; top bit first.  The lane that
    //    decides key r is the lane that empties its counts again, so one barrier on each side of the counting pass is enough
    int nb = 0;
    while ((1 << nb) <= A.n_track) ++nb;                          // x <= n_track (n_track < 2^24: the host)
    for (int b = nb - 1; b >= 0; --b) {
      for (int r = tid; r < AK_MAX_KEYS; r += MB_THREADS) {
#pragma unroll
        for (int q = 0; q < 4; ++q) s_cnt[q][r] = 0;
      }
      __syncthreads();
      ak_for_each(M, A, [&](int i, int lr, int tb, int kf) {
        const int r = rank_of(kf);
        if (i < (s_x[lr][r] | (1 << b))) atomicAdd(&s_cnt[lr][r], 1);
        if (i < (s_x[tb][r] | (1 << b))) atomicAdd(&s_cnt[tb][r], 1);
      });
      __syncthreads();
      for (int r = tid; r < AK_MAX_KEYS; r += MB_THREADS) {
#pragma unroll
        for (int q = 0; q < 4; ++q) if (s_cnt[q][r] < h) s_x[q][r] |= 1 << b;
      }
    }
    for (int r = tid; r < AK_MAX_KEYS; r += MB_THREADS)
      if (s_tstar[r] == 0) s_tstar[r] = max(max(s_x[0][r], s_x[1][r]), max(s_x[2][r], s_x[3][r]));
    __syncthreads();
    // f. the entries at or behind t*(f) that f observes
    ak_for_each(M, A, [&](int i, int, int, int kf) { const int r = rank_of(kf); if (i >= s_tstar[r]) atomicAdd(&s_str[r], 1); });
  }
  __syncthreads();
  // g. the table in ascending id: a lane's own word; the clamp of oldkey and the edge mark where the call inserts
  int n_edge_mine = 0;
  {
    uint32_t b2 = bits;
    for (int r = rank; b2; ++r) {                                 // r < n_keys <= AK_MAX_KEYS
      const int id = (tid << 5) + __ffs((int)b2) - 1;
      b2 &= b2 - 1;
      int s = s_str[r];
      if (A.clamp && id == A.oldkey) s = max(s, A.thr);
      s_str[r] = s;
      const int edge = (A.clamp && s >= A.thr) ? 1 : 0;
      n_edge_mine += edge;
      svs_map_key &K = A.keys[r];
      K.kf_id = id; K.strength = s; K.edge = edge; K.pad_ = 0;
    }
  }
  for (int r = n_keys + tid; r < AK_MAX_KEYS; r += MB_THREADS) {
    int4 *z = reinterpret_cast<int4 *>(A.keys + r);
    z[0] = make_int4(0, 0, 0, 0); z[1] = make_int4(0, 0, 0, 0);
  }
  int n_edges;
  (void)block_excl_scan(n_edge_mine, s_w, n_edges);               // (its barriers also complete s_str)
  // h. addNewPointsToMap's test (:369)
  if (A.kept)
    for (int i = tid; i < A.n_new; i += MB_THREADS) {
      const int a = A.np[i].anchor_id;
      A.kept[i] = ((unsigned)a < (unsigned)MAP_MAX_KF && s_str[rank_of(a)] >= A.thr) ? 1 : 0;
    }
  if (tid == 0) { svs_map_strength_result R; R.n_keys = n_keys; R.m = m; R.over_capacity = 0; R.n_edges = n_edges; *A.res = R; }
}

struct MapApplyK {
  const svs_map_new_point *np; const svs_map_track_point *tp; const int32_t *tflag, *kept;
  int n_new, n_track, oldkey, newkey;
  double T_rel[12];
  int2 *log_tail; svs_ba_edge *meas_tail;      // behind the pairs / the measured records the map holds
};

// one measured pair at position `at` of both tails: obs = c * scale, info as svs_map_add_measured_observations forms it (slam_graph.cpp:1010-1015)
__device__ __forceinline__ void ak_put(const MapApplyK &A, int at, int point, int kf, const double *c, double scale, int level) {
  const double s = 1.0 / (double)(1 << level);
  svs_ba_edge e;
  e.obs[0] = c[0] * scale; e.obs[1] = c[1] * scale; e.obs[2] = c[2] * scale;
  e.info[0] = s * s; e.info[1] = s * s; e.info[2] = 0.333 * 0.333;
  e.point = point; e.pose = kf; e.anchor = 0; e.pad_ = 0;
  A.meas_tail[at] = e;
  A.log_tail[at] = make_int2(point, kf);
}

// one workgroup.  The host has reserved room for every record this can write (n_new points, 2 n_new + n_track pairs) and has checked every id
__global__ __launch_bounds__(MB_THREADS) void map_addkf_apply_kernel(MapK M, MapApplyK A) {
  __shared__ int s_w[MB_THREADS / 64];
  const int tid = threadIdx.x;
  if (tid == 0) {                                                  // (behind map_scatter_kf_kernel on the stream: the record is there, its pose is not)
    double To[12], T[12];
#pragma unroll
    for (int k = 0; k < 12; ++k) To[k] = M.kf[A.oldkey].T_anchor_from_w[k];
    pose_mul(A.T_rel, To, T);
#pragma unroll
    for (int k = 0; k < 12; ++k) M.kf[A.newkey].T_anchor_from_w[k] = T[k];
  }
  // the kept new points, in list order: the point, then (point, newkey) and (point, anchor)
  int n_kept = 0;
  for (int i0 = 0; i0 < A.n_new; i0 += MB_THREADS) {              // block-uniform
    const int i = i0 + tid;
    const bool c = i < A.n_new && A.kept[i] != 0;
    int tot;
    const int pos = n_kept + block_excl_scan(c ? 1 : 0, s_w, tot);
    if (c) {
      const svs_map_new_point p = A.np[i];
      svs_candidate_point q;
#pragma unroll
      for (int k = 0; k < 3; ++k) { q.xyz_anchor[k] = p.xyz_anchor[k]; q.anchor_obs_pyr[k] = p.anchor_obs_pyr[k]; }
      q.anchor_level = p.anchor_level; q.kf_index = p.anchor_id; q.point_id = p.point_id; q.pad_ = 0;
      M.pt[p.point_id] = q;
      ak_put(A, 2 * pos, p.point_id, A.newkey, p.feat_center, 1.0, p.feat_level);
      ak_put(A, 2 * pos + 1, p.point_id, p.anchor_id, p.anchor_obs_pyr, (double)(1 << p.anchor_level), p.anchor_level);
    }
    n_kept += tot;
  }
  // the track points of the map, first occurrences, in list order: (global_id, newkey)
  int n_tr = 0;
  for (int i0 = 0; i0 < A.n_track; i0 += MB_THREADS) {            // block-uniform
    const int i = i0 + tid;
    const bool c = i < A.n_track && (A.tflag[i] & 2) != 0;
    int tot;
    const int pos = n_tr + block_excl_scan(c ? 1 : 0, s_w, tot);
    if (c) { const svs_map_track_point t = A.tp[i]; ak_put(A, 2 * n_kept + pos, t.global_id, A.newkey, t.center, 1.0, t.level); }
    n_tr += tot;
  }
}

__global__ __launch_bounds__(256) void map_get_points_kernel(MapK M, const int32_t *__restrict__ ids, int n, svs_candidate_point *__restrict__ out) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int4 *s4 = reinterpret_cast<const int4 *>(M.pt + ids[i]);
  int4 *d4 = reinterpret_cast<int4 *>(out + i);
  d4[0] = s4[0]; d4[1] = s4[1]; d4[2] = s4[2]; d4[3] = s4[3];
}

struct MapFtK { int kf, cap, n_meas; const svs_ba_edge *meas; int32_t *count, *ids; svs_ba_edge *rec; };

// one workgroup: the keyframe's row as a bitmap over point ids (row 0 of M.mark), ascending ids by popcount prefixes, then the measured store is searched for
// the keyframe's records, each placed by a binary search of its point in that list
__global__ __launch_bounds__(MB_THREADS) void map_feature_table_kernel(MapK M, MapFtK A) {
  __shared__ int s_w[MB_THREADS / 64];
  const int tid = threadIdx.x;
  uint32_t *mark = M.mark;
  const int n_words = (M.pt_hi + 31) >> 5;                        // <= mark_b
  for (int i = tid; i < n_words; i += MB_THREADS) mark[i] = 0;
  __syncthreads();
  const int e1 = M.kf_begin[A.kf + 1];
  for (int e = M.kf_begin[A.kf] + tid; e < e1; e += MB_THREADS) {
    const int p = M.kf_rows[e];
    if ((unsigned)p < (unsigned)M.pt_hi) atomicOr(&mark[p >> 5], 1u << (p & 31));
  }
  __syncthreads();
  int n = 0;
  for (int base = 0; base < n_words; base += MB_THREADS) {        // block-uniform trip count
    const int w = base + tid;
    uint32_t bits = w < n_words ? __hip_atomic_load(&mark[w], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0u;
    int tot;
    int pos = n + block_excl_scan(__popc(bits), s_w, tot);
    while (bits) {
      const int b = __ffs((int)bits) - 1;
      bits &= bits - 1;
      if (pos < A.cap) A.ids[pos] = (w << 5) + b;
      ++pos;
    }
    n += tot;
  }
  const int n_c = min(n, A.cap);
  __syncthreads();
  for (int i = tid; i < n_c; i += MB_THREADS) {
    svs_ba_edge e;
    e.obs[0] = e.obs[1] = e.obs[2] = 0.0; e.info[0] = e.info[1] = e.info[2] = 0.0;
    e.point = A.ids[i]; e.pose = A.kf; e.anchor = -1; e.pad_ = 0;
    A.rec[i] = e;
  }
  __syncthreads();
  for (int i = tid; i < A.n_meas; i += MB_THREADS) {
    const int4 *s4 = reinterpret_cast<const int4 *>(A.meas + i);
    const int4 q = s4[3];                                          // point, pose, anchor, pad_
    if (q.y != A.kf) continue;
    int lo = 0, hi = n_c;
    while (lo < hi) { const int mid = (lo + hi) >> 1; if (A.ids[mid] < q.x) lo = mid + 1; else hi = mid; }
    if (lo < n_c && A.ids[lo] == q.x) {
      int4 *d4 = reinterpret_cast<int4 *>(A.rec + lo);
      d4[0] = s4[0]; d4[1] = s4[1]; d4[2] = s4[2]; d4[3] = q;
    }
  }
  if (tid == 0) *A.count = n;
}
}  // namespace

// ---- host side -----------------------------------------------------------------------------------------------------------------------------------------------
// what both calls refuse about the two lists, and the track flags (bit 0: in E; bit 1: first occurrence in E)
static int addkf_check_lists(svs_map *m, int n_new, const svs_map_new_point *np, int n_track, const svs_map_track_point *tp, int thr, std::vector<int32_t> *flag) {
  svs_ctx *ctx = m->ctx;
  SVS_REQUIRE(ctx, thr >= 0 && n_new >= 0 && n_track >= 0 && (n_new == 0 || np) && (n_track == 0 || tp));
  MAP_CAPACITY(ctx, n_new < (1 << 24) && n_track < (1 << 24));
  for (int i = 0; i < n_new; ++i) SVS_REQUIRE(ctx, svs_map_has_keyframe(m, np[i].anchor_id));
  flag->assign((size_t)n_track, 0);
  std::unordered_set<int32_t> seen;
  for (int i = 0; i < n_track; ++i) {
    const int32_t g = tp[i].global_id;
    if (g < 0 || g >= m->max_pt || !m->pt_in[g]) continue;
    (*flag)[(size_t)i] = seen.insert(g).second ? 3 : 1;
  }
  return SVS_OK;
}

// the pieces of the two blocks: upload [head, written by the caller] | new points | track points | flags; download result | keys | kept
struct AddkfBlocks { size_t o_np, o_tp, o_flag, up_end, o_keys, o_kept, dn_end; };
static AddkfBlocks addkf_blocks(size_t head, int n_new, int n_track) {
  AddkfBlocks B{};
  B.o_np = up_align(head); B.o_tp = B.o_np + up_align((size_t)n_new * sizeof(svs_map_new_point)); B.o_flag = B.o_tp + (size_t)n_track * sizeof(svs_map_track_point);
  B.up_end = up_align(B.o_flag + (size_t)n_track * sizeof(int32_t));
  B.o_keys = sizeof(svs_map_strength_result); B.o_kept = B.o_keys + (size_t)AK_MAX_KEYS * sizeof(svs_map_key);
  B.dn_end = up_align(B.o_kept + (size_t)n_new * sizeof(int32_t));
  return B;
}

// copies the lists into the staged block (the caller has reserved it and written its head), uploads, runs the strength kernel into the download block and waits
static int addkf_strength(svs_map *m, const AddkfBlocks &B, int n_new, const svs_map_new_point *np, int n_track, const svs_map_track_point *tp,
                          const std::vector<int32_t> &flag, int thr, int half_w, int half_h, int oldkey, bool clamp) {
  svs_ctx *ctx = m->ctx;
  uint8_t *hs = m->h_up;
  if (n_new) memcpy(hs + B.o_np, np, (size_t)n_new * sizeof(svs_map_new_point));
  if (n_track) { memcpy(hs + B.o_tp, tp, (size_t)n_track * sizeof(svs_map_track_point)); memcpy(hs + B.o_flag, flag.data(), (size_t)n_track * sizeof(int32_t)); }
  if (B.up_end)
    if (int rc = map_upload(m, m->d_up, B.up_end)) return rc;
  MapStrK A{};
  const uint8_t *U = m->d_up.get();
  A.np = reinterpret_cast<const svs_map_new_point *>(U + B.o_np); A.tp = reinterpret_cast<const svs_map_track_point *>(U + B.o_tp);
  A.tflag = reinterpret_cast<const int32_t *>(U + B.o_flag);
  A.n_new = n_new; A.n_track = n_track; A.thr = thr; A.half_w = half_w; A.half_h = half_h; A.oldkey = oldkey; A.clamp = clamp ? 1 : 0;
  uint8_t *D = m->d_dn.get();
  A.res = reinterpret_cast<svs_map_strength_result *>(D); A.keys = reinterpret_cast<svs_map_key *>(D + B.o_keys);
  A.kept = clamp ? reinterpret_cast<int32_t *>(D + B.o_kept) : nullptr;
  hipLaunchKernelGGL(map_strength_kernel, dim3(1), dim3(MB_THREADS), 0, ctx->stream, m->view(), A);
  SVS_LAUNCH_CHECK(ctx);
  SVS_HIP(ctx, hipMemcpyAsync(m->h_dn, m->d_dn, B.dn_end, hipMemcpyDeviceToHost, ctx->stream));
  SVS_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return SVS_OK;
}

// the key table and the exists mask as the caller gets them
static void addkf_outputs(const svs_map *m, const AddkfBlocks &B, const std::vector<int32_t> &flag, svs_map_strength_result *h_res, svs_map_key *h_keys, int32_t *h_exists) {
  const svs_map_strength_result R = *reinterpret_cast<const svs_map_strength_result *>(m->h_dn.get());
  *h_res = R;
  if (R.over_capacity) memset(h_keys, 0, (size_t)AK_MAX_KEYS * sizeof(svs_map_key));
  else memcpy(h_keys, m->h_dn.get() + B.o_keys, (size_t)AK_MAX_KEYS * sizeof(svs_map_key));
  if (h_exists)
    for (size_t i = 0; i < flag.size(); ++i) h_exists[i] = R.over_capacity ? 0 : (flag[i] & 1);
}

extern "C" int svs_map_compute_strength(svs_map *m, int n_new, const svs_map_new_point *h_new, int n_track, const svs_map_track_point *h_track, int covis_thr,
                                        int half_width, int half_height, svs_map_strength_result *h_res, svs_map_key *h_keys, int32_t *h_track_exists) {
  svs_ctx *ctx = m ? m->ctx : nullptr;
  SVS_REQUIRE(ctx, m && h_res && h_keys);
  std::vector<int32_t> flag;
  if (int rc = addkf_check_lists(m, n_new, h_new, n_track, h_track, covis_thr, &flag)) return rc;
  SVS_DEVICE(ctx);
  const AddkfBlocks B = addkf_blocks(0, n_new, n_track);
  if (int rc = map_dn_reserve(m, B.dn_end)) return rc;
  if (int rc = map_prepare_walk(m, 1)) return rc;
  uint8_t *hs;
  if (int rc = map_stage(m, std::max<size_t>(B.up_end, 16), &hs)) return rc;
  if (int rc = addkf_strength(m, B, n_new, h_new, n_track, h_track, flag, covis_thr, half_width, half_height, -1, false)) return rc;
  addkf_outputs(m, B, flag, h_res, h_keys, h_track_exists);
  return SVS_OK;
}

extern "C" int svs_map_add_first_keyframe(svs_map *m, int32_t id, const svs_keyframe *h_keyframe, const float *disp, int32_t disp_stride, const int32_t *h_fast_thr) {
  svs_ctx *ctx = m ? m->ctx : nullptr;
  SVS_REQUIRE(ctx, m && h_keyframe && m->n_kf == 0 && m->n_pt == 0);      // (slam_graph.cpp:259-260)
  svs_keyframe kf = *h_keyframe;
  const double I[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};
  memcpy(kf.T_anchor_from_w, I, sizeof I);
  return svs_map_add_keyframes(m, 1, &id, &kf, &disp, &disp_stride, h_fast_thr);
}

extern "C" int svs_map_add_keyframe(svs_map *m, const svs_map_add_keyframe_args *a, int missing_cap, svs_map_strength_result *h_res, svs_map_key *h_keys,
                                    int32_t *h_new_kept, int32_t *h_track_exists, svs_map_constraint_result *h_cons, int32_t *h_missing) {
  svs_ctx *ctx = m ? m->ctx : nullptr;
  SVS_REQUIRE(ctx, m && a && h_res && h_keys && h_cons && missing_cap >= 0 && (missing_cap == 0 || h_missing));
  const int n_new = a->n_new, n_track = a->n_track, thr = a->covis_thr, oldkey = a->oldkey_id, newkey = a->newkey_id;
  // ---- every refusal: before anything is uploaded ---------------------------------------------------------------------------------------------------------------
  std::vector<int32_t> flag;
  if (int rc = addkf_check_lists(m, n_new, a->new_points, n_track, a->track_points, thr, &flag)) return rc;
  SVS_REQUIRE(ctx, n_new == 0 || h_new_kept);
  SVS_REQUIRE(ctx, svs_map_has_keyframe(m, oldkey) && newkey >= 0);
  MAP_CAPACITY(ctx, newkey < m->max_kf);
  SVS_REQUIRE(ctx, !m->kf_in[newkey]);
  SVS_REQUIRE(ctx, a->disp && a->disp_stride > 0 && a->fast_thr);
  for (int l = 0; l < SVS_NUM_PYR_LEVELS; ++l) SVS_REQUIRE(ctx, a->keyframe.pyr[l] && a->keyframe.stride[l] > 0);
  for (int k = 0; k < THR_N; ++k) SVS_REQUIRE(ctx, a->fast_thr[k] >= 10 && a->fast_thr[k] <= 255);
  SVS_REQUIRE(ctx, a->n_cached >= 0 && (a->n_cached == 0 || (a->cached_ids && a->cached_T)));
  MAP_CAPACITY(ctx, a->n_cached <= m->max_kf);
  for (int k = 0; k < a->n_cached; ++k) SVS_REQUIRE(ctx, a->cached_ids[k] >= 0 && a->cached_ids[k] < m->max_kf && (k == 0 || a->cached_ids[k - 1] < a->cached_ids[k]));
  bool old_is_key = false;
  {
    const uint32_t st = m->next_stamp();
    for (int i = 0; i < n_new; ++i) {
      const svs_map_new_point &p = a->new_points[i];
      SVS_REQUIRE(ctx, p.point_id >= 0);
      MAP_CAPACITY(ctx, p.point_id < m->max_pt);
      SVS_REQUIRE(ctx, !m->pt_in[p.point_id] && m->stamp[p.point_id] != st);
      m->stamp[p.point_id] = st;
      SVS_REQUIRE(ctx, p.anchor_level >= 0 && p.anchor_level < SVS_NUM_PYR_LEVELS && p.feat_level >= 0 && p.feat_level < SVS_NUM_PYR_LEVELS);
      old_is_key |= p.anchor_id == oldkey;
    }
    for (int i = 0; i < n_track; ++i) {
      const svs_map_track_point &t = a->track_points[i];
      SVS_REQUIRE(ctx, t.level >= 0 && t.level < SVS_NUM_PYR_LEVELS);
      SVS_REQUIRE(ctx, t.global_id < 0 || t.global_id >= m->max_pt || m->stamp[t.global_id] != st);
      if (flag[(size_t)i] & 1) old_is_key |= m->pairs.count(((uint64_t)(uint32_t)t.global_id << 32) | (uint32_t)oldkey) != 0;
    }
  }
  SVS_REQUIRE(ctx, old_is_key);                                   // (the reference asserts, :165)
  const int edge_bound = std::min(m->n_kf, AK_MAX_KEYS);
  MAP_CAPACITY(ctx, (size_t)m->n_obs + 2 * (size_t)n_new + (size_t)n_track <= (size_t)m->max_obs);
  MAP_CAPACITY(ctx, m->max_edges > 0 && (size_t)m->n_edges + (size_t)edge_bound <= (size_t)m->max_edges);
  SVS_DEVICE(ctx);
  // ---- room for both blocks in both directions: nothing is reallocated between the two uploads -------------------------------------------------------------------
  if (!m->d_meas) SVS_HIP(ctx, m->d_meas.alloc((size_t)m->max_obs));
  const AddkfBlocks B = addkf_blocks(sizeof(kf_up), n_new, n_track);
  const size_t o_edge = B.up_end, o_req = o_edge + up_align((size_t)edge_bound * sizeof(edge_up)), o_cid = o_req + up_align((size_t)edge_bound * sizeof(cons_req)),
               o_cT = o_cid + up_align((size_t)a->n_cached * sizeof(int32_t)), up_bytes = o_cT + (size_t)a->n_cached * 12 * sizeof(double);
  const size_t o_cons = B.dn_end, o_miss = o_cons + (size_t)edge_bound * sizeof(svs_map_constraint_result),
               dn_bytes = up_align(o_miss + (size_t)edge_bound * missing_cap * sizeof(int32_t));
  if (int rc = map_dn_reserve(m, dn_bytes)) return rc;
  if (int rc = map_prepare_walk(m, 1)) return rc;
  uint8_t *hs;
  if (int rc = map_stage(m, up_bytes, &hs)) return rc;
  // ---- the first block: the keyframe record | new points | track points | flags; the strength kernel; the small download -------------------------------------------
  {
    kf_up &u = *reinterpret_cast<kf_up *>(hs);
    u.id = newkey; u.disp_stride = a->disp_stride; u.disp = a->disp; u.kf = a->keyframe; u.kf.pad_ = 0;
    memset(u.kf.T_anchor_from_w, 0, sizeof u.kf.T_anchor_from_w);
    memcpy(u.thr, a->fast_thr, sizeof u.thr);
  }
  if (int rc = addkf_strength(m, B, n_new, a->new_points, n_track, a->track_points, flag, thr, a->half_width, a->half_height, oldkey, true)) return rc;
  addkf_outputs(m, B, flag, h_res, h_keys, h_track_exists);
  const svs_map_strength_result R = *h_res;
  const int32_t *kept = reinterpret_cast<const int32_t *>(m->h_dn.get() + B.o_kept);
  for (int i = 0; i < n_new; ++i) h_new_kept[i] = R.over_capacity ? 0 : kept[i];
  if (R.over_capacity) return SVS_OK;                             // the map unchanged
  if (R.n_edges > edge_bound) { ctx->err = "svs_map_add_keyframe: the device found more edges than the map has keyframes"; return SVS_ERR_CAPACITY; }
  // ---- the host's mirrors ------------------------------------------------------------------------------------------------------------------------------------------
  const int log0 = m->n_obs, meas0 = m->n_meas, slot0 = m->n_edges, n_e = R.n_edges;
  int n_pairs = 0;
  {
    m->kf_in[newkey] = 1;
    MapRootView &v = m->kf_view[newkey];
    for (int l = 0; l < SVS_NUM_PYR_LEVELS; ++l) { v.pyr[l] = a->keyframe.pyr[l]; v.stride[l] = a->keyframe.stride[l]; }
    v.disp = a->disp; v.disp_stride = a->disp_stride;
    m->kf_hi = std::max(m->kf_hi, newkey + 1); ++m->n_kf;
    auto pair_in = [&](int p, int k) { m->pairs.insert(((uint64_t)(uint32_t)p << 32) | (uint32_t)k); ++m->kf_nobs[k]; ++n_pairs; };
    for (int i = 0; i < n_new; ++i) {
      if (!kept[i]) continue;
      const svs_map_new_point &p = a->new_points[i];
      m->pt_in[p.point_id] = 1; m->pt_hi = std::max(m->pt_hi, p.point_id + 1); ++m->n_pt;
      pair_in(p.point_id, newkey); pair_in(p.point_id, p.anchor_id);
    }
    for (int i = 0; i < n_track; ++i) if (flag[(size_t)i] & 2) pair_in(a->track_points[i].global_id, newkey);
    m->n_obs += n_pairs; m->n_meas += n_pairs;
    m->win_valid = false;
  }
  // ---- the second block, integers: the edge records | the constraint requests | the cached ids and poses ----------------------------------------------------------------
  size_t n_rows = 0;
  {
    edge_up *eu = reinterpret_cast<edge_up *>(hs + o_edge);
    cons_req *cr = reinterpret_cast<cons_req *>(hs + o_req);
    int e = 0;
    for (int r = 0; r < R.n_keys; ++r) {
      if (!h_keys[r].edge) continue;
      const int key = h_keys[r].kf_id;
      eu[e].slot = slot0 + e; eu[e].lo = std::min(key, newkey); eu[e].hi = std::max(key, newkey); eu[e].strength = h_keys[r].strength; eu[e].type = 0; eu[e].pad_ = 0;
      cons_req u{};
      u.kf1 = key; u.kf2 = newkey; u.slot = slot0 + e; u.slot_inv = key > newkey ? 1 : 0;
      u.n_cached = a->n_cached; u.cached_off = 0; u.row_off = (long long)n_rows;
      cr[e] = u;
      n_rows += (size_t)m->kf_nobs[key];
      m->edge_slot[edge_key(key, newkey)] = slot0 + e; m->edge_marg[(size_t)slot0 + e] = 0;
      ++e;
    }
    m->n_edges += n_e;
    if (a->n_cached) { memcpy(hs + o_cid, a->cached_ids, (size_t)a->n_cached * sizeof(int32_t)); memcpy(hs + o_cT, a->cached_T, (size_t)a->n_cached * 12 * sizeof(double)); }
  }
  uint8_t *U = m->d_up.get();
  if (up_bytes > o_edge) {
    SVS_HIP(ctx, hipMemcpyAsync(U + o_edge, hs + o_edge, up_bytes - o_edge, hipMemcpyHostToDevice, ctx->stream));
    SVS_HIP(ctx, hipEventRecord(m->up_ev, ctx->stream));
    m->up_pending = true;
  }
  // ---- apply: the keyframe, the points and pairs, the edges ----------------------------------------------------------------------------------------------------------
  {
    const MapK M = m->view();
    hipLaunchKernelGGL(map_scatter_kf_kernel, dim3(1), dim3(256), 0, ctx->stream, M, reinterpret_cast<const kf_up *>(U), 1);
    MapApplyK A{};
    A.np = reinterpret_cast<const svs_map_new_point *>(U + B.o_np); A.tp = reinterpret_cast<const svs_map_track_point *>(U + B.o_tp);
    A.tflag = reinterpret_cast<const int32_t *>(U + B.o_flag); A.kept = reinterpret_cast<const int32_t *>(m->d_dn.get() + B.o_kept);
    A.n_new = n_new; A.n_track = n_track; A.oldkey = oldkey; A.newkey = newkey;
    memcpy(A.T_rel, a->T_newkey_from_oldkey, sizeof A.T_rel);
    A.log_tail = m->d_log.get() + log0; A.meas_tail = m->d_meas.get() + meas0;
    hipLaunchKernelGGL(map_addkf_apply_kernel, dim3(1), dim3(MB_THREADS), 0, ctx->stream, M, A);
    if (n_e) hipLaunchKernelGGL(map_edge_add_kernel, dim3(div_up(n_e, 4)), dim3(256), 0, ctx->stream, m->d_edges.get(), reinterpret_cast<const edge_up *>(U + o_edge), n_e);
    SVS_LAUNCH_CHECK(ctx);
  }
  if (n_e == 0) { SVS_HIP(ctx, hipStreamSynchronize(ctx->stream)); return SVS_OK; }
  // ---- computeConstraint(key, newkey) + setConstraint per new edge: the CSR rebuild, the unchanged kernel, the final download ------------------------------------------
  if (m->d_depth.bytes() < std::max<size_t>(n_rows, 1) * sizeof(double)) {
    SVS_HIP(ctx, hipStreamSynchronize(ctx->stream));
    const size_t want = std::max<size_t>(n_rows * 2, 4096);
    SVS_HIP(ctx, m->d_depth.alloc(want));
    SVS_HIP(ctx, m->d_common.alloc(want));
  }
  if (int rc = map_prepare_walk(m, n_e)) return rc;
  MapConsK C{};
  C.req = reinterpret_cast<const cons_req *>(U + o_req); C.cached_ids = reinterpret_cast<const int32_t *>(U + o_cid); C.cached_T = reinterpret_cast<const double *>(U + o_cT);
  C.res = reinterpret_cast<svs_map_constraint_result *>(m->d_dn.get() + o_cons); C.missing = reinterpret_cast<int32_t *>(m->d_dn.get() + o_miss); C.missing_cap = missing_cap;
  C.depth = m->d_depth; C.common = m->d_common; C.edges = m->d_edges;
  hipLaunchKernelGGL(map_cons_kernel, dim3(n_e), dim3(MB_THREADS), 0, ctx->stream, m->view(), C);
  SVS_LAUNCH_CHECK(ctx);
  const size_t got = o_miss + (size_t)n_e * missing_cap * sizeof(int32_t) - o_cons;
  SVS_HIP(ctx, hipMemcpyAsync(m->h_dn.get() + o_cons, m->d_dn.get() + o_cons, got, hipMemcpyDeviceToHost, ctx->stream));
  SVS_HIP(ctx, hipStreamSynchronize(ctx->stream));
  memcpy(h_cons, m->h_dn.get() + o_cons, (size_t)n_e * sizeof(svs_map_constraint_result));
  if (missing_cap) memcpy(h_missing, m->h_dn.get() + o_miss, (size_t)n_e * missing_cap * sizeof(int32_t));
  for (int e = 0; e < n_e; ++e)
    if (h_cons[e].status == SVS_CONS_OK) { m->edge_marg[(size_t)slot0 + e] = 1; ++m->n_marg; }
  return SVS_OK;
}

extern "C" int svs_map_get_points(svs_map *m, int n, const int32_t *h_ids, svs_candidate_point *h_out) {
  svs_ctx *ctx = m ? m->ctx : nullptr;
  SVS_REQUIRE(ctx, m && n >= 0 && (n == 0 || (h_ids && h_out)));
  for (int i = 0; i < n; ++i) SVS_REQUIRE(ctx, h_ids[i] >= 0 && h_ids[i] < m->max_pt && m->pt_in[h_ids[i]]);
  if (n == 0) return SVS_OK;
  SVS_DEVICE(ctx);
  const size_t bytes = (size_t)n * sizeof(svs_candidate_point);
  if (int rc = map_dn_reserve(m, bytes)) return rc;
  uint8_t *hs;
  if (int rc = map_stage(m, (size_t)n * sizeof(int32_t), &hs)) return rc;
  memcpy(hs, h_ids, (size_t)n * sizeof(int32_t));
  if (int rc = map_upload(m, m->d_up, (size_t)n * sizeof(int32_t))) return rc;
  hipLaunchKernelGGL(map_get_points_kernel, dim3(div_up(n, 256)), dim3(256), 0, ctx->stream, m->view(), reinterpret_cast<const int32_t *>(m->d_up.get()), n,
                     reinterpret_cast<svs_candidate_point *>(m->d_dn.get()));
  SVS_LAUNCH_CHECK(ctx);
  SVS_HIP(ctx, hipMemcpyAsync(m->h_dn, m->d_dn, bytes, hipMemcpyDeviceToHost, ctx->stream));
  SVS_HIP(ctx, hipStreamSynchronize(ctx->stream));
  memcpy(h_out, m->h_dn.get(), bytes);
  return SVS_OK;
}

extern "C" int svs_map_get_feature_table(svs_map *m, int32_t kf_id, int cap, int32_t *h_count, int32_t *h_point_ids, svs_ba_edge *h_meas) {
  svs_ctx *ctx = m ? m->ctx : nullptr;
  SVS_REQUIRE(ctx, m && h_count && cap >= 0 && (cap == 0 || (h_point_ids && h_meas)) && svs_map_has_keyframe(m, kf_id));
  MAP_CAPACITY(ctx, cap <= m->max_pt);
  SVS_DEVICE(ctx);
  const size_t o_ids = 16, o_rec = o_ids + up_align((size_t)cap * sizeof(int32_t)), bytes = o_rec + (size_t)cap * sizeof(svs_ba_edge);
  if (int rc = map_dn_reserve(m, bytes)) return rc;
  if (int rc = map_prepare_walk(m, 1)) return rc;
  MapFtK A{};
  A.kf = kf_id; A.cap = cap; A.n_meas = m->n_meas; A.meas = m->d_meas;
  A.count = reinterpret_cast<int32_t *>(m->d_dn.get()); A.ids = reinterpret_cast<int32_t *>(m->d_dn.get() + o_ids); A.rec = reinterpret_cast<svs_ba_edge *>(m->d_dn.get() + o_rec);
  hipLaunchKernelGGL(map_feature_table_kernel, dim3(1), dim3(MB_THREADS), 0, ctx->stream, m->view(), A);
  SVS_LAUNCH_CHECK(ctx);
  SVS_HIP(ctx, hipMemcpyAsync(m->h_dn, m->d_dn, bytes, hipMemcpyDeviceToHost, ctx->stream));
  SVS_HIP(ctx, hipStreamSynchronize(ctx->stream));
  const int n = *reinterpret_cast<const int32_t *>(m->h_dn.get()), n_c = std::min(n, cap);
  *h_count = n;
  for (int i = 0; i < cap; ++i) h_point_ids[i] = i < n_c ? reinterpret_cast<const int32_t *>(m->h_dn.get() + o_ids)[i] : -1;
  if (cap) { memcpy(h_meas, m->h_dn.get() + o_rec, (size_t)n_c * sizeof(svs_ba_edge)); memset(h_meas + n_c, 0, (size_t)(cap - n_c) * sizeof(svs_ba_edge)); }
  return SVS_OK;
}
