// map_addkf.inc -- inserting a keyframe into the resident map (SlamGraph::addKeyframe, slam_graph.cpp:143-186), included by map.hip behind map_window.inc.
//   map_strength_kernel      computeStrength (:467-552) as the closed form of include/scavislam_hip.h, one workgroup per call: the keys are an LDS bitmap over
//                            keyframe ids (new points' anchors, observer rows of the track points), popcount prefixes give the ascending key list and id -> rank,
//                            everything per key is an LDS table of 1024 entries.  t_q(f), "the index of the h-th track entry f observes in class q", is found by
//                            COUNTING, never by arrival order: x = the largest list index with fewer than h such entries in front of it, built bit by bit from the
//                            top -- one pass of integer LDS adds per bit over "entries in front of x | bit".  ceil(log2(n_track + 1)) passes whatever h is; the
//                            counts are sums of integers, so every value is a function of the input alone.
//   map_addkf_apply_kernel   addNewPointsToMap / addNewObsToOldPoints (:358-420) from the block the strength kernel read: the kept points and the kept measurement
//                            records are compacted by prefix sums into the point store, the pair log and the measured store in the order the twin calls would
//                            give them; the new keyframe's pose is pose_mul(T_newkey_from_oldkey, T_oldkey_from_world) formed here.
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
      row_each(M.pt_rows, ob[k], oe[k], [&](int kf) { if ((unsigned)kf < (unsigned)MAP_MAX_KF) f(i, lr[k], tb[k], kf); });
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
  auto rank_of = [&](int id) { return bit_rank(s_bm, s_rank, id); };
  // a. empty tables
  s_bm[tid] = 0;
  for (int r = tid; r < AK_MAX_KEYS; r += MB_THREADS) {
#pragma unroll
    for (int q = 0; q < 4; ++q) { s_cnt[q][r] = 0; s_x[q][r] = 0; }
    s_str[r] = 0; s_tstar[r] = 0;
  }
  __syncthreads();
  // b. the keys: anchors of the new points (ids the host has checked), observers of E; m = |E|
  for (int i = tid; i < A.n_new; i += MB_THREADS) { const int a = A.np[i].anchor_id; if ((unsigned)a < (unsigned)MAP_MAX_KF) bit_set(s_bm, a); }
  ak_for_each(M, A, [&](int, int, int, int kf) { bit_set(s_bm, kf); });
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
  for_each_set_bit(bits, tid << 5, rank, [&](int id, int r) {      // r < n_keys <= AK_MAX_KEYS
    int s = s_str[r];
    if (A.clamp && id == A.oldkey) s = max(s, A.thr);
    s_str[r] = s;
    const int edge = (A.clamp && s >= A.thr) ? 1 : 0;
    n_edge_mine += edge;
    svs_map_key &K = A.keys[r];
    K.kf_id = id; K.strength = s; K.edge = edge; K.pad_ = 0;
  });
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

// the first part of the two blocks: upload [the keyframe record of svs_map_add_keyframe] | new points | track points | flags; download result | keys | kept.
// svs_map_add_keyframe declares its second part behind them; up_end / dn_end are where that begins
struct AddkfBlocks {
  MapUp up; MapDn dn;
  MapPiece<kf_up> kf; MapPiece<svs_map_new_point> np; MapPiece<svs_map_track_point> tp; MapPiece<int32_t> flag;
  MapPiece<svs_map_strength_result> res; MapPiece<svs_map_key> keys; MapPiece<int32_t> kept;
  size_t up_end, dn_end;
  AddkfBlocks(svs_map *m, bool with_kf, int n_new, int n_track) : up(m), dn(m) {
    kf = up.piece<kf_up>(with_kf ? 1 : 0); np = up.piece<svs_map_new_point>(n_new); tp = up.piece<svs_map_track_point>(n_track); flag = up.piece<int32_t>(n_track);
    up_end = up.end_aligned();
    res = dn.piece<svs_map_strength_result>(1); keys = dn.piece<svs_map_key>(AK_MAX_KEYS); kept = dn.piece<int32_t>(n_new);
    dn_end = dn.end_aligned();
  }
};

// copies the lists into the staged block (the caller has reserved it and written its head), uploads, runs the strength kernel into the download block and waits
static int addkf_strength(svs_map *m, AddkfBlocks &B, const svs_map_new_point *np, const svs_map_track_point *tp, const std::vector<int32_t> &flag, int thr, int half_w,
                          int half_h, int oldkey, bool clamp) {
  svs_ctx *ctx = m->ctx;
  B.up.put(B.np, np); B.up.put(B.tp, tp); B.up.put(B.flag, flag.data());
  if (B.up_end)
    if (int rc = B.up.upload(0, B.up_end)) return rc;
  MapStrK A{};
  A.np = B.up.dev(B.np); A.tp = B.up.dev(B.tp); A.tflag = B.up.dev(B.flag);
  A.n_new = (int)B.np.n; A.n_track = (int)B.tp.n; A.thr = thr; A.half_w = half_w; A.half_h = half_h; A.oldkey = oldkey; A.clamp = clamp ? 1 : 0;
  A.res = B.dn.dev(B.res); A.keys = B.dn.dev(B.keys); A.kept = clamp ? B.dn.dev(B.kept) : nullptr;
  hipLaunchKernelGGL(map_strength_kernel, dim3(1), dim3(MB_THREADS), 0, ctx->stream, m->view(), A);
  SVS_LAUNCH_CHECK(ctx);
  return B.dn.download(0, B.dn_end);
}

// the key table and the exists mask as the caller gets them
static void addkf_outputs(const AddkfBlocks &B, const std::vector<int32_t> &flag, svs_map_strength_result *h_res, svs_map_key *h_keys, int32_t *h_exists) {
  const svs_map_strength_result R = *B.dn.host(B.res);
  *h_res = R;
  if (R.over_capacity) memset(h_keys, 0, (size_t)AK_MAX_KEYS * sizeof(svs_map_key));
  else B.dn.get(B.keys, h_keys);
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
  AddkfBlocks B(m, false, n_new, n_track);
  if (int rc = B.dn.reserve(B.dn_end)) return rc;
  if (int rc = map_prepare_walk(m, 1)) return rc;
  if (int rc = B.up.reserve(std::max<size_t>(B.up_end, 16))) return rc;
  if (int rc = addkf_strength(m, B, h_new, h_track, flag, covis_thr, half_width, half_height, -1, false)) return rc;
  addkf_outputs(B, flag, h_res, h_keys, h_track_exists);
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
  AddkfBlocks B(m, true, n_new, n_track);
  MapUp &up = B.up;
  MapDn &dn = B.dn;
  const auto edges = up.piece<edge_up>(edge_bound);
  const auto reqs = up.piece<cons_req>(edge_bound);
  const auto cached_ids = up.piece<int32_t>(a->n_cached);
  const auto cached_T = up.piece<double>(12 * (size_t)a->n_cached);
  const auto cons = dn.piece<svs_map_constraint_result>(edge_bound);
  const auto missing = dn.piece<int32_t>((size_t)edge_bound * missing_cap);
  if (int rc = dn.reserve(dn.end_aligned())) return rc;
  if (int rc = map_prepare_walk(m, 1)) return rc;
  if (int rc = up.reserve()) return rc;
  // ---- the first block: the keyframe record | new points | track points | flags; the strength kernel; the small download -------------------------------------------
  {
    kf_up &u = *up.host(B.kf);
    u.id = newkey; u.disp_stride = a->disp_stride; u.disp = a->disp; u.kf = a->keyframe; u.kf.pad_ = 0;
    memset(u.kf.T_anchor_from_w, 0, sizeof u.kf.T_anchor_from_w);
    memcpy(u.thr, a->fast_thr, sizeof u.thr);
  }
  if (int rc = addkf_strength(m, B, a->new_points, a->track_points, flag, thr, a->half_width, a->half_height, oldkey, true)) return rc;
  addkf_outputs(B, flag, h_res, h_keys, h_track_exists);
  const svs_map_strength_result R = *h_res;
  const int32_t *kept = dn.host(B.kept);
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
    edge_up *eu = up.host(edges);
    cons_req *cr = up.host(reqs);
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
    up.put(cached_ids, a->cached_ids); up.put(cached_T, a->cached_T);
  }
  if (up.end > edges.off)
    if (int rc = up.upload(edges.off, up.end)) return rc;
  // ---- apply: the keyframe, the points and pairs, the edges ----------------------------------------------------------------------------------------------------------
  {
    const MapK M = m->view();
    hipLaunchKernelGGL(map_scatter_kf_kernel, dim3(1), dim3(256), 0, ctx->stream, M, up.dev(B.kf), 1);
    MapApplyK A{};
    A.np = up.dev(B.np); A.tp = up.dev(B.tp); A.tflag = up.dev(B.flag); A.kept = dn.dev(B.kept);
    A.n_new = n_new; A.n_track = n_track; A.oldkey = oldkey; A.newkey = newkey;
    memcpy(A.T_rel, a->T_newkey_from_oldkey, sizeof A.T_rel);
    A.log_tail = m->d_log.get() + log0; A.meas_tail = m->d_meas.get() + meas0;
    hipLaunchKernelGGL(map_addkf_apply_kernel, dim3(1), dim3(MB_THREADS), 0, ctx->stream, M, A);
    if (n_e) hipLaunchKernelGGL(map_edge_add_kernel, dim3(div_up(n_e, 4)), dim3(256), 0, ctx->stream, m->d_edges.get(), up.dev(edges), n_e);
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
  C.req = up.dev(reqs); C.cached_ids = up.dev(cached_ids); C.cached_T = up.dev(cached_T);
  C.res = dn.dev(cons); C.missing = dn.dev(missing); C.missing_cap = missing_cap;
  C.depth = m->d_depth; C.common = m->d_common; C.edges = m->d_edges;
  hipLaunchKernelGGL(map_cons_kernel, dim3(n_e), dim3(MB_THREADS), 0, ctx->stream, m->view(), C);
  SVS_LAUNCH_CHECK(ctx);
  if (int rc = dn.download(cons.off, missing.off + (size_t)n_e * missing_cap * sizeof(int32_t))) return rc;      // what the n_e edges wrote of the room for edge_bound
  memcpy(h_cons, dn.host(cons), (size_t)n_e * sizeof(svs_map_constraint_result));
  if (missing_cap) memcpy(h_missing, dn.host(missing), (size_t)n_e * missing_cap * sizeof(int32_t));
  for (int e = 0; e < n_e; ++e)
    if (h_cons[e].status == SVS_CONS_OK) { m->edge_marg[(size_t)slot0 + e] = 1; ++m->n_marg; }
  return SVS_OK;
}
