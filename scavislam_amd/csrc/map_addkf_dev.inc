// map_addkf_dev.inc -- svs_map_add_keyframe with the two lists in DEVICE memory (svs_map_add_keyframe_dev), included by map.hip behind map_addkf.inc.  The list
// records never cross the bus: what the host-list call decides about them on the host (addkf_check_lists and the loops in front of its first upload) is decided by
//   map_addkf_check_kernel   one workgroup in front of the unchanged map_strength_kernel: every refusal about the records as (phase, first offending index,
//                            status), the track flags, and the id columns the host's mirrors need (point_id / anchor_id per new entry, global_id per track entry).
//                            "Twice in the list" and "first occurrence" are an atomicMin of the list index into a row over point ids (svs_map::d_first, FIRST_NONE
//                            between calls: the kernel restores every entry it touched), compared afterwards: no arrival order decides anything.  The records may hold
//                            any bits: every id is range-checked before it indexes anything.
//   map_member_add_kernel    the kept points and the new keyframe join the device's id sets.
// The id sets (svs_map::d_in_pt / d_in_kf: bitmaps over ids) mirror the host's kf_in / pt_in.  The sets only grow and every path that grows them counts in n_kf /
// n_pt, so they are current iff they were written at these two counts; otherwise they are uploaded whole (a map that is only fed through this call never does).
namespace {
constexpr int FIRST_NONE = 0x7f7f7f7f;      // above every list index (< 2^24); a hipMemset pattern
enum { CHK_ANCHORS = 1, CHK_NEW = 2, CHK_TRACK = 3, CHK_OLDKEY = 4 };      // the phases, in the order the host-list call meets them

struct MapChkK {
  const svs_map_new_point *np; const svs_map_track_point *tp;
  int n_new, n_track, oldkey, max_pt;
  const uint32_t *in_pt, *in_kf;       // [ceil(max_pt / 32)], [MAP_KF_WORDS]
  int32_t *first;                      // [max_pt], FIRST_NONE
  MapObsView obs;
  int4 *status;                        // status (SVS_OK: none), phase, index of the first offending entry (-1: CHK_OLDKEY), 0
  int32_t *new_pid, *new_anchor, *track_gid, *tflag;
};

__device__ __forceinline__ int first_load(const int32_t *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void first_reset(int32_t *p) { __hip_atomic_store(p, FIRST_NONE, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
// a barrier that also orders this workgroup's atomics and stores on A.first
__device__ __forceinline__ void chk_barrier() { __threadfence(); __syncthreads(); }

__global__ __launch_bounds__(MB_THREADS) void map_addkf_check_kernel(MapChkK A) {
  __shared__ int s_off[3];             // per list phase: the least offending key (CHK_NEW: index << 2 | status)
  __shared__ int s_old;
  const int tid = threadIdx.x;
  const unsigned max_pt = (unsigned)A.max_pt;
  if (tid < 3) s_off[tid] = 0x7fffffff;
  if (tid == 0) s_old = 0;
  __syncthreads();
  // 1. the id columns; the anchors; every new id in range leaves its least list index
  bool old_mine = false;
  for (int i = tid; i < A.n_new; i += MB_THREADS) {
    const int id = A.np[i].point_id, a = A.np[i].anchor_id;
    A.new_pid[i] = id; A.new_anchor[i] = a;
    if (!((unsigned)a < (unsigned)MAP_MAX_KF && bit_of(A.in_kf, a))) atomicMin(&s_off[0], i);
    old_mine |= a == A.oldkey;
    if ((unsigned)id < max_pt) atomicMin(&A.first[id], i);
  }
  for (int i = tid; i < A.n_track; i += MB_THREADS) A.track_gid[i] = A.tp[i].global_id;
  chk_barrier();
  // 2. the new entries (slam_graph.cpp:369-397 asks for none of this: the map's own rules); the track entries against the new ids
  for (int i = tid; i < A.n_new; i += MB_THREADS) {
    const int id = A.np[i].point_id, la = A.np[i].anchor_level, lf = A.np[i].feat_level;
    int code = SVS_OK;
    if (id < 0) code = SVS_ERR_INVALID;
    else if ((unsigned)id >= max_pt) code = SVS_ERR_CAPACITY;
    else if (bit_of(A.in_pt, id) || first_load(&A.first[id]) < i) code = SVS_ERR_INVALID;
    else if ((unsigned)la >= (unsigned)SVS_NUM_PYR_LEVELS || (unsigned)lf >= (unsigned)SVS_NUM_PYR_LEVELS) code = SVS_ERR_INVALID;
    if (code != SVS_OK) atomicMin(&s_off[1], (i << 2) | (code == SVS_ERR_CAPACITY ? 1 : 0));
  }
  for (int i = tid; i < A.n_track; i += MB_THREADS) {
    const int g = A.tp[i].global_id, l = A.tp[i].level;
    if ((unsigned)l >= (unsigned)SVS_NUM_PYR_LEVELS || ((unsigned)g < max_pt && first_load(&A.first[g]) != FIRST_NONE)) atomicMin(&s_off[2], i);
  }
  chk_barrier();
  for (int i = tid; i < A.n_new; i += MB_THREADS) { const int id = A.np[i].point_id; if ((unsigned)id < max_pt) first_reset(&A.first[id]); }
  chk_barrier();
  // 3. E = the track entries that name a point of the map; the first occurrence of an id is the entry of least index
  for (int i = tid; i < A.n_track; i += MB_THREADS) {
    const int g = A.tp[i].global_id;
    if ((unsigned)g < max_pt && bit_of(A.in_pt, g)) atomicMin(&A.first[g], i);
  }
  chk_barrier();
  for (int i = tid; i < A.n_track; i += MB_THREADS) {
    const int g = A.tp[i].global_id;
    const bool in_e = (unsigned)g < max_pt && bit_of(A.in_pt, g);
    A.tflag[i] = !in_e ? 0 : first_load(&A.first[g]) == i ? 3 : 1;
    if (in_e && !old_mine) old_mine = map_point_seen_by(A.obs, g, A.oldkey);
  }
  if (old_mine) s_old = 1;
  chk_barrier();
  for (int i = tid; i < A.n_track; i += MB_THREADS) { const int g = A.tp[i].global_id; if ((unsigned)g < max_pt && bit_of(A.in_pt, g)) first_reset(&A.first[g]); }
  if (tid == 0) {
    int4 st = make_int4(SVS_OK, 0, -1, 0);
    if (s_off[0] != 0x7fffffff) st = make_int4(SVS_ERR_INVALID, CHK_ANCHORS, s_off[0], 0);
    else if (s_off[1] != 0x7fffffff) st = make_int4((s_off[1] & 1) ? SVS_ERR_CAPACITY : SVS_ERR_INVALID, CHK_NEW, s_off[1] >> 2, 0);
    else if (s_off[2] != 0x7fffffff) st = make_int4(SVS_ERR_INVALID, CHK_TRACK, s_off[2], 0);
    else if (!s_old) st = make_int4(SVS_ERR_INVALID, CHK_OLDKEY, -1, 0);
    *A.status = st;
  }
}

__global__ __launch_bounds__(256) void map_member_add_kernel(uint32_t *in_pt, uint32_t *in_kf, const int32_t *new_pid, const int32_t *kept, int n_new, int newkey) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < n_new && kept[i]) bit_set(in_pt, new_pid[i]);            // (ids the check kernel passed)
  if (i == 0) bit_set(in_kf, newkey);
}
}  // namespace

// the device's id sets and the scratch row, current with the host's
static int map_sync_sets(svs_map *m) {
  svs_ctx *ctx = m->ctx;
  const size_t pw = ((size_t)m->max_pt + 31) / 32;
  if (!m->d_in_pt) {
    SVS_HIP(ctx, m->d_in_pt.alloc(pw));
    SVS_HIP(ctx, m->d_in_kf.alloc((size_t)MAP_KF_WORDS));
    SVS_HIP(ctx, m->d_first.alloc((size_t)m->max_pt));
    SVS_HIP(ctx, m->h_in.alloc(pw + MAP_KF_WORDS));
    SVS_HIP(ctx, hipMemsetAsync(m->d_first, FIRST_NONE & 0xff, (size_t)m->max_pt * sizeof(int32_t), ctx->stream));
    m->in_n_kf = m->in_n_pt = -1;
  }
  if (m->in_n_kf == m->n_kf && m->in_n_pt == m->n_pt) return SVS_OK;
  uint32_t *hp = m->h_in.get(), *hk = hp + pw;
  memset(hp, 0, (pw + MAP_KF_WORDS) * sizeof(uint32_t));
  for (int p = 0; p < m->pt_hi; ++p) if (m->pt_in[p]) hp[p >> 5] |= 1u << (p & 31);
  for (int k = 0; k < m->kf_hi; ++k) if (m->kf_in[k]) hk[k >> 5] |= 1u << (k & 31);
  SVS_HIP(ctx, hipMemcpyAsync(m->d_in_pt, hp, pw * sizeof(uint32_t), hipMemcpyHostToDevice, ctx->stream));
  SVS_HIP(ctx, hipMemcpyAsync(m->d_in_kf, hk, MAP_KF_WORDS * sizeof(uint32_t), hipMemcpyHostToDevice, ctx->stream));
  SVS_HIP(ctx, hipStreamSynchronize(ctx->stream));                 // (the pinned block is free again; a map fed through this call alone comes here once)
  m->in_n_kf = m->n_kf; m->in_n_pt = m->n_pt;
  return SVS_OK;
}

int svs_map_add_keyframe_lists(svs_map *m, const svs_map_add_keyframe_args *a, const MapKeyframeLists &L, int missing_cap, svs_map_strength_result *h_res,
                               svs_map_key *h_keys, int32_t *h_new_kept, int32_t *h_track_exists, svs_map_constraint_result *h_cons, int32_t *h_missing) {
  svs_ctx *ctx = m ? m->ctx : nullptr;
  SVS_REQUIRE(ctx, m && a && h_res && h_keys && h_cons && missing_cap >= 0 && (missing_cap == 0 || h_missing));
  const svs_map_new_point *const d_new = L.d_new;
  const svs_map_track_point *const d_track = L.d_track;
  const int32_t *const fast_thr = L.h_thr_late ? L.h_thr_late : a->fast_thr;
  const int n_new = a->n_new, n_track = a->n_track, thr = a->covis_thr, oldkey = a->oldkey_id, newkey = a->newkey_id;
  // ---- what the arguments and the map's counts decide: before anything runs ----------------------------------------------------------------------------------------
  SVS_REQUIRE(ctx, thr >= 0 && n_new >= 0 && n_track >= 0 && (n_new == 0 || d_new) && (n_track == 0 || d_track));
  MAP_CAPACITY(ctx, n_new < (1 << 24) && n_track < (1 << 24));
  SVS_REQUIRE(ctx, n_new == 0 || h_new_kept);
  SVS_REQUIRE(ctx, svs_map_has_keyframe(m, oldkey) && newkey >= 0);
  MAP_CAPACITY(ctx, newkey < m->max_kf);
  SVS_REQUIRE(ctx, !m->kf_in[newkey]);
  SVS_REQUIRE(ctx, a->disp && a->disp_stride > 0 && fast_thr);
  for (int l = 0; l < SVS_NUM_PYR_LEVELS; ++l) SVS_REQUIRE(ctx, a->keyframe.pyr[l] && a->keyframe.stride[l] > 0);
  if (!L.h_thr_late)
    for (int k = 0; k < THR_N; ++k) SVS_REQUIRE(ctx, fast_thr[k] >= 10 && fast_thr[k] <= 255);
  SVS_REQUIRE(ctx, a->n_cached >= 0 && (a->n_cached == 0 || (a->cached_ids && a->cached_T)));
  MAP_CAPACITY(ctx, a->n_cached <= m->max_kf);
  for (int k = 0; k < a->n_cached; ++k) SVS_REQUIRE(ctx, a->cached_ids[k] >= 0 && a->cached_ids[k] < m->max_kf && (k == 0 || a->cached_ids[k - 1] < a->cached_ids[k]));
  const int edge_bound = std::min(m->n_kf, AK_MAX_KEYS);
  MAP_CAPACITY(ctx, (size_t)m->n_obs + 2 * (size_t)n_new + (size_t)n_track <= (size_t)m->max_obs);
  MAP_CAPACITY(ctx, m->max_edges > 0 && (size_t)m->n_edges + (size_t)edge_bound <= (size_t)m->max_edges);
  SVS_DEVICE(ctx);
  // ---- room: the download block (status | id columns | flags | result | keys | kept || constraints | missing), the block of integers that goes up ---------------------
  if (!m->d_meas) SVS_HIP(ctx, m->d_meas.alloc((size_t)m->max_obs));
  MapDn dn(m);
  const auto status = dn.piece<int4>(1);
  const auto new_pid = dn.piece<int32_t>(n_new);
  const auto new_anchor = dn.piece<int32_t>(n_new);
  const auto track_gid = dn.piece<int32_t>(n_track);
  const auto flag = dn.piece<int32_t>(n_track);
  const auto res = dn.piece<svs_map_strength_result>(1);
  const auto keys = dn.piece<svs_map_key>(AK_MAX_KEYS);
  const auto kept_p = dn.piece<int32_t>(n_new);
  const size_t dn_first = dn.end_aligned();
  const auto cons = dn.piece<svs_map_constraint_result>(edge_bound);
  const auto missing = dn.piece<int32_t>((size_t)edge_bound * missing_cap);
  MapUp up(m);
  const auto kf = up.piece<kf_up>(1);
  const auto edges = up.piece<edge_up>(edge_bound);
  const auto reqs = up.piece<cons_req>(edge_bound);
  const auto cached_ids = up.piece<int32_t>(a->n_cached);
  const auto cached_T = up.piece<double>(12 * (size_t)a->n_cached);
  if (int rc = dn.reserve(dn.end_aligned())) return rc;
  if (int rc = map_prepare_walk(m, 1)) return rc;
  if (int rc = up.reserve()) return rc;
  if (int rc = map_sync_sets(m)) return rc;
  // ---- the check kernel, the strength kernel, the one download: both kernels read the map and write scratch ---------------------------------------------------------
  {
    MapChkK K{};
    K.np = d_new; K.tp = d_track; K.n_new = n_new; K.n_track = n_track; K.oldkey = oldkey; K.max_pt = m->max_pt;
    K.in_pt = m->d_in_pt; K.in_kf = m->d_in_kf; K.first = m->d_first;
    K.obs.pt_begin = m->d_pt_begin; K.obs.pt_rows = m->d_pt_rows; K.obs.pt_hi = m->pt_hi;
    K.status = dn.dev(status); K.new_pid = dn.dev(new_pid); K.new_anchor = dn.dev(new_anchor); K.track_gid = dn.dev(track_gid); K.tflag = dn.dev(flag);
    hipLaunchKernelGGL(map_addkf_check_kernel, dim3(1), dim3(MB_THREADS), 0, ctx->stream, K);
    MapStrK A{};
    A.np = d_new; A.tp = d_track; A.tflag = dn.dev(flag);
    A.n_new = n_new; A.n_track = n_track; A.thr = thr; A.half_w = a->half_width; A.half_h = a->half_height; A.oldkey = oldkey; A.clamp = 1;
    A.res = dn.dev(res); A.keys = dn.dev(keys); A.kept = dn.dev(kept_p);
    hipLaunchKernelGGL(map_strength_kernel, dim3(1), dim3(MB_THREADS), 0, ctx->stream, m->view(), A);
    SVS_LAUNCH_CHECK(ctx);
    if (int rc = dn.download(0, dn_first)) return rc;
  }
  // ---- the refusals about the records: the map and its mirrors are as they were -------------------------------------------------------------------------------------
  if (L.h_thr_late)                                               // (they came with the download)
    for (int k = 0; k < THR_N; ++k) SVS_REQUIRE(ctx, fast_thr[k] >= 10 && fast_thr[k] <= 255);
  {
    const int4 st = *dn.host(status);
    if (st.x != SVS_OK) {
      static const char *const what[] = {"", "an anchor_id that is no keyframe of the map", "a new point: id out of range, already a point, twice in the list, or a level out of range",
                                         "a track point: a level out of range, or an id that is a new point of the call", "oldkey is no key of the table"};
      char buf[512];
      snprintf(buf, sizeof buf, "svs_map_add_keyframe_dev: %s (entry %d)", what[std::min(std::max(st.y, 0), 4)], st.z);
      ctx->err = buf;
      return st.x == SVS_ERR_CAPACITY ? SVS_ERR_CAPACITY : SVS_ERR_INVALID;
    }
  }
  const int32_t *h_pid = dn.host(new_pid), *h_anchor = dn.host(new_anchor), *h_gid = dn.host(track_gid), *h_flag = dn.host(flag), *kept = dn.host(kept_p);
  const svs_map_strength_result R = *dn.host(res);
  *h_res = R;
  if (R.over_capacity) memset(h_keys, 0, (size_t)AK_MAX_KEYS * sizeof(svs_map_key));
  else dn.get(keys, h_keys);
  if (h_track_exists)
    for (int i = 0; i < n_track; ++i) h_track_exists[i] = R.over_capacity ? 0 : (h_flag[i] & 1);
  for (int i = 0; i < n_new; ++i) h_new_kept[i] = R.over_capacity ? 0 : kept[i];
  if (R.over_capacity) return SVS_OK;                             // the map unchanged
  if (R.n_edges > edge_bound) { ctx->err = "svs_map_add_keyframe_dev: the device found more edges than the map has keyframes"; return SVS_ERR_CAPACITY; }
  // ---- the host's mirrors, from the id columns -----------------------------------------------------------------------------------------------------------------------
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
      m->pt_in[h_pid[i]] = 1; m->pt_hi = std::max(m->pt_hi, h_pid[i] + 1); ++m->n_pt;
      pair_in(h_pid[i], newkey); pair_in(h_pid[i], h_anchor[i]);
    }
    for (int i = 0; i < n_track; ++i) if (h_flag[i] & 2) pair_in(h_gid[i], newkey);
    m->n_obs += n_pairs; m->n_meas += n_pairs;
    m->win_valid = false;
  }
  // ---- the block of integers: the keyframe record | the edge records | the constraint requests | the cached ids and poses ---------------------------------------------
  size_t n_rows = 0;
  {
    kf_up &u = *up.host(kf);
    u.id = newkey; u.disp_stride = a->disp_stride; u.disp = a->disp; u.kf = a->keyframe; u.kf.pad_ = 0;
    memset(u.kf.T_anchor_from_w, 0, sizeof u.kf.T_anchor_from_w);
    memcpy(u.thr, fast_thr, sizeof u.thr);
    edge_up *eu = up.host(edges);
    cons_req *cr = up.host(reqs);
    int e = 0;
    for (int r = 0; r < R.n_keys; ++r) {
      if (!h_keys[r].edge) continue;
      const int key = h_keys[r].kf_id;
      eu[e].slot = slot0 + e; eu[e].lo = std::min(key, newkey); eu[e].hi = std::max(key, newkey); eu[e].strength = h_keys[r].strength; eu[e].type = 0; eu[e].pad_ = 0;
      cons_req q{};
      q.kf1 = key; q.kf2 = newkey; q.slot = slot0 + e; q.slot_inv = key > newkey ? 1 : 0;
      q.n_cached = a->n_cached; q.cached_off = 0; q.row_off = (long long)n_rows;
      cr[e] = q;
      n_rows += (size_t)m->kf_nobs[key];
      m->edge_slot[edge_key(key, newkey)] = slot0 + e; m->edge_marg[(size_t)slot0 + e] = 0;
      ++e;
    }
    m->n_edges += n_e;
    up.put(cached_ids, a->cached_ids); up.put(cached_T, a->cached_T);
  }
  if (int rc = up.upload()) return rc;
  // ---- apply: the keyframe, the points and pairs, the id sets, the edges ---------------------------------------------------------------------------------------------
  {
    const MapK M = m->view();
    hipLaunchKernelGGL(map_scatter_kf_kernel, dim3(1), dim3(256), 0, ctx->stream, M, up.dev(kf), 1);
    MapApplyK A{};
    A.np = d_new; A.tp = d_track; A.tflag = dn.dev(flag); A.kept = dn.dev(kept_p);
    A.n_new = n_new; A.n_track = n_track; A.oldkey = oldkey; A.newkey = newkey;
    memcpy(A.T_rel, L.h_T_late ? L.h_T_late : a->T_newkey_from_oldkey, sizeof A.T_rel);
    A.log_tail = m->d_log.get() + log0; A.meas_tail = m->d_meas.get() + meas0;
    hipLaunchKernelGGL(map_addkf_apply_kernel, dim3(1), dim3(MB_THREADS), 0, ctx->stream, M, A);
    hipLaunchKernelGGL(map_member_add_kernel, dim3(std::max(div_up(n_new, 256), 1)), dim3(256), 0, ctx->stream, m->d_in_pt.get(), m->d_in_kf.get(), dn.dev(new_pid),
                       dn.dev(kept_p), n_new, newkey);
    if (n_e) hipLaunchKernelGGL(map_edge_add_kernel, dim3(div_up(n_e, 4)), dim3(256), 0, ctx->stream, m->d_edges.get(), up.dev(edges), n_e);
    SVS_LAUNCH_CHECK(ctx);
    m->in_n_kf = m->n_kf; m->in_n_pt = m->n_pt;
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
  if (int rc = dn.download(cons.off, missing.off + (size_t)n_e * missing_cap * sizeof(int32_t))) return rc;
  memcpy(h_cons, dn.host(cons), (size_t)n_e * sizeof(svs_map_constraint_result));
  if (missing_cap) memcpy(h_missing, dn.host(missing), (size_t)n_e * missing_cap * sizeof(int32_t));
  for (int e = 0; e < n_e; ++e)
    if (h_cons[e].status == SVS_CONS_OK) { m->edge_marg[(size_t)slot0 + e] = 1; ++m->n_marg; }
  return SVS_OK;
}

extern "C" int svs_map_add_keyframe_dev(svs_map *m, const svs_map_add_keyframe_args *a, const svs_map_new_point *d_new, const svs_map_track_point *d_track,
                                        int missing_cap, svs_map_strength_result *h_res, svs_map_key *h_keys, int32_t *h_new_kept, int32_t *h_track_exists,
                                        svs_map_constraint_result *h_cons, int32_t *h_missing) {
  const MapKeyframeLists L{d_new, d_track, nullptr, nullptr};
  return svs_map_add_keyframe_lists(m, a, L, missing_cap, h_res, h_keys, h_new_kept, h_track_exists, h_cons, h_missing);
}
