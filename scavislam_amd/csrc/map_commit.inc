// map_commit.inc -- committing a registration or a loop closure into the resident map (SlamGraph::registerKeyframes, slam_graph.cpp:188-205, and addLoopClosure,
// :207-251, with addNewObsToOldPoints :400-420 and addNewEdges :423-465), included by map.hip behind map_addkf.inc.  One apply path for three callers
// (reg_map.h: MapCommit): a track list of (point id, centre, level) records ON THE DEVICE -- left there by svs_reg_commit's kernel (register.hip) or staged by the
// explicit calls -- plus an edge list on the host.  The structure is svs_map_add_keyframe's: the host decides every refusal and the mask of new pairs from its
// mirrors, one staged block of integers goes up, the new pairs are appended by prefix sums, the edges go through map_edge_add_kernel and their constraints
// through map_cons_kernel with the pose override, one download.
namespace {
struct MapCommitK { const svs_map_track_point *tp; const int32_t *mask; int n_track, kf; int2 *log_tail; svs_ba_edge *meas_tail; };

// one workgroup: the masked track entries, in list order, to the tails of the pair log and the measured store (the record svs_map_add_measured_observations
// forms, slam_graph.cpp:1010-1015).  The host has counted the mask: every position is below the room it reserved
__global__ __launch_bounds__(MB_THREADS) void map_commit_append_kernel(MapCommitK A) {
  __shared__ int s_w[MB_THREADS / 64];
  const int tid = threadIdx.x;
  int n = 0;
  for (int i0 = 0; i0 < A.n_track; i0 += MB_THREADS) {            // block-uniform
    const int i = i0 + tid;
    const bool c = i < A.n_track && A.mask[i] != 0;
    int tot;
    const int pos = n + block_excl_scan(c ? 1 : 0, s_w, tot);
    if (c) {
      const svs_map_track_point t = A.tp[i];
      const double s = 1.0 / (double)(1 << t.level);
      svs_ba_edge e;
      e.obs[0] = t.center[0]; e.obs[1] = t.center[1]; e.obs[2] = t.center[2];
      e.info[0] = s * s; e.info[1] = s * s; e.info[2] = 0.333 * 0.333;
      e.point = t.global_id; e.pose = A.kf; e.anchor = 0; e.pad_ = 0;
      A.meas_tail[pos] = e;
      A.log_tail[pos] = make_int2(t.global_id, A.kf);
    }
    n += tot;
  }
}
}  // namespace

int svs_map_apply_commit(svs_map *m, MapCommit *c) {
  svs_ctx *ctx = m->ctx;
  const int n_track = c->n_track, n_e = c->n_edges, kf = c->pair_kf, missing_cap = c->missing_cap;
  // ---- every refusal: before anything is uploaded ---------------------------------------------------------------------------------------------------------------
  SVS_REQUIRE(ctx, n_track >= 0 && n_e >= 0 && missing_cap >= 0 && svs_map_has_keyframe(m, kf));
  SVS_REQUIRE(ctx, (n_track == 0 || (c->d_track ? c->h_track_ids != nullptr : c->h_track != nullptr)) && (n_e == 0 || (c->h_edge_kf && c->h_edge_strength && c->h_cons)));
  SVS_REQUIRE(ctx, missing_cap == 0 || n_e == 0 || c->h_missing);
  SVS_REQUIRE(ctx, c->edge_type >= 0 && c->edge_type <= 2);
  MAP_CAPACITY(ctx, n_track < (1 << 24) && n_e <= m->max_kf);
  SVS_REQUIRE(ctx, c->n_cached >= 0 && (c->n_cached == 0 || (c->h_cached_ids && c->h_cached_T)));
  MAP_CAPACITY(ctx, c->n_cached <= m->max_kf);
  for (int k = 0; k < c->n_cached; ++k) SVS_REQUIRE(ctx, c->h_cached_ids[k] >= 0 && c->h_cached_ids[k] < m->max_kf && (k == 0 || c->h_cached_ids[k - 1] < c->h_cached_ids[k]));
  {
    const uint32_t st = m->next_stamp();
    for (int e = 0; e < n_e; ++e) {
      const int o = c->h_edge_kf[e];
      SVS_REQUIRE(ctx, svs_map_has_keyframe(m, o) && o != kf && m->stamp[o] != st);
      m->stamp[o] = st;
      SVS_REQUIRE(ctx, !m->edge_slot.count(edge_key(o, kf)));      // (the reference asserts in insertEdge)
    }
  }
  if (!c->d_track)
    for (int i = 0; i < n_track; ++i) SVS_REQUIRE(ctx, c->h_track[i].level >= 0 && c->h_track[i].level < SVS_NUM_PYR_LEVELS);
  MAP_CAPACITY(ctx, (size_t)m->n_obs + (size_t)n_track <= (size_t)m->max_obs);
  MAP_CAPACITY(ctx, n_e == 0 || (m->max_edges > 0 && (size_t)m->n_edges + (size_t)n_e <= (size_t)m->max_edges));
  // the mask of new pairs: the entry names a point of the map (:411-414), for the first time in the list, and (point, kf) is not a pair yet
  std::vector<int32_t> mask((size_t)n_track, 0);
  int n_add = 0;
  {
    const uint32_t st = m->next_stamp();
    for (int i = 0; i < n_track; ++i) {
      const int32_t g = c->d_track ? c->h_track_ids[i] : c->h_track[i].global_id;
      if (g < 0 || g >= m->max_pt || !m->pt_in[g] || m->stamp[g] == st) continue;
      m->stamp[g] = st;
      if (m->pairs.count(((uint64_t)(uint32_t)g << 32) | (uint32_t)kf)) continue;
      mask[(size_t)i] = 1; ++n_add;
    }
  }
  SVS_DEVICE(ctx);
  // ---- room: the staged block (track records of an explicit call | mask | edge records | constraint requests | cached ids and poses), the download block --------
  if (!m->d_meas) SVS_HIP(ctx, m->d_meas.alloc((size_t)m->max_obs));
  MapUp up(m);
  const auto track = up.piece<svs_map_track_point>(c->d_track ? 0 : n_track);
  const auto p_mask = up.piece<int32_t>(n_track);
  const auto edges = up.piece<edge_up>(n_e);
  const auto reqs = up.piece<cons_req>(n_e);
  const auto cached_ids = up.piece<int32_t>(c->n_cached);
  const auto cached_T = up.piece<double>(12 * (size_t)c->n_cached);
  MapDn dn(m);
  const auto cons = dn.piece<svs_map_constraint_result>(n_e);
  const auto missing = dn.piece<int32_t>((size_t)n_e * missing_cap);
  if (int rc = dn.reserve(std::max<size_t>(dn.end_aligned(), 16))) return rc;
  if (int rc = up.reserve(16)) return rc;
  // ---- the host's mirrors --------------------------------------------------------------------------------------------------------------------------------------
  const int log0 = m->n_obs, meas0 = m->n_meas, slot0 = m->n_edges;
  for (int i = 0; i < n_track; ++i) {
    if (!mask[(size_t)i]) continue;
    const int32_t g = c->d_track ? c->h_track_ids[i] : c->h_track[i].global_id;
    m->pairs.insert(((uint64_t)(uint32_t)g << 32) | (uint32_t)kf);
  }
  m->kf_nobs[kf] += n_add; m->n_obs += n_add; m->n_meas += n_add;
  if (n_add) m->win_valid = false;         // the prepared window was one of the map without these pairs
  // ---- the staged block ----------------------------------------------------------------------------------------------------------------------------------------
  size_t n_rows = 0;
  {
    up.put(track, c->h_track); up.put(p_mask, mask.data());
    edge_up *eu = up.host(edges);
    cons_req *cr = up.host(reqs);
    for (int e = 0; e < n_e; ++e) {
      const int o = c->h_edge_kf[e], kf1 = c->other_first ? o : kf, kf2 = c->other_first ? kf : o;
      eu[e].slot = slot0 + e; eu[e].lo = std::min(o, kf); eu[e].hi = std::max(o, kf); eu[e].strength = c->h_edge_strength[e]; eu[e].type = c->edge_type; eu[e].pad_ = 0;
      cons_req u{};
      u.kf1 = kf1; u.kf2 = kf2; u.slot = slot0 + e; u.slot_inv = kf1 > kf2 ? 1 : 0;
      u.n_override = 1; u.override_id[0] = kf; memcpy(u.override_T[0], c->T_new, sizeof u.override_T[0]);
      u.n_cached = c->n_cached; u.cached_off = 0; u.row_off = (long long)n_rows;
      cr[e] = u;
      n_rows += (size_t)m->kf_nobs[kf1];
      m->edge_slot[edge_key(o, kf)] = slot0 + e; m->edge_marg[(size_t)slot0 + e] = 0;
    }
    m->n_edges += n_e;
    up.put(cached_ids, c->h_cached_ids); up.put(cached_T, c->h_cached_T);
  }
  if (up.end)
    if (int rc = up.upload()) return rc;
  // ---- apply: the pairs, the edges -------------------------------------------------------------------------------------------------------------------------------
  if (n_add) {
    MapCommitK A{};
    A.tp = c->d_track ? c->d_track : up.dev(track); A.mask = up.dev(p_mask);
    A.n_track = n_track; A.kf = kf; A.log_tail = m->d_log.get() + log0; A.meas_tail = m->d_meas.get() + meas0;
    hipLaunchKernelGGL(map_commit_append_kernel, dim3(1), dim3(MB_THREADS), 0, ctx->stream, A);
  }
  if (n_e) hipLaunchKernelGGL(map_edge_add_kernel, dim3(div_up(n_e, 4)), dim3(256), 0, ctx->stream, m->d_edges.get(), up.dev(edges), n_e);
  SVS_LAUNCH_CHECK(ctx);
  c->n_pairs_added = n_add;
  if (c->h_track_added)
    for (int i = 0; i < n_track; ++i) c->h_track_added[i] = mask[(size_t)i];
  if (n_e == 0) { SVS_HIP(ctx, hipStreamSynchronize(ctx->stream)); return SVS_OK; }
  // ---- computeConstraint + setConstraint per new edge: the CSR rebuild, the unchanged kernel with the override, the download ------------------------------------------
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
  if (int rc = dn.download()) return rc;
  dn.get(cons, c->h_cons);
  dn.get(missing, c->h_missing);
  for (int e = 0; e < n_e; ++e)
    if (c->h_cons[e].status == SVS_CONS_OK) { m->edge_marg[(size_t)slot0 + e] = 1; ++m->n_marg; }
  return SVS_OK;
}

// the explicit calls' result
static void commit_result(const MapCommit &c, int mode, int other, svs_reg_commit_result *r) {
  memset(r, 0, sizeof *r);
  r->committed = 1; r->mode = mode; r->root_id = c.pair_kf; r->other_id = other; r->n_track = c.n_track; r->n_pairs_added = c.n_pairs_added; r->n_edges = c.n_edges;
  memcpy(r->T_new, c.T_new, sizeof r->T_new);
}

extern "C" int svs_map_register_keyframes(svs_map *m, int32_t root_id, const double *T_newroot_from_w, int n_neighbors, const int32_t *h_neighbor_ids,
                                          const int32_t *h_strength, int covis_thr, int n_track, const svs_map_track_point *h_track, int n_cached,
                                          const int32_t *h_cached_ids, const double *h_cached_T, int missing_cap, svs_reg_commit_result *h_res, int32_t *h_edge_kf,
                                          svs_map_constraint_result *h_cons, int32_t *h_missing, int32_t *h_track_added) {
  svs_ctx *ctx = m ? m->ctx : nullptr;
  SVS_REQUIRE(ctx, m && T_newroot_from_w && h_res && n_neighbors >= 0 && (n_neighbors == 0 || (h_neighbor_ids && h_strength && h_cons)) && n_track >= 0 &&
                       (n_track == 0 || h_track));
  // addNewEdges' test (:434), every neighbour a keyframe and named once; the ones that pass in ascending id
  std::vector<std::pair<int32_t, int32_t>> pass;
  {
    const uint32_t st = m->next_stamp();
    for (int i = 0; i < n_neighbors; ++i) {
      const int32_t o = h_neighbor_ids[i];
      SVS_REQUIRE(ctx, svs_map_has_keyframe(m, o) && o != root_id && m->stamp[o] != st);
      m->stamp[o] = st;
      if (h_strength[i] >= covis_thr) pass.push_back(std::make_pair(o, h_strength[i]));
    }
  }
  std::sort(pass.begin(), pass.end());
  std::vector<int32_t> ekf(pass.size()), est(pass.size());
  for (size_t e = 0; e < pass.size(); ++e) { ekf[e] = pass[e].first; est[e] = pass[e].second; }
  MapCommit c{};
  c.pair_kf = root_id; memcpy(c.T_new, T_newroot_from_w, sizeof c.T_new);
  c.n_track = n_track; c.h_track = h_track;
  c.n_edges = (int)pass.size(); c.h_edge_kf = ekf.data(); c.h_edge_strength = est.data(); c.edge_type = 1; c.other_first = true;
  c.n_cached = n_cached; c.h_cached_ids = h_cached_ids; c.h_cached_T = h_cached_T; c.missing_cap = missing_cap;
  c.h_cons = h_cons; c.h_missing = h_missing; c.h_track_added = h_track_added;
  if (int rc = svs_map_apply_commit(m, &c)) return rc;
  commit_result(c, SVS_REG_LOCAL, -1, h_res);
  if (h_edge_kf)
    for (int i = 0; i < n_neighbors; ++i) h_edge_kf[i] = i < c.n_edges ? ekf[(size_t)i] : -1;
  return SVS_OK;
}

extern "C" int svs_map_add_loop_closure(svs_map *m, int32_t root_id, int32_t loop_id, const double *T_newloop_from_w, int n_track, const svs_map_track_point *h_track,
                                        int n_cached, const int32_t *h_cached_ids, const double *h_cached_T, int missing_cap, svs_reg_commit_result *h_res,
                                        svs_map_constraint_result *h_cons, int32_t *h_missing, int32_t *h_track_added) {
  svs_ctx *ctx = m ? m->ctx : nullptr;
  SVS_REQUIRE(ctx, m && T_newloop_from_w && h_res && h_cons && n_track >= 0 && (n_track == 0 || h_track) && root_id != loop_id);
  const int32_t strength = n_track;      // (trackpoint_list.size(), :214)
  MapCommit c{};
  c.pair_kf = loop_id; memcpy(c.T_new, T_newloop_from_w, sizeof c.T_new);
  c.n_track = n_track; c.h_track = h_track;
  c.n_edges = 1; c.h_edge_kf = &root_id; c.h_edge_strength = &strength; c.edge_type = 2; c.other_first = false;
  c.n_cached = n_cached; c.h_cached_ids = h_cached_ids; c.h_cached_T = h_cached_T; c.missing_cap = missing_cap;
  c.h_cons = h_cons; c.h_missing = h_missing; c.h_track_added = h_track_added;
  if (int rc = svs_map_apply_commit(m, &c)) return rc;
  commit_result(c, SVS_REG_LOOP, root_id, h_res);
  return SVS_OK;
}
