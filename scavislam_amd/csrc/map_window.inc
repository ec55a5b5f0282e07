// map_window.inc -- the double window's BA problem prepared from the resident map (ba_map.h), included by map.hip behind map_walk.inc:
// computeActivePointsAndExtendOuterWindow (slam_graph.cpp:599-663) as set operations with one workgroup per INNER keyframe -- W0 and its graph neighbours as LDS
// bitmaps, active points and the extension as bitmaps in global memory -- then ascending lists, poses and psi = invert_depth(xyz_anchor) by popcount prefixes;
// map_win_gather / map_win_store move the state to and from the optimizer.
namespace {
constexpr int MAP_WIN_MAX = 256;       // the solve's limit (ba.hip: SOLVE_MAX_P)
struct MapWinK {
  const int32_t *ids, *types, *pairs, *inner; int n0, n_pairs, window_cap, set_flags;      // staged: W0, the pairs, the INNER keyframes of W0
  uint32_t *active, *ext;              // bitmaps over point ids (the walk's row 0 of M.mark) / keyframe ids; zero before the first launch
  svs_map_window_result *res;          // zero before the first launch
  int32_t *wid, *wtype;                // [MAP_WIN_MAX] the final window
  int32_t *lids, *aids; double *poses, *psi;      // active ids | anchor ids | poses | psi
};

// one workgroup per INNER keyframe F of W0 (:611-646): W0 and F's graph neighbours are LDS bitmaps, F's feature_table row marks the active points and the extension
__global__ __launch_bounds__(MB_THREADS) void map_win_mark_kernel(MapK M, MapWinK A) {
  __shared__ uint32_t s_w0[MAP_KF_WORDS], s_nb[MAP_KF_WORDS];
  const int tid = threadIdx.x, F = A.inner[blockIdx.x];
  s_w0[tid] = 0; s_nb[tid] = 0;
  __syncthreads();
  // (ids the host has checked: in the map, so below kf_hi <= MAP_MAX_KF)
  for (int i = tid; i < A.n0; i += MB_THREADS) bit_set(s_w0, A.ids[i]);
  for (int i = tid; i < A.n_pairs; i += MB_THREADS) {          // orderd_find is symmetric
    const int a = A.pairs[2 * i], b = A.pairs[2 * i + 1];
    if (a == F) bit_set(s_nb, b);
    if (b == F) bit_set(s_nb, a);
  }
  __syncthreads();
  const int e1 = M.kf_begin[F + 1];
  for (int e0 = M.kf_begin[F]; e0 < e1; e0 += MB_THREADS) {    // block-uniform
    const int e = e0 + tid;
    const int p = e < e1 ? M.kf_rows[e] : -1;
    const bool have = (unsigned)p < (unsigned)M.pt_hi;
    const int a = have ? M.pt[p].kf_index : -1;                // the anchor's id
    const bool a_ok = (unsigned)a < (unsigned)MAP_MAX_KF;
    const bool in_w0 = a_ok && bit_of(s_w0, a);
    const bool act = a_ok && (in_w0 || bit_of(s_nb, a));       // (:627, :636)
    wave_or_by_word(A.active, p >> 5, 1u << (p & 31), act);
    wave_or_by_word(A.ext, a >> 5, 1u << (a & 31), act && !in_w0);
  }
}

// both bitmaps to ascending ids by popcount prefixes; workgroup b owns the words [b * MB_THREADS, (b + 1) * MB_THREADS) of the active bitmap, workgroup 0 also
// the window's rows, poses, flags and the result.  Every workgroup finds the final window's size itself: over window_cap nothing is written but the result
__global__ __launch_bounds__(MB_THREADS) void map_win_list_kernel(MapK M, MapWinK A) {
  __shared__ uint32_t s_w0[MAP_KF_WORDS];
  __shared__ int s_w[MB_THREADS / 64];
  const int tid = threadIdx.x;
  const uint32_t ext = A.ext[tid];
  int n_ext;
  const int ext_rank = block_excl_scan(__popc(ext), s_w, n_ext);
  const int n_window = A.n0 + n_ext;
  if (n_window > A.window_cap) {                               // block-uniform
    if (blockIdx.x == 0 && tid == 0) { svs_map_window_result R; R.n_window = n_window; R.n_initial = A.n0; R.n_active = -1; R.n_edges_bound = 0; *A.res = R; }
    return;
  }
  const int n_words = (M.pt_hi + 31) >> 5, w_first = blockIdx.x * MB_THREADS;
  int before = 0, all = 0;
  for (int w = tid; w < n_words; w += MB_THREADS) { const int c = __popc(A.active[w]); all += c; if (w < w_first) before += c; }
  int n_before, n_active;
  (void)block_excl_scan(before, s_w, n_before);
  (void)block_excl_scan(all, s_w, n_active);
  const int w = w_first + tid;
  int bound = 0;
  (void)list_words(w < n_words ? A.active[w] : 0u, w << 5, n_before, s_w, [&](int p, int pos) {      // pos < n_active <= the points of the map
    const svs_candidate_point &q = M.pt[p];
    A.lids[pos] = p; A.aids[pos] = q.kf_index;
    psi_of_xyz(q.xyz_anchor, A.psi + 3 * (size_t)pos);
    bound += M.pt_begin[p + 1] - M.pt_begin[p];
  });
  int bound_all;
  (void)block_excl_scan(bound, s_w, bound_all);
  if (tid == 0 && bound_all) atomicAdd(&A.res->n_edges_bound, bound_all);      // a sum of integers: no order in it
  if (blockIdx.x != 0) return;
  // the final window: W0 as given, the extension ascending and OUTER
  for (int i = tid; i < A.n0; i += MB_THREADS) { A.wid[i] = A.ids[i]; A.wtype[i] = A.types[i]; }
  for_each_set_bit(ext, tid << 5, A.n0 + ext_rank, [&](int id, int e) { A.wid[e] = id; A.wtype[e] = 1; });
  for (int i = n_window + tid; i < MAP_WIN_MAX; i += MB_THREADS) { A.wid[i] = -1; A.wtype[i] = -1; }
  __syncthreads();
  for (int i = tid; i < n_window * 12; i += MB_THREADS) A.poses[i] = M.kf[A.wid[i / 12]].T_anchor_from_w[i % 12];
  if (A.set_flags) {                                           // exactly the final window, as map_window_kernel's two launches leave it
    s_w0[tid] = 0;
    __syncthreads();
    for (int i = tid; i < A.n0; i += MB_THREADS) bit_set(s_w0, A.ids[i]);
    __syncthreads();
    s_w0[tid] |= ext;
    __syncthreads();
    for (int i = tid; i < M.kf_hi; i += MB_THREADS) M.kf_flags[i] = bit_of(s_w0, i) ? SVS_REG_KF_IN_WINDOW : 0;
  }
  if (tid == 0) { A.res->n_window = n_window; A.res->n_initial = A.n0; A.res->n_active = n_active; }
}

// what svs_ba_window_from_map reads at its moment: the window's poses and psi again
__global__ __launch_bounds__(256) void map_win_gather_kernel(MapK M, MapWinK A, int P, int L) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < 12 * P) A.poses[i] = M.kf[A.wid[i / 12]].T_anchor_from_w[i % 12];
  if (i < L) psi_of_xyz(M.pt[A.lids[i]].xyz_anchor, A.psi + 3 * (size_t)i);
}

// restoreDataFromG2o (:1035-1058): poses by the window's ids, xyz_anchor = invert_depth(psi) by the active ids
__global__ __launch_bounds__(256) void map_win_store_kernel(MapK M, MapWinK A, int P, int L, const double *__restrict__ poses, const double *__restrict__ psi) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < 12 * P) M.kf[A.wid[i / 12]].T_anchor_from_w[i % 12] = poses[i];
  if (i < L) xyz_of_psi(psi + 3 * (size_t)i, M.pt[A.lids[i]].xyz_anchor);
}
}  // namespace

// ---- the prepared window ------------------------------------------------------------------------------------------------------------------------------
namespace {
constexpr size_t WIN_O_EXT = 0, WIN_O_RES = WIN_O_EXT + sizeof(uint32_t) * MAP_KF_WORDS, WIN_O_WID = WIN_O_RES + sizeof(svs_map_window_result),
                 WIN_O_WTYPE = WIN_O_WID + sizeof(int32_t) * MAP_WIN_MAX, WIN_HEAD_END = WIN_O_WTYPE + sizeof(int32_t) * MAP_WIN_MAX;
size_t win_align(size_t v) { return (v + 255) & ~(size_t)255; }
// the block's pieces; the lists are as long as the map has room for points
MapWinK map_win_pieces(const svs_map *m) {
  MapWinK A{};
  uint8_t *W = m->d_win.get();
  const size_t o_lids = win_align(WIN_HEAD_END), o_aids = o_lids + win_align(sizeof(int32_t) * (size_t)m->max_pt), o_poses = o_aids + win_align(sizeof(int32_t) * (size_t)m->max_pt),
               o_psi = o_poses + win_align(sizeof(double) * 12 * MAP_WIN_MAX);
  A.ext = reinterpret_cast<uint32_t *>(W + WIN_O_EXT); A.res = reinterpret_cast<svs_map_window_result *>(W + WIN_O_RES);
  A.wid = reinterpret_cast<int32_t *>(W + WIN_O_WID); A.wtype = reinterpret_cast<int32_t *>(W + WIN_O_WTYPE);
  A.lids = reinterpret_cast<int32_t *>(W + o_lids); A.aids = reinterpret_cast<int32_t *>(W + o_aids);
  A.poses = reinterpret_cast<double *>(W + o_poses); A.psi = reinterpret_cast<double *>(W + o_psi);
  A.active = m->d_mark;
  return A;
}
size_t map_win_bytes(const svs_map *m) {
  return win_align(WIN_HEAD_END) + 2 * win_align(sizeof(int32_t) * (size_t)m->max_pt) + win_align(sizeof(double) * 12 * MAP_WIN_MAX) + win_align(sizeof(double) * 3 * (size_t)m->max_pt);
}
uint64_t next_win_serial() { static uint64_t s = 0; return __atomic_add_fetch(&s, 1, __ATOMIC_RELAXED); }
}  // namespace

// the block of the prepared window and the pinned twin of its head
static int map_win_reserve(svs_map *m) {
  svs_ctx *ctx = m->ctx;
  if (!m->d_win) SVS_HIP(ctx, m->d_win.alloc(map_win_bytes(m)));
  if (m->h_win.bytes() < WIN_HEAD_END - WIN_O_RES) SVS_HIP(ctx, m->h_win.alloc(WIN_HEAD_END - WIN_O_RES));
  return SVS_OK;
}

// from W0, its INNER keyframes and the pairs on the device (A.ids, A.types, A.inner, A.pairs, A.n0, A.n_pairs) to the prepared window: two launches, one download
static int map_win_finish(svs_map *m, const MapWinK &A, int n_inner, int window_cap, svs_map_window_result *h_res, int32_t *h_window_ids, int32_t *h_window_type) {
  svs_ctx *ctx = m->ctx;
  m->win_valid = false;                // from here on the block holds the new window, or nothing
  const MapK M = m->view();
  const int n_words = (m->pt_hi + 31) >> 5;
  SVS_HIP(ctx, hipMemsetAsync(m->d_win.get() + WIN_O_EXT, 0, WIN_O_WID - WIN_O_EXT, ctx->stream));      // the extension bitmap and the result
  if (n_words) SVS_HIP(ctx, hipMemsetAsync(m->d_mark, 0, sizeof(uint32_t) * (size_t)n_words, ctx->stream));
  hipLaunchKernelGGL(map_win_mark_kernel, dim3(n_inner), dim3(MB_THREADS), 0, ctx->stream, M, A);
  hipLaunchKernelGGL(map_win_list_kernel, dim3(std::max(1, div_up(n_words, MB_THREADS))), dim3(MB_THREADS), 0, ctx->stream, M, A);
  SVS_LAUNCH_CHECK(ctx);
  SVS_HIP(ctx, hipMemcpyAsync(m->h_win, m->d_win.get() + WIN_O_RES, WIN_HEAD_END - WIN_O_RES, hipMemcpyDeviceToHost, ctx->stream));
  SVS_HIP(ctx, hipStreamSynchronize(ctx->stream));
  const svs_map_window_result R = *reinterpret_cast<const svs_map_window_result *>(m->h_win.get());
  const int32_t *wid = reinterpret_cast<const int32_t *>(m->h_win.get() + (WIN_O_WID - WIN_O_RES)), *wtype = wid + MAP_WIN_MAX;
  *h_res = R;
  const bool over = R.n_active < 0;
  for (int i = 0; i < window_cap; ++i) {
    if (h_window_ids) h_window_ids[i] = !over && i < R.n_window ? wid[i] : -1;
    if (h_window_type) h_window_type[i] = !over && i < R.n_window ? wtype[i] : -1;
  }
  if (over) return SVS_OK;
  m->win_ids.assign(wid, wid + R.n_window); m->win_types.assign(wtype, wtype + R.n_window);
  m->win_P = R.n_window; m->win_L = R.n_active; m->win_serial = next_win_serial(); m->win_valid = true;
  return SVS_OK;
}

extern "C" int svs_map_prepare_window(svs_map *m, int n0, const int32_t *h_kf_ids, const int32_t *h_kf_type, int n_pairs, const int32_t *h_edge_pairs,
                                      int set_window_flags, int window_cap, svs_map_window_result *h_res, int32_t *h_window_ids, int32_t *h_window_type) {
  svs_ctx *ctx = m ? m->ctx : nullptr;
  SVS_REQUIRE(ctx, m && n0 >= 1 && h_kf_ids && h_kf_type && n_pairs >= 0 && (n_pairs == 0 || h_edge_pairs) && window_cap >= 1 && h_res);
  MAP_CAPACITY(ctx, n0 <= window_cap && window_cap <= MAP_WIN_MAX);
  if (int rc = map_check_ids(m, n0, h_kf_ids, m->kf_in, m->max_kf, true)) return rc;
  int n_inner = 0;
  for (int i = 0; i < n0; ++i) { SVS_REQUIRE(ctx, h_kf_type[i] == 0 || h_kf_type[i] == 1); n_inner += h_kf_type[i] == 0; }
  SVS_REQUIRE(ctx, n_inner >= 1);
  for (int i = 0; i < 2 * n_pairs; ++i) SVS_REQUIRE(ctx, svs_map_has_keyframe(m, h_edge_pairs[i]));
  if (m->n_unmeasured > 0) { ctx->err = "svs_map_prepare_window: the map holds observations without a measurement (svs_map_add_observations)"; return SVS_ERR_INVALID; }
  SVS_DEVICE(ctx);
  if (int rc = map_win_reserve(m)) return rc;
  if (int rc = map_prepare_walk(m, 1)) return rc;
  // one staged upload: W0's ids | types | the INNER ones | the pairs
  MapUp up(m);
  const auto ids = up.piece<int32_t>(n0), types = up.piece<int32_t>(n0), inner = up.piece<int32_t>(n_inner), pairs = up.piece<int32_t>(2 * (size_t)n_pairs);
  if (int rc = up.reserve()) return rc;
  up.put(ids, h_kf_ids); up.put(types, h_kf_type); up.put(pairs, h_edge_pairs);
  for (int i = 0, k = 0; i < n0; ++i) if (h_kf_type[i] == 0) up.host(inner)[k++] = h_kf_ids[i];
  if (int rc = up.upload()) return rc;
  MapWinK A = map_win_pieces(m);
  A.ids = up.dev(ids); A.types = up.dev(types); A.inner = up.dev(inner); A.pairs = up.dev(pairs);
  A.n0 = n0; A.n_pairs = n_pairs; A.window_cap = window_cap; A.set_flags = set_window_flags != 0;
  return map_win_finish(m, A, n_inner, window_cap, h_res, h_window_ids, h_window_type);
}

bool svs_map_window_is(const svs_map *m, uint64_t serial) { return m && m->win_valid && m->win_serial == serial; }

int svs_map_window_view(svs_map *m, MapWindowView *out) {
  svs_ctx *ctx = m->ctx;
  SVS_REQUIRE(ctx, m->win_valid);
  const MapWinK A = map_win_pieces(m);
  const int P = m->win_P, L = m->win_L;
  hipLaunchKernelGGL(map_win_gather_kernel, dim3(div_up(std::max(12 * P, L), 256)), dim3(256), 0, ctx->stream, m->view(), A, P, L);
  SVS_LAUNCH_CHECK(ctx);
  MapWindowView V{};
  V.P = P; V.L = L; V.window_ids = A.wid; V.h_window_ids = m->win_ids.data(); V.active_ids = A.lids; V.anchor_ids = A.aids; V.poses = A.poses; V.psi = A.psi;
  V.store = m->d_meas; V.n_store = (size_t)m->n_meas; V.kf_hi = m->kf_hi; V.pt_hi = m->pt_hi; V.serial = m->win_serial;
  V.h_window_types = m->win_types.data(); V.edges = m->d_edges;
  *out = V;
  return SVS_OK;
}

int svs_map_window_store(svs_map *m, const double *d_poses, const double *d_psi) {
  svs_ctx *ctx = m->ctx;
  SVS_REQUIRE(ctx, m->win_valid);
  const int P = m->win_P, L = m->win_L;
  hipLaunchKernelGGL(map_win_store_kernel, dim3(div_up(std::max(12 * P, L), 256)), dim3(256), 0, ctx->stream, m->view(), map_win_pieces(m), P, L, d_poses, d_psi);
  SVS_LAUNCH_CHECK(ctx);
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
  WalkDn dn(m, 1, double_size, false, true);
  if (int rc = map_walk_run(m, 1, W, &root_id, 1, dn)) return rc;
  const int4 hdr = *dn.host(dn.hdr);
  MapWinK A = map_win_pieces(m);
  A.ids = S.d_pairs.get(); A.types = A.ids + MAP_WIN_MAX; A.inner = A.types + MAP_WIN_MAX; A.pairs = A.inner + MAP_WIN_MAX;
  A.n0 = hdr.x; A.n_pairs = hdr.y; A.window_cap = window_cap; A.set_flags = set_window_flags != 0;
  return map_win_finish(m, A, hdr.z, window_cap, h_res, h_window_ids, h_window_type);
}
