// map_store.inc -- the update path of the device-resident map and its plain read-backs; included by map.hip behind map_csr.inc.
namespace {
// ---- updates: one staged upload, lane i scatters staged record i (16-byte loads of the 64-byte point records) ---------------------------------------------
struct kf_up { int32_t id, disp_stride; const float *disp; svs_keyframe kf; int32_t thr[THR_N]; };
static_assert(sizeof(kf_up) % 8 == 0, "staged as an array");

__global__ __launch_bounds__(256) void map_scatter_kf_kernel(MapK M, const kf_up *up, int n) {
  // 64 lanes per record: the thresholds are the bulk
  const int i = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (i >= n) return;
  const kf_up &u = up[i];
  const int id = u.id;
  for (int k = lane; k < THR_N; k += 64) M.kf_thr[(size_t)id * THR_N + k] = u.thr[k];
  if (lane < 17) reinterpret_cast<long long *>(M.kf + id)[lane] = reinterpret_cast<const long long *>(&u.kf)[lane];
  if (lane == 17) { M.kf_disp[id] = u.disp; M.kf_dstride[id] = u.disp_stride; M.kf_flags[id] = 0; }
}

__global__ __launch_bounds__(256) void map_scatter_pt_kernel(MapK M, const int32_t *ids, const svs_candidate_point *up, int n) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int id = ids[i];
  copy_rec64(M.pt + id, up + i, [&](int4 &q) { q.z = id; q.w = 0; });      // anchor_level, kf_index (the anchor's id), point_id, pad_
}

__global__ __launch_bounds__(256) void map_scatter_pose_kernel(MapK M, const int32_t *ids, const double *poses, int n) {
  const int t = blockIdx.x * 256 + threadIdx.x, i = t / 12, k = t % 12;
  if (i < n) M.kf[ids[i]].T_anchor_from_w[k] = poses[(size_t)i * 12 + k];
}

__global__ __launch_bounds__(256) void map_scatter_xyz_kernel(MapK M, const int32_t *ids, const double *xyz, int n) {
  const int t = blockIdx.x * 256 + threadIdx.x, i = t / 3, k = t % 3;
  if (i < n) M.pt[ids[i]].xyz_anchor[k] = xyz[(size_t)i * 3 + k];
}

// set == 0: every flag byte below kf_hi loses the bit; set == 1: the listed keyframes get it (two launches, stream order)
__global__ __launch_bounds__(256) void map_window_kernel(MapK M, const int32_t *ids, int n, int set) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (set) { if (i < n) M.kf_flags[ids[i]] = SVS_REG_KF_IN_WINDOW; }
  else if (i < M.kf_hi) M.kf_flags[i] = 0;
}

// lane i moves staged record i of svs_map_add_measured_observations to the tail of the measured store (four 16-byte loads) and its (point, keyframe) to the log's
__global__ __launch_bounds__(256) void map_append_meas_kernel(const svs_ba_edge *__restrict__ up, int n, int2 *__restrict__ log_tail, svs_ba_edge *__restrict__ store_tail) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int4 q = copy_rec64(store_tail + i, up + i);      // point, pose, anchor, pad_
  log_tail[i] = make_int2(q.x, q.y);
}

__global__ __launch_bounds__(256) void map_get_poses_kernel(MapK M, const int32_t *ids, int n, double *out) {
  const int t = blockIdx.x * 256 + threadIdx.x, i = t / 12, k = t % 12;
  if (i < n) out[t] = M.kf[ids[i]].T_anchor_from_w[k];
}

__global__ __launch_bounds__(256) void map_get_points_kernel(MapK M, const int32_t *__restrict__ ids, int n, svs_candidate_point *__restrict__ out) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  copy_rec64(out + i, M.pt + ids[i]);
}

// what the map holds of one keyframe: the record (136 bytes as 17 words of 8), the disparity's address and stride, the thresholds
struct kf_dn { svs_keyframe kf; const float *disp; int32_t disp_stride, pad_; int32_t thr[THR_N]; };
__global__ __launch_bounds__(256) void map_get_kf_kernel(MapK M, int id, kf_dn *out) {
  const int t = threadIdx.x;
  for (int k = t; k < THR_N; k += 256) out->thr[k] = M.kf_thr[(size_t)id * THR_N + k];
  if (t < 17) reinterpret_cast<long long *>(&out->kf)[t] = reinterpret_cast<const long long *>(M.kf + id)[t];
  if (t == 17) { out->disp = M.kf_disp[id]; out->disp_stride = M.kf_dstride[id]; out->pad_ = 0; }
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
    if ((unsigned)p < (unsigned)M.pt_hi) bit_set(mark, p);
  }
  __syncthreads();
  const int n = list_marked(mark, n_words, A.ids, 0, A.cap, s_w);
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
    if (lo < n_c && A.ids[lo] == q.x) copy_rec64(A.rec + lo, A.meas + i);
  }
  if (tid == 0) *A.count = n;
}
}  // namespace

extern "C" int svs_map_add_keyframes(svs_map *m, int n, const int32_t *h_ids, const svs_keyframe *h_keyframes, const float *const *h_disp_ptr,
                                     const int32_t *h_disp_stride, const int32_t *h_fast_thr) {
  svs_ctx *ctx = m ? m->ctx : nullptr;
  SVS_REQUIRE(ctx, m && n >= 0 && (n == 0 || (h_ids && h_keyframes && h_disp_ptr && h_disp_stride && h_fast_thr)));
  if (n == 0) return SVS_OK;
  if (int rc = map_check_ids(m, n, h_ids, m->kf_in, m->max_kf, false)) return rc;
  for (int i = 0; i < n; ++i) {
    SVS_REQUIRE(ctx, h_disp_ptr[i] && h_disp_stride[i] > 0);
    for (int l = 0; l < SVS_NUM_PYR_LEVELS; ++l) SVS_REQUIRE(ctx, h_keyframes[i].pyr[l] && h_keyframes[i].stride[l] > 0);
    for (int k = 0; k < THR_N; ++k) SVS_REQUIRE(ctx, h_fast_thr[(size_t)i * THR_N + k] >= 10 && h_fast_thr[(size_t)i * THR_N + k] <= 255);
  }
  SVS_DEVICE(ctx);
  MapUp up(m);
  const auto recs = up.piece<kf_up>(n);
  if (int rc = up.reserve()) return rc;
  kf_up *u = up.host(recs);
  for (int i = 0; i < n; ++i) {
    u[i].id = h_ids[i]; u[i].disp_stride = h_disp_stride[i]; u[i].disp = h_disp_ptr[i]; u[i].kf = h_keyframes[i]; u[i].kf.pad_ = 0;
    memcpy(u[i].thr, h_fast_thr + (size_t)i * THR_N, sizeof u[i].thr);
  }
  if (int rc = up.upload()) return rc;
  hipLaunchKernelGGL(map_scatter_kf_kernel, dim3(div_up(n, 4)), dim3(256), 0, ctx->stream, m->view(), up.dev(recs), n);
  SVS_LAUNCH_CHECK(ctx);
  for (int i = 0; i < n; ++i) {
    const int id = h_ids[i];
    m->kf_in[id] = 1;
    MapRootView &v = m->kf_view[id];
    for (int l = 0; l < SVS_NUM_PYR_LEVELS; ++l) { v.pyr[l] = h_keyframes[i].pyr[l]; v.stride[l] = h_keyframes[i].stride[l]; }
    v.disp = h_disp_ptr[i]; v.disp_stride = h_disp_stride[i];
    m->kf_hi = std::max(m->kf_hi, id + 1);
  }
  m->n_kf += n;
  return SVS_OK;
}

extern "C" int svs_map_add_points(svs_map *m, int n, const int32_t *h_ids, const svs_candidate_point *h_points) {
  svs_ctx *ctx = m ? m->ctx : nullptr;
  SVS_REQUIRE(ctx, m && n >= 0 && (n == 0 || (h_ids && h_points)));
  if (n == 0) return SVS_OK;
  if (int rc = map_check_ids(m, n, h_ids, m->pt_in, m->max_pt, false)) return rc;
  for (int i = 0; i < n; ++i) SVS_REQUIRE(ctx, svs_map_has_keyframe(m, h_points[i].kf_index));
  SVS_DEVICE(ctx);
  MapUp up(m);
  const auto ids = up.piece<int32_t>(n);
  const auto pts = up.piece<svs_candidate_point>(n);
  if (int rc = up.reserve()) return rc;
  up.put(ids, h_ids); up.put(pts, h_points);
  if (int rc = up.upload()) return rc;
  hipLaunchKernelGGL(map_scatter_pt_kernel, dim3(div_up(n, 256)), dim3(256), 0, ctx->stream, m->view(), up.dev(ids), up.dev(pts), n);
  SVS_LAUNCH_CHECK(ctx);
  for (int i = 0; i < n; ++i) { m->pt_in[h_ids[i]] = 1; m->pt_hi = std::max(m->pt_hi, h_ids[i] + 1); }
  m->n_pt += n;
  m->win_valid = false;                // (the prepared window's lists are sized by the points it saw)
  return SVS_OK;
}

// h_center == nullptr: svs_map_add_observations; else the pairs come with their measurements (h_level checked by the caller)
static int map_add_observations(svs_map *m, int n, const int32_t *h_point_ids, const int32_t *h_kf_ids, const double *h_center, const int32_t *h_level) {
  svs_ctx *ctx = m->ctx;
  for (int i = 0; i < n; ++i) SVS_REQUIRE(ctx, h_point_ids[i] >= 0 && h_point_ids[i] < m->max_pt && m->pt_in[h_point_ids[i]] && svs_map_has_keyframe(m, h_kf_ids[i]));
  // the pairs that are new, each once, in the caller's order
  std::vector<int2> fresh;
  std::vector<int> from;
  std::unordered_set<uint64_t> seen;
  for (int i = 0; i < n; ++i) {
    const uint64_t key = ((uint64_t)(uint32_t)h_point_ids[i] << 32) | (uint32_t)h_kf_ids[i];
    if (m->pairs.count(key) || !seen.insert(key).second) continue;
    fresh.push_back(make_int2(h_point_ids[i], h_kf_ids[i]));
    if (h_center) from.push_back(i);
  }
  MAP_CAPACITY(ctx, (size_t)m->n_obs + fresh.size() <= (size_t)m->max_obs);
  if (fresh.empty()) return SVS_OK;
  SVS_DEVICE(ctx);
  const int nf = (int)fresh.size();
  MapUp up(m);
  if (!h_center) {
    const auto pairs = up.piece<int2>(fresh.size());
    if (int rc = up.reserve()) return rc;
    up.put(pairs, fresh.data());
    if (int rc = up.upload(m->d_log.get() + m->n_obs)) return rc;      // straight to the log's tail
    m->n_unmeasured += nf;
  } else {
    if (!m->d_meas) SVS_HIP(ctx, m->d_meas.alloc((size_t)m->max_obs));
    const auto recs = up.piece<svs_ba_edge>(fresh.size());
    if (int rc = up.reserve()) return rc;
    svs_ba_edge *rec = up.host(recs);
    for (int k = 0; k < nf; ++k) {
      const int i = from[k];
      const double s = 1.0 / (double)(1 << h_level[i]);                                                 // pyrFromZero_d(1., level) (slam_graph.cpp:1012)
      svs_ba_edge e;
      for (int c = 0; c < 3; ++c) e.obs[c] = h_center[(size_t)i * 3 + c];
      e.info[0] = s * s; e.info[1] = s * s; e.info[2] = 0.333 * 0.333;
      e.point = fresh[k].x; e.pose = fresh[k].y; e.anchor = 0; e.pad_ = 0;
      rec[k] = e;
    }
    if (int rc = up.upload()) return rc;
    hipLaunchKernelGGL(map_append_meas_kernel, dim3(div_up(nf, 256)), dim3(256), 0, ctx->stream, up.dev(recs), nf, m->d_log.get() + m->n_obs, m->d_meas.get() + m->n_meas);
    SVS_LAUNCH_CHECK(ctx);
    m->n_meas += nf;
  }
  for (const int2 &o : fresh) { m->pairs.insert(((uint64_t)(uint32_t)o.x << 32) | (uint32_t)o.y); ++m->kf_nobs[o.y]; }
  m->n_obs += nf;
  m->win_valid = false;                // the prepared window was one of the map without these pairs
  return SVS_OK;
}

extern "C" int svs_map_add_observations(svs_map *m, int n, const int32_t *h_point_ids, const int32_t *h_kf_ids) {
  svs_ctx *ctx = m ? m->ctx : nullptr;
  SVS_REQUIRE(ctx, m && n >= 0 && (n == 0 || (h_point_ids && h_kf_ids)));
  if (n == 0) return SVS_OK;
  return map_add_observations(m, n, h_point_ids, h_kf_ids, nullptr, nullptr);
}

extern "C" int svs_map_add_measured_observations(svs_map *m, int n, const int32_t *h_point_ids, const int32_t *h_kf_ids, const double *h_center,
                                                 const int32_t *h_level) {
  svs_ctx *ctx = m ? m->ctx : nullptr;
  SVS_REQUIRE(ctx, m && n >= 0 && (n == 0 || (h_point_ids && h_kf_ids && h_center && h_level)));
  if (n == 0) return SVS_OK;
  for (int i = 0; i < n; ++i) SVS_REQUIRE(ctx, h_level[i] >= 0 && h_level[i] < SVS_NUM_PYR_LEVELS);
  return map_add_observations(m, n, h_point_ids, h_kf_ids, h_center, h_level);
}

extern "C" int svs_map_measured_info(svs_map *map, int32_t *n_measured, int32_t *n_unmeasured) {
  if (!map) return SVS_ERR_INVALID;
  if (n_measured) *n_measured = map->n_meas;
  if (n_unmeasured) *n_unmeasured = map->n_unmeasured;
  return SVS_OK;
}

// ids [n] and n rows of `row` doubles, scattered by `kernel`
template <class Kernel>
static int map_set_rows(svs_map *m, int n, const int32_t *ids, const double *rows, int row, Kernel kernel) {
  svs_ctx *ctx = m->ctx;
  SVS_DEVICE(ctx);
  MapUp up(m);
  const auto p_ids = up.piece<int32_t>(n);
  const auto p_rows = up.piece<double>((size_t)n * row);
  if (int rc = up.reserve()) return rc;
  up.put(p_ids, ids); up.put(p_rows, rows);
  if (int rc = up.upload()) return rc;
  hipLaunchKernelGGL(kernel, dim3(div_up(n * row, 256)), dim3(256), 0, ctx->stream, m->view(), up.dev(p_ids), up.dev(p_rows), n);
  SVS_LAUNCH_CHECK(ctx);
  return SVS_OK;
}

extern "C" int svs_map_set_poses(svs_map *m, int n, const int32_t *h_kf_ids, const double *h_poses) {
  svs_ctx *ctx = m ? m->ctx : nullptr;
  SVS_REQUIRE(ctx, m && n >= 0 && (n == 0 || (h_kf_ids && h_poses)));
  if (n == 0) return SVS_OK;
  if (int rc = map_check_ids(m, n, h_kf_ids, m->kf_in, m->max_kf, true)) return rc;
  return map_set_rows(m, n, h_kf_ids, h_poses, 12, map_scatter_pose_kernel);
}

extern "C" int svs_map_set_points(svs_map *m, int n, const int32_t *h_point_ids, const double *h_xyz_anchor) {
  svs_ctx *ctx = m ? m->ctx : nullptr;
  SVS_REQUIRE(ctx, m && n >= 0 && (n == 0 || (h_point_ids && h_xyz_anchor)));
  if (n == 0) return SVS_OK;
  if (int rc = map_check_ids(m, n, h_point_ids, m->pt_in, m->max_pt, true)) return rc;
  return map_set_rows(m, n, h_point_ids, h_xyz_anchor, 3, map_scatter_xyz_kernel);
}

extern "C" int svs_map_set_window(svs_map *m, int n, const int32_t *h_kf_ids) {
  svs_ctx *ctx = m ? m->ctx : nullptr;
  SVS_REQUIRE(ctx, m && n >= 0 && (n == 0 || h_kf_ids));
  if (int rc = map_check_ids(m, n, h_kf_ids, m->kf_in, m->max_kf, true)) return rc;
  SVS_DEVICE(ctx);
  MapUp up(m);
  const auto ids = up.piece<int32_t>(n);
  if (n) {
    if (int rc = up.reserve()) return rc;
    up.put(ids, h_kf_ids);
    if (int rc = up.upload()) return rc;
  }
  if (m->kf_hi) {
    hipLaunchKernelGGL(map_window_kernel, dim3(div_up(m->kf_hi, 256)), dim3(256), 0, ctx->stream, m->view(), (const int32_t *)nullptr, 0, 0);
    SVS_LAUNCH_CHECK(ctx);
  }
  if (n) {
    hipLaunchKernelGGL(map_window_kernel, dim3(div_up(n, 256)), dim3(256), 0, ctx->stream, m->view(), up.dev(ids), n, 1);
    SVS_LAUNCH_CHECK(ctx);
  }
  return SVS_OK;
}

extern "C" int svs_map_get_poses(svs_map *m, int n, const int32_t *h_kf_ids, double *h_poses) {
  svs_ctx *ctx = m ? m->ctx : nullptr;
  SVS_REQUIRE(ctx, m && n >= 0 && (n == 0 || (h_kf_ids && h_poses)));
  for (int i = 0; i < n; ++i) SVS_REQUIRE(ctx, svs_map_has_keyframe(m, h_kf_ids[i]));
  if (n == 0) return SVS_OK;
  return map_read_back(m, n, h_kf_ids, 12, h_poses, [&](const int32_t *ids, double *out) {
    hipLaunchKernelGGL(map_get_poses_kernel, dim3(div_up(n * 12, 256)), dim3(256), 0, ctx->stream, m->view(), ids, n, out);
  });
}

extern "C" int svs_map_get_points(svs_map *m, int n, const int32_t *h_ids, svs_candidate_point *h_out) {
  svs_ctx *ctx = m ? m->ctx : nullptr;
  SVS_REQUIRE(ctx, m && n >= 0 && (n == 0 || (h_ids && h_out)));
  for (int i = 0; i < n; ++i) SVS_REQUIRE(ctx, h_ids[i] >= 0 && h_ids[i] < m->max_pt && m->pt_in[h_ids[i]]);
  if (n == 0) return SVS_OK;
  return map_read_back(m, n, h_ids, 1, h_out, [&](const int32_t *ids, svs_candidate_point *out) {
    hipLaunchKernelGGL(map_get_points_kernel, dim3(div_up(n, 256)), dim3(256), 0, ctx->stream, m->view(), ids, n, out);
  });
}

extern "C" int svs_map_get_keyframe(svs_map *m, int32_t kf_id, svs_keyframe *h_keyframe, const float **h_disp, int32_t *h_disp_stride, int32_t *h_fast_thr) {
  svs_ctx *ctx = m ? m->ctx : nullptr;
  SVS_REQUIRE(ctx, m && svs_map_has_keyframe(m, kf_id));
  SVS_DEVICE(ctx);
  MapDn dn(m);
  const auto rec = dn.piece<kf_dn>(1);
  if (int rc = dn.reserve()) return rc;
  hipLaunchKernelGGL(map_get_kf_kernel, dim3(1), dim3(256), 0, ctx->stream, m->view(), kf_id, dn.dev(rec));
  SVS_LAUNCH_CHECK(ctx);
  if (int rc = dn.download()) return rc;
  const kf_dn &r = *dn.host(rec);
  if (h_keyframe) *h_keyframe = r.kf;
  if (h_disp) *h_disp = r.disp;
  if (h_disp_stride) *h_disp_stride = r.disp_stride;
  if (h_fast_thr) memcpy(h_fast_thr, r.thr, sizeof r.thr);
  return SVS_OK;
}

extern "C" int svs_map_get_feature_table(svs_map *m, int32_t kf_id, int cap, int32_t *h_count, int32_t *h_point_ids, svs_ba_edge *h_meas) {
  svs_ctx *ctx = m ? m->ctx : nullptr;
  SVS_REQUIRE(ctx, m && h_count && cap >= 0 && (cap == 0 || (h_point_ids && h_meas)) && svs_map_has_keyframe(m, kf_id));
  MAP_CAPACITY(ctx, cap <= m->max_pt);
  SVS_DEVICE(ctx);
  MapDn dn(m);
  const auto count = dn.piece<int32_t>(1);
  const auto ids = dn.piece<int32_t>(cap);
  const auto rec = dn.piece<svs_ba_edge>(cap);
  if (int rc = dn.reserve()) return rc;
  if (int rc = map_prepare_walk(m, 1)) return rc;
  MapFtK A{};
  A.kf = kf_id; A.cap = cap; A.n_meas = m->n_meas; A.meas = m->d_meas;
  A.count = dn.dev(count); A.ids = dn.dev(ids); A.rec = dn.dev(rec);
  hipLaunchKernelGGL(map_feature_table_kernel, dim3(1), dim3(MB_THREADS), 0, ctx->stream, m->view(), A);
  SVS_LAUNCH_CHECK(ctx);
  if (int rc = dn.download()) return rc;
  const int n = *dn.host(count), n_c = std::min(n, cap);
  *h_count = n;
  for (int i = 0; i < cap; ++i) h_point_ids[i] = i < n_c ? dn.host(ids)[i] : -1;
  if (cap) { memcpy(h_meas, dn.host(rec), (size_t)n_c * sizeof(svs_ba_edge)); memset(h_meas + n_c, 0, (size_t)(cap - n_c) * sizeof(svs_ba_edge)); }
  return SVS_OK;
}
