// map_request.inc -- the requests of the registration chain (register.hip, reg_map.h) built from the resident map, included by map.hip behind map_csr.inc:
// pointsVisibleInRoot's point walk (backend.cpp:480-497) / the query keyframe's feature_table (:853-858) as set operations, one workgroup per request.  The walk
// and direct sets and the built table are LDS bitmaps over keyframe ids, the point set the request's row of M.mark; marking walks the feature_tables of the walk
// set, and the lists are the set bits in ascending order (map_sets.h): the built request is a function of the map's content alone.
namespace {
__global__ __launch_bounds__(MB_THREADS) void map_build_kernel(MapK M, MapBuildDst D) {
  __shared__ uint32_t s_walk[MAP_KF_WORDS], s_dir[MAP_KF_WORDS], s_tab[MAP_KF_WORDS];
  __shared__ int s_rank[MAP_KF_WORDS];
  __shared__ int s_w[MB_THREADS / 64];
  const int r = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const map_req &Q = D.req[r];
  const int root = Q.root, mode = Q.mode;
  const int32_t *walk = D.ids + Q.walk_off, *direct = D.ids + Q.direct_off;
  uint32_t *mark = M.mark + (size_t)r * M.mark_b;
  const int n_words = (M.pt_hi + 31) >> 5;                      // <= mark_b
  // a. empty sets
  s_walk[tid] = 0; s_dir[tid] = 0; s_tab[tid] = 0;
  for (int i = tid; i < n_words; i += MB_THREADS) mark[i] = 0;
  __syncthreads();
  // b. the keyframe sets (ids the host has checked: in the map, so below kf_hi <= MAP_MAX_KF)
  for (int i = tid; i < Q.n_direct; i += MB_THREADS) bit_set(s_dir, direct[i]);
  for (int i = tid; i < Q.n_walk; i += MB_THREADS) bit_set(s_walk, walk[i]);
  if (tid == 0) bit_set(s_dir, root);                             // directNeighborsOf inserts the frame itself (:437)
  __syncthreads();
  // c. mark the points: a wave per feature_table
  const int n_marking = mode == SVS_REG_LOOP ? 1 : Q.n_walk;
  for (int i = wave; i < n_marking; i += MB_THREADS / 64) {
    const int kf = walk[i];
    if (mode == SVS_REG_LOCAL && bit_of(s_dir, kf)) continue;      // (:485)
    const int e1 = M.kf_begin[kf + 1];
    for (int e = M.kf_begin[kf] + lane; e < e1; e += 64) {
      const int p = M.kf_rows[e];
      if ((unsigned)p < (unsigned)M.pt_hi) bit_set(mark, p);
    }
  }
  __syncthreads();
  // d. the source list: the set bits in ascending order (SB <= NP)
  const int n_src = list_marked(mark, n_words, D.point_id + (size_t)r * D.NP, 0, D.SB, s_w);
  const int n_src_c = min(n_src, D.SB);
  __syncthreads();
  // e. the records (four 16-byte loads each); their anchors join the table
  svs_candidate_point *src = D.src + (size_t)r * D.SB;
  for (int i = tid; i < n_src_c; i += MB_THREADS) {
    const int p = D.point_id[(size_t)r * D.NP + i];
    const int4 q = copy_rec64(src + i, M.pt + p);                  // kf_index: still the anchor's id (translated in g)
    if ((unsigned)q.y < (unsigned)MAP_MAX_KF) bit_set(s_tab, q.y);
  }
  __syncthreads();
  // f. the table: entry 0 the root, behind it anchors and walk keyframes in ascending id; the rank of a word's first bit by a prefix over the popcounts
  int n_kf;
  {
    uint32_t bits = s_tab[tid] | s_walk[tid];
    if (tid == (root >> 5)) bits &= ~(1u << (root & 31));
    s_tab[tid] = bits;                                            // a lane's own word
    int tot;
    const int rank = block_excl_scan(__popc(bits), s_w, tot);
    s_rank[tid] = rank;
    n_kf = 1 + tot;
    svs_keyframe *kfs = D.kfs + (size_t)r * D.KB;
    uint8_t *flags = D.flags + (size_t)r * D.KB;
    int32_t *kf_id = D.kf_id + (size_t)r * D.KB;
    for_each_set_bit(bits, tid << 5, 1 + rank, [&](int id, int e) {
      if (e < D.KB) {
        for (int k = 0; k < 17; ++k) reinterpret_cast<long long *>(kfs + e)[k] = reinterpret_cast<const long long *>(M.kf + id)[k];
        flags[e] = (uint8_t)((M.kf_flags[id] & SVS_REG_KF_IN_WINDOW) | (bit_of(s_dir, id) ? SVS_REG_KF_DIRECT_NEIGHBOR : 0));
        kf_id[e] = id;
      }
    });
    if (tid == 0) {                                               // KB >= 1
      for (int k = 0; k < 17; ++k) reinterpret_cast<long long *>(kfs)[k] = reinterpret_cast<const long long *>(M.kf + root)[k];
      flags[0] = (uint8_t)((M.kf_flags[root] & SVS_REG_KF_IN_WINDOW) | SVS_REG_KF_DIRECT_NEIGHBOR);
      kf_id[0] = root;
    }
    // behind the table: what the stateless call's staging holds there
    for (int k = min(n_kf, D.KB) + tid; k < D.KB; k += MB_THREADS) {
      for (int q = 0; q < 17; ++q) reinterpret_cast<long long *>(kfs + k)[q] = 0;
      flags[k] = 0;
    }
  }
  __syncthreads();
  // g. anchors as table entries; the observer rows
  int32_t *ob = D.obs_begin + (size_t)r * (D.SB + 1), *ok = D.obs_kf + (size_t)r * D.OB;
  int n_obs = 0;
  for (int base = 0; base < n_src_c; base += MB_THREADS) {      // block-uniform
    const int i = base + tid;
    int c = 0, p = -1, row_b = 0, row_e = 0;
    bool has_root = false;
    if (i < n_src_c) {
      const int a = src[i].kf_index;                              // written by this lane in e
      src[i].kf_index = a == root ? 0 : 1 + bit_rank(s_tab, s_rank, a);
      if (mode == SVS_REG_LOCAL) {
        p = D.point_id[(size_t)r * D.NP + i];
        row_b = M.pt_begin[p]; row_e = M.pt_begin[p + 1];
        row_each(M.pt_rows, row_b, row_e, [&](int kf) {
          if (kf == root) has_root = true;
          else if ((unsigned)kf < (unsigned)MAP_MAX_KF && bit_of(s_tab, kf)) ++c;
        });
        c += has_root ? 1 : 0;
      }
    }
    int tot;
    int pos = n_obs + block_excl_scan(c, s_w, tot);
    if (i < n_src_c && mode == SVS_REG_LOCAL) {
      ob[i] = pos;
      if (has_root) { if (pos < D.OB) ok[pos] = 0; ++pos; }
      row_each(M.pt_rows, row_b, row_e, [&](int kf) {              // ascending ids = ascending entries
        if (kf != root && (unsigned)kf < (unsigned)MAP_MAX_KF && bit_of(s_tab, kf)) {
          if (pos < D.OB) ok[pos] = 1 + bit_rank(s_tab, s_rank, kf);
          ++pos;
        }
      });
    }
    n_obs += tot;
  }
  const bool over = n_src > D.SB || n_kf > D.KB || n_obs > D.OB;
  if (tid == 0 && mode == SVS_REG_LOCAL) ob[n_src_c] = min(n_obs, D.OB);
  // h. the request record.  Over capacity: a request without points, which the chain answers at its first exit
  reg_hdr &H = D.hdr[r];
  for (int k = tid; k < THR_N; k += MB_THREADS) (&H.thr[0][0])[k] = M.kf_thr[(size_t)root * THR_N + k];
  if (tid < 12) H.T_root[tid] = Q.T_root[tid];
  if (tid == 0) {
    H.mode = mode; H.n_kf = over ? 1 : n_kf; H.n_src = over ? 0 : n_src; H.root_kf = 0;
    H.disp = M.kf_disp[root]; H.disp_stride = M.kf_dstride[root]; H.pad_ = 0;
    D.meta[r] = make_int4(n_kf, n_src, n_obs, over ? 1 : 0);
  }
}
}  // namespace

int svs_map_build_requests(svs_map *m, int n_requests, const MapBuildDst &dst) {
  svs_ctx *ctx = m->ctx;
  if (int rc = map_prepare_walk(m, n_requests)) return rc;
  hipLaunchKernelGGL(map_build_kernel, dim3(n_requests), dim3(MB_THREADS), 0, ctx->stream, m->view(), dst);
  SVS_LAUNCH_CHECK(ctx);
  return SVS_OK;
}
