// frontend_newpoints.inc -- the svs_frontend_newpoints_* entry points: newpoint_map resident per stream (the contract is in the header, the kernels in
// newpoints.hip).  Included at the end of frontend.hip, which defines svs_frontend.  The host holds the streams' (key, count) TABLES and decides every refusal and
// every layout from them; the records themselves are only ever moved on the device.

namespace {
constexpr int NPG = SVS_NEWPOINTS_MAX_GROUPS;

// a call's working copy of the tables of the streams it names: per group its key and the segments its records will come from, in order
struct NpGroup { int32_t key; std::vector<np_seg> segs; long long len; };      // len: its records (a seed segment counts with the most it can produce)
struct NpEdit {
  svs_frontend *fe;
  std::vector<int> streams;                     // in the order first named
  std::vector<std::vector<NpGroup>> groups;     // beside it
  explicit NpEdit(svs_frontend *f) : fe(f) {}
  std::vector<NpGroup> &of(int stream) {
    for (size_t i = 0; i < streams.size(); ++i)
      if (streams[i] == stream) return groups[i];
    streams.push_back(stream);
    groups.emplace_back();
    std::vector<NpGroup> &g = groups.back();
    int at = 0;
    for (int k = 0; k < fe->np_ng[stream]; ++k) {
      const int c = fe->np_cnt[(size_t)stream * NPG + k];
      NpGroup ng{fe->np_key[(size_t)stream * NPG + k], {}, c};
      if (c > 0) ng.segs.push_back(np_seg{NP_SEG_STORE, at, c, 0});
      g.push_back(std::move(ng));
      at += c;
    }
    return g;
  }
  // the group with this key, created at the end when absent; nullptr: the stream's table is full
  NpGroup *group(int stream, int32_t key) {
    std::vector<NpGroup> &g = of(stream);
    for (NpGroup &x : g)
      if (x.key == key) return &x;
    if ((int)g.size() >= fe->np_gcap) return nullptr;
    g.push_back(NpGroup{key, {}, 0});
    return &g.back();
  }
  long long records(int stream) {
    long long t = 0;
    for (const NpGroup &x : of(stream)) t += x.len;
    return t;
  }
};

int np_capacity(svs_ctx *ctx, const char *what) { ctx->err = what; return SVS_ERR_CAPACITY; }

// (every call of the staging block fe->np ends synchronised: its pinned side is free when the next one reserves it)
// ops | segments | the `n_staged` records of staged_parts, back to back, into the pinned block, uploaded, and the compose launch behind it
int np_apply(svs_frontend *fe, const NpEdit &e, size_t n_staged, const std::vector<std::pair<const svs_candidate_point *, int>> &staged_parts,
             const svs_candidate_point *d_seed_out, const int32_t *d_seed_cnt, int seed_cap) {
  svs_ctx *ctx = fe->ctx;
  const size_t n_ops = e.streams.size();
  if (n_ops == 0) return SVS_OK;
  size_t n_seg = 0;
  for (const auto &g : e.groups) for (const NpGroup &x : g) n_seg += x.segs.size();
  Pieces<> row;
  const auto p_ops = row.piece<np_op>(n_ops); const auto p_seg = row.piece<np_seg>(n_seg); const auto p_rec = row.piece<svs_candidate_point>(n_staged);
  TwinBlock &blk = fe->np;
  if (int rc = blk.reserve(ctx, row.end)) return rc;
  np_op *ops = blk.host(p_ops);
  np_seg *segs = blk.host(p_seg);
  svs_candidate_point *rec = blk.host(p_rec);
  size_t at = 0;
  for (size_t i = 0; i < n_ops; ++i) {
    np_op &o = ops[i];
    memset(&o, 0, sizeof o);
    o.stream = e.streams[i]; o.seg_off = (int32_t)at; o.n_groups = (int32_t)e.groups[i].size();
    for (size_t g = 0; g < e.groups[i].size(); ++g) {
      o.key[g] = e.groups[i][g].key;
      for (np_seg s : e.groups[i][g].segs) { s.group = (int32_t)g; segs[at++] = s; }
    }
    o.n_seg = (int32_t)at - o.seg_off;
  }
  size_t r = 0;
  for (const auto &p : staged_parts) {
    if (p.second) memcpy(rec + r, p.first, sizeof(svs_candidate_point) * (size_t)p.second);
    r += (size_t)p.second;
  }
  if (int rc = blk.upload(ctx, 0, row.end)) return rc;
  NpCompose c{};
  c.ops = blk.dev(p_ops); c.segs = blk.dev(p_seg); c.staged = blk.dev(p_rec);
  c.seed_out = d_seed_out; c.seed_cnt = d_seed_cnt; c.seed_cap = seed_cap;
  c.rec = fe->d_np_rec; c.tmp = fe->d_np_tmp; c.key = fe->d_np_key; c.cnt = fe->d_np_cnt; c.ng = fe->d_np_ng; c.record_cap = fe->np_rcap;
  return svs_newpoints_compose(ctx, (int)n_ops, c);
}

// the mirror follows an applied edit; h_n_new: the seed counts [requests][3] behind NP_SEG_SEED segments
void np_commit(svs_frontend *fe, const NpEdit &e, const int32_t *h_n_new) {
  for (size_t i = 0; i < e.streams.size(); ++i) {
    const int s = e.streams[i];
    const std::vector<NpGroup> &g = e.groups[i];
    fe->np_ng[s] = (int32_t)g.size();
    for (int k = 0; k < NPG; ++k) {
      int c = 0;
      if (k < (int)g.size())
        for (const np_seg &sg : g[k].segs) c += sg.kind == NP_SEG_SEED ? h_n_new[3 * sg.off] + h_n_new[3 * sg.off + 1] + h_n_new[3 * sg.off + 2] : sg.len;
      fe->np_key[(size_t)s * NPG + k] = k < (int)g.size() ? g[k].key : -1;
      fe->np_cnt[(size_t)s * NPG + k] = c;
    }
  }
}
}  // namespace

extern "C" int svs_frontend_newpoints_reserve(svs_frontend *fe, int record_cap, int group_cap) {
  svs_ctx *ctx = fe ? fe->ctx : nullptr;
  SVS_REQUIRE(ctx, fe && record_cap >= 1 && group_cap >= 1 && group_cap <= NPG && !fe->submitted && fe->np_rcap == 0);
  SVS_DEVICE(ctx);
  const size_t B = (size_t)fe->B;
  SVS_HIP(ctx, fe->d_np_rec.alloc(B * record_cap));
  SVS_HIP(ctx, fe->d_np_tmp.alloc(B * record_cap));
  SVS_HIP(ctx, fe->d_np_key.alloc(B * NPG));
  SVS_HIP(ctx, fe->d_np_cnt.alloc(B * NPG));
  SVS_HIP(ctx, fe->d_np_ng.alloc(B));
  SVS_HIP(ctx, fe->d_np_removed.alloc(B));
  SVS_HIP(ctx, hipMemsetAsync(fe->d_np_rec, 0, sizeof(svs_candidate_point) * B * record_cap, ctx->stream));
  SVS_HIP(ctx, hipMemsetAsync(fe->d_np_key, 0xff, sizeof(int32_t) * B * NPG, ctx->stream));
  SVS_HIP(ctx, hipMemsetAsync(fe->d_np_cnt, 0, sizeof(int32_t) * B * NPG, ctx->stream));
  SVS_HIP(ctx, hipMemsetAsync(fe->d_np_ng, 0, sizeof(int32_t) * B, ctx->stream));
  SVS_HIP(ctx, hipStreamSynchronize(ctx->stream));
  fe->np_key.assign(B * NPG, -1); fe->np_cnt.assign(B * NPG, 0); fe->np_ng.assign(B, 0);
  fe->np_rcap = record_cap; fe->np_gcap = group_cap;
  return SVS_OK;
}

extern "C" int svs_frontend_newpoints_put(svs_frontend *fe, int n_requests, const svs_newpoints_put_request *req) {
  svs_ctx *ctx = fe ? fe->ctx : nullptr;
  SVS_REQUIRE(ctx, fe && fe->np_rcap > 0 && !fe->submitted && n_requests >= 0 && (n_requests == 0 || req));
  NpEdit e(fe);
  std::vector<std::pair<const svs_candidate_point *, int>> parts;
  size_t n_staged = 0;
  for (int r = 0; r < n_requests; ++r) {
    const svs_newpoints_put_request &q = req[r];
    SVS_REQUIRE(ctx, q.stream >= 0 && q.stream < fe->B && q.kf_id >= 0 && (q.mode == SVS_NEWPOINTS_PREPEND || q.mode == SVS_NEWPOINTS_REPLACE) && q.n >= 0 &&
                         (q.n == 0 || q.h_records));
    NpGroup *g = e.group(q.stream, q.kf_id);
    if (!g) return np_capacity(ctx, "svs_frontend_newpoints_put: more groups than group_cap");
    if (q.mode == SVS_NEWPOINTS_REPLACE) { g->segs.clear(); g->len = 0; }
    if (q.n) {
      g->segs.insert(g->segs.begin(), np_seg{NP_SEG_STAGED, (int32_t)n_staged, q.n, 0});
      g->len += q.n;
      parts.emplace_back(q.h_records, q.n);
      n_staged += (size_t)q.n;
    }
    if (e.records(q.stream) > fe->np_rcap) return np_capacity(ctx, "svs_frontend_newpoints_put: more records than record_cap");
  }
  if (n_requests == 0) return SVS_OK;
  SVS_DEVICE(ctx);
  if (int rc = np_apply(fe, e, n_staged, parts, nullptr, nullptr, 0)) return rc;
  SVS_HIP(ctx, hipStreamSynchronize(ctx->stream));
  np_commit(fe, e, nullptr);
  return SVS_OK;
}

extern "C" int svs_frontend_newpoints_drop_groups(svs_frontend *fe, int n_requests, const svs_newpoints_drop_request *req, int32_t *h_n_found) {
  svs_ctx *ctx = fe ? fe->ctx : nullptr;
  SVS_REQUIRE(ctx, fe && fe->np_rcap > 0 && !fe->submitted && n_requests >= 0 && (n_requests == 0 || (req && h_n_found)));
  for (int r = 0; r < n_requests; ++r) SVS_REQUIRE(ctx, req[r].stream >= 0 && req[r].stream < fe->B && req[r].n_keys >= 0 && (req[r].n_keys == 0 || req[r].h_keys));
  NpEdit e(fe);
  for (int r = 0; r < n_requests; ++r) {
    std::vector<NpGroup> &g = e.of(req[r].stream);
    int found = 0;
    for (int k = 0; k < req[r].n_keys; ++k)
      for (size_t i = 0; i < g.size(); ++i)
        if (g[i].key == req[r].h_keys[k]) { g.erase(g.begin() + (long)i); ++found; break; }
    h_n_found[r] = found;
  }
  if (n_requests == 0) return SVS_OK;
  SVS_DEVICE(ctx);
  if (int rc = np_apply(fe, e, 0, {}, nullptr, nullptr, 0)) return rc;
  SVS_HIP(ctx, hipStreamSynchronize(ctx->stream));
  np_commit(fe, e, nullptr);
  return SVS_OK;
}

namespace {
struct NpSeedSink : SeedSink {
  svs_frontend *fe; int n; const svs_seed_request *req; const int32_t *kf_id; int max_rec;
  NpEdit e;
  NpSeedSink(svs_frontend *f, int n_, const svs_seed_request *r, const int32_t *k, int m) : fe(f), n(n_), req(r), kf_id(k), max_rec(m), e(f) {}
  int check() override {      // (the requests' streams are in range: checked in front of this)
    svs_ctx *ctx = fe->ctx;
    for (int r = 0; r < n; ++r) {
      SVS_REQUIRE(ctx, kf_id[r] >= 0);
      NpGroup *g = e.group(req[r].stream, kf_id[r]);
      if (!g) return np_capacity(ctx, "svs_frontend_seed_newpoints: more groups than group_cap");
      g->segs.insert(g->segs.begin(), np_seg{NP_SEG_SEED, r, 0, 0});
      g->len += max_rec;
      if (e.records(req[r].stream) > fe->np_rcap) return np_capacity(ctx, "svs_frontend_seed_newpoints: the records a request can produce do not fit record_cap");
    }
    return SVS_OK;
  }
  int enqueue(const svs_candidate_point *d_rec, const int32_t *d_cnt, int cap) override { return np_apply(fe, e, 0, {}, d_rec, d_cnt, cap); }
};
}  // namespace

extern "C" int svs_frontend_seed_newpoints(svs_frontend *fe, int n, const svs_seed_request *req, const int32_t *h_kf_id, const svs_seed_params *prm, int32_t *h_n_new,
                                           svs_candidate_point *h_out, int cap_per_request) {
  svs_ctx *ctx = fe ? fe->ctx : nullptr;
  SVS_REQUIRE(ctx, fe && fe->np_rcap > 0 && prm && n >= 0 && (n == 0 || (req && h_kf_id && h_n_new)));
  const int max_rec = svs_seed_max_records(prm);
  if (!h_out) cap_per_request = max_rec;
  NpSeedSink sink(fe, n, req, h_kf_id, max_rec);
  if (int rc = fe_seed_keyframes(fe, n, req, prm, h_out, cap_per_request, h_n_new, &sink)) return rc;      // (blocking: the counts are home)
  if (n > 0) np_commit(fe, sink.e, h_n_new);
  return SVS_OK;
}

extern "C" int svs_frontend_newpoints_prune(svs_frontend *fe, int n_streams, const int32_t *h_streams, int32_t *h_n_removed, int32_t *h_group_count) {
  svs_ctx *ctx = fe ? fe->ctx : nullptr;
  SVS_REQUIRE(ctx, fe && fe->np_rcap > 0 && !fe->submitted && fe->have_prev && n_streams >= 0 && n_streams <= fe->B && (n_streams == 0 || (h_streams && h_n_removed)));
  SVS_REQUIRE(ctx, fe->n_gated >= 0);      // the records of a step on the list that is still on the device (the SVS_SEED_MORE rule)
  {
    std::vector<uint8_t> named((size_t)fe->B, 0);
    for (int i = 0; i < n_streams; ++i) {
      SVS_REQUIRE(ctx, h_streams[i] >= 0 && h_streams[i] < fe->B && !named[h_streams[i]]);
      named[h_streams[i]] = 1;
    }
  }
  if (n_streams == 0) return SVS_OK;
  SVS_DEVICE(ctx);
  const size_t B = (size_t)fe->B, mp = (size_t)fe->max_points;
  // the streams go up; the removed counts and the whole count table come home into the pinned side from the arrays the kernel writes
  Pieces<> row;
  const auto p_str = row.piece<int32_t>((size_t)n_streams); const auto p_rem = row.piece<int32_t>((size_t)n_streams); const auto p_cnt = row.piece<int32_t>(B * NPG);
  TwinBlock &blk = fe->np;
  if (int rc = blk.reserve(ctx, row.end)) return rc;
  memcpy(blk.host(p_str), h_streams, p_str.bytes());
  if (int rc = blk.upload(ctx, 0, p_str.end())) return rc;
  svs_newpoints_prune_args a{};
  a.d_res = fe->d_res; a.res_bstride = mp; a.d_pts = fe->d_pts; a.pts_bstride = mp; a.d_gated = fe->d_gated; a.gated_bstride = mp;
  a.d_n_new = fe->d_n_new; a.n = fe->n_gated; a.batch = n_streams;
  a.d_store = fe->d_np_rec; a.store_bstride = (size_t)fe->np_rcap; a.d_group_count = fe->d_np_cnt; a.group_bstride = NPG; a.d_n_groups = fe->d_np_ng;
  a.d_stream = blk.dev(p_str);
  if (int rc = svs_newpoints_prune(ctx, &a, fe->d_np_removed)) return rc;
  SVS_HIP(ctx, hipMemcpyAsync(blk.host(p_rem), fe->d_np_removed, p_rem.bytes(), hipMemcpyDeviceToHost, ctx->stream));
  SVS_HIP(ctx, hipMemcpyAsync(blk.host(p_cnt), fe->d_np_cnt, p_cnt.bytes(), hipMemcpyDeviceToHost, ctx->stream));
  SVS_HIP(ctx, hipStreamSynchronize(ctx->stream));
  const int32_t *cnt = blk.host(p_cnt);
  memcpy(h_n_removed, blk.host(p_rem), p_rem.bytes());
  for (int i = 0; i < n_streams; ++i) {
    const size_t s = (size_t)h_streams[i];
    memcpy(&fe->np_cnt[s * NPG], cnt + s * NPG, sizeof(int32_t) * NPG);
    if (h_group_count) memcpy(h_group_count + (size_t)i * NPG, cnt + s * NPG, sizeof(int32_t) * NPG);
  }
  return SVS_OK;
}

extern "C" int svs_frontend_newpoints_get(svs_frontend *fe, int n_streams, const int32_t *h_streams, int32_t *h_n_groups, int32_t *h_keys, int32_t *h_counts,
                                          svs_candidate_point *h_records) {
  svs_ctx *ctx = fe ? fe->ctx : nullptr;
  SVS_REQUIRE(ctx, fe && fe->np_rcap > 0 && n_streams >= 0 && (n_streams == 0 || h_streams));
  for (int i = 0; i < n_streams; ++i) SVS_REQUIRE(ctx, h_streams[i] >= 0 && h_streams[i] < fe->B);
  if (n_streams == 0) return SVS_OK;
  SVS_DEVICE(ctx);
  const size_t B = (size_t)fe->B;
  Pieces<> row;      // the three tables, into the pinned side
  const auto p_key = row.piece<int32_t>(B * NPG); const auto p_cnt = row.piece<int32_t>(B * NPG); const auto p_ng = row.piece<int32_t>(B);
  TwinBlock &blk = fe->np;
  if (int rc = blk.reserve(ctx, row.end)) return rc;
  SVS_HIP(ctx, hipMemcpyAsync(blk.host(p_key), fe->d_np_key, p_key.bytes(), hipMemcpyDeviceToHost, ctx->stream));
  SVS_HIP(ctx, hipMemcpyAsync(blk.host(p_cnt), fe->d_np_cnt, p_cnt.bytes(), hipMemcpyDeviceToHost, ctx->stream));
  SVS_HIP(ctx, hipMemcpyAsync(blk.host(p_ng), fe->d_np_ng, p_ng.bytes(), hipMemcpyDeviceToHost, ctx->stream));
  if (h_records)
    for (int i = 0; i < n_streams; ++i)
      SVS_HIP(ctx, hipMemcpyAsync(h_records + (size_t)i * fe->np_rcap, fe->d_np_rec + (size_t)h_streams[i] * fe->np_rcap, sizeof(svs_candidate_point) * (size_t)fe->np_rcap,
                                  hipMemcpyDeviceToHost, ctx->stream));
  SVS_HIP(ctx, hipStreamSynchronize(ctx->stream));
  const int32_t *key = blk.host(p_key), *cnt = blk.host(p_cnt), *ng = blk.host(p_ng);
  for (int i = 0; i < n_streams; ++i) {
    const size_t s = (size_t)h_streams[i];
    if (h_n_groups) h_n_groups[i] = ng[s];
    if (h_keys) memcpy(h_keys + (size_t)i * NPG, key + s * NPG, sizeof(int32_t) * NPG);
    if (h_counts) memcpy(h_counts + (size_t)i * NPG, cnt + s * NPG, sizeof(int32_t) * NPG);
  }
  return SVS_OK;
}

extern "C" int svs_frontend_set_candidates_from_newpoints(svs_frontend *fe, int n_requests, const svs_newpoints_list_request *req, svs_newpoints_list_result *h_res,
                                                          svs_candidate_point *h_records, int32_t *h_group_end) {
  svs_ctx *ctx = fe ? fe->ctx : nullptr;
  SVS_REQUIRE(ctx, fe && fe->np_rcap > 0 && !fe->submitted && n_requests >= 0 && n_requests <= fe->B && (n_requests == 0 || req));
  const int R = n_requests, B = fe->B, K = fe->max_keyframes, MP = fe->max_points;
  std::vector<np_list_req> staged;              // the requests that fit
  std::vector<int> staged_r;
  std::vector<svs_newpoints_list_result> res((size_t)R);
  size_t n_tail = 0;
  {
    std::vector<uint8_t> named((size_t)B, 0);
    std::vector<int32_t> sorted;
    for (int r = 0; r < R; ++r) {
      const svs_newpoints_list_request &q = req[r];
      SVS_REQUIRE(ctx, q.stream >= 0 && q.stream < B && !named[q.stream]);
      named[q.stream] = 1;
      SVS_REQUIRE(ctx, q.n_keys >= 1 && q.h_keys && q.h_slot_kf && q.n_tail >= 0 && q.n_tail <= MP && (q.n_tail == 0 || q.h_tail));
      if (q.n_keys > NPG - 1) return np_capacity(ctx, "svs_frontend_set_candidates_from_newpoints: more than 63 keys");
      sorted.assign(q.h_keys, q.h_keys + q.n_keys);
      SVS_REQUIRE(ctx, all_distinct(sorted) && sorted[0] >= 0);
      if (int rc = fe_check_slot_table(fe, q.stream, q.h_slot_kf, sorted)) return rc;
      if (int rc = fe_check_anchors(fe, q.stream, q.h_tail, q.n_tail)) return rc;
      // the groups named, where they lie in the stream's row
      np_list_req s;
      memset(&s, 0, sizeof s);
      s.stream = q.stream; s.n_seg = q.n_keys + 1; s.prev_len = fe->n_points[q.stream];
      svs_newpoints_list_result &o = res[r];
      memset(&o, 0, sizeof o);
      for (int k = 0; k < q.n_keys; ++k) {
        np_list_seg &sg = s.seg[k];
        sg.kind = NP_SEG_STORE; sg.kf_index = -1;
        for (int sl = 0; sl < K; ++sl)
          if (q.h_slot_kf[sl] == q.h_keys[k]) sg.kf_index = sl;
        int at = 0;
        for (int g = 0; g < fe->np_ng[q.stream]; ++g) {
          const int c = fe->np_cnt[(size_t)q.stream * NPG + g];
          if (fe->np_key[(size_t)q.stream * NPG + g] == q.h_keys[k]) { sg.off = at; sg.len = c; }
          at += c;
        }
        o.n_head += sg.len;
        if (sg.kf_index < 0) o.n_no_slot += sg.len;
      }
      s.seg[q.n_keys] = np_list_seg{NP_SEG_STAGED, (int32_t)n_tail, q.n_tail, 0};
      o.n_points = o.n_head + q.n_tail; o.n_groups = q.n_keys + 1;
      if (o.n_points > MP) { o.over_capacity = 1; o.n_no_slot = 0; continue; }
      staged.push_back(s); staged_r.push_back(r);
      n_tail += (size_t)q.n_tail;
    }
  }
  if (h_res) for (int r = 0; r < R; ++r) h_res[r] = res[r];
  if (R == 0) return SVS_OK;
  SVS_DEVICE(ctx);
  if (!staged.empty()) {
    Pieces<> row;
    const auto p_req = row.piece<np_list_req>(staged.size()); const auto p_tail = row.piece<svs_candidate_point>(n_tail);
    TwinBlock &blk = fe->np;
    if (int rc = blk.reserve(ctx, row.end)) return rc;
    memcpy(blk.host(p_req), staged.data(), p_req.bytes());
    svs_candidate_point *tail = blk.host(p_tail);
    for (size_t i = 0; i < staged.size(); ++i) {
      const svs_newpoints_list_request &q = req[staged_r[i]];
      if (q.n_tail) memcpy(tail + staged[i].seg[q.n_keys].off, q.h_tail, sizeof(svs_candidate_point) * (size_t)q.n_tail);
    }
    if (int rc = blk.upload(ctx, 0, row.end)) return rc;
    NpList L{};
    L.req = blk.dev(p_req); L.staged = blk.dev(p_tail);
    L.rec = fe->d_np_rec; L.record_cap = fe->np_rcap;
    L.pts = fe->d_pts; L.max_points = MP; L.group_end = fe->d_group_end; L.n_groups = fe->d_n_groups; L.n_new = fe->d_n_new;
    if (int rc = svs_newpoints_list(ctx, (int)staged.size(), L)) return rc;
  }
  if (h_records) SVS_HIP(ctx, hipMemcpyAsync(h_records, fe->d_pts, sizeof(svs_candidate_point) * (size_t)MP * B, hipMemcpyDeviceToHost, ctx->stream));
  if (h_group_end) SVS_HIP(ctx, hipMemcpyAsync(h_group_end, fe->d_group_end, sizeof(int32_t) * (size_t)MAX_GROUPS * B, hipMemcpyDeviceToHost, ctx->stream));
  SVS_HIP(ctx, hipStreamSynchronize(ctx->stream));
  for (size_t i = 0; i < staged.size(); ++i) {
    const int r = staged_r[i], s = req[r].stream;
    fe->n_points[s] = res[r].n_points; fe->n_new_records[s] = res[r].n_head;
    fe->max_groups_used = std::max(fe->max_groups_used, res[r].n_groups);
  }
  if (!staged.empty()) fe_lists_changed(fe);
  return SVS_OK;
}
