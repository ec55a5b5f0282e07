// keyframe.hip -- the keyframe logic behind a front-end step (svs_keyframe_decide, svs_frontend_decide_keyframes): processMatchedPoints' two AddToOptimzer lists
// (stereo_frontend.cpp:859-968), shallWeSwitchKeyframe (:446-510), shallWeDropNewKeyframe (:512-528) and the bookkeeping of addNewKeyframe (:316-415), decided on
// the device from the records, statistics and pose a step left there.  The contract is in the header; tests/keyframe_model.py restates it.
//   keyframe_decide_kernel   one workgroup (four waves) per stream.  The lists are an ordered compaction of the record array: per 256-record chunk two ballots, the
//                   waves' popcounts through LDS, a running offset -- an entry's place is its rank among the accepted records, whatever the waves' timing.  The
//                   switch test is one lane per vertex (pose.h, f64) and a serial scan of at most 64 distances by one lane, which IS the reference's loop over
//                   vertex_map in table order.  Set membership is a binary search, in the stream's staged ascending id array or in the map's by-point observer
//                   row (kf_map.h); the counts are integer sums in LDS.  strength_to_neighbors is ranked by counting the smaller (count, id) pairs.
//   keyframe_scatter_kernel  svs_frontend_set_vertex_table's staged requests into the stream-indexed resident tables, word copies.
// Reads the front end's state only.
#include "keyframe.h"
#include "kf_map.h"
#include "pose.h"

namespace {
constexpr int KD_THREADS = 256, KD_WAVES = KD_THREADS / 64;
constexpr int KD_MAX_KEYS = SVS_KF_MAX_SLOTS + SVS_KF_MAX_VERTICES;
constexpr int DEC_WORDS = sizeof(svs_keyframe_decision) / 4;
static_assert(sizeof(svs_keyframe_decision) == 800 && sizeof(svs_kf_vertex) == 112 && sizeof(svs_kf_table) == 272, "word copies below");
static_assert(sizeof(svs_map_new_point) == 96 && sizeof(svs_map_track_point) == 32, "the record types svs_map_add_keyframe takes");

struct KdK {
  svs_keyframe_decide_args a;
  svs_keyframe_decide_params p;
  MapObsView M;
  KfdFrontendSrc fs; int have_fs;
  svs_keyframe_decision *dec; svs_map_new_point *nw; svs_map_track_point *tr; int32_t *nw_rec, *tr_rec; int cap;
};

// is `id` in F(v): the staged range [beg, beg + cnt) of `ids` (strictly ascending), or the map's observer row of the point
__device__ __forceinline__ bool in_feature_set(const MapObsView &M, const int32_t *__restrict__ ids, int kf, int beg, int cnt, int id) {
  if (beg == SVS_KF_SET_MAP) return map_point_seen_by(M, id, kf);
  int lo = beg, hi = beg + cnt;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1, v = ids[mid];
    if (v == id) return true;
    if (v < id) lo = mid + 1; else hi = mid;
  }
  return false;
}

__device__ __forceinline__ double translation_norm(const double *T) { return sqrt((T[3] * T[3] + T[7] * T[7]) + T[11] * T[11]); }

__global__ __launch_bounds__(KD_THREADS) void keyframe_decide_kernel(KdK K) {
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  __shared__ svs_keyframe_decision s_dec;
  __shared__ double s_Tdiff[SVS_KF_MAX_VERTICES][12];
  __shared__ double s_dist[SVS_KF_MAX_VERTICES], s_Tcur[12], s_Tact[12];
  __shared__ int s_vkf[SVS_KF_MAX_VERTICES], s_vbeg[SVS_KF_MAX_VERTICES], s_vcnt[SVS_KF_MAX_VERTICES];
  __shared__ int s_key[SVS_KF_MAX_VERTICES], s_keycnt[SVS_KF_MAX_VERTICES];      // act (0) and its neighbours (1 ..): vertex index, track entries in F
  __shared__ int s_slot_id[SVS_KF_MAX_SLOTS], s_slot_cnt[SVS_KF_MAX_SLOTS];
  __shared__ int s_ecnt[KD_MAX_KEYS], s_eid[KD_MAX_KEYS];
  __shared__ int s_wave[2][KD_WAVES];
  __shared__ int s_bad, s_best, s_shared, s_decision, s_nstrength;

  const svs_keyframe_decide_args &A = K.a;
  for (int i = tid; i < DEC_WORDS; i += KD_THREADS) reinterpret_cast<int32_t *>(&s_dec)[i] = 0;
  if (tid == 0) { s_bad = 0; s_shared = 0; s_nstrength = 0; s_best = -1; s_decision = SVS_KF_KEEP; }
  __syncthreads();

  // rule 0: the stream was tracked, and its table can be walked without leaving it
  const svs_kf_table *tab = A.d_table + b;
  const int V = tab->n_vertex, act = tab->act, NN = tab->n_neighbors, S = A.max_keyframes;
  const svs_kf_vertex *vtx = A.d_vertex + (size_t)b * A.vertex_bstride;
  const int32_t *ids = A.d_set_ids + (size_t)b * A.set_bstride;
  bool ok = K.have_fs ? (K.fs.pstats[b].num_obs >= K.fs.min_matches && K.fs.passes[b] >= 0) : A.d_tracking_ok[b] != 0;
  ok = ok && V >= 1 && V <= SVS_KF_MAX_VERTICES && (size_t)V <= A.vertex_bstride && act >= 0 && act < V && NN >= 0 && NN < V;
  if (ok) {      // (block-uniform)
    if (tid < V) {
      const int beg = vtx[tid].set_begin, cnt = vtx[tid].set_count;
      s_vkf[tid] = vtx[tid].kf_id; s_vbeg[tid] = beg; s_vcnt[tid] = cnt;
      if (beg != SVS_KF_SET_MAP && (beg < 0 || cnt < 0 || (size_t)beg + (size_t)cnt > A.set_bstride)) s_bad = 1;
    }
    if (tid < NN) {
      const int v = tab->neighbors[tid];
      if (v < 0 || v >= V || v == act) s_bad = 1;
      s_key[1 + tid] = v;
    }
    if (tid == 0) s_key[0] = act;
    if (tid < 12) { s_Tcur[tid] = A.d_T_cur_from_actkey[(size_t)b * 12 + tid]; s_Tact[tid] = vtx[act].T_me_from_w[tid]; }
    for (int s = tid; s < S; s += KD_THREADS) { s_slot_id[s] = A.d_slot_kf[(size_t)b * A.slot_bstride + s]; s_slot_cnt[s] = 0; }
  }
  __syncthreads();
  if (!ok || s_bad) {
    for (int i = tid; i < DEC_WORDS; i += KD_THREADS) reinterpret_cast<int32_t *>(K.dec + b)[i] = 0;
    return;
  }
  const int NK = 1 + NN;      // act and its neighbours

  // rule 1: the two lists, in record order
  int n = A.d_n ? A.d_n[b] : A.n;
  n = n < 0 ? 0 : (n > A.n ? A.n : n);      // A.n <= cap: the host checked
  const svs_match_result *res = A.d_res + (size_t)b * A.res_bstride;
  const svs_candidate_point *pts = A.d_pts + (size_t)b * A.pts_bstride;
  const svs_gated_point *gated = A.d_gated + (size_t)b * A.gated_bstride;
  svs_map_new_point *nw = K.nw + (size_t)b * K.cap;
  svs_map_track_point *tr = K.tr + (size_t)b * K.cap;
  int32_t *nw_rec = K.nw_rec + (size_t)b * K.cap, *tr_rec = K.tr_rec + (size_t)b * K.cap;
  int n_new = 0, n_track = 0;
  for (int base = 0; base < n; base += KD_THREADS) {      // block-uniform
    const int i = base + tid;
    bool is_n = false, is_t = false;
    if (i < n && res[i].status == SVS_MATCH_OK && gated[i].accepted != 0) {
      is_n = gated[i].is_new != 0; is_t = !is_n;
    }
    const unsigned long long mn = __ballot(is_n), mt = __ballot(is_t);
    if (lane == 0) { s_wave[0][wave] = __popcll(mn); s_wave[1][wave] = __popcll(mt); }
    __syncthreads();
    int on = n_new, ot = n_track;
#pragma unroll
    for (int w = 0; w < KD_WAVES; ++w) {
      const int cn = s_wave[0][w], ct = s_wave[1][w];
      if (w < wave) { on += cn; ot += ct; }
      n_new += cn; n_track += ct;
    }
    __syncthreads();
    const unsigned long long below = (1ull << lane) - 1ull;
    if (is_n || is_t) {
      const svs_candidate_point c = pts[i];
      const double o0 = res[i].obs[0], o1 = res[i].obs[1], o2 = res[i].obs[2];
      if (is_n) {
        const int pos = on + __popcll(mn & below);
        const bool in = c.kf_index >= 0 && c.kf_index < S;
        svs_map_new_point q;
        for (int k = 0; k < 3; ++k) { q.xyz_anchor[k] = c.xyz_anchor[k]; q.anchor_obs_pyr[k] = c.anchor_obs_pyr[k]; }
        q.feat_center[0] = o0; q.feat_center[1] = o1; q.feat_center[2] = o2;
        q.point_id = c.point_id; q.anchor_id = in ? s_slot_id[c.kf_index] : -1; q.anchor_level = c.anchor_level; q.feat_level = c.anchor_level;
        q.pad_[0] = q.pad_[1] = 0;
        nw[pos] = q; nw_rec[pos] = i;
        if (in) atomicAdd(&s_slot_cnt[c.kf_index], 1);
      } else {
        const int pos = ot + __popcll(mt & below);
        svs_map_track_point q;
        q.center[0] = o0; q.center[1] = o1; q.center[2] = o2;
        q.global_id = c.point_id; q.level = c.anchor_level;
        tr[pos] = q; tr_rec[pos] = i;
      }
    }
  }

  // rule 2: the vertex nearest to the current pose, one lane per vertex
  if (tid < V) {
    double d = __longlong_as_double(0x7ff8000000000000LL);
    if (tid != act) {
      double Tv[12], P[12], Inv[12], D[12];
      for (int k = 0; k < 12; ++k) Tv[k] = vtx[tid].T_me_from_w[k];
      pose_mul(s_Tcur, s_Tact, P);
      pose_inv(Tv, Inv);
      pose_mul(P, Inv, D);
      for (int k = 0; k < 12; ++k) s_Tdiff[tid][k] = D[k];
      d = translation_norm(D);
    }
    s_dist[tid] = d;
  }
  __syncthreads();      // (also: the lists are written)
  if (tid == 0) {       // the reference's loop, in table order: strict <, so the first of equal distances stays
    double md = 0.5 * (double)K.p.parallax_thr;
    int best = -1;
    for (int v = 0; v < V; ++v)
      if (v != act && s_dist[v] < md) { md = s_dist[v]; best = v; }
    s_best = best;
  }
  __syncthreads();
  const int best = s_best;
  if (best >= 0) {
    const int kf = s_vkf[best], beg = s_vbeg[best], cnt = s_vcnt[best];
    int c = 0;
    for (int t = tid; t < n_track; t += KD_THREADS) c += in_feature_set(K.M, ids, kf, beg, cnt, tr[t].global_id) ? 1 : 0;
    if (c) atomicAdd(&s_shared, c);
  }
  __syncthreads();

  // rules 2 - 4: the decision and its scalars
  if (tid == 0) {
    svs_keyframe_decision &d = s_dec;
    const svs_point_stats st = A.d_stats[b];
    d.valid = 1; d.n_new = n_new; d.n_track = n_track;
    d.closest_index = best; d.closest_id = best >= 0 ? s_vkf[best] : -1; d.closest_dist = best >= 0 ? s_dist[best] : 0.0; d.shared = s_shared;
    if (best >= 0 && s_shared > K.p.switch_min_shared) {
      d.decision = SVS_KF_SWITCH;
      for (int k = 0; k < 12; ++k) d.T_cur_after[k] = s_Tdiff[best][k];
    } else {
      int featureless = 0;
      for (int k = 0; k < 4; ++k) featureless += st.num_points_grid2x2[k] < K.p.featureless_cell_min ? 1 : 0;
      double av = st.sum_track_length / (double)st.num_track_points;
      if (av != av) av = __longlong_as_double(0x7ff8000000000000LL);
      d.featureless = featureless; d.av_track_length = av;
      const bool drop = featureless > K.p.featureless_corners_thr || translation_norm(s_Tcur) > (double)K.p.parallax_thr || av > K.p.max_av_track_length;
      if (drop) {
        d.decision = SVS_KF_DROP;
        for (int k = 0; k < 9; ++k) d.add_flags[k] = st.num_points_grid3x3[k] <= K.p.min_num_points ? 1 : 0;
        double P[12];
        pose_mul(s_Tcur, s_Tact, P);
        for (int k = 0; k < 12; ++k) { d.T_newkey_from_w[k] = P[k]; d.T_cur_after[k] = (k % 5 == 0) ? 1.0 : 0.0; }
      } else {
        d.decision = SVS_KF_KEEP;
        for (int k = 0; k < 12; ++k) d.T_cur_after[k] = s_Tcur[k];
      }
    }
    s_decision = d.decision;
  }
  if (tid < NK) s_keycnt[tid] = 0;
  __syncthreads();

  // rule 4: num_matches and strength_to_neighbors
  if (s_decision == SVS_KF_DROP) {      // block-uniform
    for (int t = tid; t < n_track; t += KD_THREADS) {
      const int id = tr[t].global_id;
      for (int k = 0; k < NK; ++k) {
        const int v = s_key[k];
        if (in_feature_set(K.M, ids, s_vkf[v], s_vbeg[v], s_vcnt[v], id)) atomicAdd(&s_keycnt[k], 1);
      }
    }
    __syncthreads();
    // one entry per distinct key: the lowest slot holding the id, else the first of act / neighbours with it
    const int E = S + NK;
    for (int e = tid; e < E; e += KD_THREADS) {
      int total = 0, id = 0;
      bool owner = false;
      if (e < S) {
        id = s_slot_id[e];
        owner = s_slot_cnt[e] > 0 && id >= 0;
        for (int s = 0; s < S && owner; ++s)
          if (s_slot_cnt[s] > 0 && s_slot_id[s] == id) { if (s < e) owner = false; total += s_slot_cnt[s]; }
        for (int k = 0; k < NK && owner; ++k)
          if (s_vkf[s_key[k]] == id) total += s_keycnt[k];
      } else {
        const int k0 = e - S;
        id = s_vkf[s_key[k0]];
        owner = true;
        for (int s = 0; s < S && owner; ++s)
          if (s_slot_cnt[s] > 0 && s_slot_id[s] == id) owner = false;
        for (int k = 0; k < NK && owner; ++k)
          if (s_vkf[s_key[k]] == id) { if (k < k0) owner = false; total += s_keycnt[k]; }
      }
      const bool q = owner && total > K.p.covis_thr;
      s_ecnt[e] = q ? total : 0; s_eid[e] = id;
      if (q) atomicAdd(&s_nstrength, 1);
    }
    __syncthreads();
    const int ns = s_nstrength;
    if (ns > SVS_KF_MAX_STRENGTH) {
      if (tid == 0) s_dec.over_capacity = 1;
    } else {
      if (tid == 0) s_dec.n_strength = ns;
      for (int e = tid; e < E; e += KD_THREADS) {
        const int c = s_ecnt[e], id = s_eid[e];
        if (c <= 0) continue;      // (covis_thr >= 0: a qualifying count is positive)
        int rank = 0;
        for (int f = 0; f < E; ++f) {
          const int cf = s_ecnt[f];
          rank += (cf > 0 && (cf < c || (cf == c && s_eid[f] < id))) ? 1 : 0;
        }
        s_dec.strength_kf[rank] = id; s_dec.strength_count[rank] = c;
      }
    }
  }
  __syncthreads();
  for (int i = tid; i < DEC_WORDS; i += KD_THREADS) reinterpret_cast<int32_t *>(K.dec + b)[i] = reinterpret_cast<const int32_t *>(&s_dec)[i];
}

__device__ __forceinline__ void copy_words(void *dst, const void *src, int n_words) {
  for (int i = threadIdx.x; i < n_words; i += KD_THREADS) reinterpret_cast<int32_t *>(dst)[i] = reinterpret_cast<const int32_t *>(src)[i];
}
__global__ __launch_bounds__(KD_THREADS) void keyframe_scatter_kernel(KfdScatter s) {
  const int r = blockIdx.x;
  const kfd_up u = s.up[r];      // the host checked: stream < B, n_ids <= set_cap
  copy_words(s.d_tab + u.stream, s.tab + r, sizeof(svs_kf_table) / 4);
  copy_words(s.d_vtx + (size_t)u.stream * SVS_KF_MAX_VERTICES, s.vtx + (size_t)r * SVS_KF_MAX_VERTICES, SVS_KF_MAX_VERTICES * (int)(sizeof(svs_kf_vertex) / 4));
  copy_words(s.d_slot + (size_t)u.stream * s.S, s.slot + (size_t)r * s.S, s.S);
  copy_words(s.d_ids + (size_t)u.stream * s.set_cap, s.ids + u.ids_off, u.n_ids);
}
}  // namespace

extern "C" void svs_keyframe_decide_params_default(svs_keyframe_decide_params *p) {
  if (!p) return;
  p->parallax_thr = 0.75f; p->switch_min_shared = 100; p->featureless_cell_min = 15; p->featureless_corners_thr = 2;
  p->max_av_track_length = 75.0; p->covis_thr = 15; p->min_num_points = 25;
}

int svs_keyframe_decide_launch(svs_ctx *ctx, const svs_keyframe_decide_args *a, const svs_keyframe_decide_params *prm, const KfdFrontendSrc *fs,
                               svs_keyframe_decision *d_dec, svs_map_new_point *d_new, svs_map_track_point *d_track, int32_t *d_new_rec, int32_t *d_track_rec, int cap) {
  SVS_REQUIRE(ctx, ctx && a && prm && d_dec && d_new && d_track && d_new_rec && d_track_rec);
  SVS_REQUIRE(ctx, a->batch >= 0 && a->n >= 0 && a->max_keyframes >= 0 && prm->covis_thr >= 0);
  if (a->batch == 0) return SVS_OK;
  SVS_REQUIRE(ctx, a->d_stats && a->d_T_cur_from_actkey && (fs || a->d_tracking_ok) && a->d_table && a->d_vertex);
  SVS_REQUIRE(ctx, a->n == 0 || (a->d_res && a->d_pts && a->d_gated));
  SVS_REQUIRE(ctx, a->max_keyframes == 0 || (a->d_slot_kf && (a->batch == 1 || a->slot_bstride >= (size_t)a->max_keyframes)));
  SVS_REQUIRE(ctx, a->set_bstride == 0 || a->d_set_ids);
  SVS_REQUIRE(ctx, !a->map || svs_map_ctx(a->map) == ctx);
  if (cap < a->n) { ctx->err = "svs_keyframe_decide: cap below the record count n"; return SVS_ERR_CAPACITY; }
  if (a->vertex_bstride > SVS_KF_MAX_VERTICES) { ctx->err = "svs_keyframe_decide: more than SVS_KF_MAX_VERTICES vertices per stream"; return SVS_ERR_CAPACITY; }
  if (a->max_keyframes > SVS_KF_MAX_SLOTS) { ctx->err = "svs_keyframe_decide: more than SVS_KF_MAX_SLOTS keyframe slots"; return SVS_ERR_UNSUPPORTED; }
  SVS_DEVICE(ctx);
  KdK K{};
  K.a = *a; K.p = *prm;
  if (a->map) { if (int rc = svs_map_observer_view(a->map, &K.M)) return rc; }      // (else pt_hi = 0: a map-backed set is empty)
  if (fs) { K.fs = *fs; K.have_fs = 1; }
  K.dec = d_dec; K.nw = d_new; K.tr = d_track; K.nw_rec = d_new_rec; K.tr_rec = d_track_rec; K.cap = cap;
  hipLaunchKernelGGL(keyframe_decide_kernel, dim3(a->batch), dim3(KD_THREADS), 0, ctx->stream, K);
  SVS_LAUNCH_CHECK(ctx);
  return SVS_OK;
}

extern "C" int svs_keyframe_decide(svs_ctx *ctx, const svs_keyframe_decide_args *a, const svs_keyframe_decide_params *prm, svs_keyframe_decision *d_dec,
                                   svs_map_new_point *d_new, svs_map_track_point *d_track, int32_t *d_new_rec, int32_t *d_track_rec, int cap) {
  return svs_keyframe_decide_launch(ctx, a, prm, nullptr, d_dec, d_new, d_track, d_new_rec, d_track_rec, cap);
}

int svs_keyframe_scatter_tables(svs_ctx *ctx, int n_requests, const KfdScatter &s) {
  if (n_requests <= 0) return SVS_OK;
  hipLaunchKernelGGL(keyframe_scatter_kernel, dim3(n_requests), dim3(KD_THREADS), 0, ctx->stream, s);
  SVS_LAUNCH_CHECK(ctx);
  return SVS_OK;
}
