// frontend.hip -- one call per camera frame: the data-parallel part of StereoFrontend::processFrame
// (stereo_frontend.cpp:183-306), for ONE stream with host buffers in and out (the way stereo_slam's main loop calls it,
// stereo_slam.cpp:705) or for a BATCH of independent camera streams whose frames are already in device memory.  Chains the
// kernels of image.hip / dense.hip / motion.hip / dense_full.hip / stereo.hip / fast.hip / match.hip on the context's stream without a host
// round trip in between:
//   upload (pinned staging, optionally prefetched on a copy stream while the frame before is processed)
//   -> FrameGrabber::preprocessing (u8 pyramid; CUDA build: + f32 pyramid and derivatives)       frame_grabber.cpp:285-336
//   -> DenseTracker::denseTrackingCpu / denseTrackingGpu (device-resident LM)                    stereo_frontend.cpp:191-197
//   -> calcDisparityCpu (cv::StereoBM) unless a disparity image is given                         :199-225
//   -> computeFastCorners (FastGrid::detectAdaptively, 6 trials, use_n_levels_in_frontent levels) :228-233
//   -> matchAndTrack: GuidedMatcher::match on the active keyframe's new points, the neighbours' new points (while
//      2 * observations < ui.num_max_points), the neighbourhood's points; calcFastMotionOnly      :235-241, :976-1069
//   -> processMatchedPoints (reprojection gate + PointStatistics)                                :245-262, :834-974
//   -> computeDensePointCloudCpu / Gpu at the refined pose                                       :298-302
//   -> one download of {pose, pass count, match records, gate records, statistics}.
// Behind a step, svs_frontend_decide_keyframes (keyframe.hip) takes the keyframe switch / drop decision (:265-296) and builds the
// AddToOptimzer lists from the same device state; applying the decision stays with the caller.  The object owns the device copies of the previous frame (pyramid + reference cloud), the keyframes it was
// told to keep (Frame::clone, keyframes.h:72-83), the candidate points (ap_map) and the FAST threshold state -- per stream.
#include "common.h"
#include "fast_view.h"
#include "keyframe.h"
#include "nbh_map.h"
#include "nbr_map.h"
#include "addkf_map.h"
#include "newpoints.h"
#include "pose.h"
#include "seed.h"
#include "staging.h"
#include <string.h>
#include <algorithm>
#include <type_traits>
#include <vector>

namespace {
constexpr int MAX_GROUPS = 64;
static_assert(MAX_GROUPS == NBH_MAX_GROUPS, "the map's walk writes rows of d_group_end");

// T_cur_from_w = T_cur_from_actkey * T_actkey_from_w and T_w_from_actkey = T_actkey_from_w^-1 (matcher.cpp:326-330), formed on the
// device from the tracked pose so that the matcher needs no host round trip.  One workgroup per stream.
__global__ void frontend_pose_kernel(const double *__restrict__ T_cur_from_actkey, const double *__restrict__ T_actkey_from_w,
                                     double *__restrict__ T_cur_from_w, double *__restrict__ T_w_from_actkey) {
  if (threadIdx.x != 0) return;
  const size_t s = (size_t)blockIdx.x * 12;
  const double *A = T_cur_from_actkey + s, *Bm = T_actkey_from_w + s;
  double *Tcw = T_cur_from_w + s, *Twa = T_w_from_actkey + s;
  pose_inv(Bm, Twa);
  pose_mul(A, Bm, Tcw);
}

// matchAndTrack's neighbour cut (stereo_frontend.cpp:1000-1024): the new-point list of neighbour j is matched only while
// 2 * obs_list.size() < ui.num_max_points.  All groups were matched by one launch; this kernel counts the observations group by
// group (list order = record order) and marks the records of the neighbour lists the reference would not have visited.
// group_end[g] = one past the last record of group g; group 0 = the active keyframe's new points, groups 1 .. G-2 = the
// neighbours' new points in strength order, group G-1 = the neighbourhood's points.  One workgroup per stream.
__global__ __launch_bounds__(256) void frontend_group_cut_kernel(svs_match_result *__restrict__ res, size_t res_b, const int32_t *__restrict__ group_end,
                                                                 const int32_t *__restrict__ n_groups, int num_max_points) {
  __shared__ int s_end[MAX_GROUPS], s_cnt[MAX_GROUPS], s_cut[2];
  const int b = blockIdx.x, tid = threadIdx.x;
  const int G = n_groups[b];
  if (G <= 2) return;                          // no neighbour lists
  res += (size_t)b * res_b;
  if (tid < MAX_GROUPS) { s_end[tid] = tid < G ? group_end[(size_t)b * MAX_GROUPS + tid] : 0; s_cnt[tid] = 0; }
  __syncthreads();
  const int n_new = s_end[G - 2];
  for (int i = tid; i < n_new; i += 256) {
    if (res[i].status != SVS_MATCH_OK) continue;
    int g = 0;
    while (i >= s_end[g]) ++g;
    atomicAdd(&s_cnt[g], 1);
  }
  __syncthreads();
  if (tid == 0) {
    int obs = s_cnt[0], cut = G - 1;
    for (int j = 1; j <= G - 2; ++j) {
      if (!(2 * obs < num_max_points)) { cut = j; break; }
      obs += s_cnt[j];
    }
    s_cut[0] = cut == G - 1 ? n_new : s_end[cut - 1];
    s_cut[1] = n_new;
  }
  __syncthreads();
  for (int i = s_cut[0] + tid; i < s_cut[1]; i += 256) {
    svs_match_result r{};
    r.status = SVS_MATCH_SKIPPED;
    res[i] = r;
  }
}

// rows of `wbytes` bytes (a multiple of 4), dword copies; grid (x blocks, rows, batch)
__global__ __launch_bounds__(256) void copy_rows_kernel(const uint8_t *__restrict__ src, size_t sstride, size_t s_b, uint8_t *__restrict__ dst, size_t dstride,
                                                        size_t d_b, int wdwords) {
  const int x = blockIdx.x * 256 + threadIdx.x;
  if (x >= wdwords) return;
  const uint32_t *s = reinterpret_cast<const uint32_t *>(src + blockIdx.z * s_b + blockIdx.y * sstride);
  uint32_t *d = reinterpret_cast<uint32_t *>(dst + blockIdx.z * d_b + blockIdx.y * dstride);
  d[x] = s[x];
}
inline int round_up(int a, int b) { return (a + b - 1) / b * b; }
struct Views3 { float *p[3]; operator float *const *() const { return p; } };      // the three levels of an owner array as the pointer array the stage calls take
inline Views3 views(const DevBuf<float> (&b)[3]) { return {{b[0], b[1], b[2]}}; }
}  // namespace

struct svs_frontend {
  svs_ctx *ctx = nullptr;
  svs_frontend_params prm{};
  svs_cam cams[3]{};
  int w[3]{}, h[3]{}, stride[3]{};
  size_t lvl_elems[3]{};                // h * stride: elements between the level images of consecutive streams
  int B = 1, max_points = 0, max_keyframes = 0, n_launch = 0, max_groups_used = 2;
  std::vector<int> n_points, n_new_records;
  std::vector<uint8_t> kept;            // [B][max_keyframes]: slot filled by svs_frontend_keep_keyframe
  bool have_prev = false;
  // device: three pyramid slots per stream (previous / current / next: the next frame may be uploaded while the current one is
  // processed) with their right images / disparities, reference clouds
  DevBuf<uint8_t> d_pyr[3][3];
  int i_prev = 2, i_cur = 0, i_next = 1;
  DevBuf<uint8_t> d_right[3];          // right image / disparity of the frame in pyramid slot k
  DevBuf<float> d_disp[3];
  const float *last_disp = nullptr; int last_dstride = 0; size_t last_dbstride = 0;      // disparity the frame processed last was given / produced
  const uint8_t *ext_left = nullptr; int ext_lstride = 0; size_t ext_lbstride = 0;       // a caller's device frame waiting to be taken in by the first pyramid step
  DevBuf<float> d_cloud[3];             // quarter grid (CPU build) or full resolution (CUDA build), float4 per sample
  size_t cloud_elems[3]{};              // floats per stream and level
  // CUDA build (prm.cuda_build): f32 pyramids of the current / previous frame, derivative images of the current one
  DevBuf<float> d_f32[2][3], d_dx[3], d_dy[3];
  int i_f32 = 0;
  DevBuf<uint8_t> d_kf_pyr;             // [B][max_keyframes] x 3 levels, packed
  size_t kf_level_off[3] = {}, kf_bytes = 0;
  DevBuf<svs_keyframe> d_kfs;           // [B][max_keyframes]
  std::vector<svs_keyframe> h_kfs;
  DevBuf<svs_candidate_point> d_pts;    // [B][max_points]
  PinnedBuf<svs_candidate_point> h_cand_stage;      // pinned, [B][max_points]: svs_frontend_set_candidates_all's staging block (allocated on first use)
  // the frame's results: views, backed by d_out_block (one stream: d_small | d_res | d_gated carved from ONE allocation in h_out's layout -- the results go home
  // in one copy) or by the three blocks beside it (several streams)
  svs_match_result *d_res = nullptr;
  svs_gated_point *d_gated = nullptr;
  DevBuf<uint8_t> d_out_block; DevBuf<svs_match_result> res_block; DevBuf<svs_gated_point> gated_block; DevBuf<double> small_block;
  DevBuf<int32_t> d_group_end, d_n_groups, d_n_new;      // [B][MAX_GROUPS], [B], [B]: records of the new-feature lists
  // small device block: T [B][12] | T_actkey_from_w [B][12] | T_cur_from_w [B][12] | T_w_from_actkey [B][12] | pose stats [B] | point stats [B] | passes [B]
  double *d_small = nullptr;
  size_t small_bytes = 0;
  svs_pose_opt_stats *d_pstats = nullptr;
  svs_point_stats *d_ptstats = nullptr;
  int32_t *d_passes = nullptr;
  svs_fast *fast = nullptr;
  // cross-frame pipeline (ctx option "fe_pipeline"): the pyramid of frame N+1 is built on the side stream while frame N's pose refinement / gate / cloud run
  owned::Event ev_early[2], ev_late[2];              // by frame parity: pyramid done (side stream) / the whole frame done (context's stream)
  owned::Event ev_trk[2];                            // ... / the point of the context's stream right in front of the pose refinement's launch
  unsigned pipe_run = 0;                             // frames issued through the pipelined path since the last frame that was not
  svs_stereo *stereo = nullptr;
  // pinned host staging: two input sets (images of stream 0, poses of all streams), one output set
  PinnedBuf<uint8_t> h_in[2]; size_t h_in_bytes = 0; int i_stage = 0;
  PinnedBuf<uint8_t> h_out; size_t h_out_bytes = 0;
  owned::Stream copy_stream;
  owned::Event ev_upload[2], ev_done[2];
  // FAST (and block matching) need the new pyramid only, the dense tracker runs ~18 dependent sweeps per stream with a long tail (streams finish at
  // different times): the detector stages are enqueued on a second stream and meet the chain again in front of the matcher
  owned::Stream side_stream;
  owned::Event ev_fork, ev_join;
  bool prefetched = false, submitted = false, want_matches = false, want_gated = false;
  int n_submitted = 0;
  // accept / reject record of the dense tracker's LM loop, per stream (svs_frontend_dense_records)
  DevBuf<svs_dense_lm_record> d_rec; DevBuf<int32_t> d_nrec;
  DevBuf<void> d_trk_work;              // state of the tracker's balanced launch (dense.hip: LM work of every stream's last frame -> grid order); big batches only
  // optional stage timing (svs_frontend_set_timing): events between the stages of the last call
  bool timing = false;
  owned::Event ev_stage[SVS_FRONTEND_STAGES + 1];
  // new-point seeding (svs_frontend_seed_keyframes): records the last step's gate wrote per stream; -1 while they do not describe the candidate list (no step
  // since the last first frame, or the list was replaced behind the step), staging blocks grown on demand
  int n_gated = -1;
  PinnedBuf<uint8_t> h_seed; DevBuf<uint8_t> d_seed;
  // optional sub-pixel refinement of the matches (svs_frontend_set_subpixel; match.hip: match_subpix.inc): one launch behind the matcher while `subpix` is set.
  // d_subpix_info [B][max_points] is allocated when the option is first switched on; subpix_n = records per stream the last step's pass covered, -1: none
  bool subpix = false;
  svs_subpix_params subpix_prm{};
  DevBuf<svs_subpix_info> d_subpix_info;
  int subpix_n = -1;
  // svs_frontend_set_candidates_from_map: the staged requests and, behind them, what comes back; grown on demand
  TwinBlock nbh;
  // the keyframe decision (svs_frontend_set_vertex_table / svs_frontend_decide_keyframes, keyframe.hip): the streams' resident vertex tables, the staging block
  // of the setter, the decision records and list rows; all allocated with the first table
  std::vector<uint8_t> vt_set;          // [B]: the stream has a table
  DevBuf<svs_kf_table> d_vt_tab; DevBuf<svs_kf_vertex> d_vt_vtx; DevBuf<int32_t> d_vt_slot, d_vt_ids;
  TwinBlock vt_up;
  DevBuf<svs_keyframe_decision> d_kd_dec; DevBuf<svs_map_new_point> d_kd_new; DevBuf<svs_map_track_point> d_kd_track; DevBuf<int32_t> d_kd_new_rec, d_kd_track_rec;
  PinnedBuf<svs_keyframe_decision> h_kd_dec;
  // svs_frontend_commit_keyframe: the steps counted, the count the records in h_kd_dec were decided at (kd_have: there are any), and the pinned block the pose and
  // the thresholds of the committed stream come home in
  // pose_replaced: svs_frontend_recompute_cloud has overwritten the step's refined poses since the step (they are what a commit would insert)
  uint64_t step_serial = 0, kd_serial = 0; bool kd_have = false, pose_replaced = false;
  PinnedBuf<uint8_t> h_ck;
  // the resident newpoint_map (svs_frontend_newpoints_*, frontend_newpoints.inc / newpoints.hip): per stream a row of records with its groups packed in store order,
  // a scratch row, the (key, count) table; the host mirrors the TABLES (never a record) and decides every refusal from them.  Nothing is allocated before
  // svs_frontend_newpoints_reserve
  int np_rcap = 0, np_gcap = 0;
  DevBuf<svs_candidate_point> d_np_rec, d_np_tmp; DevBuf<int32_t> d_np_key, d_np_cnt, d_np_ng, d_np_removed;
  std::vector<int32_t> np_key, np_cnt, np_ng;      // [B][64], [B][64], [B]
  TwinBlock np;                                    // staging block of the calls, grown on demand
  // drains the streams and takes the detector / block matcher along before the members above go (also when create gives up half way)
  ~svs_frontend() {
    (void)hipStreamSynchronize(ctx->stream);
    if (copy_stream) (void)hipStreamSynchronize(copy_stream);
    if (side_stream) (void)hipStreamSynchronize(side_stream);
    if (fast) svs_fast_destroy(fast);
    if (stereo) svs_stereo_destroy(stereo);
  }
};
constexpr int REC_CAP = 64;

namespace {
// ---- what the list setters share: their checks (every one of a call runs before its first upload) and the tail in which the host state follows the download
bool all_distinct(std::vector<int32_t> &v) {      // (sorts v)
  std::sort(v.begin(), v.end());
  return std::adjacent_find(v.begin(), v.end()) == v.end();
}
// every slot a slot table names is one svs_frontend_keep_keyframe has filled, and no keyframe id is named twice
int fe_check_slot_table(svs_frontend *fe, int stream, const int32_t *h_slot_kf, std::vector<int32_t> &ids) {
  svs_ctx *ctx = fe->ctx;
  const uint8_t *kept = fe->kept.data() + (size_t)stream * fe->max_keyframes;
  ids.clear();
  for (int s = 0; s < fe->max_keyframes; ++s)
    if (h_slot_kf[s] >= 0) { SVS_REQUIRE(ctx, kept[s]); ids.push_back(h_slot_kf[s]); }
  SVS_REQUIRE(ctx, all_distinct(ids));
  return SVS_OK;
}
// group ends rise and the last equals n
int fe_check_group_ends(svs_ctx *ctx, const int32_t *h_group_end, int n_groups, int n) {
  SVS_REQUIRE(ctx, h_group_end[n_groups - 1] == n);
  for (int g = 0; g < n_groups; ++g) SVS_REQUIRE(ctx, h_group_end[g] >= (g ? h_group_end[g - 1] : 0));
  return SVS_OK;
}
// a record must name a keyframe slot that svs_frontend_keep_keyframe has filled (kf_index < 0 = "anchor not in the map", matcher.cpp:336-339)
int fe_check_anchors(svs_frontend *fe, int stream, const svs_candidate_point *h_pts, int n) {
  svs_ctx *ctx = fe->ctx;
  const uint8_t *kept = fe->kept.data() + (size_t)stream * fe->max_keyframes;
  for (int i = 0; i < n; ++i) SVS_REQUIRE(ctx, h_pts[i].kf_index < 0 || (h_pts[i].kf_index < fe->max_keyframes && kept[h_pts[i].kf_index]));
  return SVS_OK;
}
// a stream's list on the device was replaced
void fe_lists_changed(svs_frontend *fe) {
  fe->n_launch = *std::max_element(fe->n_points.begin(), fe->n_points.end());
  fe->n_gated = -1;      // the last step's gate records no longer belong to the list on the device
}
// row r (`per` elements) of a downloaded piece to the caller's optional array; for a request that wrote none: ids -1, poses 0
template <class T> void fe_row_out(T *dst, const T *src, int r, size_t per, bool none) {
  if (!dst) return;
  if (none) memset(dst + (size_t)r * per, std::is_integral<T>::value ? 0xff : 0, per * sizeof(T));
  else memcpy(dst + (size_t)r * per, src + (size_t)r * per, per * sizeof(T));
}
// the mirror of the kept keyframes takes the poses a neighbourhood call refreshed on the device: slot_T [max_keyframes][12] of the request
void fe_refresh_poses(svs_frontend *fe, const svs_map *map, int stream, const int32_t *h_slot_kf, const double *slot_T) {
  for (int k = 0; k < fe->max_keyframes; ++k)
    if (svs_map_has_keyframe(map, h_slot_kf[k])) memcpy(fe->h_kfs[(size_t)stream * fe->max_keyframes + k].T_anchor_from_w, slot_T + (size_t)k * 12, 12 * sizeof(double));
}
}  // namespace

extern "C" int svs_frontend_destroy(svs_frontend *fe) {
  if (!fe) return SVS_OK;
  delete fe;
  return SVS_OK;
}

extern "C" int svs_frontend_create_batch(svs_ctx *ctx, const svs_cam *cam, const svs_frontend_params *prm, int max_points, int max_keyframes,
                                         int n_streams, svs_frontend **out) {
  SVS_REQUIRE(ctx, ctx && cam && prm && out && max_points >= 1 && max_keyframes >= 1 && n_streams >= 1);
  SVS_REQUIRE(ctx, cam->w % 16 == 0 && cam->h % 16 == 0);              // quarter grid on three levels (dense_tracking.cpp:45-46)
  SVS_REQUIRE(ctx, prm->n_levels >= 0 && prm->n_levels <= 3 && prm->num_max_points >= 0 && prm->min_matches >= 0);
  SVS_DEVICE(ctx);
  std::unique_ptr<svs_frontend> fe(new svs_frontend());
  fe->ctx = ctx; fe->prm = *prm; fe->max_points = max_points; fe->max_keyframes = max_keyframes; fe->B = n_streams;
  if (fe->prm.n_levels == 0) fe->prm.n_levels = 3;
  if (fe->prm.num_max_points == 0) fe->prm.num_max_points = 300;      // ui.num_max_points (stereo_frontend.cpp:1000)
  if (fe->prm.min_matches == 0) fe->prm.min_matches = 20;             // :1053
  const size_t B = (size_t)n_streams;
  fe->n_points.assign(B, 0); fe->n_new_records.assign(B, 0);
  fe->kept.assign(B * max_keyframes, 0);
  size_t off = 0;
  for (int l = 0; l < 3; ++l) {
    const double s = (double)(1 << l);
    fe->cams[l] = svs_cam{cam->f / s, cam->cx / s, cam->cy / s, cam->b * (1 << l), (int)(cam->w / s), (int)(cam->h / s)};      // frame_grabber-impl.cpp:48-60
    fe->w[l] = fe->cams[l].w; fe->h[l] = fe->cams[l].h; fe->stride[l] = round_up(fe->w[l], 64);
    fe->lvl_elems[l] = (size_t)fe->h[l] * fe->stride[l];
    fe->kf_level_off[l] = off;
    off += fe->lvl_elems[l];
  }
  fe->kf_bytes = off;
  for (int k = 0; k < 3; ++k)
    for (int l = 0; l < 3; ++l) SVS_HIP(ctx, fe->d_pyr[k][l].alloc(fe->lvl_elems[l] * B));
  const size_t px0 = fe->lvl_elems[0];
  for (int k = 0; k < 3; ++k) {
    if (prm->use_block_matching) SVS_HIP(ctx, fe->d_right[k].alloc(px0 * B));
    SVS_HIP(ctx, fe->d_disp[k].alloc(px0 * B));
  }
  for (int l = 0; l < 3; ++l) {
    fe->cloud_elems[l] = prm->cuda_build ? 4 * (size_t)fe->w[l] * fe->h[l] : 4 * (size_t)(fe->w[l] / 4) * (fe->h[l] / 4);
    SVS_HIP(ctx, fe->d_cloud[l].alloc(fe->cloud_elems[l] * B));
    if (prm->cuda_build)
      for (DevBuf<float> *b : {&fe->d_f32[0][l], &fe->d_f32[1][l], &fe->d_dx[l], &fe->d_dy[l]}) SVS_HIP(ctx, b->alloc(fe->lvl_elems[l] * B));
  }
  // per-stream scalars (poses in and out, statistics): a multiple of 256 bytes, so that the record arrays may follow it in one allocation
  fe->small_bytes = ((sizeof(double) * 48 + sizeof(svs_pose_opt_stats) + sizeof(svs_point_stats) + 8) * B + 255) & ~(size_t)255;
  if (B == 1) {      // latency mode: d_small | d_res | d_gated in the layout of the pinned result buffer -- ONE device-to-host copy per frame instead of three (12 us apart each)
    SVS_HIP(ctx, fe->d_out_block.alloc(fe->small_bytes + (sizeof(svs_match_result) + sizeof(svs_gated_point)) * (size_t)max_points));
    fe->d_small = reinterpret_cast<double *>(fe->d_out_block.get());
    fe->d_res = reinterpret_cast<svs_match_result *>(fe->d_out_block + fe->small_bytes);
    fe->d_gated = reinterpret_cast<svs_gated_point *>(fe->d_out_block + fe->small_bytes + sizeof(svs_match_result) * (size_t)max_points);
  } else {
    SVS_HIP(ctx, fe->res_block.alloc(max_points * B, &fe->d_res));
    SVS_HIP(ctx, fe->gated_block.alloc(max_points * B, &fe->d_gated));
    SVS_HIP(ctx, fe->small_block.alloc_bytes(fe->small_bytes, &fe->d_small));
  }
  SVS_HIP(ctx, fe->d_kf_pyr.alloc(fe->kf_bytes * max_keyframes * B));
  SVS_HIP(ctx, fe->d_kfs.alloc(max_keyframes * B));
  SVS_HIP(ctx, fe->d_pts.alloc(max_points * B));
  SVS_HIP(ctx, fe->d_group_end.alloc(MAX_GROUPS * B));
  SVS_HIP(ctx, fe->d_n_groups.alloc(B));
  SVS_HIP(ctx, fe->d_n_new.alloc(B));
  // unused keyframe slots hold null pyramids, unused candidate records kf_index = -1 (-> SVS_MATCH_NO_ANCHOR): nothing a kernel could follow
  SVS_HIP(ctx, hipMemsetAsync(fe->d_kfs, 0, sizeof(svs_keyframe) * max_keyframes * B, ctx->stream));
  SVS_HIP(ctx, hipMemsetAsync(fe->d_pts, 0xff, sizeof(svs_candidate_point) * max_points * B, ctx->stream));
  SVS_HIP(ctx, hipMemsetAsync(fe->d_n_groups, 0, sizeof(int32_t) * B, ctx->stream));
  SVS_HIP(ctx, hipMemsetAsync(fe->d_n_new, 0, sizeof(int32_t) * B, ctx->stream));
  SVS_HIP(ctx, hipMemsetAsync(fe->d_small, 0, fe->small_bytes, ctx->stream));
  fe->d_pstats = reinterpret_cast<svs_pose_opt_stats *>(fe->d_small + 48 * B);
  fe->d_ptstats = reinterpret_cast<svs_point_stats *>(fe->d_pstats + B);
  fe->d_passes = reinterpret_cast<int32_t *>(fe->d_ptstats + B);
  fe->h_kfs.assign(max_keyframes * B, svs_keyframe{});
  svs_fastgrid grids[3];
  for (int l = 0; l < 3; ++l) fastgrid_for_level(fe->w[l], fe->h[l], l, &grids[l]);
  if (int rc = svs_fast_create(ctx, fe->prm.n_levels, fe->w, fe->h, grids, n_streams, 8192, &fe->fast)) return rc;
  if (ctx->fe_pipeline && n_streams > 1 && n_streams <= 2 * ctx->n_cu && !prm->use_block_matching && !prm->cuda_build) {
    for (int k = 0; k < 2; ++k)
      for (owned::Event *e : {&fe->ev_early[k], &fe->ev_late[k], &fe->ev_trk[k]}) SVS_HIP(ctx, e->create(hipEventDisableTiming));
  }
  if (prm->use_block_matching) if (int rc = svs_stereo_create(ctx, fe->w[0], fe->h[0], n_streams, &prm->stereo, &fe->stereo)) return rc;
  fe->h_in_bytes = 2 * (size_t)fe->w[0] * fe->h[0] + sizeof(float) * (size_t)fe->w[0] * fe->h[0] + sizeof(double) * 24 * B;
  fe->h_out_bytes = fe->small_bytes + (sizeof(svs_match_result) + sizeof(svs_gated_point)) * (size_t)max_points;
  for (int k = 0; k < 2; ++k) {
    SVS_HIP(ctx, fe->h_in[k].alloc(fe->h_in_bytes));
    SVS_HIP(ctx, fe->ev_upload[k].create(hipEventDisableTiming));
    SVS_HIP(ctx, fe->ev_done[k].create(hipEventDisableTiming));
  }
  SVS_HIP(ctx, fe->h_out.alloc(fe->h_out_bytes));
  SVS_HIP(ctx, fe->copy_stream.create(hipStreamNonBlocking));
  {
    int least = 0, greatest = 0;      // the chain's own stream keeps the first claim on the CUs
    if (hipDeviceGetStreamPriorityRange(&least, &greatest) != hipSuccess) least = 0;
    SVS_HIP(ctx, fe->side_stream.create(hipStreamNonBlocking, least));
    SVS_HIP(ctx, fe->ev_fork.create(hipEventDisableTiming));
    SVS_HIP(ctx, fe->ev_join.create(hipEventDisableTiming));
  }
  SVS_HIP(ctx, fe->d_rec.alloc(REC_CAP * B));
  SVS_HIP(ctx, fe->d_nrec.alloc(B));
  SVS_HIP(ctx, hipMemsetAsync(fe->d_nrec, 0, sizeof(int32_t) * B, ctx->stream));
  if (B >= 2 * ctx->n_cu && B <= 4096) {
    SVS_HIP(ctx, fe->d_trk_work.alloc_bytes(svs_dense_track_balance_bytes(B)));
    if (int rc = svs_dense_track_balance_init(ctx, fe->d_trk_work, B)) return rc;
  }
  SVS_HIP(ctx, hipStreamSynchronize(ctx->stream));
  *out = fe.release();
  return SVS_OK;
}

extern "C" int svs_frontend_create(svs_ctx *ctx, const svs_cam *cam, const svs_frontend_params *prm, int max_points, int max_keyframes,
                                   svs_frontend **out) {
  return svs_frontend_create_batch(ctx, cam, prm, max_points, max_keyframes, 1, out);
}

extern "C" int svs_frontend_set_candidates_grouped(svs_frontend *fe, int stream, const svs_candidate_point *h_pts, int n, const int32_t *h_group_end, int n_groups) {
  svs_ctx *ctx = fe ? fe->ctx : nullptr;
  SVS_REQUIRE(ctx, fe && stream >= 0 && stream < fe->B && n >= 0 && n <= fe->max_points && (n == 0 || h_pts));
  SVS_REQUIRE(ctx, !fe->submitted);      // between submit_frame and wait_frame the list of the frame in flight is latched (wait_frame sizes its copies by it)
  SVS_REQUIRE(ctx, h_group_end && n_groups >= 2 && n_groups <= MAX_GROUPS);
  if (int rc = fe_check_group_ends(ctx, h_group_end, n_groups, n)) return rc;
  SVS_DEVICE(ctx);
  if (int rc = fe_check_anchors(fe, stream, h_pts, n)) return rc;
  SVS_HIP(ctx, hipStreamSynchronize(ctx->stream));
  svs_candidate_point *dst = fe->d_pts + (size_t)stream * fe->max_points;
  if (n) SVS_HIP(ctx, hipMemcpyAsync(dst, h_pts, sizeof(svs_candidate_point) * (size_t)n, hipMemcpyHostToDevice, ctx->stream));
  if (fe->n_points[stream] > n) SVS_HIP(ctx, hipMemsetAsync(dst + n, 0xff, sizeof(svs_candidate_point) * (size_t)(fe->n_points[stream] - n), ctx->stream));
  int32_t ge[MAX_GROUPS] = {};
  for (int g = 0; g < n_groups; ++g) ge[g] = h_group_end[g];
  SVS_HIP(ctx, hipMemcpyAsync(fe->d_group_end + (size_t)stream * MAX_GROUPS, ge, sizeof ge, hipMemcpyHostToDevice, ctx->stream));
  SVS_HIP(ctx, hipMemcpyAsync(fe->d_n_groups + stream, &n_groups, sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
  SVS_HIP(ctx, hipMemcpyAsync(fe->d_n_new + stream, &h_group_end[n_groups - 2], sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
  SVS_HIP(ctx, hipStreamSynchronize(ctx->stream));      // h_pts may be pageable and reused by the caller
  fe->n_points[stream] = n; fe->n_new_records[stream] = h_group_end[n_groups - 2];
  fe_lists_changed(fe);
  fe->max_groups_used = std::max(fe->max_groups_used, n_groups);
  return SVS_OK;
}

extern "C" int svs_frontend_set_candidates(svs_frontend *fe, const svs_candidate_point *h_pts, int n, int n_new_records) {
  svs_ctx *ctx = fe ? fe->ctx : nullptr;
  SVS_REQUIRE(ctx, fe && n >= 0 && n_new_records >= 0 && n_new_records <= n);
  const int32_t ge[2] = {n_new_records, n};
  return svs_frontend_set_candidates_grouped(fe, 0, h_pts, n, ge, 2);
}

extern "C" int svs_frontend_keep_keyframe_of(svs_frontend *fe, int stream, int slot, const double *T_kf_from_w) {
  svs_ctx *ctx = fe ? fe->ctx : nullptr;
  SVS_REQUIRE(ctx, fe && T_kf_from_w && stream >= 0 && stream < fe->B && slot >= 0 && slot < fe->max_keyframes && fe->have_prev && !fe->submitted);
  SVS_DEVICE(ctx);
  // Frame::clone of the frame processed last (it sits in the "previous" slot after the rotation at the end of process_frame)
  const size_t idx = (size_t)stream * fe->max_keyframes + slot;
  uint8_t *base = fe->d_kf_pyr + fe->kf_bytes * idx;
  svs_keyframe &k = fe->h_kfs[idx];
  for (int l = 0; l < 3; ++l) {
    SVS_HIP(ctx, hipMemcpyAsync(base + fe->kf_level_off[l], fe->d_pyr[fe->i_prev][l] + fe->lvl_elems[l] * stream, fe->lvl_elems[l], hipMemcpyDeviceToDevice, ctx->stream));
    k.pyr[l] = base + fe->kf_level_off[l]; k.stride[l] = fe->stride[l];
  }
  for (int i = 0; i < 12; ++i) k.T_anchor_from_w[i] = T_kf_from_w[i];
  SVS_HIP(ctx, hipMemcpyAsync(fe->d_kfs + idx, &k, sizeof k, hipMemcpyHostToDevice, ctx->stream));
  SVS_HIP(ctx, hipStreamSynchronize(ctx->stream));
  fe->kept[idx] = 1;
  return SVS_OK;
}
extern "C" int svs_frontend_keep_keyframe(svs_frontend *fe, int slot, const double *T_kf_from_w) { return svs_frontend_keep_keyframe_of(fe, 0, slot, T_kf_from_w); }

/* the same for ALL streams in one go: the frame each stream processed last becomes its keyframe `slot`; h_T_kf_from_w [n_streams][12].  One strided copy per pyramid
   level and one table upload instead of 4 small copies and a synchronisation per stream. */
extern "C" int svs_frontend_keep_keyframes(svs_frontend *fe, int slot, const double *h_T_kf_from_w) {
  svs_ctx *ctx = fe ? fe->ctx : nullptr;
  SVS_REQUIRE(ctx, fe && h_T_kf_from_w && slot >= 0 && slot < fe->max_keyframes && fe->have_prev && !fe->submitted);
  SVS_DEVICE(ctx);
  const size_t B = (size_t)fe->B, slot_pitch = fe->kf_bytes * (size_t)fe->max_keyframes;      // distance between the same slot of two consecutive streams
  for (int l = 0; l < 3; ++l)
    SVS_HIP(ctx, hipMemcpy2DAsync(fe->d_kf_pyr + fe->kf_bytes * (size_t)slot + fe->kf_level_off[l], slot_pitch, fe->d_pyr[fe->i_prev][l], fe->lvl_elems[l], fe->lvl_elems[l], B,
                                  hipMemcpyDeviceToDevice, ctx->stream));
  for (size_t b = 0; b < B; ++b) {
    const size_t idx = b * fe->max_keyframes + slot;
    svs_keyframe &k = fe->h_kfs[idx];
    uint8_t *base = fe->d_kf_pyr + fe->kf_bytes * idx;
    for (int l = 0; l < 3; ++l) { k.pyr[l] = base + fe->kf_level_off[l]; k.stride[l] = fe->stride[l]; }
    for (int i = 0; i < 12; ++i) k.T_anchor_from_w[i] = h_T_kf_from_w[12 * b + i];
  }
  SVS_HIP(ctx, hipMemcpyAsync(fe->d_kfs, fe->h_kfs.data(), sizeof(svs_keyframe) * fe->h_kfs.size(), hipMemcpyHostToDevice, ctx->stream));      // (the whole table: h_kfs mirrors it)
  SVS_HIP(ctx, hipStreamSynchronize(ctx->stream));
  for (size_t b = 0; b < B; ++b) fe->kept[b * fe->max_keyframes + slot] = 1;
  return SVS_OK;
}

/* svs_frontend_set_candidates_grouped for ALL streams in one go: h_pts = the streams' records back to back (stream b: h_n[b] records), h_group_end
   [n_streams][n_groups] (every stream with the same number of groups; an absent neighbour list is an empty group).  Staged through one host buffer: three
   uploads per call instead of four per stream. */
extern "C" int svs_frontend_set_candidates_all(svs_frontend *fe, const svs_candidate_point *h_pts, const int32_t *h_n, const int32_t *h_group_end, int n_groups) {
  svs_ctx *ctx = fe ? fe->ctx : nullptr;
  SVS_REQUIRE(ctx, fe && h_n && h_group_end && n_groups >= 2 && n_groups <= MAX_GROUPS && !fe->submitted);
  SVS_DEVICE(ctx);
  const int B = fe->B;
  size_t total = 0;
  for (int b = 0; b < B; ++b) {
    SVS_REQUIRE(ctx, h_n[b] >= 0 && h_n[b] <= fe->max_points);
    if (int rc = fe_check_group_ends(ctx, h_group_end + (size_t)b * n_groups, n_groups, h_n[b])) return rc;
    total += (size_t)h_n[b];
  }
  SVS_REQUIRE(ctx, total == 0 || h_pts);
  {
    size_t off = 0;
    for (int b = 0; b < B; off += (size_t)h_n[b], ++b)
      if (int rc = fe_check_anchors(fe, b, h_pts + off, h_n[b])) return rc;
  }
  // the device list is [n_streams][max_points]: lay the records out like that in a pinned block the front end keeps (unused tails = 0xff, "no candidate") and send
  // the first m records of every stream as one strided copy, m = the longest list now or before (what lies behind a stream's list on the device is 0xff: svs_frontend_create, the per-stream setters)
  if (!fe->h_cand_stage) SVS_HIP(ctx, fe->h_cand_stage.alloc((size_t)fe->B * fe->max_points));
  int m = 0;
  for (int b = 0; b < B; ++b) m = std::max(m, std::max(h_n[b], fe->n_points[b]));
  std::vector<int32_t> ge((size_t)B * MAX_GROUPS, 0), ng((size_t)B, n_groups), nn((size_t)B);
  size_t off = 0;
  SVS_HIP(ctx, hipStreamSynchronize(ctx->stream));      // (the staging block of the previous call has been read)
  for (int b = 0; b < B; ++b) {
    svs_candidate_point *row = fe->h_cand_stage + (size_t)b * fe->max_points;
    if (h_n[b]) __builtin_memcpy(row, h_pts + off, sizeof(svs_candidate_point) * (size_t)h_n[b]);
    if (m > h_n[b]) __builtin_memset(row + h_n[b], 0xff, sizeof(svs_candidate_point) * (size_t)(m - h_n[b]));
    off += (size_t)h_n[b];
    for (int g = 0; g < n_groups; ++g) ge[(size_t)b * MAX_GROUPS + g] = h_group_end[(size_t)b * n_groups + g];
    nn[b] = h_group_end[(size_t)b * n_groups + n_groups - 2];
  }
  if (m > 0)
    SVS_HIP(ctx, hipMemcpy2DAsync(fe->d_pts, sizeof(svs_candidate_point) * (size_t)fe->max_points, fe->h_cand_stage, sizeof(svs_candidate_point) * (size_t)fe->max_points,
                                  sizeof(svs_candidate_point) * (size_t)m, (size_t)B, hipMemcpyHostToDevice, ctx->stream));
  SVS_HIP(ctx, hipMemcpyAsync(fe->d_group_end, ge.data(), sizeof(int32_t) * ge.size(), hipMemcpyHostToDevice, ctx->stream));
  SVS_HIP(ctx, hipMemcpyAsync(fe->d_n_groups, ng.data(), sizeof(int32_t) * B, hipMemcpyHostToDevice, ctx->stream));
  SVS_HIP(ctx, hipMemcpyAsync(fe->d_n_new, nn.data(), sizeof(int32_t) * B, hipMemcpyHostToDevice, ctx->stream));
  SVS_HIP(ctx, hipStreamSynchronize(ctx->stream));
  for (int b = 0; b < B; ++b) { fe->n_points[b] = h_n[b]; fe->n_new_records[b] = nn[b]; }
  fe_lists_changed(fe);
  fe->max_groups_used = std::max(fe->max_groups_used, n_groups);
  return SVS_OK;
}

/* a stream's neighbourhood list from the device-resident map (map.hip: map_nbh.inc, through nbh_map.h; the contract is in the header): everything is checked on the host first,
   then one staged upload, the map's walk writing d_pts / d_group_end / d_n_groups / d_n_new / d_kfs in place, one download from which the host state follows */
extern "C" int svs_frontend_set_candidates_from_map(svs_frontend *fe, svs_map *map, int n_requests, const svs_nbh_request *req, int refresh_poses, int vertex_cap,
                                                    svs_nbh_result *h_res, int32_t *h_point_id, int32_t *h_vertex_id, double *h_vertex_T,
                                                    svs_candidate_point *h_records) {
  svs_ctx *ctx = fe ? fe->ctx : nullptr;
  SVS_REQUIRE(ctx, fe && map && svs_map_ctx(map) == ctx && !fe->submitted && n_requests >= 0 && n_requests <= fe->B && (n_requests == 0 || req) && vertex_cap >= 1);
  if (fe->max_keyframes > 32767) { ctx->err = "svs_frontend_set_candidates_from_map: at most 32767 keyframe slots"; return SVS_ERR_UNSUPPORTED; }
  const int R = n_requests, B = fe->B, K = fe->max_keyframes, MP = fe->max_points, VB = vertex_cap;
  size_t n_ids = 0, n_head = 0;
  {
    std::vector<uint8_t> named((size_t)B, 0);
    std::vector<int32_t> sorted;
    for (int r = 0; r < R; ++r) {
      const svs_nbh_request &q = req[r];
      SVS_REQUIRE(ctx, q.stream >= 0 && q.stream < B && !named[q.stream]);
      named[q.stream] = 1;
      SVS_REQUIRE(ctx, q.n_vertex >= 1 && q.h_vertex_kf && q.h_slot_kf && q.n_head >= 0 && q.n_head <= MP && (q.n_head == 0 || q.h_head) && q.n_head_groups >= 1 &&
                           q.h_head_group_end);
      if (q.n_head_groups + 1 > MAX_GROUPS) { ctx->err = "svs_frontend_set_candidates_from_map: more than 64 groups"; return SVS_ERR_CAPACITY; }
      for (int i = 0; i < q.n_vertex; ++i) SVS_REQUIRE(ctx, svs_map_has_keyframe(map, q.h_vertex_kf[i]));
      sorted.assign(q.h_vertex_kf, q.h_vertex_kf + q.n_vertex);
      SVS_REQUIRE(ctx, all_distinct(sorted));
      if (int rc = fe_check_slot_table(fe, q.stream, q.h_slot_kf, sorted)) return rc;
      if (int rc = fe_check_group_ends(ctx, q.h_head_group_end, q.n_head_groups, q.n_head)) return rc;
      if (int rc = fe_check_anchors(fe, q.stream, q.h_head, q.n_head)) return rc;
      n_ids += (size_t)q.n_vertex + (size_t)K;
      n_head += (size_t)q.n_head;
    }
  }
  if (R == 0) return SVS_OK;
  SVS_DEVICE(ctx);
  // the block: what goes up (requests | vertex and slot ids | heads), then what comes back, the optional outputs last
  Pieces<> row;
  const size_t Rz = (size_t)R;
  const auto p_req = row.piece<nbh_req>(Rz); const auto p_ids = row.piece<int32_t>(n_ids); const auto p_head = row.piece<svs_candidate_point>(n_head);
  const size_t in_end = row.end;
  const auto p_res = row.piece<svs_nbh_result>(Rz); const auto p_slot = row.piece<double>(Rz * K * 12);
  const auto p_vid = row.piece<int32_t>(Rz * VB); const auto p_vT = row.piece<double>(Rz * VB * 12); const auto p_pid = row.piece<int32_t>(Rz * MP);
  TwinBlock &blk = fe->nbh;
  if (int rc = blk.reserve(ctx, row.end)) return rc;      // (no call is in flight: this one is blocking)
  nbh_req *hq = blk.host(p_req);
  int32_t *ids = blk.host(p_ids);
  svs_candidate_point *head = blk.host(p_head);
  size_t at_id = 0, at_head = 0;
  for (int r = 0; r < R; ++r) {
    const svs_nbh_request &q = req[r];
    nbh_req &s = hq[r];
    memset(&s, 0, sizeof s);
    s.stream = q.stream; s.n_vertex = q.n_vertex; s.n_head = q.n_head; s.n_groups = q.n_head_groups + 1; s.prev_len = fe->n_points[q.stream];
    s.vertex_off = (int32_t)at_id;
    memcpy(ids + at_id, q.h_vertex_kf, (size_t)q.n_vertex * sizeof(int32_t));
    at_id += (size_t)q.n_vertex;
    s.slot_off = (int32_t)at_id;
    for (int k = 0; k < K; ++k) ids[at_id + k] = svs_map_has_keyframe(map, q.h_slot_kf[k]) ? q.h_slot_kf[k] : -1;
    at_id += (size_t)K;
    s.head_off = (int32_t)at_head;
    if (q.n_head) memcpy(head + at_head, q.h_head, (size_t)q.n_head * sizeof(svs_candidate_point));
    at_head += (size_t)q.n_head;
    for (int g = 0; g < q.n_head_groups; ++g) s.group_end[g] = q.h_head_group_end[g];
  }
  if (int rc = blk.upload(ctx, 0, in_end)) return rc;
  MapNbhDst D{};
  D.req = blk.dev(p_req); D.ids = blk.dev(p_ids); D.head = blk.dev(p_head);
  D.pts = fe->d_pts; D.max_points = MP; D.group_end = fe->d_group_end; D.n_groups = fe->d_n_groups; D.n_new = fe->d_n_new; D.kfs = fe->d_kfs; D.max_keyframes = K;
  D.refresh = refresh_poses ? 1 : 0;
  D.res = blk.dev(p_res); D.slot_T = blk.dev(p_slot); D.vertex_id = blk.dev(p_vid); D.vertex_T = blk.dev(p_vT); D.VB = VB; D.point_id = blk.dev(p_pid);
  if (int rc = svs_map_build_neighborhoods(map, R, D)) return rc;
  // from the first output piece to the end of the last one a caller asked for
  const size_t down_end = h_point_id ? p_pid.end() : (h_vertex_id || h_vertex_T) ? p_vT.end() : p_slot.end();
  if (int rc = blk.download(ctx, p_res.off, down_end)) return rc;
  if (h_records) SVS_HIP(ctx, hipMemcpyAsync(h_records, fe->d_pts, sizeof(svs_candidate_point) * (size_t)MP * B, hipMemcpyDeviceToHost, ctx->stream));
  SVS_HIP(ctx, hipStreamSynchronize(ctx->stream));
  // ---- the host state follows the download
  const svs_nbh_result *res = blk.host(p_res);
  bool any = false;
  for (int r = 0; r < R; ++r) {
    const svs_nbh_request &q = req[r];
    const bool over = res[r].over_capacity != 0;
    if (h_res) h_res[r] = res[r];
    fe_row_out(h_point_id, blk.host(p_pid), r, (size_t)MP, over);
    fe_row_out(h_vertex_id, blk.host(p_vid), r, (size_t)VB, over);
    fe_row_out(h_vertex_T, blk.host(p_vT), r, (size_t)VB * 12, over);
    if (over) continue;
    any = true;
    fe->n_points[q.stream] = res[r].n_points; fe->n_new_records[q.stream] = q.n_head;
    fe->max_groups_used = std::max(fe->max_groups_used, q.n_head_groups + 1);
    if (refresh_poses) fe_refresh_poses(fe, map, q.stream, q.h_slot_kf, blk.host(p_slot) + (size_t)r * K * 12);
  }
  if (any) fe_lists_changed(fe);
  return SVS_OK;
}

extern "C" int svs_frontend_input_view(svs_frontend *fe, uint8_t **d_left, int32_t *lstride, size_t *l_bstride, uint8_t **d_right, int32_t *rstride,
                                       size_t *r_bstride, float **d_disp, int32_t *dstride, size_t *d_bstride) {
  if (!fe) return SVS_ERR_INVALID;
  if (d_left) *d_left = fe->d_pyr[fe->i_cur][0];
  if (lstride) *lstride = fe->stride[0];
  if (l_bstride) *l_bstride = fe->lvl_elems[0];
  if (d_right) *d_right = fe->d_right[fe->i_cur];      // NULL without block matching
  if (rstride) *rstride = fe->stride[0];
  if (r_bstride) *r_bstride = fe->lvl_elems[0];
  if (d_disp) *d_disp = fe->d_disp[fe->i_cur];        // with block matching: where the disparity will be computed
  if (dstride) *dstride = fe->stride[0];
  if (d_bstride) *d_bstride = fe->lvl_elems[0];
  return SVS_OK;
}

/* the pinned host buffers the NEXT frame of stream 0 is staged in (w x h, contiguous): a frame grabber that writes its images straight into them
   (and then passes these pointers with stride = w) saves the host-side copy of 1.5 MB per 640 x 480 frame.  Valid until the next first_frame /
   submit_frame / process_frame / prefetch_frame call, which moves on to the other staging set. */
extern "C" int svs_frontend_staging_view(svs_frontend *fe, uint8_t **h_left, uint8_t **h_right, float **h_disp) {
  if (!fe) return SVS_ERR_INVALID;
  const size_t px = (size_t)fe->w[0] * fe->h[0];
  uint8_t *base = fe->h_in[fe->i_stage];
  if (h_left) *h_left = base;
  if (h_right) *h_right = base + px;
  if (h_disp) *h_disp = reinterpret_cast<float *>(base + 2 * px);
  return SVS_OK;
}

namespace {
// stage the caller's images (stream 0) in pinned memory and enqueue their upload into the "current" slots on `s`
int frontend_upload(svs_frontend *fe, int stage, hipStream_t s, const uint8_t *h_left, int lstride, const uint8_t *h_right, int rstride, const float *h_disp,
                    int dstride) {
  svs_ctx *ctx = fe->ctx;
  const int w = fe->w[0], h = fe->h[0];
  SVS_REQUIRE(ctx, h_left && lstride >= w);
  SVS_REQUIRE(ctx, fe->prm.use_block_matching ? (h_right && rstride >= w) : (h_disp && dstride >= w));
  uint8_t *in_left = fe->h_in[stage], *in_right = fe->h_in[stage] + (size_t)w * h;
  float *in_disp = reinterpret_cast<float *>(fe->h_in[stage] + 2 * (size_t)w * h);
  // a frame the caller produced IN the staging set (svs_frontend_staging_view) needs no copy; a contiguous image is one memcpy
  auto stage_rows = [](void *dst, const void *src, size_t row_bytes, size_t sstride_bytes, int rows) {
    if (dst == src) return;
    if (sstride_bytes == row_bytes) { __builtin_memcpy(dst, src, row_bytes * (size_t)rows); return; }
    for (int y = 0; y < rows; ++y) __builtin_memcpy(static_cast<char *>(dst) + (size_t)y * row_bytes, static_cast<const char *>(src) + (size_t)y * sstride_bytes, row_bytes);
  };
  stage_rows(in_left, h_left, (size_t)w, (size_t)lstride, h);
  SVS_HIP(ctx, hipMemcpy2DAsync(fe->d_pyr[fe->i_cur][0], fe->stride[0], in_left, w, w, h, hipMemcpyHostToDevice, s));
  if (fe->prm.use_block_matching) {
    stage_rows(in_right, h_right, (size_t)w, (size_t)rstride, h);
    SVS_HIP(ctx, hipMemcpy2DAsync(fe->d_right[fe->i_cur], fe->stride[0], in_right, w, w, h, hipMemcpyHostToDevice, s));
  } else {
    stage_rows(in_disp, h_disp, sizeof(float) * (size_t)w, sizeof(float) * (size_t)dstride, h);
    SVS_HIP(ctx, hipMemcpy2DAsync(fe->d_disp[fe->i_cur], sizeof(float) * fe->stride[0], in_disp, sizeof(float) * w, sizeof(float) * w, h, hipMemcpyHostToDevice, s));
  }
  return SVS_OK;
}
// device-resident frames of all streams -> the "current" slots (skipped for pointers handed out by svs_frontend_input_view)
int frontend_take_device_frames(svs_frontend *fe, const svs_frames_dev *in) {
  svs_ctx *ctx = fe->ctx;
  const int w = fe->w[0], h = fe->h[0];
  SVS_REQUIRE(ctx, in->d_left && in->lstride >= w && (fe->B == 1 || in->l_bstride >= (size_t)h * in->lstride));
  SVS_REQUIRE(ctx, fe->prm.use_block_matching ? (in->d_right && in->rstride >= w) : (in->d_disp && in->dstride >= w));
  SVS_REQUIRE(ctx, in->lstride % 4 == 0 && (!in->d_right || in->rstride % 4 == 0));
  // "frames are complete when this event has fired, recorded on whichever stream": every read of the caller's buffers on the context's stream comes behind it -- the
  // right-image copy below, the first pyramid step of the unpipelined chain and of svs_frontend_first_frames (the pipelined chain waits on its side stream as well)
  if (in->ready_event) SVS_HIP(ctx, hipStreamWaitEvent(ctx->stream, static_cast<hipEvent_t>(in->ready_event), 0));
  const dim3 grid(div_up(w / 4, 256), h, fe->B);
  // the left image is taken into the level-0 buffer by the first pyramid step (frontend_chain): one read of the frame instead of two
  fe->ext_left = in->d_left != fe->d_pyr[fe->i_cur][0] ? in->d_left : nullptr;
  fe->ext_lstride = in->lstride; fe->ext_lbstride = in->l_bstride;
  if (fe->prm.use_block_matching && in->d_right != fe->d_right[fe->i_cur]) {
    hipLaunchKernelGGL(copy_rows_kernel, grid, dim3(256), 0, ctx->stream, in->d_right, (size_t)in->rstride, in->r_bstride, fe->d_right[fe->i_cur], (size_t)fe->stride[0],
                       fe->lvl_elems[0], w / 4);
    SVS_LAUNCH_CHECK(ctx);
  }
  return SVS_OK;
}

struct DispView { const float *p; int stride; size_t bstride; };
// everything behind the arrival of the images: pyramid, (tracking), stereo, FAST, (match, motion-only, gate), cloud.  first: processFirstFrame
#define STAGE_MARK(k) do { if (fe->timing) SVS_HIP(ctx, hipEventRecord(fe->ev_stage[k], ctx->stream)); } while (0)
int frontend_chain(svs_frontend *fe, bool first, DispView dv, bool ext_frames = false, hipEvent_t frames_ready = nullptr) {
  svs_ctx *ctx = fe->ctx;
  const int B = fe->B, cur = fe->i_cur, prev = fe->i_prev, n = fe->n_launch;
  int rc;
  // Cross-frame pipeline.  The pyramid of a frame needs nothing of the frames before but a free slot (three slots: last read by the frame before the previous
  // one).  With the frames in caller-owned device buffers whose completion the caller has tied to an EVENT (svs_frames_dev::ready_event -- without one the frames
  // may still be in the making on the context's stream, and only that stream's order protects the read) it goes to the
  // low-priority side stream and is released when the PREVIOUS frame reaches its pose refinement: a caller that enqueues frame N+1 while frame N is still running
  // gets the 0.2 ms pyramid of N+1 into the tail of N's refinement (one workgroup per stream, <= 15 dependent LM iterations, most streams done early), its gate
  // and its cloud.  Results are those of the one-stream order (tests/test_gpu_frontend_batch.py).
  const bool pipe = !first && ext_frames && frames_ready && fe->ev_early[0] && fe->side_stream && ctx->fe_pipeline && ctx->fe_overlap && !fe->timing && B <= 2 * ctx->n_cu;
  svs_fast *const F = fe->fast;
  const int par = (int)(fe->pipe_run & 1u);
  hipStream_t const chain_stream0 = ctx->stream;
  if (pipe) {
    if (fe->pipe_run == 0) {                                                                  // first pipelined frame: behind everything enqueued so far
      SVS_HIP(ctx, hipEventRecord(fe->ev_fork, chain_stream0));
      SVS_HIP(ctx, hipStreamWaitEvent(fe->side_stream, fe->ev_fork, 0));
    } else {
      if (fe->pipe_run >= 2) SVS_HIP(ctx, hipStreamWaitEvent(fe->side_stream, fe->ev_late[par], 0));      // frame N-2: the last reader of this pyramid slot
      SVS_HIP(ctx, hipStreamWaitEvent(fe->side_stream, fe->ev_trk[1 - par], 0));                          // frame N-1 has reached its pose refinement
    }
    SVS_HIP(ctx, hipStreamWaitEvent(fe->side_stream, frames_ready, 0));                          // the caller's word that the frames are complete
    ctx->stream = fe->side_stream;                                                            // (a context is used by one thread at a time)
  } else fe->pipe_run = 0;
  auto back_to_chain = [&](int rc_) { ctx->stream = chain_stream0; return rc_; };
  for (int l = 1; l < 3; ++l) {                                                               // "preprocess"
    if (l == 1 && fe->ext_left)
      rc = svs_pyr_down_u8_copy(ctx, fe->ext_left, fe->w[0], fe->h[0], fe->ext_lstride, fe->ext_lbstride, fe->d_pyr[cur][1], fe->stride[1], fe->lvl_elems[1],
                                fe->d_pyr[cur][0], fe->stride[0], fe->lvl_elems[0], B);
    else
      rc = svs_pyr_down_u8(ctx, fe->d_pyr[cur][l - 1], fe->w[l - 1], fe->h[l - 1], fe->stride[l - 1], fe->lvl_elems[l - 1], fe->d_pyr[cur][l], fe->stride[l],
                           fe->lvl_elems[l], B);
    if (rc) return back_to_chain(rc);
  }
  fe->ext_left = nullptr;
  if (pipe) {
    const hipError_t e = hipEventRecord(fe->ev_early[par], fe->side_stream);
    ctx->stream = chain_stream0;
    SVS_HIP(ctx, e);
    SVS_HIP(ctx, hipStreamWaitEvent(ctx->stream, fe->ev_early[par], 0));
  }
  const int f32c = fe->i_f32, f32p = 1 - fe->i_f32;
  if (fe->prm.cuda_build) {
    if ((rc = svs_preprocess_gpu_sem(ctx, fe->d_pyr[cur][0], fe->w[0], fe->h[0], fe->stride[0], fe->lvl_elems[0], views(fe->d_f32[f32c]), views(fe->d_dx), views(fe->d_dy), fe->stride,
                                     fe->lvl_elems, 3, B)))
      return rc;
  }
  double *d_T = fe->d_small, *d_Ta = fe->d_small + 12 * (size_t)B, *d_Tcw = fe->d_small + 24 * (size_t)B, *d_Twa = fe->d_small + 36 * (size_t)B;
  STAGE_MARK(1);
  // "stereo" + "fast": they read the new pyramid (and the right image) only
  auto detect = [&]() -> int {
    int rc2;
    if (fe->prm.use_block_matching) {                                                         // "stereo"
      if ((rc2 = svs_stereo_compute(fe->stereo, fe->d_pyr[cur][0], fe->stride[0], fe->lvl_elems[0], fe->d_right[fe->i_cur], fe->stride[0], fe->lvl_elems[0], fe->d_disp[cur],
                                    fe->stride[0], fe->lvl_elems[0], B)))
        return rc2;
      dv = DispView{fe->d_disp[cur], fe->stride[0], fe->lvl_elems[0]};
    }
    STAGE_MARK(3);
    const uint8_t *imgs[3] = {fe->d_pyr[cur][0], fe->d_pyr[cur][1], fe->d_pyr[cur][2]};
    const int trials = first ? (fe->prm.fast_trials > 1 ? fe->prm.fast_trials - 1 : 5) : fe->prm.fast_trials;      // stereo_frontend.cpp:118 / :232
    return svs_fast_detect(F, imgs, fe->stride, fe->lvl_elems, B, trials);            // "fast"
  };
  // With the stage clocks off, the detector stages of a tracked frame go to the side stream.  The fork event is recorded in FRONT of the tracker's launch, so
  // nothing but the streams' priorities (side stream: lowest) orders the two: the detector's workgroups fill what the tracker leaves idle -- above all its
  // tail, when most streams have converged.  (With the clocks on, every stage runs
  // alone on the chain's stream so that the stage times add up to the step.)
  // (Only while all of the tracker's workgroups -- one per stream, two per CU -- are resident at once: beyond that the tracker has its own queue of
  // workgroups to fill the tail with, and detector workgroups in between only delay it: 7.01 vs 6.78 ms per step at 1024 streams.)
  const bool side = !first && fe->side_stream && ctx->fe_overlap && !fe->timing && B <= 2 * ctx->n_cu;
  if (side) SVS_HIP(ctx, hipEventRecord(fe->ev_fork, ctx->stream));
  if (!first) {                                                                               // "dense tracking"
    if (fe->prm.cuda_build) {
      svs_dense_track_full_args ta{};
      for (int l = 0; l < 3; ++l) {
        ta.d_cloud4[l] = fe->d_cloud[l]; ta.stride_f4[l] = fe->w[l]; ta.cloud_bstride[l] = fe->cloud_elems[l] / 4;
        ta.d_prev[l] = fe->d_f32[f32p][l]; ta.d_cur[l] = fe->d_f32[f32c][l]; ta.d_dx[l] = fe->d_dx[l]; ta.d_dy[l] = fe->d_dy[l];
        ta.stride_f[l] = fe->stride[l]; ta.f_bstride[l] = fe->lvl_elems[l]; ta.w[l] = fe->w[l]; ta.h[l] = fe->h[l];
        ta.f[l] = fe->cams[l].f; ta.cx[l] = fe->cams[l].cx; ta.cy[l] = fe->cams[l].cy;
      }
      ta.d_record_out = fe->d_rec; ta.record_cap = REC_CAP; ta.d_n_record_out = fe->d_nrec;
      if ((rc = svs_dense_track_full(ctx, &ta, d_T, fe->d_passes, B))) return rc;
    } else {
      svs_dense_track_args ta{};
      for (int l = 0; l < 3; ++l) {
        ta.d_cloud[l] = fe->d_cloud[l]; ta.cloud_bstride[l] = fe->cloud_elems[l];
        ta.d_prev_u8[l] = fe->d_pyr[prev][l]; ta.pstride[l] = fe->stride[l]; ta.p_bstride[l] = fe->lvl_elems[l];
        ta.d_cur_u8[l] = fe->d_pyr[cur][l]; ta.c8stride[l] = fe->stride[l]; ta.c8_bstride[l] = fe->lvl_elems[l]; ta.cam_vec[l] = fe->cams[l];
      }
      ta.d_record_out = fe->d_rec; ta.record_cap = REC_CAP; ta.d_n_record_out = fe->d_nrec;
      if ((rc = svs_dense_track_cpu_sem_work(ctx, &ta, d_T, fe->d_passes, B, fe->d_trk_work))) return rc;
    }
  }
  STAGE_MARK(2);
  if (side) {
    hipStream_t chain_stream = ctx->stream;
    SVS_HIP(ctx, hipStreamWaitEvent(fe->side_stream, fe->ev_fork, 0));
    ctx->stream = fe->side_stream;                                                            // (a context is used by one thread at a time)
    rc = detect();
    const hipError_t e = rc ? hipSuccess : hipEventRecord(fe->ev_join, fe->side_stream);
    ctx->stream = chain_stream;
    if (rc) return rc;
    SVS_HIP(ctx, e);
    SVS_HIP(ctx, hipStreamWaitEvent(ctx->stream, fe->ev_join, 0));
  } else if ((rc = detect())) return rc;
  STAGE_MARK(4);
  bool fused_tail = false;
  if (!first) {
    if (n > 0) {                                                                              // "match" + calcFastMotionOnly + "process points"
      // T_cur_from_w / T_w_from_actkey (matcher.cpp:326-330): with a handful of keyframes per stream the matcher's prediction kernel forms them itself (match.hip:
      // match_predict_kernel<true>, same expressions, same bits) -- between the tracker and the matcher every launch is on the step's critical path
      const bool pose_in_matcher = fe->max_keyframes <= 8;
      if (!pose_in_matcher) {
        hipLaunchKernelGGL(frontend_pose_kernel, dim3(B), dim3(64), 0, ctx->stream, (const double *)d_T, (const double *)d_Ta, d_Tcw, d_Twa);
        SVS_LAUNCH_CHECK(ctx);
      }
      svs_match_args ma{};
      ma.d_kfs = fe->d_kfs; ma.n_kf = fe->max_keyframes; ma.kf_bstride = (size_t)fe->max_keyframes; ma.d_pts = fe->d_pts; ma.n_pts = n;
      ma.pts_bstride = (size_t)fe->max_points; ma.out_bstride = (size_t)fe->max_points;
      ma.d_T_cur_from_w = d_Tcw; ma.d_T_w_from_actkey = d_Twa;
      for (int l = 0; l < 3; ++l) { ma.d_cur_pyr[l] = fe->d_pyr[cur][l]; ma.cur_stride[l] = fe->stride[l]; ma.cur_bstride[l] = fe->lvl_elems[l]; ma.cam_vec[l] = fe->cams[l]; }
      ma.d_disp = dv.p; ma.disp_stride = dv.stride; ma.disp_bstride = dv.bstride;
      ma.search_radius = fe->prm.search_radius; ma.thr_mean = fe->prm.thr_mean; ma.thr_std = fe->prm.thr_std; ma.n_batch = B;
      ctx->match_src_T = pose_in_matcher ? d_T : nullptr; ctx->match_src_Ta = pose_in_matcher ? d_Ta : nullptr;
      rc = svs_match(ctx, &ma, F, fe->d_res);
      ctx->match_src_T = ctx->match_src_Ta = nullptr;
      if (rc) return rc;
      // the reference refines inside match (returnBestMatch, matcher.cpp:198-204): the cut below counts the observations that are left after the refinement
      if (fe->subpix && (rc = svs_match_subpixel_behind_match(ctx, &ma, &fe->subpix_prm, fe->d_res, fe->d_subpix_info))) return rc;
      if (fe->max_groups_used > 2) {
        hipLaunchKernelGGL(frontend_group_cut_kernel, dim3(B), dim3(256), 0, ctx->stream, fe->d_res, (size_t)fe->max_points, (const int32_t *)fe->d_group_end,
                           (const int32_t *)fe->d_n_groups, fe->prm.num_max_points);
        SVS_LAUNCH_CHECK(ctx);
      }
      STAGE_MARK(5);
      svs_pose_opt_params po = fe->prm.pose_opt;
      po.min_obs = fe->prm.min_matches;
      if (pipe) SVS_HIP(ctx, hipEventRecord(fe->ev_trk[par], ctx->stream));                     // releases the next frame's pyramid (side stream)
      // refinement, gate and clouds in one launch (not with the stage clocks on: the stages are then launched, and timed, one by one)
      // (and not for a stream or two: their gate and clouds are faster spread over a hundred workgroups than behind one another in the stream's own)
      if (!fe->timing && !fe->prm.cuda_build && ctx->fe_fuse_tail && 2 * B >= ctx->n_cu) {
        svs_mo_tail tl{};
        tl.pts = fe->d_pts; tl.pts_b = (size_t)fe->max_points; tl.n_new = fe->d_n_new; tl.mre = fe->prm.max_reproj_error; tl.gated = fe->d_gated;
        tl.gated_b = (size_t)fe->max_points; tl.ptstats = fe->d_ptstats; tl.disp = dv.p; tl.ds = dv.stride; tl.disp_b = dv.bstride;
        for (int l = 0; l < 3; ++l) { tl.cams[l] = fe->cams[l]; tl.cloud[l] = fe->d_cloud[l]; tl.cloud_b[l] = fe->cloud_elems[l]; }
        tl.order = fe->d_trk_work ? svs_dense_track_balance_order(ctx, fe->d_trk_work, B) : nullptr;
        rc = svs_motion_only_gate_cloud(ctx, fe->d_res, n, (size_t)fe->max_points, &fe->cams[0], &po, d_T, fe->d_pstats, &tl, B);
        if (rc == SVS_OK) fused_tail = true;
        else if (rc != SVS_ERR_UNSUPPORTED) return rc;
      }
      if (!fused_tail) {
        if ((rc = svs_motion_only(ctx, fe->d_res, n, (size_t)fe->max_points, &fe->cams[0], &po, d_T, fe->d_pstats, B))) return rc;
        STAGE_MARK(6);
        if ((rc = svs_process_matched_points_dev(ctx, fe->d_res, fe->d_pts, n, (size_t)fe->max_points, (size_t)fe->max_points, fe->d_n_new, &fe->cams[0], d_T,
                                                 fe->prm.max_reproj_error, fe->d_gated, (size_t)fe->max_points, fe->d_ptstats, B)))
          return rc;
      }
    } else {
      if (pipe) SVS_HIP(ctx, hipEventRecord(fe->ev_trk[par], ctx->stream));
      SVS_HIP(ctx, hipMemsetAsync(fe->d_pstats, 0, (sizeof(svs_pose_opt_stats) + sizeof(svs_point_stats)) * (size_t)B, ctx->stream));
      STAGE_MARK(5); STAGE_MARK(6);
    }
  } else { STAGE_MARK(5); STAGE_MARK(6); }
  STAGE_MARK(7);
  if (!fused_tail && !fe->prm.cuda_build) {                                                   // "dense point cloud" (reference for the next frame): three levels, one launch
    size_t cb[3] = {fe->cloud_elems[0], fe->cloud_elems[1], fe->cloud_elems[2]};
    if ((rc = svs_pointcloud_cpu_sem_levels(ctx, dv.p, dv.stride, dv.bstride, fe->cams, d_T, views(fe->d_cloud), cb, B))) return rc;
  }
  for (int l = 0; l < 3 && !fused_tail && fe->prm.cuda_build; ++l) {
    if (fe->prm.cuda_build)
      rc = svs_pointcloud_full_pose(ctx, d_T, &fe->cams[l], dv.p, dv.stride, dv.bstride, fe->w[l], fe->h[l], fe->w[l], fe->cloud_elems[l] / 4, 1 << l, fe->d_cloud[l], B);
    else
      rc = svs_pointcloud_cpu_sem(ctx, dv.p, dv.stride, dv.bstride, &fe->cams[l], l, d_T, fe->d_cloud[l], fe->cloud_elems[l], B);
    if (rc) return rc;
  }
  STAGE_MARK(8);
  if (pipe) { SVS_HIP(ctx, hipEventRecord(fe->ev_late[par], ctx->stream)); ++fe->pipe_run; }
  fe->last_disp = dv.p; fe->last_dstride = dv.stride; fe->last_dbstride = dv.bstride;
  fe->n_gated = first ? -1 : n;
  ++fe->step_serial; fe->pose_replaced = false;
  fe->subpix_n = fe->subpix && !first && n > 0 ? n : -1;
  return SVS_OK;
}
void frontend_rotate(svs_frontend *fe) {
  const int p = fe->i_prev;
  fe->i_prev = fe->i_cur; fe->i_cur = fe->i_next; fe->i_next = p;       // this frame is the previous one from now on
  fe->i_f32 = 1 - fe->i_f32;
  fe->prefetched = false;
}
double *stage_poses(svs_frontend *fe, int stage) { return reinterpret_cast<double *>(fe->h_in[stage] + 2 * (size_t)fe->w[0] * fe->h[0] + sizeof(float) * (size_t)fe->w[0] * fe->h[0]); }
// make staging set `stage` writable again: the copies that read it last have completed
int stage_acquire(svs_frontend *fe, int stage) {
  SVS_HIP(fe->ctx, hipEventSynchronize(fe->ev_upload[stage]));
  return SVS_OK;
}
}  // namespace

/* upload the NEXT frame of stream 0 on a copy stream while the frame submitted last is still being processed (the reference's FrameData double
   buffer, frame_grabber.hpp:93-155).  The next svs_frontend_submit_frame / process_frame / first_frame must then pass NULL images. */
extern "C" int svs_frontend_prefetch_frame(svs_frontend *fe, const uint8_t *h_left, int lstride, const uint8_t *h_right, int rstride, const float *h_disp, int dstride) {
  svs_ctx *ctx = fe ? fe->ctx : nullptr;
  SVS_REQUIRE(ctx, fe && fe->B == 1 && !fe->prefetched);
  SVS_DEVICE(ctx);
  const int stage = fe->i_stage;
  int rc = stage_acquire(fe, stage);
  if (rc) return rc;
  // the slots written here (pyramid / disparity / right-image slot i_cur) were last READ by the frame before the one in flight
  SVS_HIP(ctx, hipStreamWaitEvent(fe->copy_stream, fe->ev_done[(fe->n_submitted + 1) & 1], 0));
  if ((rc = frontend_upload(fe, stage, fe->copy_stream, h_left, lstride, h_right, rstride, h_disp, dstride))) return rc;
  SVS_HIP(ctx, hipEventRecord(fe->ev_upload[stage], fe->copy_stream));
  fe->prefetched = true;
  return SVS_OK;
}

static int frontend_begin(svs_frontend *fe, const uint8_t *h_left, int lstride, const uint8_t *h_right, int rstride, const float *h_disp, int dstride, int *stage_out) {
  svs_ctx *ctx = fe->ctx;
  const int stage = fe->i_stage;
  int rc;
  if (fe->prefetched) {
    SVS_REQUIRE(ctx, !h_left);                                        // the frame is on its way already
    SVS_HIP(ctx, hipStreamWaitEvent(ctx->stream, fe->ev_upload[stage], 0));
  } else {
    if ((rc = stage_acquire(fe, stage))) return rc;
    if ((rc = frontend_upload(fe, stage, ctx->stream, h_left, lstride, h_right, rstride, h_disp, dstride))) return rc;
  }
  *stage_out = stage;
  return SVS_OK;
}
static int frontend_end(svs_frontend *fe, int stage, bool host_images) {
  svs_ctx *ctx = fe->ctx;
  if (host_images) {
    SVS_HIP(ctx, hipEventRecord(fe->ev_upload[stage], ctx->stream));      // images (this stream waited for a prefetch) and poses have left the staging set
    fe->i_stage = 1 - fe->i_stage;
  }
  fe->n_submitted++;
  SVS_HIP(ctx, hipEventRecord(fe->ev_done[fe->n_submitted & 1], ctx->stream));
  frontend_rotate(fe);
  return SVS_OK;
}

// StereoFrontend::processFirstFrame (stereo_frontend.cpp:110-131): disparity, FAST with 5 trials, reference cloud at the identity
extern "C" int svs_frontend_first_frame(svs_frontend *fe, const uint8_t *h_left, int lstride, const uint8_t *h_right, int rstride,
                                        const float *h_disp, int dstride) {
  svs_ctx *ctx = fe ? fe->ctx : nullptr;
  SVS_REQUIRE(ctx, fe && fe->B == 1 && !fe->submitted);
  SVS_DEVICE(ctx);
  int stage, rc;
  if ((rc = frontend_begin(fe, h_left, lstride, h_right, rstride, h_disp, dstride, &stage))) return rc;
  const double I[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};
  double *in_T = stage_poses(fe, stage);
  for (int i = 0; i < 12; ++i) in_T[i] = I[i];
  SVS_HIP(ctx, hipMemcpyAsync(fe->d_small, in_T, sizeof(double) * 12, hipMemcpyHostToDevice, ctx->stream));
  if ((rc = frontend_chain(fe, true, DispView{fe->d_disp[fe->i_cur], fe->stride[0], fe->lvl_elems[0]}))) return rc;
  if ((rc = frontend_end(fe, stage, true))) return rc;
  SVS_HIP(ctx, hipStreamSynchronize(ctx->stream));
  fe->have_prev = true;
  return SVS_OK;
}

/* processFirstFrame for all streams, frames in device memory (in == NULL: written in place through svs_frontend_input_view) */
extern "C" int svs_frontend_first_frames(svs_frontend *fe, const svs_frames_dev *in) {
  svs_ctx *ctx = fe ? fe->ctx : nullptr;
  SVS_REQUIRE(ctx, fe && !fe->submitted && !fe->prefetched);
  SVS_DEVICE(ctx);
  int rc;
  if (in && (rc = frontend_take_device_frames(fe, in))) return rc;
  std::vector<double> I((size_t)fe->B * 12, 0.0);
  for (int b = 0; b < fe->B; ++b) I[12 * b] = I[12 * b + 5] = I[12 * b + 10] = 1.0;
  SVS_HIP(ctx, hipMemcpyAsync(fe->d_small, I.data(), sizeof(double) * 12 * fe->B, hipMemcpyHostToDevice, ctx->stream));
  DispView dv = in && in->d_disp ? DispView{in->d_disp, in->dstride, in->d_bstride} : DispView{fe->d_disp[fe->i_cur], fe->stride[0], fe->lvl_elems[0]};
  if ((rc = frontend_chain(fe, true, dv))) return rc;
  if ((rc = frontend_end(fe, 0, false))) return rc;
  SVS_HIP(ctx, hipStreamSynchronize(ctx->stream));
  fe->have_prev = true;
  return SVS_OK;
}

/* processFrame for all streams, asynchronous on the context's stream: frames in device memory (in == NULL: written in place through
   svs_frontend_input_view), poses [n_streams][12] from the host.  Results stay on the device until svs_frontend_results / svs_frontend_poses. */
extern "C" int svs_frontend_process_frames(svs_frontend *fe, const svs_frames_dev *in, const double *h_T_cur_from_actkey, const double *h_T_actkey_from_w) {
  svs_ctx *ctx = fe ? fe->ctx : nullptr;
  SVS_REQUIRE(ctx, fe && h_T_cur_from_actkey && h_T_actkey_from_w && fe->have_prev && !fe->submitted && !fe->prefetched);
  SVS_DEVICE(ctx);
  int rc;
  if (fe->timing) SVS_HIP(ctx, hipEventRecord(fe->ev_stage[0], ctx->stream));
  if (in && (rc = frontend_take_device_frames(fe, in))) return rc;
  const int stage = fe->i_stage;
  if ((rc = stage_acquire(fe, stage))) return rc;
  double *in_T = stage_poses(fe, stage);
  const size_t nT = (size_t)12 * fe->B;
  __builtin_memcpy(in_T, h_T_cur_from_actkey, sizeof(double) * nT);
  __builtin_memcpy(in_T + nT, h_T_actkey_from_w, sizeof(double) * nT);
  SVS_HIP(ctx, hipMemcpyAsync(fe->d_small, in_T, sizeof(double) * 2 * nT, hipMemcpyHostToDevice, ctx->stream));
  SVS_HIP(ctx, hipEventRecord(fe->ev_upload[stage], ctx->stream));
  fe->i_stage = 1 - fe->i_stage;
  DispView dv = in && in->d_disp ? DispView{in->d_disp, in->dstride, in->d_bstride} : DispView{fe->d_disp[fe->i_cur], fe->stride[0], fe->lvl_elems[0]};
  const bool ext_frames = in && fe->ext_left && in->d_disp && !fe->prm.use_block_matching;      // caller-owned, complete device frames: the pipelined schedule may run
  if ((rc = frontend_chain(fe, false, dv, ext_frames, in ? static_cast<hipEvent_t>(in->ready_event) : nullptr))) return rc;
  return frontend_end(fe, 0, false);
}

static void fill_result(const svs_frontend *fe, const uint8_t *small, int stream, svs_frame_result *out) {
  const size_t B = (size_t)fe->B;
  const double *T = reinterpret_cast<const double *>(small) + 12 * (size_t)stream;
  for (int i = 0; i < 12; ++i) out->T_cur_from_actkey[i] = T[i];
  const uint8_t *p = small + sizeof(double) * 48 * B;
  __builtin_memcpy(&out->pose_stats, p + sizeof(svs_pose_opt_stats) * stream, sizeof(svs_pose_opt_stats));
  p += sizeof(svs_pose_opt_stats) * B;
  __builtin_memcpy(&out->point_stats, p + sizeof(svs_point_stats) * stream, sizeof(svs_point_stats));
  p += sizeof(svs_point_stats) * B;
  __builtin_memcpy(&out->dense_passes, p + sizeof(int32_t) * stream, sizeof(int32_t));
  out->n_points = fe->n_points[stream];
  out->n_matched = out->n_points > 0 ? out->pose_stats.num_obs : 0;
  out->tracking_ok = out->n_matched >= fe->prm.min_matches ? 1 : 0;                            // matchAndTrack's minimum (stereo_frontend.cpp:1053-1056)
  // dense_passes < 0: the multi-workgroup tracker could not get its workgroups resident together (the device is shared with other work) and left the pose
  // untouched -- the frame was NOT tracked, whatever the matcher made of the motion-model pose (the callers turn this into SVS_ERR_BUSY)
  if (out->dense_passes < 0) out->tracking_ok = 0;
}

/* blocking: the results of one stream of the last svs_frontend_process_frames */
extern "C" int svs_frontend_results(svs_frontend *fe, int stream, svs_frame_result *out, svs_match_result *h_matches, svs_gated_point *h_gated) {
  svs_ctx *ctx = fe ? fe->ctx : nullptr;
  SVS_REQUIRE(ctx, fe && out && stream >= 0 && stream < fe->B && !fe->submitted);
  SVS_DEVICE(ctx);
  std::vector<uint8_t> small(fe->small_bytes);
  SVS_HIP(ctx, hipMemcpyAsync(small.data(), fe->d_small, fe->small_bytes, hipMemcpyDeviceToHost, ctx->stream));
  const int n = fe->n_points[stream];
  if (n > 0 && h_matches) SVS_HIP(ctx, hipMemcpyAsync(h_matches, fe->d_res + (size_t)stream * fe->max_points, sizeof(svs_match_result) * (size_t)n, hipMemcpyDeviceToHost, ctx->stream));
  if (n > 0 && h_gated) SVS_HIP(ctx, hipMemcpyAsync(h_gated, fe->d_gated + (size_t)stream * fe->max_points, sizeof(svs_gated_point) * (size_t)n, hipMemcpyDeviceToHost, ctx->stream));
  SVS_HIP(ctx, hipStreamSynchronize(ctx->stream));
  fill_result(fe, small.data(), stream, out);
  if (out->dense_passes < 0) { ctx->err = "dense tracker: workgroups of one stream not co-resident (device busy); frame not tracked, call may be repeated"; return SVS_ERR_BUSY; }
  return SVS_OK;
}

/* the sub-pixel pass behind the matcher, from the next step on; prm == NULL: off */
extern "C" int svs_frontend_set_subpixel(svs_frontend *fe, const svs_subpix_params *prm) {
  svs_ctx *ctx = fe ? fe->ctx : nullptr;
  SVS_REQUIRE(ctx, fe && !fe->submitted);
  if (!prm) { fe->subpix = false; fe->subpix_n = -1; return SVS_OK; }
  SVS_REQUIRE(ctx, svs_subpix_params_ok(prm));
  SVS_DEVICE(ctx);
  if (!fe->d_subpix_info) SVS_HIP(ctx, fe->d_subpix_info.alloc((size_t)fe->max_points * fe->B));
  fe->subpix_prm = *prm; fe->subpix = true;
  return SVS_OK;
}
/* blocking: the svs_subpix_info records of one stream's last step (n_points of them) */
extern "C" int svs_frontend_subpixel_info(svs_frontend *fe, int stream, svs_subpix_info *h_info) {
  svs_ctx *ctx = fe ? fe->ctx : nullptr;
  SVS_REQUIRE(ctx, fe && stream >= 0 && stream < fe->B && !fe->submitted);
  SVS_REQUIRE(ctx, fe->subpix && fe->subpix_n >= 0);      // refused while the option is off, and before a step has run the pass
  SVS_DEVICE(ctx);
  const int n = std::min(fe->n_points[stream], fe->subpix_n);
  if (n > 0) {
    SVS_REQUIRE(ctx, h_info);
    SVS_HIP(ctx, hipMemcpyAsync(h_info, fe->d_subpix_info + (size_t)stream * fe->max_points, sizeof(svs_subpix_info) * (size_t)n, hipMemcpyDeviceToHost, ctx->stream));
  }
  SVS_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return SVS_OK;
}

/* blocking: refined poses [n_streams][12], tracking flags [n_streams] (either may be NULL) of the last svs_frontend_process_frames */
extern "C" int svs_frontend_poses(svs_frontend *fe, double *h_T_cur_from_actkey, int32_t *h_tracking_ok) {
  svs_ctx *ctx = fe ? fe->ctx : nullptr;
  SVS_REQUIRE(ctx, fe && !fe->submitted);
  SVS_DEVICE(ctx);
  std::vector<uint8_t> small(fe->small_bytes);
  SVS_HIP(ctx, hipMemcpyAsync(small.data(), fe->d_small, fe->small_bytes, hipMemcpyDeviceToHost, ctx->stream));
  SVS_HIP(ctx, hipStreamSynchronize(ctx->stream));
  for (int b = 0; b < fe->B; ++b) {
    svs_frame_result r;
    fill_result(fe, small.data(), b, &r);
    if (h_T_cur_from_actkey) for (int i = 0; i < 12; ++i) h_T_cur_from_actkey[12 * b + i] = r.T_cur_from_actkey[i];
    if (h_tracking_ok) h_tracking_ok[b] = r.tracking_ok;
  }
  return SVS_OK;
}

/* processFrame of stream 0 in two halves: submit enqueues upload (unless prefetched: pass NULL images) + all stages + the download and returns;
   wait blocks and hands the results out.  Between the two the caller may prefetch the next frame. */
extern "C" int svs_frontend_submit_frame(svs_frontend *fe, const uint8_t *h_left, int lstride, const uint8_t *h_right, int rstride, const float *h_disp, int dstride,
                                         const double *T_cur_from_actkey, const double *T_actkey_from_w, int want_matches, int want_gated) {
  svs_ctx *ctx = fe ? fe->ctx : nullptr;
  SVS_REQUIRE(ctx, fe && fe->B == 1 && T_cur_from_actkey && T_actkey_from_w && fe->have_prev && !fe->submitted);
  SVS_DEVICE(ctx);
  int stage, rc;
  if (fe->timing) SVS_HIP(ctx, hipEventRecord(fe->ev_stage[0], ctx->stream));
  if ((rc = frontend_begin(fe, h_left, lstride, h_right, rstride, h_disp, dstride, &stage))) return rc;
  double *in_T = stage_poses(fe, stage);
  for (int i = 0; i < 12; ++i) { in_T[i] = T_cur_from_actkey[i]; in_T[12 + i] = T_actkey_from_w[i]; }
  SVS_HIP(ctx, hipMemcpyAsync(fe->d_small, in_T, sizeof(double) * 24, hipMemcpyHostToDevice, ctx->stream));
  if ((rc = frontend_chain(fe, false, DispView{fe->d_disp[fe->i_cur], fe->stride[0], fe->lvl_elems[0]}))) return rc;
  // one download: small block, then the records
  const int n = fe->n_points[0];
  if (fe->d_out_block && n > 0 && want_matches && want_gated) {      // the device block has the pinned buffer's layout: everything up to the last gated record in ONE copy
    SVS_HIP(ctx, hipMemcpyAsync(fe->h_out, fe->d_out_block, fe->small_bytes + sizeof(svs_match_result) * (size_t)fe->max_points + sizeof(svs_gated_point) * (size_t)n,
                                hipMemcpyDeviceToHost, ctx->stream));
  } else {
    SVS_HIP(ctx, hipMemcpyAsync(fe->h_out, fe->d_small, fe->small_bytes, hipMemcpyDeviceToHost, ctx->stream));
    svs_match_result *o_res = reinterpret_cast<svs_match_result *>(fe->h_out + fe->small_bytes);
    svs_gated_point *o_gated = reinterpret_cast<svs_gated_point *>(fe->h_out + fe->small_bytes + sizeof(svs_match_result) * (size_t)fe->max_points);
    if (n > 0 && want_matches) SVS_HIP(ctx, hipMemcpyAsync(o_res, fe->d_res, sizeof(svs_match_result) * (size_t)n, hipMemcpyDeviceToHost, ctx->stream));
    if (n > 0 && want_gated) SVS_HIP(ctx, hipMemcpyAsync(o_gated, fe->d_gated, sizeof(svs_gated_point) * (size_t)n, hipMemcpyDeviceToHost, ctx->stream));
  }
  if ((rc = frontend_end(fe, stage, true))) return rc;
  fe->submitted = true; fe->want_matches = want_matches != 0; fe->want_gated = want_gated != 0;
  return SVS_OK;
}
extern "C" int svs_frontend_wait_frame(svs_frontend *fe, svs_frame_result *out, svs_match_result *h_matches, svs_gated_point *h_gated) {
  svs_ctx *ctx = fe ? fe->ctx : nullptr;
  SVS_REQUIRE(ctx, fe && out && fe->submitted);
  SVS_REQUIRE(ctx, (!h_matches || fe->want_matches) && (!h_gated || fe->want_gated));
  SVS_DEVICE(ctx);
  fe->submitted = false;
  SVS_HIP(ctx, hipStreamSynchronize(ctx->stream));
  fill_result(fe, fe->h_out, 0, out);
  const int n = fe->n_points[0];
  const svs_match_result *o_res = reinterpret_cast<const svs_match_result *>(fe->h_out + fe->small_bytes);
  const svs_gated_point *o_gated = reinterpret_cast<const svs_gated_point *>(fe->h_out + fe->small_bytes + sizeof(svs_match_result) * (size_t)fe->max_points);
  if (n > 0 && h_matches) __builtin_memcpy(h_matches, o_res, sizeof(svs_match_result) * (size_t)n);
  if (n > 0 && h_gated) __builtin_memcpy(h_gated, o_gated, sizeof(svs_gated_point) * (size_t)n);
  return SVS_OK;
}

extern "C" int svs_frontend_process_frame(svs_frontend *fe, const uint8_t *h_left, int lstride, const uint8_t *h_right, int rstride,
                                          const float *h_disp, int dstride, const double *T_cur_from_actkey, const double *T_actkey_from_w,
                                          svs_frame_result *out, svs_match_result *h_matches, svs_gated_point *h_gated) {
  svs_ctx *ctx = fe ? fe->ctx : nullptr;
  SVS_REQUIRE(ctx, fe && out);
  const int rc = svs_frontend_submit_frame(fe, h_left, lstride, h_right, rstride, h_disp, dstride, T_cur_from_actkey, T_actkey_from_w, h_matches != nullptr,
                                           h_gated != nullptr);
  if (rc) return rc;
  return svs_frontend_wait_frame(fe, out, h_matches, h_gated);
}

/* computeDensePointCloudCpu / Gpu again, at a pose the caller decided on after the frame (keyframe switch, stereo_frontend.cpp:277-281) */
extern "C" int svs_frontend_recompute_cloud(svs_frontend *fe, const double *T_cur_from_actkey) {
  svs_ctx *ctx = fe ? fe->ctx : nullptr;
  SVS_REQUIRE(ctx, fe && T_cur_from_actkey && fe->have_prev && !fe->submitted);      // T_cur_from_actkey [n_streams][12]
  SVS_DEVICE(ctx);
  SVS_HIP(ctx, hipStreamSynchronize(ctx->stream));
  SVS_HIP(ctx, hipMemcpy(fe->d_small, T_cur_from_actkey, sizeof(double) * 12 * fe->B, hipMemcpyHostToDevice));
  fe->pose_replaced = true;            // (svs_frontend_commit_keyframe: the step's refined poses are gone, for every stream)
  const float *disp = fe->last_disp;      // the disparity the frame processed last was given (the caller's buffer, if it passed one) or produced
  SVS_REQUIRE(ctx, disp);
  for (int l = 0; l < 3; ++l) {
    int rc;
    if (fe->prm.cuda_build)
      rc = svs_pointcloud_full_pose(ctx, fe->d_small, &fe->cams[l], disp, fe->last_dstride, fe->last_dbstride, fe->w[l], fe->h[l], fe->w[l], fe->cloud_elems[l] / 4, 1 << l, fe->d_cloud[l], fe->B);
    else
      rc = svs_pointcloud_cpu_sem(ctx, disp, fe->last_dstride, fe->last_dbstride, &fe->cams[l], l, fe->d_small, fe->d_cloud[l], fe->cloud_elems[l], fe->B);
    if (rc) return rc;
  }
  SVS_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return SVS_OK;
}

/* device views for tests / chaining: level images of the frame processed last, its disparity, the reference clouds -- of one stream */
extern "C" int svs_frontend_device_view(svs_frontend *fe, int stream, const uint8_t **d_pyr_last, int32_t *stride, const float **d_disp, const float **d_cloud,
                                        svs_fast **fast) {
  if (!fe || stream < 0 || stream >= fe->B) return SVS_ERR_INVALID;
  for (int l = 0; l < 3; ++l) {
    if (d_pyr_last) d_pyr_last[l] = fe->d_pyr[fe->i_prev][l] + fe->lvl_elems[l] * stream;
    if (stride) stride[l] = fe->stride[l];
    if (d_cloud) d_cloud[l] = fe->d_cloud[l] + fe->cloud_elems[l] * stream;
  }
  if (d_disp) *d_disp = fe->last_disp ? fe->last_disp + fe->last_dbstride * stream : nullptr;
  if (fast) *fast = fe->fast;
  return SVS_OK;
}

/* profiling: hipEvents between the stages of the next svs_frontend_process_frame(s) / submit_frame call (off by default: ~4 us of stream time each) */
extern "C" int svs_frontend_set_timing(svs_frontend *fe, int on) {
  svs_ctx *ctx = fe ? fe->ctx : nullptr;
  SVS_REQUIRE(ctx, fe);
  SVS_DEVICE(ctx);
  if (on && !fe->ev_stage[0])
    for (owned::Event &e : fe->ev_stage) SVS_HIP(ctx, e.create());
  fe->timing = on != 0;
  return SVS_OK;
}
/* blocking: ms[SVS_FRONTEND_STAGES] of the last timed call, in the order of the reference's per_mon_ stages: preprocess (upload / copy + pyramid),
   dense tracking, stereo, fast, match, pose refinement (calcFastMotionOnly), process points, dense point cloud */
extern "C" int svs_frontend_stage_times(svs_frontend *fe, float *ms) {
  svs_ctx *ctx = fe ? fe->ctx : nullptr;
  SVS_REQUIRE(ctx, fe && ms && fe->timing && fe->ev_stage[0]);
  SVS_DEVICE(ctx);
  SVS_HIP(ctx, hipStreamSynchronize(ctx->stream));
  for (int k = 0; k < SVS_FRONTEND_STAGES; ++k) SVS_HIP(ctx, hipEventElapsedTime(&ms[k], fe->ev_stage[k], fe->ev_stage[k + 1]));
  return SVS_OK;
}
/* blocking: the accept / reject record of the dense tracker's LM loop of one stream in the last call (level, accepted, chi2 before / after per chi2
   evaluation); *n = records produced (only the first min(*n, cap, 64) are stored) */
extern "C" int svs_frontend_dense_records(svs_frontend *fe, int stream, svs_dense_lm_record *h_rec, int cap, int32_t *n) {
  svs_ctx *ctx = fe ? fe->ctx : nullptr;
  SVS_REQUIRE(ctx, fe && stream >= 0 && stream < fe->B && n && cap >= 0 && (cap == 0 || h_rec));
  SVS_DEVICE(ctx);
  SVS_HIP(ctx, hipMemcpyAsync(n, fe->d_nrec + stream, sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
  SVS_HIP(ctx, hipStreamSynchronize(ctx->stream));
  const int k = std::min(std::min((int)*n, cap), REC_CAP);
  if (k > 0) SVS_HIP(ctx, hipMemcpy(h_rec, fe->d_rec + (size_t)stream * REC_CAP, sizeof(svs_dense_lm_record) * (size_t)k, hipMemcpyDeviceToHost));
  return SVS_OK;
}

namespace {
// svs_frontend_seed_newpoints' part in the call: what is checked beside the requests before anything is uploaded, and what is enqueued behind the seed kernel on its
// outputs (records [n][cap], counts [n][3], both on the device)
struct SeedSink {
  virtual int check() = 0;
  virtual int enqueue(const svs_candidate_point *d_rec, const int32_t *d_cnt, int cap) = 0;
  virtual ~SeedSink() = default;
};
}  // namespace

/* addNewPoints / addMorePoints (stereo_frontend.cpp:682-823) for n requests from the device state the last first_frame(s) / process_frame(s) call left behind:
   the corner lists of its detection, its disparity, and for SVS_SEED_MORE its gate records and point statistics (seed.hip).  One staged upload (problems, streams,
   the callers' orders), the kernels, one download (counts and records). */
// (shared by svs_frontend_seed_keyframes and svs_frontend_seed_newpoints; h_out may be NULL with a sink: only the counts come back then)
static int fe_seed_keyframes(svs_frontend *fe, int n, const svs_seed_request *req, const svs_seed_params *prm, svs_candidate_point *h_out, int cap_per_request,
                             int32_t *h_n_new, SeedSink *sink) {
  svs_ctx *ctx = fe ? fe->ctx : nullptr;
  SVS_REQUIRE(ctx, fe && n >= 0 && (n == 0 || (req && (h_out || sink) && h_n_new)) && prm && fe->have_prev && !fe->submitted && fe->last_disp);
  SVS_REQUIRE(ctx, prm->n_levels >= 1 && prm->n_levels <= fe->prm.n_levels && prm->num_max_points >= 0 && prm->num_max_points <= 65536);
  if (cap_per_request < svs_seed_max_records(prm)) {
    ctx->err = "svs_frontend_seed_keyframes: cap_per_request below the sum over the levels of (num_max_points >> l) + 1";
    return SVS_ERR_CAPACITY;
  }
  if (n == 0) return SVS_OK;
  const FastListView fv = svs_fast_list_view_internal(fe->fast);
  size_t ob[3] = {0, 0, 0};      // the callers' order lists of a level are staged [n][ob[l]]
  bool any_generated = false;
  for (int r = 0; r < n; ++r) {
    const svs_seed_request &q = req[r];
    SVS_REQUIRE(ctx, q.stream >= 0 && q.stream < fe->B && (q.mode == SVS_SEED_FIRST || q.mode == SVS_SEED_MORE));
    SVS_REQUIRE(ctx, q.mode != SVS_SEED_MORE || fe->n_gated >= 0);      // gate records and point statistics of a step on the list that is still on the device
    const bool own = q.h_order[0] || q.h_order[1] || q.h_order[2];
    any_generated = any_generated || !own;
    for (int l = 0; l < prm->n_levels && own; ++l) {
      SVS_REQUIRE(ctx, q.n_order[l] >= 0 && q.n_order[l] <= (1 << 24));
      if (q.h_order[l]) ob[l] = std::max(ob[l], (size_t)q.n_order[l]);
    }
  }
  if (sink) if (int rc = sink->check()) return rc;
  SVS_DEVICE(ctx);
  // device block, pieces of 64 bytes' alignment: problems | streams | orders of level 0, 1, 2 ; then counts [n][3] | records [n][cap].  The pinned block is NOT its
  // twin: it holds the input pieces at the same offsets on the way up and, on the way back, the row `out` = the two output pieces from offset 0 on (the counts piece
  // begins on a 64-byte boundary, so the records lie as far behind the counts in `out` as on the device and one copy brings both) -- never the megabytes in between
  const size_t nz = (size_t)n;
  Pieces<64> dv, out;
  const auto p_prob = dv.piece<svs_seed_problem>(nz); const auto p_slot = dv.piece<int32_t>(nz);
  Piece<int32_t> p_ord[3];
  for (int l = 0; l < 3; ++l) p_ord[l] = dv.piece<int32_t>(ob[l] * nz);
  const size_t in_bytes = dv.end_aligned();
  const auto p_cnt = dv.piece<int32_t>(3 * nz); const auto p_rec = dv.piece<svs_candidate_point>((size_t)cap_per_request * nz);
  const auto h_cnt = out.piece<int32_t>(3 * nz); const auto h_rec = out.piece<svs_candidate_point>((size_t)cap_per_request * nz);
  const size_t out_bytes = out.end, d_bytes = dv.end;
  // small results go home in one copy through the pinned block; big ones as the counts, then one strided copy of the longest list's width into the caller's array
  const bool one_copy = h_out && out_bytes <= ((size_t)1 << 20);
  const size_t h_bytes = std::max(in_bytes, one_copy ? out_bytes : h_rec.off);
  if (fe->h_seed.bytes() < h_bytes || fe->d_seed.bytes() < d_bytes) SVS_HIP(ctx, hipStreamSynchronize(ctx->stream));
  if (fe->h_seed.bytes() < h_bytes) SVS_HIP(ctx, fe->h_seed.alloc_bytes(h_bytes));
  if (fe->d_seed.bytes() < d_bytes) SVS_HIP(ctx, fe->d_seed.alloc_bytes(d_bytes));
  uint8_t *const hb = fe->h_seed, *const db = fe->d_seed;
  svs_seed_problem *hp = piece_at(hb, p_prob);
  int32_t *hs = piece_at(hb, p_slot);
  for (int r = 0; r < n; ++r) {
    const svs_seed_request &q = req[r];
    svs_seed_problem p{};
    for (int i = 0; i < 12; ++i) p.T_newkey_from_cur[i] = q.T_newkey_from_cur[i];
    p.seed = q.seed; p.kf_index = q.kf_index; p.first_point_id = q.first_point_id;
    const bool more = q.mode == SVS_SEED_MORE;
    for (int k = 0; k < 9; ++k) p.add_flags[k] = 1;
    for (int l = 0; l < 3; ++l) p.n0[l] = more ? -1 : 0;      // -1: counts and flags from the stream's point statistics on the device
    p.n_tree = more ? fe->n_gated : 0;
    p.use_order = (q.h_order[0] || q.h_order[1] || q.h_order[2]) ? 1 : 0;
    for (int l = 0; l < prm->n_levels && p.use_order; ++l) {
      p.n_order[l] = q.h_order[l] ? q.n_order[l] : 0;
      if (p.n_order[l]) __builtin_memcpy(piece_at(hb, p_ord[l]) + ob[l] * (size_t)r, q.h_order[l], sizeof(int32_t) * (size_t)p.n_order[l]);
    }
    hp[r] = p; hs[r] = q.stream;
  }
  SVS_HIP(ctx, hipMemcpyAsync(db, hb, in_bytes, hipMemcpyHostToDevice, ctx->stream));
  svs_seed_args a{};
  for (int l = 0; l < prm->n_levels; ++l) {
    a.d_xy[l] = fv.xy[l]; a.xy_bstride[l] = (size_t)fv.cap * 2; a.xy_cap[l] = fv.cap;
    a.d_n[l] = fv.level_total + l; a.n_bstride[l] = (size_t)fv.n_levels;
    a.d_cell_count[l] = fv.count + fv.cell_base[l]; a.cell_bstride[l] = (size_t)fv.ncell_total; a.n_cells[l] = fv.ncell[l];
    a.d_order[l] = ob[l] ? piece_at(db, p_ord[l]) : nullptr; a.order_bstride[l] = ob[l];
  }
  a.d_disp = fe->last_disp; a.disp_stride = fe->last_dstride; a.disp_bstride = fe->last_dbstride;
  a.cam = fe->cams[0];
  a.d_prob = piece_at(db, p_prob);
  a.batch = n;
  SeedFrontendSrc fs{};
  fs.slot_of = piece_at(db, p_slot);
  fs.gated = fe->d_gated; fs.pts = fe->d_pts; fs.res = fe->d_res; fs.rec_b = (size_t)fe->max_points; fs.stats = fe->d_ptstats;
  if (int rc = svs_seed_launch(ctx, &a, prm, &fs, any_generated, piece_at(db, p_rec), cap_per_request, piece_at(db, p_cnt))) return rc;
  if (sink) if (int rc = sink->enqueue(piece_at(db, p_rec), piece_at(db, p_cnt), cap_per_request)) return rc;
  SVS_HIP(ctx, hipMemcpyAsync(piece_at(hb, h_cnt), piece_at(db, p_cnt), one_copy ? out_bytes : h_rec.off, hipMemcpyDeviceToHost, ctx->stream));
  SVS_HIP(ctx, hipStreamSynchronize(ctx->stream));
  __builtin_memcpy(h_n_new, piece_at(hb, h_cnt), h_cnt.bytes());
  int longest = 0;
  for (int r = 0; r < n; ++r) longest = std::max(longest, h_n_new[3 * r] + h_n_new[3 * r + 1] + h_n_new[3 * r + 2]);
  SVS_REQUIRE(ctx, longest <= cap_per_request);
  if (one_copy) {
    const svs_candidate_point *rec = piece_at(hb, h_rec);
    for (int r = 0; r < n; ++r) {
      const int m = h_n_new[3 * r] + h_n_new[3 * r + 1] + h_n_new[3 * r + 2];
      if (m > 0) __builtin_memcpy(h_out + (size_t)r * cap_per_request, rec + (size_t)r * cap_per_request, sizeof(svs_candidate_point) * (size_t)m);
    }
  } else if (h_out && longest > 0) {      // (behind a request's own count the caller's rows receive what the device block held there: unspecified)
    const size_t pitch = sizeof(svs_candidate_point) * (size_t)cap_per_request;
    SVS_HIP(ctx, hipMemcpy2DAsync(h_out, pitch, piece_at(db, p_rec), pitch, sizeof(svs_candidate_point) * (size_t)longest, (size_t)n, hipMemcpyDeviceToHost, ctx->stream));
    SVS_HIP(ctx, hipStreamSynchronize(ctx->stream));
  }
  return SVS_OK;
}

extern "C" int svs_frontend_seed_keyframes(svs_frontend *fe, int n, const svs_seed_request *req, const svs_seed_params *prm, svs_candidate_point *h_out,
                                           int cap_per_request, int32_t *h_n_new) {
  svs_ctx *ctx = fe ? fe->ctx : nullptr;
  SVS_REQUIRE(ctx, n <= 0 || h_out);
  return fe_seed_keyframes(fe, n, req, prm, h_out, cap_per_request, h_n_new, nullptr);
}

// the resident vertex tables, the decision records and the list rows come with the first table (tables, vertices and slot tables zeroed: a stream's rows can be
// read back before they were ever set)
static int fe_vt_reserve(svs_frontend *fe) {
  svs_ctx *ctx = fe->ctx;
  if (fe->d_vt_tab) return SVS_OK;
  const size_t Bz = (size_t)fe->B, mp = (size_t)fe->max_points, S = (size_t)fe->max_keyframes;
  SVS_HIP(ctx, fe->d_vt_tab.alloc(Bz));
  SVS_HIP(ctx, fe->d_vt_vtx.alloc(Bz * SVS_KF_MAX_VERTICES));
  SVS_HIP(ctx, fe->d_vt_slot.alloc(Bz * S));
  SVS_HIP(ctx, fe->d_vt_ids.alloc(Bz * 16 * mp));
  SVS_HIP(ctx, fe->d_kd_dec.alloc(Bz));
  SVS_HIP(ctx, fe->d_kd_new.alloc(Bz * mp));
  SVS_HIP(ctx, fe->d_kd_track.alloc(Bz * mp));
  SVS_HIP(ctx, fe->d_kd_new_rec.alloc(Bz * mp));
  SVS_HIP(ctx, fe->d_kd_track_rec.alloc(Bz * mp));
  SVS_HIP(ctx, fe->h_kd_dec.alloc(Bz));
  SVS_HIP(ctx, hipMemsetAsync(fe->d_vt_tab, 0, sizeof(svs_kf_table) * Bz, ctx->stream));
  SVS_HIP(ctx, hipMemsetAsync(fe->d_vt_vtx, 0, sizeof(svs_kf_vertex) * Bz * SVS_KF_MAX_VERTICES, ctx->stream));
  SVS_HIP(ctx, hipMemsetAsync(fe->d_vt_slot, 0, sizeof(int32_t) * Bz * S, ctx->stream));
  fe->vt_set.assign(Bz, 0);
  return SVS_OK;
}

/* neighborhood_->vertex_map of a stream as the keyframe decision reads it (keyframe.hip; the contract is in the header): everything is checked on the host first,
   then one staged upload (requests, tables, vertices, slot tables, id arrays) and one scatter launch into the stream-indexed resident tables. */
extern "C" int svs_frontend_set_vertex_table(svs_frontend *fe, int n_requests, const svs_vertex_request *req) {
  svs_ctx *ctx = fe ? fe->ctx : nullptr;
  SVS_REQUIRE(ctx, fe && n_requests >= 0 && (n_requests == 0 || req) && !fe->submitted);
  const int B = fe->B, S = fe->max_keyframes, R = n_requests;
  if (S > SVS_KF_MAX_SLOTS) { ctx->err = "svs_frontend_set_vertex_table: more than SVS_KF_MAX_SLOTS keyframe slots"; return SVS_ERR_UNSUPPORTED; }
  const size_t set_cap = (size_t)16 * fe->max_points;
  std::vector<uint8_t> seen((size_t)B, 0);
  size_t total_ids = 0;
  for (int r = 0; r < R; ++r) {
    const svs_vertex_request &q = req[r];
    SVS_REQUIRE(ctx, q.stream >= 0 && q.stream < B && !seen[q.stream]);
    seen[q.stream] = 1;
    SVS_REQUIRE(ctx, q.n_vertex >= 1 && q.h_vertex_kf && q.h_vertex_T && q.h_set_begin && q.h_set_count && q.h_slot_kf && q.n_set_ids >= 0 && (q.n_set_ids == 0 || q.h_set_ids));
    if (q.n_vertex > SVS_KF_MAX_VERTICES) { ctx->err = "svs_frontend_set_vertex_table: more than SVS_KF_MAX_VERTICES vertices"; return SVS_ERR_CAPACITY; }
    if ((size_t)q.n_set_ids > set_cap) { ctx->err = "svs_frontend_set_vertex_table: more than 16 * max_points staged ids"; return SVS_ERR_CAPACITY; }
    SVS_REQUIRE(ctx, q.act >= 0 && q.act < q.n_vertex && q.n_neighbors >= 0 && q.n_neighbors < q.n_vertex && (q.n_neighbors == 0 || q.h_neighbors));
    for (int v = 0; v < q.n_vertex; ++v) {
      for (int u = 0; u < v; ++u) SVS_REQUIRE(ctx, q.h_vertex_kf[u] != q.h_vertex_kf[v]);
      if (q.h_set_begin[v] == SVS_KF_SET_MAP) continue;
      const int beg = q.h_set_begin[v], cnt = q.h_set_count[v];
      SVS_REQUIRE(ctx, beg >= 0 && cnt >= 0 && (size_t)beg + (size_t)cnt <= (size_t)q.n_set_ids);
      for (int i = 1; i < cnt; ++i) SVS_REQUIRE(ctx, q.h_set_ids[beg + i - 1] < q.h_set_ids[beg + i]);
    }
    for (int k = 0; k < q.n_neighbors; ++k) {
      SVS_REQUIRE(ctx, q.h_neighbors[k] >= 0 && q.h_neighbors[k] < q.n_vertex && q.h_neighbors[k] != q.act);
      for (int j = 0; j < k; ++j) SVS_REQUIRE(ctx, q.h_neighbors[j] != q.h_neighbors[k]);
    }
    for (int s = 0; s < S; ++s) SVS_REQUIRE(ctx, q.h_slot_kf[s] < 0 || fe->kept[(size_t)q.stream * S + s]);
    total_ids += (size_t)q.n_set_ids;
  }
  if (R == 0) return SVS_OK;
  SVS_DEVICE(ctx);
  if (int rc = fe_vt_reserve(fe)) return rc;
  Pieces<> row;
  const size_t Rz = (size_t)R;
  const auto p_up = row.piece<kfd_up>(Rz); const auto p_tab = row.piece<svs_kf_table>(Rz); const auto p_vtx = row.piece<svs_kf_vertex>(Rz * SVS_KF_MAX_VERTICES);
  const auto p_slot = row.piece<int32_t>(Rz * S); const auto p_ids = row.piece<int32_t>(total_ids);
  TwinBlock &blk = fe->vt_up;
  if (int rc = blk.reserve(ctx, row.end)) return rc;      // (the last call's upload has been waited for: it ends with a synchronisation)
  __builtin_memset(blk.h, 0, p_ids.off);
  kfd_up *hu = blk.host(p_up);
  svs_kf_table *ht = blk.host(p_tab);
  svs_kf_vertex *hv = blk.host(p_vtx);
  int32_t *hs = blk.host(p_slot), *hi = blk.host(p_ids);
  size_t ids_off = 0;
  for (int r = 0; r < R; ++r) {
    const svs_vertex_request &q = req[r];
    hu[r].stream = q.stream; hu[r].n_ids = q.n_set_ids; hu[r].ids_off = (int32_t)ids_off;
    ht[r].n_vertex = q.n_vertex; ht[r].act = q.act; ht[r].n_neighbors = q.n_neighbors;
    for (int k = 0; k < q.n_neighbors; ++k) ht[r].neighbors[k] = q.h_neighbors[k];
    for (int v = 0; v < q.n_vertex; ++v) {
      svs_kf_vertex &x = hv[(size_t)r * SVS_KF_MAX_VERTICES + v];
      for (int i = 0; i < 12; ++i) x.T_me_from_w[i] = q.h_vertex_T[12 * v + i];
      const bool from_map = q.h_set_begin[v] == SVS_KF_SET_MAP;
      x.kf_id = q.h_vertex_kf[v]; x.set_begin = q.h_set_begin[v]; x.set_count = from_map ? 0 : q.h_set_count[v];
    }
    __builtin_memcpy(hs + (size_t)r * S, q.h_slot_kf, sizeof(int32_t) * (size_t)S);
    if (q.n_set_ids) __builtin_memcpy(hi + ids_off, q.h_set_ids, sizeof(int32_t) * (size_t)q.n_set_ids);
    ids_off += (size_t)q.n_set_ids;
  }
  SVS_REQUIRE(ctx, ids_off < ((size_t)1 << 31));
  if (int rc = blk.upload(ctx, 0, row.end)) return rc;
  KfdScatter sc{};
  sc.up = blk.dev(p_up); sc.tab = blk.dev(p_tab); sc.vtx = blk.dev(p_vtx); sc.slot = blk.dev(p_slot); sc.ids = blk.dev(p_ids);
  sc.d_tab = fe->d_vt_tab; sc.d_vtx = fe->d_vt_vtx; sc.d_slot = fe->d_vt_slot; sc.d_ids = fe->d_vt_ids; sc.S = S; sc.set_cap = (int)set_cap;
  if (int rc = svs_keyframe_scatter_tables(ctx, R, sc)) return rc;
  SVS_HIP(ctx, hipStreamSynchronize(ctx->stream));
  for (int r = 0; r < R; ++r) fe->vt_set[req[r].stream] = 1;
  return SVS_OK;
}

/* stereo_frontend.cpp:265-296 for every stream, from the device state of the last step and the resident vertex tables: one launch (keyframe.hip), one download of
   the decision records, then the list rows of the streams that need them -- one strided copy per array and run of consecutive such streams. */
extern "C" int svs_frontend_decide_keyframes(svs_frontend *fe, svs_map *map, const svs_keyframe_decide_params *prm, int want_lists, svs_keyframe_decision *h_dec,
                                             svs_map_new_point *h_new, svs_map_track_point *h_track, int32_t *h_new_rec, int32_t *h_track_rec, int cap) {
  svs_ctx *ctx = fe ? fe->ctx : nullptr;
  SVS_REQUIRE(ctx, fe && prm && h_dec && fe->have_prev && !fe->submitted && want_lists >= 0 && want_lists <= 2);
  SVS_REQUIRE(ctx, fe->n_gated >= 0);      // gate records and point statistics of a step on the list that is still on the device (the SVS_SEED_MORE rule)
  const int B = fe->B;
  SVS_REQUIRE(ctx, (int)fe->vt_set.size() == B);
  for (int b = 0; b < B; ++b) SVS_REQUIRE(ctx, fe->vt_set[b]);
  SVS_REQUIRE(ctx, !want_lists || (h_new && h_track && h_new_rec && h_track_rec));
  if (want_lists && cap < fe->n_gated) { ctx->err = "svs_frontend_decide_keyframes: cap below the step's record count"; return SVS_ERR_CAPACITY; }
  SVS_DEVICE(ctx);
  const size_t mp = (size_t)fe->max_points;
  svs_keyframe_decide_args a{};
  a.d_res = fe->d_res; a.res_bstride = mp; a.d_pts = fe->d_pts; a.pts_bstride = mp; a.d_gated = fe->d_gated; a.gated_bstride = mp;
  a.d_stats = fe->d_ptstats; a.d_T_cur_from_actkey = fe->d_small; a.n = fe->n_gated; a.batch = B;
  a.d_table = fe->d_vt_tab; a.d_vertex = fe->d_vt_vtx; a.vertex_bstride = SVS_KF_MAX_VERTICES;
  a.d_set_ids = fe->d_vt_ids; a.set_bstride = (size_t)16 * mp; a.d_slot_kf = fe->d_vt_slot; a.slot_bstride = (size_t)fe->max_keyframes; a.max_keyframes = fe->max_keyframes;
  a.map = map;
  KfdFrontendSrc fs{fe->d_pstats, fe->d_passes, fe->prm.min_matches};
  if (int rc = svs_keyframe_decide_launch(ctx, &a, prm, &fs, fe->d_kd_dec, fe->d_kd_new, fe->d_kd_track, fe->d_kd_new_rec, fe->d_kd_track_rec, fe->max_points)) return rc;
  SVS_HIP(ctx, hipMemcpyAsync(fe->h_kd_dec, fe->d_kd_dec, sizeof(svs_keyframe_decision) * (size_t)B, hipMemcpyDeviceToHost, ctx->stream));
  SVS_HIP(ctx, hipStreamSynchronize(ctx->stream));
  __builtin_memcpy(h_dec, fe->h_kd_dec, sizeof(svs_keyframe_decision) * (size_t)B);
  fe->kd_serial = fe->step_serial; fe->kd_have = true;
  if (!want_lists) return SVS_OK;
  auto wanted = [&](int b) { return h_dec[b].valid && (want_lists == 2 || h_dec[b].decision == SVS_KF_DROP); };
  bool any = false;
  for (int b0 = 0; b0 < B;) {
    if (!wanted(b0)) { ++b0; continue; }
    int b1 = b0, wn = 0, wt = 0;      // the run [b0, b1) and its longest lists
    for (; b1 < B && wanted(b1); ++b1) { wn = std::max(wn, (int)h_dec[b1].n_new); wt = std::max(wt, (int)h_dec[b1].n_track); }
    SVS_REQUIRE(ctx, wn <= cap && wt <= cap);
    const size_t rows = (size_t)(b1 - b0), o = (size_t)b0;
    if (wn) {
      SVS_HIP(ctx, hipMemcpy2DAsync(h_new + o * cap, sizeof(svs_map_new_point) * (size_t)cap, fe->d_kd_new + o * mp, sizeof(svs_map_new_point) * mp,
                                    sizeof(svs_map_new_point) * (size_t)wn, rows, hipMemcpyDeviceToHost, ctx->stream));
      SVS_HIP(ctx, hipMemcpy2DAsync(h_new_rec + o * cap, sizeof(int32_t) * (size_t)cap, fe->d_kd_new_rec + o * mp, sizeof(int32_t) * mp, sizeof(int32_t) * (size_t)wn, rows,
                                    hipMemcpyDeviceToHost, ctx->stream));
    }
    if (wt) {
      SVS_HIP(ctx, hipMemcpy2DAsync(h_track + o * cap, sizeof(svs_map_track_point) * (size_t)cap, fe->d_kd_track + o * mp, sizeof(svs_map_track_point) * mp,
                                    sizeof(svs_map_track_point) * (size_t)wt, rows, hipMemcpyDeviceToHost, ctx->stream));
      SVS_HIP(ctx, hipMemcpy2DAsync(h_track_rec + o * cap, sizeof(int32_t) * (size_t)cap, fe->d_kd_track_rec + o * mp, sizeof(int32_t) * mp, sizeof(int32_t) * (size_t)wt, rows,
                                    hipMemcpyDeviceToHost, ctx->stream));
    }
    any = any || wn || wt;
    b0 = b1;
  }
  if (any) SVS_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return SVS_OK;
}

/* applying a stream's SVS_KF_DROP decision (map.hip: map_addkf_dev.inc, through addkf_map.h; the contract is in the header): the lists stay where the decision left
   them, the kept slot gives the keyframe record, and the step's pose and the detector's thresholds come home on the map call's first download -- their copies are
   enqueued here, into a pinned block the map call reads behind that download.  The front end's state is only read. */
extern "C" int svs_frontend_commit_keyframe(svs_frontend *fe, svs_map *map, const svs_commit_keyframe_request *q, int missing_cap, svs_map_strength_result *h_res,
                                            svs_map_key *h_keys, int32_t *h_new_kept, int32_t *h_track_exists, svs_map_constraint_result *h_cons, int32_t *h_missing) {
  svs_ctx *ctx = fe ? fe->ctx : nullptr;
  SVS_REQUIRE(ctx, fe && map && q && fe->have_prev && !fe->submitted);
  SVS_REQUIRE(ctx, svs_map_ctx(map) == ctx);
  SVS_REQUIRE(ctx, q->stream >= 0 && q->stream < fe->B && q->slot >= 0 && q->slot < fe->max_keyframes);
  SVS_REQUIRE(ctx, fe->n_gated >= 0 && fe->kd_have && fe->kd_serial == fe->step_serial);      // a decision on the step and the list that are still on the device
  SVS_REQUIRE(ctx, !fe->pose_replaced);                            // ... and the step's refined pose with them: no svs_frontend_recompute_cloud since the step
  const svs_keyframe_decision &dec = fe->h_kd_dec[q->stream];
  SVS_REQUIRE(ctx, dec.valid && dec.decision == SVS_KF_DROP);
  const size_t idx = (size_t)q->stream * fe->max_keyframes + q->slot, mp = (size_t)fe->max_points;
  SVS_REQUIRE(ctx, fe->kept[idx]);
  SVS_REQUIRE(ctx, dec.n_new >= 0 && dec.n_track >= 0 && (size_t)dec.n_new <= mp && (size_t)dec.n_track <= mp);
  const FastThrView tv = svs_fast_thr_view_internal(fe->fast);
  for (int l = 0; l < tv.n_levels; ++l) SVS_REQUIRE(ctx, tv.ncell[l] <= SVS_MAX_CELLS);      // (before the first copy is enqueued)
  SVS_DEVICE(ctx);
  constexpr size_t thr_bytes = sizeof(int32_t) * SVS_NUM_PYR_LEVELS * SVS_MAX_CELLS, T_bytes = sizeof(double) * 12;
  if (!fe->h_ck) SVS_HIP(ctx, fe->h_ck.alloc(T_bytes + thr_bytes));
  double *h_T = reinterpret_cast<double *>(fe->h_ck.get());
  int32_t *h_thr = reinterpret_cast<int32_t *>(fe->h_ck + T_bytes);
  SVS_HIP(ctx, hipMemcpyAsync(h_T, fe->d_small + 12 * (size_t)q->stream, T_bytes, hipMemcpyDeviceToHost, ctx->stream));
  if (!q->h_fast_thr) {
    for (int k = 0; k < SVS_NUM_PYR_LEVELS * SVS_MAX_CELLS; ++k) h_thr[k] = 25;
    for (int l = 0; l < tv.n_levels; ++l) {
      SVS_HIP(ctx, hipMemcpyAsync(h_thr + (size_t)l * SVS_MAX_CELLS, tv.thr + (size_t)q->stream * tv.ncell_total + tv.cell_base[l], sizeof(int32_t) * (size_t)tv.ncell[l],
                                  hipMemcpyDeviceToHost, ctx->stream));
    }
  }
  svs_map_add_keyframe_args a{};
  a.newkey_id = q->newkey_id; a.oldkey_id = q->oldkey_id; a.covis_thr = q->covis_thr; a.half_width = q->half_width; a.half_height = q->half_height;
  a.disp_stride = q->disp_stride; a.n_new = dec.n_new; a.n_track = dec.n_track;
  a.keyframe = fe->h_kfs[idx];
  a.disp = q->disp; a.fast_thr = q->h_fast_thr;
  a.cached_ids = q->cached_ids; a.cached_T = q->cached_T; a.n_cached = q->n_cached;
  const MapKeyframeLists L{fe->d_kd_new + (size_t)q->stream * mp, fe->d_kd_track + (size_t)q->stream * mp, h_T, q->h_fast_thr ? nullptr : h_thr};
  const int rc = svs_map_add_keyframe_lists(map, &a, L, missing_cap, h_res, h_keys, h_new_kept, h_track_exists, h_cons, h_missing);
  if (rc) (void)hipStreamSynchronize(ctx->stream);                 // (a refusal in front of the download: the copies above have landed before the block is reused)
  return rc;
}

/* a stream's whole neighbourhood from a root id (map.hip: map_nbh.inc, through nbr_map.h; the contract is in the header): everything is checked on the host first, then one
   staged upload, the map's four launches writing d_pts / d_group_end / d_n_groups / d_n_new / d_kfs and the resident vertex tables in place, one download from
   which the host state follows */
// (from_store: svs_frontend_set_neighborhood_from_store -- the head is the stream's new-point store as it lies on the device: its group of act_id is the fixed
// group, every other group a keyed one; nothing of a head is staged)
static int fe_set_neighborhood(svs_frontend *fe, svs_map *map, int n_requests, const svs_nbr_request *req, int refresh_poses, int vertex_cap, svs_nbr_result *h_res,
                               int32_t *h_point_id, int32_t *h_vertex_id, double *h_vertex_T, int32_t *h_act_neighbors, int32_t *h_strength,
                               svs_candidate_point *h_records, svs_kf_table *h_table, svs_kf_vertex *h_vertex, double *h_slot_T, bool from_store) {
  svs_ctx *ctx = fe ? fe->ctx : nullptr;
  SVS_REQUIRE(ctx, !from_store || (fe && fe->np_rcap > 0));
  SVS_REQUIRE(ctx, fe && map && svs_map_ctx(map) == ctx && !fe->submitted && n_requests >= 0 && n_requests <= fe->B && (n_requests == 0 || req) && vertex_cap >= 1 &&
                       vertex_cap <= SVS_KF_MAX_VERTICES);
  if (fe->max_keyframes > SVS_KF_MAX_SLOTS) { ctx->err = "svs_frontend_set_neighborhood_from_root: more than SVS_KF_MAX_SLOTS keyframe slots"; return SVS_ERR_UNSUPPORTED; }
  const int R = n_requests, B = fe->B, K = fe->max_keyframes, MP = fe->max_points, VB = vertex_cap;
  size_t n_head = 0;
  {
    std::vector<uint8_t> named((size_t)B, 0);
    std::vector<int32_t> sorted;
    for (int r = 0; r < R; ++r) {
      const svs_nbr_request &q = req[r];
      SVS_REQUIRE(ctx, q.stream >= 0 && q.stream < B && !named[q.stream]);
      named[q.stream] = 1;
      SVS_REQUIRE(ctx, svs_map_has_keyframe(map, q.root_id) && svs_map_has_keyframe(map, q.act_id) && q.max_num_neighbors >= 0);
      if (from_store) {      // the four head fields are the store's to fill; the written list holds at most the store's groups, act's (also when absent) and the map's
        SVS_REQUIRE(ctx, q.h_slot_kf && q.n_head == 0 && q.n_head_groups == 0 && q.n_fixed_groups == 0 && !q.h_head_group_end && !q.h_head && !q.h_head_group_kf);
        bool have_act = false;
        for (int g = 0; g < fe->np_ng[q.stream]; ++g) have_act = have_act || fe->np_key[(size_t)q.stream * MAX_GROUPS + g] == q.act_id;
        if (fe->np_ng[q.stream] + (have_act ? 0 : 1) + 1 > MAX_GROUPS) { ctx->err = "svs_frontend_set_neighborhood_from_store: more than 64 groups"; return SVS_ERR_CAPACITY; }
        if (int rc = fe_check_slot_table(fe, q.stream, q.h_slot_kf, sorted)) return rc;
        continue;
      }
      SVS_REQUIRE(ctx, q.h_slot_kf && q.n_head >= 0 && q.n_head <= MP && (q.n_head == 0 || q.h_head) && q.n_head_groups >= 1 && q.h_head_group_end);
      if (q.n_head_groups + 1 > MAX_GROUPS) { ctx->err = "svs_frontend_set_neighborhood_from_root: more than 64 groups"; return SVS_ERR_CAPACITY; }
      SVS_REQUIRE(ctx, q.n_fixed_groups >= 1 && q.n_fixed_groups <= q.n_head_groups && (q.n_fixed_groups == q.n_head_groups || q.h_head_group_kf));
      if (int rc = fe_check_slot_table(fe, q.stream, q.h_slot_kf, sorted)) return rc;
      if (int rc = fe_check_group_ends(ctx, q.h_head_group_end, q.n_head_groups, q.n_head)) return rc;
      if (int rc = fe_check_anchors(fe, q.stream, q.h_head, q.n_head)) return rc;
      sorted.clear();
      for (int g = q.n_fixed_groups; g < q.n_head_groups; ++g) { SVS_REQUIRE(ctx, svs_map_has_keyframe(map, q.h_head_group_kf[g])); sorted.push_back(q.h_head_group_kf[g]); }
      SVS_REQUIRE(ctx, all_distinct(sorted));
      n_head += (size_t)q.n_head;
    }
  }
  if (R == 0) return SVS_OK;
  SVS_DEVICE(ctx);
  if (int rc = fe_vt_reserve(fe)) return rc;
  // the block: what goes up (requests | slot ids | heads), what comes back with the optional outputs last, and behind it the walk's work space, never copied
  Pieces<> row;
  const size_t Rz = (size_t)R;
  const auto p_req = row.piece<nbr_req>(Rz); const auto p_ids = row.piece<int32_t>(Rz * 2 * K); const auto p_head = row.piece<svs_candidate_point>(n_head);
  const size_t in_end = row.end;
  const auto p_res = row.piece<svs_nbr_result>(Rz); const auto p_slot = row.piece<double>(Rz * K * 12); const auto p_vT = row.piece<double>(Rz * VB * 12);
  const auto p_vid = row.piece<int32_t>(Rz * VB); const auto p_act = row.piece<int32_t>(Rz * VB); const auto p_str = row.piece<int32_t>(Rz * VB * VB);
  const auto p_pid = row.piece<int32_t>(Rz * MP);
  const auto p_hdr = row.piece<int4>(Rz * VB); const auto p_mid = row.piece<nbr_mid>(Rz); const auto p_list = row.piece<int2>(Rz * VB);
  const auto p_mpid = row.piece<int32_t>(Rz * MP); const auto p_wv = row.piece<int32_t>(Rz * VB); const auto p_woff = row.piece<int32_t>(Rz + 1);
  TwinBlock &blk = fe->nbh;
  if (int rc = blk.reserve(ctx, row.end)) return rc;      // (no call is in flight: this one is blocking)
  nbr_req *hq = blk.host(p_req);
  int32_t *ids = blk.host(p_ids);
  svs_candidate_point *head = blk.host(p_head);
  size_t at_head = 0;
  for (int r = 0; r < R; ++r) {
    const svs_nbr_request &q = req[r];
    nbr_req &s = hq[r];
    memset(&s, 0, sizeof s);
    s.stream = q.stream; s.root = q.root_id; s.act = q.act_id; s.max_nn = q.max_num_neighbors;
    s.n_head = q.n_head; s.n_groups = q.n_head_groups; s.n_fixed = q.n_fixed_groups; s.prev_len = fe->n_points[q.stream];
    s.slot_off = (int32_t)((size_t)r * 2 * K); s.slot_raw_off = s.slot_off + K;
    for (int k = 0; k < K; ++k) { ids[s.slot_off + k] = svs_map_has_keyframe(map, q.h_slot_kf[k]) ? q.h_slot_kf[k] : -1; ids[s.slot_raw_off + k] = q.h_slot_kf[k]; }
    if (from_store) {      // the stream's groups in store order; act's group is the fixed one -- an empty group behind the others when the store has none
      const int32_t *key = &fe->np_key[(size_t)q.stream * MAX_GROUPS], *cnt = &fe->np_cnt[(size_t)q.stream * MAX_GROUPS];
      int G = fe->np_ng[q.stream], at = 0, f = -1;
      for (int g = 0; g < G; ++g) { at += cnt[g]; s.group_end[g] = at; s.group_kf[g] = key[g]; if (key[g] == q.act_id) f = g; }
      if (f < 0) { f = G; s.group_end[G] = at; s.group_kf[G] = q.act_id; ++G; }
      s.n_head = at; s.n_groups = G; s.n_fixed = 1; s.fixed_at = 1 + f;
      continue;
    }
    s.head_off = (int32_t)at_head;
    if (q.n_head) memcpy(head + at_head, q.h_head, (size_t)q.n_head * sizeof(svs_candidate_point));
    at_head += (size_t)q.n_head;
    for (int g = 0; g < q.n_head_groups; ++g) { s.group_end[g] = q.h_head_group_end[g]; s.group_kf[g] = g >= q.n_fixed_groups ? q.h_head_group_kf[g] : -1; }
  }
  if (int rc = blk.upload(ctx, 0, in_end)) return rc;
  MapNbrDst D{};
  D.req = blk.dev(p_req); D.ids = blk.dev(p_ids); D.head = blk.dev(p_head);
  if (from_store) { D.head = fe->d_np_rec; D.head_stride = fe->np_rcap; D.from_store = 1; }
  D.R = R; D.VB = VB;
  D.pts = fe->d_pts; D.max_points = MP; D.group_end = fe->d_group_end; D.n_groups = fe->d_n_groups; D.n_new = fe->d_n_new; D.kfs = fe->d_kfs; D.max_keyframes = K;
  D.vt_tab = fe->d_vt_tab; D.vt_vtx = fe->d_vt_vtx; D.vt_slot = fe->d_vt_slot;
  D.refresh = refresh_poses ? 1 : 0;
  D.res = blk.dev(p_res); D.slot_T = blk.dev(p_slot); D.vertex_T = blk.dev(p_vT); D.vertex_id = blk.dev(p_vid); D.act_nb = blk.dev(p_act); D.strength = blk.dev(p_str);
  D.point_id = blk.dev(p_pid);
  D.walk_hdr = blk.dev(p_hdr); D.mid = blk.dev(p_mid); D.walk_list = blk.dev(p_list); D.map_pid = blk.dev(p_mpid); D.walk_v = blk.dev(p_wv); D.walk_off = blk.dev(p_woff);
  if (int rc = svs_map_build_root_neighborhoods(map, D)) return rc;
  // from the first output piece to the end of the last one a caller asked for
  const size_t down_to = h_point_id ? p_pid.end() : h_strength ? p_str.end() : h_act_neighbors ? p_act.end() : h_vertex_id ? p_vid.end() : h_vertex_T ? p_vT.end() : p_slot.end();
  if (int rc = blk.download(ctx, p_res.off, down_to)) return rc;
  if (h_records) SVS_HIP(ctx, hipMemcpyAsync(h_records, fe->d_pts, sizeof(svs_candidate_point) * (size_t)MP * B, hipMemcpyDeviceToHost, ctx->stream));
  for (int r = 0; r < R && (h_table || h_vertex); ++r) {
    const size_t b = (size_t)req[r].stream;
    if (h_table) SVS_HIP(ctx, hipMemcpyAsync(h_table + r, fe->d_vt_tab + b, sizeof(svs_kf_table), hipMemcpyDeviceToHost, ctx->stream));
    if (h_vertex)
      SVS_HIP(ctx, hipMemcpyAsync(h_vertex + (size_t)r * SVS_KF_MAX_VERTICES, fe->d_vt_vtx + b * SVS_KF_MAX_VERTICES, sizeof(svs_kf_vertex) * SVS_KF_MAX_VERTICES,
                                  hipMemcpyDeviceToHost, ctx->stream));
  }
  SVS_HIP(ctx, hipStreamSynchronize(ctx->stream));
  // ---- the host state follows the download
  const svs_nbr_result *res = blk.host(p_res);
  bool any = false;
  for (int r = 0; r < R; ++r) {
    const svs_nbr_request &q = req[r];
    const bool none = res[r].over_capacity != 0 || res[r].root_outside_window != 0;
    if (h_res) h_res[r] = res[r];
    fe_row_out(h_point_id, blk.host(p_pid), r, (size_t)MP, none);
    fe_row_out(h_vertex_id, blk.host(p_vid), r, (size_t)VB, none);
    fe_row_out(h_act_neighbors, blk.host(p_act), r, (size_t)VB, none);
    fe_row_out(h_strength, blk.host(p_str), r, (size_t)VB * VB, none);
    fe_row_out(h_vertex_T, blk.host(p_vT), r, (size_t)VB * 12, none);
    fe_row_out(h_slot_T, blk.host(p_slot), r, (size_t)K * 12, none);
    if (none) continue;
    any = true;
    fe->n_points[q.stream] = res[r].n_points; fe->n_new_records[q.stream] = res[r].n_head_kept;
    fe->max_groups_used = std::max(fe->max_groups_used, (int)res[r].n_groups);
    fe->vt_set[q.stream] = 1;
    if (refresh_poses) fe_refresh_poses(fe, map, q.stream, q.h_slot_kf, blk.host(p_slot) + (size_t)r * K * 12);
  }
  if (any) fe_lists_changed(fe);
  return SVS_OK;
}

extern "C" int svs_frontend_set_neighborhood_from_root(svs_frontend *fe, svs_map *map, int n_requests, const svs_nbr_request *req, int refresh_poses, int vertex_cap,
                                                       svs_nbr_result *h_res, int32_t *h_point_id, int32_t *h_vertex_id, double *h_vertex_T, int32_t *h_act_neighbors,
                                                       int32_t *h_strength, svs_candidate_point *h_records, svs_kf_table *h_table, svs_kf_vertex *h_vertex,
                                                       double *h_slot_T) {
  return fe_set_neighborhood(fe, map, n_requests, req, refresh_poses, vertex_cap, h_res, h_point_id, h_vertex_id, h_vertex_T, h_act_neighbors, h_strength, h_records,
                             h_table, h_vertex, h_slot_T, false);
}

extern "C" int svs_frontend_set_neighborhood_from_store(svs_frontend *fe, svs_map *map, int n_requests, const svs_nbr_request *req, int refresh_poses, int vertex_cap,
                                                        svs_nbr_result *h_res, int32_t *h_point_id, int32_t *h_vertex_id, double *h_vertex_T, int32_t *h_act_neighbors,
                                                        int32_t *h_strength, svs_candidate_point *h_records, svs_kf_table *h_table, svs_kf_vertex *h_vertex,
                                                        double *h_slot_T) {
  return fe_set_neighborhood(fe, map, n_requests, req, refresh_poses, vertex_cap, h_res, h_point_id, h_vertex_id, h_vertex_T, h_act_neighbors, h_strength, h_records,
                             h_table, h_vertex, h_slot_T, true);
}

#include "frontend_newpoints.inc"
