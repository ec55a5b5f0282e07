// match.hip -- guided 8x8 zero-mean-SSD matcher for gfx950.
// Replaces GuidedMatcher<StereoCamera>::match (matcher.cpp:312-398) incl. computePrediction
// (:98-142), warpAffinve (:403-458), computePatchScores/matchPatchZeroMeanSSD (:42-96),
// matchCandidates (:144-181), returnBestMatch (:183-214), createObervation
// (matcher-impl.cpp:33-51).
//
// One translation unit, cut by stage; each part lists its kernels:
//   match_predict.inc   match_pose_kernel (relative poses per (stream, keyframe), the level table), match_predict_kernel<FUSE> (ONE LANE per candidate point:
//                       computePrediction and the local affine of warpAffinve -- the scalar f64 part, 10 exact divisions, is evaluated once per point;
//                       <true> forms the poses itself)
//   match_order.inc     match_order_kernel: a stream's points in image order for match_kernel3 (counting sort by cell of the predicted position)
//   match_wave.inc      ONE WAVEFRONT per point, the steps written once: match_kernel (any grid and radius; option "match_legacy" 1) and match_kernel2 (the lean
//                       scan, windows narrower than a cell; windows wider than 17, and "match_legacy" 2); the readers of the corner bitmap
//   match_group.inc     match_kernel3: FOUR points per wave, 16 lanes each (windows up to 17 x 17, narrower than a cell): the default
//   match_subpix.inc    the optional sub-pixel refinement of the OK records (svs_match_subpixel; subpixelAccuracy, matcher.cpp:241-309): ONE WAVEFRONT per record
// In all three matchers the quadtree of the reference is replaced by a scan of the (2R+1)^2 search window in the corner bitmap of fast.hip (a pixel is a
// candidate iff its score clears the emit threshold of its cell); the winner is the minimum ZNSSD, and the reference's tie-break (first hit in QuadTree::query
// DFS order, strict '<') is reproduced with quadrant keys computed only on ties -- bit-exact without building a tree.
// This file keeps the records the stages hand to each other, the constants the host shares with the kernels, and the C API (svs_match: which kernels run).
// f64 geometry is compiled with -ffp-contract=off so it rounds like the host oracle.
#include "common.h"

#include "fast_view.h"
#include "pose.h"
#include "subpix_core.h"
#include <algorithm>

namespace {

// per-point result of computePrediction + the local affine of warpAffinve (everything that is one scalar evaluation per
// point): produced one LANE per point by match_predict_kernel, consumed one WAVE per point by match_kernel / match_kernel2, 16 lanes per point by match_kernel3
struct alignas(16) PointPred {      // 128 bytes = one cache line, fields grouped into 16-byte reads (match_kernel3 stages it in the LDS, 8 bytes per lane)
  int32_t status, ui, vi, lvl;
  double inv[4];          // inverse of the local affine A (matcher.cpp:415-426)
  double key_uv[2];       // anchor_obs_pyr
  // for match_kernel2/3: the keyframe's level image (saves the dependent read of the keyframe record) and where the search window's rows start in the corner
  // bitmap of fast.hip: the padded bit position of the window's first in-image column and the one cell-column boundary the window may cross
  const uint8_t *kimg;
  int32_t kstride, xb;
  int32_t yb;
  int32_t pb_lo;          // max(ui - R, 0) + gap * (cell column of it)
  int32_t kfi, pad_;
  double xyz_actkey[3];
  double pad2_;
};
static_assert(sizeof(PointPred) == 128, "PointPred layout");
// what match_kernel3 needs of a pyramid level, as a table in memory: its 16-lane groups work on points of different levels, so the level index is a vector
// register there and the per-level kernel arguments cannot be picked with scalar indexing (written by match_pose_kernel; staged in the LDS as M3Level)
struct LevelTab {
  const uint8_t *bm, *cimg;
  size_t bm_bstride, cur_bstride;
  int32_t bm_stride, cstride, w, h, xhi, yhi, gap, pad_;
};
struct MatchParams {
  svs_match_args a;
  FastView fv;
  const double *kf_T;     // [n_batch][n_kf][24]: T_cur_from_anchor, T_actkey_from_anchor (match_pose_kernel)
  PointPred *pred;        // [n_batch][n_pts]
  const int32_t *order;   // [n_batch][n_pts] or NULL: the order in which match_kernel3 takes the points of a stream (match_order_kernel)
  int32_t *keys;          // [n_batch][n_pts] or NULL: the bucket of every point (written by match_predict_kernel, read by match_order_kernel)
  int32_t ord_sx, ord_sy, ord_nbx, ord_nb;      // its buckets: level * ord_nb + (vi >> ord_sy) * ord_nbx + (ui >> ord_sx); bucket 3 * ord_nb = points that are not searched
  LevelTab *lt;           // [SVS_NUM_PYR_LEVELS]
  // optional (the one-call front end, few keyframes): the tracked pose and the active keyframe's pose per stream -- match_predict_kernel<true> then forms the two poses of
  // matcher.cpp:326-330 and the per-keyframe relative poses itself (what frontend_pose_kernel + match_pose_kernel did in two launches of their own between tracker and matcher)
  const double *src_T, *src_Ta;
  int swz;                // match_kernel3 takes its blocks in XCD-contiguous order (devutil.h: xcd_contiguous)
  int32_t k3_kmax[SVS_NUM_PYR_LEVELS];      // match_kernel3: the widest keyframe row stride of a level whose byte offsets it forms in 32 bits (k3_row_stride_max)
};

constexpr int PRED_FUSE_MAX_KF = 8;                // match_predict_kernel<true>: keyframes per stream whose poses a block forms in LDS
constexpr int ORD_MAX_BUCKETS = 6144;              // match_order_kernel: buckets its LDS counts hold
constexpr int WAVES_PER_BLOCK = 4;                 // match_kernel, match_kernel2: points per 256-lane block
constexpr int M3_GROUPS = 16;                      // match_kernel3: points per 256-lane block

#include "match_predict.inc"
#include "match_order.inc"
#include "match_wave.inc"
#include "match_group.inc"
#include "match_subpix.inc"

}  // namespace

extern "C" int svs_match(svs_ctx *ctx, const svs_match_args *a, svs_fast *f, svs_match_result *d_out) {
  SVS_REQUIRE(ctx, ctx && a && f);
  SVS_DEVICE(ctx);
  SVS_REQUIRE(ctx, a->n_pts >= 0 && a->n_batch >= 1 && a->search_radius >= 0 && a->search_radius <= 31);
  if (a->n_pts == 0) return SVS_OK;                 // empty ap_map: nothing to append (matcher.cpp:332)
  SVS_REQUIRE(ctx, d_out && a->d_pts && a->d_kfs);
  MatchParams M;
  M.a = *a;
  if (!M.a.pts_bstride) M.a.pts_bstride = (size_t)a->n_pts;
  if (!M.a.out_bstride) M.a.out_bstride = (size_t)a->n_pts;
  SVS_REQUIRE(ctx, M.a.pts_bstride >= (size_t)a->n_pts && M.a.out_bstride >= (size_t)a->n_pts);
  M.fv = svs_fast_view_internal(f);
  SVS_REQUIRE(ctx, M.fv.n_levels >= 1 && a->n_kf >= 1);
  // (option "match_legacy": 0 = the fastest kernel that applies, 1 = match_kernel, 2 = match_kernel2 where it applies)
  bool lean = ctx->match_legacy != 1;
  for (int l = 0; l < M.fv.n_levels; ++l) lean = lean && 2 * a->search_radius + 1 <= std::min(M.fv.cell_w[l], M.fv.cell_h[l]);
  const bool k3 = lean && ctx->match_legacy == 0 && 2 * a->search_radius + 1 <= 17;
  // match_kernel3 forms its offsets with 24-bit multiplies (k3_offsets_fit), as the tracker does (dense.hip, offsets_fit_24).  Refused whichever kernel the call
  // would take (a radius, a grid or an option must not decide whether a frame is accepted), and before anything is allocated or launched
  SVS_REQUIRE(ctx, a->n_pts < (1 << 24));
  for (int l = 0; l < M.fv.n_levels; ++l) {
    SVS_REQUIRE(ctx, a->cam_vec[l].w > 0 && a->cam_vec[l].w < (1 << 24));
    SVS_REQUIRE(ctx, k3_offsets_fit(a->cam_vec[l].h, a->cur_stride[l], 1) && k3_offsets_fit(a->cam_vec[l].h, M.fv.bm_stride[l], 1));
  }
  SVS_REQUIRE(ctx, k3_offsets_fit(a->cam_vec[0].h, a->disp_stride, sizeof(float)));
  for (int l = 0; l < SVS_NUM_PYR_LEVELS; ++l) M.k3_kmax[l] = k3_row_stride_max(a->cam_vec[l].h);
  // the per-call tables live in the context (one buffer: relative poses per (stream, keyframe), then the predictions per point)
  const size_t kf_bytes = (((size_t)a->n_batch * a->n_kf * 24 * sizeof(double)) + 255) & ~(size_t)255;
  const size_t pred_bytes = (size_t)a->n_batch * a->n_pts * sizeof(PointPred);
  const size_t lt_bytes = 256;
  static_assert(sizeof(LevelTab) * SVS_NUM_PYR_LEVELS <= 256, "level table");
  const size_t ord_bytes = (((size_t)a->n_batch * a->n_pts * sizeof(int32_t)) + 255) & ~(size_t)255;
  void *buf = nullptr;
  { const int rc = svs_ctx_match_scratch(ctx, lt_bytes + kf_bytes + 2 * ord_bytes + pred_bytes, &buf); if (rc) return rc; }
  M.lt = static_cast<LevelTab *>(buf);
  double *kf_T = reinterpret_cast<double *>(static_cast<char *>(buf) + lt_bytes);
  M.kf_T = kf_T;
  int32_t *order = reinterpret_cast<int32_t *>(static_cast<char *>(buf) + lt_bytes + kf_bytes);
  M.pred = reinterpret_cast<PointPred *>(static_cast<char *>(buf) + lt_bytes + kf_bytes + 2 * ord_bytes);
  M.order = nullptr; M.keys = nullptr;
  const bool ordered = k3 && ctx->match_order && a->n_pts >= 64 && (size_t)a->n_batch * a->n_pts >= 32768;      // a batch: one more launch (~10 us) is not worth it for a stream or two
  if (ordered) {      // cells of 16 x 16 pixels of level 0 (coarser for frames that would need more than ORD_MAX_BUCKETS buckets)
    int sx = 4, sy = 4;      // (16 x 16 ... 64 x 32 pixel cells measure the same within 2 %: 0.69 - 0.71 ms)
    auto nb = [&]() { return ((M.fv.w[0] + (1 << sx) - 1) >> sx) * ((M.fv.h[0] + (1 << sy) - 1) >> sy); };
    while (3 * nb() + 1 > ORD_MAX_BUCKETS) { if (sx <= sy + 1) ++sx; else ++sy; }
    M.ord_sx = sx; M.ord_sy = sy; M.ord_nbx = (M.fv.w[0] + (1 << sx) - 1) >> sx; M.ord_nb = nb();
    M.keys = order + ord_bytes / sizeof(int32_t);
  }
  M.src_T = ctx->match_src_T; M.src_Ta = ctx->match_src_Ta;
  M.swz = ctx->xcd_swizzle;
  if (M.src_T && M.src_Ta && a->n_kf <= PRED_FUSE_MAX_KF) {      // one launch instead of three (frontend_pose_kernel, match_pose_kernel, match_predict_kernel): the one-call front end
    hipLaunchKernelGGL(match_predict_kernel<true>, dim3(div_up(a->n_pts, 64), a->n_batch), dim3(64), 0, ctx->stream, M);
    SVS_LAUNCH_CHECK(ctx);
  } else {
    SVS_REQUIRE(ctx, a->d_T_cur_from_w && a->d_T_w_from_actkey);
    hipLaunchKernelGGL(match_pose_kernel, dim3(div_up(a->n_kf, 64), a->n_batch), dim3(64), 0, ctx->stream, M, kf_T);
    SVS_LAUNCH_CHECK(ctx);
    hipLaunchKernelGGL(match_predict_kernel<false>, dim3(div_up(a->n_pts, 64), a->n_batch), dim3(64), 0, ctx->stream, M);
    SVS_LAUNCH_CHECK(ctx);
  }
  dim3 grid(div_up(a->n_pts, WAVES_PER_BLOCK), a->n_batch), block(64 * WAVES_PER_BLOCK);
  // the lean scan resolves a window's cells once per point: it needs windows narrower than a cell (always so for the reference's grids and radii)
  if (k3) {
    if (ordered) {
      hipLaunchKernelGGL(match_order_kernel, dim3(a->n_batch), dim3(256), 0, ctx->stream, M, order);
      SVS_LAUNCH_CHECK(ctx);
      M.order = order;
    }
    hipLaunchKernelGGL(match_kernel3, dim3(div_up(a->n_pts, M3_GROUPS), a->n_batch), dim3(256), 0, ctx->stream, M, d_out);
  }
  else if (lean) hipLaunchKernelGGL(match_kernel2, grid, block, 0, ctx->stream, M, d_out);
  else hipLaunchKernelGGL(match_kernel, grid, block, 0, ctx->stream, M, d_out);
  SVS_LAUNCH_CHECK(ctx);
  ctx->match_pred = M.pred; ctx->match_pred_batch = a->n_batch; ctx->match_pred_pts = a->n_pts;      // for the front end's sub-pixel pass (svs_match_subpixel_behind_match)
  return SVS_OK;
}

extern "C" void svs_subpix_params_default(svs_subpix_params *p) {
  if (!p) return;
  p->iterations = 8; p->max_shift = 1.5f; p->eps = 0.03f; p->pad_ = 0;
}
// what both entries refuse, before any allocation or launch; *empty: nothing to do
static int subpix_check(svs_ctx *ctx, const svs_match_args *a, const svs_subpix_params *prm, const svs_match_result *d_results, bool *empty) {
  SVS_REQUIRE(ctx, ctx && a && prm);
  SVS_REQUIRE(ctx, svs_subpix_params_ok(prm));
  SVS_REQUIRE(ctx, a->n_pts >= 0 && a->n_batch >= 1);
  *empty = a->n_pts == 0;
  SVS_REQUIRE(ctx, *empty || d_results);
  return SVS_OK;
}
extern "C" int svs_match_subpixel(svs_ctx *ctx, const svs_match_args *a, const svs_subpix_params *prm, svs_match_result *d_results, svs_subpix_info *d_info) {
  bool empty;
  if (const int rc = subpix_check(ctx, a, prm, d_results, &empty)) return rc;
  SVS_DEVICE(ctx);
  return empty ? SVS_OK : subpix_run(ctx, a, prm, nullptr, d_results, d_info);
}
// internal (the front end): the same pass right behind svs_match(ctx, a, ...) on the same context, reading the prediction records that call left in the scratch
int svs_match_subpixel_behind_match(svs_ctx *ctx, const svs_match_args *a, const svs_subpix_params *prm, svs_match_result *d_results, svs_subpix_info *d_info) {
  bool empty;
  if (const int rc = subpix_check(ctx, a, prm, d_results, &empty)) return rc;
  if (empty) return SVS_OK;
  SVS_REQUIRE(ctx, ctx->match_pred && ctx->match_pred_batch == a->n_batch && ctx->match_pred_pts == a->n_pts);
  return subpix_run(ctx, a, prm, static_cast<PointPred *>(ctx->match_pred), d_results, d_info);
}
