// scavislam_hip.hpp -- C++ adaptor classes over the C ABI (scavislam_hip.h) that keep the
// reference's call surfaces (method names, argument meaning, blocking semantics, bool/void
// returns, no exceptions across the boundary -- README:295 house style), so that they can replace
// the reference classes inside stereo_slam where OpenCV/Eigen/Sophus exist.  This header itself
// depends on nothing but the C ABI and the STL: images are (pointer, w, h, stride) views, poses
// are 3x4 row-major double[12].  INTEGRATION.md shows the 10-line glue from cv::Mat / Sophus::SE3.
//
//   FastGrid        <- scavislam/fast_grid.h:27-63
//   GuidedMatcher   <- scavislam/matcher.hpp:62-186
//   DenseTracker    <- scavislam/dense_tracking.h:53-97  (CPU-path semantics, the parity target)
//   GpuTracker / DenseTrackerGpu <- gpu/dense_tracking.cuh:281-342, DenseTracker::denseTrackingGpu (dense_tracking.cpp:60-215)
//   StereoFrontend  <- StereoFrontend::processFrame / processFirstFrame, scavislam/stereo_frontend.h:88-95 (one call per frame)
//   SlamGraphBA     <- SlamGraph::optimize, scavislam/slam_graph.hpp:457-462
//   FrameRectifier  <- FrameGrabber<StereoCamera>::intializeRectifier / rectifyFrame / depthToDisp, scavislam/frame_grabber.cpp:245-256, frame_grabber-impl.cpp:93-152
//   BackendRegistration <- Backend::localRegisterFrame / globalLoopClosure, scavislam/backend.cpp:549-611, 830-1001 (one call per registration)
//   Communicator    <- (no reference counterpart) landmark-sharded optimize over RCCL, SURVEY.md 8e
//
// One svs_ctx per calling thread (front-end on main, re-registration matcher/FAST + optimize on
// the backend thread, backend.cpp:452-469,738,763): no static scratch like matcher.cpp:36-38.
#ifndef SCAVISLAM_HIP_HPP
#define SCAVISLAM_HIP_HPP

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <algorithm>
#include <cstring>
#include <utility>
#include <vector>

#include "scavislam_hip.h"

namespace scavislam_hip {

struct Image8 { const uint8_t *data; int w, h, stride; };
struct ImageF { const float *data; int w, h, stride; };
struct Corner { int16_t x, y; };

class Context {
 public:
  explicit Context(int device = 0, void *hip_stream = nullptr) : ctx_(nullptr) { ok_ = svs_ctx_create(device, hip_stream, &ctx_) == SVS_OK; }
  ~Context() { if (ctx_) svs_ctx_destroy(ctx_); }
  Context(const Context &) = delete;
  Context &operator=(const Context &) = delete;
  bool ok() const { return ok_; }
  svs_ctx *get() const { return ctx_; }
  const char *error() const { return svs_last_error(ctx_); }
  bool check(int rc) const { if (rc != SVS_OK) std::fprintf(stderr, "scavislam_hip: status %d: %s\n", rc, error()); return rc == SVS_OK; }

 private:
  svs_ctx *ctx_;
  bool ok_;
};

// RAII device buffer
template <class T>
class DeviceBuffer {
 public:
  DeviceBuffer() : ctx_(nullptr), p_(nullptr), n_(0) {}
  DeviceBuffer(const Context &c, size_t n) : ctx_(c.get()), p_(nullptr), n_(n) { void *p = nullptr; if (svs_malloc(ctx_, n * sizeof(T), &p) == SVS_OK) p_ = (T *)p; }
  ~DeviceBuffer() { if (p_) svs_free(ctx_, p_); }
  DeviceBuffer(DeviceBuffer &&o) noexcept : ctx_(o.ctx_), p_(o.p_), n_(o.n_) { o.p_ = nullptr; }
  DeviceBuffer &operator=(DeviceBuffer &&o) noexcept { if (this != &o) { if (p_) svs_free(ctx_, p_); ctx_ = o.ctx_; p_ = o.p_; n_ = o.n_; o.p_ = nullptr; } return *this; }
  DeviceBuffer(const DeviceBuffer &) = delete;
  DeviceBuffer &operator=(const DeviceBuffer &) = delete;
  T *get() const { return p_; }
  size_t size() const { return n_; }
  bool upload(const T *h, size_t n) { return svs_memcpy_h2d(ctx_, p_, h, n * sizeof(T)) == SVS_OK; }
  bool download(T *h, size_t n) const { return svs_memcpy_d2h(ctx_, h, p_, n * sizeof(T)) == SVS_OK; }

 private:
  svs_ctx *ctx_;
  T *p_;
  size_t n_;
};

// Device-resident u8 pyramid of one frame (Frame::pyr, keyframes.h:85) + disparity (Frame::disp)
class FrameDev {
 public:
  FrameDev(const Context &c, int w, int h) : ctx_(c) {
    for (int l = 0; l < SVS_NUM_PYR_LEVELS; ++l) {
      w_[l] = w >> l; h_[l] = h >> l; stride_[l] = (w_[l] + 63) / 64 * 64;
      pyr_[l] = DeviceBuffer<uint8_t>(c, (size_t)stride_[l] * h_[l]);
    }
    disp_ = DeviceBuffer<float>(c, (size_t)stride_[0] * h_[0]);
    for (int l = 0; l < SVS_NUM_PYR_LEVELS; ++l) {     // pyr_float32 / _dx / _dy of the CPU path (frame_grabber.cpp:315-333)
      f32_[l] = DeviceBuffer<float>(c, (size_t)stride_[l] * h_[l]);
      dx_[l] = DeviceBuffer<float>(c, (size_t)stride_[l] * h_[l]);
      dy_[l] = DeviceBuffer<float>(c, (size_t)stride_[l] * h_[l]);
    }
  }
  // FrameGrabber::preprocessing (frame_grabber.cpp:285-336): upload level 0, build the pyramid
  bool preprocessing(const Image8 &left) {
    std::vector<uint8_t> tmp((size_t)stride_[0] * h_[0]);
    for (int y = 0; y < h_[0]; ++y) std::memcpy(&tmp[(size_t)y * stride_[0]], left.data + (size_t)y * left.stride, (size_t)w_[0]);
    if (!pyr_[0].upload(tmp.data(), tmp.size())) return false;
    for (int l = 1; l < SVS_NUM_PYR_LEVELS; ++l)
      if (!ctx_.check(svs_pyr_down_u8(ctx_.get(), pyr_[l - 1].get(), w_[l - 1], h_[l - 1], stride_[l - 1], 0, pyr_[l].get(), stride_[l], 0, 1))) return false;
    for (int l = 0; l < SVS_NUM_PYR_LEVELS; ++l)
      if (!ctx_.check(svs_convert_sobel_f32(ctx_.get(), pyr_[l].get(), w_[l], h_[l], stride_[l], 0, f32_[l].get(), dx_[l].get(), dy_[l].get(), stride_[l], 0, 1))) return false;
    return true;
  }
  bool setDisparity(const ImageF &d) {
    std::vector<float> tmp((size_t)stride_[0] * h_[0]);
    for (int y = 0; y < h_[0]; ++y) std::memcpy(&tmp[(size_t)y * stride_[0]], d.data + (size_t)y * d.stride, sizeof(float) * (size_t)w_[0]);
    return disp_.upload(tmp.data(), tmp.size());
  }
  bool getDisparity(std::vector<float> *d) const {      // row-major w x h, stride removed
    std::vector<float> tmp((size_t)stride_[0] * h_[0]);
    if (!disp_.download(tmp.data(), tmp.size())) return false;
    d->resize((size_t)w_[0] * h_[0]);
    for (int y = 0; y < h_[0]; ++y) std::memcpy(&(*d)[(size_t)y * w_[0]], &tmp[(size_t)y * stride_[0]], sizeof(float) * (size_t)w_[0]);
    return true;
  }
  const uint8_t *pyr(int l) const { return pyr_[l].get(); }
  const float *disp() const { return disp_.get(); }
  const float *f32(int l) const { return f32_[l].get(); }
  const float *dx(int l) const { return dx_[l].get(); }
  const float *dy(int l) const { return dy_[l].get(); }
  int w(int l) const { return w_[l]; }
  int h(int l) const { return h_[l]; }
  int stride(int l) const { return stride_[l]; }

 private:
  const Context &ctx_;
  DeviceBuffer<uint8_t> pyr_[SVS_NUM_PYR_LEVELS];
  DeviceBuffer<float> disp_;
  DeviceBuffer<float> f32_[SVS_NUM_PYR_LEVELS], dx_[SVS_NUM_PYR_LEVELS], dy_[SVS_NUM_PYR_LEVELS];
  int w_[SVS_NUM_PYR_LEVELS], h_[SVS_NUM_PYR_LEVELS], stride_[SVS_NUM_PYR_LEVELS];
};

// FastGrid constructor arithmetic (fast_grid.cpp:23-58) -- integer bookkeeping only
inline svs_fastgrid makeFastGrid(int img_w, int img_h, int num_features_per_cell, int boundary_per_cell, int fast_thr,
                                 int grid_w, int grid_h, int fast_min = 10, int fast_max = 40) {
  svs_fastgrid g;
  g.gx = grid_w; g.gy = grid_h;
  g.min_inner = (int)(num_features_per_cell - boundary_per_cell * 0.33);
  g.min_outer = num_features_per_cell - boundary_per_cell;
  g.max_inner = (int)(num_features_per_cell + boundary_per_cell * 0.33);
  g.max_outer = num_features_per_cell + boundary_per_cell;
  g.cell_w = img_w / grid_w; g.cell_h = img_h / grid_h;
  g.fast_min = fast_min; g.fast_max = fast_max;
  for (int i = 0; i < SVS_MAX_CELLS; ++i) g.thr[i] = fast_thr;
  return g;
}

// All per-level FastGrids of StereoFrontend::fast_grid_ (stereo_frontend.cpp:73-88) in one object.
class FastGrid {
 public:
  FastGrid(const Context &c, int n_levels, const int32_t *w, const int32_t *h, const svs_fastgrid *grids, int corner_cap = 8192)
      : ctx_(c), f_(nullptr), n_levels_(n_levels), cap_(corner_cap) {
    for (int l = 0; l < n_levels; ++l) grids_[l] = grids[l];
    c.check(svs_fast_create(c.get(), n_levels, w, h, grids, 1, corner_cap, &f_));
  }
  ~FastGrid() { if (f_) svs_fast_destroy(f_); }
  FastGrid(const FastGrid &) = delete;
  FastGrid &operator=(const FastGrid &) = delete;
  // void FastGrid::detectAdaptively(const cv::Mat& img, int trials, QuadTree<int>* qt) for every level
  // (stereo_frontend.cpp:657-679); corners[l] comes back in the quadtree insertion order
  bool detectAdaptively(const FrameDev &fr, int trials, std::vector<Corner> *corners /* [n_levels] */) { return run(fr, trials, corners); }
  // static void FastGrid::detect(const cv::Mat&, const CellGrid2d&, QuadTree<int>*): stored thresholds
  bool detect(const FrameDev &fr, std::vector<Corner> *corners) { return run(fr, 0, corners); }
  // const CellGrid2d& cell_grid2d() const : persistent per-cell thresholds of one level
  std::vector<int32_t> cell_grid2d(int level) {
    std::vector<int32_t> thr((size_t)grids_[level].gx * grids_[level].gy);
    ctx_.check(svs_fast_download(f_, 0, level, nullptr, 0, nullptr, nullptr, nullptr, thr.data()));
    return thr;
  }
  // corners kept per cell by the last detection, cells row-major: the reference's quadtree content is the corner's index
  // INSIDE its cell (fast_grid.cpp:143-149), so the host walks corners[l] with these counts
  std::vector<int32_t> cell_counts(int level) {
    std::vector<int32_t> cnt((size_t)grids_[level].gx * grids_[level].gy);
    ctx_.check(svs_fast_download(f_, 0, level, nullptr, 0, nullptr, cnt.data(), nullptr, nullptr));
    return cnt;
  }
  bool set_cell_grid2d(int level, const std::vector<int32_t> &thr) { return ctx_.check(svs_fast_set_thresholds(f_, 0, level, thr.data())); }
  svs_fast *handle() const { return f_; }

 private:
  bool run(const FrameDev &fr, int trials, std::vector<Corner> *corners) {
    const uint8_t *img[SVS_NUM_PYR_LEVELS]; int32_t stride[SVS_NUM_PYR_LEVELS]; size_t bs[SVS_NUM_PYR_LEVELS];
    for (int l = 0; l < n_levels_; ++l) { img[l] = fr.pyr(l); stride[l] = fr.stride(l); bs[l] = 0; }
    if (!ctx_.check(svs_fast_detect(f_, img, stride, bs, 1, trials))) return false;
    for (int l = 0; corners && l < n_levels_; ++l) {
      corners[l].resize((size_t)cap_);
      int32_t n = 0;
      if (!ctx_.check(svs_fast_download(f_, 0, l, &corners[l][0].x, cap_, &n, nullptr, nullptr, nullptr))) return false;
      corners[l].resize((size_t)n);
    }
    return true;
  }
  const Context &ctx_;
  svs_fast *f_;
  int n_levels_, cap_;
  svs_fastgrid grids_[SVS_NUM_PYR_LEVELS];
};

// GuidedMatcher<StereoCamera>::match (matcher.hpp:67-83).  keyframe_map / vertex_map look-ups and the
// append into TrackData stay on the host (hash-map bookkeeping); the per-point arithmetic runs on
// the device.  results[i].status == SVS_MATCH_OK <=> the reference appends an observation.
class GuidedMatcher {
 public:
  explicit GuidedMatcher(const Context &c) : ctx_(c) {}
  bool match(const std::vector<svs_keyframe> &keyframes /* device pyramids + T_anchor_from_w */,
             const double T_cur_from_actkey[12], const double T_actkey_from_w[12], const FrameDev &cur_frame,
             FastGrid &feature_tree, const svs_cam cam_vec[SVS_NUM_PYR_LEVELS],
             const std::vector<svs_candidate_point> &ap_map, int SEARCHRADIUS, int thr_mean, int thr_std,
             std::vector<svs_match_result> *results) {
    const size_t n = ap_map.size();
    results->assign(n, svs_match_result());
    if (n == 0) return true;
    Call c(ctx_, keyframes, T_cur_from_actkey, T_actkey_from_w, cur_frame, cam_vec, ap_map, SEARCHRADIUS, thr_mean, thr_std);
    if (!c.ok || !ctx_.check(svs_match(ctx_.get(), &c.a, feature_tree.handle(), c.out.get()))) return false;
    return c.out.download(results->data(), n);
  }
  // subpixelAccuracy (matcher.cpp:241-309; returnBestMatch calls it, the reference keeps its body behind `#if 0`) on the records match() returned for the same
  // arguments: the SVS_MATCH_OK records get their observation from the refined position (or become SVS_MATCH_NO_DISP), in place; info: one record per result,
  // optional.  See svs_match_subpixel.
  bool refineSubpixel(const std::vector<svs_keyframe> &keyframes, const double T_cur_from_actkey[12], const double T_actkey_from_w[12], const FrameDev &cur_frame,
                      const svs_cam cam_vec[SVS_NUM_PYR_LEVELS], const std::vector<svs_candidate_point> &ap_map, const svs_subpix_params &prm,
                      std::vector<svs_match_result> *results, std::vector<svs_subpix_info> *info = 0) {
    const size_t n = ap_map.size();
    if (results->size() != n) return false;
    if (info) info->assign(n, svs_subpix_info());
    if (n == 0) return true;
    Call c(ctx_, keyframes, T_cur_from_actkey, T_actkey_from_w, cur_frame, cam_vec, ap_map, 0, 0, 0);
    DeviceBuffer<svs_subpix_info> d_info(ctx_, info ? n : 0);
    if (!c.ok || !c.out.upload(results->data(), n)) return false;
    if (!ctx_.check(svs_match_subpixel(ctx_.get(), &c.a, &prm, c.out.get(), info ? d_info.get() : 0))) return false;
    return c.out.download(results->data(), n) && (!info || d_info.download(info->data(), n));
  }

 private:
  // the device copies of one call's tables and the svs_match_args over them
  struct Call {
    DeviceBuffer<svs_keyframe> kf;
    DeviceBuffer<svs_candidate_point> pts;
    DeviceBuffer<double> T;
    DeviceBuffer<svs_match_result> out;
    svs_match_args a;
    bool ok;
    Call(const Context &ctx, const std::vector<svs_keyframe> &keyframes, const double T_cur_from_actkey[12], const double T_actkey_from_w[12], const FrameDev &cur_frame,
         const svs_cam cam_vec[SVS_NUM_PYR_LEVELS], const std::vector<svs_candidate_point> &ap_map, int SEARCHRADIUS, int thr_mean, int thr_std)
        : kf(ctx, keyframes.size()), pts(ctx, ap_map.size()), T(ctx, 24), out(ctx, ap_map.size()) {
      double TT[24];
      mul(T_cur_from_actkey, T_actkey_from_w, TT);     // matcher.cpp:330
      inv(T_actkey_from_w, TT + 12);                   // matcher.cpp:328
      ok = kf.upload(keyframes.data(), keyframes.size()) && pts.upload(ap_map.data(), ap_map.size()) && T.upload(TT, 24);
      std::memset(&a, 0, sizeof a);
      a.d_kfs = kf.get(); a.n_kf = (int32_t)keyframes.size(); a.d_pts = pts.get(); a.n_pts = (int32_t)ap_map.size();
      a.d_T_cur_from_w = T.get(); a.d_T_w_from_actkey = T.get() + 12;
      for (int l = 0; l < SVS_NUM_PYR_LEVELS; ++l) { a.d_cur_pyr[l] = cur_frame.pyr(l); a.cur_stride[l] = cur_frame.stride(l); a.cam_vec[l] = cam_vec[l]; }
      a.d_disp = cur_frame.disp(); a.disp_stride = cur_frame.stride(0);
      a.search_radius = SEARCHRADIUS; a.thr_mean = thr_mean; a.thr_std = thr_std; a.n_batch = 1;
    }
  };
  static void mul(const double *A, const double *B, double *C) {
    for (int i = 0; i < 3; ++i) { for (int j = 0; j < 4; ++j) C[4 * i + j] = A[4 * i] * B[j] + A[4 * i + 1] * B[4 + j] + A[4 * i + 2] * B[8 + j]; C[4 * i + 3] += A[4 * i + 3]; }
  }
  static void inv(const double *A, double *B) {
    for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) B[4 * i + j] = A[4 * j + i];
    for (int i = 0; i < 3; ++i) B[4 * i + 3] = -(B[4 * i] * A[3] + B[4 * i + 1] * A[7] + B[4 * i + 2] * A[11]);
  }
  const Context &ctx_;
};

// PoseOptimizer<SE3,6,IdObs<3>,3> (BA_SE3_XYZ_STEREO, pose_optimizer.h:486): calcFastMotionOnly over the matcher's
// TrackData (stereo_frontend.cpp:1058-1063).  `track` = the result records of one or more GuidedMatcher::match calls
// (entries with status != SVS_MATCH_OK are skipped, as they never reach obs_list).
struct PoseOptimizerParams {             // pose_optimizer.h:36-58
  PoseOptimizerParams(bool robust_kernel = true, double kernel_param = 1, int num_iter = 50, double initial_mu = -1)
      : robust_kernel(robust_kernel), kernel_param(kernel_param), num_iter(num_iter), initial_mu(initial_mu), tau(0.00001) {}
  bool robust_kernel; double kernel_param; int num_iter; double initial_mu; double tau;
};
class BA_SE3_XYZ_STEREO {
 public:
  explicit BA_SE3_XYZ_STEREO(const Context &c) : ctx_(c) {}
  bool calcFastMotionOnly(const std::vector<svs_match_result> &track, const svs_cam &cam, const PoseOptimizerParams &ba_params,
                          double T_cur_from_actkey[12], svs_pose_opt_stats *stats) {
    DeviceBuffer<svs_match_result> d_res(ctx_, track.size() ? track.size() : 1);
    DeviceBuffer<double> d_T(ctx_, 12);
    DeviceBuffer<svs_pose_opt_stats> d_st(ctx_, 1);
    if ((track.size() && !d_res.upload(track.data(), track.size())) || !d_T.upload(T_cur_from_actkey, 12)) return false;
    svs_pose_opt_params p;
    std::memset(&p, 0, sizeof p);
    p.robust_kernel = ba_params.robust_kernel; p.num_iter = ba_params.num_iter; p.kernel_param = ba_params.kernel_param;
    p.initial_mu = ba_params.initial_mu; p.tau = ba_params.tau;
    if (!ctx_.check(svs_motion_only(ctx_.get(), d_res.get(), (int)track.size(), track.size(), &cam, &p, d_T.get(), d_st.get(), 1))) return false;
    svs_pose_opt_stats st;
    if (!d_T.download(T_cur_from_actkey, 12) || !d_st.download(&st, 1)) return false;
    if (stats) *stats = st;
    return st.status == 0;      // 1: empty list (assert in the reference), 2: NaN residual (throw in the reference)
  }
  // StereoFrontend::processMatchedPoints (stereo_frontend.cpp:834-974), numeric part: reprojection gate at
  // T_cur_from_actkey, PointStatistics counters, level positions.  `points[i]` is the candidate point record i of
  // `track` was matched from; records below n_new_records stem from the new-feature match calls (:989-1030).
  // The caller then walks `gated` to fill new_point_list / track_point_list / point_tree (host containers).
  bool processMatchedPoints(const std::vector<svs_match_result> &track, const std::vector<svs_candidate_point> &points, int n_new_records,
                            const svs_cam &cam, const double T_cur_from_actkey[12], float max_reproj_error,
                            std::vector<svs_gated_point> *gated, svs_point_stats *stats) {
    if (track.size() != points.size() || !gated || !stats) return false;
    const size_t n = track.size();
    DeviceBuffer<svs_match_result> d_res(ctx_, n ? n : 1);
    DeviceBuffer<svs_candidate_point> d_pts(ctx_, n ? n : 1);
    DeviceBuffer<svs_gated_point> d_g(ctx_, n ? n : 1);
    DeviceBuffer<double> d_T(ctx_, 12);
    DeviceBuffer<svs_point_stats> d_st(ctx_, 1);
    if (n && (!d_res.upload(track.data(), n) || !d_pts.upload(points.data(), n))) return false;
    if (!d_T.upload(T_cur_from_actkey, 12)) return false;
    if (!ctx_.check(svs_process_matched_points(ctx_.get(), d_res.get(), d_pts.get(), (int)n, n, n, n_new_records, &cam, d_T.get(), max_reproj_error,
                                               d_g.get(), n, d_st.get(), 1))) return false;
    gated->resize(n);
    if (n && !d_g.download(gated->data(), n)) return false;
    return d_st.download(stats, 1);
  }

 private:
  const Context &ctx_;
};

// StereoFrontend::calcDisparityCpu (stereo_frontend.cpp:620-653): cv::StereoBM on the level-0 left image and the
// right image; the float disparity lands in the frame's disparity image (FrameDev::disp, -1 where filtered).
// num_disp16 = ui.num_disp16 (stereo_frontend.cpp:536 / :623), 1..10: 16 * num_disp16 disparities are searched, in frames at least that + 6 pixels wide.
class StereoBM {
 public:
  StereoBM(const Context &c, int w, int h, int num_disp16 = 2) : ctx_(c), s_(0), w_(w), h_(h), right_(c, (size_t)((w + 63) / 64 * 64) * h) {
    svs_stereo_params p = {31, 7, 0, 16 * num_disp16, 10, 15, 100, 32, 1};      // state set at stereo_frontend.cpp:626-636
    ok_ = c.check(svs_stereo_create(c.get(), w, h, 1, &p, &s_));
  }
  ~StereoBM() { if (s_) svs_stereo_destroy(s_); }
  bool ok() const { return ok_; }
  bool operator()(const FrameDev &left, const Image8 &right, FrameDev *out) {
    const int stride = left.stride(0);
    std::vector<uint8_t> tmp((size_t)stride * h_);
    for (int y = 0; y < h_; ++y) std::memcpy(&tmp[(size_t)y * stride], right.data + (size_t)y * right.stride, (size_t)w_);
    if (!ok_ || !right_.upload(tmp.data(), tmp.size())) return false;
    return ctx_.check(svs_stereo_compute(s_, left.pyr(0), stride, 0, right_.get(), stride, 0, const_cast<float *>(out->disp()), stride, 0, 1));
  }

 private:
  StereoBM(const StereoBM &);
  StereoBM &operator=(const StereoBM &);
  const Context &ctx_;
  svs_stereo *s_;
  int w_, h_;
  bool ok_;
  DeviceBuffer<uint8_t> right_;
};

// DenseTracker, CPU-path semantics (dense_tracking.h:53-97, dense_tracking.cpp:222-423).
class DenseTracker {
 public:
  DenseTracker(const Context &c, const svs_cam cam_vec[SVS_NUM_PYR_LEVELS]) : ctx_(c), d_T_(c, 12), d_T_jac_(c, 36), d_passes_(c, 1) {
    for (int l = 0; l < SVS_NUM_PYR_LEVELS; ++l) {
      cam_[l] = cam_vec[l];
      const size_t n4 = (size_t)(cam_vec[l].w / 4) * (cam_vec[l].h / 4) * 4;
      cloud_[l] = DeviceBuffer<float>(c, n4);
      d_rimg_[l] = DeviceBuffer<float>(c, n4);
      residual_img[l].assign(n4, 0.f);                                   // setTo(cv::Scalar(0,0,0,1)), dense_tracking.cpp:54
      for (size_t i = 3; i < n4; i += 4) residual_img[l][i] = 1.f;
    }
  }
  std::vector<float> residual_img[SVS_NUM_PYR_LEVELS];                   // public member of the reference (dense_tracking.h:66), float4 per sample
  // void computeDensePointCloudCpu(const SE3& T_cur_from_actkey): ref_dense_points_ from the frame's disparity
  bool computeDensePointCloudCpu(const FrameDev &fr, const double T_cur_from_actkey[12]) {
    if (!d_T_.upload(T_cur_from_actkey, 12)) return false;
    for (int l = 0; l < SVS_NUM_PYR_LEVELS; ++l)
      if (!ctx_.check(svs_pointcloud_cpu_sem(ctx_.get(), fr.disp(), fr.stride(0), 0, &cam_[l], l, d_T_.get(), cloud_[l].get(), 0, 1))) return false;
    return svs_ctx_sync(ctx_.get()) == SVS_OK;
  }
  // ref_dense_points_[level] given by the host (state restored from a saved session; tests): float4 per quarter-grid sample, row-major
  bool setDensePointCloud(int level, const float *h_cloud4) { return cloud_[level].upload(h_cloud4, cloud_[level].size()); }
  bool getDensePointCloud(int level, float *h_cloud4) const { return cloud_[level].download(h_cloud4, cloud_[level].size()); }
  // void denseTrackingCpu(SE3* T_cur_from_actkey): in/out pose, whole LM loop in one device launch
  bool denseTrackingCpu(const FrameDev &prev, const FrameDev &cur, double T_cur_from_actkey[12]) {
    svs_dense_track_args a;
    std::memset(&a, 0, sizeof a);
    for (int l = 0; l < SVS_NUM_PYR_LEVELS; ++l) {
      a.d_cloud[l] = cloud_[l].get(); a.d_prev_u8[l] = prev.pyr(l); a.pstride[l] = prev.stride(l);
      a.d_cur[l] = cur.f32(l); a.d_dx[l] = cur.dx(l); a.d_dy[l] = cur.dy(l); a.fstride[l] = cur.stride(l); a.cam_vec[l] = cam_[l];
    }
    a.d_T_jac_out = d_T_jac_.get();
    if (!d_T_.upload(T_cur_from_actkey, 12)) return false;
    if (!ctx_.check(svs_dense_track_cpu_sem(ctx_.get(), &a, d_T_.get(), d_passes_.get(), 1))) return false;
    if (want_residual_img) {                                             // the reference always writes it; here it is opt-in (GUI only)
      for (int l = 0; l < SVS_NUM_PYR_LEVELS; ++l) {
        if (!ctx_.check(svs_dense_residual_image_cpu_sem(ctx_.get(), cloud_[l].get(), 0, prev.pyr(l), prev.stride(l), 0, cur.f32(l), cur.stride(l), 0,
                                                         nullptr, 0, 0, &cam_[l], d_T_jac_.get() + 12 * l, 36, d_rimg_[l].get(), 0, 1))) return false;
        if (!d_rimg_[l].download(residual_img[l].data(), residual_img[l].size())) return false;
      }
    }
    return d_T_.download(T_cur_from_actkey, 12);
  }
  bool want_residual_img = false;

 private:
  const Context &ctx_;
  svs_cam cam_[SVS_NUM_PYR_LEVELS];
  DeviceBuffer<float> cloud_[SVS_NUM_PYR_LEVELS], d_rimg_[SVS_NUM_PYR_LEVELS];
  DeviceBuffer<double> d_T_, d_T_jac_;
  DeviceBuffer<int32_t> d_passes_;
};


// GpuTracker (gpu/dense_tracking.cuh:281-342): the CUDA build's per-pass call surface, same argument lists (device pointers into the
// caller's images, strides in elements), blocking like the reference (each call ends with a device synchronisation there too).
struct GpuIntrinsics { float focal_length, pp_x, pp_y; void set(double fl, double px, double py) { focal_length = (float)fl; pp_x = (float)px; pp_y = (float)py; } };
struct GpuMatrix34 { float data_colmajor[12]; void set(const double *m_colmajor) { for (int i = 0; i < 12; ++i) data_colmajor[i] = (float)m_colmajor[i]; } };
struct GpuMatrix4 { float data_colmajor[16]; void set(const double *m_colmajor) { for (int i = 0; i < 16; ++i) data_colmajor[i] = (float)m_colmajor[i]; } };
struct GpuTrackingData { double hessian[21], jacobian_times_res[6]; };      // packed upper by column, as GpuSymMatrix6 (f64 sums here)
// The reference's own result layout (gpu/dense_tracking.cuh:40-277): 21 + 6 FLOATS with the copyTo members its caller uses
// (`tracking_data.hessian.copyTo(H.data())`, dense_tracking.cpp:100-104), for a host that keeps the reference's loop untouched.  The sums are
// still formed in f64 on the device and narrowed once at the end.
struct GpuVector6F32 {
  static const int NUM_ROWS = 6;
  float data[NUM_ROWS];
  void copyTo(double *vec) const { for (int i = 0; i < NUM_ROWS; ++i) vec[i] = data[i]; }
};
struct GpuSymMatrix6F32 {
  static const int NUM_ROWS = 6;
  float data[21];
  void copyTo(double *mat_colmajor) const {      // gpu/dense_tracking.cuh:118-132
    int i = 0;
    for (int c = 0; c < NUM_ROWS; ++c)
      for (int r = 0; r <= c; ++r) { const float v = data[i]; mat_colmajor[r + NUM_ROWS * c] = v; mat_colmajor[c + NUM_ROWS * r] = v; ++i; }
  }
};
struct GpuTrackingDataF32 { GpuSymMatrix6F32 hessian; GpuVector6F32 jacobian_times_res; };
inline bool computePointCloud(const Context &c, const GpuMatrix4 &TQ_actkey_from_cur, const float *d_disparities, int width, int height, int stride_in,
                              int stride_out, int factor, float *d_point_cloud4) {
  return c.check(svs_pointcloud_full(c.get(), TQ_actkey_from_cur.data_colmajor, d_disparities, width, height, stride_in, stride_out, factor, d_point_cloud4)) &&
         svs_ctx_sync(c.get()) == SVS_OK;
}
class GpuTracker {
 public:
  GpuTracker(const Context &c, int /*width*/, int /*height*/) : ctx_(c), d_sums_(c, 1), cur_(nullptr), dx_(nullptr), dy_(nullptr) {}
  void bindTexture(const float *d_img_cur, const float *d_dx_img_cur, const float *d_dy_img_cur, int, int, int) { cur_ = d_img_cur; dx_ = d_dx_img_cur; dy_ = d_dy_img_cur; }
  bool jacobianReduction(const float *d_img_prev, const float *d_point_cloud_prev4, const GpuMatrix34 &T_cur_from_prev, const GpuIntrinsics &K, int width, int height,
                         int stride_float_img, int stride_float4_img, GpuTrackingData *tracking_result) {
    svs_dense_sums s;
    if (!pass(d_img_prev, d_point_cloud_prev4, T_cur_from_prev, K, width, height, stride_float_img, stride_float4_img, 1, &s)) return false;
    for (int i = 0; i < 21; ++i) tracking_result->hessian[i] = s.H[i];
    for (int i = 0; i < 6; ++i) tracking_result->jacobian_times_res[i] = s.b[i];
    return true;
  }
  // the same call with the reference's result type (21 + 6 floats)
  bool jacobianReduction(const float *d_img_prev, const float *d_point_cloud_prev4, const GpuMatrix34 &T_cur_from_prev, const GpuIntrinsics &K, int width, int height,
                         int stride_float_img, int stride_float4_img, GpuTrackingDataF32 *tracking_result) {
    GpuTrackingData d;
    if (!jacobianReduction(d_img_prev, d_point_cloud_prev4, T_cur_from_prev, K, width, height, stride_float_img, stride_float4_img, &d)) return false;
    for (int i = 0; i < 21; ++i) tracking_result->hessian.data[i] = (float)d.hessian[i];
    for (int i = 0; i < 6; ++i) tracking_result->jacobian_times_res.data[i] = (float)d.jacobian_times_res[i];
    return true;
  }
  float chi2(const float *d_img_prev, const float *d_point_cloud_prev4, const GpuMatrix34 &T_cur_from_prev, const GpuIntrinsics &K, int width, int height,
             int stride_float_img, int stride_float4_img) {
    svs_dense_sums s;
    return pass(d_img_prev, d_point_cloud_prev4, T_cur_from_prev, K, width, height, stride_float_img, stride_float4_img, 0, &s) ? (float)s.chi2 : -1.f;
  }
  bool residualImage(const float *d_img_prev, const float *d_point_cloud_prev4, const GpuMatrix34 &T, const GpuIntrinsics &K, int width, int height,
                     int stride_float_img, int stride_float4_img, float *d_res_img4) {
    return ctx_.check(svs_dense_residual_image_full(ctx_.get(), d_point_cloud_prev4, width, height, stride_float4_img, d_img_prev, cur_, stride_float_img,
                                                    K.focal_length, K.pp_x, K.pp_y, T.data_colmajor, d_res_img4)) && svs_ctx_sync(ctx_.get()) == SVS_OK;
  }

 private:
  bool pass(const float *prev, const float *cloud4, const GpuMatrix34 &T, const GpuIntrinsics &K, int w, int h, int sf, int s4, int jac, svs_dense_sums *out) {
    return ctx_.check(svs_dense_pass_full(ctx_.get(), cloud4, w, h, s4, prev, cur_, dx_, dy_, sf, K.focal_length, K.pp_x, K.pp_y, T.data_colmajor, jac, d_sums_.get())) &&
           d_sums_.download(out, 1);
  }
  const Context &ctx_;
  DeviceBuffer<svs_dense_sums> d_sums_;
  const float *cur_, *dx_, *dy_;
};

// DenseTracker of the CUDA build: denseTrackingGpu(SE3*) as ONE launch (dense_tracking.cpp:60-193).  The caller hands over the device images of
// FrameData (gpu_pyr_float32 / _dx / _dy of the current frame, gpu_pyr_float32 of the previous one) and dev_ref_dense_points_.
class DenseTrackerGpu {
 public:
  explicit DenseTrackerGpu(const Context &c) : ctx_(c), d_T_(c, 12), d_passes_(c, 1) {}
  struct Levels {                          // per pyramid level, device pointers; strides in elements (float / float4)
    const float *cloud4[SVS_NUM_PYR_LEVELS], *prev[SVS_NUM_PYR_LEVELS], *cur[SVS_NUM_PYR_LEVELS], *dx[SVS_NUM_PYR_LEVELS], *dy[SVS_NUM_PYR_LEVELS];
    int stride_f4[SVS_NUM_PYR_LEVELS], stride_f[SVS_NUM_PYR_LEVELS];
    svs_cam cam_vec[SVS_NUM_PYR_LEVELS];
  };
  // void denseTrackingGpu(SE3 * T_cur_from_actkey): in/out pose.  passes (optional): fused sweeps executed
  bool denseTrackingGpu(const Levels &L, double T_cur_from_actkey[12], int *passes = nullptr) {
    svs_dense_track_full_args a;
    std::memset(&a, 0, sizeof a);
    for (int l = 0; l < SVS_NUM_PYR_LEVELS; ++l) {
      a.d_cloud4[l] = L.cloud4[l]; a.stride_f4[l] = L.stride_f4[l]; a.d_prev[l] = L.prev[l]; a.d_cur[l] = L.cur[l]; a.d_dx[l] = L.dx[l]; a.d_dy[l] = L.dy[l];
      a.stride_f[l] = L.stride_f[l]; a.w[l] = L.cam_vec[l].w; a.h[l] = L.cam_vec[l].h; a.f[l] = L.cam_vec[l].f; a.cx[l] = L.cam_vec[l].cx; a.cy[l] = L.cam_vec[l].cy;
    }
    if (!d_T_.upload(T_cur_from_actkey, 12)) return false;
    if (!ctx_.check(svs_dense_track_full(ctx_.get(), &a, d_T_.get(), d_passes_.get(), 1))) return false;
    int32_t p = 0;
    if (!d_passes_.download(&p, 1) || p < 0) return false;
    if (passes) *passes = p;
    return d_T_.download(T_cur_from_actkey, 12);
  }

 private:
  const Context &ctx_;
  DeviceBuffer<double> d_T_;
  DeviceBuffer<int32_t> d_passes_;
};

// StereoFrontend::processFrame(bool*) / processFirstFrame() (stereo_frontend.h:88-95): the data-parallel part of a frame in ONE blocking call with
// host buffers in and out; the keyframe switch / drop decision and the AddToOptimzer lists behind it come from decideKeyframes, the caller applies them.
class BackendMap;
struct MapAddKeyframeResult {      // BackendMap::AddKeyframeResult: what addKeyframe did (StereoFrontend::addNewKeyframeToMap names it in front of BackendMap)
  std::vector<std::pair<int, int> > neighborid_to_strength;      // ascending id, after the clamp of oldkey
  std::vector<int32_t> new_neighbors;                            // the keys that got an edge (key, newkey), ascending: their slots follow this order
  std::vector<svs_map_constraint_result> constraints;            // one per new edge
  std::vector<int32_t> missing;                                  // anchors some new edge lacked, ascending, each once: computeAbsolutePoses + computeConstraints complete them
  std::vector<uint8_t> new_kept, track_exists;
  std::vector<int32_t> exclude_set;                              // addKeyframeToPlaceRecog (backend.cpp:407-430): newkey and its new neighbours
  bool do_loop_detection, over_capacity;
};
struct FrontendVertex { int frame_id; double T_me_from_w[12]; };      // an entry of neighborhood_->vertex_map: the id and the pose (the edge strengths stay with the caller)
class StereoFrontend {
 public:
  StereoFrontend(const Context &c, const svs_cam &cam, const svs_frontend_params &prm, int max_points, int max_keyframes)
      : ctx_(c), fe_(nullptr), max_points_(max_points), max_keyframes_(max_keyframes) {
    ok_ = c.check(svs_frontend_create(c.get(), &cam, &prm, max_points, max_keyframes, &fe_));
  }
  // n_streams independent front ends whose stages run as one launch each (svs_frontend_create_batch): frames in device memory through processFirstFrames /
  // processFrames below; the host-buffer calls (processFirstFrame, processFrame, ...) need n_streams == 1.  The resident new-point calls take the stream
  StereoFrontend(const Context &c, const svs_cam &cam, const svs_frontend_params &prm, int max_points, int max_keyframes, int n_streams)
      : ctx_(c), fe_(nullptr), max_points_(max_points), max_keyframes_(max_keyframes), n_streams_(n_streams) {
    ok_ = c.check(svs_frontend_create_batch(c.get(), &cam, &prm, max_points, max_keyframes, n_streams, &fe_));
  }
  ~StereoFrontend() { if (fe_) svs_frontend_destroy(fe_); }
  int streams() const { return n_streams_; }
  bool processFirstFrames(const svs_frames_dev *frames) { return ctx_.check(svs_frontend_first_frames(fe_, frames)); }
  // asynchronous; poses [n_streams][12]
  bool processFrames(const svs_frames_dev *frames, const double *T_cur_from_actkey, const double *T_actkey_from_w) {
    return ctx_.check(svs_frontend_process_frames(fe_, frames, T_cur_from_actkey, T_actkey_from_w));
  }
  bool keepKeyframes(int slot, const double *T_kf_from_w) { return ctx_.check(svs_frontend_keep_keyframes(fe_, slot, T_kf_from_w)); }
  StereoFrontend(const StereoFrontend &) = delete;
  StereoFrontend &operator=(const StereoFrontend &) = delete;
  // cuda_build: the reference compiled with SCAVISLAM_CUDA_SUPPORT (full-resolution denseTrackingGpu, matcher search radius 4, stereo_frontend.cpp:1043-1047);
  // n_levels: use_n_levels_in_frontent (stereo_frontend.cpp:68; the code default is 2, the shipped configurations set 3); num_disp16: ui.num_disp16 (:536 / :623),
  // 1..10, for use_block_matching
  static svs_frontend_params referenceParams(bool block_matching, bool cuda_build = false, int n_levels = 3, int num_disp16 = 2) {
    svs_frontend_params p;
    std::memset(&p, 0, sizeof p);
    p.fast_trials = 6; p.search_radius = cuda_build ? 4 : 8; p.thr_mean = 22; p.thr_std = 10; p.max_reproj_error = 2.f; p.use_block_matching = block_matching ? 1 : 0;
    p.n_levels = n_levels; p.num_max_points = 300; p.min_matches = 20; p.cuda_build = cuda_build ? 1 : 0;
    p.pose_opt.robust_kernel = 1; p.pose_opt.num_iter = 15; p.pose_opt.kernel_param = 2.0; p.pose_opt.initial_mu = -1.0; p.pose_opt.tau = 1e-5;
    const svs_stereo_params sp = {31, 7, 0, 16 * num_disp16, 10, 15, 100, 32, 1};
    p.stereo = sp;
    return p;
  }
  bool ok() const { return ok_; }
  bool processFirstFrame(Image8 left, const Image8 *right, const ImageF *disp) {
    return ctx_.check(svs_frontend_first_frame(fe_, left.data, left.stride, right ? right->data : nullptr, right ? right->stride : 0, disp ? disp->data : nullptr,
                                               disp ? disp->stride : 0));
  }
  bool keepKeyframe(int slot, const double T_kf_from_w[12]) { return ctx_.check(svs_frontend_keep_keyframe(fe_, slot, T_kf_from_w)); }
  bool setCandidates(const std::vector<svs_candidate_point> &ap_map, int n_new_records) {
    n_ = (int)ap_map.size();
    return ctx_.check(svs_frontend_set_candidates(fe_, ap_map.data(), n_, n_new_records));
  }
  // matchAndTrack's lists in the order it walks them (stereo_frontend.cpp:976-1050): group_end[0] = end of newpoint_map[actkey_id], one end per neighbour in
  // strength_to_neighbors order, the last = ap_map.size() = end of neighborhood_->point_list
  bool setCandidateLists(const std::vector<svs_candidate_point> &ap_map, const std::vector<int32_t> &group_end) {
    n_ = (int)ap_map.size();
    return ctx_.check(svs_frontend_set_candidates_grouped(fe_, 0, ap_map.data(), n_, group_end.data(), (int)group_end.size()));
  }
  // the grabber side of frame_grabber.hpp:93-155: hand the NEXT frame over while the current one is processed; processFrame / processFirstFrame then get no image
  bool prefetchFrame(Image8 left, const Image8 *right, const ImageF *disp) {
    return ctx_.check(svs_frontend_prefetch_frame(fe_, left.data, left.stride, right ? right->data : nullptr, right ? right->stride : 0, disp ? disp->data : nullptr,
                                                  disp ? disp->stride : 0));
  }
  bool processPrefetchedFrame(double T_cur_from_actkey[12], const double T_actkey_from_w[12], svs_frame_result *res, std::vector<svs_match_result> *matches,
                              std::vector<svs_gated_point> *gated) {
    matches->resize((size_t)n_); gated->resize((size_t)n_);
    if (!ctx_.check(svs_frontend_process_frame(fe_, nullptr, 0, nullptr, 0, nullptr, 0, T_cur_from_actkey, T_actkey_from_w, res, matches->data(), gated->data())))
      return false;
    for (int i = 0; i < 12; ++i) T_cur_from_actkey[i] = res->T_cur_from_actkey[i];
    return res->tracking_ok != 0;
  }
  // returns what matchAndTrack returns (enough features matched); *T_cur_from_actkey is in/out like the reference's member
  bool processFrame(Image8 left, const Image8 *right, const ImageF *disp, double T_cur_from_actkey[12], const double T_actkey_from_w[12], svs_frame_result *res,
                    std::vector<svs_match_result> *matches, std::vector<svs_gated_point> *gated) {
    matches->resize((size_t)n_); gated->resize((size_t)n_);
    if (!ctx_.check(svs_frontend_process_frame(fe_, left.data, left.stride, right ? right->data : nullptr, right ? right->stride : 0, disp ? disp->data : nullptr,
                                               disp ? disp->stride : 0, T_cur_from_actkey, T_actkey_from_w, res, matches->data(), gated->data())))
      return false;
    for (int i = 0; i < 12; ++i) T_cur_from_actkey[i] = res->T_cur_from_actkey[i];
    return res->tracking_ok != 0;
  }
  bool recomputeDensePointCloud(const double T_cur_from_actkey[12]) { return ctx_.check(svs_frontend_recompute_cloud(fe_, T_cur_from_actkey)); }
  // sub-pixel matches from the next step on (one stream or a batch): GuidedMatcher::refineSubpixel's pass behind the step's matcher; prm == 0 switches it off again
  bool setSubpixelAccuracy(const svs_subpix_params *prm) { return ctx_.check(svs_frontend_set_subpixel(fe_, prm)); }
  bool subpixelInfo(std::vector<svs_subpix_info> *info, int n_points, int stream = 0) {      // the last step's records of one stream; refused while the option is off
    info->assign((size_t)(n_points > 0 ? n_points : 0), svs_subpix_info());
    return ctx_.check(svs_frontend_subpixel_info(fe_, stream, info->data()));
  }
  // Backend::computeNeighborhood (backend.cpp:244-386) from the vertex list onwards, on the device-resident map: neighborhood_->point_list is written into the
  // candidate list behind the new-point groups (setCandidateLists' groups 0 .. G-2: newpoints / newpoint_group_end), neighborhood_->vertex_map comes back as ids
  // and poses, and with refresh_poses every slot of slot_keyframe_ids that names a keyframe of the map takes the map's pose.  vertex_ids: the root first, then
  // what findNeighborsOfRoot chose; slot_keyframe_ids [max_keyframes]: the frame id kept in each slot, -1 for none; point_ids: per record of the built list.
  // false: refused, or over capacity (res->over_capacity; the list is then the one of before).  Defined behind BackendMap
  inline bool setCandidatesFromMap(BackendMap &map, const std::vector<int32_t> &vertex_ids, const std::vector<int32_t> &slot_keyframe_ids,
                                   const std::vector<svs_candidate_point> &newpoints, const std::vector<int32_t> &newpoint_group_end, bool refresh_poses,
                                   svs_nbh_result *res, std::vector<int32_t> *point_ids, std::vector<FrontendVertex> *vertex_map, int vertex_cap = 64);
  // Backend::computeNeighborhood(root_id) whole (backend.cpp:244-386) on the device-resident map, which is only read (svs_frontend_set_neighborhood_from_root):
  // findNeighborsOfRoot, the points and anchors, computeAbsolutePose for the vertices outside the window, the active keyframe's strength_to_neighbors, the
  // candidate list with the new-point groups in that order, the slot poses and the resident vertex table of decideKeyframes.  newpoints / newpoint_group_end:
  // newpoint_map as groups; the first n_fixed_groups are newpoint_map[actkey_id], every later group g is newpoint_map[newpoint_group_keyframe[g]] and is left
  // out when that keyframe is no neighbour of the active one.  act_neighbors: vertex_map indices of strength_to_neighbors(actkey).  false: refused, root outside
  // the window or over capacity (see *res; the stream is then as before).  Defined behind BackendMap
  inline bool setNeighborhoodFromMap(BackendMap &map, int32_t root_id, int32_t actkey_id, const std::vector<int32_t> &slot_keyframe_ids,
                                     const std::vector<svs_candidate_point> &newpoints, const std::vector<int32_t> &newpoint_group_end, int n_fixed_groups,
                                     const std::vector<int32_t> &newpoint_group_keyframe, bool refresh_poses, svs_nbr_result *res, std::vector<int32_t> *point_ids,
                                     std::vector<FrontendVertex> *vertex_map, std::vector<int32_t> *act_neighbors, int max_num_neighbors = 10, int vertex_cap = 64);
  // computeFastCorners' outputs of the frame processed last (stereo_frontend.cpp:656-679): the corner list of a level in the order FastGrid inserts it into the
  // quadtree (cells row-major, corners of a cell row-major), corners per cell, and the persistent thresholds as they stand now (the CellGrid2d snapshot a Frame keeps)
  bool fastCorners(int level, std::vector<Corner> *corners, std::vector<int32_t> *cell_counts, std::vector<int32_t> *thresholds) {
    svs_fast *f = nullptr;
    if (!ctx_.check(svs_frontend_device_view(fe_, 0, nullptr, nullptr, nullptr, nullptr, &f)) || !f) return false;
    corners->resize(16384); cell_counts->assign(SVS_MAX_CELLS, 0); thresholds->assign(SVS_MAX_CELLS, 0);
    int32_t n = 0;
    if (!ctx_.check(svs_fast_download(f, 0, level, &(*corners)[0].x, (int)corners->size(), &n, cell_counts->data(), nullptr, thresholds->data()))) return false;
    corners->resize((size_t)n);
    return true;
  }
  // addNewPoints / addMorePoints / addMorePointsToOtherFrame (stereo_frontend.cpp:682-823) on the state the frame processed last left on the device:
  // new_keyframe_id -> the records' kf_index, first_point_id = the id getNewUniqueId would hand out next; *newpoints = newpoint_map[new_keyframe_id] in list order,
  // num_points[l] += the points taken on level l (the reference's *num_points; addNewPoints starts from 0).  The visiting order is generated from `seed`
  // (scavislam_hip.h); prm == NULL: the reference's defaults (clearance 2, ui.num_max_points 300, ui.min_num_points 25, 3 levels)
  static svs_seed_params seedParams() { svs_seed_params p; svs_seed_params_default(&p); return p; }
  bool addNewPoints(int new_keyframe_id, int first_point_id, uint64_t seed, std::vector<svs_candidate_point> *newpoints, int32_t num_points[3],
                    const svs_seed_params *prm = nullptr) {
    for (int l = 0; l < 3; ++l) num_points[l] = 0;
    return seed_(SVS_SEED_FIRST, new_keyframe_id, nullptr, first_point_id, seed, newpoints, num_points, prm);
  }
  bool addMorePoints(int new_keyframe_id, int first_point_id, uint64_t seed, std::vector<svs_candidate_point> *newpoints, int32_t num_points[3],
                     const svs_seed_params *prm = nullptr) {
    return seed_(SVS_SEED_MORE, new_keyframe_id, nullptr, first_point_id, seed, newpoints, num_points, prm);
  }
  bool addMorePointsToOtherFrame(int new_keyframe_id, const double T_newkey_from_cur[12], int first_point_id, uint64_t seed,
                                 std::vector<svs_candidate_point> *newpoints, int32_t num_points[3], const svs_seed_params *prm = nullptr) {
    return seed_(SVS_SEED_MORE, new_keyframe_id, T_newkey_from_cur, first_point_id, seed, newpoints, num_points, prm);
  }
  // neighborhood_->vertex_map as the keyframe decision reads it (svs_frontend_set_vertex_table): per vertex its pose and its feat_map as an ascending id list
  // (feature_ids[v]) or, where from_map[v] is set, the observer rows of the resident map; active = the index of actkey_id's vertex, neighbor_indices = the
  // vertices of its strength_to_neighbors, slot_keyframe_ids as in setCandidatesFromMap.  Resident until set again
  bool setVertexTable(const std::vector<FrontendVertex> &vertex_map, const std::vector<std::vector<int32_t> > &feature_ids, const std::vector<char> &from_map,
                      int active, const std::vector<int32_t> &neighbor_indices, const std::vector<int32_t> &slot_keyframe_ids) {
    const size_t V = vertex_map.size();
    if (feature_ids.size() != V || (int)slot_keyframe_ids.size() != max_keyframes_) return false;
    std::vector<int32_t> ids(V), begin(V), count(V), all;
    std::vector<double> T(12 * V);
    for (size_t v = 0; v < V; ++v) {
      ids[v] = vertex_map[v].frame_id;
      for (int i = 0; i < 12; ++i) T[12 * v + i] = vertex_map[v].T_me_from_w[i];
      const bool m = v < from_map.size() && from_map[v];
      begin[v] = m ? SVS_KF_SET_MAP : (int32_t)all.size(); count[v] = m ? 0 : (int32_t)feature_ids[v].size();
      if (!m) all.insert(all.end(), feature_ids[v].begin(), feature_ids[v].end());
    }
    svs_vertex_request q;
    std::memset(&q, 0, sizeof q);
    q.stream = 0; q.n_vertex = (int32_t)V; q.act = active; q.n_neighbors = (int32_t)neighbor_indices.size();
    q.h_vertex_kf = ids.data(); q.h_vertex_T = T.data(); q.h_set_begin = begin.data(); q.h_set_count = count.data(); q.h_set_ids = all.data();
    q.h_neighbors = neighbor_indices.data(); q.h_slot_kf = slot_keyframe_ids.data(); q.n_set_ids = (int32_t)all.size();
    return ctx_.check(svs_frontend_set_vertex_table(fe_, 1, &q));
  }
  // stereo_frontend.cpp:265-296 as ONE call behind processFrame: processMatchedPoints' AddToOptimzer lists, shallWeSwitchKeyframe, shallWeDropNewKeyframe and
  // addNewKeyframe's add_flags / T_newkey_from_w / strength_to_neighbors (svs_frontend_decide_keyframes).  The lists (and the record index of every entry, for
  // pruning newpoint_map) come back for a dropped frame, or for every tracked frame with always_lists.  map: the resident map behind from_map sets, or NULL
  static svs_keyframe_decide_params decideParams() { svs_keyframe_decide_params p; svs_keyframe_decide_params_default(&p); return p; }
  bool decideKeyframes(svs_map *map, svs_keyframe_decision *dec, std::vector<svs_map_new_point> *new_points, std::vector<svs_map_track_point> *track_points,
                       std::vector<int32_t> *new_records, std::vector<int32_t> *track_records, bool always_lists = false,
                       const svs_keyframe_decide_params *prm = nullptr) {
    const svs_keyframe_decide_params p = prm ? *prm : decideParams();
    const size_t cap = (size_t)(n_ > 0 ? n_ : 1);
    new_points->resize(cap); track_points->resize(cap); new_records->resize(cap); track_records->resize(cap);
    const bool ok = ctx_.check(svs_frontend_decide_keyframes(fe_, map, &p, always_lists ? 2 : 1, dec, new_points->data(), track_points->data(), new_records->data(),
                                                             track_records->data(), (int)cap));
    const bool have = ok && dec->valid && (always_lists || dec->decision == SVS_KF_DROP);
    new_points->resize(have ? (size_t)dec->n_new : 0); new_records->resize(new_points->size());
    track_points->resize(have ? (size_t)dec->n_track : 0); track_records->resize(track_points->size());
    return ok;
  }
  // ---- newpoint_map on the device (scavislam_hip.h: "front end: newpoint_map on the device"; stereo_frontend.cpp:360-365, :808, :989-1029).  The store keeps one
  // group of records per keyframe id; nothing of it lives on the host.  reserveNewpoints once, before the first of the calls below
  bool reserveNewpoints(int record_cap, int group_cap = SVS_NEWPOINTS_MAX_GROUPS) {
    if (!ctx_.check(svs_frontend_newpoints_reserve(fe_, record_cap, group_cap))) return false;
    record_cap_ = record_cap;
    return true;
  }
  // records already in list order in front of newpoint_map[keyframe_id] (replace: in its place); an absent key creates the list
  bool putNewpoints(int keyframe_id, const std::vector<svs_candidate_point> &records, bool replace = false, int stream = 0) {
    svs_newpoints_put_request q;
    std::memset(&q, 0, sizeof q);
    q.stream = stream; q.kf_id = keyframe_id; q.mode = replace ? SVS_NEWPOINTS_REPLACE : SVS_NEWPOINTS_PREPEND; q.n = (int32_t)records.size(); q.h_records = records.data();
    return ctx_.check(svs_frontend_newpoints_put(fe_, 1, &q));
  }
  // addNewPoints / addMorePoints / addMorePointsToOtherFrame whose records stay on the device: newpoint_map[new_keyframe_id].push_front(...) there (:808).
  // Arguments as the calls above take them, and the stream of a batch front end; only num_points comes back.  The store does not use the records' kf_index (the
  // hand-over writes the slot that holds the group's keyframe): as in the calls above it carries new_keyframe_id, and a read-back through newpoints() shows that id
  bool addNewPointsResident(int new_keyframe_id, int first_point_id, uint64_t seed, int32_t num_points[3], const svs_seed_params *prm = nullptr, int stream = 0) {
    for (int l = 0; l < 3; ++l) num_points[l] = 0;
    return seedResident_(SVS_SEED_FIRST, new_keyframe_id, nullptr, first_point_id, seed, num_points, prm, stream);
  }
  bool addMorePointsResident(int new_keyframe_id, int first_point_id, uint64_t seed, int32_t num_points[3], const svs_seed_params *prm = nullptr, int stream = 0) {
    return seedResident_(SVS_SEED_MORE, new_keyframe_id, nullptr, first_point_id, seed, num_points, prm, stream);
  }
  bool addMorePointsToOtherFrameResident(int new_keyframe_id, const double T_newkey_from_cur[12], int first_point_id, uint64_t seed, int32_t num_points[3],
                                         const svs_seed_params *prm = nullptr, int stream = 0) {
    return seedResident_(SVS_SEED_MORE, new_keyframe_id, T_newkey_from_cur, first_point_id, seed, num_points, prm, stream);
  }
  // addNewKeyframe's remove_if over every list of the map (:360-365), from the records the step left on the device; behind processFrame, before the next list is set
  bool pruneNewpoints(int32_t *n_removed = nullptr, int stream = 0) {
    const int32_t st = stream;
    int32_t removed = 0;
    if (!ctx_.check(svs_frontend_newpoints_prune(fe_, 1, &st, &removed, nullptr))) return false;
    if (n_removed) *n_removed = removed;
    return true;
  }
  // ... of the named streams of a batch front end in one launch (the streams whose step dropped); n_removed: one count per stream named
  bool pruneNewpoints(const std::vector<int32_t> &streams, std::vector<int32_t> *n_removed) {
    std::vector<int32_t> removed(streams.size() ? streams.size() : 1);
    if (!ctx_.check(svs_frontend_newpoints_prune(fe_, (int)streams.size(), streams.data(), removed.data(), nullptr))) return false;
    removed.resize(streams.size());
    if (n_removed) *n_removed = removed;
    return true;
  }
  bool dropNewpointGroups(const std::vector<int32_t> &keyframe_ids, int32_t *n_found = nullptr, int stream = 0) {
    svs_newpoints_drop_request q;
    std::memset(&q, 0, sizeof q);
    q.stream = stream; q.n_keys = (int32_t)keyframe_ids.size(); q.h_keys = keyframe_ids.data();
    int32_t found = 0;
    if (!ctx_.check(svs_frontend_newpoints_drop_groups(fe_, 1, &q, &found))) return false;
    if (n_found) *n_found = found;
    return true;
  }
  // the store read back: the lists' keyframe ids and lengths in store order, and (records != NULL) their records back to back
  bool newpoints(std::vector<int32_t> *keyframe_ids, std::vector<int32_t> *counts, std::vector<svs_candidate_point> *records = nullptr, int stream_index = 0) {
    const int32_t stream = stream_index;
    int32_t n_groups = 0;
    keyframe_ids->assign(SVS_NEWPOINTS_MAX_GROUPS, -1); counts->assign(SVS_NEWPOINTS_MAX_GROUPS, 0);
    if (records) records->resize((size_t)(record_cap_ > 0 ? record_cap_ : 1));
    if (!ctx_.check(svs_frontend_newpoints_get(fe_, 1, &stream, &n_groups, keyframe_ids->data(), counts->data(), records ? records->data() : nullptr))) return false;
    keyframe_ids->resize((size_t)n_groups); counts->resize((size_t)n_groups);
    size_t total = 0;
    for (size_t g = 0; g < counts->size(); ++g) total += (size_t)(*counts)[g];
    if (records) records->resize(total);
    return true;
  }
  // matchAndTrack's lists (:989-1029) with the head taken from the store: list_keyframe_ids = actkey_id, then its strength_to_neighbors in order; point_list =
  // neighborhood_->point_list; slot_keyframe_ids as in setCandidatesFromMap.  false: refused, or over capacity (res->over_capacity; the list is then as before)
  bool setCandidatesFromNewpoints(const std::vector<int32_t> &list_keyframe_ids, const std::vector<int32_t> &slot_keyframe_ids,
                                  const std::vector<svs_candidate_point> &point_list, svs_newpoints_list_result *res = nullptr, int stream = 0) {
    if ((int)slot_keyframe_ids.size() != max_keyframes_) return false;
    svs_newpoints_list_request q;
    std::memset(&q, 0, sizeof q);
    q.stream = stream; q.n_keys = (int32_t)list_keyframe_ids.size(); q.n_tail = (int32_t)point_list.size();
    q.h_keys = list_keyframe_ids.data(); q.h_slot_kf = slot_keyframe_ids.data(); q.h_tail = point_list.data();
    svs_newpoints_list_result r;
    std::memset(&r, 0, sizeof r);
    const bool ok = ctx_.check(svs_frontend_set_candidates_from_newpoints(fe_, 1, &q, &r, nullptr, nullptr));
    if (res) *res = r;
    if (ok && !r.over_capacity && stream == 0) n_ = r.n_points;
    return ok && !r.over_capacity;
  }
  // setNeighborhoodFromMap with the head taken from the stream's store (svs_frontend_set_neighborhood_from_store): newpoint_map[actkey_id] is the fixed group, every
  // other list of the store a keyed one; no new-point record goes up.  Defined behind BackendMap
  inline bool setNeighborhoodFromStore(BackendMap &map, int32_t root_id, int32_t actkey_id, const std::vector<int32_t> &slot_keyframe_ids, bool refresh_poses,
                                       svs_nbr_result *res, std::vector<int32_t> *point_ids, std::vector<FrontendVertex> *vertex_map,
                                       std::vector<int32_t> *act_neighbors, int max_num_neighbors = 10, int vertex_cap = 64, int stream = 0);
  // addNewKeyframe's hand-over to the back end (stereo_frontend.cpp:316-415) for a stream whose decision is SVS_KF_DROP, as ONE call (svs_frontend_commit_keyframe):
  // the keyframe kept in `slot` enters the map as newkey_id with the lists where decideKeyframes left them on the device, the step's refined T_cur_from_actkey
  // as T_newkey_from_oldkey and the detector's thresholds as cell_grid2d; no list record reaches the host.  dec: the stream's decision record (its n_new /
  // n_track size the outputs); frame.d_disp / disp_stride: the keyframe's level-0 disparity, which like the slot stays alive while the map names it
  // (frame.cell_grid2d is not read).  One-stream and batch front ends alike (stream).  Defined behind BackendMap
  inline bool addNewKeyframeToMap(BackendMap &map, int slot, int newkey_id, int oldkey_id, const svs_keyframe_decision &dec, const float *d_disp, int disp_stride,
                                  int covis_thr, const svs_cam &cam, MapAddKeyframeResult *out, const std::vector<int32_t> &cached_ids = std::vector<int32_t>(),
                                  const std::vector<double> &cached_T12 = std::vector<double>(), int missing_cap = 64, int stream = 0);
  svs_frontend *handle() const { return fe_; }

 private:
  bool seedResident_(int mode, int kf, const double *T, int first_point_id, uint64_t seed, int32_t num_points[3], const svs_seed_params *prm, int stream) {
    const svs_seed_params p = prm ? *prm : seedParams();
    svs_seed_request q;
    std::memset(&q, 0, sizeof q);
    q.stream = stream; q.mode = mode; q.kf_index = kf; q.first_point_id = first_point_id; q.seed = seed;
    for (int i = 0; i < 12; ++i) q.T_newkey_from_cur[i] = T ? T[i] : (i % 5 == 0 ? 1.0 : 0.0);
    const int32_t key = kf;
    int32_t n[3] = {0, 0, 0};
    if (!ctx_.check(svs_frontend_seed_newpoints(fe_, 1, &q, &key, &p, n, nullptr, 0))) return false;
    for (int l = 0; l < 3; ++l) num_points[l] += n[l];
    return true;
  }
  bool seed_(int mode, int kf, const double *T, int first_point_id, uint64_t seed, std::vector<svs_candidate_point> *out, int32_t num_points[3],
             const svs_seed_params *prm) {
    const svs_seed_params p = prm ? *prm : seedParams();
    svs_seed_request q;
    std::memset(&q, 0, sizeof q);
    q.stream = 0; q.mode = mode; q.kf_index = kf; q.first_point_id = first_point_id; q.seed = seed;
    for (int i = 0; i < 12; ++i) q.T_newkey_from_cur[i] = T ? T[i] : (i % 5 == 0 ? 1.0 : 0.0);
    int cap = 0;
    for (int l = 0; l < p.n_levels; ++l) cap += (p.num_max_points >> l) + 1;
    out->resize((size_t)cap);
    int32_t n[3] = {0, 0, 0};
    if (!ctx_.check(svs_frontend_seed_keyframes(fe_, 1, &q, &p, out->data(), cap, n))) { out->clear(); return false; }
    out->resize((size_t)(n[0] + n[1] + n[2]));
    for (int l = 0; l < 3; ++l) num_points[l] += n[l];
    return true;
  }
  const Context &ctx_;
  svs_frontend *fe_;
  bool ok_;
  int n_ = 0;
  int max_points_, max_keyframes_;
  int record_cap_ = 0;
  int n_streams_ = 1;
};

// The per-pixel input conversions of FrameGrabber<StereoCamera> (frame_grabber.cpp:125-186, frame_grabber-impl.cpp:93-152) on device frames of n streams:
// intializeRectifier() builds the CV_16SC2 maps on the host the way the reference calls cv::initUndistortRectifyMap (R = SO3::exp(cam.rot*_left / _right),
// new camera matrix = the camera matrix for both sides); rectifyFrame() is cv::cvtColor + cv::remap; depthToDisp() the depth-camera case.
class FrameRectifier {
 public:
  FrameRectifier(const Context &c, const svs_cam &cam, int max_batch = 1) : ctx_(c), cam_(cam), max_batch_(max_batch), rect_(nullptr) {}
  ~FrameRectifier() { if (rect_) svs_rectify_destroy(rect_); }
  FrameRectifier(const FrameRectifier &) = delete;
  FrameRectifier &operator=(const FrameRectifier &) = delete;
  // SO3::exp of a rotation vector, row-major
  static void rodrigues(const double rv[3], double R[9]) {
    const double th2 = rv[0] * rv[0] + rv[1] * rv[1] + rv[2] * rv[2], th = std::sqrt(th2);
    const double A = th < 1e-12 ? 1.0 : std::sin(th) / th, B = th < 1e-12 ? 0.0 : (1.0 - std::cos(th)) / (th * th);
    const double Kx[9] = {0.0, -rv[2], rv[1], rv[2], 0.0, -rv[0], -rv[1], rv[0], 0.0};
    for (int r = 0; r < 3; ++r)
      for (int c = 0; c < 3; ++c) {
        double k2 = 0.0;
        for (int k = 0; k < 3; ++k) k2 += Kx[3 * r + k] * Kx[3 * k + c];
        R[3 * r + c] = (r == c ? 1.0 : 0.0) + A * Kx[3 * r + c] + B * k2;
      }
  }
  // rot_* : cam.rot{x,y,z}_left / _right; dist_* : cam.dist_left1..5 / cam.dist_right1..5 (k1, k2, p1, p2, k3).  with_right = false: a left image only
  // (framepipe.disp_img / depth_img)
  bool intializeRectifier(const double rot_left[3], const double dist_left[5], const double rot_right[3], const double dist_right[5], bool with_right = true) {
    const double K[9] = {cam_.f, 0.0, cam_.cx, 0.0, cam_.f, cam_.cy, 0.0, 0.0, 1.0};
    const size_t n = (size_t)cam_.w * cam_.h;
    std::vector<int16_t> xy[2];
    std::vector<uint16_t> fr[2];
    for (int s = 0; s < (with_right ? 2 : 1); ++s) {
      double R[9];
      rodrigues(s ? rot_right : rot_left, R);
      xy[s].resize(2 * n); fr[s].resize(n);
      if (!ctx_.check(svs_rectify_build_maps(K, s ? dist_right : dist_left, R, K, cam_.w, cam_.h, xy[s].data(), fr[s].data()))) return false;
    }
    return setMaps(xy[0].data(), fr[0].data(), with_right ? xy[1].data() : nullptr, with_right ? fr[1].data() : nullptr);
  }
  // maps made elsewhere (rect_map_left_[0] / [1], rect_map_right_[0] / [1] of a host that has OpenCV); NULL for a side: conversion / copy only
  bool setMaps(const int16_t *left_xy, const uint16_t *left_frac, const int16_t *right_xy, const uint16_t *right_frac) {
    if (rect_) { svs_rectify_destroy(rect_); rect_ = nullptr; }
    return ctx_.check(svs_rectify_create(ctx_.get(), cam_.w, cam_.h, max_batch_, left_xy, left_frac, right_xy, right_frac, &rect_));
  }
  // rectifyFrame() (+ the colour conversion of processNextFrame) into e.g. the buffers StereoFrontend's input view hands out; asynchronous
  bool rectifyFrame(const svs_raw_frames_dev &raw, uint8_t *d_left, int lstride, size_t l_bstride, uint8_t *d_right, int rstride, size_t r_bstride, int n_batch = 1) {
    return rect_ && ctx_.check(svs_rectify_frames(rect_, &raw, d_left, lstride, l_bstride, d_right, rstride, r_bstride, n_batch));
  }
  bool depthToDisp(const uint16_t *d_depth16, int stride, size_t bstride, float *d_disp, int dstride, size_t d_bstride, int n_batch = 1) const {
    return ctx_.check(svs_depth_to_disp(ctx_.get(), &cam_, d_depth16, stride, bstride, d_disp, dstride, d_bstride, n_batch));
  }

 private:
  const Context &ctx_;
  svs_cam cam_;
  int max_batch_;
  svs_rectify *rect_;
};

// placerecognizer.cpp:212-246 for a batch of keyframes: SurfFeatureDetector(600, 2).detect on the level-0 image, the disparity filter,
// SurfDescriptorExtractor(2, 4, 2, false).compute (svs_surf_extract; the header has the arithmetic and its departures from OpenCV).  The places stay on the
// device; the host copies are what Place::descriptors / uvu_0_vec hold.  A build without SURF (make SURF=0) reports !ok().
class SurfPlaces {
 public:
  SurfPlaces(const Context &c, const svs_cam &stereo_cam, int w, int h, int max_batch = 1, int max_keypoints = 2048, double surf_thr = 600)
      : ctx_(c), surf_(nullptr), w_(w), h_(h), max_batch_(max_batch), max_kp_(max_keypoints), n_(0), ok_(false) {
    svs_surf_params prm;
    svs_surf_params_default(&prm);
    prm.hessian_threshold = (float)surf_thr;
    ok_ = c.check(svs_surf_create(c.get(), &stereo_cam, w, h, max_batch, max_keypoints, &prm, &surf_));
  }
  ~SurfPlaces() { if (surf_) svs_surf_destroy(surf_); }
  SurfPlaces(const SurfPlaces &) = delete;
  SurfPlaces &operator=(const SurfPlaces &) = delete;
  bool ok() const { return ok_; }
  svs_surf *get() const { return surf_; }
  // device images (stride / bstride in bytes) and device disparity (dstride / d_bstride in floats) of n_batch keyframes.  Blocking
  bool addLocations(const uint8_t *d_img, int stride, size_t bstride, const float *d_disp, int dstride, size_t d_bstride, int n_batch) {
    n_ = 0;
    if (!ok_ || n_batch < 1 || n_batch > max_batch_) return false;
    count_.assign(n_batch, 0); overflow_.assign(n_batch, 0);
    kp_.resize((size_t)n_batch * max_kp_); uvu_.resize((size_t)n_batch * max_kp_ * 3); desc_.resize((size_t)n_batch * max_kp_ * 64);
    if (!ctx_.check(svs_surf_extract(surf_, d_img, stride, bstride, d_disp, dstride, d_bstride, n_batch, count_.data(), overflow_.data(), kp_.data(), uvu_.data(),
                                     desc_.data())))
      return false;
    n_ = n_batch;
    return true;
  }
  // one keyframe from host memory (keyframe.pyr.at(0), keyframe.disp), uploaded first: tools and tests; a tracker's images are on the device already
  bool addLocation(const uint8_t *image, const float *disp) {
    void *d_img = nullptr, *d_disp = nullptr;
    const size_t n = (size_t)w_ * h_;
    bool ok = ok_ && ctx_.check(svs_malloc(ctx_.get(), n, &d_img)) && ctx_.check(svs_malloc(ctx_.get(), n * sizeof(float), &d_disp)) &&
              ctx_.check(svs_memcpy_h2d(ctx_.get(), d_img, image, n)) && ctx_.check(svs_memcpy_h2d(ctx_.get(), d_disp, disp, n * sizeof(float))) &&
              ctx_.check(svs_ctx_sync(ctx_.get())) &&
              addLocations(static_cast<const uint8_t *>(d_img), w_, n, static_cast<const float *>(d_disp), w_, n, 1);
    if (d_img) svs_free(ctx_.get(), d_img);
    if (d_disp) svs_free(ctx_.get(), d_disp);
    return ok;
  }
  int size(int image = 0) const { return image >= 0 && image < n_ ? count_[image] : 0; }
  bool overflow(int image = 0) const { return image >= 0 && image < n_ && overflow_[image] != 0; }
  const svs_surf_keypoint *keypoints(int image = 0) const { return kp_.data() + (size_t)image * max_kp_; }
  const double *uvu_0_vec(int image = 0) const { return uvu_.data() + (size_t)image * max_kp_ * 3; }
  const float *descriptors(int image = 0) const { return desc_.data() + (size_t)image * max_kp_ * 64; }

 private:
  const Context &ctx_;
  svs_surf *surf_;
  int w_, h_, max_batch_, max_kp_, n_;
  bool ok_;
  std::vector<int32_t> count_, overflow_;
  std::vector<svs_surf_keypoint> kp_;
  std::vector<double> uvu_;
  std::vector<float> desc_;
};

// PlaceRecognizer (placerecognizer.cpp:175-322) on device-resident places: addPlace() is where addLocation hands a Place over (location_map_.insert, :299),
// setVocabulary() takes words_, addLocation() is addLocation from :248 onwards (visual words, inverted index, TF-IDF scores, the > 2 test, then the geometric
// check of the candidate), geometricCheck() is the BFMatcher + RanSaC<SE3Model>::compute(100, ...) pair and the inliers > 30 test.  Detection and description
// (surf.detect, the disparity filter, surf_ext.compute, :212-246) are SurfPlaces above; addPlaceFromSurf() hands its places over on the device.
struct DetectedLoop { int query_keyframe_id, loop_keyframe_id; double T_query_from_loop[12]; };      // T: [R | t] row-major
class PlaceRecognizerGeom {
 public:
  PlaceRecognizerGeom(const Context &c, const svs_cam &stereo_cam, int desc_dim = 64, int max_desc = 2048, int max_places = 64, int num_ransac = 100)
      : ctx_(c), loop_(nullptr), num_ransac_(num_ransac), pixel_thr_(2.5), seed_(0), keyframe_id_(max_places > 0 ? max_places : 0, -1) {
    std::memset(&last_, 0, sizeof last_);
    std::memset(&last_loc_, 0, sizeof last_loc_);
    ok_ = c.check(svs_loop_create(c.get(), &stereo_cam, desc_dim, max_desc, max_places, num_ransac, 1, &loop_));
  }
  ~PlaceRecognizerGeom() { if (loop_) svs_loop_destroy(loop_); }
  PlaceRecognizerGeom(const PlaceRecognizerGeom &) = delete;
  PlaceRecognizerGeom &operator=(const PlaceRecognizerGeom &) = delete;
  bool ok() const { return ok_; }
  svs_loop *get() const { return loop_; }
  // Place::descriptors [n][desc_dim], uvu_0_vec [n][3], xyz_vec [n][3] (NULL: cam.unmap_uvu on the device)
  bool addPlace(int slot, int keyframe_id, int n, const float *descriptors, const double *uvu_0_vec, const double *xyz_vec = nullptr) {
    if (!ok_ || !ctx_.check(svs_loop_set_place(loop_, slot, n, descriptors, uvu_0_vec, xyz_vec))) return false;
    keyframe_id_[slot] = keyframe_id;
    return true;
  }
  // the place of image `image` of surf's last addLocation(s), device to device (svs_loop_set_place_from_surf): bit-identical to addPlace on its host copies
  bool addPlaceFromSurf(int slot, int keyframe_id, const SurfPlaces &surf, int image = 0) {
    if (!ok_ || !ctx_.check(svs_loop_set_place_from_surf(loop_, slot, surf.get(), image))) return false;
    keyframe_id_[slot] = keyframe_id;
    return true;
  }
  void setSeed(uint64_t seed) { seed_ = seed; }
  void setPixelThreshold(double thr) { pixel_thr_ = thr; }
  // true when inliers.size() > 30: *loop is what monitor.addLoop() takes
  bool geometricCheck(int query_slot, int train_slot, DetectedLoop *loop) {
    svs_loop_check ck;
    ck.query_slot = query_slot; ck.train_slot = train_slot; ck.n_hyp = num_ransac_; ck.pixel_thr = pixel_thr_; ck.seed = seed_++; ck.h_samples = nullptr;
    if (!ok_ || !ctx_.check(svs_loop_check_batch(loop_, 1, &ck, &last_, nullptr, nullptr, nullptr, nullptr, nullptr))) return false;
    if (loop) {
      loop->query_keyframe_id = keyframe_id_[query_slot];
      loop->loop_keyframe_id = keyframe_id_[train_slot];
      std::memcpy(loop->T_query_from_loop, last_.T_query_from_train, sizeof last_.T_query_from_train);
    }
    return last_.n_inliers > 30;
  }
  const svs_loop_result &lastResult() const { return last_; }
  // words_ [n_words][desc_dim] (the rows of surfwords10000.png); the index starts empty
  bool setVocabulary(int n_words, const float *words) { return ok_ && ctx_.check(svs_loop_set_vocabulary(loop_, n_words, words)); }
  // addLocation from :248 onwards for the place loaded into `slot` with addPlace: words, scores against every earlier location outside exclude_slots, insertion;
  // when the best score passes 2, geometricCheck(slot, best).  true when a loop was detected; *loop as for geometricCheck.  error() tells a refused call
  // from "no loop"
  bool addLocation(int slot, int keyframe_id, bool do_loop_detection, const int *exclude_slots, int n_exclude, DetectedLoop *loop) {
    svs_loop_location lc;
    std::vector<int32_t> ex(exclude_slots, exclude_slots + (n_exclude > 0 ? n_exclude : 0));
    lc.slot = slot; lc.do_loop_detection = do_loop_detection ? 1 : 0; lc.h_exclude = ex.empty() ? nullptr : ex.data(); lc.n_exclude = (int32_t)ex.size();
    lc.radius = 0.1f; lc.min_score = 2.0f;
    error_ = !ok_ || !ctx_.check(svs_loop_add_locations(loop_, 1, &lc, &last_loc_, nullptr, nullptr, nullptr));
    if (error_) return false;
    keyframe_id_[slot] = keyframe_id;
    return last_loc_.candidate && geometricCheck(slot, last_loc_.best_slot, loop);
  }
  const svs_loop_location_result &lastLocation() const { return last_loc_; }
  bool error() const { return error_; }

 private:
  const Context &ctx_;
  svs_loop *loop_;
  int num_ransac_;
  double pixel_thr_;
  uint64_t seed_;
  std::vector<int> keyframe_id_;
  svs_loop_result last_;
  svs_loop_location_result last_loc_;
  bool ok_, error_ = false;
};

// calculateWordsAndSaveThem of the reference's dictionary program (create_dictionary.cpp:144-177) without the file: descriptors in, words_ out -- what
// PlaceRecognizerGeom::setVocabulary takes.  Flat Lloyd iterations with k-means++ seeding on the device (svs_vocab_train) where the reference cuts a 32-ary
// k-means tree; the asked number of words comes back unless words end up without members (or the points run out of distinct rows).
class VocabularyTrainer {
 public:
  explicit VocabularyTrainer(const Context &c, int desc_dim = 64) : ctx_(c), desc_dim_(desc_dim) {
    svs_vocab_params_default(&prm_);
    std::memset(&last_, 0, sizeof last_);
  }
  void setIterations(int iterations) { prm_.iterations = iterations; }      // 11 (create_dictionary.cpp:150)
  void setSeed(uint64_t seed) { prm_.seed = seed; }
  void setDropEmpty(bool drop) { prm_.drop_empty = drop ? 1 : 0; }
  // descriptors [n][desc_dim]; *words becomes [lastResult().n_words_out][desc_dim].  false: refused (Context::check has the reason)
  bool createDictionary(int n, const float *descriptors, int target_num_words, std::vector<float> *words, std::vector<int32_t> *assignment = nullptr) {
    if (!words || target_num_words < 1) return false;
    prm_.n_words = target_num_words;
    words->assign((size_t)target_num_words * desc_dim_, 0.f);
    if (assignment) assignment->assign((size_t)(n > 0 ? n : 0), -1);
    if (!ctx_.check(svs_vocab_train(ctx_.get(), desc_dim_, n, descriptors, &prm_, words->data(), &last_, nullptr, assignment ? assignment->data() : nullptr, nullptr,
                                    nullptr, nullptr)))
      return false;
    words->resize((size_t)last_.n_words_out * desc_dim_);
    return true;
  }
  const svs_vocab_result &lastResult() const { return last_; }

 private:
  const Context &ctx_;
  int desc_dim_;
  svs_vocab_params prm_;
  svs_vocab_result last_;
};

// Backend::localRegisterFrame (backend.cpp:549-611) and Backend::globalLoopClosure (:830-1001) from the pose-graph walk onwards: the caller flattens the
// reference's containers -- the candidate keyframes (larger_neighborhood + the anchors' vertices) into a table, the deduplicated point walk of pointsVisibleInRoot
// (:480-498) / v_query.feature_table (:853) into a list whose kf_index names the anchor's table entry, the feature_table membership into observer rows -- and gets
// back what registerKeyframes / addLoopClosure take.  One blocking call each; the cull, FastGrid::detect, both matches and refinements, the gate and the counting
// run on the device in between.
struct RegistrationFrame {               // the root keyframe (root_frame / loop_frame) as the call needs it
  int table_entry;                       // its entry of the keyframe table: that entry's device pyramid is the frame matched into
  const float *d_disp; int disp_stride;  // its disparity, DEVICE
  std::vector<int32_t> cell_grid2d[SVS_NUM_PYR_LEVELS];      // root_frame.cell_grid2d: the stored FAST thresholds per level
  double T_from_world[12];               // v_root.T_me_from_world / T_loop_from_world (:845)
};
struct RegistrationKeyframe {            // one candidate keyframe: keyframe_map_ entry + vertex pose + its sets
  int frame_id;
  svs_keyframe kf;
  bool in_double_window;                 // IS_IN_SET(frame_id, graph_.double_window())
  bool direct_neighbor;                  // IS_IN_SET(frame_id, directNeighborsOf(root)) (:433-449)
};
struct TrackPoint { int global_id; double uvu[3]; int anchor_level; };      // StereoGraph::MyTrackPoint: point id + ImageFeature<3>(uvu, anchor_level)

// The back end's map kept on the device for re-registration (svs_map_*): the vertex_table's poses and frames, the point_table, and every feature_table as
// (point, keyframe) pairs, under the graph's own ids.  The back-end thread feeds it as the graph grows -- addKeyframes / addPoints / addObservations from
// addKeyframeToGraph, setPoses / setPoints from the restoreDataFromG2o walk, setWindow from graph_.double_window() -- and BackendRegistration::registerFrames
// names a registration by ids.  Every update is one staged upload, asynchronous on the context's stream; false = refused as a whole (Context::lastError).
class BackendMap {
 public:
  BackendMap(const Context &c, int max_keyframes = 4096, int max_points = 1 << 20, int max_observations = 1 << 22) : ctx_(c), map_(nullptr) {
    ok_ = c.check(svs_map_create(c.get(), max_keyframes, max_points, max_observations, &map_));
    if (ok_) level_.assign((size_t)max_points, 0);
  }
  ~BackendMap() { if (map_) svs_map_destroy(map_); }
  BackendMap(const BackendMap &) = delete;
  BackendMap &operator=(const BackendMap &) = delete;
  bool ok() const { return ok_; }
  svs_map *get() const { return map_; }
  // keyframes[i].kf: T_me_from_world and the device pyramid; frames[i]: d_disp / disp_stride / cell_grid2d are read (table_entry and T_from_world are not)
  bool addKeyframes(const std::vector<RegistrationKeyframe> &keyframes, const std::vector<RegistrationFrame> &frames) {
    const size_t n = keyframes.size();
    if (!ok_ || frames.size() != n) return false;
    std::vector<int32_t> ids(n), stride(n), thr(n * SVS_NUM_PYR_LEVELS * SVS_MAX_CELLS, 25);
    std::vector<svs_keyframe> kfs(n);
    std::vector<const float *> disp(n);
    for (size_t i = 0; i < n; ++i) {
      ids[i] = keyframes[i].frame_id; kfs[i] = keyframes[i].kf; disp[i] = frames[i].d_disp; stride[i] = frames[i].disp_stride;
      for (int l = 0; l < SVS_NUM_PYR_LEVELS; ++l)
        for (size_t c = 0; c < frames[i].cell_grid2d[l].size() && c < SVS_MAX_CELLS; ++c) thr[(i * SVS_NUM_PYR_LEVELS + l) * SVS_MAX_CELLS + c] = frames[i].cell_grid2d[l][c];
    }
    if (!ctx_.check(svs_map_add_keyframes(map_, (int)n, ids.data(), kfs.data(), disp.data(), stride.data(), thr.data()))) return false;
    return true;      // (in_double_window is not read: the window is set as a whole, setWindow)
  }
  // points[i].point_id: the id; points[i].kf_index: the ID of the anchor keyframe (p.anchorframe_id)
  bool addPoints(const std::vector<svs_candidate_point> &points) {
    if (!ok_) return false;
    std::vector<int32_t> ids(points.size());
    for (size_t i = 0; i < points.size(); ++i) ids[i] = points[i].point_id;
    if (!ctx_.check(svs_map_add_points(map_, (int)points.size(), ids.data(), points.data()))) return false;
    for (size_t i = 0; i < points.size(); ++i) level_[(size_t)ids[i]] = (int8_t)points[i].anchor_level;
    return true;
  }
  // v.feature_table of keyframe kf_ids[i] holds point point_ids[i]
  bool addObservations(const std::vector<int32_t> &point_ids, const std::vector<int32_t> &kf_ids) {
    return ok_ && point_ids.size() == kf_ids.size() && ctx_.check(svs_map_add_observations(map_, (int)point_ids.size(), point_ids.data(), kf_ids.data()));
  }
  // the same with the ImageFeature of each pair (feat.center [n][3], feat.level): what a caller hands over that also optimises through the map
  // (SlamGraphBA::copyDataFromMap); a map fed this way only can form a window
  bool addObservations(const std::vector<int32_t> &point_ids, const std::vector<int32_t> &kf_ids, const std::vector<double> &center3, const std::vector<int32_t> &level) {
    return ok_ && point_ids.size() == kf_ids.size() && center3.size() == 3 * point_ids.size() && level.size() == point_ids.size() &&
           ctx_.check(svs_map_add_measured_observations(map_, (int)point_ids.size(), point_ids.data(), kf_ids.data(), center3.data(), level.data()));
  }
  // computeActivePointsAndExtendOuterWindow (slam_graph.cpp:599-663) on the device, behind the caller's computeInitialDoubleWin: window / types (0 INNER, 1 OUTER)
  // are double_window_ before the extension, edge_pairs (id, id, ...) the edge_table_ entries with an end in an INNER keyframe.  On return window and types hold
  // the final window (W0, then the extension ascending and OUTER) and the map's window flags name exactly it; *n_active: the active points.  false: refused, or
  // the final window exceeds 256 keyframes (window and types are left as they were)
  bool prepareForOptimization(std::vector<int32_t> *window, std::vector<int32_t> *types, const std::vector<int32_t> &edge_pairs, int *n_active = nullptr) {
    if (!ok_ || window->size() != types->size() || edge_pairs.size() % 2) return false;
    svs_map_window_result r;
    std::vector<int32_t> ids(256), ty(256);
    if (!ctx_.check(svs_map_prepare_window(map_, (int)window->size(), window->data(), types->data(), (int)(edge_pairs.size() / 2), edge_pairs.data(), 1, 256, &r,
                                           ids.data(), ty.data()))) return false;
    if (r.n_active < 0) return false;
    window->assign(ids.begin(), ids.begin() + r.n_window); types->assign(ty.begin(), ty.begin() + r.n_window);
    if (n_active) *n_active = r.n_active;
    return true;
  }
  bool setPoses(const std::vector<int32_t> &kf_ids, const std::vector<double> &poses12) {
    return ok_ && poses12.size() == 12 * kf_ids.size() && ctx_.check(svs_map_set_poses(map_, (int)kf_ids.size(), kf_ids.data(), poses12.data()));
  }
  bool setPoints(const std::vector<int32_t> &point_ids, const std::vector<double> &xyz_anchor3) {
    return ok_ && xyz_anchor3.size() == 3 * point_ids.size() && ctx_.check(svs_map_set_points(map_, (int)point_ids.size(), point_ids.data(), xyz_anchor3.data()));
  }
  bool setWindow(const std::vector<int32_t> &kf_ids) { return ok_ && ctx_.check(svs_map_set_window(map_, (int)kf_ids.size(), kf_ids.data())); }
  // ---- the pose graph's edges (EdgeTable) and their constraints (computeConstraint, slam_graph.cpp:787-846) on the device ----
  bool reserveEdges(int max_edges) { return ok_ && ctx_.check(svs_map_reserve_edges(map_, max_edges)); }
  // insertEdge: pairs (id, id, ...), either orientation; edge_type 0 LOCAL, 1 METRIC, 2 APPEARANCE
  bool addEdges(const std::vector<int32_t> &pairs, const std::vector<int32_t> &strength, const std::vector<int32_t> &edge_type) {
    const size_t n = pairs.size() / 2;
    if (!ok_ || pairs.size() % 2 || strength.size() != n || edge_type.size() != n) return false;
    if (!ctx_.check(svs_map_add_edges(map_, (int)n, pairs.data(), strength.data(), edge_type.data()))) return false;
    for (size_t i = 0; i < n; ++i) edge_keys_.push_back(std::make_pair(std::min(pairs[2 * i], pairs[2 * i + 1]), std::max(pairs[2 * i], pairs[2 * i + 1])));
    std::sort(edge_keys_.begin(), edge_keys_.end());
    return true;
  }
  // computeConstraint for a batch (one blocking call); missing: the anchors some request has neither in the window nor among its cached poses, ascending, each
  // once (at most missing_cap per request) -- the caller's computeAbsolutePose completes them and the call is repeated
  bool computeConstraints(const std::vector<svs_map_constraint_request> &requests, std::vector<svs_map_constraint_result> *results,
                          std::vector<int32_t> *missing = nullptr, int missing_cap = 64) {
    if (!ok_ || !results || missing_cap < 1) return false;
    results->resize(requests.size());
    if (requests.empty()) { if (missing) missing->clear(); return true; }      // (nothing to ask: an empty vector has no data() to pass)
    std::vector<int32_t> miss(requests.size() * (size_t)missing_cap, -1);
    if (!ctx_.check(svs_map_compute_constraints(map_, (int)requests.size(), requests.data(), missing_cap, results->data(), miss.data(), 0, nullptr))) return false;
    if (missing) {
      missing->clear();
      for (size_t i = 0; i < miss.size(); ++i) if (miss[i] >= 0) missing->push_back(miss[i]);
      std::sort(missing->begin(), missing->end());
      missing->erase(std::unique(missing->begin(), missing->end()), missing->end());
    }
    return true;
  }
  // unmargPosesEnteringInnerW (:728-759) and margPosesLeftInnerWindow (:848-904): the pairs are selected here from the edge keys and the two windows (ids, types
  // 0 INNER / 1 OUTER), then one svs_map_unmarginalize and one storing computeConstraints with kf1 the smaller id.  The map's window flags must be those of the
  // new window.  cached_ids (ascending) / cached_T12: the caller's computeAbsolutePose results, given to every request
  bool updateMarginalization(const std::vector<int32_t> &old_ids, const std::vector<int32_t> &old_types, const std::vector<int32_t> &new_ids,
                             const std::vector<int32_t> &new_types, const std::vector<int32_t> &cached_ids, const std::vector<double> &cached_T12,
                             std::vector<svs_map_constraint_result> *results, std::vector<int32_t> *missing) {
    if (!ok_ || old_ids.size() != old_types.size() || new_ids.size() != new_types.size() || cached_T12.size() != 12 * cached_ids.size()) return false;
    std::vector<int32_t> enter, left;
    innerPairs(new_ids, new_types, &enter);
    innerPairs(old_ids, old_types, &left);
    std::vector<svs_map_constraint_request> req;
    for (size_t k = 0; k + 1 < left.size(); k += 2) {
      if (innerIn(new_ids, new_types, left[k]) && innerIn(new_ids, new_types, left[k + 1])) continue;
      svs_map_constraint_request q;
      std::memset(&q, 0, sizeof q);
      q.kf1 = left[k]; q.kf2 = left[k + 1]; q.store = 1; q.n_cached = (int32_t)cached_ids.size();
      q.cached_ids = cached_ids.empty() ? nullptr : cached_ids.data(); q.cached_T = cached_T12.empty() ? nullptr : cached_T12.data();
      req.push_back(q);
    }
    if (!enter.empty() && !ctx_.check(svs_map_unmarginalize(map_, (int)(enter.size() / 2), enter.data()))) return false;
    std::vector<svs_map_constraint_result> local;
    return computeConstraints(req, results ? results : &local, missing);
  }
  // ---- the pose graph's walks on the device (svs_map_initial_windows .. svs_map_prepare_window_from_root): ids come in the visit order of the reference's queue
  bool computeInitialDoubleWin(int root_id, int inner_window_size, int double_window_size, std::vector<int32_t> *window, std::vector<int32_t> *types) {
    if (!ok_ || !window || !types || double_window_size < 1) return false;
    int32_t root = root_id, count = 0;
    std::vector<int32_t> ids((size_t)double_window_size), ty((size_t)double_window_size);
    if (!ctx_.check(svs_map_initial_windows(map_, 1, &root, inner_window_size, double_window_size, double_window_size, &count, ids.data(), ty.data()))) return false;
    window->assign(ids.begin(), ids.begin() + count); types->assign(ty.begin(), ty.begin() + count);
    return true;
  }
  bool framesInNeighborhood(int root_id, int size_of_neighborhood, std::vector<int32_t> *ids) {
    if (!ok_ || !ids || size_of_neighborhood < 1) return false;
    int32_t root = root_id, count = 0;
    std::vector<int32_t> out((size_t)size_of_neighborhood);
    if (!ctx_.check(svs_map_frames_in_neighborhood(map_, 1, &root, size_of_neighborhood, &count, out.data()))) return false;
    ids->assign(out.begin(), out.begin() + count);
    return true;
  }
  // computeAbsolutePose for a batch: T12 [n][12], status SVS_WALK_OK / SVS_WALK_NO_PATH (T zero) per id; at most SVS_MAP_WALK_MAX_REQUESTS ids per device call
  bool computeAbsolutePoses(const std::vector<int32_t> &kf_ids, std::vector<double> *T12, std::vector<int32_t> *status) {
    if (!ok_ || !T12 || !status) return false;
    T12->assign(12 * kf_ids.size(), 0.0); status->assign(kf_ids.size(), SVS_WALK_NO_PATH);
    for (size_t at = 0; at < kf_ids.size(); at += SVS_MAP_WALK_MAX_REQUESTS) {
      const int n = (int)std::min(kf_ids.size() - at, (size_t)SVS_MAP_WALK_MAX_REQUESTS);
      if (!ctx_.check(svs_map_absolute_poses(map_, n, kf_ids.data() + at, 0, status->data() + at, nullptr, T12->data() + 12 * at, nullptr))) return false;
    }
    return true;
  }
  // false also where no path leads to the window (the reference asserts)
  bool computeAbsolutePose(int x_id, double T_x_from_w[12]) {
    std::vector<double> T; std::vector<int32_t> st;
    if (!computeAbsolutePoses(std::vector<int32_t>(1, x_id), &T, &st) || st[0] != SVS_WALK_OK) return false;
    std::copy(T.begin(), T.end(), T_x_from_w);
    return true;
  }
  // reinitializePoses over the keyframes of the map's window; changed (optional): the ids whose pose was rewritten, in visit order
  bool reinitializePoses(int root_id, const std::vector<int32_t> &old_window, int loop_id, std::vector<int32_t> *changed = nullptr) {
    if (!ok_) return false;
    int32_t n_kf = 0, n_changed = 0;
    if (!ctx_.check(svs_map_info(map_, &n_kf, nullptr, nullptr))) return false;
    std::vector<int32_t> out((size_t)std::max(n_kf, 1));
    if (!ctx_.check(svs_map_reinitialize_poses(map_, root_id, loop_id, (int)old_window.size(), old_window.empty() ? nullptr : old_window.data(), n_kf, &n_changed,
                                               out.data()))) return false;
    if (changed) changed->assign(out.begin(), out.begin() + std::min(n_changed, n_kf));
    return true;
  }
  void setWindowSizes(int inner_window_size, int double_window_size) { inner_size_ = inner_window_size; double_size_ = double_window_size; }
  // SlamGraph::prepareForOptimization (:288-310) from the root alone: the window from the root on the device, reinitializePoses against the window this object
  // prepared last, then updateMarginalization, whose missing anchors computeAbsolutePoses answers until none that has a path is left.  window / types: the final
  // window.  false: refused, the final window exceeds 256 keyframes, or it holds fewer than two (:303)
  bool prepareForOptimization(int root_id, int loop_id, std::vector<int32_t> *window, std::vector<int32_t> *types, int *n_active = nullptr,
                              std::vector<svs_map_constraint_result> *results = nullptr, std::vector<int32_t> *missing = nullptr) {
    if (!ok_ || !window || !types) return false;
    svs_map_window_result r;
    std::vector<int32_t> ids(256), ty(256);
    if (!ctx_.check(svs_map_prepare_window_from_root(map_, root_id, inner_size_, double_size_, 1, 256, &r, ids.data(), ty.data()))) return false;
    if (r.n_active < 0) return false;
    ids.resize((size_t)r.n_window); ty.resize((size_t)r.n_window);
    if (n_active) *n_active = r.n_active;
    const std::vector<int32_t> old_ids = window_ids_, old_types = window_types_;
    window_ids_ = ids; window_types_ = ty;
    *window = ids; *types = ty;
    if (!reinitializePoses(root_id, old_ids, loop_id)) return false;
    if (ids.size() < 2) return false;
    std::vector<int32_t> cached_ids, miss;
    std::vector<double> cached_T;
    for (;;) {
      if (!updateMarginalization(old_ids, old_types, ids, ty, cached_ids, cached_T, results, &miss)) return false;
      std::vector<double> T; std::vector<int32_t> st;
      if (miss.empty() || !computeAbsolutePoses(miss, &T, &st)) break;
      std::vector<std::pair<int32_t, size_t> > all;      // (id, where its pose lies: cached_T below `old`, T above)
      const size_t old = cached_ids.size();
      for (size_t i = 0; i < old; ++i) all.push_back(std::make_pair(cached_ids[i], i));
      for (size_t i = 0; i < miss.size(); ++i) if (st[i] == SVS_WALK_OK) all.push_back(std::make_pair(miss[i], old + i));
      if (all.size() == old) break;                      // no path for any of them: the caller sees them in `missing`
      std::sort(all.begin(), all.end());
      std::vector<int32_t> nid; std::vector<double> nT;
      for (size_t i = 0; i < all.size(); ++i) {
        const double *src = all[i].second < old ? &cached_T[12 * all[i].second] : &T[12 * (all[i].second - old)];
        nid.push_back(all[i].first); nT.insert(nT.end(), src, src + 12);
      }
      cached_ids.swap(nid); cached_T.swap(nT);
    }
    if (missing) *missing = miss;
    return true;
  }
  // ---- SlamGraph::addFirstKeyframe / addKeyframe (slam_graph.cpp:255-268, :143-186) on the device: svs_map_add_first_keyframe / svs_map_add_keyframe ----
  // keyframe.kf: the device pyramid (its pose is ignored: identity); frame: d_disp / disp_stride / cell_grid2d
  bool addFirstKeyframe(const RegistrationKeyframe &keyframe, const RegistrationFrame &frame) {
    if (!ok_) return false;
    std::vector<int32_t> thr;
    thresholds(frame, &thr);
    return ctx_.check(svs_map_add_first_keyframe(map_, keyframe.frame_id, &keyframe.kf, frame.d_disp, frame.disp_stride, thr.data()));
  }
  typedef MapAddKeyframeResult AddKeyframeResult;
  // newkey.kf: the device pyramid (its pose is ignored: T_newkey_from_oldkey * T_oldkey_from_world is formed on the device); covis_thr = graph_.covis_thr(),
  // cam: the level-0 camera (half sizes as computeStrength takes them, :480-481).  cached_ids (ascending) / cached_T12: the caller's computeAbsolutePose
  // results.  false: refused as a whole (Context::error); out->over_capacity: more than SVS_MAP_ADDKF_MAX_NEIGHBORS keys, the map unchanged
  bool addKeyframe(int oldkey_id, const RegistrationKeyframe &newkey, const RegistrationFrame &frame, const double T_newkey_from_oldkey[12],
                   const std::vector<svs_map_new_point> &newpoint_list, const std::vector<svs_map_track_point> &trackpoint_list, int covis_thr, const svs_cam &cam,
                   AddKeyframeResult *out, const std::vector<int32_t> &cached_ids = std::vector<int32_t>(), const std::vector<double> &cached_T12 = std::vector<double>(),
                   int missing_cap = 64) {
    if (!ok_ || !out || cached_T12.size() != 12 * cached_ids.size() || missing_cap < 1) return false;
    std::vector<int32_t> thr;
    thresholds(frame, &thr);
    svs_map_add_keyframe_args a;
    std::memset(&a, 0, sizeof a);
    a.newkey_id = newkey.frame_id; a.oldkey_id = oldkey_id; a.covis_thr = covis_thr; a.half_width = (int)(cam.w * 0.5); a.half_height = (int)(cam.h * 0.5);
    a.disp_stride = frame.disp_stride; a.n_new = (int32_t)newpoint_list.size(); a.n_track = (int32_t)trackpoint_list.size();
    std::memcpy(a.T_newkey_from_oldkey, T_newkey_from_oldkey, sizeof a.T_newkey_from_oldkey);
    a.keyframe = newkey.kf; a.disp = frame.d_disp; a.fast_thr = thr.data();
    a.new_points = newpoint_list.empty() ? nullptr : newpoint_list.data(); a.track_points = trackpoint_list.empty() ? nullptr : trackpoint_list.data();
    a.n_cached = (int32_t)cached_ids.size(); a.cached_ids = cached_ids.empty() ? nullptr : cached_ids.data(); a.cached_T = cached_T12.empty() ? nullptr : cached_T12.data();
    svs_map_strength_result r;
    int32_t n_kf = 0;
    if (!ctx_.check(svs_map_info(map_, &n_kf, nullptr, nullptr))) return false;
    const size_t edge_cap = (size_t)std::max(1, std::min((int)n_kf, (int)SVS_MAP_ADDKF_MAX_NEIGHBORS));      // every key is a keyframe of the map
    std::vector<svs_map_key> keys(SVS_MAP_ADDKF_MAX_NEIGHBORS);
    std::vector<int32_t> kept(newpoint_list.size() + 1), exists(trackpoint_list.size() + 1), miss(edge_cap * missing_cap, -1);
    std::vector<svs_map_constraint_result> cons(edge_cap);
    if (!ctx_.check(svs_map_add_keyframe(map_, &a, missing_cap, &r, keys.data(), kept.data(), exists.data(), cons.data(), miss.data()))) return false;
    addKeyframeResult_(r, keys, kept, exists, cons, miss, newpoint_list.size(), trackpoint_list.size(), newkey.frame_id, n_kf, missing_cap, out);
    for (size_t i = 0; !out->over_capacity && i < newpoint_list.size(); ++i) if (kept[i]) level_[(size_t)newpoint_list[i].point_id] = (int8_t)newpoint_list[i].anchor_level;
    return true;
  }
  // addKeyframe with the two lists in DEVICE memory of the map's context (svs_map_add_keyframe_dev): d_newpoint_list [n_new], d_trackpoint_list [n_track], complete
  // on the context's stream.  No list record crosses the bus and every refusal about the records is decided on the device; *out is what the call above gives.
  // The records never reach this object: anchorLevel() of a point inserted this way reads 0 until setAnchorLevel tells it
  bool addKeyframe(int oldkey_id, const RegistrationKeyframe &newkey, const RegistrationFrame &frame, const double T_newkey_from_oldkey[12],
                   const svs_map_new_point *d_newpoint_list, int n_new, const svs_map_track_point *d_trackpoint_list, int n_track, int covis_thr, const svs_cam &cam,
                   AddKeyframeResult *out, const std::vector<int32_t> &cached_ids = std::vector<int32_t>(), const std::vector<double> &cached_T12 = std::vector<double>(),
                   int missing_cap = 64) {
    if (!ok_ || !out || n_new < 0 || n_track < 0 || cached_T12.size() != 12 * cached_ids.size() || missing_cap < 1) return false;
    std::vector<int32_t> thr;
    thresholds(frame, &thr);
    svs_map_add_keyframe_args a;
    std::memset(&a, 0, sizeof a);
    a.newkey_id = newkey.frame_id; a.oldkey_id = oldkey_id; a.covis_thr = covis_thr; a.half_width = (int)(cam.w * 0.5); a.half_height = (int)(cam.h * 0.5);
    a.disp_stride = frame.disp_stride; a.n_new = n_new; a.n_track = n_track;
    std::memcpy(a.T_newkey_from_oldkey, T_newkey_from_oldkey, sizeof a.T_newkey_from_oldkey);
    a.keyframe = newkey.kf; a.disp = frame.d_disp; a.fast_thr = thr.data();
    a.n_cached = (int32_t)cached_ids.size(); a.cached_ids = cached_ids.empty() ? nullptr : cached_ids.data(); a.cached_T = cached_T12.empty() ? nullptr : cached_T12.data();
    AddKeyframeCall_ c(this, (size_t)n_new, (size_t)n_track, missing_cap);
    if (!c.ok || !ctx_.check(svs_map_add_keyframe_dev(map_, &a, d_newpoint_list, d_trackpoint_list, missing_cap, &c.r, c.keys.data(), c.kept.data(), c.exists.data(),
                                                      c.cons.data(), c.miss.data())))
      return false;
    addKeyframeResult_(c.r, c.keys, c.kept, c.exists, c.cons, c.miss, (size_t)n_new, (size_t)n_track, newkey.frame_id, c.n_kf, missing_cap, out);
    return true;
  }
  // StereoFrontend::addNewKeyframeToMap's half on this side (svs_frontend_commit_keyframe): the request names stream, slot, ids and the disparity; the lists, the
  // pyramid, the pose and the thresholds are the front end's.  n_new / n_track: of the stream's decision record
  bool addKeyframeFromFrontend(svs_frontend *fe, const svs_commit_keyframe_request &q, int n_new, int n_track, AddKeyframeResult *out, int missing_cap = 64) {
    if (!ok_ || !out || !fe || n_new < 0 || n_track < 0 || missing_cap < 1) return false;
    AddKeyframeCall_ c(this, (size_t)n_new, (size_t)n_track, missing_cap);
    if (!c.ok || !ctx_.check(svs_frontend_commit_keyframe(fe, map_, &q, missing_cap, &c.r, c.keys.data(), c.kept.data(), c.exists.data(), c.cons.data(), c.miss.data())))
      return false;
    addKeyframeResult_(c.r, c.keys, c.kept, c.exists, c.cons, c.miss, (size_t)n_new, (size_t)n_track, q.newkey_id, c.n_kf, missing_cap, out);
    return true;
  }
  void setAnchorLevel(int point_id, int anchor_level) { if (point_id >= 0 && (size_t)point_id < level_.size()) level_[(size_t)point_id] = (int8_t)anchor_level; }
  // ---- SlamGraph::registerKeyframes / addLoopClosure (slam_graph.cpp:188-251) on the device: svs_map_register_keyframes / svs_map_add_loop_closure, and what
  // BackendRegistration::localRegisterFrame(map, ..) / globalLoopClosure(map, ..) get from svs_reg_commit
  struct CommitResult {
    svs_reg_commit_result result;                                  // committed, the keyframe that took the pairs, T_new, the counts
    std::vector<int32_t> new_neighbors;                            // the other end of every new edge, ascending: their slots follow this order
    std::vector<svs_map_constraint_result> constraints;            // one per new edge
    std::vector<int32_t> missing;                                  // anchors some new edge lacked, ascending, each once
    std::vector<uint8_t> track_added;
  };
  // neighborid_to_strength: (frame_id, strength), any order; addNewEdges' test strength >= covis_thr is applied on the way.  false: refused as a whole
  bool registerKeyframes(int root_id, const double T_newroot_from_w[12], const std::vector<std::pair<int, int> > &neighborid_to_strength,
                         const std::vector<svs_map_track_point> &trackpoint_list, int covis_thr, CommitResult *out,
                         const std::vector<int32_t> &cached_ids = std::vector<int32_t>(), const std::vector<double> &cached_T12 = std::vector<double>(), int missing_cap = 64) {
    if (!ok_ || !out || cached_T12.size() != 12 * cached_ids.size() || missing_cap < 1) return false;
    const size_t n = neighborid_to_strength.size();
    std::vector<int32_t> ids(n + 1), st(n + 1), ekf(n + 1, -1), miss((n + 1) * missing_cap, -1), added(trackpoint_list.size() + 1);
    for (size_t i = 0; i < n; ++i) { ids[i] = neighborid_to_strength[i].first; st[i] = neighborid_to_strength[i].second; }
    std::vector<svs_map_constraint_result> cons(n + 1);
    *out = CommitResult();
    if (!ctx_.check(svs_map_register_keyframes(map_, root_id, T_newroot_from_w, (int)n, ids.data(), st.data(), covis_thr, (int)trackpoint_list.size(),
                                               trackpoint_list.empty() ? nullptr : trackpoint_list.data(), (int)cached_ids.size(), cached_ids.empty() ? nullptr : cached_ids.data(),
                                               cached_T12.empty() ? nullptr : cached_T12.data(), missing_cap, &out->result, ekf.data(), cons.data(), miss.data(), added.data())))
      return false;
    committed(out, ekf.data(), cons.data(), miss.data(), missing_cap, added.data(), trackpoint_list.size());
    return true;
  }
  // root_id: the query keyframe; the pairs go to loop_id, the APPEARANCE edge (root_id, loop_id) has strength trackpoint_list.size()
  bool addLoopClosure(int root_id, int loop_id, const double T_newloop_from_w[12], const std::vector<svs_map_track_point> &trackpoint_list, CommitResult *out,
                      const std::vector<int32_t> &cached_ids = std::vector<int32_t>(), const std::vector<double> &cached_T12 = std::vector<double>(), int missing_cap = 64) {
    if (!ok_ || !out || cached_T12.size() != 12 * cached_ids.size() || missing_cap < 1) return false;
    std::vector<int32_t> miss((size_t)missing_cap, -1), added(trackpoint_list.size() + 1);
    svs_map_constraint_result cons;
    const int32_t other = root_id;
    *out = CommitResult();
    if (!ctx_.check(svs_map_add_loop_closure(map_, root_id, loop_id, T_newloop_from_w, (int)trackpoint_list.size(), trackpoint_list.empty() ? nullptr : trackpoint_list.data(),
                                             (int)cached_ids.size(), cached_ids.empty() ? nullptr : cached_ids.data(), cached_T12.empty() ? nullptr : cached_T12.data(),
                                             missing_cap, &out->result, &cons, miss.data(), added.data())))
      return false;
    committed(out, &other, &cons, miss.data(), missing_cap, added.data(), trackpoint_list.size());
    return true;
  }
  // the result of a commit call into *out, and this object's edge keys (BackendRegistration calls it behind svs_reg_commit)
  void committed(CommitResult *out, const int32_t *edge_kf, const svs_map_constraint_result *cons, const int32_t *miss, int missing_cap, const int32_t *added, size_t n_added) {
    const int n_e = out->result.n_edges;
    out->new_neighbors.assign(edge_kf, edge_kf + n_e);
    out->constraints.assign(cons, cons + n_e);
    for (int e = 0; e < n_e; ++e)
      edge_keys_.push_back(std::make_pair(std::min(edge_kf[e], out->result.root_id), std::max(edge_kf[e], out->result.root_id)));
    std::sort(edge_keys_.begin(), edge_keys_.end());
    for (size_t i = 0; i < (size_t)n_e * missing_cap; ++i) if (miss[i] >= 0) out->missing.push_back(miss[i]);
    std::sort(out->missing.begin(), out->missing.end());
    out->missing.erase(std::unique(out->missing.begin(), out->missing.end()), out->missing.end());
    out->track_added.assign(added, added + n_added);
  }
  // directNeighborsOf (backend.cpp:433-449) from this object's edge keys: the frame itself and every keyframe it shares an edge with
  std::vector<int32_t> directNeighborsOf(int frame_id) const {
    std::vector<int32_t> out(1, frame_id);
    for (size_t i = 0; i < edge_keys_.size(); ++i) {
      if (edge_keys_[i].first == frame_id) out.push_back(edge_keys_[i].second);
      else if (edge_keys_[i].second == frame_id) out.push_back(edge_keys_[i].first);
    }
    return out;
  }
  int anchorLevel(int point_id) const { return point_id >= 0 && (size_t)point_id < level_.size() ? level_[(size_t)point_id] : 0; }

 private:
  static void thresholds(const RegistrationFrame &frame, std::vector<int32_t> *thr) {
    thr->assign((size_t)SVS_NUM_PYR_LEVELS * SVS_MAX_CELLS, 25);
    for (int l = 0; l < SVS_NUM_PYR_LEVELS; ++l)
      for (size_t c = 0; c < frame.cell_grid2d[l].size() && c < SVS_MAX_CELLS; ++c) (*thr)[(size_t)l * SVS_MAX_CELLS + c] = frame.cell_grid2d[l][c];
  }
  static bool innerIn(const std::vector<int32_t> &ids, const std::vector<int32_t> &types, int32_t id) {
    for (size_t i = 0; i < ids.size(); ++i) if (ids[i] == id) return types[i] == 0;
    return false;
  }
  // every edge between two INNER keyframes of the window, once, (lo, hi) ascending
  void innerPairs(const std::vector<int32_t> &ids, const std::vector<int32_t> &types, std::vector<int32_t> *out) const {
    std::vector<int32_t> inner;
    for (size_t i = 0; i < ids.size(); ++i) if (types[i] == 0) inner.push_back(ids[i]);
    std::sort(inner.begin(), inner.end());
    for (size_t i = 0; i < inner.size(); ++i)
      for (size_t j = i + 1; j < inner.size(); ++j)
        if (std::binary_search(edge_keys_.begin(), edge_keys_.end(), std::make_pair(inner[i], inner[j]))) { out->push_back(inner[i]); out->push_back(inner[j]); }
  }
  const Context &ctx_;
  svs_map *map_;
  std::vector<int8_t> level_;      // anchor_level by point id: MyTrackPoint carries it
  // the output arrays of one svs_map_add_keyframe* call, sized as the header asks
  struct AddKeyframeCall_ {
    svs_map_strength_result r;
    int32_t n_kf;
    bool ok;
    std::vector<svs_map_key> keys;
    std::vector<int32_t> kept, exists, miss;
    std::vector<svs_map_constraint_result> cons;
    AddKeyframeCall_(BackendMap *m, size_t n_new, size_t n_track, int missing_cap) : n_kf(0), keys(SVS_MAP_ADDKF_MAX_NEIGHBORS), kept(n_new + 1), exists(n_track + 1) {
      ok = m->ctx_.check(svs_map_info(m->map_, &n_kf, nullptr, nullptr));
      const size_t edge_cap = (size_t)std::max(1, std::min((int)n_kf, (int)SVS_MAP_ADDKF_MAX_NEIGHBORS));      // every key is a keyframe of the map
      miss.assign(edge_cap * (size_t)missing_cap, -1); cons.resize(edge_cap);
    }
  };
  // what a svs_map_add_keyframe* call left in its arrays, as AddKeyframeResult; the new edges join edge_keys_
  void addKeyframeResult_(const svs_map_strength_result &r, const std::vector<svs_map_key> &keys, const std::vector<int32_t> &kept, const std::vector<int32_t> &exists,
                          const std::vector<svs_map_constraint_result> &cons, const std::vector<int32_t> &miss, size_t n_new, size_t n_track, int newkey_id, int n_kf,
                          int missing_cap, AddKeyframeResult *out) {
    *out = AddKeyframeResult();
    out->over_capacity = r.over_capacity != 0; out->do_loop_detection = false;
    if (out->over_capacity) return;
    out->exclude_set.push_back(newkey_id);
    for (int i = 0; i < r.n_keys; ++i) {
      out->neighborid_to_strength.push_back(std::make_pair((int)keys[(size_t)i].kf_id, (int)keys[(size_t)i].strength));
      if (!keys[(size_t)i].edge) continue;
      out->new_neighbors.push_back(keys[(size_t)i].kf_id); out->exclude_set.push_back(keys[(size_t)i].kf_id);
      edge_keys_.push_back(std::make_pair(std::min(keys[(size_t)i].kf_id, (int32_t)newkey_id), std::max(keys[(size_t)i].kf_id, (int32_t)newkey_id)));
    }
    std::sort(edge_keys_.begin(), edge_keys_.end());
    out->constraints.assign(cons.begin(), cons.begin() + r.n_edges);
    for (size_t i = 0; i < (size_t)r.n_edges * missing_cap; ++i) if (miss[i] >= 0) out->missing.push_back(miss[i]);
    std::sort(out->missing.begin(), out->missing.end());
    out->missing.erase(std::unique(out->missing.begin(), out->missing.end()), out->missing.end());
    out->new_kept.assign(kept.begin(), kept.begin() + n_new); out->track_exists.assign(exists.begin(), exists.begin() + n_track);
    out->do_loop_detection = (int)out->exclude_set.size() < n_kf + 1;
  }
  std::vector<std::pair<int32_t, int32_t> > edge_keys_;      // (lo, hi) of every edge, sorted: what updateMarginalization selects its pairs from
  std::vector<int32_t> window_ids_, window_types_;           // the window prepareForOptimization(root_id, loop_id) prepared last: the next call's old_window
  int inner_size_ = 25, double_size_ = 200;                  // backend.cpp:141-144
  bool ok_;
};
inline bool StereoFrontend::setCandidatesFromMap(BackendMap &map, const std::vector<int32_t> &vertex_ids, const std::vector<int32_t> &slot_keyframe_ids,
                                                 const std::vector<svs_candidate_point> &newpoints, const std::vector<int32_t> &newpoint_group_end, bool refresh_poses,
                                                 svs_nbh_result *res, std::vector<int32_t> *point_ids, std::vector<FrontendVertex> *vertex_map, int vertex_cap) {
  if (!ok_ || !map.ok() || (int)slot_keyframe_ids.size() != max_keyframes_ || vertex_cap < 1) return false;
  const std::vector<int32_t> one_group(1, (int32_t)newpoints.size());
  const std::vector<int32_t> &ge = newpoint_group_end.empty() ? one_group : newpoint_group_end;
  svs_nbh_request q;
  std::memset(&q, 0, sizeof q);
  q.stream = 0; q.n_vertex = (int32_t)vertex_ids.size(); q.n_head = (int32_t)newpoints.size(); q.n_head_groups = (int32_t)ge.size();
  q.h_vertex_kf = vertex_ids.data(); q.h_slot_kf = slot_keyframe_ids.data(); q.h_head_group_end = ge.data(); q.h_head = newpoints.empty() ? nullptr : newpoints.data();
  svs_nbh_result r;
  std::vector<int32_t> pid((size_t)max_points_), vid((size_t)vertex_cap);
  std::vector<double> vT((size_t)vertex_cap * 12);
  if (!ctx_.check(svs_frontend_set_candidates_from_map(fe_, map.get(), 1, &q, refresh_poses ? 1 : 0, vertex_cap, &r, pid.data(), vid.data(), vT.data(), nullptr))) return false;
  if (res) *res = r;
  if (r.over_capacity) return false;
  n_ = r.n_points;
  if (point_ids) point_ids->assign(pid.begin(), pid.begin() + r.n_points);
  if (vertex_map) {
    vertex_map->resize((size_t)r.n_vertex);
    for (int i = 0; i < r.n_vertex; ++i) { (*vertex_map)[(size_t)i].frame_id = vid[(size_t)i]; std::memcpy((*vertex_map)[(size_t)i].T_me_from_w, &vT[(size_t)i * 12], 12 * sizeof(double)); }
  }
  return true;
}
inline bool StereoFrontend::setNeighborhoodFromMap(BackendMap &map, int32_t root_id, int32_t actkey_id, const std::vector<int32_t> &slot_keyframe_ids,
                                                   const std::vector<svs_candidate_point> &newpoints, const std::vector<int32_t> &newpoint_group_end, int n_fixed_groups,
                                                   const std::vector<int32_t> &newpoint_group_keyframe, bool refresh_poses, svs_nbr_result *res,
                                                   std::vector<int32_t> *point_ids, std::vector<FrontendVertex> *vertex_map, std::vector<int32_t> *act_neighbors,
                                                   int max_num_neighbors, int vertex_cap) {
  if (!ok_ || !map.ok() || (int)slot_keyframe_ids.size() != max_keyframes_ || vertex_cap < 1) return false;
  const std::vector<int32_t> one_group(1, (int32_t)newpoints.size());
  const bool grouped = !newpoint_group_end.empty();
  const std::vector<int32_t> &ge = grouped ? newpoint_group_end : one_group;
  if (grouped && newpoint_group_keyframe.size() != ge.size()) return false;
  svs_nbr_request q;
  std::memset(&q, 0, sizeof q);
  q.stream = 0; q.root_id = root_id; q.act_id = actkey_id; q.max_num_neighbors = max_num_neighbors;
  q.n_head = (int32_t)newpoints.size(); q.n_head_groups = (int32_t)ge.size(); q.n_fixed_groups = grouped ? n_fixed_groups : 1;
  q.h_slot_kf = slot_keyframe_ids.data(); q.h_head_group_end = ge.data(); q.h_head = newpoints.empty() ? nullptr : newpoints.data();
  q.h_head_group_kf = grouped ? newpoint_group_keyframe.data() : nullptr;
  svs_nbr_result r;
  std::vector<int32_t> pid((size_t)max_points_), vid((size_t)vertex_cap), nbr((size_t)vertex_cap);
  std::vector<double> vT((size_t)vertex_cap * 12);
  if (!ctx_.check(svs_frontend_set_neighborhood_from_root(fe_, map.get(), 1, &q, refresh_poses ? 1 : 0, vertex_cap, &r, pid.data(), vid.data(), vT.data(), nbr.data(),
                                                          nullptr, nullptr, nullptr, nullptr, nullptr)))
    return false;
  if (res) *res = r;
  if (r.over_capacity || r.root_outside_window) return false;
  n_ = r.n_points;
  if (point_ids) point_ids->assign(pid.begin(), pid.begin() + r.n_points);
  if (act_neighbors) act_neighbors->assign(nbr.begin(), nbr.begin() + r.n_act_neighbors);
  if (vertex_map) {
    vertex_map->resize((size_t)r.n_vertex);
    for (int i = 0; i < r.n_vertex; ++i) { (*vertex_map)[(size_t)i].frame_id = vid[(size_t)i]; std::memcpy((*vertex_map)[(size_t)i].T_me_from_w, &vT[(size_t)i * 12], 12 * sizeof(double)); }
  }
  return true;
}
inline bool StereoFrontend::setNeighborhoodFromStore(BackendMap &map, int32_t root_id, int32_t actkey_id, const std::vector<int32_t> &slot_keyframe_ids,
                                                     bool refresh_poses, svs_nbr_result *res, std::vector<int32_t> *point_ids, std::vector<FrontendVertex> *vertex_map,
                                                     std::vector<int32_t> *act_neighbors, int max_num_neighbors, int vertex_cap, int stream) {
  if (!ok_ || !map.ok() || (int)slot_keyframe_ids.size() != max_keyframes_ || vertex_cap < 1) return false;
  svs_nbr_request q;
  std::memset(&q, 0, sizeof q);
  q.stream = stream; q.root_id = root_id; q.act_id = actkey_id; q.max_num_neighbors = max_num_neighbors;
  q.h_slot_kf = slot_keyframe_ids.data();
  svs_nbr_result r;
  std::memset(&r, 0, sizeof r);
  std::vector<int32_t> pid((size_t)max_points_), vid((size_t)vertex_cap), nbr((size_t)vertex_cap);
  std::vector<double> vT((size_t)vertex_cap * 12);
  if (!ctx_.check(svs_frontend_set_neighborhood_from_store(fe_, map.get(), 1, &q, refresh_poses ? 1 : 0, vertex_cap, &r, pid.data(), vid.data(), vT.data(), nbr.data(),
                                                           nullptr, nullptr, nullptr, nullptr, nullptr)))
    return false;
  if (res) *res = r;
  if (r.over_capacity || r.root_outside_window) return false;
  if (stream == 0) n_ = r.n_points;
  if (point_ids) point_ids->assign(pid.begin(), pid.begin() + r.n_points);
  if (act_neighbors) act_neighbors->assign(nbr.begin(), nbr.begin() + r.n_act_neighbors);
  if (vertex_map) {
    vertex_map->resize((size_t)r.n_vertex);
    for (int i = 0; i < r.n_vertex; ++i) { (*vertex_map)[(size_t)i].frame_id = vid[(size_t)i]; std::memcpy((*vertex_map)[(size_t)i].T_me_from_w, &vT[(size_t)i * 12], 12 * sizeof(double)); }
  }
  return true;
}
inline bool StereoFrontend::addNewKeyframeToMap(BackendMap &map, int slot, int newkey_id, int oldkey_id, const svs_keyframe_decision &dec, const float *d_disp,
                                                int disp_stride, int covis_thr, const svs_cam &cam, MapAddKeyframeResult *out, const std::vector<int32_t> &cached_ids,
                                                const std::vector<double> &cached_T12, int missing_cap, int stream) {
  if (!ok_ || !map.ok() || cached_T12.size() != 12 * cached_ids.size()) return false;
  svs_commit_keyframe_request q;
  std::memset(&q, 0, sizeof q);
  q.stream = stream; q.slot = slot; q.newkey_id = newkey_id; q.oldkey_id = oldkey_id; q.covis_thr = covis_thr;
  q.half_width = (int)(cam.w * 0.5); q.half_height = (int)(cam.h * 0.5); q.disp_stride = disp_stride; q.disp = d_disp;
  q.n_cached = (int32_t)cached_ids.size(); q.cached_ids = cached_ids.empty() ? nullptr : cached_ids.data(); q.cached_T = cached_T12.empty() ? nullptr : cached_T12.data();
  return map.addKeyframeFromFrontend(fe_, q, dec.n_new, dec.n_track, out, missing_cap);
}
class BackendRegistration {
 public:
  BackendRegistration(const Context &c, const svs_cam &stereo_cam, int max_points = 4096, int max_keyframes = 256, int max_observers = 65536, int covis_thr = 15)
      : ctx_(c), reg_(nullptr), max_points_(max_points), max_keyframes_(max_keyframes) {
    std::memset(&last_, 0, sizeof last_);
    svs_reg_params_default(&prm_);
    prm_.covis_thr = covis_thr;
    ok_ = c.check(svs_reg_create(c.get(), &stereo_cam, 1, max_points, max_keyframes, max_observers, &reg_));
  }
  ~BackendRegistration() { if (reg_) svs_reg_destroy(reg_); }
  BackendRegistration(const BackendRegistration &) = delete;
  BackendRegistration &operator=(const BackendRegistration &) = delete;
  bool ok() const { return ok_; }
  svs_reg *get() const { return reg_; }
  // bool Backend::localRegisterFrame(int rootframe_id): true when a neighbour qualifies.  points[i].kf_index = entry of `keyframes` of the anchor; row i of the
  // observer table = obs_kf[obs_begin[i] .. obs_begin[i + 1]): the entries whose feature_table holds points[i].  neighborid_to_strength: (frame_id, strength) of
  // the qualifying keyframes in table order; trackpoint_list: per qualifying keyframe, in that order, the accepted observations it shares, in point order
  bool localRegisterFrame(const RegistrationFrame &root, const std::vector<RegistrationKeyframe> &keyframes, const std::vector<svs_candidate_point> &points,
                          const std::vector<int32_t> &obs_begin, const std::vector<int32_t> &obs_kf, double T_newroot_from_oldroot[12],
                          std::vector<std::pair<int, int> > *neighborid_to_strength, std::vector<TrackPoint> *trackpoint_list) {
    if (neighborid_to_strength) neighborid_to_strength->clear();
    if (trackpoint_list) trackpoint_list->clear();
    if (obs_begin.size() != points.size() + 1) return false;
    if (!run(SVS_REG_LOCAL, root, keyframes, points, &obs_begin, &obs_kf)) return false;
    if (T_newroot_from_oldroot) std::memcpy(T_newroot_from_oldroot, last_.T_newroot_from_oldroot, sizeof last_.T_newroot_from_oldroot);
    if (last_.status != SVS_REG_OK) return false;
    for (size_t k = 0; k < keyframes.size(); ++k) {
      if (!kf_stats_[k].qualifies) continue;
      if (neighborid_to_strength) neighborid_to_strength->push_back(std::make_pair(keyframes[k].frame_id, (int)kf_stats_[k].strength));
      for (int i = 0; trackpoint_list && i < last_.n_candidates; ++i) {
        if (!accepted_[i]) continue;
        const int s = cand_src_[i];
        bool shared = false;
        for (int32_t e = obs_begin[s]; e < obs_begin[s + 1] && !shared; ++e) shared = obs_kf[e] == (int32_t)k;
        if (shared) trackpoint_list->push_back(track_point(points[s], matches_[i]));
      }
    }
    return true;
  }
  // bool Backend::globalLoopClosure(const DetectedLoop&): loop_frame = the loop keyframe with T_from_world = T_query_from_loop^-1 * T_query_from_world (:845),
  // points = v_query.feature_table in the caller's order.  trackpoint_list: the accepted observations, in point order (:945-950)
  bool globalLoopClosure(const RegistrationFrame &loop_frame, const std::vector<RegistrationKeyframe> &keyframes, const std::vector<svs_candidate_point> &points,
                         double T_newloop_from_oldloop[12], std::vector<TrackPoint> *trackpoint_list) {
    if (trackpoint_list) trackpoint_list->clear();
    if (!run(SVS_REG_LOOP, loop_frame, keyframes, points, nullptr, nullptr)) return false;
    if (T_newloop_from_oldloop) std::memcpy(T_newloop_from_oldloop, last_.T_newroot_from_oldroot, sizeof last_.T_newroot_from_oldroot);
    if (last_.status != SVS_REG_OK) return false;
    for (int i = 0; trackpoint_list && i < last_.n_candidates; ++i)
      if (accepted_[i]) trackpoint_list->push_back(track_point(points[cand_src_[i]], matches_[i]));
    return true;
  }
  // localRegisterFrame (mode SVS_REG_LOCAL: walk = framesInNeighborhood(root), direct = directNeighborsOf(root)) / globalLoopClosure (SVS_REG_LOOP: root = the
  // loop keyframe, T_root_from_world = T_loop_from_world (:845), walk = {the query keyframe}) against a device-resident map: the point walk, the keyframe table and the
  // observer rows are built on the device.  neighborid_to_strength: (frame_id, strength) of the qualifying keyframes in ascending id (loop mode: the loop keyframe
  // with the frame-wide strength); trackpoint_list: the accepted observations once, in ascending point id -- the caller's feature tables say which of the
  // qualifying keyframes shares which.  false with lastResult().status == SVS_REG_OVER_CAPACITY: the built request exceeds this object's capacities
  bool registerFrames(const BackendMap &map, int mode, int root_id, const double T_root_from_world[12], const std::vector<int32_t> &walk, const std::vector<int32_t> &direct,
                      double T_newroot_from_oldroot[12], std::vector<std::pair<int, int> > *neighborid_to_strength, std::vector<TrackPoint> *trackpoint_list) {
    if (neighborid_to_strength) neighborid_to_strength->clear();
    if (trackpoint_list) trackpoint_list->clear();
    if (!ok_ || !map.ok()) return false;
    svs_reg_map_request q;
    std::memset(&q, 0, sizeof q);
    q.mode = mode; q.root_kf = root_id; q.n_walk = (int32_t)walk.size(); q.n_direct = (int32_t)direct.size();
    std::memcpy(q.T_root_from_world, T_root_from_world, sizeof q.T_root_from_world);
    q.h_walk_kf = walk.empty() ? nullptr : walk.data(); q.h_direct_kf = direct.empty() ? nullptr : direct.data();
    cand_src_.assign((size_t)max_points_, -1); matches_.assign((size_t)max_points_, svs_match_result()); accepted_.assign((size_t)max_points_, 0);
    kf_stats_.assign((size_t)max_keyframes_, svs_reg_kf_stats());
    point_ids_.assign((size_t)max_points_, -1); kf_ids_.assign((size_t)max_keyframes_, -1);
    int32_t n_kf = 0;
    if (!ctx_.check(svs_reg_register_map_batch(reg_, map.get(), 1, &q, &prm_, &last_, cand_src_.data(), matches_.data(), nullptr, accepted_.data(), kf_stats_.data(),
                                                nullptr, point_ids_.data(), kf_ids_.data(), &n_kf)))
      return false;
    if (T_newroot_from_oldroot) std::memcpy(T_newroot_from_oldroot, last_.T_newroot_from_oldroot, sizeof last_.T_newroot_from_oldroot);
    if (last_.status != SVS_REG_OK) return false;
    for (int k = 0; neighborid_to_strength && k < n_kf; ++k)
      if (kf_stats_[(size_t)k].qualifies) neighborid_to_strength->push_back(std::make_pair((int)kf_ids_[(size_t)k], (int)kf_stats_[(size_t)k].strength));
    for (int i = 0; trackpoint_list && i < last_.n_candidates; ++i) {
      if (!accepted_[(size_t)i]) continue;
      svs_candidate_point p;
      std::memset(&p, 0, sizeof p);
      p.point_id = point_ids_[(size_t)i]; p.anchor_level = map.anchorLevel(p.point_id);
      trackpoint_list->push_back(track_point(p, matches_[(size_t)i]));
    }
    return true;
  }
  // bool Backend::localRegisterFrame(int rootframe_id) on a device-resident map, to its end: the walk (framesInNeighborhood over directNeighborsOf(root).size() +
  // num_frames_to_check keyframes, :552-561), the registration and the commit (svs_reg_commit: registerKeyframes on the device).  true: the graph was updated
  bool localRegisterFrame(BackendMap &map, int rootframe_id, BackendMap::CommitResult *out = nullptr, int num_frames_to_check = 40,
                          const std::vector<int32_t> &cached_ids = std::vector<int32_t>(), const std::vector<double> &cached_T12 = std::vector<double>()) {
    if (!ok_ || !map.ok()) return false;
    const std::vector<int32_t> direct = map.directNeighborsOf(rootframe_id);
    std::vector<int32_t> walk;
    const int size = std::min((int)direct.size() + num_frames_to_check, max_keyframes_);
    if (!map.framesInNeighborhood(rootframe_id, size, &walk)) return false;
    double T_root[12];
    const int32_t root = rootframe_id;
    if (!ctx_.check(svs_map_get_poses(map.get(), 1, &root, T_root))) return false;
    if (!registerFrames(map, SVS_REG_LOCAL, rootframe_id, T_root, walk, direct, nullptr, nullptr, nullptr)) return false;
    return commit(map, out, cached_ids, cached_T12);
  }
  // bool Backend::globalLoopClosure(const DetectedLoop&): T_loop_from_world = inverse(T_query_from_loop) * T_query_from_world is formed here (:845) as the library's
  // kernels form a pose product (rows ((a0 b0 + a1 b1) + a2 b2) + t)
  bool globalLoopClosure(BackendMap &map, int query_keyframe_id, int loop_keyframe_id, const double T_query_from_loop[12], BackendMap::CommitResult *out = nullptr,
                         const std::vector<int32_t> &cached_ids = std::vector<int32_t>(), const std::vector<double> &cached_T12 = std::vector<double>()) {
    if (!ok_ || !map.ok()) return false;
    double Tq[12], Ti[12], T_loop[12];
    const int32_t query = query_keyframe_id;
    if (!ctx_.check(svs_map_get_poses(map.get(), 1, &query, Tq))) return false;
    for (int i = 0; i < 3; ++i) {
      for (int j = 0; j < 3; ++j) Ti[4 * i + j] = T_query_from_loop[4 * j + i];
      Ti[4 * i + 3] = -((T_query_from_loop[i] * T_query_from_loop[3] + T_query_from_loop[4 + i] * T_query_from_loop[7]) + T_query_from_loop[8 + i] * T_query_from_loop[11]);
    }
    for (int i = 0; i < 3; ++i)
      for (int j = 0; j < 4; ++j)
        T_loop[4 * i + j] = ((Ti[4 * i] * Tq[j] + Ti[4 * i + 1] * Tq[4 + j]) + Ti[4 * i + 2] * Tq[8 + j]) + (j == 3 ? Ti[4 * i + 3] : 0.0);
    const std::vector<int32_t> walk(1, query_keyframe_id);
    if (!registerFrames(map, SVS_REG_LOOP, loop_keyframe_id, T_loop, walk, std::vector<int32_t>(), nullptr, nullptr, nullptr)) return false;
    return commit(map, out, cached_ids, cached_T12);
  }
  // registerKeyframes / addLoopClosure for the request registerFrames ran last (svs_reg_commit)
  bool commit(BackendMap &map, BackendMap::CommitResult *out, const std::vector<int32_t> &cached_ids = std::vector<int32_t>(),
              const std::vector<double> &cached_T12 = std::vector<double>(), int missing_cap = 64) {
    if (!ok_ || !map.ok() || cached_T12.size() != 12 * cached_ids.size() || missing_cap < 1) return false;
    BackendMap::CommitResult r;
    std::vector<int32_t> ekf((size_t)max_keyframes_, -1), miss((size_t)max_keyframes_ * missing_cap, -1), added((size_t)max_points_ + 1, 0);
    std::vector<svs_map_constraint_result> cons((size_t)max_keyframes_);
    if (!ctx_.check(svs_reg_commit(reg_, map.get(), 0, (int)cached_ids.size(), cached_ids.empty() ? nullptr : cached_ids.data(), cached_T12.empty() ? nullptr : cached_T12.data(),
                                   missing_cap, &r.result, ekf.data(), nullptr, cons.data(), miss.data(), max_points_, nullptr, added.data())))
      return false;
    map.committed(&r, ekf.data(), cons.data(), miss.data(), missing_cap, added.data(), (size_t)r.result.n_track);
    if (out) *out = r;
    return r.result.committed != 0;
  }
  const std::vector<int32_t> &lastPointIds() const { return point_ids_; }          // registerFrames: per candidate
  const std::vector<int32_t> &lastKeyframeIds() const { return kf_ids_; }          // registerFrames: per table entry
  const svs_reg_result &lastResult() const { return last_; }                       // status says which exit was taken
  const std::vector<svs_reg_kf_stats> &lastKeyframeStats() const { return kf_stats_; }
  const std::vector<svs_match_result> &lastMatches() const { return matches_; }
  const std::vector<int32_t> &lastAccepted() const { return accepted_; }
  const std::vector<int32_t> &lastCandidates() const { return cand_src_; }

 private:
  static TrackPoint track_point(const svs_candidate_point &p, const svs_match_result &m) {
    TrackPoint t;
    t.global_id = p.point_id; t.anchor_level = p.anchor_level;
    t.uvu[0] = m.obs[0]; t.uvu[1] = m.obs[1]; t.uvu[2] = m.obs[2];
    return t;
  }
  bool run(int mode, const RegistrationFrame &root, const std::vector<RegistrationKeyframe> &keyframes, const std::vector<svs_candidate_point> &points,
           const std::vector<int32_t> *obs_begin, const std::vector<int32_t> *obs_kf) {
    if (!ok_ || keyframes.empty()) return false;
    std::vector<svs_keyframe> kfs(keyframes.size());
    std::vector<uint8_t> flags(keyframes.size());
    for (size_t k = 0; k < keyframes.size(); ++k) {
      kfs[k] = keyframes[k].kf;
      flags[k] = (uint8_t)((keyframes[k].in_double_window ? SVS_REG_KF_IN_WINDOW : 0) | (keyframes[k].direct_neighbor ? SVS_REG_KF_DIRECT_NEIGHBOR : 0));
    }
    svs_reg_request q;
    std::memset(&q, 0, sizeof q);
    q.mode = mode; q.n_kf = (int32_t)kfs.size(); q.n_src = (int32_t)points.size(); q.root_kf = root.table_entry;
    q.d_root_disp = root.d_disp; q.root_disp_stride = root.disp_stride;
    for (int l = 0; l < SVS_NUM_PYR_LEVELS; ++l)
      for (int c = 0; c < SVS_MAX_CELLS; ++c) q.fast_thr[l][c] = c < (int)root.cell_grid2d[l].size() ? root.cell_grid2d[l][c] : 25;
    std::memcpy(q.T_root_from_world, root.T_from_world, sizeof q.T_root_from_world);
    q.h_kfs = kfs.data(); q.h_kf_flags = flags.data(); q.h_src = points.empty() ? nullptr : points.data();
    q.h_obs_begin = obs_begin ? obs_begin->data() : nullptr;
    q.h_obs_kf = obs_kf && !obs_kf->empty() ? obs_kf->data() : nullptr;
    cand_src_.assign((size_t)max_points_, -1); matches_.assign((size_t)max_points_, svs_match_result()); accepted_.assign((size_t)max_points_, 0);
    kf_stats_.assign((size_t)max_keyframes_, svs_reg_kf_stats());
    return ctx_.check(svs_reg_register_batch(reg_, 1, &q, &prm_, &last_, cand_src_.data(), matches_.data(), nullptr, accepted_.data(), kf_stats_.data(), nullptr));
  }
  const Context &ctx_;
  svs_reg *reg_;
  int max_points_, max_keyframes_;
  svs_reg_params prm_;
  svs_reg_result last_;
  std::vector<int32_t> cand_src_, accepted_, point_ids_, kf_ids_;
  std::vector<svs_match_result> matches_;
  std::vector<svs_reg_kf_stats> kf_stats_;
  bool ok_;
};

// One rank of a landmark-sharded back-end: rank 0 calls uniqueId() and distributes it (MPI_Bcast, a TCP store, a file); every rank then constructs
// the communicator and attaches it to its SlamGraphBA with attach().  svs_ba_optimize all-reduces over RCCL on the context's stream.
class Communicator {
 public:
  static bool uniqueId(const Context &c, svs_unique_id *id) { return c.check(svs_comm_get_unique_id(c.get(), id)); }
  Communicator(const Context &c, const svs_unique_id &id, int rank, int world) : comm_(nullptr) { ok_ = c.check(svs_comm_create(c.get(), &id, rank, world, &comm_)); }
  ~Communicator() { if (comm_) svs_comm_destroy(comm_); }
  Communicator(const Communicator &) = delete;
  Communicator &operator=(const Communicator &) = delete;
  bool ok() const { return ok_; }
  svs_comm *get() const { return comm_; }

 private:
  svs_comm *comm_;
  bool ok_;
};

// SlamGraph::optimize(const OptParams&) (slam_graph.hpp:457-462): the caller marshals the double
// window exactly as copyDataToG2o does (slam_graph.cpp:983-1032) into flat arrays.
struct OptParams {                       // slam_graph.hpp:36-50
  OptParams(int num_iters, bool use_robust_kernel, double huber_kernel_width)
      : num_iters(num_iters), use_robust_kernel(use_robust_kernel), huber_kernel_width(huber_kernel_width) {}
  int num_iters; bool use_robust_kernel; double huber_kernel_width;
};
class SlamGraphBA {
 public:
  explicit SlamGraphBA(const Context &c) : ctx_(c), ba_(nullptr) { c.check(svs_ba_create(c.get(), &ba_)); }
  ~SlamGraphBA() { if (ba_) svs_ba_destroy(ba_); }
  SlamGraphBA(const SlamGraphBA &) = delete;
  SlamGraphBA &operator=(const SlamGraphBA &) = delete;
  // poses [P][12] and psi [L][3] are updated in place, like restoreDataFromG2o (slam_graph.cpp:1035-1058)
  bool optimize(const OptParams &opt, const svs_cam &cam, std::vector<double> *poses, std::vector<double> *psi,
                const std::vector<svs_ba_edge> &obs_edges, const std::vector<svs_ba_constraint> &constraints,
                svs_ba_stats *stats = nullptr, bool exact_self_edges = false) {
    svs_ba_params prm = params(opt, exact_self_edges);
    const int P = (int)(poses->size() / 12), L = (int)(psi->size() / 3);
    if (!ctx_.check(svs_ba_set_problem(ba_, P, poses->data(), L, psi->data(), (int)obs_edges.size(), obs_edges.data(),
                                       (int)constraints.size(), constraints.data(), &cam, &prm, 1))) return false;
    if (!ctx_.check(svs_ba_optimize(ba_, nullptr, nullptr, stats))) return false;
    return ctx_.check(svs_ba_get_state(ba_, poses->data(), psi->data()));
  }
  // ---- the marshalling of SlamGraph::copyDataToG2o / restoreDataFromG2o (slam_graph.cpp:983-1058) from records that keep the GRAPH'S OWN IDS ----
  // One record per addObsToG2o call (slam_graph-impl.cpp:44-97): the ImageFeature of vertex `pose_id`'s feature_table for point `point_id`
  struct ObsById { int point_id, pose_id, level; double center[3]; };
  // One record per addConstraintToG2o call (slam_graph-impl.cpp:99-126).  copyContraintsToG2o (slam_graph.cpp:937-981) walks ORDERED pairs of the double
  // window, so a marginalised edge with an OUTER end is handed over twice: (1, 2, T_2_from_1, Lambda_2_from_1) and (2, 1, T_1_from_2, Lambda_1_from_2) --
  // the caller passes both, as the reference does
  struct ConstraintById { int pose_id_1, pose_id_2; double T_2_from_1[12], Lambda_2_from_1[36]; };
  // pose_ids / poses [P][12]: the double window in the order of copyPosesToG2o; point_ids / anchor_ids / xyz_anchor [L][3]: the active points (Point::xyz_anchor,
  // Point::anchorframe_id) -- converted to the inverse-depth parameters the solver works on (invert_depth, slam_graph.cpp:916) and back (:1054);
  // observations from frames outside the window are skipped like slam_graph.cpp:1001-1006 does; information = diag(4^-level, 4^-level, 0.333^2) (:1010-1015).
  // poses and xyz_anchor are updated in place.  false: an anchor frame outside the window (the reference asserts), or a library error
  bool optimizeWindow(const OptParams &opt, const svs_cam &cam, const std::vector<int> &pose_ids, std::vector<double> *poses, const std::vector<int> &point_ids,
                      const std::vector<int> &anchor_ids, std::vector<double> *xyz_anchor, const std::vector<ObsById> &obs,
                      const std::vector<ConstraintById> &constraints, svs_ba_stats *stats = nullptr) {
    const size_t P = pose_ids.size(), L = point_ids.size();
    if (poses->size() != 12 * P || xyz_anchor->size() != 3 * L || anchor_ids.size() != L) return false;
    std::vector<std::pair<int, int> > pmap(P), lmap(L);                      // (id, index), sorted: the hash maps of the reference flattened
    for (size_t i = 0; i < P; ++i) pmap[i] = std::make_pair(pose_ids[i], (int)i);
    for (size_t i = 0; i < L; ++i) lmap[i] = std::make_pair(point_ids[i], (int)i);
    std::sort(pmap.begin(), pmap.end()); std::sort(lmap.begin(), lmap.end());
    std::vector<double> psi(3 * L);
    std::vector<int> anchor_idx(L);
    for (size_t i = 0; i < L; ++i) {
      const double *x = &(*xyz_anchor)[3 * i];
      psi[3 * i] = x[0] / x[2]; psi[3 * i + 1] = x[1] / x[2]; psi[3 * i + 2] = 1. / x[2];      // invert_depth (maths_utils.h:66-69)
      if ((anchor_idx[i] = find(pmap, anchor_ids[i])) < 0) return false;
    }
    std::vector<svs_ba_edge> edges;
    edges.reserve(obs.size());
    for (size_t k = 0; k < obs.size(); ++k) {
      const int pt = find(lmap, obs[k].point_id), po = find(pmap, obs[k].pose_id);
      if (pt < 0 || po < 0) continue;                                         // point not active / frame not in the double window
      svs_ba_edge e;
      std::memset(&e, 0, sizeof e);
      const double f = 1. / (double)(1 << obs[k].level);                     // pyrFromZero_d(1., level)
      for (int c = 0; c < 3; ++c) e.obs[c] = obs[k].center[c];
      e.info[0] = e.info[1] = f * f; e.info[2] = 0.333 * 0.333;               // Po2(...) (slam_graph.cpp:1010-1015)
      e.point = pt; e.pose = po; e.anchor = anchor_idx[pt];
      edges.push_back(e);
    }
    std::vector<svs_ba_constraint> cons(constraints.size());
    for (size_t k = 0; k < constraints.size(); ++k) {
      std::memcpy(cons[k].T_21, constraints[k].T_2_from_1, sizeof cons[k].T_21);
      std::memcpy(cons[k].info, constraints[k].Lambda_2_from_1, sizeof cons[k].info);
      cons[k].pose1 = find(pmap, constraints[k].pose_id_1); cons[k].pose2 = find(pmap, constraints[k].pose_id_2);
      if (cons[k].pose1 < 0 || cons[k].pose2 < 0) return false;
    }
    if (!optimize(opt, cam, poses, &psi, edges, cons, stats)) return false;
    for (size_t i = 0; i < L; ++i) {                                          // invert_depth again (slam_graph.cpp:1054)
      double *x = &(*xyz_anchor)[3 * i];
      const double *s = &psi[3 * i];
      x[0] = s[0] / s[2]; x[1] = s[1] / s[2]; x[2] = 1. / s[2];
    }
    return true;
  }
  // The same call for a window that slides: the library keeps the observations it has been given (svs_ba_window_update), a call brings the window by ids,
  // the current values and the observations made SINCE THE LAST CALL.  new_obs: ObsById records; everything else as optimizeWindow
  bool optimizeSlidingWindow(const OptParams &opt, const svs_cam &cam, const std::vector<int> &pose_ids, std::vector<double> *poses,
                             const std::vector<int> &point_ids, const std::vector<int> &anchor_ids, std::vector<double> *xyz_anchor,
                             const std::vector<ObsById> &new_obs, const std::vector<ConstraintById> &constraints, svs_ba_stats *stats = nullptr) {
    const size_t P = pose_ids.size(), L = point_ids.size();
    if (poses->size() != 12 * P || xyz_anchor->size() != 3 * L || anchor_ids.size() != L) return false;
    std::vector<double> psi(3 * L);
    for (size_t i = 0; i < L; ++i) { const double *x = &(*xyz_anchor)[3 * i]; psi[3 * i] = x[0] / x[2]; psi[3 * i + 1] = x[1] / x[2]; psi[3 * i + 2] = 1. / x[2]; }
    std::vector<svs_ba_edge> eo(new_obs.size());
    for (size_t k = 0; k < new_obs.size(); ++k) {
      std::memset(&eo[k], 0, sizeof eo[k]);
      const double f = 1. / (double)(1 << new_obs[k].level);
      for (int c = 0; c < 3; ++c) eo[k].obs[c] = new_obs[k].center[c];
      eo[k].info[0] = eo[k].info[1] = f * f; eo[k].info[2] = 0.333 * 0.333;
      eo[k].point = new_obs[k].point_id; eo[k].pose = new_obs[k].pose_id;     // ids: the library resolves them against the window
    }
    std::vector<svs_ba_constraint> cons(constraints.size());
    for (size_t k = 0; k < constraints.size(); ++k) {
      std::memcpy(cons[k].T_21, constraints[k].T_2_from_1, sizeof cons[k].T_21);
      std::memcpy(cons[k].info, constraints[k].Lambda_2_from_1, sizeof cons[k].info);
      cons[k].pose1 = constraints[k].pose_id_1; cons[k].pose2 = constraints[k].pose_id_2;
    }
    svs_ba_params prm = params(opt, false);
    if (!ctx_.check(svs_ba_window_update(ba_, (int)P, pose_ids.data(), poses->data(), (int)L, point_ids.data(), psi.data(), anchor_ids.data(), (int)eo.size(),
                                         eo.data(), (int)cons.size(), cons.data(), &cam, &prm)))
      return false;
    if (!ctx_.check(svs_ba_optimize(ba_, nullptr, nullptr, stats))) return false;
    if (!ctx_.check(svs_ba_get_state(ba_, poses->data(), psi.data()))) return false;
    for (size_t i = 0; i < L; ++i) { double *x = &(*xyz_anchor)[3 * i]; const double *s = &psi[3 * i]; x[0] = s[0] / s[2]; x[1] = s[1] / s[2]; x[2] = 1. / s[2]; }
    return true;
  }
  bool windowReset() { return ctx_.check(svs_ba_window_reset(ba_)); }
  // ---- the window BackendMap::prepareForOptimization left in the map, device to device (svs_ba_window_from_map / svs_ba_store_to_map) ----
  // copyDataToG2o: poses and points are read from the map now, the edges come from its measured observations; only the constraints (both directions, frame
  // ids of the final window, as optimizeWindow takes them) are uploaded.  Then optimize() below and restoreDataToMap
  bool copyDataFromMap(BackendMap &map, const OptParams &opt, const svs_cam &cam, const std::vector<ConstraintById> &constraints) {
    std::vector<svs_ba_constraint> ec(constraints.size());
    for (size_t k = 0; k < constraints.size(); ++k) {
      svs_ba_constraint &r = ec[k];
      std::memcpy(r.T_21, constraints[k].T_2_from_1, sizeof r.T_21);
      std::memcpy(r.info, constraints[k].Lambda_2_from_1, sizeof r.info);
      r.pose1 = constraints[k].pose_id_1; r.pose2 = constraints[k].pose_id_2;
    }
    svs_ba_params prm = params(opt, false);
    return ctx_.check(svs_ba_window_from_map(ba_, map.get(), (int)ec.size(), ec.data(), &cam, &prm));
  }
  // the same with copyContraintsToG2o done from the map's edge table (svs_ba_window_from_map_edges): nothing but a list of indices is uploaded
  bool copyDataFromMap(BackendMap &map, const OptParams &opt, const svs_cam &cam) {
    svs_ba_params prm = params(opt, false);
    return ctx_.check(svs_ba_window_from_map_edges(ba_, map.get(), &cam, &prm));
  }
  bool optimize(svs_ba_stats *stats = nullptr) { return ctx_.check(svs_ba_optimize(ba_, nullptr, nullptr, stats)); }
  // restoreDataFromG2o on the device: one launch, asynchronous
  bool restoreDataToMap(BackendMap &map) { return ctx_.check(svs_ba_store_to_map(ba_, map.get())); }
  // landmark-sharded operation: this rank passes only ITS landmarks' edges to optimize() (pose terms on exactly one rank: add_pose_terms)
  bool attach(const Communicator *comm) { return ctx_.check(svs_ba_set_comm(ba_, comm ? comm->get() : nullptr)); }
  svs_ba *get() const { return ba_; }

 private:
  static svs_ba_params params(const OptParams &opt, bool exact_self_edges) {
    svs_ba_params prm;
    prm.num_iters = opt.num_iters; prm.use_robust = opt.use_robust_kernel ? 1 : 0;
    prm.huber_delta = 1.0;               // huber_kernel_width is dead in the reference (slam_graph-impl.cpp:86-90)
    prm.lambda_init = 50.0;              // slam_graph.cpp:338
    prm.max_trials = 5;                  // slam_graph.cpp:1073
    prm.self_edge_mode = exact_self_edges ? 1 : 0;
    return prm;
  }
  static int find(const std::vector<std::pair<int, int> > &m, int id) {
    std::vector<std::pair<int, int> >::const_iterator it = std::lower_bound(m.begin(), m.end(), std::make_pair(id, -1));
    return it != m.end() && it->first == id ? it->second : -1;
  }
  const Context &ctx_;
  svs_ba *ba_;
};

}  // namespace scavislam_hip
#endif
