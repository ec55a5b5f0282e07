/*
 * scavislam_hip.h -- C ABI of the MI355X (gfx950) implementation of ScaViSLAM's two hot paths.
 *
 * The reference (strasdat/ScaViSLAM) has no FFI/plugin layer: its seams are C++ member functions
 * switched at compile time by SCAVISLAM_CUDA_SUPPORT.  Every entry point
 * below names the reference interface it replaces (file:line under /root/reference/scavislam).
 * INTEGRATION.md shows the adaptor a maintainer adds on the reference side; the C++ adaptor
 * classes with the reference's method names are in include/scavislam_hip.hpp.
 *
 * Conventions:
 *  - every function returns int status, 0 = SVS_OK; never throws, never aborts;
 *  - an svs_ctx owns one HIP stream + scratch; one ctx per calling thread (the reference calls
 *    FAST/matcher from both the front-end and the back-end thread); no process-global state;
 *  - pointers named d_* are DEVICE pointers, h_* are HOST pointers; strides are in ELEMENTS of
 *    the pointed-to type; *_bstride is the element distance between consecutive batch slots;
 *  - device entry points are asynchronous on the ctx stream; svs_ctx_sync() or any *_download /
 *    h_* output makes results visible (blocking, like every reference call);
 *  - poses are 3x4 row-major double[12] (R | t), T_a_from_b convention of the reference;
 *  - a "batch" is a set of independent camera streams / frames processed by one launch.
 */
#ifndef SCAVISLAM_HIP_H
#define SCAVISLAM_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ABI version: bumped whenever a struct of this header grows or a signature changes (round 3 grew svs_pose_opt_params / svs_match_args and put a `stream`
   argument into svs_frontend_device_view without one -- INTEGRATION.md section 6).  A caller checks svs_api_version() == SVS_API_VERSION once, zero-initialises
   every parameter struct (or takes it from the *_default() initialisers) and sets only the fields it knows. */
#define SVS_API_VERSION 9
int svs_api_version(void);             /* the SVS_API_VERSION the loaded library was built with */

enum {
  SVS_OK = 0,
  SVS_ERR_INVALID = 1,      /* bad argument */
  SVS_ERR_HIP = 2,          /* HIP runtime error; see svs_last_error */
  SVS_ERR_NO_DEVICE = 3,    /* no gfx950 device / kernels not loadable */
  SVS_ERR_CAPACITY = 4,     /* caller-provided capacity too small */
  SVS_ERR_UNSUPPORTED = 5,
  SVS_ERR_BUSY = 6          /* the workgroups of a multi-workgroup kernel could not synchronise within its bounded wait (the device is shared with
                               other work): nothing was applied, the call may be retried */
};

#define SVS_NUM_PYR_LEVELS 3   /* global.h:107 */
#define SVS_MAX_CELLS 64

/* ---- POD types ---------------------------------------------------------------------------*/
typedef struct { double f, cx, cy, b; int32_t w, h; } svs_cam;   /* frame_grabber-impl.cpp:48-60 */

typedef struct {                       /* FastGrid, fast_grid.cpp:23-58 / keyframes.h:31-44 */
  int32_t gx, gy, cell_w, cell_h;
  int32_t min_inner, min_outer, max_inner, max_outer;
  int32_t fast_min, fast_max;
  int32_t thr[SVS_MAX_CELLS];
} svs_fastgrid;

typedef struct {                       /* CandidatePoint<3>, data_structures.h:37-69 */
  double xyz_anchor[3];
  double anchor_obs_pyr[3];
  int32_t anchor_level, kf_index, point_id, pad_;
} svs_candidate_point;

typedef struct {                       /* keyframe_map entry + vertex_map pose */
  double T_anchor_from_w[12];
  const uint8_t *pyr[3];               /* DEVICE pointers for svs_match */
  int32_t stride[3];
  int32_t pad_;
} svs_keyframe;

enum { SVS_MATCH_OK = 0, SVS_MATCH_NO_ANCHOR, SVS_MATCH_BORDER, SVS_MATCH_DEPTH,
       SVS_MATCH_TEXTURE, SVS_MATCH_NONE, SVS_MATCH_NO_DISP,
       SVS_MATCH_SKIPPED /* svs_frontend_*: a neighbour's new-point list behind matchAndTrack's cut (stereo_frontend.cpp:1000-1003) */ };

typedef struct {
  int32_t status, u, v, znssd;
  double obs[3];
  double xyz_actkey[3];
} svs_match_result;

typedef struct {                       /* GpuTrackingData, gpu/dense_tracking.cuh:28-277 */
  double H[21];                        /* packed upper-by-column */
  double b[6];
  double chi2;
  int64_t n_valid;
} svs_dense_sums;

typedef struct {                       /* addObsToG2o arguments, slam_graph-impl.cpp:44-97 */
  double obs[3];
  double info[3];
  int32_t point, pose, anchor, pad_;
} svs_ba_edge;

typedef struct {                       /* addConstraintToG2o, slam_graph-impl.cpp:99-126 */
  double T_21[12];
  double info[36];
  int32_t pose1, pose2;
} svs_ba_constraint;

typedef struct {                       /* OptParams slam_graph.hpp:36-50 + setupG2o/optimize */
  int32_t num_iters;
  int32_t use_robust;
  double huber_delta;
  double lambda_init;
  int32_t max_trials;
  int32_t self_edge_mode;              /* 0 = G2O_LITERAL, 1 = EXACT */
} svs_ba_params;

typedef struct {
  int32_t iterations, trials, accepted, terminated;
  double chi2_init, chi2_final, lambda_final;
} svs_ba_stats;

/* ---- context -----------------------------------------------------------------------------*/
typedef struct svs_ctx svs_ctx;
/* hip_stream: a hipStream_t to run on (e.g. torch's current stream), or NULL to create one */
int svs_ctx_create(int device, void *hip_stream, svs_ctx **out);
int svs_ctx_destroy(svs_ctx *ctx);
int svs_ctx_sync(svs_ctx *ctx);
/* experiment / test switches (0 = automatic choice): "trk_nwg" workgroups per stream of the latency-mode quarter-grid
   tracker, "trk_regs" its register budget (1: one workgroup per CU, 2: two), "full_nwg" workgroups per stream of the
   full-resolution tracker.  The environment (SVS_TRK_NWG, SVS_TRK_ONE_PER_CU / SVS_TRK_TWO_PER_CU, SVS_FULL_NWG) only
   supplies the initial values, read once by svs_ctx_create.  A/B switches between kernels that return the same results:
   "match_legacy" (0: four candidate points per wave where the search window allows it, 1: match_kernel, the round-1/2 kernel, 2: match_kernel2,
   one wave per point with the lean scan, where windows are narrower than a FAST cell), "mo_legacy" (1: the record-walking motion-only kernel), "fe_overlap" (default 1: the one-call
   front end enqueues FAST / block matching on a side stream beside the dense tracker; 0: everything on the context's stream),
   "xcd_swizzle" (default 1: tile kernels whose neighbours share image lines -- FAST score, pyramid, block matching, the four-points-per-wave matcher -- take their
   blocks in XCD-contiguous order; 0: the dispatcher's round robin), "fast_floor" (default 1: the FAST score kernel scores and lists only from the lowest threshold a
   cell's stored threshold lets the detection reach; 0: from the lowest threshold any cell can take),
   "trk_balance" (default 1: batches of two or more streams per CU launch the tracker's workgroups in the order of the LM work their streams needed in the
   last frame; 0: stream order; larger values count as 1; initial value from SVS_TRK_BALANCE), "trk_split" (default 10: in batches of more than one stream
   per CU, which run the flat tracker kernel, a stream still iterating after that many trials on the finest level is
   finished by a second launch with eight workgroups per stream -- same accept decisions, poses equal to 1e-12, a stream's bits independent of the rest of its batch; 0: one launch).
   A context and every handle made from it are used by ONE thread at a time. */
int svs_ctx_set_option(svs_ctx *ctx, const char *name, int value);
/* The accept test of the quarter-grid tracker: DenseTracker::denseTrackingCpu accepts an LM step iff `float chi2 - float new_chi2 > 0` on two sums accumulated
   sequentially in one float (dense_tracking.cpp:229-262, 341-383).  Default ("trk_lazy_chi2" = 1): the library takes exactly those decisions -- its f64 sums decide
   wherever their difference is outside the rigorous rounding-error bound of the float sums, and inside the bound the float sums themselves are formed, bit for bit.
   "trk_seq_chi2" = 1 forms every sum by the literal sequential chain (slow; cross-check), "trk_lazy_chi2" = 0 compares the f64 sums alone (rounds 1-4).
   Counters (blocking): "trk_exact_sums" float sums formed so far by this context's tracker launches, "trk_exact_fallbacks" how many of them needed the chain.
   Host-side counters of the spin gate (kernels whose workgroups wait for each other inside one launch -- latency-mode trackers, multi-workgroup solves -- are kept from
   starving each other across the contexts of a process; DenseTracker / SlamGraph::optimize on two threads, stereo_slam.cpp:196, backend.cpp:157-224):
   "spin_lane_launches" launches of this context that skipped the gate (<= 16 workgroups AND provably fitting beside everything of that kind in flight),
   "spin_gated_launches" launches that went through it.
   What the handles of the whole PROCESS hold right now (host-side, exact): "live_device_bytes" / "live_pinned_bytes" device / pinned memory owned by contexts and
   handles (not the caller's svs_malloc blocks), "live_sync_objects" events + streams the library created + recorded graphs. */
int svs_ctx_get_stat(svs_ctx *ctx, const char *name, long long *out);
void *svs_ctx_stream(svs_ctx *ctx);
const char *svs_last_error(svs_ctx *ctx);
int svs_malloc(svs_ctx *ctx, size_t bytes, void **d_ptr);
int svs_free(svs_ctx *ctx, void *d_ptr);
int svs_memcpy_h2d(svs_ctx *ctx, void *d_dst, const void *h_src, size_t bytes);
int svs_memcpy_d2h(svs_ctx *ctx, void *h_dst, const void *d_src, size_t bytes);  /* blocking */
/* hipEvent timing on the ctx stream (bench.py roofline leg) */
int svs_timer_start(svs_ctx *ctx);
int svs_timer_stop_ms(svs_ctx *ctx, float *ms);                                  /* blocking */

/* ---- preprocessing: replaces FrameGrabber::preprocessing, frame_grabber.cpp:285-336 --------*/
/* one cv::pyrDown step on u8 (cv::buildPyramid at :290), bit-exact to OpenCV semantics */
int svs_pyr_down_u8(svs_ctx *ctx, const uint8_t *d_src, int w, int h, int sstride, size_t s_bstride,
                    uint8_t *d_dst, int dstride, size_t d_bstride, int batch);
/* convertTo(CV_32F,1/255.) + Sobel(ksize=1) dx,dy (:315-333) */
int svs_convert_sobel_f32(svs_ctx *ctx, const uint8_t *d_src, int w, int h, int sstride,
                          size_t s_bstride, float *d_img, float *d_dx, float *d_dy, int fstride,
                          size_t f_bstride, int batch);

/* ---- stereo block matching: replaces StereoFrontend::calcDisparityCpu (stereo_frontend.cpp:620-653),
   i.e. cv::StereoBM(left pyr level 0, right, disp, CV_32F) with the state set there.  [cv::StereoBM is
   OpenCV 2.4.2, external; semantics as restated in oracle/stereo.c incl. its definitions D1/D2.] ---------*/
typedef struct {
  int32_t prefilter_cap;      /* stereo_frontend.cpp:626  (31)  */
  int32_t sad_window;         /* :627  (7; only 7 supported)    */
  int32_t min_disparity;      /* :628  (0; only 0 supported)    */
  int32_t num_disparities;    /* :636  (16 * ui.num_disp16 = 32; 16, 32, 48, ..., 160 supported: num_disp16 1..10 of :536 / :623) */
  int32_t texture_threshold;  /* :630  (10) */
  int32_t uniqueness_ratio;   /* :631  (15) */
  int32_t speckle_window;     /* :632  (100; 0 = no speckle filter) */
  int32_t speckle_range;      /* :633  (32)  */
  int32_t disp12_max_diff;    /* :634  (1; < 0 = no left-right check) */
} svs_stereo_params;
typedef struct svs_stereo svs_stereo;
/* scratch for `max_batch` independent w x h frames (prefiltered images, 16-bit disparity, cost, labels).  num_disparities + 6 <= w <= 20164 (38 at the 32
   disparities of the reference: three edge columns and four searched ones), h >= 2, num_disparities a multiple of 16 in 16..160, else SVS_ERR_UNSUPPORTED with
   nothing allocated: the left-right check and the whole-frame speckle filter hold one row in LDS, 8 w + 8 ceil(w / 64) bytes of the 160 KB a workgroup of the MI355X can have
   (requests above 64 KB are announced with hipFuncAttributeMaxDynamicSharedMemorySize at create).
   svs_ctx_get_stat of the context tells which kernels svs_stereo_compute chose, one step per call (host-side): "stereo_prefilter16_calls" (rows of 16 n pixels on
   4-byte aligned pointers and strides) / "stereo_prefilter4_calls" (everything else, or SVS_STEREO_PREFILTER4=1 at create), "stereo_strip_filter_calls" (speckle
   filter on strips of rows in LDS; "stereo_strip_filter_strips" adds up the strips per frame of those calls) / "stereo_frame_filter_calls" (the whole-frame union-find: rows too wide for 16 of them in LDS, h < 16, speckle_window >= 16368,
   or SVS_STEREO_FRAME_CCL=1 at create; SVS_STEREO_STRIP_KB=8..151 at create sets the LDS of a strip), "stereo_validate_wide_calls" (left-right check with one row
   per workgroup, w > 2048), "stereo_wide_search_calls" (the search kernels for any disparity count, which keep a pixel's window sums in LDS: every
   num_disparities but 32, and 32 too under SVS_STEREO_WIDE=1 at create; 32 otherwise runs the register-ring kernels, with the same result bit for bit).
   "stereo_speckle_error_mask" (blocking) is the OR of the bits the bounded walks of the speckle filter leave when one gives up (never
   expected; 0 = none since the context was created): 1 / 2 a find inside a strip, 4 a union inside a strip, 8 / 16 a find / a union on frame labels (across
   strips, and every walk of the whole-frame filter). */
int svs_stereo_create(svs_ctx *ctx, int w, int h, int max_batch, const svs_stereo_params *prm, svs_stereo **out);
int svs_stereo_destroy(svs_stereo *s);
/* d_disp[b][y*dstride + x] = disparity in pixels, (min_disparity - 1) where filtered (all device pointers;
   strides in elements, batch strides in elements of the respective type) */
int svs_stereo_compute(svs_stereo *s, const uint8_t *d_left, int lstride, size_t l_bstride, const uint8_t *d_right,
                       int rstride, size_t r_bstride, float *d_disp, int dstride, size_t d_bstride, int n_batch);

/* ---- grid FAST: replaces FastGrid (fast_grid.h:27-63) ----------------------------------------*/
typedef struct svs_fast svs_fast;
/* one FastGrid per level (stereo_frontend.cpp:73-88); `batch` independent threshold states */
int svs_fast_create(svs_ctx *ctx, int n_levels, const int32_t *w, const int32_t *h,
                    const svs_fastgrid *grids, int batch, int corner_cap_per_level,
                    svs_fast **out);
int svs_fast_destroy(svs_fast *f);
/* FastGrid::detectAdaptively(img, trials, qt) for all levels and `n_batch` slots
   (fast_grid.cpp:86-152); trials == 0 => FastGrid::detect at the stored thresholds (:60-83).
   d_img[l] = level-l image of slot 0. */
int svs_fast_detect(svs_fast *f, const uint8_t *const *d_img, const int32_t *stride,
                    const size_t *bstride, int n_batch, int trials);
/* blocking download of one slot/level: corners in the reference's quadtree insertion order
   (cells row-major, row-major inside the cell), per-cell counts, threshold used by the last
   detection of each cell, and the persistent thresholds (cell_grid2d()). Any pointer may be NULL */
int svs_fast_download(svs_fast *f, int slot, int level, int16_t *h_xy, int cap, int32_t *h_n,
                      int32_t *h_cell_count, int32_t *h_emit_thr, int32_t *h_thr_state);
int svs_fast_set_thresholds(svs_fast *f, int slot, int level, const int32_t *h_thr);
/* device view of a level's result for callers that chain their own kernels: the corner bitmap the matcher reads (1 bit per pixel, set = a corner of the last
   detection; pixel (x, y) of cell column ci = x / cell_w is bit x + (cell_column_bits - cell_w) * ci of the row at byte y * row_stride_bytes -- cell columns start
   on dword boundaries, rows end in >= 8 zero bytes) and the per-cell thresholds of that detection.  (API 7: replaces the dense score map of API <= 6.) */
int svs_fast_device_view(svs_fast *f, int level, const uint32_t **d_corner_bits, int32_t *row_stride_bytes, size_t *batch_stride_bytes,
                         int32_t *cell_column_bits, const int32_t **d_emit_thr, size_t *emit_bstride);

/* ---- guided matcher: replaces GuidedMatcher<StereoCamera>::match (matcher.hpp:67-83) --------*/
typedef struct {
  const svs_keyframe *d_kfs; int32_t n_kf;        /* keyframe table (device) */
  const svs_candidate_point *d_pts; int32_t n_pts; /* per slot: [n_batch][n_pts] */
  const double *d_T_cur_from_w;                    /* [n_batch][12] */
  const double *d_T_w_from_actkey;                 /* [n_batch][12] */
  const uint8_t *d_cur_pyr[3]; int32_t cur_stride[3]; size_t cur_bstride[3];
  const float *d_disp; int32_t disp_stride; size_t disp_bstride;
  svs_cam cam_vec[3];
  int32_t search_radius, thr_mean, thr_std;        /* 8, 22, 10 at stereo_frontend.cpp:989-1004 */
  int32_t n_batch;
  /* element distances between the tables of consecutive slots; 0 = the default: one keyframe table shared by all slots,
     point and result arrays packed [n_batch][n_pts] */
  size_t kf_bstride, pts_bstride, out_bstride;
} svs_match_args;
/* corners come from `f` (the feature_tree argument of the reference): candidate set and
   tie-break order are those of QuadTree::query. d_out: [n_batch][n_pts] */
int svs_match(svs_ctx *ctx, const svs_match_args *a, svs_fast *f, svs_match_result *d_out);

/* ---- optional sub-pixel refinement of a match: GuidedMatcher::subpixelAccuracy (matcher.cpp:241-309), which returnBestMatch calls (:198) and whose body the
   reference keeps behind `#if 0`.  For every record with status SVS_MATCH_OK: a 2-D Gauss-Newton alignment of the current image's 8 x 8 patch at the integer match
   (u, v) to the warped key patch (warpAffinve at half size 5, central-difference gradients, bilinear taps as interpolateMat_8u), at most `iterations` steps, stopped
   once a step is below `eps` on both axes; then createObervation at the refined f32 position (the disparity is read at its truncation).  tests/subpix_model.py is
   the definition, bit for bit.  Outcomes per record (svs_subpix_info::state):
     REFINED    obs rewritten from (u + dx, v + dy)
     NO_DISP    no positive disparity at the truncated refined position: status becomes SVS_MATCH_NO_DISP, obs stays
     SINGULAR   the key patch's normal matrix has det <= 0 (no texture, or a pure edge): the record stays as it is (the reference's live behaviour, :306)
     SHIFT      an iterate left [-max_shift, max_shift]^2, or (u, v) lies outside the matcher's own margin isInFrame(uv, 6) -- nothing is read then: the record stays
     UNTOUCHED  status was not SVS_MATCH_OK: the record is read no further than its status and not written
   u, v, znssd and xyz_actkey never change.  The solve of the 2 x 2 system is f64 (the reference's dead code: Eigen's f32 ldlt) -- a declared departure.
   Not covered: the registrar's two matches (svs_reg_*) and warpPatchProjective. */
typedef struct { int32_t iterations; float max_shift; float eps; int32_t pad_; } svs_subpix_params;  /* defaults 8, 1.5f, 0.03f */
void svs_subpix_params_default(svs_subpix_params *p);
enum { SVS_SUBPIX_REFINED = 0, SVS_SUBPIX_UNTOUCHED, SVS_SUBPIX_SINGULAR, SVS_SUBPIX_SHIFT, SVS_SUBPIX_NO_DISP };
typedef struct { float dx, dy; int32_t n_iter, state; } svs_subpix_info;   /* dx, dy: the offset the observation was made with (NO_DISP: asked for with); 0 where the
                                                                              record was kept.  n_iter: the Gauss-Newton steps computed, the refused one included */
/* refines d_results [n_batch][n_pts] (a->out_bstride apart) in place; a = the arguments svs_match was called with (its corners are not needed); d_info optional, laid
   out like d_results.  Asynchronous on the context's stream, like svs_match.  Refused (SVS_ERR_INVALID, nothing launched): max_shift outside (0, 2] -- with it every
   tap lies inside the image, columns u - 6 .. u + 6 --, iterations outside 1 .. 16, eps < 0. */
int svs_match_subpixel(svs_ctx *ctx, const svs_match_args *a, const svs_subpix_params *prm, svs_match_result *d_results, svs_subpix_info *d_info);

/* ---- motion-only refinement: replaces BA_SE3_XYZ_STEREO::calcFastMotionOnly (pose_optimizer.h:134-298) as
   called behind the matcher at stereo_frontend.cpp:1058-1063 ------------------------------------------------*/
typedef struct {
  int32_t robust_kernel;   /* PoseOptimizerParams(true, 2, 15): pose_optimizer.h:36-58 */
  int32_t num_iter;
  double kernel_param;
  double initial_mu;       /* -1 => tau * max diag(J^T J) (pose_optimizer.h:187-190) */
  double tau;              /* 1e-5 */
  int32_t min_obs;         /* matchAndTrack returns before calcFastMotionOnly with fewer than 20 observations (stereo_frontend.cpp:1053-1056):
                              with fewer than min_obs the pose is left untouched and status = 3; 0 = no minimum */
  int32_t pad_;
} svs_pose_opt_params;
/* PoseOptimizerParams(robust_kernel = true, kernel_param = 2, num_iter = 15) as the front end passes it (stereo_frontend.cpp:1061); initial_mu = -1, tau = 1e-5
   (pose_optimizer.h:36-58), min_obs = 0 */
void svs_pose_opt_params_default(svs_pose_opt_params *p);
typedef struct {           /* OptimizerStatistics, pose_optimizer.h:59-98 */
  double initial_chi2, chi2, max_err;
  int32_t num_obs;
  int32_t status;          /* 0 ok; 1 empty observation list (the reference asserts); 2 residual became NaN (the reference throws);
                              3 fewer than min_obs observations: nothing done (num_obs and initial_chi2 == chi2, max_err of the list at the pose as given).
                              Status 1 and 3 leave d_T_io untouched.  Status 2 stores the last ACCEPTED pose and its chi2 / max_err; the reference throws and the
                              test suite's CPU restatement of the loop hands back the INPUT pose.  The two coincide where the NaN is in the input (an observation or a point),
                              the one case the tests cover: no trial is ever accepted then */
} svs_pose_opt_stats;
/* obs_list / point_list = the SVS_MATCH_OK entries of d_results[b][0..n) in order (several svs_match outputs may be
   concatenated, as matchAndTrack appends into one TrackData); d_T_io[b][12] = T_cur_from_actkey in/out */
int svs_motion_only(svs_ctx *ctx, const svs_match_result *d_results, int n, size_t res_bstride, const svs_cam *cam,
                    const svs_pose_opt_params *prm, double *d_T_io, svs_pose_opt_stats *d_stats, int batch);

/* ---- gating of the matched points: the data-parallel part of StereoFrontend::processMatchedPoints
   (stereo_frontend.cpp:834-974), which runs right behind calcFastMotionOnly on the same TrackData ----------*/
typedef struct {           /* per matcher record; only meaningful where status == SVS_MATCH_OK */
  int32_t accepted;        /* |uvu - map_uvu(T xyz)| < max_reproj_error * 2^level (u, v), < 3 max_reproj_error (u_right): :869-871 */
  int32_t is_new;          /* id_obs.point_id < num_new_feat_matched (:920): goes to new_point_list, else track_point_list */
  double uv_pyr[2];        /* pyrFromZero_2d(uvu.head(2), anchor_level): point_tree insert position (:918), draw line start */
  double curkey_uv_pyr[2]; /* pyrFromZero_2d(se3xyz.map(SE3(), point), anchor_level) (:896-898) */
} svs_gated_point;
typedef struct {           /* PointStatistics (stereo_frontend.h) + the track-length accumulators (:857-858,925-926,966) */
  int32_t num_points_grid2x2[4];   /* [i * 2 + j], i from u, j from v (:875-880) */
  int32_t num_points_grid3x3[9];   /* [i * 3 + j] (:882-892) */
  int32_t num_matched_points[3];   /* per anchor level (:895) */
  int32_t num_track_points;
  int32_t num_obs;                 /* obs_list.size() */
  int32_t pad_[2];
  double sum_track_length;         /* av_track_length_ = sum_track_length / num_track_points (:966) */
} svs_point_stats;
/* d_results [batch][n] (res_bstride records apart) and d_pts [batch][n] (pts_bstride apart) are the arrays svs_match was
   called with / produced (concatenated calls allowed, as in matchAndTrack); records with index < n_new_records stem from
   the "new feature" match calls (stereo_frontend.cpp:989-1030), so an OK record is "new" iff its index is below that --
   the same split as point_id < num_new_feat_matched.  d_T [batch][12] = T_cur_from_actkey after calcFastMotionOnly.
   cam = level-0 stereo camera.  max_reproj_error: ui.max_reproj_error, default 2 (:845-846). */
int svs_process_matched_points(svs_ctx *ctx, const svs_match_result *d_results, const svs_candidate_point *d_pts, int n,
                               size_t res_bstride, size_t pts_bstride, int n_new_records, const svs_cam *cam,
                               const double *d_T, float max_reproj_error, svs_gated_point *d_gated, size_t gated_bstride,
                               svs_point_stats *d_stats, int batch);

/* ---- dense tracker: replaces DenseTracker / GpuTracker ---------------------------------------*/
/* computeDensePointCloudCpu (dense_tracking.cpp:393-423): quarter-grid cloud of one level */
int svs_pointcloud_cpu_sem(svs_ctx *ctx, const float *d_disp, int disp_stride, size_t disp_bstride,
                           const svs_cam *cam, int level, const double *d_T_cur_from_actkey,
                           float *d_cloud, size_t cloud_bstride, int batch);
/* one pass of denseTrackingCpu's loop body (dense_tracking.cpp:229-261 / :278-331), CPU-path
   semantics (quarter grid, clamp +-0.1, f64 geometry).  d_out[batch] */
int svs_dense_pass_cpu_sem(svs_ctx *ctx, const float *d_cloud, size_t cloud_bstride,
                           const uint8_t *d_prev_u8, int pstride, size_t p_bstride,
                           const float *d_cur, const float *d_dx, const float *d_dy, int fstride,
                           size_t f_bstride, const svs_cam *cam, const double *d_T, int do_jac,
                           svs_dense_sums *d_out, int batch);
typedef struct {                       /* one entry per chi2 evaluation of the dense trackers' LM loops */
  int32_t level;
  int32_t accepted;                    /* 1 / 0 = trial accepted / rejected (rho > 0: dense_tracking.cpp:142-144 / :367-369); 2 = the level's initial chi2 */
  float chi2, new_chi2;                /* chi2 before the trial, chi2 at the trial pose (both `float` in the reference) */
} svs_dense_lm_record;
/* whole DenseTracker::denseTrackingCpu(SE3*) (dense_tracking.cpp:222-391), device resident:
   3 levels x <=15 LM iterations with no host round trip. d_T_io [batch][12] in/out */
typedef struct {
  const float *d_cloud[3]; size_t cloud_bstride[3];
  const uint8_t *d_prev_u8[3]; int32_t pstride[3]; size_t p_bstride[3];
  const float *d_cur[3]; const float *d_dx[3]; const float *d_dy[3];
  int32_t fstride[3]; size_t f_bstride[3];
  svs_cam cam_vec[3];
  /* optional fused source: current u8 pyramid.  If d_cur_u8[0] != NULL the f32 image and its Sobel
     taps are formed on the fly from it (bit-identical values, ~1/8 of the HBM traffic) and
     d_cur/d_dx/d_dy are ignored, i.e. the convertTo/Sobel part of preprocessing can be skipped. */
  const uint8_t *d_cur_u8[3]; int32_t c8stride[3]; size_t c8_bstride[3];
  /* optional output [batch][3][12]: the pose the LAST H,b pass of each level ran at, i.e. the pose
     DenseTracker::residual_img[level] shows (dense_tracking.cpp:279-329); feed it to
     svs_dense_residual_image_cpu_sem.  NULL = not wanted. */
  double *d_T_jac_out;
  /* optional accept / reject record of the loop, [batch][record_cap] (+ the number produced per stream).  The reference repeats a
     rejected trial once (its undamped solve gives the identical step, so the identical rejection, then stops at trial == 2,
     dense_tracking.cpp:379-384); the device loop stops at the first rejection and records it once. */
  svs_dense_lm_record *d_record_out;
  int32_t record_cap;
  int32_t *d_n_record_out;
} svs_dense_track_args;
int svs_dense_track_cpu_sem(svs_ctx *ctx, const svs_dense_track_args *a, double *d_T_io,
                            int32_t *d_passes_out, int batch);
/* Diagnostic of the accept test above (tests): out[b] = the value of `float chi2 = 0; for (i < n) chi2 += t[b][i];` (dense_tracking.cpp:229-262) for batch rows of
   non-negative terms.  how = 0: formed as the tracker forms it (parallel, bit-identical by construction: csrc/seqsum.h), 1: the same with the terms read past the caches
   (latency mode), 2: by the literal sequential chain.  Rows 16-byte aligned and followed by >= 64 readable floats (bstride >= n + 64, a multiple of 4).
   d_fell_back (optional, [batch]): 1 where the chain was used after all (n > 20 480, or a failed self-check of how = 0 / 1). */
int svs_dense_seq_sum_f32(svs_ctx *ctx, const float *d_terms, int n, size_t bstride, int batch, int how, float *d_out, int32_t *d_fell_back);
/* DenseTracker::residual_img[level] (dense_tracking.cpp:52-54,279-329): float4 per quarter-grid sample as left by an
   H,b pass at pose d_T[b * T_bstride .. +12): (0,1,0,1) no depth, (1,0,0,1) out of frame, else grey 1 - 50 res^2.
   Either d_cur (f32 level image) or d_cur_u8 (fused source, as in svs_dense_track_args) must be given. */
int svs_dense_residual_image_cpu_sem(svs_ctx *ctx, const float *d_cloud, size_t cloud_bstride,
                                     const uint8_t *d_prev_u8, int pstride, size_t p_bstride,
                                     const float *d_cur, int fstride, size_t f_bstride,
                                     const uint8_t *d_cur_u8, int c8stride, size_t c8_bstride,
                                     const svs_cam *cam, const double *d_T, size_t T_bstride,
                                     float *d_res_img4, size_t res_bstride, int batch);
/* ---- full-resolution dense tracker: the CUDA build's DenseTracker / GpuTracker (dense_tracking.cpp:60-215,
   gpu/dense_tracking.cuh:281-342).  Per-pixel arithmetic = the reference's f32 code (pinned against the reference-compiled
   kernels, oracle/_ref); sums in f64.  The texture fetch tex2D(uv + 0.5f) is the exact-weight bilinear at
   RN(uv + 0.5f) - 0.5f with clamp addressing. ------------------------------------------------------------------------*/
/* FrameGrabber::preprocessing, CUDA branch (frame_grabber.cpp:291-313; filters :102-115): level 0 = convertTo(CV_32F, 1/255.),
   level l = gpu::pyrDown(level l-1) on f32, dx / dy = ksize-1 derivative with BORDER_REPLICATE on every level.
   d_img / d_dx / d_dy: `levels` device pointers each; level l has size ((w+1)/2.., (h+1)/2..). [cv::gpu is external: semantics
   as restated in oracle/vision.c] */
int svs_preprocess_gpu_sem(svs_ctx *ctx, const uint8_t *d_src, int w, int h, int sstride, size_t s_bstride,
                           float *const *d_img, float *const *d_dx, float *const *d_dy, const int32_t *fstride,
                           const size_t *f_bstride, int levels, int batch);
typedef struct {
  const float *d_cloud4[3]; int32_t stride_f4[3]; size_t cloud_bstride[3];   /* dev_ref_dense_points_[l]: float4 per pixel, strides in float4 */
  const float *d_prev[3];              /* prev_left().gpu_pyr_float32[l] */
  const float *d_cur[3];               /* cur_left().gpu_pyr_float32[l] */
  const float *d_dx[3], *d_dy[3];      /* gpu_pyr_float32_dx / _dy[l]; all NULL => the derivative taps are formed on the fly from d_cur
                                          (I(x+1) - I(x-1), REPLICATE: bit-identical to the filters of frame_grabber.cpp:102-115, 8 B/px less) */
  int32_t stride_f[3]; size_t f_bstride[3];
  int32_t w[3], h[3];
  double f[3], cx[3], cy[3];           /* cam_vec[l] intrinsics (narrowed to float as GpuIntrinsics::set does) */
  double *d_T_jac_out;                 /* optional [batch][3][12]: pose of the last jacobianReduction of each level = the pose the reference
                                          renders residualImage with (dense_tracking.cpp:177-186) */
  svs_dense_lm_record *d_record_out;   /* optional [batch][record_cap] */
  int32_t record_cap;
  int32_t *d_n_record_out;             /* optional [batch]: records the loop produced (may exceed record_cap; only the first cap are stored) */
} svs_dense_track_full_args;
/* whole DenseTracker::denseTrackingGpu(SE3*) (dense_tracking.cpp:60-193) for `batch` independent streams in ONE launch: levels 2..0,
   damped LM (H += mu diag(H), mu0 = 0.01f), <= 15 accepted steps per level, two rejections in a row stop.  d_T_io [batch][12] in/out.
   d_passes_out [batch] (optional): fused sweeps executed (one per chi2 evaluation), or -1 if the stream's workgroups could not
   synchronise (device oversubscribed; T is then unchanged garbage-free but NOT converged). */
int svs_dense_track_full(svs_ctx *ctx, const svs_dense_track_full_args *a, double *d_T_io, int32_t *d_passes_out, int batch);
/* parity probe: per-pixel terms of jacobianReduction_kernel before its reduction, d_terms8[v * w + u] = {J0..J5, res, valid};
   d_dx == d_dy == NULL selects the on-the-fly derivative taps */
int svs_dense_pixel_terms_full(svs_ctx *ctx, const float *d_cloud4, int w, int h, int stride_f4, const float *d_prev,
                               const float *d_cur, const float *d_dx, const float *d_dy, int stride_f, float f, float cx,
                               float cy, const float *h_T34_colmajor, float *d_terms8);
/* GpuTracker::jacobianReduction / chi2 (gpu/dense_tracking.cuh:291-342, .cu:172-263,376-453):
   full resolution, f32, no clamp; T is GpuMatrix34 (12 floats column-major) by value */
int svs_dense_pass_full(svs_ctx *ctx, const float *d_cloud4, int w, int h, int stride_f4,
                        const float *d_prev, const float *d_cur, const float *d_dx,
                        const float *d_dy, int stride_f, float f, float cx, float cy,
                        const float *h_T34_colmajor, int do_jac, svs_dense_sums *d_out);
/* GpuTracker::residualImage (gpu/dense_tracking.cuh:329-337, .cu:495-569); d_res_img4 has the cloud's stride */
int svs_dense_residual_image_full(svs_ctx *ctx, const float *d_cloud4, int w, int h, int stride_f4,
                                  const float *d_prev, const float *d_cur, int stride_f, float f,
                                  float cx, float cy, const float *h_T34_colmajor, float *d_res_img4);
/* computePointCloud (gpu/dense_tracking.cu:82-148) */
int svs_pointcloud_full(svs_ctx *ctx, const float *h_TQ_colmajor, const float *d_disp, int w, int h,
                        int stride_in, int stride_out, int factor, float *d_cloud4);
/* one level of DenseTracker::computeDensePointCloudGpu (dense_tracking.cpp:195-215) for `batch` streams with the poses on the DEVICE:
   TQ = T_cur_from_actkey^-1 * cam.Q() in double (products summed in ascending k), narrowed to float, then computePointCloud.
   d_T [batch][12]; cam = cam_vec[level]; factor = 2^level; strides in elements (float / float4), batch strides likewise */
int svs_pointcloud_full_pose(svs_ctx *ctx, const double *d_T, const svs_cam *cam, const float *d_disp, int disp_stride, size_t disp_bstride,
                             int w, int h, int stride_out, size_t cloud_bstride, int factor, float *d_cloud4, int batch);

/* ---- one call per frame: replaces the data-parallel part of StereoFrontend::processFrame(bool*) / processFirstFrame()
   (stereo_frontend.h:88-95, stereo_frontend.cpp:110-131,183-306) for one camera stream, HOST buffers in and out.  The stages are
   the entry points above, chained on the context's stream with no host round trip in between; keyframe switching / dropping and
   list building (stereo_frontend.cpp:265-296) are decided by svs_frontend_decide_keyframes below and applied by the caller. ----*/
typedef struct {
  int32_t fast_trials;                 /* 6 (stereo_frontend.cpp:232); the first frame uses one less (:118) */
  int32_t search_radius, thr_mean, thr_std;      /* 8, 22, 10 (:989-1004, CPU build) */
  float max_reproj_error;              /* ui.max_reproj_error = 2 (:845-846) */
  int32_t use_block_matching;          /* 0: a disparity image comes with every frame (have_disp_img); 1: calcDisparityCpu from the right image */
  svs_pose_opt_params pose_opt;        /* PoseOptimizerParams(true, 2, 15) (:1061) */
  svs_stereo_params stereo;            /* cv::StereoBM state (:620-653); used if use_block_matching */
  int32_t n_levels;                    /* use_n_levels_in_frontent (:68): pyramid levels FAST and the matcher run on; the code default is 2, the shipped
                                          configurations set 3.  0 = 3 */
  int32_t num_max_points;              /* ui.num_max_points (:1000): neighbours' new-point lists are matched while 2 * observations < this.  0 = 300 */
  int32_t min_matches;                 /* matchAndTrack fails below this many observations (:1053).  0 = 20 */
  int32_t cuda_build;                  /* 0: the reference's CPU build (quarter-grid denseTrackingCpu, computeDensePointCloudCpu; search_radius 8);
                                          1: its SCAVISLAM_CUDA_SUPPORT build (full-resolution denseTrackingGpu on f32 pyramids, computeDensePointCloudGpu;
                                          the caller passes search_radius 4, :1043-1047) */
} svs_frontend_params;
typedef struct {
  double T_cur_from_actkey[12];        /* after dense tracking and calcFastMotionOnly */
  int32_t dense_passes;                /* fused H,b / chi2 sweeps of the dense tracker (-1: its workgroups could not synchronise) */
  int32_t n_points;                    /* candidate points matched against (= records in h_matches / h_gated) */
  int32_t n_matched;                   /* SVS_MATCH_OK records = obs_list.size() */
  int32_t tracking_ok;                 /* n_matched >= 20: what matchAndTrack returns (stereo_frontend.cpp:1053-1056) */
  svs_pose_opt_stats pose_stats;
  svs_point_stats point_stats;
} svs_frame_result;
typedef struct svs_frontend svs_frontend;
/* cam = level-0 stereo camera (w, h multiples of 16).  max_points: capacity of the candidate list (ap_map); max_keyframes: keyframe slots */
int svs_frontend_create(svs_ctx *ctx, const svs_cam *cam, const svs_frontend_params *prm, int max_points, int max_keyframes, svs_frontend **out);
/* the same for n_streams independent camera streams (one front end each: own previous frame, keyframes, candidate points, FAST thresholds) whose
   stages run as ONE launch per stage.  Stream 0 is the one the host-buffer entry points (first_frame / process_frame / ...) talk to; they need n_streams == 1 */
int svs_frontend_create_batch(svs_ctx *ctx, const svs_cam *cam, const svs_frontend_params *prm, int max_points, int max_keyframes, int n_streams,
                              svs_frontend **out);
int svs_frontend_destroy(svs_frontend *fe);
/* processFirstFrame: pyramid, disparity, FAST (fast_trials - 1), reference cloud at the identity.  h_right or h_disp per use_block_matching */
int svs_frontend_first_frame(svs_frontend *fe, const uint8_t *h_left, int lstride, const uint8_t *h_right, int rstride, const float *h_disp, int dstride);
/* Frame::clone of the frame processed last into keyframe slot `slot` with its pose (keyframe_map entry + vertex_map pose) */
int svs_frontend_keep_keyframe(svs_frontend *fe, int slot, const double *T_kf_from_w);
int svs_frontend_keep_keyframe_of(svs_frontend *fe, int stream, int slot, const double *T_kf_from_w);
/* ... of ALL streams at once into slot `slot` of each; h_T_kf_from_w [n_streams][12] (one strided copy per level + one table upload) */
int svs_frontend_keep_keyframes(svs_frontend *fe, int slot, const double *h_T_kf_from_w);
/* ap_map: h_pts[i].kf_index = keyframe slot of the anchor (a slot svs_frontend_keep_keyframe has filled; < 0 = anchor frame not in keyframe_map,
   matcher.cpp:336-339); records [0, n_new_records) are the "new feature" candidates (:989-1030) */
int svs_frontend_set_candidates(svs_frontend *fe, const svs_candidate_point *h_pts, int n, int n_new_records);
/* the candidate lists of matchAndTrack (stereo_frontend.cpp:976-1050) in the order it walks them, for one stream: group 0 = newpoint_map[actkey_id],
   groups 1 .. n_groups-2 = newpoint_map[neighbour] in the order of active_vertex.strength_to_neighbors, group n_groups-1 = neighborhood_->point_list.
   h_group_end[g] = one past the last record of group g (n_groups >= 2, <= 64; h_group_end[n_groups-1] == n).  The neighbour lists behind the cut
   "2 * obs_list.size() < ui.num_max_points" come back with status SVS_MATCH_SKIPPED and take no part in the refinement or the gate. */
int svs_frontend_set_candidates_grouped(svs_frontend *fe, int stream, const svs_candidate_point *h_pts, int n, const int32_t *h_group_end, int n_groups);
/* the lists of ALL streams in one staged upload: h_pts = the streams' records back to back (h_n[b] of stream b), h_group_end [n_streams][n_groups] (the same
   number of groups for every stream; an absent list is an empty group) */
int svs_frontend_set_candidates_all(svs_frontend *fe, const svs_candidate_point *h_pts, const int32_t *h_n, const int32_t *h_group_end, int n_groups);
/* processFrame.  T_cur_from_actkey: the motion-model guess (in); T_actkey_from_w: pose of the active keyframe.  h_matches / h_gated:
   n_points records each (may be NULL).  Blocking, like the reference call. */
int svs_frontend_process_frame(svs_frontend *fe, const uint8_t *h_left, int lstride, const uint8_t *h_right, int rstride, const float *h_disp,
                               int dstride, const double *T_cur_from_actkey, const double *T_actkey_from_w, svs_frame_result *out,
                               svs_match_result *h_matches, svs_gated_point *h_gated);
/* processFrame in two halves (stream 0, n_streams == 1): submit stages the images, enqueues upload + all stages + the download and returns; wait blocks
   and hands the results out (h_matches / h_gated only if asked for at submit).  In between the caller is free -- e.g. to prefetch the next frame. */
int svs_frontend_submit_frame(svs_frontend *fe, const uint8_t *h_left, int lstride, const uint8_t *h_right, int rstride, const float *h_disp, int dstride,
                              const double *T_cur_from_actkey, const double *T_actkey_from_w, int want_matches, int want_gated);
int svs_frontend_wait_frame(svs_frontend *fe, svs_frame_result *out, svs_match_result *h_matches, svs_gated_point *h_gated);
/* upload the NEXT frame on a copy stream while the frame submitted last is being processed -- the reference's FrameData double buffer
   (frame_grabber.hpp:93-155: the grabber thread fills the next frame while the front end works on the current one).  The following
   first_frame / submit_frame / process_frame must pass NULL images. */
int svs_frontend_prefetch_frame(svs_frontend *fe, const uint8_t *h_left, int lstride, const uint8_t *h_right, int rstride, const float *h_disp, int dstride);
/* the pinned host buffers the NEXT frame is staged in (w x h each, contiguous; right image or disparity per use_block_matching): a frame grabber that writes
   its images straight into them and passes these pointers (stride = w) to the next first_frame / submit_frame / process_frame / prefetch_frame call saves the
   host-side copy (1.5 MB per 640 x 480 frame).  The pointers change with every such call (two staging sets) */
int svs_frontend_staging_view(svs_frontend *fe, uint8_t **h_left, uint8_t **h_right, float **h_disp);
/* ---- all streams at once, frames in DEVICE memory (camera DMA target, decoder output, another kernel's result) ---- */
typedef struct {                       /* images of all streams: stream b at + b * bstride (elements); unused members NULL */
  const uint8_t *d_left; int32_t lstride; size_t l_bstride;
  const uint8_t *d_right; int32_t rstride; size_t r_bstride;   /* use_block_matching */
  const float *d_disp; int32_t dstride; size_t d_bstride;      /* otherwise; read in place during the call, not copied */
  /* WHEN are these frames complete?  NULL: when the work enqueued on the context's stream before this call has run (a kernel or copy of the caller's on that
     stream may still be writing them at call time: the library reads them behind it, in stream order).  A hipEvent_t: when that event has fired -- the caller
     recorded it behind whatever produces the frames, on whichever stream.  Only then may the library read the frames on ANOTHER stream than the context's,
     which is what lets svs_frontend_process_frames build the pyramid of frame N + 1 beside the pose refinement of frame N ("fe_pipeline"). */
  void *ready_event;
} svs_frames_dev;
/* where the NEXT frames may be written in place (then pass in == NULL below): level-0 image, right image (NULL without block matching), disparity.
   Valid until the next first_frames / process_frames call, which moves on to other buffers */
int svs_frontend_input_view(svs_frontend *fe, uint8_t **d_left, int32_t *lstride, size_t *l_bstride, uint8_t **d_right, int32_t *rstride, size_t *r_bstride,
                            float **d_disp, int32_t *dstride, size_t *d_bstride);
/* processFirstFrame for every stream (blocking) */
int svs_frontend_first_frames(svs_frontend *fe, const svs_frames_dev *in);
/* processFrame for every stream: poses [n_streams][12] from the host; ASYNCHRONOUS on the context's stream, results stay on the device.
   The frames are read during the call chain, in place: they must stay untouched until the chain has run (svs_ctx_sync, or any blocking call of this front end),
   and in->ready_event says from when on they are valid (see svs_frames_dev). */
int svs_frontend_process_frames(svs_frontend *fe, const svs_frames_dev *in, const double *h_T_cur_from_actkey, const double *h_T_actkey_from_w);
/* blocking downloads after svs_frontend_process_frames: everything of one stream; refined poses [n_streams][12] + tracking flags of all (NULL = not wanted) */
int svs_frontend_results(svs_frontend *fe, int stream, svs_frame_result *out, svs_match_result *h_matches, svs_gated_point *h_gated);
int svs_frontend_poses(svs_frontend *fe, double *h_T_cur_from_actkey, int32_t *h_tracking_ok);
/* sub-pixel matches (svs_match_subpixel): the front end's steps run the pass behind their matcher from the next step on -- one launch between the matcher and
   matchAndTrack's cut, which therefore counts the observations left after the refinement (the reference refines inside match); the refinement, the gate and the
   records handed out see the refined observations.  prm == NULL switches it off (the state of a new front end): a step then runs exactly what it ran before the
   option existed.  Parameters are refused as svs_match_subpixel refuses them; not between submit_frame and wait_frame. */
int svs_frontend_set_subpixel(svs_frontend *fe, const svs_subpix_params *prm);
/* blocking: the svs_subpix_info records of one stream's last step, n_points of them (index = candidate index).  Refused while the option is off, and before a
   step has matched with it on. */
int svs_frontend_subpixel_info(svs_frontend *fe, int stream, svs_subpix_info *h_info);
/* profiling: hipEvents between the stages of the following process_frame(s) / submit_frame calls (off by default: an event costs ~4 us of stream time).
   svs_frontend_stage_times (blocking): ms[SVS_FRONTEND_STAGES] of the last such call, in the order of the reference's per_mon_ stages
   (stereo_frontend.cpp:190-302): preprocess (upload or copy + pyramid), dense tracking, stereo, fast, match, pose refinement (calcFastMotionOnly),
   process points, dense point cloud */
#define SVS_FRONTEND_STAGES 8
int svs_frontend_set_timing(svs_frontend *fe, int on);
int svs_frontend_stage_times(svs_frontend *fe, float *ms);
/* blocking: the accept / reject record of the dense tracker's LM loop of one stream in the last call (one entry per chi2 evaluation: level, accepted,
   chi2 before / after); *n = records produced, of which the first min(*n, cap, 64) are stored */
int svs_frontend_dense_records(svs_frontend *fe, int stream, svs_dense_lm_record *h_rec, int cap, int32_t *n);
/* computeDensePointCloudCpu / Gpu again at a pose decided after the frame (keyframe switch, :277-281, :298-302); T_cur_from_actkey [n_streams][12] */
int svs_frontend_recompute_cloud(svs_frontend *fe, const double *T_cur_from_actkey);
/* device views of one stream (tests, chaining): level images of the frame processed last, strides, its disparity (the caller's buffer if it passed
   one), reference clouds (quarter grid, or full resolution in the CUDA build), the FastGrid object (shared by all streams: slot = stream) */
int svs_frontend_device_view(svs_frontend *fe, int stream, const uint8_t **d_pyr_last, int32_t *stride, const float **d_disp, const float **d_cloud,
                             svs_fast **fast);

/* ---- new-point seeding of a keyframe: replaces StereoFrontend::addNewPoints / addMorePoints / addMorePointsToOtherFrame (stereo_frontend.cpp:682-823).
   Semantics restated in tests/seed_model.py.  Per problem and per level l = 0 .. n_levels-1 the level's FAST corners (x, y) are
   walked in a visiting order; n_l starts at n0[l]; with W x H the level-0 size (cam.w, cam.h), R = clearance, a corner is taken iff
     1. d = (double)disp[(y << l) * stride + (x << l)] * (1.0 / 2^l) > 0          (interpolateDisparity, maths_utils.cpp:38-44; NaN: not taken)
     2. 1 <= x << l < W - 1 and 1 <= y << l < H - 1                                  (isInFrame(uvi, 1); the device tests this first and reads no disparity outside)
     3. add_flags[i * 3 + j] != 0, i (j) = 0 / 1 / 2 by x << l (y << l) < third, < twothird, else, with third = (int)(W * (float)(1. / 3.)),
        twothird = (int)(W * 2 * (float)(1. / 3.)) evaluated in float as the reference does (:738-742), likewise for H
     4. no point p of the level's point tree has x - R <= p.x < x + R + 1 and y - R <= p.y < y + R + 1   (isWindowEmpty, quadtree.h:713-754, cv::Rect_::contains);
        the tree holds the caller's tree points of this level and the corners taken so far in this call.  The bounds are integers, so the test is exact on
        floor(p): the device keeps one occupancy bit per pixel of the level image (ceil(W / 2^l) x ceil(H / 2^l)) in LDS
   and then: anchor_obs_pyr = (x, y, x - d); xyz_cur = unmap_uvu(cam, anchor_obs_pyr * 2^l) as written in stereo_camera.cpp:46-52 (sd = (u0 - u2) / b; z = f / sd;
   x = ((u0 - cx) / f) * z; y = ((u1 - cy) / f) * z); xyz_anchor = T_newkey_from_cur * xyz_cur, row i = ((T[4i] x + T[4i+1] y) + T[4i+2] z) + T[4i+3], no contraction;
   anchor_level = l; kf_index as given; point_id = first_point_id + k for the k-th corner taken in the call, level 0's first (getNewUniqueId); the corner enters
   the tree; ++n_l, and the level ends once n_l > (num_max_points >> l) (:815-818) -- a level that starts above its cap still takes exactly one corner.
   The records leave in the order of the reference's newpoint_map[kf] list, which is push_front: the REVERSE of the order they were taken in.
   Departures from the reference: its QuadTree::insert drops a point closer than delta = 1 to the occupant of its leaf, the device keeps it (positions the front
   end produces are integers at their level, where this cannot occur); a tree point whose floor lies outside the level image is ignored (the reference asserts).
   Visiting order, per level: either the caller's list of indices into the level's corner list (svs_fast_download order; an index outside the list is skipped), or
   generated from a 64-bit seed and the corner list alone -- never from the problem's place in the batch: with h(x) = splitmix64(seed ^ x) (the mixer of
   svs_loop_check_batch above), the corner with list index i in cell c of level l (cells as svs_fast_download counts them) has a = h(1 << 62 | l << 32 | i),
   j = the number of corners i' of its cell with (a', i') < (a, i), b = h(2 << 62 | l << 48 | j << 16 | c); the corners are visited in ascending (j, b, c): round j
   takes one corner from every cell that still has one, the cells in a per-round hashed order -- even coverage before density, which is what the reference's
   QuadTree::EquiIter is for (its own order comes from VisionTools::Sample::uniform, third-party code). -------------------------------------------------------*/
typedef struct {
  int32_t clearance;          /* params_.newpoint_clearance (2); 0 .. 31 */
  int32_t num_max_points;     /* ui.num_max_points (300) */
  int32_t min_num_points;     /* ui.min_num_points (25): svs_frontend_seed_keyframes sets add_flags[k] = num_points_grid3x3[k] <= this (:322-331) */
  int32_t n_levels;           /* USE_N_LEVELS_FOR_MATCHING (3); 1 .. 3 */
} svs_seed_params;
void svs_seed_params_default(svs_seed_params *p);      /* 2 / 300 / 25 / 3 */
typedef struct {              /* one problem of svs_seed_points; lives in DEVICE memory */
  double T_newkey_from_cur[12];
  uint64_t seed;              /* of the generated order */
  int32_t add_flags[9];       /* [i * 3 + j] */
  int32_t n0[3];              /* (*num_points)[l] on entry, >= 0 */
  int32_t n_tree;             /* tree points of this problem */
  int32_t kf_index, first_point_id;
  int32_t use_order;          /* 1: the caller's index lists (n_order[l] entries at d_order[l]); 0: generated from the seed */
  int32_t n_order[3];
  int32_t pad_;
} svs_seed_problem;
typedef struct {              /* all pointers DEVICE; problem b at + b * (its batch stride) elements */
  const int16_t *d_xy[3]; size_t xy_bstride[3]; int32_t xy_cap[3];      /* corners (x, y) of level l in svs_fast_download order; at most xy_cap[l] are read */
  const int32_t *d_n[3]; size_t n_bstride[3];                            /* their number */
  const int32_t *d_cell_count[3]; size_t cell_bstride[3]; int32_t n_cells[3];      /* corners per cell (generated order only); n_cells <= SVS_MAX_CELLS */
  const float *d_disp; int32_t disp_stride; size_t disp_bstride;
  svs_cam cam;                                                           /* the level-0 StereoCamera */
  const svs_seed_problem *d_prob;                                        /* [batch] */
  const double *d_tree_xy; const int32_t *d_tree_level; size_t tree_bstride;       /* tree points [batch][tree_bstride]: (x, y) at their level, the level */
  const int32_t *d_order[3]; size_t order_bstride[3];                    /* the caller's visiting orders (problems with use_order) */
  int32_t batch;
} svs_seed_args;
/* `batch` independent problems, ASYNCHRONOUS on the context's stream.  d_out [batch][cap] records in list order, d_n_new [batch][3] the number taken per level
   (records of a problem: their sum).  cap < sum over the levels of (num_max_points >> l) + 1 -- the most a problem can produce: SVS_ERR_CAPACITY, nothing is written.
   A generated order needs xy_cap[l] <= 8192.  A problem's outputs are a function of that problem alone */
int svs_seed_points(svs_ctx *ctx, const svs_seed_args *a, const svs_seed_params *prm, svs_candidate_point *d_out, int cap, int32_t *d_n_new);
enum { SVS_SEED_FIRST = 0,   /* addNewPoints (:682-704): empty tree, every flag set, n0 = 0 */
       SVS_SEED_MORE = 1 };  /* addMorePoints behind addNewKeyframe (:316-331, :422-427): the tree holds the accepted gate records of the last step (uv_pyr at the
                                candidate's anchor_level), n0 = its num_matched_points, flags from its num_points_grid3x3.  SVS_ERR_INVALID unless the last
                                frame call was a step (not a first frame) and no candidate list was set since: the records must be that step's */
typedef struct {
  int32_t stream, mode;
  int32_t kf_index, first_point_id;
  double T_newkey_from_cur[12];        /* the identity for addNewPoints / addMorePoints */
  uint64_t seed;
  const int32_t *h_order[3];           /* HOST; all NULL: generated order.  Otherwise n_order[l] indices per level (a NULL level is not visited) */
  int32_t n_order[3];
  int32_t pad_;
} svs_seed_request;
/* the same from the front end's own device state, for n requests (several streams, or several keyframes of one): the corners of the last detection, the disparity
   of the frame processed last, the gate records and point statistics of the last step.  Ordered behind that step on the context's stream; one staged upload of
   the requests, one download of all records (with more than 1 MiB of output rows the counts come first and the records follow as one strided copy of the
   longest list's width; what a row of h_out holds behind its own records is then unspecified).  BLOCKING.  h_out [n][cap_per_request], h_n_new [n][3].  Works for the one-stream and the batch front end.
   The add_flags of a dropped frame and the lists behind it (stereo_frontend.cpp:265-296) come from svs_frontend_decide_keyframes; putting the seeded records
   into newpoint_map is the caller's */
int svs_frontend_seed_keyframes(svs_frontend *fe, int n, const svs_seed_request *req, const svs_seed_params *prm, svs_candidate_point *h_out, int cap_per_request,
                                int32_t *h_n_new);

/* ---- between the camera and processFrame: the three per-pixel input conversions of FrameGrabber::processNextFrame (frame_grabber.cpp:125-186), for a
   caller whose frames are raw (lens-distorted, colour, or depth instead of disparity).  Bit-exact to the OpenCV 2.4 semantics restated in
   tests/rectify_model.py.  The outputs are meant for the buffers svs_frontend_input_view hands out, followed by
   svs_frontend_first_frames / svs_frontend_process_frames with in == NULL (any n_streams, 1 included). ------------------------------------------*/
/* cv::initUndistortRectifyMap(K, dist, R, Knew, (w, h), CV_16SC2, map1, map2) as intializeRectifier() calls it (frame_grabber-impl.cpp:93-134): K, R, Knew
   row-major 3 x 3, dist = (k1, k2, p1, p2, k3) = cam.dist_*1..5.  map_xy [h][w][2] int16 (x0, y0), map_frac [h][w] uint16 (fx = frac & 31, fy = frac >> 5).
   Host only: needs neither a context nor a device.  f64 in a fixed operation order; an entry can differ from OpenCV's own by 1/32 px at a rounding tie (it
   accumulates along a row and inverts by LU), which is why svs_rectify_create takes MAPS: a host that has OpenCV passes rect_map_left_[0] / [1] as they are */
int svs_rectify_build_maps(const double *K, const double *dist, const double *R, const double *Knew, int w, int h, int16_t *map_xy, uint16_t *map_frac);
typedef struct svs_rectify svs_rectify;
/* w x h frames (w a multiple of 4, both <= 2046), at most max_batch streams per call.  Maps are HOST pointers in the layout above, copied (repacked) here;
   map_frac > 1023 anywhere: SVS_ERR_INVALID.  NULL maps for a side: conversion / copy only, no remap (data/newcollege.cfg: colour, already rectified).
   NULL right maps and never a right image: the disparity-given case */
int svs_rectify_create(svs_ctx *ctx, int w, int h, int max_batch, const int16_t *h_left_xy, const uint16_t *h_left_frac, const int16_t *h_right_xy,
                       const uint16_t *h_right_frac, svs_rectify **out);
int svs_rectify_destroy(svs_rectify *r);
typedef struct {                       /* raw frames of all streams in device memory: stream b at + b * bstride; strides in BYTES */
  const uint8_t *d_left; int32_t lstride; size_t l_bstride;
  int32_t left_channels;               /* 1: gray; 3: interleaved B, G, R -> cv::cvtColor(CV_BGR2GRAY) (framepipe.color_img, frame_grabber.cpp:140-147) */
  const uint8_t *d_right; int32_t rstride; size_t r_bstride;   /* gray; NULL: no right image */
  void *ready_event;                   /* as in svs_frames_dev: NULL, or the hipEvent_t behind whatever produces the frames */
} svs_raw_frames_dev;
/* rectifyFrame() (frame_grabber.cpp:245-256) for every stream: cv::remap(CV_INTER_LINEAR, BORDER_CONSTANT 0) of left and right through the handle's maps,
   colour conversion of the left image fused in.  ASYNCHRONOUS on the context's stream.  Output strides in elements, multiples of 4, pointers 4-byte aligned;
   d_right_out NULL exactly when raw->d_right is.  Correct for ANY map (a tap outside the source reads 0, decided per tap); fast for smooth lens maps */
int svs_rectify_frames(svs_rectify *r, const svs_raw_frames_dev *raw, uint8_t *d_left_out, int lstride, size_t l_bstride, uint8_t *d_right_out, int rstride,
                       size_t r_bstride, int n_batch);
/* depthToDisp() (frame_grabber-impl.cpp:136-152, stereo_camera.cpp:55-59; framepipe.depth_img, frame_grabber.cpp:163-170): 16-bit depth (1/5000 m) -> float
   disparity with cam->f and cam->b; cam->w x cam->h pixels per stream, strides in elements.  depth 0 gives +inf, as the reference does.  ASYNCHRONOUS */
int svs_depth_to_disp(svs_ctx *ctx, const svs_cam *cam, const uint16_t *d_depth16, int stride, size_t bstride, float *d_disp, int dstride, size_t d_bstride,
                      int n_batch);

/* ---- loop closure: the geometric check of PlaceRecognizer (placerecognizer.cpp:175-202) = cv::BFMatcher(NORM_L2).match + RanSaC<SE3Model>::compute
   (ransac.cpp:28-137, ransac_models.cpp:27-81,138-181, stereo_camera.cpp:36-52) for a batch of (query place, train place) pairs.  Descriptors come from any
   extractor (the reference's SURF is svs_surf_extract below, its bag of words svs_loop_add_locations; Sim3Model / MONO stay with the caller).  Semantics restated in tests/loop_model.py (not pinned).
   The handle holds a device-resident store of places, the counterpart of location_map_. -------------------------------------------------------------------*/
typedef struct svs_loop svs_loop;
/* desc_dim 64 or 128 floats per descriptor; at most max_desc descriptors per place (<= 2^21), max_places slots, max_hyp (<= 256) hypotheses per check,
   max_checks checks per call.  cam: the level-0 StereoCamera */
int svs_loop_create(svs_ctx *ctx, const svs_cam *cam, int desc_dim, int max_desc, int max_places, int max_hyp, int max_checks, svs_loop **out);
int svs_loop_destroy(svs_loop *l);
/* Place::descriptors [n][desc_dim], uvu_0_vec [n][3]; xyz_vec [n][3] = cam.unmap_uvu(uvu) is formed on the device (f64, as written in stereo_camera.cpp:46-52:
   sd = (u0 - u2) / b; z = f / sd; x = ((u0 - cx) / f) * z; y = ((u1 - cy) / f) * z) unless h_xyz is given.  Host arrays are staged before the call returns; the
   upload is ASYNCHRONOUS on the context's stream.  n < 1 or a bad slot: SVS_ERR_INVALID; n > max_desc: SVS_ERR_CAPACITY; any uvu with uvu[0] - uvu[2] <= 0 and
   no h_xyz: SVS_ERR_INVALID (addLocation keeps disp > 0 only, placerecognizer.cpp:230).  A failed call leaves the slot as it was */
int svs_loop_set_place(svs_loop *l, int slot, int n, const float *h_desc, const double *h_uvu, const double *h_xyz);
typedef struct {
  int32_t query_slot, train_slot;
  int32_t n_hyp;                       /* numRansac (100 at placerecognizer.cpp:190); 1 .. max_hyp */
  double pixel_thr;                    /* 2.5 (ransac.hpp:43) */
  uint64_t seed;                       /* of the device's draws; unused with h_samples */
  const int32_t *h_samples;            /* [n_hyp][3] match indices (e.g. the reference's own Sample::uniform stream), or NULL: the device draws */
} svs_loop_check;
typedef struct {
  int32_t n_matches;                   /* = descriptors of the query place */
  int32_t n_inliers;                   /* of the final pass; the caller applies > 30 (placerecognizer.cpp:198) */
  int32_t best_hyp;                    /* -1: none */
  int32_t n_invalid_hyp;
  double T_query_from_train[12];       /* [R | t] row-major; the identity when best_hyp == -1 */
} svs_loop_result;
/* n_checks geometric checks in one call (two launches, one upload, one download); BLOCKING: the results are on the host when it returns.
   Matching: match i has queryIdx = i and trainIdx = argmin_j |q_i - t_j|^2 (d2 = (|q|^2 + |t|^2) - 2 q.t in f32, clamped at 0; the lowest j wins an exact tie;
   no cross-check); distance = sqrt(d2).
   Samples: a hypothesis is three distinct match indices with pairwise distinct train indices (ransac.cpp:68-96; the query indices are the match indices).
   With h_samples the caller's triples are taken as they are, and one that breaks the rule (or leaves [0, n_matches)) makes its hypothesis invalid.  Otherwise
   draw number d = 0, 1, ... of hypothesis h (every draw counts, rejected ones too) is
       idx = mulhi32(splitmix64(seed ^ ((uint64)h << 32 | d)) >> 32, n_matches)             mulhi32(a, b) = (uint32)(((uint64)a * b) >> 32)
       splitmix64(z): z += 0x9E3779B97F4A7C15; z = (z ^ z >> 30) * 0xBF58476D1CE4E5B9; z = (z ^ z >> 27) * 0x94D049BB133111EB; return z ^ z >> 31
   with the reference's rejection structure: element 0 is one draw; element 1 is redrawn alone while it equals element 0; element 2 is redrawn alone while it
   equals element 0 or 1; then, if two of the three train indices are equal, the triple starts again at element 0.  The reference loops forever when no valid
   triple exists; here a hypothesis that would need a 65th draw is invalid.  An invalid hypothesis scores nothing, is never selected, is reported as -1 -1 -1
   and counted in n_invalid_hyp.
   Fit (SE3Model::calc_motion): p0 = unmap_uvu of the three query observations, p1 = the three train points, centroids with * (1.0 / 3.0), H = sum p1 p0^T,
   R = V U^T of its SVD (f64), V.col(2) negated when det R < 0, t = c0 - R c1.
   Score (belowThreshold): match i is an inlier of T when the three residuals of map_uvu(R x + t) against the query's uvu each have square < pixel_thr^2 (NaN and
   infinity compare false).  The best hypothesis is the first with the strictly greatest count, from bestinl = 0; without one, best_hyp = -1 and T stays the
   identity -- the final pass is still made with it (ransac.cpp:126-135).  n_matches < 3: n_inliers = 0, best_hyp = -1, identity, every hypothesis invalid.
   Outputs (each optional, HOST): h_results [n_checks]; h_train_idx, h_distance, h_inlier (the final pass, in match order) [n_checks][max_desc];
   h_samples_out [n_checks][max_hyp][3]; h_hyp_inliers [n_checks][max_hyp] -- behind a check's n_matches (n_hyp) the rows hold -1 (indices) and 0.
   A check's outputs are a function of that check alone: bit-identical whatever else is in the batch, and on every repetition.
   Bad or empty slots, n_hyp < 1: SVS_ERR_INVALID; n_hyp > max_hyp, n_checks > max_checks: SVS_ERR_CAPACITY -- before anything is launched */
int svs_loop_check_batch(svs_loop *l, int n_checks, const svs_loop_check *checks, svs_loop_result *h_results, int32_t *h_train_idx, float *h_distance,
                         uint8_t *h_inlier, int32_t *h_samples_out, int32_t *h_hyp_inliers);
/* profiling: bracket the two stages of every svs_loop_check_batch with events; ms[2] = distance stage, RANSAC stage of the last call */
int svs_loop_set_timing(svs_loop *l, int on);
int svs_loop_stage_times(svs_loop *l, float *ms);

/* ---- loop closure, the front half of PlaceRecognizer::addLocation (placerecognizer.cpp:248-318): visual words, the inverted index, TF-IDF place scores and
   the candidate test.  A place's descriptors are loaded beforehand: with svs_loop_set_place from the host, or with svs_loop_set_place_from_surf from the device
   arrays of svs_surf_extract (detection and description, placerecognizer.cpp:212-246).
   svs_loop_set_vocabulary: h_words [n_words][desc_dim] f32, the counterpart of words_ (data/surfwords10000.png: 9 983 x 64); squared norms are formed as for a
   place (f64 sum of the exact f32 squares, rounded once).  Allocates the index for the handle's max_places slots and resets it to EMPTY (a second call drops
   every location; the places themselves stay loaded).  BLOCKING.  n_words < 1: SVS_ERR_INVALID; n_words > SVS_LOOP_MAX_WORDS: SVS_ERR_CAPACITY.  The index is
   dense: n_words x max_places int32 counts */
#define SVS_LOOP_MAX_WORDS 1048576
int svs_loop_set_vocabulary(svs_loop *l, int n_words, const float *h_words);
typedef struct {
  int32_t slot;                        /* the place to add: loaded, not yet a location */
  int32_t do_loop_detection;           /* pr_data.do_loop_detection: 0 adds the location without scoring */
  const int32_t *h_exclude;            /* pr_data.exclude_set as slots, [n_exclude] (NULL with 0); the location's own slot is always excluded */
  int32_t n_exclude;
  float radius;                        /* 0.1f (placerecognizer.cpp:264): cvflann's L2 is the SQUARED distance, so this is a squared radius */
  float min_score;                     /* 2.0f (:316) */
} svs_loop_location;
typedef struct {
  int32_t number_of_words;             /* Place::number_of_words: descriptors that got a word */
  int32_t n_scored;                    /* location_stats.size(): slots that received a term */
  int32_t best_slot;                   /* max_score_idx as a slot; -1: none */
  float best_score;                    /* max_score; 0 with best_slot -1 */
  int32_t candidate;                   /* best_score > min_score: the pair (slot, best_slot) is worth a geometric check */
} svs_loop_location_result;
/* addLocation from :248 to :318 for n places IN ORDER: location k sees locations 0 .. k-1 of the same call in the index.  BLOCKING; one staged upload, one
   download and SIX launches whatever n and the descriptor counts are (reset of the call's work arrays, distances, word assignment + insertion, df / idf
   pre-pass, scores, commit of df).
   Word of descriptor r: argmin_j over the vocabulary of d2 = (|q|^2 + |w_j|^2) - 2 q.w_j in f32, clamped at 0, the lowest j wins an exact tie -- the matching of
   svs_loop_check_batch, evaluated pair by pair in the same way whatever the grid.  The word is assigned iff d2 < radius (f32 compare), otherwise it is -1
   (max_number_of_words = 1, :248).  The reference asks a hierarchical k-means tree with 32 checks, an approximate search that returns SOME word inside the radius
   and depends on OpenCV's k-means++ draws; the exact search is what it approximates.
   Index state: n_loc locations; nw[slot] = number_of_words of a location; cnt[w][slot] = occurrences of word w in it; df[w] = slots with cnt[w][slot] > 0.
   Adding a location, for r = 0 .. n-1 in descriptor order; a descriptor without a word is skipped, every other one adds 1 to number_of_words and
     1. if do_loop_detection and df[w] > 0 (calcLoopStatistics, :130-172): idf = (float)n_loc / (float)df[w]; for every slot o with cnt[w][o] > 0 that is neither
        this slot nor excluded: score[o] = score[o] + ((float)cnt[w][o] / (float)nw[o]) * idf -- quotient, product and sum each rounded to f32 on their own, no FMA,
        in descriptor order (the order is part of the result: a pairwise or f64 sum differs in most cases);
     2. if cnt[w][slot] == 0 then df[w] += 1; cnt[w][slot] += 1 (:287-296).
   So a word that repeats inside one keyframe meets a df that already counts that keyframe, and n_loc does not count the keyframe being added (:299 comes after
   the loop).  Afterwards nw[slot] = number_of_words and n_loc += 1, with or without do_loop_detection.
   Results: n_scored slots received a term; best_slot = the slot with the greatest score above 0, the LOWEST slot on a tie (the reference takes the first in
   hash-map order, which is not a function of its input); candidate = best_score > min_score.
   Outputs (each optional, HOST): h_results [n]; h_word (-1: none) and h_word_d2 (the squared distance to the nearest word, assigned or not) [n][max_desc] --
   behind a place's descriptor count the rows hold -1 and 0; h_scores [n][max_places], 0 for a slot without a term.
   A location's outputs are a function of the index state before it and of that location alone: bit-identical in a batch or alone, and on every repetition.
   Refused before anything is launched, the index unchanged: no vocabulary, a bad or empty slot, a slot that is already a location, an exclude slot outside
   [0, max_places), two locations of the call naming one slot: SVS_ERR_INVALID; n > max_checks: SVS_ERR_CAPACITY.
   svs_loop_set_place on a slot that is a location keeps its behaviour (the descriptors are replaced); the index keeps the counts it took */
int svs_loop_add_locations(svs_loop *l, int n, const svs_loop_location *locs, svs_loop_location_result *h_results, int32_t *h_word, float *h_word_d2,
                           float *h_scores);
/* profiling (svs_loop_set_timing): ms[2] = words stage (reset + distances), scoring stage (the other four launches) of the last svs_loop_add_locations */
int svs_loop_index_stage_times(svs_loop *l, float *ms);

/* ---- loop closure: training the visual vocabulary (what svs_loop_set_vocabulary takes).  The reference makes its words with a program of its own
   (create_dictionary.cpp:144-177: cvflann::hierarchicalClustering with KMeansIndexParams(32, 11, FLANN_CENTERS_KMEANSPP), a cut through a 32-ary k-means tree
   that yields 1 + 31 m words).  Here: FLAT Lloyd iterations with k-means++ seeding, which is what that cut approximates, and which yields the asked number of
   words.  Needs a context and no svs_loop handle.  Semantics restated in tests/vocab_model.py (not pinned by the reference's binaries).
   svs_vocab_train is BLOCKING.  h_desc [n][desc_dim] f32 on the host; every output is optional (NULL) and on the host.
   Refused before anything is uploaded or launched: desc_dim not 64 or 128, n < 1, n_words < 1, n_words > n, iterations < 0, a component of h_desc (or h_init)
   that is not finite or has |x| >= 4 (the pipeline's descriptors are unit vectors; the bound keeps every integer sum below 2^63): SVS_ERR_INVALID;
   n > 2^21 (SVS_VOCAB_MAX_POINTS), n_words > SVS_LOOP_MAX_WORDS: SVS_ERR_CAPACITY.
   1. Seeding (h_init NULL): k-means++ on the device.  splitmix64 and mulhi32 as for svs_loop_check_batch; mulhi64(a, b) = the high 64 bits of the 128-bit product.
        i_0 = mulhi32(splitmix64(seed) >> 32, n).  Every point has a weight w_i, +inf at first.  After centre c-1 (point i_{c-1}, row y) is chosen, for every
        point with row x:  s = 0.0; for k = 0 .. K-1: d = (double)x[k] - (double)y[k]; s = s + d * d   (f64, component order, no FMA);  w_i = min(w_i, s);
        the chosen point's own weight is 0.  W_i = (uint64)(w_i * 2^28), truncated; T = sum W_i (exact: any order gives the same value).  T == 0 ends the
        seeding with n_seeded = c words.  Otherwise r = mulhi64(splitmix64(seed ^ (1 << 62 | c)), T), and i_c is the smallest i whose inclusive prefix sum of
        W exceeds r.  Word c is row i_c of h_desc.  h_seed_index [n_words] gets the indices, -1 behind n_seeded.  TWO launches per step (weights + block sums;
        total, draw and search by one workgroup), queued without a host synchronisation in between: the chosen index stays on the device.
      With h_init the start centres are its rows, n_seeded = 0 and h_seed_index is all -1.
      The clustering goes on with k = n_seeded (h_init: n_words) words.
   2. Assignment.  The word of a point is argmin_j of d2 = (|x|^2 + |c_j|^2) - 2 x.c_j in f32, clamped at 0, the lowest j wins an exact tie: the arithmetic of
      svs_loop_add_locations pair for pair (the same tile walk and MFMA order; squared norms as svs_loop_set_vocabulary forms them).
   3. Update.  q = (int64)rint((double)x[k] * 2^38); per word and component sum_q = sum of q over the word's members in int64 (exact, so independent of the
      order); c[k] = (float)(((double)sum_q / (double)count) * 2^-38).  A word without members keeps its centre.
   4. One iteration = assignment, then update.  h_changed[t] = points whose word differs from iteration t-1 (n for t = 0).  The loop ends after the first
      iteration with changed == 0 (converged = 1) or after `iterations` of them; iterations_run counts them, and h_changed holds -1 behind it.
   5. Output.  With drop_empty, the words without a member in the LAST iteration's assignment are left out and the order of the others is kept; n_empty counts
      such words whether they are dropped or not (iterations == 0: there is no such assignment, n_empty = 0 and nothing is dropped).  n_words_out rows are
      written to h_words [n_words][desc_dim] (rows behind n_words_out are 0).  ONE MORE assignment is then made against the words as returned: it gives
      h_assign [n], h_assign_d2 [n] (the clamped f32 d2), h_count [n_words] (members per returned word, 0 behind n_words_out) and
      inertia_q28 = sum over the points of (uint64)((double)d2 * 2^28).  So h_assign / h_assign_d2 are what svs_loop_add_locations with radius = +inf gives for
      the same points against h_words.
   6. The outputs are a function of the inputs alone: bit-identical on every repetition, on every context, whatever the launch shapes.
   Flat, not hierarchical; weights are resolved to 2^-28. */
#define SVS_VOCAB_MAX_POINTS 2097152
typedef struct {
  int32_t n_words;                     /* asked; 1 .. SVS_LOOP_MAX_WORDS, <= n */
  int32_t iterations;                  /* Lloyd iterations at most; 11 (create_dictionary.cpp:150); 0: seeding + final assignment only */
  uint64_t seed;
  const float *h_init;                 /* [n_words][desc_dim] start centres, or NULL: k-means++ on the device */
  int32_t drop_empty;                  /* 1: words without a member in the last iteration's assignment are left out, order kept */
} svs_vocab_params;
typedef struct {
  int32_t n_words_out, n_seeded, iterations_run, converged, n_empty;
  uint64_t inertia_q28;
} svs_vocab_result;
/* n_words 10000, iterations 11, seed 0, h_init NULL, drop_empty 1 */
void svs_vocab_params_default(svs_vocab_params *p);
int svs_vocab_train(svs_ctx *ctx, int desc_dim, int n, const float *h_desc, const svs_vocab_params *prm, float *h_words, svs_vocab_result *h_res,
                    int32_t *h_seed_index, int32_t *h_assign, float *h_assign_d2, int32_t *h_count, int32_t *h_changed);
/* profiling: ms[3] = seeding, the assignment launches of all iterations, the update launches of all iterations of the context's last svs_vocab_train (events) */
int svs_vocab_stage_times(svs_ctx *ctx, float *ms);

/* ---- loop closure, the start of PlaceRecognizer::addLocation (placerecognizer.cpp:212-246): cv::SurfFeatureDetector(600, 2).detect on the keyframe's level-0
   image, the disparity filter, cv::SurfDescriptorExtractor(2, 4, 2, false).compute -- for a batch of keyframes, device images in, device places and host records
   out, no host round trip between the stages.  SURF is Bay, Ess, Tuytelaars, Van Gool, "Speeded-Up Robust Features", CVIU 2008; the arithmetic below restates
   OpenCV 2.4's surf.cpp from its definitions.  OpenCV is not part of the reference tree, so none of this is pinned by the reference's binaries (DESIGN.md
   section 4): the yardstick is the NumPy restatement tests/surf_model.py.  OpenCV ships SURF in its `nonfree` module; the feature therefore has a translation
   unit (surf.hip), a handle and a build switch of its own (make SURF=0: every svs_surf_* call and svs_loop_set_place_from_surf return SVS_ERR_UNSUPPORTED,
   svs_surf_params_default still fills the struct) and nothing else in the library depends on it.
   Everything is compiled without contraction.  cvRound = round half to even (rint) of the value widened to f64; "f32" means every operation rounds to f32.
   1. Integral image S: int32 [h + 1][w + 1], exact.  box(x1, y1, x2, y2) at origin (oy, ox) = S[oy+y1][ox+x1] + S[oy+y2][ox+x2] - S[oy+y2][ox+x1] - S[oy+y1][ox+x2].
   2. Responses.  Octave o < n_octaves, layer l < n_octave_layers + 2: size = (9 + 6 l) << o, step = 1 << o.  Patterns {x1, y1, x2, y2, weight} on a 9-grid:
      Dx {0,2,3,7,+1} {3,2,6,7,-2} {6,2,9,7,+1}; Dy {2,0,7,3,+1} {2,3,7,6,-2} {2,6,7,9,+1}; Dxy {1,1,4,4,+1} {5,1,8,4,-1} {1,5,4,8,-1} {5,5,8,8,+1}.  Scaled with
      ratio = (float)size / 9: every corner is cvRound(ratio * corner) (f32 product), weight = w / ((float)(x2 - x1) * (y2 - y1)) (f32).  A pattern's value is a
      DOUBLE accumulator over its boxes in the order written of (float)(int box sum) * weight (f32 product), cast to float.  det = dx * dy - (0.81f * dxy) * dxy,
      trace = dx + dy (f32).  Samples (i, j), i < 1 + (h - size) / step, j < 1 + (w - size) / step, have their origin at (i step, j step) and are stored at
      (i + margin, j + margin), margin = (size / 2) / step, of a layer of (h / step) x (w / step) that is zero elsewhere.
   3. Maxima, middle layers 1 .. n_octave_layers only.  border = (size of layer + 1 / 2) / step + 1; positions border <= i < rows - border (j alike) with
      val > hessian_threshold and val strictly greater than all 26 neighbours (N9[q][3 r + s] = layer - 1 + q at (i + r - 1, j + s - 1)).
      centre = step (i - (size / 2) / step) + (size - 1) * 0.5f for y (from i) and x (from j); laplacian = sign of trace.
   4. Refinement (f32).  b = (-(N9[1][5] - N9[1][3]) / 2, -(N9[1][7] - N9[1][1]) / 2, -(N9[2][4] - N9[0][4]) / 2);  A symmetric with
      A00 = N9[1][3] - 2 N9[1][4] + N9[1][5], A11 = N9[1][1] - 2 N9[1][4] + N9[1][7], A22 = N9[0][4] - 2 N9[1][4] + N9[2][4],
      A01 = (N9[1][8] - N9[1][6] - N9[1][2] + N9[1][0]) / 4, A02 = (N9[2][5] - N9[2][3] - N9[0][5] + N9[0][3]) / 4, A12 = (N9[2][7] - N9[2][1] - N9[0][7] + N9[0][1]) / 4,
      each evaluated left to right.  A x = b by LU with partial pivoting: for r = 0, 1, 2: the pivot row is the FIRST row q >= r of the largest |A[q][r]|; a pivot
      below 10 FLT_EPSILON in magnitude: no solution, the maximum is dropped; swap rows r and the pivot row (A from column r on, and b); d = -1 / A[r][r]; for
      q > r: alpha = A[q][r] * d, A[q][s] += alpha * A[r][s] for s > r, b[q] += alpha * b[r]; A[r][r] = -d.  Back substitution for r = 2, 1, 0: s = b[r],
      s -= A[r][q] * b[q] for q = r + 1 .. 2 in that order, x[r] = s * A[r][r].  Keep iff x != 0 and every |x_k| <= 1; then pt.x += x0 * step, pt.y += x1 * step,
      size = cvRound(size + x2 * (size - size of layer - 1)).
   5. Order: response descending, size descending, then y, x, octave, layer, i * cols + j ascending -- cv::KeypointGreater made total, so the order is a function
      of the image.  The first max_keypoints of that order are kept (overflow flag: there were more).
   6. Disparity filter (require_disparity; placerecognizer.cpp:222-238): rx = round((double)x), ry = round((double)y) (C round: half away from zero); a position
      outside the image drops the keypoint; d = (double)disp[ry][rx]; uvu = (x, y, x - d) in f64; keep iff d > 0 (a NaN drops) and uvu[0] - uvu[2] > 0 (a d
      below half an ulp of x would give a place that svs_loop_set_place refuses).  require_disparity 0 and no
      d_disp: every keypoint is kept and uvu = (x, y, x).
   7. Orientation.  s = size * 1.2f / 9.0f, haar = 2 cvRound(2 s); haar > h + 1 or > w + 1 removes the keypoint.  The 113 offsets (i, j), i outer, j inner, both
      -6 .. 6 with i^2 + j^2 <= 36, x offset i, y offset j, weight g[i + 6] * g[j + 6] (f32 product) with g = the 13-tap f32 Gaussian of sigma 2.5: cf_i =
      (float)exp(-0.5 / sigma^2 * x^2), x = i - (n - 1) / 2, sum the f32 taps in f64, g_i = (float)(cf_i * (1 / sum)).  Sample at x = cvRound((cx + i * s) -
      (float)(haar - 1) / 2) (y alike, f32); skipped unless 0 <= x < w + 1 - haar and 0 <= y < h + 1 - haar; no sample left removes the keypoint.  Patterns on a
      4-grid, scaled as in 2. with ratio (float)haar / 4: x {0,0,2,4,-1} {2,0,4,4,+1}, y {0,0,4,2,+1} {0,2,4,4,-1}; X = vx * weight, Y = vy * weight.  A sample's
      angle = deg(Y, X) := (float)(atan2((double)Y, (double)X) * 57.29577951308232, + 360 if negative).  72 windows q at 5 q degrees take, IN SAMPLE ORDER, the
      samples with d = |cvRound(angle) - 5 q|, d < 30 or d > 330, into f32 sums; the first window with the strictly greatest sumx^2 + sumy^2 (f32) wins;
      dir = deg(sumy, sumx); angle = 360 - dir, 0 where |angle - 360| < FLT_EPSILON.
      DEPARTURE: OpenCV's phase / fastAtan2 is a polynomial good to about 0.3 degrees; here both angles are f64 atan2.
   8. Descriptor (64 floats).  win = (int)(21 * s).  rad = dir * (float)(pi / 180); sin_dir = (float)sin((double)rad), cos_dir alike (DEPARTURE: f64 functions on
      the f32 argument, not sinf / cosf).  off = -(float)(win - 1) / 2; start_x = cx + off * cos_dir + off * sin_dir; start_y = cy - off * sin_dir + off * cos_dir;
      row i starts after i times (start_x += sin_dir, start_y += cos_dir); along a row pixel_x += cos_dir, pixel_y -= sin_dir (running f32 sums).  WIN[i][j] =
      image at (cvRound(pixel_y), cvRound(pixel_x)), both clamped to the image.  WIN is reduced to 21 x 21 by INTER_AREA's table: scale = win / 21 (f64); for
      destination d: f1 = d scale, f2 = f1 + scale, cell = min(scale, win - f1), s1 = ceil(f1), s2 = min(floor(f2), win - 1), s1 = min(s1, s2); taps in this
      order: (s1 - 1, (s1 - f1) / cell) if s1 - f1 > 1e-3; (s, 1 / cell) for s1 <= s < s2; (s2, min(f2 - s2, 1, cell) / cell) if f2 - s2 > 1e-3; weights f64,
      stored f32.  Horizontal pass first (f32 sum of (float)pixel * weight in tap order), then vertical (f32 sum of weight * value), cvRound, clamp to 0 .. 255.
      DEPARTURE: this table is used for every win, also multiples of 21 (OpenCV takes an integer fast path there).  For i, j < 20:
      vx = (float)(P[i][j+1] - P[i][j] + P[i+1][j+1] - P[i+1][j]) * DW[i][j], vy = (float)(P[i+1][j] - P[i][j] + P[i+1][j+1] - P[i][j+1]) * DW[i][j], DW = outer
      product (f32) of the 20-tap sigma 3.3 Gaussian.  4 x 4 cells of 5 x 5, cell (ci, cj) at index 4 (4 ci + cj): (sum vx, sum vy, sum |vx|, sum |vy|) in f32 in
      raster order.  mag = f64 sum over the 64 values in index order of the f32 squares; every value is multiplied by (float)(1 / (sqrt(mag) + DBL_EPSILON)).
   Keypoints removed in 6. - 8. leave every output array together, the order is preserved.  DEPARTURES from the reference: it reads the disparity image out of
   bounds for a keypoint that rounds outside (here: dropped), and asserts that the extractor removes nothing (here: uvu stays aligned with the descriptors).
   An image's outputs are a function of that image alone: identical bits alone or in a batch, at any stride, on every repetition (no float atomics; maxima are
   appended in arrival order to a list that is then RANKED by the total order of 5., and the list grows until it holds every maximum). */
typedef struct svs_surf svs_surf;
typedef struct {
  float hessian_threshold;                                  /* 600 */
  int32_t n_octaves, n_octave_layers;                       /* 2, 2 */
  int32_t require_disparity;                                /* 1: svs_surf_extract needs d_disp */
} svs_surf_params;
typedef struct { float x, y, size, angle, response; int32_t octave, laplacian, pad_; } svs_surf_keypoint;      /* 32 bytes */
#define SVS_SURF_STAGES 6      /* integral, responses, maxima + refinement, order, orientation + descriptor, filter / compaction */
void svs_surf_params_default(svs_surf_params *p);
/* w x h images, at most max_batch per call and max_keypoints per image.  cam: the level-0 StereoCamera (its w, h, where set, must be w, h).
   w h 255 >= 2^31: SVS_ERR_CAPACITY (the integral image is int32).  An image smaller than the largest filter ((9 + 6 (n_octave_layers + 1)) << (n_octaves - 1)),
   n_octaves outside 1 .. 4, n_octave_layers outside 1 .. 4, or a largest descriptor window whose work arrays exceed 64 KiB of LDS: SVS_ERR_UNSUPPORTED */
int svs_surf_create(svs_ctx *ctx, const svs_cam *cam, int w, int h, int max_batch, int max_keypoints, const svs_surf_params *prm, svs_surf **out);
int svs_surf_destroy(svs_surf *s);
/* BLOCKING.  d_img: u8 level-0 images (stride in bytes, bstride bytes between images), d_disp: f32 level-0 disparity (dstride, d_bstride in floats; NULL only
   with require_disparity 0) -- e.g. what svs_frontend_input_view and the stereo stage leave on the device.  Host outputs, each optional:
   h_count [n_batch]; h_overflow [n_batch]; h_kp [n_batch][max_keypoints]; h_uvu [n_batch][max_keypoints][3] f64; h_desc [n_batch][max_keypoints][64] f32 -- the
   first h_count[b] rows of image b are written, the others are left alone.  The same arrays stay on the device in the handle until the next call.
   n_batch < 1: SVS_ERR_INVALID; n_batch > max_batch: SVS_ERR_CAPACITY */
int svs_surf_extract(svs_surf *s, const uint8_t *d_img, int stride, size_t bstride, const float *d_disp, int dstride, size_t d_bstride, int n_batch,
                     int32_t *h_count, int32_t *h_overflow, svs_surf_keypoint *h_kp, double *h_uvu, float *h_desc);
/* loads slot `slot` of the loop handle from image `image_index` of the last svs_surf_extract, device to device; squared norms and xyz are formed exactly as
   svs_loop_set_place forms them, so the slot is bit-identical to svs_loop_set_place on the downloaded arrays.  The handle's count 0, a bad slot / image, or a last extract without disparity (uvu[0] - uvu[2] = 0,
   which svs_loop_set_place refuses): SVS_ERR_INVALID; count > the loop handle's max_desc: SVS_ERR_CAPACITY; desc_dim of the loop handle not 64: SVS_ERR_INVALID */
int svs_loop_set_place_from_surf(svs_loop *l, int slot, svs_surf *s, int image_index);
/* profiling: bracket the stages with events; ms[SVS_SURF_STAGES] of the last svs_surf_extract */
int svs_surf_set_timing(svs_surf *s, int on);
int svs_surf_stage_times(svs_surf *s, float *ms);

/* ---- back end: re-registration of a keyframe against the map.  Backend::localRegisterFrame (backend.cpp:190-199, 549-611) and Backend::globalLoopClosure
   (:201-219, 830-1001) share one shape -- project map points into a root keyframe (pointsVisibleInRoot :472-546 / the loop at :853-893), matchAndAlign
   (:725-784), gate and count (keyframesToRegister :615-722 / :904-961) -- and run here for a batch of requests as ONE chain of launches on the context's
   stream: one staged upload, one download, no host round trip in between.  The graph bookkeeping around the call (framesInNeighborhood, the hash-set
   deduplication of the point walk, registerKeyframes / addLoopClosure, new_edges_) stays with the caller of this stateless call -- on the resident map the walk
   is svs_map_frames_in_neighborhood, the registration svs_reg_register_map_batch and registerKeyframes / addLoopClosure svs_reg_commit, all below; the MONO /
   Sim3 branches are not covered.
   The cull and the counting are restated in tests/register_model.py (backend.cpp is not among the reference-compiled pins); the
   matcher, the refinement and the gate inequality are the entry points above.
   Chain, per request:
     1. cull (:506-526 / :861-878).  Source point i is kept iff its kf_index names an entry of the request's keyframe table, anchor_level is 0 .. 2, that
        entry has SVS_REG_KF_IN_WINDOW, and with T_root_from_anchor = T_root_from_world * inverse(T_anchor_from_w) (one 3x4 product per keyframe: rows
        (a0 b0 + a1 b1) + a2 b2, translation added last; inverse = transpose and -(R^T t) summed left to right; no contraction), p = T_root_from_anchor * xyz_anchor
        (row sums left to right), u = f (p0 / p2) + cx, v = f (p1 / p2) + cy with the camera of anchor_level: 0 <= (int)u < w and 0 <= (int)v < h, the casts
        truncating toward zero (so u = -0.5 is kept).  There is NO depth test: a point behind the camera that projects into the frame is kept, and the matcher
        answers it with SVS_MATCH_DEPTH.  The reference's cast is undefined for a non-finite projection; here a point whose |u| or |v| is not below 2^31 (NaN
        included) is dropped.  Survivors keep the source order.  in_vertex_table (:537-543, :887-892) is set for root_kf and for the anchor of every survivor.
        SVS_REG_LOCAL with fewer than covis_thr survivors: status 1 (:577).
     2. FastGrid::detect at the request's stored thresholds (recomputeFastCorners :452-469), GuidedMatcher::match at search_radius[0] from the identity,
        calcFastMotionOnly(PoseOptimizerParams(true, kernel_param, num_iter[0])), match at search_radius[1], calcFastMotionOnly(.., num_iter[1]) (:735-779).
        Fewer than covis_thr observations after the first match: status 2 (:751), after the second: status 3 (:780).  Both refinements take min_obs = covis_thr:
        where the reference returns false the pose stays as it was (the reference still refines behind :775 and discards the result).
     3. gate (:644-646 / :928-930): |du|, |dv| < reproj_thr * 2^anchor_level and |du_right| < 3 reproj_thr at the refined pose -- the inequality of
        svs_process_matched_points.  SVS_REG_LOCAL: every accepted observation counts for each keyframe of its point's observer row that is in the vertex table
        and is no direct neighbour (:650-696): strength, and the halves u > w / 2 | else, v > h / 2 | else of the level-0 image; a keyframe qualifies with
        strength >= covis_thr and every half >= covis_thr / 2 (integer division, :707-711); none qualifies: status 4 (:598).  SVS_REG_LOOP: the same counters for
        the frame as a whole in entry 0 of the request's svs_reg_kf_stats row (:934-961).
   A request that left at an exit costs nothing but its share of the launches: its candidate records are answered with SVS_MATCH_NO_ANCHOR from then on, its
   accepted flags and counters are 0.  A request's outputs are a function of that request alone, bit for bit, whatever else is in the batch and on every repetition. */
enum { SVS_REG_LOCAL = 0, SVS_REG_LOOP = 1 };
enum { SVS_REG_OK = 0, SVS_REG_FEW_CANDIDATES = 1, SVS_REG_FEW_MATCHES_PASS1 = 2, SVS_REG_FEW_MATCHES_PASS2 = 3, SVS_REG_NOT_COVISIBLE = 4 };
enum { SVS_REG_KF_IN_WINDOW = 1,        /* the keyframe is in graph_.double_window() (:506, :861) */
       SVS_REG_KF_DIRECT_NEIGHBOR = 2 };/* it is the root or one of directNeighborsOf(root) (:433-449); SVS_REG_LOCAL only */
typedef struct {
  int32_t covis_thr;                   /* graph_.covis_thr() (15) */
  int32_t search_radius[2];            /* 10, 4 (:746, :771); each <= 31 */
  int32_t thr_mean, thr_std;           /* 22, 10 */
  int32_t num_iter[2];                 /* 25, 15 (:758, :777) */
  int32_t pad_;
  double reproj_thr;                   /* REPROJ_THR 2.0 (:625, :904) */
  double kernel_param;                 /* 2 */
} svs_reg_params;
void svs_reg_params_default(svs_reg_params *p);
typedef struct {
  int32_t mode;                        /* SVS_REG_LOCAL / SVS_REG_LOOP */
  int32_t n_kf, n_src;
  int32_t root_kf;                     /* the root keyframe's entry of h_kfs: its pyramid is the cur_frame of match (device pointers, as svs_match takes them) */
  const float *d_root_disp;            /* DEVICE: the root frame's f32 disparity, level 0 */
  int32_t root_disp_stride, pad_;
  int32_t fast_thr[SVS_NUM_PYR_LEVELS][SVS_MAX_CELLS];      /* root_frame.cell_grid2d[level]: the stored per-cell thresholds, cells row-major; each >= 10 */
  double T_root_from_world[12];        /* v_root.T_me_from_world / T_loop_from_world (:845) */
  const svs_keyframe *h_kfs;           /* HOST [n_kf]: the vertex-table candidates with their poses, pyramids on the device */
  const uint8_t *h_kf_flags;           /* HOST [n_kf]: SVS_REG_KF_* bits */
  const svs_candidate_point *h_src;    /* HOST [n_src]: the points in the caller's iteration order, deduplicated; kf_index = entry of h_kfs of the anchor */
  const int32_t *h_obs_begin;          /* HOST [n_src + 1], SVS_REG_LOCAL: row i of the observer table is h_obs_kf[h_obs_begin[i] .. h_obs_begin[i + 1]) */
  const int32_t *h_obs_kf;             /* HOST: entries of h_kfs whose feature_table holds the point, each at most once per row; an entry outside the table is ignored */
} svs_reg_request;
typedef struct {
  int32_t status;                      /* SVS_REG_* */
  int32_t n_candidates, n_obs_pass1, n_obs_pass2, n_accepted;
  int32_t n_qualified;                 /* keyframes that qualify (SVS_REG_LOOP: 0 or 1) */
  double T_newroot_from_oldroot[12];   /* meaningful with status 0 and 4 */
  double T_pass1[12];                  /* the pose behind the first refinement */
  svs_pose_opt_stats stats_pass1, stats_pass2;
} svs_reg_result;
typedef struct {
  int32_t strength;                    /* point_list.size() (:706) */
  int32_t n_u_hi, n_u_lo, n_v_hi, n_v_lo;      /* u > w / 2, else, v > h / 2, else (:688-695, :936-943) */
  int32_t qualifies;
  int32_t in_vertex_table;
  int32_t pad_;
} svs_reg_kf_stats;
typedef struct svs_reg svs_reg;
/* cam: the level-0 StereoCamera.  At most max_requests requests per call, max_points source points, max_keyframes (<= 1024) table entries and max_observers
   observer-table entries per request.  The handle owns its svs_fast (one slot per request, the grids of stereo_frontend.cpp:73-88), its scratch and a pinned
   staging block */
int svs_reg_create(svs_ctx *ctx, const svs_cam *cam, int max_requests, int max_points, int max_keyframes, int max_observers, svs_reg **out);
int svs_reg_destroy(svs_reg *reg);
/* BLOCKING.  Outputs (each optional, HOST): h_res [n_requests]; per candidate, rows of max_points: h_cand_src (index of the candidate in h_src; -1 behind
   n_candidates), h_matches (the record of the second match; behind n_candidates SVS_MATCH_NO_ANCHOR), h_status_pass1 (the status of the first match),
   h_accepted (the gate), h_matches_pass1 (the whole record of the first match: tests); per keyframe-table entry, rows of max_keyframes: h_kf_stats (zero behind
   n_kf).  n_requests == 0: SVS_OK, nothing runs.  n_requests > max_requests or a request beyond the capacities of the handle: SVS_ERR_CAPACITY; a malformed
   request (NULL table, root_kf outside it, a threshold below 10, a decreasing observer row): SVS_ERR_INVALID -- both before anything is launched */
int svs_reg_register_batch(svs_reg *reg, int n_requests, const svs_reg_request *req, const svs_reg_params *prm, svs_reg_result *h_res, int32_t *h_cand_src,
                           svs_match_result *h_matches, int32_t *h_status_pass1, int32_t *h_accepted, svs_reg_kf_stats *h_kf_stats,
                           svs_match_result *h_matches_pass1);
/* profiling: events between the stages of every svs_reg_register_batch; ms[SVS_REG_STAGES] of the last call: cull (+ the copy of the root frames where they do
   not lie at one stride), FAST, match 1, refinement 1, match 2, refinement 2, gate */
#define SVS_REG_STAGES 7
int svs_reg_set_timing(svs_reg *reg, int on);
int svs_reg_stage_times(svs_reg *reg, float *ms);

/* ---- back end: the map kept on the device for re-registration.  svs_reg_register_batch is stateless: every request carries its keyframe table, its source points
   and its observer rows, which the caller has walked out of the graph (pointsVisibleInRoot, backend.cpp:472-546).  An svs_map keeps what those arrays are made
   from -- keyframes, points, and the (point, keyframe) pairs of every feature_table -- in device memory under the graph's own ids, is updated incrementally, and
   svs_reg_register_map_batch names a request by ids and does the walk on the device.
   Ids are dense 32-bit integers below the capacities (frame ids and point ids come from one counter in the reference, stereo_frontend.cpp:826-831), the
   convention of svs_ba_window_update.  max_keyframes <= 16384 (SVS_ERR_UNSUPPORTED above: the keyframe sets of a request are LDS bitmaps).
   Every update is one staged upload and at most two launches, ASYNCHRONOUS on the context's stream, and is refused as a whole -- the map unchanged, nothing
   uploaded -- on: an id outside the capacity or more entries than fit (SVS_ERR_CAPACITY), an id already present, an unknown id, an id twice in one call (SVS_ERR_INVALID).
   The host keeps the id sets and the set of pairs (as the window store of svs_ba_window_update does); removal is not offered (the reference's back end never removes). */
typedef struct svs_map svs_map;
int svs_map_create(svs_ctx *ctx, int max_keyframes, int max_points, int max_observations, svs_map **out);
int svs_map_destroy(svs_map *map);
/* h_keyframes [n]: T_me_from_world and the pyramid (device pointers; the images stay where the front end keeps them); h_disp_ptr / h_disp_stride [n]: the
   level-0 f32 disparity (device pointer, stride in elements); h_fast_thr [n][SVS_NUM_PYR_LEVELS][SVS_MAX_CELLS]: cell_grid2d, the stored thresholds, each of the
   SVS_MAX_CELLS entries per level in 10 .. 255 (unused cells: 25), else SVS_ERR_INVALID as svs_reg_register_batch refuses a threshold below 10.  The new
   keyframes are outside the window until svs_map_set_window names them */
int svs_map_add_keyframes(svs_map *map, int n, const int32_t *h_ids, const svs_keyframe *h_keyframes, const float *const *h_disp_ptr, const int32_t *h_disp_stride,
                          const int32_t *h_fast_thr);
/* h_points[i].kf_index holds the ID of the anchor keyframe, which must be in the map; point_id and pad_ are ignored (the record is stored with point_id = its id) */
int svs_map_add_points(svs_map *map, int n, const int32_t *h_ids, const svs_candidate_point *h_points);
/* point h_point_ids[i] is in the feature_table of keyframe h_kf_ids[i].  A pair already present (or twice in the call) is ignored: feature_table is a map */
int svs_map_add_observations(svs_map *map, int n, const int32_t *h_point_ids, const int32_t *h_kf_ids);
/* what restoreDataFromG2o changes (slam_graph.cpp:1035-1058): h_poses [n][12] T_me_from_world; h_xyz_anchor [n][3] */
int svs_map_set_poses(svs_map *map, int n, const int32_t *h_kf_ids, const double *h_poses);
int svs_map_set_points(svs_map *map, int n, const int32_t *h_point_ids, const double *h_xyz_anchor);
/* graph_.double_window(): exactly these keyframes have SVS_REG_KF_IN_WINDOW afterwards */
int svs_map_set_window(svs_map *map, int n, const int32_t *h_kf_ids);
/* host-side counts (each optional); n_observations counts distinct pairs */
int svs_map_info(svs_map *map, int32_t *n_keyframes, int32_t *n_points, int32_t *n_observations);

/* ---- back end: the double window's BA problem built from the map (SlamGraph::prepareForOptimization / optimize, slam_graph.cpp:288-355).
   svs_map_add_measured_observations is svs_map_add_observations (the same refusals, all or nothing, asynchronous, one staged upload, a pair already present or
   twice in the call ignored) for a caller that also wants to optimise: per NEW pair one svs_ba_edge record joins a device array in log order, "the measured
   store": obs = h_center[i] (feat.center), info = (s * s, s * s, 0.333 * 0.333) with s = 1 / 2^h_level[i] (slam_graph.cpp:1010-1015, formed on the host while
   staging), point / pose = the ids, anchor unused.  A level outside 0 .. SVS_NUM_PYR_LEVELS - 1: SVS_ERR_INVALID.  svs_map_measured_info (each optional)
   counts the pairs that came with a measurement and those that came through svs_map_add_observations without one. */
int svs_map_add_measured_observations(svs_map *map, int n, const int32_t *h_point_ids, const int32_t *h_kf_ids, const double *h_center /* [n][3] */,
                                      const int32_t *h_level /* [n] */);
int svs_map_measured_info(svs_map *map, int32_t *n_measured, int32_t *n_unmeasured);
/* computeActivePointsAndExtendOuterWindow (slam_graph.cpp:599-663) on the device.  The caller may keep computeInitialDoubleWin and the edge_table_ (svs_map_prepare_window_from_root finds both on the device): it passes W0 =
   double_window_ before the extension (ids, types 0 INNER / 1 OUTER, in its order) and the edge_table_ entries with at least one end in an INNER keyframe of W0,
   in either orientation.  The reference extends double_window_ only at the end (:662), so its result is a statement about sets:
     1. point p is ACTIVE iff some INNER keyframe F of W0 has p in its feature_table and either anchor(p) is in W0 or (F, anchor(p)) is among the pairs.  A point
        whose anchor enters the window only through another point, none of whose own INNER observers has a pair to that anchor, is not active;
     2. extension = { anchor(p) : p active, anchor(p) not in W0 }, typed OUTER;
     3. final window = W0 in the caller's order, then the extension in ASCENDING ID (the reference's order is that of an unordered_map);
     4. active list in ASCENDING POINT ID.
   n_edges_bound = the sum of the active points' observer-row lengths (an upper bound of the window's edges).  set_window_flags != 0 leaves exactly the final
   window with SVS_REG_KF_IN_WINDOW, as svs_map_set_window on it would.  h_window_ids / h_window_type (optional, [window_cap]): the final window, -1 behind it.
   BLOCKING: one staged upload (ids, types, pairs), at most the CSR rebuild plus two launches (one workgroup per INNER keyframe marks; ascending lists by
   popcount prefixes, no atomic decides an order), one download.
   SVS_ERR_INVALID before anything is uploaded: an unknown id, an id twice in W0, a type other than 0 / 1, no INNER keyframe, a pair naming an unknown keyframe,
   or a map that holds a pair without a measurement.  SVS_ERR_CAPACITY: n0 > window_cap, or window_cap > 256 (the solve's limit).  A final window above
   window_cap is only known on the device: SVS_OK with n_window = the count found and n_active = -1; nothing is prepared and the flags are untouched.
   The prepared window stays valid until the next svs_map_add_points / _add_observations / _add_measured_observations that changes the map, or the next
   svs_map_prepare_window; svs_map_set_poses / svs_map_set_points do NOT invalidate it (reinitializePoses, :665-725, runs between this step and optimize). */
typedef struct { int32_t n_window, n_initial, n_active, n_edges_bound; } svs_map_window_result;
int svs_map_prepare_window(svs_map *map, int n0, const int32_t *h_kf_ids, const int32_t *h_kf_type, int n_pairs, const int32_t *h_edge_pairs /* [n_pairs][2] */,
                           int set_window_flags, int window_cap, svs_map_window_result *h_res, int32_t *h_window_ids, int32_t *h_window_type);

/* ---- the pose graph's edges (EdgeTable, slam_graph.hpp:197-363) and their constraints (computeConstraint, slam_graph.cpp:787-846) ----
   One record per undirected edge, keyed (lo, hi) with lo < hi as the reference's Edge is.  The relative pose is stored ONCE, as T_lo_from_hi, and there is ONE
   info: every call site of setConstraint passes the same Lambda for both directions (slam_graph.cpp:457-461, :246-250, :897-898), so Lambda_1_from_2 and
   Lambda_2_from_1 of the reference's Edge are equal wherever they are set.  The host keeps the key set and the is_marginalized flags (every refusal happens
   before anything is uploaded); T and info live on the device alone.  A new edge has T and info zero and is not marginalised.
   Capacity: svs_map_reserve_edges (once, >= 1; a second call: SVS_ERR_INVALID).  Without it the table holds no edge and every edge call returns
   SVS_ERR_CAPACITY. */
typedef struct {
  int32_t lo, hi;                      /* lo < hi */
  int32_t strength, edge_type;         /* 0 LOCAL, 1 METRIC, 2 APPEARANCE */
  int32_t is_marginalized, pad_;
  double T_lo_from_hi[12];
  double info[36];
} svs_map_edge;
int svs_map_reserve_edges(svs_map *map, int max_edges);
/* insertEdge (:333-354) for n edges, either orientation: ASYNCHRONOUS, one staged upload and one launch.  SVS_ERR_INVALID (the reference asserts): an unknown
   keyframe, id1 == id2, an edge already present, an edge twice in the call, a type outside 0 .. 2; SVS_ERR_CAPACITY: more edges than reserved */
int svs_map_add_edges(svs_map *map, int n, const int32_t *h_pairs /* [n][2] */, const int32_t *h_strength, const int32_t *h_type);
/* setConstraint (:295-331) with a caller's own values: pose1 / pose2 name the edge, T_21 = T_pose2_from_pose1, info for both directions.  Stored as
   T_lo_from_hi: the device inverts T_21 where pose1 < pose2 (:327 for the other orientation); sets is_marginalized.  ASYNCHRONOUS, one upload, one launch.
   SVS_ERR_INVALID: an edge that does not exist, an edge twice in the call */
int svs_map_set_constraints(svs_map *map, int n, const svs_ba_constraint *h_cons);
/* unMarginalize (:235-240): clears the flag only, T and info stay.  ASYNCHRONOUS.  SVS_ERR_INVALID: an edge that does not exist, an edge twice in the call */
int svs_map_unmarginalize(svs_map *map, int n, const int32_t *h_pairs /* [n][2] */);
/* BLOCKING read-back of the records of the named edges (either orientation).  SVS_ERR_INVALID: an edge that does not exist */
int svs_map_get_edges(svs_map *map, int n, const int32_t *h_pairs /* [n][2] */, svs_map_edge *h_out);
/* the host-side counts (each optional) */
int svs_map_edge_info(svs_map *map, int32_t *n_edges, int32_t *n_marginalized);

/* computeConstraint (slam_graph.cpp:787-846) for a batch of keyframe pairs, one workgroup per request, as a statement that does not depend on hash order:
     common points   the points of kf1's feature_table that are also in kf2's, in ascending point id;
     anchor pose     of a common point: a pose override of the request if the anchor is named there; else the map's pose if the anchor has SVS_REG_KF_IN_WINDOW
                     (double_window_, :809-813); else its entry in the request's cached list (computeAbsolutePose results: the caller's own, or those of
                     svs_map_absolute_poses, which runs shortestPathToWindow on the map); else the request ends with SVS_CONS_MISSING_ANCHOR and returns the missing anchor ids
                     ascending, each once, up to missing_cap, with n_missing = their total count: the caller asks svs_map_absolute_poses (or walks its own graph) for exactly those and calls again;
     depth           d = || T1 inv(T_anchor) xyz_anchor || evaluated right to left on the vector: pose_act(T1, pose_act(pose_inv(T_anchor), xyz)), rows
                     ((a0 b0 + a1 b1) + a2 b2) + t, no contraction, sqrt((x x + y y) + z z) in f64;
     strength        the number of common points;
     median          maths_utils.h:114-136 over the multiset of depths: odd count the middle element, even count 0.5 * (a + b) of the two middle ones
                     (a radix select over the 64-bit patterns: positive doubles order as their bits; no cap on the count, no sort);
     T_12            T_1_from_2 = pose_mul(T1, pose_inv(T2));     norm_dist = || t(T_12) || / median;
     info            diag(s a, s a, s a, s b, s b, s b), dense, s = (double)strength, a = Po2((350 * 1.0) * norm_dist), b = Po2(100 * 1.0).
   Pose overrides (n_override <= 2: id, T[12]) replace the map's pose of that keyframe for the whole request, also where it serves as an anchor, whether or not
   it is in the window: registerKeyframes (:197-204) and addLoopClosure (:233-244) bring a vertex "temporarily" to another pose.
   strength == 0 (the reference's median asserts): SVS_CONS_EMPTY, T_12 still returned, median, norm_dist and info zero, nothing stored.  strength < covis_thr
   is only a warning in the reference (:833-836) and no error here: the caller decides.
   store != 0 with SVS_CONS_OK: setConstraint(kf1, kf2, T_12, info, info) is applied to the edge by the same launch (the edge must exist).
   h_missing [n][missing_cap] (optional when missing_cap == 0): -1 behind a request's ids.  h_depths [n][depth_cap] (optional, for tests): the depths in
   ascending point id with SVS_CONS_OK, zero behind them and with every other status.
   BLOCKING: one staged upload, at most the CSR rebuild plus one launch, one download; the host's is_marginalized mirror follows the statuses.
   Refused as a whole before the upload -- SVS_ERR_INVALID: an unknown keyframe, kf1 == kf2, n_override outside 0 .. 2, an override or cached id outside the
   map's capacity, a cached list that is not strictly ascending, a storing request without its edge, two storing requests for one edge (their order would decide
   the result); SVS_ERR_CAPACITY: more than SVS_MAP_CONS_MAX_REQUESTS requests, a cached list longer than the map's keyframe capacity, h_depths with depth_cap
   below the length of a kf1's feature_table. */
enum { SVS_CONS_OK = 0, SVS_CONS_EMPTY = 1, SVS_CONS_MISSING_ANCHOR = 2 };
enum { SVS_MAP_CONS_MAX_REQUESTS = 256 };
typedef struct {
  int32_t kf1, kf2, store, n_override;
  int32_t override_id[2];
  int32_t n_cached, pad_;
  double override_T[2][12];
  const int32_t *cached_ids;           /* [n_cached] strictly ascending */
  const double *cached_T;              /* [n_cached][12] T_anchor_from_world */
} svs_map_constraint_request;
typedef struct {
  int32_t status, strength, n_missing, pad_;
  double median, norm_dist;
  double T_12[12];
  double info[36];
} svs_map_constraint_result;
int svs_map_compute_constraints(svs_map *map, int n_requests, const svs_map_constraint_request *req, int missing_cap, svs_map_constraint_result *h_res,
                                int32_t *h_missing, int depth_cap, double *h_depths);

/* ---- the pose graph's walks on the map: computeInitialDoubleWin (slam_graph.cpp:555-596), framesInNeighborhood (:105-140), shortestPathToWindow +
   computeAbsolutePose (:64-103, :762-782), reinitializePoses (:665-725).  All four are one breadth-first search that pushes a vertex's neighbours in
   neighbor_ids_ordered_by_strength.rbegin() .. rend() order and drops duplicates at pop.  Two facts make it a function of the edge table alone:
     1. ADJACENCY COMES FROM THE EDGE TABLE.  Every insertion into neighbor_ids_ordered_by_strength (:222-225, :442-445) is paired with an insertEdge of the same
        strength, the strength is never updated, and a multimap keeps equal keys in insertion order.  The reverse walk of a keyframe's neighbours is therefore its
        edges in DESCENDING (strength, edge slot), the slot being the svs_map_add_edges log order; findNeighborsOfRoot (backend.cpp:287-309) walks the same row
        forwards.  The device keeps these rows as a CSR over keyframe ids, rebuilt by the first walk behind an svs_map_add_edges (count, scan, fill, a rank sort
        per row that is correct for a row of any length).
     2. VISITED-AT-POP EQUALS VISITED-AT-PUSH.  With a FIFO queue the order in which vertices are first popped is the order in which they are first pushed, and
        the copy that is processed carries the path, parent, parent pose and mark of the first pusher.  So the visit order is "frontier in order, each frontier
        vertex's row in order, first claim wins": a minimum over (visit index of the claimer, rank in its row), which no arrival order of an atomic changes.
   One workgroup per request; a request's bytes do not depend on the rest of its batch.  Every call is BLOCKING: one staged upload, at most the adjacency rebuild
   plus one launch (svs_map_prepare_window_from_root: plus svs_map_prepare_window's two and a second download), one download.  Refused as a whole before anything
   is uploaded -- SVS_ERR_INVALID: an unknown id, inner_size < 1 or >= double_size, size < 1; SVS_ERR_CAPACITY: more than SVS_MAP_WALK_MAX_REQUESTS requests,
   double_size > window_cap, a cap above 16384 (svs_map_prepare_window_from_root: window_cap > 256).  A map without svs_map_reserve_edges has no edges: every
   walk ends at its root.
   svs_map_initial_windows: per root the keyframes in visit order up to double_size (the walk stops exactly there, inside a row or a level, or earlier when the
     component is exhausted); the first inner_size visited are INNER (0), the rest OUTER (1).  h_ids / h_type [n][window_cap], -1 behind a request's count.
   svs_map_frames_in_neighborhood: the same search over the keyframes that have SVS_REG_KF_IN_WINDOW: a keyframe outside the window is skipped and not expanded,
     a root outside it gives count 0; at most `size` ids.  The reference returns a hash set; here the ids come in VISIT ORDER, h_ids [n][size], -1 behind the
     count, directly usable as h_walk_kf of svs_reg_register_map_batch.
   svs_map_absolute_poses: per keyframe x the path x .. w to the first keyframe w in visit order that is in the window (recognised before it would be expanded; x
     itself in the window: path length 1, T = its stored pose unchanged), then T = pose(w) and, from the back of the path to its front,
     T = pose_mul(rel(new, cur), T) with rel(1, 2) = getRelativePose_1_from_2 (:271-286): the edge's stored pose where is_marginalized is set (T_lo_from_hi
     when 1 is lo, pose_inv of it when 1 is hi), else pose_mul(pose(1), pose_inv(pose(2))); f64, rows ((a0 b0 + a1 b1) + a2 b2) + t, no contraction.
     h_status SVS_WALK_OK / SVS_WALK_NO_PATH (no window keyframe in x's component: the reference asserts; T zero, path length 0); h_path_len optional; h_T
     [n][12]; h_path [n][path_cap] (optional with path_cap 0): the first path_cap ids of the path from x, -1 behind them.
   svs_map_reinitialize_poses: the search from root_id over the keyframes that have SVS_REG_KF_IN_WINDOW (the new, extended window; others are skipped, not
     expanded, not marked).  A keyframe with a parent takes T = pose_mul(rel(me, parent), T_parent) if it or an ancestor is loop_id (-1: none), or if it is not
     among h_old_window; T_parent and the parent's pose inside rel are the parent's after its own update (level by level).  The root is never changed.  Writes
     the map's poses as svs_map_set_poses would; h_changed [changed_cap] (optional with 0): the changed ids in visit order, -1 behind them; *h_n_changed their
     total count.
   svs_map_get_poses: BLOCKING read-back of T_me_from_world [n][12] of the named keyframes.
   svs_map_prepare_window_from_root: the first two steps of prepareForOptimization (:297-298) from the root alone: the initial window is found on the device, the
     "edge_table_ entries with at least one end in an INNER keyframe" are the adjacency rows of its INNER keyframes, left on the device, and svs_map_prepare_window's
     two kernels run on them unchanged: result, window lists, flags and the prepared window are byte for byte those of svs_map_prepare_window called with that W0
     (visit order) and those pairs.  Everything else as svs_map_prepare_window states. */
enum { SVS_WALK_OK = 0, SVS_WALK_NO_PATH = 1 };
enum { SVS_MAP_WALK_MAX_REQUESTS = 256 };
int svs_map_initial_windows(svs_map *map, int n, const int32_t *h_root_ids, int inner_size, int double_size, int window_cap, int32_t *h_count, int32_t *h_ids,
                            int32_t *h_type);
int svs_map_frames_in_neighborhood(svs_map *map, int n, const int32_t *h_root_ids, int size, int32_t *h_count, int32_t *h_ids);
int svs_map_absolute_poses(svs_map *map, int n, const int32_t *h_kf_ids, int path_cap, int32_t *h_status, int32_t *h_path_len, double *h_T, int32_t *h_path);
int svs_map_reinitialize_poses(svs_map *map, int32_t root_id, int32_t loop_id, int n_old, const int32_t *h_old_window, int changed_cap, int32_t *h_n_changed,
                               int32_t *h_changed);
int svs_map_get_poses(svs_map *map, int n, const int32_t *h_kf_ids, double *h_poses);
int svs_map_prepare_window_from_root(svs_map *map, int32_t root_id, int inner_size, int double_size, int set_window_flags, int window_cap,
                                     svs_map_window_result *h_res, int32_t *h_window_ids, int32_t *h_window_type);

/* ---- inserting a keyframe: SlamGraph::addKeyframe (slam_graph.cpp:143-186) with computeStrength (:467-552), addNewPointsToMap (:358-397), addNewObsToOldPoints
   (:400-420) and addNewEdges(LOCAL) (:423-465) on the map, as a statement free of hash order.
   computeStrength.  E = the track entries whose global_id is a point of the map, in list order (an id listed twice counts twice).  The keys of the table are the
     anchors of all new points and every keyframe in the observer row of an entry of E.  No entry in E: strength(f) = the new points anchored in f.  Else, with
     h = max(covis_thr / 2, 1): an entry is LEFT if center[0] < half_width (a double against an int) else RIGHT, and TOP if center[1] < half_height else BOTTOM;
     t_q(f) = the list index of the h-th entry of E that f observes in class q; a key that lacks one of the four has strength 0; otherwise
     strength(f) = the number of entries at or behind max_q t_q(f) that f observes.  (The reference zeroes the table after EVERY track point, :532-550; the four
     counts only grow, which makes this closed form its outcome.)  The key table comes in ASCENDING KEYFRAME ID, at most SVS_MAP_ADDKF_MAX_NEIGHBORS keys: more
     are only known on the device, and the result then carries n_keys, over_capacity = 1 and nothing else (keys zero, masks zero).
   svs_map_compute_strength: BLOCKING, the map unchanged.  h_keys [SVS_MAP_ADDKF_MAX_NEIGHBORS] (zero behind n_keys): strength BEFORE the clamp of oldkey, the
     four class totals, edge = 0.  h_track_exists [n_track] (optional).  SVS_ERR_INVALID: an unknown anchor_id, covis_thr < 0.
   svs_map_add_keyframe: BLOCKING, the whole addKeyframe for one keyframe:
     1. strength(oldkey) = max(strength(oldkey), covis_thr); h_keys holds the table AFTER this clamp, edge = 1 where strength >= covis_thr.
     2. the new keyframe (pyramid, disparity, thresholds as svs_map_add_keyframes takes them; args->keyframe.T_anchor_from_w is ignored) with
        T_newkey_from_world = pose_mul(T_newkey_from_oldkey, T_oldkey_from_world), formed on the device in f64 without contraction; it is outside the window.
     3. every new point, in list order, whose anchor has strength >= covis_thr (h_new_kept) becomes a point (xyz_anchor, anchor_id, anchor_obs_pyr, anchor_level;
        normal_anchor is not stored) and brings the pairs (point, newkey) measured by feat_center / feat_level and (point, anchor) measured by
        anchor_obs_pyr * 2^anchor_level at anchor_level.
     4. every entry of E adds the pair (global_id, newkey) with its centre and level; the first occurrence of an id wins.
     5. every key with edge = 1, in ASCENDING KEY ID (the reference: unordered_map order; this order decides the edge slots), gets the LOCAL edge (key, newkey) of
        that strength, then computeConstraint(key, newkey) with setConstraint: h_cons [SVS_MAP_ADDKF_MAX_NEIGHBORS] takes one result per new edge in that order,
        h_missing [SVS_MAP_ADDKF_MAX_NEIGHBORS][missing_cap] their missing anchors under the rules of svs_map_compute_constraints (only the first n_edges entries
        / rows of the two are written; arrays of min(keyframes of the map, SVS_MAP_ADDKF_MAX_NEIGHBORS) entries are enough), args->cached_ids / cached_T as its
        requests have them.  An edge whose constraint ends SVS_CONS_EMPTY or SVS_CONS_MISSING_ANCHOR exists with T and info zero and not marginalised, as
        svs_map_add_edges leaves it: the caller completes it through svs_map_absolute_poses and a storing svs_map_compute_constraints.
     The map afterwards equals, byte for byte, one built by svs_map_add_keyframes, svs_map_add_points (the kept points in list order),
     svs_map_add_measured_observations (per kept point (point, newkey) then (point, anchor); then the first occurrences of E), svs_map_add_edges and one storing
     svs_map_compute_constraints.  One staged upload of the records, one small download (key table, masks), a second staged block of integers, the CSR rebuild,
     the constraint launch, one download.
     Refused before anything is uploaded, the map unchanged -- SVS_ERR_INVALID: an unknown oldkey, newkey present, an unknown anchor_id, a point_id already in the
     map or twice in the list or equal to a track global_id, a level outside 0 .. SVS_NUM_PYR_LEVELS - 1, covis_thr < 0, an oldkey that is no key of the table (no
     new point anchored there and no pair (existing track point, oldkey)); SVS_ERR_CAPACITY: an id beyond the
     capacities, fewer than 2 n_new + n_track free observations, fewer than min(keyframes of the map, SVS_MAP_ADDKF_MAX_NEIGHBORS) free edges.  More than
     SVS_MAP_ADDKF_MAX_NEIGHBORS keys: SVS_OK with over_capacity = 1, the map unchanged.
   svs_map_add_first_keyframe: addFirstKeyframe (:255-268): identity pose; SVS_ERR_INVALID unless the map holds no keyframe.
   svs_map_get_points / svs_map_get_feature_table: BLOCKING read-backs (what cloneDrawData reads).  get_points: the stored records (kf_index = the anchor's id) of
     points of the map.  get_feature_table: the points of kf_id's feature_table in ASCENDING POINT ID, *h_count their number (only the first cap are written), and
     per point the measurement record of the measured store; a pair that came without a measurement has obs and info zero and anchor = -1. */
enum { SVS_MAP_ADDKF_MAX_NEIGHBORS = 1024 };
typedef struct {                       /* NewTwoViewPoint, data_structures.h */
  double xyz_anchor[3];
  double anchor_obs_pyr[3];
  double feat_center[3];               /* feat_newkey.center */
  int32_t point_id, anchor_id, anchor_level, feat_level;
  int32_t pad_[2];
} svs_map_new_point;                   /* 96 bytes */
typedef struct {                       /* TrackPoint: global_id, feat */
  double center[3];
  int32_t global_id, level;
} svs_map_track_point;                 /* 32 bytes */
typedef struct { int32_t kf_id, strength, n_left, n_right, n_top, n_bottom, edge, pad_; } svs_map_key;
typedef struct { int32_t n_keys, m, over_capacity, n_edges; } svs_map_strength_result;
typedef struct {
  int32_t newkey_id, oldkey_id, covis_thr, half_width, half_height, disp_stride, n_new, n_track;
  double T_newkey_from_oldkey[12];
  svs_keyframe keyframe;
  const float *disp;                   /* DEVICE, level 0 */
  const int32_t *fast_thr;             /* HOST [SVS_NUM_PYR_LEVELS][SVS_MAX_CELLS] */
  const svs_map_new_point *new_points; /* HOST [n_new] */
  const svs_map_track_point *track_points;      /* HOST [n_track] */
  const int32_t *cached_ids;           /* HOST [n_cached] strictly ascending */
  const double *cached_T;              /* HOST [n_cached][12] */
  int32_t n_cached, pad_;
} svs_map_add_keyframe_args;
int svs_map_compute_strength(svs_map *map, int n_new, const svs_map_new_point *h_new, int n_track, const svs_map_track_point *h_track, int covis_thr, int half_width,
                             int half_height, svs_map_strength_result *h_res, svs_map_key *h_keys, int32_t *h_track_exists);
int svs_map_add_keyframe(svs_map *map, const svs_map_add_keyframe_args *args, int missing_cap, svs_map_strength_result *h_res, svs_map_key *h_keys,
                         int32_t *h_new_kept, int32_t *h_track_exists, svs_map_constraint_result *h_cons, int32_t *h_missing);
int svs_map_add_first_keyframe(svs_map *map, int32_t id, const svs_keyframe *h_keyframe, const float *disp, int32_t disp_stride, const int32_t *h_fast_thr);
int svs_map_get_points(svs_map *map, int n, const int32_t *h_ids, svs_candidate_point *h_out);
int svs_map_get_feature_table(svs_map *map, int32_t kf_id, int cap, int32_t *h_count, int32_t *h_point_ids, svs_ba_edge *h_meas);
/* svs_map_get_keyframe: a DIAGNOSTIC read-back (tests, debugging; nothing of the library or of the integration needs it).  BLOCKING: what the map stores of one keyframe -- the record (pose, pyramid pointers and strides), the disparity's device
   address and stride, the thresholds [SVS_NUM_PYR_LEVELS][SVS_MAX_CELLS]; every output optional.  SVS_ERR_INVALID: no keyframe of the map. */
int svs_map_get_keyframe(svs_map *map, int32_t kf_id, svs_keyframe *h_keyframe, const float **h_disp, int32_t *h_disp_stride, int32_t *h_fast_thr);
/* svs_map_add_keyframe_dev: BLOCKING.  svs_map_add_keyframe with the two lists in DEVICE memory of the map's context (d_new [args->n_new], d_track
   [args->n_track], 8-byte aligned, complete on the context's stream and unchanged until the call returns; args->new_points / track_points are ignored).  Steps
   1-5 above hold unchanged, the six outputs are those of svs_map_add_keyframe for the same lists, and the map afterwards is byte for byte the map that call
   builds.  No list record crosses the bus: one workgroup decides on the device what the host-list call decides about the records on the host, in front of the
   unchanged strength kernel; ONE download (status, the id columns of the host's mirrors, flags, result, key table, kept mask), the block of integers up, the
   apply and edge kernels, the CSR rebuild, the constraint launch, the final download -- one blocking round trip fewer than svs_map_add_keyframe.  The records may
   hold any bits: every id is range-checked on the device before it indexes anything.
   Refusals, the map unchanged.  PRECEDENCE: first what the arguments and the map's counts decide, in this order -- SVS_ERR_INVALID: covis_thr < 0, a negative
   count, a missing pointer; SVS_ERR_CAPACITY: a list of 2^24 entries or more; SVS_ERR_INVALID: an unknown oldkey, newkey < 0; SVS_ERR_CAPACITY: newkey beyond
   the capacity; SVS_ERR_INVALID: newkey present, a missing frame pointer, a threshold outside 10 .. 255, unordered cached ids; SVS_ERR_CAPACITY: fewer than
   2 n_new + n_track free observations, fewer than min(keyframes of the map, SVS_MAP_ADDKF_MAX_NEIGHBORS) free edges.  Then what the records decide, in the order
   svs_map_add_keyframe meets it, each phase by its entry of LEAST list index: (1) an anchor_id that is no keyframe: SVS_ERR_INVALID; (2) the new entries, per
   entry point_id < 0: SVS_ERR_INVALID, point_id beyond the capacity: SVS_ERR_CAPACITY, a point of the map or equal to an earlier new entry's id:
   SVS_ERR_INVALID, a level outside 0 .. SVS_NUM_PYR_LEVELS - 1: SVS_ERR_INVALID; (3) a track entry with such a level, or whose global_id (inside the capacity) is
   a new point_id of the call: SVS_ERR_INVALID (a track id that is negative or beyond the capacity names no point and is not refused); (4) an oldkey that is no
   key of the table: SVS_ERR_INVALID.  A call that breaks only rules about the records therefore returns what svs_map_add_keyframe returns for the same lists;
   one that also breaks a count rule returns that rule's status here, where svs_map_add_keyframe, which reads the records first, may return the records'.
   The first such call of a map (and the first after the map's keyframe or point set was changed by any other call) uploads the two id sets as bitmaps,
   (max_points + 16384) / 8 bytes; a map fed through this call keeps them current on the device.  Restated in tests/commit_kf_model.py. */
int svs_map_add_keyframe_dev(svs_map *map, const svs_map_add_keyframe_args *args, const svs_map_new_point *d_new, const svs_map_track_point *d_track,
                             int missing_cap, svs_map_strength_result *h_res, svs_map_key *h_keys, int32_t *h_new_kept, int32_t *h_track_exists,
                             svs_map_constraint_result *h_cons, int32_t *h_missing);

/* A request by ids.  The device builds the svs_reg_request of the stateless call from the map:
     1. source points.  SVS_REG_LOCAL: every point with at least one observation in a keyframe of h_walk_kf that is not the root and not in h_direct_kf
        (:481-497; the root is a direct neighbour, :433-449).  SVS_REG_LOOP: every point observed by h_walk_kf[0], the query keyframe (:853-858).  Each point
        once, in ASCENDING POINT ID (the reference's order is that of a hash set and no function of its input).
     2. keyframe table.  Entry 0 is the root; behind it, in ascending id, the anchor keyframes of the source points and the keyframes of h_walk_kf, each once.
        Flags: SVS_REG_KF_IN_WINDOW from the map, SVS_REG_KF_DIRECT_NEIGHBOR for the root and the ids of h_direct_kf.  The root's pyramid, disparity and
        stored thresholds come from the map; T_root_from_world from the request (the loop closure's is not the stored pose, :845).
     3. observer rows (SVS_REG_LOCAL): for each source point the table entries of the keyframes that observe it, ascending; observers outside the table are left out.
   From there the chain of svs_reg_register_batch runs unchanged: the outputs are byte for byte those of svs_reg_register_batch on that request.  h_kf_stats and
   h_cand_src refer to the built table and list. */
enum { SVS_REG_OVER_CAPACITY = 5 };    /* svs_reg_result.status of svs_reg_register_map_batch only */
typedef struct {
  int32_t mode;                        /* SVS_REG_LOCAL / SVS_REG_LOOP */
  int32_t root_kf;                     /* id */
  int32_t n_walk, n_direct;            /* each <= the registrar's max_keyframes; SVS_REG_LOOP: n_walk >= 1 */
  double T_root_from_world[12];
  const int32_t *h_walk_kf;            /* HOST [n_walk]: framesInNeighborhood(root) (the caller's, or svs_map_frames_in_neighborhood's) / the query keyframe */
  const int32_t *h_direct_kf;          /* HOST [n_direct]: directNeighborsOf(root); the root need not be listed */
} svs_reg_map_request;
/* BLOCKING: one staged upload of ids, one download, no host synchronisation in between (the first call behind an svs_map_add_observations also rebuilds the
   map's two CSR views on the stream; the first call with more requests than any before allocates the walk's bitmaps).  map and reg belong to one context.
   Outputs as svs_reg_register_batch, and (each optional, HOST): h_cand_point_id [n_requests][max_points]: the built source list's point id of every candidate
   (-1 behind n_candidates); h_kf_ids [n_requests][max_keyframes]: the ids of the built table (-1 behind it); h_n_kf [n_requests]: its length.
   A built table above the registrar's max_keyframes, a source list above max_points or observer rows above max_observers are only known on the device: that
   request is answered with status SVS_REG_OVER_CAPACITY, every other byte of its outputs zero (h_n_kf 0), the call returns SVS_OK and the other requests of the
   batch are unaffected.  An unknown id in a request, a root whose pyramid or disparity is narrower than the registrar's camera: SVS_ERR_INVALID before anything is
   launched.  A request's outputs are a function of the map's content and of that request alone: not of the order or grouping of the updates that built the map,
   of the rest of the batch, or of repetition. */
int svs_reg_register_map_batch(svs_reg *reg, svs_map *map, int n_requests, const svs_reg_map_request *req, const svs_reg_params *prm, svs_reg_result *h_res,
                               int32_t *h_cand_src, svs_match_result *h_matches, int32_t *h_status_pass1, int32_t *h_accepted, svs_reg_kf_stats *h_kf_stats,
                               svs_match_result *h_matches_pass1, int32_t *h_cand_point_id, int32_t *h_kf_ids, int32_t *h_n_kf);

/* ---- committing a registration or a loop closure into the map: SlamGraph::registerKeyframes (slam_graph.cpp:188-205) and SlamGraph::addLoopClosure (:207-251)
   with addNewObsToOldPoints (:400-420) and addNewEdges(METRIC) (:423-465), where Backend::localRegisterFrame (backend.cpp:601-604) and globalLoopClosure
   (:964-971) end.  As a statement free of hash order, for request i of the registrar's last svs_reg_register_map_batch on the map:
     T_new = pose_mul(res[i].T_newroot_from_oldroot, req[i].T_root_from_world), f64, rows ((a0 b0 + a1 b1) + a2 b2) + t, no contraction, formed on the device
     (:601-602, :964-966; the loop request's T_root_from_world already is inverse(T_query_from_loop) * T_query_from_w).
   SVS_REG_LOCAL with status SVS_REG_OK:
     track list    the candidates with accepted != 0 whose source point has, in its observer row, at least one table entry with qualifies != 0; in candidate
                   order, which is ascending point id.  (The reference's list holds a point once per qualifying observer, :714-718; feature_table.insert keeps the
                   first and all copies carry one feature, so each point appears once here.)  Feature = ImageFeature<3>(uvu, anchor_level): centre = obs of the
                   second match's record, level = the candidate's anchor_level (:663-664).
     pairs         every track point whose pair (point, root) is not yet in the map adds it with that measurement, as svs_map_add_measured_observations records
                   it (info from the level); a pair already present keeps what it has.
     edges         every qualifying keyframe gets, in ASCENDING KEYFRAME ID (the reference: unordered_map order; this order decides the edge slots, as in
                   svs_map_add_keyframe), the edge (keyframe, root) of type METRIC (1) with strength = its svs_reg_kf_stats.strength, then computeConstraint(keyframe,
                   root) + setConstraint with the root's pose overridden by T_new for that computation only (:197-204).  The stored pose of the root is unchanged.
   SVS_REG_LOOP with status SVS_REG_OK (entry 0 qualifies), loop = the request's root, query = h_walk_kf[0]:
     track list    every accepted candidate (:945-950), in candidate order; pairs (point, loop) as above.
     edge          one edge (query, loop) of type APPEARANCE (2), strength = the number of accepted candidates (slam_graph.cpp:214: the list's length, not the number
                   of new pairs), then computeConstraint(loop, query) with loop overridden by T_new (:233-250).
   Any other status: SVS_OK, committed = 0 in the result, the map unchanged.
   The constraints follow every rule of svs_map_compute_constraints: the cached anchor list comes with the call, missing anchors are reported per edge up to
   missing_cap, an edge that ends SVS_CONS_MISSING_ANCHOR exists with T and info zero and is not marginalised, as svs_map_add_keyframe leaves it (the caller
   completes it through svs_map_absolute_poses and a storing svs_map_compute_constraints with the same override).  SVS_CONS_EMPTY cannot occur: each new edge has
   at least covis_thr common points once the pairs are in.
   svs_reg_commit: BLOCKING.  The lists are taken where the registration left them on the device (candidate records, accepted flags, the second match's records,
     observer rows, keyframe statistics, table ids): one launch builds the track list and the edge list there, one small download (counts, track point ids,
     edge list), the host decides every refusal and the mask of new pairs, one staged block of integers, append by prefix sums, svs_map_add_edges' kernel, the
     CSR rebuild, svs_map_compute_constraints' kernel, one download: one more host synchronisation than the registration alone.  ONE request per call; several
     requests of one batch may be committed one after the other, each with what the registration computed (nothing is recomputed; the mask of new pairs is taken
     against the map as it is then).  Any later registration call on the handle ends the batch.  At most the registrar's max_keyframes qualifying keyframes.
     Outputs: h_res; h_edge_kf / h_edge_strength [max_keyframes] (optional): the other end of every new edge (LOOP: the query) and its strength, -1 / 0 behind
     n_edges; h_cons [max_keyframes] and h_missing [max_keyframes][missing_cap]: the first n_edges entries / rows are written; h_track_point_ids / h_track_added
     [track_cap] (optional): the track list's point ids and whether each brought a new pair, -1 / 0 behind n_track.
   svs_map_register_keyframes / svs_map_add_loop_closure: BLOCKING, the reference's two functions with the caller's own lists, through the same apply path (the
     track list goes up in the staged block).  registerKeyframes applies addNewEdges' test strength >= covis_thr; the neighbours that pass get their edges in
     ascending id.  A track entry whose global_id is no point of the map is skipped (:411-414); the first occurrence of an id wins; h_track_added [n_track]
     (optional) says 0 / 1 per entry.  addLoopClosure: pairs go to loop_id, the edge is (root_id, loop_id) with strength n_track.  h_edge_kf [n_neighbors]
     (optional), h_cons [n_neighbors] / [1], h_missing rows likewise.
   Refused before the map changes, map and registrar untouched -- SVS_ERR_INVALID: the handle's last registration was not a map batch on this map (or there is
   none), request_index outside it, a request already committed, an edge that is already present (the reference asserts in insertEdge), an unknown keyframe id,
   a neighbour twice or equal to the root, root_id == loop_id, a level outside 0 .. SVS_NUM_PYR_LEVELS - 1, a cached list that is not strictly ascending;
   SVS_ERR_CAPACITY: fewer free observations than track points, fewer free edges than edges to add, track_cap below n_track when h_track_point_ids or
   h_track_added is given. */
typedef struct {
  int32_t committed;                   /* 1: the map took the request; 0: nothing committed */
  int32_t mode;                        /* SVS_REG_LOCAL / SVS_REG_LOOP */
  int32_t root_id;                     /* the keyframe that took the pairs: the root / the loop keyframe */
  int32_t other_id;                    /* SVS_REG_LOOP: the query keyframe; else -1 */
  int32_t n_track, n_pairs_added, n_edges;
  int32_t status;                      /* svs_reg_commit: the request's svs_reg_result.status; the explicit calls: 0 */
  double T_new[12];                    /* the override of root_id in the constraints */
} svs_reg_commit_result;               /* 128 bytes */
int svs_reg_commit(svs_reg *reg, svs_map *map, int request_index, int n_cached, const int32_t *h_cached_ids, const double *h_cached_T, int missing_cap,
                   svs_reg_commit_result *h_res, int32_t *h_edge_kf, int32_t *h_edge_strength, svs_map_constraint_result *h_cons, int32_t *h_missing, int track_cap,
                   int32_t *h_track_point_ids, int32_t *h_track_added);
int svs_map_register_keyframes(svs_map *map, int32_t root_id, const double *T_newroot_from_w, int n_neighbors, const int32_t *h_neighbor_ids,
                               const int32_t *h_strength, int covis_thr, int n_track, const svs_map_track_point *h_track, int n_cached, const int32_t *h_cached_ids,
                               const double *h_cached_T, int missing_cap, svs_reg_commit_result *h_res, int32_t *h_edge_kf, svs_map_constraint_result *h_cons,
                               int32_t *h_missing, int32_t *h_track_added);
int svs_map_add_loop_closure(svs_map *map, int32_t root_id, int32_t loop_id, const double *T_newloop_from_w, int n_track, const svs_map_track_point *h_track,
                             int n_cached, const int32_t *h_cached_ids, const double *h_cached_T, int missing_cap, svs_reg_commit_result *h_res,
                             svs_map_constraint_result *h_cons, int32_t *h_missing, int32_t *h_track_added);

/* ---- front end: a stream's neighbourhood list built from the map.  Backend::computeNeighborhood (backend.cpp:244-386) from the vertex list onwards: the caller
   names the keyframes addPoseToNeighborhood(root) + findNeighborsOfRoot(root, 10) chose (the ordering by strength and the double_window test stay with it, as
   framesInNeighborhood does for registration), the device does addPointsToNeighbors (:311-345) and addAnchorPosesToNeighbors (:371-386) on the map and writes
   neighborhood_->point_list into the stream's candidate list where svs_frontend_set_candidates_grouped would have uploaded it, behind the new-point groups
   ("the head"), which still come from the host.  The reference's orders are those of hash containers and no function of its input; a canonical one is chosen:
     1. points.  Every point with at least one observation in a keyframe of h_vertex_kf, each once, in ASCENDING POINT ID.  The record is the map's: xyz_anchor,
        anchor_obs_pyr, anchor_level, point_id = its id.
     2. vertex set.  The ids of h_vertex_kf in the given order; behind them, in ascending id, the anchors of rule 1's points that are not among them.  Each with
        T_me_from_world AS THE MAP STORES IT: for a keyframe outside the window the reference calls computeAbsolutePose (:363) -- the caller keeps the map's pose
        of such a keyframe current through svs_map_set_poses (it may take it from svs_map_absolute_poses instead of a graph of its own).
     3. slots.  kf_index of a record of rule 1 is the slot s with h_slot_kf[s] == the anchor's id, -1 when no slot holds it (the matcher answers -1 with
        SVS_MATCH_NO_ANCHOR, matcher.cpp:336-339).  An entry of h_slot_kf that is < 0, or an id that is no keyframe of the map, holds no anchor.
     4. the stream's list becomes: the n_head head records in n_head_groups groups (as svs_frontend_set_candidates_grouped takes groups 0 .. G-2), then rule 1's
        records as the last group; the group ends, the group count n_head_groups + 1 and the new-record count n_head follow, and the records between the new
        length and the stream's previous one become "no candidate" (0xff) as the other setters leave them.
     5. pose refresh (refresh_poses != 0).  Every slot whose h_slot_kf entry is a keyframe of the map takes the map's pose as its T_anchor_from_w; pyramid
        pointers and strides are not touched.  (The poses of neighborhood_->vertex_map are what the matcher reads, matcher.cpp:328-347.)
     6. all or nothing per request.  If n_head + the points of rule 1 exceed the front end's max_points, or the vertex set exceeds vertex_cap, the stream's list,
        group ends, counts and slot poses stay exactly as they were and the result has over_capacity = 1: n_points / n_map_points are the counts the walk found;
        n_vertex / n_no_slot are those of the points it read -- 0 when the points did not fit.  The call returns SVS_OK, the other requests are unaffected.
     7. a request's outputs are a function of the map's content and of that request alone: not of the order or grouping of the updates that built the map, of
        the rest of the batch, or of repetition. */
typedef struct {
  int32_t stream, n_vertex, n_head, n_head_groups;      /* n_vertex >= 1, n_head_groups >= 1 (an absent list is an empty group) */
  const int32_t *h_vertex_kf;          /* HOST [n_vertex]: ids, root first */
  const int32_t *h_slot_kf;            /* HOST [the front end's max_keyframes]: the keyframe id kept in each slot of the stream, -1 for none */
  const int32_t *h_head_group_end;     /* HOST [n_head_groups]: one past the last record of each head group; the last = n_head */
  const svs_candidate_point *h_head;   /* HOST [n_head]: kf_index = a kept slot, or < 0 */
} svs_nbh_request;
typedef struct {
  int32_t n_points;                    /* records of the stream's list: n_head + n_map_points */
  int32_t n_map_points;                /* rule 1 */
  int32_t n_vertex;                    /* rule 2 */
  int32_t n_no_slot;                   /* records of rule 1 with kf_index = -1 */
  int32_t over_capacity;               /* rule 6 */
  int32_t pad_[3];
} svs_nbh_result;
/* BLOCKING: one staged upload (ids, slot tables, head records), at most the map's CSR rebuild plus one launch (one workgroup per request), one download (the
   results, the refreshed slot poses -- the front end's host mirror follows them -- and the rows asked for).  fe and map belong to one context.
   Outputs, each optional, HOST: h_res [n_requests]; h_point_id [n_requests][max_points]: the point id of every record of the built list, -1 behind it;
   h_vertex_id [n_requests][vertex_cap] (-1 behind the set) and h_vertex_T [n_requests][vertex_cap][12] (zeros behind it): rule 2; rows of a request over capacity:
   -1 / zeros.  h_records [n_streams][max_points]: the front end's whole candidate table as it lies on the device behind the call (a second copy; for tests).
   Refused before anything is uploaded or launched, all state unchanged -- SVS_ERR_INVALID: between svs_frontend_submit_frame and _wait_frame; fe and map on
   different contexts; n_requests above the number of streams; a stream named twice; an id of a vertex list that is no keyframe of the map, or twice in the list;
   a slot-table entry >= 0 for a slot that was never kept, or one id in two slots; a head svs_frontend_set_candidates_grouped would refuse (group ends, n_head above
   max_points, kf_index of an unkept slot); SVS_ERR_CAPACITY: more than 64 groups; SVS_ERR_UNSUPPORTED: max_keyframes above 32767. */
int svs_frontend_set_candidates_from_map(svs_frontend *fe, svs_map *map, int n_requests, const svs_nbh_request *req, int refresh_poses, int vertex_cap,
                                         svs_nbh_result *h_res, int32_t *h_point_id, int32_t *h_vertex_id, double *h_vertex_T, svs_candidate_point *h_records);

/* ---- front end: the keyframe logic behind a step -- processMatchedPoints' two lists (stereo_frontend.cpp:859-968), shallWeSwitchKeyframe (:446-510),
   shallWeDropNewKeyframe (:512-528) and the bookkeeping of addNewKeyframe (:316-415) -- decided on the device from what the step left there: one workgroup per
   stream, one launch for the batch, one small decision record per stream and the two AddToOptimzer lists in the record types svs_map_add_keyframe takes.  The
   stage READS the front end's state only (pose, clouds, keyframe slots and candidate lists are untouched); the caller applies a decision through
   svs_frontend_keep_keyframe_of, svs_frontend_recompute_cloud, svs_frontend_seed_keyframes and svs_map_add_keyframe.  Restated in tests/keyframe_model.py.
   Per stream.  Inputs: the n match, candidate and gate records of the last step, its svs_point_stats, the refined T_cur_from_actkey, tracking_ok; a VERTEX TABLE
   of V <= SVS_KF_MAX_VERTICES entries in the caller's order (neighborhood_->vertex_map), each with its keyframe id, T_me_from_w and a feature set F(v) -- either a
   range of the stream's staged, strictly ascending id array, or "the map's" (set_begin = SVS_KF_SET_MAP): the points whose observer row in the resident map holds
   the keyframe AS THE MAP IS AT THE CALL (a departure: the reference snapshots feat_map when the neighbourhood is computed; without a map such a set is empty);
   the index `act` of the active keyframe's vertex; the indices of its strength_to_neighbors vertices (distinct, not act); the slot table slot_kf[max_keyframes]
   (the keyframe id kept in each slot, -1 for none, as in svs_nbh_request).  The reference's containers are hash tables; every order below is canonical:
     0. tracking_ok == 0 (:243), or a table the device finds malformed (V, act, a neighbour index or a set range out of bounds): valid = 0, every other field of
        the record zero, no list written.
     1. lists.  A = the records with status == SVS_MATCH_OK and accepted != 0, in ascending record index (obs_list's order); those with is_new != 0 form the new
        list, the others the track list.  A new entry: xyz_anchor, anchor_obs_pyr, anchor_level, point_id from the candidate, anchor_id = slot_kf[kf_index] (-1 for a
        kf_index outside the table), feat_center = obs, feat_level = anchor_level.  A track entry: center = obs, global_id = point_id, level = anchor_level.  Beside
        each list the record index of every entry (the caller prunes newpoint_map with it, :360-365).  n_new and n_track are always reported.
     2. switch.  For every v != act: T_diff(v) = pose_mul(pose_mul(T_cur_from_actkey, T_act_from_w), pose_inv(T_v_from_w)) (f64, rows summed left to right, no
        contraction), dist(v) = sqrt((tx tx + ty ty) + tz tz).  closest = the v of least (dist, table index) among dist(v) < 0.5 * (double)parallax_thr (strict; a
        NaN is never less); closest_index / closest_id / closest_dist report it (-1 / -1 / 0.0 when there is none).  shared = the track entries whose global_id is
        in F(closest), an id listed twice counting twice.  decision = SVS_KF_SWITCH iff closest exists and shared > switch_min_shared; T_cur_after = T_diff(closest).
     3. drop, only without a switch.  featureless = the num_points_grid2x2 cells below featureless_cell_min; av_track_length = sum_track_length /
        (double)num_track_points (0 / 0: the quiet NaN 0x7ff8000000000000, which compares false).  decision = SVS_KF_DROP iff featureless > featureless_corners_thr,
        or the norm of T_cur_from_actkey's translation (as in rule 2) > (double)parallax_thr, or av_track_length > max_av_track_length; else SVS_KF_KEEP with
        T_cur_after = T_cur_from_actkey.  (With a switch both figures are reported as zero.)
     4. new keyframe, only for SVS_KF_DROP.  add_flags[k] = num_points_grid3x3[k] <= min_num_points; T_newkey_from_w = pose_mul(T_cur_from_actkey, T_act_from_w);
        T_cur_after = the identity.  num_matches(k) = the new entries with anchor_id k (k >= 0), plus -- for k = act's id and the ids of act's neighbour vertices
        only -- the track entries in F(k).  strength_to_neighbors = the keys with num_matches > covis_thr in ascending (count, keyframe id) (the reference's
        multimap leaves equal counts in hash order): n_strength, strength_kf, strength_count.  More than SVS_KF_MAX_STRENGTH keys: over_capacity = 1, the list
        empty (n_strength = 0), everything else valid.
     5. a stream's outputs are a function of that stream's inputs alone: not of the batch, of repetition, or of whether a set was staged or read from a map
        with the same content.  Compaction is by ballot popcounts and a workgroup prefix, counts are integer sums: no arrival order decides an output. */
#define SVS_KF_MAX_VERTICES 64
#define SVS_KF_MAX_STRENGTH 64
#define SVS_KF_MAX_SLOTS 1024
#define SVS_KF_SET_MAP (-1)
enum { SVS_KF_KEEP = 0, SVS_KF_SWITCH = 1, SVS_KF_DROP = 2 };
typedef struct {
  float parallax_thr;                  /* ui.parallax_thr (0.75f; a pangolin::Var<float>) */
  int32_t switch_min_shared;           /* 100 (:503) */
  int32_t featureless_cell_min;        /* 15 (:519) */
  int32_t featureless_corners_thr;     /* params_.new_keyframe_featuerless_corners_thr (2) */
  double max_av_track_length;          /* 75. (:527) */
  int32_t covis_thr;                   /* params_.covis_thr (15); >= 0 */
  int32_t min_num_points;              /* ui.min_num_points (25) */
} svs_keyframe_decide_params;          /* 32 bytes */
void svs_keyframe_decide_params_default(svs_keyframe_decide_params *p);
typedef struct {
  double T_me_from_w[12];
  int32_t kf_id;
  int32_t set_begin, set_count;        /* F(v) = ids[set_begin .. set_begin + set_count) of the stream's staged array, or set_begin = SVS_KF_SET_MAP */
  int32_t pad_;
} svs_kf_vertex;                       /* 112 bytes */
typedef struct {
  int32_t n_vertex, act, n_neighbors, pad_;
  int32_t neighbors[SVS_KF_MAX_VERTICES];      /* vertex indices of act's strength_to_neighbors */
} svs_kf_table;                        /* 272 bytes */
typedef struct {
  int32_t valid, decision, n_new, n_track;
  int32_t closest_index, closest_id, shared, featureless;
  double closest_dist, av_track_length;
  double T_cur_after[12];
  double T_newkey_from_w[12];
  int32_t add_flags[9];                /* [i * 3 + j] */
  int32_t n_strength, over_capacity, pad_;
  int32_t strength_kf[SVS_KF_MAX_STRENGTH];
  int32_t strength_count[SVS_KF_MAX_STRENGTH];
} svs_keyframe_decision;               /* 800 bytes */
typedef struct {                       /* all pointers DEVICE; stream b at + b * (its batch stride) elements */
  const svs_match_result *d_res; size_t res_bstride;
  const svs_candidate_point *d_pts; size_t pts_bstride;
  const svs_gated_point *d_gated; size_t gated_bstride;
  const svs_point_stats *d_stats;      /* [batch] */
  const double *d_T_cur_from_actkey;   /* [batch][12] */
  const int32_t *d_tracking_ok;        /* [batch] */
  const int32_t *d_n;                  /* [batch] records of each stream (at most n), or NULL: n for all */
  int32_t n, batch;
  const svs_kf_table *d_table;         /* [batch] */
  const svs_kf_vertex *d_vertex; size_t vertex_bstride;      /* [batch][vertex_bstride]; vertex_bstride <= SVS_KF_MAX_VERTICES bounds n_vertex */
  const int32_t *d_set_ids; size_t set_bstride;              /* [batch][set_bstride]: the staged id arrays */
  const int32_t *d_slot_kf; size_t slot_bstride;             /* [batch][slot_bstride], max_keyframes entries read */
  int32_t max_keyframes, pad_;         /* <= SVS_KF_MAX_SLOTS */
  svs_map *map;                        /* the map behind SVS_KF_SET_MAP sets (same context), or NULL */
} svs_keyframe_decide_args;
/* stateless, ASYNCHRONOUS on the context's stream (a map whose log has grown rebuilds its CSR views first).  d_dec [batch]; d_new / d_track / d_new_rec /
   d_track_rec [batch][cap]: the lists and their record indices (entries behind a list's count are left as they were).  SVS_ERR_CAPACITY: cap < n, vertex_bstride
   above SVS_KF_MAX_VERTICES; SVS_ERR_UNSUPPORTED: max_keyframes above SVS_KF_MAX_SLOTS; SVS_ERR_INVALID: a missing pointer, covis_thr < 0, a map of another context */
int svs_keyframe_decide(svs_ctx *ctx, const svs_keyframe_decide_args *a, const svs_keyframe_decide_params *prm, svs_keyframe_decision *d_dec,
                        svs_map_new_point *d_new, svs_map_track_point *d_track, int32_t *d_new_rec, int32_t *d_track_rec, int cap);
/* a stream's vertex table, resident until it is set again.  One staged upload and one scatter launch for all requests; everything is checked first. */
typedef struct {
  int32_t stream, n_vertex, act, n_neighbors;
  const int32_t *h_vertex_kf;          /* HOST [n_vertex]: keyframe ids */
  const double *h_vertex_T;            /* HOST [n_vertex][12]: T_me_from_w */
  const int32_t *h_set_begin;          /* HOST [n_vertex]: start of F(v) in h_set_ids, or SVS_KF_SET_MAP */
  const int32_t *h_set_count;          /* HOST [n_vertex] (ignored for SVS_KF_SET_MAP) */
  const int32_t *h_set_ids;            /* HOST [n_set_ids]; every range strictly ascending */
  const int32_t *h_neighbors;          /* HOST [n_neighbors]: vertex indices */
  const int32_t *h_slot_kf;            /* HOST [max_keyframes] */
  int32_t n_set_ids, pad_;
} svs_vertex_request;
/* SVS_ERR_INVALID, nothing uploaded: a stream out of range or named twice, n_vertex < 1, an id twice in a table, act or a neighbour index out of range, a
   neighbour equal to act or listed twice, a set range outside h_set_ids or not strictly ascending, a slot entry >= 0 for a slot that was never kept, a call
   between svs_frontend_submit_frame and _wait_frame.  SVS_ERR_CAPACITY: more than SVS_KF_MAX_VERTICES vertices (the front end's vertex_cap), more than
   16 * max_points staged ids.  SVS_ERR_UNSUPPORTED: a front end with more than SVS_KF_MAX_SLOTS keyframe slots. */
int svs_frontend_set_vertex_table(svs_frontend *fe, int n_requests, const svs_vertex_request *req);
/* BLOCKING.  The decision of every stream from the last step's device state and the resident vertex tables: one launch, one download of all decision records
   (h_dec [n_streams]), then the list rows -- want_lists = 1: of the streams whose decision is SVS_KF_DROP, 2: of every valid stream, 0: none -- as one strided
   copy per array and run of consecutive such streams into h_new / h_track / h_new_rec / h_track_rec [n_streams][cap] (rows of other streams and entries behind
   a list's count are not written).  `map` may be NULL unless a table names SVS_KF_SET_MAP.  SVS_ERR_INVALID: the last frame call was not a step, a candidate list
   was set since (the SVS_SEED_MORE rule), a stream without a vertex table; SVS_ERR_CAPACITY: want_lists != 0 and cap below the step's record count. */
int svs_frontend_decide_keyframes(svs_frontend *fe, svs_map *map, const svs_keyframe_decide_params *prm, int want_lists, svs_keyframe_decision *h_dec,
                                  svs_map_new_point *h_new, svs_map_track_point *h_track, int32_t *h_new_rec, int32_t *h_track_rec, int cap);
/* svs_frontend_commit_keyframe: BLOCKING.  Applies the SVS_KF_DROP decision of ONE stream: svs_map_add_keyframe_dev on the lists where the stream's last
   svs_frontend_decide_keyframes left them (n_new / n_track of its decision record), so no list record reaches the host.  From the front end come
     the keyframe record: the pyramid pointers and strides of keyframe slot `slot` of the stream (the caller has kept the frame there,
       svs_frontend_keep_keyframe_of, and leaves the slot alone while the map names it: the map points at the front end's memory, and at `disp`, whose lifetime is
       the caller's, as with svs_map_add_keyframe);
     T_newkey_from_oldkey: the step's refined T_cur_from_actkey of the stream, bit-equal to what svs_frontend_results returns;
     the thresholds, with h_fast_thr NULL: the stream's persistent FAST thresholds as the detector holds them after the step, [SVS_NUM_PYR_LEVELS][SVS_MAX_CELLS]
       with the cells beyond a level's grid at 25 (what the reference clones into the keyframe as cell_grid2d).
   Pose and thresholds ride to the host on the call's first download; nothing else is copied.  Outputs and refusals are svs_map_add_keyframe_dev's (h_new_kept
   [n_new], h_track_exists [n_track] of the decision record; arrays of max_points entries are enough).  SVS_ERR_INVALID, nothing done: a stream or slot out of
   range, no svs_frontend_decide_keyframes since the stream's last step, a decision that is not valid or not SVS_KF_DROP, a candidate list set or a frame
   submitted since (the conditions svs_frontend_decide_keyframes checks), a svs_frontend_recompute_cloud since the step (it overwrites the refined poses of ALL
   streams, which are what a commit inserts: a batch caller commits its drops BEFORE it re-makes the clouds of the streams that switched or dropped), a slot that
   was never kept, a map of another context.  The front end's state is only read: a commit changes nothing a later step, decision or commit of another stream
   sees. */
typedef struct {
  int32_t stream, slot, newkey_id, oldkey_id, covis_thr, half_width, half_height, disp_stride;
  const float *disp;                   /* DEVICE, level 0 */
  const int32_t *h_fast_thr;           /* HOST [SVS_NUM_PYR_LEVELS][SVS_MAX_CELLS], or NULL: the detector's */
  const int32_t *cached_ids;           /* HOST [n_cached] strictly ascending */
  const double *cached_T;              /* HOST [n_cached][12] */
  int32_t n_cached, pad_;
} svs_commit_keyframe_request;         /* 72 bytes */
int svs_frontend_commit_keyframe(svs_frontend *fe, svs_map *map, const svs_commit_keyframe_request *req, int missing_cap, svs_map_strength_result *h_res,
                                 svs_map_key *h_keys, int32_t *h_new_kept, int32_t *h_track_exists, svs_map_constraint_result *h_cons, int32_t *h_missing);

/* ---- front end: a stream's whole neighbourhood from a root id.  Backend::computeNeighborhood(root_id) (backend.cpp:244-309, :347-386) and the order in which
   processMatchedPoints visits newpoint_map (stereo_frontend.cpp:989-1029), joined on the device: findNeighborsOfRoot on the map's strength-ordered adjacency,
   svs_frontend_set_candidates_from_map's point / anchor walk, svs_map_absolute_poses' search for the vertices outside the window, the edge-strength matrix, the
   active keyframe's strength_to_neighbors, the head's groups put into that order, and svs_frontend_set_vertex_table's resident table -- nothing comes back to
   the host in between, and THE MAP IS ONLY READ (computeAbsolutePose does not store its result either).  The reference's orders are those of hash containers;
   every order below is canonical.  Per request:
     1. neighbours of the root.  The root's edges in ASCENDING (strength, edge slot) -- its adjacency row walked backwards -- of which only those whose other
        end has SVS_REG_KF_IN_WINDOW count; the reference compares its count before it increments it (:304-306), so up to max_num_neighbors + 1 ids are taken.
        The vertex list is the root followed by these ids.  A root without SVS_REG_KF_IN_WINDOW (the reference asserts INNER): root_outside_window = 1, every
        other field of the result zero, the stream untouched.
     2. points, anchors, slots: rules 1-3 of svs_frontend_set_candidates_from_map for that vertex list, byte for byte.
     3. poses of the vertex set.  A vertex with SVS_REG_KF_IN_WINDOW: the map's stored pose.  Any other: exactly the T svs_map_absolute_poses returns for it;
        with SVS_WALK_NO_PATH the stored pose, counted in n_no_path.
     4. the active keyframe.  act_index = the place of act_id in the vertex set, or -1.  strength_to_neighbors(act) = every other vertex with an edge to act in
        the map's edge table (any type, marginalised or not), in ASCENDING (strength, keyframe id), as vertex indices; empty when act_index = -1.
     5. edge-strength matrix [vertex_cap][vertex_cap] (:261-282): the strength of edge (i, j); -1 where there is none, on the diagonal and behind the set.
     6. the stream's list: the n_fixed_groups leading head groups unchanged (newpoint_map[actkey_id]); then the keyed groups (group g >= n_fixed_groups is
        newpoint_map[h_head_group_kf[g]]) whose key is in rule 4's list, in that list's order, an empty one included; keyed groups whose key is not in it are
        left out and their records counted in n_head_dropped; then rule 2's records as the last group.  Group ends, group count (n_groups), new-record count
        (n_head_kept) and the 0xff tail as rule 4 of svs_frontend_set_candidates_from_map.
     7. slot poses (refresh_poses != 0): a slot whose keyframe is in the vertex set takes rule 3's pose, any other slot that names a keyframe of the map the
        map's pose; they come back for the front end's host mirror.
     8. the stream's resident vertex table, written on the device as svs_frontend_set_vertex_table writes it from rule 2's ids, rule 3's poses, every set
        SVS_KF_SET_MAP, act = act_index, neighbors = rule 4's list and h_slot_kf.  With act_index = -1 the table has act = -1 and no neighbours:
        svs_frontend_decide_keyframes then reports valid = 0 for the stream (its rule 0); the candidate list is still written.
     9. all or nothing.  over_capacity = 1 leaves list, group ends, counts, slot poses and vertex table as they were; SVS_OK, other requests unaffected.  Found
        in this order: (a) the vertex list of rule 1 above vertex_cap: n_vertex = its length, n_points = the fixed groups' records, the rest zero; (b) the fixed
        groups' records plus the map points above max_points: n_points = their sum, n_map_points, the rest zero (the points are not read); (c) the vertex set
        above vertex_cap: as (b) plus n_vertex, n_no_slot; (d) the kept head plus the map points above max_points: every count as found, n_points = their sum.
    10. a request's bytes are a function of that request and of the map's content (an edge's slot is part of it): not of the rest of the batch, of repetition
        or of any arrival order.  Compaction is by ballots, popcounts and prefixes; orderings are rank sorts over unique keys. */
typedef struct {
  int32_t stream, root_id, act_id, max_num_neighbors;   /* the reference passes 10 */
  int32_t n_head, n_head_groups, n_fixed_groups, pad_;   /* 1 <= n_fixed_groups <= n_head_groups */
  const int32_t *h_slot_kf;            /* HOST [the front end's max_keyframes], as in svs_nbh_request */
  const int32_t *h_head_group_end;     /* HOST [n_head_groups] */
  const svs_candidate_point *h_head;   /* HOST [n_head] */
  const int32_t *h_head_group_kf;      /* HOST [n_head_groups]: the key of every group g >= n_fixed_groups (the entries before are not read) */
} svs_nbr_request;                     /* 64 bytes */
typedef struct {
  int32_t n_points, n_map_points, n_vertex, n_no_slot, over_capacity;      /* as svs_nbh_result */
  int32_t root_outside_window;
  int32_t n_root_neighbors;            /* rule 1: ids taken */
  int32_t n_no_path;                   /* rule 3 */
  int32_t act_index, n_act_neighbors;  /* rule 4 */
  int32_t n_head_kept, n_head_dropped; /* rule 6: records */
  int32_t n_groups;                    /* rule 6: groups of the written list, the map's included */
  int32_t pad_[3];
} svs_nbr_result;                      /* 64 bytes */
/* BLOCKING: one staged upload (requests, slot tables, head records), at most the map's CSR and adjacency rebuilds plus four launches (selection and point walk;
   the list of vertices outside the window with its count, built on the device; the searches, a grid sized to an upper bound whose idle workgroups leave at
   once; poses, ranking, matrix, head and tables), one download.  Outputs, each optional, HOST: h_res [n_requests]; h_point_id [n_requests][max_points],
   h_vertex_id [n_requests][vertex_cap], h_vertex_T [n_requests][vertex_cap][12] as svs_frontend_set_candidates_from_map returns them (rule 3's poses);
   h_act_neighbors [n_requests][vertex_cap]: rule 4's vertex indices, -1 behind them; h_strength [n_requests][vertex_cap][vertex_cap]: rule 5; rows of a
   request over capacity or with its root outside the window: -1 / zeros.  For tests: h_records as svs_frontend_set_candidates_from_map; h_table [n_requests]
   and h_vertex [n_requests][SVS_KF_MAX_VERTICES]: the svs_kf_table / svs_kf_vertex rows of the request's stream as they lie on the device behind the call;
   h_slot_T [n_requests][max_keyframes][12]: the poses rule 7 wrote into the stream's slots, zeros for every other slot, without a refresh and for a request
   that left its stream untouched.
   Refused before anything is uploaded, all state unchanged -- SVS_ERR_INVALID: between svs_frontend_submit_frame and _wait_frame; fe and map on different
   contexts; a stream out of range or named twice; root_id or act_id no keyframe of the map; max_num_neighbors < 0; vertex_cap outside 1 ..
   SVS_KF_MAX_VERTICES; a slot table or head svs_frontend_set_candidates_from_map would refuse; n_fixed_groups outside 1 .. n_head_groups; a key that is no
   keyframe of the map or on two keyed groups; SVS_ERR_CAPACITY: more than 64 groups; SVS_ERR_UNSUPPORTED: max_keyframes above SVS_KF_MAX_SLOTS. */
int svs_frontend_set_neighborhood_from_root(svs_frontend *fe, svs_map *map, int n_requests, const svs_nbr_request *req, int refresh_poses, int vertex_cap,
                                            svs_nbr_result *h_res, int32_t *h_point_id, int32_t *h_vertex_id, double *h_vertex_T, int32_t *h_act_neighbors,
                                            int32_t *h_strength, svs_candidate_point *h_records, svs_kf_table *h_table, svs_kf_vertex *h_vertex,
                                            double *h_slot_T);

/* ---- front end: newpoint_map on the device.  StereoFrontend::newpoint_map (stereo_frontend.h:125) is a hash map from keyframe id to a list of candidate points; it
   is seeded at stereo_frontend.cpp:808 (push_front), pruned at :360-365 (every list, remove_if over the matched new points of the last step, only on a drop) and
   handed to the matcher at :989-1029 (the active keyframe's list, then the lists of its strength_to_neighbors in that order).  Each stream of a front end gets a
   STORE that holds it: an ordered sequence of GROUPS in creation order, each with a unique key kf_id >= 0 and its svs_candidate_point records in list order.  On
   the device the records of a stream lie packed, group behind group, in store order; a table of (key, count) per group lies beside them, and the front end keeps a
   host mirror of that table -- never of a record -- from which every refusal below is decided before anything is uploaded or launched.  Restated in
   tests/newpoint_model.py.  The reference's map is a hash container; every order below is canonical:
     1. reserve.  svs_frontend_newpoints_reserve sets record_cap (records per stream) and group_cap (groups per stream, <= SVS_NEWPOINTS_MAX_GROUPS) once and
        allocates; a front end that never reserves allocates nothing, and every other call of this block is refused on it.
     2. put.  SVS_NEWPOINTS_PREPEND: the n given records, already in list order, go in front of the records of group kf_id; SVS_NEWPOINTS_REPLACE: they become its
        records.  An absent key creates the group at the END of the store, also with n = 0.  The records are stored as given (kf_index included; see rule 6).
        Requests apply in request order; several may name one stream or one group.
     3. seed.  svs_frontend_seed_newpoints runs svs_frontend_seed_keyframes' problems (both modes, its SVS_SEED_MORE rule) and prepends the records request r would
        have returned there to group h_kf_id[r] of the request's stream, device to device, in request order behind one another (rule 2's PREPEND).
     4. prune.  P = the point_id of every record i of the last step with status == SVS_MATCH_OK, accepted != 0 and i < the list's new-record count (the "new list" of
        rule 1 of svs_keyframe_decide, matched_new_feat at :922-925).  Every record of every group of the stream whose point_id is in P is removed; the others keep
        their order (remove_if is stable); a group stays, also when it becomes empty.  Matching is by id, not by remembered list positions: a store changed between
        hand-over and prune is pruned all the same.  n_removed and every group's record count come back.
     5. drop.  svs_frontend_newpoints_drop_groups removes the named groups with their records; the other groups keep their order.  (The reference never erases a
        list; this keeps a long run under group_cap, and which groups go is the caller's decision.)  A key that is absent or named twice counts once or not at all:
        n_found = the groups removed.
     6. hand-over.  The stream's candidate list becomes group h_keys[0], group h_keys[1], ... (an absent key: an empty group), then the caller's n_tail tail records
        (neighborhood_->point_list) as the last group.  A head record of group k gets kf_index = the slot s with h_slot_kf[s] == k, -1 when no slot holds k (an entry
        < 0 holds nothing); the stored kf_index is not used.  Tail records are taken as given.  Group ends, the group count n_keys + 1, the new-record count (the
        head's records) and the 0xff tail behind the list follow rule 4 of svs_frontend_set_candidates_from_map.  The store is not changed.
     7. all or nothing.  A refused call changes nothing, on the host or on the device.  A hand-over request whose total exceeds max_points comes back with
        over_capacity = 1, its stream untouched, n_points / n_head as found; the call returns SVS_OK and the other requests are unaffected.
     8. a stream's bytes are a function of the calls made for that stream, in their order: not of the rest of a batch, of batch position or of repetition.
        Compaction is by ballots, popcounts and a workgroup prefix, group by group and chunk by chunk, reads complete before writes: no atomic decides a position. */
#define SVS_NEWPOINTS_MAX_GROUPS 64
enum { SVS_NEWPOINTS_PREPEND = 0, SVS_NEWPOINTS_REPLACE = 1 };
/* SVS_ERR_INVALID, nothing changed: record_cap < 1, group_cap outside 1 .. SVS_NEWPOINTS_MAX_GROUPS, a second reserve, between svs_frontend_submit_frame and _wait_frame */
int svs_frontend_newpoints_reserve(svs_frontend *fe, int record_cap, int group_cap);
typedef struct {
  int32_t stream, kf_id, mode, n;      /* mode: SVS_NEWPOINTS_PREPEND / _REPLACE */
  const svs_candidate_point *h_records;        /* HOST [n], list order */
} svs_newpoints_put_request;           /* 24 bytes */
/* BLOCKING: one staged upload, one launch (one workgroup per stream named).  Refused, nothing changed -- SVS_ERR_INVALID: no reserve, a stream out of range, kf_id < 0,
   an unknown mode, n < 0, records missing, between submit_frame and wait_frame; SVS_ERR_CAPACITY: a stream would hold more than group_cap groups or more than
   record_cap records behind ANY of its requests (every stream of the call then stays as it was) */
int svs_frontend_newpoints_put(svs_frontend *fe, int n_requests, const svs_newpoints_put_request *req);
/* BLOCKING.  h_kf_id [n]: the group of each request; h_n_new [n][3] as svs_frontend_seed_keyframes returns it; h_out [n][cap_per_request] (may be NULL; for tests):
   the records as that call returns them.  Refused, nothing changed: whatever svs_frontend_seed_keyframes refuses; SVS_ERR_INVALID: no reserve, kf_id < 0;
   SVS_ERR_CAPACITY: more than group_cap groups, or a stream's records plus THE MOST its requests can produce (the sum over the levels of (num_max_points >> l) + 1
   each) above record_cap -- the counts are known on the device only, so the bound is taken before the launch */
int svs_frontend_seed_newpoints(svs_frontend *fe, int n, const svs_seed_request *req, const int32_t *h_kf_id, const svs_seed_params *prm, int32_t *h_n_new,
                                svs_candidate_point *h_out, int cap_per_request);
typedef struct {                       /* all pointers DEVICE; entry b works on stream s = d_stream ? d_stream[b] : b, whose rows lie at + s * (the batch stride) elements */
  const svs_match_result *d_res; size_t res_bstride;
  const svs_candidate_point *d_pts; size_t pts_bstride;
  const svs_gated_point *d_gated; size_t gated_bstride;
  const int32_t *d_n;                  /* [streams] records of each stream's step (at most n), or NULL: n for all */
  const int32_t *d_n_new;              /* [streams] the new-record count of each stream's list */
  int32_t n, batch;
  svs_candidate_point *d_store; size_t store_bstride;        /* [streams][store_bstride]: the groups' records back to back, in store order; compacted in place */
  int32_t *d_group_count; size_t group_bstride;               /* [streams][group_bstride]: records per group, in and out; group_bstride <= SVS_NEWPOINTS_MAX_GROUPS bounds n_groups */
  const int32_t *d_n_groups;           /* [streams] */
  const int32_t *d_stream;             /* [batch] distinct streams, or NULL */
} svs_newpoints_prune_args;            /* 120 bytes */
/* rule 4, stateless, ASYNCHRONOUS on the context's stream: one workgroup per entry, one launch.  d_n_removed [batch].  A group table the device finds malformed (a
   count < 0, counts summing above store_bstride, n_groups outside 0 .. group_bstride) is cut where it leaves its row: nothing outside the stream's rows is read
   or written.  SVS_ERR_INVALID: a missing pointer, n or batch < 0; SVS_ERR_CAPACITY: group_bstride above SVS_NEWPOINTS_MAX_GROUPS; SVS_ERR_UNSUPPORTED: n above
   8192 (P is held, sorted, in LDS) */
int svs_newpoints_prune(svs_ctx *ctx, const svs_newpoints_prune_args *a, int32_t *d_n_removed);
/* the same for the named streams from the front end's own state (the records of the last step, the stores).  BLOCKING; h_n_removed [n_streams],
   h_group_count [n_streams][SVS_NEWPOINTS_MAX_GROUPS] (may be NULL; zeros behind a stream's groups).  SVS_ERR_INVALID, nothing changed: no reserve, a stream out of
   range or named twice, the last frame call was not a step or a candidate list was set since (the SVS_SEED_MORE rule), between submit_frame and wait_frame */
int svs_frontend_newpoints_prune(svs_frontend *fe, int n_streams, const int32_t *h_streams, int32_t *h_n_removed, int32_t *h_group_count);
typedef struct {
  int32_t stream, n_keys;
  const int32_t *h_keys;               /* HOST [n_keys] */
} svs_newpoints_drop_request;          /* 16 bytes */
/* rule 5.  BLOCKING, h_n_found [n_requests]; requests apply in order.  SVS_ERR_INVALID, nothing changed: no reserve, a stream out of range, n_keys < 0 */
int svs_frontend_newpoints_drop_groups(svs_frontend *fe, int n_requests, const svs_newpoints_drop_request *req, int32_t *h_n_found);
/* the stores of the named streams AS THEY LIE ON THE DEVICE (host mirrors, tests).  BLOCKING.  h_n_groups [n_streams]; h_keys / h_counts [n_streams]
   [SVS_NEWPOINTS_MAX_GROUPS] in store order (-1 / 0 behind a stream's groups); h_records [n_streams][record_cap], each optional: a stream's records back to back in store
   order, behind them whatever the device holds.  SVS_ERR_INVALID: no reserve, a stream out of range */
int svs_frontend_newpoints_get(svs_frontend *fe, int n_streams, const int32_t *h_streams, int32_t *h_n_groups, int32_t *h_keys, int32_t *h_counts,
                               svs_candidate_point *h_records);
typedef struct {
  int32_t stream, n_keys, n_tail, pad_;        /* 1 <= n_keys <= SVS_NEWPOINTS_MAX_GROUPS - 1 */
  const int32_t *h_keys;               /* HOST [n_keys]: the active keyframe's id, then its strength_to_neighbors in order */
  const int32_t *h_slot_kf;            /* HOST [the front end's max_keyframes], as in svs_nbh_request */
  const svs_candidate_point *h_tail;   /* HOST [n_tail]: kf_index = a kept slot, or < 0 */
} svs_newpoints_list_request;          /* 40 bytes */
typedef struct {
  int32_t n_points;                    /* records of the stream's list: n_head + n_tail */
  int32_t n_head;                      /* records taken from the store */
  int32_t n_groups;                    /* n_keys + 1 */
  int32_t n_no_slot;                   /* head records with kf_index = -1 */
  int32_t over_capacity;               /* rule 7 */
  int32_t pad_[3];
} svs_newpoints_list_result;           /* 32 bytes */
/* rule 6.  BLOCKING: one staged upload (requests, tail records), one launch (one workgroup per request).  h_res [n_requests] (may be NULL); h_records [n_streams]
   [max_points] and h_group_end [n_streams][SVS_NEWPOINTS_MAX_GROUPS] (may be NULL; for tests): the front end's whole candidate table and its rows of group ends
   behind the call.  Refused before anything is uploaded, all state unchanged --
   SVS_ERR_INVALID: no reserve, between submit_frame and wait_frame, a stream out of range or named twice, n_keys < 1, a key < 0 or named twice, a slot-table entry
   >= 0 for a slot that was never kept or one id in two slots, n_tail < 0 or above max_points, a tail record with the kf_index of an unkept slot;
   SVS_ERR_CAPACITY: more than SVS_NEWPOINTS_MAX_GROUPS - 1 keys */
int svs_frontend_set_candidates_from_newpoints(svs_frontend *fe, int n_requests, const svs_newpoints_list_request *req, svs_newpoints_list_result *h_res,
                                               svs_candidate_point *h_records, int32_t *h_group_end);

/* svs_frontend_set_neighborhood_from_root with the head taken from the stores: the same request and result types, the four head fields of every request (n_head,
   n_head_groups, n_fixed_groups and the three head pointers) zero / NULL.  Every rule of that call holds unchanged, with these readings: rule 6's fixed group is the
   store's group act_id (an empty group when the store has none), its keyed groups are all other groups of the stream's store with their keys -- a key that is no
   keyframe of the map, or no neighbour of act, is left out and counted in n_head_dropped; a head record takes its kf_index as in rule 6 of the block above (the slot
   that holds its group's keyframe among the slots that name a keyframe of the map, else -1).  The stores are only read; no record goes up or comes down.  Refused as
   that call refuses (a head cannot be malformed here), and SVS_ERR_INVALID: no reserve, a head field set; SVS_ERR_CAPACITY: the store's groups, act's and the map's
   are more than 64 */
int svs_frontend_set_neighborhood_from_store(svs_frontend *fe, svs_map *map, int n_requests, const svs_nbr_request *req, int refresh_poses, int vertex_cap,
                                             svs_nbr_result *h_res, int32_t *h_point_id, int32_t *h_vertex_id, double *h_vertex_T, int32_t *h_act_neighbors,
                                             int32_t *h_strength, svs_candidate_point *h_records, svs_kf_table *h_table, svs_kf_vertex *h_vertex,
                                             double *h_slot_T);

/* ---- multi-GPU: the library-owned collective of the landmark-sharded back-end.  The reference has no
   distributed code; one process per GPU each creates a context and a communicator (RCCL, bound at run time) --------------*/
typedef struct { char bytes[128]; } svs_unique_id;      /* = ncclUniqueId */
typedef struct svs_comm svs_comm;
/* rank 0 obtains the id and hands it to the other ranks out of band (MPI, a TCP store, a file) */
int svs_comm_get_unique_id(svs_ctx *ctx, svs_unique_id *out);
/* collective over all ranks: ncclCommInitRank on the context's device */
int svs_comm_create(svs_ctx *ctx, const svs_unique_id *id, int rank, int world, svs_comm **out);
int svs_comm_destroy(svs_comm *c);
/* sum `count` doubles at d_buf in place across ranks, on the context's stream (asynchronous like every device entry point) */
int svs_comm_allreduce_f64(svs_comm *c, void *d_buf, size_t count);
int svs_comm_stats(svs_comm *c, int32_t *rank, int32_t *world, uint64_t *n_calls, uint64_t *n_doubles);
/* Second transport behind the same svs_comm handle (svs_comm_allreduce_f64 / svs_ba_set_comm work unchanged): a ONE-SHOT exchange over peer-mapped
   mailboxes (hipIpc + xGMI P2P writes) instead of RCCL's ring -- every rank pushes its vector into every peer's mailbox, waits for the N-1 arrivals and
   sums in rank order (bit-identical on all ranks).  Meant for the small, latency-bound messages of the sharded back end; world <= 16.
     1. every rank: svs_comm_create_p2p (mailbox of 2 x world x capacity_doubles; longer messages travel in pieces) -> its svs_ipc_handle
     2. all-gather the handles out of band (MPI, a TCP store, torch.distributed), then every rank: svs_comm_connect_p2p(c, handles[world])
   A peer that never arrives makes the result NaN and is counted (svs_comm_transport); destroy collectively (no rank may still be pushing).
   The mailbox is allocated fine-grained (hipExtMallocWithFlags; uncached, then plain memory as fall-backs -- svs_comm_transport says which): peers write it while
   the owner's kernel polls it.  hipIpcOpenMemHandle cannot open a handle inside the process that exported it: one process driving several GPUs cannot use this
   transport (one process per GPU, as everywhere in this library). */
typedef struct { char bytes[64]; } svs_ipc_handle;      /* = hipIpcMemHandle_t */
int svs_comm_create_p2p(svs_ctx *ctx, int rank, int world, size_t capacity_doubles, svs_comm **out, svs_ipc_handle *h_mine);
int svs_comm_connect_p2p(svs_comm *c, const svs_ipc_handle *h_all);
/* *kind = 0: RCCL; one-shot P2P with its mailbox in 1: fine-grained, 2: uncached, 3: plain (coarse-grained) device memory; *timeouts = reduce launches that gave
   up waiting for a peer (blocking; either may be NULL) */
int svs_comm_transport(svs_comm *c, int32_t *kind, uint32_t *timeouts);

/* ---- BA: replaces SlamGraph::optimize (slam_graph.hpp:457-462, slam_graph.cpp:312-355) -------*/
typedef struct svs_ba svs_ba;
/* all-reduce hook for landmark-sharded operation: sum `count` doubles at d_buf in place across
   ranks, on the ctx stream (RCCL via torch.distributed in scavislam_amd/backend.py) */
typedef int (*svs_allreduce_fn)(void *d_buf, size_t count, void *user);

int svs_ba_create(svs_ctx *ctx, svs_ba **out);
int svs_ba_destroy(svs_ba *ba);
/* copyDataToG2o (slam_graph.cpp:983-1032): poses of the double window, active points as psi
   (inverse depth), observation edges, pose-pose constraints.  Host arrays; edges may be in any
   order.  In sharded runs each rank passes only its landmarks' edges (point ids stay global
   0..L-1) and add_pose_terms = 1 on exactly one rank (constraints counted once). */
int svs_ba_set_problem(svs_ba *ba, int P, const double *h_poses, int L, const double *h_psi,
                       int E, const svs_ba_edge *h_edges, int C, const svs_ba_constraint *h_cons,
                       const svs_cam *cam, const svs_ba_params *prm, int add_pose_terms);
/* Persistent window -- the alternative to svs_ba_set_problem for a caller whose window evolves by about one
   keyframe per optimize(): the library keeps every observation it has been given on the device; a call brings the window's definition
   by the graph's own ids (frame ids and point ids come from one counter in the reference, stereo_frontend.cpp:826-831), the current
   values, the observations made SINCE THE LAST CALL and the window's pose-pose constraints.
     h_pose_ids [P] / h_poses [P][12]      the double window in block-row order (copyPosesToG2o, slam_graph.cpp:924-935)
     h_point_ids [L] / h_psi [L][3] / h_anchor_pose_ids [L]   the active points (addPointToG2o :907-922), anchor by frame id
     h_new_obs [n_new]                     svs_ba_edge records whose .point / .pose hold IDS (.anchor ignored): addObsToG2o's arguments
     h_cons [C]                            constraints whose .pose1 / .pose2 hold frame IDS (copyContraintsToG2o :937-981)
   The window's edges = all stored observations whose point is active, whose keyframe is in the window and whose point's anchor is in
   the window (exactly the filter of slam_graph.cpp:1001-1006).  State comes back through svs_ba_get_state in the order given here.
   svs_ba_window_reset forgets the stored observations. */
int svs_ba_window_update(svs_ba *ba, int P, const int32_t *h_pose_ids, const double *h_poses, int L, const int32_t *h_point_ids,
                         const double *h_psi, const int32_t *h_anchor_pose_ids, int n_new, const svs_ba_edge *h_new_obs, int C,
                         const svs_ba_constraint *h_cons, const svs_cam *cam, const svs_ba_params *prm);
int svs_ba_window_reset(svs_ba *ba);
/* drop the stored observations of keyframes that will never be part of a window again (marginalised / removed from the map): the store is otherwise
   grow-only, and every svs_ba_window_update filters and sorts all of it.  A failed svs_ba_window_update leaves the store as it found it. */
int svs_ba_window_forget_keyframes(svs_ba *ba, const int32_t *h_pose_ids, int n);
/* optimizer.optimize(num_iters) (slam_graph.cpp:346) incl. LM control flow; allreduce may be
   NULL (single GPU) */
int svs_ba_optimize(svs_ba *ba, svs_allreduce_fn allreduce, void *user, svs_ba_stats *stats);
/* throughput mode: n independent windows (each svs_ba created on its OWN context, i.e. its own stream), all enqueued before the
   first wait so that their kernels overlap on the device; stats[n] optional.  Single-GPU (no collectives). */
int svs_ba_optimize_batch(svs_ba *const *bas, int n, svs_ba_stats *stats);
/* restoreDataFromG2o (slam_graph.cpp:1035-1058): poses [P][12], psi [L][3] */
int svs_ba_get_state(svs_ba *ba, double *h_poses, double *h_psi);
/* copyDataToG2o device to device: the window svs_map_prepare_window left in `map` becomes this handle's problem.  Poses (T_me_from_world of the final window, in
   its order) and psi = (x / z, y / z, 1 / z) of xyz_anchor (invert_depth, maths_utils.h:66-69; the active points in ascending id) are read from the map AT THIS
   MOMENT; the edge list is assembled by the kernels of svs_ba_window_update from the map's measured store -- no observation record is copied or uploaded -- with
   that call's filter (slam_graph.cpp:1001-1006): the observations of the active points in keyframes of the final window.  The observer set is the map's
   feature_table pairs; the reference iterates vis_set, which addNewPointsToMap / addNewObsToOldPoints keep equal to them: a caller whose vis_set differs must
   not use this call.  Only the constraints cross the link (h_cons: frame IDS of the final window, copyContraintsToG2o stays with the caller).  State comes back
   through svs_ba_get_state in the order of the final window / the active list.  The handle's own observation store (svs_ba_window_update) is not touched.
   SVS_ERR_INVALID: no valid prepared window, handles of two contexts, a handle with a communicator, a constraint outside the window -- each before the handle is
   touched: its problem is then as it was. */
int svs_ba_window_from_map(svs_ba *ba, svs_map *map, int C, const svs_ba_constraint *h_cons, const svs_cam *cam, const svs_ba_params *prm);
/* restoreDataFromG2o on the device (slam_graph.cpp:1035-1058), one launch, ASYNCHRONOUS: window pose i to the map's keyframe of its id, xyz_anchor =
   invert_depth(psi) to the map's point of its id.  Valid only while the handle's problem is the one svs_ba_window_from_map built from this map's prepared window */
int svs_ba_store_to_map(svs_ba *ba, svs_map *map);
/* svs_ba_window_from_map with copyContraintsToG2o (slam_graph.cpp:937-981) done from the map's edge table: for i over the final window in its order, for j over
   it in its order, j != i, an edge between them and at least one of the two OUTER: one constraint pose1 = id_i, pose2 = id_j, T_21 = T_j_from_i -- every such
   edge twice, once per direction, as the reference's double loop adds it (its order is that of an unordered_map; ours is the one just stated).  Only the list
   of (window index i, window index j, edge slot, direction) is staged; one gather launch writes the svs_ba_constraint records on the device and applies
   pose_inv for the direction against storage (slam_graph.hpp:281).  An edge of that list that is not marginalised: SVS_ERR_INVALID before the handle is
   touched (the reference asserts, :972); the other refusals are svs_ba_window_from_map's */
int svs_ba_window_from_map_edges(svs_ba *ba, svs_map *map, const svs_cam *cam, const svs_ba_params *prm);
/* the handle's constraints with window INDICES in pose1 / pose2, after any way to set a problem; *n = their count, h_cons == NULL returns only that (blocking) */
int svs_ba_window_constraints(svs_ba *ba, int32_t *n, svs_ba_constraint *h_cons);
/* landmark-sharded operation over a library-owned communicator: svs_ba_optimize(ba, NULL, NULL, stats) then all-reduces the
   packed reduced system and the two trial sums of every LM trial (32 doubles: each sum is kept in 16 partial slots) (and, once per problem, the co-visibility pattern) with
   ncclAllReduce on the ctx stream.  comm == NULL detaches.  A non-NULL `allreduce` argument of svs_ba_optimize takes precedence
   (test hook). */
int svs_ba_set_comm(svs_ba *ba, svs_comm *comm);
/* experiment / test switches of one optimizer (0 = default behaviour): "no_speculation", "one_front", "no_fused_solve",
   "no_lds_solve", "no_grid_solve", "no_tile_solve" (wide envelopes: the multi-workgroup Cholesky by block rows instead of the tile-resident one), "no_fused_cons", "debug" (1: phase timers, 2: Schur kernel timeline), "nw" (waves per Schur workgroup, 4..8),
   "p1" (rows of the reversed front), "group" (anchors dealt round-robin), "host_threads", "host_marshal" (svs_ba_set_problem: 0 = device marshalling from
   8k edges, 1 = always host, 2 = always device), "no_graph" (1: svs_ba_optimize enqueues kernel by kernel instead of replaying its recorded graph,
   see svs_ba_graph_stats), "no_lds_panel" (1: the fused solve's back-substitution panel through global memory, rounds 3-5).  The environment (SVS_BA_*,
   SVS_HOST_THREADS) only supplies the initial values, read once by svs_ba_create; values are clamped to their valid ranges. */
int svs_ba_set_option(svs_ba *ba, const char *name, int value);
/* building blocks exposed for parity tests and profiling */
int svs_ba_reset_state(svs_ba *ba, const double *h_poses, const double *h_psi);
int svs_ba_reduced_system(svs_ba *ba, double lambda, double *h_Hred /* (6P)^2 full sym */,
                          double *h_bred /* 6P */, double *h_chi2);
/* the assembled edge list in slot order (wide | anchor | point | pose), window INDICES in .point / .pose / .anchor, after any of the three ways to set a
   problem; *n = its length, h_edges == NULL returns only that (blocking) */
int svs_ba_window_edges(svs_ba *ba, int32_t *n, svs_ba_edge *h_edges);
/* the layout the next Schur and back-substitution launches take: waves per workgroup (4..8; the one svs_ba_set_problem laid the wave chunks out
   for, option "nw", or the smallest that gets the grid down to one workgroup per CU) and whether the Schur pass accumulates in the big LDS
   pool (one workgroup per CU, 22-pose window; always at 5..8 waves) or the small one (two per CU, 16 poses: four waves with more workgroups than CUs) */
int svs_ba_schur_layout(svs_ba *ba, int32_t *waves_per_workgroup, int32_t *big_pool);
/* one LM trial at `lambda` from the caller's pose step h_xp (6P, the caller's pose order) instead of the solve's: the Schur pass at the current
   state, trial poses exp(x_p) T, then the back-substitution x_l = D^-1 (b_l - W^T x_p) with the trial chi2 -- the kernels svs_ba_optimize runs
   around its solve, without graph or speculation.  Out (each optional): trial poses [P][12], trial landmarks [L][3], trial chi2 (edges +
   constraints), landmark share of the LM scale sum x_l . (lambda x_l + b_l).  The optimizer's current state is left unchanged. */
int svs_ba_trial(svs_ba *ba, double lambda, const double *h_xp, double *h_poses_trial, double *h_psi_trial, double *h_chi2_trial,
                 double *h_scale_l);
/* what the last svs_ba_set_problem led to: solve_kind 0 = global-memory blocked Cholesky, 1 = LDS-window pipeline, 2 = fused
   register-resident elimination (one front), 3 = the same with two fronts, 4 = multi-workgroup blocked Cholesky (one block row per step, trailing matrix in global memory; option "no_tile_solve"), 5 = multi-workgroup
   tile-resident blocked Cholesky (24 x 24 tiles owned by workgroups in LDS: the default for wide envelopes); envelope_rows = widest filled block row of the reduced
   system (+1); wave chunks of the Schur kernel; landmarks with more than 64 observations */
int svs_ba_info(svs_ba *ba, int32_t *solve_kind, int32_t *envelope_rows, int32_t *n_chunks, int32_t *n_wide);
/* the solve's pose order (what LinearSolverCSparse's block ordering is to the reference, slam_graph.cpp:1063-1074): envelope_rows above is that of the order the solve
   runs in; *envelope_rows_caller_order the one of the caller's pose order; *ordered = 1 when a fill-reducing order (reverse Cuthill-McKee on the pose block graph) is
   in use -- taken when it narrows the filled envelope by a quarter or more, e.g. a loop closure on a chain of keyframes; h_perm (optional, [P]): solver row k is
   the caller's pose h_perm[k] (the identity when not ordered).  Option "no_order" (svs_ba_set_option) keeps the caller's order. */
int svs_ba_order_info(svs_ba *ba, int32_t *ordered, int32_t *envelope_rows_caller_order, int32_t *h_perm);
/* profiling: bracket the Schur, solve and back-substitution kernels of every LM trial with hipEvents on the ctx stream.
   Off by default: each event record costs ~4 us of stream time (12 per optimize() = 15 % of it at 50 KF / 20k). */
int svs_ba_set_timing(svs_ba *ba, int on);
/* last-call timing of the dominant kernels, ms (zeros unless svs_ba_set_timing(ba, 1)) */
int svs_ba_kernel_times(svs_ba *ba, float *reduce_ms, float *solve_ms, float *backsub_ms,
                        int32_t *n_reduce_launches);
/* How svs_ba_optimize enqueues its work.  The all-accepted optimize of a resident window (SlamGraph::optimize, slam_graph.cpp:312-355: num_iters x { build, solve,
   update, compare }) has a fixed launch topology; the library records it once per problem layout (when a layout is seen for the second time) as a HIP graph and replays it with one launch per call (the first rejected
   trial falls back to the host-driven loop, as before).  *launches: optimizes replayed from a graph so far; *captures: recordings made (a new one whenever the layout,
   the buffers or the parameters change).  Option "no_graph" (svs_ba_set_option) keeps the kernel-by-kernel path.  Not used with an all-reduce callback / communicator,
   with svs_ba_set_timing, or with the multi-workgroup solves of wide envelopes. */
int svs_ba_graph_stats(svs_ba *ba, int64_t *launches, int64_t *captures);

#ifdef __cplusplus
}
#endif
#endif
