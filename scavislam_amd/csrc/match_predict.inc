// match_predict.inc -- the per-point scalar part of the guided matcher: relative poses per (stream, keyframe) and one PointPred per candidate point; included first
// by match.hip.  match_pose_kernel, match_predict_kernel<FUSE>; d_in_frame and d_warp_f are theirs alone, d_affine_inv is shared with match_subpix.inc.  Whichever kernel forms the poses also writes the level
// table match_kernel3 reads (LevelTab).

__device__ __forceinline__ bool d_in_frame(const svs_cam &c, int u, int v, int border) {
  return u >= border && v >= border && u < c.w - border && v < c.h - border;
}
__device__ __forceinline__ void d_warp_f(const double *T, double depth, const svs_cam &cam, double ku, double kv, double *o) {
  double p[3] = {depth * ((ku - cam.cx) / cam.f), depth * ((kv - cam.cy) / cam.f), depth * 1.0};
  double q[3];
  pose_act(T, p, q);
  o[0] = cam.f * (q[0] / q[2]) + cam.cx;
  o[1] = cam.f * (q[1] / q[2]) + cam.cy;
}
// the inverse of warpAffinve's local affine A (matcher.cpp:411-426) at the point's anchor observation; match_predict_kernel, and subpix_predict_kernel of match_subpix.inc
__device__ __forceinline__ void d_affine_inv(const double *T_cur_from_anchor, const svs_candidate_point &ap, const svs_cam &cam, double *inv) {
  // f(uv), f(uv + e_x), f(uv + e_y) (matcher.cpp:411-413); x + 0.0 is exact
  double f0[2], fu[2], fv[2];
  d_warp_f(T_cur_from_anchor, ap.xyz_anchor[2], cam, ap.anchor_obs_pyr[0] + 0.0, ap.anchor_obs_pyr[1] + 0.0, f0);
  d_warp_f(T_cur_from_anchor, ap.xyz_anchor[2], cam, ap.anchor_obs_pyr[0] + 1.0, ap.anchor_obs_pyr[1] + 0.0, fu);
  d_warp_f(T_cur_from_anchor, ap.xyz_anchor[2], cam, ap.anchor_obs_pyr[0] + 0.0, ap.anchor_obs_pyr[1] + 1.0, fv);
  const double a00 = fu[0] - f0[0], a01 = fu[1] - f0[1], a10 = fv[0] - f0[0], a11 = fv[1] - f0[1];
  const double invdet = 1.0 / (a00 * a11 - a01 * a10);
  inv[0] = a11 * invdet; inv[1] = -a01 * invdet; inv[2] = -a10 * invdet; inv[3] = a00 * invdet;
}

// The two relative poses a candidate needs depend only on (camera stream, anchor keyframe), not on
// the point: T_cur_from_anchor = T_cur_from_w * T_anchor_from_w^-1 (matcher.cpp:113) and
// (T_anchor_from_w * T_w_from_actkey)^-1 (matcher.cpp:393-394).  One lane per pair, same operation
// order as the per-point formulation => bit-identical values, ~250 f64 ops less per wavefront.
__global__ void match_pose_kernel(MatchParams M, double *__restrict__ out) {
  const svs_match_args &A = M.a;
  const int kf = blockIdx.x * blockDim.x + threadIdx.x, slot = blockIdx.y;
  if (blockIdx.x == 0 && slot == 0) {
#pragma unroll
    for (int l = 0; l < SVS_NUM_PYR_LEVELS; ++l)
      if ((int)threadIdx.x == l && l < M.fv.n_levels) {
        LevelTab t;
        t.bm = M.fv.bm[l]; t.cimg = A.d_cur_pyr[l]; t.bm_bstride = M.fv.bm_bstride[l]; t.cur_bstride = A.cur_bstride[l];
        t.bm_stride = M.fv.bm_stride[l]; t.cstride = A.cur_stride[l]; t.w = A.cam_vec[l].w; t.h = A.cam_vec[l].h;
        t.xhi = min(M.fv.gx[l] * M.fv.cell_w[l], A.cam_vec[l].w - 6); t.yhi = min(M.fv.gy[l] * M.fv.cell_h[l], A.cam_vec[l].h - 6);      // isInFrame(uv, 6) and inside the cell grid
        t.gap = M.fv.bm_gap[l]; t.pad_ = 0;
        M.lt[l] = t;
      }
  }
  if (kf >= A.n_kf) return;
  double kfT[12], Tcw[12], Twk[12], t0[12], t1[12];
  for (int i = 0; i < 12; ++i) { kfT[i] = A.d_kfs[(size_t)slot * A.kf_bstride + kf].T_anchor_from_w[i]; Tcw[i] = A.d_T_cur_from_w[(size_t)slot * 12 + i]; Twk[i] = A.d_T_w_from_actkey[(size_t)slot * 12 + i]; }
  pose_inv(kfT, t0);
  pose_mul(Tcw, t0, t1);
  double *o = out + ((size_t)slot * A.n_kf + kf) * 24;
  for (int i = 0; i < 12; ++i) o[i] = t1[i];
  pose_mul(kfT, Twk, t0);
  pose_inv(t0, t1);
  for (int i = 0; i < 12; ++i) o[12 + i] = t1[i];
}

// computePrediction (matcher.cpp:98-142) and the affine set-up of warpAffinve (:403-426), one lane per candidate point.
// The same f64 expressions as before, evaluated once per point instead of redundantly by the 64 lanes of its wave.
template <bool FUSE>
__global__ __launch_bounds__(64) void match_predict_kernel(MatchParams M) {
  const svs_match_args &A = M.a;
  const int ip = blockIdx.x * 64 + threadIdx.x, slot = blockIdx.y;
  __shared__ double s_kfT[FUSE ? PRED_FUSE_MAX_KF : 1][24];
  if constexpr (FUSE) {
    if (blockIdx.x == 0 && slot == 0) {                  // the level table match_kernel3 reads (match_pose_kernel's other job)
#pragma unroll
      for (int l = 0; l < SVS_NUM_PYR_LEVELS; ++l)
        if ((int)threadIdx.x == l && l < M.fv.n_levels) {
          LevelTab t;
          t.bm = M.fv.bm[l]; t.cimg = A.d_cur_pyr[l]; t.bm_bstride = M.fv.bm_bstride[l]; t.cur_bstride = A.cur_bstride[l];
          t.bm_stride = M.fv.bm_stride[l]; t.cstride = A.cur_stride[l]; t.w = A.cam_vec[l].w; t.h = A.cam_vec[l].h;
          t.xhi = min(M.fv.gx[l] * M.fv.cell_w[l], A.cam_vec[l].w - 6); t.yhi = min(M.fv.gy[l] * M.fv.cell_h[l], A.cam_vec[l].h - 6);
          t.gap = M.fv.bm_gap[l]; t.pad_ = 0;
          M.lt[l] = t;
        }
    }
    const int kf = threadIdx.x;
    if (kf < A.n_kf) {
      // T_cur_from_w = T_cur_from_actkey * T_actkey_from_w, T_w_from_actkey = T_actkey_from_w^-1 (matcher.cpp:326-330; frontend_pose_kernel's operation order), then the
      // two relative poses of keyframe kf (match_pose_kernel's): the same expressions in the same order, i.e. the same bits, computed per block instead of fetched
      double Tc[12], Ta[12], Tcw[12], Twk[12], kfT[12], t0[12], t1[12];
#pragma unroll
      for (int i = 0; i < 12; ++i) { Tc[i] = M.src_T[(size_t)slot * 12 + i]; Ta[i] = M.src_Ta[(size_t)slot * 12 + i]; kfT[i] = A.d_kfs[(size_t)slot * A.kf_bstride + kf].T_anchor_from_w[i]; }
      pose_mul(Tc, Ta, Tcw);
      pose_inv(Ta, Twk);
      pose_inv(kfT, t0);
      pose_mul(Tcw, t0, t1);
#pragma unroll
      for (int i = 0; i < 12; ++i) s_kfT[kf][i] = t1[i];
      pose_mul(kfT, Twk, t0);
      pose_inv(t0, t1);
#pragma unroll
      for (int i = 0; i < 12; ++i) s_kfT[kf][12 + i] = t1[i];
    }
    __syncthreads();
  }
  if (ip >= A.n_pts) return;
  const svs_candidate_point ap = A.d_pts[(size_t)slot * A.pts_bstride + ip];
  PointPred pr;
  pr.status = SVS_MATCH_OK; pr.ui = pr.vi = 0; pr.lvl = ap.anchor_level; pr.kfi = ap.kf_index; pr.pad_ = 0; pr.pad2_ = 0;
  pr.inv[0] = pr.inv[1] = pr.inv[2] = pr.inv[3] = 0; pr.key_uv[0] = ap.anchor_obs_pyr[0]; pr.key_uv[1] = ap.anchor_obs_pyr[1];
  pr.xyz_actkey[0] = pr.xyz_actkey[1] = pr.xyz_actkey[2] = 0;
  pr.kimg = nullptr; pr.kstride = 0; pr.xb = pr.yb = 0x7fffffff; pr.pb_lo = 0;
  if (ap.kf_index < 0 || ap.kf_index >= A.n_kf) pr.status = SVS_MATCH_NO_ANCHOR;
  else if (ap.anchor_level < 0 || ap.anchor_level >= M.fv.n_levels) pr.status = SVS_MATCH_NONE;  // no feature_tree for that level
  if (pr.status == SVS_MATCH_OK) {
    const svs_cam cam = A.cam_vec[ap.anchor_level];
    const double *kfT = FUSE ? s_kfT[ap.kf_index] : M.kf_T + ((size_t)slot * A.n_kf + ap.kf_index) * 24;
    double T_cur_from_anchor[12], xyz_cur[3];
#pragma unroll
    for (int i = 0; i < 12; ++i) T_cur_from_anchor[i] = kfT[i];
    pose_act(T_cur_from_anchor, ap.xyz_anchor, xyz_cur);
    const double uv0 = cam.f * (xyz_cur[0] / xyz_cur[2]) + cam.cx;
    const double uv1 = cam.f * (xyz_cur[1] / xyz_cur[2]) + cam.cy;
    const double depth_cur = 1. / xyz_cur[2], depth_anchor = 1. / ap.xyz_anchor[2];
    if (!d_in_frame(cam, (int)ap.anchor_obs_pyr[0], (int)ap.anchor_obs_pyr[1], 4)) pr.status = SVS_MATCH_BORDER;
    else if (depth_cur > depth_anchor * 3 || depth_anchor > depth_cur * 3) pr.status = SVS_MATCH_DEPTH;
    else if (!(fabs(uv0) < 1e9) || !(fabs(uv1) < 1e9)) pr.status = SVS_MATCH_NONE;
    if (pr.status == SVS_MATCH_OK) {
      pr.ui = (int)uv0; pr.vi = (int)uv1;
      d_affine_inv(T_cur_from_anchor, ap, cam, pr.inv);
      double T_actkey_from_anchor[12];
#pragma unroll
      for (int i = 0; i < 12; ++i) T_actkey_from_anchor[i] = kfT[12 + i];
      pose_act(T_actkey_from_anchor, ap.xyz_anchor, pr.xyz_actkey);
      const int lvl = ap.anchor_level, R = A.search_radius;
      const svs_keyframe &kf = A.d_kfs[(size_t)slot * A.kf_bstride + ap.kf_index];
      pr.kimg = kf.pyr[lvl]; pr.kstride = kf.stride[lvl];
      const int gx = M.fv.gx[lvl], gy = M.fv.gy[lvl], cw = M.fv.cell_w[lvl], chh = M.fv.cell_h[lvl];
      const int x0 = pr.ui - R, y0 = pr.vi - R;
      int cxa = 0, cya = 0;
      for (int q = 1; q < gx; ++q) cxa += max(x0, 0) >= q * cw;
      for (int q = 1; q < gy; ++q) cya += max(y0, 0) >= q * chh;
      pr.xb = cxa + 1 < gx ? (cxa + 1) * cw : 0x7fffffff; pr.yb = cya + 1 < gy ? (cya + 1) * chh : 0x7fffffff;
      pr.pb_lo = max(x0, 0) + M.fv.bm_gap[lvl] * cxa;
    }
  }
  M.pred[(size_t)slot * A.n_pts + ip] = pr;
  if (M.keys) {           // bucket of the point for match_order_kernel: (level, cell of the predicted position); the points that are not searched go last
    int b = 3 * M.ord_nb;
    if (pr.status == SVS_MATCH_OK) {
      const int bx = min(max(pr.ui, 0) >> M.ord_sx, M.ord_nbx - 1), by = max(pr.vi, 0) >> M.ord_sy;
      b = min(pr.lvl * M.ord_nb + by * M.ord_nbx + bx, 3 * M.ord_nb - 1);
    }
    M.keys[(size_t)slot * A.n_pts + ip] = b;
  }
}
