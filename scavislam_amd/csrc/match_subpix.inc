// match_subpix.inc -- the optional sub-pixel refinement of a match (GuidedMatcher::subpixelAccuracy, matcher.cpp:241-309, called by returnBestMatch :198; the
// reference keeps its body behind `#if 0`); included last by match.hip.  The arithmetic is subpix_core.h's, shared with the host (tests/cpp/subpix_host.cpp) and restated
// in tests/subpix_model.py, which is the definition.
//   subpix_predict_kernel   ONE LANE per record (the stateless call only): the inverse affine of an OK record's point, from the arguments svs_match took --
//                           match_predict_kernel's expressions on match_pose_kernel's pose, the same bits.  The front end skips it and reads the PointPred records the
//                           matcher has just left
//   match_subpix_kernel     ONE WAVEFRONT per record, lane = pixel 8 h + w of the 8 x 8 patch: the 10 x 10 key patch through the LDS (every lane its own pixel, 36 lanes
//                           a border pixel too), the gradients and the normal matrix once, then per iteration four byte taps of the current image, one bilinear and
//                           one butterfly for the two f64 sums; lane 0 rewrites the observation (or the status) and the info record
// Records that are not SVS_MATCH_OK are read no further than their status and never written.

struct SubpixParams {
  svs_match_args a;            // what svs_match was called with (strides filled in)
  svs_subpix_params prm;
  PointPred *pred;             // [n_batch][n_pts]: status, lvl, inv, key_uv, kimg, kstride of the OK records
  svs_match_result *res;       // [n_batch][n_pts], a.out_bstride apart
  svs_subpix_info *info;       // the same shape, or NULL
  int bps;                     // workgroups per stream: the grid is one-dimensional (blockIdx.x = stream * bps + block), no stream count meets a grid limit
};

__global__ __launch_bounds__(64) void subpix_predict_kernel(SubpixParams S) {
  const svs_match_args &A = S.a;
  const int slot = blockIdx.x / S.bps, ip = (blockIdx.x - slot * S.bps) * 64 + threadIdx.x;
  if (ip >= A.n_pts) return;
  if (S.res[(size_t)slot * A.out_bstride + ip].status != SVS_MATCH_OK) return;
  const svs_candidate_point ap = A.d_pts[(size_t)slot * A.pts_bstride + ip];
  PointPred &pr = S.pred[(size_t)slot * A.n_pts + ip];
  if (ap.kf_index < 0 || ap.kf_index >= A.n_kf || ap.anchor_level < 0 || ap.anchor_level >= SVS_NUM_PYR_LEVELS) {      // no record of svs_match's is OK with these
    pr.status = SVS_MATCH_NO_ANCHOR;
    return;
  }
  const svs_keyframe &kf = A.d_kfs[(size_t)slot * A.kf_bstride + ap.kf_index];
  double kfT[12], Tcw[12], t0[12], T_cur_from_anchor[12];
#pragma unroll
  for (int i = 0; i < 12; ++i) { kfT[i] = kf.T_anchor_from_w[i]; Tcw[i] = A.d_T_cur_from_w[(size_t)slot * 12 + i]; }
  pose_inv(kfT, t0);                                   // T_cur_from_anchor = T_cur_from_w * T_anchor_from_w^-1 (matcher.cpp:113; match_pose_kernel)
  pose_mul(Tcw, t0, T_cur_from_anchor);
  d_affine_inv(T_cur_from_anchor, ap, A.cam_vec[ap.anchor_level], pr.inv);
  pr.status = SVS_MATCH_OK; pr.lvl = ap.anchor_level;
  pr.key_uv[0] = ap.anchor_obs_pyr[0]; pr.key_uv[1] = ap.anchor_obs_pyr[1];
  pr.kimg = kf.pyr[ap.anchor_level]; pr.kstride = kf.stride[ap.anchor_level];
}

__global__ __launch_bounds__(256) void match_subpix_kernel(SubpixParams S) {
  __shared__ uint8_t s_key[WAVES_PER_BLOCK][104];      // K[iy][ix] at 10 iy + ix
  const svs_match_args &A = S.a;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int slot = blockIdx.x / S.bps;
  const int ip = __builtin_amdgcn_readfirstlane((blockIdx.x - slot * S.bps) * WAVES_PER_BLOCK + wave);
  if (ip >= A.n_pts) return;                           // wave-uniform
  svs_match_result *o = S.res + (size_t)slot * A.out_bstride + ip;
  int state = SVS_SUBPIX_UNTOUCHED, n_iter = 0;
  float px = 0.f, py = 0.f;
  if (__builtin_amdgcn_readfirstlane(o->status) == SVS_MATCH_OK) {
    const int u = __builtin_amdgcn_readfirstlane(o->u), v = __builtin_amdgcn_readfirstlane(o->v);
    const PointPred *pp = S.pred + (size_t)slot * A.n_pts + ip;
    state = SVS_SUBPIX_SHIFT;                          // a match outside the matcher's own margin (isInFrame(uv, 6)): nothing is read for it
    const int lvl = __builtin_amdgcn_readfirstlane(pp->status) == SVS_MATCH_OK ? __builtin_amdgcn_readfirstlane(pp->lvl) : -1;
    const svs_cam cam = A.cam_vec[max(lvl, 0)];
    if (lvl >= 0 && u >= 6 && v >= 6 && u < cam.w - 6 && v < cam.h - 6) {
      const int h = lane >> 3, w = lane & 7;
      const uint8_t *kimg = pp->kimg;
      const int kstride = pp->kstride;
      uint8_t *sk = s_key[wave];
      const int kc = key_pixel_at(pp->inv, pp->key_uv, kimg, kstride, cam.w, cam.h, w + 1, h + 1);
      sk[10 * (h + 1) + w + 1] = (uint8_t)kc;
      if (lane < 36) {                                 // the border: rows 0 and 9, then columns 0 and 9 of rows 1 .. 8
        const int bx = lane < 10 ? lane : lane < 20 ? lane - 10 : lane < 28 ? 0 : 9;
        const int by = lane < 10 ? 0 : lane < 20 ? 9 : lane < 28 ? lane - 19 : lane - 27;
        sk[10 * by + bx] = (uint8_t)key_pixel_at(pp->inv, pp->key_uv, kimg, kstride, cam.w, cam.h, bx, by);
      }
      wave_lds_sync();
      const int ex = (int)sk[10 * (h + 1) + w + 2] - (int)sk[10 * (h + 1) + w], ey = (int)sk[10 * (h + 2) + w + 1] - (int)sk[10 * h + w + 1];
      const float gx = svs_spx_grad(sk[10 * (h + 1) + w + 2], sk[10 * (h + 1) + w]), gy = svs_spx_grad(sk[10 * (h + 2) + w + 1], sk[10 * h + w + 1]);
      // the normal matrix: sums of quarters below 2^53, exact in any order and any format that holds them -- summed as integers (gx = ex / 2), a quarter of the shuffles
      const double H00 = 0.25 * (double)wave_sum(ex * ex), H01 = 0.25 * (double)wave_sum(ex * ey), H11 = 0.25 * (double)wave_sum(ey * ey);
      const double det = svs_spx_det(H00, H01, H11);
      if (!(det > 0)) state = SVS_SUBPIX_SINGULAR;
      else {
        const uint8_t *cimg = A.d_cur_pyr[lvl] + (size_t)slot * A.cur_bstride[lvl];
        const int cstride = A.cur_stride[lvl];
        const float kf32 = (float)kc;
        state = SVS_SUBPIX_REFINED;
        for (int it = 1; it <= S.prm.iterations; ++it) {
          int ox, oy;
          float sx, sy;
          svs_spx_axis(px, w, &ox, &sx);
          svs_spx_axis(py, h, &oy, &sy);
          const uint8_t *t = cimg + (size_t)(v + oy) * cstride + (u + ox);      // columns u - 6 .. u + 6, rows v - 6 .. v + 6: inside the image
          const float d = svs_spx_bilinear(sx, sy, t[0], t[cstride], t[1], t[cstride + 1]) - kf32;
          double b0 = (double)gx * (double)d, b1 = (double)gy * (double)d;      // exact products
          // the balanced tree over the pixel index, adjacent pairs first; a + b = b + a, so both lanes of a pair hold the same bits and so does the whole wave at the end
#pragma unroll
          for (int k = 1; k < 64; k <<= 1) { b0 += __shfl_xor(b0, k, 64); b1 += __shfl_xor(b1, k, 64); }
          float dx, dy;
          svs_spx_step(H00, H01, H11, det, b0, b1, &dx, &dy);
          n_iter = it;
          const int r = svs_spx_update(&px, &py, dx, dy, S.prm.max_shift, S.prm.eps);
          if (r == SVS_SPX_OUT) state = SVS_SUBPIX_SHIFT;
          if (r != SVS_SPX_GO_ON) break;                 // wave-uniform
        }
        if (state == SVS_SUBPIX_REFINED) {
          float nu, nv;
          int iu, iv;
          svs_spx_position(u, px, &nu, &iu);
          svs_spx_position(v, py, &nv, &iv);
          const float disp = A.d_disp[(size_t)slot * A.disp_bstride + (size_t)(iv << lvl) * A.disp_stride + (iu << lvl)];
          double o0, o1, o2;
          if (!svs_spx_observation(nu, nv, lvl, disp, &o0, &o1, &o2)) {
            state = SVS_SUBPIX_NO_DISP;
            if (lane == 0) o->status = SVS_MATCH_NO_DISP;
          } else if (lane == 0) { o->obs[0] = o0; o->obs[1] = o1; o->obs[2] = o2; }
        } else px = py = 0.f;                          // the record is kept
      }
    }
  }
  if (S.info && lane == 0) {
    svs_subpix_info r;
    r.dx = px; r.dy = py; r.n_iter = n_iter; r.state = state;
    S.info[(size_t)slot * A.out_bstride + ip] = r;
  }
}

// the launches behind the checks: with `pred` the PointPred records are taken as they are (the front end: svs_match has just left them), without they are formed first
static int subpix_run(svs_ctx *ctx, const svs_match_args *a, const svs_subpix_params *prm, PointPred *pred, svs_match_result *d_results, svs_subpix_info *d_info) {
  SubpixParams S;
  S.a = *a; S.prm = *prm; S.res = d_results; S.info = d_info;
  if (!S.a.pts_bstride) S.a.pts_bstride = (size_t)a->n_pts;
  if (!S.a.out_bstride) S.a.out_bstride = (size_t)a->n_pts;
  SVS_REQUIRE(ctx, S.a.pts_bstride >= (size_t)a->n_pts && S.a.out_bstride >= (size_t)a->n_pts);
  SVS_REQUIRE(ctx, (size_t)a->n_batch * (size_t)div_up(a->n_pts, WAVES_PER_BLOCK) < ((size_t)1 << 31));
  if (!pred) {
    SVS_REQUIRE(ctx, a->d_pts && a->d_kfs && a->n_kf >= 1 && a->d_T_cur_from_w);
    void *buf = nullptr;
    { const int rc = svs_ctx_match_scratch(ctx, (size_t)a->n_batch * a->n_pts * sizeof(PointPred), &buf); if (rc) return rc; }
    ctx->match_pred = nullptr;                         // the matcher's records are gone
    S.pred = static_cast<PointPred *>(buf);
    S.bps = div_up(a->n_pts, 64);
    hipLaunchKernelGGL(subpix_predict_kernel, dim3(S.bps * a->n_batch), dim3(64), 0, ctx->stream, S);
    SVS_LAUNCH_CHECK(ctx);
  } else S.pred = pred;
  S.bps = div_up(a->n_pts, WAVES_PER_BLOCK);
  hipLaunchKernelGGL(match_subpix_kernel, dim3(S.bps * a->n_batch), dim3(64 * WAVES_PER_BLOCK), 0, ctx->stream, S);
  SVS_LAUNCH_CHECK(ctx);
  return SVS_OK;
}
