// register.hip -- the back end's re-registration of a keyframe against the map: Backend::localRegisterFrame (backend.cpp:549-611) and Backend::globalLoopClosure
// (:830-1001) for a batch of requests as one chain of launches on the context's stream -- one staged upload, one download, no host round trip in between:
//   reg_cull_kernel     one workgroup per request, one lane per source point: pointsVisibleInRoot (:472-546) / the loop at :853-893.  The relative pose of every
//                       keyframe-table entry is formed once (f64, no contraction), the points are projected and tested, the survivors are compacted IN SOURCE ORDER
//                       (wave ballot, the waves' counts meet in LDS, a running offset over the chunks of the workgroup: no atomic decides an order), the vertex table
//                       is marked, the stored FAST thresholds go to the handle's svs_fast and exit 1 (:577) is decided from the count
//   reg_gather_kernel   only when the root frames of a batch do not lie at one stride: copies them into the handle's own pyramid / disparity slots
//   svs_fast_detect(trials = 0), svs_match(radius 10), svs_motion_only(25)        the entry points of fast.hip / match.hip / motion.hip on the handle's buffers
//   reg_pose_kernel     a request's pose behind the first refinement is kept, T_cur_from_w for the second match is formed, exit 2 (:751) is decided
//   svs_match(radius 4), svs_motion_only(15)
//   reg_gate_kernel     one workgroup per request, one lane per record of the second match: the gate inequality of processMatchedPoints (gate.h), then
//                       keyframesToRegister's walk over the point's observer row (:650-696) with the per-keyframe counters in LDS (LDS atomics: integer sums, any
//                       order gives the same value), or the frame-wide counters of :934-943; one pass applies the thresholds of :707-711 / :953-961
// A request that left at an exit has its candidate records turned into kf_index = -1, which the matcher answers with SVS_MATCH_NO_ANCHOR: the later stages
// run over it and find nothing.  Requests of a batch are padded to the longest source list with such records.
// Not pinned by the reference's binaries (backend.cpp is not among them): the yardstick of the cull and the counting is tests/register_model.py.
// svs_reg_register_map_batch (at the end) runs the same chain (reg_chain) behind requests that the device-resident map (map.hip: map_request.inc, through reg_map.h) builds from ids in this
// handle's staging block; the stateless call stages them from the host.
// svs_reg_commit (behind it) is registerKeyframes / addLoopClosure for one request of such a batch: reg_commit_kernel builds the track list and the edge list from the
// chain's outputs where they lie, the map applies them (map_commit.inc through reg_map.h).
#include "common.h"
#include "fast_view.h"
#include "gate.h"
#include "pose.h"
#include "reg_map.h"
#include <string.h>
#include <algorithm>
#include <vector>

namespace {
constexpr int RC_THREADS = 512;
constexpr int RG_THREADS = 256;
constexpr int REG_MAX_KF = 1024;

// (one request as the kernels read it: reg_hdr of reg_map.h)
struct RegK {
  // the staged requests: table r at + r * (its stride) elements
  const reg_hdr *hdr;
  const svs_keyframe *kfs; size_t kf_b;
  const uint8_t *flags;                       // stride kf_b
  const svs_candidate_point *src; size_t src_b;
  const int32_t *obs_begin; size_t ob_b;      // src_b + 1
  const int32_t *obs_kf; size_t ok_b;
  // the handle's scratch
  svs_candidate_point *cand; size_t cand_b;   // [n_req][cand_b], the first n_pad of a row are records
  int n_pad;
  uint8_t *in_vt;                             // stride kf_b
  double *Trel;                               // [n_req][kf_b][12]: T_root_from_anchor
  double *T, *Tcw, *Twa, *T1;                 // [n_req][12]: T_newroot_from_oldroot, T_cur_from_w, T_w_from_actkey, the pose behind pass 1
  int32_t *n_cand, *dead;                     // [n_req]
  svs_pose_opt_stats *st1, *st2;
  // the handle's svs_fast
  FastThrView fv;
  svs_cam cams[SVS_NUM_PYR_LEVELS];
  int covis; float reproj;
  // outputs: rows of n_pad records / kf_b entries
  svs_reg_result *res; const svs_match_result *m1, *m2; int32_t *status1, *accepted, *cand_src; svs_reg_kf_stats *kfst;
};

// grid = requests
__global__ __launch_bounds__(RC_THREADS) void reg_cull_kernel(RegK K) {
  __shared__ int s_wcnt[RC_THREADS / 64];
  const int r = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const reg_hdr &H = K.hdr[r];
  const int n_kf = min(max(H.n_kf, 0), (int)K.kf_b), n_src = min(max(H.n_src, 0), K.n_pad);
  const svs_keyframe *kfs = K.kfs + (size_t)r * K.kf_b;
  const uint8_t *flags = K.flags + (size_t)r * K.kf_b;
  uint8_t *in_vt = K.in_vt + (size_t)r * K.kf_b;
  double *Trel = K.Trel + (size_t)r * K.kf_b * 12;
  for (int kf = tid; kf < (int)K.kf_b; kf += RC_THREADS) {
    in_vt[kf] = 0;
    if (kf < n_kf) {      // T_root_from_world * T_world_from_anchor (:514-517)
      double Ta[12], Tr[12], t0[12], t1[12];
#pragma unroll
      for (int i = 0; i < 12; ++i) { Ta[i] = kfs[kf].T_anchor_from_w[i]; Tr[i] = H.T_root[i]; }
      pose_inv(Ta, t0);
      pose_mul(Tr, t0, t1);
#pragma unroll
      for (int i = 0; i < 12; ++i) Trel[(size_t)kf * 12 + i] = t1[i];
    }
  }
  if (tid == 0) {         // the poses of the first match: T_newroot_from_oldroot = the identity (SE3's default, :581), matcher.cpp:326-330
    double I[12], Tr[12], t0[12];
#pragma unroll
    for (int i = 0; i < 12; ++i) { I[i] = i % 5 == 0 ? 1.0 : 0.0; Tr[i] = H.T_root[i]; }
    pose_mul(I, Tr, t0);
#pragma unroll
    for (int i = 0; i < 12; ++i) { K.T[(size_t)r * 12 + i] = I[i]; K.Tcw[(size_t)r * 12 + i] = t0[i]; }
    pose_inv(Tr, t0);
#pragma unroll
    for (int i = 0; i < 12; ++i) K.Twa[(size_t)r * 12 + i] = t0[i];
  }
  // root_frame.cell_grid2d -> the thresholds FastGrid::detect runs at (:465-467)
  for (int l = 0; l < K.fv.n_levels; ++l)
    for (int c = tid; c < K.fv.ncell[l]; c += RC_THREADS) K.fv.thr[(size_t)r * K.fv.ncell_total + K.fv.cell_base[l] + c] = H.thr[l][c];
  __syncthreads();        // in_vt is clear and Trel is written (global memory of this workgroup: visible behind the barrier)
  const svs_candidate_point *src = K.src + (size_t)r * K.src_b;
  svs_candidate_point *cand = K.cand + (size_t)r * K.cand_b;
  int32_t *cand_src = K.cand_src + (size_t)r * K.n_pad;
  int n_out = 0;
  for (int base = 0; base < n_src; base += RC_THREADS) {      // block-uniform trip count
    const int i = base + tid;
    bool keep = false;
    int kf = -1;
    if (i < n_src) {
      kf = src[i].kf_index;
      const int lvl = src[i].anchor_level;
      if ((unsigned)kf < (unsigned)n_kf && (unsigned)lvl < (unsigned)SVS_NUM_PYR_LEVELS && (flags[kf] & SVS_REG_KF_IN_WINDOW)) {
        const double *T = Trel + (size_t)kf * 12, *x = src[i].xyz_anchor;
        double p0, p1, p2;
        pose_act(T, x[0], x[1], x[2], p0, p1, p2);
        const svs_cam &cam = K.cams[lvl];
        const double u = cam.f * (p0 / p2) + cam.cx, v = cam.f * (p1 / p2) + cam.cy;      // cam_pyr.map(project2d(xyz_root)) (:522)
        if (fabs(u) < 2147483648.0 && fabs(v) < 2147483648.0) {                           // (NaN compares false)
          const int ui = (int)u, vi = (int)v;                                             // uv_pyr.cast<int>(): toward zero
          keep = ui >= 0 && vi >= 0 && ui < cam.w && vi < cam.h;                          // isInFrame(., 0)
        }
      }
    }
    const unsigned long long m = __ballot(keep);
    if (lane == 0) s_wcnt[wave] = __popcll(m);
    __syncthreads();
    int off = n_out, tot = 0;
#pragma unroll
    for (int w = 0; w < RC_THREADS / 64; ++w) { const int k = s_wcnt[w]; off += w < wave ? k : 0; tot += k; }
    if (keep) {
      const int pos = off + __popcll(m & ((1ull << lane) - 1ull));      // < n_src <= n_pad <= cand_b
      const int4 *s4 = reinterpret_cast<const int4 *>(src + i);
      int4 *d4 = reinterpret_cast<int4 *>(cand + pos);
#pragma unroll
      for (int q = 0; q < 4; ++q) d4[q] = s4[q];
      cand_src[pos] = i;
      in_vt[kf] = 1;                                                    // (:537-543; every writer stores the same value)
    }
    n_out += tot;
    __syncthreads();
  }
  const bool dead = H.mode == SVS_REG_LOCAL && n_out < K.covis;         // candidate_point_list.size() < COVIS_THR (:577)
  for (int i = tid; i < K.n_pad; i += RC_THREADS) {
    if (i >= n_out) {
      int4 *d4 = reinterpret_cast<int4 *>(cand + i);
      d4[0] = d4[1] = d4[2] = make_int4(0, 0, 0, 0);
      d4[3] = make_int4(0, -1, -1, 0);                                  // anchor_level, kf_index, point_id, pad_
      cand_src[i] = -1;
    } else if (dead) cand[i].kf_index = -1;
  }
  if (tid == 0) {
    if ((unsigned)H.root_kf < (unsigned)n_kf) in_vt[H.root_kf] = 1;     // (:571, :851)
    K.n_cand[r] = n_out;
    K.dead[r] = dead ? 1 : 0;
  }
}

// grid = (row groups, 4 planes, requests): plane l < 3 = level l of the root pyramid, plane 3 = its disparity
struct RegGather { uint8_t *pyr[SVS_NUM_PYR_LEVELS]; int stride[SVS_NUM_PYR_LEVELS]; size_t bstride[SVS_NUM_PYR_LEVELS]; float *disp; int dstride; size_t d_bstride; };
__global__ __launch_bounds__(256) void reg_gather_kernel(RegK K, RegGather G) {
  const int r = blockIdx.z, plane = blockIdx.y;
  const reg_hdr &H = K.hdr[r];
  const uint8_t *s; uint8_t *d; size_t ss, ds; int row_bytes, rows;
  if (plane < SVS_NUM_PYR_LEVELS) {
    const svs_keyframe &kf = K.kfs[(size_t)r * K.kf_b + H.root_kf];
    s = kf.pyr[plane]; ss = (size_t)kf.stride[plane];
    d = G.pyr[plane] + (size_t)r * G.bstride[plane]; ds = (size_t)G.stride[plane];
    row_bytes = K.cams[plane].w; rows = K.cams[plane].h;
  } else {
    s = reinterpret_cast<const uint8_t *>(H.disp); ss = (size_t)H.disp_stride * 4;
    d = reinterpret_cast<uint8_t *>(G.disp + (size_t)r * G.d_bstride); ds = (size_t)G.dstride * 4;
    row_bytes = K.cams[0].w * 4; rows = K.cams[0].h;
  }
  for (int y = blockIdx.x; y < rows; y += gridDim.x) {
    const uint8_t *sr = s + (size_t)y * ss;
    uint8_t *dr = d + (size_t)y * ds;                                   // the handle's rows start on 4-byte boundaries
    if ((reinterpret_cast<uintptr_t>(sr) & 3) == 0) {
      const int nw = row_bytes >> 2;
      for (int x = threadIdx.x; x < nw; x += 256) reinterpret_cast<uint32_t *>(dr)[x] = reinterpret_cast<const uint32_t *>(sr)[x];
      for (int x = (nw << 2) + threadIdx.x; x < row_bytes; x += 256) dr[x] = sr[x];
    } else {
      for (int x = threadIdx.x; x < row_bytes; x += 256) dr[x] = sr[x];
    }
  }
}

// grid = requests, one wave
__global__ __launch_bounds__(64) void reg_pose_kernel(RegK K) {
  const int r = blockIdx.x, tid = threadIdx.x;
  const bool dead = K.dead[r] != 0 || K.st1[r].num_obs < K.covis;      // track_data->obs_list.size() < COVIS_THR (:751)
  if (dead) {
    svs_candidate_point *cand = K.cand + (size_t)r * K.cand_b;
    for (int i = tid; i < K.n_pad; i += 64) cand[i].kf_index = -1;
  }
  if (tid == 0) {
    double T[12], Tr[12], t0[12];
#pragma unroll
    for (int i = 0; i < 12; ++i) { T[i] = K.T[(size_t)r * 12 + i]; Tr[i] = K.hdr[r].T_root[i]; }
    pose_mul(T, Tr, t0);
#pragma unroll
    for (int i = 0; i < 12; ++i) { K.T1[(size_t)r * 12 + i] = T[i]; K.Tcw[(size_t)r * 12 + i] = t0[i]; }
    K.dead[r] = dead ? 1 : 0;
  }
}

// grid = requests.  Dynamic LDS: 5 counters per keyframe-table entry
__global__ __launch_bounds__(RG_THREADS) void reg_gate_kernel(RegK K) {
  extern __shared__ int s_cnt[];      // [kf_b][5]: strength, u > w / 2, else, v > h / 2, else
  __shared__ int s_nacc, s_nq;
  const int r = blockIdx.x, tid = threadIdx.x;
  const reg_hdr &H = K.hdr[r];
  const int n_kf = min(max(H.n_kf, 0), (int)K.kf_b), mode = H.mode;
  for (int i = tid; i < 5 * (int)K.kf_b; i += RG_THREADS) s_cnt[i] = 0;
  if (tid == 0) { s_nacc = 0; s_nq = 0; }
  __syncthreads();
  const svs_pose_opt_stats st1 = K.st1[r], st2 = K.st2[r];
  const int n_cand = K.n_cand[r];
  int status = SVS_REG_OK;
  if (mode == SVS_REG_LOCAL && n_cand < K.covis) status = SVS_REG_FEW_CANDIDATES;
  else if (st1.num_obs < K.covis) status = SVS_REG_FEW_MATCHES_PASS1;
  else if (st2.num_obs < K.covis) status = SVS_REG_FEW_MATCHES_PASS2;
  double T[12];
#pragma unroll
  for (int k = 0; k < 12; ++k) T[k] = K.T[(size_t)r * 12 + k];
  const svs_match_result *m1 = K.m1 + (size_t)r * K.n_pad, *m2 = K.m2 + (size_t)r * K.n_pad;
  const svs_candidate_point *cand = K.cand + (size_t)r * K.cand_b;
  const int32_t *cand_src = K.cand_src + (size_t)r * K.n_pad;
  const int32_t *ob = K.obs_begin + (size_t)r * K.ob_b, *ok = K.obs_kf + (size_t)r * K.ok_b;
  const uint8_t *flags = K.flags + (size_t)r * K.kf_b, *in_vt = K.in_vt + (size_t)r * K.kf_b;
  const svs_cam cam = K.cams[0];
  const double half_w = cam.w * 0.5, half_h = cam.h * 0.5;
  for (int i = tid; i < K.n_pad; i += RG_THREADS) {
    int acc = 0;
    if (status == SVS_REG_OK && m2[i].status == SVS_MATCH_OK) {
      double d[3];
      mo_residual<false>(T, m2[i], cam, d, nullptr);                   // uvu - se3xyz_stereo_.map(T_newroot_from_oldroot, point) (:633-636)
      const int factor = 1 << cand[i].anchor_level;                    // zeroFromPyr_i(1, anchor_level)
      if (SVS_GATE_PASSES(d, factor, K.reproj)) {
        acc = 1;
        const int iu = m2[i].obs[0] > half_w ? 1 : 2, iv = m2[i].obs[1] > half_h ? 3 : 4;
        if (mode == SVS_REG_LOOP) {
          atomicAdd(&s_cnt[0], 1); atomicAdd(&s_cnt[iu], 1); atomicAdd(&s_cnt[iv], 1);
        } else {
          const int si = cand_src[i];                                   // the point's row of the observer table
          if ((unsigned)si < (unsigned)K.src_b) {
            const int e0 = max(ob[si], 0), e1 = min(ob[si + 1], (int)K.ok_b);
            for (int e = e0; e < e1; ++e) {
              const int kf = ok[e];
              if ((unsigned)kf < (unsigned)n_kf && in_vt[kf] && !(flags[kf] & SVS_REG_KF_DIRECT_NEIGHBOR)) {
                atomicAdd(&s_cnt[5 * kf], 1); atomicAdd(&s_cnt[5 * kf + iu], 1); atomicAdd(&s_cnt[5 * kf + iv], 1);
              }
            }
          }
        }
        atomicAdd(&s_nacc, 1);
      }
    }
    K.status1[(size_t)r * K.n_pad + i] = m1[i].status;
    K.accepted[(size_t)r * K.n_pad + i] = acc;
  }
  __syncthreads();
  const int half = K.covis / 2;
  for (int kf = tid; kf < (int)K.kf_b; kf += RG_THREADS) {
    svs_reg_kf_stats o;
    o.strength = s_cnt[5 * kf]; o.n_u_hi = s_cnt[5 * kf + 1]; o.n_u_lo = s_cnt[5 * kf + 2]; o.n_v_hi = s_cnt[5 * kf + 3]; o.n_v_lo = s_cnt[5 * kf + 4];
    const bool counted = mode == SVS_REG_LOOP ? kf == 0 : kf < n_kf;
    o.qualifies = counted && status == SVS_REG_OK && o.strength >= K.covis && o.n_u_hi >= half && o.n_u_lo >= half && o.n_v_hi >= half && o.n_v_lo >= half ? 1 : 0;
    o.in_vertex_table = kf < n_kf ? in_vt[kf] : 0;
    o.pad_ = 0;
    K.kfst[(size_t)r * K.kf_b + kf] = o;
    if (o.qualifies) atomicAdd(&s_nq, 1);
  }
  __syncthreads();
  if (tid == 0) {
    svs_reg_result o;
    if (status == SVS_REG_OK && s_nq == 0) status = SVS_REG_NOT_COVISIBLE;      // neighborid_to_strength.size() <= 0 (:598) / :953-961
    o.status = status; o.n_candidates = n_cand; o.n_obs_pass1 = st1.num_obs; o.n_obs_pass2 = st2.num_obs; o.n_accepted = s_nacc; o.n_qualified = s_nq;
#pragma unroll
    for (int k = 0; k < 12; ++k) { o.T_newroot_from_oldroot[k] = T[k]; o.T_pass1[k] = K.T1[(size_t)r * 12 + k]; }
    o.stats_pass1 = st1; o.stats_pass2 = st2;
    K.res[r] = o;
  }
}

// ---- svs_reg_commit: what registerKeyframes / addLoopClosure take (backend.cpp:601-604, :714-718, :945-971), from where the chain left it.  ONE workgroup for the one
// request: the qualifying table entries as an LDS bitmap, per accepted candidate a walk of its observer row against that bitmap, the kept candidates compacted IN
// CANDIDATE ORDER by wave ballots and popcount prefixes (the waves' counts meet in LDS, a running offset over the chunks: no arrival order decides a byte), the
// qualifying entries likewise (entry 0 is the root, which never qualifies in LOCAL mode; the entries behind it ascend with their ids), T_new by one lane.
constexpr int CM_THREADS = 256;
struct reg_commit_hdr { int32_t n_track, n_edges, mode, status; double T_new[12]; int32_t pad_[4]; };      // 128 bytes
struct RegCommitK {
  int r, KB, SB, OB, NP; size_t cand_b;
  const reg_hdr *hdr; const svs_reg_result *res; const svs_match_result *m2; const int32_t *accepted, *cand_src, *obs_begin, *obs_kf, *pid, *kfid;
  const svs_reg_kf_stats *kfst; const svs_candidate_point *cand;
  int query;                                  // SVS_REG_LOOP: h_walk_kf[0]
  reg_commit_hdr *out; int32_t *edge_kf, *edge_str, *ids; svs_map_track_point *track;      // [KB], [KB], [NP], [NP]
};

// the exclusive prefix of `keep` over the workgroup and the workgroup's count; every lane calls it (two barriers inside)
__device__ __forceinline__ int cm_rank(bool keep, int *s_w, int &total) {
  const unsigned long long b = __ballot(keep);
  const int lane = lane_id(), wave = threadIdx.x >> 6;
  if (lane == 0) s_w[wave] = __popcll(b);
  __syncthreads();
  int off = 0, tot = 0;
#pragma unroll
  for (int w = 0; w < CM_THREADS / 64; ++w) { const int k = s_w[w]; off += w < wave ? k : 0; tot += k; }
  __syncthreads();
  total = tot;
  return off + __popcll(b & ((1ull << lane) - 1ull));
}

__global__ __launch_bounds__(CM_THREADS) void reg_commit_kernel(RegCommitK K) {
  __shared__ uint32_t s_q[REG_MAX_KF / 32];
  __shared__ int s_w[CM_THREADS / 64];
  const int tid = threadIdx.x, r = K.r;
  const reg_hdr &H = K.hdr[r];
  const svs_reg_result &R = K.res[r];
  const int mode = H.mode, status = R.status;
  if (status != SVS_REG_OK) {                                      // block-uniform: nothing to commit
    if (tid == 0) { reg_commit_hdr o{}; o.mode = mode; o.status = status; *K.out = o; }
    return;
  }
  const int n_kf = min(max(H.n_kf, 0), K.KB), n_cand = min(max(R.n_candidates, 0), K.NP);
  const svs_reg_kf_stats *kfst = K.kfst + (size_t)r * K.KB;
  if (tid < REG_MAX_KF / 32) s_q[tid] = 0;
  __syncthreads();
  // a. the qualifying entries: the bitmap, and (LOCAL) the edge list in ascending entry = ascending id
  int n_edges = 0;
  for (int k0 = 0; k0 < n_kf; k0 += CM_THREADS) {                  // block-uniform; n_kf <= KB <= REG_MAX_KF
    const int k = k0 + tid;
    const bool q = k < n_kf && kfst[k].qualifies != 0;
    if (q) atomicOr(&s_q[k >> 5], 1u << (k & 31));
    int tot;
    const int pos = n_edges + cm_rank(q && mode == SVS_REG_LOCAL, s_w, tot);      // < KB
    if (q && mode == SVS_REG_LOCAL) { K.edge_kf[pos] = K.kfid[(size_t)r * K.KB + k]; K.edge_str[pos] = kfst[k].strength; }
    n_edges += tot;
  }
  __syncthreads();
  // b. the track list, in candidate order
  const int32_t *accepted = K.accepted + (size_t)r * K.NP, *cand_src = K.cand_src + (size_t)r * K.NP, *pid = K.pid + (size_t)r * K.NP;
  const int32_t *ob = K.obs_begin + (size_t)r * (K.SB + 1), *ok = K.obs_kf + (size_t)r * K.OB;
  const svs_match_result *m2 = K.m2 + (size_t)r * K.NP;
  const svs_candidate_point *cand = K.cand + (size_t)r * K.cand_b;
  int n_track = 0;
  for (int i0 = 0; i0 < n_cand; i0 += CM_THREADS) {                // block-uniform
    const int i = i0 + tid;
    bool keep = false;
    int si = -1;
    if (i < n_cand && accepted[i] != 0) {
      si = cand_src[i];
      if ((unsigned)si < (unsigned)K.SB) {
        if (mode == SVS_REG_LOOP) keep = true;
        else {
          const int e0 = max(ob[si], 0), e1 = min(ob[si + 1], K.OB);
          for (int e = e0; e < e1; ++e) { const int kf = ok[e]; keep |= (unsigned)kf < (unsigned)n_kf && ((s_q[kf >> 5] >> (kf & 31)) & 1u); }
        }
      }
    }
    int tot;
    const int pos = n_track + cm_rank(keep, s_w, tot);             // < n_cand <= NP
    if (keep) {
      svs_map_track_point t;
      t.center[0] = m2[i].obs[0]; t.center[1] = m2[i].obs[1]; t.center[2] = m2[i].obs[2];
      t.global_id = pid[si]; t.level = cand[i].anchor_level;
      K.track[pos] = t;
      K.ids[pos] = t.global_id;
    }
    n_track += tot;
  }
  if (tid == 0) {
    if (mode == SVS_REG_LOOP) { K.edge_kf[0] = K.query; K.edge_str[0] = n_track; n_edges = 1; }      // (:214: the list's length)
    reg_commit_hdr o{};
    o.n_track = n_track; o.n_edges = n_edges; o.mode = mode; o.status = status;
    double T[12], Tr[12], Tn[12];
#pragma unroll
    for (int k = 0; k < 12; ++k) { T[k] = R.T_newroot_from_oldroot[k]; Tr[k] = H.T_root[k]; }
    pose_mul(T, Tr, Tn);
#pragma unroll
    for (int k = 0; k < 12; ++k) o.T_new[k] = Tn[k];
    *K.out = o;
  }
}

size_t reg_align(size_t v) { return (v + 255) & ~(size_t)255; }

#define REG_CAPACITY(ctx, cond)                                                                           \
  do {                                                                                                    \
    if (!(cond)) {                                                                                        \
      char buf_[512];                                                                                     \
      snprintf(buf_, sizeof buf_, "%s:%d capacity exceeded: %s", __FILE__, __LINE__, #cond);              \
      (ctx)->err = buf_;                                                                                  \
      return SVS_ERR_CAPACITY;                                                                            \
    }                                                                                                     \
  } while (0)

// where the tables of a call lie in the staging block / the output block, for the call's longest keyframe table (KB), source list (SB) and observer table (OB).
// by_map: a call by ids (svs_reg_register_map_batch) -- the tables are built on the device, the staged bytes are the id requests behind them, and the output
// block also carries the built lists
struct RegLayout {
  size_t hdr, kfs, flags, src, ob, ok, in_bytes, mreq, mids;
  size_t res, m2, st1, acc, csrc, kfst, pid, kfid, meta, m1, out_bytes, out_bytes_m1;
  void set(size_t R, size_t KB, size_t SB, size_t OB, size_t NP, bool by_map = false) {
    size_t o = 0;
    hdr = o; o = reg_align(o + R * sizeof(reg_hdr));
    kfs = o; o = reg_align(o + R * KB * sizeof(svs_keyframe));
    flags = o; o = reg_align(o + R * KB);
    src = o; o = reg_align(o + R * SB * sizeof(svs_candidate_point));
    ob = o; o = reg_align(o + R * (SB + 1) * sizeof(int32_t));
    ok = o; o = reg_align(o + R * OB * sizeof(int32_t));
    mreq = mids = o;
    if (by_map) {
      mreq = o; o = reg_align(o + R * sizeof(map_req));
      mids = o; o = reg_align(o + R * 2 * KB * sizeof(int32_t));
    }
    in_bytes = o;
    o = 0;
    res = o; o = reg_align(o + R * sizeof(svs_reg_result));
    m2 = o; o = reg_align(o + R * NP * sizeof(svs_match_result));
    st1 = o; o = reg_align(o + R * NP * sizeof(int32_t));
    acc = o; o = reg_align(o + R * NP * sizeof(int32_t));
    csrc = o; o = reg_align(o + R * NP * sizeof(int32_t));
    kfst = o; o = reg_align(o + R * KB * sizeof(svs_reg_kf_stats));
    pid = kfid = meta = o;
    if (by_map) {
      pid = o; o = reg_align(o + R * NP * sizeof(int32_t));
      kfid = o; o = reg_align(o + R * KB * sizeof(int32_t));
      meta = o; o = reg_align(o + R * sizeof(int4));
    }
    out_bytes = o;
    m1 = o; o = reg_align(o + R * NP * sizeof(svs_match_result));
    out_bytes_m1 = o;
  }
};
}  // namespace

struct svs_reg {
  svs_ctx *ctx = nullptr;
  svs_cam cams[SVS_NUM_PYR_LEVELS]{};
  int max_req = 0, max_pts = 0, max_kf = 0, max_obs = 0;
  svs_fast *fast = nullptr;
  int t_lo = 0, ncell[SVS_NUM_PYR_LEVELS] = {0, 0, 0};
  PinnedBuf<uint8_t> h_in, h_out;
  DevBuf<uint8_t> d_in, d_out;
  DevBuf<svs_candidate_point> d_cand;
  DevBuf<uint8_t> d_in_vt;
  DevBuf<double> d_Trel, d_T;          // d_T: [4][max_req][12]
  DevBuf<int32_t> d_cnt;               // [2][max_req]
  DevBuf<svs_pose_opt_stats> d_st;     // [2][max_req]
  DevBuf<uint8_t> d_pyr[SVS_NUM_PYR_LEVELS]; int stride[SVS_NUM_PYR_LEVELS] = {0, 0, 0};
  DevBuf<float> d_disp;
  // svs_reg_commit: the kernel's block (header | edge ids | edge strengths | track point ids | track records) and its pinned twin up to the records; the last
  // registration if it was a map batch
  DevBuf<uint8_t> d_commit; PinnedBuf<uint8_t> h_commit;
  svs_map *batch_map = nullptr; uint64_t batch_serial = 0; int batch_R = 0;
  std::vector<int32_t> batch_query; std::vector<uint8_t> batch_done;
  int timing = 0; owned::Event ev[SVS_REG_STAGES + 1]; float stage_ms[SVS_REG_STAGES] = {0, 0, 0, 0, 0, 0, 0};
  ~svs_reg() {      // (before the members go, also when create gives up)
    if (ctx) { (void)hipSetDevice(ctx->device); (void)hipStreamSynchronize(ctx->stream); }
    if (fast) svs_fast_destroy(fast);
  }
};

extern "C" void svs_reg_params_default(svs_reg_params *p) {
  if (!p) return;
  p->covis_thr = 15; p->search_radius[0] = 10; p->search_radius[1] = 4; p->thr_mean = 22; p->thr_std = 10; p->num_iter[0] = 25; p->num_iter[1] = 15; p->pad_ = 0;
  p->reproj_thr = 2.0; p->kernel_param = 2.0;
}

extern "C" int svs_reg_destroy(svs_reg *reg) {
  if (!reg) return SVS_OK;
  delete reg;
  return SVS_OK;
}

struct CommitLayout { size_t edge_kf, edge_str, ids, track, bytes; };
static CommitLayout commit_layout(int KB, int NP) {
  CommitLayout C;
  C.edge_kf = sizeof(reg_commit_hdr); C.edge_str = C.edge_kf + reg_align((size_t)KB * 4); C.ids = C.edge_str + reg_align((size_t)KB * 4);
  C.track = C.ids + reg_align((size_t)NP * 4); C.bytes = C.track + (size_t)NP * sizeof(svs_map_track_point);
  return C;
}

static int reg_alloc(svs_reg *g) {
  svs_ctx *ctx = g->ctx;
  const size_t R = (size_t)g->max_req;
  RegLayout L;
  L.set(R, (size_t)g->max_kf, (size_t)g->max_pts, (size_t)g->max_obs, (size_t)std::max(g->max_pts, 1), true);
  SVS_HIP(ctx, g->h_in.alloc(L.in_bytes));
  SVS_HIP(ctx, g->d_in.alloc(L.in_bytes));
  SVS_HIP(ctx, g->h_out.alloc(L.out_bytes_m1));
  SVS_HIP(ctx, g->d_out.alloc(L.out_bytes_m1));
  SVS_HIP(ctx, g->d_cand.alloc(R * std::max(g->max_pts, 1)));
  SVS_HIP(ctx, g->d_in_vt.alloc(R * g->max_kf));
  SVS_HIP(ctx, g->d_Trel.alloc(R * g->max_kf * 12));
  SVS_HIP(ctx, g->d_T.alloc(4 * R * 12));
  SVS_HIP(ctx, g->d_cnt.alloc(2 * R));
  SVS_HIP(ctx, g->d_st.alloc(2 * R));
  for (int l = 0; l < SVS_NUM_PYR_LEVELS; ++l) {
    g->stride[l] = (g->cams[l].w + 63) / 64 * 64;
    SVS_HIP(ctx, g->d_pyr[l].alloc(R * g->stride[l] * g->cams[l].h));
  }
  SVS_HIP(ctx, g->d_disp.alloc(R * g->stride[0] * g->cams[0].h));
  for (int i = 0; i <= SVS_REG_STAGES; ++i) SVS_HIP(ctx, g->ev[i].create());
  const CommitLayout CL = commit_layout(g->max_kf, std::max(g->max_pts, 1));
  SVS_HIP(ctx, g->d_commit.alloc(CL.bytes));
  SVS_HIP(ctx, g->h_commit.alloc(CL.track));
  return SVS_OK;
}

extern "C" int svs_reg_create(svs_ctx *ctx, const svs_cam *cam, int max_requests, int max_points, int max_keyframes, int max_observers, svs_reg **out) {
  SVS_REQUIRE(ctx, ctx && cam && out && max_requests >= 1 && max_points >= 0 && max_keyframes >= 1 && max_keyframes <= REG_MAX_KF && max_observers >= 0);
  SVS_REQUIRE(ctx, cam->f > 0.0 && cam->b > 0.0 && cam->w >= 64 && cam->h >= 64 && cam->w <= 16384 && cam->h <= 16384);
  SVS_REQUIRE(ctx, (size_t)max_requests * std::max(max_points, 1) < (1u << 30) && (size_t)max_requests * std::max(max_observers, 1) < (1u << 30));
  SVS_DEVICE(ctx);
  std::unique_ptr<svs_reg> g(new svs_reg());
  g->ctx = ctx;
  g->max_req = max_requests; g->max_pts = max_points; g->max_kf = max_keyframes; g->max_obs = max_observers;
  int32_t w[SVS_NUM_PYR_LEVELS], h[SVS_NUM_PYR_LEVELS];
  svs_fastgrid grids[SVS_NUM_PYR_LEVELS];
  for (int l = 0; l < SVS_NUM_PYR_LEVELS; ++l) {      // cam_vec of FrameGrabber<StereoCamera> (frame_grabber-impl.cpp:48-60)
    const double s = (double)(1 << l);
    g->cams[l] = svs_cam{cam->f / s, cam->cx / s, cam->cy / s, cam->b * (1 << l), (int32_t)(cam->w / s), (int32_t)(cam->h / s)};
    w[l] = g->cams[l].w; h[l] = g->cams[l].h;
    fastgrid_for_level(w[l], h[l], l, &grids[l]);
    g->ncell[l] = grids[l].gx * grids[l].gy;
  }
  if (int rc = svs_fast_create(ctx, SVS_NUM_PYR_LEVELS, w, h, grids, max_requests, 8192, &g->fast)) return rc;
  g->t_lo = svs_fast_thr_view_internal(g->fast).t_lo;
  if (int rc = reg_alloc(g.get())) return rc;
  *out = g.release();
  return SVS_OK;
}

extern "C" int svs_reg_set_timing(svs_reg *reg, int on) {
  if (!reg) return SVS_ERR_INVALID;
  reg->timing = on ? 1 : 0;
  return SVS_OK;
}
extern "C" int svs_reg_stage_times(svs_reg *reg, float *ms) {
  if (!reg || !ms) return SVS_ERR_INVALID;
  for (int i = 0; i < SVS_REG_STAGES; ++i) ms[i] = reg->stage_ms[i];
  return SVS_OK;
}

// the chain of launches behind the staged (or device-built) requests, the download and the wait.  r0 / r1: the root frames of requests 0 and 1 (direct: all
// roots lie at the stride between them and are read in place)
static int reg_chain(svs_reg *g, const svs_reg_params &P, int R, int KB, int SB, int OB, int NP, const RegLayout &L, bool direct, const MapRootView &r0,
                     const MapRootView &r1, bool want_m1) {
  svs_ctx *ctx = g->ctx;
  // ---- the chain
  const size_t MR = (size_t)g->max_req;
  RegK K{};
  uint8_t *di = g->d_in, *dout = g->d_out;
  K.hdr = reinterpret_cast<const reg_hdr *>(di + L.hdr);
  K.kfs = reinterpret_cast<const svs_keyframe *>(di + L.kfs); K.kf_b = (size_t)KB;
  K.flags = di + L.flags;
  K.src = reinterpret_cast<const svs_candidate_point *>(di + L.src); K.src_b = (size_t)SB;
  K.obs_begin = reinterpret_cast<const int32_t *>(di + L.ob); K.ob_b = (size_t)SB + 1;
  K.obs_kf = reinterpret_cast<const int32_t *>(di + L.ok); K.ok_b = (size_t)OB;
  K.cand = g->d_cand; K.cand_b = (size_t)std::max(g->max_pts, 1); K.n_pad = NP;
  K.in_vt = g->d_in_vt; K.Trel = g->d_Trel;
  K.T = g->d_T; K.Tcw = g->d_T + MR * 12; K.Twa = g->d_T + 2 * MR * 12; K.T1 = g->d_T + 3 * MR * 12;
  K.n_cand = g->d_cnt; K.dead = g->d_cnt + MR;
  K.st1 = g->d_st; K.st2 = g->d_st + MR;
  K.fv = svs_fast_thr_view_internal(g->fast);
  for (int l = 0; l < SVS_NUM_PYR_LEVELS; ++l) K.cams[l] = g->cams[l];
  K.covis = P.covis_thr; K.reproj = (float)P.reproj_thr;
  K.res = reinterpret_cast<svs_reg_result *>(dout + L.res);
  svs_match_result *d_m1 = reinterpret_cast<svs_match_result *>(dout + L.m1), *d_m2 = reinterpret_cast<svs_match_result *>(dout + L.m2);
  K.m1 = d_m1; K.m2 = d_m2;
  K.status1 = reinterpret_cast<int32_t *>(dout + L.st1); K.accepted = reinterpret_cast<int32_t *>(dout + L.acc); K.cand_src = reinterpret_cast<int32_t *>(dout + L.csrc);
  K.kfst = reinterpret_cast<svs_reg_kf_stats *>(dout + L.kfst);
  int ev = 0;
  if (g->timing) SVS_HIP(ctx, hipEventRecord(g->ev[ev++], ctx->stream));
  hipLaunchKernelGGL(reg_cull_kernel, dim3(R), dim3(RC_THREADS), 0, ctx->stream, K);
  SVS_LAUNCH_CHECK(ctx);
  svs_match_args A;
  memset(&A, 0, sizeof A);
  const uint8_t *img[SVS_NUM_PYR_LEVELS]; int32_t istride[SVS_NUM_PYR_LEVELS]; size_t ibstride[SVS_NUM_PYR_LEVELS];
  if (direct) {
    for (int l = 0; l < SVS_NUM_PYR_LEVELS; ++l) {
      img[l] = r0.pyr[l]; istride[l] = r0.stride[l];
      ibstride[l] = R > 1 ? (size_t)(r1.pyr[l] - r0.pyr[l]) : 0;
    }
    A.d_disp = r0.disp; A.disp_stride = r0.disp_stride; A.disp_bstride = R > 1 ? (size_t)(r1.disp - r0.disp) : 0;
  } else {
    RegGather G{};
    for (int l = 0; l < SVS_NUM_PYR_LEVELS; ++l) {
      G.pyr[l] = g->d_pyr[l]; G.stride[l] = g->stride[l]; G.bstride[l] = (size_t)g->stride[l] * g->cams[l].h;
      img[l] = G.pyr[l]; istride[l] = G.stride[l]; ibstride[l] = G.bstride[l];
    }
    G.disp = g->d_disp; G.dstride = g->stride[0]; G.d_bstride = (size_t)g->stride[0] * g->cams[0].h;
    A.d_disp = G.disp; A.disp_stride = G.dstride; A.disp_bstride = G.d_bstride;
    hipLaunchKernelGGL(reg_gather_kernel, dim3(std::min(g->cams[0].h, 120), SVS_NUM_PYR_LEVELS + 1, R), dim3(256), 0, ctx->stream, K, G);
    SVS_LAUNCH_CHECK(ctx);
  }
  if (g->timing) SVS_HIP(ctx, hipEventRecord(g->ev[ev++], ctx->stream));
  if (int rc = svs_fast_detect(g->fast, img, istride, ibstride, R, 0)) return rc;
  if (g->timing) SVS_HIP(ctx, hipEventRecord(g->ev[ev++], ctx->stream));
  A.d_kfs = K.kfs; A.n_kf = KB; A.kf_bstride = (size_t)KB;
  A.d_pts = K.cand; A.n_pts = NP; A.pts_bstride = K.cand_b; A.out_bstride = (size_t)NP;
  A.d_T_cur_from_w = K.Tcw; A.d_T_w_from_actkey = K.Twa;
  for (int l = 0; l < SVS_NUM_PYR_LEVELS; ++l) { A.d_cur_pyr[l] = img[l]; A.cur_stride[l] = istride[l]; A.cur_bstride[l] = ibstride[l]; A.cam_vec[l] = g->cams[l]; }
  A.thr_mean = P.thr_mean; A.thr_std = P.thr_std; A.n_batch = R;
  svs_pose_opt_params po;
  svs_pose_opt_params_default(&po);
  po.robust_kernel = 1; po.kernel_param = P.kernel_param; po.min_obs = P.covis_thr;
  // the front end's fused prediction reads its poses from the context: not here
  const double *keep_T = ctx->match_src_T, *keep_Ta = ctx->match_src_Ta;
  ctx->match_src_T = ctx->match_src_Ta = nullptr;
  int rc = SVS_OK;
  for (int pass = 0; pass < 2 && rc == SVS_OK; ++pass) {
    A.search_radius = P.search_radius[pass];
    rc = svs_match(ctx, &A, g->fast, pass == 0 ? d_m1 : d_m2);
    if (rc == SVS_OK && g->timing && hipEventRecord(g->ev[ev++], ctx->stream) != hipSuccess) rc = SVS_ERR_HIP;
    po.num_iter = P.num_iter[pass];
    if (rc == SVS_OK) rc = svs_motion_only(ctx, pass == 0 ? d_m1 : d_m2, NP, (size_t)NP, &g->cams[0], &po, K.T, pass == 0 ? K.st1 : K.st2, R);
    if (rc == SVS_OK && pass == 0) {
      hipLaunchKernelGGL(reg_pose_kernel, dim3(R), dim3(64), 0, ctx->stream, K);
      if (hipGetLastError() != hipSuccess) rc = SVS_ERR_HIP;
    }
    if (rc == SVS_OK && g->timing && hipEventRecord(g->ev[ev++], ctx->stream) != hipSuccess) rc = SVS_ERR_HIP;
  }
  ctx->match_src_T = keep_T; ctx->match_src_Ta = keep_Ta;
  if (rc) { if (rc == SVS_ERR_HIP && ctx->err.empty()) ctx->err = "svs_reg_register_batch: a launch of the chain failed"; return rc; }
  hipLaunchKernelGGL(reg_gate_kernel, dim3(R), dim3(RG_THREADS), (size_t)5 * KB * sizeof(int), ctx->stream, K);
  SVS_LAUNCH_CHECK(ctx);
  if (g->timing) SVS_HIP(ctx, hipEventRecord(g->ev[ev++], ctx->stream));
  const size_t down = want_m1 ? L.out_bytes_m1 : L.out_bytes;
  SVS_HIP(ctx, hipMemcpyAsync(g->h_out, g->d_out, down, hipMemcpyDeviceToHost, ctx->stream));
  SVS_HIP(ctx, hipStreamSynchronize(ctx->stream));
  if (g->timing)
    for (int i = 0; i < SVS_REG_STAGES; ++i) SVS_HIP(ctx, hipEventElapsedTime(&g->stage_ms[i], g->ev[i], g->ev[i + 1]));
  return SVS_OK;
}

extern "C" int svs_reg_register_batch(svs_reg *g, int n_requests, const svs_reg_request *req, const svs_reg_params *prm, svs_reg_result *h_res, int32_t *h_cand_src,
                                      svs_match_result *h_matches, int32_t *h_status_pass1, int32_t *h_accepted, svs_reg_kf_stats *h_kf_stats,
                                      svs_match_result *h_matches_pass1) {
  svs_ctx *ctx = g ? g->ctx : nullptr;
  SVS_REQUIRE(ctx, g && n_requests >= 0 && (n_requests == 0 || req));
  svs_reg_params P;
  if (prm) P = *prm; else svs_reg_params_default(&P);
  SVS_REQUIRE(ctx, P.covis_thr >= 0 && P.search_radius[0] >= 0 && P.search_radius[0] <= 31 && P.search_radius[1] >= 0 && P.search_radius[1] <= 31 && P.num_iter[0] >= 0 &&
                       P.num_iter[1] >= 0 && P.reproj_thr >= 0.0);
  REG_CAPACITY(ctx, n_requests <= g->max_req);
  int KB = 1, SB = 0, OB = 0;
  for (int r = 0; r < n_requests; ++r) {
    const svs_reg_request &q = req[r];
    SVS_REQUIRE(ctx, (q.mode == SVS_REG_LOCAL || q.mode == SVS_REG_LOOP) && q.n_kf >= 1 && q.n_src >= 0 && q.h_kfs && q.h_kf_flags && (q.n_src == 0 || q.h_src));
    REG_CAPACITY(ctx, q.n_kf <= g->max_kf);
    REG_CAPACITY(ctx, q.n_src <= g->max_pts);
    SVS_REQUIRE(ctx, q.root_kf >= 0 && q.root_kf < q.n_kf && q.d_root_disp && q.root_disp_stride >= g->cams[0].w);
    for (int l = 0; l < SVS_NUM_PYR_LEVELS; ++l) {
      SVS_REQUIRE(ctx, q.h_kfs[q.root_kf].pyr[l] && q.h_kfs[q.root_kf].stride[l] >= g->cams[l].w);
      for (int c = 0; c < g->ncell[l]; ++c) SVS_REQUIRE(ctx, q.fast_thr[l][c] >= g->t_lo && q.fast_thr[l][c] <= 255);
    }
    int n_obs = 0;
    if (q.mode == SVS_REG_LOCAL && q.n_src > 0) {
      SVS_REQUIRE(ctx, q.h_obs_begin && q.h_obs_begin[0] == 0);
      for (int i = 0; i < q.n_src; ++i) SVS_REQUIRE(ctx, q.h_obs_begin[i + 1] >= q.h_obs_begin[i]);
      n_obs = q.h_obs_begin[q.n_src];
      SVS_REQUIRE(ctx, n_obs == 0 || q.h_obs_kf);
      REG_CAPACITY(ctx, n_obs <= g->max_obs);
    }
    KB = std::max(KB, q.n_kf); SB = std::max(SB, q.n_src); OB = std::max(OB, n_obs);
  }
  if (n_requests == 0) return SVS_OK;
  SVS_DEVICE(ctx);
  g->batch_map = nullptr;              // (svs_reg_commit: the handle's last registration is no map batch)
  const int R = n_requests, NP = std::max(SB, 1);
  RegLayout L;
  L.set((size_t)R, (size_t)KB, (size_t)SB, (size_t)OB, (size_t)NP);
  // ---- stage the requests
  uint8_t *hi = g->h_in;
  memset(hi, 0, L.in_bytes);
  bool direct = true;      // the root frames lie at one stride from the first: FAST and the matcher read them in place
  const svs_keyframe &root0 = req[0].h_kfs[req[0].root_kf];
  for (int r = 0; r < R; ++r) {
    const svs_reg_request &q = req[r];
    reg_hdr *hd = reinterpret_cast<reg_hdr *>(hi + L.hdr) + r;
    hd->mode = q.mode; hd->n_kf = q.n_kf; hd->n_src = q.n_src; hd->root_kf = q.root_kf; hd->disp = q.d_root_disp; hd->disp_stride = q.root_disp_stride;
    memcpy(hd->T_root, q.T_root_from_world, sizeof hd->T_root);
    memcpy(hd->thr, q.fast_thr, sizeof hd->thr);
    memcpy(hi + L.kfs + ((size_t)r * KB) * sizeof(svs_keyframe), q.h_kfs, (size_t)q.n_kf * sizeof(svs_keyframe));
    memcpy(hi + L.flags + (size_t)r * KB, q.h_kf_flags, (size_t)q.n_kf);
    if (q.n_src) memcpy(hi + L.src + ((size_t)r * SB) * sizeof(svs_candidate_point), q.h_src, (size_t)q.n_src * sizeof(svs_candidate_point));
    if (q.mode == SVS_REG_LOCAL && q.n_src > 0) {
      memcpy(hi + L.ob + ((size_t)r * (SB + 1)) * sizeof(int32_t), q.h_obs_begin, (size_t)(q.n_src + 1) * sizeof(int32_t));
      const int n_obs = q.h_obs_begin[q.n_src];
      if (n_obs) memcpy(hi + L.ok + ((size_t)r * OB) * sizeof(int32_t), q.h_obs_kf, (size_t)n_obs * sizeof(int32_t));
    }
    const svs_keyframe &root = q.h_kfs[q.root_kf];
    for (int l = 0; l < SVS_NUM_PYR_LEVELS && r > 0; ++l) {
      const svs_keyframe &root1 = req[1].h_kfs[req[1].root_kf];
      direct = direct && root.stride[l] == root0.stride[l] && root1.pyr[l] >= root0.pyr[l] && root.pyr[l] == root0.pyr[l] + (size_t)r * (size_t)(root1.pyr[l] - root0.pyr[l]);
    }
    if (r > 0) {
      direct = direct && q.root_disp_stride == req[0].root_disp_stride && req[1].d_root_disp >= req[0].d_root_disp &&
               q.d_root_disp == req[0].d_root_disp + (size_t)r * (size_t)(req[1].d_root_disp - req[0].d_root_disp);
    }
  }
  SVS_HIP(ctx, hipMemcpyAsync(g->d_in, g->h_in, L.in_bytes, hipMemcpyHostToDevice, ctx->stream));
  MapRootView rv[2];
  for (int k = 0; k < 2; ++k) {
    const svs_reg_request &q = req[std::min(k, R - 1)];
    for (int l = 0; l < SVS_NUM_PYR_LEVELS; ++l) { rv[k].pyr[l] = q.h_kfs[q.root_kf].pyr[l]; rv[k].stride[l] = q.h_kfs[q.root_kf].stride[l]; }
    rv[k].disp = q.d_root_disp; rv[k].disp_stride = q.root_disp_stride;
  }
  if (int rc = reg_chain(g, P, R, KB, SB, OB, NP, L, direct, rv[0], rv[1], h_matches_pass1 != nullptr)) return rc;
  // ---- hand the rows out: max_points / max_keyframes long, defaults behind a request's own entries
  const uint8_t *ho = g->h_out;
  const size_t MP = (size_t)g->max_pts, MK = (size_t)g->max_kf;
  svs_match_result none;
  memset(&none, 0, sizeof none);
  none.status = SVS_MATCH_NO_ANCHOR;
  for (int r = 0; r < R; ++r) {
    const svs_reg_result *rs = reinterpret_cast<const svs_reg_result *>(ho + L.res) + r;
    const size_t n = (size_t)std::min(std::max(rs->n_candidates, 0), SB);
    if (h_res) h_res[r] = *rs;
    if (h_matches) { memcpy(h_matches + r * MP, ho + L.m2 + (size_t)r * NP * sizeof(svs_match_result), n * sizeof(svs_match_result)); std::fill(h_matches + r * MP + n, h_matches + (r + 1) * MP, none); }
    if (h_matches_pass1) { memcpy(h_matches_pass1 + r * MP, ho + L.m1 + (size_t)r * NP * sizeof(svs_match_result), n * sizeof(svs_match_result)); std::fill(h_matches_pass1 + r * MP + n, h_matches_pass1 + (r + 1) * MP, none); }
    if (h_status_pass1) { memcpy(h_status_pass1 + r * MP, ho + L.st1 + (size_t)r * NP * 4, n * 4); std::fill(h_status_pass1 + r * MP + n, h_status_pass1 + (r + 1) * MP, (int32_t)SVS_MATCH_NO_ANCHOR); }
    if (h_accepted) { memcpy(h_accepted + r * MP, ho + L.acc + (size_t)r * NP * 4, n * 4); std::fill(h_accepted + r * MP + n, h_accepted + (r + 1) * MP, 0); }
    if (h_cand_src) { memcpy(h_cand_src + r * MP, ho + L.csrc + (size_t)r * NP * 4, n * 4); std::fill(h_cand_src + r * MP + n, h_cand_src + (r + 1) * MP, -1); }
    if (h_kf_stats) {
      const size_t nk = (size_t)req[r].n_kf;
      memcpy(h_kf_stats + r * MK, ho + L.kfst + (size_t)r * KB * sizeof(svs_reg_kf_stats), nk * sizeof(svs_reg_kf_stats));
      memset(h_kf_stats + r * MK + nk, 0, (MK - nk) * sizeof(svs_reg_kf_stats));
    }
  }
  return SVS_OK;
}

// ---- requests by ids against a device-resident map (map.hip: map_request.inc): the staged bytes are the id lists, the map's walk builds the tables where the stateless call stages
// them -- at the handle's capacities, since the sizes are only known on the device; a request's outputs do not depend on the padding -- and the chain above runs
extern "C" int svs_reg_register_map_batch(svs_reg *g, svs_map *map, int n_requests, const svs_reg_map_request *req, const svs_reg_params *prm, svs_reg_result *h_res,
                                          int32_t *h_cand_src, svs_match_result *h_matches, int32_t *h_status_pass1, int32_t *h_accepted,
                                          svs_reg_kf_stats *h_kf_stats, svs_match_result *h_matches_pass1, int32_t *h_cand_point_id, int32_t *h_kf_ids,
                                          int32_t *h_n_kf) {
  svs_ctx *ctx = g ? g->ctx : nullptr;
  SVS_REQUIRE(ctx, g && map && svs_map_ctx(map) == ctx && n_requests >= 0 && (n_requests == 0 || req));
  svs_reg_params P;
  if (prm) P = *prm; else svs_reg_params_default(&P);
  SVS_REQUIRE(ctx, P.covis_thr >= 0 && P.search_radius[0] >= 0 && P.search_radius[0] <= 31 && P.search_radius[1] >= 0 && P.search_radius[1] <= 31 && P.num_iter[0] >= 0 &&
                       P.num_iter[1] >= 0 && P.reproj_thr >= 0.0);
  REG_CAPACITY(ctx, n_requests <= g->max_req);
  const int R = n_requests, KB = g->max_kf, SB = g->max_pts, OB = g->max_obs, NP = std::max(SB, 1);
  MapRootView rv[2], v;
  bool direct = true;
  for (int r = 0; r < R; ++r) {
    const svs_reg_map_request &q = req[r];
    SVS_REQUIRE(ctx, (q.mode == SVS_REG_LOCAL || q.mode == SVS_REG_LOOP) && q.n_walk >= (q.mode == SVS_REG_LOOP ? 1 : 0) && q.n_direct >= 0 &&
                         (q.n_walk == 0 || q.h_walk_kf) && (q.n_direct == 0 || q.h_direct_kf));
    REG_CAPACITY(ctx, q.n_walk <= KB);
    REG_CAPACITY(ctx, q.n_direct <= KB);
    SVS_REQUIRE(ctx, svs_map_has_keyframe(map, q.root_kf));
    for (int i = 0; i < q.n_walk; ++i) SVS_REQUIRE(ctx, svs_map_has_keyframe(map, q.h_walk_kf[i]));
    for (int i = 0; i < q.n_direct; ++i) SVS_REQUIRE(ctx, svs_map_has_keyframe(map, q.h_direct_kf[i]));
    svs_map_root_view(map, q.root_kf, &v);
    SVS_REQUIRE(ctx, v.disp_stride >= g->cams[0].w);
    for (int l = 0; l < SVS_NUM_PYR_LEVELS; ++l) SVS_REQUIRE(ctx, v.stride[l] >= g->cams[l].w);
    if (r < 2) rv[r] = v;
    if (r == 0) rv[1] = v;
    if (r > 0) {      // the roots lie at one stride from the first: FAST and the matcher read them in place
      for (int l = 0; l < SVS_NUM_PYR_LEVELS; ++l)
        direct = direct && v.stride[l] == rv[0].stride[l] && rv[1].pyr[l] >= rv[0].pyr[l] && v.pyr[l] == rv[0].pyr[l] + (size_t)r * (size_t)(rv[1].pyr[l] - rv[0].pyr[l]);
      direct = direct && v.disp_stride == rv[0].disp_stride && rv[1].disp >= rv[0].disp && v.disp == rv[0].disp + (size_t)r * (size_t)(rv[1].disp - rv[0].disp);
    }
  }
  if (R == 0) return SVS_OK;
  SVS_DEVICE(ctx);
  g->batch_map = nullptr;              // the previous batch ends here; this one can be committed once it has run
  RegLayout L;
  L.set((size_t)R, (size_t)KB, (size_t)SB, (size_t)OB, (size_t)NP, true);
  // ---- stage the ids
  uint8_t *hi = g->h_in;
  map_req *mq = reinterpret_cast<map_req *>(hi + L.mreq);
  int32_t *ids = reinterpret_cast<int32_t *>(hi + L.mids);
  int n_ids = 0;
  for (int r = 0; r < R; ++r) {
    const svs_reg_map_request &q = req[r];
    memset(&mq[r], 0, sizeof mq[r]);
    mq[r].mode = q.mode; mq[r].root = q.root_kf; mq[r].n_walk = q.n_walk; mq[r].n_direct = q.n_direct;
    mq[r].walk_off = n_ids;
    if (q.n_walk) memcpy(ids + n_ids, q.h_walk_kf, (size_t)q.n_walk * sizeof(int32_t));
    n_ids += q.n_walk;
    mq[r].direct_off = n_ids;
    if (q.n_direct) memcpy(ids + n_ids, q.h_direct_kf, (size_t)q.n_direct * sizeof(int32_t));
    n_ids += q.n_direct;
    memcpy(mq[r].T_root, q.T_root_from_world, sizeof mq[r].T_root);
  }
  const size_t up_bytes = L.mids + (size_t)n_ids * sizeof(int32_t) - L.mreq;
  uint8_t *di = g->d_in, *dout = g->d_out;
  SVS_HIP(ctx, hipMemcpyAsync(di + L.mreq, hi + L.mreq, up_bytes, hipMemcpyHostToDevice, ctx->stream));
  // ---- the walk builds the requests
  MapBuildDst D{};
  D.req = reinterpret_cast<const map_req *>(di + L.mreq); D.ids = reinterpret_cast<const int32_t *>(di + L.mids);
  D.hdr = reinterpret_cast<reg_hdr *>(di + L.hdr); D.kfs = reinterpret_cast<svs_keyframe *>(di + L.kfs); D.flags = di + L.flags;
  D.src = reinterpret_cast<svs_candidate_point *>(di + L.src); D.obs_begin = reinterpret_cast<int32_t *>(di + L.ob); D.obs_kf = reinterpret_cast<int32_t *>(di + L.ok);
  D.KB = KB; D.SB = SB; D.OB = OB; D.NP = NP;
  D.point_id = reinterpret_cast<int32_t *>(dout + L.pid); D.kf_id = reinterpret_cast<int32_t *>(dout + L.kfid); D.meta = reinterpret_cast<int4 *>(dout + L.meta);
  if (int rc = svs_map_build_requests(map, R, D)) return rc;
  if (int rc = reg_chain(g, P, R, KB, SB, OB, NP, L, direct, rv[0], rv[1], h_matches_pass1 != nullptr)) return rc;
  // ---- hand the rows out
  const uint8_t *ho = g->h_out;
  const size_t MP = (size_t)g->max_pts, MK = (size_t)g->max_kf;
  svs_match_result none;
  memset(&none, 0, sizeof none);
  none.status = SVS_MATCH_NO_ANCHOR;
  for (int r = 0; r < R; ++r) {
    const svs_reg_result *rs = reinterpret_cast<const svs_reg_result *>(ho + L.res) + r;
    const int4 meta = reinterpret_cast<const int4 *>(ho + L.meta)[r];
    if (meta.w) {      // over capacity: the status and zeros
      if (h_res) { memset(&h_res[r], 0, sizeof h_res[r]); h_res[r].status = SVS_REG_OVER_CAPACITY; }
      if (h_matches) memset(h_matches + r * MP, 0, MP * sizeof(svs_match_result));
      if (h_matches_pass1) memset(h_matches_pass1 + r * MP, 0, MP * sizeof(svs_match_result));
      if (h_status_pass1) memset(h_status_pass1 + r * MP, 0, MP * 4);
      if (h_accepted) memset(h_accepted + r * MP, 0, MP * 4);
      if (h_cand_src) memset(h_cand_src + r * MP, 0, MP * 4);
      if (h_cand_point_id) memset(h_cand_point_id + r * MP, 0, MP * 4);
      if (h_kf_stats) memset(h_kf_stats + r * MK, 0, MK * sizeof(svs_reg_kf_stats));
      if (h_kf_ids) memset(h_kf_ids + r * MK, 0, MK * 4);
      if (h_n_kf) h_n_kf[r] = 0;
      continue;
    }
    const size_t n = (size_t)std::min(std::max(rs->n_candidates, 0), SB), nk = (size_t)std::min(std::max(meta.x, 1), KB);
    if (h_res) h_res[r] = *rs;
    if (h_matches) { memcpy(h_matches + r * MP, ho + L.m2 + (size_t)r * NP * sizeof(svs_match_result), n * sizeof(svs_match_result)); std::fill(h_matches + r * MP + n, h_matches + (r + 1) * MP, none); }
    if (h_matches_pass1) { memcpy(h_matches_pass1 + r * MP, ho + L.m1 + (size_t)r * NP * sizeof(svs_match_result), n * sizeof(svs_match_result)); std::fill(h_matches_pass1 + r * MP + n, h_matches_pass1 + (r + 1) * MP, none); }
    if (h_status_pass1) { memcpy(h_status_pass1 + r * MP, ho + L.st1 + (size_t)r * NP * 4, n * 4); std::fill(h_status_pass1 + r * MP + n, h_status_pass1 + (r + 1) * MP, (int32_t)SVS_MATCH_NO_ANCHOR); }
    if (h_accepted) { memcpy(h_accepted + r * MP, ho + L.acc + (size_t)r * NP * 4, n * 4); std::fill(h_accepted + r * MP + n, h_accepted + (r + 1) * MP, 0); }
    if (h_cand_src) { memcpy(h_cand_src + r * MP, ho + L.csrc + (size_t)r * NP * 4, n * 4); std::fill(h_cand_src + r * MP + n, h_cand_src + (r + 1) * MP, -1); }
    if (h_cand_point_id) {      // the candidates' ids: the built list read through the cull's indices
      const int32_t *csrc = reinterpret_cast<const int32_t *>(ho + L.csrc) + (size_t)r * NP, *pid = reinterpret_cast<const int32_t *>(ho + L.pid) + (size_t)r * NP;
      for (size_t i = 0; i < n; ++i) h_cand_point_id[r * MP + i] = (unsigned)csrc[i] < (unsigned)SB ? pid[csrc[i]] : -1;
      std::fill(h_cand_point_id + r * MP + n, h_cand_point_id + (r + 1) * MP, -1);
    }
    if (h_kf_stats) {
      memcpy(h_kf_stats + r * MK, ho + L.kfst + (size_t)r * KB * sizeof(svs_reg_kf_stats), nk * sizeof(svs_reg_kf_stats));
      memset(h_kf_stats + r * MK + nk, 0, (MK - nk) * sizeof(svs_reg_kf_stats));
    }
    if (h_kf_ids) { memcpy(h_kf_ids + r * MK, ho + L.kfid + (size_t)r * KB * 4, nk * 4); std::fill(h_kf_ids + r * MK + nk, h_kf_ids + (r + 1) * MK, -1); }
    if (h_n_kf) h_n_kf[r] = (int32_t)nk;
  }
  g->batch_query.assign((size_t)R, -1);
  for (int r = 0; r < R; ++r) if (req[r].mode == SVS_REG_LOOP) g->batch_query[(size_t)r] = req[r].h_walk_kf[0];
  g->batch_done.assign((size_t)R, 0);
  g->batch_map = map; g->batch_serial = svs_map_serial(map); g->batch_R = R;
  return SVS_OK;
}

// ---- registerKeyframes / addLoopClosure for one request of that batch: reg_commit_kernel leaves the track list and the edge list on the device, the map applies them
extern "C" int svs_reg_commit(svs_reg *g, svs_map *map, int request_index, int n_cached, const int32_t *h_cached_ids, const double *h_cached_T, int missing_cap,
                              svs_reg_commit_result *h_res, int32_t *h_edge_kf, int32_t *h_edge_strength, svs_map_constraint_result *h_cons, int32_t *h_missing,
                              int track_cap, int32_t *h_track_point_ids, int32_t *h_track_added) {
  svs_ctx *ctx = g ? g->ctx : nullptr;
  SVS_REQUIRE(ctx, g && map && svs_map_ctx(map) == ctx && h_res && h_cons && missing_cap >= 0 && (missing_cap == 0 || h_missing) && track_cap >= 0);
  SVS_REQUIRE(ctx, g->batch_map == map && g->batch_serial == svs_map_serial(map));      // the last registration was a map batch on this map
  SVS_REQUIRE(ctx, request_index >= 0 && request_index < g->batch_R && !g->batch_done[(size_t)request_index]);
  SVS_DEVICE(ctx);
  const int r = request_index, KB = g->max_kf, SB = g->max_pts, OB = g->max_obs, NP = std::max(SB, 1);
  RegLayout L;
  L.set((size_t)g->batch_R, (size_t)KB, (size_t)SB, (size_t)OB, (size_t)NP, true);
  const CommitLayout CL = commit_layout(KB, NP);
  const uint8_t *di = g->d_in, *dout = g->d_out;
  uint8_t *dc = g->d_commit;
  RegCommitK K{};
  K.r = r; K.KB = KB; K.SB = SB; K.OB = OB; K.NP = NP; K.cand_b = (size_t)NP;
  K.hdr = reinterpret_cast<const reg_hdr *>(di + L.hdr); K.res = reinterpret_cast<const svs_reg_result *>(dout + L.res);
  K.m2 = reinterpret_cast<const svs_match_result *>(dout + L.m2); K.accepted = reinterpret_cast<const int32_t *>(dout + L.acc);
  K.cand_src = reinterpret_cast<const int32_t *>(dout + L.csrc); K.obs_begin = reinterpret_cast<const int32_t *>(di + L.ob);
  K.obs_kf = reinterpret_cast<const int32_t *>(di + L.ok); K.pid = reinterpret_cast<const int32_t *>(dout + L.pid); K.kfid = reinterpret_cast<const int32_t *>(dout + L.kfid);
  K.kfst = reinterpret_cast<const svs_reg_kf_stats *>(dout + L.kfst); K.cand = g->d_cand;
  K.query = g->batch_query[(size_t)r];
  K.out = reinterpret_cast<reg_commit_hdr *>(dc); K.edge_kf = reinterpret_cast<int32_t *>(dc + CL.edge_kf); K.edge_str = reinterpret_cast<int32_t *>(dc + CL.edge_str);
  K.ids = reinterpret_cast<int32_t *>(dc + CL.ids); K.track = reinterpret_cast<svs_map_track_point *>(dc + CL.track);
  hipLaunchKernelGGL(reg_commit_kernel, dim3(1), dim3(CM_THREADS), 0, ctx->stream, K);
  SVS_LAUNCH_CHECK(ctx);
  SVS_HIP(ctx, hipMemcpyAsync(g->h_commit, g->d_commit, CL.track, hipMemcpyDeviceToHost, ctx->stream));      // the counts, the edge list, the track point ids
  SVS_HIP(ctx, hipStreamSynchronize(ctx->stream));
  const uint8_t *hc = g->h_commit;
  const reg_commit_hdr H = *reinterpret_cast<const reg_commit_hdr *>(hc);
  const int32_t *ekf = reinterpret_cast<const int32_t *>(hc + CL.edge_kf), *est = reinterpret_cast<const int32_t *>(hc + CL.edge_str), *ids = reinterpret_cast<const int32_t *>(hc + CL.ids);
  const bool meta_over = H.status == SVS_REG_OK && (H.n_track < 0 || H.n_track > NP || H.n_edges < 0 || H.n_edges > KB);
  SVS_REQUIRE(ctx, !meta_over);
  svs_reg_commit_result out;
  memset(&out, 0, sizeof out);
  out.mode = H.mode; out.root_id = reinterpret_cast<const map_req *>(g->h_in.get() + L.mreq)[r].root; out.other_id = H.mode == SVS_REG_LOOP ? g->batch_query[(size_t)r] : -1;
  out.status = H.status;
  const bool lists = h_track_point_ids || h_track_added;
  if (H.status == SVS_REG_OK) {
    REG_CAPACITY(ctx, !lists || track_cap >= H.n_track);
    MapCommit c{};
    c.pair_kf = out.root_id; memcpy(c.T_new, H.T_new, sizeof c.T_new);
    c.n_track = H.n_track; c.d_track = K.track; c.h_track_ids = ids;
    c.n_edges = H.n_edges; c.h_edge_kf = ekf; c.h_edge_strength = est;
    c.edge_type = H.mode == SVS_REG_LOOP ? 2 : 1; c.other_first = H.mode != SVS_REG_LOOP;
    c.n_cached = n_cached; c.h_cached_ids = h_cached_ids; c.h_cached_T = h_cached_T; c.missing_cap = missing_cap;
    c.h_cons = h_cons; c.h_missing = h_missing;
    std::vector<int32_t> added((size_t)H.n_track, 0);
    c.h_track_added = added.data();
    if (int rc = svs_map_apply_commit(map, &c)) return rc;
    g->batch_done[(size_t)r] = 1;
    out.committed = 1; out.n_track = H.n_track; out.n_pairs_added = c.n_pairs_added; out.n_edges = H.n_edges;
    memcpy(out.T_new, H.T_new, sizeof out.T_new);
    for (int i = 0; i < track_cap; ++i) {
      if (h_track_point_ids) h_track_point_ids[i] = i < H.n_track ? ids[i] : -1;
      if (h_track_added) h_track_added[i] = i < H.n_track ? added[(size_t)i] : 0;
    }
  } else {
    for (int i = 0; i < track_cap; ++i) {
      if (h_track_point_ids) h_track_point_ids[i] = -1;
      if (h_track_added) h_track_added[i] = 0;
    }
  }
  for (int e = 0; e < KB; ++e) {
    if (h_edge_kf) h_edge_kf[e] = e < out.n_edges ? ekf[e] : -1;
    if (h_edge_strength) h_edge_strength[e] = e < out.n_edges ? est[e] : 0;
  }
  *h_res = out;
  return SVS_OK;
}
