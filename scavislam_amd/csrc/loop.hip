// loop.hip -- the numeric step between "place recognition names a candidate keyframe" and "the back end gets T_query_from_loop":
// PlaceRecognizer::geometricCheck (placerecognizer.cpp:175-202) =
//   cv::BFMatcher(NORM_L2).match          a nearest train descriptor for every query descriptor
//   RanSaC<SE3Model>::compute(100, ...)   three-point absolute-orientation hypotheses scored by stereo reprojection (ransac.cpp:28-137,
//                                         ransac_models.cpp:27-81,138-181, stereo_camera.cpp:36-52)
// for a batch of (query place, train place) pairs in TWO launches: loop_match_kernel (f32-input MFMA distances + per-query argmin) and
// loop_ransac_kernel (draw, fit, score, select, final pass: one workgroup per check).  A check's outputs are a function of that check alone.
// Not pinned by the reference's binaries: the yardstick is the NumPy restatement tests/loop_model.py.
// Further down, the front half of PlaceRecognizer::addLocation (placerecognizer.cpp:248-318) -- a visual word per descriptor, the inverted index, TF-IDF place
// scores, the candidate test -- for a batch of places in SIX launches (svs_loop_add_locations; yardstick tests/place_model.py).
#include "common.h"
#include "loop_words.h"
#include <math.h>
#include <string.h>
#include <algorithm>

constexpr int LOOP_MAX_HYP = 256;
constexpr int LOOP_MAX_DRAWS = 64;      // draws per hypothesis before it is given up (the reference loops forever)
// (the tile shape LM_QROWS x LM_TROWS x LM_KC of the distance walks: loop_words.h)
constexpr int LR_THREADS = 512;
constexpr double LOOP_JTOL = 8.881784197001252e-16;      // 2^-50: columns count as orthogonal when |p.q| <= this * |p| |q|

// one check as the kernels read it, followed by its [max_hyp][3] caller triples
struct loop_check_dev {
  int32_t q_slot, t_slot, n_hyp, has_samples;
  double pixel_thr;
  uint64_t seed;
  int32_t nq, nt;
};
// byte offsets inside a check's output block
struct loop_out_layout { int tidx, dist, smp, hinl, inl; size_t stride; };
struct loop_cam { double f, cx, cy, b; };
// one location as the index kernels read it, followed by its [max_places] bytes "slot o may receive a term" (a location before this one, not excluded, not itself)
struct loop_loc_dev { int32_t slot, n, do_detect, n_loc; float radius, pad_[3]; };
// what the kernels leave at the head of a location's output block
struct loop_loc_out { unsigned long long best_key; int32_t n_scored, number_of_words; };
struct loop_index_layout { int word, d2, score; size_t stride; };

struct svs_loop {
  svs_ctx *ctx = nullptr;
  loop_cam cam{};
  int K = 0, max_desc = 0, max_places = 0, max_hyp = 0, max_checks = 0;
  DevBuf<float> d_desc, d_norm;                    // [max_places][max_desc][K], [max_places][max_desc] squared norms
  DevBuf<double> d_uvu, d_xyz;                     // [max_places][max_desc][3]
  std::unique_ptr<int[]> n_place;                  // host: descriptors per slot, 0 = empty
  PinnedBuf<uint8_t> h_stage;                      // pinned: one place on its way up
  owned::Event ev_stage; bool stage_busy = false;
  size_t in_stride = 0; loop_out_layout lay{};
  PinnedBuf<uint8_t> h_in, h_out; DevBuf<uint8_t> d_in, d_out;      // pinned / device: the checks, the results
  int timing = 0; owned::Event ev[3]; float stage_ms[2] = {0.f, 0.f};
  // the place index (svs_loop_set_vocabulary / svs_loop_add_locations): a dense inverted index, word-major with the places contiguous
  int n_words = 0, n_loc = 0;
  std::unique_ptr<uint8_t[]> is_loc;               // host: the slot is a location
  DevBuf<float> d_words, d_wnorm;                  // [n_words][K], [n_words]
  DevBuf<int32_t> d_cnt, d_df, d_nw;               // [n_words][max_places], [n_words], [max_places]
  DevBuf<unsigned long long> d_wkey;               // [max_checks][max_desc]: the running minimum of (bits(d2) << 32) | word
  DevBuf<int32_t> d_first, d_nwk;                  // [max_checks][n_words]: first descriptor of the location with the word; [max_checks]: its number_of_words
  DevBuf<float> d_idf;                             // [max_checks][max_desc]: idf as descriptor r meets it; < 0: no scoring step
  size_t ix_in_stride = 0; loop_index_layout ixl{};
  PinnedBuf<uint8_t> h_ix_in, h_ix_out; DevBuf<uint8_t> d_ix_in, d_ix_out;
  float index_ms[2] = {0.f, 0.f};
  ~svs_loop() { if (ctx) { (void)hipSetDevice(ctx->device); (void)hipStreamSynchronize(ctx->stream); } }      // (before the members go, also when create gives up)
};

#define LOOP_CAPACITY(ctx, cond)                                                                          \
  do {                                                                                                    \
    if (!(cond)) {                                                                                        \
      char buf_[512];                                                                                     \
      snprintf(buf_, sizeof buf_, "%s:%d capacity exceeded: %s", __FILE__, __LINE__, #cond);              \
      (ctx)->err = buf_;                                                                                  \
      return SVS_ERR_CAPACITY;                                                                            \
    }                                                                                                     \
  } while (0)

static size_t loop_align16(size_t v) { return (v + 15) & ~(size_t)15; }

// ---- svs_loop_set_place: squared norms (f64 sum of the exact f32 squares, rounded once) and xyz = cam.unmap_uvu(uvu) ---------------------------------
// unmap_uvu as written in stereo_camera.cpp:46-52 with LinearCamera::unmap(uv) = (uv - c) / f; no contraction: bit for bit tests/loop_model.py
__device__ __forceinline__ void loop_unmap_uvu(const loop_cam &cam, double u0, double u1, double u2, double &x, double &y, double &z) {
  const double scaled_disparity = (u0 - u2) / cam.b;
  z = cam.f / scaled_disparity;
  x = ((u0 - cam.cx) / cam.f) * z;
  y = ((u1 - cam.cy) / cam.f) * z;
}
__global__ __launch_bounds__(256) void loop_place_kernel(const float *__restrict__ desc, int K, int n, float *__restrict__ norm, const double *__restrict__ uvu,
                                                        double *__restrict__ xyz, int make_xyz, loop_cam cam) {
  const int i = (int)(blockIdx.x * 256u + threadIdx.x);
  if (i >= n) return;
  norm[i] = loop_sqnorm(desc + (size_t)i * K, K);
  if (make_xyz) {
    double x, y, z;
    loop_unmap_uvu(cam, uvu[3 * i], uvu[3 * i + 1], uvu[3 * i + 2], x, y, z);
    xyz[3 * i] = x; xyz[3 * i + 1] = y; xyz[3 * i + 2] = z;
  }
}

// ---- the distance stage -------------------------------------------------------------------------------------------------------------------------------
// grid = (query blocks of 32, checks), 4 waves.  d2(q, t) = (|q|^2 + |t|^2) - 2 q.t, the dot product by v_mfma_f32_32x32x2_f32 with the TRAIN rows as
// the A operand and the QUERY rows as B: a lane then holds ONE query (column lane & 31) against 16 train rows per tile (its accumulator registers), so the
// running minimum is private to the lane.  The query fragment stays in registers for the whole walk; train tiles of 128 rows x 64 columns go through LDS
// (16-byte loads and stores, rows past the place zero-filled and never read), wave w takes rows 32 w .. 32 w + 31 of the tile.  A lane of half h = lane >> 5
// feeds columns 8 s + 4 h + e to MFMA number 4 s + e: any assignment works as long as A and B agree, and this one makes every fragment one 16-byte read.
// The minimum is taken on the key (f32 bits of d2 << 32) | train index -- d2 is clamped at 0, so the bits order like the values: the lowest index wins an
// exact tie whatever the order of evaluation.  No atomics: the two lane halves meet in a shuffle, the four waves in LDS.
template <int K>
__global__ __launch_bounds__(256) void loop_match_kernel(const float *__restrict__ desc, const float *__restrict__ norm, size_t place_rows,
                                                        const uint8_t *__restrict__ in, size_t in_stride, uint8_t *__restrict__ out, loop_out_layout lay) {
  __shared__ float4 s_tile[LM_TROWS * LM_LD4];
  __shared__ float s_tnorm[LM_TROWS];
  __shared__ unsigned long long s_best[4][LM_QROWS];
  const loop_check_dev *ck = reinterpret_cast<const loop_check_dev *>(in + (size_t)blockIdx.y * in_stride);
  const int nq = ck->nq, nt = ck->nt, q0 = (int)blockIdx.x * LM_QROWS;
  if (q0 >= nq) return;                                                    // (the grid is sized for the longest query place of the batch)
  const float *Q = desc + (size_t)ck->q_slot * place_rows * K, *T = desc + (size_t)ck->t_slot * place_rows * K;
  const float *Qn = norm + (size_t)ck->q_slot * place_rows, *Tn = norm + (size_t)ck->t_slot * place_rows;
  const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 31, hh = lane >> 5;
  const bool qok = q0 + r < nq;
  float4 qf[K / 8];
#pragma unroll
  for (int s = 0; s < K / 8; ++s)
    qf[s] = qok ? *reinterpret_cast<const float4 *>(Q + (size_t)(q0 + r) * K + 8 * s + 4 * hh) : make_float4(0.f, 0.f, 0.f, 0.f);
  const float qn = qok ? Qn[q0 + r] : 0.f;
  unsigned long long best = ~0ull;
  for (int t0 = 0; t0 < nt; t0 += LM_TROWS) {
    const bool mine = t0 + wave * 32 < nt;                                 // wave-uniform: this wave's 32 rows hold at least one train row
    f32x16 acc;
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[e] = 0.f;
#pragma unroll
    for (int kc = 0; kc < K / LM_KC; ++kc) {
      __syncthreads();                                                     // the previous tile has been read
#pragma unroll
      for (int i = tid; i < LM_TROWS * (LM_KC / 4); i += 256) {
        const int row = i >> 4, c4 = i & 15;
        s_tile[row * LM_LD4 + c4] = t0 + row < nt ? *reinterpret_cast<const float4 *>(T + (size_t)(t0 + row) * K + kc * LM_KC + 4 * c4)
                                                  : make_float4(0.f, 0.f, 0.f, 0.f);
      }
      if (kc == 0 && tid < LM_TROWS) s_tnorm[tid] = t0 + tid < nt ? Tn[t0 + tid] : 0.f;
      __syncthreads();
      if (mine) {
#pragma unroll
        for (int s = 0; s < LM_KC / 8; ++s) {
          const float4 a = s_tile[(wave * 32 + r) * LM_LD4 + 2 * s + hh], b = qf[kc * (LM_KC / 8) + s];
          acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, b.x, acc, 0, 0, 0);
          acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, b.y, acc, 0, 0, 0);
          acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.z, b.z, acc, 0, 0, 0);
          acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.w, b.w, acc, 0, 0, 0);
        }
      }
    }
    if (mine) {
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int i = (e & 3) + 8 * (e >> 2) + 4 * hh, j = t0 + wave * 32 + i;      // C/D map of the 32x32 shapes: row = train row of the tile
        float d2 = (qn + s_tnorm[wave * 32 + i]) - 2.f * acc[e];
        d2 = d2 < 0.f ? 0.f : d2;
        const unsigned long long key = ((unsigned long long)__float_as_uint(d2) << 32) | (unsigned)j;
        if (j < nt && key < best) best = key;
      }
    }
  }
  {
    const unsigned long long o = __shfl_xor(best, 32, 64);
    best = o < best ? o : best;
  }
  if (lane < 32) s_best[wave][lane] = best;
  __syncthreads();
  if (tid < LM_QROWS && q0 + tid < nq) {
    unsigned long long b = s_best[0][tid];
#pragma unroll
    for (int w = 1; w < 4; ++w) b = s_best[w][tid] < b ? s_best[w][tid] : b;
    uint8_t *o = out + (size_t)blockIdx.y * lay.stride;
    reinterpret_cast<int32_t *>(o + lay.tidx)[q0 + tid] = (int32_t)(unsigned)(b & 0xffffffffull);
    reinterpret_cast<float *>(o + lay.dist)[q0 + tid] = sqrtf(__uint_as_float((unsigned)(b >> 32)));
  }
}

// ---- the RANSAC stage ---------------------------------------------------------------------------------------------------------------------------------
// draw number d of hypothesis h (the header's text)
__device__ __forceinline__ int loop_draw(uint64_t seed, int h, int d, int n) {
  const uint64_t z = splitmix64(seed ^ (((uint64_t)(uint32_t)h << 32) | (uint32_t)d));
  return (int)(((z >> 32) * (uint64_t)(uint32_t)n) >> 32);
}

// belowThreshold(cam, T * x, uvu, thr^2) (ransac_models.cpp:27-42) with map_uvu as written in stereo_camera.cpp:36-44; P = [R | t] row-major.  NaN / inf compare false
__device__ __forceinline__ bool loop_inlier(const double *P, double x, double y, double z, double u0, double u1, double u2, const loop_cam &cam, double thr2) {
  const double X = ((P[0] * x + P[1] * y) + P[2] * z) + P[3];
  const double Y = ((P[4] * x + P[5] * y) + P[6] * z) + P[7];
  const double Z = ((P[8] * x + P[9] * y) + P[10] * z) + P[11];
  const double du = u0 - (cam.f * (X / Z) + cam.cx);
  const double dv = u1 - (cam.f * (Y / Z) + cam.cy);
  const double dr = u2 - (((X - cam.b) / Z) * cam.f + cam.cx);
  return du * du < thr2 && dv * dv < thr2 && dr * dr < thr2;
}

// one step of the one-sided (Hestenes) Jacobi SVD: rotate columns p, q of G (and of V) until they are orthogonal
__device__ __forceinline__ bool loop_jacobi_pair(double (&gp)[3], double (&gq)[3], double (&vp)[3], double (&vq)[3]) {
  const double a = (gp[0] * gp[0] + gp[1] * gp[1]) + gp[2] * gp[2], b = (gq[0] * gq[0] + gq[1] * gq[1]) + gq[2] * gq[2];
  const double g = (gp[0] * gq[0] + gp[1] * gq[1]) + gp[2] * gq[2];
  if (!(fabs(g) > LOOP_JTOL * sqrt(a * b))) return false;
  const double zeta = (b - a) / (2.0 * g);
  const double t = copysign(1.0, zeta) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
  const double c = 1.0 / sqrt(1.0 + t * t), s = c * t;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const double x = gp[k], y = gq[k], vx = vp[k], vy = vq[k];
    gp[k] = c * x - s * y; gq[k] = s * x + c * y;
    vp[k] = c * vx - s * vy; vq[k] = s * vx + c * vy;
  }
  return true;
}
__device__ __forceinline__ void loop_swap3(double (&a)[3], double (&b)[3], bool doit) {
#pragma unroll
  for (int k = 0; k < 3; ++k) { const double x = a[k], y = b[k]; a[k] = doit ? y : x; b[k] = doit ? x : y; }
}
__device__ __forceinline__ void loop_cross(const double (&a)[3], const double (&b)[3], double (&c)[3]) {
  c[0] = a[1] * b[2] - a[2] * b[1]; c[1] = a[2] * b[0] - a[0] * b[2]; c[2] = a[0] * b[1] - a[1] * b[0];
}
// SE3Model::calc_motion (ransac_models.cpp:138-169) over getOrientationAndCentriods (:44-81): p0 = query points, p1 = train points, H = sum p1 p0^T = U S V^T,
// R = V U^T with V.col(2) negated when det < 0, t = c0 - R c1.  Three centred points span a plane, so H has rank 2 and the sign rule decides the third pair:
// R = v1 u1^T + v2 u2^T + (v1 x v2)(u1 x u2)^T is that proper rotation for any signs of the two leading pairs.  The pairs come from a one-sided Jacobi SVD
// on the columns of H (H V = U S: relative accuracy of a backward-stable SVD, no squaring of the condition number).  P = [R | t] row-major
__device__ void loop_fit(double (&p0)[3][3], double (&p1)[3][3], double *P) {
  double c0[3], c1[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    c0[k] = ((p0[0][k] + p0[1][k]) + p0[2][k]) * (1.0 / 3.0);
    c1[k] = ((p1[0][k] + p1[1][k]) + p1[2][k]) * (1.0 / 3.0);
  }
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int k = 0; k < 3; ++k) { p0[i][k] -= c0[k]; p1[i][k] -= c1[k]; }
  double G[3][3], V[3][3];      // columns: G[c][r] = H(r, c) = sum_i p1_i[r] p0_i[c]
#pragma unroll
  for (int c = 0; c < 3; ++c)
#pragma unroll
    for (int rr = 0; rr < 3; ++rr) {
      G[c][rr] = (p1[0][rr] * p0[0][c] + p1[1][rr] * p0[1][c]) + p1[2][rr] * p0[2][c];
      V[c][rr] = c == rr ? 1.0 : 0.0;
    }
  for (int sweep = 0; sweep < 30; ++sweep) {
    bool moved = loop_jacobi_pair(G[0], G[1], V[0], V[1]);
    moved = loop_jacobi_pair(G[0], G[2], V[0], V[2]) || moved;
    moved = loop_jacobi_pair(G[1], G[2], V[1], V[2]) || moved;
    if (!moved) break;
  }
  // the column of the smallest singular value goes last
  double n[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) n[c] = (G[c][0] * G[c][0] + G[c][1] * G[c][1]) + G[c][2] * G[c][2];
  const bool s0 = n[0] <= n[1] && n[0] <= n[2], s1 = !s0 && n[1] <= n[2];
  loop_swap3(G[0], G[2], s0); loop_swap3(V[0], V[2], s0);
  { const double x = n[0]; n[0] = s0 ? n[2] : x; }
  loop_swap3(G[1], G[2], s1); loop_swap3(V[1], V[2], s1);
  { const double x = n[1]; n[1] = s1 ? n[2] : x; }
  double u1[3], u2[3], u3[3], v3[3];
  const double i1 = 1.0 / sqrt(n[0]), i2 = 1.0 / sqrt(n[1]);
#pragma unroll
  for (int k = 0; k < 3; ++k) { u1[k] = G[0][k] * i1; u2[k] = G[1][k] * i2; }
  loop_cross(u1, u2, u3);
  loop_cross(V[0], V[1], v3);
#pragma unroll
  for (int i = 0; i < 3; ++i) {
#pragma unroll
    for (int j = 0; j < 3; ++j) P[4 * i + j] = (V[0][i] * u1[j] + V[1][i] * u2[j]) + v3[i] * u3[j];
  }
#pragma unroll
  for (int i = 0; i < 3; ++i) P[4 * i + 3] = c0[i] - ((P[4 * i] * c1[0] + P[4 * i + 1] * c1[1]) + P[4 * i + 2] * c1[2]);
}

// grid = checks, 8 waves.  Phase A: lane = hypothesis (draw or take the triple, fit, pose into LDS).  Phase B: lane = match, loop over the hypotheses; a wave's
// count of one hypothesis is a ballot, kept by lane h & 63 in register h >> 6 until the waves' counts meet in LDS.  Phase C: the first maximum.  Phase D: the final pass.
__global__ __launch_bounds__(LR_THREADS) void loop_ransac_kernel(const double *__restrict__ uvu, const double *__restrict__ xyz, size_t place_rows,
                                                                const uint8_t *__restrict__ in, size_t in_stride, uint8_t *__restrict__ out, loop_out_layout lay,
                                                                loop_cam cam) {
  __shared__ double s_pose[LOOP_MAX_HYP][12];
  __shared__ int s_valid[LOOP_MAX_HYP];
  __shared__ int s_cnt[LR_THREADS / 64][LOOP_MAX_HYP];
  __shared__ int s_key[4], s_ninv[4], s_ninl[LR_THREADS / 64];
  const loop_check_dev *ck = reinterpret_cast<const loop_check_dev *>(in + (size_t)blockIdx.x * in_stride);
  const int32_t *smp_in = reinterpret_cast<const int32_t *>(ck + 1);
  uint8_t *o = out + (size_t)blockIdx.x * lay.stride;
  const int32_t *tidx = reinterpret_cast<const int32_t *>(o + lay.tidx);      // the distance stage's output (the launch before this one)
  int32_t *smp_out = reinterpret_cast<int32_t *>(o + lay.smp), *hinl = reinterpret_cast<int32_t *>(o + lay.hinl);
  uint8_t *inl = o + lay.inl;
  const int n = ck->nq, nt = ck->nt, H = ck->n_hyp;
  const double *qu = uvu + (size_t)ck->q_slot * place_rows * 3, *tx = xyz + (size_t)ck->t_slot * place_rows * 3;
  const double thr2 = ck->pixel_thr * ck->pixel_thr;
  const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;

  // ---- A: hypotheses
  if (tid < LOOP_MAX_HYP) {
    bool valid = false;
    int r0 = -1, r1 = -1, r2 = -1;
    if (tid < H && n >= 3) {
      if (ck->has_samples) {
        r0 = smp_in[3 * tid]; r1 = smp_in[3 * tid + 1]; r2 = smp_in[3 * tid + 2];
        valid = (unsigned)r0 < (unsigned)n && (unsigned)r1 < (unsigned)n && (unsigned)r2 < (unsigned)n && r0 != r1 && r0 != r2 && r1 != r2;
        if (valid) {
          const int t0 = tidx[r0], t1 = tidx[r1], t2 = tidx[r2];
          valid = t0 != t1 && t0 != t2 && t1 != t2;
        }
      } else {
        // ransac.cpp:68-96: a repeated element is redrawn alone, a train clash restarts the triple (query index = match index: distinct with the elements)
        const uint64_t seed = ck->seed;
        int d = 0;
        while (!valid && d < LOOP_MAX_DRAWS) {
          r0 = loop_draw(seed, tid, d++, n);
          r1 = r0;
          while (r1 == r0 && d < LOOP_MAX_DRAWS) r1 = loop_draw(seed, tid, d++, n);
          if (r1 == r0) break;
          r2 = r0;
          while ((r2 == r0 || r2 == r1) && d < LOOP_MAX_DRAWS) r2 = loop_draw(seed, tid, d++, n);
          if (r2 == r0 || r2 == r1) break;
          const int t0 = tidx[r0], t1 = tidx[r1], t2 = tidx[r2];
          valid = t0 != t1 && t0 != t2 && t1 != t2;
        }
      }
      int t0 = 0, t1 = 0, t2 = 0;
      if (valid) {
        t0 = tidx[r0]; t1 = tidx[r1]; t2 = tidx[r2];
        valid = (unsigned)t0 < (unsigned)nt && (unsigned)t1 < (unsigned)nt && (unsigned)t2 < (unsigned)nt;      // (always, by the distance stage)
      }
      if (valid) {
        const int rs[3] = {r0, r1, r2}, ts[3] = {t0, t1, t2};
        double p0[3][3], p1[3][3], P[12];
#pragma unroll
        for (int i = 0; i < 3; ++i) {
          loop_unmap_uvu(cam, qu[3 * rs[i]], qu[3 * rs[i] + 1], qu[3 * rs[i] + 2], p0[i][0], p0[i][1], p0[i][2]);
          p1[i][0] = tx[3 * ts[i]]; p1[i][1] = tx[3 * ts[i] + 1]; p1[i][2] = tx[3 * ts[i] + 2];
        }
        loop_fit(p0, p1, P);
#pragma unroll
        for (int k = 0; k < 12; ++k) s_pose[tid][k] = P[k];
      }
    }
    if (!valid) r0 = r1 = r2 = -1;
    if (tid < H) { smp_out[3 * tid] = r0; smp_out[3 * tid + 1] = r1; smp_out[3 * tid + 2] = r2; }
    s_valid[tid] = valid ? 1 : 0;
    const int ninv = __popcll(__ballot(tid < H && !valid));
    if (lane == 0) s_ninv[wave] = ninv;
  }
  __syncthreads();

  // ---- B: scores
  int c[LOOP_MAX_HYP / 64] = {0, 0, 0, 0};
  for (int base = wave * 64; base < n; base += LR_THREADS) {      // wave-uniform trip count
    const int i = base + lane;
    const bool act = i < n;
    const int ii = act ? i : 0;
    const double u0 = qu[3 * ii], u1 = qu[3 * ii + 1], u2 = qu[3 * ii + 2];
    const int t = tidx[ii];
    const double x = tx[3 * t], y = tx[3 * t + 1], z = tx[3 * t + 2];
#pragma unroll
    for (int hb = 0; hb < LOOP_MAX_HYP / 64; ++hb) {
      for (int hl = 0; hl < 64 && hb * 64 + hl < H; ++hl) {
        const int h = hb * 64 + hl;
        if (!s_valid[h]) continue;
        const int cnt = __popcll(__ballot(act && loop_inlier(s_pose[h], x, y, z, u0, u1, u2, cam, thr2)));
        c[hb] += lane == hl ? cnt : 0;
      }
    }
  }
#pragma unroll
  for (int hb = 0; hb < LOOP_MAX_HYP / 64; ++hb) s_cnt[wave][hb * 64 + lane] = c[hb];
  __syncthreads();

  // ---- C: the first hypothesis with the strictly greatest count, from bestinl = 0 (ransac.cpp:62, :120-124)
  if (tid < LOOP_MAX_HYP) {
    int tot = 0;
#pragma unroll
    for (int w = 0; w < LR_THREADS / 64; ++w) tot += s_cnt[w][tid];
    if (tid < H) hinl[tid] = tot;
    int key = tid < H && tot > 0 ? (tot << 9) | (511 - tid) : 0;      // counts <= max_desc < 2^22
#pragma unroll
    for (int m = 32; m > 0; m >>= 1) key = max(key, __shfl_xor(key, m, 64));
    if (lane == 0) s_key[wave] = key;
  }
  __syncthreads();
  const int key = max(max(s_key[0], s_key[1]), max(s_key[2], s_key[3]));
  const int best = key > 0 ? 511 - (key & 511) : -1;
  double P[12];
#pragma unroll
  for (int k = 0; k < 12; ++k) P[k] = best >= 0 ? s_pose[best][k] : (k % 5 == 0 ? 1.0 : 0.0);

  // ---- D: the final pass (ransac.cpp:126-135; with the identity when nothing was selected; not at all below three matches, :60-61)
  int ninl = 0;
  for (int base = wave * 64; base < n; base += LR_THREADS) {
    const int i = base + lane;
    const bool act = i < n;
    const int ii = act ? i : 0;
    const int t = tidx[ii];
    const bool in = act && n >= 3 && loop_inlier(P, tx[3 * t], tx[3 * t + 1], tx[3 * t + 2], qu[3 * ii], qu[3 * ii + 1], qu[3 * ii + 2], cam, thr2);
    if (act) inl[i] = in ? 1 : 0;
    ninl += __popcll(__ballot(in));
  }
  if (lane == 0) s_ninl[wave] = ninl;
  __syncthreads();
  if (tid == 0) {
    svs_loop_result *res = reinterpret_cast<svs_loop_result *>(o);
    int tot = 0;
    for (int w = 0; w < LR_THREADS / 64; ++w) tot += s_ninl[w];
    res->n_matches = n;
    res->n_inliers = tot;
    res->best_hyp = best;
    res->n_invalid_hyp = (s_ninv[0] + s_ninv[1]) + (s_ninv[2] + s_ninv[3]);
    for (int k = 0; k < 12; ++k) res->T_query_from_train[k] = P[k];
  }
}

// ---- host --------------------------------------------------------------------------------------------------------------------------------------------
extern "C" int svs_loop_destroy(svs_loop *l) {
  if (!l) return SVS_OK;
  delete l;
  return SVS_OK;
}

static int loop_alloc(svs_loop *l) {
  svs_ctx *ctx = l->ctx;
  const size_t rows = (size_t)l->max_places * l->max_desc;
  SVS_HIP(ctx, l->d_desc.alloc(rows * l->K));
  SVS_HIP(ctx, l->d_norm.alloc(rows));
  SVS_HIP(ctx, l->d_uvu.alloc(rows * 3));
  SVS_HIP(ctx, l->d_xyz.alloc(rows * 3));
  SVS_HIP(ctx, l->h_stage.alloc((size_t)l->max_desc * (l->K * sizeof(float) + 6 * sizeof(double))));
  SVS_HIP(ctx, l->ev_stage.create(hipEventDisableTiming));
  SVS_HIP(ctx, l->d_in.alloc(l->in_stride * l->max_checks));
  SVS_HIP(ctx, l->d_out.alloc(l->lay.stride * l->max_checks));
  SVS_HIP(ctx, l->h_in.alloc(l->in_stride * l->max_checks));
  SVS_HIP(ctx, l->h_out.alloc(l->lay.stride * l->max_checks));
  for (int i = 0; i < 3; ++i) SVS_HIP(ctx, l->ev[i].create());
  return SVS_OK;
}

extern "C" int svs_loop_create(svs_ctx *ctx, const svs_cam *cam, int desc_dim, int max_desc, int max_places, int max_hyp, int max_checks, svs_loop **out) {
  SVS_REQUIRE(ctx, ctx && cam && out && (desc_dim == 64 || desc_dim == 128) && max_desc >= 1 && max_desc <= (1 << 21) && max_places >= 1 && max_hyp >= 1 &&
                       max_hyp <= LOOP_MAX_HYP && max_checks >= 1);
  SVS_REQUIRE(ctx, cam->f > 0.0 && cam->b > 0.0);
  SVS_DEVICE(ctx);
  std::unique_ptr<svs_loop> l(new svs_loop());
  l->ctx = ctx;
  l->cam = loop_cam{cam->f, cam->cx, cam->cy, cam->b};
  l->K = desc_dim; l->max_desc = max_desc; l->max_places = max_places; l->max_hyp = max_hyp; l->max_checks = max_checks;
  l->n_place.reset(new int[max_places]());
  l->in_stride = loop_align16(sizeof(loop_check_dev) + (size_t)max_hyp * 3 * sizeof(int32_t));
  l->lay.tidx = (int)loop_align16(sizeof(svs_loop_result));
  l->lay.dist = l->lay.tidx + 4 * max_desc;
  l->lay.smp = l->lay.dist + 4 * max_desc;
  l->lay.hinl = l->lay.smp + 12 * max_hyp;
  l->lay.inl = l->lay.hinl + 4 * max_hyp;
  l->lay.stride = loop_align16((size_t)l->lay.inl + max_desc);
  if (int rc = loop_alloc(l.get())) return rc;
  *out = l.release();
  return SVS_OK;
}

extern "C" int svs_loop_set_place(svs_loop *l, int slot, int n, const float *h_desc, const double *h_uvu, const double *h_xyz) {
  svs_ctx *ctx = l ? l->ctx : nullptr;
  SVS_REQUIRE(ctx, l && slot >= 0 && slot < l->max_places && n >= 1 && h_desc && h_uvu);
  LOOP_CAPACITY(ctx, n <= l->max_desc);
  if (!h_xyz)
    for (int i = 0; i < n; ++i) SVS_REQUIRE(ctx, h_uvu[3 * i] - h_uvu[3 * i + 2] > 0.0);      // addLocation keeps disp > 0 only (placerecognizer.cpp:230)
  SVS_DEVICE(ctx);
  if (l->stage_busy) { SVS_HIP(ctx, hipEventSynchronize(l->ev_stage)); l->stage_busy = false; }      // the previous place has left the staging buffer
  const size_t nd = (size_t)n * l->K * sizeof(float), nu = (size_t)n * 3 * sizeof(double), row0 = (size_t)slot * l->max_desc;
  uint8_t *s = l->h_stage;
  memcpy(s, h_desc, nd);
  memcpy(s + nd, h_uvu, nu);
  if (h_xyz) memcpy(s + nd + nu, h_xyz, nu);
  SVS_HIP(ctx, hipMemcpyAsync(l->d_desc + row0 * l->K, s, nd, hipMemcpyHostToDevice, ctx->stream));
  SVS_HIP(ctx, hipMemcpyAsync(l->d_uvu + row0 * 3, s + nd, nu, hipMemcpyHostToDevice, ctx->stream));
  if (h_xyz) SVS_HIP(ctx, hipMemcpyAsync(l->d_xyz + row0 * 3, s + nd + nu, nu, hipMemcpyHostToDevice, ctx->stream));
  SVS_HIP(ctx, hipEventRecord(l->ev_stage, ctx->stream));
  l->stage_busy = true;
  hipLaunchKernelGGL(loop_place_kernel, dim3(div_up(n, 256)), dim3(256), 0, ctx->stream, l->d_desc + row0 * l->K, l->K, n, l->d_norm + row0, l->d_uvu + row0 * 3,
                     l->d_xyz + row0 * 3, h_xyz ? 0 : 1, l->cam);
  SVS_LAUNCH_CHECK(ctx);
  l->n_place[slot] = n;
  return SVS_OK;
}

// internal (common.h): svs_loop_set_place with the descriptors and uvu already on the device (svs_loop_set_place_from_surf, surf.hip).  Nothing is checked on
// the host here: whoever made the arrays guarantees uvu[0] - uvu[2] > 0 for every row (svs_surf_extract's disparity filter keeps no other keypoint).  The
// copies are device to device on the context's stream, norms and xyz by the same kernel
int svs_loop_set_place_dev(svs_loop *l, int slot, int n, const float *d_desc, const double *d_uvu) {
  svs_ctx *ctx = l ? l->ctx : nullptr;
  SVS_REQUIRE(ctx, l && slot >= 0 && slot < l->max_places && n >= 1 && d_desc && d_uvu && l->K == 64);
  LOOP_CAPACITY(ctx, n <= l->max_desc);
  SVS_DEVICE(ctx);
  const size_t nd = (size_t)n * l->K * sizeof(float), nu = (size_t)n * 3 * sizeof(double), row0 = (size_t)slot * l->max_desc;
  SVS_HIP(ctx, hipMemcpyAsync(l->d_desc + row0 * l->K, d_desc, nd, hipMemcpyDeviceToDevice, ctx->stream));
  SVS_HIP(ctx, hipMemcpyAsync(l->d_uvu + row0 * 3, d_uvu, nu, hipMemcpyDeviceToDevice, ctx->stream));
  hipLaunchKernelGGL(loop_place_kernel, dim3(div_up(n, 256)), dim3(256), 0, ctx->stream, l->d_desc + row0 * l->K, l->K, n, l->d_norm + row0, l->d_uvu + row0 * 3,
                     l->d_xyz + row0 * 3, 1, l->cam);
  SVS_LAUNCH_CHECK(ctx);
  l->n_place[slot] = n;
  return SVS_OK;
}
svs_ctx *svs_loop_ctx(svs_loop *l) { return l ? l->ctx : nullptr; }

extern "C" int svs_loop_set_timing(svs_loop *l, int on) {
  if (!l) return SVS_ERR_INVALID;
  l->timing = on ? 1 : 0;
  return SVS_OK;
}
extern "C" int svs_loop_stage_times(svs_loop *l, float *ms) {
  if (!l || !ms) return SVS_ERR_INVALID;
  ms[0] = l->stage_ms[0]; ms[1] = l->stage_ms[1];
  return SVS_OK;
}

extern "C" int svs_loop_check_batch(svs_loop *l, int n_checks, const svs_loop_check *checks, svs_loop_result *h_results, int32_t *h_train_idx, float *h_distance,
                                    uint8_t *h_inlier, int32_t *h_samples_out, int32_t *h_hyp_inliers) {
  svs_ctx *ctx = l ? l->ctx : nullptr;
  SVS_REQUIRE(ctx, l && n_checks >= 0 && (n_checks == 0 || checks));
  LOOP_CAPACITY(ctx, n_checks <= l->max_checks);
  int max_nq = 0;
  for (int c = 0; c < n_checks; ++c) {
    const svs_loop_check &k = checks[c];
    SVS_REQUIRE(ctx, k.query_slot >= 0 && k.query_slot < l->max_places && k.train_slot >= 0 && k.train_slot < l->max_places);
    SVS_REQUIRE(ctx, l->n_place[k.query_slot] > 0 && l->n_place[k.train_slot] > 0);      // an empty slot
    SVS_REQUIRE(ctx, k.n_hyp >= 1);
    LOOP_CAPACITY(ctx, k.n_hyp <= l->max_hyp);
    max_nq = std::max(max_nq, l->n_place[k.query_slot]);
  }
  if (n_checks == 0) return SVS_OK;
  SVS_DEVICE(ctx);
  for (int c = 0; c < n_checks; ++c) {
    const svs_loop_check &k = checks[c];
    loop_check_dev *d = reinterpret_cast<loop_check_dev *>(l->h_in + (size_t)c * l->in_stride);
    *d = loop_check_dev{k.query_slot, k.train_slot, k.n_hyp, k.h_samples ? 1 : 0, k.pixel_thr, k.seed, l->n_place[k.query_slot], l->n_place[k.train_slot]};
    if (k.h_samples) memcpy(d + 1, k.h_samples, (size_t)k.n_hyp * 3 * sizeof(int32_t));
  }
  SVS_HIP(ctx, hipMemcpyAsync(l->d_in, l->h_in, l->in_stride * n_checks, hipMemcpyHostToDevice, ctx->stream));
  if (l->timing) SVS_HIP(ctx, hipEventRecord(l->ev[0], ctx->stream));
  const dim3 mgrid(div_up(max_nq, LM_QROWS), n_checks);
  if (l->K == 64) hipLaunchKernelGGL(loop_match_kernel<64>, mgrid, dim3(256), 0, ctx->stream, l->d_desc, l->d_norm, (size_t)l->max_desc, l->d_in, l->in_stride, l->d_out, l->lay);
  else hipLaunchKernelGGL(loop_match_kernel<128>, mgrid, dim3(256), 0, ctx->stream, l->d_desc, l->d_norm, (size_t)l->max_desc, l->d_in, l->in_stride, l->d_out, l->lay);
  SVS_LAUNCH_CHECK(ctx);
  if (l->timing) SVS_HIP(ctx, hipEventRecord(l->ev[1], ctx->stream));
  hipLaunchKernelGGL(loop_ransac_kernel, dim3(n_checks), dim3(LR_THREADS), 0, ctx->stream, l->d_uvu, l->d_xyz, (size_t)l->max_desc, l->d_in, l->in_stride, l->d_out,
                     l->lay, l->cam);
  SVS_LAUNCH_CHECK(ctx);
  if (l->timing) SVS_HIP(ctx, hipEventRecord(l->ev[2], ctx->stream));
  SVS_HIP(ctx, hipMemcpyAsync(l->h_out, l->d_out, l->lay.stride * n_checks, hipMemcpyDeviceToHost, ctx->stream));
  SVS_HIP(ctx, hipStreamSynchronize(ctx->stream));
  if (l->timing) {
    SVS_HIP(ctx, hipEventElapsedTime(&l->stage_ms[0], l->ev[0], l->ev[1]));
    SVS_HIP(ctx, hipEventElapsedTime(&l->stage_ms[1], l->ev[1], l->ev[2]));
  }
  // rows are max_desc (max_hyp) long; what lies behind a check's n_matches (n_hyp) is -1 / 0
  const int md = l->max_desc, mh = l->max_hyp;
  for (int c = 0; c < n_checks; ++c) {
    const uint8_t *o = l->h_out + (size_t)c * l->lay.stride;
    const int n = l->n_place[checks[c].query_slot], H = checks[c].n_hyp;
    if (h_results) memcpy(&h_results[c], o, sizeof(svs_loop_result));
    if (h_train_idx) { memcpy(h_train_idx + (size_t)c * md, o + l->lay.tidx, 4 * (size_t)n); std::fill(h_train_idx + (size_t)c * md + n, h_train_idx + (size_t)(c + 1) * md, -1); }
    if (h_distance) { memcpy(h_distance + (size_t)c * md, o + l->lay.dist, 4 * (size_t)n); std::fill(h_distance + (size_t)c * md + n, h_distance + (size_t)(c + 1) * md, 0.f); }
    if (h_inlier) { memcpy(h_inlier + (size_t)c * md, o + l->lay.inl, (size_t)n); memset(h_inlier + (size_t)c * md + n, 0, (size_t)(md - n)); }
    if (h_samples_out) { memcpy(h_samples_out + (size_t)c * mh * 3, o + l->lay.smp, 12 * (size_t)H); std::fill(h_samples_out + ((size_t)c * mh + H) * 3, h_samples_out + (size_t)(c + 1) * mh * 3, -1); }
    if (h_hyp_inliers) { memcpy(h_hyp_inliers + (size_t)c * mh, o + l->lay.hinl, 4 * (size_t)H); std::fill(h_hyp_inliers + (size_t)c * mh + H, h_hyp_inliers + (size_t)(c + 1) * mh, 0); }
  }
  return SVS_OK;
}

// ---- the place index: visual words, inverted index, TF-IDF scores (placerecognizer.cpp:248-318) -----------------------------------------------------------------
// Words.  grid = (query blocks of 32, vocabulary chunks of LW_CHUNK rows, locations), 4 waves: the tile walk, the MFMA feeding and the per-pair arithmetic of
// loop_match_kernel, so a pair's d2 does not depend on the chunk or the batch it falls in; the chunks meet in a 64-bit atomic minimum on the same key, whose
// minimum is order-independent.  One keyframe of 500 descriptors against 9 983 words is 16 x 39 workgroups.  A lane issues the eight 16-byte loads of its
// share of a tile together and stores them to LDS when they have arrived.  A form that fetched the NEXT tile into registers under the MFMAs of the present one
// kept 32 registers more alive (two waves per SIMD instead of three) and measured 5 to 9 % slower at both sizes (profiles/place_index.md): the workgroups of
// the other chunks are what hides the load.
// The walk itself is loop_words_walk (loop_words.h), shared with the vocabulary trainer (vocab.hip).
template <int K>
__global__ __launch_bounds__(256) void loop_words_kernel(const float *__restrict__ desc, const float *__restrict__ norm, size_t place_rows, const float *__restrict__ W,
                                                        const float *__restrict__ Wn, int n_words, const uint8_t *__restrict__ in, size_t in_stride,
                                                        unsigned long long *__restrict__ wkey, int max_desc) {
  const loop_loc_dev *lc = reinterpret_cast<const loop_loc_dev *>(in + (size_t)blockIdx.z * in_stride);
  const int nq = lc->n, q0 = (int)blockIdx.x * LM_QROWS;
  if (q0 >= nq) return;                                                    // (the grid is sized for the longest place of the call)
  const int c0 = (int)blockIdx.y * LW_CHUNK, c1 = min(n_words, c0 + LW_CHUNK);      // this workgroup's words; c0 < n_words by the grid
  const float *Q = desc + (size_t)lc->slot * place_rows * K, *Qn = norm + (size_t)lc->slot * place_rows;
  const unsigned long long b = loop_words_walk<K>(Q, Qn, nq, q0, W, Wn, c0, c1);
  const int tid = (int)threadIdx.x;
  if (tid < LM_QROWS && q0 + tid < nq) atomicMin(wkey + (size_t)blockIdx.z * max_desc + q0 + tid, b);
}

// the call's work arrays: keys to "nothing yet", first occurrences to "none", the counters to 0.  grid-stride over locations x max(max_desc, n_words)
__global__ __launch_bounds__(256) void loop_index_reset_kernel(int n, int max_desc, int n_words, unsigned long long *__restrict__ wkey, int32_t *__restrict__ first,
                                                              int32_t *__restrict__ nwk, uint8_t *__restrict__ out, size_t out_stride) {
  const size_t m = (size_t)max(max_desc, n_words), total = m * n;
  for (size_t i = (size_t)blockIdx.x * 256u + threadIdx.x; i < total; i += (size_t)gridDim.x * 256u) {
    const size_t k = i / m, j = i - k * m;
    if (j < (size_t)max_desc) wkey[k * max_desc + j] = ~0ull;
    if (j < (size_t)n_words) first[k * n_words + j] = INT32_MAX;
    if (j == 0) {
      nwk[k] = 0;
      loop_loc_out *h = reinterpret_cast<loop_loc_out *>(out + k * out_stride);
      h->best_key = 0ull; h->n_scored = 0; h->number_of_words = 0;
    }
  }
}

// grid = (descriptor blocks, locations).  The word of every descriptor, and everything about the insertion that does not depend on the order: the place's
// column of cnt (integer atomics), the first descriptor that carries each word, the number of words
__global__ __launch_bounds__(256) void loop_assign_kernel(const uint8_t *__restrict__ in, size_t in_stride, const unsigned long long *__restrict__ wkey, int max_desc,
                                                         int n_words, int max_places, int32_t *__restrict__ cnt, int32_t *__restrict__ first, int32_t *__restrict__ nwk,
                                                         uint8_t *__restrict__ out, loop_index_layout lay) {
  const int k = (int)blockIdx.y, r = (int)(blockIdx.x * 256u + threadIdx.x);
  const loop_loc_dev *lc = reinterpret_cast<const loop_loc_dev *>(in + (size_t)k * in_stride);
  const bool act = r < lc->n;
  int w = -1;
  if (act) {
    const unsigned long long key = wkey[(size_t)k * max_desc + r];
    const float d2 = __uint_as_float((unsigned)(key >> 32));
    const unsigned j = (unsigned)(key & 0xffffffffull);
    w = d2 < lc->radius && j < (unsigned)n_words ? (int)j : -1;
    uint8_t *o = out + (size_t)k * lay.stride;
    reinterpret_cast<int32_t *>(o + lay.word)[r] = w;
    reinterpret_cast<float *>(o + lay.d2)[r] = d2;
    if (w >= 0) {
      atomicMin(first + (size_t)k * n_words + w, r);
      atomicAdd(cnt + (size_t)w * max_places + lc->slot, 1);
    }
  }
  const int c = __popcll(__ballot(w >= 0));
  if ((threadIdx.x & 63) == 0 && c) atomicAdd(nwk + k, c);
}

// grid = (descriptor blocks, locations).  df as descriptor r of location k meets it = df before the call + the earlier locations of the call that hold the word
// + this location itself once an earlier descriptor of it has inserted the word; idf = (float)n_loc / (float)df, -1 where there is no scoring step
__global__ __launch_bounds__(256) void loop_idf_kernel(const uint8_t *__restrict__ in, size_t in_stride, int max_desc, int n_words, const int32_t *__restrict__ df,
                                                      const int32_t *__restrict__ first, const int32_t *__restrict__ nwk, int32_t *__restrict__ nw,
                                                      float *__restrict__ idf, uint8_t *__restrict__ out, loop_index_layout lay) {
  const int k = (int)blockIdx.y, r = (int)(blockIdx.x * 256u + threadIdx.x);
  const loop_loc_dev *lc = reinterpret_cast<const loop_loc_dev *>(in + (size_t)k * in_stride);
  if (r >= lc->n) return;
  uint8_t *o = out + (size_t)k * lay.stride;
  const int w = reinterpret_cast<const int32_t *>(o + lay.word)[r];
  float v = -1.f;
  if (w >= 0 && lc->do_detect) {
    int d = df[w] + (first[(size_t)k * n_words + w] < r ? 1 : 0);
    for (int e = 0; e < k; ++e) d += first[(size_t)e * n_words + w] != INT32_MAX ? 1 : 0;
    if (d > 0) v = (float)lc->n_loc / (float)d;
  }
  idf[(size_t)k * max_desc + r] = v;
  if (r == 0) {
    nw[lc->slot] = nwk[k];
    reinterpret_cast<loop_loc_out *>(o)->number_of_words = nwk[k];
  }
}

// grid = (place blocks, locations): one thread per (location, place).  The thread of place o reads column o of cnt and nothing of another thread's; cnt holds
// the call's locations already, and the host's byte "o is a location before this one, not excluded, not itself" decides whether the column counts.  Word and
// idf are wave-uniform.  The LS_BLOCK loads of a block of descriptors are issued together; only the adds are a chain -- in descriptor order, every operation
// rounded on its own (no contraction in this file)
constexpr int LS_BLOCK = 32;
__global__ __launch_bounds__(256) void loop_score_kernel(const uint8_t *__restrict__ in, size_t in_stride, int max_desc, int max_places, const int32_t *__restrict__ cnt,
                                                        const int32_t *__restrict__ nw, const float *__restrict__ idf, uint8_t *__restrict__ out, loop_index_layout lay) {
  const int k = (int)blockIdx.y, o = (int)(blockIdx.x * 256u + threadIdx.x);
  const loop_loc_dev *lc = reinterpret_cast<const loop_loc_dev *>(in + (size_t)k * in_stride);
  const uint8_t *vis = reinterpret_cast<const uint8_t *>(lc + 1);
  uint8_t *ob = out + (size_t)k * lay.stride;
  const int32_t *word = reinterpret_cast<const int32_t *>(ob + lay.word);
  const float *f = idf + (size_t)k * max_desc;
  const int n = lc->n;
  float s = 0.f;
  bool got = false;
  if (o < max_places && lc->do_detect && vis[o]) {
    const float nwo = (float)nw[o];
    for (int r0 = 0; r0 < n; r0 += LS_BLOCK) {
      int c[LS_BLOCK]; float v[LS_BLOCK];
#pragma unroll
      for (int u = 0; u < LS_BLOCK; ++u) {
        const int r = r0 + u, w = r < n ? word[r] : -1;
        v[u] = r < n ? f[r] : -1.f;
        c[u] = w >= 0 && v[u] >= 0.f ? cnt[(size_t)w * max_places + o] : 0;
      }
#pragma unroll
      for (int u = 0; u < LS_BLOCK; ++u)
        if (c[u] > 0) {
          const float tf = (float)c[u] / nwo, val = tf * v[u];
          s = s + val;
          got = true;
        }
    }
  }
  if (o < max_places) reinterpret_cast<float *>(ob + lay.score)[o] = s;
  // the greatest score above 0, the lowest slot on a tie: positive floats order like their bits
  unsigned long long key = got && s > 0.f ? ((unsigned long long)__float_as_uint(s) << 32) | (0xffffffffu - (unsigned)o) : 0ull;
#pragma unroll
  for (int m = 32; m > 0; m >>= 1) {
    const unsigned long long x = __shfl_xor(key, m, 64);
    key = x > key ? x : key;
  }
  const int ngot = __popcll(__ballot(got));
  if ((threadIdx.x & 63) == 0) {
    loop_loc_out *h = reinterpret_cast<loop_loc_out *>(ob);
    if (ngot) atomicAdd(&h->n_scored, ngot);
    if (key) atomicMax(&h->best_key, key);
  }
}

// grid = (descriptor blocks, locations): df takes the call's locations (the first descriptor with a word speaks for its location)
__global__ __launch_bounds__(256) void loop_commit_kernel(const uint8_t *__restrict__ in, size_t in_stride, int n_words, const int32_t *__restrict__ first,
                                                         int32_t *__restrict__ df, const uint8_t *__restrict__ out, loop_index_layout lay) {
  const int k = (int)blockIdx.y, r = (int)(blockIdx.x * 256u + threadIdx.x);
  const loop_loc_dev *lc = reinterpret_cast<const loop_loc_dev *>(in + (size_t)k * in_stride);
  if (r >= lc->n) return;
  const int w = reinterpret_cast<const int32_t *>(out + (size_t)k * lay.stride + lay.word)[r];
  if (w >= 0 && first[(size_t)k * n_words + w] == r) atomicAdd(df + w, 1);
}

extern "C" int svs_loop_set_vocabulary(svs_loop *l, int n_words, const float *h_words) {
  svs_ctx *ctx = l ? l->ctx : nullptr;
  SVS_REQUIRE(ctx, l && n_words >= 1 && h_words);
  LOOP_CAPACITY(ctx, n_words <= SVS_LOOP_MAX_WORDS);
  SVS_DEVICE(ctx);
  SVS_HIP(ctx, hipStreamSynchronize(ctx->stream));
  l->n_words = 0; l->n_loc = 0;                                            // (no vocabulary while this call can still give up)
  const size_t P = (size_t)l->max_places, C = (size_t)l->max_checks, nwd = (size_t)n_words;
  SVS_HIP(ctx, l->d_words.alloc(nwd * l->K));
  SVS_HIP(ctx, l->d_wnorm.alloc(nwd));
  SVS_HIP(ctx, l->d_cnt.alloc(nwd * P));
  SVS_HIP(ctx, l->d_df.alloc(nwd));
  SVS_HIP(ctx, l->d_nw.alloc(P));
  SVS_HIP(ctx, l->d_wkey.alloc(C * l->max_desc));
  SVS_HIP(ctx, l->d_first.alloc(C * nwd));
  SVS_HIP(ctx, l->d_nwk.alloc(C));
  SVS_HIP(ctx, l->d_idf.alloc(C * l->max_desc));
  l->ix_in_stride = loop_align16(sizeof(loop_loc_dev) + P);
  l->ixl.word = (int)loop_align16(sizeof(loop_loc_out));
  l->ixl.d2 = l->ixl.word + 4 * l->max_desc;
  l->ixl.score = l->ixl.d2 + 4 * l->max_desc;
  l->ixl.stride = loop_align16((size_t)l->ixl.score + 4 * P);
  SVS_HIP(ctx, l->d_ix_in.alloc(l->ix_in_stride * C));
  SVS_HIP(ctx, l->h_ix_in.alloc(l->ix_in_stride * C));
  SVS_HIP(ctx, l->d_ix_out.alloc(l->ixl.stride * C));
  SVS_HIP(ctx, l->h_ix_out.alloc(l->ixl.stride * C));
  l->is_loc.reset(new uint8_t[P]());
  SVS_HIP(ctx, hipMemcpyAsync(l->d_words, h_words, nwd * l->K * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
  hipLaunchKernelGGL(loop_place_kernel, dim3(div_up(n_words, 256)), dim3(256), 0, ctx->stream, l->d_words, l->K, n_words, l->d_wnorm, (const double *)nullptr,
                     (double *)nullptr, 0, l->cam);
  SVS_LAUNCH_CHECK(ctx);
  SVS_HIP(ctx, hipMemsetAsync(l->d_cnt, 0, nwd * P * sizeof(int32_t), ctx->stream));
  SVS_HIP(ctx, hipMemsetAsync(l->d_df, 0, nwd * sizeof(int32_t), ctx->stream));
  SVS_HIP(ctx, hipMemsetAsync(l->d_nw, 0, P * sizeof(int32_t), ctx->stream));
  SVS_HIP(ctx, hipStreamSynchronize(ctx->stream));
  l->n_words = n_words;
  return SVS_OK;
}

extern "C" int svs_loop_index_stage_times(svs_loop *l, float *ms) {
  if (!l || !ms) return SVS_ERR_INVALID;
  ms[0] = l->index_ms[0]; ms[1] = l->index_ms[1];
  return SVS_OK;
}

extern "C" int svs_loop_add_locations(svs_loop *l, int n, const svs_loop_location *locs, svs_loop_location_result *h_results, int32_t *h_word, float *h_word_d2,
                                      float *h_scores) {
  svs_ctx *ctx = l ? l->ctx : nullptr;
  SVS_REQUIRE(ctx, l && n >= 0 && (n == 0 || locs));
  SVS_REQUIRE(ctx, l->n_words > 0);                                        // no vocabulary
  LOOP_CAPACITY(ctx, n <= l->max_checks);
  const int P = l->max_places, md = l->max_desc;
  int max_n = 0;
  for (int k = 0; k < n; ++k) {
    const svs_loop_location &c = locs[k];
    SVS_REQUIRE(ctx, c.slot >= 0 && c.slot < P && l->n_place[c.slot] > 0 && !l->is_loc[c.slot]);
    SVS_REQUIRE(ctx, c.n_exclude >= 0 && (c.n_exclude == 0 || c.h_exclude));
    for (int e = 0; e < c.n_exclude; ++e) SVS_REQUIRE(ctx, c.h_exclude[e] >= 0 && c.h_exclude[e] < P);
    for (int e = 0; e < k; ++e) SVS_REQUIRE(ctx, locs[e].slot != c.slot);
    max_n = std::max(max_n, l->n_place[c.slot]);
  }
  if (n == 0) return SVS_OK;
  SVS_DEVICE(ctx);
  for (int k = 0; k < n; ++k) {
    const svs_loop_location &c = locs[k];
    loop_loc_dev *d = reinterpret_cast<loop_loc_dev *>(l->h_ix_in + (size_t)k * l->ix_in_stride);
    *d = loop_loc_dev{c.slot, l->n_place[c.slot], c.do_loop_detection ? 1 : 0, l->n_loc + k, c.radius, {0.f, 0.f, 0.f}};
    uint8_t *vis = reinterpret_cast<uint8_t *>(d + 1);
    memcpy(vis, l->is_loc.get(), (size_t)P);
    for (int e = 0; e < k; ++e) vis[locs[e].slot] = 1;
    for (int e = 0; e < c.n_exclude; ++e) vis[c.h_exclude[e]] = 0;
    vis[c.slot] = 0;
  }
  SVS_HIP(ctx, hipMemcpyAsync(l->d_ix_in, l->h_ix_in, l->ix_in_stride * n, hipMemcpyHostToDevice, ctx->stream));
  if (l->timing) SVS_HIP(ctx, hipEventRecord(l->ev[0], ctx->stream));
  const size_t reset_items = (size_t)std::max(md, l->n_words) * n;
  hipLaunchKernelGGL(loop_index_reset_kernel, dim3((unsigned)std::min<size_t>((reset_items + 255) / 256, 4096)), dim3(256), 0, ctx->stream, n, md, l->n_words,
                     l->d_wkey, l->d_first, l->d_nwk, l->d_ix_out, l->ixl.stride);
  SVS_LAUNCH_CHECK(ctx);
  const dim3 wgrid(div_up(max_n, LM_QROWS), div_up(l->n_words, LW_CHUNK), n);
  if (l->K == 64) hipLaunchKernelGGL(loop_words_kernel<64>, wgrid, dim3(256), 0, ctx->stream, l->d_desc, l->d_norm, (size_t)md, l->d_words, l->d_wnorm, l->n_words,
                                     l->d_ix_in, l->ix_in_stride, l->d_wkey, md);
  else hipLaunchKernelGGL(loop_words_kernel<128>, wgrid, dim3(256), 0, ctx->stream, l->d_desc, l->d_norm, (size_t)md, l->d_words, l->d_wnorm, l->n_words, l->d_ix_in,
                          l->ix_in_stride, l->d_wkey, md);
  SVS_LAUNCH_CHECK(ctx);
  if (l->timing) SVS_HIP(ctx, hipEventRecord(l->ev[1], ctx->stream));
  const dim3 rgrid(div_up(max_n, 256), n);
  hipLaunchKernelGGL(loop_assign_kernel, rgrid, dim3(256), 0, ctx->stream, l->d_ix_in, l->ix_in_stride, l->d_wkey, md, l->n_words, P, l->d_cnt, l->d_first, l->d_nwk,
                     l->d_ix_out, l->ixl);
  SVS_LAUNCH_CHECK(ctx);
  hipLaunchKernelGGL(loop_idf_kernel, rgrid, dim3(256), 0, ctx->stream, l->d_ix_in, l->ix_in_stride, md, l->n_words, l->d_df, l->d_first, l->d_nwk, l->d_nw, l->d_idf,
                     l->d_ix_out, l->ixl);
  SVS_LAUNCH_CHECK(ctx);
  hipLaunchKernelGGL(loop_score_kernel, dim3(div_up(P, 256), n), dim3(256), 0, ctx->stream, l->d_ix_in, l->ix_in_stride, md, P, l->d_cnt, l->d_nw, l->d_idf, l->d_ix_out,
                     l->ixl);
  SVS_LAUNCH_CHECK(ctx);
  hipLaunchKernelGGL(loop_commit_kernel, rgrid, dim3(256), 0, ctx->stream, l->d_ix_in, l->ix_in_stride, l->n_words, l->d_first, l->d_df, l->d_ix_out, l->ixl);
  SVS_LAUNCH_CHECK(ctx);
  if (l->timing) SVS_HIP(ctx, hipEventRecord(l->ev[2], ctx->stream));
  SVS_HIP(ctx, hipMemcpyAsync(l->h_ix_out, l->d_ix_out, l->ixl.stride * n, hipMemcpyDeviceToHost, ctx->stream));
  SVS_HIP(ctx, hipStreamSynchronize(ctx->stream));
  if (l->timing) {
    SVS_HIP(ctx, hipEventElapsedTime(&l->index_ms[0], l->ev[0], l->ev[1]));
    SVS_HIP(ctx, hipEventElapsedTime(&l->index_ms[1], l->ev[1], l->ev[2]));
  }
  for (int k = 0; k < n; ++k) {
    const uint8_t *o = l->h_ix_out + (size_t)k * l->ixl.stride;
    const loop_loc_out *h = reinterpret_cast<const loop_loc_out *>(o);
    const int nd = l->n_place[locs[k].slot];
    if (h_results) {
      svs_loop_location_result &res = h_results[k];
      res.number_of_words = h->number_of_words;
      res.n_scored = h->n_scored;
      res.best_slot = h->best_key ? (int32_t)(0xffffffffu - (uint32_t)(h->best_key & 0xffffffffull)) : -1;
      const uint32_t bits = (uint32_t)(h->best_key >> 32);
      memcpy(&res.best_score, &bits, 4);
      res.candidate = res.best_score > locs[k].min_score ? 1 : 0;
    }
    if (h_word) { memcpy(h_word + (size_t)k * md, o + l->ixl.word, 4 * (size_t)nd); std::fill(h_word + (size_t)k * md + nd, h_word + (size_t)(k + 1) * md, -1); }
    if (h_word_d2) { memcpy(h_word_d2 + (size_t)k * md, o + l->ixl.d2, 4 * (size_t)nd); std::fill(h_word_d2 + (size_t)k * md + nd, h_word_d2 + (size_t)(k + 1) * md, 0.f); }
    if (h_scores) memcpy(h_scores + (size_t)k * P, o + l->ixl.score, 4 * (size_t)P);
    l->is_loc[locs[k].slot] = 1;
  }
  l->n_loc += n;
  return SVS_OK;
}
