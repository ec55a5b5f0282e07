// match_wave.inc -- the two matchers with ONE WAVEFRONT per candidate point; included by match.hip behind match_predict.inc, whose PointPred records they read.
//   match_kernel    the round-1/2 window scan: a lane tests four positions with corner_bit, hits go to the wave's LDS list by ballots; any grid, any radius
//   match_kernel2   the lean scan: a lane tests eight positions of a row from one 8-byte read; needs windows narrower than a cell
// They differ in their prologue (where the keyframe's image comes from) and in how they find the corners inside the search window.  Everything else is written
// once, above them, and called by both: lane = pixel of the 8 x 8 key patch (only the used centre of the reference's 10 x 10 warp is formed; the patch never leaves
// registers), texture sums by wave reduction, hits scored one lane per candidate with V_SAD_U8 / V_DOT4_U32_U8, the winner the minimum ZNSSD with the reference's
// tie-break (first hit in QuadTree::query DFS order, strict '<') reproduced by a quadrant key computed only on ties (SURVEY.md B-3), the observation, the record.
// Also here: the readers of fast.hip's corner bitmap -- corner_bit (match_kernel), window_bits and span_mask (match_kernel2, and match_kernel3 in
// match_group.inc) -- and match_observation, the one step all three kernels share.

// DFS-order key of QuadTree::query (quadtree.h:510-544,693-708): recursive halving of the level
// box, x-quadrant bit above y-quadrant bit.  The reference decides a quadrant with
// rel = 1 - (x0 + w - p)/w < 0.5 in doubles; for integer p and box sizes W/2^d that test is exactly
// p < x0 + w/2 (all quantities are dyadic, the quotient is never within an ulp of 1/2), so the key
// is computed in 2^-12 fixed point with integer compares (tests/test_oracle_cpu.py checks the order
// against the real tree).
__device__ __forceinline__ unsigned quad_key(int px, int py, int W, int H) {
  int bx = 0, by = 0, bw = W << 12, bh = H << 12;
  const int X = px << 12, Y = py << 12;
  unsigned key = 0;
#pragma unroll
  for (int d = 0; d < 12; ++d) {
    bw >>= 1; bh >>= 1;
    const unsigned hx = X >= bx + bw, hy = Y >= by + bh;
    key = (key << 2) | (hx << 1) | hy;
    bx += hx ? bw : 0;
    by += hy ? bh : 0;
  }
  return key;
}

// ---- the wave-per-point steps ------------------------------------------------------------------------------------------------------------------------------
// warpAffinve (matcher.cpp:403-458): only the centre 8x8 of the reference's 10x10 warp is ever read (KEY_PATCH, matcher.cpp:376-381) and every warped
// pixel depends on its own coordinates alone: lane = pixel (row lane>>3, column lane&7) of that centre, one pass, the value stays in a register.
// (key_pixel_at: pixel (ix, iy) of the 10 x 10 warp, 0 .. 9 each -- the sub-pixel pass, match_subpix.inc, also forms the border)
__device__ __forceinline__ int key_pixel_at(const double *inv, const double *key_uv, const uint8_t *kimg, int kstride, int W, int H, int ix, int iy) {
  const double i00 = inv[0], i01 = inv[1], i10 = inv[2], i11 = inv[3];
  const double key_u = key_uv[0], key_v = key_uv[1];
  const double dx = ix - 5, dy = iy - 5;
  const double r0 = (i00 * dx + i01 * dy) + key_u;
  const double r1 = (i10 * dx + i11 * dy) + key_v;
  const double x = floor(r0), y = floor(r1);
  uint8_t val;
  if (!(x >= 0) || !(y >= 0) || x + 1 >= W || y + 1 >= H) val = 0;
  else {
    const double sx = r0 - x, sy = r1 - y;
    const double wx0 = 1 - sx, wx1 = sx, wy0 = 1 - sy, wy1 = sy;
    const int xi = (int)x, yi = (int)y;
    const double v00 = kimg[(size_t)yi * kstride + xi], v01 = kimg[(size_t)(yi + 1) * kstride + xi];
    const double v10 = kimg[(size_t)yi * kstride + xi + 1], v11 = kimg[(size_t)(yi + 1) * kstride + xi + 1];
    const double s = (wx0 * wy0) * v00 + (wx0 * wy1) * v01 + (wx1 * wy0) * v10 + (wx1 * wy1) * v11;
    val = (uint8_t)(s < 255. ? s : 255.);
  }
  return val;
}
__device__ __forceinline__ int key_pixel(const double *inv, const double *key_uv, const uint8_t *kimg, int kstride, int W, int H, int lane) {
  return key_pixel_at(inv, key_uv, kimg, kstride, W, H, (lane & 7) + 1, (lane >> 3) + 1);
}
// the key patch of a wave: its texture sums (wave-uniform) and the patch as 16 packed dwords (8 rows x 2), wave-uniform too
struct KeyPatch { int sumA, sumAA; uint32_t d[16]; };
// the texture sums of the patch; returns what the gate holds against thr_std^2 * 64 (matcher.cpp:376-381): below it the point is SVS_MATCH_TEXTURE
__device__ __forceinline__ int key_texture(int keyv, KeyPatch &K) {
  K.sumA = wave_sum(keyv); K.sumAA = wave_sum(keyv * keyv);
  return K.sumA * K.sumA - K.sumAA;
}
// the four bytes of a dword sit in four adjacent lanes (quad shuffles), lane 4i then holds dword i
__device__ __forceinline__ void key_pack(int keyv, KeyPatch &K) {
  const uint32_t kd = (uint32_t)keyv | ((uint32_t)__shfl_down(keyv, 1, 64) << 8) | ((uint32_t)__shfl_down(keyv, 2, 64) << 16) |
                      ((uint32_t)__shfl_down(keyv, 3, 64) << 24);
#pragma unroll
  for (int i = 0; i < 16; ++i) K.d[i] = (uint32_t)__builtin_amdgcn_readlane((int)kd, 4 * i);
}
// ZNSSD of the corner (hx, hy) of the current image against the key patch (computePatchScores / matchPatchZeroMeanSSD, matcher.cpp:42-96): one lane, 8 rows x 2
// unaligned dwords, sums with V_SAD_U8 / V_DOT4_U32_U8 against the wave-uniform key dwords -- no cross-lane reduction per candidate
__device__ __forceinline__ int znssd_at(const uint8_t *cimg, int cstride, int hx, int hy, const KeyPatch &K) {
  const uint8_t *p = cimg + (size_t)(hy - 4) * cstride + (hx - 4);
  uint32_t sB = 0, sBB = 0, sAB = 0;
#pragma unroll
  for (int r = 0; r < 8; ++r) {
    uint32_t v0, v1;
    __builtin_memcpy(&v0, p + (size_t)r * cstride, 4);
    __builtin_memcpy(&v1, p + (size_t)r * cstride + 4, 4);
    sB = __builtin_amdgcn_sad_u8(v0, 0u, sB); sB = __builtin_amdgcn_sad_u8(v1, 0u, sB);
    sBB = __builtin_amdgcn_udot4(v0, v0, sBB, false); sBB = __builtin_amdgcn_udot4(v1, v1, sBB, false);
    sAB = __builtin_amdgcn_udot4(v0, K.d[2 * r], sAB, false); sAB = __builtin_amdgcn_udot4(v1, K.d[2 * r + 1], sAB, false);
  }
  const int iB = (int)sB;
  return K.sumAA - 2 * (int)sAB - (int)sBB - (K.sumA * K.sumA - 2 * K.sumA * iB - iB * iB) / 64;
}
// the best corner so far: a lane's own while the window is scanned, the wave's after wave_winner
struct Best { int z = 0x7fffffff, x = 0, y = 0; };
// strict '<' in DFS order (matcher.cpp:173)  <=>  lexicographic min of (z, key); z must also beat thr_mean (init_dist).
// The quadrant key is only needed to break ties, so it is computed lazily (ties are rare).
__device__ __forceinline__ void best_take(Best &b, int z, int hx, int hy, int init_dist, int W, int H) {
  if (z < init_dist) {
    if (z < b.z) { b.z = z; b.x = hx; b.y = hy; }
    else if (z == b.z && quad_key(hx, hy, W, H) < quad_key(b.x, b.y, W, H)) { b.x = hx; b.y = hy; }
  }
}
// one window hit ((y << 16) | x, as the scans leave it in the wave's LDS list), scored by one lane.  (The loop that hands the list out, 64 hits at a time, stands
// in the kernels: as a helper that takes the list it cost both kernels a VGPR -- a fourth value carried round the loop.)
__device__ __forceinline__ void score_hit(int packed, const uint8_t *cimg, int cstride, const KeyPatch &K, int init_dist, int W, int H, Best &b) {
  const int hx = packed & 0xffff, hy = packed >> 16;
  best_take(b, znssd_at(cimg, cstride, hx, hy, K), hx, hy, init_dist, W, H);
}
// lexicographic min of (z, quadrant key) across the wave: minimum z first (6 shuffle steps); only if several lanes
// tie on it -- rare -- are their keys computed and compared; the winner's corner is read with readlane.  false: no lane has a corner
__device__ __forceinline__ bool wave_winner(Best &b, int W, int H) {
  int zmin = b.z;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) zmin = min(zmin, __shfl_xor(zmin, o, 64));
  const bool found = zmin != 0x7fffffff;
  if (found) {
    unsigned long long tie = __ballot(b.z == zmin);
    if (__popcll(tie) > 1) {
      unsigned k = b.z == zmin ? quad_key(b.x, b.y, W, H) : 0xffffffffu;
      unsigned kmin = k;
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) kmin = min(kmin, (unsigned)__shfl_xor((int)kmin, o, 64));
      tie = __ballot(b.z == zmin && k == kmin);
    }
    const int win = __ffsll((long long)tie) - 1;
    b.z = zmin;
    b.x = __builtin_amdgcn_readlane(b.x, win);
    b.y = __builtin_amdgcn_readlane(b.y, win);
  }
  return found;
}
// createObervation (matcher-impl.cpp:33-51) of the corner (bu, bv) of level lvl from the disparity image's value at it: (u, v, u_right) in level-0 pixels, the
// coordinates through f32 as the reference's Vector2f.  false: no disparity there (SVS_MATCH_NO_DISP), the observation is left alone.  All three kernels
__device__ __forceinline__ bool match_observation(int bu, int bv, int lvl, float disp, double &o0, double &o1, double &o2) {
  const double inv_factor = 1.0 / (double)(1 << lvl);
  const double d = disp * inv_factor;
  if (!(d > 0)) return false;
  const double sc = (double)(1 << lvl);
  const float fu_ = (float)bu, fv_ = (float)bv;
  o0 = fu_ * sc; o1 = fv_ * sc; o2 = (fu_ - d) * sc;
  return true;
}
// what a wave knows of its point's record; starts as "nothing found" with the prediction's status
struct WaveResult {
  int status, best, bu = 0, bv = 0;
  double obs[3] = {0, 0, 0}, xyz_actkey[3] = {0, 0, 0};
  __device__ WaveResult(int status_, int init_dist) : status(status_), best(init_dist) {}
};
// the tail of a textured point: SVS_MATCH_NONE without a winner, else the winner, its disparity (`disp`: the stream's image) and the observation, or SVS_MATCH_NO_DISP.
// (Scalars and plain pointers, here as in the steps above: with a reference to the kernel's argument block handed to a step, the compiler no longer
// proved the keyframe image of match_kernel to be global memory and read it with flat loads.)
__device__ __forceinline__ void wave_finish(const float *disp, int disp_stride, const double *xyz_actkey, int lvl, bool found, const Best &b, WaveResult &r) {
  r.xyz_actkey[0] = xyz_actkey[0]; r.xyz_actkey[1] = xyz_actkey[1]; r.xyz_actkey[2] = xyz_actkey[2];      // point in the active keyframe (match_predict_kernel)
  if (!found) r.status = SVS_MATCH_NONE;
  else {
    r.best = b.z; r.bu = b.x; r.bv = b.y;
    if (!match_observation(r.bu, r.bv, lvl, disp[(size_t)(r.bv << lvl) * disp_stride + (r.bu << lvl)], r.obs[0], r.obs[1], r.obs[2])) r.status = SVS_MATCH_NO_DISP;
  }
}
// the record, by lane 0
__device__ __forceinline__ void wave_write(svs_match_result *o, int lane, const WaveResult &w) {
  if (lane == 0) {
    svs_match_result r;
    r.status = w.status; r.u = w.bu; r.v = w.bv; r.znssd = w.best;
    r.obs[0] = w.obs[0]; r.obs[1] = w.obs[1]; r.obs[2] = w.obs[2];
    r.xyz_actkey[0] = w.xyz_actkey[0]; r.xyz_actkey[1] = w.xyz_actkey[1]; r.xyz_actkey[2] = w.xyz_actkey[2];
    *o = r;
  }
}

// ---- the corner bitmap of fast.hip (fast.hip, LevelDev): pixel (x, y) of cell column ci is bit x + gap * ci of row y; rows end in >= 8 zero bytes ----
typedef uint32_t U2 __attribute__((ext_vector_type(2)));
// one pixel (any x inside the image), the cell column found by compares: the general matcher, whose windows may be wider than a cell
__device__ __forceinline__ bool corner_bit(const uint8_t *row, int x, int cw, int gx, int gap) {
  int ci = 0;
  for (int q = 1; q < gx; ++q) ci += x >= q * cw;
  const int pb = x + gap * ci;
  return ((row[pb >> 3] >> (pb & 7)) & 1u) != 0u;
}
// up to 25 window positions x0 .. of one row, bit k = position x0 + k, from the 8 bytes `q` at byte pb_lo >> 3 of the row: pb_lo = the padded position of max(x0, 0),
// xb = the one cell-column boundary the positions may cross (windows narrower than a cell).  Positions left of the image read 0; the bits behind the window are the
// caller's to mask.
__device__ __forceinline__ uint32_t window_bits(U2 q, int pb_lo, int x0, int xb, int gap) {
  const unsigned long long raw = (((unsigned long long)q.y << 32) | q.x) >> (pb_lo & 7);
  const unsigned long long t = raw << min(max(-x0, 0), 63);      // (a window far left of the image: everything shifted out)
  // positions in front of the boundary; no boundary (xb = INT_MAX, last cell column) or one behind the window: all 32.  (Compared before subtracting: xb - x0 must not wrap.)
  const int nb = xb >= x0 + 32 ? 32 : max(xb - x0, 0);
  const uint32_t lowmask = nb >= 32 ? 0xffffffffu : (1u << nb) - 1u;
  return ((uint32_t)t & lowmask) | ((uint32_t)(t >> gap) & ~lowmask);
}
// bits of the positions x0 + k inside [xlo, xhi), k < n
__device__ __forceinline__ uint32_t span_mask(int x0, int n, int xlo, int xhi) {
  const int a = max(xlo - x0, 0), b = min(min(xhi - x0, n), 32);
  if (b <= a) return 0u;
  const uint32_t hi = b >= 32 ? 0xffffffffu : (1u << b) - 1u;
  return hi & ~((1u << a) - 1u);
}

// ---- match_kernel: the window is scanned position by position.  Hits are compacted into a per-wave LDS list; whenever it holds >= 64 corners (and at the end)
// they are scored
__global__ __launch_bounds__(256) void match_kernel(MatchParams M, svs_match_result *__restrict__ out) {
  __shared__ int s_cand[WAVES_PER_BLOCK][320];      // per-wave list of window hits waiting to be scored ((y << 16) | x): < 64 carried + <= 256 per trip
  const svs_match_args &A = M.a;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int ip = blockIdx.x * WAVES_PER_BLOCK + wave;
  const int slot = blockIdx.y;
  if (ip >= A.n_pts) return;                       // wave-uniform
  const PointPred pp = M.pred[(size_t)slot * A.n_pts + __builtin_amdgcn_readfirstlane(ip)];      // wave-uniform record
  svs_match_result *o = &out[(size_t)slot * A.out_bstride + ip];
  const int R = A.search_radius;
  const int init_dist = A.thr_mean * A.thr_mean * 64;
  WaveResult res(pp.status, init_dist);
  if (res.status == SVS_MATCH_OK) {
    // all 64 lanes work on the same point: wave-uniform (scalar) indices, the keyframe record and the per-level tables
    // are read with scalar loads
    const int kfi = __builtin_amdgcn_readfirstlane(pp.kfi);
    const int lvl = __builtin_amdgcn_readfirstlane(pp.lvl);
    const svs_keyframe *kfp = A.d_kfs + (size_t)slot * A.kf_bstride + kfi;
    const svs_cam cam = A.cam_vec[lvl];
    const int ui = pp.ui, vi = pp.vi;
    const int keyv = key_pixel(pp.inv, pp.key_uv, kfp->pyr[lvl], kfp->stride[lvl], cam.w, cam.h, lane);
    KeyPatch K;
    if (key_texture(keyv, K) < A.thr_std * A.thr_std * 64) res.status = SVS_MATCH_TEXTURE;
    else {
      const uint8_t *bm = M.fv.bm[lvl] + (size_t)slot * M.fv.bm_bstride[lvl];
      const int bm_stride = M.fv.bm_stride[lvl], gap = M.fv.bm_gap[lvl];
      const int gx = M.fv.gx[lvl], gy = M.fv.gy[lvl], cw = M.fv.cell_w[lvl], chh = M.fv.cell_h[lvl];
      const uint8_t *cimg = A.d_cur_pyr[lvl] + (size_t)slot * A.cur_bstride[lvl];
      const int cstride = A.cur_stride[lvl];
      const int side = 2 * R + 1;
      key_pack(keyv, K);
      Best b;                                        // per-lane running best
      int ncand = 0;                                 // wave-uniform fill of s_cand
      // a lane tests four horizontally adjacent window positions against the corner bitmap
      const int ngrp = (side + 3) >> 2, ntask = side * ngrp;
      const float inv_ngrp = 1.0f / (float)ngrp;
      const int xlo = 6, xhi = min(gx * cw, cam.w - 6), ylo = 6, yhi = min(gy * chh, cam.h - 6);      // isInFrame(uv, 6) and inside the cell grid
      for (int p0 = 0; p0 < ntask; p0 += 64) {
        const int task = p0 + lane;
        const bool valid = task < ntask;
        const int wy = (int)(((float)task + 0.5f) * inv_ngrp), g4 = 4 * (task - wy * ngrp);      // exact for task < 2^12
        const int cy = vi - R + wy, cx0 = ui - R + g4;
        const bool row_ok = valid && cy >= ylo && cy < yhi;
        const uint8_t *brow = bm + (size_t)(row_ok ? cy : 0) * bm_stride;
        int nh = 0;
        unsigned long long mk[4];
        bool hk[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const int cx = cx0 + k;
          hk[k] = row_ok && g4 + k < side && cx >= xlo && cx < xhi && corner_bit(brow, cx, cw, gx, gap);
          mk[k] = __ballot(hk[k]);
        }
        const unsigned long long lt = (1ull << lane) - 1ull;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          if (hk[k]) s_cand[wave][ncand + nh + __popcll(mk[k] & lt)] = (cy << 16) | (cx0 + k);
          nh += __popcll(mk[k]);
        }
        ncand += nh;
        const bool last = p0 + 64 >= ntask;
        if (ncand < 64 && !last) continue;                           // wave-uniform
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_s_waitcnt(0xc07f);
        for (int base = 0; base < ncand; base += 64)
          if (base + lane < ncand) score_hit(s_cand[wave][base + lane], cimg, cstride, K, init_dist, cam.w, cam.h, b);
        ncand = 0;
        __builtin_amdgcn_wave_barrier();
      }
      const bool found = wave_winner(b, cam.w, cam.h);
      wave_finish(A.d_disp + (size_t)slot * A.disp_bstride, A.disp_stride, pp.xyz_actkey, lvl, found, b, res);
    }
  }
  wave_write(o, lane, res);
}

// ---- match_kernel2 (round 3): the same matcher with a leaner window scan ----------------------------------------------------------------------------------
// match_kernel above spends ~45 % of its instructions in the scan of the (2R+1)^2 window: two trips of 64 tasks at four positions each, four
// ballots per trip, per-lane cell look-ups with loops over the grid.  Here a window is narrower than a cell, so a row segment meets at most one
// cell-column boundary; a lane tests EIGHT adjacent positions of a row from one 8-byte read (17 x 3 tasks = one trip
// at R = 8), and the sparse hits (~10 of 289) go to the per-wave list through an LDS counter (their order is irrelevant: the winner is the
// lexicographic minimum of (ZNSSD, quadrant key)).  The keyframe's image comes from the point's record, not from the keyframe's.
constexpr int CAND_CAP2 = 64 * 8;
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(8, 8))) void match_kernel2(MatchParams M, svs_match_result *__restrict__ out) {
  __shared__ int s_cand[WAVES_PER_BLOCK][CAND_CAP2];
  __shared__ int s_ncand[WAVES_PER_BLOCK];
  const svs_match_args &A = M.a;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int ip = blockIdx.x * WAVES_PER_BLOCK + wave;
  const int slot = blockIdx.y;
  if (ip >= A.n_pts) return;                       // wave-uniform
  const PointPred pp = M.pred[(size_t)slot * A.n_pts + __builtin_amdgcn_readfirstlane(ip)];      // wave-uniform record
  svs_match_result *o = &out[(size_t)slot * A.out_bstride + ip];
  const int R = A.search_radius;
  const int init_dist = A.thr_mean * A.thr_mean * 64;
  WaveResult res(pp.status, init_dist);
  if (res.status == SVS_MATCH_OK) {
    const int lvl = __builtin_amdgcn_readfirstlane(pp.lvl);
    const svs_cam cam = A.cam_vec[lvl];
    const int ui = __builtin_amdgcn_readfirstlane(pp.ui), vi = __builtin_amdgcn_readfirstlane(pp.vi);
    // ---- the first (at R <= 10: the only) trip of the window scan is requested NOW: its addresses depend on the prediction alone, so the bitmap
    // read travels together with the keyframe pixels of the warp below instead of behind the texture gate
    const uint8_t *bm = M.fv.bm[lvl] + (size_t)slot * M.fv.bm_bstride[lvl];
    const int bm_stride = M.fv.bm_stride[lvl], gap = M.fv.bm_gap[lvl];
    const int gx = M.fv.gx[lvl], gy = M.fv.gy[lvl], cw = M.fv.cell_w[lvl], chh = M.fv.cell_h[lvl];
    const int side = 2 * R + 1, x0 = ui - R, y0 = vi - R;
    const int xlo = 6, xhi = min(gx * cw, cam.w - 6), ylo = 6, yhi = min(gy * chh, cam.h - 6);      // isInFrame(uv, 6) and inside the cell grid
    const int nseg = (side + 7) >> 3, ntask = side * nseg;
    const float inv_nseg = 1.0f / (float)nseg;
    // a task = eight adjacent positions of a window row (cx0 .. cx0 + 7 of row cy): `hits` = their corner bits, from the 8 bytes of the row's bitmap at the segment's
    // first in-image column (the segment crosses at most one cell-column boundary); 0 for a task outside the window, the frame or the grid
    auto read8 = [&](int task, int &cy, int &cx0, uint32_t &hits) {
      const int wy = (int)(((float)task + 0.5f) * inv_nseg);      // exact for task < 2^12
      const int g8 = 8 * (task - wy * nseg);
      cy = y0 + wy; cx0 = x0 + g8;
      const bool row_ok = task < ntask && cy >= ylo && cy < yhi && cx0 < cam.w && cx0 + 8 > 0;
      hits = 0;
      if (row_ok) {
        const int xl = max(cx0, 0);
        int ci = 0;
        for (int q = 1; q < gx; ++q) ci += xl >= q * cw;
        const int pb = xl + gap * ci;
        const U2 w = ld_unaligned<U2>(bm + (size_t)cy * bm_stride + (pb >> 3));
        hits = window_bits(w, pb, cx0, ci + 1 < gx ? (ci + 1) * cw : 0x7fffffff, gap) & span_mask(cx0, min(8, side - g8), xlo, xhi);
      }
    };
    int cy_f, cx0_f; uint32_t hits_f;
    read8(lane, cy_f, cx0_f, hits_f);
    const int keyv = key_pixel(pp.inv, pp.key_uv, pp.kimg, pp.kstride, cam.w, cam.h, lane);
    KeyPatch K;
    if (key_texture(keyv, K) < A.thr_std * A.thr_std * 64) res.status = SVS_MATCH_TEXTURE;
    else {
      const uint8_t *cimg = A.d_cur_pyr[lvl] + (size_t)slot * A.cur_bstride[lvl];
      const int cstride = A.cur_stride[lvl];
      key_pack(keyv, K);
      Best b;                                        // per-lane running best
      for (int p0 = 0; p0 < ntask; p0 += 64) {
        if (lane == 0) s_ncand[wave] = 0;
        int cy = cy_f, cx0 = cx0_f; uint32_t hits = hits_f;
        if (p0) read8(p0 + lane, cy, cx0, hits);
        __builtin_amdgcn_wave_barrier();
        while (hits) {                                 // sparse: ~10 hits per window
          const int k = __ffs((int)hits) - 1;
          hits &= hits - 1;
          const int pos = atomicAdd(&s_ncand[wave], 1);
          s_cand[wave][pos] = (cy << 16) | (cx0 + k);
        }
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_s_waitcnt(0xc07f);
        const int ncand = s_ncand[wave];
        for (int base = 0; base < ncand; base += 64)
          if (base + lane < ncand) score_hit(s_cand[wave][base + lane], cimg, cstride, K, init_dist, cam.w, cam.h, b);
        __builtin_amdgcn_wave_barrier();
      }
      const bool found = wave_winner(b, cam.w, cam.h);
      wave_finish(A.d_disp + (size_t)slot * A.disp_bstride, A.disp_stride, pp.xyz_actkey, lvl, found, b, res);
    }
  }
  wave_write(o, lane, res);
}
