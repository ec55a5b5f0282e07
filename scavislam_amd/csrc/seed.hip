// seed.hip -- new-point seeding of a keyframe: StereoFrontend::addNewPoints / addMorePoints / addMorePointsToOtherFrame (stereo_frontend.cpp:682-823) for a batch
// of independent problems.  The reference walks the FAST corners of every level in the order of QuadTree::EquiIter and keeps a corner when its disparity is
// positive, it lies inside the border, its 3 x 3 cell still needs points and no tracked or already seeded point lies in its clearance window (isWindowEmpty,
// quadtree.h:713-754).  Given the visiting order that is a greedy whose every decision is an integer predicate (the header states it; tests/seed_model.py restates
// it); the order itself comes from third-party code (VisionTools::Sample::uniform), so it is an INPUT here: the caller's index lists, or one generated from a seed.
// Two launches:
//   seed_order_kernel   (levels, problems) workgroups: the generated order.  Every corner's key (round j, hash b, cell c) has a closed-form rank -- corners of
//                       earlier rounds are sum_c' min(n_c', j), the cells in front of it in its round are counted -- so nothing is sorted
//   seed_greedy_kernel  one workgroup per problem: the levels' occupancy bitmaps (1 bit per pixel; the window bounds are integers, so the test is exact on floor(p))
//                       live in LDS, one wave per level walks its order in chunks of 64 (lane = corner; conflicts inside a chunk are resolved in visiting order by
//                       ballots), the taken corners wait in LDS until the levels' counts meet, then ids and the reversed (push_front) positions are known and the
//                       records leave as 16-byte stores.  No global atomics, no waiting between workgroups.
// Not pinned by the reference's binaries (its EquiIter needs VisionTools): the yardstick is tests/seed_model.py, which tests/test_seed_cpu.py holds against the
// reference's compiled quadtree and against the points the reference seeded in the sequence fixtures.
#include "seed.h"
#include <algorithm>

namespace {
constexpr int SEED_THREADS = 256;
constexpr int SEED_ORDER_MAX = 8192;            // corners per level the generated order can rank (their hashes live in LDS)
constexpr size_t SEED_LDS_MAX = 150 * 1024;

struct SeedStash { int16_t x, y; float d; };    // a taken corner until the levels' counts meet

struct SeedK {
  svs_seed_args a;
  SeedFrontendSrc fs; bool from_frontend;
  int32_t *gen; size_t gen_b; int gen_off[3];   // generated orders: level l of problem r at gen + r * gen_b + gen_off[l]
  int R, nmp, min_pts, n_levels;
  int third_w, twothird_w, third_h, twothird_h;
  int LW[3], LH[3], wpr[3], bm_off[3], bm_dwords;      // level images, bitmap rows in dwords, bitmap offsets in dwords
  int stash_off[3];                             // in SeedStash entries behind the bitmaps
  svs_candidate_point *out; int cap; int32_t *n_new;
};

__device__ __forceinline__ uint64_t seed_key_a(uint64_t seed, int l, int i) { return splitmix64(seed ^ ((1ull << 62) | ((uint64_t)l << 32) | (uint32_t)i)); }
__device__ __forceinline__ uint64_t seed_key_b(uint64_t seed, int l, int j, int c) {
  return splitmix64(seed ^ ((2ull << 62) | ((uint64_t)l << 48) | ((uint64_t)(uint32_t)j << 16) | (uint32_t)c));
}
__device__ __forceinline__ int seed_list_len(const SeedK &K, int l, size_t slot) {
  return min(max(K.a.d_n[l][slot * K.a.n_bstride[l]], 0), K.a.xy_cap[l]);
}

// grid (levels, problems).  Dynamic LDS: 8 bytes per corner of the longest list.  A list whose cell counts do not add up to its length keeps the rest in its last cell
__global__ __launch_bounds__(SEED_THREADS) void seed_order_kernel(SeedK K) {
  extern __shared__ uint64_t s_a[];
  __shared__ int s_start[SVS_MAX_CELLS + 1];
  const int l = blockIdx.x, r = blockIdx.y, tid = threadIdx.x;
  const svs_seed_problem &P = K.a.d_prob[r];
  if (P.use_order || !K.a.d_cell_count[l]) return;
  const size_t slot = K.fs.slot_of ? (size_t)K.fs.slot_of[r] : (size_t)r;
  const int n = min(seed_list_len(K, l, slot), SEED_ORDER_MAX), nc = K.a.n_cells[l];
  if (tid == 0) {
    const int32_t *cc = K.a.d_cell_count[l] + slot * K.a.cell_bstride[l];
    int run = 0;
    for (int c = 0; c < nc; ++c) { s_start[c] = run; run = min(run + max(cc[c], 0), n); }
    s_start[nc] = n;
  }
  const uint64_t seed = P.seed;
  for (int i = tid; i < n; i += SEED_THREADS) s_a[i] = seed_key_a(seed, l, i);
  __syncthreads();
  int32_t *ord = K.gen + (size_t)r * K.gen_b + K.gen_off[l];
  for (int i = tid; i < n; i += SEED_THREADS) {
    int c = 0;
    while (c + 1 < nc && i >= s_start[c + 1]) ++c;
    const uint64_t ai = s_a[i];
    int j = 0;
    for (int k = s_start[c]; k < s_start[c + 1]; ++k) { const uint64_t ak = s_a[k]; j += (ak < ai || (ak == ai && k < i)) ? 1 : 0; }
    const uint64_t bi = seed_key_b(seed, l, j, c);
    int pos = 0;
    for (int c2 = 0; c2 < nc; ++c2) {
      const int n2 = s_start[c2 + 1] - s_start[c2];
      pos += min(n2, j);
      if (n2 > j && c2 != c) { const uint64_t b2 = seed_key_b(seed, l, j, c2); pos += (b2 < bi || (b2 == bi && c2 < c)) ? 1 : 0; }
    }
    ord[pos] = i;      // the keys are distinct, so pos is a permutation of [0, n)
  }
}

// is any bit of the window [x - R, x + R] x [y - R, y + R], clipped to the level image, set?  (x, y) inside the image
__device__ __forceinline__ bool seed_window_occupied(const uint32_t *bm, int wpr, int LW, int LH, int x, int y, int R) {
  const int x0 = max(x - R, 0), x1 = min(x + R, LW - 1), y0 = max(y - R, 0), y1 = min(y + R, LH - 1);
  const int d0 = x0 >> 5, d1 = x1 >> 5;
  uint32_t any = 0;
  for (int yy = y0; yy <= y1; ++yy)
    for (int d = d0; d <= d1; ++d) {
      uint32_t m = ~0u;
      if (d == d0) m &= ~0u << (x0 & 31);
      if (d == d1) m &= ~0u >> (31 - (x1 & 31));
      any |= bm[yy * wpr + d] & m;
    }
  return any != 0;
}

// a corner of the visiting order with everything steps 1-3 need; ok = it passed the border test and dv is its disparity sample
struct SeedCorner { int x, y; float dv; bool ok; };
__device__ __forceinline__ SeedCorner seed_fetch(const SeedK &K, int l, int k, int n_vis, const int32_t *ord, const int16_t *xy, int n_list, const float *disp) {
  SeedCorner c{0, 0, 0.f, false};
  if (k < n_vis) {
    const int idx = ord[k];
    if ((unsigned)idx < (unsigned)n_list) {
      uint32_t pk;
      __builtin_memcpy(&pk, xy + 2 * (size_t)idx, 4);
      c.x = (int16_t)(pk & 0xffffu); c.y = (int16_t)(pk >> 16);
      const int ux = c.x * (1 << l), uy = c.y * (1 << l);
      if (ux >= 1 && ux < K.a.cam.w - 1 && uy >= 1 && uy < K.a.cam.h - 1 && c.x < K.LW[l] && c.y < K.LH[l]) {      // isInFrame(uvi, 1); nothing outside the image is read
        c.dv = disp[(size_t)uy * K.a.disp_stride + ux];
        c.ok = true;
      }
    }
  }
  return c;
}

// grid = problems, 4 waves: all lanes clear and fill the bitmaps, wave l walks level l, all lanes write the records.  Dynamic LDS: bitmaps, then the stashes
__global__ __launch_bounds__(SEED_THREADS) void seed_greedy_kernel(SeedK K) {
  extern __shared__ uint32_t s_mem[];
  __shared__ int s_cnt[3];
  const int r = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const svs_seed_problem &P = K.a.d_prob[r];
  const size_t slot = K.fs.slot_of ? (size_t)K.fs.slot_of[r] : (size_t)r;
  SeedStash *stash = reinterpret_cast<SeedStash *>(s_mem + K.bm_dwords);
  for (int i = tid; i < K.bm_dwords; i += SEED_THREADS) s_mem[i] = 0u;
  if (tid < 3) s_cnt[tid] = 0;
  __syncthreads();
  {      // the point tree: floor(p) of every tree point inside its level image
    const int nt = K.from_frontend ? min(max(P.n_tree, 0), (int)K.fs.rec_b) : (int)min((size_t)max(P.n_tree, 0), K.a.tree_bstride);
    for (int i = tid; i < nt; i += SEED_THREADS) {
      double px, py; int lv;
      if (K.from_frontend) {
        const size_t q = slot * K.fs.rec_b + i;
        if (K.fs.res[q].status != SVS_MATCH_OK || !K.fs.gated[q].accepted) continue;
        px = K.fs.gated[q].uv_pyr[0]; py = K.fs.gated[q].uv_pyr[1]; lv = K.fs.pts[q].anchor_level;
      } else {
        const size_t q = (size_t)r * K.a.tree_bstride + i;
        px = K.a.d_tree_xy[2 * q]; py = K.a.d_tree_xy[2 * q + 1]; lv = K.a.d_tree_level[q];
      }
      if (lv < 0 || lv >= K.n_levels) continue;
      if (!(px >= 0.0 && px < (double)K.LW[lv] && py >= 0.0 && py < (double)K.LH[lv])) continue;      // (NaN too)
      const int ix = (int)px, iy = (int)py;
      atomicOr(&s_mem[K.bm_off[lv] + iy * K.wpr[lv] + (ix >> 5)], 1u << (ix & 31));
    }
  }
  __syncthreads();
  if (wave < K.n_levels) {
    const int l = wave;
    const bool from_stats = K.from_frontend && P.n0[0] < 0;
    const svs_point_stats *st = from_stats ? K.fs.stats + slot : nullptr;
    unsigned flags = 0;
    for (int k = 0; k < 9; ++k) flags |= (from_stats ? (st->num_points_grid3x3[k] <= K.min_pts) : (P.add_flags[k] != 0)) ? 1u << k : 0u;
    const int n_start = max(from_stats ? st->num_matched_points[l] : P.n0[l], 0), cap_l = K.nmp >> l;
    int rem = max(cap_l - n_start, 0) + 1;      // corners the level may still take: ++n; if (n > cap) break
    const int n_list = seed_list_len(K, l, slot);
    const int16_t *xy = K.a.d_xy[l] + slot * K.a.xy_bstride[l];
    const float *disp = K.a.d_disp + slot * K.a.disp_bstride;
    const int32_t *ord = nullptr; int n_vis = 0;
    if (P.use_order) {
      if (K.a.d_order[l]) { ord = K.a.d_order[l] + (size_t)r * K.a.order_bstride[l]; n_vis = (int)min((size_t)max(P.n_order[l], 0), K.a.order_bstride[l]); }
    } else if (K.gen && K.a.d_cell_count[l]) { ord = K.gen + (size_t)r * K.gen_b + K.gen_off[l]; n_vis = min(n_list, SEED_ORDER_MAX); }
    uint32_t *bm = s_mem + K.bm_off[l];
    const int wpr = K.wpr[l], LW = K.LW[l], LH = K.LH[l], R = K.R;
    SeedStash *my = stash + K.stash_off[l];
    const double inv = 1.0 / (double)(1 << l);
    int cnt = 0;
    SeedCorner nxt = seed_fetch(K, l, lane, n_vis, ord, xy, n_list, disp);
    for (int base = 0; base < n_vis && rem > 0; base += 64) {
      const SeedCorner c = nxt;
      nxt = seed_fetch(K, l, base + 64 + lane, n_vis, ord, xy, n_list, disp);      // the next chunk's disparities are on their way while this one is resolved
      bool pass = c.ok && (double)c.dv * inv > 0.0;                                 // interpolateDisparity > 0 (NaN compares false)
      if (pass) {
        const int ux = c.x << l, uy = c.y << l;
        const int i3 = ux < K.third_w ? 0 : (ux < K.twothird_w ? 1 : 2), j3 = uy < K.third_h ? 0 : (uy < K.twothird_h ? 1 : 2);
        pass = (flags >> (i3 * 3 + j3)) & 1u;
      }
      unsigned long long pending = __ballot(pass);
      while (pending && rem > 0) {
        const bool mine = (pending >> lane) & 1ull;
        const bool blocked = mine && seed_window_occupied(bm, wpr, LW, LH, c.x, c.y, R);      // the bitmap only grows: blocked once is blocked for good
        const unsigned long long cand = __ballot(mine && !blocked);
        if (!cand) break;
        // the first candidate that lies in the window of an EARLIER candidate of the chunk ends the prefix that can be taken at once
        bool conf = false;
        for (unsigned long long m = cand; m; m &= m - 1) {
          const int j = __ffsll(m) - 1;
          const int xj = __shfl(c.x, j, 64), yj = __shfl(c.y, j, 64);
          conf = conf || (lane > j && abs(c.x - xj) <= R && abs(c.y - yj) <= R);
        }
        const unsigned long long cm = __ballot(conf && ((cand >> lane) & 1ull));
        const unsigned long long acc = cm ? cand & ((1ull << (__ffsll(cm) - 1)) - 1ull) : cand;      // (the lowest candidate never conflicts: acc != 0)
        const int rank = __popcll(acc & ((1ull << lane) - 1ull));
        if (((acc >> lane) & 1ull) && rank < rem) {      // the cap cuts the prefix
          atomicOr(&bm[c.y * wpr + (c.x >> 5)], 1u << (c.x & 31));
          my[cnt + rank] = SeedStash{(int16_t)c.x, (int16_t)c.y, c.dv};
        }
        const int na = min(__popcll(acc), rem);
        cnt += na; rem -= na;
        pending = cand & ~acc;
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");      // the bits set above are seen by the re-test of the rest
      }
    }
    if (lane == 0) s_cnt[l] = cnt;
  }
  __syncthreads();
  const int c0 = s_cnt[0], c1 = s_cnt[1], c2 = s_cnt[2], total = c0 + c1 + c2;
  const double *T = P.T_newkey_from_cur;
  const svs_cam cam = K.a.cam;
  for (int k = tid; k < total; k += SEED_THREADS) {      // k = position in the order the corners were taken in, level 0 first
    const int l = k < c0 ? 0 : (k < c0 + c1 ? 1 : 2), s = k - (l == 0 ? 0 : (l == 1 ? c0 : c0 + c1));
    const SeedStash e = stash[K.stash_off[l] + s];
    const double fac = (double)(1 << l), d = (double)e.d * (1.0 / fac);
    const double p0 = (double)e.x, p1 = (double)e.y, p2 = p0 - d;
    const double u0 = p0 * fac, u1 = p1 * fac, u2 = p2 * fac;      // zeroFromPyr_3d
    const double sd = (u0 - u2) / cam.b, z = cam.f / sd;           // unmap_uvu, stereo_camera.cpp:46-52
    const double x = ((u0 - cam.cx) / cam.f) * z, y = ((u1 - cam.cy) / cam.f) * z;
    // pose_act's rows (pose.h), spelled out here: through the helper the compiler schedules the tail of this kernel differently (profiles/shared_helpers.md)
    const double X = ((T[0] * x + T[1] * y) + T[2] * z) + T[3], Y = ((T[4] * x + T[5] * y) + T[6] * z) + T[7], Z = ((T[8] * x + T[9] * y) + T[10] * z) + T[11];
    const int pos = total - 1 - k;                                 // push_front
    if (pos < K.cap) {
      double2 *o = reinterpret_cast<double2 *>(K.out + (size_t)r * K.cap + pos);
      o[0] = make_double2(X, Y); o[1] = make_double2(Z, p0); o[2] = make_double2(p1, p2);
      reinterpret_cast<int4 *>(o)[3] = make_int4(l, P.kf_index, P.first_point_id + k, 0);
    }
  }
  if (tid < 3) K.n_new[(size_t)r * 3 + tid] = s_cnt[tid];
}
}  // namespace

extern "C" void svs_seed_params_default(svs_seed_params *p) {
  if (!p) return;
  p->clearance = 2; p->num_max_points = 300; p->min_num_points = 25; p->n_levels = 3;
}

int svs_seed_max_records(const svs_seed_params *prm) {
  int n = 0;
  for (int l = 0; l < prm->n_levels; ++l) n += (prm->num_max_points >> l) + 1;
  return n;
}

int svs_seed_launch(svs_ctx *ctx, const svs_seed_args *a, const svs_seed_params *prm, const SeedFrontendSrc *fs, bool any_generated, svs_candidate_point *d_out, int cap,
                    int32_t *d_n_new) {
  SVS_REQUIRE(ctx, ctx && a && prm && d_out && d_n_new && a->batch >= 0);
  SVS_REQUIRE(ctx, prm->n_levels >= 1 && prm->n_levels <= SVS_NUM_PYR_LEVELS && prm->clearance >= 0 && prm->clearance <= 31 && prm->num_max_points >= 0 &&
                       prm->num_max_points <= 65536);
  SVS_REQUIRE(ctx, a->cam.w >= 3 && a->cam.h >= 3 && a->cam.w <= 16384 && a->cam.h <= 16384 && a->cam.f > 0.0 && a->cam.b > 0.0);
  SVS_REQUIRE(ctx, a->d_disp && a->disp_stride >= a->cam.w && a->d_prob && (reinterpret_cast<uintptr_t>(d_out) & 15) == 0);
  SVS_REQUIRE(ctx, fs || !a->d_tree_xy == !a->d_tree_level);
  if (cap < svs_seed_max_records(prm)) {
    ctx->err = "svs_seed: output capacity below the sum over the levels of (num_max_points >> l) + 1";
    return SVS_ERR_CAPACITY;
  }
  SeedK K{};
  K.a = *a;
  if (fs) { K.fs = *fs; K.from_frontend = true; }
  if (!fs && !a->d_tree_xy) K.a.tree_bstride = 0;      // no tree points
  K.R = prm->clearance; K.nmp = prm->num_max_points; K.min_pts = prm->min_num_points; K.n_levels = prm->n_levels;
  {      // the reference's float products truncated to int (stereo_frontend.cpp:738-742)
    const float third = 1. / 3.;
    K.third_w = a->cam.w * third; K.third_h = a->cam.h * third;
    K.twothird_w = a->cam.w * 2 * third; K.twothird_h = a->cam.h * 2 * third;
  }
  size_t gen_b = 0, order_lds = 0;
  int dwords = 0, stash = 0;
  for (int l = 0; l < prm->n_levels; ++l) {
    SVS_REQUIRE(ctx, a->d_xy[l] && a->d_n[l] && a->xy_cap[l] >= 0);
    K.LW[l] = (a->cam.w + (1 << l) - 1) >> l; K.LH[l] = (a->cam.h + (1 << l) - 1) >> l;
    K.wpr[l] = (K.LW[l] + 31) / 32; K.bm_off[l] = dwords; dwords += K.LH[l] * K.wpr[l];
    K.stash_off[l] = stash; stash += (prm->num_max_points >> l) + 1;
    if (any_generated && a->d_cell_count[l]) {
      SVS_REQUIRE(ctx, a->n_cells[l] >= 1 && a->n_cells[l] <= SVS_MAX_CELLS);
      if (a->xy_cap[l] > SEED_ORDER_MAX) { ctx->err = "svs_seed: a generated order ranks at most 8192 corners per level"; return SVS_ERR_CAPACITY; }
      K.gen_off[l] = (int)gen_b; gen_b += (size_t)a->xy_cap[l];
      order_lds = std::max(order_lds, (size_t)a->xy_cap[l] * sizeof(uint64_t));
    }
  }
  K.bm_dwords = dwords;
  const size_t lds = (size_t)dwords * 4 + (size_t)stash * sizeof(SeedStash);
  if (lds > SEED_LDS_MAX) { ctx->err = "svs_seed: the levels' occupancy bitmaps do not fit in LDS"; return SVS_ERR_UNSUPPORTED; }
  K.out = d_out; K.cap = cap; K.n_new = d_n_new;
  if (a->batch == 0) return SVS_OK;
  SVS_DEVICE(ctx);
  if (gen_b) {
    void *buf = nullptr;
    if (int rc = svs_ctx_match_scratch(ctx, gen_b * sizeof(int32_t) * (size_t)a->batch, &buf)) return rc;      // per-call tables, as the matcher's: stream order protects them
    K.gen = static_cast<int32_t *>(buf); K.gen_b = gen_b;
    if (order_lds > 32 * 1024)
      SVS_HIP(ctx, hipFuncSetAttribute(reinterpret_cast<const void *>(&seed_order_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)order_lds));
    hipLaunchKernelGGL(seed_order_kernel, dim3(prm->n_levels, a->batch), dim3(SEED_THREADS), order_lds, ctx->stream, K);
    SVS_LAUNCH_CHECK(ctx);
  }
  if (lds > 32 * 1024)
    SVS_HIP(ctx, hipFuncSetAttribute(reinterpret_cast<const void *>(&seed_greedy_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  hipLaunchKernelGGL(seed_greedy_kernel, dim3(a->batch), dim3(SEED_THREADS), lds, ctx->stream, K);
  SVS_LAUNCH_CHECK(ctx);
  return SVS_OK;
}

extern "C" int svs_seed_points(svs_ctx *ctx, const svs_seed_args *a, const svs_seed_params *prm, svs_candidate_point *d_out, int cap, int32_t *d_n_new) {
  SVS_REQUIRE(ctx, ctx && a && prm);
  bool gen = false;
  for (int l = 0; l < SVS_NUM_PYR_LEVELS; ++l) gen = gen || a->d_cell_count[l];
  return svs_seed_launch(ctx, a, prm, nullptr, gen, d_out, cap, d_n_new);
}
