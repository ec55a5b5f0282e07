// match_group.inc -- the matcher with FOUR points per wave, the benchmark's kernel; included last by match.hip (window_bits, span_mask and match_observation are
// match_wave.inc's).  match_kernel3, with quad_less, row16_sum, M3Level and the two host-side bounds of its 24-bit offsets (k3_offsets_fit, k3_row_stride_max).
//
// With one wave per point (match_wave.inc) ~600 wave instructions go into a point, most of them with a handful of useful lanes: the scoring has
// one lane per candidate corner (2-10 of 64), the window scan two hits per 64 lanes, the 64-lane sums and the 16 readlanes of the key patch serve one
// point.  Here a point has a DPP row: 16 lanes = the 8 x 8 key patch as 16 dwords (lane = row, half), which is the layout V_SAD_U8 / V_DOT4_U32_U8
// want: a candidate costs one dword load and three dot products per lane and a 16-lane butterfly (quad_perm, row_half_mirror, row_mirror: DPP
// modifiers, no LDS); the key patch never moves; the (2R+1)^2 window is one row of the corner bitmap per lane (17 rows = 16 lanes + a shared last row: 17 bits of an
// 8-byte read).  Four points
// share every instruction.  Needs 2R+1 <= 17 (the reference's radii: 8 on the CPU build, 4 on the CUDA build); wider windows take match_kernel2.
// Its steps work on 16-lane groups and against a register budget of 8 waves per SIMD (tests/test_match_isa.py holds its assembly): they are its own, not the
// wave-per-point steps of match_wave.inc.

// quad_key(ax, ay) < quad_key(bx, by) without forming the keys: the two points share their box as long as their digits agree, so ONE box is halved until the
// digits differ (a rolled loop, a dozen registers: match_kernel3 calls it behind wave-uniform branches -- ties of the ZNSSD are rare -- and has no registers
// to spare for two unrolled key computations there)
__device__ __forceinline__ bool quad_less(int ax, int ay, int bx, int by, int W, int H) {
  int x0 = 0, y0 = 0, bw = W << 12, bh = H << 12;
  const int AX = ax << 12, AY = ay << 12, BX = bx << 12, BY = by << 12;
  bool less = false;
#pragma unroll 1
  for (int d = 0; d < 12; ++d) {
    bw >>= 1; bh >>= 1;
    const unsigned ahx = AX >= x0 + bw, ahy = AY >= y0 + bh, bhx = BX >= x0 + bw, bhy = BY >= y0 + bh;
    const unsigned da = (ahx << 1) | ahy, db = (bhx << 1) | bhy;
    if (da != db) { less = da < db; break; }
    x0 += ahx ? bw : 0;
    y0 += ahy ? bh : 0;
  }
  return less;
}

constexpr int M3_CAND_CAP = 17 * 17;
__device__ __forceinline__ uint32_t row16_sum(uint32_t v) {      // all-reduce over the 16 lanes of a DPP row
  v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0xB1, 0xf, 0xf, true);       // quad_perm [1,0,3,2]
  v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x4E, 0xf, 0xf, true);       // quad_perm [2,3,0,1]
  v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x141, 0xf, 0xf, true);      // row_half_mirror
  v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x140, 0xf, 0xf, true);      // row_mirror
  return v;
}
// A LevelTab row as match_kernel3 keeps it in the LDS: the block's stream already folded into the two bases (the stream is the same for the whole block, so
// stream * batch stride is scalar arithmetic, once per block), and the bound on a keyframe's row stride (MatchParams::k3_kmax)
struct alignas(16) M3Level {        // 64 bytes: a row's address is a shift of the level
  uint64_t bm, cimg;
  int32_t bm_stride, cstride, w, h;
  int32_t xhi, yhi, gap, kmax;
  int32_t pad_[4];
};
// The byte offsets inside a level image, a bitmap or the disparity image are 24-bit products (full rate; a 32 x 32 or 64-bit multiply-add is quarter rate) added to
// a 64-bit base once: rows and row strides stay below 2^24 and the image below 2^31 units of `unit` bytes, or svs_match refuses the call
bool k3_offsets_fit(int rows, int stride, int unit) {
  const int lim = 1 << 24;
  return rows > 0 && rows < lim && stride > 0 && stride < lim && (uint64_t)rows * (uint64_t)stride * (uint64_t)unit < (1ull << 31);
}
// a keyframe's images have the current frame's sizes, but their strides are in device memory: the kernel holds each against this bound and takes the byte path
// (64-bit offsets) for a stride above it
int32_t k3_row_stride_max(int rows) { return (int32_t)std::min<int64_t>((1 << 24) - 1, ((1ll << 31) - 1) / std::max(rows, 1)); }

__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(8, 8))) void match_kernel3(MatchParams M, svs_match_result *__restrict__ out) {
  __shared__ uint16_t s_cand[M3_GROUPS][M3_CAND_CAP + 7];      // per point: window positions (wy << 5 | wx) waiting to be scored
  __shared__ int s_ncand[M3_GROUPS];
  __shared__ uint32_t s_key[M3_GROUPS][16];                   // per point: the warped 8 x 8 key patch, 16 packed dwords
  __shared__ alignas(16) U2 s_pred[M3_GROUPS][16];            // per point: its PointPred, 8 bytes per lane
  __shared__ M3Level s_lvl[SVS_NUM_PYR_LEVELS];               // the level table, this block's stream folded in
  __shared__ int s_ip[M3_GROUPS];                             // per point: its index in the caller's list (kept here until the result is written, not in a register)
  const svs_match_args &A = M.a;
  const int sub = threadIdx.x & 15, grp = threadIdx.x >> 4;
  // the points of a stream come in image order (match_order_kernel): neighbouring blocks read neighbouring bitmap rows, key patches and image lines.  In XCD-contiguous
  // order an XCD works through whole streams and those lines meet in ONE L2
  unsigned wg = blockIdx.y * gridDim.x + blockIdx.x;
  if (M.swz) wg = xcd_contiguous(wg, gridDim.x * gridDim.y);
  const int ipos = (int)(wg % gridDim.x) * M3_GROUPS + grp;
  const unsigned slot = wg / gridDim.x;
  const bool live = ipos < A.n_pts;
  // ---- (0) the operands that are the same for the 16 lanes of a point, or for the block, go through the LDS once: the point's 128-byte record as ONE 8-byte request per
  // lane, the level table by one lane of the block.  Every later read of either is a broadcast ds_read: no 64-bit address, nothing on vmcnt, where the requests for
  // bitmap rows, key patch and pixels are counted (the kernel used to fetch each field with a vector load of its own, ~25 per wave).
  // One table per block behind ONE __syncthreads(), not a copy per wave: the barrier stands where the four waves have just started and wait for their record
  // anyway, and the table's scalar loads, moves and writes are issued once, not four times, in a kernel that is bound by instruction issue.
  const SVS_AS1 int32_t *order = (const SVS_AS1 int32_t *)M.order + (size_t)slot * (size_t)A.n_pts;
  const int ip = live && M.order ? order[(unsigned)ipos] : ipos;
  const SVS_AS1 uint8_t *pred = (const SVS_AS1 uint8_t *)M.pred + (size_t)slot * (size_t)A.n_pts * sizeof(PointPred);
  s_pred[grp][sub] = ld_unaligned<U2>(pred + ((unsigned)(live ? ip : A.n_pts - 1) * (unsigned)sizeof(PointPred) + 8u * sub));      // (n_pts < 2^24)
  if (threadIdx.x == 0) {
#pragma unroll
    for (int l = 0; l < SVS_NUM_PYR_LEVELS; ++l) {       // (rows behind n_levels: never written, never used)
      const LevelTab t = M.lt[l];
      // (the table's address is a kernel argument and nothing has written memory yet: scalar loads; `slot` is the block's: scalar multiplies.  The pad
      // words are not written)
      M3Level &v = s_lvl[l];
      v.bm = (uint64_t)t.bm + slot * t.bm_bstride; v.cimg = (uint64_t)t.cimg + slot * t.cur_bstride;
      v.bm_stride = t.bm_stride; v.cstride = t.cstride; v.w = t.w; v.h = t.h; v.xhi = t.xhi; v.yhi = t.yhi; v.gap = t.gap; v.kmax = M.k3_kmax[l];
    }
  }
  if (sub == 0) { s_ncand[grp] = 0; s_ip[grp] = ip; }
  __syncthreads();
  const SVS_AS3 PointPred *pp = (const SVS_AS3 PointPred *)&s_pred[grp][0];
  int status = pp->status;
  bool go = live && status == SVS_MATCH_OK;
  const int R = A.search_radius, side = 2 * R + 1;
  const int init_dist = A.thr_mean * A.thr_mean * 64;
  const int lvl = go ? pp->lvl : 0;
  const SVS_AS3 M3Level *Lp = (const SVS_AS3 M3Level *)&s_lvl[lvl];
  const int x0 = pp->ui - R, y0 = pp->vi - R;
  const int Lw = Lp->w, Lh = Lp->h;
  // The kernel is bound by instruction issue (profiles/match_staging.md) and short of registers at 8 waves per SIMD: wide requests, 24-bit offsets, and
  // values re-read from the staged point record / level table where they are needed rather than carried.  (Round 6, measured: carrying the bilinear
  // fractions from (2) to (4) instead of recomputing them -- 60 f64 instructions less, 80 VGPRs, 6 waves -- costs 0.05 ms per 512 x 2000 points: occupancy, not VALU.)
  // ---- (1) the window's corner-bitmap row of this lane and the 17th row (the same 8 bytes for the 16 lanes of the point: one request): 8-byte requests from the byte of the
  // window's first in-image column (fast.hip: a bit per pixel, cell columns on dword boundaries, rows padded with zeros)
  U2 w0 = {0u, 0u}, w1 = {0u, 0u};
  const int cy = y0 + sub, cyx = y0 + 16;
  {
    const SVS_AS1 uint8_t *bm = (const SVS_AS1 uint8_t *)Lp->bm + (unsigned)(pp->pb_lo >> 3);
    const int bm_stride = Lp->bm_stride, yhi = Lp->yhi;
    const bool col_ok = go && x0 < Lw;
    if (col_ok && sub < side && cy >= 6 && cy < yhi) w0 = ld_unaligned<U2>(bm + __umul24(cy, bm_stride));      // (rows 6 .. yhi: non-negative)
    if (col_ok && side > 16 && cyx >= 6 && cyx < yhi) w1 = ld_unaligned<U2>(bm + __umul24(cyx, bm_stride));
  }
  // ---- (2) warpAffinve, requests: the centre 8x8 of the 10x10 patch (KEY_PATCH, matcher.cpp:376-381), lane = (row, half): four pixels = one packed
  // dword.  The common case -- a warp close to a translation -- has the lane's four samples on one source row pair within 8 columns: two 8-byte
  // requests instead of sixteen single bytes; anything else takes the byte path.  px[]: the two 8-byte rows, or per pixel v00 | v10 << 8 | v01 << 16
  // | v11 << 24; flags: bit j = pixel j inside the image, bit 4 = row-pair case; offs: byte j = column offset of pixel j in the rows.
  const int prow = sub >> 1, pc0 = 4 * (sub & 1);
  uint32_t px0 = 0, px1 = 0, px2 = 0, px3 = 0, px4 = 0, px5 = 0, flags = 0, offs = 0;
  if (go) {
    const double i00 = pp->inv[0], i01 = pp->inv[1], i10 = pp->inv[2], i11 = pp->inv[3];
    const double key_u = pp->key_uv[0], key_v = pp->key_uv[1];
    const SVS_AS1 uint8_t *kimg = (const SVS_AS1 uint8_t *)pp->kimg;
    const int kstride = pp->kstride;
    const double dy = prow - 4;                    // iy - 5, iy = row + 1
    int xis[4], yis[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const double dx = pc0 + j - 4;
      const double r0 = (i00 * dx + i01 * dy) + key_u;
      const double r1 = (i10 * dx + i11 * dy) + key_v;
      const double x = floor(r0), y = floor(r1);
      const bool in = x >= 0 && y >= 0 && !(x + 1 >= Lw) && !(y + 1 >= Lh);
      flags |= in ? 1u << j : 0u;
      xis[j] = in ? (int)x : 0; yis[j] = in ? (int)y : 0;
    }
    // (round 4) the four samples may also straddle TWO source row pairs (a slightly rotated or scaled warp crosses a row boundary inside most waves: with the
    // row-pair case alone, one lane in 64 on the byte path made the whole wave issue its sixteen byte loads): three 8-byte rows y, y+1, y+2, and a bit per
    // pixel that says which pair is its own (flags bit 5 + j).  (A keyframe stride too wide for 32-bit offsets: the byte path, which forms them in 64 bits.)
    const int ymin = min(min(yis[0], yis[1]), min(yis[2], yis[3]));
    const bool oneRow = flags == 15u && (unsigned)(yis[0] - ymin) <= 1u && (unsigned)(yis[1] - ymin) <= 1u && (unsigned)(yis[2] - ymin) <= 1u &&
                        (unsigned)(yis[3] - ymin) <= 1u && (unsigned)(xis[1] - xis[0]) <= 6u && (unsigned)(xis[2] - xis[0]) <= 6u &&
                        (unsigned)(xis[3] - xis[0]) <= 6u && xis[0] + 8 <= Lw && (unsigned)(kstride - 1) < (unsigned)Lp->kmax;
    if (oneRow) {
      const SVS_AS1 uint8_t *q = kimg + (__umul24(ymin, kstride) + (unsigned)xis[0]);
      const U2 ra = ld_unaligned<U2>(q), rb = ld_unaligned<U2>(q + (unsigned)kstride), rc = ld_unaligned<U2>(q + ((unsigned)kstride << (ymin + 2 < Lh ? 1 : 0)));     // (row y+2 is only used by pixels on row y+1, whose y+2 is inside)
      px0 = ra.x; px1 = ra.y; px2 = rb.x; px3 = rb.y; px4 = rc.x; px5 = rc.y;
      flags |= 16u | (uint32_t)(yis[0] - ymin) << 5 | (uint32_t)(yis[1] - ymin) << 6 | (uint32_t)(yis[2] - ymin) << 7 | (uint32_t)(yis[3] - ymin) << 8;
      offs = (uint32_t)(xis[1] - xis[0]) << 8 | (uint32_t)(xis[2] - xis[0]) << 16 | (uint32_t)(xis[3] - xis[0]) << 24;
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (flags >> j & 1u) {
          const SVS_AS1 uint8_t *q = kimg + ((ptrdiff_t)yis[j] * kstride + xis[j]);
          const uint32_t t = (uint32_t)q[0] | (uint32_t)q[1] << 8 | (uint32_t)q[kstride] << 16 | (uint32_t)q[kstride + 1] << 24;
          if (j == 0) px0 = t; else if (j == 1) px1 = t; else if (j == 2) px2 = t; else px3 = t;
        }
    }
  }
  // ---- (3) hits of the window: the set bits of the lane's row inside [6, xhi) (isInFrame(uv, 6) and inside the cell grid).  Before the texture gate, whose verdict
  // only decides whether they are scored.
  {
    const int xb = pp->xb, pb_lo = pp->pb_lo, gap = Lp->gap;
    const uint32_t span = span_mask(x0, side, 6, Lp->xhi);
    uint32_t m = window_bits(w0, pb_lo, x0, xb, gap) & span;
    const uint32_t m17 = window_bits(w1, pb_lo, x0, xb, gap) & span;
    uint32_t ex = (m17 >> sub) & (sub == 15 ? 3u : 1u);      // the 17th row: lane = column, the last lane also the 17th column
    __builtin_amdgcn_wave_barrier();
    while (m) {
      const int k = __ffs((int)m) - 1;
      m &= m - 1;
      s_cand[grp][atomicAdd(&s_ncand[grp], 1)] = (uint16_t)((sub << 5) | k);
    }
    while (ex) {
      const int k = sub + ((ex & 1u) ? 0 : 1);
      ex &= ex - 1;
      s_cand[grp][atomicAdd(&s_ncand[grp], 1)] = (uint16_t)((16 << 5) | k);
    }
  }
  // ---- (3b) the pixels of the point's first 16 hits are requested NOW: their round trip runs under the bilinear arithmetic of (4), which reads the LDS and the key
  // patch's rows -- older requests, so that its one wait leaves these in flight (tools/match_isa.py reads that off the assembly).  A lane = a hit, eight 8-byte rows
  // from ONE running address -- the barrier keeps the compiler from forming eight addresses first: sixteen registers the kernel does not have at 8 waves per SIMD.
  // A hit lies inside [6, xhi) x [6, yhi): its patch's first row and column are non-negative, the offset a 24-bit product
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_s_waitcnt(0xc07f);
  const int cstride = Lp->cstride;
  const SVS_AS1 uint8_t *cimg = (const SVS_AS1 uint8_t *)Lp->cimg;
  // (FIRST rows only: all eight would cost sixteen registers across (4) that the kernel does not have)
  auto fetch16 = [&](int c0, int n_, int r_lo, int r_hi, U2 (&v)[8], int &wx, int &wy) __attribute__((always_inline)) {
    const bool act = c0 + sub < n_;
    const int code = act ? s_cand[grp][c0 + sub] : 0;
    wx = code & 31; wy = code >> 5;
    const SVS_AS1 uint8_t *q = cimg + (int)(__umul24(y0 - 4 + wy + r_lo, cstride) + (unsigned)(x0 - 4 + wx));
#pragma unroll
    for (int r = 0; r < 8; ++r)
      if (r >= r_lo && r < r_hi) v[r] = U2{0u, 0u};
    if (act) {
#pragma unroll
      for (int r = 0; r < 8; ++r)
        if (r >= r_lo && r < r_hi) {
          v[r] = ld_unaligned<U2>(q);
          q += cstride;
          asm volatile("" : "+v"(q));
        }
    }
  };
  constexpr int M3_PRE = 4;
  U2 v[8];
  int wx, wy;
  fetch16(0, go ? s_ncand[grp] : 0, 0, M3_PRE, v, wx, wy);
  // ---- (4) warpAffinve, arithmetic: the sample coordinates again (from the staged point record: 12 doubles not held across (3)), bilinear weights as the
  // reference forms them
  uint32_t keyd = 0;
  if (go) {
    const SVS_AS3 PointPred *pq = pp;
    asm volatile("" : "+v"(pq));
    const double i00 = pq->inv[0], i01 = pq->inv[1], i10 = pq->inv[2], i11 = pq->inv[3];
    const double key_u = pq->key_uv[0], key_v = pq->key_uv[1];
    const double dy = prow - 4;
    const bool oneRow = (flags & 16u) != 0u;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const double dx = pc0 + j - 4;
      const double r0 = (i00 * dx + i01 * dy) + key_u;
      const double r1 = (i10 * dx + i11 * dy) + key_v;
      const double sx = r0 - floor(r0), sy = r1 - floor(r1);
      uint32_t t = j == 0 ? px0 : j == 1 ? px1 : j == 2 ? px2 : px3;
      if (oneRow) {
        const uint32_t o = (offs >> (8 * j)) & 0xffu, sel = o | ((o + 1u) << 8) | 0x0c0c0000u;      // V_PERM: bytes o, o + 1 of an 8-byte row, zeros above
        const bool lower = (flags >> (5 + j) & 1u) != 0u;
        t = __builtin_amdgcn_perm(lower ? px3 : px1, lower ? px2 : px0, sel) | __builtin_amdgcn_perm(lower ? px5 : px3, lower ? px4 : px2, sel) << 16;
      }
      const double v00 = (double)(t & 0xffu), v10 = (double)(t >> 8 & 0xffu), v01 = (double)(t >> 16 & 0xffu), v11 = (double)(t >> 24);
      const double wx0 = 1 - sx, wx1 = sx, wy0 = 1 - sy, wy1 = sy;
      const double sv = (wx0 * wy0) * v00 + (wx0 * wy1) * v01 + (wx1 * wy0) * v10 + (wx1 * wy1) * v11;
      const uint32_t val = (flags >> j & 1u) ? (uint32_t)(uint8_t)(sv < 255. ? sv : 255.) : 0u;
      keyd |= val << (8 * j);
    }
  }
  const int sumA = (int)row16_sum(__builtin_amdgcn_sad_u8(keyd, 0u, 0u)), sumAA = (int)row16_sum(__builtin_amdgcn_udot4(keyd, keyd, 0u, false));
  if (go && __mul24(sumA, sumA) - sumAA < A.thr_std * A.thr_std * 64) { status = SVS_MATCH_TEXTURE; go = false; }
  const bool textured = go;
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_s_waitcnt(0xc07f);
  // ---- (5) ZNSSD of every hit, ONE LANE PER HIT (round 6): the 16 lanes of a point take 16 of its hits at a time, a lane sums its hit's whole 8 x 8 patch -- eight 8-byte
  // rows against the key rows, which all lanes of the point read from LDS (a broadcast) -- with six V_SAD_U8 / V_DOT4_U32_U8 per row and NO cross-lane step per hit; the
  // point's best is one 16-lane butterfly at the end.  (Rounds 3-5: two hits per step, lane = patch row, an 8-lane butterfly per pair of hits: ~55 wave instructions per
  // pair and as many steps as the busiest of the wave's four points has pairs -- 0.18 of the kernel's 0.49 ms at 512 x 2000 points.)  The first 16 hits' pixels were
  // requested in (3b).
  const int n = go ? s_ncand[grp] : 0;
  s_key[grp][sub] = keyd;                          // key rows: dwords 2 r, 2 r + 1 = row r
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_s_waitcnt(0xc07f);
  int best = 0x7fffffff, bu = 0, bv = 0;
  // (the first trip stands on its own in front of the loop: in ONE body the later trips, which request all eight rows, inherited the first trip's wait-count state
  // -- rows 0..3 pending from (3b) -- and waited for every one of their first four rows before they requested the next)
  auto score16 = [&](int c0) __attribute__((always_inline)) {
    const bool act = c0 + sub < n;
    uint32_t iBl = 0, sBB = 0, sAB = 0;
#pragma unroll
    for (int r = 0; r < 8; ++r) {
      const uint32_t k0 = s_key[grp][2 * r], k1 = s_key[grp][2 * r + 1];
      iBl = __builtin_amdgcn_sad_u8(v[r].y, 0u, __builtin_amdgcn_sad_u8(v[r].x, 0u, iBl));
      sBB = __builtin_amdgcn_udot4(v[r].y, v[r].y, __builtin_amdgcn_udot4(v[r].x, v[r].x, sBB, false), false);
      sAB = __builtin_amdgcn_udot4(v[r].y, k1, __builtin_amdgcn_udot4(v[r].x, k0, sAB, false), false);
    }
    const int iB = (int)iBl;
    // (sumA^2 - 2 sumA iB - iB^2 with sumA, iB <= 64 * 255: two 24-bit products, full rate, neither above 2^30 -- the same integer)
    const int z = sumAA - (int)(sBB + 2u * sAB) - (__mul24(sumA, sumA) - __mul24(iB, 2 * sumA + iB)) / 64;     // sBB + 2 sAB <= 3 * 64 * 255^2
    // strict '<' in DFS order (matcher.cpp:173)  <=>  lexicographic min of (z, quadrant key); z must also beat thr_mean.
    // The quadrant keys are only needed to break ties, which are rare: behind a wave-uniform branch, so that they are not evaluated (predicated) per hit.
    const int hx = x0 + wx, hy = y0 + wy;
    const bool good = act && z < init_dist;
    if (__ballot(good && z == best) != 0ull) {
      int hx_ = hx, bu_ = bu;
      asm volatile("" : "+v"(hx_), "+v"(bu_));      // (keeps the key arithmetic inside the branch: it is cheap enough for the compiler to speculate it)
      const SVS_AS3 M3Level *Lt = Lp;
      asm volatile("" : "+v"(Lt));                  // (the level's size from the table again: two registers not carried through the loop)
      if (good && z == best && quad_less(hx_, hy, bu_, bv, Lt->w, Lt->h)) { bu = hx; bv = hy; }
    }
    if (good && z < best) { best = z; bu = hx; bv = hy; }
  };
  if (__ballot(0 < n) != 0ull) {
    fetch16(0, n, M3_PRE, 8, v, wx, wy);                // the rest of the first 16 hits' rows
    score16(0);
    for (int c0 = 16; __ballot(c0 < n) != 0ull; c0 += 16) {      // (more than 16 hits: one point in twelve of the benchmark's)
      fetch16(c0, n, 0, 8, v, wx, wy);
      score16(c0);
    }
  }
  // the 16 lanes of the point meet: quad_perm [1,0,3,2], quad_perm [2,3,0,1], row_half_mirror, row_mirror -- after every step both partners hold the same winner
#define M3_MEET(CTRL)                                                                                                                                        \
  {                                                                                                                                                          \
    const int oz = __builtin_amdgcn_update_dpp(0, best, CTRL, 0xf, 0xf, true), ou = __builtin_amdgcn_update_dpp(0, bu, CTRL, 0xf, 0xf, true),                \
              ov = __builtin_amdgcn_update_dpp(0, bv, CTRL, 0xf, 0xf, true);                                                                                 \
    if (__ballot(oz == best && best != 0x7fffffff && (ou != bu || ov != bv)) != 0ull) {                                                                      \
      int ou_ = ou, bu_ = bu;                                                                                                                                \
      asm volatile("" : "+v"(ou_), "+v"(bu_));                                                                                                               \
      const SVS_AS3 M3Level *Lt = Lp;                                                                                                                        \
      asm volatile("" : "+v"(Lt));                                                                                                                           \
      if (oz == best && best != 0x7fffffff && quad_less(ou_, ov, bu_, bv, Lt->w, Lt->h)) { bu = ou; bv = ov; }                                               \
    }                                                                                                                                                        \
    if (oz < best) { best = oz; bu = ou; bv = ov; }                                                                                                          \
  }
  M3_MEET(0xB1) M3_MEET(0x4E) M3_MEET(0x141) M3_MEET(0x140)
#undef M3_MEET
  double obs0 = 0, obs1 = 0, obs2 = 0;
  const SVS_AS3 PointPred *pe = pp;
  asm volatile("" : "+v"(pe));        // (read here, not carried from the top of the kernel in registers the loop above needs)
  if (go) {
    if (best == 0x7fffffff) { status = SVS_MATCH_NONE; bu = bv = 0; }
    else {
      const int lvl = pe->lvl;
      const SVS_AS1 float *disp = (const SVS_AS1 float *)A.d_disp + slot * A.disp_bstride;
      if (!match_observation(bu, bv, lvl, disp[__umul24(bv << lvl, A.disp_stride) + (unsigned)(bu << lvl)], obs0, obs1, obs2)) status = SVS_MATCH_NO_DISP;
    }
  }
  if (live && sub == 0) {
    svs_match_result r;
    r.status = status; r.u = bu; r.v = bv; r.znssd = best == 0x7fffffff ? init_dist : best;
    r.obs[0] = obs0; r.obs[1] = obs1; r.obs[2] = obs2;
    r.xyz_actkey[0] = textured ? pe->xyz_actkey[0] : 0.0; r.xyz_actkey[1] = textured ? pe->xyz_actkey[1] : 0.0; r.xyz_actkey[2] = textured ? pe->xyz_actkey[2] : 0.0;
    out[slot * A.out_bstride + (unsigned)s_ip[grp]] = r;      // (a kernel argument: global memory to the compiler as it stands)
  }
}
