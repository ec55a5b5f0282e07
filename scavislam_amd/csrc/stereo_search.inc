// stereo_search.inc -- part of stereo.hip: the disparity search (findStereoCorrespondenceBM) and the left-right check
//   stereo_bm_kernel<SMALL>       32 disparities: a wave = 64 output columns x a strip of rows, the window's seven rows of row SADs in a register ring
//   stereo_bm_wide_kernel         16 .. 160 disparities: the window sums of a lane's column in LDS, a run-time loop over groups of 16 disparities
//   stereo_bm_edge_kernel<LANES>  the never-searched left border and the 3 leftmost output columns, whose right-image window clamps before the shift
//   stereo_validate_kernel        validateDisparity: a wave per image row, one LDS atomicMin of (cost, x) per source pixel
typedef unsigned short us2 __attribute__((ext_vector_type(2)));
union Pk { uint64_t q; us2 h[2]; uint32_t u[2]; };

// ---- the end of findStereoCorrespondenceBM's inner loop, shared by every selection below.  How a site finds minsad, mind, the neighbours p = sad[mind + 1] and
// n = sad[mind - 1] (mirrored ends: sad[-1] = sad[1], sad[N] = sad[N-2]) and a rival outside [mind-1, mind+1] with sad <= bm_thresh is its own business.
__device__ __forceinline__ bool bm_textured(int tsum, const StereoDev &S) { return tsum >= S.texthr; }
__device__ __forceinline__ int bm_thresh(int minsad, const StereoDev &S) { return minsad + (minsad * S.uniq / 100); }
// num / den of C (towards zero) without the 30-instruction integer division: |num| < 2^24 and den < 2^15 are exact floats, the product with the reciprocal is
// within 0.4 of the quotient, one step up or down on the integer remainder makes it exact
__device__ __forceinline__ int div_trunc_small(int num, int den) {      // |num| < 2^24, 0 < den < 2^15
  const int a = abs(num);
  int q = (int)((float)a * __builtin_amdgcn_rcpf((float)den));
  const int rem = a - q * den;
  q += rem >= den ? 1 : (rem < 0 ? -1 : 0);
  return num < 0 ? -q : q;
}
// the 16-bit disparity of the winner: parabola step through (n, minsad, p), rounded to 1/16.  A window sum is at most 49 * 126 (cap 63), so dd < 2^15 and
// |p - n| * 256 < 2^24 at every site and key width: div_trunc_small is exact.
__device__ __forceinline__ int16_t bm_subpixel(int minsad, int mind, int p, int n, int N) {
  const int dd = p + n - 2 * minsad + abs(p - n);
  return (int16_t)(((N - mind - 1) * 256 + (dd != 0 ? div_trunc_small((p - n) * 256, dd) : 0) + 15) >> 4);
}

// the window bytes one lane needs from one image row: 7 left bytes (8th masked) and 44 right bytes
struct RowWin { uint32_t l0, l1, r[11]; };
__device__ __forceinline__ RowWin load_rowwin(const uint8_t *lrow, const uint8_t *rrow) {
  RowWin wv;
  wv.l0 = ld_unaligned<uint32_t>(lrow);
  wv.l1 = ld_unaligned<uint32_t>(lrow + 4);
#pragma unroll
  for (int k = 0; k < 11; ++k) wv.r[k] = ld_unaligned<uint32_t>(rrow + 4 * k);
  return wv;
}
// horizontal 7-tap SADs of one row for the 32 disparity indices (4 per V_QSAD/V_MQSAD pair) + texture term
__device__ __forceinline__ void row_sads(const RowWin &wv, uint32_t ft4, Pk (&hh)[8], int &t) {
  const uint32_t l1 = wv.l1 & 0x00ffffffu;      // byte 7 = 0 = masked out by MQSAD
#pragma unroll
  for (int g = 0; g < 8; ++g) {
    const uint64_t hq = __builtin_amdgcn_qsad_pk_u16_u8((uint64_t)wv.r[g] | ((uint64_t)wv.r[g + 1] << 32), wv.l0, 0ull);
    hh[g].q = __builtin_amdgcn_mqsad_pk_u16_u8((uint64_t)wv.r[g + 1] | ((uint64_t)wv.r[g + 2] << 32), l1, hq);
  }
  t = (int)__builtin_amdgcn_sad_u8(l1 | (ft4 & 0xff000000u), ft4, __builtin_amdgcn_sad_u8(wv.l0, ft4, 0u));
}

// per-lane LDS scratch of bm_select; a union, so that the halfword and dword views may alias
union SelScr { uint32_t u[17]; unsigned short s[34]; };
// winner selection of one pixel from its 32 window SADs (findStereoCorrespondenceBM inner loop).  Dynamic indexing
// (sad[mind +- 1], masking the winner's neighbourhood) goes through the per-lane LDS scratch.
template <bool SMALL>      // SMALL: every SAD < 4096 (prefilter cap <= 41)
__device__ __forceinline__ void bm_select(const Pk (&sad)[8], int tsum, const StereoDev &S, SelScr &scr, int16_t &disp, uint16_t &cost) {
  disp = (int16_t)FILTERED16; cost = 0;
  int minsad, mind;
  if (SMALL) {      // 49 taps x |difference| <= 2 cap: every SAD < 4096, so a 16-bit KEY holds sad << 4 | dword index and both halves of the 16 dwords are searched
    us2 m = {0xffff, 0xffff};      // at once; first minimum wins within a half, d = 2 * index + half.  The kernel keeps its running sums AS keys (the index rides in the four
#pragma unroll                   // low bits, which the shifted row SADs never touch): the search is sixteen packed minima
    for (int g = 0; g < 8; ++g)
#pragma unroll
      for (int j = 0; j < 2; ++j) m = __builtin_elementwise_min(m, sad[g].h[j]);
    const int s0 = m.x >> 4, d0 = 2 * (m.x & 15), s1 = m.y >> 4, d1 = 2 * (m.y & 15) + 1;
    const bool first = s0 < s1 || (s0 == s1 && d0 < d1);
    minsad = first ? s0 : s1; mind = first ? d0 : d1;
  } else {
    uint32_t best = 0xffffffffu;
#pragma unroll
    for (int g = 0; g < 8; ++g) {      // first minimum wins: key = sad * 32 + d
      best = min(best, ((sad[g].u[0] & 0xffffu) << 5) | (uint32_t)(4 * g));
      best = min(best, ((sad[g].u[0] >> 16) << 5) | (uint32_t)(4 * g + 1));
      best = min(best, ((sad[g].u[1] & 0xffffu) << 5) | (uint32_t)(4 * g + 2));
      best = min(best, ((sad[g].u[1] >> 16) << 5) | (uint32_t)(4 * g + 3));
    }
    minsad = (int)(best >> 5); mind = (int)(best & 31);
  }
  if (!bm_textured(tsum, S)) return;
#pragma unroll
  for (int g = 0; g < 8; ++g) { scr.u[2 * g] = sad[g].u[0]; scr.u[2 * g + 1] = sad[g].u[1]; }
  unsigned short *s16 = scr.s;
  constexpr int KS = SMALL ? 4 : 0;      // the scratch holds keys (SMALL) or plain sums
  const int p = s16[mind == NDISP - 1 ? NDISP - 2 : mind + 1] >> KS, n = s16[mind == 0 ? 1 : mind - 1] >> KS;
  if (S.uniq > 0) {
    // the scan of the original stops at a d outside [mind-1, mind+1] with sad[d] <= thresh: mask those three, take the min
    const int thresh = bm_thresh(minsad, S);
    s16[mind] = 0xffff;
    s16[mind == 0 ? 32 : mind - 1] = 0xffff;            // slots 32/33 = spare halfword pair
    s16[mind == NDISP - 1 ? 33 : mind + 1] = 0xffff;
    us2 m = {0xffff, 0xffff};
#pragma unroll
    for (int k = 0; k < 16; ++k) { Pk t; t.u[0] = scr.u[k]; m = __builtin_elementwise_min(m, t.h[0]); }
    if ((int)(min(m.x, m.y) >> KS) <= thresh) return;      // (keys: a masked slot reads 4095 >= every real sum, and 29 real sums are always in the minimum)
  }
  disp = bm_subpixel(minsad, mind, p, n, NDISP);
  cost = (uint16_t)minsad;
}

// grid: (ceil((width1-3)/64), ceil(h/BM_STRIP), batch), block 64.  Output columns x in [3, width1), X = x + 31.
// The vertical 7-row sum slides down the strip: the entering row's 32 SADs are added, the leaving row's are subtracted.  The six rows
// of the window live in a register ring (7 slots x 16 VGPRs, slot = row mod 7: the entering row y+3 is computed straight into the slot
// the row that left one step earlier freed; the loop is unrolled by seven so that the slots are static) -- one V_QSAD / V_MQSAD pass and one row window load per output row
// instead of two (round 2 recomputed the leaving row); the next step's row window is loaded as soon as the current one is consumed.
template <bool SMALL>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(3))) void stereo_bm_kernel(StereoDev S) {
  __shared__ SelScr s_scr[64];
  // column neighbours share 44 of their right-image bytes per row, strip neighbours six rows: an XCD works through whole frames (xcd_contiguous), so those lines
  // are fetched into one L2
  unsigned wg = (blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x;
  if (S.swz) wg = xcd_contiguous(wg, gridDim.x * gridDim.y * gridDim.z);
  const int bx = wg % gridDim.x, by = (wg / gridDim.x) % gridDim.y;
  const int lane = threadIdx.x, b = wg / (gridDim.x * gridDim.y);
  const int w = S.w, h = S.h, width1 = w - NDISP + 1;
  const int x = min(3 + bx * 64 + lane, width1 - 1);      // lanes past the end redo the last column (no store)
  const bool store = 3 + bx * 64 + lane < width1;
  const int y0 = by * BM_STRIP, y1 = min(y0 + BM_STRIP, h);
  const uint8_t *lp = S.lp + (size_t)b * h * S.pitch + PADL + (NDISP - 1) - WSZ2;      // uniform bases + one 32-bit lane offset for both images
  const uint8_t *rp = S.rp + (size_t)b * h * S.pitch + PADL - WSZ2;
  const uint32_t ft4 = 0x01010101u * (uint32_t)(S.cap + 1);
  auto win = [&](int r) { const uint32_t o = (uint32_t)min(max(r, 0), h - 1) * (uint32_t)S.pitch + (uint32_t)x; return load_rowwin(lp + o, rp + o); };
  constexpr int NR = 2 * WSZ2 + 1;      // ring slots = window rows
  Pk sad[8], ring[NR][8];
  int tring[NR];
  // SMALL: the running sums are kept as the selection's KEYS, sum << 4 | dword index (bm_select): the index is put in once, the row SADs enter and leave shifted
  // (one packed shift per dword of the entering row instead of a shift and an OR per dword of every selection)
#pragma unroll
  for (int g = 0; g < 8; ++g) { sad[g].u[0] = SMALL ? 0x00010001u * (uint32_t)(2 * g) : 0u; sad[g].u[1] = SMALL ? 0x00010001u * (uint32_t)(2 * g + 1) : 0u; }
  auto as_keys = [](Pk (&r)[8]) __attribute__((always_inline)) {
    if (SMALL) {
#pragma unroll
      for (int g = 0; g < 8; ++g) { r[g].h[0] <<= 4; r[g].h[1] <<= 4; }
    }
  };
  int tsum = 0;
#pragma unroll
  for (int j = 0; j < NR - 1; ++j) {      // rows y0-3 .. y0+2 of the first window
    const RowWin wv = win(y0 - WSZ2 + j);
    row_sads(wv, ft4, ring[j], tring[j]);
    as_keys(ring[j]);
#pragma unroll
    for (int g = 0; g < 8; ++g) { sad[g].h[0] += ring[j][g].h[0]; sad[g].h[1] += ring[j][g].h[1]; }
    tsum += tring[j];
  }
  RowWin wa = win(y0 + WSZ2);
  for (int yb = y0; yb < y1; yb += NR) {
#pragma unroll
    for (int k = 0; k < NR; ++k) {      // step k: row y+3 enters into the free slot (k + 6) % 7, row y-3 leaves from slot k, which is free then
      const int y = yb + k;
      if (y < y1) {      // (uniform)
        const int in = (k + NR - 1) % NR;
        row_sads(wa, ft4, ring[in], tring[in]);
        as_keys(ring[in]);
        wa = win(y + WSZ2 + 1);      // next step's row: issued as soon as this step's is consumed, in flight during the selection
#pragma unroll
        for (int g = 0; g < 8; ++g) { sad[g].h[0] += ring[in][g].h[0]; sad[g].h[1] += ring[in][g].h[1]; }
        tsum += tring[in];
        int16_t d16; uint16_t c16;
        bm_select<SMALL>(sad, tsum, S, s_scr[lane], d16, c16);
        if (store) {
          const size_t o = ((size_t)b * h + y) * w + x + (NDISP - 1);
          S.disp16[o] = d16; S.cost[o] = c16;
        }
#pragma unroll
        for (int g = 0; g < 8; ++g) { sad[g].h[0] -= ring[k][g].h[0]; sad[g].h[1] -= ring[k][g].h[1]; }
        tsum -= tring[k];
      }
    }
  }
}

// ---- the search for any numberOfDisparities N = 16, 32, ..., 160 (the kernels above are the N = 32 case) ----------
// Seven rows of N row SADs per lane do not fit the register file (7 x N/2 VGPRs), so the ring goes: a lane keeps the N WINDOW sums of its column in LDS and
// slides them down the strip by adding the entering row's SADs and subtracting the leaving row's, both formed again from the images (two V_QSAD / V_MQSAD passes
// per output row instead of one).  The sums lie lane-major, two disparities per dword: dword k of lane l at [k * 64 + l], so that the 64 lanes of a wave touch 64
// consecutive dwords whichever k they share -- N x 128 bytes per wave, 20 KB at N = 160.  Disparities are worked through in groups of 16 by a runtime loop (one
// kernel for every N): a group needs six dwords of the right row, of which it inherits two from the group before and loads four as one 16-byte load, issued a
// group ahead.  The first minimum is found while the sums are updated, on 32-bit keys sum << 8 | d (13 bits of sum at cap 63, 8 bits of index); the uniqueness
// scan is a second pass over the sums in LDS.
typedef unsigned short __attribute__((may_alias)) lds_u16;      // halfword view of the dword sums

__device__ __forceinline__ uint64_t u64_of(uint32_t lo, uint32_t hi) { return (uint64_t)lo | ((uint64_t)hi << 32); }
// the part of an image row one lane's window needs, walked group by group: 7 left bytes (8th masked), the right row's two inherited dwords and the group's four
struct WideRow {
  uint32_t l0, l1, c0, c1;
  uint4 nx;
  const uint8_t *r;
  __device__ __forceinline__ void open(const uint8_t *lrow, const uint8_t *rrow) {
    l0 = ld_unaligned<uint32_t>(lrow); l1 = ld_unaligned<uint32_t>(lrow + 4) & 0x00ffffffu;      // byte 7 = 0 = masked out by MQSAD
    c0 = ld_unaligned<uint32_t>(rrow); c1 = ld_unaligned<uint32_t>(rrow + 4);
    nx = ld_unaligned<uint4>(rrow + 8);
    r = rrow + 24;
  }
  __device__ __forceinline__ int texture(uint32_t ft4) const { return (int)__builtin_amdgcn_sad_u8(l1 | (ft4 & 0xff000000u), ft4, __builtin_amdgcn_sad_u8(l0, ft4, 0u)); }
  // horizontal 7-tap SADs of disparity indices 16 g .. 16 g + 15; more: another group follows (its four dwords are requested here)
  __device__ __forceinline__ void group(int g, bool more, Pk (&hh)[4]) {
    const uint32_t a[6] = {c0, c1, nx.x, nx.y, nx.z, nx.w};
    c0 = nx.z; c1 = nx.w;
    if (more) nx = ld_unaligned<uint4>(r + 16 * g);      // (uniform)
#pragma unroll
    for (int u = 0; u < 4; ++u)
      hh[u].q = __builtin_amdgcn_mqsad_pk_u16_u8(u64_of(a[u + 1], a[u + 2]), l1, __builtin_amdgcn_qsad_pk_u16_u8(u64_of(a[u], a[u + 1]), l0, 0ull));
  }
};
// one step of a lane's window sums (sums: the lane's column, stride 64 dwords): + row A, - row B (SUB); SEL: best = the first minimum's key.  No half of a dword
// carries or borrows: a sum stays within [0, 49 * 126].
template <bool SUB, bool SEL>
__device__ __forceinline__ void wide_step(uint32_t *sums, int ngroups, uint32_t ft4, const uint8_t *la, const uint8_t *ra, const uint8_t *lb, const uint8_t *rb,
                                          int &tsum, uint32_t &best) {
  WideRow A, B;
  A.open(la, ra);
  tsum += A.texture(ft4);
  if (SUB) { B.open(lb, rb); tsum -= B.texture(ft4); }
  best = 0xffffffffu;
  for (int g = 0; g < ngroups; ++g) {
    Pk ha[4], hb[4];
    A.group(g, g + 1 < ngroups, ha);
    if (SUB) B.group(g, g + 1 < ngroups, hb);
    uint32_t *sg = sums + g * 8 * 64;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      uint32_t v = sg[k * 64] + ha[k >> 1].u[k & 1];
      if (SUB) v -= hb[k >> 1].u[k & 1];
      sg[k * 64] = v;
      if (SEL) {
        const uint32_t d = (uint32_t)(16 * g + 2 * k);
        best = min(best, ((v & 0xffffu) << 8) | d);
        best = min(best, ((v >> 16) << 8) | (d + 1));
      }
    }
  }
}
// the rest of findStereoCorrespondenceBM's inner loop for one pixel, from its N sums in LDS and the first minimum's key
__device__ __forceinline__ void wide_select(uint32_t *sums, uint32_t best, int tsum, const StereoDev &S, int16_t &disp, uint16_t &cost) {
  disp = (int16_t)FILTERED16; cost = 0;
  if (!bm_textured(tsum, S)) return;
  const int N = S.ndisp, minsad = (int)(best >> 8), mind = (int)(best & 255u);
  lds_u16 *s16 = reinterpret_cast<lds_u16 *>(sums);
  auto slot = [](int d) { return (d >> 1) * 128 + (d & 1); };      // halfword of disparity index d in the lane's column
  const int p = s16[slot(mind == N - 1 ? N - 2 : mind + 1)], n = s16[slot(mind == 0 ? 1 : mind - 1)];
  if (S.uniq > 0) {
    // the scan of the original stops at a d outside [mind-1, mind+1] with sad[d] <= thresh: mask those three, take the minimum, put them back (the sums slide on)
    const int thresh = bm_thresh(minsad, S);
    s16[slot(mind)] = 0xffff;
    if (mind > 0) s16[slot(mind - 1)] = 0xffff;
    if (mind < N - 1) s16[slot(mind + 1)] = 0xffff;
    us2 m = {0xffff, 0xffff};
#pragma unroll 8
    for (int k = 0; k < (N >> 1); ++k) { Pk t; t.u[0] = sums[k * 64]; m = __builtin_elementwise_min(m, t.h[0]); }
    s16[slot(mind)] = (unsigned short)minsad;
    if (mind > 0) s16[slot(mind - 1)] = (unsigned short)n;
    if (mind < N - 1) s16[slot(mind + 1)] = (unsigned short)p;
    if ((int)min(m.x, m.y) <= thresh) return;      // (at least 13 real sums are in the minimum, so a thresh >= 0xffff changes nothing)
  }
  disp = bm_subpixel(minsad, mind, p, n, N);
  cost = (uint16_t)minsad;
}
// grid: (ceil((width1-3)/WIDE_TILE), ceil(h/WIDE_STRIP), batch), block 64, dynamic LDS = N * 128 bytes.  Output columns x in [3, width1), X = x + N - 1.
// With T(y) the window sums of output row y (window rows clamped one by one), T(y) = T(y-1) + row(clamp(y+3)) - row(clamp(y-4)) holds for every y, T(y0-1)
// included: a strip starts from the seven rows of T(y0-1) and then takes one step per output row.
// Reads of a row: right bytes x-3 .. x+N+4 and left bytes x+N-4 .. x+N+3 with x <= w-N, all inside the padded row (PADL 16, PADR 48).
__global__ __launch_bounds__(64) void stereo_bm_wide_kernel(StereoDev S) {
  extern __shared__ uint32_t w_sums[];      // [N/2][64]
  unsigned wg = (blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x;
  if (S.swz) wg = xcd_contiguous(wg, gridDim.x * gridDim.y * gridDim.z);
  const int bx = wg % gridDim.x, by = (wg / gridDim.x) % gridDim.y;
  const int lane = threadIdx.x, b = wg / (gridDim.x * gridDim.y);
  const int w = S.w, h = S.h, N = S.ndisp, ngroups = N >> 4, width1 = w - N + 1;
  const int x = min(3 + bx * WIDE_TILE + lane, width1 - 1);      // lanes past the end redo the last column (no store)
  const bool store = 3 + bx * WIDE_TILE + lane < width1;
  const int y0 = by * WIDE_STRIP, y1 = min(y0 + WIDE_STRIP, h);
  const uint8_t *lp = S.lp + (size_t)b * h * S.pitch + PADL + (N - 1) - WSZ2 + x;
  const uint8_t *rp = S.rp + (size_t)b * h * S.pitch + PADL - WSZ2 + x;
  const uint32_t ft4 = 0x01010101u * (uint32_t)(S.cap + 1);
  auto row = [&](int r) { return (uint32_t)min(max(r, 0), h - 1) * (uint32_t)S.pitch; };
  uint32_t *sums = w_sums + lane;
  for (int k = 0; k < (N >> 1); ++k) sums[k * 64] = 0u;
  int tsum = 0;
  uint32_t best;
  for (int j = 0; j < 2 * WSZ2 + 1; ++j) {      // T(y0 - 1)
    const uint32_t o = row(y0 - 1 - WSZ2 + j);
    wide_step<false, false>(sums, ngroups, ft4, lp + o, rp + o, nullptr, nullptr, tsum, best);
  }
  for (int y = y0; y < y1; ++y) {
    const uint32_t oa = row(y + WSZ2), ob = row(y - WSZ2 - 1);
    wide_step<true, true>(sums, ngroups, ft4, lp + oa, rp + oa, lp + ob, rp + ob, tsum, best);
    int16_t d16; uint16_t c16;
    wide_select(sums, best, tsum, S, d16, c16);
    if (store) {
      const size_t o = ((size_t)b * h + y) * w + x + (N - 1);
      S.disp16[o] = d16; S.cost[o] = c16;
    }
  }
}

// ---- the left edge of either search: columns X < N - 1 (never searched: FILTERED) and x in [0,3), whose right-image window clamps at column 0 BEFORE the disparity
// shift (so it is not a contiguous byte window).  LANES lanes per pixel, lane = disparity index within a chunk of 64: 32 lanes (half a wave) for the 32 disparities
// of stereo_bm_kernel, a wave and up to three chunks for stereo_bm_wide_kernel's run-time N.  What the three columns of EDGE_ROWS rows read is staged once with
// aligned dword loads, per image row ybase-3 .. ybase+EDGE_ROWS+2 a record of the right bytes 0 .. N+7 (N/4 + 2 dwords) and the left bytes N-4 .. N+7 (3 dwords).
// x <= 2 and d <= N-1: the right index is at most N+4 < w, so neither image clamps on the right.
// grid: (ceil(h/EDGE_ROWS), batch), block EDGE_THREADS, dynamic LDS = wide_edge_lds_bytes(N)
constexpr int WIDE_EDGE_CHUNKS = (WIDE_MAX_NDISP + 63) / 64;
// SAD of the 7 x 7 window of column x at disparity index d = 4 q + sh, from the records of its seven rows (rec: the first, rec_n dwords each).
// A window row: left bytes x+N-4 .. x+N+2 (8th byte masked); right bytes max(x + dx, 0) + d for dx = -3..3 -- the clamp repeats column d, so the seven taps are a
// byte shuffle (V_PERM) of the bytes d .. d+7
__device__ __forceinline__ uint32_t edge_window_sad(const uint32_t *rec, int rec_n, int q, int sh, int x) {
  const uint32_t selA = x == 0 ? 0x00000000u : x == 1 ? 0x01000000u : 0x02010000u;      // taps dx = -3..0
  const uint32_t selB = x == 0 ? 0x0c030201u : x == 1 ? 0x0c040302u : 0x0c050403u;      // taps dx = 1..3, then a zero byte
  uint32_t sad_u = 0;
#pragma unroll
  for (int k = 0; k <= 2 * WSZ2; ++k, rec += rec_n) {
    const uint32_t w0 = rec[q], w1 = rec[q + 1], w2 = rec[q + 2], a0 = rec[rec_n - 3], a1 = rec[rec_n - 2], a2 = rec[rec_n - 1];
    const uint32_t r0 = __builtin_amdgcn_alignbyte(w1, w0, sh), r1 = __builtin_amdgcn_alignbyte(w2, w1, sh);
    const uint32_t l0 = __builtin_amdgcn_alignbyte(a1, a0, x), l1 = __builtin_amdgcn_alignbyte(a2, a1, x) & 0x00ffffffu;
    sad_u = __builtin_amdgcn_sad_u8(l1, __builtin_amdgcn_perm(r1, r0, selB), __builtin_amdgcn_sad_u8(l0, __builtin_amdgcn_perm(r1, r0, selA), sad_u));
  }
  return sad_u;
}
// texture sum of the same window (left image only; the same for every disparity).  A function of its own: with the sum folded into edge_window_sad behind a flag
// the 64-lane kernel was given 70 VGPRs instead of 63 (7 waves per SIMD instead of 8)
__device__ __forceinline__ uint32_t edge_window_texture(const uint32_t *rec, int rec_n, int x, uint32_t ft4) {
  uint32_t tsum_u = 0;
#pragma unroll
  for (int k = 0; k <= 2 * WSZ2; ++k, rec += rec_n) {
    const uint32_t a0 = rec[rec_n - 3], a1 = rec[rec_n - 2], a2 = rec[rec_n - 1];
    const uint32_t l0 = __builtin_amdgcn_alignbyte(a1, a0, x), l1 = __builtin_amdgcn_alignbyte(a2, a1, x) & 0x00ffffffu;
    tsum_u = __builtin_amdgcn_sad_u8(l1 | (ft4 & 0xff000000u), ft4, __builtin_amdgcn_sad_u8(l0, ft4, tsum_u));
  }
  return tsum_u;
}
template <int LANES>
__global__ __launch_bounds__(EDGE_THREADS) void stereo_bm_edge_kernel(StereoDev S) {
  static_assert(LANES == 32 || LANES == 64, "half a wave or a wave per pixel");
  constexpr int CHUNKS = LANES == 32 ? 1 : WIDE_EDGE_CHUNKS;
  extern __shared__ uint32_t e_rec[];      // [EDGE_ROWS + 6][rec_n]
  const int b = blockIdx.y, w = S.w, h = S.h, N = LANES == 32 ? NDISP : S.ndisp, tid = threadIdx.x;
  const int sub = tid & (LANES - 1), base = tid & 63 & ~(LANES - 1);      // lane within the pixel's group; the group's first lane within the wave
  const int nr = N / 4 + 2, rec_n = nr + 3;
  const int width1 = w - N + 1, ncol = min(3, width1);
  const int ybase = blockIdx.x * EDGE_ROWS, nrow = min(EDGE_ROWS, h - ybase);
  const uint8_t *lp = S.lp + (size_t)b * h * S.pitch + PADL, *rp = S.rp + (size_t)b * h * S.pitch + PADL;      // (PADL, the pitch and N are multiples of 4)
  for (int i = tid; i < (nrow + 2 * WSZ2) * rec_n; i += EDGE_THREADS) {
    const int r = i / rec_n, c = i - r * rec_n, yy = min(max(ybase - WSZ2 + r, 0), h - 1);
    e_rec[i] = *reinterpret_cast<const uint32_t *>((c < nr ? rp + 4 * c : lp + (N - 4) + 4 * (c - nr)) + (size_t)yy * S.pitch);
  }
  for (int i = tid; i < (N - 1) * nrow; i += EDGE_THREADS) {      // the never-searched left border, FILTERED
    const size_t o = ((size_t)b * h + ybase + i / (N - 1)) * w + i % (N - 1);
    S.disp16[o] = (int16_t)FILTERED16; S.cost[o] = 0;
  }
  __syncthreads();
  const uint32_t ft4 = 0x01010101u * (uint32_t)(S.cap + 1);
  for (int pix = tid / LANES; pix < ncol * nrow; pix += EDGE_THREADS / LANES) {
    const int yl = pix / ncol, x = pix - yl * ncol, y = ybase + yl;
    const uint32_t *rec = e_rec + yl * rec_n;      // the window's first row
    const int tsum = (int)edge_window_texture(rec, rec_n, x, ft4);
    int sadc[CHUNKS];
    uint32_t key = 0xffffffffu;
#pragma unroll
    for (int c = 0; c < CHUNKS; ++c) {
      sadc[c] = 0x7fffffff;
      if (64 * c < N) {      // (uniform)
        const int d = 64 * c + sub, dr = min(d, N - 1);      // lanes past N - 1 redo it and stay out of the selection
        const uint32_t sad_u = edge_window_sad(rec, rec_n, dr >> 2, dr & 3, x);
        if (d < N) { sadc[c] = (int)sad_u; key = min(key, (sad_u << 8) | (uint32_t)d); }      // first minimum wins: key = sad << 8 | d
      }
    }
    // selection across the pixel's lanes (bm_select / wide_select on one lane)
#pragma unroll
    for (int o = LANES / 2; o > 0; o >>= 1) key = min(key, (uint32_t)__shfl_xor((int)key, o, 64));
    const int minsad = (int)(key >> 8), mind = (int)(key & 255u);
    const int ip = mind == N - 1 ? N - 2 : mind + 1, in = mind == 0 ? 1 : mind - 1;
    const int thresh = bm_thresh(minsad, S);
    int p = 0, n = 0;
    bool rival = false;
#pragma unroll
    for (int c = 0; c < CHUNKS; ++c) {
      const int vp = __shfl(sadc[c], base + (ip & 63), 64), vn = __shfl(sadc[c], base + (in & 63), 64), d = 64 * c + sub;
      if ((ip >> 6) == c) p = vp;
      if ((in >> 6) == c) n = vn;
      const unsigned long long rivals = __ballot(sadc[c] <= thresh && d < N && (d < mind - 1 || d > mind + 1));
      rival = rival || ((rivals >> base) & (~0ull >> (64 - LANES))) != 0ull;
    }
    if (sub == 0) {
      int16_t d16 = (int16_t)FILTERED16; uint16_t c16 = 0;
      if (bm_textured(tsum, S) && !(S.uniq > 0 && rival)) { d16 = bm_subpixel(minsad, mind, p, n, N); c16 = (uint16_t)minsad; }
      const size_t o = ((size_t)b * h + y) * w + x + (N - 1);
      S.disp16[o] = d16; S.cost[o] = c16;
    }
  }
}

// validateDisparity (with D2): one WAVE per image row, four rows per workgroup (a row is 640 pixels: a 256-lane workgroup per row spent
// its time in dispatch and two workgroup barriers; a wave orders its own LDS traffic without them).  The reference's sequential first
// pass ("a strictly smaller cost wins", ascending x => first x on ties) is a minimum over (cost, x): every valid source pixel does one
// LDS atomicMin of the packed key (cost << 16 | x) on its target column.  grid: (ceil(h/R), batch), block 64 R, dynamic LDS = R * 2 * w ints
// (R = 4 rows per workgroup; 1 for rows wider than 2048 pixels)
__global__ __launch_bounds__(256) void stereo_validate_kernel(StereoDev S) {
  extern __shared__ int s_mem[];
  const int w = S.w, lane = threadIdx.x & 63, wave = threadIdx.x >> 6, y = blockIdx.x * (blockDim.x >> 6) + wave, b = blockIdx.y;
  if (y >= S.h) return;                                     // wave-uniform; no workgroup barrier below
  int *s_d = s_mem + wave * 2 * w;
  unsigned *s_key = reinterpret_cast<unsigned *>(s_d + w);
  const int SCALE = 1 << DISP_SHIFT, INVALID = -SCALE, maxdiff = S.disp12 * SCALE;
  int16_t *dp = S.disp16 + ((size_t)b * S.h + y) * w;
  const uint16_t *cp = S.cost + ((size_t)b * S.h + y) * w;
  // the row into LDS, one word per pixel: cost << 16 | disparity (16 bits each).  Rows of 4 n pixels: four pixels per lane and load (8 bytes of
  // each array; 2-byte loads made the wave wait on twenty narrow loads per row)
  if ((w & 3) == 0) {
    for (int x = 4 * lane; x < w; x += 256) {
      const uint2 dv = *reinterpret_cast<const uint2 *>(dp + x), cv = *reinterpret_cast<const uint2 *>(cp + x);
      int4 e;
      e.x = (int)((dv.x & 0xffffu) | (cv.x << 16)); e.y = (int)((dv.x >> 16) | (cv.x & 0xffff0000u));
      e.z = (int)((dv.y & 0xffffu) | (cv.y << 16)); e.w = (int)((dv.y >> 16) | (cv.y & 0xffff0000u));
      *reinterpret_cast<int4 *>(s_d + x) = e;
      *reinterpret_cast<uint4 *>(s_key + x) = make_uint4(0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu);
    }
  } else {
    for (int x = lane; x < w; x += 64) { s_d[x] = (int)(((unsigned)(uint16_t)dp[x]) | ((unsigned)cp[x] << 16)); s_key[x] = 0xffffffffu; }
  }
  wave_lds_sync();
  const int minX1 = S.ndisp;
  for (int x = minX1 + lane; x < w; x += 64) {
    const int e = s_d[x], d = (int16_t)(e & 0xffff);
    if (d == INVALID) continue;
    const int x2 = x - ((d + SCALE / 2) >> DISP_SHIFT);
    if (x2 >= 0 && x2 < w) atomicMin(&s_key[x2], ((unsigned)e & 0xffff0000u) | (unsigned)x);
  }
  wave_lds_sync();
  for (int x = minX1 + lane; x < w; x += 64) {
    const int d = (int16_t)(s_d[x] & 0xffff);
    if (d == INVALID) continue;
    const int x0 = x - (d >> DISP_SHIFT), x1 = x - ((d + SCALE - 1) >> DISP_SHIFT);
    bool bad0 = false, bad1 = false;
    if (x0 >= 0 && x0 < w) { const unsigned k = s_key[x0]; bad0 = k != 0xffffffffu && abs((int16_t)(s_d[k & 0xffffu] & 0xffff) - d) > maxdiff; }
    if (x1 >= 0 && x1 < w) { const unsigned k = s_key[x1]; bad1 = k != 0xffffffffu && abs((int16_t)(s_d[k & 0xffffu] & 0xffff) - d) > maxdiff; }
    if (bad0 && bad1) dp[x] = (int16_t)INVALID;
  }
}
