// stereo_speckle.inc -- part of stereo.hip: the speckle filter (filterSpeckles) = connected components + saturating size count, fused with the 1/16 float conversion
//  whole frame (rows too wide for strips, frames of fewer than 16 rows, windows beyond the strip counts, SVS_STEREO_FRAME_CCL=1):
//   stereo_ccl_runs_kernel         a pixel's label = the first pixel of its horizontal run; runs longer than the window are CCL_BIG at once
//   stereo_ccl_merge_kernel, merge4    unite vertically linked runs (one or four pixels per lane)
//   stereo_ccl_count_kernel        saturating component sizes from the run lengths; flattens the labels of the run starts
//   stereo_finish_kernel, finish4  filter the pixels of small components, convert (also the plain conversion when the filter is off)
//  by strips of rows held in LDS (every frame of the reference's cameras):
//   stereo_speckle_strip_kernel    runs, stitch, count, classify and convert of one strip; components that touch a neighbour strip stay undecided
//   stereo_speckle_merge_kernel    unite the undecided components across strip boundaries
//   stereo_speckle_resolve_kernel  count the pixels of the united roots, then filter those that stay small
//
// ---- union-find on frame labels (labels = linear pixel index inside the frame), shared by both paths ----------
// Labels: -1 = filtered pixel, CCL_BIG = member of a component already known to exceed the speckle window (any
// component containing a horizontal run longer than the window), otherwise the index of a pixel of the same set
// (roots point at themselves).  CCL_BIG is smaller than every index, so "hang the larger root under the smaller"
// (atomicMin) makes it absorb whatever gets connected to it.  Every walk is bounded: a parent index is smaller than its child and chains stay
// short (labels start as run starts); past CCL_MAX_STEPS something is broken and the walk gives up -- the library never hangs the GPU -- leaving bit 8 (find) or
// 16 (union) in *err.
constexpr int CCL_BIG = -2;
constexpr int CCL_MAX_STEPS = 1 << 16;
__device__ __forceinline__ int ccl_find(const int32_t *label, int x, int *err) {
  int p = label[x], steps = 0;
#pragma nounroll      // a pointer chase: unrolled copies of the step only cost code and registers
  while (p != x && p >= 0) { x = p; p = label[x]; if (++steps > CCL_MAX_STEPS) { atomicOr(err, 8); return CCL_BIG; } }
  return p < 0 ? CCL_BIG : x;
}
__device__ __forceinline__ void ccl_union(int32_t *label, int a, int b, int *err) {      // a, b: node indices or CCL_BIG
  for (int tries = 0; tries < CCL_MAX_STEPS; ++tries) {
    if (a >= 0) a = ccl_find(label, a, err);
    if (b >= 0) b = ccl_find(label, b, err);
    if (a == b) return;
    if (a < b) { const int t = a; a = b; b = t; }      // a > b >= CCL_BIG: hang the larger root under the smaller
    const int old = atomicMin(&label[a], b);
    if (old == a) return;
    a = old;                                            // a was no longer a root: continue from its new parent
  }
  atomicOr(err, 16);
}
__device__ __forceinline__ bool ccl_linked(int a, int b, int range) { return a != FILTERED16 && b != FILTERED16 && abs(a - b) <= range; }
// four int16 of one 8-byte load
__device__ __forceinline__ void unpack4_i16(uint2 v, int (&d)[4]) {
  d[0] = (int16_t)(v.x & 0xffff); d[1] = (int16_t)(v.x >> 16); d[2] = (int16_t)(v.y & 0xffff); d[3] = (int16_t)(v.y >> 16);
}
// The merge decision for a pixel and the pixel below it.  One union per pair of overlapping runs: the leftmost linked column of the overlap does it, every other
// column is covered by its left neighbour (which unites the same two runs).  Run labels are only ever replaced by other members of the same set (or CCL_BIG).
struct CclPair { int la, lb, da, db; };      // labels and disparities of the upper and the lower pixel
__device__ __forceinline__ bool ccl_open(int la, int lb) { return !(la == -1 || lb == -1 || (la == CCL_BIG && lb == CCL_BIG)); }      // not filtered, not big above big
template <class Left>      // left() -> the CclPair of the column to the left, asked for only when it matters (has_left: there is one in this row)
__device__ __forceinline__ void ccl_merge_pixel(int32_t *label, const CclPair &p, bool has_left, Left &&left, const StereoDev &S) {
  if (!ccl_open(p.la, p.lb) || !ccl_linked(p.da, p.db, S.speckle_range)) return;
  if (has_left) { const CclPair l = left(); if (l.la == p.la && l.lb == p.lb && ccl_linked(l.da, l.db, S.speckle_range)) return; }
  ccl_union(label, p.la, p.lb, S.err);
}
// The finish decision: d of a pixel whose run starts at label l (or CCL_BIG); components of <= speckle_window pixels are filtered
__device__ __forceinline__ void ccl_finish_pixel(const StereoDev &S, size_t base, int &d, int l) {
  if (d == FILTERED16 || l < 0) return;
  const int root = S.label[base + l];                // flattened by the count pass
  if (root >= 0 && S.count[base + root] <= S.speckle_window) d = FILTERED16;
}

// Horizontal runs: label = index of the first pixel of the maximal run of horizontally linked pixels, so the union-find
// only has to stitch rows together and its chains stay short; runs longer than the speckle window are labelled CCL_BIG
// right away -- in a real disparity map that is most valid pixels, and their vertical links cost nothing later.
// One workgroup per image row, one wave per 64-pixel segment: "last run start at or left of me" and "next run boundary
// right of me" come from two ballots per segment plus a carry over the (few) segments of the row -- three barriers per
// row.  The start pixel of every small run gets count = 0 and its length in `rlen` (the cost plane, free after the
// LR check; 0 everywhere else): the later passes find the small runs through it and nothing else needs clearing.
// grid: (h, batch), block 256, dynamic LDS = (2 w + 2 nseg) ints
__global__ __launch_bounds__(256) void stereo_ccl_runs_kernel(StereoDev S) {
  extern __shared__ int s_mem[];
  const int w = S.w, y = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const size_t base = (size_t)blockIdx.y * w * S.h + (size_t)y * w;
  const int16_t *d = S.disp16 + base;
  const int nseg = (w + 63) >> 6;
  int *s_st = s_mem, *s_len = s_mem + w, *s_segl = s_len + w, *s_segf = s_segl + nseg;
  for (int seg = wave; seg < nseg; seg += 4) {
    const int x = seg * 64 + lane;
    const bool in = x < w;
    const int dv = in ? d[x] : FILTERED16, dl = (in && x > 0) ? d[x - 1] : FILTERED16;
    const bool filt = dv == FILTERED16;                                        // lanes beyond the row end act as a boundary
    const bool start = !filt && !(x > 0 && ccl_linked(dv, dl, S.speckle_range));
    const unsigned long long sb = __ballot(start), bb = __ballot(start || filt);
    const unsigned long long lower = sb & (lane == 63 ? ~0ull : ((2ull << lane) - 1ull));
    if (in) {
      s_st[x] = filt ? -2 : (lower ? seg * 64 + 63 - __clzll((long long)lower) : -1);      // -1: the run started in an earlier segment
      const unsigned long long above = lane == 63 ? 0ull : (bb >> (lane + 1));
      s_len[x] = above ? x + __ffsll((long long)above) : -1;                               // next boundary; -1: in a later segment
    }
    if (lane == 0) {
      s_segl[seg] = sb ? seg * 64 + 63 - __clzll((long long)sb) : -1;
      s_segf[seg] = bb ? seg * 64 + __ffsll((long long)bb) - 1 : 0x7fffffff;
    }
  }
  __syncthreads();
  if (tid == 0) { int run = -1; for (int k = 0; k < nseg; ++k) { const int v = s_segl[k]; s_segl[k] = run; run = max(run, v); } }              // exclusive prefix max
  if (tid == 64) { int run = w; for (int k = nseg - 1; k >= 0; --k) { const int v = s_segf[k]; s_segf[k] = run; run = min(run, v); } }          // exclusive suffix min
  __syncthreads();
  for (int x = tid; x < w; x += 256) {
    const int seg = x >> 6;
    int st = s_st[x];
    if (st == -1) { st = s_segl[seg]; s_st[x] = st; }
    if (st == x) { int nb = s_len[x]; if (nb < 0) nb = s_segf[seg]; s_len[x] = min(nb, w) - x; }
  }
  __syncthreads();
  uint16_t *rlen = S.cost + base;
  for (int x = tid; x < w; x += 256) {
    const int st = s_st[x];
    int lab = -1, rl = 0;
    if (st >= 0) {
      const int len = s_len[st];
      const bool big = len > S.speckle_window;
      lab = big ? CCL_BIG : y * w + st;
      if (!big && st == x) { rl = len; S.count[base + x] = 0; }
    }
    S.label[base + x] = lab;
    rlen[x] = (uint16_t)rl;
  }
}
// stitch vertically linked pixels; one union per pair of overlapping runs (the leftmost linked column of the overlap).
// grid: (ceil(w*h/256), batch) -- scalar variant for widths that are not a multiple of 4
__global__ __launch_bounds__(256) void stereo_ccl_merge_kernel(StereoDev S) {
  const int i = blockIdx.x * 256 + threadIdx.x, n = S.w * S.h, w = S.w;
  if (i + w >= n) return;
  const size_t base = (size_t)blockIdx.y * n;
  const int16_t *d = S.disp16 + base;
  int32_t *label = S.label + base;
  const int la = label[i], lb = label[i + w];
  if (!ccl_open(la, lb)) return;
  ccl_merge_pixel(label, CclPair{la, lb, d[i], d[i + w]}, i % w > 0, [&] { return CclPair{label[i - 1], label[i + w - 1], d[i - 1], d[i + w - 1]}; }, S);
}
// same, four horizontally adjacent pixels per lane (w % 4 == 0): the labels of both rows arrive as two 16-byte loads and
// most lanes leave right there (filtered, or big above big); grid: (ceil(w*h/1024), batch)
__global__ __launch_bounds__(256) void stereo_ccl_merge4_kernel(StereoDev S) {
  const int i0 = (blockIdx.x * 256 + threadIdx.x) * 4, n = S.w * S.h, w = S.w;
  if (i0 + w >= n) return;
  const size_t base = (size_t)blockIdx.y * n;
  const int16_t *d = S.disp16 + base;
  int32_t *label = S.label + base;
  const int4 a4 = *reinterpret_cast<const int4 *>(label + i0), b4 = *reinterpret_cast<const int4 *>(label + i0 + w);
  const int la[4] = {a4.x, a4.y, a4.z, a4.w}, lb[4] = {b4.x, b4.y, b4.z, b4.w};
  bool any = false;
#pragma unroll
  for (int k = 0; k < 4; ++k) any |= ccl_open(la[k], lb[k]);
  if (!any) return;
  int da[4], db[4];
  unpack4_i16(*reinterpret_cast<const uint2 *>(d + i0), da);
  unpack4_i16(*reinterpret_cast<const uint2 *>(d + i0 + w), db);
#pragma unroll
  for (int k = 0; k < 4; ++k)
    ccl_merge_pixel(label, CclPair{la[k], lb[k], da[k], db[k]}, k > 0 || i0 % w > 0, [&] {
      return k > 0 ? CclPair{la[k - 1], lb[k - 1], da[k - 1], db[k - 1]} : CclPair{label[i0 - 1], label[i0 + w - 1], d[i0 - 1], d[i0 + w - 1]}; }, S);
}
// component sizes, saturating: the test is "size <= speckle_window", so a root that is already beyond the window is left
// alone.  Only the start pixels of small runs carry a length (rlen != 0): eight pixels per lane, most lanes see zeros.
// Members of CCL_BIG need no count.  grid: (ceil(w*h/2048), batch)
__global__ __launch_bounds__(256) void stereo_ccl_count_kernel(StereoDev S) {
  const int n = S.w * S.h, i0 = (blockIdx.x * 256 + threadIdx.x) * 8;
  if (i0 >= n) return;
  const size_t base = (size_t)blockIdx.y * n;
  const uint16_t *rlen = S.cost + base;
  int len[8];
  if (((base | (size_t)i0) & 7) == 0 && i0 + 8 <= n) {
    const uint4 r = *reinterpret_cast<const uint4 *>(rlen + i0);
    if ((r.x | r.y | r.z | r.w) == 0) return;
    len[0] = r.x & 0xffff; len[1] = r.x >> 16; len[2] = r.y & 0xffff; len[3] = r.y >> 16;
    len[4] = r.z & 0xffff; len[5] = r.z >> 16; len[6] = r.w & 0xffff; len[7] = r.w >> 16;
  } else {
#pragma unroll
    for (int k = 0; k < 8; ++k) len[k] = i0 + k < n ? rlen[i0 + k] : 0;
  }
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    if (len[k] == 0) continue;
    const int root = ccl_find(S.label + base, i0 + k, S.err);
    if (root != i0 + k) S.label[base + i0 + k] = root;      // flatten: the pixels of this run reach the root (or CCL_BIG) in one hop;
                                                            // roots stay roots, so concurrent finds through this node remain valid
    if (root >= 0 && S.count[base + root] <= S.speckle_window) atomicAdd(&S.count[base + root], len[k]);
  }
}
// disparity in pixels; components of <= speckle_window pixels are filtered.  use_ccl == 0: plain conversion
__global__ __launch_bounds__(256) void stereo_finish_kernel(StereoDev S, int use_ccl, float *__restrict__ out, int dstride, size_t d_bstride) {
  const int i = blockIdx.x * 256 + threadIdx.x, n = S.w * S.h;
  if (i >= n) return;
  const size_t base = (size_t)blockIdx.y * n;
  int d = S.disp16[base + i];
  if (use_ccl && d != FILTERED16) ccl_finish_pixel(S, base, d, S.label[base + i]);
  out[(size_t)blockIdx.y * d_bstride + (size_t)(i / S.w) * dstride + (i % S.w)] = (float)d * (1.f / (1 << DISP_SHIFT));
}

// same, four pixels per lane (w % 4 == 0, so the four share a row): one 8-byte disparity load, one 16-byte label load;
// grid: (ceil(w*h/1024), batch)
__global__ __launch_bounds__(256) void stereo_finish4_kernel(StereoDev S, int use_ccl, float *__restrict__ out, int dstride, size_t d_bstride) {
  const int i0 = (blockIdx.x * 256 + threadIdx.x) * 4, n = S.w * S.h;
  if (i0 >= n) return;
  const size_t base = (size_t)blockIdx.y * n;
  int d[4];
  unpack4_i16(*reinterpret_cast<const uint2 *>(S.disp16 + base + i0), d);
  if (use_ccl) {
    const int4 l4 = *reinterpret_cast<const int4 *>(S.label + base + i0);
    const int l[4] = {l4.x, l4.y, l4.z, l4.w};
#pragma unroll
    for (int k = 0; k < 4; ++k) ccl_finish_pixel(S, base, d[k], l[k]);
  }
  float *o = out + (size_t)blockIdx.y * d_bstride + (size_t)(i0 / S.w) * dstride + (i0 % S.w);
#pragma unroll
  for (int k = 0; k < 4; ++k) o[k] = (float)d[k] * (1.f / (1 << DISP_SHIFT));
}


// ---- speckle filter by strips ------------------------------------------------------------------------------------------
// filterSpeckles needs the SIZE of every 4-connected component, but only up to speckle_window (100 pixels in the reference's
// configuration): nearly every component is either far larger or a speck of a few pixels, and both kinds are decided inside a strip
// of rows held in LDS.  One workgroup per (strip, frame):
//   runs      one wave per row: a pixel's label is the strip index of the first pixel of its horizontal run (two ballots per 64-pixel
//             segment, the last run start carried across segments in an SGPR); the run's last pixel knows its length -- runs longer
//             than the window make their start a member of BIG at once;
//   stitch    vertically linked pixels unite their runs (lock-free union-find on LDS words: a root holds ~(pixels | touch << 24), i.e.
//             a negative word, every other node the index of its parent; the larger root index is hung under the smaller with a CAS);
//   count     the last pixel of every run adds its length to the root (saturating: the test is size <= window) and marks the root if
//             the run lies on a row that has a neighbour strip;
//   decide    more than window pixels, or BIG: kept.  Small and not touching a neighbour strip: filtered.  Small and touching: UNDECIDED
//             -- the pixels are kept for now and listed (pixel, node) with node = the frame index of the root pixel; the first / last
//             row of the strip leaves its node ids in `brow`.  The float conversion of the stage is fused in here.
// Three small kernels finish the undecided ones: unite nodes across strip boundaries (ccl_find / ccl_union on frame labels, as the
// whole-frame path above), count the listed pixels per united root, filter the pixels of the roots that stay <= window.
// HBM traffic of the whole filter: disparity read once (2 B/px), float written once (4 B/px); the whole-frame path moved 46 B/px.
constexpr int SPK_BIG = (int)0x80000000;           // root value of the BIG set; no real root value is that negative
// (every loop of the union-find routines is bounded: a parent index is smaller than its child, so a walk takes fewer steps than the strip
//  has pixels; past that something is broken and the walk gives up -- the library never hangs the GPU -- leaving a mark in *err)
constexpr int SPK_MAX_STEPS = 1 << 16;
__device__ __forceinline__ int spk_find(const int *lab, int x, int *err) {      // -> root index, or -1 for BIG
  int v = lab[x], steps = 0;
  while (v >= 0) { x = v; v = lab[x]; if (++steps > SPK_MAX_STEPS) { atomicOr(err, 1); return -1; } }
  return v == SPK_BIG ? -1 : x;
}
// same, halving the path on the way (a parent word is only ever replaced by an ancestor: safe next to concurrent unions and finds)
__device__ __forceinline__ int spk_find_halve(int *lab, int x, int *err) {
  int v = lab[x], steps = 0;
  while (v >= 0) {
    const int vv = lab[v];
    if (vv >= 0) lab[x] = vv;
    x = v; v = vv;
    if (++steps > SPK_MAX_STEPS) { atomicOr(err, 2); return -1; }
  }
  return v == SPK_BIG ? -1 : x;
}
__device__ __forceinline__ void spk_union(int *lab, int a, int b, int *err) {   // a, b: nodes of the strip
  for (int tries = 0;; ++tries) {
    if (tries > SPK_MAX_STEPS) { atomicOr(err, 4); return; }
    if (a >= 0) a = spk_find_halve(lab, a, err);              // (-1 = BIG stays BIG: it is not an index)
    if (b >= 0) b = spk_find_halve(lab, b, err);
    if (a == b) return;
    if (a < b) { const int t = a; a = b; b = t; }                     // a > b >= -1: hang root a under b (b == -1: a joins BIG)
    if (atomicCAS(&lab[a], ~0, b < 0 ? SPK_BIG : b) == ~0) return;    // (a root before the counting pass is ~0: zero pixels, no mark)
    // a stopped being a root in the meantime: look again from the top
  }
}
// grid: (n_strips, batch), block SPK_THREADS, dynamic LDS = strip_rows * round_up(w, 4) * 6 bytes (labels: int, disparities: int16).
// Four horizontally adjacent pixels per lane and step (one 8-byte disparity read, one 16-byte label read); a pixel of a run longer than
// the window carries SPK_BIG itself, so the common cases -- filtered, or big above big -- leave after those two reads.
// acc with lane `sel` replaced by the wave-uniform `val` (V_WRITELANE_B32; this compiler has no builtin for it).  `sel` is a constant after unrolling at every call
// site: the switch folds to the one instruction with the lane select as an inline constant.
__device__ __forceinline__ unsigned spk_writelane(unsigned acc, unsigned val, int sel) {
#define SPK_WL(n) case n: asm("v_writelane_b32 %0, %1, " #n : "+v"(acc) : "s"(val)); break;
  switch (sel) {
    SPK_WL(0) SPK_WL(1) SPK_WL(2) SPK_WL(3) SPK_WL(4) SPK_WL(5) SPK_WL(6) SPK_WL(7) SPK_WL(8) SPK_WL(9)
    SPK_WL(10) SPK_WL(11) SPK_WL(12) SPK_WL(13) SPK_WL(14) SPK_WL(15) SPK_WL(16) SPK_WL(17) SPK_WL(18) SPK_WL(19)
    SPK_WL(20) SPK_WL(21) SPK_WL(22) SPK_WL(23) SPK_WL(24) SPK_WL(25) SPK_WL(26) SPK_WL(27) SPK_WL(28) SPK_WL(29)
    SPK_WL(30) SPK_WL(31) SPK_WL(32) SPK_WL(33) SPK_WL(34) SPK_WL(35) SPK_WL(36) SPK_WL(37) SPK_WL(38) SPK_WL(39)
    default: break;
  }
#undef SPK_WL
  return acc;
}
__global__ __launch_bounds__(SPK_THREADS) void stereo_speckle_strip_kernel(StereoDev S, float *__restrict__ out, int dstride, size_t d_bstride) {
  extern __shared__ int s_mem[];
  __shared__ unsigned long long s_bb[SPK_THREADS / 64][SPK_MAX_SEG];
  __shared__ int s_npend;
  if (threadIdx.x == 0) s_npend = 0;
  const int w = S.w, h = S.h, wp = (w + 3) & ~3, gpr = wp >> 2;
  const int b = blockIdx.y, strip = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int y0 = strip * S.strip_rows, y1 = min(h, y0 + S.strip_rows), nr = y1 - y0, ng = nr * gpr;
#define SPK_STAMP(k) do { if (S.timing && tid == 0 && strip == S.n_strips / 2 && b == 0) reinterpret_cast<long long *>(S.err + 8)[k] = (long long)wall_clock64(); } while (0)
  SPK_STAMP(0);
  int *lab = s_mem;
  int16_t *dsp = reinterpret_cast<int16_t *>(s_mem + S.strip_rows * wp);
  const size_t fbase = (size_t)b * w * h, sbase = fbase + (size_t)y0 * w;
  const int range = S.speckle_range, window = S.speckle_window;
  const bool vec = (w & 3) == 0;                               // then every row of the frame starts 8-byte aligned
  const uint32_t f2 = (uint32_t)(uint16_t)FILTERED16 * 0x00010001u;
  for (int g = tid; g < ng; g += SPK_THREADS) {
    const int row = g / gpr, x0 = (g - row * gpr) * 4;
    const int16_t *src = S.disp16 + sbase + (size_t)row * w + x0;
    uint2 v;
    if (vec) v = *reinterpret_cast<const uint2 *>(src);
    else {
      uint32_t e[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) e[k] = x0 + k < w ? (uint32_t)(uint16_t)src[k] : (uint32_t)(uint16_t)FILTERED16;
      v.x = e[0] | (e[1] << 16); v.y = e[2] | (e[3] << 16);
    }
    *reinterpret_cast<uint2 *>(dsp + row * wp + x0) = v;
  }
  __syncthreads();
  SPK_STAMP(1);
  // ---- runs: one wave per row.  Left to right: the start of every pixel's run; right to left: its end, hence its length.
  //      Rows of up to SPK_NS segments (640 pixels) are handled in registers: all the row's loads in flight at once, the ballots of its
  //      segments in scalar registers, one label store per pixel -- the stepwise form below paid three LDS round trips per segment.
  const int nseg = (w + 63) >> 6;
  // Rows of up to SPK_NS segments also leave four bit masks per segment in LDS (`msk`, [row][4][SPK_NS] ballots) that the three later passes scan instead of the
  // pixels: ST = "unites its run with the one below" (vertically linked and the leftmost linked column of the two runs' overlap), CN = "last pixel of a run that
  // is not big", CL = "valid pixel of a run that is not big", S = "starts a run".  Their loops then cost two V_READLANE and a scalar branch per 64 pixels
  // where they read four disparities and evaluated four link tests per pixel (those passes were bound by VALU issue on the strip's one CU).  "Big" is the
  // state after THIS pass (a single-pixel run that joins BIG while rows are stitched stays listed: its find returns BIG and the entry is dropped).
  unsigned long long *const msk = reinterpret_cast<unsigned long long *>(dsp + S.strip_rows * wp);
  constexpr int MSK_ROW = 4 * SPK_NS;
  const bool use_msk = nseg <= SPK_NS;
  if (nseg <= SPK_NS) {
    for (int row = wave; row < nr; row += SPK_THREADS / 64) {
      const int16_t *d = dsp + row * wp;
      int *l = lab + row * wp;
      const bool has_b = row + 1 < nr;
      int dv[SPK_NS], dl[SPK_NS], db[SPK_NS], dbl[SPK_NS];
#pragma unroll
      for (int sg = 0; sg < SPK_NS; ++sg) {
        const int x = sg * 64 + lane;
        dv[sg] = x < w ? d[x] : FILTERED16;
        dl[sg] = (x < w && x > 0) ? d[x - 1] : FILTERED16;
        db[sg] = (has_b && x < w) ? d[wp + x] : FILTERED16;
        dbl[sg] = (has_b && x < w && x > 0) ? d[wp + x - 1] : FILTERED16;
      }
      // the row's 4 x SPK_NS mask words are assembled in the lanes that will store them (lane = mask * SPK_NS + segment): V_WRITELANE from the scalar ballots
      unsigned mlo = 0u, mhi = 0u;
      auto put = [&](int word, unsigned long long v) { mlo = spk_writelane(mlo, (unsigned)v, word); mhi = spk_writelane(mhi, (unsigned)(v >> 32), word); };
      unsigned long long sb[SPK_NS], bb[SPK_NS];
      unsigned long long vm_prev = 0ull;
#pragma unroll
      for (int sg = 0; sg < SPK_NS; ++sg) {
        const bool filt = dv[sg] == FILTERED16, start = !filt && !ccl_linked(dv[sg], dl[sg], range);
        sb[sg] = __ballot(start); bb[sg] = __ballot(start || filt);
        const unsigned long long vm = __ballot(ccl_linked(dv[sg], db[sg], range));        // vertically linked to the pixel below
        const unsigned long long hb = __ballot(ccl_linked(db[sg], dbl[sg], range));       // the pixel below is linked to its left neighbour
        const unsigned long long vsh = (vm << 1) | (vm_prev >> 63);                        // the left neighbours are vertically linked
        put(0 * SPK_NS + sg, vm & ~(vsh & ~bb[sg] & hb));                                  // (~bb: valid and linked to the left neighbour; 0 past the row end)
        put(3 * SPK_NS + sg, sb[sg]);
        vm_prev = vm;
      }
      int carry[SPK_NS], nbc[SPK_NS];                         // last run start left of segment sg / first boundary right of it
      { int c = 0; 
#pragma unroll
        for (int sg = 0; sg < SPK_NS; ++sg) { carry[sg] = c; if (sb[sg]) c = sg * 64 + 63 - __clzll((long long)sb[sg]); } }
      { int c = w;
#pragma unroll
        for (int sg = SPK_NS - 1; sg >= 0; --sg) { nbc[sg] = c; if (bb[sg]) c = sg * 64 + __ffsll((long long)bb[sg]) - 1; } }
#pragma unroll
      for (int sg = 0; sg < SPK_NS; ++sg) {
        const int x = sg * 64 + lane;
        const unsigned long long lower = sb[sg] & (lane == 63 ? ~0ull : ((2ull << lane) - 1ull));
        const unsigned long long above = lane == 63 ? 0ull : (bb[sg] >> (lane + 1));
        const int st = lower ? sg * 64 + 63 - __clzll((long long)lower) : carry[sg];
        const int nbx = above ? x + __ffsll((long long)above) : nbc[sg];
        const bool filt = dv[sg] == FILTERED16, isbig = !filt && nbx - st > window;
        const unsigned long long big = __ballot(isbig && x < w);
        if (x < w) l[x] = filt ? SPK_BIG + 1 : isbig ? SPK_BIG : st == x ? ~0 : row * wp + st;
        const unsigned long long cl = (sb[sg] | ~bb[sg]) & ~big;                                                   // valid (starts a run or is linked to the left) and not big
        const unsigned long long hnext = (~bb[sg] >> 1) | (sg + 1 < SPK_NS ? ~bb[sg + 1 < SPK_NS ? sg + 1 : sg] << 63 : 0ull);      // pixel x + 1 is linked to x
        put(1 * SPK_NS + sg, cl & ~hnext);
        put(2 * SPK_NS + sg, cl);
      }
      for (int x = w + lane; x < wp; x += 64) l[x] = SPK_BIG + 1;
      if (lane < MSK_ROW) msk[(size_t)row * MSK_ROW + lane] = ((unsigned long long)mhi << 32) | mlo;
    }
  } else {
    for (int row = wave; row < nr; row += SPK_THREADS / 64) {
      const int16_t *d = dsp + row * wp;
      int *l = lab + row * wp;
      int carry = 0;                                            // last run start of the earlier segments
      for (int seg = 0; seg < nseg; ++seg) {
        const int x = seg * 64 + lane;
        const bool in = x < w;
        const int dv = in ? d[x] : FILTERED16, dl = (in && x > 0) ? d[x - 1] : FILTERED16;
        const bool filt = dv == FILTERED16, start = !filt && !ccl_linked(dv, dl, range);
        const unsigned long long sb = __ballot(start), bb = __ballot(start || filt);
        const unsigned long long lower = sb & (lane == 63 ? ~0ull : ((2ull << lane) - 1ull));
        if (in) l[x] = filt ? -1 : lower ? seg * 64 + 63 - __clzll((long long)lower) : carry;
        if (lane == 0) s_bb[wave][seg] = bb;
        if (sb) carry = seg * 64 + 63 - __clzll((long long)sb);
      }
      int nb_carry = w;                                         // first boundary (run start, filtered pixel, row end) of the later segments
      for (int seg = nseg - 1; seg >= 0; --seg) {
        const int x = seg * 64 + lane;
        const unsigned long long bb = s_bb[wave][seg];
        const unsigned long long above = lane == 63 ? 0ull : (bb >> (lane + 1));
        const int nbx = above ? x + __ffsll((long long)above) : nb_carry;
        if (x < w) {
          const int st = l[x];
          l[x] = st < 0 ? SPK_BIG + 1 : (nbx - st > window) ? SPK_BIG : st == x ? ~0 : row * wp + st;
        }
        if (bb) nb_carry = seg * 64 + __ffsll((long long)bb) - 1;
      }
      for (int x = w + lane; x < wp; x += 64) l[x] = SPK_BIG + 1;
    }
  }
  __syncthreads();
  SPK_STAMP(2);
  // ---- stitch / count / classify share one shape: a wave takes a row, lane = column, all the row's operands in flight at once; the few
  //      lanes with real work (a union, a run to count, a pixel of a small component) do not do it in place -- every such block would
  //      cost the whole wave three dependent LDS round trips per segment -- but append their column to a queue, and the queue is worked
  //      off with one entry per lane.
  int *const q = reinterpret_cast<int *>(s_bb[wave]);        // 64 entries (the ballots of the stepwise runs pass are done with)
  const unsigned long long lt_mask = lane == 0 ? 0ull : (~0ull >> (64 - lane));
  // queue entry: column (12 bits) | "starts its run" << 12 | row << 16.  The queue is worked off when it is full and once after the wave's last row: a flush is a
  // chain of dependent LDS round trips whatever the number of entries, so it is not paid per row.
  int qn = 0;
  auto enqueue = [&](unsigned long long m, unsigned long long flag_m, int x0, int row, auto &&flush) {      // the set lanes of m append column x0 + lane
    if (m == 0) return;
    const int c = __popcll(m);
    if (qn + c > 64) { flush(qn); qn = 0; }
    if ((m >> lane) & 1ull) q[qn + __popcll(m & lt_mask)] = (x0 + lane) | ((int)((flag_m >> lane) & 1ull) << 12) | (row << 16);
    qn += c;
  };
  // the row scan of a pass: the rows [0, last) of this wave; the lanes to enqueue and their "starts its run" flags come from the mask words m_on / m_flag of `msk`
  // (m_flag < 0: no flag), or for rows wider than SPK_NS segments from pred(row, x, in) -> (on, flag), evaluated per pixel; then the queue's rest is worked off
  auto scan_rows = [&](int last, int m_on, int m_flag, auto &&pred, auto &&flush) __attribute__((always_inline)) {
    for (int row = wave; row < last; row += SPK_THREADS / 64) {
      if (use_msk) {
        const unsigned long long mv = lane < MSK_ROW ? msk[(size_t)row * MSK_ROW + lane] : 0ull;      // the row's masks: one LDS read, then lane broadcasts
#pragma unroll
        for (int k = 0; k < SPK_NS; ++k) enqueue(lane_bcast(mv, m_on * SPK_NS + k), m_flag < 0 ? 0ull : lane_bcast(mv, m_flag * SPK_NS + k), k * 64, row, flush);
      } else {
        for (int seg = 0; seg < nseg; ++seg) {
          const int x = seg * 64 + lane;
          bool on, flag;
          pred(row, x, x < w, on, flag);
          enqueue(__ballot(on), __ballot(flag), seg * 64, row, flush);
        }
      }
    }
    flush(qn); qn = 0;
  };
  // ---- stitch rows.  A pixel unites its run with the one below where it is the LEFTMOST linked column of the two runs' overlap:
  //      vertically linked, and not (left neighbours vertically linked + both horizontal links)
  {
    auto flush = [&](int n_) {
      if (lane < n_) {
        const int e = q[lane], x = e & 0xfff, row = e >> 16;
        const int a = lab[row * wp + x], c = lab[(row + 1) * wp + x];
        // node of a pixel = its run start (the pixel itself where it starts a run or carries SPK_BIG: its word is a root / parent word then)
        if (!(a == SPK_BIG && c == SPK_BIG)) spk_union(lab, a >= 0 ? a : row * wp + x, c >= 0 ? c : (row + 1) * wp + x, S.err);
      }
    };
    scan_rows(nr - 1, 0, -1, [&](int row, int x, bool in, bool &on, bool &flag) {
      const int16_t *da = dsp + row * wp, *db = da + wp;
      const int va = in ? da[x] : FILTERED16, vb = in ? db[x] : FILTERED16;
      const int pa = (in && x > 0) ? da[x - 1] : FILTERED16, pb = (in && x > 0) ? db[x - 1] : FILTERED16;
      const bool covered = ccl_linked(pa, pb, range) && ccl_linked(pa, va, range) && ccl_linked(pb, vb, range);
      on = ccl_linked(va, vb, range) && !covered; flag = false;
    }, flush);
  }
  __syncthreads();
  SPK_STAMP(3);
  // ---- count: the last pixel of a run adds the run to its root
  const bool nb_top = y0 > 0, nb_bot = y1 < h;
  {
    auto flush = [&](int n_) {
      if (lane < n_) {
        const int e = q[lane], x = e & 0xfff, row = e >> 16;
        const int st = ((e >> 12) & 1) ? row * wp + x : lab[row * wp + x];      // (the word of a start pixel is a root / parent word, not a start index)
        const int root = spk_find(lab, st, S.err);
        if (root >= 0) {
          if ((~lab[root] & (SPK_TOUCH - 1)) <= window) atomicSub(&lab[root], row * wp + x - st + 1);      // ~(V + len) = ~V - len
          if ((row == 0 && nb_top) || (row == nr - 1 && nb_bot)) atomicAnd(&lab[root], ~SPK_TOUCH);            // sets the mark in V
        }
      }
    };
    scan_rows(nr, 1, 3, [&](int row, int x, bool in, bool &on, bool &flag) {
      const int16_t *d = dsp + row * wp;
      const int dv = in ? d[x] : FILTERED16, lv = in ? lab[row * wp + x] : SPK_BIG + 1;
      const int dl = (in && x > 0) ? d[x - 1] : FILTERED16, dr = (in && x + 1 < w) ? d[x + 1] : FILTERED16;
      on = dv != FILTERED16 && lv != SPK_BIG && !ccl_linked(dv, dr, range);      // last pixel of a run that is not big
      flag = !ccl_linked(dv, dl, range);
    }, flush);
  }
  __syncthreads();
  SPK_STAMP(4);
  // ---- classify the pixels of the components that are not big: filtered (their disparity in LDS becomes FILTERED), kept, or undecided
  //      (kept for now and listed; on the strip's first / last row they publish their node)
  __shared__ unsigned s_pmask[2][SPK_MAX_SEG * 2];            // undecided pixels of the first / last row
  for (int i = tid; i < 2 * SPK_MAX_SEG * 2; i += SPK_THREADS) (&s_pmask[0][0])[i] = 0u;
  __syncthreads();
  {
    auto flush = [&](int n_) {
      if (lane < n_) {
        const int e = q[lane], x = e & 0xfff, row = e >> 16, idx = row * wp + x;
        const int root = spk_find(lab, ((e >> 12) & 1) ? idx : lab[idx], S.err);
        if (root >= 0) {                                      // else: joined BIG
          const int V = ~lab[root];
          if ((V & (SPK_TOUCH - 1)) <= window) {
            if (!(V & SPK_TOUCH)) dsp[idx] = (int16_t)FILTERED16;
            else {                                            // undecided: decided after the strips have been united
              const int rrow = root / wp, node = (y0 + rrow) * w + (root - rrow * wp);      // frame index of the root pixel
              if (root == idx) { S.label[fbase + node] = node; S.count[fbase + node] = 0; }
              const int slot = atomicAdd(&s_npend, 1);        // (a per-frame counter in global memory cost more than the rest of the kernel)
              S.pend[sbase + slot] = make_int2((y0 + row) * w + x, node);
              for (int side = 0; side < 2; ++side)
                if (side == 0 ? (row == 0 && nb_top) : (row == nr - 1 && nb_bot)) {
                  S.brow[((size_t)b * 2 * S.n_strips + 2 * strip + side) * w + x] = node;
                  atomicOr(&s_pmask[side][x >> 5], 1u << (x & 31));
                }
            }
          }
        }
      }
    };
    scan_rows(nr, 2, 3, [&](int row, int x, bool in, bool &on, bool &flag) {
      const int16_t *d = dsp + row * wp;
      const int dv = in ? d[x] : FILTERED16, lv = in ? lab[row * wp + x] : SPK_BIG + 1, dl = (in && x > 0) ? d[x - 1] : FILTERED16;
      on = dv != FILTERED16 && lv != SPK_BIG; flag = !ccl_linked(dv, dl, range);
    }, flush);
  }
  __syncthreads();
  SPK_STAMP(5);
  // ---- convert: the float disparity of the stage (four pixels per lane); the strip's first / last row publish -1 (filtered) / -2 (kept)
  //      where no undecided node stands
  const float sc = 1.f / (1 << DISP_SHIFT);
  for (int g = tid; g < ng; g += SPK_THREADS) {
    const int i0 = g * 4, row = g / gpr, x0 = (g - row * gpr) * 4;
    int dq[4];
    unpack4_i16(*reinterpret_cast<const uint2 *>(dsp + i0), dq);
    float *o = out + (size_t)b * d_bstride + (size_t)(y0 + row) * dstride + x0;
    if (vec && (dstride & 3) == 0 && (d_bstride & 3) == 0 && ((uintptr_t)out & 15) == 0) *reinterpret_cast<float4 *>(o) = make_float4((float)dq[0] * sc, (float)dq[1] * sc, (float)dq[2] * sc, (float)dq[3] * sc);
    else {
#pragma unroll
      for (int k = 0; k < 4; ++k) if (x0 + k < w) o[k] = (float)dq[k] * sc;
    }
#pragma unroll
    for (int side = 0; side < 2; ++side)
      if (side == 0 ? (row == 0 && nb_top) : (row == nr - 1 && nb_bot)) {
        int32_t *br = S.brow + ((size_t)b * 2 * S.n_strips + 2 * strip + side) * w + x0;
#pragma unroll
        for (int k = 0; k < 4; ++k)
          if (x0 + k < w && !((s_pmask[side][(x0 + k) >> 5] >> ((x0 + k) & 31)) & 1u)) br[k] = dq[k] == FILTERED16 ? -1 : -2;
      }
  }
  __syncthreads();
  SPK_STAMP(6);
  if (tid == 0) S.npend[b * S.n_strips + strip] = s_npend;
}
// unite the undecided components across strip boundaries.  grid: (n_strips - 1, batch), block 256
__global__ __launch_bounds__(256) void stereo_speckle_merge_kernel(StereoDev S) {
  const int w = S.w, b = blockIdx.y, k = blockIdx.x;            // boundary between strip k and k + 1
  const int yb = (k + 1) * S.strip_rows - 1;                    // last row of strip k
  const size_t fbase = (size_t)b * w * S.h;
  const int32_t *na = S.brow + ((size_t)b * 2 * S.n_strips + 2 * k + 1) * w, *nb = S.brow + ((size_t)b * 2 * S.n_strips + 2 * k + 2) * w;
  const int16_t *da = S.disp16 + fbase + (size_t)yb * w, *db = da + w;
  int32_t *label = S.label + fbase;
  for (int x = threadIdx.x; x < w; x += 256) {
    const int a = na[x], c = nb[x];
    if (a == -1 || c == -1 || (a == -2 && c == -2)) continue;
    if (!ccl_linked(da[x], db[x], S.speckle_range)) continue;
    ccl_union(label, a == -2 ? CCL_BIG : a, c == -2 ? CCL_BIG : c, S.err);
  }
}
// pass 0: pixels per united root (saturating); pass 1: filter the pixels of the roots that stay small.  grid: (n_strips, batch), block 256
__global__ __launch_bounds__(256) void stereo_speckle_resolve_kernel(StereoDev S, int pass, float *__restrict__ out, int dstride, size_t d_bstride) {
  const int b = blockIdx.y, np = S.npend[b * S.n_strips + blockIdx.x], w = S.w;
  const size_t fbase = (size_t)b * w * S.h, sbase = fbase + (size_t)blockIdx.x * S.strip_rows * w;
  for (int i = threadIdx.x; i < np; i += 256) {
    const int2 e = S.pend[sbase + i];
    const int root = ccl_find(S.label + fbase, e.y, S.err);
    if (root < 0) continue;
    if (pass == 0) { if (S.count[fbase + root] <= S.speckle_window) atomicAdd(&S.count[fbase + root], 1); }
    else if (S.count[fbase + root] <= S.speckle_window) out[(size_t)b * d_bstride + (size_t)(e.x / w) * dstride + (e.x % w)] = (float)FILTERED16 * (1.f / (1 << DISP_SHIFT));
  }
}
