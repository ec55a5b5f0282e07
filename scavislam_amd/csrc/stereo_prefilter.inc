// stereo_prefilter.inc -- part of stereo.hip: the XSOBEL prefilter (3x3 x-Sobel -> saturating table), written +1 (so 0 can act as the MQSAD mask) into
// column-padded rows (replicated borders = the MIN/MAX clamps of the original)
//   stereo_prefilter_kernel     any width, stride and alignment: 4 padded columns x 4 rows per thread
//   stereo_prefilter16_kernel   rows of 16 n pixels on dword-aligned sources: 16 padded columns x 4 rows per thread, packed 16-bit arithmetic
__device__ __forceinline__ int xsobel_tab(int v, int cap) { return v < -cap ? 0 : v > cap ? 2 * cap : v + cap; }

__device__ __forceinline__ int byte_of(uint32_t lo, uint32_t hi, int i) { return (int)((i < 4 ? lo >> (8 * i) : hi >> (8 * (i - 4))) & 0xffu); }

// dword at byte position q of a row of w bytes, read from the clamped position and shifted into place: bytes that fall
// outside the row come back as 0 (they only ever feed border columns, which are overwritten).  Branch-free on purpose:
// a per-byte border path makes every wave that holds an edge lane walk it, with a wait behind each load.
__device__ __forceinline__ uint32_t load_u32_clamped(const uint8_t *row, int q, int w) {
  const int qs = min(max(q, 0), w - 4), d = q - qs;
  const uint32_t raw = ld_unaligned<uint32_t>(row + qs);
  return d == 0 ? raw : (d >= 4 || d <= -4) ? 0u : d > 0 ? raw >> (8 * d) : raw << (-8 * d);
}
// 4 padded columns x 4 rows per thread (the six input rows of a 4-row group are read once: 12 dword loads per 16 pixels instead of 24; the
// horizontal differences of an input row serve three output rows), 16 rows per workgroup.
// grid: (ceil(pitch/256), ceil(h/16), 2*batch), block (64, 4); z = 2*b + (0 left | 1 right)
__global__ __launch_bounds__(256) void stereo_prefilter_kernel(StereoDev S, const uint8_t *__restrict__ left, int lstride, size_t l_bstride,
                                                               const uint8_t *__restrict__ right, int rstride, size_t r_bstride) {
  const int pc0 = 4 * (blockIdx.x * 64 + threadIdx.x), y0 = (blockIdx.y * 4 + threadIdx.y) * 4, b = blockIdx.z >> 1, side = blockIdx.z & 1;
  const int w = S.w, h = S.h, cap = S.cap;
  if (pc0 >= S.pitch || y0 >= h) return;      // pitch is a multiple of 4
  const uint8_t *src = side ? right + (size_t)b * r_bstride : left + (size_t)b * l_bstride;
  const int stride = side ? rstride : lstride;
  const int x0 = pc0 - PADL;
  const uint32_t fill = 0x01010101u * (uint32_t)(cap + 1);      // pads, border columns, odd last row
  // horizontal differences byte(j + 2) - byte(j), j = 0..3, of the six input rows y0-1 .. y0+4 (rows outside the image: the row the
  // original's yp / yn pick, i.e. 1 above the top and h-2 below the bottom)
  int d[6][4];
#pragma unroll
  for (int i = 0; i < 6; ++i) {
    int r = y0 - 1 + i;
    r = r < 0 ? (h > 1 ? 1 : 0) : (r > h - 1 ? (h > 1 ? h - 2 : 0) : r);
    r = min(max(r, 0), h - 1);                                  // (rows far below the image only feed rows that are not written)
    const uint8_t *row = src + (size_t)r * stride;
    const uint32_t a0 = load_u32_clamped(row, x0 - 1, w), a1 = load_u32_clamped(row, x0 + 3, w);
#pragma unroll
    for (int j = 0; j < 4; ++j) d[i][j] = byte_of(a0, a1, j + 2) - byte_of(a0, a1, j);
  }
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int y = y0 + k;
    if (y >= h) break;
    uint32_t out = fill;
    if (!((h & 1) && y == h - 1)) {
      out = 0;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int x = x0 + j;
        const int v = d[k][j] + 2 * d[k + 1][j] + d[k + 2][j];
        const uint32_t o = (x >= 1 && x <= w - 2) ? (uint32_t)(xsobel_tab(v, cap) + 1) : (uint32_t)(cap + 1);
        out |= o << (8 * j);
      }
    }
    *reinterpret_cast<uint32_t *>((side ? S.rp : S.lp) + ((size_t)b * h + y) * S.pitch + pc0) = out;
  }
}


// The same filter for rows of 16 n pixels on dword-aligned sources (every camera of the reference): 16 padded columns x 4 rows per thread.  The six input rows are
// read as 24 bytes each (one dwordx4 + the dword on either side), the arithmetic runs on pairs of pixels in packed 16-bit lanes (V_PERM_B32 picks the byte pairs:
// the pair (b[4m-1], b[4m]) is the minus operand of pixel pair 4m and the plus operand of pair 4m-2, (b[4m+1], b[4m+2]) the plus operand of 4m and the minus operand
// of 4m+2 -- nine shuffles and eight packed subtractions per input row), and a row of 16 results leaves as one 16-byte store.  Threads are dealt linearly over
// (row group, column chunk), so no lane idles on the 44 chunks of a 704-byte row.  grid: (ceil(n_chunks * n_rowgroups / 256), 1, 2 * batch), block 256
typedef short ps2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ ps2 as_ps2(uint32_t v) { ps2 r; __builtin_memcpy(&r, &v, 4); return r; }
__device__ __forceinline__ uint32_t as_u32(ps2 v) { uint32_t r; __builtin_memcpy(&r, &v, 4); return r; }
__global__ __launch_bounds__(256) void stereo_prefilter16_kernel(StereoDev S, const uint8_t *__restrict__ left, int lstride, size_t l_bstride,
                                                                 const uint8_t *__restrict__ right, int rstride, size_t r_bstride) {
  const int w = S.w, h = S.h, cap = S.cap, nct = S.pitch >> 4, nrg = (h + 3) >> 2;
  const int t = blockIdx.x * 256 + threadIdx.x, b = blockIdx.z >> 1, side = blockIdx.z & 1;
  if (t >= nct * nrg) return;
  const int rg = t / nct, ct = t - rg * nct, y0 = 4 * rg, x0 = 16 * ct - PADL;
  const uint32_t fill = 0x01010101u * (uint32_t)(cap + 1);      // pads, border columns, odd last row
  uint8_t *dst = (side ? S.rp : S.lp) + ((size_t)b * h + y0) * S.pitch + 16 * ct;
  const bool inside = x0 >= 0 && x0 < w;                        // (w is a multiple of 16: a chunk is inside the image or inside a pad)
  uint4 out[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) out[k] = make_uint4(fill, fill, fill, fill);
  if (inside) {
    const uint8_t *src = side ? right + (size_t)b * r_bstride : left + (size_t)b * l_bstride;
    const int stride = side ? rstride : lstride;
    const bool has_l = x0 >= 4, has_r = x0 + 20 <= w;
    ps2 d[6][8];
#pragma unroll
    for (int i = 0; i < 6; ++i) {
      int r = y0 - 1 + i;      // rows outside the image: the row the original's yp / yn pick, i.e. 1 above the top and h-2 below the bottom
      r = r < 0 ? (h > 1 ? 1 : 0) : (r > h - 1 ? (h > 1 ? h - 2 : 0) : r);
      r = min(max(r, 0), h - 1);                                // (rows far below the image only feed rows that are not written)
      const uint8_t *row = src + (size_t)r * stride + x0;
      const uint4 a = *reinterpret_cast<const uint4 *>(row);
      uint32_t W[6];
      W[0] = has_l ? *reinterpret_cast<const uint32_t *>(row - 4) : 0u;      // bytes outside the row only feed border columns, which are overwritten
      W[1] = a.x; W[2] = a.y; W[3] = a.z; W[4] = a.w;
      W[5] = has_r ? *reinterpret_cast<const uint32_t *>(row + 16) : 0u;
      ps2 E[5], O[4];
#pragma unroll
      for (int m = 0; m < 5; ++m) E[m] = as_ps2(__builtin_amdgcn_perm(W[m + 1], W[m], 0x0c040c03u));      // (b[4m-1], b[4m])
#pragma unroll
      for (int m = 0; m < 4; ++m) O[m] = as_ps2(__builtin_amdgcn_perm(0u, W[m + 1], 0x0c020c01u));         // (b[4m+1], b[4m+2])
#pragma unroll
      for (int m = 0; m < 4; ++m) { d[i][2 * m] = O[m] - E[m]; d[i][2 * m + 1] = E[m + 1] - O[m]; }
    }
    const ps2 lo = {(short)-cap, (short)-cap}, hi = {(short)cap, (short)cap}, off = {(short)(cap + 1), (short)(cap + 1)};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      uint32_t o[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        ps2 v[2];
#pragma unroll
        for (int e = 0; e < 2; ++e) {
          const int p = 2 * q + e;
          const ps2 s3 = d[k][p] + d[k + 1][p] + d[k + 1][p] + d[k + 2][p];
          v[e] = __builtin_elementwise_min(__builtin_elementwise_max(s3, lo), hi) + off;
        }
        o[q] = __builtin_amdgcn_perm(as_u32(v[1]), as_u32(v[0]), 0x06040200u);
      }
      if (x0 == 0) o[0] = (o[0] & 0xffffff00u) | (fill & 0x000000ffu);               // column 0
      if (x0 + 16 == w) o[3] = (o[3] & 0x00ffffffu) | (fill & 0xff000000u);          // column w-1
      out[k] = make_uint4(o[0], o[1], o[2], o[3]);
    }
  }
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int y = y0 + k;
    if (y >= h) break;
    *reinterpret_cast<uint4 *>(dst + (size_t)k * S.pitch) = ((h & 1) && y == h - 1) ? make_uint4(fill, fill, fill, fill) : out[k];
  }
}
