// rectify.hip -- the arithmetic between the camera and processFrame: FrameGrabber::processNextFrame's three per-pixel input conversions
// (frame_grabber.cpp:125-186).
//   colour -> gray      cv::cvtColor(CV_BGR2GRAY) on the left image (:140-147)
//   rectification       rectifyFrame() = cv::remap(CV_INTER_LINEAR) on left and right (:245-256), CV_16SC2 maps of cv::initUndistortRectifyMap
//                       (intializeRectifier, frame_grabber-impl.cpp:93-134)
//   depth -> disparity  depthToDisp() (frame_grabber-impl.cpp:136-152, stereo_camera.cpp:55-59)
// Integer / short float pipelines with one well-defined result each: bit-exact to the OpenCV 2.4 semantics restated in tests/rectify_model.py
// (not pinned by the reference's binaries, like pyrDown / FAST / StereoBM).
#include "common.h"
#include <math.h>
#include <vector>

// ---- svs_rectify_build_maps: host only, f64, built without contraction; the operation order is the definition (tests/rectify_model.py) ----------------
extern "C" int svs_rectify_build_maps(const double *K, const double *dist, const double *R, const double *Knew, int w, int h, int16_t *map_xy,
                                      uint16_t *map_frac) {
  if (!K || !dist || !R || !Knew || !map_xy || !map_frac || w < 1 || h < 1) return SVS_ERR_INVALID;
  double M[9];
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c) M[3 * r + c] = (Knew[3 * r] * R[c] + Knew[3 * r + 1] * R[3 + c]) + Knew[3 * r + 2] * R[6 + c];
  const double a = M[0], b = M[1], c = M[2], d = M[3], e = M[4], f = M[5], g = M[6], hh = M[7], i = M[8];
  const double A = e * i - f * hh, B = c * hh - b * i, C = b * f - c * e;
  const double D = f * g - d * i, E = a * i - c * g, F = c * d - a * f;
  const double G = d * hh - e * g, H = b * g - a * hh, I = a * e - b * d;
  const double det = (a * A + b * D) + c * G;
  if (!(det != 0.0)) return SVS_ERR_INVALID;
  const double iR[9] = {A / det, B / det, C / det, D / det, E / det, F / det, G / det, H / det, I / det};
  const double k1 = dist[0], k2 = dist[1], p1 = dist[2], p2 = dist[3], k3 = dist[4];
  const double fx = K[0], fy = K[4], u0 = K[2], v0 = K[5];
  for (int row = 0; row < h; ++row) {
    for (int col = 0; col < w; ++col) {
      const double jj = (double)col, ii = (double)row;
      const double X = (jj * iR[0] + ii * iR[1]) + iR[2];
      const double Y = (jj * iR[3] + ii * iR[4]) + iR[5];
      const double W = (jj * iR[6] + ii * iR[7]) + iR[8];
      const double x = X / W, y = Y / W;
      const double x2 = x * x, y2 = y * y;
      const double r2 = x2 + y2, _2xy = (2.0 * x) * y;
      const double kr = 1.0 + ((k3 * r2 + k2) * r2 + k1) * r2;
      const double u = fx * ((x * kr + p1 * _2xy) + p2 * (r2 + 2.0 * x2)) + u0;
      const double v = fy * ((y * kr + p1 * (r2 + 2.0 * y2)) + p2 * _2xy) + v0;
      const long long iu = (long long)rint(u * 32.0), iv = (long long)rint(v * 32.0);      // ties to even (default rounding mode)
      const size_t o = (size_t)row * w + col;
      map_xy[2 * o] = (int16_t)(uint16_t)(uint64_t)(iu >> 5);
      map_xy[2 * o + 1] = (int16_t)(uint16_t)(uint64_t)(iv >> 5);
      map_frac[o] = (uint16_t)((iv & 31) * 32 + (iu & 31));
    }
  }
  return SVS_OK;
}

// ---- the rectifier ------------------------------------------------------------------------------------------------------------------------------------
// A map entry is repacked at create time into ONE word: [31:21] y0 + 1, [20:10] x0 + 1, [9:5] fy, [4:0] fx.  An entry with a tap inside has x0 in [-1, w - 1] and
// y0 in [-1, h - 1]; every other entry (all four taps outside, whatever its int16 values) becomes RECT_ALL_OUT, which decodes to x0 = y0 = 2046: outside every
// frame the handle accepts (w, h <= 2046), so the per-tap test below needs no case of its own for it.
constexpr uint32_t RECT_ALL_OUT = 0xffffffffu;
constexpr int RECT_MAX_DIM = 2046;
constexpr int RECT_TILE_W = 64, RECT_TILE_H = 16;      // output pixels per 256-lane workgroup: 16 lanes x 4 pixels wide, 16 rows

struct svs_rectify {
  svs_ctx *ctx = nullptr;
  int w = 0, h = 0, max_batch = 0;
  DevBuf<uint32_t> d_map[2];      // left, right: [h][w] packed words; nullptr = no remap for that side
  ~svs_rectify() { if (ctx) (void)hipStreamSynchronize(ctx->stream); }      // (runs before the maps are freed, also when create gives up)
};

static int rect_pack_upload(svs_rectify *r, int side, const int16_t *xy, const uint16_t *frac) {
  svs_ctx *ctx = r->ctx;
  const size_t n = (size_t)r->w * r->h;
  std::vector<uint32_t> pk(n);
  for (size_t o = 0; o < n; ++o) {
    SVS_REQUIRE(ctx, frac[o] <= 1023);
    const int x0 = xy[2 * o], y0 = xy[2 * o + 1];
    pk[o] = (x0 < -1 || x0 > r->w - 1 || y0 < -1 || y0 > r->h - 1) ? RECT_ALL_OUT : ((uint32_t)(y0 + 1) << 21) | ((uint32_t)(x0 + 1) << 10) | frac[o];
  }
  SVS_HIP(ctx, r->d_map[side].alloc(n));
  SVS_HIP(ctx, hipMemcpy(r->d_map[side], pk.data(), n * sizeof(uint32_t), hipMemcpyHostToDevice));
  return SVS_OK;
}

extern "C" int svs_rectify_destroy(svs_rectify *r) {
  if (!r) return SVS_OK;
  delete r;
  return SVS_OK;
}

extern "C" int svs_rectify_create(svs_ctx *ctx, int w, int h, int max_batch, const int16_t *h_left_xy, const uint16_t *h_left_frac, const int16_t *h_right_xy,
                                  const uint16_t *h_right_frac, svs_rectify **out) {
  SVS_REQUIRE(ctx, ctx && out && w >= 4 && h >= 1 && w % 4 == 0 && w <= RECT_MAX_DIM && h <= RECT_MAX_DIM && max_batch >= 1);
  SVS_REQUIRE(ctx, (h_left_xy != nullptr) == (h_left_frac != nullptr) && (h_right_xy != nullptr) == (h_right_frac != nullptr));
  SVS_DEVICE(ctx);
  std::unique_ptr<svs_rectify> r(new svs_rectify());
  r->ctx = ctx; r->w = w; r->h = h; r->max_batch = max_batch;
  if (h_left_xy) if (int rc = rect_pack_upload(r.get(), 0, h_left_xy, h_left_frac)) return rc;
  if (h_right_xy) if (int rc = rect_pack_upload(r.get(), 1, h_right_xy, h_right_frac)) return rc;
  *out = r.release();
  return SVS_OK;
}

// CV_BGR2GRAY, 14-bit fixed point
__device__ __forceinline__ uint32_t rect_gray(uint32_t b, uint32_t g, uint32_t r) { return (1868u * b + 9617u * g + 4899u * r + 8192u) >> 14; }

// one output pixel.  INSIDE: the caller knows that all four taps of every lane of the wave are inside -- the two taps of a source row are one load (gray: 2 bytes;
// BGR: 6 bytes as a dword and a ushort, never a byte beyond the second tap).  Otherwise: a load per tap from a clamped address, 0 where the tap is outside (BORDER_CONSTANT
// per tap).  BGR taps go to gray first: bit for bit gray-then-remap, because gray is per pixel.
template <int CH, bool INSIDE>
__device__ __forceinline__ uint32_t rect_pixel(const uint8_t *__restrict__ src, int ss, int w, int h, uint32_t m) {
  const uint32_t fx = m & 31u, fy = (m >> 5) & 31u;
  const int x0 = (int)((m >> 10) & 2047u) - 1, y0 = (int)(m >> 21) - 1;
  uint32_t p00, p01, p10, p11;
  if (INSIDE) {
    const uint8_t *q = src + (size_t)y0 * ss + CH * x0;
    if (CH == 1) {
      const uint32_t t0 = ld_unaligned<uint16_t>(q), t1 = ld_unaligned<uint16_t>(q + ss);
      p00 = t0 & 255u; p01 = t0 >> 8; p10 = t1 & 255u; p11 = t1 >> 8;
    } else {
      const uint32_t a0 = ld_unaligned<uint32_t>(q), b0 = ld_unaligned<uint16_t>(q + 4), a1 = ld_unaligned<uint32_t>(q + ss), b1 = ld_unaligned<uint16_t>(q + ss + 4);
      p00 = rect_gray(a0 & 255u, (a0 >> 8) & 255u, (a0 >> 16) & 255u); p01 = rect_gray(a0 >> 24, b0 & 255u, b0 >> 8);
      p10 = rect_gray(a1 & 255u, (a1 >> 8) & 255u, (a1 >> 16) & 255u); p11 = rect_gray(a1 >> 24, b1 & 255u, b1 >> 8);
    }
  } else {
    uint32_t p[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const int xs = x0 + (t & 1), ys = y0 + (t >> 1);
      const bool ok = (unsigned)xs < (unsigned)w && (unsigned)ys < (unsigned)h;
      const uint8_t *q = src + (size_t)min(max(ys, 0), h - 1) * ss + CH * min(max(xs, 0), w - 1);      // always inside the image
      const uint32_t v = CH == 1 ? (uint32_t)q[0] : rect_gray(q[0], q[1], q[2]);
      p[t] = ok ? v : 0u;
    }
    p00 = p[0]; p01 = p[1]; p10 = p[2]; p11 = p[3];
  }
  // cv::remap's 15-bit weight table is 32 x these products, its rounding term 2^14: the same quotient
  return ((32u - fx) * (32u - fy) * p00 + fx * (32u - fy) * p01 + (32u - fx) * fy * p10 + fx * fy * p11 + 512u) >> 10;
}

// grid = tiles x stream slabs.  The maps are the same for every stream: a lane reads the four map words of its four adjacent output pixels ONCE and keeps them in
// registers over the slab's streams; per stream it gathers the taps (neighbouring lanes' taps are neighbours in the source: L1 serves them) and stores one dword.
// Tiles in XCD-contiguous order: neighbouring tiles of one slab share source lines.
template <int CH>
__global__ __launch_bounds__(256) void rectify_remap_kernel(const uint8_t *__restrict__ src, int ss, size_t sb, const uint32_t *__restrict__ map, int w, int h,
                                                           uint8_t *__restrict__ dst, int ds, size_t db, int n_batch, int slab, int tiles_x, int n_tiles, int swz) {
  unsigned id = blockIdx.x;
  if (swz) id = xcd_contiguous(id, gridDim.x);
  const int sl = (int)(id / (unsigned)n_tiles), tile = (int)(id % (unsigned)n_tiles);
  const int ty = tile / tiles_x, tx = tile - ty * tiles_x;
  const int x = tx * RECT_TILE_W + (int)(threadIdx.x & 15u) * 4, y = ty * RECT_TILE_H + (int)(threadIdx.x >> 4);
  if (x >= w || y >= h) return;                                        // (w % 4 == 0: a lane's four pixels are inside together)
  const uint4 mv = *reinterpret_cast<const uint4 *>(map + (size_t)y * w + x);
  const uint32_t m[4] = {mv.x, mv.y, mv.z, mv.w};
  bool in = true;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const uint32_t x1 = (m[k] >> 10) & 2047u, y1 = m[k] >> 21;
    in = in && x1 >= 1u && x1 < (uint32_t)w && y1 >= 1u && y1 < (uint32_t)h;
  }
  const bool all_in = __all(in);                                       // wave-uniform: every smooth lens map's interior
  const int b0 = sl * slab, b1 = min(b0 + slab, n_batch);
  const uint8_t *s = src + (size_t)b0 * sb;
  uint8_t *d = dst + (size_t)b0 * db + (size_t)y * ds + x;
  if (all_in) {
#pragma unroll 2
    for (int b = b0; b < b1; ++b, s += sb, d += db) {
      uint32_t o = 0;
#pragma unroll
      for (int k = 0; k < 4; ++k) o |= rect_pixel<CH, true>(s, ss, w, h, m[k]) << (8 * k);
      *reinterpret_cast<uint32_t *>(d) = o;
    }
  } else {
    for (int b = b0; b < b1; ++b, s += sb, d += db) {
      uint32_t o = 0;
#pragma unroll
      for (int k = 0; k < 4; ++k) o |= rect_pixel<CH, false>(s, ss, w, h, m[k]) << (8 * k);
      *reinterpret_cast<uint32_t *>(d) = o;
    }
  }
}

// no maps for this side: conversion (BGR) or copy (gray) only -- newcollege.cfg's case, colour but already rectified.  A lane: 4 adjacent pixels, one dword store.
template <int CH>
__global__ __launch_bounds__(256) void rectify_convert_kernel(const uint8_t *__restrict__ src, int ss, size_t sb, int w, int h, uint8_t *__restrict__ dst, int ds,
                                                             size_t db) {
  const int item = (int)(blockIdx.x * 256u + threadIdx.x), ncol = w >> 2;
  if (item >= ncol * h) return;
  const int y = item / ncol, x = 4 * (item - y * ncol);
  const uint8_t *q = src + (size_t)blockIdx.y * sb + (size_t)y * ss + CH * x;
  uint32_t o;
  if (CH == 1) o = ld_unaligned<uint32_t>(q);
  else {
    const uint32_t a = ld_unaligned<uint32_t>(q), b = ld_unaligned<uint32_t>(q + 4), c = ld_unaligned<uint32_t>(q + 8);      // B0 G0 R0 B1 | G1 R1 B2 G2 | R2 B3 G3 R3
    o = rect_gray(a & 255u, (a >> 8) & 255u, (a >> 16) & 255u) | rect_gray(a >> 24, b & 255u, (b >> 8) & 255u) << 8 |
        rect_gray((b >> 16) & 255u, b >> 24, c & 255u) << 16 | rect_gray((c >> 8) & 255u, (c >> 16) & 255u, c >> 24) << 24;
  }
  *reinterpret_cast<uint32_t *>(dst + (size_t)blockIdx.y * db + (size_t)y * ds + x) = o;
}

static int rect_side(svs_rectify *r, const uint32_t *d_map, const uint8_t *src, int ss, size_t sb, int ch, uint8_t *dst, int ds, size_t db, int n_batch) {
  svs_ctx *ctx = r->ctx;
  const int w = r->w, h = r->h;
  SVS_REQUIRE(ctx, src && dst && (ch == 1 || ch == 3) && ss >= ch * w && ds >= w && ds % 4 == 0 && db % 4 == 0 && ((uintptr_t)dst & 3) == 0);
  SVS_REQUIRE(ctx, n_batch == 1 || (sb >= (size_t)ss * (h - 1) + (size_t)ch * w && db >= (size_t)ds * (h - 1) + w));
  if (!d_map) {
    const dim3 grid(div_up((w >> 2) * h, 256), n_batch), block(256);
    if (ch == 1) hipLaunchKernelGGL(rectify_convert_kernel<1>, grid, block, 0, ctx->stream, src, ss, sb, w, h, dst, ds, db);
    else hipLaunchKernelGGL(rectify_convert_kernel<3>, grid, block, 0, ctx->stream, src, ss, sb, w, h, dst, ds, db);
  } else {
    const int tiles_x = div_up(w, RECT_TILE_W), n_tiles = tiles_x * div_up(h, RECT_TILE_H);
    // streams per workgroup: as many as leave the device a few thousand workgroups (a small batch keeps one stream per workgroup), at most 8
    const int slab = std::max(1, std::min(8, (int)((long long)n_batch * n_tiles / 4096)));
    const dim3 grid((unsigned)n_tiles * (unsigned)div_up(n_batch, slab)), block(256);
    if (ch == 1) hipLaunchKernelGGL(rectify_remap_kernel<1>, grid, block, 0, ctx->stream, src, ss, sb, d_map, w, h, dst, ds, db, n_batch, slab, tiles_x, n_tiles, ctx->xcd_swizzle);
    else hipLaunchKernelGGL(rectify_remap_kernel<3>, grid, block, 0, ctx->stream, src, ss, sb, d_map, w, h, dst, ds, db, n_batch, slab, tiles_x, n_tiles, ctx->xcd_swizzle);
  }
  SVS_LAUNCH_CHECK(ctx);
  return SVS_OK;
}

extern "C" int svs_rectify_frames(svs_rectify *r, const svs_raw_frames_dev *raw, uint8_t *d_left_out, int lstride, size_t l_bstride, uint8_t *d_right_out,
                                  int rstride, size_t r_bstride, int n_batch) {
  svs_ctx *ctx = r ? r->ctx : nullptr;
  SVS_REQUIRE(ctx, r && raw && raw->d_left && d_left_out && n_batch >= 1 && n_batch <= r->max_batch);
  SVS_REQUIRE(ctx, (raw->d_right != nullptr) == (d_right_out != nullptr));
  SVS_REQUIRE(ctx, raw->d_right || !r->d_map[1]);                       // right maps without a right image: not the disparity-given case this handle was made for
  SVS_DEVICE(ctx);
  if (raw->ready_event) SVS_HIP(ctx, hipStreamWaitEvent(ctx->stream, static_cast<hipEvent_t>(raw->ready_event), 0));
  if (int rc = rect_side(r, r->d_map[0], raw->d_left, raw->lstride, raw->l_bstride, raw->left_channels, d_left_out, lstride, l_bstride, n_batch)) return rc;
  if (raw->d_right)
    if (int rc = rect_side(r, r->d_map[1], raw->d_right, raw->rstride, raw->r_bstride, 1, d_right_out, rstride, r_bstride, n_batch)) return rc;
  return SVS_OK;
}

// ---- depthToDisp --------------------------------------------------------------------------------------------------------------------------------------
// float depth = d16 * (float)(1./5000.); float scaled = f / depth (in double, f double); return scaled / b (in double).  d16 == 0 gives +inf, as the reference does.
__device__ __forceinline__ float rect_depth_to_disp(uint32_t d16, double f, double b) {
  const float depth = (float)d16 * (float)(1. / 5000.);
  const float sd = (float)(f / (double)depth);
  return (float)((double)sd / b);
}
__global__ __launch_bounds__(256) void depth_to_disp_kernel(const uint16_t *__restrict__ src, int ss, size_t sb, int w, int h, float *__restrict__ dst, int ds, size_t db,
                                                           double f, double b, int vec) {
  const int item = (int)(blockIdx.x * 256u + threadIdx.x), ncol = (w + 3) >> 2;
  if (item >= ncol * h) return;
  const int y = item / ncol, x = 4 * (item - y * ncol);
  const uint16_t *q = src + (size_t)blockIdx.y * sb + (size_t)y * ss + x;
  float *o = dst + (size_t)blockIdx.y * db + (size_t)y * ds + x;
  if (vec && x + 3 < w) {
    const uint2 v = *reinterpret_cast<const uint2 *>(q);
    *reinterpret_cast<float4 *>(o) = make_float4(rect_depth_to_disp(v.x & 0xffffu, f, b), rect_depth_to_disp(v.x >> 16, f, b), rect_depth_to_disp(v.y & 0xffffu, f, b),
                                                 rect_depth_to_disp(v.y >> 16, f, b));
  } else {
    for (int k = 0; k < 4 && x + k < w; ++k) o[k] = rect_depth_to_disp(q[k], f, b);
  }
}
extern "C" int svs_depth_to_disp(svs_ctx *ctx, const svs_cam *cam, const uint16_t *d_depth16, int stride, size_t bstride, float *d_disp, int dstride, size_t d_bstride,
                                 int n_batch) {
  SVS_REQUIRE(ctx, ctx && cam && d_depth16 && d_disp && cam->w >= 1 && cam->h >= 1 && stride >= cam->w && dstride >= cam->w && n_batch >= 1);
  SVS_REQUIRE(ctx, n_batch == 1 || (bstride >= (size_t)stride * (cam->h - 1) + cam->w && d_bstride >= (size_t)dstride * (cam->h - 1) + cam->w));
  SVS_DEVICE(ctx);
  const int w = cam->w, h = cam->h;
  const int vec = stride % 4 == 0 && bstride % 4 == 0 && ((uintptr_t)d_depth16 & 7) == 0 && dstride % 4 == 0 && d_bstride % 4 == 0 && ((uintptr_t)d_disp & 15) == 0;
  const dim3 grid(div_up(div_up(w, 4) * h, 256), n_batch), block(256);
  hipLaunchKernelGGL(depth_to_disp_kernel, grid, block, 0, ctx->stream, d_depth16, stride, bstride, w, h, d_disp, dstride, d_bstride, cam->f, cam->b, vec);
  SVS_LAUNCH_CHECK(ctx);
  return SVS_OK;
}
