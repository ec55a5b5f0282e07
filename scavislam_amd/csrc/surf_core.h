// surf_core.h -- the arithmetic of svs_surf_extract (include/scavislam_hip.h has the definitions, tests/surf_model.py restates them in NumPy).
// Host + device, arithmetic only: every stage is written as items (a sample, a maximum, a window, a row of the descriptor window, ...) that a caller hands out as
//     for (item = tid; item < n_items; item += nt) ...;  sync();
// surf.hip runs them with the threads of a workgroup and __syncthreads, tests/cpp/surf_host.cpp with tid = 0, nt = 1 and an empty sync: the same expressions in
// the same order, so the f32 / f64 bits are the same wherever an item runs.  Compiled with -ffp-contract=off on both sides.
#pragma once
#include <float.h>
#include <math.h>
#include <stdint.h>

#include "../../include/scavislam_hip.h"

#if defined(__HIPCC__)
#define SURF_HD __host__ __device__ __forceinline__
#else
#define SURF_HD static inline
#endif

constexpr int SURF_ORI_SAMPLES = 113, SURF_ORI_WINDOWS = 72, SURF_PATCH = 20, SURF_MAX_PLANES = 24;
constexpr double SURF_DEG = 57.29577951308232;      // 180 / pi

struct surf_box { int32_t x1, y1, x2, y2; float w; };
// one (octave, layer) plane of responses
struct surf_plane {
  int32_t octave, layer, size, step, margin, rows, cols, samples_i, samples_j, cum;      // cum: samples of the planes before this one
  int64_t off;                                                                          // first element of the plane in an image's det / trace block
  surf_box dx[3], dy[3], dxy[4];
};
// a refined maximum: the record, and what makes the order total
struct surf_cand { float x, y, size, response; int32_t octave, laplacian, layer, ij; };
// the host tables
struct surf_tables { float ori_w[SURF_ORI_SAMPLES]; int8_t ori_x[SURF_ORI_SAMPLES], ori_y[SURF_ORI_SAMPLES]; float dw[SURF_PATCH * SURF_PATCH]; };

SURF_HD int surf_cvround(double v) { return (int)rint(v); }      // round half to even

// ---- host: pattern scaling (resizeHaarPattern) and the Gaussian tables --------------------------------------------------------------------------------------
static inline void surf_scale_pattern(const int src[][5], surf_box *dst, int n, int old_size, int new_size) {
  const float ratio = (float)new_size / old_size;
  for (int k = 0; k < n; ++k) {
    dst[k].x1 = surf_cvround(ratio * src[k][0]); dst[k].y1 = surf_cvround(ratio * src[k][1]);
    dst[k].x2 = surf_cvround(ratio * src[k][2]); dst[k].y2 = surf_cvround(ratio * src[k][3]);
    dst[k].w = src[k][4] / ((float)(dst[k].x2 - dst[k].x1) * (dst[k].y2 - dst[k].y1));
  }
}
static inline void surf_gaussian(int n, double sigma, float *cf) {
  const double scale2 = -0.5 / (sigma * sigma);
  double sum = 0;
  for (int i = 0; i < n; ++i) { const double x = i - (n - 1) * 0.5; cf[i] = (float)exp(scale2 * x * x); sum += cf[i]; }
  sum = 1. / sum;
  for (int i = 0; i < n; ++i) cf[i] = (float)(cf[i] * sum);
}
static inline void surf_make_tables(surf_tables *t) {
  float g[13], d[SURF_PATCH];
  surf_gaussian(13, 2.5, g);
  surf_gaussian(SURF_PATCH, 3.3, d);
  int n = 0;
  for (int i = -6; i <= 6; ++i)
    for (int j = -6; j <= 6; ++j)
      if (i * i + j * j <= 36) { t->ori_x[n] = (int8_t)i; t->ori_y[n] = (int8_t)j; t->ori_w[n++] = g[i + 6] * g[j + 6]; }
  for (int i = 0; i < SURF_PATCH; ++i)
    for (int j = 0; j < SURF_PATCH; ++j) t->dw[i * SURF_PATCH + j] = d[i] * d[j];
}
// the planes of a parameter set; returns their number.  total_samples / plane_elems: sums over the planes
static inline int surf_make_planes(int w, int h, int n_octaves, int n_layers, surf_plane *pl, int *total_samples, int64_t *plane_elems) {
  static const int DX[3][5] = {{0, 2, 3, 7, 1}, {3, 2, 6, 7, -2}, {6, 2, 9, 7, 1}}, DY[3][5] = {{2, 0, 7, 3, 1}, {2, 3, 7, 6, -2}, {2, 6, 7, 9, 1}},
                   DXY[4][5] = {{1, 1, 4, 4, 1}, {5, 1, 8, 4, -1}, {1, 5, 4, 8, -1}, {5, 5, 8, 8, 1}};
  int n = 0, cum = 0;
  int64_t off = 0;
  for (int o = 0; o < n_octaves; ++o)
    for (int l = 0; l < n_layers + 2; ++l) {
      surf_plane &p = pl[n++];
      p.octave = o; p.layer = l; p.size = (9 + 6 * l) << o; p.step = 1 << o; p.margin = (p.size / 2) / p.step;
      p.rows = h / p.step; p.cols = w / p.step;
      p.samples_i = 1 + (h - p.size) / p.step; p.samples_j = 1 + (w - p.size) / p.step;
      p.cum = cum; p.off = off;
      cum += p.samples_i * p.samples_j; off += (int64_t)p.rows * p.cols;
      surf_scale_pattern(DX, p.dx, 3, 9, p.size); surf_scale_pattern(DY, p.dy, 3, 9, p.size); surf_scale_pattern(DXY, p.dxy, 4, 9, p.size);
    }
  *total_samples = cum; *plane_elems = off;
  return n;
}

// ---- responses ------------------------------------------------------------------------------------------------------------------------------------------------
// calcHaarPattern: S points at the integral image's element of the sample's origin, sw = w + 1
SURF_HD float surf_haar(const int32_t *S, int sw, const surf_box *b, int n) {
  double d = 0;
  for (int k = 0; k < n; ++k) {
    const int v = S[b[k].y1 * sw + b[k].x1] + S[b[k].y2 * sw + b[k].x2] - S[b[k].y2 * sw + b[k].x1] - S[b[k].y1 * sw + b[k].x2];
    const float t = (float)v * b[k].w;
    d += (double)t;
  }
  return (float)d;
}
SURF_HD void surf_response(const int32_t *integral, int w, const surf_plane &p, int i, int j, float *det, float *trace) {
  const int32_t *S = integral + (int64_t)(i * p.step) * (w + 1) + j * p.step;
  const float dx = surf_haar(S, w + 1, p.dx, 3), dy = surf_haar(S, w + 1, p.dy, 3), dxy = surf_haar(S, w + 1, p.dxy, 4);
  const float a = dx * dy, b = 0.81f * dxy, c = b * dxy;
  const int64_t at = p.off + (int64_t)(i + p.margin) * p.cols + (j + p.margin);
  det[at] = a - c;
  trace[at] = dx + dy;
}

// ---- maxima and refinement ------------------------------------------------------------------------------------------------------------------------------------
// (i, j) of the middle layer m (planes lo, m, hi of one octave); true: *c is a keypoint
SURF_HD bool surf_maximum(const float *det, const float *trace, const surf_plane &lo, const surf_plane &m, const surf_plane &hi, int i, int j, float threshold,
                          surf_cand *c) {
  const int border = (hi.size / 2) / m.step + 1;
  if (i < border || i >= m.rows - border || j < border || j >= m.cols - border) return false;
  const float val = det[m.off + (int64_t)i * m.cols + j];
  if (!(val > threshold)) return false;
  float N9[3][9];
  const surf_plane *pp[3] = {&lo, &m, &hi};
  for (int q = 0; q < 3; ++q)
    for (int r = 0; r < 3; ++r)
      for (int s = 0; s < 3; ++s) N9[q][r * 3 + s] = det[pp[q]->off + (int64_t)(i + r - 1) * m.cols + (j + s - 1)];
  for (int q = 0; q < 3; ++q)
    for (int r = 0; r < 9; ++r)
      if (!(q == 1 && r == 4) && !(val > N9[q][r])) return false;
  const int sum_i = m.step * (i - (m.size / 2) / m.step), sum_j = m.step * (j - (m.size / 2) / m.step);
  const float half = (m.size - 1) * 0.5f;
  float cy = sum_i + half, cx = sum_j + half;
  // interpolateKeypoint, f32 throughout
  float b[3] = {-(N9[1][5] - N9[1][3]) / 2, -(N9[1][7] - N9[1][1]) / 2, -(N9[2][4] - N9[0][4]) / 2};
  const float dxy = (N9[1][8] - N9[1][6] - N9[1][2] + N9[1][0]) / 4, dxs = (N9[2][5] - N9[2][3] - N9[0][5] + N9[0][3]) / 4,
              dys = (N9[2][7] - N9[2][1] - N9[0][7] + N9[0][1]) / 4;
  float A[3][3] = {{N9[1][3] - 2 * N9[1][4] + N9[1][5], dxy, dxs}, {dxy, N9[1][1] - 2 * N9[1][4] + N9[1][7], dys}, {dxs, dys, N9[0][4] - 2 * N9[1][4] + N9[2][4]}};
  // LU with partial pivoting: column r, the FIRST row of the largest |A[q][r]| (q >= r) is the pivot row
  for (int r = 0; r < 3; ++r) {
    int k = r;
    for (int q = r + 1; q < 3; ++q)
      if (fabsf(A[q][r]) > fabsf(A[k][r])) k = q;
    if (!(fabsf(A[k][r]) >= FLT_EPSILON * 10)) return false;      // singular (or NaN): no solution, x = 0
    if (k != r) {
      for (int s = r; s < 3; ++s) { const float t = A[r][s]; A[r][s] = A[k][s]; A[k][s] = t; }
      const float t = b[r]; b[r] = b[k]; b[k] = t;
    }
    const float d = -1 / A[r][r];
    for (int q = r + 1; q < 3; ++q) {
      const float alpha = A[q][r] * d;
      for (int s = r + 1; s < 3; ++s) { const float t = alpha * A[r][s]; A[q][s] = A[q][s] + t; }
      const float t = alpha * b[r]; b[q] = b[q] + t;
    }
    A[r][r] = -d;
  }
  for (int r = 2; r >= 0; --r) {
    float s = b[r];
    for (int q = r + 1; q < 3; ++q) { const float t = A[r][q] * b[q]; s = s - t; }
    b[r] = s * A[r][r];
  }
  const bool ok = (b[0] != 0 || b[1] != 0 || b[2] != 0) && fabsf(b[0]) <= 1 && fabsf(b[1]) <= 1 && fabsf(b[2]) <= 1;
  if (!ok) return false;
  const float tx = b[0] * m.step, ty = b[1] * m.step, ts = b[2] * (m.size - lo.size);
  cx = cx + tx; cy = cy + ty;
  const float tr = trace[m.off + (int64_t)i * m.cols + j];
  c->x = cx; c->y = cy; c->size = (float)surf_cvround((float)m.size + ts); c->response = val;
  c->octave = m.octave; c->laplacian = (tr > 0) - (tr < 0); c->layer = m.layer; c->ij = i * m.cols + j;
  return true;
}
// the total order: a comes before b
SURF_HD bool surf_before(const surf_cand &a, const surf_cand &b) {
  if (a.response != b.response) return a.response > b.response;
  if (a.size != b.size) return a.size > b.size;
  if (a.y != b.y) return a.y < b.y;
  if (a.x != b.x) return a.x < b.x;
  if (a.octave != b.octave) return a.octave < b.octave;
  if (a.layer != b.layer) return a.layer < b.layer;
  return a.ij < b.ij;
}

// ---- disparity filter -----------------------------------------------------------------------------------------------------------------------------------------
SURF_HD bool surf_disparity(const float *disp, int dstride, int w, int h, float x, float y, double *uvu) {
  const double rx = round((double)x), ry = round((double)y);
  if (!(rx >= 0 && rx < w && ry >= 0 && ry < h)) return false;
  const double d = (double)disp[(int64_t)(int)ry * dstride + (int)rx];
  if (!(d > 0)) return false;
  const double u2 = (double)x - d;
  if (!((double)x - u2 > 0)) return false;      // a disparity below half an ulp of x: uvu[0] - uvu[2] = 0, which svs_loop_set_place refuses
  uvu[0] = (double)x; uvu[1] = (double)y; uvu[2] = u2;
  return true;
}

// ---- orientation ------------------------------------------------------------------------------------------------------------------------------------------------
SURF_HD float surf_degrees(float y, float x) {
  double a = atan2((double)y, (double)x) * SURF_DEG;
  if (a < 0) a = a + 360.0;
  return (float)a;
}
struct surf_ori_work { float X[SURF_ORI_SAMPLES], Y[SURF_ORI_SAMPLES]; int32_t A[SURF_ORI_SAMPLES], valid[SURF_ORI_SAMPLES]; float wx[SURF_ORI_WINDOWS], wy[SURF_ORI_WINDOWS];
                      int32_t n; };
SURF_HD int surf_haar_size(float size) { const float s = size * 1.2f / 9.0f; return 2 * surf_cvround(2 * s); }
// returns false: the keypoint is removed.  *angle: the keypoint's angle, *dir: the direction the descriptor window takes (degrees)
template <class Sync>
SURF_HD bool surf_orientation(const int32_t *integral, int w, int h, const surf_tables &tb, float cx, float cy, float size, surf_ori_work &wk, int tid, int nt, Sync sync,
                              float *angle, float *dir) {
  const float s = size * 1.2f / 9.0f;
  const int gws = surf_haar_size(size), sw = w + 1;
  if (h + 1 < gws || w + 1 < gws) return false;
  const int DXS[2][5] = {{0, 0, 2, 4, -1}, {2, 0, 4, 4, 1}}, DYS[2][5] = {{0, 0, 4, 2, 1}, {0, 2, 4, 4, -1}};
  surf_box bx[2], by[2];
  const float ratio = (float)gws / 4;
  for (int k = 0; k < 2; ++k) {
    bx[k].x1 = surf_cvround(ratio * DXS[k][0]); bx[k].y1 = surf_cvround(ratio * DXS[k][1]); bx[k].x2 = surf_cvround(ratio * DXS[k][2]); bx[k].y2 = surf_cvround(ratio * DXS[k][3]);
    bx[k].w = DXS[k][4] / ((float)(bx[k].x2 - bx[k].x1) * (bx[k].y2 - bx[k].y1));
    by[k].x1 = surf_cvround(ratio * DYS[k][0]); by[k].y1 = surf_cvround(ratio * DYS[k][1]); by[k].x2 = surf_cvround(ratio * DYS[k][2]); by[k].y2 = surf_cvround(ratio * DYS[k][3]);
    by[k].w = DYS[k][4] / ((float)(by[k].x2 - by[k].x1) * (by[k].y2 - by[k].y1));
  }
  const float off = (float)(gws - 1) / 2;
  for (int k = tid; k < SURF_ORI_SAMPLES; k += nt) {
    const float fx = tb.ori_x[k] * s, fy = tb.ori_y[k] * s;
    const float px = cx + fx, py = cy + fy;
    const int x = surf_cvround(px - off), y = surf_cvround(py - off);
    const bool in = !(y < 0 || y >= h + 1 - gws || x < 0 || x >= w + 1 - gws);
    wk.valid[k] = in ? 1 : 0;
    if (in) {
      const int32_t *S = integral + (int64_t)y * sw + x;
      const float vx = surf_haar(S, sw, bx, 2), vy = surf_haar(S, sw, by, 2);
      const float X = vx * tb.ori_w[k], Y = vy * tb.ori_w[k];
      wk.X[k] = X; wk.Y[k] = Y; wk.A[k] = surf_cvround(surf_degrees(Y, X));
    }
  }
  sync();
  if (tid == 0) {      // the kept samples move to the front, in order
    int n = 0;
    for (int k = 0; k < SURF_ORI_SAMPLES; ++k)
      if (wk.valid[k]) { wk.X[n] = wk.X[k]; wk.Y[n] = wk.Y[k]; wk.A[n] = wk.A[k]; ++n; }
    wk.n = n;
  }
  sync();
  const int n = wk.n;
  if (n == 0) return false;
  for (int q = tid; q < SURF_ORI_WINDOWS; q += nt) {
    float sx = 0, sy = 0;
    for (int k = 0; k < n; ++k) {
      int d = wk.A[k] - 5 * q;
      d = d < 0 ? -d : d;
      if (d < 30 || d > 330) { sx = sx + wk.X[k]; sy = sy + wk.Y[k]; }
    }
    wk.wx[q] = sx; wk.wy[q] = sy;
  }
  sync();
  float bestx = 0, besty = 0, best = 0;
  for (int q = 0; q < SURF_ORI_WINDOWS; ++q) {      // every thread: the same walk over the same 72 values
    const float a = wk.wx[q] * wk.wx[q], b = wk.wy[q] * wk.wy[q], m = a + b;
    if (m > best) { best = m; bestx = wk.wx[q]; besty = wk.wy[q]; }
  }
  const float d = surf_degrees(besty, bestx);
  float ang = 360.f - d;
  if (fabsf(ang - 360.f) < FLT_EPSILON) ang = 0.f;
  *angle = ang; *dir = d;
  sync();      // wk may be taken again
  return true;
}

// ---- descriptor ------------------------------------------------------------------------------------------------------------------------------------------------
SURF_HD int surf_window_size(float size) { const float s = size * 1.2f / 9.0f; return (int)((SURF_PATCH + 1) * s); }
// INTER_AREA's table for destination index d of 21 over `ssize` sources: calls f(source index, alpha) in table order
template <class F>
SURF_HD void surf_area_taps(int ssize, int d, F f) {
  const double scale = (double)ssize / (SURF_PATCH + 1);
  const double fsx1 = d * scale, fsx2 = fsx1 + scale;
  const double rest = ssize - fsx1, cell = scale < rest ? scale : rest;
  int sx1 = (int)ceil(fsx1), sx2 = (int)floor(fsx2);
  sx2 = sx2 < ssize - 1 ? sx2 : ssize - 1;
  sx1 = sx1 < sx2 ? sx1 : sx2;
  if (sx1 - fsx1 > 1e-3) f(sx1 - 1, (float)((sx1 - fsx1) / cell));
  for (int sx = sx1; sx < sx2; ++sx) f(sx, (float)(1.0 / cell));
  if (fsx2 - sx2 > 1e-3) {
    double a = fsx2 - sx2;
    a = a < 1. ? a : 1.;
    a = a < cell ? a : cell;
    f(sx2, (float)(a / cell));
  }
}
// work arrays of one keypoint: win_[win * win] u8, buf[win * 21] f32, patch[21 * 21] i32, dx / dy[400], vec[64], scale[1]
struct surf_desc_work { uint8_t *win; float *buf; int32_t *patch; float *dx, *dy, *vec, *scale; };
SURF_HD size_t surf_desc_work_bytes(int win) {
  return (((size_t)win * win + 15) & ~(size_t)15) + (size_t)win * (SURF_PATCH + 1) * 4 + (SURF_PATCH + 1) * (SURF_PATCH + 1) * 4 + 2 * SURF_PATCH * SURF_PATCH * 4 + 64 * 4 + 16;
}
SURF_HD surf_desc_work surf_desc_work_at(uint8_t *p, int win) {
  surf_desc_work k;
  k.win = p; p += ((size_t)win * win + 15) & ~(size_t)15;
  k.buf = (float *)p; p += (size_t)win * (SURF_PATCH + 1) * 4;
  k.patch = (int32_t *)p; p += (SURF_PATCH + 1) * (SURF_PATCH + 1) * 4;
  k.dx = (float *)p; p += SURF_PATCH * SURF_PATCH * 4;
  k.dy = (float *)p; p += SURF_PATCH * SURF_PATCH * 4;
  k.vec = (float *)p; p += 64 * 4;
  k.scale = (float *)p;
  return k;
}
template <class Sync>
SURF_HD void surf_descriptor(const uint8_t *img, int stride, int w, int h, const surf_tables &tb, float cx, float cy, float size, float dir_deg, surf_desc_work wk, int tid,
                             int nt, Sync sync, float *out) {
  constexpr int P1 = SURF_PATCH + 1;
  const int win = surf_window_size(size);
  const float dir = dir_deg * (float)(3.141592653589793 / 180);
  const float sin_dir = (float)sin((double)dir), cos_dir = (float)cos((double)dir);
  const float win_offset = -(float)(win - 1) / 2;
  for (int i = tid; i < win; i += nt) {      // a row of the window: the reference's running f32 sums, i steps down, then along the row
    const float a = win_offset * cos_dir, b = win_offset * sin_dir;
    float start_x = cx + a, start_y = cy - b;
    start_x = start_x + b; start_y = start_y + a;
    for (int k = 0; k < i; ++k) { start_x = start_x + sin_dir; start_y = start_y + cos_dir; }
    float px = start_x, py = start_y;
    for (int j = 0; j < win; ++j) {
      int x = surf_cvround(px), y = surf_cvround(py);
      x = x < 0 ? 0 : (x > w - 1 ? w - 1 : x);
      y = y < 0 ? 0 : (y > h - 1 ? h - 1 : y);
      wk.win[i * win + j] = img[(int64_t)y * stride + x];
      px = px + cos_dir; py = py - sin_dir;
    }
  }
  sync();
  for (int it = tid; it < win * P1; it += nt) {      // horizontal pass
    const int sy = it / P1, d = it - sy * P1;
    float acc = 0;
    const uint8_t *row = wk.win + sy * win;
    surf_area_taps(win, d, [&](int si, float alpha) { const float t = (float)row[si] * alpha; acc = acc + t; });
    wk.buf[it] = acc;
  }
  sync();
  for (int it = tid; it < P1 * P1; it += nt) {      // vertical pass, round half to even, saturate
    const int dy = it / P1, d = it - dy * P1;
    float acc = 0;
    surf_area_taps(win, dy, [&](int si, float beta) { const float t = beta * wk.buf[si * P1 + d]; acc = acc + t; });
    int v = surf_cvround(acc);
    wk.patch[it] = v < 0 ? 0 : (v > 255 ? 255 : v);
  }
  sync();
  for (int it = tid; it < SURF_PATCH * SURF_PATCH; it += nt) {
    const int i = it / SURF_PATCH, j = it - i * SURF_PATCH;
    const int32_t *p = wk.patch;
    const float dw = tb.dw[it];
    wk.dx[it] = (float)(p[i * P1 + j + 1] - p[i * P1 + j] + p[(i + 1) * P1 + j + 1] - p[(i + 1) * P1 + j]) * dw;
    wk.dy[it] = (float)(p[(i + 1) * P1 + j] - p[i * P1 + j] + p[(i + 1) * P1 + j + 1] - p[i * P1 + j + 1]) * dw;
  }
  sync();
  for (int c = tid; c < 16; c += nt) {      // a 5 x 5 cell in raster order
    const int ci = c / 4, cj = c - ci * 4;
    float v0 = 0, v1 = 0, v2 = 0, v3 = 0;
    for (int y = ci * 5; y < ci * 5 + 5; ++y)
      for (int x = cj * 5; x < cj * 5 + 5; ++x) {
        const float tx = wk.dx[y * SURF_PATCH + x], ty = wk.dy[y * SURF_PATCH + x];
        v0 = v0 + tx; v1 = v1 + ty; v2 = v2 + fabsf(tx); v3 = v3 + fabsf(ty);
      }
    wk.vec[4 * c] = v0; wk.vec[4 * c + 1] = v1; wk.vec[4 * c + 2] = v2; wk.vec[4 * c + 3] = v3;
  }
  sync();
  if (tid == 0) {
    double mag = 0;
    for (int k = 0; k < 64; ++k) { const float t = wk.vec[k] * wk.vec[k]; mag += (double)t; }
    wk.scale[0] = (float)(1. / (sqrt(mag) + DBL_EPSILON));
  }
  sync();
  for (int k = tid; k < 64; k += nt) out[k] = wk.vec[k] * wk.scale[0];
  sync();
}
