// subpix_core.h -- the arithmetic of the matcher's sub-pixel refinement (GuidedMatcher::subpixelAccuracy, matcher.cpp:241-309: a 2-D Gauss-Newton alignment of the
// current 8 x 8 patch to the warped key patch; the reference keeps the body behind `#if 0`).  Arithmetic only, host + device: match_subpix.inc runs it one lane per
// pixel, tests/cpp/subpix_host.cpp as loops on the host, and tests/subpix_model.py restates it in NumPy; the three agree bit for bit.  Both sides compile it with
// -ffp-contract=off: every product and every sum below is rounded on its own.
//   K[iy][ix], ix, iy = 0 .. 9    the key patch with its border: warpAffinve at half size 5 (matcher.cpp:403-458); K[1..8][1..8] is the matcher's KEY_PATCH
//   pixel (h, w), h, w = 0 .. 7   sits at K[h+1][w+1]; in the wave it is lane 8 h + w
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define SVS_SPX_HD __host__ __device__ __forceinline__
#else
#define SVS_SPX_HD static inline
#endif

// cv::Sobel with ksize 1 and scale 0.5 (matcher.cpp:259-266): the central difference of two key pixels, exact in f32 (a multiple of 1/2 below 128)
SVS_SPX_HD float svs_spx_grad(int k_plus, int k_minus) { return 0.5f * ((float)k_plus - (float)k_minus); }

// one axis of warp2d's sample position for pixel index i (w or h) at offset p, in the reference's patch coordinates (matcher.cpp:232-233 with interpolateMat_8u,
// maths_utils.cpp:67-86): *off = the first tap's distance from the match (u or v), *s = the weight of the second tap.  |p| <= 2 keeps off in -6 .. 5
SVS_SPX_HD void svs_spx_axis(float p, int i, int *off, float *s) {
  const float xf = p + (float)(i + 1);
  const float x0 = floorf(xf);
  *s = xf - x0;
  *off = (int)x0 - 5;
}
// interpolateMat_8u's value: v00 = (y, x), v01 = (y + 1, x), v10 = (y, x + 1), v11 = (y + 1, x + 1); f32, left to right
SVS_SPX_HD float svs_spx_bilinear(float sx, float sy, int v00, int v01, int v10, int v11) {
  const float wx0 = 1.f - sx, wx1 = sx, wy0 = 1.f - sy, wy1 = sy;
  return (wx0 * wy0) * (float)v00 + (wx0 * wy1) * (float)v01 + (wx1 * wy0) * (float)v10 + (wx1 * wy1) * (float)v11;
}

// the Gauss-Newton step from the normal matrix (H00, H01, H11; det = H00 H11 - H01^2 > 0) and the right-hand side: f64, every product rounded on its own, then
// cast to f32.  (A declared departure: the reference's dead code solves with Eigen's f32 ldlt.)
SVS_SPX_HD double svs_spx_det(double H00, double H01, double H11) { return H00 * H11 - H01 * H01; }
SVS_SPX_HD void svs_spx_step(double H00, double H01, double H11, double det, double b0, double b1, float *dx, float *dy) {
  *dx = (float)(-(H11 * b0 - H01 * b1) / det);
  *dy = (float)(-(H00 * b1 - H01 * b0) / det);
}

enum { SVS_SPX_GO_ON = 0, SVS_SPX_CONVERGED, SVS_SPX_OUT };
// p <- p + delta in f32.  SVS_SPX_OUT: the new offset leaves [-max_shift, max_shift]^2 (or is a NaN), p is left alone; SVS_SPX_CONVERGED: taken, and the step was
// below eps on both axes
SVS_SPX_HD int svs_spx_update(float *px, float *py, float dx, float dy, float max_shift, float eps) {
  const float nx = *px + dx, ny = *py + dy;
  if (!(fabsf(nx) <= max_shift && fabsf(ny) <= max_shift)) return SVS_SPX_OUT;
  *px = nx; *py = ny;
  return fabsf(dx) < eps && fabsf(dy) < eps ? SVS_SPX_CONVERGED : SVS_SPX_GO_ON;
}

// the refined position of one axis on the match's level, and the pixel whose disparity createObervation reads for it (truncation, matcher-impl.cpp:38-41)
SVS_SPX_HD void svs_spx_position(int u, float p, float *nu, int *iu) {
  *nu = (float)u + p;
  *iu = (int)*nu;
}
// createObervation (matcher-impl.cpp:33-51) of the f32 position (nu, nv) of level lvl: the sibling of match_observation (match_wave.inc), which takes the integer
// corner.  disp = the level-0 disparity at ((int)nv << lvl, (int)nu << lvl).  false: no disparity there, the observation is left alone
SVS_SPX_HD bool svs_spx_observation(float nu, float nv, int lvl, float disp, double *o0, double *o1, double *o2) {
  const double inv_factor = 1.0 / (double)(1 << lvl);
  const double d = disp * inv_factor;
  if (!(d > 0)) return false;
  const double sc = (double)(1 << lvl);
  *o0 = nu * sc; *o1 = nv * sc; *o2 = (nu - d) * sc;
  return true;
}
