// lm6.h -- the 6x6 step of the front end's Levenberg-Marquardt loops (f64): solve and SE3 update exp(x) * T, each in two spellings.
//  * d_solve6 / d_se3_exp_mul: one lane, out of line -- the record-walking refinement kernel (motion.hip) and the full-resolution tracker (dense_full.hip), whose
//    LM step runs on one lane while the workgroup waits;
//  * wave_solve6 / mo2_exp_mul: seven lanes of a wave, everything in registers (broadcasts: lane_bcast, devutil.h) -- the quarter-grid tracker (dense.hip) and the
//    fused refinement kernel (motion.hip).
// Included by translation units built with contraction off.  ba.hip has its own SE3 exponential (ba_solve.inc: power series, built with contraction on) and does not
// include this header.
#pragma once
#include "common.h"

namespace {

// 6x6 solve by Gaussian elimination with partial pivoting (stands in for Eigen's ldlt(), as in the oracle).  Fully unrolled
// with compile-time indices: the row exchange is a chain of predicated swaps, so the augmented matrix lives in registers
// (a dynamically indexed copy would sit in scratch memory, and this runs on one lane while the workgroup waits).
__device__ void d_solve6(const double *A, const double *b, double *x) {
  double M[6][7];
#pragma unroll
  for (int i = 0; i < 6; ++i) {
#pragma unroll
    for (int j = 0; j < 6; ++j) M[i][j] = A[i * 6 + j];
    M[i][6] = b[i];
  }
#pragma unroll
  for (int k = 0; k < 6; ++k) {
    int p = k;
    double best = fabs(M[k][k]);
#pragma unroll
    for (int i = k + 1; i < 6; ++i) { const double v = fabs(M[i][k]); if (v > best) { best = v; p = i; } }
#pragma unroll
    for (int i = k + 1; i < 6; ++i) {
      const bool sw = p == i;
#pragma unroll
      for (int j = k; j < 7; ++j) { const double a = M[k][j], c = M[i][j]; M[k][j] = sw ? c : a; M[i][j] = sw ? a : c; }
    }
    const double piv = M[k][k];
#pragma unroll
    for (int i = k + 1; i < 6; ++i) {
      const double f = M[i][k] / piv;
#pragma unroll
      for (int j = k; j < 7; ++j) M[i][j] -= f * M[k][j];
    }
  }
#pragma unroll
  for (int i = 5; i >= 0; --i) {
    double s_ = M[i][6];
#pragma unroll
    for (int j = i + 1; j < 6; ++j) s_ -= M[i][j] * x[j];
    x[i] = s_ / M[i][i];
  }
}
__device__ void d_se3_exp_mul(const double *x, const double *T, double *Tn) {   // Tn = exp(x) * T
  const double *w = x + 3;
  double th2 = w[0] * w[0] + w[1] * w[1] + w[2] * w[2], th = sqrt(th2);
  double W[9] = {0, -w[2], w[1], w[2], 0, -w[0], -w[1], w[0], 0}, W2[9], R[9], V[9];
  for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) W2[3 * i + j] = W[3 * i] * W[j] + W[3 * i + 1] * W[3 + j] + W[3 * i + 2] * W[6 + j];
  double a, b;
  if (th < 1e-10) { a = 1.0 - th2 / 6.0; b = 0.5 - th2 / 24.0; } else { a = sin(th) / th; b = (1.0 - cos(th)) / th2; }
  for (int i = 0; i < 9; ++i) R[i] = a * W[i] + b * W2[i];
  R[0] += 1; R[4] += 1; R[8] += 1;
  if (th < 1e-10) { for (int i = 0; i < 9; ++i) V[i] = R[i]; }
  else {
    double c = (1.0 - cos(th)) / th2, d = (th - sin(th)) / (th2 * th);
    for (int i = 0; i < 9; ++i) V[i] = c * W[i] + d * W2[i];
    V[0] += 1; V[4] += 1; V[8] += 1;
  }
  double t[3];
  for (int i = 0; i < 3; ++i) t[i] = V[3 * i] * x[0] + V[3 * i + 1] * x[1] + V[3 * i + 2] * x[2];
  for (int i = 0; i < 3; ++i) {
    for (int j = 0; j < 4; ++j) Tn[4 * i + j] = R[3 * i] * T[j] + R[3 * i + 1] * T[4 + j] + R[3 * i + 2] * T[8 + j];
    Tn[4 * i + 3] += t[i];
  }
}

// A x = b for a symmetric positive definite 6x6 system on seven lanes of a wave: lane c < 6 holds column c of A in col[0..6), lane 6 holds b.
// Gauss-Jordan, the multipliers of a step broadcast from the pivot column's lane; no pivoting (the reference's ldlt() pivots, which an SPD matrix
// does not need).  Every lane returns x in x[0..6).
__device__ __forceinline__ void wave_solve6(const double (&col)[6], double (&x)[6]) {
  double a[6];
#pragma unroll
  for (int r = 0; r < 6; ++r) a[r] = col[r];
#pragma unroll
  for (int k = 0; k < 6; ++k) {
    const double ip = 1.0 / lane_bcast(a[k], k);
    const double ak = a[k] * ip;               // row k of this lane's column, scaled
#pragma unroll
    for (int r = 0; r < 6; ++r) {
      if (r == k) continue;
      const double m = lane_bcast(a[r], k);     // element (r, k) of the pivot column
      a[r] -= m * ak;
    }
    a[k] = ak;
  }
#pragma unroll
  for (int r = 0; r < 6; ++r) x[r] = lane_bcast(a[r], 6);
}
// exp(x) * T with everything in registers (d_se3_exp_mul above is an out-of-line call on arrays in scratch memory)
__device__ __forceinline__ void mo2_exp_mul(const double (&x)[6], const double (&T)[12], double (&Tn)[12]) {
  const double w0 = x[3], w1 = x[4], w2 = x[5];
  const double th2 = w0 * w0 + w1 * w1 + w2 * w2, th = sqrt(th2);
  // a = sin(th) / th, b = c = (1 - cos th) / th^2, d = (th - sin th) / th^3.  An LM step rotates by far less than half a radian: there the three
  // are even power series in th^2 (9 terms: remainder < 1e-22), no square root, no division, no libm call on the chain of the trial
  double a, b, c, d;
  if (th2 < 0.25) {
    // Horner in th^2 with the coefficients 1 / (k + 1)! written out (a table would live in scratch memory)
#define SVS_IF(k) (1.0 / k)
    const double t = th2;
    a = 1.0 - t * (SVS_IF(6.) - t * (SVS_IF(120.) - t * (SVS_IF(5040.) - t * (SVS_IF(362880.) - t * (SVS_IF(39916800.) - t * (SVS_IF(6227020800.) - t * (SVS_IF(1307674368000.) -
        t * (SVS_IF(355687428096000.) - t * SVS_IF(121645100408832000.)))))))));
    b = SVS_IF(2.) - t * (SVS_IF(24.) - t * (SVS_IF(720.) - t * (SVS_IF(40320.) - t * (SVS_IF(3628800.) - t * (SVS_IF(479001600.) - t * (SVS_IF(87178291200.) -
        t * (SVS_IF(20922789888000.) - t * (SVS_IF(6402373705728000.) - t * SVS_IF(2432902008176640000.)))))))));
    d = SVS_IF(6.) - t * (SVS_IF(120.) - t * (SVS_IF(5040.) - t * (SVS_IF(362880.) - t * (SVS_IF(39916800.) - t * (SVS_IF(6227020800.) - t * (SVS_IF(1307674368000.) -
        t * (SVS_IF(355687428096000.) - t * (SVS_IF(121645100408832000.) - t * SVS_IF(51090942171709440000.)))))))));
#undef SVS_IF
    c = b;
  } else {
    double sn, cs;
    sincos(th, &sn, &cs);
    const double ith2 = 1.0 / th2;
    a = sn / th; b = (1.0 - cs) * ith2; c = b; d = (th - sn) * ith2 / th;
  }
  // W = hat(w), W2 = W * W
  const double W[9] = {0, -w2, w1, w2, 0, -w0, -w1, w0, 0};
  double W2[9], R[9], V[9];
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) W2[3 * i + j] = W[3 * i] * W[j] + W[3 * i + 1] * W[3 + j] + W[3 * i + 2] * W[6 + j];
#pragma unroll
  for (int i = 0; i < 9; ++i) { R[i] = a * W[i] + b * W2[i]; V[i] = c * W[i] + d * W2[i]; }
  R[0] += 1; R[4] += 1; R[8] += 1;
  V[0] += 1; V[4] += 1; V[8] += 1;
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    const double t = V[3 * i] * x[0] + V[3 * i + 1] * x[1] + V[3 * i + 2] * x[2];
#pragma unroll
    for (int j = 0; j < 4; ++j) Tn[4 * i + j] = R[3 * i] * T[j] + R[3 * i + 1] * T[4 + j] + R[3 * i + 2] * T[8 + j];
    Tn[4 * i + 3] += t;
  }
}

}  // namespace
