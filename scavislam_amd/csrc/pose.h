// pose.h -- SE3 as 12 row-major doubles (3 x 4, [R | t]): act on a point, multiply, invert.  One definition for every kernel that moves a pose or a point.
// Evaluation order is the oracle's and part of the contract: a row is (a0 * b0 + a1 * b1) + a2 * b2, the translation is added last.  The units that hold their
// results to the oracle bit for bit are built with contraction off; ba.hip (contraction on, 1e-6 bar) uses the same text.
#pragma once
#include "common.h"

namespace {

// (a, b, c) = T * (x0, x1, x2); the outputs must not be the inputs.  (The inputs are references, not values: inlined, every caller then compiles to the
// instructions its own spelling of the three rows gave.)
__device__ __forceinline__ void pose_act(const double *T, const double &x0, const double &x1, const double &x2, double &a, double &b, double &c) {
  a = T[0] * x0 + T[1] * x1 + T[2] * x2 + T[3];
  b = T[4] * x0 + T[5] * x1 + T[6] * x2 + T[7];
  c = T[8] * x0 + T[9] * x1 + T[10] * x2 + T[11];
}
// y = T * x (y may be x)
__device__ __forceinline__ void pose_act(const double *T, const double *x, double *y) {
  double a, b, c;
  pose_act(T, x[0], x[1], x[2], a, b, c);
  y[0] = a; y[1] = b; y[2] = c;
}
// C = A * B (C may be A or B)
__device__ __forceinline__ void pose_mul(const double *A, const double *B, double *C) {
  double t[12];
#pragma unroll
  for (int i = 0; i < 3; ++i) {
#pragma unroll
    for (int j = 0; j < 4; ++j) t[4 * i + j] = A[4 * i] * B[j] + A[4 * i + 1] * B[4 + j] + A[4 * i + 2] * B[8 + j];
    t[4 * i + 3] += A[4 * i + 3];
  }
#pragma unroll
  for (int i = 0; i < 12; ++i) C[i] = t[i];
}
// B = A^-1 = [R^T | -R^T t] (B may be A)
__device__ __forceinline__ void pose_inv(const double *A, double *B) {
  double t[12];
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) t[4 * i + j] = A[4 * j + i];
#pragma unroll
  for (int i = 0; i < 3; ++i) t[4 * i + 3] = -(t[4 * i] * A[3] + t[4 * i + 1] * A[7] + t[4 * i + 2] * A[11]);
#pragma unroll
  for (int i = 0; i < 12; ++i) B[i] = t[i];
}

}  // namespace
