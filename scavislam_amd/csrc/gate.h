// gate.h -- the stereo reprojection residual and the gate inequality on it, shared by motion.hip (calcFastMotionOnly, processMatchedPoints) and register.hip
// (keyframesToRegister / globalLoopClosure): one definition, identical bits.
#pragma once
#include "common.h"
#include "pose.h"

namespace {
// f = obs - map_uvu(T xyz) (stereo_camera.cpp:37-44); J = SE3XYZ_STEREO::frameJac (transformations.h:424-447) if wanted
template <bool JAC>
__device__ __forceinline__ void mo_residual(const double *T, const svs_match_result &o, const svs_cam &cam, double *f, double *J) {
  const double *q = o.xyz_actkey;
  double x, y, z;
  pose_act(T, q[0], q[1], q[2], x, y, z);
  const double fl = cam.f;
  // the three quotients share z: one checked reciprocal (div_rn_guarded, devutil.h) -- the bits of x / z, y / z, (x - b) / z for every operand, which is what lets
  // register.hip's gate and the loop-closure check keep this one definition
  const double num[3] = {x, y, x - cam.b};
  double p[3];
  div_rn_guarded(num, z, p);
  f[0] = o.obs[0] - (p[0] * fl + cam.cx);
  f[1] = o.obs[1] - (p[1] * fl + cam.cy);
  f[2] = o.obs[2] - (p[2] * fl + cam.cx);
  if (JAC) {
    const double ibz = 1. / z, ibz2 = 1. / (z * z);
    const double A = -fl * ibz, B = -fl * ibz, C = fl * x * ibz2, D = fl * y * ibz2, E = fl * (x - cam.b) * ibz2;
    J[0] = A; J[1] = 0; J[2] = C; J[3] = y * C; J[4] = z * A - x * C; J[5] = -y * A;
    J[6] = 0; J[7] = B; J[8] = D; J[9] = -z * B + y * D; J[10] = -x * D; J[11] = x * B;
    J[12] = A; J[13] = 0; J[14] = E; J[15] = y * E; J[16] = z * A - x * E; J[17] = -y * A;
  }
}
}  // namespace
// |uvu - map_uvu(T xyz)| < max_reproj_error * 2^level (u, v), < 3 max_reproj_error (u_right): stereo_frontend.cpp:869-871, backend.cpp:644-646, :928-930;
// d = the residual above, factor = zeroFromPyr_i(1, anchor_level) as an int, mre a float.  A macro, so that both users compile the very expression (an inline
// function turns the short-circuit chain of processMatchedPoints' kernels into other code)
#define SVS_GATE_PASSES(d, factor, mre) (fabs((d)[0]) < (mre) * (factor) && fabs((d)[1]) < (mre) * (factor) && fabs((d)[2]) < 3. * (mre))
