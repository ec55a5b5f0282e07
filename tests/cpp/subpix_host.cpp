// The arithmetic of the sub-pixel refinement (scavislam_amd/csrc/subpix_core.h) compiled for the host, with the wave's orchestration (match_subpix.inc) as loops:
// lane = pixel 8 h + w, the butterfly as a balanced tree over the pixel index.  tests/test_subpix_cpu.py holds it to tests/subpix_model.py bit for bit.
// Build: g++ -O2 -ffp-contract=off -shared -fPIC
#include "../../scavislam_amd/csrc/subpix_core.h"

namespace {
double tree_sum(double *x) {
  for (int n = 64; n > 1; n >>= 1)
    for (int i = 0; i < n / 2; ++i) x[i] = x[2 * i] + x[2 * i + 1];
  return x[0];
}
}  // namespace

// n records of one level.  K: [n][100] key patches (K[iy][ix] at 10 iy + ix); cimg: the level's current image (W x H, rows cstride apart); disp: the level-0
// disparity (rows dstride apart); uv: [n][2]; status_io [n], obs_io [n][3]: the records' fields, rewritten as svs_match_subpixel rewrites them;
// info_f [n][2] = dx, dy; info_i [n][2] = n_iter, state (0 REFINED, 2 SINGULAR, 3 SHIFT, 4 NO_DISP).  Every record is taken as SVS_MATCH_OK.
extern "C" void svs_host_subpix(int n, const uint8_t *K, const uint8_t *cimg, int cstride, int W, int H, const float *disp, int dstride, int lvl, const int32_t *uv,
                                int iterations, float max_shift, float eps, int32_t *status_io, double *obs_io, float *info_f, int32_t *info_i) {
  for (int r = 0; r < n; ++r) {
    const uint8_t *k = K + 100 * (size_t)r;
    const int u = uv[2 * r], v = uv[2 * r + 1];
    int state = 3, n_iter = 0;
    float px = 0.f, py = 0.f;
    if (u >= 6 && v >= 6 && u < W - 6 && v < H - 6) {
      float gx[64], gy[64];
      double H00 = 0, H01 = 0, H11 = 0;
      for (int h = 0; h < 8; ++h)
        for (int w = 0; w < 8; ++w) {
          const int i = 8 * h + w;
          gx[i] = svs_spx_grad(k[10 * (h + 1) + w + 2], k[10 * (h + 1) + w]);
          gy[i] = svs_spx_grad(k[10 * (h + 2) + w + 1], k[10 * h + w + 1]);
          H00 += (double)gx[i] * gx[i]; H01 += (double)gx[i] * gy[i]; H11 += (double)gy[i] * gy[i];
        }
      const double det = svs_spx_det(H00, H01, H11);
      if (!(det > 0)) state = 2;
      else {
        state = 0;
        for (int it = 1; it <= iterations; ++it) {
          double t0[64], t1[64];
          for (int h = 0; h < 8; ++h)
            for (int w = 0; w < 8; ++w) {
              int ox, oy;
              float sx, sy;
              svs_spx_axis(px, w, &ox, &sx);
              svs_spx_axis(py, h, &oy, &sy);
              const uint8_t *t = cimg + (size_t)(v + oy) * cstride + (u + ox);
              const float d = svs_spx_bilinear(sx, sy, t[0], t[cstride], t[1], t[cstride + 1]) - (float)k[10 * (h + 1) + w + 1];
              t0[8 * h + w] = (double)gx[8 * h + w] * (double)d;
              t1[8 * h + w] = (double)gy[8 * h + w] * (double)d;
            }
          float dx, dy;
          svs_spx_step(H00, H01, H11, det, tree_sum(t0), tree_sum(t1), &dx, &dy);
          n_iter = it;
          const int rc = svs_spx_update(&px, &py, dx, dy, max_shift, eps);
          if (rc == SVS_SPX_OUT) state = 3;
          if (rc != SVS_SPX_GO_ON) break;
        }
        if (state == 0) {
          float nu, nv;
          int iu, iv;
          svs_spx_position(u, px, &nu, &iu);
          svs_spx_position(v, py, &nv, &iv);
          double o0, o1, o2;
          if (!svs_spx_observation(nu, nv, lvl, disp[(size_t)(iv << lvl) * dstride + (iu << lvl)], &o0, &o1, &o2)) { state = 4; status_io[r] = 6; }
          else { obs_io[3 * r] = o0; obs_io[3 * r + 1] = o1; obs_io[3 * r + 2] = o2; }
        } else px = py = 0.f;
      }
    }
    info_f[2 * r] = px; info_f[2 * r + 1] = py; info_i[2 * r] = n_iter; info_i[2 * r + 1] = state;
  }
}
