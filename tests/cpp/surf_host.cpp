// Host mirror of the orchestration around scavislam_amd/csrc/surf_core.h (surf.hip: svs_surf_extract): the items every kernel hands to its threads run here as
// plain loops (tid = 0, nt = 1, an empty sync).  Built as a shared library by tests/test_surf_cpu.py and driven from NumPy: what it returns must equal
// tests/surf_model.py bit for bit, so the arithmetic the device compiles is held to the model without a device.
#include <stdint.h>
#include <string.h>
#include <algorithm>
#include <vector>

#include "../../scavislam_amd/csrc/surf_core.h"

namespace {
struct no_sync { void operator()() const {} };
}

extern "C" {
void svs_host_surf_tables(float *ori_w, float *dw) {
  surf_tables tb;
  surf_make_tables(&tb);
  memcpy(ori_w, tb.ori_w, sizeof tb.ori_w);
  memcpy(dw, tb.dw, sizeof tb.dw);
}

// returns the number of kept keypoints; *n_maxima: refined maxima before the truncation to max_kp.  det_out / trace_out (optional): the planes, plane after plane
int svs_host_surf_extract(const uint8_t *img, int stride, int w, int h, const float *disp, int dstride, float threshold, int n_octaves, int n_layers, int max_kp,
                          svs_surf_keypoint *kp_out, double *uvu_out, float *desc_out, int *n_maxima, float *det_out, float *trace_out) {
  surf_plane planes[SURF_MAX_PLANES] = {};
  int total_samples = 0;
  int64_t plane_elems = 0;
  const int np = surf_make_planes(w, h, n_octaves, n_layers, planes, &total_samples, &plane_elems);
  surf_tables tb;
  surf_make_tables(&tb);
  std::vector<int32_t> S((size_t)(w + 1) * (h + 1), 0);
  for (int y = 0; y < h; ++y) {
    int acc = 0;
    for (int x = 0; x < w; ++x) { acc += img[(size_t)y * stride + x]; S[(size_t)(y + 1) * (w + 1) + x + 1] = S[(size_t)y * (w + 1) + x + 1] + acc; }
  }
  std::vector<float> det((size_t)plane_elems, 0.f), trace((size_t)plane_elems, 0.f);
  for (int p = 0; p < np; ++p)
    for (int i = 0; i < planes[p].samples_i; ++i)
      for (int j = 0; j < planes[p].samples_j; ++j) surf_response(S.data(), w, planes[p], i, j, det.data(), trace.data());
  if (det_out) memcpy(det_out, det.data(), det.size() * sizeof(float));
  if (trace_out) memcpy(trace_out, trace.data(), trace.size() * sizeof(float));
  std::vector<surf_cand> cand;
  for (int o = 0; o < n_octaves; ++o)
    for (int l = 1; l <= n_layers; ++l) {
      const int p = o * (n_layers + 2) + l;
      for (int i = 0; i < planes[p].rows; ++i)
        for (int j = 0; j < planes[p].cols; ++j) {
          surf_cand c;
          if (surf_maximum(det.data(), trace.data(), planes[p - 1], planes[p], planes[p + 1], i, j, threshold, &c)) cand.push_back(c);
        }
    }
  *n_maxima = (int)cand.size();
  std::sort(cand.begin(), cand.end(), [](const surf_cand &a, const surf_cand &b) { return surf_before(a, b); });
  const int n = std::min((int)cand.size(), max_kp);
  surf_ori_work ow;
  int largest = (9 + 6 * (n_layers + 1)) << (n_octaves - 1);
  std::vector<uint8_t> work(surf_desc_work_bytes(surf_window_size((float)largest)) + 64);
  int kept = 0;
  for (int k = 0; k < n; ++k) {
    const surf_cand &c = cand[k];
    double u[3] = {(double)c.x, (double)c.y, (double)c.x};
    if (disp && !surf_disparity(disp, dstride, w, h, c.x, c.y, u)) continue;
    float angle = 0.f, dir = 0.f;
    if (!surf_orientation(S.data(), w, h, tb, c.x, c.y, c.size, ow, 0, 1, no_sync(), &angle, &dir)) continue;
    surf_descriptor(img, stride, w, h, tb, c.x, c.y, c.size, dir, surf_desc_work_at(work.data(), surf_window_size(c.size)), 0, 1, no_sync(), desc_out + (size_t)kept * 64);
    svs_surf_keypoint &o = kp_out[kept];
    o.x = c.x; o.y = c.y; o.size = c.size; o.angle = angle; o.response = c.response; o.octave = c.octave; o.laplacian = c.laplacian; o.pad_ = 0;
    for (int q = 0; q < 3; ++q) uvu_out[3 * (size_t)kept + q] = u[q];
    ++kept;
  }
  return kept;
}
}
