// Drives StereoFrontend::addNewPoints / addMorePoints of the C++ adaptor (include/scavislam_hip.hpp) on the GPU and checks that they hand back the records of
// svs_frontend_seed_keyframes called directly; tests/test_gpu_seed.py compiles and runs it.  Prints "SEED ok <first> <more>".
#include <cstdio>
#include <cstring>
#include <vector>

#include "scavislam_hip.hpp"

using namespace scavislam_hip;

static bool same(const std::vector<svs_candidate_point> &a, const svs_candidate_point *b, int n) {
  return (int)a.size() == n && (n == 0 || std::memcmp(a.data(), b, sizeof(svs_candidate_point) * (size_t)n) == 0);
}

int main() {
  Context ctx(0);
  if (!ctx.ok()) { std::puts("NODEVICE"); return 3; }
  const int w = 320, h = 240;
  const svs_cam cam = {285.0, 160.0, 120.0, 0.075, w, h};
  std::vector<uint8_t> img((size_t)w * h);
  std::vector<float> disp((size_t)w * h);
  unsigned s = 12345u;
  for (size_t i = 0; i < img.size(); ++i) { s = s * 1664525u + 1013904223u; img[i] = (uint8_t)(s >> 24); disp[i] = 4.f + (float)((s >> 12) & 7); }
  const svs_frontend_params prm = StereoFrontend::referenceParams(false);
  StereoFrontend fe(ctx, cam, prm, 1024, 2);
  if (!fe.ok()) return 4;
  const Image8 left = {img.data(), w, h, w};
  const ImageF dimg = {disp.data(), w, h, w};
  if (!fe.processFirstFrame(left, nullptr, &dimg)) return 5;
  // addNewPoints against the C call
  svs_seed_params sp = StereoFrontend::seedParams();
  std::vector<svs_candidate_point> first;
  int32_t num_points[3];
  if (!fe.addNewPoints(0, 1, 42u, &first, num_points)) return 6;
  svs_seed_request q;
  std::memset(&q, 0, sizeof q);
  q.mode = SVS_SEED_FIRST; q.kf_index = 0; q.first_point_id = 1; q.seed = 42u;
  q.T_newkey_from_cur[0] = q.T_newkey_from_cur[5] = q.T_newkey_from_cur[10] = 1.0;
  std::vector<svs_candidate_point> direct(528);
  int32_t n[3];
  if (!ctx.check(svs_frontend_seed_keyframes(fe.handle(), 1, &q, &sp, direct.data(), 528, n))) return 7;
  if (!same(first, direct.data(), n[0] + n[1] + n[2]) || num_points[0] != n[0] || num_points[1] != n[1] || num_points[2] != n[2]) { std::puts("SEED first differs"); return 8; }
  // one step on the seeded points, then addMorePoints against the C call (ui.min_num_points raised so that every 3 x 3 cell still asks for points)
  const double I[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};
  double T[12];
  std::memcpy(T, I, sizeof T);
  if (!fe.keepKeyframe(0, I) || !fe.setCandidates(first, (int)first.size())) return 9;
  svs_frame_result res;
  std::vector<svs_match_result> matches;
  std::vector<svs_gated_point> gated;
  fe.processFrame(left, nullptr, &dimg, T, I, &res, &matches, &gated);
  sp.min_num_points = 100000;
  std::vector<svs_candidate_point> more;
  int32_t before[3] = {res.point_stats.num_matched_points[0], res.point_stats.num_matched_points[1], res.point_stats.num_matched_points[2]};
  int32_t np2[3] = {before[0], before[1], before[2]};
  const int next_id = 1 + (int)first.size();
  if (!fe.addMorePoints(1, next_id, 43u, &more, np2, &sp)) return 10;
  q.mode = SVS_SEED_MORE; q.kf_index = 1; q.first_point_id = next_id; q.seed = 43u;
  if (!ctx.check(svs_frontend_seed_keyframes(fe.handle(), 1, &q, &sp, direct.data(), 528, n))) return 11;
  if (!same(more, direct.data(), n[0] + n[1] + n[2]) || np2[0] != before[0] + n[0] || np2[1] != before[1] + n[1] || np2[2] != before[2] + n[2]) { std::puts("SEED more differs"); return 12; }
  for (size_t i = 0; i < more.size(); ++i)
    if (more[i].kf_index != 1 || more[i].point_id != next_id + (int)(more.size() - 1 - i)) { std::puts("SEED more: ids"); return 13; }
  std::printf("SEED ok %zu %zu matched %d\n", first.size(), more.size(), res.n_matched);
  return 0;
}
