// StereoFrontend::setVertexTable / decideKeyframes of include/scavislam_hip.hpp through plain g++ -std=c++11: the refusals of the setter, the refusal of a decision
// without a table, and a decision behind a step that matched nothing (tracking_ok = 0: the record comes back zeroed, the lists empty).
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "scavislam_hip.hpp"

#define CHECK(c) do { if (!(c)) { std::printf("FAILED %s:%d %s\n", __FILE__, __LINE__, #c); return 1; } } while (0)

int main() {
  using namespace scavislam_hip;
  Context ctx(0);
  CHECK(ctx.ok());
  const int w = 320, h = 240;
  svs_cam cam = {285.0, 160.0, 120.0, 0.075, w, h};
  StereoFrontend fe(ctx, cam, StereoFrontend::referenceParams(false), 64, 2);
  CHECK(fe.ok());
  std::vector<uint8_t> img((size_t)w * h), nxt((size_t)w * h);
  unsigned s = 12345u;
  for (size_t i = 0; i < img.size(); ++i) { s = s * 1664525u + 1013904223u; img[i] = (uint8_t)(s >> 24); }
  for (int y = 0; y < h; ++y)
    for (int x = 0; x < w; ++x) nxt[(size_t)y * w + x] = img[(size_t)y * w + (x + 2 < w ? x + 2 : w - 1)];
  std::vector<float> disp((size_t)w * h, 8.f);
  Image8 left = {img.data(), w, h, w}, left2 = {nxt.data(), w, h, w};
  ImageF d = {disp.data(), w, h, w};
  double I[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0}, T[12];
  CHECK(fe.processFirstFrame(left, nullptr, &d));
  CHECK(fe.keepKeyframe(0, I));
  CHECK(fe.setCandidates(std::vector<svs_candidate_point>(), 0));
  for (int i = 0; i < 12; ++i) T[i] = I[i];
  svs_frame_result res;
  std::vector<svs_match_result> matches;
  std::vector<svs_gated_point> gated;
  CHECK(!fe.processFrame(left2, nullptr, &d, T, I, &res, &matches, &gated));      // nothing to match: matchAndTrack returns false
  CHECK(res.tracking_ok == 0 && res.dense_passes >= 1);

  svs_keyframe_decision dec;
  std::vector<svs_map_new_point> new_points;
  std::vector<svs_map_track_point> track_points;
  std::vector<int32_t> new_rec, track_rec;
  CHECK(!fe.decideKeyframes(nullptr, &dec, &new_points, &track_points, &new_rec, &track_rec));      // no vertex table yet

  std::vector<FrontendVertex> vm(2);
  vm[0].frame_id = 7; vm[1].frame_id = 9;
  for (int i = 0; i < 12; ++i) { vm[0].T_me_from_w[i] = I[i]; vm[1].T_me_from_w[i] = I[i]; }
  vm[1].T_me_from_w[3] = 0.1;
  std::vector<std::vector<int32_t> > feats(2);
  feats[1].push_back(3); feats[1].push_back(5);
  std::vector<char> from_map(2, 0);
  std::vector<int32_t> nbrs(1, 1), slots(2, -1);
  slots[0] = 7;
  CHECK(!fe.setVertexTable(vm, feats, from_map, 2, nbrs, slots));                 // act out of range
  nbrs[0] = 0;
  CHECK(!fe.setVertexTable(vm, feats, from_map, 0, nbrs, slots));                 // a neighbour equal to act
  nbrs[0] = 1; slots[1] = 9;
  CHECK(!fe.setVertexTable(vm, feats, from_map, 0, nbrs, slots));                 // slot 1 was never kept
  slots[1] = -1; feats[1][1] = 3;
  CHECK(!fe.setVertexTable(vm, feats, from_map, 0, nbrs, slots));                 // ids not strictly ascending
  feats[1][1] = 5; vm[1].frame_id = 7;
  CHECK(!fe.setVertexTable(vm, feats, from_map, 0, nbrs, slots));                 // an id twice
  vm[1].frame_id = 9;
  CHECK(fe.setVertexTable(vm, feats, from_map, 0, nbrs, slots));

  std::memset(&dec, 0xff, sizeof dec);
  CHECK(fe.decideKeyframes(nullptr, &dec, &new_points, &track_points, &new_rec, &track_rec, true));
  const unsigned char *b = reinterpret_cast<const unsigned char *>(&dec);
  for (size_t i = 0; i < sizeof dec; ++i) CHECK(b[i] == 0);                       // not tracked: valid = 0, everything zero
  CHECK(new_points.empty() && track_points.empty() && new_rec.empty() && track_rec.empty());
  svs_keyframe_decide_params p = StereoFrontend::decideParams();
  CHECK(p.parallax_thr == 0.75f && p.switch_min_shared == 100 && p.covis_thr == 15 && p.min_num_points == 25 && p.max_av_track_length == 75.0);
  std::puts("KEYFRAME OK");
  return 0;
}
