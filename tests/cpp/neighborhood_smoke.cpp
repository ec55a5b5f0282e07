// Drives StereoFrontend::setCandidatesFromMap of the C++ adaptor (include/scavislam_hip.hpp) on the GPU: a small map fed through BackendMap, the neighbourhood
// list of a vertex list built on the device into the front end's candidate list, and a frame processed on it; tests/test_gpu_neighborhood.py compiles and runs
// it and holds the printed counts against tests/neighborhood_model.py.
// Prints "NEIGHBORHOOD ok <n_points> <n_map_points> <n_vertex> <n_no_slot> <over_capacity> <vertex ids ...>".
// The map: keyframes 0 .. 3 (one noise frame, identity poses but keyframe 2, which is set by setPoses), points 0 .. 39, point p anchored in keyframe (p / 4) % 4
// and observed by its anchor and by keyframe p % 4.  The front end keeps keyframe 0 in slot 0 and keyframe 2 in slot 1; the vertex list is {2, 0}.
#include <cstdio>
#include <cstring>
#include <vector>

#include "scavislam_hip.hpp"

using namespace scavislam_hip;

int main() {
  Context ctx(0);
  if (!ctx.ok()) { std::puts("NODEVICE"); return 3; }
  const int w = 320, h = 240;
  const svs_cam cam = {285.0, 160.0, 120.0, 0.075, w, h};
  std::vector<uint8_t> img((size_t)w * h);
  std::vector<float> disp((size_t)w * h, 6.f);
  unsigned s = 12345u;
  for (int y = 0; y < h; ++y)
    for (int x = 0; x < w; ++x) { if (x % 4 == 0 && y % 4 == 0) s = s * 1664525u + 1013904223u; img[(size_t)y * w + x] = (uint8_t)(s >> 24); }
  FrameDev fr(ctx, w, h);
  const Image8 left = {img.data(), w, h, w};
  const ImageF dimg = {disp.data(), w, h, w};
  if (!fr.preprocessing(left) || !fr.setDisparity(dimg)) return 4;
  const double I[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};
  double T2[12];
  std::memcpy(T2, I, sizeof I);
  T2[3] = 0.25; T2[11] = -0.5;

  // the map
  BackendMap map(ctx, 16, 256, 1024);
  if (!map.ok()) return 5;
  RegistrationKeyframe k;
  std::memset(&k, 0, sizeof k);
  std::memcpy(k.kf.T_anchor_from_w, I, sizeof I);
  for (int l = 0; l < 3; ++l) { k.kf.pyr[l] = fr.pyr(l); k.kf.stride[l] = fr.stride(l); }
  std::vector<RegistrationKeyframe> kfs(4, k);
  RegistrationFrame f;
  f.table_entry = 0; f.d_disp = fr.disp(); f.disp_stride = fr.stride(0);
  std::memcpy(f.T_from_world, I, sizeof I);
  std::vector<RegistrationFrame> frames(4, f);
  for (int i = 0; i < 4; ++i) { kfs[(size_t)i].frame_id = i; kfs[(size_t)i].in_double_window = true; kfs[(size_t)i].direct_neighbor = false; }
  std::vector<svs_candidate_point> pts(40);
  std::vector<int32_t> op, ok;
  for (int p = 0; p < 40; ++p) {
    svs_candidate_point &c = pts[(size_t)p];
    std::memset(&c, 0, sizeof c);
    const double x = 20 + 7 * p, y = 30 + 4 * p, d = 6.0, z = cam.f * cam.b / d;
    c.xyz_anchor[0] = (x - cam.cx) / cam.f * z; c.xyz_anchor[1] = (y - cam.cy) / cam.f * z; c.xyz_anchor[2] = z;
    c.anchor_obs_pyr[0] = x; c.anchor_obs_pyr[1] = y; c.anchor_obs_pyr[2] = x - d;
    c.anchor_level = 0; c.kf_index = (p / 4) % 4; c.point_id = p;
    op.push_back(p); ok.push_back(p % 4);
    op.push_back(p); ok.push_back((p / 4) % 4);
  }
  if (!map.addKeyframes(kfs, frames) || !map.addPoints(pts) || !map.addObservations(op, ok)) { std::puts("NEIGHBORHOOD update refused"); return 6; }
  if (!map.setPoses(std::vector<int32_t>(1, 2), std::vector<double>(T2, T2 + 12))) return 7;

  // the front end: keyframe 0 in slot 0, keyframe 2 in slot 1 (kept with a pose the back end has moved since)
  StereoFrontend fe(ctx, cam, StereoFrontend::referenceParams(false), 256, 2);
  if (!fe.ok()) return 8;
  for (int slot = 0; slot < 2; ++slot)
    if (!fe.processFirstFrame(left, nullptr, &dimg) || !fe.keepKeyframe(slot, I)) return 9;
  std::vector<int32_t> vertex, slots, point_ids, group_end;
  vertex.push_back(2); vertex.push_back(0);
  slots.push_back(0); slots.push_back(2);
  std::vector<svs_candidate_point> newpoints;
  std::vector<FrontendVertex> vertex_map;
  svs_nbh_result res;
  if (!fe.setCandidatesFromMap(map, vertex, slots, newpoints, group_end, true, &res, &point_ids, &vertex_map)) { std::puts("NEIGHBORHOOD call failed"); return 10; }
  if ((int)point_ids.size() != res.n_points || (int)vertex_map.size() != res.n_vertex) { std::puts("NEIGHBORHOOD sizes"); return 11; }
  for (size_t i = 0; i < point_ids.size(); ++i) {
    const int p = point_ids[i];
    if ((i && p <= point_ids[i - 1]) || (p % 4 != 0 && p % 4 != 2 && (p / 4) % 4 != 0 && (p / 4) % 4 != 2)) { std::puts("NEIGHBORHOOD point ids"); return 12; }
  }
  for (size_t i = 0; i < vertex_map.size(); ++i)
    if (std::memcmp(vertex_map[i].T_me_from_w, vertex_map[i].frame_id == 2 ? T2 : I, sizeof I) != 0) { std::puts("NEIGHBORHOOD vertex pose"); return 13; }
  // over capacity: a vertex set of 4 does not fit 3 entries; the list stays
  svs_nbh_result over;
  if (fe.setCandidatesFromMap(map, vertex, slots, newpoints, group_end, true, &over, nullptr, nullptr, 3) || !over.over_capacity) { std::puts("NEIGHBORHOOD capacity"); return 14; }
  // a frame on the list: the records anchored in slots 0 and 1 are looked for, the others have no anchor
  double T[12];
  std::memcpy(T, I, sizeof I);
  svs_frame_result fres;
  std::vector<svs_match_result> matches;
  std::vector<svs_gated_point> gated;
  fe.processFrame(left, nullptr, &dimg, T, I, &fres, &matches, &gated);
  if ((int)matches.size() != res.n_points) { std::puts("NEIGHBORHOOD frame"); return 15; }
  int no_anchor = 0;
  for (size_t i = 0; i < matches.size(); ++i) no_anchor += matches[i].status == SVS_MATCH_NO_ANCHOR;
  if (no_anchor != res.n_no_slot) { std::printf("NEIGHBORHOOD no-anchor records %d, expected %d\n", no_anchor, res.n_no_slot); return 16; }
  std::printf("NEIGHBORHOOD ok %d %d %d %d %d", res.n_points, res.n_map_points, res.n_vertex, res.n_no_slot, res.over_capacity);
  for (size_t i = 0; i < vertex_map.size(); ++i) std::printf(" %d", vertex_map[i].frame_id);
  std::puts("");
  return 0;
}
