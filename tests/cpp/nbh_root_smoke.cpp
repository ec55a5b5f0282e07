// Drives StereoFrontend::setNeighborhoodFromMap of the C++ adaptor (include/scavislam_hip.hpp) on the GPU: a small map with an edge table fed through BackendMap,
// the whole neighbourhood of root 0 built on the device into the front end's candidate list and resident vertex table; tests/test_gpu_nbh_root.py compiles and
// runs it and holds the printed counts against tests/nbh_root_model.py.
// Prints "NBH_ROOT ok <the 13 counts of svs_nbr_result> <vertex ids ...> <act neighbours ...> <point ids of the written head ...>".
// The map: keyframes 0 .. 4 (one noise frame, identity poses), 0 .. 2 in the window; points 0 .. 39, point p anchored in keyframe (p / 4) % 4 and observed by
// keyframe p % 4; edges (0, 1, 9) (2, 0, 7) (1, 2, 7) (3, 1, 5).  The front end keeps keyframe 0 in slot 0 and keyframe 2 in slot 1; the active keyframe is 1;
// newpoint_map: one fixed group and groups keyed by 2, 4 (no vertex: dropped) and 0.
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

  // the map
  BackendMap map(ctx, 16, 256, 1024);
  if (!map.ok()) return 5;
  RegistrationKeyframe k;
  std::memset(&k, 0, sizeof k);
  std::memcpy(k.kf.T_anchor_from_w, I, sizeof I);
  for (int l = 0; l < 3; ++l) { k.kf.pyr[l] = fr.pyr(l); k.kf.stride[l] = fr.stride(l); }
  std::vector<RegistrationKeyframe> kfs(5, k);
  RegistrationFrame f;
  f.table_entry = 0; f.d_disp = fr.disp(); f.disp_stride = fr.stride(0);
  std::memcpy(f.T_from_world, I, sizeof I);
  std::vector<RegistrationFrame> frames(5, f);
  for (int i = 0; i < 5; ++i) { kfs[(size_t)i].frame_id = i; kfs[(size_t)i].in_double_window = false; kfs[(size_t)i].direct_neighbor = false; }
  std::vector<svs_candidate_point> pts(40);
  std::vector<int32_t> op, ok;
  for (int p = 0; p < 40; ++p) {
    svs_candidate_point &c = pts[(size_t)p];
    std::memset(&c, 0, sizeof c);
    c.xyz_anchor[2] = 1.0;
    c.anchor_level = 0; c.kf_index = (p / 4) % 4; c.point_id = p;
    op.push_back(p); ok.push_back(p % 4);
  }
  if (!map.addKeyframes(kfs, frames) || !map.addPoints(pts) || !map.addObservations(op, ok)) { std::puts("NBH_ROOT update refused"); return 6; }
  std::vector<int32_t> window;
  for (int i = 0; i < 3; ++i) window.push_back(i);
  const int32_t pairs[8] = {0, 1, 2, 0, 1, 2, 3, 1}, strength[4] = {9, 7, 7, 5};
  if (!map.setWindow(window) || !map.reserveEdges(8) ||
      !map.addEdges(std::vector<int32_t>(pairs, pairs + 8), std::vector<int32_t>(strength, strength + 4), std::vector<int32_t>(4, 0))) {
    std::puts("NBH_ROOT edges refused");
    return 7;
  }

  StereoFrontend fe(ctx, cam, StereoFrontend::referenceParams(false), 256, 2);
  if (!fe.ok()) return 8;
  for (int slot = 0; slot < 2; ++slot)
    if (!fe.processFirstFrame(left, nullptr, &dimg) || !fe.keepKeyframe(slot, I)) return 9;
  std::vector<int32_t> slots, point_ids, act_neighbors;
  slots.push_back(0); slots.push_back(2);
  std::vector<svs_candidate_point> newpoints(6);
  for (int i = 0; i < 6; ++i) { std::memset(&newpoints[(size_t)i], 0, sizeof(svs_candidate_point)); newpoints[(size_t)i].point_id = 100 + i; newpoints[(size_t)i].kf_index = -1; }
  const int32_t ends[4] = {1, 3, 4, 6}, keys[4] = {-1, 2, 4, 0};
  const std::vector<int32_t> group_end(ends, ends + 4), group_kf(keys, keys + 4);
  std::vector<FrontendVertex> vertex_map;
  svs_nbr_result res;
  if (!fe.setNeighborhoodFromMap(map, 0, 1, slots, newpoints, group_end, 1, group_kf, true, &res, &point_ids, &vertex_map, &act_neighbors)) {
    std::puts("NBH_ROOT call failed");
    return 10;
  }
  if ((int)point_ids.size() != res.n_points || (int)vertex_map.size() != res.n_vertex || (int)act_neighbors.size() != res.n_act_neighbors) { std::puts("NBH_ROOT sizes"); return 11; }
  for (size_t i = 0; i < vertex_map.size(); ++i)
    if (std::memcmp(vertex_map[i].T_me_from_w, I, sizeof I) != 0) { std::puts("NBH_ROOT vertex pose"); return 12; }
  // a root outside the window, and a vertex set that does not fit: false, the list stays
  svs_nbr_result none;
  if (fe.setNeighborhoodFromMap(map, 3, 1, slots, newpoints, group_end, 1, group_kf, true, &none, nullptr, nullptr, nullptr) || !none.root_outside_window) {
    std::puts("NBH_ROOT root outside the window");
    return 13;
  }
  if (fe.setNeighborhoodFromMap(map, 0, 1, slots, newpoints, group_end, 1, group_kf, true, &none, nullptr, nullptr, nullptr, 10, 3) || !none.over_capacity) {
    std::puts("NBH_ROOT capacity");
    return 14;
  }
  // a frame on the list, then the decision on the resident table the call wrote
  double T[12];
  std::memcpy(T, I, sizeof I);
  svs_frame_result fres;
  std::vector<svs_match_result> matches;
  std::vector<svs_gated_point> gated;
  fe.processFrame(left, nullptr, &dimg, T, I, &fres, &matches, &gated);
  if ((int)matches.size() != res.n_points) { std::puts("NBH_ROOT frame"); return 15; }
  std::printf("NBH_ROOT ok %d %d %d %d %d %d %d %d %d %d %d %d %d", res.n_points, res.n_map_points, res.n_vertex, res.n_no_slot, res.over_capacity, res.root_outside_window,
              res.n_root_neighbors, res.n_no_path, res.act_index, res.n_act_neighbors, res.n_head_kept, res.n_head_dropped, res.n_groups);
  for (size_t i = 0; i < vertex_map.size(); ++i) std::printf(" %d", vertex_map[i].frame_id);
  for (size_t i = 0; i < act_neighbors.size(); ++i) std::printf(" %d", act_neighbors[i]);
  for (int i = 0; i < res.n_head_kept; ++i) std::printf(" %d", point_ids[(size_t)i]);
  std::puts("");
  return 0;
}
