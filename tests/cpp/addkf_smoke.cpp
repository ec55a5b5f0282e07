// Drives the C++ adaptor's keyframe insertion (include/scavislam_hip.hpp) on the GPU: BackendMap::addFirstKeyframe and BackendMap::addKeyframe, which is
// SlamGraph::addKeyframe in one device call; tests/test_gpu_add_keyframe.py compiles and runs it.  Prints "ADDKF ok <keyframes> <new neighbours> <points> <strength>".
// Keyframe 20 is the first; 21 brings 30 new points anchored in 20 and no track point, so the new points' counts stand (30 >= covis_thr 15); 22 brings 30 points
// anchored in 21 and tracks the first 30 in the order (left, top), (right, top), (left, bottom), (right, bottom), ...: with h = 7 the four classes cross at the
// entries 12, 13, 12 and 14, so 20 and 21 keep the 16 entries from 14 onwards.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "scavislam_hip.hpp"

using namespace scavislam_hip;

int main() {
  Context ctx(0);
  if (!ctx.ok()) { std::puts("NODEVICE"); return 3; }
  const svs_cam cam = {285.0, 160.0, 120.0, 0.075, 320, 240};
  void *d_any = nullptr;      // the insertion never reads a pyramid or a disparity
  if (!ctx.check(svs_malloc(ctx.get(), 4096, &d_any))) return 4;
  RegistrationKeyframe kf;
  RegistrationFrame frame;
  std::memset(&kf.kf, 0, sizeof kf.kf);
  for (int l = 0; l < 3; ++l) { kf.kf.pyr[l] = static_cast<const uint8_t *>(d_any); kf.kf.stride[l] = 64; }
  kf.in_double_window = false; kf.direct_neighbor = false;
  frame.table_entry = 0; frame.d_disp = static_cast<const float *>(d_any); frame.disp_stride = 64;
  std::memset(frame.T_from_world, 0, sizeof frame.T_from_world);

  BackendMap map(ctx, 64, 1024, 4096);
  if (!map.ok() || !map.reserveEdges(16)) { std::puts("ADDKF create refused"); return 5; }
  kf.frame_id = 20;
  if (!map.addFirstKeyframe(kf, frame)) { std::puts("ADDKF addFirstKeyframe refused"); return 6; }
  if (map.addFirstKeyframe(kf, frame)) { std::puts("ADDKF a second first keyframe was taken"); return 7; }

  const int N = 30, covis_thr = 15;
  BackendMap::AddKeyframeResult res;
  int strength = 0;
  for (int step = 0; step < 2; ++step) {
    const int oldkey = 20 + step, newkey = 21 + step;
    std::vector<svs_map_new_point> np((size_t)N);
    for (int i = 0; i < N; ++i) {
      svs_map_new_point &p = np[(size_t)i];
      std::memset(&p, 0, sizeof p);
      p.xyz_anchor[0] = 0.05 * (i - 15); p.xyz_anchor[1] = 0.03 * (i % 7 - 3); p.xyz_anchor[2] = 4.0 + 0.1 * i;
      p.anchor_obs_pyr[0] = 40.0 + i; p.anchor_obs_pyr[1] = 30.0 + i; p.anchor_obs_pyr[2] = 35.0 + i;
      p.feat_center[0] = 80.0 + 2 * i; p.feat_center[1] = 60.0 + 2 * i; p.feat_center[2] = 70.0 + 2 * i;
      p.point_id = 300 + 100 * step + i; p.anchor_id = oldkey; p.anchor_level = i % 3; p.feat_level = (i + 1) % 3;
    }
    std::vector<svs_map_track_point> tp;
    for (int i = 0; step == 1 && i < N; ++i) {
      svs_map_track_point t;
      t.center[0] = (i % 2) ? 300.0 : 20.0; t.center[1] = (i % 4 < 2) ? 10.0 : 200.0; t.center[2] = t.center[0] - 3.0;
      t.global_id = 300 + i; t.level = 0;
      tp.push_back(t);
    }
    std::vector<int32_t> window;
    for (int k = 20; k <= oldkey; ++k) window.push_back(k);
    const double T_rel[12] = {1, 0, 0, 0.01, 0, 1, 0, -0.02, 0, 0, 1, -0.3};
    kf.frame_id = newkey;
    if (!map.setWindow(window) || !map.addKeyframe(oldkey, kf, frame, T_rel, np, tp, covis_thr, cam, &res)) { std::printf("ADDKF addKeyframe %d refused\n", newkey); return 8; }
    if (res.over_capacity || res.new_neighbors.size() != (size_t)(step + 1) || res.constraints.size() != res.new_neighbors.size() || !res.missing.empty()) {
      std::printf("ADDKF step %d: %zu neighbours, %zu missing\n", step, res.new_neighbors.size(), res.missing.size()); return 9;
    }
    for (size_t e = 0; e < res.constraints.size(); ++e)
      if (res.constraints[e].status != SVS_CONS_OK || res.constraints[e].strength < N) { std::printf("ADDKF step %d edge %zu: status %d strength %d\n", step, e, res.constraints[e].status, res.constraints[e].strength); return 10; }
    for (size_t i = 0; i < res.new_kept.size(); ++i) if (!res.new_kept[i]) { std::puts("ADDKF a new point was dropped"); return 11; }
    if (res.exclude_set.size() != (size_t)(step + 2) || res.do_loop_detection) { std::puts("ADDKF exclude_set"); return 12; }
    strength = res.neighborid_to_strength[0].second;
    if (step == 0 && strength != N) { std::printf("ADDKF first strength %d\n", strength); return 13; }
    if (step == 1 && res.neighborid_to_strength[1].second != strength) { std::puts("ADDKF the two strengths differ"); return 14; }
  }
  // the pose chain: pure translations add up
  double T[12];
  std::vector<double> poses(12);
  if (svs_map_get_poses(map.get(), 1, std::vector<int32_t>(1, 22).data(), poses.data()) != SVS_OK) return 15;
  std::memcpy(T, poses.data(), sizeof T);
  if (std::fabs(T[3] - 0.02) > 1e-15 || std::fabs(T[7] + 0.04) > 1e-15 || std::fabs(T[11] + 0.6) > 1e-15 || T[0] != 1.0) { std::printf("ADDKF pose %.17g %.17g %.17g\n", T[3], T[7], T[11]); return 16; }
  int32_t n_kf = 0, n_pt = 0, n_obs = 0, n_edges = 0, n_marg = 0;
  if (svs_map_info(map.get(), &n_kf, &n_pt, &n_obs) != SVS_OK || svs_map_edge_info(map.get(), &n_edges, &n_marg) != SVS_OK) return 17;
  if (n_obs != 5 * N || n_edges != 3 || n_marg != 3 || map.anchorLevel(301) != 1) { std::printf("ADDKF counts: %d pairs, %d edges, %d marginalised\n", n_obs, n_edges, n_marg); return 18; }
  svs_free(ctx.get(), d_any);
  std::printf("ADDKF ok %d %zu %d %d\n", n_kf, res.new_neighbors.size(), n_pt, strength);
  return 0;
}
