// Drives the C++ adaptor's path from the device-resident map to the optimizer (include/scavislam_hip.hpp) on the GPU: BackendMap::addObservations with centres and
// levels, BackendMap::prepareForOptimization, SlamGraphBA::copyDataFromMap / optimize / restoreDataToMap -- and checks them against SlamGraphBA::optimizeWindow,
// the adaptor's host-marshalled call, on the same tables; tests/test_gpu_ba_map.py compiles and runs it.  Prints "BA_MAP ok <window> <active> <accepted>".
// The scene: five keyframes on a line (ids 20 .. 24), 22 OUTER, 23 and 24 INNER, 20 and 21 outside W0; 90 points anchored in 20, 21 or 22 and seen from their
// anchor onwards; edge_table_ pairs (23, 22), (24, 23) and (23, 21): keyframe 21 enters the window, keyframe 20 does not.
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
  void *d_any = nullptr;      // the walks never read a pyramid or a disparity
  if (!ctx.check(svs_malloc(ctx.get(), 4096, &d_any))) return 4;
  const int K = 5, first_id = 20, N = 90;
  unsigned s = 2024u;
  auto uni = [&s]() { s = s * 1664525u + 1013904223u; return (double)(s >> 8) / (double)(1u << 24); };
  std::vector<RegistrationKeyframe> kfs((size_t)K);
  std::vector<RegistrationFrame> frames((size_t)K);
  std::vector<double> cz((size_t)K);
  for (int i = 0; i < K; ++i) {
    std::memset(&kfs[i].kf, 0, sizeof kfs[i].kf);
    cz[i] = 0.3 * i;      // T_me_from_world = [I | -c], slightly off the truth
    const double T[12] = {1, 0, 0, 0.004 * (i % 2), 0, 1, 0, -0.003 * (i % 3), 0, 0, 1, -cz[i] + 0.005 * i};
    std::memcpy(kfs[i].kf.T_anchor_from_w, T, sizeof T);
    for (int l = 0; l < 3; ++l) { kfs[i].kf.pyr[l] = static_cast<const uint8_t *>(d_any); kfs[i].kf.stride[l] = 64; }
    kfs[i].frame_id = first_id + i; kfs[i].in_double_window = false; kfs[i].direct_neighbor = false;
    frames[i].table_entry = 0; frames[i].d_disp = static_cast<const float *>(d_any); frames[i].disp_stride = 64;
    std::memset(frames[i].T_from_world, 0, sizeof frames[i].T_from_world);
  }
  std::vector<svs_candidate_point> pts((size_t)N);
  std::vector<int32_t> op, okf, lvl;
  std::vector<double> ctr;
  for (int p = 0; p < N; ++p) {
    const int a = p % 3;      // the anchor: keyframe 20, 21 or 22
    const double z = 3.0 + 9.0 * uni(), u = 30 + 260 * uni(), v = 30 + 180 * uni();
    const double xa[3] = {(u - cam.cx) / cam.f * z, (v - cam.cy) / cam.f * z, z};
    std::memset(&pts[p], 0, sizeof pts[p]);
    pts[p].xyz_anchor[0] = xa[0]; pts[p].xyz_anchor[1] = xa[1]; pts[p].xyz_anchor[2] = z * (1.0 + 0.02 * (uni() - 0.5));
    pts[p].kf_index = first_id + a; pts[p].point_id = 300 + 5 * p;
    const int last = a == 0 ? (p % 2 ? 3 : 2) : 4;      // points of keyframe 20: seen up to keyframe 22 or 23, never from 24
    for (int i = a; i <= last; ++i) {
      const double y[3] = {xa[0], xa[1], xa[2] + cz[a] - cz[i]};
      op.push_back(pts[p].point_id); okf.push_back(first_id + i); lvl.push_back(p % 3 == 1 && i == last ? 1 : 0);
      ctr.push_back(cam.f * y[0] / y[2] + cam.cx + 0.4 * (uni() - 0.5)); ctr.push_back(cam.f * y[1] / y[2] + cam.cy + 0.4 * (uni() - 0.5));
      ctr.push_back(cam.f * (y[0] - cam.b) / y[2] + cam.cx + 0.4 * (uni() - 0.5));
    }
  }
  BackendMap map(ctx, 64, 1024, 4096);
  if (!map.ok() || !map.addKeyframes(kfs, frames) || !map.addPoints(pts) || !map.addObservations(op, okf, ctr, lvl)) { std::puts("BA_MAP update refused"); return 5; }
  if (!map.addObservations(op, okf, ctr, lvl)) { std::puts("BA_MAP repeated pairs refused"); return 6; }      // ignored, as feature_table.insert
  int32_t n_meas = 0, n_unmeas = 0;
  if (svs_map_measured_info(map.get(), &n_meas, &n_unmeas) != SVS_OK || n_meas != (int)op.size() || n_unmeas != 0) { std::puts("BA_MAP measured counts"); return 7; }

  std::vector<int32_t> window, types, pairs;
  window.push_back(22); window.push_back(23); window.push_back(24);
  types.push_back(1); types.push_back(0); types.push_back(0);
  const int32_t pr[6] = {23, 22, 24, 23, 21, 23};
  pairs.assign(pr, pr + 6);
  int n_active = 0;
  if (!map.prepareForOptimization(&window, &types, pairs, &n_active)) { std::puts("BA_MAP prepare failed"); return 8; }
  // keyframe 21 enters through (23, 21); the points of keyframe 20 are seen from 23 at most, which has no pair to 20: not active
  if (window.size() != 4 || window[3] != 21 || types[3] != 1 || n_active != 60) { std::printf("BA_MAP window %zu active %d\n", window.size(), n_active); return 9; }

  // constraints along 21 - 22 - 23, both directions as copyContraintsToG2o hands them over
  std::vector<SlamGraphBA::ConstraintById> cons;
  for (int i = 1; i <= 2; ++i)
    for (int dir = 0; dir < 2; ++dir) {
      SlamGraphBA::ConstraintById c;
      std::memset(&c, 0, sizeof c);
      c.pose_id_1 = first_id + (dir ? i + 1 : i); c.pose_id_2 = first_id + (dir ? i : i + 1);
      const double dz = (dir ? 1.0 : -1.0) * (cz[i + 1] - cz[i]);
      const double T[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, dz};
      std::memcpy(c.T_2_from_1, T, sizeof T);
      for (int k = 0; k < 6; ++k) c.Lambda_2_from_1[7 * k] = k < 3 ? 3.0e4 : 3.0e5;
      cons.push_back(c);
    }
  const OptParams opt = {2, true, 3.0};

  // the yardstick: the adaptor's host-marshalled call on the same tables
  std::vector<int> pose_ids(window.begin(), window.end()), point_ids, anchor_ids;
  std::vector<double> poses, xyz;
  for (size_t i = 0; i < window.size(); ++i) poses.insert(poses.end(), kfs[window[i] - first_id].kf.T_anchor_from_w, kfs[window[i] - first_id].kf.T_anchor_from_w + 12);
  for (int p = 0; p < N; ++p)
    if (p % 3 != 0) { point_ids.push_back(pts[p].point_id); anchor_ids.push_back(pts[p].kf_index); xyz.insert(xyz.end(), pts[p].xyz_anchor, pts[p].xyz_anchor + 3); }
  std::vector<SlamGraphBA::ObsById> obs(op.size());
  for (size_t k = 0; k < op.size(); ++k) { obs[k].point_id = op[k]; obs[k].pose_id = okf[k]; obs[k].level = lvl[k]; std::memcpy(obs[k].center, &ctr[3 * k], sizeof obs[k].center); }
  const std::vector<double> poses0(poses);
  SlamGraphBA host(ctx);
  svs_ba_stats st_host;
  if (!host.optimizeWindow(opt, cam, pose_ids, &poses, point_ids, anchor_ids, &xyz, obs, cons, &st_host)) { std::puts("BA_MAP optimizeWindow failed"); return 10; }

  SlamGraphBA ba(ctx);
  svs_ba_stats st;
  if (!ba.copyDataFromMap(map, opt, cam, cons)) { std::puts("BA_MAP copyDataFromMap failed"); return 11; }
  int32_t n_edges = 0;
  if (!ctx.check(svs_ba_window_edges(ba.get(), &n_edges, nullptr))) return 12;
  if (!ba.optimize(&st) || !ba.restoreDataToMap(map)) { std::puts("BA_MAP optimize / restore failed"); return 13; }
  std::vector<double> got((size_t)12 * window.size()), psi((size_t)3 * n_active);
  if (!ctx.check(svs_ba_get_state(ba.get(), got.data(), psi.data()))) return 14;
  if (st.trials != st_host.trials || st.accepted != st_host.accepted || st.accepted < 1) { std::printf("BA_MAP LM record %d/%d vs %d/%d\n", st.trials, st.accepted, st_host.trials, st_host.accepted); return 15; }
  double upd = 0, err = 0;
  for (size_t i = 0; i < got.size(); ++i) { upd = std::fmax(upd, std::fabs(poses[i] - poses0[i])); err = std::fmax(err, std::fabs(got[i] - poses[i])); }
  if (!(upd > 1e-5) || !(err <= 1e-6 * upd)) { std::printf("BA_MAP poses differ from optimizeWindow: %g of an update of %g\n", err, upd); return 16; }
  // the map holds the optimised state: the next window starts from it, pose bytes included
  if (ba.restoreDataToMap(map) == false) { std::puts("BA_MAP second restore refused"); return 17; }      // (still this window: allowed, and idempotent)
  if (!map.prepareForOptimization(&window, &types, pairs, &n_active) || window.size() != 4 || n_active != 60) { std::puts("BA_MAP second prepare failed"); return 18; }
  if (!ba.copyDataFromMap(map, opt, cam, cons)) { std::puts("BA_MAP second copyDataFromMap failed"); return 19; }
  std::vector<double> again(got.size());
  if (!ctx.check(svs_ba_get_state(ba.get(), again.data(), nullptr))) return 20;
  if (std::memcmp(again.data(), got.data(), sizeof(double) * got.size()) != 0) { std::puts("BA_MAP the map does not hold the optimised poses"); return 21; }
  svs_free(ctx.get(), d_any);
  std::printf("BA_MAP ok %zu %d %d edges %d\n", window.size(), n_active, st.accepted, n_edges);
  return 0;
}
