// Drives the C++ adaptor's pose-graph edges and constraints (include/scavislam_hip.hpp) on the GPU: BackendMap::reserveEdges / addEdges / computeConstraints /
// updateMarginalization and the SlamGraphBA::copyDataFromMap overload without constraints; tests/test_gpu_constraints.py compiles and runs it.  Prints
// "CONSTRAINTS ok <strength> <constraints>".  The scene is the one of ba_map_smoke.cpp: five keyframes on a line (ids 20 .. 24, T_me_from_world = [I | t]), 90
// points anchored in 20, 21 or 22 and seen from their anchor onwards.  With pure translations the depth of a point is || xyz + t_1 - t_anchor ||, which the host
// forms here to compare the median and Lambda (to 1e-12: byte equality is the Python tests' business).
#include <algorithm>
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
  std::vector<double> t((size_t)3 * K);
  for (int i = 0; i < K; ++i) {
    std::memset(&kfs[i].kf, 0, sizeof kfs[i].kf);
    t[3 * i] = 0.004 * (i % 2); t[3 * i + 1] = -0.003 * (i % 3); t[3 * i + 2] = -0.3 * i + 0.005 * i;
    const double T[12] = {1, 0, 0, t[3 * i], 0, 1, 0, t[3 * i + 1], 0, 0, 1, t[3 * i + 2]};
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
    const int a = p % 3;
    const double z = 3.0 + 9.0 * uni(), u = 30 + 260 * uni(), v = 30 + 180 * uni();
    std::memset(&pts[p], 0, sizeof pts[p]);
    pts[p].xyz_anchor[0] = (u - cam.cx) / cam.f * z; pts[p].xyz_anchor[1] = (v - cam.cy) / cam.f * z; pts[p].xyz_anchor[2] = z;
    pts[p].kf_index = first_id + a; pts[p].point_id = 300 + 5 * p;
    const int last = a == 0 ? (p % 2 ? 3 : 2) : 4;
    for (int i = a; i <= last; ++i) {
      op.push_back(pts[p].point_id); okf.push_back(first_id + i); lvl.push_back(0);
      const double y[3] = {pts[p].xyz_anchor[0], pts[p].xyz_anchor[1], z + 0.3 * (a - i)};
      ctr.push_back(cam.f * y[0] / y[2] + cam.cx); ctr.push_back(cam.f * y[1] / y[2] + cam.cy); ctr.push_back(cam.f * (y[0] - cam.b) / y[2] + cam.cx);
    }
  }
  BackendMap map(ctx, 64, 1024, 4096);
  if (!map.ok() || !map.addKeyframes(kfs, frames) || !map.addPoints(pts) || !map.addObservations(op, okf, ctr, lvl)) { std::puts("CONSTRAINTS update refused"); return 5; }
  std::vector<int32_t> pairs, strength(3, 30), type(3, 0);
  const int32_t pr[6] = {22, 21, 22, 23, 24, 23};
  pairs.assign(pr, pr + 6);
  if (map.addEdges(pairs, strength, type)) { std::puts("CONSTRAINTS edges accepted without reserveEdges"); return 6; }
  if (!map.reserveEdges(8) || !map.addEdges(pairs, strength, type)) { std::puts("CONSTRAINTS addEdges refused"); return 7; }
  if (map.addEdges(pairs, strength, type)) { std::puts("CONSTRAINTS an edge twice accepted"); return 8; }
  int32_t n_edges = 0, n_marg = 0;
  if (svs_map_edge_info(map.get(), &n_edges, &n_marg) != SVS_OK || n_edges != 3 || n_marg != 0) { std::puts("CONSTRAINTS edge counts"); return 9; }

  // the window moves on: 21 and 22 were INNER with 23; now 22 is OUTER and 21 is entered by the prepare.  The pairs that leave the inner window: (21, 22), (22, 23)
  std::vector<int32_t> old_ids, old_types, window, types, wpairs;
  for (int id = 21; id <= 23; ++id) { old_ids.push_back(id); old_types.push_back(0); }
  window.push_back(22); window.push_back(23); window.push_back(24);
  types.push_back(1); types.push_back(0); types.push_back(0);
  const int32_t wp[6] = {23, 22, 24, 23, 21, 23};
  wpairs.assign(wp, wp + 6);
  int n_active = 0;
  if (!map.prepareForOptimization(&window, &types, wpairs, &n_active) || window.size() != 4 || window[3] != 21) { std::puts("CONSTRAINTS prepare failed"); return 10; }
  std::vector<svs_map_constraint_result> res;
  std::vector<int32_t> missing, no_ids;
  std::vector<double> no_T;
  if (!map.updateMarginalization(old_ids, old_types, window, types, no_ids, no_T, &res, &missing)) { std::puts("CONSTRAINTS updateMarginalization failed"); return 11; }
  // keyframe 20 anchors a third of the points and is outside the window: the first call names it
  if (res.size() != 2 || res[0].status != SVS_CONS_MISSING_ANCHOR || res[1].status != SVS_CONS_MISSING_ANCHOR || missing.size() != 1 || missing[0] != 20) {
    std::printf("CONSTRAINTS first call: %zu results, %zu missing\n", res.size(), missing.size());
    return 12;
  }
  std::vector<int32_t> cached_ids(1, 20);
  std::vector<double> cached_T(kfs[0].kf.T_anchor_from_w, kfs[0].kf.T_anchor_from_w + 12);
  if (!map.updateMarginalization(old_ids, old_types, window, types, cached_ids, cached_T, &res, &missing) || !missing.empty() || res.size() != 2) { std::puts("CONSTRAINTS second call failed"); return 13; }
  if (svs_map_edge_info(map.get(), &n_edges, &n_marg) != SVS_OK || n_marg != 2) { std::puts("CONSTRAINTS marginalised count"); return 14; }
  // request 1 is (22, 23): the points seen by both, their depth in 22
  std::vector<double> depth;
  for (int p = 0; p < N; ++p) {
    const int a = p % 3, last = a == 0 ? (p % 2 ? 3 : 2) : 4;
    if (last < 3) continue;
    double x[3];
    for (int k = 0; k < 3; ++k) x[k] = pts[p].xyz_anchor[k] + t[3 * 2 + k] - t[3 * a + k];
    depth.push_back(std::sqrt(x[0] * x[0] + x[1] * x[1] + x[2] * x[2]));
  }
  std::sort(depth.begin(), depth.end());
  const size_t n = depth.size();
  const double med = n % 2 ? depth[n / 2] : 0.5 * (depth[n / 2 - 1] + depth[n / 2]);
  double dt2 = 0;
  for (int k = 0; k < 3; ++k) dt2 += (t[6 + k] - t[9 + k]) * (t[6 + k] - t[9 + k]);
  const double nd = std::sqrt(dt2) / med, a_ = (double)n * (350 * nd) * (350 * nd), b_ = (double)n * 1e4;
  const svs_map_constraint_result &r = res[1];
  if (r.status != SVS_CONS_OK || r.strength != (int)n || std::fabs(r.median - med) > 1e-12 * med || std::fabs(r.norm_dist - nd) > 1e-12 * nd ||
      std::fabs(r.info[0] - a_) > 1e-11 * a_ || std::fabs(r.info[35] - b_) > 1e-11 * b_ || r.info[1] != 0.0 || std::fabs(r.T_12[11] - (t[8] - t[11])) > 1e-15) {
    std::printf("CONSTRAINTS (22, 23): status %d strength %d (%zu) median %.17g (%.17g) norm_dist %.17g (%.17g)\n", r.status, r.strength, n, r.median, med, r.norm_dist, nd);
    return 15;
  }
  // the optimizer takes its constraints from the table: (22, 23) and (21, 22) have an OUTER end, each in both directions
  const OptParams opt = {2, true, 3.0};
  SlamGraphBA ba(ctx);
  if (!ba.copyDataFromMap(map, opt, cam)) { std::puts("CONSTRAINTS copyDataFromMap failed"); return 16; }
  int32_t C = 0;
  if (!ctx.check(svs_ba_window_constraints(ba.get(), &C, nullptr)) || C != 4) { std::printf("CONSTRAINTS %d constraints in the window\n", C); return 17; }
  std::vector<svs_ba_constraint> cons((size_t)C);
  if (!ctx.check(svs_ba_window_constraints(ba.get(), &C, cons.data()))) return 18;
  // window order 22, 23, 24, 21: the first record is i = 0 (22), j = 1 (23), T_21 = T_23_from_22
  if (cons[0].pose1 != 0 || cons[0].pose2 != 1 || std::fabs(cons[0].T_21[11] - (t[11] - t[8])) > 1e-15 || cons[0].info[0] != r.info[0]) { std::puts("CONSTRAINTS first record"); return 19; }
  svs_ba_stats st;
  if (!ba.optimize(&st) || !ba.restoreDataToMap(map)) { std::puts("CONSTRAINTS optimize / restore failed"); return 20; }
  // an edge with an OUTER end that is not marginalised any more: refused
  const int32_t un[2] = {23, 22};
  if (!ctx.check(svs_map_unmarginalize(map.get(), 1, un)) || ba.copyDataFromMap(map, opt, cam)) { std::puts("CONSTRAINTS an unmarginalised OUTER edge accepted"); return 21; }
  svs_free(ctx.get(), d_any);
  std::printf("CONSTRAINTS ok %d %d\n", r.strength, C);
  return 0;
}
