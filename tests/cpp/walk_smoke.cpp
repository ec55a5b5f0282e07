// Drives the C++ adaptor's pose-graph walks (include/scavislam_hip.hpp) on the GPU: BackendMap::computeInitialDoubleWin / framesInNeighborhood / computeAbsolutePose
// and prepareForOptimization(root_id, loop_id), which chains the window from the root, reinitializePoses and updateMarginalization and answers the missing anchors
// itself; tests/test_gpu_walk.py compiles and runs it.  Prints "WALK ok <window> <marginalised> <strength>".  The scene is the one of constraints_smoke.cpp: five
// keyframes on a line (ids 20 .. 24, T_me_from_world = [I | t]) joined 20 - 21 - 22 - 23 - 24, 90 points anchored in 20, 21 or 22 and seen from their anchor
// onwards.  With pure translations a chained pose equals the stored one to rounding, and the depth of a point is || xyz + t_1 - t_anchor ||.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "scavislam_hip.hpp"

using namespace scavislam_hip;

static bool is(const std::vector<int32_t> &v, int a, int b, int c) { return v.size() == 3 && v[0] == a && v[1] == b && v[2] == c; }

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
  if (!map.ok() || !map.addKeyframes(kfs, frames) || !map.addPoints(pts) || !map.addObservations(op, okf, ctr, lvl)) { std::puts("WALK update refused"); return 5; }
  // slots 0 .. 3, equal strengths: a row is walked from its latest slot to its earliest
  std::vector<int32_t> pairs, strength(4, 30), type(4, 0);
  const int32_t pr[8] = {22, 21, 22, 23, 24, 23, 20, 21};
  pairs.assign(pr, pr + 8);
  if (!map.reserveEdges(8) || !map.addEdges(pairs, strength, type)) { std::puts("WALK addEdges refused"); return 6; }

  std::vector<int32_t> window, types, ids;
  if (!map.computeInitialDoubleWin(20, 1, 5, &window, &types) || window.size() != 5 || types[0] != 0 || types[1] != 1) { std::puts("WALK computeInitialDoubleWin failed"); return 7; }
  for (int i = 0; i < K; ++i) if (window[(size_t)i] != first_id + i) { std::puts("WALK the chain's order"); return 8; }
  // the first window: 22 and 23 INNER (22's row: slot 1 to 23 before slot 0 to 21), 21 OUTER; no old window: both others are reinitialised from their parent
  map.setWindowSizes(2, 3);
  int n_active = 0;
  std::vector<svs_map_constraint_result> res;
  std::vector<int32_t> missing;
  if (!map.prepareForOptimization(22, -1, &window, &types, &n_active, &res, &missing) || !is(window, 22, 23, 21) || !is(types, 0, 0, 1) || n_active < 1 || !res.empty()) {
    std::puts("WALK first prepareForOptimization failed"); return 9;
  }
  if (!map.framesInNeighborhood(22, 40, &ids) || !is(ids, 22, 23, 21)) { std::puts("WALK framesInNeighborhood failed"); return 10; }
  if (!map.framesInNeighborhood(24, 40, &ids) || !ids.empty()) { std::puts("WALK a root outside the window has a neighbourhood"); return 11; }
  // 20 lies outside the window: its path is 20 - 21, its pose the stored one to rounding; 24 goes through 23
  double T[12];
  if (!map.computeAbsolutePose(20, T) || std::fabs(T[11] - t[2]) > 1e-12 || std::fabs(T[7] - t[1]) > 1e-12 || T[0] != 1.0) { std::puts("WALK computeAbsolutePose(20) failed"); return 12; }
  if (!map.computeAbsolutePose(24, T) || std::fabs(T[11] - t[14]) > 1e-12) { std::puts("WALK computeAbsolutePose(24) failed"); return 13; }
  // the window moves on to 24: 24 and 23 INNER, 22 OUTER.  (22, 23) leaves the inner window: its constraint needs the anchors 20 and 21, both outside the window
  // now, which prepareForOptimization finds through computeAbsolutePoses (21 - 22, and 20 - 21 - 22)
  if (!map.prepareForOptimization(24, -1, &window, &types, &n_active, &res, &missing) || !is(window, 24, 23, 22) || !is(types, 0, 0, 1)) {
    std::puts("WALK second prepareForOptimization failed"); return 14;
  }
  int32_t n_edges = 0, n_marg = 0;
  if (svs_map_edge_info(map.get(), &n_edges, &n_marg) != SVS_OK || n_edges != 4 || n_marg != 1 || !missing.empty() || res.size() != 1) {
    std::printf("WALK second call: %d marginalised, %zu missing, %zu results\n", n_marg, missing.size(), res.size()); return 15;
  }
  // (22, 23): the points seen by both, their depth in 22
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
  const svs_map_constraint_result &r = res[0];
  if (r.status != SVS_CONS_OK || r.strength != (int)n || std::fabs(r.median - med) > 1e-9 * med) {
    std::printf("WALK (22, 23): status %d strength %d (%zu) median %.17g (%.17g)\n", r.status, r.strength, n, r.median, med); return 16;
  }
  // the optimizer takes the prepared window and the table's constraints
  const OptParams opt = {2, true, 3.0};
  SlamGraphBA ba(ctx);
  if (!ba.copyDataFromMap(map, opt, cam)) { std::puts("WALK copyDataFromMap failed"); return 17; }
  svs_free(ctx.get(), d_any);
  std::printf("WALK ok %zu %d %d\n", window.size(), n_marg, r.strength);
  return 0;
}
