// Drives BackendRegistration::localRegisterFrame(map, root) / globalLoopClosure(map, ..) and BackendMap::registerKeyframes of the C++ adaptor
// (include/scavislam_hip.hpp) on the GPU and checks them against svs_reg_register_map_batch + svs_reg_commit called directly on a twin map;
// tests/test_gpu_regcommit.py compiles and runs it.  Prints "REGCOMMIT ok <track points> <pairs added> <edges> <loop strength>".
// The scene of register_map_smoke.cpp: one noise frame that is the root (id 10) AND, at the same pose, the keyframe its points are anchored in (id 11);
// keyframe 12 observes every second point and anchors none.  An edge (10, 12) makes 12 a direct neighbour of the root, so the walk from 10 reaches 12 and,
// with an edge (12, 11), the keyframe 11, which is the one that qualifies.  Keyframe 13, the same frame again and without an edge, is the loop keyframe.
#include <cstdio>
#include <cstring>
#include <vector>

#include "scavislam_hip.hpp"

using namespace scavislam_hip;

static bool same_edges(const Context &ctx, BackendMap &a, BackendMap &b, const std::vector<int32_t> &pairs) {
  const int n = (int)pairs.size() / 2;
  std::vector<svs_map_edge> ea((size_t)n), eb((size_t)n);
  if (!ctx.check(svs_map_get_edges(a.get(), n, pairs.data(), ea.data())) || !ctx.check(svs_map_get_edges(b.get(), n, pairs.data(), eb.data()))) return false;
  return std::memcmp(ea.data(), eb.data(), sizeof(svs_map_edge) * (size_t)n) == 0;
}

static bool same_table(const Context &ctx, BackendMap &a, BackendMap &b, int kf) {
  int32_t na = 0, nb = 0;
  std::vector<int32_t> ia(1024), ib(1024);
  std::vector<svs_ba_edge> ra(1024), rb(1024);
  if (!ctx.check(svs_map_get_feature_table(a.get(), kf, 1024, &na, ia.data(), ra.data())) || !ctx.check(svs_map_get_feature_table(b.get(), kf, 1024, &nb, ib.data(), rb.data())))
    return false;
  return na == nb && ia == ib && std::memcmp(ra.data(), rb.data(), sizeof(svs_ba_edge) * 1024) == 0;
}

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
  int32_t lw[3], lh[3];
  svs_fastgrid grids[3];
  for (int l = 0; l < 3; ++l) {
    lw[l] = fr.w(l); lh[l] = fr.h(l);
    const int dim = l < 2 ? 3 : 2, per_cell = (2000 >> (2 * l)) / (dim * dim), bound = per_cell / 3 > 10 ? per_cell / 3 : 10;
    grids[l] = makeFastGrid(lw[l], lh[l], per_cell, bound, 25, dim, dim);
  }
  FastGrid fast(ctx, 3, lw, lh, grids);
  std::vector<Corner> corners[3];
  if (!fast.detectAdaptively(fr, 5, corners)) return 5;
  std::vector<svs_candidate_point> pts;
  const size_t step = corners[0].size() / 300 + 1;
  for (size_t i = 0; i < corners[0].size(); i += step) {
    const int x = corners[0][i].x, y = corners[0][i].y;
    if (x < 8 || y < 8 || x >= w - 8 || y >= h - 8) continue;
    svs_candidate_point p;
    std::memset(&p, 0, sizeof p);
    const double d = 6.0, z = cam.f * cam.b / d;
    p.xyz_anchor[0] = (x - cam.cx) / cam.f * z; p.xyz_anchor[1] = (y - cam.cy) / cam.f * z; p.xyz_anchor[2] = z;
    p.anchor_obs_pyr[0] = x; p.anchor_obs_pyr[1] = y; p.anchor_obs_pyr[2] = x - d;
    p.anchor_level = 0; p.kf_index = 11; p.point_id = 7000 + (int)pts.size();
    pts.push_back(p);
  }
  if (pts.size() < 40) { std::printf("REGCOMMIT few corners %zu\n", pts.size()); return 6; }
  const double I[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};
  RegistrationKeyframe k;
  std::memset(&k, 0, sizeof k);
  std::memcpy(k.kf.T_anchor_from_w, I, sizeof I);
  for (int l = 0; l < 3; ++l) { k.kf.pyr[l] = fr.pyr(l); k.kf.stride[l] = fr.stride(l); }
  std::vector<RegistrationKeyframe> kfs(4, k);
  for (int i = 0; i < 4; ++i) { kfs[i].frame_id = 10 + i; kfs[i].in_double_window = true; kfs[i].direct_neighbor = i == 0; }
  RegistrationFrame root;
  root.table_entry = 0; root.d_disp = fr.disp(); root.disp_stride = fr.stride(0);
  for (int l = 0; l < 3; ++l) root.cell_grid2d[l] = fast.cell_grid2d(l);
  std::memcpy(root.T_from_world, I, sizeof I);
  std::vector<RegistrationFrame> frames(4, root);
  std::vector<int32_t> op, okf, window, level;
  std::vector<double> center;
  for (size_t i = 0; i < pts.size(); ++i) {
    op.push_back(pts[i].point_id); okf.push_back(11);
    if (i % 2) { op.push_back(pts[i].point_id); okf.push_back(12); }
    if (i % 3 == 0) { op.push_back(pts[i].point_id); okf.push_back(10); }      // pairs the root already has: they keep what they have
  }
  for (size_t i = 0; i < op.size(); ++i) { center.push_back(1.0 + (double)i); center.push_back(2.0); center.push_back(0.5); level.push_back((int32_t)(i % 3)); }
  for (int i = 0; i < 4; ++i) window.push_back(10 + i);
  const int32_t epairs[4] = {10, 12, 12, 11};
  const std::vector<int32_t> ep(epairs, epairs + 4), es(2, 20), et(2, 0);
  BackendMap a(ctx, 16, 8192, 4096), b(ctx, 16, 8192, 4096), c(ctx, 16, 8192, 4096);
  BackendMap *maps[3] = {&a, &b, &c};
  for (int m = 0; m < 3; ++m) {
    BackendMap &M = *maps[m];
    if (!M.ok() || !M.reserveEdges(16) || !M.addKeyframes(kfs, frames) || !M.addPoints(pts) || !M.addObservations(op, okf, center, level) || !M.setWindow(window) ||
        !M.addEdges(ep, es, et)) { std::puts("REGCOMMIT update refused"); return 7; }
  }
  // a: the adaptor, to the end of localRegisterFrame
  BackendRegistration reg(ctx, cam, 512, 8, 2048);
  if (!reg.ok()) return 8;
  BackendMap::CommitResult got;
  if (!reg.localRegisterFrame(a, 10, &got)) { std::printf("REGCOMMIT localRegisterFrame: status %d, %s\n", reg.lastResult().status, ctx.error()); return 9; }
  // b: the C calls
  const int32_t walk[3] = {10, 12, 11}, direct[2] = {10, 12};
  svs_reg_map_request q;
  std::memset(&q, 0, sizeof q);
  q.mode = SVS_REG_LOCAL; q.root_kf = 10; q.n_walk = 3; q.h_walk_kf = walk; q.n_direct = 2; q.h_direct_kf = direct;
  std::memcpy(q.T_root_from_world, I, sizeof I);
  svs_reg *creg = nullptr;
  if (!ctx.check(svs_reg_create(ctx.get(), &cam, 1, 512, 8, 2048, &creg))) return 10;
  svs_reg_result res;
  svs_reg_commit_result cres;
  std::vector<svs_map_constraint_result> cons(8);
  std::vector<int32_t> miss(8 * 64), ekf(8), est(8), tid(512), tadd(512);
  bool okc = ctx.check(svs_reg_register_map_batch(creg, b.get(), 1, &q, nullptr, &res, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr)) &&
             ctx.check(svs_reg_commit(creg, b.get(), 0, 0, nullptr, nullptr, 64, &cres, ekf.data(), est.data(), cons.data(), miss.data(), 512, tid.data(), tadd.data()));
  if (!okc) { std::printf("REGCOMMIT C calls: %s\n", ctx.error()); svs_reg_destroy(creg); return 11; }
  if (std::memcmp(&res, &reg.lastResult(), sizeof res) != 0) { std::puts("REGCOMMIT registration differs"); return 12; }
  if (std::memcmp(&cres, &got.result, sizeof cres) != 0 || !cres.committed || cres.n_edges != 1 || ekf[0] != 11 || got.new_neighbors != std::vector<int32_t>(1, 11)) {
    std::printf("REGCOMMIT commit result differs: committed %d edges %d\n", cres.committed, cres.n_edges); return 13;
  }
  if (std::memcmp(cons.data(), got.constraints.data(), sizeof(svs_map_constraint_result)) != 0 || cons[0].status != SVS_CONS_OK) { std::puts("REGCOMMIT constraint differs"); return 14; }
  const int32_t e1[2] = {11, 10};
  const std::vector<int32_t> new_edge(e1, e1 + 2);
  if (!same_edges(ctx, a, b, new_edge) || !same_table(ctx, a, b, 10)) { std::puts("REGCOMMIT maps differ"); return 15; }
  if (cres.n_pairs_added <= 0 || cres.n_pairs_added >= cres.n_track) { std::printf("REGCOMMIT pairs %d of %d\n", cres.n_pairs_added, cres.n_track); return 16; }
  // c: BackendMap::registerKeyframes with the lists of the C call
  std::vector<svs_map_track_point> tl((size_t)cres.n_track);
  {
    std::vector<int32_t> ids(1024);
    std::vector<svs_ba_edge> rec(1024);
    int32_t n = 0;
    if (!ctx.check(svs_map_get_feature_table(b.get(), 10, 1024, &n, ids.data(), rec.data()))) return 17;
    for (int i = 0; i < cres.n_track; ++i) {
      int at = -1;
      for (int j = 0; j < n; ++j) if (ids[(size_t)j] == tid[(size_t)i]) at = j;
      if (at < 0) return 18;
      std::memcpy(tl[(size_t)i].center, rec[(size_t)at].obs, sizeof tl[(size_t)i].center);      // (a pair that was present: refused by the pair rule on c as well)
      tl[(size_t)i].global_id = tid[(size_t)i]; tl[(size_t)i].level = 0;
    }
  }
  BackendMap::CommitResult exp;
  std::vector<std::pair<int, int> > n2s(1, std::make_pair(11, (int)est[0]));
  n2s.push_back(std::make_pair(12, 3));                                                         // below covis_thr: no edge
  if (!c.registerKeyframes(10, cres.T_new, n2s, tl, 15, &exp)) { std::printf("REGCOMMIT registerKeyframes: %s\n", ctx.error()); return 19; }
  if (exp.result.n_edges != 1 || exp.result.n_pairs_added != cres.n_pairs_added || !same_edges(ctx, b, c, new_edge) || !same_table(ctx, b, c, 10)) {
    std::puts("REGCOMMIT explicit call differs"); return 20;
  }
  // the loop closure: query 11, loop keyframe 13 where it stands
  BackendMap::CommitResult lgot;
  if (!reg.globalLoopClosure(a, 11, 13, I, &lgot)) { std::printf("REGCOMMIT globalLoopClosure: status %d, %s\n", reg.lastResult().status, ctx.error()); return 21; }
  std::memset(&q, 0, sizeof q);
  const int32_t query[1] = {11};
  q.mode = SVS_REG_LOOP; q.root_kf = 13; q.n_walk = 1; q.h_walk_kf = query;
  std::memcpy(q.T_root_from_world, I, sizeof I);
  okc = ctx.check(svs_reg_register_map_batch(creg, b.get(), 1, &q, nullptr, &res, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr)) &&
        ctx.check(svs_reg_commit(creg, b.get(), 0, 0, nullptr, nullptr, 64, &cres, ekf.data(), est.data(), cons.data(), miss.data(), 512, tid.data(), tadd.data()));
  svs_reg_destroy(creg);
  if (!okc) { std::printf("REGCOMMIT C loop calls: %s\n", ctx.error()); return 22; }
  const int32_t e2[2] = {11, 13};
  const std::vector<int32_t> loop_edge(e2, e2 + 2);
  if (std::memcmp(&cres, &lgot.result, sizeof cres) != 0 || cres.other_id != 11 || cres.root_id != 13 || est[0] != cres.n_track || !same_edges(ctx, a, b, loop_edge) ||
      !same_table(ctx, a, b, 13)) { std::puts("REGCOMMIT loop closure differs"); return 23; }
  std::printf("REGCOMMIT ok %d %d %d %d\n", got.result.n_track, got.result.n_pairs_added, got.result.n_edges, est[0]);
  return 0;
}
