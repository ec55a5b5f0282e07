// Drives BackendMap and BackendRegistration::registerFrames of the C++ adaptor (include/scavislam_hip.hpp) on the GPU and checks that they hand back what
// svs_reg_register_map_batch called directly reports, and what the stateless adaptor call reports on the same scene; tests/test_gpu_register_map.py compiles
// and runs it.  Prints "REGISTER_MAP ok <strength> <loop track points>".
// The scene of register_smoke.cpp: one noise frame that is the root (id 10) AND, at the same pose, the keyframe its points are anchored in (id 11); keyframe 12
// observes every second point and anchors none.
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
  std::vector<svs_candidate_point> pts;      // kf_index: the anchor's table entry (1), as the stateless call takes it
  const size_t step = corners[0].size() / 300 + 1;
  for (size_t i = 0; i < corners[0].size(); i += step) {
    const int x = corners[0][i].x, y = corners[0][i].y;
    if (x < 8 || y < 8 || x >= w - 8 || y >= h - 8) continue;
    svs_candidate_point p;
    std::memset(&p, 0, sizeof p);
    const double d = 6.0, z = cam.f * cam.b / d;
    p.xyz_anchor[0] = (x - cam.cx) / cam.f * z; p.xyz_anchor[1] = (y - cam.cy) / cam.f * z; p.xyz_anchor[2] = z;
    p.anchor_obs_pyr[0] = x; p.anchor_obs_pyr[1] = y; p.anchor_obs_pyr[2] = x - d;
    p.anchor_level = 0; p.kf_index = 1; p.point_id = 7000 + (int)pts.size();
    pts.push_back(p);
  }
  if (pts.size() < 40) { std::printf("REGISTER_MAP few corners %zu\n", pts.size()); return 6; }
  const double I[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};
  RegistrationKeyframe k;
  std::memset(&k, 0, sizeof k);
  std::memcpy(k.kf.T_anchor_from_w, I, sizeof I);
  for (int l = 0; l < 3; ++l) { k.kf.pyr[l] = fr.pyr(l); k.kf.stride[l] = fr.stride(l); }
  std::vector<RegistrationKeyframe> kfs(3, k);
  kfs[0].frame_id = 10; kfs[0].in_double_window = true; kfs[0].direct_neighbor = true;
  kfs[1].frame_id = 11; kfs[1].in_double_window = true; kfs[1].direct_neighbor = false;
  kfs[2].frame_id = 12; kfs[2].in_double_window = true; kfs[2].direct_neighbor = false;
  std::vector<int32_t> ob(1, 0), ok;
  for (size_t i = 0; i < pts.size(); ++i) { ok.push_back(1); if (i % 2) ok.push_back(2); ob.push_back((int32_t)ok.size()); }
  RegistrationFrame root;
  root.table_entry = 0; root.d_disp = fr.disp(); root.disp_stride = fr.stride(0);
  for (int l = 0; l < 3; ++l) root.cell_grid2d[l] = fast.cell_grid2d(l);
  std::memcpy(root.T_from_world, I, sizeof I);

  // the stateless adaptor call: the yardstick
  BackendRegistration reg(ctx, cam, 512, 8, 2048);
  if (!reg.ok()) return 7;
  double T[12];
  std::vector<std::pair<int, int> > strength;
  std::vector<TrackPoint> track;
  if (!reg.localRegisterFrame(root, kfs, pts, ob, ok, T, &strength, &track)) { std::printf("REGISTER_MAP stateless failed: status %d\n", reg.lastResult().status); return 8; }
  const svs_reg_result local = reg.lastResult();
  const std::vector<int32_t> local_acc = reg.lastAccepted();

  // the map, through the adaptor
  BackendMap map(ctx, 16, 8192, 4096);
  if (!map.ok()) return 9;
  std::vector<RegistrationFrame> frames(3, root);
  std::vector<svs_candidate_point> mpts(pts);
  std::vector<int32_t> op, okf, window;
  for (size_t i = 0; i < mpts.size(); ++i) {
    mpts[i].kf_index = 11;      // the anchor's ID
    op.push_back(mpts[i].point_id); okf.push_back(11);
    if (i % 2) { op.push_back(mpts[i].point_id); okf.push_back(12); }
  }
  for (int i = 0; i < 3; ++i) window.push_back(kfs[i].frame_id);
  if (!map.addKeyframes(kfs, frames) || !map.addPoints(mpts) || !map.addObservations(op, okf) || !map.setWindow(window)) { std::puts("REGISTER_MAP update refused"); return 10; }
  if (map.addKeyframes(kfs, frames)) { std::puts("REGISTER_MAP duplicate keyframes accepted"); return 11; }
  const std::vector<int32_t> walk(window), direct(1, 10);
  double Tm[12];
  std::vector<std::pair<int, int> > mstrength;
  std::vector<TrackPoint> mtrack;
  if (!reg.registerFrames(map, SVS_REG_LOCAL, 10, I, walk, direct, Tm, &mstrength, &mtrack)) { std::printf("REGISTER_MAP local failed: status %d\n", reg.lastResult().status); return 12; }
  if (std::memcmp(&local, &reg.lastResult(), sizeof local) != 0) { std::puts("REGISTER_MAP local result differs from the stateless call"); return 13; }
  if (std::memcmp(local_acc.data(), reg.lastAccepted().data(), sizeof(int32_t) * 512) != 0) { std::puts("REGISTER_MAP accepted flags differ from the stateless call"); return 14; }
  if (mstrength != strength || std::memcmp(T, Tm, sizeof T) != 0) { std::puts("REGISTER_MAP neighborid_to_strength differs from the stateless call"); return 15; }
  if ((int)mtrack.size() != local.n_accepted) { std::puts("REGISTER_MAP track points differ"); return 16; }

  // the C call, directly: both modes in one batch
  svs_reg_map_request q[2];
  std::memset(q, 0, sizeof q);
  const int32_t query[1] = {11};
  for (int m = 0; m < 2; ++m) {
    q[m].mode = m == 0 ? SVS_REG_LOCAL : SVS_REG_LOOP; q[m].root_kf = 10;
    std::memcpy(q[m].T_root_from_world, I, sizeof I);
    q[m].n_walk = m == 0 ? 3 : 1; q[m].h_walk_kf = m == 0 ? walk.data() : query;
    q[m].n_direct = m == 0 ? 1 : 0; q[m].h_direct_kf = m == 0 ? direct.data() : nullptr;
  }
  svs_reg *direct_reg = nullptr;
  if (!ctx.check(svs_reg_create(ctx.get(), &cam, 2, 512, 8, 2048, &direct_reg))) return 17;
  svs_reg_result res[2];
  std::vector<int32_t> acc(2 * 512), csrc(2 * 512), pid(2 * 512), kid(2 * 8);
  std::vector<svs_match_result> m2(2 * 512);
  std::vector<svs_reg_kf_stats> kst(2 * 8);
  int32_t nkf[2];
  const bool called = ctx.check(svs_reg_register_map_batch(direct_reg, map.get(), 2, q, nullptr, res, csrc.data(), m2.data(), nullptr, acc.data(), kst.data(), nullptr,
                                                           pid.data(), kid.data(), nkf));
  svs_reg_destroy(direct_reg);
  if (!called) return 18;
  if (std::memcmp(&res[0], &local, sizeof local) != 0) { std::puts("REGISTER_MAP C call differs"); return 19; }
  if (nkf[0] != 3 || kid[0] != 10 || kid[1] != 11 || kid[2] != 12 || nkf[1] != 2 || kid[8] != 10 || kid[9] != 11) { std::puts("REGISTER_MAP keyframe table differs"); return 20; }
  for (size_t i = 0, j = 0; i < 512; ++i) {
    if (!acc[i]) continue;
    const TrackPoint &t = mtrack[j++];
    if (t.global_id != pid[i] || t.global_id != pts[(size_t)csrc[i]].point_id || std::memcmp(t.uvu, m2[i].obs, sizeof t.uvu) != 0 || t.anchor_level != 0) { std::puts("REGISTER_MAP track point"); return 21; }
  }
  // loop mode through the adaptor
  std::vector<TrackPoint> ltrack;
  std::vector<std::pair<int, int> > lstrength;
  const std::vector<int32_t> qwalk(1, 11), none;
  if (!reg.registerFrames(map, SVS_REG_LOOP, 10, I, qwalk, none, Tm, &lstrength, &ltrack)) { std::printf("REGISTER_MAP loop failed: status %d\n", reg.lastResult().status); return 22; }
  if (std::memcmp(&res[1], &reg.lastResult(), sizeof res[1]) != 0) { std::puts("REGISTER_MAP loop result differs"); return 23; }
  if ((int)ltrack.size() != res[1].n_accepted || lstrength.size() != 1 || lstrength[0].first != 10 || lstrength[0].second != res[1].n_accepted) { std::puts("REGISTER_MAP loop track points differ"); return 24; }
  std::printf("REGISTER_MAP ok %d %zu candidates %d obs %d %d\n", mstrength[0].second, ltrack.size(), res[0].n_candidates, res[0].n_obs_pass1, res[0].n_obs_pass2);
  return 0;
}
