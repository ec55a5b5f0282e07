// Drives BackendRegistration::localRegisterFrame / globalLoopClosure of the C++ adaptor (include/scavislam_hip.hpp) on the GPU and checks that they hand back what
// svs_reg_register_batch called directly reports; tests/test_gpu_register.py compiles and runs it.  Prints "REGISTER ok <strength> <loop track points>".
// The scene: one noise frame that is the root AND (at the same pose) the keyframe its candidate points are anchored in, so every corner finds itself.
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
    for (int x = 0; x < w; ++x) { if (x % 4 == 0 && y % 4 == 0) s = s * 1664525u + 1013904223u; img[(size_t)y * w + x] = (uint8_t)(s >> 24); }      // 4 x 4 blocks: corners
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
  // candidate points = level-0 corners with the frame's disparity (stereo_camera.cpp:46-52), anchored in table entry 1
  std::vector<svs_candidate_point> pts;
  const size_t step = corners[0].size() / 300 + 1;      // spread over all cells: every image half needs its share (backend.cpp:707-711)
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
  if (pts.size() < 40) { std::printf("REGISTER few corners %zu\n", pts.size()); return 6; }
  const double I[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};
  RegistrationKeyframe k;
  std::memset(&k, 0, sizeof k);
  std::memcpy(k.kf.T_anchor_from_w, I, sizeof I);
  for (int l = 0; l < 3; ++l) { k.kf.pyr[l] = fr.pyr(l); k.kf.stride[l] = fr.stride(l); }
  std::vector<RegistrationKeyframe> kfs(3, k);
  kfs[0].frame_id = 10; kfs[0].in_double_window = true; kfs[0].direct_neighbor = true;       // the root
  kfs[1].frame_id = 11; kfs[1].in_double_window = true; kfs[1].direct_neighbor = false;      // the anchor: observes every point
  kfs[2].frame_id = 12; kfs[2].in_double_window = true; kfs[2].direct_neighbor = false;      // observes every second point, anchors none: not in the vertex table
  std::vector<int32_t> ob(1, 0), ok;
  for (size_t i = 0; i < pts.size(); ++i) { ok.push_back(1); if (i % 2) ok.push_back(2); ob.push_back((int32_t)ok.size()); }
  RegistrationFrame root;
  root.table_entry = 0; root.d_disp = fr.disp(); root.disp_stride = fr.stride(0);
  for (int l = 0; l < 3; ++l) root.cell_grid2d[l] = fast.cell_grid2d(l);
  std::memcpy(root.T_from_world, I, sizeof I);

  BackendRegistration reg(ctx, cam, 512, 8, 2048);
  if (!reg.ok()) return 7;
  double T[12];
  std::vector<std::pair<int, int> > strength;
  std::vector<TrackPoint> track;
  if (!reg.localRegisterFrame(root, kfs, pts, ob, ok, T, &strength, &track)) { std::printf("REGISTER local failed: status %d\n", reg.lastResult().status); return 8; }
  const svs_reg_result local = reg.lastResult();
  const std::vector<int32_t> local_acc = reg.lastAccepted();

  // the C call, directly
  std::vector<svs_keyframe> ckf(3);
  const uint8_t flags[3] = {SVS_REG_KF_IN_WINDOW | SVS_REG_KF_DIRECT_NEIGHBOR, SVS_REG_KF_IN_WINDOW, SVS_REG_KF_IN_WINDOW};
  for (int i = 0; i < 3; ++i) ckf[i] = kfs[i].kf;
  svs_reg_request q[2];
  std::memset(q, 0, sizeof q);
  for (int m = 0; m < 2; ++m) {
    q[m].mode = m == 0 ? SVS_REG_LOCAL : SVS_REG_LOOP; q[m].n_kf = 3; q[m].n_src = (int32_t)pts.size(); q[m].root_kf = 0;
    q[m].d_root_disp = fr.disp(); q[m].root_disp_stride = fr.stride(0);
    for (int l = 0; l < 3; ++l)
      for (int c = 0; c < SVS_MAX_CELLS; ++c) q[m].fast_thr[l][c] = c < (int)root.cell_grid2d[l].size() ? root.cell_grid2d[l][c] : 25;
    std::memcpy(q[m].T_root_from_world, I, sizeof I);
    q[m].h_kfs = ckf.data(); q[m].h_kf_flags = flags; q[m].h_src = pts.data(); q[m].h_obs_begin = ob.data(); q[m].h_obs_kf = ok.data();
  }
  svs_reg *direct = nullptr;
  if (!ctx.check(svs_reg_create(ctx.get(), &cam, 2, 512, 8, 2048, &direct))) return 9;
  svs_reg_result res[2];
  std::vector<int32_t> acc(2 * 512), csrc(2 * 512);
  std::vector<svs_match_result> m2(2 * 512);
  std::vector<svs_reg_kf_stats> kst(2 * 8);
  const bool called = ctx.check(svs_reg_register_batch(direct, 2, q, nullptr, res, csrc.data(), m2.data(), nullptr, acc.data(), kst.data(), nullptr));
  svs_reg_destroy(direct);
  if (!called) return 10;
  if (std::memcmp(&res[0], &local, sizeof local) != 0) { std::puts("REGISTER local result differs"); return 11; }
  if (std::memcmp(acc.data(), local_acc.data(), sizeof(int32_t) * 512) != 0) { std::puts("REGISTER local accepted flags differ"); return 12; }
  if (strength.size() != 1 || strength[0].first != 11 || strength[0].second != kst[1].strength || kst[2].strength != 0 || kst[2].in_vertex_table) {
    std::puts("REGISTER neighborid_to_strength differs"); return 13;
  }
  if ((int)track.size() != res[0].n_accepted) { std::puts("REGISTER local track points differ"); return 14; }
  for (size_t i = 0, j = 0; i < 512; ++i) {
    if (!acc[i]) continue;
    const TrackPoint &t = track[j++];
    if (t.global_id != pts[(size_t)csrc[i]].point_id || std::memcmp(t.uvu, m2[i].obs, sizeof t.uvu) != 0 || t.anchor_level != 0) { std::puts("REGISTER local track point"); return 15; }
  }
  // loop mode through the adaptor
  std::vector<TrackPoint> ltrack;
  if (!reg.globalLoopClosure(root, kfs, pts, T, &ltrack)) { std::printf("REGISTER loop failed: status %d\n", reg.lastResult().status); return 16; }
  if (std::memcmp(&res[1], &reg.lastResult(), sizeof res[1]) != 0) { std::puts("REGISTER loop result differs"); return 17; }
  if ((int)ltrack.size() != res[1].n_accepted || kst[8].strength != res[1].n_accepted || !kst[8].qualifies) { std::puts("REGISTER loop track points differ"); return 18; }
  std::printf("REGISTER ok %d %zu candidates %d obs %d %d\n", strength[0].second, ltrack.size(), res[0].n_candidates, res[0].n_obs_pass1, res[0].n_obs_pass2);
  return 0;
}
