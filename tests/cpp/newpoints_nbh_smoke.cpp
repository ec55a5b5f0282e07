// Drives StereoFrontend::setNeighborhoodFromStore of the C++ adaptor (include/scavislam_hip.hpp) on the GPU, for the one-stream front end and for stream 1 of a batch
// front end, against StereoFrontend::setNeighborhoodFromMap fed the same lists from the host; tests/test_gpu_newpoint_store_nbh.py compiles and runs it.
// Prints "NEWPOINTS_NBH ok <n_points> <n_head_kept> <n_head_dropped> <n_groups>".
// The map is that of nbh_root_smoke.cpp: keyframes 0 .. 4, 0 .. 2 in the window; points 0 .. 39; edges (0, 1, 9) (2, 0, 7) (1, 2, 7) (3, 1, 5).  The front ends keep
// keyframe 0 in slot 0 and keyframe 2 in slot 1; the active keyframe is 1.  The store, in store order: lists of keyframes 2, 1 (the active one), 4 (no vertex:
// dropped) and 0.
#include <cstdio>
#include <cstring>
#include <vector>

#include "scavislam_hip.hpp"

using namespace scavislam_hip;

#define CHECK(c) do { if (!(c)) { std::printf("NEWPOINTS_NBH failed at line %d: %s\n", __LINE__, #c); return 1; } } while (0)

static std::vector<svs_candidate_point> recs(int first_id, int n, int kf_index) {
  std::vector<svs_candidate_point> v((size_t)n);
  for (int i = 0; i < n; ++i) { std::memset(&v[(size_t)i], 0, sizeof(svs_candidate_point)); v[(size_t)i].point_id = first_id + i; v[(size_t)i].kf_index = kf_index; }
  return v;
}

static bool fill(StereoFrontend &fe, int stream) {
  return fe.reserveNewpoints(32, 8) && fe.putNewpoints(2, recs(101, 2, 7), false, stream) && fe.putNewpoints(1, recs(100, 1, 7), false, stream) &&
         fe.putNewpoints(4, recs(103, 1, 7), false, stream) && fe.putNewpoints(0, recs(104, 2, 7), false, stream);
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
  CHECK(fr.preprocessing(left) && fr.setDisparity(dimg));
  const double I[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};
  BackendMap map(ctx, 16, 256, 1024);
  CHECK(map.ok());
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
  CHECK(map.addKeyframes(kfs, frames) && map.addPoints(pts) && map.addObservations(op, ok));
  std::vector<int32_t> window;
  for (int i = 0; i < 3; ++i) window.push_back(i);
  const int32_t pairs[8] = {0, 1, 2, 0, 1, 2, 3, 1}, strength[4] = {9, 7, 7, 5};
  CHECK(map.setWindow(window) && map.reserveEdges(8) &&
        map.addEdges(std::vector<int32_t>(pairs, pairs + 8), std::vector<int32_t>(strength, strength + 4), std::vector<int32_t>(4, 0)));

  const svs_frontend_params prm = StereoFrontend::referenceParams(false);
  StereoFrontend fe(ctx, cam, prm, 256, 2), twin(ctx, cam, prm, 256, 2);
  CHECK(fe.ok() && twin.ok());
  for (int slot = 0; slot < 2; ++slot) CHECK(fe.processFirstFrame(left, nullptr, &dimg) && fe.keepKeyframe(slot, I) && twin.processFirstFrame(left, nullptr, &dimg) && twin.keepKeyframe(slot, I));
  std::vector<int32_t> slots;
  slots.push_back(0); slots.push_back(2);
  // the twin's head: the active keyframe's list first, then the others in store order; kf_index = the slot that holds the list's keyframe
  std::vector<svs_candidate_point> head = recs(100, 1, -1), part = recs(101, 2, 1);
  head.insert(head.end(), part.begin(), part.end());
  part = recs(103, 1, -1); head.insert(head.end(), part.begin(), part.end());
  part = recs(104, 2, 0); head.insert(head.end(), part.begin(), part.end());
  const int32_t ends[4] = {1, 3, 4, 6}, keys[4] = {-1, 2, 4, 0};
  const std::vector<int32_t> group_end(ends, ends + 4), group_kf(keys, keys + 4);
  svs_nbr_result res, tres, none;
  std::vector<int32_t> pid, tpid, nb, tnb;
  std::vector<FrontendVertex> vm, tvm;
  CHECK(!fe.setNeighborhoodFromStore(map, 0, 1, slots, true, &res, &pid, &vm, &nb));      // nothing reserved
  CHECK(fill(fe, 0));
  CHECK(fe.setNeighborhoodFromStore(map, 0, 1, slots, true, &res, &pid, &vm, &nb));
  CHECK(twin.setNeighborhoodFromMap(map, 0, 1, slots, head, group_end, 1, group_kf, true, &tres, &tpid, &tvm, &tnb));
  CHECK(std::memcmp(&res, &tres, sizeof res) == 0 && pid == tpid && nb == tnb && vm.size() == tvm.size());
  for (size_t i = 0; i < vm.size(); ++i) CHECK(vm[i].frame_id == tvm[i].frame_id && std::memcmp(vm[i].T_me_from_w, tvm[i].T_me_from_w, sizeof I) == 0);
  CHECK(res.n_head_dropped == 1 && res.n_head_kept == 5);
  CHECK(!fe.setNeighborhoodFromStore(map, 3, 1, slots, true, &none, nullptr, nullptr, nullptr) && none.root_outside_window);
  CHECK(!fe.setNeighborhoodFromStore(map, 0, 1, slots, true, &none, nullptr, nullptr, nullptr, 10, 3) && none.over_capacity);
  double T[12], Tt[12];
  std::memcpy(T, I, sizeof I); std::memcpy(Tt, I, sizeof I);
  svs_frame_result fres, tfres;
  std::vector<svs_match_result> m, tm;
  std::vector<svs_gated_point> g, tg;
  fe.processFrame(left, nullptr, &dimg, T, I, &fres, &m, &g);
  twin.processFrame(left, nullptr, &dimg, Tt, I, &tfres, &tm, &tg);
  CHECK((int)m.size() == res.n_points && m.size() == tm.size() && std::memcmp(m.data(), tm.data(), sizeof(svs_match_result) * m.size()) == 0);

  // stream 1 of a batch front end: frames in device memory, the same store, the same result and point ids
  void *d_left = nullptr, *d_disp = nullptr;
  const size_t px = (size_t)w * h;
  CHECK(ctx.check(svs_malloc(ctx.get(), 2 * px, &d_left)) && ctx.check(svs_malloc(ctx.get(), 2 * px * sizeof(float), &d_disp)));
  for (int b = 0; b < 2; ++b)
    CHECK(ctx.check(svs_memcpy_h2d(ctx.get(), (uint8_t *)d_left + b * px, img.data(), px)) &&
          ctx.check(svs_memcpy_h2d(ctx.get(), (float *)d_disp + b * px, disp.data(), px * sizeof(float))));
  svs_frames_dev fd;
  std::memset(&fd, 0, sizeof fd);
  fd.d_left = (const uint8_t *)d_left; fd.lstride = w; fd.l_bstride = px; fd.d_disp = (const float *)d_disp; fd.dstride = w; fd.d_bstride = px;
  {
    StereoFrontend batch(ctx, cam, prm, 256, 2, 2);
    CHECK(batch.ok() && batch.streams() == 2);
    const double I2[24] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};
    for (int slot = 0; slot < 2; ++slot) CHECK(batch.processFirstFrames(&fd) && batch.keepKeyframes(slot, I2));
    CHECK(fill(batch, 1));
    svs_nbr_result bres;
    std::vector<int32_t> bpid, bnb, ids, counts;
    std::vector<FrontendVertex> bvm;
    CHECK(batch.setNeighborhoodFromStore(map, 0, 1, slots, true, &bres, &bpid, &bvm, &bnb, 10, 64, 1));
    CHECK(std::memcmp(&bres, &res, sizeof res) == 0 && bpid == pid && bnb == nb);
    CHECK(batch.newpoints(&ids, &counts, nullptr, 0) && ids.empty() && batch.newpoints(&ids, &counts, nullptr, 1) && ids.size() == 4 && ids[1] == 1);
    std::vector<int32_t> both, removed;
    both.push_back(0); both.push_back(1);
    CHECK(!batch.pruneNewpoints(both, &removed));      // no step yet: refused
    int32_t found = 0;
    CHECK(batch.dropNewpointGroups(std::vector<int32_t>(1, 4), &found, 1) && found == 1);
  }
  svs_free(ctx.get(), d_left); svs_free(ctx.get(), d_disp);
  std::printf("NEWPOINTS_NBH ok %d %d %d %d\n", res.n_points, res.n_head_kept, res.n_head_dropped, res.n_groups);
  return 0;
}
