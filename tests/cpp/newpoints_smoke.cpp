// Drives the resident newpoint_map of the C++ adaptor (include/scavislam_hip.hpp: StereoFrontend::reserveNewpoints / addNewPointsResident / addMorePointsResident /
// setCandidatesFromNewpoints / pruneNewpoints / newpoints) on the GPU: the records seeded into the store are those addNewPoints hands back, a step on the list
// composed from the store returns the records of a step on the same list set from the host, and the prune removes exactly the step's accepted new matches.
// tests/test_gpu_newpoints.py compiles and runs it.  Prints "NEWPOINTS ok <seeded> <removed> <more>".
#include <cstdio>
#include <cstring>
#include <vector>

#include "scavislam_hip.hpp"

using namespace scavislam_hip;

#define CHECK(c) do { if (!(c)) { std::printf("NEWPOINTS failed at line %d: %s\n", __LINE__, #c); return 1; } } while (0)

int main() {
  Context ctx(0);
  if (!ctx.ok()) { std::puts("NODEVICE"); return 3; }
  const int w = 320, h = 240;
  const svs_cam cam = {285.0, 160.0, 120.0, 0.075, w, h};
  std::vector<uint8_t> img((size_t)w * h);
  std::vector<float> disp((size_t)w * h);
  unsigned s = 12345u;
  for (size_t i = 0; i < img.size(); ++i) { s = s * 1664525u + 1013904223u; img[i] = (uint8_t)(s >> 24); disp[i] = 4.f + (float)((s >> 12) & 7); }
  const svs_frontend_params prm = StereoFrontend::referenceParams(false);
  const Image8 left = {img.data(), w, h, w};
  const ImageF dimg = {disp.data(), w, h, w};
  const double I[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};
  StereoFrontend fe(ctx, cam, prm, 1024, 2), twin(ctx, cam, prm, 1024, 2);
  CHECK(fe.ok() && twin.ok());
  CHECK(fe.processFirstFrame(left, nullptr, &dimg) && twin.processFirstFrame(left, nullptr, &dimg));
  int32_t np[3], np_host[3];
  std::vector<int32_t> ids, counts;
  std::vector<svs_candidate_point> rec, host;
  CHECK(!fe.addNewPointsResident(7, 1, 42u, np));                  // nothing reserved
  CHECK(fe.reserveNewpoints(2000, 4) && !fe.reserveNewpoints(2000, 4));
  // seeded into the store = handed back to the host
  CHECK(fe.addNewPointsResident(7, 1, 42u, np) && twin.addNewPoints(7, 1, 42u, &host, np_host));
  CHECK(np[0] == np_host[0] && np[1] == np_host[1] && np[2] == np_host[2]);
  CHECK(fe.newpoints(&ids, &counts, &rec) && ids.size() == 1 && ids[0] == 7 && counts[0] == (int32_t)host.size() && rec.size() == host.size() && host.size() > 100);
  CHECK(std::memcmp(rec.data(), host.data(), sizeof(svs_candidate_point) * host.size()) == 0);
  // the list from the store (keyframe 7 kept in slot 1, an absent neighbour 9) = the list from the host
  CHECK(fe.keepKeyframe(1, I) && twin.keepKeyframe(1, I));
  const std::vector<int32_t> keys = {7, 9}, slots = {-1, 7};
  svs_newpoints_list_result lr;
  CHECK(fe.setCandidatesFromNewpoints(keys, slots, std::vector<svs_candidate_point>(), &lr));
  CHECK(lr.n_points == (int32_t)host.size() && lr.n_head == lr.n_points && lr.n_groups == 3 && lr.n_no_slot == 0 && !lr.over_capacity);
  for (size_t i = 0; i < host.size(); ++i) host[i].kf_index = 1;
  const std::vector<int32_t> ends = {(int32_t)host.size(), (int32_t)host.size(), (int32_t)host.size()};
  CHECK(twin.setCandidateLists(host, ends));
  double T[12], Tt[12];
  std::memcpy(T, I, sizeof T); std::memcpy(Tt, I, sizeof Tt);
  svs_frame_result res, tres;
  std::vector<svs_match_result> m, tm;
  std::vector<svs_gated_point> g, tg;
  fe.processFrame(left, nullptr, &dimg, T, I, &res, &m, &g);
  twin.processFrame(left, nullptr, &dimg, Tt, I, &tres, &tm, &tg);
  CHECK(m.size() == tm.size() && std::memcmp(m.data(), tm.data(), sizeof(svs_match_result) * m.size()) == 0 && std::memcmp(T, Tt, sizeof T) == 0);
  // the prune takes the accepted new matches out of the store, stably
  int32_t want = 0, removed = -1;
  std::vector<svs_candidate_point> kept;
  for (size_t i = 0; i < m.size(); ++i) {
    const bool gone = m[i].status == SVS_MATCH_OK && g[i].accepted != 0;
    want += gone ? 1 : 0;
    if (!gone) { kept.push_back(host[i]); kept.back().kf_index = rec[i].kf_index; }
  }
  CHECK(fe.pruneNewpoints(&removed) && removed == want);
  CHECK(fe.newpoints(&ids, &counts, &rec) && rec.size() == kept.size() && (kept.empty() || std::memcmp(rec.data(), kept.data(), sizeof(svs_candidate_point) * kept.size()) == 0));
  // more points behind the step, into a second list; the first keeps its place; a list dropped
  svs_seed_params sp = StereoFrontend::seedParams();
  sp.min_num_points = 100000;
  int32_t np2[3] = {0, 0, 0};
  CHECK(fe.addMorePointsResident(8, 5000, 43u, np2, &sp));
  CHECK(fe.newpoints(&ids, &counts) && ids.size() == 2 && ids[0] == 7 && ids[1] == 8 && counts[1] == np2[0] + np2[1] + np2[2]);
  const int more = counts[1];
  CHECK(fe.putNewpoints(9, kept) && fe.newpoints(&ids, &counts) && ids.size() == 3 && ids[2] == 9 && counts[2] == (int32_t)kept.size());
  int32_t found = 0;
  CHECK(fe.dropNewpointGroups(std::vector<int32_t>(1, 7), &found) && found == 1 && fe.newpoints(&ids, &counts) && ids[0] == 8);
  CHECK(fe.setCandidatesFromNewpoints(keys, slots, std::vector<svs_candidate_point>(), &lr) && !fe.pruneNewpoints());      // a new list: the step's records are gone
  std::printf("NEWPOINTS ok %zu %d %d\n", host.size(), removed, more);
  return 0;
}
