// Drives scavislam_hip::PlaceRecognizerGeom the way PlaceRecognizer::addLocation / geometricCheck would (tests/test_gpu_loop.py compares with the Python call).
// argv[1]: int32 K, nq, nt; f64 f, cx, cy, b; u64 seed; f32 q_desc[nq][K]; f64 q_uvu[nq][3]; f32 t_desc[nt][K]; f64 t_uvu[nt][3]
#include <cinttypes>
#include <cstdio>
#include <vector>

#include "scavislam_hip.hpp"

template <class T>
static bool rd(FILE *f, T *p, size_t n) { return std::fread(p, sizeof(T), n, f) == n; }

int main(int argc, char **argv) {
  if (argc < 2) return 2;
  FILE *f = std::fopen(argv[1], "rb");
  if (!f) return 2;
  int32_t hdr[3];
  double cam4[4];
  uint64_t seed;
  if (!rd(f, hdr, 3) || !rd(f, cam4, 4) || !rd(f, &seed, 1)) return 2;
  const int K = hdr[0], nq = hdr[1], nt = hdr[2];
  std::vector<float> qd((size_t)nq * K), td((size_t)nt * K);
  std::vector<double> qu((size_t)nq * 3), tu((size_t)nt * 3);
  if (!rd(f, qd.data(), qd.size()) || !rd(f, qu.data(), qu.size()) || !rd(f, td.data(), td.size()) || !rd(f, tu.data(), tu.size())) return 2;
  std::fclose(f);
  scavislam_hip::Context ctx(0);
  if (!ctx.ok()) { std::puts("nodev"); return 3; }
  svs_cam cam = {cam4[0], cam4[1], cam4[2], cam4[3], 640, 480};
  scavislam_hip::PlaceRecognizerGeom pr(ctx, cam, K, nq > nt ? nq : nt, 4);
  if (!pr.ok()) return 4;
  pr.setSeed(seed);
  if (!pr.addPlace(0, 17, nt, td.data(), tu.data()) || !pr.addPlace(1, 42, nq, qd.data(), qu.data())) return 5;
  scavislam_hip::DetectedLoop loop;
  const bool found = pr.geometricCheck(1, 0, &loop);
  const svs_loop_result &r = pr.lastResult();
  std::printf("LOOP %d %d %d %d %d %d %d\n", found ? 1 : 0, loop.query_keyframe_id, loop.loop_keyframe_id, r.n_matches, r.n_inliers, r.best_hyp, r.n_invalid_hyp);
  std::printf("T");
  for (int i = 0; i < 12; ++i) std::printf(" %.17g", loop.T_query_from_loop[i]);
  std::printf("\n");
  return 0;
}
