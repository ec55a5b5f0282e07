// Drives scavislam_hip::PlaceRecognizerGeom::setVocabulary / addLocation the way PlaceRecognizer::addLocation runs from placerecognizer.cpp:248 onwards
// (tests/test_gpu_place_index.py writes the scenario and reads the lines).
// argv[1]: int32 K, n_words, n_places, max_desc; f64 f, cx, cy, b; f32 words[n_words][K]; per place: int32 n; f32 desc[n][K]; f64 uvu[n][3]
#include <cstdio>
#include <vector>

#include "scavislam_hip.hpp"

template <class T>
static bool rd(FILE *f, T *p, size_t n) { return std::fread(p, sizeof(T), n, f) == n; }

int main(int argc, char **argv) {
  if (argc < 2) return 2;
  FILE *f = std::fopen(argv[1], "rb");
  if (!f) return 2;
  int32_t hdr[4];
  double cam4[4];
  if (!rd(f, hdr, 4) || !rd(f, cam4, 4)) return 2;
  const int K = hdr[0], n_words = hdr[1], n_places = hdr[2], max_desc = hdr[3];
  std::vector<float> words((size_t)n_words * K);
  if (!rd(f, words.data(), words.size())) return 2;
  scavislam_hip::Context ctx(0);
  if (!ctx.ok()) { std::puts("nodev"); return 3; }
  svs_cam cam = {cam4[0], cam4[1], cam4[2], cam4[3], 640, 480};
  scavislam_hip::PlaceRecognizerGeom pr(ctx, cam, K, max_desc, n_places);
  if (!pr.ok() || !pr.setVocabulary(n_words, words.data())) return 4;
  for (int p = 0; p < n_places; ++p) {
    int32_t n;
    if (!rd(f, &n, 1) || n < 1 || n > max_desc) return 2;
    std::vector<float> desc((size_t)n * K);
    std::vector<double> uvu((size_t)n * 3);
    if (!rd(f, desc.data(), desc.size()) || !rd(f, uvu.data(), uvu.size())) return 2;
    if (!pr.addPlace(p, 100 + p, n, desc.data(), uvu.data())) return 5;
    int ex[3], ne = 0;
    for (int q = p; q >= 0 && q > p - 3; --q) ex[ne++] = q;      // itself and its two predecessors
    scavislam_hip::DetectedLoop loop;
    loop.query_keyframe_id = loop.loop_keyframe_id = -1;
    const bool found = pr.addLocation(p, 100 + p, true, ex, ne, &loop);
    if (pr.error()) return 6;
    const svs_loop_location_result &r = pr.lastLocation();
    std::printf("LOC %d %d %d %d %d %.9g %d %d %d %d\n", p, found ? 1 : 0, r.number_of_words, r.n_scored, r.best_slot, (double)r.best_score, r.candidate,
                loop.query_keyframe_id, loop.loop_keyframe_id, r.candidate ? pr.lastResult().n_inliers : -1);
  }
  std::fclose(f);
  return 0;
}
