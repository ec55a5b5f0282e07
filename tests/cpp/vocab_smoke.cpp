// Drives scavislam_hip::VocabularyTrainer::createDictionary the way create_dictionary.cpp:144-177 makes its words (tests/test_gpu_vocab.py writes the points and
// compares the lines with the Python call).
// argv[1]: int32 K, n, n_words, iterations; uint64 seed; f32 desc[n][K]
#include <cstdio>
#include <cstring>
#include <vector>

#include "scavislam_hip.hpp"

template <class T>
static bool rd(FILE *f, T *p, size_t n) { return std::fread(p, sizeof(T), n, f) == n; }

int main(int argc, char **argv) {
  if (argc < 2) return 2;
  FILE *f = std::fopen(argv[1], "rb");
  if (!f) return 2;
  int32_t hdr[4];
  uint64_t seed;
  if (!rd(f, hdr, 4) || !rd(f, &seed, 1)) return 2;
  const int K = hdr[0], n = hdr[1], n_words = hdr[2], iterations = hdr[3];
  std::vector<float> desc((size_t)n * K);
  if (!rd(f, desc.data(), desc.size())) return 2;
  std::fclose(f);
  scavislam_hip::Context ctx(0);
  if (!ctx.ok()) { std::puts("nodev"); return 3; }
  scavislam_hip::VocabularyTrainer tr(ctx, K);
  tr.setIterations(iterations);
  tr.setSeed(seed);
  std::vector<float> words;
  if (!tr.createDictionary(n, desc.data(), n_words, &words)) return 4;
  const svs_vocab_result &r = tr.lastResult();
  std::printf("RES %d %d %d %d %d %llu\n", r.n_words_out, r.n_seeded, r.iterations_run, r.converged, r.n_empty, (unsigned long long)r.inertia_q28);
  for (int j = 0; j < r.n_words_out; ++j) {
    std::printf("WORD %d", j);
    for (int k = 0; k < K; ++k) {
      uint32_t bits;
      std::memcpy(&bits, &words[(size_t)j * K + k], 4);
      std::printf(" %08x", bits);
    }
    std::printf("\n");
  }
  return 0;
}
