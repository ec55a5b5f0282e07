// staging_host.cpp -- the offset part of the library's staging (scavislam_amd/csrc/pieces.h) on the host alone, meant to be built with
// -fsanitize=address,undefined: rows of pieces for alignments 16 and 64 over element sizes {1, 4, 8, 12, 16, 96} x counts {0, 1, 3, 16, 17} in mixed order.
// Checked per row: every offset a multiple of the alignment; pieces in declaration order without overlap; the gap in front of a piece below the alignment; a
// piece of count 0 takes no bytes; `end` one past the last piece and end_aligned() its round-up.  Then a block of EXACTLY `end` bytes is written in full through
// every piece's typed address (a row one byte short is AddressSanitizer's to catch, a misaligned piece UBSan's) and read back (an overlap would show as a
// neighbour's tag).  Exit status 0 = all held.
#include "../../scavislam_amd/csrc/pieces.h"
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>

#define CHECK(cond)                                                                                        \
  do {                                                                                                     \
    if (!(cond)) {                                                                                         \
      fprintf(stderr, "%s:%d: %s fails (alignment %zu, step %d, piece %zu)\n", __FILE__, __LINE__, #cond, A, step, i); \
      return 1;                                                                                            \
    }                                                                                                      \
  } while (0)

namespace {
struct E12 { int32_t v[3]; };
struct alignas(16) E16 { float v[4]; };
struct E96 { double v[12]; };
static_assert(sizeof(E12) == 12 && sizeof(E16) == 16 && sizeof(E96) == 96, "the element sizes of the rows");

struct Rec { size_t off, n, esize; void (*fill)(uint8_t *, const Rec &, uint8_t); };
template <class T> void fill(uint8_t *base, const Rec &r, uint8_t tag) {
  T *p = piece_at(base, Piece<T>{r.off, r.n});
  T v;
  memset(&v, tag, sizeof v);
  for (size_t k = 0; k < r.n; ++k) p[k] = v;
}
template <class T, size_t A> Rec declare(Pieces<A> &row, size_t n) {
  const Piece<T> p = row.template piece<T>(n);
  if (p.bytes() != n * sizeof(T) || p.end() != p.off + n * sizeof(T)) abort();
  return Rec{p.off, p.n, sizeof(T), fill<T>};
}

// the 30 (size, count) pairs, visited with stride `step` (coprime to 30: every pair once, sizes and counts mixed)
template <size_t A> int run(int step) {
  const size_t counts[5] = {0, 1, 3, 16, 17};
  Pieces<A> row;
  std::vector<Rec> recs;
  for (int j = 0; j < 30; ++j) {
    const int k = j * step % 30;
    const size_t n = counts[k / 6];
    switch (k % 6) {
      case 0: recs.push_back(declare<uint8_t>(row, n)); break;
      case 1: recs.push_back(declare<int32_t>(row, n)); break;
      case 2: recs.push_back(declare<double>(row, n)); break;
      case 3: recs.push_back(declare<E12>(row, n)); break;
      case 4: recs.push_back(declare<E16>(row, n)); break;
      default: recs.push_back(declare<E96>(row, n)); break;
    }
  }
  size_t prev_end = 0, i = 0;
  for (; i < recs.size(); ++i) {
    const Rec &r = recs[i];
    CHECK(r.off % A == 0);
    CHECK(r.off >= prev_end);               // declaration order, no overlap
    CHECK(r.off - prev_end < A);            // no more padding than the alignment asks for
    prev_end = r.off + r.n * r.esize;
    CHECK(r.n != 0 || i + 1 == recs.size() || recs[i + 1].off - r.off < A);      // a piece of count 0 takes no bytes: the next one is not pushed back (the last: `end` below)
  }
  CHECK(row.end == prev_end);
  CHECK(row.end_aligned() % A == 0 && row.end_aligned() >= row.end && row.end_aligned() - row.end < A);
  void *mem = nullptr;
  CHECK(posix_memalign(&mem, A < sizeof(void *) ? sizeof(void *) : A, row.end) == 0);
  uint8_t *base = static_cast<uint8_t *>(mem);
  for (i = 0; i < recs.size(); ++i) recs[i].fill(base, recs[i], (uint8_t)(i + 1));
  for (i = 0; i < recs.size(); ++i)
    for (size_t b = 0; b < recs[i].n * recs[i].esize; ++b) CHECK(base[recs[i].off + b] == (uint8_t)(i + 1));
  free(mem);
  return 0;
}
}  // namespace

int main() {
  for (int step : {1, 7, 11, 13, 29}) {
    if (run<16>(step)) return 1;
    if (run<64>(step)) return 1;
  }
  printf("staging_host ok\n");
  return 0;
}
