// StereoBM of include/scavislam_hip.hpp at ui.num_disp16 = 4 (64 disparities) on one pair; tests/test_gpu_stereo_ndisp.py writes the inputs and the
// expected disparity plane (the CPU oracle's) and reads the verdict.
// usage: stereo_ndisp_smoke <left: w h then pixels> <right: pixels> <expected: w * h floats> <num_disp16>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "scavislam_hip.hpp"

using namespace scavislam_hip;

template <class T>
static bool read_vec(FILE *f, std::vector<T> *v, size_t n) { v->resize(n); return n == 0 || std::fread(v->data(), sizeof(T), n, f) == n; }

int main(int argc, char **argv) {
  if (argc < 5) return 2;
  Context ctx(0);
  if (!ctx.ok()) { std::puts("NODEVICE"); return 3; }
  FILE *f = std::fopen(argv[1], "rb");
  int wh[2];
  std::vector<uint8_t> left, right;
  if (!f || std::fread(wh, sizeof(int), 2, f) != 2 || !read_vec(f, &left, (size_t)wh[0] * wh[1])) return 4;
  std::fclose(f);
  f = std::fopen(argv[2], "rb");
  if (!f || !read_vec(f, &right, left.size())) return 4;
  std::fclose(f);
  std::vector<float> want;
  f = std::fopen(argv[3], "rb");
  if (!f || !read_vec(f, &want, left.size())) return 4;
  std::fclose(f);
  const int num_disp16 = std::atoi(argv[4]);
  FrameDev fr(ctx, wh[0], wh[1]);
  Image8 lview = {left.data(), wh[0], wh[1], wh[0]}, rview = {right.data(), wh[0], wh[1], wh[0]};
  if (!fr.preprocessing(lview)) return 5;
  StereoBM bm(ctx, wh[0], wh[1], num_disp16);
  if (!bm.ok()) { std::printf("CREATE %s\n", svs_last_error(ctx.get())); return 6; }
  std::vector<float> disp;
  if (!bm(fr, rview, &fr) || !fr.getDisparity(&disp)) return 7;
  size_t differ = 0, valid = 0, far = 0;
  for (size_t i = 0; i < disp.size(); ++i) {
    differ += std::memcmp(&disp[i], &want[i], sizeof(float)) != 0;
    valid += disp[i] >= 0;
    far += disp[i] >= 32;
  }
  std::printf("NDISP %d %zu %zu %zu\n", 16 * num_disp16, differ, valid, far);
  // a count outside 1..10 is refused, and so is a frame narrower than 16 * num_disp16 + 6
  StereoBM bad(ctx, wh[0], wh[1], 11), narrow(ctx, 16 * num_disp16 + 5, wh[1], num_disp16);
  std::printf("REFUSED %d %d\n", bad.ok() ? 0 : 1, narrow.ok() ? 0 : 1);
  return 0;
}
