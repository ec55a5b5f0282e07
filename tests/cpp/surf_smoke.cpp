// Drives scavislam_hip::SurfPlaces and PlaceRecognizerGeom::addPlaceFromSurf the way PlaceRecognizer::addLocation starts (placerecognizer.cpp:212-246, :299):
// tests/test_gpu_surf.py writes two keyframes and compares the lines with the Python calls.
// argv[1]: int32 w, h; f64 f, cx, cy, b; then per keyframe (two of them) u8 image[h][w], f32 disp[h][w]
#include <cstdio>
#include <cstring>
#include <vector>

#include "scavislam_hip.hpp"

template <class T>
static bool rd(FILE *f, T *p, size_t n) { return std::fread(p, sizeof(T), n, f) == n; }
static unsigned bits(float v) { unsigned b; std::memcpy(&b, &v, 4); return b; }

int main(int argc, char **argv) {
  if (argc < 2) return 2;
  FILE *f = std::fopen(argv[1], "rb");
  if (!f) return 2;
  int32_t wh[2];
  double c[4];
  if (!rd(f, wh, 2) || !rd(f, c, 4)) return 2;
  const int w = wh[0], h = wh[1];
  std::vector<uint8_t> img[2];
  std::vector<float> disp[2];
  for (int k = 0; k < 2; ++k) {
    img[k].resize((size_t)w * h); disp[k].resize((size_t)w * h);
    if (!rd(f, img[k].data(), img[k].size()) || !rd(f, disp[k].data(), disp[k].size())) return 2;
  }
  std::fclose(f);
  scavislam_hip::Context ctx(0);
  if (!ctx.ok()) { std::puts("nodev"); return 3; }
  svs_cam cam;
  cam.f = c[0]; cam.cx = c[1]; cam.cy = c[2]; cam.b = c[3]; cam.w = w; cam.h = h;
  scavislam_hip::SurfPlaces surf(ctx, cam, w, h, 1, 1024);
  scavislam_hip::PlaceRecognizerGeom pr(ctx, cam, 64, 1024, 2);
  if (!surf.ok() || !pr.ok()) return 4;
  for (int k = 0; k < 2; ++k) {
    if (!surf.addLocation(img[k].data(), disp[k].data())) return 5;
    std::printf("PLACE %d %d %d\n", k, surf.size(), surf.overflow() ? 1 : 0);
    for (int i = 0; i < surf.size(); ++i) {
      const svs_surf_keypoint &p = surf.keypoints()[i];
      std::printf("KP %d %08x %08x %08x %08x %08x %d %d %08x %08x\n", k, bits(p.x), bits(p.y), bits(p.size), bits(p.angle), bits(p.response), p.octave, p.laplacian,
                  bits(surf.descriptors()[(size_t)i * 64]), bits(surf.descriptors()[(size_t)i * 64 + 63]));
    }
    if (!pr.addPlaceFromSurf(k, 100 + k, surf)) return 6;
  }
  scavislam_hip::DetectedLoop loop;
  pr.setSeed(5);
  const bool found = pr.geometricCheck(1, 0, &loop);
  std::printf("LOOP %d %d %d %d %d\n", found ? 1 : 0, loop.query_keyframe_id, loop.loop_keyframe_id, pr.lastResult().n_matches, pr.lastResult().n_inliers);
  return 0;
}
