// Drives the sub-pixel refinement through the C++ adaptor (include/scavislam_hip.hpp) on the GPU: StereoFrontend::setSubpixelAccuracy inside a step, and
// GuidedMatcher::refineSubpixel on the records of a twin front end without the option -- the two must give the same records and svs_subpix_info.
// tests/test_gpu_subpix_cpp.py compiles and runs it and holds the records it writes to argv[1] against the Python binding's.
// Prints "SUBPIX ok <records> <matched> <refined>".
#include <cstdio>
#include <cstring>
#include <vector>

#include "scavislam_hip.hpp"

using namespace scavislam_hip;

template <class T>
static bool put(std::FILE *f, const std::vector<T> &v) {
  const int32_t n = (int32_t)v.size();
  return std::fwrite(&n, 4, 1, f) == 1 && (n == 0 || std::fwrite(v.data(), sizeof(T), v.size(), f) == v.size());
}

int main(int argc, char **argv) {
  Context ctx(0);
  if (!ctx.ok()) { std::puts("NODEVICE"); return 3; }
  const int w = 320, h = 240;
  const svs_cam cam = {285.0, 160.0, 120.0, 0.075, w, h};
  svs_cam cam_vec[SVS_NUM_PYR_LEVELS];
  for (int l = 0; l < SVS_NUM_PYR_LEVELS; ++l) {
    const double s = (double)(1 << l);
    const svs_cam c = {cam.f / s, cam.cx / s, cam.cy / s, cam.b * (1 << l), (int)(w / s), (int)(h / s)};
    cam_vec[l] = c;
  }
  std::vector<uint8_t> img((size_t)w * h);
  std::vector<float> disp((size_t)w * h);
  unsigned s = 12345u;
  for (size_t i = 0; i < img.size(); ++i) { s = s * 1664525u + 1013904223u; img[i] = (uint8_t)(s >> 24); disp[i] = 4.f + (float)((s >> 12) & 7); }
  const Image8 left = {img.data(), w, h, w};
  const ImageF dimg = {disp.data(), w, h, w};
  const svs_frontend_params prm = StereoFrontend::referenceParams(false);
  const double I[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};
  svs_subpix_params sp;
  svs_subpix_params_default(&sp);
  if (sp.iterations != 8 || sp.max_shift != 1.5f || sp.eps != 0.03f) return 4;

  // three front ends on the same frame: the option on, off, and with no candidates (its pose is the dense tracker's: what the matcher predicted from)
  std::vector<svs_candidate_point> pts;
  std::vector<svs_match_result> m_on, m_off, m_none;
  std::vector<svs_gated_point> gated;
  std::vector<svs_subpix_info> info_on;
  double T_tracked[12];
  for (int k = 0; k < 3; ++k) {
    StereoFrontend fe(ctx, cam, prm, 1024, 2);
    if (!fe.ok() || !fe.processFirstFrame(left, nullptr, &dimg)) return 5;
    std::vector<svs_candidate_point> seeded;           // (every front end goes through the same calls)
    int32_t num_points[3];
    if (!fe.addNewPoints(0, 1, 42u, &seeded, num_points)) return 6;
    if (k == 0) pts = seeded;
    if (!fe.keepKeyframe(0, I)) return 7;
    if (!fe.setCandidates(k == 2 ? std::vector<svs_candidate_point>() : pts, k == 2 ? 0 : (int)pts.size())) return 8;
    if (k == 0 && !fe.setSubpixelAccuracy(&sp)) return 9;
    double T[12];
    std::memcpy(T, I, sizeof T);
    svs_frame_result res;
    std::memset(&res, 0xff, sizeof res);
    // (processFrame returns matchAndTrack's answer -- false with too few matches, as with no candidates --, so the call is judged by the record it fills)
    fe.processFrame(left, nullptr, &dimg, T, I, &res, k == 0 ? &m_on : k == 1 ? &m_off : &m_none, &gated);
    if (res.n_points != (k == 2 ? 0 : (int)pts.size())) return 10;
    if (k == 0 && !fe.subpixelInfo(&info_on, (int)pts.size())) return 11;
    if (k == 1) {                                      // refused while off
      std::vector<svs_subpix_info> none;
      if (svs_frontend_subpixel_info(fe.handle(), 0, none.data()) == SVS_OK) return 12;
    }
    if (k == 2) std::memcpy(T_tracked, res.T_cur_from_actkey, sizeof T_tracked);
  }
  // the stateless call on the twin's records
  FrameDev fr(ctx, w, h);
  if (!fr.preprocessing(left) || !fr.setDisparity(dimg)) return 13;
  std::vector<svs_keyframe> kfs(2);
  std::memset(kfs.data(), 0, sizeof(svs_keyframe) * kfs.size());
  std::memcpy(kfs[0].T_anchor_from_w, I, sizeof I);
  for (int l = 0; l < SVS_NUM_PYR_LEVELS; ++l) { kfs[0].pyr[l] = fr.pyr(l); kfs[0].stride[l] = fr.stride(l); }
  kfs[1] = kfs[0];
  GuidedMatcher gm(ctx);
  std::vector<svs_match_result> m_ref = m_off;
  std::vector<svs_subpix_info> info_ref;
  if (!gm.refineSubpixel(kfs, T_tracked, I, fr, cam_vec, pts, sp, &m_ref, &info_ref)) return 14;
  if (m_ref.size() != m_on.size() || std::memcmp(m_ref.data(), m_on.data(), sizeof(svs_match_result) * m_on.size()) != 0) { std::puts("SUBPIX records differ"); return 15; }
  if (info_ref.size() != info_on.size() || std::memcmp(info_ref.data(), info_on.data(), sizeof(svs_subpix_info) * info_on.size()) != 0) { std::puts("SUBPIX info differs"); return 16; }
  if (std::memcmp(m_off.data(), m_on.data(), sizeof(svs_match_result) * m_on.size()) == 0) { std::puts("SUBPIX changed nothing"); return 17; }
  int matched = 0, refined = 0;
  for (size_t i = 0; i < m_off.size(); ++i) { matched += m_off[i].status == SVS_MATCH_OK; refined += info_on[i].state == SVS_SUBPIX_REFINED; }
  if (argc > 1) {
    std::FILE *f = std::fopen(argv[1], "wb");
    if (!f || !put(f, pts) || !put(f, m_on) || !put(f, info_on) || std::fclose(f) != 0) return 18;
  }
  std::printf("SUBPIX ok %zu %d %d\n", pts.size(), matched, refined);
  return 0;
}
