// stereo.hip -- block-matching disparity for gfx950: StereoFrontend::calcDisparityCpu (stereo_frontend.cpp:620-653)
// = cv::StereoBM (OpenCV 2.4.2, external) with XSOBEL prefilter, 7x7 SAD over 16 n disparities (n = ui.num_disp16 = 1..10; the reference's 32 by default), texture and
// uniqueness tests, sub-pixel interpolation, left-right check (validateDisparity) and speckle filter.
// Semantics as restated in oracle/stereo.c; results are bit-identical to it (integer pipeline).
//
// One translation unit, cut by stage (all HBM/LDS-bound u8/u16 integer work, no MFMA); each part lists its kernels:
//   stereo_prefilter.inc   stereo_prefilter_kernel, stereo_prefilter16_kernel: 3x3 x-Sobel -> saturating table, written +1 into column-padded rows
//   stereo_search.inc      stereo_bm_kernel<SMALL> (32 disparities, register ring), stereo_bm_wide_kernel (every other count, and 32 under SVS_STEREO_WIDE=1),
//                          stereo_bm_edge_kernel<LANES> (the 3 leftmost output columns of either), stereo_validate_kernel (validateDisparity)
//   stereo_speckle.inc     speckle filter = connected components + saturating size count, fused with the 1/16 float conversion: by strips held in LDS
//                          (stereo_speckle_strip_kernel, _merge_, _resolve_) or on the whole frame (stereo_ccl_*, stereo_finish*)
// This file keeps the parameter block, the constants and LDS sizes the host shares with the kernels, and the C API.
#include "common.h"
#include <algorithm>
#include <cstdlib>
#include <cstdio>
#include <mutex>
#include <vector>

namespace {

constexpr int PADL = 16, PADR = 48;         // prefiltered rows are padded: pitch = w + PADL + PADR
constexpr int NDISP = 32, WSZ2 = 3;
constexpr int BM_STRIP = 96;                // output rows per wave (the six rows above a strip are summed without producing output)
constexpr int DISP_SHIFT = 4;
constexpr int FILTERED16 = -(1 << DISP_SHIFT);      // (minDisparity - 1) << 4 with minDisparity 0
constexpr int WIDE_TILE = 64, WIDE_STRIP = 48;      // any-count search: output columns (= lanes) and output rows per wave
constexpr int WIDE_MAX_NDISP = 160;
// edge kernel: threads, rows per workgroup; staged per image row: the right bytes 0 .. N+7 and the left bytes N-4 .. N+7, N / 4 + 5 dwords
constexpr int EDGE_THREADS = 256, EDGE_ROWS = 64;
constexpr size_t wide_edge_lds_bytes(int ndisp) { return sizeof(uint32_t) * (size_t)(EDGE_ROWS + 2 * WSZ2) * (size_t)(ndisp / 4 + 5); }
// strip speckle filter
constexpr int SPK_THREADS = 1024;
constexpr int SPK_NS = 10;                         // segments of a row handled in registers at once
constexpr int SPK_MAX_SEG = 40;                   // 64-pixel segments per row: w <= 2560
constexpr int SPK_TOUCH = 1 << 24;                 // mark bit of a root's saturating pixel count
// LDS bytes per strip row: label (int) + disparity (int16) per pixel, and for rows of up to SPK_NS segments the four pass masks per segment
__host__ __device__ constexpr int spk_row_bytes(int w) { return ((w + 3) & ~3) * 6 + ((w + 63) / 64 <= SPK_NS ? 4 * SPK_NS * 8 : 0); }

struct StereoDev {
  int w, h, pitch;
  int cap, texthr, uniq, speckle_window, speckle_range, disp12;
  uint8_t *lp, *rp;      // [batch][h][pitch], values + 1
  int16_t *disp16;       // [batch][h][w]
  uint16_t *cost;        // [batch][h][w]
  int32_t *label, *count;// [batch][h*w]
  // strip speckle filter: components still undecided at strip boundaries
  int strip_rows, n_strips;
  int32_t *brow;         // [batch][2 * n_strips][w]: component id of the first / last row of every strip (-1 filtered, -2 big, else node)
  int2 *pend;            // [batch][h*w]: (pixel, node) of the pixels of undecided components, a list per strip (at the strip's first pixel)
  int32_t *npend;        // [batch][n_strips]
  int timing;            // SVS_STEREO_DEBUG: phase stamps of one workgroup behind the error word
  int *err;              // the context's word (svs_ctx::stereo_err): bits set when a bounded walk of the speckle filter gave up (never expected)
  int swz;               // workgroups in XCD-contiguous order (devutil.h: xcd_contiguous)
  int ndisp;             // numberOfDisparities of the handle: 16, 32, ..., 160
};

#include "stereo_prefilter.inc"
#include "stereo_search.inc"
#include "stereo_speckle.inc"

// Dynamic LDS the two kernels ask for whose request grows with the row (every other kernel's LDS is fixed, and the strip speckle filter is only chosen where 16
// rows fit).  A workgroup of the MI355X can hold 160 KB; a launch that asks for more fails, so svs_stereo_create refuses rows that svs_stereo_compute could
// not launch.  Requests above the 64 KB a kernel gets by default are announced with hipFuncAttributeMaxDynamicSharedMemorySize at create, as for the strip kernel.
constexpr size_t LDS_WORKGROUP_BYTES = 160 * 1024, LDS_DEFAULT_BYTES = 64 * 1024;
constexpr int validate_rows(int w) { return w <= 2048 ? 4 : 1; }                                                      // image rows per workgroup
constexpr size_t validate_lds_bytes(int w) { return sizeof(int) * 2 * validate_rows(w) * (size_t)w; }                 // (disparity | cost, key) per pixel
constexpr size_t ccl_runs_lds_bytes(int w) { return sizeof(int) * (2 * (size_t)w + 2 * (size_t)((w + 63) / 64)); }    // (start, length) per pixel, two carries per segment
constexpr bool row_fits_lds(int w) { return validate_lds_bytes(w) <= LDS_WORKGROUP_BYTES && ccl_runs_lds_bytes(w) <= LDS_WORKGROUP_BYTES; }
// the widest row every path can hold: 8 w + 8 ceil(w / 64) <= 163840 (stereo_ccl_runs_kernel; stereo_validate_kernel asks for 8 w there).  Both requests grow with w
// above 2048, and up to 2048 neither exceeds 64 KB.
constexpr int STEREO_MAX_W = 20164;
// hipFuncAttributeMaxDynamicSharedMemorySize belongs to the KERNEL, not to a handle: it is only ever raised, to the largest request any handle of the process has
// made so far (a later, narrower handle must not take away what an earlier one needs at launch).  Set again at every create: the value also has to reach a device
// that sees the kernel for the first time.
struct LdsRequest { std::mutex m; size_t high = 0; };
hipError_t raise_dynamic_lds(const void *kernel, LdsRequest &r, size_t bytes) {
  std::lock_guard<std::mutex> lk(r.m);
  r.high = std::max(r.high, bytes);
  return hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)r.high);
}
LdsRequest g_lds_strip, g_lds_validate, g_lds_ccl_runs;
static_assert(row_fits_lds(STEREO_MAX_W) && !row_fits_lds(STEREO_MAX_W + 1) && row_fits_lds(2048) && row_fits_lds(2049), "STEREO_MAX_W is not the LDS bound");

// an SVS_STEREO_* switch of the environment, read when a handle is created: set and not 0
int env_flag(const char *name) { const char *e = getenv(name); return e && atoi(e) != 0; }

}  // namespace

struct svs_stereo {
  svs_ctx *ctx = nullptr;
  int w = 0, h = 0, max_batch = 0, pitch = 0;
  svs_stereo_params prm{};
  DevBuf<uint8_t> d_lp, d_rp;
  DevBuf<int16_t> d_disp16;
  DevBuf<uint16_t> d_cost;
  DevBuf<int32_t> d_label, d_count;
  int strip_rows = 0, n_strips = 0;                     // strip speckle filter (0: whole-frame path)
  DevBuf<int32_t> d_brow, d_npend;
  DevBuf<int2> d_pend;
  int debug = 0;                                      // SVS_STEREO_DEBUG=1 at create
  int force_frame_ccl = 0;                            // SVS_STEREO_FRAME_CCL=1 at create: the whole-frame union-find path (tests/test_gpu_stereo_paths.py compares the two)
  int force_prefilter4 = 0;                           // SVS_STEREO_PREFILTER4=1 at create: the generic 4-pixel prefilter kernel on aligned input too (the same file compares the two)
  int force_wide = 0;                                 // SVS_STEREO_WIDE=1 at create: 32 disparities through the any-count search (tests/test_gpu_stereo_ndisp.py compares the two)
  ~svs_stereo() { (void)hipStreamSynchronize(ctx->stream); }      // (runs before the buffers are freed)
};

extern "C" int svs_stereo_create(svs_ctx *ctx, int w, int h, int max_batch, const svs_stereo_params *prm, svs_stereo **out) {
  SVS_REQUIRE(ctx, ctx && prm && out && w > 0 && h > 0 && max_batch > 0);
  SVS_DEVICE(ctx);
  const int ndisp = prm->num_disparities;
  const bool ndisp_ok = ndisp >= 16 && ndisp <= WIDE_MAX_NDISP && ndisp % 16 == 0;
  if (prm->sad_window != 7 || prm->min_disparity != 0 || !ndisp_ok || prm->prefilter_cap < 1 || prm->prefilter_cap > 63 ||
      w < ndisp + 2 * WSZ2 || h < 2 || prm->speckle_window > 65535) {
    ctx->err = "svs_stereo: only SADWindowSize 7, minDisparity 0, numberOfDisparities 16, 32, ..., 160, preFilterCap 1..63, w >= numberOfDisparities + 6" +
               (ndisp_ok ? " (= " + std::to_string(ndisp + 2 * WSZ2) + " at " + std::to_string(ndisp) + " disparities)" : std::string()) + " are supported";
    return SVS_ERR_UNSUPPORTED;
  }
  if (w > STEREO_MAX_W) {
    ctx->err = "svs_stereo: w <= " + std::to_string(STEREO_MAX_W) + " is supported (the left-right check and the whole-frame speckle filter hold a row in the 160 KB of LDS)";
    return SVS_ERR_UNSUPPORTED;
  }
  std::unique_ptr<svs_stereo> s(new svs_stereo());
  s->ctx = ctx; s->w = w; s->h = h; s->max_batch = max_batch; s->pitch = (w + PADL + PADR + 3) & ~3; s->prm = *prm;
  s->force_frame_ccl = env_flag("SVS_STEREO_FRAME_CCL");
  s->force_prefilter4 = env_flag("SVS_STEREO_PREFILTER4");      // A/B: the generic 4-pixel kernel on aligned input too
  s->force_wide = env_flag("SVS_STEREO_WIDE");                  // A/B: 32 disparities through the any-count search too
  s->debug = env_flag("SVS_STEREO_DEBUG");
  const size_t n = (size_t)w * h * max_batch, np = (size_t)s->pitch * h * max_batch + 64;
  SVS_HIP(ctx, s->d_lp.alloc(np));
  SVS_HIP(ctx, s->d_rp.alloc(np));
  SVS_HIP(ctx, s->d_disp16.alloc(n));
  SVS_HIP(ctx, s->d_cost.alloc(n));
  SVS_HIP(ctx, s->d_label.alloc(n));
  SVS_HIP(ctx, s->d_count.alloc(n));
  // strip speckle filter where a strip of >= 16 rows (labels 4 B + disparities 2 B per pixel) fits LDS, and the saturating run counts of
  // SPK_THREADS concurrent adds stay below the mark bit
  {
    const int wp = (w + 3) & ~3;
    int strip_kb = 151;                                  // dynamic LDS of a strip; the kernel's static arrays take 6 KB of the CU's 160 KB
    { const char *e = getenv("SVS_STEREO_STRIP_KB"); if (e && atoi(e) >= 8 && atoi(e) <= 151) strip_kb = atoi(e); }      // experiment: smaller strips, more workgroups per CU
    const int rows = std::min(h, (strip_kb * 1024) / spk_row_bytes(w));
    if (rows >= 16 && w <= 64 * SPK_MAX_SEG && (size_t)rows * w < (1u << 24) && (long long)(SPK_THREADS + 1) * std::max(prm->speckle_window, w) < SPK_TOUCH) {
      s->strip_rows = rows; s->n_strips = div_up(h, rows);
      SVS_HIP(ctx, s->d_brow.alloc(2 * (size_t)s->n_strips * w * max_batch));
      SVS_HIP(ctx, s->d_pend.alloc(n));
      SVS_HIP(ctx, s->d_npend.alloc((size_t)max_batch * s->n_strips));
      SVS_HIP(ctx, hipMemset(s->d_npend, 0, sizeof(int32_t) * (size_t)max_batch * s->n_strips));
      SVS_HIP(ctx, raise_dynamic_lds((const void *)stereo_speckle_strip_kernel, g_lds_strip, (size_t)rows * spk_row_bytes(w)));
    }
  }
  if (validate_lds_bytes(w) > LDS_DEFAULT_BYTES)
    SVS_HIP(ctx, raise_dynamic_lds((const void *)stereo_validate_kernel, g_lds_validate, validate_lds_bytes(w)));
  if (ccl_runs_lds_bytes(w) > LDS_DEFAULT_BYTES)
    SVS_HIP(ctx, raise_dynamic_lds((const void *)stereo_ccl_runs_kernel, g_lds_ccl_runs, ccl_runs_lds_bytes(w)));
  *out = s.release();
  return SVS_OK;
}

extern "C" int svs_stereo_destroy(svs_stereo *s) {
  if (!s) return SVS_OK;
  delete s;
  return SVS_OK;
}

extern "C" int svs_stereo_compute(svs_stereo *s, const uint8_t *d_left, int lstride, size_t l_bstride, const uint8_t *d_right, int rstride,
                                  size_t r_bstride, float *d_disp, int dstride, size_t d_bstride, int n_batch) {
  svs_ctx *ctx = s ? s->ctx : nullptr;
  SVS_REQUIRE(ctx, s && d_left && d_right && d_disp && n_batch >= 1 && n_batch <= s->max_batch && lstride >= s->w && rstride >= s->w && dstride >= s->w);
  SVS_DEVICE(ctx);
  StereoDev S{};
  S.w = s->w; S.h = s->h; S.pitch = s->pitch;
  S.cap = s->prm.prefilter_cap; S.texthr = s->prm.texture_threshold; S.uniq = s->prm.uniqueness_ratio;
  S.speckle_window = s->prm.speckle_window; S.speckle_range = s->prm.speckle_range; S.disp12 = s->prm.disp12_max_diff;
  S.lp = s->d_lp; S.rp = s->d_rp; S.disp16 = s->d_disp16; S.cost = s->d_cost; S.label = s->d_label; S.count = s->d_count;
  S.swz = ctx->xcd_swizzle; S.ndisp = s->prm.num_disparities; S.err = ctx->stereo_err;
  const int w = s->w, h = s->h, width1 = w - S.ndisp + 1, n = w * h;
  const bool aligned16 = w % 16 == 0 && s->pitch % 16 == 0 && lstride % 4 == 0 && rstride % 4 == 0 && l_bstride % 4 == 0 && r_bstride % 4 == 0 &&
                         ((uintptr_t)d_left | (uintptr_t)d_right) % 4 == 0 && !s->force_prefilter4;
  ++(aligned16 ? ctx->stereo_n_prefilter16 : ctx->stereo_n_prefilter4);
  if (aligned16)
    hipLaunchKernelGGL(stereo_prefilter16_kernel, dim3(div_up((s->pitch / 16) * div_up(h, 4), 256), 1, 2 * n_batch), dim3(256), 0, ctx->stream, S, d_left, lstride,
                       l_bstride, d_right, rstride, r_bstride);
  else
    hipLaunchKernelGGL(stereo_prefilter_kernel, dim3(div_up(s->pitch, 256), div_up(h, 16), 2 * n_batch), dim3(64, 4), 0, ctx->stream, S, d_left, lstride,
                       l_bstride, d_right, rstride, r_bstride);
  SVS_LAUNCH_CHECK(ctx);
  if (S.ndisp != NDISP || s->force_wide) {      // the any-count search; 32 disparities keep the register-ring kernels below
    ++ctx->stereo_n_wide_search;
    hipLaunchKernelGGL(stereo_bm_edge_kernel<64>, dim3(div_up(h, EDGE_ROWS), n_batch), dim3(EDGE_THREADS), wide_edge_lds_bytes(S.ndisp), ctx->stream, S);
    SVS_LAUNCH_CHECK(ctx);
    hipLaunchKernelGGL(stereo_bm_wide_kernel, dim3(div_up(width1 - 3, WIDE_TILE), div_up(h, WIDE_STRIP), n_batch), dim3(64), (size_t)S.ndisp * 128, ctx->stream, S);
    SVS_LAUNCH_CHECK(ctx);
  } else {
    hipLaunchKernelGGL(stereo_bm_edge_kernel<32>, dim3(div_up(h, EDGE_ROWS), n_batch), dim3(EDGE_THREADS), wide_edge_lds_bytes(NDISP), ctx->stream, S);
    SVS_LAUNCH_CHECK(ctx);
    if (width1 > 3) {
      if (S.cap <= 41) hipLaunchKernelGGL(stereo_bm_kernel<true>, dim3(div_up(width1 - 3, 64), div_up(h, BM_STRIP), n_batch), dim3(64), 0, ctx->stream, S);
      else hipLaunchKernelGGL(stereo_bm_kernel<false>, dim3(div_up(width1 - 3, 64), div_up(h, BM_STRIP), n_batch), dim3(64), 0, ctx->stream, S);
      SVS_LAUNCH_CHECK(ctx);
    }
  }
  if (s->prm.disp12_max_diff >= 0) {
    { const int R = validate_rows(w); hipLaunchKernelGGL(stereo_validate_kernel, dim3(div_up(h, R), n_batch), dim3(64 * R), validate_lds_bytes(w), ctx->stream, S); }
    if (validate_rows(w) == 1) ++ctx->stereo_n_validate_wide;
    SVS_LAUNCH_CHECK(ctx);
  }
  const bool ccl = s->prm.speckle_range >= 0 && s->prm.speckle_window > 0;
  const dim3 gp(div_up(n, 256), n_batch);
  if (ccl && s->strip_rows > 0 && !s->force_frame_ccl) {
    S.strip_rows = s->strip_rows; S.n_strips = s->n_strips; S.brow = s->d_brow; S.pend = s->d_pend; S.npend = s->d_npend; S.timing = s->debug;
    ++ctx->stereo_n_strip_filter; ctx->stereo_n_strips += s->n_strips;
    hipLaunchKernelGGL(stereo_speckle_strip_kernel, dim3(s->n_strips, n_batch), dim3(SPK_THREADS), (size_t)s->strip_rows * spk_row_bytes(w), ctx->stream, S, d_disp, dstride, d_bstride);
    SVS_LAUNCH_CHECK(ctx);
    if (s->n_strips > 1) {
      hipLaunchKernelGGL(stereo_speckle_merge_kernel, dim3(s->n_strips - 1, n_batch), dim3(256), 0, ctx->stream, S);
      for (int pass = 0; pass < 2; ++pass)
        hipLaunchKernelGGL(stereo_speckle_resolve_kernel, dim3(s->n_strips, n_batch), dim3(256), 0, ctx->stream, S, pass, d_disp, dstride, d_bstride);
      SVS_LAUNCH_CHECK(ctx);
    }
    if (s->debug) {
      int ev[24] = {};
      SVS_HIP(ctx, hipMemcpyAsync(ev, S.err, sizeof(ev), hipMemcpyDeviceToHost, ctx->stream));
      SVS_HIP(ctx, hipStreamSynchronize(ctx->stream));
      const int e = ev[0];
      std::vector<int> np((size_t)n_batch * s->n_strips);
      SVS_HIP(ctx, hipMemcpy(np.data(), s->d_npend, sizeof(int) * np.size(), hipMemcpyDeviceToHost));
      long tot = 0; int mx = 0;
      for (int v : np) { tot += v; mx = std::max(mx, v); }
      { const long long *t = reinterpret_cast<const long long *>(ev + 8);
        fprintf(stderr, "[svs_stereo] strip kernel phases of one workgroup (us): load %.1f runs %.1f stitch %.1f count %.1f classify %.1f convert %.1f\n", (t[1] - t[0]) * 0.01,
                (t[2] - t[1]) * 0.01, (t[3] - t[2]) * 0.01, (t[4] - t[3]) * 0.01, (t[5] - t[4]) * 0.01, (t[6] - t[5]) * 0.01); }
      fprintf(stderr, "[svs_stereo] strip speckle filter: error mask %d, undecided pixels %ld in %d frames (max %d per strip)\n", e, tot, n_batch, mx);
    }
    return SVS_OK;
  }
  if (ccl) {
    ++ctx->stereo_n_frame_filter;
    hipLaunchKernelGGL(stereo_ccl_runs_kernel, dim3(h, n_batch), dim3(256), ccl_runs_lds_bytes(w), ctx->stream, S);
    SVS_LAUNCH_CHECK(ctx);
    if (w % 4 == 0) hipLaunchKernelGGL(stereo_ccl_merge4_kernel, dim3(div_up(n, 1024), n_batch), dim3(256), 0, ctx->stream, S);
    else hipLaunchKernelGGL(stereo_ccl_merge_kernel, gp, dim3(256), 0, ctx->stream, S);
    SVS_LAUNCH_CHECK(ctx);
    hipLaunchKernelGGL(stereo_ccl_count_kernel, dim3(div_up(n, 2048), n_batch), dim3(256), 0, ctx->stream, S); SVS_LAUNCH_CHECK(ctx);
  }
  if (w % 4 == 0) hipLaunchKernelGGL(stereo_finish4_kernel, dim3(div_up(n, 1024), n_batch), dim3(256), 0, ctx->stream, S, ccl ? 1 : 0, d_disp, dstride, d_bstride);
  else hipLaunchKernelGGL(stereo_finish_kernel, gp, dim3(256), 0, ctx->stream, S, ccl ? 1 : 0, d_disp, dstride, d_bstride);
  SVS_LAUNCH_CHECK(ctx);
  return SVS_OK;
}
