// surf.hip -- svs_surf_*: detection and description of a keyframe's SURF places on the device, the start of PlaceRecognizer::addLocation
// (placerecognizer.cpp:212-246).  The arithmetic is surf_core.h (host + device, restated by tests/surf_model.py and run on the host by tests/cpp/surf_host.cpp);
// this file is the orchestration: which thread takes which item, and the lists in between.  A translation unit of its own with a build switch of its own
// (make SURF=0 compiles the stubs at the end only): OpenCV ships SURF as `nonfree`, and nothing else in the library depends on this file.
//   integral     surf_integral_rows_kernel (one wave per row, wave prefix sums) + surf_integral_cols_kernel (one thread per column, coalesced across the wave)
//   responses    surf_response_kernel: one thread per sample of every (octave, layer) plane, one launch
//   maxima       surf_maxima_kernel: one thread per position of every middle layer; test, refinement, integer-atomic append.  The list holds EVERY maximum (the
//                host grows it and repeats the launch when it was too short), so its content is a set that does not depend on arrival ...
//   order        ... and surf_order_kernel ranks that set by the total order (count of the candidates that come before), as seed_order_kernel does
//   describe     surf_orient_kernel (one wave per keypoint: disparity filter, 113 samples, 72 windows one per lane summing in sample order) and
//                surf_describe_kernel (one workgroup per keypoint, window / resize passes / patch in dynamic LDS, one lane per cell, 16-byte stores)
//   compaction   surf_compact_kernel: one workgroup per image, prefix counts in order
// Each launch covers the whole batch (blockIdx.y = image).  No float atomics anywhere.
#include "common.h"

#ifndef SVS_NO_SURF
#include "surf_core.h"
#include <algorithm>
#include <vector>

namespace {
struct surf_sync { __device__ __forceinline__ void operator()() const { __syncthreads(); } };
constexpr size_t SURF_LDS_TABLES = (sizeof(surf_tables) + 15) & ~(size_t)15;      // the describe kernel's LDS: tables, 64 output floats, the work arrays
struct surf_dims { int w, h, n_planes, n_octaves, n_layers, total_samples, total_mid; int64_t plane_elems, integral_elems; };

// ---- integral image ------------------------------------------------------------------------------------------------------------------------------------------
// grid (h + 1, batch), one wave: row y of S holds the prefix sums of image row y - 1 (row 0 and column 0 are zero); the column pass adds the rows up
__global__ __launch_bounds__(64) void surf_integral_rows_kernel(const uint8_t *__restrict__ img, int stride, size_t bstride, int w, int32_t *__restrict__ S, int64_t s_elems) {
  const int y = (int)blockIdx.x, lane = (int)threadIdx.x;
  int32_t *row = S + (int64_t)blockIdx.y * s_elems + (int64_t)y * (w + 1);
  if (y == 0) {
    for (int x = lane; x <= w; x += 64) row[x] = 0;
    return;
  }
  const uint8_t *src = img + (size_t)blockIdx.y * bstride + (size_t)(y - 1) * stride;
  if (lane == 0) row[0] = 0;
  int base = 0;
  for (int x0 = 0; x0 < w; x0 += 64) {
    const int x = x0 + lane;
    int v = x < w ? (int)src[x] : 0;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const int t = __shfl_up(v, o, 64);
      if (lane >= o) v += t;
    }
    if (x < w) row[x + 1] = base + v;
    base += __shfl(v, 63, 64);
  }
}
// grid (ceil((w + 1) / 256), batch)
__global__ __launch_bounds__(256) void surf_integral_cols_kernel(int w, int h, int32_t *__restrict__ S, int64_t s_elems) {
  const int x = (int)(blockIdx.x * 256u + threadIdx.x);
  if (x > w) return;
  int32_t *col = S + (int64_t)blockIdx.y * s_elems + x;
  int acc = 0;
  for (int y = 1; y <= h; ++y) { acc += col[(int64_t)y * (w + 1)]; col[(int64_t)y * (w + 1)] = acc; }
}

// ---- responses -----------------------------------------------------------------------------------------------------------------------------------------------
// grid (ceil(total_samples / 256), batch).  The planes were zeroed by the caller
__global__ __launch_bounds__(256) void surf_response_kernel(surf_dims dm, const surf_plane *__restrict__ planes, const int32_t *__restrict__ S, float *__restrict__ det,
                                                           float *__restrict__ trace) {
  const int idx = (int)(blockIdx.x * 256u + threadIdx.x);
  if (idx >= dm.total_samples) return;
  int p = 0;
  while (p + 1 < dm.n_planes && planes[p + 1].cum <= idx) ++p;
  const surf_plane pl = planes[p];
  const int r = idx - pl.cum, i = r / pl.samples_j, j = r - i * pl.samples_j;
  surf_response(S + (int64_t)blockIdx.y * dm.integral_elems, dm.w, pl, i, j, det + (int64_t)blockIdx.y * dm.plane_elems, trace + (int64_t)blockIdx.y * dm.plane_elems);
}

// ---- maxima --------------------------------------------------------------------------------------------------------------------------------------------------
// grid (ceil(total_mid / 256), batch): one thread per position of every middle layer.  count[b] counts EVERY keypoint; those behind `cap` are not stored
__global__ __launch_bounds__(256) void surf_maxima_kernel(surf_dims dm, const surf_plane *__restrict__ planes, const float *__restrict__ det, const float *__restrict__ trace,
                                                         float threshold, surf_cand *__restrict__ cand, int cap, int32_t *__restrict__ count) {
  int idx = (int)(blockIdx.x * 256u + threadIdx.x);
  if (idx >= dm.total_mid) return;
  int p = -1;
  for (int o = 0; o < dm.n_octaves && p < 0; ++o) {
    const int first = o * (dm.n_layers + 2), per = planes[first].rows * planes[first].cols;
    if (idx < per * dm.n_layers) p = first + 1 + idx / per, idx -= (idx / per) * per;
    else idx -= per * dm.n_layers;
  }
  if (p < 0) return;
  const surf_plane lo = planes[p - 1], m = planes[p], hi = planes[p + 1];
  const int i = idx / m.cols, j = idx - i * m.cols;
  surf_cand c;
  if (!surf_maximum(det + (int64_t)blockIdx.y * dm.plane_elems, trace + (int64_t)blockIdx.y * dm.plane_elems, lo, m, hi, i, j, threshold, &c)) return;
  const int at = atomicAdd(count + blockIdx.y, 1);
  if (at < cap) cand[(size_t)blockIdx.y * cap + at] = c;
}

// ---- order ---------------------------------------------------------------------------------------------------------------------------------------------------
// grid (ceil(longest list / 256), batch): the rank of a candidate = how many come before it; the order is total, so the ranks are a permutation
__global__ __launch_bounds__(256) void surf_order_kernel(const surf_cand *__restrict__ cand, int cap, const int32_t *__restrict__ count, int max_kp,
                                                        svs_surf_keypoint *__restrict__ sorted) {
  const int n = count[blockIdx.y], i = (int)(blockIdx.x * 256u + threadIdx.x);
  if (i >= n) return;
  const surf_cand *L = cand + (size_t)blockIdx.y * cap;
  const surf_cand me = L[i];
  int rank = 0;
  for (int k = 0; k < n; ++k) rank += surf_before(L[k], me) ? 1 : 0;
  if (rank >= max_kp) return;
  svs_surf_keypoint kp;
  kp.x = me.x; kp.y = me.y; kp.size = me.size; kp.angle = -1.f; kp.response = me.response; kp.octave = me.octave; kp.laplacian = me.laplacian; kp.pad_ = 0;
  sorted[(size_t)blockIdx.y * max_kp + rank] = kp;
}

// ---- orientation ---------------------------------------------------------------------------------------------------------------------------------------------
// grid (longest sorted list, batch), one wave per keypoint.  keep[k] = the keypoint stays; dir[k] = direction of its descriptor window
__global__ __launch_bounds__(64) void surf_orient_kernel(surf_dims dm, const surf_tables *__restrict__ tables, const int32_t *__restrict__ S, const float *__restrict__ disp,
                                                        int dstride, size_t d_bstride, const int32_t *__restrict__ count, int max_kp, svs_surf_keypoint *__restrict__ sorted,
                                                        double *__restrict__ uvu, float *__restrict__ dir, int32_t *__restrict__ keep) {
  __shared__ surf_ori_work wk;
  __shared__ surf_tables tb;
  const int n = min(count[blockIdx.y], max_kp), k = (int)blockIdx.x, tid = (int)threadIdx.x;
  if (k >= n) return;
  const size_t at = (size_t)blockIdx.y * max_kp + k;
  const svs_surf_keypoint kp = sorted[at];
  double u[3] = {(double)kp.x, (double)kp.y, (double)kp.x};
  bool ok = true;
  if (disp) ok = surf_disparity(disp + (size_t)blockIdx.y * d_bstride, dstride, dm.w, dm.h, kp.x, kp.y, u);
  if (!ok) {      // uniform: every lane read the same keypoint
    if (tid == 0) keep[at] = 0;
    return;
  }
  for (int q = tid; q < (int)(sizeof(surf_tables) / 4); q += 64) reinterpret_cast<uint32_t *>(&tb)[q] = reinterpret_cast<const uint32_t *>(tables)[q];
  __syncthreads();
  float angle = 0.f, d = 0.f;
  ok = surf_orientation(S + (int64_t)blockIdx.y * dm.integral_elems, dm.w, dm.h, tb, kp.x, kp.y, kp.size, wk, tid, 64, surf_sync(), &angle, &d);
  if (tid == 0) {
    keep[at] = ok ? 1 : 0;
    if (ok) { sorted[at].angle = angle; dir[at] = d; uvu[3 * at] = u[0]; uvu[3 * at + 1] = u[1]; uvu[3 * at + 2] = u[2]; }
  }
}

// ---- descriptor ----------------------------------------------------------------------------------------------------------------------------------------------
// grid (longest sorted list, batch), 256 threads per keypoint; dynamic LDS sized for the largest window of the parameter set
__global__ __launch_bounds__(256) void surf_describe_kernel(surf_dims dm, const surf_tables *__restrict__ tables, const uint8_t *__restrict__ img, int stride, size_t bstride,
                                                           const int32_t *__restrict__ count, int max_kp, const svs_surf_keypoint *__restrict__ sorted,
                                                           const float *__restrict__ dir, const int32_t *__restrict__ keep, int max_win, float *__restrict__ desc) {
  // everything in the dynamic region, every carve a multiple of 16 bytes: statics in front of it would shift its base off 16-byte alignment
  extern __shared__ __align__(16) uint8_t s_lds[];
  surf_tables &tb = *reinterpret_cast<surf_tables *>(s_lds);
  float *s_out = reinterpret_cast<float *>(s_lds + SURF_LDS_TABLES);
  uint8_t *s_work = s_lds + SURF_LDS_TABLES + 256;
  const int n = min(count[blockIdx.y], max_kp), k = (int)blockIdx.x, tid = (int)threadIdx.x;
  if (k >= n) return;
  const size_t at = (size_t)blockIdx.y * max_kp + k;
  if (!keep[at]) return;
  const svs_surf_keypoint kp = sorted[at];
  const int win = surf_window_size(kp.size);
  if (win < 1 || win > max_win) return;      // (never: the handle sized max_win for the largest size the refinement can return)
  for (int q = tid; q < (int)(sizeof(surf_tables) / 4); q += 256) reinterpret_cast<uint32_t *>(&tb)[q] = reinterpret_cast<const uint32_t *>(tables)[q];
  __syncthreads();
  surf_descriptor(img + (size_t)blockIdx.y * bstride, stride, dm.w, dm.h, tb, kp.x, kp.y, kp.size, dir[at], surf_desc_work_at(s_work, win), tid, 256, surf_sync(), s_out);
  if (tid < 16) reinterpret_cast<float4 *>(desc + at * 64)[tid] = reinterpret_cast<const float4 *>(s_out)[tid];
}

// ---- compaction ----------------------------------------------------------------------------------------------------------------------------------------------
// grid (batch), 256 threads: the kept keypoints of an image move to the front of the output arrays, in order
__global__ __launch_bounds__(256) void surf_compact_kernel(const int32_t *__restrict__ count, int max_kp, const svs_surf_keypoint *__restrict__ sorted,
                                                          const double *__restrict__ uvu, const float *__restrict__ desc, const int32_t *__restrict__ keep,
                                                          svs_surf_keypoint *__restrict__ o_kp, double *__restrict__ o_uvu, float *__restrict__ o_desc,
                                                          int32_t *__restrict__ o_count) {
  __shared__ int s_scan[256];
  const int n = min(count[blockIdx.x], max_kp), tid = (int)threadIdx.x;
  const size_t row0 = (size_t)blockIdx.x * max_kp;
  int base = 0;
  for (int k0 = 0; k0 < n; k0 += 256) {
    const int k = k0 + tid, f = k < n ? keep[row0 + k] : 0;
    __syncthreads();
    s_scan[tid] = f;
    __syncthreads();
    for (int off = 1; off < 256; off <<= 1) {
      const int t = tid >= off ? s_scan[tid - off] : 0;
      __syncthreads();
      s_scan[tid] += t;
      __syncthreads();
    }
    const int pos = base + s_scan[tid] - f;
    if (f) {
      o_kp[row0 + pos] = sorted[row0 + k];
      for (int q = 0; q < 3; ++q) o_uvu[3 * (row0 + pos) + q] = uvu[3 * (row0 + k) + q];
      for (int q = 0; q < 16; ++q) reinterpret_cast<float4 *>(o_desc + (row0 + pos) * 64)[q] = reinterpret_cast<const float4 *>(desc + (row0 + k) * 64)[q];
    }
    base += s_scan[255];
  }
  if (tid == 0) o_count[blockIdx.x] = base;
}
}  // namespace

struct svs_surf {
  svs_ctx *ctx = nullptr;
  svs_surf_params prm{};
  surf_dims dm{};
  int max_batch = 0, max_kp = 0, cap = 0, max_win = 0, n_last = 0, last_had_disp = 0;
  size_t lds = 0;
  DevBuf<int32_t> d_S, d_count, d_keep, d_ocount;
  DevBuf<float> d_det, d_trace, d_dir, d_desc, d_odesc;
  DevBuf<surf_plane> d_planes;
  DevBuf<surf_tables> d_tables;
  DevBuf<surf_cand> d_cand;
  DevBuf<svs_surf_keypoint> d_sorted, d_okp;
  DevBuf<double> d_uvu, d_ouvu;
  PinnedBuf<int32_t> h_count;                         // [2][max_batch]: every maximum, the kept
  std::unique_ptr<int32_t[]> n_out;                   // host: kept per image of the last call
  int timing = 0; owned::Event ev[SVS_SURF_STAGES + 1]; float stage_ms[SVS_SURF_STAGES] = {};
  ~svs_surf() { if (ctx) { (void)hipSetDevice(ctx->device); (void)hipStreamSynchronize(ctx->stream); } }      // (before the members go, also when create gives up)
};

#define SURF_REFUSE(ctx, cond, code)                                                                         \
  do {                                                                                                       \
    if (!(cond)) {                                                                                           \
      char buf_[512];                                                                                        \
      snprintf(buf_, sizeof buf_, "%s:%d refused: %s", __FILE__, __LINE__, #cond);                           \
      (ctx)->err = buf_;                                                                                     \
      return code;                                                                                           \
    }                                                                                                        \
  } while (0)

extern "C" void svs_surf_params_default(svs_surf_params *p) {
  if (!p) return;
  p->hessian_threshold = 600.f; p->n_octaves = 2; p->n_octave_layers = 2; p->require_disparity = 1;
}

extern "C" int svs_surf_destroy(svs_surf *s) {
  if (!s) return SVS_OK;
  delete s;
  return SVS_OK;
}

static int surf_alloc(svs_surf *s) {
  svs_ctx *ctx = s->ctx;
  const size_t B = (size_t)s->max_batch, rows = B * s->max_kp;
  SVS_HIP(ctx, s->d_S.alloc(B * s->dm.integral_elems));
  SVS_HIP(ctx, s->d_det.alloc(B * s->dm.plane_elems));
  SVS_HIP(ctx, s->d_trace.alloc(B * s->dm.plane_elems));
  SVS_HIP(ctx, s->d_planes.alloc(SURF_MAX_PLANES));
  SVS_HIP(ctx, s->d_tables.alloc(1));
  SVS_HIP(ctx, s->d_cand.alloc(B * s->cap));
  SVS_HIP(ctx, s->d_count.alloc(B));
  SVS_HIP(ctx, s->d_ocount.alloc(B));
  SVS_HIP(ctx, s->d_sorted.alloc(rows));
  SVS_HIP(ctx, s->d_okp.alloc(rows));
  SVS_HIP(ctx, s->d_keep.alloc(rows));
  SVS_HIP(ctx, s->d_dir.alloc(rows));
  SVS_HIP(ctx, s->d_uvu.alloc(rows * 3));
  SVS_HIP(ctx, s->d_ouvu.alloc(rows * 3));
  SVS_HIP(ctx, s->d_desc.alloc(rows * 64));
  SVS_HIP(ctx, s->d_odesc.alloc(rows * 64));
  SVS_HIP(ctx, s->h_count.alloc(2 * B));
  for (auto &e : s->ev) SVS_HIP(ctx, e.create());
  return SVS_OK;
}

extern "C" int svs_surf_create(svs_ctx *ctx, const svs_cam *cam, int w, int h, int max_batch, int max_keypoints, const svs_surf_params *prm, svs_surf **out) {
  SVS_REQUIRE(ctx, ctx && cam && prm && out && w >= 1 && h >= 1 && max_batch >= 1 && max_keypoints >= 1 && max_keypoints <= (1 << 20));
  SVS_REQUIRE(ctx, (cam->w <= 0 || cam->w == w) && (cam->h <= 0 || cam->h == h));
  SURF_REFUSE(ctx, (long long)w * h * 255 < (1ll << 31), SVS_ERR_CAPACITY);
  SURF_REFUSE(ctx, prm->n_octaves >= 1 && prm->n_octaves <= 4 && prm->n_octave_layers >= 1 && prm->n_octave_layers <= 4, SVS_ERR_UNSUPPORTED);
  const int largest = (9 + 6 * (prm->n_octave_layers + 1)) << (prm->n_octaves - 1);
  SURF_REFUSE(ctx, w >= largest && h >= largest, SVS_ERR_UNSUPPORTED);
  const int max_win = surf_window_size((float)largest);      // the refinement returns at most the largest layer's size
  const size_t lds = SURF_LDS_TABLES + 256 + ((surf_desc_work_bytes(max_win) + 15) & ~(size_t)15);
  SURF_REFUSE(ctx, lds <= 64 * 1024, SVS_ERR_UNSUPPORTED);
  SVS_DEVICE(ctx);
  std::unique_ptr<svs_surf> s(new svs_surf());
  s->ctx = ctx; s->prm = *prm; s->max_batch = max_batch; s->max_kp = max_keypoints; s->max_win = max_win; s->lds = lds;
  s->cap = std::max(2 * max_keypoints, 1024);
  surf_plane planes[SURF_MAX_PLANES] = {};
  surf_dims &dm = s->dm;
  dm.w = w; dm.h = h; dm.n_octaves = prm->n_octaves; dm.n_layers = prm->n_octave_layers;
  dm.n_planes = surf_make_planes(w, h, prm->n_octaves, prm->n_octave_layers, planes, &dm.total_samples, &dm.plane_elems);
  dm.integral_elems = (int64_t)(w + 1) * (h + 1);
  dm.total_mid = 0;
  for (int o = 0; o < dm.n_octaves; ++o) dm.total_mid += planes[o * (dm.n_layers + 2)].rows * planes[o * (dm.n_layers + 2)].cols * dm.n_layers;
  s->n_out.reset(new int32_t[max_batch]());
  if (int rc = surf_alloc(s.get())) return rc;
  surf_tables tb;
  surf_make_tables(&tb);
  SVS_HIP(ctx, hipMemcpyAsync(s->d_planes, planes, sizeof planes, hipMemcpyHostToDevice, ctx->stream));
  SVS_HIP(ctx, hipMemcpyAsync(s->d_tables, &tb, sizeof tb, hipMemcpyHostToDevice, ctx->stream));
  SVS_HIP(ctx, hipStreamSynchronize(ctx->stream));      // the host copies above are locals
  *out = s.release();
  return SVS_OK;
}

extern "C" int svs_surf_set_timing(svs_surf *s, int on) {
  if (!s) return SVS_ERR_INVALID;
  s->timing = on ? 1 : 0;
  return SVS_OK;
}
extern "C" int svs_surf_stage_times(svs_surf *s, float *ms) {
  if (!s || !ms) return SVS_ERR_INVALID;
  for (int i = 0; i < SVS_SURF_STAGES; ++i) ms[i] = s->stage_ms[i];
  return SVS_OK;
}

extern "C" int svs_surf_extract(svs_surf *s, const uint8_t *d_img, int stride, size_t bstride, const float *d_disp, int dstride, size_t d_bstride, int n_batch,
                                int32_t *h_count, int32_t *h_overflow, svs_surf_keypoint *h_kp, double *h_uvu, float *h_desc) {
  svs_ctx *ctx = s ? s->ctx : nullptr;
  SVS_REQUIRE(ctx, s && d_img && n_batch >= 1);
  SVS_REQUIRE(ctx, s->d_cand.get() && s->cap >= 1);
  SURF_REFUSE(ctx, n_batch <= s->max_batch, SVS_ERR_CAPACITY);
  const surf_dims dm = s->dm;
  SVS_REQUIRE(ctx, stride >= dm.w && (n_batch == 1 || bstride >= (size_t)stride * (dm.h - 1) + dm.w));
  SVS_REQUIRE(ctx, d_disp || !s->prm.require_disparity);
  if (d_disp) SVS_REQUIRE(ctx, dstride >= dm.w && (n_batch == 1 || d_bstride >= (size_t)dstride * (dm.h - 1) + dm.w));
  SVS_DEVICE(ctx);
  hipStream_t st = ctx->stream;
  const unsigned B = (unsigned)n_batch;
  const int T = s->timing;
  s->n_last = 0;
  // 1. integral
  if (T) SVS_HIP(ctx, hipEventRecord(s->ev[0], st));
  hipLaunchKernelGGL(surf_integral_rows_kernel, dim3(dm.h + 1, B), dim3(64), 0, st, d_img, stride, bstride, dm.w, s->d_S.get(), dm.integral_elems);
  SVS_LAUNCH_CHECK(ctx);
  hipLaunchKernelGGL(surf_integral_cols_kernel, dim3(div_up(dm.w + 1, 256), B), dim3(256), 0, st, dm.w, dm.h, s->d_S.get(), dm.integral_elems);
  SVS_LAUNCH_CHECK(ctx);
  // 2. responses
  if (T) SVS_HIP(ctx, hipEventRecord(s->ev[1], st));
  SVS_HIP(ctx, hipMemsetAsync(s->d_det, 0, (size_t)n_batch * dm.plane_elems * sizeof(float), st));
  SVS_HIP(ctx, hipMemsetAsync(s->d_trace, 0, (size_t)n_batch * dm.plane_elems * sizeof(float), st));
  hipLaunchKernelGGL(surf_response_kernel, dim3(div_up(dm.total_samples, 256), B), dim3(256), 0, st, dm, s->d_planes.get(), s->d_S.get(), s->d_det.get(), s->d_trace.get());
  SVS_LAUNCH_CHECK(ctx);
  // 3. maxima: the list must hold every one of them
  if (T) SVS_HIP(ctx, hipEventRecord(s->ev[2], st));
  int longest = 0;
  for (int attempt = 0; attempt < 2; ++attempt) {
    SVS_HIP(ctx, hipMemsetAsync(s->d_count, 0, (size_t)n_batch * sizeof(int32_t), st));
    hipLaunchKernelGGL(surf_maxima_kernel, dim3(div_up(dm.total_mid, 256), B), dim3(256), 0, st, dm, s->d_planes.get(), s->d_det.get(), s->d_trace.get(),
                       s->prm.hessian_threshold, s->d_cand.get(), s->cap, s->d_count.get());
    SVS_LAUNCH_CHECK(ctx);
    SVS_HIP(ctx, hipMemcpyAsync(s->h_count, s->d_count, (size_t)n_batch * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    SVS_HIP(ctx, hipStreamSynchronize(st));
    longest = 0;
    for (int b = 0; b < n_batch; ++b) longest = std::max(longest, (int)s->h_count[b]);
    if (longest <= s->cap) break;
    SVS_REQUIRE(ctx, attempt == 0);      // (never: the count does not depend on the capacity)
    DevBuf<surf_cand> grown;                                   // into a block of its own: a failed allocation leaves the handle as it was
    SVS_HIP(ctx, grown.alloc((size_t)s->max_batch * longest));
    s->d_cand = std::move(grown);
    s->cap = longest;
  }
  if (T) SVS_HIP(ctx, hipEventRecord(s->ev[3], st));
  const int max_kp = s->max_kp, n_sorted = std::min(longest, max_kp);
  if (longest > 0) {
    // 4. order
    hipLaunchKernelGGL(surf_order_kernel, dim3(div_up(longest, 256), B), dim3(256), 0, st, s->d_cand.get(), s->cap, s->d_count.get(), max_kp, s->d_sorted.get());
    SVS_LAUNCH_CHECK(ctx);
    if (T) SVS_HIP(ctx, hipEventRecord(s->ev[4], st));
    // 5. orientation and descriptor
    hipLaunchKernelGGL(surf_orient_kernel, dim3(n_sorted, B), dim3(64), 0, st, dm, s->d_tables.get(), s->d_S.get(), d_disp, dstride, d_bstride, s->d_count.get(), max_kp,
                       s->d_sorted.get(), s->d_uvu.get(), s->d_dir.get(), s->d_keep.get());
    SVS_LAUNCH_CHECK(ctx);
    hipLaunchKernelGGL(surf_describe_kernel, dim3(n_sorted, B), dim3(256), s->lds, st, dm, s->d_tables.get(), d_img, stride, bstride, s->d_count.get(), max_kp,
                       s->d_sorted.get(), s->d_dir.get(), s->d_keep.get(), s->max_win, s->d_desc.get());
    SVS_LAUNCH_CHECK(ctx);
  } else if (T) SVS_HIP(ctx, hipEventRecord(s->ev[4], st));
  // 6. compaction (an image without maxima: count 0)
  if (T) SVS_HIP(ctx, hipEventRecord(s->ev[5], st));
  hipLaunchKernelGGL(surf_compact_kernel, dim3(B), dim3(256), 0, st, s->d_count.get(), max_kp, s->d_sorted.get(), s->d_uvu.get(), s->d_desc.get(), s->d_keep.get(),
                     s->d_okp.get(), s->d_ouvu.get(), s->d_odesc.get(), s->d_ocount.get());
  SVS_LAUNCH_CHECK(ctx);
  if (T) SVS_HIP(ctx, hipEventRecord(s->ev[6], st));
  SVS_HIP(ctx, hipMemcpyAsync(s->h_count + s->max_batch, s->d_ocount, (size_t)n_batch * sizeof(int32_t), hipMemcpyDeviceToHost, st));
  SVS_HIP(ctx, hipStreamSynchronize(st));
  for (int b = 0; b < n_batch; ++b) {
    const int n = s->h_count[s->max_batch + b];
    const size_t row0 = (size_t)b * max_kp;
    s->n_out[b] = n;
    if (h_count) h_count[b] = n;
    if (h_overflow) h_overflow[b] = s->h_count[b] > max_kp ? 1 : 0;
    if (n > 0 && h_kp) SVS_HIP(ctx, hipMemcpyAsync(h_kp + row0, s->d_okp + row0, (size_t)n * sizeof(svs_surf_keypoint), hipMemcpyDeviceToHost, st));
    if (n > 0 && h_uvu) SVS_HIP(ctx, hipMemcpyAsync(h_uvu + row0 * 3, s->d_ouvu + row0 * 3, (size_t)n * 3 * sizeof(double), hipMemcpyDeviceToHost, st));
    if (n > 0 && h_desc) SVS_HIP(ctx, hipMemcpyAsync(h_desc + row0 * 64, s->d_odesc + row0 * 64, (size_t)n * 64 * sizeof(float), hipMemcpyDeviceToHost, st));
  }
  SVS_HIP(ctx, hipStreamSynchronize(st));
  if (T)
    for (int i = 0; i < SVS_SURF_STAGES; ++i) SVS_HIP(ctx, hipEventElapsedTime(&s->stage_ms[i], s->ev[i], s->ev[i + 1]));
  s->n_last = n_batch; s->last_had_disp = d_disp ? 1 : 0;
  return SVS_OK;
}

extern "C" int svs_loop_set_place_from_surf(svs_loop *l, int slot, svs_surf *s, int image_index) {
  svs_ctx *ctx = svs_loop_ctx(l);
  SVS_REQUIRE(ctx, l && s && s->ctx == ctx && image_index >= 0 && image_index < s->n_last);
  SVS_REQUIRE(ctx, s->last_had_disp);      // without a disparity uvu[0] - uvu[2] = 0, which svs_loop_set_place refuses
  const size_t row0 = (size_t)image_index * s->max_kp;
  return svs_loop_set_place_dev(l, slot, s->n_out[image_index], s->d_odesc + row0 * 64, s->d_ouvu + row0 * 3);
}

#else      // SVS_NO_SURF: the exports remain, nothing is built
struct svs_surf;
extern "C" void svs_surf_params_default(svs_surf_params *p) {
  if (!p) return;
  p->hessian_threshold = 600.f; p->n_octaves = 2; p->n_octave_layers = 2; p->require_disparity = 1;
}
static int surf_not_built(svs_ctx *ctx) {
  if (ctx) ctx->err = "SURF was left out of this build (make SURF=0)";
  return SVS_ERR_UNSUPPORTED;
}
extern "C" int svs_surf_create(svs_ctx *ctx, const svs_cam *, int, int, int, int, const svs_surf_params *, svs_surf **) { return surf_not_built(ctx); }
extern "C" int svs_surf_destroy(svs_surf *) { return SVS_ERR_UNSUPPORTED; }
extern "C" int svs_surf_extract(svs_surf *, const uint8_t *, int, size_t, const float *, int, size_t, int, int32_t *, int32_t *, svs_surf_keypoint *, double *, float *) {
  return SVS_ERR_UNSUPPORTED;
}
extern "C" int svs_loop_set_place_from_surf(svs_loop *l, int, svs_surf *, int) { return surf_not_built(svs_loop_ctx(l)); }
extern "C" int svs_surf_set_timing(svs_surf *, int) { return SVS_ERR_UNSUPPORTED; }
extern "C" int svs_surf_stage_times(svs_surf *, float *) { return SVS_ERR_UNSUPPORTED; }
#endif
