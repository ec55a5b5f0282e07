// map_csr.inc -- the two CSR views of the observation log (by keyframe: a feature_table; by point: an observer row, sorted by keyframe id), rebuilt by a
// counting sort when the log has grown; included by map.hip.
namespace {
// ---- the CSR rebuild -----------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void map_count_kernel(MapK M) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  const bool active = e < M.n_log;
  const int2 o = active ? M.log[e] : make_int2(0, 0);      // (point, keyframe): ids the host has checked
  if (active) atomicAdd(&M.pt_begin[o.x], 1);              // a point is in a wave once, but for pairs of different feature_tables
  (void)wave_add_by_key(M.kf_begin, o.y, active);
}

// workgroup 0: keyframes, workgroup 1: points.  Eight entries per lane and step: the single workgroup's chain of barriers is n / 4096 steps long, and the scan is
// on the path of every walk after the log has grown
__global__ __launch_bounds__(MB_THREADS) void map_scan_kernel(MapK M) {
  __shared__ int s_w[MB_THREADS / 64];
  const bool kf = blockIdx.x == 0;
  counts_to_begin<8>(kf ? M.kf_begin : M.pt_begin, kf ? M.kf_cur : M.pt_cur, kf ? M.kf_hi : M.pt_hi, s_w);
}

// the position inside a row is whatever the atomics give: rows by keyframe are read as sets, rows by point are sorted by the next kernel
__global__ __launch_bounds__(256) void map_fill_kernel(MapK M) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  const bool active = e < M.n_log;
  const int2 o = active ? M.log[e] : make_int2(0, 0);
  if (active) M.pt_rows[atomicAdd(&M.pt_cur[o.x], 1)] = o.y;      // < begin of the next row <= n_log
  const int slot = wave_add_by_key(M.kf_cur, o.y, active);
  if (active) M.kf_rows[slot] = o.x;
}

// one lane per point: its observer row ascending (rows are a handful of keyframes long: insertion sort; pairs are distinct)
__global__ __launch_bounds__(256) void map_sort_rows_kernel(MapK M) {
  const int p = blockIdx.x * 256 + threadIdx.x;
  if (p >= M.pt_hi) return;
  const int b = M.pt_begin[p], e = M.pt_begin[p + 1];
  for (int i = b + 1; i < e; ++i) {
    const int v = M.pt_rows[i];
    int j = i - 1;
    while (j >= b && M.pt_rows[j] > v) { M.pt_rows[j + 1] = M.pt_rows[j]; --j; }
    M.pt_rows[j + 1] = v;
  }
}
}  // namespace

// what every walk needs before its launch: a row of the point bitmap per request, and CSR views of the whole log
static int map_prepare_walk(svs_map *m, int n_requests) {
  svs_ctx *ctx = m->ctx;
  if (m->mark_rows < n_requests) {      // grow-only; a new block needs the stream drained of the walks that read the old one
    SVS_HIP(ctx, hipStreamSynchronize(ctx->stream));
    SVS_HIP(ctx, m->d_mark.alloc((size_t)n_requests * m->mark_b));
    m->mark_rows = n_requests;
  }
  if (m->csr_n != m->n_obs) {
    const MapK M = m->view();
    SVS_HIP(ctx, hipMemsetAsync(m->d_kf_begin, 0, ((size_t)m->kf_hi + 1) * sizeof(int32_t), ctx->stream));
    SVS_HIP(ctx, hipMemsetAsync(m->d_pt_begin, 0, ((size_t)m->pt_hi + 1) * sizeof(int32_t), ctx->stream));
    hipLaunchKernelGGL(map_count_kernel, dim3(div_up(m->n_obs, 256)), dim3(256), 0, ctx->stream, M);
    hipLaunchKernelGGL(map_scan_kernel, dim3(2), dim3(MB_THREADS), 0, ctx->stream, M);
    hipLaunchKernelGGL(map_fill_kernel, dim3(div_up(m->n_obs, 256)), dim3(256), 0, ctx->stream, M);
    hipLaunchKernelGGL(map_sort_rows_kernel, dim3(div_up(m->pt_hi, 256)), dim3(256), 0, ctx->stream, M);
    SVS_LAUNCH_CHECK(ctx);
    m->csr_n = m->n_obs;
  }
  return SVS_OK;
}

// kf_map.h: the observer rows for the keyframe decision's membership tests (keyframe.hip), current with the log
int svs_map_observer_view(svs_map *m, MapObsView *out) {
  if (int rc = map_prepare_walk(m, 0)) return rc;
  out->pt_begin = m->d_pt_begin; out->pt_rows = m->d_pt_rows; out->pt_hi = m->pt_hi;
  return SVS_OK;
}
