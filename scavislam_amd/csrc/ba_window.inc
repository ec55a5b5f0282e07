// ba_window.inc -- part of ba.hip (one translation unit): the persistent window (svs_ba_window_update / _reset / _forget_keyframes): observation store on
// the device, edge order / slots / co-visibility pattern assembled by kernels.
// ---- persistent window (SURVEY.md 8f rank 4) ----------------------------------------------------------------------------
// The reference rebuilds a whole optimizer from its graph for every optimize() (slam_graph.cpp:324, copyDataToG2o :983-1032), and
// svs_ba_set_problem mirrors that: all edge records cross PCIe and are re-ordered on every call although the window changes by about
// one keyframe.  Here the library KEEPS every observation it has been given (device-resident, 64 B each, ids of point and keyframe as
// the reference's graph names them) and a call only brings what is new: the window's poses and point values (they are the caller's
// state), the ids that define the window, the observations made since the last call, and the few hundred pose-pose constraints.
// The edge list of the window is then assembled ON THE DEVICE:
//   id -> window-index tables (direct addressed)  ->  filter the store (observation is in the window iff its point and its keyframe
//   are)  ->  slot order (wide | anchor | point | pose) WITHOUT a sort: pose masks per landmark + a counting sort of the landmarks by (wide, anchor)
//   (hand-written, five launches: see the kernels below)  ->  co-visibility pattern;
// one small read-back (landmark lengths + pattern) lets the host pack landmarks into wave chunks and build the block envelope exactly
// as svs_ba_set_problem does.  Host work per call is O(points + new observations), PCIe traffic likewise.
namespace {
struct WinCounters { int n_edges, n_lm, dup, pad; };
__global__ void win_scatter_kernel(const int *__restrict__ ids, int n, int *__restrict__ tab) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) tab[ids[i]] = i;
}
// Everything a call brings arrives as ONE block (one pinned staging area, one DMA): ids, anchors, poses, points, the new observations, the constraints.  This kernel
// puts the pieces where the optimizer keeps them (both copies of the state, the store's tail, the constraint list), clears x and fills the id -> index tables.
struct WinIn {
  const int *pids, *lids; const double *poses, *psi, *obs, *cons;
  int P, L; size_t obs_words, cons_words;
  double *poses0, *poses1, *psi0, *psi1, *store_tail, *d_cons, *d_x;
  int *pose_tab, *point_tab;
};
__global__ void win_unpack_kernel(WinIn A) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < 12 * (size_t)A.P) { const double v = A.poses[i]; A.poses0[i] = v; A.poses1[i] = v; }
  if (i < 3 * (size_t)A.L) { const double v = A.psi[i]; A.psi0[i] = v; A.psi1[i] = v; }
  if (i < A.obs_words) A.store_tail[i] = A.obs[i];
  if (i < A.cons_words) A.d_cons[i] = A.cons[i];
  if (i < 6 * (size_t)A.P) A.d_x[i] = 0.0;
  if (i < (size_t)A.P) A.pose_tab[A.pids[i]] = (int)i;
  if (i < (size_t)A.L) A.point_tab[A.lids[i]] = (int)i;
}
__global__ void win_clear_kernel(int *__restrict__ a, size_t na, int *__restrict__ b, size_t nb, int *__restrict__ z, size_t nz) {
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < na; i += stride) a[i] = -1;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < nb; i += stride) b[i] = -1;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < nz; i += stride) z[i] = 0;
}
__global__ void win_anchor_kernel(const int *__restrict__ anchor_ids, int n, const int *__restrict__ pose_tab, int *__restrict__ anchor_idx) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) anchor_idx[i] = pose_tab[anchor_ids[i]];
}
// ---- the window's edge list WITHOUT a sort (round 4; rounds 2-3 sorted 64-bit keys with hipCUB: ~9 library launches) --------------------------------------
// The slot order the Schur kernels want is (wide | anchor | point | pose).  Nothing in it needs a comparison sort:
//   * pose inside a landmark: a window has <= 256 poses, so the poses that observe a landmark are a 256-bit mask (win_mark_kernel sets the bits with
//     atomicOr; a bit that was already set is "two observations of one point in one keyframe") and an observation's place inside its landmark is the
//     number of set bits below its own;
//   * landmark order: a landmark's bucket is (wide, anchor) -- at most 2 P <= 512 buckets -- and inside a bucket the point index ascends, i.e. the order is
//     a stable counting sort of the landmark indices by bucket.  Tiles of 1024 consecutive landmarks count their buckets (landmarks and observations:
//     win_tile_hist_kernel), one workgroup turns the counts into bases per (tile, bucket) (win_col_scan_kernel), and every tile ranks its landmarks inside
//     the buckets wave by wave (win_tile_rank_kernel): that gives each landmark its position in the order AND the offset of its first edge;
//   * win_place_kernel then copies every observation of the store straight to its slot.
// Five launches, no key arrays, the store is read twice (16 + 64 bytes per observation).  The co-visibility pattern comes from the masks.
constexpr int WIN_TILE = 1024;
__device__ __forceinline__ bool win_lookup(const svs_ba_edge *__restrict__ store, size_t r, const int *__restrict__ pose_tab, size_t pose_tab_n,
                                           const int *__restrict__ point_tab, size_t point_tab_n, const int *__restrict__ anchor_idx, int &li, int &pi, int &ai) {
  const int4 ids = *reinterpret_cast<const int4 *>(reinterpret_cast<const char *>(store + r) + 48);      // point, pose, anchor, pad (include/scavislam_hip.h: svs_ba_edge)
  if ((size_t)ids.x >= point_tab_n || (size_t)ids.y >= pose_tab_n) return false;
  li = point_tab[ids.x]; pi = pose_tab[ids.y];
  if (li < 0 || pi < 0) return false;
  ai = anchor_idx[li];
  return ai >= 0;
}
__global__ void win_mark_kernel(const svs_ba_edge *__restrict__ store, size_t n, const int *__restrict__ pose_tab, size_t pose_tab_n,
                                const int *__restrict__ point_tab, size_t point_tab_n, const int *__restrict__ anchor_idx,
                                int *__restrict__ count, unsigned long long *__restrict__ mask, WinCounters *__restrict__ ctr) {
  const size_t r = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= n) return;
  int li, pi, ai;
  if (!win_lookup(store, r, pose_tab, pose_tab_n, point_tab, point_tab_n, anchor_idx, li, pi, ai)) return;
  atomicAdd(&count[li], 1);
  const unsigned long long bit = 1ull << (pi & 63);
  if (atomicOr(&mask[(size_t)li * 4 + (pi >> 6)], bit) & bit) ctr->dup = 1;      // two observations of one point in one keyframe
}
__device__ __forceinline__ int win_bucket(int cnt, int anchor, int P) { return cnt > 0 ? (cnt > 64 ? P : 0) + anchor : -1; }      // wide landmarks behind the others
__global__ __launch_bounds__(256) void win_tile_hist_kernel(const int *__restrict__ count, const int *__restrict__ anchor_idx, int L, int P, int *__restrict__ tile_tab) {
  __shared__ int s_n[512], s_e[512];
  const int NB = 2 * P, tile = blockIdx.x;
  for (int b = threadIdx.x; b < NB; b += 256) { s_n[b] = 0; s_e[b] = 0; }
  __syncthreads();
  for (int t = threadIdx.x; t < WIN_TILE; t += 256) {
    const int li = tile * WIN_TILE + t;
    if (li < L) { const int c = count[li], b = win_bucket(c, anchor_idx[li], P); if (b >= 0) { atomicAdd(&s_n[b], 1); atomicAdd(&s_e[b], c); } }
  }
  __syncthreads();
  for (int b = threadIdx.x; b < NB; b += 256) { tile_tab[((size_t)tile * NB + b) * 2] = s_n[b]; tile_tab[((size_t)tile * NB + b) * 2 + 1] = s_e[b]; }
}
// one workgroup: thread b owns bucket b's column of the (tile, bucket) table -- exclusive scan down the tiles, then the buckets' totals across
__global__ __launch_bounds__(512) void win_col_scan_kernel(int *__restrict__ tile_tab, int n_tiles, int P, WinCounters *__restrict__ ctr) {
  __shared__ int s_tn[512], s_te[512];
  const int NB = 2 * P, b = threadIdx.x;
  int rn = 0, re = 0;
  if (b < NB)
    for (int t = 0; t < n_tiles; ++t) {
      int *q = tile_tab + ((size_t)t * NB + b) * 2;
      const int cn = q[0], ce = q[1];
      q[0] = rn; q[1] = re;
      rn += cn; re += ce;
    }
  s_tn[b] = b < NB ? rn : 0; s_te[b] = b < NB ? re : 0;
  __syncthreads();
  if (b == 0) {      // (<= 512 values)
    int an = 0, ae = 0;
    for (int k = 0; k < NB; ++k) { const int cn = s_tn[k], ce = s_te[k]; s_tn[k] = an; s_te[k] = ae; an += cn; ae += ce; }
    ctr->n_lm = an; ctr->n_edges = ae;
  }
  __syncthreads();
  if (b < NB) {
    const int bn = s_tn[b], be = s_te[b];
    for (int t = 0; t < n_tiles; ++t) { int *q = tile_tab + ((size_t)t * NB + b) * 2; q[0] += bn; q[1] += be; }
  }
}
__global__ __launch_bounds__(WIN_TILE) void win_tile_rank_kernel(const int *__restrict__ count, const int *__restrict__ anchor_idx, const unsigned long long *__restrict__ mask,
                                                                 int L, int P, const int *__restrict__ tile_tab, const WinCounters *__restrict__ ctr,
                                                                 int *__restrict__ edge_off, int *__restrict__ lm_start, int *__restrict__ lm_len,
                                                                 unsigned char *__restrict__ pat) {
  __shared__ int s_n[512], s_e[512];
  __shared__ unsigned s_pat[2048];               // the tile's share of the P x P pattern, one bit per entry (P <= 256)
  const int NB = 2 * P, tile = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  for (int b = tid; b < NB; b += WIN_TILE) { s_n[b] = tile_tab[((size_t)tile * NB + b) * 2]; s_e[b] = tile_tab[((size_t)tile * NB + b) * 2 + 1]; }
  const int pat_words = (P * P + 31) >> 5;
  for (int k = tid; k < pat_words; k += WIN_TILE) s_pat[k] = 0u;
  const int li = tile * WIN_TILE + tid;
  const int c = li < L ? count[li] : 0, anc = li < L ? anchor_idx[li] : -1;
  const int b = win_bucket(c, anc, P);
  // rank inside the own wave (all waves at once): landmarks of the same bucket on lower lanes
  int rn = 0, re = 0;
  bool last = true;
  for (int j = 0; j < 64; ++j) {
    const int bj = __shfl(b, j, 64), cj = __shfl(c, j, 64);
    if (bj == b) { if (j < lane) { ++rn; re += cj; } else if (j > lane) last = false; }
  }
  int my_rank = -1, my_off = -1;
  __syncthreads();
  // co-visibility pattern as marshalling leaves it (ba.hip: every pose's farthest partners): lo = first, hi = last pose of the landmark incl. its anchor.
  // Collected in LDS bits: 20 k landmarks writing ~13 bytes each into the 2.5 KB global array serialised on its 40 cache lines (100 us per call).
  if (b >= 0) {
    unsigned long long m[4];
    for (int k = 0; k < 4; ++k) m[k] = mask[(size_t)li * 4 + k];
    int p_first = -1, p_last = -1;
    for (int k = 0; k < 4; ++k) if (m[k]) { if (p_first < 0) p_first = 64 * k + __builtin_ctzll(m[k]); p_last = 64 * k + 63 - __builtin_clzll(m[k]); }
    const int lo = min(p_first, anc), hi = max(p_last, anc);
    auto set_bit = [&](int r, int q) { const int i = r * P + q; atomicOr(&s_pat[i >> 5], 1u << (i & 31)); };
    for (int k = 0; k < 4; ++k)
      for (unsigned long long mm = m[k]; mm; mm &= mm - 1) { const int p = 64 * k + __builtin_ctzll(mm); set_bit(p, hi); set_bit(lo, p); }
    set_bit(anc, hi); set_bit(lo, hi); set_bit(lo, anc);
  }
  for (int w = 0; w < WIN_TILE / 64; ++w) {      // the waves of a tile in index order: a wave ranks its landmarks behind what the earlier ones left in LDS
    if (wave == w && b >= 0) {
      const int base_n = s_n[b], base_e = s_e[b];      // (every lane reads before any lane of this wave writes: program order inside a wave)
      my_rank = base_n + rn; my_off = base_e + re;
      if (last) { s_n[b] = my_rank + 1; s_e[b] = my_off + c; }
    }
    __syncthreads();
  }
  for (int k = tid; k < pat_words; k += WIN_TILE)
    for (unsigned bits = s_pat[k]; bits; bits &= bits - 1) pat[32 * k + __builtin_ctz(bits)] = 1;
  if (tile == 0 && tid == 0) lm_start[ctr->n_lm] = ctr->n_edges;
  if (b < 0) return;
  edge_off[li] = my_off;
  lm_start[my_rank] = my_off;
  lm_len[my_rank] = c;
}
__global__ void win_place_kernel(const svs_ba_edge *__restrict__ store, size_t n, const int *__restrict__ pose_tab, size_t pose_tab_n,
                                 const int *__restrict__ point_tab, size_t point_tab_n, const int *__restrict__ anchor_idx, const int *__restrict__ edge_off,
                                 const unsigned long long *__restrict__ mask, svs_ba_edge *__restrict__ edges) {
  const size_t r = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= n) return;
  int li, pi, ai;
  if (!win_lookup(store, r, pose_tab, pose_tab_n, point_tab, point_tab_n, anchor_idx, li, pi, ai)) return;
  int below = 0;
  for (int k = 0; k < (pi >> 6); ++k) below += __builtin_popcountll(mask[(size_t)li * 4 + k]);
  below += __builtin_popcountll(mask[(size_t)li * 4 + (pi >> 6)] & ((1ull << (pi & 63)) - 1ull));
  svs_ba_edge e = store[r];
  e.point = li; e.pose = pi; e.anchor = ai;
  edges[(size_t)edge_off[li] + below] = e;
}
// ---- order-preserving compaction of the store (svs_ba_window_forget_keyframes): tiles of 1024 records count their survivors, one workgroup scans the tile
// counts, every tile then moves its survivors behind those of the tiles before it
__device__ __forceinline__ bool win_forgotten(int pose_id, const int *__restrict__ sorted_ids, int n_ids) {
  int lo = 0, hi = n_ids;
  while (lo < hi) { const int mid = (lo + hi) >> 1; if (sorted_ids[mid] < pose_id) lo = mid + 1; else hi = mid; }
  return lo < n_ids && sorted_ids[lo] == pose_id;
}
__global__ __launch_bounds__(WIN_TILE) void win_keep_count_kernel(const svs_ba_edge *__restrict__ store, size_t n, const int *__restrict__ sorted_ids, int n_ids,
                                                                  int *__restrict__ tile_count) {
  __shared__ int s_cnt;
  if (threadIdx.x == 0) s_cnt = 0;
  __syncthreads();
  const size_t r = (size_t)blockIdx.x * WIN_TILE + threadIdx.x;
  const bool keep = r < n && !win_forgotten(store[r].pose, sorted_ids, n_ids);
  const int k = __builtin_popcountll(__ballot(keep));
  if ((threadIdx.x & 63) == 0 && k) atomicAdd(&s_cnt, k);
  __syncthreads();
  if (threadIdx.x == 0) tile_count[blockIdx.x] = s_cnt;
}
__global__ __launch_bounds__(1024) void win_scan_tiles_kernel(int *__restrict__ tile_count, int n_tiles, int *__restrict__ total) {      // one workgroup, exclusive, in place
  __shared__ int s_part[1024];
  const int tid = threadIdx.x, per = (n_tiles + 1023) / 1024, a = tid * per, b = min(n_tiles, a + per);
  int sum = 0;
  for (int i = a; i < b; ++i) sum += tile_count[i];
  s_part[tid] = sum;
  __syncthreads();
  if (tid == 0) { int acc = 0; for (int i = 0; i < 1024; ++i) { const int v = s_part[i]; s_part[i] = acc; acc += v; } *total = acc; }
  __syncthreads();
  int run = s_part[tid];
  for (int i = a; i < b; ++i) { const int v = tile_count[i]; tile_count[i] = run; run += v; }
}
__global__ __launch_bounds__(WIN_TILE) void win_keep_move_kernel(const svs_ba_edge *__restrict__ store, size_t n, const int *__restrict__ sorted_ids, int n_ids,
                                                                 const int *__restrict__ tile_base, svs_ba_edge *__restrict__ out) {
  __shared__ int s_wave[WIN_TILE / 64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const size_t r = (size_t)blockIdx.x * WIN_TILE + tid;
  const bool keep = r < n && !win_forgotten(store[r].pose, sorted_ids, n_ids);
  const unsigned long long bal = __ballot(keep);
  if (lane == 0) s_wave[wave] = __builtin_popcountll(bal);
  __syncthreads();
  int base = tile_base[blockIdx.x];
  for (int w = 0; w < wave; ++w) base += s_wave[w];
  if (keep) out[(size_t)base + __builtin_popcountll(bal & ((1ull << lane) - 1ull))] = store[r];
}
}  // namespace

// where a window's definition lies on the device, and the store its edges are filtered from
struct WinSrc {
  const int *pids, *lids, *aids; const double *poses, *psi, *obs, *cons;
  int n_new; svs_ba_edge *store_tail;      // the new observations (staged at `obs`) and where they join the store; none: 0
  const svs_ba_edge *store; size_t N;
  int max_pose_id, max_point_id;           // the id -> index tables hold at least these ids (the store's records are range-checked against the tables)
};
static int window_assemble(svs_ba *ba, int P, int L, int C, const WinSrc &S, const svs_cam *cam, const svs_ba_params *prm,
                           std::chrono::steady_clock::time_point t_0, std::chrono::steady_clock::time_point t_s);

extern "C" int svs_ba_window_reset(svs_ba *ba) {
  if (!ba) return SVS_ERR_INVALID;
  ba->w_n = 0;
  ba->problem_valid = false;
  return SVS_OK;
}

static int window_update_impl(svs_ba *ba, int P, const int32_t *h_pose_ids, const double *h_poses, int L, const int32_t *h_point_ids,
                              const double *h_psi, const int32_t *h_anchor_pose_ids, int n_new, const svs_ba_edge *h_new_obs, int C,
                              const svs_ba_constraint *h_cons, const svs_cam *cam, const svs_ba_params *prm, bool obs_checked);
// The new observations are appended to the store first and everything else is validated after that (duplicates, landmarks with more than 256
// observations, constraints on poses outside the window, allocation failures): a call that fails must leave the store as it found it, or a
// retry with the same observations would duplicate them and every later call would fail on "two observations of one point in one keyframe".
extern "C" int svs_ba_window_update(svs_ba *ba, int P, const int32_t *h_pose_ids, const double *h_poses, int L, const int32_t *h_point_ids,
                                    const double *h_psi, const int32_t *h_anchor_pose_ids, int n_new, const svs_ba_edge *h_new_obs, int C,
                                    const svs_ba_constraint *h_cons, const svs_cam *cam, const svs_ba_params *prm) {
  const size_t n_before = ba ? ba->w_n : 0;
  const int rc = window_update_impl(ba, P, h_pose_ids, h_poses, L, h_point_ids, h_psi, h_anchor_pose_ids, n_new, h_new_obs, C, h_cons, cam, prm, false);
  if (rc && ba) ba->w_n = n_before;      // roll the append back (the records behind w_n are dead storage)
  return rc;
}

/* Drop the stored observations of keyframes that can never enter a window again (marginalised / deleted by the map): the store otherwise only
   grows, and every svs_ba_window_update walks all of it.  Order-preserving compaction on the device (three launches); the ids may be any non-negative
   integers (they are looked up in a sorted list, no table of max(id) entries); the scratch comes from the handle's work arrays. */
extern "C" int svs_ba_window_forget_keyframes(svs_ba *ba, const int32_t *h_pose_ids, int n) {
  svs_ctx *ctx = ba ? ba->ctx : nullptr;
  SVS_REQUIRE(ctx, ba && n >= 0 && (n == 0 || h_pose_ids));
  SVS_DEVICE(ctx);
  if (n == 0 || ba->w_n == 0) return SVS_OK;
  SVS_REQUIRE(ctx, ba->w_n < (size_t)INT_MAX);
  for (int i = 0; i < n; ++i) SVS_REQUIRE(ctx, h_pose_ids[i] >= 0);
  std::vector<int> ids;
  try { ids.assign(h_pose_ids, h_pose_ids + n); } catch (const std::bad_alloc &) { ctx->err = "svs_ba_window_forget_keyframes: out of host memory"; return SVS_ERR_CAPACITY; }
  std::sort(ids.begin(), ids.end());
  ids.erase(std::unique(ids.begin(), ids.end()), ids.end());
  SVS_HIP(ctx, hipStreamSynchronize(ctx->stream));
  const size_t N = ba->w_n, n_tiles = (N + WIN_TILE - 1) / WIN_TILE;
  // scratch: sorted ids | tile counts | total | the compacted records
  size_t off = 0;
  auto take = [&](size_t bytes) { const size_t o = off; off = (off + bytes + 255) & ~(size_t)255; return o; };
  const size_t o_ids = take(sizeof(int) * ids.size()), o_tc = take(sizeof(int) * n_tiles), o_tot = take(sizeof(int)), o_out = take(sizeof(svs_ba_edge) * N);
  if (ba->w_work.reserve(off, off + off / 2) != hipSuccess) { ctx->err = "svs_ba_window_forget_keyframes: out of device memory"; return SVS_ERR_CAPACITY; }
  char *W = static_cast<char *>(ba->w_work.get());
  int *d_ids = (int *)(W + o_ids), *d_tc = (int *)(W + o_tc), *d_tot = (int *)(W + o_tot);
  svs_ba_edge *d_out = (svs_ba_edge *)(W + o_out);
  int num = 0;
  SVS_HIP(ctx, hipMemcpyAsync(d_ids, ids.data(), sizeof(int) * ids.size(), hipMemcpyHostToDevice, ctx->stream));
  hipLaunchKernelGGL(win_keep_count_kernel, dim3((unsigned)n_tiles), dim3(WIN_TILE), 0, ctx->stream, ba->w_store, N, d_ids, (int)ids.size(), d_tc);
  hipLaunchKernelGGL(win_scan_tiles_kernel, dim3(1), dim3(1024), 0, ctx->stream, d_tc, (int)n_tiles, d_tot);
  hipLaunchKernelGGL(win_keep_move_kernel, dim3((unsigned)n_tiles), dim3(WIN_TILE), 0, ctx->stream, ba->w_store, N, d_ids, (int)ids.size(), d_tc, d_out);
  SVS_LAUNCH_CHECK(ctx);
  SVS_HIP(ctx, hipMemcpyAsync(&num, d_tot, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
  SVS_HIP(ctx, hipStreamSynchronize(ctx->stream));
  if (num > 0) SVS_HIP(ctx, hipMemcpyAsync(ba->w_store, d_out, (size_t)num * sizeof(svs_ba_edge), hipMemcpyDeviceToDevice, ctx->stream));
  SVS_HIP(ctx, hipStreamSynchronize(ctx->stream));
  ba->w_n = (size_t)num;
  ba->problem_valid = false;              // the window's edge list referred to the old store: the next svs_ba_window_update rebuilds it
  return SVS_OK;
}

static int window_update_impl(svs_ba *ba, int P, const int32_t *h_pose_ids, const double *h_poses, int L, const int32_t *h_point_ids,
                              const double *h_psi, const int32_t *h_anchor_pose_ids, int n_new, const svs_ba_edge *h_new_obs, int C,
                              const svs_ba_constraint *h_cons, const svs_cam *cam, const svs_ba_params *prm, bool obs_checked) {
  svs_ctx *ctx = ba ? ba->ctx : nullptr;
  SVS_REQUIRE(ctx, ba && h_pose_ids && h_poses && (L == 0 || (h_point_ids && h_psi && h_anchor_pose_ids)) && (n_new == 0 || h_new_obs) && (C == 0 || h_cons) && cam && prm);
  SVS_REQUIRE(ctx, P >= 1 && L >= 0 && n_new >= 0 && C >= 0);
  SVS_REQUIRE(ctx, !ba->comm);                        // single-GPU path (a sharded window goes through svs_ba_set_problem)
  SVS_DEVICE(ctx);
  ba->problem_valid = false; ba->from_map_serial = 0;
  if (P > SOLVE_MAX_P) { ctx->err = "svs_ba: P > 256 poses not supported by the single-workgroup solve yet"; return SVS_ERR_UNSUPPORTED; }
  auto t_0 = std::chrono::steady_clock::now();
  // ---- host: ranges of the ids, constraints by index -------------------------------------------------------------------------
  int max_pose_id = -1, max_point_id = -1;
  for (int i = 0; i < P; ++i) { SVS_REQUIRE(ctx, h_pose_ids[i] >= 0); max_pose_id = std::max(max_pose_id, h_pose_ids[i]); }
  for (int i = 0; i < L; ++i) { SVS_REQUIRE(ctx, h_point_ids[i] >= 0 && h_anchor_pose_ids[i] >= 0); max_point_id = std::max(max_point_id, h_point_ids[i]); max_pose_id = std::max(max_pose_id, h_anchor_pose_ids[i]); }
  // (the observation records are range-checked while they are copied to the staging block below; svs_ba_set_problem has checked its records already --
  //  ids < L, < P -- and skips that)
  SVS_REQUIRE(ctx, L < (1 << 23));
  // the constraints by window index (host: a few hundred constraints x <= 256 poses)
  std::vector<svs_ba_constraint> &cons_idx = ba->w_cons_idx;
  cons_idx.resize((size_t)C);
  for (int c = 0; c < C; ++c) {
    cons_idx[c] = h_cons[c];
    int i1 = -1, i2 = -1;
    for (int i = 0; i < P; ++i) { if (h_pose_ids[i] == h_cons[c].pose1) i1 = i; if (h_pose_ids[i] == h_cons[c].pose2) i2 = i; }
    SVS_REQUIRE(ctx, i1 >= 0 && i2 >= 0);                   // a constraint of this window names two window poses
    cons_idx[c].pose1 = i1; cons_idx[c].pose2 = i2;
  }
  SVS_HIP(ctx, hipStreamSynchronize(ctx->stream));
  ba->h_stage_used = 0;
  // the window's own blocks grow by half: a new block first (the old contents move over where they are still needed), then the old one goes
  auto win_grow = [](auto &b, size_t bytes, size_t keep_bytes = 0) { return b.reserve_keep(bytes, bytes + bytes / 2 + 4096, keep_bytes); };
  // ---- ONE block for everything the call brings: pose ids | point ids | anchor ids | poses | points | new observations | constraints -----------------
  size_t ioff = 0;
  auto itake = [&](size_t bytes) { const size_t o = ioff; ioff = (ioff + bytes + 255) & ~(size_t)255; return o; };
  const size_t i_pids = itake(sizeof(int) * (size_t)P), i_lids = itake(sizeof(int) * (size_t)L), i_aids = itake(sizeof(int) * (size_t)L),
               i_poses = itake(sizeof(double) * 12 * (size_t)P), i_psi = itake(sizeof(double) * 3 * (size_t)L), i_obs = itake(sizeof(svs_ba_edge) * (size_t)n_new),
               i_cons = itake(sizeof(svs_ba_constraint) * (size_t)C);
  { int rc = stage_reserve(ba, ioff + sizeof(int) * (((size_t)ba->w_n + n_new) / 8 + 8 * (size_t)P) + 16384); if (rc) return rc; }
  SVS_HIP(ctx, win_grow(ba->w_in, ioff + 256));
  {
    char *hs = reinterpret_cast<char *>(ba->h_stage.get());
    std::memcpy(hs + i_pids, h_pose_ids, sizeof(int) * (size_t)P);
    if (L) { std::memcpy(hs + i_lids, h_point_ids, sizeof(int) * (size_t)L); std::memcpy(hs + i_aids, h_anchor_pose_ids, sizeof(int) * (size_t)L); }
    std::memcpy(hs + i_poses, h_poses, sizeof(double) * 12 * (size_t)P);
    if (L) std::memcpy(hs + i_psi, h_psi, sizeof(double) * 3 * (size_t)L);
    if (C) std::memcpy(hs + i_cons, cons_idx.data(), sizeof(svs_ba_constraint) * (size_t)C);
    ba->h_stage_used = ioff;
    // everything but the observations leaves now (one copy: the observation slot lies between psi and the constraints and travels in pieces below)
    SVS_HIP(ctx, hipMemcpyAsync(ba->w_in, hs, i_obs, hipMemcpyHostToDevice, ctx->stream));
    if (C) SVS_HIP(ctx, hipMemcpyAsync(static_cast<char *>(ba->w_in.get()) + i_cons, hs + i_cons, ioff - i_cons, hipMemcpyHostToDevice, ctx->stream));
    // the observation records: pieces of ~1 MB, each copied to the pinned block (and range-checked) by the worker pool and sent while the next one is being
    // copied -- one core moves ~10 GB/s, the link 50: a single memcpy of the 4 MB of a 50 KF / 20 k window was half of this call
    if (n_new) {
      const size_t rec = sizeof(svs_ba_edge), per = std::max<size_t>(((size_t)1 << 20) / rec, 1);
      HostPool *pool = (size_t)n_new >= 16384 ? host_pool(ba) : nullptr;
      std::unique_lock<std::mutex> pool_lock;
      if (pool) pool_lock = std::unique_lock<std::mutex>(pool->use_);
      std::atomic<int> bad{0};
      const int T = pool ? pool->size() : 1;
      std::vector<int> mx((size_t)2 * T, -1);
      for (size_t c0 = 0; c0 < (size_t)n_new; c0 += per) {
        const size_t c1 = std::min<size_t>(c0 + per, (size_t)n_new);
        auto body = [&](int t, int n) {
          const size_t a = c0 + (c1 - c0) * (size_t)t / n, b = c0 + (c1 - c0) * (size_t)(t + 1) / n;
          if (!obs_checked) {
            int mp = mx[2 * t], mq = mx[2 * t + 1];
            for (size_t i = a; i < b; ++i) {
              if (h_new_obs[i].point < 0 || h_new_obs[i].pose < 0) { bad.store(1); return; }
              mp = std::max(mp, h_new_obs[i].point); mq = std::max(mq, h_new_obs[i].pose);
            }
            mx[2 * t] = mp; mx[2 * t + 1] = mq;
          }
          std::memcpy(hs + i_obs + a * rec, h_new_obs + a, (b - a) * rec);
        };
        if (pool) pool->run(body); else body(0, 1);
        if (bad.load()) break;
        SVS_HIP(ctx, hipMemcpyAsync(static_cast<char *>(ba->w_in.get()) + i_obs + c0 * rec, hs + i_obs + c0 * rec, (c1 - c0) * rec, hipMemcpyHostToDevice, ctx->stream));
      }
      if (bad.load()) { (void)hipStreamSynchronize(ctx->stream); ba->h_stage_used = 0; ctx->err = "svs_ba_window_update: negative point / pose id in an observation"; return SVS_ERR_INVALID; }
      if (obs_checked) { max_point_id = std::max(max_point_id, L - 1); max_pose_id = std::max(max_pose_id, P - 1); }
      else for (int t = 0; t < T; ++t) { max_point_id = std::max(max_point_id, mx[2 * t]); max_pose_id = std::max(max_pose_id, mx[2 * t + 1]); }
    }
  }
  auto t_s = std::chrono::steady_clock::now();
  // ---- the store grows by the new observations (unpacked into its tail below) --------------------------------------------------------
  const size_t w_n_old = ba->w_n;
  SVS_HIP(ctx, win_grow(ba->w_store, (ba->w_n + (size_t)n_new) * sizeof(svs_ba_edge), ba->w_n * sizeof(svs_ba_edge)));
  ba->w_n += (size_t)n_new;
  SVS_REQUIRE(ctx, ba->w_n < (size_t)INT_MAX - 1);
  char *IN = static_cast<char *>(ba->w_in.get());
  WinSrc S;
  S.pids = (const int *)(IN + i_pids); S.lids = (const int *)(IN + i_lids); S.aids = (const int *)(IN + i_aids);
  S.poses = (const double *)(IN + i_poses); S.psi = (const double *)(IN + i_psi); S.obs = (const double *)(IN + i_obs); S.cons = (const double *)(IN + i_cons);
  S.n_new = n_new; S.store_tail = ba->w_store + w_n_old; S.store = ba->w_store; S.N = ba->w_n;
  S.max_pose_id = max_pose_id; S.max_point_id = max_point_id;
  return window_assemble(ba, P, L, C, S, cam, prm, t_0, t_s);
}

// The second half of every way to bring a window by ids: id -> index tables, the edge list in slot order filtered out of `S.store`, the co-visibility pattern, the one
// read-back, wave chunks and envelope.  ba->w_cons_idx holds the constraints by window index; the stream has been drained and the staging area reset by the caller.
static int window_assemble(svs_ba *ba, int P, int L, int C, const WinSrc &S, const svs_cam *cam, const svs_ba_params *prm,
                           std::chrono::steady_clock::time_point t_0, std::chrono::steady_clock::time_point t_s) {
  svs_ctx *ctx = ba->ctx;
  const std::vector<svs_ba_constraint> &cons_idx = ba->w_cons_idx;
  const size_t N = S.N;
  const int n_new = S.n_new, max_pose_id = S.max_pose_id, max_point_id = S.max_point_id;
  auto win_grow = [](auto &b, size_t bytes, size_t keep_bytes = 0) { return b.reserve_keep(bytes, bytes + bytes / 2 + 4096, keep_bytes); };
  // ---- id tables ---------------------------------------------------------------------------------------------------------------
  SVS_HIP(ctx, win_grow(ba->w_pose_tab, ((size_t)max_pose_id + 1) * sizeof(int)));
  SVS_HIP(ctx, win_grow(ba->w_point_tab, ((size_t)max_point_id + 2) * sizeof(int)));
  const size_t pose_tab_n = ba->w_pose_tab.bytes() / sizeof(int), point_tab_n = ba->w_point_tab.bytes() / sizeof(int);
  // ---- work arrays (one allocation): anchor_idx | [count | masks | pattern | counters: zeroed together] | landmark lengths ([pattern .. lengths]: read back
  //      together) | edge offsets | (tile, bucket) table | lm_start
  const size_t capE = N + 1;
  const size_t n_tiles = ((size_t)std::max(L, 1) + WIN_TILE - 1) / WIN_TILE;
  size_t off = 0;
  auto take = [&](size_t bytes) { const size_t o = off; off = (off + bytes + 255) & ~(size_t)255; return o; };
  const size_t o_aidx = take(sizeof(int) * (size_t)std::max(L, 1)), o_count = take(sizeof(int) * (size_t)std::max(L, 1)), o_mask = take(32 * (size_t)std::max(L, 1)),
               o_pat = take((size_t)P * P), o_ctr = take(sizeof(WinCounters)), o_lml = take(4 * ((size_t)L + 2)),
               o_eoff = take(sizeof(int) * (size_t)std::max(L, 1)), o_tile = take(sizeof(int) * 2 * n_tiles * 2 * (size_t)P), o_lms = take(4 * ((size_t)L + 2));
  SVS_HIP(ctx, win_grow(ba->w_work, off));
  char *W = static_cast<char *>(ba->w_work.get());
  int *d_aidx = (int *)(W + o_aidx), *d_count = (int *)(W + o_count);
  unsigned long long *d_mask = (unsigned long long *)(W + o_mask);
  int *d_eoff = (int *)(W + o_eoff), *d_tile = (int *)(W + o_tile), *d_lms = (int *)(W + o_lms), *d_lml = (int *)(W + o_lml);
  unsigned char *d_pat = (unsigned char *)(W + o_pat);
  WinCounters *d_ctr = (WinCounters *)(W + o_ctr);
  // device buffers of the optimizer proper (grow-only, as in svs_ba_set_problem)
  SVS_HIP(ctx, ba_grow(ba->d_edges, sizeof(svs_ba_edge) * capE));
  for (int k = 0; k < 2; ++k) {
    SVS_HIP(ctx, ba_grow(ba->d_poses[k], sizeof(double) * 12 * (size_t)P));
    SVS_HIP(ctx, ba_grow(ba->d_psi[k], sizeof(double) * 3 * (size_t)std::max(L, 1)));
  }
  SVS_HIP(ctx, ba_grow(ba->d_cons, sizeof(svs_ba_constraint) * (size_t)std::max(C, 1)));
  SVS_HIP(ctx, ba_grow(ba->d_x, sizeof(double) * 6 * (size_t)P));
  // ---- enqueue: one upload, three clears, seven kernels, one read-back ----------------------------------------------------------------------
  const int TB = 256;
  int rc = SVS_OK;
  {   // one launch instead of three memsets: both id tables to -1; count, masks, pattern, counters to 0
    const size_t nz = ((o_ctr - o_count) + sizeof(WinCounters) + 3) / 4, n_all = std::max({pose_tab_n, point_tab_n, nz});
    hipLaunchKernelGGL(win_clear_kernel, dim3((unsigned)std::min<size_t>((n_all + 4 * TB - 1) / (4 * TB), 2048)), dim3(TB), 0, ctx->stream, ba->w_pose_tab,
                       pose_tab_n, ba->w_point_tab, point_tab_n, reinterpret_cast<int *>(W + o_count), nz);
  }
  {
    WinIn A;
    A.pids = S.pids; A.lids = S.lids; A.poses = S.poses; A.psi = S.psi; A.obs = S.obs; A.cons = S.cons;
    A.P = P; A.L = L; A.obs_words = (size_t)n_new * (sizeof(svs_ba_edge) / 8); A.cons_words = (size_t)C * (sizeof(svs_ba_constraint) / 8);
    A.poses0 = ba->d_poses[0]; A.poses1 = ba->d_poses[1]; A.psi0 = ba->d_psi[0]; A.psi1 = ba->d_psi[1];
    A.store_tail = reinterpret_cast<double *>(S.store_tail); A.d_cons = reinterpret_cast<double *>(ba->d_cons.get()); A.d_x = ba->d_x;
    A.pose_tab = ba->w_pose_tab; A.point_tab = ba->w_point_tab;
    const size_t n_max = std::max<size_t>({12 * (size_t)P, 3 * (size_t)L, A.obs_words, A.cons_words, (size_t)1});
    hipLaunchKernelGGL(win_unpack_kernel, dim3((unsigned)((n_max + TB - 1) / TB)), dim3(TB), 0, ctx->stream, A);
  }
  if (L) hipLaunchKernelGGL(win_anchor_kernel, dim3(div_up(L, TB)), dim3(TB), 0, ctx->stream, S.aids, L, ba->w_pose_tab, d_aidx);
  SVS_LAUNCH_CHECK(ctx);
  auto stage = [&](const char *what) { if (ba->opt.debug >= 2) { const hipError_t e = hipStreamSynchronize(ctx->stream); fprintf(stderr, "[svs_ba] window stage %s: %s\n", what, hipGetErrorString(e)); } };
  stage("tables");
  if (N && L) {
    const unsigned gN = (unsigned)((N + TB - 1) / TB);
    hipLaunchKernelGGL(win_mark_kernel, dim3(gN), dim3(TB), 0, ctx->stream, S.store, N, ba->w_pose_tab, pose_tab_n, ba->w_point_tab, point_tab_n, d_aidx,
                       d_count, d_mask, d_ctr);
    stage("mark");
    hipLaunchKernelGGL(win_tile_hist_kernel, dim3((unsigned)n_tiles), dim3(256), 0, ctx->stream, d_count, d_aidx, L, P, d_tile);
    hipLaunchKernelGGL(win_col_scan_kernel, dim3(1), dim3(512), 0, ctx->stream, d_tile, (int)n_tiles, P, d_ctr);
    stage("landmark order");
    hipLaunchKernelGGL(win_tile_rank_kernel, dim3((unsigned)n_tiles), dim3(WIN_TILE), 0, ctx->stream, d_count, d_aidx, d_mask, L, P, d_tile, d_ctr, d_eoff, d_lms, d_lml, d_pat);
    stage("rank");
    hipLaunchKernelGGL(win_place_kernel, dim3(gN), dim3(TB), 0, ctx->stream, S.store, N, ba->w_pose_tab, pose_tab_n, ba->w_point_tab, point_tab_n, d_aidx,
                       d_eoff, d_mask, ba->d_edges);
    SVS_LAUNCH_CHECK(ctx);
    stage("place");
    if (ba->opt.debug >= 2) { WinCounters hc; (void)hipMemcpy(&hc, d_ctr, sizeof hc, hipMemcpyDeviceToHost); fprintf(stderr, "[svs_ba] window counters: n_edges %d n_lm %d dup %d (N %zu L %d P %d)\n", hc.n_edges, hc.n_lm, hc.dup, N, L, P); }
  }
  // ---- one read-back: pattern | counters | landmark lengths (contiguous in the work arrays) ------------------------------------------------
  const size_t back_bytes = (o_lml - o_pat) + 4 * ((size_t)L + 2);
  if (back_bytes > ba->w_hback.bytes()) SVS_HIP(ctx, ba->w_hback.alloc_bytes(back_bytes + back_bytes / 2));
  unsigned char *h_pat = ba->w_hback;
  WinCounters *h_ctr = reinterpret_cast<WinCounters *>(ba->w_hback + (o_ctr - o_pat));
  int *h_lml = reinterpret_cast<int *>(ba->w_hback + (o_lml - o_pat));
  SVS_HIP(ctx, hipMemcpyAsync(ba->w_hback, W + o_pat, back_bytes, hipMemcpyDeviceToHost, ctx->stream));
  auto t_e = std::chrono::steady_clock::now();
  SVS_HIP(ctx, hipStreamSynchronize(ctx->stream));
  ba->h_stage_used = 0;                                 // everything staged so far has been consumed
  auto t_1 = std::chrono::steady_clock::now();
  if (h_ctr->dup) { ctx->err = "svs_ba_window_update: two observations of one point in one keyframe"; return SVS_ERR_INVALID; }
  const int E = (N && L) ? h_ctr->n_edges : 0, n_lm = (N && L) ? h_ctr->n_lm : 0;
  // ---- host: wave chunks, wide landmarks, constraints by index, pattern -> envelope -------------------------------------------------
  std::vector<int> &cs = ba->w_cs, &cl = ba->w_cl;
  cs.clear(); cl.clear();
  int n_reg = n_lm;
  while (n_reg > 0 && h_lml[n_reg - 1] > 64) --n_reg;               // wide landmarks sort to the end (key bit 41)
  {
    int start = 0;
    for (int k = 0; k < n_reg;) {
      const int s0 = start;
      int len = 0;
      while (k < n_reg && len + h_lml[k] <= 64) { len += h_lml[k]; ++k; }
      cs.push_back(s0); cl.push_back(len);
      start += len;
    }
    ba->n_chunks = (int)cs.size();
    ba->nw_sched = 0;
    ba->n_wide = n_lm - n_reg;
    for (int k = n_reg; k < n_lm; ++k) {
      if (h_lml[k] > WIDE_THREADS) { ctx->err = "svs_ba: a landmark with more than 256 observations"; return SVS_ERR_UNSUPPORTED; }
      cs.push_back(start); cl.push_back(h_lml[k]); start += h_lml[k];
    }
  }
  ba->h_pattern.assign((size_t)P * P, 0.0);
  for (size_t i = 0; i < (size_t)P * P; ++i) if (h_pat[i]) ba->h_pattern[i] = 1.0;
  for (int c = 0; c < C; ++c) ba->h_pattern[(size_t)std::min(cons_idx[c].pose1, cons_idx[c].pose2) * P + std::max(cons_idx[c].pose1, cons_idx[c].pose2)] = 1.0;
  ba->P = P; ba->L = L; ba->E = E; ba->C = C; ba->cam = *cam; ba->prm = *prm; ba->add_pose_terms = 1; ba->cur = 0;
  ba->profile_ready = false; ba->env_R = 0; ba->use_lds_solve = ba->use_fused_solve = false;
  const size_t nblk = (size_t)P * (P + 1) / 2;
  ba->red_count = nblk * 36 + 12 * (size_t)P + SC_SLOTS;
  SVS_HIP(ctx, ba_grow(ba->d_chunk_start, sizeof(int) * (size_t)std::max(ba->n_chunks + ba->n_wide, 1)));
  SVS_HIP(ctx, ba_grow(ba->d_chunk_len, sizeof(int) * (size_t)std::max(ba->n_chunks + ba->n_wide, 1)));
  SVS_HIP(ctx, ba_grow(ba->d_red, sizeof(double) * ba->red_count));
  SVS_HIP(ctx, ba_grow(ba->d_scal, sizeof(double) * SC_N));
  SVS_HIP(ctx, ba_grow(ba->d_linv, sizeof(double) * 36 * (size_t)P));
  SVS_HIP(ctx, ba_grow(ba->d_rowmax, sizeof(int) * (size_t)P));
  SVS_HIP(ctx, ba_grow(ba->d_colmin, sizeof(int) * (size_t)P));
  SVS_HIP(ctx, ba_grow(ba->d_pattern, sizeof(double) * (size_t)P * P));
  if (!cs.empty()) {
    if ((rc = stage_upload(ba, ba->d_chunk_start, cs.data(), sizeof(int) * cs.size()))) return rc;
    if ((rc = stage_upload(ba, ba->d_chunk_len, cl.data(), sizeof(int) * cl.size()))) return rc;
  }
  if (ba->opt.debug) {
    auto us = [](std::chrono::steady_clock::time_point a, std::chrono::steady_clock::time_point b) { return std::chrono::duration<double, std::micro>(b - a).count(); };
    fprintf(stderr, "[svs_ba] window_update: store %zu obs (+%d), window %d edges / %d landmarks / %d chunks / %d wide; ids + staging + uploads %.0f us, allocations + enqueue %.0f us, wait for the read-back %.0f us, host tail %.0f us\n",
            N, n_new, E, n_lm, ba->n_chunks, ba->n_wide, us(t_0, t_s), us(t_s, t_e), us(t_e, t_1), us(t_1, std::chrono::steady_clock::now()));
  }
  ba->problem_valid = true;
  return SVS_OK;
}


// ---- the window svs_map_prepare_window left in the map (ba_map.h) ---------------------------------------------------------------------------------------
// copyDataToG2o device to device: ids, anchors, poses and psi are read where the map's kernels wrote them, the store is the map's measured store, and only the
// constraints are staged.  Everything that can be refused is refused before the handle is touched.
// from_edges: the constraints are copyContraintsToG2o's list out of the map's edge table (C and h_cons unused), gathered on the device
static int window_from_map_impl(svs_ba *ba, svs_map *map, int C, const svs_ba_constraint *h_cons, bool from_edges, const svs_cam *cam, const svs_ba_params *prm) {
  svs_ctx *ctx = ba ? ba->ctx : nullptr;
  SVS_REQUIRE(ctx, ba && map && C >= 0 && (C == 0 || h_cons) && cam && prm);
  SVS_REQUIRE(ctx, svs_map_ctx(map) == ctx);          // one context: one stream orders the map's kernels and the assembly
  SVS_REQUIRE(ctx, !ba->comm);                        // single-GPU path, as svs_ba_window_update
  SVS_DEVICE(ctx);
  std::vector<int4> list;
  if (from_edges) {                                   // (an edge that is not marginalised, no valid prepared window: nothing enqueued)
    if (int rc = svs_map_window_constraint_list(map, &list)) return rc;
    C = (int)list.size();
  }
  MapWindowView V;
  if (int rc = svs_map_window_view(map, &V)) return rc;      // no valid prepared window: nothing enqueued
  const int P = V.P, L = V.L;
  SVS_REQUIRE(ctx, P >= 1 && P <= SOLVE_MAX_P && L >= 0 && L < (1 << 23) && V.n_store < (size_t)INT_MAX - 1);
  auto t_0 = std::chrono::steady_clock::now();
  std::vector<svs_ba_constraint> cons_idx((size_t)C);
  for (int c = 0; c < C && !from_edges; ++c) {
    cons_idx[c] = h_cons[c];
    int i1 = -1, i2 = -1;
    for (int i = 0; i < P; ++i) { if (V.h_window_ids[i] == h_cons[c].pose1) i1 = i; if (V.h_window_ids[i] == h_cons[c].pose2) i2 = i; }
    SVS_REQUIRE(ctx, i1 >= 0 && i2 >= 0);                   // a constraint of this window names two keyframes of the final window
    cons_idx[c].pose1 = i1; cons_idx[c].pose2 = i2;
  }
  for (int c = 0; c < C && from_edges; ++c) { cons_idx[c] = svs_ba_constraint{}; cons_idx[c].pose1 = list[c].x; cons_idx[c].pose2 = list[c].y; }      // (the host reads the indices only)
  ba->problem_valid = false; ba->from_map_serial = 0;
  ba->w_cons_idx.swap(cons_idx);
  SVS_HIP(ctx, hipStreamSynchronize(ctx->stream));
  ba->h_stage_used = 0;
  const size_t cons_bytes = sizeof(svs_ba_constraint) * (size_t)C, o_list = (cons_bytes + 255) & ~(size_t)255, list_bytes = from_edges ? sizeof(int4) * (size_t)C : 0,
               in_bytes = o_list + list_bytes;
  { int rc = stage_reserve(ba, in_bytes + sizeof(int) * (V.n_store / 8 + 8 * (size_t)P) + 16384); if (rc) return rc; }
  SVS_HIP(ctx, ba->w_in.reserve_keep(in_bytes + 256, in_bytes + in_bytes / 2 + 4096, 0));
  if (C && !from_edges) {
    std::memcpy(ba->h_stage.get(), ba->w_cons_idx.data(), cons_bytes);
    ba->h_stage_used = (cons_bytes + 255) & ~(size_t)255;
    SVS_HIP(ctx, hipMemcpyAsync(ba->w_in, ba->h_stage.get(), cons_bytes, hipMemcpyHostToDevice, ctx->stream));
  }
  if (C && from_edges) {                              // the integer list crosses the link; the records are written where win_unpack_kernel reads them
    std::memcpy(ba->h_stage.get(), list.data(), list_bytes);
    ba->h_stage_used = (list_bytes + 255) & ~(size_t)255;
    char *IN = static_cast<char *>(ba->w_in.get());
    SVS_HIP(ctx, hipMemcpyAsync(IN + o_list, ba->h_stage.get(), list_bytes, hipMemcpyHostToDevice, ctx->stream));
    if (int rc = svs_map_gather_constraints(map, reinterpret_cast<const int4 *>(IN + o_list), C, reinterpret_cast<svs_ba_constraint *>(IN))) return rc;
  }
  WinSrc S;
  S.pids = V.window_ids; S.lids = V.active_ids; S.aids = V.anchor_ids; S.poses = V.poses; S.psi = V.psi; S.obs = nullptr;
  S.cons = static_cast<const double *>(ba->w_in.get());
  S.n_new = 0; S.store_tail = nullptr; S.store = V.store; S.N = V.n_store;
  S.max_pose_id = std::max(V.kf_hi - 1, 0); S.max_point_id = std::max(V.pt_hi - 1, 0);
  const int rc = window_assemble(ba, P, L, C, S, cam, prm, t_0, std::chrono::steady_clock::now());
  if (rc == SVS_OK) ba->from_map_serial = V.serial;
  return rc;
}

extern "C" int svs_ba_window_from_map(svs_ba *ba, svs_map *map, int C, const svs_ba_constraint *h_cons, const svs_cam *cam, const svs_ba_params *prm) {
  return window_from_map_impl(ba, map, C, h_cons, false, cam, prm);
}

extern "C" int svs_ba_window_from_map_edges(svs_ba *ba, svs_map *map, const svs_cam *cam, const svs_ba_params *prm) {
  return window_from_map_impl(ba, map, 0, nullptr, true, cam, prm);
}

extern "C" int svs_ba_window_constraints(svs_ba *ba, int32_t *n, svs_ba_constraint *h_cons) {
  svs_ctx *ctx = ba ? ba->ctx : nullptr;
  SVS_REQUIRE(ctx, ba && n && ba->problem_valid);
  *n = ba->C;
  if (!h_cons || ba->C == 0) return SVS_OK;
  SVS_DEVICE(ctx);
  SVS_HIP(ctx, hipMemcpyAsync(h_cons, ba->d_cons, sizeof(svs_ba_constraint) * (size_t)ba->C, hipMemcpyDeviceToHost, ctx->stream));
  SVS_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return SVS_OK;
}

extern "C" int svs_ba_store_to_map(svs_ba *ba, svs_map *map) {
  svs_ctx *ctx = ba ? ba->ctx : nullptr;
  SVS_REQUIRE(ctx, ba && map && svs_map_ctx(map) == ctx);
  SVS_REQUIRE(ctx, ba->problem_valid && ba->from_map_serial != 0 && svs_map_window_is(map, ba->from_map_serial));
  SVS_DEVICE(ctx);
  return svs_map_window_store(map, ba->d_poses[ba->cur], ba->d_psi[ba->cur]);
}

extern "C" int svs_ba_window_edges(svs_ba *ba, int32_t *n, svs_ba_edge *h_edges) {
  svs_ctx *ctx = ba ? ba->ctx : nullptr;
  SVS_REQUIRE(ctx, ba && n && ba->problem_valid);
  *n = ba->E;
  if (!h_edges || ba->E == 0) return SVS_OK;
  SVS_DEVICE(ctx);
  SVS_HIP(ctx, hipMemcpyAsync(h_edges, ba->d_edges, sizeof(svs_ba_edge) * (size_t)ba->E, hipMemcpyDeviceToHost, ctx->stream));
  SVS_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return SVS_OK;
}
