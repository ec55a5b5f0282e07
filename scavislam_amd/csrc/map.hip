// map.hip -- the back end's map kept on the device for keyframe re-registration (svs_map_*), and the walk that builds the requests of the registration chain
// (register.hip) from it: pointsVisibleInRoot's point walk (backend.cpp:480-497) / the query keyframe's feature_table (:853-858) as set operations.
//   storage         keyframes, points and thresholds by id; the observations as an append log of (point, keyframe) pairs plus two CSR views -- by keyframe
//                   (a feature_table) and by point (an observer row, sorted by keyframe id) -- rebuilt by a counting sort when the log has grown
//   map_scatter_*   the updates: one staged upload, one lane per record (16-byte loads of the 64-byte point records)
//   map_count / map_scan / map_fill / map_sort_rows      the CSR rebuild
//   map_build_kernel    one workgroup per request: the walk and direct sets and the built table are LDS bitmaps over keyframe ids, the point set a bitmap in
//                   global memory (one row per request); marking walks the feature_tables of the walk set, compaction turns bitmap words into ascending ids by
//                   popcounts and a wave64 / workgroup prefix, so no atomic decides an order: the built request is a function of the map's content alone
//   map_nbh_kernel      one workgroup per request of a front-end stream (nbh_map.h): addPointsToNeighbors / addAnchorPosesToNeighbors (backend.cpp:311-386) with the
//                   same sets, written straight into the stream's candidate list, group ends and keyframe slots
//   map_win_mark / map_win_list    the double window's BA problem (ba_map.h): computeActivePointsAndExtendOuterWindow (slam_graph.cpp:599-663) with one workgroup per
//                   INNER keyframe -- W0 and its graph neighbours as LDS bitmaps, active points and the extension as bitmaps in global memory -- then ascending
//                   lists, poses and psi = invert_depth(xyz_anchor) by popcount prefixes; map_win_gather / map_win_store move the state to and from the optimizer
//   map_edge_* / map_cons_kernel   the pose graph's edges (EdgeTable, slam_graph.hpp:197-363: one record per undirected edge, T_lo_from_hi and one Lambda) and
//                   computeConstraint (slam_graph.cpp:787-846) with one workgroup per keyframe pair -- common points as an ordered bitmap compaction, depths in f64,
//                   the median by a radix select over the doubles' bit patterns, setConstraint in the same launch; map_edge_gather is copyContraintsToG2o
//   map_walk.inc        the pose graph's walks (computeInitialDoubleWin, framesInNeighborhood, shortestPathToWindow + computeAbsolutePose, reinitializePoses): a
//                   strength-ordered adjacency built from the edge records and one level-synchronous breadth-first search per request; behind them the four
//                   map_nbr_* kernels of a front-end stream's whole neighbourhood from a root id (nbr_map.h): findNeighborsOfRoot, nbh_collect below, the searches
//                   from a device-built list, then poses, strength_to_neighbors, the strength matrix, the head's order, the list and the resident vertex table
//   map_addkf.inc       inserting a keyframe (SlamGraph::addKeyframe): computeStrength as counting passes over the track points' observer rows with one workgroup per
//                   call, the kept points and measured pairs compacted by prefix sums, the new edges' constraints through map_cons_kernel; two read-backs
//   map_commit.inc      registerKeyframes / addLoopClosure: a device track list and an edge list applied to the map (the new pairs appended by prefix sums, the
//                   edges through map_edge_add_kernel, their constraints through map_cons_kernel with the pose override)
// Integer and copy work throughout (but for the three divisions of invert_depth and the f64 geometry of map_cons_kernel); the host keeps the id sets and the set of pairs, so every refusal happens before anything is uploaded.
#include "reg_map.h"
#include "nbh_map.h"
#include "nbr_map.h"
#include "ba_map.h"
#include "walk_map.h"
#include "kf_map.h"
#include "pose.h"
#include <string.h>
#include <algorithm>
#include <unordered_map>
#include <unordered_set>
#include <vector>

namespace {
constexpr int MB_THREADS = 512;
constexpr int MAP_MAX_KF = 16384;
constexpr int MAP_KF_WORDS = MAP_MAX_KF / 32;      // = MB_THREADS: one bitmap word per lane
constexpr int THR_N = SVS_NUM_PYR_LEVELS * SVS_MAX_CELLS;
static_assert(MAP_KF_WORDS == MB_THREADS, "the rank pass gives every lane one word");
static_assert(sizeof(svs_candidate_point) == 64 && sizeof(svs_keyframe) == 136, "record copies below");

// the map's tables as the kernels read them
struct MapK {
  svs_keyframe *kf; const float **kf_disp; int32_t *kf_dstride; int32_t *kf_thr; uint8_t *kf_flags;
  svs_candidate_point *pt;
  const int2 *log; int n_log;
  int32_t *kf_begin, *kf_rows, *pt_begin, *pt_rows, *kf_cur, *pt_cur;
  int kf_hi, pt_hi;                    // every id in use is below these
  uint32_t *mark; size_t mark_b;       // [requests][mark_b] words: the point set of a request
};

// ---- updates: lane i scatters staged record i -------------------------------------------------------------------------------------------------------
struct kf_up { int32_t id, disp_stride; const float *disp; svs_keyframe kf; int32_t thr[THR_N]; };
static_assert(sizeof(kf_up) % 8 == 0, "staged as an array");

__global__ __launch_bounds__(256) void map_scatter_kf_kernel(MapK M, const kf_up *up, int n) {
  // 64 lanes per record: the thresholds are the bulk
  const int i = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (i >= n) return;
  const kf_up &u = up[i];
  const int id = u.id;
  for (int k = lane; k < THR_N; k += 64) M.kf_thr[(size_t)id * THR_N + k] = u.thr[k];
  if (lane < 17) reinterpret_cast<long long *>(M.kf + id)[lane] = reinterpret_cast<const long long *>(&u.kf)[lane];
  if (lane == 17) { M.kf_disp[id] = u.disp; M.kf_dstride[id] = u.disp_stride; M.kf_flags[id] = 0; }
}

__global__ __launch_bounds__(256) void map_scatter_pt_kernel(MapK M, const int32_t *ids, const svs_candidate_point *up, int n) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int id = ids[i];
  const int4 *s4 = reinterpret_cast<const int4 *>(up + i);
  int4 *d4 = reinterpret_cast<int4 *>(M.pt + id);
  int4 q = s4[3];
  q.z = id; q.w = 0;                   // anchor_level, kf_index (the anchor's id), point_id, pad_
  d4[0] = s4[0]; d4[1] = s4[1]; d4[2] = s4[2]; d4[3] = q;
}

__global__ __launch_bounds__(256) void map_scatter_pose_kernel(MapK M, const int32_t *ids, const double *poses, int n) {
  const int t = blockIdx.x * 256 + threadIdx.x, i = t / 12, k = t % 12;
  if (i < n) M.kf[ids[i]].T_anchor_from_w[k] = poses[(size_t)i * 12 + k];
}

__global__ __launch_bounds__(256) void map_scatter_xyz_kernel(MapK M, const int32_t *ids, const double *xyz, int n) {
  const int t = blockIdx.x * 256 + threadIdx.x, i = t / 3, k = t % 3;
  if (i < n) M.pt[ids[i]].xyz_anchor[k] = xyz[(size_t)i * 3 + k];
}

// set == 0: every flag byte below kf_hi loses the bit; set == 1: the listed keyframes get it (two launches, stream order)
__global__ __launch_bounds__(256) void map_window_kernel(MapK M, const int32_t *ids, int n, int set) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (set) { if (i < n) M.kf_flags[ids[i]] = SVS_REG_KF_IN_WINDOW; }
  else if (i < M.kf_hi) M.kf_flags[i] = 0;
}

// ---- the CSR rebuild -----------------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int wave_incl_scan(int v) {
  const int lane = lane_id();
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) { const int t = __shfl_up(v, o, 64); if (lane >= o) v += t; }
  return v;
}
// exclusive prefix of v over the MB_THREADS lanes of the workgroup, `total` = the sum; every lane calls it (two barriers inside)
__device__ __forceinline__ int block_excl_scan(int v, int *s_w, int &total) {
  const int lane = lane_id(), wave = threadIdx.x >> 6;
  const int inc = wave_incl_scan(v);
  if (lane == 63) s_w[wave] = inc;
  __syncthreads();
  int off = 0, tot = 0;
#pragma unroll
  for (int w = 0; w < MB_THREADS / 64; ++w) { const int k = s_w[w]; off += w < wave ? k : 0; tot += k; }
  __syncthreads();
  total = tot;
  return off + inc - v;
}

// ctr[key] += 1 for every active lane, with ONE atomic per distinct key of the wave: the log is appended a feature_table at a time, so the 64 lanes of a wave
// mostly hold one keyframe, and 64 atomics on one address serialise in the L2.  Returns the lane's slot (the counter's old value + its rank among the wave's
// lanes with that key), -1 for an inactive lane.  Every lane of the wave calls it (ballots and shuffles inside)
__device__ __forceinline__ int wave_add_by_key(int32_t *ctr, int key, bool active) {
  const int lane = lane_id();
  int slot = -1;
  unsigned long long todo = __ballot(active);
  while (todo) {                                         // wave-uniform
    const int leader = __ffsll((long long)todo) - 1;     // an active lane
    const int k0 = __shfl(key, leader, 64);
    const bool mine = active && key == k0;
    const unsigned long long mask = __ballot(mine);      // holds the leader's bit: the loop ends
    int base = 0;
    if (lane == leader) base = atomicAdd(&ctr[k0], __popcll(mask));
    base = __shfl(base, leader, 64);
    if (mine) { slot = base + __popcll(mask & ((1ull << lane) - 1ull)); active = false; }
    todo &= ~mask;
  }
  return slot;
}

__global__ __launch_bounds__(256) void map_count_kernel(MapK M) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  const bool active = e < M.n_log;
  const int2 o = active ? M.log[e] : make_int2(0, 0);      // (point, keyframe): ids the host has checked
  if (active) atomicAdd(&M.pt_begin[o.x], 1);              // a point is in a wave once, but for pairs of different feature_tables
  (void)wave_add_by_key(M.kf_begin, o.y, active);
}

// workgroup 0: keyframes, workgroup 1: points.  counts [n] -> begin [n + 1] in place, and a copy as the fill cursors.  Eight entries per lane and step (two
// 16-byte loads where all eight exist), so the single workgroup's chain of barriers is n / 4096 steps long
constexpr int SCAN_ITEMS = 8;
__global__ __launch_bounds__(MB_THREADS) void map_scan_kernel(MapK M) {
  __shared__ int s_w[MB_THREADS / 64];
  int32_t *a = blockIdx.x == 0 ? M.kf_begin : M.pt_begin, *cur = blockIdx.x == 0 ? M.kf_cur : M.pt_cur;
  const int n = blockIdx.x == 0 ? M.kf_hi : M.pt_hi;
  int run = 0;
  for (int base = 0; base <= n; base += MB_THREADS * SCAN_ITEMS) {      // block-uniform; entry n becomes the total
    const int i0 = base + threadIdx.x * SCAN_ITEMS;                     // a multiple of 8: 16-byte aligned in a hipMalloc block
    int v[SCAN_ITEMS];
    if (i0 + SCAN_ITEMS <= n) {
      const int4 lo = reinterpret_cast<const int4 *>(a + i0)[0], hi = reinterpret_cast<const int4 *>(a + i0)[1];
      v[0] = lo.x; v[1] = lo.y; v[2] = lo.z; v[3] = lo.w; v[4] = hi.x; v[5] = hi.y; v[6] = hi.z; v[7] = hi.w;
    } else {
#pragma unroll
      for (int k = 0; k < SCAN_ITEMS; ++k) v[k] = i0 + k < n ? a[i0 + k] : 0;
    }
    int sum = 0;
#pragma unroll
    for (int k = 0; k < SCAN_ITEMS; ++k) { const int c = v[k]; v[k] = sum; sum += c; }
    int tot;
    const int off = run + block_excl_scan(sum, s_w, tot);
    if (i0 + SCAN_ITEMS <= n + 1) {
      const int4 lo = make_int4(off + v[0], off + v[1], off + v[2], off + v[3]), hi = make_int4(off + v[4], off + v[5], off + v[6], off + v[7]);
      reinterpret_cast<int4 *>(a + i0)[0] = lo; reinterpret_cast<int4 *>(a + i0)[1] = hi;
      reinterpret_cast<int4 *>(cur + i0)[0] = lo; reinterpret_cast<int4 *>(cur + i0)[1] = hi;
    } else {
#pragma unroll
      for (int k = 0; k < SCAN_ITEMS; ++k)
        if (i0 + k <= n) { a[i0 + k] = off + v[k]; cur[i0 + k] = off + v[k]; }
    }
    run += tot;
  }
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

// ---- the walk: one workgroup per request ---------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ bool bit_of(const uint32_t *s, int i) { return (s[i >> 5] >> (i & 31)) & 1u; }

__global__ __launch_bounds__(MB_THREADS) void map_build_kernel(MapK M, MapBuildDst D) {
  __shared__ uint32_t s_walk[MAP_KF_WORDS], s_dir[MAP_KF_WORDS], s_tab[MAP_KF_WORDS];
  __shared__ int s_rank[MAP_KF_WORDS];
  __shared__ int s_w[MB_THREADS / 64];
  const int r = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const map_req &Q = D.req[r];
  const int root = Q.root, mode = Q.mode;
  const int32_t *walk = D.ids + Q.walk_off, *direct = D.ids + Q.direct_off;
  uint32_t *mark = M.mark + (size_t)r * M.mark_b;
  const int n_words = (M.pt_hi + 31) >> 5;                      // <= mark_b
  // a. empty sets
  s_walk[tid] = 0; s_dir[tid] = 0; s_tab[tid] = 0;
  for (int i = tid; i < n_words; i += MB_THREADS) mark[i] = 0;
  __syncthreads();
  // b. the keyframe sets (ids the host has checked: in the map, so below kf_hi <= MAP_MAX_KF)
  for (int i = tid; i < Q.n_direct; i += MB_THREADS) { const int id = direct[i]; atomicOr(&s_dir[id >> 5], 1u << (id & 31)); }
  for (int i = tid; i < Q.n_walk; i += MB_THREADS) { const int id = walk[i]; atomicOr(&s_walk[id >> 5], 1u << (id & 31)); }
  if (tid == 0) atomicOr(&s_dir[root >> 5], 1u << (root & 31));      // directNeighborsOf inserts the frame itself (:437)
  __syncthreads();
  // c. mark the points: a wave per feature_table
  const int n_marking = mode == SVS_REG_LOOP ? 1 : Q.n_walk;
  for (int i = wave; i < n_marking; i += MB_THREADS / 64) {
    const int kf = walk[i];
    if (mode == SVS_REG_LOCAL && bit_of(s_dir, kf)) continue;      // (:485)
    const int e1 = M.kf_begin[kf + 1];
    for (int e = M.kf_begin[kf] + lane; e < e1; e += 64) {
      const int p = M.kf_rows[e];
      if ((unsigned)p < (unsigned)M.pt_hi) atomicOr(&mark[p >> 5], 1u << (p & 31));
    }
  }
  __syncthreads();
  // d. the source list: the set bits in ascending order
  int n_src = 0;
  for (int base = 0; base < n_words; base += MB_THREADS) {      // block-uniform trip count
    const int w = base + tid;
    uint32_t bits = w < n_words ? __hip_atomic_load(&mark[w], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0u;
    int tot;
    int pos = n_src + block_excl_scan(__popc(bits), s_w, tot);
    while (bits) {
      const int b = __ffs((int)bits) - 1;
      bits &= bits - 1;
      if (pos < D.SB) D.point_id[(size_t)r * D.NP + pos] = (w << 5) + b;      // SB <= NP
      ++pos;
    }
    n_src += tot;
  }
  const int n_src_c = min(n_src, D.SB);
  __syncthreads();
  // e. the records (four 16-byte loads each); their anchors join the table
  svs_candidate_point *src = D.src + (size_t)r * D.SB;
  for (int i = tid; i < n_src_c; i += MB_THREADS) {
    const int p = D.point_id[(size_t)r * D.NP + i];
    const int4 *s4 = reinterpret_cast<const int4 *>(M.pt + p);
    int4 *d4 = reinterpret_cast<int4 *>(src + i);
    const int4 q = s4[3];
    d4[0] = s4[0]; d4[1] = s4[1]; d4[2] = s4[2]; d4[3] = q;      // kf_index: still the anchor's id (translated in g)
    if ((unsigned)q.y < (unsigned)MAP_MAX_KF) atomicOr(&s_tab[q.y >> 5], 1u << (q.y & 31));
  }
  __syncthreads();
  // f. the table: entry 0 the root, behind it anchors and walk keyframes in ascending id; the rank of a word's first bit by a prefix over the popcounts
  int n_kf;
  {
    uint32_t bits = s_tab[tid] | s_walk[tid];
    if (tid == (root >> 5)) bits &= ~(1u << (root & 31));
    s_tab[tid] = bits;                                            // a lane's own word
    int tot;
    const int rank = block_excl_scan(__popc(bits), s_w, tot);
    s_rank[tid] = rank;
    n_kf = 1 + tot;
    svs_keyframe *kfs = D.kfs + (size_t)r * D.KB;
    uint8_t *flags = D.flags + (size_t)r * D.KB;
    int32_t *kf_id = D.kf_id + (size_t)r * D.KB;
    int e = 1 + rank;
    while (bits) {
      const int id = (tid << 5) + __ffs((int)bits) - 1;
      bits &= bits - 1;
      if (e < D.KB) {
        for (int k = 0; k < 17; ++k) reinterpret_cast<long long *>(kfs + e)[k] = reinterpret_cast<const long long *>(M.kf + id)[k];
        flags[e] = (uint8_t)((M.kf_flags[id] & SVS_REG_KF_IN_WINDOW) | (bit_of(s_dir, id) ? SVS_REG_KF_DIRECT_NEIGHBOR : 0));
        kf_id[e] = id;
      }
      ++e;
    }
    if (tid == 0) {                                               // KB >= 1
      for (int k = 0; k < 17; ++k) reinterpret_cast<long long *>(kfs)[k] = reinterpret_cast<const long long *>(M.kf + root)[k];
      flags[0] = (uint8_t)((M.kf_flags[root] & SVS_REG_KF_IN_WINDOW) | SVS_REG_KF_DIRECT_NEIGHBOR);
      kf_id[0] = root;
    }
    // behind the table: what the stateless call's staging holds there
    for (int k = min(n_kf, D.KB) + tid; k < D.KB; k += MB_THREADS) {
      for (int q = 0; q < 17; ++q) reinterpret_cast<long long *>(kfs + k)[q] = 0;
      flags[k] = 0;
    }
  }
  __syncthreads();
  // g. anchors as table entries; the observer rows
  int32_t *ob = D.obs_begin + (size_t)r * (D.SB + 1), *ok = D.obs_kf + (size_t)r * D.OB;
  int n_obs = 0;
  for (int base = 0; base < n_src_c; base += MB_THREADS) {      // block-uniform
    const int i = base + tid;
    int c = 0, p = -1, row_b = 0, row_e = 0;
    bool has_root = false;
    if (i < n_src_c) {
      const int a = src[i].kf_index;                              // written by this lane in e
      src[i].kf_index = a == root ? 0 : 1 + s_rank[a >> 5] + __popc(s_tab[a >> 5] & ((1u << (a & 31)) - 1u));
      if (mode == SVS_REG_LOCAL) {
        p = D.point_id[(size_t)r * D.NP + i];
        row_b = M.pt_begin[p]; row_e = M.pt_begin[p + 1];
        for (int e = row_b; e < row_e; e += 4) {                   // four loads in flight: a row is read at the latency of a quarter of its entries
          int kf[4];
#pragma unroll
          for (int k = 0; k < 4; ++k) kf[k] = e + k < row_e ? M.pt_rows[e + k] : -1;
#pragma unroll
          for (int k = 0; k < 4; ++k) {
            if (kf[k] == root) has_root = true;
            else if ((unsigned)kf[k] < (unsigned)MAP_MAX_KF && bit_of(s_tab, kf[k])) ++c;
          }
        }
        c += has_root ? 1 : 0;
      }
    }
    int tot;
    int pos = n_obs + block_excl_scan(c, s_w, tot);
    if (i < n_src_c && mode == SVS_REG_LOCAL) {
      ob[i] = pos;
      if (has_root) { if (pos < D.OB) ok[pos] = 0; ++pos; }
      for (int e = row_b; e < row_e; e += 4) {                     // ascending ids = ascending entries
        int kf[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) kf[k] = e + k < row_e ? M.pt_rows[e + k] : -1;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          if (kf[k] != root && (unsigned)kf[k] < (unsigned)MAP_MAX_KF && bit_of(s_tab, kf[k])) {
            if (pos < D.OB) ok[pos] = 1 + s_rank[kf[k] >> 5] + __popc(s_tab[kf[k] >> 5] & ((1u << (kf[k] & 31)) - 1u));
            ++pos;
          }
        }
      }
    }
    n_obs += tot;
  }
  const bool over = n_src > D.SB || n_kf > D.KB || n_obs > D.OB;
  if (tid == 0 && mode == SVS_REG_LOCAL) ob[n_src_c] = min(n_obs, D.OB);
  // h. the request record.  Over capacity: a request without points, which the chain answers at its first exit
  reg_hdr &H = D.hdr[r];
  for (int k = tid; k < THR_N; k += MB_THREADS) (&H.thr[0][0])[k] = M.kf_thr[(size_t)root * THR_N + k];
  if (tid < 12) H.T_root[tid] = Q.T_root[tid];
  if (tid == 0) {
    H.mode = mode; H.n_kf = over ? 1 : n_kf; H.n_src = over ? 0 : n_src; H.root_kf = 0;
    H.disp = M.kf_disp[root]; H.disp_stride = M.kf_dstride[root]; H.pad_ = 0;
    D.meta[r] = make_int4(n_kf, n_src, n_obs, over ? 1 : 0);
  }
}

// mark[word] |= bit for every active lane, with ONE atomic per distinct word of the wave: the points a keyframe seeded have consecutive ids, so the 64 lanes of
// a wave that reads a feature_table mostly share a few words, and atomics on one address serialise in the L2 (as wave_add_by_key found for the counters).
// Every lane of the wave calls it (ballots and shuffles inside)
__device__ __forceinline__ void wave_or_by_word(uint32_t *mark, int word, uint32_t bit, bool active) {
  const int lane = lane_id();
  unsigned long long todo = __ballot(active);
  while (todo) {                                         // wave-uniform
    const int leader = __ffsll((long long)todo) - 1;     // an active lane
    const int w0 = __shfl(word, leader, 64);
    const bool mine = active && word == w0;
    uint32_t v = mine ? bit : 0u;
#pragma unroll
    for (int o = 32; o; o >>= 1) v |= (uint32_t)__shfl_xor((int)v, o, 64);
    if (lane == leader) atomicOr(&mark[w0], v);
    todo &= ~__ballot(mine);                             // holds the leader's bit: the loop ends
  }
}

// ---- the neighbourhood of a front-end stream (Backend::computeNeighborhood from the vertex list onwards, backend.cpp:311-386): one workgroup per request.
// The same sets as above -- the given vertices and the anchors as LDS bitmaps over keyframe ids, the points as the request's row of M.mark, ascending ids by
// popcounts and prefixes -- and a table id -> slot of the stream in LDS.  Everything that decides whether the request fits (the point count, the vertex count) is
// known before the first write into the front end's tables: a request over capacity returns with those untouched.
// steps a-f of the neighbourhood of a vertex list, shared by map_nbh_kernel and map_nbr_collect_kernel (map_walk.inc): the points observed by the list's keyframes
// as ascending ids in ids_row[id_off ..] (what lies at or behind ids_row[cap] is only counted), their anchors, and the anchors that are not in the list ("extra":
// this lane's word of that bitmap, `rank` the set bits in the words before it).  Every lane of the workgroup calls it (barriers inside)
struct NbhSets { int n_map, n_no_slot, n_extra, rank; uint32_t extra; bool over_points; };
__device__ __forceinline__ NbhSets nbh_collect(const MapK &M, uint32_t *mark, int32_t *ids_row, int id_off, int cap, const int32_t *vertex, int n_vertex,
                                               const int32_t *slot_kf, int K, uint32_t *s_vert, uint32_t *s_anch, int16_t *s_slot, int *s_w) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int n_words = (M.pt_hi + 31) >> 5;                      // <= mark_b
  // a. empty sets
  s_vert[tid] = 0; s_anch[tid] = 0;
  for (int i = tid; i < MAP_MAX_KF; i += MB_THREADS) s_slot[i] = -1;
  for (int i = tid; i < n_words; i += MB_THREADS) mark[i] = 0;
  __syncthreads();
  // b. the given vertices (ids the host has checked: in the map, so below kf_hi <= MAP_MAX_KF); the slots (an id in at most one slot)
  for (int i = tid; i < n_vertex; i += MB_THREADS) { const int id = vertex[i]; atomicOr(&s_vert[id >> 5], 1u << (id & 31)); }
  for (int s = tid; s < K; s += MB_THREADS) { const int id = slot_kf[s]; if ((unsigned)id < (unsigned)MAP_MAX_KF) s_slot[id] = (int16_t)s; }
  __syncthreads();
  // c. mark the points: a wave per feature_table (:316-331)
  for (int i = wave; i < n_vertex; i += MB_THREADS / 64) {
    const int kf = vertex[i];
    const int e1 = M.kf_begin[kf + 1];
    for (int e0 = M.kf_begin[kf]; e0 < e1; e0 += 64) {          // wave-uniform
      const int p = e0 + lane < e1 ? M.kf_rows[e0 + lane] : -1;
      wave_or_by_word(mark, p >> 5, 1u << (p & 31), (unsigned)p < (unsigned)M.pt_hi);
    }
  }
  __syncthreads();
  // d. the set bits in ascending order; what does not fit is only counted
  NbhSets S;
  int n_map = 0;
  for (int base = 0; base < n_words; base += MB_THREADS) {      // block-uniform trip count
    const int w = base + tid;
    uint32_t bits = w < n_words ? __hip_atomic_load(&mark[w], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0u;
    int tot;
    int pos = id_off + n_map + block_excl_scan(__popc(bits), s_w, tot);
    while (bits) {
      const int bit = __ffs((int)bits) - 1;
      bits &= bits - 1;
      if (pos < cap) ids_row[pos] = (w << 5) + bit;
      ++pos;
    }
    n_map += tot;
  }
  S.n_map = n_map;
  S.over_points = id_off + n_map > cap;
  __syncthreads();
  // e. their anchors (:374-384), and how many of them the stream holds no slot for
  int c = 0;
  if (!S.over_points)
    for (int i = tid; i < n_map; i += MB_THREADS) {
      const int a = M.pt[ids_row[id_off + i]].kf_index;
      if ((unsigned)a < (unsigned)MAP_MAX_KF) atomicOr(&s_anch[a >> 5], 1u << (a & 31));
      if ((unsigned)a >= (unsigned)MAP_MAX_KF || s_slot[a] < 0) ++c;
    }
  (void)block_excl_scan(c, s_w, S.n_no_slot);                    // (its barriers also complete s_anch)
  // f. the anchors that are not among the given vertices, ascending
  S.extra = s_anch[tid] & ~s_vert[tid];
  S.rank = block_excl_scan(__popc(S.extra), s_w, S.n_extra);
  return S;
}

__global__ __launch_bounds__(MB_THREADS) void map_nbh_kernel(MapK M, MapNbhDst D) {
  __shared__ uint32_t s_vert[MAP_KF_WORDS], s_anch[MAP_KF_WORDS];
  __shared__ int16_t s_slot[MAP_MAX_KF];                           // -1: no slot of the stream holds the keyframe
  __shared__ int s_w[MB_THREADS / 64];
  const int r = blockIdx.x, tid = threadIdx.x;
  const nbh_req &Q = D.req[r];
  const int b = Q.stream, n_vertex = Q.n_vertex, n_head = Q.n_head, G = Q.n_groups, MP = D.max_points, K = D.max_keyframes;
  const int32_t *vertex = D.ids + Q.vertex_off, *slot_kf = D.ids + Q.slot_off;
  int32_t *point_id = D.point_id + (size_t)r * MP;
  const NbhSets S = nbh_collect(M, M.mark + (size_t)r * M.mark_b, point_id, n_head, MP, vertex, n_vertex, slot_kf, K, s_vert, s_anch, s_slot, s_w);
  const int n_map = S.n_map, total = n_head + n_map, n_no_slot = S.n_no_slot, rank = S.rank;
  const bool over_points = S.over_points;
  uint32_t extra = S.extra;
  // f. the vertex set: the given ids, behind them the anchors that are not among them, ascending
  const int n_vert = over_points ? 0 : n_vertex + S.n_extra;
  if (over_points || n_vert > D.VB) {                            // block-uniform: nothing of the stream has been touched
    if (tid == 0) {
      svs_nbh_result R{};
      R.n_points = total; R.n_map_points = n_map; R.n_vertex = n_vert; R.n_no_slot = n_no_slot; R.over_capacity = 1;
      D.res[r] = R;
    }
    return;
  }
  // g. the stream's list: the head as it was staged, the map's records (four 16-byte loads each) with the anchor's slot, 0xff up to the previous length
  svs_candidate_point *pts = D.pts + (size_t)b * MP;
  int4 *d4 = reinterpret_cast<int4 *>(pts);
  const svs_candidate_point *head = D.head + Q.head_off;
  const int4 *h4 = reinterpret_cast<const int4 *>(head);
  for (int i = tid; i < n_head * 4; i += MB_THREADS) d4[i] = h4[i];
  for (int i = tid; i < n_map; i += MB_THREADS) {
    const int4 *s4 = reinterpret_cast<const int4 *>(M.pt + point_id[n_head + i]);
    int4 q = s4[3];                                              // anchor_level, the anchor's id, point_id, pad_
    q.y = (unsigned)q.y < (unsigned)MAP_MAX_KF ? (int)s_slot[q.y] : -1;
    int4 *o4 = d4 + (size_t)(n_head + i) * 4;
    o4[0] = s4[0]; o4[1] = s4[1]; o4[2] = s4[2]; o4[3] = q;
  }
  for (int i = total * 4 + tid; i < Q.prev_len * 4; i += MB_THREADS) d4[i] = make_int4(-1, -1, -1, -1);
  for (int i = tid; i < n_head; i += MB_THREADS) point_id[i] = head[i].point_id;
  for (int i = total + tid; i < MP; i += MB_THREADS) point_id[i] = -1;
  if (tid < NBH_MAX_GROUPS) D.group_end[(size_t)b * NBH_MAX_GROUPS + tid] = tid < G - 1 ? Q.group_end[tid] : tid == G - 1 ? total : 0;
  if (tid == 0) { D.n_groups[b] = G; D.n_new[b] = n_head; }
  // h. the vertex set with the poses the map stores
  int32_t *vid = D.vertex_id + (size_t)r * D.VB;
  double *vT = D.vertex_T + (size_t)r * D.VB * 12;
  for (int i = tid; i < n_vertex * 12; i += MB_THREADS) {
    const int v = i / 12, k = i % 12, id = vertex[v];
    vT[i] = M.kf[id].T_anchor_from_w[k];
    if (k == 0) vid[v] = id;
  }
  for (int e = n_vertex + rank; extra; ++e) {                    // e < n_vert <= VB
    const int id = (tid << 5) + __ffs((int)extra) - 1;
    extra &= extra - 1;
    vid[e] = id;
    for (int k = 0; k < 12; ++k) vT[(size_t)e * 12 + k] = M.kf[id].T_anchor_from_w[k];
  }
  for (int i = n_vert * 12 + tid; i < D.VB * 12; i += MB_THREADS) {
    vT[i] = 0.0;
    if (i % 12 == 0) vid[i / 12] = -1;
  }
  // i. the slots that hold a keyframe of the map take its pose (the pyramid pointers and strides stay)
  svs_keyframe *kfs = D.kfs + (size_t)b * K;
  double *sT = D.slot_T + (size_t)r * K * 12;
  for (int i = tid; i < K * 12; i += MB_THREADS) {
    const int s = i / 12, k = i % 12, id = slot_kf[s];
    double v = 0.0;
    if (D.refresh && (unsigned)id < (unsigned)MAP_MAX_KF) { v = M.kf[id].T_anchor_from_w[k]; kfs[s].T_anchor_from_w[k] = v; }
    sT[i] = v;
  }
  if (tid == 0) {
    svs_nbh_result R{};
    R.n_points = total; R.n_map_points = n_map; R.n_vertex = n_vert; R.n_no_slot = n_no_slot; R.over_capacity = 0;
    D.res[r] = R;
  }
}

// ---- the double window's BA problem (ba_map.h): computeActivePointsAndExtendOuterWindow (slam_graph.cpp:599-663) as set operations ----------------------------
// lane i moves staged record i of svs_map_add_measured_observations to the tail of the measured store (four 16-byte loads) and its (point, keyframe) to the log's
__global__ __launch_bounds__(256) void map_append_meas_kernel(const svs_ba_edge *__restrict__ up, int n, int2 *__restrict__ log_tail, svs_ba_edge *__restrict__ store_tail) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int4 *s4 = reinterpret_cast<const int4 *>(up + i);
  int4 *d4 = reinterpret_cast<int4 *>(store_tail + i);
  const int4 q = s4[3];                // point, pose, anchor, pad_
  d4[0] = s4[0]; d4[1] = s4[1]; d4[2] = s4[2]; d4[3] = q;
  log_tail[i] = make_int2(q.x, q.y);
}

constexpr int MAP_WIN_MAX = 256;       // the solve's limit (ba.hip: SOLVE_MAX_P)
struct MapWinK {
  const int32_t *ids, *types, *pairs, *inner; int n0, n_pairs, window_cap, set_flags;      // staged: W0, the pairs, the INNER keyframes of W0
  uint32_t *active, *ext;              // bitmaps over point ids (the walk's row 0 of M.mark) / keyframe ids; zero before the first launch
  svs_map_window_result *res;          // zero before the first launch
  int32_t *wid, *wtype;                // [MAP_WIN_MAX] the final window
  int32_t *lids, *aids; double *poses, *psi;      // active ids | anchor ids | poses | psi
};

// one workgroup per INNER keyframe F of W0 (:611-646): W0 and F's graph neighbours are LDS bitmaps, F's feature_table row marks the active points and the extension
__global__ __launch_bounds__(MB_THREADS) void map_win_mark_kernel(MapK M, MapWinK A) {
  __shared__ uint32_t s_w0[MAP_KF_WORDS], s_nb[MAP_KF_WORDS];
  const int tid = threadIdx.x, F = A.inner[blockIdx.x];
  s_w0[tid] = 0; s_nb[tid] = 0;
  __syncthreads();
  // (ids the host has checked: in the map, so below kf_hi <= MAP_MAX_KF)
  for (int i = tid; i < A.n0; i += MB_THREADS) { const int id = A.ids[i]; atomicOr(&s_w0[id >> 5], 1u << (id & 31)); }
  for (int i = tid; i < A.n_pairs; i += MB_THREADS) {          // orderd_find is symmetric
    const int a = A.pairs[2 * i], b = A.pairs[2 * i + 1];
    if (a == F) atomicOr(&s_nb[b >> 5], 1u << (b & 31));
    if (b == F) atomicOr(&s_nb[a >> 5], 1u << (a & 31));
  }
  __syncthreads();
  const int e1 = M.kf_begin[F + 1];
  for (int e0 = M.kf_begin[F]; e0 < e1; e0 += MB_THREADS) {    // block-uniform
    const int e = e0 + tid;
    const int p = e < e1 ? M.kf_rows[e] : -1;
    const bool have = (unsigned)p < (unsigned)M.pt_hi;
    const int a = have ? M.pt[p].kf_index : -1;                // the anchor's id
    const bool a_ok = (unsigned)a < (unsigned)MAP_MAX_KF;
    const bool in_w0 = a_ok && bit_of(s_w0, a);
    const bool act = a_ok && (in_w0 || bit_of(s_nb, a));       // (:627, :636)
    wave_or_by_word(A.active, p >> 5, 1u << (p & 31), act);
    wave_or_by_word(A.ext, a >> 5, 1u << (a & 31), act && !in_w0);
  }
}

// both bitmaps to ascending ids by popcount prefixes; workgroup b owns the words [b * MB_THREADS, (b + 1) * MB_THREADS) of the active bitmap, workgroup 0 also
// the window's rows, poses, flags and the result.  Every workgroup finds the final window's size itself: over window_cap nothing is written but the result
__global__ __launch_bounds__(MB_THREADS) void map_win_list_kernel(MapK M, MapWinK A) {
  __shared__ uint32_t s_w0[MAP_KF_WORDS];
  __shared__ int s_w[MB_THREADS / 64];
  const int tid = threadIdx.x;
  const uint32_t ext = A.ext[tid];
  int n_ext;
  const int ext_rank = block_excl_scan(__popc(ext), s_w, n_ext);
  const int n_window = A.n0 + n_ext;
  if (n_window > A.window_cap) {                               // block-uniform
    if (blockIdx.x == 0 && tid == 0) { svs_map_window_result R; R.n_window = n_window; R.n_initial = A.n0; R.n_active = -1; R.n_edges_bound = 0; *A.res = R; }
    return;
  }
  const int n_words = (M.pt_hi + 31) >> 5, w_first = blockIdx.x * MB_THREADS;
  int before = 0, all = 0;
  for (int w = tid; w < n_words; w += MB_THREADS) { const int c = __popc(A.active[w]); all += c; if (w < w_first) before += c; }
  int n_before, n_active;
  (void)block_excl_scan(before, s_w, n_before);
  (void)block_excl_scan(all, s_w, n_active);
  const int w = w_first + tid;
  uint32_t bits = w < n_words ? A.active[w] : 0u;
  int tot, bound = 0;
  int pos = n_before + block_excl_scan(__popc(bits), s_w, tot);
  while (bits) {                                               // pos < n_active <= the points of the map
    const int p = (w << 5) + __ffs((int)bits) - 1;
    bits &= bits - 1;
    const svs_candidate_point &q = M.pt[p];
    const double x = q.xyz_anchor[0], y = q.xyz_anchor[1], z = q.xyz_anchor[2];
    A.lids[pos] = p; A.aids[pos] = q.kf_index;
    A.psi[3 * (size_t)pos] = x / z; A.psi[3 * (size_t)pos + 1] = y / z; A.psi[3 * (size_t)pos + 2] = 1.0 / z;      // invert_depth (maths_utils.h:66-69)
    bound += M.pt_begin[p + 1] - M.pt_begin[p];
    ++pos;
  }
  int bound_all;
  (void)block_excl_scan(bound, s_w, bound_all);
  if (tid == 0 && bound_all) atomicAdd(&A.res->n_edges_bound, bound_all);      // a sum of integers: no order in it
  if (blockIdx.x != 0) return;
  // the final window: W0 as given, the extension ascending and OUTER
  for (int i = tid; i < A.n0; i += MB_THREADS) { A.wid[i] = A.ids[i]; A.wtype[i] = A.types[i]; }
  {
    uint32_t b = ext;
    for (int e = A.n0 + ext_rank; b; ++e) { A.wid[e] = (tid << 5) + __ffs((int)b) - 1; A.wtype[e] = 1; b &= b - 1; }
  }
  for (int i = n_window + tid; i < MAP_WIN_MAX; i += MB_THREADS) { A.wid[i] = -1; A.wtype[i] = -1; }
  __syncthreads();
  for (int i = tid; i < n_window * 12; i += MB_THREADS) A.poses[i] = M.kf[A.wid[i / 12]].T_anchor_from_w[i % 12];
  if (A.set_flags) {                                           // exactly the final window, as map_window_kernel's two launches leave it
    s_w0[tid] = 0;
    __syncthreads();
    for (int i = tid; i < A.n0; i += MB_THREADS) { const int id = A.ids[i]; atomicOr(&s_w0[id >> 5], 1u << (id & 31)); }
    __syncthreads();
    s_w0[tid] |= ext;
    __syncthreads();
    for (int i = tid; i < M.kf_hi; i += MB_THREADS) M.kf_flags[i] = bit_of(s_w0, i) ? SVS_REG_KF_IN_WINDOW : 0;
  }
  if (tid == 0) { A.res->n_window = n_window; A.res->n_initial = A.n0; A.res->n_active = n_active; }
}

// what svs_ba_window_from_map reads at its moment: the window's poses and psi again
__global__ __launch_bounds__(256) void map_win_gather_kernel(MapK M, MapWinK A, int P, int L) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < 12 * P) A.poses[i] = M.kf[A.wid[i / 12]].T_anchor_from_w[i % 12];
  if (i < L) {
    const svs_candidate_point &q = M.pt[A.lids[i]];
    const double x = q.xyz_anchor[0], y = q.xyz_anchor[1], z = q.xyz_anchor[2];
    A.psi[3 * (size_t)i] = x / z; A.psi[3 * (size_t)i + 1] = y / z; A.psi[3 * (size_t)i + 2] = 1.0 / z;
  }
}

// restoreDataFromG2o (:1035-1058): poses by the window's ids, xyz_anchor = invert_depth(psi) by the active ids
__global__ __launch_bounds__(256) void map_win_store_kernel(MapK M, MapWinK A, int P, int L, const double *__restrict__ poses, const double *__restrict__ psi) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < 12 * P) M.kf[A.wid[i / 12]].T_anchor_from_w[i % 12] = poses[i];
  if (i < L) {
    const double u = psi[3 * (size_t)i], v = psi[3 * (size_t)i + 1], q = psi[3 * (size_t)i + 2];
    double *xyz = M.pt[A.lids[i]].xyz_anchor;
    xyz[0] = u / q; xyz[1] = v / q; xyz[2] = 1.0 / q;
  }
}

// ---- the pose graph's edges (EdgeTable, slam_graph.hpp:197-363): one 408-byte record per slot, 51 eight-byte words -----------------------------------------------
constexpr int EDGE_WORDS = sizeof(svs_map_edge) / 8;
static_assert(sizeof(svs_map_edge) == 408 && sizeof(svs_ba_constraint) == 392 && sizeof(svs_map_constraint_result) == 416, "record copies below");
struct edge_up { int32_t slot, lo, hi, strength, type, pad_; };

// insertEdge: 64 lanes per staged record; T and info zero, not marginalised
__global__ __launch_bounds__(256) void map_edge_add_kernel(svs_map_edge *__restrict__ E, const edge_up *__restrict__ up, int n) {
  const int i = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (i >= n || lane >= EDGE_WORDS) return;
  const edge_up u = up[i];
  int2 w = make_int2(0, 0);
  if (lane == 0) w = make_int2(u.lo, u.hi);
  if (lane == 1) w = make_int2(u.strength, u.type);
  reinterpret_cast<int2 *>(E + u.slot)[lane] = w;
}

// setConstraint with the caller's values: 64 lanes per record.  slot_inv[i] = (slot, T_21 has to be inverted to become T_lo_from_hi)
__global__ __launch_bounds__(256) void map_edge_set_kernel(svs_map_edge *__restrict__ E, const svs_ba_constraint *__restrict__ up, const int2 *__restrict__ slot_inv, int n) {
  const int i = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (i >= n) return;
  const int2 si = slot_inv[i];
  svs_map_edge &e = E[si.x];
  if (lane < 36) e.info[lane] = up[i].info[lane];
  if (lane == 36) {
    double T[12];
#pragma unroll
    for (int k = 0; k < 12; ++k) T[k] = up[i].T_21[k];
    if (si.y) pose_inv(T, T);
#pragma unroll
    for (int k = 0; k < 12; ++k) e.T_lo_from_hi[k] = T[k];
    e.is_marginalized = 1;
  }
}

__global__ __launch_bounds__(256) void map_edge_unmarg_kernel(svs_map_edge *__restrict__ E, const int32_t *__restrict__ slots, int n) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < n) E[slots[i]].is_marginalized = 0;
}

__global__ __launch_bounds__(256) void map_edge_get_kernel(const svs_map_edge *__restrict__ E, const int32_t *__restrict__ slots, int n, svs_map_edge *__restrict__ out) {
  const int i = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (i >= n || lane >= EDGE_WORDS) return;
  reinterpret_cast<long long *>(out + i)[lane] = reinterpret_cast<const long long *>(E + slots[i])[lane];
}

// copyContraintsToG2o's records for the optimizer (ba_map.h): 64 lanes per list entry (i, j, slot, invert)
__global__ __launch_bounds__(256) void map_edge_gather_kernel(const svs_map_edge *__restrict__ E, const int4 *__restrict__ list, int n, svs_ba_constraint *__restrict__ out) {
  const int i = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (i >= n) return;
  const int4 q = list[i];
  const svs_map_edge &e = E[q.z];
  if (lane < 36) out[i].info[lane] = e.info[lane];
  if (lane == 36) {
    double T[12];
#pragma unroll
    for (int k = 0; k < 12; ++k) T[k] = e.T_lo_from_hi[k];
    if (q.w) pose_inv(T, T);
#pragma unroll
    for (int k = 0; k < 12; ++k) out[i].T_21[k] = T[k];
    out[i].pose1 = q.x; out[i].pose2 = q.y;
  }
}

// ---- computeConstraint (slam_graph.cpp:787-846) for a batch of keyframe pairs: one workgroup per request --------------------------------------------------------
// The common points are a bitmap in the request's row of M.mark (kf1's feature_table row is walked, kf2 searched in each point's sorted observer row), turned into
// ascending ids by popcount prefixes; a lane then owns whole points -- record, anchor pose, arithmetic -- and leaves the depth in the request's scratch row.  The
// median is a radix select over the depths' bit patterns (non-negative doubles order as their bits), eight passes of eight bits with LDS histograms that re-read
// the scratch row: both middle ranks are followed at once, nothing is sorted, and the row may be of any length.  No atomic decides a value or an order.
struct cons_req {
  int32_t kf1, kf2, slot, slot_inv;    // slot < 0: do not store; slot_inv: T_12 is the inverse of T_lo_from_hi (kf1 > kf2)
  int32_t n_override, override_id[2], n_cached;
  int32_t cached_off, pad_;            // into the staged cached ids / poses
  long long row_off;                   // into the scratch rows (depths, common point ids)
  double override_T[2][12];
};
static_assert(sizeof(cons_req) % 8 == 0, "staged as an array");
struct MapConsK {
  const cons_req *req; const int32_t *cached_ids; const double *cached_T;
  svs_map_constraint_result *res; int32_t *missing; int missing_cap;
  double *depth; int32_t *common; svs_map_edge *edges;
};
constexpr int CONS_UNROLL = 4;         // points of a lane whose loads are requested together

// the request's pose of keyframe `id`: an override, else the map's
__device__ __forceinline__ const double *cons_pose_of(const MapK &M, const cons_req &Q, int id) {
  if (Q.n_override > 0 && id == Q.override_id[0]) return Q.override_T[0];
  if (Q.n_override > 1 && id == Q.override_id[1]) return Q.override_T[1];
  return M.kf[id].T_anchor_from_w;
}

__global__ __launch_bounds__(MB_THREADS) void map_cons_kernel(MapK M, MapConsK A) {
  __shared__ uint32_t s_miss[MAP_KF_WORDS];
  __shared__ int s_hist[2 * 256];
  __shared__ int s_w[MB_THREADS / 64];
  __shared__ unsigned long long s_pref[2];
  __shared__ int s_rank[2];
  __shared__ double s_T[3][12];                                   // T1, T2, then T_12
  __shared__ double s_diag[2];
  const int r = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const cons_req &Q = A.req[r];
  const int kf1 = Q.kf1, kf2 = Q.kf2;
  uint32_t *mark = M.mark + (size_t)r * M.mark_b;
  double *depth = A.depth + Q.row_off;
  int32_t *common = A.common + Q.row_off;
  const int n_words = (M.pt_hi + 31) >> 5;                        // <= mark_b
  // a. empty sets; the two poses (ids the host has checked: in the map, so below kf_hi <= MAP_MAX_KF)
  s_miss[tid] = 0;
  for (int i = tid; i < n_words; i += MB_THREADS) mark[i] = 0;
  if (tid < 24) s_T[tid / 12][tid % 12] = cons_pose_of(M, Q, tid < 12 ? kf1 : kf2)[tid % 12];
  __syncthreads();
  // b. the common points: CONS_UNROLL entries of kf1's row per lane and step, their row bounds requested together, then the searches
  const int row_b = M.kf_begin[kf1], row_e = M.kf_begin[kf1 + 1];
  for (int e0 = row_b; e0 < row_e; e0 += MB_THREADS * CONS_UNROLL) {      // block-uniform
    int p[CONS_UNROLL], ob[CONS_UNROLL], oe[CONS_UNROLL];
#pragma unroll
    for (int k = 0; k < CONS_UNROLL; ++k) { const int e = e0 + k * MB_THREADS + tid; p[k] = e < row_e ? M.kf_rows[e] : -1; }
#pragma unroll
    for (int k = 0; k < CONS_UNROLL; ++k) {
      const bool have = (unsigned)p[k] < (unsigned)M.pt_hi;
      ob[k] = have ? M.pt_begin[p[k]] : 0; oe[k] = have ? M.pt_begin[p[k] + 1] : 0;
    }
#pragma unroll
    for (int k = 0; k < CONS_UNROLL; ++k) {
      bool found = false;
      for (int e = ob[k]; e < oe[k]; e += 4) {                     // four loads in flight, as map_build_kernel reads a row
        int kf[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) kf[q] = e + q < oe[k] ? M.pt_rows[e + q] : -1;
#pragma unroll
        for (int q = 0; q < 4; ++q) found |= kf[q] == kf2;
      }
      wave_or_by_word(mark, p[k] >> 5, 1u << (p[k] & 31), found);
    }
  }
  __syncthreads();
  // c. ascending ids
  int n = 0;
  for (int base = 0; base < n_words; base += MB_THREADS) {        // block-uniform trip count
    const int w = base + tid;
    uint32_t bits = w < n_words ? __hip_atomic_load(&mark[w], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0u;
    int tot;
    int pos = n + block_excl_scan(__popc(bits), s_w, tot);
    while (bits) {
      const int b = __ffs((int)bits) - 1;
      bits &= bits - 1;
      if (pos < row_e - row_b) common[pos] = (w << 5) + b;         // (always: the common points are entries of kf1's row)
      ++pos;
    }
    n += tot;
  }
  n = min(n, row_e - row_b);
  __syncthreads();
  // d. the depths: record, anchor, pose source and pose of CONS_UNROLL points requested before their arithmetic
  for (int i0 = 0; i0 < n; i0 += MB_THREADS * CONS_UNROLL) {
    int a[CONS_UNROLL];
    double x[CONS_UNROLL][3];
    const double *Ta[CONS_UNROLL];
#pragma unroll
    for (int k = 0; k < CONS_UNROLL; ++k) {
      const int i = i0 + k * MB_THREADS + tid;
      a[k] = -1;
      if (i < n) {
        const svs_candidate_point &q = M.pt[common[i]];
        x[k][0] = q.xyz_anchor[0]; x[k][1] = q.xyz_anchor[1]; x[k][2] = q.xyz_anchor[2];
        a[k] = q.kf_index;
      }
    }
#pragma unroll
    for (int k = 0; k < CONS_UNROLL; ++k) {
      Ta[k] = nullptr;
      if ((unsigned)a[k] >= (unsigned)MAP_MAX_KF) continue;
      if ((Q.n_override > 0 && a[k] == Q.override_id[0]) || (Q.n_override > 1 && a[k] == Q.override_id[1]) || (M.kf_flags[a[k]] & SVS_REG_KF_IN_WINDOW)) {
        Ta[k] = cons_pose_of(M, Q, a[k]);
      } else {
        int lo = 0, hi = Q.n_cached;                               // the cached list is ascending
        const int32_t *ids = A.cached_ids + Q.cached_off;
        while (lo < hi) { const int mid = (lo + hi) >> 1; if (ids[mid] < a[k]) lo = mid + 1; else hi = mid; }
        if (lo < Q.n_cached && ids[lo] == a[k]) Ta[k] = A.cached_T + 12 * (size_t)(Q.cached_off + lo);
        else atomicOr(&s_miss[a[k] >> 5], 1u << (a[k] & 31));
      }
    }
#pragma unroll
    for (int k = 0; k < CONS_UNROLL; ++k) {
      const int i = i0 + k * MB_THREADS + tid;
      if (i >= n) continue;
      double d = 0.0;
      if (Ta[k]) {
        double T[12], y[3], z[3];
#pragma unroll
        for (int q = 0; q < 12; ++q) T[q] = Ta[k][q];
        pose_inv(T, T);
        pose_act(T, x[k], y);
        pose_act(s_T[0], y, z);
        d = sqrt((z[0] * z[0] + z[1] * z[1]) + z[2] * z[2]);
      }
      depth[i] = d;
    }
  }
  // e. T_12 = T1 * inv(T2); the missing anchors, ascending
  if (tid == 0) {
    double Ti[12], T12[12];
    pose_inv(s_T[1], Ti);
    pose_mul(s_T[0], Ti, T12);
#pragma unroll
    for (int k = 0; k < 12; ++k) s_T[2][k] = T12[k];
  }
  __syncthreads();                                                 // (completes s_miss, the scratch row and s_T[2])
  svs_map_constraint_result &R = A.res[r];
  int32_t *missing = A.missing + (size_t)r * A.missing_cap;
  int n_missing;
  {
    uint32_t bits = s_miss[tid];
    int pos = block_excl_scan(__popc(bits), s_w, n_missing);
    while (bits) {
      if (pos < A.missing_cap) missing[pos] = (tid << 5) + __ffs((int)bits) - 1;
      bits &= bits - 1;
      ++pos;
    }
    for (int k = n_missing + tid; k < A.missing_cap; k += MB_THREADS) missing[k] = -1;
  }
  if (tid < 12) R.T_12[tid] = s_T[2][tid];
  if (n_missing > 0 || n == 0) {                                   // block-uniform
    if (tid < 36) R.info[tid] = 0.0;
    if (tid == 0) { R.status = n_missing > 0 ? SVS_CONS_MISSING_ANCHOR : SVS_CONS_EMPTY; R.strength = n; R.n_missing = n_missing; R.pad_ = 0; R.median = 0.0; R.norm_dist = 0.0; }
    return;
  }
  // f. the median (maths_utils.h:114-136): ranks (n - 1) / 2 and n / 2 of the multiset, one and the same for an odd count
  if (tid < 2) { s_pref[tid] = 0ull; s_rank[tid] = tid == 0 ? (n - 1) / 2 : n / 2; }
  __syncthreads();
  for (int shift = 56; shift >= 0; shift -= 8) {
    const unsigned long long pref0 = s_pref[0], pref1 = s_pref[1];
    const int my = tid >> 8, bin = tid & 255, rank = s_rank[my];
    s_hist[tid] = 0;
    __syncthreads();
    for (int i = tid; i < n; i += MB_THREADS) {
      const unsigned long long u = (unsigned long long)__double_as_longlong(depth[i]);
      const unsigned long long hi = shift == 56 ? 0ull : u >> (shift + 8);
      const int b = (int)(u >> shift) & 255;
      if (hi == pref0) atomicAdd(&s_hist[b], 1);
      if (hi == pref1) atomicAdd(&s_hist[256 + b], 1);
    }
    __syncthreads();
    const int v = s_hist[tid];
    const int inc = wave_incl_scan(v);
    if (lane == 63) s_w[wave] = inc;
    __syncthreads();
    int off = 0;
#pragma unroll
    for (int w = 0; w < MB_THREADS / 64; ++w) off += ((w >> 2) == my && w < wave) ? s_w[w] : 0;
    const int excl = off + inc - v;
    if (v > 0 && excl <= rank && rank < excl + v) {                // exactly one bin per rank
      s_pref[my] = ((my == 0 ? pref0 : pref1) << 8) | (unsigned long long)bin;
      s_rank[my] = rank - excl;
    }
    __syncthreads();
  }
  // g. norm_dist, Lambda; the record, and setConstraint where the request stores
  if (tid == 0) {
    const double lo = __longlong_as_double((long long)s_pref[0]), hi = __longlong_as_double((long long)s_pref[1]);
    double val = lo;
    if ((n & 1) == 0) { val += hi; val = 0.5 * val; }
    const double tx = s_T[2][3], ty = s_T[2][7], tz = s_T[2][11];
    const double norm_dist = sqrt((tx * tx + ty * ty) + tz * tz) / val;
    const double s = (double)n, v350 = (350 * 1.0) * norm_dist, v100 = 100 * 1.0;
    s_diag[0] = s * (v350 * v350); s_diag[1] = s * (v100 * v100);
    R.status = SVS_CONS_OK; R.strength = n; R.n_missing = 0; R.pad_ = 0; R.median = val; R.norm_dist = norm_dist;
  }
  __syncthreads();
  const double lam = tid < 36 ? (tid % 7 == 0 ? s_diag[tid >= 21 ? 1 : 0] : 0.0) : 0.0;
  if (tid < 36) R.info[tid] = lam;
  if (Q.slot >= 0) {
    svs_map_edge &E = A.edges[Q.slot];
    if (tid < 36) E.info[tid] = lam;
    if (tid == 36) {
      double T[12];
#pragma unroll
      for (int k = 0; k < 12; ++k) T[k] = s_T[2][k];
      if (Q.slot_inv) pose_inv(T, T);
#pragma unroll
      for (int k = 0; k < 12; ++k) E.T_lo_from_hi[k] = T[k];
      E.is_marginalized = 1;
    }
  }
}

#define MAP_CAPACITY(ctx, cond)                                                                   \
  do {                                                                                                    \
    if (!(cond)) {                                                                                        \
      char buf_[512];                                                                                     \
      snprintf(buf_, sizeof buf_, "%s:%d capacity exceeded: %s", __FILE__, __LINE__, #cond);              \
      (ctx)->err = buf_;                                                                                  \
      return SVS_ERR_CAPACITY;                                                                            \
    }                                                                                                     \
  } while (0)
}  // namespace

struct svs_map {
  svs_ctx *ctx = nullptr;
  int max_kf = 0, max_pt = 0, max_obs = 0;
  uint64_t serial = 0;                                      // of this map among all that were created (svs_reg_commit: is it the map of the last batch)
  // the host's share: the id sets, the frames (where FAST and the matcher read a root), the set of pairs
  std::vector<uint8_t> kf_in, pt_in;
  std::vector<MapRootView> kf_view;
  std::unordered_set<uint64_t> pairs;
  std::vector<uint32_t> stamp; uint32_t stamp_now = 0;      // "twice in one call", by keyframe or point id
  int n_kf = 0, n_pt = 0, n_obs = 0, kf_hi = 0, pt_hi = 0;
  int csr_n = 0;                                            // the log length the CSR views were built from
  // the device's
  DevBuf<svs_keyframe> d_kf; DevBuf<const float *> d_kf_disp; DevBuf<int32_t> d_kf_dstride, d_kf_thr; DevBuf<uint8_t> d_kf_flags;
  DevBuf<svs_candidate_point> d_pt;
  DevBuf<int2> d_log;
  DevBuf<int32_t> d_kf_begin, d_kf_rows, d_pt_begin, d_pt_rows, d_kf_cur, d_pt_cur;
  DevBuf<uint32_t> d_mark; size_t mark_b = 0; int mark_rows = 0;
  // staging of the updates: one pinned block and its device twin, reused once the upload out of the pinned block has happened
  PinnedBuf<uint8_t> h_up; DevBuf<uint8_t> d_up; owned::Event up_ev; bool up_pending = false;
  // the measured store (one svs_ba_edge per pair that came with a measurement, log order; allocated with the first of them) and the prepared window
  DevBuf<svs_ba_edge> d_meas; int n_meas = 0, n_unmeasured = 0;
  DevBuf<uint8_t> d_win; PinnedBuf<uint8_t> h_win;           // head (result | window ids | types) | extension bitmap | active ids | anchor ids | poses | psi
  bool win_valid = false; int win_P = 0, win_L = 0; uint64_t win_serial = 0;
  std::vector<int32_t> win_ids, win_types;
  // the pose graph's edges: the key set (lo << 32 | hi -> slot) and the is_marginalized flags here, the records on the device
  int max_edges = 0, n_edges = 0, n_marg = 0;
  std::unordered_map<uint64_t, int> edge_slot; std::vector<uint8_t> edge_marg;
  DevBuf<svs_map_edge> d_edges;
  // computeConstraint: the feature_table lengths (what a request's scratch row is sized by), the scratch rows, and the block the blocking calls download
  std::vector<int32_t> kf_nobs;
  DevBuf<double> d_depth; DevBuf<int32_t> d_common;
  DevBuf<uint8_t> d_dn; PinnedBuf<uint8_t> h_dn;
  // the pose graph's walks (map_walk.inc): the strength-ordered adjacency and the searches' work space
  MapWalkState walk;
  ~svs_map() {      // (before the members go, also when create gives up)
    if (ctx) { (void)hipSetDevice(ctx->device); (void)hipStreamSynchronize(ctx->stream); }
  }
  MapK view() const {
    MapK M{};
    M.kf = d_kf; M.kf_disp = d_kf_disp; M.kf_dstride = d_kf_dstride; M.kf_thr = d_kf_thr; M.kf_flags = d_kf_flags;
    M.pt = d_pt; M.log = d_log; M.n_log = n_obs;
    M.kf_begin = d_kf_begin; M.kf_rows = d_kf_rows; M.pt_begin = d_pt_begin; M.pt_rows = d_pt_rows; M.kf_cur = d_kf_cur; M.pt_cur = d_pt_cur;
    M.kf_hi = kf_hi; M.pt_hi = pt_hi;
    M.mark = d_mark; M.mark_b = mark_b;
    return M;
  }
  uint32_t next_stamp() {
    if (++stamp_now == 0) { std::fill(stamp.begin(), stamp.end(), 0u); stamp_now = 1; }
    return stamp_now;
  }
};

svs_ctx *svs_map_ctx(svs_map *map) { return map ? map->ctx : nullptr; }
uint64_t svs_map_serial(const svs_map *map) { return map ? map->serial : 0; }
bool svs_map_has_keyframe(const svs_map *map, int32_t id) { return map && id >= 0 && id < map->max_kf && map->kf_in[id]; }
void svs_map_root_view(const svs_map *map, int32_t id, MapRootView *out) { *out = map->kf_view[id]; }

extern "C" int svs_map_create(svs_ctx *ctx, int max_keyframes, int max_points, int max_observations, svs_map **out) {
  SVS_REQUIRE(ctx, ctx && out && max_keyframes >= 1 && max_points >= 1 && max_observations >= 1);
  if (max_keyframes > MAP_MAX_KF) { ctx->err = "svs_map_create: at most 16384 keyframes"; return SVS_ERR_UNSUPPORTED; }
  SVS_REQUIRE(ctx, max_points < (1 << 30) && max_observations < (1 << 30));
  SVS_DEVICE(ctx);
  std::unique_ptr<svs_map> m(new svs_map());
  m->ctx = ctx; m->max_kf = max_keyframes; m->max_pt = max_points; m->max_obs = max_observations;
  { static uint64_t made = 0; m->serial = __atomic_add_fetch(&made, 1, __ATOMIC_RELAXED); }
  m->kf_in.assign(max_keyframes, 0); m->pt_in.assign(max_points, 0);
  m->kf_view.resize(max_keyframes);
  m->kf_nobs.assign(max_keyframes, 0);
  m->stamp.assign(std::max(max_keyframes, max_points), 0u);
  const size_t K = (size_t)max_keyframes, P = (size_t)max_points, O = (size_t)max_observations;
  SVS_HIP(ctx, m->d_kf.alloc(K));
  SVS_HIP(ctx, m->d_kf_disp.alloc(K));
  SVS_HIP(ctx, m->d_kf_dstride.alloc(K));
  SVS_HIP(ctx, m->d_kf_thr.alloc(K * THR_N));
  SVS_HIP(ctx, m->d_kf_flags.alloc(K));
  SVS_HIP(ctx, m->d_pt.alloc(P));
  SVS_HIP(ctx, m->d_log.alloc(O));
  SVS_HIP(ctx, m->d_kf_begin.alloc(K + 1));
  SVS_HIP(ctx, m->d_kf_cur.alloc(K + 1));
  SVS_HIP(ctx, m->d_pt_begin.alloc(P + 1));
  SVS_HIP(ctx, m->d_pt_cur.alloc(P + 1));
  SVS_HIP(ctx, m->d_kf_rows.alloc(O));
  SVS_HIP(ctx, m->d_pt_rows.alloc(O));
  SVS_HIP(ctx, m->up_ev.create(hipEventDisableTiming));
  m->mark_b = (P + 31) / 32;
  // empty CSR views: a request on a map without observations reads them
  SVS_HIP(ctx, hipMemsetAsync(m->d_kf_begin, 0, (K + 1) * sizeof(int32_t), ctx->stream));
  SVS_HIP(ctx, hipMemsetAsync(m->d_pt_begin, 0, (P + 1) * sizeof(int32_t), ctx->stream));
  SVS_HIP(ctx, hipMemsetAsync(m->d_kf_flags, 0, K, ctx->stream));
  *out = m.release();
  return SVS_OK;
}

extern "C" int svs_map_destroy(svs_map *map) {
  if (!map) return SVS_OK;
  delete map;
  return SVS_OK;
}

extern "C" int svs_map_info(svs_map *map, int32_t *n_keyframes, int32_t *n_points, int32_t *n_observations) {
  if (!map) return SVS_ERR_INVALID;
  if (n_keyframes) *n_keyframes = map->n_kf;
  if (n_points) *n_points = map->n_pt;
  if (n_observations) *n_observations = map->n_obs;
  return SVS_OK;
}

// the pinned block, free to be written: the upload out of it that is still in flight has happened, and it holds `bytes`
static int map_stage(svs_map *m, size_t bytes, uint8_t **out) {
  svs_ctx *ctx = m->ctx;
  if (m->up_pending) { SVS_HIP(ctx, hipEventSynchronize(m->up_ev)); m->up_pending = false; }
  if (m->h_up.bytes() < bytes) {
    // the device twin may still be read by the scatter of the last update
    SVS_HIP(ctx, hipStreamSynchronize(ctx->stream));
    const size_t want = std::max(bytes * 2, (size_t)1 << 16);
    SVS_HIP(ctx, m->h_up.alloc(want));
    SVS_HIP(ctx, m->d_up.alloc(want));
  }
  *out = m->h_up;
  return SVS_OK;
}
static int map_upload(svs_map *m, void *d_dst, size_t bytes) {
  svs_ctx *ctx = m->ctx;
  SVS_HIP(ctx, hipMemcpyAsync(d_dst, m->h_up, bytes, hipMemcpyHostToDevice, ctx->stream));
  SVS_HIP(ctx, hipEventRecord(m->up_ev, ctx->stream));
  m->up_pending = true;
  return SVS_OK;
}
static size_t up_align(size_t v) { return (v + 15) & ~(size_t)15; }

// n ids, each below `cap`, each `present` in `in`, none twice
static int map_check_ids(svs_map *m, int n, const int32_t *ids, const std::vector<uint8_t> &in, int cap, bool present) {
  svs_ctx *ctx = m->ctx;
  const uint32_t st = m->next_stamp();
  for (int i = 0; i < n; ++i) {
    const int32_t id = ids[i];
    if (present) SVS_REQUIRE(ctx, id >= 0 && id < cap && in[id]);
    else { SVS_REQUIRE(ctx, id >= 0); MAP_CAPACITY(ctx, id < cap); SVS_REQUIRE(ctx, !in[id]); }
    SVS_REQUIRE(ctx, m->stamp[id] != st);
    m->stamp[id] = st;
  }
  return SVS_OK;
}

extern "C" int svs_map_add_keyframes(svs_map *m, int n, const int32_t *h_ids, const svs_keyframe *h_keyframes, const float *const *h_disp_ptr,
                                     const int32_t *h_disp_stride, const int32_t *h_fast_thr) {
  svs_ctx *ctx = m ? m->ctx : nullptr;
  SVS_REQUIRE(ctx, m && n >= 0 && (n == 0 || (h_ids && h_keyframes && h_disp_ptr && h_disp_stride && h_fast_thr)));
  if (n == 0) return SVS_OK;
  if (int rc = map_check_ids(m, n, h_ids, m->kf_in, m->max_kf, false)) return rc;
  for (int i = 0; i < n; ++i) {
    SVS_REQUIRE(ctx, h_disp_ptr[i] && h_disp_stride[i] > 0);
    for (int l = 0; l < SVS_NUM_PYR_LEVELS; ++l) SVS_REQUIRE(ctx, h_keyframes[i].pyr[l] && h_keyframes[i].stride[l] > 0);
    for (int k = 0; k < THR_N; ++k) SVS_REQUIRE(ctx, h_fast_thr[(size_t)i * THR_N + k] >= 10 && h_fast_thr[(size_t)i * THR_N + k] <= 255);
  }
  SVS_DEVICE(ctx);
  uint8_t *hs;
  if (int rc = map_stage(m, (size_t)n * sizeof(kf_up), &hs)) return rc;
  kf_up *up = reinterpret_cast<kf_up *>(hs);
  for (int i = 0; i < n; ++i) {
    up[i].id = h_ids[i]; up[i].disp_stride = h_disp_stride[i]; up[i].disp = h_disp_ptr[i]; up[i].kf = h_keyframes[i]; up[i].kf.pad_ = 0;
    memcpy(up[i].thr, h_fast_thr + (size_t)i * THR_N, sizeof up[i].thr);
  }
  if (int rc = map_upload(m, m->d_up, (size_t)n * sizeof(kf_up))) return rc;
  hipLaunchKernelGGL(map_scatter_kf_kernel, dim3(div_up(n, 4)), dim3(256), 0, ctx->stream, m->view(), reinterpret_cast<const kf_up *>(m->d_up.get()), n);
  SVS_LAUNCH_CHECK(ctx);
  for (int i = 0; i < n; ++i) {
    const int id = h_ids[i];
    m->kf_in[id] = 1;
    MapRootView &v = m->kf_view[id];
    for (int l = 0; l < SVS_NUM_PYR_LEVELS; ++l) { v.pyr[l] = h_keyframes[i].pyr[l]; v.stride[l] = h_keyframes[i].stride[l]; }
    v.disp = h_disp_ptr[i]; v.disp_stride = h_disp_stride[i];
    m->kf_hi = std::max(m->kf_hi, id + 1);
  }
  m->n_kf += n;
  return SVS_OK;
}

extern "C" int svs_map_add_points(svs_map *m, int n, const int32_t *h_ids, const svs_candidate_point *h_points) {
  svs_ctx *ctx = m ? m->ctx : nullptr;
  SVS_REQUIRE(ctx, m && n >= 0 && (n == 0 || (h_ids && h_points)));
  if (n == 0) return SVS_OK;
  if (int rc = map_check_ids(m, n, h_ids, m->pt_in, m->max_pt, false)) return rc;
  for (int i = 0; i < n; ++i) SVS_REQUIRE(ctx, svs_map_has_keyframe(m, h_points[i].kf_index));
  SVS_DEVICE(ctx);
  const size_t o_pts = up_align((size_t)n * sizeof(int32_t)), bytes = o_pts + (size_t)n * sizeof(svs_candidate_point);
  uint8_t *hs;
  if (int rc = map_stage(m, bytes, &hs)) return rc;
  memcpy(hs, h_ids, (size_t)n * sizeof(int32_t));
  memcpy(hs + o_pts, h_points, (size_t)n * sizeof(svs_candidate_point));
  if (int rc = map_upload(m, m->d_up, bytes)) return rc;
  hipLaunchKernelGGL(map_scatter_pt_kernel, dim3(div_up(n, 256)), dim3(256), 0, ctx->stream, m->view(), reinterpret_cast<const int32_t *>(m->d_up.get()),
                     reinterpret_cast<const svs_candidate_point *>(m->d_up.get() + o_pts), n);
  SVS_LAUNCH_CHECK(ctx);
  for (int i = 0; i < n; ++i) { m->pt_in[h_ids[i]] = 1; m->pt_hi = std::max(m->pt_hi, h_ids[i] + 1); }
  m->n_pt += n;
  m->win_valid = false;                // (the prepared window's lists are sized by the points it saw)
  return SVS_OK;
}

// h_center == nullptr: svs_map_add_observations; else the pairs come with their measurements (h_level checked by the caller)
static int map_add_observations(svs_map *m, int n, const int32_t *h_point_ids, const int32_t *h_kf_ids, const double *h_center, const int32_t *h_level) {
  svs_ctx *ctx = m->ctx;
  for (int i = 0; i < n; ++i) SVS_REQUIRE(ctx, h_point_ids[i] >= 0 && h_point_ids[i] < m->max_pt && m->pt_in[h_point_ids[i]] && svs_map_has_keyframe(m, h_kf_ids[i]));
  // the pairs that are new, each once, in the caller's order
  std::vector<int2> fresh;
  std::vector<int> from;
  std::unordered_set<uint64_t> seen;
  for (int i = 0; i < n; ++i) {
    const uint64_t key = ((uint64_t)(uint32_t)h_point_ids[i] << 32) | (uint32_t)h_kf_ids[i];
    if (m->pairs.count(key) || !seen.insert(key).second) continue;
    fresh.push_back(make_int2(h_point_ids[i], h_kf_ids[i]));
    if (h_center) from.push_back(i);
  }
  MAP_CAPACITY(ctx, (size_t)m->n_obs + fresh.size() <= (size_t)m->max_obs);
  if (fresh.empty()) return SVS_OK;
  SVS_DEVICE(ctx);
  const int nf = (int)fresh.size();
  uint8_t *hs;
  if (!h_center) {
    if (int rc = map_stage(m, fresh.size() * sizeof(int2), &hs)) return rc;
    memcpy(hs, fresh.data(), fresh.size() * sizeof(int2));
    if (int rc = map_upload(m, m->d_log.get() + m->n_obs, fresh.size() * sizeof(int2))) return rc;      // straight to the log's tail
    m->n_unmeasured += nf;
  } else {
    if (!m->d_meas) SVS_HIP(ctx, m->d_meas.alloc((size_t)m->max_obs));
    if (int rc = map_stage(m, fresh.size() * sizeof(svs_ba_edge), &hs)) return rc;
    svs_ba_edge *up = reinterpret_cast<svs_ba_edge *>(hs);
    for (int k = 0; k < nf; ++k) {
      const int i = from[k];
      const double s = 1.0 / (double)(1 << h_level[i]);                                                 // pyrFromZero_d(1., level) (slam_graph.cpp:1012)
      svs_ba_edge e;
      for (int c = 0; c < 3; ++c) e.obs[c] = h_center[(size_t)i * 3 + c];
      e.info[0] = s * s; e.info[1] = s * s; e.info[2] = 0.333 * 0.333;
      e.point = fresh[k].x; e.pose = fresh[k].y; e.anchor = 0; e.pad_ = 0;
      up[k] = e;
    }
    if (int rc = map_upload(m, m->d_up, fresh.size() * sizeof(svs_ba_edge))) return rc;
    hipLaunchKernelGGL(map_append_meas_kernel, dim3(div_up(nf, 256)), dim3(256), 0, ctx->stream, reinterpret_cast<const svs_ba_edge *>(m->d_up.get()), nf,
                       m->d_log.get() + m->n_obs, m->d_meas.get() + m->n_meas);
    SVS_LAUNCH_CHECK(ctx);
    m->n_meas += nf;
  }
  for (const int2 &o : fresh) { m->pairs.insert(((uint64_t)(uint32_t)o.x << 32) | (uint32_t)o.y); ++m->kf_nobs[o.y]; }
  m->n_obs += nf;
  m->win_valid = false;                // the prepared window was one of the map without these pairs
  return SVS_OK;
}

extern "C" int svs_map_add_observations(svs_map *m, int n, const int32_t *h_point_ids, const int32_t *h_kf_ids) {
  svs_ctx *ctx = m ? m->ctx : nullptr;
  SVS_REQUIRE(ctx, m && n >= 0 && (n == 0 || (h_point_ids && h_kf_ids)));
  if (n == 0) return SVS_OK;
  return map_add_observations(m, n, h_point_ids, h_kf_ids, nullptr, nullptr);
}

extern "C" int svs_map_add_measured_observations(svs_map *m, int n, const int32_t *h_point_ids, const int32_t *h_kf_ids, const double *h_center,
                                                 const int32_t *h_level) {
  svs_ctx *ctx = m ? m->ctx : nullptr;
  SVS_REQUIRE(ctx, m && n >= 0 && (n == 0 || (h_point_ids && h_kf_ids && h_center && h_level)));
  if (n == 0) return SVS_OK;
  for (int i = 0; i < n; ++i) SVS_REQUIRE(ctx, h_level[i] >= 0 && h_level[i] < SVS_NUM_PYR_LEVELS);
  return map_add_observations(m, n, h_point_ids, h_kf_ids, h_center, h_level);
}

extern "C" int svs_map_measured_info(svs_map *map, int32_t *n_measured, int32_t *n_unmeasured) {
  if (!map) return SVS_ERR_INVALID;
  if (n_measured) *n_measured = map->n_meas;
  if (n_unmeasured) *n_unmeasured = map->n_unmeasured;
  return SVS_OK;
}

// ids [n] and n rows of `row` doubles, scattered by `kernel`
template <class Kernel>
static int map_set_rows(svs_map *m, int n, const int32_t *ids, const double *rows, int row, Kernel kernel) {
  svs_ctx *ctx = m->ctx;
  SVS_DEVICE(ctx);
  const size_t o_rows = up_align((size_t)n * sizeof(int32_t)), bytes = o_rows + (size_t)n * row * sizeof(double);
  uint8_t *hs;
  if (int rc = map_stage(m, bytes, &hs)) return rc;
  memcpy(hs, ids, (size_t)n * sizeof(int32_t));
  memcpy(hs + o_rows, rows, (size_t)n * row * sizeof(double));
  if (int rc = map_upload(m, m->d_up, bytes)) return rc;
  hipLaunchKernelGGL(kernel, dim3(div_up(n * row, 256)), dim3(256), 0, ctx->stream, m->view(), reinterpret_cast<const int32_t *>(m->d_up.get()),
                     reinterpret_cast<const double *>(m->d_up.get() + o_rows), n);
  SVS_LAUNCH_CHECK(ctx);
  return SVS_OK;
}

extern "C" int svs_map_set_poses(svs_map *m, int n, const int32_t *h_kf_ids, const double *h_poses) {
  svs_ctx *ctx = m ? m->ctx : nullptr;
  SVS_REQUIRE(ctx, m && n >= 0 && (n == 0 || (h_kf_ids && h_poses)));
  if (n == 0) return SVS_OK;
  if (int rc = map_check_ids(m, n, h_kf_ids, m->kf_in, m->max_kf, true)) return rc;
  return map_set_rows(m, n, h_kf_ids, h_poses, 12, map_scatter_pose_kernel);
}

extern "C" int svs_map_set_points(svs_map *m, int n, const int32_t *h_point_ids, const double *h_xyz_anchor) {
  svs_ctx *ctx = m ? m->ctx : nullptr;
  SVS_REQUIRE(ctx, m && n >= 0 && (n == 0 || (h_point_ids && h_xyz_anchor)));
  if (n == 0) return SVS_OK;
  if (int rc = map_check_ids(m, n, h_point_ids, m->pt_in, m->max_pt, true)) return rc;
  return map_set_rows(m, n, h_point_ids, h_xyz_anchor, 3, map_scatter_xyz_kernel);
}

extern "C" int svs_map_set_window(svs_map *m, int n, const int32_t *h_kf_ids) {
  svs_ctx *ctx = m ? m->ctx : nullptr;
  SVS_REQUIRE(ctx, m && n >= 0 && (n == 0 || h_kf_ids));
  if (int rc = map_check_ids(m, n, h_kf_ids, m->kf_in, m->max_kf, true)) return rc;
  SVS_DEVICE(ctx);
  if (n) {
    uint8_t *hs;
    if (int rc = map_stage(m, (size_t)n * sizeof(int32_t), &hs)) return rc;
    memcpy(hs, h_kf_ids, (size_t)n * sizeof(int32_t));
    if (int rc = map_upload(m, m->d_up, (size_t)n * sizeof(int32_t))) return rc;
  }
  if (m->kf_hi) {
    hipLaunchKernelGGL(map_window_kernel, dim3(div_up(m->kf_hi, 256)), dim3(256), 0, ctx->stream, m->view(), (const int32_t *)nullptr, 0, 0);
    SVS_LAUNCH_CHECK(ctx);
  }
  if (n) {
    hipLaunchKernelGGL(map_window_kernel, dim3(div_up(n, 256)), dim3(256), 0, ctx->stream, m->view(), reinterpret_cast<const int32_t *>(m->d_up.get()), n, 1);
    SVS_LAUNCH_CHECK(ctx);
  }
  return SVS_OK;
}

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

int svs_map_build_requests(svs_map *m, int n_requests, const MapBuildDst &dst) {
  svs_ctx *ctx = m->ctx;
  if (int rc = map_prepare_walk(m, n_requests)) return rc;
  hipLaunchKernelGGL(map_build_kernel, dim3(n_requests), dim3(MB_THREADS), 0, ctx->stream, m->view(), dst);
  SVS_LAUNCH_CHECK(ctx);
  return SVS_OK;
}

// kf_map.h: the observer rows for the keyframe decision's membership tests (keyframe.hip), current with the log
int svs_map_observer_view(svs_map *m, MapObsView *out) {
  if (int rc = map_prepare_walk(m, 0)) return rc;
  out->pt_begin = m->d_pt_begin; out->pt_rows = m->d_pt_rows; out->pt_hi = m->pt_hi;
  return SVS_OK;
}

int svs_map_build_neighborhoods(svs_map *m, int n_requests, const MapNbhDst &dst) {
  svs_ctx *ctx = m->ctx;
  if (int rc = map_prepare_walk(m, n_requests)) return rc;
  hipLaunchKernelGGL(map_nbh_kernel, dim3(n_requests), dim3(MB_THREADS), 0, ctx->stream, m->view(), dst);
  SVS_LAUNCH_CHECK(ctx);
  return SVS_OK;
}

// ---- the prepared window ------------------------------------------------------------------------------------------------------------------------------
namespace {
constexpr size_t WIN_O_EXT = 0, WIN_O_RES = WIN_O_EXT + sizeof(uint32_t) * MAP_KF_WORDS, WIN_O_WID = WIN_O_RES + sizeof(svs_map_window_result),
                 WIN_O_WTYPE = WIN_O_WID + sizeof(int32_t) * MAP_WIN_MAX, WIN_HEAD_END = WIN_O_WTYPE + sizeof(int32_t) * MAP_WIN_MAX;
size_t win_align(size_t v) { return (v + 255) & ~(size_t)255; }
// the block's pieces; the lists are as long as the map has room for points
MapWinK map_win_pieces(const svs_map *m) {
  MapWinK A{};
  uint8_t *W = m->d_win.get();
  const size_t o_lids = win_align(WIN_HEAD_END), o_aids = o_lids + win_align(sizeof(int32_t) * (size_t)m->max_pt), o_poses = o_aids + win_align(sizeof(int32_t) * (size_t)m->max_pt),
               o_psi = o_poses + win_align(sizeof(double) * 12 * MAP_WIN_MAX);
  A.ext = reinterpret_cast<uint32_t *>(W + WIN_O_EXT); A.res = reinterpret_cast<svs_map_window_result *>(W + WIN_O_RES);
  A.wid = reinterpret_cast<int32_t *>(W + WIN_O_WID); A.wtype = reinterpret_cast<int32_t *>(W + WIN_O_WTYPE);
  A.lids = reinterpret_cast<int32_t *>(W + o_lids); A.aids = reinterpret_cast<int32_t *>(W + o_aids);
  A.poses = reinterpret_cast<double *>(W + o_poses); A.psi = reinterpret_cast<double *>(W + o_psi);
  A.active = m->d_mark;
  return A;
}
size_t map_win_bytes(const svs_map *m) {
  return win_align(WIN_HEAD_END) + 2 * win_align(sizeof(int32_t) * (size_t)m->max_pt) + win_align(sizeof(double) * 12 * MAP_WIN_MAX) + win_align(sizeof(double) * 3 * (size_t)m->max_pt);
}
uint64_t next_win_serial() { static uint64_t s = 0; return __atomic_add_fetch(&s, 1, __ATOMIC_RELAXED); }
}  // namespace

// the block of the prepared window and the pinned twin of its head
static int map_win_reserve(svs_map *m) {
  svs_ctx *ctx = m->ctx;
  if (!m->d_win) SVS_HIP(ctx, m->d_win.alloc(map_win_bytes(m)));
  if (m->h_win.bytes() < WIN_HEAD_END - WIN_O_RES) SVS_HIP(ctx, m->h_win.alloc(WIN_HEAD_END - WIN_O_RES));
  return SVS_OK;
}

// from W0, its INNER keyframes and the pairs on the device (A.ids, A.types, A.inner, A.pairs, A.n0, A.n_pairs) to the prepared window: two launches, one download
static int map_win_finish(svs_map *m, const MapWinK &A, int n_inner, int window_cap, svs_map_window_result *h_res, int32_t *h_window_ids, int32_t *h_window_type) {
  svs_ctx *ctx = m->ctx;
  m->win_valid = false;                // from here on the block holds the new window, or nothing
  const MapK M = m->view();
  const int n_words = (m->pt_hi + 31) >> 5;
  SVS_HIP(ctx, hipMemsetAsync(m->d_win.get() + WIN_O_EXT, 0, WIN_O_WID - WIN_O_EXT, ctx->stream));      // the extension bitmap and the result
  if (n_words) SVS_HIP(ctx, hipMemsetAsync(m->d_mark, 0, sizeof(uint32_t) * (size_t)n_words, ctx->stream));
  hipLaunchKernelGGL(map_win_mark_kernel, dim3(n_inner), dim3(MB_THREADS), 0, ctx->stream, M, A);
  hipLaunchKernelGGL(map_win_list_kernel, dim3(std::max(1, div_up(n_words, MB_THREADS))), dim3(MB_THREADS), 0, ctx->stream, M, A);
  SVS_LAUNCH_CHECK(ctx);
  SVS_HIP(ctx, hipMemcpyAsync(m->h_win, m->d_win.get() + WIN_O_RES, WIN_HEAD_END - WIN_O_RES, hipMemcpyDeviceToHost, ctx->stream));
  SVS_HIP(ctx, hipStreamSynchronize(ctx->stream));
  const svs_map_window_result R = *reinterpret_cast<const svs_map_window_result *>(m->h_win.get());
  const int32_t *wid = reinterpret_cast<const int32_t *>(m->h_win.get() + (WIN_O_WID - WIN_O_RES)), *wtype = wid + MAP_WIN_MAX;
  *h_res = R;
  const bool over = R.n_active < 0;
  for (int i = 0; i < window_cap; ++i) {
    if (h_window_ids) h_window_ids[i] = !over && i < R.n_window ? wid[i] : -1;
    if (h_window_type) h_window_type[i] = !over && i < R.n_window ? wtype[i] : -1;
  }
  if (over) return SVS_OK;
  m->win_ids.assign(wid, wid + R.n_window); m->win_types.assign(wtype, wtype + R.n_window);
  m->win_P = R.n_window; m->win_L = R.n_active; m->win_serial = next_win_serial(); m->win_valid = true;
  return SVS_OK;
}

extern "C" int svs_map_prepare_window(svs_map *m, int n0, const int32_t *h_kf_ids, const int32_t *h_kf_type, int n_pairs, const int32_t *h_edge_pairs,
                                      int set_window_flags, int window_cap, svs_map_window_result *h_res, int32_t *h_window_ids, int32_t *h_window_type) {
  svs_ctx *ctx = m ? m->ctx : nullptr;
  SVS_REQUIRE(ctx, m && n0 >= 1 && h_kf_ids && h_kf_type && n_pairs >= 0 && (n_pairs == 0 || h_edge_pairs) && window_cap >= 1 && h_res);
  MAP_CAPACITY(ctx, n0 <= window_cap && window_cap <= MAP_WIN_MAX);
  if (int rc = map_check_ids(m, n0, h_kf_ids, m->kf_in, m->max_kf, true)) return rc;
  int n_inner = 0;
  for (int i = 0; i < n0; ++i) { SVS_REQUIRE(ctx, h_kf_type[i] == 0 || h_kf_type[i] == 1); n_inner += h_kf_type[i] == 0; }
  SVS_REQUIRE(ctx, n_inner >= 1);
  for (int i = 0; i < 2 * n_pairs; ++i) SVS_REQUIRE(ctx, svs_map_has_keyframe(m, h_edge_pairs[i]));
  if (m->n_unmeasured > 0) { ctx->err = "svs_map_prepare_window: the map holds observations without a measurement (svs_map_add_observations)"; return SVS_ERR_INVALID; }
  SVS_DEVICE(ctx);
  if (int rc = map_win_reserve(m)) return rc;
  if (int rc = map_prepare_walk(m, 1)) return rc;
  // one staged upload: W0's ids | types | the INNER ones | the pairs
  const size_t o_types = up_align(sizeof(int32_t) * (size_t)n0), o_inner = o_types + up_align(sizeof(int32_t) * (size_t)n0),
               o_pairs = o_inner + up_align(sizeof(int32_t) * (size_t)n_inner), bytes = o_pairs + sizeof(int32_t) * 2 * (size_t)n_pairs;
  uint8_t *hs;
  if (int rc = map_stage(m, bytes, &hs)) return rc;
  memcpy(hs, h_kf_ids, sizeof(int32_t) * (size_t)n0);
  memcpy(hs + o_types, h_kf_type, sizeof(int32_t) * (size_t)n0);
  { int32_t *inner = reinterpret_cast<int32_t *>(hs + o_inner); for (int i = 0, k = 0; i < n0; ++i) if (h_kf_type[i] == 0) inner[k++] = h_kf_ids[i]; }
  if (n_pairs) memcpy(hs + o_pairs, h_edge_pairs, sizeof(int32_t) * 2 * (size_t)n_pairs);
  if (int rc = map_upload(m, m->d_up, bytes)) return rc;
  MapWinK A = map_win_pieces(m);
  const uint8_t *U = m->d_up.get();
  A.ids = reinterpret_cast<const int32_t *>(U); A.types = reinterpret_cast<const int32_t *>(U + o_types); A.inner = reinterpret_cast<const int32_t *>(U + o_inner);
  A.pairs = reinterpret_cast<const int32_t *>(U + o_pairs);
  A.n0 = n0; A.n_pairs = n_pairs; A.window_cap = window_cap; A.set_flags = set_window_flags != 0;
  return map_win_finish(m, A, n_inner, window_cap, h_res, h_window_ids, h_window_type);
}

bool svs_map_window_is(const svs_map *m, uint64_t serial) { return m && m->win_valid && m->win_serial == serial; }

int svs_map_window_view(svs_map *m, MapWindowView *out) {
  svs_ctx *ctx = m->ctx;
  SVS_REQUIRE(ctx, m->win_valid);
  const MapWinK A = map_win_pieces(m);
  const int P = m->win_P, L = m->win_L;
  hipLaunchKernelGGL(map_win_gather_kernel, dim3(div_up(std::max(12 * P, L), 256)), dim3(256), 0, ctx->stream, m->view(), A, P, L);
  SVS_LAUNCH_CHECK(ctx);
  MapWindowView V{};
  V.P = P; V.L = L; V.window_ids = A.wid; V.h_window_ids = m->win_ids.data(); V.active_ids = A.lids; V.anchor_ids = A.aids; V.poses = A.poses; V.psi = A.psi;
  V.store = m->d_meas; V.n_store = (size_t)m->n_meas; V.kf_hi = m->kf_hi; V.pt_hi = m->pt_hi; V.serial = m->win_serial;
  V.h_window_types = m->win_types.data(); V.edges = m->d_edges;
  *out = V;
  return SVS_OK;
}

int svs_map_window_store(svs_map *m, const double *d_poses, const double *d_psi) {
  svs_ctx *ctx = m->ctx;
  SVS_REQUIRE(ctx, m->win_valid);
  const int P = m->win_P, L = m->win_L;
  hipLaunchKernelGGL(map_win_store_kernel, dim3(div_up(std::max(12 * P, L), 256)), dim3(256), 0, ctx->stream, m->view(), map_win_pieces(m), P, L, d_poses, d_psi);
  SVS_LAUNCH_CHECK(ctx);
  return SVS_OK;
}

// ---- the pose graph's edges ---------------------------------------------------------------------------------------------------------------------------------
static uint64_t edge_key(int a, int b) { return ((uint64_t)(uint32_t)std::min(a, b) << 32) | (uint32_t)std::max(a, b); }

// the slots of n named edges (either orientation): every edge exists; `distinct`: none twice
static int map_edge_slots(svs_map *m, int n, const int32_t *a, const int32_t *b, int stride, bool distinct, std::vector<int32_t> *slots) {
  svs_ctx *ctx = m->ctx;
  std::unordered_set<int> seen;
  slots->resize((size_t)n);
  for (int i = 0; i < n; ++i) {
    const int x = a[(size_t)i * stride], y = b[(size_t)i * stride];
    SVS_REQUIRE(ctx, x != y && svs_map_has_keyframe(m, x) && svs_map_has_keyframe(m, y));
    const auto it = m->edge_slot.find(edge_key(x, y));
    SVS_REQUIRE(ctx, it != m->edge_slot.end());
    SVS_REQUIRE(ctx, !distinct || seen.insert(it->second).second);
    (*slots)[i] = it->second;
  }
  return SVS_OK;
}

// the block the blocking calls download: `bytes` on both sides (a new block needs the stream drained of the kernels that write the old one)
static int map_dn_reserve(svs_map *m, size_t bytes) {
  svs_ctx *ctx = m->ctx;
  if (m->d_dn.bytes() >= bytes) return SVS_OK;
  SVS_HIP(ctx, hipStreamSynchronize(ctx->stream));
  const size_t want = std::max(bytes * 2, (size_t)1 << 16);
  SVS_HIP(ctx, m->d_dn.alloc(want));
  SVS_HIP(ctx, m->h_dn.alloc(want));
  return SVS_OK;
}

extern "C" int svs_map_reserve_edges(svs_map *m, int max_edges) {
  svs_ctx *ctx = m ? m->ctx : nullptr;
  SVS_REQUIRE(ctx, m && max_edges >= 1 && max_edges < (1 << 24) && m->max_edges == 0);
  SVS_DEVICE(ctx);
  SVS_HIP(ctx, m->d_edges.alloc((size_t)max_edges));
  m->edge_marg.assign((size_t)max_edges, 0);
  m->max_edges = max_edges;
  return SVS_OK;
}

extern "C" int svs_map_add_edges(svs_map *m, int n, const int32_t *h_pairs, const int32_t *h_strength, const int32_t *h_type) {
  svs_ctx *ctx = m ? m->ctx : nullptr;
  SVS_REQUIRE(ctx, m && n >= 0 && (n == 0 || (h_pairs && h_strength && h_type)));
  MAP_CAPACITY(ctx, (size_t)m->n_edges + (size_t)n <= (size_t)m->max_edges);
  if (n == 0) return SVS_OK;
  std::unordered_set<uint64_t> seen;
  for (int i = 0; i < n; ++i) {
    const int a = h_pairs[2 * i], b = h_pairs[2 * i + 1];
    SVS_REQUIRE(ctx, a != b && svs_map_has_keyframe(m, a) && svs_map_has_keyframe(m, b) && h_type[i] >= 0 && h_type[i] <= 2);
    SVS_REQUIRE(ctx, !m->edge_slot.count(edge_key(a, b)) && seen.insert(edge_key(a, b)).second);
  }
  SVS_DEVICE(ctx);
  uint8_t *hs;
  if (int rc = map_stage(m, (size_t)n * sizeof(edge_up), &hs)) return rc;
  edge_up *up = reinterpret_cast<edge_up *>(hs);
  for (int i = 0; i < n; ++i) {
    const int a = h_pairs[2 * i], b = h_pairs[2 * i + 1];
    up[i].slot = m->n_edges + i; up[i].lo = std::min(a, b); up[i].hi = std::max(a, b); up[i].strength = h_strength[i]; up[i].type = h_type[i]; up[i].pad_ = 0;
  }
  if (int rc = map_upload(m, m->d_up, (size_t)n * sizeof(edge_up))) return rc;
  hipLaunchKernelGGL(map_edge_add_kernel, dim3(div_up(n, 4)), dim3(256), 0, ctx->stream, m->d_edges.get(), reinterpret_cast<const edge_up *>(m->d_up.get()), n);
  SVS_LAUNCH_CHECK(ctx);
  for (int i = 0; i < n; ++i) { m->edge_slot[edge_key(h_pairs[2 * i], h_pairs[2 * i + 1])] = m->n_edges + i; m->edge_marg[(size_t)m->n_edges + i] = 0; }
  m->n_edges += n;
  return SVS_OK;
}

extern "C" int svs_map_set_constraints(svs_map *m, int n, const svs_ba_constraint *h_cons) {
  svs_ctx *ctx = m ? m->ctx : nullptr;
  SVS_REQUIRE(ctx, m && n >= 0 && (n == 0 || h_cons));
  MAP_CAPACITY(ctx, n == 0 || m->max_edges > 0);
  if (n == 0) return SVS_OK;
  std::vector<int32_t> slots;
  if (int rc = map_edge_slots(m, n, &h_cons[0].pose1, &h_cons[0].pose2, (int)(sizeof(svs_ba_constraint) / sizeof(int32_t)), true, &slots)) return rc;
  SVS_DEVICE(ctx);
  const size_t o_slots = up_align((size_t)n * sizeof(svs_ba_constraint)), bytes = o_slots + (size_t)n * sizeof(int2);
  uint8_t *hs;
  if (int rc = map_stage(m, bytes, &hs)) return rc;
  memcpy(hs, h_cons, (size_t)n * sizeof(svs_ba_constraint));
  int2 *si = reinterpret_cast<int2 *>(hs + o_slots);
  // T_21 = T_pose2_from_pose1: T_lo_from_hi as it stands where pose2 is the smaller id, its inverse otherwise (slam_graph.hpp:327)
  for (int i = 0; i < n; ++i) si[i] = make_int2(slots[i], h_cons[i].pose1 < h_cons[i].pose2 ? 1 : 0);
  if (int rc = map_upload(m, m->d_up, bytes)) return rc;
  hipLaunchKernelGGL(map_edge_set_kernel, dim3(div_up(n, 4)), dim3(256), 0, ctx->stream, m->d_edges.get(), reinterpret_cast<const svs_ba_constraint *>(m->d_up.get()),
                     reinterpret_cast<const int2 *>(m->d_up.get() + o_slots), n);
  SVS_LAUNCH_CHECK(ctx);
  for (int s : slots) { m->n_marg += m->edge_marg[s] ? 0 : 1; m->edge_marg[s] = 1; }
  return SVS_OK;
}

extern "C" int svs_map_unmarginalize(svs_map *m, int n, const int32_t *h_pairs) {
  svs_ctx *ctx = m ? m->ctx : nullptr;
  SVS_REQUIRE(ctx, m && n >= 0 && (n == 0 || h_pairs));
  MAP_CAPACITY(ctx, n == 0 || m->max_edges > 0);
  if (n == 0) return SVS_OK;
  std::vector<int32_t> slots;
  if (int rc = map_edge_slots(m, n, h_pairs, h_pairs + 1, 2, true, &slots)) return rc;
  SVS_DEVICE(ctx);
  uint8_t *hs;
  if (int rc = map_stage(m, (size_t)n * sizeof(int32_t), &hs)) return rc;
  memcpy(hs, slots.data(), (size_t)n * sizeof(int32_t));
  if (int rc = map_upload(m, m->d_up, (size_t)n * sizeof(int32_t))) return rc;
  hipLaunchKernelGGL(map_edge_unmarg_kernel, dim3(div_up(n, 256)), dim3(256), 0, ctx->stream, m->d_edges.get(), reinterpret_cast<const int32_t *>(m->d_up.get()), n);
  SVS_LAUNCH_CHECK(ctx);
  for (int s : slots) { m->n_marg -= m->edge_marg[s] ? 1 : 0; m->edge_marg[s] = 0; }
  return SVS_OK;
}

extern "C" int svs_map_get_edges(svs_map *m, int n, const int32_t *h_pairs, svs_map_edge *h_out) {
  svs_ctx *ctx = m ? m->ctx : nullptr;
  SVS_REQUIRE(ctx, m && n >= 0 && (n == 0 || (h_pairs && h_out)));
  MAP_CAPACITY(ctx, n == 0 || m->max_edges > 0);
  if (n == 0) return SVS_OK;
  std::vector<int32_t> slots;
  if (int rc = map_edge_slots(m, n, h_pairs, h_pairs + 1, 2, false, &slots)) return rc;
  SVS_DEVICE(ctx);
  const size_t bytes = (size_t)n * sizeof(svs_map_edge);
  if (int rc = map_dn_reserve(m, bytes)) return rc;
  uint8_t *hs;
  if (int rc = map_stage(m, (size_t)n * sizeof(int32_t), &hs)) return rc;
  memcpy(hs, slots.data(), (size_t)n * sizeof(int32_t));
  if (int rc = map_upload(m, m->d_up, (size_t)n * sizeof(int32_t))) return rc;
  hipLaunchKernelGGL(map_edge_get_kernel, dim3(div_up(n, 4)), dim3(256), 0, ctx->stream, m->d_edges.get(), reinterpret_cast<const int32_t *>(m->d_up.get()), n,
                     reinterpret_cast<svs_map_edge *>(m->d_dn.get()));
  SVS_LAUNCH_CHECK(ctx);
  SVS_HIP(ctx, hipMemcpyAsync(m->h_dn, m->d_dn, bytes, hipMemcpyDeviceToHost, ctx->stream));
  SVS_HIP(ctx, hipStreamSynchronize(ctx->stream));
  memcpy(h_out, m->h_dn.get(), bytes);
  return SVS_OK;
}

extern "C" int svs_map_edge_info(svs_map *map, int32_t *n_edges, int32_t *n_marginalized) {
  if (!map) return SVS_ERR_INVALID;
  if (n_edges) *n_edges = map->n_edges;
  if (n_marginalized) *n_marginalized = map->n_marg;
  return SVS_OK;
}

int svs_map_window_constraint_list(svs_map *m, std::vector<int4> *out) {
  svs_ctx *ctx = m->ctx;
  SVS_REQUIRE(ctx, m->win_valid);
  out->clear();
  const int P = m->win_P;
  for (int i = 0; i < P; ++i)
    for (int j = 0; j < P; ++j) {
      if (j == i || (m->win_types[i] != 1 && m->win_types[j] != 1)) continue;
      const int a = m->win_ids[i], b = m->win_ids[j];
      const auto it = m->edge_slot.find(edge_key(a, b));
      if (it == m->edge_slot.end()) continue;
      if (!m->edge_marg[it->second]) { ctx->err = "svs_ba_window_from_map_edges: an edge with an OUTER end is not marginalised (slam_graph.cpp:972)"; return SVS_ERR_INVALID; }
      out->push_back(make_int4(i, j, it->second, a < b ? 1 : 0));      // T_21 = T_j_from_i: the stored T_lo_from_hi where id_j is the smaller
    }
  return SVS_OK;
}

int svs_map_gather_constraints(svs_map *m, const int4 *d_list, int C, svs_ba_constraint *d_out) {
  svs_ctx *ctx = m->ctx;
  SVS_REQUIRE(ctx, C >= 1 && m->max_edges > 0 && d_list && d_out);
  hipLaunchKernelGGL(map_edge_gather_kernel, dim3(div_up(C, 4)), dim3(256), 0, ctx->stream, m->d_edges.get(), d_list, C, d_out);
  SVS_LAUNCH_CHECK(ctx);
  return SVS_OK;
}

extern "C" int svs_map_compute_constraints(svs_map *m, int n, const svs_map_constraint_request *req, int missing_cap, svs_map_constraint_result *h_res,
                                           int32_t *h_missing, int depth_cap, double *h_depths) {
  svs_ctx *ctx = m ? m->ctx : nullptr;
  SVS_REQUIRE(ctx, m && n >= 0 && (n == 0 || (req && h_res)) && missing_cap >= 0 && (missing_cap == 0 || h_missing) && depth_cap >= 0 && (depth_cap == 0 || h_depths));
  if (n == 0) return SVS_OK;
  MAP_CAPACITY(ctx, n <= SVS_MAP_CONS_MAX_REQUESTS);
  // ---- every refusal: before anything is uploaded -------------------------------------------------------------------------------------------------------
  size_t n_cached = 0, n_rows = 0;
  std::vector<int32_t> slot((size_t)n, -1);
  {
    std::unordered_set<int> storing;
    for (int i = 0; i < n; ++i) {
      const svs_map_constraint_request &q = req[i];
      SVS_REQUIRE(ctx, q.kf1 != q.kf2 && svs_map_has_keyframe(m, q.kf1) && svs_map_has_keyframe(m, q.kf2));
      SVS_REQUIRE(ctx, q.n_override >= 0 && q.n_override <= 2 && q.n_cached >= 0 && (q.n_cached == 0 || (q.cached_ids && q.cached_T)));
      for (int k = 0; k < q.n_override; ++k) SVS_REQUIRE(ctx, q.override_id[k] >= 0 && q.override_id[k] < m->max_kf);
      SVS_REQUIRE(ctx, q.n_override < 2 || q.override_id[0] != q.override_id[1]);
      MAP_CAPACITY(ctx, q.n_cached <= m->max_kf);
      for (int k = 0; k < q.n_cached; ++k) SVS_REQUIRE(ctx, q.cached_ids[k] >= 0 && q.cached_ids[k] < m->max_kf && (k == 0 || q.cached_ids[k - 1] < q.cached_ids[k]));
      if (h_depths) MAP_CAPACITY(ctx, m->kf_nobs[q.kf1] <= depth_cap);
      if (q.store) {
        MAP_CAPACITY(ctx, m->max_edges > 0);
        const auto it = m->edge_slot.find(edge_key(q.kf1, q.kf2));
        SVS_REQUIRE(ctx, it != m->edge_slot.end());
        SVS_REQUIRE(ctx, storing.insert(it->second).second);
        slot[i] = it->second;
      }
      n_cached += (size_t)q.n_cached; n_rows += (size_t)m->kf_nobs[q.kf1];
    }
  }
  SVS_DEVICE(ctx);
  // ---- room: the scratch rows, the download block, a bitmap row per request, current CSR views ----------------------------------------------------------------
  if (m->d_depth.bytes() < std::max<size_t>(n_rows, 1) * sizeof(double)) {
    SVS_HIP(ctx, hipStreamSynchronize(ctx->stream));
    const size_t want = std::max<size_t>(n_rows * 2, 4096);
    SVS_HIP(ctx, m->d_depth.alloc(want));
    SVS_HIP(ctx, m->d_common.alloc(want));
  }
  const size_t o_miss = (size_t)n * sizeof(svs_map_constraint_result), o_depth = up_align(o_miss + (size_t)n * missing_cap * sizeof(int32_t)),
               dn_bytes = o_depth + (h_depths ? n_rows * sizeof(double) : 0);
  if (int rc = map_dn_reserve(m, dn_bytes)) return rc;
  if (int rc = map_prepare_walk(m, n)) return rc;
  // ---- one staged upload: the requests | cached ids | cached poses -------------------------------------------------------------------------------------------
  const size_t o_ids = up_align((size_t)n * sizeof(cons_req)), o_T = o_ids + up_align(n_cached * sizeof(int32_t)), bytes = o_T + n_cached * 12 * sizeof(double);
  uint8_t *hs;
  if (int rc = map_stage(m, bytes, &hs)) return rc;
  {
    cons_req *up = reinterpret_cast<cons_req *>(hs);
    int32_t *ids = reinterpret_cast<int32_t *>(hs + o_ids);
    double *T = reinterpret_cast<double *>(hs + o_T);
    size_t c = 0, row = 0;
    for (int i = 0; i < n; ++i) {
      const svs_map_constraint_request &q = req[i];
      cons_req u{};
      u.kf1 = q.kf1; u.kf2 = q.kf2; u.slot = slot[i]; u.slot_inv = q.kf1 > q.kf2 ? 1 : 0;
      u.n_override = q.n_override; u.n_cached = q.n_cached; u.cached_off = (int32_t)c; u.row_off = (long long)row;
      for (int k = 0; k < q.n_override; ++k) { u.override_id[k] = q.override_id[k]; memcpy(u.override_T[k], q.override_T[k], sizeof u.override_T[k]); }
      up[i] = u;
      if (q.n_cached) { memcpy(ids + c, q.cached_ids, (size_t)q.n_cached * sizeof(int32_t)); memcpy(T + 12 * c, q.cached_T, (size_t)q.n_cached * 12 * sizeof(double)); }
      c += (size_t)q.n_cached; row += (size_t)m->kf_nobs[q.kf1];
    }
  }
  if (int rc = map_upload(m, m->d_up, bytes)) return rc;
  MapConsK A{};
  A.req = reinterpret_cast<const cons_req *>(m->d_up.get()); A.cached_ids = reinterpret_cast<const int32_t *>(m->d_up.get() + o_ids);
  A.cached_T = reinterpret_cast<const double *>(m->d_up.get() + o_T);
  A.res = reinterpret_cast<svs_map_constraint_result *>(m->d_dn.get()); A.missing = reinterpret_cast<int32_t *>(m->d_dn.get() + o_miss); A.missing_cap = missing_cap;
  A.depth = m->d_depth; A.common = m->d_common; A.edges = m->d_edges;
  hipLaunchKernelGGL(map_cons_kernel, dim3(n), dim3(MB_THREADS), 0, ctx->stream, m->view(), A);
  SVS_LAUNCH_CHECK(ctx);
  if (h_depths && n_rows) SVS_HIP(ctx, hipMemcpyAsync(m->d_dn.get() + o_depth, m->d_depth, n_rows * sizeof(double), hipMemcpyDeviceToDevice, ctx->stream));
  SVS_HIP(ctx, hipMemcpyAsync(m->h_dn, m->d_dn, dn_bytes, hipMemcpyDeviceToHost, ctx->stream));
  SVS_HIP(ctx, hipStreamSynchronize(ctx->stream));
  memcpy(h_res, m->h_dn.get(), (size_t)n * sizeof(svs_map_constraint_result));
  if (missing_cap) memcpy(h_missing, m->h_dn.get() + o_miss, (size_t)n * missing_cap * sizeof(int32_t));
  size_t row = 0;
  for (int i = 0; i < n; ++i) {
    if (h_depths) {
      double *d = h_depths + (size_t)i * depth_cap;
      const int k = h_res[i].status == SVS_CONS_OK ? h_res[i].strength : 0;
      memcpy(d, m->h_dn.get() + o_depth + row * sizeof(double), (size_t)k * sizeof(double));
      std::fill(d + k, d + depth_cap, 0.0);
    }
    row += (size_t)m->kf_nobs[req[i].kf1];
    if (slot[i] >= 0 && h_res[i].status == SVS_CONS_OK) { m->n_marg += m->edge_marg[slot[i]] ? 0 : 1; m->edge_marg[slot[i]] = 1; }
  }
  return SVS_OK;
}

#include "map_walk.inc"
#include "map_addkf.inc"
#include "map_commit.inc"
