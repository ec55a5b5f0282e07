// map.hip -- the back end's map kept on the device (svs_map_*): ONE translation unit, cut by stage.  This file holds what every part shares -- the constants, the
// tables as the kernels read them (MapK), the handle (svs_map: private to this unit), create / destroy / info, the seam headers' small accessors, the id checks
// and the staging layout of the upload and download blocks -- and includes the parts in dependency order.  Each part holds its kernels AND the entry points that
// launch them:
//   map_sets.h        the set and scan idioms, once: bitmaps over ids, ascending lists by popcounts and a workgroup prefix, counts -> begin, rows and records
//   map_csr.inc       the observations' two CSR views (by keyframe: a feature_table; by point: a sorted observer row), rebuilt by a counting sort when the log
//                     has grown: map_count / scan / fill / sort_rows, map_prepare_walk, the observer view of kf_map.h
//   map_store.inc     the update path (map_scatter_*, the window flags, the measured pairs: one staged upload, one lane per record) and the plain read-backs
//                     (points, poses, a keyframe's feature_table)
//   map_request.inc   map_build_kernel: the requests of the registration chain (register.hip, reg_map.h), one workgroup per request
//   map_edges.inc     the pose graph's edge table (EdgeTable: map_edge_*) and computeConstraint (map_cons_kernel), one workgroup per keyframe pair
//   map_walk.inc      the pose graph's walks: the strength-ordered adjacency and one level-synchronous breadth-first search per request (walk_map.h)
//   map_nbh.inc       a front-end stream's neighbourhood: from a vertex list (nbh_map.h: nbh_collect, map_nbh_kernel) and from a root id (nbr_map.h: map_nbr_*)
//   map_window.inc    the double window's BA problem (ba_map.h): map_win_mark / list / gather / store, svs_map_prepare_window and _from_root
//   map_addkf.inc     inserting a keyframe (SlamGraph::addKeyframe): computeStrength by counting passes, the kept points and pairs by prefix sums
//   map_addkf_dev.inc the same insertion with the two lists in device memory: the refusals about the records, the track flags and the id columns by one workgroup
//   map_commit.inc    registerKeyframes / addLoopClosure: a device track list and an edge list applied to the map
// Integer and copy work throughout (but for the three divisions of invert_depth and the f64 geometry of map_cons_kernel); the host keeps the id sets and the set of
// pairs, so every refusal happens before anything is uploaded (map_addkf_dev.inc alone decides refusals about records it never sees on the device, from bitmap copies
// of the id sets, before anything is written); no atomic decides a value or an order, so every result is a function of the map's content alone.
#include "reg_map.h"
#include "nbh_map.h"
#include "nbr_map.h"
#include "ba_map.h"
#include "walk_map.h"
#include "kf_map.h"
#include "addkf_map.h"
#include "pose.h"
#include "staging.h"
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

#include "map_sets.h"

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
  // staging of the updates: a twin block, its pinned side reused once the upload out of it has happened
  TwinBlock up; owned::Event up_ev; bool up_pending = false;
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
  TwinBlock dn;
  // svs_map_add_keyframe_dev (map_addkf_dev.inc): the id sets as bitmaps on the device, the counts they were written at, the row over point ids its check kernel
  // leaves as it found it; all allocated with the first such call
  DevBuf<uint32_t> d_in_pt, d_in_kf; PinnedBuf<uint32_t> h_in; int in_n_kf = -1, in_n_pt = -1;
  DevBuf<int32_t> d_first;
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

// ---- staging: one upload and at most one download per call -----------------------------------------------------------------------------------------------------
// Both blocks are twin blocks of the library's staging (staging.h: rows of typed 16-byte-aligned pieces that a call declares in order, host(p) / dev(p) the only
// addresses), grown to max(2 x bytes, 64 KB).  The handles below add what is the map's own: when the pinned side is free, and the waits.
template <class T> using MapPiece = Piece<T>;
using MapPieces = Pieces<>;
constexpr size_t MAP_STAGE_FLOOR = (size_t)1 << 16;

// the upload.  reserve() hands the pinned block over free to be written: the upload out of it that is still in flight has happened, and it holds the pieces;
// upload() is the call's single hipMemcpyAsync on the map's stream, with the event the next reserve() waits for
struct MapUp : MapPieces {
  svs_map *m;
  explicit MapUp(svs_map *map) : m(map) {}
  int reserve(size_t at_least = 0) {
    svs_ctx *ctx = m->ctx;
    if (m->up_pending) { SVS_HIP(ctx, hipEventSynchronize(m->up_ev)); m->up_pending = false; }
    return m->up.reserve(ctx, std::max(end, at_least), MAP_STAGE_FLOOR);      // (draining: the device twin may still be read by the scatter of the last update)
  }
  template <class T> T *host(const MapPiece<T> &p) const { return m->up.host(p); }
  template <class T> const T *dev(const MapPiece<T> &p) const { return m->up.dev(p); }
  template <class T> void put(const MapPiece<T> &p, const T *src) const { if (p.n) memcpy(host(p), src, p.bytes()); }
  // the bytes [from, to) of the block to the same place of the twin, or the whole block to d_dst
  int upload(size_t from, size_t to, void *d_dst = nullptr) {
    svs_ctx *ctx = m->ctx;
    if (d_dst) SVS_HIP(ctx, hipMemcpyAsync(d_dst, m->up.h.get() + from, to - from, hipMemcpyHostToDevice, ctx->stream));
    else if (int rc = m->up.upload(ctx, from, to)) return rc;
    SVS_HIP(ctx, hipEventRecord(m->up_ev, ctx->stream));
    m->up_pending = true;
    return SVS_OK;
  }
  int upload(void *d_dst = nullptr) { return upload(0, end, d_dst); }
};

// the download of the blocking calls (a new block needs the stream drained of the kernels that write the old one).  The kernels write dev(p); download() copies
// the block and waits for the stream; then host(p) holds the results
struct MapDn : MapPieces {
  svs_map *m;
  explicit MapDn(svs_map *map) : m(map) {}
  int reserve(size_t at_least = 0) { return m->dn.reserve(m->ctx, std::max(end, at_least), MAP_STAGE_FLOOR); }
  template <class T> T *dev(const MapPiece<T> &p) const { return m->dn.dev(p); }
  template <class T> const T *host(const MapPiece<T> &p) const { return m->dn.host(p); }
  template <class T> void get(const MapPiece<T> &p, T *dst) const { if (p.n) memcpy(dst, host(p), p.bytes()); }
  int download(size_t from, size_t to) {
    svs_ctx *ctx = m->ctx;
    if (int rc = m->dn.download(ctx, from, to)) return rc;
    SVS_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return SVS_OK;
  }
  int download() { return download(0, end); }
};

// a plain read-back: n ids up, `per` T for each down through launch(d_ids, d_out), copied to h_out
template <class T, class Launch>
static int map_read_back(svs_map *m, int n, const int32_t *h_ids, size_t per, T *h_out, Launch launch) {
  svs_ctx *ctx = m->ctx;
  SVS_DEVICE(ctx);
  MapUp up(m);
  MapDn dn(m);
  const auto ids = up.piece<int32_t>(n);
  const auto out = dn.piece<T>(per * n);
  if (int rc = dn.reserve()) return rc;
  if (int rc = up.reserve()) return rc;
  up.put(ids, h_ids);
  if (int rc = up.upload()) return rc;
  launch(up.dev(ids), dn.dev(out));
  SVS_LAUNCH_CHECK(ctx);
  if (int rc = dn.download()) return rc;
  dn.get(out, h_out);
  return SVS_OK;
}

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

#include "map_csr.inc"
#include "map_store.inc"
#include "map_request.inc"
#include "map_edges.inc"
#include "map_walk.inc"
#include "map_nbh.inc"
#include "map_window.inc"
#include "map_addkf.inc"
#include "map_addkf_dev.inc"
#include "map_commit.inc"
