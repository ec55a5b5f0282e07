// newpoints.hip -- the front end's newpoint_map on the device (stereo_frontend.h:125; seeded at stereo_frontend.cpp:808, pruned at :360-365, handed to the matcher at
// :989-1029).  The contract is in the header; tests/newpoint_model.py restates it.  A stream's store is one row of 64-byte records, its groups packed back to back
// in store order, and a (key, count) table beside it.
//   newpoints_prune_kernel    one workgroup (four waves) per stream.  P -- the ids of the matched new points of the last step -- is an ordered compaction of the
//                   step's records into LDS (per 256-record chunk one ballot, the waves' popcounts through LDS, a running offset), sorted there.  Then every group is compacted in
//                   place, chunk by chunk: a chunk's records are read into registers, tested against P by bisection, and written to their rank among the records kept so far
//                   once every wave's loads have landed (a barrier does not drain them: each wave waits for its own first).  A record only ever moves towards the
//                   front of the row and every record in front of a chunk's end has been read by then, so nothing unread is overwritten.
//   newpoints_compose_kernel  put / seed / drop: a stream's new row gathered segment by segment into a scratch row and copied back, with its new table.
//   newpoints_list_kernel     the hand-over: the groups named, in the order named, then the staged tail, into the stream's candidate list with kf_index rewritten.
#include "newpoints.h"
#include <stddef.h>

namespace {
constexpr int NP_THREADS = 256, NP_WAVES = NP_THREADS / 64, NP_MAX_GROUPS = SVS_NEWPOINTS_MAX_GROUPS;
constexpr int NP_MAX_STEP_RECORDS = 8192;       // P in LDS, padded to a power of two for its sort: 32 KiB
static_assert(sizeof(svs_candidate_point) == 64 && offsetof(svs_candidate_point, kf_index) == 52 && offsetof(svs_candidate_point, point_id) == 56,
              "a record is four 16-byte words, the fourth (anchor_level, kf_index, point_id, pad_)");
static_assert(sizeof(svs_newpoints_prune_args) == 120 && sizeof(np_op) == 16 + 4 * NP_MAX_GROUPS && sizeof(np_list_req) == 16 + 16 * NP_MAX_GROUPS, "staged as written");

// the rank of this lane's flag among the flags of the workgroup's 256 lanes, and their number; every lane calls it (two barriers inside)
__device__ __forceinline__ int block_rank(bool flag, int *s_wave, int &total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const unsigned long long m = __ballot(flag);
  if (lane == 0) s_wave[wave] = __popcll(m);
  __syncthreads();
  int off = 0, tot = 0;
#pragma unroll
  for (int w = 0; w < NP_WAVES; ++w) { const int c = s_wave[w]; off += w < wave ? c : 0; tot += c; }
  __syncthreads();
  total = tot;
  return off + __popcll(m & ((1ull << lane) - 1ull));
}

__global__ __launch_bounds__(NP_THREADS) void newpoints_prune_kernel(svs_newpoints_prune_args A, int32_t *__restrict__ n_removed) {
  extern __shared__ int s_P[];                  // [A.n rounded up to a power of two]
  __shared__ int s_wave[NP_WAVES], s_cnt[NP_MAX_GROUPS], s_new[NP_MAX_GROUPS], s_G;
  const int tid = threadIdx.x;
  const int s = A.d_stream ? A.d_stream[blockIdx.x] : (int)blockIdx.x;

  // P: the new list of rule 1 of svs_keyframe_decide, in record order
  int n = A.d_n ? A.d_n[s] : A.n;
  n = n < 0 ? 0 : (n > A.n ? A.n : n);
  const int n_new = A.d_n_new[s];
  if (n_new < n) n = n_new < 0 ? 0 : n_new;
  const svs_match_result *res = A.d_res + (size_t)s * A.res_bstride;
  const svs_candidate_point *pts = A.d_pts + (size_t)s * A.pts_bstride;
  const svs_gated_point *gated = A.d_gated + (size_t)s * A.gated_bstride;
  int np = 0;
  for (int base = 0; base < n; base += NP_THREADS) {      // block-uniform
    const int i = base + tid;
    const bool in = i < n && res[i].status == SVS_MATCH_OK && gated[i].accepted != 0;
    int tot;
    const int pos = np + block_rank(in, s_wave, tot);
    if (in) s_P[pos] = pts[i].point_id;
    np += tot;
  }

  // P ascending (a bitonic sort over the next power of two, the padding INT_MAX): a record is then tested by bisection, not by a walk over P
  int npad = 1;
  while (npad < np) npad <<= 1;                 // <= the launch's LDS: the host sized it to A.n rounded up
  __syncthreads();
  for (int i = np + tid; i < npad; i += NP_THREADS) s_P[i] = 0x7fffffff;
  __syncthreads();
  for (int k = 2; k <= npad; k <<= 1)
    for (int j = k >> 1; j > 0; j >>= 1) {      // block-uniform
      for (int i = tid; i < npad; i += NP_THREADS) {
        const int l = i ^ j;
        if (l > i) {
          const int a = s_P[i], b = s_P[l];
          if ((a > b) == ((i & k) == 0)) { s_P[i] = b; s_P[l] = a; }
        }
      }
      __syncthreads();
    }

  // the group table, cut where it would leave the stream's rows
  if (tid == 0) {
    int G = A.d_n_groups[s];
    G = G < 0 ? 0 : (G > (int)A.group_bstride ? (int)A.group_bstride : G);
    size_t at = 0;
    for (int g = 0; g < G; ++g) {
      int c = A.d_group_count[(size_t)s * A.group_bstride + g];
      c = c < 0 ? 0 : c;
      if (at + (size_t)c > A.store_bstride) c = (int)(A.store_bstride - at);
      s_cnt[g] = c;
      at += (size_t)c;
    }
    s_G = G;
  }
  __syncthreads();      // (also: P is written)
  const int G = s_G;

  int4 *row = reinterpret_cast<int4 *>(A.d_store + (size_t)s * A.store_bstride);
  int src = 0, dst = 0;                         // records read / kept so far: block-uniform
  for (int g = 0; g < G; ++g) {
    const int cnt = s_cnt[g], dst0 = dst;
    for (int base = 0; base < cnt; base += NP_THREADS) {
      const int i = base + tid;
      const bool have = i < cnt;
      int4 q0, q1, q2, q3;
      bool keep = false;
      if (have) {
        const int4 *r = row + (size_t)(src + i) * 4;
        q0 = r[0]; q1 = r[1]; q2 = r[2]; q3 = r[3];
        int lo = 0, hi = np;                    // the first entry >= the id among the np real ones (the padding sorts behind them)
        while (lo < hi) {
          const int mid = (lo + hi) >> 1;
          if (s_P[mid] < q3.z) lo = mid + 1; else hi = mid;
        }
        keep = !(lo < np && s_P[lo] == q3.z);
      }
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");      // this wave's loads have landed before the barriers inside block_rank let any wave write
      int tot;
      const int pos = dst + block_rank(keep, s_wave, tot);
      if (keep) {
        int4 *w = row + (size_t)pos * 4;
        w[0] = q0; w[1] = q1; w[2] = q2; w[3] = q3;
      }
      dst += tot;
    }
    src += cnt;
    if (tid == 0) s_new[g] = dst - dst0;
  }
  __syncthreads();
  if (tid < G) A.d_group_count[(size_t)s * A.group_bstride + tid] = s_new[tid];
  if (tid == 0) n_removed[blockIdx.x] = src - dst;
}

__device__ __forceinline__ void copy_records(svs_candidate_point *dst, const svs_candidate_point *src, int n) {
  const int4 *s4 = reinterpret_cast<const int4 *>(src);
  int4 *d4 = reinterpret_cast<int4 *>(dst);
  for (int i = threadIdx.x; i < n * 4; i += NP_THREADS) d4[i] = s4[i];
}

__global__ __launch_bounds__(NP_THREADS) void newpoints_compose_kernel(NpCompose C) {
  __shared__ int s_cnt[NP_MAX_GROUPS];
  const int tid = threadIdx.x;
  const np_op *op = C.ops + blockIdx.x;
  const int s = op->stream, G = op->n_groups;      // the host checked: stream < B, n_groups <= 64, every segment inside its source, their sum <= record_cap
  svs_candidate_point *rec = C.rec + (size_t)s * C.record_cap, *tmp = C.tmp + (size_t)s * C.record_cap;
  if (tid < NP_MAX_GROUPS) s_cnt[tid] = 0;
  __syncthreads();
  int at = 0;
  for (int k = 0; k < op->n_seg; ++k) {            // block-uniform
    const np_seg sg = C.segs[op->seg_off + k];
    int len = sg.len;
    const svs_candidate_point *src = sg.kind == NP_SEG_STORE ? rec + sg.off : C.staged + sg.off;
    if (sg.kind == NP_SEG_SEED) {
      len = C.seed_cnt[3 * sg.off] + C.seed_cnt[3 * sg.off + 1] + C.seed_cnt[3 * sg.off + 2];
      len = len < 0 ? 0 : (len > C.seed_cap ? C.seed_cap : len);
      src = C.seed_out + (size_t)sg.off * C.seed_cap;
    }
    if (len > C.record_cap - at) len = C.record_cap - at;      // (the host's bound holds: never taken)
    copy_records(tmp + at, src, len);
    if (tid == 0) s_cnt[sg.group] += len;
    at += len;
  }
  __syncthreads();      // the scratch row is written (by this workgroup: visible behind the barrier)
  copy_records(rec, tmp, at);
  if (tid < NP_MAX_GROUPS) {
    C.key[(size_t)s * NP_MAX_GROUPS + tid] = tid < G ? op->key[tid] : -1;
    C.cnt[(size_t)s * NP_MAX_GROUPS + tid] = tid < G ? s_cnt[tid] : 0;
  }
  if (tid == 0) C.ng[s] = G;
}

__global__ __launch_bounds__(NP_THREADS) void newpoints_list_kernel(NpList L) {
  const int tid = threadIdx.x;
  const np_list_req *q = L.req + blockIdx.x;
  const int s = q->stream, G = q->n_seg;           // the host checked: the total <= max_points, every segment inside its source
  const int4 *rec = reinterpret_cast<const int4 *>(L.rec + (size_t)s * L.record_cap), *staged = reinterpret_cast<const int4 *>(L.staged);
  int4 *pts = reinterpret_cast<int4 *>(L.pts + (size_t)s * L.max_points);
  int at = 0;
  for (int g = 0; g < G; ++g) {                    // block-uniform
    const np_list_seg sg = q->seg[g];
    const int4 *src = (sg.kind == NP_SEG_STORE ? rec : staged) + (size_t)sg.off * 4;
    for (int i = tid; i < sg.len * 4; i += NP_THREADS) {
      int4 v = src[i];
      if (sg.kind == NP_SEG_STORE && (i & 3) == 3) v.y = sg.kf_index;
      pts[(size_t)at * 4 + i] = v;
    }
    at += sg.len;
    if (tid == 0) L.group_end[(size_t)s * NP_MAX_GROUPS + g] = at;
  }
  if (tid >= G && tid < NP_MAX_GROUPS) L.group_end[(size_t)s * NP_MAX_GROUPS + tid] = 0;
  if (tid == 0) { L.n_groups[s] = G; L.n_new[s] = at - q->seg[G - 1].len; }
  const int4 none = make_int4(-1, -1, -1, -1);      // "no candidate": 0xff
  for (int i = at * 4 + tid; i < q->prev_len * 4; i += NP_THREADS) pts[i] = none;
}
}  // namespace

extern "C" int svs_newpoints_prune(svs_ctx *ctx, const svs_newpoints_prune_args *a, int32_t *d_n_removed) {
  SVS_REQUIRE(ctx, ctx && a && d_n_removed && a->n >= 0 && a->batch >= 0);
  if (a->batch == 0) return SVS_OK;
  SVS_REQUIRE(ctx, a->d_n_new && a->d_store && a->d_group_count && a->d_n_groups && (a->n == 0 || (a->d_res && a->d_pts && a->d_gated)));
  if (a->group_bstride > (size_t)NP_MAX_GROUPS) { ctx->err = "svs_newpoints_prune: more than SVS_NEWPOINTS_MAX_GROUPS groups per stream"; return SVS_ERR_CAPACITY; }
  if (a->n > NP_MAX_STEP_RECORDS) { ctx->err = "svs_newpoints_prune: more than 8192 records per step"; return SVS_ERR_UNSUPPORTED; }
  size_t lds = 1;
  while (lds < (size_t)a->n) lds <<= 1;
  SVS_DEVICE(ctx);
  hipLaunchKernelGGL(newpoints_prune_kernel, dim3(a->batch), dim3(NP_THREADS), sizeof(int) * lds, ctx->stream, *a, d_n_removed);
  SVS_LAUNCH_CHECK(ctx);
  return SVS_OK;
}

int svs_newpoints_compose(svs_ctx *ctx, int n_ops, const NpCompose &c) {
  if (n_ops <= 0) return SVS_OK;
  hipLaunchKernelGGL(newpoints_compose_kernel, dim3(n_ops), dim3(NP_THREADS), 0, ctx->stream, c);
  SVS_LAUNCH_CHECK(ctx);
  return SVS_OK;
}

int svs_newpoints_list(svs_ctx *ctx, int n_requests, const NpList &l) {
  if (n_requests <= 0) return SVS_OK;
  hipLaunchKernelGGL(newpoints_list_kernel, dim3(n_requests), dim3(NP_THREADS), 0, ctx->stream, l);
  SVS_LAUNCH_CHECK(ctx);
  return SVS_OK;
}
