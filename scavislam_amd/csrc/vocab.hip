// vocab.hip -- svs_vocab_train: the visual vocabulary that svs_loop_set_vocabulary takes, trained on the device.  The counterpart of the arithmetic half of the
// reference's dictionary program (create_dictionary.cpp:144-177, cvflann::hierarchicalClustering with k-means++ centres): FLAT Lloyd iterations with k-means++
// seeding -- what the cut through the reference's 32-ary k-means tree approximates.  Not pinned by the reference's binaries: the yardstick
// is the NumPy restatement tests/vocab_model.py.
//   seeding      TWO launches per centre, queued back to back: vocab_seed_weight_kernel (f64 distance to the last centre, running minimum, fixed-point weight,
//                exact block sums) and vocab_seed_pick_kernel (one workgroup: total, draw, search of the prefix sums).  The chosen index stays on the device.
//   assignment   loop_words_walk (loop_words.h), the walk of svs_loop_add_locations, against chunks of LW_CHUNK centres; 64-bit atomic minimum on the key
//   update       64-bit INTEGER atomics on the fixed-point components: one wave instruction = one point's row (512 contiguous bytes at K = 64); the sums are
//                exact, hence independent of the order.  No float atomics anywhere.
// Every sum that crosses a thread is an integer sum, every minimum is taken on a total order: the outputs are a function of the inputs alone.
#include "common.h"
#include "loop_words.h"
#include <math.h>
#include <string.h>
#include <algorithm>
#include <vector>

typedef unsigned long long u64;
constexpr int VS_BLOCK = 256;                                        // points per workgroup of the weight kernel = weights per block sum
constexpr int VS_PICK = 1024;                                        // threads of the pick workgroup
constexpr int VS_PER = SVS_VOCAB_MAX_POINTS / VS_BLOCK / VS_PICK;    // block sums per thread of the pick workgroup at the largest n (8)
constexpr double VS_W_SCALE = 0x1p28, VS_Q_SCALE = 0x1p38, VS_Q_INV = 0x1p-38;

// ---- seeding ------------------------------------------------------------------------------------------------------------------------------------------------
// grid-stride over max(n, n_words): weights to +inf, centre 0 = i0, the others "none"; state[0] = n_seeded, -1 while the seeding has not ended early
__global__ __launch_bounds__(256) void vocab_seed_init_kernel(int n, int n_words, int i0, double *__restrict__ w, int32_t *__restrict__ seed_idx, int32_t *__restrict__ state) {
  const int m = max(n, n_words);
  for (int i = (int)(blockIdx.x * 256u + threadIdx.x); i < m; i += (int)(gridDim.x * 256u)) {
    if (i < n) w[i] = INFINITY;
    if (i < n_words) seed_idx[i] = i == 0 ? i0 : -1;
    if (i == 0) state[0] = -1;
  }
}

// step c, first launch.  grid = ceil(n / 256).  One thread per point: the f64 distance to centre c - 1 in component order (no contraction in this file)
__global__ __launch_bounds__(VS_BLOCK) void vocab_seed_weight_kernel(const float *__restrict__ X, int K, int n, int c, const int32_t *__restrict__ seed_idx,
                                                                    double *__restrict__ w, u64 *__restrict__ W, u64 *__restrict__ bsum) {
  __shared__ u64 s_sum[VS_BLOCK / 64];
  const int ci = seed_idx[c - 1];
  if (ci < 0 || ci >= n) return;                                           // the seeding has ended (T == 0): W stays all zero.  Uniform
  const int i = (int)(blockIdx.x * (unsigned)VS_BLOCK + threadIdx.x);
  u64 Wi = 0;
  if (i < n) {
    const float4 *x = reinterpret_cast<const float4 *>(X + (size_t)i * K), *y = reinterpret_cast<const float4 *>(X + (size_t)ci * K);
    double s = 0.0;
    for (int k = 0; k < K / 4; ++k) {
      const float4 a = x[k], b = y[k];
      double d = (double)a.x - (double)b.x; s = s + d * d;
      d = (double)a.y - (double)b.y; s = s + d * d;
      d = (double)a.z - (double)b.z; s = s + d * d;
      d = (double)a.w - (double)b.w; s = s + d * d;
    }
    double wi = w[i];
    wi = s < wi ? s : wi;
    if (i == ci) wi = 0.0;
    w[i] = wi;
    Wi = (u64)(wi * VS_W_SCALE);                                           // < 2^41: |x| < 4
    W[i] = Wi;
  }
  Wi = wave_sum(Wi);
  if ((threadIdx.x & 63) == 0) s_sum[threadIdx.x >> 6] = Wi;
  __syncthreads();
  if (threadIdx.x == 0) bsum[blockIdx.x] = (s_sum[0] + s_sum[1]) + (s_sum[2] + s_sum[3]);
}

// inclusive scan over the workgroup's VS_PICK values (Hillis-Steele in LDS); integer, so the order does not matter
__device__ __forceinline__ u64 vocab_block_scan(u64 *s_scan, int tid, u64 v) {
  __syncthreads();                                                         // whatever was read from s_scan before
  s_scan[tid] = v;
  __syncthreads();
  for (int off = 1; off < VS_PICK; off <<= 1) {
    const u64 t = tid >= off ? s_scan[tid - off] : 0;
    __syncthreads();
    s_scan[tid] += t;
    __syncthreads();
  }
  return s_scan[tid];
}

// step c, second launch.  ONE workgroup: T from the block sums, the draw, the block that holds the drawn position, the position inside the block
__global__ __launch_bounds__(VS_PICK) void vocab_seed_pick_kernel(int n, int nb, int c, uint64_t seed, const u64 *__restrict__ W, const u64 *__restrict__ bsum,
                                                                 int32_t *__restrict__ seed_idx, int32_t *__restrict__ state) {
  __shared__ u64 s_scan[VS_PICK];
  __shared__ u64 s_r;
  __shared__ int s_blk;
  if (seed_idx[c - 1] < 0) return;                                         // ended at an earlier step.  Uniform
  const int tid = (int)threadIdx.x;
  u64 v[VS_PER], loc = 0;
#pragma unroll
  for (int u = 0; u < VS_PER; ++u) {
    const int b = tid * VS_PER + u;
    v[u] = b < nb ? bsum[b] : 0;
    loc += v[u];
  }
  const u64 incl = vocab_block_scan(s_scan, tid, loc);
  const u64 T = s_scan[VS_PICK - 1];
  if (T == 0) {                                                            // every point coincides with a centre: n_seeded = c.  Uniform
    if (tid == 0) state[0] = c;
    return;
  }
  const u64 r = __umul64hi(splitmix64(seed ^ ((1ull << 62) | (u64)(uint32_t)c)), T);      // < T
  if (tid == 0) s_blk = -1;
  __syncthreads();
  if (incl - loc <= r && r < incl) {                                       // exactly one thread: the prefix sums are monotone and r < T
    u64 p = incl - loc;
    bool found = false;
#pragma unroll
    for (int u = 0; u < VS_PER; ++u) {
      if (!found && r < p + v[u]) { s_blk = tid * VS_PER + u; s_r = r - p; found = true; }
      p += v[u];
    }
  }
  __syncthreads();
  const int blk = s_blk;
  if (blk < 0 || blk >= nb) return;                                        // (never: r < T)
  const u64 rr = s_r;
  const int i = blk * VS_BLOCK + tid;
  const u64 wv = tid < VS_BLOCK && i < n ? W[i] : 0;
  const u64 incl2 = vocab_block_scan(s_scan, tid, wv);
  if (incl2 - wv <= rr && rr < incl2) seed_idx[c] = i;                     // the smallest i whose inclusive prefix sum exceeds r
}

// the seeded centres: row seed_idx[j] of X, zeros behind n_seeded.  One thread per float4
__global__ __launch_bounds__(256) void vocab_gather_kernel(const float *__restrict__ X, int K, int n, int n_words, const int32_t *__restrict__ seed_idx, float *__restrict__ words) {
  const int K4 = K / 4, idx = (int)(blockIdx.x * 256u + threadIdx.x);      // n_words * K4 <= 2^25
  if (idx >= n_words * K4) return;
  const int j = idx / K4, k4 = idx - j * K4, ci = seed_idx[j];
  reinterpret_cast<float4 *>(words)[idx] = ci >= 0 && ci < n ? reinterpret_cast<const float4 *>(X + (size_t)ci * K)[k4] : make_float4(0.f, 0.f, 0.f, 0.f);
}

// ---- Lloyd --------------------------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void vocab_norm_kernel(const float *__restrict__ rows, int K, int n, float *__restrict__ norm) {
  const int i = (int)(blockIdx.x * 256u + threadIdx.x);
  if (i < n) norm[i] = loop_sqnorm(rows + (size_t)i * K, K);
}

// grid = (point blocks of 32, centre chunks of LW_CHUNK).  The chunks meet in a 64-bit atomic minimum on the key, whose minimum is order-independent
template <int K>
__global__ __launch_bounds__(256) void vocab_assign_kernel(const float *__restrict__ X, const float *__restrict__ Xn, int n, const float *__restrict__ Wd,
                                                          const float *__restrict__ Wn, int k_words, u64 *__restrict__ key) {
  const int q0 = (int)blockIdx.x * LM_QROWS, c0 = (int)blockIdx.y * LW_CHUNK, c1 = min(k_words, c0 + LW_CHUNK);
  const u64 b = loop_words_walk<K>(X, Xn, n, q0, Wd, Wn, c0, c1);
  const int tid = (int)threadIdx.x;
  if (tid < LM_QROWS && q0 + tid < n) atomicMin(key + q0 + tid, b);
}

// One wave per point (grid-stride): lane k adds the fixed-point component k to the word's sum -- a wave instruction covers K-contiguous int64 of ONE row.
// Lane 0 counts the member and whether the word changed
__global__ __launch_bounds__(256) void vocab_accumulate_kernel(const float *__restrict__ X, int K, int n, int k_words, const u64 *__restrict__ key, int32_t *__restrict__ assign,
                                                              u64 *__restrict__ sum, int32_t *__restrict__ count, int32_t *__restrict__ changed) {
  const int lane = (int)(threadIdx.x & 63), nwaves = (int)(gridDim.x * 4u);
  int nchg = 0;
  for (int i = (int)((blockIdx.x * 256u + threadIdx.x) >> 6); i < n; i += nwaves) {
    const unsigned w = (unsigned)(key[i] & 0xffffffffull);                 // wave-uniform
    if (w >= (unsigned)k_words) continue;                                  // (never: every point met at least one centre)
    for (int k = lane; k < K; k += 64) {
      const long long q = __double2ll_rn((double)X[(size_t)i * K + k] * VS_Q_SCALE);
      atomicAdd(sum + (size_t)w * K + k, (u64)q);                          // two's complement: the int64 sum
    }
    if (lane == 0) {
      atomicAdd(count + w, 1);
      nchg += assign[i] != (int32_t)w ? 1 : 0;
      assign[i] = (int32_t)w;
    }
  }
  if (lane == 0 && nchg) atomicAdd(changed, nchg);
}

// one thread per (word, component); a word without members keeps its centre
__global__ __launch_bounds__(256) void vocab_update_kernel(int K, int k_words, const u64 *__restrict__ sum, const int32_t *__restrict__ count, float *__restrict__ words) {
  const int idx = (int)(blockIdx.x * 256u + threadIdx.x);                  // k_words * K <= 2^27
  if (idx >= k_words * K) return;
  const int cnt = count[idx / K];
  if (cnt > 0) words[idx] = (float)(((double)(long long)sum[idx] / (double)cnt) * VS_Q_INV);
}

// the assignment against the words as returned: word, d2, members per word, the fixed-point inertia
__global__ __launch_bounds__(256) void vocab_final_kernel(int n, int k_words, const u64 *__restrict__ key, int32_t *__restrict__ assign, float *__restrict__ d2out,
                                                         int32_t *__restrict__ count, u64 *__restrict__ inertia) {
  const int i = (int)(blockIdx.x * 256u + threadIdx.x);
  u64 q = 0;
  if (i < n) {
    const u64 k = key[i];
    const unsigned w = (unsigned)(k & 0xffffffffull);
    const float d2 = __uint_as_float((unsigned)(k >> 32));
    if (w < (unsigned)k_words) {
      assign[i] = (int32_t)w; d2out[i] = d2;
      atomicAdd(count + w, 1);
      q = (u64)((double)d2 * VS_W_SCALE);
    } else { assign[i] = -1; d2out[i] = 0.f; }                             // (never)
  }
  q = wave_sum(q);
  if ((threadIdx.x & 63) == 0 && q) atomicAdd(inertia, q);
}

// ---- host ---------------------------------------------------------------------------------------------------------------------------------------------------
namespace {
struct vocab_work {
  svs_ctx *ctx;
  DevBuf<float> d_X, d_Xn, d_words, d_wnorm, d_d2;
  DevBuf<u64> d_key, d_sum, d_W, d_bsum, d_inertia;
  DevBuf<double> d_w;
  DevBuf<int32_t> d_assign, d_count, d_changed, d_seed, d_state;
  PinnedBuf<int32_t> h_small;
  owned::Event ev[3];
  explicit vocab_work(svs_ctx *c) : ctx(c) {}
  ~vocab_work() { (void)hipStreamSynchronize(ctx->stream); }              // (before the members go, also when the call gives up)
};

int vocab_assign(svs_ctx *ctx, vocab_work &wk, int K, int n, int k) {
  SVS_HIP(ctx, hipMemsetAsync(wk.d_key, 0xff, (size_t)n * sizeof(u64), ctx->stream));
  hipLaunchKernelGGL(vocab_norm_kernel, dim3(div_up(k, 256)), dim3(256), 0, ctx->stream, wk.d_words, K, k, wk.d_wnorm);
  SVS_LAUNCH_CHECK(ctx);
  const dim3 grid(div_up(n, LM_QROWS), div_up(k, LW_CHUNK));
  if (K == 64) hipLaunchKernelGGL(vocab_assign_kernel<64>, grid, dim3(256), 0, ctx->stream, wk.d_X, wk.d_Xn, n, wk.d_words, wk.d_wnorm, k, wk.d_key);
  else hipLaunchKernelGGL(vocab_assign_kernel<128>, grid, dim3(256), 0, ctx->stream, wk.d_X, wk.d_Xn, n, wk.d_words, wk.d_wnorm, k, wk.d_key);
  SVS_LAUNCH_CHECK(ctx);
  return SVS_OK;
}
}  // namespace

extern "C" void svs_vocab_params_default(svs_vocab_params *p) {
  if (!p) return;
  p->n_words = 10000; p->iterations = 11; p->seed = 0; p->h_init = nullptr; p->drop_empty = 1;
}

extern "C" int svs_vocab_stage_times(svs_ctx *ctx, float *ms) {
  if (!ctx || !ms) return SVS_ERR_INVALID;
  for (int i = 0; i < 3; ++i) ms[i] = ctx->vocab_ms[i];
  return SVS_OK;
}

static bool vocab_rows_ok(const float *p, size_t count) {
  for (size_t i = 0; i < count; ++i)
    if (!(fabsf(p[i]) < 4.0f)) return false;                               // NaN and infinity fail the comparison too
  return true;
}

extern "C" int svs_vocab_train(svs_ctx *ctx, int desc_dim, int n, const float *h_desc, const svs_vocab_params *prm, float *h_words, svs_vocab_result *h_res,
                               int32_t *h_seed_index, int32_t *h_assign, float *h_assign_d2, int32_t *h_count, int32_t *h_changed) {
  SVS_REQUIRE(ctx, ctx && prm && h_desc && (desc_dim == 64 || desc_dim == 128) && n >= 1);
  SVS_REQUIRE(ctx, prm->n_words >= 1 && prm->iterations >= 0);
  if (n > SVS_VOCAB_MAX_POINTS || prm->n_words > SVS_LOOP_MAX_WORDS) {
    ctx->err = "svs_vocab_train: capacity exceeded (n <= SVS_VOCAB_MAX_POINTS, n_words <= SVS_LOOP_MAX_WORDS)";
    return SVS_ERR_CAPACITY;
  }
  SVS_REQUIRE(ctx, prm->n_words <= n);
  const int K = desc_dim, nw = prm->n_words, iters = prm->iterations;
  SVS_REQUIRE(ctx, vocab_rows_ok(h_desc, (size_t)n * K));                  // a component that is not finite, or |x| >= 4
  SVS_REQUIRE(ctx, !prm->h_init || vocab_rows_ok(prm->h_init, (size_t)nw * K));
  SVS_DEVICE(ctx);
  vocab_work wk(ctx);
  hipStream_t st = ctx->stream;
  const int nb = div_up(n, VS_BLOCK);
  SVS_HIP(ctx, wk.d_X.alloc((size_t)n * K));
  SVS_HIP(ctx, wk.d_Xn.alloc(n));
  SVS_HIP(ctx, wk.d_words.alloc((size_t)nw * K));
  SVS_HIP(ctx, wk.d_wnorm.alloc(nw));
  SVS_HIP(ctx, wk.d_d2.alloc(n));
  SVS_HIP(ctx, wk.d_key.alloc(n));
  SVS_HIP(ctx, wk.d_sum.alloc((size_t)nw * K));
  SVS_HIP(ctx, wk.d_inertia.alloc(1));
  SVS_HIP(ctx, wk.d_assign.alloc(n));
  SVS_HIP(ctx, wk.d_count.alloc(nw));
  SVS_HIP(ctx, wk.d_changed.alloc((size_t)std::max(iters, 1)));
  SVS_HIP(ctx, wk.d_seed.alloc(nw));
  SVS_HIP(ctx, wk.d_state.alloc(1));
  SVS_HIP(ctx, wk.h_small.alloc(4));
  for (int i = 0; i < 3; ++i) SVS_HIP(ctx, wk.ev[i].create());
  float ms_seed = 0.f, ms_assign = 0.f, ms_update = 0.f;

  SVS_HIP(ctx, hipMemcpyAsync(wk.d_X, h_desc, (size_t)n * K * sizeof(float), hipMemcpyHostToDevice, st));
  hipLaunchKernelGGL(vocab_norm_kernel, dim3(div_up(n, 256)), dim3(256), 0, st, wk.d_X, K, n, wk.d_Xn);
  SVS_LAUNCH_CHECK(ctx);

  // ---- 1. the start centres
  std::vector<int32_t> seed_index((size_t)nw, -1);
  int n_seeded = 0, k = nw;
  if (prm->h_init) {
    SVS_HIP(ctx, hipMemcpyAsync(wk.d_words, prm->h_init, (size_t)nw * K * sizeof(float), hipMemcpyHostToDevice, st));
  } else {
    SVS_HIP(ctx, wk.d_w.alloc(n));
    SVS_HIP(ctx, wk.d_W.alloc(n));
    SVS_HIP(ctx, wk.d_bsum.alloc(nb));
    const int i0 = (int)(((splitmix64(prm->seed) >> 32) * (uint64_t)(uint32_t)n) >> 32);
    SVS_HIP(ctx, hipEventRecord(wk.ev[0], st));
    hipLaunchKernelGGL(vocab_seed_init_kernel, dim3(std::min(div_up(std::max(n, nw), 256), 4096)), dim3(256), 0, st, n, nw, i0, wk.d_w, wk.d_seed, wk.d_state);
    SVS_LAUNCH_CHECK(ctx);
    for (int c = 1; c < nw; ++c) {                                         // two launches per centre, no host synchronisation
      hipLaunchKernelGGL(vocab_seed_weight_kernel, dim3(nb), dim3(VS_BLOCK), 0, st, wk.d_X, K, n, c, wk.d_seed, wk.d_w, wk.d_W, wk.d_bsum);
      hipLaunchKernelGGL(vocab_seed_pick_kernel, dim3(1), dim3(VS_PICK), 0, st, n, nb, c, prm->seed, wk.d_W, wk.d_bsum, wk.d_seed, wk.d_state);
    }
    SVS_LAUNCH_CHECK(ctx);
    hipLaunchKernelGGL(vocab_gather_kernel, dim3(div_up(nw * (K / 4), 256)), dim3(256), 0, st, wk.d_X, K, n, nw, wk.d_seed, wk.d_words);
    SVS_LAUNCH_CHECK(ctx);
    SVS_HIP(ctx, hipEventRecord(wk.ev[1], st));
    SVS_HIP(ctx, hipMemcpyAsync(seed_index.data(), wk.d_seed, (size_t)nw * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    SVS_HIP(ctx, hipMemcpyAsync(wk.h_small, wk.d_state, sizeof(int32_t), hipMemcpyDeviceToHost, st));
    SVS_HIP(ctx, hipStreamSynchronize(st));
    SVS_HIP(ctx, hipEventElapsedTime(&ms_seed, wk.ev[0], wk.ev[1]));
    n_seeded = wk.h_small[0] < 0 ? nw : std::min((int)wk.h_small[0], nw);
    k = n_seeded;
  }

  // ---- 2.-4. Lloyd iterations on k words
  std::vector<int32_t> changed((size_t)iters, -1);
  int iterations_run = 0, converged = 0;
  if (iters > 0) {
    SVS_HIP(ctx, hipMemsetAsync(wk.d_assign, 0xff, (size_t)n * sizeof(int32_t), st));      // -1: every point changes in iteration 0
    SVS_HIP(ctx, hipMemsetAsync(wk.d_changed, 0, (size_t)iters * sizeof(int32_t), st));
  }
  for (int t = 0; t < iters; ++t) {
    SVS_HIP(ctx, hipEventRecord(wk.ev[0], st));
    if (int rc = vocab_assign(ctx, wk, K, n, k)) return rc;
    SVS_HIP(ctx, hipEventRecord(wk.ev[1], st));
    SVS_HIP(ctx, hipMemsetAsync(wk.d_sum, 0, (size_t)k * K * sizeof(u64), st));
    SVS_HIP(ctx, hipMemsetAsync(wk.d_count, 0, (size_t)k * sizeof(int32_t), st));
    hipLaunchKernelGGL(vocab_accumulate_kernel, dim3(std::min(div_up(n, 4), 8192)), dim3(256), 0, st, wk.d_X, K, n, k, wk.d_key, wk.d_assign, wk.d_sum, wk.d_count,
                       wk.d_changed + t);
    SVS_LAUNCH_CHECK(ctx);
    hipLaunchKernelGGL(vocab_update_kernel, dim3(div_up(k * K, 256)), dim3(256), 0, st, K, k, wk.d_sum, wk.d_count, wk.d_words);
    SVS_LAUNCH_CHECK(ctx);
    SVS_HIP(ctx, hipEventRecord(wk.ev[2], st));
    SVS_HIP(ctx, hipMemcpyAsync(wk.h_small, wk.d_changed + t, sizeof(int32_t), hipMemcpyDeviceToHost, st));
    SVS_HIP(ctx, hipStreamSynchronize(st));
    float a = 0.f, b = 0.f;
    SVS_HIP(ctx, hipEventElapsedTime(&a, wk.ev[0], wk.ev[1]));
    SVS_HIP(ctx, hipEventElapsedTime(&b, wk.ev[1], wk.ev[2]));
    ms_assign += a; ms_update += b;
    changed[t] = wk.h_small[0];
    iterations_run = t + 1;
    if (changed[t] == 0) { converged = 1; break; }
  }

  // ---- 5. the words as returned, and the assignment against them
  std::vector<float> words((size_t)nw * K, 0.f);
  SVS_HIP(ctx, hipMemcpyAsync(words.data(), wk.d_words, (size_t)k * K * sizeof(float), hipMemcpyDeviceToHost, st));
  std::vector<int32_t> count((size_t)nw, 0);
  if (iterations_run > 0) SVS_HIP(ctx, hipMemcpyAsync(count.data(), wk.d_count, (size_t)k * sizeof(int32_t), hipMemcpyDeviceToHost, st));
  SVS_HIP(ctx, hipStreamSynchronize(st));
  int n_empty = 0, k_out = k;
  if (iterations_run > 0) {
    for (int j = 0; j < k; ++j) n_empty += count[j] == 0 ? 1 : 0;
    if (prm->drop_empty && n_empty) {
      k_out = 0;
      for (int j = 0; j < k; ++j)
        if (count[j] > 0) {
          if (k_out != j) memmove(&words[(size_t)k_out * K], &words[(size_t)j * K], (size_t)K * sizeof(float));
          ++k_out;
        }
      SVS_HIP(ctx, hipMemcpyAsync(wk.d_words, words.data(), (size_t)k_out * K * sizeof(float), hipMemcpyHostToDevice, st));
    }
  }
  std::fill(words.begin() + (size_t)k_out * K, words.end(), 0.f);
  if (int rc = vocab_assign(ctx, wk, K, n, k_out)) return rc;
  SVS_HIP(ctx, hipMemsetAsync(wk.d_count, 0, (size_t)nw * sizeof(int32_t), st));
  SVS_HIP(ctx, hipMemsetAsync(wk.d_inertia, 0, sizeof(u64), st));
  hipLaunchKernelGGL(vocab_final_kernel, dim3(div_up(n, 256)), dim3(256), 0, st, n, k_out, wk.d_key, wk.d_assign, wk.d_d2, wk.d_count, wk.d_inertia);
  SVS_LAUNCH_CHECK(ctx);
  u64 inertia = 0;
  if (h_assign) SVS_HIP(ctx, hipMemcpyAsync(h_assign, wk.d_assign, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost, st));
  if (h_assign_d2) SVS_HIP(ctx, hipMemcpyAsync(h_assign_d2, wk.d_d2, (size_t)n * sizeof(float), hipMemcpyDeviceToHost, st));
  if (h_count) SVS_HIP(ctx, hipMemcpyAsync(h_count, wk.d_count, (size_t)nw * sizeof(int32_t), hipMemcpyDeviceToHost, st));
  SVS_HIP(ctx, hipMemcpyAsync(&inertia, wk.d_inertia, sizeof(u64), hipMemcpyDeviceToHost, st));
  SVS_HIP(ctx, hipStreamSynchronize(st));
  if (h_words) memcpy(h_words, words.data(), words.size() * sizeof(float));
  if (h_seed_index) memcpy(h_seed_index, seed_index.data(), seed_index.size() * sizeof(int32_t));
  if (h_changed && iters > 0) memcpy(h_changed, changed.data(), changed.size() * sizeof(int32_t));
  if (h_res) {
    h_res->n_words_out = k_out; h_res->n_seeded = n_seeded; h_res->iterations_run = iterations_run; h_res->converged = converged; h_res->n_empty = n_empty;
    h_res->inertia_q28 = inertia;
  }
  ctx->vocab_ms[0] = ms_seed; ctx->vocab_ms[1] = ms_assign; ctx->vocab_ms[2] = ms_update;
  return SVS_OK;
}
