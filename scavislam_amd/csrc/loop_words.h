// loop_words.h -- the nearest-row walk that loop.hip (a visual word per descriptor, svs_loop_add_locations) and vocab.hip (the assignment step of
// svs_vocab_train) share, so that a (descriptor, word) pair gets the same d2 bits in both: one tile walk, one MFMA order, one way to form the squared norms.
#pragma once
#include "common.h"

constexpr int LM_QROWS = 32;            // query rows per workgroup: the N side of one 32x32 MFMA tile, one query per lane
constexpr int LM_TROWS = 128;           // train rows per LDS tile: 32 per wave
constexpr int LM_KC = 64;               // descriptor columns per LDS tile (K = 128: two tiles per train block, one accumulator)
constexpr int LM_LD4 = LM_KC / 4 + 1;   // tile row stride in float4 (one 16-byte slot of padding: fragment reads of 32 rows spread over the banks)
constexpr int LW_CHUNK = 2 * LM_TROWS;  // vocabulary rows per workgroup of the words walk

typedef float f32x16 __attribute__((ext_vector_type(16)));

// squared norm of a row of K floats: f64 sum of the exact f32 squares in component order, rounded once
__device__ __forceinline__ float loop_sqnorm(const float *__restrict__ rowp, int K) {
  const float4 *row = reinterpret_cast<const float4 *>(rowp);
  double s = 0.0;
  for (int k = 0; k < K / 4; ++k) {
    const float4 v = row[k];
    s += (double)v.x * (double)v.x; s += (double)v.y * (double)v.y; s += (double)v.z * (double)v.z; s += (double)v.w * (double)v.w;
  }
  return (float)s;
}

// One workgroup of 4 waves: query rows q0 .. q0 + 31 of Q [nq][K] (squared norms Qn) against rows c0 .. c1 - 1 of W (squared norms Wn; c1 - c0 <= LW_CHUNK is
// the callers' choice, not a limit).  The tile walk, the MFMA feeding and the per-pair arithmetic of loop_match_kernel (loop.hip), so a pair's d2 does not
// depend on the chunk or the batch it falls in.  A lane issues the eight 16-byte loads of its share of a tile together and stores them to LDS when they have
// arrived.  Returns, in threads 0 .. LM_QROWS - 1, the minimum over the chunk of the key (f32 bits of d2 << 32) | row index for query q0 + tid (~0 when the
// chunk is empty); the other threads return nothing of use.  Every thread of the workgroup must call it (barriers inside).
template <int K>
__device__ __forceinline__ unsigned long long loop_words_walk(const float *__restrict__ Q, const float *__restrict__ Qn, int nq, int q0, const float *__restrict__ W,
                                                              const float *__restrict__ Wn, int c0, int c1) {
  constexpr int NKC = K / LM_KC, PER = LM_TROWS * (LM_KC / 4) / 256;
  __shared__ float4 s_tile[LM_TROWS * LM_LD4];
  __shared__ float s_tnorm[LM_TROWS];
  __shared__ unsigned long long s_best[4][LM_QROWS];
  const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 31, hh = lane >> 5;
  const bool qok = q0 + r < nq;
  float4 qf[K / 8];
#pragma unroll
  for (int s = 0; s < K / 8; ++s)
    qf[s] = qok ? *reinterpret_cast<const float4 *>(Q + (size_t)(q0 + r) * K + 8 * s + 4 * hh) : make_float4(0.f, 0.f, 0.f, 0.f);
  const float qn = qok ? Qn[q0 + r] : 0.f;
  unsigned long long best = ~0ull;
  f32x16 acc;
  for (int t0 = c0; t0 < c1; t0 += LM_TROWS) {
    const bool mine = t0 + wave * 32 < c1;                                 // wave-uniform
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[e] = 0.f;
#pragma unroll
    for (int kc = 0; kc < NKC; ++kc) {                                     // (unrolled: the query fragment is indexed by constants and stays in registers)
      __syncthreads();                                                     // the previous tile has been read
      float4 ld[PER];                                                      // all eight loads of the lane in flight, then the stores
#pragma unroll
      for (int u = 0; u < PER; ++u) {
        const int i = tid + 256 * u, row = i >> 4, c4 = i & 15;
        ld[u] = t0 + row < c1 ? *reinterpret_cast<const float4 *>(W + (size_t)(t0 + row) * K + kc * LM_KC + 4 * c4) : make_float4(0.f, 0.f, 0.f, 0.f);
      }
      const float ldn = kc == 0 && tid < LM_TROWS && t0 + tid < c1 ? Wn[t0 + tid] : 0.f;
#pragma unroll
      for (int u = 0; u < PER; ++u) {
        const int i = tid + 256 * u;
        s_tile[(i >> 4) * LM_LD4 + (i & 15)] = ld[u];
      }
      if (kc == 0 && tid < LM_TROWS) s_tnorm[tid] = ldn;
      __syncthreads();
      if (mine) {
#pragma unroll
        for (int ss = 0; ss < LM_KC / 8; ++ss) {
          const float4 a = s_tile[(wave * 32 + r) * LM_LD4 + 2 * ss + hh], b = qf[kc * (LM_KC / 8) + ss];
          acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, b.x, acc, 0, 0, 0);
          acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, b.y, acc, 0, 0, 0);
          acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.z, b.z, acc, 0, 0, 0);
          acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.w, b.w, acc, 0, 0, 0);
        }
      }
    }
    if (mine) {
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int i = (e & 3) + 8 * (e >> 2) + 4 * hh, j = t0 + wave * 32 + i;
        float d2 = (qn + s_tnorm[wave * 32 + i]) - 2.f * acc[e];
        d2 = d2 < 0.f ? 0.f : d2;
        const unsigned long long key = ((unsigned long long)__float_as_uint(d2) << 32) | (unsigned)j;
        if (j < c1 && key < best) best = key;
      }
    }
  }
  {
    const unsigned long long o = __shfl_xor(best, 32, 64);
    best = o < best ? o : best;
  }
  if (lane < 32) s_best[wave][lane] = best;
  __syncthreads();
  unsigned long long b = ~0ull;
  if (tid < LM_QROWS) {
    b = s_best[0][tid];
#pragma unroll
    for (int w = 1; w < 4; ++w) b = s_best[w][tid] < b ? s_best[w][tid] : b;
  }
  return b;
}
