// map_sets.h -- the set and scan idioms of the device-resident map, written once (device code only; map.hip includes it behind its constants and MapK, in front
// of its parts).  The map's design rests on them: sets are bitmaps over ids, a list is the set bits in ascending order, and the place of an id in a list is a
// popcount prefix -- over the words in front of it by a workgroup scan, inside its word by a mask -- so no atomic decides an order and every result is a function
// of the map's content alone.  A workgroup is MB_THREADS lanes; s_w is an LDS array of MB_THREADS / 64 ints that the caller lends.
#pragma once
namespace {
// ---- prefixes ---------------------------------------------------------------------------------------------------------------------------------------------------
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

// counts a[0 .. n) -> begin a[0 .. n] in place (entry n becomes the total), and a copy in cur as the fill cursors; ITEMS entries per lane and step, so the single
// workgroup's chain of barriers is n / (MB_THREADS * ITEMS) steps long.  ITEMS == 8 moves two 16-byte words where all eight exist (a and cur 16-byte aligned: a
// hipMalloc block).  Every lane of ONE workgroup calls it (block_excl_scan's barriers inside)
template <int ITEMS>
__device__ __forceinline__ void counts_to_begin(int32_t *a, int32_t *cur, int n, int *s_w) {
  static_assert(ITEMS == 1 || ITEMS == 8, "one entry, or two 16-byte words");
  int run = 0;
  for (int base = 0; base <= n; base += MB_THREADS * ITEMS) {      // block-uniform; entry n becomes the total
    const int i0 = base + threadIdx.x * ITEMS;                      // ITEMS == 8: a multiple of 8
    int v[ITEMS];
    if (ITEMS == 8 && i0 + ITEMS <= n) {
      if constexpr (ITEMS == 8) {
        const int4 lo = reinterpret_cast<const int4 *>(a + i0)[0], hi = reinterpret_cast<const int4 *>(a + i0)[1];
        v[0] = lo.x; v[1] = lo.y; v[2] = lo.z; v[3] = lo.w; v[4] = hi.x; v[5] = hi.y; v[6] = hi.z; v[7] = hi.w;
      }
    } else {
#pragma unroll
      for (int k = 0; k < ITEMS; ++k) v[k] = i0 + k < n ? a[i0 + k] : 0;
    }
    int sum = 0;
#pragma unroll
    for (int k = 0; k < ITEMS; ++k) { const int c = v[k]; v[k] = sum; sum += c; }
    int tot;
    const int off = run + block_excl_scan(sum, s_w, tot);
    if (ITEMS == 8 && i0 + ITEMS <= n + 1) {
      if constexpr (ITEMS == 8) {
        const int4 lo = make_int4(off + v[0], off + v[1], off + v[2], off + v[3]), hi = make_int4(off + v[4], off + v[5], off + v[6], off + v[7]);
        reinterpret_cast<int4 *>(a + i0)[0] = lo; reinterpret_cast<int4 *>(a + i0)[1] = hi;
        reinterpret_cast<int4 *>(cur + i0)[0] = lo; reinterpret_cast<int4 *>(cur + i0)[1] = hi;
      }
    } else {
#pragma unroll
      for (int k = 0; k < ITEMS; ++k)
        if (i0 + k <= n) { a[i0 + k] = off + v[k]; cur[i0 + k] = off + v[k]; }
    }
    run += tot;
  }
}

// ---- one atomic per distinct target of a wave --------------------------------------------------------------------------------------------------------------------
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

// ---- bitmaps over ids --------------------------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ bool bit_of(const uint32_t *s, int i) { return (s[i >> 5] >> (i & 31)) & 1u; }
// id joins the set (one atomic, LDS or global; any lane, no barrier inside: the caller puts one in front of the first read)
__device__ __forceinline__ void bit_set(uint32_t *s, int id) { atomicOr(&s[id >> 5], 1u << (id & 31)); }
// the set bits in front of id, where s_rank[w] holds the set bits of the words in front of word w (any lane, no barrier inside)
__device__ __forceinline__ int bit_rank(const uint32_t *s_bits, const int *s_rank, int id) {
  return s_rank[id >> 5] + __popc(s_bits[id >> 5] & ((1u << (id & 31)) - 1u));
}

// f(id, pos) for every set bit of one word, ascending: id = base + the bit, pos counts on from `rank`.  The one-word-per-lane lister of an LDS keyframe bitmap:
// base = tid << 5, rank = block_excl_scan(__popc(word), ..).  Any lane, no barrier inside
template <class F>
__device__ __forceinline__ void for_each_set_bit(uint32_t word, int base, int rank, F f) {
  while (word) {
    const int b = __ffs((int)word) - 1;
    word &= word - 1;
    f(base + b, rank);
    ++rank;
  }
}

// one trip of a lister: every lane brings a word (`base` = the id of its bit 0; the lanes' words ascend with the lane), f(id, pos) for its set bits with pos
// counting on from `start` over the whole workgroup; returns the workgroup's count.  Every lane of the workgroup calls it (block_excl_scan's barriers inside)
template <class F>
__device__ __forceinline__ int list_words(uint32_t word, int base, int start, int *s_w, F f) {
  int tot;
  const int pos = start + block_excl_scan(__popc(word), s_w, tot);
  for_each_set_bit(word, base, pos, f);
  return tot;
}

// the lister of a bitmap in global memory that this workgroup's atomics have just marked (behind a barrier): all n_words words of `mark` become ascending ids in
// out[off ..]; entries at or behind out[cap] are counted but not written.  Returns the count.  One trip per MB_THREADS words, so the trip count is block-uniform;
// the relaxed agent-scope load reads what the atomics left in the L2.  Every lane of the workgroup calls it (barriers inside)
__device__ __forceinline__ int list_marked(const uint32_t *mark, int n_words, int32_t *out, int off, int cap, int *s_w) {
  int n = 0;
  for (int base = 0; base < n_words; base += MB_THREADS) {      // block-uniform trip count
    const int w = base + threadIdx.x;
    const uint32_t bits = w < n_words ? __hip_atomic_load(&mark[w], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0u;
    n += list_words(bits, w << 5, off + n, s_w, [&](int id, int pos) { if (pos < cap) out[pos] = id; });
  }
  return n;
}

// ---- rows and records --------------------------------------------------------------------------------------------------------------------------------------------
// f(keyframe) for the entries [b, e) of an observer row, four loads in flight: a row is read at the latency of a quarter of its entries.  f also sees -1 up to
// three times behind the row's end.  Any lane
template <class F>
__device__ __forceinline__ void row_each(const int32_t *__restrict__ pt_rows, int b, int e, F f) {
  for (int i = b; i < e; i += 4) {
    int kf[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) kf[k] = i + k < e ? pt_rows[i + k] : -1;
#pragma unroll
    for (int k = 0; k < 4; ++k) f(kf[k]);
  }
}
// does the observer row [b, e) hold keyframe kf (kf >= 0)
__device__ __forceinline__ bool row_has(const int32_t *pt_rows, int b, int e, int kf) {
  bool found = false;
  row_each(pt_rows, b, e, [&](int k) { found |= k == kf; });
  return found;
}

// a 64-byte record (svs_candidate_point, svs_ba_edge) by four 16-byte loads and stores; fix(q) may change the fourth word -- the ids -- on its way, and that word
// is returned as stored
template <class F>
__device__ __forceinline__ int4 copy_rec64(void *dst, const void *src, F fix) {
  const int4 *s4 = reinterpret_cast<const int4 *>(src);
  int4 *d4 = reinterpret_cast<int4 *>(dst);
  int4 q = s4[3];
  fix(q);
  d4[0] = s4[0]; d4[1] = s4[1]; d4[2] = s4[2]; d4[3] = q;
  return q;
}
__device__ __forceinline__ int4 copy_rec64(void *dst, const void *src) { return copy_rec64(dst, src, [](int4 &) {}); }

// invert_depth (maths_utils.h:66-69) and back: psi = (x / z, y / z, 1 / z)
__device__ __forceinline__ void psi_of_xyz(const double *xyz, double *psi) {
  const double x = xyz[0], y = xyz[1], z = xyz[2];
  psi[0] = x / z; psi[1] = y / z; psi[2] = 1.0 / z;
}
__device__ __forceinline__ void xyz_of_psi(const double *psi, double *xyz) {
  const double u = psi[0], v = psi[1], q = psi[2];
  xyz[0] = u / q; xyz[1] = v / q; xyz[2] = 1.0 / q;
}
}  // namespace
