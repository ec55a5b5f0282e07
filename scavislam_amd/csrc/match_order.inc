// match_order.inc -- the order in which match_kernel3 takes the points of a stream; included by match.hip behind match_predict.inc, whose kernels write the
// bucket keys.  match_order_kernel.
//
// The caller's lists come in hash order (the reference iterates tr1::unordered_maps): four
// points that share a wave then sit anywhere in the image, every wave touches its own bitmap, key-patch and image lines, and the kernel runs at the miss
// rate of the vector L1 / L2.  A counting sort by (level, 16 x 16 pixel cell of the predicted position) makes neighbours in the order neighbours in the image
// (match 0.83 -> 0.69 ms per 512 x 2000 points) and collects the points that are not searched (behind the camera, outside the frame) in waves of their own.
// One workgroup per stream; the order inside a cell is whatever the atomics make it -- every point is matched on its own and written to its own record, so
// the results do not depend on it.
__global__ __launch_bounds__(256) void match_order_kernel(MatchParams M, int32_t *__restrict__ order) {
  __shared__ int s_cnt[ORD_MAX_BUCKETS + 1];
  __shared__ int s_part[256];
  const int slot = blockIdx.x, n = M.a.n_pts, tid = threadIdx.x, nb_tot = 3 * M.ord_nb + 1;
  const int32_t *keys = M.keys + (size_t)slot * n;
  for (int b = tid; b < nb_tot; b += 256) s_cnt[b] = 0;
  __syncthreads();
  auto bucket = [&](int ip) { return keys[ip]; };
  for (int ip = tid; ip < n; ip += 256) atomicAdd(&s_cnt[bucket(ip)], 1);
  __syncthreads();
  // exclusive scan of the bucket counts: every thread a contiguous run, then the runs' totals
  const int per = (nb_tot + 255) / 256, b0 = tid * per, b1 = min(nb_tot, b0 + per);
  int run = 0;
  for (int b = b0; b < b1; ++b) run += s_cnt[b];
  s_part[tid] = run;
  __syncthreads();
  if (tid == 0) { int acc = 0; for (int t = 0; t < 256; ++t) { const int c = s_part[t]; s_part[t] = acc; acc += c; } }
  __syncthreads();
  int acc = s_part[tid];
  for (int b = b0; b < b1; ++b) { const int c = s_cnt[b]; s_cnt[b] = acc; acc += c; }
  __syncthreads();
  for (int ip = tid; ip < n; ip += 256) order[(size_t)slot * n + atomicAdd(&s_cnt[bucket(ip)], 1)] = ip;
}
