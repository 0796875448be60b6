// Per-step state that lives on the device (rings, queues, metric stores), so that a step captured into a hipGraph and replayed
// does what the eager step does: every position, count and offset is READ FROM device memory by the kernels below instead of
// being baked into the launch arguments by the host.  Each entry point is a copy launch that reads the old position, followed
// (stream order) by a one-thread launch that advances it: no workgroup ever reads a position another one may already have moved.
// Plain C++ stores only.

// position of a ring of Q slots held in device memory (a stale or foreign value is folded into [0, Q))
__device__ __forceinline__ long long ring_pos(const long long* ptr, int Q) {
  long long p = ptr[0] % Q;
  return p < 0 ? p + Q : p;
}

// rows [n, D] -> slots of the ring: layout 1 = bank [D, Q] (slot = column), 0 = bank [Q, D] (slot = row).
// mode 0 = truncate at the ring end (the first min(n, Q - p) rows), 1 = wrap (row i -> slot (p + i) % Q, n <= Q).
__global__ __launch_bounds__(256) void ring_copy_kernel(float* __restrict__ bank, const float* __restrict__ rows, int n, int D, int Q,
                                                        int layout, int mode, const long long* __restrict__ ptr) {
  const long long p = ring_pos(ptr, Q);
  const int m = mode == 0 ? (int)min((long long)n, Q - p) : n;
  const long total = (long)m * D;
  for (long e = (long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (long)gridDim.x * blockDim.x) {
    const int i = (int)(e / D), d = (int)(e % D);
    const long long slot = mode == 0 ? p + i : (p + i) % Q;
    if (layout) bank[(long)d * Q + slot] = rows[e];
    else bank[slot * D + d] = rows[e];
  }
}

__global__ void ring_advance_kernel(long long* __restrict__ ptr, long long* __restrict__ count, int n, int Q, int mode) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  const long long p = ring_pos(ptr, Q);
  const long long m = mode == 0 ? min((long long)n, Q - p) : (long long)n;
  ptr[0] = (p + m) % Q;
  if (count) count[0] = min(count[0] + m, (long long)Q);
}

extern "C" int stil_ring_enqueue(float* bank, const float* rows, int n, int D, int Q, int layout, int mode, long long* ptr,
                                 long long* count, int advance, void* stream) {
  STIL_REQUIRE(bank && rows && ptr && n > 0 && D > 0 && Q > 0 && (layout == 0 || layout == 1) && (mode == 0 || mode == 1),
               "stil_ring_enqueue: bad arguments");
  STIL_REQUIRE(mode == 0 || n <= Q, "stil_ring_enqueue: %d rows wrap over a ring of %d slots", n, Q);
  hipStream_t s = (hipStream_t)stream;
  const long total = (long)n * D;
  hipLaunchKernelGGL(ring_copy_kernel, dim3(min(cdiv(total, 256), 1024)), dim3(256), 0, s, bank, rows, n, D, Q, layout, mode,
                     (const long long*)ptr);
  STIL_LAUNCH_CHECK();
  if (advance) {
    hipLaunchKernelGGL(ring_advance_kernel, dim3(1), dim3(64), 0, s, ptr, count, n, Q, mode);
    STIL_LAUNCH_CHECK();
  }
  return STIL_OK;
}

// out[k] = (sum over the first r = min(count, L) rows of queue[:, k]) * (float)(1 / r): the association of stil_colsum over r rows
// (128-row chunks of four row lanes, each lane two interleaved sums; chunk c added into lane c % 8, the eight lanes in order), so the
// bits are stil_colsum's with M = r and scale = 1 / r.  One thread per column.
__global__ __launch_bounds__(256) void queue_mean_kernel(const float* __restrict__ q, int L, int K, const long long* __restrict__ count,
                                                         float* __restrict__ out) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= K) return;
  const long long cnt = count[0];
  const int M = (int)(cnt < 0 ? 0 : (cnt > L ? L : cnt));
  if (M == 0) { out[c] = 0.f; return; }
  const int nch = (M + 127) / 128;
  float lane[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  for (int ch = 0; ch < nch; ++ch) {
    const int m0 = ch * 128, m1 = min(M, m0 + 128);
    float part = 0.f;
    for (int rl = 0; rl < 4; ++rl) {
      float s0 = 0.f, s1 = 0.f;
      int m = m0 + rl;
      for (; m + 4 < m1; m += 8) { s0 += q[(long)m * K + c]; s1 += q[(long)(m + 4) * K + c]; }
      for (; m < m1; m += 4) s0 += q[(long)m * K + c];
      part = rl == 0 ? s0 + s1 : part + (s0 + s1);
    }
    lane[ch & 7] += part;
  }
  float t = 0.f;
  for (int l = 0; l < 8; ++l) t += lane[l];
  out[c] = t * (float)(1.0 / (double)M);
}

extern "C" int stil_queue_mean(const float* queue, int L, int K, const long long* count, float* out, void* stream) {
  STIL_REQUIRE(queue && count && out && L > 0 && K > 0, "stil_queue_mean: bad arguments");
  hipLaunchKernelGGL(queue_mean_kernel, dim3(cdiv(K, 256)), dim3(256), 0, (hipStream_t)stream, queue, L, K, count, out);
  STIL_LAUNCH_CHECK();
  return STIL_OK;
}

// append n score rows [n, K] and their targets at row count[0] of a store of `capacity` rows; rows past the capacity are dropped
__global__ __launch_bounds__(256) void rows_append_kernel(const float* __restrict__ src, const long long* __restrict__ tgt, int n, int K,
                                                          float* __restrict__ dst, long long* __restrict__ dst_tgt, int capacity,
                                                          const long long* __restrict__ count) {
  const long long c0 = count[0];
  const long total = (long)n * K;
  for (long e = (long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (long)gridDim.x * blockDim.x) {
    const long long r = c0 + e / K;
    if (r >= 0 && r < capacity) {
      dst[r * K + e % K] = src[e];
      if (e % K == 0) dst_tgt[r] = tgt[e / K];
    }
  }
}

__global__ void rows_advance_kernel(long long* __restrict__ count, int* __restrict__ overflow, int n, int capacity) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  const long long c = count[0] + n;
  if (c > capacity) overflow[0] = 1;
  count[0] = c;
}

extern "C" int stil_rows_append(const float* src, const long long* target, int n, int K, float* dst, long long* dst_target,
                                int capacity, long long* count, int* overflow, void* stream) {
  STIL_REQUIRE(src && target && dst && dst_target && count && overflow && n > 0 && K > 0 && capacity > 0,
               "stil_rows_append: bad arguments");
  hipStream_t s = (hipStream_t)stream;
  const long total = (long)n * K;
  hipLaunchKernelGGL(rows_append_kernel, dim3(min(cdiv(total, 256), 1024)), dim3(256), 0, s, src, target, n, K, dst, dst_target,
                     capacity, (const long long*)count);
  STIL_LAUNCH_CHECK();
  hipLaunchKernelGGL(rows_advance_kernel, dim3(1), dim3(64), 0, s, count, overflow, n, capacity);
  STIL_LAUNCH_CHECK();
  return STIL_OK;
}
