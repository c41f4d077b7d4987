// pdp_scan.hip -- device-wide exclusive scan of u32 counts (scan_u32), shared
// by the bounding passes and the pair-table path.
#include "pdp_bound_keys.h"

namespace pdp {
namespace {

// exclusive scan of u32 counts[0..n) in place, total -> counts[n]
__global__ void __launch_bounds__(kBlock) k_scan_chunks(const unsigned* __restrict__ v, int64_t n,
                                                        unsigned* __restrict__ chunk_sums) {
  __shared__ unsigned red[kBlock / 64];
  const int64_t base = (int64_t)blockIdx.x * kScanChunk + (int64_t)threadIdx.x * kScanItems;
  unsigned s = 0;
#pragma unroll
  for (int t = 0; t < kScanItems; ++t)
    if (base + t < n) s += v[base + t];
  for (int off = 32; off > 0; off >>= 1) s += __shfl_down(s, off, 64);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned t = 0;
    for (int w = 0; w < kBlock / 64; ++w) t += red[w];
    chunk_sums[blockIdx.x] = t;
  }
}

__global__ void __launch_bounds__(kBlock) k_scan_top(unsigned* chunk_sums, int64_t n_chunks) {
  __shared__ unsigned part[kBlock];
  __shared__ unsigned carry;
  if (threadIdx.x == 0) carry = 0;
  __syncthreads();
  for (int64_t base = 0; base < n_chunks; base += kBlock) {
    const int64_t i = base + threadIdx.x;
    const unsigned x = i < n_chunks ? chunk_sums[i] : 0;
    part[threadIdx.x] = x;
    __syncthreads();
    for (int off = 1; off < kBlock; off <<= 1) {
      const unsigned t = threadIdx.x >= off ? part[threadIdx.x - off] : 0;
      __syncthreads();
      part[threadIdx.x] += t;
      __syncthreads();
    }
    if (i < n_chunks) chunk_sums[i] = carry + part[threadIdx.x] - x;
    __syncthreads();
    if (threadIdx.x == kBlock - 1) carry += part[kBlock - 1];
    __syncthreads();
  }
  if (threadIdx.x == 0) chunk_sums[n_chunks] = carry;
}

__global__ void __launch_bounds__(kBlock) k_scan_apply(unsigned* v, int64_t n,
                                                       const unsigned* __restrict__ chunk_sums,
                                                       int64_t n_chunks) {
  __shared__ unsigned part[kBlock];
  const int64_t base = (int64_t)blockIdx.x * kScanChunk + (int64_t)threadIdx.x * kScanItems;
  unsigned loc[kScanItems];
  unsigned s = 0;
#pragma unroll
  for (int t = 0; t < kScanItems; ++t) {
    loc[t] = base + t < n ? v[base + t] : 0;
    s += loc[t];
  }
  part[threadIdx.x] = s;
  __syncthreads();
  for (int off = 1; off < kBlock; off <<= 1) {
    const unsigned t = threadIdx.x >= off ? part[threadIdx.x - off] : 0;
    __syncthreads();
    part[threadIdx.x] += t;
    __syncthreads();
  }
  unsigned run = chunk_sums[blockIdx.x] + part[threadIdx.x] - s;
#pragma unroll
  for (int t = 0; t < kScanItems; ++t) {
    if (base + t < n) v[base + t] = run;
    run += loc[t];
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) v[n] = chunk_sums[n_chunks];
}

// the same scan in one launch for n <= kScanSmallMax (bucket offsets: C2 1,954
// and C3 4,928 entries), 16 consecutive entries per thread
constexpr int kScanSmallThreads = 1024;
constexpr int64_t kScanSmallMax = (int64_t)kScanSmallThreads * kScanItems;
__global__ void __launch_bounds__(kScanSmallThreads) k_scan_small(unsigned* v, int64_t n) {
  __shared__ unsigned wsum[kScanSmallThreads / 64 + 1];
  const int64_t base = (int64_t)threadIdx.x * kScanItems;
  unsigned loc[kScanItems];
  unsigned s = 0;
#pragma unroll
  for (int t = 0; t < kScanItems; ++t) {
    loc[t] = base + t < n ? v[base + t] : 0u;
    s += loc[t];
  }
  unsigned total;
  unsigned run = block_excl_scan(s, wsum, &total);
#pragma unroll
  for (int t = 0; t < kScanItems; ++t) {
    if (base + t < n) v[base + t] = run;
    run += loc[t];
  }
  if (threadIdx.x == 0) v[n] = total;
}

}  // namespace

int64_t scan_chunk_sums_len(int64_t n) { return (n + kScanChunk - 1) / kScanChunk + 1; }

int scan_u32(unsigned* v, int64_t n, unsigned* chunk_sums, hipStream_t st) {
  const int64_t n_chunks = (n + kScanChunk - 1) / kScanChunk;
  if (n_chunks == 0) return set_error(PDP_E_INVALID, "scan of an empty array");
  if (n <= kScanSmallMax) return launch("k_scan_small", k_scan_small, dim3(1), dim3(kScanSmallThreads), 0, st, v, n);
  int rc = launch("k_scan_chunks", k_scan_chunks, dim3((unsigned)n_chunks), dim3(kBlock), 0, st, v, n, chunk_sums);
  if (rc != PDP_OK) return rc;
  rc = launch("k_scan_top", k_scan_top, dim3(1), dim3(kBlock), 0, st, chunk_sums, n_chunks);
  if (rc != PDP_OK) return rc;
  return launch("k_scan_apply", k_scan_apply, dim3((unsigned)n_chunks), dim3(kBlock), 0, st, v, n, chunk_sums, n_chunks);
}

}  // namespace pdp
