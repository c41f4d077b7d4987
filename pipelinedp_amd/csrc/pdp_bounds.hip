// pdp_bounds.hip — the device half of DPEngine.calculate_private_contribution_bounds
// (gfx950; pipeline_dp/dp_engine.py:450-502, private_contribution_bounds.py):
//   k_filter_rows        DPEngine._drop_partitions on dense columns: the rows
//                        whose partition is allowed, compacted into two output
//                        columns in ONE pass over the 16 B/row.  A workgroup
//                        takes tiles of kFilterTile rows (4 consecutive rows
//                        per thread, two 16-byte loads per column), scans its
//                        keep counts in LDS and reserves the tile's output
//                        range with one integer atomicAdd on the device
//                        counter.  Rows keep their order within a tile; tiles
//                        land in the order their atomics arrive, so the output
//                        order is NOT stable across tiles (the dataset
//                        histograms that read it do not depend on it).
//   k_l0_impact_dropped  L0ScoringFunction._l0_impact_dropped for every
//                        candidate bound at once, from the dense L0 histogram
//                        count row: one wave per candidate, lanes striding over
//                        the bins, a wave reduction; integer and exact.
#include "pdp_internal.h"

namespace pdp {
namespace {

constexpr int kFilterThreads = 512;
constexpr int kFilterRows = 4;  // consecutive rows per thread
constexpr int kFilterTile = kFilterThreads * kFilterRows;
constexpr int kFilterMaxGrid = 2048;  // 256 CUs x 4 workgroups of 512 threads, x 2

// VEC: both columns are 16-byte aligned, so a thread's 4 rows are two
// longlong2 loads per column (a tile starts at a multiple of 4 rows)
template <bool VEC>
__global__ void __launch_bounds__(kFilterThreads) k_filter_rows(const int64_t* __restrict__ pid,
                                                                const int64_t* __restrict__ pk,
                                                                const uint8_t* __restrict__ allowed, int64_t n,
                                                                int64_t P, int64_t* __restrict__ out_pid,
                                                                int64_t* __restrict__ out_pk,
                                                                unsigned long long* out_count, unsigned* err) {
  __shared__ unsigned wsum[kFilterThreads / 64];
  __shared__ unsigned long long tile_base;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int64_t n_tiles = (n + kFilterTile - 1) / kFilterTile;
  bool bad = false;
  for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {  // workgroup-uniform
    const int64_t i0 = tile * kFilterTile + (int64_t)threadIdx.x * kFilterRows;
    int64_t u[kFilterRows], k[kFilterRows];
    if (VEC && i0 + kFilterRows <= n) {
#pragma unroll
      for (int q = 0; q < kFilterRows; q += 2) {
        const longlong2 a = ld_nt(reinterpret_cast<const longlong2*>(pid + i0 + q));
        const longlong2 b = ld_nt(reinterpret_cast<const longlong2*>(pk + i0 + q));
        u[q] = a.x; u[q + 1] = a.y;
        k[q] = b.x; k[q + 1] = b.y;
      }
    } else {
#pragma unroll
      for (int q = 0; q < kFilterRows; ++q) {
        const bool in = i0 + q < n;
        u[q] = in ? pid[i0 + q] : 0;
        k[q] = in ? pk[i0 + q] : -1;  // past the end: not a row
      }
    }
    bool keep[kFilterRows];
    unsigned c = 0;
#pragma unroll
    for (int q = 0; q < kFilterRows; ++q) {
      const bool row = i0 + q < n;
      const bool in_range = (uint64_t)k[q] < (uint64_t)P;  // the mask is read only inside [0, P)
      bad |= row && !in_range;
      keep[q] = row && in_range && allowed[in_range ? k[q] : 0] != 0;
      c += keep[q];
    }
    // exclusive scan of c over the workgroup
    unsigned inc = c;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
      const unsigned y = __shfl_up(inc, off, 64);
      if (lane >= off) inc += y;
    }
    if (lane == 63) wsum[w] = inc;
    __syncthreads();
    unsigned before = 0, total = 0;
#pragma unroll
    for (int j = 0; j < kFilterThreads / 64; ++j) {
      const unsigned s = wsum[j];
      before += j < w ? s : 0u;
      total += s;
    }
    if (threadIdx.x == 0 && total) tile_base = atomicAdd(out_count, (unsigned long long)total);
    __syncthreads();  // tile_base written; wsum read by every thread
    if (total) {
      int64_t pos = (int64_t)tile_base + before + inc - c;  // < n: at most n rows are kept in all
#pragma unroll
      for (int q = 0; q < kFilterRows; ++q) {
        if (keep[q]) {
          out_pid[pos] = u[q];
          out_pk[pos] = k[q];
          ++pos;
        }
      }
    }
    // no barrier here: the next tile writes wsum only after every thread has
    // passed the barrier above (its wsum reads are before it), and tile_base
    // only after the next tile's first barrier, which this thread reaches
    // after its read of tile_base
  }
  if (bad) atomicOr(err, 1u);
}

// lower bound of dense logarithmic bin b (pdp_dataset_histograms), capped at
// B <= 2^32: bins with e >= 10 have lower >= 1e12 > B
__device__ __forceinline__ long long capped_lower(int b, long long B) {
  if (b < 1000) return b < B ? b : B;
  const int e = (b - 1000) / 900 + 1;
  if (e >= 10) return B;
  long long lower = (b - 1000) % 900 + 100;
  for (int j = 0; j < e; ++j) lower *= 10;
  return lower < B ? lower : B;
}

constexpr int kScoreThreads = 256;

__global__ void __launch_bounds__(kScoreThreads) k_l0_impact_dropped(const int64_t* __restrict__ count, long long B,
                                                                     const int64_t* __restrict__ cand, int64_t m,
                                                                     int64_t* __restrict__ dropped) {
  const int lane = threadIdx.x & 63;
  const int64_t c = (int64_t)blockIdx.x * (kScoreThreads / 64) + (threadIdx.x >> 6);  // wave-uniform
  if (c >= m) return;
  long long k = cand[c];
  k = k < 0 ? 0 : k;
  unsigned long long sum = 0;
  for (int b = lane; b < PDP_HIST_LOG_BINS; b += 64) {
    const long long n = count[b];
    if (n == 0) continue;
    const long long lo = capped_lower(b, B);
    if (lo > k) sum += (unsigned long long)(lo - k) * (unsigned long long)n;
  }
  for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o, 64);
  if (lane == 0) dropped[c] = (int64_t)sum;
}

}  // namespace
}  // namespace pdp

using namespace pdp;

extern "C" {

int pdp_filter_rows_workspace_bytes(int64_t n_rows, uint64_t* bytes) {
  if (bytes == nullptr || n_rows < 0) return set_error(PDP_E_INVALID, "pdp_filter_rows_workspace_bytes: bad argument");
  *bytes = 256;  // the error word
  return PDP_OK;
}

int pdp_filter_rows(const int64_t* privacy_id, const int64_t* partition, const uint8_t* allowed, int64_t n_rows,
                    int64_t n_partitions, int64_t* out_privacy_id, int64_t* out_partition, int64_t* out_count,
                    void* workspace, uint64_t workspace_bytes, void* stream) {
  if (n_rows < 0) return set_error(PDP_E_INVALID, "pdp_filter_rows: n_rows must be >= 0");
  if (n_partitions < 1) return set_error(PDP_E_INVALID, "pdp_filter_rows: n_partitions must be >= 1");
  if (out_count == nullptr) return set_error(PDP_E_INVALID, "pdp_filter_rows: out_count is NULL");
  if (workspace == nullptr || workspace_bytes < 256) return set_error(PDP_E_WORKSPACE, "workspace too small");
  hipStream_t st = (hipStream_t)stream;
  PDP_HIP_CHECK(hipMemsetAsync(workspace, 0, 16, st));
  PDP_HIP_CHECK(hipMemsetAsync(out_count, 0, 8, st));
  if (n_rows == 0) return PDP_OK;
  if (privacy_id == nullptr || partition == nullptr || allowed == nullptr || out_privacy_id == nullptr ||
      out_partition == nullptr)
    return set_error(PDP_E_INVALID, "pdp_filter_rows: NULL column");
  const int64_t n_tiles = (n_rows + kFilterTile - 1) / kFilterTile;
  const unsigned grid = (unsigned)(n_tiles < kFilterMaxGrid ? n_tiles : kFilterMaxGrid);
  const bool vec = (((uintptr_t)privacy_id | (uintptr_t)partition) & 15) == 0;
  return launch("k_filter_rows", vec ? k_filter_rows<true> : k_filter_rows<false>, dim3(grid), dim3(kFilterThreads), 0,
                st, privacy_id, partition, allowed, n_rows, n_partitions, out_privacy_id, out_partition,
                (unsigned long long*)out_count, (unsigned*)workspace);
}

int pdp_l0_impact_dropped(const int64_t* l0_count, int64_t upper_bound, const int64_t* candidates,
                          int64_t n_candidates, int64_t* dropped, void* stream) {
  if (n_candidates < 0 || upper_bound < 0) return set_error(PDP_E_INVALID, "pdp_l0_impact_dropped: bad argument");
  if (upper_bound > ((int64_t)1 << 32))
    return set_error(PDP_E_UNSUPPORTED, "pdp_l0_impact_dropped: upper_bound above 2^32 (rows * bound may pass 2^63)");
  if (n_candidates == 0) return PDP_OK;
  if (l0_count == nullptr || candidates == nullptr || dropped == nullptr)
    return set_error(PDP_E_INVALID, "pdp_l0_impact_dropped: NULL argument");
  hipStream_t st = (hipStream_t)stream;
  const int per_block = kScoreThreads / 64;
  const int64_t grid = (n_candidates + per_block - 1) / per_block;
  if (grid > 0x7FFFFFFF) return set_error(PDP_E_UNSUPPORTED, "pdp_l0_impact_dropped: too many candidates");
  return launch("k_l0_impact_dropped", k_l0_impact_dropped, dim3((unsigned)grid), dim3(kScoreThreads), 0, st, l0_count,
                (long long)upper_bound, candidates, n_candidates, dropped);
}

}  // extern "C"
