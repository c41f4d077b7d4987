// pdp_analysis_report.hip — the cross-partition stage of utility analysis
// (analysis/cross_partition_combiners.py and the grouping by partition size of
// analysis/utility_analysis.py of the reference): the [P][K] outputs of
// pdp_utility_analysis folded into one report per configuration and bucket of
// partition size, read where they lie.
//
//   k_ur_keys      partition -> sort key: its bucket (the largest bound <= its
//                  size), or kUrBuckets when it takes no part
//                  (raw_statistics[p][0] <= 0); the integer counts per bucket
//                  by integer atomics
//   k_ur_hist / k_ur_scatter
//                  one stable tile sort pass (pdp_segments.h) of the partition
//                  indices by key (39 keys), so a bucket's run holds its
//                  partitions ascending
//   k_ur_reduce    lanes across configurations: one wave per (tile of kUrTile
//                  partitions of one bucket's run, metric, chunk of 64
//                  configurations) forms the per-partition terms and keeps 20
//                  fp64 sums per lane (+ 3 selection sums in metric slot 0);
//                  every [P][K] read is 512 contiguous bytes per wave
//   k_ur_combine   one wave per (bucket, field, chunk): adds the bucket's tile
//                  partials in tile order
//   k_ur_final     the all-partitions entry from the buckets' unscaled sums in
//                  bucket order, and _average_utility_report's scaling
// No floating-point atomic, and every order of summation is fixed: two runs
// give the same bits.  Every product, sum, quotient and root is rounded on its
// own (no fused multiply-add), so a term equals its NumPy expression bit for bit.
#include "pdp_segments.h"

#pragma clang fp contract(off)

namespace pdp {
namespace {

constexpr int kUrBuckets = PDP_UA_REPORT_BUCKETS;
constexpr int kUrKeys = kUrBuckets + 1;  // the last key: takes no part
constexpr int kUrSortTile = 2048;        // partitions per sort tile
// partitions per reduce work item: a wave keeps 23 fp64 sums (46 VGPRs) beside
// one partition's terms, far under the 128 VGPRs of 4 waves per SIMD, so the
// tile is chosen for parallelism: 1e5 partitions give ~800 tiles per metric and
// chunk, and the partials are 1/128 of the bytes read
constexpr int kUrTile = 128;
constexpr int kUrSel = 3;      // sum w, sum keep, sum keep (1 - keep)
constexpr int kUrPerMetric = 20;  // sum_actual, 3 dropped, 8 absolute, 8 relative

// BUCKET_BOUNDS of analysis/utility_analysis.py: [0, 1] + [1, 2, 5] 10^i, i = 1..12
__constant__ double kUrBounds[kUrBuckets] = {
    0.0,  1.0,  1e1,  2e1,  5e1,  1e2,  2e2,  5e2,  1e3,  2e3,  5e3,  1e4,  2e4,  5e4,  1e5,  2e5,  5e5,  1e6,  2e6,
    5e6,  1e7,  2e7,  5e7,  1e8,  2e8,  5e8,  1e9,  2e9,  5e9,  1e10, 2e10, 5e10, 1e11, 2e11, 5e11, 1e12, 2e12, 5e12};

struct RWs {
  uint64_t sn, key, order, hist, chunks, partial, sums, total;
};

inline int ur_fields(int M) { return kUrSel + kUrPerMetric * M; }
inline int64_t ur_sort_tiles(int64_t P) { return seg_tiles<kUrSortTile>(P); }
// the buckets' runs are tiled one by one: at most one ragged tile per bucket
inline int64_t ur_max_tiles(int64_t P) { return P / kUrTile + kUrBuckets; }

RWs rlayout(int64_t P, int K, int flags) {
  RWs w{};
  const int M = ua_n_metrics(flags);
  const uint64_t hist_len = (uint64_t)kUrKeys * (uint64_t)ur_sort_tiles(P);
  const uint64_t FK = (uint64_t)ur_fields(M) * (uint64_t)K * 8;
  uint64_t off = 0;
  w.sn = off; off = align256(off + (uint64_t)(M > 0 ? M : 1) * (uint64_t)K * 8);
  w.key = off; off = align256(off + (uint64_t)P);
  w.order = off; off = align256(off + (uint64_t)P * 4);
  w.hist = off; off = align256(off + (hist_len + 1) * 4);
  w.chunks = off; off = align256(off + (uint64_t)scan_chunk_sums_len((int64_t)hist_len) * 4);
  w.partial = off; off = align256(off + (uint64_t)ur_max_tiles(P) * FK);
  w.sums = off; off = align256(off + (uint64_t)kUrBuckets * FK);
  w.total = off;
  return w;
}

// ------------------------------------------------------------------ sort --
// the largest bound <= size; below 0 (and NaN) bucket 0, at or above 5e12 the last
__device__ __forceinline__ int ur_bucket(double size) {
  int b = 0;
  for (int i = 1; i < kUrBuckets; ++i)
    if (kUrBounds[i] <= size) b = i;
  return b;
}

__global__ void __launch_bounds__(kBlock) k_ur_keys(int64_t P, int K, const long long* __restrict__ raw,
                                                    const double* __restrict__ size_metric, int is_public,
                                                    unsigned char* key, unsigned long long* counts) {
  __shared__ unsigned c[kUrBuckets][2];
  for (int i = threadIdx.x; i < kUrBuckets * 2; i += kBlock) (&c[0][0])[i] = 0;
  __syncthreads();
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  // a block sees at most 2^31 partitions: the u32 counters cannot wrap
  for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p < P; p += stride) {
    const long long ids = raw[2 * p];
    int b = kUrBuckets;
    if (ids > 0) {
      b = ur_bucket(size_metric != nullptr ? size_metric[(uint64_t)p * (uint64_t)K] : (double)ids);
      atomicAdd(&c[b][is_public && raw[2 * p + 1] == 0 ? 1 : 0], 1u);
    }
    key[p] = (unsigned char)b;
  }
  __syncthreads();
  for (int i = threadIdx.x; i < kUrBuckets * 2; i += kBlock) {
    const unsigned v = (&c[0][0])[i];
    if (v != 0) atomicAdd(counts + i, (unsigned long long)v);
  }
}

// the counting sort's digit is the key; only the partition's index moves
struct UrEmit {
  unsigned* order;
  __device__ void operator()(int64_t i, unsigned, unsigned pos) const { order[pos] = (unsigned)i; }
};

// ---------------------------------------------------------------- reduce --
// After the scan hist[key * n_tiles] is the first sorted position of `key`.
__device__ __forceinline__ int64_t ur_start(const unsigned* __restrict__ hist, int64_t n_tiles, int key, int64_t P) {
  const int64_t s = (int64_t)hist[(int64_t)key * n_tiles];
  return s < P ? s : P;
}
__device__ __forceinline__ int64_t ur_tiles_of(int64_t n) { return (n + kUrTile - 1) / kUrTile; }

__device__ __forceinline__ int ur_bcast(unsigned v, int j) {
  return __builtin_amdgcn_readlane((int)v, j);
}

struct UrIn {
  const double* keep;     // [P][K], NULL with public partitions
  const double* metrics;  // [M][5][P][K]
  const double* sn;       // [M][K] (workspace)
};

// Work item (tile, metric slot m = blockIdx.z, configuration chunk blockIdx.y):
// partial[tile][f][k] for the slot's fields f (slot 0 also writes the selection
// sums).  With no metric there is one slot, which writes the selection sums only.
template <bool METRIC>
__global__ void __launch_bounds__(kBlock) k_ur_reduce(int64_t P, int K, int F, UrIn in,
                                                      const unsigned* __restrict__ order,
                                                      const unsigned* __restrict__ hist, int64_t n_tiles,
                                                      double* partial) {
  const int lane = (int)(threadIdx.x & 63), wave = (int)(threadIdx.x >> 6);
  const int k = (int)blockIdx.y * 64 + lane;
  const bool active = k < K;
  const int m = (int)blockIdx.z;
  const int64_t item = (int64_t)blockIdx.x * (kBlock / 64) + wave;
  // the bucket whose run holds tile `item`, and the tile's place in the run
  int64_t t = item, a = 0, e = 0;
  bool found = false;
  for (int b = 0; b < kUrBuckets && !found; ++b) {
    const int64_t s0 = ur_start(hist, n_tiles, b, P), s1 = ur_start(hist, n_tiles, b + 1, P);
    const int64_t tiles = s1 > s0 ? ur_tiles_of(s1 - s0) : 0;
    if (t < tiles) {
      a = s0 + t * kUrTile;
      e = a + kUrTile < s1 ? a + kUrTile : s1;
      found = true;
    } else {
      t -= tiles;
    }
  }
  if (!found) return;
  const double sn = METRIC && active ? in.sn[(uint64_t)m * (uint64_t)K + k] : 0.0;
  const uint64_t PK = (uint64_t)P * (uint64_t)K;
  const double* mp = METRIC ? in.metrics + (uint64_t)m * 5 * PK : nullptr;
  double sel[kUrSel] = {0.0, 0.0, 0.0};
  double acc[kUrPerMetric];
#pragma unroll
  for (int f = 0; f < kUrPerMetric; ++f) acc[f] = 0.0;
  for (int64_t r0 = a; r0 < e; r0 += 64) {
    const int cnt = __builtin_amdgcn_readfirstlane((int)(e - r0 < 64 ? e - r0 : 64));
    const unsigned p_l = lane < cnt ? order[r0 + lane] : 0u;
    for (int j = 0; j < cnt; ++j) {
      const uint64_t p = (unsigned)ur_bcast(p_l, j);
      if (!active || p >= (uint64_t)P) continue;
      const uint64_t at = p * (uint64_t)K + k;
      const double keep = in.keep != nullptr ? in.keep[at] : 1.0;
      const double omk = 1.0 - keep;
      if (m == 0) {
        sel[0] += keep;
        sel[1] += keep;
        sel[2] += keep * omk;
      }
      if constexpr (METRIC) {
        const double s = mp[at], cmin = mp[PK + at], cmax = mp[2 * PK + at], el0 = mp[3 * PK + at],
                     sl0 = mp[4 * PK + at];
        const double linf_drop = cmin - cmax;
        const double l0_drop = -el0;
        const double after = (s - l0_drop) - linf_drop;
        const double sel_drop = after * omk;
        const double bias = (el0 + cmin) + cmax;
        const double l0_var = sl0 * sl0;
        const double var = l0_var + sn * sn;
        const double rmse = sqrt(bias * bias + var);
        const double rmse_drop = keep * rmse + omk * fabs(s);
        const double w = keep;
        const double ab[8] = {el0 * w, l0_var * w, cmin * w, cmax * w, bias * w, var * w, rmse * w, rmse_drop * w};
        acc[0] += s;
        acc[1] += l0_drop;
        acc[2] += linf_drop;
        acc[3] += sel_drop;
#pragma unroll
        for (int i = 0; i < 8; ++i) acc[4 + i] += ab[i];
        if (s != 0.0) {
          const double s2 = s * s;
#pragma unroll
          for (int i = 0; i < 8; ++i) acc[12 + i] += ab[i] / ((i == 1 || i == 5) ? s2 : s);
        }
      }
    }
  }
  if (!active) return;
  double* out = partial + (uint64_t)item * (uint64_t)F * (uint64_t)K + k;
  if (m == 0) {
#pragma unroll
    for (int f = 0; f < kUrSel; ++f) out[(uint64_t)f * K] = sel[f];
  }
  if constexpr (METRIC) {
#pragma unroll
    for (int f = 0; f < kUrPerMetric; ++f) out[(uint64_t)(kUrSel + m * kUrPerMetric + f) * K] = acc[f];
  }
}

// sums[b][f][k] = the partials of bucket b's tiles, added in tile order
// (blockIdx.x = b * F + f, one wave per block)
__global__ void __launch_bounds__(64) k_ur_combine(int64_t P, int K, int F, const unsigned* __restrict__ hist,
                                                   int64_t n_tiles, const double* __restrict__ partial, double* sums) {
  const int b = (int)blockIdx.x / F, f = (int)blockIdx.x % F;
  const int k = (int)blockIdx.y * 64 + (int)threadIdx.x;
  if (k >= K) return;
  int64_t first = 0, tiles = 0;
  for (int c = 0; c <= b; ++c) {
    const int64_t s0 = ur_start(hist, n_tiles, c, P), s1 = ur_start(hist, n_tiles, c + 1, P);
    first += tiles;
    tiles = s1 > s0 ? ur_tiles_of(s1 - s0) : 0;
  }
  const uint64_t FK = (uint64_t)F * (uint64_t)K;
  const double* src = partial + (uint64_t)first * FK + (uint64_t)f * K + k;
  double v = 0.0;
  int64_t t = 0;
  for (; t + 8 <= tiles; t += 8) {
    double x[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) x[i] = src[(uint64_t)(t + i) * FK];
#pragma unroll
    for (int i = 0; i < 8; ++i) v += x[i];
  }
  for (; t < tiles; ++t) v += src[(uint64_t)t * FK];
  sums[((uint64_t)b * F + f) * (uint64_t)K + k] = v;
}

// entry e < kUrBuckets: bucket e; e == kUrBuckets: all partitions, the
// buckets' sums added in bucket order
__device__ __forceinline__ double ur_entry(const double* __restrict__ sums, int e, uint64_t fk, uint64_t FK) {
  if (e < kUrBuckets) return sums[(uint64_t)e * FK + fk];
  double v = 0.0;
  for (int b = 0; b < kUrBuckets; ++b) v += sums[(uint64_t)b * FK + fk];
  return v;
}

// report[e][f][k]: _average_utility_report.  Absolute and relative errors times
// (W == 0 ? 0 : 1 / W), the dropped sums times (sum_actual == 0 ? 1 :
// 1 / sum_actual); the selection sums and sum_actual stay as they are.
__global__ void __launch_bounds__(kBlock) k_ur_final(int K, int F, const double* __restrict__ sums, double* report,
                                                     long long* counts) {
  const uint64_t FK = (uint64_t)F * (uint64_t)K;
  const int64_t total = (int64_t)(kUrBuckets + 1) * (int64_t)FK;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
    const int e = (int)(i / (int64_t)FK);
    const uint64_t fk = (uint64_t)(i - (int64_t)e * (int64_t)FK);
    const int f = (int)(fk / (uint64_t)K);
    const uint64_t k = fk - (uint64_t)f * (uint64_t)K;
    double v = ur_entry(sums, e, fk, FK);
    if (f >= kUrSel) {
      const int m = (f - kUrSel) / kUrPerMetric, j = (f - kUrSel) % kUrPerMetric;
      if (j >= 4) {
        const double W = ur_entry(sums, e, k, FK);
        v = v * (W == 0.0 ? 0.0 : 1.0 / W);
      } else if (j >= 1) {
        const double sa = ur_entry(sums, e, (uint64_t)(kUrSel + m * kUrPerMetric) * (uint64_t)K + k, FK);
        v = v * (sa == 0.0 ? 1.0 : 1.0 / sa);
      }
    }
    report[i] = v;
  }
  if (blockIdx.x == 0 && threadIdx.x < 2) {
    long long c = 0;
    for (int b = 0; b < kUrBuckets; ++b) c += counts[2 * b + threadIdx.x];
    counts[2 * kUrBuckets + threadIdx.x] = c;
  }
}

}  // namespace
}  // namespace pdp

using namespace pdp;

extern "C" {

int pdp_utility_report_workspace_bytes(int64_t n_partitions, int32_t n_configurations, int32_t flags,
                                       uint64_t* bytes) {
  const int rc = ua_check_shape(n_partitions, n_configurations, flags);
  if (rc != PDP_OK) return rc;
  if (bytes == nullptr) return set_error(PDP_E_INVALID, "bytes is NULL");
  *bytes = rlayout(n_partitions, n_configurations, flags).total;
  return PDP_OK;
}

int pdp_utility_report(const int64_t* raw_statistics, const double* keep_probability, const double* metrics,
                       int64_t n_partitions, int32_t n_configurations, int32_t flags, const double* std_noise,
                       double* report, int64_t* counts, void* workspace, uint64_t workspace_bytes, void* stream) {
  int rc = ua_check_shape(n_partitions, n_configurations, flags);
  if (rc != PDP_OK) return rc;
  const int K = n_configurations;
  const int64_t P = n_partitions;
  const bool is_public = (flags & PDP_UA_PUBLIC) != 0;
  const int M = ua_n_metrics(flags), F = ur_fields(M);
  if (raw_statistics == nullptr) return set_error(PDP_E_INVALID, "raw_statistics is NULL");
  if (M != 0 && metrics == nullptr) return set_error(PDP_E_INVALID, "metrics is NULL");
  if (M != 0 && std_noise == nullptr) return set_error(PDP_E_INVALID, "std_noise is NULL");
  if (!is_public && keep_probability == nullptr) return set_error(PDP_E_INVALID, "keep_probability is NULL");
  if (report == nullptr || counts == nullptr) return set_error(PDP_E_INVALID, "output report / counts is NULL");
  const RWs w = rlayout(P, K, flags);
  if (workspace == nullptr || workspace_bytes < w.total)
    return set_error(PDP_E_WORKSPACE, "workspace too small (see pdp_utility_report_workspace_bytes)");
  if (((uintptr_t)workspace) & 255) return set_error(PDP_E_INVALID, "workspace must be 256-byte aligned");

  char* ws = (char*)workspace;
  hipStream_t st = (hipStream_t)stream;
  double* dsn = (double*)(ws + w.sn);
  unsigned char* key = (unsigned char*)(ws + w.key);
  unsigned* order = (unsigned*)(ws + w.order);
  unsigned* hist = (unsigned*)(ws + w.hist);
  double* partial = (double*)(ws + w.partial);
  double* sums = (double*)(ws + w.sums);
  const int64_t n_tiles = ur_sort_tiles(P);
  const unsigned gy = (unsigned)((K + 63) / 64);

  PDP_HIP_CHECK(hipMemsetAsync(counts, 0, (uint64_t)(kUrBuckets + 1) * 16, st));
  if (M != 0) PDP_HIP_CHECK(hipMemcpyAsync(dsn, std_noise, (uint64_t)M * K * 8, hipMemcpyHostToDevice, st));
  rc = launch("k_ur_keys", k_ur_keys, dim3(grid_for(P, 4096)), dim3(kBlock), 0, st, P, K,
              (const long long*)raw_statistics, M != 0 ? metrics : nullptr, is_public ? 1 : 0, key,
              (unsigned long long*)counts);
  if (rc != PDP_OK) return rc;
  rc = tile_sort_pass<6, kUrSortTile>("k_ur_hist", "k_ur_scatter", P, kUrKeys, 0, key, UrEmit{order}, hist,
                                      (unsigned*)(ws + w.chunks), st);
  if (rc != PDP_OK) return rc;
  const UrIn in{is_public ? nullptr : keep_probability, metrics, dsn};
  const unsigned gx = (unsigned)((ur_max_tiles(P) + kBlock / 64 - 1) / (kBlock / 64));
  rc = M != 0 ? launch("k_ur_reduce", k_ur_reduce<true>, dim3(gx, gy, (unsigned)M), dim3(kBlock), 0, st, P, K, F, in,
                       order, hist, n_tiles, partial)
              : launch("k_ur_reduce", k_ur_reduce<false>, dim3(gx, gy, 1), dim3(kBlock), 0, st, P, K, F, in, order,
                       hist, n_tiles, partial);
  if (rc != PDP_OK) return rc;
  rc = launch("k_ur_combine", k_ur_combine, dim3((unsigned)(kUrBuckets * F), gy), dim3(64), 0, st, P, K, F, hist,
              n_tiles, partial, sums);
  if (rc != PDP_OK) return rc;
  return launch("k_ur_final", k_ur_final, dim3(grid_for((int64_t)(kUrBuckets + 1) * F * K)), dim3(kBlock), 0, st, K, F,
                sums, report, (long long*)counts);
}

}  // extern "C"
