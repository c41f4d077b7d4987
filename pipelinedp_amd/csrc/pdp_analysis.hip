// pdp_analysis.hip — the per-partition stage of utility analysis
// (analysis/per_partition_combiners.py:193-356 of the reference) for K
// parameter configurations in one pass over the (privacy id, partition) pairs.
//
//   k_ua_init      partition codes -> u32 sort keys (an out-of-range code gets
//                  the key P and sets the error word), row indices, and
//                  RawStatistics by integer atomics
//   k_ua_hist / k_ua_scatter
//                  a stable LSD radix sort of (key, row index) by 8-bit digits,
//                  one stable tile sort pass (pdp_segments.h) per digit
//   k_ua_offsets   segment offsets off[p] = lower_bound(sorted keys, p)
//   k_ua_gather    pair fields in sorted order (count, sum, n_partitions)
//   k_ua_reduce / k_ua_combine
//                  the segment reduce of pdp_segments.h with tiles of kUaChunk
//                  pairs and lanes across configurations: lane k of a wave keeps
//                  (l0, linf, min_sum, max_sum) of configuration k in registers
//                  and walks a piece whose pair fields are loaded 64 at a time
//                  and broadcast; fp64 accumulators per lane
//   k_ua_select    one wave per (partition, configuration): the exact
//                  Poisson-binomial PMF for n <= 100 pairs (entry i in lane
//                  i % 64), the refined normal approximation from the moments
//                  for n > 100, either dotted with the keep table
// No floating-point atomic, and every order of summation is fixed: two runs
// give the same bits.  Every product and sum is rounded on its own (no fused
// multiply-add), so a term equals the reference's NumPy expression bit for bit.
#include "pdp_segments.h"

#pragma clang fp contract(off)

namespace pdp {
namespace {

constexpr int kUaTile = 2048;        // sorted (key, index) records per sort tile
constexpr unsigned kUaChunk = 4096;  // pairs per reduce work item
constexpr unsigned kUaExact = 100;   // MAX_PROBABILITIES_IN_ACCUMULATOR
constexpr int kUaMoments = 3;

struct UWs {
  uint64_t err, params, koff, key0, key1, idx0, idx1, hist, chunks, off, scnt, ssum, snp, mom, partial, total;
};

inline bool ua_private(int flags) { return (flags & PDP_UA_PUBLIC) == 0; }
inline int ua_fields(int flags) { return 5 * ua_n_metrics(flags) + (ua_private(flags) ? kUaMoments : 0); }
inline int64_t ua_chunks(int64_t n) { return seg_tiles<kUaChunk>(n); }

UWs ulayout(int64_t n_pairs, int64_t P, int K, int flags) {
  UWs w{};
  const uint64_t n = (uint64_t)(n_pairs > 0 ? n_pairs : 1);
  const uint64_t hist_len = 256 * (uint64_t)seg_tiles<kUaTile>((int64_t)n);
  uint64_t off = 0;
  w.err = off; off = align256(off + 16);
  w.params = off; off = align256(off + (uint64_t)K * sizeof(pdp_ua_config_params));
  w.koff = off; off = align256(off + ((uint64_t)K + 1) * 8);
  w.key0 = off; off = align256(off + n * 4);
  w.key1 = off; off = align256(off + n * 4);
  w.idx0 = off; off = align256(off + n * 4);
  w.idx1 = off; off = align256(off + n * 4);
  w.hist = off; off = align256(off + (hist_len + 1) * 4);
  w.chunks = off; off = align256(off + (uint64_t)scan_chunk_sums_len((int64_t)hist_len) * 4);
  w.off = off; off = align256(off + ((uint64_t)P + 1) * 4);
  w.scnt = off; off = align256(off + n * 8);
  w.ssum = off; off = align256(off + n * 8);
  w.snp = off; off = align256(off + n * 8);
  w.mom = off; off = align256(off + (ua_private(flags) ? (uint64_t)kUaMoments * (uint64_t)P * (uint64_t)K * 8 : 0));
  w.partial = off;
  off = align256(off + (uint64_t)ua_chunks((int64_t)n) * 2 * (uint64_t)ua_fields(flags) * (uint64_t)K * 8);
  w.total = off;
  return w;
}

// ------------------------------------------------------------------ sort --
__global__ void __launch_bounds__(kBlock) k_ua_init(int64_t n, int64_t P, const int64_t* __restrict__ partition,
                                                    const int64_t* __restrict__ count, unsigned* key, unsigned* idx,
                                                    long long* raw, unsigned* err) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    const int64_t p = partition[i];
    const bool ok = p >= 0 && p < P;
    key[i] = ok ? (unsigned)p : (unsigned)P;
    idx[i] = (unsigned)i;
    if (ok) {
      atomicAdd((unsigned long long*)(raw + 2 * p), 1ULL);
      atomicAdd((unsigned long long*)(raw + 2 * p + 1), (unsigned long long)count[i]);
    } else {
      atomicOr(err, 1u);
    }
  }
}

// what the stable LSD radix sort (8-bit digits, pdp_segments.h) moves: the key and the row index
struct UaEmit {
  const unsigned* idx_in;
  unsigned *key_out, *idx_out;
  __device__ void operator()(int64_t i, unsigned k, unsigned pos) const {
    const unsigned row = idx_in[i];  // read before the first store: the two may alias for all the compiler knows
    key_out[pos] = k;
    idx_out[pos] = row;
  }
};

// off[p] = first sorted position whose key is >= p, p in [0, P]
__global__ void __launch_bounds__(kBlock) k_ua_offsets(int64_t n, int64_t P, const unsigned* __restrict__ key,
                                                       unsigned* off) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p <= P; p += stride) {
    int64_t lo = 0, hi = n;
    while (lo < hi) {
      const int64_t mid = (lo + hi) >> 1;
      if ((int64_t)key[mid] < p) lo = mid + 1; else hi = mid;
    }
    off[p] = (unsigned)lo;
  }
}

__global__ void __launch_bounds__(kBlock) k_ua_gather(int64_t n, int64_t P, const unsigned* __restrict__ off,
                                                      const unsigned* __restrict__ idx,
                                                      const int64_t* __restrict__ count,
                                                      const double* __restrict__ sum,
                                                      const int64_t* __restrict__ npart, long long* scnt,
                                                      double* ssum, long long* snp) {
  const int64_t total = off[P] < n ? off[P] : n;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r < total; r += stride) {
    const int64_t i = idx[r];
    if (i >= n) continue;
    scnt[r] = count[i];
    ssum[r] = sum != nullptr ? sum[i] : 0.0;
    snp[r] = npart[i];
  }
}

// ---------------------------------------------------------------- reduce --
// q = min(1, l0 / n_partitions), 0 for n_partitions <= 0 (np.where(n > 0, np.minimum(1, l0 / n), 0))
__device__ __forceinline__ double ua_q(double l0, double np) { return np > 0.0 ? fmin(1.0, l0 / np) : 0.0; }

// SumCombiner.create_accumulator's five terms of one pair (:244-269)
__device__ __forceinline__ void ua_term(double x, double lo, double hi, double q, double omq, double* a) {
  const double c = clip_f64(x, lo, hi);
  const double e = c - x;
  a[0] += x;
  a[1] += x < lo ? e : 0.0;
  a[2] += x > hi ? e : 0.0;
  a[3] += -c * omq;
  a[4] += c * c * q * omq;
}

// per-lane accumulators: metric slots in SUM, COUNT, PRIVACY_ID_COUNT order, then the moments
template <int M, bool SEL>
struct UaAcc {
  static constexpr int kM = ((M & 1) ? 1 : 0) + ((M & 2) ? 1 : 0) + ((M & 4) ? 1 : 0);
  static constexpr int kF = 5 * kM + (SEL ? kUaMoments : 0);
  double f[kF > 0 ? kF : 1];
};

struct UaLane {
  double l0, linf, lo, hi;
};

template <int M, bool SEL>
__device__ __forceinline__ void ua_piece(UaAcc<M, SEL>& acc, const UaLane& c, const long long* __restrict__ scnt,
                                         const double* __restrict__ ssum, const long long* __restrict__ snp,
                                         uint64_t a, uint64_t b, int lane) {
#pragma unroll
  for (int f = 0; f < UaAcc<M, SEL>::kF; ++f) acc.f[f] = 0.0;
  for (uint64_t r0 = a; r0 < b; r0 += 64) {
    const int m = __builtin_amdgcn_readfirstlane((int)(b - r0 < 64 ? b - r0 : 64));
    double cnt_l = 0.0, sum_l = 0.0, np_l = 0.0;
    if (lane < m) {
      cnt_l = (double)scnt[r0 + lane];
      sum_l = ssum[r0 + lane];
      np_l = (double)snp[r0 + lane];
    }
    for (int j = 0; j < m; ++j) {
      const double cnt = bcast_f64(cnt_l, j), sm = bcast_f64(sum_l, j), np = bcast_f64(np_l, j);
      const double q = ua_q(c.l0, np), omq = 1.0 - q;
      int s = 0;
      if constexpr ((M & 1) != 0) {
        ua_term(sm, c.lo, c.hi, q, omq, acc.f + s);
        s += 5;
      }
      if constexpr ((M & 2) != 0) {
        ua_term(cnt, 0.0, c.linf, q, omq, acc.f + s);
        s += 5;
      }
      if constexpr ((M & 4) != 0) {
        ua_term(cnt > 0.0 ? 1.0 : 0.0, 0.0, 1.0, q, omq, acc.f + s);
        s += 5;
      }
      if constexpr (SEL) {
        const double v = q * omq;
        acc.f[s] += q;
        acc.f[s + 1] += v;
        acc.f[s + 2] += v * (1.0 - 2.0 * q);
      }
    }
  }
}

struct UaOut {
  double* metrics;  // [kM][5][P][K]
  double* mom;      // [3][P][K] (workspace)
};

template <int M, bool SEL>
__device__ __forceinline__ void ua_write(const UaAcc<M, SEL>& acc, const UaOut& o, int64_t P, int K, int64_t p,
                                         int k) {
  constexpr int kM = UaAcc<M, SEL>::kM;
#pragma unroll
  for (int m = 0; m < kM; ++m) {
#pragma unroll
    for (int f = 0; f < 5; ++f) {
      const double v = acc.f[m * 5 + f];
      o.metrics[(((uint64_t)m * 5 + f) * (uint64_t)P + (uint64_t)p) * (uint64_t)K + k] = f == 4 ? sqrt(v) : v;
    }
  }
  if constexpr (SEL) {
#pragma unroll
    for (int j = 0; j < kUaMoments; ++j)
      o.mom[((uint64_t)j * (uint64_t)P + (uint64_t)p) * (uint64_t)K + k] = acc.f[kM * 5 + j];
  }
}

template <int M, bool SEL>
__global__ void __launch_bounds__(kBlock) k_ua_reduce(int64_t n, int64_t P, int K,
                                                      const pdp_ua_config_params* __restrict__ params,
                                                      const unsigned* __restrict__ off,
                                                      const long long* __restrict__ scnt,
                                                      const double* __restrict__ ssum,
                                                      const long long* __restrict__ snp, UaOut o, double* partial) {
  constexpr int kF = UaAcc<M, SEL>::kF;
  const int lane = (int)(threadIdx.x & 63);
  const int k = (int)blockIdx.y * 64 + lane;
  const bool active = k < K;
  UaLane c{1.0, 0.0, 0.0, 0.0};
  if (active) {
    c.l0 = (double)params[k].l0;
    c.linf = (double)params[k].linf;
    c.lo = params[k].min_sum;
    c.hi = params[k].max_sum;
  }
  const uint64_t total = off[P] < (uint64_t)n ? off[P] : (uint64_t)n;
  UaAcc<M, SEL> acc;
  // an empty partition is a piece: zeros
  seg_for_each_piece<kUaChunk, true>(off, P, n, total, [&](uint64_t a, uint64_t b, SegDst dst) {
    ua_piece<M, SEL>(acc, c, scnt, ssum, snp, a, b, lane);
    if (!active) return;
    if (dst.whole) {
      ua_write<M, SEL>(acc, o, P, K, (int64_t)dst.at, k);
    } else {
#pragma unroll
      for (int f = 0; f < kF; ++f) partial[(dst.at * kF + f) * (uint64_t)K + k] = acc.f[f];
    }
  });
}

// partitions of more than kUaChunk pairs: their tiles' partials, added in tile order
template <int M, bool SEL>
__global__ void __launch_bounds__(kBlock) k_ua_combine(int64_t n, int64_t P, int K, const unsigned* __restrict__ off,
                                                       const double* __restrict__ partial, UaOut o) {
  constexpr int kF = UaAcc<M, SEL>::kF;
  const int lane = (int)(threadIdx.x & 63);
  const int k = (int)blockIdx.y * 64 + lane;
  const bool active = k < K;
  const uint64_t total = off[P] < (uint64_t)n ? off[P] : (uint64_t)n;
  seg_for_each_long<kUaChunk>(off, P, total, [&](int64_t p, uint64_t t0, uint64_t t1, bool first_in_slot_1) {
    if (!active) return;
    UaAcc<M, SEL> acc;
#pragma unroll
    for (int f = 0; f < kF; ++f) acc.f[f] = 0.0;
    for (uint64_t t = t0; t <= t1; ++t) {
      const uint64_t slot = (t == t0 && first_in_slot_1) ? 1 : 0;
#pragma unroll
      for (int f = 0; f < kF; ++f) acc.f[f] += partial[((t * 2 + slot) * kF + f) * (uint64_t)K + k];
    }
    ua_write<M, SEL>(acc, o, P, K, p, k);
  });
}

template <int M, bool SEL>
int launch_ua_reduce(int64_t n, int64_t P, int K, const pdp_ua_config_params* params, const unsigned* off,
                     const long long* scnt, const double* ssum, const long long* snp, UaOut o, double* partial,
                     hipStream_t st) {
  const unsigned gy = (unsigned)((K + 63) / 64);
  const int64_t items = P + ua_chunks(n);
  int rc = launch("k_ua_reduce", k_ua_reduce<M, SEL>, dim3(grid_for(items * 64, 16384), gy), dim3(kBlock), 0, st, n,
                  P, K, params, off, scnt, ssum, snp, o, partial);
  if (rc != PDP_OK) return rc;
  return launch("k_ua_combine", k_ua_combine<M, SEL>, dim3(grid_for(P * 64, 16384), gy), dim3(kBlock), 0, st, n, P, K,
                off, partial, o);
}

template <bool SEL, typename... A>
int dispatch_ua_reduce(int metrics, A... a) {
  switch (metrics) {
    case 0: return launch_ua_reduce<0, SEL>(a...);
    case 1: return launch_ua_reduce<1, SEL>(a...);
    case 2: return launch_ua_reduce<2, SEL>(a...);
    case 3: return launch_ua_reduce<3, SEL>(a...);
    case 4: return launch_ua_reduce<4, SEL>(a...);
    case 5: return launch_ua_reduce<5, SEL>(a...);
    case 6: return launch_ua_reduce<6, SEL>(a...);
    default: return launch_ua_reduce<7, SEL>(a...);
  }
}

// ---------------------------------------------------------------- select --
__device__ __forceinline__ double ua_wave_sum(double v) {
  for (int o = 1; o < 64; o <<= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// G((x + 0.5 - mean) / sigma) clipped to [0, 1] (poisson_binomial.py:73-82)
__device__ __forceinline__ double ua_cdf(double v, double mean, double sigma, double skew) {
  const double x = (v + 0.5 - mean) / sigma;
  const double cdf = 0.5 * erfc(-x / 1.4142135623730951);
  const double pdf = exp(-(x * x) / 2.0) / 2.5066282746310002;
  const double g = cdf + skew * (1.0 - x * x) * pdf / 6.0;
  return fmin(fmax(g, 0.0), 1.0);
}

__global__ void __launch_bounds__(kBlock) k_ua_select(int64_t n, int64_t P, int K,
                                                      const pdp_ua_config_params* __restrict__ params,
                                                      const unsigned* __restrict__ off,
                                                      const long long* __restrict__ snp,
                                                      const double* __restrict__ ktab,
                                                      const long long* __restrict__ koff,
                                                      const double* __restrict__ mom, double* keep_prob) {
  const int lane = (int)(threadIdx.x & 63), wave = (int)(threadIdx.x >> 6);
  const uint64_t total = off[P] < (uint64_t)n ? off[P] : (uint64_t)n;
  const int64_t items = P * (int64_t)K;
  const int64_t wstride = (int64_t)gridDim.x * (kBlock / 64);
  for (int64_t it = (int64_t)blockIdx.x * (kBlock / 64) + wave; it < items; it += wstride) {
    const int64_t p = it / K;
    const int k = (int)(it - p * K);
    const uint64_t a = off[p], b = off[p + 1];
    if (b < a || b > total) continue;
    const uint64_t cnt = b - a;
    const double l0 = (double)params[k].l0;
    const double* tab = ktab + koff[k];
    const long long len = koff[k + 1] - koff[k];
    double part = 0.0;
    if (cnt <= kUaExact) {
      // poisson_binomial.compute_pmf: entry i of the PMF in lane i % 64 (A: i < 64, B: i >= 64)
      const int m = __builtin_amdgcn_readfirstlane((int)cnt);
      const double q0 = lane < m ? ua_q(l0, (double)snp[a + lane]) : 0.0;
      const double q1 = lane + 64 < m ? ua_q(l0, (double)snp[a + 64 + lane]) : 0.0;
      double A = lane == 0 ? 1.0 : 0.0, B = 0.0;
      for (int j = 0; j < m; ++j) {
        const double pr = j < 64 ? bcast_f64(q0, j) : bcast_f64(q1, j - 64);
        const double omp = 1.0 - pr;
        double upA = __shfl_up(A, 1, 64), upB = __shfl_up(B, 1, 64);
        const double a63 = bcast_f64(A, 63);
        if (lane == 0) {
          upA = 0.0;
          upB = a63;
        }
        A = A * omp + upA * pr;
        B = B * omp + upB * pr;
      }
      const double kA = lane < len ? tab[lane] : 1.0;
      const double kB = lane + 64 < len ? tab[lane + 64] : 1.0;
      part = (lane <= m ? A * kA : 0.0) + (lane + 64 <= m ? B * kB : 0.0);
    } else {
      // compute_pmf_approximation (:62-83) from the moments of the reduce pass
      const uint64_t at = (uint64_t)p * (uint64_t)K + k, PK = (uint64_t)P * (uint64_t)K;
      const double mean = mom[at], var = mom[PK + at], third = mom[2 * PK + at];
      const double sigma = sqrt(var);
      if (sigma == 0.0) {
        const long long v = (long long)rint(mean);
        part = lane == 0 ? (v >= 0 && v < len ? tab[v] : (v < 0 ? 0.0 : 1.0)) : 0.0;
      } else {
        const double skew = third / (sigma * sigma * sigma);
        long long start = (long long)floor(mean - 8.0 * sigma);
        if (start < 0) start = 0;
        long long end = (long long)rint(mean + 8.0 * sigma);
        if (end > (long long)cnt) end = (long long)cnt;
        for (long long v = start + lane; v <= end; v += 64) {
          const double pm = ua_cdf((double)v, mean, sigma, skew) - ua_cdf((double)(v - 1), mean, sigma, skew);
          part += pm * (v < len ? tab[v] : 1.0);
        }
      }
    }
    const double s = ua_wave_sum(part);
    if (lane == 0) keep_prob[(uint64_t)p * (uint64_t)K + k] = s;
  }
}

int ua_check_pairs(int64_t n_pairs, int64_t n_partitions, int32_t K, int32_t flags) {
  if (n_pairs < 0) return set_error(PDP_E_INVALID, "n_pairs < 0");
  if (n_pairs >= ((int64_t)1 << 31)) return set_error(PDP_E_UNSUPPORTED, "n_pairs must be < 2^31");
  return ua_check_shape(n_partitions, K, flags);
}

}  // namespace
}  // namespace pdp

using namespace pdp;

extern "C" {

int pdp_utility_analysis_workspace_bytes(int64_t n_pairs, int64_t n_partitions, int32_t n_configurations,
                                         int32_t flags, uint64_t* bytes) {
  const int rc = ua_check_pairs(n_pairs, n_partitions, n_configurations, flags);
  if (rc != PDP_OK) return rc;
  if (bytes == nullptr) return set_error(PDP_E_INVALID, "bytes is NULL");
  *bytes = ulayout(n_pairs, n_partitions, n_configurations, flags).total;
  return PDP_OK;
}

int pdp_utility_analysis(const int64_t* partition, const int64_t* count, const double* sum,
                         const int64_t* n_partitions_of_pid, int64_t n_pairs, int64_t n_partitions,
                         const pdp_ua_config_params* params, int32_t n_configurations, const double* keep_tables,
                         const int64_t* keep_offsets, int32_t flags, const pdp_ua_outputs* out, void* workspace,
                         uint64_t workspace_bytes, void* stream) {
  int rc = ua_check_pairs(n_pairs, n_partitions, n_configurations, flags);
  if (rc != PDP_OK) return rc;
  const int K = n_configurations;
  const int64_t n = n_pairs, P = n_partitions;
  const bool sel = ua_private(flags);
  const int metrics = flags & (PDP_UA_SUM | PDP_UA_COUNT | PDP_UA_PRIVACY_ID_COUNT);
  if (params == nullptr) return set_error(PDP_E_INVALID, "params is NULL");
  if (out == nullptr || out->raw_statistics == nullptr) return set_error(PDP_E_INVALID, "output raw_statistics is NULL");
  if (metrics != 0 && out->metrics == nullptr) return set_error(PDP_E_INVALID, "output metrics is NULL");
  if (sel && out->keep_probability == nullptr) return set_error(PDP_E_INVALID, "output keep_probability is NULL");
  if (n > 0 && (partition == nullptr || count == nullptr || n_partitions_of_pid == nullptr))
    return set_error(PDP_E_INVALID, "pair columns are NULL");
  if (n > 0 && (flags & PDP_UA_SUM) && sum == nullptr) return set_error(PDP_E_INVALID, "SUM needs the sum column");
  for (int k = 0; k < K; ++k) {
    const pdp_ua_config_params& c = params[k];
    if (c.l0 < 1) return set_error(PDP_E_INVALID, "params: l0 (max_partitions_contributed) must be >= 1");
    if ((flags & PDP_UA_COUNT) && c.linf < 0)
      return set_error(PDP_E_INVALID, "params: linf (max_contributions_per_partition) must be >= 0");
    if ((flags & PDP_UA_SUM) && (c.min_sum != c.min_sum || c.max_sum != c.max_sum))
      return set_error(PDP_E_INVALID, "params: min_sum / max_sum must not be NaN");
  }
  if (sel) {
    if (keep_offsets == nullptr) return set_error(PDP_E_INVALID, "keep_offsets is NULL");
    if (keep_offsets[0] != 0) return set_error(PDP_E_INVALID, "keep_offsets[0] must be 0");
    for (int k = 0; k < K; ++k) {
      const int64_t len = keep_offsets[k + 1] - keep_offsets[k];
      if (len < 0) return set_error(PDP_E_INVALID, "keep_offsets must not decrease");
      if (len > PDP_UA_MAX_KEEP_TABLE)
        return set_error(PDP_E_UNSUPPORTED, "keep table longer than PDP_UA_MAX_KEEP_TABLE");
    }
    if (keep_offsets[K] > 0 && keep_tables == nullptr) return set_error(PDP_E_INVALID, "keep_tables is NULL");
  }
  const UWs w = ulayout(n, P, K, flags);
  if (workspace == nullptr || workspace_bytes < w.total)
    return set_error(PDP_E_WORKSPACE, "workspace too small (see pdp_utility_analysis_workspace_bytes)");
  if (((uintptr_t)workspace) & 255) return set_error(PDP_E_INVALID, "workspace must be 256-byte aligned");

  char* ws = (char*)workspace;
  hipStream_t st = (hipStream_t)stream;
  unsigned* err = (unsigned*)(ws + w.err);
  pdp_ua_config_params* dparams = (pdp_ua_config_params*)(ws + w.params);
  long long* dkoff = (long long*)(ws + w.koff);
  unsigned* key[2] = {(unsigned*)(ws + w.key0), (unsigned*)(ws + w.key1)};
  unsigned* idx[2] = {(unsigned*)(ws + w.idx0), (unsigned*)(ws + w.idx1)};
  unsigned* hist = (unsigned*)(ws + w.hist);
  unsigned* off = (unsigned*)(ws + w.off);
  long long* scnt = (long long*)(ws + w.scnt);
  double* ssum = (double*)(ws + w.ssum);
  long long* snp = (long long*)(ws + w.snp);

  PDP_HIP_CHECK(hipMemsetAsync(err, 0, 16, st));
  PDP_HIP_CHECK(hipMemsetAsync(out->raw_statistics, 0, (uint64_t)P * 16, st));
  PDP_HIP_CHECK(hipMemcpyAsync(dparams, params, (uint64_t)K * sizeof(pdp_ua_config_params), hipMemcpyHostToDevice, st));
  if (sel)
    PDP_HIP_CHECK(hipMemcpyAsync(dkoff, keep_offsets, ((uint64_t)K + 1) * 8, hipMemcpyHostToDevice, st));

  int cur = 0;
  if (n > 0) {
    rc = launch("k_ua_init", k_ua_init, dim3(grid_for(n)), dim3(kBlock), 0, st, n, P, partition, count, key[0], idx[0],
                (long long*)out->raw_statistics, err);
    if (rc != PDP_OK) return rc;
    const int key_bits = bits_for(P + 1);
    for (int shift = 0; shift < key_bits; shift += 8) {
      rc = tile_sort_pass<8, kUaTile>("k_ua_hist", "k_ua_scatter", n, 256, shift, key[cur],
                                      UaEmit{idx[cur], key[cur ^ 1], idx[cur ^ 1]}, hist,
                                      (unsigned*)(ws + w.chunks), st);
      if (rc != PDP_OK) return rc;
      cur ^= 1;
    }
  }
  rc = launch("k_ua_offsets", k_ua_offsets, dim3(grid_for(P + 1)), dim3(kBlock), 0, st, n, P, key[cur], off);
  if (rc != PDP_OK) return rc;
  if (n > 0) {
    rc = launch("k_ua_gather", k_ua_gather, dim3(grid_for(n)), dim3(kBlock), 0, st, n, P, off, idx[cur], count, sum,
                n_partitions_of_pid, scnt, ssum, snp);
    if (rc != PDP_OK) return rc;
  }
  UaOut o{out->metrics, (double*)(ws + w.mom)};
  double* partial = (double*)(ws + w.partial);
  if (metrics != 0 || sel) {
    rc = sel ? dispatch_ua_reduce<true>(metrics, n, P, K, dparams, off, scnt, ssum, snp, o, partial, st)
             : dispatch_ua_reduce<false>(metrics, n, P, K, dparams, off, scnt, ssum, snp, o, partial, st);
    if (rc != PDP_OK) return rc;
  }
  if (sel) {
    rc = launch("k_ua_select", k_ua_select, dim3(grid_for(P * (int64_t)K * 64, 1 << 20)), dim3(kBlock), 0, st, n, P, K,
                dparams, off, snp, keep_tables, dkoff, o.mom, out->keep_probability);
    if (rc != PDP_OK) return rc;
  }
  return PDP_OK;
}

}  // extern "C"
