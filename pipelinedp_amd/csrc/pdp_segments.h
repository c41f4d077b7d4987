// pdp_segments.h — the two skeletons shared by VECTOR_SUM (pdp_pairs.hip), the
// per-partition utility analysis (pdp_analysis.hip) and its report
// (pdp_analysis_report.hip); the callers keep their own piece bodies.
//
// Segment reduce.  A list sorted by partition, off[p] = first entry of partition
// p (off[P] = the end), is reduced per partition without atomics in two
// launches.  The first has one wave per work item: each of the P partitions of
// at most TILE entries is reduced whole, and each tile of TILE consecutive
// entries reduces the pieces of the (at most two) longer partitions it overlaps
// into partial[tile][0 | 1]: slot 0 for the partition that owns the tile's
// first entry, slot 1 for one that starts inside the tile.  The second has one
// wave per longer partition, which adds its tiles' partials in tile order; only
// its first tile can hold it in slot 1.  Every order of summation is fixed.
//
// Stable tile sort.  One counting-sort pass by a BITS-bit digit: per tile of
// TILE records the digit counts go to a digit-major table hist[digit * n_tiles +
// tile], one device scan (scan_u32) turns them into first positions, and the
// scatter sends the tile's records out in rounds of kBlock consecutive records;
// in a round a record's rank among equal digits is the number of such records
// in earlier waves plus those in lower lanes of its own wave (ballots).  Equal
// digits so keep their order, and the result is the same in every run.
#pragma once

#include "pdp_internal.h"

namespace pdp {

// ---------------------------------------------------------- segment reduce --
template <int TILE>
__host__ __device__ inline int64_t seg_tiles(int64_t n) { return (n + TILE - 1) / TILE; }

// partition holding entry r: the p with off[p] <= r < off[p + 1] (r < off[P];
// off is non-decreasing with off[0] = 0)
__device__ __forceinline__ int64_t seg_partition_of(const unsigned* __restrict__ off, int64_t P, uint64_t r) {
  int64_t lo = 0, hi = P;  // smallest q in [1, P] with off[q] > r
  while (lo + 1 < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if ((uint64_t)off[mid] > r) hi = mid; else lo = mid;
  }
  return hi - 1;
}

struct SegDst {
  bool whole;   // true: partition `at`, all of it; false: partial slot `at` = tile * 2 + (0 | 1)
  uint64_t at;
};

// Calls piece(a, b, dst) for the entries [a, b) of every piece among this wave's
// work items (grid.x * kBlock / 64 waves stride over P + seg_tiles<TILE>(n)
// items); every lane of the wave makes the call.  `total` is the end of the
// list.  ZEROS: an empty partition is a piece too (a caller that writes its
// outputs); without it an empty partition is skipped (a caller that adds into
// them).
template <int TILE, bool ZEROS, typename Piece>
__device__ __forceinline__ void seg_for_each_piece(const unsigned* __restrict__ off, int64_t P, int64_t n,
                                                   uint64_t total, Piece&& piece) {
  constexpr uint64_t kTile = TILE;
  const int64_t items = P + seg_tiles<TILE>(n);
  const int64_t wstride = (int64_t)gridDim.x * (kBlock / 64);
  for (int64_t it = (int64_t)blockIdx.x * (kBlock / 64) + (int64_t)(threadIdx.x >> 6); it < items; it += wstride) {
    if (it < P) {
      const uint64_t a = off[it], b = off[it + 1];
      if ((ZEROS ? b < a : b <= a) || b - a > kTile || b > total) continue;
      piece(a, b, SegDst{true, (uint64_t)it});
      continue;
    }
    const uint64_t tile = (uint64_t)(it - P);
    const uint64_t r0 = tile * kTile;
    if (r0 >= total) continue;
    const uint64_t r1 = r0 + kTile < total ? r0 + kTile : total;
    const int64_t pf = seg_partition_of(off, P, r0), pl = seg_partition_of(off, P, r1 - 1);
    if (off[pf + 1] - off[pf] > kTile) piece(r0, off[pf + 1] < r1 ? off[pf + 1] : r1, SegDst{false, tile * 2});
    if (pl != pf && off[pl + 1] - off[pl] > kTile) piece(off[pl], r1, SegDst{false, tile * 2 + 1});
  }
}

// Calls whole(p, t0, t1, first_in_slot_1) for every partition of more than TILE
// entries among this wave's (waves stride over the partitions): its pieces are
// partial[t][0] of the tiles t0 < t <= t1 and partial[t0][first_in_slot_1].
template <int TILE, typename Whole>
__device__ __forceinline__ void seg_for_each_long(const unsigned* __restrict__ off, int64_t P, uint64_t total,
                                                  Whole&& whole) {
  constexpr uint64_t kTile = TILE;
  const int64_t wstride = (int64_t)gridDim.x * (kBlock / 64);
  for (int64_t p = (int64_t)blockIdx.x * (kBlock / 64) + (int64_t)(threadIdx.x >> 6); p < P; p += wstride) {
    const uint64_t a = off[p], b = off[p + 1];
    if (b <= a || b - a <= kTile || b > total) continue;
    const uint64_t t0 = a / kTile;
    whole(p, t0, (b - 1) / kTile, a != t0 * kTile);
  }
}

// value of lane `j` (wave-uniform) for every lane
__device__ __forceinline__ double bcast_f64(double v, int j) {
  const long long b = __double_as_longlong(v);
  const int lo = __builtin_amdgcn_readlane((int)(unsigned)(unsigned long long)b, j);
  const int hi = __builtin_amdgcn_readlane((int)(unsigned)((unsigned long long)b >> 32), j);
  return __longlong_as_double((long long)(((unsigned long long)(unsigned)hi << 32) | (unsigned)lo));
}

// -------------------------------------------------------- stable tile sort --
// Among the wave's valid lanes with this lane's digit: how many sit in lower
// lanes (returned) and how many there are (*n_same).
template <int BITS>
__device__ __forceinline__ unsigned wave_rank_equal(unsigned d, bool valid, int lane, unsigned* n_same) {
  unsigned long long same = __ballot(valid);
  for (int b = 0; b < BITS; ++b) {
    const bool bit = (d >> b) & 1u;
    const unsigned long long bal = __ballot(valid && bit);
    same &= bit ? bal : ~bal;
  }
  *n_same = (unsigned)__popcll(same);
  return (unsigned)__popcll(same & ((1ULL << lane) - 1ULL));
}

// hist[digit * n_tiles + tile] = records of the tile with that digit, for the
// `rows` digits in use; the digit of record i is (key[i] >> shift) & (2^BITS - 1)
template <int BITS, int TILE, typename Key>
__global__ void __launch_bounds__(kBlock) k_tile_hist(int64_t n, int rows, int shift, const Key* __restrict__ key,
                                                      unsigned* hist, int64_t n_tiles) {
  constexpr int kDigits = 1 << BITS;
  static_assert(kDigits <= kBlock && TILE % kBlock == 0, "one thread per digit, whole rounds");
  __shared__ unsigned h[kDigits];
  if (kDigits == kBlock || threadIdx.x < kDigits) h[threadIdx.x] = 0;  // 256 digits: every thread, no branch
  __syncthreads();
  const int64_t base = (int64_t)blockIdx.x * TILE;
  for (int r = 0; r < TILE / kBlock; ++r) {
    const int64_t i = base + r * kBlock + threadIdx.x;
    if (i < n) atomicAdd(&h[((unsigned)key[i] >> shift) & (kDigits - 1u)], 1u);
  }
  __syncthreads();
  if ((int)threadIdx.x < rows) hist[(int64_t)threadIdx.x * n_tiles + blockIdx.x] = h[threadIdx.x];
}

// emit(i, k, pos) writes record i, whose key is k, at its sorted position pos < n
template <int BITS, int TILE, typename Key, typename Emit>
__global__ void __launch_bounds__(kBlock) k_tile_scatter(int64_t n, int rows, int shift,
                                                         const Key* __restrict__ key, Emit emit,
                                                         const unsigned* __restrict__ hist, int64_t n_tiles) {
  constexpr int kDigits = 1 << BITS, kWaves = kBlock / 64;
  __shared__ unsigned base[kDigits];
  __shared__ unsigned cnt[kWaves][kDigits];
  const int lane = (int)(threadIdx.x & 63), wave = (int)(threadIdx.x >> 6);
  if (kDigits == kBlock || threadIdx.x < kDigits) {  // one thread per digit; 256 digits: every thread, no branch
    base[threadIdx.x] = (int)threadIdx.x < rows ? hist[(int64_t)threadIdx.x * n_tiles + blockIdx.x] : 0u;
    for (int w = 0; w < kWaves; ++w) cnt[w][threadIdx.x] = 0;
  }
  __syncthreads();
  const int64_t tile0 = (int64_t)blockIdx.x * TILE;
  for (int r = 0; r < TILE / kBlock; ++r) {
    const int64_t i = tile0 + r * kBlock + threadIdx.x;
    const bool valid = i < n;
    const unsigned k = valid ? (unsigned)key[i] : 0u;
    const unsigned d = (k >> shift) & (kDigits - 1u);
    unsigned n_same;
    const unsigned below = wave_rank_equal<BITS>(d, valid, lane, &n_same);
    if (valid && below == 0) cnt[wave][d] = n_same;
    __syncthreads();
    if (valid) {
      unsigned pos = base[d] + below;
      for (int w = 0; w < wave; ++w) pos += cnt[w][d];
      if ((int64_t)pos < n) emit(i, k, pos);
    }
    __syncthreads();
    if (kDigits == kBlock || threadIdx.x < kDigits) {
      unsigned add = 0;
      for (int w = 0; w < kWaves; ++w) {
        add += cnt[w][threadIdx.x];
        cnt[w][threadIdx.x] = 0;
      }
      base[threadIdx.x] += add;
    }
    __syncthreads();
  }
}

// One pass over n records (none: nothing to do): hist (rows * tiles + 1 words),
// its scan, the scatter.  The names are the launches' profiler names.
template <int BITS, int TILE, typename Key, typename Emit>
int tile_sort_pass(const char* hist_name, const char* scatter_name, int64_t n, int rows, int shift, const Key* key,
                   Emit emit, unsigned* hist, unsigned* chunk_sums, hipStream_t st) {
  if (n <= 0) return PDP_OK;
  const int64_t n_tiles = seg_tiles<TILE>(n);
  int rc = launch(hist_name, k_tile_hist<BITS, TILE, Key>, dim3((unsigned)n_tiles), dim3(kBlock), 0, st, n, rows,
                  shift, key, hist, n_tiles);
  if (rc != PDP_OK) return rc;
  rc = scan_u32(hist, rows * n_tiles, chunk_sums, st);
  if (rc != PDP_OK) return rc;
  return launch(scatter_name, k_tile_scatter<BITS, TILE, Key, Emit>, dim3((unsigned)n_tiles), dim3(kBlock), 0, st,
                n, rows, shift, key, emit, hist, n_tiles);
}

// ------------------------------------- utility analysis: shared host checks --
inline int ua_n_metrics(int flags) {
  return ((flags & PDP_UA_SUM) ? 1 : 0) + ((flags & PDP_UA_COUNT) ? 1 : 0) + ((flags & PDP_UA_PRIVACY_ID_COUNT) ? 1 : 0);
}

// (n_partitions, n_configurations, flags) of pdp_utility_analysis* and pdp_utility_report*
inline int ua_check_shape(int64_t n_partitions, int32_t K, int32_t flags) {
  if (n_partitions < 1) return set_error(PDP_E_INVALID, "n_partitions must be >= 1");
  if (n_partitions >= ((int64_t)1 << 31)) return set_error(PDP_E_UNSUPPORTED, "n_partitions must be < 2^31");
  if (K < 1) return set_error(PDP_E_INVALID, "n_configurations must be >= 1");
  if (K > PDP_MAX_CONFIGURATIONS)
    return set_error(PDP_E_UNSUPPORTED, "n_configurations above PDP_MAX_CONFIGURATIONS");
  if (flags & ~(PDP_UA_SUM | PDP_UA_COUNT | PDP_UA_PRIVACY_ID_COUNT | PDP_UA_PUBLIC))
    return set_error(PDP_E_INVALID, "unknown utility analysis flags");
  if ((flags & PDP_UA_PUBLIC) && ua_n_metrics(flags) == 0)
    return set_error(PDP_E_INVALID, "public partitions without a metric: nothing to analyse");
  return PDP_OK;
}

}  // namespace pdp
