// pdp_bound.hip — contribution bounding + per-partition reduction (gfx950).
//
// Replaces, for one shard of dense columns (privacy_id, partition_key, value):
//   SamplingCrossAndPerPartitionContributionBounder.bound_contributions
//     (contribution_bounders.py:72-111): "Sample per (privacy_id, partition_key)"
//     (<= linf rows) and "Sample per privacy_id" (<= l0 distinct partitions);
//   SamplingCrossPartitionContributionBounder (:168-201) when linf == 0;
//   CompoundCombiner.create_accumulator / merge_accumulators (combiners.py:749-764)
//     and LocalBackend.combine_accumulators_per_key (pipeline_backend.py:555-565).
//
// Sampling = bottom-k on counter-based keys (pdp_internal.h: pair_key, row_key),
// so the kept sets depend only on (seed, data), not on scheduling or path.
//
// Two execution paths, same results:
//
//  BUCKETED (default when the per-privacy-id state fits LDS)
//    Privacy ids are grouped in buckets of 2^bucket_bits ids (one LDS-sized
//    workgroup each) and buckets in super-buckets of 2^super_bits buckets, so
//    that every partitioning pass writes to <= 64 destinations per workgroup
//    (long coalesced runs; ~2000 direct destinations thrash L2 5x).
//    k_part_hist       per-tile histogram of bucket = pid >> bucket_bits  (8 B/row)
//    k_super_scan      per-tile write offsets of every super-bucket
//    k_gscan_*, k_scan_*   rows per bucket -> bucket starts; level-2 write
//                      cursors at every group of kL2GroupTiles tiles
//    k_scatter_l1      rows -> super-bucket order, tile runs in tile order (16 B in, 8 B out)
//    k_scatter_l2      per (tile group, super-bucket) -> bucket order, no atomics (8 B in, 8 B out)
//    k_bucket_bound    one workgroup per bucket, all sampling state in LDS:
//                      B1 bottom-l0 pair sketch per pid, B2 per-pair row count
//                      + bottom-linf row sketch, B3 gather the sampled values
//                      and merge each kept pair into the partition accumulators
//    k_range_*, k_split_*, k_fine_*   PDP_MERGE_RANGES: the pair records summed
//                      per partition (pdp_bound_merge.hip, launch_merge)
//  GLOBAL (fallback for large l0 * linf)
//    k_pair_sketch / k_pair_rows / k_reduce_pairs: the same sketches in HBM,
//    updated with device-scope atomics.
//
// Where the code lives: every kernel above is in this file but the k_scan_*
// (pdp_scan.hip, scan_u32) and the range merge (pdp_bound_merge.hip); after
// the kernels come their launch chains and the C entry points that launch.
// What they run on is decided in pdp_bound_planner.hip, host code only:
// validate, the plan (make_plan), layout, make_kp, check_ws, pdp_bound_plan
// and pdp_bound_workspace_bytes; it asks this file for the LDS sizes of
// StageLds / SieveShape (l1_stage_bytes, sieve_stage_bytes, sieve_slot_bits).
// pdp_bound_plan.h: the shared constants, Plan, Ws, KP, PairRecords, the typed
// view of a workspace region (at / at_opt) and the planner's declarations;
// pdp_bound_keys.h: device helpers of more than one file.
#include <algorithm>
#include <cstdlib>
#include <type_traits>
#include <vector>

#include "pdp_bound_keys.h"

namespace pdp {
namespace {

// ---- threshold sieve (Plan.sieve) ----------------------------------------
// With cross-partition sampling, a privacy id keeps the l0 pairs of smallest
// pair key, and its other pairs (usually most of its rows) contribute
// nothing.  The sieve keeps only rows whose 32-bit pair hash is below one
// global threshold t32 = sieve << 16: if a privacy id has >= l0 distinct
// pairs below it, its l0 smallest are among them, together with every row of
// those pairs (a pair's rows share its hash), so the level-1 pass writes and
// levels 2/3 read only those candidate rows.  Privacy ids with fewer than l0
// candidate pairs ("unresolved": the bucket kernel marks them in a bitmap
// and a list) are finished by a fix-up over ALL their rows: one streaming
// re-read of the privacy-id column (k_sieve_rescan, an LDS Bloom filter of
// the list in front of the exact bitmap), a scatter into bucket order and a
// second bucket-kernel launch whose pair records follow the main ones.
// Kept pairs and rows are exactly those of the unsieved path.
constexpr int kSieveChunkItems = 4;                            // rows per thread and chunk
constexpr int kSieveBufs = 2;  // full tiles: chunks of loads in flight (register buffers)
constexpr int kSieveItems = 12;  // stage slots per thread (records each thread handles at a flush)
// Two workgroup shapes (Plan.sieve_threads):
//  1,024 threads, a 12,288-candidate stage, 8 flush slots per tile: one
//    workgroup per CU (~150 KiB of LDS), whose flush (LDS counting sort +
//    block write) stalls the CU's loads;
//  512 threads, a 6,144-candidate stage, 16 flush slots per tile, <= 80 KiB of
//    LDS: two workgroups per CU, so one's flush overlaps the other's loads.
template <int TH>
struct SieveShape {
  static constexpr int kChunk = TH * kSieveChunkItems;  // rows filtered per chunk
  static constexpr int kCap = TH * kSieveItems;         // candidate slots of the LDS stage
  static constexpr int kSlots = TH == 1024 ? 8 : 16;    // flush blocks per tile, at most
  static constexpr int kSlotBits = TH == 1024 ? 3 : 4;
  // a tile flushes at most once per chunk, and every flush but its last holds
  // > kCap - kChunk records, so its blocks fit the kSlots level-1 slots
  static_assert((1 << kSlotBits) == kSlots, "slot bits");
  static_assert(kTileRows / kChunk <= kSlots || kTileRows / (kCap - kChunk + 1) + 1 <= kSlots,
                "sieve flushes per tile");
  static_assert(kCap <= 65535, "u16 run offsets");
};
// k_sieve_rescan: a 16 KiB LDS Bloom filter (a 64 KiB one limits the CU to
// two workgroups, and the rescan then streams at 3.7 instead of 6.1 TB/s:
// tools/stream_bench.hip, profiles/r03/stream_bench.txt); above
// kBloomMaxIds unresolved ids it is skipped and every row tests the bitmap
constexpr int kBloomWords = 4096;  // == 1 << kBloomBits
constexpr unsigned kBloomMaxIds = 8192;
constexpr int kRescanThreads = 512;
constexpr int kRescanBlocks = 1024;

// ============================================================ GLOBAL path ==
__global__ void __launch_bounds__(kBlock) k_pair_sketch(KP kp, const int64_t* __restrict__ pid,
                                                        const int64_t* __restrict__ pk,
                                                        const uint8_t* __restrict__ allowed,
                                                        unsigned long long* sketch, unsigned int* err) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < kp.n; i += stride) {
    const int64_t u = pid[i];
    const int64_t k = pk[i];
    if (u < 0 || u >= kp.U || k < 0 || k >= kp.P) {
      atomicOr(err, 1u);
      continue;
    }
    if (allowed != nullptr && allowed[k] == 0) continue;
    const uint64_t x = pair_key(kp.seed, u, k, 0, kp.rand_shift);
    unsigned long long* s = sketch + u * kp.l0;
    if (x >= s[kp.l0 - 1]) continue;  // values only decrease: a stale read is safe
    sketch_insert(s, kp.l0, x);
  }
}

template <int VALUE_KIND, bool KEEP_ALL_ROWS>
__global__ void __launch_bounds__(kBlock) k_pair_rows(KP kp, const int64_t* __restrict__ pid,
                                                      const int64_t* __restrict__ pk,
                                                      const void* __restrict__ value,
                                                      const uint8_t* __restrict__ allowed,
                                                      const unsigned long long* __restrict__ sketch,
                                                      unsigned int* pair_cnt, unsigned long long* pair_rows,
                                                      double* pair_fsum, double* pair_nsum,
                                                      double* pair_nsum2) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < kp.n; i += stride) {
    const int64_t u = pid[i];
    const int64_t k = pk[i];
    if (u < 0 || u >= kp.U || k < 0 || k >= kp.P) continue;
    if (allowed != nullptr && allowed[k] == 0) continue;
    const uint64_t x = pair_key(kp.seed, u, k, 0, kp.rand_shift);
    const unsigned long long* s = sketch + u * kp.l0;
    if (x > s[kp.l0 - 1]) continue;
    const int j = sketch_find(s, kp.l0, x);
    if (j < 0) continue;
    const int64_t slot = u * kp.l0 + j;
    atomicAdd(pair_cnt + slot, 1u);
    if (!KEEP_ALL_ROWS) {
      const uint64_t y = row_key(kp.row_seed, kp.row_offset + i, (uint32_t)i);
      unsigned long long* r = pair_rows + slot * kp.linf;
      if (y < r[kp.linf - 1]) sketch_insert(r, kp.linf, y);
    } else {
      accumulate_row<VALUE_KIND>(value, (uint32_t)i, slot, pair_fsum, pair_nsum, pair_nsum2, kp.clip);
    }
  }
}

template <int VALUE_KIND, bool KEEP_ALL_ROWS>
__global__ void __launch_bounds__(kBlock) k_reduce_pairs(KP kp, const void* __restrict__ value,
                                                         const unsigned long long* __restrict__ sketch,
                                                         const unsigned int* __restrict__ pair_cnt,
                                                         const unsigned long long* __restrict__ pair_rows,
                                                         const double* __restrict__ pair_fsum,
                                                         const double* __restrict__ pair_nsum,
                                                         const double* __restrict__ pair_nsum2,
                                                         pdp_partition_accumulators acc) {
  const int64_t n_slots = kp.U * kp.l0;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; s < n_slots; s += stride) {
    const uint64_t x = sketch[s];
    if (x == kEmpty) continue;
    const int64_t p = (int64_t)(x & kp.pk_mask);
    const unsigned int c = pair_cnt[s];
    if (c == 0) continue;
    PairSums ps;
    if (!KEEP_ALL_ROWS) {
      const long long m = c < (unsigned)kp.linf ? (long long)c : (long long)kp.linf;
      ps = pair_sums_from_rows<VALUE_KIND>(pair_rows + s * kp.linf, m, value, kp.clip);
    } else if (VALUE_KIND != PDP_VALUE_NONE) {
      ps = pair_sums_from_totals((long long)c, pair_fsum[s], pair_nsum[s], pair_nsum2[s], kp.clip);
    } else {
      ps = PairSums{(long long)c, 0, 0.0, 0.0, 0.0};
    }
    add_pair_to_partition(acc, p, ps, kp.clip.flags);
  }
}

// ========================================================== BUCKETED path ==
// A key whose random part is all ones is "dead" (non-public or invalid
// partition): it keeps its pid bits so it stays in its bucket, and is skipped.
__device__ __forceinline__ bool dead_key(uint64_t x, int rand_shift) {
  return (x | ((1ULL << rand_shift) - 1)) == kEmpty;
}

__global__ void __launch_bounds__(kPartThreads) k_part_hist(KP kp, const int64_t* __restrict__ pid,
                                                            unsigned* __restrict__ counts_tm,
                                                            unsigned* __restrict__ super_tm, unsigned* err) {
  extern __shared__ unsigned hist[];
  for (int64_t b = threadIdx.x; b < kp.n_buckets; b += blockDim.x) hist[b] = 0;
  __syncthreads();
  const int64_t t0 = (int64_t)blockIdx.x * kTileRows;
  const int64_t t1 = t0 + kTileRows < kp.n ? t0 + kTileRows : kp.n;
  for (int64_t i0 = t0 + 2 * (int64_t)threadIdx.x; i0 < t1; i0 += (int64_t)blockDim.x * kUnroll) {
    int64_t u[kUnroll];  // two consecutive rows per 16-byte load
#pragma unroll
    for (int k = 0; k < kUnroll; k += 2) {
      const int64_t i = i0 + (int64_t)k * blockDim.x;
      if (kp.keys_vec && i + 1 < t1) {
        const longlong2 a = *reinterpret_cast<const longlong2*>(pid + i);
        u[k] = a.x;
        u[k + 1] = a.y;
      } else {
        u[k] = i < t1 ? pid[i] : INT64_MIN;
        u[k + 1] = i + 1 < t1 ? pid[i + 1] : INT64_MIN;
      }
    }
#pragma unroll
    for (int k = 0; k < kUnroll; ++k) {
      if (u[k] == INT64_MIN) continue;
      if (u[k] < 0 || u[k] >= kp.U) {
        atomicOr(err, 1u);
        continue;
      }
      atomicAdd(hist + (u[k] >> kp.bucket_bits), 1u);
    }
  }
  __syncthreads();
  unsigned* row = counts_tm + (int64_t)blockIdx.x * kp.cstride;  // tile-major: coalesced
  for (int64_t b = threadIdx.x; b < kp.n_buckets; b += blockDim.x) row[b] = hist[b];
  // this tile's rows per super-bucket (the level-1 scatter's destinations)
  const int64_t nsub = (int64_t)1 << kp.super_bits;
  for (int64_t B = threadIdx.x; B < kp.n_supers; B += blockDim.x) {
    unsigned v = 0;
    const int64_t b1 = (B + 1) * nsub < kp.n_buckets ? (B + 1) * nsub : kp.n_buckets;
    for (int64_t b = B * nsub; b < b1; ++b) v += hist[b];
    super_tm[(int64_t)blockIdx.x * kp.n_supers + B] = v;
  }
}


// Level-2 cursors.  Level 2 runs one workgroup per (group of kL2GroupTiles
// tiles, super-bucket): its records are the runs of those tiles in the
// super-bucket's region, and the rows of bucket b from tiles < t start at
// start[b] + sum over t' < t of counts_tm[t'][b].  These exclusive column
// scans of the tile histogram, taken at group boundaries, are computed in
// three passes over chunks of kScanWaves * kScanTiles tiles (one wave per
// kScanTiles tiles, one lane per bucket): chunk sums, a scan over chunks
// (which also gives the bucket totals), and the cursors at group starts.
// Level 2 then needs no atomics and writes every bucket's rows in tile order.

// counts_tm2 (nullable): the tile-local level 1's second half-tile counts
__device__ __forceinline__ unsigned tile_count(const unsigned* __restrict__ counts_tm,
                                               const unsigned* __restrict__ counts_tm2, int64_t i) {
  return counts_tm[i] + (counts_tm2 != nullptr ? counts_tm2[i] : 0u);
}

__device__ __forceinline__ unsigned tile_slab_sum(const unsigned* __restrict__ counts_tm,
                                                  const unsigned* __restrict__ counts_tm2, int64_t n_tiles,
                                                  int64_t n_buckets, int64_t cstride, int64_t b, int64_t t0) {
  unsigned v = 0;
#pragma unroll
  for (int j = 0; j < kScanTiles; ++j) {
    const int64_t t = t0 + j;
    if (t < n_tiles && b < n_buckets) v += tile_count(counts_tm, counts_tm2, t * cstride + b);
  }
  return v;
}

// csum[chunk][b] = rows of bucket b in the chunk's tiles; gsum (nullable):
// gsum[g][b] = rows of bucket b in the kL2GroupTiles tiles of group g.
// PACKED16: the count rows are u16 pairs (tile-local level 1,
// flush_counts16: cstride / 2 words per row, tile_over adds 65,536 back),
// eight buckets per lane; else u32 rows of cstride, four per lane.  16-byte
// loads, a wave's kScanTiles rows in flight together (C3: 149 MB of counts)
template <bool PACKED16>
__global__ void __launch_bounds__(64 * kScanWaves) k_gscan_sums(const unsigned* __restrict__ counts_tm,
                                                                 const unsigned* __restrict__ counts_tm2,
                                                                 const unsigned* __restrict__ tile_over,
                                                                 int64_t n_tiles, int64_t n_buckets, int64_t cstride,
                                                                 unsigned* __restrict__ csum,
                                                                 unsigned* __restrict__ gsum) {
  static_assert(kScanTiles % kL2GroupTiles == 0, "group sums end inside a wave's tiles");
  constexpr int V = PACKED16 ? 8 : 4;  // buckets per lane
  __shared__ unsigned part[kScanWaves][V][64];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int64_t b0 = ((int64_t)blockIdx.x * 64 + lane) * V;
  const int64_t t0 = (int64_t)blockIdx.y * kScanChunkTiles + (int64_t)w * kScanTiles;
  const int64_t row = PACKED16 ? cstride / 2 : cstride;  // u32 words per row
  const int64_t col = PACKED16 ? b0 / 2 : b0;
  const bool in = b0 < n_buckets;  // then the 16-byte load stays inside the row
  uint4 x[kScanTiles];
  // PACKED16 halves: each u16 of a half tile is <= 2^15 (32,768 rows), so the
  // sum of two can be exactly 2^16 (a bucket holding every row of the tile).
  // The halves are added lane by lane; a lane's carry (bit k of the tile's
  // byte: bucket b0 + k) goes to cy and is added back as 65,536 below
  unsigned cy[kScanTiles / 4];
#pragma unroll
  for (int j = 0; j < kScanTiles / 4; ++j) cy[j] = 0u;
  // (loading all kScanTiles tiles' words before the adds measured slower,
  // 0.084 -> 0.099 ms at C3: the register peak costs occupancy;
  // profiles/r06/ab/ab21_*)
#pragma unroll
  for (int j = 0; j < kScanTiles; ++j) {
    const int64_t t = t0 + j;
    x[j] = make_uint4(0u, 0u, 0u, 0u);
    if (in && t < n_tiles) {
      x[j] = *reinterpret_cast<const uint4*>(counts_tm + t * row + col);
      if (counts_tm2 != nullptr) {
        const uint4 y = *reinterpret_cast<const uint4*>(counts_tm2 + t * row + col);
        if constexpr (PACKED16) {
          const unsigned a[4] = {x[j].x, x[j].y, x[j].z, x[j].w}, b[4] = {y.x, y.y, y.z, y.w};
          unsigned s[4], c = 0u;
#pragma unroll
          for (int k = 0; k < 4; ++k) {
            const unsigned lo = (a[k] & 0xFFFFu) + (b[k] & 0xFFFFu), hi = (a[k] >> 16) + (b[k] >> 16);
            s[k] = (lo & 0xFFFFu) | (hi << 16);
            c |= ((lo >> 16) | ((hi >> 16) << 1)) << (2 * k);
          }
          x[j] = make_uint4(s[0], s[1], s[2], s[3]);
          cy[j / 4] |= c << (8 * (j % 4));
        } else {
          x[j] = make_uint4(x[j].x + y.x, x[j].y + y.y, x[j].z + y.z, x[j].w + y.w);
        }
      }
    }
  }
  unsigned v[V], gv[V];
#pragma unroll
  for (int k = 0; k < V; ++k) v[k] = gv[k] = 0u;
#pragma unroll
  for (int j = 0; j < kScanTiles; ++j) {
    const unsigned e[4] = {x[j].x, x[j].y, x[j].z, x[j].w};
#pragma unroll
    for (int k = 0; k < V; ++k)
      gv[k] += PACKED16 ? ((e[k / 2] >> (16 * (k & 1))) & 0xFFFFu) + (((cy[j / 4] >> (8 * (j % 4) + k)) & 1u) << 16)
                        : e[k];
    if (PACKED16 && tile_over != nullptr && in && t0 + j < n_tiles) {
      const unsigned o = tile_over[t0 + j];  // the bucket with all 65,536 rows, or ~0
#pragma unroll
      for (int k = 0; k < V; ++k) gv[k] += (o == (unsigned)(b0 + k)) ? 65536u : 0u;
    }
    if ((j + 1) % kL2GroupTiles == 0) {
      if (gsum != nullptr && in && t0 + j + 1 - kL2GroupTiles < n_tiles) {
        unsigned* g = gsum + ((t0 + j + 1) / kL2GroupTiles - 1) * n_buckets + b0;
#pragma unroll
        for (int k = 0; k < V; ++k)
          if (b0 + k < n_buckets) g[k] = gv[k];
      }
#pragma unroll
      for (int k = 0; k < V; ++k) {
        v[k] += gv[k];
        gv[k] = 0u;
      }
    }
  }
#pragma unroll
  for (int k = 0; k < V; ++k) part[w][k][lane] = v[k];
  __syncthreads();
  if (w == 0 && in) {
    unsigned* c = csum + (int64_t)blockIdx.y * n_buckets + b0;
#pragma unroll
    for (int k = 0; k < V; ++k) {
      unsigned sum = 0;
      for (int q = 0; q < kScanWaves; ++q) sum += part[q][k][lane];
      if (b0 + k < n_buckets) c[k] = sum;
    }
  }
}

// per bucket: exclusive scan of the chunk sums in place, total -> total[b]
__global__ void __launch_bounds__(kBlock) k_gscan_chunks(unsigned* __restrict__ csum, int64_t n_chunks,
                                                         int64_t n_buckets, unsigned* __restrict__ total) {
  const int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= n_buckets) return;
  unsigned run = 0;
  constexpr int B = 16;  // loads in flight per thread (the in-place stores would serialise them)
  for (int64_t c0 = 0; c0 < n_chunks; c0 += B) {
    unsigned v[B];
#pragma unroll
    for (int j = 0; j < B; ++j) v[j] = c0 + j < n_chunks ? csum[(c0 + j) * n_buckets + b] : 0u;
#pragma unroll
    for (int j = 0; j < B; ++j) {
      if (c0 + j < n_chunks) csum[(c0 + j) * n_buckets + b] = run;
      run += v[j];
    }
  }
  total[b] = run;
}

// gcur[g][b] in place: the group sums of k_gscan_sums -> rows of bucket b in
// tiles < g * kL2GroupTiles (cpre: k_gscan_chunks' exclusive chunk sums)
__global__ void __launch_bounds__(kBlock) k_gscan_groups(const unsigned* __restrict__ cpre, int64_t n_tiles,
                                                         int64_t n_buckets, unsigned* __restrict__ gcur) {
  const int64_t n_sc = (n_tiles + kScanChunkTiles - 1) / kScanChunkTiles;
  const int64_t n_grp = (n_tiles + kL2GroupTiles - 1) / kL2GroupTiles;
  constexpr int kGroups = kScanChunkTiles / kL2GroupTiles;
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_sc * n_buckets) return;
  const int64_t c = i / n_buckets, b = i % n_buckets;
  unsigned run = cpre[i];
  unsigned v[kGroups];  // all loads first (the in-place stores would serialise them)
#pragma unroll
  for (int k = 0; k < kGroups; ++k) {
    const int64_t g = c * kGroups + k;
    v[k] = g < n_grp ? gcur[g * n_buckets + b] : 0u;
  }
#pragma unroll
  for (int k = 0; k < kGroups; ++k) {
    const int64_t g = c * kGroups + k;
    if (g < n_grp) gcur[g * n_buckets + b] = run;
    run += v[k];
  }
}

// gcur[g][b] = rows of bucket b in tiles < g * kL2GroupTiles
__global__ void __launch_bounds__(64 * kScanWaves) k_gscan_cursors(const unsigned* __restrict__ counts_tm,
                                                                    const unsigned* __restrict__ counts_tm2,
                                                                    int64_t n_tiles, int64_t n_buckets,
                                                                    int64_t cstride,
                                                                    const unsigned* __restrict__ cpre,
                                                                    unsigned* __restrict__ gcur) {
  __shared__ unsigned part[kScanWaves][64];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int64_t b = (int64_t)blockIdx.x * 64 + lane;
  const int64_t t0 = (int64_t)blockIdx.y * kScanChunkTiles + (int64_t)w * kScanTiles;
  part[w][lane] = tile_slab_sum(counts_tm, counts_tm2, n_tiles, n_buckets, cstride, b, t0);
  __syncthreads();
  if (b >= n_buckets || t0 >= n_tiles) return;
  unsigned run = cpre[(int64_t)blockIdx.y * n_buckets + b];
  for (int k = 0; k < w; ++k) run += part[k][lane];
  for (int j = 0; j < kScanTiles; ++j) {
    const int64_t t = t0 + j;
    if (t >= n_tiles) break;
    if (t % kL2GroupTiles == 0) gcur[(t / kL2GroupTiles) * n_buckets + b] = run;
    run += tile_count(counts_tm, counts_tm2, t * cstride + b);
  }
}

// super_base[B] = start of super-bucket B
__global__ void __launch_bounds__(kBlock) k_super_bases(KP kp, const unsigned* __restrict__ counts,
                                                        unsigned* __restrict__ super_base) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i <= kp.n_supers) {
    const int64_t b = i << kp.super_bits;
    super_base[i] = counts[b < kp.n_buckets ? b : kp.n_buckets];
  }
}

// LDS-staged multi-destination write: the rows of one sub-chunk (ITEMS per
// thread) are counting-sorted by destination in LDS and each destination's
// run is then written contiguously at gcur[dest] (coalesced, long runs).
constexpr int kMaxDest = 1024;

// row record key of the partition passes: u64 record (PDP_KEYS_WIDE: dead bit
// 63, bucket-within-super and local pid, partition; expand_key gives its pair key) or u32
// compact record (PDP_KEYS_COMPACT, and PDP_KEYS_PACKED from level 2 on)
template <bool COMPACT>
using RecKey = typename std::conditional<COMPACT, uint32_t, unsigned long long>::type;
// level-1 record key per format (PACKED: the u64 packed record, no row array)
template <int FMT>
using L1Key = typename std::conditional<FMT == PDP_KEYS_COMPACT, uint32_t, unsigned long long>::type;
template <int FMT>
constexpr bool kPackedL1 =
    FMT == PDP_KEYS_PACKED || FMT == PDP_KEYS_PACKED_WIDE || FMT == PDP_KEYS_PACKED64;  // no level-1 row array
// level-2 (bucket-order) record key per format
template <int FMT>
using L2Key = RecKey<FMT != PDP_KEYS_WIDE && FMT != PDP_KEYS_PACKED_WIDE && FMT != PDP_KEYS_PACKED64>;
// level-2 records of the bucket kernel: u32 key + u32 row (COMPACT, and
// PACKED from level 2 on), u64 key + u32 row (WIDE, PACKED_WIDE), one u64
// with the row in its high bits (PACKED64; all ones = dead)
constexpr int kRecCompact = 0, kRecWide = 1, kRecP64 = 2;
template <int FMT>
constexpr int kRecOf = FMT == PDP_KEYS_PACKED64 ? kRecP64
                                                 : ((FMT == PDP_KEYS_WIDE || FMT == PDP_KEYS_PACKED_WIDE) ? kRecWide
                                                                                                          : kRecCompact);
inline int rec_of(int key_format) {
  return key_format == PDP_KEYS_PACKED64 ? kRecP64
                                         : ((key_format == PDP_KEYS_WIDE || key_format == PDP_KEYS_PACKED_WIDE)
                                                ? kRecWide : kRecCompact);
}

// ------------------------------------------------------ format visitors --
// f(std::integral_constant<int, X>{}) for a run-time record kind, key format
// or (value kind, keep every row): the one place each ladder is written
template <typename F>
int with_rec(int kind, F&& f) {
  if (kind == kRecCompact) return f(std::integral_constant<int, kRecCompact>{});
  if (kind == kRecWide) return f(std::integral_constant<int, kRecWide>{});
  return f(std::integral_constant<int, kRecP64>{});
}
template <typename F>
int with_key_format(int fmt, F&& f) {
  if (fmt == PDP_KEYS_COMPACT) return f(std::integral_constant<int, PDP_KEYS_COMPACT>{});
  if (fmt == PDP_KEYS_PACKED) return f(std::integral_constant<int, PDP_KEYS_PACKED>{});
  if (fmt == PDP_KEYS_PACKED_WIDE) return f(std::integral_constant<int, PDP_KEYS_PACKED_WIDE>{});
  if (fmt == PDP_KEYS_PACKED64) return f(std::integral_constant<int, PDP_KEYS_PACKED64>{});
  return f(std::integral_constant<int, PDP_KEYS_WIDE>{});
}
template <typename F>
int with_value(int value_kind, bool keep_all, F&& f) {
  auto kind = [&](auto ka) {
    if (value_kind == PDP_VALUE_NONE) return f(std::integral_constant<int, PDP_VALUE_NONE>{}, ka);
    if (value_kind == PDP_VALUE_F64) return f(std::integral_constant<int, PDP_VALUE_F64>{}, ka);
    return f(std::integral_constant<int, PDP_VALUE_I64>{}, ka);
  };
  return keep_all ? kind(std::true_type{}) : kind(std::false_type{});
}

// MAXD destinations per stage; the small form (<= 256 destinations, u8 tags)
// fits four workgroups per CU with compact keys instead of three.  ROWS:
// the stage carries a u32 row array beside the keys.
template <typename K, int MAXD, bool ROWS, int N, int THREADS = kPartThreads>
struct StageLds {
  using D = typename std::conditional<(MAXD <= 256), uint8_t, unsigned short>::type;
  unsigned hist[MAXD];
  unsigned start[MAXD];
  unsigned gcur[MAXD];
  K keys[THREADS * N];
  unsigned rows[ROWS ? THREADS * N : 1];
  D dest[THREADS * N];
};
constexpr int kSmallDest = 256;  // u8 tags; 39.9 KB with compact keys: four workgroups per CU

}  // namespace

// the sizes the planner asks for (declared in pdp_bound_plan.h)
size_t l1_stage_bytes(int key_format) {
  switch (key_format) {
    case PDP_KEYS_COMPACT: return sizeof(StageLds<L1Key<PDP_KEYS_COMPACT>, kSmallDest, true, kL1Items, kL1Threads>);
    case PDP_KEYS_PACKED:
    case PDP_KEYS_PACKED_WIDE:
    case PDP_KEYS_PACKED64: return sizeof(StageLds<L1Key<PDP_KEYS_PACKED>, kSmallDest, false, kL1Items, kL1Threads>);
    default: return sizeof(StageLds<L1Key<PDP_KEYS_WIDE>, kSmallDest, true, kL1Items, kL1Threads>);
  }
}

template <int TH>
size_t sieve_stage_bytes_t(int key_format) {
  switch (key_format) {
    case PDP_KEYS_COMPACT: return sizeof(StageLds<L1Key<PDP_KEYS_COMPACT>, kSmallDest, true, kSieveItems, TH>);
    case PDP_KEYS_PACKED:
    case PDP_KEYS_PACKED_WIDE:
    case PDP_KEYS_PACKED64: return sizeof(StageLds<L1Key<PDP_KEYS_PACKED>, kSmallDest, false, kSieveItems, TH>);
    default: return sizeof(StageLds<L1Key<PDP_KEYS_WIDE>, kSmallDest, true, kSieveItems, TH>);
  }
}
size_t sieve_stage_bytes(int key_format, int threads) {
  return threads == kSieveThreads2 ? sieve_stage_bytes_t<kSieveThreads2>(key_format)
                                   : sieve_stage_bytes_t<kL1Threads>(key_format);
}
int sieve_slot_bits(int threads) {
  return threads == kSieveThreads2 ? SieveShape<kSieveThreads2>::kSlotBits : SieveShape<kL1Threads>::kSlotBits;
}

namespace {

// phase 1: histogram + local rank (dest < 0 = drop the row)
template <typename K, int MAXD, bool ROWS, int N, int TH>
__device__ __forceinline__ void stage_count(StageLds<K, MAXD, ROWS, N, TH>& s, int ndest, const int (&d)[N],
                                            unsigned (&rank)[N]) {
  for (int t = threadIdx.x; t < ndest; t += blockDim.x) s.hist[t] = 0;
  __syncthreads();
#pragma unroll
  for (int q = 0; q < N; ++q) rank[q] = d[q] >= 0 ? atomicAdd(s.hist + d[q], 1u) : 0;
  __syncthreads();
  if (threadIdx.x < 64) {  // exclusive scan of hist by one wave
    const int lane = threadIdx.x;
    unsigned carry = 0;
    for (int base = 0; base < ndest; base += 64) {
      const unsigned v = base + lane < ndest ? s.hist[base + lane] : 0;
      unsigned incl = v;
      for (int off = 1; off < 64; off <<= 1) {
        const unsigned up = __shfl_up(incl, off, 64);
        if (lane >= off) incl += up;
      }
      if (base + lane < ndest) s.start[base + lane] = carry + incl - v;
      carry += __shfl(incl, 63, 64);
    }
  }
  __syncthreads();
}

// phase 2: place into the LDS stage, then write every run at gcur[dest]
template <typename K, int MAXD, bool ROWS, int N, int TH>
__device__ __forceinline__ void stage_write(StageLds<K, MAXD, ROWS, N, TH>& s, int ndest, const int (&d)[N],
                                            const unsigned (&rank)[N], const K (&x)[N],
                                            const unsigned (&r)[N], K* __restrict__ out_keys,
                                            unsigned* __restrict__ out_rows) {
#pragma unroll
  for (int q = 0; q < N; ++q) {
    if (d[q] < 0) continue;
    const unsigned slot = s.start[d[q]] + rank[q];
    s.keys[slot] = x[q];
    if (ROWS) s.rows[slot] = r[q];
    s.dest[slot] = (typename StageLds<K, MAXD, ROWS, N, TH>::D)d[q];
  }
  __syncthreads();
  const unsigned total = s.start[ndest - 1] + s.hist[ndest - 1];
  for (unsigned k = threadIdx.x; k < total; k += blockDim.x) {
    const unsigned dd = s.dest[k];
    const unsigned g = s.gcur[dd] + (k - s.start[dd]);
    out_keys[g] = s.keys[k];
    if (ROWS) out_rows[g] = s.rows[k];
  }
  __syncthreads();
}

// Compact row record: bit 31 = dead (non-public / invalid partition: skipped,
// but kept in its bucket), bits [pk_bits, pk_bits + bucket_bits + super_bits)
// = the pid's bucket-within-super and bucket-local bits, [0, pk_bits) = pk.
__device__ __forceinline__ uint32_t compact_key(const KP& kp, int64_t u, int64_t k, bool dead) {
  const uint32_t mid = (uint32_t)((uint64_t)u & ((1ULL << (kp.bucket_bits + kp.super_bits)) - 1));
  return dead ? (0x80000000u | (mid << kp.pk_bits)) : ((mid << kp.pk_bits) | (uint32_t)k);
}

// Packed level-1 record (PDP_KEYS_PACKED): bit 63 = dead, bits [47, 63) = the
// row's index within its 65,536-row tile, [pk_bits, pk_bits + bucket_bits +
// super_bits) = bucket-within-super and bucket-local pid, [0, pk_bits) = pk.
// The tile is not stored: level 2 recovers it from the record's position in
// its super-bucket region (the tiles' runs there are in tile order).
constexpr int kPackedRowShift = 63 - kTileRowBits;
__device__ __forceinline__ uint64_t packed_key(const KP& kp, int64_t u, int64_t k, uint32_t tile_row, bool dead) {
  const uint64_t mid = (uint64_t)u & ((1ULL << (kp.bucket_bits + kp.super_bits)) - 1);
  return (dead ? (1ULL << 63) : 0ULL) | ((uint64_t)tile_row << kPackedRowShift) | (mid << kp.pk_bits) |
         (dead ? 0ULL : (uint64_t)k);
}

// The pair key of a row record (dead records -> kEmpty, skipped): random
// bits from rand_shift = pk_bits + bucket_bits up, the bucket-local pid, the
// partition -- pair_key(seed, pid, pk, local << pk_bits, rand_shift).  hpid[]
// holds pid_hash of the bucket's 2^bucket_bits privacy ids (LDS).  COMPACT
// records are u32 (bit 31 dead), WIDE records u64 (bit 63 dead); both keep
// the bucket-within-super bits above the local pid, which the key drops.
__device__ __forceinline__ uint64_t expand_key(const KP& kp, const uint2* hpid, uint32_t v) {
  // COMPACT records have rand_shift = pk_bits + bucket_bits <= 31, so the
  // pair key is the 32-bit pair hash above the record's (local pid,
  // partition) bits -- the bucket-within-super bits above them dropped -- and
  // pair_key_from's all-ones guard cannot fire
  if (v >> 31) return kEmpty;
  const uint32_t local = (v >> kp.pk_bits) & ((1u << kp.bucket_bits) - 1);
  return ((uint64_t)pair_hash_from(hpid[local].x, kp.seed, (int64_t)(v & (uint32_t)kp.pk_mask)) << 32) |
         (v & ((1u << kp.rand_shift) - 1));
}
__device__ __forceinline__ uint64_t expand_key(const KP& kp, const uint2* hpid, unsigned long long v) {
  if (v >> 63) return kEmpty;
  const uint64_t local = (v >> kp.pk_bits) & ((1ULL << kp.bucket_bits) - 1);
  return pair_key_from(hpid[local].x, kp.seed, (int64_t)(v & kp.pk_mask), local << kp.pk_bits, kp.rand_shift);
}

// B1's candidate test in one LDS read: hpid[local] = {pid hash, high 32 bits
// of the pid's sketch maximum (or above it: the maximum only decreases)}; a
// record whose key's high half exceeds that cannot be at or below the
// maximum.  Returns the pair key of a candidate, kEmpty otherwise.
__device__ __forceinline__ uint64_t b1_candidate(const KP& kp, const uint2* hpid, uint32_t v) {
  if (v >> 31) return kEmpty;
  const uint32_t local = (v >> kp.pk_bits) & ((1u << kp.bucket_bits) - 1);
  const uint2 e = hpid[local];
  const uint32_t h = pair_hash_from(e.x, kp.seed, (int64_t)(v & (uint32_t)kp.pk_mask));
  return h <= e.y ? (((uint64_t)h << 32) | (v & ((1u << kp.rand_shift) - 1))) : kEmpty;
}
__device__ __forceinline__ uint64_t b1_candidate(const KP& kp, const uint2* hpid, unsigned long long v) {
  const uint64_t x = expand_key(kp, hpid, v);
  if (x == kEmpty) return kEmpty;
  const uint32_t local = (uint32_t)((v >> kp.pk_bits) & ((1ULL << kp.bucket_bits) - 1));
  return (uint32_t)(x >> 32) <= hpid[local].y ? x : kEmpty;
}

// Level 1: tile rows -> super-bucket regions (<= 64 destinations per tile).
template <int FMT>
__global__ void __launch_bounds__(kL1Threads)  k_scatter_l1(KP kp, const int64_t* __restrict__ pid,
                                                             const int64_t* __restrict__ pk,
                                                             const uint8_t* __restrict__ allowed,
                                                             const unsigned* __restrict__ super_off,
                                                             const unsigned* __restrict__ super_base,
                                                             L1Key<FMT>* __restrict__ keys1,
                                                             unsigned* __restrict__ rows1, unsigned* err) {
  using K = L1Key<FMT>;
  constexpr bool ROWS = FMT != PDP_KEYS_PACKED;
  extern __shared__ unsigned long long stage_raw[];
  static_assert(kMaxSupers <= kSmallDest, "level-1 destinations must fit the small stage");
  using SL = StageLds<K, kSmallDest, ROWS, kL1Items, kL1Threads>;
  SL& s = *reinterpret_cast<SL*>(stage_raw);
  const int64_t t = blockIdx.x;
  const int nd = (int)kp.n_supers;
  // this tile's first row in each super-bucket region (k_super_scan)
  for (int B = threadIdx.x; B < nd; B += blockDim.x) s.gcur[B] = super_base[B] + super_off[t * nd + B];
  __syncthreads();
  const int64_t t0 = t * kTileRows;
  const int64_t t1 = t0 + kTileRows < kp.n ? t0 + kTileRows : kp.n;
  const int mid_bits = kp.bucket_bits + kp.super_bits;
  const uint64_t mid_mask = (1ULL << mid_bits) - 1;
  // two consecutive rows per 16-byte load (tiles and chunks start even)
  auto load = [&](int64_t c0, int64_t (&u)[kL1Items], int64_t (&k)[kL1Items]) {
#pragma unroll
    for (int q = 0; q < kL1Items; q += 2) {
      const int64_t i = c0 + 2 * ((int64_t)threadIdx.x + (int64_t)(q / 2) * blockDim.x);
      if (kp.keys_vec && i + 1 < t1) {
        const longlong2 a = *reinterpret_cast<const longlong2*>(pid + i);
        const longlong2 c = *reinterpret_cast<const longlong2*>(pk + i);
        u[q] = a.x;
        u[q + 1] = a.y;
        k[q] = c.x;
        k[q + 1] = c.y;
      } else {
        u[q] = i < t1 ? pid[i] : -1;
        k[q] = i < t1 ? pk[i] : 0;
        u[q + 1] = i + 1 < t1 ? pid[i + 1] : -1;
        k[q + 1] = i + 1 < t1 ? pk[i + 1] : 0;
      }
    }
  };
  int64_t u[kL1Items], k[kL1Items];
  if (t0 < t1) load(t0, u, k);
  for (int64_t c0 = t0; c0 < t1; c0 += kL1Rows) {
    int d[kL1Items];
    K x[kL1Items];
    unsigned r[kL1Items];
#pragma unroll
    for (int q = 0; q < kL1Items; ++q) {
      r[q] = (unsigned)(c0 + 2 * ((int64_t)threadIdx.x + (int64_t)(q / 2) * blockDim.x) + (q & 1));
      if (u[q] < 0 || u[q] >= kp.U) {  // flagged by k_part_hist, not counted
        d[q] = -1;
        x[q] = 0;
        continue;
      }
      d[q] = (int)(u[q] >> mid_bits);
      bool is_dead = false;
      if (k[q] < 0 || k[q] >= kp.P) {
        atomicOr(err, 1u);
        is_dead = true;
      } else if (allowed != nullptr && allowed[k[q]] == 0) {
        is_dead = true;
      }
      if constexpr (FMT == PDP_KEYS_COMPACT) {
        x[q] = (K)compact_key(kp, u[q], k[q], is_dead);
      } else if constexpr (FMT == PDP_KEYS_PACKED) {
        x[q] = (K)packed_key(kp, u[q], k[q], (uint32_t)(r[q] - (unsigned)t0), is_dead);
      } else {  // WIDE: u64 (dead bit 63 | bucket-within-super and local pid | partition)
        const uint64_t midv = ((uint64_t)u[q] & mid_mask) << kp.pk_bits;
        x[q] = (K)(is_dead ? ((1ULL << 63) | midv) : (midv | (uint64_t)k[q]));
      }
    }
    unsigned rank[kL1Items];
    stage_count(s, nd, d, rank);
    stage_write(s, nd, d, rank, x, r, keys1, rows1);
    for (int B = threadIdx.x; B < nd; B += blockDim.x) s.gcur[B] += s.hist[B];
    __syncthreads();
    if (c0 + kL1Rows < t1) load(c0 + kL1Rows, u, k);
  }
}

// Level 2: one workgroup per (group g of kL2GroupTiles tiles, super-bucket
// B) moves the runs of those tiles in B's region -- in tile order, so one
// contiguous range -- into B's 2^super_bits bucket regions, kL2Rows records
// per LDS stage.  Every bucket's write cursor starts at start[b] + gcur[g][b]
// (k_gscan_cursors) and advances in LDS: no atomics, each bucket's rows land
// in tile order, and consecutive stages of a workgroup append to the same
// runs (their partial cache lines meet in the same L2).  PACKED input: the
// u64 packed records are unpacked into COMPACT (key, row) pairs, the row =
// tile * 65,536 + tile row, the tile found among the group's run starts.
template <int FMT, int MAXD>
__global__ void __launch_bounds__(kL2Threads)  k_scatter_l2(KP kp, const unsigned* __restrict__ super_base,
                                                             const unsigned* __restrict__ super_off,
                                                             const unsigned* __restrict__ bucket_start,
                                                             const unsigned* __restrict__ gcur,
                                                             const L1Key<FMT>* __restrict__ keys1,
                                                             const unsigned* __restrict__ rows1,
                                                             L2Key<FMT>* __restrict__ keys2,
                                                             unsigned* __restrict__ rows2) {
  using KI = L1Key<FMT>;
  using KO = L2Key<FMT>;
  constexpr bool PACKED = FMT == PDP_KEYS_PACKED;
  constexpr int R = 16 / sizeof(KI);  // records per 16-byte key load
  extern __shared__ unsigned long long stage_raw[];
  using SL = StageLds<KO, MAXD, true, kL2Items, kL2Threads>;
  SL& s = *reinterpret_cast<SL*>(stage_raw);
  __shared__ unsigned toff[kL2GroupTiles + 1];  // run starts of the group's tiles, relative to B's region
  const int64_t g = blockIdx.x;
  const int B = blockIdx.y;
  const int64_t T0 = g * kL2GroupTiles;
  const int J = (int)(kp.n_tiles - T0 < kL2GroupTiles ? kp.n_tiles - T0 : kL2GroupTiles);
  const int64_t sb = super_base[B];
  if (threadIdx.x <= J) {
    const int64_t t = T0 + threadIdx.x;
    toff[threadIdx.x] = t < kp.n_tiles ? super_off[t * kp.n_supers + B] : (unsigned)(super_base[B + 1] - sb);
  }
  const int nsub = 1 << kp.super_bits;
  const int64_t s_first = (int64_t)B << kp.super_bits;
  for (int t = threadIdx.x; t < nsub; t += blockDim.x) {
    const int64_t b = s_first + t;
    s.gcur[t] = b < kp.n_buckets ? bucket_start[b] + gcur[g * kp.n_buckets + b] : 0u;
  }
  __syncthreads();
  const int64_t lo = sb + toff[0], hi = sb + toff[J];
  if (lo >= hi) return;  // block-uniform
  const int bb = kp.bucket_bits;
  const uint32_t local_mask = (1u << bb) - 1;
  // PACKED: tile of the record at absolute index i; a thread's records come
  // in increasing order, so the cursor only moves forward
  int jcur = 0;
  auto tile_of = [&](int64_t i) -> int64_t {
    const int64_t o = i - sb;
    while (jcur + 1 < J && (int64_t)toff[jcur + 1] <= o) ++jcur;
    return T0 + jcur;
  };
  auto unpack = [&](uint64_t v, int64_t i, KO* key, unsigned* row, int* dest) {
    const uint32_t mid = (uint32_t)((v >> kp.pk_bits) & ((1ULL << (bb + kp.super_bits)) - 1));
    *dest = (int)(mid >> bb);
    const uint32_t lpk = ((mid & local_mask) << kp.pk_bits);
    *key = (KO)((v >> 63) ? (0x80000000u | lpk) : (lpk | (uint32_t)(v & kp.pk_mask)));
    const uint32_t trow = (uint32_t)((v >> kPackedRowShift) & (kTileRows - 1));
    *row = (unsigned)(tile_of(i) * kTileRows + trow);
  };
  const int sub_shift = kp.pk_bits + kp.bucket_bits;
  const uint64_t sub_mask = (uint64_t)nsub - 1;
  for (int64_t base = lo & ~(int64_t)(R - 1); base < hi; base += kL2Rows) {
    const int64_t r0 = base > lo ? base : lo;
    const int64_t r1 = base + kL2Rows < hi ? base + kL2Rows : hi;
    KO x[kL2Items];
    unsigned r[kL2Items];
    int d[kL2Items];
#pragma unroll
    for (int q = 0; q < kL2Items; q += R) {  // R records per 16-byte key load
      const int64_t i = base + R * ((int64_t)threadIdx.x + (int64_t)(q / R) * blockDim.x);
      if (i >= r0 && i + R - 1 < r1) {
        if constexpr (PACKED) {
          const ulonglong2 a = *reinterpret_cast<const ulonglong2*>(keys1 + i);
          unpack(a.x, i, &x[q], &r[q], &d[q]);
          unpack(a.y, i + 1, &x[q + 1], &r[q + 1], &d[q + 1]);
        } else if constexpr (R == 4) {
          const uint4 a = *reinterpret_cast<const uint4*>(keys1 + i);
          const uint4 c = *reinterpret_cast<const uint4*>(rows1 + i);
          x[q] = a.x; x[q + 1] = a.y; x[q + 2] = a.z; x[q + 3] = a.w;
          r[q] = c.x; r[q + 1] = c.y; r[q + 2] = c.z; r[q + 3] = c.w;
        } else {
          const ulonglong2 a = *reinterpret_cast<const ulonglong2*>(keys1 + i);
          const uint2 c = *reinterpret_cast<const uint2*>(rows1 + i);
          x[q] = a.x; x[q + 1] = a.y;
          r[q] = c.x; r[q + 1] = c.y;
        }
        if constexpr (!PACKED) {
#pragma unroll
          for (int e = 0; e < R; ++e) d[q + e] = (int)((x[q + e] >> sub_shift) & sub_mask);
        }
      } else {
#pragma unroll
        for (int e = 0; e < R; ++e) {
          const bool ok = i + e >= r0 && i + e < r1;
          if constexpr (PACKED) {
            if (ok) unpack(keys1[i + e], i + e, &x[q + e], &r[q + e], &d[q + e]);
            else { x[q + e] = 0; r[q + e] = 0; d[q + e] = -1; }
          } else {
            x[q + e] = ok ? keys1[i + e] : 0;
            r[q + e] = ok ? rows1[i + e] : 0;
            d[q + e] = ok ? (int)((x[q + e] >> sub_shift) & sub_mask) : -1;
          }
        }
      }
    }
    unsigned rank[kL2Items];
    stage_count(s, nsub, d, rank);
    stage_write(s, nsub, d, rank, x, r, keys2, rows2);
    for (int t = threadIdx.x; t < nsub; t += blockDim.x) s.gcur[t] += s.hist[t];
    __syncthreads();
  }
}

// super_off[t][B] = rows of super-bucket B in tiles < t (exclusive scan over
// tiles, one workgroup per super-bucket): the level-1 scatter's per-tile
// write offsets, read as one contiguous row per tile
__global__ void __launch_bounds__(kBlock) k_super_scan(KP kp, const unsigned* __restrict__ super_tm,
                                                       unsigned* __restrict__ super_off) {
  __shared__ unsigned wsum[kBlock / 64 + 1];
  const int64_t B = blockIdx.x;
  unsigned carry = 0;
  for (int64_t t0 = 0; t0 < kp.n_tiles; t0 += blockDim.x) {
    const int64_t t = t0 + threadIdx.x;
    const unsigned x = t < kp.n_tiles ? super_tm[t * kp.n_supers + B] : 0u;
    unsigned total;
    const unsigned ex = block_excl_scan(x, wsum, &total);
    if (t < kp.n_tiles) super_off[t * kp.n_supers + B] = carry + ex;
    carry += total;
    __syncthreads();  // wsum is reused by the next chunk
  }
}

// ------------------------------------------------ tile-local level 1 / 2 --
// Plan.l1_local: level 1 needs no histogram pass before it.  Each 4,096-row
// stage is counting-sorted by super-bucket in LDS and written whole to its
// own block keys1[stage * kL1Rows, + rows kept) -- one contiguous span per
// stage -- with soff[stage][B] (u16, n_supers + 1 entries) = where
// super-bucket B's run starts in that block.  The tile's rows per bucket
// (counts_tm, the level-2 cursor input) are counted in LDS on the way, so the
// privacy-id column is read once (k_part_hist + k_super_scan are not run).
static_assert(kTileRows % kL1Rows == 0, "a tile is a whole number of level-1 stages");
static_assert(kL2Runs * kSieveL2Groups <= kL2Threads, "one level-1 slot per thread in the run scan");
static_assert(kSieveTileStride == kTileRows && kBandTileStride >= kTileRows, "level 2 recovers a run's tile from its position");

// the LDS stage block [0, total) -> dst, 16 bytes per lane
template <typename K>
__device__ __forceinline__ void copy_block(K* __restrict__ dst, const K* src, unsigned total) {
  constexpr unsigned V = 16 / sizeof(K);
  using VT = typename std::conditional<V == 4, uint4, ulonglong2>::type;
  const unsigned nv = total / V;
  for (unsigned k = threadIdx.x; k < nv; k += blockDim.x)
    reinterpret_cast<VT*>(dst)[k] = reinterpret_cast<const VT*>(src)[k];
  for (unsigned k = nv * V + threadIdx.x; k < total; k += blockDim.x) dst[k] = src[k];
}

// The tile-local level 1's bucket counts leave LDS as u16 pairs per u32
// word (rows of kp.cstride / 2 words; bucket 2w in the low half): half the
// bytes of u32 counts for level 1 to write and k_gscan_sums to read.  The
// LDS counts are u32 per bucket, or (U16) already u16 pairs of a half tile
// (<= 2^15 each; two halves can add up to 2^16, which k_gscan_sums adds lane
// by lane with the carry kept apart).  A u32 count of 65,536 -- every row of the tile in one
// bucket -- is stored as 0 with the bucket in tile_over[t], which the scan
// adds back (tile_over is all ones otherwise; the caller sets it so).
template <bool U16>
__device__ __forceinline__ void flush_counts16(unsigned* __restrict__ bh, int64_t n_buckets,
                                               unsigned* __restrict__ dst, unsigned* __restrict__ over, int th) {
  const int64_t n_pairs = (n_buckets + 1) / 2;
  for (int64_t w = threadIdx.x; w < n_pairs; w += th) {
    if constexpr (U16) {
      dst[w] = bh[w];
      bh[w] = 0;
    } else {
      const unsigned v0 = bh[2 * w], v1 = 2 * w + 1 < n_buckets ? bh[2 * w + 1] : 0u;
      bh[2 * w] = 0;
      if (2 * w + 1 < n_buckets) bh[2 * w + 1] = 0;
      dst[w] = (v0 & 0xFFFFu) | (v1 << 16);
      if (v0 > 0xFFFFu) *over = (unsigned)(2 * w);
      if (v1 > 0xFFFFu) *over = (unsigned)(2 * w + 1);
    }
  }
}

template <int FMT, bool U16>
__global__ void __launch_bounds__(kL1Threads)  k_scatter_l1_local(KP kp, const int64_t* __restrict__ pid,
                                                                   const int64_t* __restrict__ pk,
                                                                   const uint8_t* __restrict__ allowed,
                                                                   unsigned* __restrict__ counts_tm,
                                                                   unsigned* __restrict__ counts_tm2,
                                                                   uint16_t* __restrict__ soff,
                                                                   L1Key<FMT>* __restrict__ keys1,
                                                                   unsigned* __restrict__ rows1, unsigned* err,
                                                                   unsigned* __restrict__ tile_over) {
  using K = L1Key<FMT>;
  constexpr bool ROWS = !kPackedL1<FMT>;
  extern __shared__ unsigned long long stage_raw[];
  using SL = StageLds<K, kSmallDest, ROWS, kL1Items, kL1Threads>;
  SL& s = *reinterpret_cast<SL*>(stage_raw);
  // rows per bucket: u32 each, or (U16) two u16 per word, flushed every half
  // tile so that no count carries into its neighbour
  unsigned* bh = reinterpret_cast<unsigned*>(stage_raw + (sizeof(SL) + 7) / 8);
  const int64_t n_words = U16 ? (kp.n_buckets + 1) / 2 : kp.n_buckets;
  for (int64_t b = threadIdx.x; b < n_words; b += blockDim.x) bh[b] = 0;
  __syncthreads();
  const int64_t t = blockIdx.x;
  auto flush = [&](unsigned* __restrict__ dst) {  // after a barrier; leaves bh zeroed
    flush_counts16<U16>(bh, kp.n_buckets, dst, tile_over + t, blockDim.x);
  };
  const int nd = (int)kp.n_supers;
  const int64_t t0 = t * kTileRows;
  const int64_t t1 = t0 + kTileRows < kp.n ? t0 + kTileRows : kp.n;
  const int mid_bits = kp.bucket_bits + kp.super_bits;
  const uint64_t mid_mask = (1ULL << mid_bits) - 1;
  auto load = [&](int64_t c0, int64_t (&u)[kL1Items], int64_t (&k)[kL1Items]) {
#pragma unroll
    for (int q = 0; q < kL1Items; q += 2) {
      const int64_t i = c0 + 2 * ((int64_t)threadIdx.x + (int64_t)(q / 2) * blockDim.x);
      if (kp.keys_vec && i + 1 < t1) {
        const longlong2 a = *reinterpret_cast<const longlong2*>(pid + i);
        const longlong2 c = *reinterpret_cast<const longlong2*>(pk + i);
        u[q] = a.x;
        u[q + 1] = a.y;
        k[q] = c.x;
        k[q + 1] = c.y;
      } else {
        u[q] = i < t1 ? pid[i] : 0;
        k[q] = i < t1 ? pk[i] : 0;
        u[q + 1] = i + 1 < t1 ? pid[i + 1] : 0;
        k[q + 1] = i + 1 < t1 ? pk[i + 1] : 0;
      }
    }
  };
  int64_t u[kL1Items], k[kL1Items];
  // U16: the tile's counts in two halves (counts_tm, counts_tm2)
  const bool split = U16 && t1 - t0 > (kStagesPerTile / 2 - 1) * kL1Rows;
  if (t0 < t1) load(t0, u, k);
  for (int64_t c0 = t0; c0 < t1; c0 += kL1Rows) {
    const int64_t st = c0 / kL1Rows;  // global stage index
    int d[kL1Items];
    K x[kL1Items];
    unsigned r[kL1Items];
#pragma unroll
    for (int q = 0; q < kL1Items; ++q) {
      const int64_t i = c0 + 2 * ((int64_t)threadIdx.x + (int64_t)(q / 2) * blockDim.x) + (q & 1);
      r[q] = (unsigned)i;
      d[q] = -1;
      x[q] = 0;
      if (i >= t1) continue;
      if (u[q] < 0 || u[q] >= kp.U) {  // invalid privacy id: flagged, not counted
        atomicOr(err, 1u);
        continue;
      }
      const int64_t bkt = u[q] >> kp.bucket_bits;
      if constexpr (U16) atomicAdd(bh + (bkt >> 1), 1u << (16 * (bkt & 1)));
      else atomicAdd(bh + bkt, 1u);
      d[q] = (int)(u[q] >> mid_bits);
      bool is_dead = false;
      if (k[q] < 0 || k[q] >= kp.P) {
        atomicOr(err, 1u);
        is_dead = true;
      } else if (allowed != nullptr && allowed[k[q]] == 0) {
        is_dead = true;
      }
      if constexpr (FMT == PDP_KEYS_COMPACT) {
        x[q] = (K)compact_key(kp, u[q], k[q], is_dead);
      } else if constexpr (kPackedL1<FMT>) {
        x[q] = (K)packed_key(kp, u[q], k[q], (uint32_t)(i - t0), is_dead);
      } else {
        const uint64_t midv = ((uint64_t)u[q] & mid_mask) << kp.pk_bits;
        x[q] = (K)(is_dead ? ((1ULL << 63) | midv) : (midv | (uint64_t)k[q]));
      }
    }
    unsigned rank[kL1Items];
    stage_count(s, nd, d, rank);
#pragma unroll
    for (int q = 0; q < kL1Items; ++q) {
      if (d[q] < 0) continue;
      const unsigned slot = s.start[d[q]] + rank[q];
      s.keys[slot] = x[q];
      if (ROWS) s.rows[slot] = r[q];
    }
    __syncthreads();
    const unsigned total = s.start[nd - 1] + s.hist[nd - 1];
    copy_block(keys1 + st * kL1Rows, s.keys, total);
    if (ROWS) copy_block(rows1 + st * kL1Rows, s.rows, total);
    for (int B = threadIdx.x; B <= nd; B += blockDim.x)
      soff[st * (nd + 1) + B] = (uint16_t)(B < nd ? s.start[B] : total);
    __syncthreads();
    if (c0 + kL1Rows < t1) load(c0 + kL1Rows, u, k);
    if (split && c0 - t0 == (kStagesPerTile / 2 - 1) * kL1Rows) {  // first half tile done
      flush(counts_tm + t * (kp.cstride / 2));
      __syncthreads();
    }
  }
  __syncthreads();
  // tile-major rows: coalesced.  Counts of a half tile never exceed 2^15
  if (split) {
    flush(counts_tm2 + t * (kp.cstride / 2));
  } else {
    flush(counts_tm + t * (kp.cstride / 2));
    if constexpr (U16)
      for (int64_t w = threadIdx.x; w < kp.cstride / 2; w += blockDim.x) counts_tm2[t * (kp.cstride / 2) + w] = 0;
  }
}

// Threshold-sieve level 1 (Plan.sieve): one 1,024-thread workgroup per
// 65,536-row tile filters the tile in chunks of kSieveChunk rows.  A row is a
// candidate when it is live (valid keys, public partition) and its pair hash
// is below kp.sieve_t32; candidates' level-1 records are appended to an LDS
// stage (wave-compacted: one LDS atomic per wave and chunk).  When the stage
// cannot take another chunk, or the tile ends, it is counting-sorted by
// super-bucket and written as one block right after the tile's previous
// blocks (keys1 + tile * kSieveTileStride + sbase[slot]) with its run
// offsets in soff[slot], as k_scatter_l1_local writes a stage;
// the tile's unused slots get empty runs.  Rows with invalid keys set the
// error word; dead rows (non-public partitions) are simply dropped.  The
// tile's candidate counts per bucket feed the level-2 cursors as before.
__device__ __forceinline__ void wave_lds_fence() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

#ifdef PDP_PHASE_CLOCK
__device__ unsigned g_phase_l1, g_phase_l2, g_phase_bk;  // profiling builds: prints so far per kernel
#endif
// BAND: rows with sieve_t32 <= pair hash < band_t32 also go, as (privacy id
// << 32 | row), to this tile's band list band[t * 65,536 ...], through a
// per-wave LDS queue flushed 64 entries (512 contiguous bytes) at a time;
// band_cnt[t] = the list's length
template <int FMT, bool U16, bool BAND, int TH>
__global__ void __launch_bounds__(TH, TH == kL1Threads ? 1 : 4) k_sieve_l1(KP kp, const int64_t* __restrict__ pid,
                                                         const int64_t* __restrict__ pk,
                                                         const uint8_t* __restrict__ allowed,
                                                         unsigned* __restrict__ counts_tm,
                                                         unsigned* __restrict__ counts_tm2,
                                                         uint16_t* __restrict__ soff, unsigned* __restrict__ sbase,
                                                         L1Key<FMT>* __restrict__ keys1,
                                                         unsigned* __restrict__ rows1, unsigned* err,
                                                         unsigned long long* __restrict__ band,
                                                         unsigned* __restrict__ band_cnt,
                                                         unsigned* __restrict__ tile_over) {
  using K = L1Key<FMT>;
  using SS = SieveShape<TH>;
  constexpr bool ROWS = !kPackedL1<FMT>;
  constexpr int Q = kSieveChunkItems;
  constexpr int kSieveChunk = SS::kChunk;
  constexpr int kSieveCap = SS::kCap;
  extern __shared__ unsigned long long stage_raw[];
  using SL = StageLds<K, kSmallDest, ROWS, kSieveItems, TH>;
  SL& s = *reinterpret_cast<SL*>(stage_raw);
  unsigned* bh = reinterpret_cast<unsigned*>(stage_raw + (sizeof(SL) + 7) / 8);
  // BAND: the per-wave queues after the bucket counts (l1_hist_bytes)
  unsigned long long* const bq =
      stage_raw + (sizeof(SL) + 7) / 8 + (((U16 ? 2 : 4) * kp.n_buckets + 15) / 16 * 16) / 8;
  __shared__ unsigned fill, bfill;
  const int64_t n_words = U16 ? (kp.n_buckets + 1) / 2 : kp.n_buckets;
  for (int64_t b = threadIdx.x; b < n_words; b += TH) bh[b] = 0;
  for (int B = threadIdx.x; B < (int)kp.n_supers; B += TH) s.hist[B] = 0;
  if (threadIdx.x == 0) {
    fill = 0;
    bfill = 0;
  }
  __syncthreads();
  // persistent: workgroup g takes tiles g, g + G, ... (G = gridDim.x, about
  // one per CU), so a tile's last chunks prefetch the next tile's first ones
  // and no tile starts with its loads' latency exposed
  const int nd = (int)kp.n_supers;
  int64_t t = 0, t0 = 0, t1 = 0, next_t0 = -1;  // the tile; the next one's first row (-1: none)
  auto flush_counts = [&](unsigned* __restrict__ dst) {  // after a barrier; leaves bh zeroed
    flush_counts16<U16>(bh, kp.n_buckets, dst, tile_over + t, TH);
  };
  const int mid_bits = kp.bucket_bits + kp.super_bits;
  const uint32_t t32 = kp.sieve_t32;
  const int lane = threadIdx.x & 63;
  const unsigned long long below = (1ULL << lane) - 1;
  K* blk = nullptr;
  unsigned* rblk = nullptr;
  unsigned long long* band_tile = nullptr;
  unsigned long long* const wq = bq + (threadIdx.x >> 6) * kBandQueue;
  int qn = 0;            // wave-uniform: entries waiting in this wave's band queue
  unsigned written = 0;  // block-uniform: this tile's records already written
  int slot = 0;
  bool split = false;    // U16: the tile's counts in two halves (counts_tm, counts_tm2)
  auto begin_tile = [&](int64_t tt) {
    t = tt;
    t0 = tt * kTileRows;
    t1 = t0 + kTileRows < kp.n ? t0 + kTileRows : kp.n;
    blk = keys1 + tt * kSieveTileStride;
    rblk = ROWS ? rows1 + tt * kSieveTileStride : nullptr;
    band_tile = BAND ? band + tt * kBandTileStride : nullptr;
    written = 0;
    slot = 0;
    split = U16 && t1 - t0 > kTileRows / 2 - kSieveChunk;
  };
  // the stage's `total` records -> counting sort by super-bucket -> block
#ifdef PDP_PHASE_CLOCK
  unsigned long long fl_ticks = 0, t_start = wall_clock64();
#endif
  auto flush = [&](unsigned total) {
#ifdef PDP_PHASE_CLOCK
    const unsigned long long f0 = wall_clock64();
#endif
    // the stage's runs per super-bucket were counted as its records were
    // appended (s.hist; the tile's bucket counts too), so the flush is a
    // one-wave scan and one pass that places each record through an LDS
    // cursor per run: little work while the CU's loads are stalled
    if (threadIdx.x < 64) {
      unsigned carry = 0;
      for (int base = 0; base < nd; base += 64) {
        const unsigned v = base + lane < nd ? s.hist[base + lane] : 0;
        unsigned incl = v;
        for (int off = 1; off < 64; off <<= 1) {
          const unsigned up = __shfl_up(incl, off, 64);
          if (lane >= off) incl += up;
        }
        if (base + lane < nd) {
          s.start[base + lane] = written + carry + incl - v;
          s.gcur[base + lane] = carry + incl - v;  // stage-relative cursor
        }
        carry += __shfl(incl, 63, 64);
      }
    }
    __syncthreads();
    for (int B = threadIdx.x; B < nd; B += TH) s.hist[B] = 0;  // the next stage's counts (not read below)
    // every record straight to its run: the block (<= kSieveCap records) is
    // written whole by this workgroup, so its partial lines merge in L2
#pragma unroll
    for (int j = 0; j < kSieveItems; ++j) {
      const unsigned e = threadIdx.x + (unsigned)j * TH;
      if (e >= total) continue;
      const unsigned pos = written + atomicAdd(s.gcur + s.dest[e], 1u);
      blk[pos] = s.keys[e];
      if (ROWS) rblk[pos] = s.rows[e];
    }
    const int64_t sl = t * SS::kSlots + slot;
    for (int B = threadIdx.x; B <= nd; B += TH)
      soff[sl * (nd + 1) + B] = (uint16_t)(B < nd ? s.start[B] - written : total);
    if (threadIdx.x == 0) {
      sbase[sl] = written;
      fill = 0;
    }
    written += total;
    ++slot;
    __syncthreads();
#ifdef PDP_PHASE_CLOCK
    fl_ticks += wall_clock64() - f0;
#endif
  };
  bool bad = false;  // a key outside [0, U) x [0, P): flagged once per thread at the end
  // end of a tile: the band queues' rest and the list length, the unused
  // flush slots, the bucket counts; leaves the LDS state zeroed for the next
  auto end_tile = [&]() {
    if constexpr (BAND) {
      wave_lds_fence();
      if (qn > 0) {
        unsigned bb = 0;
        if (lane == 0) bb = atomicAdd(&bfill, (unsigned)qn);
        bb = __shfl(bb, 0, 64);
        if (lane < qn) band_tile[bb + lane] = wq[lane];
        qn = 0;
      }
      __syncthreads();
      if (threadIdx.x == 0) {
        band_cnt[t] = bfill;
        bfill = 0;
      }
    }
#ifdef PDP_PHASE_CLOCK
    if (threadIdx.x == 0 && blockIdx.x % 97 == 5 && atomicAdd(&g_phase_l1, 1u) < 40u)
      printf("l1 tile %d slots %d records %u total %llu flush %llu (10 ns)\n", (int)t, slot, written,
             wall_clock64() - t_start, fl_ticks);
    t_start = wall_clock64();
    fl_ticks = 0;
#endif
    for (int j = slot; j < SS::kSlots; ++j) {
      const int64_t sl = t * SS::kSlots + j;
      for (int B = threadIdx.x; B <= nd; B += TH) soff[sl * (nd + 1) + B] = 0;
      if (threadIdx.x == 0) sbase[sl] = written;
    }
    __syncthreads();
    if (split) {
      flush_counts(counts_tm2 + t * (kp.cstride / 2));
    } else {
      flush_counts(counts_tm + t * (kp.cstride / 2));
      if constexpr (U16)
        for (int64_t w = threadIdx.x; w < kp.cstride / 2; w += TH) counts_tm2[t * (kp.cstride / 2) + w] = 0;
    }
    __syncthreads();
  };
  // FULL (a whole tile of 16-byte aligned columns): every load is an
  // unconditional 16-byte load and the prefetch address is clamped into the
  // tile, so no branch surrounds a load and the compiler keeps two chunks of
  // loads in flight (a guarded load per row made it wait for every load);
  // otherwise guarded 8-byte loads (the last tile, unaligned columns)
  auto run = [&](auto full_tag) {
    constexpr bool FULL = decltype(full_tag)::value;
    auto load = [&](int64_t c0, int64_t (&u)[Q], int64_t (&k)[Q]) {
#pragma unroll
      for (int q = 0; q < Q; q += 2) {
        const int64_t i = c0 + 2 * ((int64_t)threadIdx.x + (int64_t)(q / 2) * TH);
        if constexpr (FULL) {
          const longlong2 a = ld_nt(reinterpret_cast<const longlong2*>(pid + i));
          const longlong2 c = ld_nt(reinterpret_cast<const longlong2*>(pk + i));
          u[q] = a.x;
          u[q + 1] = a.y;
          k[q] = c.x;
          k[q + 1] = c.y;
        } else {
          u[q] = i < t1 ? pid[i] : 0;
          k[q] = i < t1 ? pk[i] : 0;
          u[q + 1] = i + 1 < t1 ? pid[i + 1] : 0;
          k[q + 1] = i + 1 < t1 ? pk[i + 1] : 0;
        }
      }
    };
    // one chunk: its keys narrowed to 32 bits and range-checked (sieve plans
    // have U < 2^32 - 1 and P < 2^32), which frees the load registers, so the
    // loads of the chunk two ahead go out before the hashing; then filter,
    // append / flush -- two chunks of loads in flight almost all the time
    auto body = [&](int64_t c0, int64_t (&u)[Q], int64_t (&k)[Q]) {
      const bool more = c0 + kSieveChunk < t1;  // block-uniform
      bool cand[Q], bnd[Q], ok[Q];
      uint32_t ul[Q], kl[Q];
#pragma unroll
      for (int q = 0; q < Q; ++q) {
        const int64_t i = c0 + 2 * ((int64_t)threadIdx.x + (int64_t)(q / 2) * TH) + (q & 1);
        const bool valid = FULL || i < t1;
        const bool in_range = (uint64_t)u[q] < (uint64_t)kp.U && (uint64_t)k[q] < (uint64_t)kp.P;
        bad |= valid & !in_range;
        ok[q] = valid & in_range;
        ul[q] = (uint32_t)u[q];
        kl[q] = (uint32_t)k[q];
      }
      if (allowed != nullptr) {  // block-uniform; the mask bytes gathered and used before the prefetch
        uint8_t pub[Q];          // (one in-order vmcnt: a later use would wait for the prefetch too)
#pragma unroll
        for (int q = 0; q < Q; ++q) pub[q] = allowed[ok[q] ? kl[q] : 0u];
#pragma unroll
        for (int q = 0; q < Q; ++q) ok[q] = ok[q] & (pub[q] != 0);  // a non-public partition's rows are dropped
      }
      // two buffers: the next loads go out now; three or more: after the
      // append / flush below, so that a flush runs with the other buffers'
      // loads in flight and this one's registers free (the register peak)
      constexpr bool kEarly = !FULL || kSieveBufs < 3;
      auto prefetch = [&]() {
        if constexpr (FULL) {  // past the tile: the next tile's chunk, else clamped (no branch)
          const int64_t ahead = c0 + kSieveBufs * kSieveChunk;
          const int64_t cp = ahead < t1 ? ahead : (next_t0 >= 0 ? next_t0 + (ahead - t1) : t1 - kSieveChunk);
          load(cp, u, k);
        } else {
          if (c0 + 2 * kSieveChunk < t1) load(c0 + 2 * kSieveChunk, u, k);
        }
      };
      if constexpr (kEarly) prefetch();
      int d[Q];
      K x[Q];
      const uint32_t mid_mask = (uint32_t)(((uint64_t)1 << mid_bits) - 1);
      const uint32_t row0 = (uint32_t)(c0 - t0) + 2u * threadIdx.x;
#pragma unroll
      for (int q = 0; q < Q; ++q) {
        // every term evaluated (no short circuit: no branch); the pair hash
        // of an id below 2^32 (pid_hash's high word is zero)
        const uint32_t h = pair_hash_from((ul[q] ^ (uint32_t)kp.seed) * 0x9E3779B1U, kp.seed, (int64_t)kl[q]);
        bnd[q] = BAND && (ok[q] & (h >= t32) & (h < kp.band_t32));
        cand[q] = ok[q] & (h < t32);
        d[q] = mid_bits < 32 ? (int)(ul[q] >> mid_bits) : 0;
        const uint32_t mid = ul[q] & mid_mask;
        if constexpr (FMT == PDP_KEYS_COMPACT) {
          x[q] = (K)((mid << kp.pk_bits) | kl[q]);
        } else {  // PACKED / PACKED_WIDE: (row within the tile | mid | partition)
          const uint32_t tile_row = row0 + (uint32_t)((q / 2) * 2 * TH) + (uint32_t)(q & 1);
          x[q] = (K)(((uint64_t)tile_row << kPackedRowShift) | ((uint64_t)mid << kp.pk_bits) | (uint64_t)kl[q]);
        }
        // a band row is no candidate: its key slot carries its privacy id
        if constexpr (BAND) x[q] = bnd[q] ? (K)ul[q] : x[q];
      }
      // append this wave's candidates at one reserved range of the stage
      unsigned long long m[Q];
      unsigned nw = 0;
#pragma unroll
      for (int q = 0; q < Q; ++q) {
        m[q] = __ballot(cand[q]);
        nw += (unsigned)__popcll(m[q]);
      }
      unsigned base = 0;
      if (lane == 0 && nw) base = atomicAdd(&fill, nw);
      base = __shfl(base, 0, 64);
#pragma unroll
      for (int q = 0; q < Q; ++q) {
        if (cand[q]) {
          const unsigned pos = base + (unsigned)__popcll(m[q] & below);
          s.keys[pos] = x[q];
          s.dest[pos] = (typename SL::D)d[q];
          if (ROWS) s.rows[pos] = (unsigned)(c0 + 2 * ((int64_t)threadIdx.x + (int64_t)(q / 2) * TH) + (q & 1));
          // the stage's run lengths and the tile's bucket counts (bucket = id >> bucket_bits)
          atomicAdd(s.hist + d[q], 1u);
          const unsigned bkt = ul[q] >> kp.bucket_bits;
          if constexpr (U16) atomicAdd(bh + (bkt >> 1), 1u << (16 * (bkt & 1)));
          else atomicAdd(bh + bkt, 1u);
        }
        base += (unsigned)__popcll(m[q]);
      }
      if constexpr (BAND) {  // band rows -> the wave's queue; 64 of them out at once
#pragma unroll
        for (int q = 0; q < Q; ++q) {
          const unsigned long long mb = __ballot(bnd[q]);
          if (mb == 0) continue;  // wave-uniform
          const int64_t i = c0 + 2 * ((int64_t)threadIdx.x + (int64_t)(q / 2) * TH) + (q & 1);
          if (bnd[q]) wq[qn + __popcll(mb & below)] = ((unsigned long long)(uint32_t)x[q] << 32) | (uint32_t)i;
          qn += __popcll(mb);
          if (qn >= 64) {
            wave_lds_fence();
            const unsigned long long e = wq[lane];
            unsigned bb = 0;
            if (lane == 0) bb = atomicAdd(&bfill, 64u);
            bb = __shfl(bb, 0, 64);
            band_tile[bb + lane] = e;
            const unsigned long long rest = lane + 64 < qn ? wq[lane + 64] : 0ULL;
            wave_lds_fence();
            if (lane + 64 < qn) wq[lane] = rest;
            qn -= 64;
            wave_lds_fence();
          }
        }
      }
      __syncthreads();
      const unsigned f = fill;
      if (f > 0 && (f > (unsigned)(kSieveCap - kSieveChunk) || !more)) flush(f);  // block-uniform
      else __syncthreads();  // every thread has read `fill` before the next chunk's appends
      if constexpr (!kEarly) prefetch();
      if (split && c0 - t0 == kTileRows / 2 - kSieveChunk) {  // first half tile counted
        flush_counts(counts_tm + t * (kp.cstride / 2));
        __syncthreads();
      }
    };
    if constexpr (FULL) {  // a fixed trip count: the same loads are pending on every path
      constexpr int kChunks = (int)(kTileRows / kSieveChunk);
      // the ring of kSieveBufs register buffers turns a whole number of times
      // per tile, so the chunks prefetched across the tile boundary land in
      // the buffers the next tile reads them from
      static_assert(kChunks % kSieveBufs == 0, "whole ring turns per tile");
      int64_t ub[kSieveBufs][Q], kb[kSieveBufs][Q];
      const int64_t n_full = kp.n / kTileRows;  // tiles of kTileRows rows (16-byte aligned columns)
      // (workgroup g takes tiles g, g + G, ...: contiguous tile ranges per
      // workgroup measured 5 % slower, profiles/r05/ab/ab1_l1_placement.txt)
      const int64_t tile_lo = blockIdx.x, tile_hi = n_full, tile_step = gridDim.x;
      if (tile_lo >= tile_hi) return;  // block-uniform
#pragma unroll
      for (int b = 0; b < kSieveBufs; ++b) load(tile_lo * kTileRows + (int64_t)b * kSieveChunk, ub[b], kb[b]);
      for (int64_t tt = tile_lo; tt < tile_hi; tt += tile_step) {
        begin_tile(tt);
        next_t0 = tt + tile_step < tile_hi ? (tt + tile_step) * kTileRows : -1;
        for (int j = 0; j < kChunks; j += kSieveBufs) {
#pragma unroll
          for (int b = 0; b < kSieveBufs; ++b) body(t0 + (int64_t)(j + b) * kSieveChunk, ub[b], kb[b]);
        }
        end_tile();
      }
    } else {  // the last tile, unaligned columns: two chunks in flight
      int64_t ua[Q], ka[Q], ub[Q], kb[Q];
      if (t0 < t1) load(t0, ua, ka);
      if (t0 + kSieveChunk < t1) load(t0 + kSieveChunk, ub, kb);
      for (int64_t c0 = t0; c0 < t1; c0 += 2 * kSieveChunk) {
        body(c0, ua, ka);
        if (c0 + kSieveChunk < t1) body(c0 + kSieveChunk, ub, kb);  // block-uniform
      }
    }
  };
  if (kp.keys_vec) run(std::true_type{});
  // the rest: a partial last tile, or every tile when the columns are unaligned
  for (int64_t tt = (kp.keys_vec ? kp.n / kTileRows : 0) + blockIdx.x; tt < kp.n_tiles; tt += gridDim.x) {
    begin_tile(tt);
    next_t0 = -1;
    run(std::false_type{});
    end_tile();
  }
  if (bad) atomicOr(err, 1u);
}

// Level 2 over tile-local level-1 blocks: workgroup (group g of kL2GroupTiles
// tiles, super-bucket B) takes B's run from each of the group's stages
// (kL2Runs runs: keys1[st * kL1Rows + soff[st][B], + soff[st][B + 1])),
// concatenated in stage order, kL2Rows records per LDS window.  Per window an
// LDS map (the run of every record, in the stage's destination-tag array
// before the counting sort reuses it) lets each thread address its own
// records, so all of a thread's loads go out together.  Cursors as in
// k_scatter_l2; PACKED rows are (stage >> slot_bits) * 65,536 + tile row.
// level-2 key of a packed level-1 record w (bit 63 dead): COMPACT u32
// (bit 31 dead | local pid | partition) or, PACKED_WIDE, the same fields in a u64
template <typename KO>
__device__ __forceinline__ KO unpacked_key(const KP& kp, uint32_t local, uint64_t w) {
  if constexpr (sizeof(KO) == 4) {
    const uint32_t lpk = local << kp.pk_bits;
    return (KO)((w >> 63) ? (0x80000000u | lpk) : (lpk | (uint32_t)(w & kp.pk_mask)));
  } else {
    const uint64_t lpk = (uint64_t)local << kp.pk_bits;
    return (KO)((w >> 63) ? ((1ULL << 63) | lpk) : (lpk | (w & kp.pk_mask)));
  }
}

// tile-local level 2 records per thread: half for 8-byte level-2 keys with a
// row array (WIDE / PACKED_WIDE), so their LDS windows and registers leave
// room for two workgroups per CU; PACKED64 carries no row array
template <int FMT>
constexpr int l2_items() { return sizeof(L2Key<FMT>) == 8 && FMT != PDP_KEYS_PACKED64 ? kL2Items / 2 : kL2Items; }
template <int FMT>
constexpr bool kL2RowArray = FMT != PDP_KEYS_PACKED64;  // level 2 writes a row array

template <int FMT, int MAXD>
__global__ void __launch_bounds__(kL2Threads, 4) k_scatter_l2_local(KP kp, const uint16_t* __restrict__ soff,
                                                                   const unsigned* __restrict__ sbase,
                                                                   const unsigned* __restrict__ bucket_start,
                                                                   const unsigned* __restrict__ gcur,
                                                                   const L1Key<FMT>* __restrict__ keys1,
                                                                   const unsigned* __restrict__ rows1,
                                                                   L2Key<FMT>* __restrict__ keys2,
                                                                   unsigned* __restrict__ rows2) {
  using KI = L1Key<FMT>;
  using KO = L2Key<FMT>;
  constexpr int NI = l2_items<FMT>();  // records per thread and window
  constexpr int NR = kL2Threads * NI;
  constexpr bool PACKED = kPackedL1<FMT>;  // PACKED / PACKED_WIDE level-1 records
  constexpr bool ROWS1 = !PACKED;
  extern __shared__ unsigned long long stage_raw[];
  using SL = StageLds<KO, MAXD, kL2RowArray<FMT>, NI, kL2Threads>;
  using D = typename SL::D;
  SL& s = *reinterpret_cast<SL*>(stage_raw);
#ifdef PDP_PHASE_CLOCK
  unsigned long long c0 = wall_clock64(), c_tab = 0, c_ld = 0, c_sort = 0, c_wr = 0, cw = 0;
  int n_win = 0;
#endif
  // the workgroup's non-empty runs, in slot order
  // (a run's tile is rsrc / kTileRows: every level-1 block of tile t starts at
  // or after t * kTileRows, inside its tile's region -- and keeping the LDS of
  // a PACKED workgroup at <= 80 KiB lets two of them share a CU)
  __shared__ unsigned rbeg[kL2Threads + 1];  // start of each run in the concatenation
  __shared__ unsigned rsrc[kL2Threads];      // its first record in keys1
  __shared__ unsigned wsum[kL2Threads / 64 + 1], wsum2[kL2Threads / 64 + 1];
  // XCD-aware order: a group's workgroups (all super-buckets) run one after
  // another on one XCD (blocks are placed round-robin, linear id % 8), so the
  // cache lines that two neighbouring runs of a stage block share are read
  // from that XCD's L2
  // a workgroup takes kp.l2_group_mult tile groups (up to 4 with the sieve, whose
  // blocks hold a fraction of the rows; <= kL2Threads slots, one per thread)
  const int nd = (int)kp.n_supers;
  const int M = kp.l2_group_mult;
  const int64_t n_grp = (kp.n_tiles + (int64_t)kL2GroupTiles * M - 1) / ((int64_t)kL2GroupTiles * M);
  const int64_t lin = blockIdx.x, kx = lin >> 3;
  const int64_t g = (kx / nd) * 8 + (lin & 7);
  const int B = (int)(kx % nd);
  if (g >= n_grp) return;  // block-uniform
  const int64_t runs = ((int64_t)kL2GroupTiles << kp.slot_bits) * M;  // level-1 slots of the workgroup
  const int64_t S0 = g * runs;
  const int64_t n_all = kp.n_slots1 - S0 < runs ? kp.n_slots1 - S0 : runs;
  // this workgroup's bucket write cursors: loaded first, so that their
  // latency overlaps the run table's loads below (thread t < 2^super_bits)
  const int nsub = 1 << kp.super_bits;
  const int64_t s_first = (int64_t)B << kp.super_bits;
  unsigned cur0 = 0;
  if ((int)threadIdx.x < nsub && s_first + threadIdx.x < kp.n_buckets)
    cur0 = bucket_start[s_first + threadIdx.x] + gcur[g * M * kp.n_buckets + s_first + threadIdx.x];
  unsigned len = 0, src = 0;
  if ((int64_t)threadIdx.x < n_all) {
    // block sl starts at sl * kL1Rows, or (sieve, sbase != NULL) at its
    // tile's region + sbase[sl]
    const int64_t sl = S0 + threadIdx.x;
    const uint16_t* o = soff + sl * (nd + 1) + B;
    len = (unsigned)o[1] - (unsigned)o[0];
    src = (sbase != nullptr ? (unsigned)((sl >> kp.slot_bits) * kSieveTileStride) + sbase[sl]
                            : (unsigned)(sl * kL1Rows)) + o[0];
  }
  unsigned total, nnz;
  const unsigned ex = block_excl_scan(len, wsum, &total);
  const unsigned idx = block_excl_scan(len > 0 ? 1u : 0u, wsum2, &nnz);
  if (len > 0) {
    rbeg[idx] = ex;
    rsrc[idx] = src;
  }
  if (threadIdx.x == 0) rbeg[nnz] = total;
  const int nr = (int)nnz;
  if ((int)threadIdx.x < nsub) s.gcur[threadIdx.x] = cur0;
  for (int t = threadIdx.x + blockDim.x; t < nsub; t += blockDim.x) {
    const int64_t b = s_first + t;
    s.gcur[t] = b < kp.n_buckets ? bucket_start[b] + gcur[g * M * kp.n_buckets + b] : 0u;
  }
  __syncthreads();
  if (total == 0) return;  // block-uniform
#ifdef PDP_PHASE_CLOCK
  c_tab = wall_clock64() - c0;
#endif
  const int bb = kp.bucket_bits;
  const uint32_t local_mask = (1u << bb) - 1;
  const int sub_shift = kp.pk_bits + kp.bucket_bits;
  const uint64_t sub_mask = (uint64_t)nsub - 1;
  const int lane = threadIdx.x & 63, nw = blockDim.x >> 6;
  int j0 = 0;  // first run overlapping the window (block-uniform)
  for (unsigned base = 0, wend = 0; base < total; base = wend) {
    while (rbeg[j0 + 1] <= base) ++j0;
    wend = base + NR < total ? base + NR : total;
    // at most 256 runs per window (u8 run tags): a cap only tiny runs reach
    if (j0 + 256 < nr && rbeg[j0 + 256] < wend) wend = rbeg[j0 + 256];
    for (int j = j0 + (int)(threadIdx.x >> 6); j < nr && rbeg[j] < wend; j += nw) {
      const unsigned a = rbeg[j] > base ? rbeg[j] : base;
      const unsigned e = rbeg[j + 1] < wend ? rbeg[j + 1] : wend;
      for (unsigned v = a + lane; v < e; v += 64) s.dest[v - base] = (D)(j - j0);
    }
    __syncthreads();
    // records in two halves of loads in flight (register budget of two
    // workgroups per CU), unpacked into the counting sort's items
    KO x[NI];
    unsigned r[NI];
    int d[NI];
    constexpr int H = NI / 2;  // (all NI in one round spills 21-33 VGPRs: level 2 +37 %, profiles/r05/ab/ab9)
#pragma unroll
    for (int h = 0; h < NI; h += H) {
      KI raw[H];
      unsigned rr[H];  // PACKED: the record's tile's first row; else its row
      bool live[H];
#pragma unroll
      for (int q = 0; q < H; ++q) {
        const unsigned v = base + threadIdx.x + (unsigned)(h + q) * blockDim.x;
        live[q] = v < wend;
        if constexpr (ROWS1) {
          // key and row loads unconditional (a dead slot reads record 0), so
          // all H pairs go out together: under the branch each pair waited
          // for the previous one (COMPACT / WIDE)
          const int j = j0 + (int)s.dest[live[q] ? v - base : 0u];
          const unsigned i = live[q] ? rsrc[j] + (v - rbeg[j]) : 0u;
          raw[q] = keys1[i];
          rr[q] = rows1[i];
        } else if (live[q]) {
          const int j = j0 + (int)s.dest[v - base];
          const unsigned i = rsrc[j] + (v - rbeg[j]);
          raw[q] = keys1[i];
          rr[q] = rsrc[j] & ~(unsigned)(kTileRows - 1);  // first row of the run's tile
        }
      }
#pragma unroll
      for (int q = 0; q < H; ++q) {
        d[h + q] = -1;
        x[h + q] = 0;
        r[h + q] = 0;
        if (!live[q]) continue;
        if constexpr (PACKED) {
          const uint64_t v = raw[q];
          const uint32_t mid = (uint32_t)((v >> kp.pk_bits) & ((1ULL << (bb + kp.super_bits)) - 1));
          d[h + q] = (int)(mid >> bb);
          r[h + q] = rr[q] + (uint32_t)((v >> kPackedRowShift) & (kTileRows - 1));
          if constexpr (FMT == PDP_KEYS_PACKED64)  // (row | local pid | partition), all ones if dead
            x[h + q] = (KO)((v >> 63) ? ~0ULL
                                      : (((uint64_t)r[h + q] << kp.row_shift) |
                                         ((uint64_t)(mid & local_mask) << kp.pk_bits) | (v & kp.pk_mask)));
          else
            x[h + q] = unpacked_key<KO>(kp, mid & local_mask, v);
        } else {
          x[h + q] = (KO)raw[q];
          r[h + q] = rr[q];
          d[h + q] = (int)((raw[q] >> sub_shift) & sub_mask);
        }
      }
    }
    __syncthreads();  // the destination tags are rewritten by the counting sort
#ifdef PDP_PHASE_CLOCK
    const unsigned long long ca = wall_clock64();
#endif
    unsigned rank[NI];
    stage_count(s, nsub, d, rank);
#ifdef PDP_PHASE_CLOCK
    const unsigned long long cb = wall_clock64();
#endif
    stage_write(s, nsub, d, rank, x, r, keys2, rows2);
    for (int t = threadIdx.x; t < nsub; t += blockDim.x) s.gcur[t] += s.hist[t];
    __syncthreads();
#ifdef PDP_PHASE_CLOCK
    const unsigned long long cc = wall_clock64();
    c_ld += ca - (cw ? cw : c0 + c_tab);
    c_sort += cb - ca;
    c_wr += cc - cb;
    cw = cc;
    ++n_win;
#endif
  }
#ifdef PDP_PHASE_CLOCK
  if (threadIdx.x == 0 && blockIdx.x % 4001 == 77 && atomicAdd(&g_phase_l2, 1u) < 40u)
    printf("l2 wg %d runs %d records %u windows %d table %llu load %llu sort %llu write %llu total %llu (10 ns)\n",
           (int)blockIdx.x, nr, total, n_win, c_tab, c_ld, c_sort, c_wr, wall_clock64() - c0);
#endif
}

// Per-wave LDS queue of candidate rows (capacity 2 waves' worth): rows that
// pass a cheap per-row test are compacted here and the expensive per-candidate
// work then runs on full wavefronts instead of on the few lanes of each
// load that happen to hold a candidate.
struct WaveQueue {
  unsigned long long* key;  // [kQueueCap]
  unsigned* row;            // [kQueueCap]
};

// Streams the rows [begin, end) of one bucket: conv(record) gives the row's
// pair key, pred(key) selects candidates, work(key, row) handles each
// candidate on compacted wavefronts.  R = 16 / sizeof(K) rows per lane per
// 16-byte key load (and 4·R-byte row load when ROWS), KU loads in flight per
// lane; every wave runs the same trip count so the queue stays convergent.
// RM: what a candidate carries beside its key -- kRowNone, kRowLoad (rows[i],
// a 16-byte load per R records beside the keys) or kRowIndex (the record's
// position i in `keys`, for candidate lists).
// kRowFromKey: the row is the record's bits from row_shift up (PACKED64).
constexpr int kRowNone = 0, kRowLoad = 1, kRowIndex = 2, kRowFromKey = 3;
template <int KU, int RM, typename K, typename CV, typename P, typename W>
__device__ __forceinline__ void stream_bucket(const K* __restrict__ keys, const unsigned* __restrict__ rows,
                                              int64_t begin, int64_t end, WaveQueue q, CV&& conv, P&& pred,
                                              W&& work, int row_shift = 0) {
  constexpr bool ROWS = RM != kRowNone;
  constexpr bool LOADR = RM == kRowLoad;
  constexpr int R = 16 / sizeof(K);
  using KV = typename std::conditional<R == 4, uint4, ulonglong2>::type;
  using RV = typename std::conditional<R == 4, uint4, uint2>::type;
  const int lane = threadIdx.x & 63;
  const unsigned long long below = (1ULL << lane) - 1;
  int n = 0;  // wave-uniform queue length
  auto push_p = [&](uint64_t x, uint32_t r, bool p) {
    const unsigned long long m = __ballot(p);
    if (p) {
      const int pos = n + __popcll(m & below);
      q.key[pos] = x;
      if (ROWS) q.row[pos] = r;
    }
    n += __popcll(m);
    if (n >= 64) {
      wave_lds_fence();
      const uint64_t wx = q.key[lane];
      const uint32_t wr = ROWS ? q.row[lane] : 0u;
      n -= 64;
      uint64_t mx = 0;
      uint32_t mr = 0;
      if (lane < n) {
        mx = q.key[64 + lane];
        if (ROWS) mr = q.row[64 + lane];
      }
      wave_lds_fence();
      if (lane < n) {
        q.key[lane] = mx;
        if (ROWS) q.row[lane] = mr;
      }
      work(wx, wr);
    }
  };
  auto push = [&](uint64_t x, uint32_t r) { push_p(x, r, pred(x)); };
  int64_t a0 = (begin + R - 1) & ~(int64_t)(R - 1);
  if (a0 > end) a0 = end;
  const int64_t a1 = a0 + ((end - a0) & ~(int64_t)(R - 1));
  {  // unaligned head rows [begin, a0) on lanes 0..R-2, tail rows [a1, end) on lanes R..2R-2 of wave 0
    uint64_t x = kEmpty;
    uint32_t r = 0;
    const int t = threadIdx.x;
    if (t < R - 1 && begin + t < a0) {
      x = conv(keys[begin + t]);
      if (LOADR) r = rows[begin + t];
      if (RM == kRowIndex) r = (uint32_t)(begin + t);
      if (RM == kRowFromKey) r = (uint32_t)((uint64_t)keys[begin + t] >> row_shift);
    }
    if (t >= R && t < 2 * R - 1 && a1 + (t - R) < end) {
      x = conv(keys[a1 + (t - R)]);
      if (LOADR) r = rows[a1 + (t - R)];
      if (RM == kRowIndex) r = (uint32_t)(a1 + (t - R));
      if (RM == kRowFromKey) r = (uint32_t)((uint64_t)keys[a1 + (t - R)] >> row_shift);
    }
    push(x, r);
  }
  const int64_t np = (a1 - a0) / R;
  const KV* kv = reinterpret_cast<const KV*>(keys + a0);
  const RV* rv = reinterpret_cast<const RV*>(rows + a0);
  const int64_t step = (int64_t)blockDim.x * KU;
  auto load = [&](int64_t g0, KV (&kx)[KU], RV (&rx)[KU]) {
#pragma unroll
    for (int u = 0; u < KU; ++u) {
      const int64_t g = g0 + (int64_t)u * blockDim.x + threadIdx.x;
      if (g < np) {
        kx[u] = kv[g];
        if (LOADR) rx[u] = rv[g];
      } else {
        if constexpr (R == 4) kx[u] = make_uint4(~0u, ~0u, ~0u, ~0u);  // dead records
        else kx[u] = make_ulonglong2(kEmpty, kEmpty);
      }
    }
  };
  KV kx[KU];
  RV rx[KU];
  if (np > 0) load(0, kx, rx);
  for (int64_t g0 = 0; g0 < np; g0 += step) {
    // the row carried by component e of this lane's load u
    auto rowv = [&](int u, int e) -> uint32_t {
      if constexpr (RM == kRowIndex) {
        return (uint32_t)(a0 + (g0 + (int64_t)u * blockDim.x + threadIdx.x) * R + e);
      } else if constexpr (RM == kRowLoad) {
        if constexpr (R == 4) return e == 0 ? rx[u].x : (e == 1 ? rx[u].y : (e == 2 ? rx[u].z : rx[u].w));
        else return e == 0 ? rx[u].x : rx[u].y;
      } else if constexpr (RM == kRowFromKey) {
        static_assert(R == 2, "row-in-key records are 8 bytes");
        return (uint32_t)((uint64_t)(e == 0 ? kx[u].x : kx[u].y) >> row_shift);
      } else {
        return 0u;
      }
    };
    // software pipeline: the next batch's loads are in flight while this
    // batch runs through the queue (LDS work only, no vector memory)
    KV nk[KU];
    RV nr[KU];
    const bool more = g0 + step < np;  // block-uniform
    if (more) load(g0 + step, nk, nr);
#pragma unroll
    for (int u = 0; u < KU; ++u) {
      if constexpr (R == 4) {
        push(conv(kx[u].x), rowv(u, 0));
        push(conv(kx[u].y), rowv(u, 1));
        push(conv(kx[u].z), rowv(u, 2));
        push(conv(kx[u].w), rowv(u, 3));
      } else {
        push(conv(kx[u].x), rowv(u, 0));
        push(conv(kx[u].y), rowv(u, 1));
      }
    }
    if (more) {
#pragma unroll
      for (int u = 0; u < KU; ++u) {
        kx[u] = nk[u];
        if (LOADR) rx[u] = nr[u];
      }
    }
  }
  if (n > 0) {  // partial wave
    wave_lds_fence();
    if (lane < n) work((uint64_t)q.key[lane], ROWS ? q.row[lane] : 0u);
  }
}

// blockIdx -> work index with each XCD (blockIdx % 8) owning one contiguous
// block: XCD x gets q + (x < rem) indices starting at x * q + min(x, rem).
// A bijection on [0, G) for any G; a speed hint only.
__device__ __forceinline__ int64_t xcd_major(int64_t id, int64_t G) {
  const int64_t q = G >> 3, rem = G & 7, x = id & 7, j = id >> 3;
  return x * q + (x < rem ? x : rem) + j;
}


// PDP_PHASE_CLOCK (profiling builds only, tools/build_variants.sh): thread 0
// of a few buckets prints the wall-clock time (10 ns ticks) of each phase of
// k_bucket_bound; results are unchanged (the r02 ablation builds that skipped
// phases left the merge reading unwritten records)
#ifdef PDP_PHASE_CLOCK
#define PDP_PHASE(k)                             \
  do {                                           \
    __syncthreads();                             \
    if (threadIdx.x == 0) ph[k] = wall_clock64(); \
  } while (0)
#else
#define PDP_PHASE(k) \
  do {               \
  } while (0)
#endif

// FLAT: the per-id fix-up's listed launch (ids over its row cap): blist holds
// {bucket, begin, end, id}, only that id is marked, and the kept pairs go to
// the flat list instead of the bucket's record block and runs
// Static LDS of k_bucket_bound (everything else is its dynamic block).
struct BucketStatic {
  unsigned ccount;  // B1's candidate count
};
static_assert(sizeof(BucketStatic) <= (size_t)kBucketStaticLds, "make_plan counts kBucketStaticLds bytes of static LDS");

template <int VALUE_KIND, bool KEEP_ALL_ROWS, bool RANGES, int REC, bool FLAT = false>
__global__ void __launch_bounds__(kBucketThreads) k_bucket_bound(KP kp, const RecKey<REC == kRecCompact>* __restrict__ keys,
                                                                 const unsigned* __restrict__ rowidx,
                                                                 const unsigned* __restrict__ offsets,
                                                                 const void* __restrict__ value,
                                                                 pdp_partition_accumulators acc, PairRecords rec,
                                                                 RecKey<REC == kRecCompact>* __restrict__ cand_key,
                                                                 unsigned* __restrict__ cand_idx,
                                                                 unsigned* __restrict__ unres_bits,
                                                                 unsigned* __restrict__ unres_list,
                                                                 unsigned* __restrict__ sctl, unsigned* __restrict__ err,
                                                                 unsigned long long* __restrict__ fix_rec,
                                                                 const unsigned* __restrict__ unres_prev,
                                                                 const unsigned* __restrict__ blist,
                                                                 unsigned* __restrict__ id_pos,
                                                                 unsigned* __restrict__ id_seg) {
  constexpr bool COMPACT = REC == kRecCompact;
  extern __shared__ unsigned long long smem[];
  // the kernel's only static LDS, kept in one struct so that the plan's
  // allowance for it (kBucketStaticLds, make_plan) is checked where it is declared
  __shared__ BucketStatic bstat;
  unsigned& ccount = bstat.ccount;
  const int64_t S = (int64_t)1 << kp.bucket_bits;
  const int l0 = kp.l0;
  // b: the bucket; [begin, end): its records; only_id >= 0 (per-id fix-up,
  // an id over the row cap): the records are that one id's, and only it is marked
  auto body = [&](const int64_t b, const int64_t begin, const int64_t end, const int64_t only_id) {
#ifdef PDP_PHASE_CLOCK
  unsigned long long ph[6] = {0, 0, 0, 0, 0, 0};
  if (threadIdx.x == 0) ph[0] = wall_clock64();
#endif
  // threshold sieve: a privacy id of this bucket with fewer than l0
  // candidate pairs (its sketch not full; `sketch` = false: every id) may
  // have kept pairs among rows this launch did not see; mark it in the
  // bitmap (a wave covers 64 ids = one u64 word; the bucket's ids are whole
  // words) and list it.  unres_prev (the band's fix-up launch): only ids the
  // main launch left unresolved can be.
  // per-id fix-up (id_pos != NULL): a listed id's list position goes to
  // id_pos[id] and its fix-up row count (id_seg, odd words) starts at 0
  auto mark = [&](bool sketch) {
    const int lane = threadIdx.x & 63;
    const int64_t id0 = b << kp.bucket_bits;
    if constexpr (FLAT) {  // the bitmap was zeroed, other ids' bits are k_fix_ids'
      if (threadIdx.x == 0 && smem[(int64_t)(l0 - 1) * S + (only_id - id0)] == kEmpty) {
        atomicOr(unres_bits + (only_id >> 5), 1u << (only_id & 31));
        const unsigned at = atomicAdd(sctl, 1u);
        unres_list[at] = (unsigned)only_id;
        id_pos[only_id] = at;
        id_seg[2 * (int64_t)at + 1] = 0;
      }
      return;
    }
    for (int64_t p0 = (int64_t)(threadIdx.x >> 6) * 64; p0 < S; p0 += blockDim.x) {
      const int64_t id = id0 + p0 + lane;
      bool un = id < kp.U;
      if (sketch) un = un && smem[(int64_t)(l0 - 1) * S + p0 + lane] == kEmpty;  // sk is smem's first array
      if (unres_prev != nullptr) un = un && ((unres_prev[id >> 5] >> (id & 31)) & 1u);
      const unsigned long long m = __ballot(un);
      if (lane == 0) reinterpret_cast<uint2*>(unres_bits)[(id0 + p0) >> 6] = make_uint2((unsigned)m, (unsigned)(m >> 32));
      if (m) {
        unsigned base = 0;
        if (lane == 0) base = atomicAdd(sctl, (unsigned)__popcll(m));
        base = __shfl(base, 0, 64);
        if (un) {
          const unsigned at = base + __popcll(m & ((1ULL << lane) - 1));
          unres_list[at] = (unsigned)id;
          if (id_pos != nullptr) {
            id_pos[id] = at;
            id_seg[2 * (int64_t)at + 1] = 0;
          }
        }
      }
    }
  };
  // an empty bucket of a fix-up launch (most of them: only unresolved
  // privacy ids have rows there) writes its empty runs and stops -- in the
  // band's fix-up launch after marking its previously unresolved ids (none
  // of their pairs is below t2); the main launch's empty buckets still mark
  // their privacy ids unresolved
  if ((!kp.sieve_mark || unres_prev != nullptr) && begin == end) {  // block-uniform
    if (RANGES) {
      for (int t = threadIdx.x; t <= kp.n_ranges; t += blockDim.x) rec.runs[t * rec.run_stride + b] = 0;
    }
    if (kp.sieve_mark) mark(false);
    return;
  }
  const int64_t n_slots = S * l0;
  // LDS state is structure-of-arrays: entry j of privacy id p at [j * S + p]
  // (row-sketch entry t of slot s at [t * S*l0 + s]), so a wave's lanes, which
  // touch random privacy ids, spread over the LDS banks
  unsigned long long* sk = smem;                      // [l0][S] pair sketch per pid
  unsigned long long* rsk = sk + n_slots;             // bounded: [linf][S*l0] row sketches
  double* tot = (double*)(sk + n_slots);              // keep-all: [3][S*l0] pair sums
  unsigned* cnt = KEEP_ALL_ROWS ? (unsigned*)(tot + 3 * n_slots) : (unsigned*)(rsk + n_slots * kp.linf);
  unsigned* rh = cnt + n_slots;          // RANGES: [n_ranges] kept pairs per partition range
  unsigned* rcur = rh + kp.n_ranges;     //         [n_ranges] write cursors
  unsigned* wsum = rcur + kp.n_ranges;   //         block-scan scratch
  const int n_waves = (int)(blockDim.x >> 6);  // 16 or 8 (Plan.bucket_threads)
  unsigned* tail = RANGES ? wsum + n_waves + 1 : rh;
  // derived from smem by offset (not through an integer round trip) so the
  // compiler keeps the LDS address space and emits ds_* rather than flat_*
  unsigned long long* qbase = smem + (((const char*)tail - (const char*)smem) + 7) / 8;
  const int wave = threadIdx.x >> 6;
  const WaveQueue wq{qbase + wave * kQueueCap,
                     (unsigned*)(qbase + n_waves * kQueueCap) + wave * kQueueCap};
  // per privacy id of the bucket, after the queues: {pid_hash (expand_key),
  // high half of its sketch maximum (b1_candidate)}
  uint2* hpid = (uint2*)((unsigned*)(qbase + n_waves * kQueueCap) + n_waves * kQueueCap);
  for (int64_t t = threadIdx.x; t < S; t += blockDim.x)
    hpid[t] = make_uint2(pid_hash(kp.seed, (b << kp.bucket_bits) | t), 0xFFFFFFFFu);
  for (int64_t t = threadIdx.x; t < n_slots; t += blockDim.x) {
    sk[t] = kEmpty;
    cnt[t] = 0;
  }
  if (RANGES)
    for (int t = threadIdx.x; t < kp.n_ranges; t += blockDim.x) rh[t] = 0;
  if (!KEEP_ALL_ROWS) {
    for (int64_t t = threadIdx.x; t < n_slots * kp.linf; t += blockDim.x) rsk[t] = kEmpty;
  } else {
    for (int64_t t = threadIdx.x; t < 3 * n_slots; t += blockDim.x) tot[t] = 0.0;
  }
  __syncthreads();
  const uint64_t bmask = (uint64_t)S - 1;
  // PACKED64 records (row | local pid | partition; all ones dead) and their
  // candidate-list form (local pid | partition)
  auto expand64 = [&](unsigned long long v) -> uint64_t {
    if (v == ~0ULL) return kEmpty;
    const uint64_t local = (v >> kp.pk_bits) & ((1ULL << kp.bucket_bits) - 1);
    return pair_key_from(hpid[local].x, kp.seed, (int64_t)(v & kp.pk_mask), local << kp.pk_bits, kp.rand_shift);
  };
  auto conv = [&](RecKey<COMPACT> v) -> uint64_t {
    if constexpr (REC == kRecP64) return expand64(v);
    else return expand_key(kp, hpid, v);
  };
  // B1: bottom-l0 distinct pair keys per privacy id; candidates are keys at or
  // below their sketch's current maximum.  A pair kept in the end entered the
  // sketch at its first row and never left it (the maximum only decreases),
  // so every one of its rows is a candidate here: the candidates still in
  // their sketch after the insert are appended to a per-bucket list
  // (record-local key + row) and B2 reads only that list.
  if (threadIdx.x == 0) ccount = 0;
  __syncthreads();
  PDP_PHASE(1);
  const uint64_t lbits = ((uint64_t)1 << (kp.pk_bits + kp.bucket_bits)) - 1;  // local pid | partition
  // (each record's row index rides along, loaded with its key: B2 then needs
  // no dependent gather of it)
  stream_bucket<COMPACT ? 4 : kUnroll, REC == kRecP64 ? kRowFromKey : kRowLoad>(
      keys, rowidx, begin, end, wq,
      // the candidate test rides on the pid-hash read (b1_candidate)
      [&](RecKey<COMPACT> v) -> uint64_t {
        if constexpr (REC == kRecP64) {
          const uint64_t x = expand64(v);
          if (x == kEmpty) return kEmpty;
          return (uint32_t)(x >> 32) <= hpid[(v >> kp.pk_bits) & ((1ULL << kp.bucket_bits) - 1)].y ? x : kEmpty;
        } else {
          return b1_candidate(kp, hpid, v);
        }
      },
      [&](uint64_t x) { return x != kEmpty; },
      [&](uint64_t x, uint32_t i)  {  // i: the record's row
        const int64_t pl = (int64_t)((x >> kp.pk_bits) & bmask);
        unsigned long long* s = sk + pl;
        if (x < s[(l0 - 1) * S]) sketch_insert_strided(s, l0, S, x);
        const unsigned long long smax = s[(l0 - 1) * S];
        // a maximum read after this insert: never below the current one
        hpid[pl].y = (uint32_t)(smax >> 32);
        const bool keep = x <= smax;
        const unsigned long long active = __ballot(true);
        const unsigned long long m = __ballot(keep);
        const int leader = __ffsll((long long)active) - 1;
        unsigned base = 0;
        if ((int)(threadIdx.x & 63) == leader && m) base = atomicAdd(&ccount, (unsigned)__popcll(m));
        base = __shfl(base, leader, 64);
        if (keep) {
          const int64_t o = begin + base + __popcll(m & ((1ULL << (threadIdx.x & 63)) - 1));
          cand_key[o] = (RecKey<COMPACT>)(x & lbits);
          cand_idx[o] = i;
        }
      },
      kp.row_shift);
  __syncthreads();
  if (kp.sieve_mark) mark(true);  // emits nothing for its unresolved ids (B2 skips them): the fix-up's
  PDP_PHASE(2);
  // B2: rows of kept pairs, from B1's candidate list (key + row)
  const int flags = kp.clip.flags;
  stream_bucket<COMPACT ? 1 : kUnroll / 2, kRowLoad>(
      cand_key, cand_idx, begin, begin + ccount, wq, conv,
      [&](uint64_t x) {
        // (dead keys: also the padding lanes' kEmpty, whose bits name no pid)
        if (dead_key(x, kp.rand_shift)) return false;
        const unsigned long long smax = sk[(l0 - 1) * S + (int64_t)((x >> kp.pk_bits) & bmask)];
        // band: an unresolved id's candidate rows (every one of its records
        // is on the list; the sieve dropped the dead ones) go to the fix-up
        if (kp.sieve_emit && smax == kEmpty) return true;
        return x <= smax && !(kp.sieve_mark && smax == kEmpty);  // sieve: unresolved ids are the fix-up's
      },
      [&](uint64_t x, uint32_t ci)  {
      const int64_t pl = (x >> kp.pk_bits) & bmask;
      if (kp.sieve_emit) {  // block-uniform: the main launch with the band
        const bool un = sk[(l0 - 1) * S + pl] == kEmpty && ci < (uint64_t)kp.n;
        const unsigned long long mu = __ballot(un);
        if (mu) {  // wave-uniform
          const int lead = __ffsll((long long)mu) - 1;
          const int lane = threadIdx.x & 63;
          unsigned base = 0;
          if (lane == lead) base = atomicAdd(sctl + 1, (unsigned)__popcll(mu));
          base = __shfl(base, lead, 64);
          const int64_t at = (int64_t)base + __popcll(mu & ((1ULL << lane) - 1));
          if (un && at < kp.fix_cap)
            fix_rec[at] = ((unsigned long long)(uint32_t)((b << kp.bucket_bits) | pl) << 32) | (unsigned long long)ci;
        }
        if (sk[(l0 - 1) * S + pl] == kEmpty) return;
      }
      const int j = sketch_find_strided(sk + pl, l0, S, x);
      if (j < 0) return;
      const uint32_t r = ci;  // the candidate's row (B1 carried it)
      if (r >= (uint64_t)kp.n) {  // malformed record: flagged, never dereferenced
        atomicOr(err, 1u);
        return;
      }
      const int64_t slot = j * S + pl;  // entry j of pid pl (structure of arrays)
      atomicAdd(cnt + slot, 1u);
      if (!KEEP_ALL_ROWS) {
        const uint64_t y = row_key(kp.row_seed, kp.row_offset + r, r);
        unsigned long long* rs = rsk + slot;
        if (y < rs[(kp.linf - 1) * n_slots]) sketch_insert_strided(rs, kp.linf, n_slots, y);
      } else if (VALUE_KIND != PDP_VALUE_NONE) {
        double v;
        long long iv;
        load_value<VALUE_KIND>(value, r, &v, &iv);
        if (flags & PDP_SUM_PER_PARTITION) {
          if (flags & PDP_SUM_INT) atomicAdd((unsigned long long*)(tot + slot), (unsigned long long)iv);
          else atomicAdd(tot + slot, v);
        } else if (flags & PDP_ACC_SUM) {
          if (flags & PDP_SUM_INT)
            atomicAdd((unsigned long long*)(tot + slot),
                      (unsigned long long)clamp_ll(iv, (long long)kp.clip.lo, (long long)kp.clip.hi));
          else atomicAdd(tot + slot, clip_f64(v, kp.clip.lo, kp.clip.hi));
        }
        if (flags & (PDP_ACC_NSUM | PDP_ACC_NSUM2)) {
          const double c = clip_f64(v, kp.clip.lo, kp.clip.hi) - kp.clip.mid;
          if (flags & PDP_ACC_NSUM) atomicAdd(tot + n_slots + slot, c);
          if (flags & PDP_ACC_NSUM2) atomicAdd(tot + 2 * n_slots + slot, c * c);
        }
      }
  });
  __syncthreads();
  PDP_PHASE(3);
  // B2.5: the kept rows' values replace their row keys in the row sketches
  // (B3 then reads LDS only; same rows, same order, so the sums are
  // unchanged), all of a thread's gathers in flight together.  The first
  // batch (entries 0 and 1 of the thread's first G slots: all of them at C3,
  // C2 and C4) is issued before B3a's LDS histogram, scan and run-table
  // stores, which then run under the gathers' latency
  constexpr int G = 4;
  constexpr int T0 = 2;  // row-sketch entries of the pre-issued batch (C2 / C4: Linf = 2)
  constexpr bool B25 = !KEEP_ALL_ROWS && VALUE_KIND != PDP_VALUE_NONE;
  long long bits0[T0][G];
  bool live0[T0][G];
  if constexpr (B25) {
    uint32_t rr[T0][G];
#pragma unroll
    for (int t = 0; t < T0; ++t)
#pragma unroll
      for (int u = 0; u < G; ++u) {
        const int64_t slot = (int64_t)threadIdx.x + (int64_t)u * blockDim.x;
        live0[t][u] = t < kp.linf && slot < n_slots && sk[slot] != kEmpty && (unsigned)t < cnt[slot];
        rr[t][u] = live0[t][u] ? (uint32_t)rsk[t * n_slots + slot] : 0u;
      }
#pragma unroll
    for (int t = 0; t < T0; ++t)
#pragma unroll
      for (int u = 0; u < G; ++u) bits0[t][u] = live0[t][u] ? ((const long long*)value)[rr[t][u]] : 0;
  }
  PDP_PHASE(4);
  const void* const b3_value = B25 ? nullptr : value;
  if (RANGES && !FLAT) {
    // B3a: kept pairs per partition range -> this bucket's run starts
    for (int64_t slot = threadIdx.x; slot < n_slots; slot += blockDim.x) {
      const uint64_t x = sk[slot];
      if (x == kEmpty || cnt[slot] == 0 || (int64_t)(x & kp.pk_mask) >= kp.P) continue;
      atomicAdd(rh + ((x & kp.pk_mask) >> kp.range_bits), 1u);
    }
    __syncthreads();
    const unsigned h = threadIdx.x < kp.n_ranges ? rh[threadIdx.x] : 0u;  // n_ranges <= blockDim
    unsigned total;
    const unsigned ex = block_excl_scan(h, wsum, &total);
    if (threadIdx.x < kp.n_ranges) {
      rec.runs[threadIdx.x * rec.run_stride + b] = ex;
      rcur[threadIdx.x] = ex;
    }
    if (threadIdx.x == 0) rec.runs[kp.n_ranges * rec.run_stride + b] = total;
    __syncthreads();
  }
  if constexpr (B25) {
#pragma unroll
    for (int t = 0; t < T0; ++t)
#pragma unroll
      for (int u = 0; u < G; ++u)
        if (live0[t][u]) rsk[t * n_slots + (int64_t)threadIdx.x + (int64_t)u * blockDim.x] = (unsigned long long)bits0[t][u];
    // the rest (more slots than G per thread, or Linf > T0), G at a time
    for (int t = 0; t < kp.linf; ++t) {
      for (int64_t s0 = threadIdx.x + (t < T0 ? (int64_t)G * blockDim.x : 0); s0 < n_slots;
           s0 += (int64_t)G * blockDim.x) {
        uint32_t rr[G];
        bool live[G];
#pragma unroll
        for (int u = 0; u < G; ++u) {
          const int64_t slot = s0 + (int64_t)u * blockDim.x;
          live[u] = slot < n_slots && sk[slot] != kEmpty && (unsigned)t < cnt[slot];
          rr[u] = live[u] ? (uint32_t)rsk[t * n_slots + slot] : 0u;
        }
        long long bits[G];
#pragma unroll
        for (int u = 0; u < G; ++u)
          bits[u] = live[u] ? ((const long long*)value)[rr[u]] : 0;
#pragma unroll
        for (int u = 0; u < G; ++u)
          if (live[u]) rsk[t * n_slots + s0 + (int64_t)u * blockDim.x] = (unsigned long long)bits[u];
      }
    }
    __syncthreads();
  }
  // B3: merge every kept pair into its partition (RANGES: emit a pair record)
  for (int64_t slot = threadIdx.x; slot < n_slots; slot += blockDim.x) {
    const uint64_t x = sk[slot];
    if (x == kEmpty) continue;
    const int64_t p = (int64_t)(x & kp.pk_mask);
    const unsigned c = cnt[slot];
    if (c == 0) continue;
    if (p >= kp.P) {  // malformed record (pk_mask spans up to 2^pk_bits > P): flagged, skipped
      atomicOr(err, 1u);
      continue;
    }
    PairSums ps;
    if (!KEEP_ALL_ROWS) {
      const long long m = c < (unsigned)kp.linf ? (long long)c : (long long)kp.linf;
      ps = pair_sums_from_rows<VALUE_KIND>(rsk + slot, m, b3_value, kp.clip, n_slots);
    } else if (VALUE_KIND != PDP_VALUE_NONE) {
      ps = pair_sums_from_totals((long long)c, tot[slot], tot[n_slots + slot], tot[2 * n_slots + slot], kp.clip);
    } else {
      ps = PairSums{(long long)c, 0, 0.0, 0.0, 0.0};
    }
    if (RANGES) {
      // (per-id fix-up: the flat list of the fix-up's pairs, no runs)
      int64_t i;
      if constexpr (FLAT) {
        i = rec.flat_base + (int64_t)atomicAdd(rec.flat_n, 1u);
        if (i >= rec.flat_base + rec.flat_cap) continue;  // cannot happen: <= l0 pairs per id
      } else {
        i = b * n_slots + atomicAdd(rcur + (p >> kp.range_bits), 1u);
      }
      rec.key[i] = ((unsigned long long)p << 32) | (unsigned long long)(uint32_t)ps.count;
      if (flags & (PDP_ACC_SUM | PDP_SUM_PER_PARTITION))
        rec.f0[i] = (flags & PDP_SUM_INT) ? __longlong_as_double(ps.isum) : ps.fsum;
      if (flags & PDP_ACC_NSUM) rec.f1[i] = ps.nsum;
      if (flags & PDP_ACC_NSUM2) rec.f2[i] = ps.nsum2;
    } else {
      add_pair_to_partition(acc, p, ps, flags);
    }
  }
#ifdef PDP_PHASE_CLOCK
  PDP_PHASE(5);
  if (threadIdx.x == 0 && blockIdx.x % 997 == 11 && atomicAdd(&g_phase_bk, 1u) < 40u)
    printf("phase bucket %d records %u cand %u init %llu b1 %llu b2 %llu b25 %llu b3 %llu (10 ns)\n", (int)b,
           (unsigned)(end - begin), ccount, ph[1] - ph[0], ph[2] - ph[1], ph[3] - ph[2], ph[4] - ph[3],
           ph[5] - ph[4]);
#endif
  };
  if constexpr (FLAT) {
    // the per-id fix-up's ids over the row cap (k_fix_ids listed them): each
    // entry is one id's rows, a slice of the id-ordered fix-up records
    const unsigned nb = blist[0];
    for (unsigned i = blockIdx.x; i < nb; i += gridDim.x) {
      const unsigned* e = blist + 1 + 4 * (int64_t)i;
      body((int64_t)e[0], (int64_t)e[1], (int64_t)e[2], (int64_t)e[3]);
      __syncthreads();
    }
  } else if (blist == nullptr) {
    // XCD-aware bucket order: workgroups are dispatched round-robin over the
    // 8 XCDs (blockIdx % 8), so XCD x takes one contiguous block of buckets
    // and its writes to the range-major run table (and the records) share L2
    // lines
    const int64_t b = xcd_major(blockIdx.x, gridDim.x);
    body(b, offsets[b], offsets[b + 1], -1);  // offsets has n_buckets + 1 entries
  } else {
    // a fix-up launch over the buckets that hold fix-up rows only (blist[0]
    // of them, listed from blist[1]; k_fix_buckets did the empty ones'
    // work): a persistent loop, one bucket at a time
    const unsigned nb = blist[0];
    for (unsigned i = blockIdx.x; i < nb; i += gridDim.x) {
      const int64_t b = (int64_t)blist[1 + i];
      body(b, offsets[b], offsets[b + 1], -1);
      __syncthreads();  // the LDS state is the next bucket's
    }
  }
}

// ------------------------------------------------ threshold-sieve fix-up --
// Bloom filter of the unresolved privacy ids (k_sieve_rescan): one
// multiplicative hash per id, its top 12 bits the LDS word, two bit
// positions from its low 10 bits (one full-rate-cheap test per row: the
// rescan streams 8 B per row and must stay memory-bound)
constexpr int kBloomBits = 12;
static_assert(kBloomWords == 1 << kBloomBits, "Bloom filter size");
__device__ __forceinline__ uint32_t bloom_hash(uint32_t id) { return id * 0x9E3779B1u; }
__device__ __forceinline__ unsigned bloom_word(uint32_t h) { return h >> (32 - kBloomBits); }
__device__ __forceinline__ unsigned bloom_bits(uint32_t h) { return (1u << (h & 31)) | (1u << ((h >> 5) & 31)); }

// Fix-up step 1: the rows that may belong to an unresolved privacy id.  One
// streaming read of the privacy-id column (8 B per row); a row is tested
// against an LDS Bloom filter of the unresolved list (one word, two bits;
// each workgroup builds its own), and the positives -- with the filter's
// false positives, ~1e-3 of the rows -- are appended to fix_rec as
// (privacy id << 32 | row).  The test touches LDS only, and positives wait in
// a per-wave LDS queue that goes out 64 entries at a time, so the stream's
// loads (the next iteration's in flight while this one is tested) are never
// drained by a dependent global access.  k_fix_filter then keeps the exact
// ones.  Without the filter (more than kBloomMaxIds unresolved ids) every
// in-range row is tested against the bitmap here.  No unresolved id: no work.
constexpr int kRescanQueue = 128;  // per-wave queue: < 64 waiting + one batch of <= 64
template <bool BLOOM>
__device__ __forceinline__ bool rescan_maybe(const KP& kp, int64_t u, const unsigned* bloom,
                                             const unsigned* __restrict__ unres_bits) {
  if constexpr (BLOOM) {  // LDS only, no short circuit: the reads of a batch go out together
    const uint32_t h = bloom_hash((uint32_t)u);
    const unsigned bits = bloom_bits(h);
    return ((uint64_t)u < (uint64_t)kp.U) & ((bloom[bloom_word(h)] & bits) == bits);
  } else {
    return (uint64_t)u < (uint64_t)kp.U && ((unres_bits[u >> 5] >> (u & 31)) & 1u);  // invalid ids: flagged by level 1
  }
}

template <bool VEC>
__global__ void __launch_bounds__(kRescanThreads) k_sieve_rescan(KP kp, const int64_t* __restrict__ pid,
                                                                 const unsigned* __restrict__ unres_bits,
                                                                 const unsigned* __restrict__ unres_list,
                                                                 unsigned* __restrict__ sctl,
                                                                 unsigned long long* __restrict__ fix_rec) {
  __shared__ unsigned bloom[kBloomWords];
  __shared__ unsigned long long queue[kRescanThreads / 64][kRescanQueue];
  const unsigned n_unres = sctl[0];
  if (n_unres == 0) return;  // grid-uniform
  const bool use_bloom = n_unres <= kBloomMaxIds;  // grid-uniform
  for (int i = threadIdx.x; i < kBloomWords; i += blockDim.x) bloom[i] = 0;
  __syncthreads();
  for (unsigned i = threadIdx.x; use_bloom && i < n_unres; i += blockDim.x) {
    const uint32_t h = bloom_hash(unres_list[i]);
    atomicOr(bloom + bloom_word(h), bloom_bits(h));
  }
  __syncthreads();
  const int lane = threadIdx.x & 63;
  const unsigned long long below = (1ULL << lane) - 1;
  unsigned long long* const wq = queue[threadIdx.x >> 6];
  int qn = 0;  // wave-uniform queue length
  // the wave's positives (`pos` on the active lanes) into its queue; 64 out
  auto enqueue = [&](bool pos, int64_t u, int64_t i) {
    const unsigned long long m = __ballot(pos);
    if (m == 0) return;  // wave-uniform
    if (pos) wq[qn + __popcll(m & below)] = ((unsigned long long)u << 32) | (unsigned long long)(uint32_t)i;
    qn += __popcll(m);
    if (qn >= 64) {
      wave_lds_fence();
      const unsigned long long e = wq[lane];
      unsigned base = 0;
      if (lane == 0) base = atomicAdd(sctl + 1, 64u);
      base = __shfl(base, 0, 64);
      if (base + lane < kp.fix_cap) fix_rec[base + lane] = e;
      const unsigned long long rest = lane + 64 < qn ? wq[lane + 64] : 0ULL;
      wave_lds_fence();
      if (lane + 64 < qn) wq[lane] = rest;
      qn -= 64;
      wave_lds_fence();
    }
  };
  constexpr int KU = 8;  // 16-byte loads (two rows) per lane and iteration
  const int64_t per_iter = (int64_t)blockDim.x * KU;  // row pairs per block iteration
  const int64_t n_iters = VEC ? (kp.n / 2) / per_iter : 0;
  const longlong2* __restrict__ pv = reinterpret_cast<const longlong2*>(pid);
  auto run = [&](auto bloom_tag) {
    constexpr bool BLOOM = decltype(bloom_tag)::value;
    int64_t it = blockIdx.x;
    if (it < n_iters) {
      longlong2 cur[KU], nxt[KU];
#pragma unroll
      for (int v = 0; v < KU; ++v) cur[v] = pv[it * per_iter + (int64_t)v * blockDim.x + threadIdx.x];
      for (; it < n_iters; it += gridDim.x) {  // block-uniform trips
        const int64_t nx = it + gridDim.x < n_iters ? it + gridDim.x : it;  // in range: no branch around the loads
#pragma unroll
        for (int v = 0; v < KU; ++v) nxt[v] = pv[nx * per_iter + (int64_t)v * blockDim.x + threadIdx.x];
        unsigned maybe = 0;
#pragma unroll
        for (int v = 0; v < KU; ++v) {
          maybe |= (unsigned)rescan_maybe<BLOOM>(kp, cur[v].x, bloom, unres_bits) << (2 * v);
          maybe |= (unsigned)rescan_maybe<BLOOM>(kp, cur[v].y, bloom, unres_bits) << (2 * v + 1);
        }
        if (__ballot(maybe != 0) != 0) {  // wave-uniform, ~1 in 2 wave iterations at C3
#pragma unroll
          for (int v = 0; v < KU; ++v) {
            const int64_t i = 2 * (it * per_iter + (int64_t)v * blockDim.x + threadIdx.x);
            enqueue((maybe >> (2 * v)) & 1u, cur[v].x, i);
            enqueue((maybe >> (2 * v + 1)) & 1u, cur[v].y, i + 1);
          }
        }
#pragma unroll
        for (int v = 0; v < KU; ++v) cur[v] = nxt[v];
      }
    }
    // the rows no full iteration covered (all of them without VEC): every lane
    // of a wave runs the same trip count, so the queue stays wave-uniform
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    const int64_t i0 = 2 * n_iters * per_iter + (int64_t)blockIdx.x * blockDim.x;
    for (int64_t w0 = i0 + (int64_t)(threadIdx.x & ~63); w0 < kp.n; w0 += stride) {  // w0: the wave's first row
      const int64_t i = w0 + lane;
      const int64_t u = i < kp.n ? pid[i] : -1;
      enqueue(i < kp.n && rescan_maybe<BLOOM>(kp, u, bloom, unres_bits), u, i);
    }
  };
  if (use_bloom) run(std::true_type{});
  else run(std::false_type{});
  // the rest of the queue
  wave_lds_fence();
  if (qn > 0) {
    unsigned base = 0;
    if (lane == 0) base = atomicAdd(sctl + 1, (unsigned)qn);
    base = __shfl(base, 0, 64);
    if (lane < qn && base + lane < kp.fix_cap) fix_rec[base + lane] = wq[lane];
  }
}

// Fix-up step 1, side band: the tiles' band lists (privacy id << 32 | row,
// written by k_sieve_l1<BAND>) instead of the whole privacy-id column, with
// the same Bloom filter, per-wave queues and output (fix_rec, sctl[1]) as
// k_sieve_rescan; the unresolved ids' candidate rows are already on fix_rec
// (the main bucket launch put them there).  Every lane of a wave runs the
// same trips (band_cnt[t] is block-uniform), so the queues stay wave-uniform.
__global__ void __launch_bounds__(kRescanThreads) k_band_scan(KP kp, const unsigned long long* __restrict__ band,
                                                              const unsigned* __restrict__ band_cnt,
                                                              const unsigned* __restrict__ unres_bits,
                                                              const unsigned* __restrict__ unres_list,
                                                              unsigned* __restrict__ sctl,
                                                              unsigned long long* __restrict__ fix_rec) {
  __shared__ unsigned bloom[kBloomWords];
  __shared__ unsigned long long queue[kRescanThreads / 64][kRescanQueue];
  const unsigned n_unres = sctl[0];
  if (n_unres == 0) return;  // grid-uniform
  const bool use_bloom = n_unres <= kBloomMaxIds;  // grid-uniform
  for (int i = threadIdx.x; i < kBloomWords; i += blockDim.x) bloom[i] = 0;
  __syncthreads();
  for (unsigned i = threadIdx.x; use_bloom && i < n_unres; i += blockDim.x) {
    const uint32_t h = bloom_hash(unres_list[i]);
    atomicOr(bloom + bloom_word(h), bloom_bits(h));
  }
  __syncthreads();
  const int lane = threadIdx.x & 63;
  const unsigned long long below = (1ULL << lane) - 1;
  unsigned long long* const wq = queue[threadIdx.x >> 6];
  int qn = 0;
  auto enqueue = [&](bool pos, unsigned long long e) {
    const unsigned long long m = __ballot(pos);
    if (m == 0) return;  // wave-uniform
    if (pos) wq[qn + __popcll(m & below)] = e;
    qn += __popcll(m);
    if (qn >= 64) {
      wave_lds_fence();
      const unsigned long long x = wq[lane];
      unsigned base = 0;
      if (lane == 0) base = atomicAdd(sctl + 1, 64u);
      base = __shfl(base, 0, 64);
      if (base + lane < kp.fix_cap) fix_rec[base + lane] = x;
      const unsigned long long rest = lane + 64 < qn ? wq[lane + 64] : 0ULL;
      wave_lds_fence();
      if (lane + 64 < qn) wq[lane] = rest;
      qn -= 64;
      wave_lds_fence();
    }
  };
  // entries per lane and trip, loaded together (8: at an N = 8 rank's share a
  // block sees ~2 tiles, so its trips are latency rounds, not a stream)
  constexpr int KU = 8;
  const int64_t w0 = (int64_t)(threadIdx.x >> 6) * 64 * KU;
  auto run = [&](auto bloom_tag) {
    constexpr bool BLOOM = decltype(bloom_tag)::value;
    for (int64_t t = blockIdx.x; t < kp.n_tiles; t += gridDim.x) {
      const unsigned long long* __restrict__ bt = band + t * kBandTileStride;
      unsigned cnt = band_cnt[t];
      cnt = cnt <= (unsigned)kTileRows ? cnt : (unsigned)kTileRows;
      for (int64_t j0 = w0; j0 < cnt; j0 += (int64_t)blockDim.x * KU) {  // wave-uniform trips
        unsigned long long e[KU];
#pragma unroll
        for (int v = 0; v < KU; ++v) {
          const int64_t j = j0 + v * 64 + lane;
          e[v] = j < cnt ? ld_nt(bt + j) : ~0ULL;
        }
#pragma unroll
        for (int v = 0; v < KU; ++v) {
          const int64_t u = e[v] == ~0ULL ? -1 : (int64_t)(e[v] >> 32);
          enqueue(u >= 0 && rescan_maybe<BLOOM>(kp, u, bloom, unres_bits), e[v]);
        }
      }
    }
  };
  if (use_bloom) run(std::true_type{});
  else run(std::false_type{});
  wave_lds_fence();
  if (qn > 0) {
    unsigned base = 0;
    if (lane == 0) base = atomicAdd(sctl + 1, (unsigned)qn);
    base = __shfl(base, 0, 64);
    if (lane < qn && base + lane < kp.fix_cap) fix_rec[base + lane] = wq[lane];
  }
}

// Fix-up step 1b: the exact test of every listed row (the bitmap of the
// unresolved ids); a false positive's entry becomes ~0 (skipped by
// k_fix_scatter), a true one is counted for its bucket.
__global__ void __launch_bounds__(kBlock) k_fix_filter(KP kp, const unsigned* __restrict__ unres_bits,
                                                       const unsigned* __restrict__ sctl,
                                                       unsigned long long* __restrict__ fix_rec,
                                                       unsigned* __restrict__ fix_cnt, unsigned* err,
                                                       unsigned* __restrict__ blist) {
  // a list longer than its region cannot happen (each list holds distinct
  // rows); were it to, error bit 1 says so instead of reading past the region
  const int64_t listed = sctl[1];
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    if (listed > kp.fix_cap) atomicOr(err, 2u);
    blist[0] = 0;  // k_fix_buckets' count (the previous fix-up launch is done with it)
  }
  const int64_t total = listed < kp.fix_cap ? listed : kp.fix_cap;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const uint64_t u = fix_rec[i] >> 32;
    if ((unres_bits[u >> 5] >> (u & 31)) & 1u) atomicAdd(fix_cnt + (u >> kp.bucket_bits), 1u);
    else fix_rec[i] = ~0ULL;
  }
}

// Fix-up step 2: the listed rows -> bucket order (fix_start = exclusive scan
// of the per-bucket counts; a slot per row from the bucket's cursor), as the
// bucket kernel's records: (bucket-local pid << pk_bits | partition), dead
// bit for a non-public or invalid partition, and the row.
template <int REC>
__global__ void __launch_bounds__(kBlock) k_fix_scatter(KP kp, const int64_t* __restrict__ pk,
                                                        const uint8_t* __restrict__ allowed,
                                                        const unsigned long long* __restrict__ fix_rec,
                                                        const unsigned* __restrict__ sctl,
                                                        const unsigned* __restrict__ fix_start,
                                                        unsigned* __restrict__ fix_cur,
                                                        RecKey<REC == kRecCompact>* __restrict__ keys,
                                                        unsigned* __restrict__ rows) {
  const int64_t total = (int64_t)sctl[1] < kp.fix_cap ? (int64_t)sctl[1] : kp.fix_cap;
  const uint64_t lmask = ((uint64_t)1 << kp.bucket_bits) - 1;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const uint64_t e = fix_rec[i];
    if (e == ~0ULL) continue;  // a Bloom false positive (k_fix_filter)
    const uint64_t u = e >> 32;
    const uint32_t r = (uint32_t)e;
    const int64_t k = pk[r];
    const bool dead = k < 0 || k >= kp.P || (allowed != nullptr && allowed[k] == 0);
    const uint64_t lpk = (u & lmask) << kp.pk_bits;
    const int64_t b = (int64_t)(u >> kp.bucket_bits);
    const unsigned pos = fix_start[b] + atomicAdd(fix_cur + b, 1u);
    if constexpr (REC == kRecCompact)
      keys[pos] = (uint32_t)(dead ? (0x80000000ull | lpk) : (lpk | (uint64_t)k));
    else if constexpr (REC == kRecWide)
      keys[pos] = dead ? ((1ull << 63) | lpk) : (lpk | (uint64_t)k);
    else  // PACKED64: the row in the key, all ones if dead
      keys[pos] = dead ? ~0ull : (((uint64_t)r << kp.row_shift) | lpk | (uint64_t)k);
    if constexpr (REC != kRecP64) rows[pos] = r;
  }
}

// Fix-up step 3a: the buckets a fix-up bucket launch must run.  Only buckets
// holding fix-up rows are listed (blist[1 + i], blist[0] of them): their
// count is at most the unresolved ids', a small fraction of the buckets.  An
// empty bucket's launch work is done here instead: its run-table column
// (range-major, `runs` already offset to the launch's record segment) gets
// empty runs and, in the band's fix-up (prev != NULL), the ids the main
// launch left unresolved stay unresolved -- none of their pairs lies below t2
// -- so they are copied to the second bitmap and list (what k_bucket_bound's
// mark(false) does for an empty bucket).  blist[0] is zeroed by the caller.
// Grid (buckets / kBlock, kFixRunRows): blockIdx.y = 0 lists and marks,
// every y writes its share of the run-table rows (consecutive threads:
// consecutive columns of one row)
constexpr int kFixRunRows = 16;
__global__ void __launch_bounds__(kBlock) k_fix_buckets(KP kp, const unsigned* __restrict__ fix_start,
                                                        unsigned* __restrict__ runs, int64_t run_stride,
                                                        unsigned* __restrict__ blist,
                                                        const unsigned* __restrict__ prev,
                                                        unsigned* __restrict__ bits2,
                                                        unsigned* __restrict__ list2,
                                                        unsigned* __restrict__ sctl2) {
  const int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= kp.n_buckets) return;
  const bool empty = fix_start[b + 1] == fix_start[b];
  if (runs != nullptr && empty)
    for (int r = blockIdx.y; r <= kp.n_ranges; r += gridDim.y) runs[(int64_t)r * run_stride + b] = 0;
  if (blockIdx.y != 0) return;
  if (!empty) {
    blist[1 + atomicAdd(blist, 1u)] = (unsigned)b;
    return;
  }
  if (prev == nullptr) return;
  const int64_t id0 = b << kp.bucket_bits;  // bucket_bits >= 6: whole u64 words
  for (int64_t w = 0; w < ((int64_t)1 << kp.bucket_bits) / 64; ++w) {
    const int64_t i0 = id0 + 64 * w;
    const uint2 pw = reinterpret_cast<const uint2*>(prev)[i0 >> 6];
    unsigned long long m = (unsigned long long)pw.x | ((unsigned long long)pw.y << 32);
    if (i0 + 64 > kp.U) m &= kp.U > i0 ? (1ULL << (kp.U - i0)) - 1 : 0ULL;  // ids >= U are no ids
    reinterpret_cast<uint2*>(bits2)[i0 >> 6] = make_uint2((unsigned)m, (unsigned)(m >> 32));
    if (m == 0) continue;
    unsigned at = atomicAdd(sctl2, (unsigned)__popcll(m));
    for (; m; m &= m - 1) list2[at++] = (unsigned)(i0 + __ffsll((long long)m) - 1);
  }
}

// ----------------------------------------------------- per-id fix-up --
// Plan.fix_ids: the fix-up list grouped by privacy id instead of by bucket,
// and one wave per unresolved id (k_fix_ids) instead of a bucket launch over
// every bucket.  An unresolved id is known by its position in the unresolved
// list (id_pos[id], written where the id is listed); seg[2 * pos] and
// seg[2 * pos + 1] are the start and the end of the id's rows in the
// id-ordered records (the end counts the rows first, then is the scatter's
// cursor).  Four launches per round: k_fix_id_count, k_fix_id_alloc,
// k_fix_id_scatter, k_fix_ids (+ a listed bucket launch for ids over the row
// cap, else empty).  (The scan folded into the count's last finishing block
// measured 0.03 ms per launch for its device-scope fences, against 0.007 ms
// for the launch of its own: profiles/r07.)

// Step 1: k_fix_filter's exact test, the rows counted per id.
constexpr int kFixScanItems = 8;
__global__ void __launch_bounds__(kBlock) k_fix_id_count(KP kp, const unsigned* __restrict__ unres_bits,
                                                         const unsigned* __restrict__ sctl,
                                                         unsigned long long* __restrict__ fix_rec,
                                                         const unsigned* __restrict__ id_pos, unsigned* seg,
                                                         unsigned* err, unsigned* __restrict__ blist) {
  const int64_t listed = sctl[1];
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    if (listed > kp.fix_cap) atomicOr(err, 2u);  // see k_fix_filter
    blist[0] = 0;  // k_fix_ids' count of ids over the row cap
  }
  const int64_t total = listed < kp.fix_cap ? listed : kp.fix_cap;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const uint64_t u = fix_rec[i] >> 32;
    if ((unres_bits[u >> 5] >> (u & 31)) & 1u) atomicAdd(seg + 2 * (int64_t)id_pos[u] + 1, 1u);
    else fix_rec[i] = ~0ULL;
  }
}

// Step 1b: the counts -> starts, one workgroup: an exclusive scan over the
// unresolved list, eight ids per thread and trip (a few thousand ids at C3)
__global__ void __launch_bounds__(kBlock) k_fix_id_alloc(const unsigned* __restrict__ sctl, unsigned* __restrict__ seg) {
  __shared__ unsigned wsum[kBlock / 64 + 1];
  const int64_t n_ids = sctl[0];
  unsigned carry = 0;
  for (int64_t j0 = 0; j0 < n_ids; j0 += (int64_t)kBlock * kFixScanItems) {  // block-uniform trips
    const int64_t j = j0 + (int64_t)threadIdx.x * kFixScanItems;
    unsigned c[kFixScanItems], sum = 0;
#pragma unroll
    for (int k = 0; k < kFixScanItems; ++k) {
      c[k] = j + k < n_ids ? seg[2 * (j + k) + 1] : 0u;
      sum += c[k];
    }
    unsigned t;
    unsigned at = carry + block_excl_scan(sum, wsum, &t);
#pragma unroll
    for (int k = 0; k < kFixScanItems; ++k) {
      if (j + k < n_ids) {
        seg[2 * (j + k)] = at;
        seg[2 * (j + k) + 1] = at;
      }
      at += c[k];
    }
    carry += t;
    __syncthreads();  // wsum is the next trip's
  }
}

// Step 2: k_fix_scatter into id order (the same records: bucket-local pid |
// partition, dead bit, row), a slot per row from the id's cursor.
template <int REC>
__global__ void __launch_bounds__(kBlock) k_fix_id_scatter(KP kp, const int64_t* __restrict__ pk,
                                                           const uint8_t* __restrict__ allowed,
                                                           const unsigned long long* __restrict__ fix_rec,
                                                           const unsigned* __restrict__ sctl,
                                                           const unsigned* __restrict__ id_pos,
                                                           unsigned* __restrict__ seg,
                                                           RecKey<REC == kRecCompact>* __restrict__ keys,
                                                           unsigned* __restrict__ rows) {
  const int64_t total = (int64_t)sctl[1] < kp.fix_cap ? (int64_t)sctl[1] : kp.fix_cap;
  const uint64_t lmask = ((uint64_t)1 << kp.bucket_bits) - 1;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const uint64_t e = fix_rec[i];
    if (e == ~0ULL) continue;  // a Bloom false positive (k_fix_id_count)
    const uint64_t u = e >> 32;
    const uint32_t r = (uint32_t)e;
    const int64_t k = pk[r];
    const bool dead = k < 0 || k >= kp.P || (allowed != nullptr && allowed[k] == 0);
    const uint64_t lpk = (u & lmask) << kp.pk_bits;
    const unsigned pos = atomicAdd(seg + 2 * (int64_t)id_pos[u] + 1, 1u);
    if constexpr (REC == kRecCompact)
      keys[pos] = (uint32_t)(dead ? (0x80000000ull | lpk) : (lpk | (uint64_t)k));
    else if constexpr (REC == kRecWide)
      keys[pos] = dead ? ((1ull << 63) | lpk) : (lpk | (uint64_t)k);
    else  // PACKED64: the row in the key, all ones if dead
      keys[pos] = dead ? ~0ull : (((uint64_t)r << kp.row_shift) | lpk | (uint64_t)k);
    if constexpr (REC != kRecP64) rows[pos] = r;
  }
}

// where k_fix_ids lists the ids still short of l0 pairs (the band's round)
struct IdMarks {
  unsigned* bits;  // zeroed bitmap
  unsigned* list;
  unsigned* sctl;
  unsigned* seg;   // their row counts start at 0
};

// Step 3: one wave per unresolved id (a persistent grid over the list).  The
// wave streams the id's records 64 at a time, twice, with the bucket
// kernel's steps on a sketch of its own in LDS: B1 the bottom-l0 distinct
// pair keys (the same keys: pid hash, bucket-local pid, partition); with
// kp.sieve_mark an id whose sketch is not full is listed in `mk` and emits
// nothing (the rescan's round finishes it); B2 the rows of kept pairs
// counted and their bottom-linf row keys; the kept rows' values gathered
// together (B2.5); B3 one pair record per kept pair, appended to the flat
// list that the reduce kernels add to the partitions.  An id with more than
// kFixIdsRowCap rows is listed for the bucket launch that follows:
// {bucket, begin, end, id} from blist[1] on.
template <int VALUE_KIND, int REC>
__global__ void __launch_bounds__(kFixIdsThreads) k_fix_ids(KP kp, const unsigned* __restrict__ list,
                                                            const unsigned* __restrict__ sctl,
                                                            const unsigned* __restrict__ seg,
                                                            const RecKey<REC == kRecCompact>* __restrict__ keys,
                                                            const unsigned* __restrict__ rows,
                                                            const void* __restrict__ value, PairRecords rec,
                                                            IdMarks mk, unsigned* __restrict__ id_pos,
                                                            unsigned* __restrict__ blist, unsigned* err) {
  constexpr int kWaves = kFixIdsThreads / 64;
  __shared__ unsigned long long s_sk[kWaves][kFixIdsEntries];
  __shared__ unsigned s_cnt[kWaves][kFixIdsEntries];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int l0 = kp.l0, linf = kp.linf;  // l0 * (1 + linf) <= kFixIdsEntries (the plan)
  unsigned long long* sk = s_sk[wave];   // [l0] pair sketch
  unsigned long long* rsk = sk + l0;     // [linf][l0] row sketches
  unsigned* cnt = s_cnt[wave];           // [l0] rows per kept pair
  const int flags = kp.clip.flags;
  const int64_t n_ids = sctl[0];
  const uint64_t lmask = ((uint64_t)1 << kp.bucket_bits) - 1;
  for (int64_t j = (int64_t)blockIdx.x * kWaves + wave; j < n_ids; j += (int64_t)gridDim.x * kWaves) {  // wave-uniform
    const int64_t id = list[j];
    const int64_t begin = seg[2 * j], end = seg[2 * j + 1];
    if (end - begin > (int64_t)kFixIdsRowCap) {
      if (lane == 0) {
        unsigned* e = blist + 1 + 4 * (int64_t)atomicAdd(blist, 1u);
        e[0] = (unsigned)(id >> kp.bucket_bits);
        e[1] = (unsigned)begin;
        e[2] = (unsigned)end;
        e[3] = (unsigned)id;
      }
      continue;
    }
    if (lane < l0) {
      sk[lane] = kEmpty;
      cnt[lane] = 0;
    }
    if (lane < l0 * linf) rsk[lane] = kEmpty;
    wave_lds_fence();
    const uint32_t h = pid_hash(kp.seed, id);
    const uint64_t local = (uint64_t)id & lmask;
    // record i -> its pair key (kEmpty: dead) and row
    auto record = [&](int64_t i, uint32_t* r) -> uint64_t {
      const RecKey<REC == kRecCompact> v = keys[i];
      if constexpr (REC == kRecP64) {
        *r = (uint32_t)((uint64_t)v >> kp.row_shift);
        if (v == ~0ULL) return kEmpty;
      } else {
        *r = rows[i];
        if (v >> (8 * sizeof(v) - 1)) return kEmpty;
      }
      if constexpr (REC == kRecCompact)  // expand_key: rand_shift <= 31
        return ((uint64_t)pair_hash_from(h, kp.seed, (int64_t)(v & (uint32_t)kp.pk_mask)) << 32) |
               (v & ((1u << kp.rand_shift) - 1));
      else
        return pair_key_from(h, kp.seed, (int64_t)(v & kp.pk_mask), local << kp.pk_bits, kp.rand_shift);
    };
    for (int64_t i0 = begin; i0 < end; i0 += 64) {  // B1
      uint32_t r;
      const uint64_t x = i0 + lane < end ? record(i0 + lane, &r) : kEmpty;
      if (x != kEmpty && x < sk[l0 - 1]) sketch_insert_strided(sk, l0, 1, x);
    }
    wave_lds_fence();
    if (kp.sieve_mark && sk[l0 - 1] == kEmpty) {  // wave-uniform: still short of l0 pairs
      if (lane == 0) {
        atomicOr(mk.bits + (id >> 5), 1u << (id & 31));
        const unsigned at = atomicAdd(mk.sctl, 1u);
        mk.list[at] = (unsigned)id;
        id_pos[id] = at;
        mk.seg[2 * (int64_t)at + 1] = 0;
      }
      wave_lds_fence();  // the sketch is the next id's
      continue;
    }
    for (int64_t i0 = begin; i0 < end; i0 += 64) {  // B2
      uint32_t r = 0;
      const uint64_t x = i0 + lane < end ? record(i0 + lane, &r) : kEmpty;
      if (x == kEmpty || dead_key(x, kp.rand_shift)) continue;
      const int s = sketch_find_strided(sk, l0, 1, x);
      if (s < 0) continue;
      if (r >= (uint64_t)kp.n) {  // malformed record: flagged, never dereferenced
        atomicOr(err, 1u);
        continue;
      }
      atomicAdd(cnt + s, 1u);
      const uint64_t y = row_key(kp.row_seed, kp.row_offset + r, r);
      unsigned long long* rs = rsk + s;
      if (y < rs[(linf - 1) * l0]) sketch_insert_strided(rs, linf, l0, y);
    }
    wave_lds_fence();
    if constexpr (VALUE_KIND != PDP_VALUE_NONE) {  // B2.5: entry t of slot s is lane t * l0 + s
      const bool live = lane < l0 * linf && sk[lane % l0] != kEmpty && (unsigned)(lane / l0) < cnt[lane % l0];
      if (live) rsk[lane] = (unsigned long long)((const long long*)value)[(uint32_t)rsk[lane]];
      wave_lds_fence();
    }
    bool out = false;  // B3
    int64_t p = 0;
    PairSums ps{};
    if (lane < l0) {
      const uint64_t x = sk[lane];
      const unsigned c = cnt[lane];
      if (x != kEmpty && c != 0) {
        p = (int64_t)(x & kp.pk_mask);
        if (p >= kp.P) {  // malformed record: flagged, skipped
          atomicOr(err, 1u);
        } else {
          out = true;
          ps = pair_sums_from_rows<VALUE_KIND>(rsk + lane, c < (unsigned)linf ? (long long)c : (long long)linf,
                                               nullptr, kp.clip, l0);
        }
      }
    }
    const unsigned long long mo = __ballot(out);
    if (mo) {  // wave-uniform
      unsigned base = 0;
      if (lane == 0) base = atomicAdd(rec.flat_n, (unsigned)__popcll(mo));
      base = __shfl(base, 0, 64);
      const int64_t at = (int64_t)base + __popcll(mo & ((1ULL << lane) - 1));
      if (out && at < rec.flat_cap) {  // (<= l0 pairs per id: the list cannot fill)
        const int64_t i = rec.flat_base + at;
        rec.key[i] = ((unsigned long long)p << 32) | (unsigned long long)(uint32_t)ps.count;
        if (flags & (PDP_ACC_SUM | PDP_SUM_PER_PARTITION))
          rec.f0[i] = (flags & PDP_SUM_INT) ? __longlong_as_double(ps.isum) : ps.fsum;
        if (flags & PDP_ACC_NSUM) rec.f1[i] = ps.nsum;
        if (flags & PDP_ACC_NSUM2) rec.f2[i] = ps.nsum2;
      }
    }
    wave_lds_fence();  // the sketch is the next id's
  }
}


// ---------------------------------------------------------- launchers --
int launch_global_rows(const pdp_bound_config* cfg, const KP& kp, hipStream_t st, const int64_t* pid,
                       const int64_t* pk, const void* value, const uint8_t* allowed, char* ws, const Ws& w) {
  return with_value(cfg->value_kind, cfg->linf == 0, [&](auto vk, auto ka) {
    constexpr bool KA = decltype(ka)::value;
    return launch("k_pair_rows", k_pair_rows<decltype(vk)::value, KA>, dim3(grid_for(kp.n)), dim3(kBlock), 0, st, kp,
                  pid, pk, value, allowed, at<unsigned long long>(ws, w.sketch), at<unsigned>(ws, w.cnt),
                  KA ? nullptr : at<unsigned long long>(ws, w.rows), KA ? at<double>(ws, w.fsum) : nullptr,
                  KA ? at<double>(ws, w.nsum) : nullptr, KA ? at<double>(ws, w.nsum2) : nullptr);
  });
}

int launch_global_reduce(const pdp_bound_config* cfg, const KP& kp, hipStream_t st, const void* value,
                         const char* ws, const Ws& w, const pdp_partition_accumulators& acc) {
  return with_value(cfg->value_kind, cfg->linf == 0, [&](auto vk, auto ka) {
    constexpr bool KA = decltype(ka)::value;
    return launch("k_reduce_pairs", k_reduce_pairs<decltype(vk)::value, KA>, dim3(grid_for(kp.U * kp.l0)),
                  dim3(kBlock), 0, st, kp, value, at<unsigned long long>(ws, w.sketch), at<unsigned>(ws, w.cnt),
                  KA ? nullptr : at<unsigned long long>(ws, w.rows), KA ? at<double>(ws, w.fsum) : nullptr,
                  KA ? at<double>(ws, w.nsum) : nullptr, KA ? at<double>(ws, w.nsum2) : nullptr, acc);
  });
}

// where a bucket launch marks unresolved ids (the main launch: the first
// bitmap / list / counters; the band's fix-up launch: the second ones, only
// ids in `prev`), and where the main launch with the band sends their rows
struct Marks {
  unsigned* bits;
  unsigned* list;
  unsigned* sctl;
  const unsigned* prev;
  unsigned long long* fix_rec;
  unsigned* pos;  // per-id fix-up: id_pos and the list's row counts (Ws.id_seg / id_seg2), else NULL
  unsigned* seg;
};

template <int VK, bool KA>
int launch_bucket_kernel(const KP& kp, const Plan& p, hipStream_t st, const void* keys, const unsigned* rows,
                         const unsigned* offsets, const void* value, const pdp_partition_accumulators& acc,
                         PairRecords rec, char* ws, const Ws& w, const char* name, const Marks& mk,
                         const unsigned* blist = nullptr) {
  const bool ranges = p.merge == PDP_MERGE_RANGES;
  // PACKED: COMPACT records from level 2 on; PACKED_WIDE: WIDE ones; PACKED64: its own
  return with_rec(rec_of(p.key_format), [&](auto kind) {
    constexpr int REC = decltype(kind)::value;
    using K = RecKey<REC == kRecCompact>;
    const auto kern = kp.fix_ids ? k_bucket_bound<VK, KA, true, REC, true>
                      : ranges   ? k_bucket_bound<VK, KA, true, REC>
                                 : k_bucket_bound<VK, KA, false, REC>;
    const int rc = allow_dynamic_lds(kern, (size_t)p.lds_bytes);
    if (rc != PDP_OK) return rc;
    // a listed launch (fix-ups): a persistent grid of one workgroup per CU (the
    // bucket LDS allows no more) looping over the listed buckets
    // (the per-id fix-up's: up to two of its ids over the row cap per bucket at once)
    const int64_t grid = blist != nullptr ? std::min<int64_t>(kp.fix_ids ? 2 * p.n_buckets : p.n_buckets, device_cus())
                                          : p.n_buckets;
    return launch(name, kern, dim3((unsigned)grid), dim3((unsigned)p.bucket_threads), (size_t)p.lds_bytes, st, kp,
                  (const K*)keys, rows, offsets, value, acc, rec, at<K>(ws, w.cand_key), at<unsigned>(ws, w.cand_idx),
                  mk.bits, mk.list, mk.sctl, at<unsigned>(ws, w.err), mk.fix_rec, mk.prev, blist, mk.pos, mk.seg);
  });
}

// Sampling (every bucket kernel): the main launch over the level-2 records;
// with the sieve, the fix-up of the unresolved privacy ids (their rows
// gathered, scattered into bucket order, a second launch whose pair records
// follow the main ones: buckets [n_buckets, 2 n_buckets) of `rec`).  The
// rows come from a rescan of the privacy-id column, or with the band from
// the band lists plus the candidate rows the main launch sent; the band's
// fix-up launch marks the ids still short of l0 pairs, whose rows a rescan
// then gathers for a third launch (buckets [2 n_buckets, 3 n_buckets)).
// Every step past the main launch reads its counts on the device, so an
// empty fix-up costs a few near-empty launches and no host round trip.
template <int VK, bool KA>
int launch_buckets_of(const KP& kp, const Plan& p, hipStream_t st, const int64_t* pid, const int64_t* pk,
                      const uint8_t* allowed, const void* value, const pdp_partition_accumulators& acc, char* ws,
                      const Ws& w) {
  const PairRecords rec = pair_records(ws, w, p);
  unsigned long long* fix_rec = at<unsigned long long>(ws, w.fix_rec);  // level-1 blocks are dead
  unsigned* id_pos = at_opt<unsigned>(ws, w.id_pos);  // the three: per-id fix-up only
  unsigned* seg1 = at_opt<unsigned>(ws, w.id_seg);
  unsigned* seg2 = at_opt<unsigned>(ws, w.id_seg2);  // ... with the band
  void* keys2 = at<void>(ws, w.keys2);
  unsigned* rows2 = at<unsigned>(ws, w.rows2);
  unsigned* err = at<unsigned>(ws, w.err);
  Marks m1{at_opt<unsigned>(ws, w.unres_bits), at_opt<unsigned>(ws, w.unres_list), at_opt<unsigned>(ws, w.sctl),
           nullptr, p.band ? fix_rec : nullptr, id_pos, seg1};
  int rc = launch_bucket_kernel<VK, KA>(kp, p, st, keys2, rows2, at<unsigned>(ws, w.counts), value, acc, rec, ws, w,
                                        "k_bucket_bound", m1);
  if (rc != PDP_OK || !p.sieve) return rc;
  const int64_t n_slots = (int64_t)kp.l0 << kp.bucket_bits;
  // what both fix-ups launch with: the listed buckets, kernel parameters that
  // mark as asked and emit nothing, the bucket workgroup halved where `half`
  unsigned* blist = at<unsigned>(ws, w.fix_blist);
  auto fix_kp = [&](int mark) { KP kf = kp; kf.sieve_mark = mark; kf.sieve_emit = 0; return kf; };
  auto fix_plan = [&](bool half) { Plan pf = p; if (half) pf.bucket_threads = kBucketThreads / 2; return pf; };
  // one fix-up: rows listed in fix_rec (sctl[1] of them) -> exact test ->
  // bucket order -> a bucket launch over them into record segment `seg`
  auto fixup = [&](unsigned* bits, unsigned* sctl, unsigned* fix_cnt, unsigned* fix_cur, int seg, const Marks& mk,
                   int mark, const char* name) -> int {
    int r = launch("k_fix_filter", k_fix_filter, dim3(grid_for(kp.n, 1024)), dim3(kBlock), 0, st, kp, bits, sctl,
                   fix_rec, fix_cnt, err, blist);
    if (r != PDP_OK) return r;
    r = scan_u32(fix_cnt, p.n_buckets, at<unsigned>(ws, w.chunk_sums), st);  // -> starts
    if (r != PDP_OK) return r;
    r = with_rec(rec_of(p.key_format), [&](auto kind) {
      constexpr int REC = decltype(kind)::value;
      return launch("k_fix_scatter", k_fix_scatter<REC>, dim3(grid_for(kp.n, 2048)), dim3(kBlock), 0, st, kp, pk,
                    allowed, fix_rec, sctl, fix_cnt, fix_cur, (RecKey<REC == kRecCompact>*)keys2, rows2);
    });
    if (r != PDP_OK) return r;
    const KP kf = fix_kp(mark);
    PairRecords fr = rec;
    fr.runs += seg * p.n_buckets;  // column offset (range-major table)
    fr.key += seg * p.n_buckets * n_slots;
    if (fr.f0) fr.f0 += seg * p.n_buckets * n_slots;
    if (fr.f1) fr.f1 += seg * p.n_buckets * n_slots;
    if (fr.f2) fr.f2 += seg * p.n_buckets * n_slots;
    // fix-up buckets hold only unresolved ids' rows and most are empty: the
    // buckets with rows are listed (k_fix_buckets, which also writes the
    // empty ones' runs and marks) and run on 512 threads (the kernel sizes its
    // queues from blockDim)
    r = launch("k_fix_buckets", k_fix_buckets, dim3(grid_for(p.n_buckets), kFixRunRows), dim3(kBlock), 0, st, kf,
               fix_cnt, p.merge == PDP_MERGE_RANGES ? fr.runs : nullptr, fr.run_stride, blist,
               mark ? mk.prev : nullptr, mk.bits, mk.list, mk.sctl);
    if (r != PDP_OK) return r;
    const Plan pf = fix_plan(p.merge != PDP_MERGE_RANGES || p.n_ranges <= kBucketThreads / 2);
    return launch_bucket_kernel<VK, KA>(kf, pf, st, keys2, rows2, fix_cnt, value, acc, fr, ws, w, name, mk, blist);
  };
  // the same per privacy id (Plan.fix_ids): exact test + rows per id -> id
  // order -> one wave per listed id (`list`, its rows' bounds in `seg`),
  // whose kept pairs go to the flat list after the main launch's records;
  // ids over the row cap -> a listed bucket launch (empty unless there is one)
  auto fixup_ids = [&](unsigned* bits, const unsigned* list, unsigned* sctl, unsigned* seg, const Marks& mk, int mark,
                       const char* name) -> int {
    int r = launch("k_fix_filter", k_fix_id_count, dim3(grid_for(kp.n, 1024)), dim3(kBlock), 0, st, kp, bits, sctl,
                   fix_rec, id_pos, seg, err, blist);
    if (r != PDP_OK) return r;
    r = launch("k_fix_alloc", k_fix_id_alloc, dim3(1), dim3(kBlock), 0, st, sctl, seg);
    if (r != PDP_OK) return r;
    KP kf = fix_kp(mark);
    r = with_rec(rec_of(p.key_format), [&](auto kind) {
      constexpr int REC = decltype(kind)::value;
      using K = RecKey<REC == kRecCompact>;
      int r2 = launch("k_fix_scatter", k_fix_id_scatter<REC>, dim3(grid_for(kp.n, 2048)), dim3(kBlock), 0, st, kp, pk,
                      allowed, fix_rec, sctl, id_pos, seg, (K*)keys2, rows2);
      if (r2 != PDP_OK) return r2;
      const IdMarks im{mk.bits, mk.list, mk.sctl, mk.seg};
      // persistent: four ids per workgroup at a time, up to 8 workgroups per CU
      const int64_t ids = p.n_buckets << p.bucket_bits;
      const int64_t grid = std::min<int64_t>((ids + 3) / 4, 8 * device_cus());
      return launch("k_fix_ids", k_fix_ids<VK, REC>, dim3((unsigned)grid), dim3(kFixIdsThreads), 0, st, kf,
                    list, sctl, seg, (const K*)keys2, rows2, value, rec, im, id_pos, blist, err);
    });
    if (r != PDP_OK) return r;
    kf.fix_ids = 1;
    const Plan pf = fix_plan(p.n_ranges <= kBucketThreads / 2);
    return launch_bucket_kernel<VK, KA>(kf, pf, st, keys2, rows2, nullptr, value, acc, rec, ws, w, name, mk, blist);
  };
  auto rescan = [&](const unsigned* bits, const unsigned* list, unsigned* sctl) {
    return launch("k_sieve_rescan", kp.keys_vec ? k_sieve_rescan<true> : k_sieve_rescan<false>, dim3(kRescanBlocks),
                  dim3(kRescanThreads), 0, st, kp, pid, bits, list, sctl, fix_rec);
  };
  const Marks none{m1.bits, m1.list, m1.sctl, nullptr, nullptr, nullptr, nullptr};
  // the second bitmap, list and counters (regions of the band's plans only: else NULL)
  const Marks m2{at_opt<unsigned>(ws, w.unres2_bits), at_opt<unsigned>(ws, w.unres2_list),
                 at_opt<unsigned>(ws, w.sctl2), m1.bits, nullptr, id_pos, seg2};
  // fix-up n of the ids marked in m1 (n = 1) or m2 (n = 2): per id where planned, else by bucket launches
  auto fix = [&](int n, const Marks& mk, int mark, const char* name) -> int {
    const Marks& from = n == 1 ? m1 : m2;
    if constexpr (!KA)
      if (p.fix_ids) return fixup_ids(from.bits, from.list, from.sctl, n == 1 ? seg1 : seg2, mk, mark, name);
    return fixup(from.bits, from.sctl, at<unsigned>(ws, n == 1 ? w.fix_cnt : w.fix_cnt2),
                 at<unsigned>(ws, n == 1 ? w.fix_cur : w.fix_cur2), n, mk, mark, name);
  };
  if (!p.band) {
    rc = rescan(m1.bits, m1.list, m1.sctl);
    return rc != PDP_OK ? rc : fix(1, none, 0, "k_bucket_fix");
  }
  // the band: its lists (Bloom filter unless too many ids) -> fix-up launch
  // that marks the ids still unresolved -> their rescan -> a third launch
  rc = launch("k_band_scan", k_band_scan, dim3(kRescanBlocks), dim3(kRescanThreads), 0, st, kp,
              at<unsigned long long>(ws, w.band), at<unsigned>(ws, w.band_cnt), m1.bits, m1.list, m1.sctl, fix_rec);
  if (rc != PDP_OK) return rc;
  rc = fix(1, m2, 1, "k_bucket_fix");
  if (rc != PDP_OK) return rc;
  rc = rescan(m2.bits, m2.list, m2.sctl);
  if (rc != PDP_OK) return rc;
  return fix(2, m2, 0, "k_bucket_fix2");
}

int launch_buckets(int value_kind, bool keep_all, const KP& kp, const Plan& p, hipStream_t st, const int64_t* pid,
                   const int64_t* pk, const uint8_t* allowed, const void* value,
                   const pdp_partition_accumulators& acc, char* ws, const Ws& w) {
  return with_value(value_kind, keep_all, [&](auto vk, auto ka) {
    return launch_buckets_of<decltype(vk)::value, decltype(ka)::value>(kp, p, st, pid, pk, allowed, value, acc, ws, w);
  });
}


template <int FMT>
int launch_scatter(const KP& kp, const Plan& p, hipStream_t st, const int64_t* pid, const int64_t* pk,
                   const uint8_t* allowed, const unsigned* super_off, const unsigned* super_base,
                   const unsigned* bucket_start, const unsigned* gcur, char* ws, const Ws& w, unsigned* err) {
  using K1 = L1Key<FMT>;
  using K2 = L2Key<FMT>;
  constexpr bool ROWS1 = FMT != PDP_KEYS_PACKED;
  K1* keys1 = at<K1>(ws, w.keys1);
  unsigned* rows1 = ROWS1 ? at<unsigned>(ws, w.rows1) : nullptr;
  int rc = launch_big_lds("k_scatter_l1", k_scatter_l1<FMT>, dim3((unsigned)p.n_tiles), dim3(kL1Threads),
                          sizeof(StageLds<K1, kSmallDest, ROWS1, kL1Items, kL1Threads>), st, kp, pid, pk, allowed,
                          super_off, super_base, keys1, rows1, err);
  if (rc != PDP_OK || p.super_bits == 0) return rc;
  const int64_t n_grp = (p.n_tiles + kL2GroupTiles - 1) / kL2GroupTiles;
  const bool small = ((int64_t)1 << p.super_bits) <= kSmallDest;
  const auto l2 = small ? k_scatter_l2<FMT, kSmallDest> : k_scatter_l2<FMT, kMaxDest>;
  const size_t lds2 = small ? sizeof(StageLds<K2, kSmallDest, true, kL2Items, kL2Threads>)
                            : sizeof(StageLds<K2, kMaxDest, true, kL2Items, kL2Threads>);
  return launch_big_lds("k_scatter_l2", l2, dim3((unsigned)n_grp, (unsigned)p.n_supers), dim3(kL2Threads), lds2, st,
                        kp, super_base, super_off, bucket_start, gcur, keys1, rows1, at<K2>(ws, w.keys2),
                        at<unsigned>(ws, w.rows2));
}

// The small control regions a bounding call starts from (error word, the
// tiles' overflow marks, the fix-ups' counters and cursors), set by ONE
// launch instead of a memset each (C3: eight fills of 16 B - 20 KB, ~4 us
// apiece on the stream)
constexpr int kMaxFills = 10;
struct Fills {
  unsigned* p[kMaxFills];
  int64_t n[kMaxFills];  // u32 words
  unsigned v[kMaxFills];
  int k;
};
__global__ void __launch_bounds__(kBlock) k_fill(Fills f) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int j = 0; j < f.k; ++j)
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < f.n[j]; i += stride) f.p[j][i] = f.v[j];
}

int launch_fills(const Fills& f, hipStream_t st) {
  int64_t most = 0;
  for (int j = 0; j < f.k; ++j) most = std::max(most, f.n[j]);
  if (most == 0) return PDP_OK;
  return launch("k_fill", k_fill, dim3((unsigned)std::min<int64_t>((most + kBlock - 1) / kBlock, 256)), dim3(kBlock),
                0, st, f);
}

// test hook (tools/l1_probe.py): level 1 alone, timed by the profiler;
// nothing downstream reads what it wrote
bool stop_after_l1() { return test_hooks_enabled() && std::getenv("PIPELINEDP_AMD_STOP_AFTER_L1") != nullptr; }

// The per-tile bucket counts (counts_tm) -> rows per bucket -> level-2
// cursors at the tile groups (gcur) -> bucket starts (counts, scanned in
// place).  `local`: the counts of tile-local level 1 (u16 halves in counts_tm
// and counts_tm2 or u32, less the tiles in tile_over; eight buckets per lane),
// whose group sums give the cursors in one pass over the counts; else u32
// counts of k_part_hist, four per lane, and the cursors, which only a second
// level reads, by k_gscan_cursors.
int launch_bucket_starts(const KP& kp, const Plan& p, hipStream_t st, char* ws, const Ws& w, bool local) {
  const unsigned* counts_tm = at<unsigned>(ws, w.counts_tm);
  unsigned* counts = at<unsigned>(ws, w.counts);
  unsigned* csum = at<unsigned>(ws, w.csum);
  unsigned* gcur = at<unsigned>(ws, w.gcur);
  const int64_t n_sc = (p.n_tiles + kScanChunkTiles - 1) / kScanChunkTiles;
  const int64_t per_block = local ? 512 : 256;  // buckets of a k_gscan_sums workgroup: eight or four per lane
  int rc = launch("k_gscan_sums", local ? k_gscan_sums<true> : k_gscan_sums<false>,
                  dim3((unsigned)((p.n_buckets + per_block - 1) / per_block), (unsigned)n_sc), dim3(64 * kScanWaves), 0,
                  st, counts_tm, local ? at_opt<unsigned>(ws, w.counts_tm2) : nullptr,
                  local ? at<unsigned>(ws, w.tile_over) : nullptr, p.n_tiles, p.n_buckets, kp.cstride, csum,
                  local ? gcur : nullptr);
  if (rc != PDP_OK) return rc;
  rc = launch("k_gscan_chunks", k_gscan_chunks, dim3(grid_for(p.n_buckets)), dim3(kBlock), 0, st, csum, n_sc,
              p.n_buckets, counts);
  if (rc != PDP_OK) return rc;
  if (local) {
    rc = launch("k_gscan_groups", k_gscan_groups, dim3(grid_for(n_sc * p.n_buckets, (int64_t)1 << 30)), dim3(kBlock), 0,
                st, csum, p.n_tiles, p.n_buckets, gcur);
  } else if (p.super_bits > 0) {
    rc = launch("k_gscan_cursors", k_gscan_cursors, dim3((unsigned)((p.n_buckets + 63) / 64), (unsigned)n_sc),
                dim3(64 * kScanWaves), 0, st, counts_tm, nullptr, p.n_tiles, p.n_buckets, kp.cstride, csum, gcur);
  }
  if (rc != PDP_OK) return rc;
  return scan_u32(counts, p.n_buckets, at<unsigned>(ws, w.chunk_sums), st);
}

// tile-local level 1 -> level-2 cursors and bucket starts -> tile-local level 2
template <int FMT>
int launch_local_fmt(const KP& kp, const Plan& p, hipStream_t st, const int64_t* pid, const int64_t* pk,
                     const uint8_t* allowed, char* ws, const Ws& w, unsigned* err) {
  using K1 = L1Key<FMT>;
  using K2 = L2Key<FMT>;
  constexpr bool ROWS1 = !kPackedL1<FMT>;
  unsigned* counts_tm = at<unsigned>(ws, w.counts_tm);
  const bool u16 = p.hist_u16 != 0;
  unsigned* counts_tm2 = at_opt<unsigned>(ws, w.counts_tm2);  // the u16 counts' second halves
  uint16_t* soff = at<uint16_t>(ws, w.soff);
  unsigned* tile_over = at<unsigned>(ws, w.tile_over);  // all ones (k_fill) unless a tile's rows are all one bucket's
  unsigned* sbase = at_opt<unsigned>(ws, w.sbase);      // the sieve's
  K1* keys1 = at<K1>(ws, w.keys1);
  unsigned* rows1 = ROWS1 ? at<unsigned>(ws, w.rows1) : nullptr;
  if constexpr (FMT != PDP_KEYS_WIDE) {
    if (p.sieve) {
      const int th = p.sieve_threads;
      auto pick = [&](auto th_tag) {
        constexpr int TH = decltype(th_tag)::value;
        return p.band ? (u16 ? k_sieve_l1<FMT, true, true, TH> : k_sieve_l1<FMT, false, true, TH>)
                      : (u16 ? k_sieve_l1<FMT, true, false, TH> : k_sieve_l1<FMT, false, false, TH>);
      };
      const auto l1 = th == kSieveThreads2 ? pick(std::integral_constant<int, kSieveThreads2>{})
                                           : pick(std::integral_constant<int, kL1Threads>{});
      const size_t lds1 = (size_t)sieve_lds(FMT, th, p.n_buckets, u16, p.band != 0);
      int rc = allow_dynamic_lds(l1, lds1);
      if (rc != PDP_OK) return rc;
      // persistent: as many workgroups as fit at once (one per CU at 1,024
      // threads, two at 512), each looping over its tiles
      const int64_t per_cu = th == kSieveThreads2 ? 2 : 1;
      int64_t grid1 = std::min<int64_t>(p.n_tiles, per_cu * device_cus());
      // test hook: fewer workgroups, so that each loops over several tiles
      // (the cross-tile prefetch and the per-tile LDS reset) at test sizes
      if (const long long v = test_hook("PIPELINEDP_AMD_L1_GRID"); v > 0 && v < grid1) grid1 = v;
      rc = launch("k_sieve_l1", l1, dim3((unsigned)grid1), dim3(th), lds1, st, kp, pid, pk, allowed, counts_tm,
                  counts_tm2, soff, sbase, keys1, rows1, err, at_opt<unsigned long long>(ws, w.band),
                  at_opt<unsigned>(ws, w.band_cnt), tile_over);
      if (rc != PDP_OK) return rc;
    }
  }
  if ((kp.clip.flags & PDP_PROBE_LEVEL1) && p.sieve) return PDP_OK;  // placement probe: level 1 only
  if (stop_after_l1() && p.sieve) return PDP_OK;
  int rc = PDP_OK;
  if (!p.sieve) {
    const size_t lds1 = (l1_stage_bytes(FMT) + 7) / 8 * 8 + (size_t)l1_hist_bytes(p.n_buckets, u16);
    // (one workgroup per tile: a persistent form with the next stage's loads
    // issued early measured the same at C5, 3.04 vs 3.06 ms -- the 2:1
    // read/write mix, not load latency, bounds it; profiles/r04/ab/ab3_l1_local.txt)
    rc = launch_big_lds("k_scatter_l1", u16 ? k_scatter_l1_local<FMT, true> : k_scatter_l1_local<FMT, false>,
                        dim3((unsigned)p.n_tiles), dim3(kL1Threads), lds1, st, kp, pid, pk, allowed, counts_tm,
                        counts_tm2, soff, keys1, rows1, err, tile_over);
    if (rc != PDP_OK) return rc;
    if (kp.clip.flags & PDP_PROBE_LEVEL1) return PDP_OK;  // placement probe: level 1 only
  }
  rc = launch_bucket_starts(kp, p, st, ws, w, true);
  if (rc != PDP_OK) return rc;
  const int64_t n_grp = (p.n_tiles + kL2GroupTiles - 1) / kL2GroupTiles;
  const bool small = ((int64_t)1 << p.super_bits) <= kSmallDest;
  const auto l2 = small ? k_scatter_l2_local<FMT, kSmallDest> : k_scatter_l2_local<FMT, kMaxDest>;
  const size_t lds2 = small ? sizeof(StageLds<K2, kSmallDest, kL2RowArray<FMT>, l2_items<FMT>(), kL2Threads>)
                            : sizeof(StageLds<K2, kMaxDest, kL2RowArray<FMT>, l2_items<FMT>(), kL2Threads>);
  const int64_t n_mgrp = (n_grp + kp.l2_group_mult - 1) / kp.l2_group_mult;  // tile groups per workgroup
  const int64_t n_blk = (n_mgrp + 7) / 8 * 8 * p.n_supers;  // k_scatter_l2_local maps ids to (group, super)
  return launch_big_lds("k_scatter_l2", l2, dim3((unsigned)n_blk), dim3(kL2Threads), lds2, st, kp, soff, sbase,
                        at<unsigned>(ws, w.counts), at<unsigned>(ws, w.gcur), keys1, rows1, at<K2>(ws, w.keys2),
                        at<unsigned>(ws, w.rows2));
}

int launch_local(const KP& kp, const Plan& p, hipStream_t st, const int64_t* pid, const int64_t* pk,
                 const uint8_t* allowed, char* ws, const Ws& w, unsigned* err) {
  return with_key_format(p.key_format, [&](auto fmt) {
    return launch_local_fmt<decltype(fmt)::value>(kp, p, st, pid, pk, allowed, ws, w, err);
  });
}

// PDP_DEBUG_CORRUPT_RECORDS (tests only): every level-2 record of bucket 0
// gets the all-ones partition (>= P when P is not a power of two) and every
// record of bucket 1 an out-of-range row, as a malformed workspace would
// carry; the bucket kernel must flag them in the error word, not fault
template <int REC>
__global__ void __launch_bounds__(kBlock) k_debug_corrupt(KP kp, const unsigned* __restrict__ starts,
                                                          RecKey<REC == kRecCompact>* __restrict__ keys,
                                                          unsigned* __restrict__ rows) {
  const int64_t nb = kp.n_buckets < 2 ? kp.n_buckets : 2;
  for (int64_t i = (int64_t)starts[0] + blockIdx.x * blockDim.x + threadIdx.x; i < (int64_t)starts[nb];
       i += (int64_t)gridDim.x * blockDim.x) {
    if (i < (int64_t)starts[1]) {
      if (REC != kRecP64 || keys[i] != ~0ull) keys[i] = keys[i] | (RecKey<REC == kRecCompact>)kp.pk_mask;
    } else if constexpr (REC == kRecP64) {  // row field all ones but one: >= n_rows (the plan keeps rows below)
      const uint64_t low = (1ull << kp.row_shift) - 1;
      if (keys[i] != ~0ull) keys[i] = (keys[i] & low) | (((~0ull >> kp.row_shift) - 1) << kp.row_shift);
    } else {
      rows[i] = 0xFFFFFFF0u;
    }
  }
}

int launch_debug_corrupt(const KP& kp, const Plan& p, hipStream_t st, char* ws, const Ws& w) {
  if (!(kp.clip.flags & PDP_DEBUG_CORRUPT_RECORDS)) return PDP_OK;  // (kp.clip.flags: the config's)
  return with_rec(rec_of(p.key_format), [&](auto rec) {
    constexpr int REC = decltype(rec)::value;
    return launch(nullptr, k_debug_corrupt<REC>, dim3(64), dim3(kBlock), 0, st, kp, at<unsigned>(ws, w.counts),
                  at<RecKey<REC == kRecCompact>>(ws, w.keys2), at<unsigned>(ws, w.rows2));
  });
}

// histogram pass over the privacy ids -> global offsets -> level 1 -> level 2
// (plans whose tile-local level 1 does not fit)
int launch_offsets(const KP& kp, const Plan& p, hipStream_t st, const int64_t* privacy_id,
                   const int64_t* partition_key, const uint8_t* pk_allowed, char* ws, const Ws& w, unsigned* err) {
  unsigned* counts = at<unsigned>(ws, w.counts);
  unsigned* super_tm = at<unsigned>(ws, w.super_tm);
  unsigned* super_off = at<unsigned>(ws, w.super_off);
  int rc = launch_big_lds("k_part_hist", k_part_hist, dim3((unsigned)p.n_tiles), dim3(kPartThreads),
                          (size_t)p.n_buckets * 4, st, kp, privacy_id, at<unsigned>(ws, w.counts_tm), super_tm, err);
  if (rc != PDP_OK) return rc;
  rc = launch("k_super_scan", k_super_scan, dim3((unsigned)p.n_supers), dim3(kBlock), 0, st, kp, super_tm, super_off);
  if (rc != PDP_OK) return rc;
  // rows per bucket (and, with two levels, the level-2 cursors at tile-group starts)
  rc = launch_bucket_starts(kp, p, st, ws, w, false);
  if (rc != PDP_OK) return rc;
  unsigned* super_base = at<unsigned>(ws, w.super_base);
  rc = launch("k_super_bases", k_super_bases, dim3(grid_for(p.n_supers + 1)), dim3(kBlock), 0, st, kp, counts,
              super_base);
  if (rc != PDP_OK) return rc;
  // three formats only: PACKED_WIDE and PACKED64 are planned with tile-local level 1 alone
  auto scatter = [&](auto fmt) {
    return launch_scatter<decltype(fmt)::value>(kp, p, st, privacy_id, partition_key, pk_allowed, super_off,
                                                super_base, counts, at<unsigned>(ws, w.gcur), ws, w, err);
  };
  if (p.key_format == PDP_KEYS_COMPACT) return scatter(std::integral_constant<int, PDP_KEYS_COMPACT>{});
  if (p.key_format == PDP_KEYS_PACKED) return scatter(std::integral_constant<int, PDP_KEYS_PACKED>{});
  return scatter(std::integral_constant<int, PDP_KEYS_WIDE>{});
}

// the value column against the config (pdp_bound_contributions, pdp_reduce_partitions)
int check_value_args(const pdp_bound_config* cfg, const void* value) {
  if (cfg->value_kind == PDP_VALUE_NONE &&
      (cfg->flags & (PDP_ACC_SUM | PDP_ACC_NSUM | PDP_ACC_NSUM2 | PDP_SUM_PER_PARTITION)))
    return set_error(PDP_E_INVALID, "value sums requested without a value column");
  if (cfg->value_kind != PDP_VALUE_NONE && cfg->n_rows > 0 && value == nullptr)
    return set_error(PDP_E_INVALID, "value column is NULL");
  return PDP_OK;
}

// the call ran the bucketed path, so the workspace holds its counters (`p` is set only outside pairs mode)
bool ran_bucketed(const pdp_bound_config* cfg, const Plan& p) {
  return !pairs_mode(cfg) && p.algorithm == PDP_ALGO_BUCKETED && cfg->n_rows > 0;
}

}  // namespace
}  // namespace pdp

using namespace pdp;

extern "C" {

int pdp_bound_contributions(const pdp_bound_config* cfg, const int64_t* privacy_id, const int64_t* partition_key,
                            const void* value, const uint8_t* pk_allowed, void* workspace,
                            uint64_t workspace_bytes, void* stream) {
  Plan p;
  Ws w;
  int rc = check_ws(cfg, workspace, workspace_bytes, &p, &w);
  if (rc != PDP_OK) return rc;
  if (cfg->n_rows > 0 && (partition_key == nullptr || (privacy_id == nullptr && !cfg->rows_are_units)))
    return set_error(PDP_E_INVALID, "key columns are NULL");
  if (const int rcv = check_value_args(cfg, value); rcv != PDP_OK) return rcv;
  hipStream_t st = (hipStream_t)stream;
  char* ws = (char*)workspace;
  if (pairs_mode(cfg)) return pairs_bound(cfg, privacy_id, partition_key, value, pk_allowed, ws, st);
  KP kp = make_kp(cfg, p);
  kp.keys_vec = ((((uintptr_t)privacy_id) | ((uintptr_t)partition_key)) & 15) == 0;
  kp.fix_cap = (int64_t)w.fix_cap;
  // test hook: a smaller fix-up list region, so that the guard of its writes
  // and error bit 1 can be exercised (the real region cannot overflow)
  if (const long long v = test_hook("PIPELINEDP_AMD_FIX_CAP"); v > 0 && v < kp.fix_cap) kp.fix_cap = v;
  unsigned* err = at<unsigned>(ws, w.err);
  if (p.algorithm != PDP_ALGO_BUCKETED || cfg->n_rows == 0) PDP_HIP_CHECK(hipMemsetAsync(err, 0, 16, st));
  if (p.algorithm == PDP_ALGO_GLOBAL_SKETCH) {
    const uint64_t slots = (uint64_t)cfg->n_privacy_ids * (uint64_t)cfg->l0;
    unsigned long long* sketch = at<unsigned long long>(ws, w.sketch);
    PDP_HIP_CHECK(hipMemsetAsync(sketch, 0xFF, slots * 8, st));
    PDP_HIP_CHECK(hipMemsetAsync(at<unsigned>(ws, w.cnt), 0, slots * 4, st));
    if (cfg->linf > 0) PDP_HIP_CHECK(hipMemsetAsync(at<void>(ws, w.rows), 0xFF, slots * (uint64_t)cfg->linf * 8, st));
    else PDP_HIP_CHECK(hipMemsetAsync(at<void>(ws, w.fsum), 0, w.total - w.fsum, st));
    if (cfg->n_rows == 0) return PDP_OK;
    rc = launch("k_pair_sketch", k_pair_sketch, dim3(grid_for(cfg->n_rows)), dim3(kBlock), 0, st, kp, privacy_id,
                partition_key, pk_allowed, sketch, err);
    if (rc != PDP_OK) return rc;
    return launch_global_rows(cfg, kp, st, privacy_id, partition_key, value, pk_allowed, ws, w);
  }
  // bucketed: histogram -> transpose -> scan -> cursors -> scatter (1 or 2 levels)
  if (cfg->n_rows == 0) {  // rows per bucket -> bucket starts
    PDP_HIP_CHECK(hipMemsetAsync(at<unsigned>(ws, w.counts), 0, (p.n_buckets + 1) * 4, st));
    return PDP_OK;
  }
  {  // the control regions: one k_fill launch
    Fills f{};
    auto add = [&](uint64_t off, int64_t words, unsigned v) {
      f.p[f.k] = at<unsigned>(ws, off);
      f.n[f.k] = words;
      f.v[f.k] = v;
      ++f.k;
    };
    add(w.err, 4, 0u);
    if (p.l1_local) add(w.tile_over, p.n_tiles, ~0u);
    if (p.merge == PDP_MERGE_RANGES && p.sieve) add(w.sctl, 4, 0u);
    if (p.merge == PDP_MERGE_RANGES && p.sieve && !p.fix_ids) {
      add(w.fix_cnt, p.n_buckets + 1, 0u);
      add(w.fix_cur, p.n_buckets, 0u);
    }
    if (p.merge == PDP_MERGE_RANGES && p.band && !p.fix_ids) {
      add(w.fix_cnt2, p.n_buckets + 1, 0u);
      add(w.fix_cur2, p.n_buckets, 0u);
    }
    if (p.fix_ids) {  // {unused, fix-up pairs}; the second bitmap is set bit by bit
      add(w.fix_ctl, 4, 0u);
      if (p.band) add(w.unres2_bits, (p.n_buckets << p.bucket_bits) / 32, 0u);
    }
    if (const int rcf = launch_fills(f, st); rcf != PDP_OK) return rcf;
  }
  int rc2 = p.l1_local ? launch_local(kp, p, st, privacy_id, partition_key, pk_allowed, ws, w, err)
                       : launch_offsets(kp, p, st, privacy_id, partition_key, pk_allowed, ws, w, err);
  if (rc2 != PDP_OK) return rc2;
  if (cfg->flags & PDP_PROBE_LEVEL1) return PDP_OK;  // placement probe: level 1 only
  if (stop_after_l1()) return PDP_OK;
  // PDP_MERGE_ATOMIC: the bucket kernel adds into the accumulators, so it
  // runs in pdp_reduce_partitions; PDP_MERGE_RANGES: all sampling runs here
  if (p.merge != PDP_MERGE_RANGES) return PDP_OK;
  rc2 = launch_debug_corrupt(kp, p, st, ws, w);
  if (rc2 != PDP_OK) return rc2;
  const pdp_partition_accumulators none{};
  return launch_buckets(cfg->value_kind, cfg->linf == 0, kp, p, st, privacy_id, partition_key, pk_allowed, value,
                        none, ws, w);
}

int pdp_bound_stats_read(const pdp_bound_config* cfg, const void* workspace, uint64_t workspace_bytes,
                         pdp_bound_stats* out, void* stream) {
  if (out == nullptr) return set_error(PDP_E_INVALID, "out is NULL");
  Plan p;
  Ws w;
  const int rc = check_ws(cfg, workspace, workspace_bytes, &p, &w);
  if (rc != PDP_OK) return rc;
  *out = pdp_bound_stats{};
  hipStream_t st = (hipStream_t)stream;
  const char* ws = (const char*)workspace;
  PDP_HIP_CHECK(hipMemcpyAsync(&out->error_flags, at<unsigned>(ws, w.err), 4, hipMemcpyDeviceToHost, st));
  unsigned rows = 0, ctl[2] = {0, 0};
  const bool bucketed = ran_bucketed(cfg, p);
  if (bucketed) PDP_HIP_CHECK(hipMemcpyAsync(&rows, at<unsigned>(ws, w.counts) + p.n_buckets, 4, hipMemcpyDeviceToHost, st));
  if (bucketed && p.sieve) PDP_HIP_CHECK(hipMemcpyAsync(ctl, at<unsigned>(ws, w.sctl), 8, hipMemcpyDeviceToHost, st));
  unsigned ctl2[2] = {0, 0};
  std::vector<unsigned> bc;
  if (bucketed && p.band) {
    PDP_HIP_CHECK(hipMemcpyAsync(ctl2, at<unsigned>(ws, w.sctl2), 8, hipMemcpyDeviceToHost, st));
    bc.resize((size_t)p.n_tiles);
    PDP_HIP_CHECK(hipMemcpyAsync(bc.data(), at<unsigned>(ws, w.band_cnt), (size_t)p.n_tiles * 4, hipMemcpyDeviceToHost, st));
  }
  PDP_HIP_CHECK(hipStreamSynchronize(st));
  out->rows_partitioned = rows;
  out->unresolved_ids = ctl[0];
  out->fixup_rows = ctl[1];
  out->sieve = bucketed ? p.sieve : 0;
  out->band = bucketed ? p.band : 0;
  for (unsigned v : bc) out->band_rows += v;
  out->unresolved2_ids = ctl2[0];
  out->fixup2_rows = ctl2[1];
  return PDP_OK;
}

int pdp_bound_stats_async(const pdp_bound_config* cfg, const void* workspace, uint64_t workspace_bytes,
                          uint32_t* out, void* stream) {
  if (out == nullptr) return set_error(PDP_E_INVALID, "out is NULL");
  Plan p;
  Ws w;
  const int rc = check_ws(cfg, workspace, workspace_bytes, &p, &w);
  if (rc != PDP_OK) return rc;
  hipStream_t st = (hipStream_t)stream;
  const char* ws = (const char*)workspace;
  const bool bucketed = ran_bucketed(cfg, p);
  if (!(bucketed && p.sieve)) out[0] = out[1] = 0;
  if (!(bucketed && p.band)) out[2] = out[3] = 0;
  // sctl2 = sctl + 8 bytes (layout): one copy of both counter pairs
  if (bucketed && p.sieve)
    PDP_HIP_CHECK(hipMemcpyAsync(out, at<unsigned>(ws, w.sctl), p.band ? 16 : 8, hipMemcpyDeviceToHost, st));
  return PDP_OK;
}

int pdp_reduce_partitions(const pdp_bound_config* cfg, const void* value, void* workspace,
                          uint64_t workspace_bytes, const pdp_partition_accumulators* acc, void* stream) {
  Plan p;
  Ws w;
  int rc = check_ws(cfg, workspace, workspace_bytes, &p, &w);
  if (rc != PDP_OK) return rc;
  if (acc == nullptr || acc->privacy_id_count == nullptr)
    return set_error(PDP_E_INVALID, "accumulators.privacy_id_count is required");
  if ((cfg->flags & (PDP_ACC_SUM | PDP_SUM_PER_PARTITION)) && acc->sum == nullptr)
    return set_error(PDP_E_INVALID, "accumulators.sum is required by flags");
  if ((cfg->flags & PDP_ACC_NSUM) && acc->normalized_sum == nullptr)
    return set_error(PDP_E_INVALID, "accumulators.normalized_sum is required by flags");
  if ((cfg->flags & PDP_ACC_NSUM2) && acc->normalized_sum_sq == nullptr)
    return set_error(PDP_E_INVALID, "accumulators.normalized_sum_sq is required by flags");
  if (const int rcv = check_value_args(cfg, value); rcv != PDP_OK) return rcv;
  hipStream_t st = (hipStream_t)stream;
  char* ws = (char*)workspace;
  if (pairs_mode(cfg)) return pairs_reduce(cfg, value, ws, *acc, st);
  const KP kp = make_kp(cfg, p);
  if (p.algorithm == PDP_ALGO_GLOBAL_SKETCH)
    return launch_global_reduce(cfg, kp, st, value, ws, w, *acc);
  if (cfg->n_rows == 0) return PDP_OK;
  if (p.merge == PDP_MERGE_RANGES) return launch_merge(kp, p, st, ws, w, *acc);
  rc = launch_debug_corrupt(kp, p, st, ws, w);
  if (rc != PDP_OK) return rc;
  // PDP_MERGE_ATOMIC (never sieved: the key columns are not needed here)
  return launch_buckets(cfg->value_kind, cfg->linf == 0, kp, p, st, nullptr, nullptr, nullptr, value, *acc, ws, w);
}

}  // extern "C"
