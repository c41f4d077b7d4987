// pdp_bound_planner.hip -- what a bounding call runs on, decided on the host
// from its config alone: the argument checks (validate), the plan (make_plan:
// buckets, merge, key format, sieve, LDS), the workspace layout, the kernel
// parameters (make_kp) and the two C entry points that only report them.  No
// kernel: the launches are in pdp_bound.hip and pdp_bound_merge.hip.
#include <algorithm>
#include <cmath>
#include <cstdlib>

#include "pdp_bound_plan.h"

namespace pdp {
namespace {

constexpr int64_t kL1LocalLds = 150 * 1024;  // tile-local level 1: LDS cap (one 1,024-thread workgroup per CU)
inline bool l1_hist_u16(int key_format, int64_t n_buckets) {
  return (int64_t)l1_stage_bytes(key_format) + l1_hist_bytes(n_buckets, false) > kL1LocalLds;
}
constexpr int64_t kSieveLds2 = 80 * 1024 - 256;  // two 512-thread workgroups per CU
constexpr int kSieveMaxT16 = 1 << 15;                          // t <= 1/2
constexpr double kL2Target = 7000.0;  // records of a level-2 workgroup with the sieve (kSieveL2Groups)

int64_t per_pid_lds(const pdp_bound_config* c) {
  const int64_t l0 = c->l0;
  const int64_t pair = 4 + (c->linf > 0 ? 8 * (int64_t)c->linf : 24);
  return l0 * 8 + l0 * pair;  // pair sketch + per-pair state
}

// The plan with at most 2^max_bucket_bits privacy ids per bucket (make_plan
// lowers it until the bucket kernel's LDS fits), in five steps, each reading
// what the steps before it set.

// 1. bucket and super-bucket bits (and with them the algorithm)
void plan_buckets(const pdp_bound_config* c, int max_bucket_bits, Plan& p) {
  p.pk_bits = bits_for(c->n_partitions);
  const int64_t per_pid = per_pid_lds(c);
  // the bucket kernel's workgroup: 512 threads (on request) only where the
  // per-partition-range scan fits one thread per range
  const int64_t n_ranges_est = (c->n_partitions + kRangeParts - 1) >> kRangeBits;
  p.bucket_threads = c->bucket_threads == kBucketThreads / 2 &&
                             (n_ranges_est <= kBucketThreads / 2 || n_ranges_est > kMaxRanges)
                         ? kBucketThreads / 2
                         : kBucketThreads;
  const int64_t max_pids = (p.bucket_threads == kBucketThreads ? kLdsBudget : kLdsBudget2) / per_pid;
  int s = -1, s2 = 0;
  if (max_pids >= 16) {
    s = 0;
    while (((int64_t)2 << s) <= max_pids) ++s;          // largest 2^s <= max_pids
    // test hook: smaller buckets
    if (const long long v = test_hook("PIPELINEDP_AMD_BUCKET_BITS"); v >= 4 && v < s) s = (int)v;
    if (s > max_bucket_bits) s = max_bucket_bits;
    const int u_bits = bits_for(c->n_privacy_ids);
    if (s > u_bits) s = u_bits;                          // one bucket covers all pids
    const int64_t nb = (c->n_privacy_ids + ((int64_t)1 << s) - 1) >> s;
    if (nb > kSingleLevelMax) {
      // two levels: level 2's input runs are a stage's rows of one
      // super-bucket (kL1Rows / supers), its output runs a window's rows of
      // one bucket (kL2Rows / 2^s2); take the s2 whose shorter run is longest
      // (C3: 77 supers x 64 buckets, C2: 62 x 32)
      int lo = 1;
      while (((nb + ((int64_t)1 << lo) - 1) >> lo) > kMaxSupers) ++lo;
      double best = -1.0;
      for (int c = lo; c <= lo + 3 && ((int64_t)1 << c) < nb; ++c) {
        const double supers = (double)((nb + ((int64_t)1 << c) - 1) >> c);
        const double score = std::min((double)kL1Rows / supers, (double)kL2Rows / (double)((int64_t)1 << c));
        if (score > best) {
          best = score;
          s2 = c;
        }
      }
    }
    // pair keys: random bits above rand_shift = pk_bits + bucket_bits
    if (nb > kMaxBuckets || 64 - p.pk_bits - s < kMinRandomBits) s = -1;
  }
  const int auto_algo = s >= 0 ? PDP_ALGO_BUCKETED : PDP_ALGO_GLOBAL_SKETCH;
  p.algorithm = c->algorithm == PDP_ALGO_AUTO ? auto_algo : c->algorithm;
  if (p.algorithm == PDP_ALGO_BUCKETED && s < 0) p.algorithm = -1;  // infeasible
  p.bucket_bits = s < 0 ? 0 : s;
  p.super_bits = s < 0 ? 0 : s2;
  p.rand_shift = p.pk_bits + p.bucket_bits;
  p.n_buckets = (c->n_privacy_ids + ((int64_t)1 << p.bucket_bits) - 1) >> p.bucket_bits;
  p.n_supers = (p.n_buckets + ((int64_t)1 << p.super_bits) - 1) >> p.super_bits;
  p.n_tiles = (c->n_rows + kTileRows - 1) / kTileRows;
  if (p.n_tiles < 1) p.n_tiles = 1;
  p.lds_bytes = ((int64_t)1 << p.bucket_bits) * per_pid;
}

// 2. merge ranges
void plan_merge(const pdp_bound_config* c, Plan& p) {
  p.range_bits = kRangeBits;
  p.n_fine = (c->n_partitions + kRangeParts - 1) >> kRangeBits;
  p.two_level = p.n_fine > kMaxRanges;
  if (p.two_level)
    while (((c->n_partitions + ((int64_t)1 << p.range_bits) - 1) >> p.range_bits) > kCoarseRanges) ++p.range_bits;
  p.n_ranges = (int)((c->n_partitions + ((int64_t)1 << p.range_bits) - 1) >> p.range_bits);
  const bool ranges_ok = p.n_ranges <= kMaxRanges;
  if (p.algorithm != PDP_ALGO_BUCKETED) {
    p.merge = 0;
  } else if (c->merge == PDP_MERGE_AUTO) {
    p.merge = ranges_ok ? PDP_MERGE_RANGES : PDP_MERGE_ATOMIC;
  } else {
    p.merge = c->merge;
    if (p.merge == PDP_MERGE_RANGES && !ranges_ok) p.algorithm = -1;  // infeasible
  }
  if (p.merge == PDP_MERGE_RANGES) {
    // per-bucket range histogram + cursors + block-scan scratch after the sketches
    p.lds_bytes += (2 * (int64_t)p.n_ranges + p.bucket_threads / 64 + 1) * 4;
  }
}

// 3. key format and l1_local
void plan_keys(const pdp_bound_config* c, Plan& p) {
  // row records of the partition passes: u32 (sub-bucket, local pid,
  // partition) with bit 31 = dead when those fields fit (COMPACT); else the
  // level-1 u64 packed record with a tile-relative row, then COMPACT pairs
  // (PACKED); else the u64 pair key + u32 row (WIDE)
  const bool compact_ok = p.super_bits + p.bucket_bits + p.pk_bits <= 31;
  const bool packed_ok = p.bucket_bits + p.pk_bits <= 31 &&
                         p.super_bits + p.bucket_bits + p.pk_bits <= 64 - 1 - kTileRowBits;
  // PACKED level 1 with WIDE records from level 2 on (tile-local level 1 only)
  const bool packed_wide_ok = p.super_bits + p.bucket_bits + p.pk_bits <= 64 - 1 - kTileRowBits;
  // ... or with one u64 per record (PACKED64): the row above the bucket-local
  // pid and partition, all ones reserved for dead records
  const int row_bits = 64 - p.bucket_bits - p.pk_bits;
  const bool packed64_ok = packed_wide_ok && (row_bits >= 33 || c->n_rows < ((int64_t)1 << row_bits) - 2);
  p.key_format = 0;
  p.n_stages = (c->n_rows + kL1Rows - 1) / kL1Rows;
  p.l1_local = 0;
  if (p.algorithm == PDP_ALGO_BUCKETED) {
    // tile-local level 1: two levels, and the bucket counts in its LDS
    auto local_fits = [&](int fmt) {
      return p.super_bits > 0 &&
             (int64_t)l1_stage_bytes(fmt) + l1_hist_bytes(p.n_buckets, true) <= kL1LocalLds;
    };
    const int want = c->key_format;
    if (want == PDP_KEYS_AUTO) {
      // tile-local: PACKED (one u64 array at level 1, so level 2 reads each
      // run as one span), else PACKED_WIDE; else COMPACT / PACKED / WIDE
      if (packed_ok && local_fits(PDP_KEYS_PACKED))
        p.key_format = PDP_KEYS_PACKED;
      else if (!packed_ok && packed64_ok && local_fits(PDP_KEYS_PACKED64))
        p.key_format = PDP_KEYS_PACKED64;
      else if (!packed_ok && packed_wide_ok && local_fits(PDP_KEYS_PACKED_WIDE))
        p.key_format = PDP_KEYS_PACKED_WIDE;
      else
        p.key_format = compact_ok ? PDP_KEYS_COMPACT : (packed_ok ? PDP_KEYS_PACKED : PDP_KEYS_WIDE);
    } else if ((want == PDP_KEYS_COMPACT && !compact_ok) || (want == PDP_KEYS_PACKED && !packed_ok) ||
               (want == PDP_KEYS_PACKED_WIDE && !(packed_wide_ok && local_fits(PDP_KEYS_PACKED_WIDE))) ||
               (want == PDP_KEYS_PACKED64 && !(packed64_ok && local_fits(PDP_KEYS_PACKED64)))) {
      p.algorithm = -1;  // infeasible
    } else {
      p.key_format = want;
    }
    // one super-bucket (no level 2): PACKED degenerates to COMPACT, which then fits
    if (p.key_format == PDP_KEYS_PACKED && p.super_bits == 0) p.key_format = PDP_KEYS_COMPACT;
    if (p.algorithm == PDP_ALGO_BUCKETED) p.l1_local = local_fits(p.key_format) ? 1 : 0;
  }
}

// 4. sieve, band, the sieve's workgroup and hist_u16
void plan_sieve(const pdp_bound_config* c, Plan& p) {
  // threshold sieve: tile-local level 1, range merge, whole 64-pid bitmap
  // words per bucket, and the sieve's larger LDS stage must fit
  const bool sieve_ok = p.algorithm == PDP_ALGO_BUCKETED && p.l1_local && p.merge == PDP_MERGE_RANGES &&
                        p.bucket_bits >= 6 && p.key_format != PDP_KEYS_WIDE &&
                        sieve_lds(p.key_format, kL1Threads, p.n_buckets, true, false) <= kL1LocalLds &&
                        p.n_tiles * kSieveTileStride < ((int64_t)1 << 32) &&
                        c->n_privacy_ids < ((int64_t)1 << 32) - 1;  // fix-up lists hold 32-bit ids
  int t16 = 0;
  if (sieve_ok && c->sieve > 0) {
    t16 = c->sieve < kSieveMaxT16 ? c->sieve : kSieveMaxT16;
  } else if (sieve_ok && c->sieve == 0) {
    // auto: a privacy id with d distinct partitions has ~d*t candidate pairs;
    // ask for l0 + 3 sqrt(l0) + 3 of them, assuming d ~ 0.6 rows per id
    // (C3: 100 rows over Zipf(1.1) keys, t = 0.15); no sieve above t = 0.35
    const double rows_per_id = (double)c->n_rows / (double)c->n_privacy_ids;
    const double want = c->l0 + 3.0 * std::sqrt((double)c->l0) + 3.0;
    const double t = want / (0.6 * rows_per_id);
    if (t <= 0.35) t16 = (int)std::ceil(t * 65536.0);
  }
  p.sieve = t16 > 0 ? t16 : 0;
  p.band = 0;
  if (p.sieve) {
    const int t2 = 2 * p.sieve < kSieveMaxT16 ? 2 * p.sieve : kSieveMaxT16;
    const bool fits = sieve_lds(p.key_format, kL1Threads, p.n_buckets, true, true) <= kL1LocalLds;
    // auto: only below t = 1/4 -- there an id short of l0 candidate pairs,
    // and with it the 8 B/row rescan, is likely (C3: t = 0.154, ~1,600 of 1e7
    // ids; C2's t = 0.325 leaves none, and the band would only cost level 1
    // its writes: 1.43 -> 1.52 ms, profiles/r03/ab/ab4_band.txt)
    const bool want = c->sieve_band > 0 || (c->sieve_band == 0 && p.sieve <= kSieveMaxT16 / 2);
    if (t2 > p.sieve && fits && want) p.band = t2;
  }
  // the sieve's workgroup: 1,024 threads (auto), or on request two 512-thread
  // ones per CU when their LDS fits (C3: 6.86 vs 6.56 ms, level 1 3.51 vs
  // 3.44 ms and level 2 0.97 vs 0.80 ms over twice the flush blocks,
  // profiles/r04/ab/ab1_sieve_threads.txt)
  p.sieve_threads = kL1Threads;
  p.hist_u16 = p.l1_local ? (int)l1_hist_u16(p.key_format, p.n_buckets) : 0;
  if (p.sieve) {
    const bool band = p.band != 0;
    p.hist_u16 = sieve_lds(p.key_format, kL1Threads, p.n_buckets, false, band) > kL1LocalLds;
    const bool u16_2 = sieve_lds(p.key_format, kSieveThreads2, p.n_buckets, false, band) > kSieveLds2;
    const bool fits2 = sieve_lds(p.key_format, kSieveThreads2, p.n_buckets, u16_2, band) <= kSieveLds2;
    if (fits2 && c->sieve_threads == kSieveThreads2) {
      p.sieve_threads = kSieveThreads2;
      p.hist_u16 = u16_2;
    }
  }
  p.slot_bits = sieve_slot_bits(p.sieve_threads);
  if (!p.sieve) p.slot_bits = 3;
  static_assert(kStagesPerTile == 8, "non-sieve level-1 stages per tile = 2^3");
  p.n_slots1 = p.sieve ? p.n_tiles << p.slot_bits : p.n_stages;
}

// 5. derived counts and the bucket kernel's LDS
void plan_derived(const pdp_bound_config* c, Plan& p) {
  // the fix-up per privacy id where a wave's sketches (l0 pair entries, l0 *
  // linf row entries) fit its LDS slice; keep-all-rows plans (per-pair sums,
  // not row sketches) and larger bounds keep the fix-up bucket launches
  p.fix_ids = p.sieve && c->linf > 0 && (int64_t)c->l0 * (1 + (int64_t)c->linf) <= kFixIdsEntries;
  p.pair_slots = (int64_t)c->l0 << p.bucket_bits;
  // record segments of the range merge: the main launch's, and one per
  // fix-up bucket launch (the per-id fix-up lists its pairs flat, after them)
  p.buckets_out = p.sieve && !p.fix_ids ? (p.band ? 3 : 2) * p.n_buckets : p.n_buckets;
  p.l2_mult = 1;
  if (p.sieve) {
    // expected records of one (group of kL2GroupTiles tiles, super-bucket)
    const double per_group = (double)kL2GroupTiles * (double)kTileRows * ((double)p.sieve / 65536.0) /
                             (double)(p.n_supers > 0 ? p.n_supers : 1);
    int m = (int)(kL2Target / (per_group > 1.0 ? per_group : 1.0));
    const int m_max = kL2Threads / (kL2GroupTiles << p.slot_bits);  // one slot per level-2 thread
    const int cap = kSieveL2Groups < m_max ? kSieveL2Groups : m_max;
    p.l2_mult = m < 1 ? 1 : (m > cap ? cap : m);
  }
  if (p.algorithm == PDP_ALGO_BUCKETED) {  // candidate queues (key + row) per wave + pid hashes
    p.lds_bytes = ((p.lds_bytes + 7) & ~(int64_t)7) + (p.bucket_threads / 64) * kQueueCap * 12;
    p.lds_bytes += ((int64_t)8 << p.bucket_bits);  // {pid hash, sketch-maximum high half} per pid
  }
  if (p.merge == PDP_MERGE_RANGES) {
    // range r yields ceil(records_r / C) items + 1 sentinel, and a bucket
    // emits at most l0 * 2^bucket_bits records in all
    const int64_t recs = p.buckets_out * ((int64_t)c->l0 << p.bucket_bits);
    p.range_group = kRangeChunk;
    p.n_groups = recs / kRangeChunk + 2 * (int64_t)p.n_ranges + 1;
    p.fine_items = p.two_level ? recs / kRangeChunk + p.n_fine + 1 : 0;
  } else {
    p.n_ranges = 0;
    p.range_group = 0;
    p.n_groups = 0;
    p.two_level = 0;
    p.fine_items = 0;
  }
}

Plan make_plan_capped(const pdp_bound_config* c, int max_bucket_bits) {
  Plan p{};
  plan_buckets(c, max_bucket_bits, p);
  plan_merge(c, p);
  plan_keys(c, p);
  plan_sieve(c, p);
  plan_derived(c, p);
  return p;
}

// row stride of the per-tile bucket counts in buckets (KP.cstride): whole
// 16-byte rows of u16 pairs (tile-local level 1) or u32 counts, so
// k_gscan_sums reads eight or four buckets per lane
inline int64_t counts_stride(int64_t n_buckets) { return (n_buckets + 7) & ~(int64_t)7; }

}  // namespace

// kLdsBudget bounds the sketches alone; the pid-hash table (8 bytes per id),
// the wave queues and the range scratch come on top, and the bucket kernel
// cannot be launched with more than a workgroup's kLdsLimit: 4,096 ids of 28
// bytes (l0 = 1, linf = 2) or 2,048 of 60 (l0 = 3, linf = 1) went over it.
// Halve the bucket until the whole of it fits: lds_bytes is the dynamic
// request, and the kernel's static LDS (kBucketStaticLds) counts as well --
// 2,048 ids of 60 bytes under the atomic merge come to exactly kLdsLimit
// without it.
Plan make_plan(const pdp_bound_config* c) {
  Plan p = make_plan_capped(c, 63);
  while (p.algorithm == PDP_ALGO_BUCKETED && p.lds_bytes + kBucketStaticLds > kLdsLimit && p.bucket_bits > 4)
    p = make_plan_capped(c, p.bucket_bits - 1);
  return p;
}

Ws layout(const pdp_bound_config* c, const Plan& p) {
  Ws w{};
  uint64_t off = 0;
  w.err = off;
  off = align256(off + 16);
  if (p.algorithm == PDP_ALGO_GLOBAL_SKETCH) {
    const uint64_t slots = (uint64_t)c->n_privacy_ids * (uint64_t)c->l0;
    w.sketch = off; off = align256(off + slots * 8);
    w.cnt = off; off = align256(off + slots * 4);
    if (c->linf > 0) {
      w.rows = off; off = align256(off + slots * (uint64_t)c->linf * 8);
    } else {
      w.fsum = off; off = align256(off + slots * 8);  // double or int64
      w.nsum = off; off = align256(off + slots * 8);
      w.nsum2 = off; off = align256(off + slots * 8);
    }
  } else {
    const uint64_t n_counts = (uint64_t)counts_stride(p.n_buckets) * (uint64_t)p.n_tiles;
    const uint64_t n_chunks = ((uint64_t)p.n_buckets + kScanChunk - 1) / kScanChunk;
    const uint64_t n = (uint64_t)c->n_rows;
    w.counts_tm = off; off = align256(off + n_counts * 4);
    const bool u16 = p.hist_u16 != 0;
    if (p.l1_local && u16) { w.counts_tm2 = off; off = align256(off + n_counts * 4); }
    w.tile_over = off; off = align256(off + (uint64_t)p.n_tiles * 4);
    w.counts = off; off = align256(off + ((uint64_t)p.n_buckets + 1) * 4);  // bucket starts
    w.chunk_sums = off; off = align256(off + (n_chunks + 1) * 4);
    const uint64_t n_sc = ((uint64_t)p.n_tiles + kScanChunkTiles - 1) / kScanChunkTiles;
    const uint64_t n_grp = ((uint64_t)p.n_tiles + kL2GroupTiles - 1) / kL2GroupTiles;
    w.csum = off; off = align256(off + n_sc * (uint64_t)p.n_buckets * 4);
    w.gcur = off; off = align256(off + n_grp * (uint64_t)p.n_buckets * 4);
    w.super_base = off; off = align256(off + (uint64_t)(p.n_supers + 1) * 4);
    w.super_tm = off; off = align256(off + (uint64_t)p.n_tiles * p.n_supers * 4);
    w.super_off = off; off = align256(off + (uint64_t)p.n_tiles * p.n_supers * 4);
    const bool packed = (p.key_format == PDP_KEYS_PACKED || p.key_format == PDP_KEYS_PACKED_WIDE ||
                         p.key_format == PDP_KEYS_PACKED64) && p.super_bits > 0;
    const uint64_t kb1 = p.key_format == PDP_KEYS_COMPACT ? 4 : 8;  // level-1 key
    const uint64_t kb2 = (p.key_format == PDP_KEYS_WIDE || p.key_format == PDP_KEYS_PACKED_WIDE ||
                          p.key_format == PDP_KEYS_PACKED64) ? 8 : 4;  // level-2 key
    const bool rows2 = p.key_format != PDP_KEYS_PACKED64;  // PACKED64: the row rides in the key
    // level-1 records: stage blocks, or the sieve's per-tile flush blocks
    const uint64_t n1 = p.sieve ? (uint64_t)p.n_tiles * kSieveTileStride
                                : (p.l1_local ? (uint64_t)p.n_stages * kL1Rows : n);
    w.keys1 = off; off = align256(off + n1 * (packed ? 8 : kb1));
    if (!packed) { w.rows1 = off; off = align256(off + n1 * 4); }
    if (p.sieve) {  // the fix-up list reuses [keys1, end of rows1), at least 8 B per row
      if (off - w.keys1 < 8 * n) off = w.keys1 + align256(8 * n);
      w.fix_rec = w.keys1;
      w.fix_cap = (off - w.keys1) / 8;
    }
    if (p.l1_local) { w.soff = off; off = align256(off + (uint64_t)p.n_slots1 * (p.n_supers + 1) * 2); }
    if (p.sieve) {
      const uint64_t ids = (uint64_t)p.n_buckets << p.bucket_bits;
      w.sbase = off; off = align256(off + (uint64_t)p.n_slots1 * 4);
      w.unres_bits = off; off = align256(off + ids / 8);
      w.unres_list = off; off = align256(off + ids * 4);
      w.sctl = off; off = align256(off + 16);
      w.fix_cnt = off; off = align256(off + ((uint64_t)p.n_buckets + 1) * 4);
      w.fix_cur = off; off = align256(off + (uint64_t)p.n_buckets * 4);
      // listed buckets; per-id fix-up: {bucket, begin, end, id} of every id
      // over the row cap (their rows are distinct entries of the fix-up list)
      const uint64_t n_blist = p.fix_ids ? 4 * (w.fix_cap / kFixIdsRowCap + 1) : (uint64_t)p.n_buckets;
      w.fix_blist = off; off = align256(off + (n_blist + 1) * 4);
      if (p.fix_ids) {
        w.id_pos = off; off = align256(off + ids * 4);
        w.id_seg = off; off = align256(off + ids * 8);
        if (p.band) { w.id_seg2 = off; off = align256(off + ids * 8); }
        w.fix_ctl = off; off = align256(off + 16);
      }
      if (p.band) {  // the band lists; the second fix-up's unresolved ids and counts
        w.band = off; off = align256(off + (uint64_t)p.n_tiles * kBandTileStride * 8);
        w.band_cnt = off; off = align256(off + (uint64_t)p.n_tiles * 4);
        w.unres2_bits = off; off = align256(off + ids / 8);
        w.unres2_list = off; off = align256(off + ids * 4);
        w.sctl2 = w.sctl + 8;  // {count, rows} beside sctl's: pdp_bound_stats_async reads both with one copy
        w.fix_cnt2 = off; off = align256(off + ((uint64_t)p.n_buckets + 1) * 4);
        w.fix_cur2 = off; off = align256(off + (uint64_t)p.n_buckets * 4);
      }
    }
    if (p.super_bits > 0) {
      w.keys2 = off; off = align256(off + n * kb2);
      if (rows2) { w.rows2 = off; off = align256(off + n * 4); }
      else w.rows2 = w.keys2;  // unused
    } else {
      w.keys2 = w.keys1;
      w.rows2 = w.rows1;
    }
    w.cand_key = off; off = align256(off + n * kb2);
    w.cand_idx = off; off = align256(off + n * 4);
    if (p.merge == PDP_MERGE_RANGES) {
      const uint64_t recs = (uint64_t)(p.buckets_out + (p.fix_ids ? p.n_buckets : 0)) * ((uint64_t)c->l0 << p.bucket_bits);
      w.runs = off; off = align256(off + (uint64_t)p.buckets_out * (p.n_ranges + 1) * 4);
      w.rec_key = off; off = align256(off + recs * 8);
      if (c->flags & (PDP_ACC_SUM | PDP_SUM_PER_PARTITION)) { w.rec_f0 = off; off = align256(off + recs * 8); }
      if (c->flags & PDP_ACC_NSUM) { w.rec_f1 = off; off = align256(off + recs * 8); }
      if (c->flags & PDP_ACC_NSUM2) { w.rec_f2 = off; off = align256(off + recs * 8); }
      w.rr_items = off; off = align256(off + (uint64_t)p.n_groups * 16);
      w.rr_count = off; off = align256(off + 16);
      if (p.two_level) {  // fine-range counts, starts, cursors; records re-sorted by fine range
        const uint64_t nf = (uint64_t)p.n_fine;
        w.fine_total = off; off = align256(off + (nf + 1) * 4);
        w.fine_chunks = off; off = align256(off + (uint64_t)scan_chunk_sums_len((int64_t)nf) * 4);
        w.fine_cur = off; off = align256(off + nf * 4);
        w.stg_key = off; off = align256(off + recs * 8);
        if (w.rec_f0) { w.stg_f0 = off; off = align256(off + recs * 8); }
        if (w.rec_f1) { w.stg_f1 = off; off = align256(off + recs * 8); }
        if (w.rec_f2) { w.stg_f2 = off; off = align256(off + recs * 8); }
        w.fine_items = off; off = align256(off + (uint64_t)p.fine_items * 16);
        w.fine_count = off; off = align256(off + 16);
        const uint64_t F = (uint64_t)1 << (p.range_bits - kRangeBits);
        w.item_hist = off; off = align256(off + (uint64_t)p.n_groups * F * 4);
      }
    }
  }
  w.total = off;
  return w;
}

// PDP_DEBUG_CORRUPT_RECORDS deliberately corrupts the level-2 records: only
// accepted when the process asked for test hooks
bool test_hooks_enabled() {
  const char* v = std::getenv("PIPELINEDP_AMD_TEST_HOOKS");
  return v != nullptr && v[0] == '1';
}

// The positive integer in the test hook `name` (an environment variable), 0
// where it holds none or the process did not ask for test hooks; the caller
// bounds it.
long long test_hook(const char* name) {
  const char* e = test_hooks_enabled() ? std::getenv(name) : nullptr;
  const long long v = e != nullptr ? std::atoll(e) : 0;
  return v > 0 ? v : 0;
}

int validate(const pdp_bound_config* c) {
  if (c == nullptr) return set_error(PDP_E_INVALID, "config is NULL");
  if (c->n_rows < 0 || c->n_rows >= ((int64_t)1 << 32))
    return set_error(PDP_E_INVALID, "n_rows must be in [0, 2^32)");
  if (c->n_privacy_ids < 1 || c->n_privacy_ids >= ((int64_t)1 << 40))
    return set_error(PDP_E_INVALID, "n_privacy_ids must be in [1, 2^40)");
  if (c->n_partitions < 1 || c->n_partitions >= ((int64_t)1 << 32))
    return set_error(PDP_E_INVALID, "n_partitions must be in [1, 2^32)");
  if (c->l0 < 0 || c->l0 > PDP_MAX_L0)
    return set_error(PDP_E_UNSUPPORTED, "l0 out of supported range [0, PDP_MAX_L0]");
  if (c->linf < 0 || c->linf > PDP_MAX_LINF)
    return set_error(PDP_E_UNSUPPORTED, "linf out of supported range [0, PDP_MAX_LINF]");
  if (c->max_contributions < 0 || c->max_contributions > PDP_MAX_CONTRIBUTIONS)
    return set_error(PDP_E_UNSUPPORTED, "max_contributions out of supported range [0, PDP_MAX_CONTRIBUTIONS]");
  if (c->value_kind < PDP_VALUE_NONE || c->value_kind > PDP_VALUE_I64)
    return set_error(PDP_E_INVALID, "bad value_kind");
  if (c->value_kind != PDP_VALUE_I64 && (c->flags & PDP_SUM_INT))
    return set_error(PDP_E_INVALID, "PDP_SUM_INT requires int64 values");
  if (c->flags & PDP_SUM_INT) {
    // the kernels clip in int64 with (long long)bound, which C++ defines only
    // for a bound that is an int64: finite, integral, in [-2^63, 2^63)
    auto is_int64 = [](double b) {
      return std::isfinite(b) && b == std::floor(b) && b >= -9223372036854775808.0 && b < 9223372036854775808.0;
    };
    const bool per_partition = (c->flags & PDP_SUM_PER_PARTITION) != 0;
    if (per_partition ? !(is_int64(c->min_sum) && is_int64(c->max_sum))
                      : !(is_int64(c->min_value) && is_int64(c->max_value)))
      return set_error(PDP_E_UNSUPPORTED, per_partition
                                              ? "PDP_SUM_INT requires min_sum / max_sum that are int64 values"
                                              : "PDP_SUM_INT requires min_value / max_value that are int64 values");
  }
  if (c->algorithm < PDP_ALGO_AUTO || c->algorithm > PDP_ALGO_PAIR_TABLE)
    return set_error(PDP_E_INVALID, "bad algorithm");
  if (c->merge < PDP_MERGE_AUTO || c->merge > PDP_MERGE_RANGES)
    return set_error(PDP_E_INVALID, "bad merge");
  if (c->key_format < PDP_KEYS_AUTO || c->key_format > PDP_KEYS_PACKED64)
    return set_error(PDP_E_INVALID, "bad key_format");
  if (c->sieve_threads != 0 && c->sieve_threads != kSieveThreads2 && c->sieve_threads != kL1Threads)
    return set_error(PDP_E_INVALID, "sieve_threads must be 0, 512 or 1024");
  if (c->bucket_threads != 0 && c->bucket_threads != kBucketThreads / 2 && c->bucket_threads != kBucketThreads)
    return set_error(PDP_E_INVALID, "bucket_threads must be 0, 512 or 1024");
  if ((c->flags & PDP_DEBUG_CORRUPT_RECORDS) && !test_hooks_enabled())
    return set_error(PDP_E_INVALID, "PDP_DEBUG_CORRUPT_RECORDS is a test hook: set PIPELINEDP_AMD_TEST_HOOKS=1");
  if (pairs_mode(c)) return pairs_validate(c);
  if (make_plan(c).algorithm < 0)
    return set_error(PDP_E_UNSUPPORTED, "bucketed algorithm / range merge / compact keys infeasible for this l0/linf/U/P");
  return PDP_OK;
}

KP make_kp(const pdp_bound_config* c, const Plan& p) {
  KP k;
  k.n = c->n_rows;
  k.U = c->n_privacy_ids;
  k.P = c->n_partitions;
  k.l0 = c->l0;
  k.linf = c->linf;
  k.pk_bits = p.pk_bits;
  k.bucket_bits = p.bucket_bits;
  k.super_bits = p.super_bits;
  k.rand_shift = p.rand_shift;
  k.n_buckets = p.n_buckets;
  k.n_supers = p.n_supers;
  k.n_tiles = p.n_tiles;
  k.n_ranges = p.n_ranges;
  k.range_bits = p.range_bits;
  k.n_fine_ranges = p.n_fine;
  k.keys_vec = 0;
  k.n_slots1 = p.n_slots1;
  k.l2_group_mult = p.l2_mult;
  k.sieve_t32 = (uint32_t)p.sieve << 16;
  k.sieve_mark = p.sieve != 0;
  k.band_t32 = (uint32_t)p.band << 16;
  k.sieve_emit = p.band != 0;
  k.slot_bits = p.slot_bits;
  k.fix_cap = 0;  // set from the layout (Ws.fix_cap) where the fix-up runs
  k.row_shift = p.pk_bits + p.bucket_bits;
  k.fix_ids = 0;
  k.pk_mask = (1ULL << p.pk_bits) - 1;
  k.seed = c->seed;
  k.row_seed = derive_row_seed(c->seed);
  k.row_offset = c->row_offset;
  k.cstride = counts_stride(p.n_buckets);
  k.clip = ClipParams{c->min_value, c->max_value, c->middle, c->min_sum, c->max_sum, c->flags};
  return k;
}

int check_ws(const pdp_bound_config* cfg, const void* workspace, uint64_t workspace_bytes, Plan* p, Ws* w) {
  const int rc = validate(cfg);
  if (rc != PDP_OK) return rc;
  if (pairs_mode(cfg)) {
    if (workspace == nullptr || workspace_bytes < pairs_workspace_bytes(cfg))
      return set_error(PDP_E_WORKSPACE, "workspace too small (see pdp_bound_workspace_bytes)");
    return PDP_OK;
  }
  *p = make_plan(cfg);
  *w = layout(cfg, *p);
  if (workspace == nullptr || workspace_bytes < w->total)
    return set_error(PDP_E_WORKSPACE, "workspace too small (see pdp_bound_workspace_bytes)");
  return PDP_OK;
}

}  // namespace pdp

using namespace pdp;

extern "C" {

int pdp_bound_plan(const pdp_bound_config* cfg, pdp_bound_plan_info* info) {
  const int rc = validate(cfg);
  if (rc != PDP_OK) return rc;
  if (info == nullptr) return set_error(PDP_E_INVALID, "info is NULL");
  if (pairs_mode(cfg)) {
    *info = pdp_bound_plan_info{};
    info->algorithm = PDP_ALGO_PAIR_TABLE;
    info->pk_bits = bits_for(cfg->n_partitions);
    return PDP_OK;
  }
  const Plan p = make_plan(cfg);
  info->algorithm = p.algorithm;
  info->bucket_bits = p.bucket_bits;
  info->rand_shift = p.rand_shift;
  info->pk_bits = p.pk_bits;
  info->n_buckets = p.algorithm == PDP_ALGO_BUCKETED ? p.n_buckets : 0;
  info->n_tiles = p.n_tiles;
  info->lds_bytes = p.algorithm == PDP_ALGO_BUCKETED ? p.lds_bytes : 0;
  info->merge = p.merge;
  info->n_ranges = p.n_ranges;
  info->range_group = p.range_group;
  info->key_format = p.key_format;
  info->sieve = p.sieve;
  info->band = p.band;
  info->sieve_threads = p.sieve ? p.sieve_threads : 0;
  info->bucket_threads = p.bucket_threads;
  info->hist_u16 = p.algorithm == PDP_ALGO_BUCKETED && p.l1_local ? p.hist_u16 : 0;
  info->fix_ids = p.algorithm == PDP_ALGO_BUCKETED ? p.fix_ids : 0;
  return PDP_OK;
}

int pdp_bound_workspace_bytes(const pdp_bound_config* cfg, uint64_t* bytes) {
  const int rc = validate(cfg);
  if (rc != PDP_OK) return rc;
  if (bytes == nullptr) return set_error(PDP_E_INVALID, "bytes is NULL");
  *bytes = pairs_mode(cfg) ? pairs_workspace_bytes(cfg) : layout(cfg, make_plan(cfg)).total;
  return PDP_OK;
}

}  // extern "C"
