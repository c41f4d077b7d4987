// pdp_bound_plan.h -- what the bounding sources (pdp_bound*.hip) share on the
// host: the constants of the plan and the kernels, Plan / Ws / KP /
// PairRecords, the typed view of a workspace region (at), the planner's
// functions (pdp_bound_planner.hip) and the entry points of the passes that
// have their own file.
#pragma once

#include "pdp_internal.h"

namespace pdp {

constexpr int kPartThreads = 512;
// rows per thread and LDS stage of the level-1 scatter / level-2 window
constexpr int kL1Threads = 1024;
constexpr int kL1Items = 8;
constexpr int kL1Rows = kL1Threads * kL1Items;  // rows per level-1 LDS stage
constexpr int kL2Items = 16;
// level 2: two 8-wave workgroups per CU need <= 128 VGPRs (MI355X_MICROARCH.md
// register table): the kernel takes 121-123 with 16 records per thread;
// loading a stage ahead (157 VGPRs, one workgroup per CU) cost 1 ms at C3
constexpr int kL2Threads = 512;
constexpr int kL2Rows = kL2Threads * kL2Items;  // records per level-2 LDS stage
// tiles per level-2 workgroup (k_scatter_l2, k_gscan_cursors)
constexpr int kL2GroupTiles = 16;
constexpr int kScanWaves = 16;
constexpr int kScanTiles = 16;  // tiles per wave in the level-2 cursor scans; multiple of kL2GroupTiles
constexpr int kScanChunkTiles = kScanWaves * kScanTiles;
static_assert(kScanTiles % kL2GroupTiles == 0, "group starts must fall inside a wave's tiles");
constexpr int kTileRowBits = 16;
constexpr int64_t kTileRows = (int64_t)1 << kTileRowBits;
constexpr int kStagesPerTile = (int)(kTileRows / kL1Rows);  // level-1 blocks per tile
constexpr int kL2Runs = kL2GroupTiles * kStagesPerTile;  // level-1 runs per level-2 workgroup
constexpr int kUnroll = 8;
constexpr int kBucketThreads = 1024;
constexpr int64_t kLdsBudget = 124 * 1024;  // per-pid state; + range scratch + wave queues <= 160 KiB
// 512-thread bucket workgroups: per-pid state <= 56 KiB.  With the range
// scratch (<= 4 KiB at 512 ranges), 8 wave queues (12 KiB) and the pid hashes
// (8 bytes per id) two workgroups share one CU's 160 KiB where the ids are
// few enough (C3: 1,024 ids of 40 bytes, about 64 KiB each); with many small ids
// (l0 = 1, linf = 2: 2,048 of 28 bytes and 16 KiB of hashes) one workgroup
// exceeds 80 KiB and runs alone -- make_plan enforces only kLdsLimit
constexpr int64_t kLdsBudget2 = 56 * 1024;
// one workgroup's LDS on gfx950: the bucket kernel's dynamic request plus its
// static LDS (kBucketStaticLds: k_bucket_bound's ccount, with room) stays within it
constexpr int64_t kLdsLimit = 160 * 1024;
constexpr int64_t kBucketStaticLds = 64;
constexpr int kMinRandomBits = 24;
constexpr int64_t kMaxBuckets = 36 * 1024;  // u32 histogram in 144 KiB of LDS
constexpr int kMaxSupers = 128;   // destinations of a level-1 scatter
constexpr int64_t kSingleLevelMax = 64;      // buckets partitioned by one level
constexpr int kRangeBits = 11;                // partitions per merge range = 2048
constexpr int kRangeParts = 1 << kRangeBits;
constexpr int kMaxRanges = kBucketThreads;    // per-bucket range histogram <= one block scan
// More partitions than kMaxRanges ranges of 2^kRangeBits: the bucket kernel
// groups kept pairs by coarse ranges of 2^range_bits partitions (<= kCoarseRanges
// of them), k_split_* re-sort each coarse range's records into its
// 2^kRangeBits-partition ranges, k_fine_reduce sums them (two-level merge)
constexpr int kCoarseRanges = 256;
constexpr int kRangeThreads = 1024;  // k_range_plan workgroups
// range-reduce work item: the records of one partition range from a run of
// consecutive buckets, cut at bucket boundaries every kRangeChunk records
// (k_range_plan), so a Zipf-hot range spreads over many workgroups and a cold
// one is a single item
constexpr int64_t kRangeChunk = 8192;
constexpr unsigned kRangeDirect = 256;        // records below which a workgroup adds them directly
// k_range_reduce / k_fine_reduce workgroups: 512 threads (two per CU by their
// 68 KB of LDS: 16 waves, not 8): C3 k_range_reduce 0.275 -> 0.195 ms, C4
// k_fine_reduce 0.574 -> 0.540 (1,024: 0.212 / 0.537; profiles/r05/ab/ab12_merge_threads.txt)
constexpr int kReduceThreads = 512;
constexpr int kSplitThreads = 512;  // k_split_count / k_split_scatter workgroups
constexpr size_t kRangeLds = kRangeParts * (3 * 8 + 2 * 4) + kReduceThreads * (8 + 4) + (kReduceThreads / 64 + 1) * 4;
constexpr int kQueueCap = 128;                // per-wave candidate queue (bucket kernel)
// per-id sieve fix-up (k_fix_ids, Plan.fix_ids): one wave per unresolved
// privacy id, its pair sketch (l0 entries) and row sketches (l0 * linf) in a
// per-wave LDS slice of kFixIdsEntries u64 (C2 (8, 2): 24, C4/C5 (4, 2): 12,
// C3 (2, 1): 4); an id with more fix-up rows than kFixIdsRowCap goes to a
// listed bucket launch instead.  A wave takes 64 rows per trip and two passes,
// about 1 us per 64 rows when the rows sit in L2: 4,096 rows cost ~60 us,
// what a bucket workgroup spends on its fixed LDS set-up and slot sweeps, and
// past that the bucket's 8 waves on one id's rows win
constexpr int kFixIdsEntries = 32;
constexpr unsigned kFixIdsRowCap = 4096;
constexpr int kFixIdsThreads = 256;
constexpr int kScanItems = 16;
constexpr int kScanChunk = kBlock * kScanItems;

// LDS of one level-1 stage, of the sieve's level-1 stage and the flush-slot
// bits of a sieve workgroup of `threads`: sizes of StageLds / SieveShape,
// defined beside those templates (pdp_bound.hip)
size_t l1_stage_bytes(int key_format);
size_t sieve_stage_bytes(int key_format, int threads);
int sieve_slot_bits(int threads);
// tile-local level 1 bucket counts in LDS: u32 per bucket when they fit,
// else two u16 per word, flushed every half tile (32,768 rows: no carry) to
// counts_tm (first half) and counts_tm2 (second half)
inline int64_t l1_hist_bytes(int64_t n_buckets, bool u16) { return ((u16 ? 2 : 4) * n_buckets + 15) / 16 * 16; }
constexpr int kSieveThreads2 = 512;  // the sieve's second workgroup shape (SieveShape, Plan.sieve_threads)
// a tile's flush blocks lie back to back from tile * kSieveTileStride, its
// band list at tile * kBandTileStride
// (strides padded by 4 KiB measured 6 % slower at C3, profiles/r05/ab/ab1_l1_placement.txt)
// non-temporal loads (ld_nt) of the columns level 1 streams and of the band
// lists k_band_scan streams (C3 0.277 -> 0.255 ms); measured neutral or worse
// and not used: k_scatter_l1_local's key loads (C4 +0.03 ms), level 2's run
// loads and the bucket kernel's record stream (profiles/r05/ab/ab5_nt_loads.txt)
constexpr int64_t kSieveTileStride = kTileRows;
constexpr int64_t kBandTileStride = kTileRows;
// tile groups per level-2 workgroup with the sieve, at most: the plan takes
// as many as keep a workgroup's expected records (tiles x candidates per tile
// / super-buckets) within one LDS window (kL2Target), since a second window
// holding a few hundred records costs as much latency as a full one; and no
// more than one level-1 slot per level-2 thread
constexpr int kSieveL2Groups = 4;
// the side band (Plan.band): rows with t <= pair hash < t2 = 2t leave level 1
// as (privacy id << 32 | row) in a per-tile list, through a per-wave LDS queue
// written out 64 entries at a time; the fix-up reads that list instead of the
// whole privacy-id column, and only a privacy id with fewer than l0 distinct
// pairs below t2 still needs the rescan
constexpr int kBandQueue = 128;
inline int64_t sieve_band_lds(int threads) { return (threads / 64) * kBandQueue * 8; }
// LDS of a sieve workgroup: stage, bucket counts (u32, or u16 pairs), band queues
inline int64_t sieve_lds(int key_format, int threads, int64_t n_buckets, bool u16, bool band) {
  return ((int64_t)sieve_stage_bytes(key_format, threads) + 7) / 8 * 8 + l1_hist_bytes(n_buckets, u16) +
         (band ? sieve_band_lds(threads) : 0);
}

struct Plan {
  int algorithm;   // PDP_ALGO_*
  int pk_bits;
  int bucket_bits;
  int super_bits;
  int rand_shift;
  int64_t n_buckets;
  int64_t n_supers;
  int64_t n_tiles;
  int64_t lds_bytes;
  int merge;            // PDP_MERGE_* (bucketed)
  int n_ranges;         // PDP_MERGE_RANGES: ceil(P / 2^range_bits)
  int range_bits;       // partitions per merge range of the bucket kernel (kRangeBits, or coarse)
  int two_level;        // range_bits > kRangeBits: coarse ranges, then k_split_* / k_fine_*
  int64_t n_fine;       // two-level: ceil(P / 2^kRangeBits)
  int64_t fine_items;   // two-level: upper bound on the k_fine_reduce work items
  int64_t range_group;  // records per range-reduce work item (kRangeChunk)
  int64_t n_groups;     // upper bound on the range-reduce work items (+ one sentinel per range)
  int key_format;       // PDP_KEYS_WIDE / PDP_KEYS_COMPACT (bucketed)
  int l1_local;         // tile-local level 1 (k_scatter_l1_local / k_scatter_l2_local), no histogram pass
  int64_t n_stages;     // level-1 stages of kL1Rows rows
  int sieve;            // threshold sieve: t = sieve / 2^16 (0 = off); k_sieve_l1 instead of k_scatter_l1_local
  int band;             // side band: t2 = band / 2^16 (0 = off; else 2 * sieve, <= 1/2)
  int64_t n_slots1;     // level-1 blocks (stages, or sieve flush slots: n_tiles << slot_bits)
  int64_t buckets_out;  // buckets of pair records: n_buckets, x2 with the sieve (fix-up after), x3 with the band
  int l2_mult;          // tile groups per level-2 workgroup (1 without the sieve)
  int sieve_threads;    // k_sieve_l1 workgroup: 1,024 or 512 threads (SieveShape)
  int bucket_threads;   // k_bucket_bound workgroup: 1,024 or 512 threads (half-size buckets)
  int slot_bits;        // level-1 blocks per tile = 2^slot_bits (kStagesPerTile, or SieveShape::kSlots)
  int hist_u16;         // tile-local level 1 counts buckets in u16 halves (counts_tm / counts_tm2)
  int fix_ids;          // sieve fix-up per privacy id (k_fix_ids) instead of by bucket launches
  int64_t pair_slots;   // pair records of one bucket's block: l0 << bucket_bits
};

struct Ws {
  // common
  uint64_t err;
  // global path
  uint64_t sketch, cnt, rows, fsum, nsum, nsum2;
  // bucketed path
  uint64_t counts_tm, counts, chunk_sums, super_base, super_tm, super_off, keys1, rows1, keys2, rows2;
  uint64_t csum, gcur;  // level-2 cursor scans: per tile chunk, per tile group (x n_buckets)
  uint64_t cand_key, cand_idx;  // bucket kernel: B1's candidate list (record-local key, row)
  uint64_t soff;                // tile-local level 1: per stage, super-bucket run starts (u16)
  uint64_t counts_tm2;          // tile-local level 1, u16 counts: second half-tile bucket counts
  // threshold sieve: flush-block starts (u32 per slot), unresolved privacy
  // ids (bitmap + list), {unresolved count, fix-up rows}, fix-up rows per
  // bucket (-> starts) and their write cursors; the fix-up row list itself
  // reuses keys1 (dead after level 2), its bucket-ordered records keys2/rows2
  uint64_t sbase, unres_bits, unres_list, sctl, fix_cnt, fix_cur;
  // the fix-up's (id << 32 | row) list: the level-1 region (keys1, and rows1
  // right after it for COMPACT records), dead after level 2; fix_cap entries
  // (>= n_rows: every list holds distinct rows)
  uint64_t fix_rec, fix_cap;
  // side band: per-tile (pid << 32 | row) lists and their lengths; the ids
  // still unresolved after the band fix-up (bitmap, list, {count, rows}) and
  // their rescan's per-bucket counts / cursors
  uint64_t band, band_cnt, unres2_bits, unres2_list, sctl2, fix_cnt2, fix_cur2;
  uint64_t fix_blist;  // fix-up bucket launches: {count, buckets holding fix-up rows...}
  // per-id fix-up: list position of an unresolved id (valid for listed ids
  // only), {start, end} of a listed id's fix-up rows per list position for
  // the first and the second list, {unused, fix-up pairs}
  uint64_t id_pos, id_seg, id_seg2, fix_ctl;
  uint64_t tile_over;  // tile-local level 1: per tile, the bucket holding all 65,536 of its rows (else ~0)
  // bucketed PDP_MERGE_RANGES: pair records per bucket block, grouped by range
  uint64_t runs, rec_key, rec_f0, rec_f1, rec_f2;
  uint64_t rr_items, rr_count;  // range-reduce work items (uint4) and their count
  // two-level merge: fine-range totals / starts (+ scan scratch), write cursors,
  // the records re-sorted by fine range, fine work items and their count
  uint64_t fine_total, fine_chunks, fine_cur, stg_key, stg_f0, stg_f1, stg_f2, fine_items, fine_count;
  uint64_t item_hist;  // two-level: per coarse work item, its records per fine range (k_split_count)
  uint64_t total;
};

struct KP {  // kernel parameters
  int64_t n, U, P;
  int l0, linf;
  int pk_bits, bucket_bits, super_bits, rand_shift;
  int64_t n_buckets, n_supers, n_tiles;
  int n_ranges;
  int range_bits;
  int64_t n_fine_ranges;  // two-level merge: ceil(P / 2^kRangeBits)
  int keys_vec;  // privacy_id / partition_key columns are 16-byte aligned
  uint64_t pk_mask, seed, row_seed;
  int64_t row_offset;
  int64_t cstride;  // row stride of counts_tm / counts_tm2 in buckets: n_buckets rounded up to 8
  ClipParams clip;
  int64_t n_slots1;     // level-1 blocks read by level 2 (Plan.n_slots1)
  int l2_group_mult;    // tile groups per level-2 workgroup
  uint32_t sieve_t32;   // threshold sieve: candidate rows have pair_hash < sieve_t32 (0 = off)
  int sieve_mark;       // bucket kernel: mark privacy ids with < l0 candidate pairs unresolved
  uint32_t band_t32;    // side band: level 1 lists rows with sieve_t32 <= pair_hash < band_t32 (0 = off)
  int sieve_emit;       // bucket kernel (main launch, band on): unresolved ids' candidate rows -> fix_rec
  int slot_bits;        // level-1 blocks per tile = 2^slot_bits (Plan.slot_bits)
  int64_t fix_cap;      // sieve: entries the fix-up row list (fix_rec, Ws.fix_rec) holds
  int row_shift;        // PACKED64 level-2 records: the row's first bit (pk_bits + bucket_bits)
  int fix_ids;          // bucket kernel, listed launch of the per-id fix-up: blist holds {bucket, begin, end, id}
};

struct PairRecords {  // PDP_MERGE_RANGES output of the bucket kernel
  unsigned* runs;                // [n_ranges + 1][run_stride] run starts within the bucket block (range-major)
  int64_t run_stride;            // buckets_out: one column per output bucket
  unsigned long long* key;       // (partition << 32) | count
  double* f0;                    // sum (int64 bits with PDP_SUM_INT)
  double* f1;                    // normalized sum
  double* f2;                    // normalized sum of squares
  // per-id fix-up: its kept pairs, a flat list of *flat_n records from
  // flat_base on (after the buckets' blocks), added by the reduce kernels
  unsigned* flat_n;
  int64_t flat_base, flat_cap;
};

// The workspace region at byte offset `off` (a field of Ws) as a T*; at_opt:
// NULL for a region the layout left out (offset 0: only the error word is there)
template <class T> inline T* at(char* ws, uint64_t off) { return (T*)(ws + off); }
template <class T> inline const T* at(const char* ws, uint64_t off) { return (const T*)(ws + off); }
template <class T> inline T* at_opt(char* ws, uint64_t off) { return off ? at<T>(ws, off) : nullptr; }

inline PairRecords pair_records(char* ws, const Ws& w, const Plan& p) {
  PairRecords rec{};
  if (w.runs) {
    rec.runs = at<unsigned>(ws, w.runs);
    rec.run_stride = p.buckets_out;
    rec.key = at<unsigned long long>(ws, w.rec_key);
    rec.f0 = at_opt<double>(ws, w.rec_f0);
    rec.f1 = at_opt<double>(ws, w.rec_f1);
    rec.f2 = at_opt<double>(ws, w.rec_f2);
    if (p.fix_ids) {
      rec.flat_n = at<unsigned>(ws, w.fix_ctl) + 1;
      rec.flat_cap = p.n_buckets * p.pair_slots;
      rec.flat_base = rec.flat_cap;
    }
  }
  return rec;
}

// pdp_bound_planner.hip -- what a call runs on, from its config alone: the
// checks, the plan (infeasible: algorithm < 0), the workspace layout and the
// kernel parameters; check_ws: validate + plan + layout + the workspace's size
bool test_hooks_enabled();             // PIPELINEDP_AMD_TEST_HOOKS=1
long long test_hook(const char* name);  // a hook's positive integer, else 0 (always 0 without test hooks)
int validate(const pdp_bound_config* c);
Plan make_plan(const pdp_bound_config* c);
Ws layout(const pdp_bound_config* c, const Plan& p);
KP make_kp(const pdp_bound_config* c, const Plan& p);
int check_ws(const pdp_bound_config* cfg, const void* workspace, uint64_t workspace_bytes, Plan* p, Ws* w);

// pdp_bound_merge.hip -- PDP_MERGE_RANGES: the pair records of every bucket
// (p.buckets_out of them) summed per partition
int launch_merge(const KP& kp0, const Plan& p, hipStream_t st, char* ws, const Ws& w,
                 const pdp_partition_accumulators& acc);

}  // namespace pdp
