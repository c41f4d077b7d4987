// pdp_quantiles.hip — PERCENTILE: one DP quantile tree per partition (gfx950).
//
// Replaces QuantileCombiner (pipeline_dp/combiners.py:590-669), whose tree is
// PyDP's QuantileTree; the algorithm is restated in DESIGN.md §3 ("PERCENTILE")
// and pdp_quantile_plan.h holds the tree's shape.  A node's raw count is the
// number of kept rows whose leaf lies in the node's leaf range, so a
// partition's tree is kept as the ascending array of its kept rows' 16-bit
// leaf codes and a count is the difference of two lower bounds in it.
//
//   pairs_mark_kept_rows   (pdp_pairs.hip) the rows the pair table kept, their
//                          partitions and the partitions' offsets; NaN values
//                          are dropped there
//   k_q_keys               per row the sort keys: leaf code and partition
//                          (n_partitions for a row that is not kept)
//   tile_sort_pass         (pdp_segments.h) stable 8-bit passes, the two leaf
//                          digits first, then the partition's: (partition, leaf)
//   k_q_pack               the kept prefix as uint16 leaf codes
//   k_quantile_metrics     one wave per kept partition, 16 lanes (the children
//                          of the current node) per rank, four ranks a round
//   k_q_merge              several ranks: the owner's merge of the ranks'
//                          ascending runs, one array per partition again
// No floating-point atomic; two runs on the same input give the same bytes.
#include "pdp_quantile_plan.h"
#include "pdp_segments.h"

namespace pdp {
namespace {

constexpr uint32_t kQuantileSlot = PDP_QUANTILE_SLOT;

// min(L - 1, floor((clamp(v) - lo) / (hi - lo) * L)), each operation rounded on its own
template <int VK>
__device__ __forceinline__ unsigned q_leaf(const void* __restrict__ value, int64_t i, double lo, double hi) {
#pragma clang fp contract(off)
  double v = VK == PDP_VALUE_I64 ? (double)((const long long*)value)[i] : ((const double*)value)[i];
  v = v < lo ? lo : (v > hi ? hi : v);
  const double f = floor((v - lo) / (hi - lo) * (double)kQtLeaves);
  return f >= (double)(kQtLeaves - 1) ? (unsigned)(kQtLeaves - 1) : (unsigned)f;
}

template <int VK>
__global__ void __launch_bounds__(kBlock) k_q_keys(int64_t n, int64_t P, const unsigned* __restrict__ mark,
                                                   const void* __restrict__ value, double lo, double hi,
                                                   unsigned* __restrict__ leaf, unsigned* __restrict__ part) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    const unsigned k = mark[i];
    const bool kept = k != kPairsNotKept && (int64_t)k < P;
    part[i] = kept ? k : (unsigned)P;  // rows that are not kept sort behind every partition
    leaf[i] = kept ? q_leaf<VK>(value, i, lo, hi) : 0u;
  }
}

// the sorted key goes with the other key column of its record
struct QEmit {
  const unsigned* other_in;
  unsigned *key_out, *other_out;
  __device__ void operator()(int64_t i, unsigned k, unsigned pos) const {
    const unsigned o = other_in[i];  // read before the first store: the two may alias for all the compiler knows
    key_out[pos] = k;
    other_out[pos] = o;
  }
};

// kept rows come first in the sorted order: total = off[P] of them
__global__ void __launch_bounds__(kBlock) k_q_pack(int64_t n, int64_t P, const unsigned* __restrict__ off,
                                                   const unsigned* __restrict__ leaf, uint16_t* __restrict__ out) {
  const int64_t total = (int64_t)off[P] < n ? (int64_t)off[P] : n;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; j < total; j += stride) out[j] = (uint16_t)leaf[j];
}

// first position of the ascending a[0..m) whose code is >= x (x <= 65536)
__device__ __forceinline__ unsigned q_lower_bound(const uint16_t* __restrict__ a, unsigned m, unsigned x) {
  unsigned lo = 0, hi = m;
  while (lo < hi) {
    const unsigned mid = (lo + hi) >> 1;
    if ((unsigned)a[mid] < x) lo = mid + 1; else hi = mid;
  }
  return lo;
}

struct QRanks {
  double r[PDP_MAX_QUANTILES];
};

// The walk of one rank by the 16 lanes gbase .. gbase + 15 of a wave; lane
// gbase + c looks after child c of the current node.  Every lane of the wave
// calls it (the shuffles and ballots need all of them); a group that has no
// rank (`active` false) draws no noise, and each group reads only its own 16
// bits of a ballot.  All lanes of a group return the same value.  fp64
// throughout, every operation rounded on its own, in the order of DESIGN.md §3
// ("PERCENTILE", the walk).
__device__ __forceinline__ double q_walk(const uint16_t* __restrict__ seg, unsigned m, double lo, double hi, double r,
                                         bool active, int c, int gbase, const pdp_noise_params& np, uint64_t seed,
                                         int64_t node_base) {
#pragma clang fp contract(off)
  double a = lo, b = hi;
  unsigned prefix = 0;  // the current node's place within its level
  bool done = !active;
  unsigned span = (unsigned)kQtLeaves;  // leaves below a node of the level
  int64_t first = 0;                    // index of the level's first node
  for (int level = 1; level <= kQtHeight; ++level) {
    span /= kQtBranch;
    first = first * kQtBranch + 1;
    const unsigned pos = prefix * kQtBranch + (unsigned)c;
    double cnt = 0.0;
    if (!done) {
      const unsigned x0 = pos * span;
      const unsigned raw = q_lower_bound(seg, m, x0 + span) - q_lower_bound(seg, m, x0);
      const int64_t node = first + (int64_t)pos;
      const double nz = secure_add_noise(np, (double)raw, seed, node_base + node - 1, kQuantileSlot);
      cnt = nz > 0.0 ? nz : 0.0;
    }
    // the children's counts added left to right; `mine` = the sum up to and including child c
    double partial = 0.0, mine = 0.0;
    for (int k = 0; k < kQtBranch; ++k) {
      partial += __shfl(cnt, gbase + k, 64);
      if (k == c) mine = partial;
    }
    const double total = partial;
    const bool live = !done && total > 0.0;  // the same in all lanes of the group
    const unsigned reach = (unsigned)(__ballot(live && mine / total >= r - 1e-6) >> gbase) & 0xFFFFu;
    const unsigned some = (unsigned)(__ballot(live && cnt > 0.0) >> gbase) & 0xFFFFu;
    // the first child that reaches the rank, else (rounding) the last one with a count
    const int pick = reach ? __ffs((int)reach) - 1 : (some ? 31 - __clz((int)some) : 0);
    const double cnt_c = __shfl(cnt, gbase + pick, 64);
    const double upto_c = __shfl(mine, gbase + pick, 64);
    if (live) {
      const double t = (r - (upto_c - cnt_c) / total) / (cnt_c / total);
      const double t0 = 0.0 < t ? t : 0.0;  // a NaN (a child without a count) becomes 0
      r = 1.0 < t0 ? 1.0 : t0;
      const double w = b - a;
      const double na = a + (double)pick * w / 16.0;
      const double nb = a + (double)(pick + 1) * w / 16.0;
      a = na;
      b = nb;
      prefix = prefix * kQtBranch + (unsigned)pick;
    } else {
      done = true;
    }
  }
  return (1.0 - r) * a + r * b;
}

__global__ void __launch_bounds__(kBlock) k_quantile_metrics(const uint16_t* __restrict__ leaves,
                                                             const unsigned* __restrict__ off, int64_t P, double lo,
                                                             double hi, QRanks ranks, int n_ranks, pdp_noise_params np,
                                                             const int64_t* __restrict__ index, int64_t n_kept,
                                                             const int64_t* __restrict__ n_kept_dev,
                                                             int64_t partition_offset, double* __restrict__ out,
                                                             uint64_t seed) {
  int64_t n = n_kept;
  if (n_kept_dev != nullptr) {
    const int64_t dv = *n_kept_dev;
    n = dv < n ? dv : n;
  }
  const int lane = (int)(threadIdx.x & 63);
  const int grp = lane >> 4, c = lane & 15, gbase = grp << 4;
  const int64_t wstride = (int64_t)gridDim.x * (kBlock / 64);
  for (int64_t i = (int64_t)blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6); i < n; i += wstride) {
    const int64_t p = index[i];  // wave-uniform
    if (p < 0 || p >= P) continue;
    const unsigned s0 = off[p], s1 = off[p + 1];
    if (s1 > off[P]) continue;  // offsets that are no scan: nothing is read past the list's end
    const unsigned m = s1 > s0 ? s1 - s0 : 0u;
    const uint16_t* seg = leaves + s0;
    const int64_t node_base = (partition_offset + p) * kQtNodes;
    for (int j0 = 0; j0 < n_ranks; j0 += 4) {
      const int j = j0 + grp;
      const bool active = j < n_ranks;
      const double r = ranks.r[active ? j : 0];
      const double v = q_walk(seg, m, lo, hi, r, active, c, gbase, np, seed, node_base);
      if (active && c == 0) out[i * n_ranks + j] = v;
    }
  }
}

// ------------------------------------------------ merge of the ranks' trees --
// Under a process group a partition's owner receives one ascending run of
// leaf codes per source rank (parallel.exchange_quantile_leaves) and needs one
// ascending array per partition:
//   scan_u32 (run_off)  run-major scan of the counts: where run s of partition p starts in `runs`
//   k_q_merge_cols      per partition the sum of its runs' counts
//   scan_u32 (offsets)  the merged arrays' offsets
//   k_q_merge           one element per thread: its place is its own index in
//                       its run plus, per other run of the partition, the
//                       number of codes that go before it -- codes <= x in
//                       the runs before its own, codes < x in the runs after
// The places are a permutation (ties go by run, then by index): every slot has
// one writer, no atomic, no LDS, and two calls give the same bytes.
struct QMergeWs {
  uint64_t run_off, chunks, total;
};

inline QMergeWs qmerge_layout(int32_t n_runs, int64_t P) {
  QMergeWs w{};
  const uint64_t cells = (uint64_t)n_runs * (uint64_t)P;
  uint64_t off = 0;
  w.run_off = off; off = align256(off + (cells + 1) * 4);
  w.chunks = off; off = align256(off + (uint64_t)scan_chunk_sums_len((int64_t)cells) * 4);  // the longer of the two scans
  w.total = off;
  return w;
}

int qmerge_check(int32_t n_runs, int64_t P) {
  if (n_runs < 1 || n_runs > PDP_MAX_QUANTILE_RUNS)
    return set_error(PDP_E_UNSUPPORTED, "n_runs outside [1, PDP_MAX_QUANTILE_RUNS]");
  if (P < 1) return set_error(PDP_E_INVALID, "n_partitions must be >= 1");
  if ((int64_t)n_runs * P >= ((int64_t)1 << 31))
    return set_error(PDP_E_UNSUPPORTED, "quantile merge: n_runs * n_partitions must be < 2^31");
  return PDP_OK;
}

__global__ void __launch_bounds__(kBlock) k_q_merge_cols(int64_t P, int n_runs, const unsigned* __restrict__ counts,
                                                         unsigned* __restrict__ col) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p < P; p += stride) {
    unsigned s = 0;
    for (int r = 0; r < n_runs; ++r) s += counts[(int64_t)r * P + p];
    col[p] = s;
  }
}

// number of codes <= x in the ascending a[0..m)
__device__ __forceinline__ unsigned q_upper_bound(const uint16_t* __restrict__ a, unsigned m, unsigned x) {
  return q_lower_bound(a, m, x + 1);
}

// Every read of `runs` and every store to `leaves` stays below n: counts whose
// scan disagrees with n (or wraps) shorten the runs that are read and drop the
// stores that would fall outside, nothing else.
__global__ void __launch_bounds__(kBlock) k_q_merge(const uint16_t* __restrict__ runs, int64_t n, int64_t P,
                                                    int n_runs, const unsigned* __restrict__ run_off,
                                                    const unsigned* __restrict__ off, uint16_t* __restrict__ leaves) {
  const int64_t cells = (int64_t)n_runs * P;
  const unsigned lim = (int64_t)run_off[cells] < n ? run_off[cells] : (unsigned)n;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < (int64_t)lim; e += stride) {
    // the cell (run s, partition p) that holds e: the last one that starts at or before e
    int64_t lo = 0, hi = cells;
    while (lo < hi) {
      const int64_t mid = (lo + hi) >> 1;
      if ((int64_t)run_off[mid] <= e) lo = mid + 1; else hi = mid;
    }
    const int64_t cell = lo > 0 ? lo - 1 : 0;
    const int s = (int)(cell / P);
    const int64_t p = cell - (int64_t)s * P;
    const unsigned x = runs[e];
    const unsigned own = run_off[cell];
    uint64_t at = (uint64_t)off[p] + ((unsigned)e >= own ? (unsigned)e - own : 0u);
    for (int r = 0; r < n_runs; ++r) {
      if (r == s) continue;
      const int64_t c = (int64_t)r * P + p;
      const unsigned b0 = run_off[c] < lim ? run_off[c] : lim;
      const unsigned b1 = run_off[c + 1] < lim ? run_off[c + 1] : lim;
      const unsigned m = b1 > b0 ? b1 - b0 : 0u;
      at += r < s ? q_upper_bound(runs + b0, m, x) : q_lower_bound(runs + b0, m, x);
    }
    if (at < (uint64_t)n) leaves[at] = (uint16_t)x;
  }
}

int quantile_check(const pdp_bound_config* cfg) {
  pdp_bound_plan_info info;
  const int rc = pdp_bound_plan(cfg, &info);
  if (rc != PDP_OK) return rc;
  if (info.algorithm != PDP_ALGO_PAIR_TABLE)
    return set_error(PDP_E_UNSUPPORTED,
                     "quantile leaves read the pair table: set pdp_bound_config.algorithm = PDP_ALGO_PAIR_TABLE");
  const char* msg = nullptr;
  const int rs = q_check_shape(cfg->n_rows, cfg->n_partitions, &msg);
  return rs == PDP_OK ? PDP_OK : set_error(rs, msg);
}

QWs quantile_layout(const pdp_bound_config* cfg) {
  return qlayout(pairs_vector_workspace_bytes(cfg, 0), cfg->n_rows, cfg->n_partitions, scan_chunk_sums_len);
}

}  // namespace
}  // namespace pdp

using namespace pdp;

extern "C" {

int pdp_quantile_workspace_bytes(const pdp_bound_config* cfg, uint64_t* bytes) {
  const int rc = quantile_check(cfg);
  if (rc != PDP_OK) return rc;
  if (bytes == nullptr) return set_error(PDP_E_INVALID, "bytes is NULL");
  *bytes = quantile_layout(cfg).total;
  return PDP_OK;
}

int pdp_reduce_quantile_leaves(const pdp_bound_config* cfg, const int64_t* privacy_id, const int64_t* partition_key,
                               const uint8_t* pk_allowed, const void* value, int32_t value_kind, double min_value,
                               double max_value, void* workspace, uint64_t workspace_bytes, uint16_t* leaves,
                               uint32_t* offsets, void* stream) {
  int rc = quantile_check(cfg);
  if (rc != PDP_OK) return rc;
  if (value_kind != PDP_VALUE_F64 && value_kind != PDP_VALUE_I64)
    return set_error(PDP_E_INVALID, "value_kind must be PDP_VALUE_F64 or PDP_VALUE_I64");
  const char* msg = nullptr;
  if (const int rr = q_check_range(min_value, max_value, &msg); rr != PDP_OK) return set_error(rr, msg);
  const QWs w = quantile_layout(cfg);
  if (workspace == nullptr || workspace_bytes < w.total)
    return set_error(PDP_E_WORKSPACE, "workspace too small (see pdp_quantile_workspace_bytes)");
  if (offsets == nullptr) return set_error(PDP_E_INVALID, "offsets is NULL");
  const int64_t n = cfg->n_rows, P = cfg->n_partitions;
  if (n > 0 && leaves == nullptr) return set_error(PDP_E_INVALID, "leaves is NULL");
  if (n > 0 && (partition_key == nullptr || (privacy_id == nullptr && !cfg->rows_are_units)))
    return set_error(PDP_E_INVALID, "key columns are NULL");
  if (n > 0 && value == nullptr) return set_error(PDP_E_INVALID, "value is NULL");
  if ((((uintptr_t)value) & 7) || (((uintptr_t)offsets) & 3) || (((uintptr_t)leaves) & 1))
    return set_error(PDP_E_INVALID, "value, offsets and leaves must be aligned to their element size");

  char* ws = (char*)workspace;
  hipStream_t st = (hipStream_t)stream;
  PairsKeptRows kr;
  rc = pairs_mark_kept_rows(cfg, privacy_id, partition_key, pk_allowed,
                            value_kind == PDP_VALUE_F64 ? (const double*)value : nullptr, ws, &kr, st);
  if (rc != PDP_OK) return rc;
  PDP_HIP_CHECK(hipMemcpyAsync(offsets, kr.off, ((uint64_t)P + 1) * 4, hipMemcpyDeviceToDevice, st));
  if (n == 0) return PDP_OK;
  unsigned* leaf[2] = {(unsigned*)(ws + w.leaf0), (unsigned*)(ws + w.leaf1)};
  unsigned* part[2] = {(unsigned*)(ws + w.part0), (unsigned*)(ws + w.part1)};
  unsigned* hist = (unsigned*)(ws + w.hist);
  unsigned* chunks = (unsigned*)(ws + w.chunks);
  rc = launch("k_q_keys", value_kind == PDP_VALUE_I64 ? k_q_keys<PDP_VALUE_I64> : k_q_keys<PDP_VALUE_F64>,
              dim3(grid_for(n)), dim3(kBlock), 0, st, n, P, kr.mark, value, min_value, max_value, leaf[0], part[0]);
  if (rc != PDP_OK) return rc;
  int cur = 0;
  for (int shift = 0; shift < 16; shift += 8) {  // the leaf code, low digit first
    rc = tile_sort_pass<8, kQSortTile>("k_q_hist", "k_q_scatter", n, 256, shift, leaf[cur],
                                       QEmit{part[cur], leaf[cur ^ 1], part[cur ^ 1]}, hist, chunks, st);
    if (rc != PDP_OK) return rc;
    cur ^= 1;
  }
  for (int shift = 0; shift < w.part_bits; shift += 8) {  // then the partition: equal partitions keep the leaf order
    rc = tile_sort_pass<8, kQSortTile>("k_q_hist", "k_q_scatter", n, 256, shift, part[cur],
                                       QEmit{leaf[cur], part[cur ^ 1], leaf[cur ^ 1]}, hist, chunks, st);
    if (rc != PDP_OK) return rc;
    cur ^= 1;
  }
  return launch("k_q_pack", k_q_pack, dim3(grid_for(n)), dim3(kBlock), 0, st, n, P, kr.off, leaf[cur], leaves);
}

int pdp_quantile_merge_workspace_bytes(int32_t n_runs, int64_t n_partitions, uint64_t* bytes) {
  const int rc = qmerge_check(n_runs, n_partitions);
  if (rc != PDP_OK) return rc;
  if (bytes == nullptr) return set_error(PDP_E_INVALID, "bytes is NULL");
  *bytes = qmerge_layout(n_runs, n_partitions).total;
  return PDP_OK;
}

int pdp_merge_quantile_leaves(const uint16_t* runs, int64_t n_leaves, const uint32_t* run_counts, int32_t n_runs,
                              int64_t n_partitions, void* workspace, uint64_t workspace_bytes, uint16_t* leaves,
                              uint32_t* offsets, void* stream) {
  int rc = qmerge_check(n_runs, n_partitions);
  if (rc != PDP_OK) return rc;
  if (n_leaves < 0) return set_error(PDP_E_INVALID, "n_leaves < 0");
  if (n_leaves >= ((int64_t)1 << 31)) return set_error(PDP_E_UNSUPPORTED, "quantile merge: n_leaves must be < 2^31");
  const QMergeWs w = qmerge_layout(n_runs, n_partitions);
  if (workspace == nullptr || workspace_bytes < w.total)
    return set_error(PDP_E_WORKSPACE, "workspace too small (see pdp_quantile_merge_workspace_bytes)");
  if (run_counts == nullptr || offsets == nullptr) return set_error(PDP_E_INVALID, "run_counts or offsets is NULL");
  if (n_leaves > 0 && (runs == nullptr || leaves == nullptr)) return set_error(PDP_E_INVALID, "runs or leaves is NULL");
  if ((((uintptr_t)run_counts) & 3) || (((uintptr_t)offsets) & 3) || (((uintptr_t)workspace) & 3) ||
      (((uintptr_t)runs) & 1) || (((uintptr_t)leaves) & 1))
    return set_error(PDP_E_INVALID, "run_counts, offsets, workspace, runs and leaves must be aligned to their element size");
  if (n_leaves > 0 && runs == leaves) return set_error(PDP_E_INVALID, "runs and leaves must not alias");

  char* ws = (char*)workspace;
  hipStream_t st = (hipStream_t)stream;
  const int64_t P = n_partitions, cells = (int64_t)n_runs * P;
  unsigned* run_off = (unsigned*)(ws + w.run_off);
  unsigned* chunks = (unsigned*)(ws + w.chunks);
  PDP_HIP_CHECK(hipMemcpyAsync(run_off, run_counts, (uint64_t)cells * 4, hipMemcpyDeviceToDevice, st));
  rc = launch("k_q_merge_cols", k_q_merge_cols, dim3(grid_for(P)), dim3(kBlock), 0, st, P, (int)n_runs, run_counts,
              offsets);
  if (rc != PDP_OK) return rc;
  rc = scan_u32(run_off, cells, chunks, st);
  if (rc != PDP_OK) return rc;
  rc = scan_u32(offsets, P, chunks, st);
  if (rc != PDP_OK) return rc;
  if (n_leaves == 0) return PDP_OK;
  return launch("k_q_merge", k_q_merge, dim3(grid_for(n_leaves)), dim3(kBlock), 0, st, runs, n_leaves, P, (int)n_runs,
                run_off, offsets, leaves);
}

int pdp_quantile_metrics(const uint16_t* leaves, const uint32_t* offsets, int64_t n_partitions, double min_value,
                         double max_value, const double* ranks, int32_t n_ranks, const pdp_noise_params* noise,
                         const int64_t* index, int64_t n_kept, const int64_t* n_kept_dev, int64_t partition_offset,
                         double* out, uint64_t seed, void* stream) {
  const char* msg = nullptr;
  if (const int rr = q_check_ranks(ranks, n_ranks, &msg); rr != PDP_OK) return set_error(rr, msg);
  if (const int rr = q_check_range(min_value, max_value, &msg); rr != PDP_OK) return set_error(rr, msg);
  if (n_partitions < 1) return set_error(PDP_E_INVALID, "n_partitions must be >= 1");
  if (n_kept < 0) return set_error(PDP_E_INVALID, "n_kept must be >= 0");
  const int rc = check_noise(noise);
  if (rc != PDP_OK) return rc;
  if (n_kept == 0) return PDP_OK;
  if (offsets == nullptr || index == nullptr || out == nullptr) return set_error(PDP_E_INVALID, "NULL argument");
  // (leaves may be NULL: no row was kept, every partition is empty and nothing is read from it)
  QRanks qr{};
  for (int j = 0; j < n_ranks; ++j) qr.r[j] = ranks[j];
  const unsigned grid = grid_for(n_kept * 64, 2048);  // one wave per kept partition
  return launch("k_quantile_metrics", k_quantile_metrics, dim3(grid), dim3(kBlock), 0, (hipStream_t)stream, leaves,
                offsets, n_partitions, min_value, max_value, qr, (int)n_ranks, *noise, index, n_kept, n_kept_dev,
                partition_offset, out, seed);
}

}  // extern "C"
