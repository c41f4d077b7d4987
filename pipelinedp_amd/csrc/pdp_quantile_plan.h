// pdp_quantile_plan.h — host-side planning of the PERCENTILE path
// (pdp_quantiles.hip): the quantile tree's shape, the workspace layout of the
// leaf sort and the argument checks that need no device.  Plain C++ with no
// HIP type in it, so that tools/quantile_plan_check.cpp can build it on its own
// (under the address and undefined-behaviour sanitizers) and walk its edges.
#pragma once

#include <stdint.h>

#include <cmath>

#include "../../include/pipelinedp_amd.h"

namespace pdp {

// ------------------------------------------------------------- tree shape --
// Height 4, branching factor 16 (the defaults of the quantile tree the
// reference's QuantileCombiner builds).  The root is node 0 and is never
// counted; the children of node i are i * B + 1 ... i * B + B.
constexpr int kQtHeight = 4;
constexpr int kQtBranch = 16;

constexpr int64_t qt_pow(int e) { return e <= 0 ? 1 : (int64_t)kQtBranch * qt_pow(e - 1); }
// index of the first node of level `level` (0 = the root): 1 + B + ... + B^(level - 1)
constexpr int64_t qt_level_first(int level) { return (qt_pow(level) - 1) / (kQtBranch - 1); }

constexpr int64_t kQtLeaves = qt_pow(kQtHeight);                              // 65,536
constexpr int64_t kQtFirstLeaf = qt_level_first(kQtHeight);                   // 4,369
constexpr int64_t kQtNodes = qt_level_first(kQtHeight + 1) - 1;               // 69,904 counted nodes
static_assert(kQtLeaves <= 65536, "leaf codes are 16-bit");
static_assert(kQtBranch * 4 == 64, "one wave walks four ranks, 16 lanes (children) each");

// leaves below one node of `level` (1 ... H)
constexpr int64_t qt_span(int level) { return qt_pow(kQtHeight - level); }

// ------------------------------------------------------- workspace layout --
constexpr int kQSortTile = 2048;  // records per tile of the stable tile sort (pdp_segments.h)

struct QWs {
  uint64_t leaf0, leaf1, part0, part1;  // u32[n_rows] each: the sort's two key columns, ping and pong
  uint64_t hist, chunks;                // the tile sort's digit table and its scan's chunk sums
  uint64_t total;
  int64_t n_tiles;
  int part_bits;                        // bits of the partition key (the value n_partitions = not kept)
};

inline uint64_t q_align256(uint64_t x) { return (x + 255) & ~(uint64_t)255; }

inline int q_bits_for(int64_t n) {  // smallest b >= 1 with 2^b >= n
  int b = 1;
  while (b < 63 && ((int64_t)1 << b) < n) ++b;
  return b;
}

// The leaf sort's regions behind `base` bytes (the pair table's workspace and
// its kept-row marks).  scan_len(m) = words of chunk sums a device scan of m
// words needs (scan_chunk_sums_len).
inline QWs qlayout(uint64_t base, int64_t n_rows, int64_t n_partitions, int64_t (*scan_len)(int64_t)) {
  QWs w{};
  const uint64_t n = (uint64_t)n_rows;
  w.n_tiles = (n_rows + kQSortTile - 1) / kQSortTile;
  w.part_bits = q_bits_for(n_partitions + 1);
  const uint64_t hist_len = 256 * (uint64_t)w.n_tiles;
  uint64_t off = q_align256(base);
  w.leaf0 = off; off = q_align256(off + n * 4);
  w.leaf1 = off; off = q_align256(off + n * 4);
  w.part0 = off; off = q_align256(off + n * 4);
  w.part1 = off; off = q_align256(off + n * 4);
  w.hist = off; off = q_align256(off + (hist_len + 1) * 4);
  w.chunks = off; off = q_align256(off + (uint64_t)scan_len((int64_t)hist_len) * 4);
  w.total = off;
  return w;
}

// --------------------------------------------------------- argument checks --
// 0, or a PDP_E_* code with *msg set
inline int q_check_shape(int64_t n_rows, int64_t n_partitions, const char** msg) {
  if (n_rows < 0) { *msg = "n_rows < 0"; return PDP_E_INVALID; }
  if (n_partitions < 1) { *msg = "n_partitions must be >= 1"; return PDP_E_INVALID; }
  if (n_rows >= ((int64_t)1 << 31)) { *msg = "quantile leaves: n_rows must be < 2^31"; return PDP_E_UNSUPPORTED; }
  if (n_partitions >= ((int64_t)1 << 31) - 1) {
    *msg = "quantile leaves: n_partitions must be < 2^31 - 1";
    return PDP_E_UNSUPPORTED;
  }
  return PDP_OK;
}

inline int q_check_range(double lo, double hi, const char** msg) {
  if (!std::isfinite(lo) || !std::isfinite(hi) || !(lo < hi) || !std::isfinite(hi - lo)) {
    *msg = "quantiles need finite min_value < max_value with a finite width";
    return PDP_E_INVALID;
  }
  return PDP_OK;
}

inline int q_check_ranks(const double* ranks, int32_t n_ranks, const char** msg) {
  if (n_ranks < 1 || n_ranks > PDP_MAX_QUANTILES) {
    *msg = "n_ranks outside [1, PDP_MAX_QUANTILES]";
    return PDP_E_UNSUPPORTED;
  }
  if (ranks == nullptr) { *msg = "ranks is NULL"; return PDP_E_INVALID; }
  for (int32_t j = 0; j < n_ranks; ++j)
    if (!(ranks[j] >= 0.0 && ranks[j] <= 1.0)) { *msg = "every rank must lie in [0, 1]"; return PDP_E_INVALID; }
  return PDP_OK;
}

// rounds of four ranks one wave walks
inline int q_rounds(int32_t n_ranks) { return (n_ranks + 3) / 4; }

}  // namespace pdp
