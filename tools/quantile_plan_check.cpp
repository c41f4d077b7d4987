// quantile_plan_check.cpp — walks the host-side planning code of the PERCENTILE
// path (pipelinedp_amd/csrc/pdp_quantile_plan.h) on its own: tree constants,
// workspace layout at its size edges, argument checks.  No HIP, nothing loaded
// into Python; meant to be built with the sanitizers on:
//
//   c++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all \
//       -I include tools/quantile_plan_check.cpp -o quantile_plan_check && ./quantile_plan_check
//
// Prints "quantile plan ok" and exits 0, or names the first failed check.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <vector>

#include "../pipelinedp_amd/csrc/pdp_quantile_plan.h"

using namespace pdp;

#define CHECK(cond)                                                        \
  do {                                                                     \
    if (!(cond)) {                                                         \
      std::fprintf(stderr, "%s:%d: check failed: %s\n", __FILE__, __LINE__, #cond); \
      return 1;                                                            \
    }                                                                      \
  } while (0)

// the device scan's chunk sums (pdp_scan.hip: 4,096 words a chunk, one spare)
static int64_t scan_len(int64_t n) { return (n + 4095) / 4096 + 1; }

static int check_layout(uint64_t base, int64_t n, int64_t P) {
  const QWs w = qlayout(base, n, P, scan_len);
  const uint64_t col = q_align256((uint64_t)n * 4);
  CHECK(w.leaf0 == q_align256(base) && w.leaf0 % 256 == 0);
  CHECK(w.leaf1 == w.leaf0 + col && w.part0 == w.leaf1 + col && w.part1 == w.part0 + col);
  CHECK(w.hist == w.part1 + col);
  CHECK(w.n_tiles == (n + kQSortTile - 1) / kQSortTile);
  CHECK(w.chunks >= w.hist + (256 * (uint64_t)w.n_tiles + 1) * 4 && w.chunks % 256 == 0);
  CHECK(w.total >= w.chunks + (uint64_t)scan_len(256 * w.n_tiles) * 4 && w.total % 256 == 0);
  CHECK(w.part_bits >= 1 && w.part_bits <= 31);
  CHECK(((int64_t)1 << w.part_bits) >= P + 1);  // the sentinel P has a key
  // every region can be written to its last byte inside [0, total): touch a model of it
  std::vector<unsigned char> model((size_t)(w.total - q_align256(base)), 0);
  const uint64_t o = q_align256(base);
  for (uint64_t r : {w.leaf0, w.leaf1, w.part0, w.part1})
    if (n > 0) model[(size_t)(r - o + (uint64_t)n * 4 - 1)] = 1;
  model[(size_t)(w.hist - o + (256 * (uint64_t)w.n_tiles + 1) * 4 - 1)] = 1;
  model[(size_t)(w.chunks - o + (uint64_t)scan_len(256 * w.n_tiles) * 4 - 1)] = 1;
  return 0;
}

int main() {
  // tree shape: computed, and equal to the figures the documentation quotes
  CHECK(kQtLeaves == 65536 && kQtFirstLeaf == 4369 && kQtNodes == 69904);
  CHECK(qt_level_first(0) == 0 && qt_level_first(1) == 1 && qt_level_first(2) == 17 && qt_level_first(3) == 273);
  int64_t nodes = 0;
  for (int level = 1; level <= kQtHeight; ++level) {
    nodes += qt_pow(level);
    CHECK(qt_span(level) * qt_pow(level) == kQtLeaves);
    CHECK(qt_level_first(level + 1) == qt_level_first(level) + qt_pow(level));
  }
  CHECK(nodes == kQtNodes);
  // the largest Philox counter: (partitions) * nodes + node - 1 stays in int64
  CHECK((((int64_t)1 << 31) * kQtNodes + kQtNodes) > 0);

  // layout at its edges: no rows, one row, around a tile, the largest shapes (sizes only, 32 MiB model at most)
  for (int64_t n : {(int64_t)0, (int64_t)1, (int64_t)kQSortTile - 1, (int64_t)kQSortTile, (int64_t)kQSortTile + 1,
                    (int64_t)100000})
    for (int64_t P : {(int64_t)1, (int64_t)2, (int64_t)255, (int64_t)256, (int64_t)65535, (int64_t)65536})
      for (uint64_t base : {(uint64_t)0, (uint64_t)1, (uint64_t)255, (uint64_t)256, (uint64_t)4097})
        if (check_layout(base, n, P) != 0) return 1;
  {  // the largest accepted shape: arithmetic only
    const int64_t n = ((int64_t)1 << 31) - 1, P = ((int64_t)1 << 31) - 2;
    const char* msg = nullptr;
    CHECK(q_check_shape(n, P, &msg) == PDP_OK);
    const QWs w = qlayout(((uint64_t)1 << 40) + 3, n, P, scan_len);
    CHECK(w.total > w.leaf0 && w.total - w.leaf0 < ((uint64_t)1 << 36));
    CHECK(w.part_bits == 31 && w.n_tiles == (n + kQSortTile - 1) / kQSortTile);
  }

  // argument checks
  const char* msg = nullptr;
  CHECK(q_check_shape(-1, 1, &msg) == PDP_E_INVALID && msg != nullptr);
  CHECK(q_check_shape(0, 0, &msg) == PDP_E_INVALID);
  CHECK(q_check_shape((int64_t)1 << 31, 1, &msg) == PDP_E_UNSUPPORTED);
  CHECK(q_check_shape(1, ((int64_t)1 << 31) - 1, &msg) == PDP_E_UNSUPPORTED);
  CHECK(q_check_shape(0, 1, &msg) == PDP_OK);
  const double inf = std::numeric_limits<double>::infinity(), nan = std::nan("");
  CHECK(q_check_range(0.0, 1.0, &msg) == PDP_OK && q_check_range(-1e9, 1e9, &msg) == PDP_OK);
  CHECK(q_check_range(1.0, 1.0, &msg) == PDP_E_INVALID && q_check_range(2.0, 1.0, &msg) == PDP_E_INVALID);
  CHECK(q_check_range(nan, 1.0, &msg) == PDP_E_INVALID && q_check_range(0.0, nan, &msg) == PDP_E_INVALID);
  CHECK(q_check_range(-inf, 1.0, &msg) == PDP_E_INVALID && q_check_range(0.0, inf, &msg) == PDP_E_INVALID);
  CHECK(q_check_range(-1.7e308, 1.7e308, &msg) == PDP_E_INVALID);  // the width overflows
  std::vector<double> ranks(PDP_MAX_QUANTILES, 0.5);
  ranks.front() = 0.0;
  ranks.back() = 1.0;
  CHECK(q_check_ranks(ranks.data(), PDP_MAX_QUANTILES, &msg) == PDP_OK && q_check_ranks(ranks.data(), 1, &msg) == PDP_OK);
  CHECK(q_check_ranks(ranks.data(), 0, &msg) == PDP_E_UNSUPPORTED);
  CHECK(q_check_ranks(ranks.data(), PDP_MAX_QUANTILES + 1, &msg) == PDP_E_UNSUPPORTED);  // checked before any read
  CHECK(q_check_ranks(nullptr, 3, &msg) == PDP_E_INVALID);
  for (double bad : {-1e-9, 1.0000001, nan, inf}) {
    std::vector<double> r = {0.5, bad};
    CHECK(q_check_ranks(r.data(), 2, &msg) == PDP_E_INVALID);
    CHECK(q_check_ranks(r.data(), 1, &msg) == PDP_OK);  // only the first n_ranks are read
  }
  CHECK(q_rounds(1) == 1 && q_rounds(4) == 1 && q_rounds(5) == 2 && q_rounds(PDP_MAX_QUANTILES) == 16);
  std::puts("quantile plan ok");
  return 0;
}
