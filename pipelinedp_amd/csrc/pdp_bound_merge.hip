// pdp_bound_merge.hip -- PDP_MERGE_RANGES of the BUCKETED path (pdp_bound.hip
// maps the paths): the bucket kernels' pair records summed per partition, by
// partition ranges in LDS (k_range_*), or for many partitions in two levels
// (k_split_*, k_fine_*).
#include "pdp_bound_keys.h"

namespace pdp {
namespace {

// PDP_MERGE_RANGES work items.  Range r's records, taken bucket-major, are cut
// into items at bucket boundaries: a new item starts after the bucket that
// holds record position k * kRangeChunk (k >= 1), so every item holds about
// kRangeChunk records or one bucket's run, a Zipf-hot range spreads over many
// workgroups and a cold range is one item.  Range r appends its K_r =
// ceil(total_r / C) items plus a sentinel at a base taken with one atomicAdd
// (ranges land in any order); entry k + 1 holds item k's end.  Entry:
// {r | sentinel << 31, first bucket, first record position within the range}.
// last_ids (the band's second fix-up): its id count; 0 leaves the last
// `last_buckets` buckets (that launch's record segment) empty, so they are
// not read
__global__ void __launch_bounds__(kRangeThreads) k_range_plan(KP kp, const unsigned* __restrict__ runs,
                                                              uint4* __restrict__ items,
                                                              unsigned* __restrict__ n_items,
                                                              const unsigned* __restrict__ last_ids,
                                                              int64_t last_buckets) {
  __shared__ unsigned wsum[kRangeThreads / 64 + 1];
  __shared__ unsigned s_base;
  const int r = blockIdx.x;
  const int64_t stride = kp.n_buckets;  // range-major: row r is contiguous over buckets
  const int64_t n_buckets = last_ids != nullptr && *last_ids == 0u ? kp.n_buckets - last_buckets : kp.n_buckets;
  auto len_of = [&](int64_t b) -> unsigned {
    if (b >= n_buckets) return 0u;
    const unsigned* run = runs + r * stride + b;
    return run[stride] - run[0];
  };
  unsigned total = 0;
  for (int64_t c = 0; c < n_buckets; c += blockDim.x) {
    unsigned t;
    block_excl_scan(len_of(c + threadIdx.x), wsum, &t);
    total += t;
    __syncthreads();
  }
  if (total == 0) return;  // block-uniform: no items
  const unsigned C = (unsigned)kRangeChunk;
  const unsigned K = (total + C - 1) / C;
  if (threadIdx.x == 0) s_base = atomicAdd(n_items, K + 1);
  __syncthreads();
  const unsigned base = s_base;
  if (threadIdx.x == 0) items[base] = make_uint4((unsigned)r, 0u, 0u, 0u);
  if (threadIdx.x == 0 && total % C != 0)
    items[base + K] = make_uint4((unsigned)r | 0x80000000u, (unsigned)n_buckets, total, 0u);
  unsigned carry = 0;
  for (int64_t c = 0; c < n_buckets; c += blockDim.x) {
    const int64_t b = c + threadIdx.x;
    const unsigned len = len_of(b);
    unsigned t;
    const unsigned ex = carry + block_excl_scan(len, wsum, &t);
    if (len > 0) {
      // items k >= 1 with k * C in (ex, ex + len] start after this bucket
      const unsigned e = ex + len;
      for (unsigned k = ex / C + 1; k * C <= e; ++k)
        items[base + k] = make_uint4((unsigned)r | (k == K ? 0x80000000u : 0u), (unsigned)(b + 1), e, 0u);
    }
    carry += t;
    __syncthreads();
  }
}

// PDP_MERGE_RANGES: one workgroup per work item (k_range_plan) sums its
// records of partitions [r*2^11, (r+1)*2^11) in LDS, then adds the partial
// sums with coalesced device atomics (an item of few records adds them
// directly).
// workgroup -> work item: i * p mod n for the prime p = 2^31 - 1 > n (a
// bijection on [0, n)), so the many items of a Zipf-hot range, which k_range_plan
// lists together, run spread over the launch instead of side by side (their
// device atomics go to the same partitions)
__device__ __forceinline__ unsigned item_order(unsigned i, unsigned n) {
  return (unsigned)(((uint64_t)i * 2147483647ull) % (uint64_t)n);
}

// The per-id fix-up's kept pairs (PairRecords.flat_n of them from flat_base
// on: a few thousand, in no order) straight into the accumulators, a
// grid-stride share per workgroup of the reduce launch -- the first few
// workgroups take them all, the others read the count and go on.
__device__ __forceinline__ void add_flat_pairs(const KP& kp, const PairRecords& rec,
                                               const pdp_partition_accumulators& acc, unsigned* err) {
  if (rec.flat_n == nullptr) return;
  const int flags = kp.clip.flags;
  int64_t n = *rec.flat_n;
  if (n > rec.flat_cap) n = rec.flat_cap;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t o = rec.flat_base + i;
    const unsigned long long key = rec.key[o];
    const int64_t p = (int64_t)(key >> 32);
    if (p >= kp.P) {  // malformed workspace: flagged, skipped
      atomicOr(err, 1u);
      continue;
    }
    PairSums ps{(long long)(uint32_t)key, 0, 0.0, 0.0, 0.0};
    if (flags & (PDP_ACC_SUM | PDP_SUM_PER_PARTITION)) {
      if (flags & PDP_SUM_INT) ps.isum = __double_as_longlong(rec.f0[o]);
      else ps.fsum = rec.f0[o];
    }
    if (flags & PDP_ACC_NSUM) ps.nsum = rec.f1[o];
    if (flags & PDP_ACC_NSUM2) ps.nsum2 = rec.f2[o];
    add_pair_to_partition(acc, p, ps, flags);
  }
}

__global__ void __launch_bounds__(kReduceThreads) k_range_reduce(KP kp, PairRecords rec, const uint4* __restrict__ items,
                                                               const unsigned* __restrict__ n_items,
                                                               pdp_partition_accumulators acc, unsigned* err) {
  extern __shared__ unsigned long long smem[];
  double* s0 = (double*)smem;               // [kRangeParts] sum
  double* s1 = s0 + kRangeParts;            // normalized sum
  double* s2 = s1 + kRangeParts;            // normalized sum of squares
  unsigned long long* start = (unsigned long long*)(s2 + kRangeParts);  // [kReduceThreads]
  unsigned* pc = (unsigned*)(start + kReduceThreads);  // [kRangeParts] kept pairs
  unsigned* cn = pc + kRangeParts;                    // [kRangeParts] row count
  unsigned* pre = cn + kRangeParts;                   // [kReduceThreads] run prefix
  unsigned* wsum = pre + kReduceThreads;              // block-scan scratch
  add_flat_pairs(kp, rec, acc, err);
  const unsigned n_it = *n_items;
  if (blockIdx.x >= n_it) return;  // grid is an upper bound on the item count
  const unsigned iw = item_order(blockIdx.x, n_it);
  const uint4 it = items[iw];
  if (it.x >> 31) return;  // sentinel
  const uint4 nx = items[iw + 1];
  const int r = (int)it.x;
  const int64_t b_lo = it.y, b_hi = nx.y;
  const unsigned item_total = nx.z - it.z;
  if (item_total == 0) return;
  const int flags = kp.clip.flags;
  const bool f0 = flags & (PDP_ACC_SUM | PDP_SUM_PER_PARTITION), f1 = flags & PDP_ACC_NSUM,
             f2 = flags & PDP_ACC_NSUM2, sum_int = flags & PDP_SUM_INT;
  const int64_t p0 = (int64_t)r << kRangeBits;
  const int64_t n_slots = (int64_t)kp.l0 << kp.bucket_bits;
  const bool direct = item_total < kRangeDirect;  // few records: straight into the accumulators
  if (!direct) {
    for (int t = threadIdx.x; t < kRangeParts; t += blockDim.x) {
      pc[t] = 0;
      cn[t] = 0;
      s0[t] = 0.0;
      s1[t] = 0.0;
      s2[t] = 0.0;
    }
  }
  // buckets in batches of one per thread: run starts, block scan, then the
  // batch's records, RR per thread in flight (their run lookups and loads
  // issued before the atomics)
  constexpr int RR = 4;
  for (int64_t bb = b_lo; bb < b_hi; bb += blockDim.x) {
    int64_t nb = b_hi - bb;
    if (nb > blockDim.x) nb = blockDim.x;
    unsigned len = 0;
    if (threadIdx.x < nb) {
      const int64_t b = bb + threadIdx.x;
      const unsigned* run = rec.runs + r * rec.run_stride + b;
      const unsigned s = run[0];
      len = run[rec.run_stride] - s;
      start[threadIdx.x] = (unsigned long long)(b * n_slots + s);
    }
    unsigned total;
    const unsigned ex = block_excl_scan(len, wsum, &total);
    pre[threadIdx.x] = ex;
    __syncthreads();
    for (unsigned i0 = threadIdx.x; i0 < total; i0 += RR * blockDim.x) {
      uint64_t idx[RR];
      bool ok[RR];
#pragma unroll
      for (int u = 0; u < RR; ++u) {
        const unsigned i = i0 + u * blockDim.x;
        ok[u] = i < total;
        int lo = 0, hi = (int)nb - 1;  // last run with pre <= i
        while (ok[u] && lo < hi) {
          const int mid = (lo + hi + 1) >> 1;
          if (pre[mid] <= i) lo = mid;
          else hi = mid - 1;
        }
        idx[u] = ok[u] ? start[lo] + (i - pre[lo]) : 0;
      }
      unsigned long long key[RR];
      double v0[RR], v1[RR], v2[RR];
#pragma unroll
      for (int u = 0; u < RR; ++u) {
        key[u] = ok[u] ? rec.key[idx[u]] : 0ull;
        v0[u] = (ok[u] && f0) ? rec.f0[idx[u]] : 0.0;
        v1[u] = (ok[u] && f1) ? rec.f1[idx[u]] : 0.0;
        v2[u] = (ok[u] && f2) ? rec.f2[idx[u]] : 0.0;
      }
#pragma unroll
      for (int u = 0; u < RR; ++u) {
        if (!ok[u]) continue;
        // a record outside this item's range (malformed workspace): flagged, skipped
        if ((int64_t)(key[u] >> 32) >= kp.P || (key[u] >> 32) - (uint64_t)p0 >= (uint64_t)kRangeParts) {
          atomicOr(err, 1u);
          continue;
        }
        if (direct) {
          const int64_t p = (int64_t)(key[u] >> 32);
          atomicAdd((unsigned long long*)(acc.privacy_id_count + p), 1ull);
          if (acc.count) atomicAdd((unsigned long long*)(acc.count + p), (unsigned long long)(uint32_t)key[u]);
          if (f0) {
            if (sum_int) atomicAdd((unsigned long long*)acc.sum + p, (unsigned long long)__double_as_longlong(v0[u]));
            else unsafeAtomicAdd((double*)acc.sum + p, v0[u]);
          }
          if (f1) unsafeAtomicAdd(acc.normalized_sum + p, v1[u]);
          if (f2) unsafeAtomicAdd(acc.normalized_sum_sq + p, v2[u]);
          continue;
        }
        const int lp = (int)((key[u] >> 32) - (uint64_t)p0);
        atomicAdd(pc + lp, 1u);
        atomicAdd(cn + lp, (unsigned)key[u]);
        if (f0) {
          if (sum_int) atomicAdd((unsigned long long*)(s0 + lp), (unsigned long long)__double_as_longlong(v0[u]));
          else atomicAdd(s0 + lp, v0[u]);
        }
        if (f1) atomicAdd(s1 + lp, v1[u]);
        if (f2) atomicAdd(s2 + lp, v2[u]);
      }
    }
    __syncthreads();  // pre / start / wsum are reused by the next batch
  }
  if (direct) return;
  int64_t plen = kp.P - p0;
  if (plen > kRangeParts) plen = kRangeParts;
  for (int t = threadIdx.x; t < plen; t += blockDim.x) {
    if (pc[t] == 0) continue;
    const int64_t p = p0 + t;
    atomicAdd((unsigned long long*)(acc.privacy_id_count + p), (unsigned long long)pc[t]);
    if (acc.count) atomicAdd((unsigned long long*)(acc.count + p), (unsigned long long)cn[t]);
    if (f0) {
      if (sum_int) atomicAdd((unsigned long long*)acc.sum + p, (unsigned long long)__double_as_longlong(s0[t]));
      else unsafeAtomicAdd((double*)acc.sum + p, s0[t]);
    }
    if (f1) unsafeAtomicAdd(acc.normalized_sum + p, s1[t]);
    if (f2) unsafeAtomicAdd(acc.normalized_sum_sq + p, s2[t]);
  }
}

// ----------------------------------------------------- two-level merge --
// Records of coarse range r (work item from k_range_plan, buckets [b_lo,
// b_hi)) in batches of one bucket per thread; visit(idx, ok) for RR records
// per thread at a time (ok = a real record), then `after()` once per round.
template <typename V, typename A>
__device__ __forceinline__ void item_rounds(const KP& kp, const PairRecords& rec, int r, int64_t b_lo, int64_t b_hi,
                                            unsigned long long* start, unsigned* pre, unsigned* wsum, V&& visit,
                                            A&& after) {
  constexpr int RR = 4;
  const int64_t n_slots = (int64_t)kp.l0 << kp.bucket_bits;
  for (int64_t bb = b_lo; bb < b_hi; bb += blockDim.x) {
    int64_t nb = b_hi - bb;
    if (nb > blockDim.x) nb = blockDim.x;
    unsigned len = 0;
    if (threadIdx.x < nb) {
      const int64_t b = bb + threadIdx.x;
      const unsigned* run = rec.runs + r * rec.run_stride + b;
      const unsigned s0 = run[0];
      len = run[rec.run_stride] - s0;
      start[threadIdx.x] = (unsigned long long)(b * n_slots + s0);
    }
    unsigned total;
    const unsigned ex = block_excl_scan(len, wsum, &total);
    pre[threadIdx.x] = ex;
    __syncthreads();
    for (unsigned i0 = 0; i0 < total; i0 += RR * blockDim.x) {  // block-uniform trip count
      uint64_t idx[RR];
      bool ok[RR];
#pragma unroll
      for (int u = 0; u < RR; ++u) {
        const unsigned i = i0 + threadIdx.x + u * blockDim.x;
        ok[u] = i < total;
        int lo = 0, hi = (int)nb - 1;  // last run with pre <= i
        while (ok[u] && lo < hi) {
          const int mid = (lo + hi + 1) >> 1;
          if (pre[mid] <= i) lo = mid;
          else hi = mid - 1;
        }
        idx[u] = ok[u] ? start[lo] + (i - pre[lo]) : 0;
      }
      visit(idx, ok);
      after();
    }
    __syncthreads();  // pre / start / wsum are reused by the next batch
  }
}

constexpr int kFinePerCoarseMax = 1 << 13;  // 2^(range_bits - kRangeBits) <= 2^13 (P < 2^32, 256 coarse ranges)

// fine-range totals: per item an LDS histogram of its records' fine ranges,
// added to fine_total with one atomic per touched fine range
__global__ void __launch_bounds__(kSplitThreads) k_split_count(KP kp, PairRecords rec, const uint4* __restrict__ items,
                                                              const unsigned* __restrict__ n_items,
                                                              unsigned* __restrict__ fine_total,
                                                              unsigned* __restrict__ item_hist) {
  __shared__ unsigned long long start[kSplitThreads];
  __shared__ unsigned pre[kSplitThreads], wsum[kSplitThreads / 64 + 1];
  __shared__ unsigned lh[kFinePerCoarseMax];
  if (blockIdx.x >= *n_items) return;
  const uint4 it = items[blockIdx.x];
  if (it.x >> 31) return;  // sentinel
  const uint4 nx = items[blockIdx.x + 1];
  if (nx.z == it.z) return;  // empty item
  const int r = (int)it.x;
  const int F = 1 << (kp.range_bits - kRangeBits);
  const int64_t f0 = (int64_t)r << (kp.range_bits - kRangeBits);
  for (int t = threadIdx.x; t < F; t += blockDim.x) lh[t] = 0;
  __syncthreads();
  item_rounds(kp, rec, r, it.y, nx.y, start, pre, wsum,
              [&](const uint64_t (&idx)[4], const bool (&ok)[4]) {
                // the four loads unconditional (idx = 0 where !ok), so they
                // go out together: under the `ok` branch each waited for the last
                unsigned long long kk[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) kk[u] = rec.key[idx[u]];
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                  if (!ok[u]) continue;
                  const uint64_t f = (kk[u] >> (32 + kRangeBits)) - (uint64_t)f0;
                  if (f < (uint64_t)F) atomicAdd(lh + (int)f, 1u);  // else malformed: k_split_scatter skips it too
                }
              },
              [] {});
  __syncthreads();
  // the item's histogram for k_split_scatter, which then reserves its slots
  // once per fine range instead of once per round
  for (int t = threadIdx.x; t < F; t += blockDim.x) {
    const bool in = f0 + t < kp.n_fine_ranges;
    item_hist[(int64_t)blockIdx.x * F + t] = in ? lh[t] : 0u;
    if (lh[t] && in) atomicAdd(fine_total + f0 + t, lh[t]);
  }
}

// records of an item -> the fine-range-sorted arrays: the item reserves its
// slots of every fine range once (its histogram from k_split_count, one
// device atomic per touched fine range), then each record takes the next slot
// of its fine range from an LDS cursor (a returning LDS atomic) -- no
// barriers between the batches, so their loads overlap
__global__ void __launch_bounds__(kSplitThreads) k_split_scatter(KP kp, PairRecords rec, PairRecords stg,
                                                                const uint4* __restrict__ items,
                                                                const unsigned* __restrict__ n_items,
                                                                unsigned* __restrict__ fine_cur,
                                                                const unsigned* __restrict__ item_hist) {
  __shared__ unsigned long long start[kSplitThreads];
  __shared__ unsigned pre[kSplitThreads], wsum[kSplitThreads / 64 + 1];
  __shared__ unsigned lcur[kFinePerCoarseMax];
  if (blockIdx.x >= *n_items) return;
  const uint4 it = items[blockIdx.x];
  if (it.x >> 31) return;
  const uint4 nx = items[blockIdx.x + 1];
  if (nx.z == it.z) return;
  const int r = (int)it.x;
  const int F = 1 << (kp.range_bits - kRangeBits);
  const int64_t f0 = (int64_t)r << (kp.range_bits - kRangeBits);
  for (int t = threadIdx.x; t < F; t += blockDim.x) {
    const unsigned c = item_hist[(int64_t)blockIdx.x * F + t];
    lcur[t] = c ? atomicAdd(fine_cur + f0 + t, c) : 0u;
  }
  __syncthreads();
  item_rounds(kp, rec, r, it.y, nx.y, start, pre, wsum,
              [&](const uint64_t (&idx)[4], const bool (&ok)[4]) {
                unsigned long long key[4];
                double v0[4], v1[4], v2[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                  key[u] = ok[u] ? rec.key[idx[u]] : 0ull;
                  v0[u] = (ok[u] && stg.f0) ? rec.f0[idx[u]] : 0.0;
                  v1[u] = (ok[u] && stg.f1) ? rec.f1[idx[u]] : 0.0;
                  v2[u] = (ok[u] && stg.f2) ? rec.f2[idx[u]] : 0.0;
                }
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                  const uint64_t fu = (key[u] >> (32 + kRangeBits)) - (uint64_t)f0;
                  // a malformed record is skipped, as k_split_count leaves it uncounted
                  if (!ok[u] || fu >= (uint64_t)F || f0 + (int64_t)fu >= kp.n_fine_ranges) continue;
                  const uint64_t o = atomicAdd(lcur + (int)fu, 1u);
                  stg.key[o] = key[u];
                  if (stg.f0) stg.f0[o] = v0[u];
                  if (stg.f1) stg.f1[o] = v1[u];
                  if (stg.f2) stg.f2[o] = v2[u];
                }
              },
              [] {});
}

// k_split_scatter for coarse ranges of <= kSplitStageFan fine ranges (C4 /
// C5: 32): each round's records are counting-sorted by fine range in LDS
// first, so a fine range's records leave as one contiguous run (~32 per
// round) instead of one scattered 8-byte store per record and array
constexpr int kSplitStageFan = 256;
constexpr int kSplitStageRows = 4 * kSplitThreads;  // item_rounds' RR records per thread
__global__ void __launch_bounds__(kSplitThreads) k_split_scatter_staged(KP kp, PairRecords rec, PairRecords stg,
                                                                       const uint4* __restrict__ items,
                                                                       const unsigned* __restrict__ n_items,
                                                                       unsigned* __restrict__ fine_cur,
                                                                       const unsigned* __restrict__ item_hist) {
  __shared__ unsigned long long start[kSplitThreads];
  __shared__ unsigned pre[kSplitThreads], wsum[kSplitThreads / 64 + 1];
  __shared__ unsigned lcur[kSplitStageFan], hist[kSplitStageFan], hstart[kSplitStageFan], gbase[kSplitStageFan];
  __shared__ unsigned long long skey[kSplitStageRows];
  __shared__ double sf0[kSplitStageRows], sf1[kSplitStageRows], sf2[kSplitStageRows];
  __shared__ uint8_t sdest[kSplitStageRows];
  if (blockIdx.x >= *n_items) return;
  const uint4 it = items[blockIdx.x];
  if (it.x >> 31) return;
  const uint4 nx = items[blockIdx.x + 1];
  if (nx.z == it.z) return;
  const int r = (int)it.x;
  const int F = 1 << (kp.range_bits - kRangeBits);  // <= kSplitStageFan (host-checked)
  const int64_t f0 = (int64_t)r << (kp.range_bits - kRangeBits);
  for (int t = threadIdx.x; t < F; t += blockDim.x) {
    const unsigned c = item_hist[(int64_t)blockIdx.x * F + t];
    lcur[t] = c ? atomicAdd(fine_cur + f0 + t, c) : 0u;
    hist[t] = 0;
  }
  __syncthreads();
  item_rounds(kp, rec, r, it.y, nx.y, start, pre, wsum,
              [&](const uint64_t (&idx)[4], const bool (&ok)[4]) {
                unsigned long long key[4];
                double v0[4], v1[4], v2[4];
                int fu[4];
                unsigned rk[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                  key[u] = ok[u] ? rec.key[idx[u]] : 0ull;
                  v0[u] = (ok[u] && stg.f0) ? rec.f0[idx[u]] : 0.0;
                  v1[u] = (ok[u] && stg.f1) ? rec.f1[idx[u]] : 0.0;
                  v2[u] = (ok[u] && stg.f2) ? rec.f2[idx[u]] : 0.0;
                }
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                  const uint64_t f = (key[u] >> (32 + kRangeBits)) - (uint64_t)f0;
                  // a malformed record is skipped, as k_split_count leaves it uncounted
                  fu[u] = ok[u] && f < (uint64_t)F && f0 + (int64_t)f < kp.n_fine_ranges ? (int)f : -1;
                  rk[u] = fu[u] >= 0 ? atomicAdd(hist + fu[u], 1u) : 0u;
                }
                __syncthreads();
                if (threadIdx.x < 64) {  // run starts in the stage; the runs' output positions
                  const int lane = threadIdx.x;
                  unsigned carry = 0;
                  for (int b0 = 0; b0 < F; b0 += 64) {
                    const unsigned hv = b0 + lane < F ? hist[b0 + lane] : 0u;
                    unsigned incl = hv;
                    for (int o = 1; o < 64; o <<= 1) {
                      const unsigned up = __shfl_up(incl, o, 64);
                      if (lane >= o) incl += up;
                    }
                    if (b0 + lane < F) {
                      hstart[b0 + lane] = carry + incl - hv;
                      gbase[b0 + lane] = lcur[b0 + lane];
                      lcur[b0 + lane] += hv;
                    }
                    carry += __shfl(incl, 63, 64);
                  }
                }
                __syncthreads();
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                  if (fu[u] < 0) continue;
                  const unsigned sl = hstart[fu[u]] + rk[u];
                  skey[sl] = key[u];
                  sf0[sl] = v0[u];
                  sf1[sl] = v1[u];
                  sf2[sl] = v2[u];
                  sdest[sl] = (uint8_t)fu[u];
                }
                __syncthreads();
                const unsigned n = hstart[F - 1] + hist[F - 1];
                for (unsigned i = threadIdx.x; i < n; i += blockDim.x) {
                  const int f = sdest[i];
                  const uint64_t o = (uint64_t)gbase[f] + (i - hstart[f]);
                  stg.key[o] = skey[i];
                  if (stg.f0) stg.f0[o] = sf0[i];
                  if (stg.f1) stg.f1[o] = sf1[i];
                  if (stg.f2) stg.f2[o] = sf2[i];
                }
                __syncthreads();
                for (int t = threadIdx.x; t < F; t += blockDim.x) hist[t] = 0;
                __syncthreads();
              },
              [] {});
}

// fine work items: fine range f's records [start_f, start_f+1) in chunks of
// kRangeChunk, appended at a base taken with one atomic (any order)
__global__ void __launch_bounds__(kBlock) k_fine_plan(KP kp, const unsigned* __restrict__ fine_start,
                                                      uint4* __restrict__ items, unsigned* __restrict__ n_items) {
  const int64_t f = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (f >= kp.n_fine_ranges) return;
  const unsigned s0 = fine_start[f], s1 = fine_start[f + 1];
  if (s1 <= s0) return;
  const unsigned C = (unsigned)kRangeChunk;
  const unsigned k = (s1 - s0 + C - 1) / C;
  const unsigned base = atomicAdd(n_items, k);
  for (unsigned j = 0; j < k; ++j) {
    const unsigned a = s0 + j * C;
    items[base + j] = make_uint4((unsigned)f, a, (s1 - a < C ? s1 - a : C), 0u);
  }
}

// one workgroup per fine item: contiguous records of one 2^kRangeBits range,
// summed in LDS (or added directly when few), then coalesced atomics
__global__ void __launch_bounds__(kReduceThreads) k_fine_reduce(KP kp, PairRecords stg, const uint4* __restrict__ items,
                                                              const unsigned* __restrict__ n_items,
                                                              pdp_partition_accumulators acc, unsigned* err,
                                                              PairRecords rec) {
  extern __shared__ unsigned long long smem[];
  double* s0 = (double*)smem;
  double* s1 = s0 + kRangeParts;
  double* s2 = s1 + kRangeParts;
  unsigned* pc = (unsigned*)(s2 + kRangeParts);
  unsigned* cn = pc + kRangeParts;
  add_flat_pairs(kp, rec, acc, err);  // (`rec`: the bucket kernels' records, for their flat list only)
  if (blockIdx.x >= *n_items) return;
  const uint4 it = items[blockIdx.x];
  const int64_t p0 = (int64_t)it.x << kRangeBits;
  const uint64_t a = it.y;
  const unsigned len = it.z;
  const int flags = kp.clip.flags;
  const bool f0 = flags & (PDP_ACC_SUM | PDP_SUM_PER_PARTITION), f1 = flags & PDP_ACC_NSUM,
             f2 = flags & PDP_ACC_NSUM2, sum_int = flags & PDP_SUM_INT;
  const bool direct = len < kRangeDirect;
  if (!direct) {
    for (int t = threadIdx.x; t < kRangeParts; t += blockDim.x) {
      pc[t] = 0;
      cn[t] = 0;
      s0[t] = 0.0;
      s1[t] = 0.0;
      s2[t] = 0.0;
    }
    __syncthreads();
  }
  // RB records per thread loaded together, then summed
  constexpr int RB = 4;
  for (unsigned i0 = threadIdx.x; i0 < len; i0 += RB * blockDim.x) {
    unsigned long long kk[RB];
    double w0[RB], w1[RB], w2[RB];
#pragma unroll
    for (int u = 0; u < RB; ++u) {
      const unsigned i = i0 + u * blockDim.x;
      const uint64_t o = a + (i < len ? i : 0u);
      kk[u] = i < len ? stg.key[o] : ~0ull;
      w0[u] = (i < len && f0) ? stg.f0[o] : 0.0;
      w1[u] = (i < len && f1) ? stg.f1[o] : 0.0;
      w2[u] = (i < len && f2) ? stg.f2[o] : 0.0;
    }
#pragma unroll
    for (int u = 0; u < RB; ++u) {
      if (i0 + u * blockDim.x >= len) continue;
      const unsigned long long key = kk[u];
      if ((int64_t)(key >> 32) >= kp.P || (key >> 32) - (uint64_t)p0 >= (uint64_t)kRangeParts) {  // malformed
        atomicOr(err, 1u);
        continue;
      }
      const double v0 = w0[u], v1 = w1[u], v2 = w2[u];
      if (direct) {
        const int64_t p = (int64_t)(key >> 32);
        atomicAdd((unsigned long long*)(acc.privacy_id_count + p), 1ull);
        if (acc.count) atomicAdd((unsigned long long*)(acc.count + p), (unsigned long long)(uint32_t)key);
        if (f0) {
          if (sum_int) atomicAdd((unsigned long long*)acc.sum + p, (unsigned long long)__double_as_longlong(v0));
          else unsafeAtomicAdd((double*)acc.sum + p, v0);
        }
        if (f1) unsafeAtomicAdd(acc.normalized_sum + p, v1);
        if (f2) unsafeAtomicAdd(acc.normalized_sum_sq + p, v2);
        continue;
      }
      const int lp = (int)((key >> 32) - (uint64_t)p0);
      atomicAdd(pc + lp, 1u);
      atomicAdd(cn + lp, (unsigned)key);
      if (f0) {
        if (sum_int) atomicAdd((unsigned long long*)(s0 + lp), (unsigned long long)__double_as_longlong(v0));
        else atomicAdd(s0 + lp, v0);
      }
      if (f1) atomicAdd(s1 + lp, v1);
      if (f2) atomicAdd(s2 + lp, v2);
    }
  }
  if (direct) return;
  __syncthreads();
  int64_t plen = kp.P - p0;
  if (plen > kRangeParts) plen = kRangeParts;
  for (int t = threadIdx.x; t < plen; t += blockDim.x) {
    if (pc[t] == 0) continue;
    const int64_t p = p0 + t;
    atomicAdd((unsigned long long*)(acc.privacy_id_count + p), (unsigned long long)pc[t]);
    if (acc.count) atomicAdd((unsigned long long*)(acc.count + p), (unsigned long long)cn[t]);
    if (f0) {
      if (sum_int) atomicAdd((unsigned long long*)acc.sum + p, (unsigned long long)__double_as_longlong(s0[t]));
      else unsafeAtomicAdd((double*)acc.sum + p, s0[t]);
    }
    if (f1) unsafeAtomicAdd(acc.normalized_sum + p, s1[t]);
    if (f2) unsafeAtomicAdd(acc.normalized_sum_sq + p, s2[t]);
  }
}
constexpr size_t kFineLds = kRangeParts * (3 * 8 + 2 * 4);

}  // namespace

int launch_merge(const KP& kp0, const Plan& p, hipStream_t st, char* ws, const Ws& w,
                 const pdp_partition_accumulators& acc) {
  KP kp = kp0;
  kp.n_buckets = p.buckets_out;
  const PairRecords rec = pair_records(ws, w, p);
  unsigned* err = at<unsigned>(ws, w.err);
  int rc = allow_dynamic_lds(k_range_reduce, kRangeLds);
  if (rc != PDP_OK) return rc;
  uint4* items = at<uint4>(ws, w.rr_items);
  unsigned* n_items = at<unsigned>(ws, w.rr_count);
  PDP_HIP_CHECK(hipMemsetAsync(n_items, 0, 4, st));
  // (the per-id fix-up writes no record segments: one segment, nothing to skip)
  const unsigned* last_ids = p.band && !p.fix_ids ? at<unsigned>(ws, w.sctl2) : nullptr;
  rc = launch("k_range_plan", k_range_plan, dim3((unsigned)p.n_ranges), dim3(kRangeThreads), 0, st, kp, rec.runs, items,
              n_items, last_ids, (int64_t)p.n_buckets);
  if (rc != PDP_OK) return rc;
  if (!p.two_level)
    return launch("k_range_reduce", k_range_reduce, dim3((unsigned)p.n_groups), dim3(kReduceThreads), kRangeLds, st, kp,
                  rec, items, n_items, acc, err);
  // two-level: coarse items -> fine-range totals -> starts -> records
  // re-sorted by fine range -> fine items -> LDS sums
  unsigned* fine_total = at<unsigned>(ws, w.fine_total);
  unsigned* fine_cur = at<unsigned>(ws, w.fine_cur);
  PairRecords stg{};
  stg.key = at<unsigned long long>(ws, w.stg_key);
  stg.f0 = at_opt<double>(ws, w.stg_f0);
  stg.f1 = at_opt<double>(ws, w.stg_f1);
  stg.f2 = at_opt<double>(ws, w.stg_f2);
  PDP_HIP_CHECK(hipMemsetAsync(fine_total, 0, (uint64_t)(p.n_fine + 1) * 4, st));
  unsigned* item_hist = at<unsigned>(ws, w.item_hist);
  rc = launch("k_split_count", k_split_count, dim3((unsigned)p.n_groups), dim3(kSplitThreads), 0, st, kp, rec, items,
              n_items, fine_total, item_hist);
  if (rc != PDP_OK) return rc;
  rc = scan_u32(fine_total, p.n_fine, at<unsigned>(ws, w.fine_chunks), st);
  if (rc != PDP_OK) return rc;
  PDP_HIP_CHECK(hipMemcpyAsync(fine_cur, fine_total, (uint64_t)p.n_fine * 4, hipMemcpyDeviceToDevice, st));
  const bool staged = (1 << (kp.range_bits - kRangeBits)) <= kSplitStageFan;
  rc = launch("k_split_scatter", staged ? k_split_scatter_staged : k_split_scatter, dim3((unsigned)p.n_groups),
              dim3(kSplitThreads), 0, st, kp, rec, stg, items, n_items, fine_cur, item_hist);
  if (rc != PDP_OK) return rc;
  uint4* fitems = at<uint4>(ws, w.fine_items);
  unsigned* n_fitems = at<unsigned>(ws, w.fine_count);
  PDP_HIP_CHECK(hipMemsetAsync(n_fitems, 0, 4, st));
  rc = launch("k_fine_plan", k_fine_plan, dim3(grid_for(p.n_fine, 1 << 20)), dim3(kBlock), 0, st, kp, fine_total,
              fitems, n_fitems);
  if (rc != PDP_OK) return rc;
  return launch_big_lds("k_fine_reduce", k_fine_reduce, dim3((unsigned)p.fine_items), dim3(kReduceThreads), kFineLds,
                        st, kp, stg, fitems, n_fitems, acc, err, rec);
}

}  // namespace pdp
