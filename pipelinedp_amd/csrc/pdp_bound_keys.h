// pdp_bound_keys.h -- device helpers that more than one of the bounding
// sources (pdp_bound*.hip, pdp_scan.hip) uses.
#pragma once

#include "pdp_bound_plan.h"

namespace pdp {

// exclusive block-wide scan of one u32 per thread; wsum = LDS[blockDim/64]
__device__ __forceinline__ unsigned block_excl_scan(unsigned x, unsigned* wsum, unsigned* total) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, nw = blockDim.x >> 6;
  unsigned inc = x;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const unsigned y = __shfl_up(inc, off, 64);
    if (lane >= off) inc += y;
  }
  if (lane == 63) wsum[w] = inc;
  __syncthreads();
  if (w == 0) {
    const unsigned v = lane < nw ? wsum[lane] : 0;
    unsigned vi = v;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
      const unsigned y = __shfl_up(vi, off, 64);
      if (lane >= off) vi += y;
    }
    if (lane < nw) wsum[lane] = vi - v;
    if (lane == nw - 1) wsum[nw] = vi;
  }
  __syncthreads();
  *total = wsum[nw];
  return wsum[w] + inc - x;
}

}  // namespace pdp
