// opk_segment_mean.hip.h -- op_segment_means' kernel (included by op_services.hip only)
#pragma once

#include "opk_common.hip.h"
#include "opk_pairwise.hip.h"

namespace opk {

// ----------------------------------------------------------------------------------------------
// Mean keep-probability of token ranges (one thread per range), bit for bit what the reference computes on the host
// with numpy: float(block_probs[start:end].mean()) (standalone.py:3075-3082) = float32 PAIRWISE sum in numpy's order
// (umath/loops_utils.h.src, @TYPE@_pairwise_sum: < 8 elements sequential; <= 128 elements eight running sums over
// blocks of 8, combined as ((r0+r1)+(r2+r3))+((r4+r5)+(r6+r7)), then the remainder sequentially; longer ranges split
// at n/2 rounded down to a multiple of 8), divided by the count in float64 and rounded back to float32.  An empty range
// scores 1.0 (ref :3081).  process() then copies 4 bytes per FRAGMENT back instead of 4 per token and runs no numpy
// reduction per fragment.  Explicit __fadd_rn: nothing here may be contracted or reassociated.
// ----------------------------------------------------------------------------------------------
// (np_pairwise_sum_f32: opk_pairwise.hip.h)

__global__ void segment_mean_kernel(const float* __restrict__ values, const int32_t* __restrict__ seg, int n_seg,
                                    int n_values, float* __restrict__ out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_seg) return;
  int start = seg[2 * i], end = seg[2 * i + 1];
  start = start < 0 ? 0 : start;
  end = end > n_values ? n_values : end;
  if (end <= start) {
    out[i] = 1.0f;
    return;
  }
  const float sum = np_pairwise_sum_f32(values + start, end - start);
  out[i] = (float)((double)sum / (double)(end - start));
}

}  // namespace opk
