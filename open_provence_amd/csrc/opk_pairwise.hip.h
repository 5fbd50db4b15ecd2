// opk_pairwise.hip.h -- numpy's pairwise sum as device functions, bit for bit (umath/loops_utils.h.src, @TYPE@_pairwise_sum:
// < 8 elements sequential from 0; <= 128 elements eight running sums over blocks of 8, combined as
// ((r0+r1)+(r2+r3))+((r4+r5)+(r6+r7)), then the remainder sequentially; longer ranges split at n/2 rounded down to a multiple
// of 8).  np.add.reduce over a contiguous array of n elements is this sum over all n (held to numpy by tests/test_gpu_model.py
// and tests/test_decision_model.py).  The float32 form serves the per-fragment means (segment_mean_kernel,
// planned_fragment_means_kernel), the float64 form the per-sentence averages (sentence_decisions_kernel), whose values are
// fp32 means widened exactly.  Explicit __fadd_rn / __dadd_rn: nothing here may be contracted or reassociated.
#pragma once

#include <hip/hip_runtime.h>

namespace opk {

__device__ inline float np_pairwise_leaf_f32(const float* a, int n) {  // n <= 128
  if (n < 8) {
    float res = 0.f;
    for (int i = 0; i < n; ++i) res = __fadd_rn(res, a[i]);
    return res;
  }
  float r[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) r[j] = a[j];
  int i = 8;
  for (; i < n - (n % 8); i += 8) {
#pragma unroll
    for (int j = 0; j < 8; ++j) r[j] = __fadd_rn(r[j], a[i + j]);
  }
  float res = __fadd_rn(__fadd_rn(__fadd_rn(r[0], r[1]), __fadd_rn(r[2], r[3])),
                        __fadd_rn(__fadd_rn(r[4], r[5]), __fadd_rn(r[6], r[7])));
  for (; i < n; ++i) res = __fadd_rn(res, a[i]);
  return res;
}
// the recursion pairwise(a, n) = pairwise(a, n2) + pairwise(a + n2, n - n2) on an explicit stack (depth <= 24 covers any int)
__device__ inline float np_pairwise_sum_f32(const float* a, int n) {
  const float* fa[24];
  int fn[24], fstage[24];
  float fleft[24];
  int sp = 0;
  fa[0] = a; fn[0] = n; fstage[0] = 0; fleft[0] = 0.f;
  float ret = 0.f;
  while (sp >= 0) {
    if (fn[sp] <= 128) {
      ret = np_pairwise_leaf_f32(fa[sp], fn[sp]);
      --sp;
      continue;
    }
    int n2 = fn[sp] / 2;
    n2 -= n2 % 8;
    if (fstage[sp] == 0) {
      fstage[sp] = 1;
      fa[sp + 1] = fa[sp]; fn[sp + 1] = n2; fstage[sp + 1] = 0;
      ++sp;
    } else if (fstage[sp] == 1) {
      fleft[sp] = ret;
      fstage[sp] = 2;
      fa[sp + 1] = fa[sp] + n2; fn[sp + 1] = fn[sp] - n2; fstage[sp + 1] = 0;
      ++sp;
    } else {
      ret = __fadd_rn(fleft[sp], ret);
      --sp;
    }
  }
  return ret;
}

// The float64 twin over fp32 values: every element is widened (exactly) where it is read, every addition is a float64 one --
// np.add.reduce(np.asarray(values, dtype=np.float64)).
__device__ inline double np_pairwise_leaf_f64(const float* a, int n) {  // n <= 128
  if (n < 8) {
    double res = 0.0;
    for (int i = 0; i < n; ++i) res = __dadd_rn(res, (double)a[i]);
    return res;
  }
  double r[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) r[j] = (double)a[j];
  int i = 8;
  for (; i < n - (n % 8); i += 8) {
#pragma unroll
    for (int j = 0; j < 8; ++j) r[j] = __dadd_rn(r[j], (double)a[i + j]);
  }
  double res = __dadd_rn(__dadd_rn(__dadd_rn(r[0], r[1]), __dadd_rn(r[2], r[3])),
                         __dadd_rn(__dadd_rn(r[4], r[5]), __dadd_rn(r[6], r[7])));
  for (; i < n; ++i) res = __dadd_rn(res, (double)a[i]);
  return res;
}
__device__ inline double np_pairwise_sum_f64(const float* a, int n) {
  const float* fa[24];
  int fn[24], fstage[24];
  double fleft[24];
  int sp = 0;
  fa[0] = a; fn[0] = n; fstage[0] = 0; fleft[0] = 0.0;
  double ret = 0.0;
  while (sp >= 0) {
    if (fn[sp] <= 128) {
      ret = np_pairwise_leaf_f64(fa[sp], fn[sp]);
      --sp;
      continue;
    }
    int n2 = fn[sp] / 2;
    n2 -= n2 % 8;
    if (fstage[sp] == 0) {
      fstage[sp] = 1;
      fa[sp + 1] = fa[sp]; fn[sp + 1] = n2; fstage[sp + 1] = 0;
      ++sp;
    } else if (fstage[sp] == 1) {
      fleft[sp] = ret;
      fstage[sp] = 2;
      fa[sp + 1] = fa[sp] + n2; fn[sp + 1] = fn[sp] - n2; fstage[sp + 1] = 0;
      ++sp;
    } else {
      ret = __dadd_rn(fleft[sp], ret);
      --sp;
    }
  }
  return ret;
}

}  // namespace opk
