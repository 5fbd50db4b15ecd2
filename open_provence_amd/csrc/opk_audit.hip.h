// opk_audit.hip.h -- device side of the running audit of a calibrated kernel set (op_coverage_scan / op_coverage_commit /
// op_gather_rows / op_audit_compare): which token ids the audited rows have covered, the gather of a few rows of a packed
// batch into a sub-batch, and the max |difference| between two sets of logits.  All of it is memory-bound and a few
// microseconds long: plain C++ with wave reductions and ordinary atomics on global memory, no LDS beyond a scan's wave totals.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace opk {

// The handle's coverage state block (uint32 words) next to its bitmap of vocab_size bits.
constexpr int COV_ST_MAXLEN = 0;   // atomicMax: the longest audited row (lives as long as the bitmap)
constexpr int COV_ST_NOVEL = 1;    // one scan: positions whose id's bit is clear, summed over the rows
constexpr int COV_ST_LONGEST = 2;  // one scan: uint64 atomicMax of (length << 32 | ~row), so the FIRST longest row wins
constexpr int COV_ST_WORDS = 4;

// [start, start + len) of row s of a packed batch, held inside [0, total) whatever cu holds
__device__ __forceinline__ void row_span(const int32_t* __restrict__ cu, int s, int total, int& start, int& len) {
  const int a = max(cu[s], 0), b = min(cu[s + 1], total);
  start = a;
  len = max(b - a, 0);
}

// 1. One wave per row (4 rows per block): row_novel[s] = positions of row s whose id has no bit in the bitmap.  An id
// outside 0 <= id < vocab counts as novel and is never used as an index.  Read-only on the bitmap.
__global__ __launch_bounds__(256) void coverage_scan_kernel(const int32_t* __restrict__ ids, const int32_t* __restrict__ cu, int n_seqs,
                                                            int total, int vocab, const uint32_t* __restrict__ bits,
                                                            int32_t* __restrict__ row_novel, uint32_t* __restrict__ state) {
  const int lane = threadIdx.x & 63;
  const int s = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (s >= n_seqs) return;
  int start, len;
  row_span(cu, s, total, start, len);
  int count = 0;
  for (int j = lane; j < len; j += 64) {
    const uint32_t id = (uint32_t)ids[start + j];  // (one unsigned compare: a negative id is a huge value)
    const bool seen = id < (uint32_t)vocab && ((bits[id >> 5] >> (id & 31)) & 1u);
    count += seen ? 0 : 1;
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) count += __shfl_xor(count, off);
  if (lane == 0) {
    row_novel[s] = count;
    if (count) atomicAdd(state + COV_ST_NOVEL, (uint32_t)count);
    const unsigned long long key = ((unsigned long long)(uint32_t)len << 32) | (unsigned long long)(~(uint32_t)s);
    atomicMax(reinterpret_cast<unsigned long long*>(state + COV_ST_LONGEST), key);
  }
}

// 2. One wave per listed row: the bit of every id of the row is set, the longest audited length raised.  A listed row
// outside [0, n_seqs) is skipped.
__global__ __launch_bounds__(256) void coverage_commit_kernel(const int32_t* __restrict__ ids, const int32_t* __restrict__ cu, int n_seqs,
                                                              int total, const int32_t* __restrict__ rows, int n_rows, int vocab,
                                                              uint32_t* __restrict__ bits, uint32_t* __restrict__ state) {
  const int lane = threadIdx.x & 63;
  const int i = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (i >= n_rows) return;
  const int s = rows[i];
  if (s < 0 || s >= n_seqs) return;
  int start, len;
  row_span(cu, s, total, start, len);
  for (int j = lane; j < len; j += 64) {
    const uint32_t id = (uint32_t)ids[start + j];
    if (id >= (uint32_t)vocab) continue;
    const uint32_t bit = 1u << (id & 31);
    if (!(bits[id >> 5] & bit)) atomicOr(bits + (id >> 5), bit);
  }
  if (lane == 0 && len > 0) atomicMax(state + COV_ST_MAXLEN, (uint32_t)len);
}

// 3a. One block: sub_cu[i + 1] = sum of the lengths of rows[0 .. i] (sub_cu[0] = 0), 1024 rows per step with a carry.  A
// listed row outside [0, n_seqs) has length 0.
__global__ __launch_bounds__(1024) void gather_offsets_kernel(const int32_t* __restrict__ cu, int n_seqs, int total,
                                                              const int32_t* __restrict__ rows, int n_rows, int32_t* __restrict__ sub_cu) {
  __shared__ int wave_sum[16];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int carry = 0;  // (the same in every thread)
  for (int i0 = 0; i0 < n_rows; i0 += 1024) {
    const int i = i0 + tid;
    int sum = 0;
    if (i < n_rows && rows[i] >= 0 && rows[i] < n_seqs) {
      int start;
      row_span(cu, rows[i], total, start, sum);
    }
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
      const int up = __shfl_up(sum, off);
      if (lane >= off) sum += up;
    }
    if (lane == 63) wave_sum[wave] = sum;
    __syncthreads();
    int before = 0, step = 0;
#pragma unroll
    for (int w = 0; w < 16; ++w) {
      if (w < wave) before += wave_sum[w];
      step += wave_sum[w];
    }
    if (i < n_rows) sub_cu[1 + i] = carry + before + sum;
    carry += step;
    __syncthreads();
  }
  if (tid == 0) sub_cu[0] = 0;
}

// 3b. sub_ids[sub_cu[i] + j] = ids[cu[rows[i]] + j].  grid = (n_rows, column chunks): consecutive lanes read and write
// consecutive elements.
__global__ __launch_bounds__(256) void gather_rows_kernel(const int32_t* __restrict__ ids, const int32_t* __restrict__ cu, int n_seqs,
                                                          int total, const int32_t* __restrict__ rows, const int32_t* __restrict__ sub_cu,
                                                          int32_t* __restrict__ sub_ids) {
  const int i = blockIdx.x;
  const int s = rows[i];
  if (s < 0 || s >= n_seqs) return;
  int src, len;
  row_span(cu, s, total, src, len);
  const int dst = sub_cu[i];
  for (int j = blockIdx.y * 256 + threadIdx.x; j < len; j += gridDim.y * 256) sub_ids[dst + j] = ids[src + j];
}

// 4. err[0] = max |a - b| over the 2 pruning logits of every token of the listed rows and their n_labels ranking logits,
// +inf when a value on either side is not finite, a listed row lies outside [0, n_seqs) or its two lengths differ.
// Non-negative floats order as their bit patterns, so the maximum is one atomicMax on the cell's uint32 view per wave; fp32
// max does not depend on the order.  The cell holds +0.0 on entry (op_audit_compare clears it on the same stream).
// grid = (n_rows, column chunks).
__global__ __launch_bounds__(256) void audit_compare_kernel(const float* __restrict__ prune, const float* __restrict__ rank,
                                                            const int32_t* __restrict__ cu, int n_seqs, int total,
                                                            const int32_t* __restrict__ rows, const float* __restrict__ sub_prune,
                                                            const float* __restrict__ sub_rank, const int32_t* __restrict__ sub_cu,
                                                            int n_labels, float* __restrict__ err) {
  const int i = blockIdx.x;
  const int s = rows[i];
  float worst = 0.0f;
  if (s < 0 || s >= n_seqs) {
    worst = INFINITY;
  } else {
    int src, len;
    row_span(cu, s, total, src, len);
    const int dst = sub_cu[i], sub_len = sub_cu[i + 1] - dst;
    if (len != sub_len || dst < 0) worst = INFINITY;
    const int n = (len == sub_len && dst >= 0) ? 2 * len : 0;
    const float* a = prune + 2 * (size_t)src;
    const float* b = sub_prune + 2 * (size_t)dst;
    for (int j = blockIdx.y * 256 + threadIdx.x; j < n; j += gridDim.y * 256) {
      const float x = a[j], y = b[j];
      worst = fmaxf(worst, (isfinite(x) && isfinite(y)) ? fabsf(x - y) : INFINITY);
    }
    if (blockIdx.y == 0) {
      for (int j = threadIdx.x; j < n_labels; j += 256) {
        const float x = rank[(size_t)s * n_labels + j], y = sub_rank[(size_t)i * n_labels + j];
        worst = fmaxf(worst, (isfinite(x) && isfinite(y)) ? fabsf(x - y) : INFINITY);
      }
    }
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) worst = fmaxf(worst, __shfl_xor(worst, off));
  if ((threadIdx.x & 63) == 0 && worst > 0.0f) atomicMax(reinterpret_cast<uint32_t*>(err), __float_as_uint(worst));
}

}  // namespace opk
