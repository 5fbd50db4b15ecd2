// opk_padded.hip.h -- the padded [B, L] boundary on the device (op_pack_padded / op_unpack_padded): row lengths and
// validation of a padded batch, the prefix scan to cu_seqlens, the gather of the attention_mask != 0 ids into the packed
// layout, and the scatter of packed fp32 outputs back to [B, L, C].  All four are memory-bound and small next to a
// forward: plain C++ with vector loads / stores and atomics, no LDS beyond the scan's wave totals.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

namespace opk {

// The handle's device status block (uint32 words), filled by padded_lengths_kernel / padded_scan_kernel.
constexpr int PAD_ST_MASK = 0;    // atomicMin: linear index row * width + col of the first mask fault; PAD_ST_NONE = none
constexpr int PAD_ST_ID = 1;      // atomicMin: ... of the first id outside the embedding table
constexpr int PAD_ST_TOTAL = 2;   // total tokens
constexpr int PAD_ST_MAXLEN = 3;  // longest row
constexpr int PAD_ST_IDVAL = 4;   // the id at PAD_ST_ID, int64 as (lo, hi) words
constexpr int PAD_ST_WORDS = 8;
constexpr uint32_t PAD_ST_NONE = 0xffffffffu;

struct NoMask {};  // MaskT of a NULL mask: every row is full

// 4 consecutive elements of a row.  wide: p is aligned for one (uint8: 4 bytes, int32: 16 bytes) or two (int64: 2 x 16
// bytes) naturally aligned loads and all 4 lie inside the row; otherwise element loads of the n that do.
template <typename T>
__device__ __forceinline__ void load4(const T* __restrict__ p, bool wide, int n, T (&v)[4]) {
  if (wide) {
    if constexpr (sizeof(T) == 1) {
      const uint32_t w = *reinterpret_cast<const uint32_t*>(p);
      v[0] = (T)(w & 0xff), v[1] = (T)((w >> 8) & 0xff), v[2] = (T)((w >> 16) & 0xff), v[3] = (T)(w >> 24);
    } else if constexpr (sizeof(T) == 4) {
      const int4 w = *reinterpret_cast<const int4*>(p);
      v[0] = (T)w.x, v[1] = (T)w.y, v[2] = (T)w.z, v[3] = (T)w.w;
    } else {
      const longlong2 a = reinterpret_cast<const longlong2*>(p)[0], b = reinterpret_cast<const longlong2*>(p)[1];
      v[0] = (T)a.x, v[1] = (T)a.y, v[2] = (T)b.x, v[3] = (T)b.y;
    }
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k) v[k] = k < n ? p[k] : T(0);
  }
}
template <typename T>
__device__ __forceinline__ bool row_is_wide(const T* row) {
  constexpr uintptr_t bytes = sizeof(T) * 4 < 16 ? sizeof(T) * 4 : 16;
  return (reinterpret_cast<uintptr_t>(row) & (bytes - 1)) == 0;
}

// 1. One wave per row (4 rows per block): len[r] = number of non-zero mask entries, and the two checks of the padded
// boundary.  A row is right-padded (ones then zeros) when that count equals the index of its last non-zero entry + 1;
// otherwise the row's first zero entry -- which then has a non-zero entry behind it -- is the fault.  Ids are held to
// 0 <= id < vocab where the mask is non-zero only.  The first fault of each kind in row-major order wins (atomicMin on
// the linear index, which the caller keeps below 2^31).  len_out = cu_seqlens + 1: the scan runs in place.
template <typename IdT, typename MaskT>
__global__ __launch_bounds__(256) void padded_lengths_kernel(const IdT* __restrict__ ids, const MaskT* __restrict__ mask, int n_rows,
                                                             int width, int vocab, int32_t* __restrict__ len_out,
                                                             uint32_t* __restrict__ status) {
  constexpr bool HAS_MASK = !std::is_same<MaskT, NoMask>::value;
  constexpr int NONE = 0x7fffffff;
  const int lane = threadIdx.x & 63;
  const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= n_rows) return;
  const size_t base = (size_t)r * (size_t)width;
  const IdT* irow = ids + base;
  const bool iwide = row_is_wide(irow);
  const MaskT* mrow = nullptr;
  bool mwide = false;
  if constexpr (HAS_MASK) {
    mrow = mask + base;
    mwide = row_is_wide(mrow);
  }
  int count = 0, last = -1, first_zero = NONE, first_bad = NONE;
  for (int j = lane * 4; j < width; j += 256) {
    const int n = min(4, width - j);
    IdT iv[4];
    load4(irow + j, iwide && n == 4, n, iv);
    bool on[4] = {true, true, true, true};
    if constexpr (HAS_MASK) {
      MaskT mv[4];
      load4(mrow + j, mwide && n == 4, n, mv);
#pragma unroll
      for (int k = 0; k < 4; ++k) on[k] = mv[k] != MaskT(0);
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      if (k >= n) break;
      if (on[k]) {
        ++count;
        last = j + k;
        // (one unsigned compare: a negative id sign-extends to a huge value)
        if ((uint64_t)(int64_t)iv[k] >= (uint64_t)vocab) first_bad = min(first_bad, j + k);
      } else {
        first_zero = min(first_zero, j + k);
      }
    }
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    count += __shfl_xor(count, off);
    last = max(last, __shfl_xor(last, off));
    first_zero = min(first_zero, __shfl_xor(first_zero, off));
    first_bad = min(first_bad, __shfl_xor(first_bad, off));
  }
  if (lane == 0) {
    len_out[r] = count;
    if (count != last + 1) atomicMin(status + PAD_ST_MASK, (uint32_t)(base + (size_t)first_zero));  // (first_zero < last here)
    if (first_bad != NONE) atomicMin(status + PAD_ST_ID, (uint32_t)(base + (size_t)first_bad));
  }
}

// 2. One block: cu[1 + r] holds len[r] on entry and the inclusive prefix sum on exit (cu[0] = 0), 1024 rows per step
// with a carry; total tokens, the longest row and the value of the first offending id go to the status block.
template <typename IdT>
__global__ __launch_bounds__(1024) void padded_scan_kernel(int32_t* __restrict__ cu, int n_rows, const IdT* __restrict__ ids,
                                                           uint32_t* __restrict__ status) {
  __shared__ int wave_sum[16], wave_max[16];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int carry = 0, longest = 0;  // (the same in every thread)
  for (int r0 = 0; r0 < n_rows; r0 += 1024) {
    const int r = r0 + tid;
    const int len = r < n_rows ? cu[1 + r] : 0;
    int sum = len, mx = len;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
      const int up = __shfl_up(sum, off);
      if (lane >= off) sum += up;
      mx = max(mx, __shfl_xor(mx, off));
    }
    if (lane == 63) wave_sum[wave] = sum;
    if (lane == 0) wave_max[wave] = mx;
    __syncthreads();
    int before = 0, step = 0;
#pragma unroll
    for (int w = 0; w < 16; ++w) {
      if (w < wave) before += wave_sum[w];
      step += wave_sum[w];
      longest = max(longest, wave_max[w]);
    }
    if (r < n_rows) cu[1 + r] = carry + before + sum;
    carry += step;
    __syncthreads();
  }
  if (tid == 0) {
    cu[0] = 0;
    status[PAD_ST_TOTAL] = (uint32_t)carry;
    status[PAD_ST_MAXLEN] = (uint32_t)longest;
    const uint32_t bad = status[PAD_ST_ID];
    const int64_t value = bad != PAD_ST_NONE ? (int64_t)ids[bad] : 0;
    status[PAD_ST_IDVAL] = (uint32_t)(uint64_t)value;
    status[PAD_ST_IDVAL + 1] = (uint32_t)((uint64_t)value >> 32);
  }
}

// 3. out[cu[r] + j] = (int32) ids[r][j] for j < len[r].  grid = (n_rows, column chunks): consecutive lanes read and
// write consecutive elements.
template <typename IdT>
__global__ __launch_bounds__(256) void padded_gather_kernel(const IdT* __restrict__ ids, const int32_t* __restrict__ cu, int width,
                                                            int32_t* __restrict__ out) {
  const int r = blockIdx.x;
  const int start = cu[r];
  const int len = min(cu[r + 1] - start, width);
  const IdT* row = ids + (size_t)r * (size_t)width;
  for (int j = blockIdx.y * 256 + threadIdx.x; j < len; j += gridDim.y * 256) out[start + j] = (int32_t)row[j];
}

// 4. Packed [T][C] fp32 -> padded [n_rows][width][C]: EVERY destination element is written, the value at col < len[r]
// and +0.0 beyond (no memset, no index tensors).  One thread per 4 consecutive destination floats -- 4 / C positions,
// which may straddle a row boundary -- stored as one 16-byte word when dst is 16-byte aligned (wide).
template <int C>
__global__ __launch_bounds__(256) void padded_scatter_kernel(const float* __restrict__ src, const int32_t* __restrict__ cu, int n_rows,
                                                             int width, float* __restrict__ dst, bool wide) {
  static_assert(C == 1 || C == 2, "channels");
  const size_t n = (size_t)n_rows * (size_t)width * C;
  const size_t e0 = ((size_t)blockIdx.x * 256 + threadIdx.x) * 4;
  if (e0 >= n) return;
  const uint32_t pos = (uint32_t)(e0 / C);  // (e0 is a multiple of 4: channel 0 of its position)
  int r = (int)(pos / (uint32_t)width), j = (int)(pos % (uint32_t)width), ch = 0;
  int start = cu[r], len = cu[r + 1] - start;
  float v[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    v[k] = 0.0f;
    if (e0 + k < n) {
      if (j < len) v[k] = src[((size_t)start + (size_t)j) * C + ch];
      if (++ch == C) {
        ch = 0;
        if (++j == width) {
          j = 0;
          if (++r < n_rows) {
            start = cu[r];
            len = cu[r + 1] - start;
          }
        }
      }
    }
  }
  if (wide && e0 + 4 <= n) {
    *reinterpret_cast<float4*>(dst + e0) = make_float4(v[0], v[1], v[2], v[3]);
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (e0 + k < n) dst[e0 + k] = v[k];
  }
}

}  // namespace opk
