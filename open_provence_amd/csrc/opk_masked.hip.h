// opk_masked.hip.h -- op_forward_masked_native: what a dense forward under an arbitrary [B, L] attention mask adds to the
// handle's SELECTED kernel set on the row and the panel path, beside the key-mask form of attn_fp_kernel (opk_attn.hip.h) and
// of the ranking head (rank_head_masked_kernel, opk_small.hip.h): the mask in the row layout, and the row means of v^T.
// Included by op_forward.hip only.  The semantics are those of opk_f32_masked.hip.h.
#pragma once

#include "opk_common.hip.h"

namespace opk {

// ----------------------------------------------------------------------------------------------
// key_row[r] = 1 where row r of the row layout is a position whose mask byte is not 0, else 0 (alignment rows, rows behind
// the chunk, masked positions).  EVERY byte of key_row[r_pad] is written.  key_ok is indexed like the ids (row_tok).
// ----------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void key_row_kernel(const uint8_t* __restrict__ key_ok, const int32_t* __restrict__ row_tok, int r_pad,
                                                      uint8_t* __restrict__ key_row) {
  const int r = blockIdx.x * 256 + threadIdx.x;
  if (r >= r_pad) return;
  const int tok = row_tok[r];
  key_row[r] = (tok >= 0 && key_ok[tok] != 0) ? (uint8_t)1 : (uint8_t)0;
}

// ----------------------------------------------------------------------------------------------
// vmean[s][f] = the mean over the sequence's positions of v[.][f] AS THE SET STORES IT, read from the fragment-packed v^T
// [head][row / 32][plane][n4][lane = 16 kg + d'][8]: element e of a lane is key 4 kg + e (e < 4) / 16 + 4 kg + e - 4 of the
// 32-row block, piece n4 and lane row d' hold head dim 32 (n4 >> 1) + 8 (d' >> 2) + 4 (n4 & 1) + (d' & 3) -- the order
// attn_fp_kernel's epilogue reads.  H16: one fp16 plane; else bf16, hi + lo where the set's attention reads a lo plane (V_LO).
// fp32 sums in a fixed order, as vmean_f32_kernel: partial sums of 16 positions (a lane's four, in order; then the four lanes of
// the granule as (kg, kg ^ 1) + (kg ^ 2, kg ^ 3), the same value in each) added in order of position, divided by the length.
// grid = (sequences, heads), 256 threads: wave n4, lane 16 kg + d' -- one lane-linear 16-byte load per plane and 32-row block.
// ----------------------------------------------------------------------------------------------
template <bool H16, bool V_LO>
__global__ __launch_bounds__(256) void vmean_fp_kernel(const u16* __restrict__ vt_fp, const int32_t* __restrict__ cu, int s0,
                                                       const int32_t* __restrict__ roff, int H, int r_pad, float* __restrict__ vmean) {
  const int s = blockIdx.x, head = blockIdx.y;
  const int lane = threadIdx.x & 63, n4 = threadIdx.x >> 6;
  const int kg = lane >> 4, dl = lane & 15;
  const int len = cu[s0 + s + 1] - cu[s0 + s];
  const int tb0 = roff[s] >> 5;
  auto value = [](uint32_t hi, uint32_t lo) -> float {
    if constexpr (H16) {
      return (float)__builtin_bit_cast(_Float16, (u16)hi);
    } else {
      const float h = __uint_as_float(hi << 16);
      return V_LO ? h + __uint_as_float(lo << 16) : h;
    }
  };
  float acc = 0.f;
  for (int tb = 0; tb * 32 < len; ++tb) {
    const u16* src = vt_fp + (((size_t)head * (size_t)(r_pad >> 5) + (size_t)(tb0 + tb)) * 2 * 4 + n4) * 512 + lane * 8;
    const uint4 h4 = *reinterpret_cast<const uint4*>(src);
    const uint4 l4 = V_LO ? *reinterpret_cast<const uint4*>(src + 2048) : make_uint4(0u, 0u, 0u, 0u);
    const uint32_t hw[4] = {h4.x, h4.y, h4.z, h4.w}, lw[4] = {l4.x, l4.y, l4.z, l4.w};
#pragma unroll
    for (int half = 0; half < 2; ++half) {  // positions 32 tb + 16 half + 0 .. 15: this lane holds 4 kg + 0 .. 3 of them
      float part = 0.f;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int pos = 32 * tb + 16 * half + 4 * kg + e;
        const int j = 4 * half + e;  // element of the lane's eight
        const uint32_t hi = (hw[j >> 1] >> (16 * (j & 1))) & 0xffffu, lo = (lw[j >> 1] >> (16 * (j & 1))) & 0xffffu;
        if (pos < len) part += value(hi, lo);
      }
      part += __shfl_xor(part, 16, 64);
      part += __shfl_xor(part, 32, 64);
      acc += part;
    }
  }
  if (kg == 0) vmean[(size_t)s * H + head * 64 + 32 * (n4 >> 1) + 8 * (dl >> 2) + 4 * (n4 & 1) + (dl & 3)] = len > 0 ? acc / (float)len : 0.f;
}

}  // namespace opk
