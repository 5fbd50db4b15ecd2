// opk_pool.hip.h -- op_forward_packed_pooled: one entry of the hidden states, stored by the forward's own stores into a packed
// fp32 scratch entry [total_tokens][H], reduced to one row per sequence.  Two kernels of its own:
//   pool_hidden_kernel    scratch -> out[s][H]: the row of token 0 (POOL_FIRST, a copy: the same bits), or the mean over the
//                         sequence's tokens (POOL_MEAN)
//   hidden_repack_kernel  scratch -> the entry of an ordinary hidden-state request that rides on the same call, in its dtype and
//                         layout (the stores have one destination per launch)
// POOL_MEAN, per (sequence, feature): fp64 partials over POOL_PARTIAL consecutive tokens each, added in token order; the
// partials added in index order; one fp64 division by the length; one rounding to fp32.  No atomics, no order that depends
// on the grid, the batch or the chunk: a sequence's row depends on its own tokens only, so the same bits come out on every
// call, on every stream, under every batch composition and every chunking (the rule of opk_loss.hip.h).  A sequence of length
// 0 gives +0.0 under both kinds.  Every element of the rows [s0, s0 + gridDim.x) is written.
#pragma once

#include "opk_small.hip.h"

namespace opk {

constexpr int POOL_FIRST = 0, POOL_MEAN = 1;  // = enum op_pool_kind
constexpr int POOL_PARTIAL = 64;              // tokens per fp64 partial
constexpr int POOL_COLS = 64;                 // features per block: one per lane, a 256-byte row segment per wave load

// grid (sequences of the chunk, H / POOL_COLS), 256 threads: wave w adds partial 4 i + w of round i, wave 0 adds the round's
// four partials to the running total in index order.  Token bounds are held inside [0, total_tokens) whatever cu holds.
__global__ __launch_bounds__(256) void pool_hidden_kernel(const float* __restrict__ src, const int32_t* __restrict__ cu, int s0,
                                                          int total_tokens, int H, int kind, float* __restrict__ out) {
  __shared__ double part[4][POOL_COLS];
  const int s = s0 + (int)blockIdx.x;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int col = (int)blockIdx.y * POOL_COLS + lane;
  const bool live = col < H;
  const int start = max(cu[s], 0);
  const int len = min(cu[s + 1], total_tokens) - start;
  float* __restrict__ dst = out + (size_t)s * (size_t)H + col;
  if (kind != POOL_MEAN || len <= 0) {  // (block-uniform)
    if (wave == 0 && live) *dst = len > 0 ? src[(size_t)start * (size_t)H + col] : 0.f;
    return;
  }
  const float* __restrict__ from = src + (size_t)start * (size_t)H + col;
  double total = 0.0;
  for (int base = 0; base < len; base += 4 * POOL_PARTIAL) {
    const int t0 = base + wave * POOL_PARTIAL;
    const int t1 = min(t0 + POOL_PARTIAL, len);
    double acc = 0.0;
    if (live) {
#pragma unroll 8
      for (int t = t0; t < t1; ++t) acc += (double)from[(size_t)t * (size_t)H];
    }
    part[wave][lane] = acc;
    __syncthreads();
    if (wave == 0) {
#pragma unroll
      for (int w = 0; w < 4; ++w)
        if (base + w * POOL_PARTIAL < len) total += part[w][lane];
    }
    __syncthreads();  // the next round overwrites `part`
  }
  if (wave == 0 && live) *dst = (float)(total / (double)len);
}

// One wave per row of the row map: the packed fp32 scratch row of a real token -> the request's entry, as hidden_rows_kernel
// stores it (the same rounding to bf16, the same destination row).
__global__ __launch_bounds__(256) void hidden_repack_kernel(const float* __restrict__ src, int H, int r_pad, const int32_t* __restrict__ row_tok,
                                                            const int32_t* __restrict__ row_seq, const int32_t* __restrict__ row_pos, int s0,
                                                            int pad, int bf16, void* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= r_pad) return;
  const int tok = row_tok[row];
  if (tok < 0) return;
  RowVec rv;
  row_load(src + (size_t)tok * H, H, lane, rv);
  const size_t base = hidden_dst_row(tok, row_seq[row], row_pos[row], pad, s0) * (size_t)H;
  const int nchunk = H >> 2;
#pragma unroll
  for (int k = 0; k < LN_MAX_CHUNKS; ++k) {
    const int c = lane + 64 * k;
    if (c < nchunk) hidden_store4(out, bf16, base + 4 * c, rv.v[k].x, rv.v[k].y, rv.v[k].z, rv.v[k].w);
  }
}

}  // namespace opk
