// opk_attn_probs.hip.h -- op_attention_probs: the softmax probabilities of one layer as a side pass over that layer's input
// hidden state.  Two kernels of its own -- the gather of a packed fp32 state into the row layout of opk_common.hip.h and the
// probability kernel -- beside ln_f32_kernel and gemm_f32_kernel<F32_EPI_QKV> of kernel set "fp32" (opk_f32.hip.h), whose
// arithmetic the pass uses whatever set the handle's forward runs on.  op_attention_rows (one query row per sequence, per head or
// as the mean over heads) is a third kernel, attn_rows_f32_kernel, built from the probability kernel's own device functions.
//
// Composition invariance: a probability depends on its own sequence only (no atomics, no split sums, one k order).
//
// The parameter struct is visible to every unit (op_internal.h); the kernels only where OPK_ATTN_PROBS_KERNELS is defined
// (op_launch_attn_probs.hip).
#pragma once

#include "opk_common.hip.h"

namespace opk {

struct AttnProbsParams {
  const float* q;  // [r_pad][H], RoPE applied, scaled by head_dim^-0.5 (gemm_f32_kernel<F32_EPI_QKV>)
  const float* k;  // [r_pad][H], RoPE applied
  float* out;      // [n_seqs of the batch][num_heads][width][width]
  const int32_t* cu;
  int s0;          // first sequence of the chunk: blockIdx.z = s - s0
  const int32_t* roff;
  int H;
  int num_heads;
  int window;  // < 0: full attention; else keys with |q - k| <= window
  int width;   // pad_width: rows and columns of one (sequence, head) matrix
  int wide;    // width % 4 == 0 and `out` 16-byte aligned: every row segment is stored as 16-byte words
};

// op_attention_rows: one query row per sequence (attn_rows_f32_kernel)
struct AttnRowsParams {
  const float* q;  // as AttnProbsParams
  const float* k;
  float* out;           // [n_seqs of the batch][num_heads][width], or [n_seqs of the batch][width] (head mean)
  const int32_t* cu;
  const int32_t* qpos;  // [n_seqs of the batch] query position per sequence, or nullptr = position 0
  int s0;
  const int32_t* roff;
  int H;
  int num_heads;
  int window;
  int width;
};
constexpr int AR_MAX_HEADS = 64;  // head mean: the heads' row maxima and sums wait in LDS

#ifdef OPK_ATTN_PROBS_KERNELS

constexpr int AP_LDS = 68;  // LDS row stride of a 64-float row (64 + 4 pad: 16-byte aligned rows; K fragments and the staged tile read conflict-free)

__device__ __forceinline__ f32x4 ap_mfma_f32(float x, float y, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(x, y, c, 0, 0, 0); }

// ----------------------------------------------------------------------------------------------
// packed [total_tokens][H] fp32 -> the row layout [r_pad][H]: row r holds token row_tok[r], zeros where row_tok[r] < 0
// (alignment rows and the rows behind the chunk).  One wave per row.
// ----------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void gather_rows_f32_kernel(const float* __restrict__ src, const int32_t* __restrict__ row_tok, int H,
                                                              int r_pad, float* __restrict__ x) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= r_pad) return;
  const int tok = row_tok[row];
  float4* dst = reinterpret_cast<float4*>(x + (size_t)row * H);
  const float4* from = reinterpret_cast<const float4*>(src + (size_t)(tok < 0 ? 0 : tok) * H);
  for (int c = lane; c < (H >> 2); c += 64) dst[c] = tok >= 0 ? from[c] : make_float4(0.f, 0.f, 0.f, 0.f);
}

// One 64-key tile of K into LDS (keys at or beyond `len` as zeros: never read from memory), then S^T = K Q^T for this wave's 16
// queries, masked: element (m, r) of a lane = key kbase + 16 m + 4 g + r of query qpos; a key the query does not see is -3e30.
// Exactly the staging, the MFMA order and the mask of attn_f32_kernel.
__device__ __forceinline__ void ap_score_tile(const float* __restrict__ k, int H, float* sK, const f32x4 (&qf)[4], int r0, int hcol, int len,
                                              int kbase, int qpos, int win, f32x4 (&sacc)[4]) {
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int l15 = lane & 15;
  const int g = lane >> 4;
  const int prow = tid >> 4;
  const int pcol = (tid & 15) * 4;
  __syncthreads();  // previous tile fully consumed
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const int row = prow + 16 * u;
    float4 kv = make_float4(0.f, 0.f, 0.f, 0.f);
    if (kbase + row < len) kv = *reinterpret_cast<const float4*>(k + (size_t)(r0 + kbase + row) * H + hcol + pcol);
    *reinterpret_cast<float4*>(&sK[row * AP_LDS + pcol]) = kv;
  }
  __syncthreads();
#pragma unroll
  for (int m = 0; m < 4; ++m) sacc[m] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    f32x4 kf[4];
#pragma unroll
    for (int m = 0; m < 4; ++m) kf[m] = *reinterpret_cast<const f32x4*>(&sK[(m * 16 + l15) * AP_LDS + t * 16 + g * 4]);
#pragma unroll
    for (int e = 0; e < 4; ++e)
#pragma unroll
      for (int m = 0; m < 4; ++m) sacc[m] = ap_mfma_f32(kf[m][e], qf[t][e], sacc[m]);
  }
#pragma unroll
  for (int m = 0; m < 4; ++m) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int key = kbase + 16 * m + 4 * g + r;
      const int d = key - qpos;
      const bool ok = (key < len) & (d <= win) & (d >= -win);
      sacc[m][r] = ok ? sacc[m][r] : -3e30f;
    }
  }
}

// Pass 1 of a query row: the running maximum and the running sum of attn_f32_kernel over the key tiles kt_lo .. kt_hi, in
// that order, nothing else.  m_run is the row maximum, l_tot the sum of expf(s - m_run) over the row's keys (a lane's 16 keys
// per tile first, then the four lanes of the query column); both are the same in the four lanes that share a query.
__device__ __forceinline__ void ap_row_stats(const float* __restrict__ k, int H, float* sK, const f32x4 (&qf)[4], int r0, int hcol, int len,
                                             int kt_lo, int kt_hi, int qpos, int win, f32x4 (&sacc)[4], float& m_out, float& l_out) {
  float m_run = -1e30f;
  float l_run = 0.f;
  for (int kt = kt_lo; kt <= kt_hi; ++kt) {
    ap_score_tile(k, H, sK, qf, r0, hcol, len, kt * ATT_BK, qpos, win, sacc);
    float tile_max = -3e30f;
#pragma unroll
    for (int m = 0; m < 4; ++m)
#pragma unroll
      for (int r = 0; r < 4; ++r) tile_max = fmaxf(tile_max, sacc[m][r]);
    tile_max = fmaxf(tile_max, __shfl_xor(tile_max, 16, 64));
    tile_max = fmaxf(tile_max, __shfl_xor(tile_max, 32, 64));
    const float m_new = fmaxf(m_run, tile_max);
    const float alpha = expf(m_run - m_new);
    m_run = m_new;
    float psum = 0.f;
#pragma unroll
    for (int m = 0; m < 4; ++m)
#pragma unroll
      for (int r = 0; r < 4; ++r) psum += expf(sacc[m][r] - m_new);
    l_run = l_run * alpha + psum;
  }
  float l_tot = l_run + __shfl_xor(l_run, 16, 64);
  l_tot += __shfl_xor(l_tot, 32, 64);
  m_out = m_run;
  l_out = l_tot;
}

// Pass 2, one element: the probability of a score under the row's maximum and sum
__device__ __forceinline__ float ap_prob(float s, float m_run, float l_tot) { return expf(s - m_run) / l_tot; }

// 16 query rows x 64 key columns of zeros at (row0, kbase) of one (sequence, head) matrix: whole 256-byte row segments
__device__ __forceinline__ void ap_store_zero_tile(float* __restrict__ mat, int width, bool wide, int row0, int kbase, int lane) {
  if (wide) {
    const int col = kbase + (lane & 15) * 4;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int row = row0 + u * 4 + (lane >> 4);
      if (row < width && col < width) *reinterpret_cast<float4*>(mat + (size_t)row * width + col) = make_float4(0.f, 0.f, 0.f, 0.f);
    }
  } else {
    const int col = kbase + lane;
    for (int u = 0; u < 16; ++u) {
      const int row = row0 + u;
      if (row < width && col < width) mat[(size_t)row * width + col] = 0.f;
    }
  }
}

// ----------------------------------------------------------------------------------------------
// out[s][head][i][j] = softmax_j(q_i . k_j) over the keys query i sees, fp32.  The block map of attn_f32_kernel: 64 queries
// of one (sequence, head), 16 per wave, on 64-key tiles, S^T = K Q^T on v_mfma_f32_16x16x4_f32.  Two passes over the visible
// key tiles: the first keeps the running maximum m and the running sum l only, the second computes each score tile again
// (the same instructions: the same bits) and stores expf(s - m) / l.  In the MFMA's C layout a lane holds 4 consecutive keys
// of ONE query and its neighbour lanes are a whole output row apart, so every 16-query x 64-key tile goes through LDS (one
// region per wave) and leaves as 256-byte row segments, 16 bytes per lane, consecutive lanes on consecutive keys.
//
// EVERY element of the [width][width] matrix is written by this launch: +0.0 at keys the query does not see (masked, beyond
// the sequence, tiles outside a sliding window -- those are not computed), on query rows at or beyond the sequence's length,
// and out to `width` both ways.  The grid covers ceil(width / 64) query blocks and no block returns early.
// width % 4 != 0 (or an unaligned `out`): rows do not start on 16-byte boundaries; the segments are then stored as dwords, still
// consecutive lanes on consecutive keys.
// ----------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256, 2) void attn_probs_f32_kernel(AttnProbsParams p) {
  __shared__ __attribute__((aligned(16))) float sK[ATT_BK * AP_LDS];
  __shared__ __attribute__((aligned(16))) float sP[4 * 16 * AP_LDS];

  const int s = blockIdx.z;
  const int head = blockIdx.y;
  const int q0 = blockIdx.x * ATT_BQ;
  const int seq_start = p.cu[p.s0 + s];
  const int len = p.cu[p.s0 + s + 1] - seq_start;
  const int r0 = p.roff[s];
  const int alloc = p.roff[s + 1] - r0;

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int l15 = lane & 15;
  const int g = lane >> 4;
  const int width = p.width;
  const bool wide = p.wide != 0;
  const int hcol = head * HEAD_DIM;
  const int qbase = q0 + wave * 16;
  float* __restrict__ mat = p.out + ((size_t)(p.s0 + s) * p.num_heads + head) * (size_t)width * (size_t)width;
  const int n_kt = (width + ATT_BK - 1) / ATT_BK;  // key tiles of an output row

  if (q0 >= len) {  // padding rows only: zeros across the whole width
    for (int kt = 0; kt < n_kt; ++kt) ap_store_zero_tile(mat, width, wide, qbase, kt * ATT_BK, lane);
    return;
  }

  const bool active = qbase < alloc;  // alloc is a multiple of 16: whole wave in or out (an inactive wave's rows are >= len: zeros)
  const int qpos = qbase + l15;
  const size_t qrow = (size_t)(r0 + (active ? qpos : q0));
  f32x4 qf[4];  // d = 16 t + 4 g + e
#pragma unroll
  for (int t = 0; t < 4; ++t) qf[t] = *reinterpret_cast<const f32x4*>(p.q + qrow * p.H + hcol + t * 16 + g * 4);

  int kt_lo = 0, kt_hi = (len - 1) / ATT_BK;
  if (p.window >= 0) {
    const int lo_key = q0 - p.window;
    kt_lo = lo_key > 0 ? lo_key / ATT_BK : 0;
    const int hi_t = (q0 + ATT_BQ - 1 + p.window) / ATT_BK;
    kt_hi = hi_t < kt_hi ? hi_t : kt_hi;
  }
  const int win = p.window >= 0 ? p.window : (1 << 30);

  // pass 1: the running maximum and the running sum of attn_f32_kernel, nothing else
  float m_run, l_tot;
  f32x4 sacc[4];
  ap_row_stats(p.k, p.H, sK, qf, r0, hcol, len, kt_lo, kt_hi, qpos, win, sacc, m_run, l_tot);
  const bool real = qpos < len;  // (a real query sees itself: l_tot >= 1)

  // pass 2: every key tile of the output row -- computed and staged through LDS inside [kt_lo, kt_hi], zeros outside
  float* tile = sP + wave * 16 * AP_LDS;
  for (int kt = 0; kt < n_kt; ++kt) {
    const int kbase = kt * ATT_BK;
    if (kt < kt_lo || kt > kt_hi) {
      ap_store_zero_tile(mat, width, wide, qbase, kbase, lane);
      continue;
    }
    ap_score_tile(p.k, p.H, sK, qf, r0, hcol, len, kbase, qpos, win, sacc);
    // (the first barrier of ap_score_tile stands between the previous tile's reads of `tile` and these writes)
#pragma unroll
    for (int m = 0; m < 4; ++m) {
      float4 pv;
      pv.x = real ? ap_prob(sacc[m][0], m_run, l_tot) : 0.f;
      pv.y = real ? ap_prob(sacc[m][1], m_run, l_tot) : 0.f;
      pv.z = real ? ap_prob(sacc[m][2], m_run, l_tot) : 0.f;
      pv.w = real ? ap_prob(sacc[m][3], m_run, l_tot) : 0.f;
      *reinterpret_cast<float4*>(&tile[l15 * AP_LDS + 16 * m + 4 * g]) = pv;
    }
    __syncthreads();
    if (wide) {
      const int col = kbase + l15 * 4;
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int lr = u * 4 + g;
        const int row = qbase + lr;
        if (row < width && col < width)
          *reinterpret_cast<float4*>(mat + (size_t)row * width + col) = *reinterpret_cast<const float4*>(&tile[lr * AP_LDS + l15 * 4]);
      }
    } else {
      const int col = kbase + lane;
      for (int lr = 0; lr < 16; ++lr) {
        const int row = qbase + lr;
        if (row < width && col < width) mat[(size_t)row * width + col] = tile[lr * AP_LDS + lane];
      }
    }
  }
}

// ----------------------------------------------------------------------------------------------
// op_attention_rows: ONE query row per sequence.  MEAN = false: out[s][head][j] = row qpos[s] of the [width][width] matrix
// attn_probs_f32_kernel writes for (s, head), bit for bit -- the same visible key tiles in the same order (those of the
// 64-query block the position lies in), through ap_score_tile / ap_row_stats / ap_prob.  The block is the full kernel's (256
// threads stage a key tile); every column of the 16-query fragment holds the selected query, so every wave computes the row
// and wave 0 stores it: a column of the MFMA depends on its own query only.  grid (1, num_heads, sequences).
// MEAN = true: out[s][j] = the mean over heads of those fp32 probabilities, fp64 in head order, one division, one rounding.
// grid (x, 1, sequences): pass 1 of every head first (maximum and sum kept in LDS, num_heads <= AR_MAX_HEADS), then per key
// tile the heads in order.  Block x of gridDim.x takes the key tiles x, x + gridDim.x, ... of the output row (pass 1 is then
// repeated per block): an element's arithmetic does not depend on the split, which only spreads a small batch over the chip.
// EVERY element of a row is written: +0.0 at keys the query does not see and out to `width`; the whole row +0.0 when the
// position is negative or at or beyond the sequence's length (an empty sequence included) -- the position is compared before
// it is used as an index.
// ----------------------------------------------------------------------------------------------
template <bool MEAN>
__global__ __launch_bounds__(256, 2) void attn_rows_f32_kernel(AttnRowsParams p) {
  __shared__ __attribute__((aligned(16))) float sK[ATT_BK * AP_LDS];
  __shared__ float sM[MEAN ? AR_MAX_HEADS : 1];
  __shared__ float sL[MEAN ? AR_MAX_HEADS : 1];

  const int s = blockIdx.z;
  const int seq_start = p.cu[p.s0 + s];
  const int len = p.cu[p.s0 + s + 1] - seq_start;
  const int r0 = p.roff[s];
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int l15 = lane & 15;
  const int g = lane >> 4;
  const int width = p.width;
  float* __restrict__ dst = p.out + (MEAN ? (size_t)(p.s0 + s) : (size_t)(p.s0 + s) * p.num_heads + blockIdx.y) * (size_t)width;

  const int qpos = p.qpos ? p.qpos[p.s0 + s] : 0;
  if (qpos < 0 || qpos >= len) {  // (block-uniform) no such query: zeros across the whole width
    if (!MEAN || blockIdx.x == 0)
      for (int j = tid; j < width; j += 256) dst[j] = 0.f;
    return;
  }

  const int q0 = qpos / ATT_BQ * ATT_BQ;  // the query block of the full pass: its key tile range is the one walked here
  int kt_lo = 0, kt_hi = (len - 1) / ATT_BK;
  if (p.window >= 0) {
    const int lo_key = q0 - p.window;
    kt_lo = lo_key > 0 ? lo_key / ATT_BK : 0;
    const int hi_t = (q0 + ATT_BQ - 1 + p.window) / ATT_BK;
    kt_hi = hi_t < kt_hi ? hi_t : kt_hi;
  }
  const int win = p.window >= 0 ? p.window : (1 << 30);
  const int n_kt = (width + ATT_BK - 1) / ATT_BK;
  const size_t qrow = (size_t)(r0 + qpos);
  const bool writer = wave == 0 && l15 == 0;  // four lanes (g), 16 keys of every tile each

  f32x4 qf[4];  // d = 16 t + 4 g + e
  f32x4 sacc[4];
  if constexpr (!MEAN) {
    const int hcol = (int)blockIdx.y * HEAD_DIM;
#pragma unroll
    for (int t = 0; t < 4; ++t) qf[t] = *reinterpret_cast<const f32x4*>(p.q + qrow * p.H + hcol + t * 16 + g * 4);
    float m_run, l_tot;
    ap_row_stats(p.k, p.H, sK, qf, r0, hcol, len, kt_lo, kt_hi, qpos, win, sacc, m_run, l_tot);
    for (int kt = 0; kt < n_kt; ++kt) {
      const int kbase = kt * ATT_BK;
      const bool seen = kt >= kt_lo && kt <= kt_hi;
      if (seen) ap_score_tile(p.k, p.H, sK, qf, r0, hcol, len, kbase, qpos, win, sacc);
      if (writer) {
#pragma unroll
        for (int m = 0; m < 4; ++m)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int col = kbase + 16 * m + 4 * g + r;
            if (col < width) dst[col] = seen ? ap_prob(sacc[m][r], m_run, l_tot) : 0.f;
          }
      }
    }
  } else {
    for (int head = 0; head < p.num_heads; ++head) {
      const int hcol = head * HEAD_DIM;
#pragma unroll
      for (int t = 0; t < 4; ++t) qf[t] = *reinterpret_cast<const f32x4*>(p.q + qrow * p.H + hcol + t * 16 + g * 4);
      float m_run, l_tot;
      ap_row_stats(p.k, p.H, sK, qf, r0, hcol, len, kt_lo, kt_hi, qpos, win, sacc, m_run, l_tot);
      if (tid == 0) {  // (every lane holds the same pair)
        sM[head] = m_run;
        sL[head] = l_tot;
      }
    }
    __syncthreads();
    for (int kt = (int)blockIdx.x; kt < n_kt; kt += (int)gridDim.x) {
      const int kbase = kt * ATT_BK;
      const bool seen = kt >= kt_lo && kt <= kt_hi;
      double acc[16];
#pragma unroll
      for (int i = 0; i < 16; ++i) acc[i] = 0.0;
      if (seen) {
        for (int head = 0; head < p.num_heads; ++head) {
          const int hcol = head * HEAD_DIM;
#pragma unroll
          for (int t = 0; t < 4; ++t) qf[t] = *reinterpret_cast<const f32x4*>(p.q + qrow * p.H + hcol + t * 16 + g * 4);
          ap_score_tile(p.k, p.H, sK, qf, r0, hcol, len, kbase, qpos, win, sacc);
          const float m_run = sM[head], l_tot = sL[head];
#pragma unroll
          for (int m = 0; m < 4; ++m)
#pragma unroll
            for (int r = 0; r < 4; ++r) acc[4 * m + r] += (double)ap_prob(sacc[m][r], m_run, l_tot);
        }
      }
      if (writer) {
#pragma unroll
        for (int m = 0; m < 4; ++m)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int col = kbase + 16 * m + 4 * g + r;
            if (col < width) dst[col] = seen ? (float)(acc[4 * m + r] / (double)p.num_heads) : 0.f;
          }
      }
    }
  }
}

#endif  // OPK_ATTN_PROBS_KERNELS

}  // namespace opk
