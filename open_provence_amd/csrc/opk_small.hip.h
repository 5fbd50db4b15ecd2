// opk_small.hip.h -- row map, embeddings, hidden-state stores, heads: the forward's non-GEMM kernels (included by op_forward.hip
// only, which also takes opk_pool.hip.h).  The LayerNorm launches of the layers: opk_layernorm.hip.h; weight loading:
// opk_load.hip.h.
#pragma once

#include "opk_common.hip.h"
#include "opk_rowvec.hip.h"

namespace opk {

// ----------------------------------------------------------------------------------------------
// row map: sequence offsets (aligned) and per-row (seq, pos, token index)
// ----------------------------------------------------------------------------------------------
// roff[i] = sum_{j<i} ceil(len_j / unit) * scale  (exclusive prefix; roff[ns] = total).  unit = scale = ROW_ALIGN gives
// the aligned row offsets, unit = queries per attention block with scale = 1 the first work item of each sequence.
__global__ __launch_bounds__(1024) void seq_offsets_kernel(const int32_t* __restrict__ cu, int s0, int ns, int unit,
                                                           int scale, int32_t* __restrict__ roff) {
  __shared__ int sh[1024];
  __shared__ int carry;
  const int tid = threadIdx.x;
  if (tid == 0) carry = 0;
  __syncthreads();
  for (int base = 0; base < ns; base += 1024) {
    const int i = base + tid;
    int v = 0;
    if (i < ns) {
      const int len = cu[s0 + i + 1] - cu[s0 + i];
      v = (len + unit - 1) / unit * scale;
    }
    sh[tid] = v;
    __syncthreads();
    for (int off = 1; off < 1024; off <<= 1) {
      const int t = tid >= off ? sh[tid - off] : 0;
      __syncthreads();
      sh[tid] += t;
      __syncthreads();
    }
    const int incl = sh[tid];
    const int c = carry;
    if (i < ns) roff[i] = c + incl - v;
    __syncthreads();
    if (tid == 1023) carry = c + incl;
    __syncthreads();
  }
  if (tid == 0) roff[ns] = carry;
}

__global__ void row_map_kernel(const int32_t* __restrict__ cu, int s0, int ns, const int32_t* __restrict__ roff,
                               int r_pad, int32_t* __restrict__ row_seq, int32_t* __restrict__ row_pos,
                               int32_t* __restrict__ row_tok) {
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= r_pad) return;
  const int total = roff[ns];
  if (r >= total) {
    row_seq[r] = -1;
    row_pos[r] = -1;
    row_tok[r] = -1;
    return;
  }
  int lo = 0, hi = ns - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (roff[mid] <= r) lo = mid; else hi = mid - 1;
  }
  const int pos = r - roff[lo];
  const int start = cu[s0 + lo];
  const int len = cu[s0 + lo + 1] - start;
  row_seq[r] = lo;
  if (pos < len) {
    row_pos[r] = pos;
    row_tok[r] = start + pos;
  } else {
    row_pos[r] = -1;
    row_tok[r] = -1;
  }
}

// x0 = LN(E[id]) -> residual stream (fp32) and, because layer 0 has attn_norm = Identity
// (modeling_modernbert.py:309-312), directly the Wqkv operand planes.  Alignment rows get zeros.
template <bool SPLIT>
__global__ __launch_bounds__(256) void embed_ln_kernel(const int32_t* __restrict__ ids,
                                                       const int32_t* __restrict__ row_tok,
                                                       const float* __restrict__ table, const float* __restrict__ lnw,
                                                       float eps, int H, int r_pad, int vocab, float* __restrict__ x,
                                                       u16* __restrict__ a_hi, u16* __restrict__ a_lo) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= r_pad) return;
  const int tok = row_tok[row];
  RowVec rv;
  if (tok < 0) {
#pragma unroll
    for (int k = 0; k < LN_MAX_CHUNKS; ++k) rv.v[k] = make_float4(0.f, 0.f, 0.f, 0.f);
  } else {
    int id = ids[tok];
    id = id < 0 ? 0 : (id >= vocab ? vocab - 1 : id);
    row_load(table + (size_t)id * H, H, lane, rv);
    row_layer_norm(rv, lnw, H, lane, eps);
  }
  row_store_f32(rv, x + (size_t)row * H, H, lane);
  row_store_planes<SPLIT>(rv, a_hi + (size_t)row * H, a_lo + (size_t)row * H, H, lane);
}

// test hook: copy the residual stream rows of real tokens to the caller's packed [T, H] layout
__global__ __launch_bounds__(256) void capture_rows_kernel(const float* __restrict__ x,
                                                           const int32_t* __restrict__ row_tok, int H, int r_pad,
                                                           float* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= r_pad) return;
  const int tok = row_tok[row];
  if (tok < 0) return;
  RowVec rv;
  row_load(x + (size_t)row * H, H, lane, rv);
  row_store_f32(rv, out + (size_t)tok * H, H, lane);
}

// One entry of a per-call hidden-state request (op_forward_packed_hidden): the residual stream rows of real tokens to the
// request's output in its dtype (fp32 / bf16) and layout (token order, or [s0 + seq][pad][H]).  lnw != nullptr: the row goes
// through final_norm first, with final_ln_prune_kernel's arithmetic.
__global__ __launch_bounds__(256) void hidden_rows_kernel(const float* __restrict__ x, const float* __restrict__ lnw, float eps,
                                                          int H, int r_pad, const int32_t* __restrict__ row_tok,
                                                          const int32_t* __restrict__ row_seq, const int32_t* __restrict__ row_pos,
                                                          int s0, int pad, int bf16, void* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= r_pad) return;
  const int tok = row_tok[row];
  if (tok < 0) return;
  RowVec rv;
  row_load(x + (size_t)row * H, H, lane, rv);
  if (lnw) row_layer_norm(rv, lnw, H, lane, eps);
  const size_t base = hidden_dst_row(tok, row_seq[row], row_pos[row], pad, s0) * (size_t)H;
  const int nchunk = H >> 2;
#pragma unroll
  for (int k = 0; k < LN_MAX_CHUNKS; ++k) {
    const int c = lane + 64 * k;
    if (c < nchunk) hidden_store4(out, bf16, base + 4 * c, rv.v[k].x, rv.v[k].y, rv.v[k].z, rv.v[k].w);
  }
}

// final_norm + OpenProvenceHead Linear(H, 2) on every real token (standalone.py:446-448); keeps the
// normalised row for the ranking head (CLS row or, for mean pooling, every row -- written over x).
// pre_norm: the pruning head reads the row BEFORE final_norm (hidden_states[-1] of transformers 4.x, see
// op_config.prune_pre_final_norm).  keep_prob (optional) = softmax(logits)[1] = sigmoid(l1 - l0)
// (standalone.py:2918-2924 computes it on the host after the D2H copy).
__global__ __launch_bounds__(256) void final_ln_prune_kernel(float* __restrict__ x, const float* __restrict__ lnw,
                                                             float eps, int H, int r_pad,
                                                             const int32_t* __restrict__ row_tok,
                                                             const int32_t* __restrict__ row_seq,
                                                             const int32_t* __restrict__ row_pos,
                                                             const float* __restrict__ pw, const float* __restrict__ pb,
                                                             float* __restrict__ prune_out, float* __restrict__ keep_prob,
                                                             int pre_norm, int keep_all_rows, float* __restrict__ cls,
                                                             float* __restrict__ capture, const int* __restrict__ range_flag) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= r_pad) return;
  const int tok = row_tok[row];
  if (tok < 0) return;
  RowVec rv;
  row_load(x + (size_t)row * H, H, lane, rv);
  const int nchunk = H >> 2;
  float d0 = 0.f, d1 = 0.f;
  auto head_dot = [&]() {
#pragma unroll
    for (int k = 0; k < LN_MAX_CHUNKS; ++k) {
      const int c = lane + 64 * k;
      if (c < nchunk) {
        const float4 w0 = reinterpret_cast<const float4*>(pw)[c];
        const float4 w1 = reinterpret_cast<const float4*>(pw + H)[c];
        d0 += (rv.v[k].x * w0.x + rv.v[k].y * w0.y) + (rv.v[k].z * w0.z + rv.v[k].w * w0.w);
        d1 += (rv.v[k].x * w1.x + rv.v[k].y * w1.y) + (rv.v[k].z * w1.z + rv.v[k].w * w1.w);
      }
    }
  };
  if (pre_norm) head_dot();
  row_layer_norm(rv, lnw, H, lane, eps);
  if (!pre_norm) head_dot();
  d0 = wave_sum(d0);
  d1 = wave_sum(d1);
  if (lane == 0) {
    // range_flag: see rank_head_kernel -- the pruning logits of a flagged chunk leave as NaN too
    const float poison = (range_flag != nullptr && *range_flag != 0) ? __builtin_nanf("") : 0.f;
    const float l0 = d0 + pb[0] + poison, l1 = d1 + pb[1] + poison;
    prune_out[(size_t)tok * 2 + 0] = l0;
    prune_out[(size_t)tok * 2 + 1] = l1;
    if (keep_prob) keep_prob[tok] = keep_prob_of(l0, l1);
  }
  if (keep_all_rows) row_store_f32(rv, x + (size_t)row * H, H, lane);
  if (row_pos[row] == 0) row_store_f32(rv, cls + (size_t)row_seq[row] * H, H, lane);
  if (capture) row_store_f32(rv, capture + (size_t)tok * H, H, lane);
}

// ModernBertPredictionHead + classifier on the pooled row (modeling_modernbert.py:481-490, 609-622):
// logits = classifier(LN(gelu(dense(pooled)))).  One block per sequence; dense weight stored
// transposed [k][n] so that thread n reads coalesced.
__device__ __forceinline__ float block_sum_256(float v, float* red) {
  v = wave_sum(v);
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  __syncthreads();
  if (lane == 0) red[wave] = v;
  __syncthreads();
  return (red[0] + red[1]) + (red[2] + red[3]);
}

// KM (rank_head_masked_kernel: a dense batch under a key mask, key_ok[total_tokens] indexed like the ids): mean pooling sums
// the positions in the same order, a masked one contributing +0.0f, and divides by the number of valid positions -- under a
// prefix mask the bits of the packed row; cls pooling reads column 0 whatever its mask says (the reference pools it).  A
// sequence without a valid position gives zeros, as an empty one does.
template <bool KM>
__device__ __forceinline__ void rank_head_body(const float* __restrict__ cls, const float* __restrict__ y,
                                               const int32_t* __restrict__ cu, int s0, const int32_t* __restrict__ roff,
                                               const uint8_t* __restrict__ key_ok, int mean_pool, int H, int nl,
                                               const float* __restrict__ dense_t, const float* __restrict__ head_norm, float eps,
                                               const float* __restrict__ cls_w, const float* __restrict__ cls_b,
                                               float* __restrict__ rank_out, const int* __restrict__ range_flag) {
  // range_flag (may be NULL): raised by a kernel of the fp16 + e4m3 format that met an activation beyond fp16's range (or a
  // non-finite one) where the format cannot say so itself -- under MODE.FP16_OVFL = 1 conversions clamp and the fp16 MFMA
  // takes a NaN operand for a finite number (microbench/mode_probe.hip).  The ranking logits of the chunk then leave as NaN:
  // the same signal as an Inf that travelled through the residual stream, which the callers' range guard acts on.
  const bool poisoned = range_flag != nullptr && *range_flag != 0;
  __shared__ float pooled[1024];
  __shared__ float z[1024];
  __shared__ float red[4];
  const int s = blockIdx.x;
  const int tid = threadIdx.x;
  const int len = cu[s0 + s + 1] - cu[s0 + s];
  [[maybe_unused]] const uint8_t* ok = nullptr;
  float count = (float)len;
  if constexpr (KM) {
    ok = key_ok + (size_t)cu[s0 + s];
    float mine = 0.f;
    for (int p = tid; p < len; p += 256) mine += ok[p] ? 1.f : 0.f;
    count = block_sum_256(mine, red);  // (whole numbers below 2^24: exact)
  }
  if (KM ? !(count > 0.f) : len <= 0) {
    if (tid < nl) rank_out[(size_t)(s0 + s) * nl + tid] = 0.f;
    return;
  }
  for (int k = tid; k < H; k += 256) {
    float v;
    if (mean_pool) {
      const float* base = y + (size_t)roff[s] * H + k;
      float acc = 0.f;
      if constexpr (KM) {
        for (int p = 0; p < len; ++p) acc += ok[p] ? base[(size_t)p * H] : 0.0f;
        v = acc / count;
      } else {
        for (int p = 0; p < len; ++p) acc += base[(size_t)p * H];
        v = acc / (float)len;
      }
    } else {
      v = cls[(size_t)s * H + k];
    }
    pooled[k] = v;
  }
  __syncthreads();
  float lsum = 0.f;
  for (int n = tid; n < H; n += 256) {
    float acc = 0.f;
    for (int k = 0; k < H; ++k) acc = fmaf(pooled[k], dense_t[(size_t)k * H + n], acc);
    const float gl = gelu_erf(acc);
    z[n] = gl;
    lsum += gl;
  }
  const float mean = block_sum_256(lsum, red) / (float)H;
  float lq = 0.f;
  for (int n = tid; n < H; n += 256) {
    const float d = z[n] - mean;
    lq += d * d;
  }
  const float var = block_sum_256(lq, red) / (float)H;
  const float rstd = 1.0f / sqrtf(var + eps);
  for (int c = 0; c < nl; ++c) {
    float part = 0.f;
    for (int n = tid; n < H; n += 256) part += (z[n] - mean) * rstd * head_norm[n] * cls_w[(size_t)c * H + n];
    const float tot = block_sum_256(part, red);
    if (tid == 0) rank_out[(size_t)(s0 + s) * nl + c] = poisoned ? __builtin_nanf("") : tot + cls_b[c];
  }
}

__global__ __launch_bounds__(256) void rank_head_kernel(const float* __restrict__ cls, const float* __restrict__ y,
                                                        const int32_t* __restrict__ cu, int s0,
                                                        const int32_t* __restrict__ roff, int mean_pool, int H, int nl,
                                                        const float* __restrict__ dense_t,
                                                        const float* __restrict__ head_norm, float eps,
                                                        const float* __restrict__ cls_w, const float* __restrict__ cls_b,
                                                        float* __restrict__ rank_out, const int* __restrict__ range_flag) {
  rank_head_body<false>(cls, y, cu, s0, roff, nullptr, mean_pool, H, nl, dense_t, head_norm, eps, cls_w, cls_b, rank_out, range_flag);
}

__global__ __launch_bounds__(256) void rank_head_masked_kernel(const float* __restrict__ cls, const float* __restrict__ y,
                                                               const int32_t* __restrict__ cu, int s0,
                                                               const int32_t* __restrict__ roff, const uint8_t* __restrict__ key_ok,
                                                               int mean_pool, int H, int nl, const float* __restrict__ dense_t,
                                                               const float* __restrict__ head_norm, float eps,
                                                               const float* __restrict__ cls_w, const float* __restrict__ cls_b,
                                                               float* __restrict__ rank_out, const int* __restrict__ range_flag) {
  rank_head_body<true>(cls, y, cu, s0, roff, key_ok, mean_pool, H, nl, dense_t, head_norm, eps, cls_w, cls_b, rank_out, range_flag);
}

// Numerics of a narrower precision policy on a wider kernel instantiation: clear the lo plane of a fragment-packed
// tensor (every odd unit of `unit` elements) so that the wider kernel's extra product term adds exact zeros.
__global__ __launch_bounds__(256) void zero_odd_units_kernel(u16* __restrict__ base, int unit, size_t n_pairs) {
  const size_t per_unit = (size_t)unit / 8;  // 16-byte stores
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_pairs * per_unit) return;
  const size_t pair = i / per_unit, off = i % per_unit;
  reinterpret_cast<uint4*>(base + (2 * pair + 1) * unit)[off] = make_uint4(0u, 0u, 0u, 0u);
}

}  // namespace opk
