// opk_f32_masked.hip.h -- op_forward_masked: the kernels a forward under an arbitrary [B, L] attention mask adds to kernel set
// "fp32" (opk_f32.hip.h).  Such a forward is DENSE: every one of the B x L positions is a row at position = its column, a
// sequence is a whole padded row, and the mask removes KEYS only (key_ok, one byte per position, indexed like the ids).  A
// query that is left without a key -- a masked position of a sliding-window layer whose whole window is masked -- gets what an
// eager softmax over masked_fill(finfo.min) gives it: uniform weights over all L columns, i.e. the plain mean of v over the
// row (vmean_f32_kernel).  LayerNorm, the three GEMM epilogues and the RoPE lookup are the set's own.
//
// With a prefix mask every valid position's result has the bits of the set's packed forward: the same block map, tile order
// and online softmax, a masked key's p is exactly 0 and a wholly masked tile leaves the accumulators as they are.
//
// The parameter struct is visible to every unit (op_internal.h); the kernels only where OPK_F32_MASKED_KERNELS is defined
// (op_launch_f32_masked.hip).
#pragma once

#include "opk_f32.hip.h"

namespace opk {

struct F32MaskedAttnParams {
  F32AttnParams a;
  const uint8_t* key_ok;  // [total_tokens]: key `k` of sequence s0 + s is cu[s0 + s] + k
  const float* vmean;     // [chunk sequences][H] of vmean_f32_kernel, or nullptr: a query without a key gets zeros
};

// the device status word of op_forward_masked's id check: the linear index of the first id outside the table
constexpr uint32_t MASKED_ST_NONE = 0xffffffffu;

#ifdef OPK_F32_MASKED_KERNELS

// ----------------------------------------------------------------------------------------------
// cu[r] = r * width (every row is a sequence of `width` positions) and the id check: EVERY position is embedded, so every id
// is held to the table, under a zero of the mask too.  The first offender in row-major order wins (atomicMin on the linear
// index, which the caller keeps below 2^31).
// ----------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void masked_prepare_kernel(const int32_t* __restrict__ ids, int n_rows, int width, int vocab,
                                                             int32_t* __restrict__ cu, uint32_t* __restrict__ status) {
  const size_t n = (size_t)n_rows * (size_t)width;
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i <= (size_t)n_rows) cu[i] = (int32_t)(i * (size_t)width);
  if (i < n && (uint32_t)ids[i] >= (uint32_t)vocab) atomicMin(status, (uint32_t)i);  // (a negative id wraps to a huge value)
}

// ----------------------------------------------------------------------------------------------
// vmean[s][f] = mean over the sequence's positions of v[.][f]: partial sums of 16 positions added in order, as
// rank_head_f32_kernel sums tokens.  grid = (sequences, ceil(H / 256)).
// ----------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void vmean_f32_kernel(const float* __restrict__ v, const int32_t* __restrict__ cu, int s0,
                                                        const int32_t* __restrict__ roff, int H, float* __restrict__ vmean) {
  const int s = blockIdx.x;
  const int f = blockIdx.y * 256 + threadIdx.x;
  if (f >= H) return;
  const int len = cu[s0 + s + 1] - cu[s0 + s];
  float acc = 0.f;
  if (len > 0) {
    const float* base = v + (size_t)roff[s] * H + f;
    for (int p0 = 0; p0 < len; p0 += 16) {
      const int p1 = p0 + 16 < len ? p0 + 16 : len;
      float part = 0.f;
      for (int p = p0; p < p1; ++p) part += base[(size_t)p * H];
      acc += part;
    }
    acc /= (float)len;
  }
  vmean[(size_t)s * H + f] = acc;
}

// ----------------------------------------------------------------------------------------------
// attn_f32_kernel (opk_f32.hip.h) with the key_ok bytes of the tile staged beside K and V and taken into the `ok` predicate,
// and the epilogue of a query without a key.  Positions equal indices in dense rows: the tiles of a sliding-window layer are
// still bounded by the index window.
// ----------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256, 2) void attn_f32_masked_kernel(F32MaskedAttnParams mp) {
  __shared__ __attribute__((aligned(16))) float sK[ATT_BK * F32_ATT_LDS];
  __shared__ __attribute__((aligned(16))) float sV[ATT_BK * F32_ATT_LDS];
  __shared__ __attribute__((aligned(16))) uint8_t sOk[ATT_BK];

  const F32AttnParams& p = mp.a;
  const int s = blockIdx.z;
  const int head = blockIdx.y;
  const int q0 = blockIdx.x * ATT_BQ;
  const int seq_start = p.cu[p.s0 + s];
  const int len = p.cu[p.s0 + s + 1] - seq_start;
  if (q0 >= len) return;
  const int r0 = p.roff[s];
  const int alloc = p.roff[s + 1] - r0;

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int l15 = lane & 15;
  const int g = lane >> 4;
  const int H = p.H;
  const int hcol = head * HEAD_DIM;

  const int qbase = q0 + wave * 16;
  const bool active = qbase < alloc;  // alloc is a multiple of 16: whole wave in or out
  const int qpos = qbase + l15;
  const size_t qrow = (size_t)(r0 + (active ? qpos : q0));

  f32x4 qf[4];  // d = 16 t + 4 g + e
#pragma unroll
  for (int t = 0; t < 4; ++t) qf[t] = *reinterpret_cast<const f32x4*>(p.q + qrow * H + hcol + t * 16 + g * 4);

  int kt_lo = 0, kt_hi = (len - 1) / ATT_BK;
  if (p.window >= 0) {
    const int lo_key = q0 - p.window;
    kt_lo = lo_key > 0 ? lo_key / ATT_BK : 0;
    const int hi_t = (q0 + ATT_BQ - 1 + p.window) / ATT_BK;
    kt_hi = hi_t < kt_hi ? hi_t : kt_hi;
  }

  float m_run = -1e30f;
  float l_run = 0.f;
  f32x4 oacc[4];
#pragma unroll
  for (int n = 0; n < 4; ++n) oacc[n] = f32x4{0.f, 0.f, 0.f, 0.f};

  const int prow = tid >> 4;
  const int pcol = (tid & 15) * 4;
  const int win = p.window >= 0 ? p.window : (1 << 30);

  for (int kt = kt_lo; kt <= kt_hi; ++kt) {
    const int kbase = kt * ATT_BK;
    __syncthreads();  // previous tile fully consumed
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int row = prow + 16 * u;
      float4 kv = make_float4(0.f, 0.f, 0.f, 0.f), vv = kv;
      if (kbase + row < len) {
        const size_t grow = (size_t)(r0 + kbase + row) * H + hcol + pcol;
        kv = *reinterpret_cast<const float4*>(p.k + grow);
        vv = *reinterpret_cast<const float4*>(p.v + grow);
      }
      *reinterpret_cast<float4*>(&sK[row * F32_ATT_LDS + pcol]) = kv;
      *reinterpret_cast<float4*>(&sV[row * F32_ATT_LDS + pcol]) = vv;
    }
    if (tid < ATT_BK) sOk[tid] = kbase + tid < len ? mp.key_ok[(size_t)seq_start + kbase + tid] : (uint8_t)0;
    __syncthreads();

    // S^T tile: rows = keys (4 fragments of 16), column = this lane's query
    f32x4 sacc[4];
#pragma unroll
    for (int m = 0; m < 4; ++m) sacc[m] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      f32x4 kf[4];
#pragma unroll
      for (int m = 0; m < 4; ++m) kf[m] = *reinterpret_cast<const f32x4*>(&sK[(m * 16 + l15) * F32_ATT_LDS + t * 16 + g * 4]);
#pragma unroll
      for (int e = 0; e < 4; ++e)
#pragma unroll
        for (int m = 0; m < 4; ++m) sacc[m] = mfma_f32(kf[m][e], qf[t][e], sacc[m]);
    }

    // element (m, r) of this lane: key = kbase + 16 m + 4 g + r.  Masked scores become -3e30 (below the running maximum's
    // initial -1e30): expf(masked - max) is exactly 0 even when a whole tile is masked for this query, and then alpha = 1.
    float tile_max = -3e30f;
#pragma unroll
    for (int m = 0; m < 4; ++m) {
      const uint32_t ok4 = *reinterpret_cast<const uint32_t*>(&sOk[16 * m + 4 * g]);  // (keys at or beyond len: 0)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int key = kbase + 16 * m + 4 * g + r;
        const int d = key - qpos;
        const bool ok = (((ok4 >> (8 * r)) & 0xffu) != 0u) & (d <= win) & (d >= -win);
        sacc[m][r] = ok ? sacc[m][r] : -3e30f;
        tile_max = fmaxf(tile_max, sacc[m][r]);
      }
    }
    tile_max = fmaxf(tile_max, __shfl_xor(tile_max, 16, 64));
    tile_max = fmaxf(tile_max, __shfl_xor(tile_max, 32, 64));
    const float m_new = fmaxf(m_run, tile_max);
    const float alpha = expf(m_run - m_new);
    m_run = m_new;
    float psum = 0.f;
#pragma unroll
    for (int m = 0; m < 4; ++m) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float e = expf(sacc[m][r] - m_new);
        sacc[m][r] = e;
        psum += e;
      }
    }
    l_run = l_run * alpha + psum;
#pragma unroll
    for (int n = 0; n < 4; ++n) {
      oacc[n][0] *= alpha;
      oacc[n][1] *= alpha;
      oacc[n][2] *= alpha;
      oacc[n][3] *= alpha;
    }

    // O^T += V^T P^T: step (m, r) sums the keys 16 m + 4 g + r, the p this lane holds
#pragma unroll
    for (int m = 0; m < 4; ++m) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float* vrow = &sV[(m * 16 + g * 4 + r) * F32_ATT_LDS + l15];
#pragma unroll
        for (int n = 0; n < 4; ++n) oacc[n] = mfma_f32(vrow[n * 16], sacc[m][r], oacc[n]);
      }
    }
  }

  float l_tot = l_run + __shfl_xor(l_run, 16, 64);
  l_tot += __shfl_xor(l_tot, 32, 64);
  const float inv = l_tot > 0.f ? 1.0f / l_tot : 0.f;
  if (active) {
    // oacc[n][r]: d = 16n + 4g + r of query qpos.  No key at all (l_tot == 0, every p was exactly 0): the row's mean of v
    const bool fallback = !(l_tot > 0.f) && mp.vmean != nullptr;
#pragma unroll
    for (int n = 0; n < 4; ++n) {
      float4 o4 = make_float4(oacc[n][0] * inv, oacc[n][1] * inv, oacc[n][2] * inv, oacc[n][3] * inv);
      if (fallback) o4 = *reinterpret_cast<const float4*>(mp.vmean + (size_t)s * H + hcol + n * 16 + g * 4);
      *reinterpret_cast<float4*>(p.o + qrow * H + hcol + n * 16 + g * 4) = o4;
    }
  }
}

// ----------------------------------------------------------------------------------------------
// rank_head_f32_kernel with mean pooling weighted by key_ok: the same chunks of 16 positions in the same order, a masked
// position contributing +0.0f, the divisor the number of valid positions -- under a prefix mask the bits of that kernel on the
// packed row.  cls pooling reads column 0 whatever its mask says (the reference pools it).  A sequence without a valid position
// gives zeros, as an empty row does.
// ----------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void rank_head_f32_masked_kernel(const float* __restrict__ cls, const float* __restrict__ y,
                                                                   const int32_t* __restrict__ cu, int s0,
                                                                   const int32_t* __restrict__ roff, const uint8_t* __restrict__ key_ok,
                                                                   int mean_pool, int H, int nl, const float* __restrict__ dense_t,
                                                                   const float* __restrict__ head_norm, float eps,
                                                                   const float* __restrict__ cls_w, const float* __restrict__ cls_b,
                                                                   float* __restrict__ rank_out) {
  __shared__ float pooled[1024];
  __shared__ float z[1024];
  __shared__ float red[4];
  const int s = blockIdx.x;
  const int tid = threadIdx.x;
  const int seq_start = cu[s0 + s];
  const int len = cu[s0 + s + 1] - seq_start;
  const uint8_t* ok = key_ok + (size_t)seq_start;
  float mine = 0.f;
  for (int p = tid; p < len; p += 256) mine += ok[p] ? 1.f : 0.f;
  const float count = block_sum_f32(mine, red);  // (whole numbers below 2^24: exact)
  if (!(count > 0.f)) {
    if (tid < nl) rank_out[(size_t)(s0 + s) * nl + tid] = 0.f;
    return;
  }
  for (int k = tid; k < H; k += 256) {
    float v;
    if (mean_pool) {
      const float* base = y + (size_t)roff[s] * H + k;
      float acc = 0.f;
      for (int p0 = 0; p0 < len; p0 += 16) {
        const int p1 = p0 + 16 < len ? p0 + 16 : len;
        float part = 0.f;
        for (int p = p0; p < p1; ++p) part += ok[p] ? base[(size_t)p * H] : 0.0f;
        acc += part;
      }
      v = acc / count;
    } else {
      v = cls[(size_t)s * H + k];
    }
    pooled[k] = v;
  }
  __syncthreads();
  float lsum = 0.f;
  for (int n = tid; n < H; n += 256) {
    float acc = 0.f;
    for (int k0 = 0; k0 < H; k0 += 128) {  // (H is a multiple of 128)
      float part = 0.f;
      for (int k = k0; k < k0 + 128; ++k) part = fmaf(pooled[k], dense_t[(size_t)k * H + n], part);
      acc += part;
    }
    const float gl = gelu_erf_exact(acc);
    z[n] = gl;
    lsum += gl;
  }
  const float mean = block_sum_f32(lsum, red) / (float)H;
  float lq = 0.f;
  for (int n = tid; n < H; n += 256) {
    const float d = z[n] - mean;
    lq += d * d;
  }
  const float var = block_sum_f32(lq, red) / (float)H;
  const float rstd = 1.0f / sqrtf(var + eps);
  for (int c = 0; c < nl; ++c) {
    float part = 0.f;
    for (int n = tid; n < H; n += 256) part += (z[n] - mean) * rstd * head_norm[n] * cls_w[(size_t)c * H + n];
    const float tot = block_sum_f32(part, red);
    if (tid == 0) rank_out[(size_t)(s0 + s) * nl + c] = tot + cls_b[c];
  }
}

// the project's convention for the pruning logits: exact +0.0 at every masked position (final_ln_prune_kernel wrote all of them)
__global__ __launch_bounds__(256) void prune_mask_f32_kernel(float* __restrict__ prune, const uint8_t* __restrict__ key_ok, size_t t0,
                                                             size_t n_tokens) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n_tokens) return;
  if (!key_ok[t0 + i]) {
    prune[(t0 + i) * 2 + 0] = 0.f;
    prune[(t0 + i) * 2 + 1] = 0.f;
  }
}

#endif  // OPK_F32_MASKED_KERNELS

}  // namespace opk
