// opk_f32.hip.h -- kernel set "fp32": one layer with every contraction on the fp32-input MFMA (v_mfma_f32_16x16x4_f32: one
// fp32 VGPR per operand, fp32 accumulate, bit-for-bit a k-ordered fmaf chain; 1/16 of the 16-bit MFMA rate).  Every
// activation plane is row-major fp32 [rows][features] in the packed row layout of opk_common.hip.h, the weights are the
// checkpoint's fp32 tensors as loaded ([out features][in features]).  The residual stream, the RoPE tables, the embedding
// kernel and the pruning head of the other sets are fp32 already and are shared; the ranking head is this set's own
// (rank_head_f32_kernel: exact erff).
//
// Composition invariance: a row's result depends on that row (GEMMs, LayerNorm) or on its own sequence (attention) only --
// no K split across blocks, no atomics, the same k order for every row of a tile.
//
// The parameter structs are visible to every unit (op_internal.h); the kernels only where OPK_F32_KERNELS is defined
// (op_launch_f32.hip).
#pragma once

#include "opk_common.hip.h"

namespace opk {

enum F32Epilogue {
  F32_EPI_QKV = 0,       // RoPE + (q * head_dim^-0.5) -> q, k; v as it is -- one head of q, k or v per wave
  F32_EPI_RESIDUAL = 1,  // x += C
  F32_EPI_GEGLU = 2      // gelu_erf(input) * gate -> h, exact erff; Wi rows in the checkpoint's [input ; gate] order
};

struct F32GemmParams {
  const float* a;  // [r_pad][K]
  const float* w;  // [N][K]
  int K;           // reduction length (multiple of 32)
  int n_tiles;     // QKV: 3 H / 128   RESIDUAL: H / 128   GEGLU: I / 64 (64 input + the 64 matching gate features per tile)
  int m_tiles;     // r_pad / 128
  float* x;        // RESIDUAL: [r_pad][ld_out], updated in place
  float* o0;       // QKV: q   GEGLU: h
  float* o1;       // QKV: k
  float* o2;       // QKV: v
  int ld_out;      // row stride of the output: H (QKV, RESIDUAL), I (GEGLU)
  int hidden;      // H (QKV: the q | k | v column blocks)
  int inter;       // I (GEGLU: row I + f of Wi is the gate of row f)
  const int32_t* row_pos;
  const float* rope_cos;  // [max_pos][32]
  const float* rope_sin;
  int max_pos;
};

struct F32AttnParams {
  const float* q;  // [r_pad][H], scaled by head_dim^-0.5
  const float* k;
  const float* v;
  float* o;
  const int32_t* cu;
  int s0;
  const int32_t* roff;
  int H;
  int window;  // < 0: full attention; else keys with |q - k| <= window
};

#if defined(OPK_F32_KERNELS) || defined(OPK_F32_MASKED_KERNELS)  // (what opk_f32_masked.hip.h shares with the kernels below)

constexpr int F32_LDS = 36;      // LDS row stride of a 32-float K slab (32 + 4 pad: 16-byte aligned rows, spread over the banks)
constexpr int F32_ACC_SLABS = 4; // K slabs (of 32) summed in one fmaf chain before the chain is added to the running total
constexpr int F32_ATT_LDS = 68;  // LDS row stride of a 64-float K / V row (4 rows apart = 16 banks apart: the P V operand reads)

// D = X * Y + C on one wave, fp32 operands.  X: row (lane & 15), k = (lane >> 4).  Y: column (lane & 15), the same k.
// D: column (lane & 15), rows 4 * (lane >> 4) + r -- the C / D map of mfma16.
__device__ __forceinline__ f32x4 mfma_f32(float x, float y, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(x, y, c, 0, 0, 0); }

__device__ __forceinline__ float gelu_erf_exact(float x) { return 0.5f * x * (1.0f + erff(x * 0.70710678118654752440f)); }

// the sum of a 256-thread block (the ranking heads)
__device__ __forceinline__ float block_sum_f32(float v, float* red) {
  v = wave_sum(v);
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  __syncthreads();
  if (lane == 0) red[wave] = v;
  __syncthreads();
  return (red[0] + red[1]) + (red[2] + red[3]);
}

#endif

#ifdef OPK_F32_KERNELS

// ----------------------------------------------------------------------------------------------
// y = (x - mean) / sqrt(var + eps) * w into an fp32 plane: one wave per row (the arithmetic of ln_kernel, opk_layernorm.hip.h)
// ----------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void ln_f32_kernel(const float* __restrict__ x, const float* __restrict__ lnw, float eps, int H,
                                                     int r_pad, float* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= r_pad) return;
  const int nchunk = H >> 2;  // H <= 1024: at most 4 float4 per lane
  const float4* src = reinterpret_cast<const float4*>(x + (size_t)row * H);
  float4 v[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int c = lane + 64 * k;
    v[k] = (c < nchunk) ? src[c] : make_float4(0.f, 0.f, 0.f, 0.f);
  }
  float s = 0.f;
#pragma unroll
  for (int k = 0; k < 4; ++k) s += (v[k].x + v[k].y) + (v[k].z + v[k].w);
  const float mean = wave_sum(s) / (float)H;
  float q = 0.f;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    if (lane + 64 * k < nchunk) {
      const float a = v[k].x - mean, b = v[k].y - mean, c = v[k].z - mean, d = v[k].w - mean;
      q += (a * a + b * b) + (c * c + d * d);
    }
  }
  const float var = wave_sum(q) / (float)H;
  const float rstd = 1.0f / sqrtf(var + eps);
  float4* dst = reinterpret_cast<float4*>(out + (size_t)row * H);
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int c = lane + 64 * k;
    if (c < nchunk) {
      const float4 ww = reinterpret_cast<const float4*>(lnw)[c];
      dst[c] = make_float4((v[k].x - mean) * rstd * ww.x, (v[k].y - mean) * rstd * ww.y, (v[k].z - mean) * rstd * ww.z,
                           (v[k].w - mean) * rstd * ww.w);
    }
  }
}

// ----------------------------------------------------------------------------------------------
// GEMM  C[m, n] = sum_k A[m, k] * W[n, k], fp32 operands.  128 x 128 tile over LDS-staged K slabs of 32, 4 waves (2 x 2),
// each wave 64 x 64 = 4 x 4 accumulators of 16 x 16, in the swapped orientation of gemm_kernel (X = W rows, Y = A rows):
// every lane ends with 4 consecutive output features of one token.  A lane reads 4 consecutive k of a row at once
// (16 bytes); MFMA step e of such a read multiplies k = 16 s + 4 g + e on both operands, so the chain runs over a fixed
// permutation of k, the same for every row.  After F32_ACC_SLABS slabs the chain is added to a running total and starts
// again from zero: the rounding error of a sum grows with the length of its chain.
// ----------------------------------------------------------------------------------------------
template <int EPI>
__global__ __launch_bounds__(256, 2) void gemm_f32_kernel(F32GemmParams p) {
  __shared__ __attribute__((aligned(16))) float sA[GEMM_BM * F32_LDS];
  __shared__ __attribute__((aligned(16))) float sW[GEMM_BN * F32_LDS];

  // XCD-aware tile order (gemm_kernel): the feature tiles of one row tile follow each other on one XCD
  const int nwg = gridDim.x;
  const int orig = blockIdx.x;
  const int xcd = orig & 7;
  const int qd = nwg >> 3, rem = nwg & 7;
  const int wgid = (xcd < rem ? xcd * (qd + 1) : rem * (qd + 1) + (xcd - rem) * qd) + (orig >> 3);
  const int n_tile = wgid % p.n_tiles;
  const int m_tile = wgid / p.n_tiles;
  const int m0 = m_tile * GEMM_BM;
  const int n0 = n_tile * GEMM_BN;

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int wm = wave & 1;   // token half of the tile
  const int wn = wave >> 1;  // feature half of the tile
  const int l15 = lane & 15;
  const int g = lane >> 4;
  const int K = p.K;

  // staging: a slab is 128 rows x 32 floats = 1024 pieces of 16 B per operand; a thread moves pieces (srow + 32 u, skc)
  const int srow = tid >> 3;
  const int skc = (tid & 7) * 4;
  const int soff = srow * F32_LDS + skc;
  const float* ga0 = p.a + (size_t)(m0 + srow) * K + skc;
  // W row of tile row lr.  GeGLU: per 64-feature wave half, 32 input rows, then their 32 gate rows (row I + f of Wi)
  auto w_row = [&](int lr) {
    if (EPI != F32_EPI_GEGLU) return n0 + lr;
    const int f = n_tile * 64 + (lr >> 6) * 32 + (lr & 31);
    return (lr & 32) ? p.inter + f : f;
  };
  const float* gw0 = p.w + (size_t)w_row(srow) * K + skc;
  const float* gw1 = p.w + (size_t)w_row(srow + 32) * K + skc;
  const float* gw2 = p.w + (size_t)w_row(srow + 64) * K + skc;
  const float* gw3 = p.w + (size_t)w_row(srow + 96) * K + skc;
  // staging registers are plain scalars and the moves are macros (arrays captured by lambdas end up in scratch memory)
  float4 ra0, ra1, ra2, ra3, rw0, rw1, rw2, rw3;
#define OPK_F32_GLOAD(kt_)                                          \
  do {                                                              \
    const int ko_ = (kt_) * GEMM_BK;                                \
    ra0 = *reinterpret_cast<const float4*>(ga0 + ko_);              \
    ra1 = *reinterpret_cast<const float4*>(ga0 + 32 * (size_t)K + ko_); \
    ra2 = *reinterpret_cast<const float4*>(ga0 + 64 * (size_t)K + ko_); \
    ra3 = *reinterpret_cast<const float4*>(ga0 + 96 * (size_t)K + ko_); \
    rw0 = *reinterpret_cast<const float4*>(gw0 + ko_);              \
    rw1 = *reinterpret_cast<const float4*>(gw1 + ko_);              \
    rw2 = *reinterpret_cast<const float4*>(gw2 + ko_);              \
    rw3 = *reinterpret_cast<const float4*>(gw3 + ko_);              \
  } while (0)
#define OPK_F32_LSTORE()                                            \
  do {                                                              \
    *reinterpret_cast<float4*>(&sA[soff]) = ra0;                    \
    *reinterpret_cast<float4*>(&sA[soff + 32 * F32_LDS]) = ra1;     \
    *reinterpret_cast<float4*>(&sA[soff + 64 * F32_LDS]) = ra2;     \
    *reinterpret_cast<float4*>(&sA[soff + 96 * F32_LDS]) = ra3;     \
    *reinterpret_cast<float4*>(&sW[soff]) = rw0;                    \
    *reinterpret_cast<float4*>(&sW[soff + 32 * F32_LDS]) = rw1;     \
    *reinterpret_cast<float4*>(&sW[soff + 64 * F32_LDS]) = rw2;     \
    *reinterpret_cast<float4*>(&sW[soff + 96 * F32_LDS]) = rw3;     \
  } while (0)

  f32x4 acc[4][4], tot[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = tot[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  const int nk = K / GEMM_BK;
  OPK_F32_GLOAD(0);
  OPK_F32_LSTORE();
  __syncthreads();

  const int a_frag = (wm * 64 + l15) * F32_LDS + g * 4;
  const int w_frag = (wn * 64 + l15) * F32_LDS + g * 4;

  for (int kt = 0; kt < nk; ++kt) {
    if (kt + 1 < nk) OPK_F32_GLOAD(kt + 1);
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      f32x4 wf[4], af[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        wf[i] = *reinterpret_cast<const f32x4*>(&sW[w_frag + i * 16 * F32_LDS + s * 16]);
        af[i] = *reinterpret_cast<const f32x4*>(&sA[a_frag + i * 16 * F32_LDS + s * 16]);
      }
#pragma unroll
      for (int e = 0; e < 4; ++e)
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
          for (int j = 0; j < 4; ++j) acc[i][j] = mfma_f32(wf[i][e], af[j][e], acc[i][j]);
    }
    __syncthreads();
    if (kt + 1 < nk) {
      OPK_F32_LSTORE();
      __syncthreads();
    }
    if ((kt % F32_ACC_SLABS) == F32_ACC_SLABS - 1 && kt + 1 < nk) {
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          tot[i][j] += acc[i][j];
          acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
        }
    }
  }
#undef OPK_F32_GLOAD
#undef OPK_F32_LSTORE
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] += tot[i][j];

  // acc[i][j][r]: feature n0 + wn*64 + 16i + 4g + r (of the tile's row order), token m0 + wm*64 + 16j + l15
  if (EPI == F32_EPI_RESIDUAL) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int m = m0 + wm * 64 + j * 16 + l15;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int f = n0 + wn * 64 + i * 16 + g * 4;
        float4* px = reinterpret_cast<float4*>(p.x + (size_t)m * p.ld_out + f);
        float4 r4 = *px;
        r4.x += acc[i][j][0];
        r4.y += acc[i][j][1];
        r4.z += acc[i][j][2];
        r4.w += acc[i][j][3];
        *px = r4;
      }
    }
    return;
  }

  if (EPI == F32_EPI_GEGLU) {
    // i = 0, 1: 32 input features, i = 2, 3: their gates
    const int out_col0 = n_tile * 64 + wn * 32;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int m = m0 + wm * 64 + j * 16 + l15;
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        float4 v;
        v.x = gelu_erf_exact(acc[i][j][0]) * acc[i + 2][j][0];
        v.y = gelu_erf_exact(acc[i][j][1]) * acc[i + 2][j][1];
        v.z = gelu_erf_exact(acc[i][j][2]) * acc[i + 2][j][2];
        v.w = gelu_erf_exact(acc[i][j][3]) * acc[i + 2][j][3];
        *reinterpret_cast<float4*>(p.o0 + (size_t)m * p.ld_out + out_col0 + i * 16 + g * 4) = v;
      }
    }
    return;
  }

  if (EPI == F32_EPI_QKV) {
    // this wave's 64 features are exactly one head of q, of k or of v
    const int col = n0 + wn * 64;
    const int which = col / p.hidden;
    const int out_col = col - which * p.hidden;
    if (which == 2) {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int m = m0 + wm * 64 + j * 16 + l15;
#pragma unroll
        for (int i = 0; i < 4; ++i)
          *reinterpret_cast<float4*>(p.o2 + (size_t)m * p.ld_out + out_col + i * 16 + g * 4) =
              make_float4(acc[i][j][0], acc[i][j][1], acc[i][j][2], acc[i][j][3]);
      }
      return;
    }
    float* out = which == 0 ? p.o0 : p.o1;
    const float qscale = which == 0 ? 0.125f : 1.0f;  // head_dim^-0.5, an exact power of two
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int m = m0 + wm * 64 + j * 16 + l15;
      int pos = p.row_pos[m];
      pos = pos < 0 ? 0 : (pos >= p.max_pos ? p.max_pos - 1 : pos);
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        // d = 16i + 4g + r pairs with d + 32 (rotate_half)
        const float4 c4 = *reinterpret_cast<const float4*>(p.rope_cos + (size_t)pos * ROPE_HALF + i * 16 + g * 4);
        const float4 s4 = *reinterpret_cast<const float4*>(p.rope_sin + (size_t)pos * ROPE_HALF + i * 16 + g * 4);
        const float cs[4] = {c4.x, c4.y, c4.z, c4.w};
        const float sn[4] = {s4.x, s4.y, s4.z, s4.w};
        float lo_half[4], hi_half[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float x1 = acc[i][j][r], x2 = acc[i + 2][j][r];
          lo_half[r] = rope_lo(x1, x2, cs[r], sn[r]) * qscale;
          hi_half[r] = rope_hi(x1, x2, cs[r], sn[r]) * qscale;
        }
        float* dst = out + (size_t)m * p.ld_out + out_col + i * 16 + g * 4;
        *reinterpret_cast<float4*>(dst) = make_float4(lo_half[0], lo_half[1], lo_half[2], lo_half[3]);
        *reinterpret_cast<float4*>(dst + 32) = make_float4(hi_half[0], hi_half[1], hi_half[2], hi_half[3]);
      }
    }
    return;
  }
}

// ----------------------------------------------------------------------------------------------
// Attention over the packed layout, fp32.  One block = 64 queries of one (sequence, head), 16 per wave, on 64-key tiles
// (the block map and the online softmax of attn_kernel, opk_tiled.hip.h).  S^T = K Q^T leaves a lane with one query
// column and the keys 16 m + 4 g + r of the tile; O^T = V^T P^T takes those p as its Y operand where they are, with V
// read from LDS by (key, d).  Keys at or beyond the sequence's length are staged as zeros: nothing outside the rows the
// projections wrote is read.  expf, not the fast exponential.
// ----------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256, 2) void attn_f32_kernel(F32AttnParams p) {
  __shared__ __attribute__((aligned(16))) float sK[ATT_BK * F32_ATT_LDS];
  __shared__ __attribute__((aligned(16))) float sV[ATT_BK * F32_ATT_LDS];

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

  // staging: a tile is 64 keys x 64 floats = 1024 pieces of 16 B per operand; a thread moves pieces (prow + 16 u, pcol)
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
    // initial -1e30): expf(masked - max) is exactly 0 even when a whole tile is masked for this query.
    float tile_max = -3e30f;
#pragma unroll
    for (int m = 0; m < 4; ++m) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int key = kbase + 16 * m + 4 * g + r;
        const int d = key - qpos;
        const bool ok = (key < len) & (d <= win) & (d >= -win);
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
    // oacc[n][r]: d = 16n + 4g + r of query qpos
#pragma unroll
    for (int n = 0; n < 4; ++n)
      *reinterpret_cast<float4*>(p.o + qrow * H + hcol + n * 16 + g * 4) =
          make_float4(oacc[n][0] * inv, oacc[n][1] * inv, oacc[n][2] * inv, oacc[n][3] * inv);
  }
}

// ----------------------------------------------------------------------------------------------
// ModernBertPredictionHead + classifier on the pooled row: rank_head_kernel (opk_small.hip.h) with the exact erff GELU -- that
// kernel's polynomial is 2.6e-5 (relative) off at small arguments, which the LayerNorm behind it turns into 1e-5 on a
// logit when the dense layer's outputs are small (mean pooling, reference-initialised head) -- and with the sums over
// tokens and over k taken in chunks of 16 / 128.  One block per sequence; dense weight transposed [k][n].
// ----------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void rank_head_f32_kernel(const float* __restrict__ cls, const float* __restrict__ y,
                                                            const int32_t* __restrict__ cu, int s0, const int32_t* __restrict__ roff,
                                                            int mean_pool, int H, int nl, const float* __restrict__ dense_t,
                                                            const float* __restrict__ head_norm, float eps,
                                                            const float* __restrict__ cls_w, const float* __restrict__ cls_b,
                                                            float* __restrict__ rank_out) {
  __shared__ float pooled[1024];
  __shared__ float z[1024];
  __shared__ float red[4];
  const int s = blockIdx.x;
  const int tid = threadIdx.x;
  const int len = cu[s0 + s + 1] - cu[s0 + s];
  if (len <= 0) {
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
        for (int p = p0; p < p1; ++p) part += base[(size_t)p * H];
        acc += part;
      }
      v = acc / (float)len;
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

#endif  // OPK_F32_KERNELS

}  // namespace opk
