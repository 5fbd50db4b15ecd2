// opk_rowvec.hip.h -- one wave per row: load, LayerNorm and store of a residual-stream row held in registers.  Device helpers
// only, no kernel: opk_small / opk_layernorm / opk_pool .hip.h build their kernels on them.
#pragma once

#include "opk_common.hip.h"

namespace opk {

// ----------------------------------------------------------------------------------------------
// LayerNorm family: one wave per row, float4 per lane-chunk, H <= 1024, H % 4 == 0
// ----------------------------------------------------------------------------------------------
constexpr int LN_MAX_CHUNKS = 4;  // float4 chunks per lane: H <= 4 * 64 * 4 = 1024

struct RowVec {
  float4 v[LN_MAX_CHUNKS];
};

__device__ __forceinline__ void row_load(const float* __restrict__ src, int H, int lane, RowVec& rv) {
  const int nchunk = H >> 2;
#pragma unroll
  for (int k = 0; k < LN_MAX_CHUNKS; ++k) {
    const int c = lane + 64 * k;
    rv.v[k] = (c < nchunk) ? reinterpret_cast<const float4*>(src)[c] : make_float4(0.f, 0.f, 0.f, 0.f);
  }
}

// y = (x - mean) / sqrt(var + eps) * w   (biased variance, as torch.nn.LayerNorm)
__device__ __forceinline__ void row_layer_norm(RowVec& rv, const float* __restrict__ w, int H, int lane, float eps) {
  const int nchunk = H >> 2;
  float s = 0.f;
#pragma unroll
  for (int k = 0; k < LN_MAX_CHUNKS; ++k) s += (rv.v[k].x + rv.v[k].y) + (rv.v[k].z + rv.v[k].w);
  const float mean = wave_sum(s) / (float)H;
  float q = 0.f;
#pragma unroll
  for (int k = 0; k < LN_MAX_CHUNKS; ++k) {
    const int c = lane + 64 * k;
    if (c < nchunk) {
      const float a = rv.v[k].x - mean, b = rv.v[k].y - mean, cc = rv.v[k].z - mean, d = rv.v[k].w - mean;
      q += (a * a + b * b) + (cc * cc + d * d);
    }
  }
  const float var = wave_sum(q) / (float)H;
  const float rstd = 1.0f / sqrtf(var + eps);
#pragma unroll
  for (int k = 0; k < LN_MAX_CHUNKS; ++k) {
    const int c = lane + 64 * k;
    if (c < nchunk) {
      const float4 ww = reinterpret_cast<const float4*>(w)[c];
      rv.v[k].x = (rv.v[k].x - mean) * rstd * ww.x;
      rv.v[k].y = (rv.v[k].y - mean) * rstd * ww.y;
      rv.v[k].z = (rv.v[k].z - mean) * rstd * ww.z;
      rv.v[k].w = (rv.v[k].w - mean) * rstd * ww.w;
    }
  }
}

template <bool SPLIT>
__device__ __forceinline__ void row_store_planes(const RowVec& rv, u16* __restrict__ hi, u16* __restrict__ lo, int H,
                                                 int lane) {
  const int nchunk = H >> 2;
#pragma unroll
  for (int k = 0; k < LN_MAX_CHUNKS; ++k) {
    const int c = lane + 64 * k;
    if (c < nchunk) {
      const float v[4] = {rv.v[k].x, rv.v[k].y, rv.v[k].z, rv.v[k].w};
      uint2 h2, l2;
      split4<SPLIT>(v, h2, l2);
      reinterpret_cast<uint2*>(hi)[c] = h2;
      if (SPLIT) reinterpret_cast<uint2*>(lo)[c] = l2;
    }
  }
}

__device__ __forceinline__ void row_store_f32(const RowVec& rv, float* __restrict__ dst, int H, int lane) {
  const int nchunk = H >> 2;
#pragma unroll
  for (int k = 0; k < LN_MAX_CHUNKS; ++k) {
    const int c = lane + 64 * k;
    if (c < nchunk) reinterpret_cast<float4*>(dst)[c] = rv.v[k];
  }
}

}  // namespace opk
