// opk_probe.hip.h -- test hook (op_debug_primitive): one kernel per primitive that runs the device functions of
// opk_common.hip.h -- the conversions, the GELU polynomial, the exponentials, RoPE, the keep-probability and the scaled
// e4m3 MFMA -- element by element over a caller's buffer and stores what they return as raw bits.  Nothing is restated
// here: a primitive that the forward's kernels call is called, with the wave's conversion mode set the way those kernels
// set it.  tests/test_gpu_primitives.py compares the records with tests/arith_model.py's operand roundings and with
// float64.  Every index is derived from the thread index and checked against the element count; no input value is used
// as an address.
#pragma once

#include "opk_common.hip.h"

namespace opk {

// enum op_probe_kind of include/open_provence_hip.h
enum ProbeKind {
  PROBE_BF16_SPLIT = 0,
  PROBE_F16_PAIR = 1,
  PROBE_F16_F8 = 2,
  PROBE_E4M3_F16 = 3,
  PROBE_E4M3_F32 = 4,
  PROBE_GELU = 5,
  PROBE_EXP2 = 6,
  PROBE_ROPE = 7,
  PROBE_KEEP_PROB = 8,
  PROBE_MFMA_SCALE = 9,
  PROBE_KIND_COUNT = 10
};

template <int MODE>
__device__ __forceinline__ void probe_set_mode() {
  if constexpr (MODE != 0) set_saturating_conversions();
  else set_overflowing_conversions();
}

// the GELU in stages, issued as the GeGLU of the whole-layer kernels issues it (geglu_stage of opk_layer16p_body.inc,
// opk_layer32.hip.h): stage k of every value in flight before stage k + 1 of any
template <int NV>
__device__ __forceinline__ void probe_gelu_staged(const float (&src)[NV], float (&out)[NV]) {
  float gx[NV], gq[NV];
  static_for<7>([&](auto stg_tag) {
    constexpr int stg = decltype(stg_tag)::value;
    static_for<NV>([&](auto i_tag) {
      constexpr int i = decltype(i_tag)::value;
      if constexpr (stg == 0) {
        gx[i] = src[i];
        gq[i] = gelu_erf_poly(0.f, fabsf(gx[i]), 0);
      } else if constexpr (stg < 5) gq[i] = gelu_erf_poly(gq[i], fabsf(gx[i]), stg);
      else if constexpr (stg == 5) gq[i] = __builtin_amdgcn_exp2f(gq[i]);
      else gq[i] = gelu_erf_finish(gq[i], gx[i]);
    });
  });
  static_for<NV>([&](auto i_tag) { out[decltype(i_tag)::value] = gq[decltype(i_tag)::value]; });
}

// Kinds whose record belongs to a group of four inputs (the packed conversions take two or four values at a time).
// in: fp32 (PROBE_E4M3_F16: fp16 bits), n elements, n % 4 == 0; out: WORDS uint32 per element.
template <int KIND, int MODE>
__global__ void probe_convert_kernel(const void* __restrict__ in, size_t n, uint32_t* __restrict__ out) {
  probe_set_mode<MODE>();
  const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n / 4) return;
  const size_t e0 = t * 4;
  if constexpr (KIND == PROBE_E4M3_F16) {
    const u16* src = reinterpret_cast<const u16*>(in) + e0;
    const uint32_t h01 = (uint32_t)src[0] | ((uint32_t)src[1] << 16), h23 = (uint32_t)src[2] | ((uint32_t)src[3] << 16);
    const uint32_t w = f16x4_to_e4m3(h01, h23);
#pragma unroll
    for (int j = 0; j < 4; ++j) out[e0 + j] = (w >> (8 * j)) & 0xffu;
  } else {
    const float* src = reinterpret_cast<const float*>(in) + e0;
    const float v[4] = {src[0], src[1], src[2], src[3]};
    if constexpr (KIND == PROBE_BF16_SPLIT) {  // 7 words: split2 hi, lo | split2_pk hi, lo | split4 hi, lo | f2bf
      uint32_t h2[2], l2[2], hp[2], lp[2];
      split2<true>(v[0], v[1], h2[0], l2[0]);
      split2<true>(v[2], v[3], h2[1], l2[1]);
      split2_pk<true>(f32x2{v[0], v[1]}, hp[0], lp[0]);
      split2_pk<true>(f32x2{v[2], v[3]}, hp[1], lp[1]);
      uint2 h4, l4;
      split4<true>(v, h4, l4);
      const uint32_t h4w[2] = {h4.x, h4.y}, l4w[2] = {l4.x, l4.y};
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int w = j >> 1, sh = 16 * (j & 1);
        uint32_t* o = out + (e0 + j) * 7;
        o[0] = (h2[w] >> sh) & 0xffffu;
        o[1] = (l2[w] >> sh) & 0xffffu;
        o[2] = (hp[w] >> sh) & 0xffffu;
        o[3] = (lp[w] >> sh) & 0xffffu;
        o[4] = (h4w[w] >> sh) & 0xffffu;
        o[5] = (l4w[w] >> sh) & 0xffffu;
        o[6] = f2bf(v[j]);
      }
    } else if constexpr (KIND == PROBE_F16_PAIR) {  // 3 words: split4_f16 hi, lo | f2h
      uint2 hi, lo;
      split4_f16(v, hi, lo);
      const uint32_t hw[2] = {hi.x, hi.y}, lw[2] = {lo.x, lo.y};
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int w = j >> 1, sh = 16 * (j & 1);
        uint32_t* o = out + (e0 + j) * 3;
        o[0] = (hw[w] >> sh) & 0xffffu;
        o[1] = (lw[w] >> sh) & 0xffffu;
        o[2] = f2h(v[j]);
      }
    } else if constexpr (KIND == PROBE_F16_F8) {  // 2 words: split4_f8 hi (fp16 bits), lo (e4m3 byte)
      uint2 hi;
      uint32_t lo8;
      split4_f8(v, hi, lo8);
      const uint32_t hw[2] = {hi.x, hi.y};
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        uint32_t* o = out + (e0 + j) * 2;
        o[0] = (hw[j >> 1] >> (16 * (j & 1))) & 0xffffu;
        o[1] = (lo8 >> (8 * j)) & 0xffu;
      }
    } else {  // PROBE_E4M3_F32, 3 words: f32x4_to_e4m3 | the weight's e4m3 plane | the weight's lo plane (pack kernels)
      static_assert(KIND == PROBE_E4M3_F32, "unknown conversion kind");
      const uint32_t w = f32x4_to_e4m3(v);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float vj = v[j];
        const _Float16 hv = (_Float16)vj;
        uint32_t* o = out + (e0 + j) * 3;
        o[0] = (w >> (8 * j)) & 0xffu;
        o[1] = f2e4m3(vj * (float)(1 << F8_W_SHIFT));
        o[2] = f2e4m3((vj - (float)hv) * (float)(1 << (F8_LO_SHIFT + F8_W_SHIFT)));
      }
    }
  }
}

// fp32 functions.  GROUP inputs per record: GELU / EXP2 1, ROPE 4 (x1, x2, c, s), KEEP_PROB 2 (l0, l1).
// out: two fp32 per record (KEEP_PROB: one).
template <int KIND, int MODE>
__global__ void probe_function_kernel(const float* __restrict__ in, size_t n, float* __restrict__ out) {
  probe_set_mode<MODE>();
  const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if constexpr (KIND == PROBE_GELU) {  // four values per thread: the staged form runs each stage over all of them
    if (t >= (n + 3) / 4) return;
    float x[4], staged[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) x[j] = t * 4 + j < n ? in[t * 4 + j] : 0.f;
    probe_gelu_staged<4>(x, staged);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (t * 4 + j < n) {
        out[(t * 4 + j) * 2 + 0] = gelu_erf(x[j]);
        out[(t * 4 + j) * 2 + 1] = staged[j];
      }
    }
  } else if constexpr (KIND == PROBE_EXP2) {
    if (t >= n) return;
    const float x = in[t];
    out[t * 2 + 0] = __builtin_amdgcn_exp2f(x);
    out[t * 2 + 1] = __expf(x);
  } else if constexpr (KIND == PROBE_ROPE) {
    if (t >= n / 4) return;
    const float x1 = in[t * 4 + 0], x2 = in[t * 4 + 1], c = in[t * 4 + 2], s = in[t * 4 + 3];
    out[t * 2 + 0] = rope_lo(x1, x2, c, s);
    out[t * 2 + 1] = rope_hi(x1, x2, c, s);
  } else {
    static_assert(KIND == PROBE_KEEP_PROB, "unknown function kind");
    if (t >= n / 2) return;
    out[t] = keep_prob_of(in[t * 2 + 0], in[t * 2 + 1]);
  }
}

// The scaled e4m3 products, one wave per (a, b): every byte of the X operand is a, every byte of Y is b, so every element of
// D is 128 a b x (the product of the two block scales) whatever the fragment layout.  in: n / 2 byte pairs; out: four
// 16 x 16 fp32 tiles per pair, in the order mfma8<false>, mfma8<true>, mfma8w<false>, mfma8w<true>.
template <int MODE>
__global__ void probe_mfma_scale_kernel(const unsigned char* __restrict__ in, size_t n, float* __restrict__ out) {
  probe_set_mode<MODE>();
  const size_t pair = blockIdx.x;
  if (pair >= n / 2) return;
  const int lane = threadIdx.x;
  const int a = (int)(0x01010101u * (uint32_t)in[pair * 2 + 0]), b = (int)(0x01010101u * (uint32_t)in[pair * 2 + 1]);
  const i32x8 x = {a, a, a, a, a, a, a, a}, y = {b, b, b, b, b, b, b, b};
  const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
  const f32x4 d[4] = {mfma8<false>(x, y, zero), mfma8<true>(x, y, zero), mfma8w<false>(x, y, zero), mfma8w<true>(x, y, zero)};
#pragma unroll
  for (int tl = 0; tl < 4; ++tl) {
    float* o = out + (pair * 4 + tl) * 256 + (size_t)lane * 4;
#pragma unroll
    for (int r = 0; r < 4; ++r) o[r] = d[tl][r];
  }
}

}  // namespace opk
