// opk_load.hip.h -- weight loading: conversion to fp32, the tiled path's plane split, the transpose, and the fp16-fit verdict of
// the "f16 + fp8" packs (included by op_weights.hip only; the pack kernels of each family are in that family's header, behind
// OPK_PACK_KERNELS)
#pragma once

#include "opk_common.hip.h"

namespace opk {

// ----------------------------------------------------------------------------------------------
// weight re-packing (runs once per tensor at load time)
// ----------------------------------------------------------------------------------------------
__global__ void convert_to_f32_kernel(const void* __restrict__ src, int dtype, size_t n, float* __restrict__ dst) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  if (dtype == 0) {
    dst[i] = reinterpret_cast<const float*>(src)[i];
  } else if (dtype == 1) {
    dst[i] = bf2f(reinterpret_cast<const u16*>(src)[i]);
  } else {
    dst[i] = __half2float(reinterpret_cast<const __half*>(src)[i]);
  }
}

// dst planes [rows][cols]; source row for destination row r is perm(r): identity, or the GeGLU
// interleave that puts the 32 "input" rows and the 32 matching "gate" rows of Wi in one 64-row slab.
// Every weight-splitting kernel reports whether the tensor has ANY non-zero lo element (`any_lo`, set to 1; a bf16
// checkpoint has none, and then the hi x lo(weight) product term can be dropped without changing a bit), and
// `zero_lo` stores zeros in the lo plane (a precision policy without that term, run on a kernel that has it).
__global__ void split_planes_kernel(const float* __restrict__ src, int rows, int cols, int geglu_half,
                                    u16* __restrict__ hi, u16* __restrict__ lo, int zero_lo, int* __restrict__ any_lo) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (size_t)rows * cols) return;
  const int r = (int)(i / cols), c = (int)(i % cols);
  int sr = r;
  if (geglu_half > 0) {
    const int b = r >> 6, j = r & 63;
    sr = (j < 32) ? (b * 32 + j) : (geglu_half + b * 32 + (j - 32));
  }
  const float v = src[(size_t)sr * cols + c];
  const u16 h = f2bf(v);
  const u16 l = f2bf(v - bf2f(h));
  if ((l & 0x7fffu) != 0) *any_lo = 1;
  hi[i] = h;
  lo[i] = zero_lo ? (u16)0 : l;
}

__global__ void transpose_f32_kernel(const float* __restrict__ src, int rows, int cols, float* __restrict__ dst) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (size_t)rows * cols) return;
  const int r = (int)(i / cols), c = (int)(i % cols);
  dst[(size_t)c * rows + r] = src[i];
}

// "f16 + fp8" packs, per weight tensor (note_f16_fit in opk_common.hip.h): the tensor's energy (x 2^60, as the lost part),
// and the verdict once its pack kernels have run
__global__ __launch_bounds__(256) void weight_energy_kernel(const float* __restrict__ w, size_t n, float* __restrict__ fit) {
  float acc = 0.f;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) acc += w[i] * w[i];
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) acc += __shfl_xor(acc, off);
  if ((threadIdx.x & 63) == 0) atomicAdd(fit + 1, acc * 1.1529215e18f);
}
__global__ void f16_fit_close_tensor_kernel(int* __restrict__ flags, float* __restrict__ fit) {
  if (fit[0] > fit[1] * 1.4551915e-11f) flags[2] = 1;  // 2^-36
  fit[0] = 0.f;
  fit[1] = 0.f;
}

}  // namespace opk
