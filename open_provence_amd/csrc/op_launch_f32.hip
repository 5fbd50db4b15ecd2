// op_launch_f32.hip -- launches of kernel set "fp32" (opk_f32.hip.h): LayerNorm, the GEMM with its three epilogues, attention,
// the ranking head.
#define OPK_F32_KERNELS 1
#include "op_internal.h"

namespace opl {
using namespace opk;

void launch_f32_ln(hipStream_t st, const float* x, const float* w, float eps, int H, int r_pad, float* out) {
  hipLaunchKernelGGL(ln_f32_kernel, dim3((unsigned)((r_pad + 3) / 4)), dim3(256), 0, st, x, w, eps, H, r_pad, out);
}

bool launch_f32_gemm(hipStream_t st, const F32GemmParams& p, int epi) {
  const dim3 grid((unsigned)(p.n_tiles * p.m_tiles));
  switch (epi) {
    case F32_EPI_QKV: hipLaunchKernelGGL((gemm_f32_kernel<F32_EPI_QKV>), grid, dim3(256), 0, st, p); return true;
    case F32_EPI_RESIDUAL: hipLaunchKernelGGL((gemm_f32_kernel<F32_EPI_RESIDUAL>), grid, dim3(256), 0, st, p); return true;
    case F32_EPI_GEGLU: hipLaunchKernelGGL((gemm_f32_kernel<F32_EPI_GEGLU>), grid, dim3(256), 0, st, p); return true;
    default: return false;
  }
}

void launch_f32_attn(hipStream_t st, const F32AttnParams& p, dim3 grid) {
  hipLaunchKernelGGL(attn_f32_kernel, grid, dim3(256), 0, st, p);
}

void launch_f32_rank_head(hipStream_t st, int n_seqs, const float* cls, const float* y, const int32_t* cu, int s0, const int32_t* roff,
                          int mean_pool, int H, int nl, const float* dense_t, const float* head_norm, float eps, const float* cls_w,
                          const float* cls_b, float* rank_out) {
  hipLaunchKernelGGL(rank_head_f32_kernel, dim3((unsigned)n_seqs), dim3(256), 0, st, cls, y, cu, s0, roff, mean_pool, H, nl, dense_t,
                     head_norm, eps, cls_w, cls_b, rank_out);
}

}  // namespace opl
