// op_launch_f32_masked.hip -- launches of op_forward_masked's own kernels (opk_f32_masked.hip.h): the id check with the dense
// cu_seqlens, the row means of v, attention under a key mask, the ranking head with masked mean pooling, the pruning logits'
// zeros at masked positions.
#define OPK_F32_MASKED_KERNELS 1
#include "op_internal.h"

#include <algorithm>

namespace opl {
using namespace opk;

void launch_masked_prepare(hipStream_t st, const int32_t* ids, int n_rows, int width, int vocab, int32_t* cu, uint32_t* status) {
  const size_t n = std::max((size_t)n_rows * (size_t)width, (size_t)n_rows + 1);
  hipLaunchKernelGGL(masked_prepare_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, ids, n_rows, width, vocab, cu, status);
}

void launch_f32_vmean(hipStream_t st, const float* v, const int32_t* cu, int s0, const int32_t* roff, int H, int n_seqs, float* vmean) {
  hipLaunchKernelGGL(vmean_f32_kernel, dim3((unsigned)n_seqs, (unsigned)((H + 255) / 256)), dim3(256), 0, st, v, cu, s0, roff, H, vmean);
}

void launch_f32_attn_masked(hipStream_t st, const F32MaskedAttnParams& p, dim3 grid) {
  hipLaunchKernelGGL(attn_f32_masked_kernel, grid, dim3(256), 0, st, p);
}

void launch_f32_rank_head_masked(hipStream_t st, int n_seqs, const float* cls, const float* y, const int32_t* cu, int s0,
                                 const int32_t* roff, const uint8_t* key_ok, int mean_pool, int H, int nl, const float* dense_t,
                                 const float* head_norm, float eps, const float* cls_w, const float* cls_b, float* rank_out) {
  hipLaunchKernelGGL(rank_head_f32_masked_kernel, dim3((unsigned)n_seqs), dim3(256), 0, st, cls, y, cu, s0, roff, key_ok, mean_pool, H,
                     nl, dense_t, head_norm, eps, cls_w, cls_b, rank_out);
}

void launch_prune_mask(hipStream_t st, float* prune, const uint8_t* key_ok, size_t t0, size_t n_tokens) {
  if (n_tokens == 0) return;
  hipLaunchKernelGGL(prune_mask_f32_kernel, dim3((unsigned)((n_tokens + 255) / 256)), dim3(256), 0, st, prune, key_ok, t0, n_tokens);
}

}  // namespace opl
