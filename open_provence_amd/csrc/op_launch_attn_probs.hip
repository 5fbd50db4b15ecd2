// op_launch_attn_probs.hip -- launches of op_attention_probs' own kernels (opk_attn_probs.hip.h): the gather of a packed fp32
// hidden state into the row layout, the probability kernel, and the single-query row kernel of op_attention_rows.
#define OPK_ATTN_PROBS_KERNELS 1
#include <algorithm>

#include "op_internal.h"

namespace opl {
using namespace opk;

void launch_attn_probs_gather(hipStream_t st, const float* packed, const int32_t* row_tok, int H, int r_pad, float* x) {
  hipLaunchKernelGGL(gather_rows_f32_kernel, dim3((unsigned)((r_pad + 3) / 4)), dim3(256), 0, st, packed, row_tok, H, r_pad, x);
}

void launch_attn_probs(hipStream_t st, const AttnProbsParams& p, int n_seqs) {
  const unsigned q_blocks = (unsigned)((p.width + ATT_BQ - 1) / ATT_BQ);
  for (int z0 = 0; z0 < n_seqs; z0 += 65535) {  // (a grid's z extent)
    AttnProbsParams part = p;
    part.s0 = p.s0 + z0;
    part.roff = p.roff + z0;
    hipLaunchKernelGGL(attn_probs_f32_kernel, dim3(q_blocks, (unsigned)p.num_heads, (unsigned)std::min(n_seqs - z0, 65535)), dim3(256), 0, st,
                       part);
  }
}

void launch_attn_rows(hipStream_t st, const AttnRowsParams& p, int n_seqs, bool head_mean) {
  for (int z0 = 0; z0 < n_seqs; z0 += 65535) {  // (a grid's z extent)
    AttnRowsParams part = p;
    part.s0 = p.s0 + z0;
    part.roff = p.roff + z0;
    const unsigned nz = (unsigned)std::min(n_seqs - z0, 65535);
    // head mean: one block per sequence walks the heads one after the other; a small batch leaves most of the chip idle that
    // way, so its blocks split the output row's key tiles among them (the same bits either way)
    const unsigned n_kt = (unsigned)((p.width + ATT_BK - 1) / ATT_BK);
    if (head_mean)
      hipLaunchKernelGGL((attn_rows_f32_kernel<true>), dim3(n_seqs <= 128 ? n_kt : 1u, 1, nz), dim3(256), 0, st, part);
    else
      hipLaunchKernelGGL((attn_rows_f32_kernel<false>), dim3(1, (unsigned)p.num_heads, nz), dim3(256), 0, st, part);
  }
}

}  // namespace opl
