// op_launch_assemble.hip -- launch of op_assemble_rows' kernel (opk_assemble.hip.h).
#include "op_internal.h"
#include "opk_assemble.hip.h"

namespace opl {
using namespace opk;

static_assert(ASSEMBLE_PIECE_MAX == ASSEMBLE_MAX_PIECE, "op_internal.h and opk_assemble.hip.h disagree on the template pieces");

void launch_assemble_rows(hipStream_t st, const int32_t* corpus, const int32_t* frag_off, int n_frag, int n_corpus, const int32_t* query_ids,
                          const int32_t* q_off, int n_queries, int n_query_tokens, const int32_t* const pieces[3], const int n_pieces[3],
                          const int32_t* plan, const int32_t* cu, int n_rows, int total, int32_t* out) {
  AssemblePieces pc = {};
  for (int i = 0; i < n_pieces[0]; ++i) pc.prefix[i] = pieces[0][i];
  for (int i = 0; i < n_pieces[1]; ++i) pc.middle[i] = pieces[1][i];
  for (int i = 0; i < n_pieces[2]; ++i) pc.suffix[i] = pieces[2][i];
  pc.n_prefix = n_pieces[0], pc.n_middle = n_pieces[1], pc.n_suffix = n_pieces[2];
  const long long waves = (long long)n_rows * ASSEMBLE_SEGMENTS;
  hipLaunchKernelGGL(assemble_rows_kernel, dim3((unsigned)((waves + 3) / 4)), dim3(256), 0, st, corpus, frag_off, n_frag, n_corpus, query_ids,
                     q_off, n_queries, n_query_tokens, pc, plan, cu, n_rows, total, out);
}

}  // namespace opl
