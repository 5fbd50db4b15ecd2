// op_launch_audit.hip -- launches of the running audit's kernels (opk_audit.hip.h).
#include <algorithm>

#include "op_internal.h"
#include "opk_audit.hip.h"

namespace opl {
using namespace opk;

static_assert(COV_WORDS == COV_ST_WORDS && COV_MAXLEN == COV_ST_MAXLEN && COV_NOVEL == COV_ST_NOVEL && COV_LONGEST == COV_ST_LONGEST,
              "op_internal.h and opk_audit.hip.h disagree on the coverage state block");

void launch_coverage_scan(hipStream_t st, const int32_t* ids, const int32_t* cu, int n_seqs, int total, int vocab, const uint32_t* bits,
                          int32_t* row_novel, uint32_t* state) {
  hipLaunchKernelGGL(coverage_scan_kernel, dim3((unsigned)((n_seqs + 3) / 4)), dim3(256), 0, st, ids, cu, n_seqs, total, vocab, bits,
                     row_novel, state);
}

void launch_coverage_commit(hipStream_t st, const int32_t* ids, const int32_t* cu, int n_seqs, int total, const int32_t* rows, int n_rows,
                            int vocab, uint32_t* bits, uint32_t* state) {
  hipLaunchKernelGGL(coverage_commit_kernel, dim3((unsigned)((n_rows + 3) / 4)), dim3(256), 0, st, ids, cu, n_seqs, total, rows, n_rows,
                     vocab, bits, state);
}

void launch_gather_rows(hipStream_t st, const int32_t* ids, const int32_t* cu, int n_seqs, int total, const int32_t* rows, int n_rows,
                        int32_t* sub_ids, int32_t* sub_cu) {
  hipLaunchKernelGGL(gather_offsets_kernel, dim3(1), dim3(1024), 0, st, cu, n_seqs, total, rows, n_rows, sub_cu);
  // (row lengths are not on the host: 8 chunks of 256 columns stride over a row of any length)
  hipLaunchKernelGGL(gather_rows_kernel, dim3((unsigned)n_rows, 8), dim3(256), 0, st, ids, cu, n_seqs, total, rows, sub_cu, sub_ids);
}

void launch_audit_compare(hipStream_t st, const float* prune, const float* rank, const int32_t* cu, int n_seqs, int total,
                          const int32_t* rows, int n_rows, const float* sub_prune, const float* sub_rank, const int32_t* sub_cu,
                          int n_labels, float* err) {
  hipLaunchKernelGGL(audit_compare_kernel, dim3((unsigned)n_rows, 8), dim3(256), 0, st, prune, rank, cu, n_seqs, total, rows, sub_prune,
                     sub_rank, sub_cu, n_labels, err);
}

}  // namespace opl
