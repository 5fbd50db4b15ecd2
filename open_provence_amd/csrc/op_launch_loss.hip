// op_launch_loss.hip -- instantiations of the loss kernels (opk_loss.hip.h) for every kind / label type.
#include <algorithm>

#include "opk_loss.hip.h"

namespace opl {
using namespace opk;

namespace {

constexpr int LABELS_I32 = 0, LABELS_I64 = 1, LABELS_F32 = 3;  // enum op_int_dtype, OP_LABELS_F32

// blocks for n work items of `per_block` each: at least one, at most the cap (the kernels stride beyond it)
int loss_grid(long long n, int per_block) { return (int)std::min<long long>(std::max<long long>((n + per_block - 1) / per_block, 1), LOSS_MAX_BLOCKS); }

template <typename LabelT>
void finish(hipStream_t st, LossScratch* scratch, int n_partials, const void* labels, float* loss_dev) {
  hipLaunchKernelGGL((loss_finish_kernel<LabelT>), dim3(1), dim3(64), 0, st, scratch, n_partials, static_cast<const LabelT*>(labels), loss_dev);
}

}  // namespace

bool launch_loss(hipStream_t st, int kind, int labels_dtype, const LossParams& p, LossScratch* scratch, float* loss_dev) {
  const bool integer = kind == LOSS_TOKEN_CE || kind == LOSS_RANK_CE;
  if (integer ? (labels_dtype != LABELS_I32 && labels_dtype != LABELS_I64) : labels_dtype != LABELS_F32) return false;
  const bool i64 = labels_dtype == LABELS_I64;
  int blocks = 0;
  if (p.n_rows > 0) {
    switch (kind) {
      case LOSS_TOKEN_CE:
        blocks = loss_grid(p.n_rows, LOSS_THREADS / 64);
        if (i64) hipLaunchKernelGGL((loss_token_ce_kernel<int64_t>), dim3(blocks), dim3(LOSS_THREADS), 0, st, p, scratch);
        else hipLaunchKernelGGL((loss_token_ce_kernel<int32_t>), dim3(blocks), dim3(LOSS_THREADS), 0, st, p, scratch);
        break;
      case LOSS_RANK_BCE:
        blocks = loss_grid(p.n_rows, LOSS_THREADS);
        hipLaunchKernelGGL((loss_rank_bce_kernel<>), dim3(blocks), dim3(LOSS_THREADS), 0, st, p, scratch);
        break;
      case LOSS_RANK_CE:
        blocks = loss_grid(p.n_rows, LOSS_THREADS);
        if (i64) hipLaunchKernelGGL((loss_rank_ce_kernel<int64_t>), dim3(blocks), dim3(LOSS_THREADS), 0, st, p, scratch);
        else hipLaunchKernelGGL((loss_rank_ce_kernel<int32_t>), dim3(blocks), dim3(LOSS_THREADS), 0, st, p, scratch);
        break;
      case LOSS_RANK_MSE:
        blocks = loss_grid((long long)p.n_rows * p.channels, LOSS_THREADS);
        hipLaunchKernelGGL((loss_rank_mse_kernel<>), dim3(blocks), dim3(LOSS_THREADS), 0, st, p, scratch);
        break;
      default:
        return false;
    }
  } else if (kind < LOSS_TOKEN_CE || kind > LOSS_RANK_MSE) {
    return false;
  }
  if (!integer) finish<float>(st, scratch, blocks, p.labels, loss_dev);
  else if (i64) finish<int64_t>(st, scratch, blocks, p.labels, loss_dev);
  else finish<int32_t>(st, scratch, blocks, p.labels, loss_dev);
  return true;
}

}  // namespace opl
