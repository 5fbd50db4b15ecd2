// op_launch_padded.hip -- instantiations of the padded-boundary kernels (opk_padded.hip.h) for every id / mask type.
#include <algorithm>

#include "op_internal.h"
#include "opk_padded.hip.h"

namespace opl {
using namespace opk;

namespace {

template <typename IdT, typename MaskT>
void lengths_one(hipStream_t st, const void* ids, const void* mask, int n_rows, int width, int vocab, int32_t* cu, uint32_t* status) {
  hipLaunchKernelGGL((padded_lengths_kernel<IdT, MaskT>), dim3((unsigned)((n_rows + 3) / 4)), dim3(256), 0, st,
                     static_cast<const IdT*>(ids), static_cast<const MaskT*>(mask), n_rows, width, vocab, cu + 1, status);
}

template <typename IdT>
bool lengths_ids(hipStream_t st, const void* ids, const void* mask, int mask_dtype, int n_rows, int width, int vocab, int32_t* cu,
                 uint32_t* status) {
  if (!mask) lengths_one<IdT, NoMask>(st, ids, nullptr, n_rows, width, vocab, cu, status);
  else if (mask_dtype == PAD_INT_I32) lengths_one<IdT, int32_t>(st, ids, mask, n_rows, width, vocab, cu, status);
  else if (mask_dtype == PAD_INT_I64) lengths_one<IdT, int64_t>(st, ids, mask, n_rows, width, vocab, cu, status);
  else if (mask_dtype == PAD_INT_U8) lengths_one<IdT, uint8_t>(st, ids, mask, n_rows, width, vocab, cu, status);
  else return false;
  return true;
}

}  // namespace

bool launch_padded_pack(hipStream_t st, const void* ids, int ids_dtype, const void* mask, int mask_dtype, int n_rows, int width,
                        int vocab, int32_t* ids_packed, int32_t* cu, uint32_t* status) {
  if (ids_dtype != PAD_INT_I32 && ids_dtype != PAD_INT_I64) return false;
  const bool i64 = ids_dtype == PAD_INT_I64;
  if (!(i64 ? lengths_ids<int64_t>(st, ids, mask, mask_dtype, n_rows, width, vocab, cu, status)
            : lengths_ids<int32_t>(st, ids, mask, mask_dtype, n_rows, width, vocab, cu, status)))
    return false;
  const dim3 gather_grid((unsigned)n_rows, (unsigned)std::min((width + 255) / 256, 64));
  if (i64) {
    hipLaunchKernelGGL((padded_scan_kernel<int64_t>), dim3(1), dim3(1024), 0, st, cu, n_rows, static_cast<const int64_t*>(ids), status);
    hipLaunchKernelGGL((padded_gather_kernel<int64_t>), gather_grid, dim3(256), 0, st, static_cast<const int64_t*>(ids), cu, width, ids_packed);
  } else {
    hipLaunchKernelGGL((padded_scan_kernel<int32_t>), dim3(1), dim3(1024), 0, st, cu, n_rows, static_cast<const int32_t*>(ids), status);
    hipLaunchKernelGGL((padded_gather_kernel<int32_t>), gather_grid, dim3(256), 0, st, static_cast<const int32_t*>(ids), cu, width, ids_packed);
  }
  return true;
}

bool launch_padded_scatter(hipStream_t st, const float* packed, const int32_t* cu, int n_rows, int width, int channels, float* padded) {
  const size_t n = (size_t)n_rows * (size_t)width * (size_t)channels;
  const dim3 grid((unsigned)((n + 1023) / 1024));
  const bool wide = (reinterpret_cast<uintptr_t>(padded) & 15) == 0;
  if (channels == 1) hipLaunchKernelGGL((padded_scatter_kernel<1>), grid, dim3(256), 0, st, packed, cu, n_rows, width, padded, wide);
  else if (channels == 2) hipLaunchKernelGGL((padded_scatter_kernel<2>), grid, dim3(256), 0, st, packed, cu, n_rows, width, padded, wide);
  else return false;
  return true;
}

}  // namespace opl
