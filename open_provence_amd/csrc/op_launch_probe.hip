// op_launch_probe.hip -- launches of op_debug_primitive's kernels (opk_probe.hip.h): one instantiation per (kind, mode).
#include "op_internal.h"
#include "opk_probe.hip.h"

namespace opl {
using namespace opk;

int probe_group_size(int kind) {
  switch (kind) {
    case PROBE_BF16_SPLIT:
    case PROBE_F16_PAIR:
    case PROBE_F16_F8:
    case PROBE_E4M3_F16:
    case PROBE_E4M3_F32:
    case PROBE_ROPE: return 4;
    case PROBE_GELU:
    case PROBE_EXP2: return 1;
    case PROBE_KEEP_PROB:
    case PROBE_MFMA_SCALE: return 2;
    default: return 0;
  }
}

namespace {

inline dim3 probe_grid(size_t threads) { return dim3((unsigned)((threads + 255) / 256)); }

template <int MODE>
void launch_probe_mode(hipStream_t st, int kind, const void* in, size_t n, void* out) {
  uint32_t* ow = reinterpret_cast<uint32_t*>(out);
  const float* fin = reinterpret_cast<const float*>(in);
  float* fo = reinterpret_cast<float*>(out);
  switch (kind) {
    case PROBE_BF16_SPLIT: hipLaunchKernelGGL((probe_convert_kernel<PROBE_BF16_SPLIT, MODE>), probe_grid(n / 4), dim3(256), 0, st, in, n, ow); break;
    case PROBE_F16_PAIR: hipLaunchKernelGGL((probe_convert_kernel<PROBE_F16_PAIR, MODE>), probe_grid(n / 4), dim3(256), 0, st, in, n, ow); break;
    case PROBE_F16_F8: hipLaunchKernelGGL((probe_convert_kernel<PROBE_F16_F8, MODE>), probe_grid(n / 4), dim3(256), 0, st, in, n, ow); break;
    case PROBE_E4M3_F16: hipLaunchKernelGGL((probe_convert_kernel<PROBE_E4M3_F16, MODE>), probe_grid(n / 4), dim3(256), 0, st, in, n, ow); break;
    case PROBE_E4M3_F32: hipLaunchKernelGGL((probe_convert_kernel<PROBE_E4M3_F32, MODE>), probe_grid(n / 4), dim3(256), 0, st, in, n, ow); break;
    case PROBE_GELU: hipLaunchKernelGGL((probe_function_kernel<PROBE_GELU, MODE>), probe_grid((n + 3) / 4), dim3(256), 0, st, fin, n, fo); break;
    case PROBE_EXP2: hipLaunchKernelGGL((probe_function_kernel<PROBE_EXP2, MODE>), probe_grid(n), dim3(256), 0, st, fin, n, fo); break;
    case PROBE_ROPE: hipLaunchKernelGGL((probe_function_kernel<PROBE_ROPE, MODE>), probe_grid(n / 4), dim3(256), 0, st, fin, n, fo); break;
    case PROBE_KEEP_PROB: hipLaunchKernelGGL((probe_function_kernel<PROBE_KEEP_PROB, MODE>), probe_grid(n / 2), dim3(256), 0, st, fin, n, fo); break;
    default:  // PROBE_MFMA_SCALE (the caller has checked the kind): one wave per pair
      hipLaunchKernelGGL((probe_mfma_scale_kernel<MODE>), dim3((unsigned)(n / 2)), dim3(64), 0, st, reinterpret_cast<const unsigned char*>(in), n,
                         fo);
      break;
  }
}

}  // namespace

void launch_probe(hipStream_t st, int kind, int mode, const void* in, size_t n, void* out) {
  if (mode != 0) launch_probe_mode<1>(st, kind, in, n, out);
  else launch_probe_mode<0>(st, kind, in, n, out);
}

}  // namespace opl
