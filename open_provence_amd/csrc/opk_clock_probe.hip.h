// opk_clock_probe.hip.h -- op_debug_clock_probe's kernel (included by op_api.hip only)
#pragma once

#include "opk_common.hip.h"

namespace opk {

// one wave: shader cycles and 100 MHz ticks over a spin of `ticks` ticks (op_debug_clock_probe)
__global__ void clock_probe_kernel(unsigned long long ticks, unsigned long long* __restrict__ out) {
  const unsigned long long c0 = __builtin_readcyclecounter();
  const unsigned long long r0 = wall_clock64();
  unsigned long long r1 = r0;
  while (r1 - r0 < ticks) {
    __builtin_amdgcn_s_sleep(32);
    r1 = wall_clock64();
  }
  const unsigned long long c1 = __builtin_readcyclecounter();
  if (threadIdx.x == 0) {
    out[0] = c1 - c0;
    out[1] = r1 - r0;
  }
}

}  // namespace opk
