// op_launch_attn_masked.hip -- the key-mask form of attn_fp_kernel (KM; opk_attn.hip.h) for every (policy, waves, keys per
// tile, format) combination op_launch_attn.hip serves: op_forward_masked_native's attention.  A unit of its own, so that it
// compiles beside that one.
#include "op_internal.h"

namespace opl {
using namespace opk;

namespace {

#ifndef OPK_ATTN_LOCAL_STAGES
#define OPK_ATTN_LOCAL_STAGES 2  // (as op_launch_attn.hip)
#endif

template <int PI, int WAVES, int KT>
void launch_one_masked(hipStream_t st, const AttnFpParams& p, dim3 grid) {
  constexpr Policy P = kPolicies[PI];
  constexpr int NST = KT == 1 ? OPK_ATTN_LOCAL_STAGES : 2;
  hipLaunchKernelGGL((attn_fp_kernel<P.qk, P.pv, o_lo(P), WAVES, KT, false, P.fmt == 1, NST, P.fmt == 2, true>), grid, dim3(WAVES * 64), 0,
                     st, p);
}

template <int PI>
bool launch_pi_masked(hipStream_t st, const AttnFpParams& p, int waves, int kt, dim3 grid) {
  if (waves == 8 && kt == 2) launch_one_masked<PI, 8, 2>(st, p, grid);
  else if (waves == 4 && kt == 2) launch_one_masked<PI, 4, 2>(st, p, grid);
  else if (waves == 4 && kt == 1) launch_one_masked<PI, 4, 1>(st, p, grid);
  else return false;
  return true;
}

}  // namespace

bool launch_attn_masked(hipStream_t st, const AttnFpParams& p, int waves, int kt, int pi, bool zero_p_lo, dim3 grid, bool f16_in_f8_out) {
  if (p.key_row == nullptr) return false;
  if (f16_in_f8_out) {
    if (zero_p_lo || (pi != PI_F16_F8 && pi != PI_F16_F8_W)) return false;
    if (waves == 8 && kt == 2) hipLaunchKernelGGL((attn_fp_kernel<0, 0, false, 8, 2, false, true, 2, true, true>), grid, dim3(512), 0, st, p);
    else if (waves == 4 && kt == 2) hipLaunchKernelGGL((attn_fp_kernel<0, 0, false, 4, 2, false, true, 2, true, true>), grid, dim3(256), 0, st, p);
    else if (waves == 4 && kt == 1)
      hipLaunchKernelGGL((attn_fp_kernel<0, 0, false, 4, 1, false, true, OPK_ATTN_LOCAL_STAGES, true, true>), grid, dim3(256), 0, st, p);
    else return false;
    return true;
  }
  if (zero_p_lo) {  // all-terms instantiation with lo(p) cleared
    if (pi != 0) return false;
    if (waves == 8 && kt == 2) hipLaunchKernelGGL((attn_fp_kernel<3, 3, true, 8, 2, true, false, 2, false, true>), grid, dim3(512), 0, st, p);
    else if (waves == 4 && kt == 2) hipLaunchKernelGGL((attn_fp_kernel<3, 3, true, 4, 2, true, false, 2, false, true>), grid, dim3(256), 0, st, p);
    else if (waves == 4 && kt == 1) hipLaunchKernelGGL((attn_fp_kernel<3, 3, true, 4, 1, true, false, 2, false, true>), grid, dim3(256), 0, st, p);
    else return false;
    return true;
  }
  static_assert(N_POLICIES == 6, "extend the switch below");
  switch (pi) {
    case 5: return launch_pi_masked<5>(st, p, waves, kt, grid);
    case 0: return launch_pi_masked<0>(st, p, waves, kt, grid);
    case 1: return launch_pi_masked<1>(st, p, waves, kt, grid);
    case 2: return launch_pi_masked<2>(st, p, waves, kt, grid);
    case 3: return launch_pi_masked<3>(st, p, waves, kt, grid);
    case 4: return launch_pi_masked<4>(st, p, waves, kt, grid);
    default: return false;
  }
}

}  // namespace opl
