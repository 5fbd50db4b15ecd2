// op_policy.h -- the precision policies the kernel families are instantiated for.  No HIP: op_internal.h hands it to the
// launch units, op_kernel_sets.h / op_plan.h to host-only code.
#pragma once

namespace opl {

// Precision policy = one term mask per contraction family (opk::T_LEFT_LO / T_RIGHT_LO; see op_gemm_family in
// include/open_provence_hip.h for the order).  "left" is always the activation-side operand:
//   wqkv: LN(x) x Wqkv    qk: q x k    pv: p x v    attn_out: o x Wo    wi: LN(x) x Wi    mlp_out: h x Wo
struct Policy {
  int wqkv, qk, pv, attn_out, wi, mlp_out;
  int fmt = 0;  // operand format: 0 = (hi, lo) bf16 planes, 1 = fp16 hi + e4m3 lo in the whole-layer kernel (opk_common.hip.h), 2 = fp16 single plane everywhere
  constexpr bool operator==(const Policy& o) const {
    return wqkv == o.wqkv && qk == o.qk && pv == o.pv && attn_out == o.attn_out && wi == o.wi && mlp_out == o.mlp_out;
  }
};

// Curated policies: every kernel family is instantiated with exactly the product terms (and output lo planes) each
// of these needs.  Any other policy runs on the kernels of kPolicies[0] (all terms) with the unused lo operands
// cleared -- bit-identical numerics, no speed-up.
//   0  bf16x3                 every operand (hi, lo)
//   1  bf16 weights           weight lo planes are zero (bf16 checkpoint, or OP_PRECISION_BF16X2): 2 passes in the four
//                             weight GEMMs, 3 in attention (q, k, p, v are all activations)
//   2  bf16                   single pass everywhere
//   3  f16 + fp8              the terms of set 1 with the whole-layer kernel's operands as fp16 hi + e4m3 lo: 1.5 MFMA
//                             units per product instead of 2 (hidden <= 256, weights exactly representable in fp16;
//                             layer-0 q / k / v and attention run set 1's kernels, attention writes o in the new format).
//                             Never matched by terms (operator== ignores fmt): the default selection upgrades 1 -> 3.
//   4  f16 + fp8, all terms   the terms of set 0 (fp32-valued weights) in the same format: the weight's lo part rides as a
//                             third e4m3 plane (bf16 for the MLP output projection): 2 MFMA units per product instead of 3,
//                             and ONE kernel per layer where set 0 needs two with h through HBM.  Default selection: 0 -> 4.
//   5  f16                    (round 5) single pass with every operand as fp16: the kernels and layouts of set 2, 11 instead of
//                             8 significant bits per operand.  Never matched by terms and never a default: op_calibrate /
//                             op_select_kernel_set choose it when the loaded weights allow (reported as kernel set 7).
constexpr Policy kPolicies[] = {
    {3, 3, 3, 3, 3, 3},
    {1, 3, 3, 1, 1, 1},
    {0, 0, 0, 0, 0, 0},
    {1, 3, 3, 1, 1, 1, 1},
    {3, 3, 3, 3, 3, 3, 1},
    {0, 0, 0, 0, 0, 0, 2},
};
constexpr int PI_ALL_TERMS = 0, PI_BF16_WEIGHTS = 1, PI_BF16 = 2, PI_F16_F8 = 3, PI_F16_F8_W = 4, PI_F16 = 5;
constexpr int N_POLICIES = (int)(sizeof(kPolicies) / sizeof(kPolicies[0]));

}  // namespace opl
