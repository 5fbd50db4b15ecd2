// op_kernel_sets.h -- kKernelSets: what each OP_KS_* kernel set is: the kernels it runs, the operand format of each part of a
// layer, the terms it evaluates, what it needs from a handle and what it costs.  THE place a set is defined.  Host-only and
// free of HIP: op_plan.h decides on it, op_forward.hip launches by it.
#pragma once

#include "../../include/open_provence_hip.h"
#include "op_policy.h"

namespace ops {

// ---- kernel sets ------------------------------------------------------------------------------------------------------
// operand format of one part of a layer
enum Fmt {
  FMT_BF16,  // (hi, lo) bf16 planes, the lo planes the policy's terms ask for
  FMT_F16,   // one fp16 plane
  FMT_F8,    // fp16 pieces + e4m3 pieces (x 2^12) of their lo part
  FMT_F32    // fp32 planes on the fp32-input MFMA (kernel set "fp32": the whole layer, opk_f32.hip.h)
};

// what a set needs from the handle (set_available)
enum Need {
  NEED_FAST = 1,       // the row or the panel path
  NEED_PANEL = 2,      // the panel path
  NEED_F8_PACKS = 4,   // the fp16 + e4m3 weight packs
  NEED_H16_PACKS = 8,  // the fp16 single-plane weight packs
  NEED_F16_FIT = 16,   // no weight tensor on fp16's subnormal grid
  NEED_F32_PACKS = 64, // the row-major fp32 weight packs (OP_FLAG_F32_PACKS)
  NEED_ROW_LAYER = 32  // on the row path: none of OP_FLAG_NO_LAYER_FUSION / LAYER_8X16 / LAYER_M32 (the set is a whole-layer kernel there)
};

struct KernelSet {
  int pi;        // the opl::kPolicies index its kernels are instantiated for
  Fmt side;      // attention side: q / k / v projection, attention output o, attention output projection
  Fmt attn;      // q, k, v^T and the attention kernels (FMT_F8: never)
  Fmt wi;        // Wi GEMM and its LayerNorm
  Fmt mlp;       // h and the MLP output projection (row path: the whole-layer kernel runs in `side`)
  bool wlo;      // FMT_F8 GEMMs: the weights' lo part rides as a further e4m3 plane
  opl::Policy terms;  // the evaluated term masks the set reports (op_effective_policy)
  unsigned needs;     // Need bits
  float cost_row, cost_panel;  // MFMA pipe time per algorithmic product in 16-bit units: op_calibrate tries
                               // cheaper sets first (sets 4 and 5 measured in that order on base: 5.15 k vs 4.80 k pairs/s)
};

constexpr unsigned NEED_F8_SET = NEED_F8_PACKS | NEED_F16_FIT;
constexpr KernelSet kKernelSets[OP_KS_COUNT] = {
    // kernels              side      attn      wi        mlp       wlo    terms               needs                                       cost
    {opl::PI_ALL_TERMS, FMT_BF16, FMT_BF16, FMT_BF16, FMT_BF16, false, {3, 3, 3, 3, 3, 3}, 0, 3.0f, 3.0f},                                 //  0 bf16x3
    {opl::PI_BF16_WEIGHTS, FMT_BF16, FMT_BF16, FMT_BF16, FMT_BF16, false, {1, 3, 3, 1, 1, 1}, NEED_FAST, 2.0f, 2.0f},                      //  1 bf16-weights
    {opl::PI_BF16, FMT_BF16, FMT_BF16, FMT_BF16, FMT_BF16, false, {0, 0, 0, 0, 0, 0}, NEED_FAST, 1.01f, 1.01f},                            //  2 bf16 ("f16"'s MFMA count, 8 instead of 11 significant bits: tried second)
    {opl::PI_F16_F8, FMT_F8, FMT_BF16, FMT_F8, FMT_F8, false, {1, 3, 3, 1, 1, 1}, NEED_FAST | NEED_F8_SET | NEED_ROW_LAYER, 1.5f, 1.5f},   //  3 f16-f8
    {opl::PI_F16_F8_W, FMT_F8, FMT_BF16, FMT_F8, FMT_F8, true, {3, 3, 3, 3, 3, 3}, NEED_FAST | NEED_F8_SET | NEED_ROW_LAYER, 1.99f, 2.1f}, //  4 f16-f8-w
    {opl::PI_ALL_TERMS, FMT_BF16, FMT_BF16, FMT_F8, FMT_BF16, true, {3, 3, 3, 3, 3, 3}, NEED_PANEL | NEED_F8_SET, 2.5f, 2.5f},             //  5 bf16x3+wi-f16-f8-w
    {opl::PI_BF16_WEIGHTS, FMT_BF16, FMT_BF16, FMT_F8, FMT_BF16, false, {1, 3, 3, 1, 1, 1}, NEED_PANEL | NEED_F8_SET, 1.75f, 1.75f},       //  6 bf16-weights+wi-f16-f8
    {opl::PI_F16, FMT_F16, FMT_F16, FMT_F16, FMT_F16, false, {0, 0, 0, 0, 0, 0}, NEED_H16_PACKS | NEED_F16_FIT | NEED_ROW_LAYER, 1.0f, 1.0f},  //  7 f16
    {opl::PI_F16, FMT_F16, FMT_F16, FMT_F8, FMT_F8, true, {0, 0, 0, 0, 0, 0}, NEED_PANEL | NEED_H16_PACKS | NEED_F8_SET, 1.74f, 1.74f},    //  8 f16+mlp-f16-f8-w
    {opl::PI_F16, FMT_F16, FMT_F16, FMT_F8, FMT_F8, false, {0, 0, 0, 0, 0, 0}, NEED_PANEL | NEED_H16_PACKS | NEED_F8_SET, 1.375f, 1.375f}, //  9 f16+mlp-f16-f8
    {opl::PI_F16_F8_W, FMT_F8, FMT_F16, FMT_F8, FMT_F8, true, {3, 0, 0, 3, 3, 3}, NEED_PANEL | NEED_F8_SET, 1.9f, 1.9f},                   // 10 f16-f8-w+attn-f16
    {opl::PI_F16_F8, FMT_F8, FMT_F16, FMT_F8, FMT_F8, false, {1, 0, 0, 1, 1, 1}, NEED_PANEL | NEED_F8_SET, 1.45f, 1.45f},                  // 11 f16-f8+attn-f16
    // fp32 operands, 1/16 of the 16-bit MFMA rate: never cheaper than anything (op_calibrate: a reference, an escalation target)
    {opl::PI_ALL_TERMS, FMT_F32, FMT_F32, FMT_F32, FMT_F32, false, {3, 3, 3, 3, 3, 3}, NEED_F32_PACKS, 16.0f, 16.0f},                      // 12 fp32
};
// set number -1: any other term policy, on the all-terms kernels with the lo operands it does not carry cleared
constexpr KernelSet kClearedOperands = {opl::PI_ALL_TERMS, FMT_BF16, FMT_BF16, FMT_BF16, FMT_BF16, false, {3, 3, 3, 3, 3, 3}, 0, 3.0f, 3.0f};

// sets 8 / 9: the "f16" set with the MLP of the layers of a mask in the fp16 + e4m3 format (op_handle::mlp_layers)
constexpr bool mlp_by_layer(const KernelSet& k) { return k.side == FMT_F16 && k.mlp == FMT_F8; }

}  // namespace ops
