// op_sets.h -- the two host-only tables of op_api.hip (no other unit includes this header):
//   kKernelSets   what each OP_KS_* kernel set is: the kernels it runs, the operand format of each part of a layer, the
//                 terms it evaluates, what it needs from a handle and what it costs.  THE place a set is defined.
//   kWeights / kPackElems / pack_exists   the packed forms of the four GEMM weights of a layer: Weight x PackFmt.
#pragma once

#include "../../include/open_provence_hip.h"
#include "op_internal.h"

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

// ---- GEMM weight packs ------------------------------------------------------------------------------------------------
enum Weight { W_QKV, W_ATTN_OUT, W_WI, W_MLP_OUT, W_COUNT };

enum PackFmt {
  PF_HI,        // tiled path: row-major bf16 hi plane ...
  PF_LO,        // ... and lo plane
  PF_PK,        // fragment-ordered (hi, lo) bf16 planes, interleaved per k-step: chunk-major or k-streamed (row path), panel-major
  PF_PK16,      // kernel set "f16": the layout of PF_PK with fp16 values in the hi plane
  PF_ROW_F8A,   // row path, fp16 + e4m3: chunks of [fp16 plane | e4m3 plane] (Wqkv, Wi), k-streamed fp16 slabs (the two Wo)
  PF_ROW_F8B,   // ... the e4m3 K = 128 slabs of the attention Wo
  PF_PANEL16,   // panel path, fp16 + e4m3: fp16 slabs ...
  PF_PANEL8,    // ... and e4m3 slabs (w, then lo(w))
  PF_L32,       // hidden = 256: hi plane in the fragment order of the 32x32x16 whole-layer kernel (opk_layer32.hip.h)
  PF_PAIR,      // hidden = 256: one plane in the order of the wave-pair whole-layer kernel (opk_layer16p.hip.h), bf16 values
  PF_PAIR16,    // ... fp16 values
  PF_F32,       // kernel set "fp32" (OP_FLAG_F32_PACKS): the tensor as loaded, row-major fp32 (two u16 per element)
  PF_COUNT
};

// epilogue numbers of the panel launchers (op_launch_panel.hip) beyond opk::PanelEpi
constexpr int PANEL_EPI_ATTN_OUT = 100, PANEL_EPI_MLP_OUT = 101, PANEL_EPI_QKV = 102, PANEL_EPI_GEGLU_BF16_H = 103;
// WeightDesc::row_mode beyond opk::RowEpilogue: pack_kstream_kernel (k-streamed, output features permuted)
constexpr int ROW_PACK_KSTREAM = 100;

struct PanelSeg {
  int epi, th, ti;  // (th * H + ti * I) / 256 panels of 256 output features, rows permuted for opk::PanelEpi `epi`
};
struct WeightDesc {
  const char* tail;      // tensor name after "model.layers.<i>."
  int rh, ri, ch, ci;    // shape [rh * H + ri * I, ch * H + ci * I]
  int family;            // op_gemm_family
  int row_mode;          // row path: pack_rowgemm_kernel's mode, or ROW_PACK_KSTREAM
  int l32_mode, kmajor;  // pack_layer32_kernel / pack_layer16p_kernel (opk::Layer32Pack; Layer16pPack has the same numbers)
  bool geglu;            // rows are the (input, gate) halves of I (split_planes_kernel)
  PanelSeg panel[2];     // panel path: the tensor's panels in order (th = ti = 0: no second segment)
};
constexpr WeightDesc kWeights[W_COUNT] = {
    {"attn.Wqkv.weight", 3, 0, 1, 0, OP_FAM_WQKV, opk::RE_QKV, opk::L32_QKV, 0, false, {{opk::PE_QK, 2, 0}, {opk::PE_V, 1, 0}}},
    {"attn.Wo.weight", 1, 0, 1, 0, OP_FAM_ATTN_OUT, ROW_PACK_KSTREAM, opk::L32_RESID, 1, false, {{opk::PE_RESIDUAL, 1, 0}, {0, 0, 0}}},
    {"mlp.Wi.weight", 0, 2, 1, 0, OP_FAM_WI, opk::RE_GEGLU, opk::L32_GEGLU, 0, true, {{opk::PE_GEGLU, 0, 2}, {0, 0, 0}}},
    {"mlp.Wo.weight", 1, 0, 0, 1, OP_FAM_MLP_OUT, ROW_PACK_KSTREAM, opk::L32_RESID, 1, false, {{opk::PE_RESIDUAL, 1, 0}, {0, 0, 0}}},
};

constexpr size_t weight_rows(Weight w, int H, int I) { return (size_t)kWeights[w].rh * H + (size_t)kWeights[w].ri * I; }
constexpr size_t weight_cols(Weight w, int H, int I) { return (size_t)kWeights[w].ch * H + (size_t)kWeights[w].ci * I; }
constexpr size_t weight_elems(Weight w, int H, int I) { return weight_rows(w, H, I) * weight_cols(w, H, I); }

// u16 elements allocated per weight element; 0: no such pack
constexpr int kPackElems[W_COUNT][PF_COUNT] = {
    // HI LO PK PK16 ROW_F8A ROW_F8B PANEL16 PANEL8 L32 PAIR PAIR16 F32
    {1, 1, 2, 2, 2, 0, 1, 1, 1, 1, 1, 2},  // W_QKV       [fp16 | e4m3 + e4m3(lo)] chunks
    {1, 1, 2, 2, 1, 1, 1, 1, 1, 1, 1, 2},  // W_ATTN_OUT  fp16 slabs + e4m3 slabs
    {1, 1, 2, 2, 2, 0, 1, 1, 1, 1, 1, 2},  // W_WI
    {1, 1, 2, 2, 2, 0, 1, 1, 1, 1, 1, 2},  // W_MLP_OUT   fp16 slabs of w and of lo(w): no e4m3 plane
};

// does the handle build packs of this format? (tiled = neither fast path; f8 / h16 / f32: op_handle::f8_packs / h16_packs / f32_packs)
constexpr bool pack_exists(PackFmt f, bool row, bool panel, bool f8, bool h16, bool f32, int H) {
  switch (f) {
    case PF_HI:
    case PF_LO: return !row && !panel;
    case PF_PK: return row || panel;
    case PF_PK16: return (row || panel) && h16;
    case PF_ROW_F8A:
    case PF_ROW_F8B: return row && f8;
    case PF_PANEL16:
    case PF_PANEL8: return panel && f8;
    case PF_L32:
    case PF_PAIR: return row && H == 256;
    case PF_PAIR16: return row && H == 256 && h16;
    case PF_F32: return f32;
    default: return false;
  }
}

// op_create allocates per layer in this order (the parent's, so that the device footprint does not move): for each step,
// for each weight, the step's formats
struct AllocStep {
  PackFmt fmt[2];
  int n_fmt;
  Weight order[W_COUNT];
};
constexpr AllocStep kAllocOrder[] = {
    {{PF_HI, PF_LO}, 2, {W_QKV, W_ATTN_OUT, W_WI, W_MLP_OUT}},
    {{PF_PK}, 1, {W_QKV, W_WI, W_MLP_OUT, W_ATTN_OUT}},
    {{PF_PK16}, 1, {W_QKV, W_WI, W_MLP_OUT, W_ATTN_OUT}},
    {{PF_PANEL16, PF_PANEL8}, 2, {W_QKV, W_ATTN_OUT, W_WI, W_MLP_OUT}},
    {{PF_ROW_F8A, PF_ROW_F8B}, 2, {W_QKV, W_WI, W_ATTN_OUT, W_MLP_OUT}},
    {{PF_L32}, 1, {W_ATTN_OUT, W_WI, W_MLP_OUT, W_QKV}},
    {{PF_PAIR}, 1, {W_ATTN_OUT, W_WI, W_MLP_OUT, W_QKV}},
    {{PF_PAIR16}, 1, {W_ATTN_OUT, W_WI, W_MLP_OUT, W_QKV}},
    {{PF_F32}, 1, {W_QKV, W_ATTN_OUT, W_WI, W_MLP_OUT}},
};

}  // namespace ops
