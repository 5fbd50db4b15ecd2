// op_sets.h -- the host-only table of the GEMM weight packs (op_api.hip allocates them, op_weights.hip builds them, the
// forward's units read them):
// kWeights / kPackElems / pack_exists, the packed forms of the four GEMM weights of a layer:
// Weight x PackFmt.  Its rows name the kernels' pack modes, so it includes the kernel headers; the kernel sets
// (op_kernel_sets.h) do not.
#pragma once

#include "../../include/open_provence_hip.h"
#include "op_internal.h"
#include "op_kernel_sets.h"

namespace ops {

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
