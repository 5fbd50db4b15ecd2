// op_forward.h -- the forward's workspace and its launch sequence, ChunkPass, declared for its two units: op_forward.hip
// (constructor, prologue, hidden-state stores, attention, heads, run) and op_forward_layers.hip (one layer of each path).
#pragma once

#include "op_handle.h"

namespace oph {

// kernel set "fp32" only: its fp32 planes (carved behind the regions every set has; nullptr under every other set)
struct WorkspaceF32 {
  float *ln, *q, *k, *v, *o, *h;
};

struct Workspace {
  float* x;
  u16 *ln_hi, *ln_lo;
  u16 *q_hi, *q_lo, *k_hi, *k_lo;
  u16 *vt_hi, *vt_lo;
  u16 *o_hi, *o_lo;
  u16 *h_hi, *h_lo;
  int32_t *row_seq, *row_pos, *row_tok, *roff, *qboff, *qboff_l;
  float* cls;
  int* range_flag;  // panel path, fp16 + e4m3 format: "an fp16 operand was out of range" (PanelParams::range_flag)
  WorkspaceF32 f;  // reported as regions ln_f .. h_f
  size_t bytes;
};

// Clear the lo plane of a fragment-packed tensor: a policy without that operand's lo term, evaluated on the
// all-terms kernel set (the extra MFMA pass then adds exact zeros).  (op_forward.hip)
int clear_lo(Launcher& L, u16* base, int unit, size_t n_pairs);

// One chunk of sequences through the whole encoder: the launch sequence of a forward.  The arguments and what every path
// derives from them are members; prologue() (row map, padding rows, embeddings), one *_layer() per path and layer, heads().
struct ChunkPass {
  op_handle* h;
  Launcher& L;
  const Workspace& ws;
  const PackedBatch& b;  // the whole batch: ids, cu_seqlens, outputs
  int s0, ns, rows, max_len;  // this chunk: sequences [s0, s0 + ns), its rows and its longest sequence
  const AttnPlan& plan;
  const HiddenReq* hid;  // per-call hidden-state request, or nullptr
  const MaskedReq* msk;  // op_forward_masked: kernel set "fp32" with the key mask's attention and heads (native: the selected set with them), or nullptr

  int H, I;
  bool fp_layout;  // fragment-packed activations, attn_fp_kernel
  int r_pad, m_tiles;
  unsigned row_blocks;
  hipStream_t st;
  Policy E, V;  // evaluated policy, instantiated kernel set (V has every term of E)
  int pi;       // ... its opl::kPolicies index
  bool clr_q, clr_k, clr_v, clr_o, clr_h, clr_ln_attn, clr_ln_mlp, zero_p_lo, split;
  // the operand formats of the handle's kernel set (h->ks, op_kernel_sets.h), decided once here
  bool o_f8, f16, f32, attn16, wi8, wlo8, range_flagged, embed_in_qkv0;
  bool mlp8[OP_MAX_LAYERS];  // sets 8 / 9, per layer: the MLP in the fp16 + e4m3 format
  PackFmt fmt_base, fmt_f8, fmt_side, fmt_wi;  // weight packs: layer-0 q / k / v, the fp16 + e4m3 GEMMs, attention side, Wi
  size_t plane_bytes;  // one row-major plane (tiled path)
  int q_tiles;
  bool small_blocks;
  unsigned row_grid;
  const char* no_kernel = "internal: no row-stationary kernel for hidden %d";
  bool layer_fused, head_in_last_layer;
  bool pair_layers;  // whole-layer launches as wave pairs on 32x32x16 MFMAs (opk_layer16p.hip.h)
  bool head_done = false;
  int hidden_stored = -1;  // the hidden-state entry the last layer launch stored itself (wave-pair kernel), -1: none

  ChunkPass(op_handle* h_, Launcher& L_, const Workspace& ws_, const PackedBatch& b_, int s0_, int ns_, int rows_, int max_len_,
            const AttnPlan& plan_, const HiddenReq* hid_, const MaskedReq* msk_ = nullptr);

  // the pack of a GEMM weight of layer `li` in the format the constructor decided
  u16* weight(int li, Weight w, PackFmt f) const { return h->layers[li].pack[w][f]; }

  // ---- op_forward.hip --------------------------------------------------------------------------------------------------
  int prologue();
  int capture(int index);
  // Per-call hidden-state request.  Nothing below depends on it but these stores: the kernels are the ones a forward without a
  // request runs.  Entry `index` is copied from the residual stream rows a launch has just written; ln: through final_norm
  // first (entry N, post-norm convention).  Two launches store their entry from their own epilogue instead: the wave-pair
  // kernel (layer16p_hout_kernel; between two of its launches x is tiled) and the last whole-layer launch with the head fused,
  // which writes no x (rowgemm_hout_kernel).
  // A pooled request (op_forward_packed_pooled) redirects the entries it selects to its scratch entry, packed fp32: the same
  // stores, another destination.  hidden_pooled(index), behind the launch that stored the entry, reduces it to one row per
  // sequence of this chunk and hands it on to the ordinary request's entry if that wants it too.
  void* hidden_entry(int index) const {
    if (!hid) return nullptr;
    if (hid->pooled(index)) return hid->scratch;
    if (!hid->full(index)) return nullptr;
    return hid->out + (size_t)hid->slot[index] * hid->entry_bytes;
  }
  int hidden_bf16(int index) const { return hid->pooled(index) ? 0 : hid->bf16; }
  int hidden_pad(int index) const { return hid->pooled(index) ? 0 : hid->pad; }
  int hidden_pooled(int index);
  int hidden(int index, const float* ln = nullptr);
  int attention(bool is_global);
  int clear_qkv();
  int clear_h();
  int heads();
  int run();

  // ---- op_forward_layers.hip -------------------------------------------------------------------------------------------
  RowGemmParams qkv_params(int li);
  int row_layer(int li);
  int panel_layer(int li);
  int tiled_layer(int li);
  int f32_layer(int li);
};

}  // namespace oph
