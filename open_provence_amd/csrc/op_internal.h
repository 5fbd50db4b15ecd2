// op_internal.h -- host-side declarations shared by the units of the C ABI (op_handle.h) and the kernel-launch translation units
// (op_launch_*.hip).  The library is built from several translation units so that the large kernel templates
// compile in parallel; each launch unit instantiates one kernel family for every curated precision policy.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/open_provence_hip.h"
#include "op_policy.h"
#include "opk_attn.hip.h"
#include "opk_attn_probs.hip.h"
#include "opk_common.hip.h"
#include "opk_f32.hip.h"
#include "opk_f32_masked.hip.h"
#include "opk_layer32.hip.h"
#include "opk_layer16p.hip.h"
#include "opk_panel.hip.h"
#include "opk_rowgemm.hip.h"

namespace opl {

// template arguments each kernel family derives from a policy
constexpr int qkv_olo(const Policy& p) { return (p.qk & 1) | (p.qk & 2) | ((p.pv & 2) ? 4 : 0); }  // q_lo, k_lo, v_lo
constexpr int h_olo(const Policy& p) { return p.mlp_out & 1; }
constexpr bool o_lo(const Policy& p) { return (p.attn_out & 1) != 0; }

// Launchers.  `pi` indexes kPolicies.  Each returns false when the shape has no instantiation.
bool launch_row_qkv0(hipStream_t st, const opk::RowGemmParams& p, int ks, bool small, int pi, unsigned grid);
bool launch_row_geglu_fused(hipStream_t st, const opk::RowGemmParams& p, int ks, bool small, int pi, unsigned grid);
bool launch_row_qkv_fused(hipStream_t st, const opk::RowGemmParams& p, int ks, bool small, int pi, unsigned grid);
bool launch_kstream(hipStream_t st, const opk::KStreamParams& p, int nf, int pi, unsigned grid);
// one kernel per layer: x += o Wo^T; x += GeGLU(LN(x) Wi^T) Wo^T; (with_qkv) next layer's q / k / v^T.  128-row blocks.
// hout (the last layer with the head fused, p.fin_ln set): also store entry N of a hidden-state request (RowGemmParams::hid_out).
bool has_row_layer_fused(int pi);
bool launch_row_layer_fused(hipStream_t st, const opk::RowGemmParams& p, int ks, int pi, bool with_qkv, unsigned grid,
                            bool waves8, bool hout = false);
// ... of the "f16 + fp8" kernel set (hidden 128 / 256)
bool launch_row_layer_f8(hipStream_t st, const opk::RowGemmParams& p, int ks, bool with_qkv, unsigned grid, bool hout);
bool launch_row_layer_f8w(hipStream_t st, const opk::RowGemmParams& p, int ks, bool with_qkv, unsigned grid, bool hout);  // kernel set 4
// ... of the "f16" kernel set (PI_F16): the layer-0 q / k / v projection and the whole-layer kernel with fp16 operands
bool launch_row_qkv0_h16(hipStream_t st, const opk::RowGemmParams& p, int ks, bool small, unsigned grid);
bool launch_row_layer_h16(hipStream_t st, const opk::RowGemmParams& p, int ks, bool with_qkv, unsigned grid, bool waves8, bool hout);
// the same launch on the 32x32x16 shape (hidden = 256; kernel sets 1 and 2)
bool has_layer32(int pi);
bool launch_layer32(hipStream_t st, const opk::Layer32Params& p, int pi, bool with_qkv, unsigned grid);
bool launch_layer16p(hipStream_t st, const opk::Layer32Params& p, bool h16, bool with_qkv, bool xin_t, bool xout_t, unsigned grid,
                     bool hout = false);
// waves x kt: (8, 2) and (4, 2) full attention / long and short sequences, (4, 1) sliding window.
// zero_p_lo (pi == 0 only): the policy has no lo(p) x hi(v) term.
// f16_in_f8_out (kernel sets 10 / 11; pi = PI_F16_F8 / PI_F16_F8_W): the fp16 single-pass kernels of PI_F16 on fp16 q / k / v^T,
// o written as fp16 + e4m3 pieces for the attention output projection of the fp16 + e4m3 format.
bool launch_attn(hipStream_t st, const opk::AttnFpParams& p, int waves, int kt, int pi, bool zero_p_lo, dim3 grid,
                 bool f16_in_f8_out = false);
// launch_attn's arguments on the key-mask form of the same kernels (p.key_row, p.vmean; op_launch_attn_masked.hip)
bool launch_attn_masked(hipStream_t st, const opk::AttnFpParams& p, int waves, int kt, int pi, bool zero_p_lo, dim3 grid,
                        bool f16_in_f8_out = false);
bool launch_panel(hipStream_t st, const opk::PanelParams& p, int epi, int pi, dim3 grid);
// q, k and v^T panels of one layer in one launch (p.n_tiles = 3 H / 256, p.n_qk_tiles = 2 H / 256, p.o2 = v^T)
bool launch_panel_qkv(hipStream_t st, const opk::PanelParams& p, int pi, dim3 grid);
// the panel GEMMs in the fp16 + e4m3 format (kernel sets 3 / 4; wlo: the weights carry their lo part = set 4)
bool launch_panel_f8(hipStream_t st, const opk::PanelParams& p, int epi, bool wlo, dim3 grid);
// o16 (kernel sets 10 / 11): q, k, v^T as single-plane fp16 for launch_attn(.., f16_in_f8_out = true)
bool launch_panel_f8_qkv(hipStream_t st, const opk::PanelParams& p, bool wlo, bool o16, dim3 grid);

// Kernel set "fp32" (opk_f32.hip.h; op_launch_f32.hip): fp32 planes, fp32 weights as loaded, fp32-input MFMAs.
// epi: opk::F32Epilogue; false when there is no such epilogue.
void launch_f32_ln(hipStream_t st, const float* x, const float* w, float eps, int H, int r_pad, float* out);
bool launch_f32_gemm(hipStream_t st, const opk::F32GemmParams& p, int epi);
// grid: (64-query blocks of the longest sequence, heads, sequences)
void launch_f32_attn(hipStream_t st, const opk::F32AttnParams& p, dim3 grid);
// rank_head_kernel's arguments (one block per sequence), exact erff
void launch_f32_rank_head(hipStream_t st, int n_seqs, const float* cls, const float* y, const int32_t* cu, int s0, const int32_t* roff,
                          int mean_pool, int H, int nl, const float* dense_t, const float* head_norm, float eps, const float* cls_w,
                          const float* cls_b, float* rank_out);

// op_forward_masked (opk_f32_masked.hip.h; op_launch_f32_masked.hip) beside the launches above.
// cu[n_rows + 1] = r * width, and *status (preset to opk::MASKED_ST_NONE) = the linear index of the first id outside [0, vocab)
void launch_masked_prepare(hipStream_t st, const int32_t* ids, int n_rows, int width, int vocab, int32_t* cu, uint32_t* status);
// vmean[n_seqs][H]: the mean of v over each sequence's positions (the n_seqs sequences from s0 on)
void launch_f32_vmean(hipStream_t st, const float* v, const int32_t* cu, int s0, const int32_t* roff, int H, int n_seqs, float* vmean);
// launch_f32_attn's grid
void launch_f32_attn_masked(hipStream_t st, const opk::F32MaskedAttnParams& p, dim3 grid);
// launch_f32_rank_head's arguments and key_ok[total_tokens]
void launch_f32_rank_head_masked(hipStream_t st, int n_seqs, const float* cls, const float* y, const int32_t* cu, int s0,
                                 const int32_t* roff, const uint8_t* key_ok, int mean_pool, int H, int nl, const float* dense_t,
                                 const float* head_norm, float eps, const float* cls_w, const float* cls_b, float* rank_out);
// prune[t][0 .. 1] = +0.0 where key_ok[t] == 0, t in [t0, t0 + n_tokens)
void launch_prune_mask(hipStream_t st, float* prune, const uint8_t* key_ok, size_t t0, size_t n_tokens);

// op_attention_probs (opk_attn_probs.hip.h; op_launch_attn_probs.hip) beside launch_f32_ln and launch_f32_gemm(F32_EPI_QKV).
// packed [total_tokens][H] fp32 -> the row layout [r_pad][H] through row_tok (zero rows where row_tok < 0)
void launch_attn_probs_gather(hipStream_t st, const float* packed, const int32_t* row_tok, int H, int r_pad, float* x);
// grid: (64-query blocks of p.width, heads, the n_seqs sequences from p.s0 on); every element of their matrices is written
void launch_attn_probs(hipStream_t st, const opk::AttnProbsParams& p, int n_seqs);
// op_attention_rows: one query row of the n_seqs sequences from p.s0 on, per head (grid: heads x sequences) or as the mean over
// heads (grid: sequences; p.num_heads <= opk::AR_MAX_HEADS); every element of their rows is written
void launch_attn_rows(hipStream_t st, const opk::AttnRowsParams& p, int n_seqs, bool head_mean);

// op_debug_primitive (opk_probe.hip.h; op_launch_probe.hip).  probe_group_size: the number of input elements one record of
// `kind` (enum op_probe_kind) takes, 0 for an unknown kind.  launch_probe: kind, mode and n % group already checked, n > 0.
int probe_group_size(int kind);
void launch_probe(hipStream_t st, int kind, int mode, const void* in, size_t n, void* out);

// The padded [B, L] boundary (opk_padded.hip.h; op_pack_padded / op_unpack_padded).  Integer types as enum op_int_dtype.
constexpr int PAD_INT_I32 = 0, PAD_INT_I64 = 1, PAD_INT_U8 = 2;
// row lengths + validation, scan and gather of one padded batch: cu[n_rows + 1], ids_packed[<= n_rows * width] and the
// status block (opk::PAD_ST_*; the caller presets its two atomicMin words to opk::PAD_ST_NONE).  mask == nullptr: full rows.
bool launch_padded_pack(hipStream_t st, const void* ids, int ids_dtype, const void* mask, int mask_dtype, int n_rows, int width,
                        int vocab, int32_t* ids_packed, int32_t* cu, uint32_t* status);
// packed [T][channels] fp32 -> padded [n_rows][width][channels], every element written; channels 1 or 2
bool launch_padded_scatter(hipStream_t st, const float* packed, const int32_t* cu, int n_rows, int width, int channels, float* padded);

// The running audit of a calibrated kernel set (opk_audit.hip.h; op_coverage_scan / op_coverage_commit / op_gather_rows /
// op_audit_compare).  The handle's coverage state block, uint32 words (= opk::COV_ST_*): the longest audited row, then what one
// scan leaves -- the sum of the rows' novel positions and a uint64 (length << 32 | ~row) of the first longest row.
constexpr int COV_MAXLEN = 0, COV_NOVEL = 1, COV_LONGEST = 2, COV_WORDS = 4;
// row_novel[n_seqs]; the caller clears state[COV_NOVEL .. COV_WORDS) first
void launch_coverage_scan(hipStream_t st, const int32_t* ids, const int32_t* cu, int n_seqs, int total, int vocab, const uint32_t* bits,
                          int32_t* row_novel, uint32_t* state);
// commit, gather and compare: a listed row outside [0, n_seqs) is skipped (compare: counts as +inf), row bounds are held inside
// [0, total)
void launch_coverage_commit(hipStream_t st, const int32_t* ids, const int32_t* cu, int n_seqs, int total, const int32_t* rows, int n_rows,
                            int vocab, uint32_t* bits, uint32_t* state);
// the listed rows end to end in sub_ids, their prefix offsets in sub_cu[n_rows + 1]
void launch_gather_rows(hipStream_t st, const int32_t* ids, const int32_t* cu, int n_seqs, int total, const int32_t* rows, int n_rows,
                        int32_t* sub_ids, int32_t* sub_cu);
// err[0] (cleared by the caller) = max |difference|, +inf when a value is not finite
void launch_audit_compare(hipStream_t st, const float* prune, const float* rank, const int32_t* cu, int n_seqs, int total,
                          const int32_t* rows, int n_rows, const float* sub_prune, const float* sub_rank, const int32_t* sub_cu,
                          int n_labels, float* err);

// op_assemble_rows (opk_assemble.hip.h; op_launch_assemble.hip): pieces = {prefix, middle, suffix} on the host, each of
// n_pieces[i] <= ASSEMBLE_PIECE_MAX ids (checked by the caller); plan [n_rows][4] = {query, first_frag, n_frag, clip}; n_rows > 0.
constexpr int ASSEMBLE_PIECE_MAX = 8;
void launch_assemble_rows(hipStream_t st, const int32_t* corpus, const int32_t* frag_off, int n_frag, int n_corpus, const int32_t* query_ids,
                          const int32_t* q_off, int n_queries, int n_query_tokens, const int32_t* const pieces[3], const int n_pieces[3],
                          const int32_t* plan, const int32_t* cu, int n_rows, int total, int32_t* out);

// op_planned_fragment_means / op_sentence_decisions (opk_decide.hip.h; op_launch_decide.hip): the requests as the caller gave
// them, checked (opp::check_planned_means / opp::check_decisions); n_rows > 0 resp. n_instances > 0.
void launch_planned_fragment_means(hipStream_t st, const op_assemble_request& rows, const op_planned_means_request& req);
// op_located_fragment_means: the same requests (opp::check_located_means), the rows' ids [total_tokens] and ctx_start_out [n_rows]
void launch_located_fragment_means(hipStream_t st, const op_assemble_request& rows, const op_planned_means_request& req, const int32_t* ids,
                                   int32_t* ctx_start_out);
void launch_sentence_decisions(hipStream_t st, const op_decisions_request& req);

}  // namespace opl
