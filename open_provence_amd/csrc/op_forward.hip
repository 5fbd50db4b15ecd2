// op_forward.hip -- C ABI: op_forward_packed / _hidden / _pooled.  Workspace carving, chunking of the packed batch, and the
// launch sequence of one chunk around its layers (ChunkPass: prologue, hidden-state stores, attention, heads; the layers
// themselves: op_forward_layers.hip).  The one unit that compiles the forward's non-GEMM kernels (opk_small / opk_masked / opk_pool .hip.h)
// and the tiled path's attention (attn_kernel of opk_tiled.hip.h, whose GEMM op_forward_layers.hip instantiates).
#include "op_forward.h"
#include "opk_small.hip.h"
#include "opk_masked.hip.h"
#include "opk_pool.hip.h"
#include "opk_tiled.hip.h"

namespace oph {

// the rows a workspace of this geometry is carved for (op_workspace_bytes, op_forward_packed and the attention side passes)
int chunk_row_capacity(const op_handle* h, int n_seqs, int total_tokens, int max_seqlen) {
  return opp::chunk_row_capacity(h->chunk_rows, n_seqs, total_tokens, max_seqlen);
}

// the regions of a forward's workspace for a batch of this geometry; f32: with the planes of kernel set "fp32"
opp::Layout forward_layout(const op_handle* h, int n_seqs, int total_tokens, int max_seqlen, bool f32) {
  return opp::workspace_layout(h->H, h->I, opp::padded_row_capacity(h->chunk_rows, n_seqs, total_tokens, max_seqlen), n_seqs, f32);
}

// The workspace's pointers from its layout, region by region: generated from the same list as the layout (op_plan.h).
static void carve(const opp::Layout& lay, char* base, Workspace& ws) {
  int i = 0;
#define WS_TAKE(member, kind, bytes) ws.member = reinterpret_cast<decltype(ws.member)>(base + lay.regions[i++].offset);
  OPP_WORKSPACE_REGIONS(WS_TAKE)
#undef WS_TAKE
  ws.f = WorkspaceF32{};
  if (i < lay.n) {  // the planes of kernel set "fp32"
#define WS_TAKE_F32(member, bytes) ws.f.member = reinterpret_cast<float*>(base + lay.regions[i++].offset);
    OPP_WORKSPACE_F32_PLANES(WS_TAKE_F32)
#undef WS_TAKE_F32
  }
  ws.bytes = lay.bytes;
}

// Clear the lo plane of a fragment-packed tensor: a policy without that operand's lo term, evaluated on the
// all-terms kernel set (the extra MFMA pass then adds exact zeros).
int clear_lo(Launcher& L, u16* base, int unit, size_t n_pairs) {
  OP_TRY(L.begin(PK_CLEAR_LO));
  const size_t n = n_pairs * (size_t)(unit / 8);
  hipLaunchKernelGGL(zero_odd_units_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, L.stream, base, unit, n_pairs);
  return L.end();
}

void launch_side_row_map(hipStream_t stream, const int32_t* cu_dev, int s0, int ns, int r_pad, int32_t* roff, int32_t* row_seq,
                         int32_t* row_pos, int32_t* row_tok) {
  hipLaunchKernelGGL(seq_offsets_kernel, dim3(1), dim3(1024), 0, stream, cu_dev, s0, ns, ROW_ALIGN, ROW_ALIGN, roff);
  hipLaunchKernelGGL(row_map_kernel, dim3((unsigned)((r_pad + 255) / 256)), dim3(256), 0, stream, cu_dev, s0, ns, roff, r_pad,
                     row_seq, row_pos, row_tok);
}

ChunkPass::ChunkPass(op_handle* h_, Launcher& L_, const Workspace& ws_, const PackedBatch& b_, int s0_, int ns_, int rows_, int max_len_,
                     const AttnPlan& plan_, const HiddenReq* hid_, const MaskedReq* msk_)
    : h(h_), L(L_), ws(ws_), b(b_), s0(s0_), ns(ns_), rows(rows_), max_len(max_len_), plan(plan_), hid(hid_), msk(msk_) {
  H = h->H;
  I = h->I;
  // Row path: exactly the computed rows, rounded to the 128-row block -- no slack rows: a 131072-row batch is 1024
  // blocks = two full rounds of 2 blocks per CU; two extra (empty) blocks would cost a third round.  The tiled path
  // keeps 64 slack rows for its attention kernel's tile over-read.
  fp_layout = h->row_path || h->panel_path;
  r_pad = fp_layout ? align_up(rows, ROW_BM) : align_up(rows + 64, 256);
  m_tiles = r_pad / GEMM_BM;
  row_blocks = (unsigned)((r_pad + 3) / 4);
  st = L.stream;
  // Evaluated policy E, instantiated kernel set V (V has every term of E).  Where V multiplies by a lo operand that
  // E does not have, that operand is cleared: weights at load time (op_load_weight), activations in the launch sequence.
  // (a masked forward: set "fp32" on any handle with its packs -- unless it asks for the handle's own set, MaskedReq::native)
  const bool msk_f32 = msk && !msk->native;
  const KernelSet& ks = msk_f32 ? kKernelSets[OP_KS_F32] : *h->ks;
  E = msk_f32 ? ks.terms : h->eff;
  pi = ks.pi;
  V = opl::kPolicies[pi];
  o_f8 = ks.side == FMT_F8;   // o = fp16 pieces (ws.o_hi) + e4m3 pieces (ws.o_lo); panel path: every GEMM in that format
  f16 = ks.side == FMT_F16;   // kernel set "f16": set 2's layouts, fp16 values, the fp16 weight packs
  f32 = ks.side == FMT_F32;   // kernel set "fp32": fp32 planes and weights, its own layer (f32_layer) on every path
  // kernel sets 10 / 11 (panel path): q / k / v^T as single-plane fp16, attention on set 7's kernels with o in sets 3 / 4's
  // format; they neither write nor read a lo plane of q / k / v^T
  attn16 = o_f8 && ks.attn == FMT_F16;
  auto extra = [](int v, int e, int bit) { return (v & bit) != 0 && (e & bit) == 0; };
  clr_q = !attn16 && extra(V.qk, E.qk, 1);
  clr_k = !attn16 && extra(V.qk, E.qk, 2);
  clr_v = !attn16 && extra(V.pv, E.pv, 2);
  clr_o = extra(V.attn_out, E.attn_out, 1);
  clr_h = extra(V.mlp_out, E.mlp_out, 1);
  clr_ln_attn = extra(V.wqkv, E.wqkv, 1);
  clr_ln_mlp = extra(V.wi, E.wi, 1);
  zero_p_lo = !attn16 && extra(V.pv, E.pv, 1);
  // tiled path: two kernel sets only (single pass / all terms)
  split = (E.wqkv | E.qk | E.pv | E.attn_out | E.wi | E.mlp_out) != 0;
  // OP_FLAG_PANEL_F8_WI (sets 5 / 6): the format in the Wi GEMM alone -- its LayerNorm writes fp16 + e4m3 pieces, its epilogue
  // writes h as the (hi, lo) bf16 pieces the MLP output projection's kernel reads
  wi8 = !o_f8 && ks.wi == FMT_F8 && ks.mlp != FMT_F8;
  wlo8 = ks.wlo;
  // kernel sets 8 / 9: the attention side on the "f16" kernels, the MLP -- LayerNorm(mlp_norm), Wi + GeGLU with h as fp16 +
  // e4m3 pieces, MLP output projection -- on the fp16 + e4m3 kernels of sets 4 / 3, layer by layer: op_calibrate keeps it
  // only in the layers the tolerance needs it in (mlp_layers)
  for (int li = 0; li < h->N; ++li) mlp8[li] = mlp_by_layer(ks) && (li >= 64 || ((h->mlp_layers >> li) & 1ull) != 0);
  // Panel path, fp16 + e4m3 kernels (sets 3 / 4 / 8 - 11): they convert under MODE.FP16_OVFL = 1 (an h beyond fp16's range is
  // clamped) and their fp16 MFMAs take a NaN operand for a finite number, so an out-of-range activation cannot travel to the
  // outputs as Inf / NaN by itself: the kernels raise ws.range_flag and the head kernels write NaN logits.
  range_flagged = h->panel_path && (o_f8 || ks.mlp == FMT_F8);
  fmt_base = f16 ? PF_PK16 : PF_PK;
  fmt_f8 = h->row_path ? PF_ROW_F8A : PF_PANEL16;
  fmt_side = o_f8 ? fmt_f8 : fmt_base;
  fmt_wi = (o_f8 || wi8) ? fmt_f8 : fmt_base;
  // Row path without hidden-state capture: the layer-0 q / k / v kernel gathers and normalises the embeddings itself
  // (RowGemmParams::emb_table) -- no embedding launch, the residual rows are written once and not read back.
  embed_in_qkv0 = h->row_path && !f32 && !h->capture && !(h->cfg.flags & OP_FLAG_NO_HEAD_FUSION);
  plane_bytes = (size_t)r_pad * H * sizeof(u16);
  q_tiles = (max_len + ATT_BQ - 1) / ATT_BQ;
  // 4 waves x 32 rows = 128-row blocks, two per CU.  Small batches (at most one such block per CU) use 4 waves x
  // 16 rows = 64-row blocks instead: twice the blocks, so a latency-bound request spreads over twice the CUs.
  small_blocks = (r_pad / ROW_BM) <= h->n_cus && !(h->cfg.flags & OP_FLAG_NO_SMALL_BLOCKS);
  row_grid = (unsigned)(r_pad / (small_blocks ? 64 : ROW_BM));
  // Kernel sets whose GEMM weights are single-plane run a whole layer (attention output projection, MLP, next q/k/v
  // projection) as ONE kernel with h kept on chip; the all-terms set keeps the two fused kernels per layer.
  layer_fused = h->row_path && !f32 && h->set >= 0 && opl::has_row_layer_fused(pi) && !(h->cfg.flags & OP_FLAG_NO_LAYER_FUSION);
  head_in_last_layer = layer_fused && h->cfg.pooling != OP_POOL_MEAN && !h->capture && !(h->cfg.flags & OP_FLAG_NO_HEAD_FUSION);
  // (!split: the single-pass sets "f16" / "bf16")
  pair_layers = layer_fused && H == 256 && I % 64 == 0 && !split && !h->capture &&
                !(h->cfg.flags & (OP_FLAG_NO_LAYER_PAIRS | OP_FLAG_LAYER_8X16 | OP_FLAG_LAYER_M32)) &&
                weight(0, W_ATTN_OUT, f16 ? PF_PAIR16 : PF_PAIR) != nullptr;
}

// row map, the range flag, padding rows of the attention output, embeddings
int ChunkPass::prologue() {
  OP_TRY(L.begin(PK_ROWMAP));
  hipLaunchKernelGGL(seq_offsets_kernel, dim3(1), dim3(1024), 0, st, b.cu_dev, s0, ns, ROW_ALIGN, ROW_ALIGN, ws.roff);
  if (fp_layout) {
    hipLaunchKernelGGL(seq_offsets_kernel, dim3(1), dim3(1024), 0, st, b.cu_dev, s0, ns, plan.waves_g * 32, 1, ws.qboff);
    hipLaunchKernelGGL(seq_offsets_kernel, dim3(1), dim3(1024), 0, st, b.cu_dev, s0, ns, 128, 1, ws.qboff_l);
  }
  hipLaunchKernelGGL(row_map_kernel, dim3((unsigned)((r_pad + 255) / 256)), dim3(256), 0, st, b.cu_dev, s0, ns, ws.roff,
                     r_pad, ws.row_seq, ws.row_pos, ws.row_tok);
  if (msk && msk->native)  // the mask in this chunk's row layout: what the key-mask form of attn_fp_kernel reads
    hipLaunchKernelGGL(key_row_kernel, dim3((unsigned)((r_pad + 255) / 256)), dim3(256), 0, st, msk->key_ok, ws.row_tok, r_pad, msk->key_row);
  OP_TRY(L.end());

  // rows >= `rows` are never produced by the attention kernel: keep its output finite there
  if (range_flagged) OP_HIP(h, hipMemsetAsync(ws.range_flag, 0, sizeof(int), st));
  if (f32) {  // (the other sets' o planes are not read)
    const size_t tail_bytes = (size_t)(r_pad - rows) * H * sizeof(float);
    if (tail_bytes) OP_HIP(h, hipMemsetAsync(ws.f.o + (size_t)rows * H, 0, tail_bytes, st));
  } else if (fp_layout && o_f8) {
    const size_t n16 = (size_t)((r_pad - rows) / 16);
    if (n16) OP_HIP(h, hipMemsetAsync(ws.o_hi + (size_t)(rows / 16) * (H / 32) * 512, 0, n16 * (H / 32) * 512 * sizeof(u16), st));
    if (n16) OP_HIP(h, hipMemsetAsync(ws.o_lo + (size_t)(rows / 16) * h->nh * 512, 0, n16 * h->nh * 512 * sizeof(u16), st));
  } else if (fp_layout) {  // fragment-packed o: pieces of 16 rows, hi/lo interleaved, o_hi + o_lo are one buffer
    const size_t tail_off = (size_t)(rows / 16) * (H / 32) * 2 * 512;
    const size_t tail_bytes = (size_t)((r_pad - rows) / 16) * (H / 32) * 2 * 512 * sizeof(u16);
    if (tail_bytes) OP_HIP(h, hipMemsetAsync(ws.o_hi + tail_off, 0, tail_bytes, st));  // (a zero-byte node fails stream capture)
  } else {
    const size_t tail_off = (size_t)rows * H;
    const size_t tail_bytes = (size_t)(r_pad - rows) * H * sizeof(u16);
    if (tail_bytes) OP_HIP(h, hipMemsetAsync(ws.o_hi + tail_off, 0, tail_bytes, st));
    if (tail_bytes && split) OP_HIP(h, hipMemsetAsync(ws.o_lo + tail_off, 0, tail_bytes, st));
  }

  if (!embed_in_qkv0) {
    OP_TRY(L.begin(PK_EMBED_LN));
    if (split)
      hipLaunchKernelGGL((embed_ln_kernel<true>), dim3(row_blocks), dim3(256), 0, st, b.ids_dev, ws.row_tok, h->emb,
                         h->emb_norm, h->cfg.norm_eps, H, r_pad, h->V, ws.x, ws.ln_hi, ws.ln_lo);
    else
      hipLaunchKernelGGL((embed_ln_kernel<false>), dim3(row_blocks), dim3(256), 0, st, b.ids_dev, ws.row_tok, h->emb,
                         h->emb_norm, h->cfg.norm_eps, H, r_pad, h->V, ws.x, ws.ln_hi, ws.ln_lo);
    OP_TRY(L.end());
  }
  return OP_OK;
}

int ChunkPass::capture(int index) {
  if (!h->capture || msk) return OP_OK;  // (the test hook's buffer is sized for a packed batch: a masked pass leaves it alone)
  OP_TRY(L.begin(PK_CAPTURE));
  hipLaunchKernelGGL(capture_rows_kernel, dim3(row_blocks), dim3(256), 0, st, ws.x, ws.row_tok, H, r_pad,
                     h->capture + (size_t)index * b.total_tokens * H);
  return L.end();
}

int ChunkPass::hidden_pooled(int index) {
  if (!hid || !hid->pooled(index)) return OP_OK;
  OP_TRY(L.begin(PK_CAPTURE));
  hipLaunchKernelGGL(pool_hidden_kernel, dim3((unsigned)ns, (unsigned)((H + POOL_COLS - 1) / POOL_COLS)), dim3(256), 0, st, hid->scratch,
                     b.cu_dev, s0, b.total_tokens, H, hid->pool_kind, hid->pool_out + (size_t)hid->pool_slot[index] * (size_t)hid->n_seqs * H);
  if (hid->full(index))
    hipLaunchKernelGGL(hidden_repack_kernel, dim3(row_blocks), dim3(256), 0, st, hid->scratch, H, r_pad, ws.row_tok, ws.row_seq,
                       ws.row_pos, s0, hid->pad, hid->bf16, hid->out + (size_t)hid->slot[index] * hid->entry_bytes);
  return L.end();
}
int ChunkPass::hidden(int index, const float* ln) {
  void* dst = hidden_entry(index);
  if (!dst) return OP_OK;
  OP_TRY(L.begin(PK_CAPTURE));
  hipLaunchKernelGGL(hidden_rows_kernel, dim3(row_blocks), dim3(256), 0, st, ws.x, ln, h->cfg.norm_eps, H, r_pad,
                     ws.row_tok, ws.row_seq, ws.row_pos, s0, hidden_pad(index), hidden_bf16(index), dst);
  OP_TRY(L.end());
  return hidden_pooled(index);
}

int ChunkPass::attention(bool is_global) {
  OP_TRY(L.begin(is_global ? PK_ATTN_GLOBAL : PK_ATTN_LOCAL));
  const int window = is_global ? -1 : h->cfg.local_attention / 2;
  if (fp_layout) {
    // one block per (sequence, query block, head) work item: 256- or 128-query blocks on 64-key tiles for the
    // full-attention layers, 128-query blocks on 32-key tiles for the sliding-window layers
    AttnFpParams ap;  // q_hi/q_lo (k, vt, o likewise) are adjacent: together they hold the fragment-packed tensor
    ap.q_fp = ws.q_hi;
    ap.k_fp = ws.k_hi;
    ap.vt_fp = ws.vt_hi;
    ap.o_fp = ws.o_hi;
    ap.o_lo8 = ws.o_lo;
    ap.cu = b.cu_dev;
    ap.s0 = s0;
    ap.roff = ws.roff;
    ap.qboff = is_global ? ws.qboff : ws.qboff_l;
    ap.ns = ns;
    ap.H = H;
    ap.r_pad = r_pad;
    ap.window = window;
    ap.n_items = is_global ? plan.items_g : plan.items_l;
    ap.n_heads = h->nh;
    // XCD-aware block map (see attn_fp_kernel): panel path; round 3: also the row path under the fp16 + e4m3 kernel sets
    // (same-box A/B: sliding-window attention -5 %, whole forward +0.7 %; with the (hi, lo) bf16 whole-layer kernel
    // it measured -1 % in round 2 and stays off there unless OP_FLAG_ATTN_XCD_GROUP asks for it)
    ap.xcd_group = (h->panel_path || o_f8 || (h->cfg.flags & OP_FLAG_ATTN_XCD_GROUP)) ? 1 : 0;
    ap.range_flag = range_flagged ? ws.range_flag : nullptr;
    const unsigned item_span = 8u * opk::ATT_ITEM_GROUP;
    const dim3 grid((ap.xcd_group ? ((unsigned)ap.n_items + item_span - 1) / item_span * item_span : (unsigned)ap.n_items) *
                    (unsigned)h->nh);
    const int waves = is_global ? plan.waves_g : 4, kt = is_global ? 2 : 1;
    if (msk && msk->native) {
      // the mask removes keys; a query of a sliding-window layer left without one takes the row's mean of v as the set stores it
      ap.key_row = msk->key_row;
      ap.vmean = is_global ? nullptr : msk->vmean;
      if (!is_global) {
        const dim3 vgrid((unsigned)ns, (unsigned)h->nh);
        if (attn16 || V.fmt == 2)
          hipLaunchKernelGGL((vmean_fp_kernel<true, false>), vgrid, dim3(256), 0, st, ws.vt_hi, b.cu_dev, s0, ws.roff, H, r_pad, msk->vmean);
        else if (V.pv & 2)
          hipLaunchKernelGGL((vmean_fp_kernel<false, true>), vgrid, dim3(256), 0, st, ws.vt_hi, b.cu_dev, s0, ws.roff, H, r_pad, msk->vmean);
        else
          hipLaunchKernelGGL((vmean_fp_kernel<false, false>), vgrid, dim3(256), 0, st, ws.vt_hi, b.cu_dev, s0, ws.roff, H, r_pad, msk->vmean);
      }
      if (!opl::launch_attn_masked(st, ap, waves, kt, pi, zero_p_lo, grid, attn16))
        return fail(h, OP_ERR_UNSUPPORTED, "internal: no masked attention kernel for this configuration");
    } else if (!opl::launch_attn(st, ap, waves, kt, pi, zero_p_lo, grid, attn16))
      return fail(h, OP_ERR_UNSUPPORTED, "internal: no attention kernel for this configuration");
  } else {
    const dim3 grid((unsigned)q_tiles, (unsigned)h->nh, (unsigned)ns);
    AttnParams ap;
    ap.q_hi = ws.q_hi;
    ap.q_lo = ws.q_lo;
    ap.k_hi = ws.k_hi;
    ap.k_lo = ws.k_lo;
    ap.vt_hi = ws.vt_hi;
    ap.vt_lo = ws.vt_lo;
    ap.o_hi = ws.o_hi;
    ap.o_lo = ws.o_lo;
    ap.cu = b.cu_dev;
    ap.s0 = s0;
    ap.roff = ws.roff;
    ap.H = H;
    ap.r_pad = r_pad;
    ap.window = window;
    ap.zero_p_lo = (E.pv & 1) ? 0 : 1;
    if (split)
      hipLaunchKernelGGL((attn_kernel<true>), grid, dim3(256), 0, st, ap);
    else
      hipLaunchKernelGGL((attn_kernel<false>), grid, dim3(256), 0, st, ap);
  }
  OP_TRY(L.end());
  if (fp_layout && clr_o) OP_TRY(clear_lo(L, ws.o_hi, 512, (size_t)(r_pad / 16) * (H / 32)));
  if (!fp_layout && split && !(E.attn_out & 1)) OP_HIP(h, hipMemsetAsync(ws.o_lo, 0, plane_bytes, st));
  return OP_OK;
}
// fragment-packed q / k / v^T just written by a q/k/v projection: clear what the policy does not carry
int ChunkPass::clear_qkv() {
  if (clr_q) OP_TRY(clear_lo(L, ws.q_hi, 512, (size_t)(r_pad / 16) * (H / 32)));
  if (clr_k) OP_TRY(clear_lo(L, ws.k_hi, 512, (size_t)(r_pad / 16) * (H / 32)));
  if (clr_v) OP_TRY(clear_lo(L, ws.vt_hi, 2048, (size_t)h->nh * (r_pad / 32)));
  return OP_OK;
}
int ChunkPass::clear_h() {
  if (clr_h) OP_TRY(clear_lo(L, ws.h_hi, 512, (size_t)(r_pad / 16) * (I / 32)));
  return OP_OK;
}

// final_norm + pruning head (unless the last whole-layer launch did it), ranking head
int ChunkPass::heads() {
  const int mean_pool = h->cfg.pooling == OP_POOL_MEAN ? 1 : 0;
  if (head_done) OP_TRY(hidden_pooled(h->N));  // (entry N came from the last whole-layer launch's epilogue)
  if (!head_done) {
    // (before final_ln_prune_kernel: under mean pooling it writes the normalised rows over x)
    OP_TRY(hidden(h->N, h->cfg.prune_pre_final_norm ? nullptr : h->final_norm));
    OP_TRY(L.begin(PK_FINAL_LN_PRUNE));
    hipLaunchKernelGGL(final_ln_prune_kernel, dim3(row_blocks), dim3(256), 0, st, ws.x, h->final_norm, h->cfg.norm_eps, H,
                       r_pad, ws.row_tok, ws.row_seq, ws.row_pos, h->prune_w, h->prune_b, b.prune_out, b.keep_prob,
                       h->cfg.prune_pre_final_norm ? 1 : 0, mean_pool, ws.cls,
                       (h->capture && !msk) ? h->capture + (size_t)h->N * b.total_tokens * H : nullptr,
                       range_flagged ? ws.range_flag : nullptr);
    OP_TRY(L.end());
  }
  OP_TRY(L.begin(PK_RANK_HEAD));
  if (msk) {
    if (msk->native)
      hipLaunchKernelGGL(rank_head_masked_kernel, dim3((unsigned)ns), dim3(256), 0, st, ws.cls, ws.x, b.cu_dev, s0, ws.roff, msk->key_ok,
                         mean_pool, H, h->nl, h->dense_t, h->head_norm, h->cfg.norm_eps, h->cls_w, h->cls_b, b.rank_out,
                         range_flagged ? ws.range_flag : nullptr);
    else
      opl::launch_f32_rank_head_masked(st, ns, ws.cls, ws.x, b.cu_dev, s0, ws.roff, msk->key_ok, mean_pool, H, h->nl, h->dense_t,
                                       h->head_norm, h->cfg.norm_eps, h->cls_w, h->cls_b, b.rank_out);
    // (final_ln_prune_kernel wrote every position of the chunk's rows: tokens cu[s0] .. cu[s0 + ns])
    opl::launch_prune_mask(st, b.prune_out, msk->key_ok, (size_t)msk->cu_host[s0], (size_t)(msk->cu_host[s0 + ns] - msk->cu_host[s0]));
  } else if (f32)
    opl::launch_f32_rank_head(st, ns, ws.cls, ws.x, b.cu_dev, s0, ws.roff, mean_pool, H, h->nl, h->dense_t, h->head_norm, h->cfg.norm_eps,
                              h->cls_w, h->cls_b, b.rank_out);
  else
    hipLaunchKernelGGL(rank_head_kernel, dim3((unsigned)ns), dim3(256), 0, st, ws.cls, ws.x, b.cu_dev, s0, ws.roff, mean_pool,
                     H, h->nl, h->dense_t, h->head_norm, h->cfg.norm_eps, h->cls_w, h->cls_b, b.rank_out,
                     range_flagged ? ws.range_flag : nullptr);
  OP_TRY(L.end());
  return OP_OK;
}

int ChunkPass::run() {
  OP_TRY(prologue());
  if (!embed_in_qkv0) OP_TRY(hidden(0));
  for (int li = 0; li < h->N; ++li) {
    OP_TRY(capture(li));
    if (f32) OP_TRY(f32_layer(li));
    else if (h->row_path) OP_TRY(row_layer(li));
    else if (h->panel_path) OP_TRY(panel_layer(li));
    else OP_TRY(tiled_layer(li));
    // output of layer li = entry li + 1 (entry N is the head's input: heads() / the last whole-layer launch), unless the
    // wave-pair launch stored it from its epilogue
    if (li + 1 < h->N && hidden_stored != li + 1) OP_TRY(hidden(li + 1));
    if (hidden_stored == li + 1) OP_TRY(hidden_pooled(li + 1));
  }
  return heads();
}

// The batch's cu_seqlens on the host -- the caller's copy, or read back from the device (synchronises the stream once) -- held
// to what every pass over a packed batch relies on (opp::check_cu_seqlens).
int host_cu_seqlens(op_handle* h, const PackedBatch& b, std::vector<int32_t>& cu_copy, const int32_t** cu_out) {
  const int32_t* cu = b.cu_host;
  if (!cu) {
    cu_copy.resize((size_t)b.n_seqs + 1);
    OP_HIP(h, hipMemcpyAsync(cu_copy.data(), b.cu_dev, cu_copy.size() * sizeof(int32_t), hipMemcpyDeviceToHost, b.stream));
    OP_HIP(h, hipStreamSynchronize(b.stream));
    cu = cu_copy.data();
  }
  const opp::Refusal bad = opp::check_cu_seqlens(cu, b.n_seqs, b.total_tokens, b.max_seqlen, h->max_pos);
  if (bad.code != OP_OK) return fail(h, bad);
  *cu_out = cu;
  return OP_OK;
}

// op_forward_packed, and op_forward_packed_hidden / _pooled with their validated request (hid; nullptr: none)
int forward_packed_impl(op_handle* h, const PackedBatch& b, const HiddenReq* hid, const MaskedReq* msk) {
  if (!h) return fail(nullptr, OP_ERR_INVALID, "op_forward_packed: NULL handle");
  if (b.n_seqs < 0 || b.total_tokens < 0 || b.max_seqlen < 0) return fail(h, OP_ERR_INVALID, "negative size");
  if (b.n_seqs == 0 || b.total_tokens == 0) {
    if (b.n_seqs > 0 && b.rank_out) OP_HIP(h, hipMemsetAsync(b.rank_out, 0, (size_t)b.n_seqs * h->nl * sizeof(float), b.stream));
    if (b.n_seqs > 0 && hid && hid->n_pool > 0)  // only empty sequences: every pooled row is +0.0
      OP_HIP(h, hipMemsetAsync(hid->pool_out, 0, (size_t)hid->n_pool * b.n_seqs * h->H * sizeof(float), b.stream));
    return OP_OK;
  }
  if (!b.ids_dev || !b.cu_dev || !b.prune_out || !b.rank_out || !b.workspace)
    return fail(h, OP_ERR_INVALID, "op_forward_packed: NULL buffer");
  if (op_weights_ready(h) != OP_OK) return OP_ERR_STATE;
  if ((reinterpret_cast<uintptr_t>(b.workspace) & 255) != 0)
    return fail(h, OP_ERR_WORKSPACE, "workspace must be 256-byte aligned");
  const opp::Layout lay = forward_layout(h, b.n_seqs, b.total_tokens, b.max_seqlen, (msk && !msk->native) || h->set == OP_KS_F32);  // (= op_workspace_bytes)
  if (b.workspace_bytes < lay.bytes)
    return fail(h, OP_ERR_WORKSPACE, "workspace has %zu bytes, need %zu", b.workspace_bytes, lay.bytes);

  OP_HIP(h, hipSetDevice(h->cfg.device_id));
  std::vector<int32_t> cu_copy;
  const int32_t* cu = nullptr;
  OP_TRY(host_cu_seqlens(h, b, cu_copy, &cu));

  const int cap = chunk_row_capacity(h, b.n_seqs, b.total_tokens, b.max_seqlen);
  Workspace ws;
  carve(lay, reinterpret_cast<char*>(b.workspace), ws);

  Launcher L{h, b.stream};
  int s0 = 0;
  while (s0 < b.n_seqs) {
    int rows = 0, max_len = 0;
    const int s1 = opp::next_chunk(cu, s0, b.n_seqs, cap, &rows, &max_len);
    if (rows > cap) return fail(h, OP_ERR_WORKSPACE, "internal: chunk of %d rows exceeds capacity %d", rows, cap);
    const AttnPlan plan = opp::attention_plan(cu, s0, s1, max_len, h->nh, h->n_cus, h->cfg.flags);
    if (rows > 0) {
      OP_TRY(ChunkPass(h, L, ws, b, s0, s1 - s0, rows, max_len, plan, hid, msk).run());
    } else {
      // only empty sequences in this chunk
      OP_HIP(h, hipMemsetAsync(b.rank_out + (size_t)s0 * h->nl, 0, (size_t)(s1 - s0) * h->nl * sizeof(float), b.stream));
      for (int e = 0; hid && e < hid->n_pool; ++e)  // (their pooled rows: +0.0)
        OP_HIP(h, hipMemsetAsync(hid->pool_out + ((size_t)e * b.n_seqs + s0) * h->H, 0, (size_t)(s1 - s0) * h->H * sizeof(float), b.stream));
    }
    s0 = s1;
  }
  return OP_OK;
}

}  // namespace oph

// op_forward_packed_hidden / op_forward_packed_pooled: the two requests checked (their own fields first: none of them needs the
// handle), then one forward with whatever they select
static int forward_packed_requests(const char* what, op_handle* h, const PackedBatch& b, const op_hidden_request* req,
                                   const op_pool_request* pool, bool pool_required) {
  if (req) {
    if (req->struct_bytes != sizeof(op_hidden_request))
      return fail(h, OP_ERR_INVALID, "%s: op_hidden_request.struct_bytes is %u, expected %zu", what, req->struct_bytes,
                  sizeof(op_hidden_request));
    if (req->dtype != OP_HIDDEN_F32 && req->dtype != OP_HIDDEN_BF16)
      return fail(h, OP_ERR_INVALID, "%s: unknown dtype %d", what, req->dtype);
    if (req->pad_width < 0 || (req->pad_width > 0 && req->pad_width < b.max_seqlen))
      return fail(h, OP_ERR_INVALID, "%s: pad_width %d below max_seqlen %d", what, req->pad_width, b.max_seqlen);
  }
  if (pool_required && !pool) return fail(h, OP_ERR_INVALID, "%s: the pooled request is NULL", what);
  if (pool) {
    if (pool->struct_bytes != sizeof(op_pool_request))
      return fail(h, OP_ERR_INVALID, "%s: op_pool_request.struct_bytes is %u, expected %zu", what, pool->struct_bytes, sizeof(op_pool_request));
    if (pool->kind != OP_HIDDEN_POOL_FIRST && pool->kind != OP_HIDDEN_POOL_MEAN)
      return fail(h, OP_ERR_INVALID, "%s: unknown pooling kind %d", what, pool->kind);
    if ((reinterpret_cast<uintptr_t>(pool->scratch_dev) & 15) != 0)
      return fail(h, OP_ERR_INVALID, "%s: scratch_dev must be 16-byte aligned", what);
  }
  if (!h) return fail(nullptr, OP_ERR_INVALID, "%s: NULL handle", what);
  if (!req && !pool) return forward_packed_impl(h, b, nullptr);
  HiddenReq hid;
  int n_sel = 0;
  if (req) {
    hid.out = reinterpret_cast<char*>(req->out_dev);
    hid.bf16 = req->dtype == OP_HIDDEN_BF16 ? 1 : 0;
    hid.pad = req->pad_width;
    hid.slot.assign((size_t)h->N + 1, -1);
    for (int i = 0; i <= h->N; ++i)
      if (!req->select || req->select[i]) hid.slot[i] = n_sel++;
    const size_t rows = hid.pad > 0 ? (size_t)std::max(b.n_seqs, 0) * (size_t)hid.pad : (size_t)std::max(b.total_tokens, 0);
    if (rows > (size_t)INT32_MAX)  // (destination rows are 32-bit indices in the kernels' epilogues)
      return fail(h, OP_ERR_INVALID, "%s: %zu destination rows per entry exceed 2^31 - 1", what, rows);
    hid.entry_bytes = rows * (size_t)h->H * (hid.bf16 ? 2 : 4);
    if (n_sel > 0 && hid.entry_bytes > 0 && !hid.out)
      return fail(h, OP_ERR_INVALID, "%s: out_dev is NULL with %d entries selected", what, n_sel);
    if (n_sel == 0) hid.slot.clear();
  }
  if (pool) {
    hid.pool_kind = pool->kind == OP_HIDDEN_POOL_MEAN ? POOL_MEAN : POOL_FIRST;
    hid.pool_out = pool->out_dev;
    hid.scratch = reinterpret_cast<float*>(pool->scratch_dev);
    hid.n_seqs = std::max(b.n_seqs, 0);
    hid.pool_slot.assign((size_t)h->N + 1, -1);
    for (int i = 0; i <= h->N; ++i)
      if (!pool->select || pool->select[i]) hid.pool_slot[i] = hid.n_pool++;
    const size_t scratch_need = (size_t)std::max(b.total_tokens, 0) * (size_t)h->H * sizeof(float);
    if (hid.n_pool > 0 && b.n_seqs > 0 && !hid.pool_out)
      return fail(h, OP_ERR_INVALID, "%s: the pooled out_dev is NULL with %d entries selected", what, hid.n_pool);
    if (hid.n_pool > 0 && b.n_seqs > 0 && scratch_need > 0 && !hid.scratch)
      return fail(h, OP_ERR_INVALID, "%s: scratch_dev is NULL", what);
    if (hid.n_pool > 0 && b.n_seqs > 0 && pool->scratch_bytes < scratch_need)
      return fail(h, OP_ERR_INVALID, "%s: scratch has %zu bytes, one packed fp32 entry needs %zu", what, (size_t)pool->scratch_bytes, scratch_need);
    if (hid.n_pool == 0) hid.pool_slot.clear();
  }
  return forward_packed_impl(h, b, (n_sel > 0 || hid.n_pool > 0) ? &hid : nullptr);
}

extern "C" {

int op_forward_packed(op_handle* h, const int32_t* ids_dev, const int32_t* cu_dev, const int32_t* cu_host_in, int n_seqs,
                      int total_tokens, int max_seqlen, float* prune_out, float* rank_out, float* keep_prob,
                      void* workspace, size_t workspace_bytes, void* hip_stream) {
  const PackedBatch b{ids_dev,  cu_dev,    cu_host_in, n_seqs,    total_tokens,    max_seqlen,
                      prune_out, rank_out, keep_prob,  workspace, workspace_bytes, reinterpret_cast<hipStream_t>(hip_stream)};
  return forward_packed_impl(h, b, nullptr);
}

int op_forward_packed_hidden(op_handle* h, const int32_t* ids_dev, const int32_t* cu_dev, const int32_t* cu_host_in, int n_seqs,
                             int total_tokens, int max_seqlen, float* prune_out, float* rank_out, float* keep_prob,
                             void* workspace, size_t workspace_bytes, void* hip_stream, const op_hidden_request* req) {
  const PackedBatch b{ids_dev,  cu_dev,    cu_host_in, n_seqs,    total_tokens,    max_seqlen,
                      prune_out, rank_out, keep_prob,  workspace, workspace_bytes, reinterpret_cast<hipStream_t>(hip_stream)};
  return forward_packed_requests("op_forward_packed_hidden", h, b, req, nullptr, false);
}

int op_forward_packed_pooled(op_handle* h, const int32_t* ids_dev, const int32_t* cu_dev, const int32_t* cu_host_in, int n_seqs,
                             int total_tokens, int max_seqlen, float* prune_out, float* rank_out, float* keep_prob,
                             void* workspace, size_t workspace_bytes, void* hip_stream, const op_hidden_request* req,
                             const op_pool_request* pool) {
  const PackedBatch b{ids_dev,  cu_dev,    cu_host_in, n_seqs,    total_tokens,    max_seqlen,
                      prune_out, rank_out, keep_prob,  workspace, workspace_bytes, reinterpret_cast<hipStream_t>(hip_stream)};
  return forward_packed_requests("op_forward_packed_pooled", h, b, req, pool, true);
}

}  // extern "C"
