// op_forward_layers.hip -- one layer of the forward's launch sequence on each path (ChunkPass::row_layer / panel_layer /
// tiled_layer / f32_layer; op_forward.h).  The one unit that compiles the tiled GEMM (opk_tiled.hip.h) and the LayerNorm
// launches of the tiled and panel layers (opk_layernorm.hip.h).
#include "op_forward.h"
#include "opk_layernorm.hip.h"
#include "opk_tiled.hip.h"

namespace oph {

template <int EPI>
static int launch_gemm(Launcher& L, int kind, const GemmParams& p, bool split) {
  OP_TRY(L.begin(kind));
  const dim3 grid((unsigned)(p.n_tiles * p.m_tiles));
  if (split)
    hipLaunchKernelGGL((gemm_kernel<EPI, true>), grid, dim3(256), 0, L.stream, p);
  else
    hipLaunchKernelGGL((gemm_kernel<EPI, false>), grid, dim3(256), 0, L.stream, p);
  return L.end();
}

// parameters of a q/k/v projection of layer `li` (row-stationary kernels)
RowGemmParams ChunkPass::qkv_params(int li) {
  const bool is_global = h->cfg.layer_is_global[li] != 0;
  RowGemmParams rp;
  memset(&rp, 0, sizeof(rp));
  rp.eps = h->cfg.norm_eps;
  rp.hidden = H;
  rp.r_pad = r_pad;
  rp.row_pos = ws.row_pos;
  rp.rope_cos = h->rope_cos[is_global ? 1 : 0];
  rp.rope_sin = h->rope_sin[is_global ? 1 : 0];
  rp.max_pos = h->max_pos;
  rp.x_in = ws.x;
  rp.ln_w = h->layers[li].attn_norm;
  rp.wp = weight(li, W_QKV, fmt_base);
  rp.n_chunks = 3 * H / ROW_CHUNK;
  rp.n_swapped = 2 * H / ROW_CHUNK;
  rp.o0_hi = ws.q_hi;
  rp.o1_hi = ws.k_hi;
  rp.o2_hi = ws.vt_hi;
  rp.ld_out = H;
  rp.zero_a_lo = clr_ln_attn ? 1 : 0;
  return rp;
}

// one layer on the row path: (layer 0: q / k / v) -> attention -> the whole-layer kernel, or the two fused kernels of set 0
int ChunkPass::row_layer(int li) {
  const LayerWeights& lw = h->layers[li];
  const bool is_global = h->cfg.layer_is_global[li] != 0;
  // ---- row-stationary path (hidden <= 256): three launches per layer ------------------------------
  if (li == 0) {  // layer 0 has no attn_norm: split x0 directly
    RowGemmParams rp = qkv_params(0);
    if (embed_in_qkv0) {
      rp.emb_table = h->emb;
      rp.emb_ids = b.ids_dev;
      rp.emb_vocab = h->V;
      rp.row_tok = ws.row_tok;
      rp.ln_w = h->emb_norm;
      rp.x_io = ws.x;
    }
    OP_TRY(L.begin(PK_ROW_QKV));
    if (!opl::launch_row_qkv0(st, rp, H / 32, small_blocks, pi, row_grid)) return fail(h, OP_ERR_UNSUPPORTED, no_kernel, H);
    OP_TRY(L.end());
    OP_TRY(clear_qkv());
    if (embed_in_qkv0) OP_TRY(hidden(0));  // (the embedding rows were written by the launch above)
  }  // else: q/k/v of this layer were produced by the fused kernel that closed layer li-1
  OP_TRY(attention(is_global));

  if (layer_fused) {
    // x += o Wo^T ; x += GeGLU(LN(x) Wi^T) Wo^T ; q, k, v^T of the NEXT layer -- one kernel, h stays on chip
    const bool with_qkv = li + 1 < h->N;
    // The two other forms of this launch, hidden = 256.  OP_FLAG_LAYER_M32, on request: the 32x32x16 MFMA shape
    // (opk_layer32.hip.h) -- 6 % fewer cycles, but that shape draws more power per flop and the chip clocks lower under it
    // (DESIGN.md section 4).
    // Single-pass kernel sets ("f16" / "bf16"): the wave-pair kernel (opk_layer16p.hip.h), at every batch size --
    // below one 128-row block per CU too, where the other launches switch to 64-row blocks (small_blocks): 4 - 8 % faster
    // forwards from 512 to 32 k tokens than the 8 x 16 kernel's 64-row form (profiles/r06_small_request.txt).  The last layer keeps the 8 x 16 kernel (it ends with final_norm + the pruning head).  Between two
    // wave-pair launches the residual stream is TILED (coalesced 1 KiB loads / stores): the first one reads rows, the last
    // one writes rows.  Hidden-state capture reads rows after every layer: it keeps the 8 x 16 kernel.  A per-call
    // hidden-state request does not change the kernel: its entry li + 1 is stored from this launch's epilogue (layer16p_hout_kernel).
    const bool m32 = (h->cfg.flags & OP_FLAG_LAYER_M32) && weight(li, W_ATTN_OUT, PF_L32) && opl::has_layer32(pi) && I % 64 == 0;
    if (m32 || (pair_layers && with_qkv)) {
      const PackFmt pf = m32 ? PF_L32 : (f16 ? PF_PAIR16 : PF_PAIR);
      const int nx = with_qkv ? li + 1 : li;
      Layer32Params lp;
      memset(&lp, 0, sizeof(lp));
      lp.o_fp = ws.o_hi;
      lp.x_io = ws.x;
      lp.ln_mlp = lw.mlp_norm;
      lp.ln_next = with_qkv ? h->layers[nx].attn_norm : nullptr;
      lp.eps = h->cfg.norm_eps;
      lp.wo_p = weight(li, W_ATTN_OUT, pf);
      lp.wi_p = weight(li, W_WI, pf);
      lp.wo2_p = weight(li, W_MLP_OUT, pf);
      lp.wqkv_p = weight(nx, W_QKV, pf);
      lp.n_pairs = I / 32;
      lp.q_fp = ws.q_hi;
      lp.k_fp = ws.k_hi;
      lp.vt_fp = ws.vt_hi;
      lp.r_pad = r_pad;
      lp.row_pos = ws.row_pos;
      const int gl = h->cfg.layer_is_global[nx] ? 1 : 0;
      lp.rope_cos = h->rope_cos[gl];
      lp.rope_sin = h->rope_sin[gl];
      lp.max_pos = h->max_pos;
      if (!m32) lp.hid_out = hidden_entry(li + 1);
      if (lp.hid_out) {
        lp.row_tok = ws.row_tok;
        lp.row_seq = ws.row_seq;
        lp.hid_bf16 = hidden_bf16(li + 1);
        lp.hid_pad = hidden_pad(li + 1);
        lp.hid_s0 = s0;
        hidden_stored = li + 1;
      }
      OP_TRY(L.begin(PK_FUSED_LAYER));
      const unsigned grid = (unsigned)(r_pad / ROW_BM);
      if (!(m32 ? opl::launch_layer32(st, lp, pi, with_qkv, grid)
                : opl::launch_layer16p(st, lp, f16, true, /*xin_t=*/li > 0, /*xout_t=*/li + 2 < h->N, grid, lp.hid_out != nullptr)))
        return fail(h, OP_ERR_UNSUPPORTED, no_kernel, H);
      OP_TRY(L.end());
      return OP_OK;
    }
    RowGemmParams rl = qkv_params(with_qkv ? li + 1 : li);
    rl.a1_fp = ws.o_hi;
    rl.wp = weight(with_qkv ? li + 1 : li, W_QKV, fmt_side);  // (sets 3 / 4: layer 0's own projection ran on fmt_base)
    rl.w1p = weight(li, W_ATTN_OUT, fmt_side);
    rl.k1_steps = H / 32;
    rl.x_io = ws.x;
    rl.ln_w_mlp = lw.mlp_norm;
    rl.wi_pk = weight(li, W_WI, fmt_side);
    rl.wo2_ks = weight(li, W_MLP_OUT, fmt_side);
    rl.n_pairs = I / 32;
    if (o_f8) {  // the e4m3 pieces of o and of the attention Wo
      rl.a1_lo8 = ws.o_lo;
      rl.w1p8 = weight(li, W_ATTN_OUT, PF_ROW_F8B);
    }
    if (!with_qkv && head_in_last_layer) {
      // the last layer's rows go straight through final_norm + the pruning head (no write-back of x, no
      // final_ln_prune launch); mean pooling and hidden-state capture need all normalised rows and keep the kernel
      rl.fin_ln = h->final_norm;
      rl.fin_pw = h->prune_w;
      rl.fin_pb = h->prune_b;
      rl.row_tok = ws.row_tok;
      rl.row_seq = ws.row_seq;
      rl.fin_prune = b.prune_out;
      rl.fin_keep = b.keep_prob;
      rl.fin_cls = ws.cls;
      rl.fin_pre_norm = h->cfg.prune_pre_final_norm ? 1 : 0;
      head_done = true;
      rl.hid_out = hidden_entry(h->N);  // (entry N from the head's epilogue: this launch writes no x)
      if (rl.hid_out) {
        rl.hid_bf16 = hidden_bf16(h->N);
        rl.hid_pad = hidden_pad(h->N);
        rl.hid_s0 = s0;
      }
    }
    OP_TRY(L.begin(PK_FUSED_LAYER));
    if (!opl::launch_row_layer_fused(st, rl, H / 32, pi, with_qkv, (unsigned)(r_pad / ROW_BM),
                                     (h->cfg.flags & OP_FLAG_LAYER_8X16) != 0 || (V.wi & 1) == 0,
                                     rl.hid_out != nullptr))
      return fail(h, OP_ERR_UNSUPPORTED, no_kernel, H);
    OP_TRY(L.end());
    return OP_OK;
  }

  // x += o Wo^T ; h = GeGLU(LN(x) Wi^T)   -- one kernel, the hidden state stays in registers in between
  RowGemmParams rp;
  memset(&rp, 0, sizeof(rp));
  rp.eps = h->cfg.norm_eps;
  rp.hidden = H;
  rp.r_pad = r_pad;
  rp.ln_w = lw.mlp_norm;
  rp.wp = weight(li, W_WI, PF_PK);
  rp.n_chunks = 2 * I / ROW_CHUNK;
  rp.o0_hi = ws.h_hi;  // fragment-packed h (h_hi + h_lo are one buffer)
  rp.ld_out = I;
  rp.a1_fp = ws.o_hi;
  rp.w1p = weight(li, W_ATTN_OUT, PF_PK);
  rp.k1_steps = H / 32;
  rp.x_io = ws.x;
  rp.zero_a_lo = clr_ln_mlp ? 1 : 0;
  OP_TRY(L.begin(PK_FUSED_ATTN_OUT_WI));
  if (!opl::launch_row_geglu_fused(st, rp, H / 32, small_blocks, pi, row_grid)) return fail(h, OP_ERR_UNSUPPORTED, no_kernel, H);
  OP_TRY(L.end());
  OP_TRY(clear_h());

  if (li + 1 < h->N) {
    // x += h Wo^T ; q, k, v^T of the NEXT layer = RoPE / transpose of LN(x) Wqkv^T
    RowGemmParams rq = qkv_params(li + 1);
    rq.a1_fp = ws.h_hi;
    rq.w1p = weight(li, W_MLP_OUT, PF_PK);
    rq.k1_steps = I / 32;
    rq.x_io = ws.x;
    OP_TRY(L.begin(PK_FUSED_MLP_OUT_QKV));
    if (!opl::launch_row_qkv_fused(st, rq, H / 32, small_blocks, pi, row_grid)) return fail(h, OP_ERR_UNSUPPORTED, no_kernel, H);
    OP_TRY(L.end());
    OP_TRY(clear_qkv());
  } else {
    KStreamParams kp;
    kp.a_fp = ws.h_hi;
    kp.wp = weight(li, W_MLP_OUT, PF_PK);
    kp.n_ksteps = I / 32;
    kp.x = ws.x;
    OP_TRY(L.begin(PK_KSTREAM_MLP_OUT));
    if (!opl::launch_kstream(st, kp, H / 16, pi, (unsigned)(r_pad / ROW_BM))) return fail(h, OP_ERR_UNSUPPORTED, no_kernel, H);
    OP_TRY(L.end());
  }
  return OP_OK;
}

// one layer on the panel path: LayerNorm -> q / k / v -> attention -> output projection -> LayerNorm -> Wi + GeGLU -> MLP output
int ChunkPass::panel_layer(int li) {
  const LayerWeights& lw = h->layers[li];
  const bool is_global = h->cfg.layer_is_global[li] != 0;
  // ---- panel path (hidden % 256 == 0): LayerNorm -> fragment-packed planes, k-streamed panel GEMMs ----
  const dim3 ln_grid((unsigned)(r_pad / 16));
  const bool pf8 = o_f8;  // kernel sets 3 / 4 / 10 / 11: activations as fp16 pieces + e4m3 pieces (x 2^12) of their lo part
  const bool m8 = mlp8[li];
  auto layer_norm_fp = [&](const float* w, bool with_lo, bool clear, bool f8_here = false) -> int {
    OP_TRY(L.begin(PK_LN));
    if (pf8 || f8_here) {
      hipLaunchKernelGGL(ln_fp8_kernel, ln_grid, dim3(256), 0, st, ws.x, w, h->cfg.norm_eps, H, r_pad, w ? 1 : 0, ws.ln_hi,
                         ws.ln_lo);
      return L.end();
    }
    if (with_lo)
      hipLaunchKernelGGL((ln_fp_kernel<true>), ln_grid, dim3(256), 0, st, ws.x, w, h->cfg.norm_eps, H, r_pad,
                         w ? 1 : 0, ws.ln_hi);
    else if (f16)
      hipLaunchKernelGGL((ln_fp_kernel<false, true>), ln_grid, dim3(256), 0, st, ws.x, w, h->cfg.norm_eps, H, r_pad,
                         w ? 1 : 0, ws.ln_hi);
    else
      hipLaunchKernelGGL((ln_fp_kernel<false>), ln_grid, dim3(256), 0, st, ws.x, w, h->cfg.norm_eps, H, r_pad,
                         w ? 1 : 0, ws.ln_hi);
    OP_TRY(L.end());
    if (clear) OP_TRY(clear_lo(L, ws.ln_hi, 512, (size_t)(r_pad / 16) * (H / 32)));
    return OP_OK;
  };
  auto panel = [&](int kind, int epi, const PanelParams& pp, int n_tiles, bool f8_here = false, bool f8_full = false) -> int {
    OP_TRY(L.begin(kind));
    PanelParams q = pp;
    q.n_tiles = n_tiles;
    q.row_group = 8;  // sweep 1 / 2 / 4 / 8 / 16 on base and en-gte: flat within 2 %, 8 best on the Wi GEMM (-5 %)
    const unsigned per_xcd = ((unsigned)(r_pad / ROW_BM) + 7) / 8;  // row blocks each XCD owns
    const unsigned groups = (per_xcd + q.row_group - 1) / q.row_group;
    const dim3 grid(8u * groups * (unsigned)q.row_group * (unsigned)n_tiles);  // XCD-aware block map: see panel_gemm_kernel
    const bool ok = f8_here ? opl::launch_panel_f8(st, q, PANEL_EPI_GEGLU_BF16_H, wlo8, grid)
                    : f8_full ? opl::launch_panel_f8(st, q, epi, wlo8, grid)
                    : pf8   ? (epi == PANEL_EPI_QKV ? opl::launch_panel_f8_qkv(st, q, wlo8, attn16, grid) : opl::launch_panel_f8(st, q, epi, wlo8, grid))
                            : (epi == PANEL_EPI_QKV ? opl::launch_panel_qkv(st, q, pi, grid) : opl::launch_panel(st, q, epi, pi, grid));
    if (!ok) return fail(h, OP_ERR_UNSUPPORTED, "internal: no panel kernel");
    return L.end();
  };
  // layer 0: attn_norm is Identity -> plain split
  OP_TRY(layer_norm_fp(li != 0 ? lw.attn_norm : nullptr, (V.wqkv & 1) != 0, clr_ln_attn));
  PanelParams pp;
  memset(&pp, 0, sizeof(pp));
  pp.r_pad = r_pad;
  pp.hidden = H;
  pp.range_flag = range_flagged ? ws.range_flag : nullptr;
  pp.row_pos = ws.row_pos;
  pp.rope_cos = h->rope_cos[is_global ? 1 : 0];
  pp.rope_sin = h->rope_sin[is_global ? 1 : 0];
  pp.max_pos = h->max_pos;
  pp.a_fp = ws.ln_hi;
  pp.a_lo8 = ws.ln_lo;
  pp.n_ksteps = H / 32;
  pp.wp = weight(li, W_QKV, fmt_side);
  pp.wp8 = weight(li, W_QKV, PF_PANEL8);
  pp.w8_lo_off = (size_t)3 * H * H / 2;  // u16 elements: the tensor's e4m3(w) slabs, then those of lo(w)
  pp.o0 = ws.q_hi;
  pp.o1 = ws.k_hi;
  if (pf8 || !(h->cfg.flags & OP_FLAG_NO_LAYER_FUSION)) {  // q, k, v^T in one launch
    pp.o2 = ws.vt_hi;
    pp.n_qk_tiles = 2 * H / 256;
    OP_TRY(panel(PK_GEMM_QKV_ROPE, PANEL_EPI_QKV, pp, 3 * H / 256));
  } else {
    OP_TRY(panel(PK_GEMM_QK_ROPE, PE_QK, pp, 2 * H / 256));
    pp.wp = weight(li, W_QKV, fmt_base) + (size_t)(2 * H / 256) * (H / 32) * 2 * 8192;
    pp.o0 = ws.vt_hi;
    OP_TRY(panel(PK_GEMM_V_T, PE_V, pp, H / 256));
  }
  OP_TRY(clear_qkv());
  OP_TRY(attention(is_global));
  pp.a_fp = ws.o_hi;
  pp.a_lo8 = ws.o_lo;
  pp.wp = weight(li, W_ATTN_OUT, fmt_side);
  pp.wp8 = weight(li, W_ATTN_OUT, PF_PANEL8);
  pp.w8_lo_off = (size_t)H * H / 2;
  pp.x = ws.x;
  pp.ld_out = H;
  OP_TRY(panel(PK_GEMM_ATTN_OUT, PANEL_EPI_ATTN_OUT, pp, H / 256));
  OP_TRY(layer_norm_fp(lw.mlp_norm, (V.wi & 1) != 0, clr_ln_mlp && !wi8, wi8 || m8));
  pp.a_fp = ws.ln_hi;
  pp.a_lo8 = ws.ln_lo;
  pp.wp = weight(li, W_WI, m8 ? fmt_f8 : fmt_wi);
  pp.wp8 = weight(li, W_WI, PF_PANEL8);
  pp.w8_lo_off = (size_t)2 * I * H / 2;
  pp.o0 = ws.h_hi;
  pp.o0_lo8 = ws.h_lo;
  pp.ld_out = I;
  OP_TRY(panel(PK_GEMM_WI_GEGLU, PE_GEGLU, pp, I / 128, wi8, m8));
  OP_TRY(clear_h());
  pp.a_fp = ws.h_hi;
  pp.a_lo8 = ws.h_lo;
  pp.n_ksteps = I / 32;
  pp.wp = weight(li, W_MLP_OUT, m8 ? fmt_f8 : fmt_side);
  pp.wp8 = weight(li, W_MLP_OUT, PF_PANEL8);
  pp.w8_lo_off = (size_t)H * I / 2;
  pp.ld_out = H;
  OP_TRY(panel(PK_GEMM_MLP_OUT, PANEL_EPI_MLP_OUT, pp, H / 256, false, m8));
  return OP_OK;
}

// one layer on the tiled path (generic fallback)
int ChunkPass::tiled_layer(int li) {
  const LayerWeights& lw = h->layers[li];
  const bool is_global = h->cfg.layer_is_global[li] != 0;
  // ---- tiled path (any hidden % 128 == 0): separate LayerNorm kernels, 128 x 128 x 32 tiles, row-major planes.
  // Two kernel sets (single pass / all terms); a narrower policy clears the lo planes it does not carry. ----
  auto layer_norm = [&](const float* w, int term_mask) -> int {
    if (w) {
      OP_TRY(L.begin(PK_LN));
      if (split)
        hipLaunchKernelGGL((ln_kernel<true>), dim3(row_blocks), dim3(256), 0, st, ws.x, w, h->cfg.norm_eps, H, r_pad,
                           ws.ln_hi, ws.ln_lo);
      else
        hipLaunchKernelGGL((ln_kernel<false>), dim3(row_blocks), dim3(256), 0, st, ws.x, w, h->cfg.norm_eps, H, r_pad,
                           ws.ln_hi, ws.ln_lo);
      OP_TRY(L.end());
    }
    if (split && !(term_mask & 1)) OP_HIP(h, hipMemsetAsync(ws.ln_lo, 0, plane_bytes, st));
    return OP_OK;
  };
  OP_TRY(layer_norm(li != 0 ? lw.attn_norm : nullptr, E.wqkv));  // layer 0: embed_ln wrote the planes
  GemmParams p;
  memset(&p, 0, sizeof(p));
  p.a_hi = ws.ln_hi;
  p.a_lo = ws.ln_lo;
  p.K = H;
  p.m_tiles = m_tiles;
  p.hidden = H;
  p.row_pos = ws.row_pos;
  p.rope_cos = h->rope_cos[is_global ? 1 : 0];
  p.rope_sin = h->rope_sin[is_global ? 1 : 0];
  p.max_pos = h->max_pos;
  // q, k = RoPE(x Wq^T), RoPE(x Wk^T)
  p.w_hi = weight(li, W_QKV, PF_HI);
  p.w_lo = weight(li, W_QKV, PF_LO);
  p.n_tiles = 2 * H / GEMM_BN;
  p.o0_hi = ws.q_hi;
  p.o0_lo = ws.q_lo;
  p.o1_hi = ws.k_hi;
  p.o1_lo = ws.k_lo;
  p.ld_out = H;
  OP_TRY(launch_gemm<EPI_QK_ROPE>(L, PK_GEMM_QK_ROPE, p, split));
  // v^T
  p.w_hi = weight(li, W_QKV, PF_HI) + (size_t)2 * H * H;
  p.w_lo = weight(li, W_QKV, PF_LO) + (size_t)2 * H * H;
  p.n_tiles = H / GEMM_BN;
  p.o0_hi = ws.vt_hi;
  p.o0_lo = ws.vt_lo;
  p.ld_out = r_pad;
  OP_TRY(launch_gemm<EPI_V_T>(L, PK_GEMM_V_T, p, split));
  if (split && !(E.qk & 1)) OP_HIP(h, hipMemsetAsync(ws.q_lo, 0, plane_bytes, st));
  if (split && !(E.qk & 2)) OP_HIP(h, hipMemsetAsync(ws.k_lo, 0, plane_bytes, st));
  if (split && !(E.pv & 2)) OP_HIP(h, hipMemsetAsync(ws.vt_lo, 0, plane_bytes, st));

  OP_TRY(attention(is_global));

  // x += attn Wo^T
  p.a_hi = ws.o_hi;
  p.a_lo = ws.o_lo;
  p.w_hi = weight(li, W_ATTN_OUT, PF_HI);
  p.w_lo = weight(li, W_ATTN_OUT, PF_LO);
  p.K = H;
  p.n_tiles = H / GEMM_BN;
  p.x = ws.x;
  p.ld_out = H;
  OP_TRY(launch_gemm<EPI_RESIDUAL>(L, PK_GEMM_ATTN_OUT, p, split));
  // x += (gelu(a) * g) Wo^T,  (a, g) = LN(x) Wi^T
  OP_TRY(layer_norm(lw.mlp_norm, E.wi));
  p.a_hi = ws.ln_hi;
  p.a_lo = ws.ln_lo;
  p.w_hi = weight(li, W_WI, PF_HI);
  p.w_lo = weight(li, W_WI, PF_LO);
  p.K = H;
  p.n_tiles = 2 * I / GEMM_BN;
  p.o0_hi = ws.h_hi;
  p.o0_lo = ws.h_lo;
  p.ld_out = I;
  OP_TRY(launch_gemm<EPI_GEGLU>(L, PK_GEMM_WI_GEGLU, p, split));
  if (split && !(E.mlp_out & 1)) OP_HIP(h, hipMemsetAsync(ws.h_lo, 0, (size_t)r_pad * I * sizeof(u16), st));
  p.a_hi = ws.h_hi;
  p.a_lo = ws.h_lo;
  p.w_hi = weight(li, W_MLP_OUT, PF_HI);
  p.w_lo = weight(li, W_MLP_OUT, PF_LO);
  p.K = I;
  p.n_tiles = H / GEMM_BN;
  p.x = ws.x;
  p.ld_out = H;
  OP_TRY(launch_gemm<EPI_RESIDUAL>(L, PK_GEMM_MLP_OUT, p, split));
  return OP_OK;
}

// one layer of kernel set "fp32" (opk_f32.hip.h), on a handle of any path: LayerNorm, q / k / v projection, attention,
// attention output projection, LayerNorm, Wi + GeGLU, MLP output projection -- fp32 planes, the fp32 weights as loaded
int ChunkPass::f32_layer(int li) {
  const LayerWeights& lw = h->layers[li];
  const bool is_global = h->cfg.layer_is_global[li] != 0;
  auto f32_weight = [&](Weight w) { return reinterpret_cast<const float*>(weight(li, w, PF_F32)); };
  // layer 0: attn_norm is the identity, the residual stream is the operand
  auto layer_norm = [&](const float* w, const float*& plane) -> int {
    plane = ws.x;
    if (!w) return OP_OK;
    OP_TRY(L.begin(PK_LN));
    opl::launch_f32_ln(st, ws.x, w, h->cfg.norm_eps, H, r_pad, ws.f.ln);
    plane = ws.f.ln;
    return L.end();
  };
  auto gemm = [&](int kind, const F32GemmParams& p, int epi) -> int {
    OP_TRY(L.begin(kind));
    if (!opl::launch_f32_gemm(st, p, epi)) return fail(h, OP_ERR_UNSUPPORTED, "internal: no fp32 GEMM epilogue %d", epi);
    return L.end();
  };
  F32GemmParams p;
  memset(&p, 0, sizeof(p));
  p.m_tiles = m_tiles;
  p.hidden = H;
  p.inter = I;
  p.row_pos = ws.row_pos;
  p.rope_cos = h->rope_cos[is_global ? 1 : 0];
  p.rope_sin = h->rope_sin[is_global ? 1 : 0];
  p.max_pos = h->max_pos;
  // q, k = RoPE(LN(x) Wq^T), RoPE(LN(x) Wk^T); v = LN(x) Wv^T
  OP_TRY(layer_norm(li != 0 ? lw.attn_norm : nullptr, p.a));
  p.w = f32_weight(W_QKV);
  p.K = H;
  p.n_tiles = 3 * H / GEMM_BN;
  p.o0 = ws.f.q;
  p.o1 = ws.f.k;
  p.o2 = ws.f.v;
  p.ld_out = H;
  OP_TRY(gemm(PK_GEMM_QKV_ROPE, p, F32_EPI_QKV));

  OP_TRY(L.begin(is_global ? PK_ATTN_GLOBAL : PK_ATTN_LOCAL));
  F32AttnParams ap;
  ap.q = ws.f.q;
  ap.k = ws.f.k;
  ap.v = ws.f.v;
  ap.o = ws.f.o;
  ap.cu = b.cu_dev;
  ap.s0 = s0;
  ap.roff = ws.roff;
  ap.H = H;
  ap.window = is_global ? -1 : h->cfg.local_attention / 2;
  const dim3 attn_grid((unsigned)q_tiles, (unsigned)h->nh, (unsigned)ns);
  if (msk) {
    // the mask removes keys; a query of a sliding-window layer left without one takes the row's mean of v
    F32MaskedAttnParams mp;
    mp.a = ap;
    mp.key_ok = msk->key_ok;
    mp.vmean = is_global ? nullptr : msk->vmean;
    if (!is_global) opl::launch_f32_vmean(st, ws.f.v, b.cu_dev, s0, ws.roff, H, ns, msk->vmean);
    opl::launch_f32_attn_masked(st, mp, attn_grid);
  } else {
    opl::launch_f32_attn(st, ap, attn_grid);
  }
  OP_TRY(L.end());

  // x += o Wo^T
  p.a = ws.f.o;
  p.w = f32_weight(W_ATTN_OUT);
  p.n_tiles = H / GEMM_BN;
  p.x = ws.x;
  OP_TRY(gemm(PK_GEMM_ATTN_OUT, p, F32_EPI_RESIDUAL));
  // x += (gelu(a) * g) Wo^T,  (a, g) = LN(x) Wi^T
  OP_TRY(layer_norm(lw.mlp_norm, p.a));
  p.w = f32_weight(W_WI);
  p.n_tiles = I / 64;
  p.o0 = ws.f.h;
  p.ld_out = I;
  OP_TRY(gemm(PK_GEMM_WI_GEGLU, p, F32_EPI_GEGLU));
  p.a = ws.f.h;
  p.w = f32_weight(W_MLP_OUT);
  p.K = I;
  p.n_tiles = H / GEMM_BN;
  p.ld_out = H;
  OP_TRY(gemm(PK_GEMM_MLP_OUT, p, F32_EPI_RESIDUAL));
  return OP_OK;
}

}  // namespace oph
