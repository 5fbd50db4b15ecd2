// op_plan.h -- every decision of the C ABI that needs no device, as free functions over small plain structs: which kernel set
// a handle runs (selection), what op_calibrate measures and keeps (the search), how a packed batch is cut into chunks and
// attention work items, what a cu_seqlens must satisfy, and where each region of a workspace lies.  No HIP, no op_handle, no
// global state: the library calls these between its device calls, tests/host/plan_check.cpp calls them under a host sanitizer.
#pragma once

#include <stdint.h>

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <utility>
#include <vector>

#include "../../include/open_provence_hip.h"
#include "op_kernel_sets.h"

namespace opp {

using opl::Policy;
using namespace ops;

constexpr int ROW_ALIGN = 32;  // = opk::ROW_ALIGN (op_handle.h holds the two together)

inline int align_up(int v, int a) { return (v + a - 1) / a * a; }
inline size_t align_up_sz(size_t v, size_t a) { return (v + a - 1) / a * a; }

// ---- dispatch path and weight packs of a shape (op_create) --------------------------------------------------------------------
struct Paths {
  bool row;    // hidden <= 256: row-stationary GEMMs with fused LayerNorm
  bool panel;  // hidden % 256 == 0, intermediate % 128 == 0: k-streamed panel GEMMs, fragment-packed operands
};
inline Paths paths_of(int H, int I, unsigned flags) {
  // H % 64 and I % 32: every row-GEMM streams an EVEN number of 32-feature chunks on each side of the q/k -> v
  // boundary (H/16 q/k chunks, H/32 v chunks, H/32 out-projection chunks, I/16 Wi chunks) -- rowgemm_kernel's
  // two-stage loop is unrolled by two.
  const bool force_tiled = (flags & OP_FLAG_FORCE_TILED) != 0;
  Paths p;
  p.row = (H <= 256) && (H % 64 == 0) && (I % 32 == 0) && !force_tiled;
  // panels of 256 output features (4 heads; 128 GeGLU input + 128 gate columns), an even number of k-steps
  p.panel = !p.row && (H % 256 == 0) && (I % 128 == 0) && !force_tiled;
  return p;
}

struct Packs {
  bool f8;   // the "f16 + fp8" weight packs
  bool h16;  // the fp16 single-plane weight packs of kernel set "f16"
  bool f32;  // OP_FLAG_F32_PACKS: the row-major fp32 weight packs of kernel set "fp32"
};
inline Packs packs_of(Paths p, int H, unsigned flags) {
  Packs k;
  // panel path: opt-in (OP_FLAG_PANEL_F8) -- at the depth of the published models (19-25 layers) the format's error
  // reaches 0.45-1.0e-3 on logits, the (hi, lo) bf16 sets stay at 0.2-0.5e-3 (scripts/f8_depth_check.py)
  // (panel path: the packs are always built -- the Wi GEMM takes the format by default for fp32-valued weights, see
  // default_set; OP_FLAG_PANEL_F8 extends it to every GEMM of the layer)
  k.f8 = ((p.row && (H / 32) % 4 == 0) || p.panel) && !(flags & OP_FLAG_NO_F8);
  // kernel set "f16": whole-layer kernel shapes (hidden 128 / 256) or the panel path; never with the A/B flags that pick
  // another layer structure
  k.h16 = ((p.row && (H == 128 || H == 256)) || p.panel) && !(flags & (OP_FLAG_NO_F8 | OP_FLAG_NO_LAYER_FUSION | OP_FLAG_NO_POLICY_KERNELS));
  k.f32 = (flags & OP_FLAG_F32_PACKS) != 0;
  return k;
}

// ---- selection ----------------------------------------------------------------------------------------------------------------
// What the choice of a kernel set reads from a handle.
struct SelectState {
  Policy req = opl::kPolicies[0];     // requested term masks (op_config.precision / terms)
  bool any_lo[OP_FAM_COUNT] = {};     // device flags: some weight of the family has a non-zero lo element
  bool not_f16 = false;               // ... some GEMM weight is not exactly an fp16 value (no "f16 + fp8" default)
  bool f16_unfit = false;             // ... some weight TENSOR sits on fp16's subnormal grid: no set with an fp16 weight plane
  bool row_path = false, panel_path = false;
  bool f8_packs = false, h16_packs = false, f32_packs = false;
  bool f8_off = false;                // op_set_compact_operands(h, 0): keep the (hi, lo) bf16 sets although the packs exist
  unsigned flags = 0;                 // op_config.flags
  int forced_set = -1;                // op_select_kernel_set / op_calibrate: run this set, -1 = the default selection
  uint64_t forced_mlp_layers = ~0ull; // ... with this layer mask (sets 8 / 9)
};

struct Selection {
  Policy eff;           // evaluated term masks
  int set;              // the kernel set that runs (op_kernel_set numbering); -1: kClearedOperands
  uint64_t mlp_layers;  // sets 8 / 9: the layers whose MLP runs in that format
};

inline const KernelSet& set_row(int set) { return set >= 0 ? kKernelSets[set] : kClearedOperands; }

// Can this handle run kernel set `set` (op_kernel_set numbering)?  Packs present, a path that has the kernels, and no
// weight tensor below the reach of an fp16 plane for the sets that carry one: the set's `needs` (op_kernel_sets.h).
inline bool set_available(const SelectState& s, int set) {
  if (set < 0 || set >= OP_KS_COUNT) return false;
  const unsigned needs = kKernelSets[set].needs;
  if ((needs & NEED_F32_PACKS) && !s.f32_packs) return false;
  if (s.flags & OP_FLAG_NO_POLICY_KERNELS) return set == OP_KS_BF16X3 || set == OP_KS_F32;
  if ((needs & NEED_FAST) && !s.row_path && !s.panel_path) return false;
  if ((needs & NEED_PANEL) && !s.panel_path) return false;
  if ((needs & NEED_F8_PACKS) && !s.f8_packs) return false;
  if ((needs & NEED_H16_PACKS) && !s.h16_packs) return false;
  if ((needs & NEED_F16_FIT) && s.f16_unfit) return false;
  if ((needs & NEED_ROW_LAYER) && s.row_path && (s.flags & (OP_FLAG_NO_LAYER_FUSION | OP_FLAG_LAYER_8X16 | OP_FLAG_LAYER_M32)))
    return false;
  return true;
}

// MFMA pipe time per algorithmic product of a kernel set on this handle's path: op_calibrate's order of candidates
inline float set_cost(const SelectState& s, int set) { return s.panel_path ? kKernelSets[set].cost_panel : kKernelSets[set].cost_row; }

// Evaluated policy = requested policy minus the hi x lo(weight) terms whose lo planes are identically zero for this
// checkpoint (bf16 weights: dropping the term changes no bit of the result)
inline Policy evaluated_policy(const SelectState& s) {
  Policy e = s.req;
  if (!s.any_lo[OP_FAM_WQKV]) e.wqkv &= ~OP_TERM_RIGHT_LO;
  if (!s.any_lo[OP_FAM_ATTN_OUT]) e.attn_out &= ~OP_TERM_RIGHT_LO;
  if (!s.any_lo[OP_FAM_WI]) e.wi &= ~OP_TERM_RIGHT_LO;
  if (!s.any_lo[OP_FAM_MLP_OUT]) e.mlp_out &= ~OP_TERM_RIGHT_LO;
  return e;
}

// The default selection for evaluated terms `e`: the kernel set that has exactly those terms -- or -1, the all-terms kernels
// with the unused lo operands cleared.
inline int default_set(const SelectState& s, const Policy& e) {
  // the (hi, lo) bf16 set with exactly these terms (OP_FLAG_NO_POLICY_KERNELS: the all-terms one only)
  int set = -1;
  const int n_bf16_sets = (s.flags & OP_FLAG_NO_POLICY_KERNELS) ? 1 : OP_KS_BF16 + 1;
  for (int k = n_bf16_sets - 1; k >= 0; --k)
    if (kKernelSets[k].terms == e) set = k;
  // bf16-valued weights that are also exact fp16 values, on the whole-layer kernel's shapes: the "f16 + fp8" kernel
  // set evaluates the same terms at 1.5 instead of 2 MFMA units per product (op_policy.h)
  const bool f8_ok = set >= 0 && s.f8_packs && !s.f8_off && !s.f16_unfit &&
                     !(s.flags & (OP_FLAG_NO_POLICY_KERNELS | OP_FLAG_NO_LAYER_FUSION | OP_FLAG_LAYER_8X16 | OP_FLAG_LAYER_M32));
  const bool exact_f16 = !s.not_f16;
  // Panel path (hidden 512 / 768).  The whole layer in the format (OP_FLAG_PANEL_F8) costs 0.45-1.0e-3 on logits at the
  // published depths: opt-in.  The Wi GEMM ALONE -- 52 % of the GEMM FLOPs -- costs 1-1.5e-4 (base / large / en-gte at
  // 19-25 layers: <= 5.4e-4 against the oracle where the (hi, lo) bf16 sets give <= 4.7e-4; scripts/f8_depth_check.py,
  // profiles/r04_f8_depth_check.txt) and takes the fp32-valued Wi GEMM from 3 to 2 MFMA units per product: +5.6 %
  // pairs/s on base -- the DEFAULT for fp32-valued weights.  For bf16-valued weights (2 -> 1.5 units in a GEMM that
  // is not pipe-bound there) it measures +0.7 %: only on request (OP_FLAG_PANEL_F8_WI).
  const bool wi_only = s.panel_path && !(s.flags & OP_FLAG_PANEL_F8);
  // every term requested and carried (fp32-valued weights): the same format with the weights' lo part as a third
  // plane -- one kernel per layer at 2 MFMA units per product instead of two kernels at 3
  if (f8_ok && set == OP_KS_BF16X3) set = wi_only ? OP_KS_BF16X3_WI_F8 : OP_KS_F16_F8_W;
  else if (f8_ok && set == OP_KS_BF16_WEIGHTS && exact_f16 && (!wi_only || (s.flags & OP_FLAG_PANEL_F8_WI)))
    set = wi_only ? OP_KS_BF16_WEIGHTS_WI_F8 : OP_KS_F16_F8;
  return set;
}

// The default selection, or the pinned set.  A kernel set pinned by op_select_kernel_set / chosen by op_calibrate replaces the
// default selection where the handle can run it, and the evaluated terms become the set's own (a set with fewer terms than
// the checkpoint carries is an approximation -- op_calibrate measures it before choosing it).
inline Selection select(const SelectState& s) {
  Selection r;
  r.eff = evaluated_policy(s);
  const bool pinned = s.forced_set >= 0 && set_available(s, s.forced_set);
  r.set = pinned ? s.forced_set : default_set(s, r.eff);
  const KernelSet& ks = set_row(r.set);
  r.mlp_layers = (mlp_by_layer(ks) && r.set == s.forced_set) ? s.forced_mlp_layers : ~0ull;
  if (pinned) r.eff = ks.terms;
  return r;
}

// ---- op_calibrate's search ------------------------------------------------------------------------------------------------------
// max |got - ref|; +inf when the outputs are not finite.  The comparison takes a NaN difference ((NaN <= err) is false) and
// an infinite one stays; but a later finite difference takes a NaN's place again ((d <= NaN) is false too), so a NaN counts only
// from the last finite difference on.  The kernels' range guard writes NaN to every logit; outputs that are NaN in part would
// need `err != err` kept here -- left as it was: this header moved the rule, it did not change it.
inline float max_diff(const std::vector<float>& got, const std::vector<float>& ref) {
  float err = 0.f;
  for (size_t i = 0; i < got.size(); ++i) {
    const float d = std::fabs(got[i] - ref[i]);
    err = (d <= err) ? err : d;
  }
  return std::isfinite(err) ? err : INFINITY;
}

// candidates: every available kernel set cheaper than the default one, cheapest first
inline std::vector<int> calibration_candidates(const SelectState& s, int default_set) {
  std::vector<int> cand;
  for (int set = 0; set < OP_KS_COUNT; ++set)
    if (set != default_set && set_available(s, set) && set_cost(s, set) < set_cost(s, default_set)) cand.push_back(set);
  std::sort(cand.begin(), cand.end(), [&](int a, int b) { return set_cost(s, a) < set_cost(s, b); });
  if (cand.size() > 16) cand.resize(16);
  return cand;
}

inline uint64_t all_layers_mask(int n_layers) { return n_layers >= 64 ? ~0ull : ((1ull << n_layers) - 1ull); }

struct Measurement {
  int rc;     // OP_OK, or the error that ends the search
  float err;  // max_diff to the reference outputs (the reference run itself: +inf when its outputs are not finite, else 0).
              // Turning non-finite outputs into +inf is the measure's part (max_diff); the search reports what it is given and
              // never chooses on a NaN ((NaN <= tolerance) is false)
};

struct SearchResult {
  int rc = OP_OK;
  int chosen = -1;               // the set to pin; -1: the default selection stays
  uint64_t mlp_layers = ~0ull;   // ... and its layer mask (bits beyond n_layers clear)
  float default_err = 0.f;
  int n_candidates = 0;
  int candidate_set[16] = {};
  float candidate_err[16] = {};
  float mlp_layers_err = 0.f;
};

// measure(set, mlp_layers) runs the batch on that set and mask.  The first call is the reference set's.
template <typename Measure>
SearchResult calibration_search(const std::vector<int>& cand, int reference_set, int default_set, float tolerance, unsigned flags,
                                int n_layers, Measure&& measure) {
  SearchResult r;
  const bool full_report = (flags & OP_CAL_FULL_REPORT) != 0;
  const uint64_t all_layers = all_layers_mask(n_layers);
  r.mlp_layers = all_layers;
  Measurement m = measure(reference_set, ~0ull);
  r.rc = m.rc;
  const bool ref_finite = std::isfinite(m.err);
  if (r.rc == OP_OK && ref_finite && default_set != reference_set) {
    m = measure(default_set, ~0ull);
    r.rc = m.rc;
    if (r.rc == OP_OK) r.default_err = m.err;
  }
  if (r.rc == OP_OK && ref_finite) {
    for (size_t c = 0; c < cand.size() && c < 16; ++c) {
      m = measure(cand[c], ~0ull);
      r.rc = m.rc;
      if (r.rc != OP_OK) break;
      r.candidate_set[r.n_candidates] = cand[c];
      r.candidate_err[r.n_candidates] = m.err;
      r.n_candidates += 1;
      if (r.chosen < 0 && m.err <= tolerance) r.chosen = cand[c];
      if (r.chosen >= 0 && !full_report) break;  // cheapest first: the first one that holds is the answer (OP_CAL_FULL_REPORT measures them all)
    }
  }
  // Kernel sets 8 / 9 chosen (the "f16" set alone is beyond the tolerance, the MLP in the fp16 + e4m3 format brings it back):
  // the correction is a per-layer choice (panel_layer): drop it layer by layer for as long as the batch stays within the
  // tolerance.  The error is a maximum over logits, not a sum over layers, so the order of the walk decides how many layers
  // go: three walks (first to last, last to first, and by the price of dropping each layer alone), the one that keeps the
  // fewest layers wins.  About four forwards of the calibration batch per layer, at load.
  if (r.rc == OP_OK && (r.chosen == OP_KS_F16_MLP_F8 || r.chosen == OP_KS_F16_MLP_F8_W) && n_layers <= 64 && !(flags & OP_CAL_WHOLE_DEPTH)) {
    std::vector<std::pair<float, int>> alone;
    for (int li = 0; li < n_layers && r.rc == OP_OK; ++li) {
      m = measure(r.chosen, all_layers & ~(1ull << li));
      r.rc = m.rc;
      if (r.rc == OP_OK) alone.emplace_back(m.err, li);
    }
    std::vector<std::vector<int>> walks(3);
    for (int li = 0; li < n_layers; ++li) {
      walks[0].push_back(li);
      walks[1].push_back(n_layers - 1 - li);
    }
    std::vector<std::pair<float, int>> by_price = alone;
    std::stable_sort(by_price.begin(), by_price.end(), [](const std::pair<float, int>& a, const std::pair<float, int>& b) { return a.first < b.first; });
    for (const auto& pr : by_price) walks[2].push_back(pr.second);
    int best_kept = n_layers + 1;
    for (size_t w = 0; w < walks.size() && r.rc == OP_OK && alone.size() == (size_t)n_layers; ++w) {
      uint64_t mask = all_layers;
      float mask_err = 0.f;
      for (int li : walks[w]) {
        const uint64_t trial = mask & ~(1ull << li);
        if (trial == 0ull) break;  // (= the "f16" set, measured above)
        float err = alone[li].first;
        if (trial != (all_layers & ~(1ull << li))) {
          m = measure(r.chosen, trial);
          r.rc = m.rc;
          if (r.rc != OP_OK) break;
          err = m.err;
        }
        if (err <= tolerance) {
          mask = trial;
          mask_err = err;
        }
      }
      const int kept = __builtin_popcountll(mask);
      if (r.rc == OP_OK && kept < best_kept) {
        best_kept = kept;
        r.mlp_layers = mask;
        r.mlp_layers_err = mask_err;
      }
    }
  }
  // nothing cheaper holds: the default stays -- unless it cannot even represent this batch (fp16 range), or is itself further
  // from the (hi, lo) bf16 kernels than TEN times the tolerance (1e-3 at the default tolerance: the path's own bar; the O(1)
  // worst-case weights put it at 6e-4): a checkpoint with outlier channels at 30 - 100 x puts the fp16 + e4m3 default 4e-2
  // from them (scripts/trained_like_probe.py) -- then the reference set runs, the most exact arithmetic this library has
  if (r.rc == OP_OK && r.chosen < 0 && ref_finite && default_set != reference_set &&
      (!std::isfinite(r.default_err) || r.default_err > 10.0f * tolerance))
    r.chosen = reference_set;
  if (r.rc != OP_OK) r.chosen = -1;
  return r;
}

// ---- a refused argument: the code and the text the caller hands to fail() --------------------------------------------------------
struct Refusal {
  int code = OP_OK;
  char text[224] = "";
};
inline Refusal refuse(int code, const char* fmt, ...) __attribute__((format(printf, 2, 3)));
inline Refusal refuse(int code, const char* fmt, ...) {
  Refusal r;
  r.code = code;
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(r.text, sizeof(r.text), fmt, ap);
  va_end(ap);
  return r;
}

// What every pass over a packed batch relies on: 0 .. total_tokens, monotone, no row beyond max_seqlen or the RoPE tables.
inline Refusal check_cu_seqlens(const int32_t* cu, int n_seqs, int total_tokens, int max_seqlen, int max_pos) {
  if (cu[0] != 0 || cu[n_seqs] != total_tokens)
    return refuse(OP_ERR_INVALID, "cu_seqlens must start at 0 and end at total_tokens (%d): got %d..%d", total_tokens, cu[0], cu[n_seqs]);
  for (int s = 0; s < n_seqs; ++s) {
    const int len = cu[s + 1] - cu[s];
    if (len < 0) return refuse(OP_ERR_INVALID, "cu_seqlens not monotone at %d", s);
    if (len > max_seqlen) return refuse(OP_ERR_INVALID, "sequence %d has %d tokens > max_seqlen %d", s, len, max_seqlen);
    if (len > max_pos) return refuse(OP_ERR_UNSUPPORTED, "sequence %d has %d tokens > max_position_embeddings %d", s, len, max_pos);
  }
  return Refusal{};
}

// op_calibrate's own batch (host ids too; no total_tokens or max_seqlen to hold it to, and at least one token)
inline Refusal check_calibration_batch(const int32_t* ids, const int32_t* cu, int n_seqs, int max_pos, int vocab) {
  if (cu[0] != 0 || cu[n_seqs] <= 0) return refuse(OP_ERR_INVALID, "op_calibrate: cu_seqlens must start at 0 and hold at least one token");
  for (int s = 0; s < n_seqs; ++s) {
    const int len = cu[s + 1] - cu[s];
    if (len < 0 || len > max_pos)
      return refuse(OP_ERR_INVALID, "op_calibrate: row %d has %d tokens (cu_seqlens must not decrease; max_position_embeddings is %d)", s, len, max_pos);
  }
  for (int i = 0; i < cu[n_seqs]; ++i)
    if (ids[i] < 0 || ids[i] >= vocab)
      return refuse(OP_ERR_INVALID, "op_calibrate: token id %d at position %d is outside the embedding table (vocab_size %d)", ids[i], i, vocab);
  return Refusal{};
}

// ---- chunks of a packed batch -----------------------------------------------------------------------------------------------------
// rows the largest chunk can hold (before the +64 slack / 128 rounding); chunk_rows: the handle's, a multiple of ROW_ALIGN
inline int chunk_row_capacity(int chunk_rows, int n_seqs, int total_tokens, int max_seqlen) {
  const long upper = (long)total_tokens + (long)(ROW_ALIGN - 1) * n_seqs;
  const long all_rows = align_up((int)std::min<long>(upper, 1L << 30), ROW_ALIGN);
  const int one_seq = align_up(std::max(max_seqlen, 1), ROW_ALIGN);
  const long cap = std::max(chunk_rows, one_seq);
  return (int)std::min<long>(all_rows, cap);
}
// ... and the rows a workspace is carved for
inline int padded_row_capacity(int chunk_rows, int n_seqs, int total_tokens, int max_seqlen) {
  return align_up(chunk_row_capacity(chunk_rows, n_seqs, total_tokens, max_seqlen) + 64, 256);
}

// The chunk of sequences that starts at s0: as many as fit `cap` rows (at least one) -> one past its last sequence, with
// its rows (every sequence rounded up to ROW_ALIGN) and its longest sequence.
inline int next_chunk(const int32_t* cu, int s0, int n_seqs, int cap, int* rows_out, int* max_len_out) {
  int rows = 0, s1 = s0, max_len = 0;
  while (s1 < n_seqs) {
    const int len = cu[s1 + 1] - cu[s1];
    const int r = align_up(len, ROW_ALIGN);
    if (s1 > s0 && rows + r > cap) break;
    rows += r;
    max_len = std::max(max_len, len);
    ++s1;
  }
  *rows_out = rows;
  *max_len_out = max_len;
  return s1;
}

struct AttnPlan {
  int waves_g;  // waves per block of the full-attention layers (8 or 4); sliding-window layers always use 4
  int items_g;  // work items (sequence, query block) of a full-attention layer
  int items_l;  // ... of a sliding-window layer (128-query blocks)
};

// work items of sequences [s0, s1) at `waves` x 32 queries per block
inline int count_items(const int32_t* cu, int s0, int s1, int waves) {
  int items = 0;
  for (int s = s0; s < s1; ++s) items += (cu[s + 1] - cu[s] + waves * 32 - 1) / (waves * 32);
  return items;
}

// attention work items of the full-attention layers: 256-query blocks (8 waves) once a sequence is longer than
// 128 tokens, else 128 -- unless that leaves CUs idle (small request): then 128-query blocks, twice as many work
// items.  Sliding-window layers always use 128-query blocks.
inline AttnPlan attention_plan(const int32_t* cu, int s0, int s1, int max_len, int n_heads, int n_cus, unsigned flags) {
  const bool forced = (flags & (OP_FLAG_ATT_WAVES_4 | OP_FLAG_ATT_WAVES_8)) != 0;
  AttnPlan plan;
  plan.waves_g = forced ? ((flags & OP_FLAG_ATT_WAVES_4) ? 4 : 8) : (max_len > 128 ? 8 : 4);
  plan.items_g = count_items(cu, s0, s1, plan.waves_g);
  if (!forced && plan.waves_g == 8 && (long)plan.items_g * n_heads <= n_cus) {
    plan.waves_g = 4;
    plan.items_g = count_items(cu, s0, s1, 4);
  }
  plan.items_l = count_items(cu, s0, s1, 4);
  return plan;
}

// ---- workspace layout -------------------------------------------------------------------------------------------------------------
// THE list of a forward's regions, in the order they are handed out: X(name, kind, bytes) with R rows, H hidden, I intermediate,
// S sequences.  workspace_layout() below and the library's carve() are both generated from it, so neither can fall behind.
#define OPP_WORKSPACE_REGIONS(X)          \
  X(x, OP_WS_FLOAT, R * H * 4)            \
  X(ln_hi, OP_WS_FLOAT, R * H * 2)        \
  X(ln_lo, OP_WS_FLOAT, R * H * 2)        \
  X(q_hi, OP_WS_FLOAT, R * H * 2)         \
  X(q_lo, OP_WS_FLOAT, R * H * 2)         \
  X(k_hi, OP_WS_FLOAT, R * H * 2)         \
  X(k_lo, OP_WS_FLOAT, R * H * 2)         \
  X(vt_hi, OP_WS_FLOAT, R * H * 2)        \
  X(vt_lo, OP_WS_FLOAT, R * H * 2)        \
  X(o_hi, OP_WS_FLOAT, R * H * 2)         \
  X(o_lo, OP_WS_FLOAT, R * H * 2)         \
  X(h_hi, OP_WS_FLOAT, R * I * 2)         \
  X(h_lo, OP_WS_FLOAT, R * I * 2)         \
  X(row_seq, OP_WS_INDEX, R * 4)          \
  X(row_pos, OP_WS_INDEX, R * 4)          \
  X(row_tok, OP_WS_INDEX, R * 4)          \
  X(roff, OP_WS_INDEX, (S + 1) * 4)       \
  X(qboff, OP_WS_INDEX, (S + 1) * 4)      \
  X(qboff_l, OP_WS_INDEX, (S + 1) * 4)    \
  X(cls, OP_WS_FLOAT, std::max<size_t>(S, 1) * H * 4) \
  X(range_flag, OP_WS_FLAG, sizeof(int))
// ... and the fp32 planes of kernel set "fp32" behind them (reported as ln_f .. h_f): X(member, bytes)
#define OPP_WORKSPACE_F32_PLANES(X) \
  X(ln, R * H * 4)                  \
  X(q, R * H * 4)                   \
  X(k, R * H * 4)                   \
  X(v, R * H * 4)                   \
  X(o, R * H * 4)                   \
  X(h, R * I * 4)
#define OPP_COUNT_REGION(...) +1
constexpr int N_WORKSPACE_REGIONS = 0 OPP_WORKSPACE_REGIONS(OPP_COUNT_REGION) OPP_WORKSPACE_F32_PLANES(OPP_COUNT_REGION);

struct Region {
  const char* name;
  int kind;  // enum op_workspace_kind
  size_t offset, bytes;
};
struct Layout {
  Region regions[N_WORKSPACE_REGIONS];
  int n = 0;
  size_t bytes = 0;  // the whole workspace: every region rounded up to 256 bytes
};

// The regions of a forward's workspace (op_debug_workspace_layout reports them, carve() takes its pointers from them).  f32: the
// planes of kernel set "fp32" follow the regions every set has (whose offsets therefore never move).
inline Layout workspace_layout(int hidden, int inter, int cap_rows_pad, int n_seqs, bool f32) {
  Layout lay;
  auto take = [&](const char* name, int kind, size_t bytes) {
    lay.regions[lay.n++] = Region{name, kind, lay.bytes, bytes};
    lay.bytes += align_up_sz(bytes, 256);
  };
  const size_t R = (size_t)cap_rows_pad, H = (size_t)hidden, I = (size_t)inter, S = (size_t)n_seqs;
#define OPP_TAKE(name, kind, bytes) take(#name, kind, bytes);
  OPP_WORKSPACE_REGIONS(OPP_TAKE)
#undef OPP_TAKE
  if (f32) {
#define OPP_TAKE_F32(name, bytes) take(#name "_f", OP_WS_FLOAT, bytes);
    OPP_WORKSPACE_F32_PLANES(OPP_TAKE_F32)
#undef OPP_TAKE_F32
  }
  return lay;
}

// ---- op_forward_masked_native: the arguments' own checks and the handle's fitness -----------------------------------------------------
// What op_forward_masked checks before it looks at the handle, in its order and wording under the name `fn`: the report, the
// sizes, the buffers of a non-empty batch.  report_bytes: the caller's op_masked_report.struct_bytes (has_report: it gave one).
inline Refusal check_masked_args(const char* fn, bool has_report, uint32_t report_bytes, int n_rows, int width, bool ids, bool mask,
                                 bool prune, bool rank, bool workspace) {
  if (!has_report) return refuse(OP_ERR_INVALID, "%s: report is NULL", fn);
  if (report_bytes != sizeof(op_masked_report))
    return refuse(OP_ERR_INVALID, "%s: op_masked_report.struct_bytes is %u, expected %zu", fn, report_bytes, sizeof(op_masked_report));
  if (n_rows < 0) return refuse(OP_ERR_INVALID, "%s: negative n_rows %d", fn, n_rows);
  if (width < 0) return refuse(OP_ERR_INVALID, "%s: negative width %d", fn, width);
  const int64_t cells = (int64_t)n_rows * (int64_t)width;
  if (cells > (int64_t)INT32_MAX)  // (tokens and the first offending id are 32-bit linear indices)
    return refuse(OP_ERR_INVALID, "%s: n_rows * width = %lld exceeds 2^31 - 1", fn, (long long)cells);
  if (cells > 0 && !ids) return refuse(OP_ERR_INVALID, "%s: ids_dev is NULL", fn);
  if (cells > 0 && !mask) return refuse(OP_ERR_INVALID, "%s: mask_dev is NULL", fn);
  if (cells > 0 && !prune) return refuse(OP_ERR_INVALID, "%s: prune_logits_dev is NULL", fn);
  if (cells > 0 && !rank) return refuse(OP_ERR_INVALID, "%s: rank_logits_dev is NULL", fn);
  if (cells > 0 && !workspace) return refuse(OP_ERR_INVALID, "%s: workspace_dev is NULL", fn);
  return Refusal{};
}

// ... and what it asks of the handle, once there is one: the width within the RoPE tables, the key-mask kernels' paths (row or
// panel), a selected set that is not "fp32" (whose masked forward op_forward_masked is).
inline Refusal check_masked_native_handle(int width, int max_pos, bool row_path, bool panel_path, int set) {
  const char* const fn = "op_forward_masked_native";
  if (width > max_pos) return refuse(OP_ERR_INVALID, "%s: width %d exceeds max_position_embeddings %d", fn, width, max_pos);
  if (!row_path && !panel_path)
    return refuse(OP_ERR_UNSUPPORTED, "%s: the handle runs the tiled path, which has no key-mask attention kernel: use op_forward_masked (the fp32 kernels)", fn);
  if (set == OP_KS_F32)
    return refuse(OP_ERR_UNSUPPORTED, "%s: the selected kernel set is \"fp32\": op_forward_masked is this handle's masked forward", fn);
  return Refusal{};
}

// The call's own workspace: the dense cu_seqlens, the id check's word, the mask in the row layout, the row means of v, then the
// selected set's forward workspace -- offsets from the 256-aligned base, each region rounded up to 256 bytes.
struct MaskedNativeLayout {
  size_t cu, status, key_row, vmean, forward, bytes;
};
inline MaskedNativeLayout masked_native_layout(int hidden, int chunk_rows, int n_rows, int width, size_t forward_bytes) {
  MaskedNativeLayout l{};
  size_t off = 0;
  auto take = [&](size_t bytes) {
    const size_t at = off;
    off += align_up_sz(bytes, 256);
    return at;
  };
  l.cu = take(((size_t)n_rows + 1) * 4);
  l.status = take(sizeof(uint32_t));
  l.key_row = take((size_t)padded_row_capacity(chunk_rows, n_rows, n_rows * width, width));
  l.vmean = take((size_t)n_rows * (size_t)hidden * sizeof(float));
  l.forward = take(forward_bytes);
  l.bytes = off;
  return l;
}

// ---- prepared requests: fragment means and sentence decisions (op_planned_fragment_means, op_located_fragment_means,
// op_sentence_decisions) ----------------------------------------------------------------------------------------------------------
// All look at the caller's HOST copies only, before anything is enqueued and before the handle is looked at.

// `rows` is the op_assemble_request of the forward (its plan, offsets and cu_seqlens; the ids it names are not needed here).
// (`fn`: the call the refusal's text names -- op_located_fragment_means makes the same checks)
inline Refusal check_planned_means(const op_assemble_request* rows, const op_planned_means_request* req,
                                   const char* fn = "op_planned_fragment_means") {
  if (!rows || !req) return refuse(OP_ERR_INVALID, "%s: %s is NULL", fn, !rows ? "rows" : "request");
  if (rows->struct_bytes != sizeof(op_assemble_request))
    return refuse(OP_ERR_INVALID, "%s: op_assemble_request.struct_bytes is %u, expected %zu", fn, rows->struct_bytes, sizeof(op_assemble_request));
  if (req->struct_bytes != sizeof(op_planned_means_request))
    return refuse(OP_ERR_INVALID, "%s: op_planned_means_request.struct_bytes is %u, expected %zu", fn, req->struct_bytes,
                  sizeof(op_planned_means_request));
  if (rows->n_frag < 0 || rows->n_queries < 0 || rows->n_rows < 0 || rows->total_tokens < 0 || req->n_slots < 0 || rows->n_prefix < 0 ||
      rows->n_middle < 0 || rows->n_prefix > OP_ASSEMBLE_MAX_PIECE || rows->n_middle > OP_ASSEMBLE_MAX_PIECE)
    return refuse(OP_ERR_INVALID, "%s: negative count (n_frag %d, n_queries %d, n_rows %d, total_tokens %d, n_slots %d) or template piece (%d, %d)",
                  fn, rows->n_frag, rows->n_queries, rows->n_rows, rows->total_tokens, req->n_slots, rows->n_prefix, rows->n_middle);
  if (rows->n_rows == 0) return Refusal{};
  if (!rows->plan_dev || !rows->plan_host || !rows->cu_seqlens_dev || !rows->cu_seqlens_host || !rows->q_off_dev || !rows->q_off_host ||
      !rows->frag_off_dev || !rows->frag_off_host || !req->slot_off_dev || !req->slot_off_host || !req->frag_shift_dev)
    return refuse(OP_ERR_INVALID, "%s: a plan, cu_seqlens, offset, slot_off or frag_shift buffer is NULL", fn);
  if (rows->q_off_host[0] != 0 || rows->frag_off_host[0] != 0) return refuse(OP_ERR_INVALID, "%s: offsets do not start at 0", fn);
  for (int q = 0; q < rows->n_queries; ++q)
    if (rows->q_off_host[q + 1] < rows->q_off_host[q]) return refuse(OP_ERR_INVALID, "%s: q_off decreases at query %d", fn, q);
  const int n_corpus = rows->frag_off_host[rows->n_frag];
  if (n_corpus < 0) return refuse(OP_ERR_INVALID, "%s: frag_off ends at %d", fn, n_corpus);
  if (rows->cu_seqlens_host[0] != 0 || rows->cu_seqlens_host[rows->n_rows] != rows->total_tokens)
    return refuse(OP_ERR_INVALID, "%s: cu_seqlens_host runs from %d to %d, expected 0 to total_tokens (%d)", fn, rows->cu_seqlens_host[0],
                  rows->cu_seqlens_host[rows->n_rows], rows->total_tokens);
  if (req->slot_off_host[0] < 0) return refuse(OP_ERR_INVALID, "%s: slot_off_host[0] is %d", fn, req->slot_off_host[0]);
  int64_t slot = req->slot_off_host[0];
  for (int r = 0; r < rows->n_rows; ++r) {
    const int32_t* pr = rows->plan_host + (size_t)r * 4;
    const int query = pr[0], first = pr[1], n = pr[2], clip = pr[3];
    if (rows->cu_seqlens_host[r + 1] < rows->cu_seqlens_host[r]) return refuse(OP_ERR_INVALID, "%s: cu_seqlens_host decreases at row %d", fn, r);
    if (query < 0 || query >= rows->n_queries) return refuse(OP_ERR_INVALID, "%s: row %d names query %d of %d", fn, r, query, rows->n_queries);
    if (first < 0 || n < 0 || first > rows->n_frag - n)
      return refuse(OP_ERR_INVALID, "%s: row %d takes fragments %d .. %d + %d of %d", fn, r, first, first, n, rows->n_frag);
    if (n > 0) {
      const int32_t* fo = rows->frag_off_host + first;
      if (fo[0] < 0 || fo[1] < fo[0] || fo[n] < fo[1] || fo[n] > n_corpus)
        return refuse(OP_ERR_INVALID, "%s: frag_off decreases or leaves the corpus at row %d", fn, r);
      if (clip < 0 || clip > fo[1] - fo[0])
        return refuse(OP_ERR_INVALID, "%s: row %d clips its first fragment of %d ids to %d", fn, r, fo[1] - fo[0], clip);
    }
    slot += n;
    if (slot > (int64_t)req->n_slots || (int64_t)req->slot_off_host[r + 1] != slot)
      return refuse(OP_ERR_INVALID, "%s: slot_off_host[%d] is %d, the plan's fragments end at %lld of %d slots", fn, r + 1,
                    req->slot_off_host[r + 1], (long long)slot, req->n_slots);
  }
  if (rows->total_tokens > 0 && !req->keep_prob_dev) return refuse(OP_ERR_INVALID, "%s: keep_prob_dev is NULL", fn);
  if (slot > (int64_t)req->slot_off_host[0] && (!req->mean_out_dev || !req->slot_frag_out_dev))
    return refuse(OP_ERR_INVALID, "%s: mean_out_dev or slot_frag_out_dev is NULL", fn);
  return Refusal{};
}

// op_located_fragment_means: everything check_planned_means checks, and the two buffers of the lookup -- the rows' ids
// (op_assemble_rows' output for the same `rows`) and one ctx_start per row -- while there are rows.
inline Refusal check_located_means(const op_assemble_request* rows, const op_planned_means_request* req, const int32_t* ids_dev,
                                   const int32_t* ctx_start_out_dev) {
  const char* const fn = "op_located_fragment_means";
  const Refusal planned = check_planned_means(rows, req, fn);
  if (planned.code != OP_OK) return planned;
  if (rows->n_rows > 0 && !ctx_start_out_dev) return refuse(OP_ERR_INVALID, "%s: ctx_start_out_dev is NULL", fn);
  if (rows->n_rows > 0 && !ids_dev) return refuse(OP_ERR_INVALID, "%s: ids_dev is NULL", fn);
  return Refusal{};
}

inline Refusal check_decisions(const op_decisions_request* req) {
  const char* const fn = "op_sentence_decisions";
  if (!req) return refuse(OP_ERR_INVALID, "%s: request is NULL", fn);
  if (req->struct_bytes != sizeof(op_decisions_request))
    return refuse(OP_ERR_INVALID, "%s: op_decisions_request.struct_bytes is %u, expected %zu", fn, req->struct_bytes, sizeof(op_decisions_request));
  if (req->n_instances < 0 || req->n_slots < 0 || req->n_frag < 0 || req->n_out < 0)
    return refuse(OP_ERR_INVALID, "%s: negative count (n_instances %d, n_slots %d, n_frag %d, n_out %d)", fn, req->n_instances, req->n_slots,
                  req->n_frag, req->n_out);
  if (req->n_instances > 0 && (!req->instances_dev || !req->instances_host)) return refuse(OP_ERR_INVALID, "%s: instances buffer is NULL", fn);
  if (req->n_slots > 0 && (!req->mean_dev || !req->slot_frag_dev)) return refuse(OP_ERR_INVALID, "%s: mean_dev or slot_frag_dev is NULL", fn);
  if (req->n_frag > 0 && !req->frag_sent_dev) return refuse(OP_ERR_INVALID, "%s: frag_sent_dev is NULL", fn);
  if (req->n_out > 0 && (!req->avg_out_dev || !req->keep_out_dev)) return refuse(OP_ERR_INVALID, "%s: avg_out_dev or keep_out_dev is NULL", fn);
  int64_t out = 0;
  for (int i = 0; i < req->n_instances; ++i) {
    const int32_t* in = req->instances_host + (size_t)i * OP_DECISIONS_INSTANCE_WORDS;
    const int slot_begin = in[0], slot_end = in[1], out_begin = in[2], n_sent = in[3], sent_base = in[4], title = in[5];
    if (slot_begin < 0 || slot_end < slot_begin || slot_end > req->n_slots)
      return refuse(OP_ERR_INVALID, "%s: instance %d takes slots %d .. %d of %d", fn, i, slot_begin, slot_end, req->n_slots);
    if (n_sent < 0 || (int64_t)out_begin != out || out + n_sent > (int64_t)req->n_out)
      return refuse(OP_ERR_INVALID, "%s: instance %d writes sentences %d .. %d + %d, the previous one ended at %lld of %d", fn, i, out_begin,
                    out_begin, n_sent, (long long)out, req->n_out);
    if (sent_base < 0) return refuse(OP_ERR_INVALID, "%s: instance %d has item_sent_base %d", fn, i, sent_base);
    if (title < -1 || title >= n_sent)
      return refuse(OP_ERR_INVALID, "%s: instance %d has title_index %d outside [-1, %d)", fn, i, title, n_sent);
    out += n_sent;
  }
  if (out != (int64_t)req->n_out)
    return refuse(OP_ERR_INVALID, "%s: the instances hold %lld sentences, n_out is %d", fn, (long long)out, req->n_out);
  return Refusal{};
}

}  // namespace opp
