// op_api.hip -- C ABI of libopenprovence_hip.so (see include/open_provence_hip.h for the contract and
// the reference interfaces each entry point replaces).  Host side only: handle, weight re-packing,
// workspace carving, chunking of the packed batch and the launch sequence of one forward.
#include "../../include/open_provence_hip.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#define OPK_PACK_KERNELS 1
#include "op_internal.h"
#include "op_plan.h"
#include "op_sets.h"
#include "opk_small.hip.h"
#include "opk_pool.hip.h"
#include "opk_loss.hip.h"
#include "opk_padded.hip.h"
#include "opk_tiled.hip.h"

using namespace opk;
using opl::Policy;
using namespace ops;
using opp::AttnPlan;
using opp::align_up;
using opp::align_up_sz;

static_assert(opp::ROW_ALIGN == opk::ROW_ALIGN, "op_plan.h chunks a batch by the kernels' row alignment");

namespace {

thread_local std::string g_last_error;

enum ProfileKind {
  PK_ROWMAP = 0,
  PK_EMBED_LN,
  PK_LN,
  PK_GEMM_QK_ROPE,
  PK_GEMM_V_T,
  PK_ATTN_GLOBAL,
  PK_ATTN_LOCAL,
  PK_GEMM_ATTN_OUT,
  PK_GEMM_WI_GEGLU,
  PK_GEMM_MLP_OUT,
  PK_FINAL_LN_PRUNE,
  PK_RANK_HEAD,
  PK_CAPTURE,
  PK_ROW_QKV,
  PK_ROW_ATTN_OUT,
  PK_ROW_WI_GEGLU,
  PK_KSTREAM_MLP_OUT,
  PK_FUSED_ATTN_OUT_WI,
  PK_FUSED_MLP_OUT_QKV,
  PK_CLEAR_LO,
  PK_FUSED_LAYER,
  PK_GEMM_QKV_ROPE,
  PK_COUNT
};
const char* kProfileNames[PK_COUNT] = {"rowmap",        "embed_ln",      "layer_norm",    "gemm_qk_rope", "gemm_v_t",
                                       "attn_global",   "attn_local",    "gemm_attn_out", "gemm_wi_geglu",
                                       "gemm_mlp_out",  "final_ln_prune", "rank_head",    "capture",
                                       "rowgemm_ln_qkv_rope", "rowgemm_attn_out", "rowgemm_ln_wi_geglu",
                                       "kstream_mlp_out", "fused_attnout_ln_wi_geglu", "fused_mlpout_ln_qkv_rope",
                                       "clear_lo_planes", "fused_layer_attnout_mlp_qkv", "gemm_qkv_rope"};

struct LayerWeights {
  float* attn_norm = nullptr;  // absent on layer 0
  float* mlp_norm = nullptr;
  u16* pack[W_COUNT][PF_COUNT] = {};  // the GEMM weights in every format the handle builds (op_sets.h), nullptr: no such pack
};

struct ProfileEvent {
  int kind;
  hipEvent_t start, stop;
};

}  // namespace

struct op_handle {
  op_config cfg;
  int H = 0, I = 0, N = 0, nh = 0, V = 0, nl = 0, max_pos = 0;
  Policy req = opl::kPolicies[0];  // requested term masks (op_config.precision / terms)
  Policy eff = opl::kPolicies[0];  // evaluated term masks: req minus weight-lo terms that are identically zero
  int set = -1;                    // the kernel set that runs (op_kernel_set numbering); -1: `eff` is no set's, all-terms kernels with the unused lo operands cleared
  const KernelSet* ks = &kClearedOperands;  // its row of kKernelSets
  bool resolved = false;           // eff / set / ks / mlp_layers are valid (set by op_weights_ready)
  float* f16_fit_dev = nullptr;    // [2] lost / total weight energy of the tensor being packed for the "f16 + fp8" sets
  int* any_lo_dev = nullptr;       // [OP_FAM_COUNT] device flags: some weight of the family has a non-zero lo element
                                   // [OP_FAM_COUNT]: some GEMM weight is not exactly an fp16 value (no "f16 + fp8" set)
  bool f8_packs = false;           // the "f16 + fp8" weight packs exist (row path, hidden a multiple of 128)
  bool f8_off = false;             // op_set_compact_operands(h, 0): keep the (hi, lo) bf16 sets although the packs exist
  bool h16_packs = false;          // the fp16 single-plane weight packs of kernel set "f16" exist
  bool f32_packs = false;          // OP_FLAG_F32_PACKS: the row-major fp32 weight packs of kernel set "fp32" exist
  int forced_set = -1;             // op_select_kernel_set / op_calibrate: run this kernel set (op_kernel_set numbering), -1 = the default selection
  bool f16_unfit = false;          // some weight TENSOR sits on fp16's subnormal grid: no kernel set with an fp16 weight plane
  uint64_t mlp_layers = ~0ull;     // sets 8 / 9: the layers whose MLP runs in that format (bit li); the others run the "f16" set's MLP
  uint64_t forced_mlp_layers = ~0ull;  // ... as pinned with forced_set (op_calibrate's per-layer search, op_select_mlp_correction_layers)
  bool row_path = false;    // hidden <= 256: row-stationary GEMMs with fused LayerNorm
  bool panel_path = false;  // hidden % 256 == 0, intermediate % 128 == 0: k-streamed panel GEMMs, fragment-packed operands
  int n_cus = 256;          // compute units of the device (hipDeviceProp multiProcessorCount)
  int chunk_rows = 0;
  float* emb = nullptr;
  float* emb_norm = nullptr;
  float* final_norm = nullptr;
  float* dense_t = nullptr;
  float* head_norm = nullptr;
  float* cls_w = nullptr;
  float* cls_b = nullptr;
  float* prune_w = nullptr;
  float* prune_b = nullptr;
  float* rope_cos[2] = {nullptr, nullptr};  // [0] = local theta, [1] = global theta
  float* rope_sin[2] = {nullptr, nullptr};
  std::vector<LayerWeights> layers;
  std::vector<void*> allocations;
  std::vector<std::string> missing;  // weight names not loaded yet
  float* capture = nullptr;
  bool profiling = false;
  std::vector<ProfileEvent> events;
  double prof_ms[PK_COUNT] = {0};
  int prof_launches[PK_COUNT] = {0};
  uint32_t* pad_status = nullptr;    // op_pack_padded: the device status block (opk::PAD_ST_WORDS words), allocated on first use
  int32_t* pad_host = nullptr;       // ... and its pinned host staging: cu_seqlens[n_rows + 1] + the status block
  size_t pad_host_words = 0;
  opk::LossScratch* loss_scratch = nullptr;  // op_loss: the per-block partials and the result block
  opk::LossResult* loss_host = nullptr;      // ... and the result's pinned host staging, allocated by the first call with a report
  // the running audit's coverage (op_coverage_scan / op_coverage_commit): a bitmap of vocab_size bits + opl::COV_WORDS state words
  uint32_t* cov_bits = nullptr;
  uint32_t* cov_state = nullptr;
  uint32_t* cov_host = nullptr;      // pinned staging of the state block, allocated on first use
  bool cov_clear = true;             // clear bitmap and state on the stream of the next scan / commit (nothing audited yet)
  int cov_set = -2;                  // the arithmetic the coverage was collected under: kernel set (public numbering) ...
  uint64_t cov_mlp_layers = 0;       // ... and the layer mask of sets 8 / 9; another one at the next scan / commit clears too
  std::string err;
};

namespace {

int fail(op_handle* h, int code, const char* fmt, ...) {
  char buf[1024];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  if (h) h->err = buf;
  g_last_error = buf;
  return code;
}

int fail(op_handle* h, const opp::Refusal& r) { return fail(h, r.code, "%s", r.text); }

#define OP_HIP(h, expr)                                                                              \
  do {                                                                                               \
    hipError_t _e = (expr);                                                                          \
    if (_e != hipSuccess) return fail(h, OP_ERR_HIP, "%s failed: %s", #expr, hipGetErrorString(_e)); \
  } while (0)

template <typename T>
int dev_alloc(op_handle* h, T** out, size_t count) {
  void* p = nullptr;
  hipError_t e = hipMalloc(&p, std::max<size_t>(count, 1) * sizeof(T));
  if (e != hipSuccess) return fail(h, OP_ERR_NOMEM, "hipMalloc(%zu bytes) failed: %s", count * sizeof(T), hipGetErrorString(e));
  h->allocations.push_back(p);
  *out = reinterpret_cast<T*>(p);
  return OP_OK;
}


void erase_missing(op_handle* h, const std::string& name) {
  auto it = std::find(h->missing.begin(), h->missing.end(), name);
  if (it != h->missing.end()) h->missing.erase(it);
}

// RoPE tables by HF's recipe (modeling_modernbert.py:117-163), reproduced to the bit in inv_freq: HF computes
// 1.0 / (theta ** (arange(0, 64, 2, fp32) / 64)) in fp32, which rounds TWICE -- an fp32 power, then an fp32 reciprocal.  The
// power is taken in double and rounded to fp32 (torch's fp32 pow agrees with the correctly rounded one on all 32 exponents at
// theta 10000 and 160000), then divided in fp32.  Rounding once, (float)(1.0 / pow(theta, e)), is one ulp off in 10 / 8 of the
// 32 entries at those thetas, and the angle's error grows with the position: 1.2e-4 in the table at position 8191.
// angle = fp32(pos) * inv_freq in fp32; cos / sin of that fp32 angle, correctly rounded (torch's cosf is within 6e-8 of it).
// tests/test_rope_tables.py holds the tables to torch's within 2^-23 through op_debug_rope_tables.
void build_rope_host(float theta, int max_pos, std::vector<float>& cs, std::vector<float>& sn) {
  cs.resize((size_t)max_pos * ROPE_HALF);
  sn.resize((size_t)max_pos * ROPE_HALF);
  float inv_freq[ROPE_HALF];
  for (int k = 0; k < ROPE_HALF; ++k) {
    const float expo = (float)(2 * k) / (float)HEAD_DIM;
    inv_freq[k] = 1.0f / (float)std::pow((double)theta, (double)expo);
  }
  for (int p = 0; p < max_pos; ++p) {
    for (int k = 0; k < ROPE_HALF; ++k) {
      const float ang = (float)p * inv_freq[k];
      cs[(size_t)p * ROPE_HALF + k] = (float)std::cos((double)ang);
      sn[(size_t)p * ROPE_HALF + k] = (float)std::sin((double)ang);
    }
  }
}

struct Launcher {
  op_handle* h;
  hipStream_t stream;
  int begin(int kind) {
    if (!h->profiling) return OP_OK;
    ProfileEvent ev;
    ev.kind = kind;
    OP_HIP(h, hipEventCreate(&ev.start));
    OP_HIP(h, hipEventCreate(&ev.stop));
    OP_HIP(h, hipEventRecord(ev.start, stream));
    h->events.push_back(ev);
    return OP_OK;
  }
  int end() {
    OP_HIP(h, hipGetLastError());
    if (!h->profiling) return OP_OK;
    OP_HIP(h, hipEventRecord(h->events.back().stop, stream));
    return OP_OK;
  }
};

#define OP_TRY(expr)             \
  do {                           \
    int _rc = (expr);            \
    if (_rc != OP_OK) return _rc; \
  } while (0)

int drain_profile(op_handle* h) {
  for (auto& ev : h->events) {
    OP_HIP(h, hipEventSynchronize(ev.stop));
    float ms = 0.f;
    OP_HIP(h, hipEventElapsedTime(&ms, ev.start, ev.stop));
    h->prof_ms[ev.kind] += ms;
    h->prof_launches[ev.kind] += 1;
    (void)hipEventDestroy(ev.start);
    (void)hipEventDestroy(ev.stop);
  }
  h->events.clear();
  return OP_OK;
}

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

// the rows a workspace of this geometry is carved for (op_workspace_bytes, op_forward_packed and the attention side passes)
int chunk_row_capacity(const op_handle* h, int n_seqs, int total_tokens, int max_seqlen) {
  return opp::chunk_row_capacity(h->chunk_rows, n_seqs, total_tokens, max_seqlen);
}

// the regions of a forward's workspace for a batch of this geometry; f32: with the planes of kernel set "fp32"
opp::Layout forward_layout(const op_handle* h, int n_seqs, int total_tokens, int max_seqlen, bool f32) {
  return opp::workspace_layout(h->H, h->I, opp::padded_row_capacity(h->chunk_rows, n_seqs, total_tokens, max_seqlen), n_seqs, f32);
}

// The workspace's pointers from its layout, region by region: generated from the same list as the layout (op_plan.h).
void carve(const opp::Layout& lay, char* base, Workspace& ws) {
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

template <int EPI>
int launch_gemm(Launcher& L, int kind, const GemmParams& p, bool split) {
  OP_TRY(L.begin(kind));
  const dim3 grid((unsigned)(p.n_tiles * p.m_tiles));
  if (split)
    hipLaunchKernelGGL((gemm_kernel<EPI, true>), grid, dim3(256), 0, L.stream, p);
  else
    hipLaunchKernelGGL((gemm_kernel<EPI, false>), grid, dim3(256), 0, L.stream, p);
  return L.end();
}

// Clear the lo plane of a fragment-packed tensor: a policy without that operand's lo term, evaluated on the
// all-terms kernel set (the extra MFMA pass then adds exact zeros).
int clear_lo(Launcher& L, u16* base, int unit, size_t n_pairs) {
  OP_TRY(L.begin(PK_CLEAR_LO));
  const size_t n = n_pairs * (size_t)(unit / 8);
  hipLaunchKernelGGL(zero_odd_units_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, L.stream, base, unit, n_pairs);
  return L.end();
}

// A validated per-call hidden-state request (op_forward_packed_hidden): the output slot of every entry (-1: not selected);
// and / or a validated pooled request (op_forward_packed_pooled): an entry it selects is stored into `scratch` (packed fp32
// [total_tokens][H], one entry, reused by the next: the stream orders it), pooled from there, and copied from there into the
// ordinary request's entry when that selects it too (the stores have one destination per launch).
struct HiddenReq {
  char* out = nullptr;
  int bf16 = 0, pad = 0;
  size_t entry_bytes = 0;  // one entry: [total_tokens][H] or [n_seqs][pad][H] elements of the dtype
  std::vector<int> slot;   // [num_layers + 1]
  int pool_kind = 0;       // opk::POOL_FIRST / POOL_MEAN
  float* pool_out = nullptr;  // [n_pool_sel][n_seqs][H]
  float* scratch = nullptr;
  int n_seqs = 0, n_pool = 0;  // sequences of the batch, entries the pooled request selects
  std::vector<int> pool_slot;  // [num_layers + 1], empty: no pooled request
  bool pooled(int index) const { return !pool_slot.empty() && pool_slot[index] >= 0; }
  bool full(int index) const { return !slot.empty() && slot[index] >= 0; }
};

// A packed batch as an entry point receives it, filled once there and passed down by reference.  Calls that take only part
// of it (the attention side passes: no ids, no outputs) leave the rest null.
struct PackedBatch {
  const int32_t* ids_dev = nullptr;
  const int32_t* cu_dev = nullptr;
  const int32_t* cu_host = nullptr;  // the caller's host copy of cu_dev, or NULL: read back (host_cu_seqlens)
  int n_seqs = 0, total_tokens = 0, max_seqlen = 0;
  float *prune_out = nullptr, *rank_out = nullptr, *keep_prob = nullptr;
  void* workspace = nullptr;
  size_t workspace_bytes = 0;
  hipStream_t stream = nullptr;
};

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
            const AttnPlan& plan_, const HiddenReq* hid_)
      : h(h_), L(L_), ws(ws_), b(b_), s0(s0_), ns(ns_), rows(rows_), max_len(max_len_), plan(plan_), hid(hid_) {
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
    const KernelSet& ks = *h->ks;
    E = h->eff;
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

  // the pack of a GEMM weight of layer `li` in the format the constructor decided
  u16* weight(int li, Weight w, PackFmt f) const { return h->layers[li].pack[w][f]; }

  // row map, the range flag, padding rows of the attention output, embeddings
  int prologue() {
    OP_TRY(L.begin(PK_ROWMAP));
    hipLaunchKernelGGL(seq_offsets_kernel, dim3(1), dim3(1024), 0, st, b.cu_dev, s0, ns, ROW_ALIGN, ROW_ALIGN, ws.roff);
    if (fp_layout) {
      hipLaunchKernelGGL(seq_offsets_kernel, dim3(1), dim3(1024), 0, st, b.cu_dev, s0, ns, plan.waves_g * 32, 1, ws.qboff);
      hipLaunchKernelGGL(seq_offsets_kernel, dim3(1), dim3(1024), 0, st, b.cu_dev, s0, ns, 128, 1, ws.qboff_l);
    }
    hipLaunchKernelGGL(row_map_kernel, dim3((unsigned)((r_pad + 255) / 256)), dim3(256), 0, st, b.cu_dev, s0, ns, ws.roff,
                       r_pad, ws.row_seq, ws.row_pos, ws.row_tok);
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

  int capture(int index) {
    if (!h->capture) return OP_OK;
    OP_TRY(L.begin(PK_CAPTURE));
    hipLaunchKernelGGL(capture_rows_kernel, dim3(row_blocks), dim3(256), 0, st, ws.x, ws.row_tok, H, r_pad,
                       h->capture + (size_t)index * b.total_tokens * H);
    return L.end();
  }

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
  int hidden_pooled(int index) {
    if (!hid || !hid->pooled(index)) return OP_OK;
    OP_TRY(L.begin(PK_CAPTURE));
    hipLaunchKernelGGL(pool_hidden_kernel, dim3((unsigned)ns, (unsigned)((H + POOL_COLS - 1) / POOL_COLS)), dim3(256), 0, st, hid->scratch,
                       b.cu_dev, s0, b.total_tokens, H, hid->pool_kind, hid->pool_out + (size_t)hid->pool_slot[index] * (size_t)hid->n_seqs * H);
    if (hid->full(index))
      hipLaunchKernelGGL(hidden_repack_kernel, dim3(row_blocks), dim3(256), 0, st, hid->scratch, H, r_pad, ws.row_tok, ws.row_seq,
                         ws.row_pos, s0, hid->pad, hid->bf16, hid->out + (size_t)hid->slot[index] * hid->entry_bytes);
    return L.end();
  }
  int hidden(int index, const float* ln = nullptr) {
    void* dst = hidden_entry(index);
    if (!dst) return OP_OK;
    OP_TRY(L.begin(PK_CAPTURE));
    hipLaunchKernelGGL(hidden_rows_kernel, dim3(row_blocks), dim3(256), 0, st, ws.x, ln, h->cfg.norm_eps, H, r_pad,
                       ws.row_tok, ws.row_seq, ws.row_pos, s0, hidden_pad(index), hidden_bf16(index), dst);
    OP_TRY(L.end());
    return hidden_pooled(index);
  }

  int attention(bool is_global) {
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
      if (!opl::launch_attn(st, ap, is_global ? plan.waves_g : 4, is_global ? 2 : 1, pi, zero_p_lo, grid, attn16))
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
  int clear_qkv() {
    if (clr_q) OP_TRY(clear_lo(L, ws.q_hi, 512, (size_t)(r_pad / 16) * (H / 32)));
    if (clr_k) OP_TRY(clear_lo(L, ws.k_hi, 512, (size_t)(r_pad / 16) * (H / 32)));
    if (clr_v) OP_TRY(clear_lo(L, ws.vt_hi, 2048, (size_t)h->nh * (r_pad / 32)));
    return OP_OK;
  }
  int clear_h() {
    if (clr_h) OP_TRY(clear_lo(L, ws.h_hi, 512, (size_t)(r_pad / 16) * (I / 32)));
    return OP_OK;
  }

  // parameters of a q/k/v projection of layer `li` (row-stationary kernels)
  RowGemmParams qkv_params(int li) {
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
  int row_layer(int li) {
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
  int panel_layer(int li) {
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
  int tiled_layer(int li) {
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
  int f32_layer(int li) {
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
    opl::launch_f32_attn(st, ap, dim3((unsigned)q_tiles, (unsigned)h->nh, (unsigned)ns));
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

  // final_norm + pruning head (unless the last whole-layer launch did it), ranking head
  int heads() {
    const int mean_pool = h->cfg.pooling == OP_POOL_MEAN ? 1 : 0;
    if (head_done) OP_TRY(hidden_pooled(h->N));  // (entry N came from the last whole-layer launch's epilogue)
    if (!head_done) {
      // (before final_ln_prune_kernel: under mean pooling it writes the normalised rows over x)
      OP_TRY(hidden(h->N, h->cfg.prune_pre_final_norm ? nullptr : h->final_norm));
      OP_TRY(L.begin(PK_FINAL_LN_PRUNE));
      hipLaunchKernelGGL(final_ln_prune_kernel, dim3(row_blocks), dim3(256), 0, st, ws.x, h->final_norm, h->cfg.norm_eps, H,
                         r_pad, ws.row_tok, ws.row_seq, ws.row_pos, h->prune_w, h->prune_b, b.prune_out, b.keep_prob,
                         h->cfg.prune_pre_final_norm ? 1 : 0, mean_pool, ws.cls,
                         h->capture ? h->capture + (size_t)h->N * b.total_tokens * H : nullptr,
                         range_flagged ? ws.range_flag : nullptr);
      OP_TRY(L.end());
    }
    OP_TRY(L.begin(PK_RANK_HEAD));
    if (f32)
      opl::launch_f32_rank_head(st, ns, ws.cls, ws.x, b.cu_dev, s0, ws.roff, mean_pool, H, h->nl, h->dense_t, h->head_norm, h->cfg.norm_eps,
                                h->cls_w, h->cls_b, b.rank_out);
    else
      hipLaunchKernelGGL(rank_head_kernel, dim3((unsigned)ns), dim3(256), 0, st, ws.cls, ws.x, b.cu_dev, s0, ws.roff, mean_pool,
                       H, h->nl, h->dense_t, h->head_norm, h->cfg.norm_eps, h->cls_w, h->cls_b, b.rank_out,
                       range_flagged ? ws.range_flag : nullptr);
    OP_TRY(L.end());
    return OP_OK;
  }

  int run() {
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
};


// Every packed form of one GEMM weight tensor (op_load_weight), on the null stream: one method per packing kernel.
struct WeightPacker {
  op_handle* h;
  const WeightDesc& wd;
  const float* f32;  // the tensor as fp32 [d0][d1]
  int d0, d1;
  // A requested policy without the hi x lo(weight) term stores zeros in the lo plane (so that any kernel set gives
  // that policy's numerics); `any_lo` records whether the tensor had a non-zero lo element at all.
  int zero_lo;
  int* any_lo;

  size_t count() const { return (size_t)d0 * d1; }
  dim3 grid(size_t n) const { return dim3((unsigned)((n + 255) / 256)); }
  // the fp16 + e4m3 packs raise this flag (any_lo_dev[OP_FAM_COUNT]) for a weight they cannot hold exactly
  int* not_f16() const { return h->any_lo_dev + OP_FAM_COUNT; }

  // panel-major: [panel][k-step][plane][16 fragments][512], rows permuted per consumer (panel_source_row); f16: fp16 values
  void panels(u16* dst, int f16) const {
    int tile0 = 0;
    for (const PanelSeg& sg : wd.panel) {
      const int n_tiles = (sg.th * h->H + sg.ti * h->I) / 256;
      if (n_tiles)
        hipLaunchKernelGGL(pack_panel_kernel, grid((size_t)n_tiles * 256 * d1), dim3(256), 0, 0, f32, n_tiles, d1, sg.epi, h->H, h->I,
                           dst + (size_t)tile0 * 256 * d1 * 2, f16 ? 1 : zero_lo, any_lo, f16);
      tile0 += n_tiles;
    }
  }
  // the fp16 slabs + e4m3 slabs of the same panels
  void panels_f8(u16* dst16, u16* dst8) const {
    const size_t lo_off = count();  // bytes of the whole tensor's e4m3(w) slabs: the lo(w) slabs follow
    int tile0 = 0;
    for (const PanelSeg& sg : wd.panel) {
      const int n_tiles = (sg.th * h->H + sg.ti * h->I) / 256;
      if (n_tiles)
        hipLaunchKernelGGL(pack_panel_f8_kernel, grid((size_t)n_tiles * 256 * d1), dim3(256), 0, 0, f32, n_tiles, d1, sg.epi, h->H, h->I,
                           dst16 + (size_t)tile0 * 256 * d1, dst8 + (size_t)tile0 * 256 * d1 / 2, lo_off, zero_lo, not_f16(), h->f16_fit_dev);
      tile0 += n_tiles;
    }
  }
  // row path: chunk-major (pack_rowgemm_kernel) or k-streamed (pack_kstream_kernel); f16: fp16 values in the hi plane
  void rows(u16* dst, int f16) const {
    if (wd.row_mode == ROW_PACK_KSTREAM)
      hipLaunchKernelGGL(pack_kstream_kernel, grid(count()), dim3(256), 0, 0, f32, d0, d1, 1, dst, f16 ? 1 : zero_lo, any_lo, f16);
    else
      hipLaunchKernelGGL(pack_rowgemm_kernel, grid(count()), dim3(256), 0, 0, f32, d0, d1, wd.row_mode, h->H, h->I, dst, f16 ? 1 : zero_lo,
                         any_lo, f16);
  }
  void rows_f8(u16* dst_a, u16* dst_b) const {
    if (wd.row_mode == ROW_PACK_KSTREAM)
      hipLaunchKernelGGL(pack_kstream_f8_kernel, grid(count()), dim3(256), 0, 0, f32, d0, d1, 1, dst_a, dst_b, zero_lo, not_f16(), h->f16_fit_dev);
    else
      hipLaunchKernelGGL(pack_rowgemm_f8_kernel, grid(count()), dim3(256), 0, 0, f32, d0, d1, wd.row_mode, h->H, h->I, dst_a, zero_lo, not_f16(),
                         h->f16_fit_dev);
  }
  // after the one fp16 + e4m3 pack of the tensor: its energy, then the tensor's verdict (f16_unfit) from what the pack lost
  void close_f16_fit() const {
    hipLaunchKernelGGL(weight_energy_kernel, dim3(256), dim3(256), 0, 0, f32, count(), h->f16_fit_dev);
    hipLaunchKernelGGL(f16_fit_close_tensor_kernel, dim3(1), dim3(1), 0, 0, not_f16(), h->f16_fit_dev);
  }

  void run(u16* const* pk) const {  // pk[PF_COUNT]: the layer's packs of this weight
    if (pk[PF_HI])
      hipLaunchKernelGGL(split_planes_kernel, grid(count()), dim3(256), 0, 0, f32, d0, d1, wd.geglu ? h->I : 0, pk[PF_HI], pk[PF_LO], zero_lo,
                         any_lo);
    if (h->panel_path) {
      if (pk[PF_PANEL16]) {
        panels_f8(pk[PF_PANEL16], pk[PF_PANEL8]);
        close_f16_fit();
      }
      panels(pk[PF_PK], 0);
      if (pk[PF_PK16]) panels(pk[PF_PK16], 1);
    } else if (h->row_path) {
      rows(pk[PF_PK], 0);
      if (pk[PF_PK16]) rows(pk[PF_PK16], 1);
      if (pk[PF_ROW_F8A]) {
        rows_f8(pk[PF_ROW_F8A], pk[PF_ROW_F8B]);
        close_f16_fit();
      }
      if (pk[PF_L32])  // (hi plane; that kernel runs only when the lo planes are zero)
        hipLaunchKernelGGL(pack_layer32_kernel, grid(count()), dim3(256), 0, 0, f32, d0, d1, wd.l32_mode, wd.kmajor, h->H, h->I, pk[PF_L32]);
      for (PackFmt pf : {PF_PAIR, PF_PAIR16})
        if (pk[pf])
          hipLaunchKernelGGL(pack_layer16p_kernel, grid(count()), dim3(256), 0, 0, f32, d0, d1, wd.l32_mode, wd.kmajor, h->H, h->I, pk[pf],
                             pf == PF_PAIR16 ? 1 : 0);
    }
  }
};

}  // namespace

extern "C" {

int op_abi_version(void) { return OP_ABI_VERSION; }

const char* op_last_error(const op_handle* h) { return h ? h->err.c_str() : g_last_error.c_str(); }

const char* op_profile_kind_name(int kind) { return (kind >= 0 && kind < PK_COUNT) ? kProfileNames[kind] : "?"; }

int op_device_count(int* count) {
  if (!count) return fail(nullptr, OP_ERR_INVALID, "op_device_count: count is NULL");
  int n = 0;
  hipError_t e = hipGetDeviceCount(&n);
  if (e != hipSuccess) {
    *count = 0;
    return fail(nullptr, OP_ERR_HIP, "hipGetDeviceCount failed: %s", hipGetErrorString(e));
  }
  *count = n;
  return OP_OK;
}

int op_create(const op_config* cfg, op_handle** out) {
  if (!cfg || !out) return fail(nullptr, OP_ERR_INVALID, "op_create: NULL argument");
  *out = nullptr;
  if (cfg->struct_bytes != sizeof(op_config))
    return fail(nullptr, OP_ERR_INVALID, "op_create: op_config.struct_bytes=%u, library expects %zu (ABI mismatch)",
                cfg->struct_bytes, sizeof(op_config));
  const int H = cfg->hidden_size, I = cfg->intermediate_size, N = cfg->num_layers, nh = cfg->num_heads;
  if (H <= 0 || I <= 0 || N <= 0 || nh <= 0 || cfg->vocab_size <= 0 || cfg->num_labels <= 0)
    return fail(nullptr, OP_ERR_INVALID, "op_create: non-positive dimension");
  if (N > OP_MAX_LAYERS) return fail(nullptr, OP_ERR_UNSUPPORTED, "num_layers %d > %d", N, OP_MAX_LAYERS);
  if (H % nh != 0 || H / nh != HEAD_DIM)
    return fail(nullptr, OP_ERR_UNSUPPORTED, "head_dim must be 64 (hidden_size %d / num_heads %d)", H, nh);
  if (H % GEMM_BN != 0 || H > 1024)
    return fail(nullptr, OP_ERR_UNSUPPORTED, "hidden_size %d must be a multiple of 128 and <= 1024", H);
  if (I % 64 != 0) return fail(nullptr, OP_ERR_UNSUPPORTED, "intermediate_size %d must be a multiple of 64", I);
  if (cfg->num_labels > 64) return fail(nullptr, OP_ERR_UNSUPPORTED, "num_labels %d > 64", cfg->num_labels);
  Policy req;
  switch (cfg->precision) {
    case OP_PRECISION_BF16X3: req = opl::kPolicies[0]; break;
    case OP_PRECISION_BF16X2: req = opl::kPolicies[1]; break;
    case OP_PRECISION_BF16: req = opl::kPolicies[2]; break;
    case OP_PRECISION_CUSTOM:
      for (int f = 0; f < OP_FAM_COUNT; ++f)
        if (cfg->terms[f] > 3) return fail(nullptr, OP_ERR_INVALID, "terms[%d] = %d is not a term mask (0..3)", f, cfg->terms[f]);
      req = Policy{cfg->terms[OP_FAM_WQKV], cfg->terms[OP_FAM_QK], cfg->terms[OP_FAM_PV], cfg->terms[OP_FAM_ATTN_OUT],
                   cfg->terms[OP_FAM_WI], cfg->terms[OP_FAM_MLP_OUT]};
      break;
    default: return fail(nullptr, OP_ERR_INVALID, "unknown precision %d", cfg->precision);
  }
  if (cfg->pooling != OP_POOL_CLS && cfg->pooling != OP_POOL_MEAN)
    return fail(nullptr, OP_ERR_INVALID, "unknown pooling %d", cfg->pooling);
  if (cfg->local_attention < 0 || cfg->max_position_embeddings <= 0)
    return fail(nullptr, OP_ERR_INVALID, "bad local_attention / max_position_embeddings");

  int ndev = 0;
  hipError_t e = hipGetDeviceCount(&ndev);
  if (e != hipSuccess || ndev <= 0)
    return fail(nullptr, OP_ERR_HIP, "no HIP device available (%s); this library has no CPU fallback",
                e != hipSuccess ? hipGetErrorString(e) : "device count is 0");
  if (cfg->device_id < 0 || cfg->device_id >= ndev)
    return fail(nullptr, OP_ERR_INVALID, "device_id %d out of range (count %d)", cfg->device_id, ndev);

  op_handle* h = new (std::nothrow) op_handle();
  if (!h) return fail(nullptr, OP_ERR_NOMEM, "out of host memory");
  h->cfg = *cfg;
  h->H = H;
  h->I = I;
  h->N = N;
  h->nh = nh;
  h->V = cfg->vocab_size;
  h->nl = cfg->num_labels;
  h->max_pos = cfg->max_position_embeddings;
  h->req = h->eff = req;
  h->chunk_rows = cfg->chunk_rows > 0 ? align_up(cfg->chunk_rows, ROW_ALIGN) : 262144;  // grids must cover the chip several times over
  h->layers.resize(N);
  // the dispatch path of this shape (opp::paths_of)
  const opp::Paths paths = opp::paths_of(H, I, (unsigned)cfg->flags);
  h->row_path = paths.row;
  h->panel_path = paths.panel;

#define OP_CREATE_TRY(expr)  \
  do {                       \
    int _rc = (expr);        \
    if (_rc != OP_OK) {      \
      g_last_error = h->err; \
      op_destroy(h);         \
      return _rc;            \
    }                        \
  } while (0)
#define OP_CREATE_HIP(expr)                                                                  \
  do {                                                                                       \
    hipError_t _e = (expr);                                                                  \
    if (_e != hipSuccess) {                                                                  \
      int _rc = fail(h, OP_ERR_HIP, "%s failed: %s", #expr, hipGetErrorString(_e));          \
      op_destroy(h);                                                                         \
      return _rc;                                                                            \
    }                                                                                        \
  } while (0)

  OP_CREATE_HIP(hipSetDevice(cfg->device_id));
  {
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, cfg->device_id) == hipSuccess && prop.multiProcessorCount > 0)
      h->n_cus = prop.multiProcessorCount;
  }
  const size_t HH = (size_t)H * H;
  OP_CREATE_TRY(dev_alloc(h, &h->any_lo_dev, OP_FAM_COUNT + 3));  // + the fp16-fit flags of the "f16 + fp8" packs (note_f16_fit)
  OP_CREATE_HIP(hipMemset(h->any_lo_dev, 0, (OP_FAM_COUNT + 3) * sizeof(int)));
  OP_CREATE_TRY(dev_alloc(h, &h->f16_fit_dev, 2));
  OP_CREATE_HIP(hipMemset(h->f16_fit_dev, 0, 2 * sizeof(float)));
  // the weight packs this shape and these flags build (opp::packs_of)
  const opp::Packs packs = opp::packs_of(paths, H, (unsigned)cfg->flags);
  h->f8_packs = packs.f8;
  h->h16_packs = packs.h16;
  h->f32_packs = packs.f32;
  OP_CREATE_TRY(dev_alloc(h, &h->emb, (size_t)h->V * H));
  OP_CREATE_TRY(dev_alloc(h, &h->emb_norm, H));
  OP_CREATE_TRY(dev_alloc(h, &h->final_norm, H));
  OP_CREATE_TRY(dev_alloc(h, &h->dense_t, HH));
  OP_CREATE_TRY(dev_alloc(h, &h->head_norm, H));
  OP_CREATE_TRY(dev_alloc(h, &h->cls_w, (size_t)h->nl * H));
  OP_CREATE_TRY(dev_alloc(h, &h->cls_b, h->nl));
  OP_CREATE_TRY(dev_alloc(h, &h->prune_w, (size_t)2 * H));
  OP_CREATE_TRY(dev_alloc(h, &h->prune_b, 2));
  h->missing = {"model.embeddings.tok_embeddings.weight", "model.embeddings.norm.weight", "model.final_norm.weight",
                "head.dense.weight", "head.norm.weight", "classifier.weight", "classifier.bias",
                "pruning_head.classifier.weight", "pruning_head.classifier.bias"};
  for (int i = 0; i < N; ++i) {
    LayerWeights& lw = h->layers[i];
    const std::string pre = "model.layers." + std::to_string(i) + ".";
    if (i != 0) {
      OP_CREATE_TRY(dev_alloc(h, &lw.attn_norm, H));
      h->missing.push_back(pre + "attn_norm.weight");
    }
    OP_CREATE_TRY(dev_alloc(h, &lw.mlp_norm, H));
    // the GEMM weights in every format this handle's path and flags build (pack_exists); fp16 + e4m3: 4 bytes per weight element
    for (const AllocStep& step : kAllocOrder)
      for (Weight w : step.order)
        for (int f = 0; f < step.n_fmt; ++f) {
          const PackFmt pf = step.fmt[f];
          if (kPackElems[w][pf] && pack_exists(pf, h->row_path, h->panel_path, h->f8_packs, h->h16_packs, h->f32_packs, H))
            OP_CREATE_TRY(dev_alloc(h, &lw.pack[w][pf], weight_elems(w, H, I) * kPackElems[w][pf]));
        }
    h->missing.push_back(pre + "mlp_norm.weight");
    for (const WeightDesc& wd : kWeights) h->missing.push_back(pre + wd.tail);
  }
  OP_CREATE_TRY(dev_alloc(h, &h->cov_bits, ((size_t)h->V + 31) / 32));
  OP_CREATE_TRY(dev_alloc(h, &h->cov_state, (size_t)opl::COV_WORDS));
  OP_CREATE_TRY(dev_alloc(h, &h->loss_scratch, 1));  // (here, not on first use: op_loss without a report may be captured)
  for (int t = 0; t < 2; ++t) {
    std::vector<float> cs, sn;
    build_rope_host(t == 1 ? cfg->global_rope_theta : cfg->local_rope_theta, h->max_pos, cs, sn);
    OP_CREATE_TRY(dev_alloc(h, &h->rope_cos[t], cs.size()));
    OP_CREATE_TRY(dev_alloc(h, &h->rope_sin[t], sn.size()));
    OP_CREATE_HIP(hipMemcpy(h->rope_cos[t], cs.data(), cs.size() * sizeof(float), hipMemcpyHostToDevice));
    OP_CREATE_HIP(hipMemcpy(h->rope_sin[t], sn.data(), sn.size() * sizeof(float), hipMemcpyHostToDevice));
  }
  *out = h;
  return OP_OK;
}

void op_destroy(op_handle* h) {
  if (!h) return;
  (void)hipSetDevice(h->cfg.device_id);
  for (auto& ev : h->events) {
    (void)hipEventDestroy(ev.start);
    (void)hipEventDestroy(ev.stop);
  }
  for (void* p : h->allocations) (void)hipFree(p);
  if (h->pad_host) (void)hipHostFree(h->pad_host);
  if (h->cov_host) (void)hipHostFree(h->cov_host);
  if (h->loss_host) (void)hipHostFree(h->loss_host);
  delete h;
}

int op_load_weight(op_handle* h, const char* name_c, const void* data, int dtype, const int64_t* shape, int ndim) {
  if (!h || !name_c || !data || !shape) return fail(h, OP_ERR_INVALID, "op_load_weight: NULL argument");
  if (dtype != OP_DTYPE_F32 && dtype != OP_DTYPE_BF16 && dtype != OP_DTYPE_F16)
    return fail(h, OP_ERR_INVALID, "op_load_weight(%s): unknown dtype %d", name_c, dtype);
  if (ndim < 1 || ndim > 2) return fail(h, OP_ERR_INVALID, "op_load_weight(%s): ndim %d not in {1,2}", name_c, ndim);
  std::string name(name_c);
  const std::string legacy_prefix = "ranking_model.";
  if (name.compare(0, legacy_prefix.size(), legacy_prefix) == 0) name = name.substr(legacy_prefix.size());
  const int64_t d0 = shape[0], d1 = ndim == 2 ? shape[1] : 1;
  const int H = h->H, I = h->I;

  bool transpose = false;
  float* dst_f32 = nullptr;
  const WeightDesc* wd = nullptr;  // a GEMM weight ...
  u16* const* packs = nullptr;     // ... and the layer's packs of it
  int64_t want0 = 0, want1 = 1;
  auto expect = [&](int64_t a, int64_t b) {
    want0 = a;
    want1 = b;
  };

  if (name == "model.embeddings.tok_embeddings.weight") {
    dst_f32 = h->emb; expect(h->V, H);
    h->cov_clear = true;  // (the audited ids were audited against the old table)
  } else if (name == "model.embeddings.norm.weight") {
    dst_f32 = h->emb_norm; expect(H, 1);
  } else if (name == "model.final_norm.weight") {
    dst_f32 = h->final_norm; expect(H, 1);
  } else if (name == "head.dense.weight") {
    dst_f32 = h->dense_t; transpose = true; expect(H, H);
  } else if (name == "head.norm.weight") {
    dst_f32 = h->head_norm; expect(H, 1);
  } else if (name == "classifier.weight") {
    dst_f32 = h->cls_w; expect(h->nl, H);
  } else if (name == "classifier.bias") {
    dst_f32 = h->cls_b; expect(h->nl, 1);
  } else if (name == "pruning_head.classifier.weight") {
    dst_f32 = h->prune_w; expect(2, H);
  } else if (name == "pruning_head.classifier.bias") {
    dst_f32 = h->prune_b; expect(2, 1);
  } else {
    int li = -1;
    char tail[64] = {0};
    if (sscanf(name.c_str(), "model.layers.%d.%63s", &li, tail) != 2 || li < 0 || li >= h->N)
      return fail(h, OP_ERR_INVALID, "op_load_weight: unknown tensor name '%s'", name_c);
    LayerWeights& lw = h->layers[li];
    const std::string t(tail);
    if (t == "attn_norm.weight" && li != 0) {
      dst_f32 = lw.attn_norm; expect(H, 1);
    } else if (t == "mlp_norm.weight") {
      dst_f32 = lw.mlp_norm; expect(H, 1);
    } else {
      for (int w = 0; w < W_COUNT; ++w)
        if (t == kWeights[w].tail) {
          wd = &kWeights[w];
          packs = lw.pack[w];
          expect((int64_t)weight_rows((Weight)w, H, I), (int64_t)weight_cols((Weight)w, H, I));
        }
      if (!wd) return fail(h, OP_ERR_INVALID, "op_load_weight: unknown tensor name '%s'", name_c);
    }
  }
  if (d0 != want0 || d1 != want1)
    return fail(h, OP_ERR_INVALID, "op_load_weight(%s): shape [%lld, %lld] but the model needs [%lld, %lld]", name_c,
                (long long)d0, (long long)d1, (long long)want0, (long long)want1);

  OP_HIP(h, hipSetDevice(h->cfg.device_id));
  const size_t count = (size_t)d0 * (size_t)d1;
  const size_t esz = dtype == OP_DTYPE_F32 ? 4 : 2;
  void* raw = nullptr;
  float* f32 = nullptr;
  OP_HIP(h, hipMalloc(&raw, count * esz));
  hipError_t e = hipMemcpy(raw, data, count * esz, hipMemcpyDefault);
  if (e == hipSuccess) e = hipMalloc((void**)&f32, count * sizeof(float));
  if (e != hipSuccess) {
    (void)hipFree(raw);
    return fail(h, OP_ERR_HIP, "op_load_weight(%s): staging failed: %s", name_c, hipGetErrorString(e));
  }
  const unsigned blocks = (unsigned)((count + 255) / 256);
  hipLaunchKernelGGL(convert_to_f32_kernel, dim3(blocks), dim3(256), 0, 0, raw, dtype, count, f32);
  if (wd) {
    const int req_mask[OP_FAM_COUNT] = {h->req.wqkv, h->req.qk, h->req.pv, h->req.attn_out, h->req.wi, h->req.mlp_out};
    h->resolved = false;
    // a kernel set pinned by op_select_kernel_set or measured by op_calibrate belongs to the weights it was chosen on: new
    // GEMM weights start from the default selection again (and from the compact formats, if op_set_compact_operands left them)
    h->forced_set = -1;
    h->forced_mlp_layers = ~0ull;
    h->f8_off = false;
    WeightPacker{h, *wd, f32, (int)d0, (int)d1, (req_mask[wd->family] & OP_TERM_RIGHT_LO) ? 0 : 1, h->any_lo_dev + wd->family}.run(packs);
    // kernel set "fp32": the tensor as it is
    if (packs[PF_F32]) e = hipMemcpyAsync(packs[PF_F32], f32, count * sizeof(float), hipMemcpyDeviceToDevice, 0);
  } else if (transpose) {
    hipLaunchKernelGGL(transpose_f32_kernel, dim3(blocks), dim3(256), 0, 0, f32, (int)d0, (int)d1, dst_f32);
  } else {
    e = hipMemcpyAsync(dst_f32, f32, count * sizeof(float), hipMemcpyDeviceToDevice, 0);
  }
  if (e == hipSuccess) e = hipGetLastError();
  if (e == hipSuccess) e = hipStreamSynchronize(0);
  (void)hipFree(raw);
  (void)hipFree(f32);
  if (e != hipSuccess) return fail(h, OP_ERR_HIP, "op_load_weight(%s): %s", name_c, hipGetErrorString(e));
  erase_missing(h, name);
  return OP_OK;
}

}  // extern "C"

namespace {
// what selection reads from the handle (the device flags: resolve_policy)
opp::SelectState select_state(const op_handle* h) {
  opp::SelectState s;
  s.req = h->req;
  s.f16_unfit = h->f16_unfit;
  s.row_path = h->row_path;
  s.panel_path = h->panel_path;
  s.f8_packs = h->f8_packs;
  s.h16_packs = h->h16_packs;
  s.f32_packs = h->f32_packs;
  s.f8_off = h->f8_off;
  s.flags = h->cfg.flags;
  s.forced_set = h->forced_set;
  s.forced_mlp_layers = h->forced_mlp_layers;
  return s;
}

// The weights' flags from the device, the selection (opp::select), the result into the handle.
int resolve_policy(op_handle* h) {
  if (h->resolved) return OP_OK;
  // [OP_FAM_COUNT]: some GEMM weight is not exactly an fp16 value; [+ 2]: some weight TENSOR sits on fp16's subnormal grid
  // (note_f16_fit in opk_common.hip.h): the "f16 + fp8" sets cannot represent it
  int any_lo[OP_FAM_COUNT + 3] = {0};
  OP_HIP(h, hipSetDevice(h->cfg.device_id));
  OP_HIP(h, hipMemcpy(any_lo, h->any_lo_dev, sizeof(any_lo), hipMemcpyDeviceToHost));
  h->f16_unfit = any_lo[OP_FAM_COUNT + 2] != 0;
  opp::SelectState s = select_state(h);
  for (int f = 0; f < OP_FAM_COUNT; ++f) s.any_lo[f] = any_lo[f] != 0;
  s.not_f16 = any_lo[OP_FAM_COUNT] != 0;
  const opp::Selection sel = opp::select(s);
  h->eff = sel.eff;
  h->set = sel.set;
  h->ks = &opp::set_row(sel.set);
  h->mlp_layers = sel.mlp_layers;
  h->resolved = true;
  return OP_OK;
}

// run kernel set `set` with layer mask `mlp_layers` from now on where the handle can (-1: the default selection)
int pin(op_handle* h, int set, uint64_t mlp_layers = ~0ull) {
  h->forced_set = set;
  h->forced_mlp_layers = mlp_layers;
  h->resolved = false;
  return resolve_policy(h);
}

// deterministic calibration batch: 24 rows of min(512, max_pos) tokens + 14 ragged rows, ids uniform over the vocabulary
// (specials avoided as bench.py does: [1000, V - 1000) when the vocabulary is that large)
void synthetic_calibration_rows(const op_handle* h, std::vector<int32_t>& ids, std::vector<int32_t>& cu) {
  const int full = std::min(512, h->max_pos);
  // (the forward fuzz on calibrated sets finds its worst rows among the 1-3 token ones: several of them are in)
  const int ragged[14] = {1, 2, 2, 3, 5, 9, 17, 33, 64, 96, 130, 257, 333, 511};
  std::vector<int> lens(24, full);
  for (int r : ragged) lens.push_back(std::min(r, h->max_pos));
  const int lo = h->V > 4000 ? 1000 : 0, span = h->V > 4000 ? h->V - 2000 : h->V;
  uint64_t state = 0x9E3779B97F4A7C15ull;
  cu.assign(1, 0);
  ids.clear();
  for (int len : lens) {
    for (int i = 0; i < len; ++i) {
      state += 0x9E3779B97F4A7C15ull;  // splitmix64
      uint64_t z = state;
      z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
      z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
      z ^= z >> 31;
      ids.push_back(lo + (int32_t)(z % (uint64_t)span));
    }
    cu.push_back((int32_t)ids.size());
  }
}

// op_calibrate's visit to a handle.  While it lasts nothing is profiled or captured; when it ends, on whichever way out, both
// come back -- and so does what was pinned before the call, unless the call got as far as pinning its own answer (keep_pin).
struct CalibrationVisit {
  op_handle* const h;
  const bool profiling;
  float* const capture;
  const bool f8_off;
  const int forced_set;
  const uint64_t forced_mlp_layers;
  bool pin_kept = false;

  explicit CalibrationVisit(op_handle* h_)
      : h(h_), profiling(h_->profiling), capture(h_->capture), f8_off(h_->f8_off), forced_set(h_->forced_set), forced_mlp_layers(h_->forced_mlp_layers) {
    h->profiling = false;
    h->capture = nullptr;
  }
  CalibrationVisit(const CalibrationVisit&) = delete;
  void keep_pin() { pin_kept = true; }
  int restore_pin() {
    pin_kept = true;
    h->f8_off = f8_off;
    return pin(h, forced_set, forced_mlp_layers);
  }
  ~CalibrationVisit() {
    h->profiling = profiling;
    h->capture = capture;
    if (!pin_kept) (void)restore_pin();
  }
};

}  // namespace

extern "C" {

int op_weights_ready(op_handle* h) {
  if (!h) return fail(nullptr, OP_ERR_INVALID, "op_weights_ready: NULL handle");
  if (h->missing.empty()) return resolve_policy(h);
  std::string msg = "missing weights:";
  size_t shown = 0;
  for (const auto& m : h->missing) {
    if (shown++ == 8) {
      msg += " ...";
      break;
    }
    msg += " " + m;
  }
  msg += " (" + std::to_string(h->missing.size()) + " total)";
  return fail(h, OP_ERR_STATE, "%s", msg.c_str());
}

int op_set_compact_operands(op_handle* h, int enabled, int* changed) {
  if (!h) return fail(nullptr, OP_ERR_INVALID, "op_set_compact_operands: NULL handle");
  int rc = op_weights_ready(h);
  if (rc != OP_OK) return rc;
  const int before = h->set;
  h->f8_off = enabled == 0;
  // (switching off: a pinned / calibrated compact set goes too)
  rc = enabled ? pin(h, h->forced_set, h->forced_mlp_layers) : pin(h, -1);
  if (changed) *changed = (rc == OP_OK && h->set != before) ? 1 : 0;
  return rc;
}

int op_select_kernel_set(op_handle* h, int kernel_set) {
  if (!h) return fail(nullptr, OP_ERR_INVALID, "op_select_kernel_set: NULL handle");
  int rc = op_weights_ready(h);
  if (rc != OP_OK) return rc;
  if (kernel_set == OP_KS_F32 && !h->f32_packs)
    return fail(h, OP_ERR_UNSUPPORTED, "op_select_kernel_set: kernel set %d (\"fp32\") needs the fp32 weight packs: create the handle with OP_FLAG_F32_PACKS",
                kernel_set);
  if (kernel_set != OP_KS_AUTO && !opp::set_available(select_state(h), kernel_set))
    return fail(h, OP_ERR_UNSUPPORTED, "op_select_kernel_set: kernel set %d cannot run on this handle (shape, flags or weights)", kernel_set);
  return pin(h, kernel_set == OP_KS_AUTO ? -1 : kernel_set);  // (the coverage follows the arithmetic: coverage_prepare)
}

int op_mlp_correction_layers(op_handle* h, uint64_t* layer_mask) {
  if (!h || !layer_mask) return fail(h, OP_ERR_INVALID, "op_mlp_correction_layers: NULL argument");
  int rc = op_weights_ready(h);
  if (rc != OP_OK) return rc;
  *layer_mask = mlp_by_layer(*h->ks) ? (h->mlp_layers & opp::all_layers_mask(h->cfg.num_layers)) : 0ull;
  return OP_OK;
}

int op_select_mlp_correction_layers(op_handle* h, uint64_t layer_mask) {
  if (!h) return fail(nullptr, OP_ERR_INVALID, "op_select_mlp_correction_layers: NULL handle");
  int rc = op_weights_ready(h);
  if (rc != OP_OK) return rc;
  if (h->forced_set != OP_KS_F16_MLP_F8 && h->forced_set != OP_KS_F16_MLP_F8_W)
    return fail(h, OP_ERR_STATE, "op_select_mlp_correction_layers: pin kernel set %d or %d first (op_select_kernel_set / op_calibrate)", OP_KS_F16_MLP_F8_W,
                OP_KS_F16_MLP_F8);
  if (h->cfg.num_layers > 64) return fail(h, OP_ERR_UNSUPPORTED, "op_select_mlp_correction_layers: more than 64 layers");
  return pin(h, h->forced_set, layer_mask);
}

int op_calibrate(op_handle* h, float tolerance, const int32_t* ids_host, const int32_t* cu_seqlens_host, int n_seqs,
                 op_calibration* report) {
  if (!h) return fail(nullptr, OP_ERR_INVALID, "op_calibrate: NULL handle");
  if (report && report->struct_bytes != sizeof(op_calibration))
    return fail(h, OP_ERR_INVALID, "op_calibrate: op_calibration.struct_bytes=%u, library expects %zu", report->struct_bytes, sizeof(op_calibration));
  if (!(tolerance >= 0.f)) return fail(h, OP_ERR_INVALID, "op_calibrate: tolerance must be >= 0");
  if ((ids_host == nullptr) != (cu_seqlens_host == nullptr) || (ids_host && n_seqs <= 0))
    return fail(h, OP_ERR_INVALID, "op_calibrate: ids_host / cu_seqlens_host / n_seqs must be given together");
  int rc = op_weights_ready(h);
  if (rc != OP_OK) return rc;
  // the caller's batch is checked BEFORE the handle's state is touched: a refused call leaves a pinned set where it was
  if (ids_host) {
    const opp::Refusal bad = opp::check_calibration_batch(ids_host, cu_seqlens_host, n_seqs, h->cfg.max_position_embeddings, h->cfg.vocab_size);
    if (bad.code != OP_OK) return fail(h, bad);
  }
  OP_HIP(h, hipSetDevice(h->cfg.device_id));
  h->cov_clear = true;  // whatever set comes out, it has seen no real row
  CalibrationVisit visit(h);

  // the default selection and its (hi, lo) bf16 realisation = the reference of the comparison
  OP_TRY(pin(h, -1));
  const int default_set = h->set;
  h->f8_off = true;
  OP_TRY(pin(h, -1));
  // OP_CAL_REFERENCE_F32 on a handle with the fp32 packs: kernel set "fp32" is the reference, the (hi, lo) bf16 set a candidate
  // like any other (where it is cheaper than the default)
  const bool ref_f32 = report && (report->flags & OP_CAL_REFERENCE_F32) != 0 && h->set >= 0 && opp::set_available(select_state(h), OP_KS_F32);
  const int reference_set = ref_f32 ? (int)OP_KS_F32 : h->set;
  h->f8_off = visit.f8_off;
  OP_TRY(pin(h, -1));

  op_calibration rep;
  memset(&rep, 0, sizeof(rep));
  rep.struct_bytes = sizeof(rep);
  rep.tolerance = tolerance;
  rep.reference_set = reference_set;
  rep.default_set = default_set;
  rep.chosen_set = default_set;
  rep.flags = report ? report->flags : 0u;
  auto finish = [&]() -> int {
    if (report) *report = rep;
    return OP_OK;
  };
  // nothing to measure: whatever was pinned before the call stays pinned
  auto finish_unchanged = [&]() -> int {
    OP_TRY(visit.restore_pin());
    rep.chosen_set = h->set;
    return finish();
  };
  if (default_set < 0 || reference_set < 0) return finish_unchanged();  // a custom policy on the all-terms kernels: nothing cheaper is defined
  const std::vector<int> cand = opp::calibration_candidates(select_state(h), default_set);
  if (cand.empty() && !ref_f32) return finish_unchanged();  // (fp32 reference: the default itself is still measured against it)

  std::vector<int32_t> ids, cu;
  if (ids_host) {
    cu.assign(cu_seqlens_host, cu_seqlens_host + n_seqs + 1);
    ids.assign(ids_host, ids_host + cu[n_seqs]);
  } else {
    synthetic_calibration_rows(h, ids, cu);
    n_seqs = (int)cu.size() - 1;
  }
  const int total = cu[n_seqs];
  int max_len = 0;
  for (int s = 0; s < n_seqs; ++s) max_len = std::max(max_len, cu[s + 1] - cu[s]);
  rep.n_rows = n_seqs;
  rep.n_tokens = total;

  size_t ws_bytes = op_workspace_bytes(h, n_seqs, total, max_len);
  // the largest workspace of the sets that run: the fp32 set's (its planes follow everybody's regions)
  if (ref_f32) ws_bytes = std::max(ws_bytes, forward_layout(h, n_seqs, total, max_len, true).bytes);
  const size_t n_prune = (size_t)total * 2, n_rank = (size_t)n_seqs * h->nl;
  int32_t *ids_dev = nullptr, *cu_dev = nullptr;
  float* out_dev = nullptr;
  void* ws_dev = nullptr;
  hipStream_t st = nullptr;
  auto release = [&]() {
    if (st) (void)hipStreamDestroy(st);
    (void)hipFree(ids_dev);
    (void)hipFree(cu_dev);
    (void)hipFree(out_dev);
    (void)hipFree(ws_dev);
  };
  hipError_t e = hipMalloc((void**)&ids_dev, ids.size() * sizeof(int32_t));
  if (e == hipSuccess) e = hipMalloc((void**)&cu_dev, cu.size() * sizeof(int32_t));
  if (e == hipSuccess) e = hipMalloc((void**)&out_dev, (n_prune + n_rank) * sizeof(float));
  if (e == hipSuccess) e = hipMalloc(&ws_dev, ws_bytes + 256);
  if (e == hipSuccess) e = hipStreamCreate(&st);
  if (e == hipSuccess) e = hipMemcpy(ids_dev, ids.data(), ids.size() * sizeof(int32_t), hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(cu_dev, cu.data(), cu.size() * sizeof(int32_t), hipMemcpyHostToDevice);
  if (e != hipSuccess) {
    release();
    return fail(h, OP_ERR_HIP, "op_calibrate: staging failed: %s", hipGetErrorString(e));
  }
  void* ws_aligned = reinterpret_cast<void*>((reinterpret_cast<uintptr_t>(ws_dev) + 255) / 256 * 256);
  std::vector<float> ref(n_prune + n_rank), got(n_prune + n_rank);
  auto run = [&](int set, std::vector<float>& out, uint64_t mlp_layers) -> int {
    OP_TRY(pin(h, set, mlp_layers));
    OP_TRY(op_forward_packed(h, ids_dev, cu_dev, cu.data(), n_seqs, total, max_len, out_dev, out_dev + n_prune, nullptr, ws_aligned,
                             ws_bytes, st));
    OP_HIP(h, hipStreamSynchronize(st));
    OP_HIP(h, hipMemcpy(out.data(), out_dev, out.size() * sizeof(float), hipMemcpyDeviceToHost));
    return OP_OK;
  };
  bool have_ref = false;  // the search's first measurement is the reference's own run
  auto measure = [&](int set, uint64_t mlp_layers) -> opp::Measurement {
    const bool is_ref = !have_ref;
    have_ref = true;
    const int run_rc = run(set, is_ref ? ref : got, mlp_layers);
    if (run_rc != OP_OK) return {run_rc, INFINITY};
    if (!is_ref) return {OP_OK, opp::max_diff(got, ref)};
    bool ref_finite = true;
    for (float v : ref) ref_finite = ref_finite && std::isfinite(v);
    return {OP_OK, ref_finite ? 0.f : INFINITY};
  };
  const opp::SearchResult found = opp::calibration_search(cand, reference_set, default_set, tolerance, rep.flags, h->cfg.num_layers, measure);
  release();

  // what the search chose runs from now on (after an error: the default selection)
  visit.keep_pin();
  const uint64_t all_layers = opp::all_layers_mask(h->cfg.num_layers);
  const int rc2 = found.chosen >= 0 ? pin(h, found.chosen, found.mlp_layers | ~all_layers) : pin(h, -1);
  if (found.rc != OP_OK) return found.rc;
  if (rc2 != OP_OK) return rc2;
  rep.default_err = found.default_err;
  rep.n_candidates = found.n_candidates;
  std::copy(found.candidate_set, found.candidate_set + 16, rep.candidate_set);
  std::copy(found.candidate_err, found.candidate_err + 16, rep.candidate_err);
  rep.mlp_layers_err = found.mlp_layers_err;
  rep.chosen_set = h->set;
  rep.mlp_layers = mlp_by_layer(*h->ks) ? (h->mlp_layers & all_layers) : 0ull;
  return finish();
}

int op_effective_policy(op_handle* h, uint8_t* terms_out, int* kernel_set) {
  if (!h || !terms_out || !kernel_set) return fail(h, OP_ERR_INVALID, "op_effective_policy: NULL argument");
  int rc = op_weights_ready(h);
  if (rc != OP_OK) return rc;
  terms_out[OP_FAM_WQKV] = (uint8_t)h->eff.wqkv;
  terms_out[OP_FAM_QK] = (uint8_t)h->eff.qk;
  terms_out[OP_FAM_PV] = (uint8_t)h->eff.pv;
  terms_out[OP_FAM_ATTN_OUT] = (uint8_t)h->eff.attn_out;
  terms_out[OP_FAM_WI] = (uint8_t)h->eff.wi;
  terms_out[OP_FAM_MLP_OUT] = (uint8_t)h->eff.mlp_out;
  *kernel_set = h->set;
  return OP_OK;
}

size_t op_workspace_bytes(const op_handle* h, int n_seqs, int total_tokens, int max_seqlen) {
  if (!h || n_seqs < 0 || total_tokens < 0 || max_seqlen < 0) return 0;
  return forward_layout(h, n_seqs, total_tokens, max_seqlen, h->set == OP_KS_F32).bytes;
}

int op_debug_workspace_layout(const op_handle* h, int n_seqs, int total_tokens, int max_seqlen, op_workspace_region* entries,
                              int max_entries) {
  if (!h || n_seqs < 0 || total_tokens < 0 || max_seqlen < 0 || max_entries < 0 || (!entries && max_entries > 0)) return OP_ERR_INVALID;
  const opp::Layout lay = forward_layout(h, n_seqs, total_tokens, max_seqlen, h->set == OP_KS_F32);  // (as op_workspace_bytes)
  for (int i = 0; i < lay.n && i < max_entries; ++i)
    entries[i] = op_workspace_region{lay.regions[i].name, (uint64_t)lay.regions[i].offset, (uint64_t)lay.regions[i].bytes, (int32_t)lay.regions[i].kind};
  return lay.n;
}

int op_debug_rope_tables(const op_handle* h, int global_table, float theta, int max_pos, float* cos_host, float* sin_host) {
  if (max_pos <= 0 || !cos_host || !sin_host) return OP_ERR_INVALID;
  const size_t count = (size_t)max_pos * ROPE_HALF;
  if (!h) {  // no handle, no device: the tables op_create would build for this theta
    if (!(theta > 0.f)) return OP_ERR_INVALID;
    std::vector<float> cs, sn;
    build_rope_host(theta, max_pos, cs, sn);
    std::copy(cs.begin(), cs.end(), cos_host);
    std::copy(sn.begin(), sn.end(), sin_host);
    return OP_OK;
  }
  const int t = global_table ? 1 : 0;
  if (max_pos != h->max_pos || !h->rope_cos[t] || !h->rope_sin[t]) return OP_ERR_INVALID;
  if (hipSetDevice(h->cfg.device_id) != hipSuccess) return OP_ERR_HIP;
  if (hipMemcpy(cos_host, h->rope_cos[t], count * sizeof(float), hipMemcpyDeviceToHost) != hipSuccess) return OP_ERR_HIP;
  if (hipMemcpy(sin_host, h->rope_sin[t], count * sizeof(float), hipMemcpyDeviceToHost) != hipSuccess) return OP_ERR_HIP;
  return OP_OK;
}

int op_debug_primitive(op_handle* h, int kind, int mode, const void* in_dev, size_t n, void* out_dev, void* hip_stream) {
  if (!h) return fail(nullptr, OP_ERR_INVALID, "op_debug_primitive: NULL handle");
  const int group = opl::probe_group_size(kind);
  if (group == 0 || (mode != 0 && mode != 1)) return fail(h, OP_ERR_INVALID, "op_debug_primitive: unknown kind %d or mode %d", kind, mode);
  if (n % (size_t)group != 0) return fail(h, OP_ERR_INVALID, "op_debug_primitive: n = %zu is not a multiple of kind %d's group of %d", n, kind, group);
  if (n > ((size_t)1 << 31)) return fail(h, OP_ERR_INVALID, "op_debug_primitive: n = %zu is beyond 2^31 elements", n);
  if (n == 0) return OP_OK;
  if (!in_dev || !out_dev) return fail(h, OP_ERR_INVALID, "op_debug_primitive: NULL buffer");
  OP_HIP(h, hipSetDevice(h->cfg.device_id));
  opl::launch_probe((hipStream_t)hip_stream, kind, mode, in_dev, n, out_dev);
  OP_HIP(h, hipGetLastError());
  return OP_OK;
}

int op_debug_capture_hidden(op_handle* h, float* hidden_dev) {
  if (!h) return fail(nullptr, OP_ERR_INVALID, "op_debug_capture_hidden: NULL handle");
  h->capture = hidden_dev;
  return OP_OK;
}

int op_profile_enable(op_handle* h, int enabled) {
  if (!h) return fail(nullptr, OP_ERR_INVALID, "op_profile_enable: NULL handle");
  h->profiling = enabled != 0;
  return OP_OK;
}

int op_segment_means(op_handle* h, const float* keep_prob_dev, int n_values, const int32_t* seg_dev, int n_seg,
                     float* out_dev, void* hip_stream) {
  if (!h) return fail(nullptr, OP_ERR_INVALID, "op_segment_means: NULL handle");
  if (n_seg < 0 || n_values < 0 || (n_seg > 0 && (!keep_prob_dev || !seg_dev || !out_dev)))
    return fail(h, OP_ERR_INVALID, "op_segment_means: NULL buffer or negative count");
  if (n_seg == 0) return OP_OK;
  OP_HIP(h, hipSetDevice(h->cfg.device_id));
  hipLaunchKernelGGL(segment_mean_kernel, dim3((unsigned)((n_seg + 127) / 128)), dim3(128), 0, (hipStream_t)hip_stream,
                     keep_prob_dev, seg_dev, n_seg, n_values, out_dev);
  OP_HIP(h, hipGetLastError());
  return OP_OK;
}

int op_debug_clock_probe(op_handle* h, int spin_us, unsigned long long* out_dev, void* hip_stream) {
  if (!h || !out_dev || spin_us <= 0) return fail(h, OP_ERR_INVALID, "op_debug_clock_probe: bad argument");
  OP_HIP(h, hipSetDevice(h->cfg.device_id));
  hipLaunchKernelGGL(clock_probe_kernel, dim3(1), dim3(64), 0, (hipStream_t)hip_stream, (unsigned long long)spin_us * 100ull, out_dev);
  OP_HIP(h, hipGetLastError());
  return OP_OK;
}

int op_profile_reset(op_handle* h) {
  if (!h) return fail(nullptr, OP_ERR_INVALID, "op_profile_reset: NULL handle");
  int rc = drain_profile(h);
  for (int k = 0; k < PK_COUNT; ++k) {
    h->prof_ms[k] = 0;
    h->prof_launches[k] = 0;
  }
  return rc;
}

int op_profile_read(op_handle* h, op_profile_entry* entries, int max_entries) {
  if (!h || (!entries && max_entries > 0)) return fail(h, OP_ERR_INVALID, "op_profile_read: NULL argument");
  int rc = drain_profile(h);
  if (rc != OP_OK) return rc;
  int n = 0;
  for (int k = 0; k < PK_COUNT && n < max_entries; ++k) {
    if (h->prof_launches[k] == 0) continue;
    entries[n].kind = k;
    entries[n].launches = h->prof_launches[k];
    entries[n].total_ms = h->prof_ms[k];
    ++n;
  }
  return n;
}

// The batch's cu_seqlens on the host -- the caller's copy, or read back from the device (synchronises the stream once) -- held
// to what every pass over a packed batch relies on (opp::check_cu_seqlens).
static int host_cu_seqlens(op_handle* h, const PackedBatch& b, std::vector<int32_t>& cu_copy, const int32_t** cu_out) {
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
static int forward_packed_impl(op_handle* h, const PackedBatch& b, const HiddenReq* hid) {
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
  const opp::Layout lay = forward_layout(h, b.n_seqs, b.total_tokens, b.max_seqlen, h->set == OP_KS_F32);  // (= op_workspace_bytes)
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
      OP_TRY(ChunkPass(h, L, ws, b, s0, s1 - s0, rows, max_len, plan, hid).run());
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

int op_forward_packed(op_handle* h, const int32_t* ids_dev, const int32_t* cu_dev, const int32_t* cu_host_in, int n_seqs,
                      int total_tokens, int max_seqlen, float* prune_out, float* rank_out, float* keep_prob,
                      void* workspace, size_t workspace_bytes, void* hip_stream) {
  const PackedBatch b{ids_dev,  cu_dev,    cu_host_in, n_seqs,    total_tokens,    max_seqlen,
                      prune_out, rank_out, keep_prob,  workspace, workspace_bytes, reinterpret_cast<hipStream_t>(hip_stream)};
  return forward_packed_impl(h, b, nullptr);
}

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

// ---- op_attention_probs: the softmax probabilities of one layer, a side pass over that layer's input hidden state ----------
struct AttnProbsWorkspace {
  int32_t *roff, *row_seq, *row_pos, *row_tok;
  float *x, *ln, *q, *k;
  size_t bytes;
};

// (the regions in the order they are first written: row maps, the gathered state, LayerNorm(attn_norm), q and k)
static void carve_attention(const op_handle* h, char* base, int cap_rows_pad, int n_seqs, AttnProbsWorkspace& ws) {
  size_t off = 0;
  auto take = [&](size_t bytes) {
    char* p = base ? base + off : nullptr;
    off += align_up_sz(bytes, 256);
    return p;
  };
  const size_t R = (size_t)cap_rows_pad, plane = R * (size_t)h->H * sizeof(float);
  ws.roff = reinterpret_cast<int32_t*>(take(((size_t)n_seqs + 1) * 4));
  ws.row_seq = reinterpret_cast<int32_t*>(take(R * 4));
  ws.row_pos = reinterpret_cast<int32_t*>(take(R * 4));
  ws.row_tok = reinterpret_cast<int32_t*>(take(R * 4));
  ws.x = reinterpret_cast<float*>(take(plane));
  ws.ln = reinterpret_cast<float*>(take(plane));
  ws.q = reinterpret_cast<float*>(take(plane));
  ws.k = reinterpret_cast<float*>(take(plane));
  ws.bytes = off;
}

size_t op_attention_workspace_bytes(const op_handle* h, int n_seqs, int total_tokens, int max_seqlen) {
  if (!h || n_seqs < 0 || total_tokens < 0 || max_seqlen < 0) return 0;
  const int cap_pad = align_up(chunk_row_capacity(h, n_seqs, total_tokens, max_seqlen) + 64, 256);  // (as op_workspace_bytes)
  AttnProbsWorkspace ws;
  carve_attention(h, nullptr, cap_pad, n_seqs, ws);
  return ws.bytes;
}

// The part op_attention_probs and op_attention_rows share, after their own checks: workspace, chunks of sequences as the forward
// takes them, and per chunk the row map, the state's rows, LayerNorm(attn_norm), q | k with RoPE; `tail(ws, s0, ns, is_global)`
// then enqueues the call's own kernel over the chunk's q and k.
extern "C++" {
template <typename Tail>
static int attention_side_pass(op_handle* h, const char* what, const PackedBatch& b, int li, const float* hidden_dev, Tail&& tail) {
  if (!b.cu_dev || !b.workspace) return fail(h, OP_ERR_INVALID, "%s: NULL buffer", what);
  if ((reinterpret_cast<uintptr_t>(b.workspace) & 255) != 0) return fail(h, OP_ERR_WORKSPACE, "workspace must be 256-byte aligned");
  const size_t need = op_attention_workspace_bytes(h, b.n_seqs, b.total_tokens, b.max_seqlen);
  if (b.workspace_bytes < need) return fail(h, OP_ERR_WORKSPACE, "workspace has %zu bytes, need %zu", b.workspace_bytes, need);

  std::vector<int32_t> cu_copy;
  const int32_t* cu = nullptr;
  OP_TRY(host_cu_seqlens(h, b, cu_copy, &cu));

  const int H = h->H;
  const hipStream_t stream = b.stream;
  const bool is_global = h->cfg.layer_is_global[li] != 0;
  const float* attn_norm = li != 0 ? h->layers[li].attn_norm : nullptr;  // layer 0: the identity, as in the forward
  const int cap = chunk_row_capacity(h, b.n_seqs, b.total_tokens, b.max_seqlen);
  AttnProbsWorkspace ws;
  carve_attention(h, reinterpret_cast<char*>(b.workspace), align_up(cap + 64, 256), b.n_seqs, ws);

  int s0 = 0;
  while (s0 < b.n_seqs) {  // chunks of sequences, as the forward takes them
    int rows = 0, max_len = 0;
    const int s1 = opp::next_chunk(cu, s0, b.n_seqs, cap, &rows, &max_len);
    if (rows > cap) return fail(h, OP_ERR_WORKSPACE, "internal: chunk of %d rows exceeds capacity %d", rows, cap);
    const int ns = s1 - s0;
    const int r_pad = align_up(std::max(rows, 1), GEMM_BM);
    // row map; the state's rows (zero rows where the map holds no token); LayerNorm; q | k with RoPE, q scaled
    hipLaunchKernelGGL(seq_offsets_kernel, dim3(1), dim3(1024), 0, stream, b.cu_dev, s0, ns, ROW_ALIGN, ROW_ALIGN, ws.roff);
    hipLaunchKernelGGL(row_map_kernel, dim3((unsigned)((r_pad + 255) / 256)), dim3(256), 0, stream, b.cu_dev, s0, ns, ws.roff, r_pad,
                       ws.row_seq, ws.row_pos, ws.row_tok);
    opl::launch_attn_probs_gather(stream, hidden_dev, ws.row_tok, H, r_pad, ws.x);
    if (attn_norm) opl::launch_f32_ln(stream, ws.x, attn_norm, h->cfg.norm_eps, H, r_pad, ws.ln);
    F32GemmParams gp;
    memset(&gp, 0, sizeof(gp));
    gp.a = attn_norm ? ws.ln : ws.x;
    gp.w = reinterpret_cast<const float*>(h->layers[li].pack[W_QKV][PF_F32]);
    gp.K = H;
    gp.n_tiles = 2 * H / GEMM_BN;  // the q and k column tiles only
    gp.m_tiles = r_pad / GEMM_BM;
    gp.o0 = ws.q;
    gp.o1 = ws.k;
    gp.ld_out = H;
    gp.hidden = H;
    gp.inter = h->I;
    gp.row_pos = ws.row_pos;
    gp.rope_cos = h->rope_cos[is_global ? 1 : 0];
    gp.rope_sin = h->rope_sin[is_global ? 1 : 0];
    gp.max_pos = h->max_pos;
    if (!opl::launch_f32_gemm(stream, gp, F32_EPI_QKV)) return fail(h, OP_ERR_UNSUPPORTED, "internal: no fp32 GEMM epilogue %d", F32_EPI_QKV);
    tail(ws, s0, ns, is_global);
    OP_HIP(h, hipGetLastError());
    s0 = s1;
  }
  return OP_OK;
}
}  // extern "C++"

int op_attention_probs(op_handle* h, const int32_t* cu_dev, const int32_t* cu_host_in, int n_seqs, int total_tokens, int max_seqlen,
                       const op_attention_request* req, void* workspace, size_t workspace_bytes, void* hip_stream) {
  // (the request's own fields first: none of them needs the handle)
  if (!req) return fail(h, OP_ERR_INVALID, "op_attention_probs: the request is NULL");
  if (req->struct_bytes != sizeof(op_attention_request))
    return fail(h, OP_ERR_INVALID, "op_attention_probs: op_attention_request.struct_bytes is %u, expected %zu", req->struct_bytes,
                sizeof(op_attention_request));
  if (req->dtype != OP_HIDDEN_F32) return fail(h, OP_ERR_INVALID, "op_attention_probs: dtype %d is not OP_HIDDEN_F32", req->dtype);
  if (n_seqs < 0 || total_tokens < 0 || max_seqlen < 0) return fail(h, OP_ERR_INVALID, "op_attention_probs: negative size");
  const bool empty = n_seqs == 0 || total_tokens == 0;
  if (req->pad_width < 0 || req->pad_width < max_seqlen || (!empty && req->pad_width == 0))
    return fail(h, OP_ERR_INVALID, "op_attention_probs: pad_width %d below max_seqlen %d", req->pad_width, max_seqlen);
  if (!empty && !req->hidden_dev) return fail(h, OP_ERR_INVALID, "op_attention_probs: hidden_dev is NULL");
  if (!empty && !req->out_dev) return fail(h, OP_ERR_INVALID, "op_attention_probs: out_dev is NULL");
  if ((size_t)n_seqs * (size_t)req->pad_width > (size_t)INT32_MAX)  // (output rows are 32-bit indices inside a sequence's matrices)
    return fail(h, OP_ERR_INVALID, "op_attention_probs: %zu output rows per head exceed 2^31 - 1", (size_t)n_seqs * (size_t)req->pad_width);
  if (!h) return fail(nullptr, OP_ERR_INVALID, "op_attention_probs: NULL handle");
  if (req->layer < 0 || req->layer >= h->N)
    return fail(h, OP_ERR_INVALID, "op_attention_probs: layer %d outside 0 .. %d", req->layer, h->N - 1);
  if (!h->f32_packs)
    return fail(h, OP_ERR_UNSUPPORTED, "op_attention_probs: the pass needs the fp32 weight packs: create the handle with OP_FLAG_F32_PACKS");
  if (op_weights_ready(h) != OP_OK) return OP_ERR_STATE;

  OP_HIP(h, hipSetDevice(h->cfg.device_id));
  hipStream_t stream = reinterpret_cast<hipStream_t>(hip_stream);
  const int width = req->pad_width;
  const size_t mat_elems = (size_t)h->nh * (size_t)width * (size_t)width;  // one sequence
  float* out = reinterpret_cast<float*>(req->out_dev);
  if (n_seqs == 0 || width == 0) return OP_OK;
  if (total_tokens == 0) {  // only empty sequences: every row is padding
    OP_HIP(h, hipMemsetAsync(out, 0, (size_t)n_seqs * mat_elems * sizeof(float), stream));
    return OP_OK;
  }
  PackedBatch b;
  b.cu_dev = cu_dev, b.cu_host = cu_host_in, b.n_seqs = n_seqs, b.total_tokens = total_tokens, b.max_seqlen = max_seqlen;
  b.workspace = workspace, b.workspace_bytes = workspace_bytes, b.stream = stream;
  return attention_side_pass(h, "op_attention_probs", b, req->layer, req->hidden_dev,
                             [&](const AttnProbsWorkspace& ws, int s0, int ns, bool is_global) {
                               AttnProbsParams ap;
                               ap.q = ws.q;
                               ap.k = ws.k;
                               ap.out = out;
                               ap.cu = cu_dev;
                               ap.s0 = s0;
                               ap.roff = ws.roff;
                               ap.H = h->H;
                               ap.num_heads = h->nh;
                               ap.window = is_global ? -1 : h->cfg.local_attention / 2;
                               ap.width = width;
                               ap.wide = (width % 4 == 0 && (reinterpret_cast<uintptr_t>(out) & 15) == 0) ? 1 : 0;
                               opl::launch_attn_probs(stream, ap, ns);
                             });
}

// ---- op_attention_rows: one query row per sequence of op_attention_probs' matrices, per head or as the mean over heads --------
int op_attention_rows(op_handle* h, const int32_t* cu_dev, const int32_t* cu_host_in, int n_seqs, int total_tokens, int max_seqlen,
                      const op_attention_rows_request* req, void* workspace, size_t workspace_bytes, void* hip_stream) {
  // (the request's own fields first: none of them needs the handle)
  if (!req) return fail(h, OP_ERR_INVALID, "op_attention_rows: the request is NULL");
  if (req->struct_bytes != sizeof(op_attention_rows_request))
    return fail(h, OP_ERR_INVALID, "op_attention_rows: op_attention_rows_request.struct_bytes is %u, expected %zu", req->struct_bytes,
                sizeof(op_attention_rows_request));
  if (req->reduce_heads != 0 && req->reduce_heads != 1)
    return fail(h, OP_ERR_INVALID, "op_attention_rows: reduce_heads %d is neither 0 nor 1", req->reduce_heads);
  if (n_seqs < 0 || total_tokens < 0 || max_seqlen < 0) return fail(h, OP_ERR_INVALID, "op_attention_rows: negative size");
  const bool empty = n_seqs == 0 || total_tokens == 0;
  if (req->pad_width < 0 || req->pad_width < max_seqlen || (!empty && req->pad_width == 0))
    return fail(h, OP_ERR_INVALID, "op_attention_rows: pad_width %d below max_seqlen %d", req->pad_width, max_seqlen);
  if (!empty && !req->hidden_dev) return fail(h, OP_ERR_INVALID, "op_attention_rows: hidden_dev is NULL");
  if (!empty && !req->out_dev) return fail(h, OP_ERR_INVALID, "op_attention_rows: out_dev is NULL");
  if (req->query_pos_host && !req->query_pos_dev)
    return fail(h, OP_ERR_INVALID, "op_attention_rows: query_pos_host without query_pos_dev");
  if (req->query_pos_host)
    for (int s = 0; s < n_seqs; ++s)
      if (req->query_pos_host[s] < 0)
        return fail(h, OP_ERR_INVALID, "op_attention_rows: query position %d of sequence %d is negative", req->query_pos_host[s], s);
  if (!h) return fail(nullptr, OP_ERR_INVALID, "op_attention_rows: NULL handle");
  if (req->layer < 0 || req->layer >= h->N)
    return fail(h, OP_ERR_INVALID, "op_attention_rows: layer %d outside 0 .. %d", req->layer, h->N - 1);
  if (!h->f32_packs)
    return fail(h, OP_ERR_UNSUPPORTED, "op_attention_rows: the pass needs the fp32 weight packs: create the handle with OP_FLAG_F32_PACKS");
  const bool head_mean = req->reduce_heads != 0;
  if (head_mean && h->nh > AR_MAX_HEADS)
    return fail(h, OP_ERR_UNSUPPORTED, "op_attention_rows: reduce_heads with %d heads (at most %d)", h->nh, AR_MAX_HEADS);
  if (op_weights_ready(h) != OP_OK) return OP_ERR_STATE;

  OP_HIP(h, hipSetDevice(h->cfg.device_id));
  hipStream_t stream = reinterpret_cast<hipStream_t>(hip_stream);
  const int width = req->pad_width;
  const size_t row_elems = (head_mean ? (size_t)1 : (size_t)h->nh) * (size_t)width;  // one sequence
  float* out = req->out_dev;
  if (n_seqs == 0 || width == 0) return OP_OK;
  if (total_tokens == 0) {  // only empty sequences: no position lies inside one
    OP_HIP(h, hipMemsetAsync(out, 0, (size_t)n_seqs * row_elems * sizeof(float), stream));
    return OP_OK;
  }
  PackedBatch b;
  b.cu_dev = cu_dev, b.cu_host = cu_host_in, b.n_seqs = n_seqs, b.total_tokens = total_tokens, b.max_seqlen = max_seqlen;
  b.workspace = workspace, b.workspace_bytes = workspace_bytes, b.stream = stream;
  return attention_side_pass(h, "op_attention_rows", b, req->layer, req->hidden_dev,
                             [&](const AttnProbsWorkspace& ws, int s0, int ns, bool is_global) {
                               AttnRowsParams ar;
                               ar.q = ws.q;
                               ar.k = ws.k;
                               ar.out = out;
                               ar.cu = cu_dev;
                               ar.qpos = req->query_pos_dev;
                               ar.s0 = s0;
                               ar.roff = ws.roff;
                               ar.H = h->H;
                               ar.num_heads = h->nh;
                               ar.window = is_global ? -1 : h->cfg.local_attention / 2;
                               ar.width = width;
                               opl::launch_attn_rows(stream, ar, ns, head_mean);
                             });
}

int op_pack_padded(op_handle* h, const void* ids_dev, int ids_dtype, const void* mask_dev, int mask_dtype, int n_rows, int width,
                   int32_t* ids_packed_dev, int32_t* cu_seqlens_dev, int32_t* cu_seqlens_host, op_padded_report* report,
                   void* hip_stream) {
  // (the arguments' own fields first: none of them needs the handle)
  if (!report) return fail(h, OP_ERR_INVALID, "op_pack_padded: report is NULL");
  if (report->struct_bytes != sizeof(op_padded_report))
    return fail(h, OP_ERR_INVALID, "op_pack_padded: op_padded_report.struct_bytes is %u, expected %zu", report->struct_bytes,
                sizeof(op_padded_report));
  if (ids_dtype != OP_INT_I32 && ids_dtype != OP_INT_I64)
    return fail(h, OP_ERR_INVALID, "op_pack_padded: ids_dtype %d is neither OP_INT_I32 nor OP_INT_I64", ids_dtype);
  if (mask_dev && mask_dtype != OP_INT_I32 && mask_dtype != OP_INT_I64 && mask_dtype != OP_INT_U8)
    return fail(h, OP_ERR_INVALID, "op_pack_padded: unknown mask_dtype %d", mask_dtype);
  if (n_rows < 0) return fail(h, OP_ERR_INVALID, "op_pack_padded: negative n_rows %d", n_rows);
  if (width < 0) return fail(h, OP_ERR_INVALID, "op_pack_padded: negative width %d", width);
  const int64_t cells = (int64_t)n_rows * (int64_t)width;
  if (cells > (int64_t)INT32_MAX)  // (the first offender of each check is a 32-bit linear index)
    return fail(h, OP_ERR_INVALID, "op_pack_padded: n_rows * width = %lld exceeds 2^31 - 1", (long long)cells);
  if (!cu_seqlens_dev) return fail(h, OP_ERR_INVALID, "op_pack_padded: cu_seqlens_dev is NULL");
  if (!cu_seqlens_host) return fail(h, OP_ERR_INVALID, "op_pack_padded: cu_seqlens_host is NULL");
  if (cells > 0 && !ids_dev) return fail(h, OP_ERR_INVALID, "op_pack_padded: ids_dev is NULL");
  if (cells > 0 && !ids_packed_dev) return fail(h, OP_ERR_INVALID, "op_pack_padded: ids_packed_dev is NULL");
  if (!h) return fail(nullptr, OP_ERR_INVALID, "op_pack_padded: NULL handle");
  report->total_tokens = report->max_seqlen = report->status = 0;
  report->mask_row = report->mask_col = report->id_row = report->id_col = -1;
  report->id_value = 0;

  OP_HIP(h, hipSetDevice(h->cfg.device_id));
  hipStream_t stream = reinterpret_cast<hipStream_t>(hip_stream);
  hipStreamCaptureStatus capturing = hipStreamCaptureStatusNone;
  OP_HIP(h, hipStreamIsCapturing(stream, &capturing));
  if (capturing != hipStreamCaptureStatusNone)
    return fail(h, OP_ERR_STATE, "op_pack_padded: the stream is being captured (the call synchronises it to read the batch's size back)");
  if (cells == 0) {  // nothing to launch: every row is empty
    OP_HIP(h, hipMemsetAsync(cu_seqlens_dev, 0, ((size_t)n_rows + 1) * sizeof(int32_t), stream));
    std::fill(cu_seqlens_host, cu_seqlens_host + n_rows + 1, 0);
    return OP_OK;
  }
  if (!h->pad_status) OP_TRY(dev_alloc(h, &h->pad_status, (size_t)opk::PAD_ST_WORDS));
  const size_t n_cu = (size_t)n_rows + 1, words = n_cu + opk::PAD_ST_WORDS;
  if (h->pad_host_words < words) {
    if (h->pad_host) (void)hipHostFree(h->pad_host);
    h->pad_host = nullptr;
    h->pad_host_words = 0;
    void* p = nullptr;
    const size_t grown = std::max<size_t>(words, 4096);
    hipError_t e = hipHostMalloc(&p, grown * sizeof(int32_t), hipHostMallocDefault);
    if (e != hipSuccess) return fail(h, OP_ERR_NOMEM, "hipHostMalloc(%zu bytes) failed: %s", grown * sizeof(int32_t), hipGetErrorString(e));
    h->pad_host = reinterpret_cast<int32_t*>(p);
    h->pad_host_words = grown;
  }
  OP_HIP(h, hipMemsetAsync(h->pad_status, 0xff, 2 * sizeof(uint32_t), stream));  // the two atomicMin words = PAD_ST_NONE
  if (!opl::launch_padded_pack(stream, ids_dev, ids_dtype, mask_dev, mask_dtype, n_rows, width, h->V, ids_packed_dev, cu_seqlens_dev,
                               h->pad_status))
    return fail(h, OP_ERR_UNSUPPORTED, "op_pack_padded: no kernel for ids_dtype %d / mask_dtype %d", ids_dtype, mask_dtype);
  OP_HIP(h, hipGetLastError());
  uint32_t* st_host = reinterpret_cast<uint32_t*>(h->pad_host + n_cu);
  OP_HIP(h, hipMemcpyAsync(h->pad_host, cu_seqlens_dev, n_cu * sizeof(int32_t), hipMemcpyDeviceToHost, stream));
  OP_HIP(h, hipMemcpyAsync(st_host, h->pad_status, opk::PAD_ST_WORDS * sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
  OP_HIP(h, hipStreamSynchronize(stream));  // the one synchronisation: the forward's grids need T and the longest row
  std::memcpy(cu_seqlens_host, h->pad_host, n_cu * sizeof(int32_t));
  report->total_tokens = (int32_t)st_host[opk::PAD_ST_TOTAL];
  report->max_seqlen = (int32_t)st_host[opk::PAD_ST_MAXLEN];
  const uint32_t bad_mask = st_host[opk::PAD_ST_MASK], bad_id = st_host[opk::PAD_ST_ID];
  if (bad_mask != opk::PAD_ST_NONE) {
    report->status |= 1;
    report->mask_row = (int32_t)(bad_mask / (uint32_t)width);
    report->mask_col = (int32_t)(bad_mask % (uint32_t)width);
  }
  if (bad_id != opk::PAD_ST_NONE) {
    report->status |= 2;
    report->id_row = (int32_t)(bad_id / (uint32_t)width);
    report->id_col = (int32_t)(bad_id % (uint32_t)width);
    report->id_value = (int64_t)((uint64_t)st_host[opk::PAD_ST_IDVAL] | ((uint64_t)st_host[opk::PAD_ST_IDVAL + 1] << 32));
  }
  if (report->status == 0) return OP_OK;
  char mask_text[160] = "", id_text[200] = "";
  if (report->status & 1)
    snprintf(mask_text, sizeof(mask_text), "the attention mask is not ones-then-zeros at row %d, column %d", report->mask_row, report->mask_col);
  if (report->status & 2)
    snprintf(id_text, sizeof(id_text), "token id %lld at row %d, column %d is outside the embedding table (vocab_size %d)",
             (long long)report->id_value, report->id_row, report->id_col, h->V);
  return fail(h, OP_ERR_INVALID, "op_pack_padded: %s%s%s", mask_text, report->status == 3 ? "; " : "", id_text);
}

int op_unpack_padded(op_handle* h, const float* packed_dev, const int32_t* cu_seqlens_dev, int n_rows, int width, int channels,
                     float* padded_dev, void* hip_stream) {
  if (channels != 1 && channels != 2) return fail(h, OP_ERR_INVALID, "op_unpack_padded: channels is %d, expected 1 or 2", channels);
  if (n_rows < 0) return fail(h, OP_ERR_INVALID, "op_unpack_padded: negative n_rows %d", n_rows);
  if (width < 0) return fail(h, OP_ERR_INVALID, "op_unpack_padded: negative width %d", width);
  const int64_t cells = (int64_t)n_rows * (int64_t)width;
  if (cells > (int64_t)INT32_MAX)
    return fail(h, OP_ERR_INVALID, "op_unpack_padded: n_rows * width = %lld exceeds 2^31 - 1", (long long)cells);
  if (cells > 0 && !packed_dev) return fail(h, OP_ERR_INVALID, "op_unpack_padded: packed_dev is NULL");
  if (cells > 0 && !cu_seqlens_dev) return fail(h, OP_ERR_INVALID, "op_unpack_padded: cu_seqlens_dev is NULL");
  if (cells > 0 && !padded_dev) return fail(h, OP_ERR_INVALID, "op_unpack_padded: padded_dev is NULL");
  if (!h) return fail(nullptr, OP_ERR_INVALID, "op_unpack_padded: NULL handle");
  if (cells == 0) return OP_OK;
  OP_HIP(h, hipSetDevice(h->cfg.device_id));
  if (!opl::launch_padded_scatter(reinterpret_cast<hipStream_t>(hip_stream), packed_dev, cu_seqlens_dev, n_rows, width, channels, padded_dev))
    return fail(h, OP_ERR_UNSUPPORTED, "op_unpack_padded: no kernel for %d channels", channels);
  OP_HIP(h, hipGetLastError());
  return OP_OK;
}

int op_loss(op_handle* h, const op_loss_request* req, float* loss_dev, op_loss_report* report, void* hip_stream) {
  // (the arguments' own fields first: none of them needs the handle)
  if (!req) return fail(h, OP_ERR_INVALID, "op_loss: request is NULL");
  if (req->struct_bytes != sizeof(op_loss_request))
    return fail(h, OP_ERR_INVALID, "op_loss: op_loss_request.struct_bytes is %u, expected %zu", req->struct_bytes, sizeof(op_loss_request));
  if (report && report->struct_bytes != sizeof(op_loss_report))
    return fail(h, OP_ERR_INVALID, "op_loss: op_loss_report.struct_bytes is %u, expected %zu", report->struct_bytes, sizeof(op_loss_report));
  const int kind = req->kind, dtype = req->labels_dtype;
  if (kind < OP_LOSS_TOKEN_CE || kind > OP_LOSS_RANK_MSE) return fail(h, OP_ERR_INVALID, "op_loss: unknown kind %d", kind);
  if (dtype != OP_INT_I32 && dtype != OP_INT_I64 && dtype != OP_INT_U8 && dtype != OP_LABELS_F32)
    return fail(h, OP_ERR_INVALID, "op_loss: unknown labels_dtype %d", dtype);
  const bool token = kind == OP_LOSS_TOKEN_CE, integer = token || kind == OP_LOSS_RANK_CE;
  if (integer ? (dtype != OP_INT_I32 && dtype != OP_INT_I64) : dtype != OP_LABELS_F32)
    return fail(h, OP_ERR_INVALID, "op_loss: labels_dtype %d does not fit kind %d (%s)", dtype, kind,
                integer ? "OP_INT_I32 or OP_INT_I64" : "OP_LABELS_F32");
  if (req->n_rows < 0) return fail(h, OP_ERR_INVALID, "op_loss: negative n_rows %d", req->n_rows);
  if (req->channels < 0) return fail(h, OP_ERR_INVALID, "op_loss: negative channels %d", req->channels);
  if (token && req->width < 0) return fail(h, OP_ERR_INVALID, "op_loss: negative width %d", req->width);
  if (token && req->total_tokens < 0) return fail(h, OP_ERR_INVALID, "op_loss: negative total_tokens %d", req->total_tokens);
  if (token && req->channels != 2) return fail(h, OP_ERR_INVALID, "op_loss: channels is %d, OP_LOSS_TOKEN_CE takes 2", req->channels);
  if (kind == OP_LOSS_RANK_BCE && req->channels != 1)
    return fail(h, OP_ERR_INVALID, "op_loss: channels is %d, OP_LOSS_RANK_BCE takes 1", req->channels);
  if (kind == OP_LOSS_RANK_CE && req->channels < 2)
    return fail(h, OP_ERR_INVALID, "op_loss: channels is %d, OP_LOSS_RANK_CE takes at least 2", req->channels);
  const int64_t label_cells = (int64_t)req->n_rows * (int64_t)(token ? req->width : kind == OP_LOSS_RANK_MSE ? req->channels : 1);
  const int64_t logit_rows = token ? (int64_t)req->total_tokens : (int64_t)req->n_rows;
  if (token && label_cells > (int64_t)INT32_MAX)  // (the first offender is a 32-bit linear index)
    return fail(h, OP_ERR_INVALID, "op_loss: n_rows * width = %lld exceeds 2^31 - 1", (long long)label_cells);
  if (!token && (int64_t)req->n_rows * (int64_t)req->channels > (int64_t)INT32_MAX)
    return fail(h, OP_ERR_INVALID, "op_loss: n_rows * channels = %lld exceeds 2^31 - 1", (long long)req->n_rows * req->channels);
  if (token && (int64_t)req->total_tokens > label_cells)
    return fail(h, OP_ERR_INVALID, "op_loss: total_tokens %d exceeds n_rows * width = %lld", req->total_tokens, (long long)label_cells);
  if (!loss_dev) return fail(h, OP_ERR_INVALID, "op_loss: loss_dev is NULL");
  if (logit_rows * req->channels > 0 && !req->logits_dev) return fail(h, OP_ERR_INVALID, "op_loss: logits_dev is NULL");
  if (label_cells > 0 && !req->labels_dev) return fail(h, OP_ERR_INVALID, "op_loss: labels_dev is NULL");
  if (token && req->n_rows > 0 && !req->cu_seqlens_dev) return fail(h, OP_ERR_INVALID, "op_loss: cu_seqlens_dev is NULL");
  if (!h) return fail(nullptr, OP_ERR_INVALID, "op_loss: NULL handle");
  if (report) {
    report->status = 0;
    report->bad_row = report->bad_col = -1;
    report->bad_value = report->count = 0;
    report->sum = 0.0;
    report->loss = 0.0f;
    report->reserved = 0;
  }

  OP_HIP(h, hipSetDevice(h->cfg.device_id));
  hipStream_t stream = reinterpret_cast<hipStream_t>(hip_stream);
  if (report) {
    hipStreamCaptureStatus capturing = hipStreamCaptureStatusNone;
    OP_HIP(h, hipStreamIsCapturing(stream, &capturing));
    if (capturing != hipStreamCaptureStatusNone)
      return fail(h, OP_ERR_STATE, "op_loss: the stream is being captured (a call with a report synchronises it to read the result back)");
    if (!h->loss_host) {
      void* p = nullptr;
      hipError_t e = hipHostMalloc(&p, sizeof(opk::LossResult), hipHostMallocDefault);
      if (e != hipSuccess) return fail(h, OP_ERR_NOMEM, "hipHostMalloc(%zu bytes) failed: %s", sizeof(opk::LossResult), hipGetErrorString(e));
      h->loss_host = reinterpret_cast<opk::LossResult*>(p);
    }
  }
  opk::LossParams lp;
  lp.logits = req->logits_dev;
  lp.labels = req->labels_dev;
  lp.cu = token ? req->cu_seqlens_dev : nullptr;
  lp.terms = req->terms_dev;
  lp.n_rows = req->n_rows;
  lp.width = token ? req->width : 0;
  lp.channels = req->channels;
  lp.total_tokens = token ? req->total_tokens : 0;
  lp.ignore_index = (long long)req->ignore_index;
  if (!opl::launch_loss(stream, kind, dtype, lp, h->loss_scratch, loss_dev))
    return fail(h, OP_ERR_UNSUPPORTED, "op_loss: no kernel for kind %d / labels_dtype %d", kind, dtype);
  OP_HIP(h, hipGetLastError());
  if (!report) return OP_OK;
  OP_HIP(h, hipMemcpyAsync(h->loss_host, &h->loss_scratch->result, sizeof(opk::LossResult), hipMemcpyDeviceToHost, stream));
  OP_HIP(h, hipStreamSynchronize(stream));  // the one synchronisation: the caller asked for the result on the host
  const opk::LossResult& res = *h->loss_host;
  report->count = (int64_t)res.count;
  report->sum = res.sum;
  report->loss = res.loss;
  if (res.status == 0) return OP_OK;
  report->status = 1;
  report->bad_value = (int64_t)res.bad_value;
  report->bad_row = token ? (int32_t)(res.bad_index / (uint32_t)req->width) : (int32_t)res.bad_index;
  report->bad_col = token ? (int32_t)(res.bad_index % (uint32_t)req->width) : 0;
  return fail(h, OP_ERR_INVALID, "op_loss: label %lld at row %d, column %d is outside 0 <= label < %d and is not ignore_index (%lld)",
              (long long)report->bad_value, report->bad_row, report->bad_col, req->channels, (long long)req->ignore_index);
}

// The coverage belongs to one arithmetic: the kernel set (and the layer mask of sets 8 / 9) it was collected under.  It is
// emptied lazily, on the stream of the call that next looks at it -- after op_coverage_reset / op_calibrate / op_load_weight
// of the embedding table, and whenever the handle runs another arithmetic than the one the coverage belongs to.  So
// op_select_kernel_set enqueues nothing (the default audit mode never pays for a feature it does not use), and an audit's
// detour through the reference set and back finds the coverage as it left it.
static int coverage_prepare(op_handle* h, hipStream_t stream) {
  OP_HIP(h, hipSetDevice(h->cfg.device_id));
  const int set = h->resolved ? h->set : -2;
  const uint64_t mlp = (h->resolved && mlp_by_layer(*h->ks)) ? h->mlp_layers : 0ull;
  if (h->cov_clear || set != h->cov_set || mlp != h->cov_mlp_layers) {
    OP_HIP(h, hipMemsetAsync(h->cov_bits, 0, (((size_t)h->V + 31) / 32) * sizeof(uint32_t), stream));
    OP_HIP(h, hipMemsetAsync(h->cov_state, 0, opl::COV_WORDS * sizeof(uint32_t), stream));
    h->cov_clear = false;
    h->cov_set = set;
    h->cov_mlp_layers = mlp;
  }
  return OP_OK;
}

int op_coverage_scan(op_handle* h, const int32_t* ids_dev, const int32_t* cu_seqlens_dev, int n_seqs, int total_tokens,
                     int32_t* row_novel_dev, op_coverage_report* report, void* hip_stream) {
  // (the arguments' own fields first: none of them needs the handle)
  if (!report) return fail(h, OP_ERR_INVALID, "op_coverage_scan: report is NULL");
  if (report->struct_bytes != sizeof(op_coverage_report))
    return fail(h, OP_ERR_INVALID, "op_coverage_scan: op_coverage_report.struct_bytes is %u, expected %zu", report->struct_bytes,
                sizeof(op_coverage_report));
  if (n_seqs < 0) return fail(h, OP_ERR_INVALID, "op_coverage_scan: negative n_seqs %d", n_seqs);
  if (total_tokens < 0) return fail(h, OP_ERR_INVALID, "op_coverage_scan: negative total_tokens %d", total_tokens);
  if (n_seqs > 0 && !cu_seqlens_dev) return fail(h, OP_ERR_INVALID, "op_coverage_scan: cu_seqlens_dev is NULL");
  if (n_seqs > 0 && !row_novel_dev) return fail(h, OP_ERR_INVALID, "op_coverage_scan: row_novel_dev is NULL");
  if (n_seqs > 0 && total_tokens > 0 && !ids_dev) return fail(h, OP_ERR_INVALID, "op_coverage_scan: ids_dev is NULL");
  if (!h) return fail(nullptr, OP_ERR_INVALID, "op_coverage_scan: NULL handle");
  report->novel_tokens = report->longest_row_tokens = report->max_audited_tokens = 0;
  report->longest_row = -1;

  OP_HIP(h, hipSetDevice(h->cfg.device_id));
  hipStream_t stream = reinterpret_cast<hipStream_t>(hip_stream);
  hipStreamCaptureStatus capturing = hipStreamCaptureStatusNone;
  OP_HIP(h, hipStreamIsCapturing(stream, &capturing));
  if (capturing != hipStreamCaptureStatusNone)
    return fail(h, OP_ERR_STATE, "op_coverage_scan: the stream is being captured (the call synchronises it to read the report back)");
  if (!h->cov_host) {
    void* p = nullptr;
    hipError_t e = hipHostMalloc(&p, opl::COV_WORDS * sizeof(uint32_t), hipHostMallocDefault);
    if (e != hipSuccess) return fail(h, OP_ERR_NOMEM, "hipHostMalloc(%zu bytes) failed: %s", opl::COV_WORDS * sizeof(uint32_t), hipGetErrorString(e));
    h->cov_host = reinterpret_cast<uint32_t*>(p);
  }
  OP_TRY(coverage_prepare(h, stream));
  OP_HIP(h, hipMemsetAsync(h->cov_state + opl::COV_NOVEL, 0, (opl::COV_WORDS - opl::COV_NOVEL) * sizeof(uint32_t), stream));
  if (n_seqs > 0) {
    opl::launch_coverage_scan(stream, ids_dev, cu_seqlens_dev, n_seqs, total_tokens, h->V, h->cov_bits, row_novel_dev, h->cov_state);
    OP_HIP(h, hipGetLastError());
  }
  OP_HIP(h, hipMemcpyAsync(h->cov_host, h->cov_state, opl::COV_WORDS * sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
  OP_HIP(h, hipStreamSynchronize(stream));  // the one synchronisation: the caller decides on the host whether to audit
  report->max_audited_tokens = (int32_t)h->cov_host[opl::COV_MAXLEN];
  report->novel_tokens = (int32_t)h->cov_host[opl::COV_NOVEL];
  if (n_seqs > 0) {
    report->longest_row_tokens = (int32_t)h->cov_host[opl::COV_LONGEST + 1];
    report->longest_row = (int32_t)~h->cov_host[opl::COV_LONGEST];
  }
  return OP_OK;
}

// the checks commit, gather and compare share: a packed batch and a list of its rows
static int check_row_list(op_handle* h, const char* who, const void* cu_seqlens_dev, int n_seqs, int total_tokens, const void* rows_dev,
                          int n_rows) {
  if (n_seqs < 0) return fail(h, OP_ERR_INVALID, "%s: negative n_seqs %d", who, n_seqs);
  if (total_tokens < 0) return fail(h, OP_ERR_INVALID, "%s: negative total_tokens %d", who, total_tokens);
  if (n_rows < 0) return fail(h, OP_ERR_INVALID, "%s: negative n_rows %d", who, n_rows);
  if (n_rows > 0 && !cu_seqlens_dev) return fail(h, OP_ERR_INVALID, "%s: cu_seqlens_dev is NULL", who);
  if (n_rows > 0 && !rows_dev) return fail(h, OP_ERR_INVALID, "%s: rows_dev is NULL", who);
  return OP_OK;
}

int op_coverage_commit(op_handle* h, const int32_t* ids_dev, const int32_t* cu_seqlens_dev, int n_seqs, int total_tokens,
                       const int32_t* rows_dev, int n_rows, void* hip_stream) {
  OP_TRY(check_row_list(h, "op_coverage_commit", cu_seqlens_dev, n_seqs, total_tokens, rows_dev, n_rows));
  if (n_rows > 0 && total_tokens > 0 && !ids_dev) return fail(h, OP_ERR_INVALID, "op_coverage_commit: ids_dev is NULL");
  if (!h) return fail(nullptr, OP_ERR_INVALID, "op_coverage_commit: NULL handle");
  hipStream_t stream = reinterpret_cast<hipStream_t>(hip_stream);
  OP_TRY(coverage_prepare(h, stream));
  if (n_rows == 0) return OP_OK;
  opl::launch_coverage_commit(stream, ids_dev, cu_seqlens_dev, n_seqs, total_tokens, rows_dev, n_rows, h->V, h->cov_bits, h->cov_state);
  OP_HIP(h, hipGetLastError());
  return OP_OK;
}

int op_coverage_reset(op_handle* h) {
  if (!h) return fail(nullptr, OP_ERR_INVALID, "op_coverage_reset: NULL handle");
  h->cov_clear = true;
  return OP_OK;
}

int op_gather_rows(op_handle* h, const int32_t* ids_dev, const int32_t* cu_seqlens_dev, int n_seqs, int total_tokens,
                   const int32_t* rows_dev, int n_rows, int32_t* sub_ids_dev, int32_t* sub_cu_dev, void* hip_stream) {
  OP_TRY(check_row_list(h, "op_gather_rows", cu_seqlens_dev, n_seqs, total_tokens, rows_dev, n_rows));
  if (!sub_cu_dev) return fail(h, OP_ERR_INVALID, "op_gather_rows: sub_cu_dev is NULL");
  if (n_rows > 0 && total_tokens > 0 && !ids_dev) return fail(h, OP_ERR_INVALID, "op_gather_rows: ids_dev is NULL");
  if (n_rows > 0 && total_tokens > 0 && !sub_ids_dev) return fail(h, OP_ERR_INVALID, "op_gather_rows: sub_ids_dev is NULL");
  if (!h) return fail(nullptr, OP_ERR_INVALID, "op_gather_rows: NULL handle");
  OP_HIP(h, hipSetDevice(h->cfg.device_id));
  hipStream_t stream = reinterpret_cast<hipStream_t>(hip_stream);
  if (n_rows == 0) {
    OP_HIP(h, hipMemsetAsync(sub_cu_dev, 0, sizeof(int32_t), stream));
    return OP_OK;
  }
  opl::launch_gather_rows(stream, ids_dev, cu_seqlens_dev, n_seqs, total_tokens, rows_dev, n_rows, sub_ids_dev, sub_cu_dev);
  OP_HIP(h, hipGetLastError());
  return OP_OK;
}

int op_audit_compare(op_handle* h, const float* prune_dev, const float* rank_dev, const int32_t* cu_seqlens_dev, int n_seqs,
                     int total_tokens, const int32_t* rows_dev, int n_rows, const float* sub_prune_dev, const float* sub_rank_dev,
                     const int32_t* sub_cu_dev, float* err_dev, void* hip_stream) {
  OP_TRY(check_row_list(h, "op_audit_compare", cu_seqlens_dev, n_seqs, total_tokens, rows_dev, n_rows));
  if (!err_dev) return fail(h, OP_ERR_INVALID, "op_audit_compare: err_dev is NULL");
  if (n_rows > 0 && total_tokens > 0 && (!prune_dev || !sub_prune_dev)) return fail(h, OP_ERR_INVALID, "op_audit_compare: prune_dev / sub_prune_dev is NULL");
  if (n_rows > 0 && (!rank_dev || !sub_rank_dev)) return fail(h, OP_ERR_INVALID, "op_audit_compare: rank_dev / sub_rank_dev is NULL");
  if (n_rows > 0 && !sub_cu_dev) return fail(h, OP_ERR_INVALID, "op_audit_compare: sub_cu_dev is NULL");
  if (!h) return fail(nullptr, OP_ERR_INVALID, "op_audit_compare: NULL handle");
  OP_HIP(h, hipSetDevice(h->cfg.device_id));
  hipStream_t stream = reinterpret_cast<hipStream_t>(hip_stream);
  OP_HIP(h, hipMemsetAsync(err_dev, 0, sizeof(float), stream));  // +0.0: the kernel's atomicMax starts from it
  if (n_rows == 0) return OP_OK;
  opl::launch_audit_compare(stream, prune_dev, rank_dev, cu_seqlens_dev, n_seqs, total_tokens, rows_dev, n_rows, sub_prune_dev, sub_rank_dev,
                            sub_cu_dev, h->nl, err_dev);
  OP_HIP(h, hipGetLastError());
  return OP_OK;
}

int op_assemble_rows(op_handle* h, const op_assemble_request* req, int32_t* ids_dev, void* hip_stream) {
  // (the request's own fields first, on the host copies: nothing is enqueued before the last check)
  if (!req) return fail(h, OP_ERR_INVALID, "op_assemble_rows: request is NULL");
  if (req->struct_bytes != sizeof(op_assemble_request))
    return fail(h, OP_ERR_INVALID, "op_assemble_rows: op_assemble_request.struct_bytes is %u, expected %zu", req->struct_bytes,
                sizeof(op_assemble_request));
  if (req->n_frag < 0 || req->n_queries < 0 || req->n_rows < 0 || req->total_tokens < 0)
    return fail(h, OP_ERR_INVALID, "op_assemble_rows: negative count (n_frag %d, n_queries %d, n_rows %d, total_tokens %d)", req->n_frag,
                req->n_queries, req->n_rows, req->total_tokens);
  const int32_t* const pieces[3] = {req->prefix, req->middle, req->suffix};
  const int n_pieces[3] = {req->n_prefix, req->n_middle, req->n_suffix};
  static const char* const piece_names[3] = {"prefix", "middle", "suffix"};
  for (int i = 0; i < 3; ++i) {
    if (n_pieces[i] < 0 || n_pieces[i] > OP_ASSEMBLE_MAX_PIECE)
      return fail(h, OP_ERR_INVALID, "op_assemble_rows: %s holds %d ids, expected 0 .. %d", piece_names[i], n_pieces[i], OP_ASSEMBLE_MAX_PIECE);
    if (n_pieces[i] > 0 && !pieces[i]) return fail(h, OP_ERR_INVALID, "op_assemble_rows: %s is NULL", piece_names[i]);
  }
  if (req->n_rows == 0) {
    if (req->total_tokens != 0) return fail(h, OP_ERR_INVALID, "op_assemble_rows: no rows but total_tokens is %d", req->total_tokens);
    if (!h) return fail(nullptr, OP_ERR_INVALID, "op_assemble_rows: NULL handle");
    return OP_OK;
  }
  if (!req->plan_dev || !req->plan_host || !req->cu_seqlens_dev || !req->cu_seqlens_host || !req->q_off_dev || !req->q_off_host ||
      !req->frag_off_dev || !req->frag_off_host)
    return fail(h, OP_ERR_INVALID, "op_assemble_rows: a plan, cu_seqlens or offset buffer is NULL");
  if (req->q_off_host[0] != 0 || req->frag_off_host[0] != 0)
    return fail(h, OP_ERR_INVALID, "op_assemble_rows: offsets do not start at 0");
  for (int q = 0; q < req->n_queries; ++q)
    if (req->q_off_host[q + 1] < req->q_off_host[q]) return fail(h, OP_ERR_INVALID, "op_assemble_rows: q_off decreases at query %d", q);
  const int n_query_tokens = req->q_off_host[req->n_queries], n_corpus = req->frag_off_host[req->n_frag];
  if (n_corpus < 0) return fail(h, OP_ERR_INVALID, "op_assemble_rows: frag_off ends at %d", n_corpus);
  if (req->cu_seqlens_host[0] != 0) return fail(h, OP_ERR_INVALID, "op_assemble_rows: cu_seqlens_host[0] is %d", req->cu_seqlens_host[0]);
  bool any_query = false, any_ctx = false;
  int64_t at = 0;
  for (int r = 0; r < req->n_rows; ++r) {
    const int32_t* pr = req->plan_host + (size_t)r * 4;
    const int query = pr[0], first = pr[1], n = pr[2], clip = pr[3];
    if (query < 0 || query >= req->n_queries) return fail(h, OP_ERR_INVALID, "op_assemble_rows: row %d names query %d of %d", r, query, req->n_queries);
    if (first < 0 || n < 0 || first > req->n_frag - n)
      return fail(h, OP_ERR_INVALID, "op_assemble_rows: row %d takes fragments %d .. %d + %d of %d", r, first, first, n, req->n_frag);
    int64_t ctx = 0;
    if (n > 0) {
      const int32_t* fo = req->frag_off_host + first;
      if (fo[0] < 0 || fo[1] < fo[0] || fo[n] < fo[1] || fo[n] > n_corpus)
        return fail(h, OP_ERR_INVALID, "op_assemble_rows: frag_off decreases or leaves the corpus at row %d", r);
      if (clip < 0 || clip > fo[1] - fo[0])
        return fail(h, OP_ERR_INVALID, "op_assemble_rows: row %d clips its first fragment of %d ids to %d", r, fo[1] - fo[0], clip);
      ctx = clip > 0 ? (int64_t)clip + (fo[n] - fo[1]) : (int64_t)(fo[n] - fo[0]);
    } else if (clip != 0 && clip != -1) {
      return fail(h, OP_ERR_INVALID, "op_assemble_rows: row %d has clip %d and no fragment", r, clip);
    }
    const int row_suffix = (n == 0 && clip == -1) ? 0 : n_pieces[2];
    const int q_len = req->q_off_host[query + 1] - req->q_off_host[query];
    any_query |= q_len > 0;
    any_ctx |= ctx > 0;
    at += (int64_t)n_pieces[0] + q_len + n_pieces[1] + ctx + row_suffix;
    if (at > (int64_t)INT32_MAX || (int64_t)req->cu_seqlens_host[r + 1] != at)
      return fail(h, OP_ERR_INVALID, "op_assemble_rows: cu_seqlens_host[%d] is %d, the plan's rows end at %lld", r + 1,
                  req->cu_seqlens_host[r + 1], (long long)at);
  }
  if (at != (int64_t)req->total_tokens)
    return fail(h, OP_ERR_INVALID, "op_assemble_rows: the plan's rows hold %lld ids, total_tokens is %d", (long long)at, req->total_tokens);
  if (at > 0 && !ids_dev) return fail(h, OP_ERR_INVALID, "op_assemble_rows: ids_dev is NULL");
  if (any_query && !req->query_ids_dev) return fail(h, OP_ERR_INVALID, "op_assemble_rows: query_ids_dev is NULL");
  if (any_ctx && !req->corpus_dev) return fail(h, OP_ERR_INVALID, "op_assemble_rows: corpus_dev is NULL");
  if (!h) return fail(nullptr, OP_ERR_INVALID, "op_assemble_rows: NULL handle");
  if (at == 0) return OP_OK;
  OP_HIP(h, hipSetDevice(h->cfg.device_id));
  opl::launch_assemble_rows(reinterpret_cast<hipStream_t>(hip_stream), req->corpus_dev, req->frag_off_dev, req->n_frag, n_corpus,
                            req->query_ids_dev, req->q_off_dev, req->n_queries, n_query_tokens, pieces, n_pieces, req->plan_dev,
                            req->cu_seqlens_dev, req->n_rows, req->total_tokens, ids_dev);
  OP_HIP(h, hipGetLastError());
  return OP_OK;
}

int op_planned_fragment_means(op_handle* h, const op_assemble_request* rows, const op_planned_means_request* req, void* hip_stream) {
  // (the requests first, on the host copies -- opp::check_planned_means: nothing is enqueued before the last check)
  const opp::Refusal refused = opp::check_planned_means(rows, req);
  if (refused.code != OP_OK) return fail(h, refused);
  if (!h) return fail(nullptr, OP_ERR_INVALID, "op_planned_fragment_means: NULL handle");
  if (rows->n_rows == 0 || req->slot_off_host[rows->n_rows] == req->slot_off_host[0]) return OP_OK;  // (no fragment in any row)
  OP_HIP(h, hipSetDevice(h->cfg.device_id));
  opl::launch_planned_fragment_means(reinterpret_cast<hipStream_t>(hip_stream), *rows, *req);
  OP_HIP(h, hipGetLastError());
  return OP_OK;
}

int op_located_fragment_means(op_handle* h, const op_assemble_request* rows, const op_planned_means_request* req, const int32_t* ids_dev,
                              int32_t* ctx_start_out_dev, void* hip_stream) {
  const opp::Refusal refused = opp::check_located_means(rows, req, ids_dev, ctx_start_out_dev);
  if (refused.code != OP_OK) return fail(h, refused);
  if (!h) return fail(nullptr, OP_ERR_INVALID, "op_located_fragment_means: NULL handle");
  if (rows->n_rows == 0) return OP_OK;  // (a row without fragments still gets its ctx_start)
  OP_HIP(h, hipSetDevice(h->cfg.device_id));
  opl::launch_located_fragment_means(reinterpret_cast<hipStream_t>(hip_stream), *rows, *req, ids_dev, ctx_start_out_dev);
  OP_HIP(h, hipGetLastError());
  return OP_OK;
}

int op_sentence_decisions(op_handle* h, const op_decisions_request* req, void* hip_stream) {
  const opp::Refusal refused = opp::check_decisions(req);
  if (refused.code != OP_OK) return fail(h, refused);
  if (!h) return fail(nullptr, OP_ERR_INVALID, "op_sentence_decisions: NULL handle");
  if (req->n_instances == 0) return OP_OK;  // (n_out is 0 too: the instances tile the outputs)
  OP_HIP(h, hipSetDevice(h->cfg.device_id));
  opl::launch_sentence_decisions(reinterpret_cast<hipStream_t>(hip_stream), *req);
  OP_HIP(h, hipGetLastError());
  return OP_OK;
}

}  // extern "C"
