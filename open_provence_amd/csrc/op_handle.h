// op_handle.h -- what the units of the C ABI share (op_api / op_weights / op_select / op_forward / op_forward_layers /
// op_forward_masked / op_attention_side / op_services .hip): the handle, the error and launch helpers, a packed batch as an entry point receives
// it, and the declarations of the functions one unit defines and another calls.  Host side only.
#pragma once

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

#include "op_internal.h"
#include "op_plan.h"
#include "op_sets.h"
#include "opk_loss.hip.h"

using namespace opk;
using opl::Policy;
using namespace ops;
using opp::AttnPlan;
using opp::align_up;
using opp::align_up_sz;

static_assert(opp::ROW_ALIGN == opk::ROW_ALIGN, "op_plan.h chunks a batch by the kernels' row alignment");

namespace oph {

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

struct LayerWeights {
  float* attn_norm = nullptr;  // absent on layer 0
  float* mlp_norm = nullptr;
  u16* pack[W_COUNT][PF_COUNT] = {};  // the GEMM weights in every format the handle builds (op_sets.h), nullptr: no such pack
};

struct ProfileEvent {
  int kind;
  hipEvent_t start, stop;
};

}  // namespace oph

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
  std::vector<oph::LayerWeights> layers;
  std::vector<void*> allocations;
  std::vector<std::string> missing;  // weight names not loaded yet
  float* capture = nullptr;
  bool profiling = false;
  std::vector<oph::ProfileEvent> events;
  double prof_ms[oph::PK_COUNT] = {0};
  int prof_launches[oph::PK_COUNT] = {0};
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

namespace oph {

// op_api.hip: the error text into the handle (if any) and the thread's last error; returns `code`
int fail(op_handle* h, int code, const char* fmt, ...);
int fail(op_handle* h, const opp::Refusal& r);

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

// op_forward_masked's addition to a forward: the batch is dense (a sequence = a padded row of `width` positions), runs on kernel
// set "fp32" whatever set the handle has selected, and the mask removes keys (opk_f32_masked.hip.h).
// native (op_forward_masked_native; row and panel path): the pass stays on the handle's selected kernel set -- attn_fp_kernel's
// key-mask form over key_row, the row means of v^T, the ranking head's masked mean pooling (opk_masked.hip.h).
struct MaskedReq {
  const uint8_t* key_ok = nullptr;  // [total_tokens]
  float* vmean = nullptr;           // [n_seqs][H]: the row means of v of the sliding-window layer in flight
  const int32_t* cu_host = nullptr; // [n_seqs + 1]: the dense cu_seqlens on the host (a chunk's tokens, for the pruning logits' zeros)
  bool native = false;
  uint8_t* key_row = nullptr;       // native: [padded row capacity] the mask in the row layout of the chunk in flight
};

// ---- defined once, in the unit named; called from others -------------------------------------------------------------------
// op_api.hip
int drain_profile(op_handle* h);
void build_rope_host(float theta, int max_pos, std::vector<float>& cs, std::vector<float>& sn);
// op_select.hip: the weights' flags from the device, the selection (opp::select), the result into the handle
int resolve_policy(op_handle* h);
// ... run kernel set `set` with layer mask `mlp_layers` from now on where the handle can (-1: the default selection)
int pin(op_handle* h, int set, uint64_t mlp_layers = ~0ull);
// op_forward.hip
// the rows a workspace of this geometry is carved for (op_workspace_bytes, op_forward_packed and the attention side passes)
int chunk_row_capacity(const op_handle* h, int n_seqs, int total_tokens, int max_seqlen);
// the regions of a forward's workspace for a batch of this geometry; f32: with the planes of kernel set "fp32"
opp::Layout forward_layout(const op_handle* h, int n_seqs, int total_tokens, int max_seqlen, bool f32);
int host_cu_seqlens(op_handle* h, const PackedBatch& b, std::vector<int32_t>& cu_copy, const int32_t** cu_out);
// op_forward_packed, and op_forward_packed_hidden / _pooled with their validated request (hid; nullptr: none); msk: the dense
// forward of op_forward_masked over its own workspace
int forward_packed_impl(op_handle* h, const PackedBatch& b, const HiddenReq* hid, const MaskedReq* msk = nullptr);
// the row map of the chunk [s0, s0 + ns) as the attention side passes take it: the forward's seq_offsets_kernel (aligned row
// offsets into roff) and row_map_kernel, which only the forward unit holds
void launch_side_row_map(hipStream_t stream, const int32_t* cu_dev, int s0, int ns, int r_pad, int32_t* roff, int32_t* row_seq,
                         int32_t* row_pos, int32_t* row_tok);

}  // namespace oph

using namespace oph;
