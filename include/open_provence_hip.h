/*
 * open_provence_hip.h -- C ABI of libopenprovence_hip.so (MI355X / gfx950).
 *
 * Drop-in boundary for ONE path of hotchpotch/open_provence: the batched (query, context) cross-encoder
 * forward.  Each entry point names the reference interface it replaces (paths relative to the
 * reference tree; "standalone.py" = open_provence/modeling_open_provence_standalone.py; "HF" = the
 * third-party transformers ModernBERT the reference instantiates at standalone.py:1341).
 *
 * Conventions
 *   - plain pointers and sizes only; no C++/torch types cross this boundary;
 *   - every function returns OP_OK (0) or a negative OP_ERR_* code and never throws;
 *     the message is available from op_last_error(handle) (or op_last_error(NULL) when no
 *     handle exists yet);
 *   - one handle per device; calls on one handle must be serialised by the caller (host side); the
 *     forward is asynchronous with respect to the given HIP stream, and forwards enqueued on DIFFERENT
 *     streams with DIFFERENT workspaces may run side by side on the device (the weights are read-only;
 *     profiling and hidden-state capture off) -- HipEncoder.forward_packed_on does that on two streams
 *     bound to disjoint halves of the CUs;
 *   - the caller owns every I/O buffer and the workspace; the library owns only its re-packed weights.
 */
#ifndef OPEN_PROVENCE_HIP_H
#define OPEN_PROVENCE_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define OP_ABI_VERSION 10 /* 10: op_hidden_request, op_forward_packed_hidden (per-call hidden states on the kernels of op_forward_packed); 9: kernel sets 8 / 9 layer by layer (op_calibration.mlp_layers / mlp_layers_err, OP_CAL_WHOLE_DEPTH, op_mlp_correction_layers, op_select_mlp_correction_layers); 8: op_calibration.flags (OP_CAL_FULL_REPORT; the search stops at the first candidate that holds otherwise), op_calibrate validates its batch before it touches the handle, op_load_weight of a GEMM weight drops a pinned / calibrated kernel set; 7: kernel sets 10 / 11 (fp16 attention inside the fp16 + e4m3 sets), op_calibration holds 16 candidates; 6: op_select_kernel_set, op_calibrate, kernel set 7 ("f16": single-pass fp16 operands); 5: op_set_compact_operands (run-time fallback to the (hi, lo) bf16 kernel sets); 4: kernel set 3 (fp16 + e4m3 operands), flag NO_F8; 3: op_segment_means, flags LAYER_M32 / NO_HEAD_FUSION (struct layouts as in 2) */
#define OP_MAX_LAYERS 128

typedef struct op_handle op_handle;

enum op_status {
  OP_OK = 0,
  OP_ERR_INVALID = -1,     /* bad argument                                   */
  OP_ERR_UNSUPPORTED = -2, /* configuration the kernels do not implement     */
  OP_ERR_HIP = -3,         /* HIP runtime failure (message has the HIP text) */
  OP_ERR_STATE = -4,       /* call order (e.g. forward before all weights)   */
  OP_ERR_WORKSPACE = -5,   /* workspace too small / misaligned               */
  OP_ERR_NOMEM = -6
};

enum op_dtype { OP_DTYPE_F32 = 0, OP_DTYPE_BF16 = 1, OP_DTYPE_F16 = 2 };

/* Arithmetic of the MFMA contractions (accumulation is always fp32; LayerNorm, softmax, GELU,
 * RoPE and the residual stream are always fp32).  Every operand can be carried as a (hi, lo) bf16
 * pair (hi = RNE(v), lo = RNE(v - hi), ~16 mantissa bits together); a contraction left x right then
 * evaluates hi*hi plus the optional terms of its mask:
 *   OP_TERM_LEFT_LO   lo(left) * hi(right)        OP_TERM_RIGHT_LO   hi(left) * lo(right)
 * "left" is the activation-side operand.  One mask per contraction family (enum op_gemm_family):
 *   OP_PRECISION_BF16X3  all masks 3: the mode that meets the 1e-3 parity bar against the fp32 CPU
 *                        reference for any checkpoint;
 *   OP_PRECISION_BF16X2  weights rounded to bf16 (no hi*lo(weight) term in the four weight GEMMs),
 *                        activations (hi, lo), attention all terms;
 *   OP_PRECISION_BF16    all masks 0: single-pass bf16 operands (what the reference itself computes
 *                        with on a GPU: standalone.py:219-233 picks bf16), ~1e-2 on logits;
 *   OP_PRECISION_CUSTOM  op_config.terms[] as given.
 * Independently of the mode, the hi*lo(weight) term of a family is dropped -- without changing a bit
 * of the result -- when every lo element of every weight of that family is zero, i.e. for bf16
 * checkpoints (detected in op_load_weight, applied in op_weights_ready; see op_effective_policy). */
enum op_precision { OP_PRECISION_BF16X3 = 0, OP_PRECISION_BF16 = 1, OP_PRECISION_BF16X2 = 2, OP_PRECISION_CUSTOM = 3 };
enum op_term { OP_TERM_LEFT_LO = 1, OP_TERM_RIGHT_LO = 2 };
enum op_gemm_family {
  OP_FAM_WQKV = 0,     /* LN(x) x Wqkv        HF :272      */
  OP_FAM_QK = 1,       /* q x k               HF :166-185  */
  OP_FAM_PV = 2,       /* softmax(..) x v                  */
  OP_FAM_ATTN_OUT = 3, /* attention out x Wo  HF :299      */
  OP_FAM_WI = 4,       /* LN(x) x Wi          HF :90       */
  OP_FAM_MLP_OUT = 5,  /* GeGLU out x Wo      HF :91       */
  OP_FAM_COUNT = 6
};

/* op_config.flags */
enum op_flags {
  OP_FLAG_FORCE_TILED = 1,      /* generic 128x128x32 tiled kernels for every shape (test hook)             */
  OP_FLAG_NO_SMALL_BLOCKS = 2,  /* never use the 64-row GEMM blocks of the latency regime (measurement hook) */
  OP_FLAG_ATT_WAVES_4 = 4,      /* 128-query attention blocks for full-attention layers (measurement hook)   */
  OP_FLAG_ATT_WAVES_8 = 8,      /* 256-query attention blocks for full-attention layers (measurement hook)   */
  OP_FLAG_NO_POLICY_KERNELS = 16, /* always run the all-terms kernels with cleared lo operands (test hook)   */
  OP_FLAG_NO_LAYER_FUSION = 32,   /* two fused kernels per layer instead of the whole-layer kernel (A/B hook) */
  OP_FLAG_LAYER_8X16 = 64,        /* whole-layer kernel as 8 waves x 16 rows (two waves per SIMD) (A/B hook)   */
  OP_FLAG_NO_HEAD_FUSION = 256,   /* embedding + LayerNorm and final_norm + pruning head as their own launches on the row path too (A/B hook) */
  OP_FLAG_LAYER_M32 = 128,        /* whole-layer kernel on 32x32x16 MFMAs (hidden = 256): fewer cycles, more power per flop -- slower under the power limit (A/B hook) */
  OP_FLAG_ATTN_XCD_GROUP = 1024,  /* row path too: the XCD-grouped attention block map (the query blocks of a sequence-head follow each other on one XCD; default on the panel path only) (A/B hook) */
  OP_FLAG_PANEL_F8 = 2048,        /* hidden 512 / 768 (panel GEMMs): select the fp16 + e4m3 kernel sets there too.  OFF by default: through 19-25 layers their error against the fp32 reference reaches 0.45-1.0e-3 on logits (the (hi, lo) bf16 sets: 0.2-0.5e-3), too close to the 1e-3 bar of the path for +2.5 % (bf16 checkpoint) / +14 % (fp32) pairs/s.  On this opt-in path the MLP activation h is an fp16 operand converted with saturation: a value beyond 65504 is CLAMPED, not reported (the row path's sets turn it into NaN and fall back; the default panel sets keep h as (hi, lo) bf16 pairs with fp32's range) */
  OP_FLAG_PANEL_F8_WI = 4096,     /* hidden 512 / 768: the fp16 + e4m3 format in the Wi GEMM alone (52 % of the GEMM FLOPs; LayerNorm(mlp_norm) written in that format, h still as (hi, lo) bf16 pieces for the MLP output projection): the cheapest place for the format's error.  DEFAULT for fp32-valued weights (+5.6 % pairs/s on base, <= 5.4e-4 at 19-25 layers); this flag requests it for bf16-valued weights too (+0.7 %).  OP_FLAG_NO_F8 switches it off */
  OP_FLAG_NO_LAYER_PAIRS = 8192,  /* hidden = 256, single-pass kernel sets ("f16" / "bf16"): keep the 8 waves x 16 rows whole-layer kernel instead of the wave-pair kernel (opk_layer16p.hip.h) (A/B and test hook) */
  OP_FLAG_F32_PACKS = 16384,      /* op_load_weight also keeps a row-major fp32 copy of the four GEMM weights of every layer (4 bytes per weight element more on the device): what kernel set 12 ("fp32", OP_KS_F32) runs on.  Without it no handle's device footprint or allocation order changes, and OP_KS_F32 is refused */
  OP_FLAG_NO_F8 = 512             /* never select kernel set 3 (fp16 hi + e4m3 lo operands in the whole-layer kernel): keep the (hi, lo) bf16 kernel sets (A/B and bit-identity test hook) */
};

enum op_pooling { OP_POOL_CLS = 0, OP_POOL_MEAN = 1 };

/* Mirrors the fields of HF ModernBertConfig that change the arithmetic
 * (transformers/models/modernbert/configuration_modernbert.py:77-162) plus
 * OpenProvenceConfig.num_labels (standalone.py:1279). */
typedef struct op_config {
  uint32_t struct_bytes; /* = sizeof(op_config), checked */
  int32_t device_id;
  int32_t vocab_size;
  int32_t hidden_size;
  int32_t intermediate_size;
  int32_t num_layers;
  int32_t num_heads; /* head_dim = hidden_size / num_heads must be 64 */
  int32_t num_labels;
  int32_t local_attention; /* full window; keys with |q-k| <= local_attention/2 are visible */
  int32_t max_position_embeddings;
  int32_t pooling;   /* enum op_pooling */
  int32_t precision; /* enum op_precision */
  float norm_eps;
  float global_rope_theta;
  float local_rope_theta;
  int32_t chunk_rows; /* rows of the packed batch processed per pass (0 = library default) */
  uint8_t layer_is_global[OP_MAX_LAYERS]; /* 1 = full attention, 0 = sliding window */
  uint8_t terms[8];   /* OP_PRECISION_CUSTOM: term mask per op_gemm_family (entries >= OP_FAM_COUNT unused) */
  uint32_t flags;     /* enum op_flags */
  /* Which hidden state feeds the pruning head (standalone.py:1695 takes outputs.hidden_states[-1]):
   * 0 = the final_norm output (transformers >= 5 ties hidden_states[-1] to last_hidden_state,
   * utils/output_capturing.py:269-277 -- what the reference computes in this image), 1 = the last
   * layer's output BEFORE final_norm (what transformers 4.x ModernBertModel.forward appended, i.e.
   * what the reference computes under its own uv.lock pin 4.57.1).  The rank head always sees the
   * normalised state. */
  int32_t prune_pre_final_norm;
} op_config;

int op_abi_version(void);

/* Replaces: OpenProvencePreTrainedModel.__init__ building the backbone from
 * config.base_model_config (standalone.py:1340-1342, 1354-1375). */
int op_create(const op_config* cfg, op_handle** out);

/* Replaces: PreTrainedModel.load_state_dict on the reference's checkpoint keys
 * (standalone.py:1448-1464; key list in SURVEY.md section 8b).  `name` is the checkpoint key with or
 * without the "ranking_model." prefix (legacy checkpoints omit it).  `data` may be a host or a
 * device pointer; the tensor is copied and re-packed (bf16 hi/lo planes, GeGLU row interleave),
 * the caller keeps ownership of the source. */
int op_load_weight(op_handle* h, const char* name, const void* data, int dtype, const int64_t* shape, int ndim);

/* OP_OK when every tensor of the model has been loaded; otherwise OP_ERR_STATE and
 * op_last_error() lists the missing keys. */
int op_weights_ready(op_handle* h);

/* Bytes of caller-provided device workspace needed by op_forward_packed for a batch of `n_seqs`
 * sequences, `total_tokens` tokens, longest sequence `max_seqlen`. */
size_t op_workspace_bytes(const op_handle* h, int n_seqs, int total_tokens, int max_seqlen);

/* After op_weights_ready: the term masks actually evaluated (requested policy minus the weight-lo
 * terms that are identically zero for this checkpoint), terms_out[OP_FAM_COUNT], and *kernel_set =
 * index of the curated kernel set that implements them with exactly those MFMA passes (0 = all
 * terms, 1 = bf16 weights, 2 = single pass, 3 = the terms of 1 with the whole-layer kernel's
 * operands carried as fp16 hi + e4m3 lo -- 1.5 instead of 2 MFMA units per product, 4 = the terms
 * of 0 in that format with the weights' lo part as a second e4m3 plane -- 2 units instead of 3 and
 * one kernel per layer instead of two), or -1 when the policy runs on the all-terms kernels with
 * cleared lo operands (same numerics, no speed-up); 5 / 6 = sets 0 / 1 on the panel path with the Wi GEMM alone in the
 * format of sets 4 / 3 (OP_FLAG_PANEL_F8_WI); 7 = "f16", single-pass fp16 operands (only ever chosen by op_calibrate /
 * op_select_kernel_set: then terms_out holds that set's masks, not the checkpoint's).  Sets 3 / 4 replace 1 / 0 for hidden <= 256
 * (hidden 512 / 768: with OP_FLAG_PANEL_F8) unless OP_FLAG_NO_F8 is set, set 3 needs every GEMM
 * weight to be exactly an fp16 value, and neither is taken for a checkpoint with a weight TENSOR
 * scaled into fp16's subnormal range (checked at load time).  Their fp16 operand plane has fp16's
 * range: an MLP activation beyond it turns the outputs into NaN (on purpose: not clamped; on the panel path through a
 * range flag the kernels raise in the workspace and the head kernels turn into NaN logits -- under MODE.FP16_OVFL = 1 a
 * conversion clamps and the fp16 MFMA takes a NaN operand for a finite number). */
int op_effective_policy(op_handle* h, uint8_t* terms_out, int* kernel_set);

/* Kernel sets (the numbering of op_effective_policy).  MFMA pipe time per algorithmic product in 16-bit units:
 * BF16X3 3, BF16X3_WI_F8 ~2.5 (panel path), F16_F8_W 2, BF16_WEIGHTS 2, BF16_WEIGHTS_WI_F8 ~1.75, F16_F8 1.5, BF16 1,
 * F16 1.  F16 (round 5) = the kernels and layouts of BF16 with every operand carried as fp16 (11 significant bits
 * instead of 8; fp16's range: an activation beyond 65504 turns the outputs into NaN, as on sets 3 / 4). */
enum op_kernel_set {
  OP_KS_AUTO = -1, /* op_select_kernel_set: back to the default selection of op_weights_ready */
  OP_KS_BF16X3 = 0,
  OP_KS_BF16_WEIGHTS = 1,
  OP_KS_BF16 = 2,
  OP_KS_F16_F8 = 3,
  OP_KS_F16_F8_W = 4,
  OP_KS_BF16X3_WI_F8 = 5,
  OP_KS_BF16_WEIGHTS_WI_F8 = 6,
  OP_KS_F16 = 7,
  /* panel path (hidden 512 / 768) only: the attention side of a layer (q / k / v projection, attention, output projection)
   * on set 7, its MLP (LayerNorm(mlp_norm), Wi GEMM + GeGLU, MLP output projection) in the fp16 + e4m3 format of set 4
   * (F16_MLP_F8_W: the weights' lo part too) or of set 3 (F16_MLP_F8).  On weights of a trained checkpoint's scale the
   * MLP's two contractions carry ~6 x the error of the other four families together (scripts/family_error_probe.py), and
   * they are 75 % of the linear FLOPs: ~1.75 / ~1.4 MFMA units per product. */
  OP_KS_F16_MLP_F8_W = 8,
  OP_KS_F16_MLP_F8 = 9,
  /* panel path only: sets 4 / 3 with the ATTENTION itself (q x k, p x v) single pass on fp16 operands -- the q / k / v
   * projection writes single-plane fp16 q, k, v^T, attention runs set 7's kernels and writes o as fp16 + e4m3 pieces; the
   * four weight GEMMs keep every term of sets 4 / 3.  Attention is 18 - 21 % of large 64 x 2048 / en-gte varlen on sets
   * 4 / 3 (three MFMA passes per product), and q x k / p x v are the two families whose single-pass error is smallest
   * (scripts/family_error_probe.py). */
  OP_KS_F16_F8_W_ATTN_F16 = 10,
  OP_KS_F16_F8_ATTN_F16 = 11,
  /* "fp32": every contraction of a layer on the fp32-input MFMA (v_mfma_f32_16x16x4_f32: fp32 operands, fp32 accumulate, a
   * k-ordered fmaf chain; 1/16 of the 16-bit rate), fp32 activation planes, the checkpoint's fp32 weights as loaded, exact erff
   * and expf -- the reference's fp32 arithmetic up to the order of its sums.  Any handle shape (row, panel or tiled) created
   * with OP_FLAG_F32_PACKS.  Never a default and never cheaper than another set: pinned by op_select_kernel_set, or the
   * reference / escalation target of op_calibrate under OP_CAL_REFERENCE_F32.  No fp16 plane: no range guard applies. */
  OP_KS_F32 = 12,
  OP_KS_COUNT = 13
};

/* Pin the kernel set the forward runs on (OP_KS_AUTO: un-pin).  A set with fewer product terms than the loaded
 * checkpoint carries (e.g. OP_KS_F16 on any checkpoint, OP_KS_F16_F8 on fp32-valued weights) is an APPROXIMATION of the
 * requested policy: op_calibrate is the call that measures it first.  OP_ERR_UNSUPPORTED when the handle cannot run the
 * set (shape without those kernels, packs not built because of OP_FLAG_NO_F8, a weight tensor below fp16's reach; OP_KS_F32
 * on a handle created without OP_FLAG_F32_PACKS: the message names the flag).
 * Replaces: the reference choosing its arithmetic from the device and what loads (standalone.py:219-244, 1589-1615). */
int op_select_kernel_set(op_handle* h, int kernel_set);

/* Choose the arithmetic from the checkpoint that is loaded.  The default selection of op_weights_ready is safe for ANY
 * weights (it only drops terms that are identically zero) -- and therefore priced for the worst case: weights of O(1)
 * scale, where every dropped term costs >= 7e-3 on a logit.  A trained checkpoint's weights are ~0.02: there most of
 * the correction terms are below the parity bar by orders of magnitude.  op_calibrate runs one batch (ids_host /
 * cu_seqlens_host / n_seqs: the caller's sample of real inputs; NULL / NULL / 0: 24 rows x min(512, max positions) + 14
 * ragged rows of uniform token ids) through the (hi, lo) bf16 realisation of the requested policy (`reference_set`) and
 * through every available kernel set CHEAPER than the default one, cheapest first, and keeps the first whose
 * max |logit difference| (pruning and ranking logits) to the reference outputs is <= tolerance and finite; if none is,
 * the default selection stays (unless its own outputs on that batch are not finite: then the reference set runs).  The north_star bar against the fp32 CPU reference is 1e-3; 1e-4 is the tolerance the
 * Python layer uses.  Synchronous (load-time call; its temporary device buffers are freed before it returns).
 * Replaces: standalone.py:219-244 / 1589-1615 / 1631-1642 (dtype and attention implementation chosen per device and
 * checkpoint, with a retry) -- the reference decides its arithmetic at load time too. */
typedef struct op_calibration {
  uint32_t struct_bytes; /* = sizeof(op_calibration), checked when a report is requested */
  float tolerance;
  int32_t reference_set; /* the (hi, lo) bf16 kernel set the candidates were compared with (OP_CAL_REFERENCE_F32: 12) */
  int32_t default_set;   /* what op_weights_ready selects for this checkpoint */
  int32_t chosen_set;    /* what the forward runs on from now on */
  int32_t n_candidates;
  int32_t candidate_set[16];
  float candidate_err[16]; /* max |difference| to the reference outputs; +inf: non-finite outputs */
  int32_t n_rows, n_tokens; /* the calibration batch */
  float default_err;        /* the default set's own difference to the reference outputs on that batch.  It is not held to
                             * the tolerance (it is the set the parity tests stand on), but when it is NOT FINITE -- an
                             * activation beyond fp16's range on sets 3 - 6 -- or beyond 10 x tolerance, and no candidate
                             * passes, the reference set is chosen right away (ABI 8: the bound on a finite default_err) */
  uint32_t flags;           /* IN: OP_CAL_* bits */
  float mlp_layers_err;     /* chosen_set 8 / 9 with layers dropped: the difference of what runs now (0 when no layer was dropped) */
  uint64_t mlp_layers;      /* chosen_set 8 / 9 (the "f16" set with the MLP in the fp16 + e4m3 format): bit li = layer li keeps that
                             * MLP; in the other layers the batch stayed within the tolerance on the "f16" set's MLP (ABI 9).
                             * 0 for every other chosen_set */
} op_calibration;
#define OP_CAL_FULL_REPORT 1u /* measure every candidate (the report lists them all); default: cheapest first, stop at the first that holds */
#define OP_CAL_WHOLE_DEPTH 2u /* sets 8 / 9 for the whole depth or not at all (no per-layer search) */
/* Opt-in, on a handle created with OP_FLAG_F32_PACKS (ignored without the packs): the candidates and the default set are
 * compared with kernel set 12 ("fp32") instead of the (hi, lo) bf16 set -- reference_set = 12 --, the (hi, lo) bf16 set is
 * a candidate like any other (where it is cheaper than the default), and a default beyond 10 x tolerance escalates to
 * set 12.  Without the bit nothing about the call or its report changes. */
#define OP_CAL_REFERENCE_F32 4u
int op_calibrate(op_handle* h, float tolerance, const int32_t* ids_host, const int32_t* cu_seqlens_host, int n_seqs,
                 op_calibration* report);

/* Kernel sets 8 / 9 layer by layer: bit li of *layer_mask = layer li runs its MLP in the fp16 + e4m3 format (0 when another
 * set runs).  op_select_mlp_correction_layers pins a mask on a handle whose set 8 / 9 was pinned by op_select_kernel_set or
 * chosen by op_calibrate (OP_ERR_STATE otherwise; at most 64 layers) -- what a process group uses to give every rank the
 * mask one rank measured.  Replaces: nothing (see op_calibrate). */
int op_mlp_correction_layers(op_handle* h, uint64_t* layer_mask);
int op_select_mlp_correction_layers(op_handle* h, uint64_t layer_mask);

/* Run-time switch between the fp16 + e4m3 kernel sets (3 / 4) and the (hi, lo) bf16 sets (1 / 0) they replace: both
 * weight packs of a handle stay resident, so this only re-runs the selection of op_weights_ready (with enabled = 0 as if
 * OP_FLAG_NO_F8 were set).  The Python layer calls it when a forward on sets 3 / 4 returns non-finite outputs -- an MLP
 * activation beyond fp16's range -- and repeats that forward, so that process() returns what the reference returns
 * instead of raising.  Replaces: nothing; precedent for a silent, correct retry: the reference's own fallback from an
 * unsupported dtype / attention implementation at load time (standalone.py:1631-1642).  Returns OP_OK; *changed (may
 * be NULL) = 1 when the evaluated kernel set is different afterwards (sets 5 / 6 and a pinned / calibrated set count:
 * enabled = 0 also drops a set chosen by op_select_kernel_set / op_calibrate).  The workspace size may change: query
 * op_workspace_bytes again. */
int op_set_compact_operands(op_handle* h, int enabled, int* changed);

/* Replaces: OpenProvenceModel.forward (standalone.py:1666-1739) = HF
 * ModernBertForSequenceClassification.forward + OpenProvenceHead.forward (standalone.py:434-448),
 * on the UNPADDED batch: ids_dev[total_tokens] are the attention_mask==1 tokens of all rows laid
 * end to end, cu_seqlens[n_seqs+1] their prefix offsets.  cu_seqlens_host may be NULL (the library
 * then reads cu_seqlens_dev back, which synchronises the stream once).
 *   prune_logits_dev [total_tokens, 2]  fp32   (pruning_logits at attention_mask==1 positions)
 *   rank_logits_dev  [n_seqs, num_labels] fp32 (ranking_logits)
 *   keep_prob_dev    [total_tokens] fp32 or NULL: softmax(pruning_logits, -1)[:, 1] evaluated as
 *                    sigmoid(l1 - l0) in the same kernel (replaces standalone.py:2918-2924)
 * Work is enqueued on hip_stream (a hipStream_t, NULL = default stream).
 * The workspace may hold anything on entry: the outputs depend on ids, cu_seqlens and the weights only, and nothing outside
 * [workspace_dev, workspace_dev + op_workspace_bytes) and the output buffers is written. */
int op_forward_packed(op_handle* h, const int32_t* ids_dev, const int32_t* cu_seqlens_dev,
                      const int32_t* cu_seqlens_host, int n_seqs, int total_tokens, int max_seqlen,
                      float* prune_logits_dev, float* rank_logits_dev, float* keep_prob_dev,
                      void* workspace_dev, size_t workspace_bytes, void* hip_stream);

/* Replaces: output_hidden_states=True of the reference forward (standalone.py:1689, 1727), per call.  One forward
 * exactly as op_forward_packed enqueues it -- the same kernels, bit-identical logits -- that also writes the hidden states
 * `req` selects.  Entry 0 is the embedding LayerNorm output, entry i (1 <= i < num_layers) the output of layer i-1, entry
 * num_layers the final_norm output (op_config.prune_pre_final_norm = 0) or the un-normalised output of the last layer (= 1):
 * hidden_states[-1] of the reference under each transformers line, the pruning head's input either way.
 *   select   host array of num_layers + 1 flags (entry i = hidden_states[i]), or NULL = every entry
 *   out_dev  the selected entries in order, each
 *              pad_width == 0: packed [total_tokens][hidden]
 *              pad_width  > 0: padded [n_seqs][pad_width][hidden], token t of sequence s at [s][t - cu[s]]; positions at or
 *                              beyond a sequence's length are NOT written (the caller zeroes them); pad_width >= max_seqlen
 *   dtype    OP_HIDDEN_F32, or OP_HIDDEN_BF16 = the fp32 state rounded to nearest even
 * The request lives for this call only (no handle state): the call is as stream-safe as op_forward_packed.  A wrong
 * struct_bytes, an unknown dtype, a pad_width below max_seqlen, or out_dev == NULL with an entry selected (of a non-empty
 * batch) return
 * OP_ERR_INVALID before anything is enqueued.  req == NULL is op_forward_packed. */
enum op_hidden_dtype { OP_HIDDEN_F32 = 0, OP_HIDDEN_BF16 = 1 };
typedef struct op_hidden_request {
  uint32_t struct_bytes; /* sizeof(op_hidden_request) */
  int32_t dtype;         /* enum op_hidden_dtype */
  int32_t pad_width;     /* 0: packed [n_sel][total_tokens][H]; > 0: padded [n_sel][n_seqs][pad_width][H] */
  const uint8_t* select; /* host array of num_layers + 1 flags, or NULL = all; entry i = hidden_states[i] */
  void* out_dev;         /* written in the order of the selected entries */
} op_hidden_request;
int op_forward_packed_hidden(op_handle* h, const int32_t* ids_dev, const int32_t* cu_seqlens_dev,
                             const int32_t* cu_seqlens_host, int n_seqs, int total_tokens, int max_seqlen,
                             float* prune_logits_dev, float* rank_logits_dev, float* keep_prob_dev,
                             void* workspace_dev, size_t workspace_bytes, void* hip_stream, const op_hidden_request* req);

/* Replaces: what callers of output_hidden_states=True usually compute from it -- one vector per sequence and entry (a CLS
 * probe, a layer-wise probe, a pooled embedding) -- reduced on the device, so that the (N + 1) x tokens x H states are never
 * held.  Additive to ABI 10 (op_abi_version() is unchanged: detect the call by symbol).  One forward exactly as
 * op_forward_packed enqueues it -- the same kernels, bit-identical logits -- whose stores of the entries `pool` selects (numbered
 * as in op_hidden_request) go to ONE packed fp32 scratch entry [total_tokens][hidden]; a reduction kernel of the call's own
 * pools the scratch behind each entry and the next entry reuses it (the stream orders this): the extra device memory is one
 * entry plus the output, not num_layers + 1 entries.
 *   kind     OP_HIDDEN_POOL_FIRST  the row of token 0 of each sequence (what classifier_pooling = "cls" reads): bit-identical
 *                                  to that row of the fp32 entry op_forward_packed_hidden writes
 *            OP_HIDDEN_POOL_MEAN   the mean over the sequence's tokens of the fp32 rows of the entry: fp64 partials over 64
 *                                  consecutive tokens each, added in token order; the partials added in index order; one fp64
 *                                  division; one rounding to fp32.  No floating-point atomics: the same bits on every call, on
 *                                  every stream, under every batch composition and every chunk_rows (the rule of op_loss), within
 *                                  1 fp32 ulp of the exact mean
 *   select   host array of num_layers + 1 flags, or NULL = every entry
 *   out_dev  fp32 [n_sel][n_seqs][hidden], the selected entries in order.  EVERY element is written (the caller zeroes
 *            nothing); a sequence of length 0 gives a row of exactly +0.0 under both kinds
 *   scratch_dev / scratch_bytes  caller-allocated, at least total_tokens * hidden * 4 bytes, 16-byte aligned; may hold
 *            anything on entry, holds the last selected entry afterwards
 * `req` (may be NULL) is an ordinary op_hidden_request riding on the same call, with its own selection, dtype and layout; an
 * entry both select is stored once (into the scratch) and copied from there into `req`'s entry: the same values.  The final
 * entry follows op_config.prune_pre_final_norm as in op_forward_packed_hidden.  No handle state is stored: as stream-safe as
 * op_forward_packed (a scratch per concurrent call).  OP_ERR_INVALID before anything is enqueued, and -- for the requests' own
 * fields -- before the handle is looked at: pool == NULL, a wrong struct_bytes of either request, an unknown kind, a misaligned
 * scratch, everything op_forward_packed_hidden refuses in `req`; once the handle is known: out_dev or scratch_dev NULL, or
 * scratch_bytes below one entry, with an entry selected of a non-empty batch. */
enum op_hidden_pool_kind { OP_HIDDEN_POOL_FIRST = 0, OP_HIDDEN_POOL_MEAN = 1 };
typedef struct op_pool_request {
  uint32_t struct_bytes; /* sizeof(op_pool_request) */
  int32_t kind;          /* enum op_hidden_pool_kind */
  const uint8_t* select; /* host array of num_layers + 1 flags, or NULL = all; entry i = hidden_states[i] */
  float* out_dev;        /* fp32 [n_sel][n_seqs][hidden] */
  void* scratch_dev;     /* one packed fp32 entry: total_tokens * hidden * 4 bytes, 16-byte aligned */
  size_t scratch_bytes;
} op_pool_request;
int op_forward_packed_pooled(op_handle* h, const int32_t* ids_dev, const int32_t* cu_seqlens_dev,
                             const int32_t* cu_seqlens_host, int n_seqs, int total_tokens, int max_seqlen,
                             float* prune_logits_dev, float* rank_logits_dev, float* keep_prob_dev,
                             void* workspace_dev, size_t workspace_bytes, void* hip_stream, const op_hidden_request* req,
                             const op_pool_request* pool);

/* Replaces: output_attentions=True of the reference forward under eager attention (standalone.py:1689, 1727; HF :166-185):
 * the softmax probabilities of ONE layer, as a side pass over that layer's input hidden state.  Additive to ABI 10
 * (op_abi_version() is unchanged: detect the two calls by symbol).  The residual stream is fp32 at every layer boundary on every
 * kernel set, so the pass is the same whatever set the handle's forward runs on, and it touches none of the forward's kernels
 * or its workspace:
 *   hidden_dev  packed fp32 [total_tokens][hidden] = hidden_states[layer], the INPUT of that layer: entry `layer` of
 *               op_forward_packed_hidden (pad_width 0, OP_HIDDEN_F32)
 *   out_dev     [n_seqs][num_heads][pad_width][pad_width] fp32; out[s][h][i][j] = the probability query token i of sequence
 *               s puts on key token j in head h.  Only keys j < len[s] are visible, on a sliding-window layer only those with
 *               |i - j| <= local_attention / 2; the layer's own RoPE theta, q scaled by head_dim^-0.5 -- what the attention
 *               kernel of kernel set "fp32" computes before its P V product.
 * EVERY element of out_dev is written (the caller zeroes nothing, as with op_unpack_padded): exactly +0.0 at masked keys, at keys
 * >= len[s], on whole query rows i >= len[s], and out to pad_width in both directions.  DIFFERENCE to the reference: it holds a
 * softmax row at padded query positions (over the visible keys); this call returns zeros there, as the hidden states do.
 * Arithmetic: the fp32 kernels of kernel set "fp32" -- LayerNorm(attn_norm) (none on layer 0, as in the forward), the q | k
 * column tiles of the Wqkv projection with RoPE on the fp32-input MFMA (v is not computed) -- and one kernel of the call's own:
 * two passes over the visible 64-key tiles, the first for the row maximum and sum, the second stores expf(s - max) / sum.  A
 * probability depends on its own sequence only.  The pass needs the fp32 weight packs: OP_ERR_UNSUPPORTED on a handle created
 * without OP_FLAG_F32_PACKS (the message names the flag); any handle shape (row, panel, tiled).
 * Refused with OP_ERR_INVALID before anything is enqueued and before the handle is looked at: a NULL request, a wrong
 * struct_bytes, a dtype other than OP_HIDDEN_F32, a pad_width below max_seqlen (or 0 for a non-empty batch), hidden_dev /
 * out_dev NULL for a non-empty batch, n_seqs * pad_width beyond 2^31 - 1 (element counts themselves are size_t).  `layer` is
 * checked once the handle is known.
 * The workspace is the call's own: op_attention_workspace_bytes (row maps, the state in the row layout, the LayerNorm plane, q
 * and k; large batches go through in chunks of sequences, as in the forward).  It may hold anything on entry, and nothing
 * outside it and out_dev is written.  Asynchronous on hip_stream (cu_seqlens_host == NULL: cu_seqlens_dev is read back, which
 * synchronises the stream once); no handle state is stored: as stream-safe as op_forward_packed. */
typedef struct op_attention_request {
  uint32_t struct_bytes;   /* sizeof(op_attention_request) */
  int32_t layer;           /* 0 <= layer < num_layers */
  int32_t dtype;           /* OP_HIDDEN_F32 only for now; anything else OP_ERR_INVALID */
  int32_t pad_width;       /* >= max_seqlen (and > 0 for a non-empty batch) */
  const float* hidden_dev; /* packed fp32 [total_tokens][hidden] = hidden_states[layer] */
  void* out_dev;           /* [n_seqs][num_heads][pad_width][pad_width] fp32 */
} op_attention_request;
size_t op_attention_workspace_bytes(const op_handle* h, int n_seqs, int total_tokens, int max_seqlen);
int op_attention_probs(op_handle* h, const int32_t* cu_seqlens_dev, const int32_t* cu_seqlens_host, int n_seqs, int total_tokens,
                       int max_seqlen, const op_attention_request* req, void* workspace_dev, size_t workspace_bytes,
                       void* hip_stream);

/* Replaces: reading one query row out of output_attentions=True -- "what does the pooled token look at" -- without the
 * [heads][L][L] matrices: ONE query position per sequence of ONE layer, as a side pass over hidden_states[layer].  Additive to
 * ABI 10 (op_abi_version() is unchanged: detect the call by symbol).  Inputs, arithmetic, fp32 packs and workspace are those of
 * op_attention_probs (op_attention_workspace_bytes is sufficient; large batches go through in chunks of sequences): the same
 * LayerNorm and q | k projection over all tokens, then one kernel of the call's own that walks the visible 64-key tiles of the
 * selected query's 64-query block in op_attention_probs' order through the same device functions, with the selected query in a
 * 16-query fragment.
 *   query_pos_dev   int32 [n_seqs]: the query position of each sequence; NULL = position 0 everywhere
 *   query_pos_host  NULL, or the caller's host copy of query_pos_dev: a negative position in it is refused (OP_ERR_INVALID)
 *   reduce_heads 0  out_dev [n_seqs][num_heads][pad_width] fp32; out[s][h][j] is BIT-IDENTICAL to
 *                   out[s][h][query_pos[s]][j] of op_attention_probs on the same inputs
 *   reduce_heads 1  out_dev [n_seqs][pad_width] fp32: the mean over heads of those fp32 probabilities, accumulated in fp64 in
 *                   head order, divided once, rounded to fp32 once (at most 64 heads: OP_ERR_UNSUPPORTED beyond)
 * EVERY element of out_dev is written: exactly +0.0 at masked keys, at keys >= len[s] and out to pad_width; a whole row of +0.0
 * when the position is at or beyond len[s] (an empty sequence included) or negative (on the device a position is compared
 * with the length before it is used as an index).
 * OP_ERR_UNSUPPORTED on a handle created without OP_FLAG_F32_PACKS (the message names the flag).  Refused with OP_ERR_INVALID
 * before anything is enqueued and before the handle is looked at: a NULL request, a wrong struct_bytes, a reduce_heads other
 * than 0 / 1, a pad_width below max_seqlen (or 0 for a non-empty batch), hidden_dev / out_dev NULL for a non-empty batch,
 * query_pos_host without query_pos_dev, a negative position in query_pos_host.  `layer` is checked once the handle is known.
 * Asynchronous on hip_stream (cu_seqlens_host == NULL: cu_seqlens_dev is read back, which synchronises the stream once); no
 * handle state is stored. */
typedef struct op_attention_rows_request {
  uint32_t struct_bytes;         /* sizeof(op_attention_rows_request) */
  int32_t layer;                 /* 0 <= layer < num_layers */
  int32_t pad_width;             /* >= max_seqlen (and > 0 for a non-empty batch) */
  int32_t reduce_heads;          /* 0: a row per head; 1: their mean */
  const float* hidden_dev;       /* packed fp32 [total_tokens][hidden] = hidden_states[layer] */
  const int32_t* query_pos_dev;  /* [n_seqs], or NULL = position 0 */
  const int32_t* query_pos_host; /* optional host copy of query_pos_dev */
  float* out_dev;                /* [n_seqs][num_heads][pad_width] or [n_seqs][pad_width] fp32 */
} op_attention_rows_request;
int op_attention_rows(op_handle* h, const int32_t* cu_seqlens_dev, const int32_t* cu_seqlens_host, int n_seqs, int total_tokens,
                      int max_seqlen, const op_attention_rows_request* req, void* workspace_dev, size_t workspace_bytes,
                      void* hip_stream);

/* The padded boundary on the device.  Replaces: the reference forward taking `input_ids[B, L]` + `attention_mask[B, L]` as
 * they come from the tokenizer (standalone.py:1666-1690) and returning `pruning_logits[B, L, 2]` (standalone.py:1695-1739);
 * additive to ABI 10 (op_abi_version() is unchanged: detect the two calls by symbol).
 *
 * op_pack_padded: padded device tensors -> the inputs of op_forward_packed, without the batch visiting the host.
 *   ids_dev   [n_rows][width] int32 or int64 (ids_dtype: OP_INT_I32 / OP_INT_I64), contiguous
 *   mask_dev  [n_rows][width] uint8 (= bool), int32 or int64 (mask_dtype), contiguous; != 0 means "token".  NULL: every row
 *             is full (mask_dtype is ignored)
 *   ids_packed_dev  room for n_rows * width int32; receives ids[r][j] of the j < len[r] positions, rows end to end
 *   cu_seqlens_dev / cu_seqlens_host  [n_rows + 1] prefix offsets of the row lengths, on the device and on the host
 *   report    struct_bytes set by the caller; the call fills the rest (total_tokens and max_seqlen are what
 *             op_workspace_bytes / op_forward_packed ask for)
 * Two checks run on the device, because a batch that never visits the host cannot be checked there:
 *   status bit 0  a row's mask is not ones-then-zeros (left padding, a hole): the packed path derives positions from token
 *                 order.  (mask_row, mask_col) = the first zero entry, in row-major order, that has a non-zero entry behind
 *                 it in its row;
 *   status bit 1  an id outside 0 <= id < vocab_size at a position whose mask is non-zero (ids under padding are not
 *                 looked at).  (id_row, id_col, id_value) = the first one in row-major order.  op_forward_packed itself
 *                 only clamps such an id (a memory-safety net): this is the call that refuses it, as nn.Embedding does.
 * Returns OP_OK when status == 0; otherwise OP_ERR_INVALID with the report filled and an op_last_error text that names
 * row, column and id (cu_seqlens and ids_packed then hold the counts of non-zero entries: not a batch to run).
 * The call enqueues its kernels on hip_stream, copies cu_seqlens and the report to the host and SYNCHRONISES THAT STREAM
 * ONCE: the forward's grids and workspace need total_tokens and max_seqlen on the host (op_forward_packed reads cu_seqlens
 * back the same way when it is given no host copy).  A stream that is being captured is therefore refused (OP_ERR_STATE).
 * The small device status block and its pinned staging belong to the handle: like every call on a handle, serialised by
 * the caller.  Refused with OP_ERR_INVALID before anything is enqueued (and before the handle is looked at): a NULL report,
 * a wrong struct_bytes, an unknown ids_dtype / mask_dtype, a negative n_rows / width, n_rows * width >= 2^31, a NULL
 * buffer.  n_rows == 0 or width == 0 launches nothing (cu_seqlens = 0).  Rows longer than max_position_embeddings are
 * op_forward_packed's business.
 *
 * op_unpack_padded: packed_dev [total_tokens][channels] fp32 (channels = 2: prune_logits_dev, 1: keep_prob_dev) ->
 * padded_dev [n_rows][width][channels]: EVERY element is written, the value at positions below the row's length and +0.0
 * beyond it (the caller zeroes nothing).  Asynchronous on hip_stream.  width is not checked against the lengths: positions
 * at or beyond width are simply not produced. */
enum op_int_dtype { OP_INT_I32 = 0, OP_INT_I64 = 1, OP_INT_U8 = 2 };
typedef struct op_padded_report {
  uint32_t struct_bytes; /* sizeof(op_padded_report) */
  int32_t total_tokens, max_seqlen;
  int32_t status;             /* bit 0: mask not ones-then-zeros; bit 1: id outside the embedding table */
  int32_t mask_row, mask_col; /* first offender of bit 0 (row-major); -1 when clear */
  int32_t id_row, id_col;     /* first offender of bit 1 (row-major); -1 when clear */
  int64_t id_value;
} op_padded_report;
int op_pack_padded(op_handle* h, const void* ids_dev, int ids_dtype, const void* mask_dev, int mask_dtype, int n_rows, int width,
                   int32_t* ids_packed_dev, int32_t* cu_seqlens_dev, int32_t* cu_seqlens_host, op_padded_report* report,
                   void* hip_stream);
int op_unpack_padded(op_handle* h, const float* packed_dev, const int32_t* cu_seqlens_dev, int n_rows, int width, int channels,
                     float* padded_dev, void* hip_stream);

/* A forward under ANY [n_rows][width] attention mask: left padding, holes, ones behind the padding.  Replaces: the reference
 * forward handing whatever mask it is given to the encoder under eager attention (standalone.py:1666-1739); additive to ABI 10
 * (op_abi_version() is unchanged: detect the two calls by symbol).  The packed calls above derive RoPE positions and the sliding
 * window from token order and so take ones-then-zeros rows only (op_pack_padded status bit 0); this one runs DENSE:
 *   - every one of the n_rows * width positions is a row of the forward, at position = its column; masked positions are
 *     queries too (the reference pools column 0 under cls pooling, and under left padding column 0 is a pad token);
 *   - the mask removes KEYS: a query sees the positions with mask != 0, on a sliding-window layer those of them with
 *     |q - k| <= local_attention / 2;
 *   - a query left without a key (a masked position of a sliding-window layer whose whole window is masked) gets what the
 *     reference's softmax over masked_fill(finfo.min) gives it: uniform weights over all `width` columns of its row, i.e. the
 *     plain mean of v over the row, per head.  Such a position is never a key: it shows in the cls-pooled ranking logit only;
 *   - mean pooling sums the final-norm output over the mask != 0 positions and divides by their count.
 * Outputs: prune_logits_dev [n_rows][width][2] fp32, exactly +0.0 wherever mask == 0 (the reference holds values there);
 * rank_logits_dev [n_rows][num_labels].  A row whose mask is all zeros gives zeros in both (the reference: a finite cls value,
 * a NaN mean).  EVERY element of both outputs is written.
 * Arithmetic: kernel set "fp32" (OP_KS_F32) whatever set the handle has selected -- its LayerNorm, GEMM epilogues and RoPE
 * lookup, with the attention kernel and the ranking head taking the key mask.  Under a ones-then-zeros mask the outputs at
 * mask != 0 and the ranking logits are BIT-IDENTICAL to that set's op_forward_packed on the packed rows.  The dense pass
 * computes the pads and runs at the fp32 MFMA rate: a capability, not a fast path.  Needs the fp32 weight packs:
 * OP_ERR_UNSUPPORTED on a handle created without OP_FLAG_F32_PACKS (the message names the flag).
 *   ids_dev   [n_rows][width] int32, contiguous.  EVERY position is embedded, so an id outside 0 <= id < vocab_size is refused
 *             wherever it sits, under a zero of the mask too (as nn.Embedding does): OP_ERR_INVALID, report->status = 2 and
 *             (id_row, id_col, id_value) = the first one in row-major order, named in op_last_error; nothing else has run
 *   mask_dev  [n_rows][width] uint8, contiguous; != 0 means "key"
 *   report    struct_bytes set by the caller; the call fills the rest
 * The workspace is the call's own: op_masked_workspace_bytes (the dense cu_seqlens, the id check's status word, the row means
 * of v, and a forward workspace of kernel set "fp32" for n_rows sequences of `width` tokens; large batches go through in
 * chunks of rows, as in the forward).  It may hold anything on entry, and nothing outside it and the two outputs is written;
 * op_workspace_bytes and op_debug_workspace_layout are unchanged.  The id check is read back before the forward is enqueued:
 * the call SYNCHRONISES hip_stream ONCE, and a stream that is being captured is refused (OP_ERR_STATE).  No handle state is
 * stored: as stream-safe as op_forward_packed.
 * Refused before anything is enqueued: OP_ERR_INVALID for a NULL report, a wrong struct_bytes, n_rows < 0, width < 0,
 * n_rows * width >= 2^31, a NULL buffer of a non-empty batch (all before the handle is looked at), a NULL handle,
 * width > max_position_embeddings; OP_ERR_UNSUPPORTED without the fp32 packs; OP_ERR_WORKSPACE for a workspace that is too
 * small or not 256-byte aligned.  n_rows == 0 or width == 0 returns OP_OK with nothing written. */
typedef struct op_masked_report {
  uint32_t struct_bytes;  /* sizeof(op_masked_report) */
  int32_t status;         /* bit 1 (= 2, as op_padded_report): an id outside the embedding table */
  int32_t id_row, id_col; /* its first offender (row-major); -1 when clear */
  int64_t id_value;
} op_masked_report;
size_t op_masked_workspace_bytes(const op_handle* h, int n_rows, int width);
int op_forward_masked(op_handle* h, const int32_t* ids_dev, const uint8_t* mask_dev, int n_rows, int width, void* workspace_dev,
                      size_t workspace_bytes, float* prune_logits_dev, float* rank_logits_dev, op_masked_report* report,
                      void* hip_stream);

/* op_forward_masked on the handle's SELECTED kernel set.  The same arguments, semantics, outputs, id check, single stream
 * synchronisation and capturing-stream refusal; the refusals come in the same order with the same wording (under this call's
 * name).  Additive to ABI 10 (op_abi_version() is unchanged: detect the call by symbol).
 * Arithmetic: the kernel set the handle's op_forward_packed runs on (the default selection, op_select_kernel_set, op_calibrate;
 * the layer mask of sets 8 / 9 and the range guard of the fp16 + e4m3 sets included: a flagged chunk leaves NaN logits at
 * mask != 0) -- its RoPE, whole-layer kernels, embedding and head fusions unchanged.  Three places take the mask: the
 * attention kernel (a key-mask form of the same instantiation: the same tiles in the same order), mean pooling in the
 * ranking head, and the zeros of the outputs.  A query without a key takes the mean of v over its row AS THE SET STORES v
 * (sliding-window layers) or +0.0 (full-attention layers: only in a row whose mask is all zeros).  Under a ones-then-zeros
 * mask the outputs at mask != 0 and the ranking logits are BIT-IDENTICAL to the handle's op_forward_packed on the packed
 * rows, given the same attention plan (OP_FLAG_ATT_WAVES_4 / _8 pin it; the default plan reads the row lengths).  The dense
 * pass still computes the pads.  It does NOT need the fp32 weight packs.
 * OP_ERR_UNSUPPORTED, in the place of op_forward_masked's check for the packs and with a message that names
 * op_forward_masked: a handle on the tiled path (neither the row nor the panel path; OP_FLAG_FORCE_TILED included), and a
 * handle whose selected set is "fp32" (that call IS its masked forward).
 * The workspace is the call's own: op_masked_native_workspace_bytes (the dense cu_seqlens, the id check's status word, the
 * mask in the row layout, the row means of v, and a forward workspace of the selected set for n_rows sequences of `width`
 * tokens).  It may hold anything on entry; op_workspace_bytes and op_debug_workspace_layout are unchanged. */
size_t op_masked_native_workspace_bytes(const op_handle* h, int n_rows, int width);
int op_forward_masked_native(op_handle* h, const int32_t* ids_dev, const uint8_t* mask_dev, int n_rows, int width,
                             void* workspace_dev, size_t workspace_bytes, float* prune_logits_dev, float* rank_logits_dev,
                             op_masked_report* report, void* hip_stream);

/* Evaluation losses on the device.  Replaces: the losses the reference's inference file computes in its own forward when it
 * is handed labels -- nn.BCEWithLogitsLoss / nn.CrossEntropyLoss on the ranking logits (standalone.py:1707-1722) and
 * nn.CrossEntropyLoss over the pruning logits of the attention_mask == 1 positions (standalone.py:3870-3881) -- plus the
 * ranking term of its training objective, nn.MSELoss (losses.py:56-57), so that a checkpoint can be validated by it.
 * Additive to ABI 10 (op_abi_version() is unchanged: detect the call by symbol).  A side pass over logits that are already
 * on the device: it touches none of the forward's kernels or its workspace.
 *   kind               logits_dev                          labels_dev (labels_dtype)            term                    mean over
 *   OP_LOSS_TOKEN_CE   prune_logits_dev [total_tokens][2]  [n_rows][width] int32 / int64        2-class cross entropy   tokens whose label != ignore_index
 *                      as op_forward_packed leaves them    token t of row r reads
 *                      (packed: no unpacking)              labels[r][t - cu[r]]
 *   OP_LOSS_RANK_BCE   rank_logits_dev [n_rows][1]         [n_rows] fp32 (OP_LABELS_F32)        max(z,0) - z y          n_rows
 *                                                                                               + log1p(exp(-|z|))
 *   OP_LOSS_RANK_CE    rank_logits_dev [n_rows][C >= 2]    [n_rows] int32 / int64               C-class cross entropy   rows whose label != ignore_index
 *   OP_LOSS_RANK_MSE   rank_logits_dev [n_rows][C]         [n_rows][C] fp32 (OP_LABELS_F32)     (z - y)^2               n_rows * C
 * channels = 2 / 1 / C / C; width, total_tokens and cu_seqlens_dev [n_rows + 1] belong to the token kind and are ignored
 * by the others.  Labels under padding (column >= the row's length) are never read.
 * Arithmetic: every term in fp64 from the fp32 inputs in its stable form -- softplus(z_other - z_label) =
 * max(d, 0) + log1p(exp(-|d|)) for two classes, log-sum-exp after subtracting the maximum for C (the maximum's own term is
 * the 1 of a log1p, which for C = 2 is the same softplus) -- so logits of magnitude 1e4 lose nothing and a loss of 1e-35 keeps
 * its digits.  The sum is fp64 in a FIXED order (per-block partials in a tree, then a single-block launch that adds
 * them in index order, divides once and rounds once to fp32; no floating-point atomics): the same inputs give the same bits
 * on every call and on every stream, and the result is within 1 fp32 ulp of the exact mean.  A count of zero (n_rows == 0,
 * every label ignored) gives 0.0 / 0 = NaN, as torch does; n_rows == 0 launches the finishing step only.
 *   loss_dev   one fp32, always written
 *   terms_dev  NULL, or fp32 [total_tokens] (token kind) / [n_rows] / [n_rows][C]: every element is written (the caller
 *              zeroes nothing), the fp64 term rounded once; exactly +0.0 where the label is ignored
 * A label outside 0 <= y < C that is not ignore_index is never used as an index and contributes nothing; the first one in
 * row-major order is reported (status bit 0; bad_row, bad_col, bad_value; bad_col is 0 for OP_LOSS_RANK_CE) and makes the
 * loss NaN.
 *   report == NULL  fully asynchronous on hip_stream, nothing is read back (capturable).
 *   report != NULL  struct_bytes set by the caller; the result block is copied back and hip_stream is SYNCHRONISED ONCE.  A
 *                   stream that is being captured is refused (OP_ERR_STATE), as in op_pack_padded.  A label out of range
 *                   returns OP_ERR_INVALID with the report filled and an op_last_error text that names row, column and value.
 * The 5 KB scratch block of the partials belongs to the handle whatever the batch size (the grid is capped, blocks stride
 * over the rows): like every call on a handle, serialised by the caller.  Refused with OP_ERR_INVALID before anything is
 * enqueued (and before the handle is looked at): a NULL request, a wrong struct_bytes (request or report), an unknown kind
 * or labels_dtype, a labels_dtype that does not fit the kind, a negative size, channels != 2 (token kind) / != 1 (BCE) / < 2
 * (rank CE), total_tokens beyond n_rows * width, n_rows * width or n_rows * channels >= 2^31, a NULL loss_dev, a NULL
 * buffer of a non-empty batch. */
enum op_loss_kind { OP_LOSS_TOKEN_CE = 0, OP_LOSS_RANK_BCE = 1, OP_LOSS_RANK_CE = 2, OP_LOSS_RANK_MSE = 3 };
enum op_labels_dtype { OP_LABELS_F32 = 3 }; /* beside OP_INT_I32 / OP_INT_I64 of enum op_int_dtype */
typedef struct op_loss_request {
  uint32_t struct_bytes; /* sizeof(op_loss_request) */
  int32_t kind;          /* enum op_loss_kind */
  const float* logits_dev;
  const void* labels_dev;
  int32_t labels_dtype; /* OP_INT_I32 / OP_INT_I64 (the two CE kinds) or OP_LABELS_F32 (BCE, MSE) */
  int32_t n_rows;
  int32_t width;        /* token kind: columns of labels_dev */
  int32_t channels;     /* logits per token / row */
  int32_t total_tokens; /* token kind: rows of logits_dev */
  int32_t reserved;
  const int32_t* cu_seqlens_dev; /* token kind: [n_rows + 1] */
  int64_t ignore_index;          /* callers pass -100 */
  float* terms_dev;              /* nullable */
} op_loss_request;
typedef struct op_loss_report {
  uint32_t struct_bytes; /* sizeof(op_loss_report) */
  int32_t status;        /* bit 0: a label out of range */
  int32_t bad_row, bad_col; /* the first one in row-major order; -1 when clear */
  int64_t bad_value;
  int64_t count; /* terms that entered the mean */
  double sum;    /* their fp64 sum */
  float loss;    /* = *loss_dev */
  int32_t reserved;
} op_loss_report;
int op_loss(op_handle* h, const op_loss_request* req, float* loss_dev, op_loss_report* report, void* hip_stream);

/* The running audit of a calibrated kernel set (HipEncoder's audit policy "running").  Replaces: nothing
 * in the reference, which picks its dtype once at load (standalone.py:1631-1642) and never looks again.  Additive to ABI 10
 * (op_abi_version() is unchanged: detect the five calls by symbol).  The handle owns a bitmap of vocab_size bits -- the token
 * ids the audited rows have held -- and the longest audited row.  Both belong to ONE arithmetic: they start empty at op_create
 * and are emptied by op_coverage_reset, by op_load_weight of the embedding table, by op_calibrate, and whenever the handle runs
 * another kernel set (or another layer mask of sets 8 / 9) than the one they were collected under -- a new arithmetic has seen
 * nothing.  Emptying enqueues nothing: the memory is cleared on the stream of the next scan or commit, which is also where the
 * kernel set is looked at, so op_select_kernel_set to another set AND BACK between two such calls (the audit's own detour
 * through the reference set) keeps the coverage.  Rows are rows of a packed batch (ids_dev [total_tokens], cu_seqlens_dev
 * [n_seqs + 1]); rows_dev [n_rows] int32 lists some of them.  On the device a listed row outside 0 <= row < n_seqs is skipped
 * and row bounds are held inside [0, total_tokens), whatever cu_seqlens_dev holds.  Every call checks its arguments before it
 * enqueues (OP_ERR_INVALID: a NULL report or buffer, a wrong struct_bytes, a negative count) and before it looks at the
 * handle.  Like every call on a handle, serialised by the caller.
 *
 * op_coverage_scan: read-only.  row_novel_dev[s] = the number of positions of row s whose id has no bit in the bitmap
 *   (duplicates count once per position; an id outside 0 <= id < vocab_size counts as novel and is never used as an index).
 *   The report receives the sum of those counts, the longest row of the batch with its index (the first of equals; -1 for
 *   an empty batch) and the handle's longest audited row.  The call copies the report to the host and SYNCHRONISES
 *   hip_stream ONCE, as op_pack_padded does; a stream that is being captured is refused (OP_ERR_STATE).
 * op_coverage_commit: sets the bit of every id of the listed rows and raises the longest audited row.  Asynchronous.
 * op_coverage_reset: empties both.
 * op_gather_rows: lays the listed rows end to end in sub_ids_dev (room for their tokens) and writes their prefix offsets to
 *   sub_cu_dev [n_rows + 1] -- a packed batch for op_forward_packed.  Asynchronous.
 * op_audit_compare: err_dev[0] = max |difference| between the pruning logits ([token][2]) of the listed rows' tokens in
 *   prune_dev and the same tokens in sub_prune_dev (laid out by sub_cu_dev, as op_gather_rows leaves them), and between the
 *   rows' ranking logits rank_dev[rows[i]][num_labels] and sub_rank_dev[i][num_labels]; +inf when a value on either side is
 *   not finite, a listed row is not a row of the batch, or a row's two lengths differ.  The call initialises the cell on
 *   hip_stream (the caller zeroes nothing); fp32 max does not depend on the order, so the result is exact.  n_rows == 0
 *   leaves +0.0.  Asynchronous. */
typedef struct op_coverage_report {
  uint32_t struct_bytes;      /* sizeof(op_coverage_report) */
  int32_t novel_tokens;       /* sum of row_novel_dev */
  int32_t longest_row_tokens; /* the batch's longest row ... */
  int32_t longest_row;        /* ... and its index */
  int32_t max_audited_tokens; /* the handle's longest audited row */
} op_coverage_report;
int op_coverage_scan(op_handle* h, const int32_t* ids_dev, const int32_t* cu_seqlens_dev, int n_seqs, int total_tokens,
                     int32_t* row_novel_dev, op_coverage_report* report, void* hip_stream);
int op_coverage_commit(op_handle* h, const int32_t* ids_dev, const int32_t* cu_seqlens_dev, int n_seqs, int total_tokens,
                       const int32_t* rows_dev, int n_rows, void* hip_stream);
int op_coverage_reset(op_handle* h);
int op_gather_rows(op_handle* h, const int32_t* ids_dev, const int32_t* cu_seqlens_dev, int n_seqs, int total_tokens,
                   const int32_t* rows_dev, int n_rows, int32_t* sub_ids_dev, int32_t* sub_cu_dev, void* hip_stream);
int op_audit_compare(op_handle* h, const float* prune_dev, const float* rank_dev, const int32_t* cu_seqlens_dev, int n_seqs,
                     int total_tokens, const int32_t* rows_dev, int n_rows, const float* sub_prune_dev, const float* sub_rank_dev,
                     const int32_t* sub_cu_dev, float* err_dev, void* hip_stream);

/* Replaces: the per-fragment `float(block_probs[start:end].mean())` of the reference's post-processing
 * (standalone.py:3075-3082), evaluated on the device on the keep-probabilities a forward left there:
 *   seg_dev [n_seg, 2] int32  token ranges [start, end) into keep_prob_dev (clamped to [0, n_values))
 *   out_dev [n_seg]    fp32   mean of the range in numpy's float32 pairwise order, bit for bit; 1.0 for
 *                             an empty range (ref :3081)
 * so that process() copies back 4 bytes per fragment instead of 4 per token.  Enqueued on hip_stream. */
int op_segment_means(op_handle* h, const float* keep_prob_dev, int n_values, const int32_t* seg_dev, int n_seg,
                     float* out_dev, void* hip_stream);

/* Replaces: the host loop that concatenates `[CLS] query [SEP] context [SEP]` rows block by block (standalone.py:2104-2196)
 * for a PREPARED corpus (OpenProvenceModel.prepare_contexts): the fragments' token ids live on the device, a request brings
 * its queries' ids and a plan of rows, and the packed input of op_forward_packed is laid out there.  Additive to ABI 10
 * (op_abi_version() is unchanged: detect the call by symbol).
 *   corpus_dev   [frag_off[n_frag]] int32   the fragments' ids end to end; frag_off_dev / frag_off_host [n_frag + 1] their
 *                                           offsets (non-decreasing from 0; the total stays below 2^31)
 *   query_ids_dev [q_off[n_queries]] int32  the request's queries end to end; q_off_dev / q_off_host [n_queries + 1]
 *   prefix, middle, suffix                  HOST arrays of n_prefix / n_middle / n_suffix ids, at most OP_ASSEMBLE_MAX_PIECE
 *                                           each: the specials layout as a template (for BERT: [CLS], [SEP], [SEP])
 *   plan_dev / plan_host [n_rows][4] int32  per row {query, first_frag, n_frag, clip}: the row is
 *                                           prefix + query + middle + context + suffix, where context = the fragments
 *                                           first_frag .. first_frag + n_frag - 1 of the corpus (consecutive, so one
 *                                           contiguous copy), or with clip > 0 only the first `clip` ids of fragment
 *                                           first_frag followed by the others whole (two copies).  n_frag = 0: no
 *                                           context, clip = 0; or clip = -1: no context AND no suffix, the row is
 *                                           prefix + query + middle (what tokenizers build for an empty second sequence)
 *   cu_seqlens_dev / cu_seqlens_host [n_rows + 1]  the rows' offsets in ids_dev, from 0 to total_tokens: known on the host
 *                                           from lengths alone, so nothing is read back
 *   ids_dev [total_tokens] int32            the output; nothing outside [0, total_tokens) is written, and every element
 *                                           of it is written when the host and device copies agree
 * The *_host arrays are the caller's host copies of the *_dev ones; the call checks the request on them and the kernel
 * reads the device copies, holding every index it finds there inside the buffers all the same.  Asynchronous on hip_stream;
 * the handle's state is neither read nor changed beyond its device and error text.  OP_ERR_INVALID, before anything is
 * enqueued: a NULL request or handle, a wrong struct_bytes, a negative count, a template piece longer than
 * OP_ASSEMBLE_MAX_PIECE (or NULL with a positive count), a NULL buffer while n_rows > 0, a row whose query or fragments lie
 * outside the request / the corpus or whose clip exceeds its first fragment (or is positive without one), offsets that decrease,
 * and cu_seqlens_host not equal to the prefix sums of the plan's row lengths from 0 to total_tokens.  n_rows == 0 with
 * total_tokens == 0 enqueues nothing.  Kernel: a wave per row segment, 16-byte stores where alignment allows, vector
 * stores only, no atomics (csrc/opk_assemble.hip.h). */
#define OP_ASSEMBLE_MAX_PIECE 8
typedef struct op_assemble_request {
  uint32_t struct_bytes; /* sizeof(op_assemble_request) */
  int32_t n_frag;
  int32_t n_queries;
  int32_t n_rows;
  int32_t total_tokens;
  int32_t n_prefix, n_middle, n_suffix;
  const int32_t* prefix; /* host */
  const int32_t* middle; /* host */
  const int32_t* suffix; /* host */
  const int32_t* corpus_dev;
  const int32_t* frag_off_dev;
  const int32_t* frag_off_host;
  const int32_t* query_ids_dev;
  const int32_t* q_off_dev;
  const int32_t* q_off_host;
  const int32_t* plan_dev;
  const int32_t* plan_host;
  const int32_t* cu_seqlens_dev;
  const int32_t* cu_seqlens_host;
} op_assemble_request;
int op_assemble_rows(op_handle* h, const op_assemble_request* req, int32_t* ids_dev, void* hip_stream);

/* Replaces: the per-fragment `float(block_probs[start:end].mean())` of the reference's post-processing
 * (standalone.py:3075-3082) for a PREPARED request, with the token ranges derived on the device from the row plan that
 * op_assemble_rows laid the rows out from -- op_segment_means without the host loop that builds and uploads the ranges.
 * Additive to ABI 10 (op_abi_version() is unchanged: detect the call by symbol).
 *   rows                                    the op_assemble_request of the forward whose keep-probabilities are averaged
 *                                           (corpus_dev, query_ids_dev and the template's ids are not read, the pieces'
 *                                           lengths are)
 *   keep_prob_dev [rows->total_tokens] fp32 the keep-probabilities of that forward (op_forward_packed's keep_prob_dev)
 *   frag_shift_dev [rows->n_frag] int32     per fragment of the corpus, the title tokens in front of its sentence: its
 *                                           range is shifted LEFT by as much (ref :3075-3081); values only, no index
 *   slot_off_dev / slot_off_host [n_rows + 1] int32  where each row's fragments go in the outputs: slot_off[r + 1] =
 *                                           slot_off[r] + n_frag of row r, from any slot_off[0] >= 0 (a forward's slice of
 *                                           the slots of a whole request) to at most n_slots
 *   mean_out_dev [n_slots] fp32, slot_frag_out_dev [n_slots] int32
 *                                           for fragment j of row r, f = first_frag + j, at slot_off[r] + j: the mean of
 *                                           keep_prob over the fragment's range within the row -- from n_prefix + query
 *                                           length + n_middle + the lengths of the row's fragments before it (the first
 *                                           one `clip` long where clip > 0), as long as the fragment, both ends less
 *                                           frag_shift[f], clamped to [0, row length) -- in numpy's float32 pairwise order,
 *                                           divided in float64, bit for bit as op_segment_means; 1.0 for an empty range;
 *                                           and f itself.  Nothing outside the rows' slots is written, and every one of
 *                                           them is when the host and device copies agree.
 * The request is checked on the host copies (rows->*_host, slot_off_host) and the kernel holds every index it reads from the
 * device copies inside the buffers all the same.  Asynchronous on hip_stream; the handle's state is neither read nor changed
 * beyond its device and error text.  OP_ERR_INVALID, before anything is enqueued: a NULL request, rows or handle, a wrong
 * struct_bytes (either struct), a negative count, a NULL buffer while there are rows, a row whose query or fragments lie
 * outside the request / the corpus or whose clip exceeds its first fragment, offsets that decrease, cu_seqlens_host that does
 * not run from 0 to total_tokens, and a slot_off_host that is not the prefix sums of the rows' n_frag inside [0, n_slots].
 * Kernel: a wave per row, a lane per fragment, vector stores only, no atomics (csrc/opk_decide.hip.h). */
typedef struct op_planned_means_request {
  uint32_t struct_bytes; /* sizeof(op_planned_means_request) */
  int32_t n_slots;
  const float* keep_prob_dev;
  const int32_t* frag_shift_dev;
  const int32_t* slot_off_dev;
  const int32_t* slot_off_host;
  float* mean_out_dev;
  int32_t* slot_frag_out_dev;
} op_planned_means_request;
int op_planned_fragment_means(op_handle* h, const op_assemble_request* rows, const op_planned_means_request* req, void* hip_stream);

/* Replaces: op_planned_fragment_means for a request whose contexts may also occur further LEFT in their rows, i.e. the
 * reference's own way of placing a context (standalone.py:2104-2196): it does not compute where the context starts, it looks the
 * whole context up in the finished row and takes the first place it occurs (`_find_subsequence`).  Almost always that is
 * n_prefix + query length + n_middle; it is earlier when the context's ids also occur in prefix + query + middle, or in those
 * followed by the beginning of the context's own copy -- and the fragments' ranges, means and kept sentences start there.
 * Additive to ABI 10 (op_abi_version() is unchanged: detect the call by symbol).
 *   rows, req                               exactly what op_planned_fragment_means takes, read and checked the same way
 *   ids_dev [rows->total_tokens] int32      the rows themselves: the output of op_assemble_rows for the same `rows`
 *   ctx_start_out_dev [rows->n_rows] int32  per row r, with head_len = n_prefix + query length + n_middle and n_ctx = the ids
 *                                           of the row's fragments (the first one `clip` long where clip > 0), held to row
 *                                           length - head_len: the smallest idx in [0, head_len] with
 *                                           ids[idx + j] == ids[head_len + j] for every 0 <= j < n_ctx (idx = head_len always
 *                                           qualifies).  A row without fragments or without context ids gets head_len and
 *                                           none of its slots is written.
 *   req->mean_out_dev, req->slot_frag_out_dev  as op_planned_fragment_means writes them, with every range starting from
 *                                           ctx_start_out[r] instead of head_len: same shift, same clamp to [0, row length),
 *                                           same float32 pairwise sum and float64 division, 1.0 for an empty range
 * The request is checked on the host copies and the kernel holds every index it reads from the device copies inside the buffers
 * all the same; every id it compares lies inside the row's own [cu[r], cu[r + 1]) within [0, total_tokens).  Asynchronous on
 * hip_stream; the handle's state is neither read nor changed beyond its device and error text.  OP_ERR_INVALID, before anything
 * is enqueued: every refusal of op_planned_fragment_means, and ids_dev or ctx_start_out_dev NULL while there are rows.
 * Kernel: a wave per row; the lookup runs a lane per candidate place in ascending passes of 64 and ends with the first pass
 * that holds a match (at most head_len x n_ctx id compares per row), then a lane per fragment; vector stores only, no atomics,
 * no LDS (csrc/opk_decide.hip.h). */
int op_located_fragment_means(op_handle* h, const op_assemble_request* rows, const op_planned_means_request* req, const int32_t* ids_dev,
                              int32_t* ctx_start_out_dev, void* hip_stream);

/* Replaces: the per-sentence loop of the reference's post-processing (standalone.py:3100-3140) for a PREPARED request: the
 * average of a sentence's fragment means, clamped to [0, 1], the threshold, and the title rule, on the slots
 * op_planned_fragment_means filled.  Additive to ABI 10 (op_abi_version() is unchanged: detect the call by symbol).
 *   instances_dev / instances_host [n_instances][OP_DECISIONS_INSTANCE_WORDS] int32
 *                                           per (query, context) pair of the request {slot_begin, slot_end, sent_out_begin,
 *                                           n_sentences, item_sent_base, title_index}: its fragments' slots
 *                                           [slot_begin, slot_end) in fragment order, where its n_sentences results go,
 *                                           the corpus-wide number of its first sentence, and the sentence the title rule
 *                                           keeps (or -1)
 *   mean_dev [n_slots] fp32, slot_frag_dev [n_slots] int32   the outputs of op_planned_fragment_means
 *   frag_sent_dev [n_frag] int32            per fragment of the corpus, the corpus-wide number of its sentence; within a
 *                                           context it must not decrease from fragment to fragment
 *   threshold                               fp64
 *   avg_out_dev [n_out] fp64, keep_out_dev [n_out] uint8
 *                                           sentence k of an instance, at sent_out_begin + k: its values are the run of the
 *                                           instance's slots whose fragment belongs to sentence item_sent_base + k, widened
 *                                           to fp64; avg = 0.0 without values, the value itself for one, else their sum in
 *                                           numpy's float64 pairwise order divided by their number; then Python's
 *                                           max(0.0, min(avg, 1.0)) (a NaN average comes out as 0.0); keep = avg > threshold;
 *                                           and where title_index >= 0 and any sentence of the instance is kept,
 *                                           keep[title_index] = 1.  Every element is written.
 * Checked on instances_host; the kernel holds what it reads from the device copies inside the buffers all the same.
 * Asynchronous on hip_stream; no handle state.  OP_ERR_INVALID, before anything is enqueued: a NULL request or handle, a wrong
 * struct_bytes, a negative count, a NULL buffer while there is something to read or write, an instance whose slots lie outside
 * [0, n_slots] or run backwards, whose sentences do not start where the previous instance's ended (from 0 to n_out: the
 * instances' results tile the outputs), whose item_sent_base is negative, or whose title_index lies outside
 * [-1, n_sentences).  Kernel: one thread per instance, sequential (the data is a few KB), vector stores only, no atomics
 * (csrc/opk_decide.hip.h). */
#define OP_DECISIONS_INSTANCE_WORDS 6
typedef struct op_decisions_request {
  uint32_t struct_bytes; /* sizeof(op_decisions_request) */
  int32_t n_instances;
  int32_t n_slots;
  int32_t n_frag;
  int32_t n_out;
  double threshold;
  const int32_t* instances_dev;
  const int32_t* instances_host;
  const float* mean_dev;
  const int32_t* slot_frag_dev;
  const int32_t* frag_sent_dev;
  double* avg_out_dev;
  uint8_t* keep_out_dev;
} op_decisions_request;
int op_sentence_decisions(op_handle* h, const op_decisions_request* req, void* hip_stream);

/* Test hook.  Replaces: output_hidden_states=True of the reference forward (standalone.py:1689,
 * 1727).  When `hidden_dev` is non-NULL the next forwards also write the (num_layers+1) hidden
 * states, fp32 [num_layers+1, total_tokens, hidden]; entry num_layers is the post-final_norm
 * tensor, as in HF (transformers >= 5).  Pass NULL to switch capturing off. */
int op_debug_capture_hidden(op_handle* h, float* hidden_dev);

/* Test hook.  Replaces: nothing.  The regions op_forward_packed carves out of a workspace of this geometry, in order, as the
 * carving code itself hands them out (a region added there appears here): entries[i] = {name of the region, offset from
 * the 256-aligned workspace base, bytes used, kind}.  Every region starts on a 256-byte boundary; the last one, rounded up
 * to 256, ends at op_workspace_bytes.  Returns the number of regions (at most max_entries are written; entries may be NULL
 * with max_entries = 0 to ask for the count), OP_ERR_INVALID on a NULL handle or a negative size.  `name` points into the
 * library.  Additive to ABI 10 (op_abi_version() is unchanged: detect the call by symbol).  For tests that fill a workspace
 * with a pattern per kind: an index region must only ever be given in-range values. */
enum op_workspace_kind {
  OP_WS_FLOAT = 0, /* floating-point operands of a kernel (fp32, bf16 / fp16 planes, e4m3 pieces) */
  OP_WS_INDEX = 1, /* int32 row maps and offsets: kernels address memory through them */
  OP_WS_FLAG = 2   /* an int32 flag */
};
typedef struct op_workspace_region {
  const char* name;
  uint64_t offset;
  uint64_t bytes;
  int32_t kind; /* enum op_workspace_kind */
} op_workspace_region;
int op_debug_workspace_layout(const op_handle* h, int n_seqs, int total_tokens, int max_seqlen, op_workspace_region* entries,
                              int max_entries);

/* Test hook.  Replaces: nothing.  The RoPE tables as the library builds them, fp32 [max_pos, 32] each (head_dim 64: entry
 * [p][k] is cos / sin of fp32(p) * inv_freq[k]; the kernels read column k for dimensions k and k + 32), copied to HOST memory.
 *   h == NULL: the tables op_create builds for `theta` and `max_pos`, by the same function, without touching a device
 *              (global_table is ignored);
 *   h != NULL: the handle's own table on its device -- global_table != 0: the full-attention layers' (global_rope_theta),
 *              else the sliding-window layers' -- `max_pos` must be the handle's max_position_embeddings (theta is ignored).
 * Synchronous.  OP_ERR_INVALID on a NULL buffer, max_pos <= 0, theta <= 0 or a max_pos that is not the handle's.
 * Additive to ABI 10 (op_abi_version() is unchanged: detect the call by symbol). */
int op_debug_rope_tables(const op_handle* h, int global_table, float theta, int max_pos, float* cos_host, float* sin_host);

/* Test hook.  Replaces: nothing.  Runs the device functions the forward's kernels are built from (opk_common.hip.h: the
 * operand conversions, the GELU polynomial, the exponentials, RoPE, the keep-probability, the scaled e4m3 MFMA) over `n`
 * input elements at in_dev and stores what they return, as raw bits, at out_dev: one launch on `hip_stream`, asynchronous.
 * `mode` is the wave's conversion mode while the primitive runs: 0 = IEEE overflow (fp16 -> Inf, e4m3 -> NaN), 1 =
 * saturating (MODE.FP16_OVFL: fp16 clamps to +-65504, e4m3 to +-448), the mode of every kernel that writes e4m3 planes.
 * Inputs are fp32 unless stated; a record is written per input element unless stated; "word" = uint32.
 *   kind                 group  record
 *   OP_PROBE_BF16_SPLIT    4    7 words: (hi, lo) bf16 bits of split2, of split2_pk, of split4; f2bf bits
 *   OP_PROBE_F16_PAIR      4    3 words: (hi, lo) fp16 bits of split4_f16; f2h bits
 *   OP_PROBE_F16_F8        4    2 words: hi fp16 bits, lo e4m3 byte of split4_f8 (lo = e4m3((v - hi) x 2^12))
 *   OP_PROBE_E4M3_F16      4    1 word : e4m3 byte of f16x4_to_e4m3 (input: uint16 fp16 bits)
 *   OP_PROBE_E4M3_F32      4    3 words: e4m3 byte of f32x4_to_e4m3; of a weight's e4m3 plane e4m3(v x 2^6); of its lo plane
 *                               e4m3((v - fp16(v)) x 2^18), the last two as the weight pack kernels write them
 *   OP_PROBE_GELU          1    2 fp32 : gelu_erf(x); the same polynomial issued in stages, as the whole-layer kernels do
 *   OP_PROBE_EXP2          1    2 fp32 : the attention's exp2 (v_exp_f32); __expf(x)
 *   OP_PROBE_ROPE          4    2 fp32 per group (x1, x2, cos, sin): rope_lo, rope_hi
 *   OP_PROBE_KEEP_PROB     2    1 fp32 per group (l0, l1): the keep-probability 1 / (1 + e^(l0 - l1)) of the pruning head
 *   OP_PROBE_MFMA_SCALE    2    4 x 256 fp32 per group (input: uint8 e4m3 bytes a, b): the 16 x 16 results of the four scaled
 *                               e4m3 products (K = 128) of the "f16 + fp8" sets with every byte of one operand = a and of
 *                               the other = b: lo(activation) x e4m3(weight) in both operand orders, then e4m3(activation) x
 *                               lo(weight) in both; every element is 128 a b 2^-18
 * OP_ERR_INVALID, before anything is enqueued, on a NULL handle, an unknown kind or mode, an n that is not a multiple of the
 * kind's group, n > 2^31, or a NULL buffer with n > 0; n == 0 launches nothing.  The kernels index by element number only,
 * checked against n: no input value is used as an address.  Additive to ABI 10 (op_abi_version() is unchanged: detect the
 * call by symbol).  tests/test_gpu_primitives.py holds every record to tests/arith_model.py's operand roundings, bit for
 * bit, and the fp32 functions to float64. */
enum op_probe_kind {
  OP_PROBE_BF16_SPLIT = 0,
  OP_PROBE_F16_PAIR = 1,
  OP_PROBE_F16_F8 = 2,
  OP_PROBE_E4M3_F16 = 3,
  OP_PROBE_E4M3_F32 = 4,
  OP_PROBE_GELU = 5,
  OP_PROBE_EXP2 = 6,
  OP_PROBE_ROPE = 7,
  OP_PROBE_KEEP_PROB = 8,
  OP_PROBE_MFMA_SCALE = 9
};
int op_debug_primitive(op_handle* h, int kind, int mode, const void* in_dev, size_t n, void* out_dev, void* hip_stream);

/* Measurement hook: when enabled every kernel launch of the forward is bracketed by HIP events
 * on the launch stream; op_profile_read returns accumulated milliseconds and launch counts per
 * kernel kind (names via op_profile_kind_name) and resets nothing; op_profile_reset clears. */
typedef struct op_profile_entry {
  int32_t kind;
  int32_t launches;
  double total_ms;
} op_profile_entry;
int op_profile_enable(op_handle* h, int enabled);
int op_profile_read(op_handle* h, op_profile_entry* entries, int max_entries); /* returns count, syncs */
int op_profile_reset(op_handle* h);
const char* op_profile_kind_name(int kind);

/* Measurement hook: one wave spins for `spin_us` microseconds (of the constant 100 MHz counter) on `hip_stream` --
 * a stream of its own, next to the timed work -- and writes out_dev[0] = shader cycles elapsed (s_memtime), out_dev[1] =
 * 100 MHz ticks elapsed (s_memrealtime): out[0] / out[1] / 10 = the shader clock in GHz the chip HELD while the timed
 * loop ran (the power limit, not the nominal 2.4 GHz, sets it: DESIGN.md section 4).  out_dev: two uint64. */
int op_debug_clock_probe(op_handle* h, int spin_us, unsigned long long* out_dev, void* hip_stream);

/* Replaces: nothing in the reference (it has no multi-GPU path); helper for SURVEY.md section 8e. */
int op_device_count(int* count);

void op_destroy(op_handle* h);
const char* op_last_error(const op_handle* h);

#ifdef __cplusplus
}
#endif
#endif /* OPEN_PROVENCE_HIP_H */
