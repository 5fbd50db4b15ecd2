"""ctypes binding of ``libopenprovence_hip.so`` (C ABI: ``include/open_provence_hip.h``).

The library is built in-tree by :func:`open_provence_amd.build_ext.build` (hipcc, gfx950).  There is no
fallback of any kind: if the shared object is missing, or there is no HIP device, the product path
raises.
"""

from __future__ import annotations

import ctypes
import os
from pathlib import Path

OP_MAX_LAYERS = 128
OP_ABI_VERSION = 10

OP_OK = 0
OP_ERR_INVALID, OP_ERR_UNSUPPORTED, OP_ERR_HIP, OP_ERR_STATE, OP_ERR_WORKSPACE, OP_ERR_NOMEM = -1, -2, -3, -4, -5, -6
OP_DTYPE_F32, OP_DTYPE_BF16, OP_DTYPE_F16 = 0, 1, 2
OP_PRECISION_BF16X3, OP_PRECISION_BF16, OP_PRECISION_BF16X2, OP_PRECISION_CUSTOM = 0, 1, 2, 3
OP_TERM_LEFT_LO, OP_TERM_RIGHT_LO = 1, 2
# enum op_gemm_family: one term mask per contraction
OP_FAMILIES = ("wqkv", "qk", "pv", "attn_out", "wi", "mlp_out")
OP_FLAG_FORCE_TILED, OP_FLAG_NO_SMALL_BLOCKS, OP_FLAG_ATT_WAVES_4, OP_FLAG_ATT_WAVES_8, OP_FLAG_NO_POLICY_KERNELS = 1, 2, 4, 8, 16
OP_FLAG_NO_LAYER_FUSION = 32
OP_FLAG_LAYER_8X16 = 64
OP_FLAG_LAYER_M32 = 128
OP_FLAG_NO_HEAD_FUSION = 256
OP_FLAG_NO_F8 = 512
OP_FLAG_ATTN_XCD_GROUP = 1024
OP_FLAG_PANEL_F8 = 2048
OP_FLAG_PANEL_F8_WI = 4096
OP_FLAG_NO_LAYER_PAIRS = 8192
OP_FLAG_F32_PACKS = 16384  # keep the fp32 GEMM weights on the device too: kernel set "fp32" (12) needs them
OP_POOL_CLS, OP_POOL_MEAN = 0, 1
# enum op_kernel_set (op_effective_policy / op_select_kernel_set / op_calibrate)
OP_KS_AUTO = -1
KERNEL_SET_NAMES = {0: "bf16x3", 1: "bf16-weights", 2: "bf16", 3: "f16-f8", 4: "f16-f8-w", 5: "bf16x3+wi-f16-f8-w",
                    6: "bf16-weights+wi-f16-f8", 7: "f16", 8: "f16+mlp-f16-f8-w", 9: "f16+mlp-f16-f8",
                    10: "f16-f8-w+attn-f16", 11: "f16-f8+attn-f16", 12: "fp32",
                    -1: "all-terms kernels, cleared lo operands"}
KERNEL_SET_IDS = {name: number for number, name in KERNEL_SET_NAMES.items() if number >= 0}
# kernel sets with an fp16 operand plane: an activation beyond fp16's range comes out as NaN (range guard in engine.py)
FP16_PLANE_SETS = ("f16-f8", "f16-f8-w", "bf16x3+wi-f16-f8-w", "bf16-weights+wi-f16-f8", "f16", "f16+mlp-f16-f8-w", "f16+mlp-f16-f8",
                   "f16-f8-w+attn-f16", "f16-f8+attn-f16")

LIB_NAME = "libopenprovence_hip.so"

# every symbol include/open_provence_hip.h declares (checked by tests/test_abi.py)
EXPORTED_SYMBOLS = (
    "op_abi_version",
    "op_create",
    "op_load_weight",
    "op_weights_ready",
    "op_effective_policy",
    "op_set_compact_operands",
    "op_select_kernel_set",
    "op_mlp_correction_layers",
    "op_select_mlp_correction_layers",
    "op_calibrate",
    "op_workspace_bytes",
    "op_forward_packed",
    "op_forward_packed_hidden",
    "op_forward_packed_pooled",
    "op_attention_workspace_bytes",
    "op_attention_probs",
    "op_attention_rows",
    "op_pack_padded",
    "op_unpack_padded",
    "op_masked_workspace_bytes",
    "op_forward_masked",
    "op_masked_native_workspace_bytes",
    "op_forward_masked_native",
    "op_loss",
    "op_coverage_scan",
    "op_coverage_commit",
    "op_coverage_reset",
    "op_gather_rows",
    "op_audit_compare",
    "op_segment_means",
    "op_assemble_rows",
    "op_planned_fragment_means",
    "op_located_fragment_means",
    "op_sentence_decisions",
    "op_debug_workspace_layout",
    "op_debug_rope_tables",
    "op_debug_primitive",
    "op_debug_capture_hidden",
    "op_profile_enable",
    "op_profile_read",
    "op_profile_reset",
    "op_profile_kind_name",
    "op_device_count",
    "op_debug_clock_probe",
    "op_destroy",
    "op_last_error",
)


class HipLibraryError(RuntimeError):
    """The HIP library is missing, failed to load, or returned an error code."""


class OpConfig(ctypes.Structure):
    _fields_ = [
        ("struct_bytes", ctypes.c_uint32),
        ("device_id", ctypes.c_int32),
        ("vocab_size", ctypes.c_int32),
        ("hidden_size", ctypes.c_int32),
        ("intermediate_size", ctypes.c_int32),
        ("num_layers", ctypes.c_int32),
        ("num_heads", ctypes.c_int32),
        ("num_labels", ctypes.c_int32),
        ("local_attention", ctypes.c_int32),
        ("max_position_embeddings", ctypes.c_int32),
        ("pooling", ctypes.c_int32),
        ("precision", ctypes.c_int32),
        ("norm_eps", ctypes.c_float),
        ("global_rope_theta", ctypes.c_float),
        ("local_rope_theta", ctypes.c_float),
        ("chunk_rows", ctypes.c_int32),
        ("layer_is_global", ctypes.c_uint8 * OP_MAX_LAYERS),
        ("terms", ctypes.c_uint8 * 8),
        ("flags", ctypes.c_uint32),
        ("prune_pre_final_norm", ctypes.c_int32),
    ]


class OpCalibration(ctypes.Structure):
    _fields_ = [
        ("struct_bytes", ctypes.c_uint32),
        ("tolerance", ctypes.c_float),
        ("reference_set", ctypes.c_int32),
        ("default_set", ctypes.c_int32),
        ("chosen_set", ctypes.c_int32),
        ("n_candidates", ctypes.c_int32),
        ("candidate_set", ctypes.c_int32 * 16),
        ("candidate_err", ctypes.c_float * 16),
        ("n_rows", ctypes.c_int32),
        ("n_tokens", ctypes.c_int32),
        ("default_err", ctypes.c_float),
        ("flags", ctypes.c_uint32),
        ("mlp_layers_err", ctypes.c_float),
        ("mlp_layers", ctypes.c_uint64),
    ]


class OpHiddenRequest(ctypes.Structure):
    """``op_hidden_request``: the hidden states one ``op_forward_packed_hidden`` call writes."""

    _fields_ = [
        ("struct_bytes", ctypes.c_uint32),
        ("dtype", ctypes.c_int32),
        ("pad_width", ctypes.c_int32),
        ("select", ctypes.POINTER(ctypes.c_uint8)),
        ("out_dev", ctypes.c_void_p),
    ]


OP_HIDDEN_F32, OP_HIDDEN_BF16 = 0, 1


class OpPoolRequest(ctypes.Structure):
    """``op_pool_request``: the entries one ``op_forward_packed_pooled`` call reduces to a row per sequence, and its scratch."""

    _fields_ = [
        ("struct_bytes", ctypes.c_uint32),
        ("kind", ctypes.c_int32),
        ("select", ctypes.POINTER(ctypes.c_uint8)),
        ("out_dev", ctypes.c_void_p),
        ("scratch_dev", ctypes.c_void_p),
        ("scratch_bytes", ctypes.c_size_t),
    ]


# enum op_hidden_pool_kind, by the names HiddenRequest.pool takes
POOL_KINDS = {"first": 0, "mean": 1}
OP_HIDDEN_POOL_FIRST, OP_HIDDEN_POOL_MEAN = 0, 1


class OpAttentionRequest(ctypes.Structure):
    """``op_attention_request``: the layer whose attention probabilities one ``op_attention_probs`` call writes."""

    _fields_ = [
        ("struct_bytes", ctypes.c_uint32),
        ("layer", ctypes.c_int32),
        ("dtype", ctypes.c_int32),
        ("pad_width", ctypes.c_int32),
        ("hidden_dev", ctypes.c_void_p),
        ("out_dev", ctypes.c_void_p),
    ]


class OpAttentionRowsRequest(ctypes.Structure):
    """``op_attention_rows_request``: the layer and the query position per sequence of one ``op_attention_rows`` call."""

    _fields_ = [
        ("struct_bytes", ctypes.c_uint32),
        ("layer", ctypes.c_int32),
        ("pad_width", ctypes.c_int32),
        ("reduce_heads", ctypes.c_int32),
        ("hidden_dev", ctypes.c_void_p),
        ("query_pos_dev", ctypes.c_void_p),
        ("query_pos_host", ctypes.c_void_p),
        ("out_dev", ctypes.c_void_p),
    ]


class OpPaddedReport(ctypes.Structure):
    """``op_padded_report``: what ``op_pack_padded`` found in one padded batch."""

    _fields_ = [
        ("struct_bytes", ctypes.c_uint32),
        ("total_tokens", ctypes.c_int32),
        ("max_seqlen", ctypes.c_int32),
        ("status", ctypes.c_int32),
        ("mask_row", ctypes.c_int32),
        ("mask_col", ctypes.c_int32),
        ("id_row", ctypes.c_int32),
        ("id_col", ctypes.c_int32),
        ("id_value", ctypes.c_int64),
    ]


class OpMaskedReport(ctypes.Structure):
    """``op_masked_report``: what ``op_forward_masked``'s id check found."""

    _fields_ = [
        ("struct_bytes", ctypes.c_uint32),
        ("status", ctypes.c_int32),
        ("id_row", ctypes.c_int32),
        ("id_col", ctypes.c_int32),
        ("id_value", ctypes.c_int64),
    ]


OP_INT_I32, OP_INT_I64, OP_INT_U8 = 0, 1, 2
OP_PADDED_BAD_MASK, OP_PADDED_BAD_ID = 1, 2  # op_padded_report.status bits


class OpLossRequest(ctypes.Structure):
    """``op_loss_request``: the logits, labels and kind of one ``op_loss`` call."""

    _fields_ = [
        ("struct_bytes", ctypes.c_uint32),
        ("kind", ctypes.c_int32),
        ("logits_dev", ctypes.c_void_p),
        ("labels_dev", ctypes.c_void_p),
        ("labels_dtype", ctypes.c_int32),
        ("n_rows", ctypes.c_int32),
        ("width", ctypes.c_int32),
        ("channels", ctypes.c_int32),
        ("total_tokens", ctypes.c_int32),
        ("reserved", ctypes.c_int32),
        ("cu_seqlens_dev", ctypes.c_void_p),
        ("ignore_index", ctypes.c_int64),
        ("terms_dev", ctypes.c_void_p),
    ]


class OpLossReport(ctypes.Structure):
    """``op_loss_report``: what ``op_loss`` read back -- the first label out of range, the count, the fp64 sum, the loss."""

    _fields_ = [
        ("struct_bytes", ctypes.c_uint32),
        ("status", ctypes.c_int32),
        ("bad_row", ctypes.c_int32),
        ("bad_col", ctypes.c_int32),
        ("bad_value", ctypes.c_int64),
        ("count", ctypes.c_int64),
        ("sum", ctypes.c_double),
        ("loss", ctypes.c_float),
        ("reserved", ctypes.c_int32),
    ]


# enum op_loss_kind, by the names HipEncoder.loss takes
LOSS_KINDS = {"token_ce": 0, "rank_bce": 1, "rank_ce": 2, "rank_mse": 3}
OP_LOSS_TOKEN_CE, OP_LOSS_RANK_BCE, OP_LOSS_RANK_CE, OP_LOSS_RANK_MSE = 0, 1, 2, 3
OP_LABELS_F32 = 3  # op_loss_request.labels_dtype beside OP_INT_I32 / OP_INT_I64
OP_LOSS_BAD_LABEL = 1  # op_loss_report.status bit


class OpCoverageReport(ctypes.Structure):
    """``op_coverage_report``: what ``op_coverage_scan`` found in one packed batch."""

    _fields_ = [
        ("struct_bytes", ctypes.c_uint32),
        ("novel_tokens", ctypes.c_int32),
        ("longest_row_tokens", ctypes.c_int32),
        ("longest_row", ctypes.c_int32),
        ("max_audited_tokens", ctypes.c_int32),
    ]


class OpAssembleRequest(ctypes.Structure):
    """``op_assemble_request``: the resident corpus, a request's queries, the row template and the plan of one ``op_assemble_rows`` call."""

    _fields_ = [
        ("struct_bytes", ctypes.c_uint32),
        ("n_frag", ctypes.c_int32),
        ("n_queries", ctypes.c_int32),
        ("n_rows", ctypes.c_int32),
        ("total_tokens", ctypes.c_int32),
        ("n_prefix", ctypes.c_int32),
        ("n_middle", ctypes.c_int32),
        ("n_suffix", ctypes.c_int32),
        ("prefix", ctypes.c_void_p),
        ("middle", ctypes.c_void_p),
        ("suffix", ctypes.c_void_p),
        ("corpus_dev", ctypes.c_void_p),
        ("frag_off_dev", ctypes.c_void_p),
        ("frag_off_host", ctypes.c_void_p),
        ("query_ids_dev", ctypes.c_void_p),
        ("q_off_dev", ctypes.c_void_p),
        ("q_off_host", ctypes.c_void_p),
        ("plan_dev", ctypes.c_void_p),
        ("plan_host", ctypes.c_void_p),
        ("cu_seqlens_dev", ctypes.c_void_p),
        ("cu_seqlens_host", ctypes.c_void_p),
    ]


OP_ASSEMBLE_MAX_PIECE = 8


class OpPlannedMeansRequest(ctypes.Structure):
    """``op_planned_means_request``: the keep-probabilities of a forward, the corpus' shift table and where the rows' fragment
    means go (``op_planned_fragment_means``; the rows themselves are the forward's ``op_assemble_request``)."""

    _fields_ = [
        ("struct_bytes", ctypes.c_uint32),
        ("n_slots", ctypes.c_int32),
        ("keep_prob_dev", ctypes.c_void_p),
        ("frag_shift_dev", ctypes.c_void_p),
        ("slot_off_dev", ctypes.c_void_p),
        ("slot_off_host", ctypes.c_void_p),
        ("mean_out_dev", ctypes.c_void_p),
        ("slot_frag_out_dev", ctypes.c_void_p),
    ]


OP_DECISIONS_INSTANCE_WORDS = 6  # slot_begin, slot_end, sent_out_begin, n_sentences, item_sent_base, title_index


class OpDecisionsRequest(ctypes.Structure):
    """``op_decisions_request``: the (query, context) instances of a prepared request, the fragment means and the outputs of
    one ``op_sentence_decisions`` call."""

    _fields_ = [
        ("struct_bytes", ctypes.c_uint32),
        ("n_instances", ctypes.c_int32),
        ("n_slots", ctypes.c_int32),
        ("n_frag", ctypes.c_int32),
        ("n_out", ctypes.c_int32),
        ("threshold", ctypes.c_double),
        ("instances_dev", ctypes.c_void_p),
        ("instances_host", ctypes.c_void_p),
        ("mean_dev", ctypes.c_void_p),
        ("slot_frag_dev", ctypes.c_void_p),
        ("frag_sent_dev", ctypes.c_void_p),
        ("avg_out_dev", ctypes.c_void_p),
        ("keep_out_dev", ctypes.c_void_p),
    ]


class OpWorkspaceRegion(ctypes.Structure):
    """``op_workspace_region``: one region of the forward's workspace (``op_debug_workspace_layout``)."""

    _fields_ = [
        ("name", ctypes.c_char_p),
        ("offset", ctypes.c_uint64),
        ("bytes", ctypes.c_uint64),
        ("kind", ctypes.c_int32),
    ]


OP_WS_FLOAT, OP_WS_INDEX, OP_WS_FLAG = 0, 1, 2
WORKSPACE_KINDS = {OP_WS_FLOAT: "float", OP_WS_INDEX: "index", OP_WS_FLAG: "flag"}

# enum op_probe_kind (op_debug_primitive): name -> (kind, input dtype name, inputs per group, output dtype name, outputs per group)
PROBE_KINDS = {
    "BF16_SPLIT": (0, "float32", 4, "int32", 28),
    "F16_PAIR": (1, "float32", 4, "int32", 12),
    "F16_F8": (2, "float32", 4, "int32", 8),
    "E4M3_F16": (3, "int16", 4, "int32", 4),
    "E4M3_F32": (4, "float32", 4, "int32", 12),
    "GELU": (5, "float32", 1, "float32", 2),
    "EXP2": (6, "float32", 1, "float32", 2),
    "ROPE": (7, "float32", 4, "float32", 2),
    "KEEP_PROB": (8, "float32", 2, "float32", 1),
    "MFMA_SCALE": (9, "uint8", 2, "float32", 1024),
}

OP_CAL_FULL_REPORT = 1
OP_CAL_WHOLE_DEPTH = 2
OP_CAL_REFERENCE_F32 = 4  # op_calibrate compares with kernel set "fp32" (a handle created with OP_FLAG_F32_PACKS)


class OpProfileEntry(ctypes.Structure):
    _fields_ = [("kind", ctypes.c_int32), ("launches", ctypes.c_int32), ("total_ms", ctypes.c_double)]


def library_path() -> Path:
    override = os.environ.get("OPEN_PROVENCE_HIP_LIB")
    if override:
        return Path(override)
    return Path(__file__).resolve().parent / LIB_NAME


_LIB: ctypes.CDLL | None = None


def load_library() -> ctypes.CDLL:
    """Load (once) and type the shared library; raises :class:`HipLibraryError` when it is absent."""

    global _LIB
    if _LIB is not None:
        return _LIB
    path = library_path()
    if not path.exists():
        raise HipLibraryError(
            f"{path} not found. Build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(hipcc --offload-arch=gfx950). There is no CPU or PyTorch fallback for the forward path."
        )
    try:
        lib = ctypes.CDLL(str(path))
    except OSError as exc:
        raise HipLibraryError(f"failed to load {path}: {exc}") from exc

    vp, ci, cs = ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t
    lib.op_abi_version.restype = ci
    lib.op_abi_version.argtypes = []
    lib.op_create.restype = ci
    lib.op_create.argtypes = [ctypes.POINTER(OpConfig), ctypes.POINTER(vp)]
    lib.op_load_weight.restype = ci
    lib.op_load_weight.argtypes = [vp, ctypes.c_char_p, vp, ci, ctypes.POINTER(ctypes.c_int64), ci]
    lib.op_weights_ready.restype = ci
    lib.op_weights_ready.argtypes = [vp]
    lib.op_workspace_bytes.restype = cs
    lib.op_workspace_bytes.argtypes = [vp, ci, ci, ci]
    lib.op_forward_packed.restype = ci
    lib.op_forward_packed.argtypes = [vp, vp, vp, vp, ci, ci, ci, vp, vp, vp, vp, cs, vp]
    if hasattr(lib, "op_forward_packed_hidden"):
        lib.op_forward_packed_hidden.restype = ci
        lib.op_forward_packed_hidden.argtypes = [vp, vp, vp, vp, ci, ci, ci, vp, vp, vp, vp, cs, vp, ctypes.POINTER(OpHiddenRequest)]
    if hasattr(lib, "op_forward_packed_pooled"):  # (additive to ABI 10)
        lib.op_forward_packed_pooled.restype = ci
        lib.op_forward_packed_pooled.argtypes = [vp, vp, vp, vp, ci, ci, ci, vp, vp, vp, vp, cs, vp, ctypes.POINTER(OpHiddenRequest),
                                                 ctypes.POINTER(OpPoolRequest)]
    if hasattr(lib, "op_attention_rows"):  # (additive to ABI 10; the workspace is op_attention_workspace_bytes)
        lib.op_attention_rows.restype = ci
        lib.op_attention_rows.argtypes = [vp, vp, vp, ci, ci, ci, ctypes.POINTER(OpAttentionRowsRequest), vp, cs, vp]
    if hasattr(lib, "op_attention_probs"):  # (additive to ABI 10: an older library loaded for an A/B has neither)
        lib.op_attention_workspace_bytes.restype = cs
        lib.op_attention_workspace_bytes.argtypes = [vp, ci, ci, ci]
        lib.op_attention_probs.restype = ci
        lib.op_attention_probs.argtypes = [vp, vp, vp, ci, ci, ci, ctypes.POINTER(OpAttentionRequest), vp, cs, vp]
    lib.op_effective_policy.restype = ci
    lib.op_effective_policy.argtypes = [vp, ctypes.POINTER(ctypes.c_uint8), ctypes.POINTER(ci)]
    if hasattr(lib, "op_set_compact_operands"):  # (absent only in an older library loaded for a same-box A/B, see below)
        lib.op_set_compact_operands.restype = ci
        lib.op_set_compact_operands.argtypes = [vp, ci, ctypes.POINTER(ci)]
    if hasattr(lib, "op_select_kernel_set"):
        lib.op_select_kernel_set.restype = ci
        lib.op_select_kernel_set.argtypes = [vp, ci]
        if hasattr(lib, "op_mlp_correction_layers"):
            lib.op_mlp_correction_layers.restype = ci
            lib.op_mlp_correction_layers.argtypes = [vp, ctypes.POINTER(ctypes.c_uint64)]
            lib.op_select_mlp_correction_layers.restype = ci
            lib.op_select_mlp_correction_layers.argtypes = [vp, ctypes.c_uint64]
        lib.op_calibrate.restype = ci
        lib.op_calibrate.argtypes = [vp, ctypes.c_float, vp, vp, ci, ctypes.POINTER(OpCalibration)]
    if hasattr(lib, "op_pack_padded"):  # (additive to ABI 10: an older library loaded for an A/B has neither)
        lib.op_pack_padded.restype = ci
        lib.op_pack_padded.argtypes = [vp, vp, ci, vp, ci, ci, ci, vp, vp, vp, ctypes.POINTER(OpPaddedReport), vp]
        lib.op_unpack_padded.restype = ci
        lib.op_unpack_padded.argtypes = [vp, vp, vp, ci, ci, ci, vp, vp]
    if hasattr(lib, "op_forward_masked"):  # (additive to ABI 10; the workspace is the call's own)
        lib.op_masked_workspace_bytes.restype = cs
        lib.op_masked_workspace_bytes.argtypes = [vp, ci, ci]
        lib.op_forward_masked.restype = ci
        lib.op_forward_masked.argtypes = [vp, vp, vp, ci, ci, vp, cs, vp, vp, ctypes.POINTER(OpMaskedReport), vp]
    if hasattr(lib, "op_forward_masked_native"):  # (additive to ABI 10: op_forward_masked on the selected kernel set)
        lib.op_masked_native_workspace_bytes.restype = cs
        lib.op_masked_native_workspace_bytes.argtypes = [vp, ci, ci]
        lib.op_forward_masked_native.restype = ci
        lib.op_forward_masked_native.argtypes = [vp, vp, vp, ci, ci, vp, cs, vp, vp, ctypes.POINTER(OpMaskedReport), vp]
    if hasattr(lib, "op_loss"):  # (additive to ABI 10)
        lib.op_loss.restype = ci
        lib.op_loss.argtypes = [vp, ctypes.POINTER(OpLossRequest), vp, ctypes.POINTER(OpLossReport), vp]
    if hasattr(lib, "op_coverage_scan"):  # (the running audit's five calls, additive to ABI 10 like the two above)
        lib.op_coverage_scan.restype = ci
        lib.op_coverage_scan.argtypes = [vp, vp, vp, ci, ci, vp, ctypes.POINTER(OpCoverageReport), vp]
        lib.op_coverage_commit.restype = ci
        lib.op_coverage_commit.argtypes = [vp, vp, vp, ci, ci, vp, ci, vp]
        lib.op_coverage_reset.restype = ci
        lib.op_coverage_reset.argtypes = [vp]
        lib.op_gather_rows.restype = ci
        lib.op_gather_rows.argtypes = [vp, vp, vp, ci, ci, vp, ci, vp, vp, vp]
        lib.op_audit_compare.restype = ci
        lib.op_audit_compare.argtypes = [vp, vp, vp, vp, ci, ci, vp, ci, vp, vp, vp, vp, vp]
    if hasattr(lib, "op_debug_workspace_layout"):  # (test hook, additive to ABI 10)
        lib.op_debug_workspace_layout.restype = ci
        lib.op_debug_workspace_layout.argtypes = [vp, ci, ci, ci, ctypes.POINTER(OpWorkspaceRegion), ci]
    if hasattr(lib, "op_debug_rope_tables"):  # (test hook, additive to ABI 10)
        lib.op_debug_rope_tables.restype = ci
        lib.op_debug_rope_tables.argtypes = [vp, ci, ctypes.c_float, ci, vp, vp]
    if hasattr(lib, "op_debug_primitive"):  # (test hook, additive to ABI 10)
        lib.op_debug_primitive.restype = ci
        lib.op_debug_primitive.argtypes = [vp, ci, ci, vp, cs, vp, vp]
    if hasattr(lib, "op_assemble_rows"):  # (prepared contexts, additive to ABI 10)
        lib.op_assemble_rows.restype = ci
        lib.op_assemble_rows.argtypes = [vp, ctypes.POINTER(OpAssembleRequest), vp, vp]
    if hasattr(lib, "op_planned_fragment_means"):  # (prepared requests, additive to ABI 10)
        lib.op_planned_fragment_means.restype = ci
        lib.op_planned_fragment_means.argtypes = [vp, ctypes.POINTER(OpAssembleRequest), ctypes.POINTER(OpPlannedMeansRequest), vp]
    if hasattr(lib, "op_located_fragment_means"):
        lib.op_located_fragment_means.restype = ci
        lib.op_located_fragment_means.argtypes = [vp, ctypes.POINTER(OpAssembleRequest), ctypes.POINTER(OpPlannedMeansRequest), vp, vp, vp]
    if hasattr(lib, "op_sentence_decisions"):
        lib.op_sentence_decisions.restype = ci
        lib.op_sentence_decisions.argtypes = [vp, ctypes.POINTER(OpDecisionsRequest), vp]
    lib.op_segment_means.restype = ci
    lib.op_segment_means.argtypes = [vp, vp, ci, vp, ci, vp, vp]
    lib.op_debug_capture_hidden.restype = ci
    lib.op_debug_capture_hidden.argtypes = [vp, vp]
    lib.op_profile_enable.restype = ci
    lib.op_profile_enable.argtypes = [vp, ci]
    lib.op_profile_read.restype = ci
    lib.op_profile_read.argtypes = [vp, ctypes.POINTER(OpProfileEntry), ci]
    lib.op_profile_reset.restype = ci
    lib.op_profile_reset.argtypes = [vp]
    lib.op_profile_kind_name.restype = ctypes.c_char_p
    lib.op_profile_kind_name.argtypes = [ci]
    lib.op_debug_clock_probe.restype = ci
    lib.op_debug_clock_probe.argtypes = [vp, ci, vp, vp]
    lib.op_device_count.restype = ci
    lib.op_device_count.argtypes = [ctypes.POINTER(ci)]
    lib.op_destroy.restype = None
    lib.op_destroy.argtypes = [vp]
    lib.op_last_error.restype = ctypes.c_char_p
    lib.op_last_error.argtypes = [vp]

    version = lib.op_abi_version()
    # measurement hook: scripts/ab_lib.sh times an OLDER build of the library against the tree's (same box, alternating
    # runs); OPEN_PROVENCE_HIP_LIB_ANY_ABI=1 lets the explicitly named library through with its own version
    any_abi = os.environ.get("OPEN_PROVENCE_HIP_LIB") and os.environ.get("OPEN_PROVENCE_HIP_LIB_ANY_ABI") == "1"
    if version != OP_ABI_VERSION and not any_abi:
        raise HipLibraryError(f"{path} has ABI version {version}, the Python layer expects {OP_ABI_VERSION}; rebuild")
    _LIB = lib
    return lib


def last_error(lib: ctypes.CDLL, handle) -> str:
    raw = lib.op_last_error(handle)
    return raw.decode("utf-8", "replace") if raw else ""


def check(lib: ctypes.CDLL, handle, code: int, what: str) -> None:
    if code != OP_OK:
        raise HipLibraryError(f"{what} failed with code {code}: {last_error(lib, handle)}")
