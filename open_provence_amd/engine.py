"""``HipEncoder``: one handle of ``libopenprovence_hip.so`` bound to one GPU.

PyTorch-ROCm is used here for exactly three things -- owning device buffers (ids, outputs, workspace),
naming the current HIP stream, and reading checkpoint tensors -- never for arithmetic on the forward
path.  Everything numerical happens inside ``op_forward_packed`` (``include/open_provence_hip.h``).  How a calibrated kernel
set is re-checked on real batches -- the policy, its state and the one audit path -- is ``audit.py``; the encoder supplies the
device steps.
"""

from __future__ import annotations

import ctypes
import os
import warnings
from contextlib import contextmanager, nullcontext
from dataclasses import dataclass
from typing import Iterator, Mapping, NamedTuple, Sequence

import numpy as np
import torch

from . import _lib
from .audit import (DEFAULT_AUDIT_TOKENS, DEFAULT_CALIBRATION_TOLERANCE, MIN_AUDIT_TOKENS, AuditState, coverage_counts,  # noqa: F401
                    first_batch_audit, maybe_audit, resolve_audit_mode, select_audit_rows)
from .config import EncoderDims
from .packing import pack_rows

_PRECISIONS = {"bf16x3": _lib.OP_PRECISION_BF16X3, "bf16x2": _lib.OP_PRECISION_BF16X2, "bf16": _lib.OP_PRECISION_BF16}
# measurement / test switches, read ONCE when an encoder is created (the C ABI keeps no process-global state)
_ENV_FLAGS = {
    "OPEN_PROVENCE_FORCE_TILED": _lib.OP_FLAG_FORCE_TILED,
    "OPEN_PROVENCE_NO_SMALL_BLOCKS": _lib.OP_FLAG_NO_SMALL_BLOCKS,
    "OPEN_PROVENCE_NO_POLICY_KERNELS": _lib.OP_FLAG_NO_POLICY_KERNELS,
    "OPEN_PROVENCE_NO_LAYER_FUSION": _lib.OP_FLAG_NO_LAYER_FUSION,
    "OPEN_PROVENCE_LAYER_8X16": _lib.OP_FLAG_LAYER_8X16,
    "OPEN_PROVENCE_LAYER_M32": _lib.OP_FLAG_LAYER_M32,
    "OPEN_PROVENCE_NO_HEAD_FUSION": _lib.OP_FLAG_NO_HEAD_FUSION,
    "OPEN_PROVENCE_NO_F8": _lib.OP_FLAG_NO_F8,
    "OPEN_PROVENCE_ATTN_XCD_GROUP": _lib.OP_FLAG_ATTN_XCD_GROUP,
    "OPEN_PROVENCE_PANEL_F8": _lib.OP_FLAG_PANEL_F8,
    "OPEN_PROVENCE_PANEL_F8_WI": _lib.OP_FLAG_PANEL_F8_WI,
    "OPEN_PROVENCE_NO_LAYER_PAIRS": _lib.OP_FLAG_NO_LAYER_PAIRS,
}


@dataclass(frozen=True)
class HiddenRequest:
    """The hidden states one forward returns beside its logits (``op_forward_packed_hidden``).

    ``layers``: the entries 0 .. num_layers to write (entry 0 = embedding LayerNorm output, entry i = output of layer i-1, entry
    num_layers = the pruning head's input: the ``final_norm`` output, or the raw last layer under ``prune_pre_final_norm``);
    None = all of them.  ``dtype``: ``torch.float32`` or ``torch.bfloat16`` (the fp32 state rounded to nearest even).
    ``pad_width``: 0 = packed ``[n_sel, total_tokens, H]``; > 0 = padded ``[n_sel, n_seqs, pad_width, H]`` (zeros beyond each
    sequence's length; at least ``max_seqlen``).

    ``pool`` (``op_forward_packed_pooled``): None = the states themselves; ``"first"`` = the row of token 0 of each sequence (what
    ``classifier_pooling="cls"`` reads, bit-identical to that row of the full entry); ``"mean"`` = the mean over the sequence's
    tokens (fp64 in a fixed order, rounded once: the same bits whatever the batch around the sequence).  The result is then fp32
    ``[n_sel, n_seqs, H]`` -- a row of zeros for an empty sequence -- reduced on the device from ONE scratch entry, so ``dtype``
    must stay ``torch.float32`` and ``pad_width`` 0."""

    layers: "Sequence[int] | None" = None
    dtype: torch.dtype = torch.float32
    pad_width: int = 0
    pool: "str | None" = None

    def __post_init__(self) -> None:
        if self.pool is None:
            return
        if self.pool not in _lib.POOL_KINDS:
            raise ValueError(f"HiddenRequest.pool must be None, 'first' or 'mean', got {self.pool!r}")
        if self.dtype != torch.float32 or int(self.pad_width) != 0:
            raise ValueError("a pooled HiddenRequest is fp32 [n_sel, n_seqs, H]: dtype must be torch.float32 and pad_width 0")


@dataclass(frozen=True)
class AttentionRequest:
    """The attention probabilities one forward returns beside its logits (``op_attention_probs``, a side pass over the
    hidden states the forward hands out; the encoder must have been created with ``attention_outputs=True``).

    ``layers``: the layers 0 .. num_layers - 1 to return; None = all of them.  ``pad_width``: rows and columns of every
    ``[B, heads, pad_width, pad_width]`` fp32 tensor (zeros at masked keys, beyond each sequence's length and on padded query
    rows); 0 = ``max_seqlen``, otherwise at least that.

    ``query`` (``op_attention_rows``): None = the whole matrices; ``"first"`` = the row of query position 0 of each sequence; an
    integer tensor ``[n_seqs]`` = one query position per sequence (on the host or on the encoder's device; a position at or
    beyond a sequence's length gives a row of zeros, a negative one is refused where it is visible on the host).  Every tensor is
    then ``[B, heads, pad_width]``, bit-identical to that row of the whole matrix, or with ``reduce_heads=True`` ``[B, pad_width]``,
    the mean over heads (fp64 in head order, rounded once).  ``reduce_heads`` needs a ``query``."""

    layers: "Sequence[int] | None" = None
    pad_width: int = 0
    query: "str | torch.Tensor | None" = None
    reduce_heads: bool = False

    def __post_init__(self) -> None:
        query = self.query
        if isinstance(query, str):
            if query != "first":
                raise ValueError(f"AttentionRequest.query must be None, 'first' or an integer tensor [n_seqs], got {query!r}")
        elif query is not None:
            if not isinstance(query, torch.Tensor) or query.ndim != 1 or query.dtype not in (torch.int32, torch.int64):
                raise ValueError("AttentionRequest.query must be None, 'first' or an int32 / int64 tensor [n_seqs]")
            if query.device.type == "cpu" and query.numel() and int(query.min()) < 0:
                raise ValueError("AttentionRequest.query holds a negative position")
        if not isinstance(self.reduce_heads, (bool, int)) or int(self.reduce_heads) not in (0, 1):
            raise ValueError("AttentionRequest.reduce_heads must be a bool")
        if self.reduce_heads and query is None:
            raise ValueError("AttentionRequest.reduce_heads needs a query (the head mean of whole matrices is not offered)")


class PackedCall(NamedTuple):
    """What one ``op_forward_packed[_hidden]`` call needs: the batch, where its logits go, and what it runs with."""

    ids: torch.Tensor  # int32 [total] on the device
    cu_seqlens: torch.Tensor  # int32 [n_seqs + 1] on the device
    cu_host: np.ndarray  # the same, int32, on the host
    n_seqs: int
    total: int
    max_seqlen: int
    prune: torch.Tensor  # fp32 [total, 2]: written by the call
    rank: torch.Tensor  # fp32 [n_seqs, num_labels]: written by the call
    keep_prob: "torch.Tensor | None"
    ws: "torch.Tensor | None"  # uint8 workspace (None only for an empty batch, which is never launched)
    stream: int  # raw HIP stream
    hidden_req: "_lib.OpHiddenRequest | None" = None
    ids_host: "np.ndarray | None" = None
    rows: "torch.Tensor | None" = None  # of an audit's sub-batch: the rows it was gathered from (int32 on the device)
    # an audit's reference call: `ws` is checked against the kernel set selected WHEN THE CALL IS LAUNCHED and replaced if that set
    # needs more (op_workspace_bytes depends on the selection: kernel set "fp32" has fp32 planes of its own)
    size_ws_at_launch: bool = False
    pool_req: "_lib.OpPoolRequest | None" = None  # a pooled hidden request: op_forward_packed_pooled


def parse_precision(precision: "str | Mapping[str, int]") -> tuple[int, list[int]]:
    """``"bf16x3" | "bf16x2" | "bf16"`` or a per-family term-mask mapping / ``"wqkv=1,qk=3,..."`` string
    (families: ``_lib.OP_FAMILIES``; mask bit 0 = lo(activation) x hi, bit 1 = hi x lo(weight / key / value);
    families left out keep all terms) -> (enum op_precision, terms[8])."""

    terms = [3] * len(_lib.OP_FAMILIES) + [0] * (8 - len(_lib.OP_FAMILIES))
    if isinstance(precision, str) and precision in _PRECISIONS:
        return _PRECISIONS[precision], terms
    if isinstance(precision, str):
        try:
            mapping = {k.strip(): int(v) for k, v in (item.split("=") for item in precision.split(",") if item.strip())}
        except ValueError as exc:
            raise ValueError(f"precision must be one of {sorted(_PRECISIONS)} or 'family=mask,...': {precision!r}") from exc
    else:
        mapping = dict(precision)
    for name, mask in mapping.items():
        if name not in _lib.OP_FAMILIES:
            raise ValueError(f"unknown contraction family {name!r}; expected one of {_lib.OP_FAMILIES}")
        if int(mask) not in (0, 1, 2, 3):
            raise ValueError(f"term mask of {name!r} must be 0..3, got {mask!r}")
        terms[_lib.OP_FAMILIES.index(name)] = int(mask)
    return _lib.OP_PRECISION_CUSTOM, terms
_DTYPES = {torch.float32: _lib.OP_DTYPE_F32, torch.bfloat16: _lib.OP_DTYPE_BF16, torch.float16: _lib.OP_DTYPE_F16}

PATH_TOLERANCE = 1e-3  # BASELINE.json north_star: logits within 1e-3 of the fp32 CPU reference


def resolve_calibration_tolerance(calibrate: "bool | float | None") -> float:
    """``False`` / ``0`` -> 0.0 (no calibration); a float -> that tolerance; ``True`` / ``None`` -> ``OPEN_PROVENCE_CALIBRATE``
    (``0`` / ``off`` disables, a number is the tolerance) or :data:`DEFAULT_CALIBRATION_TOLERANCE`."""

    if isinstance(calibrate, (bool, np.bool_)):  # (by TYPE: `1` / `np.True_` are not `True` by identity)
        if not calibrate:
            return 0.0
        calibrate = None
    if calibrate is not None:
        tolerance = float(calibrate)
        if isinstance(calibrate, (int, np.integer)) and tolerance == 1.0:
            calibrate = None  # `calibrate=1` means "on", not a tolerance of 1.0 logit
        elif not tolerance < PATH_TOLERANCE:  # (also NaN)
            raise ValueError(f"calibration tolerance {calibrate!r} is not inside the path's own bar ({PATH_TOLERANCE:g} on a logit): "
                             "any candidate would pass; use kernel_set= to pin a set regardless of its error")
        else:
            return max(tolerance, 0.0)
    env = os.environ.get("OPEN_PROVENCE_CALIBRATE", "").strip().lower()
    if env in ("0", "off", "false", "no"):
        return 0.0
    if env and env not in ("1", "on", "true", "yes"):
        try:
            tolerance = max(float(env), 0.0)
            if not tolerance < PATH_TOLERANCE:
                raise ValueError
            return tolerance
        except ValueError as exc:
            raise ValueError(f"OPEN_PROVENCE_CALIBRATE must be 0 / off or a tolerance below {PATH_TOLERANCE:g}, got {env!r}") from exc
    return DEFAULT_CALIBRATION_TOLERANCE


CALIBRATION_REFERENCES = ("bf16x3", "fp32")


def check_arithmetic_arguments(kernel_set: "str | None", calibration_reference: "str | None") -> "tuple[str | None, str]":
    """Validate ``kernel_set=`` / ``calibration_reference=`` before anything touches the device: an unknown name is a
    ``ValueError``.  Returns them normalised (``"auto"`` -> ``None``; no reference given -> ``"bf16x3"``)."""

    if kernel_set is not None and kernel_set != "auto" and str(kernel_set) not in _lib.KERNEL_SET_IDS:
        raise ValueError(f"unknown kernel set {kernel_set!r}; expected one of {sorted(_lib.KERNEL_SET_IDS)} or 'auto'")
    reference = "bf16x3" if calibration_reference is None else str(calibration_reference)
    if reference not in CALIBRATION_REFERENCES:
        raise ValueError(f"unknown calibration_reference {calibration_reference!r}; expected one of {CALIBRATION_REFERENCES}")
    return (None if kernel_set in (None, "auto") else str(kernel_set)), reference


ATTENTION_MASKS = ("prefix", "any")


def check_attention_masks(attention_masks: "str | None") -> str:
    """Validate ``attention_masks=`` before anything touches the device: ``"prefix"`` (None: the default) or ``"any"``."""

    value = "prefix" if attention_masks is None else attention_masks
    if not isinstance(value, str) or value not in ATTENTION_MASKS:
        raise ValueError(f"unknown attention_masks {attention_masks!r}; expected one of {ATTENTION_MASKS}")
    return value


MASKED_KERNELS = ("fp32", "selected")


def check_masked_kernels(masked_kernels: "str | None") -> str:
    """Validate ``masked_kernels=`` before anything touches the device: ``"fp32"`` (None: the default) or ``"selected"``."""

    value = "fp32" if masked_kernels is None else masked_kernels
    if not isinstance(value, str) or value not in MASKED_KERNELS:
        raise ValueError(f"unknown masked_kernels {masked_kernels!r}; expected one of {MASKED_KERNELS}")
    return value


def check_masked_selected(dims: EncoderDims, flags: int, kernel_set: "str | None") -> None:
    """``attention_masks="any"`` with ``masked_kernels="selected"``: what ``op_forward_masked_native`` would refuse on every
    call is a ``ValueError`` at construction -- a handle pinned to kernel set "fp32" (whose masked forward is the fp32 one),
    and a shape on the tiled path (neither row nor panel path: the rule of ``op_plan.h``'s ``paths_of``)."""

    if kernel_set == "fp32":
        raise ValueError('masked_kernels="selected" with kernel_set="fp32": that set\'s masked forward is masked_kernels="fp32"')
    hidden, inter = int(dims.hidden_size), int(dims.intermediate_size)
    tiled = bool(flags & _lib.OP_FLAG_FORCE_TILED)
    row = hidden <= 256 and hidden % 64 == 0 and inter % 32 == 0 and not tiled
    panel = not row and hidden % 256 == 0 and inter % 128 == 0 and not tiled
    if not (row or panel):
        raise ValueError(
            f'masked_kernels="selected": hidden_size {hidden} / intermediate_size {inter}'
            + (" under OP_FLAG_FORCE_TILED" if tiled else "")
            + ' runs the tiled path, which has no key-mask attention kernel; use masked_kernels="fp32"')


def require_gpu(device: torch.device | str | int | None = None) -> torch.device:
    """Resolve a HIP device or fail loudly (the product has no CPU path)."""

    if not torch.cuda.is_available():
        raise _lib.HipLibraryError(
            "No HIP device visible to PyTorch-ROCm: the OpenProvence MI355X path runs only on a GPU "
            "(there is no CPU fallback; the CPU restatement under oracle/ is test infrastructure)."
        )
    if device is None:
        return torch.device("cuda", torch.cuda.current_device())
    dev = torch.device(device) if not isinstance(device, int) else torch.device("cuda", device)
    if dev.type != "cuda":
        raise _lib.HipLibraryError(f"device {dev} is not a HIP device")
    if dev.index is None:
        dev = torch.device("cuda", torch.cuda.current_device())
    return dev


class HipEncoder:
    """ModernBERT cross-encoder + pruning/ranking heads as hand-written gfx950 kernels."""

    def __init__(
        self,
        dims: EncoderDims,
        *,
        device: torch.device | str | int | None = None,
        precision: "str | Mapping[str, int]" = "bf16x3",
        chunk_rows: int | None = None,
        prune_pre_final_norm: bool = False,
        flags: int | None = None,
        audit: "str | bool | None" = None,
        audit_every: int = 0,
        audit_tokens: int = DEFAULT_AUDIT_TOKENS,
        kernel_set: "str | None" = None,
        calibration_reference: str = "bf16x3",
        attention_outputs: bool = False,
        attention_masks: str = "prefix",
        masked_kernels: str = "fp32",
    ) -> None:
        """``audit`` / ``audit_every`` / ``audit_tokens``: how a kernel set chosen by :meth:`calibrate` is re-checked on real
        batches -- ``"first"`` (default; ``None`` reads ``OPEN_PROVENCE_AUDIT``): once, on the first real batch
        (``audit.first_batch_audit``); ``"running"``: also later, see ``audit.maybe_audit``; ``"off"``: never.

        ``kernel_set``: the set :meth:`load_state_dict` pins when it is given none (``None``: ``OPEN_PROVENCE_KERNEL_SET`` or
        calibration).  ``"fp32"`` (here or in the environment) makes the handle keep the fp32 GEMM weights that set runs on.
        ``calibration_reference``: what :meth:`calibrate` compares with -- ``"bf16x3"`` (default: the (hi, lo) bf16 set) or
        ``"fp32"`` (kernel set "fp32"; keeps the fp32 weights too).
        ``attention_outputs``: keep the fp32 GEMM weights (4 bytes per weight element more on the device) so that
        :meth:`attention_probs` / ``forward_packed(attentions=...)`` can run; it changes nothing else.  ``kernel_set="fp32"``
        and ``calibration_reference="fp32"`` imply it.
        ``attention_masks``: ``"prefix"`` (default: right-padded masks only) or ``"any"`` -- :meth:`forward_masked` takes any
        ``[B, L]`` mask on the fp32 kernels; implies the fp32 weights, as ``attention_outputs=True`` does.
        ``masked_kernels`` (with ``attention_masks="any"`` only): ``"fp32"`` (default) or ``"selected"`` -- :meth:`forward_masked`
        runs on the kernel set the packed forward runs on (``op_forward_masked_native``; row and panel path) and the mask no longer
        asks for the fp32 weights.  A tiled-path shape or ``kernel_set="fp32"`` is a ``ValueError`` here."""

        self.kernel_set, self.calibration_reference = check_arithmetic_arguments(kernel_set, calibration_reference)
        self.attention_masks = check_attention_masks(attention_masks)
        self.masked_kernels = check_masked_kernels(masked_kernels)
        self.masked_native = self.attention_masks == "any" and self.masked_kernels == "selected"
        self.audit_mode = resolve_audit_mode(audit)
        self.audit_every = int(audit_every)
        self.audit_tokens = int(audit_tokens)
        if self.audit_every < 0 or self.audit_tokens < 1:
            raise ValueError("audit_every must be >= 0 and audit_tokens >= 1")
        precision_code, terms = parse_precision(precision)
        if flags is None:
            flags = 0
            for name, bit in _ENV_FLAGS.items():
                if os.environ.get(name):
                    flags |= bit
            waves = os.environ.get("OPEN_PROVENCE_ATT_WAVES")
            if waves:
                flags |= _lib.OP_FLAG_ATT_WAVES_4 if int(waves) == 4 else _lib.OP_FLAG_ATT_WAVES_8
        if self.masked_native:  # (before the device is touched)
            check_masked_selected(dims, int(flags), self.kernel_set or os.environ.get("OPEN_PROVENCE_KERNEL_SET"))
        self.lib = _lib.load_library()
        self.device = require_gpu(device)
        self.dims = dims
        self.precision = precision
        if dims.num_layers > _lib.OP_MAX_LAYERS:
            raise ValueError("too many layers")
        cfg = _lib.OpConfig()
        cfg.struct_bytes = ctypes.sizeof(_lib.OpConfig)
        cfg.device_id = int(self.device.index)
        cfg.vocab_size = dims.vocab_size
        cfg.hidden_size = dims.hidden_size
        cfg.intermediate_size = dims.intermediate_size
        cfg.num_layers = dims.num_layers
        cfg.num_heads = dims.num_heads
        cfg.num_labels = dims.num_labels
        cfg.local_attention = dims.local_attention
        cfg.max_position_embeddings = dims.max_position_embeddings
        cfg.pooling = _lib.OP_POOL_MEAN if dims.classifier_pooling == "mean" else _lib.OP_POOL_CLS
        cfg.precision = precision_code
        for i, mask in enumerate(terms):
            cfg.terms[i] = mask
        if "fp32" in (self.kernel_set, self.calibration_reference) or os.environ.get("OPEN_PROVENCE_KERNEL_SET") == "fp32":
            flags |= _lib.OP_FLAG_F32_PACKS
        if attention_outputs or (self.attention_masks == "any" and not self.masked_native):
            flags |= _lib.OP_FLAG_F32_PACKS
        self.attention_outputs = bool(flags & _lib.OP_FLAG_F32_PACKS)  # the fp32 weight packs op_attention_probs reads exist
        cfg.flags = int(flags)
        cfg.prune_pre_final_norm = 1 if prune_pre_final_norm else 0
        self.prune_pre_final_norm = bool(prune_pre_final_norm)
        cfg.norm_eps = dims.norm_eps
        cfg.global_rope_theta = dims.global_rope_theta
        cfg.local_rope_theta = dims.local_rope_theta
        cfg.chunk_rows = int(chunk_rows or 0)
        for i, flag in enumerate(dims.layer_is_global):
            cfg.layer_is_global[i] = 1 if flag else 0
        handle = ctypes.c_void_p()
        code = self.lib.op_create(ctypes.byref(cfg), ctypes.byref(handle))
        _lib.check(self.lib, None, code, "op_create")
        self._handle = handle
        self._split_state: dict | None = None  # the two pipeline streams + their workspaces (forward_packed_on)
        self._workspace: torch.Tensor | None = None
        self._attention_workspace: torch.Tensor | None = None  # op_attention_probs' own, reused across layers and calls
        self._masked_workspace: torch.Tensor | None = None  # op_forward_masked's / op_forward_masked_native's own
        self._audit_workspace: torch.Tensor | None = None  # of an audit's reference forward, when the batch's own is too small for it
        self._capture: torch.Tensor | None = None
        self._capture_result: torch.Tensor | None = None
        self.calibration: dict | None = None  # report of the last calibrate() (load_state_dict runs it by default)
        self.audit_state = AuditState(dims.vocab_size)
        self.audit_factor = 3.0  # an audit's bound, in calibration tolerances
        self.audit_collective = False  # under a process group the ranks audit TOGETHER (sharding.collective_audit)
        self.fallbacks = 0  # fp16 range-guard fallbacks: reported by process() (timing / performance_trace)
        self._f8_active: bool | None = None  # cache of f8_active(); None = ask the handle
        self._profiling = False
        self.last_loss_report: dict | None = None  # op_loss_report of the last loss(check=True) call

    # -- lifecycle -------------------------------------------------------------------------------
    def close(self) -> None:
        handle = getattr(self, "_handle", None)
        if handle is not None and handle.value:
            self.lib.op_destroy(handle)
            self._handle = ctypes.c_void_p()
        # (the two CU-masked streams of forward_packed_on stay alive for the life of the process: torch's caching allocator
        # keeps events on them for the outputs handed over with record_stream, and destroying a stream under it faults)
        self._split_state = None

    def __del__(self) -> None:  # pragma: no cover - interpreter shutdown order
        try:
            self.close()
        except Exception:
            pass

    # -- weights ---------------------------------------------------------------------------------
    def load_weight(self, name: str, tensor: torch.Tensor) -> None:
        t = tensor.detach()
        if t.dtype not in _DTYPES:
            t = t.to(torch.float32)
        t = t.contiguous()
        shape = (ctypes.c_int64 * max(t.ndim, 1))(*([int(s) for s in t.shape] or [1]))
        code = self.lib.op_load_weight(
            self._handle, name.encode("utf-8"), ctypes.c_void_p(t.data_ptr()), _DTYPES[t.dtype], shape, max(t.ndim, 1)
        )
        _lib.check(self.lib, self._handle, code, f"op_load_weight({name})")

    def load_state_dict(self, state: Mapping[str, torch.Tensor], *, calibrate: "bool | float | None" = None,
                        kernel_set: "str | None" = None, calibration_rows: "Sequence[Sequence[int]] | None" = None) -> None:
        """Checkpoint keys as in the reference's ``model.safetensors`` (``ranking_model.*`` /
        ``pruning_head.*``; legacy checkpoints without the prefix are accepted, standalone.py:1452-1464).
        Non-persistent buffers (``inv_freq``) and training-only tensors are skipped.

        Then the arithmetic is chosen FROM THE LOADED WEIGHTS (the reference decides its dtype and attention
        implementation at load time too, standalone.py:219-244, 1589-1615, 1631-1642): ``kernel_set`` (or
        ``OPEN_PROVENCE_KERNEL_SET``) pins a kernel set by name; otherwise :meth:`calibrate` runs with tolerance
        ``calibrate`` (a float; ``True`` / ``None`` = ``OPEN_PROVENCE_CALIBRATE`` or 1e-4; ``False`` / ``0`` = keep the
        default selection, which is safe for any weights and priced for the worst case)."""

        for name, tensor in state.items():
            if "inv_freq" in name or name.endswith("pooling_weights.weight") or name.endswith("pooling_weights.bias"):
                continue
            self.load_weight(name, tensor)
        _lib.check(self.lib, self._handle, self.lib.op_weights_ready(self._handle), "op_weights_ready")
        # A kernel set pinned or calibrated on the PREVIOUS checkpoint is not a property of this one: op_load_weight drops it
        # for every GEMM weight that changes (ABI 8); a state dict that reloads only norms / heads / embeddings keeps the
        # weights the set was measured on, but the measurement covered those tensors too -- back to the default selection.
        _lib.check(self.lib, self._handle, self.lib.op_select_kernel_set(self._handle, int(_lib.OP_KS_AUTO)), "op_select_kernel_set(auto)")
        self._f8_active = None
        self.audit_state.pending = False
        self._reset_coverage(running=False)
        self.calibration = None
        pinned = kernel_set or self.kernel_set or os.environ.get("OPEN_PROVENCE_KERNEL_SET")
        if pinned:
            self.select_kernel_set(pinned)
            return
        tolerance = resolve_calibration_tolerance(calibrate)
        if tolerance > 0.0 and hasattr(self.lib, "op_calibrate"):
            self.calibrate(tolerance, rows=calibration_rows)

    def select_kernel_set(self, name: "str | None") -> None:
        """Pin the kernel set by its :meth:`effective_policy` name (``None`` / ``"auto"``: the default selection).  A set with
        fewer product terms than the checkpoint carries is an approximation: :meth:`calibrate` is what measures one."""

        self._select_kernel_set(name)
        self.audit_state.pending = False  # (a pinned set is the caller's decision: nothing to audit)
        self._reset_coverage(running=False)

    def _select_kernel_set(self, name: "str | None") -> None:
        """``op_select_kernel_set`` alone: the audits' detour through the reference set leaves the audit state where it is."""

        number = _lib.OP_KS_AUTO if name in (None, "auto") else _lib.KERNEL_SET_IDS.get(str(name))
        if number is None:
            raise ValueError(f"unknown kernel set {name!r}; expected one of {sorted(_lib.KERNEL_SET_IDS)} or 'auto'")
        _lib.check(self.lib, self._handle, self.lib.op_select_kernel_set(self._handle, int(number)), f"op_select_kernel_set({name})")
        self._f8_active = None

    def _repin_calibrated(self, chosen: str) -> None:
        """Pin the calibrated set again after a detour through another one (the audits run the reference set in between):
        ``op_select_kernel_set`` means the whole depth, so the layer mask of sets 8 / 9 is pinned again behind it."""

        self._select_kernel_set(chosen)
        layers = (self.calibration or {}).get("mlp_correction_layers")
        if layers is not None and chosen in ("f16+mlp-f16-f8-w", "f16+mlp-f16-f8") and chosen == (self.calibration or {}).get("chosen_set"):
            mask = sum(1 << int(li) for li in layers)
            _lib.check(self.lib, self._handle, self.lib.op_select_mlp_correction_layers(self._handle, ctypes.c_uint64(mask)),
                       "op_select_mlp_correction_layers")

    def calibrate(self, tolerance: float = 1e-4, rows: "Sequence[Sequence[int]] | None" = None, *, full_report: "bool | None" = None,
                  whole_depth: "bool | None" = None) -> dict:
        """``op_calibrate``: one batch (``rows`` of token ids -- a sample of real inputs -- or the library's synthetic
        batch) through the (hi, lo) bf16 kernels and through every kernel set cheaper than the default one; the
        cheapest whose logits stay within ``tolerance`` of them (and finite) is what the forward runs on from now on.
        Returns (and keeps as ``self.calibration``) the report: ``{"tolerance", "reference_set", "default_set",
        "chosen_set", "candidates": {set name: max |logit difference|}, "rows", "tokens", "batch"}`` -- plus, when the choice is
        kernel set 8 / 9, ``"mlp_correction_layers"`` (the layers that keep the fp16 + e4m3 MLP) and ``"mlp_correction_err"``."""

        report = _lib.OpCalibration()
        report.struct_bytes = ctypes.sizeof(_lib.OpCalibration)
        # cheapest first, stop at the first candidate that holds (up to 11 fewer forwards at load on the deep models);
        # full_report=True / OPEN_PROVENCE_CALIBRATE_FULL=1 measures every candidate (scripts/calibration_probe.py)
        if full_report is None:
            full_report = os.environ.get("OPEN_PROVENCE_CALIBRATE_FULL", "").strip().lower() in ("1", "on", "true", "yes")
        report.flags = _lib.OP_CAL_FULL_REPORT if full_report else 0
        # kernel sets 8 / 9 are refined layer by layer (ABI 9); whole_depth=True / OPEN_PROVENCE_CALIBRATE_WHOLE_DEPTH=1 keeps them whole
        if whole_depth is None:
            whole_depth = os.environ.get("OPEN_PROVENCE_CALIBRATE_WHOLE_DEPTH", "").strip().lower() in ("1", "on", "true", "yes")
        if whole_depth:
            report.flags |= _lib.OP_CAL_WHOLE_DEPTH
        if self.calibration_reference == "fp32":
            report.flags |= _lib.OP_CAL_REFERENCE_F32
        if rows is not None:
            ids_np, cu_np, _ = pack_rows(rows)
            self.check_ids(ids_np)
            ids_np = np.ascontiguousarray(ids_np, dtype=np.int32)
            cu_np = np.ascontiguousarray(cu_np, dtype=np.int32)
            args = (ids_np.ctypes.data_as(ctypes.c_void_p), cu_np.ctypes.data_as(ctypes.c_void_p), int(cu_np.shape[0]) - 1)
        else:
            args = (None, None, 0)
        with torch.cuda.device(self.device):
            code = self.lib.op_calibrate(self._handle, ctypes.c_float(float(tolerance)), *args, ctypes.byref(report))
        _lib.check(self.lib, self._handle, code, "op_calibrate")
        names = _lib.KERNEL_SET_NAMES
        self._f8_active = None
        self.calibration = {
            "tolerance": float(report.tolerance),
            "reference_set": names.get(int(report.reference_set), str(report.reference_set)),
            "default_set": names.get(int(report.default_set), str(report.default_set)),
            "chosen_set": names.get(int(report.chosen_set), str(report.chosen_set)),
            "candidates": {names.get(int(report.candidate_set[i]), str(report.candidate_set[i])): float(report.candidate_err[i])
                           for i in range(int(report.n_candidates))},
            "default_err": float(report.default_err),
            "rows": int(report.n_rows),
            "tokens": int(report.n_tokens),
            "batch": "caller rows" if rows is not None else "synthetic (uniform token ids)",
        }
        # kernel sets 8 / 9 layer by layer (ABI 9): the layers that keep the fp16 + e4m3 MLP, the others run the "f16" set's
        if self.calibration["chosen_set"] in ("f16+mlp-f16-f8-w", "f16+mlp-f16-f8"):
            mask = int(report.mlp_layers)
            self.calibration["mlp_correction_layers"] = [li for li in range(self.dims.num_layers) if (mask >> li) & 1]
            self.calibration["mlp_correction_err"] = float(report.mlp_layers_err)
        # a set chosen on SYNTHETIC token ids is audited on the first real batch (audit.first_batch_audit); the caller's own rows
        # are real inputs already.  audit="off" / OPEN_PROVENCE_AUDIT=0 switches the audit off; audit="running" keeps auditing.
        mode = self.audit_mode
        cheaper = self.calibration["chosen_set"] != self.calibration["default_set"]
        self.audit_state.pending = rows is None and cheaper and mode != "off"
        self._reset_coverage(running=(mode == "running" and cheaper and self.calibration["reference_set"] in _lib.KERNEL_SET_IDS
                                      and self.calibration["reference_set"] != self.calibration["chosen_set"]
                                      and hasattr(self.lib, "op_coverage_scan")))
        return self.calibration

    def effective_policy(self) -> dict:
        """Term masks actually evaluated (the requested policy minus weight-lo terms that are identically zero
        for the loaded checkpoint) and the kernel set running them: ``{"terms": {family: mask}, "kernel_set":
        "bf16x3" | "bf16-weights" | "bf16" | "f16-f8" | "f16-f8-w" | "all-terms kernels, cleared lo operands"}`` ("f16-f8":
        the terms of "bf16-weights" with the whole-layer kernel's operands carried as fp16 hi + e4m3 lo; "f16-f8-w": the
        terms of "bf16x3" in that format, the weights' lo part as a third plane)."""

        terms = (ctypes.c_uint8 * 8)()
        kernel_set = ctypes.c_int(0)
        code = self.lib.op_effective_policy(self._handle, terms, ctypes.byref(kernel_set))
        _lib.check(self.lib, self._handle, code, "op_effective_policy")
        names = _lib.KERNEL_SET_NAMES
        policy = {
            "terms": {name: int(terms[i]) for i, name in enumerate(_lib.OP_FAMILIES)},
            "kernel_set": names.get(int(kernel_set.value), str(kernel_set.value)),
        }
        if policy["kernel_set"] in ("f16+mlp-f16-f8-w", "f16+mlp-f16-f8") and hasattr(self.lib, "op_mlp_correction_layers"):
            mask = ctypes.c_uint64(0)
            code = self.lib.op_mlp_correction_layers(self._handle, ctypes.byref(mask))
            _lib.check(self.lib, self._handle, code, "op_mlp_correction_layers")
            policy["mlp_correction_layers"] = [li for li in range(self.dims.num_layers) if (int(mask.value) >> li) & 1]
        return policy

    # -- the range guard of the fp16 + e4m3 kernel sets ---------------------------------------------
    def f8_active(self) -> bool:
        """True while the forward runs on kernel sets 3 / 4 (fp16 hi + e4m3 lo operands): their fp16 plane has fp16's
        range, and an MLP activation beyond it comes out as NaN by design (never clamped)."""

        if self._f8_active is None:
            self._f8_active = self.effective_policy()["kernel_set"] in _lib.FP16_PLANE_SETS
        return self._f8_active

    def fall_back_from_f8(self, reason: str = "") -> bool:
        """Switch this model to the (hi, lo) bf16 kernel sets for good (``op_set_compact_operands``: both weight packs are resident,
        nothing is re-loaded) and warn once.  Returns True when the kernel set changed, i.e. when repeating the forward
        can give a different answer.  The reference's own precedent for a silent, correct retry: its fallback from an
        unsupported dtype / attention implementation at load time (standalone.py:1631-1642)."""

        if not self.f8_active() or not hasattr(self.lib, "op_set_compact_operands"):
            return False
        changed = ctypes.c_int(0)
        code = self.lib.op_set_compact_operands(self._handle, 0, ctypes.byref(changed))
        _lib.check(self.lib, self._handle, code, "op_set_compact_operands")
        self._f8_active = None
        if changed.value:
            if self.calibration is not None:  # the report names what RUNS, not what was chosen before the fallback
                self.calibration["chosen_set"] = self.effective_policy()["kernel_set"]
                self.calibration["fallback"] = "fp16 range guard"
            self.audit_state.pending = False
            self._reset_coverage(running=False)
            self.fallbacks += 1
            warnings.warn(
                "open_provence_amd: a forward on the fp16 + e4m3 kernel set returned non-finite values"
                + (f" ({reason})" if reason else "")
                + ": an activation left fp16's range.  The batch is repeated on the (hi, lo) bf16 kernels (fp32 range) and "
                "this model stays on them (slower: 2-3 instead of 1.5-2 MFMA products per term); set OPEN_PROVENCE_NO_F8=1 "
                "to start there.",
                RuntimeWarning, stacklevel=3,
            )
        return bool(changed.value)

    def forward_packed_checked(self, ids, cu_seqlens, cu_seqlens_host, max_seqlen, keep_prob=None, hidden=None, ids_host=None,
                               attentions=None, pooled=None):
        """``forward_packed`` + the range guard: on kernel sets 3 / 4 the outputs are tested for NaN / Inf (one device
        reduction, one synchronisation) and a non-finite batch is repeated on the (hi, lo) bf16 sets.  On those sets
        nothing is tested: whatever comes out is what the reference's arithmetic gives.  With a ``hidden`` request the
        result is ``(prune, rank, hidden_states)``, the states of the forward whose logits are returned; with an
        ``attentions`` request its last element is the list of that forward's attention probabilities."""

        extra = {} if attentions is None else {"attentions": attentions}
        if pooled is not None:  # (a repeated batch repeats its pooled request as it repeats a full one)
            extra["pooled"] = pooled
        out = self.forward_packed(ids, cu_seqlens, cu_seqlens_host, max_seqlen, keep_prob=keep_prob, hidden=hidden, ids_host=ids_host, **extra)
        if self.f8_active():
            prune, rank = out[0], out[1]
            ok = torch.isfinite(rank).all() & torch.isfinite(prune).all()
            if not bool(ok.item()) and self.fall_back_from_f8("forward"):
                out = self.forward_packed(ids, cu_seqlens, cu_seqlens_host, max_seqlen, keep_prob=keep_prob, hidden=hidden, ids_host=ids_host, **extra)
        return out

    # -- forward ---------------------------------------------------------------------------------
    def _ensure_workspace(self, n_seqs: int, total_tokens: int, max_seqlen: int) -> torch.Tensor:
        need = int(self.lib.op_workspace_bytes(self._handle, n_seqs, total_tokens, max_seqlen))
        if need <= 0:
            raise _lib.HipLibraryError("op_workspace_bytes returned 0")
        ws = self._workspace
        if ws is None or ws.numel() < need:
            self._workspace = None
            ws = torch.empty(need + 256, dtype=torch.uint8, device=self.device)
            self._workspace = ws
        return ws

    def workspace_layout(self, n_seqs: int, total_tokens: int, max_seqlen: int) -> "list[dict]":
        """Test hook (``op_debug_workspace_layout``): the regions a forward of this geometry carves out of its workspace, in
        order, ``[{"name", "offset", "bytes", "kind": "float" | "index" | "flag"}]``; offsets from the 256-aligned base."""

        if not hasattr(self.lib, "op_debug_workspace_layout"):
            raise _lib.HipLibraryError("this library has no op_debug_workspace_layout")
        count = int(self.lib.op_debug_workspace_layout(self._handle, n_seqs, total_tokens, max_seqlen, None, 0))
        _lib.check(self.lib, self._handle, min(count, 0), "op_debug_workspace_layout")
        entries = (_lib.OpWorkspaceRegion * count)()
        assert int(self.lib.op_debug_workspace_layout(self._handle, n_seqs, total_tokens, max_seqlen, entries, count)) == count
        return [{"name": e.name.decode(), "offset": int(e.offset), "bytes": int(e.bytes), "kind": _lib.WORKSPACE_KINDS[int(e.kind)]}
                for e in entries]

    def rope_tables(self, global_table: bool) -> "tuple[torch.Tensor, torch.Tensor]":
        """Test hook (``op_debug_rope_tables``): this handle's cos / sin tables as they lie on the device, fp32
        ``[max_position_embeddings, 32]`` each on the CPU; ``global_table``: the full-attention layers' table."""

        if not hasattr(self.lib, "op_debug_rope_tables"):
            raise _lib.HipLibraryError("this library has no op_debug_rope_tables")
        n = int(self.dims.max_position_embeddings)
        cos, sin = torch.empty(n, 32, dtype=torch.float32), torch.empty(n, 32, dtype=torch.float32)
        code = self.lib.op_debug_rope_tables(self._handle, int(bool(global_table)), 0.0, n, ctypes.c_void_p(cos.data_ptr()),
                                             ctypes.c_void_p(sin.data_ptr()))
        _lib.check(self.lib, self._handle, int(code), "op_debug_rope_tables")
        return cos, sin

    def debug_primitive(self, kind: "str | int", mode: int, inputs: torch.Tensor) -> torch.Tensor:
        """Test hook (``op_debug_primitive``): the device functions of one ``_lib.PROBE_KINDS`` entry over ``inputs`` (a flat
        CPU or device tensor of the kind's input dtype) under conversion mode ``mode`` (0 overflowing, 1 saturating);
        returns the records on the CPU, ``[groups, outputs per group]`` in the kind's output dtype (words as int32)."""

        if not hasattr(self.lib, "op_debug_primitive"):
            raise _lib.HipLibraryError("this library has no op_debug_primitive")
        if isinstance(kind, str):
            number, in_dtype, group, out_dtype, out_per_group = _lib.PROBE_KINDS[kind]
        else:
            number, in_dtype, group, out_dtype, out_per_group = next(v for v in _lib.PROBE_KINDS.values() if v[0] == int(kind))
        if inputs.dtype != getattr(torch, in_dtype) or inputs.ndim != 1:
            raise TypeError(f"inputs must be a flat {in_dtype} tensor")
        src = inputs.to(self.device).contiguous()
        n = int(src.numel())
        out = torch.empty(n // group, out_per_group, dtype=getattr(torch, out_dtype), device=self.device)
        stream = torch.cuda.current_stream(self.device).cuda_stream
        code = self.lib.op_debug_primitive(self._handle, number, int(mode), ctypes.c_void_p(src.data_ptr() if n else 0), n,
                                           ctypes.c_void_p(out.data_ptr() if out.numel() else 0), ctypes.c_void_p(stream))
        _lib.check(self.lib, self._handle, int(code), "op_debug_primitive")
        return out.cpu()

    def segment_means(self, values: torch.Tensor, segments: torch.Tensor) -> torch.Tensor:
        """``values[T]`` fp32 and ``segments[S, 2]`` int32 (token ranges ``[start, end)``) on this device ->
        ``[S]`` fp32: ``values[start:end].mean()`` in numpy's float32 pairwise order, bit for bit; 1.0 for an empty
        range (the reference's per-fragment score, standalone.py:3075-3082).  Asynchronous on the current stream."""

        if values.dtype != torch.float32 or segments.dtype != torch.int32:
            raise TypeError("values must be fp32 and segments int32")
        if values.device != self.device or segments.device != self.device:
            raise ValueError(f"values / segments must live on {self.device}")
        if not values.is_contiguous() or not segments.is_contiguous() or segments.ndim != 2 or segments.shape[1] != 2:
            raise ValueError("values must be contiguous and segments a contiguous [S, 2] tensor")
        n_seg = int(segments.shape[0])
        out = torch.empty(n_seg, dtype=torch.float32, device=self.device)
        if n_seg == 0:
            return out
        with torch.cuda.device(self.device):
            stream = torch.cuda.current_stream(self.device).cuda_stream
            code = self.lib.op_segment_means(
                self._handle, ctypes.c_void_p(values.data_ptr()), int(values.numel()), ctypes.c_void_p(segments.data_ptr()),
                n_seg, ctypes.c_void_p(out.data_ptr()), ctypes.c_void_p(stream),
            )
        _lib.check(self.lib, self._handle, code, "op_segment_means")
        return out

    def assemble_rows(self, corpus: torch.Tensor, frag_off: torch.Tensor, frag_off_host: np.ndarray, query_ids: torch.Tensor,
                      q_off: torch.Tensor, q_off_host: np.ndarray, template: "Sequence[Sequence[int]]", plan: torch.Tensor,
                      plan_host: np.ndarray, cu_seqlens: torch.Tensor, cu_seqlens_host: np.ndarray,
                      out: "torch.Tensor | None" = None) -> torch.Tensor:
        """``op_assemble_rows``: the packed ``ids[T]`` of ``prefix + query + middle + context + suffix`` rows, laid out on
        this device from a resident corpus (``corpus`` int32: the fragments' ids end to end, ``frag_off`` their offsets),
        the request's queries (``query_ids`` / ``q_off``) and a plan ``[n_rows, 4]`` int32 of ``{query, first_frag, n_frag,
        clip}`` per row; ``template`` = the three pieces (at most 8 ids each).  The ``*_host`` numpy arrays are the host
        copies of the device tensors of the same name: the library checks the request on them (``cu_seqlens_host`` must be
        the prefix sums of the plan's row lengths) and refuses before it enqueues, so nothing is read back.  Asynchronous on
        the current stream; ``out`` (int32, at least T elements) or a new tensor."""

        if not hasattr(self.lib, "op_assemble_rows"):
            raise _lib.HipLibraryError("this library has no op_assemble_rows")
        req, _pieces, total = self._assemble_request(corpus, frag_off, frag_off_host, query_ids, q_off, q_off_host, template, plan, plan_host,
                                                     cu_seqlens, cu_seqlens_host)
        if out is None:
            out = torch.empty(max(total, 0), dtype=torch.int32, device=self.device)
        elif out.dtype != torch.int32 or out.device != self.device or not out.is_contiguous() or out.numel() < total:
            raise ValueError(f"out must be a contiguous int32 tensor of at least {total} elements on {self.device}")
        with torch.cuda.device(self.device):
            stream = torch.cuda.current_stream(self.device).cuda_stream
            code = self.lib.op_assemble_rows(self._handle, ctypes.byref(req), ctypes.c_void_p(out.data_ptr()) if out.numel() else None,
                                             ctypes.c_void_p(stream))
        _lib.check(self.lib, self._handle, code, "op_assemble_rows")
        return out[:total]

    def _assemble_request(self, corpus: "torch.Tensor | None", frag_off: torch.Tensor, frag_off_host: np.ndarray,
                          query_ids: "torch.Tensor | None", q_off: torch.Tensor, q_off_host: np.ndarray, template: "Sequence[Sequence[int]]",
                          plan: torch.Tensor, plan_host: np.ndarray, cu_seqlens: torch.Tensor,
                          cu_seqlens_host: np.ndarray) -> "tuple[_lib.OpAssembleRequest, list[np.ndarray], int]":
        """The ``op_assemble_request`` of :meth:`assemble_rows` and :meth:`planned_fragment_means` from their shared arguments,
        sizes and dtypes checked -> (the request, the template pieces it points into, total tokens).  ``corpus`` / ``query_ids``
        may be None where the call does not read the ids."""

        device_side = {"frag_off": frag_off, "q_off": q_off, "plan": plan, "cu_seqlens": cu_seqlens}
        if corpus is not None:
            device_side["corpus"] = corpus
        if query_ids is not None:
            device_side["query_ids"] = query_ids
        for name, tensor in device_side.items():
            if tensor.dtype != torch.int32 or tensor.device != self.device or not tensor.is_contiguous():
                raise ValueError(f"{name} must be a contiguous int32 tensor on {self.device}")
        hosts = []
        for name, array in (("frag_off_host", frag_off_host), ("q_off_host", q_off_host), ("plan_host", plan_host), ("cu_seqlens_host", cu_seqlens_host)):
            if not isinstance(array, np.ndarray) or array.dtype != np.int32 or not array.flags.c_contiguous:
                raise ValueError(f"{name} must be a C-contiguous int32 numpy array")
            hosts.append(array)
        n_rows = int(cu_seqlens_host.shape[0]) - 1
        if (n_rows < 0 or plan_host.size != 4 * n_rows or plan.numel() != 4 * n_rows or cu_seqlens.numel() != n_rows + 1
                or frag_off.numel() != frag_off_host.size or q_off.numel() != q_off_host.size or frag_off_host.size < 1 or q_off_host.size < 1):
            raise ValueError("plan / cu_seqlens / offsets: the host and device copies differ in size, or do not describe n_rows rows")
        if (corpus is not None and corpus.numel() < int(frag_off_host[-1])) or (query_ids is not None and query_ids.numel() < int(q_off_host[-1])):
            raise ValueError("corpus / query_ids are shorter than their offsets say")
        total = int(cu_seqlens_host[-1])
        pieces = [np.ascontiguousarray(np.asarray(piece, dtype=np.int32).reshape(-1)) for piece in template]
        if len(pieces) != 3:
            raise ValueError("template must be (prefix, middle, suffix)")
        req = _lib.OpAssembleRequest()
        req.struct_bytes = ctypes.sizeof(_lib.OpAssembleRequest)
        req.n_frag, req.n_queries, req.n_rows, req.total_tokens = int(frag_off_host.size) - 1, int(q_off_host.size) - 1, n_rows, total
        req.n_prefix, req.n_middle, req.n_suffix = (int(p.size) for p in pieces)
        req.prefix, req.middle, req.suffix = (p.ctypes.data if p.size else None for p in pieces)
        req.corpus_dev = corpus.data_ptr() if corpus is not None and corpus.numel() else None
        req.frag_off_dev, req.frag_off_host = frag_off.data_ptr(), frag_off_host.ctypes.data
        req.query_ids_dev = query_ids.data_ptr() if query_ids is not None and query_ids.numel() else None
        req.q_off_dev, req.q_off_host = q_off.data_ptr(), q_off_host.ctypes.data
        req.plan_dev, req.plan_host = (plan.data_ptr(), plan_host.ctypes.data) if n_rows else (None, None)
        req.cu_seqlens_dev, req.cu_seqlens_host = cu_seqlens.data_ptr(), cu_seqlens_host.ctypes.data
        return req, pieces, total

    def planned_fragment_means(self, frag_off: torch.Tensor, frag_off_host: np.ndarray, q_off: torch.Tensor, q_off_host: np.ndarray,
                               template: "Sequence[Sequence[int]]", plan: torch.Tensor, plan_host: np.ndarray, cu_seqlens: torch.Tensor,
                               cu_seqlens_host: np.ndarray, keep_prob: torch.Tensor, frag_shift: torch.Tensor, slot_off: torch.Tensor,
                               slot_off_host: np.ndarray, mean_out: torch.Tensor, slot_frag_out: torch.Tensor) -> None:
        """``op_planned_fragment_means``: for the rows :meth:`assemble_rows` laid out from the same ``plan`` (same arguments,
        without the ids), the mean of ``keep_prob`` (fp32, the forward's keep-probabilities) over every fragment's token range
        -- derived on the device from the plan, shifted left by ``frag_shift[f]`` (int32, per fragment of the corpus) and
        clamped to the row; numpy's float32 pairwise order bit for bit, 1.0 for an empty range -- into ``mean_out[slot]``
        (fp32), and the fragment's number into ``slot_frag_out[slot]`` (int32), ``slot = slot_off[row] + j``.  ``slot_off`` /
        ``slot_off_host`` (int32 ``[n_rows + 1]``) are the prefix sums of the rows' ``n_frag`` from any start inside the
        outputs.  The library checks the request on the host copies and refuses before it enqueues.  Asynchronous on the
        current stream."""

        if not hasattr(self.lib, "op_planned_fragment_means"):
            raise _lib.HipLibraryError("this library has no op_planned_fragment_means")
        rows, _pieces, req = self._planned_means_request(frag_off, frag_off_host, q_off, q_off_host, template, plan, plan_host, cu_seqlens,
                                                         cu_seqlens_host, keep_prob, frag_shift, slot_off, slot_off_host, mean_out, slot_frag_out)
        with torch.cuda.device(self.device):
            stream = torch.cuda.current_stream(self.device).cuda_stream
            code = self.lib.op_planned_fragment_means(self._handle, ctypes.byref(rows), ctypes.byref(req), ctypes.c_void_p(stream))
        _lib.check(self.lib, self._handle, code, "op_planned_fragment_means")

    def located_fragment_means(self, frag_off: torch.Tensor, frag_off_host: np.ndarray, q_off: torch.Tensor, q_off_host: np.ndarray,
                               template: "Sequence[Sequence[int]]", plan: torch.Tensor, plan_host: np.ndarray, cu_seqlens: torch.Tensor,
                               cu_seqlens_host: np.ndarray, keep_prob: torch.Tensor, frag_shift: torch.Tensor, slot_off: torch.Tensor,
                               slot_off_host: np.ndarray, mean_out: torch.Tensor, slot_frag_out: torch.Tensor, ids: torch.Tensor,
                               ctx_start_out: torch.Tensor) -> None:
        """``op_located_fragment_means``: :meth:`planned_fragment_means` (same arguments) with every row's context looked up in
        the row first, as the reference looks it up: ``ids`` (int32, at least the rows' tokens) is what :meth:`assemble_rows`
        laid out from the same ``plan``; ``ctx_start_out`` (int32 ``[n_rows]``) receives, per row, the first place at or left
        of ``len(prefix) + len(query) + len(middle)`` where the row's whole context occurs, and the fragments' ranges start
        there.  Asynchronous on the current stream."""

        if not hasattr(self.lib, "op_located_fragment_means"):
            raise _lib.HipLibraryError("this library has no op_located_fragment_means")
        rows, _pieces, req = self._planned_means_request(frag_off, frag_off_host, q_off, q_off_host, template, plan, plan_host, cu_seqlens,
                                                         cu_seqlens_host, keep_prob, frag_shift, slot_off, slot_off_host, mean_out, slot_frag_out)
        for name, tensor in (("ids", ids), ("ctx_start_out", ctx_start_out)):
            if tensor.dtype != torch.int32 or tensor.device != self.device or not tensor.is_contiguous():
                raise ValueError(f"{name} must be a contiguous {torch.int32} tensor on {self.device}")
        if ids.numel() < int(rows.total_tokens) or ctx_start_out.numel() != int(rows.n_rows):
            raise ValueError("ids / ctx_start_out: sizes do not fit the rows")
        with torch.cuda.device(self.device):
            stream = torch.cuda.current_stream(self.device).cuda_stream
            code = self.lib.op_located_fragment_means(
                self._handle, ctypes.byref(rows), ctypes.byref(req), ctypes.c_void_p(ids.data_ptr()) if ids.numel() else None,
                ctypes.c_void_p(ctx_start_out.data_ptr()) if ctx_start_out.numel() else None, ctypes.c_void_p(stream))
        _lib.check(self.lib, self._handle, code, "op_located_fragment_means")

    def _planned_means_request(self, frag_off, frag_off_host, q_off, q_off_host, template, plan, plan_host, cu_seqlens, cu_seqlens_host,
                               keep_prob, frag_shift, slot_off, slot_off_host, mean_out,
                               slot_frag_out) -> "tuple[_lib.OpAssembleRequest, list[np.ndarray], _lib.OpPlannedMeansRequest]":
        """The two requests of :meth:`planned_fragment_means` and :meth:`located_fragment_means` from their shared arguments,
        dtypes, devices and sizes checked -> (rows, the template pieces it points into, the means request)."""

        rows, pieces, total = self._assemble_request(None, frag_off, frag_off_host, None, q_off, q_off_host, template, plan, plan_host,
                                                     cu_seqlens, cu_seqlens_host)
        n_rows = int(rows.n_rows)
        for name, tensor, dtype in (("keep_prob", keep_prob, torch.float32), ("frag_shift", frag_shift, torch.int32), ("slot_off", slot_off, torch.int32),
                                    ("mean_out", mean_out, torch.float32), ("slot_frag_out", slot_frag_out, torch.int32)):
            if tensor.dtype != dtype or tensor.device != self.device or not tensor.is_contiguous():
                raise ValueError(f"{name} must be a contiguous {dtype} tensor on {self.device}")
        if not isinstance(slot_off_host, np.ndarray) or slot_off_host.dtype != np.int32 or not slot_off_host.flags.c_contiguous:
            raise ValueError("slot_off_host must be a C-contiguous int32 numpy array")
        if (slot_off_host.size != n_rows + 1 or slot_off.numel() != n_rows + 1 or keep_prob.numel() < total
                or frag_shift.numel() != int(frag_off_host.size) - 1 or slot_frag_out.numel() != mean_out.numel()):
            raise ValueError("keep_prob / frag_shift / slot_off / outputs: sizes do not fit the rows, the corpus or each other")
        req = _lib.OpPlannedMeansRequest()
        req.struct_bytes = ctypes.sizeof(_lib.OpPlannedMeansRequest)
        req.n_slots = int(mean_out.numel())
        req.keep_prob_dev = keep_prob.data_ptr() if keep_prob.numel() else None
        req.frag_shift_dev = frag_shift.data_ptr() if frag_shift.numel() else None
        req.slot_off_dev, req.slot_off_host = slot_off.data_ptr(), slot_off_host.ctypes.data
        req.mean_out_dev = mean_out.data_ptr() if mean_out.numel() else None
        req.slot_frag_out_dev = slot_frag_out.data_ptr() if slot_frag_out.numel() else None
        return rows, pieces, req

    def sentence_decisions(self, instances: torch.Tensor, instances_host: np.ndarray, means: torch.Tensor, slot_frag: torch.Tensor,
                           frag_sent: torch.Tensor, threshold: float, avg_out: "torch.Tensor | None" = None,
                           keep_out: "torch.Tensor | None" = None) -> "tuple[torch.Tensor, torch.Tensor]":
        """``op_sentence_decisions``: per (query, context) instance ``{slot_begin, slot_end, sent_out_begin, n_sentences,
        item_sent_base, title_index}`` (``instances`` int32 ``[n, 6]`` and its host copy) the sentences' averages over the
        fragment means in ``means[slot]`` (fp32; ``slot_frag[slot]`` names the fragment, ``frag_sent[f]`` its corpus-wide
        sentence) -- fp64, numpy's pairwise order, Python's ``max(0.0, min(avg, 1.0))`` -- and ``avg > threshold`` with the
        title rule -> ``(avg[n_out] fp64, keep[n_out] uint8)`` on this device, ``n_out`` = the instances' sentences, which tile
        the outputs in order.  Asynchronous on the current stream; ``avg_out`` / ``keep_out`` or new tensors."""

        if not hasattr(self.lib, "op_sentence_decisions"):
            raise _lib.HipLibraryError("this library has no op_sentence_decisions")
        for name, tensor, dtype in (("instances", instances, torch.int32), ("means", means, torch.float32), ("slot_frag", slot_frag, torch.int32),
                                    ("frag_sent", frag_sent, torch.int32)):
            if tensor.dtype != dtype or tensor.device != self.device or not tensor.is_contiguous():
                raise ValueError(f"{name} must be a contiguous {dtype} tensor on {self.device}")
        words = _lib.OP_DECISIONS_INSTANCE_WORDS
        if (not isinstance(instances_host, np.ndarray) or instances_host.dtype != np.int32 or not instances_host.flags.c_contiguous
                or instances_host.size % words or instances.numel() != instances_host.size):
            raise ValueError(f"instances_host must be a C-contiguous int32 numpy array of {words} words per instance, as large as instances")
        if slot_frag.numel() != means.numel():
            raise ValueError("means and slot_frag differ in size")
        table = instances_host.reshape(-1, words)
        n_out = int(table[:, 3].sum()) if table.shape[0] else 0
        if avg_out is None:
            avg_out = torch.empty(n_out, dtype=torch.float64, device=self.device)
        if keep_out is None:
            keep_out = torch.empty(n_out, dtype=torch.uint8, device=self.device)
        for name, tensor, dtype in (("avg_out", avg_out, torch.float64), ("keep_out", keep_out, torch.uint8)):
            if tensor.dtype != dtype or tensor.device != self.device or not tensor.is_contiguous() or tensor.numel() != n_out:
                raise ValueError(f"{name} must be a contiguous {dtype} tensor of {n_out} elements on {self.device}")
        req = _lib.OpDecisionsRequest()
        req.struct_bytes = ctypes.sizeof(_lib.OpDecisionsRequest)
        req.n_instances, req.n_slots, req.n_frag, req.n_out = int(table.shape[0]), int(means.numel()), int(frag_sent.numel()), n_out
        req.threshold = float(threshold)
        req.instances_dev, req.instances_host = (instances.data_ptr(), instances_host.ctypes.data) if table.shape[0] else (None, None)
        req.mean_dev = means.data_ptr() if means.numel() else None
        req.slot_frag_dev = slot_frag.data_ptr() if slot_frag.numel() else None
        req.frag_sent_dev = frag_sent.data_ptr() if frag_sent.numel() else None
        req.avg_out_dev = avg_out.data_ptr() if n_out else None
        req.keep_out_dev = keep_out.data_ptr() if n_out else None
        with torch.cuda.device(self.device):
            stream = torch.cuda.current_stream(self.device).cuda_stream
            code = self.lib.op_sentence_decisions(self._handle, ctypes.byref(req), ctypes.c_void_p(stream))
        _lib.check(self.lib, self._handle, code, "op_sentence_decisions")
        return avg_out, keep_out

    def forward_packed(
        self,
        ids: torch.Tensor,
        cu_seqlens: torch.Tensor,
        cu_seqlens_host: np.ndarray,
        max_seqlen: int,
        keep_prob: torch.Tensor | None = None,
        hidden: "HiddenRequest | None" = None,
        ids_host: "np.ndarray | None" = None,
        attentions: "AttentionRequest | None" = None,
        pooled: "HiddenRequest | None" = None,
    ) -> tuple[torch.Tensor, ...]:
        """``ids[T]`` / ``cu_seqlens[B+1]`` int32 on this device -> (prune_logits[T, 2], rank_logits[B, nl]) fp32.
        ``keep_prob`` (optional, fp32 ``[T]`` on this device) additionally receives
        ``softmax(prune_logits, -1)[:, 1]``, evaluated in the head kernel.  ``hidden`` (a :class:`HiddenRequest`): the
        result is ``(prune, rank, hidden_states)``, the selected entries written by the same kernels in one device buffer
        (packed ``[n_sel, T, H]`` or padded ``[n_sel, B, pad_width, H]``, zeros at padding); the logits are bit-identical
        to those of the same forward without the request.  ``ids_host`` (optional): the host copy of ``ids`` the caller
        already holds (what it handed to :meth:`check_ids`); the running audit decides coverage on it without touching the
        device (``audit.maybe_audit``).  ``attentions`` (an :class:`AttentionRequest`; the encoder needs
        ``attention_outputs=True``): the result tuple gains, as its LAST element, the list of the requested layers' attention
        probabilities ``[B, heads, W, W]`` fp32.  The forward then runs with a packed fp32 hidden request for those layers'
        inputs (merged with the caller's ``hidden`` request, whose states are laid out from the merged ones) and
        ``op_attention_probs`` runs once per layer behind it on the same stream; logits and hidden states are bit-identical to
        those of the same call without the request.  With ``AttentionRequest(query=...)`` the list holds one query row per
        sequence, ``[B, heads, W]`` or ``[B, W]`` (``op_attention_rows``).

        A ``hidden`` request with ``pool`` set returns ``[n_sel, B, H]`` in the place of the states.  ``pooled`` (a
        :class:`HiddenRequest` with ``pool`` set) is a pooled request that rides on the same call BESIDE an ordinary ``hidden``
        request: the result is then ``(prune, rank, hidden_states, pooled_states[, attentions])``.

        Asynchronous on the current torch stream of ``self.device`` (a forward that is audited synchronises it once)."""

        if self._capture is not None and ids.numel():
            self._capture = torch.zeros(
                (self.dims.num_layers + 1, int(ids.numel()), self.dims.hidden_size), dtype=torch.float32, device=self.device
            )
            capture_ptr = ctypes.c_void_p(self._capture.data_ptr())
            _lib.check(self.lib, self._handle, self.lib.op_debug_capture_hidden(self._handle, capture_ptr), "capture")
        if hidden is not None and isinstance(hidden, HiddenRequest) and hidden.pool is not None:
            if pooled is not None:
                raise ValueError("two pooled requests: pass the ordinary request as hidden= and the pooled one as pooled=")
            hidden, pooled = None, hidden
        if pooled is not None and (not isinstance(pooled, HiddenRequest) or pooled.pool is None):
            raise ValueError("pooled must be a HiddenRequest with pool='first' or pool='mean'")
        if attentions is not None:
            return self._forward_with_attentions(ids, cu_seqlens, cu_seqlens_host, max_seqlen, keep_prob, hidden, ids_host, attentions, pooled)
        call, states, pooled_states = self._forward(None, ids, cu_seqlens, cu_seqlens_host, max_seqlen, keep_prob, hidden, ids_host,
                                                    pooled=pooled)
        return (call.prune, call.rank) + tuple(t for t in (states, pooled_states) if t is not None)

    # -- attention probabilities: a side pass over the hidden states the forward hands out ---------------------------------------
    def _require_attention_outputs(self) -> None:
        if not self.attention_outputs:
            raise ValueError("attention probabilities need the fp32 weight packs: create the encoder / model with attention_outputs=True")
        if not hasattr(self.lib, "op_attention_probs"):
            raise _lib.HipLibraryError("this library has no op_attention_probs")

    def _forward_with_attentions(self, ids, cu_seqlens, cu_seqlens_host, max_seqlen, keep_prob, hidden, ids_host, attentions, pooled=None):
        """One forward with the merged hidden request, then ``op_attention_probs`` (``attentions.query``: ``op_attention_rows``) per
        requested layer."""

        if not isinstance(attentions, AttentionRequest):
            raise TypeError("attentions must be an AttentionRequest")
        self._require_attention_outputs()
        n_layers = self.dims.num_layers
        layers = list(range(n_layers)) if attentions.layers is None else [int(i) for i in attentions.layers]
        if any(i < 0 or i >= n_layers for i in layers):
            raise ValueError(f"attentions.layers must lie in 0 .. {n_layers - 1}")
        max_seqlen = int(max_seqlen)
        width = int(attentions.pad_width) or max_seqlen
        if width < max_seqlen:
            raise ValueError(f"attentions.pad_width must be 0 (= max_seqlen) or at least max_seqlen ({max_seqlen}), got {width}")
        # the caller's own request is validated as it would be alone (its tensors are not needed: the merged request's are)
        own = None
        if hidden is not None:
            own = sorted(set(range(n_layers + 1) if hidden.layers is None else (int(i) for i in hidden.layers)))
            self._hidden_request(hidden, 0, 0, max_seqlen)
        # hidden_states[i] is the input of layer i: one packed fp32 request for every entry either side needs
        merged = sorted(set(layers) | set(own or ()))
        call, states, pooled_states = self._forward(None, ids, cu_seqlens, cu_seqlens_host, max_seqlen, keep_prob,
                                                    HiddenRequest(layers=merged, dtype=torch.float32, pad_width=0), ids_host, pooled=pooled)
        slot = {entry: k for k, entry in enumerate(merged)}
        if attentions.query is None:
            probs = [self.attention_probs(states[slot[i]], i, cu_seqlens, call.cu_host, max_seqlen, width) for i in layers]
        else:
            query = None if isinstance(attentions.query, str) else attentions.query
            probs = [self.attention_rows(states[slot[i]], i, cu_seqlens, call.cu_host, max_seqlen, width, query=query,
                                         reduce_heads=bool(attentions.reduce_heads)) for i in layers]
        tail = (probs,) if pooled_states is None else (pooled_states, probs)
        if own is None:
            return (call.prune, call.rank) + tail
        mine = states if own == merged else states[[slot[i] for i in own]]
        if hidden.pad_width > 0:  # (the layout the kernels give a padded request: zeros beyond each sequence's length)
            from .packing import unpack_to_padded

            mine = torch.stack([unpack_to_padded(entry, call.cu_host, int(hidden.pad_width)) for entry in mine]) if len(own) else \
                mine.new_zeros((0, call.n_seqs, int(hidden.pad_width), self.dims.hidden_size))
        return (call.prune, call.rank, mine.to(hidden.dtype)) + tail

    def attention_probs(self, hidden_packed: torch.Tensor, layer: int, cu_seqlens: torch.Tensor, cu_seqlens_host: np.ndarray,
                        max_seqlen: int, pad_width: int = 0) -> torch.Tensor:
        """``hidden_packed[T, H]`` fp32 on this device = ``hidden_states[layer]``, the INPUT of that layer (entry ``layer`` of a
        packed fp32 :class:`HiddenRequest`) -> its attention probabilities ``[B, heads, W, W]`` fp32, ``W = pad_width`` (0:
        ``max_seqlen``): ``out[s, h, i, j]`` = what query token ``i`` of sequence ``s`` puts on key ``j``; exactly 0 at masked
        keys, beyond the sequence's length and on padded query rows (every element is written by the call).  fp32 arithmetic
        of kernel set "fp32" whatever set the forward runs on.  Asynchronous on the current torch stream."""

        self._require_attention_outputs()
        H, max_seqlen = self.dims.hidden_size, int(max_seqlen)
        if (hidden_packed.dtype != torch.float32 or hidden_packed.device != self.device or hidden_packed.ndim != 2
                or hidden_packed.shape[1] != H or not hidden_packed.is_contiguous()):
            raise ValueError(f"hidden_packed must be a contiguous fp32 [total_tokens, {H}] tensor on {self.device}")
        if cu_seqlens.dtype != torch.int32 or cu_seqlens.device != self.device:
            raise ValueError(f"cu_seqlens must be int32 on {self.device}")
        if not 0 <= int(layer) < self.dims.num_layers:
            raise ValueError(f"layer must lie in 0 .. {self.dims.num_layers - 1}")
        total, n_seqs = int(hidden_packed.shape[0]), int(cu_seqlens.numel()) - 1
        width = int(pad_width) or max_seqlen
        if width < max_seqlen:
            raise ValueError(f"pad_width must be 0 (= max_seqlen) or at least max_seqlen ({max_seqlen}), got {width}")
        cu_host = np.ascontiguousarray(cu_seqlens_host, dtype=np.int32)
        if cu_host.shape[0] != n_seqs + 1:
            raise ValueError("cu_seqlens_host length mismatch")
        vp = ctypes.c_void_p
        with torch.cuda.device(self.device):
            out = torch.empty((n_seqs, self.dims.num_heads, width, width), dtype=torch.float32, device=self.device)
            if out.numel() == 0:
                return out
            need = int(self.lib.op_attention_workspace_bytes(self._handle, n_seqs, total, max_seqlen)) + 256
            ws = self._attention_workspace
            if ws is None or ws.numel() < need:
                ws = self._attention_workspace = torch.empty(need, dtype=torch.uint8, device=self.device)
            base = ws.data_ptr()
            aligned = (base + 255) // 256 * 256
            req = _lib.OpAttentionRequest()
            req.struct_bytes = ctypes.sizeof(_lib.OpAttentionRequest)
            req.layer = int(layer)
            req.dtype = _lib.OP_HIDDEN_F32
            req.pad_width = width
            req.hidden_dev = vp(hidden_packed.data_ptr()) if total else None
            req.out_dev = vp(out.data_ptr())
            code = self.lib.op_attention_probs(
                self._handle, vp(cu_seqlens.data_ptr()), cu_host.ctypes.data_as(vp), n_seqs, total, max_seqlen, ctypes.byref(req),
                vp(aligned), ctypes.c_size_t(ws.numel() - (aligned - base)), vp(torch.cuda.current_stream(self.device).cuda_stream),
            )
        _lib.check(self.lib, self._handle, code, "op_attention_probs")
        return out

    def attention_rows(self, hidden_packed: torch.Tensor, layer: int, cu_seqlens: torch.Tensor, cu_seqlens_host: np.ndarray,
                       max_seqlen: int, pad_width: int = 0, query: "torch.Tensor | None" = None, reduce_heads: bool = False) -> torch.Tensor:
        """One query row per sequence of :meth:`attention_probs`' matrices, without the matrices (``op_attention_rows``; the same
        inputs, arithmetic and workspace).  ``query``: an int32 / int64 tensor ``[B]`` of query positions, on the host (negative
        positions are refused) or on this device; None = position 0.  -> ``[B, heads, W]`` fp32, ``out[s, h, j]`` bit-identical to
        ``attention_probs(...)[s, h, query[s], j]``, or with ``reduce_heads`` ``[B, W]``: the mean over heads (fp64 in head order,
        rounded once).  Every element is written: a position at or beyond a sequence's length gives a row of zeros.
        Asynchronous on the current torch stream."""

        self._require_attention_outputs()
        if not hasattr(self.lib, "op_attention_rows"):
            raise _lib.HipLibraryError("this library has no op_attention_rows")
        H, max_seqlen = self.dims.hidden_size, int(max_seqlen)
        if (hidden_packed.dtype != torch.float32 or hidden_packed.device != self.device or hidden_packed.ndim != 2
                or hidden_packed.shape[1] != H or not hidden_packed.is_contiguous()):
            raise ValueError(f"hidden_packed must be a contiguous fp32 [total_tokens, {H}] tensor on {self.device}")
        if cu_seqlens.dtype != torch.int32 or cu_seqlens.device != self.device:
            raise ValueError(f"cu_seqlens must be int32 on {self.device}")
        if not 0 <= int(layer) < self.dims.num_layers:
            raise ValueError(f"layer must lie in 0 .. {self.dims.num_layers - 1}")
        total, n_seqs = int(hidden_packed.shape[0]), int(cu_seqlens.numel()) - 1
        width = int(pad_width) or max_seqlen
        if width < max_seqlen:
            raise ValueError(f"pad_width must be 0 (= max_seqlen) or at least max_seqlen ({max_seqlen}), got {width}")
        cu_host = np.ascontiguousarray(cu_seqlens_host, dtype=np.int32)
        if cu_host.shape[0] != n_seqs + 1:
            raise ValueError("cu_seqlens_host length mismatch")
        query_dev, query_host = None, None
        if query is not None:
            if not isinstance(query, torch.Tensor) or query.ndim != 1 or query.dtype not in (torch.int32, torch.int64) or query.numel() != n_seqs:
                raise ValueError(f"query must be an int32 / int64 tensor of {n_seqs} positions")
            if query.device.type == "cpu":
                if n_seqs and int(query.min()) < 0:
                    raise ValueError("query holds a negative position")
                if n_seqs and int(query.max()) > np.iinfo(np.int32).max:
                    raise ValueError("query holds a position beyond int32")
                query_host = np.ascontiguousarray(query.numpy(), dtype=np.int32)
            elif query.device != self.device:
                raise ValueError(f"query must live on the host or on {self.device}")
            # (int64 on the device: clamped into int32 first, so that a huge position stays "beyond the length" and a negative one negative)
            query_dev = query.to(self.device).clamp(-1, np.iinfo(np.int32).max).to(torch.int32).contiguous()
        vp = ctypes.c_void_p
        with torch.cuda.device(self.device):
            shape = (n_seqs, width) if reduce_heads else (n_seqs, self.dims.num_heads, width)
            out = torch.empty(shape, dtype=torch.float32, device=self.device)
            if out.numel() == 0:
                return out
            need = int(self.lib.op_attention_workspace_bytes(self._handle, n_seqs, total, max_seqlen)) + 256
            ws = self._attention_workspace
            if ws is None or ws.numel() < need:
                ws = self._attention_workspace = torch.empty(need, dtype=torch.uint8, device=self.device)
            base = ws.data_ptr()
            aligned = (base + 255) // 256 * 256
            req = _lib.OpAttentionRowsRequest()
            req.struct_bytes = ctypes.sizeof(_lib.OpAttentionRowsRequest)
            req.layer = int(layer)
            req.pad_width = width
            req.reduce_heads = 1 if reduce_heads else 0
            req.hidden_dev = vp(hidden_packed.data_ptr()) if total else None
            req.query_pos_dev = vp(query_dev.data_ptr()) if query_dev is not None else None
            req.query_pos_host = query_host.ctypes.data_as(vp) if query_host is not None else None
            req.out_dev = vp(out.data_ptr())
            code = self.lib.op_attention_rows(
                self._handle, vp(cu_seqlens.data_ptr()), cu_host.ctypes.data_as(vp), n_seqs, total, max_seqlen, ctypes.byref(req),
                vp(aligned), ctypes.c_size_t(ws.numel() - (aligned - base)), vp(torch.cuda.current_stream(self.device).cuda_stream),
            )
        _lib.check(self.lib, self._handle, code, "op_attention_rows")
        return out

    def _forward(self, part: "int | None", ids, cu_seqlens, cu_seqlens_host, max_seqlen, keep_prob=None, hidden=None, ids_host=None,
                 running: "bool | None" = True, pooled=None) -> "tuple[PackedCall, torch.Tensor | None, torch.Tensor | None]":
        """The one body of :meth:`forward_packed` (``part`` None: the current stream, the encoder's workspace) and
        :meth:`forward_packed_on` (pipeline ``part``: its stream and workspace): checks, outputs, workspace, the launch and the
        audits (``running``: whether the running audit may look at this forward; None: no audit at all) -> (the call with its
        outputs, the hidden states of a ``hidden`` request, the rows of a ``pooled`` request)."""

        if ids.dtype != torch.int32 or cu_seqlens.dtype != torch.int32:
            raise TypeError("ids and cu_seqlens must be int32")
        if ids.device != self.device or cu_seqlens.device != self.device:
            raise ValueError(f"ids/cu_seqlens must live on {self.device}")
        total, n_seqs, max_seqlen = int(ids.numel()), int(cu_seqlens.numel()) - 1, int(max_seqlen)
        if keep_prob is not None and (
            keep_prob.dtype != torch.float32 or keep_prob.device != self.device or keep_prob.numel() != total
            or not keep_prob.is_contiguous()
        ):
            raise ValueError("keep_prob must be a contiguous fp32 tensor of total_tokens elements on the encoder's device")
        cu_host = np.ascontiguousarray(cu_seqlens_host, dtype=np.int32)
        if cu_host.shape[0] != n_seqs + 1:
            raise ValueError("cu_seqlens_host length mismatch")
        states, req = self._hidden_request(hidden, n_seqs, total, max_seqlen) if hidden is not None else (None, None)
        pooled_states, pool_req = self._pool_request(pooled, n_seqs, total) if pooled is not None else (None, None)
        slots = self._split_streams() if part is not None else None
        # The outputs of a pipeline come from the SIDE stream's pool of the caching allocator (allocated under that stream): a
        # block of that pool is only ever recycled in side-stream order, so the kernels that write them can never land on memory
        # a still-queued reader of the caller's stream owns (allocated from the caller's pool, a block freed there and
        # whose last reader is still queued could be handed out here and overwritten early: nothing orders the side
        # stream behind the caller's).  Consumers wait on pipeline_stream(part) before reading; a consumer that reads
        # them on ANOTHER stream and drops them right away should record_stream() them there, as with any tensor that
        # crosses streams.
        with torch.cuda.device(self.device), (torch.cuda.stream(slots["streams"][part]) if slots else nullcontext()):
            prune = torch.empty((total, 2), dtype=torch.float32, device=self.device)
            rank = torch.empty((n_seqs, self.dims.num_labels), dtype=torch.float32, device=self.device)
            if n_seqs == 0:
                ws = None
            elif slots is None:
                ws = self._ensure_workspace(n_seqs, total, max_seqlen)
            else:
                ws = slots["ws"][part] = self._grown_workspace(slots["ws"][part], n_seqs, total, max_seqlen)
            call = PackedCall(ids, cu_seqlens, cu_host, n_seqs, total, max_seqlen, prune, rank, keep_prob, ws,
                              torch.cuda.current_stream(self.device).cuda_stream, req, ids_host, pool_req=pool_req)
            if n_seqs:
                self._forward_native(call)
                # (an audit synchronises the call's stream once; on a pipeline, the other one must not be mid-forward on another
                # host thread while it runs -- the pipelines of one encoder are driven from ONE thread everywhere in this package)
                if running is not None:
                    maybe_audit(self, call, running)
        return call, states, pooled_states

    def _pool_request(self, pooled: "HiddenRequest", n_seqs: int, total: int):
        """-> (output tensor ``[n_sel, n_seqs, H]``, ``_lib.OpPoolRequest``) of one forward; the struct keeps its select array and
        its scratch entry (one packed fp32 entry, reused by every selected entry) alive."""

        if not isinstance(pooled, HiddenRequest) or pooled.pool is None:
            raise TypeError("a pooled request is a HiddenRequest with pool='first' or pool='mean'")
        n_entries = self.dims.num_layers + 1
        layers = range(n_entries) if pooled.layers is None else [int(i) for i in pooled.layers]
        if any(i < 0 or i >= n_entries for i in layers):
            raise ValueError(f"hidden.layers must lie in 0 .. {n_entries - 1} (entry {n_entries - 1} = the pruning head's input)")
        selected = sorted(set(layers))
        H = self.dims.hidden_size
        out = torch.empty((len(selected), n_seqs, H), dtype=torch.float32, device=self.device)
        scratch = torch.empty((total, H), dtype=torch.float32, device=self.device)
        flags = (ctypes.c_uint8 * n_entries)(*[1 if i in selected else 0 for i in range(n_entries)])
        req = _lib.OpPoolRequest()
        req.struct_bytes = ctypes.sizeof(_lib.OpPoolRequest)
        req.kind = _lib.POOL_KINDS[pooled.pool]
        req.select = ctypes.cast(flags, ctypes.POINTER(ctypes.c_uint8))
        req.out_dev = ctypes.c_void_p(out.data_ptr()) if out.numel() else None
        req.scratch_dev = ctypes.c_void_p(scratch.data_ptr()) if scratch.numel() else None
        req.scratch_bytes = scratch.numel() * 4
        req._keep = (flags, scratch)  # (alive as long as the struct)
        return out, req
    def _hidden_request(self, hidden: "HiddenRequest", n_seqs: int, total: int, max_seqlen: int):
        """-> (output tensor, ``_lib.OpHiddenRequest``) of one forward; the struct keeps its select array alive."""

        if not isinstance(hidden, HiddenRequest):
            raise TypeError("hidden must be a HiddenRequest")
        n_entries = self.dims.num_layers + 1
        layers = range(n_entries) if hidden.layers is None else [int(i) for i in hidden.layers]
        if any(i < 0 or i >= n_entries for i in layers):
            raise ValueError(f"hidden.layers must lie in 0 .. {n_entries - 1} (entry {n_entries - 1} = the pruning head's input)")
        selected = sorted(set(layers))
        dtypes = {torch.float32: _lib.OP_HIDDEN_F32, torch.bfloat16: _lib.OP_HIDDEN_BF16}
        if hidden.dtype not in dtypes:
            raise ValueError("hidden.dtype must be torch.float32 or torch.bfloat16")
        pad = int(hidden.pad_width)
        if pad < 0 or (pad > 0 and pad < max_seqlen):
            raise ValueError(f"hidden.pad_width must be 0 (packed) or at least max_seqlen ({max_seqlen}), got {pad}")
        H = self.dims.hidden_size
        if pad > 0:  # (positions beyond a sequence's length are not written)
            out = torch.zeros((len(selected), n_seqs, pad, H), dtype=hidden.dtype, device=self.device)
        else:
            out = torch.empty((len(selected), total, H), dtype=hidden.dtype, device=self.device)
        flags = (ctypes.c_uint8 * n_entries)(*[1 if i in selected else 0 for i in range(n_entries)])
        req = _lib.OpHiddenRequest()
        req.struct_bytes = ctypes.sizeof(_lib.OpHiddenRequest)
        req.dtype = dtypes[hidden.dtype]
        req.pad_width = pad
        req.select = ctypes.cast(flags, ctypes.POINTER(ctypes.c_uint8))
        req.out_dev = ctypes.c_void_p(out.data_ptr()) if out.numel() else None
        req._flags = flags  # (keeps the array alive as long as the struct)
        return out, req

    # -- the audits of a calibrated kernel set: the device steps of audit.py ------------------------------------------------
    @property
    def audit_pending(self) -> bool:
        """True while a kernel set chosen on the library's synthetic batch has not seen real rows yet."""

        return self.audit_state.pending

    def audit_rows(self, rows: "Sequence[Sequence[int]]") -> "bool | None":
        """The first-real-batch audit as an explicit call that only MEASURES: ``rows`` through the calibrated set and through the
        reference set, ``calibration["audit"]`` filled, the pending flag cleared; the kernel set is left where it is (the
        caller -- ``sharding.collective_audit`` -- combines the ranks' verdicts and reverts all of them or none).  Returns the
        verdict, or None when there is nothing to audit (no calibrated set pending, or fewer than 64 tokens)."""

        if not self.audit_pending:
            return None
        ids_np, cu_np, max_len = pack_rows(rows)
        if int(cu_np[-1]) < MIN_AUDIT_TOKENS:
            return None
        self.check_ids(ids_np)
        ids = torch.from_numpy(ids_np).to(self.device)
        cu = torch.from_numpy(cu_np).to(self.device)
        call, _, _ = self._forward(None, ids, cu, cu_np, max_len, running=None)  # (what is pinned now: the calibrated set, its layer mask included)
        return first_batch_audit(self, call, collective=True)

    def revert_to_default(self, reason: str, *, warning: "str | None" = None, stacklevel: int = 3,
                          recompute: "PackedCall | None" = None) -> str:
        """Back to the default selection of ``op_weights_ready`` for good (what a failed audit does), with a warning, and
        ``recompute`` -- the forward whose audit failed -- run again there, into the caller's outputs.  ``warning`` (the
        first-batch audit's own sentence, ``{after!r}`` = the set that runs from now on) replaces the standard one and keeps
        ``reason`` out of the report."""

        before = self.effective_policy()["kernel_set"]
        self.select_kernel_set("auto")
        after = self.effective_policy()["kernel_set"]
        if self.calibration is not None:
            self.calibration["chosen_set"] = after
            if warning is None:
                self.calibration["reverted"] = reason
        if warning is not None:
            warnings.warn(warning.format(after=after), RuntimeWarning, stacklevel=stacklevel)
        elif after != before:
            warnings.warn(f"open_provence_amd: kernel set {before!r} dropped ({reason}); this model runs on {after!r} from now on.",
                          RuntimeWarning, stacklevel=stacklevel)
        if recompute is not None:
            self._forward_native(recompute)
        return after

    def _reset_coverage(self, running: bool) -> None:
        """Forget what was audited, on the host and in the handle (a new arithmetic has seen nothing), and switch the running
        audit on or off."""

        self.audit_state.reset(running)
        if hasattr(self.lib, "op_coverage_reset") and self._handle:
            self.lib.op_coverage_reset(self._handle)

    def _audit_blocked(self) -> bool:
        """No audit now: a debug hidden capture, a process group's collective audit, or a stream being captured into a hipGraph."""

        return self._capture is not None or bool(self.audit_collective) or torch.cuda.is_current_stream_capturing()

    def _commit_coverage(self, call: PackedCall) -> None:
        """Every row of ``call`` into the handle's coverage bitmap (``op_coverage_commit`` on the current stream)."""

        rows_dev = torch.arange(call.n_seqs, dtype=torch.int32, device=self.device)
        vp = ctypes.c_void_p
        code = self.lib.op_coverage_commit(self._handle, vp(call.ids.data_ptr()), vp(call.cu_seqlens.data_ptr()), call.n_seqs, call.total,
                                           vp(rows_dev.data_ptr()), call.n_seqs, vp(call.stream))
        _lib.check(self.lib, self._handle, code, "op_coverage_commit")

    def coverage_scan_device(self, ids: torch.Tensor, cu_seqlens: torch.Tensor, n_seqs: int, total: int) -> "tuple[torch.Tensor, dict]":
        """``op_coverage_scan`` on the current stream (synchronised once): ``(row_novel[int32, n_seqs] on the device, {"novel",
        "longest", "longest_row", "max_audited"})`` -- the coverage decision for a batch whose ids are not on the host."""

        row_novel = torch.empty(max(n_seqs, 1), dtype=torch.int32, device=self.device)
        report = _lib.OpCoverageReport()
        report.struct_bytes = ctypes.sizeof(_lib.OpCoverageReport)
        with torch.cuda.device(self.device):
            stream = torch.cuda.current_stream(self.device).cuda_stream
            code = self.lib.op_coverage_scan(self._handle, ctypes.c_void_p(ids.data_ptr()) if total else None, ctypes.c_void_p(cu_seqlens.data_ptr()),
                                             int(n_seqs), int(total), ctypes.c_void_p(row_novel.data_ptr()), ctypes.byref(report),
                                             ctypes.c_void_p(stream))
        _lib.check(self.lib, self._handle, code, "op_coverage_scan")
        return row_novel[:n_seqs], {"novel": int(report.novel_tokens), "longest": int(report.longest_row_tokens),
                                    "longest_row": int(report.longest_row), "max_audited": int(report.max_audited_tokens)}

    def _reference_call(self, call: PackedCall, rows: "Sequence[int] | None" = None) -> PackedCall:
        """The forward an audit runs on the reference set: ``call``'s batch, or its ``rows`` gathered into a sub-batch on the
        device (``op_gather_rows``), into outputs of its own, with no ``keep_prob`` and no hidden request."""

        if rows is None:
            return call._replace(prune=torch.empty_like(call.prune), rank=torch.empty_like(call.rank), keep_prob=None, hidden_req=None,
                                 pool_req=None, size_ws_at_launch=True)
        sub_lengths = np.diff(call.cu_host)[list(rows)]
        sub_cu_host = np.concatenate(([0], np.cumsum(sub_lengths))).astype(np.int32)
        sub_ids_host = None if call.ids_host is None else np.concatenate([call.ids_host[call.cu_host[r]: call.cu_host[r + 1]] for r in rows])
        n_sub, sub_total, sub_max = len(rows), int(sub_cu_host[-1]), int(sub_lengths.max())
        rows_dev = torch.tensor(rows, dtype=torch.int32, device=self.device)
        sub_ids = torch.empty(sub_total, dtype=torch.int32, device=self.device)
        sub_cu = torch.empty(n_sub + 1, dtype=torch.int32, device=self.device)
        vp = ctypes.c_void_p
        code = self.lib.op_gather_rows(self._handle, vp(call.ids.data_ptr()), vp(call.cu_seqlens.data_ptr()), call.n_seqs, call.total,
                                       vp(rows_dev.data_ptr()), n_sub, vp(sub_ids.data_ptr()), vp(sub_cu.data_ptr()), vp(call.stream))
        _lib.check(self.lib, self._handle, code, "op_gather_rows")
        return PackedCall(sub_ids, sub_cu, sub_cu_host, n_sub, sub_total, sub_max,
                          torch.empty((sub_total, 2), dtype=torch.float32, device=self.device),
                          torch.empty((n_sub, self.dims.num_labels), dtype=torch.float32, device=self.device), None,
                          call.ws, call.stream, None, sub_ids_host, rows_dev, True)

    def _logit_error(self, call: PackedCall, ref: PackedCall) -> float:
        """max |logit difference| between ``call``'s outputs and those of ``ref`` (:meth:`_reference_call`); synchronises.  The
        whole batch: in torch (a non-finite logit gives NaN).  A sub-batch: ``op_audit_compare`` against its rows (+inf)."""

        if ref.rows is None:
            return float(torch.maximum((call.prune - ref.prune).abs().max(), (call.rank - ref.rank).abs().max()).item())
        err_dev = torch.empty(1, dtype=torch.float32, device=self.device)
        vp = ctypes.c_void_p
        code = self.lib.op_audit_compare(self._handle, vp(call.prune.data_ptr()), vp(call.rank.data_ptr()), vp(call.cu_seqlens.data_ptr()),
                                         call.n_seqs, call.total, vp(ref.rows.data_ptr()), ref.n_seqs, vp(ref.prune.data_ptr()),
                                         vp(ref.rank.data_ptr()), vp(ref.cu_seqlens.data_ptr()), vp(err_dev.data_ptr()), vp(call.stream))
        _lib.check(self.lib, self._handle, code, "op_audit_compare")
        return float(err_dev.item())

    def _grown_workspace(self, ws: "torch.Tensor | None", n_seqs: int, total: int, max_seqlen: int) -> torch.Tensor:
        """``ws`` if it holds a forward of this geometry (``op_workspace_bytes`` + 256 for alignment), else a new one that does."""

        need = int(self.lib.op_workspace_bytes(self._handle, n_seqs, total, max_seqlen)) + 256
        return ws if ws is not None and ws.numel() >= need else torch.empty(need, dtype=torch.uint8, device=self.device)

    def _forward_native(self, call: PackedCall) -> None:
        """``op_forward_packed[_hidden]``: the only place a :class:`PackedCall` becomes C arguments."""

        vp = ctypes.c_void_p
        ws = call.ws
        if call.size_ws_at_launch:
            need = int(self.lib.op_workspace_bytes(self._handle, call.n_seqs, call.total, call.max_seqlen)) + 256
            if ws is None or ws.numel() < need:
                # kept on the encoder: the forward is asynchronous, and the next audit finds it again
                ws = self._audit_workspace = self._grown_workspace(self._audit_workspace, call.n_seqs, call.total, call.max_seqlen)
        base = ws.data_ptr()
        aligned = (base + 255) // 256 * 256
        extra = () if call.hidden_req is None else (ctypes.byref(call.hidden_req),)
        entry = self.lib.op_forward_packed if call.hidden_req is None else self.lib.op_forward_packed_hidden
        if call.pool_req is not None:
            if not hasattr(self.lib, "op_forward_packed_pooled"):
                raise _lib.HipLibraryError("this library has no op_forward_packed_pooled")
            entry = self.lib.op_forward_packed_pooled
            extra = (ctypes.byref(call.hidden_req) if call.hidden_req is not None else None, ctypes.byref(call.pool_req))
        code = entry(
            self._handle, vp(call.ids.data_ptr()), vp(call.cu_seqlens.data_ptr()), call.cu_host.ctypes.data_as(vp),
            call.n_seqs, call.total, call.max_seqlen, vp(call.prune.data_ptr()), vp(call.rank.data_ptr()),
            vp(call.keep_prob.data_ptr()) if call.keep_prob is not None else None,
            vp(aligned), ctypes.c_size_t(ws.numel() - (aligned - base)), vp(call.stream), *extra,
        )
        _lib.check(self.lib, self._handle, code, "op_forward_packed_pooled" if call.pool_req is not None else
                   "op_forward_packed" if call.hidden_req is None else "op_forward_packed_hidden")

    def _split_streams(self) -> dict:
        """Two HIP streams of their own (hipExtStreamCreateWithCUMask with the full mask: own hardware queues, no CU partition since
        round 6; plain streams if the runtime refuses) and a workspace per stream, created once."""

        st = self._split_state
        if st is None:
            n_cus = int(torch.cuda.get_device_properties(self.device).multi_processor_count)
            streams = []
            raw_streams: list[int] = []
            hip = None
            try:
                hip = ctypes.CDLL("libamdhip64.so")
                words = (n_cus + 31) // 32
                with torch.cuda.device(self.device):
                    for half in range(2):
                        # Which CUs a pipeline gets (round 6): ALL of them -- two streams created through the CU-mask API (their
                        # own hardware queues) with the full mask.  Halves of the chip (contiguous halves of the mask's bit index =
                        # 16 CUs of every XCD each: rounds 2 - 5) leave the two launch sequences in one of two phase relations for
                        # a whole run, the bad one BELOW one sequence (63.6 - 64.3 k pairs/s in 4 of 5 hundred-step runs on one
                        # box, 68.8 k on another); unpartitioned, the blocks of the two sequences share the CUs as they come --
                        # 66.8 - 69.5 k on both boxes, never below (profiles/r06_exp_phase_diversity.txt, section 6; which CUs a
                        # mask really gives: microbench/cu_mask_probe.hip -- alternate bits or runs of 4 are NOT honoured as a
                        # partition, both streams get all 256 CUs).  OPEN_PROVENCE_PIPELINE_MASK_GROUP: 0 = the contiguous
                        # halves, g > 0 = runs of g bits alternate (measurement hook).
                        group = int(os.environ.get("OPEN_PROVENCE_PIPELINE_MASK_GROUP", "-1") or 0)
                        bits = [True if group < 0 else ((c // group) % 2 if group > 0 else (c * 2 // n_cus)) == half for c in range(n_cus)]
                        mask = (ctypes.c_uint32 * words)(
                            *[sum(1 << b for b in range(32) if w * 32 + b < n_cus and bits[w * 32 + b]) for w in range(words)]
                        )
                        handle = ctypes.c_void_p()
                        if hip.hipExtStreamCreateWithCUMask(ctypes.byref(handle), ctypes.c_uint32(words), mask) != 0:
                            raise OSError("hipExtStreamCreateWithCUMask failed")
                        raw_streams.append(int(handle.value))
                        streams.append(torch.cuda.ExternalStream(handle.value, device=self.device))
            except (OSError, AttributeError):
                streams = [torch.cuda.Stream(self.device) for _ in range(2)]
            st = self._split_state = {"streams": streams, "ws": [None, None], "raw_streams": raw_streams[: len(streams)] if len(raw_streams) == len(streams) else [], "hip": hip}
        return st

    def forward_packed_on(
        self,
        part: int,
        ids: torch.Tensor,
        cu_seqlens: torch.Tensor,
        cu_seqlens_host: np.ndarray,
        max_seqlen: int,
        keep_prob: torch.Tensor | None = None,
        hidden: "HiddenRequest | None" = None,
        attentions: "AttentionRequest | None" = None,
    ) -> tuple[torch.Tensor, torch.Tensor]:
        """``forward_packed`` enqueued on pipeline ``part`` (0 or 1): its own HIP stream (own hardware queue; the whole chip
        since round 6, see ``_split_streams``) and its own workspace -- nothing is ordered against the caller's current stream or the other
        pipeline (inputs must already be resident; wait on ``pipeline_stream(part)`` before reading the outputs).

        Why two pipelines: every CU of a launch is in the same phase at the same time -- all fetch, then all multiply
        -- so HBM idles while the matrix pipes work and vice versa; two INDEPENDENT launch sequences
        drift apart and fill each other's gaps (xsmall, 2 x 128 pairs x 512 against 1 x 256: +3 .. +6 % pairs/s, same box).
        Forking and joining the halves inside every forward instead re-aligns them each time and loses 4 %."""

        if part not in (0, 1):
            raise ValueError("part must be 0 or 1")
        if self._capture is not None:
            raise RuntimeError("hidden-state capture is not available on the pipelined path (use forward_packed)")
        if hidden is not None:
            raise NotImplementedError("hidden-state requests are not available on the pipelined path (use forward_packed(hidden=...))")
        if attentions is not None:
            raise NotImplementedError("attention requests are not available on the pipelined path (use forward_packed(attentions=...))")
        call, _, _ = self._forward(part, ids, cu_seqlens, cu_seqlens_host, max_seqlen, keep_prob, running=False)
        return call.prune, call.rank

    def pipeline_stream(self, part: int) -> torch.cuda.Stream:
        return self._split_streams()["streams"][part]

    def check_ids(self, ids: np.ndarray) -> None:
        """``nn.Embedding`` raises on out-of-range ids (the reference's behaviour); the kernel only clamps them as a
        memory-safety net, so the host validates wherever ids are still in host memory."""

        if ids.size and (int(ids.min()) < 0 or int(ids.max()) >= self.dims.vocab_size):
            raise IndexError(
                f"token id out of range for the embedding table: ids span [{int(ids.min())}, {int(ids.max())}], "
                f"vocab_size is {self.dims.vocab_size}"
            )

    # -- any attention mask: the dense forward on the fp32 kernels (op_forward_masked) ------------------------------------------
    def forward_masked(self, input_ids: torch.Tensor, attention_mask: torch.Tensor,
                       workspace: "torch.Tensor | None" = None) -> "tuple[torch.Tensor, torch.Tensor]":
        """``input_ids[B, L]`` + ANY ``attention_mask[B, L]`` (left padding, holes; CPU or this device) -> ``(pruning_logits[B, L,
        2], ranking_logits[B, num_labels])`` fp32 on the device, on an encoder created with ``attention_masks="any"``.  Every
        position is a row at position = its column and the mask removes keys only, as in the reference under eager attention;
        a query left without a key in a sliding-window layer takes the mean of ``v`` over its row.  Pruning logits are exact
        zeros where the mask is 0; a row whose mask is all zeros gives zeros in both outputs.  fp32 arithmetic of kernel set
        "fp32" whatever set the forward runs on; the dense pass computes the pads.  Every position is embedded: an id outside
        the table raises ``IndexError`` wherever it sits.  The current torch stream is synchronised once (the id check).
        ``workspace``: a uint8 device tensor to carve instead of the encoder's own (concurrent calls on several streams).

        On an encoder created with ``masked_kernels="selected"`` the same call runs ``op_forward_masked_native``: the arithmetic of
        the kernel set the packed forward runs on (a query without a key: the mean of ``v`` as that set stores it), and on the
        fp16 + e4m3 sets the range guard of :meth:`forward_packed_checked` -- a non-finite result is repeated on the (hi, lo)
        bf16 sets, where the encoder then stays."""

        if self.attention_masks != "any":
            raise ValueError('forward_masked needs the fp32 weight packs: create the encoder / model with attention_masks="any"')
        entry = "op_forward_masked_native" if self.masked_native else "op_forward_masked"
        sizer = "op_masked_native_workspace_bytes" if self.masked_native else "op_masked_workspace_bytes"
        if not hasattr(self.lib, entry):
            raise _lib.HipLibraryError(f"this library has no {entry}")
        input_ids, attention_mask = torch.as_tensor(input_ids), torch.as_tensor(attention_mask)
        if input_ids.ndim != 2:
            raise ValueError("input_ids must be [B, L]")
        n_rows, width = int(input_ids.shape[0]), int(input_ids.shape[1])
        if tuple(attention_mask.shape) != (n_rows, width):
            raise ValueError("attention_mask shape must match input_ids")
        if n_rows * width >= 2**31:
            raise ValueError("batch has more than 2^31 positions")
        if width > self.dims.max_position_embeddings:
            raise ValueError(f"width {width} exceeds max_position_embeddings {self.dims.max_position_embeddings}")
        ids_in = input_ids.detach()
        if ids_in.dtype.is_floating_point or ids_in.dtype in (torch.bool, torch.complex64, torch.complex128):
            raise TypeError(f"input_ids must be an integer tensor, got {ids_in.dtype}")
        ids_in = ids_in.to(self.device)
        if ids_in.dtype != torch.int32:  # (an id beyond int32 is outside every table: it stays outside, -1 or 2^31 - 1)
            ids_in = ids_in.to(torch.int64).clamp(-1, 2**31 - 1).to(torch.int32)
        ids_in = ids_in.contiguous()
        mask_in = attention_mask.detach().to(self.device).ne(0).contiguous().view(torch.uint8)
        vp = ctypes.c_void_p
        report = _lib.OpMaskedReport()
        report.struct_bytes = ctypes.sizeof(_lib.OpMaskedReport)
        with torch.cuda.device(self.device):
            prune = torch.empty((n_rows, width, 2), dtype=torch.float32, device=self.device)
            rank = torch.empty((n_rows, self.dims.num_labels), dtype=torch.float32, device=self.device)
            if prune.numel() == 0:
                return prune, rank.zero_()
            need = int(getattr(self.lib, sizer)(self._handle, n_rows, width)) + 256
            ws = workspace if workspace is not None else self._masked_workspace
            if ws is None or ws.numel() < need:
                if workspace is not None:
                    raise ValueError(f"workspace has {ws.numel()} bytes, need {need}")
                ws = self._masked_workspace = torch.empty(need, dtype=torch.uint8, device=self.device)
            base = ws.data_ptr()
            aligned = (base + 255) // 256 * 256

            def run() -> int:
                return getattr(self.lib, entry)(
                    self._handle, vp(ids_in.data_ptr()), vp(mask_in.data_ptr()), n_rows, width, vp(aligned),
                    ctypes.c_size_t(ws.numel() - (aligned - base)), vp(prune.data_ptr()), vp(rank.data_ptr()), ctypes.byref(report),
                    vp(torch.cuda.current_stream(self.device).cuda_stream),
                )

            code = run()
            # (the range guard of forward_packed_checked: the selected set may be an fp16 + e4m3 one)
            if code == _lib.OP_OK and self.masked_native and self.f8_active():
                ok = torch.isfinite(rank).all() & torch.isfinite(prune).all()
                if not bool(ok.item()) and self.fall_back_from_f8("forward_masked"):
                    code = run()
        if code == _lib.OP_ERR_INVALID and int(report.status) & _lib.OP_PADDED_BAD_ID:
            raise IndexError(
                f"token id out of range for the embedding table: id {int(report.id_value)} at row {int(report.id_row)}, "
                f"column {int(report.id_col)}; vocab_size is {self.dims.vocab_size}"
            )
        _lib.check(self.lib, self._handle, code, entry)
        return prune, rank

    # -- the padded boundary on the device (op_pack_padded / op_unpack_padded) -----------------------------------------
    def pack_padded_device(self, input_ids: torch.Tensor, attention_mask: "torch.Tensor | None"
                           ) -> "tuple[torch.Tensor, torch.Tensor, np.ndarray, int]":
        """``packing.pack_padded`` + :meth:`check_ids` for a batch that is already on this device: ``input_ids[B, L]`` (+
        right-padded ``attention_mask[B, L]`` or None) -> ``(ids[int32, T], cu_seqlens[int32, B+1], cu_seqlens_host, max_len)``,
        the first two on the device -- the arguments of :meth:`forward_packed`.  Lengths, both checks, the scan and the gather
        run in HIP kernels on the current stream, which is synchronised once (the forward needs T and ``max_len`` on the host).
        Raises what the host path raises: ``NotImplementedError`` for a mask that is not ones-then-zeros (it wins when both
        faults are present, as on the host), ``IndexError`` for an id outside the embedding table at an unmasked position."""

        return self._pack_padded_device(input_ids, attention_mask, non_prefix_ok=False)

    def _pack_padded_device(self, input_ids, attention_mask, non_prefix_ok: bool):
        """:meth:`pack_padded_device`; ``non_prefix_ok``: a mask that is not ones-then-zeros returns None instead of raising
        (forward() on an ``attention_masks="any"`` model then runs :meth:`forward_masked`: the same single synchronisation
        has decided the route)."""

        if input_ids.ndim != 2:
            raise ValueError("input_ids must be [B, L]")
        n_rows, width = int(input_ids.shape[0]), int(input_ids.shape[1])
        if attention_mask is not None and tuple(attention_mask.shape) != (n_rows, width):
            raise ValueError("attention_mask shape must match input_ids")
        if input_ids.device != self.device or (attention_mask is not None and attention_mask.device != self.device):
            raise ValueError(f"input_ids / attention_mask must live on {self.device}")
        if n_rows * width >= 2**31:
            raise ValueError("batch has more than 2^31 positions")
        int_types = {torch.int32: _lib.OP_INT_I32, torch.int64: _lib.OP_INT_I64, torch.uint8: _lib.OP_INT_U8}
        ids_in = input_ids.detach()
        if ids_in.dtype not in (torch.int32, torch.int64):
            if ids_in.dtype.is_floating_point or ids_in.dtype in (torch.bool, torch.complex64, torch.complex128):
                raise TypeError(f"input_ids must be an integer tensor, got {ids_in.dtype}")
            ids_in = ids_in.to(torch.int64)
        ids_in = ids_in.contiguous()
        mask_in = None
        if attention_mask is not None:
            mask_in = attention_mask.detach()
            if mask_in.dtype == torch.bool:
                mask_in = mask_in.contiguous().view(torch.uint8)
            elif mask_in.dtype not in int_types:  # other integer and float masks: reduced to bool on the device
                mask_in = mask_in.ne(0).view(torch.uint8)
            mask_in = mask_in.contiguous()
        packed = torch.empty(n_rows * width, dtype=torch.int32, device=self.device)
        cu = torch.empty(n_rows + 1, dtype=torch.int32, device=self.device)
        cu_host = np.zeros(n_rows + 1, dtype=np.int32)
        report = _lib.OpPaddedReport()
        report.struct_bytes = ctypes.sizeof(_lib.OpPaddedReport)
        with torch.cuda.device(self.device):
            stream = torch.cuda.current_stream(self.device).cuda_stream
            code = self.lib.op_pack_padded(
                self._handle, ctypes.c_void_p(ids_in.data_ptr()) if ids_in.numel() else None, int_types[ids_in.dtype],
                ctypes.c_void_p(mask_in.data_ptr()) if mask_in is not None and mask_in.numel() else None,
                int_types[mask_in.dtype] if mask_in is not None else 0, n_rows, width,
                ctypes.c_void_p(packed.data_ptr()) if packed.numel() else None, ctypes.c_void_p(cu.data_ptr()),
                cu_host.ctypes.data_as(ctypes.c_void_p), ctypes.byref(report), ctypes.c_void_p(stream),
            )
        status = int(report.status)
        if code == _lib.OP_ERR_INVALID and status & _lib.OP_PADDED_BAD_MASK:
            if non_prefix_ok:
                return None
            raise NotImplementedError(
                "attention_mask must be right-padded (ones then zeros): the packed HIP path derives positions "
                "from token order, exactly what the reference's process() produces (standalone.py:2832-2880)."
                f"  First offender: row {int(report.mask_row)}, column {int(report.mask_col)}."
            )
        if code == _lib.OP_ERR_INVALID and status & _lib.OP_PADDED_BAD_ID:
            raise IndexError(
                f"token id out of range for the embedding table: id {int(report.id_value)} at row {int(report.id_row)}, "
                f"column {int(report.id_col)}; vocab_size is {self.dims.vocab_size}"
            )
        _lib.check(self.lib, self._handle, code, "op_pack_padded")
        return packed[: int(report.total_tokens)], cu, cu_host, int(report.max_seqlen)

    def unpack_padded_device(self, values: torch.Tensor, cu_seqlens: torch.Tensor, n_rows: int, width: int) -> torch.Tensor:
        """``packing.unpack_to_padded`` in one kernel: packed fp32 ``values[T, 2]`` (pruning logits) or ``values[T]`` / ``[T, 1]``
        (keep-probabilities) -> ``[n_rows, width, 2]`` / ``[n_rows, width]`` / ``[n_rows, width, 1]`` with +0.0 at the positions
        beyond each row's length.  Every element of the result is written by the kernel (no memset, no index tensors).
        Asynchronous on the current stream."""

        if values.dtype != torch.float32 or cu_seqlens.dtype != torch.int32:
            raise TypeError("values must be fp32 and cu_seqlens int32")
        if values.device != self.device or cu_seqlens.device != self.device:
            raise ValueError(f"values / cu_seqlens must live on {self.device}")
        channels = 1 if values.ndim == 1 else int(values.shape[1]) if values.ndim == 2 else 0
        if channels not in (1, 2):
            raise ValueError("values must be [T], [T, 1] or [T, 2]")
        n_rows, width = int(n_rows), int(width)
        if n_rows < 0 or width < 0 or n_rows * width >= 2**31 or int(cu_seqlens.numel()) != n_rows + 1:
            raise ValueError("n_rows / width do not describe cu_seqlens")
        if not values.is_contiguous() or not cu_seqlens.is_contiguous():
            raise ValueError("values and cu_seqlens must be contiguous")
        shape = (n_rows, width) + tuple(values.shape[1:])
        if values.shape[0] == 0:  # (nothing to read: an empty batch, or empty rows only)
            return torch.zeros(shape, dtype=torch.float32, device=self.device)
        out = torch.empty(shape, dtype=torch.float32, device=self.device)
        if out.numel() == 0:
            return out
        with torch.cuda.device(self.device):
            stream = torch.cuda.current_stream(self.device).cuda_stream
            code = self.lib.op_unpack_padded(
                self._handle, ctypes.c_void_p(values.data_ptr()), ctypes.c_void_p(cu_seqlens.data_ptr()), n_rows, width, channels,
                ctypes.c_void_p(out.data_ptr()), ctypes.c_void_p(stream),
            )
        _lib.check(self.lib, self._handle, code, "op_unpack_padded")
        return out

    # -- the evaluation losses on the device (op_loss) -----------------------------------------------------------------
    def loss(self, kind: str, logits: torch.Tensor, labels: torch.Tensor, *, cu: "torch.Tensor | None" = None,
             width: "int | None" = None, ignore_index: int = -100, terms: bool = False, check: bool = True
             ) -> "torch.Tensor | tuple[torch.Tensor, torch.Tensor]":
        """The losses of the reference's inference file over logits that are already on this device (``op_loss``): a 0-dim fp32
        device tensor, and with ``terms=True`` also the unreduced fp32 terms (+0.0 where the label is ``ignore_index``).

        ``kind``: ``"token_ce"`` -- packed pruning ``logits[T, 2]`` as :meth:`forward_packed` leaves them, padded integer
        ``labels[n_rows, width]`` and the batch's ``cu`` (int32 ``[n_rows + 1]``); the mean 2-class cross entropy over the
        tokens whose label is not ``ignore_index`` (terms ``[T]``).  ``"rank_bce"`` -- ``logits[n_rows]`` or ``[n_rows, 1]``,
        fp32 ``labels[n_rows]`` (terms ``[n_rows]``).  ``"rank_ce"`` -- ``logits[n_rows, C]``, integer ``labels[n_rows]``
        (terms ``[n_rows]``).  ``"rank_mse"`` -- ``logits[n_rows, C]`` and fp32 ``labels`` of the same shape (terms too).
        Terms are evaluated in fp64 and added in a fixed order: the same inputs give the same bits on every call.

        ``check=True`` reads the call's report back (one synchronisation of the current stream) and raises ``IndexError`` for
        a label outside ``0 <= y < C`` that is not ``ignore_index``, naming its row, column and value, as torch does on the
        CPU.  ``check=False`` is asynchronous; such a label then makes the loss NaN."""

        if kind not in _lib.LOSS_KINDS:
            raise ValueError(f"unknown loss kind {kind!r}: one of {sorted(_lib.LOSS_KINDS)}")
        if logits.dtype != torch.float32:
            raise TypeError(f"logits must be fp32, got {logits.dtype}")
        if logits.device != self.device or labels.device != self.device or (cu is not None and cu.device != self.device):
            raise ValueError(f"logits / labels / cu must live on {self.device}")
        integer = kind in ("token_ce", "rank_ce")
        labels = labels.detach()
        if integer:
            if labels.dtype.is_floating_point or labels.dtype.is_complex or labels.dtype == torch.bool:
                raise TypeError(f"{kind} labels must be an integer tensor, got {labels.dtype}")
            if labels.dtype not in (torch.int32, torch.int64):
                labels = labels.to(torch.int64)
        elif labels.dtype != torch.float32:
            raise TypeError(f"{kind} labels must be fp32, got {labels.dtype}")
        logits, labels = logits.detach().contiguous(), labels.contiguous()
        total = 0
        if kind == "token_ce":
            if logits.ndim != 2 or logits.shape[1] != 2:
                raise ValueError("token_ce logits must be packed [T, 2]")
            if labels.ndim != 2 or (width is not None and int(width) != labels.shape[1]):
                raise ValueError("token_ce labels must be [n_rows, width]")
            n_rows, width, channels, total = int(labels.shape[0]), int(labels.shape[1]), 2, int(logits.shape[0])
            if cu is None or cu.dtype != torch.int32 or cu.ndim != 1 or int(cu.numel()) != n_rows + 1 or not cu.is_contiguous():
                raise ValueError("token_ce needs cu: contiguous int32 [n_rows + 1]")
            if total > n_rows * width:
                raise ValueError(f"{total} packed tokens do not fit labels of shape {tuple(labels.shape)}")
            terms_shape: tuple = (total,)
        else:
            if kind == "rank_bce" and logits.ndim == 1:
                logits = logits.unsqueeze(1)
            if logits.ndim != 2:
                raise ValueError(f"{kind} logits must be [n_rows, C]")
            n_rows, channels, width = int(logits.shape[0]), int(logits.shape[1]), 0
            if kind == "rank_bce" and channels != 1:
                raise ValueError("rank_bce takes one logit per row")
            if kind == "rank_ce" and channels < 2:
                raise ValueError("rank_ce takes at least two logits per row")
            want = (n_rows, channels) if kind == "rank_mse" else (n_rows,)
            if tuple(labels.shape) != want:
                raise ValueError(f"{kind} labels must have shape {want}, got {tuple(labels.shape)}")
            terms_shape = want
        if n_rows * max(width, channels) >= 2**31:
            raise ValueError("batch has more than 2^31 positions")
        out = torch.empty((), dtype=torch.float32, device=self.device)
        terms_out = torch.empty(terms_shape, dtype=torch.float32, device=self.device) if terms else None
        ptr = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None and t.numel() else None  # noqa: E731
        req = _lib.OpLossRequest()
        req.struct_bytes = ctypes.sizeof(_lib.OpLossRequest)
        req.kind = _lib.LOSS_KINDS[kind]
        req.logits_dev, req.labels_dev, req.cu_seqlens_dev, req.terms_dev = ptr(logits), ptr(labels), ptr(cu), ptr(terms_out)
        req.labels_dtype = {torch.int32: _lib.OP_INT_I32, torch.int64: _lib.OP_INT_I64, torch.float32: _lib.OP_LABELS_F32}[labels.dtype]
        req.n_rows, req.width, req.channels, req.total_tokens = n_rows, width, channels, total
        req.ignore_index = int(ignore_index)
        report = None
        if check:
            report = _lib.OpLossReport()
            report.struct_bytes = ctypes.sizeof(_lib.OpLossReport)
        with torch.cuda.device(self.device):
            stream = torch.cuda.current_stream(self.device).cuda_stream
            code = self.lib.op_loss(self._handle, ctypes.byref(req), ctypes.c_void_p(out.data_ptr()),
                                    ctypes.byref(report) if report is not None else None, ctypes.c_void_p(stream))
        # what the last checked call read back (None after an unchecked one): the count and fp64 sum behind the mean
        self.last_loss_report = ({name: getattr(report, name) for name in ("status", "bad_row", "bad_col", "bad_value", "count", "sum", "loss")}
                                 if report is not None else None)
        if report is not None and code == _lib.OP_ERR_INVALID and int(report.status) & _lib.OP_LOSS_BAD_LABEL:
            raise IndexError(f"label {int(report.bad_value)} at row {int(report.bad_row)}, column {int(report.bad_col)} is out of "
                             f"range for {channels} classes (ignore_index is {int(ignore_index)})")
        _lib.check(self.lib, self._handle, code, "op_loss")
        return (out, terms_out) if terms else out

    def forward_rows(self, rows: Sequence[Sequence[int]]) -> tuple[torch.Tensor, torch.Tensor, np.ndarray]:
        """Convenience: host id rows -> one H2D copy -> forward.  Returns (prune[T,2], rank[B,nl], cu_host)."""

        ids_np, cu_np, max_len = pack_rows(rows)
        self.check_ids(ids_np)
        ids = torch.from_numpy(ids_np).to(self.device, non_blocking=False)
        cu = torch.from_numpy(cu_np).to(self.device, non_blocking=False)
        prune, rank = self.forward_packed(ids, cu, cu_np, max_len, ids_host=ids_np)
        return prune, rank, cu_np

    # -- test / measurement hooks ------------------------------------------------------------------
    @contextmanager
    def capture_hidden(self) -> Iterator[None]:
        """While active, each forward also stores the N+1 hidden states; read :attr:`captured`."""

        self._capture = torch.empty(0)
        try:
            yield
        finally:
            self.lib.op_debug_capture_hidden(self._handle, None)
            self._capture_result = self._capture
            self._capture = None

    @property
    def captured(self) -> torch.Tensor:
        return self._capture_result

    def clock_probe(self, spin_us: int) -> "tuple[torch.Tensor, torch.cuda.Stream]":
        """Start a one-wave probe on a stream of its own that spins for ``spin_us`` microseconds beside whatever runs
        meanwhile; returns (uint64 tensor [shader cycles, 100 MHz ticks], its stream).  After synchronising that stream,
        ``cycles / ticks / 10`` = the shader clock in GHz the chip held (measurement hook: bench.py)."""

        with torch.cuda.device(self.device):
            side = torch.cuda.Stream(self.device)
            out = torch.zeros(2, dtype=torch.int64, device=self.device)
            side.wait_stream(torch.cuda.current_stream(self.device))
            code = self.lib.op_debug_clock_probe(self._handle, int(spin_us), ctypes.c_void_p(out.data_ptr()), ctypes.c_void_p(side.cuda_stream))
        _lib.check(self.lib, self._handle, code, "op_debug_clock_probe")
        return out, side

    def profile_enable(self, enabled: bool) -> None:
        _lib.check(self.lib, self._handle, self.lib.op_profile_enable(self._handle, 1 if enabled else 0), "profile")
        self._profiling = bool(enabled)

    def profile_reset(self) -> None:
        _lib.check(self.lib, self._handle, self.lib.op_profile_reset(self._handle), "profile_reset")

    def profile_read(self) -> dict[str, dict[str, float]]:
        """Kernel kind -> {launches, total_ms, avg_ms}; HIP events recorded on the launch stream."""

        entries = (_lib.OpProfileEntry * 32)()
        n = self.lib.op_profile_read(self._handle, entries, 32)
        if n < 0:
            _lib.check(self.lib, self._handle, n, "op_profile_read")
        out: dict[str, dict[str, float]] = {}
        for i in range(n):
            e = entries[i]
            name = self.lib.op_profile_kind_name(e.kind).decode()
            out[name] = {
                "launches": int(e.launches),
                "total_ms": float(e.total_ms),
                "avg_ms": float(e.total_ms) / max(int(e.launches), 1),
            }
        return out
