"""``OpenProvenceModel`` -- the drop-in for the reference's inference class on MI355X.

Same public surface as ``open_provence/modeling_open_provence_standalone.py`` (class, method and keyword
names, result keys, error behaviour) for the path BASELINE.json names:

* ``forward(input_ids, attention_mask, ...)``   ref: standalone.py:1666-1739
* ``process(question, context, ...)``           ref: standalone.py:3314-3808
* ``get_raw_predictions(_batch)`` / ``predict_with_thresholds``   ref: :1741-1881
* ``from_pretrained(path, device=, max_length=, torch_dtype=)``   ref: :1557-1664
* ``OpenProvenceForSequenceClassification`` / ``OpenProvenceForTokenClassification``  ref: :3814-3906

The arithmetic is NOT here: ``forward`` packs the batch and calls the C ABI
(``include/open_provence_hip.h``) through :class:`open_provence_amd.engine.HipEncoder`.  Without the HIP
library or without a GPU, construction raises -- there is no fallback.
"""

from __future__ import annotations

import contextlib
import functools
import itertools
import json
import logging
import os
import warnings
from collections.abc import Callable, Iterable, Mapping, Sequence
from dataclasses import dataclass
from pathlib import Path
from time import perf_counter
from typing import Any

import numpy as np
import torch

from . import launches, pipeline as pl, request as rq
from .config import DEFAULT_PROCESS_THRESHOLD, EncoderDims, OpenProvenceConfig
from .engine import (AttentionRequest, HiddenRequest, HipEncoder, check_arithmetic_arguments, check_attention_masks,
                     check_masked_kernels, require_gpu)
from .packing import pack_padded, pack_rows, unpack_to_padded
from .pipeline import ContextState, FragmentRecord, RawPrediction
from .prepared import PreparedContexts, PreparedItem, as_request as _as_prepared_request, derive_row_template
from .splitters import SentenceSplitter, resolve_sentence_splitter

LOGGER = logging.getLogger(__name__)
# As the reference (standalone.py:160), the Rust tokenizer's own thread pool is off unless the environment says otherwise.
# The parallelism of the split / tokenize stage is this module's worker threads, each encoding the sentences of a whole
# GROUP of contexts with one GIL-free `encode_batch` (pipeline.tokenize_sentence_groups): 4 threads without the pool
# measure 8.5 k / 10.9 k contexts/s at 1024 / 4096 contexts for 1.1 s of CPU time, the pool without threads 6.0-7.6 k /
# 7.2 k for 2.9 s (it spins on every core of the host), both together 6.1 k.
os.environ.setdefault("TOKENIZERS_PARALLELISM", "false")

DEFAULT_SPLITTER_LANGUAGE = "auto"
OpenProvenceRawPrediction = RawPrediction

_PROGRESS_BAR_ENABLED = True


def enable_progress_bar() -> None:
    global _PROGRESS_BAR_ENABLED
    _PROGRESS_BAR_ENABLED = True


def disable_progress_bar() -> None:
    global _PROGRESS_BAR_ENABLED
    _PROGRESS_BAR_ENABLED = False


def is_progress_bar_enabled() -> bool:
    return _PROGRESS_BAR_ENABLED


@dataclass(frozen=True)
class ProcessPerformanceTrace:
    """Stage timers returned by every ``process()`` call (ref: standalone.py:377-404).  Unlike the
    reference, ``inference_seconds`` is measured with a device synchronisation on both sides."""

    preprocess_seconds: float = 0.0
    assembly_seconds: float = 0.0
    inference_seconds: float = 0.0
    postprocess_seconds: float = 0.0
    total_seconds: float = 0.0
    sentence_collect_seconds: float = 0.0
    sentence_normalize_seconds: float = 0.0
    tokenize_seconds: float = 0.0
    fragment_split_seconds: float = 0.0
    fragment_decode_seconds: float = 0.0

    def as_dict(self) -> dict[str, Any]:
        """The reference's ten stage timers (ref :377-404) + the NUMERIC facts the MI355X path adds when it has something to
        say: ``fallback_from_f8`` (how often the range guard left an fp16-plane kernel set on this model), ``host_replicas``
        (host-stage worker processes of the call).  Callers do arithmetic over this dict (``float(v)``, sums over calls):
        everything in it is a number; the kernel set's NAME and the calibration report are ``performance_trace.runtime``."""

        out: dict[str, Any] = {name: float(getattr(self, name)) for name in self.__dataclass_fields__}
        out.update({k: v for k, v in (getattr(self, "runtime", None) or {}).items() if isinstance(v, (int, float)) and not isinstance(v, bool)})
        return out


_NO_PROBS = np.zeros(0, dtype=np.float32)


class OpenProvenceOutput(dict):
    """Forward result usable both as a Mapping and through attributes, exposing the reference's fields:
    ``logits`` (= ``ranking_logits``), ``ranking_logits``, ``pruning_logits``, ``loss``, ``hidden_states``; and this package's
    own reduced outputs ``pooled_hidden_states`` / ``attention_rows`` (None unless requested)."""

    def __getattr__(self, name: str) -> Any:
        try:
            return self[name]
        except KeyError as exc:
            raise AttributeError(name) from exc

    def __setattr__(self, name: str, value: Any) -> None:
        self[name] = value


def _precision_from_dtype(dtype: Any) -> str:
    """``torch_dtype`` of the reference API -> MFMA operand mode.  fp32 / None -> the parity-grade split
    mode; bf16 / fp16 -> single-pass bf16 operands (what those dtypes mean on the reference's GPU path)."""

    if dtype is None:
        return "bf16x3"
    if isinstance(dtype, torch.dtype):
        if dtype == torch.float32:
            return "bf16x3"
        if dtype in (torch.bfloat16, torch.float16):
            return "bf16"
        raise TypeError(f"Unsupported dtype value: {dtype!r}")
    text = str(dtype).strip().lower()
    if text in {"auto", "float32", "fp32", "32", "bf16x3"}:
        return "bf16x3"
    if text in {"bfloat16", "bf16", "float16", "fp16", "half"}:
        return "bf16"
    raise TypeError(f"Unsupported dtype value: {dtype!r}")


def _load_checkpoint_tensors(directory: Path) -> dict[str, torch.Tensor]:
    from safetensors.torch import load_file

    single = directory / "model.safetensors"
    if single.exists():
        return load_file(str(single))
    index = directory / "model.safetensors.index.json"
    if index.exists():
        with open(index, "r", encoding="utf-8") as handle:
            shards = sorted(set(json.load(handle)["weight_map"].values()))
        state: dict[str, torch.Tensor] = {}
        for shard in shards:
            state.update(load_file(str(directory / shard)))
        return state
    legacy = directory / "pytorch_model.bin"
    if legacy.exists():
        return torch.load(str(legacy), map_location="cpu", weights_only=True)
    raise FileNotFoundError(f"no model.safetensors / pytorch_model.bin under {directory}")


def resolve_pruning_hidden_state(config: OpenProvenceConfig, override: str | None = None) -> str:
    """Which hidden state the pruning head reads: ``"post_final_norm"`` or ``"pre_final_norm"``.

    The reference feeds ``outputs.hidden_states[-1]`` of the HF backbone to the head (standalone.py:1695).  Under
    transformers >= 5 that entry is tied to ``last_hidden_state`` = the ``final_norm`` output
    (utils/output_capturing.py:269-277); the 4.x line the reference pins (uv.lock: 4.57.1) appended the last layer's
    output BEFORE ``final_norm`` -- so a released checkpoint's head was trained on, and the reference under its own
    lock evaluates, the un-normalised state.  Order of precedence: the ``pruning_hidden_state`` argument, the config
    field of the same name (``save_pretrained`` always writes it, so the guess below runs at most once per checkpoint),
    then ``"auto"``, a HEURISTIC that is logged as a warning because it changes pruning logits by > 0.1:
    * the ``transformers_version`` HF wrote into config.json (major < 5 -> pre-norm).  That stamp names the environment
      that last SAVED the config, not the one that trained the head: a 4.x checkpoint re-saved through a 5.x config
      path flips -- pass ``pruning_hidden_state=`` explicitly for such files;
    * no stamp, config read from a checkpoint directory: pre-norm (the reference's lock is 4.57.1: released
      checkpoints were trained on the un-normalised state);
    * no stamp, config built in code: the installed transformers' behaviour (post-norm under >= 5 -- what the
      reference computes in this image -- else pre-norm)."""

    choice = override or getattr(config, "extra", {}).get("pruning_hidden_state") or "auto"
    if choice in ("post_final_norm", "pre_final_norm"):
        return choice
    if choice != "auto":
        raise ValueError("pruning_hidden_state must be 'auto', 'post_final_norm' or 'pre_final_norm'")
    version = str(getattr(config, "extra", {}).get("transformers_version") or "")
    try:
        major: int | None = int(version.split(".")[0])
    except ValueError:
        major = None
    if major is not None:
        resolved, why = ("pre_final_norm" if major < 5 else "post_final_norm"), f"config.json transformers_version={version}"
    elif getattr(config, "_from_file", False):
        resolved, why = "pre_final_norm", "checkpoint config without a transformers_version stamp (reference lock: 4.57.1)"
    else:
        try:
            import importlib.metadata as _md

            installed = int(_md.version("transformers").split(".")[0])
        except Exception:  # transformers absent: nothing to imitate
            installed = 5
        resolved = "pre_final_norm" if installed < 5 else "post_final_norm"
        why = f"config built in code, installed transformers major {installed}"
    LOGGER.warning("pruning_hidden_state='auto' resolved to %r (%s); pass pruning_hidden_state= or set it in config.json "
                   "to pin it", resolved, why)
    return resolved


class OpenProvenceModel:
    """Reranker + pruning head on hand-written gfx950 kernels, with the reference's public API."""

    config_class = OpenProvenceConfig

    # ------------------------------------------------------------------------------------------
    # construction
    # ------------------------------------------------------------------------------------------
    def __init__(
        self,
        config: OpenProvenceConfig,
        *,
        device: str | torch.device | None = None,
        tokenizer: Any | None = None,
        state_dict: Mapping[str, torch.Tensor] | None = None,
        precision: str | None = None,
        torch_dtype: Any | None = None,
        chunk_rows: int | None = None,
        pruning_hidden_state: str | None = None,
        kernel_set: str | None = None,
        calibrate: "bool | float | None" = None,
        calibration_rows: "Sequence[Sequence[int]] | None" = None,
        forward_token_budget: int | None = None,
        audit: "str | bool | None" = None,
        audit_every: int = 0,
        audit_tokens: int | None = None,
        calibration_reference: str | None = None,
        attention_outputs: bool = False,
        attention_masks: str = "prefix",
        masked_kernels: str = "fp32",
    ) -> None:
        # attention_outputs: keep the fp32 GEMM weights on the device so that forward(output_attentions=True) can run
        # (HipEncoder; nothing else changes);
        # attention_masks: "prefix" (right-padded masks only) or "any": forward() also takes left padding and holes, on the
        # fp32 kernels (HipEncoder.forward_masked; keeps the fp32 weights too) -- or, with masked_kernels="selected", on the
        # kernel set the packed forward runs on (row and panel path; no fp32 weights on the mask's account);
        # kernel_set / calibrate / calibration_rows: how the arithmetic is chosen from the loaded weights
        # (HipEncoder.load_state_dict; the reference's counterpart: standalone.py:219-244, 1589-1615);
        # calibration_reference: what a calibration compares with, "bf16x3" (default) or "fp32" (kernel set "fp32");
        # audit / audit_every / audit_tokens: how a calibrated choice is re-checked on real batches (audit.maybe_audit)
        kernel_set, calibration_reference = check_arithmetic_arguments(kernel_set, calibration_reference)
        attention_masks = check_attention_masks(attention_masks)
        masked_kernels = check_masked_kernels(masked_kernels)
        self._kernel_set_request = kernel_set
        self._calibrate_request = calibrate
        self._calibration_rows = calibration_rows
        self.config = config
        self.max_length = int(config.max_length)
        self.num_labels = int(config.num_labels)
        self.num_pruning_labels = int(config.num_pruning_labels)
        if self.num_pruning_labels != 2:
            raise ValueError("the pruning head has exactly 2 labels (keep / drop)")
        self.default_splitter_language = DEFAULT_SPLITTER_LANGUAGE
        try:
            self._runtime_device = require_gpu(self._normalize_device(device))
        except ValueError as exc:
            raise ValueError(f"Invalid device specification for {type(self).__name__}: {device!r}") from exc
        self.dims: EncoderDims = config.encoder_dims()
        head_hidden = int(config.pruning_config.get("hidden_size", self.dims.hidden_size))
        if head_hidden != self.dims.hidden_size:
            raise ValueError("pruning_config.hidden_size must equal the backbone hidden_size")
        self.precision = precision or _precision_from_dtype(torch_dtype)
        if chunk_rows is None and os.getenv("OPEN_PROVENCE_CHUNK_ROWS"):
            chunk_rows = int(os.environ["OPEN_PROVENCE_CHUNK_ROWS"])
        self.pruning_hidden_state = resolve_pruning_hidden_state(config, pruning_hidden_state)
        self.encoder = HipEncoder(
            self.dims, device=self._runtime_device, precision=self.precision, chunk_rows=chunk_rows,
            prune_pre_final_norm=self.pruning_hidden_state == "pre_final_norm",
            audit=audit, audit_every=audit_every, **({} if audit_tokens is None else {"audit_tokens": audit_tokens}),
            kernel_set=kernel_set, calibration_reference=calibration_reference, attention_outputs=attention_outputs,
            attention_masks=attention_masks, masked_kernels=masked_kernels,
        )
        if state_dict is not None:
            self.load_state_dict(state_dict)
        self.tokenizer = tokenizer if tokenizer is not None else self._init_tokenizer(config)
        self._manual_special_tokens_required = False
        self._manual_cls_token_id: int | None = None
        self._manual_sep_token_id: int | None = None
        self._update_tokenizer_runtime()
        self._update_runtime_defaults()
        self.default_threshold = self._resolve_default_threshold(config)
        self.forward_token_budget = forward_token_budget  # (None: OPEN_PROVENCE_FORWARD_TOKENS, else the device's default)

    # -- how many tokens process() puts into one forward (pipeline.plan_forward_chunks) ----------------------------------
    # One round of the chip is n_cus x ROW_BM rows: the whole-layer kernels run one 128-row block per CU, and a launch takes
    # one block period however few blocks it has -- so a forward costs about the same up to that many tokens, and the budget is
    # counted in such rounds (round_token_budget).  FORWARD_BUDGET_ROUNDS is the default (0 would be the fixed batch_size
    # stride): one round -- never slower than the stride in any measured workload, 20 - 27 % less inference_seconds where a granule
    # holds more than batch_size rows, and the only R that is not sometimes worse than a smaller one
    # (profiles/process_token_budget.txt).
    FORWARD_BUDGET_ROUNDS = 1
    FORWARD_ROUND_ROWS_PER_CU = 128

    @property
    def forward_token_budget(self) -> int:
        """Token budget of one forward of ``process()`` / ``get_raw_predictions_batch`` on the native path: chunks of
        ``batch_size`` rows are coalesced while their padded tokens fit (``pipeline.plan_forward_chunks``); 0 = the fixed
        ``batch_size`` stride of the reference.  A row's outputs do not depend on its companions, so results do not change."""

        value = self.__dict__.get("_forward_token_budget")
        if value is None:
            value = self.__dict__["_forward_token_budget"] = self._default_forward_token_budget()
        return value

    @forward_token_budget.setter
    def forward_token_budget(self, value: int | None) -> None:
        if value is None:  # OPEN_PROVENCE_FORWARD_TOKENS, else the device's default
            self.__dict__["_forward_token_budget"] = self._default_forward_token_budget()
            return
        if isinstance(value, bool) or not isinstance(value, (int, np.integer)):
            raise ValueError(f"forward_token_budget must be a non-negative integer, got {value!r}")
        if value < 0:
            raise ValueError(f"forward_token_budget must be >= 0 (0 = the fixed batch_size stride), got {value!r}")
        self.__dict__["_forward_token_budget"] = int(value)

    def round_token_budget(self, rounds: int = 1) -> int:
        """``rounds`` rounds of the model's device in tokens (``n_cus`` x 128 each); 0 without a device."""

        dev = getattr(self, "_runtime_device", None)
        if isinstance(dev, torch.device) and dev.type == "cuda" and torch.cuda.is_available():
            n_cus = int(torch.cuda.get_device_properties(dev).multi_processor_count)
            return int(rounds) * n_cus * self.FORWARD_ROUND_ROWS_PER_CU
        return 0

    def _default_forward_token_budget(self) -> int:
        text = os.environ.get("OPEN_PROVENCE_FORWARD_TOKENS", "").strip()
        if text:
            try:
                value = int(text)
            except ValueError:
                raise ValueError(f"OPEN_PROVENCE_FORWARD_TOKENS must be a non-negative integer, got {text!r}") from None
            if value < 0:
                raise ValueError(f"OPEN_PROVENCE_FORWARD_TOKENS must be >= 0, got {text!r}")
            return value
        # (no device -- a model whose forward was replaced, which keeps the fixed stride anyway -- gives 0)
        return self.round_token_budget(self.FORWARD_BUDGET_ROUNDS) if self.FORWARD_BUDGET_ROUNDS else 0

    @staticmethod
    def _normalize_device(device: str | torch.device | None) -> torch.device | None:
        if device is None or isinstance(device, torch.device):
            return device
        text = str(device).strip().lower()
        if not text or text == "auto":
            return None
        if text.startswith("cuda"):
            return torch.device(text)
        if text == "cpu" or text.startswith("mps"):
            raise ValueError(f"{device!r}: the MI355X path has no CPU/MPS implementation")
        raise ValueError(f"Unsupported device specification: {device!r}")

    def _init_tokenizer(self, config: OpenProvenceConfig) -> Any:
        reference = config.tokenizer_name_or_path or config._name_or_path or config.base_model_name_or_path
        if not reference:
            raise ValueError("Unable to determine tokenizer reference for OpenProvence model.")
        try:
            from transformers import AutoTokenizer  # text front-end only; never on the arithmetic path

            return AutoTokenizer.from_pretrained(reference)
        except Exception as exc:
            raise RuntimeError(f"Failed to initialize tokenizer from '{reference}'.") from exc

    def _update_tokenizer_runtime(self, max_length_override: int | None = None) -> None:
        """Lift the tokenizer's model_max_length so sentence pre-tokenisation never truncates (ref :1391-1399)."""

        if self.tokenizer is None:
            return
        upper = max(getattr(self.tokenizer, "model_max_length", 0) or 0, 1_000_000)
        if max_length_override is not None and max_length_override > 0:
            upper = max(upper, int(max_length_override))
        elif self.max_length and self.max_length > 0:
            upper = max(upper, int(self.max_length))
        try:
            self.tokenizer.model_max_length = upper
        except Exception:  # pragma: no cover - exotic tokenizer objects
            pass

    def _update_runtime_defaults(self) -> None:
        self._manual_special_tokens_required = pl.requires_manual_special_tokens(self.tokenizer)
        if self._manual_special_tokens_required:
            cls_c, sep_c = pl.special_token_candidates(self.tokenizer)
            self._manual_cls_token_id = cls_c[0] if cls_c else None
            self._manual_sep_token_id = sep_c[0] if sep_c else None
        else:
            self._manual_cls_token_id = None
            self._manual_sep_token_id = None

    def _resolve_default_threshold(self, config: OpenProvenceConfig) -> float:
        value = getattr(config, "default_threadshold", None)
        if value is None:
            return DEFAULT_PROCESS_THRESHOLD
        try:
            return float(value)
        except (TypeError, ValueError) as exc:
            raise TypeError("OpenProvenceConfig.default_threadshold must be numeric when provided.") from exc

    def _resolve_process_threshold(self, threshold: float | None) -> float:
        resolved = threshold
        if resolved is None:
            resolved = getattr(self, "default_threshold", DEFAULT_PROCESS_THRESHOLD)
            if resolved is None:
                resolved = DEFAULT_PROCESS_THRESHOLD
        try:
            return float(resolved)
        except (TypeError, ValueError) as exc:
            raise TypeError("Resolved threshold must be numeric.") from exc

    # nn.Module-flavoured no-ops so that calling code written for the reference keeps working
    def eval(self) -> "OpenProvenceModel":
        return self

    def to(self, *args: Any, **kwargs: Any) -> "OpenProvenceModel":
        target = kwargs.get("device", args[0] if args else None)
        if target is not None and not isinstance(target, torch.dtype):
            resolved = require_gpu(self._normalize_device(target))
            if resolved != self._runtime_device:
                raise NotImplementedError("moving a loaded model between GPUs is not supported; reload on the target device")
        return self

    @property
    def device(self) -> torch.device:
        return self._runtime_device

    @staticmethod
    def _convert_legacy_state_dict(state_dict: Mapping[str, torch.Tensor]) -> Mapping[str, torch.Tensor]:
        """Checkpoints saved without the ``ranking_model.`` prefix are re-prefixed (ref :1452-1464)."""

        if any(key.startswith("ranking_model.") for key in state_dict):
            return state_dict
        return {(k if k.startswith("pruning_head.") else f"ranking_model.{k}"): v for k, v in state_dict.items()}

    def load_state_dict(self, state_dict: Mapping[str, torch.Tensor], strict: bool = True) -> None:
        converted = self._convert_legacy_state_dict(state_dict)
        self.encoder.load_state_dict(converted, kernel_set=getattr(self, "_kernel_set_request", None),
                                     calibrate=getattr(self, "_calibrate_request", None),
                                     calibration_rows=getattr(self, "_calibration_rows", None))
        # The device library keeps only its re-packed copies; the original tensors are retained on the host (by
        # reference when they already live there) so that state_dict() / save_pretrained() work like the reference's.
        self._weights = {
            key: value.detach().to("cpu") for key, value in converted.items() if "inv_freq" not in key
        }

    def state_dict(self) -> dict[str, torch.Tensor]:
        """Checkpoint tensors under the reference's keys (``ranking_model.*``, ``pruning_head.*``; ref :1452-1464)."""

        weights = getattr(self, "_weights", None)
        if weights is None:
            raise RuntimeError("no weights have been loaded into this model")
        return dict(weights)

    def save_pretrained(self, save_directory: str | Path, *, safe_serialization: bool = True) -> None:
        """Write a checkpoint directory in the reference's format (writer: encoder.py:1040-1094; reader:
        standalone.py:1557-1664 and :func:`from_pretrained` here): ``config.json`` with the OpenProvence fields plus
        ``architectures`` / ``auto_map`` / ``vocab_size`` / ``hidden_size``, ``model.safetensors`` with the prefixed
        tensors, the tokenizer's own files, and -- where the reference copies its standalone modeling file for
        ``AutoModel.from_pretrained(dir, trust_remote_code=True)`` -- a freshly written module of the same name that
        re-exports THIS implementation (open_provence_amd/hf_auto.py)."""

        directory = Path(save_directory)
        directory.mkdir(parents=True, exist_ok=True)
        state = {key: value.contiguous() for key, value in self.state_dict().items()}
        payload = self.config.to_dict()
        base = payload.get("base_model_config") or {}
        payload["max_length"] = int(self.max_length)
        payload["num_labels"] = int(self.num_labels)
        payload["num_pruning_labels"] = 2
        payload.setdefault("mode", "reranking_pruning")
        if payload.get("encoder_architecture") is None:
            payload["encoder_architecture"] = base.get("model_type")
        payload["vocab_size"] = base.get("vocab_size", self.dims.vocab_size)
        payload["hidden_size"] = base.get("hidden_size", self.dims.hidden_size)
        payload["architectures"] = ["OpenProvenceForSequenceClassification"]
        payload["pruning_hidden_state"] = self.pruning_hidden_state  # explicit: no transformers-version guess on reload
        module = "modeling_open_provence_standalone"
        payload["auto_map"] = {
            "AutoConfig": f"{module}.OpenProvenceConfig",
            "AutoModel": f"{module}.OpenProvenceForSequenceClassification",
            "AutoModelForSequenceClassification": f"{module}.OpenProvenceForSequenceClassification",
            "AutoModelForTokenClassification": f"{module}.OpenProvenceForTokenClassification",
        }
        with open(directory / "config.json", "w", encoding="utf-8") as handle:
            json.dump(payload, handle, indent=2, sort_keys=True)
        if safe_serialization:
            from safetensors.torch import save_file

            save_file(state, str(directory / "model.safetensors"))
        else:
            torch.save(state, str(directory / "pytorch_model.bin"))
        saver = getattr(self.tokenizer, "save_pretrained", None)
        if callable(saver):
            saver(str(directory))
        (directory / "modeling_open_provence_standalone.py").write_text(_remote_code_shim_source(), encoding="utf-8")

    @classmethod
    def from_pretrained(
        cls,
        pretrained_model_name_or_path: str | Path,
        *,
        device: str | torch.device | None = None,
        trust_remote_code: bool = True,
        max_length: int | None = None,
        torch_dtype: torch.dtype | str | None = None,
        tokenizer: Any | None = None,
        **kwargs: Any,
    ) -> "OpenProvenceModel":
        """Load ``config.json`` + ``model.safetensors`` (+ tokenizer files) from a local checkpoint directory
        in the reference's format (ref: encoder.py:1040-1094).  There is no network in this build: hub ids
        must already be materialised on disk."""

        directory = Path(pretrained_model_name_or_path)
        if not directory.is_dir():
            raise FileNotFoundError(
                f"{pretrained_model_name_or_path!r} is not a local checkpoint directory (hub download is unavailable)"
            )
        auto_config = kwargs.pop("config", None)  # AutoModel.from_pretrained passes the AutoConfig result along
        if auto_config is not None and hasattr(auto_config, "to_native"):
            config = auto_config.to_native()
        elif isinstance(auto_config, OpenProvenceConfig):
            config = auto_config
        else:
            config = OpenProvenceConfig.from_json_file(directory / "config.json")
        config._name_or_path = str(directory)
        config._from_file = True  # every route here reads a checkpoint's config.json (resolve_pruning_hidden_state)
        if "dtype" in kwargs and torch_dtype is None:
            torch_dtype = kwargs.pop("dtype")
        # HF plumbing the Auto* factories add; the HIP attention kernel is the only attention implementation
        for hf_only in ("attn_implementation", "_from_auto", "adapter_kwargs", "cache_dir", "force_download", "local_files_only",
                        "proxies", "revision", "subfolder", "token", "code_revision", "_commit_hash", "low_cpu_mem_usage",
                        "device_map", "quantization_config"):
            kwargs.pop(hf_only, None)
        if max_length is not None:
            config.max_length = int(max_length)
        state = _load_checkpoint_tensors(directory)
        model = cls(
            config,
            device=device,
            tokenizer=tokenizer,
            state_dict=state,
            torch_dtype=torch_dtype,
            precision=kwargs.pop("precision", None),
            chunk_rows=kwargs.pop("chunk_rows", None),
            pruning_hidden_state=kwargs.pop("pruning_hidden_state", None),
            kernel_set=kwargs.pop("kernel_set", None),
            calibrate=kwargs.pop("calibrate", None),
            calibration_rows=kwargs.pop("calibration_rows", None),
            forward_token_budget=kwargs.pop("forward_token_budget", None),
            audit=kwargs.pop("audit", None),
            audit_every=kwargs.pop("audit_every", 0),
            audit_tokens=kwargs.pop("audit_tokens", None),
            calibration_reference=kwargs.pop("calibration_reference", None),
            attention_outputs=bool(kwargs.pop("attention_outputs", False)),
            attention_masks=kwargs.pop("attention_masks", "prefix"),
            masked_kernels=kwargs.pop("masked_kernels", "fp32"),
        )
        if max_length is not None:
            model.max_length = int(max_length)
        model._update_tokenizer_runtime(max_length_override=max_length)
        model._update_runtime_defaults()
        return model

    # ------------------------------------------------------------------------------------------
    # forward boundary
    # ------------------------------------------------------------------------------------------
    @staticmethod
    def _extract_model_output(outputs: Any, key: str) -> torch.Tensor:
        """``key`` of a forward result that may be a Mapping or an attribute bag (the boundary contract of
        standalone.py:1540-1555: the reference's tests replace ``forward`` by a plain dict); ``logits`` stands in for
        ``ranking_logits``."""

        names = (key, "logits") if key == "ranking_logits" else (key,)
        for name in names:
            value = outputs.get(name) if isinstance(outputs, Mapping) else None
            if value is None:
                value = getattr(outputs, name, None)
            if value is not None:
                return value
        raise KeyError(f"{key} not found in model outputs")

    def forward(
        self,
        input_ids: torch.Tensor | None = None,
        attention_mask: torch.Tensor | None = None,
        labels: torch.Tensor | None = None,
        return_dict: bool | None = None,
        output_hidden_states: bool | None = None,
        output_attentions: bool | None = None,
        pooled_hidden_states: str | None = None,
        attention_rows: "str | torch.Tensor | None" = None,
        attention_rows_reduce_heads: bool = False,
        **kwargs: Any,
    ) -> OpenProvenceOutput | tuple[torch.Tensor, ...]:
        """``input_ids[B, L]`` (+ right-padded ``attention_mask``) -> ``ranking_logits[B, nl]`` and
        ``pruning_logits[B, L, 2]`` (fp32, on the GPU; zeros at padding positions).  ``token_type_ids`` and
        other HF kwargs are accepted and ignored, as ModernBERT ignores them.

        ``output_hidden_states=True``: ``hidden_states`` is a tuple of num_layers + 1 fp32 tensors ``[B, L, H]`` (zeros at
        padding positions) as the reference returns them (standalone.py:1689, 1727): the embedding LayerNorm output, the
        output of every layer, and last the pruning head's input (``final_norm`` output, or the raw last layer under
        ``prune_pre_final_norm``).  They are views of one device buffer ``[N + 1, B, L, H]`` that the forward's own
        kernels write; the logits are bit-identical to those of the same call without the flag.

        ``output_attentions=True`` (a model created with ``attention_outputs=True``; ``ValueError`` otherwise): ``attentions``
        is a tuple of num_layers fp32 tensors ``[B, heads, L, L]`` as the reference returns them under eager attention
        (standalone.py:1689, 1727) -- except that padded QUERY rows are zeros here, where the reference holds a softmax row.
        A side pass over the hidden states (``op_attention_probs``): logits and hidden states are bit-identical to those of
        the same call without the flag.  Memory: ``num_layers x B x heads x L^2 x 4`` bytes.

        ``pooled_hidden_states="first" | "mean"`` (no counterpart in the reference): ``pooled_hidden_states`` is one fp32 tensor
        ``[num_layers + 1, B, H]`` -- per entry of ``hidden_states`` the row of token 0 of each sequence (bit-identical to it) or
        the mean over the sequence's tokens (fp64 in a fixed order, rounded once; a row of zeros for an empty sequence) --
        reduced on the device from one scratch entry (``op_forward_packed_pooled``): ``(N + 1) x B x H x 4`` bytes instead of
        ``(N + 1) x B x L x H x 4``.  ``attention_rows="first"`` or an integer tensor ``[B]`` of query positions (a model created
        with ``attention_outputs=True``; ``ValueError`` otherwise): ``attention_rows`` is a tuple of num_layers fp32 tensors
        ``[B, heads, L]``, the selected query's row of ``attentions`` bit for bit, or with ``attention_rows_reduce_heads=True``
        ``[B, L]``, its mean over heads (``op_attention_rows``).  Both may be combined with the two flags above; logits are
        bit-identical with or without them.

        ``labels``: ``loss`` is the reference's evaluation loss of the ranking head (standalone.py:1707-1722) as a 0-dim fp32
        device tensor -- ``BCEWithLogitsLoss`` on ``labels.float()`` when ``num_labels == 1``, otherwise ``CrossEntropyLoss``
        on integer ``labels.view(-1)`` -- computed by ``op_loss`` over the ranking logits the forward left on the device (fp64
        terms, fixed-order sum: within 1 fp32 ulp of the exact mean).  ``labels`` holds one entry per row (``ValueError``
        otherwise) on the CPU or on the device; a class outside ``0 <= y < num_labels`` that is not -100 raises ``IndexError``.
        Every other output is bit-identical to the same call without labels; ``return_dict=False`` then returns
        ``(loss, ranking_logits, pruning_logits)``."""

        if input_ids is None:
            raise ValueError("input_ids must be provided")
        rank_labels = self._ranking_labels(labels, int(input_ids.shape[0])) if labels is not None else None
        reduced: dict[str, Any] = {}
        rank, pruning_logits, hidden_states, attentions, _ = self._forward_padded(
            input_ids, attention_mask, output_hidden_states, output_attentions,
            reduced=self._reduced_requests(pooled_hidden_states, attention_rows, attention_rows_reduce_heads, reduced))
        loss = None
        if rank_labels is not None:
            loss = self.encoder.loss("rank_bce" if rank.shape[1] == 1 else "rank_ce", rank, rank_labels)
        if return_dict is not None and not return_dict:
            return (rank, pruning_logits) if loss is None else (loss, rank, pruning_logits)
        return OpenProvenceOutput(
            loss=loss, logits=rank, ranking_logits=rank, pruning_logits=pruning_logits, hidden_states=hidden_states,
            attentions=attentions, pooled_hidden_states=reduced.get("pooled_hidden_states"), attention_rows=reduced.get("attention_rows"),
        )

    def _reduced_requests(self, pooled_hidden_states, attention_rows, reduce_heads, results: "dict[str, Any]") -> "dict[str, Any] | None":
        """The ``reduced`` argument of :meth:`_forward_padded` for forward()'s three keywords (None: none of them is set);
        ``results`` receives ``pooled_hidden_states`` / ``attention_rows``."""

        if pooled_hidden_states is None and attention_rows is None:
            if reduce_heads:
                raise ValueError("attention_rows_reduce_heads=True needs attention_rows")
            return None
        if attention_rows is not None and not self.encoder.attention_outputs:
            raise ValueError("attention_rows needs the fp32 weight packs: create the model with attention_outputs=True")
        return {"pool": pooled_hidden_states, "query": attention_rows, "reduce_heads": bool(reduce_heads), "results": results}

    def _ranking_labels(self, labels: torch.Tensor, n_rows: int) -> torch.Tensor:
        """``labels`` as the ranking loss reads them (standalone.py:1711, 1715), on the model's device: ``[B]`` fp32 for one
        label, ``[B]`` integer classes otherwise."""

        labels = torch.as_tensor(labels)
        if labels.numel() != n_rows:
            raise ValueError(f"labels must hold one entry per row: {labels.numel()} entries for {n_rows} rows")
        labels = labels.detach().reshape(-1).to(self._runtime_device)
        if int(self.dims.num_labels) == 1:
            return labels.float()
        if labels.dtype.is_floating_point or labels.dtype.is_complex or labels.dtype == torch.bool:
            raise TypeError(f"class labels must be an integer tensor, got {labels.dtype}")
        return labels

    def _forward_padded(self, input_ids, attention_mask, output_hidden_states, output_attentions, reduced=None, token_loss=False):
        """The forward of a padded batch without its losses: ``(ranking_logits, pruning_logits, hidden_states, attentions,
        packed)``; ``packed`` = the pruning logits as the kernels left them, ``[T, 2]`` on the device, with the batch's
        ``cu_seqlens`` on the device and the token count -- what the token-classification loss reads.  ``reduced``
        (:meth:`_reduced_requests`): the pooled hidden states and / or attention rows go into its ``results``.

        On a model created with ``attention_masks="any"`` a batch with a row that is not ones-then-zeros goes through
        :meth:`HipEncoder.forward_masked` (``packed`` is then None); a prefix-mask batch takes the packed path as ever.
        ``token_loss``: the caller wants ``packed`` for the token-classification loss."""

        if output_attentions and not self.encoder.attention_outputs:
            raise ValueError("output_attentions=True needs the fp32 weight packs: create the model with attention_outputs=True")
        dev = self._runtime_device
        # A batch that already lives on the model's GPU is packed, checked and (below) unpacked there by HIP kernels
        # (op_pack_padded / op_unpack_padded: same results, same errors); CPU tensors, and tensors of another GPU, go through
        # the host as before.
        on_device = (dev.type == "cuda" and isinstance(input_ids, torch.Tensor) and input_ids.device == dev
                     and (attention_mask is None or (isinstance(attention_mask, torch.Tensor) and attention_mask.device == dev)))
        ids_np = None  # (a device-resident batch has no host copy: the running audit scans it on the device)
        any_mask = attention_mask is not None and getattr(self.encoder, "attention_masks", "prefix") == "any"
        if on_device:
            # (op_pack_padded's one synchronisation reports the mask's shape too: no second round trip decides the route)
            packed_batch = (self.encoder._pack_padded_device(input_ids, attention_mask, non_prefix_ok=True) if any_mask
                            else self.encoder.pack_padded_device(input_ids, attention_mask))
            if packed_batch is None:
                return self._forward_any_mask(input_ids, attention_mask, output_hidden_states, output_attentions, reduced, token_loss)
            ids, cu, cu_np, max_len = packed_batch
        else:
            try:
                ids_np, cu_np, max_len = pack_padded(input_ids, attention_mask)
            except NotImplementedError:  # (a row that is not ones-then-zeros)
                if not any_mask:
                    raise
                return self._forward_any_mask(input_ids, attention_mask, output_hidden_states, output_attentions, reduced, token_loss)
            self.encoder.check_ids(ids_np)
            ids = torch.from_numpy(ids_np).to(dev)
            cu = torch.from_numpy(cu_np).to(dev)
        width = int(input_ids.shape[1])
        # (the fp16 + e4m3 kernel sets are range-guarded: a non-finite result is repeated on the (hi, lo) bf16 sets)
        hidden_states = attentions = None
        requests: dict[str, Any] = {}
        if output_hidden_states:
            requests["hidden"] = HiddenRequest(dtype=torch.float32, pad_width=width)
        rows_request = self._attention_rows_request(reduced, width, int(cu_np.shape[0]) - 1)
        if output_attentions:
            requests["attentions"] = AttentionRequest(pad_width=width)
        elif rows_request is not None:  # (beside the whole matrices: a pass of its own, below)
            requests["attentions"] = rows_request
        if reduced is not None and reduced["pool"] is not None:
            requests["pooled"] = HiddenRequest(pool=reduced["pool"])
        prune, rank, *extra = self.encoder.forward_packed_checked(ids, cu, cu_np, max_len, ids_host=ids_np, **requests)
        if output_attentions:
            attentions = tuple(extra.pop())
            if rows_request is not None:
                *_, rows = self.encoder.forward_packed_checked(ids, cu, cu_np, max_len, ids_host=ids_np, attentions=rows_request)
                reduced["results"]["attention_rows"] = tuple(rows)
        elif rows_request is not None:
            reduced["results"]["attention_rows"] = tuple(extra.pop())
        if "pooled" in requests:
            reduced["results"]["pooled_hidden_states"] = extra.pop()
        if output_hidden_states:
            hidden = extra.pop()
            # ([N + 1, B, L, H]; with L = 0 the request is packed and empty: the same shape, no data)
            hidden_states = tuple(hidden.reshape(hidden.shape[0], int(input_ids.shape[0]), width, hidden.shape[-1]).unbind(0))
        if on_device:
            pruning_logits = self.encoder.unpack_padded_device(prune, cu, int(input_ids.shape[0]), width)
        else:
            pruning_logits = unpack_to_padded(prune, cu_np, width)
        return rank, pruning_logits, hidden_states, attentions, (prune, cu, int(cu_np[-1]))

    def _forward_any_mask(self, input_ids, attention_mask, output_hidden_states, output_attentions, reduced, token_loss):
        """:meth:`_forward_padded` for a batch with a non-prefix row, on a model created with ``attention_masks="any"``: the
        dense forward on the fp32 kernels, or on the selected kernel set (``masked_kernels="selected"``).  The requests it does not serve yet raise ``NotImplementedError`` by name."""

        requested = [name for name, on in (
            ("output_hidden_states", output_hidden_states), ("output_attentions", output_attentions),
            ("attention_rows", reduced is not None and reduced["query"] is not None),
            ("pooled_hidden_states", reduced is not None and reduced["pool"] is not None),
            ("the token-classification loss (labels)", token_loss)) if on]
        if requested:
            raise NotImplementedError(
                f"{', '.join(requested)}: not available for an attention_mask that is not right-padded (ones then zeros); "
                "forward() serves the logits and the ranking loss for such a batch")
        prune, rank = self.encoder.forward_masked(input_ids, attention_mask)
        return rank, prune, None, None, None

    @staticmethod
    def _attention_rows_request(reduced, width: int, n_rows: int) -> "AttentionRequest | None":
        """forward(attention_rows=...) as the encoder's request: every layer, one query row per sequence."""

        if reduced is None or reduced["query"] is None:
            return None
        query = reduced["query"]
        if not isinstance(query, str):
            query = torch.as_tensor(query)
            if query.ndim != 1 or query.numel() != n_rows:
                raise ValueError(f"attention_rows must be 'first' or hold one query position per row ({n_rows})")
        return AttentionRequest(pad_width=width, query=query, reduce_heads=reduced["reduce_heads"])

    def __call__(self, *args: Any, **kwargs: Any):
        return self.forward(*args, **kwargs)

    @classmethod
    def register_for_auto_class(cls, auto_class: Any = "AutoModel") -> None:
        """``AutoModel.from_pretrained(..., trust_remote_code=True)`` calls this on the class it resolved through
        ``auto_map`` (transformers auto_factory); the HIP classes keep no per-class registry."""

        cls._auto_class = getattr(auto_class, "__name__", auto_class)

    def _forward_is_native(self) -> bool:
        """True unless ``forward`` was overridden / monkeypatched (the reference's tests do that, and the
        boundary must keep accepting any Mapping-returning replacement: tests/test_modeling_open_provence.py:940-949)."""

        if "forward" in self.__dict__:
            return False
        return type(self).forward in (
            OpenProvenceModel.forward,
            OpenProvenceForSequenceClassification.forward,
        )

    # -- host-stage replicas (frontend.py, mode="host"): process() without a GPU, forwards run by the owner's process -----
    def _host_stage_spec(self) -> dict[str, Any]:
        """What a replica needs to run the host stages of ``process()`` exactly as this model does (picklable)."""

        dims = getattr(self, "dims", None)
        return {
            "tokenizer": self.tokenizer,
            "tokenizer_model_max_length": getattr(self.tokenizer, "model_max_length", None),
            "max_length": int(self.max_length),
            "default_threshold": getattr(self, "default_threshold", DEFAULT_PROCESS_THRESHOLD),
            "default_splitter_language": getattr(self, "default_splitter_language", DEFAULT_SPLITTER_LANGUAGE),
            "manual": (self._manual_special_tokens_required, self._manual_cls_token_id, self._manual_sep_token_id),
            "vocab_size": int(dims.vocab_size) if dims is not None else None,
            "num_labels": int(getattr(dims, "num_labels", 0) or getattr(self, "num_labels", 1) or 1),
            "forward_token_budget": int(self.forward_token_budget),  # replicas plan their forwards as the owner would
        }

    @classmethod
    def _host_stage_replica(cls, spec: Mapping[str, Any], remote_forward: Any) -> "OpenProvenceModel":
        """A model object with the tokenizer and the request-level settings of ``spec`` and NO encoder: it splits,
        tokenizes, assembles and post-processes; every forward goes through ``remote_forward`` (``submit`` / ``result``) to
        the process that owns the GPU.  It cannot compute a forward by itself -- there is no CPU arithmetic path."""

        model = cls.__new__(cls)
        model.tokenizer = spec["tokenizer"] if spec.get("tokenizer") is not None else spec["tokenizer_factory"]()
        if spec.get("tokenizer_model_max_length") is not None:
            try:
                model.tokenizer.model_max_length = spec["tokenizer_model_max_length"]
            except Exception:  # pragma: no cover - exotic tokenizer objects
                pass
        model.max_length = int(spec["max_length"])
        model.num_labels = int(spec["num_labels"])
        model._runtime_device = torch.device("cpu")
        model.default_threshold = spec["default_threshold"]
        model.default_splitter_language = spec["default_splitter_language"]
        model._manual_special_tokens_required, model._manual_cls_token_id, model._manual_sep_token_id = spec["manual"]
        model._remote_forward = remote_forward
        model._dist = None
        model.forward_token_budget = int(spec.get("forward_token_budget", 0))
        return model

    # -- data parallelism over (query, block) rows -----------------------------------
    def attach_process_group(self, group: Any | None = None, *, dst: int = 0, enabled: bool = True,
                             single_rank_gather: bool = False, shard: str = "jobs") -> None:
        """Shard every forward batch of ``process()`` / ``get_raw_predictions_batch`` over the ranks of a
        ``torch.distributed`` process group (backend "nccl" = RCCL over xGMI with one process per GPU; "gloo" in the
        CPU tests).  Every rank calls ``process()`` with the SAME arguments; each runs its token-balanced share of the
        rows (full weight replica per GPU, no data-path collective), ONE gather moves the keep-probabilities
        (4 B per token) + ranking logits to rank ``dst``, which post-processes and returns the result; the other
        ranks' ``process()`` returns ``None``.  The reference has no multi-GPU path (its jobs are independent:
        standalone.py:2748-2756).  The pipelined path of ``process()`` stays in force: every rank enqueues its share
        asynchronously (pinned staging, on-device fragment means) and the gather moves 4 bytes per FRAGMENT.
        ``single_rank_gather`` (test hook): run the sharded code path on a one-rank group as well.

        ``shard`` selects what ``process()`` divides among the ranks:

        * ``"jobs"`` (default): the (query, context) JOBS.  Every rank splits, tokenizes, assembles, runs and
          post-processes only its own contexts (deterministic cost-balanced assignment, ``pipeline.assign_jobs``) through
          the plain single-GPU pipeline, and ONE ``gather_object`` at the end moves the per-context results to ``dst``:
          the host stages -- most of the time of a call with short contexts -- scale with the ranks too.
        * ``"rows"``: every rank runs the whole host pipeline and only the forward batches are divided (as described
          above).  ``get_raw_predictions_batch`` always shards rows.

        Every rank must hold the same ``forward_token_budget``: the ranks derive the chunks of a row-sharded call from it and
        would mismatch their collectives otherwise.  ``round_token_budget()`` is ``n_cus`` x 128 of each rank's own device:
        on a node of unlike GPUs set one explicit number on every rank."""

        import torch.distributed as dist

        if not enabled:
            self._dist = None
            return
        if not dist.is_available() or not dist.is_initialized():
            raise RuntimeError("attach_process_group needs an initialised torch.distributed process group")
        if shard not in ("jobs", "rows"):
            raise ValueError("shard must be 'jobs' or 'rows'")
        self._dist = {"group": group, "dst": int(dst), "rank": dist.get_rank(group), "world": dist.get_world_size(group),
                      "force": bool(single_rank_gather), "shard": shard, "local_only": False}
        # one arithmetic per job: the ranks compare their load-time kernel sets now, and audit a calibrated set TOGETHER on
        # the head of the first request (sharding.collective_audit) instead of each on its own shard
        encoder = getattr(self, "encoder", None)
        if encoder is not None and self._dist["world"] > 1 and self._forward_is_native():
            from .sharding import agree_on_kernel_set

            encoder.audit_collective = True
            agree_on_kernel_set(encoder, group)

    def _audit_rows_of_request(self, queries: Any, contexts: Any, limit: int = 8) -> list[list[int]]:
        """Token rows for a collective audit from the head of a ``process()`` request: the first query against its first
        ``limit`` contexts, through the tokenizer's own pair encoding (truncated to ``max_length``).  Every rank of a job-
        sharded call holds the whole request, so every rank builds the same rows."""

        try:
            query = queries[0] if isinstance(queries, (list, tuple)) else queries
            first = contexts[0] if contexts and isinstance(contexts[0], (list, tuple)) else contexts
            texts = []
            for ctx in list(first)[:limit]:
                texts.append(" ".join(str(t) for t in ctx) if isinstance(ctx, (list, tuple)) else str(ctx))
            rows = [list(self.tokenizer(str(query), text, truncation=True, max_length=int(self.max_length))["input_ids"]) for text in texts]
            return [r for r in rows if r]
        except Exception:  # (an exotic tokenizer / request shape: no audit rows -- the same on every rank)
            return []

    def _predict_rows(self, rows: list[list[int]], type_rows: list[list[int]] | None) -> tuple[torch.Tensor, list[np.ndarray]]:
        """Rows of token ids -> (ranking_logits[B, nl] fp32 CPU, per-row keep probabilities fp32); sharded over the
        attached process group when there is one (non-root ranks get zero-filled placeholders: their ``process()``
        result is discarded)."""

        info = getattr(self, "_dist", None)
        if not info or info["world"] <= 1 or info.get("local_only"):
            return self._predict_rows_local(rows, type_rows)
        import torch.distributed as dist

        from .sharding import ShardPlan

        if self._forward_is_native() and self.encoder.audit_pending:  # (the same state on every rank: every rank enters or none)
            from .sharding import collective_audit

            collective_audit(self.encoder, rows[: min(len(rows), 32)], info["group"])
        lengths = [len(r) for r in rows]
        nl = int(getattr(getattr(self, "dims", None), "num_labels", 0) or getattr(getattr(self, "config", None), "num_labels", 1) or 1)
        plan = ShardPlan(lengths, info["world"], width=1, num_labels=nl)
        mine = plan.local_rows(info["rank"])
        local_rank, local_keeps = self._predict_rows_local(
            [rows[i] for i in mine], [type_rows[i] for i in mine] if type_rows else None
        ) if mine else (torch.zeros((0, nl), dtype=torch.float32), [])
        backend = dist.get_backend(info["group"])
        comm_device = self._runtime_device if backend == "nccl" else torch.device("cpu")
        keep_flat = np.concatenate([np.asarray(k[: lengths[i]], dtype=np.float32) for k, i in zip(local_keeps, mine)]) if mine else np.zeros(0, np.float32)
        gathered = plan.gather(
            torch.from_numpy(np.ascontiguousarray(keep_flat)).to(comm_device),
            local_rank.to(torch.float32).reshape(len(mine), nl).to(comm_device),
            dst=info["dst"], group=info["group"],
        )
        if gathered is None:
            return torch.zeros((len(rows), nl), dtype=torch.float32), [np.zeros(n, dtype=np.float32) for n in lengths]
        keep_all, rank_all = gathered
        keep_np = keep_all.reshape(-1).cpu().numpy()
        cu = plan.cu
        return rank_all.cpu(), [keep_np[cu[i] : cu[i + 1]] for i in range(len(rows))]

    # -- asynchronous forward: launch now, collect later (launches.py; host stages of the neighbouring batches overlap the GPU) --
    def _can_pipeline(self) -> bool:
        # (also with a process group attached: _launch_rows enqueues this rank's share, _collect_rows gathers)
        return self._forward_is_native()

    @functools.cached_property
    def _staging(self) -> launches.Staging:
        """The pinned staging pools of this model's launches and their rotation, made on first use."""

        return launches.Staging()

    _pack_launch = staticmethod(launches.pack_launch)
    _dist_info = launches.dist_info
    _count_forward = launches.count_forward
    _launch_rows = launches.launch_rows
    _enqueue_packed = launches.enqueue_packed
    _guard_launch = launches.guard_launch
    _finish_launch = launches.finish_launch
    _collect_rows = launches.collect_rows
    _collect_packed = launches.collect_packed

    def _enqueue_local(self, rows: list[list[int]], segments: list[list[tuple[int, int]]] | None) -> launches.Launch:
        """The launch of ``_launch_rows`` for THIS process's rows."""

        return self._enqueue_packed(*self._pack_launch(rows, segments))

    def _predict_rows_local(self, rows: list[list[int]], type_rows: list[list[int]] | None) -> tuple[torch.Tensor, list[np.ndarray]]:
        """This process's rows -> (ranking_logits[B, nl] fp32 CPU, per-row keep probabilities fp32).

        Native path: one packed H2D copy, one forward (keep-probability evaluated by the head kernel), one D2H copy.
        Overridden ``forward``: the reference's padded protocol (standalone.py:2832-2924)."""

        if self._forward_is_native():
            ids_np, cu_np, max_len = pack_rows(rows)
            self.encoder.check_ids(ids_np)
            dev = self._runtime_device
            # keep-probability = softmax(pruning_logits)[:, 1], evaluated by the head kernel itself (no ATen
            # arithmetic on the product path; the D2H payload is 4 B per token)
            keep_dev = torch.empty(int(cu_np[-1]), dtype=torch.float32, device=dev)
            ids_dev, cu_dev = torch.from_numpy(ids_np).to(dev), torch.from_numpy(cu_np).to(dev)
            _, rank = self.encoder.forward_packed(ids_dev, cu_dev, cu_np, max_len, keep_prob=keep_dev)
            self._count_forward(len(rows), int(cu_np[-1]))
            keep = keep_dev.cpu().numpy()
            rank_cpu = rank.cpu()
            if self.encoder.f8_active() and not (np.isfinite(keep).all() and bool(torch.isfinite(rank_cpu).all())):
                # range guard of the fp16 + e4m3 kernel sets: repeat on the (hi, lo) bf16 sets, stay there
                if self.encoder.fall_back_from_f8("get_raw_predictions"):
                    _, rank = self.encoder.forward_packed(ids_dev, cu_dev, cu_np, max_len, keep_prob=keep_dev)
                    self._count_forward(len(rows), int(cu_np[-1]))
                    keep, rank_cpu = keep_dev.cpu().numpy(), rank.cpu()
            return rank_cpu, [keep[cu_np[i] : cu_np[i + 1]] for i in range(len(rows))]

        pad_raw = getattr(self.tokenizer, "pad_token_id", None)
        pad_id = int(pad_raw) if pad_raw is not None else 0
        width = max((len(r) for r in rows), default=0)
        ids = torch.full((len(rows), width), pad_id, dtype=torch.long)
        mask = torch.zeros((len(rows), width), dtype=torch.long)
        types = torch.zeros((len(rows), width), dtype=torch.long) if type_rows and any(type_rows) else None
        for i, row in enumerate(rows):
            n = len(row)
            if n == 0:
                continue
            ids[i, :n] = torch.tensor(row, dtype=torch.long)
            mask[i, :n] = 1
            if types is not None:
                t = list(type_rows[i] or [0] * n)[:n]
                t = t + [t[-1] if t else 0] * (n - len(t))
                types[i, :n] = torch.tensor(t, dtype=torch.long)
        inputs: dict[str, torch.Tensor] = {"input_ids": ids, "attention_mask": mask}
        if types is not None:
            inputs["token_type_ids"] = types
        outputs = self.forward(return_dict=True, **inputs)
        rank_cpu = self._extract_model_output(outputs, "ranking_logits").detach().cpu().to(torch.float32)
        prune_cpu = self._extract_model_output(outputs, "pruning_logits").detach().cpu().to(torch.float32)
        keeps: list[np.ndarray] = []
        for i in range(len(rows)):
            probs = torch.softmax(prune_cpu[i], dim=-1).numpy()
            if probs.ndim == 2 and probs.shape[1] == 2:
                probs = probs[:, 1]
            elif probs.ndim != 1:
                probs = probs.reshape(-1)
            keeps.append(probs)
        return rank_cpu, keeps

    def _sync(self) -> None:
        dev = getattr(self, "_runtime_device", None)
        if isinstance(dev, torch.device) and dev.type == "cuda" and torch.cuda.is_available():
            torch.cuda.synchronize(dev)

    @staticmethod
    def _ranking_score(logits: torch.Tensor) -> float:
        if logits.ndim == 0 or logits.numel() == 1:
            return torch.sigmoid(logits.flatten())[0].item()
        return torch.sigmoid(logits[..., 0]).item()

    # ------------------------------------------------------------------------------------------
    # single-block API (ref: get_raw_predictions_batch :1752-1841, predict_with_thresholds :1843-1881)
    # ------------------------------------------------------------------------------------------
    def _encode_texts(self, texts: list[str], truncate: bool) -> list[list[int]]:
        encoded = self.tokenizer(
            texts, padding=False, truncation=truncate, max_length=self.max_length if truncate else None
        )
        return [[int(t) for t in ids] for ids in encoded["input_ids"]]

    def _context_ranges_from_contexts(self, query: str, contexts: Sequence[str]) -> list[tuple[int, int]]:
        if not contexts:
            return []
        prefix = query + (self.tokenizer.sep_token or "")
        cumulative = [prefix + "".join(contexts[: i + 1]) for i in range(len(contexts))]
        boundaries = [len(ids) for ids in self._encode_texts(cumulative, truncate=True)]
        prev = len(self._encode_texts([prefix], truncate=False)[0])
        ranges = []
        for boundary in boundaries:
            ranges.append((prev, boundary))
            prev = boundary
        return ranges

    def get_raw_predictions_batch(
        self, query: str | Sequence[str], contexts_batch: Sequence[Sequence[str]], batch_size: int | None = None
    ) -> list[RawPrediction]:
        if not contexts_batch:
            return []
        sep = self.tokenizer.sep_token or ""
        if batch_size is None or batch_size <= 0:
            batch_size = len(contexts_batch)
        if isinstance(query, Sequence) and not isinstance(query, str):
            queries = [str(q) for q in query]
            if len(queries) != len(contexts_batch):
                raise ValueError("When providing multiple queries, their count must match contexts_batch.")
        else:
            queries = [str(query)] * len(contexts_batch)
        results: list[RawPrediction] = []
        n_blocks = len(contexts_batch)
        spans = [(start, min(start + batch_size, n_blocks)) for start in range(0, n_blocks, batch_size)]
        all_rows = widths = None
        if n_blocks > batch_size and self._forward_is_native() and self.forward_token_budget > 0:
            # native forward: chunks of batch_size rows coalesced within the token budget (pipeline.plan_forward_chunks); a
            # row's tokens do not depend on its batch (no padding), and each row keeps the padded width of ITS batch_size chunk
            all_rows = self._encode_texts([q + sep + "".join(c) for q, c in zip(queries, contexts_batch)], truncate=True)
            lengths = [len(r) for r in all_rows]
            widths = [max(lengths[a:b], default=0) for a, b in spans]
            spans = pl.plan_forward_chunks(lengths, batch_size, self.forward_token_budget)
        for start, stop in spans:
            chunk = contexts_batch[start:stop]
            chunk_queries = queries[start:stop]
            if all_rows is not None:
                rows = all_rows[start:stop]
            else:
                rows = self._encode_texts([q + sep + "".join(c) for q, c in zip(chunk_queries, chunk)], truncate=True)
            rank, keeps = self._predict_rows(rows, None)
            # the reference returns every row's probabilities at the padded batch width (standalone.py:1820-1823: softmax
            # over the padded logits tensor); positions past the row's tokens carry softmax([0, 0])[1] = 0.5 here (the
            # forward boundary zero-fills masked positions; the reference's values there are whatever the model makes of
            # pad tokens, and no range ever addresses them)
            # (the padded width of a row is that of ITS batch_size chunk, whatever forward it travelled in)
            row_widths = ([widths[at // batch_size] for at in range(start, stop)] if widths is not None
                          else [max((len(r) for r in rows), default=0)] * len(rows))
            for i, ctxs in enumerate(chunk):
                if len(ctxs) == 0:
                    continue
                width = row_widths[i]
                probs = np.asarray(keeps[i], dtype=np.float32)
                if len(probs) < width:
                    probs = np.concatenate([probs, np.full(width - len(probs), 0.5, dtype=np.float32)])
                results.append(
                    RawPrediction(
                        query=chunk_queries[i],
                        contexts=list(ctxs),
                        ranking_score=self._ranking_score(rank[i]),
                        pruning_probs=probs,
                        context_ranges=self._context_ranges_from_contexts(chunk_queries[i], ctxs),
                    )
                )
        return results

    def get_raw_predictions(self, query: str, contexts: Iterable[str]) -> RawPrediction:
        return self.get_raw_predictions_batch(query, [list(contexts)])[0]

    def predict_with_thresholds(
        self, query: str, contexts: Iterable[str], thresholds: Iterable[float], *, use_majority: bool = False
    ) -> dict[str, Any]:
        raw = self.get_raw_predictions(query, contexts)
        predictions: dict[float, list[int]] = {}
        for threshold in thresholds:
            flags: list[int] = []
            for start, end in raw.context_ranges:
                segment = raw.pruning_probs[start:end]
                if segment.size == 0:
                    flags.append(1)
                elif use_majority:
                    flags.append(1 if np.count_nonzero(segment > threshold) >= (segment.size / 2) else 0)
                else:
                    flags.append(1 if float(segment.mean()) > threshold else 0)
            predictions[threshold] = flags
        return {
            "query": raw.query,
            "contexts": raw.contexts,
            "ranking_score": raw.ranking_score,
            "predictions": predictions,
            "context_ranges": raw.context_ranges,
            "pruning_probs": raw.pruning_probs,
        }

    # ------------------------------------------------------------------------------------------
    # process(): host stages (thin wrappers over pipeline.py so they can be overridden / tested)
    # ------------------------------------------------------------------------------------------
    def _normalize_inputs(self, question, context):
        return pl.normalize_inputs(question, context)

    def _resolve_titles(self, queries, contexts, title, *, first_line_as_title: bool):
        return pl.resolve_titles(queries, contexts, title, first_line_as_title=first_line_as_title)

    def _resolve_prefix_sentences(self, title_spec, context_idx: int):
        return pl.resolve_prefix_sentences(title_spec, context_idx)

    def _resolve_sentence_splitter(self, splitter, language):
        return resolve_sentence_splitter(splitter, language, getattr(self, "default_splitter_language", None))

    def _truncate_fragment(self, fragment: FragmentRecord, max_tokens: int) -> FragmentRecord:
        return pl.truncate_fragment(self.tokenizer, fragment, max_tokens)

    def _assemble_blocks_from_fragments(self, query_token_length: int, sep_token_length: int, fragments):
        return pl.assemble_blocks(self.tokenizer, fragments, query_token_length, sep_token_length, self.max_length)

    def _prepare_block_inputs(self, query_tokens, fragments):
        return pl.prepare_block_inputs(
            self.tokenizer,
            query_tokens,
            fragments,
            manual_specials=getattr(self, "_manual_special_tokens_required", False),
            manual_cls=getattr(self, "_manual_cls_token_id", None),
            manual_sep=getattr(self, "_manual_sep_token_id", None),
        )

    def _extract_first_line_titles(self, contexts):
        return pl.extract_first_line_titles(contexts)

    def _prepare_titles(self, title, queries, contexts):
        return pl.prepare_titles(title, queries, contexts)

    @staticmethod
    def _as_state(info: Any) -> ContextState | None:
        """Accept the reference's dict-shaped ``contexts_info`` entries as well as ContextState."""

        if info is None or isinstance(info, ContextState):
            return info
        return ContextState(
            sentences=list(info.get("sentences", [])),
            fragments=list(info.get("fragments", [])),
            blocks=list(info.get("blocks", [])),
            prefix_length=int(info.get("prefix_length", 0)),
            prefix_sentences=list(info.get("prefix_sentences", []) or []),
            prefix_token_counts=list(info.get("prefix_token_counts", []) or []),
            title_is_first_sentence=bool(info.get("title_is_first_sentence", False)),
            original_text=info.get("original_text", ""),
            raw_blocks=list(info.get("raw_blocks", [])),
        )

    def _postprocess_contexts(self, queries, contexts, contexts_info, *, threshold: float, always_select_title: bool,
                              use_best_reranker_score: bool, sentence_probability_groups_requested: bool,
                              collect_sentence_texts: bool, first_line_as_title: bool, zero_score_when_empty: bool):
        """Reference-shaped entry point (ref: _postprocess_contexts :2962-3202): returns the 8-tuple
        (pruned, scores, compression, kept, removed, titles, sentence_probabilities, seconds)."""

        t0 = perf_counter()
        states = {key: self._as_state(value) for key, value in contexts_info.items()}
        res = pl.postprocess_contexts(
            queries, contexts, states, threshold=threshold, always_select_title=always_select_title,
            use_best_reranker_score=use_best_reranker_score, want_sentence_probabilities=sentence_probability_groups_requested,
            want_sentence_texts=collect_sentence_texts, first_line_as_title=first_line_as_title, zero_score_when_empty=zero_score_when_empty)
        return (*res.as_tuple(), perf_counter() - t0)

    def _apply_reordering(self, pruned_contexts, reranking_scores, compression_rates, kept_sentences, removed_sentences, title_values,
                          sentence_probability_groups, *, top_k: int | None):
        """Reference-shaped entry point (ref: _apply_reordering :3204-3312)."""

        result = pl.PostprocessResult(pruned_contexts, reranking_scores, compression_rates, kept_sentences, removed_sentences,
                                      title_values, sentence_probability_groups)
        return pl.apply_reordering(result, top_k).as_tuple()

    def _estimate_device_memory_bytes(self) -> int | None:
        override = os.getenv("OPEN_PROVENCE_DEVICE_MEMORY_GB")
        if override:
            try:
                parsed = float(override)
            except ValueError:
                parsed = None
            if parsed and parsed > 0:
                return int(parsed * (1024**3))
        try:
            return int(torch.cuda.get_device_properties(self._runtime_device).total_memory)
        except Exception:
            return None

    def _auto_tune_preprocess_loader(self, **kwargs: Any) -> tuple[int, int, int | None]:
        return pl.auto_tune_preprocess_loader(device_memory_bytes=self._estimate_device_memory_bytes(), **kwargs)

    def _iter_jobs(
        self, queries, contexts, titles, splitter: SentenceSplitter, query_token_ids: list[list[int]], *,
        strip_sentences: bool, timing: dict[str, float], workers: int = 0, group_size: int = 64,
        owned: Sequence[Sequence[bool]] | None = None, fragment_args: Mapping[str, Any] | None = None,
    ):
        """One job per (query, context), produced lazily: sentences (prefix + split or pre-split), their token lists
        and the prefix token counts (ref: _build_preprocess_jobs :2436-2519, _precompute_sentences_and_tokens :2198).
        ``query_token_ids`` gains a query's ids before the first of its jobs is yielded.

        The reference hands this stage to DataLoader workers so that it overlaps the forward (:2681-2760); here the
        consumer launches a forward asynchronously after every granule of jobs and comes back for the next ones, so the
        same overlap happens on one host thread.

        Contexts are prepared in groups of ``group_size``: sentence splitting per context, then ONE tokenizer call over
        the sentences of the whole group (``pipeline.tokenize_sentence_groups``; same ids, a fraction of the call
        overhead, and a fast tokenizer's own thread pool gets a batch worth spreading)."""

        def specs():
            for q_idx, query in enumerate(queries):
                query_token_ids.append(pl.tokenize_query(self.tokenizer, query))
                for c_idx, entry in enumerate(contexts[q_idx]):
                    if owned is None or owned[q_idx][c_idx]:  # job-sharded call: the other ranks' contexts are skipped
                        yield q_idx, c_idx, entry

        def build_group(group):
            """Jobs of a group of contexts: sentences per context, then ONE tokenizer call over all of them."""

            prepared = []
            t_collect = t_norm = 0.0
            for q_idx, c_idx, entry in group:
                if isinstance(entry, list):
                    manual = [str(s) for s in entry if str(s).strip()]
                    text = "".join(manual)
                else:
                    manual = None
                    text = entry
                prefix, title_is_first = self._resolve_prefix_sentences(titles[q_idx], c_idx)
                payload = {"context_text": text, "prefix_sentences": prefix, "manual_sentences": manual}
                t0 = perf_counter()
                raw = pl.collect_candidate_sentences(payload, splitter)
                t1 = perf_counter()
                sentences = pl.normalize_sentences(raw, text, strip_sentences)
                t2 = perf_counter()
                t_collect += t1 - t0
                t_norm += t2 - t1
                prepared.append((q_idx, c_idx, text, prefix, title_is_first, sentences))
            t2 = perf_counter()
            token_groups = pl.tokenize_sentence_groups(self.tokenizer, [p[5] for p in prepared])
            t3 = perf_counter()
            jobs = [
                {
                    "query_idx": q_idx,
                    "context_idx": c_idx,
                    "context_text": text,
                    "prefix_sentences": prefix,
                    "title_is_first_sentence": title_is_first,
                    "prefix_token_counts": [len(t) for t in token_lists[: len(prefix)]],
                    "sentences": sentences,
                    "token_lists": token_lists,
                }
                for (q_idx, c_idx, text, prefix, title_is_first, sentences), token_lists in zip(prepared, token_groups)
            ]
            t_frag = 0.0
            if fragment_args is not None:  # fragments of the group too (one decode call), off the consumer's thread
                t4 = perf_counter()
                fragments = pl.fragmentize_many(self.tokenizer, [(job["token_lists"], job["context_text"]) for job in jobs], **fragment_args)
                for job, records in zip(jobs, fragments):
                    job["fragments"] = records
                t_frag = perf_counter() - t4
            return jobs, (t_collect, t_norm, t3 - t2, t_frag)

        # With worker threads the per-stage seconds are summed over threads that run side by side: they are scaled by
        # 1 / workers so that the trace's stage timers add up to wall-clock seconds of the stage (what the reference's
        # single-thread timers mean), never to more than the call took.
        share = 1.0 / max(1, int(workers))

        def account(times):
            timing["sentence_collect_seconds"] += times[0] * share
            timing["sentence_normalize_seconds"] += times[1] * share
            timing["tokenize_seconds"] += times[2] * share
            timing["fragment_decode_seconds"] += times[3] * share

        def groups():
            it = specs()
            while True:
                group = list(itertools.islice(it, max(1, int(group_size))))
                if not group:
                    return
                yield group

        if workers <= 0:
            for group in groups():
                jobs, times = build_group(group)
                account(times)
                yield from jobs
            return
        # preprocess_workers > 0: the reference runs this stage in DataLoader worker processes (standalone.py:3589,
        # :2478-2519).  Here: worker THREADS with a bounded look-ahead over GROUPS of contexts, results yielded in order.
        # The expensive calls release the GIL where it matters -- a Hugging Face fast tokenizer (Rust `encode_batch`) and
        # the Rust / C sentence splitters (fast-bunkai, nltk's regex core) -- and no process is forked next to a live HIP
        # runtime.
        from collections import deque
        from concurrent.futures import ThreadPoolExecutor

        window = max(2 * workers, 4)
        with ThreadPoolExecutor(max_workers=workers, thread_name_prefix="open-provence-prep") as pool:
            inflight: deque = deque()
            for group in groups():
                inflight.append(pool.submit(build_group, group))
                if len(inflight) >= window:
                    jobs, times = inflight.popleft().result()
                    account(times)
                    yield from jobs
            while inflight:
                jobs, times = inflight.popleft().result()
                account(times)
                yield from jobs

    def _build_jobs(
        self, queries, contexts, titles, splitter: SentenceSplitter, *, strip_sentences: bool, timing: dict[str, float]
    ) -> tuple[list[dict[str, Any]], list[list[int]]]:
        query_token_ids: list[list[int]] = []
        jobs = list(self._iter_jobs(queries, contexts, titles, splitter, query_token_ids, strip_sentences=strip_sentences, timing=timing))
        return jobs, query_token_ids

    def _run_inference_batches(
        self,
        inference_jobs: list[dict[str, Any]],
        batch_size: int,
        queries: list[str],
        query_token_ids: list[list[int]],
        states: dict[tuple[int, int], ContextState],
        pending: list[Any] | None = None,
    ) -> float:
        """Blocks -> ``[CLS] q [SEP] ctx [SEP]`` rows -> forward -> per-block raw predictions (ref :2761-2960).
        Returns the seconds spent launching / waiting for the forward.

        With ``pending`` (a list owned by ``process()``) and the native forward the loop is pipelined: a chunk's forward
        is only ENQUEUED (pinned staging, asynchronous copies), and the previous chunk's results are collected right
        after -- so packing chunk k + 1 and unpacking chunk k - 1 overlap the GPU working on chunk k; the caller flushes
        what is still in flight with :meth:`_flush_pending`.  The reference's loop is launch -> wait -> convert, one
        row at a time (standalone.py:2854-2898)."""

        elapsed = 0.0
        pipelined = pending is not None and self._can_pipeline()
        n_jobs = len(inference_jobs)
        spans = [(start, min(start + batch_size, n_jobs)) for start in range(0, n_jobs, batch_size)]
        prepared = None
        # Native forward: a forward costs the same up to about one round of the chip, so the chunks of batch_size rows are
        # coalesced within the model's token budget (pipeline.plan_forward_chunks; rows are independent, results do not
        # change).  The plan needs every row's length: the rows of the granule are built first.  A replaced forward keeps
        # the reference's contract: at most batch_size rows per call.
        if n_jobs > batch_size and self._forward_is_native() and self.forward_token_budget > 0:
            prepared = [
                self._prepare_block_inputs(query_token_ids[job["query_idx"]],
                                           states[(job["query_idx"], job["context_idx"])].blocks[job["block_idx"]])
                for job in inference_jobs
            ]
            spans = pl.plan_forward_chunks([len(p[0]) for p in prepared], batch_size, self.forward_token_budget)
        for start, stop in spans:
            chunk = inference_jobs[start:stop]
            if not chunk:
                continue
            rows: list[list[int]] = []
            type_rows: list[list[int]] = []
            ranges_per_job: list[list[tuple[int, int]]] = []
            for at, job in enumerate(chunk, start):
                if prepared is not None:
                    ids, _mask, type_ids, ranges = prepared[at]
                else:
                    block = states[(job["query_idx"], job["context_idx"])].blocks[job["block_idx"]]
                    ids, _mask, type_ids, ranges = self._prepare_block_inputs(query_token_ids[job["query_idx"]], block)
                rows.append(ids)
                type_rows.append(type_ids)
                ranges_per_job.append(ranges)
            if pipelined:
                # the token range every fragment is averaged over is known now: the means are taken on the device
                segments = [
                    pl.fragment_token_ranges(
                        states[(job["query_idx"], job["context_idx"])],
                        states[(job["query_idx"], job["context_idx"])].blocks[job["block_idx"]], ranges_per_job[i], len(rows[i]),
                    )
                    for i, job in enumerate(chunk)
                ]
                t0 = perf_counter()
                handle = self._launch_rows(rows, segments)
                elapsed += perf_counter() - t0
                pending.append((handle, chunk, ranges_per_job, queries, states))
                if len(pending) > 1:  # the previous chunk has had a whole launch + host stage to finish
                    elapsed += self._flush_pending(pending, keep_last=1)
                continue
            self._sync()
            t0 = perf_counter()
            rank, keeps = self._predict_rows(rows, type_rows)
            self._sync()
            elapsed += perf_counter() - t0
            self._store_raw_predictions(chunk, ranges_per_job, queries, states, rank, keeps)
        return elapsed

    @staticmethod
    def _ranking_scores(rank: torch.Tensor) -> list[float]:
        """Ranking logits ``[rows, nl]`` (or flat) -> the rows' scores as Python floats."""

        rank_scores = rank[:, 0] if rank.ndim == 2 and rank.shape[1] > 1 else rank.reshape(-1)
        # = _ranking_score row by row (ref :2913-2916), bit for bit: ATen's vectorized sigmoid of a contiguous batch differs
        # from the scalar one the reference's one-row tensors take by 1 ulp in ~4 % of the elements -- and by WHICH elements
        # depends on a row's position in the batch.  A strided view sends every element through the scalar functor.
        spread = torch.empty((rank_scores.numel(), 2), dtype=torch.float32)
        spread[:, 0] = rank_scores.reshape(-1).to(torch.float32)
        return torch.sigmoid(spread[:, 0]).tolist()

    def _warn_nan_once(self) -> None:
        if self.__dict__.get("_nan_warned"):
            return
        # The fp16 + e4m3 kernel sets turn an MLP activation beyond fp16's range into Inf on purpose
        # (csrc/opk_common.hip.h: set_overflowing_conversions) and _guard_launch / _predict_rows_local have already
        # repeated such a batch on the (hi, lo) bf16 sets: what arrives here is NaN in fp32-range arithmetic, i.e.
        # what the reference computes for this checkpoint / input too.  It goes on as the reference's does (a NaN
        # probability fails `> threshold`, standalone.py:3130) -- said once, not raised: a drop-in must not fail
        # where the reference returns, and a raise on one rank of a process group would strand the others.
        self.__dict__["_nan_warned"] = True
        LOGGER.warning("the forward returned NaN for a (query, context) block on kernel set %r (every set with an fp16 operand "
                       "plane has been left by now): the checkpoint holds non-finite weights or the inputs overflow fp32; results "
                       "follow the reference (NaN scores)", self.encoder.effective_policy()["kernel_set"] if self._forward_is_native() else "replaced forward")

    def _store_raw_predictions(self, chunk, ranges_per_job, queries, states, rank, keeps) -> None:
        scores = self._ranking_scores(rank)
        for i, job in enumerate(chunk):
            reduced = isinstance(keeps[i], list)  # per-fragment means from the device (see _launch_rows)
            if scores[i] != scores[i] or (reduced and any(m != m for m in keeps[i])):
                self._warn_nan_once()
            states[(job["query_idx"], job["context_idx"])].raw_blocks.append(
                (
                    job["block_idx"],
                    RawPrediction(
                        query=queries[job["query_idx"]],
                        contexts=list(job["texts"]),
                        ranking_score=scores[i],
                        pruning_probs=_NO_PROBS if reduced else keeps[i],
                        context_ranges=ranges_per_job[i],
                        fragment_means=keeps[i] if reduced else None,
                    ),
                )
            )

    def _flush_pending(self, pending: list[Any], keep_last: int = 0) -> float:
        """Collect launched forwards (all but the newest ``keep_last``); returns the seconds spent waiting."""

        waited = 0.0
        while len(pending) > keep_last:
            handle, chunk, ranges_per_job, queries, states = pending.pop(0)
            t0 = perf_counter()
            rank, keeps = self._collect_rows(handle)
            waited += perf_counter() - t0
            self._store_raw_predictions(chunk, ranges_per_job, queries, states, rank, keeps)
        return waited

    # ------------------------------------------------------------------------------------------
    # prepared contexts (prepared.py): the query-independent stages once per corpus
    # ------------------------------------------------------------------------------------------
    def prepare_contexts(
        self,
        contexts: Sequence[str] | Sequence[Sequence[str]],
        title: None | str | Sequence[str] = "first_sentence",
        first_line_as_title: bool = False,
        *,
        sentence_splitter: SentenceSplitter | Mapping[str, SentenceSplitter] | None = None,
        language: str | None = None,
        strip_sentences: bool = False,
        respect_sentence_boundaries: bool = False,
        preprocess_workers: int | None = None,
    ) -> PreparedContexts:
        """Split, tokenise and fragmentise a corpus ONCE: ``contexts`` is a flat sequence, each entry a string or a list
        of pre-split sentences, as one question's context list is in :meth:`process`; ``title`` / ``first_line_as_title``
        as there for one question.  ``process(question, prepared)`` or ``process(question, prepared.select(indices))``
        then returns what ``process(question, [those contexts], title=...)`` with the same arguments returns, while the
        host only tokenises the question and plans blocks and forwards from lengths; on the native forward the rows are
        laid out on the device from the fragments' token ids, which are uploaded on first use (4 bytes per token, below
        2^31 tokens in all).  The object belongs to this model, its tokenizer and ``max_length``.  Sharded and front-end
        requests are not supported on prepared contexts."""

        if isinstance(contexts, (str, bytes)) or not pl._is_sequence(contexts):
            raise ValueError("prepare_contexts takes a flat sequence of contexts (strings or lists of sentences)")
        splitter = self._resolve_sentence_splitter(sentence_splitter, language)
        _queries, nested, _structure = pl.normalize_inputs("", list(contexts))
        nested, titles = self._resolve_titles([""], nested, title, first_line_as_title=first_line_as_title)
        entries = nested[0]
        timing = pl.empty_stage_timing()
        if preprocess_workers is not None:
            workers = min(max(0, int(preprocess_workers)), 32)
        else:
            workers = rq.default_thread_workers(self, len(entries), splitter)
        t0 = perf_counter()
        jobs = self._iter_jobs(
            [""], [entries], titles, splitter, [], strip_sentences=strip_sentences, timing=timing, workers=workers,
            fragment_args=dict(max_fragment_tokens=pl.max_fragment_tokens(self.max_length, respect_sentence_boundaries),
                               strip_sentences=strip_sentences, respect_sentence_boundaries=respect_sentence_boundaries),
        )
        items: list[PreparedItem] = []
        frag_base = 0
        for job in jobs:
            items.append(PreparedItem(entries[job["context_idx"]], job, frag_base))
            frag_base += len(job["fragments"])
        timing["total_seconds"] = perf_counter() - t0
        template = derive_row_template(
            lambda query, ctx: self._prepare_block_inputs(query, [FragmentRecord("", 0, 0, 0, len(ctx), list(ctx))])[0])
        settings = {
            "title": title if (title is None or isinstance(title, str)) else [list(t) if pl._is_sequence(t) else str(t) for t in title],
            "first_line_as_title": bool(first_line_as_title), "sentence_splitter": sentence_splitter, "language": language,
            "strip_sentences": bool(strip_sentences), "respect_sentence_boundaries": bool(respect_sentence_boundaries),
            "manual_specials": (getattr(self, "_manual_special_tokens_required", False), getattr(self, "_manual_cls_token_id", None),
                                getattr(self, "_manual_sep_token_id", None)),
        }
        return PreparedContexts(self, items, settings, template, timing)

    def _check_prepared_request(self, corpus: PreparedContexts, given: Mapping[str, Any]) -> None:
        """The refusals of ``process()`` on prepared contexts (``ValueError``)."""

        if corpus.model is not self:
            raise ValueError("these contexts were prepared by another model instance: prepare them with this model's prepare_contexts()")
        manual = (getattr(self, "_manual_special_tokens_required", False), getattr(self, "_manual_cls_token_id", None),
                  getattr(self, "_manual_sep_token_id", None))
        if corpus.tokenizer is not self.tokenizer or manual != corpus.settings["manual_specials"]:
            raise ValueError("the model's tokenizer has changed since these contexts were prepared: prepare them again")
        if int(self.max_length) != corpus.max_length:
            raise ValueError(f"max_length is {self.max_length} but these contexts were prepared with max_length {corpus.max_length}: "
                             "prepare them again")
        defaults = {"title": "first_sentence", "first_line_as_title": False, "sentence_splitter": None, "language": None,
                    "strip_sentences": False, "respect_sentence_boundaries": False}
        for name, default in defaults.items():
            value, kept = given[name], corpus.settings[name]
            if name == "title" and not (value is None or isinstance(value, str)):
                value = [list(t) if pl._is_sequence(t) else str(t) for t in value]
            same_as_default = value is default or (isinstance(default, str) and value == default)
            if not same_as_default and not (value is kept or value == kept):
                raise ValueError(f"process() on prepared contexts got {name}={given[name]!r}, but they were prepared with "
                                 f"{name}={kept!r}: these arguments belong to prepare_contexts()")
        if getattr(self, "_dist", None) or self.__dict__.get("_remote_forward") is not None:
            raise ValueError("prepared contexts do not support a process group or a host front-end: sharded prepared requests "
                             "are out of scope (detach the group, or pass the raw texts)")

    def _prepared_device_corpus(self, corpus: PreparedContexts) -> dict[str, Any]:
        """The resident corpus of ``op_assemble_rows``, uploaded on first use: the fragments' token ids as one flat int32
        buffer in context order then fragment order, their offsets, the template pieces -- ids checked against the
        embedding table once, here."""

        device = corpus._device
        if device is None or device["device"] != self._runtime_device:
            ids_np, frag_off_np = corpus.flat_tokens()
            pieces = [np.asarray(p, dtype=np.int32) for p in (corpus.template.prefix, corpus.template.middle, corpus.template.suffix)]
            self.encoder.check_ids(ids_np)
            for piece in pieces:
                self.encoder.check_ids(piece)
            dev = self._runtime_device
            device = corpus._device = {
                "device": dev, "ids": torch.from_numpy(ids_np).to(dev), "frag_off": torch.from_numpy(frag_off_np).to(dev),
                "frag_off_np": frag_off_np, "pieces": pieces,
            }
            # the tables of the last stages on the device (an eligible corpus; 8 more bytes per fragment)
            tables = corpus.decision_tables()
            if tables is not None:
                device["frag_shift"] = torch.from_numpy(tables["frag_shift"]).to(dev)
                device["frag_sent"] = torch.from_numpy(tables["frag_sent"]).to(dev)
        return device

    def _assemble_on_device(self, assemble: dict[str, Any], plan_dev, plan_np, cu_dev, cu_np) -> torch.Tensor:
        corpus, queries = assemble["corpus"], assemble["queries"]
        return self.encoder.assemble_rows(corpus["ids"], corpus["frag_off"], corpus["frag_off_np"], queries["ids"], queries["off"],
                                          queries["off_np"], corpus["pieces"], plan_dev, plan_np, cu_dev, cu_np)

    def _planned_means_on_device(self, planned: dict[str, Any], cu_dev, cu_np, keep_dev, ids_dev=None) -> torch.Tensor:
        """The fragment means of one forward of a prepared request, from its plan (``planned``: the forward's ``assemble``
        with ``plan_dev``) -> the forward's slice of the request's means buffer (``means["values"]``).  With
        ``means["locate"]`` every context is looked up in its row first (``ids_dev``: the launch's assembled rows;
        ``op_located_fragment_means``), its place landing in the forward's slice of ``means["ctx_start"]``."""

        corpus, queries, means = planned["corpus"], planned["queries"], planned["means"]
        first, last = means["rows"]
        shared = (corpus["frag_off"], corpus["frag_off_np"], queries["off"], queries["off_np"], corpus["pieces"], planned["plan_dev"], planned["plan"],
                  cu_dev, cu_np, keep_dev, corpus["frag_shift"], means["slot_off"][first: last + 1], means["slot_off_np"][first: last + 1],
                  means["values"], means["slot_frag"])
        if means.get("locate"):
            if ids_dev is None:
                raise RuntimeError("a located launch without its assembled rows")
            self.encoder.located_fragment_means(*shared, ids_dev, means["ctx_start"][first:last])
        else:
            self.encoder.planned_fragment_means(*shared)
        slot_off = means["slot_off_np"]
        return means["values"][int(slot_off[first]): int(slot_off[last])]

    def _gather_job_results(self, result, owned, info, error: BaseException | None = None):
        """Job-sharded ``process()``: every rank sends the post-processed fields of the contexts it owns to rank
        ``dst`` (one ``gather_object``; the payload is the texts and a few floats per context), which writes them into
        its own full-size result lists -- the entries of contexts a rank does not own are placeholders until then.

        A rank whose share FAILED (a splitter / tokenizer error on one of its contexts, an out-of-range id, ...) still
        enters the collective -- with an error marker instead of results (``error``: called from process()'s exit
        handler) -- and ``dst`` then tells every rank who failed (one ``broadcast_object_list``), so that all ranks raise
        instead of the healthy ones waiting forever for a peer that has left."""

        group, dst, rank, world = info["group"], info["dst"], info["rank"], info["world"]
        if world <= 1 and not info.get("force"):
            return result
        fields = []
        if error is None:
            fields = list(result.as_tuple())
            mine = {
                (q, c): tuple(None if f is None else f[q][c] for f in fields)
                for q, per_query in enumerate(owned) for c, own in enumerate(per_query) if own
            }
        else:
            mine = {"__error__": f"{type(error).__name__}: {error}"}
        transport = info.get("transport")
        if transport is not None:
            # host-mode front-end (frontend.py): pipes instead of a collective.  A replica hands its part to the GPU owner
            # and is done; the owner -- which owns no job -- serves the replicas' forwards until every part has arrived.
            gathered = transport.exchange(self, mine)
            failed = [{r: part["__error__"] for r, part in enumerate(gathered) if isinstance(part, dict) and "__error__" in part}]
        else:
            import torch.distributed as dist

            dst_global = dist.get_global_rank(group, dst) if group is not None and group is not dist.group.WORLD else dst
            gathered = [None] * world if rank == dst else None
            device = getattr(self, "device", None)
            ctx = torch.cuda.device(device) if (device is not None and torch.device(device).type == "cuda") else contextlib.nullcontext()
            with ctx:  # (the NCCL backend moves pickled objects through tensors on the CURRENT device)
                dist.gather_object(mine, gathered, dst=dst_global, group=group)
                failed = [{r: part["__error__"] for r, part in enumerate(gathered) if isinstance(part, dict) and "__error__" in part}] if rank == dst else [None]
                dist.broadcast_object_list(failed, src=dst_global, group=group)
        if failed[0]:
            if error is not None:
                return result  # this rank's own exception is already propagating
            raise RuntimeError("process() over the process group failed on rank(s) "
                               + "; ".join(f"{r}: {msg}" for r, msg in sorted(failed[0].items())))
        if rank != dst:
            return result
        for part_rank, part in enumerate(gathered):
            if part_rank == rank or not part:
                continue
            for (q, c), values in part.items():
                for f, v in zip(fields, values):
                    if f is not None:
                        f[q][c] = v
        return result

    # ------------------------------------------------------------------------------------------
    # process()
    # ------------------------------------------------------------------------------------------
    def process(
        self,
        question: str | Sequence[str],
        context: str | Sequence[str] | Sequence[Sequence[str]],
        title: None | str | Sequence[str] | Sequence[Sequence[str]] = "first_sentence",
        first_line_as_title: bool = False,
        *,
        batch_size: int = 32,
        threshold: float | None = None,
        always_select_title: bool = False,
        reorder: bool = False,
        top_k: int | None = None,
        sentence_splitter: SentenceSplitter | Mapping[str, SentenceSplitter] | None = None,
        language: str | None = None,
        use_best_reranker_score: bool = True,
        zero_score_when_empty: bool = True,
        show_progress: bool = True,
        debug_messages: bool | Callable[[str], None] = False,
        enable_warnings: bool = True,
        strip_sentences: bool = False,
        respect_sentence_boundaries: bool = False,
        return_sentence_metrics: bool = False,
        return_sentence_texts: bool = False,
        show_inference_progress: bool | None = None,
        preprocess_workers: int | None = None,
        preprocess_batch_size: int | None = None,
        torch_dataloader_kwargs: Mapping[str, Any] | None = None,
    ) -> dict[str, Any]:
        """Prune contexts sentence by sentence and score them against the question(s).

        Same parameters, input-shape dispatch and result keys as the reference's ``process``
        (standalone.py:3314-3808): ``pruned_context``, ``reranking_score``, ``compression_rate``, ``title``,
        ``timing``, ``performance_trace`` and, on request, ``kept_sentences`` / ``removed_sentences`` /
        ``sentence_probabilities``.  ``preprocess_workers`` / ``torch_dataloader_kwargs["num_workers"]`` start that many worker THREADS for the
        split / tokenize stage; the other loader keys are accepted for
        compatibility; preprocessing runs in-process (the reference's worker processes only re-copied cached
        token ids) but the preprocess-batch heuristics that cap the forward batch are kept."""

        # OPEN_PROVENCE_HOST_REPLICAS=N (or "auto"): large requests go through a HostFrontEnd kept on the model -- N worker
        # processes run the host stages, this process runs every forward (frontend.py).  The environment's counterpart of
        # the reference's DataLoader worker processes (standalone.py:3589) for callers that do not construct a front-end;
        # a request whose arguments cannot be pickled (a lambda as sentence_splitter) takes the in-process path below.
        # Round 5: without the variable too -- ``preprocess_workers=N`` / ``torch_dataloader_kwargs["num_workers"]`` ask for N such
        # worker PROCESSES (what the reference's parameter means), and a request of >= 2000 contexts starts them by itself
        # (the reference's auto rule, standalone.py:2588-2596), whenever the tokenizer and the splitter can be sent to a
        # process that does not import the caller's __main__; threads otherwise.  OPEN_PROVENCE_HOST_REPLICAS=0 keeps
        # everything in this process.
        # Prepared contexts (prepare_contexts): a PreparedContexts / PreparedView, or a list of views with a list of questions.
        # The request stays in this process -- no front-end, no process group -- and only its query-dependent half runs.
        prepared = _as_prepared_request(question, context)
        if prepared is not None:
            self._check_prepared_request(prepared[1][0].corpus, dict(
                title=title, first_line_as_title=first_line_as_title, sentence_splitter=sentence_splitter, language=language,
                strip_sentences=strip_sentences, respect_sentence_boundaries=respect_sentence_boundaries))
            settings = prepared[1][0].corpus.settings
            first_line_as_title = settings["first_line_as_title"]
            strip_sentences, respect_sentence_boundaries = settings["strip_sentences"], settings["respect_sentence_boundaries"]
        replicas, implicit = ("", True) if prepared is not None else self._front_end_request(context, preprocess_workers, torch_dataloader_kwargs)
        call = dict(
            question=question, context=context, title=title, first_line_as_title=first_line_as_title, batch_size=batch_size,
            threshold=threshold, always_select_title=always_select_title, reorder=reorder, top_k=top_k,
            sentence_splitter=sentence_splitter, language=language, use_best_reranker_score=use_best_reranker_score,
            zero_score_when_empty=zero_score_when_empty, show_progress=show_progress, debug_messages=debug_messages,
            enable_warnings=enable_warnings, strip_sentences=strip_sentences,
            respect_sentence_boundaries=respect_sentence_boundaries, return_sentence_metrics=return_sentence_metrics,
            return_sentence_texts=return_sentence_texts, show_inference_progress=show_inference_progress,
            preprocess_workers=preprocess_workers, preprocess_batch_size=preprocess_batch_size,
            torch_dataloader_kwargs=torch_dataloader_kwargs)
        if (replicas and not getattr(self, "_dist", None) and self.__dict__.get("_remote_forward") is None
                and not isinstance(context, str)):
            routed = self._process_through_front_end(replicas, implicit, call)
            if routed is not None:
                return routed

        # The request's host pipeline allocates ~10 short-lived containers per context and no reference cycles: the
        # cyclic collector only adds pauses that grow with the request (measured: -22 % at 1024 contexts).
        import gc

        gc_was_enabled = gc.isenabled()
        gc.disable()
        try:
            return self._process_impl(prepared=prepared, **call)
        finally:
            self.__dict__.pop("_forward_stats", None)  # (the call's counter: later get_raw_predictions* calls count nowhere)
            if gc_was_enabled:
                gc.enable()

    IMPLICIT_FRONT_END_CONTEXTS = 2000  # the reference's auto rule starts workers from 2000 jobs on (standalone.py:2591-2592)
    WORKER_REQUEST_MIN_CONTEXTS = 256   # preprocess_workers=N on a smaller request: threads (process start-up is seconds)

    @staticmethod
    def _count_contexts(ctx: Any) -> int:
        return sum(len(c) if isinstance(c, (list, tuple)) else 1 for c in ctx) if isinstance(ctx, (list, tuple)) else 1

    def _front_end_request(self, context: Any, preprocess_workers: int | None, loader_kwargs: Mapping[str, Any] | None) -> tuple[str, bool]:
        """-> (replicas: "" = none, "auto" or a number; implicit: not asked for through OPEN_PROVENCE_HOST_REPLICAS)."""

        env = os.environ.get("OPEN_PROVENCE_HOST_REPLICAS", "")
        if env:
            return ("" if env == "0" else env), False
        if isinstance(context, str):
            return "", True
        asked = preprocess_workers
        if asked is None and loader_kwargs and "num_workers" in loader_kwargs:
            asked = int(loader_kwargs["num_workers"])
        n_contexts = self._count_contexts(context)
        if asked is not None:
            return (str(int(asked)) if int(asked) > 0 and n_contexts >= self.WORKER_REQUEST_MIN_CONTEXTS else ""), True
        if os.getenv("OPEN_PROVENCE_PREPROCESS_WORKERS"):
            return "", True  # (that variable asks for worker THREADS, as before)
        return ("auto" if n_contexts >= self.IMPLICIT_FRONT_END_CONTEXTS else ""), True

    @staticmethod
    def _lives_in_main(obj: Any) -> bool:
        """A callable (or a mapping of them) defined in the caller's ``__main__``: a worker that does not import that module
        cannot resolve it."""

        values = obj.values() if isinstance(obj, Mapping) else [obj]
        return any(callable(v) and getattr(v, "__module__", None) in ("__main__", "__mp_main__") for v in values)

    def _process_through_front_end(self, replicas: str, implicit: bool, call: dict[str, Any]) -> dict[str, Any] | None:
        """``process()`` through a ``HostFrontEnd`` that lives on the model (started on first use, restarted when the
        number changes) -- asked for by OPEN_PROVENCE_HOST_REPLICAS, or ``implicit``: by ``preprocess_workers=`` / the
        size of the request; implicit front-ends do not import the caller's ``__main__`` in their workers (a script without an
        ``if __name__ == "__main__"`` guard would run again in each).  None = take the in-process path (few contexts, or
        arguments that cannot be sent to worker processes)."""

        import pickle

        from .frontend import HostFrontEnd, default_host_workers

        try:
            workers = default_host_workers() if replicas == "auto" else int(replicas)
        except ValueError:
            return None
        n_contexts = self._count_contexts(call["context"])
        if workers < 1 or n_contexts < 4 * workers:
            return None  # (a replica's fixed cost per request is not worth a handful of contexts)
        if implicit and (self._lives_in_main(call.get("sentence_splitter")) or self._lives_in_main(call.get("debug_messages"))
                         or not self._forward_is_native()):
            return None  # (a replaced forward -- tests, experiments -- stays in the process that replaced it)
        try:
            pickle.dumps({k: v for k, v in call.items() if k not in ("question", "context")})
        except Exception:
            if not self.__dict__.get("_front_end_warned"):
                self.__dict__["_front_end_warned"] = True
                LOGGER.warning("OPEN_PROVENCE_HOST_REPLICAS: the arguments of this process() call cannot be pickled (a lambda or "
                               "local function as sentence_splitter / debug_messages?): running it in this process")
            return None
        front = self.__dict__.get("_host_front_end")
        if (front is None or front.world != workers or not front._open
                or front.__dict__.get("forward_token_budget") != self.forward_token_budget):  # (replicas plan with the budget they were built with)
            if front is not None:
                front.close()
            if self.__dict__.get("_front_end_unavailable"):
                return None
            try:
                front = self.__dict__["_host_front_end"] = HostFrontEnd(self, workers=workers, import_main=not implicit)
                front.forward_token_budget = self.forward_token_budget
            except Exception as exc:  # the tokenizer cannot be sent to worker processes, or a worker failed to start
                self.__dict__["_front_end_unavailable"] = True
                self.__dict__["_host_front_end"] = None
                LOGGER.warning("host front-end unavailable (%s: %s): process() runs in this process", type(exc).__name__, exc)
                return None
        try:
            return front.process(**call)
        except (EOFError, BrokenPipeError, ConnectionError, OSError, RuntimeError) as exc:
            if isinstance(exc, RuntimeError) and "worker process has gone" not in str(exc):
                raise  # an error of the request itself (the replicas report those by message): the caller's to see
            # a replica died: one request is not worth a process() that fails for good -- drop the front-end (its workers
            # with it), remember not to restart it, and run this and every later request in-process
            LOGGER.warning("host front-end lost a worker (%s: %s): closed, process() runs in this process from now on", type(exc).__name__, exc)
            try:
                front.close()
            except Exception:
                pass
            self.__dict__["_host_front_end"] = None
            self.__dict__["_front_end_unavailable"] = True
            return None

    def _process_impl(
        self, question, context, title, first_line_as_title, *, batch_size, threshold, always_select_title, reorder, top_k,
        sentence_splitter, language, use_best_reranker_score, zero_score_when_empty, show_progress, debug_messages,
        enable_warnings, strip_sentences, respect_sentence_boundaries, return_sentence_metrics, return_sentence_texts,
        show_inference_progress, preprocess_workers, preprocess_batch_size, torch_dataloader_kwargs, prepared=None,
    ):
        """One request through its stages (request.py); the forwards go through the launch layer (launches.py)."""

        batch_size = max(1, batch_size)
        threshold = self._resolve_process_threshold(threshold)
        start_total = perf_counter()
        forward_stats = self.__dict__["_forward_stats"] = {"launches": 0, "rows": 0, "tokens": 0}
        splitter = self._resolve_sentence_splitter(sentence_splitter, language)
        debug_callback = rq.debug_callback_of(debug_messages, LOGGER)
        timing = pl.empty_stage_timing()
        run = rq.Run()

        with contextlib.ExitStack() as stack:
            if not enable_warnings:
                stack.enter_context(warnings.catch_warnings())
                warnings.simplefilter("ignore")
            request = rq.resolve_request(self, question, context, title, first_line_as_title, respect_sentence_boundaries, prepared)
            sharding = rq.enter_job_sharding(self, request, stack)
            total_jobs = sharding.total_jobs if sharding is not None else request.total_jobs
            thread_workers, preprocess_batch = rq.plan_host_stages(
                self, total_jobs, batch_size, splitter, preprocess_workers, preprocess_batch_size, torch_dataloader_kwargs, debug_callback)
            if prepared is not None:
                rq.run_prepared_request(self, request, run, batch_size)
            else:
                rq.run_raw_jobs(self, request, run, splitter, sharding.owned if sharding is not None else None, thread_workers,
                                preprocess_batch, batch_size, timing, strip_sentences=strip_sentences,
                                respect_sentence_boundaries=respect_sentence_boundaries)
            run.inference_seconds += self._flush_pending(run.pending)
            if show_progress and run.blocks and is_progress_bar_enabled():
                message = f"[OpenProvenceModel] Model inference time: {run.inference_seconds:.2f}s ({run.blocks} blocks)"
                if debug_callback is None:
                    print(message, flush=True)
                else:
                    debug_callback(message)
            result, post_time = rq.postprocess_and_gather(
                self, request, run, sharding, threshold=threshold, always_select_title=always_select_title,
                use_best_reranker_score=use_best_reranker_score, sentence_probability_groups_requested=return_sentence_metrics,
                collect_sentence_texts=return_sentence_texts, first_line_as_title=first_line_as_title,
                zero_score_when_empty=zero_score_when_empty)

        preprocess_time, inference_time, post_time = rq.owner_stage_seconds(
            self, start_total, run.assembly_seconds, (sum(timing.values()), run.inference_seconds, post_time))
        trace = ProcessPerformanceTrace(
            preprocess_seconds=preprocess_time, assembly_seconds=run.assembly_seconds, inference_seconds=inference_time,
            postprocess_seconds=post_time, total_seconds=perf_counter() - start_total, **timing)
        runtime = rq.runtime_facts(self, forward_stats, run.prepared_decisions)
        if runtime:
            object.__setattr__(trace, "runtime", runtime)  # (frozen dataclass: an attribute beside its ten fields)
        if debug_callback is not None:
            debug_callback(f"[OpenProvenceModel] Timing: preprocess={trace.preprocess_seconds:.2f}s assembly={trace.assembly_seconds:.2f}s "
                           f"inference={trace.inference_seconds:.2f}s postprocess={trace.postprocess_seconds:.2f}s "
                           f"total={trace.total_seconds:.2f}s")

        if reorder:
            result = pl.apply_reordering(result, top_k)
        pruned, scores, rates, kept, removed, title_out, probs = pl.shape_outputs(result, request.structure)
        payload: dict[str, Any] = {"pruned_context": pruned, "reranking_score": scores, "compression_rate": rates, "title": title_out,
                                   "timing": trace.as_dict(), "performance_trace": trace}
        if kept is not None:
            payload["kept_sentences"] = kept
        if removed is not None:
            payload["removed_sentences"] = removed
        if probs is not None:
            payload["sentence_probabilities"] = probs
        info = getattr(self, "_dist", None)
        if info and info["world"] > 1 and info["rank"] != info["dst"]:
            return None  # type: ignore[return-value]  # only the gather's destination rank holds the forward outputs
        return payload


def _remote_code_shim_source() -> str:
    from .hf_auto import SHIM_SOURCE

    return SHIM_SOURCE


class OpenProvenceForSequenceClassification(OpenProvenceModel):
    """AutoModel-style alias: ``.logits`` are the ranking logits (ref: standalone.py:3814-3831)."""


class OpenProvenceForTokenClassification(OpenProvenceModel):
    """``.logits`` are the per-token pruning logits; ``ranking_logits`` rides along (ref: standalone.py:3834-3901)."""

    def __init__(self, config: OpenProvenceConfig, **kwargs: Any) -> None:
        super().__init__(config, **kwargs)
        self.num_labels = config.num_pruning_labels

    def forward(self, input_ids=None, attention_mask=None, labels=None, return_dict=None, output_hidden_states=None,
                output_attentions=None, pooled_hidden_states=None, attention_rows=None, attention_rows_reduce_heads=False,
                **kwargs: Any):
        """The base forward without labels, as the reference runs it (standalone.py:3857-3863); with ``labels[B, L]`` (integer
        classes 0 / 1, -100 = ignored; CPU or device) ``loss`` is its ``CrossEntropyLoss`` over the pruning logits of the
        active positions (standalone.py:3870-3881) as a 0-dim fp32 device tensor.  ``op_loss`` reads the PACKED logits the
        forward left on the device with the forward's own ``cu_seqlens``: the active positions are the packed ones -- the
        ``attention_mask`` tokens, or every position without a mask.  A mask without any active position gives exactly 0.0
        (:3878-3879); active positions that are all -100 give NaN, as torch does.  ``return_dict=False`` returns
        ``(loss, pruning_logits)`` with labels, ``(pruning_logits,)`` without.  ``pooled_hidden_states`` / ``attention_rows`` /
        ``attention_rows_reduce_heads``: as in :meth:`OpenProvenceModel.forward`."""

        if input_ids is None:
            raise ValueError("input_ids must be provided")
        token_labels = None
        if labels is not None:
            token_labels = torch.as_tensor(labels)
            if token_labels.dtype.is_floating_point or token_labels.dtype.is_complex or token_labels.dtype == torch.bool:
                raise TypeError(f"token labels must be an integer tensor, got {token_labels.dtype}")
            if tuple(token_labels.shape) != tuple(input_ids.shape):
                raise ValueError(f"labels must have the shape of input_ids {tuple(input_ids.shape)}, got {tuple(token_labels.shape)}")
            token_labels = token_labels.detach().to(self._runtime_device)
        reduced: dict[str, Any] = {}
        rank, pruning_logits, hidden_states, attentions, packed = self._forward_padded(
            input_ids, attention_mask, output_hidden_states, output_attentions,
            reduced=self._reduced_requests(pooled_hidden_states, attention_rows, attention_rows_reduce_heads, reduced),
            token_loss=token_labels is not None)
        loss = None
        if token_labels is not None:
            prune, cu, total = packed
            if attention_mask is not None and total == 0:
                loss = torch.zeros((), dtype=torch.float32, device=pruning_logits.device)
            else:
                loss = self.encoder.loss("token_ce", prune, token_labels, cu=cu)
        if return_dict is not None and not return_dict:
            return (pruning_logits,) if loss is None else (loss, pruning_logits)
        return OpenProvenceOutput(
            loss=loss,
            logits=pruning_logits,
            pruning_logits=pruning_logits,
            ranking_logits=rank,
            hidden_states=hidden_states,
            attentions=attentions,
            pooled_hidden_states=reduced.get("pooled_hidden_states"),
            attention_rows=reduced.get("attention_rows"),
        )


# module-level helpers under the reference's names (its tests import these: tests/test_modeling_open_provence.py:11-29)
_FragmentRecord = FragmentRecord
_split_token_lists = pl.split_token_lists
_collect_candidate_sentences = pl.collect_candidate_sentences
_normalize_sentences = pl.normalize_sentences


def _tokenize_sentences_with_context(tokenizer, sentences, prefix_count, context_text, *, strip_sentences):
    return pl.tokenize_sentences(tokenizer, sentences)


def _fragmentize_example(
    example: dict[str, Any],
    tokenizer: Any,
    max_fragment_tokens: int,
    splitter: SentenceSplitter,
    strip_sentences: bool,
    *,
    respect_sentence_boundaries: bool = False,
) -> dict[str, Any]:
    """Sentences + fragments of one context, in the reference's dict shape (ref: _fragmentize_example :1146-1243)."""

    context_text = str(example.get("context_text", ""))
    if example.get("cached_sentences") is not None:
        sentences = [str(s) for s in example["cached_sentences"]]
    else:
        sentences = pl.normalize_sentences(pl.collect_candidate_sentences(example, splitter), context_text, strip_sentences)
    if example.get("cached_token_lists") is not None:
        token_lists = [[int(t) for t in ids] for ids in example["cached_token_lists"]]
    else:
        token_lists = pl.tokenize_sentences(tokenizer, sentences)
    if not pl.split_token_lists(token_lists, max_fragment_tokens, keep_sentence_boundaries=respect_sentence_boundaries):
        sentences = [pl.fallback_sentence(context_text, strip_sentences)]
    records = pl.fragmentize(
        tokenizer,
        token_lists,
        context_text,
        max_fragment_tokens,
        strip_sentences=strip_sentences,
        respect_sentence_boundaries=respect_sentence_boundaries,
    )
    return {
        "sentences": sentences,
        "fragment_texts": [r.text for r in records],
        "fragment_sentence_index": [r.sentence_index for r in records],
        "fragment_fragment_index": [r.fragment_index for r in records],
        "fragment_global_index": [r.global_index for r in records],
        "fragment_token_ids": [list(r.token_ids) for r in records],
    }


OpenProvenceEncoderConfig = OpenProvenceConfig
OpenProvenceEncoderForSequenceClassification = OpenProvenceForSequenceClassification
OpenProvenceEncoderForTokenClassification = OpenProvenceForTokenClassification

__all__ = [
    "OpenProvenceModel",
    "OpenProvenceRawPrediction",
    "OpenProvenceConfig",
    "OpenProvenceForSequenceClassification",
    "OpenProvenceForTokenClassification",
]
