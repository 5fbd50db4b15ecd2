"""The evaluation losses without a GPU: the float64 restatement the kernels are compared with (tests/loss_model.py) held
against torch's own losses in float64, called as the reference's inference file calls them (standalone.py:1709-1716,
3871-3881; losses.py:56-57); the mistakes a kernel could make shown to move that restatement; and ``op_loss`` -- declared,
bound, exported, additive to ABI 10 -- refusing every malformed request before it looks at the handle.

The bound between the restatement and torch: both are float64 evaluations of a mean of non-negative terms in a stable form,
a few roundings of 2^-53 apart per term and in the sum -- ``2^-50 * max(1, |value|)``, 8 units in the last place."""

import ctypes
import re
from pathlib import Path

import numpy as np
import pytest
import torch

import loss_model as lm
from open_provence_amd import _lib

HEADER = Path(__file__).resolve().parents[1] / "include" / "open_provence_hip.h"


def _bound(value: float) -> float:
    return 2.0**-50 * max(1.0, abs(value))


def _agree(got: float, want: float) -> bool:
    if np.isnan(want) or np.isnan(got):
        return bool(np.isnan(want) and np.isnan(got))
    return abs(got - want) <= _bound(want)


def _logit_sets(rng, shape):
    """fp32 logits: random, magnitude 80, magnitude 1e4, exact ties -- and all of them mixed."""

    random = rng.standard_normal(shape).astype(np.float32) * 3
    big = (rng.choice([-80.0, 80.0], size=shape) + rng.standard_normal(shape) * 0.5).astype(np.float32)
    huge = (rng.choice([-1e4, 1e4], size=shape) + rng.standard_normal(shape)).astype(np.float32)
    ties = np.broadcast_to(rng.standard_normal(shape[:-1] + (1,)).astype(np.float32), shape).copy()
    mixed = np.where(rng.random(shape[:-1] + (1,)) < 0.25, huge, np.where(rng.random(shape[:-1] + (1,)) < 0.3, ties, random))
    exact = rng.choice(np.array([-1e4, -80.0, 0.0, 80.0, 1e4], dtype=np.float32), size=shape)
    return {"random": random, "80": big, "1e4": huge, "ties": ties, "mixed": mixed.astype(np.float32), "exact": exact}


def _torch_token_loss(pruning_logits, labels, attention_mask):
    """standalone.py:3871-3881 in float64."""

    loss_fct = torch.nn.CrossEntropyLoss()
    pruning_logits = torch.from_numpy(np.asarray(pruning_logits, dtype=np.float64))
    labels = torch.from_numpy(np.asarray(labels, dtype=np.int64))
    if attention_mask is not None:
        active_loss = torch.from_numpy(np.asarray(attention_mask)).view(-1) == 1
        active_logits = pruning_logits.view(-1, 2)[active_loss]
        active_labels = labels.view(-1)[active_loss]
        if active_logits.numel() > 0:
            return float(loss_fct(active_logits, active_labels))
        return 0.0
    return float(loss_fct(pruning_logits.view(-1, 2), labels.view(-1)))


def _ragged_mask(lengths, width):
    return (np.arange(width)[None, :] < np.asarray(lengths)[:, None]).astype(np.int64)


def test_token_loss_restatement_is_torchs_in_float64():
    rng = np.random.default_rng(11)
    n_rows, width = 9, 37
    lengths = np.array([37, 0, 1, 20, 36, 5, 37, 13, 2])
    mask = _ragged_mask(lengths, width)
    for name, logits in _logit_sets(rng, (n_rows, width, 2)).items():
        labels = rng.integers(0, 2, size=(n_rows, width))
        sprinkled = np.where(rng.random((n_rows, width)) < 0.3, -100, labels)
        for tag, y in (("plain", labels), ("sprinkled", sprinkled), ("all ignored", np.full_like(labels, -100))):
            for m in (mask, None):
                want = _torch_token_loss(logits, y, m)
                got, terms, count = lm.token_ce_padded(logits, y, m)
                assert _agree(got, want), (name, tag, m is None, got, want)
                if tag == "all ignored":
                    assert np.isnan(got) and count == 0
            # the packed form the kernel reads gives the same number as the padded one
            packed, cu = lm.pack(logits, lengths)
            value, terms, count = lm.token_ce(packed, y, cu)
            assert _agree(value, _torch_token_loss(logits, y, mask)), (name, tag)
            assert terms.shape == (int(lengths.sum()),) and (terms >= 0).all()
            assert count == int((np.concatenate([y[r, : lengths[r]] for r in range(n_rows)]) != -100).sum())
    # a mask without any active position: exactly 0.0 (standalone.py:3878-3879); without a mask an empty batch is torch's NaN
    logits = rng.standard_normal((3, 5, 2)).astype(np.float32)
    labels = rng.integers(0, 2, size=(3, 5))
    empty = np.zeros((3, 5), dtype=np.int64)
    assert _torch_token_loss(logits, labels, empty) == 0.0 == lm.token_ce_padded(logits, labels, empty)[0]
    assert np.isnan(lm.token_ce(np.zeros((0, 2), np.float32), labels, np.zeros(4, np.int32))[0])
    assert np.isnan(_torch_token_loss(logits[:0], labels[:0], None)) and np.isnan(lm.token_ce_padded(logits[:0], labels[:0], None)[0])


def test_ranking_loss_restatements_are_torchs_in_float64():
    rng = np.random.default_rng(12)
    n = 301
    for name, logits in _logit_sets(rng, (n, 1)).items():
        labels = torch.from_numpy(rng.integers(0, 2, size=n))
        soft = torch.from_numpy(rng.random(n))
        for y in (labels, soft):
            # standalone.py:1710-1711: loss_fct(ranking_logits.view(-1), labels.float())
            target = y.float()
            want = float(torch.nn.BCEWithLogitsLoss()(torch.from_numpy(logits.astype(np.float64)).view(-1), target.double()))
            got, terms, count = lm.rank_bce(logits, target.numpy())
            assert _agree(got, want), (name, got, want)
            assert count == n and terms.shape == (n,)
    for C in (2, 3, 5):
        for name, logits in _logit_sets(rng, (n, C)).items():
            labels = rng.integers(0, C, size=(n, 1))
            sprinkled = np.where(rng.random((n, 1)) < 0.3, -100, labels)
            for y in (labels, sprinkled, np.full_like(labels, -100)):
                # standalone.py:1713-1716: loss_fct(ranking_logits.view(-1, num_labels), labels.view(-1))
                want = float(torch.nn.CrossEntropyLoss()(torch.from_numpy(logits.astype(np.float64)).view(-1, C), torch.from_numpy(y).view(-1)))
                got, terms, count = lm.rank_ce(logits, y)
                assert _agree(got, want), (C, name, got, want)
                assert count == int((y != -100).sum())
    for C in (1, 3):
        for name, logits in _logit_sets(rng, (n, C)).items():
            target = rng.standard_normal((n, C)).astype(np.float32)
            want = float(torch.nn.MSELoss()(torch.from_numpy(logits.astype(np.float64)), torch.from_numpy(target.astype(np.float64))))
            got, terms, count = lm.rank_mse(logits, target)
            assert _agree(got, want), (C, name, got, want)
            assert count == n * C
    assert np.isnan(lm.rank_bce(np.zeros(0, np.float32), np.zeros(0, np.float32))[0])
    assert np.isnan(lm.rank_mse(np.zeros((0, 3), np.float32), np.zeros((0, 3), np.float32))[0])
    assert np.isnan(float(torch.nn.BCEWithLogitsLoss()(torch.zeros(0, dtype=torch.float64), torch.zeros(0, dtype=torch.float64))))


def test_each_mistake_moves_the_restatement():
    rng = np.random.default_rng(13)
    n_rows, width = 6, 21
    lengths = np.array([21, 3, 0, 17, 9, 21])
    mask = _ragged_mask(lengths, width)
    sets = _logit_sets(rng, (n_rows, width, 2))
    labels = rng.integers(0, 2, size=(n_rows, width))
    sprinkled = np.where(rng.random((n_rows, width)) < 0.3, -100, labels)

    def moved(good, bad):
        return not _agree(bad, good) and not (np.isnan(good) and np.isnan(bad))

    # the mean over all positions instead of the non-ignored ones
    logits = sets["random"]
    packed, cu = lm.pack(logits, lengths)
    assert moved(lm.token_ce(packed, sprinkled, cu)[0], lm.token_ce(packed, sprinkled, cu, mutate="mean_over_all")[0])
    one_ignored = np.where(np.arange(n_rows) == 1, -100, labels[:, 0])
    assert moved(lm.rank_ce(logits[:, 0], one_ignored)[0], lm.rank_ce(logits[:, 0], one_ignored, mutate="mean_over_all")[0])
    # padding counted as active (the padded logits are zeros there, the labels are not ignored)
    padded = logits * mask[:, :, None]
    assert moved(lm.token_ce_padded(padded, labels, mask)[0], lm.token_ce_padded(padded, labels, mask, mutate="padding_active")[0])
    # lse - z_y without subtracting the maximum, on the 1e4 logits: exp overflows
    packed, cu = lm.pack(sets["1e4"], lengths)
    good, bad = lm.token_ce(packed, labels, cu)[0], lm.token_ce(packed, labels, cu, mutate="raw_lse")[0]
    assert np.isfinite(good) and (not np.isfinite(bad) or moved(good, bad))
    rank = sets["1e4"][:, :5, :].reshape(n_rows * 2, 5)
    y = rng.integers(0, 5, size=n_rows * 2)
    good, bad = lm.rank_ce(rank, y)[0], lm.rank_ce(rank, y, mutate="raw_lse")[0]
    assert np.isfinite(good) and (not np.isfinite(bad) or moved(good, bad))
    # BCE without the max(z, 0) term
    z = sets["random"][:, :, 0].reshape(-1)
    target = rng.random(z.shape[0]).astype(np.float32)
    assert moved(lm.rank_bce(z, target)[0], lm.rank_bce(z, target, mutate="bce_no_max")[0])
    # label columns offset by one row
    packed, cu = lm.pack(logits, lengths)
    assert moved(lm.token_ce(packed, labels, cu)[0], lm.token_ce(packed, labels, cu, mutate="label_row_offset")[0])
    assert moved(lm.rank_ce(logits[:, 0], labels[:, 0])[0], lm.rank_ce(logits[:, 0], labels[:, 0], mutate="label_row_offset")[0])


def test_the_call_is_declared_and_the_abi_version_stays(hip_library):
    assert _lib.OP_ABI_VERSION == 10 == hip_library.op_abi_version()
    text = re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)
    assert "#define OP_ABI_VERSION 10" in text
    assert "op_loss" in _lib.EXPORTED_SYMBOLS and re.search(r"\bint op_loss\s*\(", text)
    assert hasattr(hip_library, "op_loss") and len(hip_library.op_loss.argtypes) == 5
    assert hip_library.op_loss.argtypes[1] is ctypes.POINTER(_lib.OpLossRequest)
    assert hip_library.op_loss.argtypes[3] is ctypes.POINTER(_lib.OpLossReport)
    # request: 2 x 4, 2 pointers, 6 x 4, pointer, int64, pointer = 72 bytes; report: 4 x 4, 2 x int64, double, float + 4 = 48
    assert ctypes.sizeof(_lib.OpLossRequest) == 72 and _lib.OpLossRequest.ignore_index.offset == 56
    assert ctypes.sizeof(_lib.OpLossReport) == 48 and _lib.OpLossReport.sum.offset == 32
    assert _lib.LOSS_KINDS == {"token_ce": 0, "rank_bce": 1, "rank_ce": 2, "rank_mse": 3}
    assert _lib.OP_LABELS_F32 == 3 and _lib.OP_LABELS_F32 not in (_lib.OP_INT_I32, _lib.OP_INT_I64, _lib.OP_INT_U8)
    for value, name in ((0, "OP_LOSS_TOKEN_CE"), (1, "OP_LOSS_RANK_BCE"), (2, "OP_LOSS_RANK_CE"), (3, "OP_LOSS_RANK_MSE"), (3, "OP_LABELS_F32")):
        assert re.search(rf"\b{name} = {value}\b", text), name


# (never dereferenced: every call below is refused before the handle, let alone a device, is touched)
_BUF = 0x1000

_TOKEN = dict(kind=_lib.OP_LOSS_TOKEN_CE, labels_dtype=_lib.OP_INT_I64, n_rows=4, width=6, channels=2, total_tokens=17, cu_seqlens_dev=_BUF)
_BCE = dict(kind=_lib.OP_LOSS_RANK_BCE, labels_dtype=_lib.OP_LABELS_F32, n_rows=4, channels=1)
_CE = dict(kind=_lib.OP_LOSS_RANK_CE, labels_dtype=_lib.OP_INT_I32, n_rows=4, channels=3)
_MSE = dict(kind=_lib.OP_LOSS_RANK_MSE, labels_dtype=_lib.OP_LABELS_F32, n_rows=4, channels=3)


def _loss(lib, base, *, request=True, struct_bytes=None, report=None, report_bytes=None, loss=_BUF, **fields):
    req = _lib.OpLossRequest()
    req.struct_bytes = ctypes.sizeof(_lib.OpLossRequest) if struct_bytes is None else struct_bytes
    req.logits_dev, req.labels_dev, req.ignore_index = _BUF, _BUF, -100
    for k, v in {**base, **fields}.items():
        setattr(req, k, v)
    rep = None
    if report:
        rep = _lib.OpLossReport()
        rep.struct_bytes = ctypes.sizeof(_lib.OpLossReport) if report_bytes is None else report_bytes
    return lib.op_loss(None, ctypes.byref(req) if request else None, ctypes.c_void_p(loss) if loss else None,
                       ctypes.byref(rep) if rep is not None else None, None)


def test_malformed_loss_requests_are_refused_before_the_handle(hip_library):
    lib = hip_library
    cases = [
        (_TOKEN, dict(request=False), "request is NULL"),
        (_TOKEN, dict(struct_bytes=12), "op_loss_request.struct_bytes"),
        (_TOKEN, dict(report=True, report_bytes=40), "op_loss_report.struct_bytes"),
        (_TOKEN, dict(kind=4), "unknown kind"),
        (_TOKEN, dict(kind=-1), "unknown kind"),
        (_TOKEN, dict(labels_dtype=7), "unknown labels_dtype"),
        (_TOKEN, dict(labels_dtype=-1), "unknown labels_dtype"),
        (_TOKEN, dict(labels_dtype=_lib.OP_INT_U8), "does not fit"),
        (_TOKEN, dict(labels_dtype=_lib.OP_LABELS_F32), "does not fit"),
        (_CE, dict(labels_dtype=_lib.OP_LABELS_F32), "does not fit"),
        (_BCE, dict(labels_dtype=_lib.OP_INT_I64), "does not fit"),
        (_MSE, dict(labels_dtype=_lib.OP_INT_I32), "does not fit"),
        (_TOKEN, dict(n_rows=-1), "negative n_rows"),
        (_BCE, dict(n_rows=-3), "negative n_rows"),
        (_TOKEN, dict(width=-6), "negative width"),
        (_TOKEN, dict(total_tokens=-1), "negative total_tokens"),
        (_MSE, dict(channels=-1), "negative channels"),
        (_TOKEN, dict(channels=1), "channels"),
        (_TOKEN, dict(channels=3), "channels"),
        (_BCE, dict(channels=2), "channels"),
        (_BCE, dict(channels=0), "channels"),
        (_CE, dict(channels=1), "channels"),
        (_CE, dict(channels=0), "channels"),
        (_TOKEN, dict(n_rows=1 << 16, width=1 << 15), "n_rows * width"),
        (_TOKEN, dict(n_rows=(1 << 31) - 1, width=2), "n_rows * width"),
        (_MSE, dict(n_rows=1 << 30, channels=2), "n_rows * channels"),
        (_TOKEN, dict(total_tokens=25), "total_tokens"),
        (_TOKEN, dict(loss=None), "loss_dev"),
        (_TOKEN, dict(logits_dev=None), "logits_dev"),
        (_TOKEN, dict(labels_dev=None), "labels_dev"),
        (_TOKEN, dict(cu_seqlens_dev=None), "cu_seqlens_dev"),
        (_BCE, dict(logits_dev=None), "logits_dev"),
        (_CE, dict(labels_dev=None), "labels_dev"),
        (_MSE, dict(labels_dev=None), "labels_dev"),
    ]
    for base, kwargs, field in cases:
        assert _loss(lib, base, **kwargs) == _lib.OP_ERR_INVALID, kwargs
        message = _lib.last_error(lib, None)
        assert field in message and "NULL handle" not in message, (kwargs, message)
    # a well-formed request gets as far as the handle: every kind with every label type it takes, with and without a report or
    # terms, the largest batch, and the empty ones (whose buffers may be NULL)
    well_formed = [(_TOKEN, dict()), (_TOKEN, dict(labels_dtype=_lib.OP_INT_I32)), (_TOKEN, dict(report=True)), (_TOKEN, dict(terms_dev=_BUF)),
                   (_BCE, dict()), (_CE, dict()), (_CE, dict(labels_dtype=_lib.OP_INT_I64, channels=2)), (_MSE, dict()), (_MSE, dict(channels=1)),
                   (_TOKEN, dict(n_rows=(1 << 31) - 1, width=1)), (_TOKEN, dict(total_tokens=24)),
                   (_TOKEN, dict(n_rows=0, total_tokens=0, logits_dev=None, labels_dev=None, cu_seqlens_dev=None)),
                   (_TOKEN, dict(width=0, total_tokens=0, logits_dev=None, labels_dev=None)),
                   (_TOKEN, dict(total_tokens=0, logits_dev=None)),
                   (_BCE, dict(n_rows=0, logits_dev=None, labels_dev=None)), (_CE, dict(n_rows=0, logits_dev=None, labels_dev=None)),
                   (_MSE, dict(n_rows=0, logits_dev=None, labels_dev=None)), (_BCE, dict(width=-1, total_tokens=-1))]
    for base, kwargs in well_formed:
        assert _loss(lib, base, **kwargs) == _lib.OP_ERR_INVALID, kwargs
        assert "NULL handle" in _lib.last_error(lib, None), kwargs


def test_encoder_and_models_expose_the_loss():
    import inspect

    from open_provence_amd.engine import HipEncoder
    from open_provence_amd.modeling import OpenProvenceForTokenClassification, OpenProvenceModel

    params = inspect.signature(HipEncoder.loss).parameters
    assert list(params) == ["self", "kind", "logits", "labels", "cu", "width", "ignore_index", "terms", "check"]
    assert all(params[name].kind is inspect.Parameter.KEYWORD_ONLY for name in ("cu", "width", "ignore_index", "terms", "check"))
    assert (params["ignore_index"].default, params["terms"].default, params["check"].default) == (-100, False, True)
    for cls in (OpenProvenceModel, OpenProvenceForTokenClassification):
        assert "labels" in inspect.signature(cls.forward).parameters
        assert "NotImplementedError" not in inspect.getsource(cls.forward)
