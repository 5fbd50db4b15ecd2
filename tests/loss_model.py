"""A numpy float64 restatement of the four losses ``op_loss`` computes (include/open_provence_hip.h), as the reference's
inference file calls them (standalone.py:1709-1716, 3871-3881) plus the ranking term of its training objective
(losses.py:56-57): the stable form of every term, ``ignore_index``, the active set, the zero-count rules and the per-element
terms.  Terms are float64 from the inputs as given (the kernels' inputs are fp32: pass fp32 arrays, they are widened
exactly); the terms that count are added exactly (``math.fsum``) and divided once.

Every function returns ``(value, terms, count)``: the mean as a Python float (NaN for a count of zero, as torch's mean of
nothing), the unreduced float64 terms (+0.0 where the label is ignored) and the number of terms behind the mean.

``mutate`` names one deliberate mistake (tests/test_loss_model.py shows that each moves the value): the model is only worth
comparing a kernel with if the things a kernel can get wrong are visible in it.
"""

from __future__ import annotations

import math

import numpy as np

IGNORE_INDEX = -100
MUTATIONS = ("mean_over_all", "padding_active", "raw_lse", "bce_no_max", "label_row_offset")


def softplus(d: np.ndarray) -> np.ndarray:
    """log(1 + e^d) without overflow or cancellation."""

    d = np.asarray(d, dtype=np.float64)
    return np.maximum(d, 0.0) + np.log1p(np.exp(-np.abs(d)))


def _mean(terms: np.ndarray, counted: np.ndarray, count: "int | None" = None) -> "tuple[float, int]":
    count = int(counted.sum()) if count is None else int(count)
    picked = terms[counted]
    # (fsum refuses inf - inf; a non-finite term makes the sum what IEEE addition makes it)
    with np.errstate(invalid="ignore"):
        total = math.fsum(float(t) for t in picked) if np.isfinite(picked).all() else float(np.sum(picked))
    return (total / count if count else float("nan")), count


def cross_entropy_terms(logits: np.ndarray, labels: np.ndarray, *, raw_lse: bool = False) -> np.ndarray:
    """Cross entropy of each row of ``logits[n, C]`` against ``labels[n]`` (every label inside 0 <= y < C): log-sum-exp after
    subtracting the row maximum, ``log1p(sum of the other classes' exp(z_c - max)) + (max - z_label)``; for two classes that
    is ``softplus(z_other - z_label)``, which is the form used then."""

    z = np.asarray(logits, dtype=np.float64)
    y = np.asarray(labels, dtype=np.int64)
    rows = np.arange(z.shape[0])
    if raw_lse:  # the mistake: lse - z_y on the raw logits
        with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
            return np.log(np.exp(z).sum(axis=1)) - z[rows, y]
    if z.shape[1] == 2:
        return softplus(z[rows, 1 - y] - z[rows, y])
    # (the maximum's own exp(0) is the 1 of log1p: log(1 + 4e-35) would be 0, and for C = 2 this is the softplus above)
    at = z.argmax(axis=1)
    top = z[rows, at]
    rest = np.exp(z - top[:, None])
    rest[rows, at] = 0.0
    return np.log1p(rest.sum(axis=1)) + (top - z[rows, y])


def token_ce(packed_logits: np.ndarray, labels: np.ndarray, cu: np.ndarray, ignore_index: int = IGNORE_INDEX, mutate: "str | None" = None):
    """OP_LOSS_TOKEN_CE: ``packed_logits[T, 2]``, padded ``labels[n_rows, width]``, ``cu[n_rows + 1]``; token t of row r reads
    ``labels[r][t - cu[r]]``.  Mean over the tokens whose label is not ``ignore_index``; ``terms[T]``."""

    z = np.asarray(packed_logits, dtype=np.float64).reshape(-1, 2)
    labels = np.asarray(labels, dtype=np.int64)
    cu = np.asarray(cu, dtype=np.int64)
    n_rows = labels.shape[0]
    if mutate == "label_row_offset":  # the mistake: row r reads the label row of r + 1
        labels = np.roll(labels, -1, axis=0)
    y = (np.concatenate([labels[r, : cu[r + 1] - cu[r]] for r in range(n_rows)]) if n_rows else np.zeros(0, dtype=np.int64))
    assert y.shape[0] == z.shape[0] == (cu[-1] if n_rows else 0)
    counted = y != ignore_index
    terms = np.zeros(z.shape[0], dtype=np.float64)
    terms[counted] = cross_entropy_terms(z[counted], y[counted], raw_lse=mutate == "raw_lse")
    value, count = _mean(terms, counted, z.shape[0] if mutate == "mean_over_all" else None)
    return value, terms, count


def token_ce_padded(pruning_logits: np.ndarray, labels: np.ndarray, attention_mask: "np.ndarray | None",
                    ignore_index: int = IGNORE_INDEX, mutate: "str | None" = None):
    """The token-classification forward's loss (standalone.py:3871-3881) from its PADDED ``pruning_logits[B, L, 2]``: the
    active positions are ``attention_mask == 1`` (every position without a mask); a mask without any active position gives
    exactly 0.0 -- the one place the reference leaves torch's NaN.  ``terms`` has one entry per active position."""

    z = np.asarray(pruning_logits, dtype=np.float64).reshape(-1, 2)
    y = np.asarray(labels, dtype=np.int64).reshape(-1)
    if mutate == "label_row_offset":
        y = np.roll(np.asarray(labels, dtype=np.int64), -1, axis=0).reshape(-1)
    if attention_mask is not None and mutate != "padding_active":  # (the mistake: padding counts as active)
        active = np.asarray(attention_mask).reshape(-1) == 1
        if not active.any():
            return 0.0, np.zeros(0, dtype=np.float64), 0
        z, y = z[active], y[active]
    counted = y != ignore_index
    terms = np.zeros(z.shape[0], dtype=np.float64)
    terms[counted] = cross_entropy_terms(z[counted], y[counted], raw_lse=mutate == "raw_lse")
    value, count = _mean(terms, counted, z.shape[0] if mutate == "mean_over_all" else None)
    return value, terms, count


def rank_bce(logits: np.ndarray, labels: np.ndarray, mutate: "str | None" = None):
    """OP_LOSS_RANK_BCE: ``max(z, 0) - z y + log1p(exp(-|z|))`` of ``logits[n]`` against fp ``labels[n]``, mean over n."""

    z = np.asarray(logits, dtype=np.float64).reshape(-1)
    y = np.asarray(labels, dtype=np.float64).reshape(-1)
    # (left to right, as written: at z = 80, y = 1 the first two terms cancel exactly and the tail of 1.8e-35 is the loss)
    head = -z * y if mutate == "bce_no_max" else np.maximum(z, 0.0) - z * y  # (the mistake: the max(z, 0) term left out)
    terms = head + np.log1p(np.exp(-np.abs(z)))
    value, count = _mean(terms, np.ones(z.shape[0], dtype=bool))
    return value, terms, count


def rank_ce(logits: np.ndarray, labels: np.ndarray, ignore_index: int = IGNORE_INDEX, mutate: "str | None" = None):
    """OP_LOSS_RANK_CE: ``logits[n, C]`` against integer ``labels[n]``, mean over the rows whose label is not ``ignore_index``."""

    z = np.asarray(logits, dtype=np.float64)
    y = np.asarray(labels, dtype=np.int64).reshape(-1)
    if mutate == "label_row_offset":
        y = np.roll(y, -1)
    counted = y != ignore_index
    terms = np.zeros(z.shape[0], dtype=np.float64)
    terms[counted] = cross_entropy_terms(z[counted], y[counted], raw_lse=mutate == "raw_lse")
    value, count = _mean(terms, counted, z.shape[0] if mutate == "mean_over_all" else None)
    return value, terms, count


def rank_mse(logits: np.ndarray, labels: np.ndarray):
    """OP_LOSS_RANK_MSE: ``(z - y)^2`` of ``logits[n, C]`` against ``labels[n, C]``, mean over n * C."""

    z = np.asarray(logits, dtype=np.float64)
    y = np.asarray(labels, dtype=np.float64)
    terms = (z - y) ** 2
    value, count = _mean(terms.reshape(-1), np.ones(terms.size, dtype=bool))
    return value, terms, count


def pack(padded: np.ndarray, lengths) -> "tuple[np.ndarray, np.ndarray]":
    """Rows of ``padded[n_rows, width, ...]`` cut to ``lengths`` and laid end to end, with their ``cu_seqlens`` (int32)."""

    lengths = np.asarray(lengths, dtype=np.int64)
    cu = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int32)
    rows = [padded[r, : lengths[r]] for r in range(len(lengths))]
    packed = np.concatenate(rows) if rows else padded.reshape((0,) + padded.shape[2:])
    return packed, cu


def ulp32(value: float) -> float:
    """One fp32 unit in the last place at ``value``, at least one fp32 subnormal step."""

    return float(max(np.spacing(np.float32(abs(value))), np.float32(1.401298464324817e-45)))
