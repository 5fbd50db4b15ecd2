"""The two reductions of ``op_forward_packed_pooled`` / ``op_attention_rows`` restated in float64 (test infrastructure), the
distance the GPU tests measure them by, and three wrong restatements that the distance must tell apart.

The bound is derived, not measured: an fp64 sum of at most 8192 fp32 values is wrong by at most ~8192 x 2^-53 ~ 1e-12 relative
to the sum of magnitudes, far below half an fp32 ulp (6e-8) unless the mean cancels to nothing; one rounding to fp32 follows.  Two
such results, each a correctly rounded neighbour of the exact mean, are at most 1 fp32 ulp apart."""

from __future__ import annotations

import numpy as np

ULP_BOUND = 1.0


def pooled_first(entry: np.ndarray, cu: np.ndarray) -> np.ndarray:
    """``entry[T, H]`` fp32, ``cu[B + 1]`` -> ``[B, H]`` fp32: the row of token 0 of each sequence, +0.0 for an empty one."""

    out = np.zeros((len(cu) - 1, entry.shape[1]), dtype=np.float32)
    for s in range(len(cu) - 1):
        if cu[s + 1] > cu[s]:
            out[s] = entry[cu[s]]
    return out


def pooled_mean(entry: np.ndarray, cu: np.ndarray) -> np.ndarray:
    """``[B, H]`` fp32: the float64 mean over each sequence's tokens of the fp32 rows, rounded once; +0.0 for an empty one."""

    out = np.zeros((len(cu) - 1, entry.shape[1]), dtype=np.float32)
    for s in range(len(cu) - 1):
        if cu[s + 1] > cu[s]:
            out[s] = (entry[cu[s]: cu[s + 1]].astype(np.float64).sum(axis=0) / float(cu[s + 1] - cu[s])).astype(np.float32)
    return out


def head_mean(rows: np.ndarray) -> np.ndarray:
    """``rows[B, heads, W]`` fp32 -> ``[B, W]`` fp32: the float64 mean over heads, rounded once."""

    return (rows.astype(np.float64).sum(axis=1) / float(rows.shape[1])).astype(np.float32)


# ---- wrong restatements: what a plausible kernel bug computes ------------------------------------------------------------------
def pooled_mean_length_rounded_up(entry: np.ndarray, cu: np.ndarray, unit: int = 32) -> np.ndarray:
    """The mean over the length rounded up to the row alignment (dividing by the allocated rows)."""

    out = np.zeros((len(cu) - 1, entry.shape[1]), dtype=np.float32)
    for s in range(len(cu) - 1):
        n = int(cu[s + 1] - cu[s])
        if n:
            out[s] = (entry[cu[s]: cu[s + 1]].astype(np.float64).sum(axis=0) / float((n + unit - 1) // unit * unit)).astype(np.float32)
    return out


def pooled_mean_without_last_token(entry: np.ndarray, cu: np.ndarray) -> np.ndarray:
    """The sum stops one token early (an off-by-one in the last partial); still divided by the length."""

    out = np.zeros((len(cu) - 1, entry.shape[1]), dtype=np.float32)
    for s in range(len(cu) - 1):
        n = int(cu[s + 1] - cu[s])
        if n:
            out[s] = (entry[cu[s]: cu[s + 1] - 1].astype(np.float64).sum(axis=0) / float(n)).astype(np.float32)
    return out


def head_mean_one_head_missing(rows: np.ndarray) -> np.ndarray:
    """The last head never enters the sum; still divided by the number of heads."""

    return (rows[:, :-1].astype(np.float64).sum(axis=1) / float(rows.shape[1])).astype(np.float32)


def ulp_distance(got: np.ndarray, want: np.ndarray) -> float:
    """max over elements of ``|got - want|`` in units of the fp32 spacing at ``want`` (``want`` = the restatement, fp32)."""

    got, want = np.asarray(got, dtype=np.float32), np.asarray(want, dtype=np.float32)
    assert got.shape == want.shape, (got.shape, want.shape)
    if got.size == 0:
        return 0.0
    spacing = np.spacing(np.abs(want)).astype(np.float64)
    return float((np.abs(got.astype(np.float64) - want.astype(np.float64)) / spacing).max())
