"""Rows beyond 2048 tokens, up to max_position_embeddings = 8192, on every dispatch path against the float64 model of the
pinned kernel set's arithmetic (tests/arith_model.py): each hidden state, the pruning logits and the ranking logits, with the
statistic and the bounds of tests/test_kernel_set_conformance.py (``conf._compare``: 2 x RMS and 4 x max-abs of (model - exact),
the per-entry floors; hidden states travel padded).

What such rows reach and the 700- and 2048-token rows of that module do not: RoPE table rows 2048 .. 8191 and the position
clamp next to the last one, 33 to 128 key tiles per query block (the lazy softmax reference moves late in the row), 9 to 32 work
items of one sequence in the XCD-grouped block map, sliding-window tile ranges far from the row's start, a single sequence
larger than ``chunk_rows``.  tests/test_arith_model.py emulates the mistakes these rows are there for on the model's entries.

Lengths: LONG = 8192 (the last table row), 4097 (one token past 4096), 2049 (one past the old limit), 5 (a short neighbour);
MID leaves the 8192-token row out.  Weights: peaked, as ``conf.test_a_2048_token_row`` (the late-rescale branch runs).  The model
runs are cached per module by ``conf._model``; the table of results is printed when the module ends."""

from __future__ import annotations

import pytest
import torch

import arith_model as am
import test_kernel_set_conformance as conf

pytestmark = pytest.mark.gpu

MAX_POSITIONS = 8192
LONG = (8192, 4097, 2049, 5)
MID = (4097, 2049, 5)
SWEEP_ROWS = (2049, 5)
GROUPED_ROWS = (8192, 5)  # 8192 tokens of one sequence: 32 work items under the grouped block map of the panel path

# (model, kernel set, flags, rows)
CASES = (
    [("row", s, (), LONG) for s in ("bf16x3", "f16-f8-w", "f16")]
    + [("row", "f16", ("NO_LAYER_PAIRS",), MID)]
    + [("panel512", s, (), MID) for s in ("bf16x3", "f16", "f16-f8-w+attn-f16")]
    + [("panel512", "f16", (), GROUPED_ROWS)]
    + [("tiled", "bf16x3", (), MID)]
)
# the window sweep at depth: (model, kernel set, window)
WINDOW_CASES = [(m, s, w) for m, s in (("row", "f16"), ("panel512", "bf16x3")) for w in (2, 1024)]
CHUNK_ROWS = 256  # every sequence of LONG but the 5-token one exceeds it

_FIRST_LINE = [0]


@pytest.fixture(scope="module", autouse=True)
def _print_table():
    _FIRST_LINE[0] = len(conf.TABLE)
    yield
    print("\n[long rows] model     set                      flags              weights        window rows  | worst ratio to the bound: "
          "over the entries that check a rounding scheme (hidden_0: the fp32 floor) | the kernel against exact")
    for line in conf.TABLE[_FIRST_LINE[0]:]:
        print("[long rows]", line)


def _rows_label(lengths) -> str:
    return "+".join(str(n) for n in lengths)


def _check(model, kernel_set, flag_names, window, lengths, *, chunk_rows=None, compare=True):
    """``conf._check`` on a handle that takes rows of MAX_POSITIONS tokens, peaked weights; returns the kernel's entries."""

    weights = conf.weights_for(kernel_set, "peaked")
    dims = conf._dims(model, window, max_position_embeddings=MAX_POSITIONS)
    enc = conf._encoder(model, weights, window, kernel_set, conf._flag_bits(flag_names), chunk_rows=chunk_rows, dims=dims)
    try:
        got = conf._run(enc, conf._rows(lengths))
        after = enc.effective_policy()["kernel_set"]
    finally:
        enc.close()
    label = (f"{model:9s} {kernel_set:24s} {'+'.join(flag_names) or '-':18s} {weights:14s} w{window:<5d} {_rows_label(lengths)}"
             + (f" chunk_rows {chunk_rows}" if chunk_rows else ""))
    assert after == kernel_set, f"{label}: the forward ran on {after}"
    if compare:
        own = conf._model(model, weights, window, lengths, kernel_set)
        exact = conf._model(model, weights, window, lengths, "exact")
        base_set = am.BASE_SET.get(kernel_set)
        base = conf._model(model, weights, window, lengths, base_set) if base_set else None
        conf._compare(label, got, own, exact, f"hidden_{conf.SHAPES[model][3]}", base)
    return got


@pytest.mark.parametrize("model,kernel_set,flags,lengths", CASES,
                         ids=[f"{m}-{s}-{'+'.join(f) or 'default'}-{_rows_label(l)}" for m, s, f, l in CASES])
def test_long_rows_match_the_model(model, kernel_set, flags, lengths):
    _check(model, kernel_set, list(flags), 128, lengths)


@pytest.mark.parametrize("model,kernel_set,window", WINDOW_CASES)
def test_window_at_depth_matches_the_model(model, kernel_set, window):
    _check(model, kernel_set, [], window, SWEEP_ROWS)


def test_sequences_larger_than_a_chunk_are_bit_identical_to_one_chunk():
    """chunk_rows 256 on LONG: the 8192-, 4097- and 2049-token sequences each exceed the chunk and get one of their own.  Every
    entry is bit for bit the one-chunk run's, which test_long_rows_match_the_model compares with the model."""

    whole = _check("row", "bf16x3", [], 128, LONG, compare=False)
    chunked = _check("row", "bf16x3", [], 128, LONG, chunk_rows=CHUNK_ROWS, compare=False)
    assert set(whole) == set(chunked)
    differing = {}
    for name in whole:
        assert whole[name].shape == chunked[name].shape, name
        n = int((whole[name] != chunked[name]).sum()) if not torch.equal(whole[name], chunked[name]) else 0
        if n:
            differing[name] = (n, whole[name].numel(), float((whole[name] - chunked[name]).abs().max()))
    line = (f"{'row':9s} {'bf16x3':24s} {'-':18s} {'peaked':14s} w128   {_rows_label(LONG)} chunk_rows {CHUNK_ROWS} | entries not "
            f"bit-identical to one chunk: {differing or 'none'}")
    conf.TABLE.append(line)
    print("[long rows]", line)
    assert not differing, f"chunk_rows {CHUNK_ROWS} changed (entries, of, max |difference|): {differing}"
