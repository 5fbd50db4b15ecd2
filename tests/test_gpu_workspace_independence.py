"""The forward's outputs do not depend on what its workspace held before, and it writes nothing outside the workspace and its
output buffers (the contract stated at op_forward_packed in include/open_provence_hip.h).

The forward owns no memory: every intermediate buffer and row map is carved out of a workspace the caller allocates once and
reuses for every batch and kernel set.  What keeps stale content out of the outputs is a handful of clears and clamps in the
launch sequence (the tail rows of the attention output, the lo planes a policy does not carry, key tiles past the last row);
tests that run each case on a fresh allocation see zeros or finite leftovers there, which hide a missing one: a stale V^T row
under a zero probability is invisible when finite and fatal when NaN, a stale score in a running maximum is dropped when NaN
and fatal when huge.

Every assertion is the same: for each poisoned fill (tests/workspace_utils.py: ``nan``, ``huge``, wrong-but-in-range row
maps), the pruning logits, ranking logits, keep probabilities and every hidden state are ``torch.equal`` to those of the same
encoder and batch on a zeroed workspace -- bit identity, the kernels are deterministic -- and both guards of the workspace
and of every canaried output are untouched.  The reference is the same kernels on a clean workspace, which
tests/test_kernel_set_conformance.py ties to the float64 model; models, sets, flags and weights are imported from there, so
a new set or flag is covered here without an edit.

Batches: the smallest at which the invariant can break, from ROW_ALIGN 32, ROW_BM 128, the 64 / 128-key tiles, the 128 /
256-query blocks and the tiled path's rows + 64 -> 256 rule (TAILS, LIST, SHRINK, CHUNK_LENGTHS below).

Two things the code shows, which decide what can see a missing clear:

* On the row and panel paths only a FULL-attention layer reads keys past the last computed row (64-key tiles over 32-row
  alignment; a sliding-window layer's 32-key tiles end with the sequence), and what it reads there is the q / k / v^T the layer
  before it derived from the tail rows of the attention output.  The conformance models have their one global layer FIRST,
  where those rows still come from the embeddings: the tail clears of ChunkPass::prologue() are invisible on them.  The layer
  patterns of tests/test_kernel_set_geometry.py put a global layer behind another layer (test_global_layers_behind_another_layer).
* Under a pinned curated set the instantiated kernels have exactly the evaluated terms, so no clr_* clear runs at all; they run
  when a policy is evaluated on the all-terms kernels (OP_FLAG_NO_POLICY_KERNELS: test_cleared_operand_policies).  The planes
  they clear were written by the launch just before them, so the outputs cannot depend on stale content through a missing one:
  that is a departure from the policy's arithmetic, which tests/test_gpu_policy.py holds against the curated sets."""

from __future__ import annotations

import re
from pathlib import Path

import pytest
import torch

import test_kernel_set_conformance as conf
import test_kernel_set_geometry as geo
import workspace_utils as wu

pytestmark = pytest.mark.gpu

# the last sequence ends everywhere inside its final key tile; rows % 128 takes the values 32, 64, 96 and 0
TAIL_TOKENS = [1, 31, 32, 33, 63, 64, 65, 96, 97, 127, 128, 129]
TAILS = [[t, 0] for t in TAIL_TOKENS] + [[130, t] for t in TAIL_TOKENS]
LIST = list(conf.LENGTHS)  # 0 .. 700, empties included
SHRINK = [5, 0]  # after LIST on the same workspace, no refill: stale data of a larger geometry
CHUNK_ROWS, CHUNK_LENGTHS = 256, [257, 40, 300, 3, 0, 64]  # later, smaller chunks run over earlier chunks' leftovers
FLAG_TAILS = [b for t in (33, 65, 129) for b in ([t, 0], [130, t])]
SWITCH_MODELS = ["row", "panel512"]
PIPELINE_CASES = [("row", "f16"), ("panel512", "bf16x3")]
DIRECT_CASES = [("row", "f16"), ("row", "bf16x3"), ("panel512", "f16-f8-w+attn-f16"), ("tiled", "bf16x3")]


class Failures:
    """Collects every batch of a case that breaks the invariant; ``leaking_regions`` names the regions for the first one."""

    def __init__(self, label: str):
        self.label, self.lines = label, []

    def check(self, enc, rows, ref, got, what: str, pattern: str, *, runner=wu.run, diagnose: bool = True):
        assert all(bool(torch.isfinite(t.float()).all()) for t in ref if t is not None), f"{self.label} {what}: non-finite on a zeroed workspace"
        if wu.same(ref, got):
            return
        line = f"{what}: first difference at {wu.first_difference(ref, got, rows)}"
        if diagnose and not self.lines:
            leaks = wu.leaking_regions(enc, rows, pattern, runner)
            line += f"; regions whose content reaches an output in one forward of this batch: {leaks or 'none (only the sequence of forwards shows it)'}"
        self.lines.append(line)

    def done(self):
        assert not self.lines, f"{self.label}: outputs depend on what the workspace held before ({len(self.lines)} comparisons):\n  " + "\n  ".join(self.lines)


def _compare_fills(fails: Failures, enc, lengths, *, runner=wu.run):
    rows = conf._rows(lengths)
    ref = runner(enc, rows, "zeros")
    for pattern in wu.POISONS:
        fails.check(enc, rows, ref, runner(enc, rows, pattern), f"{lengths} on {pattern!r}", pattern, runner=runner)


def _encoder(model, kernel_set, flag=None, window=128, chunk_rows=None, weights=None):
    return conf._encoder(model, weights or conf.weights_for(kernel_set, "o1"), window, kernel_set, conf._flag_bits([flag] if flag else []),
                         chunk_rows=chunk_rows)


# -- the layout hook --------------------------------------------------------------------------------------------------------------
def _workspace_members() -> list[str]:
    """The pointer members of ``struct Workspace`` (op_forward.h), read from the source."""

    text = (Path(__file__).resolve().parents[1] / "open_provence_amd" / "csrc" / "op_forward.h").read_text()
    body = re.search(r"struct Workspace \{(.*?)\n\};", text, flags=re.S).group(1)
    body = re.sub(r"//[^\n]*", "", body)
    names = []
    for statement in body.split(";"):
        if "*" in statement:
            names += [re.findall(r"\w+", decl)[-1] for decl in statement.split(",")]
    return names


@pytest.mark.parametrize("model", ["row", "panel512", "tiled"])
def test_layout_is_what_carve_hands_out(model):
    enc = _encoder(model, "bf16x3")
    try:
        for n_seqs, total, max_len in [(2, 2, 1), (17, sum(LIST), max(LIST)), (2600, 40000, 300)]:
            layout = enc.workspace_layout(n_seqs, total, max_len)
            need = int(enc.lib.op_workspace_bytes(enc._handle, n_seqs, total, max_len))
            end = 0
            for region in layout:
                assert region["offset"] % 256 == 0 and region["bytes"] > 0 and region["kind"] in ("float", "index", "flag"), region
                assert region["offset"] == end, f"{region} does not start where the region before it ends ({end})"
                end = region["offset"] + (region["bytes"] + 255) // 256 * 256
            assert end == need
            names = [r["name"] for r in layout]
            assert len(set(names)) == len(names) and sorted(names) == sorted(_workspace_members())
            kinds = {r["name"]: r["kind"] for r in layout}
            assert kinds["x"] == "float" and kinds["row_tok"] == "index" and kinds["roff"] == "index" and kinds["range_flag"] == "flag"
            assert {n for n, k in kinds.items() if k == "index"} == {"row_seq", "row_pos", "row_tok", "roff", "qboff", "qboff_l"}
    finally:
        enc.close()


# -- 1. every set of every model, default flags ---------------------------------------------------------------------------------------
SET_CASES = [(m, s) for m in conf.MODELS for s in conf.SUPPORTED[m]]


@pytest.mark.parametrize("model,kernel_set", SET_CASES)
def test_tails_list_and_shrink(model, kernel_set):
    fails = Failures(f"{model} {kernel_set}")
    enc = _encoder(model, kernel_set)
    try:
        for lengths in TAILS + [LIST]:
            _compare_fills(fails, enc, lengths)
        small = conf._rows(SHRINK)
        ref = wu.run(enc, small, "zeros")
        for pattern in wu.POISONS:
            wu.run(enc, conf._rows(LIST), pattern)
            got = wu.run(enc, small, None)  # the workspace as the larger batch left it
            fails.check(enc, small, ref, got, f"{SHRINK} after {LIST} on {pattern!r}", pattern)
    finally:
        enc.close()
    fails.done()


@pytest.mark.parametrize("model,kernel_set", SET_CASES)
def test_chunks_run_over_earlier_chunks(model, kernel_set):
    fails = Failures(f"{model} {kernel_set} chunk_rows {CHUNK_ROWS}")
    enc = _encoder(model, kernel_set, chunk_rows=CHUNK_ROWS)
    try:
        _compare_fills(fails, enc, CHUNK_LENGTHS)
    finally:
        enc.close()
    fails.done()


# -- 2. the flag regimes ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model,flag,kernel_set", conf.FLAG_CASES)
def test_flag_regimes(model, flag, kernel_set):
    fails = Failures(f"{model} {kernel_set} {flag}")
    enc = _encoder(model, kernel_set, flag)
    try:
        for lengths in [LIST] + FLAG_TAILS:
            _compare_fills(fails, enc, lengths)
    finally:
        enc.close()
    fails.done()


# -- 3. the window moves kt_lo and kt_hi ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("window", [2, 30, 64, 200, 1024])
@pytest.mark.parametrize("model,kernel_set", conf.WINDOW_RUNS)
def test_windows(model, kernel_set, window):
    fails = Failures(f"{model} {kernel_set} window {window}")
    enc = _encoder(model, kernel_set, window=window)
    try:
        _compare_fills(fails, enc, LIST)
    finally:
        enc.close()
    fails.done()


# -- a global layer behind another layer; policies on the all-terms kernels --------------------------------------------------------------
@pytest.mark.parametrize("pattern", geo.LAYER_PATTERNS)
@pytest.mark.parametrize("model,kernel_set,flag", geo.PATTERN_CASES)
def test_global_layers_behind_another_layer(model, kernel_set, flag, pattern):
    fails = Failures(f"{model} {kernel_set} {flag or '-'} layers {pattern}")
    enc = conf._encoder(model, conf.weights_for(kernel_set, "o1"), 128, kernel_set, conf._flag_bits([flag] if flag else []),
                        dims=conf._dims(model, 128, layer_types=pattern))
    try:
        for lengths in TAILS + [LIST]:
            _compare_fills(fails, enc, lengths)
    finally:
        enc.close()
    fails.done()


@pytest.mark.parametrize("precision", ["bf16x2", "bf16"])
@pytest.mark.parametrize("model", SWITCH_MODELS)
def test_cleared_operand_policies(model, precision):
    """A policy with fewer terms than the all-terms kernels multiply by: every clr_* clear of the launch sequence runs."""

    from open_provence_amd.engine import HipEncoder

    fails = Failures(f"{model} {precision} on the all-terms kernels")
    enc = HipEncoder(conf._dims(model), device="cuda:0", precision=precision, flags=conf._flag_bits(["NO_POLICY_KERNELS"]))
    try:
        enc.load_state_dict(conf._state(model, "o1-bf16"), calibrate=False)
        assert enc.effective_policy()["kernel_set"].startswith("all-terms")
        for lengths in [LIST] + FLAG_TAILS:
            _compare_fills(fails, enc, lengths)
    finally:
        enc.close()
    fails.done()


# -- 4. switching sets on one handle and one workspace ----------------------------------------------------------------------------------
@pytest.mark.parametrize("first_fill", ["zeros", "nan"])
@pytest.mark.parametrize("model", SWITCH_MODELS)
def test_set_switching_over_real_stale_planes(model, first_fill):
    """bf16x3 writes every lo plane; each other set then runs over them with no refill, and must give what a fresh encoder of
    that set gives on zeros: real stale planes of another format under every set.  One checkpoint for all sets (O(1),
    fp32-valued)."""

    rows = conf._rows(LIST)
    fails = Failures(f"{model} set switching, first fill {first_fill!r}")
    enc = _encoder(model, "bf16x3", weights="o1")
    try:
        wu.run(enc, rows, first_fill)
        for kernel_set in [s for s in conf.SUPPORTED[model] if s != "bf16x3"]:
            fresh = _encoder(model, kernel_set, weights="o1")
            try:
                ref = wu.run(fresh, rows, "zeros")
            finally:
                fresh.close()
            enc.select_kernel_set(kernel_set)
            assert enc.effective_policy()["kernel_set"] == kernel_set
            got = wu.run(enc, rows, None)
            fails.check(enc, rows, ref, got, f"{kernel_set} after the sets before it", "nan", diagnose=False)
    finally:
        enc.close()
    fails.done()


# -- 5. the two pipelines ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model,kernel_set", PIPELINE_CASES)
def test_pipelines(model, kernel_set):
    rows = conf._rows(LIST)
    fails = Failures(f"{model} {kernel_set} pipelines")
    enc = _encoder(model, kernel_set)
    try:
        for part in (0, 1):
            ref = wu.run(enc, rows, "zeros", part=part)
            for pattern in wu.POISONS:
                fails.check(enc, rows, ref, wu.run(enc, rows, pattern, part=part), f"pipeline {part} on {pattern!r}", pattern, diagnose=False)
    finally:
        enc.close()
    fails.done()


# -- 6. the C ABI itself, every output between canaries ------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("padded", [False, True], ids=["packed", "padded"])
@pytest.mark.parametrize("model,kernel_set", DIRECT_CASES)
def test_direct_call_stays_inside_its_buffers(model, kernel_set, padded, dtype):
    def runner(enc, rows, fill, only=None):
        return wu.run_direct(enc, rows, fill, padded=padded, dtype=dtype, only=only)

    fails = Failures(f"{model} {kernel_set} direct {'padded' if padded else 'packed'} {dtype}")
    enc = _encoder(model, kernel_set)
    try:
        for lengths in (LIST, [130, 33]):
            _compare_fills(fails, enc, lengths, runner=runner)
    finally:
        enc.close()
    fails.done()
