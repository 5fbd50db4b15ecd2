"""Token-budgeted forwards of ``process()``: the planner (``pipeline.plan_forward_chunks``), its wiring on a model without
a GPU, and the rule that a replaced forward keeps the reference's contract of at most ``batch_size`` rows per call."""

import json
import math

import numpy as np
import pytest
import torch

from helpers import (
    GOLDEN_DIR,
    CharTokenizer,
    assert_process_result_matches,
    golden_stub_forward,
    host_only_model,
    period_splitter,
)
from open_provence_amd.pipeline import plan_forward_chunks

TIMING_KEYS = {
    "preprocess_seconds", "assembly_seconds", "inference_seconds", "postprocess_seconds", "total_seconds",
    "sentence_collect_seconds", "sentence_normalize_seconds", "tokenize_seconds", "fragment_split_seconds",
    "fragment_decode_seconds",
}


def _cost(length):
    return math.ceil(length / 32) * 32


def _fixed_stride(n, batch_size):
    return [(s, min(s + batch_size, n)) for s in range(0, n, batch_size)]


def _length_lists():
    rng = np.random.default_rng(20240611)
    lists = [[], [0], [5], [5000], [0, 0, 0, 0, 0], [32] * 70, [33] * 70, [2048] * 64]
    for _ in range(60):
        n = int(rng.integers(1, 400))
        kind = int(rng.integers(0, 4))
        if kind == 0:
            lengths = rng.integers(0, 140, n)  # short contexts, some empty
        elif kind == 1:
            lengths = rng.integers(1, 2049, n)  # anything up to a full window
        elif kind == 2:
            lengths = np.where(rng.random(n) < 0.1, rng.integers(3000, 9000, n), rng.integers(0, 200, n))  # rows above the budget
        else:
            lengths = np.where(rng.random(n) < 0.3, 0, rng.integers(90, 130, n))
        lists.append([int(v) for v in lengths])
    return lists


@pytest.mark.parametrize("batch_size", [1, 4, 32, 256])
@pytest.mark.parametrize("budget", [1, 31, 32, 512, 2048, 4096, 32768, 131072, 10**9])
def test_planner_properties(batch_size, budget):
    for lengths in _length_lists():
        n = len(lengths)
        chunks = plan_forward_chunks(lengths, batch_size, budget)
        # a partition of range(n), in order, no empty chunk
        assert [i for a, b in chunks for i in range(a, b)] == list(range(n)), (lengths, chunks)
        assert all(b > a for a, b in chunks)
        assert chunks == plan_forward_chunks(list(lengths), batch_size, budget)  # the same arguments, the same chunks
        assert chunks == plan_forward_chunks(tuple(lengths), batch_size, budget)
        costs = [sum(_cost(v) for v in lengths[a:b]) for a, b in chunks]
        for k, ((a, b), cost) in enumerate(zip(chunks, costs)):
            if k + 1 < len(chunks):
                assert b - a >= batch_size, (lengths, chunks)  # never fewer rows than the fixed stride gives a forward
                # closed early: the next row was refused because it did not fit
                assert cost + _cost(lengths[b]) > budget, (lengths, chunks, k)
            if b - a > batch_size:
                assert cost <= budget, (lengths, chunks, k)
        assert len(chunks) <= len(_fixed_stride(n, batch_size))


@pytest.mark.parametrize("batch_size", [1, 4, 32, 256])
def test_budget_zero_is_the_fixed_stride(batch_size):
    for lengths in _length_lists():
        for budget in (0, -1, -4096):
            assert plan_forward_chunks(lengths, batch_size, budget) == _fixed_stride(len(lengths), batch_size)


def test_planner_examples():
    assert plan_forward_chunks([], 32, 4096) == []
    # 110-token contexts cost 128 rows each: 32 per forward by stride, 256 within a budget of 32768
    assert plan_forward_chunks([110] * 600, 32, 32768) == [(0, 256), (256, 512), (512, 600)]
    # full windows at batch_size 32 already exceed the budget: unchanged
    assert plan_forward_chunks([2048] * 100, 32, 32768) == _fixed_stride(100, 32)
    # a single row above the budget still travels with its batch_size companions
    assert plan_forward_chunks([5000, 10, 10, 10, 10], 4, 64) == [(0, 4), (4, 5)]
    # empty rows cost nothing
    assert plan_forward_chunks([0] * 50, 4, 32) == [(0, 50)]
    # the cost is the padded length: 33 tokens occupy 64 rows
    assert plan_forward_chunks([33] * 8, 1, 128) == [(0, 2), (2, 4), (4, 6), (6, 8)]
    assert plan_forward_chunks([32] * 8, 1, 128) == [(0, 4), (4, 8)]


def _stub_case(index=4):
    with open(GOLDEN_DIR / "g3_process_stub.json", "r", encoding="utf-8") as handle:
        meta = json.load(handle)
    return meta, meta["cases"][index]  # 4: a long document, several blocks


def test_a_replaced_forward_keeps_the_batch_size_contract():
    """A stub forward under a huge budget: still at most ``batch_size`` rows per call, the reference's result, the ten
    timing keys and no ``forwards`` entry (that is the native path's)."""

    meta, case = _stub_case()
    seen = []

    def recording_forward(input_ids=None, attention_mask=None, **kw):
        seen.append(int(input_ids.shape[0]))
        return golden_stub_forward(input_ids=input_ids, attention_mask=attention_mask, **kw)

    model = host_only_model(CharTokenizer(emit_specials=meta["emit_specials"]), max_length=meta["max_length"], forward=recording_forward)
    model.forward_token_budget = 10**9
    assert model.forward_token_budget == 10**9
    for batch_size in (1, 2, 4):
        del seen[:]
        result = model.process(question=case["question"], context=case["context"], sentence_splitter=period_splitter,
                               show_progress=False, return_sentence_metrics=True, return_sentence_texts=True,
                               batch_size=batch_size, **case["kwargs"])
        assert seen and max(seen) <= batch_size, seen
        if batch_size < 4:
            assert len(seen) > 1  # (the case has several blocks: the contract was exercised)
        assert_process_result_matches(result, case["expected"], prob_tol=1e-6, score_tol=1e-6)
        assert set(result["timing"]) == TIMING_KEYS
        assert result["performance_trace"].as_dict() == result["timing"]
        assert "forwards" not in (getattr(result["performance_trace"], "runtime", None) or {})
    del seen[:]
    raws = model.get_raw_predictions_batch("q?", [["One. ", "Two."]] * 7, batch_size=2)
    assert len(raws) == 7 and seen == [2, 2, 2, 1]


def test_budget_validation(monkeypatch):
    model = host_only_model(forward=golden_stub_forward)
    monkeypatch.delenv("OPEN_PROVENCE_FORWARD_TOKENS", raising=False)
    assert model.forward_token_budget == 0  # no device: nothing to size a round by
    for bad in (-1, -4096, 1.5, 4096.0, "4096", True):
        with pytest.raises(ValueError):
            model.forward_token_budget = bad
    model.forward_token_budget = np.int64(8192)
    assert model.forward_token_budget == 8192 and type(model.forward_token_budget) is int
    model.forward_token_budget = 0
    assert model.forward_token_budget == 0
    monkeypatch.setenv("OPEN_PROVENCE_FORWARD_TOKENS", "12288")
    model.forward_token_budget = None  # back to the default: the environment first
    assert model.forward_token_budget == 12288
    assert host_only_model(forward=golden_stub_forward).forward_token_budget == 12288
    assert model._host_stage_spec()["forward_token_budget"] == 12288
    monkeypatch.setenv("OPEN_PROVENCE_FORWARD_TOKENS", "-5")
    with pytest.raises(ValueError):
        host_only_model(forward=golden_stub_forward).forward_token_budget
    monkeypatch.setenv("OPEN_PROVENCE_FORWARD_TOKENS", "many")
    with pytest.raises(ValueError):
        host_only_model(forward=golden_stub_forward).forward_token_budget


class _RecordingRemote:
    """The remote forward of a host-stage replica (``submit`` / ``result``), answered here by the golden stub's
    arithmetic row by row; records the rows of every submitted forward."""

    def __init__(self):
        self.launches = []
        self.submitted = []  # (rows, segments) of the forwards not yet answered, in order

    def submit(self, rows, segments):
        from open_provence_amd.launches import RemoteLaunch

        self.launches.append([len(r) for r in rows])
        self.submitted.append((rows, segments))
        return RemoteLaunch(remote=self, rows=len(rows), cu=None, seg_counts=[len(s) for s in segments])

    def result(self, launch):
        ranks, means = [], []
        for row, segs in zip(*self.submitted.pop(0)):
            out = golden_stub_forward(input_ids=torch.tensor([row], dtype=torch.long))
            keep = torch.softmax(out["pruning_logits"][0], dim=-1)[:, 1].numpy()
            ranks.append(out["ranking_logits"][0])
            means.append([float(keep[a:b].mean()) if b > a else 1.0 for a, b in segs])
        return torch.stack(ranks), means


def _replica(budget):
    from open_provence_amd.modeling import OpenProvenceModel

    spec = host_only_model(max_length=512)._host_stage_spec()  # (one block per context below)
    spec["forward_token_budget"] = budget
    remote = _RecordingRemote()
    return OpenProvenceModel._host_stage_replica(spec, remote), remote


def test_native_path_plans_its_forwards_within_each_granule():
    """A host-stage replica takes the native path without a GPU (its forwards go to a remote): with a budget it submits the
    planner's chunks of every granule, without one the fixed stride; the results are equal and the trace says what ran."""

    words = "the tower is tall boats carry fish and salt to north city harbour many years ago it was new".split()
    contexts = [" ".join(" ".join(words[(i * 5 + s * 3 + k) % len(words)] for k in range(4 + (i + s) % 5)).capitalize() + "."
                         for s in range(1 + i % 4)) for i in range(150)]
    call = dict(question="which boats carry salt?", context=contexts, sentence_splitter=period_splitter, show_progress=False,
                return_sentence_metrics=True, return_sentence_texts=True, batch_size=8, threshold=0.4)
    runs = {}
    for budget, granule in ((0, 150), (2048, 150), (2048, 40), (10**9, 150), (10**9, 40)):
        model, remote = _replica(budget)
        assert model.forward_token_budget == budget
        result = model.process(preprocess_batch_size=granule, **call)
        runs[(budget, granule)] = (result, remote.launches)
        forwards = result["performance_trace"].runtime["forwards"]
        assert forwards == {"launches": len(remote.launches), "rows": sum(len(rows) for rows in remote.launches),
                            "tokens": sum(sum(rows) for rows in remote.launches), "token_budget": budget}
        assert set(result["timing"]) == TIMING_KEYS
    legacy, legacy_launches = runs[(0, 150)]
    lengths = [n for rows in legacy_launches for n in rows]
    assert [len(rows) for rows in legacy_launches] == [b - a for a, b in plan_forward_chunks(lengths, 8, 0)]
    assert len(lengths) == 150  # one block per context, so a granule of 40 contexts is 40 rows
    for (budget, granule), (result, launches) in runs.items():
        assert [n for rows in launches for n in rows] == lengths  # the same rows in the same order
        for key in legacy:
            if key not in ("timing", "performance_trace"):
                assert result[key] == legacy[key], (budget, granule, key)
        if budget:
            # chunks do not span granules: the plan of every granule's rows, one after the other
            want = []
            for at in range(0, len(lengths), granule):
                want += [b - a for a, b in plan_forward_chunks(lengths[at : at + granule], 8, budget)]
            assert [len(rows) for rows in launches] == want, (budget, granule)
            assert len(launches) < len(legacy_launches)
    assert len(runs[(10**9, 150)][1]) == 1 and len(runs[(10**9, 40)][1]) == 4
