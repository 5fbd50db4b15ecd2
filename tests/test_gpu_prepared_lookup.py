"""Prepared requests whose contexts are looked up in their rows on the device: ``op_located_fragment_means`` held to its
restatement (tests/lookup_model.py, itself held to the host path by tests/test_lookup_model.py) -- the places as integers, the
means on uint32 views with ``==``, guard regions and unnamed slots untouched -- on rows laid out by ``op_assemble_rows`` from
the same plan, at the smallest shapes at which each part of the search can go wrong; and ``process(q, prepared)`` under
``OPEN_PROVENCE_PREPARED_DECISIONS=2`` on the model of tests/test_gpu_prepared_decisions.py against the host path and the
raw-text call in all result keys with ``==``."""

import os
import warnings

import numpy as np
import pytest
import torch

import lookup_model as lm
from helpers import CharTokenizer, period_splitter
from test_gpu_prepared_decisions import METRICS, WORDS, _decisions_of, _in_process, _same, _text, model  # noqa: F401  (fixtures)

from open_provence_amd import pipeline as pl

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
POISON_F32, POISON_I32 = -7.5, -1234567
FILL = 50                      # the queries' filler id: in no context below
C3, C4 = [60, 61, 62], [60, 61, 62, 63]
PERIODIC = [60, 61, 2, 60, 61, 2, 60, 61]


def _put(idx, ids):
    return {idx + j: t for j, t in enumerate(ids)}


# (name, head_len, {place in the row: id} written over the query's filler, the row's fragments, clip, their shifts, the place wanted)
SPECS = [
    ("empty query, no match: no pass at all behind the prefix and middle", 2, {}, [C3], 0, None, 2),
    ("head_len 63, at head_len - 1 (the middle and the context's first id): one pass", 63, {}, [[2, 2]], 0, None, 62),
    ("head_len 64, at 63: exactly one pass, its last lane", 64, {}, [[2, 2]], 0, None, 63),
    ("head_len 64, none", 64, {}, [C3], 0, None, 64),
    ("head_len 65, at 64: the second pass, its first lane", 65, {}, [[2, 2]], 0, None, 64),
    ("head_len 129, at 128: the third pass", 129, {}, [[2, 2]], 0, None, 128),
    ("at 0: the context begins with the prefix", 129, {}, [[1, FILL, FILL]], 0, None, 0),
    ("at 63", 129, _put(63, C3), [C3], 0, None, 63),
    ("at 64", 129, _put(64, C3), [C3], 0, None, 64),
    ("two matches in one pass: the lower", 65, {**_put(10, C3), **_put(40, C3)}, [C3], 0, None, 10),
    ("two matches, the lower one in a later lane of its pass than the higher one in its own", 129, {**_put(60, C3), **_put(70, C3)}, [C3], 0, None, 60),
    ("a pass full of first-id-only matches in front of the pass with the real one", 129,
     {**{i: 1 for i in range(1, 64)}, **_put(80, [1, 61, 62])}, [[1, 61, 62]], 0, None, 80),
    ("agrees on n_ctx - 1 ids, fails on the last; no match", 65, _put(5, [60, 61, 62, 99]), [C4], 0, None, 65),
    ("... and a match behind it", 65, {**_put(5, [60, 61, 62, 99]), **_put(30, C4)}, [C4], 0, None, 30),
    ("the match runs into the context's own copy", 5, {1: 120, 2: 60, 3: 61}, [PERIODIC], 0, None, 2),
    ("... across a pass boundary", 65, _put(62, [60, 61]), [PERIODIC], 0, None, 62),
    ("n_ctx 1", 20, {7: 60}, [[60]], 0, None, 7),
    ("n_ctx 1, none", 20, {}, [[60]], 0, None, 20),
    ("a clipped first fragment: found at its clipped length", 20, _put(3, [60, 61, 70, 71]), [[60, 61, 62, 63, 64], [70, 71]], 2, None, 3),
    ("... and not at its whole length", 20, _put(3, [60, 61, 62, 63, 64, 70, 71]), [[60, 61, 62, 63, 64], [70, 71]], 2, None, 20),
    ("three fragments, shifted: the ranges clamp at 0", 20, _put(2, [60, 61, 62, 63, 64]), [[60, 61], [62], [63, 64]], 0, [0, 5, 4], 2),
]


def _rows(specs, *, slot_base=0, seed=3) -> lm.Rows:
    fragments, queries, plan, shifts = [], [], [], []
    for _name, head_len, writes, parts, clip, part_shifts, _want in specs:
        query = [FILL] * (head_len - 2)
        for place, value in writes.items():
            query[place - 1] = value  # (behind the one-id prefix)
        plan.append((len(queries), len(fragments), len(parts), clip))
        queries.append(query)
        fragments += parts
        shifts += part_shifts or [0] * len(parts)
    return lm.Rows(fragments, queries, plan, shifts, slot_base=slot_base, seed=seed)


TABLES = {"1 row": _rows(SPECS[:1]), "4 rows": _rows(SPECS[:4]), "5 rows": _rows(SPECS[:5]), "all rows": _rows(SPECS),
          "slots from 3": _rows(SPECS[-6:], slot_base=3, seed=4)}
WANT = {name: rows.model(fill=(POISON_F32, POISON_I32)) for name, rows in TABLES.items()}  # (computed once, left unchanged)


def test_the_tables_are_what_they_claim():
    rows = TABLES["all rows"]
    ctx_start = WANT["all rows"][0]
    assert ctx_start.tolist() == [spec[6] for spec in SPECS]
    assert [rows.head_len(i) for i in range(len(SPECS))] == [spec[1] for spec in SPECS]
    assert {2, 63, 64, 65, 129} <= {spec[1] for spec in SPECS}
    means = WANT["all rows"][1]
    last = int(rows.slot_off[-2])
    assert means[last + 1] == 1.0 and means[last] != 1.0 and means[last + 2] != 1.0  # (a range shifted to empty at 0)
    assert len(TABLES["all rows"].plan) > 8 and TABLES["slots from 3"].slot_off[0] == 3


def _dev(array, dtype=np.int32):
    return torch.from_numpy(np.ascontiguousarray(array, dtype=dtype).reshape(-1)).to(DEV)


class _Run:
    """The device side of one table: its inputs, the assembled ids, and guarded outputs."""

    def __init__(self, enc, rows: lm.Rows, *, tail=0, guard=64):
        self.enc, self.rows, self.guard, self.n, self.n_rows = enc, rows, guard, rows.n_slots + tail, len(rows.plan)
        self.shared = (_dev(rows.frag_off), rows.frag_off, _dev(rows.q_off), rows.q_off, lm.PIECES, _dev(rows.plan_np),
                       np.ascontiguousarray(rows.plan_np.reshape(-1)), _dev(rows.cu), rows.cu)
        self.ids = enc.assemble_rows(_dev(rows.corpus), self.shared[0], rows.frag_off, _dev(rows.query_ids), *self.shared[2:])
        self.rest = (torch.from_numpy(rows.keep_prob).to(DEV), _dev(rows.frag_shift_np), _dev(rows.slot_off), rows.slot_off)

    def __call__(self):
        guard, n, n_rows = self.guard, self.n, self.n_rows
        mean = torch.full((guard + n + guard,), POISON_F32, dtype=torch.float32, device=DEV)
        frag = torch.full((guard + n + guard,), POISON_I32, dtype=torch.int32, device=DEV)
        start = torch.full((guard + n_rows + guard,), POISON_I32, dtype=torch.int32, device=DEV)
        stream = torch.cuda.current_stream(torch.device(DEV))
        self.enc.located_fragment_means(*self.shared, *self.rest, mean[guard: guard + n], frag[guard: guard + n], self.ids,
                                        start[guard: guard + n_rows])
        stream.synchronize()
        return start.cpu().numpy(), mean.cpu().numpy(), frag.cpu().numpy()

    def check(self, outputs, want):
        guard, n, n_rows, named = self.guard, self.n, self.n_rows, self.rows.n_slots
        start, mean, frag = outputs
        want_start, want_mean, want_frag = want
        assert np.array_equal(start[guard: guard + n_rows], want_start)
        assert np.array_equal(lm.bits(mean[guard: guard + named]), lm.bits(want_mean))  # (unnamed slots in front keep the fill: the model's too)
        assert np.array_equal(frag[guard: guard + named], want_frag)
        # the guard bands of all three outputs and the slots behind the rows' keep what they held
        for buf, body, fill in ((start, n_rows, POISON_I32), (frag, named, POISON_I32)):
            assert (buf[:guard] == fill).all() and (buf[guard + body:] == fill).all()
        filled = np.full(1, POISON_F32, dtype=np.float32)
        assert (lm.bits(mean[:guard]) == lm.bits(filled)).all() and (lm.bits(mean[guard + named:]) == lm.bits(filled)).all()


@pytest.mark.parametrize("name", list(TABLES))
def test_located_fragment_means_are_the_models(model, name):
    rows = TABLES[name]
    run = _Run(model.encoder, rows, tail=5 if rows.slot_off[0] else 0)
    torch.cuda.synchronize()
    assert np.array_equal(run.ids.cpu().numpy(), rows.ids)  # (the rows the model searched are the rows the device laid out)
    first = run()
    run.check(first, WANT[name])
    # twice, and on a second stream: the same outputs
    again = run()
    side = torch.cuda.Stream(device=DEV)
    with torch.cuda.stream(side):
        third = run()
    for other in (again, third):
        for a, b in zip(first, other):
            assert np.array_equal(lm.bits(a), lm.bits(b))


def test_the_engine_checks_its_arguments(model):
    rows = TABLES["4 rows"]
    run = _Run(model.encoder, rows)
    mean = torch.empty(rows.n_slots, dtype=torch.float32, device=DEV)
    frag = torch.empty(rows.n_slots, dtype=torch.int32, device=DEV)
    start = torch.empty(len(rows.plan), dtype=torch.int32, device=DEV)
    call = model.encoder.located_fragment_means
    with pytest.raises(ValueError, match="ids"):
        call(*run.shared, *run.rest, mean, frag, run.ids.to(torch.int64), start)
    with pytest.raises(ValueError, match="ctx_start_out"):
        call(*run.shared, *run.rest, mean, frag, run.ids, start.cpu())
    with pytest.raises(ValueError, match="sizes"):
        call(*run.shared, *run.rest, mean, frag, run.ids[:-1], start)
    with pytest.raises(ValueError, match="sizes"):
        call(*run.shared, *run.rest, mean, frag, run.ids, start[:-1])
    call(*run.shared, *run.rest, mean, frag, run.ids, start)
    torch.cuda.synchronize()
    assert np.array_equal(start.cpu().numpy(), WANT["4 rows"][0])


# -- process() -------------------------------------------------------------------------------------------------------------------------
COMMON = dict(sentence_splitter=period_splitter, show_progress=False, **METRICS)
LOWER = "which of " + " ".join(WORDS)  # (holds the first letter of every word of the texts)


def _process(model, monkeypatch, value, *args, **kwargs):
    monkeypatch.setenv("OPEN_PROVENCE_PREPARED_DECISIONS", value)
    return model.process(*args, **COMMON, **kwargs)


def _counting(model, calls):
    inner = model.encoder.located_fragment_means
    model.encoder.located_fragment_means = lambda *a, **k: calls.append(1) or inner(*a, **k)


def test_a_question_that_shares_first_ids_runs_on_the_device(model, monkeypatch):
    rng = np.random.default_rng(12)
    texts = [_text(rng, 200), _text(rng, 90), _text(rng, 1400)]
    assert all(text[0] in LOWER for text in texts)
    prepared = model.prepare_contexts(texts, sentence_splitter=period_splitter)
    calls = []
    _counting(model, calls)
    try:
        located = _process(model, monkeypatch, "2", LOWER, prepared)
        n_located = len(calls)
        planned = _process(model, monkeypatch, "1", LOWER, prepared)
        off = _process(model, monkeypatch, "0", LOWER, prepared)
        assert len(calls) == n_located >= 1  # (the means came from the locating kernel, under "2" alone)
    finally:
        del model.encoder.located_fragment_means
    assert _decisions_of(located) == "device" and _decisions_of(planned) == "host" and _decisions_of(off) == "host"
    _same(located, off)
    _same(located, model.process(LOWER, texts, **COMMON))
    assert any(s is not None and np.isfinite(s) for row in located["reranking_score"] for s in (row if isinstance(row, list) else [row]))


def test_contexts_that_occur_in_their_question(model, monkeypatch):
    """Each short context is a word of the question, and one is periodic around the separator's id and continues the question's
    end: the host path finds them LEFT of prefix + question + middle (asserted here on the CPU), and so must the device."""

    rng = np.random.default_rng(13)
    question = "is paris nearer to rome than xab"
    texts = ["paris", "rome", "ab\x02ab\x02ab", _text(rng, 150), "is paris. rome than."]
    prepared = model.prepare_contexts(texts, sentence_splitter=period_splitter)
    query = pl.tokenize_query(model.tokenizer, question)
    head_len = 1 + len(query) + 1
    places = []
    for item in prepared.items[:3]:
        fragments = list(item.fragments)
        ranges = pl.prepare_block_inputs(model.tokenizer, query, fragments)[3]
        places.append((ranges[0][0], ranges[-1][1] - ranges[0][0]))
    assert places[0][0] == 1 + question.index("paris") and places[1][0] == 1 + question.index("rome")
    assert places[2][0] == head_len - 3 and places[2][0] + places[2][1] > head_len  # (into the context's own copy)
    assert all(start < head_len for start, _n in places)
    located = _process(model, monkeypatch, "2", question, prepared)
    off = _process(model, monkeypatch, "0", question, prepared)
    assert _decisions_of(located) == "device" and _decisions_of(off) == "host"
    _same(located, off)
    _same(located, model.process(question, texts, **COMMON))


def test_two_questions_over_two_views(model, monkeypatch):
    rng = np.random.default_rng(14)
    texts = [_text(rng, 300), "delta", _text(rng, 700), _text(rng, 60), "eta theta. iota."]
    prepared = model.prepare_contexts(texts, sentence_splitter=period_splitter)
    questions, views = [LOWER, "where is delta and eta theta"], ([0, 1, 1, 4], [3, 2, 1, 4, 0])
    contexts = [prepared.select(v) for v in views]
    located = _process(model, monkeypatch, "2", questions, contexts)
    off = _process(model, monkeypatch, "0", questions, contexts)
    assert _decisions_of(located) == "device" and _decisions_of(off) == "host"
    _same(located, off)
    _same(located, model.process(questions, [[texts[i] for i in v] for v in views], **COMMON))


def test_an_empty_context_still_takes_the_host_stages(model, monkeypatch):
    rng = np.random.default_rng(15)
    texts = [_text(rng, 200), "", _text(rng, 90)]
    prepared = model.prepare_contexts(texts, sentence_splitter=period_splitter)
    got = _process(model, monkeypatch, "2", LOWER, prepared)
    assert _decisions_of(got) == "host"
    _same(got, model.process(LOWER, texts, **COMMON))
    assert _decisions_of(_process(model, monkeypatch, "2", LOWER, prepared.select([0, 2]))) == "device"


def test_the_range_guards_repeat_takes_the_located_means_again():
    """tests/test_gpu_prepared_decisions.py's test of the same name, with a lower-case question under "2": the repeat on the
    (hi, lo) bf16 sets must look the contexts up again in the ids the first launch laid out and land in the same slots, so that
    the result equals a model that never ran the fp16 + e4m3 sets."""

    import test_gpu_policy as policy
    from open_provence_amd.config import OpenProvenceConfig
    from open_provence_amd.modeling import OpenProvenceModel

    meta, _dims, _rows_, state = policy._overflowing_state()
    cfg = OpenProvenceConfig(base_model_config=meta["base_model_config"], tokenizer_name_or_path="x",
                             pruning_config={"hidden_size": meta["base_model_config"]["hidden_size"]}, max_length=512)
    text = "alpha beta gamma. delta epsilon zeta eta. theta iota kappa lambda mu. " * 6
    texts = [text, text[:120], text[:300], "gamma"]
    question = "what is gamma and alpha?"
    results, calls = {}, {}
    old = {name: os.environ.pop(name, None) for name in ("OPEN_PROVENCE_NO_F8", "OPEN_PROVENCE_PREPARED_DECISIONS", "OPEN_PROVENCE_HOST_REPLICAS")}
    try:
        os.environ["OPEN_PROVENCE_HOST_REPLICAS"] = "0"
        for no_f8 in (True, False):
            if no_f8:
                os.environ["OPEN_PROVENCE_NO_F8"] = "1"
            else:
                os.environ.pop("OPEN_PROVENCE_NO_F8", None)
            model = OpenProvenceModel(cfg, device="cuda", tokenizer=CharTokenizer(), state_dict=state, calibrate=False)
            os.environ["OPEN_PROVENCE_PREPARED_DECISIONS"] = "2"
            prepared = model.prepare_contexts(texts, sentence_splitter=period_splitter)
            assert model.encoder.f8_active() == (not no_f8)
            calls[no_f8] = []
            _counting(model, calls[no_f8])
            with warnings.catch_warnings(record=True):
                warnings.simplefilter("always")
                results[no_f8] = model.process(question, prepared, **COMMON)
            assert not model.encoder.f8_active() and _decisions_of(results[no_f8]) == "device"
    finally:
        for name, value in old.items():
            os.environ.pop(name, None)
            if value is not None:
                os.environ[name] = value
    _same(results[False], results[True])
    assert int(results[False]["performance_trace"].runtime["fallback_from_f8"]) >= 1
    assert len(calls[False]) > len(calls[True]) >= 1  # (the repeat took the located means again)
    assert all(s is not None and np.isfinite(s) for s in results[False]["reranking_score"])
