"""Prepared contexts on the host (``OpenProvenceModel.prepare_contexts``, ``prepared.py``): ``process(q, prepared)`` returns what
``process(q, raw)`` returns -- every key but the two timing ones, floats with ``==`` -- for each tokenizer of tests/helpers.py,
through a replaced forward (rows built on the host from the cached fragments); the refusals; and the Python restatement of
``op_assemble_rows`` (tests/assemble_model.py) against ``pipeline.prepare_block_inputs`` row by row, with five mistakes
that each have to move a row.  No GPU."""

import ctypes

import numpy as np
import pytest
import assemble_model as am
from helpers import CharTokenizer, build_wordpiece_tokenizer, golden_stub_forward, host_only_model, period_splitter

from open_provence_amd import _lib, pipeline as pl
from open_provence_amd.prepared import PreparedContexts, PreparedView, derive_row_template

TOKENIZERS = {
    "char": lambda: CharTokenizer(True),
    "char_manual": lambda: CharTokenizer(False),
    "wp": lambda: build_wordpiece_tokenizer(True),
    "wp_manual": lambda: build_wordpiece_tokenizer(False),
    "wp_v5": lambda: build_wordpiece_tokenizer(True, legacy_methods=False),
    "wp_v5_plain": lambda: build_wordpiece_tokenizer(False, legacy_methods=False),
}
# the row template each of them must be found to have: [CLS] q [SEP] ctx [SEP] (ids 1, 2, 2), built by the tokenizer or by the
# manual-specials path
EXPECTED_TEMPLATE = ([1], [2], [2])

_LONG = " ".join(f"In year {i} the boats carry fish and salt to the harbour of the north city." for i in range(9))
CORPUS = [
    _LONG,                                                                         # several blocks at max_length 64 - 96
    "Rivers flow to the sea. Mountains are tall! Rivers carry water and silt.",
    "",                                                                            # empty: the fallback sentence, no tokens
    ["The old bridge is made of stone. ", "Boats carry fish and salt.", "   "],    # pre-split sentences
    "North city\nThere is a small city in the north. The king built a harbour.\nMany years ago it was new.",
    "The tower is tall. It was built long ago! Many people visit it. Bread is made from flour.",
]
TITLES = ["Boats", "Rivers", "Nothing", "The bridge", "North", "The tower"]
QUESTION = "which boats carry salt?"
# a question beside which a fragment of max_length // 2 tokens no longer fits (it is clipped): 43 characters, 49 word pieces
LONG_QUESTIONS = {"char": "which boats carry fish and salt to the sea?",
                  "wp": "which boats carry fish and salt to the harbour of the north city in the year the king built it " * 2
                        + "and how many people visit the old bridge?"}
VIEWS = ([0, 2, 2, 3], [5, 1, 0])

_SKIP = ("timing", "performance_trace")


def _model(name, max_length=64):
    model = host_only_model(tokenizer=TOKENIZERS[name](), max_length=max_length, forward=golden_stub_forward)
    model.default_splitter_language = "en"
    return model


def _same(got, want):
    assert set(got) == set(want)
    for key in want:
        if key not in _SKIP:
            assert got[key] == want[key], key


# (prepare-time arguments, request-time arguments, question)
SCENARIOS = {
    "default_metrics": (dict(), dict(return_sentence_metrics=True, return_sentence_texts=True, threshold=0.4), QUESTION),
    "no_title": (dict(title=None), dict(always_select_title=True, return_sentence_texts=True), QUESTION),
    "explicit_titles": (dict(title=TITLES), dict(always_select_title=True, return_sentence_metrics=True, threshold=0.5), QUESTION),
    "first_line": (dict(first_line_as_title=True), dict(always_select_title=True, return_sentence_texts=True), QUESTION),
    "strip": (dict(strip_sentences=True), dict(return_sentence_texts=True, return_sentence_metrics=True), QUESTION),
    "boundaries": (dict(respect_sentence_boundaries=True), dict(return_sentence_metrics=True, batch_size=2), QUESTION),
    "reorder_top_k": (dict(), dict(reorder=True, top_k=2, return_sentence_metrics=True, use_best_reranker_score=False), QUESTION),
    "clipped": (dict(), dict(return_sentence_metrics=True, zero_score_when_empty=False), LONG_QUESTIONS),
    "empty_query": (dict(), dict(return_sentence_metrics=True, batch_size=3), ""),
}


def _raw_kwargs(prep_kwargs, indices_per_query):
    raw = dict(prep_kwargs)
    if isinstance(raw.get("title"), list):
        per_query = [[raw["title"][i] for i in indices] for indices in indices_per_query]
        raw["title"] = per_query[0] if len(per_query) == 1 else per_query
    return raw


@pytest.mark.parametrize("scenario", sorted(SCENARIOS))
@pytest.mark.parametrize("name", sorted(TOKENIZERS))
def test_process_on_prepared_contexts_equals_process_on_raw_texts(name, scenario):
    prep_kwargs, call_kwargs, question = SCENARIOS[scenario]
    question = question[name.split("_")[0]] if isinstance(question, dict) else question
    model = _model(name)
    common = dict(sentence_splitter=period_splitter, show_progress=False)
    prepared = model.prepare_contexts(CORPUS, sentence_splitter=period_splitter, **prep_kwargs)
    assert isinstance(prepared, PreparedContexts) and len(prepared) == len(CORPUS)
    assert prepared.template is not None and not prepared.host_assembled
    assert (prepared.template.prefix, prepared.template.middle, prepared.template.suffix) == EXPECTED_TEMPLATE, prepared.template

    # one question, the whole corpus
    got = model.process(question, prepared, **common, **call_kwargs)
    want = model.process(question, CORPUS, **common, **_raw_kwargs(prep_kwargs, [range(len(CORPUS))]), **call_kwargs)
    _same(got, want)
    assert all(got["timing"][k] == 0.0 for k in ("sentence_collect_seconds", "sentence_normalize_seconds", "tokenize_seconds",
                                                  "fragment_split_seconds", "fragment_decode_seconds"))
    assert got["performance_trace"].total_seconds > 0.0

    # one question, a view with a repeated context
    view = prepared.select(VIEWS[0])
    assert isinstance(view, PreparedView) and len(view) == 4
    _same(model.process(question, view, **common, **call_kwargs),
          model.process(question, [CORPUS[i] for i in VIEWS[0]], **common, **_raw_kwargs(prep_kwargs, [VIEWS[0]]), **call_kwargs))

    # two questions, a view each
    questions = [question, "what do rivers carry?"]
    got = model.process(questions, [prepared.select(v) for v in VIEWS], **common, **call_kwargs)
    want = model.process(questions, [[CORPUS[i] for i in v] for v in VIEWS], **common, **_raw_kwargs(prep_kwargs, VIEWS), **call_kwargs)
    _same(got, want)
    assert len(got["pruned_context"]) == 2 and [len(p) for p in got["pruned_context"]] == ([2, 2] if "top_k" in call_kwargs else [4, 3])


@pytest.mark.parametrize("name", sorted(TOKENIZERS))
def test_the_shapes_the_cases_are_meant_to_cover(name):
    """Several blocks per context, a clipped fragment, an empty context with a token-less fallback fragment, an empty query."""

    model = _model(name)
    prepared = model.prepare_contexts(CORPUS, sentence_splitter=period_splitter)
    long_question = LONG_QUESTIONS[name.split("_")[0]]
    *_, plan, blocks = am.request_plan(model, prepared, [QUESTION, long_question, ""], [prepared.select(range(len(CORPUS)))] * 3)
    rows_of_first = [p for p in plan if p[0] == 0 and p[1] < len(prepared.items[0].fragments)]
    assert len(rows_of_first) > 1                                      # the long context splits into several blocks
    assert any(p[3] > 0 for p in plan if p[0] == 1)                    # the long question clips a fragment
    assert not any(p[3] > 0 for p in plan if p[0] != 1)                # ... the others leave room for every fragment
    assert [len(f.token_ids) for f in prepared.items[2].fragments] == [0]  # the empty context: one fragment without tokens
    assert model.tokenizer.encode("", add_special_tokens=False) == []
    # select(): order kept, repeats allowed, negative indices as Python's, out of range refused
    assert prepared.select([3, 3, -1]).indices == [3, 3, len(CORPUS) - 1]
    assert prepared.select([4, 0, 2]).select([2, 0]).indices == [2, 4]
    with pytest.raises(IndexError):
        prepared.select([len(CORPUS)])
    assert prepared.device_bytes == 4 * (prepared.n_tokens + prepared.n_fragments + 1)
    ids, frag_off = prepared.flat_tokens()
    assert ids.dtype == frag_off.dtype == np.int32 and frag_off[0] == 0 and frag_off[-1] == ids.size == prepared.n_tokens
    assert ids.tolist() == [t for item in prepared.items for f in item.fragments for t in f.token_ids]


def test_a_layout_without_a_template_is_assembled_on_the_host():
    """A tokenizer whose rows depend on the pair in another way than by concatenation: no template, rows from the host, same
    results."""

    class Reversing(CharTokenizer):
        def build_inputs_with_special_tokens(self, tokens_a, tokens_b=None):
            return [self.cls_token_id, *list(tokens_b or []), self.sep_token_id, *tokens_a, self.sep_token_id]

    model = host_only_model(tokenizer=Reversing(), max_length=96, forward=golden_stub_forward)
    prepared = model.prepare_contexts(CORPUS, sentence_splitter=period_splitter)
    assert prepared.template is None and prepared.host_assembled
    _same(model.process(QUESTION, prepared, sentence_splitter=period_splitter, show_progress=False, return_sentence_metrics=True),
          model.process(QUESTION, CORPUS, sentence_splitter=period_splitter, show_progress=False, return_sentence_metrics=True))
    assert derive_row_template(lambda q, c: [1, *q, 2, *c, 2, *q]) is None            # the query twice
    assert derive_row_template(lambda q, c: [1, *q, 2, *c] + [2] * len(q)) is None     # pieces that differ between the probes
    assert derive_row_template(lambda q, c: [7] * 9 + [*q, *c]) is None                # a piece of more than 8 ids
    assert derive_row_template(lambda q, c: ([1, *q, 2] if q else []) + [*c, 2]) is None  # an empty query laid out differently
    plain = derive_row_template(lambda q, c: [*q, *c])
    assert (plain.prefix, plain.middle, plain.suffix) == ([], [], [])


def test_replaced_forward_keeps_batch_size_rows_per_call():
    calls = []

    def forward(input_ids=None, attention_mask=None, **kw):
        calls.append(int(input_ids.shape[0]))
        return golden_stub_forward(input_ids=input_ids, attention_mask=attention_mask, **kw)

    model = host_only_model(tokenizer=CharTokenizer(), max_length=64, forward=forward)
    prepared = model.prepare_contexts(CORPUS, sentence_splitter=period_splitter)
    model.process(QUESTION, prepared, batch_size=3, show_progress=False)
    assert len(calls) > 2 and max(calls) == 3 and all(n == 3 for n in calls[:-1])
    assert "forwards" not in getattr(model.process(QUESTION, prepared, show_progress=False)["performance_trace"], "runtime", {})


def test_refusals():
    model = _model("char")
    prepared = model.prepare_contexts(CORPUS, title=TITLES, sentence_splitter=period_splitter, language="en", strip_sentences=True)
    ok = dict(show_progress=False)
    model.process(QUESTION, prepared, **ok)
    # the preparation's own arguments may be repeated; others are refused
    model.process(QUESTION, prepared, title=list(TITLES), sentence_splitter=period_splitter, language="en", strip_sentences=True, **ok)
    for bad in (dict(title=None), dict(title=TITLES[::-1]), dict(first_line_as_title=True), dict(sentence_splitter=lambda t: [t]),
                dict(language="ja"), dict(respect_sentence_boundaries=True)):
        with pytest.raises(ValueError, match="prepared with"):
            model.process(QUESTION, prepared, **bad, **ok)
    plain = model.prepare_contexts(CORPUS, sentence_splitter=period_splitter)
    with pytest.raises(ValueError, match="prepared with"):
        model.process(QUESTION, plain, strip_sentences=True, **ok)
    # another model
    other = _model("char")
    with pytest.raises(ValueError, match="another model"):
        other.process(QUESTION, prepared, **ok)
    # max_length or the tokenizer changed since
    model.max_length = 80
    with pytest.raises(ValueError, match="max_length"):
        model.process(QUESTION, prepared, **ok)
    model.max_length = 64
    kept = model.tokenizer
    model.tokenizer = CharTokenizer()
    with pytest.raises(ValueError, match="tokenizer"):
        model.process(QUESTION, prepared, **ok)
    model.tokenizer = kept
    # a process group or a host front-end
    model._dist = {"world": 2, "rank": 0, "dst": 0, "group": None}
    with pytest.raises(ValueError, match="process group"):
        model.process(QUESTION, prepared, **ok)
    del model._dist
    model.__dict__["_remote_forward"] = object()
    with pytest.raises(ValueError, match="front-end"):
        model.process(QUESTION, prepared, **ok)
    del model.__dict__["_remote_forward"]
    # shapes
    with pytest.raises(ValueError):
        model.process([QUESTION, QUESTION], prepared, **ok)
    with pytest.raises(ValueError):
        model.process(QUESTION, [prepared.select([0]), prepared.select([1])], **ok)
    with pytest.raises(ValueError):
        model.process([QUESTION, QUESTION], [prepared.select([0])], **ok)
    with pytest.raises(ValueError):
        model.process([QUESTION, QUESTION], [prepared.select([0]), "raw text"], **ok)
    with pytest.raises(ValueError):
        model.process([QUESTION, QUESTION], [prepared.select([0]), plain.select([0])], **ok)
    with pytest.raises(ValueError):
        model.prepare_contexts("one string")
    model.process(QUESTION, prepared, **ok)  # (and it still works)


# -- the restatement of the kernel -------------------------------------------------------------------------------------------------
def _compare_all(mutate=None):
    """-> the number of compared rows that differ from ``prepare_block_inputs`` (over every tokenizer's pipeline plans and the
    synthetic plan)."""

    differing = compared = 0
    for name in sorted(TOKENIZERS):
        model = _model(name)
        prepared = model.prepare_contexts(CORPUS, sentence_splitter=period_splitter)
        questions = [QUESTION, LONG_QUESTIONS[name.split("_")[0]], "", "what do rivers carry?"]
        views = [prepared.select(range(len(CORPUS))), prepared.select(range(len(CORPUS))), prepared.select(VIEWS[0]), prepared.select(VIEWS[1])]
        corpus, frag_off, query_ids, q_off, pieces, plan, blocks = am.request_plan(model, prepared, questions, views)
        cases = [(corpus, frag_off, query_ids, q_off, pieces, plan, blocks)]
        frags, queries, synthetic = am.synthetic_case(np.random.default_rng(3))
        s_blocks = []
        for query, first, n, clip in synthetic:
            block = list(frags[first: first + n])
            if clip > 0:
                block[0] = pl.truncate_fragment(model.tokenizer, block[0], clip)
            s_blocks.append((queries[query], block))
        cases.append((*am.flat_arrays(frags, queries), pieces, synthetic, s_blocks))
        for corpus, frag_off, query_ids, q_off, pieces, plan, blocks in cases:
            lengths = am.row_lengths(frag_off, q_off, pieces, plan)
            cu = np.concatenate(([0], np.cumsum(lengths))).astype(np.int32)
            out = am.assemble_rows(corpus, frag_off, query_ids, q_off, pieces, plan, cu, mutate=mutate)
            for r, (query, block) in enumerate(blocks):
                want = model._prepare_block_inputs(query, block)[0]
                assert len(want) == lengths[r], (name, r)
                compared += 1
                differing += out[cu[r]: cu[r + 1]].tolist() != want
    assert compared > 100
    return differing


def test_restatement_reproduces_prepare_block_inputs_row_by_row():
    assert _compare_all() == 0


@pytest.mark.parametrize("mutation", am.MUTATIONS)
def test_each_mistake_moves_a_row(mutation):
    assert _compare_all(mutate=mutation) > 0


# -- the C call: declared, and refused on the host copies before the handle is looked at -----------------------------------------
def test_the_call_is_declared_and_refuses_a_malformed_request_before_the_handle(hip_library):
    import re
    from pathlib import Path

    lib = hip_library
    header = re.sub(r"/\*.*?\*/", "", (Path(_lib.__file__).resolve().parents[1] / "include" / "open_provence_hip.h").read_text(), flags=re.S)
    assert _lib.OP_ABI_VERSION == 10 == lib.op_abi_version()
    assert "op_assemble_rows" in _lib.EXPORTED_SYMBOLS and re.search(r"\bint op_assemble_rows\s*\(", header)
    assert re.search(r"#define OP_ASSEMBLE_MAX_PIECE 8\b", header) and _lib.OP_ASSEMBLE_MAX_PIECE == 8
    assert hasattr(lib, "op_assemble_rows") and lib.op_assemble_rows.argtypes[1] is ctypes.POINTER(_lib.OpAssembleRequest)
    # 8 x 4 bytes, then 13 pointers
    assert ctypes.sizeof(_lib.OpAssembleRequest) == 32 + 13 * 8 and _lib.OpAssembleRequest.prefix.offset == 32

    frags, queries, plan = am.synthetic_case(np.random.default_rng(3))
    assert lib.op_assemble_rows(None, None, ctypes.c_void_p(am.FAKE_POINTER), None) == _lib.OP_ERR_INVALID
    assert "request is NULL" in _lib.last_error(lib, None)
    for label, overrides, word in am.refusal_cases() + [("null output", dict(), "ids_dev is NULL")]:
        req, _keep = am.build_request(frags, queries, plan, **overrides)
        out = None if label == "null output" else ctypes.c_void_p(am.FAKE_POINTER)
        assert lib.op_assemble_rows(None, ctypes.byref(req), out, None) == _lib.OP_ERR_INVALID, label
        message = _lib.last_error(lib, None)
        assert word in message and "NULL handle" not in message, (label, message)
    # well-formed requests get as far as the handle: the synthetic plan, no rows at all, rows without any token
    for overrides in (dict(), dict(n_rows=0, total_tokens=0, plan_dev=None, cu_seqlens_dev=None)):
        req, _keep = am.build_request(frags, queries, plan, **overrides)
        assert lib.op_assemble_rows(None, ctypes.byref(req), ctypes.c_void_p(am.FAKE_POINTER), None) == _lib.OP_ERR_INVALID
        assert "NULL handle" in _lib.last_error(lib, None), overrides
    req, _keep = am.build_request(frags, queries, [(0, 0, 0, 0)] * 3, pieces=([], [], []), corpus_dev=None, query_ids_dev=None)
    assert req.total_tokens == 0
    assert lib.op_assemble_rows(None, ctypes.byref(req), None, None) == _lib.OP_ERR_INVALID
    assert "NULL handle" in _lib.last_error(lib, None)
