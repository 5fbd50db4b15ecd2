"""Prepared contexts on the GPU: ``op_assemble_rows`` against the host rows id for id (guard regions, refusals), and
``process(q, prepared)`` on the xsmall synthetic model against ``process(q, raw)`` with ``==`` -- the same ids, and a row's
outputs do not depend on its companions in a launch -- with fewer forwards, and with the running audit in force."""

import ctypes
import warnings

import numpy as np
import pytest
import torch

import assemble_model as am
from helpers import CharTokenizer, period_splitter

from open_provence_amd import _lib, pipeline as pl
from open_provence_amd.prepared import derive_row_template

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
POISON = -1234567
MAX_LENGTH = 512


@pytest.fixture(autouse=True)
def _in_process(monkeypatch):
    monkeypatch.setenv("OPEN_PROVENCE_HOST_REPLICAS", "0")
    monkeypatch.delenv("OPEN_PROVENCE_FORWARD_TOKENS", raising=False)


@pytest.fixture(scope="module")
def model():
    from open_provence_amd.config import OpenProvenceConfig
    from open_provence_amd.modeling import OpenProvenceModel
    from open_provence_amd.synthetic import named_dims, synth_state_dict

    dims = named_dims("xsmall")
    cfg = OpenProvenceConfig(base_model_config=dims.to_base_model_config(), tokenizer_name_or_path="char-tokenizer",
                             pruning_config={"hidden_size": dims.hidden_size}, max_length=MAX_LENGTH, num_labels=1)
    return OpenProvenceModel(cfg, device=DEV, tokenizer=CharTokenizer(), state_dict=synth_state_dict(dims, 7))


# -- the kernel ----------------------------------------------------------------------------------------------------------------------
def _i32(values):
    return torch.from_numpy(np.ascontiguousarray(values, dtype=np.int32).reshape(-1)).to(DEV)


def _assemble(enc, frags, queries, plan, pieces, guard=64):
    """-> (the rows the kernel wrote, the guard regions before and behind them)."""

    corpus, frag_off, query_ids, q_off = am.flat_arrays(frags, queries)
    plan_np = np.array(plan, dtype=np.int32).reshape(-1, 4)
    lengths = am.row_lengths(frag_off, q_off, pieces, plan)
    cu = np.concatenate(([0], np.cumsum(lengths))).astype(np.int32)
    total = int(cu[-1])
    buf = torch.full((guard + total + 64,), POISON, dtype=torch.int32, device=DEV)
    out = enc.assemble_rows(_i32(corpus), _i32(frag_off), frag_off, _i32(query_ids), _i32(q_off), q_off, pieces, _i32(plan_np), plan_np,
                            _i32(cu), cu, out=buf[guard: guard + total])
    assert out.data_ptr() == buf.data_ptr() + 4 * guard and out.numel() == total
    host = buf.cpu().numpy()
    return host[guard: guard + total], cu, (host[:guard], host[guard + total:])


def _frags(rng, lengths, low=10, high=400):
    return [pl.FragmentRecord("", 0, i, i, n, [int(t) for t in rng.integers(low, high, n)]) for i, n in enumerate(lengths)]


def _host_rows(tokenizer, manual, frags, queries, plan):
    rows = []
    for query, first, n, clip in plan:
        block = list(frags[first: first + n])
        if clip > 0:
            block[0] = pl.truncate_fragment(tokenizer, block[0], clip)
        rows.append(pl.prepare_block_inputs(tokenizer, queries[query], block, manual_specials=manual[0], manual_cls=manual[1],
                                            manual_sep=manual[2])[0])
    return rows


class _PairTokenizer(CharTokenizer):
    """A tokenizer-built layout with longer pieces: ``<s> q </s></s> ctx </s>``."""

    def build_inputs_with_special_tokens(self, tokens_a, tokens_b=None):
        return [1, *tokens_a, 2, 2, *list(tokens_b or []), 2]


# the three template kinds: built by the tokenizer, the manual-specials path, the plain concatenation
LAYOUTS = {
    "tokenizer_built": (_PairTokenizer(), (False, None, None), ([1], [2, 2], [2])),
    "manual_specials": (CharTokenizer(False), (True, 1, 2), ([1], [2], [2])),
    "plain_concatenation": (CharTokenizer(False), (False, None, None), ([], [], [])),
}


def _shapes():
    rng = np.random.default_rng(11)
    q20 = [int(t) for t in rng.integers(10, 400, 20)]
    shapes = {}
    # 1 row
    shapes["one_row"] = (_frags(rng, [5, 7]), [q20], [(0, 0, 2, 0)])
    # rows of 1 token of context, with queries of 0 - 5 ids: every alignment of the context's first element
    queries = [[int(t) for t in rng.integers(10, 400, n)] for n in range(6)]
    shapes["one_token_contexts"] = (_frags(rng, [1] * 24), queries, [(i % 6, i, 1, 0) for i in range(24)])
    # a row of exactly max_length beside short ones: [CLS] + 20 + [SEP] + 489 + [SEP] = 512 with the one-id pieces
    shapes["max_length_row"] = (_frags(rng, [3, 200, 200, 89, 2]), [q20], [(0, 0, 1, 0), (0, 1, 3, 0), (0, 4, 1, 0)])
    # a clipped first fragment followed by further fragments, clips of 1 and of all but 1
    shapes["clipped_then_more"] = (_frags(rng, [40, 9, 13, 1, 30, 6]), [q20, q20[:3]],
                                   [(0, 0, 4, 17), (1, 0, 2, 1), (0, 4, 2, 29), (1, 1, 3, 8), (1, 2, 2, 0)])
    # 257 rows of 1 - 3 fragments: 771 waves, 193 blocks, the last one ragged; the total is no multiple of 4
    lengths = [int(n) for n in rng.integers(1, 40, 600)]
    plan, first = [], 0
    for i in range(257):
        n = 1 + i % 3
        plan.append((i % 2, first, n, 0 if i % 5 else min(2, lengths[first])))
        first += n
    shapes["ragged_grid"] = (_frags(rng, lengths), [q20[:7], q20], plan)
    # rows without context tokens between ordinary ones (clip: _no_context_clip of the layout)
    shapes["no_context_rows"] = (_frags(rng, [6, 3]), [q20[:5], [], q20], [(0, 0, 1, 0), (2, 1, 0, None), (1, 0, 0, None), (0, 1, 1, 0), (0, 2, 0, None)])
    return shapes


@pytest.mark.parametrize("layout", sorted(LAYOUTS))
@pytest.mark.parametrize("shape", ["one_row", "one_token_contexts", "max_length_row", "clipped_then_more", "ragged_grid", "no_context_rows"])
def test_assemble_rows_reproduces_the_host_rows(model, shape, layout):
    tokenizer, manual, pieces = LAYOUTS[layout]
    found = derive_row_template(lambda q, c: pl.prepare_block_inputs(tokenizer, q, [pl.FragmentRecord("", 0, 0, 0, len(c), list(c))],
                                                                     manual_specials=manual[0], manual_cls=manual[1], manual_sep=manual[2])[0])
    assert (found.prefix, found.middle, found.suffix) == pieces
    # a row without context: the pair tokenizer keeps its suffix, the manual path drops it, the plain one has none
    assert found.empty_context == {"tokenizer_built": "keep", "manual_specials": "drop", "plain_concatenation": "keep"}[layout]
    frags, queries, plan = _shapes()[shape]
    plan = [(q, f, n, (-1 if found.empty_context == "drop" else 0) if clip is None else clip) for q, f, n, clip in plan]
    want = _host_rows(tokenizer, manual, frags, queries, plan)
    if shape == "max_length_row" and layout == "manual_specials":
        assert max(len(r) for r in want) == MAX_LENGTH
    for guard in (64, 61):  # a 16-byte aligned output and one that starts 4 bytes before a boundary
        got, cu, guards = _assemble(model.encoder, frags, queries, plan, pieces, guard=guard)
        assert all((g == POISON).all() for g in guards)
        assert len(cu) - 1 == len(want) and int(cu[-1]) == sum(len(r) for r in want)
        if shape == "ragged_grid":  # (totals of this layout: 13857 / 13600 / 12829 ids; the misaligned output shifts all three)
            assert len(want) == 257 and (int(cu[-1]) % 4 != 0 or layout == "manual_specials")
        if shape in ("one_row", "clipped_then_more") and layout == "manual_specials":
            assert int(cu[-1]) % 4 != 0  # 35 and 185 ids: the last 16-byte store of the batch is a partial one
        for r, row in enumerate(want):
            assert got[cu[r]: cu[r + 1]].tolist() == row, (shape, layout, guard, r)
        # ... and the restatement the CPU tests hold to prepare_block_inputs says the same
        corpus, frag_off, query_ids, q_off = am.flat_arrays(frags, queries)
        assert np.array_equal(got, am.assemble_rows(corpus, frag_off, query_ids, q_off, pieces, plan, cu))


def test_every_refusal_is_invalid_and_enqueues_nothing(model):
    enc = model.encoder
    frags, queries, plan = am.synthetic_case(np.random.default_rng(3))
    corpus, frag_off, query_ids, q_off = am.flat_arrays(frags, queries)
    base, keep = am.build_request(frags, queries, plan)
    total = base.total_tokens
    device = {"corpus_dev": _i32(corpus), "frag_off_dev": _i32(frag_off), "query_ids_dev": _i32(query_ids), "q_off_dev": _i32(q_off),
              "plan_dev": _i32(keep["plan"]), "cu_seqlens_dev": _i32(keep["cu"])}
    out = torch.full((total + 128,), POISON, dtype=torch.int32, device=DEV)
    stream = ctypes.c_void_p(torch.cuda.current_stream(torch.device(DEV)).cuda_stream)

    def call(overrides, out_ptr=out.data_ptr()):
        req, kept = am.build_request(frags, queries, plan, **overrides)
        for name, tensor in device.items():
            if name not in overrides:
                setattr(req, name, tensor.data_ptr())
        return enc.lib.op_assemble_rows(enc._handle, ctypes.byref(req), ctypes.c_void_p(out_ptr) if out_ptr else None, stream), kept

    assert enc.lib.op_assemble_rows(enc._handle, None, ctypes.c_void_p(out.data_ptr()), stream) == _lib.OP_ERR_INVALID
    for label, overrides, word in am.refusal_cases():
        code, _kept = call(overrides)
        assert code == _lib.OP_ERR_INVALID, label
        assert word in _lib.last_error(enc.lib, enc._handle), (label, _lib.last_error(enc.lib, enc._handle))
    code, _kept = call({}, out_ptr=0)
    assert code == _lib.OP_ERR_INVALID and "ids_dev is NULL" in _lib.last_error(enc.lib, enc._handle)
    torch.cuda.synchronize()
    assert bool((out == POISON).all())  # nothing was enqueued
    # the same request, well formed: written, and only inside [0, total)
    code, _kept = call({})
    assert code == _lib.OP_OK, _lib.last_error(enc.lib, enc._handle)
    host = out.cpu().numpy()
    assert np.array_equal(host[:total], am.assemble_rows(corpus, frag_off, query_ids, q_off, am.BERT_PIECES, plan, keep["cu"]))
    assert (host[total:] == POISON).all()
    # the engine's own argument checks
    with pytest.raises(ValueError):
        enc.assemble_rows(device["corpus_dev"], device["frag_off_dev"], frag_off, device["query_ids_dev"], device["q_off_dev"], q_off,
                          am.BERT_PIECES, device["plan_dev"], keep["plan"], device["cu_seqlens_dev"].cpu(), keep["cu"])
    with pytest.raises(_lib.HipLibraryError, match="cu_seqlens_host"):
        wrong = keep["cu"].copy()
        wrong[2] += 1
        enc.assemble_rows(device["corpus_dev"], device["frag_off_dev"], frag_off, device["query_ids_dev"], device["q_off_dev"], q_off,
                          am.BERT_PIECES, device["plan_dev"], keep["plan"], device["cu_seqlens_dev"], wrong)


# -- process() -------------------------------------------------------------------------------------------------------------------------
WORDS = ["alpha", "beta", "gamma", "delta", "epsilon", "zeta", "eta", "theta", "iota", "kappa", "lambda", "mu"]


def _text(rng, chars):
    parts, total = [], 0
    while total < chars:
        sent = " ".join(WORDS[int(i)] for i in rng.integers(0, len(WORDS), int(rng.integers(5, 12)))) + ". "
        parts.append(sent)
        total += len(sent)
    return "".join(parts)[:chars].rstrip() + "."


def _corpus():
    rng = np.random.default_rng(5)
    return [
        _text(rng, 1500),                                       # several blocks at max_length 512
        _text(rng, 300),
        "",                                                     # the fallback sentence, no tokens: this forward's rows come from the host
        [_text(rng, 60) + " ", _text(rng, 90), "  "],           # pre-split sentences
        "Greek letters\n" + _text(rng, 200) + "\n" + _text(rng, 120),
        _text(rng, 470),
        _text(rng, 31),
        _text(rng, 400).replace(".", ",") + ".",                # one long sentence: fragments of 256 and 145 tokens
    ]


QUESTION = "which greek letters appear here"
TITLES = ["Long", "Short", "Nothing", "Split", "Lines", "Usual", "Tiny", "One sentence"]
VIEWS = ([0, 2, 2, 3, 6, 7], [5, 1, 0, 4])
CASES = {
    "default_metrics": (dict(), dict(return_sentence_metrics=True, return_sentence_texts=True, threshold=0.1), QUESTION),
    "explicit_titles": (dict(title=TITLES), dict(always_select_title=True, return_sentence_metrics=True), QUESTION),
    "first_line_no_title": (dict(title=None, first_line_as_title=True), dict(always_select_title=True, return_sentence_texts=True), QUESTION),
    "strip_boundaries": (dict(strip_sentences=True, respect_sentence_boundaries=True), dict(return_sentence_metrics=True, batch_size=2), QUESTION),
    "reorder_top_k": (dict(), dict(reorder=True, top_k=2, return_sentence_metrics=True), QUESTION),
    "clipped": (dict(), dict(return_sentence_metrics=True), " ".join(WORDS * 5)[:300] + "?"),  # 301 + 1 + a 256-token fragment > 510
    "empty_query": (dict(), dict(return_sentence_metrics=True), ""),
}


def _same(got, want):
    assert set(got) == set(want)
    for key in want:
        if key not in ("timing", "performance_trace"):
            assert got[key] == want[key], key


def _raw_kwargs(prep_kwargs, indices_per_query):
    raw = dict(prep_kwargs)
    if isinstance(raw.get("title"), list):
        per_query = [[raw["title"][i] for i in indices] for indices in indices_per_query]
        raw["title"] = per_query[0] if len(per_query) == 1 else per_query
    return raw


@pytest.mark.parametrize("case", sorted(CASES))
def test_process_on_prepared_contexts_is_bit_identical(model, case):
    prep_kwargs, call_kwargs, question = CASES[case]
    corpus = _corpus()
    common = dict(sentence_splitter=period_splitter, show_progress=False)
    prepared = model.prepare_contexts(corpus, sentence_splitter=period_splitter, **prep_kwargs)
    assert not prepared.host_assembled
    assembled = []
    inner = model.encoder.assemble_rows
    model.encoder.assemble_rows = lambda *a, **k: assembled.append(1) or inner(*a, **k)
    try:
        got = model.process(question, prepared, **common, **call_kwargs)
        got_view = model.process(question, prepared.select(VIEWS[0]), **common, **call_kwargs)
        questions = [question, "where is " + WORDS[3]]
        got_two = model.process(questions, [prepared.select(v) for v in VIEWS], **common, **call_kwargs)
    finally:
        del model.encoder.assemble_rows
    assert len(assembled) >= 3  # the rows came from the kernel
    assert prepared._device is not None and prepared._device["ids"].numel() == prepared.n_tokens
    _same(got, model.process(question, corpus, **common, **_raw_kwargs(prep_kwargs, [range(len(corpus))]), **call_kwargs))
    _same(got_view, model.process(question, [corpus[i] for i in VIEWS[0]], **common, **_raw_kwargs(prep_kwargs, [VIEWS[0]]), **call_kwargs))
    _same(got_two, model.process(questions, [[corpus[i] for i in v] for v in VIEWS], **common, **_raw_kwargs(prep_kwargs, VIEWS), **call_kwargs))
    scores = got["reranking_score"]
    assert any(s is not None and np.isfinite(s) for s in scores)
    if case == "clipped":
        *_, plan, _blocks = am.request_plan(model, prepared, [question], [prepared.select(range(len(corpus)))])
        assert any(p[3] > 0 for p in plan)


def test_a_prepared_request_takes_fewer_forwards(model):
    rng = np.random.default_rng(9)
    corpus = [_text(rng, 470) for _ in range(300)]
    common = dict(sentence_splitter=period_splitter, show_progress=False, return_sentence_metrics=True)
    prepared = model.prepare_contexts(corpus, sentence_splitter=period_splitter)
    got = model.process(QUESTION, prepared, **common)
    raw = model.process(QUESTION, corpus, **common)
    _same(got, raw)
    fast, slow = got["performance_trace"].runtime["forwards"], raw["performance_trace"].runtime["forwards"]
    print(f"forwards: prepared {fast}, raw {slow}")
    assert fast["rows"] == slow["rows"] >= 300 and fast["tokens"] == slow["tokens"]
    assert 1 <= fast["launches"] < slow["launches"]


def test_the_running_audit_sees_a_prepared_request(model):
    """A calibrated set under ``audit="running"``: a request whose token ids no audited row has held triggers a coverage
    audit -- on the device-assembled ids (``op_coverage_scan``) exactly as on the host ids of the raw request."""

    from open_provence_amd.config import OpenProvenceConfig
    from open_provence_amd.modeling import OpenProvenceModel
    from open_provence_amd.synthetic import XSMALL, named_dims, refinit_state_dict

    dims = named_dims("xsmall", num_layers=3, vocab_size=500)
    base = dict(XSMALL, vocab_size=500, num_hidden_layers=3, model_type="modernbert", local_attention=128, global_attn_every_n_layers=3,
                global_rope_theta=160000.0, local_rope_theta=10000.0, max_position_embeddings=8192, pad_token_id=0, cls_token_id=1,
                sep_token_id=2)
    cfg = OpenProvenceConfig(base_model_config=base, tokenizer_name_or_path="char-tokenizer", pruning_config={"hidden_size": 256},
                             max_length=256, num_labels=1)
    rng = np.random.default_rng(21)
    first = [_text(rng, 150) for _ in range(6)]
    second = [t.upper() for t in first]  # token ids (code points) the first request never held
    results, audits = {}, {}
    for mode in ("raw", "prepared"):
        audited = OpenProvenceModel(cfg, device=DEV, tokenizer=CharTokenizer(), state_dict=refinit_state_dict(dims, 7), precision="bf16x3",
                                    audit="running")
        chosen = audited.encoder.effective_policy()["kernel_set"]
        assert audited.encoder.audit_mode == "running" and chosen == "f16"  # (calibrated on the library's own batch, first audit pending)
        counts = []
        outs = []
        for texts in (first, first, second):
            context = audited.prepare_contexts(texts, sentence_splitter=period_splitter) if mode == "prepared" else texts
            with warnings.catch_warnings():
                warnings.simplefilter("ignore", RuntimeWarning)
                outs.append(audited.process(QUESTION, context, sentence_splitter=period_splitter, show_progress=False, return_sentence_metrics=True))
            report = (audited.encoder.calibration or {}).get("audits") or {"count": 0, "by_trigger": {}, "last": None}
            counts.append((report["count"], dict(report["by_trigger"]), (report["last"] or {}).get("passed"),
                           audited.encoder.effective_policy()["kernel_set"]))
        results[mode], audits[mode] = outs, (chosen, counts)
    print(audits)
    chosen, counts = audits["prepared"]
    assert audits["prepared"] == audits["raw"]
    # the first request is the first audit (its ids join the coverage), the same request again holds nothing new, the
    # upper-case one holds ids no audited row had
    assert counts[0][0] >= 1 and counts[0][2] is True, counts
    assert counts[1][1].get("coverage", 0) == counts[0][1].get("coverage", 0) < counts[2][1].get("coverage", 0), counts
    for got, want in zip(results["prepared"], results["raw"]):
        _same(got, want)
