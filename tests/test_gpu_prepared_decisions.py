"""Prepared requests whose last stages run on the device: ``op_planned_fragment_means`` and ``op_sentence_decisions`` held to
their restatement (tests/decision_model.py, itself held to the host path by tests/test_decision_model.py) on uint32 / uint64
views with ``==`` -- guard regions, outputs independent of what they held, refusals before anything is enqueued -- and
``process(q, prepared)`` on the xsmall synthetic model with the device path against the host path and the raw-text call in all
result keys with ``==``."""

import ctypes
import warnings

import numpy as np
import pytest
import torch

import decision_model as dm
from helpers import CharTokenizer, period_splitter

from open_provence_amd import _lib

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
MAX_LENGTH = 512
POISON_F32, POISON_I32, POISON_F64, POISON_U8 = -7.5, -1234567, -3.25, 0xA5
THRESHOLDS = (0.0, 0.5, 1.0)


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


# -- the kernels -----------------------------------------------------------------------------------------------------------------------
def _cases():
    rng = np.random.default_rng(41)
    cases = {"boundary": dm.boundary_case(rng), "nan": dm.nan_case(rng), "cut": dm.cut_case(rng)}
    cases.update({f"random{i}": dm.random_case(rng) for i in range(3)})
    return cases


KERNEL_CASES = _cases()  # (built once: the expectations below are computed from them once, too)


def _dev(array, dtype):
    return torch.from_numpy(np.ascontiguousarray(array, dtype=dtype).reshape(-1)).to(DEV)


def _planned_means(enc, case, *, base=0, tail=0, guard=64, fill=(POISON_F32, POISON_I32)):
    """Run op_planned_fragment_means on ``case`` with its slots from ``base`` on in outputs of ``base + n_slots + tail`` slots ->
    (means, slot_frag, the guard regions around both outputs) on the host."""

    n = base + case.n_slots + tail
    mean_buf = torch.full((guard + n + guard,), fill[0], dtype=torch.float32, device=DEV)
    frag_buf = torch.full((guard + n + guard,), fill[1], dtype=torch.int32, device=DEV)
    slot_off = (case.slot_off + base).astype(np.int32)
    frag_shift = case.tables()[0]
    enc.planned_fragment_means(
        _dev(case.frag_off, np.int32), case.frag_off, _dev(case.q_off, np.int32), case.q_off, dm.PIECES, _dev(case.plan, np.int32),
        np.ascontiguousarray(case.plan.reshape(-1)), _dev(case.cu, np.int32), case.cu, torch.from_numpy(case.keep_prob).to(DEV),
        _dev(frag_shift, np.int32), _dev(slot_off, np.int32), slot_off, mean_buf[guard: guard + n], frag_buf[guard: guard + n])
    torch.cuda.synchronize()
    mean_host, frag_host = mean_buf.cpu().numpy(), frag_buf.cpu().numpy()
    guards = (mean_host[:guard], mean_host[guard + n:], frag_host[:guard], frag_host[guard + n:])
    return mean_host[guard: guard + n], frag_host[guard: guard + n], guards


@pytest.mark.parametrize("name", sorted(KERNEL_CASES))
def test_planned_fragment_means_are_the_models(model, name):
    case = KERNEL_CASES[name]
    frag_shift = case.tables()[0]
    want_mean, want_frag = dm.planned_fragment_means(case.keep_prob, case.cu, case.plan.tolist(), case.frag_off, frag_shift, case.q_off,
                                                     case.slot_off, case.n_slots)
    assert np.array_equal(dm.bits(want_mean), dm.bits(case.host_means()))  # (the model is the host path's, here too)
    for base, tail, fill in ((0, 0, (POISON_F32, POISON_I32)), (3, 5, (float("nan"), 77))):
        mean, frag, guards = _planned_means(model.encoder, case, base=base, tail=tail, fill=fill)
        assert np.array_equal(dm.bits(mean[base: base + case.n_slots]), dm.bits(want_mean)), (name, base)
        assert np.array_equal(frag[base: base + case.n_slots], want_frag)
        # guard regions and the slots no row names keep what they held -- whatever that was
        untouched = np.concatenate([guards[0], guards[1], mean[:base], mean[base + case.n_slots:]])
        assert np.array_equal(dm.bits(untouched), dm.bits(np.full(untouched.shape, fill[0], dtype=np.float32)))
        assert (np.concatenate([guards[2], guards[3], frag[:base], frag[base + case.n_slots:]]) == fill[1]).all()


def _decisions(enc, case, means, slot_frag, threshold, always_select_title, *, guard=32, fill=(POISON_F64, POISON_U8)):
    instances, n_out = case.instance_table(always_select_title)
    avg_buf = torch.full((guard + n_out + guard,), fill[0], dtype=torch.float64, device=DEV)
    keep_buf = torch.full((guard + n_out + guard,), fill[1], dtype=torch.uint8, device=DEV)
    frag_sent = case.tables()[1]
    enc.sentence_decisions(_dev(instances, np.int32), np.ascontiguousarray(instances.reshape(-1)), torch.from_numpy(means).to(DEV),
                           _dev(slot_frag, np.int32), _dev(frag_sent, np.int32), threshold, avg_buf[guard: guard + n_out],
                           keep_buf[guard: guard + n_out])
    torch.cuda.synchronize()
    avg_host, keep_host = avg_buf.cpu().numpy(), keep_buf.cpu().numpy()
    guards = (avg_host[:guard], avg_host[guard + n_out:], keep_host[:guard], keep_host[guard + n_out:])
    return avg_host[guard: guard + n_out], keep_host[guard: guard + n_out], guards


@pytest.mark.parametrize("name", sorted(KERNEL_CASES))
def test_sentence_decisions_are_the_models(model, name):
    case = KERNEL_CASES[name]
    frag_shift, frag_sent, _base, _first = case.tables()
    means, slot_frag = dm.planned_fragment_means(case.keep_prob, case.cu, case.plan.tolist(), case.frag_off, frag_shift, case.q_off,
                                                 case.slot_off, case.n_slots)
    for threshold in THRESHOLDS:
        for always_select_title in (False, True):
            instances, n_out = case.instance_table(always_select_title)
            want_avg, want_keep = dm.sentence_decisions(instances.tolist(), means, slot_frag, frag_sent, threshold, n_out)
            for fill in ((POISON_F64, POISON_U8), (float("nan"), 1)):
                avg, keep, guards = _decisions(model.encoder, case, means, slot_frag, threshold, always_select_title, fill=fill)
                assert np.array_equal(dm.bits(avg), dm.bits(want_avg)), (name, threshold, always_select_title)
                assert np.array_equal(keep, want_keep), (name, threshold, always_select_title)
                filled = np.full(guards[0].shape, fill[0], dtype=np.float64)
                assert np.array_equal(dm.bits(guards[0]), dm.bits(filled)) and np.array_equal(dm.bits(guards[1]), dm.bits(filled))
                assert (guards[2] == fill[1]).all() and (guards[3] == fill[1]).all()
    if name == "nan":
        assert np.isnan(means).any() and not np.isnan(want_avg).any()  # a NaN average comes out as 0.0


def test_every_refusal_is_invalid_and_enqueues_nothing(model):
    """The host copies are broken one way at a time while the device copies stay well formed: each call must end with
    OP_ERR_INVALID on the host check, before a kernel could meet the disagreement.  Afterwards every output still holds its fill."""

    enc = model.encoder
    case = KERNEL_CASES["random0"]
    frag_shift, frag_sent, _base, _first = case.tables()
    stream = ctypes.c_void_p(torch.cuda.current_stream(torch.device(DEV)).cuda_stream)
    device = {"frag_off": _dev(case.frag_off, np.int32), "q_off": _dev(case.q_off, np.int32), "plan": _dev(case.plan, np.int32),
              "cu": _dev(case.cu, np.int32), "slot_off": _dev(case.slot_off, np.int32), "frag_shift": _dev(frag_shift, np.int32),
              "keep_prob": torch.from_numpy(case.keep_prob).to(DEV), "frag_sent": _dev(frag_sent, np.int32)}
    mean_out = torch.full((case.n_slots,), POISON_F32, dtype=torch.float32, device=DEV)
    frag_out = torch.full((case.n_slots,), POISON_I32, dtype=torch.int32, device=DEV)

    def means_call(spoil):
        host = {"frag_off": case.frag_off.copy(), "q_off": case.q_off.copy(), "plan": case.plan.reshape(-1).copy(), "cu": case.cu.copy(),
                "slot_off": case.slot_off.copy()}
        piece = np.array([1], dtype=np.int32)
        rows = _lib.OpAssembleRequest()
        rows.struct_bytes = ctypes.sizeof(_lib.OpAssembleRequest)
        rows.n_frag, rows.n_queries, rows.n_rows, rows.total_tokens = case.n_frag, len(case.queries), len(case.plan), int(case.cu[-1])
        rows.n_prefix = rows.n_middle = rows.n_suffix = 1
        rows.prefix = rows.middle = rows.suffix = piece.ctypes.data
        rows.frag_off_dev, rows.q_off_dev = device["frag_off"].data_ptr(), device["q_off"].data_ptr()
        rows.plan_dev, rows.cu_seqlens_dev = device["plan"].data_ptr(), device["cu"].data_ptr()
        req = _lib.OpPlannedMeansRequest()
        req.struct_bytes = ctypes.sizeof(_lib.OpPlannedMeansRequest)
        req.n_slots = case.n_slots
        req.keep_prob_dev, req.frag_shift_dev = device["keep_prob"].data_ptr(), device["frag_shift"].data_ptr()
        req.slot_off_dev = device["slot_off"].data_ptr()
        req.mean_out_dev, req.slot_frag_out_dev = mean_out.data_ptr(), frag_out.data_ptr()
        spoil(rows, req, host)
        rows.frag_off_host, rows.q_off_host = host["frag_off"].ctypes.data, host["q_off"].ctypes.data
        rows.plan_host, rows.cu_seqlens_host = host["plan"].ctypes.data, host["cu"].ctypes.data
        req.slot_off_host = host["slot_off"].ctypes.data
        return enc.lib.op_planned_fragment_means(enc._handle, ctypes.byref(rows), ctypes.byref(req), stream)

    def set_at(key, at, value):
        def spoil(_rows, _req, host):
            host[key][at] = value
        return spoil

    n_rows = len(case.plan)
    means_refusals = [
        ("struct_bytes", lambda rows, req, host: setattr(req, "struct_bytes", 12), "struct_bytes"),
        ("rows struct_bytes", lambda rows, req, host: setattr(rows, "struct_bytes", 12), "struct_bytes"),
        ("negative slots", lambda rows, req, host: setattr(req, "n_slots", -1), "negative count"),
        ("negative rows", lambda rows, req, host: setattr(rows, "n_rows", -2), "negative count"),
        ("null keep_prob", lambda rows, req, host: setattr(req, "keep_prob_dev", None), "keep_prob_dev is NULL"),
        ("null mean_out", lambda rows, req, host: setattr(req, "mean_out_dev", None), "mean_out_dev"),
        ("null frag_shift", lambda rows, req, host: setattr(req, "frag_shift_dev", None), "NULL"),
        ("null slot_off", lambda rows, req, host: setattr(req, "slot_off_dev", None), "NULL"),
        ("query outside", set_at("plan", 0, len(case.queries)), "names query"),
        ("fragments past the corpus", set_at("plan", 4 * (n_rows - 1) + 1, case.n_frag), "takes fragments"),
        ("negative fragment count", set_at("plan", 2, -1), "takes fragments"),
        ("clip beyond the fragment", set_at("plan", 3, 1 << 20), "clips its first fragment"),
        ("slot_off not prefix sums", set_at("slot_off", n_rows, case.n_slots - 1), "slot_off_host"),
        ("slot_off past the outputs", lambda rows, req, host: host["slot_off"].__iadd__(1), "slots"),
        ("slot_off negative", set_at("slot_off", 0, -1), "slot_off_host[0]"),
        ("cu end", set_at("cu", n_rows, int(case.cu[-1]) + 1), "cu_seqlens_host"),
        ("frag_off from 1", set_at("frag_off", 0, 1), "do not start at 0"),
    ]
    assert enc.lib.op_planned_fragment_means(enc._handle, None, None, stream) == _lib.OP_ERR_INVALID
    for label, spoil, word in means_refusals:
        assert means_call(spoil) == _lib.OP_ERR_INVALID, label
        assert word in _lib.last_error(enc.lib, enc._handle), (label, _lib.last_error(enc.lib, enc._handle))

    means, slot_frag = dm.planned_fragment_means(case.keep_prob, case.cu, case.plan.tolist(), case.frag_off, frag_shift, case.q_off,
                                                 case.slot_off, case.n_slots)
    instances, n_out = case.instance_table(True)
    means_dev, slot_frag_dev, instances_dev = torch.from_numpy(means).to(DEV), _dev(slot_frag, np.int32), _dev(instances, np.int32)
    avg_out = torch.full((n_out,), POISON_F64, dtype=torch.float64, device=DEV)
    keep_out = torch.full((n_out,), POISON_U8, dtype=torch.uint8, device=DEV)

    def decisions_call(spoil):
        host = instances.reshape(-1).copy()
        req = _lib.OpDecisionsRequest()
        req.struct_bytes = ctypes.sizeof(_lib.OpDecisionsRequest)
        req.n_instances, req.n_slots, req.n_frag, req.n_out = len(instances), case.n_slots, case.n_frag, n_out
        req.threshold = 0.5
        req.instances_dev, req.mean_dev, req.slot_frag_dev = instances_dev.data_ptr(), means_dev.data_ptr(), slot_frag_dev.data_ptr()
        req.frag_sent_dev, req.avg_out_dev, req.keep_out_dev = device["frag_sent"].data_ptr(), avg_out.data_ptr(), keep_out.data_ptr()
        spoil(req, host)
        req.instances_host = host.ctypes.data
        return enc.lib.op_sentence_decisions(enc._handle, ctypes.byref(req), stream)

    def word_at(at, value):
        def spoil(_req, host):
            host[at] = value
        return spoil

    last = 6 * (len(instances) - 1)
    decisions_refusals = [
        ("struct_bytes", lambda req, host: setattr(req, "struct_bytes", 16), "struct_bytes"),
        ("negative instances", lambda req, host: setattr(req, "n_instances", -1), "negative count"),
        ("null avg_out", lambda req, host: setattr(req, "avg_out_dev", None), "avg_out_dev"),
        ("null means", lambda req, host: setattr(req, "mean_dev", None), "mean_dev"),
        ("null instances", lambda req, host: setattr(req, "instances_dev", None), "instances buffer"),
        ("slots past the buffer", word_at(last + 1, case.n_slots + 1), "takes slots"),
        ("slots backwards", word_at(0, int(instances[0, 1]) + 1), "takes slots"),
        ("sentences past the outputs", word_at(last + 3, int(instances[-1, 3]) + 1), "writes sentences"),
        ("sentences elsewhere", word_at(last + 2, int(instances[-1, 2]) + 1), "writes sentences"),
        ("outputs not tiled", lambda req, host: setattr(req, "n_out", n_out + 1), "n_out is"),
        ("title past the sentences", word_at(5, int(instances[0, 3])), "title_index"),
        ("title below -1", word_at(5, -2), "title_index"),
        ("negative sentence base", word_at(4, -1), "item_sent_base"),
    ]
    assert enc.lib.op_sentence_decisions(enc._handle, None, stream) == _lib.OP_ERR_INVALID
    for label, spoil, word in decisions_refusals:
        assert decisions_call(spoil) == _lib.OP_ERR_INVALID, label
        assert word in _lib.last_error(enc.lib, enc._handle), (label, _lib.last_error(enc.lib, enc._handle))

    torch.cuda.synchronize()
    assert bool((mean_out == POISON_F32).all()) and bool((frag_out == POISON_I32).all())  # nothing was enqueued
    assert bool((avg_out == POISON_F64).all()) and bool((keep_out == POISON_U8).all())
    # the same requests, well formed: accepted, and the outputs are the model's
    assert means_call(lambda rows, req, host: None) == _lib.OP_OK, _lib.last_error(enc.lib, enc._handle)
    assert decisions_call(lambda req, host: None) == _lib.OP_OK, _lib.last_error(enc.lib, enc._handle)
    torch.cuda.synchronize()
    want_avg, want_keep = dm.sentence_decisions(instances.tolist(), means, slot_frag, frag_sent, 0.5, n_out)
    assert np.array_equal(dm.bits(mean_out.cpu().numpy()), dm.bits(means)) and np.array_equal(frag_out.cpu().numpy(), slot_frag)
    assert np.array_equal(dm.bits(avg_out.cpu().numpy()), dm.bits(want_avg)) and np.array_equal(keep_out.cpu().numpy(), want_keep)
    # the engine's own argument checks
    with pytest.raises(ValueError):
        enc.sentence_decisions(instances_dev, instances.reshape(-1).astype(np.int64), means_dev, slot_frag_dev, device["frag_sent"], 0.5)
    with pytest.raises(_lib.HipLibraryError, match="title_index"):
        wrong = instances.copy()
        wrong[0, 5] = wrong[0, 3]
        enc.sentence_decisions(instances_dev, np.ascontiguousarray(wrong.reshape(-1)), means_dev, slot_frag_dev, device["frag_sent"], 0.5)


# -- process() -------------------------------------------------------------------------------------------------------------------------
# One token per character (id = code point): the texts are lower case and the questions upper case, so that no block begins with
# an id of its question -- a request where one does takes the host path (test_fallbacks_*).
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
        _text(rng, 1500),                                       # longer than max_length 512: several blocks
        _text(rng, 300),
        [_text(rng, 60) + " ", _text(rng, 90), "  "],           # pre-split sentences
        "greek letters\n" + _text(rng, 200) + "\n" + _text(rng, 120),
        _text(rng, 470),
        _text(rng, 31),
        _text(rng, 400).replace(".", ",") + ".",                # one long sentence: fragments of 256 and 145 tokens
    ]


QUESTION = "WHICH_GREEK_LETTERS_APPEAR_HERE?"
SECOND_QUESTION = "WHERE_IS_DELTA?"
TITLES = ["long", "short", "split", "lines", "usual", "tiny", "one sentence"]
VIEWS = ([0, 2, 2, 3, 6, 5, 0], [4, 1, 0, 3])  # (repeated indices in the first)
METRICS = dict(return_sentence_metrics=True, return_sentence_texts=True)
CASES = {
    "default_title_threshold_0": (dict(), dict(METRICS, threshold=0.0), QUESTION),
    "default_title_threshold_half": (dict(), dict(METRICS, threshold=0.5, always_select_title=True), QUESTION),
    "default_title_threshold_1": (dict(), dict(METRICS, threshold=1.0, always_select_title=True), QUESTION),
    "no_title": (dict(title=None), dict(METRICS, always_select_title=True, threshold=0.1), QUESTION),
    "explicit_titles": (dict(title=TITLES), dict(METRICS, always_select_title=True, threshold=0.1), QUESTION),
    "explicit_titles_not_selected": (dict(title=TITLES), dict(METRICS, threshold=0.1, use_best_reranker_score=False), QUESTION),
    "first_line_title": (dict(title=None, first_line_as_title=True), dict(METRICS, always_select_title=True), QUESTION),
    "reorder_top_k": (dict(), dict(METRICS, reorder=True, top_k=2), QUESTION),
    "clipped": (dict(), dict(METRICS), "_".join(w.upper() for w in WORDS * 5)[:300] + "?"),  # 301 + 1 + a 256-token fragment > 510
    "plain_outputs": (dict(), dict(threshold=0.1), QUESTION),
}
_PREPARED = {}


def _prepared(model, prep_kwargs):
    key = repr(sorted(prep_kwargs.items()))
    if key not in _PREPARED:
        _PREPARED[key] = model.prepare_contexts(_corpus(), sentence_splitter=period_splitter, **prep_kwargs)
    return _PREPARED[key]


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


def _decisions_of(result):
    return result["performance_trace"].runtime["prepared_decisions"]


@pytest.mark.parametrize("case", sorted(CASES))
def test_process_with_device_decisions_is_bit_identical(model, monkeypatch, case):
    prep_kwargs, call_kwargs, question = CASES[case]
    corpus = _corpus()
    common = dict(sentence_splitter=period_splitter, show_progress=False)
    prepared = _prepared(model, prep_kwargs)
    assert prepared.decision_tables() is not None
    questions = [question, SECOND_QUESTION]
    requests = [  # (question, prepared contexts, the raw-text call's contexts and the indices its titles follow)
        (question, prepared, corpus, [range(len(corpus))]),
        (question, prepared.select(VIEWS[0]), [corpus[i] for i in VIEWS[0]], [VIEWS[0]]),
        (questions, [prepared.select(v) for v in VIEWS], [[corpus[i] for i in v] for v in VIEWS], VIEWS),
    ]
    planned = []
    inner = model.encoder.planned_fragment_means
    model.encoder.planned_fragment_means = lambda *a, **k: planned.append(1) or inner(*a, **k)
    try:
        for q, contexts, raw_contexts, indices in requests:
            monkeypatch.setenv("OPEN_PROVENCE_PREPARED_DECISIONS", "1")
            on = model.process(q, contexts, **common, **call_kwargs)
            launches = len(planned)
            monkeypatch.setenv("OPEN_PROVENCE_PREPARED_DECISIONS", "0")
            off = model.process(q, contexts, **common, **call_kwargs)
            assert len(planned) == launches  # (switched off: the host stages)
            raw = model.process(q, raw_contexts, **common, **_raw_kwargs(prep_kwargs, indices), **call_kwargs)
            assert _decisions_of(on) == "device" and _decisions_of(off) == "host"
            assert "prepared_decisions" not in raw["performance_trace"].runtime
            _same(on, off)
            _same(on, raw)
            assert on["performance_trace"].runtime["forwards"] == off["performance_trace"].runtime["forwards"]
    finally:
        del model.encoder.planned_fragment_means
    assert len(planned) >= 3  # the means came from the kernel
    scores = on["reranking_score"]
    assert any(s is not None and np.isfinite(s) for row in scores for s in row)
    if case == "clipped":
        item = prepared.items[6]
        plan = item.blocks_for(model.tokenizer, len(question), 1, model.max_length)[1]
        assert any(clip > 0 for _first, _count, clip, _ctx in plan)
    if case in ("default_title_threshold_0", "default_title_threshold_1"):  # everything is above 0.0, nothing above 1.0
        kept = [s for per_query in on["kept_sentences"] for ctx in per_query for s in ctx]
        assert (len(kept) == 0) == (call_kwargs["threshold"] == 1.0)


def test_fallbacks_report_host_and_stay_equal(model, monkeypatch):
    """A request with an empty context (a row without context tokens), and one whose context begins with a token id of its
    question: both take the host stages, and say so."""

    monkeypatch.setenv("OPEN_PROVENCE_PREPARED_DECISIONS", "1")
    common = dict(sentence_splitter=period_splitter, show_progress=False, **METRICS)
    rng = np.random.default_rng(12)
    with_empty = [_text(rng, 200), "", _text(rng, 90)]
    prepared = model.prepare_contexts(with_empty, sentence_splitter=period_splitter)
    got = model.process(QUESTION, prepared, **common)
    assert _decisions_of(got) == "host"
    _same(got, model.process(QUESTION, with_empty, **common))
    # ... without the empty context the same corpus is scored on the device
    assert _decisions_of(model.process(QUESTION, prepared.select([0, 2]), **common)) == "device"

    texts = [_text(rng, 200), _text(rng, 90)]
    prepared = model.prepare_contexts(texts, sentence_splitter=period_splitter)
    lower = "which of " + " ".join(WORDS)  # (holds the first letter of every word of the texts)
    assert texts[0][0] in lower
    got = model.process(lower, prepared, **common)
    assert _decisions_of(got) == "host"
    _same(got, model.process(lower, texts, **common))
    on = model.process(QUESTION, prepared, **common)
    assert _decisions_of(on) == "device"
    _same(on, model.process(QUESTION, texts, **common))


def test_the_range_guards_repeat_takes_the_planned_means_again():
    """A checkpoint whose activations leave fp16's range (tests/test_gpu_policy.py): the first launch comes back non-finite, the
    range guard repeats it on the (hi, lo) bf16 sets -- and the repeat's fragment means must land in the same slots, so that the
    device path equals a model that never ran the fp16 + e4m3 sets."""

    import os

    import test_gpu_policy as policy
    from open_provence_amd.config import OpenProvenceConfig
    from open_provence_amd.modeling import OpenProvenceModel

    meta, _dims, _rows, state = policy._overflowing_state()
    cfg = OpenProvenceConfig(base_model_config=meta["base_model_config"], tokenizer_name_or_path="x",
                             pruning_config={"hidden_size": meta["base_model_config"]["hidden_size"]}, max_length=512)
    text = "alpha beta gamma. delta epsilon zeta eta. theta iota kappa lambda mu. " * 6
    texts = [text, text[:120], text[:300]]
    common = dict(sentence_splitter=period_splitter, show_progress=False, **METRICS)
    results = {}
    old = {name: os.environ.pop(name, None) for name in ("OPEN_PROVENCE_NO_F8", "OPEN_PROVENCE_PREPARED_DECISIONS")}
    try:
        for no_f8 in (True, False):
            if no_f8:
                os.environ["OPEN_PROVENCE_NO_F8"] = "1"
            else:
                os.environ.pop("OPEN_PROVENCE_NO_F8", None)
            model = OpenProvenceModel(cfg, device="cuda", tokenizer=CharTokenizer(), state_dict=state, calibrate=False)
            os.environ["OPEN_PROVENCE_PREPARED_DECISIONS"] = "1"
            prepared = model.prepare_contexts(texts, sentence_splitter=period_splitter)
            assert model.encoder.f8_active() == (not no_f8)
            with warnings.catch_warnings(record=True):
                warnings.simplefilter("always")
                results[no_f8] = model.process("WHAT_IS_GAMMA?", prepared, **common)
            assert not model.encoder.f8_active() and _decisions_of(results[no_f8]) == "device"
    finally:
        for name, value in old.items():
            os.environ.pop(name, None)
            if value is not None:
                os.environ[name] = value
    _same(results[False], results[True])
    assert int(results[False]["performance_trace"].runtime["fallback_from_f8"]) >= 1
    assert all(s is not None and np.isfinite(s) for s in results[False]["reranking_score"])
