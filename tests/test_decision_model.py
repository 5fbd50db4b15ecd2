"""The restatement of ``op_planned_fragment_means`` / ``op_sentence_decisions`` (tests/decision_model.py) held to the product's
host path without a GPU: the means to ``pl.fragment_token_ranges`` + ``pl.mean_f32_slice``, the averages and keep flags to
``pl.postprocess_contexts`` (``sentence_probabilities`` and ``kept_sentences``), the corpus tables to
``PreparedContexts.decision_tables``, and ``pl.postprocess_decided`` to ``pl.postprocess_contexts`` in every field -- all on bits.
Each mutation of the restatement must change a result; the host checks of the two calls are held by tests/host/decide_check.cpp
under AddressSanitizer and UBSan."""

from __future__ import annotations

import ctypes
import re
import shutil
import subprocess
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import pytest

import decision_model as dm
from open_provence_amd import _lib, pipeline as pl
from open_provence_amd.prepared import PreparedContexts, PreparedItem

ROOT = Path(__file__).resolve().parents[1]
THRESHOLDS = (0.0, 0.5, 1.0)


def _cases():
    rng = np.random.default_rng(41)
    return [dm.boundary_case(rng), dm.nan_case(rng), dm.cut_case(rng)] + [dm.random_case(rng) for _ in range(40)]


CASES = _cases()


def _model_outputs(case, threshold, always_select_title, mutate=None):
    frag_shift, frag_sent, _sent_base, _first = case.tables(mutate=mutate)
    means, slot_frag = dm.planned_fragment_means(case.keep_prob, case.cu, case.plan.tolist(), case.frag_off, frag_shift, case.q_off,
                                                 case.slot_off, case.n_slots, mutate=mutate)
    instances, n_out = case.instance_table(always_select_title)
    avg, keep = dm.sentence_decisions(instances.tolist(), means, slot_frag, frag_sent, threshold, n_out, mutate=mutate)
    return means, slot_frag, avg, keep, instances


def test_pairwise_sum_is_numpys_bit_for_bit():
    rng = np.random.default_rng(1)
    for dtype in (np.float32, np.float64):
        for n in (1, 2, 7, 8, 9, 15, 16, 17, 127, 128, 129, 130, 255, 256, 257, 264, 1000):
            for _ in range(20):
                values = (rng.random(n) * 10.0 ** int(rng.integers(-3, 4))).astype(dtype)
                assert dm.bits(np.array([dm.pairwise_sum(values)], dtype=dtype))[0] == dm.bits(np.array([np.add.reduce(values)], dtype=dtype))[0], (dtype, n)


def test_means_are_the_host_paths():
    for case in CASES:
        means, slot_frag, *_ = _model_outputs(case, 0.5, False)
        assert np.array_equal(dm.bits(means), dm.bits(case.host_means()))
        want = [f for _q, first, n, _c in case.plan.tolist() for f in range(first, first + n)]
        assert slot_frag.tolist() == want


def test_the_cases_cover_what_they_are_for():
    boundary, nan, cut = CASES[:3]
    means = _model_outputs(boundary, 0.5, False)[0]
    assert (boundary.tables()[0] > 0).any() and (boundary.plan[:, 3] > 0).any()
    # the fragments of "shifted away" behind its title: ranges shifted to empty
    shifted = boundary.slot_off[sum(len(blocks) for _q, _at, blocks in boundary.instances[:4])]
    assert means[shifted + 1] == 1.0 and means[shifted + 2] == 1.0 and means[shifted] != 1.0
    sizes = {n for item in boundary.items for n in np.bincount([f.sentence_index for f in item.fragments]).tolist()}
    assert {1, 2, 8, 9, 129, 130} <= sizes
    assert {1, 7, 8, 9, 127, 128, 129} <= {f.token_length for item in boundary.items for f in item.fragments}
    assert np.isnan(_model_outputs(nan, 0.5, False)[0]).any()
    assert int(cut.cu[1]) < 1 + 2 + 1 + sum(f.token_length for f in cut.items[0].fragments) + 1


@pytest.mark.parametrize("always_select_title", [False, True])
@pytest.mark.parametrize("threshold", THRESHOLDS)
def test_decisions_are_postprocess_contexts(threshold, always_select_title):
    options = dict(threshold=threshold, always_select_title=always_select_title, use_best_reranker_score=True, want_sentence_probabilities=True,
                   want_sentence_texts=True, first_line_as_title=False, zero_score_when_empty=False)
    kept_some = kept_none = 0
    for case in CASES:
        means, _slot_frag, avg, keep, instances = _model_outputs(case, threshold, always_select_title)
        host = case.host_result(means, [0.25] * len(case.plan), **options)
        for c_idx, (_sb, _se, out, n, _base, title) in enumerate(instances.tolist()):
            item = case.items[case.instances[c_idx][1]]
            want = np.array(host.sentence_probabilities[0][c_idx], dtype=np.float64)
            assert np.array_equal(dm.bits(avg[out: out + n]), dm.bits(want))
            assert [s for s, k in zip(item.sentences, keep[out: out + n]) if k] == host.kept_sentences[0][c_idx]
            if title >= 0:
                kept_some += bool(keep[out: out + n].any())
                kept_none += not keep[out: out + n].any()
    if always_select_title:  # the title rule met both ways: nothing is above 1.0 (the title is not kept either), something is above 0.5
        assert kept_none if threshold == 1.0 else kept_some


def test_a_nan_average_is_zero():
    case = CASES[1]
    means, _slot_frag, avg, keep, _instances = _model_outputs(case, 0.0, True)
    assert np.isnan(means).any() and not np.isnan(avg).any()
    nan_kept = _model_outputs(case, 0.0, True, mutate="nan_kept")[2]
    assert np.isnan(nan_kept).any()


@pytest.mark.parametrize("mutate", dm.MUTATIONS)
def test_every_mutation_changes_a_result(mutate):
    changed = 0
    for case in CASES[:3]:
        for threshold in THRESHOLDS:
            good = _model_outputs(case, threshold, True)
            bad = _model_outputs(case, threshold, True, mutate=mutate)
            changed += any(not np.array_equal(dm.bits(g), dm.bits(b)) for g, b in zip(good[:4], bad[:4]))
    assert changed, mutate


# -- the product's tables and its flat post-processing ---------------------------------------------------------------------------
def _prepared(case) -> PreparedContexts:
    model = SimpleNamespace(tokenizer=None, max_length=512)
    items, base = [], 0
    for item in case.items:
        job = {"context_text": item.context_text, "sentences": item.sentences, "prefix_sentences": item.prefix_sentences,
               "prefix_token_counts": item.prefix_token_counts, "title_is_first_sentence": item.title_is_first_sentence, "fragments": item.fragments}
        items.append(PreparedItem(item.entry, job, base))
        base += len(item.fragments)
    return PreparedContexts(model, items, {}, None, {})


def test_the_products_tables_are_the_restated_ones():
    for case in CASES:
        tables = _prepared(case).decision_tables()
        frag_shift, frag_sent, sent_base, first_id = case.tables()
        assert tables is not None
        for name, want in (("frag_shift", frag_shift), ("frag_sent", frag_sent), ("sent_base", sent_base), ("frag_first_id", first_id)):
            assert tables[name].dtype == np.int32 and np.array_equal(tables[name], want), name
        titles = [row[5] for row in case.instance_table(True)[0].tolist()]
        assert titles == [int(tables["item_title"][at]) for _q, at, _b in case.instances]


def test_corpora_the_device_cannot_walk_are_not_eligible():
    rng = np.random.default_rng(2)
    for spoil in ("decreasing", "outside"):
        case = dm.random_case(rng)
        item = max(case.items, key=lambda it: len(it.fragments))
        if spoil == "decreasing":
            item.fragments.append(pl.FragmentRecord("x", 0, 9, 99, 1, [5]))
            item.fragments.insert(0, pl.FragmentRecord("y", 1, 9, 98, 1, [5]))
            item.sentences.append("one more. ")
        else:
            item.fragments[-1].sentence_index = len(item.sentences)
        assert _prepared(case).decision_tables() is None, spoil
    # a fragment without tokens (an empty context's fallback sentence) leaves the corpus eligible: its first id is -1, and a
    # request that takes a row from it keeps the host stages (tests/test_gpu_prepared_decisions.py)
    case = dm.random_case(rng)
    case.items[0].fragments[0].token_ids = []
    assert int(_prepared(case).decision_tables()["frag_first_id"][0]) == -1


@pytest.mark.parametrize("options", [
    dict(use_best_reranker_score=False, first_line_as_title=False, zero_score_when_empty=False),
    dict(use_best_reranker_score=True, first_line_as_title=True, zero_score_when_empty=True),
])
@pytest.mark.parametrize("threshold", THRESHOLDS)
def test_postprocess_decided_is_postprocess_contexts(threshold, options):
    rng = np.random.default_rng(8)
    for case in CASES:
        for always_select_title in (False, True):
            means, _slot_frag, avg, keep, instances = _model_outputs(case, threshold, always_select_title)
            scores = rng.random(len(case.plan)).tolist()
            if len(scores) > 2:
                scores[1] = float("nan")
            full = dict(options, threshold=threshold, always_select_title=always_select_title, want_sentence_probabilities=True, want_sentence_texts=True)
            want = case.host_result(means, scores, **full)
            rows, first = [], 0
            for _q, _at, blocks in case.instances:
                rows.append((first, first + len(blocks)))
                first += len(blocks)
            del full["threshold"], full["always_select_title"]
            got = pl.postprocess_decided(
                [""], [[case.items[at].entry for _q, at, _b in case.instances]], [[case.items[at] for _q, at, _b in case.instances]],
                [list(range(len(case.instances)))], rows, instances[:, 2], scores, avg, keep, **full)
            assert repr(got.as_tuple()) == repr(want.as_tuple())  # (repr: NaN scores compare equal, floats print round-trip exact)


def test_contexts_without_rows_keep_their_branches():
    rng = np.random.default_rng(4)
    empty = dm.Item("", "", [], [], [], False, [])
    unblocked = dm.make_item(rng, "no blocks", 1, [1, 1], [3, 2])
    options = dict(use_best_reranker_score=False, want_sentence_probabilities=True, want_sentence_texts=True, first_line_as_title=True,
                   zero_score_when_empty=False)
    got = pl.postprocess_decided(["q"], [[empty.entry, unblocked.entry]], [[empty, unblocked]], [[-1, -1]], [], np.zeros(0, dtype=np.int64), [],
                                 np.zeros(0), np.zeros(0, dtype=np.uint8), **options)
    state = pl.ContextState(list(unblocked.sentences), unblocked.fragments, [], 1, unblocked.prefix_sentences, unblocked.prefix_token_counts,
                            False, unblocked.context_text)
    want = pl.postprocess_contexts(["q"], [[empty.entry, unblocked.entry]], {(0, 1): state}, threshold=0.5, always_select_title=True, **options)
    assert got == want and got.sentence_probabilities == [[[], [1.0, 1.0]]] and got.titles == [[None, unblocked.sentences[0]]]


# -- header and binding ----------------------------------------------------------------------------------------------------------------
def test_the_two_calls_are_declared_and_bound(hip_library):
    header = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "open_provence_hip.h").read_text(), flags=re.S)
    assert _lib.OP_ABI_VERSION == 10 == hip_library.op_abi_version()
    for name in ("op_planned_fragment_means", "op_sentence_decisions"):
        assert name in _lib.EXPORTED_SYMBOLS and re.search(rf"\bint {name}\s*\(", header) and hasattr(hip_library, name), name
    assert re.search(r"#define OP_DECISIONS_INSTANCE_WORDS 6\b", header) and _lib.OP_DECISIONS_INSTANCE_WORDS == 6
    assert hip_library.op_planned_fragment_means.argtypes[2] is ctypes.POINTER(_lib.OpPlannedMeansRequest)
    assert hip_library.op_sentence_decisions.argtypes[1] is ctypes.POINTER(_lib.OpDecisionsRequest)
    # 2 x 4 bytes, then 6 pointers; 5 x 4 bytes + 4 of padding, a double, then 7 pointers
    assert ctypes.sizeof(_lib.OpPlannedMeansRequest) == 8 + 6 * 8 and _lib.OpPlannedMeansRequest.keep_prob_dev.offset == 8
    assert ctypes.sizeof(_lib.OpDecisionsRequest) == 24 + 8 + 7 * 8 and _lib.OpDecisionsRequest.threshold.offset == 24
    # refused before the handle is looked at: a NULL request with a NULL handle is OP_ERR_INVALID, not a crash
    assert hip_library.op_sentence_decisions(None, None, None) == _lib.OP_ERR_INVALID
    assert hip_library.op_planned_fragment_means(None, None, None, None) == _lib.OP_ERR_INVALID


# -- the host checks (csrc/op_plan.h) under a host sanitizer ------------------------------------------------------------------------
SOURCE = ROOT / "tests" / "host" / "decide_check.cpp"
SANITIZE = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]


def test_every_refusal_of_the_host_checks(tmp_path):
    """tests/host/decide_check.cpp has a main of its own and no HIP: it builds a well-formed pair of requests, breaks them one
    way at a time and prints ``label code message`` per attempt; compiled with the host C++ compiler under AddressSanitizer
    and UBSan (a plain build where the sanitized link fails, as tests/test_plan_host.py does)."""

    compilers = [c for c in (shutil.which("c++"), shutil.which("g++"), "/opt/rocm/llvm/bin/clang++") if c and Path(c).exists()]
    assert compilers, "no host C++ compiler"
    exe, done, errors = tmp_path / "decide_check", None, []
    for extra in (SANITIZE, []):
        for cxx in compilers:
            built = subprocess.run([cxx, "-std=c++17", "-O1", "-g", *extra, str(SOURCE), "-o", str(exe)], capture_output=True, text=True)
            if built.returncode == 0:
                done = subprocess.run([str(exe)], capture_output=True, text=True)
                if done.returncode == 0:
                    break
                errors.append(f"{cxx} {' '.join(extra)}: exit {done.returncode}: {done.stderr[-2000:]}")
                done = None
            else:
                errors.append(f"{cxx} {' '.join(extra)}: {built.stderr[-2000:]}")
        if done is not None:
            break
    assert done is not None, "decide_check.cpp does not build or run:\n" + "\n".join(errors)
    lines = [line.split(" ", 2) for line in done.stdout.splitlines()]
    seen = {label: (int(code), message) for label, code, message in lines}
    assert seen.pop("means:well_formed") == (0, "-") and seen.pop("decisions:well_formed") == (0, "-")
    assert seen.pop("means:no_rows") == (0, "-") and seen.pop("decisions:no_instances") == (0, "-")
    expected = {  # label -> a word of the refusal
        "means:null_rows": "rows is NULL", "means:null_request": "request is NULL", "means:rows_struct_bytes": "op_assemble_request.struct_bytes",
        "means:struct_bytes": "op_planned_means_request.struct_bytes", "means:negative_rows": "negative count", "means:negative_slots": "negative count",
        "means:negative_total": "negative count", "means:null_plan_host": "NULL", "means:null_plan_dev": "NULL", "means:null_cu_host": "NULL",
        "means:null_frag_off_host": "NULL", "means:null_q_off_dev": "NULL", "means:null_slot_off_host": "NULL", "means:null_slot_off_dev": "NULL",
        "means:null_frag_shift": "NULL", "means:null_keep_prob": "keep_prob_dev is NULL", "means:null_mean_out": "mean_out_dev or slot_frag_out_dev",
        "means:null_slot_frag_out": "mean_out_dev or slot_frag_out_dev", "means:query_outside": "names query 2", "means:negative_query": "names query -1",
        "means:fragments_past_the_corpus": "takes fragments", "means:negative_first_fragment": "takes fragments",
        "means:negative_fragment_count": "takes fragments", "means:clip_beyond_the_fragment": "clips its first fragment",
        "means:negative_clip": "clips its first fragment", "means:frag_off_decreases": "frag_off decreases", "means:q_off_decreases": "q_off decreases",
        "means:offsets_from_1": "do not start at 0", "means:cu_start": "cu_seqlens_host runs from 1", "means:cu_end": "cu_seqlens_host runs from 0 to",
        "means:cu_decreases": "cu_seqlens_host decreases at row 1", "means:slot_off_negative": "slot_off_host[0] is -1",
        "means:slot_off_not_prefix_sums": "slot_off_host[2]", "means:slot_off_past_the_outputs": "of 5 slots",
        "decisions:null_request": "request is NULL", "decisions:struct_bytes": "struct_bytes", "decisions:negative_instances": "negative count",
        "decisions:negative_slots": "negative count", "decisions:negative_frag": "negative count", "decisions:negative_out": "negative count",
        "decisions:null_instances_dev": "instances buffer is NULL", "decisions:null_instances_host": "instances buffer is NULL",
        "decisions:null_mean": "mean_dev or slot_frag_dev", "decisions:null_slot_frag": "mean_dev or slot_frag_dev",
        "decisions:null_frag_sent": "frag_sent_dev is NULL", "decisions:null_avg_out": "avg_out_dev or keep_out_dev",
        "decisions:null_keep_out": "avg_out_dev or keep_out_dev", "decisions:slots_past_the_buffer": "takes slots", "decisions:negative_slot": "takes slots",
        "decisions:slots_backwards": "takes slots", "decisions:sentences_past_the_outputs": "writes sentences",
        "decisions:sentences_overlap": "writes sentences", "decisions:negative_sentences": "writes sentences",
        "decisions:outputs_not_tiled": "n_out is", "decisions:negative_sent_base": "item_sent_base -1",
        "decisions:title_past_the_sentences": "title_index 3 outside [-1, 3)", "decisions:title_below_minus_one": "title_index -2",
    }
    assert set(seen) == set(expected)
    for label, word in expected.items():
        code, message = seen[label]
        assert code == _lib.OP_ERR_INVALID and word in message, (label, code, message)
