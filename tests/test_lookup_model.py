"""The restatement of ``op_located_fragment_means`` (tests/lookup_model.py) held to the product's host path without a GPU:
where ``pl.prepare_block_inputs`` finds a context in its row, and the means ``pl.fragment_token_ranges`` +
``pl.mean_f32_slice`` give from there -- on a fuzz of 2000 rows over the alphabet {2, 97, 98}, whose short queries and contexts
repeat each other often enough that every way a search can go wrong shows: each mutation of the restatement must change a
result.  The host check of the call is held by tests/host/locate_check.cpp under AddressSanitizer and UBSan.

``after_prefix`` (a search that starts behind the prefix) cannot show on that alphabet: the prefix is the id 1, which no row of
it holds elsewhere.  ``PREFIX_ROWS`` -- 200 more rows over {1, 2, 97}, held to the host path in the same way -- are there for
it; the shares below are asserted on the 2000 rows alone."""

from __future__ import annotations

import ctypes
import re
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

import lookup_model as lm
from helpers import CharTokenizer
from open_provence_amd import _lib, pipeline as pl

ROOT = Path(__file__).resolve().parents[1]
TOKENIZER = CharTokenizer()
N_FUZZ = 2000


def _fuzz():
    rng = np.random.default_rng(7)
    return lm.fuzz_rows(rng, N_FUZZ // 2, multi=False), lm.fuzz_rows(rng, N_FUZZ // 2, multi=True), lm.fuzz_rows(rng, 200, alphabet=(1, 2, 97))


SINGLE, MULTI, PREFIX_ROWS = _fuzz()
FUZZ = (SINGLE, MULTI)
GOOD = {id(rows): rows.model() for rows in (*FUZZ, PREFIX_ROWS)}  # (computed once, left unchanged)


def test_the_alphabet_is_the_separators_and_two_letters():
    assert TOKENIZER.sep_token_id == 2 == lm.PIECES[1][0] == lm.PIECES[2][0] and TOKENIZER.cls_token_id == 1 == lm.PIECES[0][0]
    assert lm.ALPHABET == (2, 97, 98)
    for rows in FUZZ:
        assert set(rows.corpus.tolist()) | set(rows.query_ids.tolist()) == set(lm.ALPHABET)
        assert {len(q) for q in rows.queries} == set(range(0, 9))
        assert {len(rows.context(first, n, clip)) for _q, first, n, clip in rows.plan} == set(range(1, 7))
    assert (MULTI.plan_np[:, 2] > 1).any() and (MULTI.plan_np[:, 3] > 0).any() and any(MULTI.frag_shift)
    assert (SINGLE.plan_np[:, 2] == 1).all() and not (SINGLE.plan_np[:, 3] > 0).any()


@pytest.mark.parametrize("rows", [SINGLE, MULTI, PREFIX_ROWS], ids=["single", "multi", "prefix"])
def test_the_restatement_is_the_host_path(rows):
    ids, starts, means = rows.host(TOKENIZER)
    assert np.array_equal(ids, rows.ids)  # (the rows restated in lookup_model.Rows are the tokenizer's)
    ctx_start, got_means, slot_frag = GOOD[id(rows)]
    assert np.array_equal(ctx_start, starts)
    assert np.array_equal(lm.bits(got_means), lm.bits(means))
    assert slot_frag.tolist() == [f for _q, first, n, _c in rows.plan for f in range(first, first + n)]


def test_the_fuzz_covers_what_it_is_for():
    """Asserted, so that the fuzz cannot quietly stop covering the case.  On the host path alone: the shares are
    ``prepare_block_inputs``'s, not the restatement's."""

    left = overlap = at_head = 0
    for rows in FUZZ:
        starts = rows.host(TOKENIZER)[1]
        for i, (_q, first, n, clip) in enumerate(rows.plan):
            head_len, n_ctx = rows.head_len(i), len(rows.context(first, n, clip))
            left += starts[i] < head_len
            overlap += starts[i] < head_len < starts[i] + n_ctx
            at_head += starts[i] == head_len
    print(f"start < head_len: {left / N_FUZZ:.3f}, overlapping the context's own copy: {overlap / N_FUZZ:.3f}, at head_len: {at_head / N_FUZZ:.3f}")
    assert left >= 0.15 * N_FUZZ and overlap >= 0.01 * N_FUZZ and at_head >= 0.50 * N_FUZZ
    assert left + at_head == N_FUZZ
    # the supplement: a context found at the prefix itself
    starts = PREFIX_ROWS.host(TOKENIZER)[1]
    assert (starts == 0).any()


@pytest.mark.parametrize("mutate", lm.MUTATIONS)
def test_every_mutation_changes_a_result(mutate):
    changed = 0
    for rows in (*FUZZ, PREFIX_ROWS) if mutate == "after_prefix" else FUZZ:
        good, bad = GOOD[id(rows)], rows.model(mutate=mutate)
        changed += (not np.array_equal(good[0], bad[0])) or (not np.array_equal(lm.bits(good[1]), lm.bits(bad[1])))
    assert changed, mutate


def test_start_unused_finds_the_place_and_ignores_it():
    good, bad = GOOD[id(MULTI)], MULTI.model(mutate="start_unused")
    assert np.array_equal(good[0], bad[0]) and not np.array_equal(lm.bits(good[1]), lm.bits(bad[1]))


@pytest.mark.parametrize("question, context, want", [
    ("Is Paris nice", "Paris", 4),
    ("xab", "ab\x02ab\x02ab", 2),  # the match runs into the context's own copy
    ("aaaa", "aaaaaaaa", 6),        # the place by lengths
])
def test_named_cases(question, context, want):
    query = pl.tokenize_query(TOKENIZER, question)
    fragment = pl.FragmentRecord(context, 0, 0, 0, len(context), TOKENIZER.encode(context))
    ids, _mask, _types, ranges = pl.prepare_block_inputs(TOKENIZER, query, [fragment])
    assert ranges[0][0] == want
    rows = lm.text_rows(TOKENIZER, [(question, context)])
    assert rows.ids.tolist() == ids
    ctx_start, means, _slot_frag = rows.model()
    assert ctx_start.tolist() == [want]
    assert means[0] == np.float32(pl.mean_f32_slice(rows.keep_prob[want: want + len(context)]))


def test_rows_without_context_get_head_len_and_no_slots():
    rows = lm.Rows([[97, 98]], [[97], []], [(0, 0, 0, 0), (1, 0, 1, 0), (0, 0, 0, 0)], slot_base=2)
    ctx_start, means, slot_frag = rows.model(fill=(-7.5, -9))
    assert ctx_start.tolist() == [3, 2, 3]
    assert means[:2].tolist() == [-7.5, -7.5] and slot_frag.tolist() == [-9, -9, 0] and rows.n_slots == 3


# -- header and binding ----------------------------------------------------------------------------------------------------------------
def test_the_call_is_declared_and_bound(hip_library):
    text = (ROOT / "include" / "open_provence_hip.h").read_text()
    header = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert re.search(r"#define OP_ABI_VERSION 10\b", text) and _lib.OP_ABI_VERSION == 10 == hip_library.op_abi_version()
    name = "op_located_fragment_means"
    assert name in _lib.EXPORTED_SYMBOLS and re.search(rf"\bint {name}\s*\(", header) and hasattr(hip_library, name)
    argtypes = hip_library.op_located_fragment_means.argtypes
    assert len(argtypes) == 6 and argtypes[1] is ctypes.POINTER(_lib.OpAssembleRequest) and argtypes[2] is ctypes.POINTER(_lib.OpPlannedMeansRequest)
    # neither struct changed
    assert ctypes.sizeof(_lib.OpPlannedMeansRequest) == 8 + 6 * 8
    # refused before the handle is looked at: NULL requests with a NULL handle are OP_ERR_INVALID, not a crash
    assert hip_library.op_located_fragment_means(None, None, None, None, None, None) == _lib.OP_ERR_INVALID


# -- the host check (csrc/op_plan.h) under a host sanitizer --------------------------------------------------------------------------
SOURCE = ROOT / "tests" / "host" / "locate_check.cpp"
SANITIZE = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]


def test_every_refusal_of_the_host_check(tmp_path):
    """tests/host/locate_check.cpp has a main of its own and no HIP: it builds a well-formed request, breaks it one field at a
    time and prints ``label code message`` per attempt; compiled with the host C++ compiler under AddressSanitizer and UBSan (a
    plain build where the sanitized link fails, as tests/test_decision_model.py does)."""

    compilers = [c for c in (shutil.which("c++"), shutil.which("g++"), "/opt/rocm/llvm/bin/clang++") if c and Path(c).exists()]
    assert compilers, "no host C++ compiler"
    exe, done, errors = tmp_path / "locate_check", None, []
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
    assert done is not None, "locate_check.cpp does not build or run:\n" + "\n".join(errors)
    lines = [line.split(" ", 2) for line in done.stdout.splitlines()]
    seen = {label: (int(code), message) for label, code, message in lines}
    assert len(seen) == len(lines)
    for label in ("well_formed", "no_rows", "no_rows_null_buffers"):
        assert seen.pop(label) == (0, "-"), label
    expected = {  # label -> a word of the refusal
        "null_ids": "ids_dev is NULL", "null_ctx_start_out": "ctx_start_out_dev is NULL", "null_both": "NULL",
        "null_rows": "rows is NULL", "null_request": "request is NULL", "rows_struct_bytes": "op_assemble_request.struct_bytes",
        "struct_bytes": "op_planned_means_request.struct_bytes", "negative_rows": "negative count", "negative_slots": "negative count",
        "negative_total": "negative count", "negative_frag": "negative count", "negative_queries": "negative count",
        "long_prefix": "template piece", "negative_middle": "template piece",
        "null_plan_host": "NULL", "null_plan_dev": "NULL", "null_cu_host": "NULL", "null_cu_dev": "NULL", "null_frag_off_host": "NULL",
        "null_frag_off_dev": "NULL", "null_q_off_host": "NULL", "null_q_off_dev": "NULL", "null_slot_off_host": "NULL", "null_slot_off_dev": "NULL",
        "null_frag_shift": "NULL", "null_keep_prob": "keep_prob_dev is NULL", "null_mean_out": "mean_out_dev or slot_frag_out_dev",
        "null_slot_frag_out": "mean_out_dev or slot_frag_out_dev", "query_outside": "names query 2", "negative_query": "names query -1",
        "fragments_past_the_corpus": "takes fragments", "negative_first_fragment": "takes fragments",
        "negative_fragment_count": "takes fragments", "clip_beyond_the_fragment": "clips its first fragment",
        "negative_clip": "clips its first fragment", "frag_off_decreases": "frag_off decreases", "q_off_decreases": "q_off decreases",
        "offsets_from_1": "do not start at 0", "cu_start": "cu_seqlens_host runs from 1", "cu_end": "cu_seqlens_host runs from 0 to",
        "cu_decreases": "cu_seqlens_host decreases at row 1", "slot_off_negative": "slot_off_host[0] is -1",
        "slot_off_not_prefix_sums": "slot_off_host[2]", "slot_off_past_the_outputs": "of 5 slots",
    }
    assert set(seen) == set(expected)
    for label, word in expected.items():
        code, message = seen[label]
        assert code == _lib.OP_ERR_INVALID and word in message and message.startswith("op_located_fragment_means:"), (label, code, message)
