"""A Python restatement of ``op_assemble_rows`` (csrc/opk_assemble.hip.h): plan + template -> packed ids, with the
mistakes a kernel of this kind can make as ``mutate=`` switches (test infrastructure, not product code).

The arguments are the C call's: ``corpus`` / ``frag_off`` (the fragments' ids end to end and their offsets), ``query_ids`` /
``q_off``, ``pieces`` = (prefix, middle, suffix), ``plan`` rows ``(query, first_frag, n_frag, clip)`` -- ``n_frag = 0``: no context,
with ``clip = -1`` no suffix either -- and ``cu`` (row offsets).
Like the kernel, a row is written inside its own ``[cu[r], cu[r + 1])`` only."""

from __future__ import annotations

import ctypes

import numpy as np

from open_provence_amd import _lib
from open_provence_amd.pipeline import FragmentRecord

BERT_PIECES = ([1], [2], [2])  # [CLS] q [SEP] ctx [SEP]

MUTATIONS = ("clip_off_by_one", "suffix_dropped", "middle_after_context", "tail_from_first_offset", "query_row_shift")


def row_lengths(frag_off, q_off, pieces, plan) -> list[int]:
    fixed = sum(len(p) for p in pieces)
    out = []
    for query, first, n, clip in plan:
        if n == 0:
            ctx = -len(pieces[2]) if clip == -1 else 0  # (no context and no suffix)
        elif clip > 0:
            ctx = clip + int(frag_off[first + n]) - int(frag_off[first + 1])
        else:
            ctx = int(frag_off[first + n]) - int(frag_off[first])
        out.append(fixed + int(q_off[query + 1]) - int(q_off[query]) + ctx)
    return out


def request_plan(model, prepared, questions, views):
    """What a prepared request hands to the C call, built from the product's own pieces (``PreparedContexts.flat_tokens``,
    ``PreparedItem.blocks_for``, the template): ``(corpus, frag_off, query_ids, q_off, pieces, plan, blocks)`` with ``blocks[r]``
    = ``(query token ids, the block's FragmentRecords)`` of plan row ``r``."""

    corpus, frag_off = prepared.flat_tokens()
    template = prepared.template
    pieces = (template.prefix, template.middle, template.suffix)
    queries = [[int(t) for t in model.tokenizer.encode(q, add_special_tokens=False)] for q in questions]
    q_off = np.concatenate(([0], np.cumsum([len(q) for q in queries]))).astype(np.int32)
    query_ids = np.array([t for q in queries for t in q], dtype=np.int32)
    sep_len = len(model.tokenizer.encode(model.tokenizer.sep_token or "", add_special_tokens=False))
    plan, blocks = [], []
    for q_idx, view in enumerate(views):
        for at in view.indices:
            item = prepared.items[at]
            item_blocks, item_plan = item.blocks_for(model.tokenizer, len(queries[q_idx]), sep_len, model.max_length)
            for block, (first, count, clip, ctx) in zip(item_blocks, item_plan):
                if ctx == 0:  # (no context tokens: no fragments, and no suffix where the tokenizer builds none)
                    count, clip = 0, -1 if template.empty_context == "drop" and template.suffix else 0
                plan.append((q_idx, item.frag_base + first, count, clip))
                blocks.append((queries[q_idx], block))
    return corpus, frag_off, query_ids, q_off, pieces, plan, blocks


def assemble_rows(corpus, frag_off, query_ids, q_off, pieces, plan, cu, *, mutate: str | None = None, fill: int = -1) -> np.ndarray:
    assert mutate is None or mutate in MUTATIONS, mutate
    corpus, query_ids = [int(t) for t in corpus], [int(t) for t in query_ids]
    prefix, middle, suffix = ([int(t) for t in p] for p in pieces)
    n_queries = len(q_off) - 1
    out = np.full(int(cu[-1]), fill, dtype=np.int32)
    for r, (query, first, n, clip) in enumerate(plan):
        if mutate == "query_row_shift":
            query = (query + 1) % n_queries
        q = query_ids[int(q_off[query]): int(q_off[query + 1])]
        if n == 0:
            ctx = []
        elif clip > 0:
            kept = clip + (1 if mutate == "clip_off_by_one" else 0)
            a0 = int(frag_off[first])
            tail_len = int(frag_off[first + n]) - int(frag_off[first + 1])
            b0 = a0 + kept if mutate == "tail_from_first_offset" else int(frag_off[first + 1])
            ctx = corpus[a0: a0 + kept] + corpus[b0: b0 + tail_len]
        else:
            ctx = corpus[int(frag_off[first]): int(frag_off[first + n])]
        if mutate == "middle_after_context":
            row = prefix + q + ctx + middle + suffix
        else:
            row = prefix + q + middle + ctx + ([] if mutate == "suffix_dropped" or (n == 0 and clip == -1) else suffix)
        lo, hi = int(cu[r]), int(cu[r + 1])
        row = row[: hi - lo]
        out[lo: lo + len(row)] = row
    return out


# -- a synthetic request, and the ways to break it ----------------------------------------------------------------------------------
def synthetic_case(rng):
    """A corpus of 12 fragments (1 - 9 ids), 3 queries (0, 2 and 5 ids) and a plan that has what the pipeline's own plans
    lack: a clipped first fragment FOLLOWED by further fragments (assemble_blocks fills a clipped block), clips of 1 id.
    The pieces that go with it are ``BERT_PIECES``."""

    lengths = [3, 1, 9, 4, 1, 1, 7, 2, 5, 8, 1, 6]
    frags = [FragmentRecord("", 0, i, i, n, [int(t) for t in rng.integers(10, 400, n)]) for i, n in enumerate(lengths)]
    queries = [[], [401, 402], [403, 404, 405, 406, 407]]
    plan = [(1, 0, 3, 0), (2, 2, 3, 4), (0, 2, 1, 1), (1, 6, 2, 6), (2, 9, 3, 7), (0, 11, 1, 0), (1, 3, 1, 0), (2, 8, 4, 2),
            (1, 5, 0, -1), (0, 12, 0, -1)]  # ... and rows without context that end behind `middle`
    return frags, queries, plan


def flat_arrays(frags, queries):
    frag_off = np.concatenate(([0], np.cumsum([len(f.token_ids) for f in frags]))).astype(np.int32)
    corpus = np.array([t for f in frags for t in f.token_ids], dtype=np.int32)
    q_off = np.concatenate(([0], np.cumsum([len(q) for q in queries]))).astype(np.int32)
    return corpus, frag_off, np.array([t for q in queries for t in q], dtype=np.int32), q_off


FAKE_POINTER = 0x1000  # (stands for a device buffer in calls that end before anything is enqueued: never dereferenced)


def build_request(frags, queries, plan, /, pieces=BERT_PIECES, **overrides):
    corpus, frag_off, query_ids, q_off = flat_arrays(frags, queries)
    plan_np = np.array(plan, dtype=np.int32).reshape(-1, 4)
    lengths = row_lengths(frag_off, q_off, pieces, plan)
    cu = np.concatenate(([0], np.cumsum(lengths))).astype(np.int32)
    keep = {"frag_off": frag_off, "q_off": q_off, "plan": plan_np, "cu": cu, "pieces": [np.array(p, dtype=np.int32) for p in pieces]}
    for key in ("frag_off", "q_off", "plan", "cu"):
        if key in overrides:
            keep[key] = np.ascontiguousarray(overrides.pop(key), dtype=np.int32)
    req = _lib.OpAssembleRequest()
    req.struct_bytes = ctypes.sizeof(_lib.OpAssembleRequest)
    req.n_frag, req.n_queries, req.n_rows, req.total_tokens = len(frags), len(queries), len(plan), int(cu[-1])
    req.n_prefix, req.n_middle, req.n_suffix = (int(p.size) for p in keep["pieces"])
    req.prefix, req.middle, req.suffix = (p.ctypes.data if p.size else None for p in keep["pieces"])
    req.corpus_dev = req.frag_off_dev = req.query_ids_dev = req.q_off_dev = req.plan_dev = req.cu_seqlens_dev = FAKE_POINTER
    req.frag_off_host, req.q_off_host = keep["frag_off"].ctypes.data, keep["q_off"].ctypes.data
    req.plan_host, req.cu_seqlens_host = keep["plan"].ctypes.data, keep["cu"].ctypes.data
    for key, value in overrides.items():
        setattr(req, key, value)
    return req, keep


def refusal_cases():
    """(label, keyword overrides of a well-formed request over ``synthetic_case``, a word of the error text)."""

    frags, queries, plan = synthetic_case(np.random.default_rng(3))
    _, frag_off, _, q_off = flat_arrays(frags, queries)
    lengths = row_lengths(frag_off, q_off, BERT_PIECES, plan)
    cu = np.concatenate(([0], np.cumsum(lengths))).astype(np.int32)

    def changed(array, at, value):
        out = np.array(array, dtype=np.int32)
        out.reshape(-1)[at] = value
        return out

    return [
        ("struct_bytes", dict(struct_bytes=8), "struct_bytes"),
        ("negative rows", dict(n_rows=-1), "negative count"),
        ("negative fragments", dict(n_frag=-2), "negative count"),
        ("negative queries", dict(n_queries=-1), "negative count"),
        ("negative total", dict(total_tokens=-5), "negative count"),
        ("long prefix", dict(n_prefix=9), "prefix holds 9"),
        ("long middle", dict(n_middle=9), "middle holds 9"),
        ("long suffix", dict(n_suffix=100), "suffix holds 100"),
        ("negative piece", dict(n_suffix=-1), "suffix holds -1"),
        ("null piece", dict(prefix=None), "prefix is NULL"),
        ("null plan", dict(plan_dev=None), "NULL"),
        ("null plan host", dict(plan_host=None), "NULL"),
        ("null cu", dict(cu_seqlens_dev=None), "NULL"),
        ("null cu host", dict(cu_seqlens_host=None), "NULL"),
        ("null frag_off", dict(frag_off_dev=None), "NULL"),
        ("null q_off host", dict(q_off_host=None), "NULL"),
        ("null corpus", dict(corpus_dev=None), "corpus_dev is NULL"),
        ("null queries", dict(query_ids_dev=None), "query_ids_dev is NULL"),
        ("cu one short", dict(cu=changed(cu, 3, cu[3] - 1)), "cu_seqlens_host[3]"),
        ("cu last", dict(cu=changed(cu, len(cu) - 1, cu[-1] + 1), total_tokens=int(cu[-1]) + 1), "cu_seqlens_host"),
        ("cu start", dict(cu=changed(cu, 0, 1)), "cu_seqlens_host[0]"),
        ("total", dict(total_tokens=int(cu[-1]) + 4), "total_tokens"),
        ("query out of range", dict(plan=changed(plan, 4 * 2 + 0, 3)), "names query 3"),
        ("negative query", dict(plan=changed(plan, 0, -1)), "names query -1"),
        ("fragments past the corpus", dict(plan=changed(plan, 4 * 5 + 2, 2)), "takes fragments"),
        ("negative first fragment", dict(plan=changed(plan, 4 * 1 + 1, -1)), "takes fragments"),
        ("negative fragment count", dict(plan=changed(plan, 4 * 1 + 2, -3)), "takes fragments"),
        ("clip beyond the fragment", dict(plan=changed(plan, 4 * 1 + 3, 10)), "clips its first fragment"),
        ("negative clip", dict(plan=changed(plan, 4 * 6 + 3, -1)), "clips its first fragment"),
        ("clip without a fragment", dict(plan=changed(changed(plan, 4 * 6 + 2, 0), 4 * 6 + 3, 1)), "no fragment"),
        ("clip -2 without a fragment", dict(plan=changed(plan, 4 * 8 + 3, -2)), "no fragment"),
        ("frag_off decreases", dict(frag_off=changed(frag_off, 3, 2)), "frag_off"),
        ("q_off decreases", dict(q_off=changed(q_off, 2, -1)), "q_off decreases"),
        ("offsets from 1", dict(q_off=changed(q_off, 0, 1)), "do not start at 0"),
    ]
