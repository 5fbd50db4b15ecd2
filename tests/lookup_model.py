"""A Python restatement of ``op_located_fragment_means`` (csrc/opk_decide.hip.h): ``op_planned_fragment_means`` with every
row's context looked up in the assembled row first, as ``pipeline.prepare_block_inputs`` looks it up (``_find_subsequence``) --
with the mistakes a search of this kind can make as ``mutate=`` switches, and the hand-built tables both test modules run it on
(test infrastructure, not product code).

The arguments are the C call's: ``ids`` (the rows end to end, as ``op_assemble_rows`` lays them out), ``keep_prob``, ``cu``,
``plan`` rows ``(query, first_frag, n_frag, clip)``, the corpus' ``frag_off`` / ``frag_shift``, ``q_off``, ``slot_off``.  The
template is decision_model's: ``[CLS] q [SEP] ctx [SEP]`` with ids 1, 2, 2 -- ``tests/helpers.CharTokenizer``'s."""

from __future__ import annotations

from dataclasses import dataclass, field
from types import SimpleNamespace

import numpy as np

from decision_model import N_MIDDLE, N_PREFIX, PIECES, bits, pairwise_sum  # noqa: F401  (bits, PIECES: for the test modules)
from open_provence_amd import pipeline as pl
from open_provence_amd.pipeline import FragmentRecord

MUTATIONS = ("first_id_only", "last_match", "no_overlap", "after_prefix", "unclipped", "start_unused")
ALPHABET = (2, 97, 98)  # the separator and two letters: short queries and contexts over it repeat each other often


def located_fragment_means(ids, keep_prob, cu, plan, frag_off, frag_shift, q_off, slot_off, n_slots, *, mutate: str | None = None, fill=None):
    """-> (ctx_start[n_rows] int32, mean[n_slots] float32, slot_frag[n_slots] int32); slots no row names keep ``fill`` (a
    (float, int) pair).  A row without fragments or without context ids gets ``head_len`` and no slots."""

    assert mutate is None or mutate in MUTATIONS, mutate
    means = np.full(n_slots, np.float32(0 if fill is None else fill[0]), dtype=np.float32)
    slot_frag = np.full(n_slots, 0 if fill is None else fill[1], dtype=np.int32)
    ctx_start = np.zeros(len(plan), dtype=np.int32)
    for i, (query, first, n, clip) in enumerate(plan):
        lo, hi = int(cu[i]), int(cu[i + 1])
        row = [int(t) for t in ids[lo:hi]]
        head_len = N_PREFIX + int(q_off[query + 1]) - int(q_off[query]) + N_MIDDLE
        ctx_start[i] = head_len
        if n <= 0:
            continue
        whole_first = int(frag_off[first + 1]) - int(frag_off[first])
        first_len = clip if clip > 0 else whole_first
        n_ctx = (whole_first if mutate == "unclipped" else first_len) + int(frag_off[first + n]) - int(frag_off[first + 1])
        n_ctx = min(n_ctx, len(row) - head_len)
        if n_ctx <= 0:
            continue
        ctx = row[head_len: head_len + n_ctx]
        candidates = range(N_PREFIX if mutate == "after_prefix" else 0, head_len)
        if mutate == "no_overlap":
            candidates = [idx for idx in candidates if idx + n_ctx <= head_len]
        if mutate == "first_id_only":
            matches = [idx for idx in candidates if row[idx] == ctx[0]]
        else:
            matches = [idx for idx in candidates if row[idx: idx + n_ctx] == ctx]
        matches.append(head_len)
        found = matches[-1] if mutate == "last_match" else matches[0]
        ctx_start[i] = found
        cursor = head_len if mutate == "start_unused" else found
        for j in range(n):
            f = first + j
            length = first_len if j == 0 else int(frag_off[f + 1]) - int(frag_off[f])
            start, end = cursor - int(frag_shift[f]), cursor + length - int(frag_shift[f])
            cursor += length
            start, end = max(start, 0), min(end, hi - lo)
            if end <= start:
                value = np.float32(1.0)
            else:
                part = keep_prob[lo + start: lo + end]
                with np.errstate(all="ignore"):
                    value = np.float32(np.float64(pairwise_sum(part)) / np.float64(len(part)))
            means[int(slot_off[i]) + j] = value
            slot_frag[int(slot_off[i]) + j] = f
    return ctx_start, means, slot_frag


# -- hand-built tables ---------------------------------------------------------------------------------------------------------------
@dataclass
class Rows:
    """A corpus of fragments, queries and a plan of rows over them, with everything both calls take derived from them: the
    offsets, the rows' ids as ``op_assemble_rows`` lays them out (restated here: prefix + query + middle + context + suffix),
    ``cu``, ``slot_off`` (from ``slot_base``) and random keep-probabilities.  ``sentence[f]`` / ``title_tokens``: what the host
    path derives ``frag_shift`` from -- a fragment of sentence k > 0 is shifted by ``title_tokens`` (the tokens of sentence 0
    when that is a title, else 0), per context; ``context_of[f]`` names the context."""

    fragments: list[list[int]]
    queries: list[list[int]]
    plan: list[tuple[int, int, int, int]]
    frag_shift: list[int] | None = None
    slot_base: int = 0
    seed: int = 0
    sentence: list[int] = field(default_factory=list)

    def __post_init__(self) -> None:
        self.n_frag = len(self.fragments)
        if self.frag_shift is None:
            self.frag_shift = [0] * self.n_frag
        self.frag_off = np.concatenate(([0], np.cumsum([len(f) for f in self.fragments]))).astype(np.int32)
        self.q_off = np.concatenate(([0], np.cumsum([len(q) for q in self.queries]))).astype(np.int32)
        self.corpus = np.array([t for f in self.fragments for t in f], dtype=np.int32)
        self.query_ids = np.array([t for q in self.queries for t in q], dtype=np.int32)
        rows = []
        for query, first, n, clip in self.plan:
            rows.append(PIECES[0] + list(self.queries[query]) + PIECES[1] + self.context(first, n, clip) + PIECES[2])
        self.rows = rows
        self.ids = np.array([t for row in rows for t in row], dtype=np.int32)
        self.cu = np.concatenate(([0], np.cumsum([len(row) for row in rows]))).astype(np.int32)
        self.plan_np = np.array(self.plan, dtype=np.int32).reshape(-1, 4)
        self.slot_off = (self.slot_base + np.concatenate(([0], np.cumsum(self.plan_np[:, 2])))).astype(np.int32)
        self.n_slots = int(self.slot_off[-1])
        self.keep_prob = np.random.default_rng(self.seed).random(int(self.cu[-1]), dtype=np.float32)
        self.frag_shift_np = np.array(self.frag_shift, dtype=np.int32)

    def context(self, first: int, n: int, clip: int) -> list[int]:
        ctx: list[int] = []
        for j in range(n):
            ids = self.fragments[first + j]
            ctx += ids[:clip] if (j == 0 and clip > 0) else ids
        return ctx

    def head_len(self, row: int) -> int:
        return N_PREFIX + len(self.queries[self.plan[row][0]]) + N_MIDDLE

    def model(self, *, mutate: str | None = None, fill=None):
        return located_fragment_means(self.ids, self.keep_prob, self.cu, self.plan, self.frag_off, self.frag_shift_np, self.q_off, self.slot_off,
                                      self.n_slots, mutate=mutate, fill=fill)

    # -- the product's host path on the same rows ------------------------------------------------------------------------------------
    def host(self, tokenizer):
        """``pl.prepare_block_inputs`` + ``pl.fragment_token_ranges`` + ``pl.mean_f32_slice`` per row -> (the rows' ids end to
        end, ctx_start per row, the means in slot order).  Needs ``sentence``; the prefix counts follow from ``frag_shift``."""

        ids, starts, means = [], [], []
        for i, (query, first, n, clip) in enumerate(self.plan):
            block = []
            for j in range(n):
                tokens = self.fragments[first + j]
                tokens = tokens[:clip] if (j == 0 and clip > 0) else tokens
                block.append(FragmentRecord(f"f{first + j}", self.sentence[first + j], j, first + j, len(tokens), list(tokens)))
            shifts = sorted({self.frag_shift[first + j] for j in range(n) if self.sentence[first + j] > 0})
            assert len(shifts) <= 1  # (one title per context here)
            state = SimpleNamespace(prefix_token_counts=[shifts[0]] if shifts and shifts[0] else [])
            row_ids, _mask, _types, ranges = pl.prepare_block_inputs(tokenizer, self.queries[query], block)
            lo, hi = int(self.cu[i]), int(self.cu[i + 1])
            assert len(row_ids) == hi - lo
            ids += row_ids
            starts.append(ranges[0][0])
            probs = self.keep_prob[lo:hi]
            for start, end in pl.fragment_token_ranges(state, block, ranges, hi - lo):
                with np.errstate(all="ignore"):
                    means.append(1.0 if end <= start else pl.mean_f32_slice(probs[start:end]))
        return np.array(ids, dtype=np.int32), np.array(starts, dtype=np.int32), np.array(means, dtype=np.float32)


def fuzz_rows(rng, n_rows: int, *, alphabet=ALPHABET, multi: bool = True) -> Rows:
    """``n_rows`` rows, each over a context of its own: a query of 0-8 ids and a context of 1-6, both drawn from ``alphabet``.
    ``multi``: the context is cut into 1-3 fragments, a third of the first fragments are longer in the corpus than in the row
    (clipped), and in a third of the contexts of several fragments the first one is a title (the others shift left by it)."""

    fragments, queries, plan, frag_shift, sentence = [], [], [], [], []
    for _ in range(n_rows):
        queries.append([int(t) for t in rng.choice(alphabet, int(rng.integers(0, 9)))])
        ctx = [int(t) for t in rng.choice(alphabet, int(rng.integers(1, 7)))]
        k = int(rng.integers(1, min(3, len(ctx)) + 1)) if multi else 1
        cuts = sorted(rng.choice(np.arange(1, len(ctx)), k - 1, replace=False).tolist()) if k > 1 else []
        parts = [ctx[a:b] for a, b in zip([0] + cuts, cuts + [len(ctx)])]
        clip = 0
        if multi and rng.integers(0, 3) == 0:
            clip = len(parts[0])
            parts[0] = parts[0] + [int(t) for t in rng.choice(alphabet, int(rng.integers(1, 4)))]
        titled = multi and k > 1 and rng.integers(0, 3) == 0
        plan.append((len(queries) - 1, len(fragments), k, clip))
        for j, part in enumerate(parts):
            fragments.append(part)
            sentence.append(j)
            frag_shift.append(len(parts[0]) if (titled and j > 0) else 0)
    return Rows(fragments, queries, plan, frag_shift, seed=int(rng.integers(0, 1 << 30)), sentence=sentence)


def text_rows(tokenizer, pairs) -> Rows:
    """(question, context) texts -> single-fragment rows, one per pair."""

    fragments = [tokenizer.encode(context) for _question, context in pairs]
    queries = [tokenizer.encode(question) for question, _context in pairs]
    return Rows(fragments, queries, [(i, i, 1, 0) for i in range(len(pairs))], sentence=[0] * len(pairs))
