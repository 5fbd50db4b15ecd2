"""A Python restatement of ``op_planned_fragment_means`` and ``op_sentence_decisions`` (csrc/opk_decide.hip.h) and of the
corpus tables behind them (``PreparedContexts.decision_tables``), with the mistakes code of this kind can make as ``mutate=``
switches, and the synthetic corpora both test modules run them on (test infrastructure, not product code).

The arguments are the C calls': flat int32 tables, ``plan`` rows ``(query, first_frag, n_frag, clip)``, ``cu`` (row offsets into
``keep_prob``), ``slot_off`` (prefix sums of ``n_frag``), instances ``(slot_begin, slot_end, sent_out_begin, n_sentences,
item_sent_base, title_index)``.  Sums are numpy's pairwise sums written out element by element (``pairwise_sum``)."""

from __future__ import annotations

from dataclasses import dataclass, field

import numpy as np

from open_provence_amd import pipeline as pl
from open_provence_amd.pipeline import FragmentRecord

MUTATIONS = ("no_shift", "shift_uncapped", "end_unclamped", "sequential_f64", "ge_threshold", "nan_kept", "title_forced")
N_PREFIX, N_MIDDLE, N_SUFFIX = 1, 1, 1  # [CLS] q [SEP] ctx [SEP]
PIECES = ([1], [2], [2])


# -- numpy's pairwise sum, one scalar addition at a time ---------------------------------------------------------------------------
def _leaf(a, zero):
    n = len(a)
    if n < 8:
        res = zero
        for x in a:
            res = res + x
        return res
    r = [a[j] for j in range(8)]
    i = 8
    while i < n - n % 8:
        for j in range(8):
            r[j] = r[j] + a[i + j]
        i += 8
    res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]))
    while i < n:
        res = res + a[i]
        i += 1
    return res


def pairwise_sum(values: np.ndarray):
    """``np.add.reduce(values)`` for a 1-D float32 / float64 array, as scalar additions of that type in numpy's order."""

    def rec(a):
        n = len(a)
        if n <= 128:
            return _leaf(a, values.dtype.type(0))
        n2 = n // 2
        n2 -= n2 % 8
        return rec(a[:n2]) + rec(a[n2:])

    with np.errstate(all="ignore"):
        return rec(values)


# -- the two kernels -------------------------------------------------------------------------------------------------------------------
def planned_fragment_means(keep_prob, cu, plan, frag_off, frag_shift, q_off, slot_off, n_slots, *, mutate: str | None = None, fill=None):
    """-> (mean[n_slots] float32, slot_frag[n_slots] int32); slots no row names keep ``fill`` (a (float, int) pair)."""

    assert mutate is None or mutate in MUTATIONS, mutate
    means = np.full(n_slots, np.float32(0 if fill is None else fill[0]), dtype=np.float32)
    slot_frag = np.full(n_slots, 0 if fill is None else fill[1], dtype=np.int32)
    for i, (query, first, n, clip) in enumerate(plan):
        lo, hi = int(cu[i]), int(cu[i + 1])
        cursor = N_PREFIX + int(q_off[query + 1]) - int(q_off[query]) + N_MIDDLE
        for j in range(n):
            f = first + j
            length = clip if (j == 0 and clip > 0) else int(frag_off[f + 1]) - int(frag_off[f])
            start, end = cursor, cursor + length
            cursor = end
            if mutate != "no_shift":
                start, end = start - int(frag_shift[f]), end - int(frag_shift[f])
            start = max(start, 0)
            if mutate != "end_unclamped":
                end = min(end, hi - lo)
            if end <= start:
                value = np.float32(1.0)
            else:
                part = keep_prob[lo + start: lo + end]
                with np.errstate(all="ignore"):
                    value = np.float32(np.float64(pairwise_sum(part)) / np.float64(len(part)))
            means[int(slot_off[i]) + j] = value
            slot_frag[int(slot_off[i]) + j] = f
    return means, slot_frag


def sentence_decisions(instances, means, slot_frag, frag_sent, threshold: float, n_out: int, *, mutate: str | None = None):
    """-> (avg[n_out] float64, keep[n_out] uint8)."""

    assert mutate is None or mutate in MUTATIONS, mutate
    avg_out = np.zeros(n_out, dtype=np.float64)
    keep_out = np.zeros(n_out, dtype=np.uint8)
    for slot_begin, slot_end, out_begin, n_sent, sent_base, title in instances:
        slot = slot_begin
        any_kept = False
        for k in range(n_sent):
            want = sent_base + k
            while slot < slot_end and int(frag_sent[slot_frag[slot]]) < want:
                slot += 1
            run = slot
            while slot < slot_end and int(frag_sent[slot_frag[slot]]) == want:
                slot += 1
            values = means[run:slot].astype(np.float64)
            if len(values) == 0:
                avg = 0.0
            elif len(values) == 1:
                avg = float(values[0])
            elif mutate == "sequential_f64":
                total = np.float64(0)
                for v in values:
                    total = total + v
                avg = float(total / np.float64(len(values)))
            else:
                with np.errstate(all="ignore"):
                    avg = float(pairwise_sum(values) / np.float64(len(values)))
            if mutate == "nan_kept" and avg != avg:
                clamped = avg
            else:
                capped = 1.0 if 1.0 < avg else avg
                clamped = capped if capped > 0.0 else 0.0
            keep = clamped >= threshold if mutate == "ge_threshold" else clamped > threshold
            any_kept = any_kept or keep
            avg_out[out_begin + k] = clamped
            keep_out[out_begin + k] = 1 if keep else 0
        if title >= 0 and (any_kept or mutate == "title_forced"):
            keep_out[out_begin + title] = 1
    return avg_out, keep_out


# -- synthetic corpora and requests ---------------------------------------------------------------------------------------------------
@dataclass
class Item:
    """One context: what ``PreparedItem`` keeps (same attribute names), built without a tokenizer."""

    entry: str
    context_text: str
    sentences: list[str]
    prefix_sentences: list[str]
    prefix_token_counts: list[int]
    title_is_first_sentence: bool
    fragments: list[FragmentRecord]
    frag_base: int = 0


def make_item(rng, name: str, n_prefix: int, fragments_per_sentence, token_lengths, *, title_first: bool = False, counts=None) -> Item:
    """``fragments_per_sentence[k]`` fragments for sentence ``k`` (0: a sentence without fragments), their token counts drawn
    from ``token_lengths`` in turn; ``counts``: the prefix token counts, by default the tokens of the prefix sentences."""

    sentences = [f"{name} sentence {k}. " for k in range(len(fragments_per_sentence))]
    fragments, at = [], 0
    for k, n in enumerate(fragments_per_sentence):
        for j in range(n):
            length = int(token_lengths[at % len(token_lengths)])
            fragments.append(FragmentRecord(f"{name}/{k}/{j}", k, j, at, length, [int(t) for t in rng.integers(10, 400, length)]))
            at += 1
    if counts is None:
        counts = [sum(f.token_length for f in fragments if f.sentence_index == k) for k in range(n_prefix)]
    return Item(name, "".join(sentences[n_prefix:]), sentences, sentences[:n_prefix], list(counts), title_first, fragments)


@dataclass
class Case:
    """A corpus, a request over it, and the keep-probabilities of its rows.  ``instances[i] = (query, item, blocks)`` with
    ``blocks`` = ``[(n_frag, clip), ...]`` consecutive over the item's fragments.  ``row_cut``: tokens taken off the END of
    given rows (a row shorter than its plan says: what the end clamp is for)."""

    items: list[Item]
    queries: list[list[int]]
    instances: list[tuple[int, int, list[tuple[int, int]]]]
    seed: int = 0
    nan_rows: tuple = ()
    row_cut: dict = field(default_factory=dict)
    wide_range: bool = False

    def __post_init__(self) -> None:
        base = 0
        for item in self.items:
            item.frag_base = base
            base += len(item.fragments)
        self.n_frag = base
        self.frag_off = np.concatenate(([0], np.cumsum([f.token_length for it in self.items for f in it.fragments]))).astype(np.int32)
        self.q_off = np.concatenate(([0], np.cumsum([len(q) for q in self.queries]))).astype(np.int32)
        plan, lengths, self.blocks = [], [], []
        for query, at, blocks in self.instances:
            item, first = self.items[at], 0
            assert sum(n for n, _ in blocks) == len(item.fragments)
            for n, clip in blocks:
                block = list(item.fragments[first: first + n])
                if clip > 0:
                    f = block[0]
                    assert clip < f.token_length
                    block[0] = FragmentRecord(f.text, f.sentence_index, f.fragment_index, f.global_index, clip, f.token_ids[:clip])
                plan.append((query, item.frag_base + first, n, clip))
                self.blocks.append(block)
                lengths.append(N_PREFIX + len(self.queries[query]) + N_MIDDLE + sum(f.token_length for f in block) + N_SUFFIX
                               - self.row_cut.get(len(lengths), 0))
                first += n
        self.plan = np.array(plan, dtype=np.int32).reshape(-1, 4)
        self.cu = np.concatenate(([0], np.cumsum(lengths))).astype(np.int32)
        self.slot_off = np.concatenate(([0], np.cumsum(self.plan[:, 2]))).astype(np.int32)
        self.n_slots = int(self.slot_off[-1])
        rng = np.random.default_rng(self.seed)
        self.keep_prob = rng.random(int(self.cu[-1]), dtype=np.float32)
        if self.wide_range:
            # fp32 means between 2^-45 and 1: their float64 sum is then not exact, so its ORDER shows (the sum of a few fp32
            # values of like magnitude is exact in float64 in any order)
            self.keep_prob *= np.exp2(-rng.integers(0, 46, self.keep_prob.size)).astype(np.float32)
        for row in self.nan_rows:
            self.keep_prob[self.cu[row]: self.cu[row + 1]] = np.nan

    # -- the tables, restated ------------------------------------------------------------------------------------------------------
    def tables(self, *, mutate: str | None = None):
        """-> (frag_shift, frag_sent, sent_base[n_items + 1], frag_first_id), from the definitions."""

        frag_shift, frag_sent, first_id, sent_base = [], [], [], [0]
        for item in self.items:
            counts = item.prefix_token_counts
            for f in item.fragments:
                k = f.sentence_index
                shift = 0 if k == 0 else sum(counts[: min(k, len(counts))])
                if mutate == "shift_uncapped" and counts and k > len(counts):  # (as if every sentence before k were a title)
                    shift += (k - len(counts)) * counts[-1]
                frag_shift.append(shift)
                frag_sent.append(sent_base[-1] + k)
                first_id.append(f.token_ids[0] if f.token_ids else -1)
            sent_base.append(sent_base[-1] + len(item.sentences))
        return (np.array(frag_shift, dtype=np.int32), np.array(frag_sent, dtype=np.int32), np.array(sent_base, dtype=np.int32),
                np.array(first_id, dtype=np.int32))

    def instance_table(self, always_select_title: bool) -> tuple[np.ndarray, int]:
        """-> (instances [n, 6] int32, n_out)."""

        sent_base = self.tables()[2]
        rows, slot, out = [], 0, 0
        for _query, at, blocks in self.instances:
            item = self.items[at]
            n_slots = sum(n for n, _ in blocks)
            title = -1
            if always_select_title and item.sentences and (item.prefix_sentences or item.title_is_first_sentence):
                title = 0
            rows.append((slot, slot + n_slots, out, len(item.sentences), int(sent_base[at]), title))
            slot += n_slots
            out += len(item.sentences)
        return np.array(rows, dtype=np.int32).reshape(-1, 6), out

    # -- the product's host path on the same request ---------------------------------------------------------------------------------
    def host_means(self) -> np.ndarray:
        """``pl.fragment_token_ranges`` + ``pl.mean_f32_slice`` per fragment, in slot order."""

        out, row = [], 0
        for query, at, blocks in self.instances:
            state = self._state(at, [])
            for _ in blocks:
                block = self.blocks[row]
                lo, hi = int(self.cu[row]), int(self.cu[row + 1])
                cursor, ranges = N_PREFIX + len(self.queries[query]) + N_MIDDLE, []
                for f in block:
                    ranges.append((cursor, cursor + f.token_length))
                    cursor += f.token_length
                probs = self.keep_prob[lo:hi]
                for start, end in pl.fragment_token_ranges(state, block, ranges, hi - lo):
                    with np.errstate(all="ignore"):
                        out.append(1.0 if end <= start else pl.mean_f32_slice(probs[start:end]))
                row += 1
        return np.array(out, dtype=np.float32)

    def _state(self, at: int, blocks) -> pl.ContextState:
        item = self.items[at]
        return pl.ContextState(list(item.sentences), item.fragments, blocks, len(item.prefix_sentences), item.prefix_sentences,
                               item.prefix_token_counts, item.title_is_first_sentence, item.context_text)

    def host_result(self, means: np.ndarray, scores, **options) -> pl.PostprocessResult:
        """``pl.postprocess_contexts`` over states that hold ``means`` as the device-reduced fragment means of their blocks
        (one query per instance list position: instance ``i`` is context ``i`` of query 0)."""

        states, row = {}, 0
        for c_idx, (_query, at, blocks) in enumerate(self.instances):
            state = self._state(at, [self.blocks[row + b] for b in range(len(blocks))])
            for b_idx in range(len(blocks)):
                lo, hi = int(self.slot_off[row]), int(self.slot_off[row + 1])
                state.raw_blocks.append((b_idx, pl.RawPrediction("", [], scores[row], np.zeros(0, dtype=np.float32), [],
                                                                 fragment_means=means[lo:hi].tolist())))
                row += 1
            states[(0, c_idx)] = state
        contexts = [[self.items[at].entry for _q, at, _b in self.instances]]
        return pl.postprocess_contexts([""], contexts, states, **options)


def boundary_case(rng) -> Case:
    """Sentences of 1, 2, 8, 9, 129 and 130 fragments and fragments of 1, 7, 8, 9, 127, 128 and 129 tokens (numpy's pairwise
    boundaries), titles whose shift is not 0 and sentence indices beyond the prefix counts, a clipped first fragment, contexts of
    several blocks, a sentence without fragments, a range shifted to empty, a title that is the first sentence."""

    lengths = [1, 7, 8, 9, 127, 128, 129]
    items = [
        make_item(rng, "plain", 0, [1, 2, 8, 9], lengths),
        make_item(rng, "titled", 1, [1, 3, 0, 2, 9], [5, 3, 9, 1, 8, 7]),                      # shift 5 from sentence 1 on, k up to 4 > len(counts)
        make_item(rng, "two titles", 2, [1, 1, 2, 130], [4, 6, 2, 3, 1]),                      # shifts 4, then 10
        make_item(rng, "long", 0, [129, 1, 2], [3, 1, 2]),
        make_item(rng, "shifted away", 1, [1, 1, 1], [2, 3, 2], counts=[40]),                  # a shift beyond the row's head: empty ranges
        make_item(rng, "first is title", 0, [1, 2, 1], [6, 2, 9, 4], title_first=True),
        make_item(rng, "wide", 0, [1, 1], [129, 128]),
    ]
    queries = [[int(t) for t in rng.integers(10, 400, n)] for n in (5, 0, 17)]
    instances = [
        (0, 0, [(20, 0)]),
        (0, 1, [(4, 0), (5, 2), (6, 0)]),            # several blocks, the second one clipped to 2 of its 8 tokens
        (2, 2, [(60, 0), (74, 0)]),
        (1, 3, [(132, 0)]),
        (0, 4, [(3, 0)]),
        (2, 5, [(1, 3), (3, 0)]),                    # clipped first block
        (1, 6, [(1, 100), (1, 0)]),
        (2, 1, [(15, 0)]),                           # the same item again, for another query
    ]
    return Case(items, queries, instances, seed=17, wide_range=True)


def nan_case(rng) -> Case:
    """Rows whose keep-probabilities are NaN (every mean of those rows is), beside finite ones."""

    items = [make_item(rng, "a", 1, [1, 2, 2], [3, 4, 2]), make_item(rng, "b", 0, [2, 1], [5, 1, 2], title_first=True)]
    return Case(items, [[11, 12, 13]], [(0, 0, [(2, 0), (3, 0)]), (0, 1, [(3, 0)]), (0, 0, [(5, 0)])], seed=3, nan_rows=(1, 2))


def cut_case(rng) -> Case:
    """Rows shorter than their plan says (a row before the last one loses its suffix and 4 context tokens)."""

    items = [make_item(rng, "a", 0, [2, 2], [6, 5, 4, 3]), make_item(rng, "b", 1, [1, 2], [2, 7, 3])]
    return Case(items, [[21, 22]], [(0, 0, [(4, 0)]), (0, 1, [(3, 0)])], seed=5, row_cut={0: 5})


def random_case(rng) -> Case:
    items = []
    for i in range(int(rng.integers(2, 6))):
        n_prefix = int(rng.integers(0, 3))
        per_sentence = [int(rng.integers(1, 3)) for _ in range(n_prefix)] + [int(rng.integers(0, 4)) for _ in range(int(rng.integers(1, 6)))]
        if sum(per_sentence) == 0:
            per_sentence[-1] = 1
        items.append(make_item(rng, f"item{i}", n_prefix, per_sentence, rng.integers(1, 12, 16), title_first=bool(rng.integers(0, 2))))
    queries = [[int(t) for t in rng.integers(10, 400, int(rng.integers(0, 9)))] for _ in range(int(rng.integers(1, 3)))]
    instances = []
    for _ in range(int(rng.integers(1, 7))):
        at = int(rng.integers(0, len(items)))
        left, blocks = len(items[at].fragments), []
        while left:
            n = int(rng.integers(1, left + 1))
            first = items[at].fragments[len(items[at].fragments) - left]
            clip = int(rng.integers(1, first.token_length)) if first.token_length > 1 and rng.integers(0, 3) == 0 else 0
            blocks.append((n, clip))
            left -= n
        instances.append((int(rng.integers(0, len(queries))), at, blocks))
    return Case(items, queries, instances, seed=int(rng.integers(0, 1 << 30)))


def bits(values: np.ndarray) -> np.ndarray:
    """float32 -> uint32, float64 -> uint64 views: equality on bits (NaN payloads and signed zeros included)."""

    values = np.ascontiguousarray(values)
    return values.view({4: np.uint32, 8: np.uint64}[values.dtype.itemsize]) if values.dtype.kind == "f" else values
