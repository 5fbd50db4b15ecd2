"""Prepared contexts: the query-independent half of ``process()`` done once for a corpus.

``OpenProvenceModel.prepare_contexts`` splits, tokenises and fragmentises every context a single time and keeps, per
context, exactly what ``process()`` puts into a job.  A request then names contexts by index (``select``) and the host is
left with the query's tokens and length arithmetic: which fragments share a block, how long each row is, which forward a
row goes into.  On the native forward the rows themselves are laid out on the device (``op_assemble_rows``) from the
fragments' token ids, which are uploaded once.  Nothing here touches a device: the model does (``modeling.py``).
"""

from __future__ import annotations

from typing import Any, Sequence

import numpy as np

from . import pipeline as pl
from .pipeline import FragmentRecord

MAX_TEMPLATE_PIECE = 8  # = OP_ASSEMBLE_MAX_PIECE: ids per piece of the row template


class RowTemplate:
    """``prefix + query + middle + context + suffix``: the specials layout of a row, each piece a short id list.
    ``empty_context``: what a row WITHOUT context tokens (an empty context's fallback sentence) looks like -- ``"keep"``: the
    template with nothing between middle and suffix; ``"drop"``: ``prefix + query + middle``, what BERT-style tokenizers and
    the manual-specials path build for an empty second sequence; None: neither (such rows are built on the host)."""

    __slots__ = ("prefix", "middle", "suffix", "empty_context")

    def __init__(self, prefix: Sequence[int], middle: Sequence[int], suffix: Sequence[int], empty_context: str | None = "keep") -> None:
        self.prefix, self.middle, self.suffix = [int(t) for t in prefix], [int(t) for t in middle], [int(t) for t in suffix]
        self.empty_context = empty_context

    def row(self, query: Sequence[int], ctx: Sequence[int]) -> list[int]:
        if not ctx and self.empty_context == "drop":
            return self.prefix + list(query) + self.middle
        return self.prefix + list(query) + self.middle + list(ctx) + self.suffix

    def __repr__(self) -> str:
        return f"RowTemplate(prefix={self.prefix}, middle={self.middle}, suffix={self.suffix}, empty_context={self.empty_context!r})"


def derive_row_template(build_row) -> RowTemplate | None:
    """The template behind ``build_row(query_ids, ctx_ids) -> input_ids`` (``pipeline.prepare_block_inputs`` with the
    model's settings), from two probe pairs of different lengths; None when the rows do not fit one -- the ids of a probe
    missing from its row or found twice, pieces that differ between the probes or are longer than 8 ids, or an empty
    query that is laid out differently.  Probe ids only ever pass through list concatenation: they index nothing."""

    probes = [([1000003, 1000033], [1000037]), ([1000039], [1000081, 1000099, 1000117])]
    found = []
    for query, ctx in probes:
        try:
            ids = [int(t) for t in build_row(query, ctx)]
        except Exception:
            return None
        q_at, c_at = pl._find_subsequence(ids, query), pl._find_subsequence(ids, ctx)
        if q_at < 0 or c_at < q_at + len(query) or sum(ids.count(t) for t in query + ctx) != len(query) + len(ctx):
            return None
        found.append((ids[:q_at], ids[q_at + len(query): c_at], ids[c_at + len(ctx):]))
    if found[0] != found[1] or any(len(piece) > MAX_TEMPLATE_PIECE for piece in found[0]):
        return None
    template = RowTemplate(*found[0])
    try:
        if [int(t) for t in build_row([], probes[1][1])] != template.row([], probes[1][1]):
            return None
        empty = [[int(t) for t in build_row(query, [])] for query in (probes[0][0], [])]
    except Exception:
        return None
    for mode in ("keep", "drop"):
        template.empty_context = mode
        if all(row == template.row(query, []) for row, query in zip(empty, (probes[0][0], []))):
            return template
    template.empty_context = None
    return template


class PreparedItem:
    """One context of a prepared corpus: what ``process()`` keeps in a job, its fragments, and where they start in the
    corpus' flat fragment numbering.  ``blocks_for`` caches the block plan per (query + separator) length."""

    __slots__ = ("entry", "context_text", "sentences", "prefix_sentences", "prefix_token_counts", "title_is_first_sentence",
                 "fragments", "frag_base", "_plans")

    def __init__(self, entry, job: dict[str, Any], frag_base: int) -> None:
        self.entry = entry
        self.context_text = job["context_text"]
        self.sentences = job["sentences"]
        self.prefix_sentences = job["prefix_sentences"]
        self.prefix_token_counts = job["prefix_token_counts"]
        self.title_is_first_sentence = job["title_is_first_sentence"]
        self.fragments: list[FragmentRecord] = job["fragments"]
        self.frag_base = int(frag_base)
        self._plans: dict[int, tuple] = {}

    def blocks_for(self, tokenizer, query_len: int, sep_len: int, max_length: int):
        """``(blocks, plan)``: ``pipeline.assemble_blocks`` over the cached fragments, and per block ``(first fragment within
        the context, fragments, clip, context tokens)`` -- ``clip`` = the tokens kept of a first fragment that was cut
        because it does not fit beside the query, 0 otherwise.  Blocks take consecutive fragments in order."""

        base = int(query_len) + int(sep_len)
        cached = self._plans.get(base)
        if cached is None:
            blocks = pl.assemble_blocks(tokenizer, self.fragments, query_len, sep_len, max_length)
            plan, first = [], 0
            for block in blocks:
                clipped = block[0] is not self.fragments[first]
                plan.append((first, len(block), len(block[0].token_ids) if clipped else 0, sum(len(f.token_ids) for f in block)))
                first += len(block)
            cached = self._plans[base] = (blocks, plan)
        return cached


class PreparedView:
    """Some contexts of a :class:`PreparedContexts`, in the caller's order, repeats allowed: what one question is scored
    against.  Holds indices only."""

    __slots__ = ("corpus", "indices")

    def __init__(self, corpus: "PreparedContexts", indices: Sequence[int]) -> None:
        n = len(corpus.items)
        out = []
        for i in indices:
            j = int(i)
            if not -n <= j < n:
                raise IndexError(f"context index {j} is outside a prepared corpus of {n} contexts")
            out.append(j % n if n else j)
        self.corpus, self.indices = corpus, out

    def __len__(self) -> int:
        return len(self.indices)

    def select(self, indices: Sequence[int]) -> "PreparedView":
        return PreparedView(self.corpus, [self.indices[int(i)] for i in indices])


class PreparedContexts:
    """A corpus prepared once by ``OpenProvenceModel.prepare_contexts``; ``process(question, prepared)`` scores it, or a
    ``select(indices)`` view of it, as ``process(question, [the raw contexts])`` would.

    It records what it was made with -- the model instance, its tokenizer, ``max_length`` and specials settings, the title
    mode, ``strip_sentences``, ``respect_sentence_boundaries``, the splitter arguments -- and ``process()`` refuses
    (``ValueError``) a request that disagrees.  ``timing`` holds the one-off stage seconds of the preparation."""

    def __init__(self, model, items: list[PreparedItem], settings: dict[str, Any], template: RowTemplate | None,
                 timing: dict[str, float]) -> None:
        self.model = model
        self.tokenizer = model.tokenizer
        self.max_length = int(model.max_length)
        self.items = items
        self.settings = dict(settings)
        self.template = template
        self.timing = dict(timing)
        self.n_fragments = sum(len(item.fragments) for item in items)
        self.n_tokens = sum(len(f.token_ids) for item in items for f in item.fragments)
        self._device: dict[str, Any] | None = None  # the resident corpus, uploaded on first use with the native forward
        self._decision_tables: "dict[str, np.ndarray] | None | bool" = False  # (False: not built yet; see decision_tables)

    def __len__(self) -> int:
        return len(self.items)

    def select(self, indices: Sequence[int]) -> PreparedView:
        return PreparedView(self, indices)

    @property
    def host_assembled(self) -> bool:
        """True when rows are always built on the host: the tokenizer's rows do not fit a template."""

        return self.template is None

    @property
    def device_bytes(self) -> int:
        """Device memory of the resident corpus: 4 bytes per token and per fragment offset."""

        return 4 * (self.n_tokens + self.n_fragments + 1)

    def flat_tokens(self) -> tuple[np.ndarray, np.ndarray]:
        """``(ids[int32, n_tokens], frag_off[int32, n_fragments + 1])``: the fragments' token ids in context order then
        fragment order, and their offsets -- the resident corpus of ``op_assemble_rows``."""

        if self.n_tokens >= 2**31 - 1:
            raise ValueError(f"a prepared corpus holds at most 2^31 - 2 tokens on the device, this one has {self.n_tokens}")
        lengths = np.fromiter((len(f.token_ids) for item in self.items for f in item.fragments), dtype=np.int64, count=self.n_fragments)
        frag_off = np.zeros(self.n_fragments + 1, dtype=np.int32)
        frag_off[1:] = np.cumsum(lengths)
        ids = np.fromiter((t for item in self.items for f in item.fragments for t in f.token_ids), dtype=np.int32, count=self.n_tokens)
        return ids, frag_off

    def decision_tables(self) -> "dict[str, np.ndarray] | None":
        """The per-corpus tables behind the last stages of a request on the device (``op_planned_fragment_means``,
        ``op_sentence_decisions``), built on first use -- or None for a corpus that is not eligible.  Per fragment, int32:

        * ``frag_shift``: the left shift of ``pipeline.fragment_token_ranges`` / ``score_fragments``: 0 for a fragment of
          sentence 0, else ``sum(prefix_token_counts[:min(k, len(counts))])`` for sentence index ``k``;
        * ``frag_sent``: the corpus-wide number of its sentence, the item's sentence base plus ``sentence_index``;
        * ``frag_first_id`` (host only): its first token id, -1 for a fragment without tokens (an empty context's fallback
          sentence: a request that takes a row from it keeps the host stages);

        and per item ``sent_base`` (``[n_items + 1]``, the prefix sums of ``len(sentences)``) and ``item_title`` (the sentence
        ``always_select_title`` keeps when any is kept: 0 with prefix sentences or a title that is the first sentence, else
        -1, as ``postprocess_contexts`` picks it).  Eligible: in every item
        ``sentence_index`` does not decrease over the fragments and lies inside ``len(sentences)`` -- a sentence's fragments are
        then one run of the context's fragments, which is what the device walks."""

        if self._decision_tables is False:
            n_sentences = np.fromiter((len(item.sentences) for item in self.items), dtype=np.int64, count=len(self.items))
            sent_base = np.zeros(len(self.items) + 1, dtype=np.int64)
            sent_base[1:] = np.cumsum(n_sentences)
            tables = None
            if int(sent_base[-1]) < 2**31 - 1 and self.n_tokens < 2**31 - 1:
                frag_shift = np.zeros(self.n_fragments, dtype=np.int32)
                frag_sent = np.zeros(self.n_fragments, dtype=np.int32)
                frag_first_id = np.zeros(self.n_fragments, dtype=np.int32)
                eligible, at = True, 0
                for item, base in zip(self.items, sent_base.tolist()):
                    counts = item.prefix_token_counts
                    offsets = [0]
                    for c in counts:
                        offsets.append(offsets[-1] + c)
                    previous, limit, last = 0, len(item.sentences), len(counts)
                    for fragment in item.fragments:
                        k = fragment.sentence_index
                        if k < previous or k >= limit:
                            eligible = False
                            break
                        previous = k
                        frag_shift[at] = offsets[k if k < last else last] if k > 0 else 0
                        frag_sent[at] = base + k
                        frag_first_id[at] = fragment.token_ids[0] if fragment.token_ids else -1
                        at += 1
                    if not eligible:
                        break
                if eligible:
                    item_title = np.fromiter(
                        (0 if item.sentences and (item.prefix_sentences or item.title_is_first_sentence) else -1 for item in self.items),
                        dtype=np.int32, count=len(self.items))
                    tables = {"frag_shift": frag_shift, "frag_sent": frag_sent, "frag_first_id": frag_first_id,
                              "sent_base": sent_base.astype(np.int32), "item_title": item_title}
            self._decision_tables = tables
        return self._decision_tables


def as_request(question: Any, context: Any) -> "tuple[list[str], list[PreparedView], str] | None":
    """``process()``'s input-shape dispatch for prepared contexts: ``(queries, one view per query, structure)``, or None
    when ``context`` is not prepared (raw texts).  One question goes with one prepared object or view (structure
    ``"list"``), a list of questions with a list of as many (``"nested"``)."""

    def as_view(value: Any) -> PreparedView | None:
        if isinstance(value, PreparedContexts):
            return PreparedView(value, range(len(value)))
        return value if isinstance(value, PreparedView) else None

    single = as_view(context)
    if single is not None:
        if isinstance(question, str):
            return [question], [single], "list"
        queries = [str(q) for q in question]
        if len(queries) != 1:
            raise ValueError("one prepared object or view goes with one question; pass a list of views, one per question")
        return queries, [single], "list"
    if not isinstance(context, (list, tuple)) or not context or not any(as_view(c) is not None for c in context):
        return None
    views = [as_view(c) for c in context]
    if any(v is None for v in views):
        raise ValueError("a list of contexts is either all prepared views or all raw texts")
    if isinstance(question, str):
        raise ValueError("a list of prepared views needs a list of questions, one per view")
    queries = [str(q) for q in question]
    if len(queries) != len(views):
        raise ValueError("Number of prepared views must match number of queries")
    if any(v.corpus is not views[0].corpus for v in views):
        raise ValueError("the views of one request must come from one prepared corpus")
    return queries, views, "nested"
