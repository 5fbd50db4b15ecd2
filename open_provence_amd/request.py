"""One ``process()`` request, stage by stage.

``OpenProvenceModel._process_impl`` is the driver; the stages it names live here, each readable alone: resolve the
request (raw texts, handed over by a front-end, or prepared contexts), set up job sharding, settle the loader and its
worker threads, run the raw job loop or the prepared request, post-process and gather, and account for the time.  The
pure pieces (loader settings, the shape of the outputs, the small records of the job stream) are in ``pipeline.py``, the
forwards go through the launch layer (``launches.py``) by the model's methods.
"""

from __future__ import annotations

import itertools
import os
from collections.abc import Callable, Mapping, Sequence
from dataclasses import dataclass, field
from time import perf_counter
from typing import Any, NamedTuple

import numpy as np
import torch

from . import pipeline as pl
from .launches import flatten_segments
from .pipeline import ContextState
from .prepared import PreparedView
from .splitters import is_builtin_splitter


# -- 1. the request --------------------------------------------------------------------------------------------------
@dataclass
class Request:
    """``views``: prepared contexts, one view per query (``contexts`` = the entries post-processing falls back to, as title
    resolution left them at preparation); ``handed``: the normalised request a host-mode front-end's owner gave this replica."""

    queries: list[str]
    contexts: list[list[Any]]
    titles: list[Any]
    structure: str
    max_fragment_tokens: int
    sep_len: int
    views: Sequence[PreparedView] | None = None
    handed: Mapping[str, Any] | None = None

    @property
    def total_jobs(self) -> int:
        return sum(len(per_query) for per_query in self.contexts) if self.views is None else 0


def resolve_request(model, question, context, title, first_line_as_title: bool, respect_sentence_boundaries: bool, prepared) -> Request:
    # (host-mode front-end: the owner has normalised the request and assigned the jobs once for all replicas; a
    # replica gets the normalised structure with the texts of the contexts it does not own blanked)
    handed = (getattr(model, "_dist", None) or {}).get("prenormalized")
    views = None
    if prepared is not None:  # (prepared.as_request)
        queries, views, structure = prepared
        contexts = [[view.corpus.items[i].entry for i in view.indices] for view in views]
        titles = [None] * len(queries)
    else:
        if handed is not None:
            queries, contexts, structure = handed["queries"], handed["contexts"], handed["structure"]
        else:
            queries, contexts, structure = model._normalize_inputs(question, context)
        contexts, titles = model._resolve_titles(queries, contexts, title, first_line_as_title=first_line_as_title)
    sep_token_ids = model.tokenizer.encode(model.tokenizer.sep_token or "", add_special_tokens=False)
    return Request(queries, contexts, titles, structure, pl.max_fragment_tokens(model.max_length, respect_sentence_boundaries),
                   len(sep_token_ids), views, handed)


def debug_callback_of(debug_messages: bool | Callable[[str], None], logger) -> Callable[[str], None] | None:
    if isinstance(debug_messages, bool):
        return logger.info if debug_messages else None
    if callable(debug_messages):
        return debug_messages
    raise TypeError("debug_messages must be a bool or a callable that accepts a string")


# -- 2. job sharding -------------------------------------------------------------------------------------------------
@dataclass
class JobSharding:
    """A job-sharded call on this rank: the group (``model._dist``), which contexts the rank owns, how many, and whether
    the rank has entered the gather (with its results, or with the error marker)."""

    info: dict[str, Any]
    owned: list[list[bool]]
    total_jobs: int
    entered: bool = False


def enter_job_sharding(model, request: Request, stack) -> JobSharding | None:
    """Job-level sharding (``attach_process_group(shard="jobs")``): this rank prepares, runs and post-processes only the
    contexts it owns; its forward batches are then purely local (``local_only``, reset when ``stack`` unwinds).  None
    without such a group."""

    info = getattr(model, "_dist", None)
    if not (info and info.get("shard") == "jobs" and (info["world"] > 1 or info.get("force"))):
        return None
    handed = request.handed
    owner = handed["owner"] if handed is not None else pl.assign_jobs(request.contexts, info["world"])
    owned = [[r == info["rank"] for r in per_query] for per_query in owner]
    sharding = JobSharding(info, owned, sum(sum(per_query) for per_query in owned))
    info["local_only"] = True
    stack.callback(info.__setitem__, "local_only", False)
    if info["world"] > 1 and handed is None and model._forward_is_native() and model.encoder.audit_pending:
        # every rank has the whole request: the audit rows are its head (first query, up to eight contexts), the
        # same on every rank, whatever jobs a rank owns
        from .sharding import collective_audit

        collective_audit(model.encoder, model._audit_rows_of_request(request.queries, request.contexts), info["group"])

    def _leave_with_error(_exc_type, exc, _tb):
        # an exception on this rank before its gather: enter the collective with an error marker, so that
        # the peers are told instead of blocking in gather_object forever; then let the exception go on
        if exc is not None and not sharding.entered:
            sharding.entered = True
            try:
                model._gather_job_results(None, None, info, error=exc)
            except Exception:  # (a broken group must not mask the original error)
                pass
        return False

    stack.push(_leave_with_error)
    return sharding


# -- 3. loader settings, worker threads, granule ---------------------------------------------------------------------
def default_thread_workers(model, total_jobs: int, splitter) -> int:
    """Worker threads for the split / tokenize stage WITHOUT a request for them: four from 128 jobs on when BOTH hold: the
    tokenizer is a Hugging Face fast one (its Rust batch calls run outside the GIL) and the sentence splitter is one of
    this package's own (thread-safe: stateless regex / lazily initialised under a lock).  A caller-supplied splitter is
    never called from several threads unless workers were asked for -- the reference only ever ran splitters in separate
    processes (standalone.py:3589).  Pure-Python tokenizers are served best by the lazy single-thread pipeline (the
    reference's own default is 0 workers under 2000 jobs, standalone.py:2591-2592)."""

    fast = hasattr(getattr(model.tokenizer, "_tokenizer", None), "encode_batch")
    return 4 if (total_jobs >= 128 and is_builtin_splitter(splitter) and fast) else 0


def pipelining_granule(total_jobs: int, preprocess_batch: int) -> int:
    """Native pipelined path: the forward of one granule of contexts runs on the GPU while the host splits,
    tokenizes and assembles the next one (rows are independent, so the granule does not change results).
    A call costs about (launch overhead) x N / g for its launches plus (GPU time per context) x g for the
    last granule, which nothing overlaps: with ~0.3 ms and ~29 us measured on xsmall at seq_len 512 the
    optimum is g ~ 3.2 sqrt(N) (51 / 103 / 205 contexts at N = 256 / 1024 / 4096; a sweep over 64 / 128 / 256
    agrees).
    (A host-stage replica keeps this granule: with many replicas the GPU owner already sees a stream of
    batches, and every extra batch costs a replica ~1 ms of fixed work -- measured at 1024 contexts and 31
    replicas: one batch per replica 27.2 k contexts/s, four 23.8 k, six 22.8 k.)"""

    granule = -(-int(3.2 * total_jobs**0.5) // 16) * 16
    preprocess_batch = min(preprocess_batch, max(32, granule))
    if preprocess_batch < total_jobs <= preprocess_batch * 3 // 2:
        preprocess_batch = total_jobs  # (no separate launch for a remainder of less than half a granule)
    return preprocess_batch


def plan_host_stages(model, total_jobs: int, batch_size: int, splitter, preprocess_workers, preprocess_batch_size,
                     torch_dataloader_kwargs, debug_callback) -> tuple[int, int]:
    """-> (worker threads of the split / tokenize stage, contexts per granule of the job loop)."""

    given = pl.loader_settings(preprocess_workers, preprocess_batch_size, batch_size, torch_dataloader_kwargs,
                               os.getenv("OPEN_PROVENCE_PREPROCESS_WORKERS"))
    workers, preprocess_batch, _prefetch = model._auto_tune_preprocess_loader(
        total_jobs=total_jobs, inference_batch_size=batch_size, current_workers=given.workers,
        current_preprocess_batch=given.preprocess_batch, current_prefetch=given.prefetch, workers_explicit=given.workers_explicit,
        batch_explicit=given.batch_explicit, prefetch_explicit=given.prefetch_explicit)
    # as many threads as explicitly requested (preprocess_workers=, the OPEN_PROVENCE_PREPROCESS_WORKERS variable or
    # torch_dataloader_kwargs["num_workers"]); without a request, the default rule
    if given.workers_explicit:
        thread_workers = min(int(workers), 32) if workers > 0 else 0
    else:
        thread_workers = default_thread_workers(model, total_jobs, splitter)
    if debug_callback is not None:
        debug_callback(f"[OpenProvenceModel] preprocess_workers={workers} preprocess_threads={thread_workers} "
                       f"preprocess_batch={preprocess_batch} default_workers={pl.default_preprocess_workers()}")
    if model._can_pipeline() and not given.batch_explicit:  # (an explicit preprocess batch is honoured as given)
        preprocess_batch = pipelining_granule(total_jobs, preprocess_batch)
    return thread_workers, preprocess_batch


# -- 4. run ----------------------------------------------------------------------------------------------------------
@dataclass
class Run:
    """What the forwards of a request leave behind: the per-context states, the forwards in flight (pipelined native
    path), the seconds of the assembly and inference stages, the blocks that went through a forward."""

    states: dict[tuple[int, int], ContextState] = field(default_factory=dict)
    pending: list[Any] = field(default_factory=list)
    assembly_seconds: float = 0.0
    inference_seconds: float = 0.0
    blocks: int = 0
    # a prepared request: where its fragment means and sentence decisions were taken ("device" / "host"), and on the device
    # what post-processing needs (:class:`Decided`)
    prepared_decisions: str | None = None
    decided: "Decided | None" = None


def run_raw_jobs(model, request: Request, run: Run, splitter, owned, thread_workers: int, preprocess_batch: int, batch_size: int,
                 timing: dict[str, float], *, strip_sentences: bool, respect_sentence_boundaries: bool) -> None:
    """The job loop of a request of raw texts: a granule of jobs from the stream, their fragments and blocks, their forwards."""

    fragment_args = dict(max_fragment_tokens=request.max_fragment_tokens, strip_sentences=strip_sentences,
                         respect_sentence_boundaries=respect_sentence_boundaries)
    query_token_ids: list[list[int]] = []
    job_stream = model._iter_jobs(
        request.queries, request.contexts, request.titles, splitter, query_token_ids, strip_sentences=strip_sentences,
        timing=timing, workers=thread_workers, group_size=min(64, max(1, preprocess_batch)), owned=owned,
        fragment_args=fragment_args if thread_workers > 0 else None,
    )
    while True:
        batch_jobs = list(itertools.islice(job_stream, preprocess_batch))
        if not batch_jobs:
            break
        inference_jobs: list[dict[str, Any]] = []
        t_asm = perf_counter()
        if "fragments" in batch_jobs[0]:  # the worker threads decoded them with their group
            fragments_per_job = [job["fragments"] for job in batch_jobs]
        else:
            t0 = perf_counter()
            # one batch_decode over the fragments of the whole batch
            fragments_per_job = pl.fragmentize_many(
                model.tokenizer, [(job["token_lists"], job["context_text"]) for job in batch_jobs], **fragment_args)
            timing["fragment_decode_seconds"] += perf_counter() - t0
        for job, fragments in zip(batch_jobs, fragments_per_job):
            q_idx, c_idx = job["query_idx"], job["context_idx"]
            blocks = model._assemble_blocks_from_fragments(len(query_token_ids[q_idx]), request.sep_len, fragments)
            run.states[(q_idx, c_idx)] = pl.context_state(job, fragments, blocks)
            inference_jobs.extend(pl.inference_job(q_idx, c_idx, b_idx, block) for b_idx, block in enumerate(blocks))
        run.assembly_seconds += perf_counter() - t_asm
        if inference_jobs:
            run.inference_seconds += model._run_inference_batches(inference_jobs, batch_size, request.queries, query_token_ids,
                                                                  run.states, run.pending)
            run.blocks += len(inference_jobs)


# -- prepared contexts (prepared.py): the request-time half --------------------------------------------------------------
def _prepared_state(states, q_idx: int, c_idx: int, item, blocks) -> ContextState:
    state = states.get((q_idx, c_idx))
    if state is None:
        state = states[(q_idx, c_idx)] = pl.context_state(item, item.fragments, blocks)
    return state


def prepared_rows(model, views: Sequence[PreparedView], query_token_ids: list[list[int]], sep_len: int, states) -> list[tuple]:
    """Per row of the request: query, context, block, the context's item and blocks, (first fragment within the context,
    fragments, clip, context tokens).  Lengths only: states and jobs are built forward by forward, beside the GPU -- but
    for a context without blocks, whose state is made here."""

    corpus = views[0].corpus
    rows: list[tuple] = []
    for q_idx, view in enumerate(views):
        q_len = len(query_token_ids[q_idx])
        for c_idx, at in enumerate(view.indices):
            item = corpus.items[at]
            blocks, plan = item.blocks_for(model.tokenizer, q_len, sep_len, model.max_length)
            if not blocks:
                _prepared_state(states, q_idx, c_idx, item, blocks)
            for b_idx, entry in enumerate(plan):
                rows.append((q_idx, c_idx, b_idx, item, blocks, entry))
    return rows


class _RowLayout(NamedTuple):
    """Where things are in the rows of a prepared request: the row template, the suffix ids an empty context drops, and per
    query where the context starts and the ids a context must not begin with."""

    template: Any
    drop: int
    ctx_at: list[int]
    heads: list[set]


def _upload_queries(model, query_token_ids: list[list[int]], q_lens: list[int]) -> dict[str, Any]:
    """The request's query ids on the device (flat, with offsets), checked against the embedding table."""

    q_off_np = np.zeros(len(query_token_ids) + 1, dtype=np.int32)
    q_off_np[1:] = np.cumsum(q_lens)
    q_ids_np = np.fromiter((t for q in query_token_ids for t in q), dtype=np.int32, count=int(q_off_np[-1]))
    model.encoder.check_ids(q_ids_np)
    dev = model._runtime_device
    return {"ids": torch.from_numpy(q_ids_np).to(dev), "off": torch.from_numpy(q_off_np).to(dev), "off_np": q_off_np}


def _plan_prepared_forward(model, layout: _RowLayout, rows: list[tuple], lengths: list[int], query_token_ids, states):
    """One forward of a prepared request -> (its inference jobs, the assembly plan (4 words per row), the fragments' token
    ranges per row, the ranges their means are taken over, whether a row's layout must come from the host)."""

    chunk: list[dict[str, Any]] = []
    plan_np = np.empty((len(rows), 4), dtype=np.int32)
    ranges_per_job: list[list[tuple[int, int]]] = []
    segments: list[list[tuple[int, int]]] = []
    on_host = False
    heads, ctx_at = layout.heads, layout.ctx_at
    for i, (q_idx, c_idx, b_idx, item, blocks, (first, count, clip, ctx_len)) in enumerate(rows):
        state = _prepared_state(states, q_idx, c_idx, item, blocks)
        block = blocks[b_idx]
        chunk.append(pl.inference_job(q_idx, c_idx, b_idx, block))
        if ctx_len == 0:
            on_host = on_host or layout.template.empty_context is None
            plan_np[i] = (q_idx, item.frag_base + first, 0, -1 if layout.drop else 0)
        else:
            plan_np[i] = (q_idx, item.frag_base + first, count, clip)
        if ctx_len == 0 or not block[0].token_ids or block[0].token_ids[0] in heads[q_idx]:
            ranges = model._prepare_block_inputs(query_token_ids[q_idx], block)[3]
        else:
            ranges, cursor = [], ctx_at[q_idx]
            for fragment in block:
                ranges.append((cursor, cursor + len(fragment.token_ids)))
                cursor += len(fragment.token_ids)
        ranges_per_job.append(ranges)
        segments.append(pl.fragment_token_ranges(state, block, ranges, lengths[i]))
    return chunk, plan_np, ranges_per_job, segments, on_host


# -- prepared requests whose fragment means and sentence decisions are taken on the device ---------------------------------------
# OPEN_PROVENCE_PREPARED_DECISIONS, read at call time: "0" keeps the host stages (_plan_prepared_forward, score_fragments,
# postprocess_contexts) for every prepared request; anything else lets an eligible request take the device path.  Under "1" a
# request is not eligible when a block begins with a token id of its question -- nearly every request of scripts/process_e2e.py
# --prepared with its own question under the char tokenizer (profiles/prepared_decisions.txt).  "2": as "1", and the device
# looks every context up in its assembled row as the host path does (op_located_fragment_means), so such a request runs on the
# device too; on a library without that call "2" is "1".  Unset = "2": on the request the switch was to be judged by (that
# script with its own question, parent commit and this tree in turns) the wall time falls from 13.9 to 9.2, 43.4 to 35.0 and 162
# to 133-139 ms at 256 / 1024 / 4096 contexts, more than the parent's spread at every size (profiles/prepared_lookup.txt,
# DESIGN.md section 7).
PREPARED_DECISIONS_DEFAULT = "2"


@dataclass
class Decided:
    """A prepared request on the device path: its rows and (query, context) instances as flat tables, the request's device
    buffers, and the ranking logits of the launches collected so far.  No ``ContextState``, no ``FragmentRecord`` is touched."""

    tables: dict[str, np.ndarray]     # PreparedContexts.decision_tables()
    corpus: dict[str, Any]            # the resident corpus (model._prepared_device_corpus)
    items: list[list[Any]]            # per query, per context: the prepared item
    instance_of: list[list[int]]      # ... and its instance, -1 for a context without rows
    instance_item: np.ndarray         # per instance: its item's index in the corpus
    instance_rows: list[tuple[int, int]]  # ... its rows [first, last) of the request, in block order
    instance_slots: np.ndarray        # ... its fragments' slots [n, 2]
    means: dict[str, Any]             # values / slot_frag [n_slots] and slot_off [n_rows + 1] on the device, slot_off_np
    rank: np.ndarray                  # [n_rows, num_labels] ranking logits
    nan_seen: bool = False


def prepared_decisions_on_device(model, corpus) -> bool:
    """What a prepared request needs, whatever its rows, for its last host stages to run on the device."""

    lib = model.encoder.lib
    return (os.getenv("OPEN_PROVENCE_PREPARED_DECISIONS", PREPARED_DECISIONS_DEFAULT) != "0"
            and hasattr(lib, "op_planned_fragment_means") and hasattr(lib, "op_sentence_decisions")
            and corpus.decision_tables() is not None)


def prepared_contexts_located(model) -> bool:
    """``OPEN_PROVENCE_PREPARED_DECISIONS=2`` on a library with ``op_located_fragment_means``: the device looks every context up
    in its row, so a context that begins with an id of its question no longer sends the request to the host stages.  Without
    the symbol "2" behaves as "1"."""

    return (os.getenv("OPEN_PROVENCE_PREPARED_DECISIONS", PREPARED_DECISIONS_DEFAULT) == "2"
            and hasattr(model.encoder.lib, "op_located_fragment_means"))


def _plan_decided(model, views: Sequence[PreparedView], q_lens: list[int], sep_len: int, n_fixed: int):
    """The rows of a prepared request as flat arrays -> (plan [n_rows, 4] int32, row lengths int64, per query the items and
    their instances, per instance its item / rows / slots).  Per row: four plan words and a length."""

    items_all = views[0].corpus.items
    tokenizer, max_length = model.tokenizer, model.max_length
    plan_words: list[int] = []
    lengths: list[int] = []
    items: list[list[Any]] = []
    instance_of: list[list[int]] = []
    instance_item: list[int] = []
    instance_rows: list[tuple[int, int]] = []
    instance_slots: list[int] = []
    n_slots = 0
    for q_idx, view in enumerate(views):
        q_len = q_lens[q_idx]
        fixed = n_fixed + q_len
        q_items, q_instances = [], []
        for at in view.indices:
            item = items_all[at]
            q_items.append(item)
            plan = item.blocks_for(tokenizer, q_len, sep_len, max_length)[1]
            if not plan:
                q_instances.append(-1)
                continue
            q_instances.append(len(instance_item))
            instance_item.append(at)
            first_row, base, slot_begin = len(lengths), item.frag_base, n_slots
            for first, count, clip, ctx_len in plan:
                plan_words += (q_idx, base + first, count, clip)
                lengths.append(fixed + ctx_len)
                n_slots += count
            instance_rows.append((first_row, len(lengths)))
            instance_slots += (slot_begin, n_slots)
        items.append(q_items)
        instance_of.append(q_instances)
    return (np.array(plan_words, dtype=np.int32).reshape(-1, 4), np.array(lengths, dtype=np.int64), items, instance_of,
            np.array(instance_item, dtype=np.int64), instance_rows, np.array(instance_slots, dtype=np.int32).reshape(-1, 2))


def _run_decided(model, request: Request, run: Run, batch_size: int, query_token_ids: list[list[int]], t_asm: float) -> bool:
    """The device path of :func:`run_prepared_request`; False (nothing enqueued, ``run`` untouched) when a row of the request
    rules it out: a row without fragments or context tokens, or a first fragment that begins with an id of its query's
    ``heads`` (its place in the row then does not follow from lengths alone) -- the last one unless the device looks the
    contexts up itself (:func:`prepared_contexts_located`)."""

    views = request.views
    corpus = views[0].corpus
    template, q_lens = corpus.template, [len(q) for q in query_token_ids]
    n_head = len(template.prefix) + len(template.middle)
    n_fixed = n_head + len(template.suffix)
    tables = corpus.decision_tables()
    plan_np, lengths, items, instance_of, instance_item, instance_rows, instance_slots = _plan_decided(model, views, q_lens, request.sep_len, n_fixed)
    n_rows = int(plan_np.shape[0])
    if n_rows == 0:
        return False
    q_of_row = plan_np[:, 0]
    if (plan_np[:, 2] <= 0).any() or (lengths - n_fixed - np.asarray(q_lens, dtype=np.int64)[q_of_row] <= 0).any():
        return False
    first_ids = tables["frag_first_id"][plan_np[:, 1]]
    if (first_ids < 0).any():  # (a block that begins with a fragment without tokens)
        return False
    # "2": every forward looks its contexts up in the rows it assembled (op_located_fragment_means), as the host path does
    located = prepared_contexts_located(model)
    if not located:
        for q_idx, query in enumerate(query_token_ids):
            heads = np.fromiter(set(template.prefix) | set(query) | set(template.middle), dtype=np.int64)
            if heads.size and np.isin(first_ids[q_of_row == q_idx], heads).any():
                return False

    run.blocks += n_rows
    spans = pl.plan_forward_chunks(lengths.tolist(), batch_size, model.forward_token_budget)
    dev = model._runtime_device
    corpus_dev = model._prepared_device_corpus(corpus)
    slot_off_np = np.zeros(n_rows + 1, dtype=np.int32)
    slot_off_np[1:] = np.cumsum(plan_np[:, 2])
    n_slots = int(slot_off_np[-1])
    means = {"values": torch.empty(n_slots, dtype=torch.float32, device=dev), "slot_frag": torch.empty(n_slots, dtype=torch.int32, device=dev),
             "slot_off": torch.from_numpy(slot_off_np).to(dev), "slot_off_np": slot_off_np}
    if located:  # (per row, where its context was found: written by the kernel, read by nobody on the host)
        means.update(locate=True, ctx_start=torch.empty(n_rows, dtype=torch.int32, device=dev))
    assemble = {"corpus": corpus_dev, "queries": _upload_queries(model, query_token_ids, q_lens)}
    counts = plan_np[:, 2].tolist()
    decided = Decided(tables, corpus_dev, items, instance_of, instance_item, instance_rows, instance_slots, means,
                      np.empty((n_rows, int(model.dims.num_labels)), dtype=np.float32))
    run.assembly_seconds += perf_counter() - t_asm

    def collect(entry) -> None:
        launch, start, stop = entry
        launch, rank, values = model._finish_launch(launch)  # (the range guard's repeat runs the planned means again)
        decided.rank[start:stop] = rank
        decided.nan_seen = decided.nan_seen or bool(np.isnan(values).any())

    in_flight: list[tuple] = []
    for start, stop in spans:
        t_asm = perf_counter()
        cu_np = np.zeros(stop - start + 1, dtype=np.int32)
        cu_np[1:] = np.cumsum(lengths[start:stop])
        forward = dict(assemble, plan=plan_np[start:stop], means=dict(means, rows=(start, stop)), seg_counts=counts[start:stop])
        run.assembly_seconds += perf_counter() - t_asm
        t0 = perf_counter()
        in_flight.append((model._enqueue_packed(None, cu_np, int(lengths[start:stop].max()), None, None, assemble=forward), start, stop))
        if len(in_flight) > 1:
            collect(in_flight.pop(0))
        run.inference_seconds += perf_counter() - t0
    t0 = perf_counter()
    while in_flight:
        collect(in_flight.pop(0))
    run.inference_seconds += perf_counter() - t0
    run.decided = decided
    return True


def postprocess_decided_request(model, request: Request, decided: Decided, *, threshold: float, always_select_title: bool,
                                use_best_reranker_score: bool, sentence_probability_groups_requested: bool, collect_sentence_texts: bool,
                                first_line_as_title: bool, zero_score_when_empty: bool) -> tuple[pl.PostprocessResult, float]:
    """After the last launch of a device-path request is collected: ONE ``op_sentence_decisions`` over every instance, one copy
    of the averages and keep flags, one synchronise, then the texts (``pipeline.postprocess_decided``) -> (result, seconds)."""

    t0 = perf_counter()
    tables, item_of = decided.tables, decided.instance_item
    n_inst = int(item_of.shape[0])
    sent_base = tables["sent_base"]
    n_sent = sent_base[item_of + 1] - sent_base[item_of]
    out_at = np.zeros(n_inst + 1, dtype=np.int64)
    out_at[1:] = np.cumsum(n_sent)
    n_out = int(out_at[-1])
    instances = np.empty((n_inst, 6), dtype=np.int32)  # slot_begin, slot_end, sent_out_begin, n_sentences, item_sent_base, title_index
    instances[:, 0:2] = decided.instance_slots
    instances[:, 2], instances[:, 3], instances[:, 4] = out_at[:-1], n_sent, sent_base[item_of]
    instances[:, 5] = tables["item_title"][item_of] if always_select_title else -1
    dev = model._runtime_device
    # averages (fp64) and keep flags (uint8) side by side in one buffer: one copy back, one synchronise
    out_dev = torch.empty(9 * n_out, dtype=torch.uint8, device=dev)
    model.encoder.sentence_decisions(torch.from_numpy(instances).to(dev), instances, decided.means["values"], decided.means["slot_frag"],
                                     decided.corpus["frag_sent"], float(threshold), out_dev[: 8 * n_out].view(torch.float64), out_dev[8 * n_out:])
    out_np = out_dev.cpu().numpy()
    averages, keeps = out_np[: 8 * n_out].view(np.float64), out_np[8 * n_out:]
    scores = model._ranking_scores(torch.from_numpy(decided.rank))
    if decided.nan_seen or any(s != s for s in scores):
        model._warn_nan_once()
    result = pl.postprocess_decided(
        request.queries, request.contexts, decided.items, decided.instance_of, decided.instance_rows, out_at, scores, averages, keeps,
        use_best_reranker_score=use_best_reranker_score, want_sentence_probabilities=sentence_probability_groups_requested,
        want_sentence_texts=collect_sentence_texts, first_line_as_title=first_line_as_title, zero_score_when_empty=zero_score_when_empty)
    return result, perf_counter() - t0


def run_prepared_request(model, request: Request, run: Run, batch_size: int) -> None:
    """The request-time half of ``process()`` on prepared contexts.

    Blocks come from the cached fragments by length arithmetic (``PreparedItem.blocks_for``); the states are what the job
    loop builds from a job.  A replaced forward, a corpus without a row template, or a library without
    ``op_assemble_rows``: the rows are built on the host from the cached fragments (``_run_inference_batches``,
    at most ``batch_size`` rows per call of a replaced forward).  Native forward: ONE ``plan_forward_chunks`` over all
    rows of the request within the token budget; per forward the plan (4 words per row), ``cu_seqlens`` and the
    fragment ranges are uploaded, ``op_assemble_rows`` lays the ids out and the forward runs on them."""

    t_asm = perf_counter()
    views, queries, states, pending = request.views, request.queries, run.states, run.pending
    query_token_ids = [pl.tokenize_query(model.tokenizer, query) for query in queries]
    corpus = views[0].corpus
    on_device = (model._forward_is_native() and corpus.template is not None and hasattr(model.encoder.lib, "op_assemble_rows")
                 and model.__dict__.get("_remote_forward") is None)
    # An eligible corpus (prepared.decision_tables) on a library with op_planned_fragment_means / op_sentence_decisions: the
    # fragments' ranges and means follow on the device from the plan of op_assemble_rows, the sentence decisions from the means
    # (postprocess_decided_request) -- the host keeps four plan words and a length per row.  A request it does not fit (a row
    # without context tokens; under "1", a context that begins with a token of its query or of the template) goes on below, as
    # before.  Under "2" (the default) the device looks the contexts up itself: op_located_fragment_means.
    run.prepared_decisions = "host"
    if on_device and prepared_decisions_on_device(model, corpus) and _run_decided(model, request, run, batch_size, query_token_ids, t_asm):
        run.prepared_decisions = "device"
        return
    rows = prepared_rows(model, views, query_token_ids, request.sep_len, states)
    run.blocks += len(rows)
    if not rows or not on_device:
        inference_jobs = []
        for q_idx, c_idx, b_idx, item, blocks, _entry in rows:
            _prepared_state(states, q_idx, c_idx, item, blocks)
            inference_jobs.append(pl.inference_job(q_idx, c_idx, b_idx, blocks[b_idx]))
        run.assembly_seconds += perf_counter() - t_asm
        if inference_jobs:
            run.inference_seconds += model._run_inference_batches(inference_jobs, batch_size, queries, query_token_ids, states, pending)
        return

    template, q_lens = corpus.template, [len(q) for q in query_token_ids]
    n_fixed = len(template.prefix) + len(template.middle) + len(template.suffix)
    layout = _RowLayout(
        template,
        # a row without context tokens (an empty context's fallback sentence): no fragments in its plan, and no suffix where
        # the tokenizer builds none for an empty second sequence; a layout that is neither comes from the host (below)
        drop=len(template.suffix) if template.empty_context == "drop" else 0,
        ctx_at=[len(template.prefix) + n + len(template.middle) for n in q_lens],
        # ids a context must not begin with for its place in the row to follow from lengths alone: the reference looks the
        # context's tokens up in the row (pipeline.prepare_block_inputs), and an earlier occurrence can only start there
        heads=[set(template.prefix) | set(q) | set(template.middle) for q in query_token_ids])
    lengths = [n_fixed + q_lens[row[0]] + row[5][3] - (0 if row[5][3] else layout.drop) for row in rows]
    spans = pl.plan_forward_chunks(lengths, batch_size, model.forward_token_budget)
    assemble = {"corpus": model._prepared_device_corpus(corpus), "queries": _upload_queries(model, query_token_ids, q_lens)}
    run.assembly_seconds += perf_counter() - t_asm
    for start, stop in spans:
        t_asm = perf_counter()
        chunk, plan_np, ranges_per_job, segments, on_host = _plan_prepared_forward(
            model, layout, rows[start:stop], lengths[start:stop], query_token_ids, states)
        if on_host:  # (a row without context tokens that fits no layout) this forward's rows are built on the host
            host_rows = [model._prepare_block_inputs(query_token_ids[row[0]], row[4][row[2]])[0] for row in rows[start:stop]]
            run.assembly_seconds += perf_counter() - t_asm
            t0 = perf_counter()
            launch = model._launch_rows(host_rows, segments)
        else:
            cu_np = np.zeros(stop - start + 1, dtype=np.int32)
            cu_np[1:] = np.cumsum(lengths[start:stop])
            seg_flat, seg_counts = flatten_segments(cu_np, segments)
            run.assembly_seconds += perf_counter() - t_asm
            t0 = perf_counter()
            launch = model._enqueue_packed(None, cu_np, max(lengths[start:stop]), seg_flat, seg_counts, assemble=dict(assemble, plan=plan_np))
        run.inference_seconds += perf_counter() - t0
        pending.append((launch, chunk, ranges_per_job, queries, states))
        if len(pending) > 1:
            run.inference_seconds += model._flush_pending(pending, keep_last=1)


# -- 5. post-process and gather --------------------------------------------------------------------------------------
def postprocess_and_gather(model, request: Request, run: Run, sharding: JobSharding | None, **options: Any) -> tuple[pl.PostprocessResult, float]:
    """-> (the per-query, per-context results -- on the gather's destination rank of a job-sharded call: of every rank --,
    post-processing seconds, the gather included)."""

    if run.decided is not None:  # (a prepared request on the device path; never sharded)
        result, post_time = postprocess_decided_request(model, request, run.decided, **options)
    else:
        *fields, post_time = model._postprocess_contexts(request.queries, request.contexts, run.states, **options)
        result = pl.PostprocessResult(*fields)
    if sharding is not None:
        t_gather = perf_counter()
        sharding.entered = True
        result = model._gather_job_results(result, sharding.owned, sharding.info)
        post_time += perf_counter() - t_gather
    return result, post_time


# -- 6. the time line and the runtime facts of the trace -------------------------------------------------------------
def owner_stage_seconds(model, start_total: float, assembly: float, stages: tuple[float, float, float]) -> tuple[float, float, float]:
    """(preprocess, inference, postprocess) seconds as measured -- rewritten for the owner of a host-mode front-end.

    The owner prepares, runs and post-processes NO job of its own: its stage timers are
    zero and the whole call used to land under postprocess_seconds -- the field the reference's harness reads for
    its published timings (scripts/eval_datasets.py:225, 359-365).  From the owner's time line of the request:
      preprocess  = request start -> the first forward batch of a replica is launched (the replicas' host stages
                    up to their first submit; later batches overlap the forward),
      inference   = that launch -> the last reply (every launch is collected synchronised before it is answered),
      postprocess = the rest: the replicas' post-processing of their last blocks, their results coming back."""

    hub = (getattr(model, "_dist", None) or {}).get("transport")
    if hub is None or not hasattr(hub, "conns") or not isinstance(getattr(hub, "trace", None), dict):
        return stages
    first = hub.trace.get("first_batch_seconds")
    replies = hub.trace.get("reply_at") or []
    if first is None or not replies:
        return stages
    total_now = perf_counter() - start_total
    preprocess = float(min(first, total_now))
    inference = float(min(max(replies[-1] / 1e3 - first, 0.0), total_now - preprocess))
    return preprocess, inference, float(max(total_now - preprocess - inference - assembly, 0.0))


def runtime_facts(model, forward_stats: dict[str, int], prepared_decisions: str | None = None) -> dict[str, Any]:
    """``performance_trace.runtime``: the kernel set and its calibration, the forwards of the call, the host replicas; on a
    prepared request ``prepared_decisions``: ``"device"`` or ``"host"``, where its fragment means and sentence decisions were taken."""

    runtime: dict[str, Any] = {}
    if prepared_decisions is not None:
        runtime["prepared_decisions"] = prepared_decisions
    if model._forward_is_native() and getattr(model, "encoder", None) is not None:
        runtime["kernel_set"] = model.encoder.effective_policy()["kernel_set"]
        runtime["calibration"] = model.encoder.calibration
        runtime["fallback_from_f8"] = int(getattr(model.encoder, "fallbacks", 0))
    if model._forward_is_native():
        # the forwards this process enqueued (the owner of a host front-end: its replicas' merged batches) or, a
        # host-stage replica, submitted.  A dict on purpose: as_dict() / "timing" keep numbers only
        runtime["forwards"] = dict(forward_stats, token_budget=int(model.forward_token_budget))
    transport = (getattr(model, "_dist", None) or {}).get("transport")
    if transport is not None and hasattr(transport, "conns"):  # the owner of a host-mode front-end
        runtime["host_replicas"] = len(transport.conns)
    return runtime
