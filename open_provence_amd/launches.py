"""The launch layer of ``process()``: enqueue a forward now, collect its results later.

The host stages of the neighbouring batches overlap the GPU: a launch is pinned H2D copies, the forward, pinned D2H copies
and one event (:func:`enqueue_packed`); a collector waits for the event and hands the values on -- per-row lists
(:func:`collect_rows`), packed arrays for a host-mode front-end (:func:`collect_packed`), or the gather of a row-sharded
call (:func:`collect_rows_sharded`).  The functions take the model: its encoder, device, process group and
:class:`Staging`.  ``OpenProvenceModel`` keeps them as methods of the same names (``_launch_rows``, ``_collect_rows``, ...).
"""

from __future__ import annotations

from dataclasses import dataclass
from typing import Any, Sequence

import numpy as np
import torch

from .packing import pack_rows


# -- token ranges of a packed batch ----------------------------------------------------------------------------------
def flatten_segments(cu: Sequence[int], segments: Sequence[Sequence[tuple[int, int]]]) -> tuple[np.ndarray, list[int]]:
    """Per-row token ranges (positions within the row) -> (the ranges as absolute ``(start, end)`` positions of the packed
    batch whose row offsets are ``cu``, int32 ``[2 * n]``; ranges per row).  An empty range is written as ``(start, start)``."""

    counts = [len(s) for s in segments]
    flat = np.empty(2 * sum(counts), dtype=np.int32)
    pos = 0
    for i, segs in enumerate(segments):
        base = int(cu[i])
        for start, end in segs:
            flat[pos] = base + start
            flat[pos + 1] = base + end if end > start else base + start
            pos += 2
    return flat, counts


def split_by_counts(values: Any, counts: Sequence[int]) -> list[Any]:
    """A flat list or array of values -> one slice per row, ``counts[i]`` values each (the inverse of flattening)."""

    out, pos = [], 0
    for c in counts:
        out.append(values[pos : pos + c])
        pos += c
    return out


def pack_launch(rows: list[list[int]], segments: list[list[tuple[int, int]]] | None):
    """Rows (+ per-row token ranges) -> the arrays a launch consumes: packed ids, row offsets, the longest row, the
    ranges as absolute (start, end) token positions of the packed batch, ranges per row.  This is also what a
    host-stage replica sends to the GPU owner (frontend.py) -- a few numpy buffers instead of lists of Python ints."""

    ids_np, cu_np, max_len = pack_rows(rows)
    if segments is None:
        return ids_np, cu_np, max_len, None, None
    return (ids_np, cu_np, max_len, *flatten_segments(cu_np, segments))


# -- what a launch leaves behind until it is collected ---------------------------------------------------------------
@dataclass
class Launch:
    """One enqueued forward of this process.  ``pool``: the staging slot its results land in; ``total`` / ``rows``: tokens and
    rows of the launch; ``seg_counts``: ranges per row when the means are taken on the device, else None; ``alive``: the
    device tensors of the launch, held until it is collected; ``shard``: the row assignment of a row-sharded call
    (:func:`launch_rows`); ``retry`` / ``f8`` / ``slot`` / ``ids_dev``: what the range guard needs to repeat it; ``planned``: the
    tables of a prepared request whose fragment means come from the row plan (``op_planned_fragment_means``), for the repeat too."""

    event: Any
    pool: Any
    total: int
    rows: int
    cu: Any
    seg_counts: list[int] | None
    alive: Any = None
    shard: dict[str, Any] | None = None
    retry: tuple | None = None
    f8: bool = False
    slot: int | None = None
    ids_dev: Any = None
    planned: dict[str, Any] | None = None

    @classmethod
    def empty(cls, cu: Any, reduced: bool) -> "Launch":
        """(more ranks than rows) nothing was enqueued here; the gather still runs on every rank."""

        return cls(event=None, pool=None, total=0, rows=0, cu=cu, seg_counts=[] if reduced else None)


@dataclass
class RemoteLaunch:
    """A forward a host-stage replica has sent to the GPU owner (``remote.submit``): ``remote.result(launch)`` receives it."""

    remote: Any
    rows: int
    cu: Any
    seg_counts: list[int] | None


class Staging:
    """Pinned host staging buffers of a model's launches (two slots, grown on demand, reused across calls: pinning memory
    costs ms) and the rotation between them.

    The host side fills and drains them through numpy views: an ATen CPU ``copy_`` of a batch this size starts the
    intra-op thread pool, whose workers then spin on every core for a while -- measured on the 256-thread host of
    the GPU box as 3 s of user time inside a 0.17 s ``process()`` call and 2-3x slower Python stages around it."""

    def __init__(self) -> None:
        self.pools: list[dict[str, Any] | None] = [None, None]
        self.slot = -1

    def next_slot(self) -> int:
        self.slot = (self.slot + 1) % 2
        return self.slot

    def pool(self, slot: int, n_tokens: int, n_rows: int, num_labels: int) -> dict[str, Any]:
        pool = self.pools[slot]
        if pool is None or pool["ids"].numel() < n_tokens or pool["cu"].numel() < n_rows + 1:
            cap_t, cap_r = max(n_tokens, 1) * 5 // 4 + 64, max(n_rows + 1, 2) * 5 // 4 + 8
            pool = {
                "ids": torch.empty(cap_t, dtype=torch.int32).pin_memory(),
                "cu": torch.empty(cap_r, dtype=torch.int32).pin_memory(),
                "keep": torch.empty(cap_t, dtype=torch.float32).pin_memory(),
                "rank": torch.empty(cap_r * num_labels, dtype=torch.float32).pin_memory(),
                "seg": torch.empty(2 * cap_t, dtype=torch.int32).pin_memory(),  # a fragment has at least one token
            }
            for name in ("ids", "cu", "keep", "rank", "seg"):
                pool[name + "_np"] = pool[name].numpy()
            self.pools[slot] = pool
        return pool


# -- launch ----------------------------------------------------------------------------------------------------------
def dist_info(model) -> dict[str, Any] | None:
    info = getattr(model, "_dist", None)
    if info and info.get("local_only"):  # inside a job-sharded process(): this rank's forward batches are its own
        return None
    return info if info and (info["world"] > 1 or info.get("force")) else None


def count_forward(model, n_rows: int, n_tokens: int) -> None:
    """One forward this process enqueued (or, a host-stage replica, submitted): ``performance_trace.runtime["forwards"]``."""

    stats = model.__dict__.get("_forward_stats")
    if stats is not None:
        stats["launches"] += 1
        stats["rows"] += int(n_rows)
        stats["tokens"] += int(n_tokens)


def launch_rows(model, rows: list[list[int]], segments: list[list[tuple[int, int]]] | None = None) -> "Launch | RemoteLaunch":
    """Enqueue one forward on the current stream: pinned H2D of the packed ids, the forward (keep-probability from
    the head kernel), pinned D2H of keep-probabilities + ranking logits, one event.  Nothing here waits for the GPU.

    With ``segments`` (per row, token ranges within the row) the keep-probabilities stay on the device: their mean
    over every range is taken there (``op_segment_means``: numpy's float32 pairwise order, bit for bit) and only
    4 bytes per range come back."""

    remote = model.__dict__.get("_remote_forward")
    if remote is not None:  # host-stage replica (frontend.py, mode="host"): the GPU owner's process runs the forward
        count_forward(model, len(rows), sum(len(r) for r in rows))
        return remote.submit(rows, segments)
    info = dist_info(model)
    if info is None:
        return model._enqueue_local(rows, segments)
    # Data parallelism over the rows: the token-balanced plan every rank derives from the
    # row lengths alone; this rank enqueues only its share -- same pinned staging, same asynchronous copies, same
    # on-device fragment means as the single-GPU path -- and collect_rows gathers 4 bytes per FRAGMENT (or per
    # token, without segments) + the ranking logits on the post-processing rank.
    from .sharding import ShardPlan

    lengths = [len(r) for r in rows]
    token_plan = ShardPlan(lengths, info["world"], width=1, num_labels=int(model.dims.num_labels))
    mine = token_plan.local_rows(info["rank"])
    launch = model._enqueue_local([rows[i] for i in mine], [segments[i] for i in mine] if segments is not None else None)
    launch.shard = {"mine": mine, "n_rows_all": len(rows), "lengths": lengths, "shards": token_plan.shards,
                    "counts_all": [len(sg) for sg in segments] if segments is not None else None}
    return launch


def enqueue_packed(model, ids_np: np.ndarray | None, cu_np: np.ndarray, max_len: int, seg_flat: np.ndarray | None,
                   seg_counts: list[int] | None, reuse_slot: int | None = None, *, assemble: dict[str, Any] | None = None,
                   ids_dev: torch.Tensor | None = None, planned: dict[str, Any] | None = None) -> Launch:
    """Enqueue one forward over packed rows (:func:`pack_launch`); also what the range guard of the fp16 + e4m3
    kernel sets repeats, see :func:`guard_launch`."""

    retry = (ids_np, cu_np, max_len, seg_flat, seg_counts)
    # Prepared contexts (``ids_np`` is None): the ids are laid out on the device by ``assemble`` (``_assemble_on_device``
    # from the request's plan) or, the range guard's repeat, are the launch's own ``ids_dev`` once more.  They were
    # checked when the corpus and the request's queries were uploaded.  With ``assemble["means"]`` (or, the repeat, ``planned``)
    # the fragment means follow from the same plan on the device (``_planned_means_on_device``), into the forward's slice of
    # the request's buffer; 4 bytes per fragment come back for the range guard, as with ``seg_flat``.
    if ids_np is not None:
        model.encoder.check_ids(ids_np)
    total, n_rows, nl = int(cu_np[-1]), len(cu_np) - 1, int(model.dims.num_labels)
    if n_rows == 0:
        return Launch.empty(cu_np, seg_counts is not None)
    staging: Staging = model._staging
    if reuse_slot is not None:
        # the synchronous repeat of a guarded launch re-uses THAT launch's staging slot (its values have been read) and
        # leaves the rotation alone: with A on slot 0 and B still in flight on slot 1, a repeat of A that advanced the
        # rotation would hand slot 1 to the next launch while B's results are uncollected there
        slot = reuse_slot
    else:
        slot = staging.next_slot()
    pool = staging.pool(slot, max(total, 4 * n_rows) if assemble is not None else total, n_rows, nl)
    dev = model._runtime_device
    np.copyto(pool["cu_np"][: n_rows + 1], cu_np)
    cu_dev = pool["cu"][: n_rows + 1].to(dev, non_blocking=True)
    if ids_np is not None:
        np.copyto(pool["ids_np"][:total], ids_np)
        ids_dev = pool["ids"][:total].to(dev, non_blocking=True)
    elif assemble is not None:
        # the plan travels through the slot's id staging (4 words per row instead of the row's tokens)
        plan_np = assemble["plan"]
        np.copyto(pool["ids_np"][: plan_np.size], plan_np.reshape(-1))
        plan_dev = pool["ids"][: plan_np.size].to(dev, non_blocking=True)
        ids_dev = model._assemble_on_device(assemble, plan_dev, plan_np, cu_dev, cu_np)
        if "means" in assemble:
            planned = dict(assemble, plan_dev=plan_dev)
    keep_dev = torch.empty(total, dtype=torch.float32, device=dev)
    seg_dev = means_dev = None
    n_seg = 0
    if planned is not None:
        seg_flat, seg_counts = None, planned["seg_counts"]
        n_seg = sum(seg_counts)
    elif seg_counts is not None:
        n_seg = sum(seg_counts)
        if 2 * n_seg > pool["seg"].numel():
            seg_flat = seg_counts = None  # (cannot happen for non-empty fragments; fall back to the token payload)
    if seg_counts is not None and planned is None:
        np.copyto(pool["seg_np"][: 2 * n_seg], seg_flat)
        seg_dev = pool["seg"][: 2 * n_seg].to(dev, non_blocking=True).view(n_seg, 2)
    _, rank_dev = model.encoder.forward_packed(ids_dev, cu_dev, cu_np, max_len, keep_prob=keep_dev, ids_host=ids_np)
    count_forward(model, n_rows, total)
    if planned is not None:
        # (ids_dev: the rows this launch assembled or, the range guard's repeat, the first launch's -- what a located request,
        # ``means["locate"]``, looks its contexts up in)
        means_dev = model._planned_means_on_device(planned, cu_dev, cu_np, keep_dev, ids_dev)
        pool["keep"][:n_seg].copy_(means_dev, non_blocking=True)
    elif seg_counts is not None:
        means_dev = model.encoder.segment_means(keep_dev, seg_dev)
        pool["keep"][:n_seg].copy_(means_dev, non_blocking=True)
    else:
        pool["keep"][:total].copy_(keep_dev, non_blocking=True)
    pool["rank"][: n_rows * nl].copy_(rank_dev.reshape(-1), non_blocking=True)
    event = torch.cuda.Event()
    event.record(torch.cuda.current_stream(dev))
    return Launch(event=event, pool=pool, total=total, rows=n_rows, cu=cu_np, seg_counts=seg_counts,
                  alive=(ids_dev, cu_dev, keep_dev, rank_dev, seg_dev, means_dev), retry=retry,
                  f8=model.encoder.f8_active(), slot=slot, ids_dev=ids_dev if ids_np is None else None, planned=planned)


def guard_launch(model, launch: Launch) -> Launch:
    """Range guard of the fp16 + e4m3 kernel sets for a pipelined launch (the launch has completed): when its
    results -- fragment means or keep-probabilities, ranking logits -- are not finite and it ran on those sets, the
    model falls back to the (hi, lo) bf16 sets (``HipEncoder.fall_back_from_f8``: warn once, stay there) and THIS
    launch is repeated synchronously; the repeat is returned.  Launches already in flight are guarded
    the same way when they are collected.  On the bf16 sets nothing is tested (reference arithmetic, fp32 range)."""

    if not launch.f8 or launch.retry is None or launch.rows == 0:
        return launch
    pool, nl = launch.pool, int(model.dims.num_labels)
    n_val = sum(launch.seg_counts) if launch.seg_counts is not None else launch.total
    if np.isfinite(pool["keep_np"][:n_val]).all() and np.isfinite(pool["rank_np"][: launch.rows * nl]).all():
        return launch
    model.encoder.fall_back_from_f8("process")
    if model.encoder.f8_active():
        return launch  # (nothing to fall back to: the caller reports the NaN)
    launch.alive = None
    # (a device-assembled launch is repeated on the ids it laid out: the same device buffer, no second assembly)
    # (... and its planned fragment means are taken again, into the same slice of the request's buffer)
    again = model._enqueue_packed(*launch.retry, reuse_slot=launch.slot, ids_dev=launch.ids_dev, planned=launch.planned)
    again.shard = launch.shard
    again.event.synchronize()
    return again


# -- collect ---------------------------------------------------------------------------------------------------------
def finish_launch(model, launch: Launch) -> tuple[Launch, np.ndarray, np.ndarray]:
    """Wait for a launch and take its results off the staging slot -> (the launch, or the range guard's repeat of it;
    ranking logits ``[rows, nl]``; the launch's values as one float32 array: per-range means when it had ranges, else
    per-token keep-probabilities).  A rank that enqueued nothing (:meth:`Launch.empty`) gets empty arrays."""

    nl = int(model.dims.num_labels)
    if launch.event is not None:
        launch.event.synchronize()
        launch = model._guard_launch(launch)  # (a rank of a group repeats ITS rows before the gather: the payload is finite)
    n_rows = launch.rows
    n_val = sum(launch.seg_counts) if launch.seg_counts is not None else launch.total
    if n_rows:
        rank = launch.pool["rank_np"][: n_rows * nl].copy().reshape(n_rows, nl)
        values = launch.pool["keep_np"][:n_val].copy()  # the slot is reused two launches later
    else:
        rank, values = np.zeros((0, nl), dtype=np.float32), np.zeros(0, dtype=np.float32)
    launch.alive = None
    return launch, rank, values


def collect_rows(model, launch: "Launch | RemoteLaunch") -> tuple[torch.Tensor, list[Any]]:
    """-> (ranking logits, per row: its keep-probabilities, or -- launched with ``segments`` -- the list of its
    range means as Python floats)."""

    if isinstance(launch, RemoteLaunch):
        return launch.remote.result(launch)
    if launch.shard is not None:
        return collect_rows_sharded(model, launch)
    launch, rank, values = finish_launch(model, launch)
    if launch.seg_counts is not None:
        return torch.from_numpy(rank), split_by_counts(values.tolist(), launch.seg_counts)  # float32 -> Python float, exact
    return torch.from_numpy(rank), split_by_counts(values, np.diff(launch.cu).tolist())


def collect_packed(model, launch: Launch) -> tuple[np.ndarray, np.ndarray, bool]:
    """:func:`collect_rows` without the per-row Python objects: (ranking logits [rows, nl], the launch's values as one
    float32 array, reduced?) -- values = per-range means when the launch had ranges (reduced), else per-token
    keep-probabilities.  What the GPU owner of a host-mode front-end sends back to its replicas (frontend.py)."""

    launch, rank, values = finish_launch(model, launch)
    return rank, values, launch.seg_counts is not None


def collect_rows_sharded(model, launch: Launch) -> tuple[torch.Tensor, list[Any]]:
    """The group form of :func:`collect_rows`: wait for this rank's launch, then ONE gather of fixed-size payloads
    (per-fragment means -- or, launched without segments, per-token keep-probabilities -- + ranking logits) to
    rank ``dst`` (RCCL over xGMI with backend "nccl"; the payload is KBs).  Every rank calls this for the same
    launches in the same order; ranks other than ``dst`` get zero placeholders (their ``process()`` result is
    discarded)."""

    import torch.distributed as dist

    from .sharding import ShardPlan

    info, shard = dist_info(model), launch.shard
    nl = int(model.dims.num_labels)
    n_all, lengths, counts_all = shard["n_rows_all"], shard["lengths"], shard["counts_all"]
    per_row = counts_all if counts_all is not None else lengths  # values per row in the payload
    launch, rank_local, values = finish_launch(model, launch)
    plan = ShardPlan(per_row, info["world"], width=1, num_labels=nl, shards=shard["shards"])  # the launch's row assignment
    comm = model._runtime_device if dist.get_backend(info["group"]) == "nccl" else torch.device("cpu")
    gathered = plan.gather(torch.from_numpy(values).to(comm), torch.from_numpy(rank_local).to(comm), dst=info["dst"], group=info["group"])
    if gathered is None:
        if counts_all is not None:
            return torch.zeros((n_all, nl), dtype=torch.float32), [[0.0] * c for c in counts_all]
        return torch.zeros((n_all, nl), dtype=torch.float32), [np.zeros(n, dtype=np.float32) for n in lengths]
    vals, rank_all = gathered
    flat = vals.reshape(-1).cpu().numpy()
    return rank_all.cpu(), split_by_counts(flat.tolist() if counts_all is not None else flat, per_row)  # (tolist: exact)
