"""Re-checking a calibrated kernel set on real batches: the policy, its state and the one audit path.  Nothing here touches a
device or ctypes: ``enc`` is the encoder (``engine.HipEncoder``, or a test's fake) that does, ``call`` an ``engine.PackedCall``."""

from __future__ import annotations

import os
from typing import Callable, Sequence

import numpy as np

from ._lib import KERNEL_SET_IDS

DEFAULT_CALIBRATION_TOLERANCE = 1e-4  # max |logit difference| to the (hi, lo) bf16 kernels; the path's bar is 1e-3
AUDIT_MODES = ("off", "first", "running")
# Tokens one running audit may re-run on the reference set.  A forward of up to 16 k tokens sits at the 0.68 - 0.72 ms launch
# floor on xsmall (profiles/r06_small_request.txt), so half of that is priced like the smallest forward -- ON THE CHOSEN SET: what
# the reference set costs at this size has not been measured.
DEFAULT_AUDIT_TOKENS = 8192
MIN_AUDIT_TOKENS = 64  # batches below this are not audited (first-batch audit and running audit alike)


def resolve_audit_mode(audit: "str | bool | None") -> str:
    """``"off" | "first" | "running"``; ``False`` / ``True`` = ``"off"`` / ``"first"``; ``None`` = ``OPEN_PROVENCE_AUDIT``
    (``0 / off / false / no`` -> ``"off"``, ``running`` -> ``"running"``, anything else or unset -> ``"first"``)."""

    if isinstance(audit, (bool, np.bool_)):
        return "first" if audit else "off"
    if audit is None:
        env = os.environ.get("OPEN_PROVENCE_AUDIT", "1").strip().lower()
        return "off" if env in ("0", "off", "false", "no") else "running" if env == "running" else "first"
    mode = str(audit).strip().lower()
    if mode not in AUDIT_MODES:
        raise ValueError(f"audit must be one of {AUDIT_MODES}, got {audit!r}")
    return mode


def coverage_counts(ids: np.ndarray, cu_seqlens: np.ndarray, covered: np.ndarray) -> np.ndarray:
    """Per row of a packed batch, the positions whose token id is not in ``covered`` (bool ``[vocab]``): what
    ``op_coverage_scan`` writes to ``row_novel_dev``.  Duplicates count once per position; an id outside the table is novel."""

    ids = np.asarray(ids).astype(np.int64, copy=False)
    inside = (ids >= 0) & (ids < covered.shape[0])
    novel = np.ones(ids.shape[0], dtype=bool)
    novel[inside] = ~covered[ids[inside]]
    csum = np.concatenate(([0], np.cumsum(novel, dtype=np.int64)))
    cu = np.asarray(cu_seqlens, dtype=np.int64)
    return (csum[cu[1:]] - csum[cu[:-1]]).astype(np.int32)


def select_audit_rows(row_novel: "Sequence[int]", lengths: "Sequence[int]", budget: int, longest: "int | None" = None) -> list[int]:
    """The rows one running audit re-runs: ``longest`` first (the index of the batch's longest row, given when the length
    trigger fired), then by (novel positions descending, length descending, index ascending) until the next row would take
    the sub-batch past ``budget`` tokens.  At least one row is always taken, whatever its length; no rows give ``[]``."""

    n = len(row_novel)
    if n == 0:
        return []
    order = sorted(range(n), key=lambda i: (-int(row_novel[i]), -int(lengths[i]), i))
    if longest is not None:
        order = [int(longest)] + [i for i in order if i != int(longest)]
    picked, tokens = [], 0
    for i in order:
        if picked and tokens + int(lengths[i]) > int(budget):
            break
        picked.append(i)
        tokens += int(lengths[i])
    return picked


class AuditState:
    """What the audits of one encoder remember: whether the first-real-batch audit is still ``pending``, whether the ``running``
    audit is on, which token ids audited rows have held (``cov_mirror``, bool ``[vocab]``: the host mirror of the handle's
    bitmap), the longest audited row (``cov_max_len``) and the forwards since the last audit (``since_audit``)."""

    def __init__(self, vocab_size: int) -> None:
        self.vocab_size = int(vocab_size)
        self.pending = False
        self.reset(running=False)

    def reset(self, running: bool) -> None:
        """Forget what was audited (a new arithmetic has seen nothing) and switch the running audit on or off."""

        self.running = bool(running)
        self.cov_mirror = np.zeros(self.vocab_size, dtype=bool)
        self.cov_max_len = 0
        self.since_audit = 0

    def plan(self, lengths: np.ndarray, ids_host: "np.ndarray | None", scan: Callable, audit_every: int, audit_tokens: int,
             blocked: bool = False) -> "tuple[str, list[int]] | None":
        """One forward of the running audit: count it, and decide whether it is audited -- ``(trigger, rows to re-run)`` or
        None.  ``blocked`` forwards and batches under 64 tokens only count.  ``"coverage"`` (a position whose id no audited row
        held, or a row longer than any audited row -- that row is then re-run whatever its novelty) comes before ``"every_n"``.
        Coverage is decided on ``ids_host`` against the mirror, or, without it, by ``scan()`` (``coverage_scan_device``)."""

        self.since_audit += 1
        if blocked or int(np.sum(lengths)) < MIN_AUDIT_TOKENS:
            return None
        longest = int(np.argmax(lengths))
        row_novel = None
        if ids_host is not None:
            too_long = int(lengths[longest]) > self.cov_max_len
            if too_long or not self.cov_mirror[ids_host].all():
                row_novel = coverage_counts(ids_host, np.concatenate(([0], np.cumsum(lengths))), self.cov_mirror)
        else:
            novel_dev, report = scan()
            too_long = report["longest"] > report["max_audited"]
            if too_long or report["novel"] > 0:
                row_novel = novel_dev.cpu().numpy()
        trigger = "coverage" if row_novel is not None else None
        if trigger is None and audit_every > 0 and self.since_audit >= audit_every:
            trigger, row_novel = "every_n", np.zeros(len(lengths), dtype=np.int32)
        if trigger is None:
            return None
        return trigger, select_audit_rows(row_novel, lengths, audit_tokens, longest=longest if too_long else None)

    def commit(self, sub_ids_host: np.ndarray, sub_lengths: np.ndarray) -> None:
        """An audit passed: its rows' ids join the coverage and the longest audited length rises (the host mirror's half)."""

        self.cov_mirror[np.asarray(sub_ids_host, dtype=np.int64)] = True
        if len(sub_lengths):
            self.cov_max_len = max(self.cov_max_len, int(np.max(sub_lengths)))

    def record(self, report: "dict | None", trigger: str, rows: "Sequence[int]", tokens: int, err: float, bound: float, passed: bool) -> None:
        """One running audit into ``report["audits"]`` (``report``: the encoder's ``calibration``); the forward count restarts."""

        audits = (report if report is not None else {}).setdefault("audits", {"count": 0, "by_trigger": {}, "last": None})
        audits["count"] += 1
        audits["by_trigger"][trigger] = audits["by_trigger"].get(trigger, 0) + 1
        audits["last"] = {"rows": [int(r) for r in rows], "tokens": int(tokens), "max_abs_err": float(err), "bound": float(bound),
                          "passed": bool(passed), "trigger": trigger}
        self.since_audit = 0


def reference_error(enc, call, rows: "Sequence[int] | None" = None):
    """THE comparison of every audit: ``call``'s batch (or its ``rows``, gathered into a sub-batch) once more on the
    calibration's reference set, against the logits the chosen set wrote into ``call`` -> ``(max |difference|, bound, passed,
    the reference call)``; None when there is nothing to audit (no calibrated set, the default one, or an unknown reference).
    ``bound`` = ``audit_factor`` x the calibration tolerance.  A non-finite logit fails: the whole-batch comparison gives NaN,
    the sub-batch's (``op_audit_compare``) +inf.

    The detour: the reference forward runs with per-kernel profiling suspended (the audit's launches are not the caller's
    workload), and ``chosen`` and its layer mask are pinned again behind it, whatever happens in between.  The running
    audit's coverage stays as it is on both sides: the handle's belongs to the arithmetic it was collected under and is
    looked at again only once ``chosen`` is back."""

    cal = enc.calibration or {}
    chosen, reference = cal.get("chosen_set"), cal.get("reference_set")
    if not chosen or chosen == cal.get("default_set") or reference not in KERNEL_SET_IDS:
        return None
    ref = enc._reference_call(call, rows)
    profiling = enc._profiling
    if profiling:
        enc.profile_enable(False)
    enc._select_kernel_set(reference)
    try:
        enc._forward_native(ref)
    finally:
        enc._repin_calibrated(chosen)
        if profiling:
            enc.profile_enable(True)
    err = float(enc._logit_error(call, ref))  # (synchronises: the one float an audit reads back)
    bound = float(cal.get("tolerance", DEFAULT_CALIBRATION_TOLERANCE)) * float(enc.audit_factor)
    return err, bound, bool(err <= bound), ref


def first_batch_audit(enc, call, collective: bool = False) -> "bool | None":
    """The calibration ran on synthetic token ids; the FIRST real batch a calibrated model sees is its audit: the same
    batch once more through the reference kernel set of the calibration, max |logit difference| against what the chosen
    set just returned.  Within ``audit_factor`` (3) x the calibration tolerance -- 3e-4, still 3 x inside the path's bar;
    the forward fuzz puts the worst row of other inputs at <= 2.7 x a calibration batch's maximum -- the choice stands
    (one synchronisation, two extra forwards, once per load).  Beyond it, or non-finite: the model goes back to the
    default selection of ``op_weights_ready`` for good, warns, and THIS batch is recomputed there before it is returned
    (with the caller's hidden-state request: the reference forward of the audit itself writes none).  ``collective``: only
    measure -- the ranks of a process group revert together or not at all (``sharding.collective_audit``).
    Returns the verdict (None: there was nothing to audit)."""

    enc.audit_state.pending = False
    result = reference_error(enc, call)
    if result is None:
        return None
    err, bound, passed, _ = result
    cal = enc.calibration
    cal["audit"] = {"tokens": int(call.total), "rows": int(call.n_seqs), "max_abs_err": err, "bound": bound, "passed": passed}
    if collective:
        cal["audit"]["collective"] = True
    elif not passed:  # (stacklevel: the caller of forward_packed, six frames above revert_to_default's warn)
        enc.revert_to_default("", stacklevel=6, recompute=call, warning=(
            f"open_provence_amd: the first real batch disagrees with the load-time calibration: kernel set {cal['chosen_set']!r} is "
            f"{err:.2e} from the {cal['reference_set']!r} kernels on it (bound {bound:.1e}); this model runs on " "{after!r} from now on.  "
            "Pass calibration_rows= (a sample of real token ids) to calibrate on representative inputs."))
    return passed


def _commit_audited(enc, audited) -> None:
    """Every row of ``audited`` passed an audit: into the coverage, on the host and in the handle's bitmap."""

    ids_host = audited.ids_host if audited.ids_host is not None else audited.ids.cpu().numpy()
    enc.audit_state.commit(ids_host, np.diff(audited.cu_host))
    enc._commit_coverage(audited)


def running_audit(enc, call, trigger: str, rows: "Sequence[int]") -> None:
    """One running audit: ``rows`` of the batch gathered into a sub-batch on the device (``op_gather_rows``), run on the
    calibration's reference set, compared on the device with the logits the chosen set just wrote for those rows
    (``op_audit_compare``; per-row outputs do not depend on the batch's composition, so the comparison is exact), one
    float read back.  Within ``audit_factor`` x the calibration tolerance: the rows' ids join the coverage.  Beyond it,
    or non-finite: what a failed first-batch audit does -- ``revert_to_default``, one ``RuntimeWarning``, and THIS
    batch recomputed there (with the caller's hidden-state request) before it is returned."""

    result = reference_error(enc, call, rows)
    if result is None:
        return
    err, bound, passed, sub = result
    enc.audit_state.record(enc.calibration, trigger, rows, sub.total, err, bound, passed)
    if passed:
        _commit_audited(enc, sub)
        return
    enc.revert_to_default(f"running audit ({trigger}): {err:.2e} from the {enc.calibration['reference_set']!r} kernels on rows "
                          f"{list(rows)[:8]} of a batch, bound {bound:.1e}", stacklevel=6, recompute=call)


def maybe_audit(enc, call, running: bool) -> None:
    """The audits of a calibrated kernel set, from EITHER forward entry point (``forward_packed`` / ``forward_packed_on``).

    The first-real-batch audit of a synthetically calibrated set (modes ``"first"`` and ``"running"``) is skipped -- and left
    pending -- for batches under 64 tokens, while hidden states are captured (the debug hook; a per-call request is
    audited like any batch), and while the stream is being captured into a hipGraph (the audit synchronises and switches
    the handle's kernel set in the middle of the forward).

    The RUNNING audit (mode ``"running"``, a calibrated set that is not the default one) re-checks later forwards when a
    trigger fires: ``audit_every`` forwards have passed since the last audit (0 = never), or the batch holds positions
    whose token id was in no audited row so far, or a row longer than any audited row (``"coverage"``).  Coverage is
    decided where the ids are: on ``ids_host`` in numpy against a host mirror of the handle's bitmap -- a forward that
    does not audit then synchronises nothing -- or, without it, by ``op_coverage_scan`` (one small kernel and one
    synchronisation per forward): :meth:`AuditState.plan`.  An audit re-runs up to ``audit_tokens`` tokens of the batch
    (:func:`select_audit_rows`) on the reference set and compares on the device (:func:`running_audit`).  It is skipped -- the
    forward counts towards ``audit_every`` all the same -- for batches under 64 tokens, under a debug hidden capture, on a
    capturing stream, from ``forward_packed_on`` (the pipelined path), and on an encoder with ``audit_collective`` set: a process
    group keeps its collective first-batch audit, and a collective running audit is future work."""

    state = enc.audit_state
    running = bool(running and state.running)
    if not state.pending and not running:
        return
    blocked = call.total < MIN_AUDIT_TOKENS or enc._audit_blocked()
    if not state.pending:
        planned = state.plan(np.diff(call.cu_host), call.ids_host,
                             lambda: enc.coverage_scan_device(call.ids, call.cu_seqlens, call.n_seqs, call.total),
                             enc.audit_every, enc.audit_tokens, blocked=blocked)
        if planned is not None:
            running_audit(enc, call, *planned)
        return
    if running:
        state.since_audit += 1
    if blocked:
        return
    verdict = first_batch_audit(enc, call)
    if running and verdict is not None:
        # in running mode the first batch is the first running audit too: every row of it was just audited
        first = enc.calibration["audit"]
        state.record(enc.calibration, "coverage", range(call.n_seqs), call.total, first["max_abs_err"], first["bound"], verdict)
        if verdict:
            _commit_audited(enc, call)
