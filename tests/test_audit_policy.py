"""The audit of a calibrated kernel set as a decision, on the host: ``audit.maybe_audit`` and ``AuditState`` driven with a fake in
place of the encoder.  The fake records which rows a reference forward was requested for and answers with a scripted error;
vocab 32 and batches of 3 to 5 rows, 4 to 130 tokens long, are the smallest that still show the 64-token floor and a row
"longer than any audited row".  What runs on the device is covered by tests/test_gpu_running_audit.py."""

import numpy as np
import pytest
import torch

from open_provence_amd.audit import AuditState, coverage_counts, maybe_audit
from open_provence_amd.engine import PackedCall

VOCAB = 32
FIRST_KEYS = {"tokens", "rows", "max_abs_err", "bound", "passed"}


def _call(rows, host=True):
    ids = np.concatenate([np.asarray(r, dtype=np.int32) for r in rows])
    cu = np.concatenate(([0], np.cumsum([len(r) for r in rows]))).astype(np.int32)
    return PackedCall(torch.from_numpy(ids), torch.from_numpy(cu), cu, len(rows), int(cu[-1]), max(len(r) for r in rows),
                      None, None, None, None, 0, None, ids if host else None)


def _row(length, ids=range(20), shift=0):
    ids = list(ids)
    return [ids[(shift + i) % len(ids)] for i in range(length)]


class FakeEncoder:
    """The device side of audit.py, recorded: ``log`` holds ("reference", rows | None), ("select", set), ("repin", set),
    ("profile", on), ("commit", n_rows), ("revert", reason, warning, recompute) in the order they happened."""

    def __init__(self, pending=False, running=True, errors=(), audit_every=0, audit_tokens=8192):
        self.calibration = {"tolerance": 1e-4, "chosen_set": "f16", "reference_set": "bf16x3", "default_set": "bf16x3"}
        self.audit_state = AuditState(VOCAB)
        self.audit_state.pending = pending
        self.audit_state.reset(running)
        self.audit_factor, self.audit_every, self.audit_tokens, self._profiling = 3.0, audit_every, audit_tokens, False
        self.errors, self.log, self.scans, self.blocked, self.raise_in_forward = list(errors), [], 0, False, None
        self.bitmap = np.zeros(VOCAB, dtype=bool)  # (the handle's coverage, as op_coverage_commit / op_coverage_scan keep it)
        self.bitmap_max_len = 0

    def references(self):
        return [entry[1] for entry in self.log if entry[0] == "reference"]

    def _audit_blocked(self):
        return self.blocked

    def _reference_call(self, call, rows=None):
        self.log.append(("reference", None if rows is None else list(rows)))
        if rows is None:
            return call
        ids = call.ids.numpy()
        return _call([ids[call.cu_host[r]: call.cu_host[r + 1]] for r in rows], host=call.ids_host is not None)

    def _forward_native(self, call):
        if self.raise_in_forward is not None:
            raise self.raise_in_forward

    def _logit_error(self, call, ref):
        return self.errors.pop(0) if self.errors else 5e-5

    def _select_kernel_set(self, name):
        self.log.append(("select", name))

    def _repin_calibrated(self, chosen):
        self.log.append(("repin", chosen))

    def profile_enable(self, enabled):
        self._profiling = bool(enabled)
        self.log.append(("profile", bool(enabled)))

    def coverage_scan_device(self, ids, cu_seqlens, n_seqs, total):
        self.scans += 1
        lengths = np.diff(cu_seqlens.numpy())
        novel = coverage_counts(ids.numpy(), cu_seqlens.numpy(), self.bitmap)
        return torch.from_numpy(novel), {"novel": int(novel.sum()), "longest": int(lengths.max()), "longest_row": int(lengths.argmax()),
                                         "max_audited": self.bitmap_max_len}

    def _commit_coverage(self, call):
        self.log.append(("commit", call.n_seqs))
        self.bitmap[call.ids.numpy()] = True
        self.bitmap_max_len = max(self.bitmap_max_len, int(np.diff(call.cu_host).max()))

    def revert_to_default(self, reason, *, warning=None, stacklevel=3, recompute=None):
        self.log.append(("revert", reason, warning, recompute))
        self.audit_state.pending = False  # (what select_kernel_set("auto") does)
        self.audit_state.reset(running=False)
        self.calibration["chosen_set"] = self.calibration["default_set"]


def _audits(enc):
    return enc.calibration["audits"]


def _primed(**kw):
    """A running-mode encoder whose first batch -- ids 0 .. 19, rows of at most 64 tokens -- has passed its audit."""

    enc = FakeEncoder(pending=True, **kw)
    maybe_audit(enc, _call([_row(4), _row(64, shift=3), _row(30, shift=7)]), running=True)
    assert _audits(enc)["count"] == 1 and enc.audit_state.cov_max_len == 64 and not enc.audit_state.pending
    return enc


def test_the_first_batch_in_running_mode_audits_every_row_and_commits_it():
    enc = FakeEncoder(pending=True)
    batch = _call([_row(4), _row(70, shift=3), _row(30, shift=7)])
    maybe_audit(enc, batch, running=True)
    state = enc.audit_state
    assert enc.references() == [None]  # (the whole batch)
    assert set(enc.calibration["audit"]) == FIRST_KEYS and enc.calibration["audit"]["passed"] is True
    assert enc.calibration["audit"]["tokens"] == 104 and enc.calibration["audit"]["rows"] == 3
    assert enc.calibration["audit"]["bound"] == pytest.approx(3e-4)
    audits = _audits(enc)
    assert audits["count"] == 1 and audits["by_trigger"] == {"coverage": 1}
    assert audits["last"] == {"rows": [0, 1, 2], "tokens": 104, "max_abs_err": 5e-5, "bound": pytest.approx(3e-4), "passed": True,
                              "trigger": "coverage"}
    assert not state.pending and state.cov_max_len == 70 and state.since_audit == 0
    assert np.flatnonzero(state.cov_mirror).tolist() == list(range(20)) and ("commit", 3) in enc.log
    # the same batch again holds nothing new
    maybe_audit(enc, batch, running=True)
    assert enc.references() == [None] and _audits(enc)["count"] == 1
    assert state.plan(np.diff(batch.cu_host), batch.ids_host, None, 0, 8192) is None
    # mode "first": the same audit, no running record, nothing committed
    first = FakeEncoder(pending=True, running=False)
    maybe_audit(first, batch, running=True)
    assert first.references() == [None] and "audits" not in first.calibration and not first.audit_state.cov_mirror.any()
    assert not first.audit_state.pending and first.audit_state.since_audit == 0


def test_known_ids_in_a_longer_row_trigger_coverage_and_that_row_is_taken():
    enc = _primed(audit_tokens=200)
    batch = _call([_row(64), _row(40, shift=5), _row(130, shift=2), _row(64, shift=9)])  # ids 0 .. 19 only: no novelty
    maybe_audit(enc, batch, running=True)
    last = _audits(enc)["last"]
    # the 130-token row first although its novelty is 0; 200 tokens then leave room for one 64-token row
    assert last["trigger"] == "coverage" and last["rows"] == [2, 0] and last["tokens"] == 194 and last["passed"]
    assert enc.references()[-1] == [2, 0] and enc.audit_state.cov_max_len == 130
    maybe_audit(enc, batch, running=True)
    assert _audits(enc)["count"] == 2 and len(enc.references()) == 2


def test_one_unseen_id_selects_its_row_first_and_a_small_budget_selects_it_alone():
    enc = _primed()
    rows = [_row(40), _row(50, shift=4), _row(30, shift=8)]
    rows[2][11] = 31  # the one id no audited row held
    state = enc.audit_state
    planned = state.plan(np.diff(_call(rows).cu_host), _call(rows).ids_host, None, 0, 8192)
    assert planned == ("coverage", [2, 1, 0])
    assert state.plan(np.diff(_call(rows).cu_host), _call(rows).ids_host, None, 0, 29) == ("coverage", [2])
    enc.audit_tokens = 29
    maybe_audit(enc, _call(rows), running=True)
    assert enc.references()[-1] == [2] and _audits(enc)["last"]["tokens"] == 30 and state.cov_mirror[31]


def test_audit_every_counts_forwards_and_coverage_takes_precedence():
    enc = _primed(audit_every=2)
    batch = _call([_row(30), _row(64, shift=1), _row(10, shift=2)])
    counts = []
    for _ in range(5):
        maybe_audit(enc, batch, running=True)
        counts.append(_audits(enc)["count"])
    assert counts == [1, 2, 2, 3, 3]  # (1 = the first batch) forwards 2 and 4
    assert _audits(enc)["by_trigger"] == {"coverage": 1, "every_n": 2} and _audits(enc)["last"]["rows"] == [1, 0, 2]
    assert enc.audit_state.since_audit == 1
    novel = _call([_row(30), _row(64, ids=[25]), _row(10)])
    maybe_audit(enc, novel, running=True)  # forward 6: both triggers fire
    assert _audits(enc)["last"]["trigger"] == "coverage" and _audits(enc)["last"]["rows"][0] == 1
    assert _audits(enc)["by_trigger"] == {"coverage": 2, "every_n": 2} and enc.audit_state.since_audit == 0
    # audit_every = 0: never
    never = _primed()
    for _ in range(4):
        maybe_audit(never, batch, running=True)
    assert _audits(never)["count"] == 1 and never.audit_state.since_audit == 4


def test_a_batch_under_64_tokens_plans_nothing_but_counts():
    small = _call([_row(4, ids=[30]), _row(29, ids=[31]), _row(30, ids=[29])])  # 63 tokens, all of them new
    enc = FakeEncoder(pending=True)
    maybe_audit(enc, small, running=True)
    assert enc.log == [] and enc.audit_state.pending and enc.audit_state.since_audit == 1
    enc = _primed(audit_every=2)
    maybe_audit(enc, small, running=True)
    maybe_audit(enc, small, running=True)
    assert enc.audit_state.since_audit == 2 and _audits(enc)["count"] == 1 and len(enc.references()) == 1
    maybe_audit(enc, _call([_row(64)]), running=True)  # the skipped forwards counted: this one is due
    assert _audits(enc)["last"]["trigger"] == "every_n"
    # a blocked forward (hidden capture, collective audit, capturing stream) and the pipelined path: the same
    enc = FakeEncoder(pending=True)
    enc.blocked = True
    maybe_audit(enc, _call([_row(70)]), running=True)
    assert enc.log == [] and enc.audit_state.pending and enc.audit_state.since_audit == 1
    maybe_audit(enc, _call([_row(70)]), running=False)
    assert enc.audit_state.since_audit == 1


def test_the_scan_is_used_only_without_host_ids_and_decides_the_same():
    batches = [[_row(64), _row(40, shift=5), _row(130, shift=2)],  # a longer row
               [_row(40), _row(50, ids=[3, 4, 27]), _row(30, ids=[28])],  # new ids
               [_row(40), _row(50, shift=4), _row(30, shift=8)]]  # nothing new
    on_host, on_device = _primed(audit_every=3, audit_tokens=150), _primed(audit_every=3, audit_tokens=150)
    assert on_device.scans == 0  # (the first batch is audited whole: nothing to scan)
    for n, rows in enumerate(batches, start=1):
        maybe_audit(on_host, _call(rows), running=True)
        maybe_audit(on_device, _call(rows, host=False), running=True)
        assert on_host.scans == 0 and on_device.scans == n
        assert on_host.references() == on_device.references() and _audits(on_host) == _audits(on_device)
        assert np.array_equal(on_host.audit_state.cov_mirror, on_device.audit_state.cov_mirror)
    assert _audits(on_host)["by_trigger"] == {"coverage": 3} and on_host.references()[1:] == [[2], [2, 1, 0]]
    # plan() itself: the report of a scan against the same coverage gives the same answer as the host ids
    state, call = on_host.audit_state, _call([_row(20), _row(131, ids=[3, 30]), _row(9)])
    scan = lambda: on_host.coverage_scan_device(call.ids, call.cu_seqlens, call.n_seqs, call.total)  # noqa: E731
    by_scan = state.plan(np.diff(call.cu_host), None, scan, 0, 8192)
    assert by_scan == state.plan(np.diff(call.cu_host), call.ids_host, None, 0, 8192) == ("coverage", [1, 0, 2])
    assert on_host.scans == 1


def test_reset_clears_the_state_and_a_failed_audit_commits_nothing():
    enc = _primed(errors=[5e-5, 1.0])
    state = enc.audit_state
    before = state.cov_mirror.copy()
    batch = _call([_row(40), _row(70, ids=[30, 31]), _row(30)])
    maybe_audit(enc, batch, running=True)
    last = _audits(enc)["last"]
    assert last["passed"] is False and last["trigger"] == "coverage" and last["rows"][0] == 1 and last["max_abs_err"] == 1.0
    kind, reason, warning, recompute = enc.log[-1]
    assert kind == "revert" and reason.startswith("running audit (coverage): 1.00e+00 from the 'bf16x3' kernels on rows [1, ")
    assert warning is None and recompute is batch and [e for e in enc.log if e[0] == "commit"] == [("commit", 3)]  # (the first batch's)
    assert not before[[30, 31]].any() and not state.cov_mirror.any() and not state.running  # (the revert reset the state)
    # a failed first batch: the first-batch sentence, no running commit, THIS call recomputed
    enc = FakeEncoder(pending=True, errors=[float("nan")])
    maybe_audit(enc, batch, running=True)
    kind, reason, warning, recompute = enc.log[-1]
    assert kind == "revert" and "disagrees with the load-time calibration" in warning and "{after!r}" in warning and recompute is batch
    assert set(enc.calibration["audit"]) == FIRST_KEYS and enc.calibration["audit"]["passed"] is False
    assert _audits(enc)["last"]["passed"] is False and not enc.audit_state.cov_mirror.any() and not any(e[0] == "commit" for e in enc.log)
    # reset()
    state = _primed().audit_state
    state.since_audit = 3
    state.reset(running=False)
    assert not state.running and not state.cov_mirror.any() and state.cov_max_len == 0 and state.since_audit == 0


@pytest.mark.parametrize("first", [True, False])
def test_an_exception_in_the_reference_forward_pins_the_chosen_set_again(first):
    """The reference forward raises: the calibrated set (``_repin_calibrated``: the set and its layer mask) is pinned again and
    profiling is back on.  The pending flag is cleared BEFORE the forward, as it always was: a first-batch audit that raised
    is not tried again.  Nothing is recorded or committed."""

    enc = FakeEncoder(pending=True) if first else _primed()
    enc.log.clear()
    enc._profiling = True
    enc.raise_in_forward = RuntimeError("op_forward_packed failed")
    with pytest.raises(RuntimeError, match="op_forward_packed failed"):
        maybe_audit(enc, _call([_row(70, ids=[30]), _row(10), _row(12)]), running=True)
    rows = None if first else [0, 2, 1]
    assert enc.log == [("reference", rows), ("profile", False), ("select", "bf16x3"), ("repin", "f16"), ("profile", True)]
    assert enc._profiling and not enc.audit_state.pending and enc.calibration["chosen_set"] == "f16"
    assert "audits" not in enc.calibration if first else _audits(enc)["count"] == 1
    assert first or "audit" in enc.calibration  # (the primed encoder's passed first batch; the raising one wrote no report)
    assert not first or "audit" not in enc.calibration
