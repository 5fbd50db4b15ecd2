"""The running audit of a calibrated kernel set on the GPU (``HipEncoder(audit="running")``).

* the kernels -- ``op_coverage_scan`` / ``op_coverage_commit`` / ``op_gather_rows`` / ``op_audit_compare`` -- against numpy /
  torch, exact equality (integers, and an fp32 maximum that does not depend on the order);
* the two triggers (every N forwards, coverage: unseen token ids or a longer row) and their bookkeeping;
* the test that fails without the feature: a batch with a token the calibration never saw drifts past the audit bound on
  "f16" with FINITE outputs (tests/test_running_audit_host.py shows why, on the float64 model) -- an ``audit="first"``
  encoder returns it, an ``audit="running"`` encoder catches it, goes back to the default set and returns that set's answer;
* device-resident ``forward()`` (no host ids: the scan path) and ``process()``.

Shape: xsmall cut to 3 layers (global, local, local), vocab 500, rows of at most 130 tokens."""

import ctypes
import warnings

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
EDGE_IDS = (0, 31, 32, 63, 499)  # word boundaries of the bitmap and the last id of a vocabulary that is no multiple of 32


def _dims():
    from open_provence_amd.synthetic import named_dims

    return named_dims("xsmall", num_layers=3, vocab_size=500)


@pytest.fixture(scope="module")
def fixture():
    """Weights with the planted token, the benign rows, and the batches the policy tests run."""

    from open_provence_amd.synthetic import outlier_token_rows, outlier_token_state_dict

    dims = _dims()
    benign, outlier = outlier_token_rows()
    short = benign[:5]  # 3, 17, 40, 63, 64 tokens: 187 in all
    seen = [t for row in short for t in row]
    long_row = (seen * 2)[40: 170]  # 130 tokens, every id of which the short rows hold: only its LENGTH is new
    return {"dims": dims, "state": outlier_token_state_dict(dims), "benign": benign, "short": short,
            "with_long_row": short[:2] + [long_row] + short[2:], "with_outlier": [short[3], short[4], outlier, short[2]]}


def _encoder(fx, audit, **kwargs):
    from open_provence_amd.engine import HipEncoder

    calibrate = kwargs.pop("calibrate", True)
    enc = HipEncoder(fx["dims"], device=DEV, precision="bf16x3", flags=0, audit=audit, **kwargs)
    with warnings.catch_warnings():
        warnings.simplefilter("error", RuntimeWarning)  # (loading and calibrating on the benign rows drops no kernel set)
        enc.load_state_dict(fx["state"], calibrate=calibrate, calibration_rows=fx["benign"] if calibrate else None)
    if calibrate:
        cal = enc.calibration
        assert cal["chosen_set"] == "f16" == enc.effective_policy()["kernel_set"], cal  # the headline case
        assert cal["reference_set"] == "bf16x3" and cal["default_set"] != "f16", cal
    return enc


def _run(enc, rows):
    prune, rank, _ = enc.forward_rows(rows)
    return prune.cpu().numpy(), rank.cpu().numpy()


def _audits(enc):
    return (enc.calibration or {}).get("audits") or {"count": 0, "by_trigger": {}, "last": None}


# -- the kernels ---------------------------------------------------------------------------------------------------------------
def _i32(values):
    return torch.tensor(np.asarray(values, dtype=np.int32), dtype=torch.int32, device=DEV)


def _vp(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None and t.numel() else None


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream(torch.device(DEV)).cuda_stream)


def _scan(enc, ids, cu):
    from open_provence_amd import _lib

    n_seqs, total = int(cu.numel()) - 1, int(ids.numel())
    novel = torch.full((max(n_seqs, 1),), -7, dtype=torch.int32, device=DEV)
    report = _lib.OpCoverageReport()
    report.struct_bytes = ctypes.sizeof(_lib.OpCoverageReport)
    code = enc.lib.op_coverage_scan(enc._handle, _vp(ids), _vp(cu), n_seqs, total, _vp(novel), ctypes.byref(report), _stream())
    assert code == 0, _lib.last_error(enc.lib, enc._handle)
    return novel[:n_seqs].cpu().numpy(), report


def _commit(enc, ids, cu, rows):
    code = enc.lib.op_coverage_commit(enc._handle, _vp(ids), _vp(cu), int(cu.numel()) - 1, int(ids.numel()), _vp(_i32(rows)), len(rows),
                                      _stream())
    assert code == 0


def _kernel_batches():
    rng = np.random.default_rng(17)
    pool = np.array(EDGE_IDS + (1, 30, 33, 62, 64, 250, 498), dtype=np.int32)

    def rows(lengths):
        out = [rng.choice(pool, size=n).astype(np.int32) for n in lengths]
        for r in out:
            if len(r) >= 3:
                r[1] = r[2] = r[0]  # duplicates inside a row
        return out

    many = rng.integers(20, 131, size=40).tolist()
    many[7] = 130
    assert sum(many) > 2048  # more than one block of every kernel
    return {"one-token": [np.array([499], dtype=np.int32)], "edges": rows([1, 63, 64, 65, 130]), "forty-rows": rows(many)}


@pytest.fixture(scope="module")
def plain_encoder(fixture):
    return _encoder(fixture, "first", calibrate=False)


@pytest.mark.parametrize("name", ["one-token", "edges", "forty-rows"])
def test_scan_commit_and_gather_equal_numpy(plain_encoder, name):
    from open_provence_amd.engine import coverage_counts

    enc, rows = plain_encoder, _kernel_batches()[name]
    lengths = np.array([len(r) for r in rows])
    cu_np = np.concatenate(([0], np.cumsum(lengths))).astype(np.int32)
    ids_np = np.concatenate(rows)
    ids, cu = _i32(ids_np), _i32(cu_np)
    assert enc.lib.op_coverage_reset(enc._handle) == 0
    covered = np.zeros(500, dtype=bool)

    novel, report = _scan(enc, ids, cu)  # nothing audited yet: every position is novel
    assert novel.tolist() == lengths.tolist()
    assert (report.novel_tokens, report.longest_row_tokens, report.longest_row, report.max_audited_tokens) == \
        (int(lengths.sum()), int(lengths.max()), int(lengths.argmax()), 0)

    listed = list(range(0, len(rows), 2))  # every other row, the first included
    _commit(enc, ids, cu, listed)
    for r in listed:
        covered[rows[r]] = True
    novel, report = _scan(enc, ids, cu)
    assert novel.tolist() == coverage_counts(ids_np, cu_np, covered).tolist()
    assert report.novel_tokens == int(novel.sum()) and report.max_audited_tokens == int(lengths[listed].max())
    assert (report.longest_row_tokens, report.longest_row) == (int(lengths.max()), int(lengths.argmax()))
    novel_again, _ = _scan(enc, ids, cu)  # the scan is read-only
    assert novel_again.tolist() == novel.tolist()

    # ids outside the table count as novel and are never an index; a listed row that is no row of the batch is skipped
    wild = _i32([0, -1, 500, 2**31 - 1, 499])
    _commit(enc, ids, cu, [-1, len(rows), 2**31 - 1])
    assert _scan(enc, ids, cu)[0].tolist() == novel.tolist()
    got, _ = _scan(enc, wild, _i32([0, 5]))
    assert got.tolist() == [5 - int(covered[0]) - int(covered[499])]

    # gather: the listed rows end to end, in the order listed, with their prefix offsets
    order = list(reversed(listed)) + [0]
    sub_ids = torch.full((int(lengths[order].sum()),), -1, dtype=torch.int32, device=DEV)
    sub_cu = torch.full((len(order) + 1,), -1, dtype=torch.int32, device=DEV)
    def gather(listed_rows):
        code = enc.lib.op_gather_rows(enc._handle, _vp(ids), _vp(cu), len(rows), int(ids.numel()), _vp(_i32(listed_rows)), len(listed_rows),
                                      _vp(sub_ids), _vp(sub_cu), _stream())
        assert code == 0
        return sub_ids.cpu().numpy().tolist(), sub_cu.cpu().numpy().tolist()

    got_ids, got_cu = gather(order)
    assert got_ids == np.concatenate([rows[r] for r in order]).tolist()
    assert got_cu == np.concatenate(([0], np.cumsum(lengths[order]))).tolist()
    # a listed row that is no row of the batch is an empty row of the sub-batch
    strays = [len(rows) if len(order) % 2 else -1] + order[:-1]  # (as many entries as sub_cu has room for)
    got_ids, got_cu = gather(strays)
    assert got_cu == np.concatenate(([0, 0], np.cumsum(lengths[order[:-1]]))).tolist()
    assert got_ids[: got_cu[-1]] == np.concatenate([rows[r] for r in order[:-1]]).tolist()

    # a detour through another kernel set and back keeps the coverage (what an audit does); looking at it under another
    # set, and the explicit reset, empty it
    default_set = enc.effective_policy()["kernel_set"]
    enc._select_kernel_set("bf16x3")
    enc._select_kernel_set("auto")
    assert enc.effective_policy()["kernel_set"] == default_set != "bf16x3"
    assert _scan(enc, ids, cu)[0].tolist() == novel.tolist()
    for forget in (lambda: enc.lib.op_coverage_reset(enc._handle), lambda: enc._select_kernel_set("bf16x3"), lambda: enc.select_kernel_set("auto")):
        _commit(enc, ids, cu, [0])
        forget()
        fresh, report = _scan(enc, ids, cu)
        assert fresh.tolist() == lengths.tolist() and report.max_audited_tokens == 0


def test_compare_is_the_exact_maximum_and_infinite_on_a_non_finite_value(plain_encoder):
    enc = plain_encoder
    rng = np.random.default_rng(23)
    lengths = np.array([5, 130, 1, 64, 77, 65])
    cu_np = np.concatenate(([0], np.cumsum(lengths))).astype(np.int32)
    prune = torch.from_numpy(rng.standard_normal((int(cu_np[-1]), 2)).astype(np.float32)).to(DEV)
    rank = torch.from_numpy(rng.standard_normal((len(lengths), 1)).astype(np.float32)).to(DEV)
    cu = _i32(cu_np)

    def compare(rows, sub_prune, sub_rank):
        sub_cu = _i32(np.concatenate(([0], np.cumsum(lengths[rows]))))
        err = torch.full((1,), -3.0, dtype=torch.float32, device=DEV)  # (the call initialises the cell)
        code = enc.lib.op_audit_compare(enc._handle, _vp(prune), _vp(rank), _vp(cu), len(lengths), int(cu_np[-1]), _vp(_i32(rows)), len(rows),
                                        _vp(sub_prune), _vp(sub_rank), _vp(sub_cu), _vp(err), _stream())
        assert code == 0
        return float(err.item())

    def sub_of(rows):
        sub_prune = torch.cat([prune[cu_np[r]: cu_np[r + 1]] for r in rows]).clone()
        sub_rank = rank[rows].clone()
        sub_prune += torch.from_numpy(rng.standard_normal(tuple(sub_prune.shape)).astype(np.float32) * 1e-3).to(DEV)
        sub_rank += torch.from_numpy(rng.standard_normal(tuple(sub_rank.shape)).astype(np.float32) * 1e-3).to(DEV)
        return sub_prune, sub_rank

    def expected(rows, sub_prune, sub_rank):
        full = torch.cat([prune[cu_np[r]: cu_np[r + 1]] for r in rows])
        return float(torch.maximum((full - sub_prune).abs().max(), (rank[rows] - sub_rank).abs().max()).item())

    for rows in ([4, 1, 3], [1], [2], [0, 1, 2, 3, 4, 5]):
        sub_prune, sub_rank = sub_of(rows)
        assert compare(rows, sub_prune, sub_rank) == expected(rows, sub_prune, sub_rank), rows
    rows = [4, 1, 3]
    sub_prune, sub_rank = sub_of(rows)
    sub_rank[1, 0] += 0.5  # the maximum sits in a ranking logit
    assert compare(rows, sub_prune, sub_rank) == expected(rows, sub_prune, sub_rank) > 0.4
    exact_prune, exact_rank = torch.cat([prune[cu_np[r]: cu_np[r + 1]] for r in rows]).clone(), rank[rows].clone()
    assert compare(rows, exact_prune, exact_rank) == 0.0
    for value in (float("nan"), float("inf"), float("-inf")):
        for side in ("sub_prune", "sub_rank"):
            sub_prune, sub_rank = sub_of(rows)
            (sub_prune if side == "sub_prune" else sub_rank).view(-1)[-1] = value
            assert compare(rows, sub_prune, sub_rank) == float("inf"), (value, side)
    # a non-finite value in a row that is NOT listed does not count
    keep = prune[cu_np[5]].clone()
    prune[cu_np[5]] = float("nan")
    sub_prune, sub_rank = sub_of(rows)
    assert compare(rows, sub_prune, sub_rank) == expected(rows, sub_prune, sub_rank)
    assert compare([5], *sub_of([5])) == float("inf")
    prune[cu_np[5]] = keep
    # a listed row that is no row of the batch cannot be compared: +inf, and nothing is read for it
    sub_prune, sub_rank = sub_of([1])
    sub_cu_one = _i32([0, int(lengths[1])])
    for stray in (-1, len(lengths)):
        err = torch.zeros(1, dtype=torch.float32, device=DEV)
        assert enc.lib.op_audit_compare(enc._handle, _vp(prune), _vp(rank), _vp(cu), len(lengths), int(cu_np[-1]), _vp(_i32([stray])), 1,
                                        _vp(sub_prune), _vp(sub_rank), _vp(sub_cu_one), _vp(err), _stream()) == 0
        assert float(err.item()) == float("inf")


def test_argument_errors_are_refused_before_anything_is_enqueued(plain_encoder):
    from open_provence_amd import _lib

    enc = plain_encoder
    buf = _i32([0, 1, 2, 3])
    err = torch.full((1,), 5.0, dtype=torch.float32, device=DEV)
    report = _lib.OpCoverageReport()
    report.struct_bytes = 4
    h, vp = enc._handle, _vp
    assert enc.lib.op_coverage_scan(h, vp(buf), vp(buf), 1, 4, vp(buf), ctypes.byref(report), _stream()) == _lib.OP_ERR_INVALID
    assert enc.lib.op_coverage_scan(h, vp(buf), vp(buf), 1, 4, vp(buf), None, _stream()) == _lib.OP_ERR_INVALID
    assert enc.lib.op_coverage_commit(h, vp(buf), vp(buf), 1, 4, None, 1, _stream()) == _lib.OP_ERR_INVALID
    assert enc.lib.op_coverage_commit(h, vp(buf), vp(buf), 1, 4, vp(buf), -1, _stream()) == _lib.OP_ERR_INVALID
    assert enc.lib.op_coverage_commit(h, vp(buf), vp(buf), -1, 4, vp(buf), 1, _stream()) == _lib.OP_ERR_INVALID
    assert enc.lib.op_gather_rows(h, vp(buf), vp(buf), 1, 4, vp(buf), 1, vp(buf), None, _stream()) == _lib.OP_ERR_INVALID
    assert enc.lib.op_gather_rows(h, vp(buf), vp(buf), 1, 4, vp(buf), -1, vp(buf), vp(buf), _stream()) == _lib.OP_ERR_INVALID
    assert enc.lib.op_gather_rows(h, vp(buf), vp(buf), 1, -4, vp(buf), 1, vp(buf), vp(buf), _stream()) == _lib.OP_ERR_INVALID
    assert enc.lib.op_audit_compare(h, vp(err), vp(err), vp(buf), 1, 4, vp(buf), 1, vp(err), None, vp(buf), vp(err), _stream()) == _lib.OP_ERR_INVALID
    assert enc.lib.op_audit_compare(h, vp(err), vp(err), vp(buf), 1, 4, vp(buf), 1, vp(err), vp(err), vp(buf), None, _stream()) == _lib.OP_ERR_INVALID
    assert "err_dev" in _lib.last_error(enc.lib, h)
    torch.cuda.synchronize()
    assert buf.cpu().tolist() == [0, 1, 2, 3] and float(err.item()) == 5.0  # nothing ran


# -- the policy ------------------------------------------------------------------------------------------------------------------
def test_every_n_audits_at_the_expected_forwards_and_changes_no_output(fixture):
    first = _encoder(fixture, "first")
    running = _encoder(fixture, "running", audit_every=2)
    want = _run(first, fixture["short"])
    counts = []
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        for _ in range(5):
            got = _run(running, fixture["short"])
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
            counts.append(_audits(running)["count"])
    # forward 1: everything is new (coverage); then every second forward
    assert counts == [1, 1, 2, 2, 3], counts
    audits = _audits(running)
    assert audits["by_trigger"] == {"coverage": 1, "every_n": 2}
    last = audits["last"]
    assert last["trigger"] == "every_n" and last["passed"] and last["max_abs_err"] <= last["bound"] == pytest.approx(3e-4)
    assert last["tokens"] == sum(len(r) for r in fixture["short"]) and sorted(last["rows"]) == [0, 1, 2, 3, 4]
    assert running.effective_policy()["kernel_set"] == "f16" and "audits" not in (first.calibration or {})


def test_coverage_fires_on_new_ids_and_on_a_longer_row_only(fixture):
    running = _encoder(fixture, "running", audit_tokens=200)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        _run(running, fixture["short"])
        _run(running, fixture["short"])
        assert _audits(running)["count"] == 1  # the second run holds nothing new
        assert running.audit_state.cov_max_len == 64
        _run(running, fixture["with_long_row"])  # known ids, but a 130-token row after rows of at most 64
        audits = _audits(running)
        assert audits["count"] == 2 and audits["by_trigger"] == {"coverage": 2}
        last = audits["last"]
        # the longest row is always taken; the budget of 200 tokens then leaves room for the next 64-token row only
        assert last["passed"] and last["rows"][0] == 2 and last["tokens"] <= 200, last
        assert running.audit_state.cov_max_len == 130
        _run(running, fixture["with_long_row"])
        assert _audits(running)["count"] == 2
    assert running.effective_policy()["kernel_set"] == "f16"


def test_a_token_the_calibration_never_saw_is_caught_by_the_running_audit(fixture):
    from open_provence_amd.synthetic import OUTLIER_TOKEN

    batch = fixture["with_outlier"]
    assert OUTLIER_TOKEN in batch[2] and all(OUTLIER_TOKEN not in r for i, r in enumerate(batch) if i != 2)
    lengths = [len(r) for r in batch]
    lo, hi = sum(lengths[:2]), sum(lengths[:3])

    # 1. the fixture bites on hardware: an audit="first" encoder returns row 2 on "f16", beyond the bound from the reference set
    first = _encoder(fixture, "first")
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        _run(first, fixture["short"])
        on_f16 = _run(first, batch)
        assert first.effective_policy()["kernel_set"] == "f16"
        first.select_kernel_set("bf16x3")
        on_reference = _run(first, batch)
    bound = 3e-4
    drift = max(float(np.abs(on_f16[0][lo:hi] - on_reference[0][lo:hi]).max()), float(np.abs(on_f16[1][2] - on_reference[1][2]).max()))
    print(f"row 2 on 'f16' against 'bf16x3': {drift:.3e} (bound {bound:.1e})")
    assert np.isfinite(on_f16[0]).all() and np.isfinite(on_f16[1]).all()  # nothing the range guard would see
    assert drift > bound

    # 2. the running audit catches it, reverts for good, and returns the default set's answer for THIS batch
    running = _encoder(fixture, "running")
    default_set = running.calibration["default_set"]
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        _run(running, fixture["short"])
    assert _audits(running)["last"]["passed"] and running.effective_policy()["kernel_set"] == "f16"
    with pytest.warns(RuntimeWarning, match="running audit") as caught:
        got = _run(running, batch)
    assert len([w for w in caught if issubclass(w.category, RuntimeWarning)]) == 1
    assert running.effective_policy()["kernel_set"] == default_set == running.calibration["chosen_set"]
    uncalibrated = _encoder(fixture, "first", calibrate=False)
    assert uncalibrated.effective_policy()["kernel_set"] == default_set
    want = _run(uncalibrated, batch)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    last = _audits(running)["last"]
    assert last["trigger"] == "coverage" and last["passed"] is False and 2 in last["rows"], last
    assert last["max_abs_err"] > last["bound"] and np.isfinite(last["max_abs_err"])
    count = _audits(running)["count"]
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        again = _run(running, batch)  # from then on: the default set, nothing left to audit
    assert np.array_equal(again[0], want[0]) and _audits(running)["count"] == count
    assert running.effective_policy()["kernel_set"] == default_set


# -- the public entries ----------------------------------------------------------------------------------------------------------
def _model(state, audit, **kwargs):
    from open_provence_amd.config import OpenProvenceConfig
    from open_provence_amd.modeling import OpenProvenceModel
    from open_provence_amd.synthetic import XSMALL

    from helpers import CharTokenizer

    base = dict(XSMALL, vocab_size=500, num_hidden_layers=3, model_type="modernbert", local_attention=128, global_attn_every_n_layers=3,
                global_rope_theta=160000.0, local_rope_theta=10000.0, max_position_embeddings=8192, pad_token_id=0, cls_token_id=1,
                sep_token_id=2)
    cfg = OpenProvenceConfig(base_model_config=base, tokenizer_name_or_path="char-tokenizer", pruning_config={"hidden_size": 256},
                             max_length=256, num_labels=1)
    return OpenProvenceModel(cfg, device=DEV, tokenizer=CharTokenizer(), state_dict=state, precision="bf16x3", audit=audit, **kwargs)


def test_device_resident_forward_takes_the_scan_path_to_the_same_verdict(fixture):
    from open_provence_amd.synthetic import pad_rows

    scans = {False: 0, True: 0}

    def verdicts(on_device):
        model = _model(fixture["state"], "running", calibration_rows=fixture["benign"])
        assert model.encoder.effective_policy()["kernel_set"] == "f16"
        scan = model.encoder.coverage_scan_device

        def counted(*args):
            scans[on_device] += 1
            return scan(*args)

        model.encoder.coverage_scan_device = counted
        seen, outs = [], []
        for rows in (fixture["short"], fixture["short"], fixture["with_long_row"], fixture["with_long_row"], fixture["with_outlier"]):
            ids, mask = pad_rows(rows)
            if on_device:
                ids, mask = ids.to(DEV), mask.to(DEV)
            with warnings.catch_warnings():
                warnings.simplefilter("ignore", RuntimeWarning)
                out = model.forward(input_ids=ids, attention_mask=mask)
            outs.append((out.ranking_logits.cpu().numpy(), out.pruning_logits.cpu().numpy()))
            last = _audits(model.encoder)["last"]
            seen.append((_audits(model.encoder)["count"], last["trigger"], last["passed"], last["rows"], model.encoder.effective_policy()["kernel_set"]))
        return seen, outs

    host, host_outs = verdicts(False)
    device, device_outs = verdicts(True)
    assert [s[0] for s in host] == [1, 1, 2, 2, 3] and host[-1][2] is False and host[-1][4] != "f16", host
    assert device == host
    # host ids: the device is never asked; device-resident: one scan per forward while the calibrated set runs (the fifth
    # forward's scan is what found the token, the set is dropped after it)
    assert scans == {False: 0, True: 5}, scans
    for (rank_h, prune_h), (rank_d, prune_d) in zip(host_outs, device_outs):
        assert np.array_equal(rank_h, rank_d) and np.array_equal(prune_h, prune_d)


def test_process_returns_what_the_first_batch_mode_returns(fixture):
    from open_provence_amd.synthetic import refinit_state_dict

    from helpers import period_splitter

    state = refinit_state_dict(fixture["dims"], 7)  # (plain weights: calibrated on the library's own batch, first audit pending)
    words = "the tower is tall boats carry fish and salt to north city harbour many years ago it was new".split()
    contexts = [" ".join(" ".join(words[(i * 5 + s * 3 + k) % len(words)] for k in range(4 + (i + s) % 5)).capitalize() + "."
                         for s in range(1 + i % 4)) for i in range(6)]
    results = {}
    for audit in ("first", "running"):
        model = _model(state, audit)
        assert model.encoder.audit_mode == audit and model.encoder.effective_policy()["kernel_set"] == "f16"
        with warnings.catch_warnings():
            warnings.simplefilter("error", RuntimeWarning)
            results[audit] = model.process(question="where do the boats carry fish?", context=contexts, sentence_splitter=period_splitter,
                                           show_progress=False, return_sentence_metrics=True)
        audits = _audits(model.encoder)
        assert model.encoder.calibration["audit"]["passed"]  # the first batch's own report, in both modes
        assert (audits["count"] >= 1 and audits["last"]["passed"]) if audit == "running" else audits["count"] == 0
        assert model.encoder.effective_policy()["kernel_set"] == "f16"
    def plain(value):  # (numpy scalars and arrays as Python values: compared exactly)
        if isinstance(value, dict):
            return {k: plain(v) for k, v in value.items() if k not in ("timing", "performance_trace")}
        if isinstance(value, (list, tuple)):
            return [plain(v) for v in value]
        return value.tolist() if isinstance(value, (np.ndarray, np.generic)) else value

    assert plain(results["first"]) == plain(results["running"])
    assert results["first"]["pruned_context"] is not None
