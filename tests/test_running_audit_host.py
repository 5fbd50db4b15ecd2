"""The running audit of a calibrated kernel set, the parts that need no GPU: the coverage counts and the row selection against
plain-Python restatements, the five C calls (declared, bound, exported, refused before the handle when malformed -- additive
to ABI 10), the audit policy's argument forms, and the fixture of tests/test_gpu_running_audit.py checked on the float64 model
of the kernel sets' arithmetic (tests/arith_model.py): the planted token must be wrong on "f16" for the reason the audit
exists -- finite, in range, beyond the bound -- while the benign rows stay within the calibration tolerance."""

import ctypes
import inspect
import re
from pathlib import Path

import numpy as np
import pytest

from open_provence_amd import _lib
from open_provence_amd.engine import (DEFAULT_AUDIT_TOKENS, DEFAULT_CALIBRATION_TOLERANCE, HipEncoder, coverage_counts,
                                      resolve_audit_mode, select_audit_rows)

HEADER = Path(__file__).resolve().parents[1] / "include" / "open_provence_hip.h"
CALLS = ("op_coverage_scan", "op_coverage_commit", "op_coverage_reset", "op_gather_rows", "op_audit_compare")


# -- coverage counts ---------------------------------------------------------------------------------------------------------
def _counts_reference(ids, cu, covered):
    return [sum(1 for t in ids[cu[s]: cu[s + 1]] if not (0 <= t < len(covered) and covered[t])) for s in range(len(cu) - 1)]


def test_coverage_counts_match_a_plain_restatement():
    rng = np.random.default_rng(5)
    covered = np.zeros(500, dtype=bool)
    covered[[0, 31, 32, 63, 499]] = True
    lengths = [1, 0, 63, 64, 65, 130, 7]
    cu = np.concatenate(([0], np.cumsum(lengths))).astype(np.int32)
    ids = rng.choice([0, 31, 32, 63, 499, 1, 33, 64, 498, 250], size=int(cu[-1])).astype(np.int32)
    ids[5] = ids[6] = 250  # a duplicate inside a row counts once per position
    got = coverage_counts(ids, cu, covered)
    assert got.dtype == np.int32 and got.tolist() == _counts_reference(ids.tolist(), cu.tolist(), covered)
    assert got[1] == 0 and got.sum() == int((~covered[ids]).sum())
    # an id outside the table is novel and never an index
    wild = np.array([0, -1, 500, 31], dtype=np.int64)
    assert coverage_counts(wild, np.array([0, 4]), covered).tolist() == [2]
    assert coverage_counts(np.zeros(0, dtype=np.int32), np.array([0]), covered).tolist() == []
    assert coverage_counts(ids, cu, np.ones(500, dtype=bool)).tolist() == [0] * len(lengths)


# -- row selection -----------------------------------------------------------------------------------------------------------
def _select_reference(row_novel, lengths, budget, longest=None):
    order = sorted(range(len(row_novel)), key=lambda i: (-row_novel[i], -lengths[i], i))
    if longest is not None:
        order.remove(longest)
        order.insert(0, longest)
    picked, tokens = [], 0
    for i in order:
        if picked and tokens + lengths[i] > budget:
            break
        picked.append(i)
        tokens += lengths[i]
    return picked


def test_select_audit_rows_orders_by_novelty_then_length_then_index():
    assert select_audit_rows([0, 5, 2], [10, 10, 10], 100) == [1, 2, 0]
    # ties on novelty go to the longer row, ties on both to the lower index
    assert select_audit_rows([3, 3, 3, 3], [10, 20, 20, 5], 100) == [1, 2, 0, 3]
    # the selection stops before the budget is exceeded -- it does not skip ahead to a row that would still fit
    assert select_audit_rows([9, 8, 7], [40, 70, 10], 100) == [0]
    assert select_audit_rows([9, 8, 7], [40, 60, 10], 100) == [0, 1]
    # a budget smaller than the first row: that row alone
    assert select_audit_rows([1, 4], [50, 300], 64) == [1]
    # the longest row is forced in first when the length trigger fired, whatever its novelty
    assert select_audit_rows([5, 0, 2], [10, 130, 10], 140, longest=1) == [1, 0]
    assert select_audit_rows([5, 0, 2], [10, 130, 10], 64, longest=1) == [1]
    assert select_audit_rows([], [], 100) == [] == select_audit_rows([], [], 100, longest=None)
    rng = np.random.default_rng(11)
    for _ in range(200):
        n = int(rng.integers(1, 12))
        novel, lengths = rng.integers(0, 4, n).tolist(), rng.integers(1, 131, n).tolist()
        budget = int(rng.integers(1, 400))
        longest = int(np.argmax(lengths)) if rng.integers(0, 2) else None
        got = select_audit_rows(novel, lengths, budget, longest)
        assert got == _select_reference(novel, lengths, budget, longest)
        assert len(got) >= 1 and len(set(got)) == len(got)
        assert len(got) == 1 or sum(lengths[i] for i in got) <= budget


# -- policy --------------------------------------------------------------------------------------------------------------------
def test_audit_policy_argument_forms(monkeypatch):
    monkeypatch.delenv("OPEN_PROVENCE_AUDIT", raising=False)
    assert resolve_audit_mode(None) == "first" == resolve_audit_mode(True) == resolve_audit_mode("first")
    assert resolve_audit_mode(False) == "off" == resolve_audit_mode("off")
    assert resolve_audit_mode("running") == "running" == resolve_audit_mode(" Running ")
    with pytest.raises(ValueError):
        resolve_audit_mode("always")
    for env in ("0", "off", "false", "no", "OFF"):
        monkeypatch.setenv("OPEN_PROVENCE_AUDIT", env)
        assert resolve_audit_mode(None) == "off", env
    monkeypatch.setenv("OPEN_PROVENCE_AUDIT", "running")
    assert resolve_audit_mode(None) == "running" and resolve_audit_mode("first") == "first"  # (an argument wins)
    monkeypatch.setenv("OPEN_PROVENCE_AUDIT", "1")
    assert resolve_audit_mode(None) == "first"
    assert DEFAULT_AUDIT_TOKENS == 8192
    from open_provence_amd.modeling import OpenProvenceModel

    enc = inspect.signature(HipEncoder.__init__).parameters
    model = inspect.signature(OpenProvenceModel.__init__).parameters
    assert enc["audit"].default is None and enc["audit_every"].default == 0 and enc["audit_tokens"].default == DEFAULT_AUDIT_TOKENS
    assert all(name in model for name in ("audit", "audit_every", "audit_tokens"))
    assert "ids_host" in inspect.signature(HipEncoder.forward_packed).parameters


# -- header and binding ----------------------------------------------------------------------------------------------------------
def test_the_five_calls_are_declared_and_the_abi_version_stays():
    assert _lib.OP_ABI_VERSION == 10
    text = re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)
    for name in CALLS:
        assert name in _lib.EXPORTED_SYMBOLS
        assert re.search(rf"\bint {name}\s*\(", text), name
    assert "#define OP_ABI_VERSION 10" in text
    assert ctypes.sizeof(_lib.OpCoverageReport) == 20  # uint32 + 4 x int32, no padding
    assert [f[0] for f in _lib.OpCoverageReport._fields_] == ["struct_bytes", "novel_tokens", "longest_row_tokens", "longest_row", "max_audited_tokens"]


def test_library_exports_and_binds_the_calls(hip_library):
    assert hip_library.op_abi_version() == 10
    for name, n_args in zip(CALLS, (8, 8, 1, 10, 13)):
        assert hasattr(hip_library, name), name
        assert len(getattr(hip_library, name).argtypes) == n_args, name
    assert hip_library.op_coverage_scan.argtypes[-2] is ctypes.POINTER(_lib.OpCoverageReport)


# (never dereferenced: every call below is refused before the handle, let alone a device, is touched)
_BUF = ctypes.c_void_p(0x1000)


def _refused(lib, code, field):
    message = _lib.last_error(lib, None)
    assert code == _lib.OP_ERR_INVALID and field in message and "NULL handle" not in message, (code, message)


def _reaches_the_handle(lib, code):
    assert code == _lib.OP_ERR_INVALID and "NULL handle" in _lib.last_error(lib, None), (code, _lib.last_error(lib, None))


def test_malformed_calls_are_refused_before_the_handle(hip_library):
    lib = hip_library
    report = _lib.OpCoverageReport()
    report.struct_bytes = ctypes.sizeof(_lib.OpCoverageReport)
    ref = ctypes.byref(report)
    _refused(lib, lib.op_coverage_scan(None, _BUF, _BUF, 2, 8, _BUF, None, None), "report")
    bad = _lib.OpCoverageReport()
    bad.struct_bytes = 12
    _refused(lib, lib.op_coverage_scan(None, _BUF, _BUF, 2, 8, _BUF, ctypes.byref(bad), None), "struct_bytes")
    _refused(lib, lib.op_coverage_scan(None, _BUF, _BUF, -1, 8, _BUF, ref, None), "n_seqs")
    _refused(lib, lib.op_coverage_scan(None, _BUF, _BUF, 2, -8, _BUF, ref, None), "total_tokens")
    _refused(lib, lib.op_coverage_scan(None, None, _BUF, 2, 8, _BUF, ref, None), "ids_dev")
    _refused(lib, lib.op_coverage_scan(None, _BUF, None, 2, 8, _BUF, ref, None), "cu_seqlens_dev")
    _refused(lib, lib.op_coverage_scan(None, _BUF, _BUF, 2, 8, None, ref, None), "row_novel_dev")
    _reaches_the_handle(lib, lib.op_coverage_scan(None, _BUF, _BUF, 2, 8, _BUF, ref, None))
    _reaches_the_handle(lib, lib.op_coverage_scan(None, None, None, 0, 0, None, ref, None))

    def commit(ids=_BUF, cu=_BUF, n_seqs=2, total=8, rows=_BUF, n=1):
        return lib.op_coverage_commit(None, ids, cu, n_seqs, total, rows, n, None)

    def gather(ids=_BUF, cu=_BUF, n_seqs=2, total=8, rows=_BUF, n=1, sub_ids=_BUF, sub_cu=_BUF):
        return lib.op_gather_rows(None, ids, cu, n_seqs, total, rows, n, sub_ids, sub_cu, None)

    def compare(**kw):
        a = dict(prune=_BUF, rank=_BUF, cu=_BUF, n_seqs=2, total=8, rows=_BUF, n=1, sp=_BUF, sr=_BUF, scu=_BUF, err=_BUF)
        a.update(kw)
        return lib.op_audit_compare(None, a["prune"], a["rank"], a["cu"], a["n_seqs"], a["total"], a["rows"], a["n"], a["sp"], a["sr"],
                                    a["scu"], a["err"], None)

    for call in (commit, gather, compare):  # the three share the checks of a packed batch and a list of its rows
        _refused(lib, call(n=-1), "n_rows")
        _refused(lib, call(n_seqs=-1), "n_seqs")
        _refused(lib, call(total=-3), "total_tokens")
        _refused(lib, call(cu=None), "cu_seqlens_dev")
        _refused(lib, call(rows=None), "rows_dev")
        _reaches_the_handle(lib, call())
    _refused(lib, commit(ids=None), "ids_dev")
    _reaches_the_handle(lib, commit(ids=None, cu=None, rows=None, n=0))
    _reaches_the_handle(lib, lib.op_coverage_reset(None))
    _refused(lib, gather(sub_cu=None), "sub_cu_dev")
    _refused(lib, gather(ids=None), "ids_dev")
    _refused(lib, gather(sub_ids=None), "sub_ids_dev")
    _refused(lib, compare(err=None), "err_dev")
    for key, field in (("prune", "prune_dev"), ("sp", "sub_prune_dev"), ("rank", "rank_dev"), ("sr", "sub_rank_dev"), ("scu", "sub_cu_dev")):
        _refused(lib, compare(**{key: None}), field)


# -- the fixture bites, on the CPU -------------------------------------------------------------------------------------------------
def test_the_outlier_fixture_bites_on_the_model_of_the_f16_set():
    """"f16" against "bf16x3" on the float64 model: the six benign rows within the calibration tolerance (the set calibrates,
    the first audit passes), the 70-token row holding the planted token at least twice the audit bound away (the verdict does
    not hang on accumulation order), and that difference finite with max |hidden| far inside fp16's range (65504): the range
    guard is not what fires."""

    import arith_model as am
    from open_provence_amd.synthetic import OUTLIER_CHANNEL, OUTLIER_TOKEN, named_dims, outlier_token_rows, outlier_token_state_dict

    dims = named_dims("xsmall", num_layers=3, vocab_size=500)
    assert (dims.hidden_size, dims.num_heads, tuple(dims.layer_is_global)) == (256, 4, (True, False, False))
    state = outlier_token_state_dict(dims)
    emb = state["ranking_model.model.embeddings.tok_embeddings.weight"]
    assert (emb[:, OUTLIER_CHANNEL] != 0).nonzero().flatten().tolist() == [OUTLIER_TOKEN] and int((emb[OUTLIER_TOKEN] != 0).sum()) == 1
    benign, outlier = outlier_token_rows()
    assert [len(r) for r in benign] == [3, 17, 40, 63, 64, 130] and len(outlier) == 70
    assert max(max(r) for r in benign) < 400 and outlier.count(OUTLIER_TOKEN) == 1 and max(t for t in outlier if t != OUTLIER_TOKEN) < 400

    def difference(rows):
        chosen, reference = am.forward(state, dims, rows, "f16"), am.forward(state, dims, rows, "bf16x3")
        err = max(float((chosen.prune - reference.prune).abs().max()), float((chosen.rank - reference.rank).abs().max()))
        return err, max(float(h.abs().max()) for h in chosen.hidden)

    bound = 3.0 * DEFAULT_CALIBRATION_TOLERANCE
    benign_err, _ = difference(benign)
    outlier_err, outlier_peak = difference([outlier])
    print(f"benign {benign_err:.3e}  outlier {outlier_err:.3e}  max |hidden| {outlier_peak:.1f}")
    assert benign_err <= DEFAULT_CALIBRATION_TOLERANCE
    assert outlier_err >= 2.0 * bound == pytest.approx(6e-4)
    assert np.isfinite(outlier_err) and outlier_peak < 65504.0 / 64
