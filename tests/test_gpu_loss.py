"""The evaluation losses on the device: ``op_loss`` through ``HipEncoder.loss`` on synthetic logits against the float64
restatement (tests/loss_model.py), and ``forward(labels=...)`` of the three model classes on the row path and the panel path.

The gates hold no measured number.  Every term and the scalar are fp64 values rounded once to fp32, so they sit within 1 fp32
ulp of ``float32(restatement)`` (floor: one fp32 subnormal step).  The scalar is also held to torch's own fp32 loss on the CPU
by the triangle inequality, ``|got - ref32| <= |ref32 - want64| + 1 ulp``; ``|ref32 - want64|`` is printed per case (``-s``;
profiles/loss_distance.txt is the first run's record)."""

from __future__ import annotations

import dataclasses

import numpy as np
import pytest
import torch

import loss_model as lm
from helpers import CharTokenizer

pytestmark = pytest.mark.gpu

N_ROWS = (0, 1, 3, 1500)  # 1500: more rows than the grid has blocks (256 blocks of 4 waves / 256 threads)
WIDTHS = (1, 67, 160)
SPECIAL = np.array([80.0, -80.0, 1e4, -1e4], dtype=np.float32)


@pytest.fixture(scope="module")
def enc():
    """A handle without weights: the loss needs only logits."""

    from open_provence_amd.engine import HipEncoder
    from open_provence_amd.synthetic import named_dims

    encoder = HipEncoder(named_dims("xsmall", vocab_size=1000, num_layers=1), device="cuda:0")
    yield encoder
    encoder.close()


def _logits(rng, shape):
    """fp32 logits of order 1 with +/-80, +/-1e4 and exact ties (a whole row at one value) mixed in."""

    z = (rng.standard_normal(shape) * 3).astype(np.float32)
    pick = rng.random(shape) < 0.15
    z[pick] = rng.choice(SPECIAL, size=int(pick.sum()))
    if len(shape) > 1 and shape[0]:
        tie = rng.random(shape[0]) < 0.1
        z[tie] = z[tie][..., :1]
        if shape[0] > 2:
            z[2] = 1e4  # a tie at the largest magnitude
    return z


def _lengths(rng, n_rows, width, short):
    if short:  # rows of at most 4 tokens
        lengths = rng.integers(0, min(width, 4) + 1, size=n_rows)
    else:
        lengths = rng.integers(0, width + 1, size=n_rows)
    if n_rows >= 3:
        lengths[:3] = (0, 1, min(width, 4) if short else width)
    elif n_rows == 1:
        lengths[0] = width
    if lengths.sum() % 64 == 0 and n_rows:  # total_tokens is never a multiple of the wave
        lengths[-1] = lengths[-1] - 1 if lengths[-1] else 1
    return lengths


def _bits(t):
    return t.contiguous().view(torch.int32)


def _assert_within_one_ulp(got32, want64, what):
    """Every element of fp32 ``got32`` within 1 fp32 ulp of float32(want64) (floor: one subnormal step); NaN matches NaN."""

    got32, want64 = np.atleast_1d(np.asarray(got32)), np.atleast_1d(np.asarray(want64, dtype=np.float64))
    assert got32.dtype == np.float32 and got32.shape == want64.shape, what
    with np.errstate(over="ignore"):
        want32 = want64.astype(np.float32)
    nan = np.isnan(want32)
    assert np.array_equal(np.isnan(got32), nan), what
    with np.errstate(invalid="ignore"):
        tol = np.maximum(np.spacing(np.abs(want32)), np.float32(1.401298464324817e-45)).astype(np.float64)
        err = np.abs(got32.astype(np.float64) - want32.astype(np.float64))
    bad = ~nan & np.isfinite(want32) & ~(err <= tol)
    assert not bad.any(), (what, int(bad.sum()), got32[bad][:4], want32[bad][:4])
    inf = ~nan & ~np.isfinite(want32)
    assert np.array_equal(got32[inf], want32[inf]), what


def _assert_near_torch(got: float, ref32: float, want64: float, what):
    """|got - ref32| <= |ref32 - want64| + 1 ulp: the triangle inequality through the restatement."""

    if np.isnan(want64):
        assert np.isnan(got) and np.isnan(ref32), what
        return
    distance = abs(ref32 - want64)
    print(f"[loss distance] {what}: |torch fp32 - fp64 restatement| = {distance:.3e} (loss {want64:.6g})")
    assert abs(got - ref32) <= distance + lm.ulp32(want64), (what, got, ref32, want64)


def _torch_ce32(logits, labels):
    if logits.shape[0] == 0:
        return float("nan")
    return float(torch.nn.CrossEntropyLoss()(torch.from_numpy(logits), torch.from_numpy(labels.astype(np.int64))))


# -- the kernels through HipEncoder.loss -----------------------------------------------------------------------------------
@pytest.mark.parametrize("label_dtype", [torch.int64, torch.int32])
@pytest.mark.parametrize("width", WIDTHS)
def test_token_loss_and_terms_against_the_restatement(enc, width, label_dtype):
    rng = np.random.default_rng(100 + width)
    for n_rows, short in [(n, False) for n in N_ROWS] + [(1500, True)]:
        what = f"token_ce rows={n_rows} width={width} short={short} {label_dtype}"
        lengths = _lengths(rng, n_rows, width, short)
        total = int(lengths.sum())
        assert total % 64 != 0 or total == 0
        cu = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int32)
        packed = _logits(rng, (total, 2))
        valid = np.arange(width)[None, :] < lengths[:, None]
        labels = rng.integers(0, 2, size=(n_rows, width))
        labels[rng.random((n_rows, width)) < 0.2] = -100
        # labels under the padding: garbage in one copy, zeros in the other -- they are never read
        garbage = np.where(valid, labels, np.where(np.arange(width)[None, :] % 2 == 0, 7, -12345))
        zeros = np.where(valid, labels, 0)
        want, want_terms, count = lm.token_ce(packed, zeros, cu)

        logits_d, cu_d = torch.from_numpy(packed).cuda(), torch.from_numpy(cu).cuda()
        got, terms = enc.loss("token_ce", logits_d, torch.from_numpy(garbage).to(label_dtype).cuda(), cu=cu_d, terms=True)
        assert got.shape == () and got.dtype == torch.float32 and got.device == enc.device and terms.shape == (total,)
        assert enc.last_loss_report["count"] == count and enc.last_loss_report["status"] == 0
        got_z, terms_z = enc.loss("token_ce", logits_d, torch.from_numpy(zeros).to(label_dtype).cuda(), cu=cu_d, width=width, terms=True)
        assert torch.equal(_bits(got), _bits(got_z)) and torch.equal(_bits(terms), _bits(terms_z)), what
        # twice, without terms, unchecked, and on a second stream: the same bits
        again = enc.loss("token_ce", logits_d, torch.from_numpy(garbage).to(label_dtype).cuda(), cu=cu_d, check=False)
        assert torch.equal(_bits(got), _bits(again)), what
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            other, other_terms = enc.loss("token_ce", logits_d, torch.from_numpy(garbage).to(label_dtype).cuda(), cu=cu_d, terms=True)
        side.synchronize()
        torch.cuda.current_stream().wait_stream(side)
        assert torch.equal(_bits(got), _bits(other)) and torch.equal(_bits(terms), _bits(other_terms)), what

        terms_np = terms.cpu().numpy()
        _assert_within_one_ulp(terms_np, want_terms, what)
        y_packed = np.concatenate([labels[r, : lengths[r]] for r in range(n_rows)]) if n_rows else np.zeros(0, dtype=np.int64)
        ignored = y_packed == -100
        assert (terms_np[ignored].view(np.int32) == 0).all(), what  # exactly +0.0
        _assert_within_one_ulp(got.cpu().numpy(), want, what)
        if count == 0:
            assert np.isnan(float(got)), what
        keep = ~ignored
        _assert_near_torch(float(got), _torch_ce32(packed[keep], y_packed[keep]), want, what)


def test_token_loss_zero_counts_are_nan(enc):
    rng = np.random.default_rng(7)
    width = 9
    for lengths, labels_fill in (([9, 4, 0], -100), ([0, 0, 0], 1)):  # all ignored; no active position (the 0.0 rule is the model's)
        lengths = np.array(lengths)
        cu = torch.from_numpy(np.concatenate([[0], np.cumsum(lengths)]).astype(np.int32)).cuda()
        logits = torch.from_numpy(_logits(rng, (int(lengths.sum()), 2))).cuda()
        labels = torch.full((3, width), labels_fill, dtype=torch.int64, device="cuda")
        got, terms = enc.loss("token_ce", logits, labels, cu=cu, terms=True)
        assert np.isnan(float(got)) and enc.last_loss_report["count"] == 0 and enc.last_loss_report["sum"] == 0.0
        assert (terms.cpu().numpy().view(np.int32) == 0).all()
        assert np.isnan(float(enc.loss("token_ce", logits, labels, cu=cu, check=False)))
    # another ignore_index
    lengths = np.array([5, 9, 2])
    cu_np = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int32)
    packed = _logits(rng, (16, 2))
    labels = rng.integers(0, 2, size=(3, width))
    labels[rng.random((3, width)) < 0.4] = -1
    got = enc.loss("token_ce", torch.from_numpy(packed).cuda(), torch.from_numpy(labels).cuda(), cu=torch.from_numpy(cu_np).cuda(), ignore_index=-1)
    _assert_within_one_ulp(got.cpu().numpy(), lm.token_ce(packed, labels, cu_np, ignore_index=-1)[0], "ignore_index=-1")


def test_ranking_losses_against_the_restatement(enc):
    rng = np.random.default_rng(21)
    for n_rows in N_ROWS:
        # binary cross entropy with logits: hard and soft targets
        z = _logits(rng, (n_rows, 1))
        for y in (rng.integers(0, 2, size=n_rows).astype(np.float32), rng.random(n_rows).astype(np.float32)):
            what = f"rank_bce rows={n_rows}"
            want, want_terms, count = lm.rank_bce(z, y)
            got, terms = enc.loss("rank_bce", torch.from_numpy(z).cuda(), torch.from_numpy(y).cuda(), terms=True)
            assert enc.last_loss_report["count"] == count == n_rows
            flat = enc.loss("rank_bce", torch.from_numpy(z[:, 0].copy()).cuda(), torch.from_numpy(y).cuda(), check=False)
            assert torch.equal(_bits(got), _bits(flat)), what
            _assert_within_one_ulp(terms.cpu().numpy(), want_terms, what)
            _assert_within_one_ulp(got.cpu().numpy(), want, what)
            ref32 = float(torch.nn.BCEWithLogitsLoss()(torch.from_numpy(z).view(-1), torch.from_numpy(y))) if n_rows else float("nan")
            _assert_near_torch(float(got), ref32, want, what)
        # C-class cross entropy
        for C in (2, 3, 5):
            for label_dtype in (torch.int64, torch.int32):
                what = f"rank_ce rows={n_rows} C={C} {label_dtype}"
                z = _logits(rng, (n_rows, C))
                y = rng.integers(0, C, size=n_rows)
                y[rng.random(n_rows) < 0.2] = -100
                want, want_terms, count = lm.rank_ce(z, y)
                got, terms = enc.loss("rank_ce", torch.from_numpy(z).cuda(), torch.from_numpy(y).to(label_dtype).cuda(), terms=True)
                assert enc.last_loss_report["count"] == count
                again = enc.loss("rank_ce", torch.from_numpy(z).cuda(), torch.from_numpy(y).to(label_dtype).cuda())
                assert torch.equal(_bits(got), _bits(again)), what
                terms_np = terms.cpu().numpy()
                _assert_within_one_ulp(terms_np, want_terms, what)
                assert (terms_np[y == -100].view(np.int32) == 0).all(), what
                _assert_within_one_ulp(got.cpu().numpy(), want, what)
                _assert_near_torch(float(got), _torch_ce32(z[y != -100], y[y != -100]), want, what)
        # mean squared error
        for C in (1, 3):
            what = f"rank_mse rows={n_rows} C={C}"
            z, y = _logits(rng, (n_rows, C)), rng.standard_normal((n_rows, C)).astype(np.float32)
            want, want_terms, count = lm.rank_mse(z, y)
            got, terms = enc.loss("rank_mse", torch.from_numpy(z).cuda(), torch.from_numpy(y).cuda(), terms=True)
            assert enc.last_loss_report["count"] == count == n_rows * C and terms.shape == (n_rows, C)
            _assert_within_one_ulp(terms.cpu().numpy(), want_terms, what)
            _assert_within_one_ulp(got.cpu().numpy(), want, what)
            ref32 = float(torch.nn.MSELoss()(torch.from_numpy(z), torch.from_numpy(y))) if n_rows else float("nan")
            _assert_near_torch(float(got), ref32, want, what)
    # every label ignored: NaN, count 0
    z = torch.from_numpy(_logits(rng, (5, 3))).cuda()
    got = enc.loss("rank_ce", z, torch.full((5,), -100, dtype=torch.int64, device="cuda"))
    assert np.isnan(float(got)) and enc.last_loss_report["count"] == 0


def test_a_label_out_of_range_is_reported_not_used(enc):
    rng = np.random.default_rng(31)
    n_rows, width = 40, 23
    lengths = rng.integers(8, width + 1, size=n_rows)
    cu_np = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int32)
    packed = _logits(rng, (int(lengths.sum()), 2))
    labels = rng.integers(0, 2, size=(n_rows, width))
    labels[:, 7:] = np.where(np.arange(width)[None, 7:] < lengths[:, None], labels[:, 7:], 2)  # 2 under the padding does not count
    logits_d, cu_d = torch.from_numpy(packed).cuda(), torch.from_numpy(cu_np).cuda()
    good = enc.loss("token_ce", logits_d, torch.from_numpy(labels).cuda(), cu=cu_d)
    for value in (2, -1, 1 << 40):
        bad, other = labels.copy(), value * 3 + 1
        bad[31, 2], bad[17, 5], bad[17, 3], bad[3, 6] = value, value, other, 5  # row-major first: (3, 6) = 5
        bad_d = torch.from_numpy(bad).cuda()
        with pytest.raises(IndexError, match=r"label 5 at row 3, column 6 "):
            enc.loss("token_ce", logits_d, bad_d, cu=cu_d)
        report = enc.last_loss_report
        assert (report["status"], report["bad_row"], report["bad_col"], report["bad_value"]) == (1, 3, 6, 5)
        assert np.isnan(report["loss"]) and report["count"] == int(lengths.sum()) - 4
        bad[3, 6] = labels[3, 6]
        with pytest.raises(IndexError, match=rf"label {other} at row 17, column 3 "):
            enc.loss("token_ce", logits_d, torch.from_numpy(bad).cuda(), cu=cu_d)
        assert enc.last_loss_report["bad_value"] == other
        unchecked, terms = enc.loss("token_ce", logits_d, bad_d, cu=cu_d, check=False, terms=True)  # nothing raises
        assert np.isnan(float(unchecked)) and enc.last_loss_report is None
        assert float(terms[int(cu_np[3]) + 6]) == 0.0 and torch.isfinite(terms).all()
        assert torch.equal(_bits(enc.loss("token_ce", logits_d, torch.from_numpy(labels).cuda(), cu=cu_d)), _bits(good))  # the handle works
    # int32 labels; the ranking cross entropy: C and -1
    with pytest.raises(IndexError, match=r"label 2 at row 0, column 0 "):
        first = labels.copy()
        first[0, 0] = 2
        enc.loss("token_ce", logits_d, torch.from_numpy(first).to(torch.int32).cuda(), cu=cu_d)
    for C in (2, 3, 5):
        z = torch.from_numpy(_logits(rng, (300, C))).cuda()
        y = rng.integers(0, C, size=300)
        y[5] = -100
        good = enc.loss("rank_ce", z, torch.from_numpy(y).cuda())
        for value, row in ((C, 299), (-1, 258), (C, 4)):
            y[row] = value
            with pytest.raises(IndexError, match=rf"label {value} at row {row}, column 0 "):
                enc.loss("rank_ce", z, torch.from_numpy(y).cuda())
            assert enc.last_loss_report["bad_row"] == row and enc.last_loss_report["bad_value"] == value
            assert np.isnan(float(enc.loss("rank_ce", z, torch.from_numpy(y).to(torch.int32).cuda(), check=False)))
        y[[299, 258, 4]] = 0
        y2 = y.copy()
        y2[[299, 258, 4]] = -100
        want = lm.rank_ce(z.cpu().numpy(), y2)[0]
        _assert_within_one_ulp(enc.loss("rank_ce", z, torch.from_numpy(y2).cuda()).cpu().numpy(), want, f"rank_ce after errors C={C}")
        assert torch.isfinite(good)


def test_loss_argument_errors(enc):
    z2 = torch.zeros(6, 2, device="cuda")
    cu = torch.tensor([0, 2, 6], dtype=torch.int32, device="cuda")
    labels = torch.zeros(2, 4, dtype=torch.int64, device="cuda")
    assert float(enc.loss("token_ce", z2, labels, cu=cu)) == pytest.approx(np.log(2.0), rel=1e-7)
    with pytest.raises(ValueError):
        enc.loss("hinge", z2, labels, cu=cu)
    with pytest.raises(ValueError):
        enc.loss("token_ce", z2, labels)  # no cu
    with pytest.raises(ValueError):
        enc.loss("token_ce", z2, labels, cu=cu[:-1])
    with pytest.raises(ValueError):
        enc.loss("token_ce", z2, labels, cu=cu, width=5)
    with pytest.raises(ValueError):
        enc.loss("token_ce", torch.zeros(9, 2, device="cuda"), labels, cu=cu)  # more tokens than label cells
    with pytest.raises(TypeError):
        enc.loss("token_ce", z2, labels.float(), cu=cu)
    with pytest.raises(TypeError):
        enc.loss("token_ce", z2.double(), labels, cu=cu)
    with pytest.raises(ValueError):
        enc.loss("token_ce", z2, labels.cpu(), cu=cu)
    with pytest.raises(TypeError):
        enc.loss("rank_bce", z2[:, :1].contiguous(), torch.zeros(6, dtype=torch.int64, device="cuda"))
    with pytest.raises(ValueError):
        enc.loss("rank_bce", z2, torch.zeros(6, device="cuda"))
    with pytest.raises(ValueError):
        enc.loss("rank_ce", z2[:, :1].contiguous(), torch.zeros(6, dtype=torch.int64, device="cuda"))
    with pytest.raises(ValueError):
        enc.loss("rank_ce", z2, torch.zeros(5, dtype=torch.int64, device="cuda"))
    with pytest.raises(ValueError):
        enc.loss("rank_mse", z2, torch.zeros(6, device="cuda"))
    # other integer label types are converted
    assert torch.equal(_bits(enc.loss("token_ce", z2, labels.to(torch.int16), cu=cu)), _bits(enc.loss("token_ce", z2, labels, cu=cu)))


# -- forward(labels=...) ---------------------------------------------------------------------------------------------------
ROWS, WIDTH = 24, 160


def _models(name):
    from open_provence_amd.config import OpenProvenceConfig
    from open_provence_amd.modeling import OpenProvenceForSequenceClassification, OpenProvenceForTokenClassification, OpenProvenceModel
    from open_provence_amd.synthetic import named_dims, refinit_state_dict

    dims = named_dims(name, vocab_size=2048, num_layers=3)

    def build(cls, num_labels, **kw):
        cfg = OpenProvenceConfig(base_model_config=dims.to_base_model_config(), tokenizer_name_or_path="char-tokenizer",
                                 pruning_config={"hidden_size": dims.hidden_size}, max_length=512, num_labels=num_labels,
                                 pruning_hidden_state="post_final_norm")
        state = refinit_state_dict(dataclasses.replace(dims, num_labels=num_labels), seed=5)
        return cls(cfg, device="cuda:0", tokenizer=CharTokenizer(), state_dict=state, calibrate=False, **kw)

    return dims, {"rank1": build(OpenProvenceModel, 1, attention_outputs=True), "rank3": build(OpenProvenceForSequenceClassification, 3),
                  "token": build(OpenProvenceForTokenClassification, 1)}


@pytest.fixture(scope="module", params=["xsmall", "base"])  # the row path and the panel path
def models(request):
    return _models(request.param)


def _ragged_inputs(dims, rows=ROWS, width=WIDTH, seed=3):
    from open_provence_amd.synthetic import pad_rows, synth_pair_batch

    rng = np.random.default_rng(seed)
    lengths = rng.integers(28, width + 1, size=rows).tolist()
    lengths[0], lengths[1] = width, 28
    return pad_rows(synth_pair_batch(dims, rows, lengths, seed=seed))


def _assert_same_outputs(got, want):
    assert torch.equal(got.ranking_logits, want.ranking_logits) and torch.equal(got.pruning_logits, want.pruning_logits)
    for name in ("hidden_states", "attentions"):
        a, b = got[name], want[name]
        assert (a is None) == (b is None), name
        if b is not None:
            assert len(a) == len(b) and all(torch.equal(x, y) for x, y in zip(a, b)), name


def test_token_classification_loss(models):
    dims, built = models
    model = built["token"]
    ids, mask = _ragged_inputs(dims)
    rng = np.random.default_rng(5)
    labels = torch.from_numpy(np.where(rng.random(ids.shape) < 0.2, -100, rng.integers(0, 2, size=ids.shape)))
    labels = torch.where(mask.bool(), labels, torch.full_like(labels, 7))  # garbage under the padding
    plain = model(input_ids=ids, attention_mask=mask, output_hidden_states=True)
    assert plain.loss is None
    out = model(input_ids=ids, attention_mask=mask, labels=labels, output_hidden_states=True)
    _assert_same_outputs(out, plain)
    assert out.logits is out.pruning_logits and out.loss.shape == () and out.loss.dtype == torch.float32 and out.loss.is_cuda
    want = lm.token_ce_padded(out.pruning_logits.cpu().numpy(), labels.numpy(), mask.numpy())[0]
    _assert_within_one_ulp(out.loss.cpu().numpy(), want, "token loss")
    ref32 = float(torch.nn.CrossEntropyLoss()(out.pruning_logits.cpu().view(-1, 2)[mask.view(-1) == 1], labels.view(-1)[mask.view(-1) == 1]))
    _assert_near_torch(float(out.loss), ref32, want, f"forward token loss hidden={dims.hidden_size}")
    # device tensors and CPU tensors; every integer label type
    on_device = model(input_ids=ids.cuda(), attention_mask=mask.cuda(), labels=labels.cuda())
    assert torch.equal(_bits(on_device.loss), _bits(out.loss)) and torch.equal(on_device.pruning_logits, out.pruning_logits)
    for dtype, where in ((torch.int32, "cuda"), (torch.int16, "cpu"), (torch.int64, "cuda")):
        mixed = model(input_ids=ids.cuda(), attention_mask=mask.cuda(), labels=labels.to(dtype).to(where))
        assert torch.equal(_bits(mixed.loss), _bits(out.loss))
    # the tuples
    loss_t, prune_t = model(input_ids=ids, attention_mask=mask, labels=labels, return_dict=False)
    assert torch.equal(_bits(loss_t), _bits(out.loss)) and torch.equal(prune_t, out.pruning_logits)
    (only,) = model(input_ids=ids, attention_mask=mask, return_dict=False)
    assert torch.equal(only, out.pruning_logits)
    # no mask on a full batch = an all-ones mask
    full_ids, full_labels = ids[:, :28].contiguous(), labels[:, :28].contiguous()
    for dev in ("cpu", "cuda"):
        a = model(input_ids=full_ids.to(dev), labels=full_labels.to(dev))
        b = model(input_ids=full_ids.to(dev), attention_mask=torch.ones_like(full_ids).to(dev), labels=full_labels.to(dev))
        assert torch.equal(_bits(a.loss), _bits(b.loss)) and torch.isfinite(a.loss)
        want_full = lm.token_ce_padded(a.pruning_logits.cpu().numpy(), full_labels.numpy(), None)[0]
        _assert_within_one_ulp(a.loss.cpu().numpy(), want_full, "token loss, no mask")
    # a mask without any active position: exactly 0.0; active positions that are all -100: NaN
    for dev in ("cpu", "cuda"):
        none_active = model(input_ids=ids[:3].to(dev), attention_mask=torch.zeros_like(mask[:3]).to(dev), labels=labels[:3].to(dev))
        assert _bits(none_active.loss).item() == 0 and none_active.loss.is_cuda
        ignored = model(input_ids=ids.to(dev), attention_mask=mask.to(dev), labels=torch.full_like(labels, -100).to(dev))
        assert torch.isnan(ignored.loss)
    # errors
    with pytest.raises(ValueError):
        model(input_ids=ids, attention_mask=mask, labels=labels[:, :-1])
    with pytest.raises(ValueError):
        model(input_ids=ids, attention_mask=mask, labels=labels[0])
    with pytest.raises(TypeError):
        model(input_ids=ids, attention_mask=mask, labels=labels.float())
    bad = labels.clone()
    bad[1, 3] = 2
    with pytest.raises(IndexError, match="row 1, column 3"):
        model(input_ids=ids.cuda(), attention_mask=mask.cuda(), labels=bad)
    assert torch.equal(_bits(model(input_ids=ids, attention_mask=mask, labels=labels).loss), _bits(out.loss))


@pytest.mark.parametrize("which,num_labels", [("rank1", 1), ("rank3", 3)])
def test_ranking_loss(models, which, num_labels):
    dims, built = models
    model = built[which]
    ids, mask = _ragged_inputs(dims)
    rng = np.random.default_rng(6)
    extras = dict(output_hidden_states=True, output_attentions=True) if which == "rank1" else dict(output_hidden_states=True)
    if num_labels == 1:
        labels = torch.from_numpy(rng.integers(0, 2, size=ids.shape[0]))  # integer 0 / 1: the forward takes labels.float()
    else:
        labels = torch.from_numpy(np.where(rng.random(ids.shape[0]) < 0.2, -100, rng.integers(0, num_labels, size=ids.shape[0])))
    plain = model(input_ids=ids, attention_mask=mask, **extras)
    assert plain.loss is None and plain.ranking_logits.shape == (ids.shape[0], num_labels)
    out = model(input_ids=ids, attention_mask=mask, labels=labels, **extras)
    _assert_same_outputs(out, plain)
    assert out.logits is out.ranking_logits and out.loss.shape == () and out.loss.dtype == torch.float32 and out.loss.is_cuda
    rank = out.ranking_logits.cpu()
    if num_labels == 1:
        want = lm.rank_bce(rank.numpy(), labels.float().numpy())[0]
        ref32 = float(torch.nn.BCEWithLogitsLoss()(rank.view(-1), labels.float()))
    else:
        want = lm.rank_ce(rank.numpy(), labels.numpy())[0]
        ref32 = float(torch.nn.CrossEntropyLoss()(rank.view(-1, num_labels), labels.view(-1)))
    _assert_within_one_ulp(out.loss.cpu().numpy(), want, which)
    _assert_near_torch(float(out.loss), ref32, want, f"forward {which} loss hidden={dims.hidden_size}")
    on_device = model(input_ids=ids.cuda(), attention_mask=mask.cuda(), labels=labels.cuda())
    assert torch.equal(_bits(on_device.loss), _bits(out.loss)) and torch.equal(on_device.ranking_logits, out.ranking_logits)
    column = model(input_ids=ids.cuda(), attention_mask=mask.cuda(), labels=labels.view(-1, 1))  # labels.view(-1) of any shape that fits
    assert torch.equal(_bits(column.loss), _bits(out.loss))
    loss_t, rank_t, prune_t = model(input_ids=ids, attention_mask=mask, labels=labels, return_dict=False)
    assert torch.equal(_bits(loss_t), _bits(out.loss)) and torch.equal(rank_t, out.ranking_logits) and torch.equal(prune_t, out.pruning_logits)
    assert len(model(input_ids=ids, attention_mask=mask, return_dict=False)) == 2
    # no mask on a full batch = an all-ones mask
    full_ids = ids[:, :28].contiguous()
    a = model(input_ids=full_ids.cuda(), labels=labels)
    b = model(input_ids=full_ids.cuda(), attention_mask=torch.ones_like(full_ids).cuda(), labels=labels)
    assert torch.equal(_bits(a.loss), _bits(b.loss)) and torch.isfinite(a.loss)
    with pytest.raises(ValueError):
        model(input_ids=ids, attention_mask=mask, labels=labels[:-1])
    with pytest.raises(ValueError):
        model(input_ids=ids, attention_mask=mask, labels=torch.zeros(ids.shape, dtype=torch.int64))
    if num_labels > 1:
        with pytest.raises(TypeError):
            model(input_ids=ids, attention_mask=mask, labels=labels.float())
        bad = labels.clone()
        bad[4] = num_labels
        with pytest.raises(IndexError, match="row 4, column 0"):
            model(input_ids=ids, attention_mask=mask, labels=bad)
    else:
        soft = torch.from_numpy(rng.random(ids.shape[0]).astype(np.float32))
        got = model(input_ids=ids, attention_mask=mask, labels=soft)
        _assert_within_one_ulp(got.loss.cpu().numpy(), lm.rank_bce(rank.numpy(), soft.numpy())[0], "soft BCE targets")
