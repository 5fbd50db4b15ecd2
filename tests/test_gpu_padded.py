"""The padded boundary on the device: op_pack_padded / op_unpack_padded against packing.pack_padded / unpack_to_padded (exact
equality), the two device-side checks against the host's errors, and OpenProvenceModel.forward on device tensors against the
same call on CPU tensors (bit-identical outputs, and no visit to the host packing functions)."""

from __future__ import annotations

import ctypes

import numpy as np
import pytest
import torch

from helpers import CharTokenizer, load_golden, state_from_fixture

pytestmark = pytest.mark.gpu

VOCAB = 1000
# (rows, width): up to a few thousand rows; widths 1, 7, 64, 513 and 2048 (513 and 7: rows that start off the 16-byte grid)
SHAPES = [(3000, 1), (3001, 7), (2500, 64), (257, 513), (5, 513), (64, 2048), (1, 2048), (1, 1)]


@pytest.fixture(scope="module")
def enc():
    """A handle without weights: the padded calls need only the vocabulary size."""

    from open_provence_amd.engine import HipEncoder
    from open_provence_amd.synthetic import named_dims

    encoder = HipEncoder(named_dims("xsmall", vocab_size=VOCAB, num_layers=1), device="cuda:0")
    yield encoder
    encoder.close()


def _batch(rng, rows, width, *, ids_dtype=torch.int64, mask_dtype=torch.int64):
    """Random right-padded batch on the CPU with empty rows, full rows, and garbage (out-of-range) ids under the padding."""

    lengths = rng.integers(0, width + 1, size=rows)
    lengths[rng.random(rows) < 0.1] = 0
    lengths[rng.random(rows) < 0.1] = width
    cols = np.arange(width)[None, :]
    valid = cols < lengths[:, None]
    ids = rng.integers(0, VOCAB, size=(rows, width))
    ids = np.where(valid, ids, rng.choice([-7, VOCAB, VOCAB + 123456, 3], size=(rows, width)))
    mask = None if mask_dtype is None else torch.from_numpy(valid.astype(np.int64)).to(mask_dtype)
    return torch.from_numpy(ids).to(ids_dtype), mask, lengths


def _assert_pack_equals_host(enc, ids, mask):
    from open_provence_amd.packing import pack_padded

    want_ids, want_cu, want_max = pack_padded(ids, mask)
    enc.check_ids(want_ids)
    got_ids, got_cu, got_cu_host, got_max = enc.pack_padded_device(ids.cuda(), None if mask is None else mask.cuda())
    assert got_ids.dtype == torch.int32 and got_cu.dtype == torch.int32 and got_cu_host.dtype == np.int32
    assert got_ids.device == enc.device and got_cu.device == enc.device and got_ids.is_contiguous()
    assert np.array_equal(got_cu_host, want_cu)
    assert np.array_equal(got_cu.cpu().numpy(), want_cu)
    assert np.array_equal(got_ids.cpu().numpy(), want_ids)
    assert got_max == want_max and isinstance(got_max, int)


@pytest.mark.parametrize("ids_dtype", [torch.int32, torch.int64])
@pytest.mark.parametrize("mask_dtype", [torch.bool, torch.int32, torch.int64])
def test_pack_equals_the_host_packing(enc, ids_dtype, mask_dtype):
    rng = np.random.default_rng(11)
    for rows, width in SHAPES:
        ids, mask, _ = _batch(rng, rows, width, ids_dtype=ids_dtype, mask_dtype=mask_dtype)
        _assert_pack_equals_host(enc, ids, mask)


@pytest.mark.parametrize("ids_dtype", [torch.int32, torch.int64])
def test_pack_without_a_mask_takes_every_position(enc, ids_dtype):
    rng = np.random.default_rng(12)
    for rows, width in SHAPES:
        ids = torch.from_numpy(rng.integers(0, VOCAB, size=(rows, width))).to(ids_dtype)
        _assert_pack_equals_host(enc, ids, None)


def test_pack_edge_rows_other_dtypes_and_views(enc):
    from open_provence_amd.packing import pack_padded

    rng = np.random.default_rng(13)
    # all rows empty, all rows full
    ids = torch.from_numpy(rng.integers(0, VOCAB, size=(33, 64)))
    _assert_pack_equals_host(enc, ids, torch.zeros(33, 64, dtype=torch.int64))
    _assert_pack_equals_host(enc, ids, torch.ones(33, 64, dtype=torch.bool))
    # no rows / no columns: nothing is launched
    for shape in ((0, 16), (4, 0), (0, 0)):
        empty = torch.zeros(shape, dtype=torch.int64)
        _assert_pack_equals_host(enc, empty, torch.zeros(shape, dtype=torch.int64))
        _assert_pack_equals_host(enc, empty, None)
    # other mask / id dtypes are converted on the device; a transposed view is made contiguous
    ids, mask, _ = _batch(rng, 40, 96)
    want = pack_padded(ids, mask)
    for m in (mask.to(torch.float32), mask.to(torch.int16), mask.to(torch.uint8), mask.to(torch.float16)):
        got = enc.pack_padded_device(ids.cuda(), m.cuda())
        assert np.array_equal(got[0].cpu().numpy(), want[0]) and np.array_equal(got[2], want[1]) and got[3] == want[2]
    got = enc.pack_padded_device(ids.to(torch.int16).cuda(), mask.cuda())
    assert np.array_equal(got[0].cpu().numpy(), want[0]) and np.array_equal(got[2], want[1])
    got = enc.pack_padded_device(ids.cuda().t().contiguous().t(), mask.cuda().t().contiguous().t())
    assert np.array_equal(got[0].cpu().numpy(), want[0]) and np.array_equal(got[2], want[1])
    # buffers that start 4 / 8 / 1 bytes off the 16-byte grid (contiguous views with a storage offset)
    for ids_dtype, mask_dtype in ((torch.int32, torch.bool), (torch.int64, torch.int32)):
        ids, mask, _ = _batch(rng, 31, 128, ids_dtype=ids_dtype, mask_dtype=mask_dtype)
        ids_off = torch.empty(ids.numel() + 1, dtype=ids_dtype, device="cuda")[1:].view(ids.shape).copy_(ids)
        mask_off = torch.empty(mask.numel() + 1, dtype=mask_dtype, device="cuda")[1:].view(mask.shape).copy_(mask)
        assert ids_off.data_ptr() % 16 != 0 and mask_off.data_ptr() % 16 != 0
        want = pack_padded(ids, mask)
        got = enc.pack_padded_device(ids_off, mask_off)
        assert np.array_equal(got[0].cpu().numpy(), want[0]) and np.array_equal(got[2], want[1]) and got[3] == want[2]
    # shape errors stay ValueError, raised on the host
    with pytest.raises(ValueError):
        enc.pack_padded_device(torch.zeros(8, dtype=torch.int64, device="cuda"), None)
    with pytest.raises(ValueError):
        enc.pack_padded_device(torch.zeros(2, 8, dtype=torch.int64, device="cuda"), torch.ones(2, 7, dtype=torch.int64, device="cuda"))


# -- unpack ------------------------------------------------------------------------------------------------------------------
def _values(rng, total, channels):
    v = rng.standard_normal((total, channels)).astype(np.float32)
    v[rng.random((total, channels)) < 0.2] = -0.0  # the sign of a zero VALUE survives; padding is +0.0
    v[rng.random((total, channels)) < 0.1] = 0.0
    return torch.from_numpy(v if channels == 2 else v[:, 0].copy())


def _bits(t):
    return t.contiguous().view(torch.int32)


@pytest.mark.parametrize("channels", [1, 2])
def test_unpack_equals_the_host_scatter_bit_for_bit(enc, channels):
    from open_provence_amd.packing import unpack_to_padded

    rng = np.random.default_rng(21 + channels)
    for rows, width in SHAPES + [(0, 16), (7, 0), (3, 5)]:
        _, _, lengths = _batch(rng, rows, width)
        if (rows, width) == (3, 5):
            lengths[:] = 0  # empty rows only: nothing to read
        cu_np = np.zeros(rows + 1, dtype=np.int32)
        np.cumsum(lengths, out=cu_np[1:])
        values = _values(rng, int(cu_np[-1]), channels).cuda()
        cu = torch.from_numpy(cu_np).cuda()
        want = unpack_to_padded(values, cu_np, width)
        got = enc.unpack_padded_device(values, cu, rows, width)
        assert got.shape == want.shape and got.dtype == torch.float32 and got.device == values.device
        assert torch.equal(_bits(got), _bits(want)), (rows, width)
        if got.numel():
            assert bool((_bits(got)[torch.from_numpy(np.arange(width)[None, :] >= lengths[:, None]).cuda()] == 0).all())


@pytest.mark.parametrize("channels", [1, 2])
def test_unpack_writes_every_element_of_a_nan_filled_destination(enc, channels):
    from open_provence_amd.packing import unpack_to_padded

    rng = np.random.default_rng(31 + channels)
    for rows, width in [(257, 513), (3001, 7), (64, 2048), (3, 1), (1, 3)]:
        _, _, lengths = _batch(rng, rows, width)
        cu_np = np.zeros(rows + 1, dtype=np.int32)
        np.cumsum(lengths, out=cu_np[1:])
        total = int(cu_np[-1])
        buffer = torch.from_numpy(rng.standard_normal((max(total, 1), channels)).astype(np.float32)).cuda()  # (never a NULL source)
        values = buffer[:total]
        cu = torch.from_numpy(cu_np).cuda()
        # 16-byte aligned, and 8 / 4 bytes off the grid (the kernel's narrow-store path)
        for offset in (0, 2, 1):
            backing = torch.full((rows * width * channels + offset + 4,), float("nan"), dtype=torch.float32, device="cuda")
            dst = backing[offset: offset + rows * width * channels]
            code = enc.lib.op_unpack_padded(enc._handle, ctypes.c_void_p(buffer.data_ptr()), ctypes.c_void_p(cu.data_ptr()), rows, width,
                                            channels, ctypes.c_void_p(dst.data_ptr()), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
            assert code == 0, enc.lib.op_last_error(enc._handle)
            torch.cuda.synchronize()
            assert not bool(torch.isnan(dst).any()), (rows, width, offset)
            assert bool(torch.isnan(backing[:offset]).all()) and bool(torch.isnan(backing[offset + dst.numel():]).all())  # and nothing else
            assert torch.equal(_bits(dst.view(rows, width, channels)), _bits(unpack_to_padded(values, cu_np, width)))


def test_unpack_to_a_narrower_width_drops_the_positions_beyond_it(enc):
    lengths = np.array([5, 0, 9, 3, 12], dtype=np.int64)
    cu_np = np.zeros(6, dtype=np.int32)
    np.cumsum(lengths, out=cu_np[1:])
    values = torch.arange(1, int(cu_np[-1]) * 2 + 1, dtype=torch.float32).view(-1, 2)
    got = enc.unpack_padded_device(values.cuda(), torch.from_numpy(cu_np).cuda(), 5, 6).cpu()
    want = torch.zeros(5, 6, 2)
    for r, n in enumerate(lengths):
        keep = min(int(n), 6)
        want[r, :keep] = values[cu_np[r]: cu_np[r] + keep]
    assert torch.equal(got, want)


# -- the two checks ----------------------------------------------------------------------------------------------------------
def _c_pack(enc, ids, mask):
    """op_pack_padded itself -> (code, report, message)."""

    from open_provence_amd import _lib

    codes = {torch.int32: _lib.OP_INT_I32, torch.int64: _lib.OP_INT_I64, torch.uint8: _lib.OP_INT_U8}
    ids, mask = ids.cuda().contiguous(), (None if mask is None else mask.cuda().contiguous())
    rows, width = ids.shape
    packed = torch.empty(rows * width, dtype=torch.int32, device="cuda")
    cu = torch.empty(rows + 1, dtype=torch.int32, device="cuda")
    cu_host = np.zeros(rows + 1, dtype=np.int32)
    report = _lib.OpPaddedReport()
    report.struct_bytes = ctypes.sizeof(_lib.OpPaddedReport)
    code = enc.lib.op_pack_padded(enc._handle, ctypes.c_void_p(ids.data_ptr()), codes[ids.dtype],
                                  ctypes.c_void_p(mask.data_ptr()) if mask is not None else None, codes[mask.dtype] if mask is not None else 0,
                                  rows, width, ctypes.c_void_p(packed.data_ptr()), ctypes.c_void_p(cu.data_ptr()),
                                  cu_host.ctypes.data_as(ctypes.c_void_p), ctypes.byref(report), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    return code, report, _lib.last_error(enc.lib, enc._handle)


def _clean(rows=300, width=200, seed=41):
    rng = np.random.default_rng(seed)
    lengths = rng.integers(8, width + 1, size=rows)
    valid = np.arange(width)[None, :] < lengths[:, None]
    ids = np.where(valid, rng.integers(0, VOCAB, size=(rows, width)), 0)
    return torch.from_numpy(ids), torch.from_numpy(valid.astype(np.int64)), lengths


@pytest.mark.parametrize("mask_dtype", [torch.uint8, torch.int32, torch.int64])
def test_a_hole_or_left_padding_is_refused_with_its_position(enc, mask_dtype):
    from open_provence_amd.packing import pack_padded

    ids, mask, lengths = _clean()
    assert _c_pack(enc, ids, mask.to(mask_dtype))[0] == 0
    # a hole: the first zero that has a one behind it is the offender
    row = 137
    col = int(lengths[row]) // 2
    holed = mask.clone()
    holed[row, col] = 0
    code, report, message = _c_pack(enc, ids, holed.to(mask_dtype))
    assert code == -1 and report.status == 1 and (report.mask_row, report.mask_col) == (row, col)
    assert (report.id_row, report.id_col) == (-1, -1)
    assert f"row {row}" in message and f"column {col}" in message
    # two faulty rows: the first in row-major order is named, whatever its column
    holed[21, 5] = 0
    code, report, _ = _c_pack(enc, ids, holed.to(mask_dtype))
    assert code == -1 and report.status == 1 and (report.mask_row, report.mask_col) == (21, 5)
    # left padding: column 0 of the first row that is not full
    flipped = torch.flip(mask, dims=[1])
    first = int(np.argmax(lengths < mask.shape[1]))
    code, report, _ = _c_pack(enc, ids, flipped.to(mask_dtype))
    assert code == -1 and report.status == 1 and (report.mask_row, report.mask_col) == (first, 0)
    # a one behind the padding, in the last column
    tail = mask.clone()
    short = int(np.argmax(lengths < mask.shape[1] - 1))
    tail[short, -1] = 1
    code, report, _ = _c_pack(enc, ids, tail.to(mask_dtype))
    assert code == -1 and report.status == 1 and (report.mask_row, report.mask_col) == (short, int(lengths[short]))
    # the Python layer raises what the host path raises
    for bad in (holed, flipped, tail):
        with pytest.raises(NotImplementedError, match="right-padded"):
            pack_padded(ids, bad.to(mask_dtype))
        with pytest.raises(NotImplementedError, match="right-padded"):
            enc.pack_padded_device(ids.cuda(), bad.to(mask_dtype).cuda())


@pytest.mark.parametrize("ids_dtype", [torch.int32, torch.int64])
@pytest.mark.parametrize("bad_value", [VOCAB, -1])
def test_an_id_outside_the_table_is_refused_with_row_col_and_value(enc, ids_dtype, bad_value):
    from open_provence_amd.packing import pack_padded

    ids, mask, lengths = _clean(seed=43)
    row = 211
    col = int(lengths[row]) - 1  # the last valid position of the row
    bad = ids.clone()
    bad[row, col] = bad_value
    code, report, message = _c_pack(enc, bad.to(ids_dtype), mask)
    assert code == -1 and report.status == 2
    assert (report.id_row, report.id_col, report.id_value) == (row, col, bad_value)
    assert (report.mask_row, report.mask_col) == (-1, -1)
    assert f"row {row}" in message and f"column {col}" in message and str(bad_value) in message
    with pytest.raises(IndexError, match="out of range"):
        enc.check_ids(pack_padded(bad.to(ids_dtype), mask)[0])
    with pytest.raises(IndexError, match="out of range") as caught:
        enc.pack_padded_device(bad.to(ids_dtype).cuda(), mask.cuda())
    assert str(bad_value) in str(caught.value) and f"row {row}" in str(caught.value)
    # an earlier offender wins, in row-major order; without a mask every position counts
    bad[3, 7] = VOCAB + 5
    code, report, _ = _c_pack(enc, bad.to(ids_dtype), mask)
    assert (report.status, report.id_row, report.id_col, report.id_value) == (2, 3, 7, VOCAB + 5)
    code, report, _ = _c_pack(enc, bad.to(ids_dtype), None)
    assert (report.status, report.id_row, report.id_col, report.id_value) == (2, 3, 7, VOCAB + 5)
    # the same bad ids under the padding are accepted, as on the host
    under = ids.clone()
    short = int(np.argmax(lengths < ids.shape[1]))
    under[short, int(lengths[short]):] = bad_value
    code, report, _ = _c_pack(enc, under.to(ids_dtype), mask)
    assert code == 0 and report.status == 0 and report.total_tokens == int(lengths.sum()) and report.max_seqlen == int(lengths.max())
    got = enc.pack_padded_device(under.to(ids_dtype).cuda(), mask.cuda())
    assert np.array_equal(got[0].cpu().numpy(), pack_padded(under, mask)[0])
    if ids_dtype == torch.int64:  # a value beyond 32 bits is reported whole
        bad[3, 7] = 1 << 40
        code, report, _ = _c_pack(enc, bad, mask)
        assert (report.status, report.id_row, report.id_col, report.id_value) == (2, 3, 7, 1 << 40)


def test_both_faults_together_raise_the_mask_error(enc):
    ids, mask, lengths = _clean(seed=47)
    ids[5, 2] = VOCAB  # the id fault comes first in row-major order: the mask fault still wins
    mask[90, 3] = 0
    code, report, message = _c_pack(enc, ids, mask)
    assert code == -1 and report.status == 3
    assert (report.mask_row, report.mask_col) == (90, 3) and (report.id_row, report.id_col, report.id_value) == (5, 2, VOCAB)
    assert "ones-then-zeros" in message and "embedding table" in message
    with pytest.raises(NotImplementedError, match="right-padded"):
        enc.pack_padded_device(ids.cuda(), mask.cuda())
    # the handle is usable afterwards
    ids[5, 2] = 1
    mask[90, 3] = 1
    assert _c_pack(enc, ids, mask)[0] == 0


# -- forward() ---------------------------------------------------------------------------------------------------------------
def _synthetic_model(name, cls=None, **kw):
    from open_provence_amd.config import OpenProvenceConfig
    from open_provence_amd.modeling import OpenProvenceModel
    from open_provence_amd.synthetic import named_dims, refinit_state_dict

    dims = named_dims(name, vocab_size=2048, num_layers=3)
    cfg = OpenProvenceConfig(base_model_config=dims.to_base_model_config(), tokenizer_name_or_path="char-tokenizer",
                             pruning_config={"hidden_size": dims.hidden_size}, max_length=512, num_labels=1,
                             pruning_hidden_state="post_final_norm")
    state = refinit_state_dict(dims, seed=5)
    model = (cls or OpenProvenceModel)(cfg, device="cuda:0", tokenizer=CharTokenizer(), state_dict=state, calibrate=False, **kw)
    return model, dims, cfg, state


def _ragged_inputs(dims, rows=24, width=160, seed=3):
    from open_provence_amd.synthetic import pad_rows, synth_pair_batch

    rng = np.random.default_rng(seed)
    lengths = rng.integers(28, width + 1, size=rows).tolist()
    lengths[0], lengths[1] = width, 28
    return pad_rows(synth_pair_batch(dims, rows, lengths, seed=seed))


def _assert_same_output(got, want):
    assert torch.equal(got.ranking_logits, want.ranking_logits) and torch.equal(got.pruning_logits, want.pruning_logits)
    assert got.logits is got.ranking_logits
    assert (got.hidden_states is None) == (want.hidden_states is None)
    if want.hidden_states is not None:
        assert len(got.hidden_states) == len(want.hidden_states)
        for a, b in zip(got.hidden_states, want.hidden_states):
            assert torch.equal(a, b)


@pytest.mark.parametrize("name,hidden", [("xsmall", 256), ("base", 512)])  # the row path and the panel path
def test_forward_on_device_tensors_equals_forward_on_cpu_tensors(monkeypatch, name, hidden):
    from open_provence_amd import modeling
    from open_provence_amd.modeling import OpenProvenceForTokenClassification

    model, dims, cfg, state = _synthetic_model(name)
    assert dims.hidden_size == hidden and model.encoder.effective_policy()["kernel_set"]
    ids, mask = _ragged_inputs(dims)
    want = model(input_ids=ids, attention_mask=mask)
    want_h = model(input_ids=ids, attention_mask=mask, output_hidden_states=True)
    assert want.pruning_logits.shape == (ids.shape[0], ids.shape[1], 2) and len(want_h.hidden_states) == dims.num_layers + 1

    calls = {"pack": 0, "unpack": 0}
    host_pack, host_unpack = modeling.pack_padded, modeling.unpack_to_padded

    def counted_pack(*a, **k):
        calls["pack"] += 1
        return host_pack(*a, **k)

    def counted_unpack(*a, **k):
        calls["unpack"] += 1
        return host_unpack(*a, **k)

    monkeypatch.setattr(modeling, "pack_padded", counted_pack)
    monkeypatch.setattr(modeling, "unpack_to_padded", counted_unpack)
    ids_d, mask_d = ids.cuda(), mask.cuda()
    _assert_same_output(model(input_ids=ids_d, attention_mask=mask_d), want)
    _assert_same_output(model(input_ids=ids_d, attention_mask=mask_d, output_hidden_states=True), want_h)
    # every id / mask type of the boundary, and a float mask
    for i_t, m_t in ((torch.int32, torch.bool), (torch.int32, torch.int32), (torch.int64, torch.bool), (torch.int64, torch.float32)):
        _assert_same_output(model(input_ids=ids_d.to(i_t), attention_mask=mask_d.to(m_t), token_type_ids=torch.zeros_like(ids_d)), want)
    rank_t, prune_t = model(input_ids=ids_d, attention_mask=mask_d, return_dict=False)
    assert torch.equal(rank_t, want.ranking_logits) and torch.equal(prune_t, want.pruning_logits)
    assert calls == {"pack": 0, "unpack": 0}  # the device path never reached the host packing
    # no mask = full rows
    full_ids = ids[:, :28].contiguous()
    want_full = model(input_ids=full_ids)
    assert calls == {"pack": 1, "unpack": 1}  # ... and the CPU-tensor call still does
    _assert_same_output(model(input_ids=full_ids.cuda()), want_full)
    # a mixed call (ids on the device, mask on the host) keeps the host path
    _assert_same_output(model(input_ids=ids_d, attention_mask=mask), want)
    assert calls == {"pack": 2, "unpack": 2}

    # on a non-default current stream
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        got = model(input_ids=ids_d, attention_mask=mask_d, output_hidden_states=True)
    side.synchronize()
    _assert_same_output(got, want_h)

    # an empty batch
    for shape in ((0, 16),):
        empty_ids, empty_mask = torch.zeros(shape, dtype=torch.int64), torch.zeros(shape, dtype=torch.int64)
        want_e = model(input_ids=empty_ids, attention_mask=empty_mask)
        got_e = model(input_ids=empty_ids.cuda(), attention_mask=empty_mask.cuda())
        assert got_e.pruning_logits.shape == want_e.pruning_logits.shape == (shape[0], shape[1], 2)
        assert got_e.ranking_logits.shape == want_e.ranking_logits.shape
        assert torch.equal(got_e.pruning_logits, want_e.pruning_logits)

    # the errors of the boundary, from device tensors
    with pytest.raises(NotImplementedError):
        model(input_ids=ids_d, attention_mask=torch.flip(mask_d, dims=[1]))
    bad = ids_d.clone()
    bad[1, 3] = dims.vocab_size
    with pytest.raises(IndexError):
        model(input_ids=bad, attention_mask=mask_d)
    with pytest.raises(ValueError):
        model(input_ids=ids_d, attention_mask=mask_d[:, :-1])
    with pytest.raises(ValueError):
        model(input_ids=ids_d[0], attention_mask=mask_d[0])
    _assert_same_output(model(input_ids=ids_d, attention_mask=mask_d), want)  # and the model still works

    # the token-classification wrapper goes through the same forward
    tok_model = OpenProvenceForTokenClassification(cfg, device="cuda:0", tokenizer=CharTokenizer(), state_dict=state, calibrate=False)
    before = dict(calls)
    tout = tok_model(input_ids=ids_d, attention_mask=mask_d)
    assert calls == before
    assert tout.logits.shape[-1] == 2 and torch.equal(tout.logits, want.pruning_logits) and torch.equal(tout.ranking_logits, want.ranking_logits)
    (only,) = tok_model(input_ids=ids_d, attention_mask=mask_d, return_dict=False)
    assert torch.equal(only, want.pruning_logits)


def test_device_tensor_forward_does_not_reach_the_host_packing(monkeypatch):
    """With the host functions patched to raise, a device-tensor call goes through; a CPU-tensor call raises."""

    from open_provence_amd import modeling

    model, dims, _, _ = _synthetic_model("xsmall")
    ids, mask = _ragged_inputs(dims, rows=6, width=64)
    want = model(input_ids=ids, attention_mask=mask)

    def refuse(*a, **k):
        raise AssertionError("host packing reached")

    monkeypatch.setattr(modeling, "pack_padded", refuse)
    monkeypatch.setattr(modeling, "unpack_to_padded", refuse)
    _assert_same_output(model(input_ids=ids.cuda(), attention_mask=mask.cuda()), want)
    with pytest.raises(AssertionError, match="host packing reached"):
        model(input_ids=ids, attention_mask=mask)


def test_first_device_tensor_forward_of_a_calibrated_model_runs_its_audit():
    from open_provence_amd.config import OpenProvenceConfig
    from open_provence_amd.modeling import OpenProvenceModel

    arrays, meta = load_golden("g7_xsmall_refinit")
    cfg = OpenProvenceConfig(
        base_model_config=meta["base_model_config"], tokenizer_name_or_path="char-tokenizer",
        pruning_config={"hidden_size": meta["base_model_config"]["hidden_size"]}, max_length=8192, num_labels=1,
        pruning_hidden_state="post_final_norm",
    )
    state = state_from_fixture(arrays, meta)
    ids = torch.from_numpy(arrays["input_ids"])
    mask = torch.from_numpy(arrays["attention_mask"])
    outs = []
    for on_device in (True, False):
        model = OpenProvenceModel(cfg, device="cuda:0", tokenizer=CharTokenizer(), state_dict=state, calibrate=True)
        cal = model.encoder.calibration
        assert cal is not None and cal["chosen_set"] != cal["default_set"] and model.encoder.audit_pending
        out = model(input_ids=ids.cuda() if on_device else ids, attention_mask=mask.cuda() if on_device else mask)
        assert not model.encoder.audit_pending
        audit = model.encoder.calibration["audit"]
        assert audit["passed"] and audit["rows"] == ids.shape[0] and audit["tokens"] == int(mask.sum())
        outs.append(out)
    _assert_same_output(outs[0], outs[1])
