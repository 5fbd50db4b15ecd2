"""forward() under ANY attention mask (left padding, holes) on the fp32 kernels: ``op_forward_masked`` against the CPU oracle.

The bound is the one of tests/test_gpu_fp32_set.py, against the fp64 oracle evaluated at run time on the same batch:

    max(4 x e_ref, 16 ulp of the quantity's largest magnitude),   e_ref = |fp32 oracle - fp64 oracle|

on ``logits`` (the pruning logits at ``mask == 1`` and the ranking logits of every row with a one) and ``keep_prob`` (at
``mask == 1``); nothing else is left out.  Pruning logits at ``mask == 0`` and both outputs of an all-zero row are exact
zeros.  Each case prints ``err / e_ref``.

Models: the SMALL table of that module, restated in tests/masked_model.py with the mask cases (width 200 crosses the 64-key
tile and the 128-row tile and is no multiple of 16; widths 77 and 1).  tests/test_masked_model.py shows on the CPU that these
inputs notice each mistake a kernel could make.  Then the bit identities the call promises, its workspace, and the behaviour of
forward() around it."""

from __future__ import annotations

import ctypes
import functools

import numpy as np
import pytest
import torch

import masked_model as mm
import workspace_utils as wu
from helpers import CharTokenizer

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _state(case):
    from open_provence_amd.synthetic import refinit_state_dict, synth_state_dict

    return (refinit_state_dict if case[7] == "refinit" else synth_state_dict)(mm.small_dims(*case[:6]), 5)


def _encoder(case, kernel_set="bf16x3", attention_masks="any", **kw):
    from open_provence_amd.engine import HipEncoder

    enc = HipEncoder(mm.small_dims(*case[:6]), device="cuda:0", kernel_set=kernel_set if kernel_set == "fp32" else None,
                     attention_masks=attention_masks, prune_pre_final_norm=case[6], **kw)
    try:
        enc.load_state_dict(_state(case), calibrate=False, kernel_set=kernel_set)
        assert enc.effective_policy()["kernel_set"] == kernel_set
    except BaseException:
        enc.close()
        raise
    return enc


def _check(label, prune, rank, mask, ref: mm.Reference):
    prune, rank = prune.cpu(), rank.cpu()
    on = mask.bool()
    assert prune.shape == tuple(mask.shape) + (2,) and prune.dtype == torch.float32 and rank.shape[0] == mask.shape[0]
    assert bool((prune[~on].view(torch.int32) == 0).all()), f"{label}: a pruning logit at mask == 0 is not +0.0"
    dead = ~on.any(1)
    assert bool((rank[dead].view(torch.int32) == 0).all()), f"{label}: the ranking logits of an all-zero row are not +0.0"
    got = mm.compared(prune, rank, mask)
    for name, want in ref.entries.items():
        assert got[name].shape == want.shape and bool(torch.isfinite(got[name]).all()), f"{label}: {name} is not finite"
        err = float((got[name] - want).abs().max()) if want.numel() else 0.0
        e_ref, bound = ref.e_ref[name], ref.bound(name)
        print(f"[masked] {label:52s} {name:10s} err {err:.3e}  e_ref {e_ref:.3e}  err/e_ref {err / max(e_ref, 1e-30):7.2f}  bound {bound:.3e}")
        assert err <= bound, f"{label}: {name} is {err:.3e} from the fp64 oracle, bound {bound:.3e} (e_ref {e_ref:.3e})"


# -- against the oracle ----------------------------------------------------------------------------------------------------------------
PAIRS = [(case, 200) for case in mm.SMALL] + [(mm.SMALL[0], 77), (mm.SMALL[1], 77), (mm.SMALL[0], 1), (mm.SMALL[1], 1)]


@pytest.mark.parametrize("case,width", PAIRS, ids=lambda v: mm.case_id(v) if isinstance(v, tuple) else f"L{v}")
def test_every_mask_case_matches_the_oracle(case, width):
    torch.set_num_threads(16)
    ids, mask, _ = mm.batch(width)
    ref = mm.Reference(_state(case), mm.small_dims(*case[:6]), ids, mask, case[6])
    enc = _encoder(case)
    try:
        prune, rank = enc.forward_masked(ids, mask)
        torch.cuda.synchronize()
        _check(f"{mm.case_id(case)} L{width}", prune, rank, mask, ref)
    finally:
        enc.close()


# -- bit identities ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [mm.SMALL[0], mm.SMALL[5]], ids=mm.case_id)
def test_a_right_padded_mask_gives_the_bits_of_the_fp32_set(case):
    """op_forward_masked on ones-then-zeros rows = kernel set "fp32"'s forward_packed of the packed rows, at valid positions and
    in the ranking logits -- on a handle that runs another set, and on one that runs "fp32" itself."""

    from open_provence_amd.packing import pack_padded

    ids, mask = mm.prefix_batch(200)
    ids_np, cu_np, max_len = pack_padded(ids, mask)
    f32 = _encoder(case, kernel_set="fp32")
    other = _encoder(case, kernel_set="bf16x3")
    try:
        want_prune, want_rank = f32.forward_packed(torch.from_numpy(ids_np).cuda(), torch.from_numpy(cu_np).cuda(), cu_np, max_len)[:2]
        for name, enc in (("fp32 handle", f32), ("bf16x3 handle", other)):
            prune, rank = enc.forward_masked(ids, mask)
            torch.cuda.synchronize()
            assert torch.equal(prune[mask.bool().cuda()], want_prune), f"{name}: pruning logits at valid positions"
            assert torch.equal(rank, want_rank), f"{name}: ranking logits"
            assert bool((prune[~mask.bool().cuda()].view(torch.int32) == 0).all())
    finally:
        f32.close()
        other.close()


def test_a_row_alone_equals_the_row_in_the_batch_and_chunking_changes_nothing():
    case = mm.SMALL[3]
    ids, mask, names = mm.batch(200)
    enc = _encoder(case)
    chunked = _encoder(case, chunk_rows=256)  # (one dense row of 200 positions per chunk)
    try:
        prune, rank = enc.forward_masked(ids, mask)
        prune_c, rank_c = chunked.forward_masked(ids, mask)
        assert torch.equal(prune, prune_c) and torch.equal(rank, rank_c), "chunk_rows = 256 changes the bits"
        for s in range(0, len(names), 3):
            p1, r1 = enc.forward_masked(ids[s: s + 1], mask[s: s + 1])
            assert torch.equal(p1[0], prune[s]) and torch.equal(r1[0], rank[s]), f"row {s} ({names[s]})"
    finally:
        enc.close()
        chunked.close()


def test_two_streams_give_the_same_bits():
    case = mm.SMALL[4]
    ids, mask, _ = mm.batch(200)
    enc = _encoder(case)
    try:
        want = enc.forward_masked(ids, mask)
        torch.cuda.synchronize()
        need = int(enc.lib.op_masked_workspace_bytes(enc._handle, *ids.shape)) + 256
        streams = [torch.cuda.Stream(), torch.cuda.Stream()]
        spaces = [torch.empty(need, dtype=torch.uint8, device="cuda:0") for _ in streams]
        outs = []
        ids_d, mask_d = ids.cuda(), mask.cuda()
        torch.cuda.synchronize()
        for stream, space in zip(streams, spaces):
            with torch.cuda.stream(stream):
                outs.append(enc.forward_masked(ids_d, mask_d, workspace=space))
        torch.cuda.synchronize()
        for got in outs:
            assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    finally:
        enc.close()


# -- the workspace -------------------------------------------------------------------------------------------------------------------
def _direct(enc, ids, mask, fill, layout_enc=None):
    """op_forward_masked itself on a workspace of exactly op_masked_workspace_bytes and on outputs that are all views between
    canaries; ``fill``: zeros, or a poison per region kind (float planes NaN / huge bytes, index regions a wrong but in-range
    entry: the rule of workspace_utils) -> (prune, rank).  ``layout_enc``: a handle of the same dims that runs kernel set "fp32"
    and so reports the inner forward workspace's regions, where ``enc`` itself runs another set."""

    layout_enc = layout_enc or enc

    n_rows, width = (int(v) for v in ids.shape)
    nl = enc.dims.num_labels
    need = int(enc.lib.op_masked_workspace_bytes(enc._handle, n_rows, width))
    # the call's own regions in front (cu_seqlens, the id check's word, the row means of v), then a forward workspace of kernel
    # set "fp32" -- the layout this fp32 handle reports for the dense geometry
    assert need == int(layout_enc.lib.op_masked_workspace_bytes(layout_enc._handle, n_rows, width))
    forward_need = int(layout_enc.lib.op_workspace_bytes(layout_enc._handle, n_rows, n_rows * width, width))
    head = need - forward_need
    assert need % 256 == 0 and head >= 256 * 3
    mem = wu.canaried(need, enc.device)
    mem.view.zero_()
    if fill != "zeros":
        byte = wu.NAN_BYTE if fill == "nan" else wu.HUGE_BYTE
        cu_bytes = ((n_rows + 1) * 4 + 255) // 256 * 256
        mem.view[:cu_bytes].view(torch.int32).fill_(1)
        mem.view[cu_bytes: head].fill_(byte)
        sub = wu.ControlledWorkspace(wu.Canaried(mem.backing, mem.view[head:], mem.guard, mem.canary), forward_need,
                                     layout_enc.workspace_layout(n_rows, n_rows * width, width), 1)
        wu.fill_workspace(sub, fill)
    bufs = {"prune": wu.canaried(n_rows * width * 2 * 4, enc.device), "rank": wu.canaried(n_rows * nl * 4, enc.device)}
    ids_d, mask_d = ids.to(torch.int32).cuda().contiguous(), mask.ne(0).cuda().contiguous().view(torch.uint8)
    ids_guard, mask_guard = ids_d.clone(), mask_d.clone()
    from open_provence_amd import _lib

    report = _lib.OpMaskedReport()
    report.struct_bytes = ctypes.sizeof(_lib.OpMaskedReport)
    vp = ctypes.c_void_p
    with torch.cuda.device(enc.device):
        code = enc.lib.op_forward_masked(enc._handle, vp(ids_d.data_ptr()), vp(mask_d.data_ptr()), n_rows, width, vp(mem.view.data_ptr()),
                                         ctypes.c_size_t(need), vp(bufs["prune"].view.data_ptr()), vp(bufs["rank"].view.data_ptr()),
                                         ctypes.byref(report), vp(torch.cuda.current_stream(enc.device).cuda_stream))
    _lib.check(enc.lib, enc._handle, code, "op_forward_masked")
    torch.cuda.synchronize()
    mem.assert_intact(f"fill {fill!r}: workspace")
    for name, buf in bufs.items():
        buf.assert_intact(f"fill {fill!r}: {name}")
    assert torch.equal(ids_d, ids_guard) and torch.equal(mask_d, mask_guard)
    return bufs["prune"].view.view(torch.float32).view(n_rows, width, 2).clone(), bufs["rank"].view.view(torch.float32).view(n_rows, nl).clone()


@pytest.mark.parametrize("case", [mm.SMALL[0], mm.SMALL[5]], ids=mm.case_id)
def test_outputs_do_not_depend_on_what_the_workspace_held(case):
    ids, mask, _ = mm.batch(200)
    enc = _encoder(case, kernel_set="fp32")
    try:
        want = _direct(enc, ids, mask, "zeros")
        again = enc.forward_masked(ids, mask)
        assert torch.equal(again[0], want[0]) and torch.equal(again[1], want[1])
        for fill in wu.POISONS:
            got = _direct(enc, ids, mask, fill)
            assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]), f"fill {fill!r} reaches an output"
    finally:
        enc.close()


@pytest.mark.parametrize("case", [mm.SMALL[3], mm.SMALL[4]], ids=mm.case_id)
def test_the_workspace_holds_on_a_handle_that_runs_another_set(case):
    """The call's main use: a handle whose own forward runs "bf16x3" (its rows are padded by another rule than the fp32 set's).
    Exactly op_masked_workspace_bytes between canaries, zeros and both poisons: the same bits, nothing written outside."""

    ids, mask, _ = mm.batch(200)
    enc = _encoder(case, kernel_set="bf16x3")
    f32 = _encoder(case, kernel_set="fp32")
    try:
        want = _direct(enc, ids, mask, "zeros", layout_enc=f32)
        again = enc.forward_masked(ids, mask)
        assert torch.equal(again[0], want[0]) and torch.equal(again[1], want[1])
        for fill in wu.POISONS:
            got = _direct(enc, ids, mask, fill, layout_enc=f32)
            assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]), f"fill {fill!r} reaches an output"
    finally:
        enc.close()
        f32.close()


# -- forward() ------------------------------------------------------------------------------------------------------------------------
def _model(attention_masks=None, cls=None, pooling=None):
    from open_provence_amd.config import OpenProvenceConfig
    from open_provence_amd.modeling import OpenProvenceModel
    from open_provence_amd.synthetic import named_dims, refinit_state_dict

    dims = named_dims("xsmall", vocab_size=2048, num_layers=3)
    cfg = OpenProvenceConfig(base_model_config=dims.to_base_model_config(), tokenizer_name_or_path="char-tokenizer",
                             pruning_config={"hidden_size": dims.hidden_size}, max_length=512, num_labels=1,
                             pruning_hidden_state="post_final_norm")
    kw = {} if attention_masks is None else {"attention_masks": attention_masks}
    model = (cls or OpenProvenceModel)(cfg, device="cuda:0", tokenizer=CharTokenizer(), state_dict=refinit_state_dict(dims, seed=5),
                                       calibrate=False, **kw)
    return model, dims, refinit_state_dict(dims, seed=5)


def _inputs(dims, rows=12, width=96, seed=3):
    from open_provence_amd.synthetic import pad_rows, synth_pair_batch

    rng = np.random.default_rng(seed)
    lengths = rng.integers(28, width + 1, size=rows).tolist()
    lengths[0], lengths[1] = width, 28
    ids, mask = pad_rows(synth_pair_batch(dims, rows, lengths, seed=seed))
    return ids, mask


@pytest.fixture(scope="module")
def models():
    made = {"any": _model("any"), "prefix": _model()}
    yield made
    for model, _, _ in made.values():
        model.encoder.close()


def test_a_default_model_still_raises(models):
    model, dims, _ = models["prefix"]
    assert model.encoder.attention_masks == "prefix"
    ids, mask = _inputs(dims)
    left = torch.flip(mask, [1])
    for to in (lambda t: t, lambda t: t.cuda()):
        with pytest.raises(NotImplementedError, match="right-padded"):
            model(input_ids=to(ids), attention_mask=to(left))
    with pytest.raises(ValueError, match="attention_masks"):
        model.encoder.forward_masked(ids, left)
    out = model(input_ids=ids, attention_mask=mask)  # the model is usable afterwards
    assert bool(torch.isfinite(out.ranking_logits).all())


def test_forward_takes_a_left_padded_batch_within_the_bound_of_the_oracle(models):
    model, dims, state = models["any"]
    ids, mask = _inputs(dims)
    left = torch.flip(mask, [1])
    ref = mm.Reference(state, dims, ids, left, False)
    out = model(input_ids=ids, attention_mask=left)
    _check("forward(), left-padded, CPU inputs", out.pruning_logits, out.ranking_logits, left, ref)
    # CPU inputs and device-resident inputs: the same bits
    dev = model(input_ids=ids.cuda(), attention_mask=left.cuda())
    assert torch.equal(dev.pruning_logits, out.pruning_logits) and torch.equal(dev.ranking_logits, out.ranking_logits)
    rank, prune = model(input_ids=ids, attention_mask=left, return_dict=False)
    assert torch.equal(rank, out.ranking_logits) and torch.equal(prune, out.pruning_logits)
    # the ranking loss reads the logits: the reference's BCE on them
    labels = torch.arange(ids.shape[0]) % 2
    with_loss = model(input_ids=ids, attention_mask=left, labels=labels)
    assert torch.equal(with_loss.ranking_logits, out.ranking_logits)
    want = torch.nn.BCEWithLogitsLoss()(out.ranking_logits.double().cpu().view(-1), labels.double())
    assert abs(float(with_loss.loss) - float(want)) <= 2e-6 * max(1.0, abs(float(want)))


def test_a_prefix_mask_on_an_any_model_takes_todays_path(models):
    (any_model, dims, _), (prefix_model, _, _) = models["any"], models["prefix"]
    ids, mask = _inputs(dims)
    for to in (lambda t: t, lambda t: t.cuda()):
        a = any_model(input_ids=to(ids), attention_mask=to(mask), output_hidden_states=True)
        b = prefix_model(input_ids=to(ids), attention_mask=to(mask), output_hidden_states=True)
        assert torch.equal(a.pruning_logits, b.pruning_logits) and torch.equal(a.ranking_logits, b.ranking_logits)
        assert all(torch.equal(x, y) for x, y in zip(a.hidden_states, b.hidden_states))
    assert any_model.encoder.effective_policy()["kernel_set"] == prefix_model.encoder.effective_policy()["kernel_set"]


def test_requests_that_are_later_work_raise_by_name_and_leave_the_model_usable(models):
    from open_provence_amd.modeling import OpenProvenceForTokenClassification

    model, dims, _ = models["any"]
    ids, mask = _inputs(dims)
    left = torch.flip(mask, [1])
    want = model(input_ids=ids, attention_mask=left)
    for kwargs, name in ((dict(output_hidden_states=True), "output_hidden_states"), (dict(output_attentions=True), "output_attentions"),
                         (dict(attention_rows="first"), "attention_rows"), (dict(pooled_hidden_states="mean"), "pooled_hidden_states")):
        for to in (lambda t: t, lambda t: t.cuda()):
            with pytest.raises(NotImplementedError, match=name):
                model(input_ids=to(ids), attention_mask=to(left), **kwargs)
        again = model(input_ids=ids, attention_mask=left)
        assert torch.equal(again.pruning_logits, want.pruning_logits) and torch.equal(again.ranking_logits, want.ranking_logits)
    tok, _, _ = _model("any", cls=OpenProvenceForTokenClassification)
    try:
        with pytest.raises(NotImplementedError, match="token-classification loss"):
            tok(input_ids=ids, attention_mask=left, labels=torch.zeros_like(ids))
        out = tok(input_ids=ids, attention_mask=left)  # without labels it runs
        assert torch.equal(out.logits, want.pruning_logits)
    finally:
        tok.encoder.close()


def test_an_id_outside_the_table_raises_wherever_it_sits(models):
    model, dims, _ = models["any"]
    ids, mask = _inputs(dims)
    left = torch.flip(mask, [1])
    want = model(input_ids=ids, attention_mask=left)
    row = 1
    col = int(torch.nonzero(left[row] == 0)[0])  # under a zero of the mask
    for value in (dims.vocab_size, -1):
        bad = ids.clone()
        bad[row, col] = value
        for to in (lambda t: t, lambda t: t.cuda()):
            with pytest.raises(IndexError, match=f"row {row}, column {col}") as info:
                model(input_ids=to(bad), attention_mask=to(left))
            assert str(value) in str(info.value)
        again = model(input_ids=ids, attention_mask=left)  # the handle is usable after the refusal
        assert torch.equal(again.pruning_logits, want.pruning_logits) and torch.equal(again.ranking_logits, want.ranking_logits)
    # the right-padded path keeps accepting garbage under padding
    bad = ids.clone()
    bad[1, -1] = dims.vocab_size + 5
    assert int(mask[1, -1]) == 0
    ok = model(input_ids=bad, attention_mask=mask)
    assert torch.equal(ok.ranking_logits, model(input_ids=ids, attention_mask=mask).ranking_logits)


def test_refusals_that_need_a_handle(models):
    from open_provence_amd import _lib

    model, dims, _ = models["prefix"]
    enc = model.encoder
    assert not enc.attention_outputs  # no fp32 packs on a default model
    report = _lib.OpMaskedReport()
    report.struct_bytes = ctypes.sizeof(_lib.OpMaskedReport)
    vp = ctypes.c_void_p
    buf = torch.zeros(4096, dtype=torch.uint8, device="cuda:0")
    args = lambda h, width=8, ws_bytes=1024: (h, vp(buf.data_ptr()), vp(buf.data_ptr()), 2, width, vp(buf.data_ptr()), ctypes.c_size_t(ws_bytes),  # noqa: E731
                                              vp(buf.data_ptr()), vp(buf.data_ptr()), ctypes.byref(report), None)
    assert enc.lib.op_forward_masked(*args(enc._handle)) == _lib.OP_ERR_UNSUPPORTED
    assert "OP_FLAG_F32_PACKS" in _lib.last_error(enc.lib, enc._handle)
    any_enc = models["any"][0].encoder
    assert any_enc.lib.op_forward_masked(*args(any_enc._handle, width=dims.max_position_embeddings + 1)) == _lib.OP_ERR_INVALID
    assert "max_position_embeddings" in _lib.last_error(any_enc.lib, any_enc._handle)
    assert any_enc.lib.op_forward_masked(*args(any_enc._handle)) == _lib.OP_ERR_WORKSPACE  # 1024 bytes: too small
    misaligned = (any_enc._handle, vp(buf.data_ptr()), vp(buf.data_ptr()), 2, 8, vp(buf.data_ptr() + 4), ctypes.c_size_t(1 << 30),
                  vp(buf.data_ptr()), vp(buf.data_ptr()), ctypes.byref(report), None)
    assert any_enc.lib.op_forward_masked(*misaligned) == _lib.OP_ERR_WORKSPACE
    # an empty batch: OP_OK, nothing written
    before = buf.clone()
    empty = (any_enc._handle, None, None, 0, 8, None, ctypes.c_size_t(0), None, None, ctypes.byref(report), None)
    assert any_enc.lib.op_forward_masked(*empty) == _lib.OP_OK
    empty = (any_enc._handle, None, None, 3, 0, None, ctypes.c_size_t(0), None, None, ctypes.byref(report), None)
    assert any_enc.lib.op_forward_masked(*empty) == _lib.OP_OK
    torch.cuda.synchronize()
    assert torch.equal(buf, before)
    prune, rank = any_enc.forward_masked(torch.zeros((3, 0), dtype=torch.int64), torch.zeros((3, 0), dtype=torch.int64))
    assert prune.shape == (3, 0, 2) and rank.shape == (3, 1)
