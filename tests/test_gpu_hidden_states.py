"""Per-call hidden states (op_forward_packed_hidden / HipEncoder.forward_packed(hidden=...) / forward(output_hidden_states=True)):
the reference's hidden_states from the same kernels that produce the logits, against the stored reference states, and the
logits of a forward with the request bit-identical to those of the same forward without it."""

from __future__ import annotations

import numpy as np
import pytest
import torch

from helpers import dims_from_meta, load_golden, rows_from_fixture, state_from_fixture

pytestmark = pytest.mark.gpu

ROW_SETS = ["bf16x3", "bf16-weights", "bf16", "f16-f8", "f16-f8-w", "f16"]


def _encoder(dims, state, *, kernel_set=None, calibrate=False, flags=None, chunk_rows=None, pre_norm=False):
    from open_provence_amd.engine import HipEncoder

    enc = HipEncoder(dims, device="cuda:0", chunk_rows=chunk_rows, flags=flags, prune_pre_final_norm=pre_norm)
    enc.load_state_dict(state, calibrate=calibrate, kernel_set=kernel_set)
    return enc


def _fixture_encoder(name, **kw):
    arrays, meta = load_golden(name)
    dims = dims_from_meta(meta)
    state = state_from_fixture(arrays, meta)
    enc = _encoder(dims, state, pre_norm=bool(meta.get("prune_pre_final_norm", False)), **kw)
    return enc, arrays, meta, state, rows_from_fixture(arrays)


def _forward(enc, rows, hidden=None):
    from open_provence_amd.packing import pack_rows

    ids_np, cu_np, max_len = pack_rows(rows)
    ids = torch.from_numpy(ids_np).to(enc.device)
    cu = torch.from_numpy(cu_np).to(enc.device)
    out = enc.forward_packed(ids, cu, cu_np, max_len, hidden=hidden)
    torch.cuda.synchronize()
    return tuple(t.cpu() for t in out), cu_np


def _strided_error(hidden_padded, arrays, meta, entries):
    """max |hidden - reference| per entry at the fixture's strided positions; hidden_padded [N+1, B, L, H] (numpy)."""

    stride = meta["hidden_stride"]
    lengths = arrays["attention_mask"].astype(bool).sum(axis=1)
    errs = []
    for i in entries:
        ref_h = arrays[f"hidden_{i}"]
        worst = 0.0
        for b, length in enumerate(lengths):
            pos = np.arange(0, int(length), stride)
            worst = max(worst, float(np.abs(hidden_padded[i, b, pos] - ref_h[b, : len(pos)]).max()))
        errs.append(worst)
    return errs


def _model(name, **kw):
    from open_provence_amd.config import OpenProvenceConfig
    from open_provence_amd.modeling import OpenProvenceModel
    from helpers import CharTokenizer

    arrays, meta = load_golden(name)
    cfg = OpenProvenceConfig(
        base_model_config=meta["base_model_config"], tokenizer_name_or_path="char-tokenizer",
        pruning_config={"hidden_size": meta["base_model_config"]["hidden_size"]}, max_length=8192, num_labels=1,
        pruning_hidden_state="post_final_norm",
    )
    state = state_from_fixture(arrays, meta)
    return OpenProvenceModel(cfg, device="cuda:0", tokenizer=CharTokenizer(), state_dict=state, **kw), arrays, meta


# 1. reference parity through the model's forward --------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["g1_xsmall", "g7_xsmall_refinit"])
def test_model_forward_returns_the_reference_hidden_states(name):
    model, arrays, meta = _model(name)
    ids = torch.from_numpy(arrays["input_ids"])
    mask = torch.from_numpy(arrays["attention_mask"])
    plain = model(input_ids=ids, attention_mask=mask)
    assert plain.hidden_states is None
    out = model(input_ids=ids, attention_mask=mask, output_hidden_states=True)
    n = meta["n_hidden_states"]
    B, L = ids.shape
    assert isinstance(out.hidden_states, tuple) and len(out.hidden_states) == n == 11
    for h in out.hidden_states:
        assert h.shape == (B, L, 256) and h.dtype == torch.float32 and h.device.type == "cuda"
    hidden = torch.stack(out.hidden_states).cpu().numpy()
    m = mask.bool().numpy()
    assert np.all(hidden[:, ~m] == 0.0)  # zero at padding
    assert torch.equal(out.pruning_logits, plain.pruning_logits) and torch.equal(out.ranking_logits, plain.ranking_logits)
    errs = _strided_error(hidden, arrays, meta, range(n))
    kernel_set = model.encoder.effective_policy()["kernel_set"]
    print(f"[hidden] {name} on {kernel_set}: per-entry max|err| {['%.2e' % e for e in errs]}")
    # "f16" (G7 calibrates to it): measured 3.6e-5 at the deepest entry; the bound is 1.5 x that
    assert max(errs) < (5.5e-5 if kernel_set == "f16" else 2e-3), (kernel_set, errs)
    rank_t, prune_t = model(input_ids=ids, attention_mask=mask, return_dict=False, output_hidden_states=True)
    assert torch.equal(rank_t, plain.ranking_logits) and torch.equal(prune_t, plain.pruning_logits)


@pytest.mark.parametrize("name,kernel_set,bound", [("g1_xsmall", "bf16x3", 2e-3), ("g1_xsmall", "f16-f8-w", 2e-3),
                                                   ("g7_xsmall_refinit", "bf16x3", 2e-3), ("g7_xsmall_refinit", "f16-f8-w", 2e-3),
                                                   ("g7_xsmall_refinit", "f16", 5.5e-5)])  # (f16 measured: 3.6e-5)
def test_hidden_states_match_the_reference_per_kernel_set(name, kernel_set, bound):
    from open_provence_amd.engine import HiddenRequest

    enc, arrays, meta, _, rows = _fixture_encoder(name, kernel_set=kernel_set)
    assert enc.effective_policy()["kernel_set"] == kernel_set
    L = arrays["input_ids"].shape[1]
    (_, _, hidden), _ = _forward(enc, rows, HiddenRequest(pad_width=L))
    errs = _strided_error(hidden.numpy(), arrays, meta, range(meta["n_hidden_states"]))
    print(f"[hidden] {name} on {kernel_set}: max|err| {max(errs):.3e} (per entry {['%.2e' % e for e in errs]})")
    enc.close()
    assert max(errs) < bound, errs


# 2. same kernels, same logits -------------------------------------------------------------------------------------------
def _timed_batch(dims, n=256, length=512):
    from open_provence_amd.synthetic import synth_pair_batch

    return synth_pair_batch(dims, n, [length] * n, seed=3)


@pytest.mark.parametrize("kernel_set", ROW_SETS)
def test_logits_with_every_entry_requested_are_bit_identical(kernel_set):
    from open_provence_amd.engine import HiddenRequest
    from open_provence_amd.synthetic import named_dims, refinit_state_dict

    dims = named_dims("xsmall", vocab_size=4096)
    state = refinit_state_dict(dims, seed=11)
    enc = _encoder(dims, state, kernel_set=kernel_set)
    assert enc.effective_policy()["kernel_set"] == kernel_set
    rows = _timed_batch(dims)
    (p0, r0), _ = _forward(enc, rows)
    (p1, r1, h1), _ = _forward(enc, rows, HiddenRequest())
    enc.close()
    assert np.array_equal(p0.numpy(), p1.numpy()) and np.array_equal(r0.numpy(), r1.numpy())
    assert h1.shape == (dims.num_layers + 1, len(rows) * 512, dims.hidden_size) and bool(torch.isfinite(h1).all())
    if kernel_set == "f16":
        # the wave-pair kernel (256 x 512 on "f16") against the 8 x 16 kernel: the request changes neither
        from open_provence_amd import _lib

        enc8 = _encoder(dims, state, kernel_set=kernel_set, flags=_lib.OP_FLAG_NO_LAYER_PAIRS)
        (p8, r8), _ = _forward(enc8, rows)
        (p8h, r8h, h8), _ = _forward(enc8, rows, HiddenRequest())
        enc8.close()
        assert np.array_equal(p8.numpy(), p8h.numpy()) and np.array_equal(r8.numpy(), r8h.numpy())
        same = np.array_equal(p8.numpy(), p0.numpy())
        # The two kernels differ here (they sum in different orders; measured: 1.8e-5 in the pruning logits), so the bit-identity
        # above was taken on the wave-pair kernel, with the request's copies of its tiled residual stream
        assert not same
        print(f"[hidden] f16 wave-pair vs 8 x 16 kernel: logits bit-identical={same}, "
              f"max|prune diff|={float((p8 - p0).abs().max()):.2e}, max|hidden diff|={float((h8 - h1).abs().max()):.2e}")
        assert float((h8 - h1).abs().max()) < 5e-2


def test_logits_bit_identical_on_the_panel_path():
    from open_provence_amd.engine import HiddenRequest

    enc, arrays, meta, _, rows = _fixture_encoder("g8_base_refinit")
    (p0, r0), _ = _forward(enc, rows)
    (p1, r1, h1), _ = _forward(enc, rows, HiddenRequest(pad_width=arrays["input_ids"].shape[1]))
    enc.close()
    assert np.array_equal(p0.numpy(), p1.numpy()) and np.array_equal(r0.numpy(), r1.numpy())


# 3. head identity ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,kernel_set", [("g12_prenorm_tf4", "bf16x3"), ("g12_prenorm_tf4", "f16-f8-w"), ("g12_prenorm_tf4", "f16"),
                                             ("g1_xsmall", "bf16x3"), ("g1_xsmall", "f16-f8-w"), ("g7_xsmall_refinit", "f16")])
def test_last_entry_is_the_pruning_heads_input(name, kernel_set):
    from open_provence_amd.engine import HiddenRequest

    enc, arrays, meta, state, rows = _fixture_encoder(name, kernel_set=kernel_set)
    n = enc.dims.num_layers
    (prune, _, hidden), _ = _forward(enc, rows, HiddenRequest(layers=[n]))
    enc.close()
    w = state["pruning_head.classifier.weight"].double()
    b = state["pruning_head.classifier.bias"].double()
    logits = hidden[0].double() @ w.T + b
    scale = float(prune.abs().max())
    assert float((logits - prune.double()).abs().max()) <= 1e-5 * max(scale, 1.0)
    if meta.get("prune_pre_final_norm") and kernel_set != "f16":  # ("f16" on G12's O(1) weights is 1e-2 from the oracle by itself)
        # entry N is the raw last layer (transformers 4.x); final_norm of it is the oracle's post-norm last state
        from oracle.modernbert_oracle import oracle_forward
        from open_provence_amd.synthetic import pad_rows

        ids, mask = pad_rows(rows)
        with torch.no_grad():
            ref = oracle_forward(state, enc.dims, ids, mask, return_hidden=True)
        g = state["ranking_model.model.final_norm.weight"].float()
        normed = torch.nn.functional.layer_norm(hidden[0], (enc.dims.hidden_size,), eps=enc.dims.norm_eps) * g
        post = ref.hidden_states[-1][mask.bool()]
        assert float((normed - post).abs().max()) < 2e-3


# 4. selection, dtype, layout ----------------------------------------------------------------------------------------------
def test_selection_dtype_and_layout_agree_with_the_full_capture():
    from open_provence_amd.engine import HiddenRequest

    enc, arrays, meta, _, rows = _fixture_encoder("g1_xsmall", kernel_set="f16-f8-w")
    L = arrays["input_ids"].shape[1]
    (_, _, full), cu = _forward(enc, rows, HiddenRequest())
    (_, _, sub), _ = _forward(enc, rows, HiddenRequest(layers=[0, 3, 10]))
    (_, _, bf), _ = _forward(enc, rows, HiddenRequest(dtype=torch.bfloat16))
    (_, _, padded), _ = _forward(enc, rows, HiddenRequest(pad_width=L + 5))
    enc.close()
    assert torch.equal(sub, full[[0, 3, 10]])
    assert bf.dtype == torch.bfloat16 and torch.equal(bf.view(torch.int16), full.to(torch.bfloat16).view(torch.int16))
    assert padded.shape == (11, len(rows), L + 5, 256)
    for s in range(len(rows)):
        assert torch.equal(padded[:, s, : cu[s + 1] - cu[s]], full[:, cu[s] : cu[s + 1]])
        assert bool((padded[:, s, cu[s + 1] - cu[s]:] == 0).all())


def test_invalid_requests_are_refused():
    from open_provence_amd.engine import HiddenRequest

    enc, arrays, meta, _, rows = _fixture_encoder("g12_prenorm_tf4")
    with pytest.raises(ValueError):
        _forward(enc, rows, HiddenRequest(pad_width=10))
    with pytest.raises(ValueError):
        _forward(enc, rows, HiddenRequest(layers=[5]))
    with pytest.raises(ValueError):
        _forward(enc, rows, HiddenRequest(dtype=torch.float16))
    with pytest.raises(NotImplementedError):
        ids = torch.zeros(4, dtype=torch.int32, device=enc.device)
        cu = torch.tensor([0, 4], dtype=torch.int32, device=enc.device)
        enc.forward_packed_on(0, ids, cu, np.array([0, 4], dtype=np.int32), 4, hidden=HiddenRequest())
    enc.close()


# 5. chunked and ragged batches --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kernel_set", ["bf16x3", "f16-f8-w", "f16"])
def test_chunked_and_ragged_batches(kernel_set):
    from open_provence_amd.engine import HiddenRequest
    from open_provence_amd.synthetic import named_dims, refinit_state_dict

    dims = named_dims("xsmall", vocab_size=4096)
    state = refinit_state_dict(dims, seed=13)
    lengths = [1, 63, 64, 65, 511, 512, 300, 532]  # 2048 tokens
    rng = np.random.default_rng(5)
    rows = [[dims.cls_token_id] + rng.integers(4, dims.vocab_size, n - 1).tolist() for n in lengths]
    whole = _encoder(dims, state, kernel_set=kernel_set)
    chunked = _encoder(dims, state, kernel_set=kernel_set, chunk_rows=256)
    req = HiddenRequest(pad_width=600)
    (pa, ra, ha), cu = _forward(whole, rows, req)
    (pb, rb, hb), _ = _forward(chunked, rows, req)
    (pp, rp, hp), _ = _forward(whole, rows, HiddenRequest())
    whole.close()
    chunked.close()
    assert sum(lengths) == 2048
    # chunks change the launch shapes (small blocks, pair kernel), not one bit of a row's arithmetic: measured on these three sets
    # here and on the 2 600-row batch of tests/test_kernel_set_geometry.py, which also holds the rows to the model's bound
    assert torch.equal(ha, hb) and torch.equal(pa, pb) and torch.equal(ra, rb)
    for s in range(len(lengths)):
        assert torch.equal(ha[:, s, : lengths[s]], hp[:, cu[s] : cu[s + 1]])
        assert bool((ha[:, s, lengths[s]:] == 0).all()) and bool((hb[:, s, lengths[s]:] == 0).all())


# 6. panel path and gte varlen ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["g8_base_refinit", "g2_gte_varlen"])
def test_panel_and_varlen_fixtures_match_the_oracle(name):
    from open_provence_amd.engine import HiddenRequest
    from open_provence_amd.synthetic import pad_rows
    from oracle.modernbert_oracle import oracle_forward

    enc, arrays, meta, state, rows = _fixture_encoder(name)
    (_, _, hidden), cu = _forward(enc, rows, HiddenRequest())
    kernel_set = enc.effective_policy()["kernel_set"]
    n = enc.dims.num_layers
    enc.close()
    spot = sorted({0, len(rows) - 1})  # spot pairs: the oracle runs on the CPU
    ids, mask = pad_rows([rows[s] for s in spot])
    with torch.no_grad():
        ref = oracle_forward(state, enc.dims, ids, mask, return_hidden=True, attn="sdpa")
    errs = []
    for i in range(n):  # entries 0 .. N-1 (the oracle's entry N is post-norm, as under transformers 5)
        worst = 0.0
        for j, s in enumerate(spot):
            length = cu[s + 1] - cu[s]
            worst = max(worst, float((hidden[i, cu[s] : cu[s + 1]] - ref.hidden_states[i][j, :length]).abs().max()))
        errs.append(worst)
    print(f"[hidden] {name} on {kernel_set}: per-entry max|err| {['%.2e' % e for e in errs]}")
    assert max(errs) < 2e-3, errs


# 7. audit and wrappers ----------------------------------------------------------------------------------------------------
def test_audit_runs_on_a_first_batch_that_requests_hidden_states():
    from open_provence_amd.engine import HiddenRequest

    enc, arrays, meta, _, rows = _fixture_encoder("g7_xsmall_refinit", calibrate=True)
    cal = enc.calibration
    assert cal is not None and cal["chosen_set"] != cal["default_set"] and enc.audit_pending
    (prune, rank, hidden), _ = _forward(enc, rows, HiddenRequest())
    assert "audit" in enc.calibration and enc.calibration["audit"]["passed"]
    assert not enc.audit_pending
    (p2, r2, h2), _ = _forward(enc, rows, HiddenRequest())
    enc.close()
    assert torch.equal(prune, p2) and torch.equal(hidden, h2)


def test_failed_audit_recomputes_the_batch_with_its_hidden_states():
    from open_provence_amd.engine import HiddenRequest

    enc, arrays, meta, _, rows = _fixture_encoder("g7_xsmall_refinit", calibrate=True)
    cal = enc.calibration
    assert cal["chosen_set"] != cal["default_set"] and enc.audit_pending
    enc.audit_factor = 0.0  # no difference from the reference set passes: the audit fails and reverts
    with pytest.warns(RuntimeWarning, match="disagrees with the load-time calibration"):
        (prune, rank, hidden), _ = _forward(enc, rows, HiddenRequest(layers=[0, 5, 10], dtype=torch.bfloat16))
    assert not enc.calibration["audit"]["passed"]
    assert enc.effective_policy()["kernel_set"] == cal["default_set"]
    # what was returned is the batch recomputed on the default set, hidden states included
    (p2, r2, h2), _ = _forward(enc, rows, HiddenRequest(layers=[0, 5, 10], dtype=torch.bfloat16))
    enc.close()
    assert torch.equal(prune, p2) and torch.equal(rank, r2)
    assert torch.equal(hidden.view(torch.int16), h2.view(torch.int16))


def test_model_forward_with_empty_width_keeps_the_shape():
    model, arrays, meta = _model("g1_xsmall")
    ids = torch.zeros((3, 0), dtype=torch.int64)
    out = model(input_ids=ids, attention_mask=torch.zeros_like(ids), output_hidden_states=True)
    assert len(out.hidden_states) == 11 and all(h.shape == (3, 0, 256) for h in out.hidden_states)


def test_token_classification_wrapper_passes_the_flag_through():
    from open_provence_amd.config import OpenProvenceConfig
    from open_provence_amd.modeling import OpenProvenceForTokenClassification
    from helpers import CharTokenizer

    model, arrays, meta = _model("g1_xsmall")
    cfg = OpenProvenceConfig(
        base_model_config=meta["base_model_config"], tokenizer_name_or_path="char-tokenizer",
        pruning_config={"hidden_size": 256}, max_length=8192, num_labels=1, pruning_hidden_state="post_final_norm",
    )
    tok = OpenProvenceForTokenClassification(cfg, device="cuda:0", tokenizer=CharTokenizer(), state_dict=state_from_fixture(arrays, meta))
    ids = torch.from_numpy(arrays["input_ids"])
    mask = torch.from_numpy(arrays["attention_mask"])
    a = model(input_ids=ids, attention_mask=mask, output_hidden_states=True)
    b = tok(input_ids=ids, attention_mask=mask, output_hidden_states=True)
    assert tok(input_ids=ids, attention_mask=mask).hidden_states is None
    assert len(b.hidden_states) == 11 and torch.equal(b.logits, a.pruning_logits)
    for x, y in zip(a.hidden_states, b.hidden_states):
        assert torch.equal(x, y)
