"""Attention probabilities (op_attention_probs / HipEncoder.attention_probs / forward_packed(attentions=...) /
forward(output_attentions=True)) against the reference's eager attentions (fixtures g13 / g14), with the logits and hidden
states of a forward bit-identical to those of the same forward without the request.

Measured in this file's first GPU run (tests/golden/attention_bounds.json holds the per-layer figures; the bound is 1.5 x each;
profiles/attention_probs.txt is the readable record)."""

from __future__ import annotations

import json

import numpy as np
import pytest
import torch

from attention_utils import c_attention_probs as _c_attention_probs, fixture_encoder, fixture_errors, packed_batch, selectable_sets, visible_mask
from helpers import GOLDEN_DIR, CharTokenizer, dims_from_meta, load_golden, state_from_fixture

pytestmark = pytest.mark.gpu

FIXTURES = ["g13_attn_hd64", "g14_attn_h256"]
PARITY_BAR = 1e-3  # the project's bar; a probability is at most 1


def _model(name, cls=None, **kw):
    from open_provence_amd.config import OpenProvenceConfig
    from open_provence_amd.modeling import OpenProvenceModel

    arrays, meta = load_golden(name)
    cfg = OpenProvenceConfig(
        base_model_config=meta["base_model_config"], tokenizer_name_or_path="char-tokenizer",
        pruning_config={"hidden_size": meta["base_model_config"]["hidden_size"]}, max_length=8192, num_labels=1,
        pruning_hidden_state="post_final_norm",
    )
    kw.setdefault("calibrate", False)
    model = (cls or OpenProvenceModel)(cfg, device="cuda:0", tokenizer=CharTokenizer(), state_dict=state_from_fixture(arrays, meta), **kw)
    return model, arrays, meta


def _assert_zero_pattern(attentions, dims, mask):
    """Exact zeros at padded rows and columns and outside the window; a real row sums to 1."""

    for i, a in enumerate(attentions):
        a = a.cpu()
        vis = visible_mask(dims, mask, i)[:, None].expand_as(a)
        assert bool((a[~vis] == 0).all()), f"layer {i}: a non-zero where the mask hides the key"
        assert not bool(torch.signbit(a).any()), f"layer {i}: a negative zero"
        sums = a.double().sum(-1)
        real = mask.bool()[:, None, :].expand_as(sums)
        assert float((sums[real] - 1.0).abs().max()) < 1e-5 and bool((sums[~real] == 0).all())


# 1. the model's forward ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", FIXTURES)
def test_model_forward_returns_the_attentions(name):
    model, arrays, meta = _model(name, attention_outputs=True)
    dims = dims_from_meta(meta)
    ids = torch.from_numpy(arrays["input_ids"])
    mask = torch.from_numpy(arrays["attention_mask"])
    B, L = ids.shape
    plain = model(input_ids=ids, attention_mask=mask)
    assert plain.attentions is None
    out = model(input_ids=ids, attention_mask=mask, output_attentions=True)
    assert out.hidden_states is None
    assert isinstance(out.attentions, tuple) and len(out.attentions) == dims.num_layers == meta["n_attentions"]
    for a in out.attentions:
        assert a.shape == (B, dims.num_heads, L, L) and a.dtype == torch.float32 and a.device.type == "cuda"
    _assert_zero_pattern(out.attentions, dims, mask)
    assert torch.equal(out.pruning_logits, plain.pruning_logits) and torch.equal(out.ranking_logits, plain.ranking_logits)
    # together with the hidden states: neither changes the other
    hs = model(input_ids=ids, attention_mask=mask, output_hidden_states=True)
    both = model(input_ids=ids, attention_mask=mask, output_hidden_states=True, output_attentions=True)
    assert torch.equal(both.pruning_logits, plain.pruning_logits) and torch.equal(both.ranking_logits, plain.ranking_logits)
    assert len(both.hidden_states) == len(hs.hidden_states) == dims.num_layers + 1
    assert all(torch.equal(x, y) for x, y in zip(both.hidden_states, hs.hidden_states))
    assert all(torch.equal(x, y) for x, y in zip(both.attentions, out.attentions))
    # the device-resident route
    dev = model(input_ids=ids.cuda(), attention_mask=mask.cuda(), output_attentions=True)
    assert torch.equal(dev.ranking_logits, plain.ranking_logits)
    assert all(torch.equal(x, y) for x, y in zip(dev.attentions, out.attentions))
    rank_t, prune_t = model(input_ids=ids, attention_mask=mask, return_dict=False, output_attentions=True)
    assert torch.equal(rank_t, plain.ranking_logits) and torch.equal(prune_t, plain.pruning_logits)
    # against the reference, on whatever set the model runs
    stride = meta["query_stride"]
    errs = [float((a[:, :, ::stride].cpu() - torch.from_numpy(arrays[f"attn_{i}"])).abs().max()) for i, a in enumerate(out.attentions)]
    kernel_set = model.encoder.effective_policy()["kernel_set"]
    print(f"[attn] {name} model forward on {kernel_set}: per-layer max|err| {['%.2e' % e for e in errs]}")
    bounds = json.loads((GOLDEN_DIR / "attention_bounds.json").read_text())[name][kernel_set]
    assert all(e <= 1.5 * b for e, b in zip(errs, bounds)), (errs, bounds)


def test_wrappers_pass_the_flag_through():
    from open_provence_amd.modeling import OpenProvenceForSequenceClassification, OpenProvenceForTokenClassification

    model, arrays, meta = _model("g13_attn_hd64", attention_outputs=True)
    ids = torch.from_numpy(arrays["input_ids"])
    mask = torch.from_numpy(arrays["attention_mask"])
    base = model(input_ids=ids, attention_mask=mask, output_attentions=True)
    for cls in (OpenProvenceForSequenceClassification, OpenProvenceForTokenClassification):
        other, _, _ = _model("g13_attn_hd64", cls=cls, attention_outputs=True)
        assert other(input_ids=ids, attention_mask=mask).attentions is None
        out = other(input_ids=ids, attention_mask=mask, output_attentions=True)
        assert len(out.attentions) == len(base.attentions) and all(torch.equal(x, y) for x, y in zip(out.attentions, base.attentions))
        assert torch.equal(out.ranking_logits, base.ranking_logits)


# 2. every kernel set the handle can select, against the fixture --------------------------------------------------------------
@pytest.mark.parametrize("name", FIXTURES)
def test_every_selectable_kernel_set_against_the_fixture(name):
    enc, arrays, meta, rows = fixture_encoder(name)
    bounds = json.loads((GOLDEN_DIR / "attention_bounds.json").read_text())[name]
    sets = selectable_sets(enc)
    assert "fp32" in sets and "bf16x3" in sets
    failures = []
    for kernel_set in sets:
        enc.select_kernel_set(kernel_set)
        assert enc.effective_policy()["kernel_set"] == kernel_set
        errs = fixture_errors(enc, arrays, meta, rows)
        print(f"[attn] {name} {kernel_set} per-layer max|err| {['%.2e' % e for e in errs]}")
        if kernel_set == "fp32":
            ratios = [e / r for e, r in zip(errs, meta["ref_to_fp64"])]
            print(f"[attn] {name} fp32: ratio to the reference's own distance to fp64 {['%.2f' % r for r in ratios]}")
        measured = bounds.get(kernel_set)
        if measured is None:
            failures.append(f"{kernel_set}: no measured bound in attention_bounds.json")
        elif not all(e <= 1.5 * b for e, b in zip(errs, measured)):
            failures.append(f"{kernel_set}: {errs} beyond 1.5 x {measured}")
        if kernel_set in ("fp32", "bf16x3") and not max(errs) < PARITY_BAR:
            failures.append(f"{kernel_set}: {max(errs):.3e} is not below the parity bar {PARITY_BAR:g}")
    enc.close()
    assert sorted(bounds) == sorted(sets), "attention_bounds.json lists other sets than the handle can select"
    assert not failures, failures


# 3. the C call itself ---------------------------------------------------------------------------------------------------------
def _hidden_states(enc, rows):
    """-> (packed fp32 hidden states [N + 1, T, H] of one forward, cu on the device, cu on the host, max_seqlen)"""

    from open_provence_amd.engine import HiddenRequest

    ids, cu, cu_np, max_len = packed_batch(enc, rows)
    _, _, states = enc.forward_packed(ids, cu, cu_np, max_len, hidden=HiddenRequest())
    return states, cu, cu_np, max_len


def test_every_element_is_written():
    """out_dev full of NaN, a poisoned workspace, pad_width 131 (beyond max_seqlen, no multiple of 4: the dword store path):
    the result is finite, zeros are in place, and its [128, 128] corner is the result of the 16-byte store path at width 128."""

    from open_provence_amd import _lib

    enc, arrays, meta, rows = fixture_encoder("g13_attn_hd64")
    dims = enc.dims
    states, cu, cu_np, max_len = _hidden_states(enc, rows)
    B, W = len(rows), 131
    need = int(enc.lib.op_attention_workspace_bytes(enc._handle, B, int(states.shape[1]), max_len))
    assert need > 0
    mask = torch.zeros((B, W), dtype=torch.int64)
    for b, row in enumerate(rows):
        mask[b, : len(row)] = 1
    for layer in range(dims.num_layers):
        out = torch.full((B, dims.num_heads, W, W), float("nan"), dtype=torch.float32, device=enc.device)
        ws = torch.full((need + 256,), 0xFF, dtype=torch.uint8, device=enc.device)  # fp32 NaN everywhere, -1 in every index
        assert _c_attention_probs(enc, states[layer], layer, cu, cu_np, max_len, out, ws) == _lib.OP_OK, _lib.last_error(enc.lib, enc._handle)
        torch.cuda.synchronize()
        assert bool(torch.isfinite(out).all())
        vis = visible_mask(dims, mask, layer)[:, None].expand(B, dims.num_heads, W, W)
        assert bool((out.cpu()[~vis] == 0).all()) and not bool(torch.signbit(out).any())
        narrow = enc.attention_probs(states[layer], layer, cu, cu_np, max_len, 128)
        assert torch.equal(out[:, :, :128, :128], narrow)
    enc.close()


@pytest.mark.parametrize("name", FIXTURES)
def test_layer_subsets_equal_the_all_layers_call(name):
    from open_provence_amd.engine import AttentionRequest, HiddenRequest

    enc, arrays, meta, rows = fixture_encoder(name)
    ids, cu, cu_np, max_len = packed_batch(enc, rows)
    prune, rank = enc.forward_packed(ids, cu, cu_np, max_len)
    p_all, r_all, every = enc.forward_packed(ids, cu, cu_np, max_len, attentions=AttentionRequest())
    assert torch.equal(p_all, prune) and torch.equal(r_all, rank) and len(every) == enc.dims.num_layers
    *_, one = enc.forward_packed(ids, cu, cu_np, max_len, attentions=AttentionRequest(layers=[1]))
    *_, two = enc.forward_packed(ids, cu, cu_np, max_len, attentions=AttentionRequest(layers=[0, 3]))
    assert len(one) == 1 and torch.equal(one[0], every[1])
    assert len(two) == 2 and torch.equal(two[0], every[0]) and torch.equal(two[1], every[3])
    # merged with the caller's own hidden request, in every form it takes
    _, _, own = enc.forward_packed(ids, cu, cu_np, max_len, hidden=HiddenRequest(layers=[0, 2, 4], dtype=torch.bfloat16, pad_width=max_len + 3))
    _, _, merged, probs = enc.forward_packed(ids, cu, cu_np, max_len, hidden=HiddenRequest(layers=[0, 2, 4], dtype=torch.bfloat16, pad_width=max_len + 3),
                                            attentions=AttentionRequest(layers=[3]))
    assert merged.shape == own.shape and torch.equal(merged.view(torch.int16), own.view(torch.int16)) and torch.equal(probs[0], every[3])
    with pytest.raises(ValueError):
        enc.forward_packed(ids, cu, cu_np, max_len, attentions=AttentionRequest(layers=[4]))
    with pytest.raises(ValueError):
        enc.forward_packed(ids, cu, cu_np, max_len, attentions=AttentionRequest(pad_width=max_len - 1))
    with pytest.raises(NotImplementedError):
        enc.forward_packed_on(0, ids, cu, cu_np, max_len, attentions=AttentionRequest())
    enc.close()


@pytest.mark.parametrize("name", FIXTURES)
def test_chunked_pass_equals_the_whole_pass(name):
    """Composition invariance: the same states through a handle that takes the batch whole and one that takes it in chunks."""

    whole, arrays, meta, rows = fixture_encoder(name)
    chunked, *_ = fixture_encoder(name, chunk_rows=128)
    states, cu, cu_np, max_len = _hidden_states(whole, rows)
    assert int(np.sum((np.diff(cu_np) + 31) // 32 * 32)) > 2 * 128  # more than two chunks
    for layer in range(whole.dims.num_layers):
        a = whole.attention_probs(states[layer], layer, cu, cu_np, max_len, max_len)
        b = chunked.attention_probs(states[layer], layer, cu, cu_np, max_len, max_len)
        assert torch.equal(a, b)
    # no host copy of cu_seqlens: the call reads it back
    a = whole.attention_probs(states[0], 0, cu, cu_np, max_len)
    out = torch.empty_like(a)
    ws = torch.empty(int(whole.lib.op_attention_workspace_bytes(whole._handle, len(rows), int(states.shape[1]), max_len)) + 256,
                     dtype=torch.uint8, device=whole.device)

    assert _c_attention_probs(whole, states[0], 0, cu, cu_np, max_len, out, ws, host_cu=False) == 0
    torch.cuda.synchronize()
    assert torch.equal(out, a)
    whole.close()
    chunked.close()


# 4. without the packs ---------------------------------------------------------------------------------------------------------
def test_without_the_packs_the_call_is_refused():
    from open_provence_amd import _lib
    from open_provence_amd.engine import AttentionRequest

    enc, arrays, meta, rows = fixture_encoder("g13_attn_hd64", attention_outputs=False)
    assert not enc.attention_outputs
    states, cu, cu_np, max_len = _hidden_states(enc, rows)
    out = torch.zeros((len(rows), enc.dims.num_heads, max_len, max_len), dtype=torch.float32, device=enc.device)
    ws = torch.empty(1 << 20, dtype=torch.uint8, device=enc.device)
    assert _c_attention_probs(enc, states[0], 0, cu, cu_np, max_len, out, ws) == _lib.OP_ERR_UNSUPPORTED
    assert "OP_FLAG_F32_PACKS" in _lib.last_error(enc.lib, enc._handle)
    with pytest.raises(ValueError, match="attention_outputs=True"):
        enc.forward_packed(*packed_batch(enc, rows), attentions=AttentionRequest())
    # with the packs, a layer the model does not have is refused once the handle is known
    enc.close()
    enc, *_ = fixture_encoder("g13_attn_hd64")
    out4 = out.clone()
    for layer in (-1, enc.dims.num_layers):
        assert _c_attention_probs(enc, states[0], layer, cu, cu_np, max_len, out4, ws) == _lib.OP_ERR_INVALID
        assert "layer" in _lib.last_error(enc.lib, enc._handle)
    enc.close()
    model, arrays, meta = _model("g13_attn_hd64")
    ids = torch.from_numpy(arrays["input_ids"])
    with pytest.raises(ValueError, match="attention_outputs=True"):
        model(input_ids=ids, attention_mask=torch.from_numpy(arrays["attention_mask"]), output_attentions=True)
    assert model(input_ids=ids, attention_mask=torch.from_numpy(arrays["attention_mask"])).attentions is None
