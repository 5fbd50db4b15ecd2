"""The attention fixtures (tests/golden/make_golden_attentions.py: the reference under eager attention) against the fp64
restatement of tests/attention_utils.py.  This checks the YARDSTICK the GPU tests measure with, not the feature."""

from __future__ import annotations

import numpy as np
import pytest
import torch

from attention_utils import attention_probs, visible_mask
from helpers import dims_from_meta, load_golden, state_from_fixture
from oracle.modernbert_oracle import oracle_forward

FIXTURES = ["g13_attn_hd64", "g14_attn_h256"]


@pytest.fixture(scope="module", params=FIXTURES)
def fixture(request):
    arrays, meta = load_golden(request.param)
    dims = dims_from_meta(meta)
    state = state_from_fixture(arrays, meta)
    ids = torch.from_numpy(arrays["input_ids"])
    mask = torch.from_numpy(arrays["attention_mask"])
    with torch.no_grad():
        exact = oracle_forward(state, dims, ids, mask, dtype=torch.float64, return_hidden=True)
        restated = [attention_probs(state, dims, exact.hidden_states[i], mask, i).numpy() for i in range(dims.num_layers)]
    return arrays, meta, dims, mask, exact, restated


def test_fixture_shapes_and_model(fixture):
    arrays, meta, dims, mask, exact, _ = fixture
    B, L = arrays["input_ids"].shape
    stride = meta["query_stride"]
    assert meta["n_attentions"] == dims.num_layers and mask.sum(dim=1).tolist() == meta["lengths"]
    for i in range(dims.num_layers):
        a = arrays[f"attn_{i}"]
        assert a.shape == (B, dims.num_heads, len(range(0, L, stride)), L) and a.dtype == np.float32 and np.isfinite(a).all()
    # the model is the one the seed describes: its ranking logits are the oracle's
    assert float(np.abs(arrays["ranking_logits"] - exact.ranking_logits.numpy()).max()) < 1e-3


def test_fixture_is_within_twice_its_own_distance_to_fp64(fixture):
    arrays, meta, dims, _, _, restated = fixture
    stride = meta["query_stride"]
    for i in range(dims.num_layers):
        err = float(np.abs(arrays[f"attn_{i}"].astype(np.float64) - restated[i][:, :, ::stride]).max())
        print(f"[attn-fixture] {meta['name']} layer {i}: max|reference - fp64| {err:.2e} (recorded {meta['ref_to_fp64'][i]:.2e})")
        assert err <= 2.0 * meta["ref_to_fp64"][i]


def test_exact_zeros_where_the_mask_says_and_rows_sum_to_one(fixture):
    arrays, meta, dims, mask, _, _ = fixture
    stride = meta["query_stride"]
    lengths = meta["lengths"]
    for i in range(dims.num_layers):
        a = arrays[f"attn_{i}"]
        vis = visible_mask(dims, mask, i).numpy()[:, ::stride]  # [B, queries, L]
        hidden = np.broadcast_to(~vis[:, None], a.shape)
        assert np.all(a[hidden] == 0.0)
        sums = a.astype(np.float64).sum(axis=-1)  # [B, heads, queries]
        for b, n in enumerate(lengths):
            real = np.arange(0, a.shape[3], stride) < n
            assert float(np.abs(sums[b][:, real] - 1.0).max()) <= 1e-6
            assert np.all(sums[b][:, ~real] == 0.0)
    one = [b for b, n in enumerate(lengths) if n == 1]
    for b in one:  # a 1-token row holds exactly 1.0
        assert all(np.all(arrays[f"attn_{i}"][b, :, 0, 0] == 1.0) for i in range(dims.num_layers))
