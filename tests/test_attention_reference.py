"""The references of tests/test_gpu_attention_conformance.py, checked on the CPU: the closed form of a zero state, the plumbing of
the fp64 / fp32 restatement pair and of its bound, and the peaked construction."""

from __future__ import annotations

import numpy as np
import pytest
import torch

import attention_utils as au

UNIFORM_WINDOWS = [1, 2, 6, 16, 126, 128, 130, 1024]  # half-windows 0, 1, 3, 8, 63, 64, 65 and 512


def _edge_mask():
    mask = torch.zeros((len(au.EDGE), max(au.EDGE)), dtype=torch.int64)
    for b, n in enumerate(au.EDGE):
        mask[b, :n] = 1
    return mask


@pytest.mark.parametrize("window", UNIFORM_WINDOWS)
def test_uniform_probs_is_the_restatement_on_a_zero_state(window):
    from open_provence_amd.synthetic import synth_state_dict

    dims = au.small_dims(128, 2, "GL", window)
    state = synth_state_dict(dims, 5)
    mask = _edge_mask()
    zeros = torch.zeros((len(au.EDGE), max(au.EDGE), dims.hidden_size), dtype=torch.float32)
    for layer in range(dims.num_layers):
        want = au.uniform_probs(dims, mask, layer)
        got = au.attention_probs(state, dims, zeros, mask, layer, torch.float64)
        assert got.shape == (len(au.EDGE), dims.num_heads, max(au.EDGE), max(au.EDGE))
        assert float((got - want[:, None]).abs().max()) == 0.0
        # the counts themselves: a full row of a global layer, at most 2 w + 1 keys on a sliding one, the diagonal alone at w = 0
        count = au.visible_mask(dims, mask, layer).sum(-1)
        lengths = torch.tensor(au.EDGE)[:, None]
        if dims.layer_is_global[layer]:
            assert bool((count == lengths * mask).all())
        else:
            i = torch.arange(max(au.EDGE))[None, :]
            w = dims.half_window
            assert bool((count == ((torch.minimum(i + w, lengths - 1) - (i - w).clamp(min=0) + 1) * mask)).all())
            if w == 0:
                assert bool((want[mask.bool()].sum(-1) == 1).all()) and bool((torch.diagonal(want, dim1=1, dim2=2)[mask.bool()] == 1).all())


def test_fp32_restatement_is_inside_its_own_bound_on_model_a():
    """Trivially true (err = e_ref); it guards the plumbing of probs_reference, check_probs and the bound."""

    ref = au.probs_reference("A")
    assert ref.mask.shape == (len(au.EDGE), max(au.EDGE)) and [len(r) for r in ref.rows] == au.EDGE
    assert au.probs_bound(0.0) == 16 * float(np.spacing(np.float32(1.0))) and au.probs_bound(1e-5) == 4e-5
    for layer in range(ref.dims.num_layers):
        assert ref.inputs[layer].dtype == torch.float32 and ref.p64[layer].dtype == torch.float64
        assert ref.packed(layer).shape == (sum(au.EDGE), ref.dims.hidden_size)
        p32 = au.attention_probs(ref.state, ref.dims, ref.inputs[layer], ref.mask, layer, torch.float32)
        ratio = au.check_probs("fp32 restatement A", p32, ref, layer)
        assert 0.0 < ref.e_ref[layer] < 1e-5 and ratio == pytest.approx(1.0)
        # ... and the check does fail on what it is there to catch
        wrong = p32.clone()
        shift = 2 * au.probs_bound(ref.e_ref[layer])  # mass moved between two visible keys: the row still sums to 1
        assert float(wrong[0, 0, 5, 4]) > shift
        wrong[0, 0, 5, 3] += shift
        wrong[0, 0, 5, 4] -= shift
        with pytest.raises(AssertionError, match="from the fp64 restatement"):
            au.check_probs("perturbed", wrong, ref, layer)
        leaked = p32.clone()
        leaked[-1, 0, 0, 1] = 1e-30  # a key beyond the one-token row
        with pytest.raises(AssertionError):
            au.check_probs_pattern("leaked", leaked, ref.dims, ref.mask, layer)


@pytest.mark.parametrize("name", ["A", "B"])
def test_peaked_construction_is_peaked(name):
    ref = au.probs_reference(name, peaked=True)
    plain = au.probs_reference(name)
    assert torch.equal(ref.inputs[0], plain.inputs[0] * au.PEAK_GAIN)
    assert all(torch.equal(a, b) for a, b in zip(ref.inputs[1:], plain.inputs[1:]))
    for layer in range(ref.dims.num_layers):
        top = ref.median_row_max(layer)
        print(f"[attn-ref] peaked {name} layer {layer}: median row maximum {top:.4f}  e_ref {ref.e_ref[layer]:.3e}")
        assert top >= 0.9
        au.check_probs_pattern(f"peaked {name}", ref.p64[layer].float(), ref.dims, ref.mask, layer)
