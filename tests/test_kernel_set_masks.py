"""The per-layer mask of kernel sets 8 / 9 (op_select_mlp_correction_layers, op_calibration.mlp_layers): bit li keeps the
fp16 + e4m3 MLP in layer li, every other layer runs the "f16" set's MLP.  Two instruments, because the aggregate bound of
tests/test_kernel_set_conformance.py cannot localise a bit (an uncorrected layer carries the "f16" MLP's error, the bound is
twice that, and moving the uncorrected layer moves an error of the same size: tests/test_arith_model.py prints the figures):

* WHICH layer a bit means, with no tolerance: flipping bit li leaves the fp32 hidden entries 0 .. li bit-identical and
  changes entry li + 1 (entry N, the pruning and the ranking logits for the last layer).  With the two identities of
  test_gpu_calibration.py::test_mlp_correction_layer_mask_through_the_c_abi (mask 0 is the "f16" set, all ones the whole
  depth) this pins bit li to layer li.  A mask applied in reversed bit order, off by one, or indexed by anything but the
  layer fails it.
* WHAT a masked forward computes: prefix masks and mixed masks against the float64 model with that mask
  (arith_model.Arith.mlp_layers) on the MLP-isolating weights, under the conformance bound, and closer (RMS) to its own
  mask's model than to every neighbouring mask's at every entry behind the first layer where the two differ.  A layer
  without the correction that read the previous layer's stale e4m3 plane of LN(x) or h would be off by the size of the
  correction itself, far over the bound.

Out of scope: models deeper than 64 layers (the mask is a uint64; layers li >= 64 always keep the correction).
"""

from __future__ import annotations

import ctypes

import pytest
import torch

import arith_model as am
import test_kernel_set_conformance as conf

pytestmark = pytest.mark.gpu

MODEL = "panel512x4"
N_LAYERS = conf.SHAPES[MODEL][3]
MASKED_SETS = list(am.MASKED_SETS)
# the masks whose forward is held to its model: every proper prefix and two mixed ones on set 8, one mixed one on set 9
MODEL_MASKS = {"f16+mlp-f16-f8-w": [0b0001, 0b0011, 0b0111, 0b0101, 0b1010], "f16+mlp-f16-f8": [0b0110]}
# the masks every bit is flipped from
FLIP_FROM = [0b0000, 0b0101]

TABLE: list[str] = []


@pytest.fixture(scope="module", autouse=True)
def _print_table():
    yield
    for line in TABLE:
        print("[conformance]", line)


def layers_of(mask: int, n_layers: int = N_LAYERS) -> tuple:
    return tuple(li for li in range(n_layers) if (mask >> li) & 1)


def first_differing_layer(a: int, b: int) -> int:
    return ((a ^ b) & -(a ^ b)).bit_length() - 1


def neighbours(mask: int, n_layers: int = N_LAYERS) -> list[int]:
    """The masks a wrong implementation would run instead: one bit flipped (each layer), shifted by one layer either way,
    bit order reversed, all, none -- without `mask` itself and without repeats, in that order."""

    full = (1 << n_layers) - 1
    cand = [mask ^ (1 << li) for li in range(n_layers)]
    cand += [(mask << 1) & full, mask >> 1]
    cand += [sum(1 << (n_layers - 1 - li) for li in range(n_layers) if (mask >> li) & 1), full, 0]
    out = []
    for c in cand:
        if c != mask and c not in out:
            out.append(c)
    return out


def _select_layers(enc, mask: int) -> None:
    from open_provence_amd import _lib

    _lib.check(enc.lib, enc._handle, enc.lib.op_select_mlp_correction_layers(enc._handle, ctypes.c_uint64(mask)),
               "op_select_mlp_correction_layers")
    assert enc.effective_policy()["mlp_correction_layers"] == list(layers_of(mask, enc.dims.num_layers))


def _differing(a, b) -> list[str]:
    return [n for n in a if not torch.equal(a[n], b[n])]


# -- which layer a mask bit means ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kernel_set", MASKED_SETS)
def test_flipping_bit_li_changes_the_forward_from_layer_li_on(kernel_set):
    weights = conf.weights_for(kernel_set, "o1", damped=True)
    rows = conf._rows(conf.LENGTHS)
    enc = conf._encoder(MODEL, weights, 128, kernel_set, 0)
    try:
        for mask in FLIP_FROM:
            _select_layers(enc, mask)
            base = conf._run(enc, rows)
            _select_layers(enc, mask)
            assert not _differing(base, conf._run(enc, rows)), "the forward is not deterministic: no bit-identity can be read"
            for li in range(N_LAYERS):
                _select_layers(enc, mask ^ (1 << li))
                got = conf._run(enc, rows)
                changed = _differing(base, got)
                TABLE.append(f"{MODEL:9s} {kernel_set:24s} mask {mask:04b} bit {li} flipped: entries that changed: {' '.join(changed)}")
                same = [f"hidden_{i}" for i in range(li + 1)]
                assert not set(same) & set(changed), f"mask {mask:04b}, bit {li}: changed at or before the input of layer {li}: {changed}"
                assert f"hidden_{li + 1}" in changed, f"mask {mask:04b}, bit {li}: the output of layer {li} did not change ({changed})"
                if li == N_LAYERS - 1:
                    assert "prune" in changed and "rank" in changed, changed
    finally:
        enc.close()


def test_the_calibrated_mask_pinned_on_a_fresh_handle_is_the_calibrated_forward():
    """base dims at full depth on reference-initialised weights calibrate to set 8 with the correction kept in some layers
    (test_gpu_calibration.py); that set and op_calibration.mlp_layers pinned on a fresh handle give the same outputs, bit
    for bit, hidden states included -- and another mask of as many layers does not."""

    from open_provence_amd.engine import HipEncoder
    from open_provence_amd.synthetic import named_dims, refinit_state_dict, synth_pair_batch

    dims = named_dims("base")
    state = refinit_state_dict(dims, seed=7)
    full = synth_pair_batch(dims, 6, 512, seed=99)
    rows = [full[i][:n] for i, n in enumerate((512, 17, 130, 333, 64, 257))]
    outs = {}
    enc = HipEncoder(dims, device="cuda:0", precision="bf16x3", flags=0)
    try:
        enc.load_state_dict(state, calibrate=1e-4)
        cal = enc.calibration
        assert cal["chosen_set"] == "f16+mlp-f16-f8-w" and 0 < len(cal["mlp_correction_layers"]) < dims.num_layers, cal
        kept = cal["mlp_correction_layers"]
        outs["calibrated"] = conf._run(enc, rows)  # (the first batch: audited against the reference set, the mask pinned again)
        assert enc.effective_policy()["kernel_set"] == "f16+mlp-f16-f8-w" and enc.effective_policy()["mlp_correction_layers"] == kept
    finally:
        enc.close()
    mask = sum(1 << li for li in kept)
    n = dims.num_layers
    reversed_mask = sum(1 << (n - 1 - li) for li in kept)
    if reversed_mask == mask:  # a palindrome: take the mask shifted by one layer instead
        reversed_mask = mask >> 1
    enc = HipEncoder(dims, device="cuda:0", precision="bf16x3", flags=0)
    try:
        enc.load_state_dict(state, calibrate=False, kernel_set="f16+mlp-f16-f8-w")
        for label, m in (("pinned", mask), ("reversed", reversed_mask)):  # ("reversed": bit order reversed, the wrong mask)
            _select_layers(enc, m)
            outs[label] = conf._run(enc, rows)
    finally:
        enc.close()
    TABLE.append(f"base x {n} layers, calibrated mask {kept}: pinned on a fresh handle differs at {_differing(outs['calibrated'], outs['pinned'])}, "
                 f"the bit-reversed mask at {len(_differing(outs['calibrated'], outs['reversed']))} entries")
    assert not _differing(outs["calibrated"], outs["pinned"])
    first = first_differing_layer(mask, reversed_mask)
    changed = _differing(outs["calibrated"], outs["reversed"])
    assert f"hidden_{first + 1}" in changed and not {f"hidden_{i}" for i in range(first + 1)} & set(changed), (kept, changed)


# -- what a masked forward computes -------------------------------------------------------------------------------------------
MASK_CASES = [(s, m) for s, masks in MODEL_MASKS.items() for m in masks]


@pytest.mark.parametrize("kernel_set,mask", MASK_CASES, ids=[f"{s}-{m:04b}" for s, m in MASK_CASES])
def test_masked_forward_matches_the_model_of_its_mask(kernel_set, mask):
    weights = conf.weights_for(kernel_set, "o1", damped=True)
    lengths = tuple(conf.LENGTHS)
    own = conf._model(MODEL, weights, 128, lengths, kernel_set, layers_of(mask))
    exact = conf._model(MODEL, weights, 128, lengths, "exact")
    enc = conf._encoder(MODEL, weights, 128, kernel_set, 0)
    try:
        _select_layers(enc, mask)
        got = conf._run(enc, conf._rows(lengths))
        assert enc.effective_policy()["mlp_correction_layers"] == list(layers_of(mask))
    finally:
        enc.close()
    label = f"{MODEL:9s} {kernel_set:24s} {'mask ' + format(mask, '04b'):18s} {weights:14s} w128   list "
    lines_before = len(conf.TABLE)
    try:
        conf._compare(label, got, own, exact, f"hidden_{N_LAYERS}")
    finally:
        TABLE.extend(conf.TABLE[lines_before:])
        del conf.TABLE[lines_before:]
    order = list(own)
    for other in neighbours(mask):
        theirs = conf._model(MODEL, weights, 128, lengths, kernel_set, layers_of(other))
        behind = order[order.index(f"hidden_{first_differing_layer(mask, other) + 1}"):]
        dist = {n: (am.rms(got[n] - own[n]), am.rms(got[n] - theirs[n])) for n in behind}
        worst = max(dist, key=lambda n: am._ratio(*dist[n]))
        TABLE.append(f"{label} | against mask {other:04b} from {behind[0]}: own / other model rms closest at {worst}: "
                     f"{dist[worst][0]:.2e} / {dist[worst][1]:.2e}")
        not_closer = [n for n, (mine, their) in dist.items() if not mine < their]
        assert not not_closer, f"{label}: as close to mask {other:04b}'s model as to its own at {not_closer}: {[dist[n] for n in not_closer]}"
