"""The float64 model of the kernel sets' arithmetic (tests/arith_model.py), on the CPU: it is the oracle when nothing is
rounded, the inputs of the GPU conformance tests reach the branches they are meant to reach, and the bounds those tests
apply would see a subtly wrong kernel.

Mutations: each lo term dropped, each fp16 family on bf16, the sliding window one key short, the e4m3 lo scale off by one,
emulated on the GPU test's own models, rows and O(1) weights (bf16-valued for the sets without a lo(W) term, as there).
157 of 188 exceed the bound.  The 31 that do not are listed in UNDETECTED with the reason; they are all on the sets
whose single-pass fp16 attention (10, 11) or attention side (8, 9) dominates their error, plus the bf16 rounding of an
MLP activation that the row path carries as an fp16 pair.  The test fails if that list is wrong in either direction.
"""

from __future__ import annotations

import math

import numpy as np
import pytest
import torch

import arith_model as am
from arith_model import SCHEMES, Scheme

LENGTHS = [0, 1, 2, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 700]
WINDOWS = [128, 2, 30, 64, 200, 1024]


def _dims(H=256, I=1024, nh=4, nl=3, window=128, pooling="cls", labels=1):
    from open_provence_amd.config import EncoderDims

    return EncoderDims.from_base_model_config(
        dict(model_type="modernbert", vocab_size=512, hidden_size=H, intermediate_size=I, num_hidden_layers=nl,
             num_attention_heads=nh, local_attention=window, global_attn_every_n_layers=nl, global_rope_theta=160000.0,
             local_rope_theta=10000.0, max_position_embeddings=2048, pad_token_id=0, cls_token_id=1, sep_token_id=2,
             classifier_pooling=pooling),
        num_labels=labels)


def _rows(lengths, seed=7):
    rng = np.random.default_rng(seed)
    return [([1] + rng.integers(3, 512, n - 1).tolist()) if n else [] for n in lengths]


# 1. exactness ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("window,pooling,labels,pre_norm", [(128, "cls", 1, False), (2, "cls", 1, False), (30, "mean", 3, False),
                                                           (1024, "cls", 2, True), (64, "mean", 1, True)])
def test_exact_scheme_is_the_float64_oracle(window, pooling, labels, pre_norm):
    from open_provence_amd.synthetic import pad_rows, synth_state_dict
    from oracle.modernbert_oracle import oracle_forward

    torch.set_num_threads(8)
    dims = _dims(H=128, I=256, nh=2, nl=3, window=window, pooling=pooling, labels=labels)
    state = synth_state_dict(dims, 4)
    lengths = [1, 2, 33, 0, 65, 200, 129]
    rows = _rows(lengths)
    got = am.forward(state, dims, rows, "exact", prune_pre_final_norm=pre_norm)
    keep = [i for i, n in enumerate(lengths) if n]
    ids, mask = pad_rows([rows[i] for i in keep])
    ref = oracle_forward(state, dims, ids, mask, dtype=torch.float64, return_hidden=True, prune_pre_final_norm=pre_norm)
    m = mask.bool()
    n = dims.num_layers
    for i in range(n + 1):
        mine = got.hidden[i][keep]
        if i == n and pre_norm:  # entry N is the raw last layer; its final_norm is the oracle's last entry
            w = state["ranking_model.model.final_norm.weight"].double()
            mine = am._layer_norm(mine, w, dims.norm_eps)
        assert float((mine[m] - ref.hidden_states[i][m]).abs().max()) <= 1e-10, i
    assert float((got.prune[keep][m] - ref.pruning_logits[m]).abs().max()) <= 1e-10
    assert float((got.rank[keep] - ref.ranking_logits).abs().max()) <= 1e-10
    assert bool((got.rank[[i for i, n in enumerate(lengths) if not n]] == 0).all())
    for h in got.hidden:  # zeros beyond every row
        assert bool((h[~am.valid_mask(lengths, h.shape[1])] == 0).all())


def test_contract_restates_the_operand_formats():
    torch.manual_seed(0)
    a, b = torch.randn(64, 256, dtype=torch.float64), torch.randn(256, 32, dtype=torch.float64)
    exact = a @ b
    err = {k: float((am.contract(a, b, k) - exact).abs().max() / exact.abs().max()) for k in SCHEMES}
    assert err["exact"] == 0.0
    # more planes, less error; each order of magnitude is what the formats' significant bits give
    assert err["bf16x3"] < err["f16+2f8"] < err["f16+f8"] < err["f16"] < err["bf16"]
    assert err["f16x3"] < err["f16x2"] < err["f16"] and err["bf16x3"] < err["bf16x2"] < err["bf16"]
    assert 1e-4 < err["bf16"] < 3e-2 and 1e-5 < err["f16"] < 4e-3 and err["bf16x3"] < 1e-4


# 2. coverage of the inputs the GPU tests use -------------------------------------------------------------------------------------
def test_length_list_is_the_conformance_list():
    import test_kernel_set_conformance as conf

    assert conf.LENGTHS == LENGTHS and conf.WINDOWS == WINDOWS
    assert max(conf.LONG_LENGTHS) == 2048


def test_peaked_weights_reach_the_late_rescale_branch(monkeypatch):
    """On the peaked recipe the lazy reference moves after a query's first tile for >= 20 % of the query-heads, in the
    global layer (64-key tiles) and in the sliding-window layers (32-key tiles) alike -- on the float64 scores, in the
    kernels' tile order, with their threshold of 2^6."""

    torch.set_num_threads(8)
    dims = _dims()
    state = am.peaked_state_dict(dims, 21)
    seen = {True: [0, 0], False: [0, 0]}
    span, top = [0.0], [0.0]
    real = am.attention

    def spy(q, k, v, vis, arith, layer, tile):
        s = q @ k.transpose(-1, -2)
        _, late = am.lazy_reference(s, vis, tile)
        seen[tile == am.TILE_KEYS_GLOBAL][0] += int(late.sum())
        seen[tile == am.TILE_KEYS_GLOBAL][1] += late.numel()
        sv = s.masked_fill(~vis, math.nan)
        span[0] = max(span[0], float((sv.nan_to_num(-math.inf).amax(-1) - sv.nan_to_num(math.inf).amin(-1)).max()))
        top[0] = max(top[0], float(s.masked_fill(~vis, 0.0).abs().max()))
        return real(q, k, v, vis, arith, layer, tile)

    monkeypatch.setattr(am, "attention", spy)
    am.forward(state, dims, _rows(LENGTHS), "exact")
    frac = {glob: n / total for glob, (n, total) in seen.items()}
    print(f"late rescales: global {frac[True]:.1%}, local {frac[False]:.1%}; widest score span {span[0]:.1f}, "
          f"largest |score| {top[0]:.1f} log2 units")
    assert frac[True] >= 0.2 and frac[False] >= 0.2, frac
    # the scores stay far inside fp16's range (the fp16 attention's accumulators start at -m; q itself is smaller still)
    assert top[0] < 2.0**15


@pytest.mark.parametrize("window", WINDOWS)
def test_window_edges_land_on_and_between_tile_boundaries(window):
    """For every window of the sweep some query's lowest visible key is the first key of a 32-key tile and some query's is
    inside one, and likewise for the highest visible key (the last key of a tile / inside one), within the length list."""

    hw = window // 2
    on_lo = mid_lo = on_hi = mid_hi = False
    for n in LENGTHS:
        for q in range(n):
            lo, hi = q - hw, q + hw
            if lo > 0:
                on_lo |= lo % am.TILE_KEYS_LOCAL == 0
                mid_lo |= lo % am.TILE_KEYS_LOCAL != 0
            if hi < n - 1:
                on_hi |= hi % am.TILE_KEYS_LOCAL == am.TILE_KEYS_LOCAL - 1
                mid_hi |= hi % am.TILE_KEYS_LOCAL != am.TILE_KEYS_LOCAL - 1
    assert on_lo and mid_lo and on_hi and mid_hi, (window, on_lo, mid_lo, on_hi, mid_hi)


# 3. sensitivity: the bounds see the mutations ----------------------------------------------------------------------------------
# the GPU test's models: every row set on the row model, the panel-only sets and the panel form of sets 3 / 4 on panel512
SENS_CASES = [("row", s) for s in ("bf16x3", "bf16-weights", "bf16", "f16-f8", "f16-f8-w", "f16")] + [
    ("panel512", s) for s in ("f16-f8", "f16-f8-w", "bf16x3+wi-f16-f8-w", "bf16-weights+wi-f16-f8", "f16+mlp-f16-f8-w",
                              "f16+mlp-f16-f8", "f16-f8-w+attn-f16", "f16-f8+attn-f16")]

# Mutations the GPU test's bound cannot see on its O(1) inputs (the model, rows and weights of its default case), per
# (model, set).  Each is a correction term well below the error of a cheaper family of the same set.
_UNDETECTED: dict[tuple[str, str], list[str]] = {
    # the whole-layer kernel carries h as an fp16 (hi, lo) pair: a bf16 pair is as exact
    ("row", "f16-f8"): ["bf16 for fp16: mlp_out"],
    ("row", "f16-f8-w"): ["bf16 for fp16: mlp_out"],
    # the single-pass fp16 attention side dominates the error of the MLP's correction terms
    ("panel512", "f16+mlp-f16-f8-w"): ["drop left lo: mlp_out", "drop left lo: wi", "drop right lo: mlp_out", "drop right lo: wi",
                                       "lo shift off by one: mlp_out", "lo shift off by one: wi"],
    ("panel512", "f16+mlp-f16-f8"): ["drop left lo: mlp_out", "drop left lo: wi", "lo shift off by one: mlp_out", "lo shift off by one: wi"],
    # the single-pass fp16 attention dominates the error of the weight GEMMs' correction terms
    ("panel512", "f16-f8-w+attn-f16"): ["drop left lo: attn_out", "drop left lo: mlp_out", "drop left lo: wi", "drop left lo: wqkv",
                                        "drop right lo: attn_out", "drop right lo: mlp_out", "drop right lo: wi", "drop right lo: wqkv",
                                        "lo shift off by one: attn_out", "lo shift off by one: mlp_out", "lo shift off by one: wi",
                                        "lo shift off by one: wqkv"],
    ("panel512", "f16-f8+attn-f16"): ["drop left lo: attn_out", "drop left lo: mlp_out", "drop left lo: wi", "lo shift off by one: attn_out",
                                      "lo shift off by one: mlp_out", "lo shift off by one: wi", "lo shift off by one: wqkv"],
}
UNDETECTED = {(m, s, name) for (m, s), names in _UNDETECTED.items() for name in names}


def _mutations(arith: am.Arith):
    """name -> mutated Arith: each lo term dropped, each fp16 family on bf16, the window one key short, the e4m3 lo scale
    off by one (decoded as x 2^11 where it was encoded x 2^12: the correction term doubled)."""

    out = {}
    for fam in am.FAMILIES:
        s = arith.schemes[fam]
        for side in ("left", "right"):
            if getattr(s, f"{side}_lo"):
                lo = ("", s.right_lo) if side == "left" else (s.left_lo, "")
                out[f"drop {side} lo: {fam}"] = arith.with_family(fam, Scheme(s.name + "-", s.hi, *lo, s.lo_decode))
        if s.hi is torch.float16:
            pairs = (s.left_lo if s.left_lo == "pair" else "", s.right_lo if s.right_lo == "pair" else "")
            out[f"bf16 for fp16: {fam}"] = arith.with_family(fam, Scheme(s.name + "b", torch.bfloat16, *pairs))
        if "e4m3" in (s.left_lo, s.right_lo):
            out[f"lo shift off by one: {fam}"] = arith.with_family(fam, Scheme(s.name + "s", s.hi, s.left_lo, s.right_lo, am.LO_SHIFT - 1))
    out["window one key short"] = am.Arith(arith.schemes, arith.layer0_wqkv, window_delta=-1)
    return out


@pytest.mark.parametrize("model,kernel_set", SENS_CASES)
def test_mutations_exceed_the_bound(model, kernel_set):
    import test_kernel_set_conformance as conf

    torch.set_num_threads(16)
    weights = conf.weights_for(kernel_set, "o1")
    state, dims, rows = conf._state(model, weights), conf._dims(model), conf._rows(conf.LENGTHS)
    exact = am.model_entries(am.forward(state, dims, rows, "exact"))
    arith = am.arith_for(kernel_set, conf.PATH_OF[model])
    own = am.model_entries(am.forward(state, dims, rows, arith))
    bnd = am.bounds(own, exact)
    missed = set()
    for name, mutant in _mutations(arith).items():
        per = am.ratios(am.model_entries(am.forward(state, dims, rows, mutant)), own, bnd)
        where = max(per, key=lambda n: per[n][0])
        print(f"[sensitivity] {model:9s} {kernel_set:24s} {weights:8s} {name:32s} x{per[where][0]:8.2f} of the bound at {where}")
        if am.first_over(per) is None:
            missed.add((model, kernel_set, name))
    expected = {m for m in UNDETECTED if m[:2] == (model, kernel_set)}
    assert missed == expected, f"undetected {sorted(missed)}, listed {sorted(expected)}"
