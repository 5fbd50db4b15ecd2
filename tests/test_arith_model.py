"""The float64 model of the kernel sets' arithmetic (tests/arith_model.py), on the CPU: it is the oracle when nothing is
rounded, the inputs of the GPU conformance tests reach the branches they are meant to reach, and the bounds those tests
apply would see a subtly wrong kernel.

Mutations: each lo term dropped, each fp16 family on bf16, the sliding window one key short, the e4m3 lo scale off by one,
emulated on the GPU test's own models, rows and O(1) weights (bf16-valued for the sets without a lo(W) term, as there) --
plain and, for the sets the GPU test runs on it, MLP-isolating (every attn.Wo x 2^-8: am.mlp_isolating_state_dict).  A
mutation counts as seen when either recipe's bound sees it.  On the default models (row, panel512) 177 of 188 exceed a
bound; the plain recipe alone misses 31, and the 20 of those that sit in the Wi GEMM or the MLP output projection of the
composite sets 8 - 11 come out at 5 - 18 x on the MLP-isolating one.  The 11 that stay are listed in UNDETECTED with the
reason: the q / k / v and output projections' correction terms of sets 10 / 11, at the size of the single-plane fp16
rounding of q, k, v^T and p next to them, and the bf16 rounding of an MLP activation that the row path carries as an fp16
pair.  On the added shapes (768 x 1152, hidden 128, 256 x 320) 93 of 100 exceed a bound and the 7 that do not carry the
same names.  The test fails if the list is wrong in either direction.  Detections under 1.2 x are printed as thin.

Rows beyond 2048 tokens (tests/test_kernel_set_long_rows.py): a RoPE position clamped at 2047 or taken modulo 4096, a full
attention that stops after 32 key tiles and a sliding-window tile range computed from query 0 for late query blocks, emulated
on that module's rows (4097, 2049, 5), are each 46 - 17 000 x the bound (>= 10 x required); the library's former once-rounded
inv_freq stays at 0.1 - 0.3 x and is listed as unseen -- the RoPE tables have a bit-level test of their own for that reason
(tests/test_rope_tables.py).

The layer mask of kernel sets 8 / 9: the model of a mask equals its neighbours' up to the first layer where they differ and
is separated from them behind it (figures printed: the yardstick of tests/test_kernel_set_masks.py).
"""

from __future__ import annotations

import dataclasses
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
# ... and the shapes the conformance test adds, under the sets they add
SHAPE_SENS_CASES = [("engte", "f16-f8-w"), ("engte", "f16+mlp-f16-f8-w"), ("engte", "f16-f8-w+attn-f16"),
                    ("row128", "f16-f8-w"), ("row128", "f16"), ("row320", "f16-f8-w")]
THIN = 1.2  # a mutation detected at less than this x the bound is printed as thin (no assertion hangs on it)

# Mutations the GPU test's bounds cannot see on its O(1) inputs, plain or MLP-isolating (attn.Wo x 2^-8), per (model, set).
_ROW_PAIR = "the whole-layer kernel carries h as an fp16 (hi, lo) pair: a bf16 pair is as exact"
_ATTN_SIDE = ("q, k, v^T and p are rounded to single-plane fp16 right behind the q / k / v projection and right in front of the "
              "output projection, at the same 2^-12 relative size as the terms dropped")
_UNDETECTED: dict[tuple[str, str], tuple[str, list[str]]] = {
    ("row", "f16-f8"): (_ROW_PAIR, ["bf16 for fp16: mlp_out"]),
    ("row", "f16-f8-w"): (_ROW_PAIR, ["bf16 for fp16: mlp_out"]),
    ("panel512", "f16-f8-w+attn-f16"): (_ATTN_SIDE, ["drop left lo: attn_out", "drop left lo: wqkv", "drop right lo: attn_out",
                                                     "drop right lo: wqkv", "lo shift off by one: attn_out", "lo shift off by one: wqkv"]),
    ("panel512", "f16-f8+attn-f16"): (_ATTN_SIDE, ["drop left lo: attn_out", "lo shift off by one: attn_out", "lo shift off by one: wqkv"]),
    # the added shapes: a subset of the same names, for the same reasons
    # ("drop right lo: wqkv" is seen there, thinly: 1.04 x on the plain recipe)
    ("engte", "f16-f8-w+attn-f16"): (_ATTN_SIDE, ["drop left lo: attn_out", "drop left lo: wqkv", "drop right lo: attn_out",
                                                  "lo shift off by one: attn_out", "lo shift off by one: wqkv"]),
    ("row128", "f16-f8-w"): (_ROW_PAIR, ["bf16 for fp16: mlp_out"]),
    ("row320", "f16-f8-w"): (_ROW_PAIR, ["bf16 for fp16: mlp_out"]),
}
UNDETECTED = {(m, s, name) for (m, s), (_, names) in _UNDETECTED.items() for name in names}


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
    out["window one key short"] = dataclasses.replace(arith, window_delta=-1)
    return out


def test_the_undetected_list_is_the_named_eleven():
    """On the GPU test's default models at most the 11 named mutations stay listed; the added shapes list a subset of the
    same names."""

    default = {u for u in UNDETECTED if u[0] in ("row", "panel512")}
    assert len(default) <= 11, sorted(default)
    names = {(s, n) for _, s, n in default}
    assert all((s, n) in names for m, s, n in UNDETECTED), sorted(UNDETECTED - default)


@pytest.mark.parametrize("model,kernel_set", SENS_CASES + SHAPE_SENS_CASES)
def test_mutations_exceed_the_bound(model, kernel_set):
    """Each mutation under the plain O(1) recipe and, for the sets the GPU test runs on it, under the MLP-isolating one: a
    mutation is detected when either recipe's bound sees it."""

    import test_kernel_set_conformance as conf

    torch.set_num_threads(16)
    dims, rows = conf._dims(model), conf._rows(conf.LENGTHS)
    arith = am.arith_for(kernel_set, conf.PATH_OF[model])
    mutants = _mutations(arith)
    best = {name: 0.0 for name in mutants}
    # the damped recipe only where the conformance test runs it (the panel models, DAMPED_SETS) -- except that the row
    # sets 3 / 4 take it too: cheap, and it shows the recipe does not rescue their bf16-pair mutation
    damped = kernel_set in conf.DAMPED_SETS and (model in conf.DAMPED_MODELS or conf.PATH_OF[model] == "row")
    for weights in [conf.weights_for(kernel_set, "o1")] + ([conf.weights_for(kernel_set, "o1", damped=True)] if damped else []):
        state = conf._state(model, weights)
        exact = am.model_entries(am.forward(state, dims, rows, "exact"))
        own = am.model_entries(am.forward(state, dims, rows, arith))
        bnd = am.bounds(own, exact)
        for name, mutant in mutants.items():
            per = am.ratios(am.model_entries(am.forward(state, dims, rows, mutant)), own, bnd)
            where = max(per, key=lambda n: per[n][0])
            r = per[where][0]
            note = "" if not r > 1.0 else (" (thin)" if r < THIN else "")
            print(f"[sensitivity] {model:9s} {kernel_set:24s} {weights:14s} {name:32s} x{r:8.2f} of the bound at {where}{note}")
            best[name] = max(best[name], r)
    missed = {(model, kernel_set, name) for name, r in best.items() if not r > 1.0}
    for name, r in best.items():
        if 1.0 < r < THIN:
            print(f"[sensitivity] {model:9s} {kernel_set:24s} thin: {name} is detected at x{r:.2f} only")
    expected = {m for m in UNDETECTED if m[:2] == (model, kernel_set)}
    assert missed == expected, f"undetected {sorted(missed)}, listed {sorted(expected)}"


# 4. the layer mask of kernel sets 8 / 9 ------------------------------------------------------------------------------------------
def test_layer_mask_selects_the_f16_scheme_outside_it():
    a = am.arith_for("f16+mlp-f16-f8-w", "panel", mlp_layers=[0, 2])
    for li in range(4):
        for fam in am.FAMILIES:
            want = "f16+2f8" if fam in am.MLP_FAMILIES and li in (0, 2) else "f16"
            assert a.scheme(fam, li).name == want, (fam, li)
    assert am.arith_for("f16+mlp-f16-f8", "panel").mlp_layers is None
    with pytest.raises(ValueError):
        am.arith_for("f16", "panel", mlp_layers=[0])


def test_empty_and_full_masks_are_the_f16_and_whole_depth_models():
    import test_kernel_set_masks as masks

    torch.set_num_threads(16)
    dims = _dims(H=256, I=512, nh=4, nl=3)
    from open_provence_amd.synthetic import synth_state_dict

    state = am.mlp_isolating_state_dict(synth_state_dict(dims, 3))
    rows = _rows([1, 33, 130])
    run = lambda a: am.model_entries(am.forward(state, dims, rows, a, path="panel"))  # noqa: E731
    none, f16 = run(am.arith_for("f16+mlp-f16-f8-w", "panel", [])), run(am.arith_for("f16", "panel"))
    full, whole = run(am.arith_for("f16+mlp-f16-f8-w", "panel", range(3))), run(am.arith_for("f16+mlp-f16-f8-w", "panel"))
    for n in none:
        assert torch.equal(none[n], f16[n]) and torch.equal(full[n], whole[n]), n
    assert masks.neighbours(0b0101, 4) == [0b0100, 0b0111, 0b0001, 0b1101, 0b1010, 0b0010, 0b1111, 0b0000]


@pytest.mark.parametrize("kernel_set", ["f16+mlp-f16-f8-w", "f16+mlp-f16-f8"])
def test_neighbouring_masks_are_separated_at_the_first_differing_layer(kernel_set):
    """For the masks the GPU test pins (tests/test_kernel_set_masks.py), on its model, rows and damped weights: the model of
    every neighbouring mask (one bit flipped, shifted by one layer, bit order reversed, all, none) equals the pinned
    mask's up to the first layer where the masks differ, and leaves it at the entry behind that layer by more than 100 x
    the comparison's floor.  rms(model A - model B) there is printed next to rms(model A - exact): the yardstick for the GPU
    test's "closer to its own mask's model" clause, which holds for any kernel within half of the first figure."""

    import test_kernel_set_conformance as conf
    import test_kernel_set_masks as masks

    n_layers = conf.SHAPES[masks.MODEL][3]
    weights = conf.weights_for(kernel_set, "o1", damped=True)
    lengths = tuple(conf.LENGTHS)
    exact = conf._model(masks.MODEL, weights, 128, lengths, "exact")
    for mask in masks.MODEL_MASKS[kernel_set]:
        own = conf._model(masks.MODEL, weights, 128, lengths, kernel_set, masks.layers_of(mask, n_layers))
        for other in masks.neighbours(mask, n_layers):
            theirs = conf._model(masks.MODEL, weights, 128, lengths, kernel_set, masks.layers_of(other, n_layers))
            first = masks.first_differing_layer(mask, other)
            for li in range(first + 1):
                assert torch.equal(own[f"hidden_{li}"], theirs[f"hidden_{li}"]), (mask, other, li)
            entry = f"hidden_{first + 1}"
            apart, err = am.rms(own[entry] - theirs[entry]), am.rms(own[entry] - exact[entry])
            print(f"[mask sensitivity] {kernel_set:18s} mask {mask:04b} vs {other:04b}: first differing layer {first}, at {entry} "
                  f"rms(A - B) {apart:.3e}, rms(A - exact) {err:.3e}, ratio {apart / err:.2f}")
            assert apart > 100 * am.FLOOR * am.rms(exact[entry]), (mask, other, apart)


# 5. rows beyond 2048 tokens: the mistakes tests/test_kernel_set_long_rows.py is there for ------------------------------------------
LONG_ROW_CASES = [("row", "bf16x3"), ("row", "f16"), ("panel512", "bf16x3")]
LONG_ROW_DETECTED = 10.0  # x the bound, as tests/test_geometry_inputs.py
PARENT_INV_FREQ = "inv_freq rounded once, (float)(1.0 / pow(theta, e))"
# (model, set, mutation) under 10 x the bound -> reason.  The once-rounded inv_freq is what the library computed before
# tests/test_rope_tables.py existed: one ulp off in 10 / 8 of 32 entries, 1.2e-4 / 6.1e-5 in the tables at position 8191, and
# inside the conformance bound almost everywhere -- which is why the tables have a bit-level test of their own.
_ONCE_ROUNDED = "an angle off by position x 2^-24 relative moves the logits by 1e-4 .. 1e-3, inside what the set's own rounding moves them by"
LONG_ROW_UNSEEN = {  # (measured worst ratio, reason)
    ("row", "bf16x3", PARENT_INV_FREQ): (0.27, _ONCE_ROUNDED),
    ("row", "f16", PARENT_INV_FREQ): (0.11, _ONCE_ROUNDED),
    ("panel512", "bf16x3", PARENT_INV_FREQ): (0.23, _ONCE_ROUNDED),
}


def _long_row_mutations(dims):
    """name -> keywords of ``am.forward``: what a kernel that is wrong only far into a row would compute."""

    def table_rows(index):  # the RoPE table row of position p taken at index(p)
        def rope(head_dim, theta, n):
            cos, sin = am._rope(head_dim, theta, n)
            at = index(torch.arange(n))
            return cos[at], sin[at]
        return rope

    def once_rounded(head_dim, theta, n):  # build_rope_host before its fix, restated
        inv = torch.tensor([1.0 / math.pow(float(theta), 2.0 * k / head_dim) for k in range(head_dim // 2)], dtype=torch.float64).float()
        angle = torch.arange(n, dtype=torch.float32)[:, None] * inv[None, :]
        emb = torch.cat((angle, angle), dim=-1).double()
        return emb.cos().float().double(), emb.sin().float().double()

    def stops_after_32_tiles(vis, is_global):  # full attention: keys from 32 x 64 on are never visited
        return vis & (torch.arange(vis.shape[1]) < 32 * am.TILE_KEYS_GLOBAL)[None, :] if is_global else vis

    def tile_range_from_zero(vis, is_global):
        """Sliding window: from the 9th block of 128 queries on, the range of 32-key tiles is computed as for the block at 0."""

        if is_global:
            return vis
        n = vis.shape[0]
        last_tile = (127 + dims.half_window) // am.TILE_KEYS_LOCAL
        beyond = torch.arange(n) >= (last_tile + 1) * am.TILE_KEYS_LOCAL
        late_block = torch.arange(n) // 128 >= 8
        return vis & ~(late_block[:, None] & beyond[None, :])

    return {
        "RoPE position clamped at 2047": dict(rope=table_rows(lambda p: p.clamp(max=2047))),
        "RoPE position modulo 4096": dict(rope=table_rows(lambda p: p % 4096)),
        "full attention stops after the 32nd 64-key tile": dict(visibility=stops_after_32_tiles),
        "window tile range from query 0 beyond the 8th block": dict(visibility=tile_range_from_zero),
        PARENT_INV_FREQ: dict(rope=once_rounded),
    }


@pytest.mark.parametrize("model,kernel_set", LONG_ROW_CASES)
def test_long_row_mutations_exceed_ten_times_the_bound(model, kernel_set):
    """On the rows (4097, 2049, 5) of tests/test_kernel_set_long_rows.py, its peaked weights and window: each emulated mistake's
    worst ratio to the bound ``conf._compare`` applies.  One under 10 x is listed in LONG_ROW_UNSEEN, not dropped."""

    import test_kernel_set_conformance as conf
    import test_kernel_set_long_rows as long_rows

    torch.set_num_threads(16)
    lengths, path = long_rows.MID, conf.PATH_OF[model]
    weights = conf.weights_for(kernel_set, "peaked")
    dims, state, rows = conf._dims(model, 128, max_position_embeddings=long_rows.MAX_POSITIONS), conf._state(model, weights), conf._rows(lengths)
    own = conf._model(model, weights, 128, lengths, kernel_set)
    bnd = am.bounds(own, conf._model(model, weights, 128, lengths, "exact"))
    arith = am.arith_for(kernel_set, path)
    same = am.model_entries(am.forward(state, dims, rows, arith, path=path, rope=am._rope, visibility=lambda vis, is_global: vis))
    assert all(torch.equal(same[k], own[k]) for k in own)  # the hooks that change nothing are the model
    low = set()
    for name, hooks in _long_row_mutations(dims).items():
        per = am.ratios(am.model_entries(am.forward(state, dims, rows, arith, path=path, **hooks)), own, bnd)
        where = max(per, key=lambda n: per[n][0])
        r = per[where][0]
        note = "" if r >= LONG_ROW_DETECTED else "UNDER 10 x"
        print(f"[long-row sensitivity] {model:9s} {kernel_set:8s} {name:52s} x{r:12.2f} of the bound at {where:8s} (prune x{per['prune'][0]:.2f}, "
              f"max |d prune| {per['prune'][2]:.2e}; rank x{per['rank'][0]:.2f}) {note}")
        if r < LONG_ROW_DETECTED:
            low.add((model, kernel_set, name))
    listed = {k for k in LONG_ROW_UNSEEN if k[:2] == (model, kernel_set)}
    assert low == listed, f"under {LONG_ROW_DETECTED} x: {sorted(low)}, listed {sorted(listed)}"
