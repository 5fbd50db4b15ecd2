"""Every kernel set on every dispatch path against the float64 model of ITS OWN arithmetic (tests/arith_model.py), entry by
entry: each hidden state (op_forward_packed_hidden, fp32, padded), the pruning logits and the ranking logits.

Statistic per entry, over the valid tokens: RMS and max-abs of (kernel - model of the pinned set).  Bound: 2 x the RMS and
4 x the max-abs of (model - exact) on the same rows, floored at 1e-6 x the entry's RMS (fp32 accumulation).  A set whose
kernels are subtly wrong -- a dropped correction term, a window one key short, a mis-scaled e4m3 plane -- moves its error
by more than that (tests/test_arith_model.py emulates those mutations on these models and rows and lists the ones the
bound cannot see).  A composite set (5, 6, 8 - 11) must in addition be closer to its own model than to the model of the
set whose kernels it replaces in some families: one that silently ran its base set's kernels stays inside 2 x.

Weights: O(1) (``synth_state_dict``) and peaked (its q rows scaled up: the late-rescale branch of the attention runs).  The
sets without a lo(W) term (am.BF16_WEIGHT_SETS) exist for bf16-valued checkpoints and run on bf16-valued versions of both:
on fp32-valued weights their rounding of W would dominate their error and hide every other departure.  The sets that carry
a correction term in the MLP behind an fp16 weight plane (3, 4, 8 - 11) run a second time on the MLP-isolating recipe
(``am.mlp_isolating_state_dict``: every attn.Wo x 2^-8): on the plain weights the single-pass fp16 attention side of sets
8 - 11 hides a dropped or mis-scaled correction term of their MLP, which is all those sets add to "f16".  Both recipes stay:
the attention-side mutations are only visible on the plain one.  The layer mask of sets 8 / 9: tests/test_kernel_set_masks.py.

The CPU side (one model forward per (model, weights, window, rows, set)) is computed once per module.  The table of results
is printed when the module ends, one line per comparison in the order they ran."""

from __future__ import annotations

import functools

import numpy as np
import pytest
import torch

import arith_model as am

pytestmark = pytest.mark.gpu

LENGTHS = [0, 1, 2, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 700]
LONG_LENGTHS = [2048, 5]
WINDOWS = [128, 2, 30, 64, 200, 1024]
ACCEPTED_WINDOWS = WINDOWS  # every window of the sweep runs; op_create refuses a negative one
REFUSED_WINDOWS = [-2]
ALL_SETS = list(am.KERNEL_SETS)

# model -> (hidden, intermediate, heads, layers); one global layer, then sliding-window layers
MODELS = {
    "row": (256, 1024, 4, 3),
    "panel512": (512, 2048, 8, 3),
    "panel768": (768, 3072, 12, 2),
    "tiled": (384, 192, 6, 2),
    "engte": (768, 1152, 12, 2),  # the published en-gte shape: nine 128-wide Wi tiles, 36 k-steps of the MLP output projection
    "h1024": (1024, 512, 16, 2),  # four 256-wide tiles, 16 heads: the largest hidden op_create takes
    "row128": (128, 512, 2, 3),  # the other row shape with fp16 / e4m3 packs; no wave-pair kernel
    "row320": (256, 320, 4, 3),  # intermediate not 4 x hidden: 5 x 64, an odd count in the wave-pair kernel's MLP loop
}
# ... and the 4-layer panel model of tests/test_kernel_set_masks.py (the layer mask of sets 8 / 9)
# ... and the 3-layer tiled model of tests/test_kernel_set_geometry.py (its layer patterns have three letters)
SHAPES = {**MODELS, "panel512x4": (512, 2048, 8, 4), "tiled3": (384, 192, 6, 3)}
PATH_OF = {"row": "row", "panel512": "panel", "panel768": "panel", "tiled": "tiled", "engte": "panel", "h1024": "panel",
           "row128": "row", "row320": "row", "panel512x4": "panel", "tiled3": "tiled"}

# What each path supports, as an explicit expectation (op_plan.h set_available): every other set must be refused.
ROW_SETS = ["bf16x3", "bf16-weights", "bf16", "f16-f8", "f16-f8-w", "f16"]
SUPPORTED = {
    "row": ROW_SETS,
    "panel512": ALL_SETS,
    "panel768": ALL_SETS,
    "tiled": ["bf16x3"],
    "engte": ALL_SETS,
    "h1024": ALL_SETS,
    "row128": ROW_SETS,
    "row320": ROW_SETS,
}
# the MLP-isolating recipe (am.mlp_isolating_state_dict) runs on the sets whose weight hi plane is fp16 and that carry a
# correction term in the MLP: 8 - 11, and 3 / 4, whose fp16 + e4m3 MLP launches sets 8 - 11 reuse (launch_panel_f8)
DAMPED_SETS = ["f16-f8", "f16-f8-w", "f16+mlp-f16-f8-w", "f16+mlp-f16-f8", "f16-f8-w+attn-f16", "f16-f8+attn-f16"]
DAMPED_MODELS = ["panel512", "panel768", "engte", "h1024"]
# flag -> sets it leaves available on the row / panel path (the test hooks' header comments in open_provence_hip.h)
SUPPORTED_WITH_FLAG = {
    ("row", "NO_SMALL_BLOCKS"): ROW_SETS,
    ("row", "NO_LAYER_PAIRS"): ROW_SETS,
    ("row", "LAYER_8X16"): ["bf16x3", "bf16-weights", "bf16"],
    ("row", "LAYER_M32"): ["bf16x3", "bf16-weights", "bf16"],
    ("row", "NO_LAYER_FUSION"): ["bf16x3", "bf16-weights", "bf16"],
    ("row", "NO_HEAD_FUSION"): ROW_SETS,
    ("row", "NO_POLICY_KERNELS"): ["bf16x3"],
    ("row", "FORCE_TILED"): ["bf16x3"],
    ("row", "ATT_WAVES_4"): ROW_SETS,
    ("row", "ATT_WAVES_8"): ROW_SETS,
    ("row", "ATTN_XCD_GROUP"): ROW_SETS,
    ("row", "NO_F8"): ["bf16x3", "bf16-weights", "bf16"],
    ("panel512", "PANEL_F8"): ALL_SETS,
    ("panel512", "PANEL_F8_WI"): ALL_SETS,
    ("panel512", "NO_F8"): ["bf16x3", "bf16-weights", "bf16"],
    ("panel512", "ATT_WAVES_4"): ALL_SETS,
    ("panel512", "ATT_WAVES_8"): ALL_SETS,
}
# the sets each flag is run under (the sets whose kernels it changes), O(1) weights
FLAG_RUNS = {
    ("row", "NO_SMALL_BLOCKS"): ROW_SETS,
    ("row", "NO_LAYER_PAIRS"): ["bf16", "f16"],
    ("row", "LAYER_8X16"): ["bf16x3", "bf16-weights", "bf16"],
    ("row", "LAYER_M32"): ["bf16-weights", "bf16"],
    ("row", "NO_LAYER_FUSION"): ["bf16x3", "bf16-weights", "bf16"],
    ("row", "NO_HEAD_FUSION"): ROW_SETS,
    ("row", "NO_POLICY_KERNELS"): ["bf16x3"],
    ("row", "FORCE_TILED"): ["bf16x3"],
    ("row", "ATT_WAVES_4"): ROW_SETS,
    ("row", "ATT_WAVES_8"): ROW_SETS,
    ("row", "ATTN_XCD_GROUP"): ROW_SETS,
    ("row", "NO_F8"): ["bf16x3", "bf16-weights", "bf16"],
    ("panel512", "PANEL_F8"): ["f16-f8", "f16-f8-w"],
    ("panel512", "PANEL_F8_WI"): ["bf16x3+wi-f16-f8-w", "bf16-weights+wi-f16-f8"],
    ("panel512", "NO_F8"): ["bf16x3", "bf16-weights", "bf16"],
    ("panel512", "ATT_WAVES_4"): ["bf16x3", "f16", "f16-f8-w+attn-f16"],
    ("panel512", "ATT_WAVES_8"): ["bf16x3", "f16", "f16-f8-w+attn-f16"],
}
# the three attention families of the window sweep: (model, set)
WINDOW_RUNS = [("row", "bf16x3"), ("row", "f16"), ("panel512", "f16-f8-w+attn-f16")]
# the evaluated term masks a pinned set reports, in _lib.OP_FAMILIES order (wqkv, qk, pv, attn_out, wi, mlp_out)
SET_TERMS = {
    "bf16x3": (3, 3, 3, 3, 3, 3),
    "bf16-weights": (1, 3, 3, 1, 1, 1),
    "bf16": (0, 0, 0, 0, 0, 0),
    "f16-f8": (1, 3, 3, 1, 1, 1),
    "f16-f8-w": (3, 3, 3, 3, 3, 3),
    "bf16x3+wi-f16-f8-w": (3, 3, 3, 3, 3, 3),
    "bf16-weights+wi-f16-f8": (1, 3, 3, 1, 1, 1),
    "f16": (0, 0, 0, 0, 0, 0),
    "f16+mlp-f16-f8-w": (0, 0, 0, 0, 0, 0),
    "f16+mlp-f16-f8": (0, 0, 0, 0, 0, 0),
    "f16-f8-w+attn-f16": (3, 0, 0, 3, 3, 3),
    "f16-f8+attn-f16": (1, 0, 0, 1, 1, 1),
}

TABLE: list[str] = []


@pytest.fixture(scope="module", autouse=True)
def _print_table():
    yield
    print("\n[conformance] model     set                      flags              weights        window rows  | worst ratio to the bound: "
          "over the entries that check a rounding scheme (hidden_0: the fp32 floor) | the kernel against exact")
    for line in TABLE:
        print("[conformance]", line)


def _dims(model: str, window: int = 128, *, layer_types: "str | None" = None, pooling: "str | None" = None,
          labels: "int | None" = None, max_position_embeddings: int = 2048):
    """``layer_types``: one letter per layer, "G" (full attention) / "L" (sliding window), None = one global layer, then
    sliding-window layers; ``pooling``: "cls" (None) / "mean"; ``labels``: ranking labels (None = 1);
    ``max_position_embeddings``: the longest row the handle takes (tests/test_kernel_set_long_rows.py: 8192)."""

    from open_provence_amd.config import EncoderDims

    H, I, nh, nl = SHAPES[model]
    cfg = dict(model_type="modernbert", vocab_size=512, hidden_size=H, intermediate_size=I, num_hidden_layers=nl,
               num_attention_heads=nh, local_attention=window, global_attn_every_n_layers=nl, global_rope_theta=160000.0,
               local_rope_theta=10000.0, max_position_embeddings=max_position_embeddings, pad_token_id=0, cls_token_id=1, sep_token_id=2)
    if layer_types is not None:
        assert len(layer_types) == nl and set(layer_types) <= {"G", "L"}, layer_types
        cfg["layer_types"] = ["full_attention" if t == "G" else "sliding_attention" for t in layer_types]
    if pooling is not None:
        cfg["classifier_pooling"] = pooling
    return EncoderDims.from_base_model_config(cfg, num_labels=1 if labels is None else labels)


def _rows(lengths, seed=7):
    rng = np.random.default_rng(seed)
    return [([1] + rng.integers(3, 512, n - 1).tolist()) if n else [] for n in lengths]


def weights_for(kernel_set: str, recipe: str, damped: bool = False) -> str:
    """The weights a set is checked on: ``recipe`` ("o1" / "peaked"), bf16-valued for the sets without a lo(W) term;
    ``damped``: then the MLP-isolating recipe on top (every attn.Wo x 2^-8, on fp16's grid)."""

    return recipe + ("-bf16" if kernel_set in am.BF16_WEIGHT_SETS else "") + ("-damped" if damped else "")


@functools.lru_cache(maxsize=None)
def _state(model: str, weights: str, window: int = 128, labels: "int | None" = None):
    from open_provence_amd.synthetic import synth_state_dict

    dims = _dims(model, window, labels=labels)  # (of a model's dims only the shapes enter its weights)
    recipe, *marks = weights.split("-")
    assert recipe in ("o1", "peaked") and set(marks) <= {"bf16", "damped"}, weights
    state = synth_state_dict(dims, 21) if recipe == "o1" else am.peaked_state_dict(dims, 21)
    if "bf16" in marks:
        state = am.bf16_valued(state)
    return am.mlp_isolating_state_dict(state) if "damped" in marks else state


@functools.lru_cache(maxsize=None)
def _model(model: str, weights: str, window: int, lengths: tuple, kernel_set: str, mlp_layers: "tuple | None" = None):
    """Entries of the model of `kernel_set` ("exact" included; `mlp_layers`: the layer mask of sets 8 / 9) on the rows of
    `lengths` -- once per module."""

    torch.set_num_threads(16)
    arith = am.arith_for(kernel_set, PATH_OF[model], mlp_layers)
    out = am.forward(_state(model, weights, window), _dims(model, window), _rows(lengths), arith, path=PATH_OF[model])
    return am.model_entries(out)


def _encoder(model: str, weights: str, window: int, kernel_set: str, flags: int, *, chunk_rows: "int | None" = None,
             prune_pre_final_norm: bool = False, dims=None):
    """``dims``: the model's dims with another layer pattern or head (``_dims(model, window, ...)``); None = ``_dims(model, window)``."""

    from open_provence_amd.engine import HipEncoder

    dims = _dims(model, window) if dims is None else dims
    enc = HipEncoder(dims, device="cuda:0", flags=flags, chunk_rows=chunk_rows, prune_pre_final_norm=prune_pre_final_norm)
    try:
        enc.load_state_dict(_state(model, weights, window, None if dims.num_labels == 1 else dims.num_labels), calibrate=False,
                            kernel_set=kernel_set)
        assert enc.effective_policy()["kernel_set"] == kernel_set
    except BaseException:
        enc.close()
        raise
    return enc


def _run(enc, rows):
    from open_provence_amd.engine import HiddenRequest
    from open_provence_amd.packing import pack_rows

    ids_np, cu_np, max_len = pack_rows(rows)
    ids = torch.from_numpy(ids_np).to(enc.device)
    cu = torch.from_numpy(cu_np).to(enc.device)
    prune, rank, hidden = enc.forward_packed(ids, cu, cu_np, max_len, hidden=HiddenRequest(pad_width=max(max_len, 1)))
    torch.cuda.synchronize()
    lengths = [len(r) for r in rows]
    padded = torch.zeros(len(rows), max(max_len, 1), 2)
    for s in range(len(rows)):
        padded[s, : lengths[s]] = prune[int(cu_np[s]) : int(cu_np[s + 1])].cpu()
    hidden = hidden.cpu()
    return am.entries([hidden[i] for i in range(hidden.shape[0])], padded, rank.cpu(), lengths)


def _flag_bits(names):
    from open_provence_amd import _lib

    bits = 0
    for n in names:
        bits |= getattr(_lib, f"OP_FLAG_{n}")
    return bits


def _compare(label: str, got, own, exact, deepest: str, base=None):
    """Record one comparison in the table; fail on the shallowest entry over its bound, then on a composite set that is
    not closer to its own model than to its base set's."""

    bnd = am.bounds(own, exact)
    per = am.ratios(got, own, bnd)
    checked = [n for n in per if not bnd[n].at_floor]
    worst = max(checked, key=lambda n: per[n][0])
    floor_worst = max((per[n][0] for n in per if bnd[n].at_floor), default=0.0)
    vs_exact = am.ratios(got, exact, bnd)
    line = (f"{label} | worst {per[worst][0]:6.3f} at {worst:8s} (floor entries {floor_worst:5.3f}) | vs exact: {deepest} rms "
            f"{vs_exact[deepest][1]:.2e} max {vs_exact[deepest][2]:.2e}, prune max {vs_exact['prune'][2]:.2e} "
            f"(model {bnd['prune'].max / am.MAX_FACTOR:.2e})")
    closer = None
    if base is not None:
        vs_base = am.ratios(got, base, bnd)
        # the entries where the two models differ by more than the floor: hidden_1 .. hidden_N and the pruning logits
        closer = {n: (per[n][1], vs_base[n][1]) for n in per if n.startswith("hidden") and not bnd[n].at_floor or n == "prune"}
        line += f" | own / base model rms at {deepest}: {closer[deepest][0]:.2e} / {closer[deepest][1]:.2e}"
    TABLE.append(line)
    print("[conformance]", line)
    first = am.first_over(per)
    if first is not None:
        b = bnd[first]
        layer = first.split("_")[1] if first.startswith("hidden") else first
        pytest.fail(f"{label}: first entry over its bound is {first} (layer {layer}): rms {per[first][1]:.3e} (bound {b.rms:.3e}) "
                    f"max {per[first][2]:.3e} (bound {b.max:.3e})")
    if closer is not None:
        worse = [n for n, (own_rms, base_rms) in closer.items() if not own_rms < base_rms]
        assert not worse, f"{label}: as close to the base set's model as to its own at {worse}: {[closer[n] for n in worse]}"


def _check(model, kernel_set, flag_names, recipe, window, lengths=tuple(LENGTHS), damped=False):
    weights = weights_for(kernel_set, recipe, damped)
    rows = _rows(lengths)
    own = _model(model, weights, window, lengths, kernel_set)
    exact = _model(model, weights, window, lengths, "exact")
    base_set = am.BASE_SET.get(kernel_set)
    base = _model(model, weights, window, lengths, base_set) if base_set else None
    enc = _encoder(model, weights, window, kernel_set, _flag_bits(flag_names))
    try:
        got = _run(enc, rows)
        after = enc.effective_policy()["kernel_set"]
    finally:
        enc.close()
    rows_label = "L2048" if max(lengths) == 2048 else "list"
    label = f"{model:9s} {kernel_set:24s} {'+'.join(flag_names) or '-':18s} {weights:14s} w{window:<5d} {rows_label:5s}"
    assert after == kernel_set, f"{label}: the forward ran on {after}"
    _compare(label, got, own, exact, f"hidden_{SHAPES[model][3]}", base)


# -- which sets each path has -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model,flag", [(m, None) for m in MODELS] + [k for k in SUPPORTED_WITH_FLAG])
def test_supported_sets_are_exactly_the_expected_ones(model, flag):
    from open_provence_amd import _lib
    from open_provence_amd._lib import HipLibraryError
    from open_provence_amd.engine import HipEncoder

    expected = SUPPORTED[model] if flag is None else SUPPORTED_WITH_FLAG[(model, flag)]
    enc = HipEncoder(_dims(model), device="cuda:0", flags=_flag_bits([flag] if flag else []))
    try:
        enc.load_state_dict(_state(model, "o1"), calibrate=False)
        for name in ALL_SETS:
            if name in expected:
                enc.select_kernel_set(name)
                policy = enc.effective_policy()
                assert policy["kernel_set"] == name
                assert tuple(policy["terms"][f] for f in _lib.OP_FAMILIES) == SET_TERMS[name], (name, policy["terms"])
            else:
                with pytest.raises(HipLibraryError):
                    enc.select_kernel_set(name)
    finally:
        enc.close()


# -- every supported set, default flags, O(1) and peaked weights --------------------------------------------------------------
DEFAULT_CASES = [(m, s, w) for m in MODELS for s in SUPPORTED[m] for w in (("o1", "peaked") if m in ("row", "panel512") else ("o1",))]


@pytest.mark.parametrize("model,kernel_set,recipe", DEFAULT_CASES)
def test_kernel_set_matches_its_model(model, kernel_set, recipe):
    _check(model, kernel_set, [], recipe, 128)


# -- the MLP-isolating recipe: the correction terms of the MLP of sets 8 - 11 (and of 3 / 4, whose launches they reuse) -------
@pytest.mark.parametrize("model", DAMPED_MODELS)
@pytest.mark.parametrize("weights", ["o1-damped", "o1-bf16-damped"])
def test_damped_weights_keep_every_expected_set(model, weights):
    """The damped output projection sits on fp16's grid, so no set with an fp16 weight plane is refused for it
    (f16_unfit in op_plan.h): every set the model supports still pins."""

    from open_provence_amd.engine import HipEncoder

    enc = HipEncoder(_dims(model), device="cuda:0", flags=0)
    try:
        enc.load_state_dict(_state(model, weights), calibrate=False)
        for name in SUPPORTED[model]:
            enc.select_kernel_set(name)
            assert enc.effective_policy()["kernel_set"] == name
    finally:
        enc.close()


@pytest.mark.parametrize("model", DAMPED_MODELS)
@pytest.mark.parametrize("kernel_set", DAMPED_SETS)
def test_kernel_set_matches_its_model_on_mlp_isolating_weights(model, kernel_set):
    """With every attn.Wo x 2^-8 the attention side's error shrinks 256-fold and the MLP's arithmetic dominates each entry:
    a dropped lo term or a mis-scaled e4m3 plane in the Wi GEMM or the MLP output projection of sets 8 - 11 is 5 - 18 x
    the bound here (tests/test_arith_model.py), and under it on the plain weights."""

    _check(model, kernel_set, [], "o1", 128, damped=True)


@pytest.mark.parametrize("model,kernel_set", [("row", "bf16x3"), ("row", "f16"), ("row", "f16-f8-w")])
def test_a_2048_token_row(model, kernel_set):
    _check(model, kernel_set, [], "peaked", 128, lengths=tuple(LONG_LENGTHS))


# -- the test-hook flags, under the sets they change ---------------------------------------------------------------------------
FLAG_CASES = [(m, f, s) for (m, f), sets in FLAG_RUNS.items() for s in sets]


@pytest.mark.parametrize("model,flag,kernel_set", FLAG_CASES)
def test_flag_regime_matches_the_model(model, flag, kernel_set):
    _check(model, kernel_set, [flag], "o1", 128)


# -- windows on the three attention families -----------------------------------------------------------------------------------
@pytest.mark.parametrize("window", WINDOWS)
@pytest.mark.parametrize("model,kernel_set", WINDOW_RUNS)
def test_window_matches_the_model(model, kernel_set, window):
    assert window in ACCEPTED_WINDOWS  # (op_create raises below if the library refuses it)
    _check(model, kernel_set, [], "peaked", window)


@pytest.mark.parametrize("window", REFUSED_WINDOWS)
def test_refused_window_is_refused_at_create(window):
    from open_provence_amd._lib import HipLibraryError
    from open_provence_amd.engine import HipEncoder

    with pytest.raises(HipLibraryError, match="op_create"):
        HipEncoder(_dims("row", window), device="cuda:0", flags=0).close()


# -- a row-path batch above 256 blocks of 128 rows ------------------------------------------------------------------------------
def test_large_row_batch_sample():
    n_rows, length = 300, 128  # 38 400 tokens: 300 blocks of 128 rows
    rows = _rows([length] * n_rows, seed=11)
    sample = list(range(0, n_rows, n_rows // 16))[:16]
    enc = _encoder("row", "o1", 128, "f16", 0)
    try:
        got_all = _run(enc, rows)
        assert enc.effective_policy()["kernel_set"] == "f16"
    finally:
        enc.close()
    dims = _dims("row")
    srows = [rows[i] for i in sample]
    own = am.model_entries(am.forward(_state("row", "o1"), dims, srows, "f16", path="row"))
    exact = am.model_entries(am.forward(_state("row", "o1"), dims, srows, "exact", path="row"))
    idx = torch.cat([torch.arange(i * length, (i + 1) * length) for i in sample])
    got = {k: (v[idx] if k != "rank" else v[sample]) for k, v in got_all.items()}
    _compare(f"{'row':9s} {'f16':24s} {'-':18s} {'o1':14s} w128   300x128 (16 rows compared)", got, own, exact, "hidden_3")
