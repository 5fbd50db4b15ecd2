"""Kernel set "fp32" (12): every contraction on the fp32-input MFMA, checked against the CPU oracle.

The bound of every comparison.  For a (weights, batch) pair and a quantity (the logits -- pruning logits at real tokens and
ranking logits --, the keep probabilities, one hidden state) let ``e_ref`` be the maximum difference between the oracle in
fp32 and the oracle in fp64: the reference's own rounding error.  The set must be within

    max(4 x e_ref, 16 ulp of the largest magnitude of the quantity)

of the FP64 oracle.  The factor 4 is the room for a sequential k-ordered fmaf chain against the CPU's blocked sums (two CPU
fp32 evaluations, eager and SDPA attention, differ by 1.4 x already); the ulp floor covers quantities the reference computes
almost exactly (the embedding LayerNorm).  A hidden state asked for in bf16 is the fp32 state rounded to nearest even: 2^-8
relative (half an ulp of 8 significant bits) on top.  The trained-like proxy is held to 4 x e_ref alone.  Each test prints ``err / e_ref`` per case.

The oracle is evaluated at run time, once per (weights, batch), and shared.

What the module does not do.  The small models are 8 of the 64 combinations of the parameter table (SMALL: every value, and
every pair named there, at least once).  Under ``prune_pre_final_norm`` hidden entry N is the raw last layer, which the oracle
does not hand out: the fp32 entry is taken through ``final_norm`` in fp64 on the host and compared with the oracle's
normalised entry; the bf16 request's entry N is checked there only through the logits, which are linear in it."""

from __future__ import annotations

import functools

import numpy as np
import pytest
import torch

import workspace_utils as wu
from helpers import CharTokenizer, dims_from_meta, load_golden, period_splitter, rows_from_fixture, state_from_fixture

pytestmark = pytest.mark.gpu

RAGGED = [1, 2, 8, 9, 15, 16, 17, 63, 64, 65, 127, 128, 129, 130, 200]
BATCHES = {
    "ragged": RAGGED,
    "total128": [100, 28],       # exactly one 128-row tile of tokens
    "total256": [129, 127],      # exactly two
    "total210": [77, 130, 3],    # no multiple of 128
}
F32_REGIONS = ["ln_f", "q_f", "k_f", "v_f", "o_f", "h_f"]


# -- models --------------------------------------------------------------------------------------------------------------------
def _small_dims(hidden, heads, pattern, window, pooling, labels, max_positions=2048):
    from open_provence_amd.config import EncoderDims

    cfg = dict(model_type="modernbert", vocab_size=512, hidden_size=hidden, intermediate_size=192, num_hidden_layers=3,
               num_attention_heads=heads, local_attention=window, global_attn_every_n_layers=3, global_rope_theta=160000.0,
               local_rope_theta=10000.0, max_position_embeddings=max_positions, pad_token_id=0, cls_token_id=1, sep_token_id=2,
               layer_types=["full_attention" if t == "G" else "sliding_attention" for t in pattern], classifier_pooling=pooling)
    return EncoderDims.from_base_model_config(cfg, num_labels=labels)


# every value of every parameter of the issue's table, each pair of (hidden, pattern), (hidden, window), (pattern, window) and
# (head, pre-norm) at least once: (hidden, heads, pattern, window, pooling, labels, prune_pre_final_norm, weights)
SMALL = [
    (128, 2, "GLL", 16, "cls", 1, False, "refinit"),
    (128, 2, "LGL", 128, "mean", 2, True, "synth"),
    (128, 2, "GLL", 128, "mean", 2, False, "refinit"),
    (128, 2, "LGL", 16, "cls", 1, True, "synth"),
    (384, 6, "GLL", 128, "cls", 1, True, "synth"),
    (384, 6, "LGL", 16, "mean", 2, False, "refinit"),
    (384, 6, "GLL", 16, "mean", 2, True, "refinit"),
    (384, 6, "LGL", 128, "cls", 1, False, "synth"),
]


@functools.lru_cache(maxsize=None)
def _small_state(case):
    from open_provence_amd.synthetic import refinit_state_dict, synth_state_dict

    dims = _small_dims(*case[:6])
    return (refinit_state_dict if case[7] == "refinit" else synth_state_dict)(dims, 5)


def _rows(lengths, seed=7, vocab=512):
    rng = np.random.default_rng(seed)
    return [[1] + rng.integers(3, vocab, n - 1).tolist() for n in lengths]


def _encoder(dims, state, kernel_set="fp32", **kw):
    from open_provence_amd.engine import HipEncoder

    enc = HipEncoder(dims, device="cuda:0", kernel_set=kernel_set if kernel_set == "fp32" else None, **kw)
    try:
        enc.load_state_dict(state, calibrate=False, kernel_set=kernel_set)
        assert enc.effective_policy()["kernel_set"] == kernel_set
    except BaseException:
        enc.close()
        raise
    return enc


# -- the oracle, its own error, the bound ----------------------------------------------------------------------------------------
class Reference:
    """fp64 oracle entries of one batch and, per entry, the fp32 oracle's distance to them."""

    def __init__(self, state, dims, rows, pre_norm):
        from open_provence_amd.synthetic import pad_rows
        from oracle.modernbert_oracle import oracle_forward

        torch.set_num_threads(16)
        ids, mask = pad_rows(rows)
        real = mask.bool()
        self.lengths = [len(r) for r in rows]
        self.entries, self.e_ref = {}, {}
        outs = {}
        for dtype in (torch.float64, torch.float32):
            out = oracle_forward(state, dims, ids, mask, dtype=dtype, return_hidden=True, prune_pre_final_norm=pre_norm)
            ent = {"logits": torch.cat([out.pruning_logits[real].double().flatten(), out.ranking_logits.double().flatten()]),
                   "keep_prob": torch.softmax(out.pruning_logits[real].double(), dim=-1)[:, 1]}
            for i in range(len(out.hidden_states)):
                ent[f"hidden_{i}"] = out.hidden_states[i][real].double()
            outs[dtype] = ent
        self.entries = outs[torch.float64]
        # entry N is the pruning head's input: under prune_pre_final_norm the raw last layer -- _check normalises it first
        pre = "ranking_model." if any(k.startswith("ranking_model.") for k in state) else ""
        self.raw_last = f"hidden_{dims.num_layers}" if pre_norm else None
        self.final_norm, self.eps = state[pre + "model.final_norm.weight"].double(), float(dims.norm_eps)
        self.e_ref = {k: float((outs[torch.float32][k] - v).abs().max()) for k, v in self.entries.items()}

    def bound(self, name):
        top = float(self.entries[name].abs().max())
        return max(4.0 * self.e_ref[name], 16.0 * float(np.spacing(np.float32(top))))


def _forward(enc, rows, dtype=torch.float32, padded=False):
    """-> entries of one forward_packed with keep_prob and every hidden state (packed fp32, or padded in ``dtype``)."""

    from open_provence_amd.engine import HiddenRequest
    from open_provence_amd.packing import pack_rows

    ids_np, cu_np, max_len = pack_rows(rows)
    ids, cu = torch.from_numpy(ids_np).to(enc.device), torch.from_numpy(cu_np).to(enc.device)
    keep = torch.full((int(ids.numel()),), float("nan"), device=enc.device)
    req = HiddenRequest(dtype=dtype, pad_width=max_len if padded else 0)
    prune, rank, hidden = enc.forward_packed(ids, cu, cu_np, max_len, keep_prob=keep, hidden=req)
    torch.cuda.synchronize()
    hidden = hidden.cpu()
    if padded:
        real = torch.zeros(len(rows), max_len, dtype=torch.bool)
        for s, r in enumerate(rows):
            real[s, : len(r)] = True
        assert bool((hidden[:, ~real] == 0).all()), "padding positions of a padded hidden state are not zero"
        hidden = hidden[:, real]
    out = {"logits": torch.cat([prune.cpu().double().flatten(), rank.cpu().double().flatten()]), "keep_prob": keep.cpu().double()}
    for i in range(hidden.shape[0]):
        out[f"hidden_{i}"] = hidden[i].double()
    return out, (prune, rank, hidden, keep)


def _check(label, got, ref: Reference, *, bf16_hidden=False, only=None):
    """Assert every entry of ``ref`` within its bound; print err / e_ref.  -> the worst ratio err / bound."""

    worst = 0.0
    for name, want in ref.entries.items():
        if only is not None and name not in only:
            continue
        assert bool(torch.isfinite(got[name]).all()), f"{label}: {name} is not finite"
        mine = got[name]
        if name == ref.raw_last:
            if bf16_hidden:
                continue
            mean = mine.mean(dim=-1, keepdim=True)
            mine = (mine - mean) / torch.sqrt(((mine - mean) ** 2).mean(dim=-1, keepdim=True) + ref.eps) * ref.final_norm
        diff = (mine - want).abs()
        bound = torch.full_like(want, ref.bound(name))
        if bf16_hidden and name.startswith("hidden"):
            bound = bound + 2.0 ** -8 * (want.abs() + bound)
        err, e_ref = float(diff.max()), ref.e_ref[name]
        print(f"[fp32-set] {label:46s} {name:10s} err {err:.3e}  e_ref {e_ref:.3e}  err/e_ref {err / max(e_ref, 1e-30):7.2f}  bound {ref.bound(name):.3e}")
        ratio = float((diff / bound).max())
        assert ratio <= 1.0, f"{label}: {name} is {err:.3e} from the fp64 oracle, bound {ref.bound(name):.3e} (e_ref {e_ref:.3e})"
        worst = max(worst, ratio)
    return worst


# -- small models --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", SMALL, ids=lambda c: f"h{c[0]}-{c[2]}-w{c[3]}-{c[4]}{c[5]}-{'pre' if c[6] else 'post'}-{c[7]}")
def test_small_models_match_the_oracle_and_do_not_depend_on_chunking(case):
    dims, state, pre_norm = _small_dims(*case[:6]), _small_state(case), case[6]
    enc = _encoder(dims, state, prune_pre_final_norm=pre_norm)
    chunked = _encoder(dims, state, prune_pre_final_norm=pre_norm, chunk_rows=256)
    try:
        for name, lengths in BATCHES.items():
            rows = _rows(lengths)
            ref = Reference(state, dims, rows, pre_norm)
            got, raw = _forward(enc, rows)
            _check(f"{case[0]} {case[2]} w{case[3]} {name}", got, ref)
            got16, _ = _forward(enc, rows, dtype=torch.bfloat16, padded=True)
            _check(f"{case[0]} {case[2]} w{case[3]} {name} bf16 padded", got16, ref, bf16_hidden=True)
            assert torch.equal(got16["logits"], got["logits"]) and torch.equal(got16["keep_prob"], got["keep_prob"])
            _, raw_chunked = _forward(chunked, rows)
            assert all(torch.equal(a, b) for a, b in zip(raw, raw_chunked)), f"{name}: chunk_rows = 256 changes the bits"
    finally:
        enc.close()
        chunked.close()


@pytest.mark.parametrize("case", [SMALL[0], SMALL[5]], ids=["h128", "h384"])
def test_a_row_alone_equals_the_row_inside_the_ragged_batch(case):
    dims, state = _small_dims(*case[:6]), _small_state(case)
    enc = _encoder(dims, state, prune_pre_final_norm=case[6])
    try:
        rows = _rows(RAGGED)
        _, (prune, rank, hidden, keep) = _forward(enc, rows)
        cu = np.concatenate(([0], np.cumsum(RAGGED)))
        for s, row in enumerate(rows):
            _, (p1, r1, h1, k1) = _forward(enc, [row])
            a, b = int(cu[s]), int(cu[s + 1])
            assert torch.equal(p1, prune[a:b]) and torch.equal(r1, rank[s: s + 1]) and torch.equal(k1, keep[a:b]), f"row {s} ({len(row)} tokens)"
            assert torch.equal(h1, hidden[:, a:b]), f"row {s} ({len(row)} tokens): hidden states"
    finally:
        enc.close()


LONG_LENGTHS = [4097, 5]  # one token past 4096: 65 key tiles, RoPE table rows beyond 2048, the window far from the row's start


def test_a_4097_token_row_matches_the_oracle():
    """The set at length (no other row of this module exceeds 512 tokens): every entry within the module's bound of the fp64
    oracle, on a handle whose max_position_embeddings is 8192, one full-attention and two sliding-window layers."""

    case = SMALL[2]
    dims, state = _small_dims(*case[:6], max_positions=8192), _small_state(case)
    rows = _rows(LONG_LENGTHS)
    ref = Reference(state, dims, rows, case[6])
    enc = _encoder(dims, state, prune_pre_final_norm=case[6])
    try:
        got, _ = _forward(enc, rows)
        _check(f"{case[0]} {case[2]} w{case[3]} rows 4097+5", got, ref)
    finally:
        enc.close()


# -- golden fixtures -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["g0b_hd64_refinit", "g0c_hd64_synth", "g1_xsmall", "g1m_meanpool", "g12_prenorm_tf4", "g8_base_refinit"])
def test_golden_fixtures_match_the_oracle(name):
    """g1_xsmall is a row-path handle, g8_base_refinit a panel-path one, the others tiled or row: the set runs on all of them."""

    arrays, meta = load_golden(name)
    dims, state, rows = dims_from_meta(meta), state_from_fixture(arrays, meta), rows_from_fixture(arrays)
    pre_norm = bool(meta.get("prune_pre_final_norm", False))
    ref = Reference(state, dims, rows, pre_norm)
    enc = _encoder(dims, state, prune_pre_final_norm=pre_norm)
    try:
        got, _ = _forward(enc, rows)
        _check(name, got, ref)
    finally:
        enc.close()


# -- trained-like proxy --------------------------------------------------------------------------------------------------------------
PROXY_LENGTHS = [512, 511, 130, 129, 65, 64, 2, 1]


@functools.lru_cache(maxsize=None)
def _proxy(outlier_range):
    from open_provence_amd.synthetic import named_dims, trained_like_state_dict, zipf_token_rows

    dims = named_dims("xsmall")
    state = trained_like_state_dict(dims, 7, outlier_range=outlier_range)
    rows = [r[:n] for r, n in zip(zipf_token_rows(dims, 8, 512, 11), PROXY_LENGTHS)]
    return dims, state, rows, Reference(state, dims, rows, False)


@pytest.mark.parametrize("outlier_range", [(30.0, 100.0), (5.0, 20.0)], ids=["30-100x", "5-20x"])
def test_trained_like_proxy_within_four_times_the_reference_error(outlier_range):
    dims, state, rows, ref = _proxy(outlier_range)
    errs = {}
    for kernel_set in ("fp32", "bf16x3"):
        enc = _encoder(dims, state, kernel_set)
        try:
            got, _ = _forward(enc, rows)
        finally:
            enc.close()
        errs[kernel_set] = float((got["logits"] - ref.entries["logits"]).abs().max())
    e_ref = ref.e_ref["logits"]
    print(f"[fp32-set] proxy {outlier_range}: e_ref {e_ref:.3e}  fp32 err {errs['fp32']:.3e} (err/e_ref {errs['fp32'] / e_ref:.2f})  "
          f"bf16x3 err {errs['bf16x3']:.3e}")
    assert errs["fp32"] <= 4.0 * e_ref, (errs, e_ref)
    assert errs["fp32"] < 0.5 * errs["bf16x3"], errs


CALIBRATION_KEYS = {"tolerance", "reference_set", "default_set", "chosen_set", "candidates", "default_err", "rows", "tokens", "batch"}


def test_calibration_against_the_fp32_set_escalates_to_it_on_the_proxy():
    from open_provence_amd import _lib
    from open_provence_amd.engine import HipEncoder

    dims, state, rows, ref = _proxy((30.0, 100.0))
    enc = HipEncoder(dims, device="cuda:0", calibration_reference="fp32", audit="off")
    plain = HipEncoder(dims, device="cuda:0", audit="off")
    packs = HipEncoder(dims, device="cuda:0", audit="off", flags=_lib.OP_FLAG_F32_PACKS)  # the fp32 weights, not the reference
    try:
        enc.load_state_dict(state, calibrate=1e-4)
        assert enc.calibration["reference_set"] == "fp32" and enc.calibration["chosen_set"] == "fp32", enc.calibration
        assert enc.effective_policy()["kernel_set"] == "fp32"
        assert "fp32" not in enc.calibration["candidates"] and enc.calibration["default_err"] > 1e-3, enc.calibration
        got, _ = _forward(enc, rows)
        assert float((got["logits"] - ref.entries["logits"]).abs().max()) <= 4.0 * ref.e_ref["logits"]
        # without the argument: the report of a calibration against the (hi, lo) bf16 set, the keys it has always had
        plain.load_state_dict(state, calibrate=1e-4)
        cal = plain.calibration
        assert set(cal) <= CALIBRATION_KEYS | {"mlp_correction_layers", "mlp_correction_err"} and CALIBRATION_KEYS <= set(cal), sorted(cal)
        assert cal["reference_set"] == "bf16x3" and "fp32" not in cal["candidates"] and cal["chosen_set"] != "fp32", cal
        assert "bf16x3" not in cal["candidates"], cal  # (the reference is no candidate)
        # ... value for value what a handle that merely holds the fp32 weights reports: without the bit they change nothing
        packs.load_state_dict(state, calibrate=1e-4)
        assert packs.calibration == cal, (packs.calibration, cal)
        assert packs.effective_policy() == plain.effective_policy()
    finally:
        enc.close()
        plain.close()
        packs.close()


@pytest.mark.parametrize("mode", ["first", "running"])
def test_audits_run_on_the_fp32_reference_when_a_cheaper_set_is_kept(mode, monkeypatch):
    """A well-conditioned checkpoint keeps a set cheaper than the default; its audits then run the batch (first-batch audit) or
    a sub-batch (running audit) on kernel set "fp32", whose workspace is larger than the chosen set's."""

    from open_provence_amd.engine import HipEncoder
    from open_provence_amd.synthetic import named_dims, refinit_state_dict

    monkeypatch.delenv("OPEN_PROVENCE_AUDIT", raising=False)
    dims = named_dims("xsmall", vocab_size=2048, num_hidden_layers=4)
    enc = HipEncoder(dims, device="cuda:0", calibration_reference="fp32",
                     **({} if mode == "first" else {"audit": "running", "audit_tokens": 128}))
    try:
        enc.load_state_dict(refinit_state_dict(dims, 5), calibrate=1e-4)
        cal = enc.calibration
        chosen = cal["chosen_set"]
        assert cal["reference_set"] == "fp32" and chosen not in ("fp32", cal["default_set"]), cal
        rng = np.random.default_rng(3)
        first = [[1] + rng.integers(3, 1000, n - 1).tolist() for n in (70, 33, 5)]
        prune, rank, _ = enc.forward_rows(first)
        torch.cuda.synchronize()
        assert bool(torch.isfinite(prune).all()) and bool(torch.isfinite(rank).all())
        assert cal["audit"]["passed"] and cal["audit"]["tokens"] == 108 and cal["audit"]["max_abs_err"] <= cal["audit"]["bound"], cal
        assert enc.effective_policy()["kernel_set"] == chosen
        if mode == "running":
            later = [[1] + rng.integers(1000, 2000, n - 1).tolist() for n in (90, 64, 40, 7)]  # ids no audited row held
            prune, rank, _ = enc.forward_rows(later)
            torch.cuda.synchronize()
            audits = cal["audits"]
            assert audits["count"] == 2 and audits["last"]["trigger"] == "coverage" and audits["last"]["passed"], audits
            assert 0 < audits["last"]["tokens"] <= 201 and len(audits["last"]["rows"]) >= 1, audits
            assert bool(torch.isfinite(prune).all()) and enc.effective_policy()["kernel_set"] == chosen
    finally:
        enc.close()


# -- workspace -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [SMALL[1], SMALL[4]], ids=["h128", "h384"])
def test_outputs_do_not_depend_on_what_the_workspace_held(case):
    dims, state = _small_dims(*case[:6]), _small_state(case)
    enc = _encoder(dims, state, prune_pre_final_norm=case[6])
    try:
        for lengths in (RAGGED, [33, 1], [130, 65], [129, 127]):
            rows = _rows(lengths)
            names = [r["name"] for r in enc.workspace_layout(len(rows), sum(lengths), max(lengths))]
            assert names[-len(F32_REGIONS):] == F32_REGIONS and len(set(names)) == len(names), names
            ref = wu.run(enc, rows, "zeros")
            assert [r["name"] for r in enc._controlled.layout] == names
            assert all(bool(torch.isfinite(t.float()).all()) for t in ref), f"{lengths}: non-finite on a zeroed workspace"
            for pattern in wu.POISONS:
                got = wu.run(enc, rows, pattern)
                assert wu.same(ref, got), (f"{lengths} on {pattern!r}: first difference at {wu.first_difference(ref, got, rows)}; "
                                           f"leaking regions: {wu.leaking_regions(enc, rows, pattern)}")
    finally:
        enc.close()


def test_layout_covers_the_workspace_and_only_the_fp32_set_has_the_fp32_planes():
    dims, state = _small_dims(*SMALL[0][:6]), _small_state(SMALL[0])
    enc = _encoder(dims, state)
    try:
        geometry = (15, sum(RAGGED), max(RAGGED))
        layout = enc.workspace_layout(*geometry)
        need = int(enc.lib.op_workspace_bytes(enc._handle, *geometry))
        end = 0
        for region in layout:
            assert region["offset"] == end and region["bytes"] > 0, region
            end = region["offset"] + (region["bytes"] + 255) // 256 * 256
        assert end == need
        enc.select_kernel_set("bf16x3")
        other = enc.workspace_layout(*geometry)
        assert other == layout[: -len(F32_REGIONS)] and not set(F32_REGIONS) & {r["name"] for r in other}
        assert int(enc.lib.op_workspace_bytes(enc._handle, *geometry)) < need
    finally:
        enc.close()


# -- selection without the create flag -------------------------------------------------------------------------------------------------
def test_a_handle_without_the_flag_refuses_the_set_and_keeps_its_own():
    from open_provence_amd import _lib
    from open_provence_amd.engine import HipEncoder

    dims, state = _small_dims(*SMALL[0][:6]), _small_state(SMALL[0])
    enc = HipEncoder(dims, device="cuda:0")
    try:
        enc.load_state_dict(state, calibrate=False)
        before_set = enc.effective_policy()["kernel_set"]
        rows = _rows(RAGGED)
        _, before = _forward(enc, rows)
        code = enc.lib.op_select_kernel_set(enc._handle, _lib.KERNEL_SET_IDS["fp32"])
        assert code == _lib.OP_ERR_UNSUPPORTED and "OP_FLAG_F32_PACKS" in _lib.last_error(enc.lib, enc._handle)
        with pytest.raises(_lib.HipLibraryError, match="OP_FLAG_F32_PACKS"):
            enc.select_kernel_set("fp32")
        assert enc.effective_policy()["kernel_set"] == before_set
        _, after = _forward(enc, rows)
        assert all(torch.equal(a, b) for a, b in zip(before, after))
    finally:
        enc.close()


# -- the public surfaces ---------------------------------------------------------------------------------------------------------------
def test_model_forward_and_process_run_on_the_set():
    from open_provence_amd.config import OpenProvenceConfig
    from open_provence_amd.modeling import OpenProvenceModel
    from open_provence_amd.synthetic import pad_rows

    arrays, meta = load_golden("g0c_hd64_synth")
    state = state_from_fixture(arrays, meta)
    cfg = OpenProvenceConfig(base_model_config=meta["base_model_config"], tokenizer_name_or_path="x",
                             pruning_config={"hidden_size": meta["base_model_config"]["hidden_size"]}, max_length=128)
    model = OpenProvenceModel(cfg, device="cuda", tokenizer=CharTokenizer(), state_dict=state, kernel_set="fp32")
    assert model.encoder.effective_policy()["kernel_set"] == "fp32"
    rows = rows_from_fixture(arrays)
    ref = Reference(state, dims_from_meta(meta), rows, False)
    ids, mask = pad_rows(rows)
    out = model(input_ids=ids.cuda(), attention_mask=mask.cuda())
    real = mask.bool()
    got = {"logits": torch.cat([out.pruning_logits.cpu()[real].double().flatten(), out.ranking_logits.cpu().double().flatten()])}
    _check("OpenProvenceModel.forward g0c", got, ref, only=("logits",))
    assert bool((out.pruning_logits.cpu()[~real] == 0).all())
    result = model.process(question="How tall is the tower?",
                           context="The tower is tall. It was built long ago! Many people visit it. Bread is made from flour.",
                           sentence_splitter=period_splitter, show_progress=False, return_sentence_metrics=True, threshold=0.5)
    assert np.isfinite(result["reranking_score"]) and result["pruned_context"] is not None
    assert result["performance_trace"].runtime["kernel_set"] == "fp32"
    assert model.encoder.effective_policy()["kernel_set"] == "fp32"
