"""The configuration ``bench.py`` TIMES, checked against the oracle (GPU).

``bench.py`` (BASELINE.json configs[1]): xsmall dims, 256 pairs x 512 tokens, synthetic weights of seed 7 -- by default
rounded to bf16 (a bf16 checkpoint), or kept fp32 (``--weights fp32``) -- default flags, no hidden-state capture, the
batch either as ONE launch sequence (``forward_packed``) or as TWO half-batch sequences on CU-partitioned streams
(``forward_packed_on``).  At that size every launch runs its large-batch form (128-row blocks; the layer-0 q / k / v
kernel gathers the embeddings itself over 1024 blocks; the last whole-layer launch carries final_norm + the pruning
head), which the small fixtures of the other parity tests never reach.  Here exactly that path runs and spread pairs --
the first and the last pair of each half included -- are compared with ``oracle_forward`` on the same weights.

Tolerance of the path (north_star): 1e-3 on pruning and ranking logits against the CPU reference arithmetic
(reference forward: standalone.py:1686-1719 + HF modeling_modernbert.py:434-652, restated in oracle/modernbert_oracle.py).
"""

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

PAIRS, SEQ_LEN = 256, 512
CHECKED = list(range(PAIRS))  # EVERY pair of the timed batch (the oracle takes ~10 s for 256 x 512 on the box's 16 cores):
# the maximum over 256 rows sits 1.3-1.4 x above what ten spot-checked pairs show (profiles/r04_error_tail.txt)


def _bench_setup(weights: str):
    from open_provence_amd.engine import HipEncoder
    from open_provence_amd.synthetic import named_dims, synth_pair_batch, synth_state_dict

    dims = named_dims("xsmall")
    state = synth_state_dict(dims, seed=7)
    if weights == "bf16":  # exactly bench.py's rounding of the GEMM weights
        state = {k: (v.to(torch.bfloat16).to(torch.float32) if v.ndim == 2 and "embeddings" not in k else v) for k, v in state.items()}
    rows = synth_pair_batch(dims, PAIRS, SEQ_LEN, seed=1234)
    enc = HipEncoder(dims, device="cuda:0", precision="bf16x3", flags=0)  # default flags, as the driver's bench run
    enc.load_state_dict(state)
    return dims, state, rows, enc


def _oracle(tag, state, dims, rows):
    from oracle_cache import oracle_rows  # the stored oracle outputs of this workload, or the oracle itself (tests/oracle_cache.py)

    return oracle_rows(tag, state, dims, rows)


@pytest.mark.parametrize("weights,kernel_set", [("bf16", "f16-f8"), ("fp32", "f16-f8-w")])
def test_bench_configuration_matches_the_oracle(weights, kernel_set):
    from open_provence_amd.packing import pack_rows

    dims, state, rows, enc = _bench_setup(weights)
    assert enc.effective_policy()["kernel_set"] == kernel_set
    dev = enc.device

    # one launch sequence over the whole batch (bench.py: one_pipeline / every rank of a multi-GPU run)
    ids_np, cu_np, max_len = pack_rows(rows)
    ids, cu = torch.from_numpy(ids_np).to(dev), torch.from_numpy(cu_np).to(dev)
    enc.profile_enable(True)
    prune1, rank1 = enc.forward_packed(ids, cu, cu_np, max_len)
    torch.cuda.synchronize()
    kinds = set(enc.profile_read())
    enc.profile_enable(False)
    # the launches bench.py times: no embedding / final-norm launches, the large-batch q / k / v kernel with the gather
    assert "embed_ln" not in kinds and "rowgemm_ln_qkv_rope" in kinds, kinds
    assert "fused_layer_attnout_mlp_qkv" in kinds and "final_ln_prune" not in kinds, kinds  # one launch per layer, either dtype
    prune1, rank1 = prune1.cpu().numpy().reshape(PAIRS, SEQ_LEN, 2), rank1.cpu().numpy()

    # two half-batch launch sequences on CU-partitioned streams (bench.py --pipelines 2; the default with OPEN_PROVENCE_NO_F8=1)
    half = PAIRS // 2
    outs = []
    for part, part_rows in enumerate((rows[:half], rows[half:])):
        p_ids_np, p_cu_np, p_max = pack_rows(part_rows)
        p_ids, p_cu = torch.from_numpy(p_ids_np).to(dev), torch.from_numpy(p_cu_np).to(dev)
        torch.cuda.synchronize()
        outs.append(enc.forward_packed_on(part, p_ids, p_cu, p_cu_np, p_max))
    for part in range(2):
        enc.pipeline_stream(part).synchronize()
    prune2 = np.concatenate([o[0].cpu().numpy() for o in outs]).reshape(PAIRS, SEQ_LEN, 2)
    rank2 = np.concatenate([o[1].cpu().numpy() for o in outs])
    enc.close()

    assert np.isfinite(prune1).all() and np.isfinite(rank1).all()
    # a pair's outputs do not depend on its batch companions, the chunking or the CUs that ran it: bit for bit
    assert np.array_equal(prune1, prune2) and np.array_equal(rank1, rank2)

    ref_prune, ref_rank = _oracle(f"timed_xsmall_o1_{weights}_256x512", state, dims, [rows[i] for i in CHECKED])
    got_prune, got_rank = prune1[CHECKED], rank1[CHECKED]
    # bar of the path: 1e-3; regression bound of THIS configuration: 8e-4 (measured over all 256 pairs: 6.5e-4 fp32-valued,
    # 4.9e-4 bf16-valued)
    assert np.abs(got_prune - ref_prune).max() < 8e-4, float(np.abs(got_prune - ref_prune).max())
    assert np.abs(got_rank - ref_rank).max() < 8e-4, float(np.abs(got_rank - ref_rank).max())
    # the decision quantity of process(): keep-probabilities (standalone.py:2918-2924)
    keep = 1.0 / (1.0 + np.exp(-(got_prune[..., 1] - got_prune[..., 0]).astype(np.float64)))
    keep_ref = 1.0 / (1.0 + np.exp(-(ref_prune[..., 1] - ref_prune[..., 0]).astype(np.float64)))
    assert np.abs(keep - keep_ref).max() < 1e-3


# ---- the panel path (hidden 512 / 768: BASELINE configs 3-5) at the sizes bench.py times it ------------------------------
# Full depth, default flags, both checkpoint dtypes.  At >= 256 row blocks the XCD-aware block maps of the panel GEMMs
# (op_forward_layers.hip: per_xcd / groups / row_group all follow r_pad / 128), the XCD-grouped attention map and the 256-query
# attention blocks take the values they have in the bench -- none of which the 1..7-row-block fixtures reach.  Checked
# pairs: first / last of the batch and pairs whose 4 row blocks sit at the boundaries of the 8-row-block XCD groups.

def _panel_setup(model: str, weights: str):
    from open_provence_amd.engine import HipEncoder
    from open_provence_amd.synthetic import named_dims, synth_state_dict

    dims = named_dims(model)
    state = synth_state_dict(dims, seed=7)
    if weights == "bf16":
        state = {k: (v.to(torch.bfloat16).to(torch.float32) if v.ndim == 2 and "embeddings" not in k else v) for k, v in state.items()}
    enc = HipEncoder(dims, device="cuda:0", precision="bf16x3", flags=0)
    enc.load_state_dict(state)
    return dims, state, enc


def _run_and_check(tag, enc, dims, state, rows, checked, expect_kinds):
    from open_provence_amd.packing import pack_rows

    ids_np, cu_np, max_len = pack_rows(rows)
    ids, cu = torch.from_numpy(ids_np).to(enc.device), torch.from_numpy(cu_np).to(enc.device)
    enc.profile_enable(True)
    prune, rank = enc.forward_packed(ids, cu, cu_np, max_len)
    torch.cuda.synchronize()
    kinds = set(enc.profile_read())
    enc.profile_enable(False)
    assert expect_kinds <= kinds, kinds
    prune, rank = prune.cpu().numpy(), rank.cpu().numpy()
    assert np.isfinite(prune).all() and np.isfinite(rank).all()
    ref_prune, ref_rank = _oracle(tag, state, dims, [rows[i] for i in checked])
    worst = 0.0
    for j, i in enumerate(checked):
        n = len(rows[i])
        got = prune[cu_np[i] : cu_np[i + 1]]
        worst = max(worst, float(np.abs(got - ref_prune[j, :n]).max()), float(np.abs(rank[i] - ref_rank[j]).max()))
    return worst


PANEL_KINDS = {"gemm_qkv_rope", "gemm_attn_out", "gemm_wi_geglu", "gemm_mlp_out", "layer_norm", "attn_global", "attn_local"}


@pytest.mark.parametrize("weights,kernel_set", [("fp32", "bf16x3+wi-f16-f8-w"), ("bf16", "bf16-weights")])
def test_base_model_at_bench_size_matches_the_oracle(weights, kernel_set):
    """bench.py's `base_model` sub-record and `--model base`: base dims (H = 512, 19 layers), 256 x 512 = 1024 row blocks."""

    from open_provence_amd.synthetic import synth_pair_batch

    dims, state, enc = _panel_setup("base", weights)
    assert enc.effective_policy()["kernel_set"] == kernel_set
    rows = synth_pair_batch(dims, PAIRS, SEQ_LEN, seed=1234)
    # pairs 1 / 2 and 15 / 16 straddle XCD-group boundaries (8 row blocks = 2 pairs per group, 8 groups per round)
    worst = _run_and_check(f"timed_base_o1_{weights}_256x512_spots", enc, dims, state, rows, [0, 1, 2, 15, 16, 127, 128, 200, 254, 255], PANEL_KINDS)
    enc.close()
    assert worst < 8e-4, worst  # (bar of the path: 1e-3; these configurations measure 2e-4 .. 5e-4)


@pytest.mark.parametrize("weights", ["fp32", "bf16"])
def test_en_gte_varlen_at_bench_size_matches_the_oracle(weights):
    """`bench.py --model en-gte --varlen` (BASELINE config 5): mixed lengths 128..2048, ~131 072 tokens, 22 layers."""

    from open_provence_amd.synthetic import synth_pair_batch, synth_varlen_lengths

    dims, state, enc = _panel_setup("en-gte", weights)
    lengths = synth_varlen_lengths(PAIRS * SEQ_LEN, seed=1234)
    rows = [synth_pair_batch(dims, 1, n, seed=1234 + 7 * i)[0] for i, n in enumerate(lengths)]
    assert sum(lengths) >= PAIRS * SEQ_LEN
    # first, last, the longest and the shortest row, and two in the middle
    order = sorted(range(len(rows)), key=lambda i: len(rows[i]))
    checked = sorted({0, len(rows) - 1, order[0], order[-1], len(rows) // 3, 2 * len(rows) // 3})
    worst = _run_and_check(f"timed_gte_o1_{weights}_varlen_spots", enc, dims, state, rows, checked, PANEL_KINDS)
    enc.close()
    assert worst < 8e-4, worst  # (bar of the path: 1e-3; these configurations measure 2e-4 .. 5e-4)


@pytest.mark.parametrize("weights", ["fp32", "bf16"])
def test_large_model_at_2048_matches_the_oracle(weights):
    """`bench.py --model large --seq-len 2048 --pairs 64` (BASELINE config 4): 25 layers, 64 x 2048 = 1024 row blocks; both
    checkpoint dtypes (tests/golden/bench_checksums.json stores `large|64x2048|bf16` too).  Pairs: first / last and the ones
    on either side of the XCD-group boundaries (a pair = 16 row blocks = two groups of 8)."""

    from open_provence_amd.synthetic import synth_pair_batch

    dims, state, enc = _panel_setup("large", weights)
    rows = synth_pair_batch(dims, 64, 2048, seed=1234)
    worst = _run_and_check(f"timed_large_o1_{weights}_64x2048_spots", enc, dims, state, rows, [0, 1, 31, 32, 62, 63], PANEL_KINDS)
    enc.close()
    assert worst < 8e-4, worst  # (bar of the path: 1e-3; these configurations measure 2e-4 .. 5e-4)


@pytest.mark.parametrize("init,weights,kernel_set", [("o1", "fp32", "f16-f8-w"), ("o1", "bf16", "f16-f8"), ("refinit", "fp32", "f16")])
def test_xsmall_at_2048_matches_the_oracle_on_every_pair(init, weights, kernel_set):
    """bench.py's `seq_len_2048` sub-record (north_star names seq_len 2048): xsmall dims, 64 pairs x 2048 tokens -- the
    256-query attention blocks over 32 key tiles, rotary positions up to 2047 -- on the O(1) weights of `--init o1` (both
    checkpoint dtypes; `xsmall|64x2048|*` in tests/golden/bench_checksums.json) and on the reference-initialised headline
    weights with the calibrated kernel set.  All 64 pairs."""

    from open_provence_amd.engine import HipEncoder
    from open_provence_amd.synthetic import named_dims, refinit_state_dict, synth_pair_batch, synth_state_dict

    dims = named_dims("xsmall")
    state = (refinit_state_dict if init == "refinit" else synth_state_dict)(dims, seed=7)
    if weights == "bf16":
        state = {k: (v.to(torch.bfloat16).to(torch.float32) if v.ndim == 2 and "embeddings" not in k else v) for k, v in state.items()}
    enc = HipEncoder(dims, device="cuda:0", precision="bf16x3", flags=0)
    enc.load_state_dict(state)
    assert enc.effective_policy()["kernel_set"] == kernel_set, enc.calibration
    rows = synth_pair_batch(dims, 64, 2048, seed=1234)
    worst = _run_and_check(f"timed_xsmall_{init}_{weights}_64x2048", enc, dims, state, rows, list(range(64)), {"fused_layer_attnout_mlp_qkv", "attn_global", "attn_local"})
    enc.close()
    assert worst < (3e-4 if init == "refinit" else 8e-4), worst
