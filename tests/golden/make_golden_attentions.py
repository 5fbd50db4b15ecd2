#!/usr/bin/env python
"""Generate the attention-probability fixtures (g13 / g14) by running the REAL reference under eager attention.

Build-container only, like make_golden.py (whose loader, model builder and config helper this imports).  The reference
returns ``attentions`` only under eager attention: ``model.ranking_model.set_attn_implementation("eager")``, then
``forward(..., output_attentions=True)`` -> num_layers tensors ``[B, heads, L, L]``.  Stored with the padded QUERY rows
zeroed (the reference holds a softmax row there; the HIP path returns zeros, as its hidden states do), every
``query_stride``-th query row, plus the ranking logits as a cross-check that the model is the one the seed describes.

``ref_to_fp64`` in the meta: per layer, max |reference - fp64 restatement from the oracle's fp64 hidden states|
(tests/attention_utils.py) -- the reference's own distance to exact arithmetic, the unit the tests' bounds are read in.

Usage:  python tests/golden/make_golden_attentions.py [--only NAME ...]
"""

from __future__ import annotations

import argparse
import json
from typing import Any

import numpy as np
import torch

from make_golden import HERE, base_cfg, build_model, load_reference, versions  # noqa: E402  (also puts the repo on sys.path)

from attention_utils import attention_probs  # noqa: E402
from open_provence_amd.synthetic import pad_rows  # noqa: E402
from oracle.modernbert_oracle import oracle_forward  # noqa: E402


def attention_rows(dims, lengths: list[int], seed: int):
    """[CLS] + uniform ids (+ [SEP] from two tokens on): rows down to ONE token, which synth_pair_batch cannot make."""

    rng = np.random.default_rng(seed)
    lo, hi = max(4, dims.vocab_size // 8), dims.vocab_size - max(4, dims.vocab_size // 8)
    rows = []
    for n in lengths:
        body = rng.integers(lo, hi, size=max(n - 2, 0)).tolist()
        rows.append(([dims.cls_token_id or 1] + body + [dims.sep_token_id or 2])[:n] if n > 1 else [dims.cls_token_id or 1])
    return pad_rows(rows, pad_id=dims.pad_token_id or 0)


def attention_fixture(name: str, cfg: dict[str, Any], lengths: list[int], *, weight_seed: int, query_stride: int, input_seed: int = 4321) -> None:
    ref = load_reference()
    model, dims = build_model(ref, cfg, max_length=max(lengths), seed=0, weight_seed=weight_seed)
    model.ranking_model.set_attn_implementation("eager")
    ids, mask = attention_rows(dims, lengths, input_seed)
    with torch.no_grad():
        out = model(input_ids=ids, attention_mask=mask, output_attentions=True)
    attentions = out.attentions
    assert len(attentions) == dims.num_layers, len(attentions)
    state = {k: v for k, v in model.state_dict().items() if "inv_freq" not in k}
    with torch.no_grad():
        exact = oracle_forward(state, dims, ids, mask, dtype=torch.float64, return_hidden=True)
    real = mask.bool()
    arrays: dict[str, np.ndarray] = {
        "input_ids": ids.numpy(),
        "attention_mask": mask.numpy(),
        "ranking_logits": out.ranking_logits.float().numpy(),
    }
    ref_to_fp64, row_max, zeros_identical = [], [], []
    for i, a in enumerate(attentions):
        a = a.float().clone()
        assert a.shape == (len(lengths), dims.num_heads, max(lengths), max(lengths)), a.shape
        a[~real[:, None, :].expand(-1, dims.num_heads, -1)] = 0.0  # padded query rows
        assert bool(torch.isfinite(a).all())
        with torch.no_grad():
            restated = attention_probs(state, dims, exact.hidden_states[i], mask, i)
        zeros_identical.append(bool(((a == 0) == (restated == 0)).all()))  # (False: an fp32 underflow among the visible keys)
        ref_to_fp64.append(float((a.double() - restated).abs().max()))
        row_max.append(float(a.max()))
        arrays[f"attn_{i}"] = a[:, :, ::query_stride, :].numpy()
    one = [b for b, n in enumerate(lengths) if n == 1]
    for b in one:
        assert all(float(arrays[f"attn_{i}"][b, :, 0, 0].min()) == 1.0 for i in range(dims.num_layers))
    meta = {
        "name": name,
        "base_model_config": cfg,
        "num_labels": 1,
        "lengths": lengths,
        "input_seed": input_seed,
        "weight_seed": weight_seed,
        "weight_init": "synth",
        "query_stride": query_stride,
        "n_attentions": len(attentions),
        "ref_to_fp64": ref_to_fp64,
        "max_probability": row_max,
        "zero_pattern_identical_to_fp64": zeros_identical,
        "attn_implementation": "eager",
        "layer_types": list(model.ranking_model.config.layer_types),
        "generator": "tests/golden/make_golden_attentions.py (reference OpenProvenceModel.forward, eager attention, output_attentions=True, CPU fp32)",
        "versions": versions(),
    }
    np.savez_compressed(HERE / f"{name}.npz", **arrays)
    (HERE / f"{name}.json").write_text(json.dumps(meta, indent=2, sort_keys=True))
    size = (HERE / f"{name}.npz").stat().st_size
    print(f"[golden] {name}: {size / 1e6:.2f} MB, ref_to_fp64 {['%.1e' % e for e in ref_to_fp64]}, max p {['%.3f' % p for p in row_max]}")


def main() -> None:
    parser = argparse.ArgumentParser()
    parser.add_argument("--only", nargs="*", default=None)
    args = parser.parse_args()

    def want(name: str) -> bool:
        return args.only is None or name in args.only

    # G13: g0c's config (head_dim 64, 2 heads, global / local / local / global, window +-8: it straddles a 64-key tile
    # edge); sequence ends on, before and after the tile edge, at non-multiples of 16, and at 1.
    if want("g13_attn_hd64"):
        attention_fixture(
            "g13_attn_hd64",
            base_cfg(vocab_size=256, hidden_size=128, intermediate_size=128, num_hidden_layers=4, num_attention_heads=2, local_attention=16),
            [128, 100, 65, 64, 33, 17, 1], weight_seed=11, query_stride=1,
        )
    # G14: g12's config (xsmall width, 4 heads, window +-64: it spans several tiles), width 200 (no multiple of 64).
    if want("g14_attn_h256"):
        attention_fixture(
            "g14_attn_h256",
            base_cfg(vocab_size=2048, hidden_size=256, intermediate_size=1024, num_hidden_layers=4, num_attention_heads=4),
            [200, 129, 64], weight_seed=61, query_stride=7,
        )


if __name__ == "__main__":
    main()
