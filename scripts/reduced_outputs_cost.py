#!/usr/bin/env python
"""Price of the reduced outputs beside the full requests they replace (profiles/reduced_outputs_cost.txt): forwards of xsmall at
32 x 512 and 256 x 512 on kernel sets "f16" and "f16-f8-w" (--base: base at 32 x 512 too), event-timed on one stream, warm,
5 x 10 forwards per variant with the variants TAKING TURNS (one repeat of each, then the next repeat), median and min .. max:
  plain                       no request
  hidden_full                 every entry, packed fp32 (op_forward_packed_hidden)
  pooled_first / pooled_mean  every entry pooled (op_forward_packed_pooled)
  attn_full_1 / attn_full_all op_attention_probs behind the forward, one layer / every layer
  rows_1 / rows_all           op_attention_rows (query "first"), per head
  rows_mean_1 / rows_mean_all ... as the mean over heads
Usage: reduced_outputs_cost.py [--steps 10] [--repeats 5] [--base] [--only-new] (--only-new: the variants with new kernels
alone, a few steps: what a kernel trace of its own runs)"""

from __future__ import annotations

import argparse
import json
import statistics
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

from open_provence_amd.engine import AttentionRequest, HiddenRequest, HipEncoder  # noqa: E402
from open_provence_amd.packing import pack_rows  # noqa: E402
from open_provence_amd.synthetic import named_dims, refinit_state_dict, synth_pair_batch  # noqa: E402


def timed(fn, steps: int) -> float:
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(steps):
        fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) / steps


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--base", action="store_true")
    ap.add_argument("--only-new", action="store_true")
    args = ap.parse_args()
    cases = [("xsmall", s, pairs) for pairs in (32, 256) for s in ("f16", "f16-f8-w")] + ([("base", None, 32)] if args.base else [])
    results = []
    for model, kernel_set, pairs in cases:
        dims = named_dims(model, vocab_size=4096)
        enc = HipEncoder(dims, device="cuda:0", attention_outputs=True)
        enc.load_state_dict(refinit_state_dict(dims, seed=7), calibrate=False, kernel_set=kernel_set)
        ids_np, cu_np, max_len = pack_rows(synth_pair_batch(dims, pairs, [512] * pairs, seed=1))
        ids, cu = torch.from_numpy(ids_np).cuda(), torch.from_numpy(cu_np).cuda()
        every, one = None, [dims.num_layers // 2]

        def fwd(**requests):
            return lambda: enc.forward_packed(ids, cu, cu_np, max_len, **requests)

        variants = {
            "plain": fwd(),
            "hidden_full": fwd(hidden=HiddenRequest()),
            "pooled_first": fwd(hidden=HiddenRequest(pool="first")),
            "pooled_mean": fwd(hidden=HiddenRequest(pool="mean")),
            "attn_full_1": fwd(attentions=AttentionRequest(layers=one)),
            "attn_full_all": fwd(attentions=AttentionRequest(layers=every)),
            "rows_1": fwd(attentions=AttentionRequest(layers=one, query="first")),
            "rows_all": fwd(attentions=AttentionRequest(layers=every, query="first")),
            "rows_mean_1": fwd(attentions=AttentionRequest(layers=one, query="first", reduce_heads=True)),
            "rows_mean_all": fwd(attentions=AttentionRequest(layers=every, query="first", reduce_heads=True)),
        }
        if args.only_new:
            variants = {k: v for k, v in variants.items() if k.startswith(("pooled", "rows"))}
        for fn in variants.values():  # warm: allocations, workspaces
            fn()
            fn()
        torch.cuda.synchronize()
        times = {name: [] for name in variants}
        for _ in range(args.repeats):
            for name, fn in variants.items():
                times[name].append(timed(fn, args.steps))
        row = {"model": model, "kernel_set": enc.effective_policy()["kernel_set"], "pairs": pairs, "length": 512, "layers": dims.num_layers,
               "steps": args.steps, "repeats": args.repeats,
               "ms": {n: {"median": statistics.median(t), "min": min(t), "max": max(t)} for n, t in times.items()}}
        results.append(row)
        print(f"{model} {pairs} x 512 on {row['kernel_set']} ({dims.num_layers} layers)")
        for name, t in row["ms"].items():
            print(f"  {name:14s} {t['median']:9.3f} ms (min {t['min']:.3f} .. max {t['max']:.3f})", flush=True)
        enc.close()
        del variants, enc
        torch.cuda.empty_cache()
    print(json.dumps({"device": torch.cuda.get_device_name(0), "results": results}))


if __name__ == "__main__":
    main()
