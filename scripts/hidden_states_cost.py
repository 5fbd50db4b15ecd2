#!/usr/bin/env python
"""Price of the per-call hidden-state request (HipEncoder.forward_packed(hidden=...)): 256 x 512 forwards of xsmall (kernel sets
"f16" and "f16-f8-w") and base, each event-timed on one stream -- without a request, with every entry in fp32, with every entry in
bf16, and through the debug hook engine.capture_hidden() (which switches the fused kernels off).  Usage:
hidden_states_cost.py [--steps K] [--warmup W]"""

from __future__ import annotations

import argparse
import json
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

from open_provence_amd.engine import HiddenRequest, HipEncoder  # noqa: E402
from open_provence_amd.packing import pack_rows  # noqa: E402
from open_provence_amd.synthetic import named_dims, refinit_state_dict, synth_pair_batch  # noqa: E402


def timed(fn, steps: int, warmup: int) -> float:
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(steps):
        fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) / steps


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    results = []
    for model, kernel_set in (("xsmall", "f16"), ("xsmall", "f16-f8-w"), ("base", None)):
        dims = named_dims(model, vocab_size=4096)
        enc = HipEncoder(dims, device="cuda:0")
        enc.load_state_dict(refinit_state_dict(dims, seed=7), calibrate=False, kernel_set=kernel_set)
        rows = synth_pair_batch(dims, 256, [512] * 256, seed=1)
        ids_np, cu_np, max_len = pack_rows(rows)
        ids = torch.from_numpy(ids_np).cuda()
        cu = torch.from_numpy(cu_np).cuda()

        def fwd(hidden=None):
            return lambda: enc.forward_packed(ids, cu, cu_np, max_len, hidden=hidden)

        row = {"model": model, "kernel_set": enc.effective_policy()["kernel_set"], "tokens": int(cu_np[-1])}
        row["plain_ms"] = timed(fwd(), args.steps, args.warmup)
        row["all_fp32_ms"] = timed(fwd(HiddenRequest()), args.steps, args.warmup)
        row["all_bf16_ms"] = timed(fwd(HiddenRequest(dtype=torch.bfloat16)), args.steps, args.warmup)
        with enc.capture_hidden():
            row["debug_capture_ms"] = timed(fwd(), args.steps, args.warmup)
        row["fp32_over_plain"] = row["all_fp32_ms"] / row["plain_ms"]
        row["bf16_over_plain"] = row["all_bf16_ms"] / row["plain_ms"]
        row["extra_store_gb_fp32"] = (dims.num_layers + 1) * row["tokens"] * dims.hidden_size * 4 / 1e9
        enc.close()
        results.append(row)
        print(f"{model:7s} {row['kernel_set']:10s} plain {row['plain_ms']:.3f} ms | all fp32 {row['all_fp32_ms']:.3f} ms "
              f"(x{row['fp32_over_plain']:.3f}) | all bf16 {row['all_bf16_ms']:.3f} ms (x{row['bf16_over_plain']:.3f}) | "
              f"debug capture {row['debug_capture_ms']:.3f} ms | {row['extra_store_gb_fp32']:.2f} GB of fp32 states", flush=True)
        torch.cuda.empty_cache()
    print(json.dumps({"device": torch.cuda.get_device_name(0), "steps": args.steps, "results": results}))


if __name__ == "__main__":
    main()
