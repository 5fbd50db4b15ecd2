#!/usr/bin/env python
"""What the padded boundary costs around the kernels: wall-clock time of one ``OpenProvenceModel.forward(input_ids,
attention_mask)`` on CUDA tensors (synchronised before and after; the median of the timed calls after a warm-up -- event time
would miss the host's share, which is the point), beside ``HipEncoder.forward_packed`` on the same batch already packed, timed
the same way.  Shapes: xsmall 256 x 512 and 32 x 128, base 64 x 512, all with ragged lengths.  Only the public ``forward()``
and ``forward_packed`` are used, so the same file measures any revision of the package.  Usage:
padded_forward_cost.py [--steps K] [--warmup W]"""

from __future__ import annotations

import argparse
import json
import statistics
import sys
import time
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

from open_provence_amd.config import OpenProvenceConfig  # noqa: E402
from open_provence_amd.modeling import OpenProvenceModel  # noqa: E402
from open_provence_amd.packing import pack_rows  # noqa: E402
from open_provence_amd.synthetic import named_dims, pad_rows, refinit_state_dict, synth_pair_batch  # noqa: E402
from helpers import CharTokenizer  # noqa: E402  (forward() never tokenizes; the model wants one to hold)


def wall_ms(fn, steps: int, warmup: int) -> dict:
    for _ in range(warmup):
        fn()
    samples = []
    for _ in range(steps):
        torch.cuda.synchronize()
        start = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        samples.append((time.perf_counter() - start) * 1e3)
    samples.sort()
    return {"median": statistics.median(samples), "min": samples[0], "p90": samples[int(0.9 * (len(samples) - 1))]}


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--label", default="")
    args = ap.parse_args()
    results = []
    for model_name, kernel_set, n_rows, width in (("xsmall", "f16", 256, 512), ("xsmall", "f16", 32, 128), ("base", None, 64, 512)):
        dims = named_dims(model_name, vocab_size=4096)
        cfg = OpenProvenceConfig(base_model_config=dims.to_base_model_config(), tokenizer_name_or_path="x",
                                 pruning_config={"hidden_size": dims.hidden_size}, max_length=width)
        model = OpenProvenceModel(cfg, device="cuda:0", tokenizer=CharTokenizer(), state_dict=refinit_state_dict(dims, seed=7),
                                  calibrate=False, kernel_set=kernel_set)
        rng = np.random.default_rng(n_rows * 1000 + width)
        lengths = rng.integers(width // 4, width + 1, size=n_rows).tolist()
        lengths[0] = width
        rows = synth_pair_batch(dims, n_rows, lengths, seed=1)
        ids_pad, mask_pad = pad_rows(rows, pad_id=3)
        ids_dev, mask_dev = ids_pad.cuda(), mask_pad.cuda()
        ids_np, cu_np, max_len = pack_rows(rows)
        ids_packed, cu_dev = torch.from_numpy(ids_np).cuda(), torch.from_numpy(cu_np).cuda()

        forward = wall_ms(lambda: model(input_ids=ids_dev, attention_mask=mask_dev), args.steps, args.warmup)
        packed = wall_ms(lambda: model.encoder.forward_packed(ids_packed, cu_dev, cu_np, max_len), args.steps, args.warmup)
        row = {"model": model_name, "kernel_set": model.encoder.effective_policy()["kernel_set"], "rows": n_rows, "width": width,
               "tokens": int(cu_np[-1]), "forward_ms": forward, "forward_packed_ms": packed,
               "gap_ms": forward["median"] - packed["median"]}
        results.append(row)
        print(f"{model_name:7s} {n_rows:4d} x {width:4d} ({row['tokens']:6d} tokens, {row['kernel_set']}): forward() {forward['median']:8.3f} ms "
              f"(min {forward['min']:.3f}, p90 {forward['p90']:.3f}) | forward_packed {packed['median']:8.3f} ms (min {packed['min']:.3f}, "
              f"p90 {packed['p90']:.3f}) | gap {row['gap_ms']:7.3f} ms", flush=True)
        model.encoder.close()
        del model
        torch.cuda.empty_cache()
    print(json.dumps({"label": args.label, "device": torch.cuda.get_device_name(0), "steps": args.steps, "warmup": args.warmup,
                      "results": results}))


if __name__ == "__main__":
    main()
