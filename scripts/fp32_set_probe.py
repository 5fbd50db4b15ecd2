#!/usr/bin/env python
"""Kernel set "fp32" (12) on the GPU: how far it is from the fp64 CPU oracle, per fixture, in units of the fp32 oracle's own
distance to it (e_ref), beside kernel set 0 ("bf16x3"); and its throughput beside set 0's on the same box.

    timeout 900 python scripts/fp32_set_probe.py [--out profiles/fp32_set.txt] [--steps 6] [--parent-lib PATH]

``--parent-lib``: a build of the parent commit's library (the ABI is the same); set 0 is then timed on it too, in a child
process of its own (a process binds one library), on the same box.

One process, one GPU.  The bound the tests hold the set to is max(4 x e_ref, 16 ulp of the largest |logit|)
(tests/test_gpu_fp32_set.py); this script records the ratios."""

from __future__ import annotations

import argparse
import os
import subprocess
import sys
import time
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[1]
for p in (str(ROOT), str(ROOT / "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

from open_provence_amd.engine import HipEncoder  # noqa: E402
from open_provence_amd.packing import pack_rows  # noqa: E402
from open_provence_amd.synthetic import (named_dims, pad_rows, synth_pair_batch, synth_state_dict, trained_like_state_dict,  # noqa: E402
                                         zipf_token_rows)
from oracle.modernbert_oracle import oracle_forward  # noqa: E402

FIXTURES = ["g0b_hd64_refinit", "g0c_hd64_synth", "g1_xsmall", "g1m_meanpool", "g12_prenorm_tf4", "g8_base_refinit"]
PROXY_LENGTHS = [512, 511, 130, 129, 65, 64, 2, 1]


def logits_of(prune, rank):
    return torch.cat([prune.double().flatten(), rank.double().flatten()])


def oracle_logits(state, dims, rows, pre_norm, dtype):
    ids, mask = pad_rows(rows)
    out = oracle_forward(state, dims, ids, mask, dtype=dtype, prune_pre_final_norm=pre_norm)
    return logits_of(out.pruning_logits[mask.bool()], out.ranking_logits)


def gpu_logits(dims, state, rows, pre_norm, kernel_set):
    enc = HipEncoder(dims, device="cuda:0", prune_pre_final_norm=pre_norm, kernel_set="fp32" if kernel_set == "fp32" else None)
    try:
        enc.load_state_dict(state, calibrate=False, kernel_set=kernel_set)
        path = "row" if dims.hidden_size <= 256 else ("panel" if dims.hidden_size % 256 == 0 and dims.intermediate_size % 128 == 0 else "tiled")
        prune, rank, _ = enc.forward_rows(rows)
        torch.cuda.synchronize()
        return logits_of(prune.cpu(), rank.cpu()), path
    finally:
        enc.close()


def error_line(label, dims, state, rows, pre_norm):
    torch.set_num_threads(16)
    ref = oracle_logits(state, dims, rows, pre_norm, torch.float64)
    e_ref = float((oracle_logits(state, dims, rows, pre_norm, torch.float32) - ref).abs().max())
    got12, path = gpu_logits(dims, state, rows, pre_norm, "fp32")
    got0, _ = gpu_logits(dims, state, rows, pre_norm, "bf16x3")
    err12, err0 = float((got12 - ref).abs().max()), float((got0 - ref).abs().max())
    top = float(ref.abs().max())
    bound = max(4.0 * e_ref, 16.0 * float(np.spacing(np.float32(top))))
    return (f"{label:28s} {path:6s} e_ref {e_ref:.3e}  fp32 {err12:.3e} (err/e_ref {err12 / e_ref:6.2f}, err/bound {err12 / bound:5.2f})  "
            f"bf16x3 {err0:.3e} (err/e_ref {err0 / e_ref:8.2f})  max|logit| {top:.2f}")


def pairs_per_second(dims, state, rows, kernel_set, steps, warmup=2):
    enc = HipEncoder(dims, device="cuda:0", kernel_set="fp32" if kernel_set == "fp32" else None)
    try:
        enc.load_state_dict(state, calibrate=False, kernel_set=kernel_set)
        ids_np, cu_np, max_len = pack_rows(rows)
        ids, cu = torch.from_numpy(ids_np).to(enc.device), torch.from_numpy(cu_np).to(enc.device)
        for _ in range(warmup):
            enc.forward_packed(ids, cu, cu_np, max_len)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            enc.forward_packed(ids, cu, cu_np, max_len)
        torch.cuda.synchronize()
        return steps * len(rows) / (time.perf_counter() - t0)
    finally:
        enc.close()


def main() -> int:
    from helpers import dims_from_meta, load_golden, rows_from_fixture, state_from_fixture

    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "fp32_set.txt"))
    ap.add_argument("--steps", type=int, default=6)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--set0-rate-only", action="store_true", help=argparse.SUPPRESS)  # (the child process of --parent-lib)
    args = ap.parse_args()
    if args.set0_rate_only:
        dims = named_dims("xsmall")
        print("RATE0", pairs_per_second(dims, synth_state_dict(dims, 5), synth_pair_batch(dims, 256, 512, seed=9), "bf16x3", args.steps * 4))
        return 0
    lines = [f"kernel set \"fp32\" (12) against the fp64 CPU oracle -- {torch.cuda.get_device_name(0)}",
             "e_ref = max |fp32 oracle - fp64 oracle| over pruning logits at real tokens and ranking logits; errors are against the fp64 oracle",
             ""]
    for name in FIXTURES:
        arrays, meta = load_golden(name)
        lines.append(error_line(name, dims_from_meta(meta), state_from_fixture(arrays, meta), rows_from_fixture(arrays),
                                bool(meta.get("prune_pre_final_norm", False))))
        print(lines[-1], flush=True)
    dims = named_dims("xsmall")
    for outlier_range in ((30.0, 100.0), (5.0, 20.0)):
        state = trained_like_state_dict(dims, 7, outlier_range=outlier_range)
        rows = [r[:n] for r, n in zip(zipf_token_rows(dims, 8, 512, 11), PROXY_LENGTHS)]
        lines.append(error_line(f"trained-like {outlier_range[0]:g}-{outlier_range[1]:g}x", dims, state, rows, False))
        print(lines[-1], flush=True)
    state = synth_state_dict(dims, 5)
    rows = synth_pair_batch(dims, 256, 512, seed=9)
    rate0 = pairs_per_second(dims, state, rows, "bf16x3", args.steps * 4)
    rate12 = pairs_per_second(dims, state, rows, "fp32", args.steps)
    lines += ["", f"xsmall 256 x 512, one stream, forward_packed: set 0 (bf16x3) {rate0:9.1f} pairs/s   set 12 (fp32) {rate12:9.1f} pairs/s   "
                  f"ratio {rate12 / rate0:.3f}",
              ]
    if args.parent_lib:
        env = dict(os.environ, OPEN_PROVENCE_HIP_LIB=os.path.abspath(args.parent_lib))
        child = subprocess.run([sys.executable, __file__, "--set0-rate-only", "--steps", str(args.steps)], env=env, capture_output=True,
                               text=True, timeout=300)
        if child.returncode != 0:
            print(child.stdout[-2000:], child.stderr[-2000:])
            return child.returncode or 1
        parent0 = float([line for line in child.stdout.splitlines() if line.startswith("RATE0 ")][-1].split()[1])
        lines.append(f"the parent commit's library, same box, same batch: set 0 (bf16x3) {parent0:9.1f} pairs/s   this library / parent {rate0 / parent0:.4f}")
    else:
        lines.append("(no --parent-lib given: the parent commit's figure for set 0 was not measured)")
    print("\n".join(lines[-2:]), flush=True)
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
