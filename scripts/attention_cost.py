#!/usr/bin/env python
"""Price of forward_packed(attentions=...): xsmall at 32 x 512, every layer and one layer, beside a plain forward on the same
box -- each a warm, event-timed loop on one stream, repeated (median, min .. max) -- and the store rate of the side pass
(op_attention_probs: gather, LayerNorm, q | k projection and the probability kernel, whose stores are ~all of its bytes)
beside a hipMemsetAsync of the same bytes.  Usage: attention_cost.py [--steps K] [--warmup W] [--repeats R]"""

from __future__ import annotations

import argparse
import ctypes
import json
import statistics
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

from open_provence_amd.engine import AttentionRequest, HiddenRequest, HipEncoder  # noqa: E402
from open_provence_amd.packing import pack_rows  # noqa: E402
from open_provence_amd.synthetic import named_dims, refinit_state_dict, synth_pair_batch  # noqa: E402


def timed(fn, steps: int, warmup: int, repeats: int) -> dict:
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(repeats):
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        for _ in range(steps):
            fn()
        stop.record()
        stop.synchronize()
        ms.append(start.elapsed_time(stop) / steps)
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms)}


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--pairs", type=int, default=32)
    ap.add_argument("--length", type=int, default=512)
    args = ap.parse_args()
    dims = named_dims("xsmall", vocab_size=4096)
    enc = HipEncoder(dims, device="cuda:0", attention_outputs=True)
    enc.load_state_dict(refinit_state_dict(dims, seed=7), calibrate=False)
    rows = synth_pair_batch(dims, args.pairs, [args.length] * args.pairs, seed=1)
    ids_np, cu_np, max_len = pack_rows(rows)
    ids, cu = torch.from_numpy(ids_np).cuda(), torch.from_numpy(cu_np).cuda()
    t = lambda fn: timed(fn, args.steps, args.warmup, args.repeats)  # noqa: E731
    res = {"device": torch.cuda.get_device_name(0), "kernel_set": enc.effective_policy()["kernel_set"], "pairs": args.pairs,
           "length": args.length, "steps": args.steps, "repeats": args.repeats}
    res["plain"] = t(lambda: enc.forward_packed(ids, cu, cu_np, max_len))
    res["all_layers"] = t(lambda: enc.forward_packed(ids, cu, cu_np, max_len, attentions=AttentionRequest()))
    res["one_layer"] = t(lambda: enc.forward_packed(ids, cu, cu_np, max_len, attentions=AttentionRequest(layers=[5])))
    layer_bytes = args.pairs * dims.num_heads * max_len * max_len * 4
    res["bytes_per_layer"] = layer_bytes
    # the side pass alone, on a global and on a sliding-window layer, beside a fill of the same bytes
    _, _, states = enc.forward_packed(ids, cu, cu_np, max_len, hidden=HiddenRequest(layers=[0, 1]))
    for key, layer in (("pass_global", 0), ("pass_local", 1)):
        res[key] = t(lambda: enc.attention_probs(states[layer], layer, cu, cu_np, max_len))
        res[key]["store_gb_per_s"] = layer_bytes / res[key]["median_ms"] / 1e6
    hip = ctypes.CDLL("libamdhip64.so")
    hip.hipMemsetAsync.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t, ctypes.c_void_p]
    buf = torch.empty(layer_bytes, dtype=torch.uint8, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    res["memset"] = t(lambda: hip.hipMemsetAsync(buf.data_ptr(), 0, layer_bytes, stream))
    res["memset"]["store_gb_per_s"] = layer_bytes / res["memset"]["median_ms"] / 1e6
    enc.close()
    for key in ("plain", "all_layers", "one_layer", "pass_global", "pass_local", "memset"):
        r = res[key]
        rate = f" | {r['store_gb_per_s']:.0f} GB/s stored" if "store_gb_per_s" in r else ""
        print(f"{key:12s} {r['median_ms']:.3f} ms (min {r['min_ms']:.3f} .. max {r['max_ms']:.3f}){rate}", flush=True)
    print(f"xsmall {args.pairs} x {args.length} on {res['kernel_set']}: attentions of every layer +{res['all_layers']['median_ms'] - res['plain']['median_ms']:.3f} ms, "
          f"of one layer +{res['one_layer']['median_ms'] - res['plain']['median_ms']:.3f} ms beside a plain forward; "
          f"{layer_bytes / 1e6:.1f} MB per layer")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
