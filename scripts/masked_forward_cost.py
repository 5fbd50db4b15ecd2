"""What a left-padded batch costs on an ``attention_masks="any"`` model -- on the fp32 kernels (``op_forward_masked``: dense, the
default) and on the calibrated set (``masked_kernels="selected"``: ``op_forward_masked_native``, dense) -- against the same rows
right-padded on kernel set "fp32" and on the calibrated set.  xsmall dims, 32 x 512, lengths 128 .. 512; device-resident
inputs; the four forwards alternate, each call ends in a device synchronise; median of the timed calls after warm-up.

    python scripts/masked_forward_cost.py [--out profiles/masked_forward_cost.txt]
"""

from __future__ import annotations

import argparse
import statistics
import sys
import time
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
sys.path.insert(0, str(Path(__file__).resolve().parents[1] / "tests"))


def main() -> None:
    from helpers import CharTokenizer
    from open_provence_amd.config import OpenProvenceConfig
    from open_provence_amd.modeling import OpenProvenceModel
    from open_provence_amd.synthetic import named_dims, pad_rows, refinit_state_dict, synth_pair_batch

    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=32)
    ap.add_argument("--width", type=int, default=512)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    dims = named_dims("xsmall")
    cfg = OpenProvenceConfig(base_model_config=dims.to_base_model_config(), tokenizer_name_or_path="char-tokenizer",
                             pruning_config={"hidden_size": dims.hidden_size}, max_length=args.width, num_labels=1,
                             pruning_hidden_state="post_final_norm")
    state = refinit_state_dict(dims, seed=5)

    def model(**kw):
        return OpenProvenceModel(cfg, device="cuda:0", tokenizer=CharTokenizer(), state_dict=state, **kw)

    lengths = np.linspace(128, args.width, args.rows).astype(int).tolist()
    ids, mask = pad_rows(synth_pair_batch(dims, args.rows, lengths, seed=3))
    ids_d, right, left = ids.cuda(), mask.cuda(), torch.flip(mask, [1]).cuda()
    left_ids = torch.flip(ids, [1]).cuda()  # the same tokens behind the padding (a left-padding tokenizer's batch)

    any_model = model(attention_masks="any", calibrate=True)
    f32_model = model(kernel_set="fp32", calibrate=False)
    sel_model = model(attention_masks="any", masked_kernels="selected", calibrate=True)
    chosen = any_model.encoder.effective_policy()["kernel_set"]
    assert sel_model.encoder.effective_policy()["kernel_set"] == chosen and not sel_model.encoder.attention_outputs
    runs = {
        'left-padded, attention_masks="any" (op_forward_masked)': lambda: any_model(input_ids=left_ids, attention_mask=left),
        'right-padded, kernel set "fp32"': lambda: f32_model(input_ids=ids_d, attention_mask=right),
        f'right-padded, calibrated set "{chosen}"': lambda: any_model(input_ids=ids_d, attention_mask=right),
        f'left-padded, masked_kernels="selected" ("{chosen}")': lambda: sel_model(input_ids=left_ids, attention_mask=left),
    }
    times = {name: [] for name in runs}
    for i in range(args.warmup + args.calls):
        for name, call in runs.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            call()
            torch.cuda.synchronize()
            if i >= args.warmup:
                times[name].append((time.perf_counter() - t0) * 1e3)
    tokens, cells = int(mask.sum()), int(mask.numel())
    lines = [f"forward() of {args.rows} x {args.width} (xsmall dims, reference-initialised weights), lengths {lengths[0]} .. {lengths[-1]}: "
             f"{tokens} tokens in {cells} positions; device-resident inputs",
             f"median (min .. max) of {args.calls} alternating calls after {args.warmup} warm-up calls, each ending in a device synchronise", ""]
    base = statistics.median(times[list(runs)[1]])
    for name, ts in times.items():
        med = statistics.median(ts)
        lines.append(f"  {name:62s} {med:8.3f} ms  ({min(ts):.3f} .. {max(ts):.3f})   x {med / base:5.2f} of the fp32 set right-padded")
    lines += ["", f"The dense passes compute all {cells} positions ({cells / tokens:.2f} x the tokens) and synchronise the stream once per call (id check)."]
    # the reading, from the figures above: nothing here is fixed in advance
    names = list(runs)
    med = {name: statistics.median(ts) for name, ts in times.items()}
    spread = {name: max(ts) - min(ts) for name, ts in times.items()}
    masked_f32, packed_sel, masked_sel = names[0], names[2], names[3]
    gap = med[masked_f32] - med[masked_sel]
    widest = max(spread[masked_f32], spread[masked_sel])
    lines += ["", f"Reading: the left-padded forward on the calibrated set takes {med[masked_sel] / med[masked_f32]:.2f} x the fp32 masked route's time "
              f"({med[masked_f32] / med[masked_sel]:.2f} x faster); the medians differ by {gap:.3f} ms, the wider min .. max spread of the two is {widest:.3f} ms"
              f" -- {'beyond' if gap > widest else 'WITHIN'} it.",
              f"It costs {med[masked_sel] / med[packed_sel]:.2f} x the same rows right-padded on the same set, beside the {cells / tokens:.2f} x positions "
              "the dense pass computes; the fp32 masked route costs "
              f"{med[masked_f32] / med[packed_sel]:.2f} x that forward.  Skipping all-pad tiles or packing the valid queries is what would recover the rest."]
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(text)


if __name__ == "__main__":
    main()
