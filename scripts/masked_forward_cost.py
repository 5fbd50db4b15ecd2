"""What a left-padded batch costs on an ``attention_masks="any"`` model (``op_forward_masked``: dense, fp32 kernels) against the
same rows right-padded on kernel set "fp32" and on the calibrated set.  xsmall dims, 32 x 512, lengths 128 .. 512; device-resident
inputs; the three forwards alternate, each call ends in a device synchronise; median of the timed calls after warm-up.

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
    runs = {
        'left-padded, attention_masks="any" (op_forward_masked)': lambda: any_model(input_ids=left_ids, attention_mask=left),
        'right-padded, kernel set "fp32"': lambda: f32_model(input_ids=ids_d, attention_mask=right),
        f'right-padded, calibrated set "{any_model.encoder.effective_policy()["kernel_set"]}"': lambda: any_model(input_ids=ids_d, attention_mask=right),
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
    lines += ["", f"The dense pass computes all {cells} positions ({cells / tokens:.2f} x the tokens) and synchronises the stream once per call (id check)."]
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(text)


if __name__ == "__main__":
    main()
