#!/usr/bin/env python
"""GPU box: measure the attention probabilities of every kernel set a fixture's handle can select against the attention
fixtures (g13 / g14), exactly as tests/test_gpu_attentions.py computes the error, and write
  <out>/attention_bounds.json   per fixture and kernel set, the MEASURED per-layer max |error| (-> tests/golden/; the test
                                     asserts 1.5 x each)
  <out>/attention_probs.txt     the same as text, with the "fp32" set's ratio to the reference's own distance to fp64
                                     (-> profiles/)
<out> is the first argument (default: bench_out/ in the repository, which git ignores).  Regenerate (and review the diff) whenever the arithmetic of a kernel set or of op_attention_probs changes."""
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

from attention_utils import fixture_encoder, fixture_errors, selectable_sets  # noqa: E402

FIXTURES = ["g13_attn_hd64", "g14_attn_h256"]

out, lines = {}, []
for name in FIXTURES:
    enc, arrays, meta, rows = fixture_encoder(name)
    out[name] = {}
    lines.append(f"{name}: reference to fp64 per layer {['%.2e' % r for r in meta['ref_to_fp64']]}")
    for kernel_set in selectable_sets(enc):
        enc.select_kernel_set(kernel_set)
        errs = fixture_errors(enc, arrays, meta, rows)
        out[name][kernel_set] = errs
        line = f"[attn] {name} {kernel_set} per-layer max|err| {['%.2e' % e for e in errs]}"
        if kernel_set == "fp32":
            line += f"  ratio to reference-to-fp64 {['%.2f' % (e / r) for e, r in zip(errs, meta['ref_to_fp64'])]}"
        lines.append(line)
        print(line, flush=True)
    enc.close()
out_dir = sys.argv[1] if len(sys.argv) > 1 else os.path.join(REPO, "bench_out")
os.makedirs(out_dir, exist_ok=True)
with open(os.path.join(out_dir, "attention_bounds.json"), "w") as fh:
    json.dump(out, fh, indent=1, sort_keys=True)
with open(os.path.join(out_dir, "attention_probs.txt"), "w") as fh:
    fh.write("\n".join(lines) + "\n")
print(f"wrote attention_bounds.json and attention_probs.txt under {out_dir}")
