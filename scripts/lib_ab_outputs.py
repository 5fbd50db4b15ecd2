#!/usr/bin/env python
"""Are two builds of the library the same function?  Raw bytes of every output, case by case.

    python scripts/lib_ab_outputs.py libA.so libB.so [--baseline] [--cases-per-child K] [--only a,c] [--out table.txt]

Each case is one encoder of the conformance suite (tests/test_kernel_set_conformance.py: its models, weights, row list, vocab 512,
seed 7) and one forward with every hidden state requested (fp32, packed): the pruning logits, the ranking logits and all hidden
entries are compared byte for byte between the two libraries.  Cases:
  a  every (model, set) of MODELS x SUPPORTED on the weights weights_for() gives the set
  b  every (model, flag, set) of FLAG_RUNS
  c  the default selection (no pin) on row / panel512 / tiled, fp32-valued and bf16-valued O(1) weights; these also report the
     drop in free device memory across encoder creation + weight load, which must be equal
  d  a custom term policy no kernel set matches (all-terms kernels, cleared lo operands) on row and panel512
  e  set f16+mlp-f16-f8-w on the 4-layer panel model, layer mask {0, 2}
  f  mean pooling, and prune_pre_final_norm, on row "f16"
A library is loaded once per process (OPEN_PROVENCE_HIP_LIB), so every (case, library) runs in a fresh child with its own time
limit; --cases-per-child K lets one child run K consecutive cases (fewer process starts).  The driver stops at
the first child that fails.  --baseline runs libA a second time first: a case that is not bit-identical run to run on libA is
listed as such and held to "max-abs difference no larger than libA showed against itself"; every other case must show zero
differing bytes.  Exit status 1 if any case fails."""
import argparse
import json
import os
import subprocess
import sys
import tempfile
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

CUSTOM_TERMS = "wqkv=3,qk=1,pv=3,attn_out=3,wi=3,mlp_out=3"  # no lo(k) term: no curated set has these masks
CHILD_SECONDS = 240


def all_cases():
    import test_kernel_set_conformance as conf

    def case(group, model, kernel_set, weights, **extra):
        name = f"{group} {model} {kernel_set or 'default'} {weights}" + "".join(f" {k}={v}" for k, v in extra.items())
        return dict(group=group, name=name, model=model, set=kernel_set, weights=weights, **extra)

    cases = [case("a", m, s, conf.weights_for(s, "o1")) for m in conf.MODELS for s in conf.SUPPORTED[m]]
    cases += [case("b", m, s, conf.weights_for(s, "o1"), flags=f) for (m, f), sets in conf.FLAG_RUNS.items() for s in sets]
    cases += [case("c", m, None, w, mem=1) for m in ("row", "panel512", "tiled") for w in ("o1", "o1-bf16")]
    cases += [case("d", m, None, "o1", precision=CUSTOM_TERMS) for m in ("row", "panel512")]
    cases += [case("e", "panel512x4", "f16+mlp-f16-f8-w", conf.weights_for("f16+mlp-f16-f8-w", "o1"), mask=0b101)]
    cases += [case("f", "row", "f16", conf.weights_for("f16", "o1"), pooling="mean"),
              case("f", "row", "f16", conf.weights_for("f16", "o1"), pre_norm=1)]
    return cases


def run_child(spec_path: str, out_path: str) -> None:
    import ctypes

    import torch

    import test_kernel_set_conformance as conf
    from open_provence_amd import _lib
    from open_provence_amd.engine import HiddenRequest, HipEncoder
    from open_provence_amd.packing import pack_rows

    torch.cuda.init()
    torch.cuda.synchronize()
    rows = conf._rows(conf.LENGTHS)
    ids_np, cu_np, max_len = pack_rows(rows)
    ids, cu = torch.from_numpy(ids_np).cuda(), torch.from_numpy(cu_np).cuda()
    out = {}
    for i, c in enumerate(json.loads(Path(spec_path).read_text())):
        dims = conf._dims(c["model"], pooling=c.get("pooling"))
        state = conf._state(c["model"], c["weights"])
        torch.cuda.synchronize()
        free_before = torch.cuda.mem_get_info()[0]
        enc = HipEncoder(dims, device="cuda:0", precision=c.get("precision", "bf16x3"), flags=conf._flag_bits([c["flags"]] if c.get("flags") else []),
                         prune_pre_final_norm=bool(c.get("pre_norm")))
        try:
            enc.load_state_dict(state, calibrate=False, kernel_set=c["set"])
            torch.cuda.synchronize()
            out[f"{i}.mem"] = np.array([free_before - torch.cuda.mem_get_info()[0]], dtype=np.int64)
            if c.get("mask") is not None:
                _lib.check(enc.lib, enc._handle, enc.lib.op_select_mlp_correction_layers(enc._handle, ctypes.c_uint64(c["mask"])),
                           "op_select_mlp_correction_layers")
            policy = enc.effective_policy()
            if c["set"]:
                assert policy["kernel_set"] == c["set"], policy
            prune, rank, hidden = enc.forward_packed(ids, cu, cu_np, max_len, hidden=HiddenRequest())
            torch.cuda.synchronize()
            out[f"{i}.ran"] = np.frombuffer(str(policy["kernel_set"]).encode(), dtype=np.uint8)
            for key, t in (("prune", prune), ("rank", rank), ("hidden", hidden)):
                assert t.dtype == torch.float32
                out[f"{i}.{key}"] = t.cpu().contiguous().numpy().reshape(-1)
        finally:
            enc.close()
    np.savez(out_path, **out)


def compare(x: dict, y: dict, i: int):
    """(differing bytes, max-abs difference (NaN-aware: inf if finiteness differs), bytes compared) over the three outputs"""

    diff = total = 0
    worst = 0.0
    for key in ("prune", "rank", "hidden"):
        p, q = x[f"{i}.{key}"], y[f"{i}.{key}"]
        assert p.shape == q.shape, (key, p.shape, q.shape)
        diff += int(np.count_nonzero(p.view(np.uint8) != q.view(np.uint8)))
        total += p.nbytes
        both = np.isfinite(p) & np.isfinite(q)
        if not np.array_equal(np.isfinite(p), np.isfinite(q)):
            worst = float("inf")
        elif both.any():
            worst = max(worst, float(np.max(np.abs(p[both].astype(np.float64) - q[both].astype(np.float64)))))
    return diff, worst, total


def main() -> int:
    if len(sys.argv) == 4 and sys.argv[1] == "--child":
        run_child(sys.argv[2], sys.argv[3])
        return 0
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("lib_a")
    ap.add_argument("lib_b")
    ap.add_argument("--baseline", action="store_true", help="run lib_a twice first: its own run-to-run difference is the bound")
    ap.add_argument("--cases-per-child", type=int, default=1)
    ap.add_argument("--only", default="", help="comma-separated case groups (a..f)")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    only = set(filter(None, args.only.split(",")))
    cases = [c for c in all_cases() if not only or c["group"] in only]
    batches = []
    for c in cases:
        if batches and len(batches[-1]) < args.cases_per_child:
            batches[-1].append(c)
        else:
            batches.append([c])
    runs = [("A", args.lib_a)] + ([("A2", args.lib_a)] if args.baseline else []) + [("B", args.lib_b)]
    lines = [f"A = {args.lib_a}", f"B = {args.lib_b}",
             f"{len(cases)} cases in {len(batches)} children per library run; rows {'baseline A/A2, ' if args.baseline else ''}A/B: differing bytes (max-abs)"]
    failed = 0
    with tempfile.TemporaryDirectory() as tmp:
        for bi, batch in enumerate(batches):
            spec = Path(tmp) / f"spec{bi}.json"
            spec.write_text(json.dumps(batch))
            got = {}
            for tag, lib in runs:
                out = Path(tmp) / f"out{bi}{tag}.npz"
                env = dict(os.environ, OPEN_PROVENCE_HIP_LIB=str(Path(lib).resolve()))
                try:
                    r = subprocess.run([sys.executable, str(Path(__file__).resolve()), "--child", str(spec), str(out)], env=env, cwd=str(ROOT),
                                       capture_output=True, text=True, timeout=CHILD_SECONDS)
                except subprocess.TimeoutExpired:
                    print("\n".join(lines))
                    print(f"STOP: child {tag} of batch {bi} ({batch[0]['name']} ...) ran past {CHILD_SECONDS} s", flush=True)
                    return 2
                if r.returncode != 0:
                    print("\n".join(lines))
                    print(f"STOP: child {tag} of batch {bi} ({batch[0]['name']} ...) exited {r.returncode}:\n{r.stderr[-2000:]}", flush=True)
                    return 2
                with np.load(out) as z:
                    got[tag] = {k: z[k] for k in z.files}
            for i, c in enumerate(batch):
                ran = {tag: bytes(got[tag][f"{i}.ran"]).decode() for tag in got}
                d_ab, w_ab, total = compare(got["A"], got["B"], i)
                d_aa, w_aa = (compare(got["A"], got["A2"], i)[:2]) if args.baseline else (0, 0.0)
                ok = ran["A"] == ran["B"] and (d_ab == 0 if d_aa == 0 else w_ab <= w_aa)
                mem = ""
                if c.get("mem"):
                    ma, mb = int(got["A"][f"{i}.mem"][0]), int(got["B"][f"{i}.mem"][0])
                    ok = ok and ma == mb
                    mem = f" | device memory A {ma} B {mb} bytes"
                failed += 0 if ok else 1
                base = f"A/A2 {d_aa} ({w_aa:.3g}) " if args.baseline else ""
                note = "" if d_aa == 0 else " [not bit-identical run to run on A]"
                line = f"{'ok  ' if ok else 'FAIL'} {c['name']:70s} ran {ran['A']}/{ran['B']} | {total} bytes | {base}A/B {d_ab} ({w_ab:.3g}){note}{mem}"
                lines.append(line)
                print(line, flush=True)
    lines.append(f"{len(cases) - failed} of {len(cases)} cases pass")
    print(lines[-1], flush=True)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text("\n".join(lines) + "\n")
    return 1 if failed else 0


if __name__ == "__main__":
    sys.exit(main())
