#!/usr/bin/env python
"""GPU-box probe: end-to-end ``process()`` (host pipeline + HIP forward) on a synthetic 1-query x N-context
request with the char tokenizer of the tests; prints the reference-style timing breakdown and, with
--profile, the top of a cProfile run.  Usage: scripts/process_e2e.py [--contexts 256] [--chars 470] [--profile]

--forward-tokens 0,r1,r2,r4 compares token budgets of the forwards (OpenProvenceModel.forward_token_budget; "rN" = N rounds
of the chip, n_cus x 128 tokens; 0 = the fixed batch_size stride): the settings take turns (--passes times: a warm-up call,
then --reps timed calls each) and every setting gets one JSON line with the median and the spread of its calls."""
import argparse
import cProfile
import io
import json
import os
import pstats
import resource
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

import numpy as np
import torch

from helpers import CharTokenizer, period_splitter


def make_request(n_contexts: int, chars: int, seed: int = 5):
    rng = np.random.default_rng(seed)
    words = ["alpha", "beta", "gamma", "delta", "epsilon", "zeta", "eta", "theta", "iota", "kappa", "lambda", "mu"]
    contexts = []
    for _ in range(n_contexts):
        parts, total = [], 0
        while total < chars:
            n = int(rng.integers(5, 12))
            sent = " ".join(words[int(i)] for i in rng.integers(0, len(words), n)) + ". "
            parts.append(sent)
            total += len(sent)
        contexts.append("".join(parts)[:chars].rstrip() + ".")
    return "which greek letters appear here", contexts


def build_e2e_tokenizer():
    """Tokenizer factory (module level: HostFrontEnd's replicas rebuild it by name); kind from the environment."""

    if os.environ.get("E2E_TOKENIZER", "char") == "wordpiece":
        from helpers import build_wordpiece_tokenizer

        return build_wordpiece_tokenizer(True, legacy_methods=os.environ.get("E2E_STOCK_TOKENIZER") != "1")
    return CharTokenizer()


def build_e2e_model():
    """Model factory (module level: ProcessFrontEnd's worker processes rebuild it by name); tokenizer from the environment."""

    from open_provence_amd.config import OpenProvenceConfig
    from open_provence_amd.modeling import OpenProvenceModel
    from open_provence_amd.synthetic import named_dims, refinit_state_dict, synth_state_dict

    dims = named_dims("xsmall")
    cfg = OpenProvenceConfig(base_model_config=dims.to_base_model_config(), tokenizer_name_or_path="x",
                             pruning_config={"hidden_size": dims.hidden_size}, max_length=512)
    if os.environ.get("E2E_TOKENIZER", "char") == "wordpiece":
        from helpers import build_wordpiece_tokenizer

        tok = build_wordpiece_tokenizer(True, legacy_methods=os.environ.get("E2E_STOCK_TOKENIZER") != "1")
    else:
        tok = CharTokenizer()
    # E2E_WEIGHTS=refinit: reference-initialised weights, which calibrate to kernel set "f16" -- the case the audits of a
    # calibrated set (--audit) exist for; the O(1) default keeps the default set, where no audit ever runs
    make_state = refinit_state_dict if os.environ.get("E2E_WEIGHTS", "synth") == "refinit" else synth_state_dict
    model = OpenProvenceModel(cfg, device="cuda", tokenizer=tok, state_dict=make_state(dims, 7))
    model.tokenizer.model_max_length = 512
    return model


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--front-end", type=int, default=0,
                    help="N > 0: open_provence_amd.frontend.ProcessFrontEnd with N worker processes (all on cuda:0) beside the caller")
    ap.add_argument("--host-front-end", type=int, default=0,
                    help="N > 0: open_provence_amd.frontend.HostFrontEnd -- N host-stage replicas WITHOUT a GPU; this process runs every forward")
    ap.add_argument("--contexts", type=int, default=256)
    ap.add_argument("--chars", type=int, default=470)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--batch-size", type=int, default=256)
    ap.add_argument("--preprocess-batch", type=int, default=None, help="explicit preprocess batch (default: the pipeline granule)")
    ap.add_argument("--profile", action="store_true")
    ap.add_argument("--tokenizer", default="char", choices=["char", "wordpiece"],
                    help="char: the pure-Python tokenizer of the tests; wordpiece: a Hugging Face fast (Rust) tokenizer built offline")
    ap.add_argument("--workers", type=int, default=None, help="preprocess_workers (worker threads of the split / tokenize stage)")
    ap.add_argument("--stock-tokenizer", action="store_true",
                    help="wordpiece: the plain transformers PreTrainedTokenizerFast object (what a checkpoint's tokenizer files load as; "
                    "it pickles, so process() can start host replicas by itself) instead of the test helper's local 4.x-style subclass")
    ap.add_argument("--forward-tokens", default=None,
                    help="token budget of one forward: a number (0 = the fixed batch_size stride), rN (N rounds of n_cus x 128 tokens) or "
                    "'default'; a comma-separated list compares the settings in turns (in-process or with the replicas process() starts)")
    ap.add_argument("--passes", type=int, default=2, help="--forward-tokens with several settings: how often the settings take turns")
    ap.add_argument("--dump-result", default=None, help="write the result of the last call of every setting (without timings) as JSON here")
    ap.add_argument("--chars-are-words", action="store_true", help="wordpiece: size the contexts in words (~tokens) instead of characters")
    ap.add_argument("--weights", default="synth", choices=["synth", "refinit"],
                    help="synth: O(1) worst-case weights (the default kernel set stays); refinit: reference initialisation (calibrates to 'f16')")
    ap.add_argument("--audit", default=None, choices=["off", "first", "running"],
                    help="audit policy of the calibrated kernel set (HipEncoder(audit=...), here through OPEN_PROVENCE_AUDIT)")
    ap.add_argument("--prepared", action="store_true",
                    help="prepare the contexts once, outside the timed region (OpenProvenceModel.prepare_contexts), and time requests on the "
                    "prepared object; in-process only.  The line gains the one-off preparation time and the forwards of a request")
    ap.add_argument("--question", default=None,
                    help="the question, instead of the lower-case default.  With the char tokenizer nearly every context begins with a letter "
                    "of the default question: under OPEN_PROVENCE_PREPARED_DECISIONS=1 that keeps a prepared request on the host stages, "
                    "under =2 the device looks the contexts up in their rows and the request runs there (INTEGRATION.md section 6); an "
                    "upper-case question shares no token id with the contexts and is eligible under either value")
    args = ap.parse_args()
    if args.prepared and (args.front_end or args.host_front_end):
        raise SystemExit("--prepared runs in this process: prepared contexts take no front-end")
    os.environ["E2E_WEIGHTS"] = args.weights
    if args.audit is not None:
        os.environ["OPEN_PROVENCE_AUDIT"] = {"off": "0", "first": "1", "running": "running"}[args.audit]

    os.environ["E2E_TOKENIZER"] = args.tokenizer
    if args.stock_tokenizer:
        os.environ["E2E_STOCK_TOKENIZER"] = "1"
    question, contexts = make_request(args.contexts, args.chars)
    if args.question is not None:
        question = args.question
    budgets = [b.strip() for b in args.forward_tokens.split(",")] if args.forward_tokens else []

    def budget_value(text):
        if text == "default":
            return None
        if text.startswith("r"):
            return int(text[1:]) * int(torch.cuda.get_device_properties(0).multi_processor_count) * 128
        return int(text)

    if len(budgets) == 1:  # (front-end workers and replicas take the budget of the model they are built from)
        value = budget_value(budgets[0])
        if value is not None:
            os.environ["OPEN_PROVENCE_FORWARD_TOKENS"] = str(value)
    front = None
    if args.front_end > 0:
        from open_provence_amd.frontend import ProcessFrontEnd

        front = ProcessFrontEnd(build_e2e_model, workers=args.front_end)
        target = front
    elif args.host_front_end > 0:
        from open_provence_amd.frontend import HostFrontEnd

        front = HostFrontEnd(build_e2e_model(), workers=args.host_front_end, tokenizer_factory=build_e2e_tokenizer)
        target = front
    else:
        target = build_e2e_model()

    prepared, prepare_seconds = None, None
    if args.prepared:
        t0 = time.perf_counter()
        prepared = target.prepare_contexts(contexts, sentence_splitter=period_splitter, preprocess_workers=args.workers)
        prepare_seconds = time.perf_counter() - t0

    def call():
        return target.process(question, contexts if prepared is None else prepared, threshold=0.1, batch_size=args.batch_size,
                              sentence_splitter=period_splitter, show_progress=False, preprocess_batch_size=args.preprocess_batch,
                              preprocess_workers=args.workers)

    if len(budgets) > 1:
        if front is not None:
            raise SystemExit("--forward-tokens with several settings: in-process, or the replicas process() starts by itself")
        compare_budgets(args, target, call, [(b, budget_value(b)) for b in budgets])
        return
    def audits_so_far():
        encoder = getattr(target, "encoder", None)
        return int(((getattr(encoder, "calibration", None) or {}).get("audits") or {}).get("count", 0))

    call()
    torch.cuda.synchronize()
    audits_warm = audits_so_far()
    best = None
    inference_all, stages_all = [], []
    walls, forwards = [], None
    for _ in range(args.reps):
        r0 = resource.getrusage(resource.RUSAGE_SELF)
        t0 = time.perf_counter()
        out = call()
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        r1 = resource.getrusage(resource.RUSAGE_SELF)
        usage = {"user_s": round(r1.ru_utime - r0.ru_utime, 4), "sys_s": round(r1.ru_stime - r0.ru_stime, 4),
                 "minor_faults": r1.ru_minflt - r0.ru_minflt, "vol_ctx_switches": r1.ru_nvcsw - r0.ru_nvcsw,
                 "invol_ctx_switches": r1.ru_nivcsw - r0.ru_nivcsw}
        inference_all.append(round(float(out["timing"]["inference_seconds"]), 5))
        stages_all.append({k: round(float(out["timing"][k]), 5) for k in ("assembly_seconds", "postprocess_seconds", "inference_seconds")})
        if best is None or dt < best[0]:
            best = (dt, out["timing"], usage)
        walls.append(round(dt, 5))
        forwards = getattr(out["performance_trace"], "runtime", {}).get("forwards")
    dt, timing, usage = best
    encoder = getattr(target, "encoder", None)
    audit_info = {} if encoder is None else {"weights": args.weights, "audit": encoder.audit_mode, "kernel_set": encoder.effective_policy()["kernel_set"],
                                             "audits_in_warm_up": audits_warm, "audits_in_timed_calls": audits_so_far() - audits_warm,
                                             "inference_seconds_per_call": inference_all}
    if args.prepared:
        audit_info = {**audit_info, "prepared": True, "prepare_seconds": round(prepare_seconds, 4),
                      "prepare_stage_seconds": {k: round(float(v), 4) for k, v in prepared.timing.items()},
                      "corpus_tokens": prepared.n_tokens, "corpus_device_bytes": prepared.device_bytes,
                      "prepared_decisions": getattr(out["performance_trace"], "runtime", {}).get("prepared_decisions"),
                      "stage_seconds_per_call": stages_all}
    audit_info = {**audit_info, "batch_size": args.batch_size, "forwards": forwards, "wall_s_per_call": walls,
                  "wall_s_median": round(float(np.median(walls)), 5)}
    print(json.dumps({**audit_info, "contexts": args.contexts, "chars": args.chars, "tokenizer": args.tokenizer, "workers": args.workers, "front_end_processes": args.front_end, "host_replicas": args.host_front_end, "wall_s": dt, "contexts_per_s": args.contexts / dt, "rusage": usage, "owner_trace": getattr(front, "last_trace", None),
                      "timing": {k: round(float(v), 5) for k, v in timing.items()}}))
    if args.profile:
        pr = cProfile.Profile()
        pr.enable()
        call()
        pr.disable()
        buf = io.StringIO()
        pstats.Stats(pr, stream=buf).sort_stats("cumulative").print_stats(35)
        print(buf.getvalue()[:6000])
    if front is not None:
        front.close()


def compare_budgets(args, model, call, settings):
    """The same call under every budget in turns; one JSON line per setting."""

    runs = {label: [] for label, _ in settings}
    last = {}
    for _ in range(max(1, args.passes)):
        for label, value in settings:
            model.forward_token_budget = value
            call()  # warm-up (with replicas: they are restarted with the new budget here)
            torch.cuda.synchronize()
            for _ in range(args.reps):
                t0 = time.perf_counter()
                out = call()
                torch.cuda.synchronize()
                runs[label].append((time.perf_counter() - t0, out))
            last[label] = out
    keep = lambda out: {k: v for k, v in out.items() if k not in ("timing", "performance_trace")}
    first = keep(last[settings[0][0]])
    for label, value in settings:
        walls = np.array([dt for dt, _ in runs[label]])
        inference = np.array([out["timing"]["inference_seconds"] for _, out in runs[label]])
        total = np.array([out["timing"]["total_seconds"] for _, out in runs[label]])
        forwards = [getattr(out["performance_trace"], "runtime", {}).get("forwards", {}) for _, out in runs[label]]
        stat = lambda a: {"median": round(float(np.median(a)), 5), "min": round(float(a.min()), 5), "max": round(float(a.max()), 5)}
        print(json.dumps({"forward_tokens": label, "token_budget": forwards[-1].get("token_budget"), "contexts": args.contexts,
                          "batch_size": args.batch_size, "tokenizer": args.tokenizer, "calls": len(walls),
                          "host_replicas": runs[label][-1][1]["timing"].get("host_replicas", 0),
                          "inference_seconds": stat(inference), "total_seconds": stat(total), "wall_seconds": stat(walls),
                          "contexts_per_s": round(args.contexts / float(np.median(walls)), 1),
                          "launches": sorted({f.get("launches") for f in forwards}, key=lambda v: -1 if v is None else v),
                          "equals_first_setting": keep(last[label]) == first}), flush=True)
    if args.dump_result:
        with open(args.dump_result, "w", encoding="utf-8") as handle:
            json.dump({label: keep(out) for label, out in last.items()}, handle)
    front = model.__dict__.get("_host_front_end")
    if front is not None:
        front.close()


if __name__ == "__main__":
    main()
