"""The host-only planning header (open_provence_amd/csrc/op_plan.h) without a GPU: kernel-set availability and selection,
op_calibrate's candidate order and search, chunking, the attention plan, the workspace layout and the cu_seqlens checks.

tests/host/plan_check.cpp -- a program with a main of its own, no HIP -- is compiled against the header with the host C++
compiler under AddressSanitizer and UBSan (a plain build where the sanitized link fails), run once as a child process with
every query of this module on its stdin, and answers one line per query.  Every expectation is written out here or computed
by a short restatement here; none comes from the header."""

from __future__ import annotations

import itertools
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

import test_kernel_set_conformance as conf
from open_provence_amd import _lib

ROOT = Path(__file__).resolve().parents[1]
SOURCE = ROOT / "tests" / "host" / "plan_check.cpp"
SANITIZE = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
ROW_ALIGN = 32
ALL = "ffffffffffffffff"  # the layer mask of a set that is not 8 / 9, and of a call without one
FULL_REPORT, WHOLE_DEPTH = 1, 2
OK, INVALID, UNSUPPORTED, HIP_ERROR = 0, -1, -2, -3
FLOAT, INDEX, FLAG = 0, 1, 2


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    compilers = [c for c in (shutil.which("c++"), shutil.which("g++"), "/opt/rocm/llvm/bin/clang++") if c and Path(c).exists()]
    assert compilers, "no host C++ compiler"
    exe = tmp_path_factory.mktemp("plan") / "plan_check"
    errors = []
    for extra in (SANITIZE, []):  # (the sanitized link first; a plain build still makes every assertion below)
        for cxx in compilers:
            built = subprocess.run([cxx, "-std=c++17", "-O1", "-g", *extra, str(SOURCE), "-o", str(exe)], capture_output=True, text=True)
            if built.returncode == 0 and subprocess.run([str(exe)], input="", capture_output=True, text=True).returncode == 0:
                return exe
            errors.append(f"{cxx} {' '.join(extra)}: {built.stderr[-2000:]}")
    pytest.fail("plan_check.cpp does not build:\n" + "\n".join(errors))


def ask(program, queries):
    """One answer line per query line; a sanitizer report ends the child with a non-zero status."""

    done = subprocess.run([str(program)], input="\n".join(queries) + "\n", capture_output=True, text=True)
    assert done.returncode == 0, done.stderr[-4000:]
    answers = done.stdout.splitlines()
    assert len(answers) == len(queries)
    return answers


def ints(line):
    return [int(v) for v in line.split()]


# ---- availability ---------------------------------------------------------------------------------------------------------------
def test_available_sets_per_model_and_flag(program):
    cases = [(model, 0) for model in conf.MODELS] + [(model, conf._flag_bits([flag])) for model, flag in conf.SUPPORTED_WITH_FLAG]
    expected = [conf.SUPPORTED[model] for model in conf.MODELS] + list(conf.SUPPORTED_WITH_FLAG.values())
    answers = ask(program, [f"avail {conf.MODELS[m][0]} {conf.MODELS[m][1]} {flags} 0" for m, flags in cases])
    for (model, flags), names, line in zip(cases, expected, answers):
        assert ints(line) == sorted(_lib.KERNEL_SET_IDS[n] for n in names), (model, flags)
    # the fp32 set: with its packs only, on every path, and beside set 0 under NO_POLICY_KERNELS
    f32 = _lib.OP_FLAG_F32_PACKS
    row, tiled = conf.MODELS["row"], conf.MODELS["tiled"]
    got = ask(program, [f"avail {tiled[0]} {tiled[1]} {f32} 0", f"avail {row[0]} {row[1]} {f32 | _lib.OP_FLAG_NO_POLICY_KERNELS} 0",
                        f"avail {row[0]} {row[1]} 0 1"])  # (last: a tensor on fp16's subnormal grid)
    assert [ints(line) for line in got] == [[0, 12], [0, 12], [0, 1, 2]]


# ---- default selection and pinning ----------------------------------------------------------------------------------------------
ROW, PANEL = (256, 1024), (512, 2048)
ALL_TERMS, BF16_WEIGHTS, SINGLE = (3, 3, 3, 3, 3, 3), (1, 3, 3, 1, 1, 1), (0, 0, 0, 0, 0, 0)


def select_query(shape, flags=0, req=ALL_TERMS, lo=1, not_f16=1, unfit=0, f8_off=0, forced=-1, mask=ALL):
    return f"select {shape[0]} {shape[1]} {flags} {' '.join(map(str, req))} {lo} {lo} {lo} {lo} {not_f16} {unfit} {f8_off} {forced} {mask}"


def test_default_selection_and_pins(program):
    f = _lib
    cases = [  # (query, evaluated terms, set, layer mask)
        # fp32-valued weights
        (select_query(ROW), ALL_TERMS, 4, ALL),
        (select_query(PANEL), ALL_TERMS, 5, ALL),
        (select_query(PANEL, f.OP_FLAG_PANEL_F8), ALL_TERMS, 4, ALL),
        # bf16-valued, exact fp16
        (select_query(ROW, lo=0, not_f16=0), BF16_WEIGHTS, 3, ALL),
        (select_query(PANEL, lo=0, not_f16=0), BF16_WEIGHTS, 1, ALL),
        (select_query(PANEL, f.OP_FLAG_PANEL_F8_WI, lo=0, not_f16=0), BF16_WEIGHTS, 6, ALL),
        (select_query(PANEL, f.OP_FLAG_PANEL_F8, lo=0, not_f16=0), BF16_WEIGHTS, 3, ALL),
        # bf16-valued, not exact fp16
        (select_query(ROW, lo=0, not_f16=1), BF16_WEIGHTS, 1, ALL),
        # a tensor on fp16's subnormal grid: no set with an fp16 plane
        (select_query(ROW, unfit=1), ALL_TERMS, 0, ALL),
        (select_query(ROW, lo=0, not_f16=0, unfit=1), BF16_WEIGHTS, 1, ALL),
        (select_query(PANEL, unfit=1), ALL_TERMS, 0, ALL),
        # NO_POLICY_KERNELS: the all-terms kernels, as set 0 or with cleared operands
        (select_query(ROW, f.OP_FLAG_NO_POLICY_KERNELS), ALL_TERMS, 0, ALL),
        (select_query(ROW, f.OP_FLAG_NO_POLICY_KERNELS, lo=0, not_f16=0), BF16_WEIGHTS, -1, ALL),
        # a custom policy that is no set's
        (select_query(ROW, req=(3, 3, 3, 3, 3, 1)), (3, 3, 3, 3, 3, 1), -1, ALL),
        (select_query(ROW, req=(3, 1, 3, 3, 3, 3), lo=0, not_f16=0), (1, 1, 3, 1, 1, 1), -1, ALL),
        # requested single pass
        (select_query(ROW, req=SINGLE), SINGLE, 2, ALL),
        # op_set_compact_operands(0)
        (select_query(ROW, f8_off=1), ALL_TERMS, 0, ALL),
        (select_query(ROW, lo=0, not_f16=0, f8_off=1), BF16_WEIGHTS, 1, ALL),
        # a pinned set the handle can run wins, and its terms are the evaluated ones; one it cannot run is ignored
        (select_query(ROW, forced=7), SINGLE, 7, ALL),
        (select_query(ROW, forced=1), BF16_WEIGHTS, 1, ALL),
        (select_query(ROW, forced=9), ALL_TERMS, 4, ALL),
        (select_query(ROW, forced=12), ALL_TERMS, 4, ALL),
        (select_query(ROW, f.OP_FLAG_F32_PACKS, forced=12), ALL_TERMS, 12, ALL),
        (select_query(PANEL, forced=10), (3, 0, 0, 3, 3, 3), 10, ALL),
        # the layer mask belongs to sets 8 / 9
        (select_query(PANEL, forced=9, mask="5"), SINGLE, 9, "5"),
        (select_query(PANEL, forced=8, mask="a"), SINGLE, 8, "a"),
        (select_query(PANEL, forced=7, mask="5"), SINGLE, 7, ALL),
    ]
    for (query, terms, kernel_set, mask), line in zip(cases, ask(program, [c[0] for c in cases])):
        got = line.split()
        assert (tuple(map(int, got[:6])), int(got[6]), got[7]) == (terms, kernel_set, mask), query


def test_candidate_order(program):
    got = ask(program, [f"cand {ROW[0]} {ROW[1]} 0 4", f"cand {PANEL[0]} {PANEL[1]} 0 5", f"cand {ROW[0]} {ROW[1]} 0 7",
                        f"cand 384 192 0 0"])
    assert [ints(line) for line in got] == [[7, 2, 3], [7, 2, 9, 11, 3, 8, 6, 10, 1, 4], [], []]


# ---- the search -----------------------------------------------------------------------------------------------------------------
def search(program, n_layers, tol, flags, reference, default, cand, rules):
    """rules: (set, mask as hex or '*', error, rc) of the scripted measure; an exact mask goes before '*'."""

    query = (f"search {n_layers} {tol!r} {flags} {reference} {default} {len(cand)} {' '.join(map(str, cand))} {len(rules)} "
             + " ".join(f"{s} {m} {e} {rc}" for s, m, e, rc in rules))
    head, calls = ask(program, [query])[0].split("|")
    head = head.split()
    return dict(rc=int(head[0]), chosen=int(head[1]), mask=int(head[2], 16), default_err=float(head[3]), mask_err=float(head[4]),
                candidates=[(int(c.split("=")[0]), float(c.split("=")[1])) for c in head[6:]], n=int(head[5]),
                calls=[(int(c.split(":")[0]), c.split(":")[1]) for c in calls.split()])


ROW_CAND = [7, 2, 3]
ROW_RULES = [(0, "*", 0, OK), (4, "*", 5e-5, OK), (7, "*", 1e-3, OK), (2, "*", 5e-5, OK), (3, "*", 1e-5, OK)]


def test_search_stops_at_the_first_candidate_that_holds(program):
    r = search(program, 3, 1e-4, 0, 0, 4, ROW_CAND, ROW_RULES)
    assert (r["rc"], r["chosen"], r["mask"]) == (OK, 2, 0b111)
    assert r["calls"] == [(0, ALL), (4, ALL), (7, ALL), (2, ALL)]
    assert r["candidates"] == [(7, pytest.approx(1e-3, rel=1e-6)), (2, pytest.approx(5e-5, rel=1e-6))] and r["n"] == 2
    assert r["default_err"] == pytest.approx(5e-5, rel=1e-6) and r["mask_err"] == 0
    full = search(program, 3, 1e-4, FULL_REPORT, 0, 4, ROW_CAND, ROW_RULES)
    assert (full["rc"], full["chosen"]) == (OK, 2) and [c for c, _ in full["candidates"]] == ROW_CAND
    assert full["calls"] == [(0, ALL), (4, ALL), (7, ALL), (2, ALL), (3, ALL)]


def test_search_reference_rules(program):
    # the default is the reference: it is not measured a second time
    r = search(program, 3, 1e-4, 0, 0, 0, ROW_CAND, ROW_RULES)
    assert r["calls"] == [(0, ALL), (7, ALL), (2, ALL)] and r["chosen"] == 2 and r["default_err"] == 0
    # a non-finite reference: nothing else runs, nothing is chosen
    r = search(program, 3, 1e-4, FULL_REPORT, 0, 4, ROW_CAND, [(0, "*", "inf", OK)] + ROW_RULES[1:])
    assert (r["rc"], r["chosen"], r["n"], r["calls"]) == (OK, -1, 0, [(0, ALL)])


def test_search_falls_back_to_the_reference_beyond_ten_tolerances(program):
    tol = 0.125  # (10 x tol is exact in fp32)
    above = float(np.nextafter(np.float32(1.25), np.float32(2)))
    for default_err, chosen in ((above, 0), (1.25, -1), ("inf", 0)):
        r = search(program, 3, tol, 0, 0, 4, ROW_CAND, [(0, "*", 0, OK), (4, "*", default_err, OK), (7, "*", 1, OK), (2, "*", 1, OK), (3, "*", 1, OK)])
        assert (r["rc"], r["chosen"], r["n"]) == (OK, chosen, 3), default_err
    # (the default is the reference: there is nothing to fall back to)
    r = search(program, 3, tol, 0, 0, 0, ROW_CAND, [(0, "*", 0, OK), (7, "*", 1, OK), (2, "*", 1, OK), (3, "*", 1, OK)])
    assert r["chosen"] == -1


def test_search_non_finite_and_failing_measurements(program):
    r = search(program, 3, 1e-4, 0, 0, 4, ROW_CAND, [(0, "*", 0, OK), (4, "*", 5e-5, OK), (7, "*", "inf", OK), (2, "*", "inf", OK), (3, "*", 1e-5, OK)])
    assert r["chosen"] == 3 and r["candidates"][:2] == [(7, float("inf")), (2, float("inf"))]
    # a measure that hands the search a NaN all the same: (NaN <= tolerance) is false, the set is never chosen
    r = search(program, 3, 1e-4, FULL_REPORT, 0, 4, ROW_CAND, [(0, "*", 0, OK), (4, "*", 5e-5, OK), (7, "*", "nan", OK), (2, "*", "nan", OK), (3, "*", "nan", OK)])
    assert (r["rc"], r["chosen"], r["n"]) == (OK, -1, 3) and all(e != e for _, e in r["candidates"])
    r = search(program, 3, 1e-4, 0, 0, 4, ROW_CAND, [(0, "*", 0, OK), (4, "*", "nan", OK), (7, "*", "nan", OK), (2, "*", 1, OK), (3, "*", 1, OK)])
    assert (r["rc"], r["chosen"]) == (OK, 0)  # (a default that is not finite: the reference set)
    # the conversion to +inf is the measure's (max_diff): it turns non-finite outputs into +inf: all of them NaN (what the range guard of the fp16 formats writes),
    # or the last one; inf - inf likewise.  (As in the library before the header: a NaN difference that a finite one FOLLOWS is
    # dropped by the comparison -- see max_diff; not asserted here, neither way.)
    got = ask(program, ["maxdiff 3 nan nan nan 1 2 3", "maxdiff 3 1 2 nan 1 2 3", "maxdiff 3 1 2 3.5 1 2 3", "maxdiff 2 1 inf 1 inf",
                        "maxdiff 2 1 inf 1 2", "maxdiff 0"])
    assert [float(v) for v in got] == [float("inf"), float("inf"), 0.5, float("inf"), float("inf"), 0.0]
    # a failing measurement ends the search with its code and nothing chosen
    r = search(program, 3, 1e-4, 0, 0, 4, ROW_CAND, [(0, "*", 0, OK), (4, "*", 5e-5, OK), (7, "*", 1e-3, OK), (2, "*", 0, HIP_ERROR)])
    assert (r["rc"], r["chosen"]) == (HIP_ERROR, -1) and r["calls"][-1] == (2, ALL) and len(r["calls"]) == 4
    r = search(program, 3, 1e-4, 0, 0, 4, ROW_CAND, [(0, "*", 0, HIP_ERROR)])
    assert (r["rc"], r["chosen"], r["calls"]) == (HIP_ERROR, -1, [(0, ALL)])


# error of set 9 by layer mask, 4 layers, tolerance 1: the three walks keep 2, 3 and 1 layers
WALK_ERR = {1: 0.75, 2: 1.5, 3: 2.0, 4: 2.0, 5: 1.5, 6: 0.5, 7: 1.5, 8: 3.0, 9: 0.75, 10: 0.75, 11: 1.5, 12: 2.0, 13: 0.25, 14: 0.5, 15: 0.5}


def walks_restated(n, tol, err):
    """The per-layer search: each layer dropped alone, then first-to-last, last-to-first and by that price."""

    every = (1 << n) - 1
    calls = []

    def measure(mask):
        calls.append(mask)
        return err[mask]

    alone = [measure(every & ~(1 << li)) for li in range(n)]
    best = None
    for order in (list(range(n)), list(range(n - 1, -1, -1)), sorted(range(n), key=lambda li: alone[li])):  # (sorted is stable)
        mask, mask_err = every, 0.0
        for li in order:
            trial = mask & ~(1 << li)
            if trial == 0:
                break
            e = alone[li] if trial == every & ~(1 << li) else measure(trial)
            if e <= tol:
                mask, mask_err = trial, e
        kept = bin(mask).count("1")
        if best is None or kept < best[0]:
            best = (kept, mask, mask_err)
    return best, calls


def test_search_walks_the_layers_of_sets_8_and_9(program):
    rules = [(0, "*", 0, OK), (5, "*", 0.5, OK), (7, "*", 9, OK), (2, "*", 9, OK)] + [(9, f"{m:x}", e, OK) for m, e in WALK_ERR.items()] + [(9, "*", 0.5, OK)]
    r = search(program, 4, 1.0, 0, 0, 5, [7, 2, 9, 11], rules)
    assert (r["rc"], r["chosen"], r["mask"], r["mask_err"]) == (OK, 9, 0b0001, 0.75)
    walk_calls = ["e", "d", "b", "7", "c", "a", "2", "c", "c", "9", "1"]
    assert r["calls"] == [(0, ALL), (5, ALL), (7, ALL), (2, ALL), (9, ALL)] + [(9, m) for m in walk_calls]
    (kept, mask, mask_err), calls = walks_restated(4, 1.0, WALK_ERR)
    assert (kept, mask, mask_err) == (1, 0b0001, 0.75) and [f"{c:x}" for c in calls] == walk_calls
    # OP_CAL_WHOLE_DEPTH: no per-layer search
    r = search(program, 4, 1.0, WHOLE_DEPTH, 0, 5, [7, 2, 9, 11], rules)
    assert (r["chosen"], r["mask"], r["calls"][-1]) == (9, 0b1111, (9, ALL))
    # a tie between walks: the earlier one wins (dropping layer 0 or layer 3 holds, never both)
    tie = {m: 2.0 for m in range(1, 15)}
    tie[0b1110], tie[0b0111] = 0.5, 0.25
    r = search(program, 4, 1.0, 0, 0, 5, [9], [(0, "*", 0, OK), (5, "*", 0.5, OK)] + [(9, f"{m:x}", e, OK) for m, e in tie.items()] + [(9, "*", 0.5, OK)])
    assert (r["mask"], r["mask_err"]) == (0b1110, 0.5)
    assert walks_restated(4, 1.0, {**tie, 15: 0.5})[0] == (3, 0b1110, 0.5)


def test_search_at_64_and_more_layers(program):
    # 64 layers, no layer can go: the mask is all ones, built without a shift by 64; every walk reuses the "alone" measurements
    rules = [(0, "*", 0, OK), (5, "*", 0.5, OK), (9, ALL, 0.5, OK), (9, "*", 2.0, OK)]
    r = search(program, 64, 1.0, 0, 0, 5, [9], rules)
    assert (r["rc"], r["chosen"], r["mask"], r["mask_err"]) == (OK, 9, (1 << 64) - 1, 0)
    assert r["calls"] == [(0, ALL), (5, ALL), (9, ALL)] + [(9, f"{((1 << 64) - 1) & ~(1 << li):x}") for li in range(64)]
    # ... and the last layer alone can: the walks drop bit 63
    rules = [(0, "*", 0, OK), (5, "*", 0.5, OK), (9, ALL, 0.5, OK), (9, f"{(1 << 63) - 1:x}", 0.75, OK), (9, "*", 2.0, OK)]
    r = search(program, 64, 1.0, 0, 0, 5, [9], rules)
    assert (r["mask"], r["mask_err"]) == ((1 << 63) - 1, 0.75)
    # more than 64 layers: whole depth
    r = search(program, 65, 1.0, 0, 0, 5, [9], rules)
    assert (r["chosen"], r["mask"], len(r["calls"])) == (9, (1 << 64) - 1, 3)


# ---- chunking -------------------------------------------------------------------------------------------------------------------
def aligned(n):
    return (n + ROW_ALIGN - 1) // ROW_ALIGN * ROW_ALIGN


def test_chunks_partition_every_batch(program):
    lengths, capacities = [0, 1, 63, 64, 65, 128, 129], [64, 128, 256]
    cases = [(cap, lens) for cap in capacities for n in range(1, 5) for lens in itertools.product(lengths, repeat=n)]
    answers = ask(program, [f"chunks {cap} {len(lens)} {' '.join(map(str, lens))}" for cap, lens in cases])
    for (chunk_rows, lens), line in zip(cases, answers):
        got = ints(line)
        cap, chunks = got[0], [tuple(got[i:i + 3]) for i in range(1, len(got), 3)]
        # capacity: the handle's chunk_rows, never below one aligned sequence of the longest length, never above the whole batch
        whole = aligned(min(sum(lens) + (ROW_ALIGN - 1) * len(lens), 1 << 30))
        assert cap == min(whole, max(chunk_rows, aligned(max(max(lens), 1)))) and cap >= min(whole, aligned(max(max(lens), 1))), (chunk_rows, lens)
        s0 = 0
        for s1, rows, longest in chunks:
            part = lens[s0:s1]
            assert s1 > s0, (chunk_rows, lens)  # at least one sequence, in order
            assert rows == sum(aligned(n) for n in part) and longest == max(part), (chunk_rows, lens)
            assert rows <= cap or len(part) == 1, (chunk_rows, lens)
            # greedy: the next sequence did not fit
            assert s1 == len(lens) or rows + aligned(lens[s1]) > cap, (chunk_rows, lens)
            s0 = s1
        assert s0 == len(lens), (chunk_rows, lens)
    # spot values, written out
    got = ask(program, ["chunks 64 3 65 1 63", "chunks 128 4 64 64 1 129", "chunks 256 1 0", "chunks 64 2 0 0"])
    assert [ints(line) for line in got] == [[96, 1, 96, 65, 3, 96, 63], [160, 3, 160, 64, 4, 160, 129], [32, 1, 0, 0], [64, 2, 0, 0]]


# ---- attention plan -------------------------------------------------------------------------------------------------------------
def test_attention_work_items_and_waves(program):
    f = _lib
    lists = {(1,): (1, 1), (0, 128, 129, 256, 257): (0 + 1 + 2 + 2 + 3, 0 + 1 + 1 + 1 + 2), (700, 5, 511): (6 + 1 + 4, 3 + 1 + 2), (2048,): (16, 8)}
    queries = [f"items {waves} {len(lens)} {' '.join(map(str, lens))}" for lens in lists for waves in (4, 8)]
    assert [int(v) for v in ask(program, queries)] == [n for pair in lists.values() for n in pair]

    def plan(lens, heads, cus, flags=0):
        return f"plan {heads} {cus} {flags} {len(lens)} {' '.join(map(str, lens))}"

    cases = [  # (query, waves_g, items_g, items_l)
        (plan((128, 100), 4, 256), 4, 2, 2),  # no sequence beyond 128 tokens: 128-query blocks
        (plan((129,) * 70, 4, 256), 8, 70, 140),  # 70 x 4 = 280 blocks > 256 CUs: 256-query blocks
        (plan((129,) * 64, 4, 256), 4, 128, 128),  # 64 x 4 = 256 <= 256: fewer items than CUs, back to 128-query blocks
        (plan((129,) * 64, 4, 255), 8, 64, 128),  # ... one CU fewer: 256 > 255
        (plan((129,) * 65, 4, 256), 8, 65, 130),
        (plan((129,) * 64, 4, 256, f.OP_FLAG_ATT_WAVES_8), 8, 64, 128),  # forced: no fallback
        (plan((2048,) * 64, 4, 256, f.OP_FLAG_ATT_WAVES_4), 4, 1024, 1024),
        (plan((5,), 4, 256, f.OP_FLAG_ATT_WAVES_8), 8, 1, 1),
        (plan((5,), 4, 256, f.OP_FLAG_ATT_WAVES_4 | f.OP_FLAG_ATT_WAVES_8), 4, 1, 1),  # (both: 4 wins)
    ]
    for (query, *want), line in zip(cases, ask(program, [c[0] for c in cases])):
        assert ints(line) == want, query


# ---- workspace layout -----------------------------------------------------------------------------------------------------------
COMMON = ["x", "ln_hi", "ln_lo", "q_hi", "q_lo", "k_hi", "k_lo", "vt_hi", "vt_lo", "o_hi", "o_lo", "h_hi", "h_lo", "row_seq", "row_pos",
          "row_tok", "roff", "qboff", "qboff_l", "cls", "range_flag"]
F32_PLANES = ["ln_f", "q_f", "k_f", "v_f", "o_f", "h_f"]


def regions(line):
    got = line.split()
    return int(got[0]), [(got[i], int(got[i + 1]), int(got[i + 2]), int(got[i + 3])) for i in range(1, len(got), 4)]


@pytest.mark.parametrize("model", ["row", "panel512", "tiled"])
def test_workspace_layout(program, model):
    hidden, inter = conf.MODELS[model][:2]
    rows, n_seqs = 768, 17
    (total, plain), (total_f32, with_f32) = (regions(line) for line in ask(program, [f"layout {hidden} {inter} {rows} {n_seqs} {f}" for f in (0, 1)]))
    assert [r[0] for r in plain] == COMMON and [r[0] for r in with_f32] == COMMON + F32_PLANES
    assert with_f32[:len(COMMON)] == plain  # the common regions do not move
    size = {"x": rows * hidden * 4, "h_hi": rows * inter * 2, "h_lo": rows * inter * 2, "row_seq": rows * 4, "row_pos": rows * 4, "row_tok": rows * 4,
            "roff": (n_seqs + 1) * 4, "qboff": (n_seqs + 1) * 4, "qboff_l": (n_seqs + 1) * 4, "cls": n_seqs * hidden * 4, "range_flag": 4,
            "h_f": rows * inter * 4, **{n: rows * hidden * 4 for n in F32_PLANES[:-1]}}
    index = {"row_seq", "row_pos", "row_tok", "roff", "qboff", "qboff_l"}
    end = 0
    for name, kind, offset, nbytes in with_f32:
        assert offset % 256 == 0 and offset == end, name  # 256-aligned, increasing, no gap and no overlap
        assert nbytes == size.get(name, rows * hidden * 2), name
        assert kind == (INDEX if name in index else FLAG if name == "range_flag" else FLOAT), name
        end = offset + (nbytes + 255) // 256 * 256
    assert end == total_f32 and plain[-1][2] + 256 == total
    # no sequence: the pooled rows keep one row
    assert dict((r[0], r[3]) for r in regions(ask(program, [f"layout {hidden} {inter} 256 0 0"])[0])[1])["cls"] == hidden * 4


# ---- cu_seqlens -----------------------------------------------------------------------------------------------------------------
def test_cu_seqlens_refusals(program):
    def cu(total, max_seqlen, max_pos, *values):
        return f"cu {total} {max_seqlen} {max_pos} {len(values) - 1} {' '.join(map(str, values))}"

    cases = [  # (query, code, message): each refusal on its smallest input
        (cu(1, 1, 8, 0, 1), OK, ""),
        (cu(0, 0, 8, 0), OK, ""),
        (cu(3, 2, 8, 0, 1, 1, 3), OK, ""),
        (cu(1, 1, 8, 1, 1), INVALID, "cu_seqlens must start at 0 and end at total_tokens (1): got 1..1"),
        (cu(1, 1, 8, 0, 2), INVALID, "cu_seqlens must start at 0 and end at total_tokens (1): got 0..2"),
        (cu(0, 1, 8, 0, 1, 0), INVALID, "cu_seqlens not monotone at 1"),
        (cu(2, 1, 8, 0, 2), INVALID, "sequence 0 has 2 tokens > max_seqlen 1"),
        (cu(3, 9, 2, 0, 0, 3), UNSUPPORTED, "sequence 1 has 3 tokens > max_position_embeddings 2"),
    ]
    for (query, code, message), line in zip(cases, ask(program, [c[0] for c in cases])):
        got_code, _, got_message = line.partition(" ")
        assert (int(got_code), got_message) == (code, message), query
