"""The inputs of tests/test_kernel_set_geometry.py, on the CPU: the swarm has the placements it promises, and the bound that
module applies would see the mistakes it is there for.  Each mistake is emulated on the model's own entries and its worst ratio
to the bound (2 x RMS / 4 x max-abs of (model - exact), as ``conf._compare``) must be >= 10, under "bf16x3" and under "f16", on
the row and the panel512 model.

  * mis-mapped sequences of the swarm: every row from index 1024 on takes the outputs of the row 1024 earlier (the scan's
    carry lost), all rows shifted by one sequence, two adjacent rows of equal length swapped, an empty run collapsed (the rows
    behind it shifted).  A row that takes another row's outputs takes them token by token (the last token repeated where the
    source is shorter, zeros from an empty source): closer to the truth than a kernel's mistake would be.  Compared on the
    pruning head's input, the pruning logits and the ranking logits -- ``_compare`` takes the worst over more entries;
  * the RoPE table of a layer taken from the previous layer's type, per layer pattern (``am.forward(rope_is_global=...)``);
  * the head: mean over the row length rounded up to 32, mean that leaves out the last token, the pruning head on the wrong
    side of final_norm, the label rows of the classifier permuted.

An emulation that changes nothing (a pattern whose layers are all of one type, a permutation of one label) is listed in
UNCHANGED; one that stays under 10 x on some (model, set) in UNDETECTED with its measured ratio.  The test fails if either
list is wrong in either direction."""

from __future__ import annotations

import pytest
import torch

import arith_model as am
import test_kernel_set_conformance as conf
import test_kernel_set_geometry as geo

SENS_MODELS = ["row", "panel512"]
SENS_SETS = ["bf16x3", "f16"]
DETECTED = 10.0  # x the bound

# (kind, model, set, mutation) -> why the emulation changes no entry
UNCHANGED = {
    ("rope", m, s, p): "every layer is of one type: the previous layer's table is the layer's own"
    for m in SENS_MODELS for s in SENS_SETS for p in ("LLL", "GGG")
}
UNCHANGED.update({("head", m, s, "mean-1-pre: labels permuted"): "one label" for m in SENS_MODELS for s in SENS_SETS})
# (kind, model, set, mutation) -> (measured ratio, reason): under 10 x the bound
UNDETECTED: dict = {}


def _report(kind, model, kernel_set, found):
    """`found`: mutation -> worst ratio.  Prints them and holds them against the two lists."""

    low, same = {}, set()
    for name, r in found.items():
        note = "unchanged" if r == 0.0 else ("" if r >= DETECTED else "UNDER 10 x")
        print(f"[geometry sensitivity] {kind:5s} {model:9s} {kernel_set:8s} {name:44s} x{r:12.2f} of the bound {note}")
        if r == 0.0:
            same.add((kind, model, kernel_set, name))
        elif r < DETECTED:
            low[(kind, model, kernel_set, name)] = r
    mine = lambda table: {k for k in table if k[:3] == (kind, model, kernel_set)}  # noqa: E731
    assert same == mine(UNCHANGED), f"unchanged {sorted(same)}, listed {sorted(mine(UNCHANGED))}"
    assert set(low) == mine(UNDETECTED), f"under {DETECTED} x: {low}, listed {sorted(mine(UNDETECTED))}"


def _worst(got, own, bnd):
    return am.worst_ratio(got, own, bnd)[0]


# 1. the swarm's placements ---------------------------------------------------------------------------------------------------------
def test_contents_are_distinct_rows():
    rows = geo.contents()
    assert [len(r) for r in rows] == geo.CONTENT_LENGTHS and len(rows) == 52
    assert all(r[0] == 1 for r in rows if r)
    assert len({tuple(r) for r in rows}) == len(rows)
    for a, b in geo.TWIN_OF.items():
        assert len(rows[a]) == len(rows[b]) and rows[a] != rows[b]


def test_swarm_placements():
    idx = geo.swarm_index()
    n = len(idx)
    length = lambda i: geo.CONTENT_LENGTHS[idx[i]]  # noqa: E731
    assert n == geo.SWARM_ROWS == 2600 and n > 2 * geo.SCAN_PASS
    assert idx == geo.swarm_index() and set(idx) == set(range(len(geo.CONTENT_LENGTHS)))  # a fixed draw; every content occurs
    four = sorted(geo.CONTENT_LENGTHS)[-4:]
    assert sorted(length(i) for i in (0, 1023, 1024, 1025)) == four and length(n - 1) in four
    assert all(length(i) == 0 for i in (2047, 2048, 2049)) and length(2046) in four and length(2050) in four
    assert all(length(i) == 0 for i in (1020, 1021, 1022))  # (1023 .. 1025 hold the long rows)
    assert length(1) == 0 and length(n - 2) == 0
    for at, twin_len in geo.TWIN_PLACES.items():
        assert length(at) == length(at + 1) == twin_len and idx[at] != idx[at + 1]
    assert geo.equal_content_pairs(idx) == []
    both_empty = [(i, i + d) for d in geo.DISTANCES for i in range(n - d) if length(i) == 0 and length(i + d) == 0]
    assert both_empty == [(1020, 1021), (1021, 1022), (2047, 2048), (2048, 2049)]  # two empty rows meet inside the forced runs only
    tokens = sum(length(i) for i in range(n))
    print(f"[geometry sensitivity] swarm: {n} rows, {tokens} tokens")
    assert 50_000 <= tokens <= 70_000


def test_expanded_entries_are_the_entries_of_the_batch():
    """``am.expand_entries`` on the contents' entries == the model run on the assembled batch (rows do not see each other)."""

    torch.set_num_threads(16)
    index = [5, 0, 33, 33, 44, 0, 0, 51, 12]
    dims = conf._dims("row128", pooling="mean", labels=2)
    state = conf._state("row128", "o1", 128, 2)
    rows = geo.contents()
    content = am.model_entries(am.forward(state, dims, rows, "f16"))
    direct = am.model_entries(am.forward(state, dims, [rows[c] for c in index], "f16"))
    expanded = am.expand_entries(content, geo.CONTENT_LENGTHS, index)
    assert set(expanded) == set(direct)
    for name in direct:
        assert expanded[name].shape == direct[name].shape, name
        # (equal up to the batched matrix products' summation order)
        assert float((expanded[name] - direct[name]).abs().max()) <= 1e-12 * max(1.0, am.amax(direct[name])), name


def test_label_count_changes_no_tensor_of_the_layers():
    """``geo.content_model`` runs the layers once for every head configuration of a model."""

    for model in ("row", "panel512", "tiled"):
        one = conf._state(model, "o1")
        for labels in (2, 3):
            many = conf._state(model, "o1", 128, labels)
            differ = {k for k in one if one[k].shape != many[k].shape or not torch.equal(one[k], many[k])}
            assert set(one) == set(many) and all(k.split(".")[-2] == "classifier" and "pruning_head" not in k for k in differ), differ


def test_backbone_and_heads_are_the_forward():
    dims = conf._dims("row128", pooling="mean", labels=2)
    state = conf._state("row128", "o1", 128, 2)
    rows = geo.contents()[:36]
    whole = am.model_entries(am.forward(state, dims, rows, "f16", prune_pre_final_norm=True))
    parts = am.model_entries(am.heads(state, dims, am.backbone(state, dims, rows, "f16"), prune_pre_final_norm=True))
    assert all(torch.equal(whole[k], parts[k]) for k in whole)


# 2. mis-mapped sequences of the swarm ------------------------------------------------------------------------------------------------
def _take_rows(content, index, source):
    """The swarm's entries when batch row i leaves with the outputs of batch row source[i], token by token."""

    lens = geo.CONTENT_LENGTHS
    start = [0]
    for n in lens:
        start.append(start[-1] + n)
    tok, zero, rank_src = [], [], []
    slot, k = {}, 0
    for c, n in enumerate(lens):
        if n:
            slot[c], k = k, k + 1
    for i, c in enumerate(index):
        n, src = lens[c], index[source[i]]
        m = lens[src]
        for p in range(n):
            tok.append(start[src] + min(p, m - 1) if m else 0)
            zero.append(m == 0)
        if n:
            rank_src.append(slot.get(src, -1))
    tok, zero = torch.tensor(tok), torch.tensor(zero)
    rank_src = torch.tensor(rank_src)
    out = {}
    for name, t in content.items():
        if name == "rank":
            out[name] = torch.where((rank_src < 0)[:, None], torch.zeros((), dtype=t.dtype), t[rank_src.clamp(min=0)])
        else:
            out[name] = torch.where(zero[:, None], torch.zeros((), dtype=t.dtype), t[tok])
    return out


def _mis_mappings(idx):
    n = len(idx)
    ident = list(range(n))
    lost_carry = [i if i < geo.SCAN_PASS else i - geo.SCAN_PASS for i in ident]
    shifted = [(i + 1) % n for i in ident]
    at = min(geo.TWIN_PLACES)
    swapped = list(ident)
    swapped[at], swapped[at + 1] = at + 1, at
    a, e = geo.EMPTY_RUNS[0]
    collapsed = [i if i < a else min(i + (e - a), n - 1) for i in ident]
    return {"rows from 1024 on take the row 1024 earlier": lost_carry, "all rows shifted by one sequence": shifted,
            "two adjacent equal-length rows swapped": swapped, "an empty run collapsed": collapsed}


@pytest.mark.parametrize("kernel_set", SENS_SETS)
@pytest.mark.parametrize("model", SENS_MODELS)
def test_mis_mapped_sequences_exceed_the_bound(model, kernel_set):
    idx = geo.swarm_index()
    deepest = f"hidden_{conf.SHAPES[model][3]}"
    keep = (deepest, "prune", "rank")  # of the entries _compare pools; it takes the worst over more
    weights = conf.weights_for(kernel_set, "o1")
    own_c = {k: v for k, v in geo.content_model(model, weights, kernel_set).items() if k in keep}
    exact_c = {k: v for k, v in geo.content_model(model, weights, "exact").items() if k in keep}
    own = am.expand_entries(own_c, geo.CONTENT_LENGTHS, idx)
    bnd = am.bounds(own, am.expand_entries(exact_c, geo.CONTENT_LENGTHS, idx))
    same = _take_rows(own_c, idx, list(range(len(idx))))
    assert all(torch.equal(same[k], own[k]) for k in keep)  # the emulation with every row in its place is the model
    found = {name: _worst(_take_rows(own_c, idx, source), own, bnd) for name, source in _mis_mappings(idx).items()}
    _report("swarm", model, kernel_set, found)


# 3. the RoPE table of the previous layer's type ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("kernel_set", SENS_SETS)
@pytest.mark.parametrize("model", SENS_MODELS)
def test_rope_table_of_the_previous_layer_exceeds_the_bound(model, kernel_set):
    torch.set_num_threads(16)
    weights = conf.weights_for(kernel_set, "o1")
    path = conf.PATH_OF[model]
    found = {}
    for pattern in geo.LAYER_PATTERNS + ["GGG"]:
        own = geo.content_model(model, weights, kernel_set, pattern)
        bnd = am.bounds(own, geo.content_model(model, weights, "exact", pattern))
        is_global = [t == "G" for t in pattern]
        wrong = [is_global[0]] + is_global[:-1]  # layer li + 1 takes the table of layer li; layer 0 has no previous layer
        dims = conf._dims(model, 128, layer_types=pattern)
        mutant = am.forward(conf._state(model, weights), dims, geo.contents(), am.arith_for(kernel_set, path), path=path,
                            rope_is_global=wrong)
        found[pattern] = _worst(am.model_entries(mutant), own, bnd)
    _report("rope", model, kernel_set, found)


# 4. the head ---------------------------------------------------------------------------------------------------------------------------
def _head_mutations(model, weights, kernel_set, head):
    """name -> entries of the mutated model of one head configuration, on the contents."""

    pooling, labels, pre_norm = geo.HEADS[head]
    path = conf.PATH_OF[model]
    dims = conf._dims(model, 128, pooling=pooling, labels=labels)
    state = conf._state(model, weights, 128, labels)
    arith = am.arith_for(kernel_set, path)
    out = am.forward(state, dims, geo.contents(), arith, path=path, prune_pre_final_norm=pre_norm)
    own = am.model_entries(out)
    lengths = out.lengths
    pre = "ranking_model." if any(k.startswith("ranking_model.") for k in state) else ""
    last = [out.hidden[-1][b, :n] for b, n in enumerate(lengths)]
    if pre_norm:  # entry N is the raw last layer: the ranking head reads its final_norm
        last = [am._layer_norm(r, state[pre + "model.final_norm.weight"].double(), float(dims.norm_eps)) for r in last]
    nonempty = torch.tensor([n > 0 for n in lengths])
    with_rank = lambda rank: {**own, "rank": rank[nonempty]}  # noqa: E731
    assert torch.allclose(am.rank_logits(state, dims, last)[nonempty], own["rank"], rtol=0, atol=1e-12)
    mutants = {}
    if pooling == "mean":
        mutants["mean over the length rounded up to 32"] = with_rank(
            am.rank_logits(state, dims, last, pool=lambda r: r.sum(dim=0) / ((r.shape[0] + 31) // 32 * 32)))
        mutants["mean without the last token"] = with_rank(
            am.rank_logits(state, dims, last, pool=lambda r: r[: max(r.shape[0] - 1, 1)].mean(dim=0)))
    flipped = am.model_entries(am.forward(state, dims, geo.contents(), arith, path=path, prune_pre_final_norm=not pre_norm))
    mutants["pruning head on the wrong side of final_norm"] = {**own, "prune": flipped["prune"]}
    mutants["labels permuted"] = with_rank(am.rank_logits(state, dims, last)[:, list(range(1, labels)) + [0]])
    return own, mutants


@pytest.mark.parametrize("kernel_set", SENS_SETS)
@pytest.mark.parametrize("model", SENS_MODELS)
def test_head_mutations_exceed_the_bound(model, kernel_set):
    torch.set_num_threads(16)
    weights = conf.weights_for(kernel_set, "o1")
    found = {}
    for head, (pooling, labels, pre_norm) in geo.HEADS.items():
        own, mutants = _head_mutations(model, weights, kernel_set, head)
        exact = geo.content_model(model, weights, "exact", None, pooling, labels, pre_norm)
        bnd = am.bounds(own, exact)
        for name, entries in mutants.items():
            found[f"{head}: {name}"] = _worst(entries, own, bnd)
    _report("head", model, kernel_set, found)
