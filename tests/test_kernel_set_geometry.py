"""The axes tests/test_kernel_set_conformance.py holds fixed -- the batch's geometry, the layer pattern, the head -- swept under
the same statistic: every kernel set against the float64 model of its own arithmetic (tests/arith_model.py), entry by entry,
at 2 x RMS / 4 x max-abs of (model - exact), pooled over all rows of the batch (``conf._compare``, unchanged).

Contents: 52 distinct rows ``[cls] + random ids`` -- lengths 0 .. 40, 63, 64, 65, 129, 130, 257, 300 and a second row
("twin") of the lengths 7, 33, 64, 129.  The model runs once per (model, weights, set, layer pattern, head) on these rows;
a batch of any size is assembled from COPIES of contents and the model's entries for it by indexing
(``am.expand_entries``), so every row of a 2 600-row batch is compared with the model.  Hidden states travel packed
(``HiddenRequest()``, pad_width 0).

The swarm (``swarm_index``): 2 600 rows drawn from the contents with a fixed seed (97 % from the lengths 0 .. 40), about
60 k tokens, more than 1024 sequences in one chunk: the second and third pass of ``seq_offsets_kernel`` run and the binary
searches of ``row_map_kernel`` / ``attn_fp_kernel`` go through prefixes that carry a sum.  Forced placements:
  * the four longest contents at 0, 1023, 1024, 1025 and at the last index: the carry of the first pass is large and ragged;
  * an empty run at 2047 .. 2049, straddling the second pass boundary, between two long rows (2046, 2050); the run of the
    first boundary sits at 1020 .. 1022, right in front of the long rows, which hold 1023 .. 1025 themselves;
  * an empty row first-but-one and last-but-one;
  * twins side by side (equal lengths, other ids) at 100 / 101, 1500 / 1501 and 2200 / 2201;
  * no row equal in content to its neighbour, to the row 32 places away or to the row 1024 places away (two empty rows of
    one run excepted: an empty row has no entries but its zero ranking logits).  A sequence that takes a neighbour's rows,
    the rows of the work item 32 further, or those of the pass before, therefore differs from the model by O(1)
    (tests/test_geometry_inputs.py emulates these mistakes on the model's entries: each is > 10 x the bound).

Cases: the swarm in one chunk; the swarm in chunks (chunk_rows 4096: 27 chunks, s0 up to ~2 500; 256: the 257- and 300-token
rows exceed it and get a chunk of their own), every entry bit-identical to the one-chunk run (measured on all ten combinations,
so asserted: BIT_IDENTICAL; elsewhere the share is printed and the model's bound is the assertion); the layer patterns LGL, LLG, GGL, LLL on the contents (every fused launch that writes the next layer's q / k / v picks its
RoPE table from that layer's type); the head configurations (mean pooling, several labels, the pruning head in front of
final_norm).  keep_prob: against 1 / (1 + exp(l0 - l1)) in float64 on the kernel's own fp32 pruning logits.

The table of results is printed when the module ends, one line per comparison in the order they ran."""

from __future__ import annotations

import functools

import numpy as np
import pytest
import torch

import arith_model as am
import test_kernel_set_conformance as conf

pytestmark = pytest.mark.gpu

TWIN_LENGTHS = [7, 33, 64, 129]
CONTENT_LENGTHS = list(range(41)) + [63, 64, 65, 129, 130, 257, 300] + TWIN_LENGTHS
N_PLAIN = len(CONTENT_LENGTHS) - len(TWIN_LENGTHS)
TWIN_OF = {CONTENT_LENGTHS.index(n): N_PLAIN + i for i, n in enumerate(TWIN_LENGTHS)}  # content -> its twin
SWARM_ROWS = 2600
SCAN_PASS = 1024  # sequences per pass of seq_offsets_kernel
ITEM_GROUP = 32  # work items per group of the XCD-grouped attention block map
EMPTY = 0  # the content of length 0
LONGEST = [N_PLAIN - 1, N_PLAIN - 2, N_PLAIN - 3, N_PLAIN - 4]  # 300, 257, 130, 129 tokens
EMPTY_RUNS = [(1020, 1023), (2047, 2050)]
TWIN_PLACES = {100: 33, 1500: 64, 2200: 129}  # batch index -> length of the twins at (index, index + 1)
DISTANCES = (1, ITEM_GROUP, SCAN_PASS)

# keep_prob = 1 / (1 + expf(l0 - l1)) on fp32 logits: a value <= 1 from one fp32 subtraction, one expf, one add and one
# divide, each within 1 - 2 ulp
KEEP_PROB_BOUND = 8 * 2.0**-24

LAYER_PATTERNS = ["LGL", "LLG", "GGL", "LLL"]
# (pooling, labels, pruning head in front of final_norm)
HEADS = {"mean-3-post": ("mean", 3, False), "cls-2-pre": ("cls", 2, True), "mean-1-pre": ("mean", 1, True)}

# Sets per path: one per family of launches the axis reaches, not every set (the module's time is held to about 15 % of the
# suite's).  The batch's geometry enters through the row map, which every set shares, and through the attention kernels' work-item
# maps: the 3-term bf16 family (bf16x3, f16-f8-w) and the fp16 family (f16, f16-f8-w+attn-f16).  The next layer's RoPE table is
# picked on the row path by the two fused kernels of bf16x3, the whole-layer kernel (bf16-weights, f16-f8-w), the wave-pair kernel
# (f16) and the 32x32x16 whole-layer kernel (LAYER_M32); the panel and tiled layers pick their own layer's.
SWARM_CASES = ([("row", s, None) for s in ("bf16x3", "f16-f8-w", "f16")] + [("row", "f16", "ATTN_XCD_GROUP")]
               + [("panel512", s, None) for s in ("bf16x3", "f16", "f16-f8-w+attn-f16")] + [("tiled", "bf16x3", None)])
CHUNKED_CASES = [("row", "bf16x3"), ("row", "f16"), ("panel512", "bf16x3"), ("panel512", "f16-f8-w+attn-f16"), ("tiled", "bf16x3")]
CHUNK_ROWS = [4096, 256]
PATTERN_CASES = ([("row", s, None) for s in ("bf16x3", "bf16-weights", "f16-f8-w", "f16")] + [("row", "bf16-weights", "LAYER_M32")]
                 + [("panel512", s, None) for s in ("bf16x3", "f16-f8-w", "f16", "f16-f8-w+attn-f16")] + [("tiled3", "bf16x3", None)])
HEAD_CASES = ([("row", s, None) for s in ("bf16x3", "f16-f8-w", "f16")]
              + [("panel512", s, None) for s in ("bf16x3", "f16", "f16-f8-w+attn-f16")]
              + [("tiled", "bf16x3", None), ("row", "f16", "NO_HEAD_FUSION")])
# (model, set, chunk_rows) whose chunked run is bit-identical to the one-chunk run in every entry (hidden states, pruning and
# ranking logits): measured 100 % on all ten, asserted.  Such a run IS the run test_swarm_in_one_chunk compares with the model.  A
# combination taken off this list has its share printed and is compared with the model itself.
BIT_IDENTICAL = {(m, s, c) for m, s in CHUNKED_CASES for c in CHUNK_ROWS}
assert all((m, s, None) in SWARM_CASES for m, s in CHUNKED_CASES)

TABLE: list[str] = []


@pytest.fixture(scope="module", autouse=True)
def _print_table():
    yield
    print("\n[geometry] case     model     set                      flags              weights        | worst ratio to the bound ... "
          "(as [conformance]) | keep_prob: worst |kernel - float64| / bound | chunked: share of entries bit-identical to one chunk")
    for line in TABLE:
        print("[geometry]", line)


# -- contents and batches (no GPU: tests/test_geometry_inputs.py imports these) ---------------------------------------------------
@functools.lru_cache(maxsize=None)
def contents():
    return conf._rows(CONTENT_LENGTHS)


@functools.lru_cache(maxsize=None)
def swarm_index(n_rows: int = SWARM_ROWS, seed: int = 23) -> tuple:
    """Content index of every row of the swarm (module docstring)."""

    assert n_rows > 2 * SCAN_PASS + 2
    rng = np.random.default_rng(seed)
    short = [i for i, n in enumerate(CONTENT_LENGTHS) if n <= 40]
    long = [i for i, n in enumerate(CONTENT_LENGTHS) if n > 40]

    def draw():
        return int(rng.choice(long if rng.random() < 0.03 else short))

    idx = [draw() for _ in range(n_rows)]
    forced = {0: LONGEST[0], SCAN_PASS - 1: LONGEST[1], SCAN_PASS: LONGEST[2], SCAN_PASS + 1: LONGEST[3], n_rows - 1: LONGEST[1],
              2 * SCAN_PASS - 2: LONGEST[0], 2 * SCAN_PASS + 2: LONGEST[2], 1: EMPTY, n_rows - 2: EMPTY}
    for a, e in EMPTY_RUNS:
        forced.update({i: EMPTY for i in range(a, e)})
    for at, length in TWIN_PLACES.items():
        first = CONTENT_LENGTHS.index(length)
        forced.update({at: first, at + 1: TWIN_OF[first]})
    for i, c in forced.items():
        idx[i] = c

    def clashes(i):
        return any(0 <= j < n_rows and idx[j] == idx[i] for d in DISTANCES for j in (i - d, i + d))

    for i in range(n_rows):  # a redrawn row clashes with none of its six places, so one pass settles every free row
        while i not in forced and clashes(i):
            idx[i] = draw()
    return tuple(idx)


def equal_content_pairs(idx) -> list:
    """(i, j) with j - i in DISTANCES and the same content, two empty rows excepted."""

    return [(i, i + d) for d in DISTANCES for i in range(len(idx) - d) if idx[i] == idx[i + d] and idx[i] != EMPTY]


def batch_of(index):
    rows = contents()
    return [rows[c] for c in index]


ALL_CONTENTS = tuple(range(len(CONTENT_LENGTHS)))


# -- the CPU side -------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _content_backbone(model: str, weights: str, kernel_set: str, layer_types: "str | None" = None):
    """The layers of the model of `kernel_set` on the contents: no head configuration enters them."""

    torch.set_num_threads(16)
    path = conf.PATH_OF[model]
    return am.backbone(conf._state(model, weights), conf._dims(model, 128, layer_types=layer_types), contents(),
                       am.arith_for(kernel_set, path), path=path)


@functools.lru_cache(maxsize=None)
def content_model(model: str, weights: str, kernel_set: str, layer_types: "str | None" = None, pooling: "str | None" = None,
                  labels: "int | None" = None, pre_norm: bool = False):
    """Entries of the model of `kernel_set` ("exact" included) on the contents -- the layers once per module and (model,
    weights, set, layer pattern), the heads once per head configuration.  The label count changes the classifier's shape and
    no tensor of the layers (tests/test_geometry_inputs.py holds that)."""

    dims = conf._dims(model, 128, layer_types=layer_types, pooling=pooling, labels=labels)
    out = am.heads(conf._state(model, weights, 128, labels), dims, _content_backbone(model, weights, kernel_set, layer_types),
                   prune_pre_final_norm=pre_norm)
    return am.model_entries(out)


@functools.lru_cache(maxsize=2)
def _swarm_exact(model: str, weights: str):
    """(the exact model's entries of the swarm serve every set of a model: the last two are kept)"""

    return am.expand_entries(content_model(model, weights, "exact"), CONTENT_LENGTHS, swarm_index())


def models_for(model, kernel_set, index, **config):
    """(weights, own, exact, base or None): the entries of the batch `index` under the three models."""

    weights = conf.weights_for(kernel_set, "o1")
    base_set = am.BASE_SET.get(kernel_set)
    of = lambda s: am.expand_entries(content_model(model, weights, s, **config), CONTENT_LENGTHS, index)  # noqa: E731
    plain_swarm = index is swarm_index() and not any(config.values())
    return weights, of(kernel_set), _swarm_exact(model, weights) if plain_swarm else of("exact"), of(base_set) if base_set else None


# -- the GPU side -------------------------------------------------------------------------------------------------------------------
def _forward(enc, rows, keep: bool):
    """One forward with a packed hidden-state request: (prune [T, 2], rank [B, labels], hidden [N + 1, T, H], keep_prob [T] or
    None) on the device."""

    from open_provence_amd.engine import HiddenRequest
    from open_provence_amd.packing import pack_rows

    ids_np, cu_np, max_len = pack_rows(rows)
    ids = torch.from_numpy(ids_np).to(enc.device)
    cu = torch.from_numpy(cu_np).to(enc.device)
    kp = torch.full((int(cu_np[-1]),), float("nan"), dtype=torch.float32, device=enc.device) if keep else None
    prune, rank, hidden = enc.forward_packed(ids, cu, cu_np, max_len, keep_prob=kp, hidden=HiddenRequest())
    torch.cuda.synchronize()
    return prune, rank, hidden, kp


def _entries(outputs, lengths, label):
    """The comparison entries of one forward (packed: token order IS the entries' order); the ranking logits of empty rows must
    be exactly 0."""

    prune, rank, hidden, _ = outputs
    nonempty = torch.tensor([n > 0 for n in lengths], dtype=torch.bool)
    rank = rank.cpu()
    assert bool((rank[~nonempty] == 0).all()), f"{label}: ranking logits of an empty row are not 0"
    named = {f"hidden_{i}": hidden[i].cpu() for i in range(hidden.shape[0])}
    named["prune"] = prune.cpu()
    named["rank"] = rank[nonempty]
    return named


def _keep_prob_ratio(outputs, label):
    prune, _, _, kp = outputs
    l = prune.cpu().double()
    want = 1.0 / (1.0 + torch.exp(l[:, 0] - l[:, 1]))
    err = (kp.cpu().double() - want).abs()
    worst = float(err.max()) if err.numel() else 0.0
    assert worst == worst, f"{label}: keep_prob holds a NaN (a token it was not written for)"
    return worst / KEEP_PROB_BOUND


def _worst_row(got, own, exact, index):
    """Names the row that holds the worst element of the shallowest entry over its bound."""

    bnd = am.bounds(own, exact)
    first = am.first_over(am.ratios(got, own, bnd))
    if first is None:
        return ""
    lengths = [CONTENT_LENGTHS[c] for c in index]
    d = (got[first].double() - own[first]).abs()
    d = torch.nan_to_num(d, nan=float("inf")).reshape(d.shape[0], -1).amax(dim=1)
    at = int(d.argmax())
    if first == "rank":
        row = [b for b, n in enumerate(lengths) if n > 0][at]
        where = f"batch row {row}"
    else:
        cu = np.cumsum([0] + lengths)
        row = int(np.searchsorted(cu, at, side="right") - 1)
        where = f"token {at - int(cu[row])} of batch row {row}"
    return f"; worst element of {first}: {where} (content {index[row]}, {lengths[row]} tokens), |kernel - model| {float(d[at]):.3e}"


def _check(case, model, kernel_set, flag, index, *, chunk_rows=None, keep=False, layer_types=None, pooling=None, labels=None,
           pre_norm=False, against=None):
    """One forward of the batch `index` against the model.  `against`: the one-chunk outputs the share of bit-identical entries
    is counted against.  Returns the forward's device outputs."""

    config = dict(layer_types=layer_types, pooling=pooling, labels=labels, pre_norm=pre_norm)
    weights, own, exact, base = models_for(model, kernel_set, index, **config)
    rows = batch_of(index)
    lengths = [len(r) for r in rows]
    flags = [flag] if flag else []
    label = f"{case:8s} {model:9s} {kernel_set:24s} {'+'.join(flags) or '-':18s} {weights:14s}"
    dims = conf._dims(model, 128, layer_types=layer_types, pooling=pooling, labels=labels)
    enc = conf._encoder(model, weights, 128, kernel_set, conf._flag_bits(flags), chunk_rows=chunk_rows, prune_pre_final_norm=pre_norm,
                        dims=dims)
    try:
        outputs = _forward(enc, rows, keep)
        after = enc.effective_policy()["kernel_set"]
    finally:
        enc.close()
    assert after == kernel_set, f"{label}: the forward ran on {after}"
    got = _entries(outputs, lengths, label)
    n_before = len(conf.TABLE)
    try:
        conf._compare(label, got, own, exact, f"hidden_{conf.SHAPES[model][3]}", base)
    except (pytest.fail.Exception, AssertionError) as exc:
        pytest.fail(f"{exc}{_worst_row(got, own, exact, index)}")
    finally:
        line = conf.TABLE.pop() if len(conf.TABLE) > n_before else label  # (this module prints its own table)
        if keep:
            kp_ratio = _keep_prob_ratio(outputs, label)
            line += f" | keep_prob {kp_ratio:5.3f}"
        if against is not None:
            same = [int((a == b).sum()) for a, b in zip(outputs[:3], against[:3])]
            total = sum(int(a.numel()) for a in outputs[:3])
            line += f" | bit-identical to one chunk: {sum(same)} of {total} ({sum(same) / total:.4%})"
        TABLE.append(line)
        print("[geometry]", line)
    if keep:
        # one fp32 subtraction, one expf, one add, one divide (KEEP_PROB_BOUND)
        assert kp_ratio <= 1.0, f"{label}: keep_prob is {kp_ratio:.2f} x its bound of 8 x 2^-24 from sigmoid(l1 - l0) of its own logits"
    return outputs


# -- the swarm ------------------------------------------------------------------------------------------------------------------------
def test_the_swarm_crosses_two_scan_passes_in_one_chunk():
    idx = swarm_index()
    lengths = [CONTENT_LENGTHS[c] for c in idx]
    rows = sum((n + 31) // 32 * 32 for n in lengths)
    print(f"[geometry] swarm: {len(idx)} rows, {sum(lengths)} tokens, {rows} aligned rows, {sum(n == 0 for n in lengths)} empty")
    assert len(idx) > 2 * SCAN_PASS and rows < 262144  # one chunk under the default chunk_rows
    assert not equal_content_pairs(idx)


@pytest.mark.parametrize("model,kernel_set,flag", SWARM_CASES)
def test_swarm_in_one_chunk(model, kernel_set, flag):
    _check("swarm", model, kernel_set, flag, swarm_index(), keep=True)


@pytest.mark.parametrize("model,kernel_set", CHUNKED_CASES)
def test_swarm_in_chunks(model, kernel_set):
    """chunk_rows 4096: s0 > 0 in every chunk but the first (rank_out, cls and the hidden-state destinations are indexed through
    it); 256: the cap rule gives the 257- and 300-token rows a chunk of their own.  A chunked run that equals the one-chunk run
    bit for bit IS the run test_swarm_in_one_chunk compares with the model; one that does not is compared with the model here."""

    idx = swarm_index()
    rows = batch_of(idx)
    weights = conf.weights_for(kernel_set, "o1")

    def run(chunk_rows):
        enc = conf._encoder(model, weights, 128, kernel_set, 0, chunk_rows=chunk_rows)
        try:
            return _forward(enc, rows, False)
        finally:
            enc.close()

    whole = run(None)
    for chunk_rows in CHUNK_ROWS:
        chunked = run(chunk_rows)
        same = sum(int((a == b).sum()) for a, b in zip(chunked[:3], whole[:3]))
        total = sum(int(a.numel()) for a in whole[:3])
        if same == total:
            line = (f"{'chunk%d' % chunk_rows:8s} {model:9s} {kernel_set:24s} {'-':18s} {weights:14s} | bit-identical to one chunk: "
                    f"{same} of {total} (100%): the comparison with the model is test_swarm_in_one_chunk's")
            TABLE.append(line)
            print("[geometry]", line)
            continue
        del chunked
        assert (model, kernel_set, chunk_rows) not in BIT_IDENTICAL, f"chunk_rows {chunk_rows} changed {total - same} of {total} entries"
        _check(f"chunk{chunk_rows}", model, kernel_set, None, idx, chunk_rows=chunk_rows, against=whole)


# -- layer patterns -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pattern", LAYER_PATTERNS)
@pytest.mark.parametrize("model,kernel_set,flag", PATTERN_CASES)
def test_layer_pattern_matches_the_model(model, kernel_set, flag, pattern):
    _check(pattern, model, kernel_set, flag, ALL_CONTENTS, layer_types=pattern)


# -- head configurations --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("head", list(HEADS))
@pytest.mark.parametrize("model,kernel_set,flag", HEAD_CASES)
def test_head_configuration_matches_the_model(model, kernel_set, flag, head):
    pooling, labels, pre_norm = HEADS[head]
    _check(head, model, kernel_set, flag, ALL_CONTENTS, keep=True, pooling=pooling, labels=labels, pre_norm=pre_norm)
