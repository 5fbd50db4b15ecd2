"""The pure pieces of a ``process()`` request (``pipeline.py``, ``request.py``) and of the launch layer (``launches.py``),
against values written out by hand from the rules they carry."""

from types import SimpleNamespace

import numpy as np
import pytest

from open_provence_amd import pipeline as pl
from open_provence_amd.launches import Launch, RemoteLaunch, flatten_segments, pack_launch, split_by_counts
from open_provence_amd.request import pipelining_granule

# two queries: the first with two contexts, the second with one
FULL = dict(
    pruned=[["a", "b"], ["c"]], scores=[[0.9, 0.1], [0.5]], rates=[[10.0, 20.0], [30.0]],
    kept=[[["k1"], ["k2"]], [["k3"]]], removed=[[["r1"], []], [["r3"]]], titles=[["t1", None], ["t3"]],
    probs=[[[0.1, 0.2], [0.3]], [[0.4]]],
)
# one query without contexts
EMPTY_FIRST = dict(pruned=[[]], scores=[[]], rates=[[]], kept=[[]], removed=[[]], titles=[[]], probs=[[]])


def _result(pruned, scores, rates, kept, removed, titles, probs):
    return pl.PostprocessResult(pruned, scores, rates, kept, removed, titles, probs)


SHAPED = {
    ("full", "nested"): tuple(FULL.values()),
    ("full", "str"): ("a", 0.9, 10.0, ["k1"], ["r1"], "t1", [0.1, 0.2]),
    ("full", "list"): (["a", "b"], [0.9, 0.1], [10.0, 20.0], [["k1"], ["k2"]], [["r1"], []], ["t1", None], [[0.1, 0.2], [0.3]]),
    ("full", "aligned"): (["a", "c"], [0.9, 0.5], [10.0, 30.0], [["k1"], ["k3"]], [["r1"], ["r3"]], ["t1", "t3"], [[0.1, 0.2], [0.4]]),
    ("empty", "nested"): ([[]], [[]], [[]], [[]], [[]], [[]], [[]]),
    ("empty", "str"): ("", None, 0.0, [], [], None, [[]]),
    ("empty", "list"): ([], [], [], [], [], [], []),
    ("empty", "aligned"): ([""], [None], [0.0], [[]], [[]], [None], [[]]),
}


@pytest.mark.parametrize("case,structure", sorted(SHAPED))
def test_outputs_take_the_shape_of_the_request(case, structure):
    fields = FULL if case == "full" else EMPTY_FIRST
    assert pl.shape_outputs(_result(**fields), structure) == SHAPED[(case, structure)]


@pytest.mark.parametrize("structure", ["str", "list", "aligned", "nested"])
def test_outputs_that_were_not_asked_for_stay_none_and_empty_probabilities_stay_empty(structure):
    shaped = pl.shape_outputs(_result(**dict(FULL, kept=None, removed=None, probs=None)), structure)
    assert shaped[:3] == SHAPED[("full", structure)][:3] and shaped[5] == SHAPED[("full", structure)][5]
    assert shaped[3] is None and shaped[4] is None and shaped[6] is None
    shaped = pl.shape_outputs(_result(**dict(FULL, probs=[])), structure)
    assert shaped[:6] == SHAPED[("full", structure)][:6] and shaped[6] == []
    # a result without queries keeps its lists, whatever the structure
    assert pl.shape_outputs(_result([], [], [], None, [], [], []), structure) == ([], [], [], None, [], [], [])


LOADER_CASES = [
    # (preprocess_workers, preprocess_batch_size, torch_dataloader_kwargs, environment) ->
    #     (workers, preprocess batch, prefetch, workers explicit, batch explicit, prefetch explicit); the host's default is 7
    ((None, None, None, None), (7, 32, None, False, False, False)),
    ((0, None, None, None), (0, 32, None, True, False, False)),
    ((3, None, None, None), (3, 32, None, True, False, False)),
    ((-2, None, None, None), (0, 32, None, True, False, False)),
    ((3, None, None, "2"), (3, 32, None, True, False, False)),
    ((None, None, None, "2"), (2, 32, None, True, False, False)),
    ((None, None, None, "0"), (7, 32, None, False, False, False)),
    ((None, None, None, "x"), (7, 32, None, False, False, False)),
    ((None, None, None, ""), (7, 32, None, False, False, False)),
    ((None, 64, None, None), (7, 64, None, False, True, False)),
    ((None, None, {}, None), (7, 32, None, False, False, False)),
    ((None, None, {"num_workers": 5}, None), (5, 32, None, True, False, False)),
    ((3, None, {"num_workers": "5"}, None), (5, 32, None, True, False, False)),
    ((None, None, {"batch_size": 16}, None), (7, 16, None, False, True, False)),
    ((None, 64, {"batch_size": 16, "pin_memory": True}, None), (7, 16, None, False, True, False)),
    ((None, None, {"prefetch_factor": 4}, None), (7, 32, 4, False, False, True)),
    ((None, None, {"prefetch_factor": "4"}, None), (7, 32, 4, False, False, True)),
    ((None, None, {"prefetch_factor": "x"}, None), (7, 32, None, False, False, True)),
    ((None, None, {"prefetch_factor": None}, None), (7, 32, None, False, False, True)),
]


@pytest.mark.parametrize("given,expected", LOADER_CASES)
def test_loader_settings(monkeypatch, given, expected):
    monkeypatch.setattr(pl, "default_preprocess_workers", lambda: 7)
    workers, batch, loader_kwargs, env = given
    assert tuple(pl.loader_settings(workers, batch, 32, loader_kwargs, env)) == expected


def test_token_ranges_are_flattened_to_batch_positions_and_cut_back_by_counts():
    cu = np.asarray([0, 10, 14, 30], dtype=np.int32)
    # a row with two ranges, one with none, one with an empty range, a reversed one and the whole row
    segments = [[(1, 4), (4, 9)], [], [(5, 5), (7, 3), (0, 16)]]
    flat, counts = flatten_segments(cu, segments)
    assert flat.dtype == np.int32 and flat.tolist() == [1, 4, 4, 9, 19, 19, 21, 21, 14, 30]
    assert counts == [2, 0, 3]
    values = [0.5, 1.5, 2.5, 3.5, 4.5]
    assert split_by_counts(values, counts) == [[0.5, 1.5], [], [2.5, 3.5, 4.5]]
    assert [len(part) for part in split_by_counts(values, counts)] == counts
    as_array = split_by_counts(np.asarray(values, dtype=np.float32), counts)
    assert [part.tolist() for part in as_array] == [[0.5, 1.5], [], [2.5, 3.5, 4.5]]
    assert split_by_counts([], []) == [] and flatten_segments(cu[:1], [])[0].size == 0

    ids, cu_packed, max_len, seg_flat, seg_counts = pack_launch([[7] * 10, [8] * 4, [9] * 16], segments)
    assert cu_packed.tolist() == cu.tolist() and max_len == 16 and ids.tolist() == [7] * 10 + [8] * 4 + [9] * 16
    assert seg_flat.tolist() == flat.tolist() and seg_counts == counts
    assert pack_launch([[7] * 10, [8] * 4], None)[3:] == (None, None)


def test_an_empty_launch_has_every_field_of_a_launch():
    cu = np.zeros(1, dtype=np.int32)
    populated = Launch(event=object(), pool={"keep_np": np.zeros(3, np.float32), "rank_np": np.zeros(1, np.float32)}, total=3, rows=1,
                       cu=np.asarray([0, 3], dtype=np.int32), seg_counts=[2], alive=(), retry=(None,) * 5, f8=True, slot=1, ids_dev=None)
    for reduced, seg_counts in ((True, []), (False, None)):
        empty = Launch.empty(cu, reduced)
        assert set(vars(empty)) == set(vars(populated))
        assert (empty.event, empty.pool, empty.total, empty.rows, empty.seg_counts) == (None, None, 0, 0, seg_counts)
        assert empty.cu is cu and empty.alive is None and empty.shard is None and empty.retry is None and not empty.f8
    remote = RemoteLaunch(remote=None, rows=1, cu=populated.cu, seg_counts=[2])
    assert set(vars(remote)) - {"remote"} <= set(vars(populated))


def test_the_small_rules_of_a_request():
    assert [pl.max_fragment_tokens(n, whole) for n, whole in ((512, False), (512, True), (20, False), (17, True), (8192, False))] \
        == [256, 510, 16, 16, 4096]
    assert pl.empty_stage_timing() == {"sentence_collect_seconds": 0.0, "sentence_normalize_seconds": 0.0, "tokenize_seconds": 0.0,
                                       "fragment_split_seconds": 0.0, "fragment_decode_seconds": 0.0}
    assert pl.empty_stage_timing() is not pl.empty_stage_timing()
    block = [pl.FragmentRecord("One. ", 0, 0, 0, 2, [5, 6]), pl.FragmentRecord("Two.", 1, 0, 1, 1, [7])]
    assert pl.inference_job(2, 3, 1, block) == {"query_idx": 2, "context_idx": 3, "block_idx": 1, "texts": ["One. ", "Two."]}
    job = {"sentences": ["T. ", "One. ", "Two."], "prefix_sentences": ["T. "], "prefix_token_counts": [2], "title_is_first_sentence": True,
           "context_text": "One. Two.", "query_idx": 0, "context_idx": 0, "token_lists": [[4, 4], [5, 6], [7]]}
    want = pl.ContextState(sentences=["T. ", "One. ", "Two."], fragments=block, blocks=[block], prefix_length=1, prefix_sentences=["T. "],
                           prefix_token_counts=[2], title_is_first_sentence=True, original_text="One. Two.")
    for source in (job, SimpleNamespace(**job)):
        state = pl.context_state(source, block, [block])
        assert state == want and state.raw_blocks == [] and state.sentences is not job["sentences"]

    class Tokenizer:
        def encode(self, text, add_special_tokens=True):
            assert add_special_tokens is False
            return np.asarray([ord(c) for c in text], dtype=np.int64)

    ids = pl.tokenize_query(Tokenizer(), "ab?")
    assert ids == [97, 98, 63] and all(type(t) is int for t in ids)
    # contexts per granule of the pipelined job loop: 16 x ceil(3.2 sqrt(N) / 16), at least 32, within the preprocess batch; a
    # remainder of less than half a granule gets no launch of its own
    assert [pipelining_granule(n, batch) for n, batch in ((256, 96), (1024, 192), (4096, 192), (90, 90), (40, 40), (48, 32), (49, 32), (3, 3))] \
        == [64, 112, 192, 32, 40, 48, 32, 3]
