"""``process()`` / ``get_raw_predictions_batch`` with token-budgeted forwards (``OpenProvenceModel.forward_token_budget``,
``pipeline.plan_forward_chunks``) on the GPU: fewer, larger forwards, the planner's count of them, and results equal to
the fixed ``batch_size`` stride's with ``==`` -- a row's outputs do not depend on its companions in a launch."""

import math

import numpy as np
import pytest

from helpers import CharTokenizer, period_splitter

pytestmark = pytest.mark.gpu

N_CONTEXTS = 600
BATCH = 32


def _request(n_contexts, chars=470, seed=5):
    """1 query x n contexts of about ``chars`` characters (the generator of scripts/process_e2e.py)."""

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


def _model(weights):
    from open_provence_amd.config import OpenProvenceConfig
    from open_provence_amd.modeling import OpenProvenceModel
    from open_provence_amd.synthetic import named_dims, refinit_state_dict, synth_state_dict

    dims = named_dims("xsmall")
    cfg = OpenProvenceConfig(base_model_config=dims.to_base_model_config(), tokenizer_name_or_path="char-tokenizer",
                             pruning_config={"hidden_size": dims.hidden_size}, max_length=512, num_labels=1)
    state = refinit_state_dict(dims, seed=7) if weights == "refinit" else synth_state_dict(dims, 7)
    return OpenProvenceModel(cfg, device="cuda:0", tokenizer=CharTokenizer(), state_dict=state)


@pytest.fixture(scope="module")
def synth_model():
    return _model("synth")


@pytest.fixture(scope="module")
def refinit_model():
    return _model("refinit")


@pytest.fixture(autouse=True)
def _in_process(monkeypatch):
    monkeypatch.setenv("OPEN_PROVENCE_HOST_REPLICAS", "0")
    monkeypatch.delenv("OPEN_PROVENCE_FORWARD_TOKENS", raising=False)


class _Counted:
    """Counts the forwards of a model independently of its trace: wraps ``model.encoder.forward_packed``."""

    def __init__(self, model):
        self.model, self.lengths = model, []

    def __enter__(self):
        inner = self.inner = self.model.encoder.forward_packed

        def counted(ids, cu_seqlens, cu_seqlens_host, max_seqlen, *args, **kwargs):
            self.lengths.append(np.diff(np.asarray(cu_seqlens_host, dtype=np.int64)).tolist())
            return inner(ids, cu_seqlens, cu_seqlens_host, max_seqlen, *args, **kwargs)

        self.model.encoder.forward_packed = counted
        return self

    def __exit__(self, *_exc):
        del self.model.encoder.forward_packed  # (the instance attribute: the class's method is back)

    @property
    def launches(self):
        return len(self.lengths)

    @property
    def rows(self):
        return [n for launch in self.lengths for n in launch]


def _process(model, budget, contexts_and_question, **extra):
    question, contexts = contexts_and_question
    model.forward_token_budget = budget
    with _Counted(model) as counted:
        result = model.process(question, contexts, threshold=0.1, batch_size=BATCH, sentence_splitter=period_splitter,
                               show_progress=False, return_sentence_metrics=True, return_sentence_texts=True, **extra)
    return result, counted


def _assert_equal_results(got, want):
    assert set(got) == set(want)
    for key in want:
        if key not in ("timing", "performance_trace"):
            assert got[key] == want[key], key


def _round_budget(model):
    """One round of the chip, ``n_cus`` x 128 tokens: the budget these tests compare with budget 0.  The default is
    ``FORWARD_BUDGET_ROUNDS`` such rounds (one: profiles/process_token_budget.txt), which is checked here too."""

    import torch

    n_cus = int(torch.cuda.get_device_properties(model.device).multi_processor_count)
    model.forward_token_budget = None
    assert model.FORWARD_BUDGET_ROUNDS in (1, 2, 4) and model.forward_token_budget == model.FORWARD_BUDGET_ROUNDS * n_cus * 128
    assert model.round_token_budget() == n_cus * 128 and model.round_token_budget(4) == 4 * n_cus * 128
    return n_cus * 128


def _legacy_against_default(model, kernel_set):
    from open_provence_amd.pipeline import plan_forward_chunks

    request = _request(N_CONTEXTS)
    default = _round_budget(model)
    legacy, legacy_count = _process(model, 0, request, preprocess_batch_size=N_CONTEXTS)
    got, got_count = _process(model, default, request, preprocess_batch_size=N_CONTEXTS)
    assert legacy["performance_trace"].runtime["kernel_set"] == kernel_set == got["performance_trace"].runtime["kernel_set"]
    lengths = legacy_count.rows
    blocks = len(lengths)
    assert blocks >= N_CONTEXTS and got_count.rows == lengths
    print(f"[{kernel_set}] blocks={blocks} tokens={sum(lengths)} legacy launches={legacy_count.launches} "
          f"one-round budget={default} launches={got_count.launches}")
    assert legacy_count.launches == math.ceil(blocks / BATCH)
    assert got_count.launches == len(plan_forward_chunks(lengths, BATCH, default)) < legacy_count.launches
    for result, counted, budget in ((legacy, legacy_count, 0), (got, got_count, default)):
        assert result["performance_trace"].runtime["forwards"] == {
            "launches": counted.launches, "rows": blocks, "tokens": sum(lengths), "token_budget": budget}
        assert "forwards" not in result["timing"] and all(isinstance(v, (int, float)) for v in result["timing"].values())
    _assert_equal_results(got, legacy)
    return legacy, lengths


def test_one_round_budget_equals_the_fixed_stride_with_fewer_forwards(synth_model):
    _legacy_against_default(synth_model, "f16-f8-w")


def test_extreme_budgets(synth_model):
    from open_provence_amd.pipeline import plan_forward_chunks

    request = _request(N_CONTEXTS)
    legacy, legacy_count = _process(synth_model, 0, request, preprocess_batch_size=N_CONTEXTS)
    lengths = legacy_count.rows
    padded = sum(-(-n // 32) * 32 for n in lengths)
    whole, whole_count = _process(synth_model, padded, request, preprocess_batch_size=N_CONTEXTS)
    assert whole_count.launches == 1 and whole_count.rows == lengths
    small, small_count = _process(synth_model, 4096, request, preprocess_batch_size=N_CONTEXTS)
    assert small_count.launches == len(plan_forward_chunks(lengths, BATCH, 4096))
    _assert_equal_results(whole, legacy)
    _assert_equal_results(small, legacy)
    # the default granule (no explicit preprocess batch) is at most batch_size contexts -- here one row each --, and chunks
    # stay inside the granules: the stride's forwards, whatever the budget
    auto, auto_count = _process(synth_model, padded, request)
    assert auto_count.rows == lengths and auto_count.launches <= legacy_count.launches
    if len(lengths) == N_CONTEXTS:
        assert auto_count.lengths == legacy_count.lengths
    _assert_equal_results(auto, legacy)


def test_single_pass_fp16_set(refinit_model):
    """Reference-initialised weights calibrate to the single-pass fp16 set, whose launches differ most by size."""

    _legacy_against_default(refinit_model, "f16")


def test_get_raw_predictions_batch(synth_model):
    model = synth_model
    question, contexts = _request(200)
    blocks = [period_splitter(c) for c in contexts]
    outs = {}
    for label, budget in (("legacy", 0), ("default", _round_budget(model))):
        model.forward_token_budget = budget
        with _Counted(model) as counted:
            outs[label] = (model.get_raw_predictions_batch(question, blocks, batch_size=BATCH), counted.launches, counted.rows)
    (legacy, legacy_launches, legacy_rows), (got, got_launches, got_rows) = outs["legacy"], outs["default"]
    assert legacy_launches == math.ceil(200 / BATCH) > got_launches >= 1 and got_rows == legacy_rows
    assert len(got) == len(legacy) == 200
    for a, b in zip(got, legacy):
        assert a.ranking_score == b.ranking_score and a.context_ranges == b.context_ranges and a.contexts == b.contexts
        assert np.array_equal(a.pruning_probs, b.pruning_probs)


@pytest.mark.timeout(600)
def test_host_front_end_plans_with_the_owners_budget(synth_model, monkeypatch):
    """Two host-stage replicas: they plan their forwards with the owner's budget (carried in the spec they are built from),
    the owner merges what they submit.  The result equals the in-process call's; the owner enqueues no more forwards
    under the one-round budget than under budget 0 (each replica submits a half or less of the batches, and the owner
    never splits one)."""

    from open_provence_amd.frontend import HostFrontEnd

    monkeypatch.delenv("OPEN_PROVENCE_HOST_REPLICAS")
    model = synth_model
    question, contexts = request = _request(N_CONTEXTS)
    want, _ = _process(model, 0, request, preprocess_batch_size=N_CONTEXTS)
    call = dict(threshold=0.1, batch_size=BATCH, sentence_splitter=period_splitter, show_progress=False,
                return_sentence_metrics=True, return_sentence_texts=True, preprocess_batch_size=N_CONTEXTS)
    counts, batches = {}, {}
    for label, budget in (("legacy", 0), ("default", _round_budget(model))):
        model.forward_token_budget = budget
        with HostFrontEnd(model, workers=2) as front:
            front.process(question, contexts[:64], **call)  # (the replicas' first request pays their imports)
            with _Counted(model) as counted:
                got = front.process(question, contexts, **call)
            batches[label] = front.last_trace["batches"]  # forward batches the replicas submitted: their own plans
        _assert_equal_results(got, want)
        forwards = got["performance_trace"].runtime["forwards"]
        assert forwards["launches"] == counted.launches and forwards["rows"] == len(counted.rows) >= N_CONTEXTS
        assert forwards["token_budget"] == budget and got["timing"]["host_replicas"] == 2
        counts[label] = counted.launches
    print(f"owner launches: {counts} replica batches: {batches}")
    # the replicas planned with the owner's budget: fewer, larger batches than the stride's (deterministic: their plans)
    assert batches["default"] < batches["legacy"]
    assert 1 <= counts["default"] <= counts["legacy"]
