"""forward() under ANY attention mask on the handle's SELECTED kernel set: ``op_forward_masked_native`` (row and panel path).

The reference is the fp64 CPU oracle with the mask.  The yardstick is the set's own arithmetic: per compared quantity
(tests/masked_model.py: ``logits``, ``keep_prob``), ``e_set`` = the distance of the same set's PACKED forward -- code the masked
route does not touch -- to the fp64 oracle on ``prefix_batch(width)`` of the same model, measured here; the bound is

    max(4 x e_set, 16 ulp of the quantity's largest magnitude)

the form and the factor of ``masked_model.Reference.bound``, for the same reason: other rows, another count of keys per query.
Every kernel set the handle can pin except "fp32" (whose masked forward is ``op_forward_masked``), ``calibrate=False``.

Models (head dim 64, 3 layers, vocab 512): two on the row path, two on the panel path -- both layer patterns, both windows,
both poolings.  Masks and widths: ``masked_model.batch`` (200: crosses the 64-key tile and the 128-row block; 77; 1).

Then: a prefix mask gives the BITS of the packed forward under a pinned attention plan; each mistake of
``masked_model.MUTATIONS`` would be seen; independence of batch, chunking, stream and workspace content; refusals; forward().
With ``MASKED_NATIVE_CONFORMANCE_OUT`` set, the worst ratios per (model, set) are also written to that file
(profiles/masked_native_conformance.txt is such a run)."""

from __future__ import annotations

import ctypes
import functools
import os
import warnings

import numpy as np
import pytest
import torch

import masked_model as mm
import workspace_utils as wu
from helpers import CharTokenizer

pytestmark = pytest.mark.gpu

# (name, hidden, heads, intermediate, pattern, window, pooling, labels, prune_pre_final_norm, weights)
MODELS = [
    ("row-h128-GLL-w16-cls1-refinit", 128, 2, 192, "GLL", 16, "cls", 1, False, "refinit"),
    ("row-h256-LGL-w128-mean2-pre-synth", 256, 4, 256, "LGL", 128, "mean", 2, True, "synth"),
    ("panel-h512-GLL-w16-mean2-synth", 512, 8, 256, "GLL", 16, "mean", 2, False, "synth"),
    ("panel-h512-LGL-w128-cls1-synth", 512, 8, 256, "LGL", 128, "cls", 1, False, "synth"),
]
WIDTHS = mm.WIDTHS
QUANTITIES = ("logits", "keep_prob")


def _dims(model, max_positions=2048):
    from open_provence_amd.config import EncoderDims

    _, hidden, heads, inter, pattern, window, pooling, labels, _, _ = model
    cfg = dict(model_type="modernbert", vocab_size=512, hidden_size=hidden, intermediate_size=inter, num_hidden_layers=3,
               num_attention_heads=heads, local_attention=window, global_attn_every_n_layers=3, global_rope_theta=160000.0,
               local_rope_theta=10000.0, max_position_embeddings=max_positions, pad_token_id=0, cls_token_id=1, sep_token_id=2,
               layer_types=["full_attention" if t == "G" else "sliding_attention" for t in pattern], classifier_pooling=pooling)
    return EncoderDims.from_base_model_config(cfg, num_labels=labels)


@functools.lru_cache(maxsize=None)
def _state(model):
    from open_provence_amd.synthetic import refinit_state_dict, synth_state_dict

    return (refinit_state_dict if model[9] == "refinit" else synth_state_dict)(_dims(model), 5)


def _encoder(model, *, masked_kernels="selected", attention_masks="any", kernel_set=None, state=None, **kw):
    from open_provence_amd.engine import HipEncoder

    enc = HipEncoder(_dims(model), device="cuda:0", attention_masks=attention_masks, masked_kernels=masked_kernels,
                     prune_pre_final_norm=model[8], kernel_set="fp32" if kernel_set == "fp32" else None, **kw)
    try:
        enc.load_state_dict(state or _state(model), calibrate=False, kernel_set=kernel_set)
    except BaseException:
        enc.close()
        raise
    return enc


def _sets(enc):
    import attention_utils as au

    return [name for name in au.selectable_sets(enc) if name != "fp32"]


def _packed(enc, ids, mask):
    """forward_packed of a right-padded batch -> (prune[T, 2], rank) on the device."""

    from open_provence_amd.packing import pack_padded

    ids_np, cu_np, max_len = pack_padded(ids, mask)
    prune, rank = enc.forward_packed(torch.from_numpy(ids_np).cuda(), torch.from_numpy(cu_np).cuda(), cu_np, max_len)[:2]
    return prune, rank


@functools.lru_cache(maxsize=None)
def _oracle(model, width, prefix):
    """The fp64 oracle's compared quantities of ``batch(width)`` (``prefix``: of ``prefix_batch(width)``), computed once."""

    from oracle.modernbert_oracle import oracle_forward

    torch.set_num_threads(16)
    ids, mask = mm.prefix_batch(width) if prefix else mm.batch(width)[:2]
    out = oracle_forward(_state(model), _dims(model), ids, mask, dtype=torch.float64, prune_pre_final_norm=model[8])
    return mm.compared(out.pruning_logits, out.ranking_logits, mask)


def _compared_packed(prune, rank):
    """masked_model.compared of a packed forward's outputs (every row has a token: prune[mask == 1] is the packed order)."""

    return {"logits": torch.cat([prune.double().flatten(), rank.double().flatten()]), "keep_prob": torch.softmax(prune.double(), dim=-1)[:, 1]}


def _distance(got, want):
    out = {}
    for name in QUANTITIES:
        assert got[name].shape == want[name].shape, name
        out[name] = float((got[name] - want[name]).abs().max()) if want[name].numel() else 0.0
    return out


def _bound(e_set, want, name):
    top = float(want[name].abs().max()) if want[name].numel() else 0.0
    return max(4.0 * e_set[name], 16.0 * float(np.spacing(np.float32(top))))


def _zeros_where_masked(label, prune, rank, mask):
    prune, rank, on = prune.cpu(), rank.cpu(), mask.bool()
    assert prune.shape == tuple(mask.shape) + (2,) and prune.dtype == torch.float32 and rank.shape[0] == mask.shape[0]
    assert bool((prune[~on].view(torch.int32) == 0).all()), f"{label}: a pruning logit at mask == 0 is not +0.0"
    assert bool((rank[~on.any(1)].view(torch.int32) == 0).all()), f"{label}: the ranking logits of an all-zero row are not +0.0"


# -- test 1: against the oracle, every (model, set, width) ---------------------------------------------------------------------------
WORST: "dict[tuple[str, str], dict]" = {}


@functools.lru_cache(maxsize=None)
def _measure(model, width):
    """-> {set: {quantity: (err, e_set, bound)}} of one (model, width): one handle, every selectable set."""

    ids, mask, _ = mm.batch(width)
    pids, pmask = mm.prefix_batch(width)
    want, pwant = _oracle(model, width, False), _oracle(model, width, True)
    enc = _encoder(model)
    out = {}
    try:
        assert not enc.attention_outputs  # (no fp32 packs on the mask's account)
        for name in _sets(enc):
            enc.select_kernel_set(name)
            pprune, prank = _packed(enc, pids, pmask)
            e_set = _distance(_compared_packed(pprune.cpu(), prank.cpu()), pwant)
            prune, rank = enc.forward_masked(ids, mask)
            torch.cuda.synchronize()
            label = f"{model[0]} {name} L{width}"
            assert enc.effective_policy()["kernel_set"] == name, f"{label}: the range guard left the set"
            _zeros_where_masked(label, prune, rank, mask)
            got = mm.compared(prune.cpu(), rank.cpu(), mask)
            assert all(bool(torch.isfinite(got[q]).all()) for q in QUANTITIES), f"{label}: not finite"
            err = _distance(got, want)
            out[name] = {q: (err[q], e_set[q], _bound(e_set, want, q)) for q in QUANTITIES}
            for q in QUANTITIES:
                e, es, b = out[name][q]
                print(f"[masked-native] {label:64s} {q:10s} err {e:.3e}  e_set {es:.3e}  err/e_set {e / max(es, 1e-30):7.2f}  bound {b:.3e}")
                worst = WORST.setdefault((model[0], name), {"err/e_set": 0.0, "err/bound": 0.0, "where": ""})
                if e / b >= worst["err/bound"]:
                    worst.update({"err/e_set": e / max(es, 1e-30), "err/bound": e / b, "where": f"L{width} {q}"})
    finally:
        enc.close()
    return out


@pytest.mark.parametrize("width", WIDTHS, ids=lambda w: f"L{w}")
@pytest.mark.parametrize("model", MODELS, ids=lambda m: m[0])
def test_every_set_matches_the_oracle_within_its_own_error(model, width):
    measured = _measure(model, width)
    assert len(measured) >= 4, sorted(measured)
    for name, per in measured.items():
        for q, (err, e_set, bound) in per.items():
            assert err <= bound, f"{model[0]} {name} L{width}: {q} is {err:.3e} from the fp64 oracle, bound {bound:.3e} (e_set {e_set:.3e})"


# -- test 2: prefix masks give the bits of the packed forward ------------------------------------------------------------------------------
@pytest.mark.parametrize("waves", (4, 8), ids=lambda w: f"waves{w}")
@pytest.mark.parametrize("model", MODELS, ids=lambda m: m[0])
def test_a_prefix_mask_gives_the_bits_of_the_packed_forward(model, waves):
    """The attention plan reads the row lengths (dense rows are longer than packed ones), so it is pinned alike on both."""

    from open_provence_amd import _lib

    ids, mask = mm.prefix_batch(200)
    on = mask.bool().cuda()
    enc = _encoder(model, flags=_lib.OP_FLAG_ATT_WAVES_4 if waves == 4 else _lib.OP_FLAG_ATT_WAVES_8)
    try:
        for name in _sets(enc):
            enc.select_kernel_set(name)
            want_prune, want_rank = _packed(enc, ids, mask)
            prune, rank = enc.forward_masked(ids, mask)
            torch.cuda.synchronize()
            assert torch.equal(prune[on], want_prune), f"{name}: pruning logits at valid positions"
            assert torch.equal(rank, want_rank), f"{name}: ranking logits"
            assert bool((prune[~on].view(torch.int32) == 0).all()), f"{name}: a pruning logit at mask == 0 is not +0.0"
    finally:
        enc.close()


# -- test 3: the mask rules are visible -------------------------------------------------------------------------------------------------------
# the rows of batch(200) a mutation is looked for in (the restatement walks query by query: the whole batch would take minutes)
MUTATION_ROWS = ("left-padded to 17", "left-padded to 64", "left-padded to 129", "random holes 0", "hole over columns 64..127")


@functools.lru_cache(maxsize=None)
def _mutation_rows(model):
    """-> (ids, mask, the fp64 oracle's compared quantities) of MUTATION_ROWS."""

    from oracle.modernbert_oracle import oracle_forward

    torch.set_num_threads(16)
    ids, mask, names = mm.batch(200)
    pick = [names.index(n) for n in MUTATION_ROWS]
    ids, mask = ids[pick], mask[pick]
    out = oracle_forward(_state(model), _dims(model), ids, mask, dtype=torch.float64, prune_pre_final_norm=model[8])
    return ids, mask, mm.compared(out.pruning_logits, out.ranking_logits, mask)


@pytest.mark.parametrize("mutation", mm.MUTATIONS)
def test_each_mutation_of_the_mask_rules_would_be_seen(mutation):
    """Each mistake, applied to masked_model.masked_forward in float64, must move a compared quantity of some model's batch(200)
    by more than 2 x that case's bound of test 1 (a row's shift is the batch's): asserted for "bf16x3" -- the masking code is one
    template for all sets --, printed for every set."""

    shifts = {}
    for model in MODELS:
        ids, mask, want = _mutation_rows(model)
        prune, rank = mm.masked_forward(_state(model), _dims(model), ids, mask, prune_pre_final_norm=model[8], mutation=mutation)
        shifts[model] = _distance(mm.compared(*mm.project_outputs(prune, rank, mask), mask), want)
    seen = {}
    for name in sorted({name for model in MODELS for name in _measure(model, 200)}):
        per_model = [(model, _measure(model, 200)[name]) for model in MODELS if name in _measure(model, 200)]
        seen[name] = max(shifts[model][q] / per[q][2] for model, per in per_model for q in QUANTITIES)
        print(f"[masked-native] mutation {mutation:24s} {name:24s} moves a quantity by {seen[name]:12.1f} x its bound")
    assert seen["bf16x3"] > 2.0, f"{mutation} hides on bf16x3: {seen['bf16x3']:.2f} x the bound"


# -- test 4: independence and refusals ----------------------------------------------------------------------------------------------------------
def _two_sets(enc):
    names = _sets(enc)
    return [n for n in ("bf16x3", "f16") if n in names] + [n for n in names if "f8" in n][:1]


@pytest.mark.parametrize("model", [MODELS[1], MODELS[2]], ids=lambda m: m[0])
def test_a_row_alone_equals_the_row_in_the_batch_and_chunking_changes_nothing(model):
    ids, mask, names = mm.batch(200)
    enc = _encoder(model)
    chunked = _encoder(model, chunk_rows=256)  # (one dense row of 200 positions per chunk)
    try:
        for name in _two_sets(enc):
            enc.select_kernel_set(name)
            chunked.select_kernel_set(name)
            prune, rank = enc.forward_masked(ids, mask)
            prune_c, rank_c = chunked.forward_masked(ids, mask)
            assert torch.equal(prune, prune_c) and torch.equal(rank, rank_c), f"{name}: chunk_rows = 256 changes the bits"
            for s in range(0, len(names), 3):
                p1, r1 = enc.forward_masked(ids[s: s + 1], mask[s: s + 1])
                assert torch.equal(p1[0], prune[s]) and torch.equal(r1[0], rank[s]), f"{name}: row {s} ({names[s]})"
    finally:
        enc.close()
        chunked.close()


def test_two_streams_give_the_same_bits():
    model = MODELS[3]
    ids, mask, _ = mm.batch(200)
    enc = _encoder(model)
    try:
        want = enc.forward_masked(ids, mask)
        torch.cuda.synchronize()
        need = int(enc.lib.op_masked_native_workspace_bytes(enc._handle, *ids.shape)) + 256
        streams = [torch.cuda.Stream(), torch.cuda.Stream()]
        spaces = [torch.empty(need, dtype=torch.uint8, device="cuda:0") for _ in streams]
        outs = []
        ids_d, mask_d = ids.cuda(), mask.cuda()
        torch.cuda.synchronize()
        for stream, space in zip(streams, spaces):
            with torch.cuda.stream(stream):
                outs.append(enc.forward_masked(ids_d, mask_d, workspace=space))
        torch.cuda.synchronize()
        for got in outs:
            assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    finally:
        enc.close()


def _direct(enc, ids, mask, fill):
    """op_forward_masked_native itself on a workspace of exactly op_masked_native_workspace_bytes and on outputs that are views
    between canaries.  ``fill``: zeros, or a poison per region kind (the rule of workspace_utils: float planes NaN / huge bytes,
    index regions a wrong but in-range entry).  The call's own regions come first -- cu_seqlens (an index region), the id check's
    word, key_row, vmean -- then the selected set's forward workspace, whose regions the handle reports."""

    from open_provence_amd import _lib

    n_rows, width = (int(v) for v in ids.shape)
    nl = enc.dims.num_labels
    need = int(enc.lib.op_masked_native_workspace_bytes(enc._handle, n_rows, width))
    forward_need = int(enc.lib.op_workspace_bytes(enc._handle, n_rows, n_rows * width, width))
    head = need - forward_need
    assert need % 256 == 0 and head >= 256 * 4
    mem = wu.canaried(need, enc.device)
    mem.view.zero_()
    if fill != "zeros":
        cu_bytes = ((n_rows + 1) * 4 + 255) // 256 * 256
        mem.view[:cu_bytes].view(torch.int32).fill_(1)
        mem.view[cu_bytes: head].fill_(wu.NAN_BYTE if fill == "nan" else wu.HUGE_BYTE)
        sub = wu.ControlledWorkspace(wu.Canaried(mem.backing, mem.view[head:], mem.guard, mem.canary), forward_need,
                                     enc.workspace_layout(n_rows, n_rows * width, width), 1)
        wu.fill_workspace(sub, fill)
    bufs = {"prune": wu.canaried(n_rows * width * 2 * 4, enc.device), "rank": wu.canaried(n_rows * nl * 4, enc.device)}
    ids_d, mask_d = ids.to(torch.int32).cuda().contiguous(), mask.ne(0).cuda().contiguous().view(torch.uint8)
    ids_guard, mask_guard = ids_d.clone(), mask_d.clone()
    report = _lib.OpMaskedReport()
    report.struct_bytes = ctypes.sizeof(_lib.OpMaskedReport)
    vp = ctypes.c_void_p
    with torch.cuda.device(enc.device):
        code = enc.lib.op_forward_masked_native(enc._handle, vp(ids_d.data_ptr()), vp(mask_d.data_ptr()), n_rows, width,
                                                vp(mem.view.data_ptr()), ctypes.c_size_t(need), vp(bufs["prune"].view.data_ptr()),
                                                vp(bufs["rank"].view.data_ptr()), ctypes.byref(report),
                                                vp(torch.cuda.current_stream(enc.device).cuda_stream))
    _lib.check(enc.lib, enc._handle, code, "op_forward_masked_native")
    torch.cuda.synchronize()
    mem.assert_intact(f"fill {fill!r}: workspace")
    for name, buf in bufs.items():
        buf.assert_intact(f"fill {fill!r}: {name}")
    assert torch.equal(ids_d, ids_guard) and torch.equal(mask_d, mask_guard)
    return bufs["prune"].view.view(torch.float32).view(n_rows, width, 2).clone(), bufs["rank"].view.view(torch.float32).view(n_rows, nl).clone()


@pytest.mark.parametrize("model", [MODELS[0], MODELS[1], MODELS[2]], ids=lambda m: m[0])
def test_outputs_do_not_depend_on_what_the_workspace_held(model):
    ids, mask, _ = mm.batch(200)
    enc = _encoder(model)
    try:
        for name in _two_sets(enc):
            enc.select_kernel_set(name)
            want = _direct(enc, ids, mask, "zeros")
            again = enc.forward_masked(ids, mask)
            assert torch.equal(again[0], want[0]) and torch.equal(again[1], want[1]), name
            for fill in wu.POISONS:
                got = _direct(enc, ids, mask, fill)
                assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]), f"{name}: fill {fill!r} reaches an output"
    finally:
        enc.close()


def test_an_id_outside_the_table_raises_wherever_it_sits():
    model = MODELS[0]
    ids, mask, names = mm.batch(200)
    enc = _encoder(model)
    try:
        want = enc.forward_masked(ids, mask)
        row = names.index("left-padded to 64")
        for col in (0, 199):  # under a zero of the mask, and at a valid position
            for value in (512, -1):
                bad = ids.clone()
                bad[row, col] = value
                for to in (lambda t: t, lambda t: t.cuda()):
                    with pytest.raises(IndexError, match=f"row {row}, column {col}") as info:
                        enc.forward_masked(to(bad), to(mask))
                    assert str(value) in str(info.value)
        again = enc.forward_masked(ids, mask)  # the handle is usable after the refusals
        assert torch.equal(again[0], want[0]) and torch.equal(again[1], want[1])
    finally:
        enc.close()


def test_refusals_and_a_handle_without_the_fp32_packs():
    from open_provence_amd import _lib

    report = _lib.OpMaskedReport()
    report.struct_bytes = ctypes.sizeof(_lib.OpMaskedReport)
    vp = ctypes.c_void_p
    buf = torch.zeros(4096, dtype=torch.uint8, device="cuda:0")

    def args(handle, width=8, ws_bytes=1024, ws_offset=0):
        return (handle, vp(buf.data_ptr()), vp(buf.data_ptr()), 2, width, vp(buf.data_ptr() + ws_offset), ctypes.c_size_t(ws_bytes),
                vp(buf.data_ptr()), vp(buf.data_ptr()), ctypes.byref(report), None)

    # (attention_masks="any" alone: construction refuses nothing, the C call does)
    tiled = ("tiled-h384", 384, 6, 192, "GLL", 16, "cls", 1, False, "synth")
    for model, kernel_set, word in ((tiled, None, "tiled path"), (MODELS[0], "fp32", '"fp32"')):
        enc = _encoder(model, masked_kernels="fp32", kernel_set=kernel_set)
        try:
            assert enc.lib.op_forward_masked_native(*args(enc._handle)) == _lib.OP_ERR_UNSUPPORTED
            message = _lib.last_error(enc.lib, enc._handle)
            assert word in message and "op_forward_masked" in message.replace("op_forward_masked_native", ""), message
            ids, mask, _ = mm.batch(77)
            prune, rank = enc.forward_masked(ids, mask)  # ... and the fp32 pass serves the handle
            assert bool(torch.isfinite(rank).all())
        finally:
            enc.close()
    # ... and with masked_kernels="selected" construction raises, naming the reason
    from open_provence_amd.engine import HipEncoder

    with pytest.raises(ValueError, match="tiled path"):
        HipEncoder(_dims(tiled), device="cuda:0", attention_masks="any", masked_kernels="selected")
    with pytest.raises(ValueError, match='kernel_set="fp32"'):
        HipEncoder(_dims(MODELS[0]), device="cuda:0", attention_masks="any", masked_kernels="selected", kernel_set="fp32")

    enc = _encoder(MODELS[0])
    try:
        assert not enc.attention_outputs
        # the fp32 pass needs the packs this handle does not have; the native one runs
        assert enc.lib.op_forward_masked(*args(enc._handle)) == _lib.OP_ERR_UNSUPPORTED
        ids, mask, _ = mm.batch(77)
        prune, rank = enc.forward_masked(ids, mask)
        assert bool(torch.isfinite(rank).all()) and bool(torch.isfinite(prune).all())
        # the refusals of op_forward_masked, in its order
        assert enc.lib.op_forward_masked_native(*args(enc._handle, width=2049)) == _lib.OP_ERR_INVALID
        assert "max_position_embeddings" in _lib.last_error(enc.lib, enc._handle)
        assert enc.lib.op_forward_masked_native(*args(enc._handle)) == _lib.OP_ERR_WORKSPACE  # 1024 bytes: too small
        assert enc.lib.op_forward_masked_native(*args(enc._handle, ws_bytes=1 << 30, ws_offset=4)) == _lib.OP_ERR_WORKSPACE
        assert "aligned" in _lib.last_error(enc.lib, enc._handle)
        bad = _lib.OpMaskedReport()
        bad.struct_bytes = 8
        assert enc.lib.op_forward_masked_native(*args(enc._handle)[:-2], ctypes.byref(bad), None) == _lib.OP_ERR_INVALID
        assert enc.lib.op_forward_masked_native(*args(None)) == _lib.OP_ERR_INVALID  # NULL handle
        # an empty batch: OP_OK, nothing written
        before = buf.clone()
        for n_rows, width in ((0, 8), (3, 0)):
            empty = (enc._handle, None, None, n_rows, width, None, ctypes.c_size_t(0), None, None, ctypes.byref(report), None)
            assert enc.lib.op_forward_masked_native(*empty) == _lib.OP_OK
        torch.cuda.synchronize()
        assert torch.equal(buf, before)
        prune, rank = enc.forward_masked(torch.zeros((3, 0), dtype=torch.int64), torch.zeros((3, 0), dtype=torch.int64))
        assert prune.shape == (3, 0, 2) and rank.shape == (3, 1)
    finally:
        enc.close()


# -- test 5: forward() ---------------------------------------------------------------------------------------------------------------------------
def _model(**kw):
    from open_provence_amd.config import OpenProvenceConfig
    from open_provence_amd.modeling import OpenProvenceModel
    from open_provence_amd.synthetic import named_dims, refinit_state_dict

    dims = named_dims("xsmall", vocab_size=2048, num_layers=3)
    cfg = OpenProvenceConfig(base_model_config=dims.to_base_model_config(), tokenizer_name_or_path="char-tokenizer",
                             pruning_config={"hidden_size": dims.hidden_size}, max_length=512, num_labels=1,
                             pruning_hidden_state="post_final_norm")
    state = refinit_state_dict(dims, seed=5)
    return OpenProvenceModel(cfg, device="cuda:0", tokenizer=CharTokenizer(), state_dict=state, calibrate=False, **kw), dims, state


def _inputs(dims, rows=12, width=96, seed=3):
    from open_provence_amd.synthetic import pad_rows, synth_pair_batch

    rng = np.random.default_rng(seed)
    lengths = rng.integers(28, width + 1, size=rows).tolist()
    lengths[0], lengths[1] = width, 28
    return pad_rows(synth_pair_batch(dims, rows, lengths, seed=seed))


@pytest.fixture(scope="module")
def models():
    made = {"selected": _model(attention_masks="any", masked_kernels="selected"), "any": _model(attention_masks="any"), "default": _model()}
    yield made
    for model, _, _ in made.values():
        model.encoder.close()


def test_forward_takes_a_left_padded_batch_on_the_selected_set(models):
    from oracle.modernbert_oracle import oracle_forward

    model, dims, state = models["selected"]
    assert model.encoder.masked_kernels == "selected" and not model.encoder.attention_outputs
    ids, mask = _inputs(dims)
    left = torch.flip(mask, [1])
    # the yardstick: this model's own forward of the right-padded rows against the fp64 oracle
    torch.set_num_threads(16)
    ref = oracle_forward(state, dims, ids, mask, dtype=torch.float64)
    packed = model(input_ids=ids, attention_mask=mask)
    e_set = _distance(mm.compared(packed.pruning_logits.cpu(), packed.ranking_logits.cpu(), mask),
                      mm.compared(ref.pruning_logits, ref.ranking_logits, mask))
    ref = oracle_forward(state, dims, ids, left, dtype=torch.float64)
    want = mm.compared(ref.pruning_logits, ref.ranking_logits, left)
    out = model(input_ids=ids, attention_mask=left)
    _zeros_where_masked("forward(), left-padded", out.pruning_logits, out.ranking_logits, left)
    err = _distance(mm.compared(out.pruning_logits.cpu(), out.ranking_logits.cpu(), left), want)
    for q in QUANTITIES:
        bound = _bound(e_set, want, q)
        print(f"[masked-native] forward(), left-padded, {model.encoder.effective_policy()['kernel_set']:12s} {q:10s} err {err[q]:.3e}  "
              f"e_set {e_set[q]:.3e}  bound {bound:.3e}")
        assert err[q] <= bound, (q, err[q], bound)
    # CPU inputs and device-resident inputs: the same bits
    dev = model(input_ids=ids.cuda(), attention_mask=left.cuda())
    assert torch.equal(dev.pruning_logits, out.pruning_logits) and torch.equal(dev.ranking_logits, out.ranking_logits)
    rank, prune = model(input_ids=ids, attention_mask=left, return_dict=False)
    assert torch.equal(rank, out.ranking_logits) and torch.equal(prune, out.pruning_logits)
    labels = torch.arange(ids.shape[0]) % 2
    with_loss = model(input_ids=ids, attention_mask=left, labels=labels)
    assert torch.equal(with_loss.ranking_logits, out.ranking_logits)
    loss = torch.nn.BCEWithLogitsLoss()(out.ranking_logits.double().cpu().view(-1), labels.double())
    assert abs(float(with_loss.loss) - float(loss)) <= 2e-6 * max(1.0, abs(float(loss)))
    # the requests a non-prefix batch does not serve keep raising in this mode
    for kwargs, name in ((dict(output_hidden_states=True), "output_hidden_states"), (dict(pooled_hidden_states="mean"), "pooled_hidden_states")):
        with pytest.raises(NotImplementedError, match=name):
            model(input_ids=ids, attention_mask=left, **kwargs)


def test_prefix_batches_and_the_fp32_mode_are_what_they_were(models):
    (selected, dims, _), (any_model, _, _), (default, _, _) = models["selected"], models["any"], models["default"]
    ids, mask = _inputs(dims)
    left = torch.flip(mask, [1])
    for to in (lambda t: t, lambda t: t.cuda()):
        a = selected(input_ids=to(ids), attention_mask=to(mask), output_hidden_states=True)
        b = default(input_ids=to(ids), attention_mask=to(mask), output_hidden_states=True)
        assert torch.equal(a.pruning_logits, b.pruning_logits) and torch.equal(a.ranking_logits, b.ranking_logits)
        assert all(torch.equal(x, y) for x, y in zip(a.hidden_states, b.hidden_states))
    assert selected.encoder.effective_policy()["kernel_set"] == default.encoder.effective_policy()["kernel_set"]
    # attention_masks="any" alone: the fp32 pass, as before
    assert any_model.encoder.masked_kernels == "fp32" and any_model.encoder.attention_outputs
    out = any_model(input_ids=ids, attention_mask=left)
    prune, rank = any_model.encoder.forward_masked(ids, left)
    assert torch.equal(out.pruning_logits, prune) and torch.equal(out.ranking_logits, rank)
    with pytest.raises(NotImplementedError, match="right-padded"):
        default(input_ids=ids, attention_mask=left)


def test_a_non_finite_result_on_an_fp16_e4m3_set_is_repeated_on_the_bf16_sets():
    """As on the packed route (tests/test_gpu_policy.py, whose overflowing checkpoint this borrows): the batch is repeated on the
    (hi, lo) bf16 sets through the same op_set_compact_operands switch, with one warning, and the encoder stays there; the
    result has the bits of an encoder created with OP_FLAG_NO_F8."""

    import test_gpu_policy as policy
    from open_provence_amd import _lib
    from open_provence_amd.engine import HipEncoder
    from open_provence_amd.synthetic import pad_rows

    _meta, dims, rows, state = policy._overflowing_state()
    ids, mask = pad_rows(rows)
    left = torch.flip(mask, [1])
    assert not bool((left == mask).all())

    def encoder(flags):
        enc = HipEncoder(dims, device="cuda:0", precision="bf16x3", flags=flags, attention_masks="any", masked_kernels="selected")
        enc.load_state_dict(state, calibrate=False)
        return enc

    ref_enc = encoder(_lib.OP_FLAG_NO_F8)
    try:
        assert ref_enc.effective_policy()["kernel_set"] == "bf16x3"
        ref_p, ref_r = ref_enc.forward_masked(ids, left)
        assert bool(torch.isfinite(ref_p).all()) and bool(torch.isfinite(ref_r).all())
    finally:
        ref_enc.close()
    enc = encoder(0)
    try:
        assert enc.effective_policy()["kernel_set"] == "f16-f8-w" and enc.f8_active()
        with warnings.catch_warnings(record=True) as caught:
            warnings.simplefilter("always")
            p, r = enc.forward_masked(ids, left)
            assert any("fp16 + e4m3" in str(w.message) for w in caught)
        assert enc.effective_policy()["kernel_set"] == "bf16x3" and not enc.f8_active() and enc.fallbacks == 1
        assert torch.equal(p, ref_p) and torch.equal(r, ref_r)
        with warnings.catch_warnings(record=True) as caught:
            warnings.simplefilter("always")
            p2, _ = enc.forward_masked(ids, left)
            assert not caught
        assert torch.equal(p2, ref_p)
    finally:
        enc.close()


# -- the table -----------------------------------------------------------------------------------------------------------------------------------
def test_zz_the_worst_ratio_per_model_and_set():
    """Printed; written to ``MASKED_NATIVE_CONFORMANCE_OUT`` where that is set (after test 1 has measured every case)."""

    for model in MODELS:
        for width in WIDTHS:
            _measure(model, width)
    lines = ["op_forward_masked_native against the fp64 oracle (tests/test_gpu_masked_native.py): the worst case per (model, kernel set)",
             "over widths 200 / 77 / 1 and the quantities logits / keep_prob.  e_set = the same set's packed forward against the oracle on",
             "prefix_batch(width); bound = max(4 x e_set, 16 ulp).", "",
             f"{'model':36s} {'kernel set':24s} {'err / e_set':>12s} {'err / bound':>12s}  at"]
    for (model, name), worst in sorted(WORST.items()):
        lines.append(f"{model:36s} {name:24s} {worst['err/e_set']:12.2f} {worst['err/bound']:12.3f}  {worst['where']}")
    print("\n".join(lines))
    assert all(w["err/bound"] <= 1.0 for w in WORST.values())
    out = os.environ.get("MASKED_NATIVE_CONFORMANCE_OUT")
    if out:
        with open(out, "w") as f:
            f.write("\n".join(lines) + "\n")
