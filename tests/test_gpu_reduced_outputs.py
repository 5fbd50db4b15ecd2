"""Pooled hidden states (op_forward_packed_pooled) and attention rows (op_attention_rows) on the device.

The yardsticks are the parent's own calls on the same inputs -- the full fp32 hidden request and op_attention_probs -- which
this feature leaves untouched: ``first`` and the per-head rows are held to them with ``==``, ``mean`` and the head mean to the
float64 restatements of tests/reduced_outputs_model.py within 1 fp32 ulp (a derived bound, see there).  Lengths
[0, 1, 5, 63, 64, 65, 129, 300]: an empty row, a single token, both sides of the 64-key tile, more than one 128-query block, and
a sliding window (128) that hides keys; once more with the 300-token row first; once more on a handle whose chunk_rows puts chunk
boundaries inside the batch."""

from __future__ import annotations

import ctypes

import numpy as np
import pytest
import torch

import attention_utils as au
import reduced_outputs_model as rom
import test_kernel_set_conformance as conf
import workspace_utils as wu

pytestmark = pytest.mark.gpu

LENGTHS = [0, 1, 5, 63, 64, 65, 129, 300]
REORDERED = [300, 0, 1, 5, 63, 64, 65, 129]
ORDER = [LENGTHS.index(n) for n in REORDERED]  # REORDERED[i] is row ORDER[i] of LENGTHS
CHUNK_ROWS = 256  # the 300-token row alone, the others in two chunks
NAN32 = 0x7FC00000

# (model, kernel set, flags, pooling of the ranking head)
POOL_CASES = [
    ("row", "bf16x3", (), None),
    ("row", "f16", (), None),  # wave-pair epilogue store (layer16p_hout_kernel) + head-fused last launch
    ("row", "f16-f8-w", (), None),  # head-fused last launch (rowgemm_hout_kernel)
    ("panel512", "bf16x3", (), None),
    ("tiled", "bf16x3", (), None),
    ("row", "f16", ("NO_HEAD_FUSION",), None),
    ("row", "bf16x3", (), "mean"),  # a mean-pooling head: no head fusion, final_ln_prune_kernel writes over x
]


def _rows(lengths):
    by_length = dict(zip(LENGTHS, conf._rows(LENGTHS)))
    return [by_length[n] for n in lengths]


def _batch(enc, rows):
    from open_provence_amd.packing import pack_rows

    ids_np, cu_np, max_len = pack_rows(rows)
    return torch.from_numpy(ids_np).to(enc.device), torch.from_numpy(cu_np).to(enc.device), cu_np, max_len


def _pool_encoder(model, kernel_set, flags, pooling, chunk_rows=None):
    dims = conf._dims(model, 128, pooling=pooling)
    return conf._encoder(model, conf.weights_for(kernel_set, "o1"), 128, kernel_set, conf._flag_bits(flags), chunk_rows=chunk_rows, dims=dims)


def _forward(enc, rows, **requests):
    ids, cu, cu_np, max_len = _batch(enc, rows)
    out = enc.forward_packed(ids, cu, cu_np, max_len, **requests)
    torch.cuda.synchronize()
    return out, cu_np


def _same_bits(a: torch.Tensor, b: torch.Tensor) -> bool:
    return a.shape == b.shape and bool((wu._bits(a) == wu._bits(b)).all())


def _no_negative_zero(t: torch.Tensor) -> bool:
    return not bool((torch.signbit(t) & (t == 0)).any())


@pytest.mark.parametrize("model,kernel_set,flags,pooling", POOL_CASES)
def test_pooled_hidden_states(model, kernel_set, flags, pooling):
    from open_provence_amd.engine import HiddenRequest

    rows = _rows(LENGTHS)
    enc = _pool_encoder(model, kernel_set, flags, pooling)
    try:
        n_entries = enc.dims.num_layers + 1
        (prune0, rank0), cu_np = _forward(enc, rows)
        (prune_f, rank_f, full), _ = _forward(enc, rows, hidden=HiddenRequest())
        assert _same_bits(prune_f, prune0) and _same_bits(rank_f, rank0)
        full_np = full.cpu().numpy()
        pooled = {}
        for kind in ("first", "mean"):
            (prune, rank, got), _ = _forward(enc, rows, hidden=HiddenRequest(pool=kind))
            assert got.shape == (n_entries, len(rows), enc.dims.hidden_size) and got.dtype == torch.float32
            assert _same_bits(prune, prune0) and _same_bits(rank, rank0), f"{kind}: the logits moved"
            assert bool(torch.isfinite(got).all())
            pooled[kind] = got
            got_np = got.cpu().numpy()
            empty = LENGTHS.index(0)
            assert (got_np[:, empty] == 0).all() and not np.signbit(got_np[:, empty]).any(), f"{kind}: the empty row is not +0.0"
            for e in range(n_entries):
                if kind == "first":
                    assert (got_np[e] == rom.pooled_first(full_np[e], cu_np)).all(), f"first: entry {e} is not the full entry's row"
                else:
                    d = rom.ulp_distance(got_np[e], rom.pooled_mean(full_np[e], cu_np))
                    print(f"[pooled] {model} {kernel_set} {'+'.join(flags) or '-'} {pooling or 'cls'} mean entry {e}: {d:.2f} ulp")
                    assert d <= rom.ULP_BOUND, f"mean: entry {e} is {d:.2f} ulp from the float64 mean"
            # the same bits on a second call and on another stream
            (_, _, again), _ = _forward(enc, rows, hidden=HiddenRequest(pool=kind))
            assert _same_bits(again, got), f"{kind}: a second call gave other bits"
            side = torch.cuda.Stream(enc.device)
            side.wait_stream(torch.cuda.current_stream(enc.device))
            with torch.cuda.stream(side):
                (_, _, other), _ = _forward(enc, rows, hidden=HiddenRequest(pool=kind))
            assert _same_bits(other, got), f"{kind}: another stream gave other bits"
            # another batch around each sequence: the 300-token row first; the 129-token row alone
            (_, _, moved), _ = _forward(enc, _rows(REORDERED), hidden=HiddenRequest(pool=kind))
            assert _same_bits(moved, got[:, ORDER]), f"{kind}: the batch's order changed a sequence's row"
            (_, _, alone), _ = _forward(enc, _rows([129]), hidden=HiddenRequest(pool=kind))
            assert _same_bits(alone[:, 0], got[:, LENGTHS.index(129)]), f"{kind}: a sequence alone differs from the batch's"
        # a subset of entries, and a pooled request beside a full one (bf16, padded) in one call
        some = [0, n_entries - 1]
        (_, _, subset), _ = _forward(enc, rows, hidden=HiddenRequest(layers=some, pool="mean"))
        assert _same_bits(subset, pooled["mean"][some])
        width = max(LENGTHS) + 3
        beside = HiddenRequest(layers=[1, n_entries - 1], dtype=torch.bfloat16, pad_width=width)
        (_, _, want_states), _ = _forward(enc, rows, hidden=beside)
        (prune, rank, states, got), _ = _forward(enc, rows, hidden=beside, pooled=HiddenRequest(layers=[0, 1], pool="first"))
        assert _same_bits(prune, prune0) and _same_bits(rank, rank0)
        assert _same_bits(states, want_states), "the full request beside a pooled one differs from the full request alone"
        assert _same_bits(got, pooled["first"][[0, 1]])
    finally:
        enc.close()
    # chunk boundaries inside the batch: the same bits as the whole handle
    enc = _pool_encoder(model, kernel_set, flags, pooling, chunk_rows=CHUNK_ROWS)
    try:
        for kind in ("first", "mean"):
            for lengths, want in ((LENGTHS, pooled[kind]), (REORDERED, pooled[kind][:, ORDER])):
                (_, _, got), _ = _forward(enc, _rows(lengths), hidden=HiddenRequest(pool=kind))
                assert _same_bits(got, want), f"{kind}: chunk_rows {CHUNK_ROWS} changed the pooled rows ({lengths[0]} first)"
    finally:
        enc.close()


def _c_pooled(enc, rows, kind, *, fill, scratch_fill, select=None, hidden_req=None, pool_fields=None, scratch_bytes=None, handle=True,
              pool=True):
    """op_forward_packed_pooled itself: the logits, the pooled output and the scratch are views between canaries, the output
    pre-filled with NaN, scratch and workspace with ``scratch_fill`` / ``fill`` -> (code, prune, rank, out); canaries asserted."""

    from open_provence_amd import _lib

    ids, cu, cu_np, max_len = _batch(enc, rows)
    n_seqs, total = len(rows), int(ids.numel())
    H, n_entries, nl = enc.dims.hidden_size, enc.dims.num_layers + 1, enc.dims.num_labels
    n_sel = n_entries if select is None else int(sum(select))
    cw = wu.controlled_workspace(enc, n_seqs, total, max_len)
    wu.fill_workspace(cw, fill)
    bufs = {"prune": wu.canaried(total * 2 * 4, enc.device), "rank": wu.canaried(n_seqs * nl * 4, enc.device),
            "out": wu.canaried(n_sel * n_seqs * H * 4, enc.device), "scratch": wu.canaried(total * H * 4, enc.device)}
    bufs["out"].view.view(torch.int32).fill_(NAN32)
    bufs["scratch"].view.fill_({"zeros": 0, "nan": wu.NAN_BYTE, "huge": wu.HUGE_BYTE}[scratch_fill])
    vp = ctypes.c_void_p
    req = _lib.OpPoolRequest()
    req.struct_bytes = ctypes.sizeof(_lib.OpPoolRequest)
    req.kind = _lib.POOL_KINDS[kind] if isinstance(kind, str) else kind
    flags = None if select is None else (ctypes.c_uint8 * n_entries)(*select)
    req.select = None if flags is None else ctypes.cast(flags, ctypes.POINTER(ctypes.c_uint8))
    req.out_dev = vp(bufs["out"].view.data_ptr())
    req.scratch_dev = vp(bufs["scratch"].view.data_ptr())
    req.scratch_bytes = total * H * 4 if scratch_bytes is None else scratch_bytes
    for name, value in (pool_fields or {}).items():
        setattr(req, name, value)
    with torch.cuda.device(enc.device):
        code = enc.lib.op_forward_packed_pooled(
            enc._handle if handle else None, vp(ids.data_ptr()), vp(cu.data_ptr()), cu_np.ctypes.data_as(vp), n_seqs, total, max_len,
            vp(bufs["prune"].view.data_ptr()), vp(bufs["rank"].view.data_ptr()), None, vp(cw.view.data_ptr()), ctypes.c_size_t(cw.need),
            vp(torch.cuda.current_stream(enc.device).cuda_stream), ctypes.byref(hidden_req) if hidden_req is not None else None,
            ctypes.byref(req) if pool else None)
    torch.cuda.synchronize()
    cw.mem.assert_intact("pooled call: workspace")
    for name, buf in bufs.items():
        buf.assert_intact(f"pooled call: {name}")
    return (code, bufs["prune"].view.view(torch.float32).view(total, 2), bufs["rank"].view.view(torch.float32).view(n_seqs, nl),
            bufs["out"].view.view(torch.float32).view(n_sel, n_seqs, H))


@pytest.mark.parametrize("model,kernel_set", [("row", "f16"), ("panel512", "bf16x3")])
def test_pooled_buffers_are_written_whole_and_nothing_else(model, kernel_set):
    """Outputs pre-filled with NaN between canaries: every element inside is written, the margins are intact; a poisoned
    workspace and scratch give the bits of zeroed ones."""

    rows = _rows(LENGTHS)
    enc = _pool_encoder(model, kernel_set, (), None)
    try:
        for kind in ("first", "mean"):
            code, prune0, rank0, want = _c_pooled(enc, rows, kind, fill="zeros", scratch_fill="zeros")
            assert code == 0
            assert bool(torch.isfinite(want).all()), f"{kind}: an element of the output was not written"
            for poison in wu.POISONS:
                code, prune, rank, got = _c_pooled(enc, rows, kind, fill=poison, scratch_fill=poison)
                assert code == 0
                assert _same_bits(got, want) and _same_bits(prune, prune0) and _same_bits(rank, rank0), f"{kind}: {poison} leaked"
        # only empty sequences: rows of +0.0, nothing else
        code, _, _, got = _c_pooled(enc, [[], []], "mean", fill="nan", scratch_fill="nan")
        assert code == 0 and bool((got == 0).all()) and _no_negative_zero(got)
    finally:
        enc.close()


def test_pooled_request_needs_one_entry_of_memory():
    """A condition, not a measurement: at 64 x 128 on the row model the peak of a pooled request of all entries, over that of a
    plain forward, is at most one packed fp32 entry + the outputs + 1 MB; the full request exceeds that."""

    from open_provence_amd.engine import HiddenRequest

    enc = _pool_encoder("row", "f16", (), None)
    try:
        rows = conf._rows([128] * 64, seed=11)
        ids, cu, cu_np, max_len = _batch(enc, rows)
        H, n_entries = enc.dims.hidden_size, enc.dims.num_layers + 1
        entry, outputs = 64 * 128 * H * 4, n_entries * 64 * H * 4

        def peak(**requests):
            enc.forward_packed(ids, cu, cu_np, max_len, **requests)  # (the workspace exists from here on)
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats(enc.device)
            base = torch.cuda.memory_allocated(enc.device)
            out = enc.forward_packed(ids, cu, cu_np, max_len, **requests)
            torch.cuda.synchronize()
            top = torch.cuda.max_memory_allocated(enc.device) - base
            del out
            return top

        plain = peak()
        for kind in ("first", "mean"):
            extra = peak(hidden=HiddenRequest(pool=kind)) - plain
            print(f"[pooled] memory over a plain forward, {kind}: {extra} bytes (one entry {entry}, outputs {outputs})")
            assert extra <= entry + outputs + (1 << 20)
        assert peak(hidden=HiddenRequest()) - plain > entry + outputs + (1 << 20)
    finally:
        enc.close()


def test_pooled_refusals():
    from open_provence_amd import _lib
    from open_provence_amd.engine import HiddenRequest

    rows = _rows([5, 64])
    enc = _pool_encoder("row", "bf16x3", (), None)
    try:
        (prune0, rank0), _ = _forward(enc, rows)

        def refused(what, **kw):
            code, prune, rank, out = _c_pooled(enc, rows, kw.pop("kind", "mean"), fill="zeros", scratch_fill="zeros", **kw)
            assert code == _lib.OP_ERR_INVALID, (what, code)
            message = _lib.last_error(enc.lib, enc._handle if kw.get("handle", True) else None)
            assert "op_forward_packed_pooled" in message, (what, message)
            # nothing was enqueued: the canary-initialised logits and the NaN output are as they were
            assert bool((prune.view(torch.int32) == wu.CANARY).all()) and bool((out.view(torch.int32) == NAN32).all()), what

        refused("no pooled request", pool=False)
        refused("struct_bytes", pool_fields={"struct_bytes": 8})
        refused("struct_bytes, before the handle", pool_fields={"struct_bytes": 8}, handle=False)
        refused("unknown kind", kind=2)
        refused("unknown kind, before the handle", kind=-1, handle=False)
        refused("scratch too small", scratch_bytes=(5 + 64) * enc.dims.hidden_size * 4 - 4)
        refused("NULL scratch", pool_fields={"scratch_dev": None})
        refused("NULL output", pool_fields={"out_dev": None})
        refused("misaligned scratch", pool_fields={"scratch_dev": ctypes.c_void_p(0x1004)})
        bad = _lib.OpHiddenRequest()
        bad.struct_bytes = 4
        refused("the hidden request's struct_bytes", hidden_req=bad)
        bad = _lib.OpHiddenRequest()
        bad.struct_bytes, bad.pad_width = ctypes.sizeof(_lib.OpHiddenRequest), 3
        refused("the hidden request's pad_width", hidden_req=bad)
        # and the handle still works
        code, prune, rank, _ = _c_pooled(enc, rows, "first", fill="zeros", scratch_fill="zeros", select=[1, 0, 0, 1])
        assert code == 0 and _same_bits(prune, prune0) and _same_bits(rank, rank0)
        ids, cu, cu_np, max_len = _batch(enc, rows)
        with pytest.raises(ValueError):
            enc.forward_packed(ids, cu, cu_np, max_len, hidden=HiddenRequest(pool="mean"), pooled=HiddenRequest(pool="first"))
        with pytest.raises(ValueError):
            enc.forward_packed(ids, cu, cu_np, max_len, pooled=HiddenRequest())
        with pytest.raises(ValueError):
            enc.forward_packed(ids, cu, cu_np, max_len, hidden=HiddenRequest(layers=[7], pool="first"))
        with pytest.raises(NotImplementedError):
            enc.forward_packed_on(0, ids, cu, cu_np, max_len, hidden=HiddenRequest(pool="first"))
    finally:
        enc.close()


# ---- attention rows ---------------------------------------------------------------------------------------------------------------
# layer 0 (no attn_norm) slides, then a global layer: a global layer WITH attn_norm, a sliding layer with one, and layer 0
ATTN_MODELS = {"row": "LGL", "panel512": "LGL", "tiled": "LG"}


def _attn_encoder(model, chunk_rows=None):
    from open_provence_amd.engine import HipEncoder

    dims = conf._dims(model, 128, layer_types=ATTN_MODELS[model])
    enc = HipEncoder(dims, device="cuda:0", chunk_rows=chunk_rows, attention_outputs=True)
    try:
        enc.load_state_dict(conf._state(model, "o1", 128), calibrate=False, kernel_set="bf16x3")
    except BaseException:
        enc.close()
        raise
    return enc


def _queries(lengths):
    """name -> host int64 positions (None: the NULL request): the last token of each row (0 for the empty row: beyond it), and a
    position beyond some of the lengths"""

    return {"first": None, "last": torch.tensor([max(n - 1, 0) for n in lengths]), "beyond": torch.tensor([64] * len(lengths))}


def _expected_rows(full: torch.Tensor, lengths, query) -> torch.Tensor:
    """``full[B, heads, W, W]`` of op_attention_probs -> ``[B, heads, W]``: row query[s], zeros when it is not a token of s"""

    want = torch.zeros(full.shape[:3], dtype=full.dtype)
    for s, n in enumerate(lengths):
        q = 0 if query is None else int(query[s])
        if q < n:
            want[s] = full[s, :, q]
    return want


@pytest.mark.parametrize("model", list(ATTN_MODELS))
def test_attention_rows(model):
    from open_provence_amd.engine import AttentionRequest, HiddenRequest
    from open_provence_amd.synthetic import pad_rows

    enc = _attn_encoder(model)
    chunked = _attn_encoder(model, chunk_rows=CHUNK_ROWS)
    try:
        dims, state = enc.dims, conf._state(model, "o1", 128)
        rows = _rows(LENGTHS)
        ids, cu, cu_np, max_len = _batch(enc, rows)
        (prune0, rank0, states), _ = _forward(enc, rows, hidden=HiddenRequest())
        _, mask = pad_rows([r or [0] for r in rows])
        mask[LENGTHS.index(0)] = 0
        moved_cu = np.concatenate(([0], np.cumsum(REORDERED))).astype(np.int32)
        for layer in range(dims.num_layers):
            hidden = states[layer].contiguous()
            padded = torch.zeros(len(rows), max_len, dims.hidden_size)
            padded[mask.bool()] = hidden.cpu()
            p64 = au.attention_probs(state, dims, padded, mask, layer, torch.float64)
            e_ref = float((au.attention_probs(state, dims, padded, mask, layer, torch.float32).double() - p64).abs().max())
            for width in (max_len, max_len + 3):
                full = enc.attention_probs(hidden, layer, cu, cu_np, max_len, width).cpu()  # (the parent's code: the yardstick)
                for name, query in _queries(LENGTHS).items():
                    want = _expected_rows(full, LENGTHS, query)
                    label = f"{model} layer {layer} width {width} query {name}"
                    for place in ("host", "device"):
                        q = query if query is None or place == "host" else query.to(enc.device)
                        got = enc.attention_rows(hidden, layer, cu, cu_np, max_len, width, query=q).cpu()
                        assert got.shape == (len(rows), dims.num_heads, width)
                        assert _same_bits(got, want), f"{label} ({place}): not the row of op_attention_probs"
                    assert _no_negative_zero(got) and bool(torch.isfinite(got).all())
                    # the fp64 restatement, within the module's bound
                    ref = _expected_rows(torch.nn.functional.pad(p64, (0, width - max_len, 0, width - max_len)), LENGTHS, query)
                    err = float((got.double() - ref).abs().max())
                    print(f"[attn-rows] {label}: err {err:.3e} e_ref {e_ref:.3e} bound {au.probs_bound(e_ref):.3e}")
                    assert err <= au.probs_bound(e_ref), f"{label}: {err:.3e} from the fp64 restatement"
                    # exact zeros: beyond each length, out to the width, whole rows without a query
                    for s, n in enumerate(LENGTHS):
                        assert bool((got[s, :, n:] == 0).all()), f"{label}: row {s} is not zero beyond its length"
                        if (0 if query is None else int(query[s])) >= n:
                            assert bool((got[s] == 0).all()), f"{label}: row {s} has no such query and is not zero"
                    # the head mean: 1 ulp of the float64 mean of those rows
                    mean = enc.attention_rows(hidden, layer, cu, cu_np, max_len, width, query=query, reduce_heads=True).cpu()
                    assert mean.shape == (len(rows), width) and _no_negative_zero(mean)
                    d = rom.ulp_distance(mean.numpy(), rom.head_mean(got.numpy()))
                    print(f"[attn-rows] {label}: head mean {d:.2f} ulp")
                    assert d <= rom.ULP_BOUND, f"{label}: the head mean is {d:.2f} ulp from the float64 mean"
                    assert bool((mean[want.sum(1) == 0] == 0).all())
                    if width != max_len:
                        continue
                    # a second call; the chunked handle; the 300-token row first
                    assert _same_bits(enc.attention_rows(hidden, layer, cu, cu_np, max_len, width, query=query).cpu(), got)
                    c_hidden, c_cu = hidden.to(chunked.device), cu.to(chunked.device)
                    assert _same_bits(chunked.attention_rows(c_hidden, layer, c_cu, cu_np, max_len, width, query=query).cpu(), got), label
                    assert _same_bits(chunked.attention_rows(c_hidden, layer, c_cu, cu_np, max_len, width, query=query, reduce_heads=True).cpu(),
                                      mean), label
                    m_hidden = torch.cat([hidden[int(cu_np[s]): int(cu_np[s + 1])] for s in ORDER]).contiguous()
                    m_query = None if query is None else query[ORDER]
                    m_cu = torch.from_numpy(moved_cu).to(enc.device)
                    for handle in (enc, chunked):
                        moved = handle.attention_rows(m_hidden, layer, m_cu, moved_cu, max_len, width, query=m_query).cpu()
                        assert _same_bits(moved, got[ORDER]), f"{label}: the batch's order changed a sequence's row"
        # through one forward: AttentionRequest(query=...) beside the logits, which stay what they were
        prune, rank, rows_out = enc.forward_packed(ids, cu, cu_np, max_len, attentions=AttentionRequest(layers=[1], query="first", reduce_heads=True))
        want = enc.attention_rows(states[1].contiguous(), 1, cu, cu_np, max_len, reduce_heads=True)
        assert _same_bits(prune, prune0) and _same_bits(rank, rank0) and len(rows_out) == 1 and _same_bits(rows_out[0], want)
    finally:
        enc.close()
        chunked.close()


def test_head_mean_of_a_large_batch_matches_the_small_batch():
    """Beyond 128 sequences the head mean runs one block per sequence, up to there its blocks split the key tiles: the same bits
    for the same sequence either way, and within 1 ulp of the float64 mean of the per-head rows."""

    from open_provence_amd.engine import HiddenRequest

    enc = _attn_encoder("row")
    try:
        lengths = [1, 5, 65, 129, 0] * 26  # 130 sequences
        rows = [r for _ in range(26) for r in _rows([1, 5, 65, 129, 0])]
        ids, cu, cu_np, max_len = _batch(enc, rows)
        query = torch.tensor([0, 4, 64, 100, 0] * 26)
        (_, _, states), _ = _forward(enc, rows, hidden=HiddenRequest(layers=[1, 2]))
        for slot, layer in enumerate((1, 2)):
            hidden = states[slot].contiguous()
            per_head = enc.attention_rows(hidden, layer, cu, cu_np, max_len, query=query).cpu()
            mean = enc.attention_rows(hidden, layer, cu, cu_np, max_len, query=query, reduce_heads=True).cpu()
            assert rom.ulp_distance(mean.numpy(), rom.head_mean(per_head.numpy())) <= rom.ULP_BOUND
            small_cu = cu_np[:6].copy()
            small = enc.attention_rows(hidden[: int(small_cu[-1])].contiguous(), layer, cu[:6].contiguous(), small_cu, max_len, query=query[:5],
                                       reduce_heads=True).cpu()
            for block in range(0, len(lengths), 5):
                assert _same_bits(mean[block: block + 5], small), f"layer {layer}: sequences {block} .. differ from the small batch"
    finally:
        enc.close()


def _c_rows(enc, hidden, layer, cu, cu_np, max_len, width, *, fill, query=None, query_host=None, reduce_heads=0, fields=None, handle=True,
            request=True):
    """op_attention_rows itself, with a NaN-filled output between canaries and a workspace filled with ``fill`` -> (code, out)"""

    from open_provence_amd import _lib

    n_seqs, total = len(cu_np) - 1, int(hidden.shape[0])
    need = int(enc.lib.op_attention_workspace_bytes(enc._handle, n_seqs, total, max_len))
    ws = wu.canaried(need, enc.device)
    ws.view.fill_({"zeros": 0, "nan": wu.NAN_BYTE, "huge": wu.HUGE_BYTE}[fill])
    out = wu.canaried(n_seqs * (1 if reduce_heads == 1 else enc.dims.num_heads) * width * 4, enc.device)
    out.view.view(torch.int32).fill_(NAN32)
    vp = ctypes.c_void_p
    req = _lib.OpAttentionRowsRequest()
    req.struct_bytes = ctypes.sizeof(_lib.OpAttentionRowsRequest)
    req.layer, req.pad_width, req.reduce_heads = layer, width, reduce_heads
    req.hidden_dev, req.out_dev = vp(hidden.data_ptr()), vp(out.view.data_ptr())
    req.query_pos_dev = vp(query.data_ptr()) if query is not None else None
    req.query_pos_host = query_host.ctypes.data_as(vp) if query_host is not None else None
    for name, value in (fields or {}).items():
        setattr(req, name, value)
    with torch.cuda.device(enc.device):
        code = enc.lib.op_attention_rows(enc._handle if handle else None, vp(cu.data_ptr()), cu_np.ctypes.data_as(vp), n_seqs, total, max_len,
                                         ctypes.byref(req) if request else None, vp(ws.view.data_ptr()), ctypes.c_size_t(need),
                                         vp(torch.cuda.current_stream(enc.device).cuda_stream))
    torch.cuda.synchronize()
    ws.assert_intact("op_attention_rows: workspace")
    out.assert_intact("op_attention_rows: output")
    shape = (n_seqs, width) if reduce_heads == 1 else (n_seqs, enc.dims.num_heads, width)
    return code, out.view.view(torch.float32).view(shape)


def test_attention_rows_buffers_and_refusals():
    from open_provence_amd import _lib
    from open_provence_amd.engine import AttentionRequest, HiddenRequest, HipEncoder

    enc = _attn_encoder("row")
    try:
        rows = _rows(LENGTHS)
        ids, cu, cu_np, max_len = _batch(enc, rows)
        (_, _, states), _ = _forward(enc, rows, hidden=HiddenRequest(layers=[1, 2]))
        width = max_len + 3  # an odd width, an unaligned tail
        query = torch.tensor([0, 0, 4, 70, 63, 64, 128, 299], dtype=torch.int32, device=enc.device)  # (70: beyond its 63-token row)
        for slot, layer in enumerate((1, 2)):
            hidden = states[slot].contiguous()
            for reduce_heads in (0, 1):
                code, want = _c_rows(enc, hidden, layer, cu, cu_np, max_len, width, fill="zeros", query=query, reduce_heads=reduce_heads)
                assert code == 0 and bool(torch.isfinite(want).all()), "an element of the output was not written"
                assert _same_bits(want, enc.attention_rows(hidden, layer, cu, cu_np, max_len, width, query=query, reduce_heads=bool(reduce_heads)))
                for poison in wu.POISONS:
                    code, got = _c_rows(enc, hidden, layer, cu, cu_np, max_len, width, fill=poison, query=query, reduce_heads=reduce_heads)
                    assert code == 0 and _same_bits(got, want), f"layer {layer}: a {poison} workspace leaked"
        # a negative position that only the device sees: a row of zeros, never an index
        hidden = states[0].contiguous()
        negative = torch.tensor([0, 0, -1, -(2**31), 3, -7, 2, 1], dtype=torch.int32, device=enc.device)
        code, got = _c_rows(enc, hidden, 1, cu, cu_np, max_len, width, fill="nan", query=negative)
        assert code == 0 and bool(torch.isfinite(got).all())
        for s in (0, 2, 3, 5):
            assert bool((got[s] == 0).all()) and _no_negative_zero(got[s])
        assert float(got[7].sum()) > 0

        def refused(what, want=_lib.OP_ERR_INVALID, **kw):
            code, out = _c_rows(enc, hidden, kw.pop("layer", 1), cu, cu_np, max_len, kw.pop("width", width), fill="zeros", **kw)
            assert code == want, (what, code)
            assert "op_attention_rows" in _lib.last_error(enc.lib, enc._handle if kw.get("handle", True) else None), what
            assert bool((out.view(torch.int32) == NAN32).all()), f"{what}: something was enqueued"

        refused("no request", request=False)
        refused("no request, before the handle", request=False, handle=False)
        refused("struct_bytes", fields={"struct_bytes": 16})
        refused("struct_bytes, before the handle", fields={"struct_bytes": 16}, handle=False)
        refused("reduce_heads", reduce_heads=2)
        refused("pad_width below max_seqlen", width=max_len - 1)
        refused("NULL hidden", fields={"hidden_dev": None})
        refused("NULL output", fields={"out_dev": None}, handle=False)
        refused("a negative position visible on the host", query=negative, query_host=negative.cpu().numpy())
        refused("host positions without device positions", query_host=negative.cpu().numpy())
        refused("layer", layer=3)
        refused("layer", layer=-1)
        with pytest.raises(ValueError):
            enc.attention_rows(hidden, 1, cu, cu_np, max_len, query=torch.tensor([0, 0, -1, 0, 0, 0, 0, 0]))
        with pytest.raises(ValueError):
            enc.attention_rows(hidden, 1, cu, cu_np, max_len, query=torch.tensor([0, 0]))
        with pytest.raises(ValueError):
            enc.attention_rows(hidden, 1, cu, cu_np, max_len, pad_width=max_len - 1)
    finally:
        enc.close()
    # without the fp32 packs: OP_ERR_UNSUPPORTED naming the flag; the Python layer raises before the call
    plain = HipEncoder(conf._dims("row", 128), device="cuda:0")
    try:
        plain.load_state_dict(conf._state("row", "o1", 128), calibrate=False, kernel_set="bf16x3")
        ids, cu, cu_np, max_len = _batch(plain, _rows([5, 64]))
        hidden = torch.zeros(69, plain.dims.hidden_size, device=plain.device)
        code, out = _c_rows(plain, hidden, 1, cu, cu_np, max_len, max_len, fill="zeros")
        assert code == _lib.OP_ERR_UNSUPPORTED and "OP_FLAG_F32_PACKS" in _lib.last_error(plain.lib, plain._handle)
        assert bool((out.view(torch.int32) == NAN32).all())
        with pytest.raises(ValueError):
            plain.attention_rows(hidden, 1, cu, cu_np, max_len)
        with pytest.raises(ValueError):
            plain.forward_packed(ids, cu, cu_np, max_len, attentions=AttentionRequest(query="first"))
    finally:
        plain.close()


def test_model_forward_reduced_outputs():
    """forward(pooled_hidden_states=..., attention_rows=...): the new fields against the full outputs of the same model, on the
    host-packed and the device-resident route; defaults leave them None."""

    from helpers import CharTokenizer
    from open_provence_amd.config import OpenProvenceConfig
    from open_provence_amd.modeling import OpenProvenceForTokenClassification, OpenProvenceModel
    from open_provence_amd.synthetic import pad_rows

    dims = conf._dims("row", 128)
    base = dict(model_type="modernbert", vocab_size=512, hidden_size=256, intermediate_size=1024, num_hidden_layers=3, num_attention_heads=4,
                local_attention=128, global_attn_every_n_layers=3, global_rope_theta=160000.0, local_rope_theta=10000.0,
                max_position_embeddings=2048, pad_token_id=0, cls_token_id=1, sep_token_id=2)
    cfg = OpenProvenceConfig(base_model_config=base, tokenizer_name_or_path="char-tokenizer", pruning_config={"hidden_size": 256},
                             max_length=2048, num_labels=1, pruning_hidden_state="post_final_norm")
    state = conf._state("row", "o1", 128)
    lengths = [1, 5, 65, 129]
    ids, mask = pad_rows(conf._rows(lengths))
    query = torch.tensor([0, 4, 64, 200])
    for cls in (OpenProvenceModel, OpenProvenceForTokenClassification):
        model = cls(cfg, device="cuda:0", tokenizer=CharTokenizer(), state_dict=state, attention_outputs=True, kernel_set="bf16x3")
        assert model.dims.num_layers == dims.num_layers
        plain = model(input_ids=ids, attention_mask=mask)
        assert plain.pooled_hidden_states is None and plain.attention_rows is None
        full = model(input_ids=ids, attention_mask=mask, output_hidden_states=True, output_attentions=True)
        for route in ("host", "device"):
            a, m = (ids, mask) if route == "host" else (ids.to("cuda:0"), mask.to("cuda:0"))
            out = model(input_ids=a, attention_mask=m, pooled_hidden_states="first", attention_rows=query)
            assert _same_bits(out.pruning_logits, plain.pruning_logits) and _same_bits(out.ranking_logits, plain.ranking_logits)
            assert out.hidden_states is None and out.attentions is None
            assert _same_bits(out.pooled_hidden_states, torch.stack([h[:, 0] for h in full.hidden_states]))
            assert len(out.attention_rows) == dims.num_layers
            for got, whole in zip(out.attention_rows, full.attentions):
                assert _same_bits(got.cpu(), _expected_rows(whole.cpu(), lengths, query))
            both = model(input_ids=a, attention_mask=m, output_hidden_states=True, output_attentions=True, pooled_hidden_states="mean",
                         attention_rows="first", attention_rows_reduce_heads=True)
            assert all(_same_bits(x, y) for x, y in zip(both.hidden_states, full.hidden_states))
            assert all(_same_bits(x, y) for x, y in zip(both.attentions, full.attentions))
            cu_np = np.concatenate(([0], np.cumsum(lengths))).astype(np.int32)
            for e, entry in enumerate(full.hidden_states):
                packed = entry.cpu()[mask.bool()].numpy()
                assert rom.ulp_distance(both.pooled_hidden_states[e].cpu().numpy(), rom.pooled_mean(packed, cu_np)) <= rom.ULP_BOUND
            for got, whole in zip(both.attention_rows, full.attentions):
                assert rom.ulp_distance(got.cpu().numpy(), rom.head_mean(whole.cpu()[:, :, 0].numpy())) <= rom.ULP_BOUND
        with pytest.raises(ValueError):
            model(input_ids=ids, attention_mask=mask, pooled_hidden_states="max")
        with pytest.raises(ValueError):
            model(input_ids=ids, attention_mask=mask, attention_rows_reduce_heads=True)
    bare = OpenProvenceModel(cfg, device="cuda:0", tokenizer=CharTokenizer(), state_dict=state, kernel_set="bf16x3")
    with pytest.raises(ValueError, match="attention_outputs=True"):
        bare(input_ids=ids, attention_mask=mask, attention_rows="first")
    with pytest.raises(ValueError, match="attention_outputs=True"):
        bare(input_ids=ids, attention_mask=mask, output_attentions=True)
