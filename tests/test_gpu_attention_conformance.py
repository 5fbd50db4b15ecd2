"""op_attention_probs (attn_probs_f32_kernel and its gather) against an fp64 restatement evaluated at run time.

The bound.  The kernel is fed the bits the reference is fed: ``hidden_states[i]`` of the fp64 oracle rounded to fp32
(``attention_utils.probs_reference``).  With ``e_ref`` = max |fp32 restatement - fp64 restatement| on those bits, the kernel must be
within

    max(4 x e_ref, 16 ulp_fp32(1.0))

of the fp64 restatement -- the bound of every kernel set (test_gpu_fp32_set.py); the ulp floor is taken at 1.0 because a
probability is at most 1.  Each case prints ``err / e_ref`` (profiles/attention_conformance.txt is the first run's table).
``attention_bounds.json`` (test_gpu_attentions.py) stays what it is: a regression record measured on the kernel.

1. the kernel alone, every layer of models A / B / C, refinit weights (the ulp floor is the bound), the trained-like proxy
   (probabilities down to 1e-32) and peaked rows (the running-max rescale of pass 1, expf underflow);
2. a zero state gives ``1 / count`` on every visible key, to 1 ulp: every window edge, sequence end and tile edge of every
   query, whatever mass sits there;
3. nothing but ``out`` and the advertised workspace bytes is written, on both store paths at both alignments of ``out``;
4. batch composition: a row alone, a chunked handle, empty sequences inside a batch; a 4097-token row next to an empty and a
   5-token sequence (every other row of the module has at most 321 tokens);
5. end to end on kernel set "fp32" (the forward's rounding included in e_ref)."""

from __future__ import annotations

import numpy as np
import pytest
import torch

import attention_utils as au

pytestmark = pytest.mark.gpu

NAN_BITS = 0x7FC00000
GUARD = 4096  # sentinel floats before and after `out`; sentinel bytes behind the workspace


# 1. the kernel alone against fp64 -----------------------------------------------------------------------------------------------
KERNEL_CASES = [("A", "synth", False), ("A", "refinit", False), ("B", "synth", False), ("C", "synth", False), ("T", "synth", False),
                ("A", "synth", True), ("B", "synth", True)]


@pytest.mark.parametrize("name,weights,peaked", KERNEL_CASES, ids=lambda v: {True: "peaked", False: "plain"}.get(v, v))
def test_kernel_alone_within_four_times_the_reference_error(name, weights, peaked):
    ref = au.probs_reference(name, weights, peaked)
    if peaked:  # the construction does what it is for, on the reference itself
        assert all(ref.median_row_max(i) >= 0.9 for i in range(ref.dims.num_layers))
    enc = au.conformance_encoder(ref.dims, ref.state)
    try:
        for layer in range(ref.dims.num_layers):
            got = au.kernel_probs(enc, ref.packed(layer), layer, au.EDGE)
            assert got.shape == ref.p64[layer].shape and got.dtype == torch.float32
            au.check_probs(f"kernel {name} {weights}{' peaked' if peaked else ''}", got, ref, layer)
    finally:
        enc.close()


# 2. exact geometry: a zero state gives a uniform row ------------------------------------------------------------------------------
@pytest.mark.parametrize("window", [1, 2, 6, 16, 126, 128, 130, 1024])
def test_zero_state_gives_one_over_the_visible_count(window):
    """q = k = 0 on every layer (no bias anywhere, LayerNorm(0) = 0): every partial sum of the kernel is a sum of exact 1.0s and
    only the final division rounds."""

    from open_provence_amd.synthetic import synth_state_dict

    dims = au.small_dims(128, 2, "GL", window)
    enc = au.conformance_encoder(dims, synth_state_dict(dims, 5))
    mask = torch.zeros((len(au.EDGE), max(au.EDGE)), dtype=torch.int64)
    for b, n in enumerate(au.EDGE):
        mask[b, :n] = 1
    zeros = torch.zeros((sum(au.EDGE), dims.hidden_size), dtype=torch.float32)
    try:
        for layer in range(dims.num_layers):
            got = au.kernel_probs(enc, zeros, layer, au.EDGE).cpu()
            want = au.uniform_probs(dims, mask, layer).float()[:, None].expand_as(got)
            vis = au.visible_mask(dims, mask, layer)[:, None].expand_as(got)
            assert bool((got[~vis] == 0).all()) and not bool(torch.signbit(got).any()), f"w {dims.half_window} layer {layer}: a hidden key is not +0.0"
            ulp = torch.from_numpy(np.spacing(want[vis].numpy())).double()
            off = (got[vis].double() - want[vis].double()).abs() / ulp
            assert float(off.max()) <= 1.0, f"w {dims.half_window} layer {layer}: {float(off.max()):.2f} ulp from 1 / count"
    finally:
        enc.close()


# 3. nothing outside the output and the advertised workspace is touched ---------------------------------------------------------------
def _guarded_call(enc, hidden, layer, cu, cu_np, max_len, shape, float_offset, need):
    """op_attention_probs into a slice of a NaN-filled buffer (GUARD floats on either side, the slice ``float_offset`` floats
    behind a 16-byte boundary) with exactly ``need`` workspace bytes advertised and GUARD bytes of 0xA5 behind them -> out"""

    from open_provence_amd import _lib

    n = int(np.prod(shape))
    buffer = torch.full((GUARD + float_offset + n + GUARD,), float("nan"), dtype=torch.float32, device=enc.device)
    begin = GUARD + float_offset
    out = buffer[begin: begin + n].view(shape)
    assert out.data_ptr() % 16 == 4 * float_offset
    ws = torch.full((need + 256 + GUARD,), 0xA5, dtype=torch.uint8, device=enc.device)
    skip = (-ws.data_ptr()) % 256
    code = au.c_attention_probs(enc, hidden, layer, cu, cu_np, max_len, out, ws, ws_bytes=need)
    assert code == _lib.OP_OK, _lib.last_error(enc.lib, enc._handle)
    torch.cuda.synchronize()
    bits = buffer.view(torch.int32)
    assert bool((bits[:begin] == NAN_BITS).all()), "a write in front of out"
    assert bool((bits[begin + n:] == NAN_BITS).all()), "a write behind out"
    assert bool((ws[:skip] == 0xA5).all()) and bool((ws[skip + need:] == 0xA5).all()), "a write outside the advertised workspace bytes"
    return out


@pytest.mark.parametrize("layer", [0, 1])
def test_nothing_outside_out_and_the_workspace_is_written(layer):
    """Widths max_len + 0 .. 3 and the next tile edge + 0 and 1, `out` on a 16-byte boundary (16-byte stores where the width
    allows) and one float behind it (dwords: with a width that is a multiple of 4 the branch nothing else reaches)."""

    ref = au.probs_reference("A")
    dims, B, max_len = ref.dims, len(au.EDGE), max(au.EDGE)
    enc = au.conformance_encoder(dims, ref.state)
    try:
        hidden = ref.packed(layer).to(enc.device)
        cu_np = np.concatenate(([0], np.cumsum(au.EDGE))).astype(np.int32)
        cu = torch.from_numpy(cu_np).to(enc.device)
        need = int(enc.lib.op_attention_workspace_bytes(enc._handle, B, int(hidden.shape[0]), max_len))
        assert need > 0
        base = _guarded_call(enc, hidden, layer, cu, cu_np, max_len, (B, dims.num_heads, 324, 324), 0, need)[:, :, :max_len, :max_len].clone()
        au.check_probs("guarded A W 324", base, ref, layer)
        for width in (321, 322, 323, 324, 384, 385):
            mask = torch.zeros((B, width), dtype=torch.int64)
            for b, n in enumerate(au.EDGE):
                mask[b, :n] = 1
            for float_offset in (0, 1):
                out = _guarded_call(enc, hidden, layer, cu, cu_np, max_len, (B, dims.num_heads, width, width), float_offset, need)
                au.check_probs_pattern(f"W {width} offset {float_offset}", out, dims, mask, layer)
                assert torch.equal(out[:, :, :max_len, :max_len], base), f"W {width} offset {float_offset}: other bits than the aligned W = 324 call"
    finally:
        enc.close()


# 4. batch composition -----------------------------------------------------------------------------------------------------------------
def test_a_row_alone_equals_the_row_inside_the_batch():
    ref = au.probs_reference("B")
    enc = au.conformance_encoder(ref.dims, ref.state)
    try:
        for layer in range(ref.dims.num_layers):
            batch = au.kernel_probs(enc, ref.packed(layer), layer, au.EDGE)
            for s, n in enumerate(au.EDGE):
                alone = au.kernel_probs(enc, ref.inputs[layer][s, :n].contiguous(), layer, [n])
                assert alone.shape == (1, ref.dims.num_heads, n, n)
                assert torch.equal(alone[0], batch[s, :, :n, :n]), f"layer {layer} row {s} ({n} tokens)"
                assert bool((batch[s, :, n:, :] == 0).all()) and bool((batch[s, :, :, n:] == 0).all()), f"layer {layer} row {s}: a non-zero outside its [{n}, {n}] corner"
    finally:
        enc.close()


def test_chunked_handle_equals_the_whole_batch_handle_on_peaked_rows():
    ref = au.probs_reference("B", peaked=True)
    whole = au.conformance_encoder(ref.dims, ref.state)
    chunked = au.conformance_encoder(ref.dims, ref.state, chunk_rows=128)
    try:
        for layer in range(ref.dims.num_layers):
            a = au.kernel_probs(whole, ref.packed(layer), layer, au.EDGE)
            b = au.kernel_probs(chunked, ref.packed(layer), layer, au.EDGE)
            assert torch.equal(a, b), f"layer {layer}: chunk_rows = 128 changes the bits"
    finally:
        whole.close()
        chunked.close()


def test_empty_sequences_inside_a_batch():
    """cu_seqlens with an empty sequence first, in the middle and last: OP_OK, their matrices all +0.0, the others what the
    same rows give without them."""

    from open_provence_amd import _lib

    ref = au.probs_reference("B")
    dims = ref.dims
    lengths = [0, 65, 0, 1, 129, 0]
    full = [n for n in lengths if n]
    width = max(lengths)
    enc = au.conformance_encoder(dims, ref.state)
    try:
        for layer in range(dims.num_layers):
            packed = torch.cat([ref.inputs[layer][au.EDGE.index(n), :n] for n in full]).contiguous().to(enc.device)
            want = au.kernel_probs(enc, packed, layer, full, width)
            cu_np = np.concatenate(([0], np.cumsum(lengths))).astype(np.int32)
            cu = torch.from_numpy(cu_np).to(enc.device)
            need = int(enc.lib.op_attention_workspace_bytes(enc._handle, len(lengths), int(packed.shape[0]), width))
            for host_cu in (True, False):
                out = torch.full((len(lengths), dims.num_heads, width, width), float("nan"), dtype=torch.float32, device=enc.device)
                ws = torch.full((need + 256,), 0xFF, dtype=torch.uint8, device=enc.device)
                code = au.c_attention_probs(enc, packed, layer, cu, cu_np, width, out, ws, host_cu=host_cu)
                assert code == _lib.OP_OK, _lib.last_error(enc.lib, enc._handle)
                torch.cuda.synchronize()
                empty = [s for s, n in enumerate(lengths) if not n]
                assert bool((out[empty].view(torch.int32) == 0).all()), f"layer {layer}: an empty sequence's matrix is not all +0.0"
                assert torch.equal(out[[s for s, n in enumerate(lengths) if n]], want), f"layer {layer}: the empty sequences change the others"
    finally:
        enc.close()


LONG_LENGTHS = [4097, 0, 5]


def test_a_4097_token_row_next_to_an_empty_and_a_short_one():
    """One token past 4096 (65 key tiles, RoPE table rows beyond 2048, window ranges far from the row's start) on the first
    full-attention and the first sliding-window layer of the 4-head trained-like model, pad_width 4097: each real row within
    the module's bound of the fp64 restatement of that row alone, exact +0.0 outside the visible keys and in the whole matrix of
    the empty sequence, nothing written around ``out`` or behind the advertised workspace bytes."""

    from open_provence_amd.synthetic import pad_rows
    from oracle.modernbert_oracle import oracle_forward

    torch.set_num_threads(16)
    dims, state = au.conformance_model("T")
    assert dims.num_heads == 4 and dims.max_position_embeddings >= max(LONG_LENGTHS)
    kinds = [bool(g) for g in dims.layer_is_global]
    layers = [kinds.index(True), kinds.index(False)]
    real = [n for n in LONG_LENGTHS if n]
    ids, mask = pad_rows(au.edge_rows(real, vocab=dims.vocab_size))
    hidden = oracle_forward(state, dims, ids, mask, dtype=torch.float64, return_hidden=True).hidden_states
    width, B = max(LONG_LENGTHS), len(LONG_LENGTHS)
    cu_np = np.concatenate(([0], np.cumsum(LONG_LENGTHS))).astype(np.int32)
    enc = au.conformance_encoder(dims, state)
    try:
        cu = torch.from_numpy(cu_np).to(enc.device)
        need = int(enc.lib.op_attention_workspace_bytes(enc._handle, B, int(cu_np[-1]), width))
        assert need > 0
        for layer in layers:
            h32 = hidden[layer].to(torch.float32)
            packed = h32[mask.bool()].contiguous().to(enc.device)
            got = _guarded_call(enc, packed, layer, cu, cu_np, width, (B, dims.num_heads, width, width), 0, need).cpu()
            err = e_ref = 0.0
            source = iter(range(len(real)))
            for s, n in enumerate(LONG_LENGTHS):
                if not n:
                    assert bool((got[s].view(torch.int32) == 0).all()), f"layer {layer}: the empty sequence's matrix is not all +0.0"
                    continue
                row_mask = torch.zeros((1, width), dtype=torch.int64)
                row_mask[0, :n] = 1
                au.check_probs_pattern(f"long row {s} ({n} tokens)", got[s: s + 1], dims, row_mask, layer)
                alone, ones = h32[next(source)][None, :n], torch.ones((1, n), dtype=torch.int64)
                want = au.attention_probs(state, dims, alone, ones, layer, torch.float64)
                e_ref = max(e_ref, float((au.attention_probs(state, dims, alone, ones, layer, torch.float32).double() - want).abs().max()))
                err = max(err, float((got[s, :, :n, :n].double() - want[0]).abs().max()))
            bound = au.probs_bound(e_ref)
            print(f"[attn-conf] {'kernel T rows 4097+0+5':30s} layer {layer}  err {err:.3e}  e_ref {e_ref:.3e}  err/e_ref {err / max(e_ref, 1e-30):6.2f}  "
                  f"bound {bound:.3e}")
            assert err <= bound, f"layer {layer}: {err:.3e} from the fp64 restatement, bound {bound:.3e} (e_ref {e_ref:.3e})"
    finally:
        enc.close()


# 5. end to end on kernel set "fp32" ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["A", "T"])
def test_forward_on_the_fp32_set_within_four_times_the_oracle_error(name):
    from open_provence_amd.engine import AttentionRequest

    ref = au.forward_reference(name)
    enc = au.conformance_encoder(ref.dims, ref.state, kernel_set="fp32")
    try:
        assert enc.effective_policy()["kernel_set"] == "fp32"
        ids, cu, cu_np, max_len = au.packed_batch(enc, ref.rows)
        *_, probs = enc.forward_packed(ids, cu, cu_np, max_len, attentions=AttentionRequest())
        assert len(probs) == ref.dims.num_layers
        for layer, got in enumerate(probs):
            au.check_probs(f"forward fp32 {name}", got, ref, layer)
    finally:
        enc.close()
