"""Attention probabilities of one layer restated from that layer's input hidden state (test infrastructure): what
``op_attention_probs`` computes, in any dtype, on top of the oracle's own pieces.  fp64 from the oracle's fp64 hidden states is
the yardstick the attention fixtures carry their own distance to (``ref_to_fp64``)."""

from __future__ import annotations

import torch

from oracle.modernbert_oracle import _layer_norm, _rotate_half, rope_tables


def attention_probs(state, dims, hidden: torch.Tensor, attention_mask: torch.Tensor, layer: int,
                    dtype: torch.dtype = torch.float64) -> torch.Tensor:
    """``hidden[B, L, H]`` = ``hidden_states[layer]`` (the INPUT of that layer) -> softmax probabilities ``[B, heads, L, L]``:
    keys beyond a row's length and, on a sliding layer, beyond ``half_window`` are exactly 0; so are padded query rows."""

    pre = "ranking_model." if any(k.startswith("ranking_model.") for k in state) else ""
    B, L, H = hidden.shape
    nh = dims.num_heads
    hd = H // nh
    x = hidden.to(dtype)
    p = f"{pre}model.layers.{layer}."
    h = x if layer == 0 else _layer_norm(x, state[p + "attn_norm.weight"].to(dtype), float(dims.norm_eps))
    qk = h @ state[p + "attn.Wqkv.weight"].to(dtype)[: 2 * H].T
    q, k = (qk.view(B, L, 2, nh, hd)[:, :, j].transpose(1, 2) for j in range(2))
    is_global = bool(dims.layer_is_global[layer])
    positions = torch.arange(L)
    cos, sin = (t.to(dtype) for t in rope_tables(hd, dims.global_rope_theta if is_global else dims.local_rope_theta, positions))
    q = q * cos + _rotate_half(q) * sin
    k = k * cos + _rotate_half(k) * sin
    key_ok = attention_mask.to(torch.bool)
    visible = key_ok[:, None, None, :].expand(B, 1, L, L)
    if not is_global:
        visible = visible & ((positions[:, None] - positions[None, :]).abs() <= dims.half_window)[None, None]
    scores = ((q * hd**-0.5) @ k.transpose(2, 3)).masked_fill(~visible, float("-inf"))
    # (a padded query of a sliding layer may see no key at all: its row is zeroed below, NaN or not)
    probs = torch.softmax(scores, dim=-1)
    return torch.where(key_ok[:, None, :, None], probs, torch.zeros((), dtype=dtype))


def visible_mask(dims, attention_mask: torch.Tensor, layer: int) -> torch.Tensor:
    """``[B, L, L]`` bool: query i of row b may put probability on key j (real query, real key, inside the window)."""

    key_ok = attention_mask.to(torch.bool)
    L = key_ok.shape[1]
    vis = key_ok[:, :, None] & key_ok[:, None, :]
    if not dims.layer_is_global[layer]:
        positions = torch.arange(L)
        vis = vis & ((positions[:, None] - positions[None, :]).abs() <= dims.half_window)[None]
    return vis


# ---- GPU side: one fixture through HipEncoder, kernel set by kernel set (tests/test_gpu_attentions.py, scripts/attention_bounds.py)
def fixture_encoder(name: str, **kw):
    """-> (encoder with the fp32 packs and the fixture's weights, no calibration; arrays; meta; rows)"""

    from helpers import dims_from_meta, load_golden, rows_from_fixture, state_from_fixture
    from open_provence_amd.engine import HipEncoder

    arrays, meta = load_golden(name)
    kw.setdefault("attention_outputs", True)
    enc = HipEncoder(dims_from_meta(meta), device="cuda:0", **kw)
    enc.load_state_dict(state_from_fixture(arrays, meta), calibrate=False)
    return enc, arrays, meta, rows_from_fixture(arrays)


def selectable_sets(enc) -> list[str]:
    """The kernel sets this handle can pin, in the ABI's numbering order (the handle is left on the last one)."""

    from open_provence_amd import _lib

    names = []
    for number in sorted(_lib.KERNEL_SET_NAMES):
        if number < 0:
            continue
        try:
            enc.select_kernel_set(_lib.KERNEL_SET_NAMES[number])
        except _lib.HipLibraryError:
            continue
        names.append(_lib.KERNEL_SET_NAMES[number])
    return names


def packed_batch(enc, rows):
    from open_provence_amd.packing import pack_rows

    ids_np, cu_np, max_len = pack_rows(rows)
    return torch.from_numpy(ids_np).to(enc.device), torch.from_numpy(cu_np).to(enc.device), cu_np, max_len


def fixture_errors(enc, arrays, meta, rows) -> list[float]:
    """Per layer: max |attentions of a forward on the encoder's current kernel set - fixture| at the stored query rows."""

    from open_provence_amd.engine import AttentionRequest

    ids, cu, cu_np, max_len = packed_batch(enc, rows)
    width = int(arrays["input_ids"].shape[1])
    *_, probs = enc.forward_packed(ids, cu, cu_np, max_len, attentions=AttentionRequest(pad_width=width))
    stride = int(meta["query_stride"])
    return [float((p[:, :, ::stride].cpu() - torch.from_numpy(arrays[f"attn_{i}"])).abs().max()) for i, p in enumerate(probs)]
