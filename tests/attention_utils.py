"""Attention probabilities of one layer restated from that layer's input hidden state (test infrastructure): what
``op_attention_probs`` computes, in any dtype, on top of the oracle's own pieces.  fp64 from the oracle's fp64 hidden states is
the yardstick the attention fixtures carry their own distance to (``ref_to_fp64``)."""

from __future__ import annotations

import ctypes
import functools

import numpy as np
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


def uniform_probs(dims, attention_mask: torch.Tensor, layer: int) -> torch.Tensor:
    """``[B, L, L]`` fp64, the same for every head: what a layer gives on q = k = 0 (a zero hidden state: no tensor has a
    bias) -- ``1 / count`` at each of the ``count`` keys a query sees, 0 elsewhere and on padded query rows."""

    vis = visible_mask(dims, attention_mask, layer)
    count = vis.sum(-1, keepdim=True).clamp(min=1).double()
    return torch.where(vis, 1.0 / count, torch.zeros((), dtype=torch.float64))


# ---- conformance of the kernel alone (tests/test_attention_reference.py, tests/test_gpu_attention_conformance.py) ---------------
# Sequence ends on, before and after a 64-key tile edge and a 16-row wave edge; up to 6 query blocks x 6 key tiles.
EDGE = [321, 257, 193, 129, 128, 127, 65, 64, 63, 17, 16, 2, 1]
ULP_ONE = float(np.spacing(np.float32(1.0)))  # a probability is at most 1
# name -> (hidden, heads, layer pattern, local_attention); "T" is the trained-like proxy (conformance_model)
CONFORMANCE_MODELS = {"A": (128, 2, "GLL", 16), "B": (384, 6, "LGL", 128), "C": (768, 12, "LG", 6)}


def small_dims(hidden: int, heads: int, pattern: str, window: int):
    """As ``test_gpu_fp32_set._small_dims`` (vocab 512, intermediate 192), with one layer per letter of ``pattern``."""

    from open_provence_amd.config import EncoderDims

    cfg = dict(model_type="modernbert", vocab_size=512, hidden_size=hidden, intermediate_size=192, num_hidden_layers=len(pattern),
               num_attention_heads=heads, local_attention=window, global_attn_every_n_layers=3, global_rope_theta=160000.0,
               local_rope_theta=10000.0, max_position_embeddings=2048, pad_token_id=0, cls_token_id=1, sep_token_id=2,
               layer_types=["full_attention" if t == "G" else "sliding_attention" for t in pattern], classifier_pooling="cls")
    return EncoderDims.from_base_model_config(cfg, num_labels=1)


def edge_rows(lengths=EDGE, seed: int = 7, vocab: int = 512) -> list[list[int]]:
    """As ``test_gpu_fp32_set._rows``: ``[1] +`` uniform ids."""

    rng = np.random.default_rng(seed)
    return [[1] + rng.integers(3, vocab, n - 1).tolist() for n in lengths]


@functools.lru_cache(maxsize=None)
def conformance_model(name: str, weights: str = "synth"):
    """-> (dims, state) of model A / B / C with ``synth`` or ``refinit`` weights, or of "T", the trained-like proxy."""

    from open_provence_amd.synthetic import named_dims, refinit_state_dict, synth_state_dict, trained_like_state_dict

    if name == "T":
        dims = named_dims("xsmall", num_hidden_layers=4, vocab_size=2048)
        return dims, trained_like_state_dict(dims, 7, outlier_range=(30, 100))
    dims = small_dims(*CONFORMANCE_MODELS[name])
    return dims, (refinit_state_dict if weights == "refinit" else synth_state_dict)(dims, 5)


PEAK_GAIN = 4.0


def peaked_state(state, gain: float = PEAK_GAIN):
    """A copy of ``state`` with every ``attn_norm.weight`` times ``gain``: q and k grow by ``gain``, the scores by its square.
    (Layer 0 has no norm: its INPUT takes the factor, ``probs_reference(peaked=True)``.)"""

    return {k: v * gain if k.endswith("attn_norm.weight") else v for k, v in state.items()}


@functools.lru_cache(maxsize=None)
def _oracle_hidden(name: str, weights: str, dtype: torch.dtype):
    """-> (hidden states of the oracle in ``dtype`` on the EDGE batch, attention mask, rows)"""

    from open_provence_amd.synthetic import pad_rows
    from oracle.modernbert_oracle import oracle_forward

    dims, state = conformance_model(name, weights)
    rows = edge_rows(vocab=dims.vocab_size)
    ids, mask = pad_rows(rows)
    return oracle_forward(state, dims, ids, mask, dtype=dtype, return_hidden=True).hidden_states, mask, rows


def probs_bound(e_ref: float) -> float:
    """The project's bound (test_gpu_fp32_set.py) on a probability: ``max(4 x e_ref, 16 ulp of 1.0)``."""

    return max(4.0 * e_ref, 16.0 * ULP_ONE)


class ProbsReference:
    """Per layer of one model on the EDGE batch: the fp32 input ``inputs[i]`` ``[B, L, H]`` every implementation is fed, its
    attention probabilities in fp64 ``p64[i]`` and ``e_ref[i]`` = max |fp32 restatement - fp64| on those same bits."""

    def __init__(self, dims, state, rows, mask, inputs, p64, e_ref):
        self.dims, self.state, self.rows, self.mask = dims, state, rows, mask
        self.inputs, self.p64, self.e_ref = inputs, p64, e_ref

    def packed(self, layer: int) -> torch.Tensor:
        """``inputs[layer]`` as the packed ``[T, H]`` fp32 state ``HipEncoder.attention_probs`` takes"""

        return self.inputs[layer][self.mask.bool()].contiguous()

    def median_row_max(self, layer: int) -> float:
        """Median over real queries (and heads) of the largest probability of the row, in fp64."""

        top = self.p64[layer].max(dim=-1).values  # [B, heads, L]
        return float(top[self.mask.bool()[:, None, :].expand_as(top)].median())


@functools.lru_cache(maxsize=None)
def probs_reference(name: str, weights: str = "synth", peaked: bool = False) -> ProbsReference:
    """The kernel alone: ``hidden_states[i]`` of the fp64 oracle rounded to fp32, restated in fp64 and fp32 from those bits.
    ``peaked``: ``peaked_state`` of the weights, layer 0's input times ``PEAK_GAIN``, the same inputs otherwise."""

    dims, state = conformance_model(name, weights)
    hidden, mask, rows = _oracle_hidden(name, weights, torch.float64)
    if peaked:
        state = peaked_state(state)
    inputs, p64, e_ref = [], [], []
    for i in range(dims.num_layers):
        h32 = (hidden[i] * PEAK_GAIN if peaked and i == 0 else hidden[i]).to(torch.float32)
        want = attention_probs(state, dims, h32, mask, i, torch.float64)
        e_ref.append(float((attention_probs(state, dims, h32, mask, i, torch.float32).double() - want).abs().max()))
        inputs.append(h32)
        p64.append(want)
    return ProbsReference(dims, state, rows, mask, inputs, p64, e_ref)


@functools.lru_cache(maxsize=None)
def forward_reference(name: str, weights: str = "synth") -> ProbsReference:
    """End to end: the fp64 oracle's attentions (its own fp64 hidden states) and, as ``e_ref``, the distance of the fp32
    oracle's attentions (fp32 hidden states, fp32 restatement) to them -- the forward's own rounding included."""

    dims, state = conformance_model(name, weights)
    h64, mask, rows = _oracle_hidden(name, weights, torch.float64)
    h32, _, _ = _oracle_hidden(name, weights, torch.float32)
    p64 = [attention_probs(state, dims, h64[i], mask, i, torch.float64) for i in range(dims.num_layers)]
    e_ref = [float((attention_probs(state, dims, h32[i], mask, i, torch.float32).double() - p64[i]).abs().max())
             for i in range(dims.num_layers)]
    return ProbsReference(dims, state, rows, mask, None, p64, e_ref)


def check_probs_pattern(label: str, a: torch.Tensor, dims, mask: torch.Tensor, layer: int) -> None:
    """``a[B, heads, W, W]`` (``mask[B, W]``): finite, no negative zero, exactly 0 wherever ``visible_mask`` is False, real rows
    sum to 1 within 1e-5 in fp64, padded rows to exactly 0."""

    a = a.cpu()
    assert bool(torch.isfinite(a).all()), f"{label} layer {layer}: not finite"
    assert not bool(torch.signbit(a).any()), f"{label} layer {layer}: a negative zero (or a negative value)"
    vis = visible_mask(dims, mask, layer)[:, None].expand_as(a)
    assert bool((a[~vis] == 0).all()), f"{label} layer {layer}: a non-zero where the mask hides the key"
    sums = a.double().sum(-1)
    real = mask.bool()[:, None, :].expand_as(sums)
    assert float((sums[real] - 1.0).abs().max()) <= 1e-5, f"{label} layer {layer}: a real row does not sum to 1"
    assert bool((sums[~real] == 0).all()), f"{label} layer {layer}: a padded row is not zero"


def check_probs(label: str, got: torch.Tensor, ref: ProbsReference, layer: int) -> float:
    """The pattern, then max |got - fp64| <= max(4 x e_ref, 16 ulp(1.0)); prints and returns ``err / e_ref``."""

    check_probs_pattern(label, got, ref.dims, ref.mask, layer)
    err = float((got.cpu().double() - ref.p64[layer]).abs().max())
    e_ref, bound = ref.e_ref[layer], probs_bound(ref.e_ref[layer])
    ratio = err / max(e_ref, 1e-30)
    print(f"[attn-conf] {label:30s} layer {layer}  err {err:.3e}  e_ref {e_ref:.3e}  err/e_ref {ratio:6.2f}  bound {bound:.3e}")
    assert err <= bound, f"{label} layer {layer}: {err:.3e} from the fp64 restatement, bound {bound:.3e} (e_ref {e_ref:.3e})"
    return ratio


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


def c_attention_probs(enc, hidden, layer, cu, cu_np, max_len, out, ws, host_cu=True, ws_bytes=None):
    """op_attention_probs with the caller's own output and workspace tensors (host_cu=False: no host copy of cu_seqlens, the call
    reads it back; ws_bytes: the workspace size to advertise instead of everything behind the 256-aligned base) -> the return code"""

    from open_provence_amd import _lib

    vp = ctypes.c_void_p
    req = _lib.OpAttentionRequest()
    req.struct_bytes = ctypes.sizeof(_lib.OpAttentionRequest)
    req.layer, req.dtype, req.pad_width = layer, _lib.OP_HIDDEN_F32, int(out.shape[-1])
    req.hidden_dev, req.out_dev = vp(hidden.data_ptr()), vp(out.data_ptr())
    base = ws.data_ptr()
    aligned = (base + 255) // 256 * 256
    size = ws.numel() - (aligned - base) if ws_bytes is None else int(ws_bytes)
    assert 0 <= size <= ws.numel() - (aligned - base)
    return enc.lib.op_attention_probs(enc._handle, vp(cu.data_ptr()), cu_np.ctypes.data_as(vp) if host_cu else None, len(cu_np) - 1, int(hidden.shape[0]), max_len,
                                      ctypes.byref(req), vp(aligned), ctypes.c_size_t(size),
                                      vp(torch.cuda.current_stream(enc.device).cuda_stream))


def conformance_encoder(dims, state, **kw):
    """-> a handle with the fp32 packs and ``state``, no calibration"""

    from open_provence_amd.engine import HipEncoder

    enc = HipEncoder(dims, device="cuda:0", attention_outputs=True, **kw)
    try:
        enc.load_state_dict(state, calibrate=False, **({"kernel_set": kw["kernel_set"]} if kw.get("kernel_set") else {}))
    except BaseException:
        enc.close()
        raise
    return enc


def kernel_probs(enc, packed: torch.Tensor, layer: int, lengths, pad_width: int = 0) -> torch.Tensor:
    """``HipEncoder.attention_probs`` on a host ``[T, H]`` fp32 state of sequences of ``lengths`` (zeros allowed)"""

    cu_np = np.concatenate(([0], np.cumsum(lengths))).astype(np.int32)
    assert int(cu_np[-1]) == int(packed.shape[0])
    cu = torch.from_numpy(cu_np).to(enc.device)
    return enc.attention_probs(packed.to(enc.device), layer, cu, cu_np, int(max(lengths)), pad_width)
