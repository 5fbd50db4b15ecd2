"""Float64 CPU model of each kernel set's arithmetic (test infrastructure, not product code).

The forward of ``oracle/modernbert_oracle.py`` restated so that every contraction goes through one function,
:func:`contract`, which rounds its two operands the way a kernel set does for that contraction family (products and
sums stay in float64: what is modelled is the operand representation, not the accumulation order).  With the
``"exact"`` scheme the model IS the float64 oracle (``tests/test_arith_model.py`` holds it to 1e-10).

Families ("left" is always the activation-side operand; ``_lib.OP_FAMILIES``):
  wqkv: LN(x) x Wqkv    qk: q x k    pv: p x v    attn_out: o x Wo    wi: LN(x) x Wi    mlp_out: GeGLU(..) x Wo

Schemes of one family (the operand formats of ``include/open_provence_hip.h`` and ``opk_common.hip.h``):
  exact        no rounding
  bf16 / f16   single pass, both operands RNE bf16 / fp16
  bf16x2       left as a (hi, lo) bf16 pair, right bf16                  (term mask 1: no lo(weight) term)
  bf16x3       both operands as (hi, lo) bf16 pairs, lo x lo dropped      (term mask 3)
  f16x2, f16x3 the same with fp16 pairs
  f16+f8       left = fp16 hi + e4m3((left - hi) x 2^12); hi x fp16(right) + lo x e4m3(right x 2^6)
  f16+2f8      f16+f8 plus e4m3(left) x e4m3((right - fp16(right)) x 2^18)   (the weight's lo part as a third plane)

What the kernels compute on purpose and the model restates (rather than a bound widened for it):
  * the score scale 1/sqrt(head_dim) and log2(e) are folded into q BEFORE q is rounded; the softmax is 2^(s - m);
  * the softmax reference m is the lazy running reference of ``opk_attn.hip.h``: key tiles of 64 (full attention) or 32
    (sliding window) keys in order, m = the first visible tile's maximum, moved to a later tile's maximum only when that
    exceeds m by more than 2^6 (:data:`RESCALE_LOG2`).  p = 2^(s - m) <= 2^6 is rounded RELATIVE TO THAT m;
  * the row sum l: the fp16 attention (kernel sets 7 - 11) sums the ROUNDED p on the matrix pipe, the bf16 attention
    sums the unrounded p in fp32;
  * kernel sets 3 / 4 on the row path run layer 0's q / k / v projection on the kernels of sets 1 / 0 and their attention
    at 3-term bf16 (sets 1 / 0 too); o is written in the fp16 + e4m3 format for the output projection, and the
    whole-layer kernel carries the MLP activation h as an fp16 (hi, lo) pair (K is streamed 32 at a time: too short for
    the e4m3 shape) against fp16(W) (set 3) plus fp16(W - fp16(W)) (set 4): schemes f16x2 / f16x3.  The panel path keeps
    every family of those sets in the fp16 + e4m3 format;
  * kernel sets 8 / 9 under a layer mask (op_select_mlp_correction_layers): a layer outside the mask runs the "f16" set's
    MLP -- single-plane fp16 LN(x), Wi and MLP output projection on the fp16 packs (``Arith.mlp_layers``).

Not modelled (below the 1e-6 floor of the comparison, or outside what a contraction sees): fp32 accumulation order,
fp32 LayerNorm / GELU / RoPE / softmax exponent, the fp32 residual stream, fp16 subnormal flushing of p below 2^-24.
The operand roundings above (:func:`rne`, :func:`e4m3`) and the fp32 GELU / exponent / RoPE / keep-probability are held to the
device's element by element in tests/test_gpu_primitives.py.  Where the device departs from them, on inputs no forward reaches:
under saturating conversions a finite value beyond bf16's range (|v| >= 0x7f7f8000) becomes +-max bf16 where :func:`rne` gives
Inf; a weight whose fp32 product with 2^6 (its lo part: with 2^18) is infinite, |w| >= 2^122 (2^110), packs as NaN where
:func:`e4m3` clamps to 448; NaN payloads are not compared.
"""

from __future__ import annotations

import math
from dataclasses import dataclass, replace
from typing import Mapping, Sequence

import torch

FAMILIES = ("wqkv", "qk", "pv", "attn_out", "wi", "mlp_out")
F8 = torch.float8_e4m3fn
LO_SHIFT = 12  # e4m3 lo planes are stored x 2^12 (opk_common.hip.h F8_LO_SHIFT)
W_SHIFT = 6  # e4m3 planes of a weight are stored x 2^6, its lo plane x 2^18 (F8_W_SHIFT)
RESCALE_LOG2 = 6.0  # the lazy softmax reference moves when a tile's maximum exceeds it by more than this (log2 units)
TILE_KEYS_GLOBAL, TILE_KEYS_LOCAL = 64, 32  # key tiles of the full-attention / sliding-window attention kernels
LOG2E = 1.0 / math.log(2.0)


# -- operand formats ------------------------------------------------------------------------------------------------------
def rne(x: torch.Tensor, dtype: torch.dtype) -> torch.Tensor:
    """RNE to ``dtype`` from the fp32 value the kernels hold, back to float64."""

    return x.to(torch.float32).to(dtype).to(torch.float64)


def e4m3(x: torch.Tensor, shift: int = 0, decode_shift: "int | None" = None) -> torch.Tensor:
    """e4m3(x * 2^shift) / 2^decode_shift with the kernels' saturating conversion (decode_shift defaults to shift)."""

    y = (x.to(torch.float32) * 2.0**shift).clamp(-448.0, 448.0).to(F8).to(torch.float64)
    return y / 2.0 ** (shift if decode_shift is None else decode_shift)


@dataclass(frozen=True)
class Scheme:
    """One family's operand format.  ``hi``: dtype of the hi (or only) operands, None = exact; ``left_lo`` /
    ``right_lo``: "" (no lo term), "pair" (lo in the dtype of hi) or "e4m3" (the fp16 + e4m3 format); ``lo_decode``:
    mutation hook, the shift the e4m3 lo planes are decoded with (None = LO_SHIFT, what they are encoded with)."""

    name: str
    hi: "torch.dtype | None" = None
    left_lo: str = ""
    right_lo: str = ""
    lo_decode: "int | None" = None


BF16, F16 = torch.bfloat16, torch.float16
SCHEMES = {
    "exact": Scheme("exact"),
    "bf16": Scheme("bf16", BF16),
    "bf16x2": Scheme("bf16x2", BF16, "pair"),
    "bf16x3": Scheme("bf16x3", BF16, "pair", "pair"),
    "f16": Scheme("f16", F16),
    "f16x2": Scheme("f16x2", F16, "pair"),
    "f16x3": Scheme("f16x3", F16, "pair", "pair"),
    "f16+f8": Scheme("f16+f8", F16, "e4m3"),
    "f16+2f8": Scheme("f16+2f8", F16, "e4m3", "e4m3"),
}


def contract(left: torch.Tensor, right: torch.Tensor, scheme: "Scheme | str") -> torch.Tensor:
    """left [..., K] @ right [..., K, N] in float64 with the scheme's operand roundings."""

    s = SCHEMES[scheme] if isinstance(scheme, str) else scheme
    a, b = left.to(torch.float64), right.to(torch.float64)
    if s.hi is None:
        return a @ b
    ah, bh = rne(a, s.hi), rne(b, s.hi)
    out = ah @ bh
    dec = LO_SHIFT if s.lo_decode is None else s.lo_decode
    if s.left_lo == "pair":
        out = out + rne(a - ah, s.hi) @ bh
    elif s.left_lo == "e4m3":
        out = out + e4m3(a - ah, LO_SHIFT, dec) @ e4m3(b, W_SHIFT)
    if s.right_lo == "pair":
        out = out + ah @ rne(b - bh, s.hi)
    elif s.right_lo == "e4m3":
        out = out + e4m3(a) @ e4m3(b - bh, LO_SHIFT + W_SHIFT, dec + W_SHIFT)
    return out


# -- the kernel sets (numbering and names of _lib.KERNEL_SET_NAMES) -----------------------------------------------------------
def _table(*schemes: str) -> dict[str, str]:
    return dict(zip(FAMILIES, schemes))


_BF16X3 = _table(*["bf16x3"] * 6)
_BF16W = _table("bf16x2", "bf16x3", "bf16x3", "bf16x2", "bf16x2", "bf16x2")
_F16F8 = _table("f16+f8", "bf16x3", "bf16x3", "f16+f8", "f16+f8", "f16+f8")
_F16F8W = _table("f16+2f8", "bf16x3", "bf16x3", "f16+2f8", "f16+2f8", "f16+2f8")
_F16 = _table(*["f16"] * 6)

# Set name -> per-family scheme.  From op_policy.h kPolicies (term masks 3 = bf16x3, 1 = bf16x2, 0 = single pass;
# fmt 1 = the fp16 + e4m3 format, fmt 2 = fp16 single plane), kKernelSets in op_kernel_sets.h (which families a composite set
# takes from which) and the set descriptions of include/open_provence_hip.h.  Row-path departures: ROW_PATH below.
KERNEL_SETS: dict[str, dict[str, str]] = {
    "bf16x3": _BF16X3,                                           # 0: every operand (hi, lo)
    "bf16-weights": _BF16W,                                      # 1: no lo(weight) term, attention all terms
    "bf16": _table(*["bf16"] * 6),                               # 2: single pass
    "f16-f8": _F16F8,                                            # 3: terms of 1 in the fp16 + e4m3 format
    "f16-f8-w": _F16F8W,                                         # 4: terms of 0 in that format, lo(W) as a third plane
    "bf16x3+wi-f16-f8-w": {**_BF16X3, "wi": "f16+2f8"},          # 5: set 0, the Wi GEMM in the format of 4 (panel)
    "bf16-weights+wi-f16-f8": {**_BF16W, "wi": "f16+f8"},        # 6: set 1, the Wi GEMM in the format of 3 (panel)
    "f16": _F16,                                                 # 7: single pass fp16
    "f16+mlp-f16-f8-w": {**_F16, "wi": "f16+2f8", "mlp_out": "f16+2f8"},  # 8: attention side of 7, MLP of 4 (panel)
    "f16+mlp-f16-f8": {**_F16, "wi": "f16+f8", "mlp_out": "f16+f8"},      # 9: attention side of 7, MLP of 3 (panel)
    "f16-f8-w+attn-f16": {**_F16F8W, "qk": "f16", "pv": "f16"},           # 10: set 4, attention single pass fp16 (panel)
    "f16-f8+attn-f16": {**_F16F8, "qk": "f16", "pv": "f16"},              # 11: set 3, attention single pass fp16 (panel)
}
# sets that drop the lo(W) term while carrying lo terms elsewhere: made for bf16-valued checkpoints (tested on them)
WEIGHT_FAMILIES = ("wqkv", "attn_out", "wi", "mlp_out")
BF16_WEIGHT_SETS = tuple(n for n, t in KERNEL_SETS.items()
                         if not any(SCHEMES[t[f]].right_lo for f in WEIGHT_FAMILIES) and any(SCHEMES[v].left_lo for v in t.values()))
# composite set -> the set whose kernels it replaces in some families (a composite silently running them must be seen)
BASE_SET = {"bf16x3+wi-f16-f8-w": "bf16x3", "bf16-weights+wi-f16-f8": "bf16-weights", "f16+mlp-f16-f8-w": "f16",
            "f16+mlp-f16-f8": "f16", "f16-f8-w+attn-f16": "f16-f8-w", "f16-f8+attn-f16": "f16-f8"}
# kernel sets 8 / 9 take a per-layer mask: outside it the two MLP families run at the "f16" set's scheme
MLP_FAMILIES = ("wi", "mlp_out")
MASKED_SETS = ("f16+mlp-f16-f8-w", "f16+mlp-f16-f8")
# row path (hidden <= 256): (layer 0's wqkv scheme, mlp_out scheme) of sets 3 / 4 -- see the module docstring
ROW_PATH = {"f16-f8": ("bf16x2", "f16x2"), "f16-f8-w": ("bf16x3", "f16x3")}


@dataclass(frozen=True)
class Arith:
    """What one model forward computes: a scheme per family, layer 0's wqkv scheme, and the knobs mutations turn."""

    schemes: Mapping[str, Scheme]
    layer0_wqkv: "Scheme | None" = None
    window_delta: int = 0  # added to half_window of the sliding-window layers (mutation: -1 = one key short)
    # kernel sets 8 / 9 layer by layer (op_select_mlp_correction_layers): the layers whose MLP keeps the fp16 + e4m3
    # format; in every other layer wi and mlp_out run on the "f16" set's kernels.  None = the whole depth.
    mlp_layers: "frozenset[int] | None" = None

    def scheme(self, family: str, layer: int) -> Scheme:
        if family == "wqkv" and layer == 0 and self.layer0_wqkv is not None:
            return self.layer0_wqkv
        if family in MLP_FAMILIES and self.mlp_layers is not None and layer not in self.mlp_layers:
            return SCHEMES["f16"]
        return self.schemes[family]

    def with_family(self, family: str, scheme: Scheme) -> "Arith":
        return replace(self, schemes={**self.schemes, family: scheme})


def arith_for(kernel_set: str, path: str = "row", mlp_layers: "Sequence[int] | None" = None) -> Arith:
    """The model of ``kernel_set`` ("exact" or a name of :data:`KERNEL_SETS`) on ``path`` ("row" / "panel" / "tiled").
    ``mlp_layers``: the layer mask of kernel sets 8 / 9 (the layers that keep the fp16 + e4m3 MLP; None = all)."""

    if kernel_set == "exact":
        return Arith({f: SCHEMES["exact"] for f in FAMILIES})
    table = dict(KERNEL_SETS[kernel_set])
    layer0 = None
    if path == "row" and kernel_set in ROW_PATH:
        layer0, table["mlp_out"] = ROW_PATH[kernel_set]
    if mlp_layers is not None and kernel_set not in MASKED_SETS:
        raise ValueError(f"a layer mask applies to {MASKED_SETS}, not to {kernel_set!r}")
    return Arith({f: SCHEMES[v] for f, v in table.items()}, SCHEMES[layer0] if layer0 else None,
                 mlp_layers=None if mlp_layers is None else frozenset(int(li) for li in mlp_layers))


# -- forward ----------------------------------------------------------------------------------------------------------------
def _layer_norm(x, w, eps):
    mean = x.mean(dim=-1, keepdim=True)
    var = ((x - mean) ** 2).mean(dim=-1, keepdim=True)
    return (x - mean) / torch.sqrt(var + eps) * w


def _gelu(x):
    return 0.5 * x * (1.0 + torch.erf(x / math.sqrt(2.0)))


def _rope(head_dim: int, theta: float, n: int):
    inv = 1.0 / (theta ** (torch.arange(0, head_dim, 2, dtype=torch.float32) / head_dim))
    fr = torch.arange(n, dtype=torch.float32)[:, None] * inv[None, :]
    emb = torch.cat((fr, fr), dim=-1)
    return emb.cos().double(), emb.sin().double()


def _rot(x):
    h = x.shape[-1] // 2
    return torch.cat((-x[..., h:], x[..., :h]), dim=-1)


def visible(n: int, half_window: "int | None") -> torch.Tensor:
    """[n, n] bool: key j visible from query i (|i - j| <= half_window; None = full attention)."""

    if half_window is None:
        return torch.ones(n, n, dtype=torch.bool)
    pos = torch.arange(n)
    return (pos[:, None] - pos[None, :]).abs() <= half_window


def lazy_reference(s: torch.Tensor, vis: torch.Tensor, tile: int) -> tuple[torch.Tensor, torch.Tensor]:
    """The kernels' running softmax reference of every query: s [..., n_q, n_k] scores in log2 units, vis [n_q, n_k].
    Returns (m [..., n_q, 1], late [..., n_q] bool: the reference moved after the query's first visible tile)."""

    n_k = s.shape[-1]
    n_t = (n_k + tile - 1) // tile
    sm = torch.nn.functional.pad(s.masked_fill(~vis, -math.inf), (0, n_t * tile - n_k), value=-math.inf)
    tmax = sm.view(*sm.shape[:-1], n_t, tile).amax(dim=-1)  # [..., n_q, n_t]
    m = torch.full(s.shape[:-1], -math.inf, dtype=s.dtype)
    late = torch.zeros(s.shape[:-1], dtype=torch.bool)
    for t in range(n_t):
        tm = tmax[..., t]
        fresh = torch.isinf(m)
        moved = torch.where(fresh, torch.isfinite(tm), tm > m + RESCALE_LOG2)
        late |= moved & ~fresh
        m = torch.where(moved, tm, m)
    return m[..., None], late


def attention(q, k, v, vis, arith: Arith, layer: int, tile: int):
    """q / k / v [heads, n, hd] float64 (q already scaled by head_dim^-0.5 * log2(e)); returns o [heads, n, hd]."""

    sqk, spv = arith.scheme("qk", layer), arith.scheme("pv", layer)
    s = contract(q, k.transpose(-1, -2), sqk)
    if sqk.hi is None:  # exact: the reference is the true maximum (it cancels in an exact softmax)
        m = s.masked_fill(~vis, -math.inf).amax(dim=-1, keepdim=True)
    else:
        m, _ = lazy_reference(s, vis, tile)
    p = torch.exp2(s - m).masked_fill(~vis, 0.0)
    fsm = sqk.hi is F16  # the fp16 attention sums the rounded p
    l = (rne(p, F16) if fsm else p).sum(dim=-1, keepdim=True)
    o = contract(p, v, spv) / l
    if bool(vis.any(dim=-1).all()):
        return o
    return o.masked_fill(~vis.any(dim=-1)[..., None], 0.0)  # (only a mutated mask hides every key of a query: its output is 0)


def rank_logits(state: Mapping[str, torch.Tensor], dims, last_rows: Sequence[torch.Tensor], pool=None) -> torch.Tensor:
    """The ranking head on the final_norm output of every row ([len, H] each): [B, num_labels]; an empty row's logits are
    defined as zeros.  ``pool``: mutation hook, rows [len, H] -> the pooled vector [H] (None = the model's pooling)."""

    pre = "ranking_model." if any(k.startswith("ranking_model.") for k in state) else ""
    W = lambda n: state[pre + n].to(torch.float64)  # noqa: E731
    if pool is None:
        pool = (lambda r: r.mean(dim=0)) if dims.classifier_pooling == "mean" else (lambda r: r[0])
    rank = torch.zeros(len(last_rows), dims.num_labels, dtype=torch.float64)
    for b, rows in enumerate(last_rows):
        if rows.shape[0] == 0:
            continue
        pooled = _layer_norm(_gelu(pool(rows.to(torch.float64)) @ W("head.dense.weight").T), W("head.norm.weight"), float(dims.norm_eps))
        rank[b] = pooled @ W("classifier.weight").T + W("classifier.bias")
    return rank


@dataclass
class ModelOutput:
    hidden: list[torch.Tensor]  # N + 1 entries, padded [B, Lmax, H] float64 (zeros beyond each row)
    prune: torch.Tensor  # [B, Lmax, 2]
    rank: torch.Tensor  # [B, num_labels]
    lengths: list[int]


@dataclass
class Backbone:
    """The encoder without its heads, packed: what :func:`heads` turns into a :class:`ModelOutput` under any pooling, label count
    and side of final_norm (none of which enters a layer)."""

    states: list[torch.Tensor]  # N entries [T, H]: the embedding LayerNorm output, then the outputs of layers 0 .. N - 2
    x: torch.Tensor  # [T, H]: the output of the last layer, before final_norm
    lengths: list[int]


def backbone(state: Mapping[str, torch.Tensor], dims, rows: Sequence[Sequence[int]], arith: "Arith | str" = "exact", *,
             path: str = "row", rope_is_global: "Sequence[bool] | None" = None, rope=None, visibility=None) -> Backbone:
    """The layers of :func:`forward` (its arguments)."""

    if isinstance(arith, str):
        arith = arith_for(arith, path)
    if rope_is_global is not None and len(rope_is_global) != dims.num_layers:
        raise ValueError("rope_is_global needs one flag per layer")
    pre = "ranking_model." if any(k.startswith("ranking_model.") for k in state) else ""
    W = lambda n: state[pre + n].to(torch.float64)  # noqa: E731
    H, nh = dims.hidden_size, dims.num_heads
    hd = H // nh
    eps = float(dims.norm_eps)
    lengths = [len(r) for r in rows]
    B, Lmax = len(rows), max(lengths, default=0)
    offs = [0]
    for n in lengths:
        offs.append(offs[-1] + n)
    ids = torch.tensor([int(t) for r in rows for t in r], dtype=torch.long)
    T = offs[-1]
    rope = {g: (rope or _rope)(hd, dims.global_rope_theta if g else dims.local_rope_theta, max(Lmax, 1)) for g in (True, False)}
    qscale = hd**-0.5 * LOG2E

    x = _layer_norm(W("model.embeddings.tok_embeddings.weight")[ids], W("model.embeddings.norm.weight"), eps)
    states = [x]
    for i in range(dims.num_layers):
        p = f"model.layers.{i}."
        glob = bool(dims.layer_is_global[i])
        h = x if i == 0 else _layer_norm(x, W(p + "attn_norm.weight"), eps)
        qkv = contract(h, W(p + "attn.Wqkv.weight").T, arith.scheme("wqkv", i)).view(T, 3, nh, hd)
        ctx = torch.zeros(T, H, dtype=torch.float64)
        hw = None if glob else dims.half_window + arith.window_delta
        tile = TILE_KEYS_GLOBAL if glob else TILE_KEYS_LOCAL
        for b in range(B):
            a, e = offs[b], offs[b + 1]
            if a == e:
                continue
            n = e - a
            c, s = (t[:n] for t in rope[glob if rope_is_global is None else bool(rope_is_global[i])])
            q, k, v = (qkv[a:e, j].transpose(0, 1) for j in range(3))  # [nh, n, hd]
            q = (q * c + _rot(q) * s) * qscale
            k = k * c + _rot(k) * s
            vis = visible(n, hw) if visibility is None else visibility(visible(n, hw), glob)
            ctx[a:e] = attention(q, k, v, vis, arith, i, tile).transpose(0, 1).reshape(n, H)
        x = x + contract(ctx, W(p + "attn.Wo.weight").T, arith.scheme("attn_out", i))
        h = _layer_norm(x, W(p + "mlp_norm.weight"), eps)
        g_in, gate = contract(h, W(p + "mlp.Wi.weight").T, arith.scheme("wi", i)).chunk(2, dim=-1)
        x = x + contract(_gelu(g_in) * gate, W(p + "mlp.Wo.weight").T, arith.scheme("mlp_out", i))
        if i != dims.num_layers - 1:
            states.append(x)
    return Backbone(states, x, lengths)


def heads(state: Mapping[str, torch.Tensor], dims, body: Backbone, *, prune_pre_final_norm: bool = False) -> ModelOutput:
    """final_norm, the pruning head and the ranking head of :func:`forward` on a backbone's last layer."""

    pre = "ranking_model." if any(k.startswith("ranking_model.") for k in state) else ""
    lengths, x = body.lengths, body.x
    B, Lmax = len(lengths), max(lengths, default=0)
    offs = [0]
    for n in lengths:
        offs.append(offs[-1] + n)
    last = _layer_norm(x, state[pre + "model.final_norm.weight"].to(torch.float64), float(dims.norm_eps))
    states = body.states + [x if prune_pre_final_norm else last]

    pw = state["pruning_head.classifier.weight"].to(torch.float64)
    pb = state["pruning_head.classifier.bias"].to(torch.float64)
    prune_packed = (x if prune_pre_final_norm else last) @ pw.T + pb
    rank = rank_logits(state, dims, [last[offs[b] : offs[b + 1]] for b in range(B)])

    def pad(t):
        out = torch.zeros(B, Lmax, t.shape[-1], dtype=torch.float64)
        for b in range(B):
            out[b, : lengths[b]] = t[offs[b] : offs[b + 1]]
        return out

    return ModelOutput([pad(t) for t in states], pad(prune_packed), rank, lengths)


def forward(state: Mapping[str, torch.Tensor], dims, rows: Sequence[Sequence[int]], arith: "Arith | str" = "exact", *,
            path: str = "row", prune_pre_final_norm: bool = False,
            rope_is_global: "Sequence[bool] | None" = None, rope=None, visibility=None) -> ModelOutput:
    """The forward on ragged ``rows`` of token ids (no padding enters any row's arithmetic).  Hidden entry 0 is the
    embedding LayerNorm output, entry i the output of layer i - 1, entry N the final_norm output -- or, under
    ``prune_pre_final_norm``, the un-normalised last layer (the pruning head's input either way, as op_hidden_request).
    ``rope_is_global``: mutation hook, per layer which RoPE table its q / k take (None = the layer's own type; the mask and
    the key tiles always follow the layer's own type); ``rope``: mutation hook, a replacement for :func:`_rope` ((head_dim, theta,
    n) -> cos, sin [n, head_dim] float64); ``visibility``: mutation hook, (the layer's [n, n] mask, the layer is global) -> the
    mask the attention applies (a query left without a visible key gets a zero attention output)."""

    body = backbone(state, dims, rows, arith, path=path, rope_is_global=rope_is_global, rope=rope, visibility=visibility)
    return heads(state, dims, body, prune_pre_final_norm=prune_pre_final_norm)


# -- the statistic the conformance tests bound ------------------------------------------------------------------------------
FLOOR = 1e-6  # x the entry's RMS: fp32 accumulation, which the model does not restate
RMS_FACTOR, MAX_FACTOR = 2.0, 4.0


def valid_mask(lengths: Sequence[int], width: int) -> torch.Tensor:
    return torch.arange(width)[None, :] < torch.tensor(list(lengths), dtype=torch.long)[:, None]


def entries(hidden: Sequence[torch.Tensor], prune: torch.Tensor, rank: torch.Tensor, lengths: Sequence[int]) -> dict[str, torch.Tensor]:
    """Named comparison entries, each over the valid tokens: hidden_0 .. hidden_N ([B, W, H] padded), prune ([B, W, 2]
    padded), rank ([B, labels]; empty rows left out)."""

    m = valid_mask(lengths, prune.shape[1])
    named = {f"hidden_{i}": h[m].double() for i, h in enumerate(hidden)}
    named["prune"] = prune[m].double()
    named["rank"] = rank[torch.tensor([n > 0 for n in lengths], dtype=torch.bool)].double()
    return named


def model_entries(out: ModelOutput) -> dict[str, torch.Tensor]:
    return entries(out.hidden, out.prune, out.rank, out.lengths)


def expand_entries(content: Mapping[str, torch.Tensor], lengths: Sequence[int], index: Sequence[int]) -> dict[str, torch.Tensor]:
    """The entries of the batch whose row b is a copy of content row ``index[b]``: ``content`` holds the entries of the
    content rows (of ``lengths``) run as one batch; no row's arithmetic depends on its neighbours, so the batch's entries
    are the contents' token blocks (and, for the non-empty rows, ranking logits) gathered in batch order."""

    lens = torch.tensor(list(lengths), dtype=torch.long)
    idx = torch.tensor(list(index), dtype=torch.long)
    start = torch.cumsum(lens, 0) - lens
    n = lens[idx]
    # token t of the batch: offset within its row + the start of that row's content
    row_of = torch.repeat_interleave(torch.arange(len(idx)), n)
    within = torch.arange(int(n.sum())) - (torch.cumsum(n, 0) - n)[row_of]
    tok = start[idx][row_of] + within
    rank_slot = torch.cumsum((lens > 0).long(), 0) - 1  # content row -> its line of the "rank" entry (empty rows are left out)
    rank_idx = rank_slot[idx[n > 0]]
    return {name: t[rank_idx] if name == "rank" else t[tok] for name, t in content.items()}


def rms(t: torch.Tensor) -> float:
    return float(t.double().pow(2).mean().sqrt()) if t.numel() else 0.0


def amax(t: torch.Tensor) -> float:
    return float(t.double().abs().max()) if t.numel() else 0.0


@dataclass(frozen=True)
class Bound:
    rms: float  # 2 x RMS of (model - exact), floored
    max: float  # 4 x max-abs of (model - exact), floored
    at_floor: bool  # the model's own error is below the floor: the entry checks fp32 noise, not a rounding scheme


def bounds(model: Mapping[str, torch.Tensor], exact: Mapping[str, torch.Tensor]) -> dict[str, Bound]:
    """Per entry: 2 x / 4 x the model's own error against exact, floored at FLOOR x the entry's RMS."""

    out = {}
    for name, ex in exact.items():
        floor = FLOOR * rms(ex)
        d = model[name] - ex
        b_rms, b_max = RMS_FACTOR * rms(d), MAX_FACTOR * amax(d)
        out[name] = Bound(max(b_rms, floor), max(b_max, floor), b_rms <= floor)
    return out


def _ratio(x: float, bound: float) -> float:
    return x / bound if bound > 0 else (0.0 if x == 0 else math.inf)


def ratios(got: Mapping[str, torch.Tensor], model: Mapping[str, torch.Tensor], bnd: Mapping[str, Bound]):
    """Per entry, in the order hidden_0 .. hidden_N, prune, rank: (ratio of the worse statistic to its bound, rms, max) of
    got - model.  A non-finite difference is an infinite ratio."""

    out = {}
    for name, b in bnd.items():
        d = got[name].double() - model[name]
        r, mx = rms(d), amax(d)
        if not (math.isfinite(r) and math.isfinite(mx)):
            r = mx = math.inf
        out[name] = (max(_ratio(r, b.rms), _ratio(mx, b.max)), r, mx)
    return out


def worst_ratio(got: Mapping[str, torch.Tensor], model: Mapping[str, torch.Tensor], bnd: Mapping[str, Bound]):
    """(worst ratio of a statistic to its bound, the first entry holding it, per-entry (rms, max) of got - model)."""

    per = ratios(got, model, bnd)
    where = max(per, key=lambda n: per[n][0])
    return per[where][0], where, {n: (r, mx) for n, (_, r, mx) in per.items()}


def first_over(per: Mapping[str, tuple], limit: float = 1.0) -> "str | None":
    """The shallowest entry whose ratio exceeds ``limit`` (hidden_0 .. hidden_N, then prune, rank), or None."""

    return next((n for n, v in per.items() if not v[0] <= limit), None)


# -- weight recipes ---------------------------------------------------------------------------------------------------------
PEAK_Q_SCALE = 4.0


def peaked_state_dict(dims, seed: int, q_scale: float = PEAK_Q_SCALE) -> dict[str, torch.Tensor]:
    """``synth_state_dict`` with the q rows of every Wqkv scaled by ``q_scale``: scores spread over tens of log2 units, so
    the lazy softmax reference moves late (its rescale branch runs) while q stays far inside fp16's range."""

    from open_provence_amd.synthetic import synth_state_dict

    state = synth_state_dict(dims, seed)
    H = dims.hidden_size
    for name, t in list(state.items()):
        if name.endswith("attn.Wqkv.weight"):
            t = t.clone()
            t[:H] *= q_scale
            state[name] = t
    return state


def bf16_valued(state: Mapping[str, torch.Tensor]) -> dict[str, torch.Tensor]:
    """Every tensor rounded to bf16 and held as fp32: what a bf16 checkpoint holds.  The kernel sets without a lo(W) term
    (:data:`BF16_WEIGHT_SETS`) exist for such checkpoints; on fp32-valued weights their rounding of W would dominate
    their error and hide every smaller departure of the kernels."""

    return {k: v.to(torch.bfloat16).to(torch.float32) for k, v in state.items()}


MLP_ISOLATING_SHIFT = 8


def mlp_isolating_state_dict(state: Mapping[str, torch.Tensor], shift: int = MLP_ISOLATING_SHIFT) -> dict[str, torch.Tensor]:
    """Every ``attn.Wo.weight`` x 2^-shift, put on fp16's grid and held as fp32 (apply after :func:`peaked_state_dict` /
    :func:`bf16_valued`).  A power of two changes no operand's rounding pattern; it shrinks what the attention side adds to
    the residual stream, and that side's error with it, 2^shift-fold, so the MLP's arithmetic dominates every entry's error:
    the correction terms of the MLP of kernel sets 8 - 11, invisible under their single-pass fp16 attention side on the plain
    weights, come out at 5 - 18 x the bound (tests/test_arith_model.py).

    Why fp16's grid: the library refuses every kernel set with an fp16 weight plane when the part of a tensor that fp16's
    subnormal grid loses carries more than 2^-36 of the tensor's energy (note_f16_fit in opk_common.hip.h).  A uniform
    (+-sqrt(3 / H)) tensor x 2^-8 loses about 2^-29 at H = 512.  Rounded onto the grid the loss is zero, and the model and
    the kernels read identical weights.  The recipe is for the sets whose weight hi plane is fp16 (3, 4, 8 - 11): the damped
    tensor is fp16-valued, not bf16-valued.  Single elements of it are fp16 subnormals and underflow in the weight's e4m3
    plane (stored x 2^6); the model converts them as torch does (gradual underflow, RNE); that branch is damped 2^shift-fold, and the kernels'
    attention-output entries agree with the model on every damped case (profiles/kernel_set_conformance.txt)."""

    out = dict(state)
    for name, t in state.items():
        if name.endswith("attn.Wo.weight"):
            out[name] = (t.to(torch.float32) * 2.0**-shift).to(torch.float16).to(torch.float32)
    return out
