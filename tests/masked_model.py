"""The dense forward under an arbitrary attention mask (``op_forward_masked``), restated in float64 -- and the inputs its
tests share.

What the kernels are held to is ``oracle.modernbert_oracle.oracle_forward``; this file says the same thing the way the
kernels do it, row by row and query by query, so that each rule can be broken on purpose (``mutation=``) and the tests'
inputs shown to notice:

* every position of a padded row is a query at position = its column, masked ones included;
* the keys of a query are the positions with ``mask == 1``, in a sliding-window layer those with ``|q - k| <= window // 2``;
* a query without a key takes the plain mean of ``v`` over ALL ``L`` positions of its row (what a softmax over scores that
  are all ``finfo.min`` gives: uniform weights over the padded row);
* cls pooling reads column 0 whatever its mask says; mean pooling sums the final-norm output over ``mask == 1`` and divides
  by their count;
* outputs (the project's convention): pruning logits are 0 where ``mask == 0``; a row without a one gives zeros in both.

Mutations (each a mistake a kernel could make):

  no_fallback            a query without a key gets a zero attention output
  fallback_valid_keys    ... the mean of v over the row's valid positions
  fallback_window        ... the mean of v over its index window
  local_mask_ignored     sliding-window layers see masked keys
  global_mask_ignored    full-attention layers see masked keys
  masked_queries_skipped masked positions get a zero attention output
  cls_first_valid        cls pooling reads the first valid position instead of column 0
  mean_over_all          mean pooling runs over all L positions
"""

from __future__ import annotations

import math

import numpy as np
import torch

MUTATIONS = ("no_fallback", "fallback_valid_keys", "fallback_window", "local_mask_ignored", "global_mask_ignored",
             "masked_queries_skipped", "cls_first_valid", "mean_over_all")

# -- models and inputs shared by tests/test_masked_model.py and tests/test_gpu_masked_forward.py ---------------------------------
RAGGED = [1, 2, 8, 9, 15, 16, 17, 63, 64, 65, 127, 128, 129, 130, 200]
# (hidden, heads, pattern, window, pooling, labels, prune_pre_final_norm, weights): the table of tests/test_gpu_fp32_set.py
SMALL = [
    (128, 2, "GLL", 16, "cls", 1, False, "refinit"),
    (128, 2, "LGL", 128, "mean", 2, True, "synth"),
    (128, 2, "GLL", 128, "mean", 2, False, "refinit"),
    (128, 2, "LGL", 16, "cls", 1, True, "synth"),
    (384, 6, "GLL", 128, "cls", 1, True, "synth"),
    (384, 6, "LGL", 16, "mean", 2, False, "refinit"),
    (384, 6, "GLL", 16, "mean", 2, True, "refinit"),
    (384, 6, "LGL", 128, "cls", 1, False, "synth"),
]
WIDTHS = (200, 77, 1)


def case_id(c) -> str:
    return f"h{c[0]}-{c[2]}-w{c[3]}-{c[4]}{c[5]}-{'pre' if c[6] else 'post'}-{c[7]}"


def small_dims(hidden, heads, pattern, window, pooling, labels, max_positions=2048):
    from open_provence_amd.config import EncoderDims

    cfg = dict(model_type="modernbert", vocab_size=512, hidden_size=hidden, intermediate_size=192, num_hidden_layers=3,
               num_attention_heads=heads, local_attention=window, global_attn_every_n_layers=3, global_rope_theta=160000.0,
               local_rope_theta=10000.0, max_position_embeddings=max_positions, pad_token_id=0, cls_token_id=1, sep_token_id=2,
               layer_types=["full_attention" if t == "G" else "sliding_attention" for t in pattern], classifier_pooling=pooling)
    return EncoderDims.from_base_model_config(cfg, num_labels=labels)


def masks(width: int, seed: int = 3) -> "tuple[np.ndarray, list[str]]":
    """The mask cases of one batch of ``width`` columns -> (mask[B, width] int64, a name per row).  At width 200: the RAGGED
    lengths as LEFT padding (pads from 0 to 199: the empty-window fallback at both window sizes), random holes at about 20 %,
    a hole of 40 columns in mid-row (longer than window 16), a hole over columns 64 .. 127 exactly (a whole key tile), a row
    with its only one in the last column, a full row, an all-zero row, and prefix rows."""

    rng = np.random.default_rng(seed)
    rows, names = [], []

    def add(name, row):
        rows.append(np.asarray(row, dtype=np.int64))
        names.append(name)

    for n in sorted({min(n, width) for n in RAGGED}):
        row = np.zeros(width, np.int64)
        row[width - n:] = 1
        add(f"left-padded to {n}", row)
    for k in range(2):
        add(f"random holes {k}", (rng.random(width) >= 0.2).astype(np.int64))
    row = np.ones(width, np.int64)
    row[width // 2 - min(20, width // 4): width // 2 + min(20, width // 4)] = 0
    add("hole of 40 in mid-row", row)
    row = np.ones(width, np.int64)
    row[64:128] = 0
    add("hole over columns 64..127", row)
    row = np.zeros(width, np.int64)
    row[-1] = 1
    add("only the last column", row)
    add("full", np.ones(width, np.int64))
    add("all zero", np.zeros(width, np.int64))
    for n in (1, width // 3 + 1, max(width - 1, 1)):
        row = np.zeros(width, np.int64)
        row[: min(n, width)] = 1
        add(f"prefix {min(n, width)}", row)
    return np.stack(rows), names


def batch(width: int, seed: int = 7, vocab: int = 512) -> "tuple[torch.Tensor, torch.Tensor, list[str]]":
    """-> (input_ids[B, width] int64 -- a token at EVERY position, column 0 included: masked positions are embedded too --,
    attention_mask[B, width] int64, row names)."""

    mask, names = masks(width)
    rng = np.random.default_rng(seed)
    ids = rng.integers(3, vocab, size=mask.shape)
    return torch.from_numpy(ids), torch.from_numpy(mask), names


def prefix_batch(width: int = 200) -> "tuple[torch.Tensor, torch.Tensor]":
    """The RAGGED lengths (clipped to ``width``) right-padded: what both the masked and the packed forward take."""

    lengths = [min(n, width) for n in RAGGED]
    rng = np.random.default_rng(7)
    ids = torch.from_numpy(rng.integers(3, 512, size=(len(lengths), width)))
    mask = (torch.arange(width)[None, :] < torch.tensor(lengths)[:, None]).long()
    return ids, mask


# -- the restatement -----------------------------------------------------------------------------------------------------------------
def _ln(x, w, eps):
    mean = x.mean(-1, keepdim=True)
    return (x - mean) / torch.sqrt(((x - mean) ** 2).mean(-1, keepdim=True) + eps) * w


def _gelu(x):
    return 0.5 * x * (1.0 + torch.erf(x / math.sqrt(2.0)))


def _rope(x, pos, theta):
    """x[L, heads, hd] rotated at positions pos[L] (rotate_half pairs d with d + hd / 2)."""

    hd = x.shape[-1]
    inv = 1.0 / (theta ** (torch.arange(0, hd, 2, dtype=torch.float32) / hd))  # (the fp32 table the reference builds)
    ang = pos.to(torch.float32)[:, None] * inv[None, :]
    cos, sin = ang.cos().double()[:, None, :], ang.sin().double()[:, None, :]
    lo, hi = x[..., : hd // 2], x[..., hd // 2:]
    return torch.cat((lo * cos - hi * sin, hi * cos + lo * sin), dim=-1)


def masked_forward(state, dims, input_ids, attention_mask, *, prune_pre_final_norm=False, mutation=None):
    """-> (pruning_logits[B, L, 2], ranking_logits[B, nl]) float64, in the reference's semantics at EVERY position (no zeroing:
    :func:`project_outputs` applies the project's convention)."""

    assert mutation is None or mutation in MUTATIONS, mutation
    pre = "ranking_model." if any(k.startswith("ranking_model.") for k in state) else ""
    W = lambda name: state[pre + name].double()  # noqa: E731
    B, L = input_ids.shape
    H, nh = dims.hidden_size, dims.num_heads
    hd, eps, half = H // nh, float(dims.norm_eps), int(dims.local_attention) // 2
    pos = torch.arange(L)
    prune_rows, pooled_rows = [], []
    for b in range(B):
        ok = attention_mask[b].bool()
        x = _ln(W("model.embeddings.tok_embeddings.weight")[input_ids[b]], W("model.embeddings.norm.weight"), eps)
        for i in range(dims.num_layers):
            p = f"model.layers.{i}."
            is_global = bool(dims.layer_is_global[i])
            h = x if i == 0 else _ln(x, W(p + "attn_norm.weight"), eps)
            qkv = (h @ W(p + "attn.Wqkv.weight").T).view(L, 3, nh, hd)
            theta = dims.global_rope_theta if is_global else dims.local_rope_theta
            q, k, v = _rope(qkv[:, 0], pos, theta), _rope(qkv[:, 1], pos, theta), qkv[:, 2]
            keys = ok.clone()
            if mutation == ("global_mask_ignored" if is_global else "local_mask_ignored"):
                keys = torch.ones_like(ok)
            ctx = torch.zeros(L, nh, hd, dtype=torch.float64)
            for t in range(L):
                if mutation == "masked_queries_skipped" and not bool(ok[t]):
                    continue
                window = torch.ones(L, dtype=torch.bool) if is_global else (pos - t).abs() <= half
                mine = keys & window
                if not bool(mine.any()):  # no key: uniform over the padded row
                    if mutation == "no_fallback":
                        continue
                    pick = torch.ones(L, dtype=torch.bool)
                    if mutation == "fallback_valid_keys" and bool(ok.any()):
                        pick = ok
                    if mutation == "fallback_window":
                        pick = window
                    ctx[t] = v[pick].mean(0)
                    continue
                s = torch.einsum("hd,khd->hk", q[t], k[mine]) * hd**-0.5
                ctx[t] = torch.einsum("hk,khd->hd", torch.softmax(s, dim=-1), v[mine])
            x = x + ctx.reshape(L, H) @ W(p + "attn.Wo.weight").T
            a, g = (_ln(x, W(p + "mlp_norm.weight"), eps) @ W(p + "mlp.Wi.weight").T).chunk(2, dim=-1)
            x = x + (_gelu(a) * g) @ W(p + "mlp.Wo.weight").T
        last = _ln(x, W("model.final_norm.weight"), eps)
        if dims.classifier_pooling == "mean":
            sel = torch.ones_like(ok) if mutation == "mean_over_all" else ok
            pooled = last[sel].sum(0) / sel.sum()  # (0 / 0 = NaN for a row without a one, as in the reference)
        else:
            first = int(torch.nonzero(ok)[0]) if mutation == "cls_first_valid" and bool(ok.any()) else 0
            pooled = last[first]
        pooled_rows.append(pooled)
        prune_rows.append((x if prune_pre_final_norm else last) @ state["pruning_head.classifier.weight"].double().T
                          + state["pruning_head.classifier.bias"].double())
    pooled = _ln(_gelu(torch.stack(pooled_rows) @ W("head.dense.weight").T), W("head.norm.weight"), eps)
    return torch.stack(prune_rows), pooled @ W("classifier.weight").T + W("classifier.bias")


def project_outputs(prune, rank, attention_mask):
    """The project's convention on top of the reference's values: pruning logits 0 where the mask is 0, a row without a one
    zeros in both outputs."""

    on = attention_mask.bool()
    return torch.where(on[..., None], prune, torch.zeros_like(prune)), torch.where(on.any(1)[:, None], rank, torch.zeros_like(rank))


# -- compared quantities and the bound -----------------------------------------------------------------------------------------------
def compared(prune, rank, attention_mask) -> "dict[str, torch.Tensor]":
    """What the tests compare, as tests/test_gpu_fp32_set.py names it: ``logits`` = the pruning logits at ``mask == 1`` and the
    ranking logits of every row with a one; ``keep_prob`` = softmax(pruning logits)[1] at ``mask == 1``."""

    on = attention_mask.bool()
    alive = on.any(1)
    return {"logits": torch.cat([prune[on].double().flatten(), rank[alive].double().flatten()]),
            "keep_prob": torch.softmax(prune[on].double(), dim=-1)[:, 1]}


class Reference:
    """The fp64 oracle's compared quantities of one batch and, per quantity, the fp32 oracle's distance to them; the bound of
    tests/test_gpu_fp32_set.py: ``max(4 x e_ref, 16 ulp of the quantity's largest magnitude)``."""

    def __init__(self, state, dims, input_ids, attention_mask, pre_norm):
        from oracle.modernbert_oracle import oracle_forward

        outs = {}
        for dtype in (torch.float64, torch.float32):
            out = oracle_forward(state, dims, input_ids, attention_mask, dtype=dtype, prune_pre_final_norm=pre_norm)
            outs[dtype] = compared(out.pruning_logits, out.ranking_logits, attention_mask)
        self.entries = outs[torch.float64]
        self.e_ref = {k: float((outs[torch.float32][k] - v).abs().max()) if v.numel() else 0.0 for k, v in self.entries.items()}

    def bound(self, name) -> float:
        top = float(self.entries[name].abs().max()) if self.entries[name].numel() else 0.0
        return max(4.0 * self.e_ref[name], 16.0 * float(np.spacing(np.float32(top))))
