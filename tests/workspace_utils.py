"""Controlled workspaces for the forward: a workspace of exactly ``op_workspace_bytes`` between two canaried guards, filled
with a pattern per region before a forward (tests/test_gpu_workspace_independence.py).

The contract under test (include/open_provence_hip.h, op_forward_packed): the workspace may hold anything on entry, the
outputs depend on ids, cu_seqlens and the weights only, and nothing outside the workspace and the output buffers is written.

The purpose of a fill is to detect VALUE dependence: an output that changes with what a region held before the forward.  A
fill must never hand a kernel an out-of-range index -- a kernel that reads a stale row map would then address memory
outside its buffers, which is a GPU fault and not a test result.  That is why the fills go by the layout the
library reports (``HipEncoder.workspace_layout`` = op_debug_workspace_layout, computed by the carving code itself) and not by
a byte pattern over the whole workspace:

  zeros   every region zero: the baseline of every comparison
  nan     float and flag regions: byte 0xFF (NaN as fp32, fp16, bf16 and e4m3fn; a raised flag)
  huge    float regions: byte 0x7B (1.3058e36 fp32, 61280 fp16, 1.3033e36 bf16, 352 e4m3fn: finite, the 16-bit values near the
          top of their ranges); the flag region: 1

and in both poisoned fills every index region holds the int32 value 1: a WRONG entry of each map (row -> sequence, position,
token, sequence -> row offset, query-block offset) that is still in range, because every batch of the module has at least
two sequences (an empty second row where need be) and at least two tokens.  The one batch with a single token gets 0 there
(``wrong_index``).  tests/test_workspace_fills.py pins what the byte patterns mean, on the CPU."""

from __future__ import annotations

import ctypes
from dataclasses import dataclass

import numpy as np
import torch

FILLS = ("zeros", "nan", "huge")
POISONS = ("nan", "huge")
NAN_BYTE, HUGE_BYTE = 0xFF, 0x7B
GUARD_BYTES = 65536
# the guards' content: differs from both poison bytes, so a kernel that copies poisoned data past a buffer's end is seen
CANARY = 0x5AA5C3A5
# ... and around keep_prob, a NaN (with a payload of its own)
NAN_CANARY = 0x7FC0A5C3
OUTPUT_NAMES = ("prune", "rank", "hidden", "keep_prob")


@dataclass
class Canaried:
    """``view``: ``nbytes`` bytes in the middle of ``backing`` (uint8), ``guard`` bytes of ``canary`` (an int32 pattern) on
    either side."""

    backing: torch.Tensor
    view: torch.Tensor
    guard: int
    canary: int

    def assert_intact(self, what: str) -> None:
        n = self.view.numel()
        for side, part in (("below", self.backing[: self.guard]), ("above", self.backing[self.guard + n:])):
            words = part.view(torch.int32)
            bad = torch.nonzero(words != self.canary)
            if bad.numel():
                first = int(bad[0])
                at = first * 4 if side == "above" else first * 4 - self.guard
                raise AssertionError(f"{what}: the guard {side} the buffer was written: {int(bad.numel())} words differ from the canary, "
                                     f"the first at byte {at:+d} from the buffer's {'end' if side == 'above' else 'start'} "
                                     f"(holds {int(words[first]) & 0xFFFFFFFF:#010x})")


def canaried(nbytes: int, device, *, guard: int = GUARD_BYTES, canary: int = CANARY) -> Canaried:
    assert nbytes % 4 == 0 and guard % 256 == 0, (nbytes, guard)
    backing = torch.empty(guard + nbytes + guard, dtype=torch.uint8, device=device)
    backing.view(torch.int32).fill_(canary)
    view = backing[guard: guard + nbytes]
    assert view.data_ptr() % 256 == 0 or backing.device.type == "cpu"  # (device allocations are 256-aligned, the guard keeps it)
    return Canaried(backing, view, guard, canary)


@dataclass
class ControlledWorkspace:
    mem: Canaried
    need: int  # op_workspace_bytes of the geometry it was made for
    layout: list  # HipEncoder.workspace_layout of that geometry
    wrong_index: int
    installed: "torch.Tensor | None" = None  # what a pipeline holds: the view + its 256 bytes of alignment slack

    @property
    def view(self) -> torch.Tensor:
        return self.mem.view


def _geometry(rows):
    lengths = [len(r) for r in rows]
    return len(rows), sum(lengths), max(lengths)


def controlled_workspace(enc, n_seqs: int, total: int, max_len: int, guard: int = GUARD_BYTES, *, part: "int | None" = None
                         ) -> ControlledWorkspace:
    """A workspace of exactly ``op_workspace_bytes`` for this geometry, 256-aligned, between two ``guard``-byte canaries,
    installed as the encoder's own (``part``: as the workspace of that pipeline of ``forward_packed_on``, which asks for 256
    bytes of alignment slack at the end: they are canary too and checked with the guard above)."""

    need = int(enc.lib.op_workspace_bytes(enc._handle, n_seqs, total, max_len))
    assert need > 0 and need % 256 == 0, need
    layout = enc.workspace_layout(n_seqs, total, max_len)
    mem = canaried(need, enc.device, guard=guard)
    cw = ControlledWorkspace(mem, need, layout, 1 if min(n_seqs, total) >= 2 else 0)
    if part is None:
        enc._workspace = mem.view
    else:
        slack = mem.backing[guard: guard + need + 256]  # (the forward is handed need + 256 bytes from an aligned base: it uses `need`)
        enc._split_streams()["ws"][part] = slack
        cw.installed = slack
    enc._controlled = cw
    return cw


def fill_workspace(cw: ControlledWorkspace, fill: str, only: "str | None" = None) -> None:
    """``only``: poison that region alone, zeros everywhere else (``leaking_regions``)."""

    assert fill in FILLS, fill
    cw.view.zero_()
    if fill == "zeros":
        return
    for region in cw.layout:
        if only is not None and region["name"] != only:
            continue
        size = (region["bytes"] + 255) // 256 * 256
        part = cw.view[region["offset"]: region["offset"] + size]
        if region["kind"] == "index":
            part.view(torch.int32).fill_(cw.wrong_index)
        elif region["kind"] == "float":
            part.fill_(NAN_BYTE if fill == "nan" else HUGE_BYTE)
        elif fill == "nan":
            part.fill_(NAN_BYTE)
        else:
            part.view(torch.int32).fill_(1)


def _check_workspace(enc, cw: ControlledWorkspace, what: str, part: "int | None" = None) -> None:
    held = enc._workspace if part is None else enc._split_streams()["ws"][part]
    mine = cw.view if part is None else cw.installed
    assert held is mine, f"{what}: the engine replaced the workspace it was given ({cw.need} bytes) by one of {held.numel()} bytes"
    cw.mem.assert_intact(f"{what}: workspace")


def _device_batch(enc, rows):
    from open_provence_amd.packing import pack_rows

    ids_np, cu_np, max_len = pack_rows(rows)
    return torch.from_numpy(ids_np).to(enc.device), torch.from_numpy(cu_np).to(enc.device), cu_np, max_len


def _prepare(enc, rows, fill, only=None, part=None) -> ControlledWorkspace:
    """``fill`` None: the workspace the encoder already runs on, as the last forward left it."""

    if fill is None:
        cw = enc._controlled
        assert cw.need >= int(enc.lib.op_workspace_bytes(enc._handle, *_geometry(rows)))
    else:
        cw = controlled_workspace(enc, *_geometry(rows), part=part)
        fill_workspace(cw, fill, only)
    return cw


def run(enc, rows, fill: "str | None", keep: bool = True, *, only: "str | None" = None, part: "int | None" = None):
    """One ``forward_packed`` (``part``: ``forward_packed_on`` that pipeline, without hidden states) of ``rows`` on a controlled
    workspace filled with ``fill`` (None: left as it is), with a packed ``HiddenRequest()`` and ``keep_prob`` a view inside a
    NaN-canaried buffer -> (prune, rank, hidden, keep_prob) on the device; guards and canaries are asserted."""

    from open_provence_amd.engine import HiddenRequest

    cw = _prepare(enc, rows, fill, only, part)
    ids, cu, cu_np, max_len = _device_batch(enc, rows)
    kp = canaried(int(ids.numel()) * 4, enc.device, canary=NAN_CANARY) if keep else None
    keep_prob = kp.view.view(torch.float32) if keep else None
    if part is None:
        prune, rank, hidden = enc.forward_packed(ids, cu, cu_np, max_len, keep_prob=keep_prob, hidden=HiddenRequest())
        torch.cuda.synchronize()
    else:
        torch.cuda.synchronize()  # (the fill ran on the caller's stream; nothing orders the pipeline's behind it)
        prune, rank = enc.forward_packed_on(part, ids, cu, cu_np, max_len, keep_prob=keep_prob)
        enc.pipeline_stream(part).synchronize()
        hidden = None
    what = f"fill {fill!r}, lengths {[len(r) for r in rows]}"
    _check_workspace(enc, cw, what, part)
    if keep:
        kp.assert_intact(f"{what}: keep_prob")
    return prune, rank, hidden, keep_prob


def run_direct(enc, rows, fill: "str | None", *, padded: bool, dtype: torch.dtype, only: "str | None" = None):
    """The same forward through ``op_forward_packed_hidden`` itself: prune, rank, keep_prob and the hidden output (every entry;
    packed, or padded to the longest row with zeros at the positions the call does not write) are ALL views between canaries,
    asserted afterwards -> (prune, rank, hidden, keep_prob)."""

    from open_provence_amd import _lib

    cw = _prepare(enc, rows, fill, only)
    ids, cu, cu_np, max_len = _device_batch(enc, rows)
    n_seqs, total = len(rows), int(ids.numel())
    H, n_entries, nl = enc.dims.hidden_size, enc.dims.num_layers + 1, enc.dims.num_labels
    pad = max(max_len, 1) if padded else 0
    item = {torch.float32: 4, torch.bfloat16: 2}[dtype]
    hidden_shape = (n_entries, n_seqs, pad, H) if padded else (n_entries, total, H)
    bufs = {
        "prune": canaried(total * 2 * 4, enc.device),
        "rank": canaried(n_seqs * nl * 4, enc.device),
        "keep_prob": canaried(total * 4, enc.device, canary=NAN_CANARY),
        "hidden": canaried(int(np.prod(hidden_shape)) * item, enc.device),
    }
    bufs["hidden"].view.zero_()
    req = _lib.OpHiddenRequest()
    req.struct_bytes = ctypes.sizeof(_lib.OpHiddenRequest)
    req.dtype = _lib.OP_HIDDEN_F32 if dtype == torch.float32 else _lib.OP_HIDDEN_BF16
    req.pad_width = pad
    req.select = None
    req.out_dev = ctypes.c_void_p(bufs["hidden"].view.data_ptr())
    vp = ctypes.c_void_p
    with torch.cuda.device(enc.device):
        code = enc.lib.op_forward_packed_hidden(
            enc._handle, vp(ids.data_ptr()), vp(cu.data_ptr()), cu_np.ctypes.data_as(vp), n_seqs, total, max_len,
            vp(bufs["prune"].view.data_ptr()), vp(bufs["rank"].view.data_ptr()), vp(bufs["keep_prob"].view.data_ptr()),
            vp(cw.view.data_ptr()), ctypes.c_size_t(cw.need), vp(torch.cuda.current_stream(enc.device).cuda_stream), ctypes.byref(req))
    _lib.check(enc.lib, enc._handle, code, "op_forward_packed_hidden")
    torch.cuda.synchronize()
    what = f"direct call, fill {fill!r}, {'padded' if padded else 'packed'} {dtype}, lengths {[len(r) for r in rows]}"
    cw.mem.assert_intact(f"{what}: workspace")
    for name, buf in bufs.items():
        buf.assert_intact(f"{what}: {name}")
    return (bufs["prune"].view.view(torch.float32).view(total, 2), bufs["rank"].view.view(torch.float32).view(n_seqs, nl),
            bufs["hidden"].view.view(dtype).view(hidden_shape), bufs["keep_prob"].view.view(torch.float32))


def _bits(t: torch.Tensor) -> torch.Tensor:
    return t.contiguous().view(torch.int32 if t.element_size() == 4 else torch.int16)


def first_difference(ref, got, rows) -> "str | None":
    """The first entry whose bits differ between two results of ``run`` / ``run_direct`` on ``rows``, the hidden states (the
    shallowest one) before the logits: which output (which hidden state), token and row."""

    cu = np.concatenate(([0], np.cumsum([len(r) for r in rows])))

    def token(t: int) -> str:
        s = int(np.searchsorted(cu, t, side="right")) - 1
        return f"token {t} (row {s}, position {t - int(cu[s])})"

    for name, a, b in sorted(zip(OUTPUT_NAMES, ref, got), key=lambda e: e[0] != "hidden"):
        if a is None or b is None:
            continue
        diff = torch.nonzero(_bits(a) != _bits(b))
        if not diff.numel():
            continue
        at = [int(v) for v in diff[0]]
        value = f"{a[tuple(at)].item()!r} on zeros, {b[tuple(at)].item()!r} here; {int(diff.shape[0])} entries differ"
        if name == "rank":
            return f"rank[row {at[0]}, label {at[1]}]: {value}"
        if name == "hidden" and a.ndim == 4:
            return f"hidden_{at[0]}[row {at[1]}, position {at[2]}, channel {at[3]}]: {value}"
        if name == "hidden":
            return f"hidden_{at[0]}[{token(at[1])}, channel {at[2]}]: {value}"
        return f"{name}[{token(at[0])}{', ' + str(at[1]) if len(at) > 1 else ''}]: {value}"
    return None


def same(ref, got) -> bool:
    """``torch.equal`` of every output (a NaN in either makes them differ)."""

    return all(torch.equal(a, b) for a, b in zip(ref, got) if a is not None)


def leaking_regions(enc, rows, pattern: str, runner=run) -> "list[str]":
    """After a failure: one forward of ``rows`` per region of the workspace, that region alone poisoned with ``pattern`` -> the
    regions whose content reaches an output, each with the first entry that differs from the run on zeros."""

    ref = runner(enc, rows, "zeros")
    found = []
    for region in enc._controlled.layout:
        got = runner(enc, rows, pattern, only=region["name"])
        where = first_difference(ref, got, rows)
        if where is not None:
            found.append(f"{region['name']} -> {where}")
    return found
