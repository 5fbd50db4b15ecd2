"""The forward under an arbitrary attention mask without a GPU: the float64 restatement (tests/masked_model.py) held against the
CPU oracle in float64 on the GPU test's own inputs; the mistakes a kernel could make shown to move a compared quantity of
those inputs by more than 10 x its bound; and ``op_forward_masked`` -- declared, bound, exported, additive to ABI 10 --
refusing every malformed call that needs no device, with the constructor argument that opts a model in."""

import ctypes
import functools
import inspect
import re
from pathlib import Path

import pytest
import torch

import masked_model as mm
from open_provence_amd import _lib

HEADER = Path(__file__).resolve().parents[1] / "include" / "open_provence_hip.h"


@functools.lru_cache(maxsize=None)
def _state(case):
    from open_provence_amd.synthetic import refinit_state_dict, synth_state_dict

    return (refinit_state_dict if case[7] == "refinit" else synth_state_dict)(mm.small_dims(*case[:6]), 5)


@functools.lru_cache(maxsize=None)
def _reference(case, width):
    ids, mask, _ = mm.batch(width)
    return mm.Reference(_state(case), mm.small_dims(*case[:6]), ids, mask, case[6])


@functools.lru_cache(maxsize=None)
def _restated(case, width, mutation=None):
    ids, mask, _ = mm.batch(width)
    prune, rank = mm.masked_forward(_state(case), mm.small_dims(*case[:6]), ids, mask, prune_pre_final_norm=case[6], mutation=mutation)
    return mm.compared(prune, rank, mask)


# every model at the width that holds every mask case; the two small widths on one cls and one mean model
PAIRS = [(case, 200) for case in mm.SMALL] + [(mm.SMALL[0], 77), (mm.SMALL[1], 77), (mm.SMALL[0], 1), (mm.SMALL[1], 1)]


@pytest.mark.parametrize("case,width", PAIRS, ids=lambda v: mm.case_id(v) if isinstance(v, tuple) else f"L{v}")
def test_restatement_is_the_oracle_in_float64(case, width):
    ref, got = _reference(case, width), _restated(case, width)
    for name, want in ref.entries.items():
        assert got[name].shape == want.shape and bool(torch.isfinite(want).all()), name
        top = max(float(want.abs().max()), 1e-300) if want.numel() else 1.0
        err = float((got[name] - want).abs().max()) if want.numel() else 0.0
        assert err <= 1e-12 * top, f"{name}: {err:.3e} from the oracle (largest magnitude {top:.3e})"


# where each mistake must show: the fallback and the masked queries reach an output through the cls-pooled ranking logit only
MUTATION_CASES = {
    "no_fallback": [mm.SMALL[0], mm.SMALL[7]],
    "fallback_valid_keys": [mm.SMALL[0], mm.SMALL[7]],
    "fallback_window": [mm.SMALL[0], mm.SMALL[7]],
    "local_mask_ignored": [mm.SMALL[0], mm.SMALL[1]],
    "global_mask_ignored": [mm.SMALL[0], mm.SMALL[1]],
    "masked_queries_skipped": [mm.SMALL[0], mm.SMALL[7]],
    "cls_first_valid": [mm.SMALL[0], mm.SMALL[7]],
    "mean_over_all": [mm.SMALL[1], mm.SMALL[5]],
}


@pytest.mark.parametrize("mutation", mm.MUTATIONS)
def test_the_inputs_notice_each_mistake(mutation):
    """Each mistake moves a compared quantity of the GPU test's width-200 batch by more than 10 x that quantity's bound, on every
    model listed for it (window 16 and window 128 for the fallback)."""

    assert set(MUTATION_CASES) == set(mm.MUTATIONS)
    for case in MUTATION_CASES[mutation]:
        ref, clean, broken = _reference(case, 200), _restated(case, 200), _restated(case, 200, mutation)
        moved = {name: float((torch.nan_to_num(broken[name], nan=1e30) - clean[name]).abs().max()) / ref.bound(name) for name in ref.entries}
        print(f"[masked-model] {mutation:24s} {mm.case_id(case):36s} " + "  ".join(f"{k} {v:.3g} x bound" for k, v in moved.items()))
        assert max(moved.values()) > 10.0, f"{mutation} on {mm.case_id(case)} moves nothing by more than 10 x its bound: {moved}"


def test_the_mask_cases_cover_what_they_name():
    mask, names = mm.masks(200)
    by = dict(zip(names, mask))
    pads = sorted(int((row == 0).sum()) for name, row in by.items() if name.startswith("left-padded"))
    assert pads[0] == 0 and pads[-1] == 199 and any(8 < p for p in pads) and any(64 < p for p in pads)  # both half windows
    assert all(bool((row[200 - int(row.sum()):] == 1).all()) for name, row in by.items() if name.startswith("left-padded"))
    assert by["hole over columns 64..127"][64:128].sum() == 0 and by["hole over columns 64..127"].sum() == 136
    assert by["hole of 40 in mid-row"].sum() == 160 and by["only the last column"].tolist() == [0] * 199 + [1]
    assert by["all zero"].sum() == 0 and by["full"].sum() == 200
    holes = [row for name, row in by.items() if name.startswith("random holes")]
    assert all(0.1 < 1 - row.mean() < 0.3 for row in holes)
    assert sum(name.startswith("prefix") for name in names) == 3
    for width in (77, 1):
        m, n = mm.masks(width)
        assert m.shape == (len(n), width)


def test_projection_zeroes_masked_positions_and_empty_rows():
    prune, rank = torch.ones(2, 3, 2, dtype=torch.float64), torch.ones(2, 1, dtype=torch.float64)
    mask = torch.tensor([[0, 1, 0], [0, 0, 0]])
    p, r = mm.project_outputs(prune, rank, mask)
    assert p[0, 1].tolist() == [1, 1] and p[0, 0].tolist() == [0, 0] and float(p[1].abs().sum()) == 0 and r.flatten().tolist() == [1, 0]


# -- the C call: declared, bound, exported, refusing without a device -------------------------------------------------------------------
def test_the_calls_are_declared_bound_and_additive():
    text = HEADER.read_text()
    assert re.search(r"\bsize_t\s+op_masked_workspace_bytes\s*\(", text) and re.search(r"\bint\s+op_forward_masked\s*\(", text)
    assert re.search(r"#define\s+OP_ABI_VERSION\s+10\b", text), "the calls are additive: the header's version stays 10"
    assert _lib.OP_ABI_VERSION == 10
    assert "op_forward_masked" in _lib.EXPORTED_SYMBOLS and "op_masked_workspace_bytes" in _lib.EXPORTED_SYMBOLS
    # the report as the header lays it out: uint32, 3 x int32, int64
    body = re.search(r"typedef struct op_masked_report \{(.*?)\} op_masked_report;", text, re.S).group(1)
    fields = re.findall(r"\b(uint32_t|int32_t|int64_t)\s+([^;]+);", body)
    names = [n.strip() for _, group in fields for n in group.split(",")]
    assert names == [name for name, _ in _lib.OpMaskedReport._fields_]
    assert ctypes.sizeof(_lib.OpMaskedReport) == 24


def test_library_exports_the_calls(hip_library):
    assert hip_library.op_abi_version() == 10
    assert hasattr(hip_library, "op_forward_masked") and hasattr(hip_library, "op_masked_workspace_bytes")
    assert hip_library.op_masked_workspace_bytes(None, 4, 16) == 0  # (no handle: no size)


def _call(lib, report, *, ids=0x1000, mask=0x1000, n_rows=2, width=8, ws=0x1000, ws_bytes=1 << 20, prune=0x1000, rank=0x1000):
    vp = ctypes.c_void_p
    return lib.op_forward_masked(None, vp(ids), vp(mask), n_rows, width, vp(ws), ctypes.c_size_t(ws_bytes), vp(prune), vp(rank),
                                 ctypes.byref(report) if report is not None else None, None)


def test_malformed_calls_are_refused_before_the_handle_is_looked_at(hip_library):
    """Every pointer below is a number that is never dereferenced: each call is refused on its arguments alone."""

    lib = hip_library
    good = _lib.OpMaskedReport()
    good.struct_bytes = ctypes.sizeof(_lib.OpMaskedReport)
    assert _call(lib, None) == _lib.OP_ERR_INVALID and "report is NULL" in _lib.last_error(lib, None)
    bad = _lib.OpMaskedReport()
    bad.struct_bytes = 12
    assert _call(lib, bad) == _lib.OP_ERR_INVALID and "struct_bytes" in _lib.last_error(lib, None)
    for kwargs, text in (
        (dict(n_rows=-1), "negative n_rows"),
        (dict(width=-1), "negative width"),
        (dict(n_rows=1 << 16, width=1 << 15), "exceeds 2^31 - 1"),
        (dict(ids=0), "ids_dev is NULL"),
        (dict(mask=0), "mask_dev is NULL"),
        (dict(prune=0), "prune_logits_dev is NULL"),
        (dict(rank=0), "rank_logits_dev is NULL"),
        (dict(ws=0), "workspace_dev is NULL"),
        (dict(), "NULL handle"),
        (dict(n_rows=0), "NULL handle"),  # (an empty batch still needs a handle)
    ):
        assert _call(lib, good, **kwargs) == _lib.OP_ERR_INVALID, kwargs
        assert text in _lib.last_error(lib, None), (kwargs, _lib.last_error(lib, None))


# -- the constructor argument ------------------------------------------------------------------------------------------------------
def test_attention_masks_argument_is_validated_and_defaults_to_prefix():
    from open_provence_amd.engine import ATTENTION_MASKS, HipEncoder, check_attention_masks
    from open_provence_amd.modeling import OpenProvenceModel

    assert ATTENTION_MASKS == ("prefix", "any")
    assert check_attention_masks(None) == "prefix" and check_attention_masks("prefix") == "prefix" and check_attention_masks("any") == "any"
    for wrong in ("left", "ANY", "", True, 1):
        with pytest.raises(ValueError, match="attention_masks"):
            check_attention_masks(wrong)
    for cls in (HipEncoder, OpenProvenceModel):
        assert inspect.signature(cls.__init__).parameters["attention_masks"].default == "prefix"
    assert callable(HipEncoder.forward_masked)
    # an unknown value is refused before anything touches the device or the library
    dims = mm.small_dims(*mm.SMALL[0][:6])
    with pytest.raises(ValueError, match="attention_masks"):
        HipEncoder(dims, attention_masks="holes")


def test_the_host_packers_keep_refusing():
    from open_provence_amd.packing import lengths_from_mask, pack_padded

    ids, mask, _ = mm.batch(77)
    with pytest.raises(NotImplementedError, match="right-padded"):
        lengths_from_mask(mask)
    with pytest.raises(NotImplementedError, match="right-padded"):
        pack_padded(ids, mask)
