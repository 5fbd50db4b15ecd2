"""``masked_kernels="selected"`` without a GPU: the keyword is validated before the device is touched, the two symbols are
declared and bound, and the host checks ``op_forward_masked_native`` makes (open_provence_amd/csrc/op_plan.h:
``check_masked_args``, ``check_masked_native_handle``, ``masked_native_layout``) hold under a host sanitizer.

tests/host/masked_check.cpp -- a program with a main of its own, no HIP -- is compiled with the host C++ compiler under
AddressSanitizer and UBSan (a plain build where the sanitized link fails, as tests/test_lookup_model.py does) and prints
``label code message`` per attempt; every expectation is written out here.  The wording and the order of the argument
refusals are those of ``op_forward_masked`` (open_provence_amd/csrc/op_forward_masked.hip), read from its source here."""

from __future__ import annotations

import re
import shutil
import subprocess
from pathlib import Path

import pytest

from open_provence_amd import _lib
from open_provence_amd import engine

ROOT = Path(__file__).resolve().parents[1]
SOURCE = ROOT / "tests" / "host" / "masked_check.cpp"
SANITIZE = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
FN = "op_forward_masked_native"


# -- the keyword ----------------------------------------------------------------------------------------------------------------------
def _dims(hidden=256, inter=384):
    import masked_model as mm

    dims = mm.small_dims(hidden, hidden // 64, "GLL", 16, "cls", 1)
    return dims if inter == dims.intermediate_size else type(dims)(**{**dims.__dict__, "intermediate_size": inter})


def test_masked_kernels_is_validated_before_the_device_is_touched(monkeypatch):
    assert engine.MASKED_KERNELS == ("fp32", "selected")
    assert engine.check_masked_kernels(None) == "fp32" and engine.check_masked_kernels("selected") == "selected"
    touched = []
    monkeypatch.setattr(_lib, "load_library", lambda *a, **k: touched.append("library") or pytest.fail("the library was loaded"))
    monkeypatch.setattr(engine, "require_gpu", lambda *a, **k: touched.append("device") or pytest.fail("the device was asked for"))
    monkeypatch.delenv("OPEN_PROVENCE_KERNEL_SET", raising=False)
    for bad in ("native", "any", "", 1, True):
        for masks in ("prefix", "any"):
            with pytest.raises(ValueError, match="masked_kernels"):
                engine.HipEncoder(_dims(), attention_masks=masks, masked_kernels=bad)
    # what op_forward_masked_native would refuse on every call is refused here, by name
    with pytest.raises(ValueError, match='kernel_set="fp32"'):
        engine.HipEncoder(_dims(), attention_masks="any", masked_kernels="selected", kernel_set="fp32")
    monkeypatch.setenv("OPEN_PROVENCE_KERNEL_SET", "fp32")
    with pytest.raises(ValueError, match='kernel_set="fp32"'):
        engine.HipEncoder(_dims(), attention_masks="any", masked_kernels="selected")
    monkeypatch.delenv("OPEN_PROVENCE_KERNEL_SET")
    with pytest.raises(ValueError, match="tiled path"):
        engine.HipEncoder(_dims(384, 192), attention_masks="any", masked_kernels="selected")
    with pytest.raises(ValueError, match="OP_FLAG_FORCE_TILED"):
        engine.HipEncoder(_dims(), attention_masks="any", masked_kernels="selected", flags=_lib.OP_FLAG_FORCE_TILED)
    assert touched == []


def test_only_the_pair_of_keywords_changes_anything():
    """The shape rule is restated from op_plan.h's paths_of; with attention_masks="prefix" the keyword refuses nothing."""

    ok = engine.check_masked_selected
    for hidden, inter in ((128, 192), (256, 384), (64, 32), (512, 256), (768, 1152)):
        ok(_dims(hidden, inter), 0, None)
        ok(_dims(hidden, inter), 0, "bf16x3")
    for hidden, inter in ((384, 192), (512, 192), (320, 256)):
        with pytest.raises(ValueError, match="tiled path"):
            ok(_dims(hidden, inter), 0, None)


def test_the_symbols_are_declared_and_bound():
    text = (ROOT / "include" / "open_provence_hip.h").read_text()
    assert re.search(r"\bsize_t\s+op_masked_native_workspace_bytes\s*\(", text) and re.search(r"\bint\s+op_forward_masked_native\s*\(", text)
    assert "op_forward_masked_native" in _lib.EXPORTED_SYMBOLS and "op_masked_native_workspace_bytes" in _lib.EXPORTED_SYMBOLS
    assert re.search(r"#define\s+OP_ABI_VERSION\s+10\b", text) and _lib.OP_ABI_VERSION == 10  # additive: detect by symbol


# -- the host checks -------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def answers(tmp_path_factory):
    compilers = [c for c in (shutil.which("c++"), shutil.which("g++"), "/opt/rocm/llvm/bin/clang++") if c and Path(c).exists()]
    assert compilers, "no host C++ compiler"
    exe, errors = tmp_path_factory.mktemp("masked") / "masked_check", []
    for extra in (SANITIZE, []):
        for cxx in compilers:
            built = subprocess.run([cxx, "-std=c++17", "-O1", "-g", *extra, str(SOURCE), "-o", str(exe)], capture_output=True, text=True)
            if built.returncode != 0:
                errors.append(f"{cxx} {' '.join(extra)}: {built.stderr[-2000:]}")
                continue
            done = subprocess.run([str(exe)], capture_output=True, text=True)
            if done.returncode == 0:
                return done.stdout.splitlines()
            errors.append(f"{cxx} {' '.join(extra)}: exit {done.returncode}: {done.stderr[-2000:]}")
    pytest.fail("masked_check.cpp does not build or run:\n" + "\n".join(errors))


def _refusals(answers):
    lines = [line.split(" ", 2) for line in answers if not line.startswith("layout ")]
    seen = {label: (int(code), message) for label, code, message in lines}
    assert len(seen) == len(lines)
    return seen


def test_argument_refusals_have_the_order_and_wording_of_op_forward_masked(answers):
    seen = _refusals(answers)
    for label in ("well_formed", "cells_below_the_limit", "empty_rows", "empty_width"):
        assert seen[label] == (_lib.OP_OK, "-"), label
    expected = {
        "null_report": "report is NULL", "report_struct_bytes": "op_masked_report.struct_bytes is 8, expected 24",
        "negative_rows": "negative n_rows -1", "negative_width": "negative width -5",
        "too_many_cells": "n_rows * width = 2147483648 exceeds 2^31 - 1", "null_ids": "ids_dev is NULL", "null_mask": "mask_dev is NULL",
        "null_prune": "prune_logits_dev is NULL", "null_rank": "rank_logits_dev is NULL", "null_workspace": "workspace_dev is NULL",
        "order_report_first": "report is NULL", "order_rows_before_width": "negative n_rows -1", "order_ids_first": "ids_dev is NULL",
    }
    for label, text in expected.items():
        assert seen[label] == (_lib.OP_ERR_INVALID, f"{FN}: {text}"), (label, seen[label])
    # the same sentences, in the same order, as the source of op_forward_masked states them under its own name
    source = (ROOT / "open_provence_amd" / "csrc" / "op_forward_masked.hip").read_text()
    body = source[source.index("int op_forward_masked(op_handle* h"):]
    theirs = re.findall(r'"op_forward_masked: ([^"%]*)', body[: body.index("if (!h) return fail(nullptr")])
    plan = (ROOT / "open_provence_amd" / "csrc" / "op_plan.h").read_text()
    mine = plan[plan.index("inline Refusal check_masked_args"):]
    ours = re.findall(r'"%s: ([^"%]*)', mine[: mine.index("return Refusal{};")])
    assert theirs == ours and len(ours) == 10


def test_handle_refusals_name_op_forward_masked(answers):
    seen = _refusals(answers)
    for label in ("row_path", "panel_path", "cleared_operands"):
        assert seen[label] == (_lib.OP_OK, "-"), label
    assert seen["too_wide"] == (_lib.OP_ERR_INVALID, f"{FN}: width 2049 exceeds max_position_embeddings 2048")
    assert seen["order_width_first"][0] == _lib.OP_ERR_INVALID
    for label, word in (("tiled_path", "tiled path"), ("set_fp32", '"fp32"'), ("order_path_before_set", "tiled path")):
        code, message = seen[label]
        assert code == _lib.OP_ERR_UNSUPPORTED and message.startswith(f"{FN}: ") and word in message, (label, code, message)
        assert "use op_forward_masked" in message or "op_forward_masked is" in message, message


def _up(v, a):
    return (v + a - 1) // a * a


def test_the_workspace_layout(answers):
    """cu_seqlens, the status word, key_row (one byte per row of the padded row capacity), vmean, the forward's workspace: in
    that order, each rounded up to 256 bytes.  The row capacity is restated here from the chunking rule."""

    rows = [line for line in answers if line.startswith("layout ")]
    assert len(rows) == 4
    for line in rows:
        left, right = line[len("layout "):].split(" : ")
        hidden, chunk_rows, n_rows, width, forward = (int(v) for v in left.split())
        cu, status, key_row, vmean, fwd, total = (int(v) for v in right.split())
        cap = min(_up(min(n_rows * width + 31 * n_rows, 1 << 30), 32), max(chunk_rows, _up(max(width, 1), 32)))
        r_pad = _up(cap + 64, 256)
        assert cu == 0 and status == _up((n_rows + 1) * 4, 256) and key_row == status + 256
        assert vmean == key_row + _up(r_pad, 256) and fwd == vmean + _up(n_rows * hidden * 4, 256) and total == fwd + _up(forward, 256)
        assert all(v % 256 == 0 for v in (cu, status, key_row, vmean, fwd, total))
