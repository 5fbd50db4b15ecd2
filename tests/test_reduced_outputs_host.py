"""Pooled hidden states and attention rows, without a GPU: the new symbols and their ctypes structs against the header, the
new request fields' validation, and the float64 restatements of the two reductions (tests/reduced_outputs_model.py) against
torch's mean -- with three wrong restatements the GPU tests' 1-ulp distance must tell apart."""

import ctypes
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest
import torch

import reduced_outputs_model as rom
from open_provence_amd import _lib

HEADER_DIR = Path(__file__).resolve().parents[1] / "include"


def test_library_exports_the_new_calls(hip_library):
    for name in ("op_forward_packed_pooled", "op_attention_rows"):
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(hip_library, name), name
    assert hip_library.op_abi_version() == 10  # (additive: detected by symbol)


STRUCTS = {
    "op_pool_request": (_lib.OpPoolRequest, ["struct_bytes", "kind", "select", "out_dev", "scratch_dev", "scratch_bytes"]),
    "op_attention_rows_request": (_lib.OpAttentionRowsRequest, ["struct_bytes", "layer", "pad_width", "reduce_heads", "hidden_dev",
                                                                "query_pos_dev", "query_pos_host", "out_dev"]),
    # (unchanged by this feature: pinned here beside the new ones)
    "op_hidden_request": (_lib.OpHiddenRequest, ["struct_bytes", "dtype", "pad_width", "select", "out_dev"]),
    "op_attention_request": (_lib.OpAttentionRequest, ["struct_bytes", "layer", "dtype", "pad_width", "hidden_dev", "out_dev"]),
}


def test_ctypes_structs_match_the_header(tmp_path):
    """A stand-alone C program compiled against include/open_provence_hip.h prints sizeof and offsetof of every field."""

    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    assert cc, "no host C compiler"
    lines = []
    for name, (_, fields) in STRUCTS.items():
        lines.append(f'  printf("{name} %zu\\n", sizeof({name}));')
        lines += [f'  printf("{name}.{f} %zu\\n", offsetof({name}, {f}));' for f in fields]
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "open_provence_hip.h"\nint main(void) {\n' + "\n".join(lines)
                   + "\n  return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.run([cc, "-std=c99", f"-I{HEADER_DIR}", str(src), "-o", str(exe)], check=True, capture_output=True, text=True)
    printed = dict(line.split() for line in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    for name, (struct, fields) in STRUCTS.items():
        assert [f for f, _ in struct._fields_] == fields, name
        assert ctypes.sizeof(struct) == int(printed[name]), name
        for f in fields:
            assert getattr(struct, f).offset == int(printed[f"{name}.{f}"]), f"{name}.{f}"
    assert (_lib.OP_HIDDEN_POOL_FIRST, _lib.OP_HIDDEN_POOL_MEAN) == (0, 1) and _lib.POOL_KINDS == {"first": 0, "mean": 1}
    header = (HEADER_DIR / "open_provence_hip.h").read_text()
    assert "OP_HIDDEN_POOL_FIRST = 0, OP_HIDDEN_POOL_MEAN = 1" in header


def test_request_fields_validate_without_a_device():
    from open_provence_amd.engine import AttentionRequest, HiddenRequest

    assert HiddenRequest().pool is None and AttentionRequest().query is None and AttentionRequest().reduce_heads is False
    for kind in ("first", "mean"):
        assert HiddenRequest(layers=[0, 2], pool=kind).pool == kind
    for bad in (dict(pool="max"), dict(pool="cls"), dict(pool=1), dict(pool="mean", pad_width=8), dict(pool="first", dtype=torch.bfloat16)):
        with pytest.raises(ValueError):
            HiddenRequest(**bad)
    assert AttentionRequest(query="first", reduce_heads=True).reduce_heads
    assert AttentionRequest(query=torch.tensor([0, 3], dtype=torch.int32)).query.numel() == 2
    for bad in (dict(query="last"), dict(query=3), dict(query=torch.tensor([0.0])), dict(query=torch.zeros(2, 2, dtype=torch.int64)),
                dict(query=torch.tensor([1, -1])), dict(reduce_heads=True), dict(query="first", reduce_heads=2)):
        with pytest.raises(ValueError):
            AttentionRequest(**bad)


LENGTHS = [0, 1, 5, 63, 64, 65, 129, 300]


def _entry(seed=3, hidden=48):
    rng = np.random.default_rng(seed)
    cu = np.concatenate(([0], np.cumsum(LENGTHS))).astype(np.int32)
    # (an offset and a spread of magnitudes: a mean that cancels to nothing has no relative bound)
    entry = (rng.standard_normal((int(cu[-1]), hidden)) * np.exp(rng.uniform(-3, 3, hidden)) + rng.uniform(0.5, 2.0, hidden)).astype(np.float32)
    return entry, cu


def _rows(seed=5, heads=6, width=67):
    rng = np.random.default_rng(seed)
    logits = rng.standard_normal((len(LENGTHS), heads, width)) * 3
    return (np.exp(logits) / np.exp(logits).sum(-1, keepdims=True)).astype(np.float32)


def test_restatements_agree_with_torch():
    entry, cu = _entry()
    first, mean = rom.pooled_first(entry, cu), rom.pooled_mean(entry, cu)
    assert first.dtype == mean.dtype == np.float32 and first.shape == mean.shape == (len(LENGTHS), entry.shape[1])
    for s, n in enumerate(LENGTHS):
        if n == 0:
            for out in (first, mean):
                assert (out[s] == 0).all() and not np.signbit(out[s]).any()
            continue
        rows = torch.from_numpy(entry[cu[s]: cu[s + 1]])
        assert (first[s] == entry[cu[s]]).all()
        assert (mean[s] == rows.double().mean(0).float().numpy()).all()
    rows = _rows()
    assert (rom.head_mean(rows) == torch.from_numpy(rows).double().mean(1).float().numpy()).all()
    assert rom.ulp_distance(mean, mean) == 0 and rom.ulp_distance(np.nextafter(mean, np.float32(np.inf)), mean) <= rom.ULP_BOUND


def test_wrong_restatements_are_beyond_the_bound():
    entry, cu = _entry()
    want = rom.pooled_mean(entry, cu)
    assert rom.ulp_distance(rom.pooled_mean_length_rounded_up(entry, cu), want) > rom.ULP_BOUND
    assert rom.ulp_distance(rom.pooled_mean_without_last_token(entry, cu), want) > rom.ULP_BOUND
    rows = _rows()
    assert rom.ulp_distance(rom.head_mean_one_head_missing(rows), rom.head_mean(rows)) > rom.ULP_BOUND
    # each sequence that can show the bug shows it: not the longest row alone
    for wrong, affected in ((rom.pooled_mean_length_rounded_up, [n % 32 != 0 for n in LENGTHS]),
                            (rom.pooled_mean_without_last_token, [n > 0 for n in LENGTHS])):
        got = wrong(entry, cu)
        for s, hit in enumerate(affected):
            assert (rom.ulp_distance(got[s], want[s]) > rom.ULP_BOUND) == (hit and LENGTHS[s] > 0), (wrong.__name__, LENGTHS[s])
