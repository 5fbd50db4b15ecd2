"""Kernel set "fp32" (12) on a CPU-only box: numbers and names agree between the header and the Python binding, the library
loads and exports what the header declares, and the two new arguments are validated before anything touches a device."""

from __future__ import annotations

import re
from pathlib import Path

import pytest

from open_provence_amd import _lib

HEADER = Path(__file__).resolve().parents[1] / "include" / "open_provence_hip.h"


def _header_value(name: str) -> int:
    text = HEADER.read_text()
    found = re.search(rf"\b{name}\s*=\s*(-?\d+)", text) or re.search(rf"#define\s+{name}\s+(\d+)u?\b", text)
    assert found, f"{name} is not in {HEADER.name}"
    return int(found.group(1))


def test_the_set_has_number_12_and_the_name_fp32():
    assert _lib.KERNEL_SET_IDS["fp32"] == 12 and _lib.KERNEL_SET_NAMES[12] == "fp32"
    assert _header_value("OP_KS_F32") == 12 and _header_value("OP_KS_COUNT") == 13
    assert sorted(n for n in _lib.KERNEL_SET_NAMES if n >= 0) == list(range(_header_value("OP_KS_COUNT")))
    assert "fp32" not in _lib.FP16_PLANE_SETS  # no fp16 plane: the range guard does not apply


def test_flag_and_calibration_bit_agree_with_the_header():
    assert _lib.OP_FLAG_F32_PACKS == _header_value("OP_FLAG_F32_PACKS") == 16384
    assert _lib.OP_CAL_REFERENCE_F32 == _header_value("OP_CAL_REFERENCE_F32") == 4
    # the next free bit: no other create flag of the header or the binding has it
    flags = {int(v) for v in re.findall(r"\bOP_FLAG_\w+\s*=\s*(\d+)", HEADER.read_text())}
    assert len(flags) == len(re.findall(r"\bOP_FLAG_\w+\s*=\s*\d+", HEADER.read_text())) and max(flags) == 16384
    assert [n for n in dir(_lib) if n.startswith("OP_FLAG_") and getattr(_lib, n) == 16384] == ["OP_FLAG_F32_PACKS"]
    assert {_lib.OP_CAL_FULL_REPORT, _lib.OP_CAL_WHOLE_DEPTH, _lib.OP_CAL_REFERENCE_F32} == {1, 2, 4}


def test_the_library_loads_without_a_gpu_and_exports_what_the_header_names(hip_library):
    declared = set(re.findall(r"\b(op_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)))
    assert declared == set(_lib.EXPORTED_SYMBOLS)
    for symbol in declared:
        assert hasattr(hip_library, symbol), symbol
    assert hip_library.op_abi_version() == _lib.OP_ABI_VERSION == _header_value("OP_ABI_VERSION")


def test_kernel_set_and_calibration_reference_are_validated_before_the_device():
    from open_provence_amd.engine import CALIBRATION_REFERENCES, HipEncoder, check_arithmetic_arguments
    from open_provence_amd.synthetic import named_dims

    assert CALIBRATION_REFERENCES == ("bf16x3", "fp32")
    assert check_arithmetic_arguments("fp32", None) == ("fp32", "bf16x3")
    assert check_arithmetic_arguments("auto", "fp32") == (None, "fp32")
    assert check_arithmetic_arguments(None, "bf16x3") == (None, "bf16x3")
    dims = named_dims("xsmall")
    for bad in (dict(kernel_set="fp64"), dict(calibration_reference="fp64"), dict(calibration_reference="f16"),
                dict(kernel_set="FP32")):
        with pytest.raises(ValueError):
            check_arithmetic_arguments(bad.get("kernel_set"), bad.get("calibration_reference"))
        with pytest.raises(ValueError):  # (raised before the library or a device is looked for)
            HipEncoder(dims, **bad)


def test_the_model_class_validates_them_too():
    from helpers import CharTokenizer
    from open_provence_amd.config import OpenProvenceConfig
    from open_provence_amd.modeling import OpenProvenceModel

    base = dict(model_type="modernbert", vocab_size=512, hidden_size=128, intermediate_size=192, num_hidden_layers=3,
                num_attention_heads=2, local_attention=16, global_attn_every_n_layers=3, max_position_embeddings=2048)
    cfg = OpenProvenceConfig(base_model_config=base, tokenizer_name_or_path="x", pruning_config={"hidden_size": 128}, max_length=128)
    for bad in (dict(kernel_set="fp64"), dict(calibration_reference="fp64")):
        with pytest.raises(ValueError, match="fp64"):
            OpenProvenceModel(cfg, tokenizer=CharTokenizer(), **bad)
