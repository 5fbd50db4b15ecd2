"""The padded boundary's two C calls (op_pack_padded / op_unpack_padded) on a CPU-only box: declared, bound, exported -- additive
to ABI 10 -- and refused before any device call when malformed (both check their own arguments before they look at the handle)."""

import ctypes
import inspect
import re
from pathlib import Path

from open_provence_amd import _lib

HEADER = Path(__file__).resolve().parents[1] / "include" / "open_provence_hip.h"


def test_the_two_calls_are_declared_and_the_abi_version_stays():
    assert _lib.OP_ABI_VERSION == 10
    text = re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)
    for name in ("op_pack_padded", "op_unpack_padded"):
        assert name in _lib.EXPORTED_SYMBOLS
        assert re.search(rf"\bint {name}\s*\(", text), name
    assert "#define OP_ABI_VERSION 10" in text
    # uint32 + 7 x int32, then one int64: 40 bytes, no padding
    assert ctypes.sizeof(_lib.OpPaddedReport) == 40
    assert _lib.OpPaddedReport.id_value.offset == 32
    assert (_lib.OP_INT_I32, _lib.OP_INT_I64, _lib.OP_INT_U8) == (0, 1, 2)
    assert (_lib.OP_PADDED_BAD_MASK, _lib.OP_PADDED_BAD_ID) == (1, 2)


def test_library_exports_and_binds_the_calls(hip_library):
    assert hip_library.op_abi_version() == 10
    assert hasattr(hip_library, "op_pack_padded") and hasattr(hip_library, "op_unpack_padded")
    assert hip_library.op_pack_padded.argtypes[-2] is ctypes.POINTER(_lib.OpPaddedReport)
    assert len(hip_library.op_pack_padded.argtypes) == 12 and len(hip_library.op_unpack_padded.argtypes) == 8


def test_encoder_and_model_expose_the_device_path():
    from open_provence_amd.engine import HipEncoder

    assert list(inspect.signature(HipEncoder.pack_padded_device).parameters) == ["self", "input_ids", "attention_mask"]
    assert list(inspect.signature(HipEncoder.unpack_padded_device).parameters) == ["self", "values", "cu_seqlens", "n_rows", "width"]


def _report(**fields):
    report = _lib.OpPaddedReport()
    report.struct_bytes = ctypes.sizeof(_lib.OpPaddedReport)
    for k, v in fields.items():
        setattr(report, k, v)
    return report


# (never dereferenced: every call below is refused before the handle, let alone a device, is touched)
_BUF = ctypes.c_void_p(0x1000)
_HOST = (ctypes.c_int32 * 8)()


def _pack(lib, *, report=True, ids=_BUF, ids_dtype=_lib.OP_INT_I64, mask=_BUF, mask_dtype=_lib.OP_INT_U8, n_rows=4, width=6,
          packed=_BUF, cu=_BUF, cu_host=_HOST, **fields):
    rep = _report(**fields) if report else None
    return lib.op_pack_padded(None, ids, ids_dtype, mask, mask_dtype, n_rows, width, packed, cu, cu_host,
                              ctypes.byref(rep) if rep is not None else None, None)


def _unpack(lib, *, values=_BUF, cu=_BUF, n_rows=4, width=6, channels=2, out=_BUF):
    return lib.op_unpack_padded(None, values, cu, n_rows, width, channels, out, None)


def test_malformed_pack_calls_are_refused_before_the_handle(hip_library):
    lib = hip_library
    cases = [
        (dict(report=False), "report"),
        (dict(struct_bytes=12), "struct_bytes"),
        (dict(ids_dtype=_lib.OP_INT_U8), "ids_dtype"),
        (dict(ids_dtype=7), "ids_dtype"),
        (dict(mask_dtype=3), "mask_dtype"),
        (dict(mask_dtype=-1), "mask_dtype"),
        (dict(n_rows=-1), "n_rows"),
        (dict(width=-5), "width"),
        (dict(n_rows=1 << 16, width=1 << 15), "n_rows * width"),
        (dict(n_rows=(1 << 31) - 1, width=2), "n_rows * width"),
        (dict(ids=None), "ids_dev"),
        (dict(packed=None), "ids_packed_dev"),
        (dict(cu=None), "cu_seqlens_dev"),
        (dict(cu_host=None), "cu_seqlens_host"),
    ]
    for kwargs, field in cases:
        assert _pack(lib, **kwargs) == _lib.OP_ERR_INVALID, kwargs
        message = _lib.last_error(lib, None)
        assert field in message and "NULL handle" not in message, (kwargs, message)
    # a well-formed call gets as far as the handle: every dtype pair, no mask (its dtype is then ignored), the largest batch
    for kwargs in ([dict(ids_dtype=i, mask_dtype=m) for i in (_lib.OP_INT_I32, _lib.OP_INT_I64) for m in (0, 1, 2)]
                   + [dict(mask=None, mask_dtype=99), dict(n_rows=(1 << 31) - 1, width=1), dict(n_rows=0, ids=None, packed=None),
                      dict(width=0, ids=None, packed=None)]):
        assert _pack(lib, **kwargs) == _lib.OP_ERR_INVALID, kwargs
        assert "NULL handle" in _lib.last_error(lib, None), kwargs


def test_malformed_unpack_calls_are_refused_before_the_handle(hip_library):
    lib = hip_library
    cases = [
        (dict(channels=0), "channels"),
        (dict(channels=3), "channels"),
        (dict(n_rows=-2), "n_rows"),
        (dict(width=-1), "width"),
        (dict(n_rows=1 << 20, width=1 << 11), "n_rows * width"),
        (dict(values=None), "packed_dev"),
        (dict(cu=None), "cu_seqlens_dev"),
        (dict(out=None), "padded_dev"),
    ]
    for kwargs, field in cases:
        assert _unpack(lib, **kwargs) == _lib.OP_ERR_INVALID, kwargs
        message = _lib.last_error(lib, None)
        assert field in message and "NULL handle" not in message, (kwargs, message)
    for kwargs in (dict(), dict(channels=1), dict(n_rows=0, values=None, cu=None, out=None)):
        assert _unpack(lib, **kwargs) == _lib.OP_ERR_INVALID, kwargs
        assert "NULL handle" in _lib.last_error(lib, None), kwargs
