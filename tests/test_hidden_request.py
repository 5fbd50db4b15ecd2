"""The per-call hidden-state request of ABI 10 on a CPU-only box: declared, bound, and refused before any device call when
malformed (op_forward_packed_hidden checks the request's own fields before it looks at the handle)."""

import ctypes
import inspect

import torch

from open_provence_amd import _lib


def test_abi_10_declares_the_hidden_state_call():
    assert _lib.OP_ABI_VERSION == 10
    assert "op_forward_packed_hidden" in _lib.EXPORTED_SYMBOLS
    # uint32 + 2 x int32, then two pointers: 32 bytes on x86-64
    assert ctypes.sizeof(_lib.OpHiddenRequest) == 32
    assert (_lib.OP_HIDDEN_F32, _lib.OP_HIDDEN_BF16) == (0, 1)


def test_library_binds_the_call(hip_library):
    assert hip_library.op_abi_version() == 10
    assert hip_library.op_forward_packed_hidden.argtypes[-1] is ctypes.POINTER(_lib.OpHiddenRequest)


def test_model_and_wrappers_accept_the_keyword():
    from open_provence_amd.engine import HiddenRequest, HipEncoder
    from open_provence_amd.modeling import OpenProvenceForTokenClassification, OpenProvenceModel

    for fn in (OpenProvenceModel.forward, OpenProvenceForTokenClassification.forward):
        assert "output_hidden_states" in inspect.signature(fn).parameters
    for fn in (HipEncoder.forward_packed, HipEncoder.forward_packed_checked, HipEncoder.forward_packed_on):
        assert "hidden" in inspect.signature(fn).parameters
    req = HiddenRequest()
    assert req.layers is None and req.dtype == torch.float32 and req.pad_width == 0


def _call(lib, req, max_seqlen=8):
    return lib.op_forward_packed_hidden(None, None, None, None, 1, 8, max_seqlen, None, None, None, None, 0, None,
                                        ctypes.byref(req) if req is not None else None)


def _request(**fields):
    req = _lib.OpHiddenRequest()
    req.struct_bytes = ctypes.sizeof(_lib.OpHiddenRequest)
    for k, v in fields.items():
        setattr(req, k, v)
    return req


def test_malformed_requests_are_refused_before_the_handle(hip_library):
    assert _call(hip_library, _request(struct_bytes=12)) == _lib.OP_ERR_INVALID
    assert "struct_bytes" in _lib.last_error(hip_library, None)
    assert _call(hip_library, _request(dtype=2)) == _lib.OP_ERR_INVALID
    assert "dtype" in _lib.last_error(hip_library, None)
    assert _call(hip_library, _request(pad_width=7), max_seqlen=8) == _lib.OP_ERR_INVALID
    assert "pad_width" in _lib.last_error(hip_library, None)
    assert _call(hip_library, _request(pad_width=-1)) == _lib.OP_ERR_INVALID
    assert "pad_width" in _lib.last_error(hip_library, None)
    # a well-formed request (or none) gets as far as the handle
    for req in (_request(pad_width=8), _request(dtype=_lib.OP_HIDDEN_BF16), None):
        assert _call(hip_library, req) == _lib.OP_ERR_INVALID
        assert "NULL handle" in _lib.last_error(hip_library, None)
