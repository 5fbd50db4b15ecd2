"""The attention-probability call (additive to ABI 10) on a CPU-only box: declared, bound, and refused before any device call
when malformed (op_attention_probs checks the request's own fields before it looks at the handle)."""

import ctypes
import inspect

from open_provence_amd import _lib


def test_abi_declares_the_attention_calls():
    assert _lib.OP_ABI_VERSION == 10
    assert "op_attention_probs" in _lib.EXPORTED_SYMBOLS and "op_attention_workspace_bytes" in _lib.EXPORTED_SYMBOLS
    # uint32 + 3 x int32, then two pointers: 32 bytes on x86-64
    assert ctypes.sizeof(_lib.OpAttentionRequest) == 32
    assert [name for name, _ in _lib.OpAttentionRequest._fields_] == ["struct_bytes", "layer", "dtype", "pad_width", "hidden_dev", "out_dev"]


def test_library_binds_the_calls(hip_library):
    assert hip_library.op_abi_version() == 10
    assert hip_library.op_attention_probs.argtypes[6] is ctypes.POINTER(_lib.OpAttentionRequest)
    assert hip_library.op_attention_workspace_bytes.restype is ctypes.c_size_t
    assert hip_library.op_attention_workspace_bytes(None, 1, 8, 8) == 0  # (no handle: no size)


def test_model_and_encoder_accept_the_keywords():
    from open_provence_amd.engine import AttentionRequest, HipEncoder
    from open_provence_amd.modeling import (OpenProvenceForSequenceClassification, OpenProvenceForTokenClassification,
                                            OpenProvenceModel)

    for fn in (OpenProvenceModel.forward, OpenProvenceForSequenceClassification.forward, OpenProvenceForTokenClassification.forward):
        assert "output_attentions" in inspect.signature(fn).parameters
    for fn in (HipEncoder.forward_packed, HipEncoder.forward_packed_checked, HipEncoder.forward_packed_on):
        assert "attentions" in inspect.signature(fn).parameters
    assert list(inspect.signature(HipEncoder.attention_probs).parameters)[1:] == [
        "hidden_packed", "layer", "cu_seqlens", "cu_seqlens_host", "max_seqlen", "pad_width"]
    for fn in (HipEncoder.__init__, OpenProvenceModel.__init__):
        assert inspect.signature(fn).parameters["attention_outputs"].default is False
    assert "output_attentions" not in inspect.signature(OpenProvenceModel.process).parameters
    req = AttentionRequest()
    assert req.layers is None and req.pad_width == 0


def _request(**fields):
    req = _lib.OpAttentionRequest()
    req.struct_bytes = ctypes.sizeof(_lib.OpAttentionRequest)
    req.dtype = _lib.OP_HIDDEN_F32
    req.pad_width = 8
    req.hidden_dev = 256  # (never dereferenced: every call below ends at the argument checks)
    req.out_dev = 256
    for k, v in fields.items():
        setattr(req, k, v)
    return req


def _call(lib, req, n_seqs=1, total=8, max_seqlen=8):
    return lib.op_attention_probs(None, None, None, n_seqs, total, max_seqlen, ctypes.byref(req) if req is not None else None, None, 0, None)


def test_malformed_requests_are_refused_before_the_handle(hip_library):
    lib = hip_library
    for req, word in [(None, "request"), (_request(struct_bytes=12), "struct_bytes"), (_request(dtype=_lib.OP_HIDDEN_BF16), "dtype"),
                      (_request(dtype=7), "dtype"), (_request(pad_width=7), "pad_width"), (_request(pad_width=-1), "pad_width"),
                      (_request(hidden_dev=None), "hidden_dev"), (_request(out_dev=None), "out_dev")]:
        assert _call(lib, req) == _lib.OP_ERR_INVALID
        assert word in _lib.last_error(lib, None), (word, _lib.last_error(lib, None))
    # a non-empty batch needs a width of its own even when max_seqlen is given as 0
    assert _call(lib, _request(pad_width=0), max_seqlen=0) == _lib.OP_ERR_INVALID
    assert "pad_width" in _lib.last_error(lib, None)
    # per-sequence rows are 32-bit indices
    assert _call(lib, _request(pad_width=1 << 20), n_seqs=1 << 12, total=1 << 12) == _lib.OP_ERR_INVALID
    assert "2^31" in _lib.last_error(lib, None)
    # a well-formed request gets as far as the handle -- whatever its layer, which only the handle can judge
    for req in (_request(), _request(pad_width=131), _request(layer=99), _request(layer=-1)):
        assert _call(lib, req) == _lib.OP_ERR_INVALID
        assert "NULL handle" in _lib.last_error(lib, None)
    # an empty batch needs no buffers
    assert _call(lib, _request(hidden_dev=None, out_dev=None, pad_width=0), n_seqs=0, total=0, max_seqlen=0) == _lib.OP_ERR_INVALID
    assert "NULL handle" in _lib.last_error(lib, None)


def test_model_without_the_packs_refuses_the_flag():
    """``output_attentions`` was swallowed by **kwargs until now; a model that cannot serve it says so (and how to get one)."""

    import pytest
    import torch

    from helpers import host_only_model

    class _Encoder:
        attention_outputs = False

    model = host_only_model()
    model.encoder = _Encoder()
    with pytest.raises(ValueError, match="attention_outputs=True"):
        model.forward(input_ids=torch.zeros((1, 4), dtype=torch.int64), output_attentions=True)
