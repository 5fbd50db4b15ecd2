"""The RoPE tables the library builds (op_create -> build_rope_host, both in op_api.hip, reached through op_debug_rope_tables)
against the reference's recipe in torch fp32 (``oracle.modernbert_oracle.rope_tables``: inv_freq = 1 / theta ** (arange(0, 64,
2, fp32) / 64), an fp32 power and an fp32 reciprocal; angle = fp32(pos) * inv_freq; cos / sin of that fp32 angle), for both
thetas of the published checkpoints, head_dim 64 and positions 0 .. 8191.

Bound: max |library - torch| <= 2^-23 over both tables.  Both sides are within one ulp of the true cos / sin of the SAME fp32
angle and every value is at most 1, so the bound holds exactly when the two agree on every angle, that is on every inv_freq
entry bit for bit: a single entry one ulp off moves the angle at position p by p x 2^-24 relative, which is 1.5e-5 or more in
the table by position 2048 -- over 100 x the bound.  (A library that rounds inv_freq once, as (float)(1.0 / pow(theta, e)),
differs in 10 of 32 entries at theta 10000 and 8 of 32 at 160000, and by 1.2e-4 / 6.1e-5 in the tables at 8192 positions.)

The host-side call needs no device; the GPU test holds the tables of a handle, as they lie on the device, to the same call."""

from __future__ import annotations

import ctypes
import hashlib

import pytest
import torch

THETAS = [10000.0, 160000.0]
HEAD_DIM = 64
POSITIONS = 8192
BOUND = 2.0**-23


def _library_tables(lib, theta: float, n: int):
    cos, sin = torch.full((n, HEAD_DIM // 2), 7.0), torch.full((n, HEAD_DIM // 2), 7.0)
    code = lib.op_debug_rope_tables(None, 0, theta, n, ctypes.c_void_p(cos.data_ptr()), ctypes.c_void_p(sin.data_ptr()))
    assert code == 0, code
    return cos, sin


@pytest.mark.parametrize("theta", THETAS)
def test_library_tables_are_the_reference_recipe(hip_library, theta):
    from oracle.modernbert_oracle import rope_tables

    cos, sin = _library_tables(hip_library, theta, POSITIONS)
    ref_cos, ref_sin = rope_tables(HEAD_DIM, theta, torch.arange(POSITIONS))
    half = HEAD_DIM // 2
    assert ref_cos.dtype == torch.float32 and ref_cos.shape == (POSITIONS, HEAD_DIM)
    # the kernels read column k for dimensions k and k + 32: the reference's two halves are one table
    assert torch.equal(ref_cos[:, :half], ref_cos[:, half:]) and torch.equal(ref_sin[:, :half], ref_sin[:, half:])
    d_cos, d_sin = (cos.double() - ref_cos[:, :half].double()).abs(), (sin.double() - ref_sin[:, :half].double()).abs()
    worst = max(float(d_cos.max()), float(d_sin.max()))
    at_2048 = max(float(d_cos[:2048].max()), float(d_sin[:2048].max()))
    columns = sorted(set(torch.nonzero((d_cos > BOUND) | (d_sin > BOUND))[:, 1].tolist()))
    inv_freq = 1.0 / (theta ** (torch.arange(0, HEAD_DIM, 2, dtype=torch.float32) / HEAD_DIM))
    print(f"[rope tables] theta {theta:g}: max |library - torch| {worst:.3e} over {POSITIONS} positions, {at_2048:.3e} over the "
          f"first 2048 (bound {BOUND:.3e}); columns over the bound: {columns}; torch {torch.__version__} inv_freq sha256 "
          f"{hashlib.sha256(inv_freq.numpy().tobytes()).hexdigest()[:16]}")
    assert worst <= BOUND, f"theta {theta:g}: {worst:.3e} > {BOUND:.3e}, in columns {columns}"


def test_rope_table_call_validates_its_arguments(hip_library):
    buf = torch.zeros(4, HEAD_DIM // 2)
    ptr = ctypes.c_void_p(buf.data_ptr())
    call = hip_library.op_debug_rope_tables
    assert call(None, 0, 10000.0, 4, ptr, ptr) == 0
    for bad in ((None, 0, 10000.0, 0, ptr, ptr), (None, 0, 0.0, 4, ptr, ptr), (None, 0, 10000.0, 4, None, ptr),
                (None, 0, 10000.0, 4, ptr, None)):
        assert call(*bad) < 0, bad
    # a shorter table is the head of a longer one (each entry depends on its position alone)
    short, long = _library_tables(hip_library, 160000.0, 5), _library_tables(hip_library, 160000.0, 9)
    assert torch.equal(short[0], long[0][:5]) and torch.equal(short[1], long[1][:5])


@pytest.mark.gpu
def test_a_handle_holds_these_tables_on_its_device(hip_library):
    """What the kernels read: the two tables of a handle with max_position_embeddings 8192, copied back from its device,
    are bit for bit the host call's tables for the handle's two thetas."""

    import test_kernel_set_conformance as conf
    from open_provence_amd.engine import HipEncoder

    dims = conf._dims("row128", max_position_embeddings=POSITIONS)
    enc = HipEncoder(dims, device="cuda:0", flags=0)
    try:
        for is_global, theta in ((False, dims.local_rope_theta), (True, dims.global_rope_theta)):
            cos, sin = enc.rope_tables(is_global)
            want_cos, want_sin = _library_tables(hip_library, float(theta), POSITIONS)
            assert torch.equal(cos, want_cos) and torch.equal(sin, want_sin), theta
    finally:
        enc.close()
