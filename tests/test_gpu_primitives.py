"""The device primitives under every kernel, element by element (``op_debug_primitive`` -> ``opk_probe.hip.h``, which calls
the functions of ``opk_common.hip.h`` -- nothing is restated on the device side).

Every conformance module compares a whole forward with ``tests/arith_model.py``; that model ASSUMES that ``am.rne`` /
``am.e4m3`` (torch's CPU casts) are what v_cvt_pk_bf16_f32, v_cvt_pk_f16_f32, v_fma_mix_f32, v_cvt_scalef32_pk_fp8_f32 / _f16
and v_cvt_pk_fp8_f32 produce under the MODE.FP16_OVFL bit the kernels flip, and takes the fp32 GELU polynomial, the exponentials,
RoPE and the keep-probability as exact to 1e-6.  Here both assumptions are held on ``tests/primitive_inputs.py``'s sweeps: all
fp16 and bf16 bit patterns, every tie with its fp32 neighbours, the subnormal, +-448 and 65504 / 65520 edges, -0, Inf and NaN,
the lo-plane and weight-plane shifts; 4 M points of [-12, 12] and a log grid to +-3e38 for the functions.

  * conversions: bit for bit (decoded values compared exactly, so +0 == -0; NaN positions exactly) against ``am.rne`` /
    ``am.e4m3``, in both conversion modes.  An fp32-subnormal input may be read as itself or as a zero of its sign -- one
    choice per primitive, printed; nothing else is left out.
  * GELU: the two forms bit-identical; against float64 erfc within 1.25 x the fp32 emulation's maximum on the same inputs
    (measured here: 6.39e-7 on the [-12, 12] grid near x = 4; the 25 % is v_exp_f32's last place, |x| he(|x|) 2^-23 <= 2e-8)
    and below ``am.FLOOR``; on x < 0, where gelu = -|x| he(|x|) has no cancellation, within 2^-21 RELATIVE of the emulation
    (v_exp_f32's bound plus three roundings: ``primitive_inputs.GELU_TAIL_REL``) -- the absolute bounds cannot see the 5th digit
    of the three leading coefficients, this one sees every digit fp32 holds; exact ends; non-finite in, non-finite out.
  * exp2 / __expf / keep-probability / RoPE: exact special values, monotonicity, and bounds derived from the formats:
    2^-22 relative (four fp32 ulps: below the floor and 2^10 below what any operand format keeps of p), 1e-6 absolute for
    __expf on p <= 1, ``KEEP_PROB_BOUND`` of the geometry module over the whole difference range, one product rounding plus one
    FMA rounding for RoPE.
  * the scaled e4m3 MFMA: 128 a b 2^-18 exactly, in both operand orders of both products.

Every measured maximum is printed in the ``[primitives]`` table when the module ends."""

from __future__ import annotations

import ctypes
import math

import numpy as np
import pytest
import torch

import arith_model as am
import primitive_inputs as pi
import test_kernel_set_conformance as conf
from test_kernel_set_geometry import KEEP_PROB_BOUND

pytestmark = pytest.mark.gpu

BF16, F16, F8 = pi.BF16, pi.F16, pi.F8
TABLE: list[str] = []
MODES = {0: "overflowing", 1: "saturating"}


@pytest.fixture(scope="module", autouse=True)
def _print_table():
    yield
    print("\n[primitives] primitive                          mode         | elements compared, mismatches, sign-of-zero differences, "
          "fp32-subnormal inputs read as | measured maxima")
    for line in TABLE:
        print("[primitives]", line)


@pytest.fixture(scope="module")
def enc():
    from open_provence_amd.engine import HipEncoder

    e = HipEncoder(conf._dims("row128"), device="cuda:0")  # (no weights: the hook needs the handle's device only)
    yield e
    e.close()


def _bits16(words: torch.Tensor, dtype) -> torch.Tensor:
    return torch.from_numpy(words.numpy().astype(np.uint16).view(np.int16).copy()).view(dtype).to(torch.float64)


def _bytes8(words: torch.Tensor) -> torch.Tensor:
    return torch.from_numpy(words.numpy().astype(np.uint8).copy()).view(F8).to(torch.float64)


def _hex(v: torch.Tensor) -> list:
    return [f"{float(x)!r} (0x{int(b) & 0xFFFFFFFF:08x})" for x, b in zip(v, v.view(torch.int32))]


def _hold(label: str, mode: "int | None", v: torch.Tensor, got: torch.Tensor, expect, where: torch.Tensor) -> list:
    """`got` (decoded float64, one per element of the fp32 inputs `v`) against expect(inputs) on the elements of `where`.
    Returns the failure messages (empty: it holds) and adds the table line."""

    sub = pi.is_f32_subnormal(v) & where
    exp_v, exp_f = expect(v), expect(pi.flushed(v))
    bad_v, bad_f = pi.mismatches(got, exp_v) & where, pi.mismatches(got, exp_f) & where
    on_v, on_f = not bool(bad_v[sub].any()), not bool(bad_f[sub].any())
    reads = "either" if on_v and on_f else "v" if on_v else "zero" if on_f else "MIXED"
    bad = bad_f if reads == "zero" else bad_v
    exp = exp_f if reads == "zero" else exp_v
    n_bad = int(bad.sum())
    zs = pi.zero_sign_differences(got[where], exp[where])
    TABLE.append(f"{label:34s} {MODES.get(mode, '-'):12s} | {int(where.sum()):8d} {n_bad:8d} {zs:6d}  {reads}")
    out = []
    if reads == "MIXED":
        out.append(f"{label}: fp32-subnormal inputs are read neither all as themselves ({int(bad_v[sub].sum())} off) nor all as zeros "
                   f"({int(bad_f[sub].sum())} off)")
    if n_bad:
        idx = torch.nonzero(bad).flatten()[:8]
        out.append(f"{label} mode {mode}: {n_bad} of {int(where.sum())} differ; first: "
                   + "; ".join(f"v = {h}: device {float(g)!r}, model {float(e)!r}" for h, g, e in zip(_hex(v[idx]), got[idx], exp[idx])))
    return out


def _note(label: str, mode: "int | None", text: str) -> None:
    TABLE.append(f"{label:34s} {MODES.get(mode, '-'):12s} | {text}")


# -- the hook's argument checks -----------------------------------------------------------------------------------------------------
def test_invalid_arguments_are_refused_before_anything_runs(enc):
    from open_provence_amd import _lib

    call, h = enc.lib.op_debug_primitive, enc._handle
    buf = torch.zeros(64, dtype=torch.float32, device=enc.device)
    out = torch.zeros(1024, dtype=torch.float32, device=enc.device)
    src, dst = ctypes.c_void_p(buf.data_ptr()), ctypes.c_void_p(out.data_ptr())
    assert call(None, 0, 0, src, 4, dst, None) == _lib.OP_ERR_INVALID
    for kind in (-1, len(_lib.PROBE_KINDS), 1000):
        assert call(h, kind, 0, src, 4, dst, None) == _lib.OP_ERR_INVALID
    for mode in (-1, 2):
        assert call(h, 0, mode, src, 4, dst, None) == _lib.OP_ERR_INVALID
    for name, (kind, _, group, _, _) in _lib.PROBE_KINDS.items():
        if group > 1:
            assert call(h, kind, 0, src, group + 1, dst, None) == _lib.OP_ERR_INVALID, name
        assert call(h, kind, 0, None, group, dst, None) == _lib.OP_ERR_INVALID, name
        assert call(h, kind, 0, src, group, None, None) == _lib.OP_ERR_INVALID, name
        assert call(h, kind, 1, None, 0, None, None) == _lib.OP_OK, name
    torch.cuda.synchronize()
    assert float(out.abs().sum()) == 0.0  # nothing ran
    assert sorted(v[0] for v in _lib.PROBE_KINDS.values()) == list(range(len(_lib.PROBE_KINDS)))
    assert enc.debug_primitive("GELU", 0, torch.zeros(0)).shape == (0, 2)


# -- conversions, bit for bit ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [0, 1])
def test_bf16_split(enc, mode):
    v = pi.sweep()
    rec = enc.debug_primitive("BF16_SPLIT", mode, v).view(-1, 7)
    finite, nan = torch.isfinite(v), torch.isnan(v)
    fails = []
    for name, (h, l) in {"split2": (0, 1), "split2_pk": (2, 3), "split4": (4, 5)}.items():
        fails += _hold(f"BF16_SPLIT {name} hi", mode, v, _bits16(rec[:, h], BF16), lambda x: pi.expect_bf16_split(x, mode=mode)[0], finite)
        fails += _hold(f"BF16_SPLIT {name} lo", mode, v, _bits16(rec[:, l], BF16), lambda x: pi.expect_bf16_split(x, mode=mode)[1], finite)
        assert bool(torch.isnan(_bits16(rec[:, h], BF16)[nan]).all()), f"{name}: NaN in must give a NaN hi"
    # the three forms agree bit for bit on every input, NaN payloads included
    same = bool((rec[:, 0:2] == rec[:, 2:4]).all()) and bool((rec[:, 0:2] == rec[:, 4:6]).all())
    _note("BF16_SPLIT three forms", mode, "bit-identical on every input" if same else "DIFFER")
    # f2bf is integer arithmetic: no conversion mode enters, a finite value beyond the range rounds to Inf as am.rne's does
    fails += _hold("BF16_SPLIT f2bf (finite inputs)", mode, v, _bits16(rec[:, 6], BF16), lambda x: pi.expect_bf16_split(x)[0], finite)
    # below 0x7f7f8000 (the tie to the first value out of range) the expectation IS am.rne, in either mode
    reach = finite & (v.abs() < float(np.uint32(0x7F7F8000).view(np.float32)))
    hi_own = am.rne(v.double(), BF16)
    own = (hi_own, am.rne(v.double() - hi_own, BF16))
    for j in range(2):
        assert not bool(pi.mismatches(pi.expect_bf16_split(v, mode=mode)[j][reach], own[j][reach]).any())
    _note("BF16_SPLIT |v| >= 0x7f7f8000", mode, f"{int((finite & ~reach).sum())} finite inputs round to "
          + ("+-max bf16 (the conversion clamps; am.rne: Inf)" if mode == 1 else "Inf, as am.rne"))
    assert same, "split2 / split2_pk / split4 differ in some bit"
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("mode", [0, 1])
def test_f16_pair(enc, mode):
    v = pi.sweep()
    rec = enc.debug_primitive("F16_PAIR", mode, v).view(-1, 3)
    hi, lo, f2h = (_bits16(rec[:, j], F16) for j in range(3))
    finite = torch.isfinite(v)
    exp_hi = pi.expect_f16_pair(v, mode)[0]
    fails = _hold("F16_PAIR hi", mode, v, hi, lambda x: pi.expect_f16_pair(x, mode)[0], finite)
    fails += _hold("F16_PAIR lo (finite hi)", mode, v, lo, lambda x: pi.expect_f16_pair(x, mode)[1], finite & torch.isfinite(exp_hi))
    fails += _hold("F16_PAIR f2h", mode, v, f2h, lambda x: pi.expect_f16_pair(x, mode)[2], finite)
    assert not bool(torch.isfinite(hi[~finite]).any()) and bool(torch.isnan(hi[torch.isnan(v)]).all()), "a non-finite input gave a finite hi"
    if mode == 1:
        assert float(hi[finite].abs().max()) == 65504.0 and float(f2h[finite].abs().max()) == 65504.0  # clamps, as OP_FLAG_PANEL_F8's text says
    else:
        assert bool(torch.isinf(hi[finite & (v.abs() >= 65520.0)]).all())
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("mode", [0, 1])
def test_f16_f8(enc, mode):
    v = pi.sweep()
    rec = enc.debug_primitive("F16_F8", mode, v).view(-1, 2)
    hi, lo = _bits16(rec[:, 0], F16), _bytes8(rec[:, 1]) / 2.0**am.LO_SHIFT
    finite = torch.isfinite(v)
    exp_hi, exp_lo = pi.expect_f16_f8(v, mode)
    fails = _hold("F16_F8 hi", mode, v, hi, lambda x: pi.expect_f16_f8(x, mode)[0], finite)
    fails += _hold("F16_F8 lo (finite hi)", mode, v, lo, lambda x: pi.expect_f16_f8(x, mode)[1], finite & torch.isfinite(exp_hi))
    sat = finite & torch.isfinite(exp_hi) & (((v.double() - exp_hi) * 2.0**am.LO_SHIFT).abs() > 448.0)
    _note("F16_F8 lo beyond +-448", mode, f"{int(sat.sum())} inputs: {int(torch.isnan(lo[sat]).sum())} NaN, "
          f"{int((lo[sat].abs() * 2.0**am.LO_SHIFT == 448.0).sum())} at +-448")
    if mode == 1:  # the lo plane saturates and is never NaN for a finite input
        assert not bool(torch.isnan(lo[finite]).any()), "a finite input gave a NaN lo byte in saturating mode"
        assert int(sat.sum()) > 0 and bool((lo[sat].abs() * 2.0**am.LO_SHIFT == 448.0).all())
        # ... and there it IS the model's am.e4m3
        assert not bool(pi.mismatches(exp_lo[finite], am.e4m3(v.double() - exp_hi, am.LO_SHIFT)[finite]).any())
    assert not bool(torch.isfinite(hi[~finite]).any()), "a non-finite input gave a finite hi"
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("mode", [1, 0])
def test_e4m3_of_every_fp16_value(enc, mode):
    h = pi.fp16_patterns()
    val = torch.from_numpy(pi.fp16_grid())
    got = _bytes8(enc.debug_primitive("E4M3_F16", mode, h).view(-1))
    everything = torch.ones_like(val, dtype=torch.bool)
    fails = _hold("E4M3_F16 all 65536 patterns", mode, val, got, lambda x: pi.expect_e4m3_f16(x, mode), everything)
    if mode == 1:
        assert not bool(pi.mismatches(pi.expect_e4m3_f16(val, 1), am.e4m3(val.double())).any())  # the expectation IS am.e4m3
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("mode", [1, 0])
def test_e4m3_of_fp32_and_the_weight_planes(enc, mode):
    v = pi.sweep()
    rec = enc.debug_primitive("E4M3_F32", mode, v).view(-1, 3)
    finite = torch.isfinite(v)
    scale = (0, am.W_SHIFT, am.LO_SHIFT + am.W_SHIFT)
    names = ("f32x4_to_e4m3", "weight plane (x 2^6)", "weight lo plane (x 2^18)")
    fails = []
    for j in range(3):
        got = _bytes8(rec[:, j]) / 2.0 ** scale[j]
        fails += _hold(f"E4M3_F32 {names[j]}", mode, v, got, lambda x, j=j: pi.expect_e4m3_f32(x, mode)[j], finite)
        if mode == 1:
            # never NaN for a finite input -- up to the weights whose shifted fp32 product is infinite (primitive_inputs' docstring)
            reach = finite if j == 0 else finite & (v.abs() < pi.W_LO_OVERFLOW)
            assert not bool(torch.isnan(got[reach]).any()), f"{names[j]}: NaN byte for a finite input in saturating mode"
            if j:
                _note(f"E4M3_F32 {names[j]}: Inf product", mode, f"{int((torch.isnan(got) & finite).sum())} finite inputs pack as NaN "
                      f"(am.e4m3: 448), the smallest |v| = {float(v[torch.isnan(got) & finite].abs().min()):.3e}")
    if mode == 1:  # the expectations ARE the model's functions with the model's shifts
        x = v.double()
        own = (am.e4m3(x), am.e4m3(x, am.W_SHIFT), am.e4m3(x - pi.to_f16(x, 1), am.LO_SHIFT + am.W_SHIFT))
        reach = finite & (v.abs() < pi.W_LO_OVERFLOW)
        assert int((finite & ~reach).sum()) > 0 and pi.W_LO_OVERFLOW >= 2.0**100
        for j in range(3):
            assert not bool(pi.mismatches(pi.expect_e4m3_f32(v, 1)[j][reach], own[j][reach]).any())
    assert not fails, "\n".join(fails)


# -- the scaled e4m3 MFMA -------------------------------------------------------------------------------------------------------------
def _e4m3_byte(x: torch.Tensor, shift: int) -> torch.Tensor:
    return (x.to(torch.float32) * 2.0**shift).clamp(-448.0, 448.0).to(F8).view(torch.uint8)


def test_mfma_block_scales(enc):
    # form 1: bytes given; every element of every tile is 128 a b 2^-18
    raw = torch.tensor([0x00, 0x80, 0x01, 0x81, 0x07, 0x08, 0x38, 0xB8, 0x3C, 0x4B, 0x7E, 0xFE], dtype=torch.uint8)
    a, b = torch.meshgrid(raw, raw, indexing="ij")
    pairs = torch.stack([a.flatten(), b.flatten()], 1).contiguous()
    tiles = enc.debug_primitive("MFMA_SCALE", 1, pairs.view(-1)).view(-1, 4, 256).double()
    want = 128.0 * pairs[:, 0].view(F8).double() * pairs[:, 1].view(F8).double() * 2.0 ** -(am.LO_SHIFT + am.W_SHIFT)
    off = tiles != want[:, None, None]
    _note("MFMA_SCALE bytes a, b", 1, f"{tiles.numel()} elements of {len(pairs)} (a, b) x 4 products, {int(off.sum())} off 128 a b 2^-18")
    assert not bool(off.any()), f"pairs off: {pairs[off.any(dim=2).any(dim=1)][:8].tolist()}"
    # form 2: planes of different magnitude, encoded and decoded as the model does
    gen = torch.Generator().manual_seed(5)
    n = 256
    sign = lambda: torch.randint(0, 2, (n,), generator=gen).double() * 2 - 1  # noqa: E731
    x_lo = sign() * torch.exp2(torch.rand(n, generator=gen).double() * 9 - 21)  # an activation's remainder: up to 2^-12
    w = sign() * torch.exp2(torch.rand(n, generator=gen).double() * 9 - 8)  # a weight: 2^-8 .. 2
    act = sign() * torch.exp2(torch.rand(n, generator=gen).double() * 8 - 4)  # an activation: 2^-4 .. 16
    w_lo = sign() * torch.exp2(torch.rand(n, generator=gen).double() * 9 - 25)  # a weight's remainder
    for label, left, lshift, right, rshift, which in (("lo(x) x e4m3(w)", x_lo, am.LO_SHIFT, w, am.W_SHIFT, (0, 1)),
                                                      ("e4m3(x) x lo(w)", act, 0, w_lo, am.LO_SHIFT + am.W_SHIFT, (2, 3))):
        pairs = torch.stack([_e4m3_byte(left, lshift), _e4m3_byte(right, rshift)], 1).contiguous()
        tiles = enc.debug_primitive("MFMA_SCALE", 1, pairs.view(-1)).view(-1, 4, 256).double()[:, list(which)]
        want = 128.0 * am.e4m3(left, lshift) * am.e4m3(right, rshift)
        assert float(want.abs().min()) > 0
        off = tiles != want[:, None, None]
        _note(f"MFMA_SCALE {label}", 1, f"{tiles.numel()} elements, {int(off.sum())} off the model's decode")
        assert not bool(off.any()), label


# -- fp32 functions ---------------------------------------------------------------------------------------------------------------------
def test_gelu(enc):
    x = pi.function_sweep()
    rec = enc.debug_primitive("GELU", 0, x)
    assert torch.equal(rec[:, 0].view(torch.int32), rec[:, 1].view(torch.int32)), "gelu_erf and the staged form differ in some bit"
    assert torch.equal(rec.view(torch.int32), enc.debug_primitive("GELU", 1, x).view(torch.int32))
    g = rec[:, 0]
    xn = x.numpy()
    finite = np.isfinite(xn)
    exact = pi.gelu_exact(xn[finite])
    dev_err = np.abs(g.numpy()[finite].astype(np.float64) - exact)
    emu_err = np.abs(pi.gelu_emulated(xn[finite]).astype(np.float64) - exact)
    at = xn[finite][int(dev_err.argmax())]
    lin = np.zeros_like(finite)
    lin[pi.linear_part()] = True
    lin_dev, lin_emu = dev_err[lin[finite]].max(), emu_err[lin[finite]].max()
    grid = np.zeros_like(finite)
    grid[:65536] = True
    _note("GELU two forms", None, "bit-identical on every input, NaNs included")
    _note("GELU vs float64 erfc", None, f"{int(finite.sum())} finite inputs: device max {dev_err.max():.3e} at x = {float(at):.5f} (emulation "
          f"{emu_err.max():.3e}); [-12, 12] grid {lin_dev:.3e} (emulation {lin_emu:.3e}); fp16 grid {dev_err[grid[finite]].max():.3e} "
          f"(emulation {emu_err[grid[finite]].max():.3e})")
    tail, tail_at, tail_n = pi.gelu_tail_ratio(xn, g.numpy(), pi.gelu_emulated(xn))
    _note("GELU vs the emulation, x < 0", None, f"{tail_n} inputs with |gelu| >= 2^-120: worst |device - emulation| / (2^-21 |emulation|) = "
          f"{tail:.3f} at x = {tail_at:.5f}")
    assert dev_err.max() <= pi.GELU_MARGIN * emu_err.max(), (dev_err.max(), emu_err.max(), at)
    assert tail <= 1.0, (tail, tail_at)  # (primitive_inputs.GELU_TAIL_REL: the device evaluates THIS polynomial, to v_exp_f32's error)
    assert dev_err.max() < pi.GELU_FLOOR, (dev_err.max(), at)
    # exact ends: gelu(+-0) = 0; gelu(x) == x from 13 on; zero from -13 down (q(13) ~ -182: 2^q is below fp32's range)
    assert bool((g[x == 0] == 0).all())
    up, down = (x >= 13.0) & torch.isfinite(x), (x <= -13.0) & torch.isfinite(x)
    assert int(up.sum()) > 1000 and int(down.sum()) > 1000
    assert torch.equal(g[up].view(torch.int32), x[up].view(torch.int32)) and bool((g[down] == 0).all())
    assert float(pi.gelu_emulated(np.float32([13.0]))[0]) == 13.0
    # non-finite in, non-finite out (the fp16 range guard's "loud NaN" goes through here)
    assert int((~torch.isfinite(x)).sum()) > 2000 and not bool(torch.isfinite(g[~torch.isfinite(x)]).any())


def test_exp2_and_expf(enc):
    x = pi.function_sweep()
    rec = enc.debug_primitive("EXP2", 0, x)
    e2, ex = rec[:, 0], rec[:, 1]
    for special in (pi.MASK_VALUE, -math.inf):
        at = x == float(np.float32(special))
        assert int(at.sum()) >= 1 and bool((e2[at].view(torch.int32) == 0).all()), f"exp2({special}) is not +0"
    assert float(e2[x <= 6.0].max()) <= 64.0
    order = torch.argsort(x[torch.isfinite(x)])
    ordered = e2[torch.isfinite(x)][order]
    assert bool((ordered[1:] >= ordered[:-1]).all()), "exp2 is not non-decreasing"
    xd = x.double()
    inside = (xd >= -160.0) & (xd <= 6.0)
    exact = torch.exp2(xd)
    normal = inside & (exact >= 2.0**-126)
    rel = ((e2.double() - exact).abs() / exact)[normal]
    below = (e2.double() - exact).abs()[inside & ~normal]
    _note("EXP2 v_exp_f32 on [-160, 6]", None, f"{int(normal.sum())} results >= 2^-126: max relative error {float(rel.max()):.3e} "
          f"(bound 2^-22 = {2.0**-22:.3e}); {int(below.numel())} below: max absolute error {float(below.max()):.3e}, "
          f"{int((e2[inside & ~normal] == 0).sum())} of them zero")
    assert float(rel.max()) < 2.0**-22
    neg = (xd >= -100.0) & (xd <= 0.0)
    err = (ex.double() - torch.exp(xd)).abs()[neg]
    _note("EXP2 __expf on [-100, 0]", None, f"{int(neg.sum())} inputs: max absolute error {float(err.max()):.3e} (bound 1e-6)")
    assert float(err.max()) < 1e-6


def test_keep_probability(enc):
    l = pi.keep_prob_inputs()
    got = enc.debug_primitive("KEEP_PROB", 0, l.reshape(-1)).view(-1).double()
    d = l[:, 0].double() - l[:, 1].double()
    exact = 1.0 / (1.0 + torch.exp(d))
    ok = ~torch.isnan(d)
    err = (got - exact).abs()[ok]
    _note("KEEP_PROB", None, f"{int(ok.sum())} logit pairs, differences over [-120, 120] and +-Inf: max |device - float64| "
          f"{float(err.max()):.3e} = {float(err.max()) / KEEP_PROB_BOUND:.3f} x the bound 8 x 2^-24")
    assert float(err.max()) <= KEEP_PROB_BOUND
    assert int((d > 89.0).sum()) > 1000 and bool((got[d > 89.0] == 0).all())  # expf overflows to Inf: exactly 0
    assert bool((got[d == math.inf] == 0).all()) and bool((got[d == -math.inf] == 1).all())
    assert int((~ok).sum()) >= 4 and bool(torch.isnan(got[~ok]).all())


def test_rope(enc):
    t = pi.rope_inputs()
    got = enc.debug_primitive("ROPE", 0, t.reshape(-1)).double()
    x1, x2, c, s = (t[:, j].double() for j in range(4))
    bound = 2.0**-23 * ((x1 * c).abs() + (x2 * s).abs())
    bound_hi = 2.0**-23 * ((x2 * c).abs() + (x1 * s).abs())
    r_lo = ((got[:, 0] - (x1 * c - x2 * s)).abs() / bound).max()
    r_hi = ((got[:, 1] - (x2 * c + x1 * s)).abs() / bound_hi).max()
    _note("ROPE rope_lo / rope_hi", None, f"{len(t)} (x1, x2, cos, sin): worst |device - float64| / (2^-23 (|x1 c| + |x2 s|)) = "
          f"{float(r_lo):.3f} / {float(r_hi):.3f}")
    assert float(r_lo) <= 1.0 and float(r_hi) <= 1.0
