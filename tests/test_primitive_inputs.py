"""The inputs of tests/test_gpu_primitives.py, on the CPU: the sweep holds every class of input it promises, and the
expected values that module compares the device with would move under each mistake it is there for.

  * classes: all fp16 / bf16 bit patterns, ties per format, subnormal results, saturating inputs, inputs whose lo plane is exactly
    zero, -0, Inf, NaN, fp32 subnormals -- each counted, each non-empty;
  * the restated formats (``primitive_inputs.quantize``) agree with ``am.rne`` / ``am.e4m3`` on the whole sweep: the mutations
    below differ from the model's functions by the mutation alone;
  * every mutation of ``primitive_inputs.MUTATIONS`` changes the expected value of at least 16 elements (the count is printed):
    a mutation the sweep cannot tell from the truth would be a hole in the inputs;
  * GELU: every coefficient moved in its 5th significant digit, and the polynomial applied to x instead of |x|, push the
    fp32 emulation's maximum error against float64 erfc over the bound tests/test_gpu_primitives.py applies to the device --
    1.25 x the unmutated emulation's maximum on the same inputs, or the 1e-6 floor.

The absolute bounds alone do not see every coefficient: one unit of the 5th significant digit of the three leading ones (of
|x|^5, |x|^4, |x|^3) moves the emulation's maximum error to 6.373e-7 / 6.397e-7, 6.366e-7 / 6.402e-7 and 7.172e-7 / 7.915e-7
(+ / -), 0.80 - 0.99 x the 7.986e-7 that 1.25 x the emulation's 6.389e-7 allows -- such a move changes gelu by at most 3e-9 / 2e-8
/ 1.5e-7, inside the 25 % margin -- while coefficients 3 - 5 reach 2.3 - 15 x.  The device test therefore also holds the negative
side to the emulation RELATIVELY (``primitive_inputs.GELU_TAIL_REL`` = 2^-21, derived there from v_exp_f32's bound and three
roundings): there he's relative change ln 2 |x|^(5-k) delta is not hidden under max(x, 0), and every mutation is far over it.  Each
case prints both ratios and must exceed at least one of the bounds the device is held to."""

from __future__ import annotations

import numpy as np
import pytest
import torch

import arith_model as am
import primitive_inputs as pi

MIN_DISTINGUISHED = 16
BF16, F16, F8 = pi.BF16, pi.F16, pi.F8


def _finite():
    v = pi.sweep()
    return v, torch.isfinite(v)


def _count(label: str, n: int, at_least: int = 1) -> int:
    print(f"[primitive inputs] {label:58s} {n:9d}")
    assert n >= at_least, label
    return n


# 1. the classes --------------------------------------------------------------------------------------------------------------
def test_sweep_holds_every_bit_pattern_and_special():
    v = pi.sweep()
    assert v.dtype == torch.float32 and v.numel() % 4 == 0 and 1_400_000 <= v.numel() <= 1_600_000
    pi.sweep.cache_clear()
    assert torch.equal(v.view(torch.int32), pi.sweep().view(torch.int32))  # deterministic, bit for bit
    bits = set((v.view(torch.int32).numpy().astype(np.int64) & 0xFFFFFFFF).tolist())
    f16 = pi.fp16_grid()
    assert len(f16) == 65536 and set((f16.view(np.uint32).astype(np.int64)).tolist()) <= bits
    assert all((b << 16) in bits for b in range(65536))  # every bf16 pattern
    _count("NaN inputs", int(torch.isnan(v).sum()), 2000)
    _count("+-Inf inputs", int(torch.isinf(v).sum()), 4)
    _count("-0 inputs", int(((v == 0) & torch.signbit(v)).sum()), 2)
    _count("fp32-subnormal inputs", int(pi.is_f32_subnormal(v).sum()), 200)
    for edge in (65504.0, 65519.99609375, 65520.0, 65536.0, 1e5, 2.0**-14, 2.0**-24, 2.0**-25, float(np.nextafter(np.float32(2.0**-25), np.float32(1)))):
        for s in (1.0, -1.0):
            assert bool((v == np.float32(s * edge).item()).any()), edge


def test_ties_per_format():
    v, finite = _finite()
    x = v.double()
    tie_bf16 = finite & ((v.view(torch.int32) & 0xFFFF) == 0x8000)
    _count("bf16 ties (hi)", int(tie_bf16.sum()), 16000)
    h = pi.quantize(x, F16, "trunc")
    up = pi.quantize(x, F16, "away")
    tie_f16 = finite & (x.abs() <= 65520.0) & (x != h) & ((x - h).abs() * 2 == (up - h).abs()) & (up != h)
    _count("fp16 ties (hi), subnormal and 65520 included", int(tie_f16.sum()), 60000)
    assert bool(tie_f16[v == 65520.0].all()) and bool(tie_f16[v == np.float32(2.0**-25).item()].all())
    # each tie comes with both fp32 neighbours
    allbits = set(v.view(torch.int32).tolist())
    for t in v[tie_f16][:: max(int(tie_f16.sum()) // 500, 1)].view(torch.int32).tolist():
        assert t - 1 in allbits and t + 1 in allbits
    # e4m3 ties of the three e4m3 planes: the activation's lo plane, the weight plane, the weight's lo plane
    hi = pi.to_f16(x, 1)
    for label, val, shift in (("activation lo plane (x 2^12)", x - hi, pi.LO_SHIFT), ("weight plane (x 2^6)", x, pi.W_SHIFT),
                              ("weight lo plane (x 2^18)", x - hi, pi.LO_SHIFT + pi.W_SHIFT)):
        s = (val * 2.0**shift)
        lo, aw = pi.quantize(s, F8, "trunc"), pi.quantize(s, F8, "away")
        tie = finite & (s.abs() <= 464.0) & (s != lo) & ((s - lo).abs() * 2 == (aw - lo).abs())
        _count(f"e4m3 ties, {label}", int(tie.sum()), 200)
        _count(f"  ... of them to zero (|scaled| = 2^-10)", int((tie & (s.abs() == 2.0**-10)).sum()), 2)
        _count(f"  ... and at 464 (the tie to the first value out of range)", int((tie & (s.abs() == 464.0)).sum()), 2)


def test_subnormal_saturating_and_zero_lo_classes():
    v, finite = _finite()
    x = v.double()
    for mode in (0, 1):
        hi, lo = pi.expect_f16_f8(v, mode)
        _count(f"mode {mode}: fp16 subnormal hi", int((finite & (hi != 0) & (hi.abs() < 2.0**-14)).sum()), 2000)
        s = lo * 2.0**pi.LO_SHIFT
        _count(f"mode {mode}: e4m3 subnormal lo", int((finite & (s != 0) & (s.abs() < 2.0**-6)).sum()), 1000)
        _count(f"mode {mode}: lo plane exactly zero", int((finite & torch.isfinite(hi) & (lo == 0)).sum()), 60000)
        big = finite & torch.isfinite(hi) & (((x - hi) * 2.0**pi.LO_SHIFT).abs() > 448.0)
        _count(f"mode {mode}: lo plane beyond +-448", int(big.sum()), 10000)
        assert bool(torch.isnan(lo[big & (((x - hi) * 2.0**pi.LO_SHIFT).abs() > 464.0)]).all()) == (mode == 0)
        if mode == 1:
            assert bool((s[big].abs() == 448.0).all())
            _count("mode 1: |v| in [256, 65504] with a saturated lo plane", int((big & (x.abs() >= 256) & (x.abs() <= 65504)).sum()), 10000)
            _count("mode 1: hi clamped to +-65504", int((finite & (x.abs() >= 65520.0) & (hi.abs() == 65504.0)).sum()), 1000)
        else:
            _count("mode 0: hi overflows to Inf", int((finite & torch.isinf(hi)).sum()), 1000)
    _, w, wlo = pi.expect_e4m3_f32(v, 1)
    _count("weight plane at +-448 (|w| >= 7)", int((finite & (w.abs() * 2.0**pi.W_SHIFT == 448.0)).sum()), 1000)
    sw = w * 2.0**pi.W_SHIFT
    _count("weight plane subnormal (|w| < 2^-12)", int((finite & (sw != 0) & (sw.abs() < 2.0**-6)).sum()), 1000)
    _count("weight 2^-16 (the tie to zero after x 2^6)", int((v.abs() == 2.0**-16).sum()), 2)
    _count("weight 2^-15 (e4m3's smallest subnormal after x 2^6)", int((v.abs() == 2.0**-15).sum()), 2)
    _count("weight lo plane at +-448", int((finite & (v.abs() < pi.W_LO_OVERFLOW) & (wlo.abs() * 2.0 ** (pi.LO_SHIFT + pi.W_SHIFT) == 448.0)).sum()), 200)
    _count("weights whose shifted lo part overflows fp32 (packed as NaN)", int((finite & torch.isnan(wlo)).sum()), 16)
    sat_bf16 = finite & torch.isinf(am.rne(x, BF16))
    _count("finite inputs beyond bf16's range", int(sat_bf16.sum()), 4)


def test_plane_edges_land_on_the_points_they_aim_at():
    """hi + t 2^-shift with hi = 1.5 x 2^e: fp16(v) is hi and the lo plane is exactly the e4m3 point t."""

    for shift in (pi.LO_SHIFT, pi.LO_SHIFT + pi.W_SHIFT):
        t, v = pi.plane_edge_centres(shift)
        v = torch.from_numpy(v)
        hi = am.rne(v.double(), F16)
        assert bool((((v.double() - hi) * 2.0**shift) == torch.from_numpy(t)).all())
        assert bool((((hi.abs().log2() % 1) - 0.5849625).abs() < 1e-6).all())  # 1.5 x 2^e
        assert {448.0, 464.0, 480.0, 2.0**-9, 2.0**-10, 1.5 * 2.0**-9, -448.0, -(2.0**-10)}.issubset(set(t.tolist()))
        assert set(v.view(torch.int32).tolist()) <= set(pi.sweep().view(torch.int32).tolist())


# 2. the restated formats are the model's ------------------------------------------------------------------------------------------
def test_restated_formats_agree_with_the_model():
    v, finite = _finite()
    x = v.double()
    for dtype in (BF16, F16):
        own = pi.quantize(x, dtype)
        own = torch.where(own.abs() > pi.FORMATS[dtype][2], torch.sign(own) * float("inf"), own)
        assert not bool(pi.mismatches(am.rne(x, dtype)[finite], own[finite]).any()), dtype
    for shift in (0, pi.W_SHIFT, pi.LO_SHIFT):
        ok = finite & torch.isfinite((v * 2.0**shift))
        own = pi.quantize((v * 2.0**shift).double(), F8).clamp(-448.0, 448.0) / 2.0**shift
        assert not bool(pi.mismatches(am.e4m3(x, shift)[ok], own[ok]).any()), shift
    # and the unmutated expectations are built from am.rne / am.e4m3 alone
    hi = am.rne(x, F16)
    reach = finite & (x.abs() < 65520.0)
    e_hi, e_lo = pi.expect_f16_f8(v, 1)
    assert not bool(pi.mismatches(e_hi[reach], hi[reach]).any())
    assert not bool(pi.mismatches(e_lo[reach], am.e4m3(x - hi, am.LO_SHIFT)[reach]).any())


# 3. mutations ---------------------------------------------------------------------------------------------------------------------
def _expected(v, mode, rules):
    return (*pi.expect_bf16_split(v, rules, mode), *pi.expect_f16_pair(v, mode, rules)[:2], *pi.expect_f16_f8(v, mode, rules),
            pi.expect_e4m3_f16(torch.from_numpy(pi.fp16_grid()), mode, rules), *pi.expect_e4m3_f32(v, mode, rules))


RECORDS = ("bf16 hi", "bf16 lo", "f16 hi", "f16 lo", "f16+f8 hi", "f16+f8 lo", "e4m3(fp16)", "e4m3(fp32)", "weight plane", "weight lo plane")
# the records a mutation must show in (it may show in more)
MUST_SHOW = {
    "bf16 / fp16 round half away": ("bf16 hi", "bf16 lo", "f16 hi", "f16 lo", "f16+f8 hi"),
    "e4m3 round half away": ("f16+f8 lo", "e4m3(fp16)", "e4m3(fp32)", "weight plane", "weight lo plane"),
    "bf16 / fp16 truncation": ("bf16 hi", "bf16 lo", "f16 hi", "f16 lo", "f16+f8 hi"),
    "e4m3 truncation": ("f16+f8 lo", "e4m3(fp16)", "e4m3(fp32)", "weight plane", "weight lo plane"),
    "lo from the unrounded value (lo = 0)": ("bf16 lo", "f16 lo", "f16+f8 lo"),
    "lo decoded at 2^11": ("f16+f8 lo",),
    "e4m3 without the clamp": ("f16+f8 lo", "e4m3(fp16)", "e4m3(fp32)", "weight plane", "weight lo plane"),
    "e4m3 subnormals flushed": ("f16+f8 lo", "e4m3(fp16)", "e4m3(fp32)", "weight plane", "weight lo plane"),
    "fp16 subnormals flushed": ("f16 hi", "f16 lo", "f16+f8 hi", "f16+f8 lo"),
    "weight shift 2^5": ("weight plane", "weight lo plane"),
    "modes swapped": ("f16 hi", "f16+f8 hi", "f16+f8 lo", "e4m3(fp16)", "e4m3(fp32)", "weight plane", "weight lo plane"),
}


@pytest.fixture(scope="module")
def plain():
    v = pi.sweep()
    return {mode: _expected(v, mode, pi.PLAIN) for mode in (0, 1)}


@pytest.mark.parametrize("name", list(pi.MUTATIONS))
def test_mutation_changes_the_expected_values(plain, name):
    assert set(MUST_SHOW) == set(pi.MUTATIONS)
    v, finite = _finite()
    rules = pi.MUTATIONS[name]
    # "without the clamp" is a statement about saturating mode only; every other mutation must show in the mode it is run in
    modes = (1,) if name == "e4m3 without the clamp" else (0, 1)
    counts = {}
    for mode in modes:
        for rec, a, b in zip(RECORDS, plain[mode], _expected(v, mode, rules)):
            where = finite if a.numel() == v.numel() else torch.ones_like(a, dtype=torch.bool)
            counts[rec] = max(counts.get(rec, 0), int((pi.mismatches(a, b) & where).sum()))
    print(f"[primitive inputs] mutation {name:38s} " + "  ".join(f"{rec}: {n}" for rec, n in counts.items() if n))
    for rec in MUST_SHOW[name]:
        assert counts[rec] >= MIN_DISTINGUISHED, (name, rec, counts[rec])


# 4. GELU ----------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def gelu_reference():
    x = pi.function_sweep().numpy()
    x = x[np.isfinite(x)]
    exact = pi.gelu_exact(x)
    own = float(np.abs(pi.gelu_emulated(x).astype(np.float64) - exact).max())
    return x, exact, own


def test_gelu_emulation_and_its_bound(gelu_reference):
    x, exact, own = gelu_reference
    lin = np.linspace(-12.0, 12.0, pi.LINEAR_POINTS).astype(np.float32)
    e_lin = np.abs(pi.gelu_emulated(lin).astype(np.float64) - pi.gelu_exact(lin))
    grid = pi.fp16_grid()
    grid = grid[np.isfinite(grid)]
    e_grid = np.abs(pi.gelu_emulated(grid).astype(np.float64) - pi.gelu_exact(grid))
    print(f"[primitive inputs] GELU emulation: max |gelu - exact| {own:.4e} over {len(x)} finite inputs; [-12, 12] grid {e_lin.max():.4e} at "
          f"x = {float(lin[e_lin.argmax()]):.5f}; fp16 grid {e_grid.max():.4e} at x = {float(grid[e_grid.argmax()]):.5f}")
    assert 6.3e-7 < e_lin.max() < 6.5e-7 and 6.0e-7 < e_grid.max() < 6.3e-7  # the figures of opk_common.hip.h's comment
    assert own * pi.GELU_MARGIN < pi.GELU_FLOOR  # the two bounds of the device test are consistent: (a) implies (b)
    # the ends the device test asserts exactly
    assert bool((pi.gelu_emulated(np.float32([0.0, -0.0])) == 0).all())
    far = np.float32([13.0, 20.0, 1e4, 3e38])
    assert bool((pi.gelu_emulated(far) == far).all()) and bool((pi.gelu_emulated(-far) == 0).all())
    assert bool(np.isnan(pi.gelu_emulated(np.float32([np.inf, -np.inf, np.nan]))).all())
    # q is decreasing and below fp32's exponent range from 13 on
    a = np.linspace(0.0, 200.0, 2_000_001)
    q = np.polyval(pi.GELU_COEFFS, a)
    assert bool((np.diff(q) < 0).all()) and q[a >= 13.0].max() < -150.0


GELU_MUTATIONS = {f"coefficient {k} {'+' if s > 0 else '-'} 1 in its 5th digit": dict(coeffs=pi.perturbed_coeffs(k, s))
                  for k in range(6) for s in (1.0, -1.0)}
GELU_MUTATIONS["he applied to x instead of |x|"] = dict(he_on_x=True)


@pytest.mark.parametrize("name", list(GELU_MUTATIONS))
def test_gelu_mutation_breaks_the_bound(gelu_reference, name):
    x, exact, own = gelu_reference
    mutated = pi.gelu_emulated(x, **GELU_MUTATIONS[name])
    err = float(np.nanmax(np.abs(mutated.astype(np.float64) - exact)))
    bound = min(pi.GELU_MARGIN * own, pi.GELU_FLOOR)
    tail, tail_at, _ = pi.gelu_tail_ratio(x, mutated, pi.gelu_emulated(x))
    print(f"[primitive inputs] GELU mutation {name:40s} max error {err:.3e} = {err / bound:6.2f} x the absolute bound {bound:.3e}; "
          f"x < 0 against the emulation: {tail:10.3g} x the relative bound, at x = {tail_at:.4f}")
    assert err > bound or tail > 1.0


def test_gelu_tail_bound_is_not_vacuous(gelu_reference):
    """The unmutated emulation sits at 0 of the relative bound by construction; what the bound must allow is the device's
    v_exp_f32: an emulation whose exp2 is off by 2^-22 relative (the instruction's asserted bound) stays inside, one whose exp2 is
    off by 2^-20 does not."""

    x, _, _ = gelu_reference
    emu = pi.gelu_emulated(x).astype(np.float64)
    n = pi.gelu_tail_ratio(x, emu, emu)[2]
    assert n > 1_900_000  # the polynomial underflows (he flushed) from |x| ~ 11.6 on
    assert pi.gelu_tail_ratio(x, (emu * (1 + 2.0**-22)).astype(np.float32), emu)[0] <= 1.0
    assert pi.gelu_tail_ratio(x, (emu * (1 + 2.0**-20)).astype(np.float32), emu)[0] > 1.0


# 5. the other function sweeps -------------------------------------------------------------------------------------------------------
def test_function_sweeps_hold_their_specials():
    x = pi.function_sweep()
    assert x.numel() > 4_000_000
    for special in (0.0, pi.MASK_VALUE, float("inf"), float("-inf"), 6.0, -160.0, 13.0, -13.0):
        assert bool((x == np.float32(special).item()).any()), special
    assert bool(((x == 0) & torch.signbit(x)).any()) and bool(torch.isnan(x).any())
    assert float(x[torch.isfinite(x)].abs().max()) >= 2.9e38
    l = pi.keep_prob_inputs()
    d = l[:, 0].double() - l[:, 1].double()
    assert float(d[torch.isfinite(d)].min()) <= -120 and float(d[torch.isfinite(d)].max()) >= 120
    assert bool((d == float("inf")).any()) and bool((d == float("-inf")).any()) and int(torch.isnan(d).sum()) >= 4
    near = (l.abs().min(dim=1).values > 9000) & (d.abs() <= 8)
    assert int(near.sum()) > 60000  # logits of magnitude 1e4 with small differences
    r = pi.rope_inputs()
    assert r.shape[1] == 4 and bool(torch.isfinite(r).all())
    assert float((r[:, 2] ** 2 + r[:, 3] ** 2 - 1).abs().max()) < 1e-6
