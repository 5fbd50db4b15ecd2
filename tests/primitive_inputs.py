"""Inputs and expected values of tests/test_gpu_primitives.py (test infrastructure, no GPU): the sweeps the device primitives
of ``op_debug_primitive`` are run over, what ``tests/arith_model.py``'s operand roundings (``am.rne`` / ``am.e4m3``) make of
every element, and an fp32 emulation of the GELU polynomial.  ``tests/test_primitive_inputs.py`` holds this module to its
promises: every class of input is there, and every mutation of :class:`Rules` changes the expected values on the sweep.

The expected-value functions take a :class:`Rules`; the default one calls ``am.rne`` / ``am.e4m3`` themselves (the test pins the
MODEL's functions to the hardware), a mutated one goes through :func:`quantize`, an independent restatement of the formats.

Conversion modes (``opk_common.hip.h`` set_overflowing_conversions / set_saturating_conversions, MODE.FP16_OVFL):
  0  a finite value beyond the format's range becomes Inf (fp16, from |v| >= 65520) or NaN (e4m3, beyond 464: e4m3 has no Inf);
  1  it becomes the largest finite value, +-65504 / +-448 (``am.e4m3``'s clamp); an infinite input stays infinite (fp16).
Two things the device does that ``am.rne`` / ``am.e4m3`` do not, both measured by tests/test_gpu_primitives.py on inputs no forward
reaches, restated here so that they are asserted as observed (and listed under "Not modelled" in tests/arith_model.py):
  * mode 1 clamps a bf16 overflow too: v_cvt_pk_bf16_f32 of a finite |v| >= 0x7f7f8000 (3.396e38) gives +-max bf16, not Inf;
  * v_cvt_pk_fp8_f32 (f2e4m3: the weight planes) gives NaN for an INFINITE input in either mode, so a weight whose shifted
    fp32 product overflows (|w| >= 2^122; |w - fp16(w)| x 2^18: |w| >= 2^110) packs as NaN where ``am.e4m3`` clamps to 448.
    The scaled conversions (v_cvt_scalef32_pk_fp8_f16: f16x4_to_e4m3) clamp an infinite input to +-448, as ``am.e4m3`` does.
"""

from __future__ import annotations

import functools
import math
from dataclasses import dataclass

import numpy as np
import torch

import arith_model as am

BF16, F16, F8 = torch.bfloat16, torch.float16, am.F8
LO_SHIFT, W_SHIFT = am.LO_SHIFT, am.W_SHIFT
FORMATS = {BF16: (7, -126, float(torch.finfo(BF16).max)), F16: (10, -14, 65504.0), F8: (3, -6, 448.0)}  # mantissa bits, emin, max
F32_MIN_NORMAL = 2.0**-126


# -- the formats, restated (mutations; the unmutated path is am.rne / am.e4m3) -------------------------------------------------
def quantize(x: torch.Tensor, dtype: torch.dtype, how: str = "rne") -> torch.Tensor:
    """float64 ``x`` on the grid of ``dtype`` (gradual underflow, NO overflow handling: the result may exceed the format's
    maximum), rounding ``how``: "rne", "away" (round half away from zero) or "trunc"."""

    mant, emin, _ = FORMATS[dtype]
    x = x.to(torch.float64)
    _, e = torch.frexp(x)  # |x| in [2^(e - 1), 2^e)
    ulp = torch.ldexp(torch.ones_like(x), (e - 1).clamp(min=emin) - mant)
    q = x / ulp
    if how == "rne":
        r = torch.round(q)
    elif how == "away":
        r = torch.sign(q) * torch.floor(q.abs() + 0.5)
    elif how == "trunc":
        r = torch.trunc(q)
    else:
        raise ValueError(how)
    out = r * ulp
    return torch.where(torch.isfinite(x), out, x)


@dataclass(frozen=True)
class Rules:
    """What the expected values assume; every field but the defaults is a mutation (tests/test_primitive_inputs.py)."""

    round16: str = "rne"  # bf16 / fp16 rounding
    round8: str = "rne"  # e4m3 rounding
    lo_zero: bool = False  # the lo plane computed from the unrounded value: v - v = 0
    lo_decode: int = LO_SHIFT  # the shift an activation's e4m3 lo plane is decoded with
    e4m3_clamp: bool = True  # saturating mode clamps e4m3 (False: NaN beyond the range, as mode 0)
    e4m3_flush: bool = False  # e4m3 subnormals flushed to zero
    f16_flush: bool = False  # fp16 subnormals flushed to zero
    w_shift: int = W_SHIFT  # the shift a weight's e4m3 plane is ENCODED with (decoded with W_SHIFT)
    swap_modes: bool = False  # mode 0 saturates, mode 1 overflows


PLAIN = Rules()
MUTATIONS = {
    "bf16 / fp16 round half away": Rules(round16="away"),
    "e4m3 round half away": Rules(round8="away"),
    "bf16 / fp16 truncation": Rules(round16="trunc"),
    "e4m3 truncation": Rules(round8="trunc"),
    "lo from the unrounded value (lo = 0)": Rules(lo_zero=True),
    "lo decoded at 2^11": Rules(lo_decode=LO_SHIFT - 1),
    "e4m3 without the clamp": Rules(e4m3_clamp=False),
    "e4m3 subnormals flushed": Rules(e4m3_flush=True),
    "fp16 subnormals flushed": Rules(f16_flush=True),
    "weight shift 2^5": Rules(w_shift=W_SHIFT - 1),
    "modes swapped": Rules(swap_modes=True),
}


def _saturating(mode: int, rules: Rules) -> bool:
    return (mode == 1) != rules.swap_modes


def to_bf16(x: torch.Tensor, rules: Rules = PLAIN, mode: int = 0) -> torch.Tensor:
    """bf16 of the fp32 value ``x`` holds (float64 in, float64 out); a finite value beyond bf16's range: Inf in mode 0, the
    largest bf16 value in mode 1 (module docstring)."""

    x = x.to(torch.float32).to(torch.float64)
    if rules.round16 == "rne":
        y = am.rne(x, BF16)
    else:
        y = quantize(x, BF16, rules.round16)
        y = torch.where(y.abs() > FORMATS[BF16][2], torch.sign(y) * math.inf, y)
    if _saturating(mode, rules):
        y = torch.where(torch.isinf(y) & torch.isfinite(x), torch.sign(x) * FORMATS[BF16][2], y)
    return y


def to_f16(x: torch.Tensor, mode: int, rules: Rules = PLAIN) -> torch.Tensor:
    """fp16 of the fp32 value ``x`` holds under conversion mode ``mode``."""

    x = x.to(torch.float32).to(torch.float64)
    sat = _saturating(mode, rules)
    if rules.round16 == "rne":
        y = am.rne(torch.where(torch.isinf(x), x, x.clamp(-65504.0, 65504.0)) if sat else x, F16)
    else:
        y = quantize(x, F16, rules.round16)
        y = torch.where(y.abs() > 65504.0, torch.sign(y) * (65504.0 if sat else math.inf), y)
        y = torch.where(torch.isinf(x), x, y)
    if rules.f16_flush:
        y = torch.where(y.abs() < 2.0**-14, y * 0.0, y)
    return y


def to_e4m3(x: torch.Tensor, shift: int, mode: int, rules: Rules = PLAIN, decode: "int | None" = None,
            inf_is_nan: bool = False) -> torch.Tensor:
    """e4m3(x * 2^shift) / 2^decode under conversion mode ``mode`` (``decode`` defaults to ``shift``); NaN where the
    conversion gives NaN.  ``inf_is_nan``: the unscaled conversion of f2e4m3, NaN where the fp32 product x * 2^shift is infinite."""

    sat = _saturating(mode, rules) and rules.e4m3_clamp
    scaled = x.to(torch.float32) * 2.0**shift
    if rules.round8 == "rne":
        y = am.e4m3(x, shift, 0) if sat else scaled.to(F8).to(torch.float64)
    else:
        y = quantize(scaled.to(torch.float64), F8, rules.round8)
        over = y.abs() > 448.0
        y = torch.where(over, torch.sign(y) * 448.0 if sat else y * math.nan, y)
    if rules.e4m3_flush:
        y = torch.where(y.abs() < 2.0**-6, y * 0.0, y)
    if inf_is_nan:
        y = torch.where(torch.isinf(scaled), scaled.to(torch.float64) * math.nan, y)
    return y / 2.0 ** (shift if decode is None else decode)


# -- expected records (float64 VALUES; the device's bits are decoded and compared as values, NaN positions exactly) -------------
def expect_bf16_split(v: torch.Tensor, rules: Rules = PLAIN, mode: int = 0):
    """(hi, lo) of split2 / split2_pk / split4: hi = RNE_bf16(v), lo = RNE_bf16(v - hi)."""

    x = v.to(torch.float64)
    hi = to_bf16(x, rules, mode)
    lo = to_bf16((x - x) if rules.lo_zero else (x - hi), rules, mode)
    return hi, lo


def expect_f16_pair(v: torch.Tensor, mode: int, rules: Rules = PLAIN):
    """(hi, lo, f2h) of split4_f16 / f2h."""

    x = v.to(torch.float64)
    hi = to_f16(x, mode, rules)
    lo = to_f16((x - x) if rules.lo_zero else (x - hi), mode, rules)
    return hi, lo, hi


def expect_f16_f8(v: torch.Tensor, mode: int, rules: Rules = PLAIN):
    """(hi, lo) of split4_f8: hi fp16, lo = e4m3((v - hi) x 2^12), returned DECODED (x 2^-12, the scale the MFMA applies)."""

    x = v.to(torch.float64)
    hi = to_f16(x, mode, rules)
    lo = to_e4m3((x - x) if rules.lo_zero else (x - hi), LO_SHIFT, mode, rules, rules.lo_decode)
    return hi, lo


def expect_e4m3_f16(h: torch.Tensor, mode: int, rules: Rules = PLAIN):
    """f16x4_to_e4m3 of the fp16 values ``h`` (given as float)."""

    return to_e4m3(h.to(torch.float64), 0, mode, rules)


def expect_e4m3_f32(v: torch.Tensor, mode: int, rules: Rules = PLAIN):
    """(f32x4_to_e4m3(v), the weight plane e4m3(v x 2^6), the weight's lo plane e4m3((v - fp16(v)) x 2^18)), decoded."""

    x = v.to(torch.float64)
    hv = to_f16(x, mode, rules)
    return (to_e4m3(x, 0, mode, rules), to_e4m3(x, rules.w_shift, mode, rules, W_SHIFT, inf_is_nan=True),
            to_e4m3(x - hv, LO_SHIFT + rules.w_shift, mode, rules, LO_SHIFT + W_SHIFT, inf_is_nan=True))


W_LO_OVERFLOW = 2.0 ** (128 - LO_SHIFT - W_SHIFT)  # from here on a weight's shifted lo part can overflow fp32 (no checkpoint's weight)


def flushed(v: torch.Tensor) -> torch.Tensor:
    """``v`` with its fp32 subnormals replaced by zeros of their sign."""

    return torch.where(is_f32_subnormal(v), v * 0.0, v)


def is_f32_subnormal(v: torch.Tensor) -> torch.Tensor:
    return (v.abs() < F32_MIN_NORMAL) & (v != 0)


def mismatches(got: torch.Tensor, exp: torch.Tensor) -> torch.Tensor:
    """Elementwise: the values differ (+0 == -0), or one is NaN and the other is not."""

    gn, en = torch.isnan(got), torch.isnan(exp)
    return (gn != en) | (~gn & ~en & (got != exp))


def zero_sign_differences(got: torch.Tensor, exp: torch.Tensor) -> int:
    return int(((got == 0) & (exp == 0) & (torch.signbit(got) != torch.signbit(exp))).sum())


# -- the conversion sweep ----------------------------------------------------------------------------------------------------------
def fp16_grid() -> np.ndarray:
    """All 65 536 fp16 bit patterns, widened to fp32."""

    return np.arange(65536, dtype=np.uint32).astype(np.uint16).view(np.float16).astype(np.float32)


def bf16_grid() -> np.ndarray:
    """All 65 536 bf16 bit patterns as fp32 (fp32 subnormals, +-Inf and NaNs among them)."""

    return (np.arange(65536, dtype=np.uint32) << 16).view(np.float32)


def with_neighbours(x: np.ndarray) -> np.ndarray:
    """Every value with its fp32 predecessor and successor."""

    x = np.asarray(x, dtype=np.float32)
    return np.concatenate([np.nextafter(x, np.float32(-np.inf)), x, np.nextafter(x, np.float32(np.inf))])


def fp16_ties() -> np.ndarray:
    """Every midpoint between adjacent finite fp16 values (65520 = the midpoint to the first value out of range included)."""

    h = fp16_grid()
    h = np.unique(h[np.isfinite(h)]).astype(np.float64)
    mid = np.concatenate([(h[:-1] + h[1:]) / 2, [65520.0, -65520.0]])
    assert (mid.astype(np.float32).astype(np.float64) == mid).all()
    return mid.astype(np.float32)


BF16_TIE_EXPONENTS = np.unique(np.linspace(0, 254, 64).astype(np.uint32))  # the biased exponents sampled (0 = subnormals)


def bf16_ties() -> np.ndarray:
    """Midpoints between adjacent bf16 values: 64 exponents x all mantissas x both signs."""

    e, m, s = np.meshgrid(BF16_TIE_EXPONENTS, np.arange(128, dtype=np.uint32), np.arange(2, dtype=np.uint32), indexing="ij")
    return ((s << 31) | (e << 23) | (m << 16) | 0x8000).astype(np.uint32).ravel().view(np.float32)


def e4m3_points(neighbours: bool = True) -> np.ndarray:
    """float64: every non-negative finite e4m3 value, every midpoint between two of them, 464 (the tie to the first value
    out of range), 480, 512 and 1024 -- with the fp32 neighbours of each (``neighbours``), in both signs."""

    vals = torch.arange(0, 0x7F, dtype=torch.uint8).view(F8).to(torch.float64).numpy()
    pts = np.concatenate([vals, (vals[:-1] + vals[1:]) / 2, [464.0, 480.0, 512.0, 1024.0]])
    if neighbours:
        pts = with_neighbours(pts.astype(np.float32)).astype(np.float64)
    pts = np.unique(pts)
    return np.concatenate([pts, -pts])


def plane_edge_centres(shift: int):
    """(t, v): the non-zero points t of :func:`e4m3_points` (without neighbours) and fp32 inputs v = hi + t x 2^-shift with
    hi = 1.5 x 2^e an fp16 value whose half ulp is above |t| x 2^-shift (e >= -13): fp16(v) = hi and v - hi = t x 2^-shift,
    exact in fp32, so the e4m3 lo plane of v (stored x 2^shift) converts exactly t."""

    t = e4m3_points(False)
    t = t[t != 0]
    e = np.clip(np.ceil(np.log2(np.abs(t))) - shift + 12, -13, 15)
    v = 1.5 * 2.0**e + t * 2.0**-shift
    assert (v.astype(np.float32).astype(np.float64) == v).all()
    return t, v.astype(np.float32)


def plane_edges(shift: int) -> np.ndarray:
    """:func:`plane_edge_centres` in both signs, and the same t on hi = 1 and hi = 0 -- each with its fp32 neighbours."""

    t, v = plane_edge_centres(shift)
    vs = np.concatenate([v, (1.0 + t * 2.0**-shift).astype(np.float32), (t * 2.0**-shift).astype(np.float32)])
    return with_neighbours(np.concatenate([vs, -vs]))


def fp16_edges() -> np.ndarray:
    big = np.float32(65520.0)
    pts = [65504.0, np.nextafter(big, np.float32(0)), 65520.0, np.nextafter(big, np.float32(np.inf)), 65536.0, 1e5, 2.0**-14, 2.0**-24,
           2.0**-25, np.nextafter(np.float32(2.0**-25), np.float32(1)), np.nextafter(np.float32(2.0**-25), np.float32(0)), 0.0]
    pts = np.asarray(pts, dtype=np.float32)
    return np.concatenate([pts, -pts])


RANDOM_COUNT, RANDOM_SEED = 2**20, 20261
SATURATING_COUNT = 2**14


def random_values() -> np.ndarray:
    """2^20 values, log-uniform magnitude over [2^-30, 2^17], random sign; and 2^14 over [256, 65504], where half an fp16
    ulp x 2^12 is beyond e4m3's range: the lo plane must saturate."""

    rng = np.random.default_rng(RANDOM_SEED)
    a = np.exp2(rng.uniform(-30.0, 17.0, RANDOM_COUNT)) * rng.choice([-1.0, 1.0], RANDOM_COUNT)
    b = np.minimum(np.exp2(rng.uniform(8.0, 16.0, SATURATING_COUNT)), 65504.0) * rng.choice([-1.0, 1.0], SATURATING_COUNT)
    return np.concatenate([a, b]).astype(np.float32)


@functools.lru_cache(maxsize=None)
def sweep() -> torch.Tensor:
    """The fp32 conversion sweep (module docstring of tests/test_gpu_primitives.py), padded with zeros to a multiple of 4."""

    w = e4m3_points() * 2.0**-W_SHIFT  # the weight's e4m3 plane (x 2^6) on every point: |w| x 2^6 around 448, 2^-15, 2^-16 ...
    parts = [fp16_grid(), bf16_grid(), with_neighbours(fp16_ties()), with_neighbours(bf16_ties()), fp16_edges(),
             plane_edges(LO_SHIFT), with_neighbours(w.astype(np.float32)), plane_edges(LO_SHIFT + W_SHIFT), random_values()]
    v = np.concatenate(parts).astype(np.float32)
    v = np.concatenate([v, np.zeros(-len(v) % 4, dtype=np.float32)])
    return torch.from_numpy(v)


def fp16_patterns() -> torch.Tensor:
    """All fp16 bit patterns as int16 (the input of the E4M3_F16 kind) -- in the order of :func:`fp16_grid`."""

    return torch.from_numpy(np.arange(65536, dtype=np.uint32).astype(np.uint16).view(np.int16).copy())


# -- sweeps of the fp32 functions ----------------------------------------------------------------------------------------------------
MASK_VALUE = -3e30  # the attention's score of a masked key
LINEAR_POINTS = 4_000_001
SPECIALS = np.asarray([0.0, -0.0, np.inf, -np.inf, np.nan, MASK_VALUE], dtype=np.float32)


def log_grid(lo_exp: float = -149.0, hi: float = 3e38, per_octave: int = 64) -> np.ndarray:
    mag = np.exp2(np.arange(lo_exp * per_octave, math.log2(hi) * per_octave) / per_octave)
    mag = np.concatenate([mag, [hi]]).astype(np.float32)
    return np.concatenate([mag, -mag])


@functools.lru_cache(maxsize=None)
def function_sweep() -> torch.Tensor:
    """GELU / EXP2: the fp16 grid, 4 000 001 points on [-12, 12], a log grid out to +-3e38, the integers of [-200, 200]
    and their halves, +-0, +-Inf, NaN and the mask value."""

    lin = np.linspace(-12.0, 12.0, LINEAR_POINTS).astype(np.float32)
    halves = (np.arange(-400, 401) / 2.0).astype(np.float32)
    return torch.from_numpy(np.concatenate([fp16_grid(), lin, log_grid(), halves, SPECIALS]).astype(np.float32))


def linear_part() -> slice:
    return slice(65536, 65536 + LINEAR_POINTS)


@functools.lru_cache(maxsize=None)
def keep_prob_inputs() -> torch.Tensor:
    """[n, 2] (l0, l1): differences over [-120, 120] on zero-centred logits, the same on logits of magnitude 1e4 (small
    differences: those fp32 keeps there), +-Inf differences, overflowing differences and NaN."""

    d = np.linspace(-120.0, 120.0, 480_001)
    rng = np.random.default_rng(RANDOM_SEED + 1)
    base = rng.uniform(-4.0, 4.0, d.shape)
    pairs = [np.stack([base + d / 2, base - d / 2], 1)]
    small = np.linspace(-8.0, 8.0, 65_537)
    big = rng.choice([-1e4, 1e4], small.shape) + rng.uniform(-50.0, 50.0, small.shape)
    pairs.append(np.stack([big + small, big], 1))
    inf, nan = np.inf, np.nan
    pairs.append(np.asarray([[inf, 0.0], [0.0, -inf], [-inf, 0.0], [0.0, inf], [89.0, 0.0], [100.0, 0.0], [1e4, -1e4], [3e38, -3e38],
                             [-89.0, 0.0], [-1e4, 1e4], [-3e38, 3e38], [0.0, 0.0], [nan, 0.0], [0.0, nan], [inf, inf], [-inf, -inf]]))
    return torch.from_numpy(np.concatenate(pairs).astype(np.float32))


@functools.lru_cache(maxsize=None)
def rope_inputs() -> torch.Tensor:
    """[n, 4] (x1, x2, cos, sin): q / k magnitudes log-uniform over [2^-20, 2^10], angles uniform -- cos / sin as fp32 --
    plus the axis angles and cancelling pairs (x1 c == x2 s up to rounding)."""

    rng = np.random.default_rng(RANDOM_SEED + 2)
    n = 2**18
    x = np.exp2(rng.uniform(-20.0, 10.0, (n, 2))) * rng.choice([-1.0, 1.0], (n, 2))
    a = rng.uniform(0.0, 2 * math.pi, n)
    a[:8] = np.arange(8) * math.pi / 4
    c, s = np.cos(a), np.sin(a)
    x[n // 2:, 1] = x[n // 2:, 0] * c[n // 2:] / np.where(np.abs(s[n // 2:]) < 1e-3, 1.0, s[n // 2:])  # x1 c - x2 s ~ 0
    return torch.from_numpy(np.concatenate([x, c[:, None], s[:, None]], 1).astype(np.float32))


# -- GELU: the polynomial of opk_common.hip.h gelu_erf, emulated in fp32 ------------------------------------------------------------
GELU_COEFFS = (-4.7330930829e-04, 7.0845573209e-03, -5.1827382296e-02, -4.5999243855e-01, -1.1507878304e+00, -1.0000376701e+00)
GELU_FLOOR = am.FLOOR  # what arith_model's "not modelled" list claims for the fp32 GELU
GELU_MARGIN = 1.25  # x the emulation's maximum: v_exp_f32's last place enters as |x| he(|x|) 2^-23 <= 2e-8, ~3 % of 6.4e-7


# The negative side, relative to the polynomial itself.  For x < 0, gelu = -|x| 2^q(|x|): q is the same chain of five IEEE fp32
# FMAs on the device and in the emulation (the same bits); the device's 2^q is v_exp_f32's, within 2^-22 relative (the bound
# tests/test_gpu_primitives.py asserts for the instruction on [-160, 6]), the emulation's is correctly rounded, 2^-24; the closing
# FMA rounds -he |x| + 0 once on each side, 2^-24 each: |device - emulation| <= (2^-22 + 3 x 2^-24) |emulation| < 2^-21 |emulation|.
# Held where the emulation's result is a normal number clear of v_exp_f32's flush (|gelu| >= 2^-120).  The absolute bounds above
# resolve a coefficient only down to ~1.6e-7 of gelu; this one resolves 2^-21 of he, i.e. every digit the fp32 coefficients hold.
GELU_TAIL_REL = 2.0**-21
GELU_TAIL_MIN = 2.0**-120


def gelu_tail_ratio(x: np.ndarray, got: np.ndarray, emulated: np.ndarray):
    """(worst |got - emulated| / (GELU_TAIL_REL |emulated|), the x it is at, elements compared) over the finite x < 0 whose
    emulated gelu is at least GELU_TAIL_MIN in magnitude."""

    x = np.asarray(x, dtype=np.float32)
    e = np.asarray(emulated, dtype=np.float64)
    where = np.isfinite(x) & (x < 0) & (np.abs(e) >= GELU_TAIL_MIN)
    with np.errstate(all="ignore"):
        r = np.abs(np.asarray(got, dtype=np.float64)[where] - e[where]) / (GELU_TAIL_REL * np.abs(e[where]))
    r = np.where(np.isnan(r), np.inf, r)
    k = int(r.argmax())
    return float(r[k]), float(x[where][k]), int(where.sum())


def _fma32(a, b, c):
    """One fp32 FMA (the float64 product of two fp32 values is exact; the sum is rounded to float64, then to fp32)."""

    with np.errstate(all="ignore"):
        return (a.astype(np.float64) * b.astype(np.float64) + np.asarray(c, dtype=np.float64)).astype(np.float32)


def gelu_emulated(x: np.ndarray, coeffs=GELU_COEFFS, he_on_x: bool = False) -> np.ndarray:
    """gelu_erf in numpy fp32: five FMAs, a correctly rounded exp2 (flushed below fp32's normal range, as v_exp_f32 does),
    max(x, 0) and one FMA.  ``he_on_x``: mutation, the polynomial applied to x instead of |x|."""

    x = np.asarray(x, dtype=np.float32)
    ax = np.abs(x)
    arg = x if he_on_x else ax
    c = [np.float32(v) for v in coeffs]
    q = _fma32(np.full_like(arg, c[0]), arg, c[1])
    for k in c[2:]:
        q = _fma32(q, arg, k)
    with np.errstate(all="ignore"):
        he = np.exp2(q.astype(np.float64)).astype(np.float32)
    he = np.where(np.abs(he) < np.float32(F32_MIN_NORMAL), np.float32(0), he)
    relu = np.where(np.isnan(x), x, np.maximum(x, np.float32(0)))
    return _fma32(-he, ax, relu)


def gelu_exact(x: np.ndarray) -> np.ndarray:
    """0.5 x erfc(-x / sqrt 2) in float64 (no cancellation on the negative side)."""

    t = torch.from_numpy(np.asarray(x, dtype=np.float64))
    return (0.5 * t * torch.erfc(-t / math.sqrt(2.0))).numpy()


def perturbed_coeffs(k: int, sign: float = 1.0):
    """GELU_COEFFS with coefficient k moved by one unit of its 5th significant digit."""

    c = list(GELU_COEFFS)
    c[k] += sign * 10.0 ** (math.floor(math.log10(abs(c[k]))) - 4)
    return tuple(c)
