"""The case table of csrc/og_math.h and csrc/og_dual.h: one set of inputs per function, used by the CPU tests
(tests/test_og_math_edges.py: the host build against mpmath) and by the GPU tests (tests/test_og_math_gpu.py: the
device build against the host build, bit for bit).  Everything is seeded; the table is the same object everywhere.

Also here: the three builds of tests/og_math_probe.hip, the high-precision reference, and ``--report``, which writes
profiles/og_math_edges.md.

Bit equality: two doubles are equal when their 64 bits are, EXCEPT that a NaN equals a NaN whatever its payload and
sign (x86 and gfx950 produce different default NaNs); the sign of a zero counts.
"""
from __future__ import annotations

import ctypes as C
import math
import os
import re
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
CSRC = os.path.join(ROOT, "opengoddard_amd", "csrc")
PROBE = os.path.join(ROOT, "tests", "og_math_probe.hip")

# function ids of the probe (the order of its enum; checked against ogp_name by load())
FUNCS = ["exp", "log", "sin", "cos", "tan", "atan", "asin", "acos", "expm1", "log1p", "sinh", "cosh", "tanh", "log2",
         "log10", "cbrt", "sqrt", "fabs", "floor", "trunc", "atan2", "hypot", "pow", "mod", "fmod", "scalb", "interp",
         "div", "mul"]
ONE_ARG = FUNCS[:FUNCS.index("atan2")]
TWO_ARG = ["atan2", "hypot", "pow", "mod", "fmod"]
DUAL_ONE = ["exp", "log", "sin", "cos", "tan", "atan", "asin", "acos", "expm1", "log1p", "sinh", "cosh", "tanh", "log2",
            "log10", "cbrt", "sqrt", "fabs"]                       # og_dual.h has a rule for these ...
DUAL_TWO = ["atan2", "hypot", "pow", "mod", "fmod", "div", "mul"]  # ... and these (and interp)

INF, NAN = np.inf, np.nan
DBL_MIN, DBL_MAX, DENORM_MIN = 2.2250738585072014e-308, 1.7976931348623157e308, 5e-324
MAX_SUBNORMAL = np.nextafter(DBL_MIN, 0.0)
EPS = 2.0 ** -52


# ---------------------------------------------------------------------------------------------------------------------
# the random distributions of tests/test_og_math.py (it imports them from here: the two cannot drift)
# (function, NumPy reference, sample(rng), allowance in ulp against NumPy)
N_RANDOM = 200000
RANDOM_BASIC = [
    ("exp", np.exp, lambda r: r.uniform(-700, 700, N_RANDOM), 1.0),
    ("exp", np.exp, lambda r: r.uniform(-1, 1, N_RANDOM) * 10.0 ** r.integers(-12, 1, N_RANDOM), 1.0),
    ("log", np.log, lambda r: np.exp(r.uniform(-700, 700, N_RANDOM)), 1.0),
    ("sin", np.sin, lambda r: r.uniform(-100, 100, N_RANDOM), 1.0),
    ("cos", np.cos, lambda r: r.uniform(-100, 100, N_RANDOM), 1.0),
    ("sin", np.sin, lambda r: r.uniform(-1e5, 1e5, N_RANDOM), 1.0),
    ("cos", np.cos, lambda r: r.uniform(-1e5, 1e5, N_RANDOM), 1.0),
    # beyond the Cody-Waite range (2^20 * pi/2): the double-double reduction, up to 2^45
    ("sin", np.sin, lambda r: r.uniform(-1, 1, N_RANDOM) * 10.0 ** r.uniform(6.3, 13.5, N_RANDOM), 1.0),
    ("cos", np.cos, lambda r: r.uniform(-1, 1, N_RANDOM) * 10.0 ** r.uniform(6.3, 13.5, N_RANDOM), 1.0),
    ("tan", np.tan, lambda r: r.uniform(-1, 1, N_RANDOM) * 10.0 ** r.uniform(6.3, 13.5, N_RANDOM), 2.0),
    ("tan", np.tan, lambda r: r.uniform(-1.5, 1.5, N_RANDOM), 2.0),
    ("atan", np.arctan, lambda r: r.standard_normal(N_RANDOM) * 10.0 ** r.integers(-10, 10, N_RANDOM), 1.0),
    ("asin", np.arcsin, lambda r: r.uniform(-1, 1, N_RANDOM), 1.0),
    ("acos", np.arccos, lambda r: r.uniform(-1, 1, N_RANDOM), 1.0),
    ("asin", np.arcsin, lambda r: np.sign(r.uniform(-1, 1, N_RANDOM)) * (1 - 10.0 ** r.uniform(-12, -1, N_RANDOM)), 1.0),
    ("acos", np.arccos, lambda r: np.sign(r.uniform(-1, 1, N_RANDOM)) * (1 - 10.0 ** r.uniform(-12, -1, N_RANDOM)), 1.0),
]
RANDOM_WIDENED = [
    ("expm1", np.expm1, lambda r: r.uniform(-1, 1, N_RANDOM) * 10.0 ** r.integers(-12, 3, N_RANDOM), 3.0),
    ("expm1", np.expm1, lambda r: r.uniform(-40, 700, N_RANDOM), 3.0),
    ("log1p", np.log1p, lambda r: r.uniform(-1, 1, N_RANDOM) * 10.0 ** r.integers(-12, 1, N_RANDOM), 2.0),
    ("log1p", np.log1p, lambda r: np.exp(r.uniform(-30, 700, N_RANDOM)), 2.0),
    ("sinh", np.sinh, lambda r: r.uniform(-1, 1, N_RANDOM) * 10.0 ** r.integers(-10, 3, N_RANDOM), 3.0),
    ("cosh", np.cosh, lambda r: r.uniform(-1, 1, N_RANDOM) * 10.0 ** r.integers(-10, 3, N_RANDOM), 2.0),
    ("tanh", np.tanh, lambda r: r.uniform(-1, 1, N_RANDOM) * 10.0 ** r.integers(-10, 2, N_RANDOM), 3.0),
    ("log2", np.log2, lambda r: np.exp(r.uniform(-700, 700, N_RANDOM)), 1.0),
    ("log10", np.log10, lambda r: np.exp(r.uniform(-700, 700, N_RANDOM)), 1.0),
    # the whole exponent range (the sample stopped at 10^+-100 before cbrt_ was found wrong beyond 10^+-230)
    ("cbrt", np.cbrt, lambda r: r.standard_normal(N_RANDOM) * 10.0 ** r.integers(-100, 100, N_RANDOM), 1.0),
    ("cbrt", lambda x: np.cbrt(x), lambda r: r.standard_normal(N_RANDOM) * 10.0 ** r.integers(-307, 308, N_RANDOM), 1.0),
]
RANDOM_WIDENED[-1][1].__name__ = "cbrt_over_the_exponent_range"        # (its own test id: the case above keeps its id)


def random_atan2():
    rng = np.random.default_rng(1)
    y = rng.standard_normal(300000) * 10.0 ** rng.integers(-8, 8, 300000)
    x = rng.standard_normal(300000) * 10.0 ** rng.integers(-8, 8, 300000)
    return y, x


def random_hypot():
    """-> the generator (test_og_math.py goes on drawing from it), (a, b) wide, (a, b) of similar size"""
    r = np.random.default_rng(2)
    a = r.standard_normal(300000) * 10.0 ** r.integers(-150, 150, 300000)
    b = r.standard_normal(300000) * 10.0 ** r.integers(-150, 150, 300000)
    b2 = a * 10.0 ** r.uniform(-3, 3, a.size)
    return r, (a, b), (a, b2)


def random_pow(r=None):
    if r is None:
        r = random_hypot()[0]
    return np.exp(r.uniform(-5, 5, 300000)), r.uniform(-4, 4, 300000)


def random_mod():
    rng = np.random.default_rng(5)
    a = rng.uniform(-50, 50, 200000) * 10.0 ** rng.integers(-3, 6, 200000)
    b = rng.uniform(-5, 5, 200000)
    b[b == 0.0] = 1.0
    return a, b


def random_inputs(name):
    """every shared random distribution of one function -> list of (a, b) (b None for one argument)"""
    out = [(sample(np.random.default_rng(0)), None) for n, _, sample, _ in RANDOM_BASIC + RANDOM_WIDENED if n == name]
    if name == "atan2":
        out.append(random_atan2())
    if name == "hypot":
        out += list(random_hypot()[1:])
    if name == "pow":
        out.append(random_pow())
    if name in ("mod", "fmod"):
        a, b = random_mod()
        out += [(a, b), (np.round(a), np.round(b) + (np.round(b) == 0))]
    return out


# ---------------------------------------------------------------------------------------------------------------------
# allowances: what tests/test_og_math.py asserts against NumPy, in ulp (pow: times max(1, |y log x|))
ALLOWANCE = {n: tol for n, _, _, tol in RANDOM_BASIC + RANDOM_WIDENED}
ALLOWANCE.update(atan2=1.0, hypot=1.0, pow=3.0, sqrt=0.0, fabs=0.0)
NUMPY = {"exp": np.exp, "log": np.log, "sin": np.sin, "cos": np.cos, "tan": np.tan, "atan": np.arctan,
         "asin": np.arcsin, "acos": np.arccos, "expm1": np.expm1, "log1p": np.log1p, "sinh": np.sinh, "cosh": np.cosh,
         "tanh": np.tanh, "log2": np.log2, "log10": np.log10, "cbrt": np.cbrt, "sqrt": np.sqrt, "fabs": np.fabs,
         "floor": np.floor, "trunc": np.trunc, "atan2": np.arctan2, "hypot": np.hypot, "pow": np.power,
         "mod": np.remainder, "fmod": np.fmod}


# ---------------------------------------------------------------------------------------------------------------------
# branch thresholds, read off csrc/og_math.h; the comment names the line each comes from.  test_..._knows_every_threshold
# greps the header for the constants in conditions and fails on one that is not listed for the function it stands in.
def hi(word):
    """the double whose high word is ``word`` and whose low word is 0 (the `ix < 0x...u` cuts)"""
    return float(np.array([word << 32], dtype=np.uint64).view(np.float64)[0])


LN2_HALF, TWO_M28, TWO_M27, PIO4 = 0.34657359027997264, 3.725290298461914e-09, 7.450580596923828e-09, 7.85398163397448278999e-01
EXP_OVER, EXP_UNDER = 7.09782712893383973096e+02, -7.45133219101941108420e+02
TRIG = [PIO4,                       # sin_/cos_/tan_: `ax <= 7.85398163397448278999e-01`, tan_: `ax > ...`
        TWO_M27,                    # `ax < 7.450580596923828e-09`
        1647099.0,                  # rem_pio2: `!(fabs_(x) < 1647099.0)`
        35184372088832.0,           # rem_pio2_large: `!(fabs_(x) < 35184372088832.0)` (2^45: NaN from here on)
        0.30000001192092896,        # kcos: `ax < 0.30000001192092896`
        0.78125,                    # kcos: `(ax > 0.78125) ? 0.28125 : ...`
        0.5, 1.5707963267948966]    # rem_pio2: `x < 0.0 ? -0.5 : 0.5` (the quadrant changes at odd multiples of pi/4)
THRESHOLDS = {
    "exp": [EXP_OVER,               # `x > 7.09782712893383973096e+02`
            EXP_UNDER,              # `x < -7.45133219101941108420e+02`
            LN2_HALF,               # `ax > 0.34657359027997264`
            TWO_M28,                # `ax < 3.725290298461914e-09`
            0.5, 1.0397207708399179],       # nearest_int: `v < 0.0 ? v - 0.5 : v + 0.5` (k changes at 1.5 ln 2)
    "log": [DBL_MIN,                # `(u >> 52) == 0`: subnormal
            hi(0x3fe6a09e), hi(0x3ff6a09e), 1.0],   # `hx += 0x3ff00000 - 0x3fe6a09e`: the mantissa cut at sqrt(2)/2
    "sin": TRIG, "cos": TRIG, "tan": TRIG,
    "atan": [hi(0x44100000),        # `ix >= 0x44100000u`  2^66
             hi(0x3fdc0000),        # `ix < 0x3fdc0000u`   0.4375
             hi(0x3e200000),        # `ix < 0x3e200000u`   2^-29
             hi(0x3ff30000),        # `ix < 0x3ff30000u`   1.1875
             hi(0x3fe60000),        # `ix < 0x3fe60000u`   0.6875
             hi(0x40038000)],       # `ix < 0x40038000u`   2.4375
    "asin": [1.0,                   # `ax >= 1.0`, `ax == 1.0`
             hi(0x3fe00000),        # `ix < 0x3fe00000u`   0.5
             hi(0x3e500000),        # `ix < 0x3e500000u`   2^-26
             hi(0x3fef3333)],       # `ix >= 0x3fef3333u`  0.975
    "acos": [1.0, hi(0x3fe00000),
             hi(0x3c600000)],       # `ix <= 0x3c600000u`  2^-57
    "expm1": [709.8,                # `x > 709.8`
              -40.0,                # `x < -40.0`
              1.0],                 # `fabs_(x) < 1.0`
    "log1p": [-1.0,                 # `x < -1.0`
              2.0 ** -53, 2.0 ** -54, 1.0],  # `u == 1.0`, u = 1 + x
    "sinh": [1.0, 22.0, 709.0,      # `ax < 1.0`, `ax < 22.0`, `ax < 709.0`
             710.4758600739439, 2 * EXP_OVER],      # result overflows; exp_(0.5 ax) overflows
    "cosh": [1.0, 22.0, 709.0, 710.4758600739439, 2 * EXP_OVER],
    "tanh": [22.0,                  # `ax >= 22.0`
             1.0, EXP_OVER / 2],    # `ax < 1.0`
    "log2": [DBL_MIN,               # `x < 2.2250738585072014e-308`
             1.4142135623730951,    # `m > 1.4142135623730951`
             1.4142135623730951 * 2.0 ** 500, 1.4142135623730951 * 2.0 ** -1000, 1.0, hi(0x3fe6a09e), hi(0x3ff6a09e)],
    "log10": [DBL_MIN, hi(0x3fe6a09e), hi(0x3ff6a09e), 1.0, 10.0, 1e15, 1e22],    # log_'s; exact powers of ten
    "cbrt": [2.0 ** -700,           # `ax < 0x1p-700`
             2.0 ** 700,            # `ax > 0x1p+700`
             2.0 ** -766, 2.0 ** 807, 8.0, 27.0],       # where the unscaled Newton step under- / overflowed
    "sqrt": [DBL_MIN, 1.0, 4.0], "fabs": [DBL_MIN], "floor": [1.0, 0.5, 2.0 ** 52, 2.0 ** 53],
    "trunc": [1.0, 0.5, 2.0 ** 52, 2.0 ** 53],
    # two arguments: thresholds of the first / second argument or of their quotient, see two_arg_table
    "atan2": [1.0,                  # `x == 1.0`
              2.0 ** 60, 2.0 ** -60, 2.0 ** 61, 2.0 ** -61],    # `k > 60`, `k < -60`, k the difference of the exponents
    "hypot": [1.0, 2.0 ** 27, 2.0 ** -27, 2.0 ** 54, 2.0 ** -54],   # `a < b`; where b^2 vanishes against a^2
    "pow": [64.0,                   # `fabs_(y) <= 64.0`
            9007199254740992.0,     # `fabs_(y) >= 9007199254740992.0`  2^53
            1.0, 2147483648.0, 9.0e15, 9223372036854775808.0],     # `x == 1.0`, `fabs_(x) == 1.0`; the casts' ranges
    "mod": [1.0], "fmod": [1.0],
    "scalb": [1000.0, -1000.0],     # `k > 1000`, `k < -1000`
}
# constants in conditions of og_math.h that are not thresholds on an input, each with its reason
NOT_A_THRESHOLD = {
    1.0e300: "`ax < 1.0e300 * 1.0e300` is `ax < inf`: the infinities are in the special values",
    0.0: "comparisons with zero: +-0 and the smallest subnormals are in the special values of every function",
    0.28125: "kcos: the value of qx, not a condition (it stands in the arm of the ?:)",
}
# internal helpers -> the public functions whose table must hold their thresholds
OWNER = {"nearest_int": ["exp"], "rem_pio2": ["sin", "cos", "tan"], "rem_pio2_large": ["sin", "cos", "tan"],
         "ksin": ["sin", "cos", "tan"], "kcos": ["sin", "cos", "tan"], "scalb_": ["scalb"]}

# the guards in front of the float-to-int casts: (guard, function, inputs just inside and outside it).  Host and device
# saturate an out-of-range cast differently, so the guards must keep every cast in range on both.
CAST_GUARDS = [
    ("nearest_int: |v| < 2^31, reached from exp_ only, behind exp_'s overflow / underflow returns", "exp",
     [EXP_OVER, EXP_UNDER, 710.0, -746.0, 1e10, -1e10, 3e9, -3e9, DBL_MAX, -DBL_MAX]),
    ("rem_pio2_large: (long long)(x * inv_pio2 +- 0.5) behind `!(fabs_(x) < 2^45)`", "sin",
     [35184372088832.0, 1.4e19, 1.5e19, 9.3e18, 2.0 ** 63 * 1.5707963267948966, 1e300]),
    ("rem_pio2_large: (long long)(x * inv_pio2 +- 0.5) behind `!(fabs_(x) < 2^45)`", "cos",
     [35184372088832.0, 1.4e19, 1.5e19, 9.3e18, 2.0 ** 63 * 1.5707963267948966, 1e300]),
    ("rem_pio2_large: (long long)(x * inv_pio2 +- 0.5) behind `!(fabs_(x) < 2^45)`", "tan",
     [35184372088832.0, 1.4e19, 1.5e19, 9.3e18, 2.0 ** 63 * 1.5707963267948966, 1e300]),
]
POW_CAST_Y = [64.0, 65.0, 2147483647.0, 2147483648.0, 2147483649.0, 4294967296.0, 4294967297.0, 9.0e15, 9.0e15 + 1.0,
              2.0 ** 53 - 1.0, 2.0 ** 53, 2.0 ** 53 + 2.0, 2.0 ** 63 - 1024.0, 2.0 ** 63, 2.0 ** 64, 1e16, 1e19, 1e300,
              DBL_MAX]          # `(int)y` behind |y| <= 64, `(long long)y` behind |y| < 2^53


def neighbours(values, k=4):
    """each value with its k neighbours below and above, both signs"""
    out = []
    for v in values:
        v = float(v)
        lo = up = v
        out.append(v)
        for _ in range(k):
            with np.errstate(over="ignore"):                # above DBL_MAX: inf, wanted
                lo, up = np.nextafter(lo, -INF), np.nextafter(up, INF)
            out += [float(lo), float(up)]
    out = np.array(out)
    return np.concatenate([out, -out])


def sweep_exponents():
    """the 64 exponents at either end, every 8th between, every one in [-80, 80] (2^-57, 2^-29 ... 2^66: the small
    cuts and exp / sinh / trig regime changes), and those around a result's change of regime"""
    es = set(range(-1074, -1074 + 64)) | set(range(1023 - 63, 1024)) | set(range(-1074, 1024, 8)) | set(range(-80, 81))
    for centre in (-1022, -969, -770, -766, -727, -700, -512, -341, 341, 512, 700, 802, 807):
        es |= set(range(centre - 3, centre + 4))
    return sorted(e for e in es if -1074 <= e <= 1023)


def exponent_sweep():
    out = [math.ldexp(m, e) for e in sweep_exponents() for m in (1.0, 1.0 + EPS, 1.5, 2.0 - EPS)]
    out = np.unique(np.array(out))
    return np.concatenate([out, -out])


SPECIALS = np.array([0.0, -0.0, INF, -INF, NAN, DENORM_MIN, -DENORM_MIN, MAX_SUBNORMAL, -MAX_SUBNORMAL, DBL_MIN,
                     -DBL_MIN, DBL_MAX, -DBL_MAX, 1.0, -1.0])
ORDINARY = np.array([0.5, -0.5, 2.0, -2.0, 3.0, -3.0, 2.5, -2.5, 0.75, 7.0, -7.0, 1e-3, -1e3, 1e10, 1e-10, 123.456,
                     -1e300])
GRID = np.concatenate([SPECIALS, ORDINARY])         # 32 values: the 32 x 32 grid of the two-argument functions
assert GRID.size == 32


def large_angles():
    """log-uniform samples from 1.6e6 to 2^45, multiples of pi/2 rounded to double over that range (worst cancellation),
    and the points just below and above 2^45"""
    r = np.random.default_rng(45)
    x = np.exp(r.uniform(np.log(1.6e6), np.log(2.0 ** 45), 1500))
    k = np.floor(np.exp(r.uniform(np.log(1.6e6), np.log(2.0 ** 45 / 1.5707963267948966), 1500)))
    m = k * 1.5707963267948966
    m = m[m < 2.0 ** 45]
    edge = neighbours([2.0 ** 45])
    out = np.concatenate([x, m, np.nextafter(m, INF), np.nextafter(m, -INF)])
    return np.concatenate([out, -out, edge])


def one_arg_table(name):
    parts = [neighbours(THRESHOLDS.get(name, [])), exponent_sweep(), SPECIALS, ORDINARY]
    if name in ("sin", "cos", "tan"):
        parts.append(large_angles())
        k = np.arange(1, 200.0)
        parts.append(neighbours(k * PIO4, 1))               # the quadrant boundaries and the zeros / poles nearby
    for _, fn, xs in CAST_GUARDS:
        if fn == name:
            parts.append(neighbours(xs, 1))
    return np.concatenate(parts), None


def two_arg_table(name):
    a, b = [g.ravel() for g in np.meshgrid(GRID, GRID, indexing="ij")]
    parts = [(a, b)]
    sweep = exponent_sweep()[::3]
    r = np.random.default_rng(7)
    if name == "pow":
        ys = np.concatenate([np.arange(-70.0, 71.0), np.arange(-70.0, 71.0) + 0.5, neighbours(THRESHOLDS["pow"][:2], 2),
                             POW_CAST_Y, -np.array(POW_CAST_Y)])
        xs = np.array([-INF, -DBL_MAX, -1e300, -8.0, -2.0, -1.0 - EPS, -1.0, -1.0 + EPS / 2, -0.5, -1e-300, -DENORM_MIN,
                       -0.0, 0.0, DENORM_MIN, 1e-300, 0.5, 1.0 - EPS / 2, 1.0, 1.0 + EPS, 2.0, 10.0, 1e300, DBL_MAX, INF])
        x2, y2 = [g.ravel() for g in np.meshgrid(xs, ys, indexing="ij")]
        parts.append((x2, y2))
        for y in (2.0, -3.0, 0.5, -0.5, 65.0, -65.0, 1.0 / 3.0):          # the exponent range of the base
            parts.append((np.abs(sweep), np.full(sweep.size, y)))
        parts.append((np.exp(r.uniform(-1, 1, 400)), r.uniform(-1000, 1000, 400)))      # results over the whole range
    elif name == "atan2":
        for q in THRESHOLDS["atan2"]:
            x = np.concatenate([np.abs(sweep[::5]), [1.0, 3.0, 1e-200, 1e200]])
            for sy in (1.0, -1.0):
                for sx in (1.0, -1.0):
                    for f in neighbours([q], 2)[:5]:
                        with np.errstate(all="ignore"):
                            parts.append((sy * x * f, sx * x))
        parts.append((sweep, np.ones(sweep.size)))
        parts.append((np.ones(sweep.size), sweep))
        parts.append((sweep, sweep[::-1].copy()))
    elif name == "hypot":
        for q in THRESHOLDS["hypot"]:
            x = np.abs(sweep)
            with np.errstate(all="ignore"):
                parts += [(x, x * q), (x * q, -x), (x, np.nextafter(x * q, INF))]
        parts.append((sweep, sweep[::-1].copy()))
    else:                                                   # mod, fmod
        parts.append((sweep, np.full(sweep.size, 3.0)))
        parts.append((sweep, np.full(sweep.size, -DBL_MIN)))
        parts.append((np.full(sweep.size, 1e300), sweep))
        parts.append((sweep, sweep[::-1].copy()))
        k = np.arange(-40.0, 41.0)
        parts.append((k * 0.5, np.full(k.size, 2.0)))
        parts.append((k * 0.5, np.full(k.size, -2.0)))
    a = np.concatenate([p[0] for p in parts])
    b = np.concatenate([p[1] for p in parts])
    return a, b


def scalb_table():
    ks = np.concatenate([np.arange(-2100.0, 2101.0, 7.0), neighbours_int([1000, -1000, 0, 2100, -2100, 1023, -1074])])
    ks = ks[(ks >= -2100) & (ks <= 2100)]
    xs = np.concatenate([SPECIALS, [1.5, -1.5, 1.0 + EPS, 2.0 - EPS, 1e300, 1e-300, 3e-320]])
    a, b = [g.ravel() for g in np.meshgrid(xs, ks, indexing="ij")]
    return a, b


def neighbours_int(values):
    return np.array([float(v + d) for v in values for d in (-2, -1, 0, 1, 2)])


_TABLES = {}


def table(name):
    """-> (a, b): the inputs of one function (b None for one argument)"""
    if name not in _TABLES:
        if name in ONE_ARG:
            _TABLES[name] = one_arg_table(name)
        elif name == "scalb":
            _TABLES[name] = scalb_table()
        elif name in ("div", "mul"):
            a, b = [g.ravel() for g in np.meshgrid(GRID, GRID, indexing="ij")]
            _TABLES[name] = (a, b)
        else:
            _TABLES[name] = two_arg_table(name)
    return _TABLES[name]


# ---------------------------------------------------------------------------------------------------------------------
# interp_linear: tables of n = 2, 3, 257 knots, uniform and not; x at, between, next to and outside the knots
def interp_tables():
    r = np.random.default_rng(11)
    out = []
    for n in (2, 3, 257):
        uniform = np.linspace(-1.0, 3.0, n)
        ragged = np.cumsum(np.concatenate([[-5.0], 10.0 ** r.uniform(-3, 1, n - 1)]))
        for kind, xg in (("uniform", uniform), ("non-uniform", ragged)):
            yg = r.standard_normal(n) * 10.0
            out.append(("n=%d %s" % (n, kind), xg, yg))
    return out


def interp_queries(xg):
    mid = 0.5 * (xg[:-1] + xg[1:])
    r = np.random.default_rng(12)
    between = r.uniform(xg[0], xg[-1], 200)
    edge = neighbours([xg[0], xg[-1]], 2)[:10]
    span = xg[-1] - xg[0]
    outside = np.array([xg[0] - 0.5 * span, xg[0] - 1e6, xg[-1] + 0.5 * span, xg[-1] + 1e6, -DBL_MAX, DBL_MAX])
    return np.concatenate([xg, np.nextafter(xg, INF), np.nextafter(xg, -INF), mid, between, edge, outside,
                           [INF, -INF, NAN]])


FILLS = (-7.25, 11.5)


def all_cases():
    """(label, function, variant, a, b, da, db, table) over the whole case table: what the two host compilers and the
    device are compared on"""
    for name in ONE_ARG:
        a, _ = table(name)
        yield name, name, 0, a, None, None, None, None
        if name in DUAL_ONE:
            yield name + " dual d=1", name, 1, a, None, np.ones(a.size), None, None
            yield name + " dual d=0", name, 1, a, None, np.zeros(a.size), None, None
    for name in TWO_ARG + ["scalb", "div", "mul"]:
        a, b = table(name)
        yield name, name, 0, a, b, None, None, None
        if name in DUAL_TWO:
            for label, variant, da, db in (("both", 1, 1.0, -0.5), ("first", 1, 1.0, 0.0), ("second", 1, 0.0, 1.0),
                                           ("none", 1, 0.0, 0.0), ("(dual, double)", 2, 1.0, 0.0),
                                           ("(double, dual)", 3, 0.0, 1.0)):
                yield "%s dual %s" % (name, label), name, variant, a, b, np.full(a.size, da), np.full(a.size, db), None
    for label, xg, yg in interp_tables():
        x = interp_queries(xg)
        for mode in (0, 1, 2):
            yield "interp %s mode %d" % (label, mode), "interp", 0, x, None, None, None, (xg, yg, mode)
            yield "interp %s mode %d dual" % (label, mode), "interp", 1, x, None, np.ones(x.size), None, (xg, yg, mode)


# ---------------------------------------------------------------------------------------------------------------------
# the three builds of the probe
def _compile_host(compiler, out):
    subprocess.check_call([compiler, "-O2", "-std=c++17", "-ffp-contract=off", "-mfma", "-fPIC", "-shared", "-I" + CSRC,
                           "-x", "c++", PROBE, "-o", out])
    return out


def clangxx():
    from opengoddard_amd import build
    for cand in (os.path.join(os.path.dirname(os.path.realpath(build.hipcc())), "..", "llvm", "bin", "clang++"),
                 "/opt/rocm/llvm/bin/clang++", "/opt/rocm/lib/llvm/bin/clang++"):
        if os.path.exists(cand):
            return os.path.realpath(cand)
    raise RuntimeError("clang++ of the ROCm toolchain not found next to hipcc")


def probe_path(kind, csrc=None):
    """where a build of the probe lives: next to the other JIT products, keyed by the content of its sources"""
    from opengoddard_amd import build
    digest = build._digest_files([PROBE, os.path.join(csrc or CSRC, "og_math.h"), os.path.join(csrc or CSRC, "og_dual.h")])
    os.makedirs(build.JITDIR, exist_ok=True)
    return os.path.join(build.JITDIR, "ogmath_probe_%s_%s.so" % (kind, digest))


def build_probe(kind):
    """kind: "gxx" (the twin's compiler), "clang" (the host compiler of a HIP module) or "hip" (hipcc with
    build.HIP_FLAGS unchanged: the kernel, the launcher and clang's host loop) -> path of the shared object"""
    from opengoddard_amd import build
    out = probe_path(kind)
    if os.path.exists(out):
        return out
    tmp = out + ".tmp%d" % os.getpid()
    if kind == "gxx":
        _compile_host("g++", tmp)
    elif kind == "clang":
        _compile_host(clangxx(), tmp)
    else:
        build._run([build.hipcc()] + build.HIP_FLAGS + ["-I" + CSRC, PROBE, "-o", tmp])
    os.replace(tmp, out)
    return out


_DP = C.POINTER(C.c_double)


class Probe:
    def __init__(self, path):
        self.lib = C.CDLL(path)
        self.lib.ogp_name.restype = C.c_char_p
        names = [self.lib.ogp_name(i).decode() for i in range(self.lib.ogp_count())]
        assert names == FUNCS, "tests/og_math_probe.hip and og_math_cases.FUNCS list different functions"
        self.lib.ogp_host.restype = None
        self.lib.ogp_host.argtypes = [C.c_int, C.c_int, _DP, _DP, _DP, _DP, _DP, _DP, C.c_int, _DP, _DP, C.c_int,
                                      C.c_int, C.c_double, C.c_double]
        if hasattr(self.lib, "ogp_device"):
            self.lib.ogp_device.restype = C.c_int
            self.lib.ogp_device.argtypes = [C.c_int, C.c_int, _DP, _DP, _DP, _DP, _DP, _DP, C.c_int, C.c_int, _DP, _DP,
                                            C.c_int, C.c_int, C.c_double, C.c_double]

    @staticmethod
    def _args(a, b, da, db, tab):
        a = np.ascontiguousarray(a, dtype=np.float64).ravel()
        full = lambda v, fill: (np.full(a.size, fill) if v is None else
                                np.ascontiguousarray(np.broadcast_to(np.asarray(v, dtype=np.float64), a.shape)).copy())
        b, da, db = full(b, 1.0), full(da, 1.0), full(db, 0.0)
        if tab is None:
            tab = (np.array([0.0, 1.0]), np.array([0.0, 1.0]), 1)
        xg, yg, mode = np.ascontiguousarray(tab[0], dtype=np.float64), np.ascontiguousarray(tab[1], dtype=np.float64), tab[2]
        assert xg.size == yg.size >= 2
        return a, b, da, db, xg, yg, int(mode)

    def host(self, name, a, b=None, da=None, db=None, variant=0, tab=None):
        """-> (values, derivatives) of function ``name`` over the arrays, on the host"""
        a, b, da, db, xg, yg, mode = self._args(a, b, da, db, tab)
        ov, od = np.empty_like(a), np.empty_like(a)
        p = lambda v: v.ctypes.data_as(_DP)
        self.lib.ogp_host(FUNCS.index(name), variant, p(a), p(b), p(da), p(db), p(ov), p(od), a.size, p(xg), p(yg),
                          xg.size, mode, FILLS[0], FILLS[1])
        return ov, od

    def device(self, name, a, b=None, da=None, db=None, variant=0, tab=None, block=64):
        """the same on the GPU -> (HIP's error code, values, derivatives)"""
        a, b, da, db, xg, yg, mode = self._args(a, b, da, db, tab)
        ov, od = np.empty_like(a), np.empty_like(a)
        p = lambda v: v.ctypes.data_as(_DP)
        err = self.lib.ogp_device(FUNCS.index(name), variant, p(a), p(b), p(da), p(db), p(ov), p(od), a.size, block,
                                  p(xg), p(yg), xg.size, mode, FILLS[0], FILLS[1])
        return err, ov, od


_PROBES = {}


def load(kind):
    if kind not in _PROBES:
        _PROBES[kind] = Probe(build_probe(kind))
    return _PROBES[kind]


def same_bits(x, y):
    """elementwise: equal bits, or both NaN (see the module docstring)"""
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    return (x.view(np.uint64) == y.view(np.uint64)) | (np.isnan(x) & np.isnan(y))


# ---------------------------------------------------------------------------------------------------------------------
# the high-precision reference (mpmath, 200 bits; inputs converted exactly)
PREC = 200


def _mp():
    try:
        import mpmath
    except ImportError as exc:                      # no skip: without the reference the accuracy claim is unchecked
        raise AssertionError("mpmath is needed for the high-precision reference of og_math.h: %s" % exc)
    mpmath.mp.prec = PREC
    return mpmath


def round_to_double(v):
    """an mpf -> the nearest double (ties to even), subnormals and overflow included; one rounding"""
    sign, man, exp, bc = v._mpf_
    if man == 0:
        return 0.0
    e = exp + bc - 1
    if e > 1023:
        return -INF if sign else INF
    if e < -1076:                                   # below half the smallest subnormal
        return -0.0 if sign else 0.0
    q = max(e - 52, -1074)
    shift = exp - q
    if shift >= 0:
        n = man << shift
    else:
        s = -shift
        n, rem, half = man >> s, man & ((1 << s) - 1), 1 << (s - 1)
        if rem > half or (rem == half and (n & 1)):
            n += 1
    try:
        r = math.ldexp(float(n), q)
    except OverflowError:
        r = INF
    return -r if sign else r


def _truth_one(name):
    """-> f(x: finite non-zero double) -> mpf, or None where the real function is not defined"""
    mp = _mpf = _mp()
    ln2, ln10 = mp.log(2), mp.log(10)
    dom = {"log": lambda x: x > 0, "log2": lambda x: x > 0, "log10": lambda x: x > 0, "log1p": lambda x: x > -1,
           "asin": lambda x: abs(x) <= 1, "acos": lambda x: abs(x) <= 1, "sqrt": lambda x: x > 0}
    fn = {"exp": mp.exp, "log": mp.log, "sin": mp.sin, "cos": mp.cos, "tan": mp.tan, "atan": mp.atan, "asin": mp.asin,
          "acos": mp.acos, "expm1": mp.expm1, "log1p": mp.log1p, "sinh": mp.sinh, "cosh": mp.cosh, "tanh": mp.tanh,
          "log2": lambda x: mp.log(x) / ln2, "log10": lambda x: mp.log(x) / ln10,
          "cbrt": lambda x: mp.sign(x) * mp.cbrt(abs(x)), "sqrt": mp.sqrt, "fabs": abs}[name]
    ok = dom.get(name, lambda x: True)
    del _mpf
    return lambda x: fn(x) if ok(x) else None


# C99 Annex F (F.10) at the arguments a real function has no value for: +0, -0, +inf, -inf (NaN gives NaN everywhere)
ANNEX_F = {
    "exp": (1.0, 1.0, INF, 0.0), "log": (-INF, -INF, INF, NAN), "sin": (0.0, -0.0, NAN, NAN), "cos": (1.0, 1.0, NAN, NAN),
    "tan": (0.0, -0.0, NAN, NAN), "atan": (0.0, -0.0, 1.5707963267948966, -1.5707963267948966),
    "asin": (0.0, -0.0, NAN, NAN), "acos": (1.5707963267948966, 1.5707963267948966, NAN, NAN),
    "expm1": (0.0, -0.0, INF, -1.0), "log1p": (0.0, -0.0, INF, NAN), "sinh": (0.0, -0.0, INF, -INF),
    "cosh": (1.0, 1.0, INF, INF), "tanh": (0.0, -0.0, 1.0, -1.0), "log2": (-INF, -INF, INF, NAN),
    "log10": (-INF, -INF, INF, NAN), "cbrt": (0.0, -0.0, INF, -INF), "sqrt": (0.0, -0.0, INF, NAN),
    "fabs": (0.0, 0.0, INF, INF),
}


class Truth:
    """the true results of one function over its table: ``cr`` the correctly rounded doubles, ``err(got)`` the error
    of an array of results in ulp of ``cr`` (units of 2^-1074 where cr is subnormal or zero; NaN where cr is not finite)"""

    def __init__(self, name, a, b=None):
        mp = _mp()
        self.name, self.a, self.b = name, a, b
        self.exact = [None] * a.size
        self.cr = np.empty(a.size)
        one = _truth_one(name) if b is None else None
        with np.errstate(all="ignore"):
            libm = NUMPY[name](a) if b is None else NUMPY[name](a, b)
        for i in range(a.size):
            x = float(a[i])
            if b is None:
                if x != x:
                    self.cr[i] = NAN
                elif x == 0.0 or abs(x) == INF:
                    self.cr[i] = ANNEX_F[name][(0 if x == 0.0 else 2) + (1 if math.copysign(1.0, x) < 0 else 0)]
                else:
                    v = one(mp.mpf(x))
                    self.exact[i] = v
                    self.cr[i] = NAN if v is None else round_to_double(v)
                    if name == "log1p" and x == -1.0:
                        self.cr[i] = -INF           # the pole (F.10.3.9)
                continue
            y = float(b[i])
            v = self._two(mp, x, y)
            if v is None:       # an operand is 0, inf or NaN (or the power is not real): C99 Annex F, as NumPy's libm has it
                self.cr[i] = libm[i]
            else:
                self.exact[i] = v
                self.cr[i] = round_to_double(v)
                if self.cr[i] == 0.0 and name == "pow" and x < 0 and y == int(y) and int(y) % 2 == 1:
                    self.cr[i] = -0.0
        for i, v in enumerate(self.exact):              # a result that underflows to zero keeps the true result's sign
            if v is not None and self.cr[i] == 0.0 and v < 0:
                self.cr[i] = -0.0

    def _two(self, mp, x, y):
        special = lambda t: t != t or t == 0.0 or abs(t) == INF
        if special(x) or special(y):
            return None
        X, Y = mp.mpf(x), mp.mpf(y)
        if self.name == "atan2":
            return mp.atan2(X, Y)                       # table order: (y, x)
        if self.name == "hypot":
            return mp.sqrt(X * X + Y * Y)
        if x < 0:
            if y != math.floor(y):
                return None
            r = mp.exp(Y * mp.log(-X))
            return -r if int(y) % 2 else r
        return mp.exp(Y * mp.log(X))

    def err(self, got):
        mp = _mp()
        out = np.full(self.a.size, NAN)
        for i, v in enumerate(self.exact):
            if v is None or not np.isfinite(got[i]):
                continue
            cr = self.cr[i]
            unit = 2.0 ** 971 if abs(cr) >= DBL_MAX else float(np.spacing(abs(cr)))
            out[i] = float(abs(mp.mpf(float(got[i])) - v) / mp.mpf(unit))
        return out


def half_up(x):
    """round up to the next half ulp"""
    return math.ceil(2.0 * x - 1e-12) / 2.0


def nan_by_design(name, a):
    """the documented exceptions: trigonometric arguments of magnitude >= 2^45 give NaN (og_math.h, rem_pio2_large)"""
    if name in ("sin", "cos", "tan"):
        return np.abs(a) >= 2.0 ** 45
    return np.zeros(a.size, dtype=bool)


# inputs left out of a comparison, per function, each with its reason (at most 1 % of the function's table)
LEFT_OUT = {}


def pow_scale(a, b):
    """the |y log x| factor of pow_'s allowance (exp(y log x) carries the rounding of its argument)"""
    with np.errstate(all="ignore"):
        s = np.abs(b * np.log(np.abs(a)))
    return np.maximum(1.0, np.where(np.isfinite(s), s, 1.0))


def measure(name, probe):
    """-> dict: inputs, NumPy's and this code's worst error against the truth, the allowance, the bound; and the arrays"""
    a, b = table(name)
    truth = Truth(name, a, b)
    with np.errstate(all="ignore"):
        ref = NUMPY[name](a) if b is None else NUMPY[name](a, b)
    got = probe.host(name, a, b)[0]
    skip = nan_by_design(name, a)
    scale = pow_scale(a, b) if name == "pow" else 1.0
    e_np, e_og = truth.err(ref) / scale, truth.err(got) / scale
    e_np[skip] = NAN
    e_og[skip] = NAN
    worst = lambda e: float(np.nanmax(e)) if np.isfinite(e).any() else 0.0
    allowance = ALLOWANCE[name]
    return dict(name=name, inputs=int(a.size), compared=int(np.isfinite(e_og).sum()), numpy_worst=worst(e_np),
                allowance=allowance, bound=allowance + half_up(worst(e_np)), og_worst=worst(e_og),
                worst_at=(float(a[np.nanargmax(e_og)]) if np.isfinite(e_og).any() else NAN,
                          None if b is None else float(b[np.nanargmax(e_og)])),
                a=a, b=b, got=got, cr=truth.cr, skip=skip, e_og=e_og, numpy=ref)


ACCURACY = ["exp", "log", "sin", "cos", "tan", "atan", "asin", "acos", "expm1", "log1p", "sinh", "cosh", "tanh", "log2",
            "log10", "cbrt", "sqrt", "fabs", "atan2", "hypot", "pow"]


# ---------------------------------------------------------------------------------------------------------------------
# the header's thresholds, found by grep
_FLOAT = re.compile(r"(?<![\w.])(0x[0-9a-fA-F]*\.?[0-9a-fA-F]*p[+-]?\d+|\d+\.\d*(?:[eE][+-]?\d+)?|\d+[eE][+-]?\d+)(?![\w.])")
_HIWORD = re.compile(r"\b(0x[0-9a-fA-F]{8})u\b")
_FUNC = re.compile(r"^OG_HDI?\s+[\w\s\*]+?\b(\w+)\(")


def _conditions(line):
    """the texts of the conditions on a source line: inside `if (...)` / `while (...)`, left of a `?`, and the right-hand
    side of a `bool` flag"""
    out = []
    for m in re.finditer(r"\b(?:if|while)\s*\(", line):
        depth, j = 1, m.end()
        while j < len(line) and depth:
            depth += {"(": 1, ")": -1}.get(line[j], 0)
            j += 1
        out.append(line[m.end():j - 1])
    m = re.search(r"\bbool\s+\w+\s*=(.*);", line)           # a condition kept in a flag: `const bool ybig = ...;`
    if m:
        out.append(m.group(1))
    if "?" in line:
        code = line.split("//")[0]
        pieces = code.split("?")
        for piece in pieces[:-1]:
            out.append(re.split(r"=(?!=)|\breturn\b|:", piece)[-1] if "if" not in piece else "")
    return out


def header_thresholds(path=None):
    """-> list of (function, constant as written, value) for every constant in a condition of og_math.h"""
    found, func = [], None
    with open(path or os.path.join(CSRC, "og_math.h")) as fh:
        for line in fh:
            m = _FUNC.match(line)
            if m:
                func = m.group(1)
            code = line.split("//")[0]
            for cond in _conditions(code):
                for lit in _FLOAT.findall(cond):
                    found.append((func, lit, float.fromhex(lit) if lit.lower().startswith("0x") else float(lit)))
                for lit in _HIWORD.findall(cond):
                    found.append((func, lit + "u", hi(int(lit, 16))))
    return found


def unknown_thresholds(path=None):
    """the constants in conditions of the header that the table of the function they stand in does not hold"""
    missing = []
    for func, lit, value in header_thresholds(path):
        if value in NOT_A_THRESHOLD:
            continue
        owners = OWNER.get(func, [func[:-1] if func.endswith("_") else func])
        for owner in owners:
            known = set(abs(float(v)) for v in THRESHOLDS.get(owner, []))
            if abs(value) not in known:
                missing.append((func, lit, owner))
    return missing


# ---------------------------------------------------------------------------------------------------------------------
# the dual rules at smooth points: name -> (domain, sample(rng), the textbook derivative in float64 with NumPy's own
# functions, the same in mpmath, allowance in ulp: those of the og_math functions the rule calls, each times the factor
# by which the rule's formula carries a relative error of that function into the derivative)
def _dual_smooth():
    mp = _mp()
    n = 4000
    logu = lambda r, lo, hi_: np.exp(r.uniform(np.log(lo), np.log(hi_), n))
    pm = lambda r, v: v * np.where(r.uniform(-1, 1, v.size) < 0, -1.0, 1.0)
    return {
        "sqrt": ("[1e-300, 1e300]", lambda r: logu(r, 1e-300, 1e300), lambda x: 1.0 / (2.0 * np.sqrt(x)),
                 lambda x: 1 / (2 * mp.sqrt(x)), 0.0),
        "exp": ("[-700, 700]", lambda r: r.uniform(-700, 700, n), np.exp, mp.exp, 1.0),
        "log": ("+-[1e-300, 1e300] (x > 0)", lambda r: logu(r, 1e-300, 1e300), lambda x: 1.0 / x, lambda x: 1 / x, 0.0),
        "sin": ("[-100, 100]", lambda r: r.uniform(-100, 100, n), np.cos, mp.cos, 1.0),
        "cos": ("[-100, 100]", lambda r: r.uniform(-100, 100, n), lambda x: -np.sin(x), lambda x: -mp.sin(x), 1.0),
        "tan": ("[-1.5, 1.5]", lambda r: r.uniform(-1.5, 1.5, n), lambda x: 1.0 + np.tan(x) ** 2,
                lambda x: 1 + mp.tan(x) ** 2, 2 * 2.0),
        "atan": ("+-[1e-10, 1e10]", lambda r: pm(r, logu(r, 1e-10, 1e10)), lambda x: 1.0 / (1.0 + x * x),
                 lambda x: 1 / (1 + x * x), 0.0),
        "asin": ("[-0.9, 0.9]", lambda r: r.uniform(-0.9, 0.9, n), lambda x: 1.0 / np.sqrt(1.0 - x * x),
                 lambda x: 1 / mp.sqrt(1 - x * x), 0.0),
        "acos": ("[-0.9, 0.9]", lambda r: r.uniform(-0.9, 0.9, n), lambda x: -(1.0 / np.sqrt(1.0 - x * x)),
                 lambda x: -1 / mp.sqrt(1 - x * x), 0.0),
        "tanh": ("[-0.5, 0.5]", lambda r: r.uniform(-0.5, 0.5, n), lambda x: 1.0 - np.tanh(x) ** 2,
                 lambda x: 1 - mp.tanh(x) ** 2, 3 * 2.0),
        "sinh": ("+-[1e-5, 700]", lambda r: pm(r, logu(r, 1e-5, 700)), np.cosh, mp.cosh, 2.0),
        "cosh": ("+-[1e-5, 700]", lambda r: pm(r, logu(r, 1e-5, 700)), np.sinh, mp.sinh, 3.0),
        "expm1": ("[-40, 700]", lambda r: r.uniform(-40, 700, n), np.exp, mp.exp, 1.0),
        "log1p": ("(-1, 1e300]", lambda r: np.concatenate([logu(r, 1e-300, 1e300)[:n // 2], -logu(r, 1e-300, 0.999)[:n // 2]]),
                  lambda x: 1.0 / (1.0 + x), lambda x: 1 / (1 + x), 0.0),
        "log2": ("[1e-300, 1e300]", lambda r: logu(r, 1e-300, 1e300), lambda x: 1.0 / (x * np.log(2.0)),
                 lambda x: 1 / (x * mp.log(2)), 0.0),
        "log10": ("[1e-300, 1e300]", lambda r: logu(r, 1e-300, 1e300), lambda x: 1.0 / (x * np.log(10.0)),
                  lambda x: 1 / (x * mp.log(10)), 0.0),
        "cbrt": ("+-[1e-150, 1e150]", lambda r: pm(r, logu(r, 1e-150, 1e150)), lambda x: 1.0 / (3.0 * np.cbrt(x) ** 2),
                 lambda x: 1 / (3 * mp.cbrt(abs(x)) ** 2), 2 * 1.0),
        "fabs": ("+-[1e-300, 1e300]", lambda r: pm(r, logu(r, 1e-300, 1e300)), np.sign, mp.sign, 0.0),
    }


def measure_dual(name, probe):
    """the derivative part of rule ``name`` at smooth points, seed 1 -> worst relative error in ulp of this code and of
    the float64 formula, and the bound built from the latter"""
    mp = _mp()
    domain, sample, f64, exact, allowance = _dual_smooth()[name]
    x = sample(np.random.default_rng(21))
    got = probe.host(name, x, da=np.ones(x.size), variant=1)[1]
    with np.errstate(all="ignore"):
        ref = f64(x)
    e_og, e_np = np.empty(x.size), np.empty(x.size)
    for i in range(x.size):
        v = exact(mp.mpf(float(x[i])))
        unit = mp.mpf(float(np.spacing(abs(round_to_double(mp.mpf(v))))))
        e_og[i] = float(abs(mp.mpf(float(got[i])) - v) / unit)
        e_np[i] = float(abs(mp.mpf(float(ref[i])) - v) / unit)
    return dict(name=name, domain=domain, inputs=int(x.size), numpy_worst=float(e_np.max()), allowance=allowance,
                bound=allowance + half_up(float(e_np.max())), og_worst=float(e_og.max()), x=x, got=got)


# ---------------------------------------------------------------------------------------------------------------------
def report(path):
    probe = load("gxx")
    lines = ["# og_math.h / og_dual.h at their branches and edges: what the host build measures",
             "",
             "Written by `python tests/og_math_cases.py --report` (the g++ build of `tests/og_math_probe.hip` against",
             "mpmath at %d bits, NumPy %s).  The table of inputs is `tests/og_math_cases.py`; the assertions are" % (PREC, np.__version__),
             "`tests/test_og_math_edges.py`.  Errors are in ulp of the correctly rounded result (units of 2^-1074 where it is",
             "subnormal).  **bound = allowance + NumPy's worst error on the same inputs, rounded up to the next half ulp**: the",
             "allowance is what `tests/test_og_math.py` asserts against NumPy; nothing in the bound comes from `og_math.h`.",
             "`pow`: every figure is divided by max(1, |y log x|), the documented scale of its allowance.",
             "Everything here is measured on the host; the device is compared with the host bit for bit",
             "(`tests/test_og_math_gpu.py`), so it inherits these figures where that test counts 0 differences.",
             "",
             "## Values",
             "",
             "| function | inputs | compared | NumPy worst | allowance | bound | og_math worst | at |",
             "|---|---|---|---|---|---|---|---|"]
    for name in ACCURACY:
        m = measure(name, probe)
        at = "%r" % m["worst_at"][0] if m["worst_at"][1] is None else "(%r, %r)" % m["worst_at"]
        lines.append("| %s | %d | %d | %.3f | %g | %g | %.3f | %s |" % (
            name, m["inputs"], m["compared"], m["numpy_worst"], m["allowance"], m["bound"], m["og_worst"], at))
    lines += ["",
              "`compared` counts the inputs with a finite true result; at the others (poles, arguments outside the domain,",
              "NaN, overflow) the finite / infinite / NaN pattern and the sign of zero are asserted equal to the correctly",
              "rounded result's.  The only inputs answered differently by design: |x| >= 2^45 for `sin cos tan` (NaN, asserted).",
              "`mod fmod floor trunc scalb interp`: exact operations, asserted bit for bit against NumPy / SciPy.",
              "",
              "## Dual rules at smooth points (seed d = 1)",
              "",
              "Relative error of the derivative part against the textbook derivative in mpmath.  `float64 worst` is the same",
              "formula evaluated with NumPy's functions on the same inputs; the allowance is that of the og_math functions the",
              "rule calls, times the factor by which the formula carries their relative error (t^2 doubles it).",
              "",
              "| rule | domain | inputs | float64 worst | allowance | bound | og_dual worst |",
              "|---|---|---|---|---|---|---|"]
    for name in _dual_smooth():
        m = measure_dual(name, probe)
        lines.append("| %s | %s | %d | %.3f | %g | %g | %.3f |" % (
            name, m["domain"], m["inputs"], m["numpy_worst"], m["allowance"], m["bound"], m["og_worst"]))
    lines += ["",
              "Ill-conditioned by construction, sampled apart and judged by the absolute error of the factor: `1 - t*t` of",
              "tanh for 0.5 <= |x| < 22 (bound: float64's error on the same inputs + 6 * 2^-53, what 3 ulp of t <= 1 move",
              "t*t by), `1 - v*v` of asin / acos for 0.9 < |v| < 1 (bound: float64's error on the same inputs).",
              "",
              "## Device",
              "",
              "Nothing above was measured on a GPU.  `tests/test_og_math_gpu.py` counts the results whose bits differ between",
              "gfx950 and this host build (expected: 0) and records the count per function through",
              "`conftest.record_measurement`; no count of a device run is recorded in this file yet.",
              ""]
    with open(path, "w") as fh:
        fh.write("\n".join(lines))


PINS = os.path.join(ROOT, "tests", "golden", "og_math_bits.json")


def bit_digests(probe):
    """label -> SHA-256 of the bits of the results (values, then derivatives; every NaN as 0x7ff8000000000000) over the
    case table and the shared random distributions.  tests/golden/og_math_bits.json holds those of the host build: a
    change of og_math.h / og_dual.h that moves a single result bit anywhere on the table shows, even inside the bounds
    (rewrite the file with --pin when the change is meant)."""
    import hashlib

    def digest(v, d):
        both = np.concatenate([v, d]).copy()
        both[np.isnan(both)] = NAN
        return hashlib.sha256(both.view(np.uint64).tobytes()).hexdigest()[:24]
    out = {}
    for label, name, variant, a, b, da, db, tab in all_cases():
        out[label] = digest(*probe.host(name, a, b, da, db, variant, tab))
    for name in FUNCS:
        for k, (a, b) in enumerate(random_inputs(name)):
            out["%s random %d" % (name, k)] = digest(*probe.host(name, a, b))
    return out


if __name__ == "__main__":
    if "--report" in sys.argv:
        report(os.path.join(ROOT, "profiles", "og_math_edges.md"))
    elif "--pin" in sys.argv:
        import json
        with open(PINS, "w") as fh:
            json.dump(bit_digests(load("gxx")), fh, indent=0, sort_keys=True)
            fh.write("\n")
    else:
        print(__doc__)
