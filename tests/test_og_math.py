"""csrc/og_math.h on the host (g++): accuracy against NumPy on random samples, and special values.  The branch
thresholds, the exponent range and og_dual.h are checked against mpmath in tests/test_og_math_edges.py; the same source
is compiled for gfx950, and bit-equality host<->device is checked on the GPU over that table and these samples by
tests/test_og_math_gpu.py (and, for eight functions with timings, by tools/gpu_probe.hip:
tests/test_gpu_parity.py::test_hardware_probe)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
# the random distributions live next to the case table of the edge tests (tests/og_math_cases.py), which the GPU tests
# run too: shared, so that the two cannot drift
from og_math_cases import RANDOM_BASIC, RANDOM_WIDENED, random_atan2, random_hypot, random_mod, random_pow

SRC = r"""
#include "og_math.h"
extern "C" {
void v_exp(const double* x, double* y, int n) { for (int i = 0; i < n; ++i) y[i] = ogm::exp_(x[i]); }
void v_log(const double* x, double* y, int n) { for (int i = 0; i < n; ++i) y[i] = ogm::log_(x[i]); }
void v_sin(const double* x, double* y, int n) { for (int i = 0; i < n; ++i) y[i] = ogm::sin_(x[i]); }
void v_cos(const double* x, double* y, int n) { for (int i = 0; i < n; ++i) y[i] = ogm::cos_(x[i]); }
void v_tan(const double* x, double* y, int n) { for (int i = 0; i < n; ++i) y[i] = ogm::tan_(x[i]); }
void v_atan(const double* x, double* y, int n) { for (int i = 0; i < n; ++i) y[i] = ogm::atan_(x[i]); }
void v_asin(const double* x, double* y, int n) { for (int i = 0; i < n; ++i) y[i] = ogm::asin_(x[i]); }
void v_acos(const double* x, double* y, int n) { for (int i = 0; i < n; ++i) y[i] = ogm::acos_(x[i]); }
void v_atan2(const double* yy, const double* xx, double* o, int n) { for (int i = 0; i < n; ++i) o[i] = ogm::atan2_(yy[i], xx[i]); }
#define V1(f) void v_##f(const double* x, double* y, int n) { for (int i = 0; i < n; ++i) y[i] = ogm::f##_(x[i]); }
V1(expm1) V1(log1p) V1(sinh) V1(cosh) V1(tanh) V1(log2) V1(log10) V1(cbrt)
void v_hypot(const double* a, const double* b, double* o, int n) { for (int i = 0; i < n; ++i) o[i] = ogm::hypot_(a[i], b[i]); }
void v_pow(const double* a, const double* b, double* o, int n) { for (int i = 0; i < n; ++i) o[i] = ogm::pow_(a[i], b[i]); }
void v_mod(const double* a, const double* b, double* o, int n) { for (int i = 0; i < n; ++i) o[i] = ogm::mod_(a[i], b[i]); }
void v_fmod(const double* a, const double* b, double* o, int n) { for (int i = 0; i < n; ++i) o[i] = ogm::fmod_(a[i], b[i]); }
}
"""


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    d = tmp_path_factory.mktemp("ogmath")
    src = d / "m.cpp"
    src.write_text(SRC)
    so = d / "m.so"
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-mfma", "-fPIC", "-shared",
                           "-I" + os.path.join(ROOT, "opengoddard_amd", "csrc"), str(src), "-o", str(so)])
    return C.CDLL(str(so))


def call(lib, name, x):
    x = np.ascontiguousarray(x, dtype=np.float64)
    y = np.empty_like(x)
    dp = C.POINTER(C.c_double)
    getattr(lib, name)(x.ctypes.data_as(dp), y.ctypes.data_as(dp), x.size)
    return y


def ulps(a, b):
    return np.abs(a - b) / np.spacing(np.abs(b))


@pytest.mark.parametrize("name,ref,sample,tol", [("v_" + n, ref, sample, tol) for n, ref, sample, tol in RANDOM_BASIC])
def test_within_one_ulp_of_numpy(lib, name, ref, sample, tol):
    x = sample(np.random.default_rng(0))
    got, want = call(lib, name, x), ref(x)
    assert np.max(ulps(got, want)) <= tol


def test_atan2_within_one_ulp_and_special_values(lib):
    y, x = random_atan2()
    yy, xx = np.ascontiguousarray(y), np.ascontiguousarray(x)
    out = np.empty_like(yy)
    dp = C.POINTER(C.c_double)
    lib.v_atan2(yy.ctypes.data_as(dp), xx.ctypes.data_as(dp), out.ctypes.data_as(dp), yy.size)
    assert np.max(ulps(out, np.arctan2(y, x))) <= 1.0
    inf, nan = np.inf, np.nan
    ys = np.array([0.0, -0.0, 0.0, -0.0, 1.0, -1.0, inf, -inf, inf, 1.0, -1.0, 1.0, nan, 1.0, 3.0])
    xs = np.array([1.0, 1.0, -1.0, -1.0, 0.0, 0.0, inf, inf, -inf, inf, -inf, -inf, 1.0, nan, 1.0])
    out = np.empty_like(ys)
    lib.v_atan2(ys.ctypes.data_as(dp), xs.ctypes.data_as(dp), out.ctypes.data_as(dp), ys.size)
    want = np.arctan2(ys, xs)
    assert np.array_equal(np.isnan(out), np.isnan(want))
    ok = ~np.isnan(want)
    assert np.max(ulps(out[ok][want[ok] != 0], want[ok][want[ok] != 0])) <= 1.0
    assert np.array_equal(out[ok][want[ok] == 0], want[ok][want[ok] == 0])
    assert np.array_equal(np.signbit(out[ok]), np.signbit(want[ok]))
    edge = call(lib, "v_asin", [1.0, -1.0, 0.0, 1.5, 1e-300])
    assert ulps(edge[:2], np.arcsin([1.0, -1.0])).max() <= 1.0 and edge[2] == 0.0 and np.isnan(edge[3])
    assert edge[4] == 1e-300
    edge = call(lib, "v_acos", [1.0, -1.0, 0.0, -1.5])
    assert edge[0] == 0.0 and ulps(edge[1:3], np.arccos([-1.0, 0.0])).max() <= 1.0 and np.isnan(edge[3])
    big = call(lib, "v_atan", [inf, -inf, 1e300, -1e300, 0.0, -0.0])
    assert ulps(big[:4], np.arctan([inf, -inf, 1e300, -1e300])).max() <= 1.0
    assert big[4] == 0.0 and np.signbit(big[5])


def test_special_values(lib):
    inf, nan = np.inf, np.nan
    e = call(lib, "v_exp", [0.0, -0.0, inf, -inf, nan, 710.0, -746.0, 1e-300, 709.78, -745.0])
    assert e[0] == 1.0 and e[1] == 1.0 and e[2] == inf and e[3] == 0.0 and np.isnan(e[4])
    assert e[5] == inf and e[6] == 0.0 and e[7] == 1.0
    assert ulps(e[8:], np.exp([709.78, -745.0])).max() <= 1.0          # near overflow / subnormal
    lg = call(lib, "v_log", [1.0, 0.0, -0.0, -1.0, inf, nan, 5e-324, 2.2250738585072014e-308])
    assert lg[0] == 0.0 and lg[1] == -inf and lg[2] == -inf and np.isnan(lg[3]) and lg[4] == inf
    assert np.isnan(lg[5])
    assert ulps(lg[6:], np.log([5e-324, 2.2250738585072014e-308])).max() <= 1.0
    for name in ("v_sin", "v_cos", "v_tan"):
        v = call(lib, name, [inf, -inf, nan])
        assert np.isnan(v).all()
    s = call(lib, "v_sin", [0.0, -0.0, 1e-300])
    assert s[0] == 0.0 and np.signbit(s[1]) and s[2] == 1e-300
    assert call(lib, "v_cos", [0.0, 1e-300]).tolist() == [1.0, 1.0]


def test_trig_of_absurd_angles_is_nan_not_noise(lib):
    """Above 2^45 the argument reduction gives up: NaN (caught by the engine's non-finite detection), never a
    value outside [-1, 1]; the cast that used to be undefined behaviour above 9.2e18 is not reached."""
    x = np.array([3.6e13, 1e17, -1e17, 9.3e18, 1e300, -1e305, np.inf, -np.inf, np.nan])
    for name in ("v_sin", "v_cos", "v_tan"):
        assert np.isnan(call(lib, name, x)).all(), name
    near = np.array([3.5184e13, -3.5184e13, 1.7e6, -1.7e6, 1647098.9, 1647099.1])
    for name, ref in (("v_sin", np.sin), ("v_cos", np.cos)):
        y = call(lib, name, near)
        assert np.all(np.abs(y) <= 1.0) and np.all(ulps(y, ref(near)) <= 1.0)


def call2(lib, name, a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    y = np.empty_like(a)
    dp = C.POINTER(C.c_double)
    getattr(lib, name)(a.ctypes.data_as(dp), b.ctypes.data_as(dp), y.ctypes.data_as(dp), a.size)
    return y


@pytest.mark.parametrize("name,ref,sample,tol", [("v_" + n, ref, sample, tol) for n, ref, sample, tol in RANDOM_WIDENED])
def test_widened_function_set_within_a_few_ulp_of_numpy(lib, name, ref, sample, tol):
    """The functions the tracer gained in round 3 (tanh, sinh, cosh, log10, log2, log1p, expm1, cbrt): composed of
    exp_ / log_ with classical correction steps - 1 ulp for log2 / log10 / cbrt on these samples (log10: 2 over the whole
    exponent range, profiles/og_math_edges.md), 2 for cosh / log1p, 3 for the expm1
    family (one rounded exp, two rounded products); bit-reproducible on the GPU for the same reason exp_ / log_ are."""
    x = sample(np.random.default_rng(0))
    with np.errstate(all="ignore"):
        got, want = call(lib, name, x), ref(x)
    assert np.array_equal(np.isfinite(got), np.isfinite(want))
    ok = np.isfinite(want) & (want != 0)
    assert np.max(ulps(got[ok], want[ok])) <= tol


def test_hypot_pow_and_special_values_of_the_widened_set(lib):
    r, (a, b), (_, b2) = random_hypot()
    assert np.max(ulps(call2(lib, "v_hypot", a, b), np.hypot(a, b))) <= 1.0
    assert np.max(ulps(call2(lib, "v_hypot", a, b2), np.hypot(a, b2))) <= 1.0
    # traced exponents: exp(y log x) - |y log x| ulp from libm's pow at worst (documented in og_math.h)
    x, y = random_pow(r)
    assert np.max(ulps(call2(lib, "v_pow", x, y), np.power(x, y)) / np.maximum(1.0, np.abs(y * np.log(x)))) <= 3.0
    with np.errstate(all="ignore"):
        xs = np.array([0.0, -0.0, 0.0, -8.0, -8.0, 2.0, -2.0, 1.0, 5.0, np.nan, 0.5, -2.0, -0.5, -1.0, -np.inf, -np.inf,
                       -1.0, -3.0])
        ys = np.array([2.0, 3.0, -1.0, 3.0, 0.5, 0.0, 2.0, np.nan, -np.inf, 0.0, np.inf, 1e16, 1e300, 1e300, 0.5, -0.5,
                       np.inf, 2.0 ** 53 - 1.0])
        got, want = call2(lib, "v_pow", xs, ys), np.power(xs, ys)
    assert np.array_equal(np.isnan(got), np.isnan(want))
    plain = np.isfinite(want) & (want != 0)
    assert np.array_equal(got[~np.isnan(want) & ~plain], want[~np.isnan(want) & ~plain])       # zeros, infinities
    assert np.max(ulps(got[plain], want[plain])) <= 4.0                                        # (-8) ** 3 = -512 to rounding
    assert np.array_equal(call(lib, "v_log2", 2.0 ** np.arange(-1070, 1020)), np.arange(-1070.0, 1020.0))   # exact
    inf, nan = np.inf, np.nan
    t = call(lib, "v_tanh", [0.0, -0.0, inf, -inf, nan, 1e-300, 40.0])
    assert t[0] == 0.0 and np.signbit(t[1]) and t[2] == 1.0 and t[3] == -1.0 and np.isnan(t[4]) and t[5] == 1e-300 and t[6] == 1.0
    c = call(lib, "v_cbrt", [0.0, -0.0, inf, -inf, -8.0, 27.0, nan])
    assert c[0] == 0.0 and np.signbit(c[1]) and c[2] == inf and c[3] == -inf and c[4] == -2.0 and c[5] == 3.0 and np.isnan(c[6])
    l = call(lib, "v_log1p", [-1.0, -2.0, 0.0, inf, 1e-300])
    assert l[0] == -inf and np.isnan(l[1]) and l[2] == 0.0 and l[3] == inf and l[4] == 1e-300
    e = call(lib, "v_expm1", [0.0, -inf, inf, 710.0, -800.0])
    assert e[0] == 0.0 and e[1] == -1.0 and e[2] == inf and e[3] == inf and e[4] == -1.0
    assert call(lib, "v_cosh", [0.0, 800.0, -800.0]).tolist() == [1.0, inf, inf]
    assert call(lib, "v_sinh", [800.0, -800.0]).tolist() == [inf, -inf]
    assert call2(lib, "v_hypot", [inf, nan, 0.0, 3.0], [nan, 1.0, 0.0, 4.0]).tolist()[::3] == [inf, 5.0]


def test_mod_and_fmod_are_numpys_bit_for_bit(lib):
    """np.remainder (= np.mod, Python's %: the divisor's sign) and np.fmod (the dividend's sign) are exact operations:
    the device functions must give NumPy's bits, signed zeros and special values included."""
    a, b = random_mod()
    for name, ref in (("v_mod", np.remainder), ("v_fmod", np.fmod)):
        assert np.array_equal(call2(lib, name, a, b), ref(a, b))
        assert np.array_equal(call2(lib, name, np.round(a), np.round(b) + (np.round(b) == 0)),
                              ref(np.round(a), np.round(b) + (np.round(b) == 0)))
    inf, nan = np.inf, np.nan
    aa = np.array([6.0, -6.0, 6.0, -6.0, 0.0, -0.0, 5.0, 5.0, inf, 5.0, -5.0, nan, 1.0, 7.5, -7.5])
    bb = np.array([3.0, 3.0, -3.0, -3.0, 2.0, 2.0, 0.0, -0.0, 2.0, inf, inf, 1.0, nan, -2.0, 2.0])
    with np.errstate(all="ignore"):
        for name, ref in (("v_mod", np.remainder), ("v_fmod", np.fmod)):
            got, want = call2(lib, name, aa, bb), ref(aa, bb)
            assert np.array_equal(got, want, equal_nan=True)
            assert np.array_equal(np.signbit(got), np.signbit(want)) or np.array_equal(
                np.signbit(got[~np.isnan(want)]), np.signbit(want[~np.isnan(want)]))
