"""csrc/og_math.h and csrc/og_dual.h on the host, at every branch threshold, over the whole exponent range and at the
special values, against mpmath at 200 bits (the case table: tests/og_math_cases.py).  The device is compared with this
host build bit for bit in tests/test_og_math_gpu.py, which gives it these results.

The bound of a function is not fixed in advance: it is the allowance tests/test_og_math.py asserts for it against
NumPy plus NumPy's own worst error against mpmath on the very same inputs, rounded up to the next half ulp.  The
figures of one run are in profiles/og_math_edges.md."""
import ctypes as C
import os

import numpy as np
import pytest

import og_math_cases as cases
from og_math_cases import INF, NAN, same_bits


@pytest.fixture(scope="module")
def probe():
    return cases.load("gxx")


# ---------------------------------------------------------------------------------------------------------------------
def test_the_table_knows_every_threshold_of_the_header(tmp_path):
    """Every floating literal and high-word cut in a condition of og_math.h is a threshold of the table of the
    function it stands in (or is named as not being one); a threshold added to the source alone is caught."""
    found = cases.header_thresholds()
    assert len(found) >= 70
    assert ("atan_", "0x3fdc0000u", 0.4375) in found and ("cbrt_", "0x1p-700", 2.0 ** -700) in found
    assert ("pow_", "9007199254740992.0", 2.0 ** 53) in found and ("kcos", "0.78125", 0.78125) in found
    assert cases.unknown_thresholds() == []
    with open(os.path.join(cases.CSRC, "og_math.h")) as fh:
        text = fh.read()
    changed = tmp_path / "og_math.h"
    changed.write_text(text.replace("    if (ax < 22.0) {\n        const double e = exp_(ax);",
                                    "    if (ax < 0.125) return x;\n    if (ax < 22.0) {\n        const double e = exp_(ax);")
                       .replace("if (ix < 0x3fe60000u) { id = 0;", "if (ix < 0x3fe70000u) { id = 0;"))
    assert sorted(cases.unknown_thresholds(str(changed))) == [("atan_", "0x3fe70000u", "atan"), ("sinh_", "0.125", "sinh")]


def test_the_table_holds_what_it_promises():
    es = cases.sweep_exponents()
    assert set(range(-1074, -1010)) <= set(es) and set(range(960, 1024)) <= set(es)
    assert np.max(np.diff(es)) <= 8
    for name in cases.ONE_ARG:
        a, _ = cases.table(name)
        for s in cases.SPECIALS:
            assert same_bits(a, s).any(), (name, s)
        for t in cases.THRESHOLDS.get(name, []):
            for v in (t, np.nextafter(t, INF), np.nextafter(t, -INF), -t):
                assert (a == v).any(), (name, v)
        for e in (-1074, -1022, 0, 1023):
            for m in (1.0, 1.5):
                v = np.ldexp(m, e)
                assert (a == v).any() and (a == -v).any(), (name, e, m)
    for name in cases.TWO_ARG:
        a, b = cases.table(name)
        assert a.size == b.size >= 1024
        for s in (0.0, -0.0, INF, -INF, NAN, cases.DENORM_MIN, cases.DBL_MAX):
            for t in (-0.0, INF, NAN, cases.DBL_MIN, -1.0):
                assert (same_bits(a, s) & same_bits(b, t)).any(), (name, s, t)
    x = cases.table("sin")[0]
    assert ((np.abs(x) > 1.6e6) & (np.abs(x) < 2.0 ** 45)).sum() >= 5000
    assert (x == 2.0 ** 45).any() and (x == np.nextafter(2.0 ** 45, 0)).any() and (x == np.nextafter(2.0 ** 45, INF)).any()
    # the same object on every machine: seeded
    cases._TABLES.pop("sin")
    assert same_bits(cases.table("sin")[0], x).all()


# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", cases.ACCURACY)
def test_values_against_mpmath(probe, name):
    """Error in ulp of the correctly rounded result at every input of the table; the finite / infinite / NaN pattern
    and the sign of zero are the correctly rounded result's.  bound = allowance + NumPy's worst error on these inputs."""
    m = cases.measure(name, probe)
    got, cr, skip = m["got"], m["cr"], m["skip"]
    print("%s: %d inputs, %d compared, NumPy worst %.3f ulp, allowance %g, bound %g, og_math worst %.3f ulp at %r" % (
        name, m["inputs"], m["compared"], m["numpy_worst"], m["allowance"], m["bound"], m["og_worst"], m["worst_at"]))
    # the documented exception, asserted: trigonometric arguments of magnitude >= 2^45 give NaN
    assert np.isnan(got[skip]).all()
    # anything else left out of the comparison is named in the helper with its reason: at most 1 % (today: nothing)
    left_out = cases.LEFT_OUT.get(name, np.zeros(skip.size, dtype=bool))
    assert left_out.sum() <= 0.01 * m["inputs"], "%d of %d inputs left out" % (left_out.sum(), m["inputs"])
    keep = ~(left_out | skip)

    def show(mask):
        idx = np.flatnonzero(mask)[:8]
        return [(m["a"][i], None if m["b"] is None else m["b"][i], got[i], cr[i]) for i in idx]
    bad = keep & (np.isnan(got) != np.isnan(cr))
    assert not bad.any(), "NaN pattern differs (input, input, got, correctly rounded): %r" % show(bad)
    bad = keep & (np.isinf(got) != np.isinf(cr))
    assert not bad.any(), "infinite where the true result is finite, or the reverse: %r" % show(bad)
    bad = keep & ~np.isnan(cr) & (np.signbit(got) != np.signbit(cr))
    assert not bad.any(), "sign (of zero) differs: %r" % show(bad)
    assert m["compared"] >= 0.45 * m["inputs"]
    bad = keep & (m["e_og"] > m["bound"])
    assert not bad.any(), "beyond %g ulp: %r" % (m["bound"], show(bad))
    if name in ("sqrt", "fabs"):                                    # correctly rounded operations: the bits
        assert same_bits(got, cr).all()


def test_cbrt_and_pow_where_they_were_wrong(probe):
    """cbrt_ was NaN for x >= 2^802 and hundreds of ulp off below 2^-770; pow_ was NaN for a negative base with a whole
    exponent >= 9e15 and for (-inf) ** (a non-integer), and 0 where x ** -k is a subnormal number."""
    e = np.arange(-1074, 1024)
    x = np.ldexp(1.0, e)
    got = probe.host("cbrt", x)[0]
    third = e % 3 == 0
    assert same_bits(got[third], np.ldexp(1.0, e[third] // 3)).all()            # exact cubes
    assert np.all(np.abs(got - np.cbrt(x)) <= np.spacing(np.cbrt(x)))
    assert same_bits(probe.host("cbrt", [cases.DBL_MAX, -cases.DBL_MAX, cases.DENORM_MIN])[0],
                     [5.643803094122362e+102, -5.643803094122362e+102, np.cbrt(cases.DENORM_MIN)]).all()
    xs = [-2.0, -0.5, -1.0, -2.0, -INF, -INF, -INF, -INF, -1.0, -1.0, 8.958978968711216e+102, -3.0, -3.0]
    ys = [1e16, 1e300, 1e300, -1e16, 0.5, -0.5, 3.0, -3.0, INF, -INF, -3.0, 2.0 ** 53 - 1.0, 9.0e15 + 1.0]
    want = [INF, 0.0, 1.0, 0.0, INF, 0.0, -INF, -0.0, 1.0, 1.0, 1.390671161567e-309, -INF, -INF]
    got = probe.host("pow", xs, ys)[0]
    with np.errstate(all="ignore"):
        ref = np.power(xs, ys)
    assert same_bits(want[:10] + want[11:], np.delete(ref, 10)).all() and abs(ref[10] - want[10]) <= 1e-321
    assert same_bits(got[:10], want[:10]).all() and same_bits(got[11:], want[11:]).all(), got
    assert abs(got[10] - want[10]) <= 800 * 5e-324             # 3 |y log x| = 711 units of 2^-1074: a subnormal number, not 0
    a, b = [g.ravel() for g in np.meshgrid(cases.GRID, cases.GRID, indexing="ij")]
    with np.errstate(all="ignore"):
        want = np.power(a, b)
    got = probe.host("pow", a, b)[0]
    special = ~np.isfinite(want) | (want == 0) | ~np.isfinite(a) | ~np.isfinite(b) | (a == 0) | (b == 0)
    assert same_bits(got[special], want[special]).all(), "pow_'s special cases are not NumPy's on the 32 x 32 grid"


def test_exact_operations_have_numpys_bits(probe):
    """mod_ fmod_ floor_ trunc_ are exact operations: NumPy's bits at every input of their tables; scalb_ is ldexp
    wherever the result is not subnormal (there it may round twice: within one unit of 2^-1074)."""
    for name in ("floor", "trunc"):
        a, _ = cases.table(name)
        assert same_bits(probe.host(name, a)[0], cases.NUMPY[name](a)).all(), name
    for name in ("mod", "fmod"):
        a, b = cases.table(name)
        with np.errstate(all="ignore"):
            want = cases.NUMPY[name](a, b)
        got = probe.host(name, a, b)[0]
        bad = ~same_bits(got, want)
        assert not bad.any(), (name, a[bad][:5], b[bad][:5], got[bad][:5], want[bad][:5])
    a, k = cases.table("scalb")
    with np.errstate(all="ignore"):
        want = np.ldexp(a, k.astype(np.int64))
    got = probe.host("scalb", a, k)[0]
    sub = np.isfinite(want) & (np.abs(want) < cases.DBL_MIN) & (want != 0) | (np.isfinite(a) & (a != 0) & (want == 0))
    assert same_bits(got[~sub], want[~sub]).all()
    assert np.all(np.abs(got[sub] - want[sub]) <= 5e-324) and np.array_equal(np.signbit(got[sub]), np.signbit(want[sub]))


def _interp_numpy(xg, yg, x, mode, fills):
    """the formula of scipy.interpolate.interp1d(kind="linear"), restated"""
    with np.errstate(all="ignore"):
        i = np.clip(np.searchsorted(xg, x, "left"), 1, xg.size - 1)
        y = (yg[i] - yg[i - 1]) / (xg[i] - xg[i - 1]) * (x - xg[i - 1]) + yg[i - 1]
    if mode != 1:
        y = np.where(x == xg[i], yg[i], y)                      # np.interp, which SciPy calls in these two modes
        y = np.where(x < xg[0], fills[0] if mode == 0 else NAN, np.where(x > xg[-1], fills[1] if mode == 0 else NAN, y))
    return y


def _interp_scipy(xg, yg, x, mode, fills):
    from scipy.interpolate import interp1d
    with np.errstate(all="ignore"):
        if mode == 0:
            return interp1d(xg, yg, kind="linear", bounds_error=False, fill_value=fills)(x)
        if mode == 1:
            return interp1d(xg, yg, kind="linear", fill_value="extrapolate")(x)
        f = interp1d(xg, yg, kind="linear", bounds_error=True)
        out = np.empty(x.size)
        for i, v in enumerate(x):
            try:
                out[i] = f(v)
            except ValueError:
                out[i] = NAN                                     # a kernel cannot raise
        return out


def test_interp_linear_has_scipys_bits_and_the_promised_slopes(probe):
    for label, xg, yg in cases.interp_tables():
        x = cases.interp_queries(xg)
        n = xg.size
        for mode in (0, 1, 2):
            v, d = probe.host("interp", x, da=np.full(x.size, 2.0), variant=1, tab=(xg, yg, mode))
            plain = probe.host("interp", x, tab=(xg, yg, mode))[0]
            for ref in (_interp_scipy, _interp_numpy):
                want = ref(xg, yg, x, mode, cases.FILLS)
                bad = ~same_bits(plain, want)
                assert not bad.any(), (label, mode, ref.__name__, x[bad][:5], plain[bad][:5], want[bad][:5])
            assert same_bits(v, plain).all(), (label, mode)
            # the slope of the segment to the right at a knot, 0 on the constant fills, the end segments' when extrapolating
            seg = np.clip(np.searchsorted(xg, x, "right"), 1, n - 1)
            slope = (yg[seg] - yg[seg - 1]) / (xg[seg] - xg[seg - 1])
            if mode != 1:
                slope = np.where((x < xg[0]) | (x > xg[-1]), 0.0, slope)
            ok = ~np.isnan(x)
            assert same_bits(d[ok], (slope * 2.0)[ok]).all(), (label, mode)
            knots = np.flatnonzero(np.isin(x, xg[:-1]))[:n - 1]
            assert same_bits(d[knots], 2.0 * (yg[1:] - yg[:-1]) / (xg[1:] - xg[:-1])).all(), (label, mode)
            assert np.isfinite(d[ok]).all()
            d0 = probe.host("interp", x, da=np.zeros(x.size), variant=1, tab=(xg, yg, mode))[1]
            assert np.all(d0[ok] == 0.0)


# ---------------------------------------------------------------------------------------------------------------------
# og_dual.h
@pytest.mark.parametrize("name", cases.DUAL_ONE)
def test_dual_rule_at_smooth_points(probe, name):
    """The derivative part, seed 1, against the textbook derivative in mpmath at the exact double input; the bound is
    the error of the same formula in float64 with NumPy's functions on the same inputs plus the allowances of the
    og_math functions the rule calls.  Seed 0 gives 0; seed -2.5 scales."""
    m = cases.measure_dual(name, probe)
    print("d %s on %s: %d inputs, float64 worst %.3f ulp, allowance %g, bound %g, og_dual worst %.3f ulp" % (
        name, m["domain"], m["inputs"], m["numpy_worst"], m["allowance"], m["bound"], m["og_worst"]))
    assert m["og_worst"] <= m["bound"]
    x = m["x"]
    assert np.all(probe.host(name, x, da=np.zeros(x.size), variant=1)[1] == 0.0)
    assert same_bits(probe.host(name, x, da=np.full(x.size, 4.0), variant=1)[1], 4.0 * m["got"]).all()   # exact scaling


def _rel_ulp(mp, got, exact):
    unit = mp.mpf(float(np.spacing(abs(cases.round_to_double(mp.mpf(exact))))))
    return float(abs(mp.mpf(float(got)) - exact) / unit)


@pytest.mark.parametrize("name", cases.DUAL_TWO)
def test_dual_rule_of_two_arguments_at_smooth_points(probe, name):
    """The three seedings (first, second, both) of a two-argument rule at points with both arguments positive, where
    the rule's own sum does not cancel; the mixed overloads (ogdual, double) / (double, ogdual) give the same bits as
    the full rule with a zero seed."""
    mp = cases._mp()
    r = np.random.default_rng(31)
    n = 1500
    a, b = np.exp(r.uniform(-3, 3, n)), np.exp(r.uniform(-3, 3, n))
    if name == "pow":
        a, b = 1.1 + np.exp(r.uniform(-3, 3.5, n)), r.uniform(0.5, 4.0, n)
    if name in ("mod", "fmod"):             # away from the jumps (left out: the derivative does not exist there)
        q = a / b
        far = np.abs(q - np.round(q)) > 1e-6
        assert far.mean() > 0.99
        a, b = a[far], b[far]
    both = 1.0 if name in ("hypot", "mul", "pow") else -1.0
    scale = np.ones(a.size)
    if name == "pow":
        scale = np.maximum(1.0, np.maximum(np.abs(b * np.log(a)), np.abs((b - 1.0) * np.log(a))))
    # allowances of the functions the rule calls: hypot_ 1; pow_ 3 |y log x| and log_ 1; the others only + - * / floor
    allowance = {"hypot": 1.0, "pow": 4.0}.get(name, 0.0)
    f64 = {"atan2": lambda y, x, dy, dx: (x * dy - y * dx) / (x * x + y * y),
           "hypot": lambda x, y, dx, dy: (x * dx + y * dy) / np.hypot(x, y),
           "pow": lambda x, y, dx, dy: y * np.power(x, y - 1.0) * dx + np.power(x, y) * np.log(x) * dy,
           "mod": lambda x, y, dx, dy: dx - np.floor(x / y) * dy, "fmod": lambda x, y, dx, dy: dx - np.trunc(x / y) * dy,
           "div": lambda x, y, dx, dy: (dx - (x / y) * dy) / y, "mul": lambda x, y, dx, dy: dx * y + x * dy}[name]
    exact = {"atan2": lambda y, x, dy, dx: (x * dy - y * dx) / (x * x + y * y),
             "hypot": lambda x, y, dx, dy: (x * dx + y * dy) / mp.sqrt(x * x + y * y),
             "pow": lambda x, y, dx, dy: y * mp.exp((y - 1) * mp.log(x)) * dx + mp.exp(y * mp.log(x)) * mp.log(x) * dy,
             "mod": lambda x, y, dx, dy: dx - mp.floor(x / y) * dy, "fmod": lambda x, y, dx, dy: dx - mp.floor(x / y) * dy,
             "div": lambda x, y, dx, dy: (dx - (x / y) * dy) / y, "mul": lambda x, y, dx, dy: dx * y + x * dy}[name]
    for da, db in ((1.0, 0.0), (0.0, 1.0), (1.0, both)):
        got = probe.host(name, a, b, da=np.full(a.size, da), db=np.full(a.size, db), variant=1)[1]
        ref = f64(a, b, da, db)
        e_og, e_np = np.zeros(a.size), np.zeros(a.size)
        for i in range(a.size):
            v = exact(mp.mpf(float(a[i])), mp.mpf(float(b[i])), mp.mpf(da), mp.mpf(db))
            if v == 0:
                assert got[i] == 0.0
                continue
            e_og[i], e_np[i] = _rel_ulp(mp, got[i], v) / scale[i], _rel_ulp(mp, ref[i], v) / scale[i]
        bound = allowance + cases.half_up(e_np.max())
        print("d %s seeds (%g, %g): float64 worst %.3f, allowance %g, bound %g, og_dual worst %.3f" % (
            name, da, db, e_np.max(), allowance, bound, e_og.max()))
        assert e_og.max() <= bound, (name, da, db)
        if db == 0.0:
            assert same_bits(probe.host(name, a, b, da=np.full(a.size, da), variant=2)[1], got).all()
        if da == 0.0:
            assert same_bits(probe.host(name, a, b, db=np.full(a.size, db), variant=3)[1], got).all()
    assert np.all(probe.host(name, a, b, da=np.zeros(a.size), db=np.zeros(a.size), variant=1)[1] == 0.0)


def test_dual_rules_where_their_factor_is_ill_conditioned(probe):
    """`1 - t*t` of tanh for 0.5 <= |x| < 22 and `1 - v*v` of asin / acos for 0.9 < |v| < 1 cancel by construction: they
    are judged by the ABSOLUTE error of that factor.  Bound: the absolute error of the same factor in float64 with
    NumPy on the same inputs, plus for tanh what the allowance of tanh_ (3 ulp of t <= 1) moves t*t by: 2 * 3 * 2^-53."""
    mp = cases._mp()
    r = np.random.default_rng(32)
    x = np.exp(r.uniform(np.log(0.5), np.log(22.0), 3000)) * np.where(r.uniform(-1, 1, 3000) < 0, -1.0, 1.0)
    got = probe.host("tanh", x, da=np.ones(x.size), variant=1)[1]
    ref = 1.0 - np.tanh(x) ** 2
    e_og = max(float(abs(mp.mpf(float(g)) - (1 - mp.tanh(mp.mpf(float(v))) ** 2))) for g, v in zip(got, x))
    e_np = max(float(abs(mp.mpf(float(g)) - (1 - mp.tanh(mp.mpf(float(v))) ** 2))) for g, v in zip(ref, x))
    print("tanh factor: float64 %.3g, og_dual %.3g (absolute)" % (e_np, e_og))
    assert e_og <= e_np + 6.0 * 2.0 ** -53
    assert np.all(got >= 0.0) and np.all(got <= 1.0)
    v = np.sign(r.uniform(-1, 1, 3000)) * (1.0 - 10.0 ** r.uniform(-15, -1, 3000))
    v = v[np.abs(v) < 1.0]
    for name, sign in (("asin", 1.0), ("acos", -1.0)):
        got = probe.host(name, v, da=np.ones(v.size), variant=1)[1]
        ref = sign / np.sqrt(1.0 - v * v)
        assert np.all(np.isfinite(got)) and np.all(np.sign(got) == sign)
        factor = lambda d, t: float(abs(1 / mp.mpf(float(d)) ** 2 - (1 - mp.mpf(float(t)) ** 2)))
        e_og = max(factor(g, t) for g, t in zip(got, v))
        e_np = max(factor(g, t) for g, t in zip(ref, v))
        print("%s factor: float64 %.3g, og_dual %.3g (absolute)" % (name, e_np, e_og))
        assert e_og <= e_np


def test_dual_rules_at_their_singular_points(probe):
    """Every promise in the comments of og_dual.h: a derivative of exactly 0, never NaN or inf."""
    zero = lambda d: np.all(d == 0.0) and not np.signbit(d).any() or np.all(d == 0.0)

    def d1(name, a, da, **kw):
        return probe.host(name, np.atleast_1d(a), da=np.full(np.size(a), da), variant=1, **kw)[1]

    def d2(name, a, b, da, db, variant=1):
        return probe.host(name, np.atleast_1d(a), np.atleast_1d(b), da=np.full(np.size(a), da),
                          db=np.full(np.size(a), db), variant=variant)[1]
    # sqrt at 0 (also with a seed: V |V|-like terms), and where V^2 underflowed
    assert zero(d1("sqrt", [0.0, -0.0], 1.0)) and zero(d1("sqrt", [0.0, -0.0, 4.0], 0.0))
    assert d1("sqrt", 4.0, 1.0)[0] == 0.25
    # a quantity that does not depend on the seeded variable keeps derivative 0 through a pole
    for name, pole in (("log", 0.0), ("log2", 0.0), ("log10", 0.0), ("log", -0.0), ("log1p", -1.0), ("asin", 1.0),
                       ("asin", -1.0), ("acos", 1.0), ("acos", -1.0)):
        assert zero(d1(name, pole, 0.0)), (name, pole)
    # quotient: 0/0-free when both derivatives are 0
    assert zero(d2("div", [1.0, 0.0, -1.0, INF], [0.0, 0.0, -0.0, INF], 0.0, 0.0))
    # |x| at +-0, cbrt at 0, hypot at the origin (every seeding), atan2 with both seeds 0 (at the origin too)
    assert zero(d1("fabs", [0.0, -0.0], 1.0)) and zero(d1("fabs", [0.0, -0.0], -3.0))
    assert zero(d1("cbrt", [0.0, -0.0], 1.0))
    for da, db in ((1.0, 0.0), (0.0, 1.0), (1.0, 1.0), (0.0, 0.0)):
        assert zero(d2("hypot", [0.0, -0.0], [0.0, 0.0], da, db))
    assert zero(d2("hypot", [0.0], [0.0], 1.0, 0.0, variant=2)) and zero(d2("hypot", [0.0], [0.0], 0.0, 1.0, variant=3))
    assert zero(d2("atan2", [0.0, 0.0, 1.0, -0.0], [0.0, -0.0, 0.0, 0.0], 0.0, 0.0))
    # mod / fmod with an infinite quotient: the dividend's derivative alone
    for name in ("mod", "fmod"):
        d = d2(name, [1.0, 1e300, -1e300, 5.0], [0.0, 1e-300, 1e-300, -0.0], 1.0, 1.0)
        assert np.all(d == 1.0), (name, d)
        assert np.all(d2(name, [1.0, 5.0], [0.0, 2.0], 1.0, 0.0, variant=2) == 1.0)
    # pow with only one factor seeded at x = 0: the other part stays out (0 log 0), no NaN
    d = d2("pow", [0.0, 0.0, 0.0, -0.0], [2.0, 1.0, 3.5, 2.0], 1.0, 0.0)
    assert np.array_equal(d, [0.0, 1.0, 0.0, 0.0]), d
    assert same_bits(d2("pow", [0.0, 0.0], [2.0, 1.0], 1.0, 0.0, variant=2), [0.0, 1.0]).all()
    d = d2("pow", [0.0, 0.0, 2.0], [2.0, 0.5, 0.0], 0.0, 1.0)
    assert same_bits(d, [0.0, 0.0, np.log(2.0)]).all(), d           # d/dy 0^y = 0 for y > 0: not 0 * -inf
    assert same_bits(d2("pow", [0.0], [2.0], 0.0, 1.0, variant=3), [0.0]).all()


def test_the_value_part_of_every_dual_result_has_the_bits_of_the_plain_function(probe):
    for name in cases.DUAL_ONE:
        a, _ = cases.table(name)
        plain = probe.host(name, a)[0]
        for seed in (1.0, 0.0):
            assert same_bits(probe.host(name, a, da=np.full(a.size, seed), variant=1)[0], plain).all(), (name, seed)
    for name in cases.DUAL_TWO:
        a, b = cases.table(name)
        plain = probe.host(name, a, b)[0]
        for variant in (1, 2, 3):
            got = probe.host(name, a, b, da=np.ones(a.size), db=np.full(a.size, -0.5), variant=variant)[0]
            assert same_bits(got, plain).all(), (name, variant)


# ---------------------------------------------------------------------------------------------------------------------
def test_two_host_compilers_give_the_same_bits(probe):
    """The twin is built by g++, the host half of a HIP module by clang: equal bits over the whole table, plain and
    dual (both with -ffp-contract=off, as the product)."""
    other = cases.load("clang")
    count = 0
    for label, name, variant, a, b, da, db, tab in cases.all_cases():
        v1, d1 = probe.host(name, a, b, da, db, variant, tab)
        v2, d2 = other.host(name, a, b, da, db, variant, tab)
        bad = ~(same_bits(v1, v2) & same_bits(d1, d2))
        assert not bad.any(), "%s: g++ and clang++ differ at %r" % (label, a[bad][:5])
        count += a.size
    assert count > 500000


def test_host_bits_are_the_recorded_ones(probe):
    """A change to og_math.h / og_dual.h that moves one result bit anywhere on the case table or the shared random
    distributions shows here, also where it stays inside its bound (a branch moved onto its threshold, a coefficient
    changed): the bits are the contract between the twin, the kernels and the goldens."""
    import json
    with open(cases.PINS) as fh:
        want = json.load(fh)
    got = cases.bit_digests(probe)
    assert sorted(got) == sorted(want)
    changed = sorted(k for k in got if got[k] != want[k])
    assert not changed, "result bits changed for: %s" % ", ".join(changed)


def test_probe_cross_compiles_for_gfx950_with_the_flags_of_the_product():
    """A build break of the device probe is seen on a machine without a GPU."""
    from opengoddard_amd import build
    path = cases.build_probe("hip")
    assert os.path.dirname(path) == build.JITDIR and cases.build_probe("hip") == path
    with open(path, "rb") as fh:
        blob = fh.read()
    assert b"gfx950" in blob and b"ogp_kernel" in blob
    lib = C.CDLL(path)
    assert hasattr(lib, "ogp_device") and hasattr(lib, "ogp_host")
    # clang's host loop inside the HIP module (no -mfma there: fma through libm) has the twin's bits too
    hip, gxx = cases.load("hip"), cases.load("gxx")
    for name in ("sin", "cbrt", "log2", "hypot", "pow"):
        a, b = cases.table(name)
        assert same_bits(hip.host(name, a, b)[0], gxx.host(name, a, b)[0]).all(), name
