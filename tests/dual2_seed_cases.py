"""The cases of tests/test_dual2_seeds.py (host) and tests/test_dual2_gpu.py (device): every rule of csrc/og_dual2.h over
every zero / non-zero pattern of its seeds, at ill-conditioned and edge points, and over the og_math case table with one
whole seed slot zero.

Also here: the three builds of tests/og_dual2_probe.hip (g++, ROCm's clang++, hipcc with build.HIP_FLAGS), the truth -
closed-form partial derivatives in mpmath at 50 digits, no numerical differentiation anywhere - the same closed forms in
plain float64 (NumPy), whose own error gives a record its bound where the committed one is out of reach, and
``--report``, which writes profiles/dual2_seeds.md / .json.

A record is 10 doubles ``[op, form, a.v, a.d1, a.d2, a.dd, b.v, b.d1, b.d2, b.dd]`` as tests/dual2_probe.cpp reads them
(op: the index in PROBE_OPS; form 0: dual o dual, 1: dual o double, 2: double o dual); a result is 8 doubles, the rule's
``v, d1, d2, dd`` and og_dual.h's ``(v, d)`` on the projections along seed 1 and seed 2.

Units and bounds.  The error of a part is measured in the unit of ``hessian_cases.rule_truth``: the sum of the absolute
values of the rule's terms (1 where there is none).  A record's bound is ``test_hessian.RULE_BOUNDS`` of its op, or, where
that is larger, four times the error of the float64 closed form at the same record against the same truth: the
conditioning of the record itself, measured on the reference and never on the header.  A difference of at most 2^-1074
(half the spacing of the subnormals) always passes.  A part whose truth is not finite (a pole, an undefined slope) carries
no accuracy claim: og_dual.h's bits are pinned there (rule (a)); a part whose truth is beyond DBL_MAX must be that infinity.
"""
from __future__ import annotations

import ctypes as C
import itertools
import json
import os
import sys

import numpy as np

import hessian_cases as hc
import og_math_cases as omc
from og_math_cases import same_bits

ROOT = omc.ROOT
CSRC = omc.CSRC
PROBE = os.path.join(ROOT, "tests", "og_dual2_probe.hip")
REPORT = os.path.join(ROOT, "profiles", "dual2_seeds")

PROBE_OPS = list(hc.OPS) + ["interp2"]                # the probe's ids: hessian_cases.OPS, then mode 2 of interp_linear
BINARY = hc.BINARY
INTERP = ("interp0", "interp1", "interp2")
STANDALONE_OPS = len(hc.OPS)                          # tests/dual2_probe.cpp knows the ops below this id
XG, YG, FILLS = np.array(hc.XG), np.array(hc.YG), hc.FILLS
SEEDS_A, SEEDS_B = hc.SEEDS_A, hc.SEEDS_B
MASKS = list(itertools.product((1.0, 0.0), repeat=3))           # (d1, d2, dd) kept or zeroed; the first keeps all
HALF_DENORM = 2.0 ** -1075
DBL_MAX, DBL_MIN, DENORM_MIN = omc.DBL_MAX, omc.DBL_MIN, omc.DENORM_MIN
INF, NAN = np.inf, np.nan


def forms(name):
    return (0, 1, 2) if name in BINARY else (0,)


def rule_bound(name):
    """the committed bound of an op (interp2 shares interp0's formula)"""
    import test_hessian
    return test_hessian.RULE_BOUNDS["interp0" if name == "interp2" else name]


# ---------------------------------------------------------------------------------------------------------------------
# the three builds of the probe
def _compile_host(compiler, out):
    import subprocess
    subprocess.check_call([compiler, "-O2", "-std=c++17", "-ffp-contract=off", "-mfma", "-fPIC", "-shared", "-I" + CSRC,
                           "-x", "c++", PROBE, "-o", out])
    return out


def probe_path(kind):
    """where a build of the probe lives: next to the other JIT products, keyed by the content of its sources"""
    from opengoddard_amd import build
    digest = build._digest_files([PROBE] + [os.path.join(CSRC, h) for h in ("og_math.h", "og_dual.h", "og_dual2.h")])
    os.makedirs(build.JITDIR, exist_ok=True)
    return os.path.join(build.JITDIR, "ogdual2_probe_%s_%s.so" % (kind, digest))


def build_probe(kind):
    """kind: "gxx", "clang" (the flags of og_math_cases._compile_host) or "hip" (hipcc with build.HIP_FLAGS unchanged: the
    kernel, the launcher and clang's host loop) -> path of the shared object"""
    from opengoddard_amd import build
    out = probe_path(kind)
    if os.path.exists(out):
        return out
    tmp = out + ".tmp%d" % os.getpid()
    if kind == "gxx":
        _compile_host("g++", tmp)
    elif kind == "clang":
        _compile_host(omc.clangxx(), tmp)
    else:
        build._run([build.hipcc()] + build.HIP_FLAGS + ["-I" + CSRC, PROBE, "-o", tmp])
    os.replace(tmp, out)
    return out


_DP = C.POINTER(C.c_double)


class Probe:
    def __init__(self, path):
        self.lib = C.CDLL(path)
        self.lib.og2p_name.restype = C.c_char_p
        names = [self.lib.og2p_name(i).decode() for i in range(self.lib.og2p_count())]
        assert names == PROBE_OPS, "tests/og_dual2_probe.hip and dual2_seed_cases.PROBE_OPS list different ops"
        assert [n for n in PROBE_OPS if self.lib.og2p_name(PROBE_OPS.index(n)).decode() != n] == []
        assert self.lib.og2p_name(-1) == b"" and self.lib.og2p_name(len(PROBE_OPS)) == b""
        self.lib.og2p_host.restype = None
        self.lib.og2p_host.argtypes = [C.c_int, C.c_int, _DP, _DP, C.c_int, _DP, _DP, C.c_int, C.c_double, C.c_double]
        if hasattr(self.lib, "og2p_device"):
            self.lib.og2p_device.restype = C.c_int
            self.lib.og2p_device.argtypes = [C.c_int, C.c_int, _DP, _DP, C.c_int, C.c_int, _DP, _DP, C.c_int, C.c_double,
                                             C.c_double]

    @staticmethod
    def _in(args):
        args = np.ascontiguousarray(args, dtype=np.float64)
        assert args.ndim == 2 and args.shape[1] == 8
        return args, np.full(args.shape, NAN)

    def host(self, name, form, args):
        """``args[n, 8]`` -> ``out[n, 8]`` of op ``name`` in ``form``, on the host"""
        args, out = self._in(args)
        p = lambda v: v.ctypes.data_as(_DP)
        self.lib.og2p_host(PROBE_OPS.index(name), form, p(args), p(out), len(args), p(XG), p(YG), XG.size, *FILLS)
        return out

    def device(self, name, form, args, block=64):
        """the same on the GPU -> (HIP's error code, out)"""
        args, out = self._in(args)
        p = lambda v: v.ctypes.data_as(_DP)
        err = self.lib.og2p_device(PROBE_OPS.index(name), form, p(args), p(out), len(args), block, p(XG), p(YG), XG.size,
                                   *FILLS)
        return err, out

    def run(self, records):
        """records ``[R, 10]`` -> ``[R, 8]`` on the host, grouped by (op, form)"""
        records = np.asarray(records, dtype=np.float64)
        out = np.full((len(records), 8), NAN)
        key = records[:, 0] * 4 + records[:, 1]
        for k in np.unique(key):
            sel = key == k
            out[sel] = self.host(PROBE_OPS[int(k) // 4], int(k) % 4, records[sel, 2:])
        return out


_PROBES = {}


def load(kind):
    if kind not in _PROBES:
        _PROBES[kind] = Probe(build_probe(kind))
    return _PROBES[kind]


# ---------------------------------------------------------------------------------------------------------------------
# closed-form partial derivatives, written once for two kinds of number: mpmath (the truth) and float64 (the textbook
# formula as a user would type it: its error at a record is that record's conditioning)
class _Mp:
    def __init__(self):
        import mpmath as mp
        self.mp = mp
        for f in ("sqrt", "exp", "log", "sin", "cos", "tan", "atan", "asin", "acos", "tanh", "sinh", "cosh", "expm1", "log1p",
                  "atan2", "hypot", "floor", "ceil", "power"):
            setattr(self, f, getattr(mp, f))
        self.inf, self.nan = mp.inf, mp.nan

    def num(self, v):
        return self.mp.mpf(float(v))

    def cbrt(self, t):
        return self.mp.sign(t) * self.mp.cbrt(abs(t))

    def ln(self, k):
        return self.mp.log(k)

    def finite(self, v):
        return self.mp.isfinite(v)


class _Np:
    inf, nan = np.float64(INF), np.float64(NAN)
    sqrt, exp, log, sin, cos, tan, atan, asin, acos = np.sqrt, np.exp, np.log, np.sin, np.cos, np.tan, np.arctan, np.arcsin, np.arccos
    tanh, sinh, cosh, expm1, log1p, atan2, hypot, floor, ceil, power, cbrt = (np.tanh, np.sinh, np.cosh, np.expm1, np.log1p,
                                                                             np.arctan2, np.hypot, np.floor, np.ceil, np.power, np.cbrt)
    num = staticmethod(np.float64)
    ln = staticmethod(lambda k: np.log(np.float64(k)))
    finite = staticmethod(np.isfinite)


def _interp(M, mode, a):
    xg, yg = [M.num(v) for v in XG], [M.num(v) for v in YG]
    zero = M.num(0)
    if not M.finite(a):
        return M.nan, M.nan
    i = min(max(sum(1 for g in xg if g <= a), 1), len(xg) - 1)       # the right-hand segment at a knot
    slope = (yg[i] - yg[i - 1]) / (xg[i] - xg[i - 1])
    y = slope * (a - xg[i - 1]) + yg[i - 1]
    if mode != 1:
        for k, g in enumerate(xg):
            if a == g:
                y = yg[k]                                              # a knot's own value
        if a < xg[0] or a > xg[-1]:
            y = M.nan if mode == 2 else M.num(FILLS[0] if a < xg[0] else FILLS[1])
            slope = zero
    return y, slope


def partials(M, name, a, b):
    """``(f, fx, fy, fxx, fxy, fyy)`` of the op at ``(a, b)`` in M's numbers, every one a closed form (a unary op: the y
    parts are 0; a piecewise-linear op: no curvature, its branch taken from the values as the header takes it)."""
    zero, one = M.num(0), M.num(1)
    if name in ("add", "sub"):
        return (a + b if name == "add" else a - b), one, (one if name == "add" else -one), zero, zero, zero
    if name == "neg":
        return -a, -one, zero, zero, zero, zero
    if name == "fabs":
        return abs(a), (one if a > 0 else (-one if a < 0 else zero)), zero, zero, zero, zero
    if name in ("max", "min"):
        first = (a > b) if name == "max" else (a < b)
        return (a if first else b), (one if first else zero), (zero if first else one), zero, zero, zero
    if name in ("mod", "fmod"):
        if b == 0:
            return M.nan, one, M.nan, zero, zero, zero
        r = a / b
        q = M.floor(r) if (name == "mod" or r >= 0) else M.ceil(r)
        return a - q * b, one, -q, zero, zero, zero
    if name in INTERP:
        y, slope = _interp(M, INTERP.index(name), a)
        return y, slope, zero, zero, zero, zero
    if name == "sqrt":
        r = M.sqrt(a)
        return r, 1 / (2 * r), zero, -1 / (4 * r * a), zero, zero
    if name in ("exp", "expm1"):
        e = M.exp(a)
        return (e if name == "exp" else M.expm1(a)), e, zero, e, zero, zero
    if name in ("log", "log2", "log10"):
        k = one if name == "log" else M.ln(2 if name == "log2" else 10)
        return M.log(a) / k, 1 / (a * k), zero, -1 / (a * a * k), zero, zero
    if name == "log1p":
        g = 1 + a
        return M.log1p(a), 1 / g, zero, -1 / (g * g), zero, zero
    if name == "sin":
        return M.sin(a), M.cos(a), zero, -M.sin(a), zero, zero
    if name == "cos":
        return M.cos(a), -M.sin(a), zero, -M.cos(a), zero, zero
    if name == "tan":
        t = M.tan(a)
        return t, 1 + t * t, zero, 2 * t * (1 + t * t), zero, zero
    if name == "tanh":
        t = M.tanh(a)
        return t, 1 - t * t, zero, -2 * t * (1 - t * t), zero, zero
    if name == "sinh":
        return M.sinh(a), M.cosh(a), zero, M.sinh(a), zero, zero
    if name == "cosh":
        return M.cosh(a), M.sinh(a), zero, M.cosh(a), zero, zero
    if name == "atan":
        g = 1 + a * a
        return M.atan(a), 1 / g, zero, -2 * a / (g * g), zero, zero
    if name in ("asin", "acos"):
        g = 1 - a * a
        r = M.sqrt(g)
        s = one if name == "asin" else -one
        return (M.asin(a) if name == "asin" else M.acos(a)), s / r, zero, s * a / (g * r), zero, zero
    if name == "cbrt":
        c = M.cbrt(a)
        return c, 1 / (3 * c * c), zero, -2 / (9 * c * c * a), zero, zero
    if name == "mul":
        return a * b, b, a, zero, one, zero
    if name == "div":
        return a / b, 1 / b, -a / (b * b), zero, -1 / (b * b), 2 * a / (b * b * b)
    if name == "atan2":                                 # atan2(y = a, x = b)
        r2 = a * a + b * b
        return M.atan2(a, b), b / r2, -a / r2, -2 * a * b / (r2 * r2), (a * a - b * b) / (r2 * r2), 2 * a * b / (r2 * r2)
    if name == "hypot":
        h = M.hypot(a, b)                               # y^2 / h^3, -x y / h^3, x^2 / h^3 through the direction cosines:
        cx, cy = a / h, b / h                           # h^3 itself leaves float64 at 1e-200 and at 1e200
        return h, cx, cy, cy * cy / h, -(cx * cy) / h, cx * cx / h
    assert name == "pow", name
    if a == 0:                                          # b > 0 in every case here: the limits at the corner
        pw = lambda e: one if e == 0 else (zero if e > 0 else M.inf)
    elif a < 0:                                         # whole exponents only
        pw = lambda e: M.power(-a, e) * (-1 if int(e) % 2 else 1)
    else:
        pw = lambda e: M.power(a, e)
    p, A = pw(b), pw(b - 1)
    fxx = zero if b * (b - 1) == 0 else b * (b - 1) * pw(b - 2)
    if a > 0:
        L = M.log(a)
        return p, b * A, p * L, fxx, A * (1 + b * L), p * L * L
    if a == 0:                                          # x^y log x -> 0; d/dy of y x^(y-1) at 0: 0 beyond y = 1, a pole up to it
        return p, b * A, zero, fxx, (zero if b > 1 else -M.inf), zero
    return p, b * A, M.nan, fxx, M.nan, M.nan           # x < 0: no derivative along y


def _combine(M, name, form, rec8):
    """-> (parts[4], units[4]): the rule's four parts and per part the sum of the absolute values of its terms.  A term
    whose seed factor is zero is left out (it IS zero wherever the partial is finite)."""
    a, a1, a2, a12, b, b1, b2, b12 = (M.num(v) for v in rec8)
    zero = M.num(0)
    if name not in BINARY or form == 1:
        b1 = b2 = b12 = zero
    if name in BINARY and form == 2:
        a1 = a2 = a12 = zero
    f, fx, fy, fxx, fxy, fyy = partials(M, name, a, b)

    def term(p, *seeds):
        if any(s == 0 for s in seeds):
            return zero
        for s in seeds:
            p = p * s
        return p
    parts = [[f], [term(fx, a1), term(fy, b1)], [term(fx, a2), term(fy, b2)],
             [term(fxx, a1, a2), term(fxy, a1, b2), term(fxy, a2, b1), term(fyy, b1, b2), term(fx, a12), term(fy, b12)]]
    total = lambda p: sum(p[1:], p[0])
    return [total(p) for p in parts], [total([abs(t) for t in p]) for p in parts]


def judge(records, got):
    """-> ``(err[R, 4], ref[R, 4], claim[R, 4])``: the error of ``got[:, :4]`` and of the float64 closed form against the
    50-digit truth, in the truth's unit, and whether the part carries an accuracy claim (its truth is finite).  Where the
    truth is beyond DBL_MAX the error is 0 for the right infinity and inf otherwise."""
    import mpmath as mp
    M, N = _Mp(), _Np
    R = len(records)
    err, ref, claim = np.zeros((R, 4)), np.zeros((R, 4)), np.zeros((R, 4), dtype=bool)
    with mp.workdps(50), np.errstate(all="ignore"):
        for i, r in enumerate(records):
            name, form = PROBE_OPS[int(r[0])], int(r[1])
            truth, unit = _combine(M, name, form, r[2:])
            textbook, _ = _combine(N, name, form, r[2:])
            for k in range(4):
                if not (mp.isfinite(truth[k]) and mp.isfinite(unit[k])):
                    continue
                claim[i, k] = True
                u = unit[k] if unit[k] != 0 else mp.mpf(1)
                for value, dest in ((got[i, k], err), (float(textbook[k]), ref)):
                    if abs(truth[k]) > DBL_MAX:
                        dest[i, k] = 0.0 if value == (INF if truth[k] > 0 else -INF) else INF
                    elif not np.isfinite(value):
                        dest[i, k] = INF
                    else:
                        diff = abs(mp.mpf(float(value)) - truth[k])
                        dest[i, k] = 0.0 if diff <= HALF_DENORM * 2 else float(diff / u)
    return err, ref, claim


def bounds(records, ref):
    """per record and part: the committed bound of the op, or four times the float64 closed form's error where larger"""
    base = np.array([rule_bound(PROBE_OPS[int(r[0])]) for r in records])
    return np.maximum(base[:, None], 4.0 * ref)


# ---------------------------------------------------------------------------------------------------------------------
# 2.1 the seed lattice at interior points
def _rec(name, form, a, sa, b=0.0, sb=(0.0, 0.0, 0.0)):
    return [PROBE_OPS.index(name), form, a, *sa, b, *sb]


def _masked(seeds, mask):
    return tuple(s * m for s, m in zip(seeds, mask))


def lattice_records():
    """every op and form at hessian_cases' points under every zero / non-zero mask of (d1, d2, dd) of a - and of b for a
    binary op, in all three forms (a form ignores the seeds of its plain argument, whatever they are)."""
    rec = []
    for name in PROBE_OPS:
        if name in BINARY:
            for a, b in hc.BINARY_POINTS[name]:
                for form in (0, 1, 2):
                    for ma in MASKS:
                        for mb in MASKS:
                            rec.append(_rec(name, form, a, _masked(SEEDS_A, ma), b, _masked(SEEDS_B, mb)))
        else:
            for a in hc.UNARY_POINTS["interp0" if name == "interp2" else name]:
                for ma in MASKS:
                    rec.append(_rec(name, 0, a, _masked(SEEDS_A, ma)))
    return np.array(rec, dtype=np.float64)


def special_seed_records():
    """a few records whose seeds are -0.0, inf or NaN: rule (a) and the equality of the builds are asserted on them; a
    -0.0 seed is a zero seed (its terms are left out)"""
    rec = []
    for name in PROBE_OPS:
        a, b = (hc.BINARY_POINTS[name][0] if name in BINARY else
                (hc.UNARY_POINTS["interp0" if name == "interp2" else name][0], 0.0))
        for sa, sb in (((-0.0, -1.25, 0.4375), (-0.625, -0.0, -0.3125)), ((0.75, -0.0, -0.0), (-0.0, 1.5, -0.0)),
                       ((-0.0, -0.0, -0.0), (-0.0, -0.0, -0.0)), ((INF, -1.25, 0.4375), (-0.625, 1.5, -INF)),
                       ((0.75, NAN, 0.4375), (-0.625, 1.5, -0.3125)), ((0.75, -1.25, INF), (NAN, 1.5, 0.0))):
            for form in forms(name):
                rec.append(_rec(name, form, a, sa, b, sb))
    return np.array(rec, dtype=np.float64)


# ---------------------------------------------------------------------------------------------------------------------
# 2.2 ill-conditioned and edge points: (name, form, a, b, pin).  pin: og_dual.h's own slope is not the derivative there
# (it leaves a term out or is not finite), so the record pins rule (a) only.  Each runs under the masks of EDGE_MASKS.
EDGE_MASKS = [((1, 1, 1), (1, 1, 1)), ((1, 1, 0), (1, 1, 0)), ((1, 1, 1), (0, 0, 0)), ((0, 0, 0), (1, 1, 1)),
              ((1, 0, 1), (0, 1, 1)), ((1, 1, 0), (0, 0, 0)), ((0, 0, 1), (0, 0, 1))]
PI_2 = 1.5707963267948966
SUBNORMAL = 3 * DENORM_MIN


def edge_points():
    pts = []
    for ratio in (1e-2, 1e-4, 1e-8):
        for x in (-3.0, 1.0):
            c = abs(x) * ratio
            for name in ("hypot", "atan2"):
                for form in (0, 1, 2):
                    pts += [(name, form, x, c, False), (name, form, c, x, False)]
    for v in (1e-200, 1e200):
        for form in (0, 1, 2):
            pts.append(("hypot", form, v, v, False))
            pts.append(("hypot", form, -v, 0.5 * v, False))
    for y in (1.0, 2.0, 3.0, 0.5):
        pts.append(("pow", 1, 0.0, y, False))              # y constant
        pts.append(("pow", 0, 0.0, y, False))              # y seeded
    pts.append(("pow", 1, 0.0, 0.0, True))                  # d/dx x^0 at 0: og_dual.h's 0 * inf
    for x, y in ((-2.0, 3.0), (-1.5, 2.0), (-2.0, -3.0), (-0.5, 1.0), (-3.0, 0.0)):
        pts.append(("pow", 1, x, y, False))
    for name in ("sqrt", "cbrt", "log", "log2", "log10"):
        for v in (DBL_MIN, SUBNORMAL, DENORM_MIN):
            pts.append((name, 0, v, 0.0, False))
    pts += [("cbrt", 0, -DBL_MIN, 0.0, False), ("cbrt", 0, -SUBNORMAL, 0.0, False)]
    for v in (PI_2, np.nextafter(PI_2, 0.0), np.nextafter(PI_2, 2.0), -PI_2):
        pts.append(("tan", 0, float(v), 0.0, False))
    pts += [("fabs", 0, 0.0, 0.0, False), ("fabs", 0, -0.0, 0.0, False)]
    for name in ("max", "min"):
        for form in (0, 1, 2):
            pts += [(name, form, 0.7, 0.7, False), (name, form, 0.0, -0.0, False), (name, form, -0.0, 0.0, False)]
    for name in ("mod", "fmod"):
        for form in (0, 1, 2):
            pts += [(name, form, 7.5, 2.5, False), (name, form, 5.0, 2.5, False), (name, form, -7.5, 2.5, False),
                    (name, form, 7.5, -2.5, False), (name, form, 0.0, 2.5, False),
                    (name, form, 1.0, 0.0, True), (name, form, 1e300, 1e-300, True), (name, form, -1e300, 1e-300, True)]
    for name in INTERP:
        for v in (0.0, 1.0, 2.5, 4.0, np.nextafter(0.0, -1.0), np.nextafter(0.0, 1.0), np.nextafter(4.0, 0.0),
                  np.nextafter(4.0, 5.0), np.nextafter(1.0, 0.0), np.nextafter(2.5, 3.0), -1.0, 5.0):
            pts.append((name, 0, float(v), 0.0, False))
    return pts


def edge_records():
    """-> (records[R, 10], pin[R])"""
    rec, pin = [], []
    for name, form, a, b, p in edge_points():
        for ma, mb in (EDGE_MASKS if name in BINARY else [(m, (0, 0, 0)) for m in MASKS]):
            if name in BINARY and ((form == 1 and not any(ma)) or (form == 2 and not any(mb))):
                continue
            rec.append(_rec(name, form, a, _masked(SEEDS_A, ma), b, _masked(SEEDS_B, mb)))
            pin.append(p)
    return np.array(rec, dtype=np.float64), np.array(pin)


# ---------------------------------------------------------------------------------------------------------------------
# 2.3 exact zeros: one whole seed slot zero and both dd zero, over the og_math case table
ZERO_SEEDS = (("slot 1 zero", (0.0, -1.25, 0.0), (0.0, 1.5, 0.0)), ("slot 2 zero", (0.75, 0.0, 0.0), (-0.625, 0.0, 0.0)))
_TABLE_OF = {"neg": None, "add": None, "sub": None, "max": None, "min": None, "mul": "mul", "div": "div"}


def zero_values(name):
    """-> (a, b): og_math_cases.table of the function behind the op; the 32 x 32 GRID for an op without one"""
    if name in INTERP:
        return np.concatenate([omc.interp_queries(XG), omc.GRID]), None
    fn = _TABLE_OF.get(name, name)
    if fn is None:
        a, b = [g.ravel() for g in np.meshgrid(omc.GRID, omc.GRID, indexing="ij")]
        return (a, b) if name in BINARY else (a, None)
    return omc.table(fn)


def zero_args(name):
    """-> ``args[n, 8]``: both seed patterns over the values of the op"""
    a, b = zero_values(name)
    out = []
    for _, sa, sb in ZERO_SEEDS:
        args = np.zeros((a.size, 8))
        args[:, 0], args[:, 1:4] = a, sa
        args[:, 4], args[:, 5:8] = (0.0 if b is None else b), sb
        out.append(args)
    return np.concatenate(out)


def zero_exceptions(name, form, args, out):
    """-> (n_nonzero, n_permitted): results whose dd is not exactly zero, and those of them the header's comment permits:
    ``double / ogdual2`` where og_dual.h's unguarded slope along the seeded slot is itself not finite"""
    bad = ~(out[:, 3] == 0.0)
    seeded = np.where(args[:, 5] != 0.0, out[:, 5], out[:, 7])          # og_dual.h's d along the slot that is seeded
    permitted = bad & (name == "div") & (form == 2) & ~np.isfinite(seeded)
    return int(bad.sum()), int(permitted.sum())


# ---------------------------------------------------------------------------------------------------------------------
# what the device test runs: per (op, form) the records of 2.1 - 2.3 as args[n, 8], never a multiple of 64
def device_groups(sections=("seeds", "zeros")):
    """(op, form, args[n, 8]) - "seeds": the records of 2.1 and 2.2, "zeros": those of 2.3, every value of the table
    under one of the two seed patterns in turn (the host test runs both on each: the device run stays at a few hundred
    thousand records)"""
    lat, spec, (edge, _) = lattice_records(), special_seed_records(), edge_records()
    for name in PROBE_OPS:
        zeros = zero_args(name)
        half = np.arange(len(zeros) // 2)
        zeros = zeros[half + (half % 2) * half.size]
        for form in forms(name):
            code = PROBE_OPS.index(name)
            parts = [r[(r[:, 0] == code) & (r[:, 1] == form)][:, 2:] for r in (lat, spec, edge)] if "seeds" in sections else []
            args = np.concatenate(parts + ([zeros] if "zeros" in sections else []))
            yield name, form, (args[:-1] if len(args) % 64 == 0 else args)


def branch_key(name, args):
    """inputs of one key take the same branches of og_math.h (the interval between the function's thresholds that each
    value falls in, sign and NaN apart) and leave the same terms of og_dual2.h out (which seeds are zero)"""
    fn = {"interp0": None, "interp1": None, "interp2": None}.get(name, name)
    cuts = np.unique(np.abs(np.array(omc.THRESHOLDS.get(fn, []) + [0.0, DBL_MIN, 1.0, INF] + list(XG))))
    value = lambda a: np.searchsorted(cuts, np.abs(a), side="right") * 4 + np.signbit(a) * 2 + np.isnan(a)
    mask = sum((args[:, k] != 0.0).astype(np.int64) << j for j, k in enumerate((1, 2, 3, 5, 6, 7)))
    return (value(args[:, 0]) * 4096 + value(args[:, 4])) * 64 + mask


# ---------------------------------------------------------------------------------------------------------------------
def measure(probe):
    """-> per op: records, worst error, the bound there and where it came from, the count of exceptions of 2.3"""
    lat, (edge, pin) = lattice_records(), edge_records()
    records = np.concatenate([lat, edge[~pin]])
    got = probe.run(records)
    err, ref, claim = judge(records, got)
    bnd = bounds(records, ref)
    rows = {}
    for code, name in enumerate(PROBE_OPS):
        sel = np.flatnonzero(records[:, 0] == code)
        e = np.where(claim[sel], err[sel], 0.0)
        slack = np.where(claim[sel], e / np.where(bnd[sel] > 0, bnd[sel], 1.0), 0.0)
        i, k = np.unravel_index(np.argmax(e), e.shape)
        committed = rule_bound(name)
        widened = int((bnd[sel] > committed).any(axis=1).sum())
        needed = int((claim[sel] & (err[sel] > committed)).any(axis=1).sum())
        nonzero = permitted = count = 0
        zeros = zero_args(name)
        for form in forms(name):
            out = probe.host(name, form, zeros)
            n, p = zero_exceptions(name, form, zeros, out)
            nonzero, permitted, count = nonzero + n, permitted + p, count + len(zeros)
        rows[name] = dict(records=int(sel.size), pinned_only=int((edge[pin][:, 0] == code).sum()), worst=float(e[i, k]),
                          worst_part=("v", "d1", "d2", "dd")[k], worst_record=[float(v) for v in records[sel[i]]],
                          bound_there=float(bnd[sel[i], k]), committed_bound=committed,
                          bound_from=("4 x the float64 closed form's error at the record" if bnd[sel[i], k] > committed
                                      else "test_hessian.RULE_BOUNDS"),
                          records_on_the_float64_bound=widened, records_beyond_the_committed_bound=needed,
                          float64_worst=float(np.where(claim[sel], ref[sel], 0.0).max()),
                          worst_share_of_bound=float(slack.max()) if (bnd[sel] > 0).all() else None,
                          zero_records=count, zero_exceptions=nonzero, zero_exceptions_permitted=permitted)
    return rows


def report(stem=REPORT):
    rows = measure(load("gxx"))
    with open(stem + ".json", "w") as fh:
        json.dump(rows, fh, indent=1, sort_keys=True)
        fh.write("\n")
    lines = ["# og_dual2.h over every seed pattern, at its edges and over the og_math case table",
             "",
             "Written by `python tests/dual2_seed_cases.py --report` (the g++ build of `tests/og_dual2_probe.hip` against",
             "closed-form partial derivatives in mpmath at 50 digits); the assertions are `tests/test_dual2_seeds.py`.",
             "Errors are in units of the sum of the absolute values of the rule's terms, the worst over the four parts",
             "`v, d1, d2, dd` and over the records of sections 2.1 (the seed lattice at interior points) and 2.2 (the edge",
             "points) that carry an accuracy claim.  `bound there` is the bound of the record with the worst error: the",
             "committed `RULE_BOUNDS` of `tests/test_hessian.py`, or four times the error of the float64 closed form at that",
             "record where that is larger (`on float64 bound` counts the records judged that way, `beyond committed` those of",
             "them whose error is in fact beyond the committed bound).  `pinned` records have no",
             "finite derivative in og_dual.h itself and pin rule (a) only.  The last columns are section 2.3: results whose",
             "`dd` is not exactly zero with one whole seed slot zero, all of them `double / ogdual2` at a divisor where",
             "og_dual.h's unguarded slope is itself not finite.  Nothing here was measured on a GPU:",
             "`tests/test_dual2_gpu.py` compares the device with this host build bit for bit.",
             "",
             "| op | records | pinned | worst error | part | bound there | from | committed bound | float64 worst | on float64 bound | beyond committed | zero-slot records | dd != 0 | of them permitted |",
             "|---|---|---|---|---|---|---|---|---|---|---|---|---|---|"]
    for name in PROBE_OPS:
        r = rows[name]
        lines.append("| %s | %d | %d | %.2e | %s | %.2e | %s | %.2e | %.2e | %d | %d | %d | %d | %d |" % (
            name, r["records"], r["pinned_only"], r["worst"], r["worst_part"], r["bound_there"], r["bound_from"],
            r["committed_bound"], r["float64_worst"], r["records_on_the_float64_bound"], r["records_beyond_the_committed_bound"],
            r["zero_records"],
            r["zero_exceptions"], r["zero_exceptions_permitted"]))
    total = lambda k: sum(r[k] for r in rows.values())
    lines += ["", "Totals: %d records with an accuracy claim, %d zero-slot records, %d with dd != 0, %d of them permitted." % (
        total("records"), total("zero_records"), total("zero_exceptions"), total("zero_exceptions_permitted")), ""]
    with open(stem + ".md", "w") as fh:
        fh.write("\n".join(lines))


if __name__ == "__main__":
    if "--report" in sys.argv:
        report()
    else:
        print(__doc__)
