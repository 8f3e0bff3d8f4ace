"""Exact Hessian-vector products ``grad^2 (w . F)(x) v`` without a GPU: the rules of ``csrc/og_dual2.h`` against mpmath,
the host probe of ``csrc/og_hvp.h`` (the terms the kernels sum, in the order of ``csrc/og_adj.h``) against the adjoint
probe, against itself (symmetry, linearity) and against central differences of the oracle's complex-step Jacobian, the
host logic of ``Problem.hessian_vector_product`` / ``evaluate_batch(hessian_products=)`` on a stand-in engine, the build
of the Hessian part and the C signatures.  Cases, references and the probes' builds are in ``hessian_cases``.

The rules.  Every operator and ``ogm::`` function, each overload, on second-order duals with non-zero ``d1``, ``d2``,
``dd``, at interior points and on both sides of every branch; all four parts against mpmath at 50 digits, the error in
units of the sum of the absolute values of the rule's terms.  Measured worst per function (g++ = clang++; this file
writes them to profiles/hessian.md): at most 6.2e-16 (``tanh_``); ``RULE_BOUNDS`` is four times each function's figure.

The reference of the product: central differences of ``oracle.exact_jac.jacobian`` at ``x +- h v`` times ``w`` in long
double, Richardson-extrapolated from ``h`` and ``h / 2``; its own error is estimated from the oracle alone (against the
extrapolation from ``h / 2`` and ``h / 4``), and the probe must be within ten times the shape's worst estimate, in units
of a column's ``max(1, sum_r |w_r d2F_r/dx_j dv|)``.  ``h`` is 2^-9, and 2^-13 for ``G17``, whose stencil at 2^-9 leaves
more than one column in fifty above 1e-6 of the scale.  Measured (estimate / probe's worst, this file writes them):
B5 6.4e-13 / 6.7e-13, G17 2.3e-08 / 1.5e-09, layout_8 8.0e-11 / 6.5e-11, P2U 8.7e-13 / 1.0e-12, B90 5.1e-13 / 5.3e-13.

The errors of the C calls that need a live handle are in tests/test_hessian_gpu.py.
"""
import ctypes
import os

import numpy as np
import pytest

import adjoint_cases as ac
import hessian_cases as hc
import og_math_cases
import parameter_exact_cases as ec
from opengoddard_amd import _native, build, optimize, problems

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REPORT = os.path.join(ROOT, "profiles", "hessian.md")
HEAD = ["# Exact grad^2 (w . F)(x) v: the rules of csrc/og_dual2.h and the host probe of csrc/og_hvp.h", "",
        "Rules: worst difference from mpmath (50 digits) over the four parts of every record of the function, in units of",
        "the sum of the absolute values of the rule's terms.  Shapes: the oracle reference's own error estimate and the",
        "probe's worst difference from it, per column in units of max(1, sum_r |w_r d2F_r/dx_j dv|).  Written by",
        "tests/test_hessian.py; the \"referee\", \"surface\" and \"surface triangles\" lines (oracle/exact_hess.py against the",
        "difference reference, the probe against that referee in units of its own scale, and the two orientations of a Hessian",
        "entry, over the traced surface at its four named points) by tests/test_hessian_surface.py.", "",
        "| what | figure |", "|---|---|"]


def _note(key, text):
    """One line of profiles/hessian.md (the key's line is replaced, not repeated)."""
    try:
        old = open(REPORT).read().split("\n") if os.path.exists(REPORT) else []
        kept = [row for row in (old or HEAD) if not row.startswith("| %s |" % key)]
        while kept and kept[-1] == "":
            kept.pop()
        with open(REPORT, "w") as fh:
            fh.write("\n".join(kept + ["| %s | %s |" % (key, text)]) + "\n")
    except OSError:
        pass


@pytest.fixture(scope="module")
def probe_dir(tmp_path_factory):
    return str(tmp_path_factory.mktemp("hvp_probe"))


# ------------------------------------------------------------------------------------------------ 1. the rules
# four times the measured worst of each function (units: the sum of the absolute values of the rule's terms)
MEASURED = {"add": 0.0, "sub": 6.94e-17, "mul": 1.06e-16, "div": 6.34e-17, "neg": 0.0, "sqrt": 1.25e-16, "exp": 1.36e-16,
            "log": 2.19e-16, "sin": 9.23e-17, "cos": 1.26e-16, "tan": 4.49e-16, "fabs": 0.0, "atan": 7.87e-17,
            "asin": 1.86e-16, "acos": 1.86e-16, "atan2": 2.01e-16, "tanh": 6.18e-16, "sinh": 1.25e-16, "cosh": 1.81e-16,
            "expm1": 7.86e-17, "log1p": 1.78e-16, "log2": 1.08e-16, "log10": 2.38e-16, "cbrt": 1.52e-16,
            "hypot": 1.39e-16, "mod": 0.0, "fmod": 0.0, "pow": 4.46e-16, "interp0": 4.44e-16, "interp1": 4.44e-16,
            "max": 0.0, "min": 0.0}
RULE_BOUNDS = {name: 4.0 * worst for name, worst in MEASURED.items()}


def test_the_rules_against_mpmath(probe_dir, capsys):
    import mpmath as mp
    gxx = hc.build_rules_probe(probe_dir, "g++")
    clang = hc.build_rules_probe(probe_dir, og_math_cases.clangxx())
    san = hc.build_rules_probe(probe_dir, "g++", sanitize=True)
    rec = hc.rule_records()
    assert set(hc.OPS[int(c)] for c in rec[:, 0]) == set(hc.OPS) == set(MEASURED)
    assert np.all(rec[rec[:, 1] == 0][:, 3:6] != 0.0), "d1, d2, dd of the argument are non-zero"
    got = hc.run_rules_probe(gxx, probe_dir, rec)
    for other in (clang, san):
        again = hc.run_rules_probe(other, probe_dir, rec, "rules_other")
        assert np.array_equal(again, got, equal_nan=True) and np.array_equal(np.signbit(again), np.signbit(got))
    assert np.all(np.isfinite(got))
    # rule (a): the projections are og_dual.h's, bit for bit
    assert np.array_equal(got[:, [0, 1]], got[:, [4, 5]]) and np.array_equal(got[:, [0, 2]], got[:, [6, 7]])
    worst = {}
    for r, g in zip(rec, got):
        name = hc.OPS[int(r[0])]
        truth, unit = hc.rule_truth(r)
        for part in range(4):
            u = unit[part] if unit[part] != 0 else mp.mpf(1)
            worst[name] = max(worst.get(name, 0.0), float(abs(mp.mpf(float(g[part])) - truth[part]) / u))
    for name in hc.OPS:
        _note("rule " + name, "%.2e" % worst[name])
        with capsys.disabled():
            if os.environ.get("OG_SURFACE_REPORT"):
                print("rule %-8s %.2e (bound %.2e)" % (name, worst[name], RULE_BOUNDS[name]))
    for name in hc.OPS:
        assert worst[name] <= RULE_BOUNDS[name], (name, worst[name], RULE_BOUNDS[name])


def test_zero_seeds_stay_zero_at_the_guarded_points(probe_dir):
    exe = hc.build_rules_probe(probe_dir, "g++")
    got = hc.run_rules_probe(exe, probe_dir, hc.singular_records(), "singular")
    for (name, a, b), g in zip(hc.SINGULAR, got):
        assert np.array_equal(g[[0, 1]], g[[4, 5]], equal_nan=True) and np.array_equal(g[[0, 2]], g[[6, 7]], equal_nan=True)
        assert g[3] == 0.0, (name, a, b, g)                # the mixed part: zero seeds, whatever the value is
        if name not in ("mul", "exp"):                      # (og_dual.h does not guard these two: 0 * inf is its d)
            assert g[1] == 0.0 and g[2] == 0.0, (name, a, b, g)


# ------------------------------------------------------------------------------------------------ 2. the host probe
STEP = {"G17": 2.0 ** -13}              # (the others: hessian_cases.H_STEP)
_RUNS = {}


def _probed(key, probe_dir):
    """The g++ probe of a shape at its second point and last parameter set for the eight pairs, once per session."""
    if key not in _RUNS:
        C = hc.case(key)
        W, V = hc.pairs(C)
        exe = hc.build_probe(C, probe_dir, "g++")
        x, theta = C.points[1], C.thetas[-1]
        _RUNS[key] = (C, exe, x, theta, W, V, hc.run_probe(C, exe, probe_dir, x, W, V, theta))
    return _RUNS[key]


@pytest.mark.parametrize("key", hc.GPU_KEYS)
def test_first_order_parts_are_the_adjoint_probes_bits(key, probe_dir):
    C, exe, x, theta, W, V, r = _probed(key, probe_dir)
    assert np.all(np.isfinite(r.Q))
    for other in (hc.build_probe(C, probe_dir, og_math_cases.clangxx()), hc.build_probe(C, probe_dir, "g++", sanitize=True)):
        o = hc.run_probe(C, other, probe_dir, x, W, V, theta, "other")
        assert np.array_equal(o.Q, r.Q) and np.array_equal(np.signbit(o.Q), np.signbit(r.Q)) and np.array_equal(o.G, r.G)
    G, F0 = ac.run_probe(C, ac.build_probe(C, probe_dir, "g++"), probe_dir, x, W, theta, "hvp_adj")
    assert np.array_equal(r.G, G) and np.array_equal(np.signbit(r.G), np.signbit(G)) and np.array_equal(r.F0, F0)
    assert not r.Q[6].any() and not np.signbit(r.Q[6]).any(), "the zero pair: +0.0 everywhere"
    unread = r.terms == 0
    assert not r.Q[:, unread].any() and not np.signbit(r.Q[:, unread]).any()


def test_the_shapes_cover_every_path_of_the_kernel(probe_dir):
    terms, heavy, reads = {}, {}, {}
    for key in hc.GPU_KEYS:
        r = _probed(key, probe_dir)[6]
        terms[key], heavy[key], reads[key] = r.terms, r.heavy, set(int(v) for v in r.reads)
    assert len(hc.GPU_KEYS) == 7
    # every value of a slot's `reads` word: bit 1 (og_hvp.h: the second-order part of every entry of the own block, not
    # of the diagonal alone) on NL2 without bit 0 and on NL0 with it
    assert reads["NL2"] == {-1, 1, 2} and reads["NL0"] == {-1, 3}
    assert set().union(*reads.values()) == {-1, 0, 1, 2, 3}
    assert all(2 not in v and 3 not in v for key, v in reads.items() if key not in ("NL2", "NL0"))
    assert any((t > 256).any() for t in terms.values())             # a thread's second trip through its chain
    assert any((t == 0).any() for t in terms.values())              # a column with no term
    assert all(((t > 0) & (t < 64) & (h == 0)).any() for t, h in zip(terms.values(), heavy.values()))   # light columns
    assert any(h.any() for h in heavy.values())                     # the workgroup path
    assert (terms["B90"] > 256).sum() == 1 and heavy["B90"][hc.case("B90").n - 1] == 1
    assert (terms["layout_8"] == 0).sum() == 130


@pytest.mark.parametrize("key", hc.GPU_KEYS)
def test_symmetry(key, probe_dir):
    """``u . H(w) v == v . H(w) u`` within 1e-12 of ``sum |w_r d2F_r/dx_i dx_j u_i v_j|``, estimated from the probe's own
    terms: ``sum_j |u_j| sum_r |w_r d2F_r/dx_j dv|`` and the same with u and v exchanged are both no larger than that
    sum (the inner sum over i is taken before the absolute value), so the larger of the two asks no less."""
    C, exe, x, theta, W, V, _ = _probed(key, probe_dir)
    w = W[3]
    U = np.stack([V[0], V[1], V[0], V[3], V[4]])
    T = np.stack([V[1], V[2], V[4], V[0], V[2]])
    ru = hc.run_probe(C, exe, probe_dir, x, np.tile(w, (5, 1)), U, theta, "sym_u")
    rt = hc.run_probe(C, exe, probe_dir, x, np.tile(w, (5, 1)), T, theta, "sym_t")
    seen = 0.0
    for d in range(5):
        left = np.dot(T[d].astype(np.longdouble), ru.Q[d].astype(np.longdouble))          # t . H u
        right = np.dot(U[d].astype(np.longdouble), rt.Q[d].astype(np.longdouble))         # u . H t
        scale = max(float(np.abs(T[d]) @ ru.S[d]), float(np.abs(U[d]) @ rt.S[d]))
        assert abs(left - right) <= hc.BOUND * scale, (key, d, float(left), float(right), scale)
        seen = max(seen, scale)
    assert seen > 0


@pytest.mark.parametrize("key", hc.GPU_KEYS)
def test_the_probe_against_differences_of_the_oracle(key, probe_dir, capsys):
    C, exe, x, theta, W, V, r = _probed(key, probe_dir)
    h = STEP.get(key, hc.H_STEP)
    estimate = worst = 0.0
    for d in range(W.shape[0]):
        ref, err = hc.oracle_products(C, x, W[d:d + 1], V[d], theta, h)
        scale = np.maximum(1.0, r.S[d])
        own = err[0] / scale
        smooth = own <= 1e-6                            # (else: a kink inside the stencil)
        assert (~smooth).sum() * 50 <= C.n, (key, d, int((~smooth).sum()))
        estimate = max(estimate, float(own[smooth].max()))
        worst = max(worst, float((np.abs(r.Q[d] - ref[0]).astype(float) / scale)[smooth].max()))
    _note("shape " + key, "estimate %.1e, probe %.1e" % (estimate, worst))
    with capsys.disabled():
        if os.environ.get("OG_SURFACE_REPORT"):
            print("hessian %-10s estimate %.2e probe %.2e" % (key, estimate, worst))
    assert estimate > 0 and worst <= 10.0 * estimate, (key, estimate, worst)


def test_linearity_in_w_and_a_pair_alone(probe_dir):
    C, exe, x, theta, W, V, r = _probed("layout_8", probe_dir)
    # pair d of K is the call with that pair alone, bit for bit
    for d in (0, 4, 7):
        one = hc.run_probe(C, exe, probe_dir, x, W[d], V[d], theta, "one")
        assert one.Q.shape == (1, C.n) and np.array_equal(one.Q[0], r.Q[d]) and np.array_equal(one.F0, r.F0)
    # H(a w1 + b w2) v = a H(w1) v + b H(w2) v: exactly for powers of two on one vector, within the bound for a sum
    v = V[0]
    lin = hc.run_probe(C, exe, probe_dir, x, np.stack([W[3], W[4], 4.0 * W[3], W[3] + 0.5 * W[4]]), np.tile(v, (4, 1)),
                       theta, "lin")
    assert np.array_equal(lin.Q[2], 4.0 * lin.Q[0])
    scale = np.maximum(1.0, lin.S[0] + 0.5 * lin.S[1])
    assert np.all(np.abs(lin.Q[3] - (lin.Q[0] + 0.5 * lin.Q[1])) <= hc.BOUND * scale)


# ------------------------------------------------------------------------------------------------ 3. host logic
class StandIn:
    """``Problem``'s engine protocol without a device: values from the problem's own callbacks are not needed here - the
    stand-in records its calls and returns a product that names the lane (its parameters, point, weights, direction)."""

    n, m, m_eq = 29, 33, 0

    def __init__(self, prob, obj):
        C = hc.case("P2U")
        self.n, self.m = C.n, C.m
        self.theta = np.array(list(prob.parameters.values()), dtype=float)
        self.calls = []

    def set_parameters(self, theta):
        self.theta = np.asarray(theta, dtype=float).copy()

    def values(self, p):
        return np.float64(p[0]), np.zeros(2), np.zeros(self.m - 3)

    @staticmethod
    def product(theta, x, W, V):
        return np.stack([np.sum(theta) * x + np.sum(w) * v for w, v in zip(W, V)])

    def hessian_vector(self, x, W, V):
        self.calls.append((self.theta.copy(), np.array(x, dtype=float), np.array(W, dtype=float), np.array(V, dtype=float)))
        return self.product(self.theta, x, W, V), np.zeros(self.m)


class NoHessian(StandIn):
    hessian_vector = property()         # (hasattr is False)


def _p2u():
    C = hc.case("P2U")
    prob, obj = ec.CASES["P2U"][0]()
    W, V = hc.pairs(C)
    return C, prob, obj, W, V


def test_hessian_vector_product_shapes_and_broadcast(monkeypatch):
    monkeypatch.setattr(optimize, "ENGINE_FACTORY", StandIn)
    C, prob, obj, W, V = _p2u()
    x, th = C.points[0], C.thetas[0]
    got = prob.hessian_vector_product(obj, W, V, x)
    eng = prob._engine
    assert got.shape == (8, C.n) and len(eng.calls) == 1 and getattr(prob, "_batch", None) is None
    assert np.array_equal(eng.calls[0][1], x) and np.array_equal(eng.calls[0][2], W) and np.array_equal(eng.calls[0][3], V)
    assert np.array_equal(got, StandIn.product(th, x, W, V))
    # one weight vector for every direction: one lambda, many v
    got = prob.hessian_vector_product(obj, W[3], V[:5], x)
    assert got.shape == (5, C.n) and np.array_equal(eng.calls[-1][2], np.tile(W[3], (5, 1)))
    assert np.array_equal(got, StandIn.product(th, x, np.tile(W[3], (5, 1)), V[:5]))
    # a single direction: [n] back, with [m] or [1, m] weights
    one = prob.hessian_vector_product(obj, W[4], V[2], x)
    assert one.shape == (C.n,) and eng.calls[-1][2].shape == (1, C.m) and eng.calls[-1][3].shape == (1, C.n)
    assert np.array_equal(one, prob.hessian_vector_product(obj, W[4:5], V[2], x))
    at_p = prob.hessian_vector_product(obj, W[4], V[2])                     # the default point: prob.p
    assert np.array_equal(eng.calls[-1][1], prob.p) and at_p.shape == (C.n,)
    prob.set_parameters(C.thetas[1])                                        # at new values: the engine is told first
    prob.hessian_vector_product(obj, W[:2], V[:2], x)
    assert np.array_equal(eng.calls[-1][0], C.thetas[1])


def test_refusals(monkeypatch):
    monkeypatch.setattr(optimize, "ENGINE_FACTORY", StandIn)
    C, prob, obj, W, V = _p2u()
    x = C.points[0]
    for bad in (V[0][:-1], V[:, :-1], np.zeros((0, C.n)), np.zeros((2, 2, C.n))):
        with pytest.raises(ValueError, match="directions must have"):
            prob.hessian_vector_product(obj, W[0], bad, x)
    for bad in (W[0][:-1], W[:3, :-1], W[:2], np.zeros((3, 2, C.m)), np.append(W[0], 0.0)):
        with pytest.raises(ValueError, match="weights must have"):
            prob.hessian_vector_product(obj, bad, V[:3], x)
    X = np.stack([x, C.points[1]])
    for bad in ((W[:2, :-1], V[:2]), (W[:2], V[:2, :-1]), (W[0], V[:2]), (W[:2],), W[:2]):
        with pytest.raises(ValueError, match="hessian_products must"):
            prob.evaluate_batch(obj, X, hessian_products=bad)
    with pytest.raises(ValueError, match="hessian_products holds 3 and 3 rows for 2 points"):
        prob.evaluate_batch(obj, X, hessian_products=(W[:3], V[:3]))
    with pytest.raises(ValueError, match="hessian_products holds 2 and 3 rows"):
        prob.evaluate_batch(obj, X, hessian_products=(W[:2], V[:3]))
    monkeypatch.setattr(optimize, "ENGINE_FACTORY", NoHessian)
    C, prob, obj, W, V = _p2u()
    with pytest.raises(ValueError, match="no exact Hessian-vector product"):
        prob.hessian_vector_product(obj, W, V, x)
    with pytest.raises(ValueError, match="no exact Hessian-vector product"):
        prob.evaluate_batch(obj, X, hessian_products=(W[:2], V[:2]))
    assert prob.evaluate_batch(obj, X).hessian_product is None      # (nothing else needs the method)


def test_evaluate_batch_serves_every_lane_with_its_own_pair(monkeypatch):
    monkeypatch.setattr(optimize, "ENGINE_FACTORY", StandIn)
    C, prob, obj, W, V = _p2u()
    X = np.stack([C.points[0], C.points[1], C.points[0]])
    TH = np.stack([C.thetas[1], C.thetas[0], C.thetas[1]])
    res = prob.evaluate_batch(obj, X, parameters=TH, hessian_products=(W[3:6], V[3:6]))
    assert res.hessian_product.shape == (3, C.n)
    calls = prob._engine.calls
    assert len(calls) == 3 and [tuple(c[0]) for c in calls] == [tuple(t) for t in TH]
    for k in range(3):
        assert np.array_equal(res.hessian_product[k], StandIn.product(TH[k], X[k], W[3 + k:4 + k], V[3 + k:4 + k])[0])
        assert calls[k][2].shape == (1, C.m) and np.array_equal(calls[k][2][0], W[3 + k])
        assert calls[k][3].shape == (1, C.n) and np.array_equal(calls[k][3][0], V[3 + k])
    plain = prob.evaluate_batch(obj, X, parameters=TH)
    assert plain.hessian_product is None and len(calls) == 3
    assert np.array_equal(plain.cost, res.cost)
    # one trajectory scanned over the parameter sets: its one pair goes with it
    scan = prob.evaluate_batch(obj, X[:1], parameters=TH, hessian_products=(W[:1], V[:1]))
    assert scan.hessian_product.shape == (3, C.n)
    assert np.array_equal(scan.hessian_product[2], StandIn.product(TH[2], X[0], W[:1], V[:1])[0])
    assert np.array_equal(prob._engine.theta, C.thetas[0])          # (the engine is back at the problem's values)


def test_a_real_engine_without_the_keyword_is_not_asked_for_anything_new():
    class Batch:
        capacity, engine, pattern = 2, None, None

        class _handle:
            value = 1

        def values(self, P):
            return np.zeros((P.shape[0], 3))

        def hessian_vector(self, X, W, V):
            raise AssertionError("hessian_vector was called")

    class Engine:
        m_eq, n_par, m = 1, 0, 3

        def hessian_vector(self, x, W, V):
            raise AssertionError("the engine's own hessian_vector was called")

        def _load_hessian_part(self):
            raise AssertionError("the part was asked for")

        def batch(self, B):
            bt = Batch()
            bt.engine = self
            return bt

    prob, obj = problems.build("brachistochrone")
    prob._engine = Engine()
    X = np.stack([prob.p, prob.p])
    res = prob.evaluate_batch(obj, X)
    assert res.hessian_product is None and res.cost.shape == (2,)
    with pytest.raises(AssertionError, match="hessian_vector was called"):
        prob.evaluate_batch(obj, X, hessian_products=(np.zeros((2, 3)), np.zeros_like(X)))
    prob._engine = None


# ------------------------------------------------------------------------------------------------ 4. the build
def test_the_hessian_part_is_a_file_of_its_own(monkeypatch, tmp_path):
    assert build.HESSIAN_PART == 9
    assert (build.MODULE_PARTS, build.BATCH_PART, build.BATCH_EXACT_PART, build.PARAMETER_PART, build.DIRECTIONAL_PART,
            build.ADJOINT_PART) == ((0, 2, 3, 1), 4, 5, 6, 7, 8)
    out = build.module_path("0123456789abcdef")
    others = [build.part_path(out, i) for i in range(len(build.MODULE_PARTS))] + [
        build.batch_part_path(out), build.batch_exact_part_path(out), build.parameter_part_path(out),
        build.directional_part_path(out), build.adjoint_part_path(out)]
    assert build.hessian_part_path(out).endswith(".hvp.so") and build.hessian_part_path(out) not in others
    sources = [os.path.basename(p) for p in build._kernel_sources()]
    assert "og_dual2.h" in sources and "og_hvp.h" in sources
    monkeypatch.setattr(build, "JITDIR", str(tmp_path))
    header = hc.case("B5").header
    mod = build.module_path(build.module_digest(header))
    assert os.path.dirname(mod) == str(tmp_path)
    stale = {}
    for path in [build.part_path(mod, i) for i in range(4)] + [build.batch_part_path(mod), build.parameter_part_path(mod),
                                                               build.directional_part_path(mod),
                                                               build.adjoint_part_path(mod)]:
        with open(path, "w") as fh:
            fh.write("untouched " + os.path.basename(path))
        stale[path] = os.stat(path).st_mtime_ns
    commands = []

    def run(cmd):
        commands.append(cmd)
        with open(cmd[cmd.index("-o") + 1], "w") as fh:
            fh.write("part")
    monkeypatch.setattr(build, "_run", run)
    part = build.build_hessian_part(header)
    assert part == build.hessian_part_path(mod) and os.path.exists(part)
    assert len(commands) == 1 and "-DOGK_PART=9" in commands[0]
    for path, stamp in stale.items():
        assert os.stat(path).st_mtime_ns == stamp and open(path).read() == "untouched " + os.path.basename(path)
    made = set(os.listdir(str(tmp_path))) - {os.path.basename(p) for p in stale}
    assert made == {os.path.basename(part), "og_gen_%s.h" % build.module_digest(header)}
    assert build.build_hessian_part(header) == part and len(commands) == 1      # cached


def test_the_hessian_part_cross_compiles_and_knows_its_two_modes_only():
    header = hc.case("B5").header
    part = build.build_hessian_part(header)
    with open(part, "rb") as fh:
        blob = fh.read()
    assert b"gfx950" in blob and b"ogk_exact_hvp" in blob and b"ogk_exact_hvp_batch" in blob
    assert b"ogk_exact_adj" not in blob and b"ogk_exact_dir" not in blob and b"ogk_fused" not in blob
    lib = ctypes.CDLL(part)
    assert hasattr(lib, "ogk_launch_batch") and hasattr(lib, "ogk_get_info")
    lib.ogk_launch.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p]
    lib.ogk_launch_batch.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p]
    # a record of zeros: the launcher refuses it before it touches the device (what og_hessian_vector_load relies on); a
    # mode of another part is that part's
    record = ctypes.create_string_buffer(4096)
    invalid = 1                                         # hipErrorInvalidValue
    assert lib.ogk_launch(record, 21, None) == invalid
    assert lib.ogk_launch(record, 19, None) == -4242 and lib.ogk_launch(record, 4, None) == -4242
    assert lib.ogk_launch_batch(record, 22, None) == invalid and lib.ogk_launch_batch(None, 22, None) == invalid
    assert lib.ogk_launch_batch(record, 20, None) == invalid


# ------------------------------------------------------------------------------------------------ 5. the C signatures
HESSIAN_FUNCTIONS = ("og_hessian_vector_load", "og_hessian_vector_dev", "og_hessian_vector", "og_hessian_vector_batch_dev",
                     "og_hessian_vector_batch")


def test_signatures_and_null_handles():
    C = ctypes
    dp = _native.SIGNATURES["og_directional"][1][1]                 # (the module's double pointer type)
    vp = C.c_void_p
    want = {
        "og_hessian_vector_load": [vp, C.c_char_p],
        "og_hessian_vector_dev": [vp, vp, C.c_int32, vp, vp, vp, vp, vp],
        "og_hessian_vector": [vp, dp, C.c_int32, dp, dp, dp, dp],
        "og_hessian_vector_batch_dev": [vp, C.c_int32, vp, vp, vp, vp, vp, vp],
        "og_hessian_vector_batch": [vp, C.c_int32, dp, dp, dp, dp, dp],
    }
    assert set(want) == set(HESSIAN_FUNCTIONS)
    lib = _native.lib()
    for name in HESSIAN_FUNCTIONS:
        restype, argtypes = _native.SIGNATURES[name]
        assert restype is C.c_int and argtypes == want[name], name
        assert getattr(lib, name).argtypes == want[name]                # AttributeError: not exported

    def error_text():
        msg = lib.og_last_error()
        return msg.decode() if msg else ""

    ptr = _native.dptr(np.zeros(4))
    calls = {
        "og_hessian_vector_load": (lambda: lib.og_hessian_vector_load(None, b"/nonexistent.so"), "null handle"),
        "og_hessian_vector_dev": (lambda: lib.og_hessian_vector_dev(None, 8, 1, 8, 8, 8, None, None), "null argument"),
        "og_hessian_vector": (lambda: lib.og_hessian_vector(None, ptr, 1, ptr, ptr, ptr, None), "null argument"),
        "og_hessian_vector_batch_dev": (lambda: lib.og_hessian_vector_batch_dev(None, 1, 8, 8, 8, None, 8, None),
                                        "null batch"),
        "og_hessian_vector_batch": (lambda: lib.og_hessian_vector_batch(None, 1, ptr, ptr, ptr, None, ptr), "null batch"),
    }
    for name, (call, what) in calls.items():
        assert call() == 1, name
        text = error_text()
        assert text.startswith(name + ":") and what in text, text
