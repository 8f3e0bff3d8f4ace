"""Exact dF/dtheta for run-time parameters, without a GPU: the header's hook and work lists, the host probe of
``csrc/og_par.h`` (the one function the kernels compute every entry with) against the complex step in theta, and the
host logic of ``Problem.parameter_sensitivity(exact=True)`` / ``evaluate_batch(parameter_jacobian=True)`` on a stand-in
engine.  The cases, the reference and the probe's build are in ``parameter_exact_cases``.

The probe is compared with the complex step within ``BOUND = 1e-12`` of the row's largest entry over the parameters (the
bound of tests/test_exact_surface.py for the same comparison in x), at every case, parameter set and point.  Measured
worst per case (g++, this file appends them to profiles/params_exact.md): P2 1.9e-16, P2U 3.3e-16, G9 2.2e-16, G17 2.6e-16,
E 5.6e-16.
"""
import os
import re
import warnings

import numpy as np
import pytest

import og_math_cases
import parameter_cases as pc
import parameter_exact_cases as ec
from opengoddard_amd import _native, codegen, optimize, problems
from oracle import program_eval, twin

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REPORT = os.path.join(ROOT, "profiles", "params_exact.md")
KEYS = list(ec.CASES)


def _random_points(C, count=5):
    rng = np.random.default_rng(11)
    return [C.points[0] * (1.0 + 0.02 * rng.standard_normal(C.points[0].size)) for _ in range(count)]


# ------------------------------------------------------------------------------------------------ 1. the header
def test_the_hook_appears_only_in_a_header_with_parameters():
    prob, obj = problems.build("brachistochrone")
    P = codegen.trace_problem(prob, obj)
    plain = codegen.emit_header(P)
    for word in ("par_leaf", "OG_GEN_HAS_PAR", "PAR_ROW_PTR", "PAR_ENTRIES"):
        assert word not in plain
    assert codegen.parameter_sparsity(P).shape == (0, P.m)
    for key in KEYS:
        C = ec.case(key)
        assert "#define OG_GEN_HAS_PAR 1" in C.header and "PAR_ENTRIES" in C.header
        # every parameter leaf goes through the hook: no bare subscript of the parameter tail is left
        tail = range(C.program.par_off, C.program.par_off + C.n_par)
        assert not [i for i in map(int, re.findall(r"cv\[(\d+)\]", C.header)) if i in tail]
        read = sorted({int(i) - C.program.par_off for i in re.findall(r"par_leaf\(x, cv, (\d+), 0\)", C.header)})
        assert read == [k for k in range(C.n_par) if k not in ec.UNREAD[key]]


def test_a_parameterised_header_does_not_depend_on_the_values():
    for key in ("P2U", "E"):
        factory, _, thetas = ec.CASES[key]
        assert codegen.emit_header(pc.trace(*factory(thetas[1]))) == ec.case(key).header


@pytest.mark.parametrize("key", KEYS)
def test_the_untouched_twin_compiles_the_header_and_equals_the_interpreter(key):
    C = ec.case(key)
    tw = twin.Twin(C.prob, C.obj, program=C.program, header=C.header)       # (oracle/twin.cpp: XVec / XDual get cv[i])
    for theta in C.thetas[:3]:
        tw._cv[C.program.par_off:] = theta
        P = ec._AtTheta(C.program, C.cvec(theta))
        for x in C.points:
            want = program_eval.evaluate(P, C.prob, x)
            assert np.all(np.abs(tw.values(x) - want) <= 1e-9 * np.maximum(1.0, np.abs(want)))
            # the seed is on no decision variable's path: the twin's exact Jacobian in x is what it was with cv[i]
            assert np.all(np.isfinite(tw.exact(x, cols=[0, C.program.n - 1])[1]))


@pytest.mark.parametrize("key", KEYS)
def test_parameter_sparsity_contains_what_the_complex_step_finds(key):
    C = ec.case(key)
    S = codegen.parameter_sparsity(C.program)
    assert S.shape == (C.n_par, C.m) and S.dtype == bool
    union = np.zeros_like(S)
    for theta in C.thetas[:3] if key != "E" else C.thetas:
        for x in _random_points(C):
            ref = ec.complex_step(C, theta, x)
            assert np.all(np.isfinite(ref))
            assert not np.any(ref[~S]), "a row outside the pattern depends on a parameter"
            union |= ref != 0.0
    for k in ec.UNREAD[key]:
        assert not S[k].any()
    # every read parameter has a non-zero row at each test point
    for theta in C.thetas[:3]:
        for x in C.points:
            ref = ec.complex_step(C, theta, x)
            assert all(np.any(ref[k]) for k in range(C.n_par) if k not in ec.UNREAD[key]), (key, theta)
    if key in ("P2", "E"):
        assert np.array_equal(union, S)             # nothing cancels structurally in these two
    # (P2U: the knot row of the state whose unit is the parameter is (p u) / u - (p u) / u - in the pattern, and zero up
    # to the rounding of the two quotients: containment is all that holds there)


def test_the_warning_about_an_unread_parameter_is_unchanged():
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        codegen.trace_problem(*pc.p2())
    texts = [str(w.message) for w in caught if issubclass(w.category, RuntimeWarning)]
    assert len(texts) == 1 and texts[0].startswith("parameter 'e' is declared but the traced callbacks never read it")


def test_an_operand_that_reads_a_parameter_is_in_the_work_lists():
    C = ec.case("P2U")
    plan = codegen.ParameterPlan(C.program)
    # the unit's state: tail and operand (3); the other state of each phase reads it through its dynamics term only (1)
    assert sorted(plan.slots[5]) == [(0, 3, 1), (1, 3, 3), (2, 4, 1), (3, 4, 3)]
    assert plan.entries == [9, 1, 9, 1, 0, 20]
    assert all(reads == 1 for k in range(5) for _, _, reads in plan.slots[k])


# ------------------------------------------------------------------------------------------------ 2. the host probe
@pytest.fixture(scope="module")
def probe_dir(tmp_path_factory):
    return str(tmp_path_factory.mktemp("par_exact_probe"))


def _note(key, worst):
    """The measured worst error of a case into profiles/params_exact.md (the case's line is replaced, not repeated)."""
    line = "| %s | %.1e |" % (key, worst)
    try:
        old = open(REPORT).read().split("\n") if os.path.exists(REPORT) else []
        if not old:
            old = ["# Exact dF/dtheta: the host probe of csrc/og_par.h against the complex step in theta", "",
                   "Worst difference over every parameter set and point of the case, in units of the row's largest entry",
                   "(bound: 1e-12).  Written by tests/test_parameter_exact.py.", "",
                   "| case | worst |", "|---|---|"]
        kept = [row for row in old if not row.startswith("| %s |" % key)]
        while kept and kept[-1] == "":
            kept.pop()
        with open(REPORT, "w") as fh:
            fh.write("\n".join(kept + [line]) + "\n")
    except OSError:
        pass


@pytest.mark.parametrize("key", KEYS)
def test_the_probe_equals_the_complex_step_and_the_twin(key, probe_dir, capsys):
    C = ec.case(key)
    S = codegen.parameter_sparsity(C.program)
    gxx = ec.build_probe(C, probe_dir, "g++")
    clang = ec.build_probe(C, probe_dir, og_math_cases.clangxx())
    san = ec.build_probe(C, probe_dir, "g++", sanitize=True)
    tw = twin.Twin(C.prob, C.obj, program=C.program, header=C.header)
    worst = 0.0
    for t, theta in enumerate(C.thetas):
        tw._cv[C.program.par_off:] = theta
        for i, x in enumerate(C.points):
            dF, F0 = ec.run_probe(C, gxx, probe_dir, theta, x)
            assert np.array_equal(F0, tw.values(x))
            outside = dF[~S]
            assert not outside.any() and not np.signbit(outside).any()        # exact +0.0 outside the pattern
            for other in ([clang] if (t, i) != (0, 0) else [clang, san]):         # (the sanitizer build: once per case)
                dF2, F02 = ec.run_probe(C, other, probe_dir, theta, x, "other")
                assert np.array_equal(dF2, dF) and np.array_equal(F02, F0)
            err = ec.worst_error(dF, ec.complex_step(C, theta, x))
            worst = max(worst, err)
            with capsys.disabled():
                if os.environ.get("OG_SURFACE_REPORT"):
                    print("parameter exact %-4s theta %d point %d %.2e" % (key, t, i, err))
            assert err <= ec.BOUND, (key, t, i, err)
    _note(key, worst)


# ------------------------------------------------------------------------------------------------ 3. host logic
class StandIn:
    """``Problem``'s engine protocol on the C++ twin (point by point, no ``batch``), with ``parameter_jacobian`` by the
    complex step at the parameters it was last given."""

    def __init__(self, prob, obj):
        self.C = ec.case("P2")
        self.tw = twin.Twin(prob, obj, program=pc.trace(prob, obj))
        self.m_eq = self.tw.m_eq
        self.theta = np.array(list(prob.parameters.values()), dtype=float)
        self.par_calls = []

    def set_parameters(self, theta):
        self.theta = np.asarray(theta, dtype=float).copy()
        self.tw._cv[self.tw.program.par_off:] = self.theta

    def values(self, p):
        F = self.tw.values(p)
        return F[0], F[1:1 + self.m_eq], F[1 + self.m_eq:]

    def jacobians(self, p, lb, ub):
        h = _native.fd_step(p, lb, ub)
        F0, JT = self.tw.sweep(p, h)
        J = JT.T
        return (J[0].copy(), J[1:1 + self.m_eq], J[1 + self.m_eq:]), h

    def exact_stacked(self, p):
        return self.tw.exact(p)

    def parameter_jacobian(self, x):
        self.par_calls.append((self.theta.copy(), np.array(x, dtype=float)))
        return ec.complex_step(self.C, self.theta, x), self.tw.values(x)


class NoExact(StandIn):
    parameter_jacobian = property()         # (hasattr is False)


def test_exact_sensitivity_is_one_engine_call_and_no_batch(monkeypatch):
    monkeypatch.setattr(optimize, "ENGINE_FACTORY", StandIn)
    prob, obj = pc.p2()
    C = ec.case("P2")
    x = C.points[0]
    got = prob.parameter_sensitivity(obj, x, exact=True)
    eng = prob._engine
    assert len(eng.par_calls) == 1 and np.array_equal(eng.par_calls[0][1], x)
    assert getattr(prob, "_batch", None) is None
    assert got.shape == (5, C.m) and np.array_equal(got, ec.complex_step(C, pc.P2_THETA[0], x))
    # the default is the forward-difference form it was: the same numbers with and without the keyword, no engine call
    fd = prob.parameter_sensitivity(obj, x)
    assert len(eng.par_calls) == 1
    assert np.array_equal(fd, prob.parameter_sensitivity(obj, x, exact=False))
    theta = pc.P2_THETA[0]
    h = _native.fd_step(theta, np.full(5, -np.inf), np.full(5, np.inf))
    base = eng.tw.values(x)
    for k in range(5):
        eng.set_parameters(theta + h[k] * (np.arange(5) == k))
        assert np.array_equal(fd[k], (eng.tw.values(x) - base) / h[k])
    eng.set_parameters(theta)
    assert np.max(np.abs(fd - got)) <= 1e-6 * max(1.0, np.abs(got).max())
    # at new values: the engine is told first
    prob.set_parameters(pc.P2_THETA[1])
    got = prob.parameter_sensitivity(obj, exact=True)
    assert np.array_equal(eng.par_calls[-1][0], pc.P2_THETA[1]) and np.array_equal(eng.par_calls[-1][1], prob.p)
    assert np.array_equal(got, ec.complex_step(C, pc.P2_THETA[1], prob.p))


def test_refusals(monkeypatch):
    monkeypatch.setattr(optimize, "ENGINE_FACTORY", NoExact)
    prob, obj = pc.p2()
    x = ec.case("P2").points[0]
    with pytest.raises(ValueError, match="no exact parameter Jacobian"):
        prob.parameter_sensitivity(obj, x, exact=True)
    with pytest.raises(ValueError, match="no exact parameter Jacobian"):
        prob.evaluate_batch(obj, x[None, :], parameter_jacobian=True)
    assert prob.parameter_sensitivity(obj, x).shape == (5, ec.case("P2").m)        # (the FD form needs no such method)
    plain, pobj = problems.build("brachistochrone")
    for call in (lambda: plain.parameter_sensitivity(pobj, exact=True),
                 lambda: plain.evaluate_batch(pobj, plain.p[None, :], parameter_jacobian=True)):
        with pytest.raises(ValueError, match="declares no parameter"):
            call()


@pytest.mark.parametrize("jacobian", [False, "fd", "exact"])
def test_evaluate_batch_gives_every_lane_its_own_parameters(jacobian, monkeypatch):
    monkeypatch.setattr(optimize, "ENGINE_FACTORY", StandIn)
    prob, obj = pc.p2()
    C = ec.case("P2")
    X = np.stack([C.points[0], C.points[1], C.points[0]])
    TH = np.stack(pc.P2_THETA)
    res = prob.evaluate_batch(obj, X, jacobian=jacobian, parameters=TH, parameter_jacobian=True)
    assert res.parameter_jacobian.shape == (3, 5, C.m) and np.array_equal(res.parameters, TH)
    for k in range(3):
        assert np.array_equal(res.parameter_jacobian[k], ec.complex_step(C, TH[k], X[k]))
    calls = prob._engine.par_calls
    assert [tuple(c[0]) for c in calls] == [tuple(t) for t in TH]
    # without the flag nothing is computed and the result is what it was
    plain = prob.evaluate_batch(obj, X, jacobian=jacobian, parameters=TH)
    assert plain.parameter_jacobian is None and len(prob._engine.par_calls) == 3
    assert np.array_equal(plain.cost, res.cost) and np.array_equal(plain.equality, res.equality)
    if jacobian:
        assert np.array_equal(plain.values, res.values)
    # one trajectory scanned over the parameter sets, and the engine back at the problem's values afterwards
    scan = prob.evaluate_batch(obj, X[:1], parameters=TH, parameter_jacobian=True)
    assert scan.parameter_jacobian.shape == (3, 5, C.m)
    assert np.array_equal(scan.parameter_jacobian[2], ec.complex_step(C, TH[2], X[0]))
    assert np.array_equal(prob._engine.theta, pc.P2_THETA[0])
