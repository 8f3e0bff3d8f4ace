"""Run-time parameters on the CPU: the tracer (``trace.Parameter``), the lowering (``codegen``: the parameter table is
the tail of the constant table and nothing looks at its values), both CPU oracles (the NumPy interpreter of the lowered
program and the C++ twin of the generated header) and the host logic of ``Problem`` (``set_parameter``,
``evaluate_batch(parameters=...)``, ``parameter_sensitivity``) on a stand-in engine.  The problems are those of
tests/parameter_cases.py.  The GPU side is tests/test_parameters_gpu.py."""
import json
import math
import os
import warnings

import numpy as np
import pytest

import parameter_cases as pc
from conftest import GOLDEN
from opengoddard_amd import _native, codegen, optimize, problems
from opengoddard_amd.trace import Parameter, TraceError
from oracle import np_path, program_eval, twin


def _make(key, **kw):
    return pc.p2(**kw) if key == "P2" else pc.goddard(int(key[1:]), **kw)


def _thetas(key):
    return pc.P2_THETA if key == "P2" else pc.G_THETA


# ------------------------------------------------------------------------------------------------ 1. header
@pytest.mark.parametrize("key", ["P2", "G17"])
def test_the_header_does_not_depend_on_the_parameter_values(key):
    prob, obj = _make(key)
    P = pc.trace(prob, obj)
    header = codegen.emit_header(P)
    n_par = len(prob.parameters)
    assert P.n_par == n_par and P.par_names == tuple(prob.parameters) and P.par_off + n_par == P.cvec.size
    assert np.array_equal(P.cvec[P.par_off:], _thetas(key)[0])
    assert "N_PAR = %d;" % n_par in header and "PAR_OFF = %d;" % P.par_off in header
    rng = np.random.default_rng(5)
    # (0 and 1 are what a simplifier would key on: x*1, x+0, x*0)
    for theta in (np.zeros(n_par), np.ones(n_par), rng.standard_normal(n_par) * 10.0, -np.ones(n_par)):
        prob.set_parameters(theta)
        P2 = pc.trace(prob, obj)
        assert codegen.emit_header(P2) == header, "the header changed with the parameter values %s" % theta
        assert np.array_equal(P2.cvec[P2.par_off:], theta)
    baked = codegen.emit_header(codegen.trace_problem(*_make(key, baked=True)))
    assert baked != header and "N_PAR" not in baked and "PAR_OFF" not in baked


# ------------------------------------------------------------------------------------------------ 2. parent-commit hashes
@pytest.mark.parametrize("name", problems.NAMES)
def test_a_problem_without_parameters_keeps_its_header(name):
    """The hashes were recorded on the commit before parameters existed: the module, its cache entry and every golden of
    an unparameterised problem are untouched."""
    with open(os.path.join(GOLDEN, "header_hashes_before_parameters.json")) as fh:
        want = json.load(fh)
    prob, obj = problems.build(name)
    P = codegen.trace_problem(prob, obj)
    assert P.n_par == 0 and P.par_names == ()
    assert codegen.program_hash(codegen.emit_header(P)) == want[name]


# ------------------------------------------------------------------------------------------------ 3. interpreter
def _graph_key(P):
    return (P.eg.nodes, P.pieces, P.n, P.m_eq, P.m_ineq, P.cvec_off, P.par_off, P.n_par,
            [(s.phase, s.length, s.operand, s.leaf_base) for s in P.mv])


@pytest.mark.parametrize("key", ["P2", "G9"])
def test_the_interpreter_equals_numpy_at_every_parameter_value(key):
    prob, obj = _make(key)
    P = pc.trace(prob, obj)                     # ONE program, traced once
    x = pc.point(prob)
    results = []
    for theta in _thetas(key):
        prob.set_parameters(theta)
        want = np_path.stacked_values(prob, obj, x)             # the callbacks on a plain array
        P.cvec[P.par_off:] = theta
        got = program_eval.evaluate(P, prob, x)
        assert np.array_equal(got, want), "theta = %s" % theta
        results.append(want)
    assert not np.array_equal(results[0], results[1])           # (the parameters do something)
    again = pc.trace(prob, obj)                                 # traced at another theta: the same graph
    assert _graph_key(again) == _graph_key(P)
    assert np.array_equal(again.cvec[:P.par_off], P.cvec[:P.par_off])


# ------------------------------------------------------------------------------------------------ 4. twin
@pytest.mark.parametrize("key", ["P2", "G9"])
def test_the_twin_follows_its_table(key):
    from test_oracle_and_codegen import _row_scales
    prob, obj = _make(key)
    tw = twin.Twin(prob, obj, program=pc.trace(prob, obj))
    x = pc.point(prob)
    for theta in _thetas(key):
        prob.set_parameters(theta)
        want = np_path.stacked_values(prob, obj, x)
        tw._cv[tw.program.par_off:] = theta
        got = tw.values(x)
        assert np.all(np.abs(got - want) <= 1e-9 * _row_scales(tw.program, prob, x, want)), "theta = %s" % theta


@pytest.mark.parametrize("nodes", [9, 17])
def test_the_parameterised_twin_equals_the_baked_twin_bit_for_bit(nodes):
    prob, obj = pc.goddard(nodes)
    tw = twin.Twin(prob, obj)
    x = pc.point(prob)
    lb, ub = np_path.bounds_arrays(prob)
    h = _native.fd_step(x, lb, ub)
    for theta in pc.G_THETA[1:]:
        tw._cv[tw.program.par_off:] = theta
        baked = twin.Twin(*pc.goddard(nodes, theta, baked=True))
        assert baked.header != tw.header
        assert np.array_equal(tw.values(x), baked.values(x))
        for a, b in zip(tw.sweep(x, h), baked.sweep(x, h)):
            assert np.array_equal(a, b)
        for a, b in zip(tw.exact(x), baked.exact(x)):
            assert np.array_equal(a, b)


# ------------------------------------------------------------------------------------------------ 5. baking is excluded
EXPRESSIONS = {
    "g0 * p": lambda obj, x, y: obj.g0 * obj.q,
    "p * 2.0": lambda obj, x, y: obj.q * 2.0,
    "2.0 / p": lambda obj, x, y: 2.0 / obj.q,
    "-p": lambda obj, x, y: -obj.q,
    "p ** 2": lambda obj, x, y: obj.q ** 2,
    "abs(p) + p": lambda obj, x, y: abs(obj.q) + obj.q,
    "np.sqrt(p)": lambda obj, x, y: np.sqrt(obj.q),
    "np.where(p > 1, x, y)": lambda obj, x, y: np.where(obj.q > 1, x, y),
    "np.maximum(x, p)": lambda obj, x, y: np.maximum(x, obj.q),
    "x - p": lambda obj, x, y: x - obj.q,
    "p - x": lambda obj, x, y: obj.q - x,
}


def _expression_problem(value):
    """One equality row (or one per node) per expression of ``EXPRESSIONS``."""
    prob = optimize.Problem([0.0, 1.0], [4], [1], [1], 1)
    obj = pc.Model()
    obj.g0 = 1.25
    obj.q = prob.parameter("q", value)
    prob.set_states(0, 0, np.array([0.5, 1.5, 2.5, 3.5]))
    prob.set_controls(0, 0, np.array([-1.0, 0.25, 4.0, 9.0]))

    def dynamics(prob, obj, section):
        rhs = optimize.Dynamics(prob, section)
        rhs[0] = prob.controls(0, section)
        return rhs()

    def equality(prob, obj):
        x, y = prob.states(0, 0), prob.controls(0, 0)
        rows = optimize.Condition()
        for fn in EXPRESSIONS.values():
            rows.add(fn(obj, x, y) + 0.0 * x[0])
        return rows()

    prob.dynamics = [dynamics]
    prob.cost = lambda prob, obj: prob.states(0, 0)[-1]
    prob.equality = equality
    prob.inequality = lambda prob, obj: optimize.Condition()()
    return prob, obj


def test_every_spelling_reads_the_table_entry():
    # (1.5 and 0.25: their squares are exact, so that Python's pow() outside a trace and x*x inside agree; they lie on
    # either side of the switch and of the states)
    prob, obj = _expression_problem(1.5)
    P = codegen.trace_problem(prob, obj)
    x = prob.p.copy()
    rows = {}
    for value in (1.5, 0.25):
        prob.set_parameter("q", value)
        want = np_path.stacked_values(prob, obj, x)
        P.cvec[P.par_off:] = value
        got = program_eval.evaluate(P, prob, x)
        assert np.array_equal(got, want), "q = %s" % value
        rows[value] = got
    # every expression's rows moved with the table entry: nothing was baked in at 1.5
    at, user = 1, {}
    for name, fn in EXPRESSIONS.items():
        ln = np.size(fn(obj, prob.states(0, 0), prob.controls(0, 0)) + 0.0 * x[0])
        user[name] = slice(at, at + ln)
        at += ln
    for name, sl in user.items():
        assert not np.array_equal(rows[1.5][sl], rows[0.25][sl]), "%s does not depend on the parameter" % name
    assert float(obj.q) == 0.25 and obj.q * 2.0 == 0.5 and isinstance(obj.q * 2.0, float)


# ------------------------------------------------------------------------------------------------ 6. errors and warnings
def _needs_a_number(kind):
    def use(prob, obj, x):
        if kind == "float":
            return x * float(obj.q)
        if kind == "math.sqrt":
            return x * math.sqrt(obj.q)
        if kind == "if":
            if obj.q > 0:
                return x * 2.0
            return x
        if kind == "index":
            return x[int(obj.q)] + x
        if kind == "length":
            return x + np.zeros(obj.q)[0]
        if kind == "derived if":
            if obj.q * 2.0 > 1.0:
                return x
            return -x
        raise AssertionError(kind)
    return use


@pytest.mark.parametrize("kind", ["float", "math.sqrt", "if", "index", "length", "derived if"])
def test_what_needs_the_number_raises_and_names_the_line(kind):
    prob, obj = _expression_problem(2.0)
    use = _needs_a_number(kind)
    prob.equality = lambda prob, obj: use(prob, obj, prob.states(0, 0))
    # outside a trace it is the plain callback that it looks like
    want = np_path.stacked_values(prob, obj, prob.p.copy())
    assert np.all(np.isfinite(want))
    with pytest.raises(TraceError) as err:
        codegen.trace_problem(prob, obj)
    text = str(err.value)
    assert "a parameter is a run-time value" in text and "np.where" in text
    assert os.path.basename(__file__) in text and "\n  at " in text and "obj.q" in text
    assert err.value.user_frame[0].endswith(os.path.basename(__file__))


def test_outside_a_trace_a_parameter_is_its_value():
    prob = optimize.Problem([0.0, 1.0], [4], [1], [1], 1)
    q = prob.parameter("q", 2.0)
    assert isinstance(q, Parameter) and not isinstance(q, float)
    assert float(q) == 2.0 and int(q) == 2 and math.sqrt(q) == math.sqrt(2.0) and bool(q > 0) and q == 2.0
    assert [10, 11, 12][q] == 12 and np.zeros(q).shape == (2,)
    for got, want in ((q * 3, 6.0), (3 * q, 6.0), (q / 4, 0.5), (1 / q, 0.5), (-q, -2.0), (q ** 2, 4.0), (2 ** q, 4.0),
                      (q - 1, 1.0), (1 - q, -1.0), (abs(-q), 2.0), (np.sqrt(q), np.sqrt(2.0)), (np.maximum(q, 3.0), 3.0)):
        assert got == want and isinstance(got, float)
    arr = np.arange(3.0)
    assert np.array_equal(arr * q, arr * 2.0) and np.array_equal(q * arr, arr * 2.0) and type(arr * q) is np.ndarray
    assert np.array_equal(np.where(arr > q, arr, q), np.where(arr > 2.0, arr, 2.0))
    prob.set_parameter("q", 0.5)
    assert float(q) == 0.5 and prob.parameters == {"q": 0.5}
    with pytest.raises(TypeError):
        [10, 11][q]


def test_declaring_and_setting_by_name():
    prob, obj = pc.p2()
    assert list(prob.parameters) == list(pc.P2_NAMES)
    assert prob.parameters == dict(zip(pc.P2_NAMES, pc.P2_THETA[0]))
    with pytest.raises(ValueError, match="already declared"):
        prob.parameter("a", 1.0)
    with pytest.raises(ValueError, match="unknown parameter"):
        prob.set_parameter("T_max", 1.0)
    with pytest.raises(ValueError, match="unknown parameter"):
        prob.set_parameters({"a": 1.0, "zeta": 2.0})
    with pytest.raises(ValueError):
        prob.set_parameters([1.0, 2.0])
    assert prob.parameters == dict(zip(pc.P2_NAMES, pc.P2_THETA[0]))        # (a refused call changes nothing)
    prob.set_parameters({"d": 0.5, "a": -1.0})
    assert prob.parameters["a"] == -1.0 and prob.parameters["d"] == 0.5 and float(obj.a) == -1.0
    with pytest.warns(RuntimeWarning, match="'e'"):
        codegen.trace_problem(prob, obj)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        codegen.trace_problem(*pc.goddard(9))                                # every parameter read: no warning
    # a parameter of another problem cannot be traced into this one
    other, _ = pc.p2()
    obj.a = other.parameter("stray", 1.0)
    with pytest.raises(TraceError, match="another Problem"):
        pc.trace(prob, obj)


def test_evaluate_batch_refuses_malformed_parameters():
    prob, obj = pc.p2()
    X = np.tile(prob.p, (3, 1))
    for bad in (np.zeros((3, 4)), np.zeros(5), np.zeros((2, 5)), {"zeta": 1.0}, {"a": np.zeros((3, 1))},
                {"a": np.zeros(3), "b": np.zeros(2)}, {"a": np.zeros(2)}):
        with pytest.raises(ValueError):
            prob.evaluate_batch(obj, X, parameters=bad)
    plain, obj2 = problems.build("brachistochrone")
    with pytest.raises(ValueError, match="declares no parameter"):
        plain.evaluate_batch(obj2, plain.p[None, :], parameters=np.zeros((1, 1)))


# ------------------------------------------------------------------------------------------------ 7. a stand-in engine
class TwinEngine:
    """``Problem``'s engine protocol on the C++ twin, parameters included; no ``batch``: served point by point."""

    def __init__(self, prob, obj):
        self.tw = twin.Twin(prob, obj, program=pc.trace(prob, obj))
        self.m_eq = self.tw.m_eq
        self.sets = []

    def set_parameters(self, theta):
        theta = np.asarray(theta, dtype=float)
        self.sets.append(theta.copy())
        self.tw._cv[self.tw.program.par_off:] = theta

    def values(self, p):
        F = self.tw.values(p)
        return F[0], F[1:1 + self.m_eq], F[1 + self.m_eq:]

    def jacobians(self, p, lb, ub):
        h = _native.fd_step(p, lb, ub)
        F0, JT = self.tw.sweep(p, h)
        J = JT.T
        return (J[0].copy(), J[1:1 + self.m_eq], J[1 + self.m_eq:]), h


@pytest.mark.parametrize("key", ["P2", "G9"])
def test_a_stand_in_engine_is_served_point_by_point(key, monkeypatch):
    monkeypatch.setattr(optimize, "ENGINE_FACTORY", TwinEngine)
    prob, obj = _make(key)
    thetas = np.stack(_thetas(key))
    names = list(prob.parameters)
    x = pc.point(prob)
    ref = twin.Twin(prob, obj, program=pc.trace(prob, obj))

    def row(theta, at=x):
        ref._cv[ref.program.par_off:] = theta
        return ref.values(at)

    # one trajectory, scanned
    res = prob.evaluate_batch(obj, x[None, :], parameters=thetas)
    assert len(res) == 3 and np.array_equal(res.parameters, thetas)
    for k in range(3):
        F = row(thetas[k])
        assert np.array_equal(np.concatenate([[res.cost[k]], res.equality[k], res.inequality[k]]), F)
    # afterwards the engine is back at the current values, and None means those
    assert np.array_equal(prob._engine.sets[-1], thetas[0])
    X = np.stack([pc.point(prob, seed) for seed in (1, 2)])
    res = prob.evaluate_batch(obj, X)
    assert np.array_equal(res.parameters, np.tile(thetas[0], (2, 1)))
    assert np.array_equal(res.equality[1], row(thetas[0], X[1])[1:1 + ref.m_eq])
    # by name: what is not named keeps its current value; with Jacobians
    res = prob.evaluate_batch(obj, X, jacobian=True, parameters={names[0]: thetas[1:, 0]})
    want = np.tile(thetas[0], (2, 1))
    want[:, 0] = thetas[1:, 0]
    assert np.array_equal(res.parameters, want)
    lb, ub = np_path.bounds_arrays(prob)
    for k in range(2):
        ref._cv[ref.program.par_off:] = want[k]
        F0, JT = ref.sweep(X[k], _native.fd_step(X[k], lb, ub))
        assert np.array_equal(res.values[k], JT.reshape(-1)) and np.array_equal(res.cost[k], F0[0])
    # the difference quotients, from the same rows
    prob.set_parameters(thetas[1])
    assert np.array_equal(prob._engine.sets[-1], thetas[1])                 # (a live engine follows set_parameters)
    dF = prob.parameter_sensitivity(obj, x)
    n_par = len(names)
    assert dF.shape == (n_par, ref.m)
    h = _native.fd_step(thetas[1], np.full(n_par, -np.inf), np.full(n_par, np.inf))
    F0 = row(thetas[1])
    for k in range(n_par):
        moved = thetas[1].copy()
        moved[k] += h[k]
        assert np.array_equal(dF[k], (row(moved) - F0) / h[k]), names[k]
    assert np.any(dF[0] != 0.0)
    if key == "P2":
        assert not dF[4].any()                                             # `e` is read by nothing

    # an engine that cannot change them
    prob2, obj2 = _make(key)
    monkeypatch.setattr(optimize, "ENGINE_FACTORY", lambda p, o: type("E", (), {"values": TwinEngine(p, o).values})())
    with pytest.raises(ValueError, match="cannot change parameters"):
        prob2.evaluate_batch(obj2, x[None, :], parameters=thetas)
