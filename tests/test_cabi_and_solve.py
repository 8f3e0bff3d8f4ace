"""C-ABI surface (no compute without a GPU), solve() host logic with the oracle engine injected,
and the fail-loudly contract of the product path."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT, has_gpu
from opengoddard_amd import _native, build, problems
from opengoddard_amd import optimize as og


def test_library_exports_every_symbol_the_header_declares():
    with open(os.path.join(ROOT, "include", "ogpsx.h")) as fh:
        text = re.sub(r"/\*.*?\*/", "", fh.read(), flags=re.S)
    declared = set(re.findall(r"\b(og_[a-z_0-9]+)\s*\(", text))
    assert declared, "no declarations parsed"
    assert declared == set(_native.SIGNATURES), declared ^ set(_native.SIGNATURES)
    raw = C.CDLL(build.build_core())
    for name in sorted(declared):
        assert getattr(raw, name) is not None
    _native.lib()


def test_error_reporting_without_compute():
    lib = _native.lib()
    assert lib.og_lgl(2, None, None, None) != 0
    assert b"N must be >= 3" in lib.og_last_error()
    handle = C.c_void_p()
    desc = _native.OgDesc(abi_version=999, device=0, n=1, m_eq=0, m_ineq=0, n_phase=1)
    assert lib.og_problem_create(C.byref(desc), C.byref(handle)) != 0
    assert b"ABI" in lib.og_last_error()
    assert not handle.value
    lib.og_problem_destroy(None)                 # destroying a null handle is a no-op
    assert lib.og_device_count() >= 0


@pytest.mark.skipif(has_gpu(), reason="only meaningful on a machine without a GPU")
def test_product_path_fails_loudly_without_gpu():
    """No silent CPU fallback: solve() must raise when the HIP engine cannot run."""
    prob, obj = problems.build("brachistochrone")
    assert og.ENGINE_FACTORY is None
    with pytest.raises(RuntimeError, match="no HIP device"):
        prob.solve(obj)


@pytest.fixture
def oracle_engine():
    from oracle import np_path
    og.ENGINE_FACTORY = np_path.NumpyEngine
    yield
    og.ENGINE_FACTORY = None


def test_kkt_oracle_tells_an_optimum_from_a_start(oracle_engine, capsys):
    """oracle/kkt.py (the checker of the converged solves on the GPU box, tests/test_gpu_solve.py and bench.py's solve
    leg) on the two configurations SciPy's own core finishes here: at the optimum SciPy returns every residual is
    small (the reference's ftol of 1e-6 leaves 1e-4 of stationarity at C1; C2 with ftol 1e-8: 1.3e-4, with 1e-10: 5e-6), at the initial guess the
    same function reports an infeasible, non-stationary point; a degenerate active set (C2's singular arc: 42 rows at
    zero, 6 of them priced negative by a plain least-squares fit) is handled by releasing those rows."""
    from oracle import kkt, np_path
    for name, opts, bound in (("brachistochrone", {}, 2e-4), ("goddard", {"ftol": 1e-8}, 5e-4)):
        prob, obj = problems.build(name)
        prob.solve(obj, sqp_core="scipy", **opts)
        capsys.readouterr()
        assert prob.last_result.status == 0
        k = kkt.residuals(prob, obj, prob.last_result.x, prob._engine.m_eq)
        assert k["kkt"] <= bound and k["feasibility"] <= 1e-8 and k["dual"] == 0.0, k
        assert abs(k["cost"] - prob.last_result.fun) <= 1e-12
        fresh, obj2 = problems.build(name)
        lb, ub = np_path.bounds_arrays(fresh)
        k0 = kkt.residuals(fresh, obj2, np.clip(fresh.p, lb, ub), prob._engine.m_eq)
        assert k0["kkt"] >= 0.5 and k0["feasibility"] >= 0.5
        # a point that is feasible but not optimal: the optimum with its final time stretched is caught by stationarity
        # or feasibility, never passed
        x = prob.last_result.x.copy()
        x[-1] *= 1.05
        assert kkt.residuals(prob, obj, x, prob._engine.m_eq)["kkt"] >= 1e-3


def test_solve_host_logic_brachistochrone(oracle_engine, capsys):
    """Restart loop, jac= plumbing, caching and quirk Q13 with the oracle engine injected:
    converges to the known answer tf = sqrt(pi) (reference: 1.77245410898455)."""
    prob, obj = problems.build("brachistochrone")
    calls = []
    prob.solve(obj, lambda: calls.append(prob.time_final(-1)))
    out = capsys.readouterr().out
    assert "---- iteration : 1 ----" in out and "Optimization terminated successfully" in out
    assert abs(prob.time_final(-1) - 1.7724541) < 2e-6
    assert abs(prob.time_final(-1) - np.sqrt(np.pi)) < 1e-5
    assert len(calls) == prob.iterator + 1 and prob.iterator < prob.maxIterator
    x = prob.states_all_section(0)
    assert abs(x[0]) < 1e-8 and abs(x[-1] - 1.0) < 1e-8


def test_solve_options_and_q13(oracle_engine, capsys):
    prob, obj = problems.build("goddard")
    prob.maxIterator = 2
    prob.solve(obj, maxiter=2, ftol=1e-10)
    out = capsys.readouterr().out
    assert out.count("---- iteration") == 2 and "Iteration limit reached" in out
    assert prob.iterator == 2
    # exit mode 9: the last callback was a Jacobian request -> p[-1] carries the FD step (Q13)
    frac = prob.p[-1]
    assert isinstance(prob.p, np.ndarray) and np.isfinite(frac)


@pytest.mark.reference
@pytest.mark.parametrize("tag,script", [
    ("ex01", "01_Brachistochrone_Problem.py"), ("ex02", "02_Brachistochrone_TokyoOsaka.py"),
    ("ex03", "03_2d_simple_rocket.py"), ("ex04", "04_Goddard_0knot.py"),
    ("ex05", "05_Goddard_1knot.py"), ("ex06", "06_Rocket_Ascent_SingleStage.py"),
    ("ex07", "07_Rocket_Ascent_TwoStage.py"), ("ex08", "08_Rocket_Ascent_Polar_SSTO.py"),
    ("ex09", "09_Rocket_Ascent_Polar_TSTO.py"), ("ex10", "10_Low_Thrust_Orbit_Transfer.py"),
    ("ex11", "11_Polar_TSTO_Taiki.py")])
def test_shipped_example_scripts_run_unmodified(tag, script, golden, lgl_golden, oracle_engine,
                                                monkeypatch, tmp_path):
    """API conformance (build container only): the reference's example script, executed
    against THIS package's ``OpenGoddard`` import path, must hand SciPy callables whose values
    and Jacobians equal the goldens captured from the reference itself - bit for bit once the
    reference's LGL data is injected.  Also checks that the script's callbacks trace."""
    import runpy
    import sys
    from scipy import optimize as sciopt
    from conftest import inject_reference_lgl
    from opengoddard_amd import codegen
    from oracle import np_path, program_eval
    os.environ["MPLBACKEND"] = "Agg"
    sys.dont_write_bytecode = True
    got = {}

    class Stop(Exception):
        pass

    def fake_minimize(fun, x0, args=(), bounds=None, constraints=(), jac=None, **kw):
        got.update(fun=fun, x0=np.array(x0), args=args, bounds=bounds, constraints=constraints,
                   jac=jac)
        raise Stop()

    monkeypatch.setattr(sciopt, "minimize", fake_minimize)
    # example 11 reads its CSV tables relative to the examples directory (read-only)
    monkeypatch.chdir("/root/reference/examples" if tag == "ex11" else tmp_path)
    assert sys.modules.get("OpenGoddard.optimize") is None or \
        sys.modules["OpenGoddard.optimize"].__file__.startswith(ROOT)
    with pytest.raises(Stop):
        runpy.run_path(os.path.join("/root/reference/examples", script), run_name="__conformance__")
    G = golden(tag)
    prob, obj = got["args"]
    assert type(prob).__module__ == "opengoddard_amd.optimize"
    lb, ub = np_path.bounds_arrays(prob)
    assert np.array_equal(lb, G["lb"]) and np.array_equal(ub, G["ub"])
    assert np.max(np.abs(np.clip(got["x0"], lb, ub) - G["x"][0])) <= 1e-13
    inject_reference_lgl(prob, lgl_golden)
    prob._engine.m_eq = None
    m_eq = int(G["m_eq"])
    for k in range(G["x"].shape[0]):
        x, Fg = G["x"][k], G["F"][k]
        vals = [got["fun"](x, *got["args"]), got["constraints"][0]["fun"](x, *got["args"]),
                got["constraints"][1]["fun"](x, *got["args"])]
        assert np.array_equal(np.concatenate([np.atleast_1d(v) for v in vals]), Fg)
    if G["cols"].size == G["x"].shape[1]:                   # full Jacobians stored
        x = G["x"][0]
        Jeq = got["constraints"][0]["jac"](x, *got["args"])
        Jin = got["constraints"][1]["jac"](x, *got["args"])
        assert np.array_equal(Jeq, G["JT"][0].T[1:1 + m_eq])
        assert np.array_equal(Jin, G["JT"][0].T[1 + m_eq:])
    # and the unmodified callbacks are traceable into device code
    P = codegen.trace_problem(prob, obj)
    assert np.array_equal(program_eval.evaluate(P, prob, G["x"][1]), G["F"][1])
    assert "struct OgGen" in codegen.emit_header(P)


@pytest.mark.parametrize("tag,name", [("ex01", "brachistochrone"), ("ex04", "goddard"), ("ex05", "goddard_1knot"),
                                      ("ex08", "polar_ssto"), ("ex09", "polar_tsto_shipped"),
                                      ("ex10", "low_thrust_shipped")])
def test_reauthored_examples_through_the_opengoddard_import_path(tag, name, golden, lgl_golden, oracle_engine,
                                                                 monkeypatch):
    """The same conformance as above without the reference's scripts: the examples this repository re-authors
    (opengoddard_amd/problems), built on the ``OpenGoddard.optimize`` import path and started with ``prob.solve``, must
    hand SciPy callables whose values and Jacobians equal the goldens captured from the reference's own example
    scripts (``ex*.npz``) - bit for bit once the reference's LGL data is injected."""
    from scipy import optimize as sciopt
    from conftest import inject_reference_lgl
    from OpenGoddard import optimize as api
    from oracle import np_path
    got = {}

    class Stop(Exception):
        pass

    def fake_minimize(fun, x0, args=(), bounds=None, constraints=(), jac=None, **kw):
        got.update(fun=fun, x0=np.array(x0), args=args, bounds=bounds, constraints=constraints, jac=jac)
        raise Stop()

    monkeypatch.setattr(sciopt, "minimize", fake_minimize)
    prob, obj = problems.build(name, api=api)
    with pytest.raises(Stop):
        prob.solve(obj)
    G = golden(tag)
    assert got["args"][0] is prob and type(prob).__module__ == "opengoddard_amd.optimize"
    lb, ub = np_path.bounds_arrays(prob)
    assert np.array_equal(lb, G["lb"]) and np.array_equal(ub, G["ub"])
    assert np.max(np.abs(np.clip(got["x0"], lb, ub) - G["x"][0])) <= 1e-13
    inject_reference_lgl(prob, lgl_golden)
    prob._engine.m_eq = None
    m_eq = int(G["m_eq"])
    for k in range(G["x"].shape[0]):
        x, Fg = G["x"][k], G["F"][k]
        vals = [got["fun"](x, *got["args"]), got["constraints"][0]["fun"](x, *got["args"]),
                got["constraints"][1]["fun"](x, *got["args"])]
        assert np.array_equal(np.concatenate([np.atleast_1d(v) for v in vals]), Fg)
    if G["cols"].size == G["x"].shape[1]:                   # full Jacobians stored
        x = G["x"][0]
        Jeq = got["constraints"][0]["jac"](x, *got["args"])
        Jin = got["constraints"][1]["jac"](x, *got["args"])
        assert np.array_equal(Jeq, G["JT"][0].T[1:1 + m_eq])
        assert np.array_equal(Jin, G["JT"][0].T[1 + m_eq:])


@pytest.mark.parametrize("name,delimiter,tag", [("brachistochrone", ",", ""), ("polar_tsto_shipped", ",", ""),
                                                 ("polar_tsto_shipped", ";", "_semicolon")])
def test_to_csv_writes_the_reference_bytes(name, delimiter, tag, lgl_golden, tmp_path, capsys):
    """``Problem.to_csv`` (the reference's wire format, ``optimize.py:844-863``) against
    files written by the reference itself (tools/make_golden_csv.py): header text, delimiter, ``%.18e``, column order
    and - with the reference's own LGL nodes injected - every byte.  With this package's nodes the file has the same
    shape and differs only in the time column's last place."""
    from conftest import inject_reference_lgl
    want = open(os.path.join(ROOT, "tests", "golden", "to_csv_%s%s.csv" % (name, tag)), "rb").read()

    def write(inject):
        prob, obj = problems.build(name)
        if inject:
            inject_reference_lgl(prob, lgl_golden)
        rng = np.random.default_rng(20260928)                  # the point of tools/make_golden_csv.py: move()
        prob.p = rng.uniform(0.1, 1.0, prob.p.size)
        prob.p[-prob.number_of_section:] = np.cumsum(rng.uniform(0.2, 0.7, prob.number_of_section))
        path = tmp_path / ("out_%d.csv" % inject)
        prob.to_csv(str(path), delimiter=delimiter)
        assert 'Completed saving "%s"' % path in capsys.readouterr().out       # the reference's message
        return open(path, "rb").read()

    assert write(True) == want
    own = write(False)
    own_lines, want_lines = own.decode().splitlines(), want.decode().splitlines()
    assert own_lines[0] == want_lines[0] and len(own_lines) == len(want_lines)
    a = np.array([[float(v) for v in line.split(delimiter)] for line in own_lines[1:]])
    b = np.array([[float(v) for v in line.split(delimiter)] for line in want_lines[1:]])
    assert np.array_equal(a[:, 1:], b[:, 1:])                                   # states and controls: the same numbers
    assert np.max(np.abs(a[:, 0] - b[:, 0])) <= 4e-15 * max(1.0, np.abs(b[:, 0]).max())


def test_auto_falls_back_to_scipys_core_when_the_hip_core_cannot_take_the_problem(monkeypatch, capsys):
    """``sqp_core="auto"`` must never turn a problem the reference's core solves into an error.  The
    HIP SQP core needs torch with a GPU and has capacity limits (include/ogsqp.h); ``sqp.prepare`` says why it cannot
    run, ``Problem.solve`` then warns, records the reason and hands the solve to SciPy's SLSQP."""
    import types
    from opengoddard_amd import sqp
    from oracle import np_path
    try:                                              # torch without a GPU - on a machine with one as well
        import torch
        monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    except ImportError:
        pass
    assert "16384" in sqp.prepare(types.SimpleNamespace(n=17000, m_eq=10))
    assert "null space" in sqp.prepare(types.SimpleNamespace(n=8000, m_eq=100))
    # the edges themselves (og_qp_create refuses the same two shapes: tests/test_qp_wide_rows.py, on the device): one
    # variable beyond the longest row with the null space at its limit, and the longest row with one equality too few
    assert (sqp.MAX_N1, sqp.MAX_NULL_SPACE) == (16384, 6736)
    assert "16384" in sqp.prepare(types.SimpleNamespace(n=16384, m_eq=9649))
    assert "null space of the equalities (6737)" in sqp.prepare(types.SimpleNamespace(n=16383, m_eq=9647))
    for accepted in (types.SimpleNamespace(n=16383, m_eq=9648), types.SimpleNamespace(n=300, m_eq=100)):
        reason = sqp.prepare(accepted)                # (inside both limits: the next question is the device)
        assert reason is not None and ("GPU" in reason or "torch" in reason)

    class Engine(np_path.NumpyEngine):                # an engine "auto" would give the HIP core (n >= AUTO_HIP_FROM)
        def __init__(self, prob, obj):
            super().__init__(prob, obj)
            self.n = int(prob.number_of_variables)
            self.m_eq, self.m_ineq, self.device = 213, 160, 0
            self.m = 1 + self.m_eq + self.m_ineq

    monkeypatch.setattr(og, "_default_engine", lambda prob, obj, devices=None: Engine(prob, obj))
    prob, obj = problems.build("polar_tsto_shipped")
    assert prob.number_of_variables >= og.AUTO_HIP_FROM
    prob.maxIterator = 1
    with pytest.warns(RuntimeWarning, match="HIP SQP core is not available"):
        prob.solve(obj, maxiter=2)
    capsys.readouterr()
    assert prob.sqp_core_used == "scipy" and prob.sqp_core_fallback == reason
    assert prob.last_result.nit == 2
    # forcing the core does not fall back: it fails loudly
    prob2, obj2 = problems.build("polar_tsto_shipped")
    prob2.maxIterator = 1
    with pytest.raises((RuntimeError, ImportError)):
        prob2.solve(obj2, maxiter=2, sqp_core="hip")
    capsys.readouterr()
