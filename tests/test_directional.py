"""Exact directional derivatives ``F'(x) v`` without a GPU: the host probe of ``csrc/og_dir.h`` (the one function the
kernels compute every entry with) against two references, the host logic of ``Problem.directional_derivative`` /
``evaluate_batch(directions=)`` on a stand-in engine, and the build of the directional part.  The cases, the references
and the probe's build are in ``directional_cases``.

Reference 1: the complex step ``Im F(x + i 1e-30 v) / 1e-30`` of the lowered program (oracle/exact_jac.py).  Reference 2:
``J v`` accumulated in ``np.longdouble`` with ``J`` from the twin's ``exact(x)``.  The error is measured per row in units
of ``max(1, sum_j |J_rj v_j|)`` and bounded by ``1e-12`` (``test_exact_surface.BOUND``) at every case, parameter set,
point and direction.  Measured worst per case (g++; this file writes them to profiles/directional.md): at most 1.3e-15
(table_ascent), 8e-16 or less on the seven others.
"""
import os

import numpy as np
import pytest

import directional_cases as dc
import og_math_cases
import parameter_exact_cases as ec
from opengoddard_amd import build, optimize, problems
from oracle import twin

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REPORT = os.path.join(ROOT, "profiles", "directional.md")


@pytest.fixture(scope="module")
def probe_dir(tmp_path_factory):
    return str(tmp_path_factory.mktemp("dir_probe"))


def _note(key, worst):
    """The measured worst error of a case into profiles/directional.md (the case's line is replaced, not repeated)."""
    line = "| %s | %.1e |" % (key, worst)
    try:
        old = open(REPORT).read().split("\n") if os.path.exists(REPORT) else []
        if not old:
            old = ["# Exact F'(x) v: the host probe of csrc/og_dir.h against the complex step and the twin's J v", "",
                   "Worst difference from either reference over every parameter set, point and direction of the case, per",
                   "row in units of max(1, sum_j |J_rj v_j|) (bound: 1e-12).  Written by tests/test_directional.py.", "",
                   "| case | worst |", "|---|---|"]
        kept = [row for row in old if not row.startswith("| %s |" % key)]
        while kept and kept[-1] == "":
            kept.pop()
        with open(REPORT, "w") as fh:
            fh.write("\n".join(kept + [line]) + "\n")
    except OSError:
        pass


# ------------------------------------------------------------------------------------------------ 1. the host probe
@pytest.mark.parametrize("key", dc.CPU_KEYS)
def test_the_probe_equals_the_complex_step_and_the_twin(key, probe_dir, capsys):
    C = dc.case(key)
    gxx = dc.build_probe(C, probe_dir, "g++")
    clang = dc.build_probe(C, probe_dir, og_math_cases.clangxx())
    san = dc.build_probe(C, probe_dir, "g++", sanitize=True)
    tw = twin.Twin(C.prob, C.obj, program=C.program, header=C.header)
    V = C.directions()
    n = C.n
    assert V.shape == (7, n) and V[0, 0] == 1 and V[1, n - 1] == 1 and V[2, n - len(C.prob.nodes)] == 1
    assert np.all(np.abs(V[3:6]).max(axis=1) == 1.0) and not V[6].any()
    worst = 0.0
    for t, theta in enumerate(C.thetas):
        if theta is not None:
            tw._cv[C.program.par_off:] = theta
        for i, x in enumerate(C.points):
            # (run_probe: the probe pre-fills with NaN and fails unless every row of every direction is written once)
            dF, F0 = dc.run_probe(C, gxx, probe_dir, x, V, theta)
            assert np.all(np.isfinite(dF)), (key, t, i)
            F0t, JT = tw.exact(x)
            assert np.array_equal(F0, tw.values(x)) and np.array_equal(F0, F0t), (key, t, i)
            for other in ([clang] if (t, i) != (0, 0) else [clang, san]):         # (the sanitizer build: once per case)
                dF2, F02 = dc.run_probe(C, other, probe_dir, x, V, theta, "other")
                assert np.array_equal(dF2, dF) and np.array_equal(F02, F0), (key, t, i, other)
            assert not dF[6].any(), "the zero direction"
            prod, scale = dc.twin_product(JT, V)
            err_c = dc.worst_error(dF, dc.complex_step(C, x, V, theta), scale)
            err_t = dc.worst_error(dF, prod, scale)
            # v = e_j: column j of the twin's exact Jacobian (scale: max(1, |J_rj|))
            for d, j in ((0, 0), (1, n - 1), (2, n - len(C.prob.nodes))):
                err_t = max(err_t, dc.worst_error(dF[d], JT[j], np.maximum(1.0, np.abs(JT[j]))))
            worst = max(worst, err_c, err_t)
            with capsys.disabled():
                if os.environ.get("OG_SURFACE_REPORT"):
                    print("directional %-16s theta %d point %d complex step %.2e twin %.2e" % (key, t, i, err_c, err_t))
            assert err_c <= dc.BOUND and err_t <= dc.BOUND, (key, t, i, err_c, err_t)
    _note(key, worst)


def test_a_direction_alone_gives_the_bits_it_gives_among_others(probe_dir):
    C = dc.case("ragged_two_phase")
    exe = dc.build_probe(C, probe_dir, "g++")
    V = C.directions()
    dF, F0 = dc.run_probe(C, exe, probe_dir, C.points[1], V)
    for d in (0, 4):
        one, F1 = dc.run_probe(C, exe, probe_dir, C.points[1], V[d], tag="one")
        assert one.shape == (1, C.m) and np.array_equal(one[0], dF[d]) and np.array_equal(F1, F0)


def test_no_parameter_derivative_leaks_in(probe_dir):
    """P2U reads parameters in tails, rows and a collocation operand.  ``OgDirX`` has no ``par_seed``: a parameter leaf
    is the plain table entry (the values come through ``cv`` only).  An accessor that has the member, set to no
    parameter's index, makes every leaf a dual number with a zero derivative: the same bits.  And the parameters do move
    the result (the test would pass trivially otherwise)."""
    C = dc.case("P2U")
    exe = dc.build_probe(C, probe_dir, "g++")
    V = C.directions()
    for theta in C.thetas:
        for x in C.points[:2]:
            plain, F0 = dc.run_probe(C, exe, probe_dir, x, V, theta)
            seeded, F1 = dc.run_probe(C, exe, probe_dir, x, V, theta, tag="seeded", seeded=True)
            assert np.array_equal(plain, seeded) and np.array_equal(F0, F1)
    a = dc.run_probe(C, exe, probe_dir, C.points[0], V, C.thetas[0])[0]
    b = dc.run_probe(C, exe, probe_dir, C.points[0], V, C.thetas[1])[0]
    assert not np.array_equal(a, b)


# ------------------------------------------------------------------------------------------------ 2. host logic
class StandIn:
    """``Problem``'s engine protocol on the C++ twin (point by point, no ``batch``), with ``directional`` by the complex
    step at the parameters it was last given."""

    KEY = "P2U"

    def __init__(self, prob, obj):
        self.C = dc.case(self.KEY)
        self.tw = twin.Twin(prob, obj, program=self.C.program, header=self.C.header)
        self.m_eq = self.tw.m_eq
        self.theta = np.array(list(prob.parameters.values()), dtype=float)
        self.tw._cv[self.C.program.par_off:] = self.theta
        self.dir_calls = []

    def set_parameters(self, theta):
        self.theta = np.asarray(theta, dtype=float).copy()
        self.tw._cv[self.C.program.par_off:] = self.theta

    def values(self, p):
        F = self.tw.values(p)
        return F[0], F[1:1 + self.m_eq], F[1 + self.m_eq:]

    def exact_stacked(self, p):
        return self.tw.exact(p)

    def directional(self, x, V):
        self.dir_calls.append((self.theta.copy(), np.array(x, dtype=float), np.array(V, dtype=float)))
        return dc.complex_step(self.C, x, V, self.theta), self.tw.values(x)


class NoDirectional(StandIn):
    directional = property()            # (hasattr is False)


def test_directional_derivative_shapes_and_one_engine_call(monkeypatch):
    monkeypatch.setattr(optimize, "ENGINE_FACTORY", StandIn)
    C = dc.case("P2U")
    prob, obj = ec.CASES["P2U"][0]()
    x, V = C.points[0], C.directions()
    got = prob.directional_derivative(obj, V, x)
    eng = prob._engine
    assert got.shape == (7, C.m) and len(eng.dir_calls) == 1 and getattr(prob, "_batch", None) is None
    assert np.array_equal(eng.dir_calls[0][1], x) and np.array_equal(eng.dir_calls[0][2], V)
    assert np.array_equal(got, dc.complex_step(C, x, V, C.thetas[0]))
    one = prob.directional_derivative(obj, V[3], x)                 # the 1-D form
    # (the stand-in's NumPy products depend on the number of columns in the last bits: its own answer for one direction)
    assert one.shape == (C.m,) and np.array_equal(one, dc.complex_step(C, x, V[3], C.thetas[0])[0])
    assert eng.dir_calls[-1][2].shape == (1, C.n) and np.array_equal(eng.dir_calls[-1][2][0], V[3])
    at_p = prob.directional_derivative(obj, V[4])                   # the default point: prob.p
    assert np.array_equal(eng.dir_calls[-1][1], prob.p) and at_p.shape == (C.m,)
    prob.set_parameters(C.thetas[1])                                # at new values: the engine is told first
    got = prob.directional_derivative(obj, V[:2], x)
    assert np.array_equal(eng.dir_calls[-1][0], C.thetas[1])
    assert np.array_equal(got, dc.complex_step(C, x, V[:2], C.thetas[1]))


def test_refusals(monkeypatch):
    C = dc.case("P2U")
    x, V = C.points[0], C.directions()
    monkeypatch.setattr(optimize, "ENGINE_FACTORY", StandIn)
    prob, obj = ec.CASES["P2U"][0]()
    for bad in (V[0][:-1], V[:, :-1], np.zeros((0, C.n)), np.zeros((2, 2, C.n)), np.append(V[0], 0.0)):
        with pytest.raises(ValueError, match="directions must have"):
            prob.directional_derivative(obj, bad, x)
    X = np.stack([x, C.points[1]])
    with pytest.raises(ValueError, match="directions must have shape"):
        prob.evaluate_batch(obj, X, directions=V[:2, :-1])
    with pytest.raises(ValueError, match="directions must have shape"):
        prob.evaluate_batch(obj, X, directions=V[0])
    with pytest.raises(ValueError, match="directions holds 3 rows for 2 points"):
        prob.evaluate_batch(obj, X, directions=V[:3])
    assert getattr(prob, "_engine", None) is None                  # refused before any engine exists
    monkeypatch.setattr(optimize, "ENGINE_FACTORY", NoDirectional)
    prob, obj = ec.CASES["P2U"][0]()
    with pytest.raises(ValueError, match="no exact directional derivative"):
        prob.directional_derivative(obj, V, x)
    with pytest.raises(ValueError, match="no exact directional derivative"):
        prob.evaluate_batch(obj, X, directions=V[:2])
    assert prob.evaluate_batch(obj, X).directional is None          # (nothing else needs the method)


@pytest.mark.parametrize("jacobian", [False, "exact"])
def test_evaluate_batch_differentiates_every_lane_along_its_own_row(jacobian, monkeypatch):
    monkeypatch.setattr(optimize, "ENGINE_FACTORY", StandIn)
    C = dc.case("P2U")
    prob, obj = ec.CASES["P2U"][0]()
    X = np.stack([C.points[0], C.points[1], C.points[0]])
    V = C.directions()[3:6]
    TH = np.stack([C.thetas[1], C.thetas[0], C.thetas[1]])
    res = prob.evaluate_batch(obj, X, jacobian=jacobian, parameters=TH, directions=V)
    assert res.directional.shape == (3, C.m)
    for k in range(3):
        assert np.array_equal(res.directional[k], dc.complex_step(C, X[k], V[k], TH[k])[0])
    calls = prob._engine.dir_calls
    assert len(calls) == 3 and [tuple(c[0]) for c in calls] == [tuple(t) for t in TH]
    assert all(c[2].shape == (1, C.n) and np.array_equal(c[2][0], V[k]) for k, c in enumerate(calls))
    # directions=None is the default: no engine call, and the result is what it was
    plain = prob.evaluate_batch(obj, X, jacobian=jacobian, parameters=TH)
    assert plain.directional is None and len(prob._engine.dir_calls) == 3
    assert np.array_equal(plain.cost, res.cost) and np.array_equal(plain.equality, res.equality)
    assert np.array_equal(plain.inequality, res.inequality)
    if jacobian:
        assert np.array_equal(plain.values, res.values)
    # without parameters= every lane is at the problem's values; the engine is back at them afterwards
    res = prob.evaluate_batch(obj, X, directions=V)
    assert np.array_equal(res.directional[1], dc.complex_step(C, X[1], V[1], C.thetas[0])[0])
    assert np.array_equal(prob._engine.theta, C.thetas[0])
    # one trajectory scanned over the parameter sets: its one direction goes with it
    scan = prob.evaluate_batch(obj, X[:1], parameters=TH, directions=V[:1])
    assert scan.directional.shape == (3, C.m)
    assert np.array_equal(scan.directional[2], dc.complex_step(C, X[0], V[0], TH[2])[0])


def test_a_real_engine_without_the_keyword_is_not_asked_for_anything_new():
    """``directions=None`` on an engine WITH a batch: ``BatchSweep.directional`` is not called (a batch object that
    would raise if it were)."""
    class Batch:
        capacity, engine, pattern = 2, None, None

        class _handle:
            value = 1

        def values(self, P):
            return np.zeros((P.shape[0], 3))

        def directional(self, X, V):
            raise AssertionError("directional was called")

    class Engine:
        m_eq, n_par = 1, 0

        def batch(self, B):
            bt = Batch()
            bt.engine = self
            return bt

    prob, obj = problems.build("brachistochrone")
    prob._engine = Engine()
    res = prob.evaluate_batch(obj, np.stack([prob.p, prob.p]))
    assert res.directional is None and res.cost.shape == (2,)
    with pytest.raises(AssertionError, match="directional was called"):
        prob.evaluate_batch(obj, np.stack([prob.p, prob.p]), directions=np.zeros((2, prob.number_of_variables)))
    prob._engine = None


# ------------------------------------------------------------------------------------------------ 3. the build
def test_the_directional_part_is_a_file_of_its_own(monkeypatch, tmp_path):
    assert build.DIRECTIONAL_PART == 7
    assert (build.MODULE_PARTS, build.BATCH_PART, build.BATCH_EXACT_PART, build.PARAMETER_PART) == ((0, 2, 3, 1), 4, 5, 6)
    out = build.module_path("0123456789abcdef")
    others = [build.part_path(out, i) for i in range(len(build.MODULE_PARTS))] + [
        build.batch_part_path(out), build.batch_exact_part_path(out), build.parameter_part_path(out)]
    assert build.directional_part_path(out).endswith(".dir.so") and build.directional_part_path(out) not in others
    # asking for the part compiles that file alone (OGK_PART=7) and leaves every other file of the folder as it is
    monkeypatch.setattr(build, "JITDIR", str(tmp_path))
    header = dc.case("B5").header
    mod = build.module_path(build.module_digest(header))
    assert os.path.dirname(mod) == str(tmp_path)
    stale = {}
    for path in [build.part_path(mod, i) for i in range(4)] + [build.batch_part_path(mod), build.parameter_part_path(mod)]:
        with open(path, "w") as fh:
            fh.write("untouched " + os.path.basename(path))
        stale[path] = os.stat(path).st_mtime_ns
    commands = []

    def run(cmd):
        commands.append(cmd)
        with open(cmd[cmd.index("-o") + 1], "w") as fh:
            fh.write("part")
    monkeypatch.setattr(build, "_run", run)
    part = build.build_directional_part(header)
    assert part == build.directional_part_path(mod) and os.path.exists(part)
    assert len(commands) == 1 and "-DOGK_PART=7" in commands[0]
    for path, stamp in stale.items():
        assert os.stat(path).st_mtime_ns == stamp and open(path).read() == "untouched " + os.path.basename(path)
    made = set(os.listdir(str(tmp_path))) - {os.path.basename(p) for p in stale}
    assert made == {os.path.basename(part), "og_gen_%s.h" % build.module_digest(header)}
    assert build.build_directional_part(header) == part and len(commands) == 1      # cached
