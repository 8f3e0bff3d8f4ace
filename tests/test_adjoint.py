"""Exact adjoint products ``F'(x)^T w`` without a GPU: the host probe of ``csrc/og_adj.h`` (the terms and the order of
sums that the kernels implement) against the twin's exact Jacobian and against the shipped directional probe, the host
logic of ``Problem.adjoint_product`` / ``evaluate_batch(adjoints=)`` on a stand-in engine, the build of the adjoint part
and the C signatures.  The cases, the reference and the probe's build are in ``adjoint_cases``.

Reference: ``J^T w`` accumulated in ``np.longdouble`` with ``J`` from the twin's ``exact(x)``.  The error is measured per
column in units of ``max(1, sum_r |J_rj w_r|)`` and bounded by ``1e-12`` (``test_exact_surface.BOUND``) at every case,
parameter set, point and weight vector.  Measured worst per case (g++; this file writes them to profiles/adjoint.md):
at most 3.7e-16 (table_ascent).  Duality with the directional probe, ``w . (F'(x) v) = (F'(x)^T w) . v`` in long double: within
``1e-12`` of ``sum_rj |w_r J_rj v_j|``.

The errors of the C calls that need a live handle (``k`` out of range, the part not loaded) are in
tests/test_adjoint_gpu.py: a handle cannot be created without a device.
"""
import ctypes
import os

import numpy as np
import pytest

import adjoint_cases as ac
import directional_cases as dc
import og_math_cases
import parameter_exact_cases as ec
from opengoddard_amd import _native, build, optimize, problems
from oracle import twin

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REPORT = os.path.join(ROOT, "profiles", "adjoint.md")


@pytest.fixture(scope="module")
def probe_dir(tmp_path_factory):
    return str(tmp_path_factory.mktemp("adj_probe"))


def _note(key, worst):
    """The measured worst error of a case into profiles/adjoint.md (the case's line is replaced, not repeated)."""
    line = "| %s | %.1e |" % (key, worst)
    try:
        old = open(REPORT).read().split("\n") if os.path.exists(REPORT) else []
        if not old:
            old = ["# Exact F'(x)^T w: the host probe of csrc/og_adj.h against the twin's J^T w", "",
                   "Worst difference from the reference over every parameter set, point and weight vector of the case, per",
                   "column in units of max(1, sum_r |J_rj w_r|) (bound: 1e-12).  Written by tests/test_adjoint.py.", "",
                   "| case | worst |", "|---|---|"]
        kept = [row for row in old if not row.startswith("| %s |" % key)]
        while kept and kept[-1] == "":
            kept.pop()
        with open(REPORT, "w") as fh:
            fh.write("\n".join(kept + [line]) + "\n")
    except OSError:
        pass


def _twin(C):
    return twin.Twin(C.prob, C.obj, program=C.program, header=C.header)


# ------------------------------------------------------------------------------------------------ 1. the host probe
@pytest.mark.parametrize("key", ac.CPU_KEYS)
def test_the_probe_equals_the_twins_product(key, probe_dir, capsys):
    C = ac.case(key)
    gxx = ac.build_probe(C, probe_dir, "g++")
    clang = ac.build_probe(C, probe_dir, og_math_cases.clangxx())
    san = ac.build_probe(C, ac.probe_folder(C, probe_dir) if key in ac.SANITIZE_WITH_CLANG else probe_dir,
                         ac.sanitizer_compiler(key), sanitize=True)
    tw = _twin(C)
    W = ac.weights(C)
    m, rows = C.m, ac.defect_rows(C)
    assert W.shape == (8, m) and W[0, 0] == 1 and W[1, m - 1] == 1 and np.all(W[2] == 1) and not W[6].any()
    assert np.all(np.abs(W[3:6]).max(axis=1) == 1.0) and rows.size and not W[7, rows].any() and W[7].any()
    worst = 0.0
    for t, theta in enumerate(C.thetas):
        if theta is not None:
            tw._cv[C.program.par_off:] = theta
        for i, x in enumerate(C.points):
            # (run_probe: the probe pre-fills with NaN and fails unless every entry of every vector is written once)
            G, F0 = ac.run_probe(C, gxx, probe_dir, x, W, theta)
            assert np.all(np.isfinite(G)), (key, t, i)
            F0t, JT = tw.exact(x)
            assert np.array_equal(F0, tw.values(x)) and np.array_equal(F0, F0t), (key, t, i)
            for other in ([clang] if (t, i) != (0, 0) else [clang, san]):         # (the sanitizer build: once per case)
                G2, F02 = ac.run_probe(C, other, probe_dir, x, W, theta, "other")
                assert np.array_equal(G2, G) and np.array_equal(np.signbit(G2), np.signbit(G)), (key, t, i, other)
                assert np.array_equal(F02, F0)
            assert not G[6].any() and not np.signbit(G[6]).any(), "the zero vector: +0.0 everywhere"
            prod, scale = ac.twin_adjoint(JT, W)
            err = ac.worst_error(G, prod, scale)
            # w = e_r: row r of the exact Jacobian, entry by entry (a single term per column: no rounding of a sum)
            for d, r in ((0, 0), (1, m - 1)):
                assert np.array_equal(G[d], JT[:, r] + 0.0), (key, t, i, d)
            worst = max(worst, err)
            with capsys.disabled():
                if os.environ.get("OG_SURFACE_REPORT"):
                    print("adjoint %-16s theta %d point %d twin %.2e" % (key, t, i, err))
            assert err <= ac.BOUND, (key, t, i, err)
    _note(key, worst)


@pytest.mark.parametrize("key", ac.CPU_KEYS)
def test_duality_with_the_directional_probe(key, probe_dir):
    """``w . (F'(x) v) == (F'(x)^T w) . v``: the two matrix-free halves are one operator and its transpose."""
    C = ac.case(key)
    adj = ac.build_probe(C, probe_dir, "g++")
    fwd = dc.build_probe(C, probe_dir, "g++")
    tw = _twin(C)
    V, W = C.directions(), ac.weights(C)
    for t, theta in enumerate(C.thetas):
        if theta is not None:
            tw._cv[C.program.par_off:] = theta
        x = C.points[t % len(C.points)]
        G, _ = ac.run_probe(C, adj, probe_dir, x, W, theta, "dual")
        dF, _ = dc.run_probe(C, fwd, probe_dir, x, V, theta, "dual_dir")
        JA = np.abs(tw.exact(x)[1]).astype(np.longdouble)                   # |J_T| [n, m]
        left = W.astype(np.longdouble) @ dF.astype(np.longdouble).T         # [8, 7]: w_a . (J v_b)
        right = G.astype(np.longdouble) @ V.astype(np.longdouble).T         # (J^T w_a) . v_b
        scale = np.abs(W).astype(np.longdouble) @ JA.T @ np.abs(V).astype(np.longdouble).T
        assert np.any(scale > 0)
        assert np.all(np.abs(left - right) <= 1e-12 * scale), (key, t, float(np.max(np.abs(left - right))))


def test_a_vector_alone_gives_the_bits_it_gives_among_others(probe_dir):
    C = ac.case("ragged_two_phase")
    exe = ac.build_probe(C, probe_dir, "g++")
    W = ac.weights(C)
    G, F0 = ac.run_probe(C, exe, probe_dir, C.points[1], W)
    for d in (0, 4, 7):
        one, F1 = ac.run_probe(C, exe, probe_dir, C.points[1], W[d], tag="one")
        assert one.shape == (1, C.n) and np.array_equal(one[0], G[d]) and np.array_equal(F1, F0)


def test_a_zero_weight_is_not_skipped(probe_dir):
    """A row with ``w_r = 0`` stays a term: with an infinite entry in that row the sum is NaN, as the product gives.
    The brachistochrone's dynamics divide nothing; its inequality ``y >= 0`` is linear - so the infinity is put into
    the point: ``v = inf`` makes the entries of the defect rows that read it infinite or NaN."""
    C = ac.case("B5")
    exe = ac.build_probe(C, probe_dir, "g++")
    x = C.points[0].copy()
    vj = 2 * 5 + 2                                      # node 2 of the third state (v)
    x[vj] = np.inf
    W = np.zeros((1, C.m))
    data_ok = ac.run_probe(C, exe, probe_dir, C.points[0], W, tag="zero")[0]
    assert not data_ok.any()
    G, _ = ac.run_probe(C, exe, probe_dir, x, W, tag="inf")
    assert np.isnan(G).any(), "0 * inf must reach the sum"


def test_an_unread_variable_gets_plus_zero(probe_dir):
    C = ac.case("layout_8")
    exe = ac.build_probe(C, probe_dir, "g++")
    W = ac.weights(C)
    G, _, terms, _ = ac.run_probe(C, exe, probe_dir, C.points[0], W, structure=True)
    unread = np.flatnonzero(terms == 0)
    assert unread.size == 130
    assert not G[:, unread].any() and not np.signbit(G[:, unread]).any()
    JT = _twin(C).exact(C.points[0])[1]
    assert not JT[unread].any()                          # (the twin agrees: those columns are structurally empty)


@pytest.mark.parametrize("key", ac.GPU_KEYS)
def test_the_gpu_shapes_cover_what_the_cases_file_states(key, probe_dir):
    C = ac.case(key)
    exe = ac.build_probe(C, probe_dir, "g++")
    G, _, terms, reads = ac.run_probe(C, exe, probe_dir, C.points[0], ac.weights(C)[:1], C.thetas[0], structure=True)
    assert (int((terms > 256).sum()), int((terms == 0).sum()), set(int(r) for r in reads)) == ac.COVERAGE[key]
    assert (terms < 64).any()
    if key == "B90":
        assert terms[C.n - 1] == 272 and int(((terms >= 64) & (terms <= 256)).sum()) == 270
        # the probe at the shape the other CPU cases do not hold: against the twin here
        tw = _twin(C)
        W = ac.weights(C)
        G, F0 = ac.run_probe(C, exe, probe_dir, C.points[1], W)
        F0t, JT = tw.exact(C.points[1])
        prod, scale = ac.twin_adjoint(JT, W)
        assert np.array_equal(F0, F0t) and ac.worst_error(G, prod, scale) <= ac.BOUND


def test_the_reads_words_of_the_surface_problems_and_of_all_shapes(probe_dir):
    """The surface problems and the parameterised ones produce 0 and 1 only - but for ``wide_reductions``, whose dynamics
    reduce over a state's slice (3 next to 1); the shapes of ``nonlocal_cases`` bring 2 and 3, so the GPU shapes between
    them hold every value of the word."""
    seen = {}
    for key in ac.CPU_KEYS:
        C = ac.case(key)
        exe = ac.build_probe(C, probe_dir, "g++")
        reads = ac.run_probe(C, exe, probe_dir, C.points[0], ac.weights(C)[:1], C.thetas[0], structure=True)[3]
        seen[key] = set(int(r) for r in reads)
    assert set(dc.NONLOCAL_KEYS) == {"NL2", "NL0"} and set(dc.NONLOCAL_KEYS) <= set(ac.CPU_KEYS)
    surface_keys = dc.SURFACE_KEYS + dc.PARAMETER_KEYS
    assert set().union(*(seen[key] for key in surface_keys if key != "wide_reductions")) == {-1, 0, 1}
    assert seen["wide_reductions"] == {-1, 1, 3}
    assert seen["NL2"] == ac.COVERAGE["NL2"][2] == {-1, 1, 2} and seen["NL0"] == ac.COVERAGE["NL0"][2] == {-1, 3}
    covered = set().union(*(c[2] for c in ac.COVERAGE.values()))
    assert covered == {-1, 0, 1, 2, 3} and set().union(*seen.values()) == covered


# ------------------------------------------------------------------------------------------------ 2. host logic
class StandIn:
    """``Problem``'s engine protocol on the C++ twin (point by point, no ``batch``), with ``adjoint`` as the product of
    the twin's exact Jacobian at the parameters it was last given."""

    KEY = "P2U"

    def __init__(self, prob, obj):
        self.C = ac.case(self.KEY)
        self.tw = twin.Twin(prob, obj, program=self.C.program, header=self.C.header)
        self.m_eq = self.tw.m_eq
        self.theta = np.array(list(prob.parameters.values()), dtype=float)
        self.tw._cv[self.C.program.par_off:] = self.theta
        self.adj_calls = []

    def set_parameters(self, theta):
        self.theta = np.asarray(theta, dtype=float).copy()
        self.tw._cv[self.C.program.par_off:] = self.theta

    def values(self, p):
        F = self.tw.values(p)
        return F[0], F[1:1 + self.m_eq], F[1 + self.m_eq:]

    def exact_stacked(self, p):
        return self.tw.exact(p)

    def adjoint(self, x, W):
        self.adj_calls.append((self.theta.copy(), np.array(x, dtype=float), np.array(W, dtype=float)))
        F0, JT = self.tw.exact(x)
        return np.stack([JT @ w for w in W]), F0


def _want(C, x, W, theta):
    tw = _want.twins.setdefault(C.key, _twin(C))
    tw._cv[C.program.par_off:] = theta
    JT = tw.exact(x)[1]
    return np.stack([JT @ w for w in np.atleast_2d(W)])


_want.twins = {}


class NoAdjoint(StandIn):
    adjoint = property()                # (hasattr is False)


def test_adjoint_product_shapes_and_one_engine_call(monkeypatch):
    monkeypatch.setattr(optimize, "ENGINE_FACTORY", StandIn)
    C = ac.case("P2U")
    prob, obj = ec.CASES["P2U"][0]()
    x, W = C.points[0], ac.weights(C)
    got = prob.adjoint_product(obj, W, x)
    eng = prob._engine
    assert got.shape == (8, C.n) and len(eng.adj_calls) == 1 and getattr(prob, "_batch", None) is None
    assert np.array_equal(eng.adj_calls[0][1], x) and np.array_equal(eng.adj_calls[0][2], W)
    assert np.array_equal(got, _want(C, x, W, C.thetas[0]))
    one = prob.adjoint_product(obj, W[3], x)                        # the 1-D form
    assert one.shape == (C.n,) and np.array_equal(one, got[3])
    assert eng.adj_calls[-1][2].shape == (1, C.m) and np.array_equal(eng.adj_calls[-1][2][0], W[3])
    at_p = prob.adjoint_product(obj, W[4])                          # the default point: prob.p
    assert np.array_equal(eng.adj_calls[-1][1], prob.p) and at_p.shape == (C.n,)
    prob.set_parameters(C.thetas[1])                                # at new values: the engine is told first
    got = prob.adjoint_product(obj, W[:2], x)
    assert np.array_equal(eng.adj_calls[-1][0], C.thetas[1])
    assert np.array_equal(got, _want(C, x, W[:2], C.thetas[1]))


def test_refusals(monkeypatch):
    C = ac.case("P2U")
    x, W = C.points[0], ac.weights(C)
    monkeypatch.setattr(optimize, "ENGINE_FACTORY", StandIn)
    prob, obj = ec.CASES["P2U"][0]()
    for bad in (W[0][:-1], W[:, :-1], np.zeros((0, C.m)), np.zeros((2, 2, C.m)), np.append(W[0], 0.0)):
        with pytest.raises(ValueError, match="weights must have"):
            prob.adjoint_product(obj, bad, x)
    X = np.stack([x, C.points[1]])
    with pytest.raises(ValueError, match="adjoints must have shape"):
        prob.evaluate_batch(obj, X, adjoints=W[:2, :-1])
    with pytest.raises(ValueError, match="adjoints must have shape"):
        prob.evaluate_batch(obj, X, adjoints=W[0])
    with pytest.raises(ValueError, match="adjoints holds 3 rows for 2 points"):
        prob.evaluate_batch(obj, X, adjoints=W[:3])
    monkeypatch.setattr(optimize, "ENGINE_FACTORY", NoAdjoint)
    prob, obj = ec.CASES["P2U"][0]()
    with pytest.raises(ValueError, match="no exact adjoint product"):
        prob.adjoint_product(obj, W, x)
    with pytest.raises(ValueError, match="no exact adjoint product"):
        prob.evaluate_batch(obj, X, adjoints=W[:2])
    assert prob.evaluate_batch(obj, X).adjoint is None              # (nothing else needs the method)


@pytest.mark.parametrize("jacobian", [False, "exact"])
def test_evaluate_batch_serves_every_lane_with_its_own_vector(jacobian, monkeypatch):
    monkeypatch.setattr(optimize, "ENGINE_FACTORY", StandIn)
    C = ac.case("P2U")
    prob, obj = ec.CASES["P2U"][0]()
    X = np.stack([C.points[0], C.points[1], C.points[0]])
    W = ac.weights(C)[3:6]
    TH = np.stack([C.thetas[1], C.thetas[0], C.thetas[1]])
    res = prob.evaluate_batch(obj, X, jacobian=jacobian, parameters=TH, adjoints=W)
    assert res.adjoint.shape == (3, C.n)
    for k in range(3):
        assert np.array_equal(res.adjoint[k], _want(C, X[k], W[k], TH[k])[0])
    calls = prob._engine.adj_calls
    assert len(calls) == 3 and [tuple(c[0]) for c in calls] == [tuple(t) for t in TH]
    assert all(c[2].shape == (1, C.m) and np.array_equal(c[2][0], W[k]) for k, c in enumerate(calls))
    # adjoints=None is the default: no engine call, and the result is what it was
    plain = prob.evaluate_batch(obj, X, jacobian=jacobian, parameters=TH)
    assert plain.adjoint is None and len(prob._engine.adj_calls) == 3
    assert np.array_equal(plain.cost, res.cost) and np.array_equal(plain.equality, res.equality)
    assert np.array_equal(plain.inequality, res.inequality)
    if jacobian:
        assert np.array_equal(plain.values, res.values)
    # without parameters= every lane is at the problem's values; the engine is back at them afterwards
    res = prob.evaluate_batch(obj, X, adjoints=W)
    assert np.array_equal(res.adjoint[1], _want(C, X[1], W[1], C.thetas[0])[0])
    assert np.array_equal(prob._engine.theta, C.thetas[0])
    # one trajectory scanned over the parameter sets: its one weight vector goes with it
    scan = prob.evaluate_batch(obj, X[:1], parameters=TH, adjoints=W[:1])
    assert scan.adjoint.shape == (3, C.n)
    assert np.array_equal(scan.adjoint[2], _want(C, X[0], W[0], TH[2])[0])


def test_a_real_engine_without_the_keyword_is_not_asked_for_anything_new():
    """``adjoints=None`` on an engine WITH a batch: ``BatchSweep.adjoint`` is not called (a batch object that would raise
    if it were)."""
    class Batch:
        capacity, engine, pattern = 2, None, None

        class _handle:
            value = 1

        def values(self, P):
            return np.zeros((P.shape[0], 3))

        def adjoint(self, X, W):
            raise AssertionError("adjoint was called")

    class Engine:
        m_eq, n_par, m = 1, 0, 3

        def adjoint(self, x, W):
            raise AssertionError("the engine's own adjoint was called")

        def batch(self, B):
            bt = Batch()
            bt.engine = self
            return bt

    prob, obj = problems.build("brachistochrone")
    prob._engine = Engine()
    res = prob.evaluate_batch(obj, np.stack([prob.p, prob.p]))
    assert res.adjoint is None and res.cost.shape == (2,)
    with pytest.raises(AssertionError, match="adjoint was called"):
        prob.evaluate_batch(obj, np.stack([prob.p, prob.p]), adjoints=np.zeros((2, 3)))
    prob._engine = None


# ------------------------------------------------------------------------------------------------ 3. the build
def test_the_adjoint_part_is_a_file_of_its_own(monkeypatch, tmp_path):
    assert build.ADJOINT_PART == 8
    assert (build.MODULE_PARTS, build.BATCH_PART, build.BATCH_EXACT_PART, build.PARAMETER_PART,
            build.DIRECTIONAL_PART) == ((0, 2, 3, 1), 4, 5, 6, 7)
    out = build.module_path("0123456789abcdef")
    others = [build.part_path(out, i) for i in range(len(build.MODULE_PARTS))] + [
        build.batch_part_path(out), build.batch_exact_part_path(out), build.parameter_part_path(out),
        build.directional_part_path(out)]
    assert build.adjoint_part_path(out).endswith(".adj.so") and build.adjoint_part_path(out) not in others
    # asking for the part compiles that file alone (OGK_PART=8) and leaves every other file of the folder as it is
    monkeypatch.setattr(build, "JITDIR", str(tmp_path))
    header = ac.case("B5").header
    mod = build.module_path(build.module_digest(header))
    assert os.path.dirname(mod) == str(tmp_path)
    stale = {}
    for path in [build.part_path(mod, i) for i in range(4)] + [build.batch_part_path(mod), build.parameter_part_path(mod),
                                                               build.directional_part_path(mod)]:
        with open(path, "w") as fh:
            fh.write("untouched " + os.path.basename(path))
        stale[path] = os.stat(path).st_mtime_ns
    commands = []

    def run(cmd):
        commands.append(cmd)
        with open(cmd[cmd.index("-o") + 1], "w") as fh:
            fh.write("part")
    monkeypatch.setattr(build, "_run", run)
    part = build.build_adjoint_part(header)
    assert part == build.adjoint_part_path(mod) and os.path.exists(part)
    assert len(commands) == 1 and "-DOGK_PART=8" in commands[0]
    for path, stamp in stale.items():
        assert os.stat(path).st_mtime_ns == stamp and open(path).read() == "untouched " + os.path.basename(path)
    made = set(os.listdir(str(tmp_path))) - {os.path.basename(p) for p in stale}
    assert made == {os.path.basename(part), "og_gen_%s.h" % build.module_digest(header)}
    assert build.build_adjoint_part(header) == part and len(commands) == 1      # cached


def test_the_adjoint_part_cross_compiles_and_knows_its_two_modes_only():
    header = ac.case("B5").header
    part = build.build_adjoint_part(header)
    with open(part, "rb") as fh:
        blob = fh.read()
    assert b"gfx950" in blob and b"ogk_exact_adj" in blob and b"ogk_exact_adj_batch" in blob
    assert b"ogk_exact_dir" not in blob and b"ogk_exact_struct" not in blob and b"ogk_fused" not in blob
    lib = ctypes.CDLL(part)
    assert hasattr(lib, "ogk_launch_batch") and hasattr(lib, "ogk_get_info")
    lib.ogk_launch.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p]
    lib.ogk_launch_batch.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p]
    # a record of zeros: the launcher refuses it before it touches the device (what og_adjoint_load relies on); a mode
    # of another part is that part's
    record = ctypes.create_string_buffer(4096)
    invalid = 1                                         # hipErrorInvalidValue
    assert lib.ogk_launch(record, 19, None) == invalid
    assert lib.ogk_launch(record, 17, None) == -4242 and lib.ogk_launch(record, 4, None) == -4242
    assert lib.ogk_launch_batch(record, 20, None) == invalid and lib.ogk_launch_batch(None, 20, None) == invalid
    assert lib.ogk_launch_batch(record, 18, None) == invalid


# ------------------------------------------------------------------------------------------------ 4. the C signatures
ADJOINT_FUNCTIONS = ("og_adjoint_load", "og_adjoint_dev", "og_adjoint", "og_adjoint_batch_dev", "og_adjoint_batch")


def test_signatures_and_null_handles():
    C = ctypes
    dp = _native.SIGNATURES["og_directional"][1][1]                 # (the module's double pointer type)
    want = {
        "og_adjoint_load": [C.c_void_p, C.c_char_p],
        "og_adjoint_dev": [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p],
        "og_adjoint": [C.c_void_p, dp, C.c_int32, dp, dp, dp],
        "og_adjoint_batch_dev": [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p],
        "og_adjoint_batch": [C.c_void_p, C.c_int32, dp, dp, dp, dp],
    }
    assert set(want) == set(ADJOINT_FUNCTIONS)
    lib = _native.lib()
    for name in ADJOINT_FUNCTIONS:
        restype, argtypes = _native.SIGNATURES[name]
        assert restype is C.c_int and argtypes == want[name], name
        assert getattr(lib, name).argtypes == want[name]                # AttributeError: not exported
        assert not name.startswith("og_batch_") and not name.startswith("og_jacobian_exact_batch")

    def error_text():
        msg = lib.og_last_error()
        return msg.decode() if msg else ""

    x = np.zeros(4)
    ptr = _native.dptr(x)
    calls = {
        "og_adjoint_load": (lambda: lib.og_adjoint_load(None, b"/nonexistent.so"), "null handle"),
        "og_adjoint_dev": (lambda: lib.og_adjoint_dev(None, 8, 1, 8, 8, None, None), "null argument"),
        "og_adjoint": (lambda: lib.og_adjoint(None, ptr, 1, ptr, ptr, None), "null argument"),
        "og_adjoint_batch_dev": (lambda: lib.og_adjoint_batch_dev(None, 1, 8, 8, None, 8, None), "null batch"),
        "og_adjoint_batch": (lambda: lib.og_adjoint_batch(None, 1, ptr, ptr, None, ptr), "null batch"),
    }
    for name, (call, what) in calls.items():
        assert call() == 1, name
        text = error_text()
        assert text.startswith(name + ":") and what in text, text
