"""Exact mixed derivatives ``d(F'(x)^T w)/dtheta_k`` without a GPU: the host probe of ``csrc/og_mix.h`` (the terms the
kernels sum, in the order of ``csrc/og_adj.h``) against an independent reference, against the adjoint probe and the
parameter probe bit for bit and against itself, the host logic of ``Problem.adjoint_parameter_sensitivity`` /
``evaluate_batch(adjoint_parameter=)`` on a stand-in engine, the build of the mixed part and the C signatures.  Cases,
the reference and the probe's build are in ``mixed_cases``.

The reference: central differences in ``theta_k`` of ``oracle.exact_jac.jacobian`` times ``w`` in long double,
Richardson-extrapolated from a step and its half; its own error is estimated from the oracle alone (against the
extrapolation from the half and the quarter step), and the probe must be within ten times the worst estimate of its
group - one point, one parameter set, one parameter - in units of an entry's ``max(1, sum_r |w_r d2F_r/dx_j dtheta_k|)``:
the rule of tests/test_hessian.py, with a group per parameter set instead of per shape, so that a parameter set of
``E`` that sits on a switch does not widen the bound of the others.  Every point, every parameter set, every
parameter, all nine weight vectors and every entry take part; none is skipped.  The step is ``2^-9 max(1, |theta_k|)``,
at which the estimate is finite everywhere on these cases.  A group whose estimate is zero (the parameter enters no
mixed term: a row of +0.0 against differences that cancel exactly) must agree exactly.

Where a parameter set puts ``q`` of ``E`` ON a switch (``parameter_exact_cases.E_THETA[:6]``: a ``clip`` edge, the tie of
``maximum``, the ``where`` threshold, a table knot), ``F'(x)^T w`` has a kink or a jump in ``theta`` there, a central
difference returns the mean of the two one-sided derivatives with an estimate near zero, and no bound on it can hold for
the derivative of the branch ``F(x)`` takes, which is what the kernels define.  There the reference also has the two
one-sided forms (second-order one-sided differences, Richardson-extrapolated, their own estimates taken the same
way), and the weight vectors are one per piece of the traced program - ones on the rows of one expression - instead of
the nine mixed ones: two expressions of ``E`` sit on switches of opposite sides at ``q = 1`` (the table's knot takes the
segment above, ``where(q > 1, ...)`` the branch below), and a sum over both matches neither side.  A form whose stencil
holds a jump shows it in its estimate (above 1e-6 of the scale, the threshold tests/test_hessian.py uses for a kink
inside a stencil) and is not used for that vector; every vector has a form that is used, and every entry must be within
ten times the group's worst estimate over the forms that are used of one of them - the same bound, against the side the
branch is on.

Measured (worst estimate / probe's worst difference from it, over the smooth groups; this file writes them to
profiles/mixed.md): P2U 5.5e-11 / 3.8e-12, P2 5.2e-13 / 3.6e-13, G9 8.3e-11 / 5.5e-12, G17 8.3e-11 / 5.5e-12,
E 1.2e-10 / 8.1e-12, B90g 3.4e-13 / 2.6e-13; the worst ratio of a group is 1.35 (P2, parameter ``d``); on the switches
of E 2.9e-07 / 1.1e-11.

The errors of the C calls that need a live handle are in tests/test_mixed_gpu.py.
"""
import ctypes
import os
import warnings

import numpy as np
import pytest

import adjoint_cases as ac
import mixed_cases as mc
import og_math_cases
import parameter_exact_cases as ec
from opengoddard_amd import _native, build, codegen, optimize, problems

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REPORT = os.path.join(ROOT, "profiles", "mixed.md")
HEAD = ["# Exact d(F'(x)^T w)/dtheta_k: the host probe of csrc/og_mix.h against its reference", "",
        "Per case, over every point, parameter set, parameter and weight vector: the oracle reference's own error estimate",
        "and the probe's worst difference from it, per entry in units of max(1, sum_r |w_r d2F_r/dx_j dtheta_k|), and the",
        "worst ratio of the two within one group (one point, one parameter set, one parameter; the bound is 10).  Smooth:",
        "the groups whose parameter set is on no switch; on a switch: the one-sided forms (tests/test_mixed.py).  Written",
        "by tests/test_mixed.py.", "", "| what | figure |", "|---|---|"]


def _note(key, text):
    """One line of profiles/mixed.md (the key's line is replaced, not repeated)."""
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
    return str(tmp_path_factory.mktemp("mix_probe"))


_RUNS = {}


def _probed(key, probe_dir, ip=1, it=-1):
    """The g++ probe of a case at one of its points and parameter sets for the nine vectors, once per session."""
    C = mc.case(key)
    it = it % len(C.thetas)
    if (key, ip, it) not in _RUNS:
        exe = mc.build_probe(C, probe_dir, "g++")
        _RUNS[(key, ip, it)] = mc.run_probe(C, exe, probe_dir, C.points[ip], mc.weights(C), C.thetas[it], "p%d_t%d" % (ip, it))
    return C, _RUNS[(key, ip, it)]


# ------------------------------------------------------------------------------------------------ 1. the reference
ON_A_SWITCH = {"E": 6}                  # the first six parameter sets of E put q on a switch
SMOOTH = 1e-6                           # (tests/test_hessian.py: above it, a kink or a jump is inside the stencil)


def _one_sided(C, x, W, theta, k, side, h=mc.H_STEP):
    """``(ref, err)`` as ``mixed_cases.oracle_mixed``, from the second-order one-sided difference on ``side`` (+1 / -1):
    ``side (-3 f(t) + 4 f(t + side s) - f(t + 2 side s)) / (2 s)``, Richardson-extrapolated from ``s`` and ``s / 2``."""
    from oracle import exact_jac
    WL = np.atleast_2d(np.asarray(W, dtype=float)).astype(np.longdouble)
    theta = np.asarray(theta, dtype=float)
    unit = np.zeros_like(theta)
    unit[k] = 1.0
    base = h * max(1.0, abs(theta[k]))
    f = lambda t: exact_jac.jacobian(C.at(t), C.prob, x).astype(np.longdouble)
    f0 = f(theta)

    def diff(step):
        return side * ((-3 * f0 + 4 * f(theta + side * step * unit) - f(theta + 2 * side * step * unit)) @ WL.T).T / \
            np.longdouble(2.0 * step)

    d0, d1, d2 = diff(base), diff(base / 2), diff(base / 4)
    r0, r1 = (4 * d1 - d0) / 3, (4 * d2 - d1) / 3
    return r1, np.abs(r1 - r0).astype(float)


def _piece_weights(C):
    """One weight vector per piece of the traced program (the cost, every expression of the callbacks, every defect
    block): ones on its rows."""
    W = np.zeros((len(C.program.pieces), C.m))
    for d, (row, ln, _eid, _kind) in enumerate(C.program.pieces):
        W[d, row:row + ln] = 1.0
    return W


def _probed_pieces(key, probe_dir, ip, it):
    C = mc.case(key)
    if (key, ip, it, "pieces") not in _RUNS:
        exe = mc.build_probe(C, probe_dir, "g++")
        _RUNS[(key, ip, it, "pieces")] = mc.run_probe(C, exe, probe_dir, C.points[ip], _piece_weights(C), C.thetas[it], "pieces")
    return _RUNS[(key, ip, it, "pieces")]


@pytest.mark.parametrize("key", mc.KEYS)
def test_the_probe_against_differences_of_the_oracle(key, probe_dir, capsys):
    C = mc.case(key)
    W = mc.weights(C)
    exe = mc.build_probe(C, probe_dir, "g++")
    estimate = worst = ratio = 0.0
    switch_estimate = switch_worst = 0.0
    for ip, x in enumerate(C.points):
        for it, theta in enumerate(C.thetas):
            r = _probed(key, probe_dir, ip, it)[1]
            assert np.all(np.isfinite(r.S))
            for k in range(C.n_par):
                scale = np.maximum(1.0, r.A[:, k, :])
                with warnings.catch_warnings():
                    warnings.simplefilter("ignore", RuntimeWarning)
                    forms = [mc.oracle_mixed(C, x, W, theta, k)]
                assert all(np.all(np.isfinite(err)) for _, err in forms), (key, ip, it, k)
                own = [float((err / scale).max()) for _, err in forms]
                dev = [np.abs(r.S[:, k, :] - ref).astype(float) / scale for ref, _ in forms]
                if it >= ON_A_SWITCH.get(key, 0):
                    assert own[0] <= SMOOTH, (key, ip, it, k, own)
                    assert dev[0].max() <= 10.0 * own[0], (key, ip, it, k, own[0], float(dev[0].max()))
                    estimate, worst = max(estimate, own[0]), max(worst, float(dev[0].max()))
                    if own[0] > 0:
                        ratio = max(ratio, float(dev[0].max()) / own[0])
                    continue
                # on a switch: one expression per weight vector (two expressions of E can sit on switches of opposite
                # sides at one q: the table's knot at 1.0 takes the segment above, `where(q > 1, ...)` the branch below)
                rp = _probed_pieces(key, probe_dir, ip, it)
                WP = _piece_weights(C)
                scale = np.maximum(1.0, rp.A[:, k, :])
                with warnings.catch_warnings():
                    warnings.simplefilter("ignore", RuntimeWarning)
                    forms = [mc.oracle_mixed(C, x, WP, theta, k)] + [_one_sided(C, x, WP, theta, k, side) for side in (1, -1)]
                assert all(np.all(np.isfinite(err)) for _, err in forms), (key, ip, it, k)
                own = np.stack([(err / scale).max(axis=1) for _, err in forms])                     # [3, K]
                dev = np.stack([np.abs(rp.S[:, k, :] - ref).astype(float) / scale for ref, _ in forms])   # [3, K, n]
                used = own <= SMOOTH
                assert used.any(axis=0).all(), (key, ip, it, k, own)
                group = float(own[used].max())              # the group's worst estimate over the forms that are used
                ok = (used[:, :, None] & (dev <= 10.0 * group)).any(axis=0)
                assert ok.all(), (key, ip, it, k, group, np.argwhere(~ok))
                switch_estimate = max(switch_estimate, group)
                switch_worst = max(switch_worst, float(np.where(used[:, :, None], dev, np.inf).min(axis=0).max()))
    text = "smooth: estimate %.1e, probe %.1e, worst ratio %.2f" % (estimate, worst, ratio)
    if key in ON_A_SWITCH:
        text += "; on a switch: estimate %.1e, probe %.1e" % (switch_estimate, switch_worst)
    _note("case " + key, text)
    with capsys.disabled():
        if os.environ.get("OG_SURFACE_REPORT"):
            print("mixed %-5s %s" % (key, text))
    assert estimate > 0 and worst > 0


# ------------------------------------------------------------------------------------------------ 2. bits
OPERAND_PARAMETER = {"P2U": {5}}        # `unit`: the collocation operand reads it


@pytest.mark.parametrize("key", mc.KEYS)
def test_first_order_parts_are_the_adjoint_and_the_parameter_probes_bits(key, probe_dir):
    """Slot 1 (rule (a) of og_dual2.h end to end): the terms' parts along ``x_j``, summed in the order of og_adj.h, are
    the adjoint probe's ``F'(x)^T w`` - the probe itself fails unless they are the same for every parameter.  Slot 2: a
    row item's part along ``theta_k`` is the parameter probe's ``dF_row/dtheta_k`` - the probe fails unless every column
    with an item in a row agrees - except on a defect row for a parameter the collocation operand reads, where
    og_par_entry adds ``sum_l D[k][l] d(operand_l)/dtheta`` and the row item of another variable's column does not hold
    it."""
    C, r = _probed(key, probe_dir)
    x, theta, W = C.points[1], C.thetas[-1], mc.weights(C)
    # clang++ and a sanitized g++ build (a plain process of its own): the same bits.  On the two shapes that between them
    # hold every path: the operand term and the unread parameter, the heavy column of more than 256 terms
    for other in ((mc.build_probe(C, probe_dir, og_math_cases.clangxx()), mc.build_probe(C, probe_dir, "g++", sanitize=True))
                  if key in ("P2U", "B90g") else ()):
        o = mc.run_probe(C, other, probe_dir, x, W, theta, "other")
        assert np.array_equal(o.S, r.S) and np.array_equal(np.signbit(o.S), np.signbit(r.S))
        assert np.array_equal(o.G, r.G) and np.array_equal(o.P, r.P)
    G, F0 = ac.run_probe(C, ac.build_probe(C, probe_dir, "g++"), probe_dir, x, W, theta, "mix_adj")
    assert np.array_equal(r.G, G) and np.array_equal(np.signbit(r.G), np.signbit(G)) and np.array_equal(r.F0, F0)
    dF, F1 = ec.run_probe(C, ec.build_probe(C, probe_dir, "g++"), probe_dir, theta, x, "mix_par")
    assert np.array_equal(F1, r.F0) and r.have.all()
    defect = np.zeros(C.m, dtype=bool)
    defect[ac.defect_rows(C)] = True
    for k in range(C.n_par):
        rows = r.have & ~(defect if k in OPERAND_PARAMETER.get(key, ()) else np.zeros(C.m, dtype=bool))
        # (a row the parameter's work lists do not hold is the parameter probe's +0.0 fill; the item's part there is a zero
        # of either sign: -0.0 for the cost -x)
        assert np.array_equal(r.P[k, rows], dF[k, rows])
    for k in OPERAND_PARAMETER.get(key, ()):
        assert not np.array_equal(r.P[k, defect], dF[k, defect])        # (the exception above is needed)
    assert not r.S[6].any() and not np.signbit(r.S[6]).any(), "the zero vector: +0.0 everywhere"
    unread = r.terms == 0
    assert not r.S[:, :, unread].any() and not np.signbit(r.S[:, :, unread]).any()


def test_the_shapes_cover_every_path_of_the_kernel(probe_dir):
    runs = {key: _probed(key, probe_dir) for key in mc.KEYS}
    C, r = runs["B90g"]
    j = C.n - 1                                                         # the final time
    assert (r.terms > 256).sum() == 1 and r.terms[j] > 256 and r.heavy[j] == 1
    assert np.abs(r.S[2, 0, j]) > 0                                     # ... and it reads the parameter
    for key in ("G9", "G17"):
        assert runs[key][0].n % 4 != 0                                  # the wavefront mapping's last workgroup
    assert all(((r.terms > 0) & (r.terms < 64) & (r.heavy == 0)).any() for _, r in runs.values())     # light columns
    assert ((runs["B90g"][1].terms >= 64) & (runs["B90g"][1].heavy == 0)).any()  # more than one block of a wavefront's loop
    assert any(r.heavy.any() for _, r in runs.values())
    # the operand term: the unit parameter of P2U reaches the column's own collocation block
    C, r = runs["P2U"]
    assert np.abs(r.S[2, 5]).max() > 0
    assert set(mc.case("P2U").unread) == {4}
    # bit 1 of a slot's `reads` word (og_mix.h: the dynamics part of every entry of the own block): NLP, and only it
    assert len(mc.KEYS) == 7
    assert set(int(v) for v in runs["NLP"][1].reads) == {-1, 1, 3}
    assert all(set(int(v) for v in r.reads) <= {-1, 0, 1} for key, (_, r) in runs.items() if key != "NLP")


def test_the_nonlocal_case_has_mixed_terms_off_the_diagonal_of_the_own_block(probe_dir):
    """``NLP``: ``dx[0] = v - a * (x - x.mean())`` - ``d2 defect_x(k) / dx_l da`` is ``(delta_kl - 1/N)`` times half the
    phase's duration, so off the diagonal it is ``-0.5 / 21``.  og_mix.h reaches those entries through ``reads & 2`` alone.
    From the oracle (differences in ``a`` of the complex-step Jacobian), which knows nothing of the bit: at least 1e-4."""
    C, r = _probed("NLP", probe_dir)
    assert set(int(v) for v in r.reads) == {-1, 1, 3} and C.names == ("a", "b") and len(C.thetas) == 2
    sl = C.program.mv[0]
    plan = codegen.SweepPlan(C.program)
    assert (plan.mv_diag[0], plan.mv_generic[0], sl.length) == (1, 1, 21)
    leaf, N, row0 = sl.leaf_base, sl.length, plan.slot_row0[0]
    ks = (2, 17)
    W = np.zeros((len(ks), C.m))
    for d, k in enumerate(ks):
        W[d, row0 + k] = 1.0                            # row d of the result: d2 defect_x(k) / dx da
    exe = mc.build_probe(C, probe_dir, "g++")
    for theta in C.thetas:
        ref, err = mc.oracle_mixed(C, C.points[1], W, theta, 0)
        got = mc.run_probe(C, exe, probe_dir, C.points[1], W, theta, "own_block").S[:, 0, :]
        assert err.max() <= SMOOTH
        for d, k in enumerate(ks):
            off = np.array([l for l in range(N) if l != k])
            assert np.abs(ref[d, leaf + off]).min() >= 1e-4, (k, float(np.abs(ref[d, leaf + off]).min()))
            assert np.abs(got[d, leaf + off]).min() >= 1e-4
            assert np.max(np.abs(got[d] - ref[d]).astype(float)) <= max(10.0 * err.max(), 1e-12)
            # closed form: the oracle's entries are -(t_f - t_0) / 2 / N there
            half = 0.5 * (C.points[1][C.n - 2] - 0.0)
            assert np.allclose(ref[d, leaf + off].astype(float), half / N, rtol=1e-6, atol=0) or \
                np.allclose(ref[d, leaf + off].astype(float), -half / N, rtol=1e-6, atol=0)


def test_a_vector_of_nine_is_the_call_with_that_vector_alone(probe_dir):
    C, r = _probed("P2U", probe_dir)
    exe, W = mc.build_probe(C, probe_dir, "g++"), mc.weights(C)
    assert W.shape[0] == 9
    for d in (0, 4, 8):
        one = mc.run_probe(C, exe, probe_dir, C.points[1], W[d], C.thetas[-1], "one")
        assert one.S.shape == (1, C.n_par, C.n) and np.array_equal(one.S[0], r.S[d]) and np.array_equal(one.F0, r.F0)
        assert np.array_equal(np.signbit(one.S[0]), np.signbit(r.S[d]))


def test_a_zero_weight_is_not_skipped(probe_dir):
    """A row with ``w_r = 0`` stays a term: with a non-finite term in that row the sum is NaN, as the product gives.  The
    running cost ``d u^2`` of P2 has the mixed term ``2 u`` times the quadrature weight: a control at infinity makes it
    infinite."""
    C = mc.case("P2")
    exe = mc.build_probe(C, probe_dir, "g++")
    W = np.zeros((1, C.m))
    fine = mc.run_probe(C, exe, probe_dir, C.points[0], W, C.thetas[0], "zero")
    assert not fine.S.any() and not np.signbit(fine.S).any()
    x = C.points[0].copy()
    uj = 2 * 5 + 2                                      # node 2 of the control of the first phase
    x[uj] = np.inf
    r = mc.run_probe(C, exe, probe_dir, x, W, C.thetas[0], "inf")
    assert np.isnan(r.S[0, 3, uj]), "0 * inf must reach the sum"


@pytest.mark.parametrize("key", ("P2U", "P2"))
def test_an_unread_parameter_gets_a_row_of_plus_zero(key, probe_dir):
    C = mc.case(key)
    exe, W = mc.build_probe(C, probe_dir, "g++"), mc.weights(C)
    for ip, x in enumerate(C.points):
        for it, theta in enumerate(C.thetas):
            r = _probed(key, probe_dir, ip, it)[1]
            for k in C.unread:
                assert not r.S[:, k].any() and not np.signbit(r.S[:, k]).any()
                assert not r.A[:, k].any()
            assert r.S[:, 0].any()                                              # (a parameter that is read)


def test_a_parameter_that_enters_linearly_has_its_closed_form(probe_dir):
    """``maximum(q, 0.75) * x`` of E above the tie is ``q x_k`` in the rows of that expression: with weights on those
    rows only, ``s_{q, x_k} = w_k`` exactly (every other term of the column is finite and has weight zero), every other
    entry and the whole row of ``r`` are zero.  ``q * q * x`` next to it: ``2 q w_k``, exactly (``q + q`` is exact)."""
    C = mc.case("E")
    exe = mc.build_probe(C, probe_dir, "g++")
    x = C.points[0]
    obj = mc.pc.Model()
    for it in (2, 3, 8, 9, 10):                                                 # q = 1.0, 1.25, 1.1, 1.7, 2.5: above 0.75
        theta = C.thetas[it]
        obj.q, obj.r, obj.table = theta[0], theta[1], C.obj.table
        row, rows_of = 1, {}
        values = {}
        for name, fn in ec.E_EXPRESSIONS.items():
            v = np.atleast_1d(fn(obj, x[:4], x[4:8]) + 0.0 * x[0])
            rows_of[name], values[name] = np.arange(row, row + v.size), v
            row += v.size
        w = np.array([0.5, -1.25, 3.0, 0.7])
        for name, factor in (("maximum", 1.0), ("q * q", 2.0 * theta[0])):
            assert rows_of[name].size == 4
            W = np.zeros((1, C.m))
            W[0, rows_of[name]] = w
            r = mc.run_probe(C, exe, probe_dir, x, W, theta, "closed")
            assert np.allclose(r.F0[rows_of[name]], values[name], rtol=1e-14, atol=0)   # (the rows are that expression's)
            want = np.zeros((C.n_par, C.n))
            want[0, :4] = factor * w
            assert np.array_equal(r.S[0], want), (name, it, r.S[0], want)


# ------------------------------------------------------------------------------------------------ 3. host logic
class StandIn:
    """``Problem``'s engine protocol without a device: the stand-in records its calls and returns a result that names
    the lane (its parameters, point and weights)."""

    m_eq = 0

    def __init__(self, prob, obj):
        C = mc.case("P2U")
        self.n, self.m, self.n_par = C.n, C.m, C.n_par
        self.theta = np.array(list(prob.parameters.values()), dtype=float)
        self.calls = []

    def set_parameters(self, theta):
        self.theta = np.asarray(theta, dtype=float).copy()

    def values(self, p):
        return np.float64(p[0]), np.zeros(2), np.zeros(self.m - 3)

    @staticmethod
    def result(theta, x, W):
        return np.stack([np.outer(theta, x) + np.sum(w) for w in W])

    def adjoint_parameter(self, x, W):
        self.calls.append((self.theta.copy(), np.array(x, dtype=float), np.array(W, dtype=float)))
        return self.result(self.theta, x, W), np.zeros(self.m)


class NoMixed(StandIn):
    adjoint_parameter = property()      # (hasattr is False)


def _p2u():
    C = mc.case("P2U")
    prob, obj = ec.CASES["P2U"][0]()
    return C, prob, obj, mc.weights(C)


def test_adjoint_parameter_sensitivity_shapes(monkeypatch):
    monkeypatch.setattr(optimize, "ENGINE_FACTORY", StandIn)
    C, prob, obj, W = _p2u()
    x, th = C.points[0], C.thetas[0]
    got = prob.adjoint_parameter_sensitivity(obj, W, x)
    eng = prob._engine
    assert got.shape == (9, C.n_par, C.n) and len(eng.calls) == 1 and getattr(prob, "_batch", None) is None
    assert np.array_equal(eng.calls[0][1], x) and np.array_equal(eng.calls[0][2], W)
    assert np.array_equal(got, StandIn.result(th, x, W))
    one = prob.adjoint_parameter_sensitivity(obj, W[4], x)                  # a single vector: [n_par, n] back
    assert one.shape == (C.n_par, C.n) and eng.calls[-1][2].shape == (1, C.m)
    assert np.array_equal(one, prob.adjoint_parameter_sensitivity(obj, W[4:5], x)[0])
    at_p = prob.adjoint_parameter_sensitivity(obj, W[4])                    # the default point: prob.p
    assert np.array_equal(eng.calls[-1][1], prob.p) and at_p.shape == (C.n_par, C.n)
    prob.set_parameters(C.thetas[1])                                        # at new values: the engine is told first
    prob.adjoint_parameter_sensitivity(obj, W[:2], x)
    assert np.array_equal(eng.calls[-1][0], C.thetas[1])


def test_refusals(monkeypatch):
    monkeypatch.setattr(optimize, "ENGINE_FACTORY", StandIn)
    C, prob, obj, W = _p2u()
    x = C.points[0]
    for bad in (W[0][:-1], W[:3, :-1], np.zeros((0, C.m)), np.zeros((3, 2, C.m)), np.append(W[0], 0.0)):
        with pytest.raises(ValueError, match="weights must have"):
            prob.adjoint_parameter_sensitivity(obj, bad, x)
    X = np.stack([x, C.points[1]])
    for bad in (W[0], W[:2, :-1], np.zeros((2, 2, C.m))):
        with pytest.raises(ValueError, match="adjoint_parameter must have shape"):
            prob.evaluate_batch(obj, X, adjoint_parameter=bad)
    with pytest.raises(ValueError, match="adjoint_parameter holds 3 rows for 2 points"):
        prob.evaluate_batch(obj, X, adjoint_parameter=W[:3])
    monkeypatch.setattr(optimize, "ENGINE_FACTORY", NoMixed)
    C, prob, obj, W = _p2u()
    with pytest.raises(ValueError, match="no exact mixed derivative"):
        prob.adjoint_parameter_sensitivity(obj, W, x)
    with pytest.raises(ValueError, match="no exact mixed derivative"):
        prob.evaluate_batch(obj, X, adjoint_parameter=W[:2])
    assert prob.evaluate_batch(obj, X).adjoint_parameter is None    # (nothing else needs the method)
    # a problem that declares no parameter
    monkeypatch.setattr(optimize, "ENGINE_FACTORY", StandIn)
    plain, pobj = problems.build("brachistochrone", nodes=[5])
    with pytest.raises(ValueError, match="declares no parameter"):
        plain.adjoint_parameter_sensitivity(pobj, np.zeros(C.m))
    with pytest.raises(ValueError, match="declares no parameter"):
        plain.evaluate_batch(pobj, plain.p[None, :], adjoint_parameter=np.zeros((1, C.m)))


def test_evaluate_batch_serves_every_lane_with_its_own_vector_and_parameters(monkeypatch):
    monkeypatch.setattr(optimize, "ENGINE_FACTORY", StandIn)
    C, prob, obj, W = _p2u()
    X = np.stack([C.points[0], C.points[1], C.points[0]])
    TH = np.stack([C.thetas[1], C.thetas[0], C.thetas[1]])
    res = prob.evaluate_batch(obj, X, parameters=TH, adjoint_parameter=W[3:6])
    assert res.adjoint_parameter.shape == (3, C.n_par, C.n)
    calls = prob._engine.calls
    assert len(calls) == 3 and [tuple(c[0]) for c in calls] == [tuple(t) for t in TH]
    for k in range(3):
        assert np.array_equal(res.adjoint_parameter[k], StandIn.result(TH[k], X[k], W[3 + k:4 + k])[0])
        assert calls[k][2].shape == (1, C.m) and np.array_equal(calls[k][2][0], W[3 + k])
    plain = prob.evaluate_batch(obj, X, parameters=TH)
    assert plain.adjoint_parameter is None and len(calls) == 3
    assert np.array_equal(plain.cost, res.cost)
    # one trajectory scanned over the parameter sets: its one vector goes with it
    scan = prob.evaluate_batch(obj, X[:1], parameters=TH, adjoint_parameter=W[:1])
    assert scan.adjoint_parameter.shape == (3, C.n_par, C.n)
    assert np.array_equal(scan.adjoint_parameter[2], StandIn.result(TH[2], X[0], W[:1])[0])
    assert np.array_equal(prob._engine.theta, C.thetas[0])          # (the engine is back at the problem's values)


def test_a_real_engine_without_the_keyword_is_not_asked_for_anything_new():
    class Batch:
        capacity, engine, pattern = 2, None, None

        class _handle:
            value = 1

        def values(self, P):
            return np.zeros((P.shape[0], 3))

        def set_parameters(self, TH):
            pass

        def adjoint_parameter(self, X, W):
            raise AssertionError("adjoint_parameter was called")

    class Engine:
        m_eq, n_par, m = 1, 6, 3

        def adjoint_parameter(self, x, W):
            raise AssertionError("the engine's own adjoint_parameter was called")

        def _load_mix_part(self):
            raise AssertionError("the part was asked for")

        def batch(self, B):
            bt = Batch()
            bt.engine = self
            return bt

    prob, obj = ec.CASES["P2U"][0]()
    prob._engine = Engine()
    X = np.stack([prob.p, prob.p])
    res = prob.evaluate_batch(obj, X)
    assert res.adjoint_parameter is None and res.cost.shape == (2,)
    with pytest.raises(AssertionError, match="adjoint_parameter was called"):
        prob.evaluate_batch(obj, X, adjoint_parameter=np.zeros((2, 3)))
    prob._engine = None


# ------------------------------------------------------------------------------------------------ 4. the build
def test_the_mixed_part_is_a_file_of_its_own(monkeypatch, tmp_path):
    assert build.MIX_PART == 10
    assert (build.MODULE_PARTS, build.BATCH_PART, build.BATCH_EXACT_PART, build.PARAMETER_PART, build.DIRECTIONAL_PART,
            build.ADJOINT_PART, build.HESSIAN_PART) == ((0, 2, 3, 1), 4, 5, 6, 7, 8, 9)
    out = build.module_path("0123456789abcdef")
    others = [build.part_path(out, i) for i in range(len(build.MODULE_PARTS))] + [
        build.batch_part_path(out), build.batch_exact_part_path(out), build.parameter_part_path(out),
        build.directional_part_path(out), build.adjoint_part_path(out), build.hessian_part_path(out)]
    assert build.mix_part_path(out).endswith(".mix.so") and build.mix_part_path(out) not in others
    assert "og_mix.h" in [os.path.basename(p) for p in build._kernel_sources()]
    monkeypatch.setattr(build, "JITDIR", str(tmp_path))
    header = mc.case("P2").header
    mod = build.module_path(build.module_digest(header))
    assert os.path.dirname(mod) == str(tmp_path)
    stale = {}
    for path in [build.part_path(mod, i) for i in range(4)] + [build.batch_part_path(mod), build.parameter_part_path(mod),
                                                               build.directional_part_path(mod),
                                                               build.adjoint_part_path(mod), build.hessian_part_path(mod)]:
        with open(path, "w") as fh:
            fh.write("untouched " + os.path.basename(path))
        stale[path] = os.stat(path).st_mtime_ns
    commands = []

    def run(cmd):
        commands.append(cmd)
        with open(cmd[cmd.index("-o") + 1], "w") as fh:
            fh.write("part")
    monkeypatch.setattr(build, "_run", run)
    part = build.build_mix_part(header)
    assert part == build.mix_part_path(mod) and os.path.exists(part)
    assert len(commands) == 1 and "-DOGK_PART=10" in commands[0]
    for path, stamp in stale.items():
        assert os.stat(path).st_mtime_ns == stamp and open(path).read() == "untouched " + os.path.basename(path)
    made = set(os.listdir(str(tmp_path))) - {os.path.basename(p) for p in stale}
    assert made == {os.path.basename(part), "og_gen_%s.h" % build.module_digest(header)}
    assert build.build_mix_part(header) == part and len(commands) == 1      # cached


def test_the_mixed_part_cross_compiles_and_knows_its_two_modes_only():
    header = mc.case("P2").header
    part = build.build_mix_part(header)
    with open(part, "rb") as fh:
        blob = fh.read()
    assert b"gfx950" in blob and b"ogk_exact_mix" in blob and b"ogk_exact_mix_batch" in blob
    assert b"ogk_fused" not in blob and b"ogk_exact_hvp" not in blob and b"ogk_exact_adj" not in blob
    lib = ctypes.CDLL(part)
    assert hasattr(lib, "ogk_launch_batch") and hasattr(lib, "ogk_get_info")
    lib.ogk_launch.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p]
    lib.ogk_launch_batch.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p]
    # a record of zeros: the launcher refuses it before it touches the device (what og_adjoint_parameter_load relies
    # on); a mode of another part is that part's
    record = ctypes.create_string_buffer(4096)
    invalid = 1                                         # hipErrorInvalidValue
    assert lib.ogk_launch(record, 23, None) == invalid
    assert lib.ogk_launch(record, 21, None) == -4242 and lib.ogk_launch(record, 4, None) == -4242
    assert lib.ogk_launch_batch(record, 24, None) == invalid and lib.ogk_launch_batch(None, 24, None) == invalid
    assert lib.ogk_launch_batch(record, 21, None) == -4242 and lib.ogk_launch_batch(record, 4, None) == -4242


# ------------------------------------------------------------------------------------------------ 5. the C signatures
MIXED_FUNCTIONS = ("og_adjoint_parameter_load", "og_adjoint_parameter_dev", "og_adjoint_parameter",
                   "og_adjoint_parameter_batch_dev", "og_adjoint_parameter_batch")


def test_signatures_and_null_handles():
    C = ctypes
    dp = _native.SIGNATURES["og_directional"][1][1]                 # (the module's double pointer type)
    vp = C.c_void_p
    want = {
        "og_adjoint_parameter_load": [vp, C.c_char_p],
        "og_adjoint_parameter_dev": [vp, vp, C.c_int32, vp, vp, vp, vp],
        "og_adjoint_parameter": [vp, dp, C.c_int32, dp, dp, dp],
        "og_adjoint_parameter_batch_dev": [vp, C.c_int32, vp, vp, vp, vp, vp],
        "og_adjoint_parameter_batch": [vp, C.c_int32, dp, dp, dp, dp],
    }
    assert set(want) == set(MIXED_FUNCTIONS)
    with open(os.path.join(ROOT, "include", "ogpsx.h")) as fh:
        text = fh.read()
    lib = _native.lib()
    for name in MIXED_FUNCTIONS:
        assert not name.startswith("og_batch_") and not name.startswith("og_jacobian_exact_batch")
        assert "int %s(" % name in text
        restype, argtypes = _native.SIGNATURES[name]
        assert restype is C.c_int and argtypes == want[name], name
        assert getattr(lib, name).argtypes == want[name]                # AttributeError: not exported

    def error_text():
        msg = lib.og_last_error()
        return msg.decode() if msg else ""

    ptr = _native.dptr(np.zeros(4))
    calls = {
        "og_adjoint_parameter_load": (lambda: lib.og_adjoint_parameter_load(None, b"/nonexistent.so"), "null handle"),
        "og_adjoint_parameter_dev": (lambda: lib.og_adjoint_parameter_dev(None, 8, 1, 8, 8, None, None), "null argument"),
        "og_adjoint_parameter": (lambda: lib.og_adjoint_parameter(None, ptr, 1, ptr, ptr, None), "null argument"),
        "og_adjoint_parameter_batch_dev": (lambda: lib.og_adjoint_parameter_batch_dev(None, 1, 8, 8, None, 8, None),
                                           "null batch"),
        "og_adjoint_parameter_batch": (lambda: lib.og_adjoint_parameter_batch(None, 1, ptr, ptr, None, ptr), "null batch"),
    }
    for name, (call, what) in calls.items():
        assert call() == 1, name
        text = error_text()
        assert text.startswith(name + ":") and what in text, text
