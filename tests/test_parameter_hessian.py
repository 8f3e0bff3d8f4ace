"""Exact second derivatives of ``w . F`` in the run-time parameters, ``S_kl = sum_r w_r d2F_r/dtheta_k dtheta_l``, without
a GPU: the host probe of ``csrc/og_pp.h`` (the entries the kernels sum, in the order of ``csrc/og_adj.h``) against an
independent reference, against closed forms, against the parameter probe bit for bit (inside the probe itself) and
against itself, the host logic of ``Problem.parameter_hessian`` / ``evaluate_batch(parameter_hessians=)`` on a stand-in
engine, the generated headers, the build of the part and the C signatures.  Cases, the reference and the probe's build
are in ``parameter_hessian_cases``.

The reference: central differences in ``theta_l`` of ``parameter_exact_cases.complex_step`` (``dF/dtheta_k`` by the
oracle's complex step) contracted with ``w`` in long double, Richardson-extrapolated from the step
``2^-9 max(1, |theta_l|)`` and its half; its own error is estimated from the oracle alone (against the extrapolation from
the half and the quarter step), and the probe must be within ten times the worst estimate of its group - one point, one
parameter set, one pair ``(k, l)`` - in units of ``max(1, A_kl)``, ``A_kl = sum_r |w_r d2F_r/dtheta_k dtheta_l|``: the rule
of tests/test_mixed.py.  Every point, parameter set, ordered pair, weight vector takes part; none is skipped.  A group
whose estimate is zero must agree exactly.

Where a parameter set puts ``q`` of ``E`` ON a switch (``parameter_exact_cases.E_THETA[:6]``) ``dF/dtheta`` has a jump
there, and the reference has the central form and the two one-sided forms of tests/test_mixed.py, with one weight vector
per expression - and two more one-sided forms whose stencils leave ``theta`` itself out: at the kink of ``abs`` the
complex step's ``dF/dq`` is that of neither side (slope 0 between -1 and +1), so all three of the other forms hold a
jump there (measured: their estimates are 0.2 to 2 of the scale); a form whose stencil holds a jump shows it in its estimate (above 1e-6 of the scale) and is not used for
that vector; every vector has a form that is used (``test_the_reference_alone_has_a_smooth_form_on_every_switch`` checks
this of the reference alone), and every entry must be within ten times the group's worst estimate over the forms that
are used of one of them.

Measured (worst estimate / probe's worst difference from it / worst ratio of a group, over the smooth groups; this file
writes them to profiles/parameter_hessian.md): E 1.0e-09 / 6.8e-11 / 1.11, P2U 1.1e-10 / 7.4e-12 / 1.00, NLP 0 / 0 (every
entry is an exact +0.0 and every difference cancels exactly), G17 2.5e-10 / 1.7e-11 / 0.08, G90 5.8e-10 / 3.8e-11 / 0.07,
G257 8.8e-10 / 5.9e-11 / 0.07; on the switches of E 9.9e-07 / 3.7e-11.  The closed forms ``4 / q^3`` and ``-1 / q^2`` hold
within the 4 ulp stated.

The errors of the C calls that need a live handle are in tests/test_parameter_hessian_gpu.py.
"""
import ctypes
import hashlib
import os
import re
import warnings

import numpy as np
import pytest

import og_math_cases
import parameter_exact_cases as ec
import parameter_hessian_cases as hc
from opengoddard_amd import _native, build, codegen, optimize, problems

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REPORT = os.path.join(ROOT, "profiles", "parameter_hessian.md")
HEAD = ["# Exact d2(w . F)/dtheta_k dtheta_l: the host probe of csrc/og_pp.h against its reference", "",
        "Per case, over every point, parameter set, ordered pair and weight vector: the oracle reference's own error",
        "estimate and the probe's worst difference from it, per entry in units of max(1, sum_r |w_r d2F_r/dtheta_k dtheta_l|),",
        "and the worst ratio of the two within one group (one point, one parameter set, one pair; the bound is 10).  Smooth:",
        "the groups whose parameter set is on no switch; on a switch: the one-sided forms (tests/test_parameter_hessian.py).",
        "Written by tests/test_parameter_hessian.py.", "", "| what | figure |", "|---|---|"]


def _note(key, text):
    """One line of profiles/parameter_hessian.md (the key's line is replaced, not repeated)."""
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
    return str(tmp_path_factory.mktemp("pp_probe"))


_RUNS = {}


def _probed(key, probe_dir, ip=1, it=-1):
    """The g++ probe of a case at one of its points and parameter sets for the nine vectors, once per session."""
    C = hc.case(key)
    it = it % len(C.thetas)
    if (key, ip, it) not in _RUNS:
        exe = hc.build_probe(C, probe_dir, "g++")
        _RUNS[(key, ip, it)] = hc.run_probe(C, exe, probe_dir, C.points[ip], hc.weights(C), C.thetas[it], "p%d_t%d" % (ip, it))
    return C, _RUNS[(key, ip, it)]


def _same(a, b):
    """bit for bit, the sign of a zero included"""
    return np.array_equal(a, b) and np.array_equal(np.signbit(a), np.signbit(b))


# ------------------------------------------------------------------------------------------------ 1. the reference
ON_A_SWITCH = {"E": 6}                  # the first six parameter sets of E put q on a switch
SMOOTH = 1e-6                           # (tests/test_mixed.py: above it, a kink or a jump is inside the stencil)


def _piece_weights(C):
    """One weight vector per piece of the traced program (the cost, every expression of the callbacks, every defect
    block): ones on its rows."""
    W = np.zeros((len(C.program.pieces), C.m))
    for d, (row, ln, _eid, _kind) in enumerate(C.program.pieces):
        W[d, row:row + ln] = 1.0
    return W


def _switch_forms(C, x, WP, theta, l):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        return [hc.oracle_second(C, x, WP, theta, l)] + [hc.one_sided_second(C, x, WP, theta, l, side) for side in (1, -1)] + \
            [hc.open_sided_second(C, x, WP, theta, l, side) for side in (1, -1)]


def test_the_reference_alone_has_a_smooth_form_on_every_switch():
    """Of the reference alone, before anything relies on it: on every switch set of ``E``, for every expression's weight
    vector, every parameter ``theta_l`` and every ``k``, one of the five forms has an estimate below 1e-6 in units of
    ``max(1, |reference|)`` (the scale ``A_kl`` of the comparison is the probe's; the reference's own magnitude stands in
    for it here)."""
    C = hc.case("E")
    WP = _piece_weights(C)
    for x in C.points:
        for it in range(ON_A_SWITCH["E"]):
            for l in range(C.n_par):
                forms = _switch_forms(C, x, WP, C.thetas[it], l)
                assert all(np.all(np.isfinite(err)) for _, err in forms)
                own = np.stack([err / np.maximum(1.0, np.abs(ref).astype(float)) for ref, err in forms])   # [5, K, n_par]
                assert (own <= SMOOTH).any(axis=0).all(), (it, l, np.argwhere(~(own <= SMOOTH).any(axis=0)))


@pytest.mark.parametrize("key", hc.KEYS)
def test_the_probe_against_differences_of_the_oracle(key, probe_dir, capsys):
    C = hc.case(key)
    W = hc.weights(C)
    exe = hc.build_probe(C, probe_dir, "g++")
    estimate = worst = ratio = 0.0
    switch_estimate = switch_worst = 0.0
    for ip, x in enumerate(C.points):
        for it, theta in enumerate(C.thetas):
            r = _probed(key, probe_dir, ip, it)[1]
            assert np.all(np.isfinite(r.S))
            smooth = it >= ON_A_SWITCH.get(key, 0)
            if not smooth:
                # on a switch: one expression per weight vector (tests/test_mixed.py)
                WP = _piece_weights(C)
                rp = hc.run_probe(C, exe, probe_dir, x, WP, theta, "pieces")
            for l in range(C.n_par):
                if smooth:
                    with warnings.catch_warnings():
                        warnings.simplefilter("ignore", RuntimeWarning)
                        ref, err = hc.oracle_second(C, x, W, theta, l)
                    assert np.all(np.isfinite(err)), (key, ip, it, l)
                    for k in range(C.n_par):                                    # the group: (ip, it, (k, l))
                        scale = np.maximum(1.0, r.A[:, k, l])
                        own = float((err[:, k] / scale).max())
                        dev = float((np.abs(r.S[:, k, l] - ref[:, k]).astype(float) / scale).max())
                        with capsys.disabled():
                            if os.environ.get("OG_SURFACE_REPORT") == "2":
                                print("pp %s point %d set %d pair (%d, %d): estimate %.3e probe %.3e" % (key, ip, it, k, l, own, dev))
                        assert own <= SMOOTH, (key, ip, it, k, l, own)
                        assert dev <= 10.0 * own, (key, ip, it, k, l, own, dev)
                        estimate, worst = max(estimate, own), max(worst, dev)
                        if own > 0:
                            ratio = max(ratio, dev / own)
                    continue
                forms = _switch_forms(C, x, WP, theta, l)
                assert all(np.all(np.isfinite(e)) for _, e in forms), (key, ip, it, l)
                for k in range(C.n_par):
                    scale = np.maximum(1.0, rp.A[:, k, l])
                    own = np.stack([e[:, k] / scale for _, e in forms])                                 # [5, K]
                    dev = np.stack([np.abs(rp.S[:, k, l] - f[:, k]).astype(float) / scale for f, _ in forms])
                    used = own <= SMOOTH
                    assert used.any(axis=0).all(), (key, ip, it, k, l, own)
                    group = float(own[used].max())          # the group's worst estimate over the forms that are used
                    ok = (used & (dev <= 10.0 * group)).any(axis=0)
                    assert ok.all(), (key, ip, it, k, l, group, np.argwhere(~ok), dev[:, ~ok])
                    switch_estimate = max(switch_estimate, group)
                    switch_worst = max(switch_worst, float(np.where(used, dev, np.inf).min(axis=0).max()))
    text = "smooth: estimate %.1e, probe %.1e, worst ratio %.2f" % (estimate, worst, ratio)
    if key in ON_A_SWITCH:
        text += "; on a switch: estimate %.1e, probe %.1e" % (switch_estimate, switch_worst)
    _note("case " + key, text)
    with capsys.disabled():
        if os.environ.get("OG_SURFACE_REPORT"):
            print("parameter hessian %-5s %s" % (key, text))
    if key == "NLP":                    # both parameters enter linearly, each in a slot of its own: S is +0.0 throughout,
        assert worst == 0.0             # and where the reference's differences cancel exactly the probe agrees exactly
    else:
        assert estimate > 0 and worst > 0


# ------------------------------------------------------------------------------------------------ 2. closed forms
def _e_rows(C, theta, x):
    """``name -> rows`` of E's expressions in ``F`` (row 0 is the cost) and their values at ``(theta, x)``."""
    obj = hc.pc.Model()
    obj.q, obj.r, obj.table = theta[0], theta[1], C.obj.table
    row, rows_of, values = 1, {}, {}
    for name, fn in ec.E_EXPRESSIONS.items():
        v = np.atleast_1d(fn(obj, x[:4], x[4:8]) + 0.0 * x[0])
        rows_of[name], values[name] = np.arange(row, row + v.size), v
        row += v.size
    return rows_of, values


ULP4 = 4.0 * 2.0 ** -52         # 4 ulp of a result, relative: the two-rule chain of a quotient (csrc/og_dual2.h measures
                                # 6.2e-16 per rule term)


def test_closed_forms_on_e_off_the_switches(probe_dir):
    C = hc.case("E")
    exe = hc.build_probe(C, probe_dir, "g++")
    x = C.points[0]
    for it in range(ON_A_SWITCH["E"], len(C.thetas)):
        theta = C.thetas[it]
        q = float(theta[0])
        rows_of, values = _e_rows(C, theta, x)
        picks = [("q * r", int(rows_of["q * r"][2])), ("q ** 2", int(rows_of["q ** 2"][0])),
                 ("2 / q", int(rows_of["2 / q"][0])), ("log", int(rows_of["log"][0]))]
        W = np.zeros((len(picks), C.m))
        for d, (_, row) in enumerate(picks):
            W[d, row] = 1.0
        r = hc.run_probe(C, exe, probe_dir, x, W, theta, "closed")
        for name in ("q * r", "q ** 2", "2 / q", "log"):                        # (the rows are those expressions')
            assert np.allclose(r.F0[rows_of[name]], values[name], rtol=1e-14, atol=0), name
        assert _same(r.S[0], np.array([[0.0, 1.0], [1.0, 0.0]])), (it, r.S[0])  # q * r + x: cross 1.0, diagonals +0.0
        assert _same(r.S[1], np.array([[2.0, 0.0], [0.0, 0.0]])), (it, r.S[1])  # q ** 2
        for d, want in ((2, 4.0 / q ** 3), (3, -1.0 / q ** 2)):
            got = r.S[d]
            assert abs(got[0, 0] - want) <= ULP4 * abs(want), (it, picks[d][0], got[0, 0], want,
                                                               abs(got[0, 0] - want) / abs(want) / 2.0 ** -52)
            assert _same(got[0, 1:], np.zeros(1)) and _same(got[1], np.zeros(2))


# ------------------------------------------------------------------------------------------------ 3. structure
@pytest.mark.parametrize("key", hc.KEYS)
def test_symmetry_and_the_owner_rule(key, probe_dir):
    """``S[l][k]`` is ``S[k][l]`` bit for bit; the probe walked the list of the parameter with fewer entries, the lower
    index at a tie (from ``codegen.ParameterPlan`` alone); a pair with an empty list is +0.0 with no work."""
    C, r = _probed(key, probe_dir)
    assert _same(r.S, np.transpose(r.S, (0, 2, 1))) and _same(r.A, np.transpose(r.A, (0, 2, 1)))
    ent = hc.entries(C)
    for q, (k, l) in enumerate(hc.pairs(C.n_par)):
        own = hc.owner(C, k, l)
        assert r.owner[q] == own and r.partner[q] == k + l - own and r.entries[q] == ent[own] == min(ent[k], ent[l])
        assert r.have[q].sum() == ent[own]
        if k == l:
            assert r.checked2[q] == ent[k]              # the diagonal: slot 2 is slot 1, every entry is held to it
            assert _same(r.D1[q], r.D2[q])
        if ent[own] == 0:
            assert not r.S[:, k, l].any() and not np.signbit(r.S[:, k, l]).any() and not r.A[:, k, l].any()
    assert not r.S[6].any() and not np.signbit(r.S[6]).any(), "the zero vector: +0.0 everywhere"


def test_the_shapes_cover_every_path(probe_dir):
    want = {"G17": [17, 17, 17, 18], "G90": [90, 90, 90, 91], "G257": [257, 257, 257, 258]}
    for key, ent in want.items():
        assert hc.entries(hc.case(key)) == ent
    C, r = _probed("P2U", probe_dir)
    assert hc.entries(C)[4] == 0 and C.n_par == 6 and set(C.unread) == {4}
    # the operand term: `unit` (parameter 5) reaches the collocation operand - its own diagonal and its pair with `a`
    assert np.abs(r.S[2, 5, 5]) > 0 and np.abs(r.S[2, 0, 5]) > 0
    # a pair of one row item each that is held to the partner's entry (b, b) and pairs whose lists differ in shape
    assert r.checked2[hc.pairs(6).index((0, 5))] == 0 and r.entries[hc.pairs(6).index((0, 5))] == 9
    E, re_ = _probed("E", probe_dir)
    assert hc.entries(E) == [71, 9] and list(re_.owner) == [0, 1, 1] and list(re_.checked2) == [71, 9, 9]


def test_an_unread_parameter_gets_a_row_and_a_column_of_plus_zero(probe_dir):
    C = hc.case("P2U")
    for ip in range(len(C.points)):
        for it in range(len(C.thetas)):
            r = _probed("P2U", probe_dir, ip, it)[1]
            for k in C.unread:
                for part in (r.S[:, k, :], r.S[:, :, k], r.A[:, k, :], r.A[:, :, k]):
                    assert not part.any() and not np.signbit(part).any()
            assert r.S[:, 5, 5].any()                                           # (a parameter that is read)


def test_a_parameter_that_enters_linearly_has_a_diagonal_of_plus_zero(probe_dir):
    C = hc.case("NLP")
    for ip in range(len(C.points)):
        for it in range(len(C.thetas)):
            r = _probed("NLP", probe_dir, ip, it)[1]
            d = np.diagonal(r.S, axis1=1, axis2=2)
            assert not d.any() and not np.signbit(d).any()
            assert r.entries.min() > 0                                          # (... over entries that were evaluated)


def test_a_vector_of_nine_is_the_call_with_that_vector_alone(probe_dir):
    for key in ("P2U", "G257"):
        C, r = _probed(key, probe_dir)
        exe, W = hc.build_probe(C, probe_dir, "g++"), hc.weights(C)
        assert W.shape[0] == 9
        for d in (0, 4, 8):
            one = hc.run_probe(C, exe, probe_dir, C.points[1], W[d], C.thetas[-1], "one")
            assert one.S.shape == (1, C.n_par, C.n_par) and _same(one.S[0], r.S[d]) and _same(one.F0, r.F0)
        three = hc.run_probe(C, exe, probe_dir, C.points[1], W[[2, 4, 6]], C.thetas[-1], "three")
        assert _same(three.S, r.S[[2, 4, 6]])


def test_a_zero_weight_is_not_skipped(probe_dir):
    """A row with ``w_r = 0`` stays a term: ``q * q * x`` of E has ``d2/dq2 = 2 x``, infinite for a state at infinity, and
    ``0 * inf`` must reach the sum."""
    C = hc.case("E")
    exe = hc.build_probe(C, probe_dir, "g++")
    theta = C.thetas[-1]
    W = np.zeros((1, C.m))
    fine = hc.run_probe(C, exe, probe_dir, C.points[0], W, theta, "zero")
    assert not fine.S.any() and not np.signbit(fine.S).any()
    x = C.points[0].copy()
    x[2] = np.inf
    r = hc.run_probe(C, exe, probe_dir, x, W, theta, "inf", check=False)
    assert np.isnan(r.S[0, 0, 0]), "0 * inf must reach the sum"


@pytest.mark.parametrize("key", ("E", "P2U"))
def test_other_compilers_and_the_sanitizers_give_the_same_bits(key, probe_dir):
    """clang++ and a g++ build under AddressSanitizer / UBSan (a plain process of its own, nothing preloaded)."""
    C, r = _probed(key, probe_dir)
    x, theta, W = C.points[1], C.thetas[-1], hc.weights(C)
    for other in (hc.build_probe(C, probe_dir, og_math_cases.clangxx()), hc.build_probe(C, probe_dir, "g++", sanitize=True)):
        o = hc.run_probe(C, other, probe_dir, x, W, theta, "other")
        assert _same(o.S, r.S) and _same(o.D1, r.D1) and _same(o.D2, r.D2) and np.array_equal(o.A, r.A)
    if key == "E":                                      # ... and on a switch set, with both seeds on a kinked leaf
        san = hc.build_probe(C, probe_dir, "g++", sanitize=True)
        for it in range(ON_A_SWITCH["E"]):
            o = hc.run_probe(C, san, probe_dir, x, W, C.thetas[it], "other")
            assert _same(o.S, _probed(key, probe_dir, 1, it)[1].S)


# ------------------------------------------------------------------------------------------------ 4. host logic
class StandIn:
    """``Problem``'s engine protocol without a device: the stand-in records its calls and returns a result that names
    the lane (its parameters, point and weights)."""

    m_eq = 0

    def __init__(self, prob, obj):
        C = hc.case("P2U")
        self.n, self.m, self.n_par = C.n, C.m, C.n_par
        self.theta = np.array(list(prob.parameters.values()), dtype=float)
        self.calls = []

    def set_parameters(self, theta):
        self.theta = np.asarray(theta, dtype=float).copy()

    def values(self, p):
        return np.float64(p[0]), np.zeros(2), np.zeros(self.m - 3)

    @staticmethod
    def result(theta, x, W):
        return np.stack([np.outer(theta, theta) * x[0] + np.sum(w) for w in W])

    def parameter_hessian(self, x, W):
        self.calls.append((self.theta.copy(), np.array(x, dtype=float), np.array(W, dtype=float)))
        return self.result(self.theta, x, W), np.zeros(self.m)


class NoSecond(StandIn):
    parameter_hessian = property()      # (hasattr is False)


def _p2u():
    C = hc.case("P2U")
    prob, obj = ec.CASES["P2U"][0]()
    return C, prob, obj, hc.weights(C)


def test_parameter_hessian_shapes(monkeypatch):
    monkeypatch.setattr(optimize, "ENGINE_FACTORY", StandIn)
    C, prob, obj, W = _p2u()
    x, th = C.points[0], C.thetas[0]
    got = prob.parameter_hessian(obj, W, x)
    eng = prob._engine
    assert got.shape == (9, C.n_par, C.n_par) and len(eng.calls) == 1 and getattr(prob, "_batch", None) is None
    assert np.array_equal(eng.calls[0][1], x) and np.array_equal(eng.calls[0][2], W)
    assert np.array_equal(got, StandIn.result(th, x, W))
    one = prob.parameter_hessian(obj, W[4], x)                              # a single vector: [n_par, n_par] back
    assert one.shape == (C.n_par, C.n_par) and eng.calls[-1][2].shape == (1, C.m)
    assert np.array_equal(one, prob.parameter_hessian(obj, W[4:5], x)[0])
    at_p = prob.parameter_hessian(obj, W[4])                                # the default point: prob.p
    assert np.array_equal(eng.calls[-1][1], prob.p) and at_p.shape == (C.n_par, C.n_par)
    prob.set_parameters(C.thetas[1])                                        # at new values: the engine is told first
    prob.parameter_hessian(obj, W[:2], x)
    assert np.array_equal(eng.calls[-1][0], C.thetas[1])


def test_refusals(monkeypatch):
    monkeypatch.setattr(optimize, "ENGINE_FACTORY", StandIn)
    C, prob, obj, W = _p2u()
    x = C.points[0]
    for bad in (W[0][:-1], W[:3, :-1], np.zeros((0, C.m)), np.zeros((3, 2, C.m)), np.append(W[0], 0.0)):
        with pytest.raises(ValueError, match="weights must have"):
            prob.parameter_hessian(obj, bad, x)
    X = np.stack([x, C.points[1]])
    for bad in (W[0], W[:2, :-1], np.zeros((2, 2, C.m))):
        with pytest.raises(ValueError, match="parameter_hessians must have shape"):
            prob.evaluate_batch(obj, X, parameter_hessians=bad)
    with pytest.raises(ValueError, match="parameter_hessians holds 3 rows for 2 points"):
        prob.evaluate_batch(obj, X, parameter_hessians=W[:3])
    monkeypatch.setattr(optimize, "ENGINE_FACTORY", NoSecond)
    C, prob, obj, W = _p2u()
    with pytest.raises(ValueError, match="no exact parameter Hessian"):
        prob.parameter_hessian(obj, W, x)
    with pytest.raises(ValueError, match="no exact parameter Hessian"):
        prob.evaluate_batch(obj, X, parameter_hessians=W[:2])
    assert prob.evaluate_batch(obj, X).parameter_hessian is None    # (nothing else needs the method)
    # a problem that declares no parameter
    monkeypatch.setattr(optimize, "ENGINE_FACTORY", StandIn)
    plain, pobj = problems.build("brachistochrone", nodes=[5])
    with pytest.raises(ValueError, match="declares no parameter"):
        plain.parameter_hessian(pobj, np.zeros(C.m))
    with pytest.raises(ValueError, match="declares no parameter"):
        plain.evaluate_batch(pobj, plain.p[None, :], parameter_hessians=np.zeros((1, C.m)))


def test_evaluate_batch_serves_every_lane_with_its_own_vector_and_parameters(monkeypatch):
    monkeypatch.setattr(optimize, "ENGINE_FACTORY", StandIn)
    C, prob, obj, W = _p2u()
    X = np.stack([C.points[0], C.points[1], C.points[0]])
    TH = np.stack([C.thetas[1], C.thetas[0], C.thetas[1]])
    res = prob.evaluate_batch(obj, X, parameters=TH, parameter_hessians=W[3:6])
    assert res.parameter_hessian.shape == (3, C.n_par, C.n_par)
    calls = prob._engine.calls
    assert len(calls) == 3 and [tuple(c[0]) for c in calls] == [tuple(t) for t in TH]
    for k in range(3):
        assert np.array_equal(res.parameter_hessian[k], StandIn.result(TH[k], X[k], W[3 + k:4 + k])[0])
        assert calls[k][2].shape == (1, C.m) and np.array_equal(calls[k][2][0], W[3 + k])
    plain = prob.evaluate_batch(obj, X, parameters=TH)
    assert plain.parameter_hessian is None and len(calls) == 3
    assert np.array_equal(plain.cost, res.cost)
    # one trajectory scanned over the parameter sets: its one vector goes with it
    scan = prob.evaluate_batch(obj, X[:1], parameters=TH, parameter_hessians=W[:1])
    assert scan.parameter_hessian.shape == (3, C.n_par, C.n_par)
    assert np.array_equal(scan.parameter_hessian[2], StandIn.result(TH[2], X[0], W[:1])[0])
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

        def parameter_hessian(self, X, W):
            raise AssertionError("parameter_hessian was called")

    class Engine:
        m_eq, n_par, m = 1, 6, 3

        def parameter_hessian(self, x, W):
            raise AssertionError("the engine's own parameter_hessian was called")

        def _load_pp_part(self):
            raise AssertionError("the part was asked for")

        def batch(self, B):
            bt = Batch()
            bt.engine = self
            return bt

    prob, obj = ec.CASES["P2U"][0]()
    prob._engine = Engine()
    X = np.stack([prob.p, prob.p])
    res = prob.evaluate_batch(obj, X)
    assert res.parameter_hessian is None and res.cost.shape == (2,)
    with pytest.raises(AssertionError, match="parameter_hessian was called"):
        prob.evaluate_batch(obj, X, parameter_hessians=np.zeros((2, 3)))
    prob._engine = None


# ------------------------------------------------------------------------------------------------ 5. the headers
# sha256 of the header of brachistochrone on 5 nodes as the code generator emitted it before the par_leaf overload of
# csrc/og_pp.h was added to the parameter section: a header without parameters has no such section and stays byte for
# byte what it was
PLAIN_HEADER_SHA256 = "136d5c33453adf1178b35d106949531181fda441c5cef5f2b3dafaa97c42c85d"


def test_a_header_without_parameters_is_what_it_was(monkeypatch, tmp_path):
    prob, obj = problems.build("brachistochrone", nodes=[5])
    first = codegen.emit_header(codegen.trace_problem(prob, obj))
    assert hashlib.sha256(first.encode()).hexdigest() == PLAIN_HEADER_SHA256
    for word in ("par_leaf", "par_seed", "OG_GEN_HAS_PAR"):
        assert word not in first
    # ... with the parameter-Hessian part requested in between: the request reads the header and does not change it
    monkeypatch.setattr(build, "JITDIR", str(tmp_path))
    seen = []

    def run(cmd):
        seen.append(cmd)
        with open(cmd[cmd.index("-o") + 1], "w") as fh:
            fh.write("part")
    monkeypatch.setattr(build, "_run", run)
    build.build_pp_part(first)
    assert len(seen) == 1
    with open(os.path.join(str(tmp_path), "og_gen_%s.h" % build.module_digest(first))) as fh:
        assert fh.read() == first
    prob, obj = problems.build("brachistochrone", nodes=[5])
    assert codegen.emit_header(codegen.trace_problem(prob, obj)) == first


@pytest.mark.parametrize("key", ("E", "P2U", "NLP", "G17"))
def test_a_parameterised_header_reads_every_parameter_leaf_as_before(key):
    """The call sites are what they were - ``par_leaf(x, cv, <index>, 0)`` - and the section has three overloads: the two
    it had, and the one an accessor with ``par_seed2`` selects."""
    C = hc.case(key)
    sites = re.findall(r"par_leaf\([^)]*\)", C.header)
    calls = [s for s in sites if not s.startswith("par_leaf(const X&")]
    assert calls and all(re.fullmatch(r"par_leaf\(x, cv, \d+, 0\)", s) for s in calls), [s for s in calls][:5]
    read = sorted({int(re.fullmatch(r"par_leaf\(x, cv, (\d+), 0\)", s).group(1)) - C.program.par_off for s in calls})
    assert read == sorted(set(range(C.n_par)) - set(C.unread))
    assert len(sites) - len(calls) == 3
    assert C.header.count("decltype((void)x.par_seed,") == 1 and C.header.count("decltype((void)x.par_seed2,") == 1
    assert C.header.count("const int i, long)") == 1


# ------------------------------------------------------------------------------------------------ 6. the build
def test_the_part_is_a_file_of_its_own(monkeypatch, tmp_path):
    assert build.PP_PART == 12
    assert (build.MODULE_PARTS, build.BATCH_PART, build.BATCH_EXACT_PART, build.PARAMETER_PART, build.DIRECTIONAL_PART,
            build.ADJOINT_PART, build.HESSIAN_PART, build.MIX_PART, build.HESSIAN_MATRIX_PART) == (
                (0, 2, 3, 1), 4, 5, 6, 7, 8, 9, 10, 11)
    out = build.module_path("0123456789abcdef")
    others = [build.part_path(out, i) for i in range(len(build.MODULE_PARTS))] + [
        build.batch_part_path(out), build.batch_exact_part_path(out), build.parameter_part_path(out),
        build.directional_part_path(out), build.adjoint_part_path(out), build.hessian_part_path(out),
        build.mix_part_path(out), build.hessian_matrix_part_path(out)]
    assert build.pp_part_path(out).endswith(".pp.so") and build.pp_part_path(out) not in others
    assert "og_pp.h" in [os.path.basename(p) for p in build._kernel_sources()]
    monkeypatch.setattr(build, "JITDIR", str(tmp_path))
    header = hc.case("P2U").header
    mod = build.module_path(build.module_digest(header))
    assert os.path.dirname(mod) == str(tmp_path)
    stale = {}
    for path in [build.part_path(mod, i) for i in range(4)] + [build.batch_part_path(mod), build.parameter_part_path(mod),
                                                               build.directional_part_path(mod),
                                                               build.adjoint_part_path(mod), build.hessian_part_path(mod),
                                                               build.mix_part_path(mod),
                                                               build.hessian_matrix_part_path(mod)]:
        with open(path, "w") as fh:
            fh.write("untouched " + os.path.basename(path))
        stale[path] = os.stat(path).st_mtime_ns
    commands = []

    def run(cmd):
        commands.append(cmd)
        with open(cmd[cmd.index("-o") + 1], "w") as fh:
            fh.write("part")
    monkeypatch.setattr(build, "_run", run)

    # only a first parameter_hessian call builds the part: an engine's other calls do not ask for it
    from opengoddard_amd import engine as engine_module

    class Lib:
        def og_parameter_hessian_load(self, handle, path):
            loaded.append(path.decode())
            return 0

    loaded = []
    eng = engine_module.HipEngine.__new__(engine_module.HipEngine)
    eng.header, eng._lib, eng._handle, eng.n_par = header, Lib(), None, 6
    assert commands == [] and getattr(eng, "pp_part_path", None) is None
    eng._load_pp_part()
    part = build.pp_part_path(mod)
    assert eng.pp_part_path == part and loaded == [part] and os.path.exists(part)
    assert len(commands) == 1 and "-DOGK_PART=12" in commands[0]
    for path, stamp in stale.items():
        assert os.stat(path).st_mtime_ns == stamp and open(path).read() == "untouched " + os.path.basename(path)
    made = set(os.listdir(str(tmp_path))) - {os.path.basename(p) for p in stale}
    assert made == {os.path.basename(part), "og_gen_%s.h" % build.module_digest(header)}
    eng._load_pp_part()
    assert build.build_pp_part(header) == part and len(commands) == 1 and loaded == [part]     # cached, loaded once
    eng.n_par = 0
    eng.pp_part_path = None
    with pytest.raises(ValueError, match="declares no parameter"):
        eng._load_pp_part()


def test_the_part_cross_compiles_and_knows_its_two_modes_only():
    header = hc.case("P2U").header
    part = build.build_pp_part(header)
    with open(part, "rb") as fh:
        blob = fh.read()
    assert b"gfx950" in blob and b"ogk_exact_pp" in blob and b"ogk_exact_pp_batch" in blob
    assert b"ogk_fused" not in blob and b"ogk_exact_mix" not in blob and b"ogk_exact_par" not in blob
    lib = ctypes.CDLL(part)
    assert hasattr(lib, "ogk_launch_batch") and hasattr(lib, "ogk_get_info")
    lib.ogk_launch.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p]
    lib.ogk_launch_batch.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p]
    # a record of zeros: the launcher refuses it before it touches the device (what og_parameter_hessian_load relies
    # on); a mode of another part is that part's
    record = ctypes.create_string_buffer(4096)
    invalid = 1                                         # hipErrorInvalidValue
    assert lib.ogk_launch(record, 27, None) == invalid
    assert lib.ogk_launch(record, 23, None) == -4242 and lib.ogk_launch(record, 15, None) == -4242
    assert lib.ogk_launch_batch(record, 28, None) == invalid and lib.ogk_launch_batch(None, 28, None) == invalid
    assert lib.ogk_launch_batch(record, 24, None) == -4242 and lib.ogk_launch_batch(record, 16, None) == -4242
    # a module without parameters: the part builds and refuses both modes
    prob, obj = problems.build("brachistochrone", nodes=[5])
    plain = ctypes.CDLL(build.build_pp_part(codegen.emit_header(codegen.trace_problem(prob, obj))))
    plain.ogk_launch.argtypes = lib.ogk_launch.argtypes
    plain.ogk_launch_batch.argtypes = lib.ogk_launch_batch.argtypes
    assert plain.ogk_launch(record, 27, None) == invalid and plain.ogk_launch_batch(record, 28, None) == invalid


# ------------------------------------------------------------------------------------------------ 7. the C signatures
FUNCTIONS = ("og_parameter_hessian_load", "og_parameter_hessian_dev", "og_parameter_hessian",
             "og_parameter_hessian_batch_dev", "og_parameter_hessian_batch")


def test_signatures_and_null_handles():
    C = ctypes
    dp = _native.SIGNATURES["og_directional"][1][1]                 # (the module's double pointer type)
    vp = C.c_void_p
    want = {
        "og_parameter_hessian_load": [vp, C.c_char_p],
        "og_parameter_hessian_dev": [vp, vp, C.c_int32, vp, vp, vp, vp],
        "og_parameter_hessian": [vp, dp, C.c_int32, dp, dp, dp],
        "og_parameter_hessian_batch_dev": [vp, C.c_int32, vp, vp, vp, vp, vp],
        "og_parameter_hessian_batch": [vp, C.c_int32, dp, dp, dp, dp],
    }
    assert set(want) == set(FUNCTIONS)
    with open(os.path.join(ROOT, "include", "ogpsx.h")) as fh:
        text = fh.read()
    lib = _native.lib()
    for name in FUNCTIONS:
        assert "int %s(" % name in text
        restype, argtypes = _native.SIGNATURES[name]
        assert restype is C.c_int and argtypes == want[name], name
        assert getattr(lib, name).argtypes == want[name]                # AttributeError: not exported

    def error_text():
        msg = lib.og_last_error()
        return msg.decode() if msg else ""

    ptr = _native.dptr(np.zeros(4))
    calls = {
        "og_parameter_hessian_load": (lambda: lib.og_parameter_hessian_load(None, b"/nonexistent.so"), "null handle"),
        "og_parameter_hessian_dev": (lambda: lib.og_parameter_hessian_dev(None, 8, 1, 8, 8, None, None), "null argument"),
        "og_parameter_hessian": (lambda: lib.og_parameter_hessian(None, ptr, 1, ptr, ptr, None), "null argument"),
        "og_parameter_hessian_batch_dev": (lambda: lib.og_parameter_hessian_batch_dev(None, 1, 8, 8, None, 8, None),
                                           "null batch"),
        "og_parameter_hessian_batch": (lambda: lib.og_parameter_hessian_batch(None, 1, ptr, ptr, None, ptr), "null batch"),
    }
    for name, (call, what) in calls.items():
        assert call() == 1, name
        text = error_text()
        assert text.startswith(name + ":") and what in text, text
