"""Host logic vs the reference's goldens: LGL construction (og_lgl through the C ABI), the
decision-vector layout / getters / index helpers with their quirks, unit scaling, Guess."""
import json
import math
import os

import numpy as np
import pytest

from conftest import GOLDEN
from opengoddard_amd import _native
from opengoddard_amd.optimize import Condition, Dynamics, Guess, Problem

LGL_SIZES = (3, 4, 5, 10, 20, 25, 30, 40, 50, 80, 100, 128, 200)
# above the reference's float64 goldens, up to codegen.max_phase_nodes(1): tests/golden/lgl_hp.npz (tools/make_golden_lgl_hp.py)
LGL_HP_SIZES = (201, 255, 256, 257, 341, 452, 453, 632, 633, 840, 1187, 1188)


def lgl_sample(n):
    """``(rows, cols)`` of the entries of D that are compared one by one: every entry with ``|k - l| <= 3``, the first
    and last two rows and columns, the centre row, and 2000 seeded random entries."""
    k = np.arange(n)
    pick = np.zeros((n, n), dtype=bool)
    pick[np.abs(k[:, None] - k[None, :]) <= 3] = True
    for edge in (0, 1, n - 2, n - 1):
        pick[edge, :] = True
        pick[:, edge] = True
    pick[n // 2, :] = True
    rng = np.random.default_rng(n)
    pick[rng.integers(0, n, 2000), rng.integers(0, n, 2000)] = True
    return np.nonzero(pick)


@pytest.mark.parametrize("n", LGL_SIZES)
def test_lgl_matches_reference(n, lgl_golden):
    """north_star: index ordering identical; tau within 1e-15; w and D within 1e-12 *relative*
    (an absolute 1e-12 on D is below the reference's own error)."""
    tau, w, D = _native.lgl(n)
    rt, rw, rD = lgl_golden["tau_%d" % n], lgl_golden["w_%d" % n], lgl_golden["D_%d" % n]
    assert tau.shape == (n,) and w.shape == (n,) and D.shape == (n, n)
    assert np.all(np.diff(tau) > 0) and tau[0] == -1.0 and tau[-1] == 1.0
    assert np.max(np.abs(tau - rt)) <= 1e-15
    assert np.array_equal(tau, -tau[::-1])                     # antisymmetric to the bit
    assert np.max(np.abs(w / rw - 1.0)) <= 1e-12
    nz = rD != 0
    assert np.array_equal(D == 0, ~nz)                         # same structural zeros
    assert np.max(np.abs(D[nz] / rD[nz] - 1.0)) <= 1e-12
    assert D[0, 0] == -n * (n - 1) * 0.25 and D[-1, -1] == n * (n - 1) * 0.25


def test_lgl_known_values_and_errors():
    tau = _native.lgl(10)[0]      # printed by the reference's smoke script (optimize.py:1135-1150)
    ref = [-1, -0.91953391, -0.73877387, -0.47792495, -0.16527896]
    assert np.allclose(tau[:5], ref, atol=5e-9)
    assert abs(_native.lgl(20)[1].sum() - 2.0) < 1e-14          # quadrature weights sum to 2
    D = _native.lgl(30)[2]
    assert np.max(np.abs(D.sum(axis=1))) < 1e-11                # derivative of a constant
    t = _native.lgl(30)[0]
    assert np.max(np.abs(D @ t ** 3 - 3 * t ** 2)) < 1e-11      # exact for polynomials
    with pytest.raises(_native.NativeError):
        _native.lgl(2)
    with pytest.raises(ValueError):
        Problem([0.0, 1.0], [2], [1], [1])                      # quirk Q2


def _hp(pair):
    """A double-double pair as one high-precision array: ``np.longdouble`` where it has at least 64 significant bits
    (x86-64: 64, aarch64: 113), else mpmath numbers in an object array."""
    if np.finfo(np.longdouble).eps < 2e-19:
        return pair[0].astype(np.longdouble) + pair[1].astype(np.longdouble)
    import mpmath
    return np.array([mpmath.mpf(float(a)) + mpmath.mpf(float(b)) for a, b in zip(pair[0], pair[1])], dtype=object)


def _hp_of(values):
    """float64 numbers in the arithmetic of ``_hp`` (exactly)."""
    if np.finfo(np.longdouble).eps < 2e-19:
        return np.asarray(values, dtype=np.float64).astype(np.longdouble)
    import mpmath
    return np.array([mpmath.mpf(float(v)) for v in np.ravel(values)], dtype=object).reshape(np.shape(values))


def _whole(n, half, sign):
    """The whole symmetric rule from its non-negative half (the centre node first when ``n`` is odd)."""
    upper = half[1:] if n % 2 else half
    centre = half[:1] if n % 2 else half[:0]
    return np.concatenate([sign * upper[::-1], centre, upper])


def lgl_truth(n, G):
    """``(tau, P_{N-1}(tau))`` of the true rule in high precision, from tests/golden/lgl_hp.npz."""
    return _whole(n, _hp(G["tau_%d" % n]), -1), _whole(n, _hp(G["p_%d" % n]), -1 if (n - 1) % 2 else 1)


def lgl_rows(n):
    """The whole rows of D that the ``D @ v`` checks use."""
    return (0, 1, n // 2, n - 2, n - 1)


def lgl_errors(n, tau, w, D, G):
    """What ``(tau, w, D)`` is off by against the truth - worst absolute node error, worst relative weight error,
    worst relative error of D over ``lgl_sample`` - and, for ``v = tau ** 3`` and ``v = 1`` on the rows ``lgl_rows``,
    the worst ``|D @ v - v'|`` of this D beside the float64 sum's own bound with the true D."""
    tt, pt = lgl_truth(n, G)
    node = float(np.max(np.abs(_hp_of(tau) - tt)))
    wt = 2 / (n * (n - 1) * pt * pt)
    weight = float(np.max(np.abs(_hp_of(w) / wt - 1)))
    rows, cols = lgl_sample(n)
    off = rows != cols
    rows, cols = rows[off], cols[off]
    Dt = pt[rows] / pt[cols] / (tt[rows] - tt[cols])
    dmat = float(np.max(np.abs(_hp_of(D[rows, cols]) / Dt - 1)))
    eps = np.finfo(float).eps
    out = {"node": node, "weight": weight, "D": dmat}
    for name, v, dv in (("cubic", tau ** 3, 3 * tau ** 2), ("constant", np.ones(n), np.zeros(n))):
        got, allowed = 0.0, 0.0
        for r in lgl_rows(n):
            gap = tt[r] - tt
            gap[r] = 1
            row = pt[r] / pt / gap
            row[r] = D[r, r]                                        # (the diagonal is exact by construction)
            true_row = np.array([float(x) for x in row])            # the true D rounded to float64
            got = max(got, abs(float(D[r] @ v) - dv[r]))
            # what a float64 dot product of N terms may be off by (n eps sum |D_rl v_l|), the true row's own residual
            # on these float64 nodes, and the entries' allowed relative error times the same sum
            mass = float(np.abs(true_row) @ np.abs(v))
            allowed = max(allowed, abs(float(true_row @ v) - dv[r]) + n * eps * mass)
            out[name + "_mass"] = max(out.get(name + "_mass", 0.0), mass)
        out[name], out[name + "_true"] = got, allowed
    return out


def check_lgl_against_truth(n, tau, w, D, G, report=None):
    """The assertions of ``test_lgl_against_the_true_rule`` on one ``(tau, w, D)``: the host's or the device's."""
    assert tau.shape == (n,) and w.shape == (n,) and D.shape == (n, n)
    assert np.all(np.diff(tau) > 0) and tau[0] == -1.0 and tau[-1] == 1.0
    assert np.array_equal(tau, -tau[::-1])                                       # antisymmetric to the bit
    k = np.arange(n)
    assert np.array_equal(D == 0, (k[:, None] == k[None, :]) & (k[:, None] > 0) & (k[:, None] < n - 1))
    assert D[0, 0] == -n * (n - 1) * 0.25 and D[-1, -1] == n * (n - 1) * 0.25
    ref_node, ref_weight, ref_D = (float(v) for v in G["ref_%d" % n])
    E = lgl_errors(n, tau, w, D, G)
    if report is not None:
        report(n, E, (ref_node, ref_weight, ref_D))
    assert E["node"] <= 4 * ref_node, (n, E["node"], ref_node)
    assert E["weight"] <= 4 * ref_weight, (n, E["weight"], ref_weight)
    assert E["D"] <= 4 * ref_D, (n, E["D"], ref_D)
    assert abs(math.fsum(w) - 2.0) <= n * np.spacing(2.0)                        # quadrature: within N ulp
    for name in ("cubic", "constant"):
        assert E[name] <= E[name + "_true"] + 4 * ref_D * E[name + "_mass"], (n, name, E)


@pytest.fixture(scope="module")
def lgl_hp():
    return np.load(os.path.join(GOLDEN, "lgl_hp.npz"))


@pytest.mark.parametrize("n", LGL_HP_SIZES)
def test_lgl_against_the_true_rule(n, lgl_hp, capsys):
    """Above the reference's float64 goldens, up to the longest phase the engine accepts: ``oglgl::node``'s Newton
    iteration and ``P_{N-1}``'s recurrence against the true rule (mpmath, tests/golden/lgl_hp.npz).  Allowed: 4 times
    what the reference's own float64 construction is off by at that N - not 1, because both constructions round the
    same ill-conditioned quotient ``1 / (t_k - t_l)``, and which way a node's last bit falls is chance.  ``D @ tau ** 3``
    and ``D @ 1`` on whole rows: within what the same float64 sum with the true D rounded to float64 leaves (its own
    residual plus N eps sum |D_rl v_l|) plus the entries' allowed relative error times sum |D_rl v_l|.
    Measured and allowed figures per N: profiles/exact_surface.md."""
    def report(n, E, ref):
        if os.environ.get("OG_SURFACE_REPORT"):
            with capsys.disabled():
                print("lgl %5d node %.2e (ref %.2e) w %.2e (ref %.2e) D %.2e (ref %.2e) cubic %.2e (true D %.2e) "
                      "constant %.2e (true D %.2e)" % ((n, E["node"], ref[0], E["weight"], ref[1], E["D"], ref[2],
                                                        E["cubic"], E["cubic_true"], E["constant"], E["constant_true"])))
    tau, w, D = _native.lgl(n)
    check_lgl_against_truth(n, tau, w, D, lgl_hp, report)


def _load_layout():
    with open(os.path.join(GOLDEN, "layout.json")) as fh:
        return json.load(fh)


def test_layout_getters_and_index_helpers_match_reference():
    data = _load_layout()
    for case in data["layouts"]:
        nodes, ns, nc = case["nodes"], case["ns"], case["nc"]
        p = Problem([float(i) for i in range(len(nodes) + 1)], list(nodes), list(ns), list(nc))
        assert p.div == case["div"]
        assert int(p.number_of_variables) == case["nvar"]
        for i in range(len(nodes)):
            assert list(p.bounds[p.index_time_final(i)]) == case["tf_bounds"][i]
        p.p = np.arange(p.number_of_variables, dtype=float) + 0.5
        for name, args, expect in case["calls"]:
            if isinstance(expect, str) and expect.startswith("raise:"):
                with pytest.raises(Exception) as info:
                    getattr(p, name)(*args)
                assert type(info.value).__name__ == expect[6:], (name, args)
                continue
            got = getattr(p, name)(*args)
            if name == "time_update":
                # depends on tau: the reference's differs from og_lgl by <= 1.2e-16
                assert np.allclose(got, expect, rtol=0, atol=1e-14)
            else:
                assert np.array_equal(np.asarray(got, dtype=float), np.asarray(expect, dtype=float)), \
                    (name, args)


def test_units_bounds_and_time_scaling_match_reference():
    u = _load_layout()["units"]
    p = Problem([0.0, 100.0, 200.0], [5, 4], [2, 2], [1, 1])
    p.set_unit_states_all_section(0, 10.0)
    p.set_unit_controls_all_section(0, 4.0)
    p.set_unit_time(50.0)
    p.set_states_all_section(0, np.linspace(1.0, 9.0, 9))
    p.set_controls(0, 1, np.array([1.0, 2.0, 3.0, 4.0]))
    p.set_states_bounds(1, 0, -5.0, None)
    p.set_controls_bounds_all_section(0, None, 8.0)
    p.set_time_final_bounds(1, None, 300.0)
    assert np.array_equal(p.p, u["p"])
    assert [float(v) for v in p.time_init] == u["time_init"] and float(p.t0) == u["t0"]
    assert np.allclose(p.time_all_section, u["time_all_section"], rtol=0, atol=1e-14)
    got = [[None if b is None else float(b) for b in pair] for pair in p.bounds]
    assert got == u["bounds"]
    assert [float(p.time_start(i)) for i in range(2)] == u["time_start"]
    assert [float(p.time_final(i)) for i in range(2)] == u["time_final"]
    assert np.allclose(p.time_to_tau(p.time_all_section), u["tau_of_time"], rtol=0, atol=1e-14)


def test_guess_helpers_match_reference_bitwise():
    g = _load_layout()["guess"]
    t = np.array(g["t"])
    assert np.array_equal(Guess.linear(t, 1.5, -2.0), g["linear"])
    assert np.array_equal(Guess.cubic(t, 1.0, -0.6, 0.6, 0.25), g["cubic"])
    assert np.array_equal(Guess.constant(t, 3.25), g["constant"])
    assert np.array_equal(Guess.zeros(t), g["zeros"])


def test_condition_and_dynamics_semantics():
    c = Condition()
    c.equal(np.array([3.0, 4.0]), 1.0, unit=2.0)
    c.lower_bound(5.0, 2.0)
    c.upper_bound(np.array([1.0]), 4.0, unit=3.0)
    assert np.array_equal(c(), [1.0, 1.5, 3.0, 1.0])
    z = Condition(4)
    z.change_value(2, 7.0)
    assert np.array_equal(z(), [0, 0, 7.0, 0])
    p = Problem([0.0, 1.0], [4], [2], [1])
    p.set_unit_states(1, 0, 5.0)
    p.unit_time = 2.0
    d = Dynamics(p, 0)
    d[0] = np.arange(4.0)
    out = d()                                  # state 1 never assigned -> zeros (optimize.py:1111)
    assert np.array_equal(out, np.concatenate([np.arange(4.0) * 2.0, np.zeros(4)]))
    with pytest.raises(AssertionError):
        d[2] = 1.0


def test_setter_length_assertion_and_repr():
    p = Problem([0.0, 1.0], [4], [1], [1])
    with pytest.raises(AssertionError):
        p.set_states(0, 0, np.zeros(5))                          # quirk Q6
    assert "number of variables = 9" in repr(p)
