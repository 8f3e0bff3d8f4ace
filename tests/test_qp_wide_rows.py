"""The HIP QP core on rows of 8193 to 16384 entries - five to eight workgroups per column-split panel of the wide LQ
sweep (``k_lq_panel16_wide``, ``ogsqp_lqwide.h``) - against QPs whose solution is known exactly.

``tests/test_qp_boundaries.py`` certifies the core up to rows of 2113 entries, the extended-precision referee's largest
case has 6149 (four column slabs); above that only finite iterates were asserted.  ``qp_referee.refine`` cannot follow
(a ``longdouble`` copy of Z and a QR of the active rows: minutes per answer at n = 16383), so the subproblems here are
built backwards from their answer (``oracle/qp_manufactured.py``): step, multipliers and active set are chosen, the data is
derived from them in integer arithmetic and is EXACT, and the reference costs two products with the matrix.

CPU: the builder itself - its data is exact (rational arithmetic), the NumPy restatement and the referee find the
builder's answer, and the comparison used on the GPU refuses each kind of wrong answer.

GPU: three shapes at the smallest sizes that put 5 and 8 workgroups on a panel and at the core's limits, each solved
cold, warm-started from its own rotated factor, and relaxed; then the limits themselves."""
import fractions
import functools
import time
import types

import numpy as np
import pytest

from conftest import record_measurement
from oracle import qp_manufactured, qp_referee, slsqp_np
from opengoddard_amd import _sqp_native, sqp
from test_qp_boundaries import TOL, default_forms  # noqa: F401  (the fixture is used by name)
from test_slsqp_core import canonical_ids

RHO = 100.0
KINDS = ("plain", "relaxed")


# ------------------------------------------------------------------------------------------- CPU: the builder
SMALL = [(24, 6, 30), (40, 10, 50), (60, 0, 90)]
SMALL_BOTH = [(n, meq, mg, kind) for n, meq, mg in SMALL for kind in KINDS]


@functools.lru_cache(maxsize=None)
def small(n, meq, mg):
    """A small manufactured QP, a third of the general rows and a quarter of the variables active (shared: read only)."""
    return qp_manufactured.manufacture(n + meq + mg, n, meq, mg, mg // 3, n // 8, n // 8, RHO)


def builders_answer(qp, kind):
    k = qp.kinds[kind]
    return 1, k["d"].copy(), k["mult"].copy(), k["bm"].copy(), list(qp.active)


def compare(qp, kind, answer):
    return qp_manufactured.compare(qp, kind, *answer, TOL["tol_d"], TOL["tol_mu"])


def relaxed_rounding_bound(qp):
    """How far the exact solution of the relaxed data can lie from the builder's ``d*``: at ``(d*, r*, bm*)`` the KKT
    residual is one rounding of g per entry (2^-53 |g_i|) and, in the delta row, one rounding of the pivot multiplier
    (2^-53 |extra_p r_p|); on the fixed active set the step moves by at most ``|B^-1|_2 = max(z^2)`` (>= 1 / rho^2)
    times the residual's 2-norm."""
    k = qp.kinds["relaxed"]
    g, p = k["g"], k["pivot"]
    delta_row = k["c"][p] * k["mult"][p]                       # (extra_p = -c_p: an equality, or a row with c_p < 0)
    return float((qp.z ** 2).max() * 2.0 ** -53 * np.sqrt(g @ g + delta_row ** 2))


@pytest.mark.parametrize("n,meq,mg", SMALL + [(1100, 300, 64)])
def test_manufactured_data_is_exact(n, meq, mg):
    """The plain kind's doubles satisfy the KKT conditions of their QP at ``(d*, r*, bm*)`` with NO residual, in rational
    arithmetic (in float64 at n = 1100, where the integer products run over several chunks: sums of multiples of 2^-12
    below 2^40 are exact in any order); the relaxed kind's feasibility is exact and its stationarity is off by one
    rounding of g per entry and of one multiplier in the delta row; the strict margins are the 0.25 the builder promises."""
    qp = small(n, meq, mg)
    A, F = qp.matrix(), fractions.Fraction
    general = np.array([j for j in qp.active if j < mg], dtype=int)
    inactive = np.setdiff1d(np.arange(mg), general)
    p, q = qp.kinds["plain"], qp.kinds["relaxed"]
    d = p["d"]
    # feasibility, both kinds: equalities and active rows hold exactly, the others by 0.25 or more
    for k, factor in ((p, 1.0), (q, 0.5)):                     # (relaxed: a_j d + c_j (1 - delta) on the rows with c_j < 0)
        value = A @ d + np.where((np.arange(qp.m) < meq) | (k["c"] < 0.0), factor, 1.0) * k["c"]
        assert not value[:meq].any() and not value[meq + general].any()
        assert value[meq + inactive].min() >= 0.25
    low = [(j - mg) >> 1 for j in qp.active if j >= mg and not (j - mg) & 1]
    up = [(j - mg) >> 1 for j in qp.active if j >= mg and (j - mg) & 1]
    assert np.array_equal(qp.lb[low], d[low]) and np.array_equal(qp.ub[up], d[up])
    assert (p["bm"][low] >= 0.25).all() and (p["bm"][up] <= -0.25).all() and (p["mult"][meq + general] >= 0.25).all()
    rest = np.setdiff1d(np.arange(n), low + up)
    assert (d[rest] - qp.lb[rest]).min() >= 0.25 and (qp.ub[rest] - d[rest]).min() >= 0.25
    assert not qp.zero_mult[:meq].any() and not p["mult"][qp.zero_mult].any() and not p["bm"][qp.zero_bm].any()
    assert 0.25 <= np.isinf(qp.lb[rest]).mean() <= 0.42 or n < 100      # (a third of them has no bounds)
    if n > 100:
        assert not (A.T @ p["mult"] + p["bm"] - d / qp.z ** 2 - p["g"]).any()
        return
    # stationarity in rational arithmetic
    Af = [[F(float(v)) for v in row] for row in A]

    def residual(k):
        return [F(float(d[i])) / F(float(qp.z[i])) ** 2 + F(float(k["g"][i])) - F(float(k["bm"][i])) -
                sum(Af[j][i] * F(float(k["mult"][j])) for j in range(qp.m)) for i in range(n)]

    assert not any(residual(p))
    extra = np.concatenate([-q["c"][:meq], np.maximum(-q["c"][meq:], 0.0)])
    # (one rounding to double behind one to longdouble: 2^-53 + 2^-63)
    assert all(abs(r) <= (F(2) ** -53 + F(2) ** -63) * abs(F(float(gi))) for r, gi in zip(residual(q), q["g"]))
    delta_row = F(RHO) ** 2 / 2 - sum(F(float(e)) * F(float(r)) for e, r in zip(extra, q["mult"]))
    pivot = q["pivot"]
    assert abs(delta_row) <= F(2) ** -53 * abs(F(float(extra[pivot])) * F(float(q["mult"][pivot])))
    assert pivot < meq or q["mult"][pivot] >= 0.25


@pytest.mark.parametrize("n,meq,mg,kind", SMALL_BOTH)
def test_restatement_finds_the_manufactured_answer(n, meq, mg, kind):
    qp = small(n, meq, mg)
    Z, g, A, c, lo, hi, _ = qp.data(kind)
    d, lam, mu, mode, _, info = slsqp_np.qp_solve(Z, g, A[:meq], c[:meq], A[meq:], c[meq:], lo, hi)
    assert mode == 1
    ids = canonical_ids(info["active"], mg)
    assert ids == qp.active
    measured = compare(qp, kind, (mode, d, np.concatenate([lam, mu]), info["bound_multipliers"], ids))
    assert measured["step"] <= 1e-11 and measured["multipliers"] <= 1e-11     # (test_gpu_qp_matches_restatement's 1e-11)


@pytest.mark.parametrize("n,meq,mg,kind", SMALL_BOTH)
def test_referee_certifies_the_manufactured_answer(n, meq, mg, kind):
    """``qp_referee.certify`` accepts ``(d*, r*, bm*, active)``, and its refined step lies on ``d*``: within the referee's
    own convergence (1e-15, the bound of test_certificate_accepts_the_restatement) for the exact plain data; within
    ``relaxed_rounding_bound`` for the relaxed data.  Measured: plain <= 4.7e-19; relaxed 2.6e-15 (n = 24), 8.4e-16 (40),
    3.7e-15 (60) against bounds of 2.2e-12 to 2.3e-12."""
    qp = small(n, meq, mg)
    data = qp.data(kind)
    status, d, mult, bm, active = builders_answer(qp, kind)
    measured = qp_referee.certify(*data, status, d, mult, bm, active, **TOL)
    distance, _, info = qp_referee.distances(*data, active, {"builder": d})
    bound = 1e-15 if kind == "plain" else relaxed_rounding_bound(qp)
    record_measurement("test_referee_certifies_the_manufactured_answer", n=n, kind=kind, distance=distance["builder"],
                       bound=bound, multipliers=measured["multipliers"], least_multiplier=measured["dual"])
    print("n = %d %s: |d_referee - d*| = %.2e (bound %.2e), multipliers %.2e" % (
        n, kind, distance["builder"], bound, measured["multipliers"]))
    assert info["active_rows"] == meq + len(active)
    assert distance["builder"] <= bound
    assert measured["multipliers"] <= 1e-13 and measured["dual"] > 0.0 and measured["primal"] <= 1e-15


@pytest.mark.parametrize("n,meq,mg,kind", SMALL_BOTH)
def test_comparison_accepts_the_answer_and_refuses_a_moved_step(n, meq, mg, kind):
    qp = small(n, meq, mg)
    assert compare(qp, kind, builders_answer(qp, kind)) == {"step": 0.0, "multipliers": 0.0}
    status, d, mult, bm, active = builders_answer(qp, kind)
    d[n // 2] += 1e-6
    with pytest.raises(qp_manufactured.ManufacturedError) as err:
        compare(qp, kind, (status, d, mult, bm, active))
    assert err.value.failed == ["step"], str(err.value)
    assert 0.4e-6 <= err.value.measured["step"] <= 1e-6        # (relative to max(1, |d*|_inf), |d*| <= 2)
    status, d, mult, bm, active = builders_answer(qp, kind)
    d[0] = np.nan
    with pytest.raises(qp_manufactured.ManufacturedError) as err:
        compare(qp, kind, (status, d, mult, bm, active))
    assert "step" in err.value.failed
    with pytest.raises(qp_manufactured.ManufacturedError) as err:
        compare(qp, kind, (4,) + builders_answer(qp, kind)[1:])
    assert err.value.failed == ["status"]


@pytest.mark.parametrize("n,meq,mg,kind", SMALL_BOTH)
def test_comparison_refuses_an_altered_multiplier(n, meq, mg, kind):
    """One slot at a time moved by 1e-4: an equality's, an active general row's, an active bound's (multipliers), an
    inactive row's and a free variable's bound slot (these must be exactly 0.0: refused at 1e-300 as well)."""
    qp = small(n, meq, mg)
    want = qp.kinds[kind]
    mscale = max(1.0, np.abs(want["mult"]).max(), np.abs(want["bm"]).max())
    assert 1e-4 > 1.2 * TOL["tol_mu"] * mscale                 # (the alteration is beyond the bound)
    general = [j for j in qp.active if j < mg]
    slots = [("mult", meq + general[0]), ("bm", int(np.argmax(np.abs(want["bm"]))))] + ([("mult", meq - 1)] if meq else [])
    for which, k in slots:
        status, d, mult, bm, active = builders_answer(qp, kind)
        (mult if which == "mult" else bm)[k] += 1e-4
        with pytest.raises(qp_manufactured.ManufacturedError) as err:
            compare(qp, kind, (status, d, mult, bm, active))
        assert err.value.failed == ["multipliers"], (which, k, str(err.value))
    zeros = [("mult", int(np.nonzero(qp.zero_mult)[0][0])), ("bm", int(np.nonzero(qp.zero_bm)[0][0]))]
    if kind == "relaxed":
        zeros.append(("bm", n))                                # (delta* is interior: its bound multiplier is 0)
    for which, k in zeros:
        for change, failed in ((1e-4, ["multipliers", "inactive multipliers"]), (1e-300, ["inactive multipliers"])):
            status, d, mult, bm, active = builders_answer(qp, kind)
            (mult if which == "mult" else bm)[k] += change
            with pytest.raises(qp_manufactured.ManufacturedError) as err:
                compare(qp, kind, (status, d, mult, bm, active))
            assert err.value.failed == failed, (which, k, change, str(err.value))


@pytest.mark.parametrize("n,meq,mg,kind", SMALL_BOTH)
def test_comparison_refuses_another_active_set(n, meq, mg, kind):
    """One row dropped (a general row, a bound), one row added (an inactive general row, the other bound of a variable
    at a bound, a free variable's bound, delta's bounds in the relaxed kind)."""
    qp = small(n, meq, mg)
    status, d, mult, bm, active = builders_answer(qp, kind)
    general = [j for j in active if j < mg]
    bounds = [j for j in active if j >= mg]
    outside = [j for j in range(mg + 2 * n) if j not in active]
    others = [active[:k] + active[k + 1:] for k in (active.index(general[0]), active.index(bounds[-1]))]
    other_side = mg + ((bounds[0] - mg) ^ 1)                   # (the other bound of a variable that is at a bound)
    others += [sorted(active + [j]) for j in (outside[0], other_side, outside[-1])]
    if kind == "relaxed":
        others += [active + [mg + 2 * n], active + [mg + 2 * n + 1]]
    for other in others:
        assert other != active
        with pytest.raises(qp_manufactured.ManufacturedError) as err:
            compare(qp, kind, (status, d, mult, bm, other))
        assert err.value.failed == ["active set"], (other, str(err.value))
    if kind == "relaxed":
        for delta in (0.0, 1.0):
            moved = d.copy()
            moved[n] = delta
            with pytest.raises(qp_manufactured.ManufacturedError) as err:
                compare(qp, kind, (status, moved, mult, bm, active))
            assert err.value.failed == ["step", "delta"]


# ------------------------------------------------------------------------------------------- GPU: rows of 8193 .. 16384
# The slab count of a panel is ceil((nq - k) / 2048), nq = n (plain) or n + 1 (relaxed); a sweep of m_eq reflectors walks
# the length down from nq to nq - m_eq, and the handle needs n + 1 - m_eq <= 6736: the smallest m_eq per n.
#   W5   plain nq 8193: five workgroups, the fifth holding ONE column (L = 1: the clamped dbl4 load, the masked lanes),
#        four full slabs from the second panel on; relaxed nq 8194 (L = 2).  The first handle with beyond_fallback.
#   W8a  eight workgroups with L = 1 in the eighth, seven from the second panel on; the sweep walks 8 -> 7 -> 6 -> 5 -> 4
#        slabs with last-slab widths = 1 mod 16.
#   W8b  the core's limit: plain nq 16383 (last slab 2047), relaxed nq 16384 (eight full slabs, the exact multiples of
#        2048 on the way down); n + 1 - m_eq = 6736, the null-space limit, at the same time.
# 64 general rows, 24 of them active; 20 lower-active and 20 upper-active bounds; a third of the other variables unbounded.
# Measured on the MI355X (worst of the case's three answers, relative as ``qp_manufactured.compare`` measures; factor: the
# stored factor against B^-1 after the cold plain solve; changes cold plain / warm / cold relaxed; seconds: building
# the QP on the host / uploads and read-back / the three solves):
#   case   step      multipliers  factor    changes      seconds
#   W5     3.6e-13   4.5e-13      5.3e-15   64 / 0 / 64  0.1 / 0.18 / 0.055 + 0.032 + 0.055
#   W8a    5.3e-13   2.0e-12      1.2e-14   64 / 0 / 64  0.9 / 0.22 / 0.332 + 0.295 + 0.333
#   W8b    5.3e-13   1.6e-12      1.6e-14   64 / 0 / 64  1.3 / 0.30 / 0.514 + 0.470 + 0.513
# (bounds: step 1e-9, multipliers 1e-7, factor 1e-12.)  The cold solves are the 64 changes the active set needs and no
# more; of a W8b test's 3.4 s, 1.3 are the 1.6e8 normal deviates of the matrix, 1.5 the solves and 0.3 the factor's trips.
# Tried once against a build whose panel exchange leaves the LAST slab's partial products out of the total when a panel has
# five or more workgroups (one column of 8193 at W5's first panel; no panel of up to four workgroups is touched): W5's
# cold and relaxed answers are refused with the step 9e-2 and the multipliers 3e-3 off, on the right active set.
WIDE_CASES = [("W5", 8193, 1458, 64), ("W8a", 14337, 7602, 64), ("W8b", 16383, 9648, 64)]
ACTIVE_GENERAL, AT_LOWER, AT_UPPER = 24, 20, 20


def device_rows(qp):
    """The Jacobian in the sweep's own layout on the device: n rows of leading dimension ``m + 1 + 5``, row i =
    ``[NaN, a_1i .. a_mi, NaN x 5]`` - ``include/ogsqp.h`` promises that column 0 is not read, and nothing behind column
    m belongs to the matrix: a read outside 1 .. m shows as a NaN in the answer.  -> ``(tensor, ld)``."""
    import torch
    ld = qp.m + 1 + 5
    jt = torch.full((qp.n, ld), float("nan"), dtype=torch.float64, device="cuda")
    jt[:, 1:qp.m + 1] = torch.from_numpy(qp.AT).cuda().to(torch.float64).div_(qp_manufactured.SCALE)
    torch.cuda.synchronize()
    return jt, ld


def solve_dev(core, qp, jt, ld, kind):
    k = qp.kinds[kind]
    lo, hi = qp.bounds(kind)
    t0 = time.time()
    d, mult, bm, status, iters = core.solve_dev(jt.data_ptr(), ld, k["g"], k["c"], lo, hi, kind == "relaxed", k["rho"])
    seconds = time.time() - t0
    answer = (status, d.copy(), mult.copy(), bm.copy(), sorted(int(v) for v in core.get_active()))
    return answer, iters, seconds


@pytest.mark.gpu
@pytest.mark.parametrize("case,n,meq,mg", WIDE_CASES, ids=[c[0] for c in WIDE_CASES])
def test_gpu_wide_rows_reach_the_manufactured_answer(case, n, meq, mg, default_forms):
    """One handle per case, the matrix uploaded once (``device_rows``), three subproblems through ``solve_dev``:

    1. ``set_factor(diag(z))``, ``set_active()``, plain: cold;
    2. plain again, the handle untouched: warm-started from the rows of 1 and from the dense rotated factor ``Z Q`` that 1
       left - the same B, hence the same answer, and the only place where the 5- to 8-slab sweep is applied to a dense
       factor; no change of the active set (what test_gpu_warm_started_active_set_reaches_the_same_solution asserts of
       an unchanged problem).  ``C (Z Q)`` is lower triangular already, up to rounding: the reflectors of the equalities
       are near the identity here, those of the 64 warm rows behind them are not;
    3. ``set_factor(diag(z))``, ``set_active()``, relaxed: cold, rows one entry longer.

    Every answer is the builder's (``qp_manufactured.compare`` at test_qp_boundaries' ``TOL``: status, active set, step,
    multipliers, exact zeros, delta inside (0, 1)); no wait gave up; the two-launch active-set form served (null spaces
    this large).  After 1 the stored factor is still a factor of B: ``Zg (Zg' v) = z^2 v`` for three random v within the
    1e-12 that test_gpu_qp_matches_restatement_on_random_qps asserts of ``Zg Zg'``.  The relaxed data is within
    ``relaxed_rounding_bound`` of an exact QP's: asserted to be below a hundredth of ``tol_d``."""
    import torch
    assert n + 1 - meq == sqp.MAX_NULL_SPACE and n + 1 <= sqp.MAX_N1 and meq + ACTIVE_GENERAL + AT_LOWER + AT_UPPER <= n
    t0 = time.time()
    qp = qp_manufactured.manufacture(n + meq + mg, n, meq, mg, ACTIVE_GENERAL, AT_LOWER, AT_UPPER, RHO)
    assert relaxed_rounding_bound(qp) <= 0.01 * TOL["tol_d"]
    t_build = time.time() - t0
    t0 = time.time()
    jt, ld = device_rows(qp)
    Z = qp.factor()
    core = _sqp_native.QpCore(n, meq, mg)
    try:
        core.set_factor(Z)
        core.set_active()
        t_moves = time.time() - t0
        cold, changes_cold, s1 = solve_dev(core, qp, jt, ld, "plain")
        t0 = time.time()
        Zg = core.get_factor()
        t_moves += time.time() - t0
        warm, changes_warm, s2 = solve_dev(core, qp, jt, ld, "plain")
        t0 = time.time()
        core.set_factor(Z)
        core.set_active()
        t_moves += time.time() - t0
        relaxed, changes_relaxed, s3 = solve_dev(core, qp, jt, ld, "relaxed")
        recoveries, resident = core.recoveries(), core.resident_stats()
    finally:
        core.close()
        del jt
        torch.cuda.empty_cache()
    del Z
    v = np.random.default_rng(n).standard_normal((n, 3))
    want = qp.z[:, None] ** 2 * v
    factor = float(np.abs(Zg @ (Zg.T @ v) - want).max() / np.abs(want).max())
    del Zg
    results, refused = {}, []
    for name, kind, answer in (("cold", "plain", cold), ("warm", "plain", warm), ("relaxed", "relaxed", relaxed)):
        try:
            results[name] = qp_manufactured.compare(qp, kind, *answer, TOL["tol_d"], TOL["tol_mu"])
        except qp_manufactured.ManufacturedError as exc:
            results[name] = exc.measured
            refused.append("%s: %s" % (name, exc))
    worst = {key: float(np.max([m.get(key, np.nan) for m in results.values()])) for key in ("step", "multipliers")}
    changes = [changes_cold, changes_warm, changes_relaxed]
    seconds = {"build": round(t_build, 2), "moves": round(t_moves, 2), "solves": [round(s, 3) for s in (s1, s2, s3)]}
    record_measurement("test_gpu_wide_rows_reach_the_manufactured_answer", case=case, n=n, m_eq=meq, step=worst["step"],
                       multipliers=worst["multipliers"], factor=factor, changes=changes, recoveries=recoveries,
                       each={k: m for k, m in results.items()}, seconds=seconds)
    print("%s: worst step %.2e multipliers %.2e factor %.2e; changes %s; recoveries %d; %s" % (
        case, worst["step"], worst["multipliers"], factor, changes, recoveries, seconds))
    assert not refused, "\n".join(refused)
    assert changes_cold >= len(qp.active) and changes_relaxed >= len(qp.active)
    assert changes_warm == 0
    assert recoveries == 0 and resident == (0, 0), (recoveries, resident)
    assert factor <= 1e-12


@pytest.mark.gpu
def test_gpu_limits_of_the_handle_are_the_ones_the_driver_announces(default_forms):
    """``og_qp_create`` refuses a 16384th variable and a null space of 6737 coordinates, by name and before it allocates
    anything (the checks precede the first allocation in ``og_qp_create``); ``sqp.MAX_N1`` and ``sqp.MAX_NULL_SPACE`` are
    those limits, and ``sqp.prepare`` gives a reason for the same shapes.  W8b above is the accepted side of both edges."""
    n_max, null_max = sqp.MAX_N1 - 1, sqp.MAX_NULL_SPACE
    assert WIDE_CASES[-1][1:3] == (n_max, n_max + 1 - null_max)
    with pytest.raises(_sqp_native.SqpNativeError, match="og_qp_create: more than %d variables" % n_max):
        _sqp_native.QpCore(n_max + 1, n_max + 2 - null_max, 0)             # (null space 6736: only the row length is over)
    with pytest.raises(_sqp_native.SqpNativeError, match=r"n \+ 1 - m_eq = %d" % (null_max + 1)):
        _sqp_native.QpCore(n_max, n_max - null_max, 0)
    assert str(sqp.MAX_N1) in sqp.prepare(types.SimpleNamespace(n=n_max + 1, m_eq=n_max + 2 - null_max))
    assert "null space" in sqp.prepare(types.SimpleNamespace(n=n_max, m_eq=n_max - null_max))
