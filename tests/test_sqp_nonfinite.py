"""SLSQP at non-finite trial points ("non-finite trial points"; the cases and what each of them
is for: tests/sqp_nonfinite_cases.py; measured mismatches: profiles/sqp_nonfinite.md).

CPU: SciPy's own run of every case meets the non-finite trial point the case is for; the restatement
(``oracle/slsqp_np.py``), free-running, reproduces SciPy's status, message and counts, and its accepted iterates but for
the cases named in ``WEAKER`` and ``DRIFTING``; the driver
(``opengoddard_amd/sqp.py: minimize_slsqp_hip``) on a stand-in engine and QP core built from the restatement's own QP
reproduces the restatement bit for bit.

GPU: the Problem-API cases through ``Problem.solve`` with either SQP core, the driver against the restatement on the
twin, the persistent-zero ``J_T`` across solves after a NaN sweep, and the guard in front of the QP core seen from
outside.  No test hands the QP core non-finite data."""
import warnings

import numpy as np
import pytest
from scipy.optimize import minimize

import sqp_nonfinite_cases as nc
from opengoddard_amd import _native, sqp
from oracle import np_path, slsqp_np, twin

# the bound of test_slsqp_core.py::test_slsqp_restatement_replays_scipy_iterates for the small problems
WORST, TYPICAL = 1e-9, 1e-11
# ... and of test_gpu_qp_replays_scipy_iterates
GPU_WORST, GPU_TYPICAL = 1e-6, 1e-9
MAXITER, FTOL = 25, 1e-6                         # of the Problem-API cases


# ------------------------------------------------------------------------------------------- cases and their runs
class TwinCase:
    """A Problem-API case behind the interface of ``nc.Analytic``: the compiled CPU twin's values, SciPy's forward
    differences of them."""

    def __init__(self, key):
        self.key = key
        self.prob, self.obj, self.program, self.header = nc.traced(key)
        self.twin = twin.Twin(self.prob, self.obj, program=self.program)
        self.lb, self.ub = np_path.bounds_arrays(self.prob)
        self.n, self.meq, self.mineq = self.program.n, self.program.m_eq, self.program.m_ineq
        self.x0 = np.array(self.prob.p, dtype=float)
        self.kind = nc.PROBLEMS[key][1:]
        self.maxiter, self.ftol = MAXITER, FTOL

    def fun(self, x):
        F = self.twin.values(x)
        return float(F[0]), F[1:]

    def jac(self, x):
        _, JT = self.twin.sweep(x, _native.fd_step(x, self.lb, self.ub))
        return JT[:, 0].copy(), JT[:, 1:].T.copy()

    hit = nc.Analytic.hit


_CASES = {}


def case(key):
    if key not in _CASES:
        _CASES[key] = nc.ANALYTIC[key] if key in nc.ANALYTIC else TwinCase(key)
    return _CASES[key]


class Logged:
    """``fun`` / ``jac`` of a case, logging every distinct call in order: ``("f", x, f, c)`` and ``("j", x)``."""

    def __init__(self, C):
        self.C = C
        self.events = []
        self._f = self._j = None

    def fun(self, x):
        x = np.array(x, dtype=float)
        if self._f is None or not np.array_equal(self._f[0], x, equal_nan=True):
            with np.errstate(all="ignore"):
                self._f = (x, self.C.fun(x))
        last = self.events[-1] if self.events else None
        if last is None or last[0] != "f" or not np.array_equal(last[1], x, equal_nan=True):
            self.events.append(("f", x, self._f[1][0], self._f[1][1]))
        return self._f[1]

    def jac(self, x):
        x = np.array(x, dtype=float)
        if self._j is None or not np.array_equal(self._j[0], x, equal_nan=True):
            with np.errstate(all="ignore"):
                self._j = (x, self.C.jac(x))
        last = self.events[-1] if self.events else None
        if last is None or last[0] != "j" or not np.array_equal(last[1], x, equal_nan=True):
            self.events.append(("j", x))
        return self._j[1]

    def iterates(self):
        """Where the Jacobian was asked for: the start and every accepted iterate."""
        out = []
        for e in self.events:
            if e[0] == "j" and not (out and np.array_equal(out[-1], e[1], equal_nan=True)):
                out.append(e[1])
        return out

    def searches(self):
        """Per stretch of evaluations between two linearisations: was each one non-finite in the case's way?"""
        out, cur = [], []
        for e in self.events:
            if e[0] == "j":
                if cur:
                    out.append(cur)
                cur = []
            else:
                cur.append(bool(self.C.hit(e[2], e[3])))
        if cur:
            out.append(cur)
        return out


_SCIPY = {}


def outside(key):
    """A start of a Problem-API case that is outside the domain of its term: ``x = 1.5`` at the third node."""
    x0 = case(key).x0.copy()
    x0[2] = 1.5
    return x0


def scipy_run(key, outside_start=False):
    """SciPy's SLSQP, live, on the case's callbacks -> (result, log); computed once per session."""
    if outside_start:
        key = (key, "outside")
    if key not in _SCIPY:
        C = case(key[0]) if outside_start else case(key)
        start = outside(key[0]) if outside_start else C.x0
        L = Logged(C)
        meq = C.meq
        cons = [{"type": "eq", "fun": lambda x: L.fun(x)[1][:meq], "jac": lambda x: L.jac(x)[1][:meq]},
                {"type": "ineq", "fun": lambda x: L.fun(x)[1][meq:], "jac": lambda x: L.jac(x)[1][meq:]}]
        with warnings.catch_warnings(), np.errstate(all="ignore"):
            warnings.simplefilter("ignore")
            res = minimize(lambda x: L.fun(x)[0], start.copy(), jac=lambda x: L.jac(x)[0],
                           bounds=list(zip(C.lb, C.ub)), constraints=cons, method="SLSQP",
                           options={"maxiter": C.maxiter, "ftol": C.ftol})
        _SCIPY[key] = (res, L)
    return _SCIPY[key]


_RESTATED = {}


def restatement_run(key, outside_start=False):
    """The restatement, free-running -> (result, log, QP calls as ``(augmented, mode, d)``)."""
    if outside_start:
        key = (key, "outside")
    if key not in _RESTATED:
        C = case(key[0]) if outside_start else case(key)
        start = outside(key[0]) if outside_start else C.x0
        L = Logged(C)
        solves = []

        def qp(Z, g, Cm, c, G, h, lb, ub):
            assert all(np.all(np.isfinite(v)) for v in (Z, g, Cm, c, G, h)), "a QP was solved on non-finite data"
            out = slsqp_np.qp_solve(Z, g, Cm, c, G, h, lb, ub)
            solves.append((Z.shape[0] == C.n + 1, out[3], out[0]))
            return out

        with warnings.catch_warnings(), np.errstate(all="ignore"):
            warnings.simplefilter("ignore")
            res = slsqp_np.slsqp(L.fun, L.jac, start.copy(), C.lb, C.ub, C.meq, ftol=C.ftol, maxiter=C.maxiter, qp=qp)
        _RESTATED[key] = (res, L, solves)
    return _RESTATED[key]


def mismatch(ours, theirs):
    """Per accepted iterate: ``|ours - theirs|`` and the length of the step that led to it (max norms)."""
    assert len(ours) == len(theirs)
    gap = np.array([np.max(np.abs(a - b)) for a, b in zip(ours[1:], theirs[1:])])
    step = np.array([np.max(np.abs(b - a)) for a, b in zip(theirs[:-1], theirs[1:])])
    return gap, step


ALL_KEYS = list(nc.ANALYTIC) + list(nc.PROBLEMS)


# ------------------------------------------------------------------------------------------- CPU: the table itself
@pytest.mark.parametrize("key", ALL_KEYS)
def test_scipys_own_run_meets_the_nonfinite_trial_point_the_case_is_for(key):
    """A case whose SciPy run never sees the non-finite value it is named after would be a test of nothing."""
    C = case(key)
    ref, L = scipy_run(key)
    searches = L.searches()
    assert sum(sum(s) for s in searches) >= 1, "SciPy never met a %s %s" % C.kind[::-1]
    assert np.all(np.abs(C.lb) <= nc.BOUND) and np.all(np.abs(C.ub) <= nc.BOUND) and np.all(np.isfinite(C.x0))
    assert np.all(np.isfinite(ref.x))                                      # no case relies on an overflow of x itself
    if key == "first_cut_only":
        assert max(sum(s) for s in searches) == 1                          # the full step alone, in every search ...
        assert any(s[-2:] == [True, False] for s in searches)              # ... and the first cut was accepted
    if key in ("two_cuts", "cost_nan_log", "cost_pinf", "ineq_ninf"):
        assert any(s[-2:] == [True, False] for s in searches) and ref.status == 0
    if key == "two_cuts":
        assert any(s[-3:] == [True, True, False] for s in searches)
    if key == "all_ten_cuts":
        assert [len(s) for s in searches if all(s)][-1] == 11 and ref.nfev == 12      # ended on line > 10
    if key.startswith("start_"):
        f0, c0 = C.fun(C.x0)
        assert C.hit(f0, c0)
    if key == "start_cost_value":
        assert np.all(np.isfinite(C.jac(C.x0)[0])) and ref.nfev == 1 + 11 * (ref.nit - 1)
    if key == "relaxed":
        # (seen in the restatement, which the next test ties to SciPy's run: the first subproblem is inconsistent, its
        # relaxed form has h4 = 1 - d[n] != 1, and the full step of THAT search is the non-finite one)
        _, _, solves = restatement_run(key)
        assert solves[0][:2] == (False, 4) and solves[1][:2] == (True, 1) and 0.0 < solves[1][2][C.n] < 1.0
        first = next(i for i, s in enumerate(searches) if len(s) > 1)       # (before it: evaluations of x0 alone)
        assert searches[first][0] is True


def typical(gap, step):
    """Median of mismatch / step, as test_slsqp_restatement_replays_scipy_iterates takes it."""
    return float(np.median(gap / np.maximum(step, 1e-12))) if gap.size else 0.0


# Under the WEAKER contract (fails like SciPy: ``status != 0``, ``success is False``, SciPy's ``nit``, no QP solved on
# non-finite data) instead of the median bound on the iterates:
# ``start_cost_value`` - SciPy (9, 100, 1090, 100), "Iteration limit reached".  No trial point is ever accepted, every
#     search ends on its tenth cut: 99 steps of 7.07e-11 at ``a = 2``, where doubles are spaced 4.4e-16 apart.  The
#     restatement's iterates are SciPy's to one or two spacings (worst 6.7e-13 of max(step, 1e-3): that bound holds and is
#     asserted), which is 3e-6 .. 6e-6 of such a step: median mismatch / step 3.1e-06 against the bound of 1e-11.  The
#     counts, status and message are SciPy's all the same, and are asserted.
WEAKER = ("start_cost_value",)
# Not within the FREE-RUNNING iterate bound: the Problem-API cases.  Their Jacobians are forward differences of the
# callbacks, which turn 1e-13 in x into 1e-5 in A (oracle/slsqp_np.py: slsqp): worst free-running mismatch / step
# 5.6e-05 (P_SQRT_DYN), 5.6e-06 (P_LOG_INEQ), 2.5e-15 (P_LOG_INEQ_TAKEN), 3.7e-05 (P_LOG_COST), 1.1e-03 (P_INF_COST) against
# 1e-9.  Asserted for them instead: free-running counts, status and message; where both runs converge, the optimum within
# the bounds two converged solves are held to in test_solve_with_hip_core_converges_like_scipy_core (1e-6 on the cost,
# 1e-3 on x; measured 6e-11 and 1.4e-6); and every step within the bound when it starts from SciPy's previous iterate.
DRIFTING = tuple(nc.PROBLEMS)


@pytest.mark.parametrize("key", ALL_KEYS)
def test_restatement_free_running_reproduces_scipy_at_nonfinite_trial_points(key):
    """No teacher: status, message and counts are SciPy's, and so is every accepted iterate of the analytic cases.  (With
    Python's ``max`` in the step cut and ``np.maximum`` in the inequality terms ``eq_nan`` ends after 12 evaluations
    instead of 7, on a NaN iterate: checked, profiles/sqp_nonfinite.md.)  ``WEAKER`` and ``DRIFTING`` above name the cases
    that do not meet the iterate bounds, with their figures and what is asserted of them instead."""
    ref, Ls = scipy_run(key)
    ours, Lo, solves = restatement_run(key)
    assert (ours["status"], ours["nit"], ours["nfev"], ours["njev"]) == (ref.status, ref.nit, ref.nfev, ref.njev)
    assert ours["message"] == ref.message and ours["success"] == ref.success
    assert np.array_equal(np.isnan(ours["fun"]), np.isnan(ref.fun))
    C = case(key)
    if key not in DRIFTING:
        gap, step = mismatch(Lo.iterates(), Ls.iterates())
        assert np.max(np.abs(ours["x"] - ref.x)) <= WORST * max(1e-3, step.max(initial=0.0))
    else:
        drift, step = mismatch(Lo.iterates(), Ls.iterates())
        print("%s: free-running mismatch / step %.2e, |dx| %.2e, |dfun| %.2e" % (
            key, (drift / np.maximum(step, 1e-3)).max(initial=0.0), np.max(np.abs(ours["x"] - ref.x)),
            abs(ours["fun"] - ref.fun)))
        if ref.status == 0:
            assert abs(ours["fun"] - ref.fun) <= 1e-6 and np.max(np.abs(ours["x"] - ref.x)) <= 1e-3
        trace = []
        with warnings.catch_warnings(), np.errstate(all="ignore"):
            warnings.simplefilter("ignore")
            led = slsqp_np.slsqp(C.fun, C.jac, C.x0.copy(), C.lb, C.ub, C.meq, ftol=C.ftol, maxiter=C.maxiter,
                                 trace=trace, teacher=Ls.iterates())
        assert (led["status"], led["nit"], led["nfev"], led["njev"]) == (ref.status, ref.nit, ref.nfev, ref.njev)
        gap = np.array([t["mismatch"] for t in trace if "mismatch" in t])
        step = np.array([t["step"] for t in trace if "mismatch" in t])
        assert gap.size >= ref.njev - 1
    assert np.all(np.isfinite(gap))
    print("%s: %d iterates, worst mismatch / step %.2e, median %.2e" % (
        key, gap.size, (gap / np.maximum(step, 1e-3)).max(initial=0.0), typical(gap, step)))
    assert np.all(gap <= WORST * np.maximum(step, 1e-3)), (gap / np.maximum(step, 1e-3)).max()
    if key in WEAKER:
        assert ref.status != 0 and ours["status"] != 0 and ours["success"] is False and ours["nit"] == ref.nit
        assert len(solves) == ours["nit"] - 1                  # (each of them on finite data: restatement_run checks)
    else:
        assert typical(gap, step) <= TYPICAL


OUTSIDE_STARTS = {"P_SQRT_DYN": 5, "P_LOG_INEQ": 4, "P_LOG_COST": 4, "P_INF_COST": 4}


@pytest.mark.parametrize("key", list(OUTSIDE_STARTS))
def test_exit_mode_of_a_first_subproblem_on_nonfinite_data_at_the_traced_problems_sizes(key):
    """The mode 4 / mode 5 rule of ``_nonfinite_exit`` was read off two-variable problems; here it is at 16 to 28
    variables: a start outside the domain makes the first linearisation non-finite - the defect rows (mode 5), the
    inequality rows or the cost and its gradient (mode 4).  SciPy's answer, live, and the restatement's; no QP is solved."""
    C = case(key)
    f0, c0 = C.fun(outside(key))
    assert C.hit(f0, c0)
    ref, _ = scipy_run(key, outside_start=True)
    ours, _, solves = restatement_run(key, outside_start=True)
    assert (ref.status, ref.nit, ref.nfev, ref.njev) == (OUTSIDE_STARTS[key], 1, 1, 1)
    assert (ours["status"], ours["nit"], ours["nfev"], ours["njev"]) == (ref.status, ref.nit, ref.nfev, ref.njev)
    assert ours["message"] == ref.message and ours["success"] is False and not solves


def test_known_gap_an_equality_contradicted_by_a_bound_is_not_reported_incompatible():
    """Finite data; DESIGN.md section 10.  ``a^2 = 4`` linearised at ``a = 0.1`` wants ``d_a = 19.95``, the bound allows
    4.9 and the other variable does not enter the row.  SciPy answers such a subproblem with mode 4 and takes the relaxed
    QP.  ``qp_solve`` leaves the bound out of the active-set problem - its projection onto the null space of the equality
    vanishes - clips the step at the end and reports mode 1 with the equality violated.  This test records that: when the
    QP is mended it fails, and is to be turned round (mode 4)."""
    a = 0.1
    d, lam, mug, mode, _, _ = slsqp_np.qp_solve(np.eye(2), np.array([2.0 * (a - 2.0), -2.0]), np.array([[2.0 * a, 0.0]]),
                                                np.array([a * a - 4.0]), np.array([[0.0, 1.0]]), np.array([0.5]),
                                                np.array([-nc.BOUND - a, -nc.BOUND]), np.array([nc.BOUND - a, nc.BOUND]))
    assert mode == 1 and d[0] == nc.BOUND - a
    assert abs(2.0 * a * d[0] + a * a - 4.0) > 3.0           # the "solved" subproblem's equality: -3.01, not 0


# ------------------------------------------------------------------------------------------- CPU: the driver
class StandInEngine:
    """What ``minimize_slsqp_hip`` asks of an engine, on a case's closures.  (Test-only: the product has no CPU path.)"""

    def __init__(self, L):
        self.L = L
        C = L.C
        self.n, self.m_eq, self.m_ineq = C.n, C.meq, C.mineq
        self.m = 1 + C.meq + C.mineq
        jacobian = StandInJacobian(self)
        self._sqp_cache = (jacobian, StandInCore(jacobian, C.n, C.meq))

    def eval_stacked(self, x):
        f, c = self.L.fun(x)
        return np.concatenate([[f], c])


class StandInJacobian:
    """``DeviceJacobian`` without a device: ``ptr`` is the object itself, the core reads ``g`` and ``A`` from it."""
    stream = 0

    def __init__(self, engine):
        self.engine = engine
        self.ld = engine.m
        self.ptr = self

    def sweep(self, x, lb, ub):
        self.last_step = _native.fd_step(x, lb, ub)
        f, c = self.engine.L.fun(x)
        self.g, self.A = self.engine.L.jac(x)
        return np.concatenate([[f], c])


class StandInCore:
    """``QpCore`` on the restatement's own QP and BFGS update, keeping the factor the way the device does."""

    def __init__(self, jacobian, n, meq):
        self.n, self.meq = n, meq
        self.Z = np.eye(n)
        self.solves = 0

    def reset(self):
        self.Z = np.eye(self.n)

    def solve_dev(self, ptr, ld, g, c, dl, du, relaxed, rho, stream):
        n, meq = self.n, self.meq
        assert np.all(np.isfinite(g)) and np.all(np.isfinite(c)) and np.all(np.isfinite(ptr.A)), \
            "the QP core was handed non-finite data"
        self.solves += 1
        A = ptr.A
        if relaxed:
            Za = np.zeros((n + 1, n + 1))
            Za[:n, :n] = self.Z
            Za[n, n] = 1.0 / rho
            extra = np.concatenate([-c[:meq], np.maximum(-c[meq:], 0.0)])
            Aa = np.hstack([A, extra[:, None]])
            d, lam, mug, mode, _, info = slsqp_np.qp_solve(Za, np.append(g, 0.0), Aa[:meq], c[:meq], Aa[meq:], c[meq:],
                                                           dl, du)
        else:
            d, lam, mug, mode, Zq, info = slsqp_np.qp_solve(self.Z, g, A[:meq], c[:meq], A[meq:], c[meq:], dl, du)
            if mode == 1:
                self.Z = Zq
        bmult = info.get("bound_multipliers", np.zeros(d.size))
        return d, np.concatenate([lam, mug]), bmult, mode, info.get("ldp_iterations", 0)

    def jt_times(self, ptr, ld, coef, stream):
        with np.errstate(all="ignore"):
            out = ptr.A.T @ coef[1:]
            return out if coef[0] == 0.0 else coef[0] * ptr.g + out

    def bfgs(self, s, eta, Bs):
        Znew = slsqp_np.bfgs_factor_update(self.Z, s, eta, Bs)
        if Znew is None:
            return True
        self.Z = Znew
        return False

    def recoveries(self):
        return 0

    def resident_stats(self):
        return 0, 0

    def close(self):
        pass


def driver_run(key):
    C = case(key)
    L = Logged(C)
    engine = StandInEngine(L)
    with warnings.catch_warnings(), np.errstate(all="ignore"):
        warnings.simplefilter("ignore")
        res = sqp.minimize_slsqp_hip(engine, C.x0.copy(), C.lb, C.ub, ftol=C.ftol, maxiter=C.maxiter)
    return res, L, engine._sqp_cache[1]


@pytest.mark.parametrize("key", list(nc.ANALYTIC))
def test_driver_on_a_standin_core_reproduces_the_restatement_bit_for_bit(key):
    """``minimize_slsqp_hip`` with the restatement's QP behind the core's interface: the same decisions on the same
    numbers, so the same bits - counts, status, message, every trial point and every accepted iterate.  The stand-in
    core refuses non-finite data: the guard sits in front of it."""
    ours, Lo, _ = restatement_run(key)
    got, Ld, core = driver_run(key)
    assert (got.status, got.nit, got.nfev, got.njev) == (ours["status"], ours["nit"], ours["nfev"], ours["njev"])
    assert got.message == ours["message"] and got.success == ours["success"]
    mine, theirs = Ld.iterates(), Lo.iterates()
    assert len(mine) == len(theirs) and all(np.array_equal(a, b) for a, b in zip(mine, theirs))
    trials = [[e[1] for e in L.events if e[0] == "f"] for L in (Ld, Lo)]
    assert len(trials[0]) == len(trials[1]) and all(np.array_equal(a, b) for a, b in zip(*trials))
    assert np.array_equal(got.x, ours["x"]) and np.array_equal(got.fun, ours["fun"], equal_nan=True)
    assert got.timing["qp_solves"] == core.solves


def test_guard_ends_the_solve_before_the_core_sees_a_nonfinite_linearisation():
    """The cases that end on a non-finite linearisation: as many QP solves as finite linearisations (none from a
    non-finite start), SciPy's ``nit`` and SciPy's mode - 5, or 4 for a first subproblem whose equality rows are finite."""
    ended = [("ineq_nan", 1), ("cost_ninf", 1), ("ineq_pinf", 1), ("all_ten_cuts", 1)]
    ended += [(key, 0) for key in nc.ANALYTIC if key.startswith("start_") and key != "start_cost_value"]
    modes = {}
    for key, solves in ended:
        ref, _ = scipy_run(key)
        got, Ld, core = driver_run(key)
        finite = sum(1 for x in Ld.iterates() if sqp._finite_linearisation(case(key).fun(x)[1], case(key).jac(x)[0]))
        assert core.solves == got.timing["qp_solves"] == finite == solves
        assert got.status == ref.status != 0 and got.success is False and got.nit == ref.nit
        modes[key] = got.status
    assert sorted(k for k, mode in modes.items() if mode == 4) == [
        "start_cost", "start_cost_ninf", "start_cost_pinf", "start_ineq_nan", "start_ineq_pinf"]       # every other one: 5


# ------------------------------------------------------------------------------------------- GPU
class EvalLog:
    """Every ``HipEngine.eval_stacked`` / ``DeviceJacobian.sweep`` result of the solves inside the ``with``."""

    def __init__(self, monkeypatch):
        from opengoddard_amd.engine import HipEngine
        self.values, self.sweeps = [], []
        ev, sw = HipEngine.eval_stacked, sqp.DeviceJacobian.sweep

        def eval_stacked(engine, x):
            F = ev(engine, x)
            self.values.append((np.array(x, dtype=float), F.copy()))
            return F

        def sweep(jacobian, x, lb, ub):
            F = sw(jacobian, x, lb, ub)
            self.sweeps.append((np.array(x, dtype=float), F.copy()))
            return F

        monkeypatch.setattr(HipEngine, "eval_stacked", eval_stacked)
        monkeypatch.setattr(sqp.DeviceJacobian, "sweep", sweep)


def solve_with(key, core):
    prob, obj = nc.problem(key)
    prob.maxIterator = 1
    with np.errstate(all="ignore"), warnings.catch_warnings():
        warnings.simplefilter("ignore")
        prob.solve(obj, maxiter=MAXITER, ftol=FTOL, sqp_core=core)
    return prob


@pytest.mark.gpu
@pytest.mark.parametrize("key", list(nc.PROBLEMS))
def test_solve_with_hip_core_meets_nonfinite_trial_points_like_scipy_core(key, monkeypatch, capsys):
    """``Problem.solve(sqp_core="hip")`` against ``sqp_core="scipy"``: equal status and counts; where SciPy converges
    the optimum within the bounds of test_solve_with_hip_core_converges_like_scipy_core, where it ends in mode 5 the
    same failure at the same iteration.  The device really was non-finite there, entry for entry like the twin."""
    C = case(key)
    log = EvalLog(monkeypatch)
    ours = solve_with(key, "hip")
    hip_values = list(log.values)
    ref = solve_with(key, "scipy")
    capsys.readouterr()
    a, b = ours.last_result, ref.last_result
    assert a.status == b.status and a.message == b.message
    assert (a.nit, a.nfev, a.njev) == (b.nit, b.nfev, b.njev)
    if b.status == 0:
        assert abs(a.fun - b.fun) <= 1e-6 and np.max(np.abs(ours.p - ref.p)) <= 1e-3
    else:
        assert a.status != 0 and a.success is False
    nonfinite = [(x, F) for x, F in hip_values if not np.all(np.isfinite(F))]
    assert nonfinite and any(C.hit(F[0], F[1:]) for _, F in nonfinite)
    for x, F in nonfinite:
        assert np.array_equal(F, C.twin.values(x), equal_nan=True)
    if b.status == 5:
        finite = sum(1 for _, F in log.sweeps[:a.njev] if np.all(np.isfinite(F)))
        assert ours.sqp_timing["qp_solves"] == finite == a.njev - 1       # the guard, seen from outside


@pytest.mark.gpu
@pytest.mark.parametrize("key", list(OUTSIDE_STARTS))
def test_solve_from_a_start_outside_the_domain_ends_like_scipy_core_before_any_qp(key, capsys):
    """The same starts through ``Problem.solve``: either core ends at once with the same mode and message, and the HIP
    core has solved no QP."""
    found = {}
    for core in ("hip", "scipy"):
        prob, obj = nc.problem(key)
        prob.p[2] = 1.5
        prob.maxIterator = 1
        with np.errstate(all="ignore"), warnings.catch_warnings():
            warnings.simplefilter("ignore")
            prob.solve(obj, maxiter=MAXITER, ftol=FTOL, sqp_core=core)
        found[core] = prob
    capsys.readouterr()
    a, b = found["hip"].last_result, found["scipy"].last_result
    assert (a.status, a.nit, a.nfev, a.njev) == (b.status, b.nit, b.nfev, b.njev) == (OUTSIDE_STARTS[key], 1, 1, 1)
    assert a.message == b.message and a.success is False
    assert found["hip"].sqp_timing["qp_solves"] == 0


@pytest.mark.gpu
@pytest.mark.parametrize("key", list(nc.PROBLEMS))
def test_hip_driver_against_the_restatement_on_the_twin_at_nonfinite_trial_points(key):
    """``minimize_slsqp_hip`` on the engine against the restatement on the twin, which is handed the driver's accepted
    iterates (as in test_gpu_qp_replays_scipy_iterates): equal counts and status, every step within its bound."""
    from conftest import record_measurement
    from opengoddard_amd.engine import HipEngine
    C = case(key)
    prob, obj = nc.problem(key)
    eng = HipEngine(prob, obj)
    accepted = [np.clip(C.x0, C.lb, C.ub)]
    with np.errstate(all="ignore"):
        got = sqp.minimize_slsqp_hip(eng, C.x0.copy(), C.lb, C.ub, ftol=FTOL, maxiter=MAXITER,
                                     callback=lambda x: accepted.append(x.copy()))
    eng.close()
    trace = []
    with np.errstate(all="ignore"), warnings.catch_warnings():
        warnings.simplefilter("ignore")
        ours = slsqp_np.slsqp(C.fun, C.jac, C.x0.copy(), C.lb, C.ub, C.meq, ftol=FTOL, maxiter=MAXITER, trace=trace,
                              teacher=accepted)
    assert (got.status, got.nit, got.nfev, got.njev) == (ours["status"], ours["nit"], ours["nfev"], ours["njev"])
    assert got.message == ours["message"]
    mism = np.array([t["mismatch"] for t in trace if "mismatch" in t])
    step = np.array([t["step"] for t in trace if "mismatch" in t])
    assert mism.size >= 1 and np.all(np.isfinite(mism))
    record_measurement("hip_driver_at_nonfinite_trial_points", key=key, subproblems=int(mism.size),
                       worst_ratio=float((mism / np.maximum(step, 1e-3)).max()),
                       median_ratio=float(np.median(mism / np.maximum(step, 1e-12))), bound=GPU_WORST)
    assert np.all(mism <= GPU_WORST * np.maximum(step, 1e-3)), (mism / np.maximum(step, 1e-3)).max()
    assert np.median(mism / np.maximum(step, 1e-12)) <= GPU_TYPICAL


@pytest.mark.gpu
def test_second_solve_on_an_engine_after_a_nan_sweep_gives_the_bits_of_a_fresh_engine():
    """The driver's ``J_T`` is registered persistent-zero: a sweep writes the non-zeros only.  ``P_LOG_INEQ_TAKEN`` ends
    on a non-finite linearisation, so its last sweep leaves NaN in that buffer; the next solve on the same engine, from
    a finite start, must not see any of it."""
    from opengoddard_amd.engine import HipEngine
    key = "P_LOG_INEQ_TAKEN"
    C = case(key)
    start = np.full(C.n, 0.1)                       # (every trial point from here is finite: nine full steps on the twin)
    start[-1] = C.x0[-1]

    def run(eng, x0):
        seen = []
        with np.errstate(all="ignore"):
            res = sqp.minimize_slsqp_hip(eng, x0.copy(), C.lb, C.ub, ftol=FTOL, maxiter=MAXITER,
                                         callback=lambda x: seen.append(x.copy()))
        return res, seen

    prob, obj = nc.problem(key)
    used = HipEngine(prob, obj)
    first, _ = run(used, C.x0)
    assert first.status == 5
    left = used._sqp_cache[0].d_JT.cpu().numpy()
    assert not np.all(np.isfinite(left))                                  # the NaN fill is really there
    again, seen_used = run(used, start)
    used.close()
    prob, obj = nc.problem(key)
    fresh = HipEngine(prob, obj)
    base, seen_fresh = run(fresh, start)
    fresh.close()
    assert base.nit >= 3 and np.all(np.isfinite(base.x))
    assert (again.status, again.nit, again.nfev, again.njev) == (base.status, base.nit, base.nfev, base.njev)
    assert len(seen_used) == len(seen_fresh) and all(np.array_equal(a, b) for a, b in zip(seen_used, seen_fresh))
    assert np.array_equal(again.x, base.x) and again.fun == base.fun
