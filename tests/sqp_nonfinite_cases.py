"""The cases of tests/test_sqp_nonfinite.py (and of ``__graft_entry__.build``, which compiles the modules of the
Problem-API cases ahead of the GPU run): SLSQP at NON-FINITE TRIAL POINTS.

In a trajectory problem a full SQP step routinely lands where ``sqrt``, ``log`` or a division is NaN or inf.  That is a
trial point of the line search, not an error: SciPy's SLSQP cuts the step by tenths until the merit function is finite
again, does not see a NaN inequality row at all, and ends with mode 5 ("Singular matrix E in LSQ subproblem") when a
subproblem has to be built AT such a point.  The SQP driver (``opengoddard_amd/sqp.py``) and its restatement
(``oracle/slsqp_np.py``) are held to that here.

(a) ANALYTIC - ``fun(x) -> (f, c)`` / ``jac(x) -> (g, A)`` closures of two variables ``(a, b)`` with analytic gradients,
CPU only.  The base problem is ``min w (a - k)^2 + (b - 1)^2`` s.t. ``a + b = 1.5``, ``b + 0.5 >= 0``, ``-5 <= a, b <= 5``
from ``(0, 0)`` with ``w = 1``, ``k = 2``: its first full step goes to ``a = 1.75``.  Every case puts one term on it that
leaves its domain at ``a = 1``; ``kind = (where, what)`` names the non-finite value SciPy's own run has to meet at a trial
point.  (The equality cases take ``w = 3``, ``k = 0.8``: the first step still overshoots to ``a > 1``, the minimiser is
inside the domain - with ``k = 2`` it sits on the edge, where ``sqrt`` has no slope, and free-running iterates of two
correct solvers drift apart by 1e-8 of a step.)

====================  ==========  =====  ============================================================================
key                   where       what   the term
====================  ==========  =====  ============================================================================
``eq_nan``            equality    NaN    ``+ 0.5 (sqrt(1 - a) - 1)`` on the equality
``ineq_nan``          inequality  NaN    a second inequality ``sqrt(1 - a) - 0.2 >= 0``: the merit function does not
                                         see the NaN row, the point is TAKEN, the next subproblem is mode 5
``cost_nan_sqrt``     cost        NaN    ``- sqrt(1 - a)`` on the cost
``cost_nan_log``      cost        NaN    ``- 0.1 log(1 - a)`` on the cost (a barrier: the minimiser is inside)
``cost_pinf``         cost        +inf   ``- 0.1 log(max(1 - a, 0))``
``cost_ninf``         cost        -inf   ``+ 0.1 log(max(1 - a, 0))`` (the line search TAKES ``-inf``: mode 5)
``eq_pinf``           equality    +inf   ``- 0.1 log(max(1 - a, 0))`` on the equality
``eq_ninf``           equality    -inf   ``+ 0.1 log(max(1 - a, 0))`` on the equality
``two_cuts``          equality    -inf   ``eq_ninf`` with ``w = 1``, ``k = 1.2``: searches that cut twice in a row
``ineq_pinf``         inequality  +inf   a second inequality ``1 - 0.1 log(max(1 - a, 0)) >= 0`` (``+inf`` is feasible:
                                         TAKEN, mode 5)
``ineq_ninf``         inequality  -inf   a second inequality ``2 + log(max(1 - a, 0)) >= 0``
``first_cut_only``    cost        NaN    ``cost_nan_log`` from ``(0.6, 0.9)``: in every search the full step alone is
                                         non-finite, one cut brings it back inside
``all_ten_cuts``      cost        NaN    ``+ (1 - a)^1.5`` from ``(1, 0.5)``: value and slope are finite ON the edge, the
                                         direction points out of the domain, the search ends on ``line > 10``
``relaxed``           cost        NaN    a second inequality ``a^2 - 1 >= 0`` from ``(0.1, 0)``: its linearisation wants
                                         ``a >= 5.05``, ``b + 0.5 >= 0`` and the equality allow 2 - mode 4, the relaxed QP
                                         (``h4 != 1``); ``- 0.1 log(1.8 - a)`` on the cost, the full step goes to 2
``start_cost``        cost        NaN    ``cost_nan_sqrt`` from ``(2, 0)``: ``f(x0)`` and ``g(x0)`` are NaN
``start_eq``          equality    NaN    ``eq_nan`` from ``(2, 0)``: ``c(x0)`` itself is NaN
``start_cost_pinf``   cost        +inf   ``cost_pinf``, ``cost_ninf``, ``eq_pinf``, ``eq_ninf``, ``ineq_nan``, ``ineq_pinf`` from
``start_cost_ninf``   cost        -inf   ``(2, 0)``: which exit mode SciPy gives a FIRST subproblem on non-finite data - 5
``start_eq_pinf``     equality    +inf   when an equality row is non-finite, 4 ("Inequality constraints incompatible")
``start_eq_ninf``     equality    -inf   when only the gradient or an inequality row is
``start_ineq_nan``    inequality  NaN
``start_ineq_pinf``   inequality  +inf
``start_cost_value``  cost        NaN    ``cost_nan_log`` from ``(2, 0)``: ``f(x0)`` is NaN, its gradient ``0.1 / (1 - a)``
                                         is finite - the subproblems are sound, no trial point is ever accepted
====================  ==========  =====  ============================================================================

(b) PROBLEM API - one phase, two states ``x, v``, one control ``u``, times ``[0, 1]``: ``x' = v``, ``v' = u``,
``x(0) = 0``, ``v(0) = 0``, the final time fixed, every variable within ``[-5, 5]``, ``u >= -5`` as the inequality;
minimise ``PULL (x(1) - 0.9)^2 + integral u^2`` from the all-zero guess.  The weight ``PULL`` is the ``w`` of (a): the
first full step overshoots ``x(1) = 0.9`` and leaves the domain ``x < 1`` of the case's term, the optimum is inside.
The same four terms, on the traced callbacks (trace, module, engine, driver - the whole chain on the GPU):

====================  =====  ====  ==========  ======================================================================
key                   nodes  PULL  where       the term
====================  =====  ====  ==========  ======================================================================
``P_SQRT_DYN``        7      30    equality    ``x' = v + 0.3 (sqrt(1 - x) - 1)``: NaN in the defect rows
``P_LOG_INEQ``        6      30    inequality  ``log(1 - x) + 3 >= 0`` at every node (the NaN point costs more: cut)
``P_LOG_INEQ_TAKEN``  6      13.8  inequality  the same with a smaller overshoot: the NaN point is TAKEN, mode 5 (SciPy
                                               does so for ``PULL`` between 13.2 and 14.3)
``P_LOG_COST``        5      30    cost        running cost ``u^2 - 0.1 log(1 - x)``
``P_INF_COST``        9      30    cost        running cost ``u^2 + exp(2000 (x - 1))``: +inf from ``x = 1.355``
====================  =====  ====  ==========  ======================================================================
"""
import numpy as np

from opengoddard_amd import codegen
from opengoddard_amd.optimize import Condition, Dynamics, Problem

BOUND = 5.0


def classify(value):
    """'nan' / '+inf' / '-inf' of the worst entry of a value, or None when all are finite."""
    v = np.atleast_1d(np.asarray(value, dtype=float))
    if np.any(np.isnan(v)):
        return "nan"
    if np.any(v == np.inf):
        return "+inf"
    if np.any(v == -np.inf):
        return "-inf"
    return None


# ------------------------------------------------------------------------------------------------ (a) analytic
def _sqrt1(a):
    """sqrt(1 - a) and its derivative in a."""
    with np.errstate(all="ignore"):
        r = np.sqrt(1.0 - a)
        return r, -0.5 / r


def _log1(a, edge=1.0):
    with np.errstate(all="ignore"):
        return np.log(edge - a), -1.0 / (edge - a)


def _pow15(a):
    """(1 - a)^1.5: 0 with slope 0 ON the edge, NaN beyond it."""
    with np.errstate(all="ignore"):
        t = np.float64(1.0 - a)
        return t ** 1.5, -1.5 * t ** 0.5


def _logc(a):
    """log(max(1 - a, 0)): -inf beyond the edge, never NaN."""
    with np.errstate(all="ignore"):
        t = max(1.0 - a, 0.0)
        return np.log(t), -np.float64(1.0) / t


class Analytic:
    """``kind = (where, what)``; ``cost(a) -> (value, d/da)`` is ADDED to ``weight (a - centre)^2 + (b - 1)^2``, ``eq(a)``
    to ``a + b - 1.5``; ``ineq(a) -> (value, d/da)`` is a second inequality row."""

    def __init__(self, key, kind, cost=None, eq=None, ineq=None, x0=(0.0, 0.0), centre=2.0, weight=1.0, maxiter=100, ftol=1e-6):
        self.key, self.kind = key, kind
        self._cost, self._eq, self._ineq, self.centre, self.weight = cost, eq, ineq, centre, weight
        self.x0 = np.array(x0, dtype=float)
        self.n, self.meq, self.mineq = 2, 1, 1 + (ineq is not None)
        self.lb, self.ub = np.full(2, -BOUND), np.full(2, BOUND)
        self.maxiter, self.ftol = maxiter, ftol

    def _all(self, x):
        a, b = float(x[0]), float(x[1])
        k, w = self.centre, self.weight
        f, g = w * (a - k) ** 2 + (b - 1.0) ** 2, np.array([2.0 * w * (a - k), 2.0 * (b - 1.0)])
        if self._cost is not None:
            v, d = self._cost(a)
            f, g = f + v, g + np.array([d, 0.0])
        c, A = [a + b - 1.5], [[1.0, 1.0]]
        if self._eq is not None:
            v, d = self._eq(a)
            c[0] += v
            A[0][0] += d
        c.append(b + 0.5)
        A.append([0.0, 1.0])
        if self._ineq is not None:
            v, d = self._ineq(a)
            c.append(v)
            A.append([d, 0.0])
        return float(f), np.array(c, dtype=float), np.asarray(g, dtype=float), np.array(A, dtype=float)

    def fun(self, x):
        f, c, _, _ = self._all(x)
        return f, c

    def jac(self, x):
        _, _, g, A = self._all(x)
        return g, A

    def hit(self, f, c):
        """Is this value of ``fun`` non-finite in the intended way?"""
        where, what = self.kind
        part = {"cost": f, "equality": c[:self.meq], "inequality": c[self.meq:]}[where]
        return classify(part) == what


def _scaled(fn, k, shift=0.0):
    def term(a):
        v, d = fn(a)
        return k * v + shift, k * d
    return term


ANALYTIC = {c.key: c for c in [
    Analytic("eq_nan", ("equality", "nan"), eq=_scaled(_sqrt1, 0.5, -0.5), centre=0.8, weight=3.0),
    Analytic("ineq_nan", ("inequality", "nan"), ineq=_scaled(_sqrt1, 1.0, -0.2)),
    Analytic("cost_nan_sqrt", ("cost", "nan"), cost=_scaled(_sqrt1, -1.0), maxiter=400),
    Analytic("cost_nan_log", ("cost", "nan"), cost=_scaled(_log1, -0.1)),
    Analytic("cost_pinf", ("cost", "+inf"), cost=_scaled(_logc, -0.1)),
    Analytic("cost_ninf", ("cost", "-inf"), cost=_scaled(_logc, 0.1)),
    Analytic("eq_pinf", ("equality", "+inf"), eq=_scaled(_logc, -0.1), centre=0.8, weight=3.0),
    Analytic("eq_ninf", ("equality", "-inf"), eq=_scaled(_logc, 0.1), centre=0.8, weight=3.0),
    Analytic("two_cuts", ("equality", "-inf"), eq=_scaled(_logc, 0.1), centre=1.2),
    Analytic("ineq_pinf", ("inequality", "+inf"), ineq=_scaled(_logc, -0.1, 1.0)),
    Analytic("ineq_ninf", ("inequality", "-inf"), ineq=_scaled(_logc, 1.0, 2.0)),
    Analytic("first_cut_only", ("cost", "nan"), cost=_scaled(_log1, -0.1), x0=(0.6, 0.9)),
    Analytic("all_ten_cuts", ("cost", "nan"), cost=_pow15, x0=(1.0, 0.5)),
    Analytic("relaxed", ("cost", "nan"), cost=_scaled(lambda a: _log1(a, 1.8), -0.1), ineq=lambda a: (a * a - 1.0, 2.0 * a),
             x0=(0.1, 0.0)),
    Analytic("start_cost", ("cost", "nan"), cost=_scaled(_sqrt1, -1.0), x0=(2.0, 0.0)),
    Analytic("start_eq", ("equality", "nan"), eq=_scaled(_sqrt1, 0.5, -0.5), x0=(2.0, 0.0)),
    Analytic("start_cost_pinf", ("cost", "+inf"), cost=_scaled(_logc, -0.1), x0=(2.0, 0.0)),
    Analytic("start_cost_ninf", ("cost", "-inf"), cost=_scaled(_logc, 0.1), x0=(2.0, 0.0)),
    Analytic("start_eq_pinf", ("equality", "+inf"), eq=_scaled(_logc, -0.1), x0=(2.0, 0.0)),
    Analytic("start_eq_ninf", ("equality", "-inf"), eq=_scaled(_logc, 0.1), x0=(2.0, 0.0)),
    Analytic("start_ineq_nan", ("inequality", "nan"), ineq=_scaled(_sqrt1, 1.0, -0.2), x0=(2.0, 0.0)),
    Analytic("start_ineq_pinf", ("inequality", "+inf"), ineq=_scaled(_logc, -0.1, 1.0), x0=(2.0, 0.0)),
    Analytic("start_cost_value", ("cost", "nan"), cost=_scaled(_log1, -0.1), x0=(2.0, 0.0)),
]}


# ------------------------------------------------------------------------------------------------ (b) Problem API
# key -> (nodes, where, what)
PROBLEMS = {
    "P_SQRT_DYN": (7, "equality", "nan"),
    "P_LOG_INEQ": (6, "inequality", "nan"),
    "P_LOG_INEQ_TAKEN": (6, "inequality", "nan"),
    "P_LOG_COST": (5, "cost", "nan"),
    "P_INF_COST": (9, "cost", "+inf"),
}
X_FINAL = 0.9
PULL = {"P_SQRT_DYN": 30.0, "P_LOG_INEQ": 30.0, "P_LOG_INEQ_TAKEN": 13.8, "P_LOG_COST": 30.0, "P_INF_COST": 30.0}


class Obj:
    pass


def problem(key):
    """-> ``(prob, obj)``, at its guess (all zeros but the final time, which is fixed)."""
    nodes = PROBLEMS[key][0]
    prob = Problem([0.0, 1.0], [nodes], [2], [1], 1)
    obj = Obj()

    def dynamics(prob, obj, section):
        x, v, u = prob.states(0, section), prob.states(1, section), prob.controls(0, section)
        dx = Dynamics(prob, section)
        dx[0] = v + 0.3 * (np.sqrt(1.0 - x) - 1.0) if key == "P_SQRT_DYN" else v
        dx[1] = u
        return dx()

    def equality(prob, obj):
        rows = Condition()
        rows.equal(prob.states(0, 0)[0], 0.0)
        rows.equal(prob.states(1, 0)[0], 0.0)
        rows.equal(prob.time_final(-1), 1.0)
        return rows()

    def inequality(prob, obj):
        rows = Condition()
        rows.lower_bound(prob.controls_all_section(0), -BOUND)
        if key.startswith("P_LOG_INEQ"):
            rows.lower_bound(np.log(1.0 - prob.states_all_section(0)) + 3.0, 0.0)
        return rows()

    def running_cost(prob, obj):
        x, u = prob.states_all_section(0), prob.controls_all_section(0)
        if key == "P_LOG_COST":
            return u * u - 0.1 * np.log(1.0 - x)
        if key == "P_INF_COST":
            return u * u + np.exp(2000.0 * (x - 1.0))
        return u * u

    prob.dynamics = [dynamics]
    prob.knot_states_smooth = []
    prob.cost = lambda prob, obj: PULL[key] * (prob.states(0, 0)[-1] - X_FINAL) ** 2
    prob.running_cost = running_cost
    prob.equality = equality
    prob.inequality = inequality
    prob.set_states_bounds_all_section(0, -BOUND, BOUND)
    prob.set_states_bounds_all_section(1, -BOUND, BOUND)
    prob.set_controls_bounds_all_section(0, -BOUND, BOUND)
    prob.set_time_final_bounds(0, 0.5, 2.0)
    return prob, obj


_TRACED = {}


def traced(key):
    """-> ``(prob, obj, program, header)`` of a key, traced once."""
    if key not in _TRACED:
        import warnings
        prob, obj = problem(key)
        with warnings.catch_warnings(), np.errstate(all="ignore"):
            warnings.simplefilter("ignore", RuntimeWarning)
            program = codegen.trace_problem(prob, obj)
        _TRACED[key] = (prob, obj, program, codegen.emit_header(program))
    return _TRACED[key]


# what __graft_entry__.build compiles for tests/test_sqp_nonfinite.py: (label, header)
def modules():
    return [("sqp non-finite " + key, traced(key)[3]) for key in PROBLEMS]
