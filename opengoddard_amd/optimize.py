"""Host-side mirror of ``OpenGoddard.optimize`` for the MI355X engine.

Same public surface as the reference module (``Problem``, ``Guess``, ``Condition``,
``Dynamics``; reference ``OpenGoddard/optimize.py:38-1127``) so that OpenGoddard problem scripts
run unmodified, but the hot path is different: ``Problem.solve`` traces the user callbacks once
(:mod:`opengoddard_amd.trace`), lowers them to HIP device code
(:mod:`opengoddard_amd.codegen`) and hands SciPy's SLSQP *analytic-looking* ``jac=`` callables
that are one batched forward-difference sweep on the GPU (:mod:`opengoddard_amd.engine`),
instead of letting SciPy call Python closures ``3n+2`` times per major iteration
(SURVEY.md section 3.3 / 8(b)).

The decision-vector layout, the getters' ``p*unit`` convention and the API quirks Q1-Q16 of
SURVEY.md Appendix A are reproduced on purpose; each method's docstring cites the reference
lines it mirrors.  There is no CPU evaluation path in ``solve``: without the HIP extension and
a GPU it raises.
"""
from __future__ import annotations

import os

import numpy as np

from . import trace as _tr

__all__ = ["Problem", "Guess", "Condition", "Dynamics", "BatchResult"]

# Callable ``factory(prob, obj) -> engine`` used by ``Problem.solve``.  ``None`` selects the HIP
# engine.  The test-suite swaps in the NumPy oracle here to exercise host logic without a GPU
# (tests/conftest.py); nothing in this package ever sets it.
ENGINE_FACTORY = None
# 'scipy': SciPy's Fortran SLSQP driven by GPU callbacks (the reference's own core);
# 'hip': the same major iteration with the QP subproblem on the GPU (sqp.py, include/ogsqp.h);
# 'auto': 'hip' from AUTO_HIP_FROM decision variables on, 'scipy' below, and 'scipy' whenever the HIP core cannot take
# the problem (its capacity limits, no torch: Problem.sqp_core_fallback says why).  SciPy's core is O(n^3) per major
# iteration (16 s at n = 1442 against a few ms for the HIP core).  Where the HIP core overtakes it was measured in
# round 4 (tools/small_n_crossover.sh, profiles/r04_small_n.jsonl, same solves, MI355X box): n = 81 0.37 s vs 0.44 s
# (a tie: both are Python start-up), n = 201 0.85 vs 4.40 s, n = 281 0.50 vs 4.79 s, n = 701 0.82 vs 29.5 s - the HIP
# core from everything above the smallest shipped example, which keeps the reference's own arithmetic, iterate for
# iterate.  (Round 3 drew the line at 400.)
DEFAULT_SQP_CORE = "auto"
AUTO_HIP_FROM = 150


def _default_engine(prob, obj, devices=None):
    from .engine import HipEngine        # raises if the HIP library / a GPU is missing
    return HipEngine(prob, obj, devices=devices)


def _noop():
    pass


class SparseHessian:
    """What :meth:`Problem.hessian_matrix` returns: ``values`` (``[K, nnz]``, or ``[nnz]`` for one weight vector) are the
    stored entries of the lower triangle in CSR form, ``cols[indptr[j]:indptr[j + 1]]`` the partners ``l <= j`` of
    variable ``j``."""

    def __init__(self, values, indptr, cols):
        self.values, self.indptr, self.cols = values, np.asarray(indptr), np.asarray(cols)
        self.n = self.indptr.size - 1

    def _row(self, d):
        return self.values if self.values.ndim == 1 else self.values[d]

    def tocsr(self, d=0, symmetric=True):
        """Weight vector ``d``'s Hessian as a ``scipy.sparse.csr_matrix``: the lower triangle mirrored
        (``symmetric=True``, the default) or as stored."""
        import scipy.sparse as sp
        vals = self._row(d)
        lower = sp.csr_matrix((vals, self.cols, self.indptr), shape=(self.n, self.n))
        if not symmetric:
            return lower
        rows = np.repeat(np.arange(self.n), np.diff(self.indptr))
        off = rows != self.cols
        return (lower + sp.csr_matrix((vals[off], (self.cols[off], rows[off])), shape=(self.n, self.n))).tocsr()

    def toarray(self, d=0):
        """Weight vector ``d``'s Hessian as a dense symmetric ``[n, n]`` array."""
        rows = np.repeat(np.arange(self.n), np.diff(self.indptr))
        out = np.zeros((self.n, self.n))
        out[rows, self.cols] = out[self.cols, rows] = self._row(d)
        return out


class BatchResult:
    """What :meth:`Problem.evaluate_batch` returns for ``B`` points: ``cost[B]``, ``equality[B, m_eq]``,
    ``inequality[B, m_ineq]`` and ``violation[B]`` - SLSQP's measure of infeasibility, ``sum |c_eq| +
    sum max(-c_ineq, 0)`` - and, when the Jacobians were asked for, ``gradient[B, n]`` (the cost gradient),
    ``steps[B, n]`` (the signed forward-difference steps), ``values[B, nnz]`` (the structural non-zeros of every
    point's transposed Jacobian ``J_T[j, r] = dF_r/dx_j`` of ``F = [cost | c_eq | c_ineq]``) and ``pattern =
    (indptr, rows)``: the entries of column ``j`` are ``values[:, indptr[j]:indptr[j + 1]]``, their rows
    ``rows[indptr[j]:indptr[j + 1]]``.  ``nonfinite[B]`` counts the non-finite rows of ``F`` per point.
    ``jacobian`` says what ``values`` and ``gradient`` hold: ``None`` (no Jacobians were asked for), ``"fd"`` (forward
    differences) or ``"exact"`` (forward-mode derivatives of the traced callbacks; there is no step, ``steps`` is
    ``None``).  ``parameters[B, n_par]`` are the values of the problem's run-time parameters each point was evaluated
    with, in declaration order (``n_par`` is 0 for a problem that declares none)."""

    def __init__(self, F, m_eq):
        F = np.asarray(F, dtype=float)
        self.cost = F[:, 0].copy()
        self.equality = F[:, 1:1 + m_eq].copy()
        self.inequality = F[:, 1 + m_eq:].copy()
        self.violation = np.sum(np.abs(self.equality), axis=1) + np.sum(np.maximum(-self.inequality, 0.0), axis=1)
        self.nonfinite = np.sum(~np.isfinite(F), axis=1).astype(np.int32)
        self.gradient = self.steps = self.values = self.pattern = None
        self.jacobian = None
        self.parameters = None          # [B, n_par]: the parameter values every point was evaluated with
        self.parameter_jacobian = None  # [B, n_par, m]: exact dF/dtheta (evaluate_batch(parameter_jacobian=True))
        self.directional = None         # [B, m]: exact F'(x_k) v_k (evaluate_batch(directions=V))
        self.adjoint = None             # [B, n]: exact F'(x_k)^T w_k (evaluate_batch(adjoints=W))
        self.hessian_product = None     # [B, n]: exact grad^2 (w_k . F)(x_k) v_k (evaluate_batch(hessian_products=(W, V)))
        self.adjoint_parameter = None   # [B, n_par, n]: exact d(F'(x_k)^T w_k)/dtheta (evaluate_batch(adjoint_parameter=W))
        self.parameter_hessian = None   # [B, n_par, n_par]: exact d2(w_k . F)(x_k)/dtheta2 (evaluate_batch(parameter_hessians=W))
        self.hessian = None             # [B, nnz]: exact sparse Hessian of w_k . F at x_k (evaluate_batch(hessians=W))
        self.hessian_pattern = None     # (indptr, cols) of it: the lower triangle in CSR form

    def __len__(self):
        return self.cost.shape[0]


class Problem:
    """Multi-phase LGL pseudospectral transcription of an optimal-control problem.

    Args mirror the reference constructor (``optimize.py:759-823``): ``time_init`` is the list
    of phase boundary times ``[t0, t1, ..., tS]``; ``nodes``, ``number_of_states``,
    ``number_of_controls`` are per-phase lists; ``maxIterator`` bounds the SLSQP restart loop.
    ``method`` is accepted and ignored exactly like the reference (quirk Q1).

    Decision vector ``p`` (``optimize.py:237-245, 781``): for each phase, ``state0[N] ...
    state_{ns-1}[N] control0[N] ...``; phases concatenated; the last ``S`` entries are the phase
    final times.  Everything in ``p`` is divided by its canonical unit.
    """

    # ------------------------------------------------------------------ construction
    def __init__(self, time_init, nodes, number_of_states, number_of_controls,
                 maxIterator=100, method="LGL"):
        assert isinstance(time_init, list), "error: time_init is not list"
        assert isinstance(nodes, list), "error: nodes are not list"
        assert isinstance(number_of_states, list), "error: number of states are not list"
        assert isinstance(number_of_controls, list), "error: number of controls are not list"
        assert len(time_init) == len(nodes) + 1, "error: time_init length is not match nodes length"
        assert len(nodes) == len(number_of_states), "error: nodes length is not match states length"
        assert len(nodes) == len(number_of_controls), \
            "error: nodes length is not match controls length"
        from . import _native

        self.nodes = nodes
        self.number_of_states = number_of_states
        self.number_of_controls = number_of_controls
        self.number_of_section = len(nodes)
        self.number_of_param = np.array(number_of_states) + np.array(number_of_controls)
        self.div = self._make_param_division(nodes, number_of_states, number_of_controls)
        self.number_of_variables = int(sum(self.number_of_param * nodes)) + self.number_of_section

        self.tau, self.w, self.D, self.time = [], [], [], []
        for i, n in enumerate(nodes):
            if n < 3:   # quirk Q2: the reference's Gauss-Jacobi call rejects fewer than 3 nodes
                raise ValueError("n must be positive.")
            tau, w, D = _native.lgl(n)
            self.tau.append(tau)
            self.w.append(w)
            self.D.append(D)
            self.time.append(self._phase_grid(time_init[i], time_init[i + 1], tau))
        self.maxIterator = maxIterator
        self.iterator = 0
        self.time_init = time_init
        self.t0 = time_init[0]
        self.time_all_section = np.concatenate(self.time)

        self.unit_states = [[1.0] * ns for ns in number_of_states]
        self.unit_controls = [[1.0] * nc for nc in number_of_controls]
        self.unit_time = 1.0

        self.p = np.zeros(self.number_of_variables, dtype=float)
        self.bounds = [(None, None)] * self.number_of_variables
        for i in range(self.number_of_section):
            self.set_time_final_bounds(i, 0.0, None)

        self.dynamics = [None] * self.number_of_section
        self.knot_states_smooth = [True] * (self.number_of_section - 1)
        self.cost = None
        self.running_cost = None
        self.cost_derivative = None
        self.equality = None
        self.inequality = None
        for i in range(self.number_of_section):
            self.set_time_final(i, time_init[i + 1])
        self._par_names = []            # run-time parameters in declaration order (parameter / set_parameter)
        self._par_values = []           # their current values: the list every Parameter of this problem reads

    # ------------------------------------------------------------------ run-time parameters
    def parameter(self, name, value):
        """Declare a scalar model constant that can change WITHOUT a new trace and a new module and return it
        (:class:`opengoddard_amd.trace.Parameter`): ``obj.T_max = prob.parameter("T_max", 3.5)``.  The callbacks use it
        like the number it replaces; in the compiled module it is entry ``index`` (the order of declaration) of a table
        on the device that ``set_parameter`` rewrites, so a trade study or a continuation in it re-solves on the same
        kernels, and ``evaluate_batch(..., parameters=...)`` gives every point of a batch values of its own.  The
        reference has no counterpart (its constants are attributes of ``obj``, read by Python at every call).

        Outside the callbacks a parameter is its current value (guesses, bounds, plots).  Set-up code is NOT followed:
        ``obj.c = 0.5 * np.sqrt(obj.g0)`` in ``__init__`` is a float at the value of that moment - such a quantity is a
        parameter itself, or it is computed inside the callback.  Scalars only; table values and interpolation knots
        stay constants.  A parameter no callback reads gives a ``RuntimeWarning`` when the problem is traced."""
        name = str(name)
        if name in self._par_names:
            raise ValueError("parameter %r is already declared" % name)
        self._par_names.append(name)
        self._par_values.append(float(value))
        return _tr.Parameter(name, len(self._par_names) - 1, self._par_values)

    @property
    def parameters(self):
        """``{name: current value}`` of the declared parameters, in declaration order."""
        return dict(zip(self._par_names, self._par_values))

    def set_parameters(self, values):
        """New values for declared parameters: ``{name: value}``, or all of them as a sequence in declaration order.
        A live engine (of an earlier ``solve`` / ``evaluate_batch``) is updated too, every lane of its batches
        included; the next ``solve`` loads the same module - no compiler runs - and starts from ``prob.p``."""
        if isinstance(values, dict):
            unknown = [k for k in values if k not in self._par_names]
            if unknown:
                raise ValueError("unknown parameter%s %s (declared: %s)" % ("s" if len(unknown) > 1 else "",
                                 ", ".join(repr(k) for k in unknown), ", ".join(self._par_names) or "none"))
            items = [(self._par_names.index(k), float(v)) for k, v in values.items()]
        else:
            vec = np.asarray(values, dtype=float).reshape(-1)
            if vec.size != len(self._par_names):
                raise ValueError("%d values for %d declared parameters" % (vec.size, len(self._par_names)))
            items = list(enumerate(float(v) for v in vec))
        for i, v in items:
            self._par_values[i] = v                      # (in place: the Parameter objects read this list)
        engine = getattr(self, "_engine", None)
        closed = engine is not None and hasattr(engine, "_handle") and not engine._handle.value      # (a closed HipEngine)
        if engine is not None and items and hasattr(engine, "set_parameters") and not closed:
            engine.set_parameters(list(self._par_values))

    def set_parameter(self, name, value):
        """``set_parameters({name: value})``."""
        self.set_parameters({name: value})

    def _batch_parameters(self, parameters, B):
        """``parameters`` of ``evaluate_batch`` -> ``[B', n_par]`` array (B' = B, or any when B == 1), or None."""
        n_par = len(self._par_names)
        if parameters is None:
            return None
        if n_par == 0:
            raise ValueError("parameters= given, but this problem declares no parameter")
        if isinstance(parameters, dict):
            unknown = [k for k in parameters if k not in self._par_names]
            if unknown:
                raise ValueError("unknown parameter%s %s (declared: %s)" % ("s" if len(unknown) > 1 else "",
                                 ", ".join(repr(k) for k in unknown), ", ".join(self._par_names)))
            cols = {k: np.asarray(v, dtype=float) for k, v in parameters.items()}
            sizes = {c.size for c in cols.values() if c.ndim > 0}
            if any(c.ndim > 1 for c in cols.values()) or len(sizes) > 1:
                raise ValueError("parameters: every entry must be a scalar or one [B] array")
            rows = sizes.pop() if sizes else B
            TH = np.tile(np.asarray(self._par_values, dtype=float), (rows, 1))
            for k, c in cols.items():
                TH[:, self._par_names.index(k)] = c
        else:
            TH = np.array(parameters, dtype=float)
            if TH.ndim != 2 or TH.shape[1] != n_par:
                raise ValueError("parameters must have shape [B, %d] (declaration order: %s), got %s"
                                 % (n_par, ", ".join(self._par_names), TH.shape))
        if TH.shape[0] != B and B != 1:
            raise ValueError("parameters has %d rows for %d points" % (TH.shape[0], B))
        if TH.shape[0] < 1:
            raise ValueError("parameters holds no row")
        return np.ascontiguousarray(TH)

    def _batch_engine(self, obj):
        """The engine of an earlier ``solve`` / ``evaluate_batch``, or a new one that the next ``solve`` closes."""
        engine = getattr(self, "_engine", None)
        if engine is None:
            engine = ENGINE_FACTORY(self, obj) if ENGINE_FACTORY is not None else _default_engine(self, obj)
            self._engine = engine
            self._engine_of_batch = True         # (solve closes an engine that was only made for batches)
        return engine

    def parameter_sensitivity(self, obj, p=None, exact=False):
        """``dF/dtheta`` of ``F = [cost | c_eq | c_ineq]`` at the decision vector ``p`` (default ``prob.p``) and the
        current parameter values, shape ``[n_par, m]``.

        ``exact=True``: forward-mode derivatives of the traced callbacks with the seed on the parameter's table entry -
        as exact as ``jacobian="exact"`` is in ``p``, no step and no forward-difference noise.  ONE call to the engine
        (``HipEngine.parameter_jacobian``: an evaluation and one small launch); no batch is made.  An engine without
        that method is a ``ValueError``.

        The default is forward differences: ONE batched evaluation of ``n_par + 1``
        lanes at the same point - lane 0 at ``theta``, lane ``k + 1`` at ``theta + h_k e_k`` with SciPy's step rule
        (``og_fd_step`` without bounds) - and row ``k`` is ``(F(theta + h_k e_k) - F(theta)) / h_k``, formed on the host.
        The lanes are not chunked: ``evaluate_batch`` re-creates the problem's batch with ``n_par + 1`` lanes when the one
        it has is smaller (a lane owns a dense n x m matrix on the device)."""
        from . import _native
        n_par = len(self._par_names)
        if n_par == 0:
            raise ValueError("this problem declares no parameter")
        if exact:
            engine = self._batch_engine(obj)
            if not hasattr(engine, "parameter_jacobian"):
                raise ValueError("this engine has no exact parameter Jacobian (it has no parameter_jacobian)")
            point = np.asarray(self.p if p is None else p, dtype=float).reshape(-1)
            return np.array(engine.parameter_jacobian(point)[0], dtype=float, copy=True)
        theta = np.asarray(self._par_values, dtype=float)
        inf = np.full(n_par, np.inf)
        h = _native.fd_step(theta, -inf, inf)
        TH = np.tile(theta, (n_par + 1, 1))
        TH[np.arange(1, n_par + 1), np.arange(n_par)] += h
        point = np.asarray(self.p if p is None else p, dtype=float).reshape(1, -1)
        res = self.evaluate_batch(obj, point, parameters=TH)
        F = np.hstack([res.cost[:, None], res.equality, res.inequality])
        return (F[1:] - F[0]) / h[:, None]

    @staticmethod
    def _phase_grid(ta, tb, tau):
        return (tb - ta) / 2.0 * tau + (tb + ta) / 2.0

    # LGL helpers kept under the reference's private names (``optimize.py:183-213``); the
    # numbers come from the native library (csrc/og_lgl.h), not from scipy.special.
    def _nodes_LGL(self, n):
        from . import _native
        return _native.lgl(n)[0]

    def _weight_LGL(self, n):
        from . import _native
        return _native.lgl(n)[1]

    def _differentiation_matrix_LGL(self, n):
        from . import _native
        return _native.lgl(n)[2]

    # ------------------------------------------------------------------ layout
    def _make_param_division(self, nodes, number_of_states, number_of_controls):
        """Cumulative slice ends per phase (``optimize.py:237-245``)."""
        ends, base = [], 0
        for n, ns, nc in zip(nodes, number_of_states, number_of_controls):
            row = [base + n * (k + 1) for k in range(ns + nc)]
            base = row[-1]
            ends.append(row)
        return ends

    def _division_states(self, state, section):
        """(back, front) of a state slice; negative indices leak through like the reference
        (``optimize.py:247-260``, quirk Q4)."""
        assert section < len(self.nodes), "section argument out of own section range"
        assert state < self.number_of_states[section], "states argument out of own states range"
        if state != 0:
            front = self.div[section][state - 1]
        elif section == 0:
            front = 0
        else:
            front = self.div[section - 1][-1]
        return self.div[section][state], front

    def _division_controls(self, control, section):
        """(back, front) of a control slice (``optimize.py:262-269``)."""
        assert section < len(self.nodes), "section argument out of own section range"
        assert control < self.number_of_controls[section], \
            "controls argument out of own controls range"
        at = self.number_of_states[section] + control
        return self.div[section][at], self.div[section][at - 1]

    def _tf_slot(self, section):
        return range(-self.number_of_section, 0)[section]

    # ------------------------------------------------------------------ getters
    def states(self, state, section):
        """State ``state`` of phase ``section`` in physical units (``optimize.py:271-284``)."""
        back, front = self._division_states(state, section)
        return self.p[front:back] * self.unit_states[section][state]

    def controls(self, control, section):
        """Control ``control`` of phase ``section`` in physical units (``optimize.py:302-315``)."""
        back, front = self._division_controls(control, section)
        return self.p[front:back] * self.unit_controls[section][control]

    def states_all_section(self, state):
        """All phases of one state, concatenated (``optimize.py:286-300``)."""
        return _tr.cat([self.states(state, i) for i in range(self.number_of_section)])

    def controls_all_section(self, control):
        """All phases of one control, concatenated (``optimize.py:317-331``)."""
        return _tr.cat([self.controls(control, i) for i in range(self.number_of_section)])

    def time_start(self, section):
        """Start time of a phase (``optimize.py:333-347``; quirk Q8 for phase 0)."""
        if section == 0:
            return self.t0
        slot = range(-self.number_of_section - 1, 0)[section]
        return self.p[slot] * self.unit_time

    def time_final(self, section):
        """Final time of a phase; negative ``section`` counts from the end (``optimize.py:349-360``)."""
        return self.p[self._tf_slot(section)] * self.unit_time

    def time_final_all_section(self):
        """List of all phase final times (``optimize.py:362-375``)."""
        return [self.time_final(i) for i in range(self.number_of_section)]

    # ------------------------------------------------------------------ setters
    def set_states(self, state, section, value):
        """``optimize.py:377-388`` (quirk Q6: length must equal the phase's node count)."""
        assert len(value) == self.nodes[section], "Error: value length is NOT match nodes length"
        back, front = self._division_states(state, section)
        self.p[front:back] = value / self.unit_states[section][state]

    def set_controls(self, control, section, value):
        """``optimize.py:404-415``."""
        assert len(value) == self.nodes[section], "Error: value length is NOT match nodes length"
        back, front = self._division_controls(control, section)
        self.p[front:back] = value / self.unit_controls[section][control]

    def _split_by_phase(self, value_all_section):
        at = 0
        for i, n in enumerate(self.nodes):
            yield i, value_all_section[at:at + n]
            at += n

    def set_states_all_section(self, state, value_all_section):
        """``optimize.py:390-402``."""
        for i, chunk in self._split_by_phase(value_all_section):
            self.set_states(state, i, chunk)

    def set_controls_all_section(self, control, value_all_section):
        """``optimize.py:417-429``."""
        for i, chunk in self._split_by_phase(value_all_section):
            self.set_controls(control, i, chunk)

    def set_time_final(self, section, value):
        """``optimize.py:431-440``."""
        self.p[self._tf_slot(section)] = value / self.unit_time

    # ------------------------------------------------------------------ bounds
    @staticmethod
    def _scaled_pair(lb, ub, unit, lb_default=None):
        lo = lb / unit if lb is not None else lb_default
        hi = ub / unit if ub is not None else None
        return lo, hi

    def set_states_bounds(self, state, section, lb, ub):
        """``optimize.py:442-455``."""
        pair = self._scaled_pair(lb, ub, self.unit_states[section][state])
        back, front = self._division_states(state, section)
        self.bounds[front:back] = [pair] * self.nodes[section]

    def set_states_bounds_all_section(self, state, lb, ub):
        """``optimize.py:457-467``."""
        for i in range(self.number_of_section):
            self.set_states_bounds(state, i, lb, ub)

    def set_controls_bounds(self, control, section, lb, ub):
        """``optimize.py:469-482``."""
        pair = self._scaled_pair(lb, ub, self.unit_controls[section][control])
        back, front = self._division_controls(control, section)
        self.bounds[front:back] = [pair] * self.nodes[section]

    def set_controls_bounds_all_section(self, control, lb, ub):
        """``optimize.py:484-494``."""
        for i in range(self.number_of_section):
            self.set_controls_bounds(control, i, lb, ub)

    def set_time_final_bounds(self, section, lb, ub):
        """``optimize.py:496-507``; a missing lower bound becomes 0.0, not -inf (quirk Q3)."""
        self.bounds[self.index_time_final(section)] = \
            self._scaled_pair(lb, ub, self.unit_time, lb_default=0.0)

    # ------------------------------------------------------------------ time helpers
    def time_to_tau(self, time):
        """Affine map of a time grid onto [-1, 1] (``optimize.py:509-516``)."""
        lo, hi = min(time), max(time)
        mid = (lo + hi) / 2
        return np.array([2 / (hi - lo) * (t - mid) for t in time])

    def time_update(self):
        """Rebuild the physical time grid from the optimised final times (``optimize.py:518-531``;
        starts from literal 0, quirk Q11)."""
        knots = [0] + self.time_final_all_section()
        self.time = [self._phase_grid(knots[i], knots[i + 1], self.tau[i])
                     for i in range(self.number_of_section)]
        return np.concatenate(self.time)

    def time_knots(self):
        """``optimize.py:533-540``."""
        return [0] + self.time_final_all_section()

    # ------------------------------------------------------------------ index helpers
    @staticmethod
    def _pick(front, back, index):
        if index is None:
            return front
        span = back - front
        assert index < span, "Error, index out of range"
        return front + (index + span if index < 0 else index)

    def index_states(self, state, section, index=None):
        """Position in ``p`` of a state sample (``optimize.py:542-559``, quirk Q5)."""
        back, front = self._division_states(state, section)
        return self._pick(front, back, index)

    def index_controls(self, control, section, index=None):
        """``optimize.py:561-568``."""
        back, front = self._division_controls(control, section)
        return self._pick(front, back, index)

    def index_time_final(self, section):
        """``optimize.py:570-572``."""
        return self.number_of_variables + self._tf_slot(section)

    # ------------------------------------------------------------------ canonical units
    def set_unit_states(self, state, section, value):
        """``optimize.py:579-588``."""
        self.unit_states[section][state] = value

    def set_unit_states_all_section(self, state, value):
        """``optimize.py:590-599``."""
        for i in range(self.number_of_section):
            self.unit_states[i][state] = value

    def set_unit_controls(self, control, section, value):
        """``optimize.py:601-610``."""
        self.unit_controls[section][control] = value

    def set_unit_controls_all_section(self, control, value):
        """``optimize.py:612-621``."""
        for i in range(self.number_of_section):
            self.unit_controls[i][control] = value

    def set_unit_time(self, value):
        """Switch to non-dimensional time (``optimize.py:623-639``, quirk Q8): ``time_init``,
        ``time``, ``t0`` and ``time_all_section`` become scaled, the tf entries of ``p`` are
        rewritten."""
        self.unit_time = value
        scaled = np.array(self.time_init) / value
        self.time_init = list(scaled)
        self.time = [self._phase_grid(scaled[i], scaled[i + 1], self.tau[i])
                     for i in range(self.number_of_section)]
        self.t0 = scaled[0]
        self.time_all_section = np.concatenate(self.time)
        for i in range(self.number_of_section):
            self.set_time_final(i, scaled[i + 1] * value)

    # ------------------------------------------------------------------ NLP assembly (traced once)
    def _collocation_derivative(self, section, vec):
        if _tr.is_sym(vec):
            return _tr.matvec(section, vec)
        return self.D[section].dot(vec)

    def _assemble_equality(self, obj):
        """User equalities, collocation defects ``D x - (tf-t0)/2 f``, knot continuity, in the
        reference's row order and operation order (``optimize.py:670-698``; quirks Q7, Q9)."""
        blocks = [self.equality(self, obj)]
        for i in range(self.number_of_section):
            deriv = [self._collocation_derivative(i, self.states(j, i) / self.unit_states[i][j])
                     for j in range(self.number_of_states[i])]
            t_a = self.time_start(i) / self.unit_time
            t_b = self.time_final(i) / self.unit_time
            rhs = self.dynamics[i](self, obj, i)
            blocks.append(_tr.cat(deriv) - (t_b - t_a) / 2.0 * rhs)
        for knot in range(self.number_of_section - 1):
            if self.number_of_states[knot] != self.number_of_states[knot + 1]:
                continue
            for s in range(self.number_of_states[knot]):
                left = self.states(s, knot) / self.unit_states[knot][s]
                right = self.states(s, knot + 1) / self.unit_states[knot][s]
                if self.knot_states_smooth[knot]:
                    blocks.append(left[-1] - right[0])
        return _tr.cat(blocks)

    def _assemble_cost(self, obj):
        """Mayer term plus LGL quadrature of the running cost with the raw weights, no
        ``(tf-t0)/2`` factor (``optimize.py:700-709``, quirk Q10)."""
        mayer = self.cost(self, obj)
        if self.running_cost is None:
            return mayer
        integrand = self.running_cost(self, obj) * np.concatenate(self.w)
        if _tr.is_sym(integrand):
            return mayer + _tr.seqsum(integrand)
        return mayer + sum(integrand)

    # ------------------------------------------------------------------ solve
    def solve(self, obj, display_func=_noop, **options):
        """Run the SLSQP restart loop (``optimize.py:649-755``) with GPU-evaluated callbacks.

        Options honoured are the reference's: ``ftol`` (1e-6) and ``maxiter`` (25); two more select what
        the reference does not have: ``sqp_core`` ("auto", the default: the HIP SQP core - QP subproblems on the GPU,
        sqp.py - from 150 decision variables on, SciPy's Fortran core below; "hip" / "scipy" force one) and
        ``jacobian="exact"`` (forward-mode derivatives of the traced callbacks instead of SciPy's
        forward differences; same optimum, fewer iterations, no FD noise).  Cost,
        equality and inequality values come from a single-column launch of the sweep kernel;
        the three Jacobians SLSQP asks for at each major iteration come from one
        forward-difference sweep over all ``n`` decision-vector columns, with SciPy's step
        rule.  A user ``cost_derivative`` is used as-is, like the
        reference does (``optimize.py:730-733``).
        """
        from scipy import optimize as _sciopt

        assert len(self.dynamics) != 0, "It must be set dynamics"
        assert self.cost is not None, "It must be set cost function"
        assert self.equality is not None, "It must be set equality function"
        assert self.inequality is not None, "It must be set inequality function"

        core = options.pop("sqp_core", None) or os.environ.get("OG_SQP_CORE", DEFAULT_SQP_CORE)
        if core not in ("scipy", "hip", "auto"):
            raise ValueError("sqp_core must be 'scipy', 'hip' or 'auto', got %r" % (core,))
        auto = core == "auto"
        if auto:
            # a stand-in engine of the test-suite (ENGINE_FACTORY) has no device-resident Jacobian for the HIP core
            core = "hip" if (self.number_of_variables >= AUTO_HIP_FROM and ENGINE_FACTORY is None) else "scipy"
        self.sqp_core_used = core
        self.sqp_core_fallback = None

        jacobian = options.pop("jacobian", None) or os.environ.get("OG_JACOBIAN", "fd")
        if jacobian not in ("fd", "exact"):
            raise ValueError("jacobian must be 'fd' or 'exact', got %r" % (jacobian,))

        # devices=[0, 1, ...]: the FD columns of every sweep are split over these GPUs of the node (one process,
        # RCCL all-gather of the packed non-zeros; include/ogpsx.h og_comm_init / og_multi_fd_sweep)
        devices = options.pop("devices", None)
        if devices is None and os.environ.get("OG_DEVICES"):
            devices = [int(v) for v in os.environ["OG_DEVICES"].split(",")]
        if devices is not None and len(devices) > 1 and ENGINE_FACTORY is not None:
            # not silently: a stand-in engine has no devices at all
            import warnings
            warnings.warn("Problem.solve: devices=%r is not used with a stand-in engine" % (list(devices),),
                          RuntimeWarning, stacklevel=2)
        # lanes of an earlier evaluate_batch (B dense matrices on the device) do not live through the solve, nor does the
        # engine evaluate_batch built for them: this solve makes its own
        stale = self.__dict__.pop("_batch", None)
        if stale is not None:
            stale.close()
        if self.__dict__.pop("_engine_of_batch", False) and getattr(self, "_engine", None) is not None \
                and hasattr(self._engine, "close"):
            self._engine.close()
        if ENGINE_FACTORY is not None:
            engine = ENGINE_FACTORY(self, obj)
        else:
            engine = _default_engine(self, obj, devices=devices)
        self._engine = engine
        if core == "hip" and auto:
            # 'auto' never makes a problem unsolvable that the reference's core solves (slowly): the HIP core needs
            # torch for its device buffers and has capacity limits (include/ogsqp.h) - when it cannot be built for this
            # problem the solve goes to SciPy's core and says so (sqp_core_used / sqp_core_fallback)
            from . import sqp as _sqp
            reason = _sqp.prepare(engine)
            if reason is not None:
                import warnings
                warnings.warn("Problem.solve: the HIP SQP core is not available for this problem (%s); "
                              "using SciPy's SLSQP core" % reason, RuntimeWarning, stacklevel=2)
                core = self.sqp_core_used = "scipy"
                self.sqp_core_fallback = reason
        if jacobian == "exact":
            if not hasattr(engine, "exact_stacked"):
                raise ValueError("this engine has no exact-Jacobian mode")
            engine.jacobian_mode = "exact"
        lb = np.array([-np.inf if b[0] is None else b[0] for b in self.bounds], dtype=float)
        ub = np.array([np.inf if b[1] is None else b[1] for b in self.bounds], dtype=float)

        def value_of(which):
            def fun(p, prob, obj_):
                self.p = p
                return engine.values(p)[which]
            return fun

        def jacobian_of(which):
            def jac(p, prob, obj_):
                blocks, h = engine.jacobians(p, lb, ub)
                # quirk Q13: the reference leaves prob.p at the last FD column's input
                last = np.array(p, dtype=float, copy=True)
                last[-1] += h[-1]
                self.p = last
                return blocks[which]
            return jac

        cons = ({"type": "eq", "fun": value_of(1), "jac": jacobian_of(1), "args": (self, obj)},
                {"type": "ineq", "fun": value_of(2), "jac": jacobian_of(2), "args": (self, obj)})
        if self.cost_derivative is None:
            cost_jac = jacobian_of(0)
        else:
            def cost_jac(p, prob, obj_):
                self.p = p
                return self.cost_derivative(self, obj)

        ftol = options.setdefault("ftol", 1e-6)
        maxiter = options.setdefault("maxiter", 25)
        if core == "hip":
            from . import sqp as _sqp
            user_gradient = None
            if self.cost_derivative is not None:
                def user_gradient(p):
                    self.p = p
                    return self.cost_derivative(self, obj)
        while self.iterator < self.maxIterator:
            print("---- iteration : {0} ----".format(self.iterator + 1))
            if core == "hip":
                # same major iteration, QP subproblem and BFGS factor on the GPU (sqp.py)
                opt = _sqp.minimize_slsqp_hip(engine, self.p, lb, ub, ftol=ftol, maxiter=maxiter,
                                              cost_derivative=user_gradient, disp=True)
                self.p = opt.last_callback_p
                self.sqp_timing = opt.timing
                self.sqp_timings = getattr(self, "sqp_timings", []) + [opt.timing]
            else:
                opt = _sciopt.minimize(value_of(0), self.p, args=(self, obj), bounds=self.bounds,
                                       constraints=cons, jac=cost_jac, method="SLSQP",
                                       options={"disp": True, "maxiter": maxiter, "ftol": ftol})
            self.last_result = opt
            print(opt.message)
            display_func()
            print("")
            if not opt.status:
                break
            self.iterator += 1

    def directional_derivative(self, obj, directions, p=None):
        """``F'(p) v`` of ``F = [cost | c_eq | c_ineq]`` at the decision vector ``p`` (default ``prob.p``) and the current
        parameter values, EXACT and without forming the Jacobian: one forward-mode pass of the traced callbacks per
        direction, the seed ``v_i`` on variable ``i`` (``HipEngine.directional``: an evaluation and one small launch for
        all ``K`` directions).  ``directions``: ``[K, number_of_variables]`` -> ``[K, m]``, or one vector -> ``[m]``.
        What it serves: checking a problem's derivatives (compare with ``J v``), the exact slope of a merit function
        along a search direction, the first-order effect of ``K`` dispersion directions on the constraints, the term
        ``F'(x) dx/dtheta`` of a continuation's tangent residual, any matrix-free method.  A direction in PARAMETER space
        needs no call of its own: by linearity it is ``sum_k w_k dF/dtheta_k`` of :meth:`parameter_sensitivity`.  An
        engine without ``directional`` and a direction of the wrong length are ``ValueError``s."""
        V = np.asarray(directions, dtype=float)
        single = V.ndim == 1
        if single:
            V = V[None, :]
        if V.ndim != 2 or V.shape[1] != self.number_of_variables or V.shape[0] < 1:
            raise ValueError("directions must have %d entries (number_of_variables) each, got shape %s" % (
                self.number_of_variables, np.shape(directions)))
        engine = self._batch_engine(obj)
        if not hasattr(engine, "directional"):
            raise ValueError("this engine has no exact directional derivative (it has no directional)")
        point = np.asarray(self.p if p is None else p, dtype=float).reshape(-1)
        dF = np.array(engine.directional(point, np.ascontiguousarray(V))[0], dtype=float, copy=True)
        return dF[0] if single else dF

    @staticmethod
    def _rows_of(engine, point):
        """m, the rows of ``F``: the engine's ``m``, or the length of its values at ``point``."""
        m = getattr(engine, "m", None)
        if m is None:
            m = sum(np.atleast_1d(np.asarray(v)).size for v in engine.values(point))
        return int(m)

    def adjoint_product(self, obj, weights, p=None):
        """``F'(p)^T w``, ``g_j = sum_r w_r dF_r/dx_j``, of ``F = [cost | c_eq | c_ineq]`` at the decision vector ``p``
        (default ``prob.p``) and the current parameter values, EXACT and without forming the Jacobian
        (``HipEngine.adjoint``: an evaluation and one launch for all ``K`` weight vectors; the column entries are computed
        once and shared by the vectors).  ``weights``: ``[K, m]`` over the rows of ``F`` -> ``[K, number_of_variables]``,
        or one vector -> ``[number_of_variables]``.  What it serves: ``w = e_0`` is the gradient of the cost,
        ``w = [1, lambda]`` the gradient of the Lagrangian (a KKT residual), ``w = [0, W c]`` the gradient of a penalty or
        feasibility merit ``1/2 c' W c``; with :meth:`directional_derivative` it is the pair ``J v`` / ``J^T w`` that LSQR
        or CG need, a least-squares multiplier estimate for instance.  The order of every sum is fixed, so the result is
        reproducible to the bit; run-time parameters are constants.  An engine without ``adjoint`` and a weight vector
        of the wrong length are ``ValueError``s."""
        W = np.asarray(weights, dtype=float)
        single = W.ndim == 1
        if single:
            W = W[None, :]
        if W.ndim != 2 or W.shape[0] < 1:
            raise ValueError("weights must have shape [K, m] or [m], got shape %s" % (np.shape(weights),))
        engine = self._batch_engine(obj)
        if not hasattr(engine, "adjoint"):
            raise ValueError("this engine has no exact adjoint product (it has no adjoint)")
        point = np.asarray(self.p if p is None else p, dtype=float).reshape(-1)
        m = self._rows_of(engine, point)
        if W.shape[1] != m:
            raise ValueError("weights must have %d entries (the rows of F) each, got shape %s" % (m, np.shape(weights)))
        G = np.array(engine.adjoint(point, np.ascontiguousarray(W))[0], dtype=float, copy=True)
        return G[0] if single else G

    def hessian_vector_product(self, obj, weights, directions, p=None):
        """``grad^2 (w . F)(p) v``, ``q_j = sum_r w_r d2F_r/dx_j dv``, of ``F = [cost | c_eq | c_ineq]`` at the decision
        vector ``p`` (default ``prob.p``) and the current parameter values, EXACT and without forming a Hessian
        (``HipEngine.hessian_vector``: an evaluation and one launch for all ``K`` pairs; second-order dual numbers, no
        step).  ``directions``: ``[K, number_of_variables]`` -> ``[K, number_of_variables]``, or one vector ->
        ``[number_of_variables]``.  ``weights``: ``[K, m]`` over the rows of ``F``, one vector per direction, or ONE
        ``[m]`` used for every direction - one ``lambda``, many ``v`` is the common call.  With ``w = [1, lambda]`` it is
        the Hessian of the Lagrangian times ``v``: the curvature ``v' H v`` along a step or a null-space direction, the
        product Newton-CG or Lanczos ask for, a check on what a quasi-Newton factor has learnt.  The order of every sum
        is fixed, so the result is reproducible to the bit; run-time parameters are constants.  An engine without
        ``hessian_vector`` and vectors of the wrong length are ``ValueError``s."""
        V = np.asarray(directions, dtype=float)
        single = V.ndim == 1
        if single:
            V = V[None, :]
        if V.ndim != 2 or V.shape[0] < 1 or V.shape[1] != self.number_of_variables:
            raise ValueError("directions must have shape [K, %d] or [%d] (number_of_variables), got shape %s" % (
                self.number_of_variables, self.number_of_variables, np.shape(directions)))
        W = np.asarray(weights, dtype=float)
        if W.ndim == 1:
            W = np.repeat(W[None, :], V.shape[0], axis=0)
        if W.ndim != 2 or W.shape[0] != V.shape[0]:
            raise ValueError("weights must have shape [%d, m] (one vector per direction) or [m], got shape %s" % (
                V.shape[0], np.shape(weights)))
        engine = self._batch_engine(obj)
        if not hasattr(engine, "hessian_vector"):
            raise ValueError("this engine has no exact Hessian-vector product (it has no hessian_vector)")
        point = np.asarray(self.p if p is None else p, dtype=float).reshape(-1)
        m = self._rows_of(engine, point)
        if W.shape[1] != m:
            raise ValueError("weights must have %d entries (the rows of F) each, got shape %s" % (m, np.shape(weights)))
        Q = np.array(engine.hessian_vector(point, np.ascontiguousarray(W), np.ascontiguousarray(V))[0], dtype=float,
                     copy=True)
        return Q[0] if single else Q

    def hessian_pattern(self, obj):
        """``(indptr, cols)``: the static lower-triangle pattern of the Hessian of ``w . F`` in CSR form - the partners
        ``l <= j`` of variable ``j`` at row ``j`` - from the traced callbacks (no GPU work).  Every pair outside it is an
        exact zero of the Hessian, whatever the weights and the point."""
        engine = self._batch_engine(obj)
        if not hasattr(engine, "hessian_pattern"):
            raise ValueError("this engine has no exact sparse Hessian (it has no hessian_pattern)")
        return engine.hessian_pattern()

    def hessian_matrix(self, obj, weights):
        """The Hessian ``sum_r w_r grad^2 F_r`` of ``F = [cost | c_eq | c_ineq]`` at ``prob.p`` and the current
        parameter values as a SPARSE matrix, EXACT (``HipEngine.hessian_matrix``: an evaluation and one launch that
        evaluates only the second derivatives that can be non-zero, once for up to 8 weight vectors; second-order dual
        numbers, no step).  ``weights``: ``[K, m]`` over the rows of ``F``, or one ``[m]``; with ``w = [1, lambda]`` it is
        the Hessian of the Lagrangian - a sparse-direct Newton or interior-point step, the (1, 1) block of the KKT
        matrix next to :meth:`adjoint_product` / :meth:`directional_derivative`, a reduced-Hessian check, the truth a
        quasi-Newton factor is compared with.  Returns a :class:`SparseHessian`: ``values`` (``[K, nnz]``, or ``[nnz]``
        for one vector) in the order of ``indptr`` / ``cols`` (the lower triangle in CSR form, :meth:`hessian_pattern`),
        ``tocsr(d=0, symmetric=True)`` and ``toarray(d=0)``.  Every stored entry is bit for bit
        :meth:`hessian_vector_product` with a unit direction; run-time parameters are constants.  An engine without
        ``hessian_matrix`` and a weight vector of the wrong length are ``ValueError``s."""
        W = np.asarray(weights, dtype=float)
        single = W.ndim == 1
        if single:
            W = W[None, :]
        if W.ndim != 2 or W.shape[0] < 1:
            raise ValueError("weights must have shape [K, m] or [m], got shape %s" % (np.shape(weights),))
        engine = self._batch_engine(obj)
        if not hasattr(engine, "hessian_matrix") or not hasattr(engine, "hessian_pattern"):
            raise ValueError("this engine has no exact sparse Hessian (it has no hessian_matrix / hessian_pattern)")
        point = np.asarray(self.p, dtype=float).reshape(-1)
        m = self._rows_of(engine, point)
        if W.shape[1] != m:
            raise ValueError("weights must have %d entries (the rows of F) each, got shape %s" % (m, np.shape(weights)))
        H = np.array(engine.hessian_matrix(point, np.ascontiguousarray(W))[0], dtype=float, copy=True)
        indptr, cols = engine.hessian_pattern()
        return SparseHessian(H[0] if single else H, indptr, cols)

    def adjoint_parameter_sensitivity(self, obj, weights, p=None):
        """``d(F'(p)^T w)/dtheta``, ``s_{k,j} = sum_r w_r d2F_r/dx_j dtheta_k``, of ``F = [cost | c_eq | c_ineq]`` for every
        declared run-time parameter at the decision vector ``p`` (default ``prob.p``) and the current parameter values,
        EXACT (``HipEngine.adjoint_parameter``: an evaluation and one launch for all ``K`` weight vectors and all
        parameters; second-order dual numbers with the second seed on the parameter, no step in ``theta`` and no
        ``set_parameters`` launch).  ``weights``: ``[K, m]`` over the rows of ``F`` -> ``[K, n_par, number_of_variables]``,
        or one vector -> ``[n_par, number_of_variables]``.  With ``w = [1, lambda]`` it is ``d(grad_x L)/dtheta``: the
        block of the linearised KKT system next to :meth:`hessian_vector_product`, :meth:`directional_derivative` /
        :meth:`adjoint_product` and :meth:`parameter_sensitivity`, the right-hand side of a continuation tangent.  The
        order of every sum is :meth:`adjoint_product`'s, so the result is reproducible to the bit; a parameter nothing
        reads gets a row of ``+0.0``.  A problem that declares no parameter, an engine without ``adjoint_parameter``
        and a weight vector of the wrong length are ``ValueError``s."""
        W = np.asarray(weights, dtype=float)
        single = W.ndim == 1
        if single:
            W = W[None, :]
        if W.ndim != 2 or W.shape[0] < 1:
            raise ValueError("weights must have shape [K, m] or [m], got shape %s" % (np.shape(weights),))
        if not self._par_names:
            raise ValueError("this problem declares no parameter")
        engine = self._batch_engine(obj)
        if not hasattr(engine, "adjoint_parameter"):
            raise ValueError("this engine has no exact mixed derivative (it has no adjoint_parameter)")
        point = np.asarray(self.p if p is None else p, dtype=float).reshape(-1)
        m = self._rows_of(engine, point)
        if W.shape[1] != m:
            raise ValueError("weights must have %d entries (the rows of F) each, got shape %s" % (m, np.shape(weights)))
        S = np.array(engine.adjoint_parameter(point, np.ascontiguousarray(W))[0], dtype=float, copy=True)
        return S[0] if single else S

    def parameter_hessian(self, obj, weights, p=None):
        """``S_kl = sum_r w_r d2F_r/dtheta_k dtheta_l``, the second derivatives of ``w . F`` in the declared run-time
        parameters, ``F = [cost | c_eq | c_ineq]``, at the decision vector ``p`` (default ``prob.p``) and the current
        parameter values, EXACT (``HipEngine.parameter_hessian``: an evaluation and one launch for all ``K`` weight
        vectors and all pairs; second-order dual numbers with one seed on each parameter of a pair, no step in ``theta``
        and no ``set_parameters`` launch).  ``weights``: ``[K, m]`` over the rows of ``F`` -> ``[K, n_par, n_par]``, or
        one vector -> ``[n_par, n_par]``.  With ``w = [1, lambda]`` it is ``d2L/dtheta2``: the block of the Hessian of
        the Lagrangian in ``(x, theta)`` next to :meth:`hessian_vector_product` / :meth:`hessian_matrix` (``xx``) and
        :meth:`adjoint_parameter_sensitivity` (``x theta``); with ``x`` held fixed the exact Hessian in ``theta``.  The
        order of every sum is :meth:`adjoint_product`'s, so the result is reproducible to the bit; it is symmetric by
        construction, and a parameter nothing reads gets a row and a column of ``+0.0``.  A problem that declares no
        parameter, an engine without ``parameter_hessian`` and a weight vector of the wrong length are ``ValueError``s."""
        W = np.asarray(weights, dtype=float)
        single = W.ndim == 1
        if single:
            W = W[None, :]
        if W.ndim != 2 or W.shape[0] < 1:
            raise ValueError("weights must have shape [K, m] or [m], got shape %s" % (np.shape(weights),))
        if not self._par_names:
            raise ValueError("this problem declares no parameter")
        engine = self._batch_engine(obj)
        if not hasattr(engine, "parameter_hessian"):
            raise ValueError("this engine has no exact parameter Hessian (it has no parameter_hessian)")
        point = np.asarray(self.p if p is None else p, dtype=float).reshape(-1)
        m = self._rows_of(engine, point)
        if W.shape[1] != m:
            raise ValueError("weights must have %d entries (the rows of F) each, got shape %s" % (m, np.shape(weights)))
        S = np.array(engine.parameter_hessian(point, np.ascontiguousarray(W))[0], dtype=float, copy=True)
        return S[0] if single else S

    # ------------------------------------------------------------------ many points at once
    def evaluate_batch(self, obj, points, jacobian=False, parameters=None, parameter_jacobian=False, directions=None,
                       adjoints=None, hessian_products=None, adjoint_parameter=None, hessians=None, parameter_hessians=None):
        """Cost, constraints and constraint violation of ``B`` decision vectors in one GPU launch - screening initial
        guesses before a solve, a dispersed family of trajectories around a solution, a parameter scan.  ``points`` has
        shape ``[B, number_of_variables]`` in the layout of ``Problem.p`` (scaled by the canonical units);
        ``jacobian=True`` (or ``"fd"``) adds the forward-difference Jacobians SLSQP would see at every point (SciPy's
        step rule with this problem's bounds); ``jacobian="exact"`` adds the exact ones instead - forward-mode
        derivatives of the traced callbacks, the ``jacobian="exact"`` of :meth:`solve`, without a step and its noise
        (``BatchResult.steps`` is then ``None``).  Any other string is a ``ValueError``; the environment's
        ``OG_JACOBIAN`` is not consulted here.  Returns a :class:`BatchResult`; every row of it is bit for bit what the
        single-point path (``engine.values`` / ``engine.jacobians`` / ``engine.exact_stacked``) gives.  The reference has
        no counterpart (one ``Problem``, one ``solve``): per point this replaces what ``solve`` replaces
        (``optimize.py:670-733``).  ``self.p`` is left alone.

        The engine of an earlier ``solve`` is reused when there is one.  A stand-in engine (``ENGINE_FACTORY``) without
        a ``batch`` method is served point by point through its ``values`` / ``jacobians`` (``exact_stacked`` for the
        exact Jacobians: an engine without one has no exact mode, a ``ValueError``).

        ``parameters`` gives every point values of the declared run-time parameters of its own (a dispersion in the
        vehicle, a scan of a constant): a ``[B, n_par]`` array in declaration order, or a dict from name to a scalar or a
        ``[B]`` array (names not given keep their current value).  ``None``: every point is evaluated at the current
        values.  ``points`` with ONE row is repeated for every row of ``parameters`` - a scan at one trajectory.  A
        stand-in engine is served point by point through its ``set_parameters`` (without one: ``ValueError``).
        ``BatchResult.parameters`` holds the values used.

        ``parameter_jacobian=True`` adds ``BatchResult.parameter_jacobian``, ``[B, n_par, m]``: the EXACT ``dF/dtheta`` of
        every point at its own row of ``parameters`` (``BatchSweep.parameter_jacobian``; a stand-in engine is served
        point by point through its ``parameter_jacobian``, without one: ``ValueError``).  It combines with any
        ``jacobian=``; a problem without parameters is a ``ValueError``.

        ``directions=V`` (``[B, number_of_variables]``, one row per row of ``points``) adds ``BatchResult.directional``,
        ``[B, m]``: the EXACT derivative ``F'(x_k) v_k`` of every point along its own direction, without a Jacobian
        (``BatchSweep.directional``; a stand-in engine is served point by point through its ``directional``, without one:
        ``ValueError``).  A point with its own row of ``parameters`` is differentiated at those values.  It combines with
        any ``jacobian=``; more directions at one point: repeat the point.  ``None``: nothing is computed and the call
        makes exactly the launches it makes without the keyword.

        ``adjoints=W`` (``[B, m]``, one weight vector over the rows of ``F`` per row of ``points``) adds
        ``BatchResult.adjoint``, ``[B, number_of_variables]``: the EXACT adjoint product ``F'(x_k)^T w_k`` of every point
        with its own vector, without a Jacobian (``BatchSweep.adjoint``; a stand-in engine is served point by point
        through its ``adjoint``, without one: ``ValueError``).  A point with its own row of ``parameters`` is
        differentiated at those values; one point scanned over ``parameters`` takes its one vector along.  It combines
        with every other keyword.  ``None``: nothing is computed and the call makes exactly the launches it makes
        without the keyword.

        ``hessian_products=(W, V)`` (``W`` ``[B, m]``, ``V`` ``[B, number_of_variables]``: one pair per row of ``points``)
        adds ``BatchResult.hessian_product``, ``[B, number_of_variables]``: the EXACT ``grad^2 (w_k . F)(x_k) v_k`` of
        every point with its own pair, without a Hessian (``BatchSweep.hessian_vector``; a stand-in engine is served
        point by point through its ``hessian_vector``, without one: ``ValueError``).  A point with its own row of
        ``parameters`` is differentiated at those values; one point scanned over ``parameters`` takes its one pair
        along.  It combines with every other keyword.  ``None``: nothing is computed and the call builds, loads and
        launches exactly what it does without the keyword.

        ``adjoint_parameter=W`` (``[B, m]``, one weight vector over the rows of ``F`` per row of ``points``) adds
        ``BatchResult.adjoint_parameter``, ``[B, n_par, number_of_variables]``: the EXACT ``d(F'(x_k)^T w_k)/dtheta`` of
        every point with its own vector, for every declared parameter (``BatchSweep.adjoint_parameter``; a stand-in
        engine is served point by point through its ``adjoint_parameter``, without one: ``ValueError``).  A point with
        its own row of ``parameters`` is differentiated at those values; one point scanned over ``parameters`` takes
        its one vector along.  It combines with every other keyword; a problem without parameters is a ``ValueError``.
        ``None``: nothing is computed and the call builds, loads and launches exactly what it does without the
        keyword.

        ``hessians=W`` (``[B, m]``, one weight vector over the rows of ``F`` per row of ``points``) adds
        ``BatchResult.hessian``, ``[B, nnz]``, and ``BatchResult.hessian_pattern``: the EXACT sparse Hessian of
        ``w_k . F`` at every point with its own vector, the stored entries of :meth:`hessian_pattern` in its order
        (``BatchSweep.hessian_matrix``; a stand-in engine is served point by point through its ``hessian_matrix`` and
        ``hessian_pattern``, without them: ``ValueError``).  A point with its own row of ``parameters`` is
        differentiated at those values; one point scanned over ``parameters`` takes its one vector along.  It combines
        with every other keyword.  ``None``: nothing is computed and the call builds, loads and launches exactly what it
        does without the keyword.

        ``parameter_hessians=W`` (``[B, m]``, one weight vector over the rows of ``F`` per row of ``points``) adds
        ``BatchResult.parameter_hessian``, ``[B, n_par, n_par]``: the EXACT second derivatives of ``w_k . F`` in the
        declared parameters at every point with its own vector (``BatchSweep.parameter_hessian``; a stand-in engine is
        served point by point through its ``parameter_hessian``, without one: ``ValueError``).  A point with its own
        row of ``parameters`` is differentiated at those values; one point scanned over ``parameters`` takes its one
        vector along.  It combines with every other keyword; a problem without parameters is a ``ValueError``.
        ``None``: nothing is computed and the call builds, loads and launches exactly what it does without the
        keyword."""
        if (parameter_jacobian or adjoint_parameter is not None or parameter_hessians is not None) and not self._par_names:
            raise ValueError("this problem declares no parameter")
        points = np.asarray(points, dtype=float)
        if directions is not None:
            directions = np.asarray(directions, dtype=float)
            if directions.ndim != 2 or directions.shape[1] != self.number_of_variables:
                raise ValueError("directions must have shape [B, %d] (number_of_variables), got %s" % (
                    self.number_of_variables, directions.shape))
            if points.ndim == 2 and directions.shape[0] != points.shape[0]:
                raise ValueError("directions holds %d rows for %d points" % (directions.shape[0], points.shape[0]))
        if adjoints is not None:
            adjoints = np.asarray(adjoints, dtype=float)
            if adjoints.ndim != 2:
                raise ValueError("adjoints must have shape [B, m] (the rows of F), got %s" % (adjoints.shape,))
            if points.ndim == 2 and adjoints.shape[0] != points.shape[0]:
                raise ValueError("adjoints holds %d rows for %d points" % (adjoints.shape[0], points.shape[0]))
        mix_w = None
        if adjoint_parameter is not None:
            mix_w = np.asarray(adjoint_parameter, dtype=float)
            if mix_w.ndim != 2:
                raise ValueError("adjoint_parameter must have shape [B, m] (the rows of F), got %s" % (mix_w.shape,))
            if points.ndim == 2 and mix_w.shape[0] != points.shape[0]:
                raise ValueError("adjoint_parameter holds %d rows for %d points" % (mix_w.shape[0], points.shape[0]))
        pp_w = None
        if parameter_hessians is not None:
            pp_w = np.asarray(parameter_hessians, dtype=float)
            if pp_w.ndim != 2:
                raise ValueError("parameter_hessians must have shape [B, m] (the rows of F), got %s" % (pp_w.shape,))
            if points.ndim == 2 and pp_w.shape[0] != points.shape[0]:
                raise ValueError("parameter_hessians holds %d rows for %d points" % (pp_w.shape[0], points.shape[0]))
        full_w = None
        if hessians is not None:
            full_w = np.asarray(hessians, dtype=float)
            if full_w.ndim != 2:
                raise ValueError("hessians must have shape [B, m] (the rows of F), got %s" % (full_w.shape,))
            if points.ndim == 2 and full_w.shape[0] != points.shape[0]:
                raise ValueError("hessians holds %d rows for %d points" % (full_w.shape[0], points.shape[0]))
        hess_w = hess_v = None
        if hessian_products is not None:
            if not isinstance(hessian_products, (tuple, list)) or len(hessian_products) != 2:
                raise ValueError("hessian_products must be a pair (W [B, m], V [B, number_of_variables])")
            hess_w, hess_v = (np.asarray(a, dtype=float) for a in hessian_products)
            if hess_w.ndim != 2 or hess_v.ndim != 2 or hess_v.shape[1] != self.number_of_variables:
                raise ValueError("hessian_products must have shapes [B, m] and [B, %d], got %s and %s" % (
                    self.number_of_variables, hess_w.shape, hess_v.shape))
            if hess_w.shape[0] != hess_v.shape[0] or (points.ndim == 2 and hess_v.shape[0] != points.shape[0]):
                raise ValueError("hessian_products holds %d and %d rows for %d points" % (
                    hess_w.shape[0], hess_v.shape[0], points.shape[0] if points.ndim == 2 else 1))
        assert points.ndim == 2, "points must have shape [B, number_of_variables], got %s" % (points.shape,)
        assert points.shape[1] == self.number_of_variables, \
            "points must have %d columns (number_of_variables), got %d" % (self.number_of_variables, points.shape[1])
        assert points.shape[0] >= 1, "points holds no point"
        assert len(self.dynamics) != 0, "It must be set dynamics"
        assert self.cost is not None, "It must be set cost function"
        assert self.equality is not None, "It must be set equality function"
        assert self.inequality is not None, "It must be set inequality function"
        if isinstance(jacobian, str):
            if jacobian not in ("fd", "exact"):
                raise ValueError("jacobian must be 'fd' or 'exact', got %r" % (jacobian,))
        else:
            jacobian = "fd" if jacobian else None
        TH = self._batch_parameters(parameters, points.shape[0])

        engine = self._batch_engine(obj)
        if TH is not None and TH.shape[0] != points.shape[0]:
            points = np.repeat(points, TH.shape[0], axis=0)          # one trajectory, scanned
            if directions is not None:
                directions = np.repeat(directions, TH.shape[0], axis=0)
            if adjoints is not None:
                adjoints = np.repeat(adjoints, TH.shape[0], axis=0)
            if hess_w is not None:
                hess_w, hess_v = np.repeat(hess_w, TH.shape[0], axis=0), np.repeat(hess_v, TH.shape[0], axis=0)
            if mix_w is not None:
                mix_w = np.repeat(mix_w, TH.shape[0], axis=0)
            if full_w is not None:
                full_w = np.repeat(full_w, TH.shape[0], axis=0)
            if pp_w is not None:
                pp_w = np.repeat(pp_w, TH.shape[0], axis=0)
        points = np.ascontiguousarray(points)
        if directions is not None:
            directions = np.ascontiguousarray(directions)
        B, n = points.shape
        if adjoints is not None:
            if not hasattr(engine, "adjoint"):
                raise ValueError("this engine has no exact adjoint product (it has no adjoint)")
            adjoints = np.ascontiguousarray(adjoints)
            m_rows = self._rows_of(engine, points[0])
            if adjoints.shape[1] != m_rows:
                raise ValueError("adjoints must have shape [B, %d] (the rows of F), got %s" % (m_rows, adjoints.shape))
        if hess_w is not None:
            if not hasattr(engine, "hessian_vector"):
                raise ValueError("this engine has no exact Hessian-vector product (it has no hessian_vector)")
            hess_w, hess_v = np.ascontiguousarray(hess_w), np.ascontiguousarray(hess_v)
            m_rows = self._rows_of(engine, points[0])
            if hess_w.shape[1] != m_rows:
                raise ValueError("hessian_products must have shapes [B, %d] and [B, %d], got %s and %s" % (
                    m_rows, n, hess_w.shape, hess_v.shape))
        if mix_w is not None:
            if not hasattr(engine, "adjoint_parameter"):
                raise ValueError("this engine has no exact mixed derivative (it has no adjoint_parameter)")
            mix_w = np.ascontiguousarray(mix_w)
            m_rows = self._rows_of(engine, points[0])
            if mix_w.shape[1] != m_rows:
                raise ValueError("adjoint_parameter must have shape [B, %d] (the rows of F), got %s" % (m_rows, mix_w.shape))
        if pp_w is not None:
            if not hasattr(engine, "parameter_hessian"):
                raise ValueError("this engine has no exact parameter Hessian (it has no parameter_hessian)")
            pp_w = np.ascontiguousarray(pp_w)
            m_rows = self._rows_of(engine, points[0])
            if pp_w.shape[1] != m_rows:
                raise ValueError("parameter_hessians must have shape [B, %d] (the rows of F), got %s" % (m_rows, pp_w.shape))
        if full_w is not None:
            if not hasattr(engine, "hessian_matrix") or not hasattr(engine, "hessian_pattern"):
                raise ValueError("this engine has no exact sparse Hessian (it has no hessian_matrix / hessian_pattern)")
            full_w = np.ascontiguousarray(full_w)
            m_rows = self._rows_of(engine, points[0])
            if full_w.shape[1] != m_rows:
                raise ValueError("hessians must have shape [B, %d] (the rows of F), got %s" % (m_rows, full_w.shape))
        used = TH if TH is not None else np.tile(np.asarray(self._par_values, dtype=float), (B, 1))
        lb = np.array([-np.inf if b[0] is None else b[0] for b in self.bounds], dtype=float)
        ub = np.array([np.inf if b[1] is None else b[1] for b in self.bounds], dtype=float)
        if jacobian == "exact" and not hasattr(engine, "exact_stacked"):
            raise ValueError("this engine has no exact-Jacobian mode")

        if not hasattr(engine, "batch"):
            if TH is not None and not hasattr(engine, "set_parameters"):
                raise ValueError("this engine cannot change parameters (it has no set_parameters)")
            if parameter_jacobian and not hasattr(engine, "parameter_jacobian"):
                raise ValueError("this engine has no exact parameter Jacobian (it has no parameter_jacobian)")
            if directions is not None and not hasattr(engine, "directional"):
                raise ValueError("this engine has no exact directional derivative (it has no directional)")

            def lanes():
                for k, p in enumerate(points):
                    if TH is not None:
                        engine.set_parameters(TH[k])
                    yield p
            saved = self.p
            par_jac = along = back = curv = mixed = full = second = None
            try:
                if full_w is not None:
                    full = np.stack([np.array(engine.hessian_matrix(p, full_w[k:k + 1])[0], dtype=float).reshape(-1)
                                     for k, p in enumerate(lanes())])
                if parameter_jacobian:
                    par_jac = np.stack([np.array(engine.parameter_jacobian(p)[0], dtype=float, copy=True) for p in lanes()])
                if directions is not None:
                    along = np.stack([np.array(engine.directional(p, directions[k:k + 1])[0], dtype=float).reshape(-1)
                                      for k, p in enumerate(lanes())])
                if adjoints is not None:
                    back = np.stack([np.array(engine.adjoint(p, adjoints[k:k + 1])[0], dtype=float).reshape(-1)
                                     for k, p in enumerate(lanes())])
                if hess_w is not None:
                    curv = np.stack([np.array(engine.hessian_vector(p, hess_w[k:k + 1], hess_v[k:k + 1])[0],
                                              dtype=float).reshape(-1) for k, p in enumerate(lanes())])
                if mix_w is not None:
                    mixed = np.stack([np.array(engine.adjoint_parameter(p, mix_w[k:k + 1])[0], dtype=float)[0]
                                      for k, p in enumerate(lanes())])
                if pp_w is not None:
                    second = np.stack([np.array(engine.parameter_hessian(p, pp_w[k:k + 1])[0], dtype=float)[0]
                                       for k, p in enumerate(lanes())])
                if not jacobian:
                    rows = [np.concatenate([np.atleast_1d(np.asarray(v, dtype=float)) for v in engine.values(p)])
                            for p in lanes()]
                    # (m_eq from the LAST point: the engine is at the last lane's parameters now, its cached values serve)
                    res = BatchResult(np.stack(rows), int(np.atleast_1d(engine.values(points[-1])[1]).size))
                    res.parameters, res.parameter_jacobian, res.directional, res.adjoint = used, par_jac, along, back
                    res.hessian_product, res.adjoint_parameter, res.parameter_hessian = curv, mixed, second
                    if full is not None:
                        res.hessian, res.hessian_pattern = full, engine.hessian_pattern()
                    return res
                rows, dense, steps = [], [], []
                if jacobian == "exact":
                    for p in lanes():
                        F0, JT = engine.exact_stacked(p)
                        rows.append(np.array(F0, dtype=float, copy=True))
                        dense.append(np.array(JT, dtype=float, copy=True))
                    m_eq = int(np.atleast_1d(engine.values(points[-1])[1]).size)
                else:
                    for p in lanes():
                        (grad, jeq, jineq), h = engine.jacobians(p, lb, ub)
                        rows.append(np.concatenate([np.atleast_1d(np.asarray(v, dtype=float)) for v in engine.values(p)]))
                        dense.append(np.vstack([np.atleast_2d(grad), np.atleast_2d(jeq), np.atleast_2d(jineq)]).T.copy())
                        steps.append(np.array(h, dtype=float, copy=True))
                    m_eq = int(np.atleast_2d(jeq).shape[0])
            finally:
                self.p = saved
                if TH is not None:
                    engine.set_parameters(list(self._par_values))      # (the engine goes back to the current values)
            res = BatchResult(np.stack(rows), m_eq)
            res.parameters, res.parameter_jacobian, res.directional, res.adjoint = used, par_jac, along, back
            res.hessian_product, res.adjoint_parameter, res.parameter_hessian = curv, mixed, second
            if full is not None:
                res.hessian, res.hessian_pattern = full, engine.hessian_pattern()
            m = rows[0].size
            # a stand-in knows no pattern: every entry of the dense matrix is one
            res.pattern = (np.arange(n + 1, dtype=np.int64) * m, np.tile(np.arange(m, dtype=np.int32), n))
            res.values = np.stack([d.reshape(-1) for d in dense])
            res.gradient = np.stack([d[:, 0] for d in dense])
            res.steps = np.stack(steps) if jacobian == "fd" else None
            res.jacobian = jacobian
            return res

        batch = getattr(self, "_batch", None)
        if batch is None or batch.engine is not engine or batch.capacity < B or not batch._handle.value:
            if batch is not None:
                batch.close()
            batch = self._batch = engine.batch(B)
        if getattr(engine, "n_par", 0):
            # (None binds the handle's values to every lane: per-lane values of an earlier call do not leak into this one)
            batch.set_parameters(TH)
        par_jac = None
        if parameter_jacobian:
            if not hasattr(batch, "parameter_jacobian"):
                raise ValueError("this engine has no exact parameter Jacobian (its batch has no parameter_jacobian)")
            par_jac = batch.parameter_jacobian(points)[0]
        along = None
        if directions is not None:
            if not hasattr(batch, "directional"):
                raise ValueError("this engine has no exact directional derivative (its batch has no directional)")
            along = batch.directional(points, directions)[0]
        back = None
        if adjoints is not None:
            if not hasattr(batch, "adjoint"):
                raise ValueError("this engine has no exact adjoint product (its batch has no adjoint)")
            back = batch.adjoint(points, adjoints)[0]
        curv = None
        if hess_w is not None:
            if not hasattr(batch, "hessian_vector"):
                raise ValueError("this engine has no exact Hessian-vector product (its batch has no hessian_vector)")
            curv = batch.hessian_vector(points, hess_w, hess_v)[0]
        mixed = None
        if mix_w is not None:
            if not hasattr(batch, "adjoint_parameter"):
                raise ValueError("this engine has no exact mixed derivative (its batch has no adjoint_parameter)")
            mixed = batch.adjoint_parameter(points, mix_w)[0]
        second = None
        if pp_w is not None:
            if not hasattr(batch, "parameter_hessian"):
                raise ValueError("this engine has no exact parameter Hessian (its batch has no parameter_hessian)")
            second = batch.parameter_hessian(points, pp_w)[0]
        full = full_pattern = None
        if full_w is not None:
            if not hasattr(batch, "hessian_matrix"):
                raise ValueError("this engine has no exact sparse Hessian (its batch has no hessian_matrix)")
            full, full_pattern = batch.hessian_matrix(points, full_w)[0], engine.hessian_pattern()
        if not jacobian:
            res = BatchResult(batch.values(points), engine.m_eq)
            res.parameters, res.parameter_jacobian, res.directional, res.adjoint = used, par_jac, along, back
            res.hessian_product, res.adjoint_parameter, res.parameter_hessian = curv, mixed, second
            res.hessian, res.hessian_pattern = full, full_pattern
            return res
        if jacobian == "exact":
            F0, vals, nonfinite = batch.exact(points)
            H = None
        else:
            F0, vals, nonfinite, H = batch.jacobians(points, lb, ub)
        res = BatchResult(F0, engine.m_eq)
        res.parameters, res.parameter_jacobian, res.directional, res.adjoint = used, par_jac, along, back
        res.hessian_product, res.adjoint_parameter, res.parameter_hessian = curv, mixed, second
        res.hessian, res.hessian_pattern = full, full_pattern
        indptr, rows = batch.pattern
        res.pattern, res.values, res.steps, res.jacobian = (indptr, rows), vals, H, jacobian
        # column 0 of J_T: the pattern entries whose row is the cost
        res.gradient = np.zeros((B, n))
        at = np.flatnonzero(rows == 0)
        res.gradient[:, np.searchsorted(indptr, at, side="right") - 1] = vals[:, at]
        # (FD: NaN rows fill every column, which the packed form cannot say; the exact kernel writes pattern entries only)
        for k in np.flatnonzero(nonfinite) if jacobian == "fd" else ():
            res.gradient[k] = batch.dense(k)[:, 0]
        return res

    # ------------------------------------------------------------------ reporting
    def __repr__(self):
        rows = ["---- parameter ----",
                "nodes = %s" % (self.nodes,),
                "number of states    = %s" % (self.number_of_states,),
                "number of controls  = %s" % (self.number_of_controls,),
                "number of sections  = %s" % (self.number_of_section,),
                "number of variables = %s" % (self.number_of_variables,),
                "---- algorithm ----",
                "max iteration = %s" % (self.maxIterator,),
                "---- function  ----",
                "dynamics        = %s" % (self.dynamics,),
                "cost            = %s" % (self.cost,),
                "cost_derivative = %s" % (self.cost_derivative,),
                "equality        = %s" % (self.equality,),
                "inequality      = %s" % (self.inequality,),
                "knot_states_smooth = %s" % (self.dynamics,)]
        return "\n".join(rows) + "\n"

    def to_csv(self, filename="OpenGoddard_output.csv", delimiter=","):
        """Time, states and controls (phase-0 counts) as CSV columns (``optimize.py:844-863``)."""
        cols, names = [self.time_update()], ["time"]
        for i in range(self.number_of_states[0]):
            cols.append(self.states_all_section(i))
            names.append("state%d" % i)
        for i in range(self.number_of_controls[0]):
            cols.append(self.controls_all_section(i))
            names.append("control%d" % i)
        header = "".join(n + ", " for n in names)
        np.savetxt(filename, np.vstack(cols).T, delimiter=delimiter, header=header)
        print("Completed saving \"%s\"" % (filename))

    def plot(self, title_comment=""):
        """Scatter of the raw decision vector with slice boundaries (``optimize.py:865-880``)."""
        import matplotlib.pyplot as plt
        plt.figure()
        plt.title("OpenGoddard inner variables" + title_comment)
        plt.plot(self.p, "o")
        plt.xlabel("variables")
        plt.ylabel("value")
        for i in range(self.number_of_section):
            for edge in self.div[i]:
                plt.axvline(edge, color="C%d" % ((i + 1) % 6), alpha=0.5)
        plt.grid()


class Guess:
    """Initial-guess generators on a time grid (``optimize.py:883-975``)."""

    @classmethod
    def zeros(cls, time):
        return np.zeros(len(time))

    @classmethod
    def constant(cls, time, const):
        return np.ones(len(time)) * const

    @classmethod
    def linear(cls, time, y0, yf):
        """Straight line through ``(time[0], y0)`` and ``(time[-1], yf)``.  Same arithmetic as
        the two-point ``scipy.interpolate.interp1d`` the reference builds (``optimize.py:928-931``):
        ``slope * (t - t_first) + y0``."""
        time = np.asarray(time, dtype=float)
        slope = (np.float64(yf) - np.float64(y0)) / (time[-1] - time[0])
        return slope * (time - time[0]) + np.float64(y0)

    @classmethod
    def cubic(cls, time, y0, yprime0, yf, yprimef):
        """Cubic Hermite profile from end values and end slopes (``optimize.py:933-956``): the
        4x4 collocation system is inverted with ``np.linalg.inv`` like the reference."""
        ta, tb = time[0], time[-1]
        rows = []
        for t in (ta, tb):
            rows.append([1, t, t ** 2, t ** 3])
            rows.append([0, 1, 2 * t, 3 * t ** 2])
        coef = np.linalg.inv(np.array(rows)).dot(np.array([y0, yprime0, yf, yprimef]))
        return coef[0] + coef[1] * time + coef[2] * time ** 2 + coef[3] * time ** 3

    @classmethod
    def plot(cls, x, y, title="", xlabel="", ylabel=""):
        import matplotlib.pyplot as plt
        plt.figure()
        plt.plot(x, y, "-o")
        plt.title(title)
        plt.xlabel(xlabel)
        plt.ylabel(ylabel)
        plt.grid()


class Condition(object):
    """Growable constraint-row vector (``optimize.py:978-1072``).  ``equal(a, b)`` appends
    ``(a-b)/unit``; ``lower_bound(a, b)`` appends ``(a-b)/unit`` (feasible when >= 0);
    ``upper_bound(a, b)`` appends ``(b-a)/unit``."""

    def __init__(self, length=0):
        self._condition = np.zeros(length)

    def add(self, arg, unit=1.0):
        self._condition = _tr.cat([self._condition, arg / unit])

    def equal(self, arg1, arg2, unit=1.0):
        self.add(arg1 - arg2, unit)

    def lower_bound(self, arg1, arg2, unit=1.0):
        self.add(arg1 - arg2, unit)

    def upper_bound(self, arg1, arg2, unit=1.0):
        self.add(arg2 - arg1, unit)

    def change_value(self, index, value):
        self._condition[index] = value

    def __call__(self):
        return self._condition


class Dynamics(object):
    """Per-state right-hand-side holder for one phase (``optimize.py:1075-1127``).  Calling it
    stacks the states' time derivatives scaled by ``unit_time / unit_state``; states that were
    never assigned contribute zeros."""

    def __init__(self, prob, section=0):
        self.section = section
        self.number_of_state = prob.number_of_states[section]
        self.unit_states = prob.unit_states
        self.unit_time = prob.unit_time
        self._rhs = {i: np.zeros(prob.nodes[section]) for i in range(self.number_of_state)}

    def __getitem__(self, key):
        assert key < self.number_of_state, "Error, Dynamics key out of range"
        return self._rhs[key]

    def __setitem__(self, key, value):
        assert key < self.number_of_state, "Error, Dynamics key out of range"
        self._rhs[key] = value

    def __call__(self):
        units = self.unit_states[self.section]
        return _tr.cat([self._rhs[i] * (self.unit_time / units[i])
                        for i in range(self.number_of_state)])
