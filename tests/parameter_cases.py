"""The problems of tests/test_parameters.py and tests/test_parameters_gpu.py (and of ``__graft_entry__.build``, which
compiles their modules ahead of the GPU run): the smallest shapes that reach every place a run-time parameter can be
read.

P2: 2 phases, nodes [5, 4], 2 states and 1 control each, smooth knot, n = 29.  ``a`` multiplies the control inside the
dynamics of both phases (the defect tails, ``tail_one``); ``b`` is the right-hand side of a boundary equality (a row
item); ``c`` is an upper bound on the control (an inequality row per node); ``d`` weighs the running cost ``d * u**2``
(``sum_term``, the cached sequential sum); ``e`` is declared and never read.

G17 / G9: ``problems.build("goddard", nodes=[17] / [9])`` with ``T_max``, ``Hc``, ``c`` and ``Mf`` replaced by
parameters of the same values.  17 nodes: a second 16-node tile that holds one node.  Every use of them is + - * / or
unary minus ahead of the ``exp``, so the parameterised module and the module with the same numbers baked in agree bit
for bit.
"""
import warnings

import numpy as np

from opengoddard_amd import optimize as api
from opengoddard_amd import problems

P2_NAMES = ("a", "b", "c", "d", "e")
P2_THETA = (np.array([1.5, 0.7, 2.0, 0.3, 9.0]),
            np.array([0.8, -0.4, 1.25, 1.75, -3.0]),
            np.array([-2.5, 0.0, 0.5, 0.0625, 0.0]))
G_NAMES = ("T_max", "Hc", "c", "Mf")
G_THETA = (np.array([3.5, 500.0, 0.5, 0.6]),
           np.array([3.6, 480.0, 0.55, 0.58]),
           np.array([2.9, 510.0, 0.45, 0.63]))


class Model:
    pass


def _p2_callbacks():
    def dynamics(prob, obj, section):
        x0, x1 = prob.states(0, section), prob.states(1, section)
        u = prob.controls(0, section)
        rhs = api.Dynamics(prob, section)
        rhs[0] = x1
        rhs[1] = obj.a * u - x0
        return rhs()

    def equality(prob, obj):
        x0, x1 = prob.states_all_section(0), prob.states_all_section(1)
        rows = api.Condition()
        rows.equal(x0[0], 0.0)
        rows.equal(x1[-1], obj.b)
        return rows()

    def inequality(prob, obj):
        u = prob.controls_all_section(0)
        rows = api.Condition()
        rows.upper_bound(u, obj.c)
        rows.lower_bound(prob.time_final(-1), 0.5)
        return rows()

    def cost(prob, obj):
        return -prob.states_all_section(0)[-1]

    def running_cost(prob, obj):
        u = prob.controls_all_section(0)
        return obj.d * u ** 2

    return dynamics, equality, inequality, cost, running_cost


def p2(theta=None, baked=False):
    """-> ``(prob, obj)``; ``baked``: the same problem with plain floats in place of the parameters."""
    theta = P2_THETA[0] if theta is None else np.asarray(theta, dtype=float)
    prob = api.Problem([0.0, 1.0, 2.0], [5, 4], [2, 2], [1, 1], 5)
    obj = Model()
    for name, value in zip(P2_NAMES, theta):
        setattr(obj, name, float(value) if baked else prob.parameter(name, value))
    for sec in range(2):
        t = prob.time[sec]
        prob.set_states(0, sec, 0.5 * t + 0.1 * np.sin(3.0 * t))
        prob.set_states(1, sec, 0.5 + 0.25 * np.cos(2.0 * t))
        prob.set_controls(0, sec, 1.0 - 0.3 * t + 0.2 * np.sin(5.0 * t))
    dynamics, equality, inequality, cost, running_cost = _p2_callbacks()
    prob.dynamics = [dynamics, dynamics]
    prob.cost, prob.running_cost = cost, running_cost
    prob.equality, prob.inequality = equality, inequality
    return prob, obj


def goddard(nodes, theta=None, baked=False):
    theta = G_THETA[0] if theta is None else np.asarray(theta, dtype=float)
    prob, obj = problems.build("goddard", nodes=[int(nodes)])
    for name, value in zip(G_NAMES, theta):
        setattr(obj, name, float(value) if baked else prob.parameter(name, value))
    return prob, obj


def trace(prob, obj):
    """``codegen.trace_problem`` without P2's warning about ``e`` (one test asks for that warning by name)."""
    from opengoddard_amd import codegen
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        return codegen.trace_problem(prob, obj)


def point(prob, seed=0):
    """A decision vector inside the bounds, a little away from the guess."""
    rng = np.random.default_rng(seed)
    lb = np.array([-np.inf if b[0] is None else b[0] for b in prob.bounds])
    ub = np.array([np.inf if b[1] is None else b[1] for b in prob.bounds])
    return np.clip(prob.p * (1.0 + 0.01 * rng.standard_normal(prob.p.size)), lb, ub)


# what __graft_entry__.build compiles: (label, factory, batched?)
def modules():
    return [("parameters P2", lambda: p2(), True),
            ("parameters G17", lambda: goddard(17), True),
            ("parameters G9", lambda: goddard(9), True),
            ("parameters G17 baked", lambda: goddard(17, G_THETA[1], baked=True), False),
            ("parameters G9 baked", lambda: _g9_at_3_6(), False)]


def _g9_at_3_6():
    theta = G_THETA[0].copy()
    theta[0] = 3.6
    return goddard(9, theta, baked=True)
