"""The cases of tests/test_nonlocal.py and tests/test_nonlocal_gpu.py (and of ``__graft_entry__.build``, which compiles
their modules ahead of the GPU run): dynamics whose right-hand side reads a state ACROSS the nodes of a phase - it
normalises by, or relaxes towards, the state's mean, its sum of squares, its first or its last value.

A collocation slot carries a two-bit ``reads`` word (``OGT_SLOT.v[6]``, from ``SweepPlan.mv_diag`` and ``mv_generic``): bit
0 - the slot's dynamics term at node k reads the state at node k; bit 1 - the term reads the state's own slice in some
other way.  With bit 1 every entry ``(k, l)`` of the state's own N x N block is ``D[k][l] d(op_l)`` minus a derivative of
the dynamics term, not only the diagonal.  No other problem of the suite sets bit 1 on a slot whose term really reads the
slice (``wide_reductions`` has the bit on a slot whose own term is node-local); these do:

=========  =========  ==================================  ===============================================  ============
key        nodes      dx[0]                               dx[1]                                            reads (x, v)
=========  =========  ==================================  ===============================================  ============
``NL3``    [21, 6]    ``v - 0.3 * (x - x.mean())``        ``u - 0.2 * v``                                  3, 1
``NL2``    [21, 6]    ``v - 0.05 * np.sum(x * x)``        ``u - 0.2 * v``                                  2, 1
``NL0``    [21, 6]    ``v * np.cos(x - x[0])``            ``u - 0.2 * v / (1 + x[-1] ** 2) - 0.1 * v[0]``  3, 3
``NLX``    [21, 6]    ``v - 0.1 * v.mean() * x``          ``u - 0.2 * v - 0.05 * (x * x).sum()``           3, 3
                                                          ``+ 0.1 * u[0] * u``
``NLS``    [21, 6]    ``v - 0.01 * sum(x * x)``           ``u - 0.2 * v * sum(u)``   (Python's ``sum``)    2, 1
``NL130``  [130, 5]   as ``NL3``                          as ``NL3``                                       3, 1
``NL100``  [100, 5]   as ``NL3``                          as ``NL3``                                       3, 1
``NLP``    [21, 6]    ``v - a * (x - x.mean())``          ``u - b * v * x[0]``                             3, 1
=========  =========  ==================================  ===============================================  ============

(``a``, ``b`` of ``NLP`` are run-time parameters at 0.3 and 0.2; a second set, 0.45 and 0.1, is for the mixed
derivatives.  Its second row reads ``v`` node by node and ``x[0]``, another state's slice: bit 1 of ``v`` stays clear.)

``mv_generic`` is taken from the dependencies of the whole group, so ``NLX`` has bit 1 on both slots although neither
right-hand side reads its OWN state across the nodes (``v.mean()`` stands in the row of ``x``, ``(x * x).sum()`` in the row
of ``v``): its own blocks are ``D`` off the diagonal, the generic branch recomputes terms that are zero there, and what it
adds to the suite is a phase whose 44 state columns are all heavy.  ``CROSS_ONLY`` names it; every other case bites.

21 nodes fill two node tiles, the second with 5 rows, and N is no multiple of 4; 6 nodes fill one partly filled tile.  130 nodes are nine column tiles and a tile workgroup holds at most seven, so a node tile's columns are split
over two tile workgroups of five and four (``OGT_FTILE.y > 0`` in the second).  A workgroup of five column tiles still
has a free wavefront for the diagonal term; one of six or seven has none (``diag_wave < 0`` in ``fz_tile_body``), and 100
nodes - seven column tiles in one workgroup - are the smallest shape of this family with such a workgroup.
tests/test_nonlocal.py asserts these facts from the emitted records.

Structure of every problem: two phases, two states ``x, v``, one control ``u``, times ``[0, 1, 2.5]``, no units, a knot that
is not smooth; ``x(0) = 0.1``, ``v(0) = 0``, ``x_1[0] = x_0[-1]``; ``x >= -3`` at every node; the final time as the cost.
"""
import re

import numpy as np

import directional_cases as dc
import parameter_cases as pc
from opengoddard_amd import codegen
from opengoddard_amd.optimize import Condition, Dynamics, Problem

# key -> (nodes, right-hand side)
SHAPES = {
    "NL3": ([21, 6], "mean"),
    "NL2": ([21, 6], "sum"),
    "NL0": ([21, 6], "first"),
    "NLX": ([21, 6], "cross"),
    "NLS": ([21, 6], "pysum"),
    "NL130": ([130, 5], "mean"),
    "NL100": ([100, 5], "mean"),
    "NLP": ([21, 6], "parameters"),
}
KEYS = tuple(SHAPES)
# the `reads` words of the slots (x, v) - the same in both phases
READS = {"NL3": (3, 1), "NL2": (2, 1), "NL0": (3, 3), "NLX": (3, 3), "NLS": (2, 1), "NL130": (3, 1), "NL100": (3, 1),
         "NLP": (3, 1)}
EXACT_KEYS = ("NL3", "NL2", "NL0", "NL130", "NL100")      # og_jacobian_exact against the twin, both layouts
BATCH_KEYS = ("NL2", "NL0")                               # ... and the two batch kernels
DERIVATIVE_KEYS = ("NL2", "NL0")                          # the shapes the derivative kernels' case tables take from here
NLP_NAMES = ("a", "b")
NLP_THETA = (np.array([0.3, 0.2]), np.array([0.45, 0.1]))
CROSS_ONLY = ("NLX",)     # bit 1 without a term that reads the slot's own slice across the nodes (see above)
BITE = 1e-4             # what ignoring bit 1 must cost at the least: 1e8 times the bound of any comparison with a reference


class Obj:
    pass


def problem(key):
    """-> ``(prob, obj)`` of a key, at the first parameter set."""
    nodes, kind = SHAPES[key]
    prob = Problem([0.0, 1.0, 2.5], list(nodes), [2, 2], [1, 1], 3)
    obj = Obj()
    if kind == "parameters":
        obj.a, obj.b = (prob.parameter(name, value) for name, value in zip(NLP_NAMES, NLP_THETA[0]))

    def dynamics(prob, obj, section):
        x, v, u = prob.states(0, section), prob.states(1, section), prob.controls(0, section)
        dx = Dynamics(prob, section)
        if kind == "mean":
            dx[0] = v - 0.3 * (x - x.mean())
            dx[1] = u - 0.2 * v
        elif kind == "sum":
            dx[0] = v - 0.05 * np.sum(x * x)
            dx[1] = u - 0.2 * v
        elif kind == "first":
            dx[0] = v * np.cos(x - x[0])
            dx[1] = u - 0.2 * v / (1.0 + x[-1] ** 2) - 0.1 * v[0]
        elif kind == "cross":
            dx[0] = v - 0.1 * v.mean() * x
            dx[1] = u - 0.2 * v - 0.05 * (x * x).sum() + 0.1 * u[0] * u
        elif kind == "pysum":
            dx[0] = v - 0.01 * sum(x * x)
            dx[1] = u - 0.2 * v * sum(u)
        else:
            dx[0] = v - obj.a * (x - x.mean())
            dx[1] = u - obj.b * v * x[0]
        return dx()

    def equality(prob, obj):
        rows = Condition()
        rows.equal(prob.states(0, 0)[0], 0.1)
        rows.equal(prob.states(1, 0)[0], 0.0)
        rows.equal(prob.states(0, 1)[0], prob.states(0, 0)[-1])
        return rows()

    def inequality(prob, obj):
        rows = Condition()
        rows.lower_bound(prob.states_all_section(0), -3.0)
        return rows()

    prob.p[:-2] = np.random.default_rng(5).uniform(-1.0, 1.0, prob.number_of_variables - 2)
    prob.dynamics = [dynamics, dynamics]
    prob.knot_states_smooth = [False]
    prob.cost = lambda prob, obj: prob.time_final(-1)
    prob.running_cost = None
    prob.equality = equality
    prob.inequality = inequality
    return prob, obj


class NonLocal(dc.Case):
    """One case, traced once: program, header, three points (the guess and two seeded 2 % perturbations of it), and for
    ``NLP`` its two parameter sets."""

    def __init__(self, key):
        self.key = key
        self.prob, self.obj = problem(key)
        self.program = pc.trace(self.prob, self.obj)
        self.header = codegen.emit_header(self.program)
        self.n, self.m, self.n_par = self.program.n, self.program.m, self.program.n_par
        self.thetas = [None]
        self.names, self.unread = (), set()
        if key == "NLP":
            self.thetas, self.names = list(NLP_THETA), NLP_NAMES
        base = np.array(self.prob.p, dtype=float)
        rng = np.random.default_rng(17)
        self.points = [base] + [base * (1.0 + 0.02 * rng.standard_normal(base.size)) for _ in range(2)]

    def _cvec(self, theta):
        cv = np.array(self.program.cvec, dtype=np.float64)
        cv[self.program.par_off:] = theta
        return cv


_CASES = {}


def case(key):
    if key not in _CASES:
        _CASES[key] = NonLocal(key)
    return _CASES[key]


# ------------------------------------------------------------------------------------------------ what the tables say
def slots(C):
    """Per collocation slot: ``(phase, state, leaf, N, row0, reads)`` from the program and its ``SweepPlan``."""
    plan = codegen.SweepPlan(C.program)
    out = []
    for si, sl in enumerate(C.program.mv):
        g = C.program.groups[plan.slot_group[si]]
        out.append((sl.phase, si - g.mv_slots[0], sl.leaf_base, sl.length, plan.slot_row0[si],
                    plan.mv_diag[si] | (plan.mv_generic[si] << 1)))
    return out


def table(C, name):
    """The rows of an integer table of the emitted header, ``[[int, ...], ...]``."""
    body = re.search(r"%s\[\d+\] = \{(.*?)\n\};" % name, C.header, re.S).group(1)
    return [[int(v) for v in re.findall(r"-?\d+", row)] for row in re.findall(r"\{([^{}]*)\}", body)]


def diag_only(JT, C):
    """The matrix a kernel that ignored bit 1 would write, from the right ``J_T [n, m]``: inside the own block of every
    slot with bit 1, off the diagonal, the entry ``(k, l)`` is ``D[k][l] * d(op_l)`` alone - the dynamics term's part is
    gone.  (No units here, so the operand of node l is ``x_l`` itself and ``d(op_l) = 1``.)"""
    out = np.array(JT, dtype=float, copy=True)
    for phase, state, leaf, N, row0, reads in slots(C):
        if not reads & 2:
            continue
        assert C.prob.unit_states[phase][state] == 1.0
        D = np.asarray(C.prob.D[phase], dtype=float)
        off = ~np.eye(N, dtype=bool)
        block = out[leaf:leaf + N, row0:row0 + N]                 # [l, k] = d defect(k) / d x(l)
        block[off] = (D.T * 1.0)[off]
    return out


def bite(JT, C):
    """Per slot with bit 1: ``max |J - diag_only(J)|`` over its own block."""
    gap = np.abs(np.asarray(JT) - diag_only(JT, C))
    return {(phase, state): float(gap[leaf:leaf + N, row0:row0 + N].max())
            for phase, state, leaf, N, row0, reads in slots(C) if reads & 2}


def cuts(C):
    """Column blocks that cut a state's own slice off the 16-column grid: for the first slot of the longest phase
    ``(leaf + 3, leaf + 19)`` and ``(leaf + 16, leaf + N)``, then the last column alone, and - where the slice has a
    ninth column tile - a block that starts inside it."""
    phase, state, leaf, N, row0, reads = max(slots(C), key=lambda s: (s[3], -s[2]))
    out = [(leaf + 3, leaf + 19), (leaf + 16, leaf + N), (C.n - 1, C.n)]
    if N > 8 * 16 + 1:
        out.append((leaf + 8 * 16 + 1, leaf + N + 2))
    return out


# what __graft_entry__.build compiles for tests/test_nonlocal_gpu.py: (label, header, with the two batch parts)
def modules():
    return [("nonlocal " + key, case(key).header, key in BATCH_KEYS) for key in KEYS]
