"""The cases of tests/test_parameter_exact.py and tests/test_parameter_exact_gpu.py (and of ``__graft_entry__.build``,
which compiles their modules and parameter parts ahead of the GPU run): problems, parameter values, points, the
complex-step reference in theta and the host probe of ``csrc/og_par.h``.

P2, G9, G17: ``parameter_cases``.  P2 reaches every reader - ``a`` the defect tails of two phases, ``b`` a row item,
``c`` an inequality row per node, ``d`` the sequential sum, ``e`` nothing.

P2U: P2 whose second state's unit is a sixth parameter ``unit`` (``set_unit_states_all_section(1, unit)``: the getters
multiply by it, the collocation operand divides by it again) - the one way a callback-free piece of set-up puts a
parameter into ``mv_operand``: its defect rows get ``sum_l D[k][l] d(operand_l)``.

E: the shape of ``_expression_problem`` of tests/test_parameters.py on 4 nodes, with two parameters ``q`` and ``r``: ``q``
goes through every ``og_dual`` rule a callback can spell, twice through one expression, and together with ``r``.  Its
parameter values put ``q`` on either side of every switch and exactly on it: the ``where`` threshold (1.0), the tie of
``maximum`` (0.75), both edges of ``clip`` (0.5, 2.0), a table knot (1.5), the kink of ``abs`` (1.25).
"""
import os
import subprocess

import numpy as np
from scipy import interpolate

import parameter_cases as pc
from opengoddard_amd import codegen
from opengoddard_amd import optimize as api
from oracle import exact_jac

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "opengoddard_amd", "csrc")
PROBE_SOURCE = os.path.join(ROOT, "tests", "par_exact_probe.cpp")
PROBE_FLAGS = ["-O2", "-std=c++17", "-ffp-contract=off", "-mfma", "-Wno-unused-value", "-I", CSRC]
BOUND = 1e-12           # of the row's largest entry: tests/test_exact_surface.py's bound for the same comparison in x

E_NAMES = ("q", "r")
# q on the switches, then on either side of them; r on either side of q * x
E_THETA = tuple(np.array(v) for v in ((0.5, 0.8), (0.75, 0.8), (1.0, 10.0), (1.25, 0.8), (1.5, 0.8), (2.0, 10.0),
                                      (0.6, 0.8), (0.9, 10.0), (1.1, 0.8), (1.7, 0.8), (2.5, 0.8)))
E_KNOTS = np.array([0.0, 0.5, 1.0, 1.5, 2.0, 3.0])
E_TABLE = np.array([1.0, 1.5, 1.25, 2.0, 4.0, 3.0])

E_EXPRESSIONS = {
    "sqrt": lambda o, x, y: np.sqrt(o.q) * x,
    "exp": lambda o, x, y: np.exp(-o.q) * y,
    "log": lambda o, x, y: np.log(o.q),
    "sin cos": lambda o, x, y: np.sin(o.q) * np.cos(o.q * x),
    "tan": lambda o, x, y: np.tan(0.5 * o.q),
    "arctan": lambda o, x, y: np.arctan(o.q * y),
    "tanh": lambda o, x, y: np.tanh(o.q - x),
    "abs": lambda o, x, y: abs(o.q - 1.25) + 2.0 * o.q,
    "cbrt": lambda o, x, y: np.cbrt(o.q) + x,
    "hypot": lambda o, x, y: np.hypot(o.q, x),
    "q ** 2": lambda o, x, y: o.q ** 2,
    "x ** q": lambda o, x, y: x ** o.q,
    "q ** r": lambda o, x, y: o.q ** o.r,
    "2 / q": lambda o, x, y: 2.0 / o.q,
    "q * q": lambda o, x, y: o.q * o.q * x,
    "q / (1 + q)": lambda o, x, y: o.q / (1.0 + o.q),
    "where": lambda o, x, y: np.where(o.q > 1, x * o.q, y + o.q),
    "maximum": lambda o, x, y: np.maximum(o.q, 0.75) * x,
    "minimum": lambda o, x, y: np.minimum(o.q * x, o.r),
    "clip": lambda o, x, y: np.clip(o.q, 0.5, 2.0) * y,
    "%": lambda o, x, y: (o.q % 0.35) * x,
    "interp1d": lambda o, x, y: o.table(1.0 * o.q) * x,       # (a table's argument is a traced value, not the bare parameter)
    "q * r": lambda o, x, y: o.q * o.r + x,
}


def expression_problem(theta=None):
    theta = E_THETA[0] if theta is None else np.asarray(theta, dtype=float)
    prob = api.Problem([0.0, 1.0], [4], [1], [1], 1)
    obj = pc.Model()
    obj.q, obj.r = prob.parameter("q", theta[0]), prob.parameter("r", theta[1])
    obj.table = interpolate.interp1d(E_KNOTS, E_TABLE, fill_value="extrapolate")
    prob.set_states(0, 0, np.array([0.5, 1.5, 2.5, 3.5]))
    prob.set_controls(0, 0, np.array([-1.0, 0.25, 4.0, 9.0]))

    def dynamics(prob, obj, section):
        rhs = api.Dynamics(prob, section)
        rhs[0] = prob.controls(0, section)
        return rhs()

    def equality(prob, obj):
        x, y = prob.states(0, 0), prob.controls(0, 0)
        rows = api.Condition()
        for fn in E_EXPRESSIONS.values():
            rows.add(fn(obj, x, y) + 0.0 * x[0])
        return rows()

    prob.dynamics = [dynamics]
    prob.cost = lambda prob, obj: prob.states(0, 0)[-1]
    prob.equality = equality
    prob.inequality = lambda prob, obj: api.Condition()()
    return prob, obj


P2U_NAMES = pc.P2_NAMES + ("unit",)
P2U_THETA = tuple(np.append(t, u) for t, u in zip(pc.P2_THETA, (2.0, 0.5, 1.25)))


def p2_unit(theta=None):
    theta = P2U_THETA[0] if theta is None else np.asarray(theta, dtype=float)
    prob, obj = pc.p2(theta[:5])
    unit = prob.parameter("unit", theta[5])
    guess = [prob.states(1, sec) for sec in range(2)]
    prob.set_unit_states_all_section(1, unit)
    for sec in range(2):
        prob.set_states(1, sec, guess[sec])
    return prob, obj


# case -> (factory(theta), names, thetas)
CASES = {
    "P2": (pc.p2, pc.P2_NAMES, pc.P2_THETA),
    "P2U": (p2_unit, P2U_NAMES, P2U_THETA),
    "G9": (lambda theta=None: pc.goddard(9, theta), pc.G_NAMES, pc.G_THETA),
    "G17": (lambda theta=None: pc.goddard(17, theta), pc.G_NAMES, pc.G_THETA),
    "E": (expression_problem, E_NAMES, E_THETA),
}
UNREAD = {"P2": {4}, "P2U": {4}, "G9": set(), "G17": set(), "E": set()}


def points(key, prob, count=2):
    """``count`` decision vectors a little away from the guess.  The goddard guess has the speed at 0 everywhere and the
    altitude at ``H0`` at node 0, where ``dF/dHc`` is numerically zero: there the speed and the altitude excess are
    moved above zero at every node."""
    out = []
    for seed in range(count):
        x = pc.point(prob, seed)
        if key in ("G9", "G17"):
            N = prob.nodes[0]
            x[:N] += 0.0005 * (1.0 + np.arange(N)) * (1.0 + 0.25 * seed)
            x[N:2 * N] = 0.05 + 0.02 * np.arange(N) + 0.01 * seed
        out.append(x)
    return out


class Case:
    """One case, traced once: the program, the header, the problem at ``thetas[0]``."""

    def __init__(self, key):
        factory, self.names, self.thetas = CASES[key]
        self.key = key
        self.prob, self.obj = factory()
        self.program = pc.trace(self.prob, self.obj)
        self.header = codegen.emit_header(self.program)
        self.points = points(key, self.prob)
        self.n_par, self.m = self.program.n_par, self.program.m

    def cvec(self, theta):
        cv = np.array(self.program.cvec, dtype=np.float64)
        cv[self.program.par_off:] = theta
        return cv


_CASES = {}


def case(key):
    if key not in _CASES:
        _CASES[key] = Case(key)
    return _CASES[key]


# ------------------------------------------------------------------------------------------------ complex step in theta
class _ThetaEval(exact_jac._ComplexEval):
    """``_ComplexEval`` casts a scalar table entry to float64; here a parameter leaf carries the complex seed: column c of
    the evaluation has ``theta_c + i EPS``."""

    def elem(self, eid, length, memo):
        node = self.P.eg.nodes[eid]
        P = self.P
        if node[0] == "CV" and node[3] == 0 and node[1] == P.par_table:
            base = P.cvec_off[node[1]] + node[2]
            return P.cvec[base] + 1j * exact_jac.EPS * (np.arange(self.C) == base - P.par_off)
        return super().elem(eid, length, memo)


class _AtTheta:
    """The program with another parameter tail (the traced program itself is left alone)."""

    def __init__(self, P, cvec):
        self.__dict__.update(P.__dict__)
        self.cvec = cvec
        self.m = P.m


def complex_step(C, theta, x):
    """``dF[k, r] = dF_r/dtheta_k`` at ``x``: the lowered program on ``theta + i EPS e_k``, NumPy's complex arithmetic.
    It shares no generated code and no derivative rule with the kernels."""
    P = _AtTheta(C.program, C.cvec(theta))
    z = np.repeat(np.asarray(x, dtype=complex)[:, None], C.n_par, axis=1)
    ev = _ThetaEval(P, z, C.prob.D)
    F = np.full((C.m, C.n_par), np.nan, dtype=complex)
    for row, ln, eid, _kind in C.program.pieces:
        F[row:row + ln] = ev.elem(eid, ln, {})
    return np.imag(F).T / exact_jac.EPS


def worst_error(dF, ref):
    """Largest difference, in units of the row's largest entry over the parameters (at least 1: ``worst_error`` of
    tests/test_exact_surface.py)."""
    scale = np.maximum(1.0, np.abs(ref).max(axis=0))[None, :]
    return float(np.max(np.abs(dF - ref) / scale)) if dF.size else 0.0


# ------------------------------------------------------------------------------------------------ the host probe
def build_probe(C, folder, compiler="g++", sanitize=False):
    """tests/par_exact_probe.cpp against this case's header: a program of its own."""
    header = os.path.join(folder, "og_gen_%s.h" % C.key)
    if not os.path.exists(header):
        with open(header, "w") as fh:
            fh.write(C.header)
    exe = os.path.join(folder, "par_probe_%s_%s%s" % (C.key, os.path.basename(compiler).replace("+", "x"), "_san" if sanitize else ""))
    if os.path.exists(exe):
        return exe
    base = [compiler] + PROBE_FLAGS + ["-DOG_GEN_HEADER=\"%s\"" % header, PROBE_SOURCE, "-o", exe,
                                          "-lstdc++", "-lm"]      # (the toolchain's clang++ may resolve to the C driver)
    if sanitize:
        base = base[:1] + ["-O1", "-fsanitize=address,undefined"] + base[1:]
        proc = subprocess.run(base + ["-static-libasan", "-static-libubsan"], stdout=subprocess.PIPE,
                              stderr=subprocess.STDOUT, text=True)
        if proc.returncode == 0:
            return exe
    proc = subprocess.run(base, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert proc.returncode == 0, proc.stdout[-3000:]
    return exe


def run_probe(C, exe, folder, theta, x, tag="run"):
    """-> ``(dF[n_par, m], F0[m])`` of the probe at ``(theta, x)``."""
    data, out = os.path.join(folder, "%s_%s.in" % (C.key, tag)), os.path.join(folder, "%s_%s.out" % (C.key, tag))
    cv = C.cvec(theta)
    np.concatenate([np.asarray(x, dtype=np.float64), cv if cv.size else np.zeros(1)] +
                   [np.ascontiguousarray(D, dtype=np.float64).reshape(-1) for D in C.prob.D]).tofile(data)
    env = dict(os.environ, UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    proc = subprocess.run([exe, data, out], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, env=env, timeout=300)
    assert proc.returncode == 0 and "runtime error" not in proc.stdout, proc.stdout[-3000:]
    got = np.fromfile(out)
    assert got.size == (C.n_par + 1) * C.m
    return got[:C.n_par * C.m].reshape(C.n_par, C.m), got[C.n_par * C.m:]


# what __graft_entry__.build compiles besides parameter_cases.modules(): (label, factory), each with its parameter part
def modules():
    return [("parameter exact " + key, (lambda key=key: CASES[key][0]())) for key in ("P2U", "E")]
