"""The cases of tests/test_mixed.py and tests/test_mixed_gpu.py (and of ``__graft_entry__.build``, which compiles the
cases' modules, batch parts and mixed parts ahead of the GPU run): weight vectors, the host probe of ``csrc/og_mix.h``
and the independent reference of ``d(F'(x)^T w)/dtheta_k``.

The cases are the parameterised ones of ``parameter_exact_cases`` - ``P2U`` (a state's unit is a parameter, so the
collocation operand reads it: the operand term of a column's own block is not zero; parameter 4 is read by nothing),
``P2``, ``G9`` / ``G17`` (``n`` no multiple of 4: the last workgroup of the wavefront mapping is partly filled), ``E``
(every operator applied to a parameter, parameter values on every switch) - and ``B90g``: the 90-node brachistochrone of
``adjoint_cases.ManyTerms`` with the gravity declared a parameter, the only shape whose heavy column (the final time, 272
terms: a thread's second trip through its chain, the workgroup path) reads a parameter - and ``NLP`` of
``nonlocal_cases``: ``dx[0] = v - a * (x - x.mean())`` sets bit 1 of the ``reads`` word of ``x``, so the term
``d2 tail_k / dx_l da`` of og_mix.h is not zero off the diagonal of that state's own block (the only case where it is
not), at both of its parameter sets.  These are the smallest shapes at which each path of the kernel runs.
"""
import os
import subprocess

import numpy as np

import adjoint_cases as ac
import parameter_cases as pc
import parameter_exact_cases as ec
from opengoddard_amd import codegen, problems
from oracle import exact_jac

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROBE_SOURCE = os.path.join(ROOT, "tests", "mix_probe.cpp")
KEYS = ("P2U", "P2", "G9", "G17", "E", "B90g", "NLP")
B90G_THETA = (np.array([1.0]), np.array([0.8125]), np.array([1.375]))


class Case:
    """One case, traced once: program, header, points, parameter sets."""

    def __init__(self, key):
        self.key = key
        if key == "B90g":
            self.prob, self.obj = problems.build("brachistochrone", nodes=[90])
            self.obj.gravity = self.prob.parameter("g", B90G_THETA[0][0])
            self.names, self.thetas = ("g",), list(B90G_THETA)
            self.program = pc.trace(self.prob, self.obj)
            self.header = codegen.emit_header(self.program)
            base = np.array(self.prob.p, dtype=float)
            rng = np.random.default_rng(17)
            # (the guess has the speed at zero everywhere: moved off it, so that the terms in v are not all zero)
            self.points = [base * (1.0 + 0.02 * rng.standard_normal(base.size)) + 0.01 * rng.random(base.size)
                           for _ in range(2)]
        else:
            if key == "NLP":
                import nonlocal_cases
                C = nonlocal_cases.case(key)
            else:
                C = ec.case(key)
            self.prob, self.obj, self.program, self.header = C.prob, C.obj, C.program, C.header
            self.names, self.thetas, self.points = tuple(C.names), list(C.thetas), list(C.points)
        self.n, self.m, self.n_par = self.program.n, self.program.m, self.program.n_par
        self.unread = ec.UNREAD.get(key, set())

    def cvec(self, theta=None):
        cv = np.array(self.program.cvec, dtype=np.float64)
        if theta is not None:
            cv[self.program.par_off:] = theta
        return cv

    def at(self, theta):
        """The program with the parameter tail ``theta`` (the traced program itself is left alone)."""
        return ec._AtTheta(self.program, self.cvec(theta))


_CASES = {}


def case(key):
    if key not in _CASES:
        _CASES[key] = Case(key)
    return _CASES[key]


def weights(C):
    """``[9, m]``: the eight vectors of ``adjoint_cases.weights`` (e_0, the last row, ones, three seeded, zero, one
    without the defect rows) and a ninth seeded one."""
    w = np.random.default_rng(31).standard_normal(C.m)
    return np.vstack([ac.weights(C), w / np.abs(w).max()])


# ------------------------------------------------------------------------------------------------ the host probe
def build_probe(C, folder, compiler="g++", sanitize=False):
    """tests/mix_probe.cpp against this case's header, with ``parameter_exact_cases.PROBE_FLAGS``: a program of its
    own."""
    header = os.path.join(folder, "og_gen_%s.h" % C.key)
    if not os.path.exists(header):
        with open(header, "w") as fh:
            fh.write(C.header)
    exe = os.path.join(folder, "mix_probe_%s_%s%s" % (C.key, os.path.basename(compiler).replace("+", "x"),
                                                     "_san" if sanitize else ""))
    if os.path.exists(exe):
        return exe
    base = [compiler] + ec.PROBE_FLAGS + ["-DOG_GEN_HEADER=\"%s\"" % header, PROBE_SOURCE, "-o", exe, "-lstdc++", "-lm"]
    if sanitize:
        base = base[:1] + ["-O1", "-fsanitize=address,undefined"] + base[1:]
        proc = subprocess.run(base + ["-static-libasan", "-static-libubsan"], stdout=subprocess.PIPE,
                              stderr=subprocess.STDOUT, text=True)
        if proc.returncode == 0:
            return exe
    proc = subprocess.run(base, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert proc.returncode == 0, proc.stdout[-3000:]
    return exe


class Probed:
    """What one run of the probe returns: ``S[K, n_par, n]`` (the mixed derivatives), ``G[K, n]`` (the slot-1 first-order
    parts of the same terms in the same order of sums), ``A[K, n_par, n]`` (``sum_r |w_r d2F_r/dx_j dtheta_k|``),
    ``F0[m]``, ``P[n_par, m]`` (the slot-2 first-order part of a row's items) with ``have[m]`` (the row has an item), and
    per variable ``terms``, ``reads`` (-1: no node of a collocated state) and ``heavy``."""


def run_probe(C, exe, folder, x, W, theta, tag="run"):
    """The probe at ``x`` and ``theta`` for the rows of ``W``.  The probe itself fails (exit status 1) unless every one
    of the ``n_par * n`` entries of every vector, pre-filled with NaN, is written exactly once, no column has two terms
    in one row, a term's slot-1 part does not depend on the parameter and a row item's slot-2 part not on the column."""
    W = np.atleast_2d(np.asarray(W, dtype=np.float64))
    K, n, m, n_par = W.shape[0], C.n, C.m, C.n_par
    assert W.shape == (K, m)
    data, out = os.path.join(folder, "%s_%s.in" % (C.key, tag)), os.path.join(folder, "%s_%s.out" % (C.key, tag))
    np.concatenate([np.asarray(x, dtype=np.float64), C.cvec(theta)] +
                   [np.ascontiguousarray(D, dtype=np.float64).reshape(-1) for D in C.prob.D] + [W.reshape(-1)]).tofile(data)
    env = dict(os.environ, UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    proc = subprocess.run([exe, data, out], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, env=env,
                          timeout=300)
    assert proc.returncode == 0 and "runtime error" not in proc.stdout, proc.stdout[-3000:]
    assert "vectors=%d parameters=%d variables=%d " % (K, n_par, n) in proc.stdout and " bad=0" in proc.stdout, \
        proc.stdout[-3000:]
    got = np.fromfile(out)
    sizes = [K * n_par * n, K * n, K * n_par * n, m, n_par * m, m, n, n, n]
    assert got.size == sum(sizes)
    S, G, A, F0, P, have, terms, reads, heavy = np.split(got, np.cumsum(sizes)[:-1])
    r = Probed()
    r.S, r.G, r.A, r.F0 = S.reshape(K, n_par, n), G.reshape(K, n), A.reshape(K, n_par, n), F0
    r.P, r.have = P.reshape(n_par, m), have.astype(bool)
    r.terms, r.reads, r.heavy = terms.astype(int), reads.astype(int), heavy.astype(int)
    return r


# ------------------------------------------------------------------------------------------------ the reference
H_STEP = 2.0 ** -9


def oracle_mixed(C, x, W, theta, k, h=H_STEP):
    """``(ref[K, n], err[K, n])`` for ONE parameter ``k`` and the rows of ``W``: central differences in ``theta_k`` of the
    oracle's complex-step ``J^T w`` (``oracle.exact_jac.jacobian`` of the program at ``theta +- step e_k``, the product in
    ``np.longdouble``), Richardson-extrapolated from ``step`` and ``step / 2``; ``err`` is the reference's own error
    estimate, the difference between the extrapolations from ``(step, step / 2)`` and ``(step / 2, step / 4)``.  The
    step is ``h max(1, |theta_k|)``.  It shares no generated code and no derivative rule with the kernels, and uses
    neither ``og_dual2.h`` nor ``og_mix.h``."""
    WL = np.atleast_2d(np.asarray(W, dtype=float)).astype(np.longdouble)
    theta = np.asarray(theta, dtype=float)
    unit = np.zeros_like(theta)
    unit[k] = 1.0
    base = h * max(1.0, abs(theta[k]))

    def central(step):
        up = exact_jac.jacobian(C.at(theta + step * unit), C.prob, x).astype(np.longdouble)       # J_T [n, m]
        dn = exact_jac.jacobian(C.at(theta - step * unit), C.prob, x).astype(np.longdouble)
        return ((up - dn) @ WL.T).T / np.longdouble(2.0 * step)

    d0, d1, d2 = central(base), central(base / 2), central(base / 4)
    r0, r1 = (4 * d1 - d0) / 3, (4 * d2 - d1) / 3
    return r1, np.abs(r1 - r0).astype(float)


# what __graft_entry__.build compiles for tests/test_mixed_gpu.py: (label, header), each with its mixed part and its
# batch part
def modules():
    return [("mixed " + key, case(key).header) for key in KEYS]
