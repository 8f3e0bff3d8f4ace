"""The cases of tests/test_parameter_hessian.py and tests/test_parameter_hessian_gpu.py (and of
``__graft_entry__.build``, which compiles the cases' modules, batch parts and parameter-Hessian parts ahead of the GPU
run): the host probe of ``csrc/og_pp.h`` and the independent reference of
``S_kl = sum_r w_r d2F_r/dtheta_k dtheta_l``.

The cases are the smallest shapes at which each path of the definition and of the kernel can go wrong; all reuse existing
factories:

``E``     of ``parameter_exact_cases``: 4 nodes, two parameters, every operator applied to a parameter - among its rows
          ``q ** r``, ``q * r + x``, ``minimum(q * x, r)``, ``q ** 2``, ``2 / q`` - at all 11 parameter sets, six of
          which sit on a switch.
``P2U``   six parameters; parameter 4 is read by nothing; a state's unit is a parameter, so the operand term of a
          collocation entry is not zero.
``NLP``   of ``nonlocal_cases``: the tail reads across nodes and the parameter enters linearly: the diagonal is +0.0.
``G17``   ``parameter_cases.goddard(17)``: lists of 17 and 18 entries - one partly filled block of 64 chains and three
          empty blocks.
``G90``   ``goddard(90)``: 90 and 91 entries, the second block partly filled.
``G257``  ``goddard(257)``: 257 and 258 entries - chains 0 and 1 make a second trip, the others one.

The weight vectors are the nine of ``mixed_cases.weights``: K = 9 is one full chunk of 8 and a chunk of one vector.
"""
import os
import subprocess

import numpy as np

import mixed_cases as mc
import parameter_cases as pc
import parameter_exact_cases as ec
from opengoddard_amd import codegen

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROBE_SOURCE = os.path.join(ROOT, "tests", "pp_probe.cpp")
KEYS = ("E", "P2U", "NLP", "G17", "G90", "G257")
GODDARD_NODES = {"G90": 90, "G257": 257}
weights = mc.weights


class _Goddard:
    """``parameter_cases.goddard(N)`` in the form of ``mixed_cases.Case``."""

    def __init__(self, key):
        self.key = key
        N = GODDARD_NODES[key]
        self.prob, self.obj = pc.goddard(N)
        self.names, self.thetas = tuple(pc.G_NAMES), list(pc.G_THETA)
        self.program = pc.trace(self.prob, self.obj)
        self.header = codegen.emit_header(self.program)
        # (as parameter_exact_cases.points does for G9 / G17: the speed and the altitude excess above zero at every node)
        self.points = []
        for seed in range(2):
            x = pc.point(self.prob, seed)
            x[:N] += 0.0005 * (1.0 + np.arange(N)) * (1.0 + 0.25 * seed) * 17.0 / N
            x[N:2 * N] = 0.05 + 0.02 * np.arange(N) * 17.0 / N + 0.01 * seed
            self.points.append(x)
        self.n, self.m, self.n_par = self.program.n, self.program.m, self.program.n_par
        self.unread = set()

    cvec = mc.Case.cvec
    at = mc.Case.at


_CASES = {}


def case(key):
    if key not in _CASES:
        _CASES[key] = _Goddard(key) if key in GODDARD_NODES else mc.case(key)
    return _CASES[key]


def pairs(n_par):
    """The pairs ``(k, l)``, ``k <= l``, in the order of ``og_pp_pair``: row-major over the upper triangle."""
    return [(k, l) for k in range(n_par) for l in range(k, n_par)]


def entries(C):
    """``PAR_ENTRIES`` of the case's header, per parameter."""
    return list(codegen.ParameterPlan(C.program).entries)


def owner(C, k, l):
    """The owner of the pair by the rule of og_pp.h, from the plan alone: fewer entries, a tie to the lower index."""
    e = entries(C)
    return l if e[l] < e[k] else k


# ------------------------------------------------------------------------------------------------ the host probe
def build_probe(C, folder, compiler="g++", sanitize=False):
    """tests/pp_probe.cpp against this case's header, with ``parameter_exact_cases.PROBE_FLAGS``: a program of its
    own."""
    header = os.path.join(folder, "og_gen_%s.h" % C.key)
    if not os.path.exists(header):
        with open(header, "w") as fh:
            fh.write(C.header)
    exe = os.path.join(folder, "pp_probe_%s_%s%s" % (C.key, os.path.basename(compiler).replace("+", "x"),
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
    """What one run of the probe returns: ``S[K, n_par, n_par]``, ``A[K, n_par, n_par]``
    (``sum_r |w_r d2F_r/dtheta_k dtheta_l|``), ``F0[m]``, per pair (in the order of :func:`pairs`) ``owner``,
    ``partner``, ``entries`` and ``checked2`` (the entries whose slot-2 part was held to the partner's ``og_par_entry``),
    and ``D1[pairs, m]``, ``D2[pairs, m]``, ``have[pairs, m]``: the slot-1 and slot-2 first-order parts of the pair's
    entries by row."""


def run_probe(C, exe, folder, x, W, theta, tag="run", check=True):
    """The probe at ``x`` and ``theta`` for the rows of ``W``.  The probe itself fails (exit status 1) unless every one
    of the ``n_par * n_par`` entries of every vector, pre-filled with NaN, is written exactly once, every entry's slot-1
    part is the owner's ``og_par_entry`` and its slot-2 part the partner's at the same row, bit for bit."""
    W = np.atleast_2d(np.asarray(W, dtype=np.float64))
    K, m, P = W.shape[0], C.m, C.n_par
    Q = P * (P + 1) // 2
    assert W.shape == (K, m)
    data, out = os.path.join(folder, "%s_%s.in" % (C.key, tag)), os.path.join(folder, "%s_%s.out" % (C.key, tag))
    np.concatenate([np.asarray(x, dtype=np.float64), C.cvec(theta)] +
                   [np.ascontiguousarray(D, dtype=np.float64).reshape(-1) for D in C.prob.D] + [W.reshape(-1)]).tofile(data)
    env = dict(os.environ, UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    proc = subprocess.run([exe, data, out], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, env=env,
                          timeout=300)
    assert "runtime error" not in proc.stdout and "Sanitizer" not in proc.stdout, proc.stdout[-3000:]
    if check:
        assert proc.returncode == 0, proc.stdout[-3000:]
        assert "vectors=%d parameters=%d pairs=%d " % (K, P, Q) in proc.stdout and " bad=0" in proc.stdout, \
            proc.stdout[-3000:]
    got = np.fromfile(out)
    sizes = [K * P * P, K * P * P, m, Q, Q, Q, Q * m, Q * m, Q * m, Q]
    assert got.size == sum(sizes)
    S, A, F0, own, partner, ent, D1, D2, have, checked2 = np.split(got, np.cumsum(sizes)[:-1])
    r = Probed()
    r.S, r.A, r.F0 = S.reshape(K, P, P), A.reshape(K, P, P), F0
    r.owner, r.partner, r.entries, r.checked2 = own.astype(int), partner.astype(int), ent.astype(int), checked2.astype(int)
    r.D1, r.D2, r.have = D1.reshape(Q, m), D2.reshape(Q, m), have.reshape(Q, m).astype(bool)
    r.stdout, r.returncode = proc.stdout, proc.returncode
    return r


# ------------------------------------------------------------------------------------------------ the reference
H_STEP = 2.0 ** -9


def _steps(theta, l, h):
    theta = np.asarray(theta, dtype=float)
    unit = np.zeros_like(theta)
    unit[l] = 1.0
    return theta, unit, h * max(1.0, abs(theta[l]))


def oracle_second(C, x, W, theta, l, h=H_STEP):
    """``(ref[K, n_par], err[K, n_par])``: column ``l`` of ``S`` for the rows of ``W`` - central differences in
    ``theta_l`` of ``parameter_exact_cases.complex_step`` (``dF/dtheta_k`` by the oracle's complex step), contracted with
    ``w`` in ``np.longdouble``, Richardson-extrapolated from the step ``h max(1, |theta_l|)`` and its half; ``err`` is the
    reference's own error estimate: the difference from the extrapolation from the half and the quarter step.  It shares
    no generated code and no derivative rule with the kernels."""
    WL = np.atleast_2d(np.asarray(W, dtype=float)).astype(np.longdouble)
    theta, unit, base = _steps(theta, l, h)

    def central(step):
        up = ec.complex_step(C, theta + step * unit, x).astype(np.longdouble)       # [n_par, m]
        dn = ec.complex_step(C, theta - step * unit, x).astype(np.longdouble)
        return (WL @ (up - dn).T) / np.longdouble(2.0 * step)                       # [K, n_par]

    d0, d1, d2 = central(base), central(base / 2), central(base / 4)
    r0, r1 = (4 * d1 - d0) / 3, (4 * d2 - d1) / 3
    return r1, np.abs(r1 - r0).astype(float)


def one_sided_second(C, x, W, theta, l, side, h=H_STEP):
    """As :func:`oracle_second`, from the second-order one-sided difference on ``side`` (+1 / -1) - the form of
    tests/test_mixed.py: ``side (-3 f(t) + 4 f(t + side s) - f(t + 2 side s)) / (2 s)``, Richardson-extrapolated."""
    WL = np.atleast_2d(np.asarray(W, dtype=float)).astype(np.longdouble)
    theta, unit, base = _steps(theta, l, h)
    f = lambda t: ec.complex_step(C, t, x).astype(np.longdouble)
    f0 = f(theta)

    def diff(step):
        return side * (WL @ (-3 * f0 + 4 * f(theta + side * step * unit) - f(theta + 2 * side * step * unit)).T) / \
            np.longdouble(2.0 * step)

    d0, d1, d2 = diff(base), diff(base / 2), diff(base / 4)
    r0, r1 = (4 * d1 - d0) / 3, (4 * d2 - d1) / 3
    return r1, np.abs(r1 - r0).astype(float)


def open_sided_second(C, x, W, theta, l, side, h=H_STEP):
    """As :func:`one_sided_second`, from a stencil that does not hold ``theta`` itself:
    ``side (-5 f(t + side s) + 8 f(t + 2 side s) - 3 f(t + 3 side s)) / (2 s)``, the second-order extrapolation of the
    difference quotient to ``t`` (the coefficients solve ``a + b + c = 0``, ``a + 2 b + 3 c = 1 / s``,
    ``a + 4 b + 9 c = 0``), Richardson-extrapolated from ``s`` and ``s / 2`` like the others.  Needed where ``dF/dtheta`` AT
    a kink is that of neither side - the complex step gives ``abs`` the slope 0 at 0, between -1 and +1 - so that both
    closed one-sided stencils hold a jump."""
    WL = np.atleast_2d(np.asarray(W, dtype=float)).astype(np.longdouble)
    theta, unit, base = _steps(theta, l, h)
    f = lambda t: ec.complex_step(C, t, x).astype(np.longdouble)

    def diff(step):
        return side * (WL @ (-5 * f(theta + side * step * unit) + 8 * f(theta + 2 * side * step * unit) -
                             3 * f(theta + 3 * side * step * unit)).T) / np.longdouble(2.0 * step)

    d0, d1, d2 = diff(base), diff(base / 2), diff(base / 4)
    r0, r1 = (4 * d1 - d0) / 3, (4 * d2 - d1) / 3
    return r1, np.abs(r1 - r0).astype(float)


# what __graft_entry__.build compiles for tests/test_parameter_hessian_gpu.py: (label, header), each with its batch part
# and its parameter-Hessian part
def modules():
    return [("parameter Hessian " + key, case(key).header) for key in KEYS]
