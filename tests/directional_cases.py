"""The cases of tests/test_directional.py and tests/test_directional_gpu.py (and of ``__graft_entry__.build``, which
compiles the GPU cases' modules and directional parts ahead of the GPU run): problems, points, directions, the two
references of ``F'(x) v`` and the host probe of ``csrc/og_dir.h``.

Cases: ``brachistochrone``; every problem of ``test_exact_surface.PROBLEMS`` - the 8 edge problems, the 9 random layouts
and ``table_ascent`` (``interp1d``) - at their own four named points; the
parameterised ``P2U`` and ``G17`` of tests/parameter_exact_cases.py (imported: their own points and parameter sets);
``B5``, the brachistochrone on 5 nodes.  Every case adds seeded 2 % perturbations of its first point.  ``NL2`` and ``NL0``
are built by ``nonlocal_cases`` (dynamics that read a state across the nodes of its phase: bit 1 of a slot's ``reads``
word, which no other case here sets), with its own three points.
"""
import os
import subprocess

import numpy as np

import parameter_exact_cases as ec
import test_exact_surface as surface
from opengoddard_amd import codegen, problems
from oracle import exact_jac

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROBE_SOURCE = os.path.join(ROOT, "tests", "dir_probe.cpp")
BOUND = surface.BOUND           # 1e-12, of max(1, sum_j |J_rj v_j|) per row

SURFACE_KEYS = ("brachistochrone",) + tuple(surface.PROBLEMS)
PARAMETER_KEYS = ("P2U", "G17")
NONLOCAL_KEYS = ("NL2", "NL0")
CPU_KEYS = SURFACE_KEYS + PARAMETER_KEYS + NONLOCAL_KEYS
# the GPU test's shapes: 5 nodes (N no multiple of 4, one partly filled workgroup); 17 nodes (across the 16-row block of
# the operand image); two phases of 65 and 31 nodes (DFRAG_OFF, 423 entries: blockIdx.x = 1 with a ragged workgroup);
# a parameterised module; two phases of 21 and 6 nodes whose own collocation blocks are full (a sum of squares over the
# state's slice; its first and last value)
GPU_KEYS = ("B5", "G17", "layout_8", "P2U") + NONLOCAL_KEYS


class Case:
    """One case, traced once: program, header, points, and for a parameterised case its parameter sets."""

    def __init__(self, key):
        self.key = key
        self.thetas = [None]
        if key in PARAMETER_KEYS:
            C = ec.case(key)
            self.prob, self.obj, self.program, self.header = C.prob, C.obj, C.program, C.header
            self.points = list(C.points)
            self.thetas = list(C.thetas[:2])
            self._cvec = C.cvec
        else:
            if key == "B5":
                self.prob, self.obj = problems.build("brachistochrone", nodes=[5])
            elif key == "brachistochrone":
                self.prob, self.obj = problems.build(key)
            else:
                self.prob, self.obj = surface.build_problem(key)
            self.program = codegen.trace_problem(self.prob, self.obj)
            self.header = codegen.emit_header(self.program)
            if key in ("B5", "brachistochrone"):
                self.points = [np.array(self.prob.p, dtype=float)]
            else:
                named = surface.surface_points(key, self.prob)
                self.points = [named[name] for name in surface.POINTS]
        rng = np.random.default_rng(17)
        base = self.points[0]
        self.points += [base * (1.0 + 0.02 * rng.standard_normal(base.size)) for _ in range(2)]
        self.n, self.m = self.program.n, self.program.m

    def cvec(self, theta=None):
        if theta is None:
            return np.array(self.program.cvec, dtype=np.float64)
        return self._cvec(theta)

    def at(self, theta=None):
        """The program with the parameter tail ``theta`` (the traced program itself is left alone)."""
        return self.program if theta is None else ec._AtTheta(self.program, self.cvec(theta))

    def directions(self):
        """``[7, n]``: e_0, e_{n-1}, the unit vector of the first phase's final time, three seeded random vectors of
        unit max-norm, the zero vector.  (The final times are the last ``number_of_section`` variables: n - 1 is the last
        phase's, so with one phase rows 1 and 2 coincide.)"""
        n = self.n
        V = np.zeros((7, n))
        V[0, 0] = V[1, n - 1] = 1.0
        V[2, n - len(self.prob.nodes)] = 1.0
        rng = np.random.default_rng(23)
        for r in range(3, 6):
            v = rng.standard_normal(n)
            V[r] = v / np.abs(v).max()
        return V


_CASES = {}


def case(key):
    if key not in _CASES:
        if key in NONLOCAL_KEYS:
            import nonlocal_cases               # (it imports this module for ``Case``)
            _CASES[key] = nonlocal_cases.case(key)
        else:
            _CASES[key] = Case(key)
    return _CASES[key]


# ------------------------------------------------------------------------------------------------ the two references
def complex_step(C, x, V, theta=None):
    """``[K, m]``: ``Im F(x + i EPS v) / EPS`` of the lowered program, NumPy's complex arithmetic, one column per
    direction.  It shares no generated code and no derivative rule with the kernels."""
    V = np.atleast_2d(np.asarray(V, dtype=float))
    z = np.asarray(x, dtype=complex)[:, None] + 1j * exact_jac.EPS * V.T
    ev = exact_jac._ComplexEval(C.at(theta), z, C.prob.D)
    F = np.full((C.m, V.shape[0]), np.nan, dtype=complex)
    for row, ln, eid, _kind in C.program.pieces:
        F[row:row + ln] = ev.elem(eid, ln, {})
    return np.imag(F).T / exact_jac.EPS


def twin_product(JT, V):
    """``(J v [K, m], scale [K, m])`` from the twin's exact ``J_T [n, m]``: the product accumulated in
    ``np.longdouble``, and ``max(1, sum_j |J_rj v_j|)`` per row - the unit of every error here."""
    V = np.atleast_2d(np.asarray(V, dtype=float))
    JL, VL = JT.astype(np.longdouble), V.astype(np.longdouble)
    prod = np.stack([(JL * v[:, None]).sum(axis=0) for v in VL])
    scale = np.stack([np.abs(JL * v[:, None]).sum(axis=0) for v in VL])
    return prod, np.maximum(1.0, scale.astype(float))


def worst_error(dF, ref, scale):
    return float(np.max(np.abs(dF.astype(np.longdouble) - ref) / scale)) if dF.size else 0.0


# ------------------------------------------------------------------------------------------------ the host probe
def build_probe(C, folder, compiler="g++", sanitize=False):
    """tests/dir_probe.cpp against this case's header, with ``parameter_exact_cases.PROBE_FLAGS``: a program of its
    own."""
    header = os.path.join(folder, "og_gen_%s.h" % C.key)
    if not os.path.exists(header):
        with open(header, "w") as fh:
            fh.write(C.header)
    exe = os.path.join(folder, "dir_probe_%s_%s%s" % (C.key, os.path.basename(compiler).replace("+", "x"),
                                                     "_san" if sanitize else ""))
    if os.path.exists(exe):
        return exe
    base = [compiler] + ec.PROBE_FLAGS + ["-DOG_GEN_HEADER=\"%s\"" % header, PROBE_SOURCE, "-o", exe,
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


def run_probe(C, exe, folder, x, V, theta=None, tag="run", seeded=False):
    """-> ``(dF[K, m], F0[m])`` of the probe at ``x`` along the rows of ``V``.  The probe itself fails (exit status 1)
    unless every one of the ``m`` rows of every direction, pre-filled with NaN, is written exactly once."""
    V = np.atleast_2d(np.asarray(V, dtype=np.float64))
    data, out = os.path.join(folder, "%s_%s.in" % (C.key, tag)), os.path.join(folder, "%s_%s.out" % (C.key, tag))
    cv = C.cvec(theta)
    np.concatenate([np.asarray(x, dtype=np.float64), cv if cv.size else np.zeros(1)] +
                   [np.ascontiguousarray(D, dtype=np.float64).reshape(-1) for D in C.prob.D] +
                   [V.reshape(-1)]).tofile(data)
    env = dict(os.environ, UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    proc = subprocess.run([exe, data, out] + (["seeded"] if seeded else []), stdout=subprocess.PIPE,
                          stderr=subprocess.STDOUT, text=True, env=env, timeout=300)
    assert proc.returncode == 0 and "runtime error" not in proc.stdout, proc.stdout[-3000:]
    assert "directions=%d rows=%d entries=%d bad=0" % (V.shape[0], C.m, C.m) in proc.stdout, proc.stdout[-3000:]
    got = np.fromfile(out)
    assert got.size == (V.shape[0] + 1) * C.m
    return got[:V.shape[0] * C.m].reshape(V.shape[0], C.m), got[V.shape[0] * C.m:]


# what __graft_entry__.build compiles for tests/test_directional_gpu.py: (label, header), each with its directional part
# and its batch part
def modules():
    return [("directional " + key, case(key).header) for key in GPU_KEYS]
