"""The cases of tests/test_adjoint.py and tests/test_adjoint_gpu.py (and of ``__graft_entry__.build``, which compiles the
GPU cases' modules, batch parts and adjoint parts ahead of the GPU run): weight vectors, the reference of
``F'(x)^T w`` and the host probe of ``csrc/og_adj.h``.  Problems, points and parameter sets are those of
``directional_cases`` (``dc.case``), the probe's flags ``parameter_exact_cases.PROBE_FLAGS``.

What the GPU shapes cover (``COVERAGE`` below, checked on the CPU by tests/test_adjoint.py against the term counts and
``reads`` words the probe reports; a term is one entry of a column of the exact Jacobian).  The six shapes of the
directional GPU test have no column with more than 256 terms - nor has any surface problem - so ``B90``, the
brachistochrone on 90 nodes, joins them:

* more than 256 terms, so a thread's second trip through its chain: the final time of ``B90``, its last variable, 272
  terms (3 states x 90 defect rows and two rows that read it) - and only it;
* 64 to 256 terms (more than one wavefront holds a term): the 270 state columns of ``B90`` (the state's own 90 defect rows
  and its row items), 132 columns of ``layout_8``;
* fewer than 64 terms (three of the four wavefronts hold nothing but +0.0): every column of ``B5``, ``G17`` and ``P2U``,
  the control columns of ``B90``;
* no term at all: the variables 195 .. 324 of ``layout_8``, which no callback of that random layout reads;
* a collocation slot's ``reads`` word (bit 0: the dynamics term at node k reads the state at node k, bit 1: it reads the
  state's slice in some other way, and then every entry of the column's own block has a dynamics part) takes the values
  0 and 1 on the surface problems and the parameterised ones: 1 on all five of their shapes, 0 on ``B5``, ``B90`` and
  ``layout_8``.  (One surface problem that is no GPU shape has 3: ``wide_reductions`` reduces over a state's slice.)
  ``NL2`` and ``NL0`` of ``nonlocal_cases`` bring the other two: 2 on ``NL2`` (``np.sum(x * x)`` and nothing else of ``x``
  in its own row), 3 on ``NL0`` (``cos(x - x[0])``; ``v[0]`` next to ``v``).  A column that is no
  node of a collocated state (controls, final times; -1 here) is on all of them.
"""
import os
import subprocess

import numpy as np

import directional_cases as dc
import parameter_exact_cases as ec
import test_exact_surface as surface
from opengoddard_amd import codegen, problems

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROBE_SOURCE = os.path.join(ROOT, "tests", "adj_probe.cpp")
BOUND = surface.BOUND           # 1e-12, of max(1, sum_r |J_rj w_r|) per column

CPU_KEYS = dc.CPU_KEYS
# g++ needs more than ten minutes per probe for the build with the address and undefined-behaviour sanitizers on this
# problem's header (407 variables, reductions over 135 nodes); the toolchain's clang++ needs four.  So the sanitizer builds
# of this key are clang++'s, and ``__graft_entry__.build`` compiles them ahead (``hessian_matrix_cases.probe_jobs``).
SANITIZE_WITH_CLANG = ("wide_reductions",)
PREBUILT = os.path.join(ROOT, "tools", "_build", "hess_probes")


def sanitizer_compiler(key):
    import og_math_cases
    return og_math_cases.clangxx() if key in SANITIZE_WITH_CLANG else "g++"


_VERSIONS = {}


def _version(compiler):
    if compiler not in _VERSIONS:
        _VERSIONS[compiler] = subprocess.run([compiler, "--version"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT).stdout
    return _VERSIONS[compiler]


def prebuilt_folder(C):
    """``tools/_build/hess_probes/<key>_<digest>``: the digest is over everything a probe of this case is compiled from -
    the header, the probes' sources, ``csrc/*.h``, the flags and both compilers' versions - so a stale one is never
    picked up."""
    import hashlib
    import og_math_cases
    h = hashlib.sha1(C.header.encode())
    csrc, tests = os.path.join(ROOT, "opengoddard_amd", "csrc"), os.path.join(ROOT, "tests")
    for path in sorted(os.path.join(tests, f) for f in os.listdir(tests) if f.endswith("_probe.cpp")) + \
            sorted(os.path.join(csrc, f) for f in os.listdir(csrc) if f.endswith(".h")):
        with open(path, "rb") as fh:
            h.update(fh.read())
    h.update(repr(ec.PROBE_FLAGS).encode())
    h.update(_version("g++") + _version(og_math_cases.clangxx()))
    return os.path.join(PREBUILT, "%s_%s" % (C.key, h.hexdigest()[:16]))


def probe_folder(C, fallback):
    """Where probes of this case built ahead are: the folder ``build()`` filled, or ``fallback`` (compiled there)."""
    folder = prebuilt_folder(C)
    return folder if os.path.isdir(folder) else fallback
GPU_KEYS = dc.GPU_KEYS + ("B90",)


class ManyTerms(dc.Case):
    """``B90``, the brachistochrone on 90 nodes: its final time has more than 256 terms."""

    def __init__(self):
        self.key = "B90"
        self.thetas = [None]
        self.prob, self.obj = problems.build("brachistochrone", nodes=[90])
        self.program = codegen.trace_problem(self.prob, self.obj)
        self.header = codegen.emit_header(self.program)
        self.points = [np.array(self.prob.p, dtype=float)]
        rng = np.random.default_rng(17)
        self.points += [self.points[0] * (1.0 + 0.02 * rng.standard_normal(self.points[0].size)) for _ in range(2)]
        self.n, self.m = self.program.n, self.program.m


def case(key):
    if key == "B90":
        if key not in dc._CASES:
            dc._CASES[key] = ManyTerms()
        return dc._CASES[key]
    return dc.case(key)


def defect_rows(C):
    """The rows of ``F`` that are collocation defects."""
    rows = []
    for g in C.program.groups:
        if g.kind == "defect":
            for out in g.outputs:
                rows += range(out[0], out[0] + g.length)
    return np.array(sorted(rows), dtype=int)


def weights(C):
    """``[8, m]``: e_0 (the cost row: the gradient of the cost), the last row, all ones, three seeded vectors of unit
    max-norm, the zero vector, a seeded vector with zeros on every defect row."""
    m = C.m
    W = np.zeros((8, m))
    W[0, 0] = W[1, m - 1] = 1.0
    W[2] = 1.0
    rng = np.random.default_rng(29)
    for r in (3, 4, 5, 7):
        w = rng.standard_normal(m)
        W[r] = w / np.abs(w).max()
    W[7, defect_rows(C)] = 0.0
    return W


# ------------------------------------------------------------------------------------------------ the reference
def twin_adjoint(JT, W):
    """``(J^T w [K, n], scale [K, n])`` from the twin's exact ``J_T [n, m]``: the product accumulated in
    ``np.longdouble``, and ``max(1, sum_r |J_rj w_r|)`` per column - the unit of every error here."""
    W = np.atleast_2d(np.asarray(W, dtype=float))
    JL, WL = JT.astype(np.longdouble), W.astype(np.longdouble)
    prod = np.stack([(JL * w[None, :]).sum(axis=1) for w in WL])
    scale = np.stack([np.abs(JL * w[None, :]).sum(axis=1) for w in WL])
    return prod, np.maximum(1.0, scale.astype(float))


def worst_error(G, ref, scale):
    return float(np.max(np.abs(G.astype(np.longdouble) - ref) / scale)) if G.size else 0.0


# ------------------------------------------------------------------------------------------------ the host probe
def build_probe(C, folder, compiler="g++", sanitize=False):
    """tests/adj_probe.cpp against this case's header, with ``parameter_exact_cases.PROBE_FLAGS``: a program of its
    own."""
    header = os.path.join(folder, "og_gen_%s.h" % C.key)
    if not os.path.exists(header):
        with open(header, "w") as fh:
            fh.write(C.header)
    exe = os.path.join(folder, "adj_probe_%s_%s%s" % (C.key, os.path.basename(compiler).replace("+", "x"),
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


def run_probe(C, exe, folder, x, W, theta=None, tag="run", structure=False):
    """-> ``(G[K, n], F0[m])`` of the probe at ``x`` for the rows of ``W``; with ``structure`` also ``terms[n]`` and
    ``reads[n]`` (ints; -1: the variable is no node of a collocated state).  The probe itself fails (exit status 1)
    unless every one of the ``n`` entries of every vector, pre-filled with NaN, is written exactly once and no column
    has two terms in one row."""
    W = np.atleast_2d(np.asarray(W, dtype=np.float64))
    assert W.shape[1] == C.m
    data, out = os.path.join(folder, "%s_%s.in" % (C.key, tag)), os.path.join(folder, "%s_%s.out" % (C.key, tag))
    cv = C.cvec(theta)
    np.concatenate([np.asarray(x, dtype=np.float64), cv if cv.size else np.zeros(1)] +
                   [np.ascontiguousarray(D, dtype=np.float64).reshape(-1) for D in C.prob.D] +
                   [W.reshape(-1)]).tofile(data)
    env = dict(os.environ, UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    proc = subprocess.run([exe, data, out], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, env=env,
                          timeout=300)
    assert proc.returncode == 0 and "runtime error" not in proc.stdout, proc.stdout[-3000:]
    assert "vectors=%d variables=%d " % (W.shape[0], C.n) in proc.stdout and " bad=0" in proc.stdout, proc.stdout[-3000:]
    got = np.fromfile(out)
    K, n, m = W.shape[0], C.n, C.m
    assert got.size == K * n + m + 2 * n
    G, F0 = got[:K * n].reshape(K, n), got[K * n:K * n + m]
    if structure:
        return G, F0, got[K * n + m:K * n + m + n].astype(int), got[K * n + m + n:].astype(int)
    return G, F0


# what the module docstring states, per GPU shape: (columns with more than 256 terms, columns without a term, the
# values of `reads` among its columns)
COVERAGE = {
    "B5": (0, 0, {-1, 0, 1}),
    "G17": (0, 0, {-1, 1}),
    "layout_8": (0, 130, {-1, 0, 1}),
    "P2U": (0, 0, {-1, 1}),
    "B90": (1, 0, {-1, 0, 1}),
    "NL2": (0, 0, {-1, 1, 2}),
    "NL0": (0, 0, {-1, 3}),
}


# what __graft_entry__.build compiles for tests/test_adjoint_gpu.py: (label, header), each with its adjoint part and its
# batch part
def modules():
    return [("adjoint " + key, case(key).header) for key in GPU_KEYS]
