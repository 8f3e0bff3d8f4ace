"""The cases of tests/test_hessian_matrix.py and tests/test_hessian_matrix_gpu.py (and of ``__graft_entry__.build``, which
compiles the GPU cases' modules, batch parts, Hessian parts and Hessian-matrix parts ahead of the GPU run): the plan
(``codegen.HessianPlan``) of every shape and the host probe of ``csrc/og_hess.h``.

Shapes, points and parameter sets are those of ``hessian_cases.GPU_KEYS`` (``B5``, ``G17``, ``layout_8``, ``P2U``, ``NL2``,
``NL0``, ``B90``), the weights ``adjoint_cases.weights``.  The reference of the bit-for-bit tests is the existing probe of
``csrc/og_hvp.h`` (``hessian_cases.run_probe``) with the ``n`` unit directions.
"""
import os

import numpy as np

import hessian_cases as hc
from opengoddard_amd import codegen

ROOT = hc.ROOT
PROBE_SOURCE = os.path.join(ROOT, "tests", "hess_probe.cpp")
BOUND = hc.BOUND                # 1e-12: the project's bound for exact modes (the symmetry test)

GPU_KEYS = hc.GPU_KEYS
SURFACE_KEYS, GPU_SURFACE_KEYS = hc.SURFACE_KEYS, hc.GPU_SURFACE_KEYS      # tests/test_hessian_surface*.py
case = hc.case
weights = hc.ac.weights

_PLANS = {}


def plan(C):
    """The case's ``codegen.HessianPlan``, computed once."""
    if C.key not in _PLANS:
        _PLANS[C.key] = codegen.HessianPlan(C.program)
    return _PLANS[C.key]


def pairs_of(hp):
    """``(row[nnz], col[nnz], owner[nnz], partner[nnz])`` of the stored entries, in pattern order."""
    indptr, cols, owner = (np.asarray(a) for a in (hp.indptr, hp.cols, hp.owner))
    row = np.repeat(np.arange(hp.n), np.diff(indptr))
    partner = np.where(owner == row, cols, row)
    return row, cols, owner, partner


def build_probe(C, folder, compiler="g++", sanitize=False):
    """tests/hess_probe.cpp against this case's header: a program of its own."""
    header = os.path.join(folder, "og_gen_%s.h" % C.key)
    if not os.path.exists(header):
        with open(header, "w") as fh:
            fh.write(C.header)
    exe = hc._exe(folder, "hess_probe_" + C.key, compiler, sanitize)
    if os.path.exists(exe):
        return exe
    return hc._compile(PROBE_SOURCE, exe, compiler, sanitize, ["-DOG_GEN_HEADER=\"%s\"" % header])


class Probed:
    """What one run of the probe returns: ``H[K, nnz]`` (the stored entries in pattern order), ``S[K, nnz]`` (the sum of
    ``|w_r d2F_r/dx_owner dx_partner|`` over the entry's listed terms), ``F0[m]`` and ``terms[n]``."""


def probe_input(C, x, W, theta=None, arrays=None):
    """The probe's input file as one array of doubles (``arrays``: a plan other than the case's own)."""
    W = np.atleast_2d(np.asarray(W, dtype=np.float64))
    indptr, cols, owner, tptr, tlist = arrays if arrays is not None else plan(C).arrays()
    nnz, ntl = int(indptr[-1]), int(tptr[-1])
    cv = C.cvec(theta)
    return np.concatenate([np.asarray(x, dtype=np.float64), cv if cv.size else np.zeros(1)] +
                          [np.ascontiguousarray(D, dtype=np.float64).reshape(-1) for D in C.prob.D] +
                          [np.array([nnz, ntl, W.shape[0]], dtype=np.float64)] +
                          [np.asarray(a, dtype=np.float64) for a in (indptr, cols[:nnz], owner[:nnz], tptr, tlist[:max(ntl, 1)])] +
                          [W.reshape(-1)])


def run_probe(C, exe, folder, x, W, theta=None, tag="hess"):
    """The probe at ``x`` for the rows of ``W``.  The probe itself fails (exit status 1) unless the plan is well formed
    and every stored entry of every vector, pre-filled with NaN, is written exactly once."""
    W = np.atleast_2d(np.asarray(W, dtype=np.float64))
    K, n, m, nnz = W.shape[0], C.n, C.m, plan(C).nnz
    assert W.shape == (K, m)
    data, out = os.path.join(folder, "%s_%s.in" % (C.key, tag)), os.path.join(folder, "%s_%s.out" % (C.key, tag))
    probe_input(C, x, W, theta).tofile(data)
    text = hc._run([exe, data, out])
    assert "vectors=%d entries=%d " % (K, nnz) in text and " bad=0" in text, text[-3000:]
    got = np.fromfile(out)
    assert got.size == 2 * K * nnz + m + n
    r = Probed()
    r.H, r.S = got[:K * nnz].reshape(K, nnz), got[K * nnz:2 * K * nnz].reshape(K, nnz)
    r.F0 = got[2 * K * nnz:2 * K * nnz + m]
    r.terms = got[2 * K * nnz + m:].astype(int)
    return r


def unit_products(C, exe, folder, x, W, theta=None, tag="unit"):
    """``(Q[K, n, n], S[K, n, n])`` from the probe of ``csrc/og_hvp.h``: ``Q[d, l, j] = hvp(W[d], e_l)[j]`` and the
    sum of the absolute values of its terms, every weight vector with all ``n`` unit directions."""
    W = np.atleast_2d(np.asarray(W, dtype=np.float64))
    K, n = W.shape[0], C.n
    r = hc.run_probe(C, exe, folder, x, np.repeat(W, n, axis=0), np.tile(np.eye(n), (K, 1)), theta, tag=tag)
    return r.Q.reshape(K, n, n), r.S.reshape(K, n, n)


# ------------------------------------------------------------------------------------------------ probes built ahead
# The g++ probes of the surface shapes take up to half a minute to compile (wide_reductions: a header of 407 variables) and
# that problem's sanitizer builds four minutes each with clang++; ``__graft_entry__.build`` compiles them into
# ``adjoint_cases.prebuilt_folder`` so that tests/test_hessian_surface_gpu.py, tests/test_hessian_surface.py and
# tests/test_adjoint.py only run them.
prebuilt_folder, probe_folder = hc.ac.prebuilt_folder, hc.ac.probe_folder


def probe_jobs():
    """One callable per probe ``__graft_entry__.build`` compiles ahead."""
    def job(key, build, compiler, sanitize):
        def run():
            C = case(key)
            folder = prebuilt_folder(C)
            os.makedirs(folder, exist_ok=True)
            for entry in os.listdir(hc.ac.PREBUILT):    # an older revision's
                if entry.startswith(key + "_") and entry != os.path.basename(folder):
                    import shutil
                    shutil.rmtree(os.path.join(hc.ac.PREBUILT, entry), ignore_errors=True)
            return build(C, folder, compiler, sanitize)
        return run
    jobs = [job(key, build, hc.ac.sanitizer_compiler(key), True) for key in hc.ac.SANITIZE_WITH_CLANG
            for build in (hc.build_probe, build_probe, hc.ac.build_probe)]         # the long ones first
    return jobs + [job(key, build, "g++", False) for key in GPU_SURFACE_KEYS for build in (hc.build_probe, build_probe)]


# what __graft_entry__.build compiles for tests/test_hessian_matrix_gpu.py and tests/test_hessian_surface_gpu.py: (label,
# header), each with its Hessian-matrix part, its Hessian part (the unit-direction check) and its batch part
def modules():
    return [("hessian matrix " + key, case(key).header) for key in GPU_KEYS + GPU_SURFACE_KEYS]
