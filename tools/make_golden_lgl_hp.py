#!/usr/bin/env python3
"""High-precision LGL data above the node counts the reference's float64 goldens cover (tests/golden/lgl.npz stops at
N = 200; the engine accepts phases up to ``codegen.max_phase_nodes`` = 1188 nodes).

Build container only (the reference at /root/reference never travels; the tests read the file this writes):

    python tools/make_golden_lgl_hp.py

For every N of ``SIZES`` ``tests/golden/lgl_hp.npz`` gets

* ``tau_N``, ``p_N``: the true LGL nodes and ``P_{N-1}`` at them as double-double pairs ``[2, (N + 1) // 2]`` (row 0 the
  nearest float64, row 1 the float64 nearest to the rest) - the non-negative half in ascending order, from the centre
  outwards to +1; the rule is symmetric (``tau_{N-1-k} = -tau_k``, ``P_{N-1}(-t) = (-1)^{N-1} P_{N-1}(t)``).  mpmath at
  ``PREC`` bits: Newton on ``P'_{N-1}`` by the three-term recurrence, started from
  ``scipy.special.roots_jacobi(N - 2, 1, 1)``, until the step is below 1e-50.
* ``ref_N``: three numbers - what the reference's own float64 construction (``_nodes_LGL``, ``_weight_LGL``,
  ``_differentiation_matrix_LGL``, ``OpenGoddard/optimize.py:183-213``) is off by against that truth: the worst
  absolute node error, the worst relative weight error, the worst relative error of D over the sample of
  ``tests/test_lgl_and_layout.lgl_sample``.  The sampled entries of the reference's D are formed by its own expression
  from its own ``_LegendreFunction`` and ``_nodes_LGL`` (the full matrix costs N^2 calls of ``scipy.special.lpn``; up
  to N = 341 the full matrix is built as well and the sampled entries are checked to be its entries, bit for bit).
"""
import os
import sys

sys.dont_write_bytecode = True
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = "/root/reference"
OUT = os.path.join(REPO, "tests", "golden", "lgl_hp.npz")
sys.path.insert(0, REF)
sys.path.append(REPO)
sys.path.append(os.path.join(REPO, "tests"))

import mpmath                                        # noqa: E402
import numpy as np                                   # noqa: E402
from scipy import special                            # noqa: E402
import OpenGoddard.optimize as ref                   # noqa: E402
from test_lgl_and_layout import LGL_HP_SIZES as SIZES, lgl_sample      # noqa: E402

assert ref.__file__.startswith(REF), ref.__file__
PREC = 256
mp = mpmath.mp


def legendre_pair(n, x):
    p0, p1 = mp.mpf(1), x
    for j in range(1, n):
        p0, p1 = p1, ((2 * j + 1) * x * p1 - j * p0) / (j + 1)
    return p1, p0


def true_half(N):
    """(tau, P_{N-1}(tau)) for the non-negative half, ascending, as mpf lists."""
    n = N - 1
    start = special.roots_jacobi(N - 2, 1, 1)[0]
    half = [float(s) for s in start[(N - 2) // 2:]]           # the non-negative interior roots (with the centre one)
    taus, ps = [], []
    for k, s in enumerate(half):
        if N % 2 == 1 and k == 0:
            x = mp.mpf(0)
        else:
            x = mp.mpf(s)
            for _ in range(60):
                pn, pnm1 = legendre_pair(n, x)
                om = (1 - x) * (1 + x)
                d1 = n * (pnm1 - x * pn) / om
                d2 = (2 * x * d1 - n * (n + 1) * pn) / om
                dx = d1 / d2
                x -= dx
                if abs(dx) < mp.mpf("1e-50"):
                    break
            else:
                raise RuntimeError("Newton did not converge at N = %d, k = %d" % (N, k))
            assert abs(x - s) < 1e-9, (N, k)                 # still the root it was started at
        taus.append(x)
        ps.append(legendre_pair(n, x)[0])
    taus.append(mp.mpf(1))
    ps.append(mp.mpf(1))
    assert len(taus) == (N + 1) // 2
    assert all(b > a for a, b in zip(taus, taus[1:]))
    return taus, ps


def pairs(values):
    hi = np.array([float(v) for v in values])
    lo = np.array([float(v - mp.mpf(h)) for v, h in zip(values, hi)])
    return np.stack([hi, lo])


def full(N, half, odd_sign):
    """The whole rule from its non-negative half (``half[0]`` is the centre node when N is odd)."""
    upper = half[1:] if N % 2 == 1 else half
    lower = [odd_sign * v for v in reversed(upper)]
    return lower + ([half[0]] if N % 2 == 1 else []) + upper


def reference_errors(N, tau, p):
    obj = object.__new__(ref.Problem)
    rt = obj._nodes_LGL(N)
    rw = obj._weight_LGL(N)
    node_err = max(abs(mp.mpf(float(a)) - b) for a, b in zip(rt, tau))
    weight_err = max(abs(mp.mpf(float(a)) / (2 / (N * (N - 1) * q * q)) - 1) for a, q in zip(rw, p))
    rp = [obj._LegendreFunction(t, N - 1) for t in rt]
    rows, cols = lgl_sample(N)
    Dfull = obj._differentiation_matrix_LGL(N) if N <= 341 else None
    worst = mp.mpf(0)
    for i, j in zip(rows.tolist(), cols.tolist()):
        if i == j:
            continue
        d = rp[i] / rp[j] / (rt[i] - rt[j])                   # optimize.py:204-206
        if Dfull is not None:
            assert d == Dfull[i, j]
        true = p[i] / p[j] / (tau[i] - tau[j])
        worst = max(worst, abs(mp.mpf(float(d)) / true - 1))
    return np.array([float(node_err), float(weight_err), float(worst)])


def main():
    mp.prec = PREC
    out = {}
    for N in SIZES:
        taus, ps = true_half(N)
        out["tau_%d" % N] = pairs(taus)
        out["p_%d" % N] = pairs(ps)
        sign = -1 if (N - 1) % 2 else 1
        out["ref_%d" % N] = reference_errors(N, full(N, taus, -1), full(N, ps, sign))
        print(N, out["ref_%d" % N], flush=True)
    np.savez(OUT, **out)
    print(OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
