"""TEST INFRASTRUCTURE - an extended-precision referee for one QP subproblem of the SQP core.

Two solvers of the same strictly convex QP (SciPy's Fortran chain, ``oracle/slsqp_np.py``, ``csrc/ogsqp.hip``)
agree only as far as the conditioning of the subproblem lets them: the first subproblem of the BASELINE
configurations is a *vertex* solution, where a 1e-12 relative perturbation of the Jacobian moves the step by 2e-4
(DESIGN.md section 9).  A tolerance chosen from that argument says nothing about WHICH solver is nearer the exact
step.  This module computes the exact step of the subproblem the solvers were given - the double-precision data taken
as exact - on the active set they report, and so gives both a distance that can be compared.

On the active set the solution of

    min 1/2 d'B d + g'd      rows d + rhs = 0          (B^-1 = Z Z')

is, with d = Z y and T = rows Z, the solution of  y - T'lam = -Z'g,  T y = -rhs.  It is solved once in double
(Householder QR of T', LAPACK) and then refined: the residuals of BOTH equations are evaluated in ``np.longdouble``
(64-bit mantissa, products with ``rows`` and ``Z`` themselves, never with the rounded product T), the correction
comes from the double factorisation.  Each sweep shrinks the error by about cond(T) x 1e-16; the fixed point is
accurate to about cond(T) x 5e-20 - seven or more digits beyond what a double solver can deliver on these problems.
Only ``tests/`` and ``bench.py``'s parity check call this; it is the checker, never the thing measured.
(No reference counterpart: SciPy's ``slsqp`` has no such check; ``scipy/optimize/_slsqp_py.py:427-432`` is the call
whose result this referees.)

:func:`certify` turns the refined solution into a certificate of one solver answer - step, multipliers and the active set
it reports - that fails with the name of the check that broke; :func:`relaxed_subproblem` builds the data of the relaxed
subproblem (n + 1 variables) the way ``include/ogsqp.h`` defines it.
"""
from __future__ import annotations

import numpy as np
from scipy.linalg import solve_triangular

LD = np.longdouble


def active_rows(A, c, lo, hi, m_eq, active, n):
    """The active set as equality rows: ``(rows, rhs)`` with ``rows d + rhs = 0``.  ``A``: m x n general rows
    (``a_j d + c_j``), the first ``m_eq`` always active; ``active``: ids in the numbering of ``og_qp_get_active`` -
    general inequality j (< m_ineq), then ``m_ineq + 2 i`` / ``m_ineq + 2 i + 1`` for the lower / upper bound of
    variable i."""
    m_ineq = A.shape[0] - m_eq
    rows, rhs = [A[:m_eq]], [c[:m_eq]]
    gen = sorted(j for j in active if j < m_ineq)
    if gen:
        rows.append(A[m_eq + np.array(gen)])
        rhs.append(c[m_eq + np.array(gen)])
    for j in sorted(j for j in active if j >= m_ineq):
        i, upper = (j - m_ineq) >> 1, (j - m_ineq) & 1
        e = np.zeros((1, n))                   # d_i - lo_i >= 0  /  hi_i - d_i >= 0: multipliers >= 0 like a general row's
        e[0, i] = -1.0 if upper else 1.0
        rows.append(e)
        rhs.append(np.array([hi[i] if upper else -lo[i]]))
    return np.vstack(rows), np.concatenate(rhs)


def refine(Z, g, rows, rhs, sweeps=6):
    """Exact solution (to about cond x 5e-20) of the equality-constrained QP above.
    -> ``(d, lam, history)``: step, multipliers (``B d + g = rows' lam``) as longdouble arrays; ``history["residuals"]``
    the largest residual entry before each sweep (it falls by orders of magnitude per sweep, then stalls at ~1e-19 x
    the size of the terms that cancel in it - large multipliers raise that floor), ``history["step_moved"]`` how far
    each sweep moved the step: the last entries bound the error of the returned step."""
    Z = np.ascontiguousarray(Z, dtype=np.float64)
    rows = np.ascontiguousarray(rows, dtype=np.float64)
    n, ma = Z.shape[0], rows.shape[0]
    if ma > n:
        raise ValueError("more active rows (%d) than variables (%d): the reported active set is not independent" % (ma, n))
    T = rows @ Z
    Q, R = np.linalg.qr(T.T)                               # T' = Q R,  n x ma, ma x ma
    Zl, Al = Z.astype(LD), rows.astype(LD)
    gl, cl = np.asarray(g, dtype=LD), np.asarray(rhs, dtype=LD)
    ztg = Zl.T @ gl
    y, lam = np.zeros(n, dtype=LD), np.zeros(ma, dtype=LD)
    history, moved, d_prev = [], [], None
    for _ in range(sweeps + 1):
        d = Zl @ y
        if d_prev is not None:
            moved.append(float(np.abs(d - d_prev).max()))
        d_prev = d
        r1 = y + ztg - Zl.T @ (Al.T @ lam)                  # y - T'lam + Z'g
        r2 = Al @ d + cl                                    # T y + rhs
        history.append(float(max(np.abs(r1).max(initial=0.0), np.abs(r2).max(initial=0.0))))
        r1d, r2d = r1.astype(np.float64), r2.astype(np.float64)
        # dy - T'dlam = -r1,  T dy = -r2  with  dy = Q a + w,  w orthogonal to range(Q)
        a = -solve_triangular(R, r2d, trans="T")
        qr1 = Q.T @ r1d
        dlam = solve_triangular(R, a + qr1)
        dy = Q @ a - (r1d - Q @ qr1)
        y = y + dy.astype(LD)
        lam = lam + dlam.astype(LD)
    d = Zl @ y
    moved.append(float(np.abs(d - d_prev).max()))
    return d, lam, {"residuals": history, "step_moved": moved}


def distances(Z, g, A, c, lo, hi, m_eq, active, steps, sweeps=6):
    """Distance of each candidate step in ``steps`` (dict name -> d) to the refined solution on ``active``,
    relative to max(1, |d*|_inf).  -> ``(dict name -> distance, d*, info)``."""
    n = Z.shape[0]
    rows, rhs = active_rows(A, c, lo, hi, m_eq, active, n)
    d_star, lam, history = refine(Z, g, rows, rhs, sweeps)
    scale = max(1.0, float(np.abs(d_star).max()))
    out = {k: float(np.abs(np.asarray(v, dtype=LD)[:n] - d_star).max() / scale) for k, v in steps.items()}
    info = {"active_rows": int(rows.shape[0]), "residual_history": history["residuals"],
            "step_moved": [v / scale for v in history["step_moved"]],
            "min_multiplier_of_inequalities": float(lam[m_eq:].min()) if rows.shape[0] > m_eq else None}
    return out, d_star, info


def relaxed_subproblem(Z, g, A, c, lo, hi, m_eq, rho):
    """The relaxed subproblem of slsqp label 140-150 (``og_qp_solve_dev(augmented=1, rho)``) as plain data in n + 1
    variables, in the form :func:`distances` and :func:`certify` take: the last column of ``A`` is
    ``[-c_eq, max(-c_ineq, 0)]`` (``a_j d + c_j (1 - delta) = 0``, ``a_j d + c_j + max(-c_j, 0) delta >= 0``),
    ``Z[n, n] = 1 / rho``, the relaxation variable delta bounded by [0, 1].  -> ``(Z, g, A, c, lo, hi)``."""
    n = Z.shape[0]
    Za = np.zeros((n + 1, n + 1))
    Za[:n, :n] = Z
    Za[n, n] = 1.0 / rho
    extra = np.concatenate([-np.asarray(c[:m_eq], dtype=np.float64), np.maximum(-np.asarray(c[m_eq:], dtype=np.float64), 0.0)])
    return (Za, np.append(g, 0.0), np.hstack([A, extra[:, None]]), np.asarray(c, dtype=np.float64),
            np.append(lo, 0.0), np.append(hi, 1.0))


class CertificateError(AssertionError):
    """:func:`certify` refused an answer.  ``failed``: the names of the checks that broke ("status", "active set",
    "referee", "step", "dual feasibility", "primal feasibility", "multipliers"); ``measured``: what was measured."""

    def __init__(self, failed, measured, details):
        self.failed, self.measured = list(failed), dict(measured)
        super().__init__("certificate refused: " + "; ".join(details))


def certify(Z, g, A, c, lo, hi, m_eq, status, d, mult, bound_mult, active, tol_d=1e-9, tol_mu=1e-7, tol_p=1e-7,
            tol_conv=1e-13, sweeps=6):
    """Certify one answer of a QP solver against the refined solution on the active set it reports.

    Data as :func:`distances` takes it (``A``: the ``m_eq`` equality rows first; for the relaxed subproblem build it with
    :func:`relaxed_subproblem`); ``status``, ``d``, ``mult`` (m), ``bound_mult`` (n) as ``og_qp_solve`` returns them
    (``grad L = B d + g - A' mult - bound_mult``, ``bound_mult > 0`` where a lower bound is active, ``< 0`` an upper one:
    ``include/ogsqp.h``); ``active`` in the numbering of ``og_qp_get_active``.  The checks, each relative to a scale:

    * referee converged - the last two sweeps moved d* by at most ``tol_conv`` x max(1, |d*|_inf); otherwise the
      certificate is void (the referee cannot vouch for anything);
    * step - ``|d - d*|_inf <= tol_d`` x max(1, |d*|_inf);
    * dual feasibility - every multiplier of an active inequality or bound in lambda* ``>= -tol_mu`` x max(1, |lambda*|_inf);
    * primal feasibility - at d*, every general inequality and every finite bound holds within ``tol_p`` x max(1, |c|_inf);
    * multipliers - ``mult`` and ``bound_mult`` equal lambda* in their slots (zero where nothing is active) within
      ``tol_mu`` x max(1, |lambda*|_inf).

    -> dict of the measured (relative) values; raises :class:`CertificateError` naming every check that broke."""
    n, m = Z.shape[0], A.shape[0]
    m_ineq = m - m_eq
    d, mult, bound_mult = (np.asarray(v, dtype=np.float64) for v in (d, mult, bound_mult))
    if status != 1:
        raise CertificateError(["status"], {}, ["status: %d, not a solution (1)" % status])
    if d.shape != (n,) or mult.shape != (m,) or bound_mult.shape != (n,):
        raise ValueError("d, mult, bound_mult: expected %d, %d, %d entries, got %s, %s, %s" % (
            n, m, n, d.shape, mult.shape, bound_mult.shape))
    active = sorted(int(j) for j in active)
    if len(set(active)) != len(active) or any(j < 0 or j >= m_ineq + 2 * n for j in active):
        raise CertificateError(["active set"], {}, ["active set: repeated or out-of-range ids"])
    try:
        rows, rhs = active_rows(A, c, lo, hi, m_eq, active, n)
        d_star, lam, history = refine(Z, g, rows, rhs, sweeps)
    except ValueError as exc:
        raise CertificateError(["active set"], {}, ["active set: %s" % exc])
    scale = max(1.0, float(np.abs(d_star).max()))
    referee = max(history["step_moved"][-2:]) / scale
    measured = {"active_rows": int(rows.shape[0]), "referee": referee}
    if not referee <= tol_conv:
        raise CertificateError(["referee"], measured, [
            "referee: the refinement did not converge (its last sweeps moved d* by %.2e x max(1, |d*|) > %.0e): the "
            "certificate is void" % (referee, tol_conv)])
    failed, details = [], []

    def check(name, ok, text):
        if not ok:
            failed.append(name)
            details.append(name + ": " + text)

    # step
    measured["step"] = float(np.abs(d.astype(LD) - d_star).max()) / scale
    check("step", measured["step"] <= tol_d, "|d - d*| = %.2e x max(1, |d*|) > tol_d %.0e" % (measured["step"], tol_d))
    # dual feasibility: lambda* of the active inequalities and bounds
    lam64 = lam.astype(np.float64)
    mscale = max(1.0, float(np.abs(lam64).max(initial=0.0)))
    least = float(lam64[m_eq:].min()) / mscale if rows.shape[0] > m_eq else 0.0
    measured["dual"] = least
    check("dual feasibility", least >= -tol_mu,
          "a multiplier of an active inequality is %.2e x max(1, |lambda*|) < -tol_mu %.0e" % (least, tol_mu))
    # primal feasibility at d*: every general inequality, every finite bound
    pscale = max(1.0, float(np.abs(np.asarray(c, dtype=np.float64)).max(initial=0.0)))
    worst = 0.0
    if m_ineq:
        vals = A[m_eq:].astype(LD) @ d_star + np.asarray(c[m_eq:], dtype=LD)
        worst = max(worst, float(-vals.min()))
    lo, hi = np.asarray(lo, dtype=np.float64), np.asarray(hi, dtype=np.float64)
    for bound, sign in ((lo, 1.0), (hi, -1.0)):
        fin = np.isfinite(bound)
        if fin.any():
            worst = max(worst, float((-sign * (d_star[fin] - bound[fin].astype(LD))).max()))
    measured["primal"] = max(worst, 0.0) / pscale
    check("primal feasibility", measured["primal"] <= tol_p,
          "a constraint is violated at d* by %.2e x max(1, |c|) > tol_p %.0e" % (measured["primal"], tol_p))
    # multipliers, mapped to the solver's slots (the order of active_rows: equalities, general rows, bounds)
    want_mult, want_bm = np.zeros(m), np.zeros(n)
    want_mult[:m_eq] = lam64[:m_eq]
    general = [j for j in active if j < m_ineq]
    bounds = [j for j in active if j >= m_ineq]
    want_mult[m_eq + np.array(general, dtype=int)] = lam64[m_eq:m_eq + len(general)]
    for j, v in zip(bounds, lam64[m_eq + len(general):]):
        i, upper = (j - m_ineq) >> 1, (j - m_ineq) & 1
        want_bm[i] += -v if upper else v
    measured["multipliers"] = max(float(np.abs(mult - want_mult).max(initial=0.0)),
                                  float(np.abs(bound_mult - want_bm).max(initial=0.0))) / mscale
    check("multipliers", measured["multipliers"] <= tol_mu,
          "|(mult, bound_mult) - lambda*| = %.2e x max(1, |lambda*|) > tol_mu %.0e" % (measured["multipliers"], tol_mu))
    if failed:
        raise CertificateError(failed, measured, details)
    return measured
