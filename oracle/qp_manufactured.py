"""TEST INFRASTRUCTURE - QP subproblems of the SQP core built backwards from their answer, with exact data.

``qp_referee.refine`` needs a ``longdouble`` copy of Z and a QR of the active rows: at rows of 16384 entries that is
minutes per answer.  Here the answer comes first and the data is derived from it, at the cost of two products with the
constraint matrix: choose the step ``d*``, the multipliers ``r*`` (free sign on the equalities, >= 0.25 on the active
general rows, 0 elsewhere) and the bound multipliers ``bm*`` (>= 0.25 lower-active, <= -0.25 upper-active, 0 elsewhere),
then, in the convention of ``include/ogsqp.h`` (``B d + g - A'r - bound_mult = 0``),

    c_eq = -C d*                      h_active = -G_a d*          h_inactive = -G_i d* + slack,  slack >= 0.25
    g    = A'r* + bm* - B d*          dl_i = d*_i (lower-active)  du_i = d*_i (upper-active)
    every other bound: at least 0.25 away from d*_i, or infinite

These are the KKT conditions of a strictly convex QP with strict complementarity: ``(d*, r*, bm*)`` and the active set
are its unique answer as long as the active rows are independent (generic data with ``m_eq + active <= n``).

The data is exact, not merely accurate.  The entries of ``A = [C; G]`` are a standard normal sample rounded to multiples
of 2^-6 and clipped to +-8; ``d*``, ``r*``, ``bm*``, the slacks and the gaps to the inactive bounds are multiples of 2^-6
of size <= 2 (multipliers <= 1); ``Z = diag(z)`` with ``z_i`` in {0.5, 1, 2}, so ``B = diag(1 / z_i^2)`` has the entries
4, 1, 0.25.  ``c``, ``h`` and ``g`` are formed in ``int64`` arithmetic on the scaled integers and divided by a power of two
once: every sum has far fewer than 53 bits (the builder asserts its bound), so the doubles handed to a solver ARE the data
of a QP whose exact solution is ``d*``.  No tolerance is spent on the reference.

The relaxed kind (``og_qp_solve_dev(augmented=1, rho)``; its data as ``qp_referee.relaxed_subproblem`` defines it) uses the
same ``A``, ``d*``, bounds and multipliers with ``delta* = 0.5`` interior (``bm_delta = 0``): ``c_eq = -2 C d*``; for an
inequality row with ``t = slack - G d*`` (slack 0 on an active row) ``h = 2 t`` where ``t < 0``, else ``h = t`` - exact like
the plain kind's.  The delta row of stationarity, ``rho^2 delta* = extra . r*`` with ``extra = [-c_eq, max(-h, 0)]``,
cannot be met through ``g`` (the API fixes g's delta entry at 0): it is met by solving for ONE multiplier - of the equality
with the largest ``|c_j|``, or without equalities of the active general row with the most negative ``h`` (which must
come out >= 0.25).  That multiplier is a correctly rounded quotient of exact numbers, and its row's share of ``g`` is
added in ``longdouble`` (the product of a 10-bit and a 53-bit number is exact there) and rounded once per entry: the
relaxed data is within one rounding of ``g`` and of one multiplier of an exact QP, not exact.  tests/test_qp_wide_rows.py
measures what that is worth against the referee (the step moves by less than 4e-15 at n = 24 to 60).

:func:`compare` is the check of one solver answer against the builder's: status, active set, step, multipliers, exact
zeros on the inactive slots, ``0 < delta < 1``.  No reference counterpart (SciPy's ``lsq`` is handed whatever the NLP
gives, ``scipy/optimize/_slsqp_py.py:427-432``).
"""
from __future__ import annotations

import numpy as np

SCALE = 64                      # every chosen number is an integer over 2^6
CLIP = 8 * SCALE                # |A_ij| <= 8
QUARTER = SCALE // 4            # the least multiplier, slack and gap: 0.25
SIZE = 2 * SCALE                # the largest: 2
CHUNK = 512                     # rows of A' per partial product


def _int_times(AT, vec, transposed):
    """Exact ``A vec`` (``transposed``: ``A' vec``) in int64 for ``AT = A'`` (n x m, int16), ``vec`` int64."""
    n, m = AT.shape
    out = np.zeros(n if transposed else m, dtype=np.int64)
    for lo in range(0, n, CHUNK):
        block = AT[lo:lo + CHUNK]                               # (int16 x int64 -> int64 products, int64 sums)
        if transposed:
            out[lo:lo + CHUNK] = np.einsum("ij,j->i", block, vec)
        else:
            out += np.einsum("i,ij->j", vec[lo:lo + CHUNK], block)
    return out


class ManufacturedQP:
    """One matrix, one answer, two kinds of subproblem.  Fields: ``n, meq, mg, m``; ``AT`` (n x m, int16: ``A' * 64``);
    ``z`` (the diagonal of Z); ``lb, ub`` (n); ``active`` (sorted ids in the numbering of ``og_qp_get_active``);
    ``zero_mult`` (m) / ``zero_bm`` (n): the slots of inactive rows and bounds; per kind
    ``"plain"`` / ``"relaxed"`` in ``self.kinds``: ``g`` (n), ``c`` (m), ``d`` (the step: n, or n + 1 with delta last),
    ``mult`` (m), ``bm`` (like d), ``rho``."""

    def factor(self):
        return np.diag(self.z)

    def matrix(self):
        """A as doubles, m x n (small cases; the device is handed ``AT``: tests/test_qp_wide_rows.py, ``device_rows``)."""
        return np.ascontiguousarray(self.AT.T, dtype=np.float64) / SCALE

    def data(self, kind):
        """``(Z, g, A, c, lb, ub, meq)`` in the form ``qp_referee.certify`` / ``distances`` take (the relaxed kind through
        ``qp_referee.relaxed_subproblem``)."""
        from oracle import qp_referee
        k = self.kinds[kind]
        base = (self.factor(), k["g"], self.matrix(), k["c"], self.lb, self.ub)
        if kind == "relaxed":
            base = qp_referee.relaxed_subproblem(*base, self.meq, k["rho"])
        return (*base, self.meq)

    def bounds(self, kind):
        if kind == "relaxed":
            return np.append(self.lb, 0.0), np.append(self.ub, 1.0)
        return self.lb, self.ub


def manufacture(seed, n, meq, mg, active_general, lower, upper, rho=100.0):
    """-> :class:`ManufacturedQP` with ``active_general`` of the ``mg`` general rows active, ``lower`` / ``upper``
    variables at their lower / upper bound, a third of the other variables without bounds."""
    assert meq + active_general + lower + upper <= n and active_general <= mg and lower + upper <= n
    rng = np.random.default_rng(seed)
    m = meq + mg
    qp = ManufacturedQP()
    qp.n, qp.meq, qp.mg, qp.m = n, meq, mg, m
    sample = rng.standard_normal((n, m), dtype=np.float32)
    sample *= SCALE
    np.rint(sample, out=sample)
    np.clip(sample, -CLIP, CLIP, out=sample)
    AT = qp.AT = sample.astype(np.int16)
    del sample

    def whole(lo, hi, size):                                   # integers over 2^6 in [lo, hi]
        return rng.integers(lo, hi + 1, size=size, dtype=np.int64)

    D = whole(-SIZE, SIZE, n)                                  # d* in [-2, 2]
    zexp = rng.integers(-1, 2, size=n)                         # z = 2^zexp; 1 / z^2 = W / 4, W in {16, 4, 1}
    qp.z = np.ldexp(1.0, zexp)
    W = np.array([16, 4, 1], dtype=np.int64)[zexp + 1]
    R = np.zeros(m, dtype=np.int64)
    R[:meq] = whole(1, SCALE, meq) * rng.choice(np.array([-1, 1], dtype=np.int64), size=meq)
    general = np.sort(rng.choice(mg, size=active_general, replace=False))
    R[meq + general] = whole(QUARTER, SCALE, active_general)
    at_bound = rng.choice(n, size=lower + upper, replace=False)
    low, up = np.sort(at_bound[:lower]), np.sort(at_bound[lower:])
    BM = np.zeros(n, dtype=np.int64)
    BM[low] = whole(QUARTER, SCALE, lower)
    BM[up] = -whole(QUARTER, SCALE, upper)
    slack = whole(QUARTER, SIZE, mg)
    slack[general] = 0
    # bounds: the active ones at d*, the others a gap away; a third of the variables that are at no bound have none
    lo_gap, hi_gap = whole(QUARTER, SIZE, n), whole(QUARTER, SIZE, n)
    lo_gap[low], hi_gap[up] = 0, 0
    qp.lb, qp.ub = (D - lo_gap) / SCALE, (D + hi_gap) / SCALE
    rest = np.setdiff1d(np.arange(n), at_bound)
    unbounded = rest[rng.uniform(size=rest.size) < 1.0 / 3.0]
    qp.lb[unbounded], qp.ub[unbounded] = -np.inf, np.inf
    qp.zero_mult = np.ones(m, dtype=bool)                      # the slots a solver must leave at exactly 0.0
    qp.zero_mult[:meq], qp.zero_mult[meq + general] = False, False
    qp.zero_bm = np.ones(n, dtype=bool)
    qp.zero_bm[at_bound] = False
    qp.active = sorted([int(j) for j in general] + [mg + 2 * int(i) for i in low] + [mg + 2 * int(i) + 1 for i in up])
    # every sum below is an integer of fewer than 53 bits: (terms) x |A| x |d*, r*| plus the single terms
    largest = max(n, m) * CLIP * SIZE + SCALE * SIZE * 2 + 16 * 16 * SIZE
    assert 2 * largest < 2 ** 52, largest
    assert np.abs(AT).max() <= CLIP and max(np.abs(D).max(), np.abs(R).max(), np.abs(BM).max()) <= SIZE

    AD = _int_times(AT, D, False)                              # A d* * 2^12
    unit = SCALE * SCALE
    # ---- plain
    c = -AD
    c[meq:] += SCALE * slack
    G_int = _int_times(AT, R, True) + SCALE * BM - 16 * W * D  # (A'r* + bm* - B d*) * 2^12
    assert max(np.abs(c).max(initial=0), np.abs(G_int).max()) <= largest
    mult = R / SCALE
    qp.kinds = {"plain": {"g": G_int / unit, "c": c / unit, "d": D / SCALE, "mult": mult, "bm": BM / SCALE, "rho": rho}}
    # ---- relaxed: delta* = 1/2
    t = SCALE * slack - AD[meq:]
    cr = np.concatenate([-2 * AD[:meq], np.where(t < 0, 2 * t, t)])
    extra = np.concatenate([-cr[:meq], np.maximum(-cr[meq:], 0)])             # * 2^12
    if meq:
        pivot = int(np.argmax(np.abs(cr[:meq])))
    else:
        pivot = meq + int(general[np.argmax(extra[meq + general])])
    assert extra[pivot] != 0, "the relaxed kind needs a row with c_j != 0 to carry the delta row of stationarity"
    Rr = R.copy()
    Rr[pivot] = 0
    # rho^2 delta* = extra . r*:  r_pivot = (rho^2 / 2 - sum of the others) / extra_pivot, numerator and denominator exact
    half_rho2 = rho * rho / 2.0
    assert half_rho2 == int(half_rho2)
    numerator = int(half_rho2) * unit * SCALE - int(extra @ Rr)               # * 2^18
    r_pivot = numerator / (SCALE * int(extra[pivot]))                         # (int / int: correctly rounded)
    assert pivot < meq or r_pivot >= 0.25, r_pivot
    S = G_int - AT[:, pivot].astype(np.int64) * R[pivot]                      # (the pivot row's share goes in rounded)
    LD = np.longdouble
    g_relaxed = (S.astype(LD) / unit + (AT[:, pivot].astype(LD) / SCALE) * LD(r_pivot)).astype(np.float64)
    mult_r = Rr / SCALE
    mult_r[pivot] = r_pivot
    qp.kinds["relaxed"] = {"g": g_relaxed, "c": cr / unit, "d": np.append(D / SCALE, 0.5), "mult": mult_r,
                           "bm": np.append(BM / SCALE, 0.0), "rho": rho, "pivot": pivot}
    return qp


class ManufacturedError(AssertionError):
    """:func:`compare` refused an answer.  ``failed``: the names of the checks that broke ("status", "active set",
    "step", "multipliers", "inactive multipliers", "delta"); ``measured``: what was measured."""

    def __init__(self, failed, measured, details):
        self.failed, self.measured = list(failed), dict(measured)
        super().__init__("not the manufactured answer: " + "; ".join(details))


def compare(qp, kind, status, d, mult, bm, active, tol_d, tol_mu):
    """One solver answer against the builder's.  The checks:

    * status - 1;
    * active set - ``active`` (the numbering of ``og_qp_get_active``) is exactly the builder's;
    * step - ``|d - d*|_inf <= tol_d`` x max(1, |d*|_inf), and every entry finite;
    * multipliers - ``mult`` and ``bm`` within ``tol_mu`` x max(1, |r*|_inf, |bm*|_inf) of ``r*`` and ``bm*``;
    * inactive multipliers - exactly 0.0 wherever the builder's are (rows and bounds outside the active set);
    * delta (relaxed kind) - ``0 < d[n] < 1``.

    -> ``{"step", "multipliers"}`` (relative, as above); raises :class:`ManufacturedError` naming every check that broke."""
    want = qp.kinds[kind]
    d, mult, bm = (np.asarray(v, dtype=np.float64) for v in (d, mult, bm))
    if status != 1:
        raise ManufacturedError(["status"], {}, ["status: %d, not a solution (1)" % status])
    if d.shape != want["d"].shape or mult.shape != want["mult"].shape or bm.shape != want["bm"].shape:
        raise ValueError("d, mult, bm: expected %s, %s, %s entries, got %s, %s, %s" % (
            want["d"].shape, want["mult"].shape, want["bm"].shape, d.shape, mult.shape, bm.shape))
    failed, details, measured = [], [], {}

    def check(name, ok, text):
        if not ok:
            failed.append(name)
            details.append(name + ": " + text)

    got = sorted(int(j) for j in active)
    check("active set", got == qp.active, "%d rows missing, %d rows too many (first: %s / %s)" % (
        len(set(qp.active) - set(got)), len(set(got) - set(qp.active)),
        sorted(set(qp.active) - set(got))[:3], sorted(set(got) - set(qp.active))[:3]))
    scale = max(1.0, float(np.abs(want["d"]).max()))
    with np.errstate(invalid="ignore"):
        measured["step"] = float(np.abs(d - want["d"]).max()) / scale
        mscale = max(1.0, float(np.abs(want["mult"]).max(initial=0.0)), float(np.abs(want["bm"]).max()))
        measured["multipliers"] = max(float(np.abs(mult - want["mult"]).max(initial=0.0)),
                                      float(np.abs(bm - want["bm"]).max())) / mscale
    check("step", measured["step"] <= tol_d, "|d - d*| = %.2e x max(1, |d*|) > tol_d %.0e" % (measured["step"], tol_d))
    check("multipliers", measured["multipliers"] <= tol_mu,
          "|(mult, bm) - (r*, bm*)| = %.2e x max(1, |r*|, |bm*|) > tol_mu %.0e" % (measured["multipliers"], tol_mu))
    zero_bm = np.append(qp.zero_bm, True) if kind == "relaxed" else qp.zero_bm
    stray = int(np.count_nonzero(mult[qp.zero_mult])) + int(np.count_nonzero(bm[zero_bm]))
    check("inactive multipliers", stray == 0, "%d multipliers of inactive rows or bounds are not exactly 0.0" % stray)
    if kind == "relaxed":
        check("delta", 0.0 < d[qp.n] < 1.0, "delta = %r is not inside (0, 1)" % d[qp.n])
    if failed:
        raise ManufacturedError(failed, measured, details)
    return measured
