"""The quasi-Newton factor ``Z`` (``B^-1 = Z Z'``) through the two places that change it: the QP solve, which leaves
``Z Q``, and the Powell-damped BFGS update in product form.

A wrong entry of ``Z`` raises no error and moves no step of the subproblem that produced it: the tests of the LQ forms
compare ``d`` and the multipliers.  Here the factor itself is read back and measured.  Every reference is plain NumPy in
``np.longdouble`` (eps_L = 1.08e-19 where long double is the x87 format) and calls neither the function under test nor
its restatement; every bound is either derived in the docstring that asserts it or is 10 x what the restatement
(``oracle/slsqp_np.py``, LAPACK's LQ) measures on the same data, floored at 2^-52 - the margin this suite gives the core
over the restatement elsewhere.  u = 2^-53 below.

1. CPU: ``slsqp_np.bfgs_factor_update`` IS damped BFGS - against the textbook recursion on ``B`` in longdouble.
2. GPU: ``og_qp_bfgs`` at every workgroup and row-pitch edge, against the product formula in longdouble.
3. GPU: the factor a solve leaves, in every form of the LQ sweep; CPU: the two metrics refuse wrong factors.
4. GPU: solve -> BFGS -> solve ... as the driver chains them, against ``B_k`` carried in longdouble.
5. GPU: ``og_jt_times`` on widths and paddings of its own."""
import functools

import numpy as np
import pytest

from conftest import record_measurement
from oracle import slsqp_np
from opengoddard_amd import _sqp_native
from test_slsqp_core import random_qp

LD = np.longdouble
EPS_L = float(np.finfo(LD).eps)
U = 2.0 ** -53
FLOOR = 2.0 ** -52
FORM_KEYS = ("OGSQP_RESIDENT", "OGSQP_GI", "OGSQP_LQ", "OGSQP_TRSV", "OGSQP_WIDE", "OGSQP_SPIN_LIMIT", "OGSQP_WARM",
             "OGSQP_ROWS", "OGSQP_WARM_SPREAD", "OGSQP_WIDE_AHEAD", "OGSQP_WIDE_INBLOCK")


@pytest.fixture
def default_forms(monkeypatch):
    """The handles of a test are made with the default forms, whatever the suite's environment selects."""
    for key in FORM_KEYS:
        monkeypatch.delenv(key, raising=False)
    return monkeypatch


def ld(a):
    return np.asarray(a, dtype=LD)


# ------------------------------------------------------------------------------------------- longdouble references
def inverse_ld(A):
    """``A^-1`` in longdouble: the double inverse refined by Newton-Schulz steps ``X <- X + X (I - A X)`` (quadratic
    from a residual of cond * u; what is left is the rounding of the last step)."""
    A = ld(A)
    X = ld(np.linalg.inv(A.astype(np.float64)))
    eye = np.eye(A.shape[0], dtype=LD)
    for _ in range(3):
        X = X + X @ (eye - A @ X)
    return X


def branch_in_double(s, eta, Bs):
    """The branch the code under test takes: ``s'eta < 0.2 s'Bs`` with both sums in double - in the order of the core's
    host loop and in NumPy's.  The inputs of these tests are chosen so that the two orders decide alike (asserted)."""
    h1 = h2 = 0.0
    for a, b, c in zip(s.tolist(), eta.tolist(), Bs.tolist()):
        h1 += a * b
        h2 += a * c
    damped = h1 < 0.2 * h2
    assert damped == (float(s @ eta) < 0.2 * float(s @ Bs)), "the input sits where the order of a sum picks the branch"
    return damped


def update_ld(Z, s, eta, Bs, damped):
    """The product formula ``Z+ = Z - s ((r - alpha Bs)'Z) / (alpha^2 h2)`` in longdouble, on the branch given.
    -> ``Z+`` and the scalars and ``r`` that the bounds below are made of."""
    Z, s, eta, Bs = ld(Z), ld(s), ld(eta), ld(Bs)
    h1, h2 = s @ eta, s @ Bs
    theta = LD(1)
    if damped:
        theta = LD(4) * h2 / (LD(5) * (h2 - h1))
        h1 = h2 / LD(5)
    r = theta * eta + (LD(1) - theta) * Bs
    alpha = np.sqrt(h1 / h2)
    Zp = Z - np.outer(s, (r - alpha * Bs) @ Z) / (alpha * alpha * h2)
    return Zp, {"theta": float(theta), "alpha": float(alpha), "h1": float(h1), "h2": float(h2), "r": r}


def textbook_bfgs_ld(B, s, eta, damped):
    """Damped BFGS on ``B`` itself, in longdouble: ``B+ = B - (Bs)(Bs)'/h2 + r r'/(s'r)``, ``r = theta eta + (1 - theta) Bs``,
    ``theta = 0.8 h2 / (h2 - h1)`` on the damped branch, else 1 (Powell 1978; Nocedal & Wright, Procedure 18.2)."""
    B, s, eta = ld(B), ld(s), ld(eta)
    Bs = B @ s
    h1, h2 = s @ eta, s @ Bs
    theta = LD(4) * h2 / (LD(5) * (h2 - h1)) if damped else LD(1)
    r = theta * eta + (LD(1) - theta) * Bs
    return B - np.outer(Bs, Bs) / h2 + np.outer(r, r) / (s @ r), r, Bs


def rounding_bound(Z, s, eta, Bs, info):
    """Elementwise bound on ``|fl(Z+) - Z+|`` for the product formula evaluated in double, first order in u:

        (11 n + 26) u kappa ( |Z| + |s| ((R + alpha |Bs|)' |Z|) / (alpha^2 h2) ),   R = theta |eta| + (1 - theta) |Bs|,
        kappa = max(1, S1 / h1', S1 / h2, S2 / h2),   S1 = sum |s_i eta_i|,  S2 = sum |s_i Bs_i|,  h1' = h1 after damping.

    Derivation.  A length-n sum of products in any order, fused or not, errs by at most w = n u times the sum of the
    terms' magnitudes: the host's h1 and h2 have relative errors e1 <= w S1 / h1 and e2 <= w S2 / h2, both <= w kappa.
    Damped branch (0 < theta < 1, h1' = 0.2 h2, alpha^2 = 0.2):
    * theta = (h2 - 0.2 h2) / (h2 - h1).  The numerator errs by 1.5 e2 + 1.5 u of 0.8 h2.  The denominator is at least
      0.8 h2 and errs by w (S1 + S2) + u of itself: at most 2.5 w kappa + u.  With the division,
      e_theta <= 4 w kappa + 3.5 u.
    * alpha = sqrt(0.2 h2 / h2) is formed from the computed h2 on both sides: e_alpha <= 2.5 u, no kappa.
    * r_i = theta eta_i + (1 - theta) Bs_i: roundings 3 u R_i; the error of theta moves it by e_theta theta |eta_i - Bs_i|
      <= e_theta (R_i + 2.24 alpha |Bs_i|), as theta |eta_i| <= R_i and theta |Bs_i| <= |Bs_i| = alpha |Bs_i| / sqrt(0.2).
    * v_i = (r_i - alpha Bs_i) / (alpha h2): the numerator adds (e_alpha + u) alpha |Bs_i| and u of itself, the
      denominator and the division e_alpha + e2 + 2 u of the quotient.  Altogether
      |dv_i| alpha h2 <= (2.24 e_theta + 2 e_alpha + e2 + 6 u) (R_i + alpha |Bs_i|) <= (10 w kappa + 19 u) (R_i + alpha |Bs_i|).
    * on the device: the sum v'Z over n rows, w on sum_i |v_i| |Z_ik|; 1 / alpha (e_alpha + u), the two products
      (2 u), and the subtraction from Z_ik, u (|Z_ik| + |term|).
    The sum is (10 kappa + 1) w + 25.5 u on the term and u on Z_ik: at most (11 n + 26) u kappa.
    Undamped branch (theta = 1 and r = eta exactly): e_alpha <= (e1 + e2 + u) / 2 + u <= w kappa + 1.5 u;
    |dv_i| alpha h2 <= (2 e_alpha + e2 + 4 u) (R_i + alpha |Bs_i|); with the device's share, (5 n + 13) u kappa.
    ``R + alpha |Bs|`` stands where the formula has ``r - alpha Bs``, and ``R`` where it has ``r``, so that cancellation
    inside v and inside r is covered; kappa carries the cancellation of the host's sums into theta and alpha.
    The issue's outline reads (2 n + 16) with |r|: it counts one length-n sum, while h2 enters through theta, alpha
    (three times) and the denominator.  The derived constant of the damped branch, the larger, is used for both."""
    n = s.size
    theta, alpha, h1, h2 = info["theta"], info["alpha"], info["h1"], info["h2"]
    S1, S2 = float(np.abs(s * eta).sum()), float(np.abs(s * Bs).sum())
    kappa = max(1.0, S1 / h1, S1 / h2, S2 / h2)
    R = theta * np.abs(eta) + (1.0 - theta) * np.abs(Bs)
    term = np.outer(np.abs(s), (R + alpha * np.abs(Bs)) @ np.abs(Z)) / (alpha * alpha * h2)
    return (11 * n + 26) * U * kappa * (np.abs(Z) + term), kappa


# ------------------------------------------------------------------------------------------- inputs of the update
KINDS = ("undamped", "damped", "threshold")


def dense_factor(rng, n):
    return rng.normal(size=(n, n)) / np.sqrt(n) + np.eye(n)


def threshold_vectors(n, seed):
    """Integer-valued ``s, eta, Bs`` with ``s'eta == 0.2 * (s'Bs)`` exactly in double, and the unimodular factor they
    are consistent with: ``W = I + a sub-diagonal of -1 / 0 / 1``, ``Z = W^-1`` (entries -1 / 0 / 1), ``B = W'W``,
    ``s = 5 t`` with ``t`` in -1 / 0 / 1 and ``t_0 = 1``, ``Bs = B s``, ``eta`` zero but for ``eta_0`` and six small
    entries.  (A random ``Z`` has no integer ``B s``.)  Most of ``s'eta`` is the one product ``s_0 eta_0``, so that
    ``eta_0`` moved by one ulp still moves the double sum in any order.  -> Z, B, s, eta, Bs and eta with eta_0 one ulp
    down; the preconditions are asserted by the tests that use them."""
    for trial in range(200):
        rng = np.random.default_rng(1000 * seed + trial)
        W = np.eye(n) + np.diag(rng.integers(-1, 2, size=n - 1).astype(float), -1)
        Z = np.round(np.linalg.inv(W))
        B = W.T @ W
        t = rng.integers(-1, 2, size=n).astype(float)
        t[0] = 1.0
        s = 5.0 * t
        Bs = B @ s
        eta = np.zeros(n)
        if n > 1:
            where = 1 + rng.permutation(n - 1)[:6]
            eta[where] = rng.integers(-3, 4, size=where.size)
        eta[0] = (float(s @ Bs) / 5.0 - float(s[1:] @ eta[1:])) / 5.0
        down = eta.copy()
        down[0] = np.nextafter(eta[0], -np.inf)
        ok = (np.array_equal(W @ Z, np.eye(n)) and eta[0] >= 1.0 and eta[0] == np.round(eta[0])
              and float(s @ eta) == 0.2 * float(s @ Bs) and float(s @ down) < 0.2 * float(s @ Bs)
              and np.abs(s * eta).sum() <= 20.0 * float(s @ eta) and np.abs(s * Bs).sum() <= 20.0 * float(s @ Bs))
        if ok:
            return Z, B, s, eta, Bs, down
    raise AssertionError("no threshold input found for n = %d" % n)


def random_vectors(kind, rng, s, Bs):
    """``eta`` of the two random kinds.  Undamped: ``Bs + 0.1 noise``.  Damped: ``Bs - 2 noise``, where the noise has the
    signs of ``s`` and is scaled to ``s'noise = s'Bs`` (``s'eta = -s'Bs``): with plain Gaussian noise ``s'noise`` grows
    like sqrt(n) and ``s'Bs`` like n, and from n of a few dozen on the kind would not be damped at all."""
    noise = rng.normal(size=s.size)
    if kind == "undamped":
        return Bs + 0.1 * noise
    noise = np.abs(noise) * np.where(s >= 0.0, 1.0, -1.0)
    return Bs - 2.0 * noise * (float(s @ Bs) / float(s @ noise))


@functools.lru_cache(maxsize=None)
def device_update_inputs(kind, n):
    """A dense non-symmetric ``Z`` and ``s, eta, Bs`` of one kind for the device (``Bs`` is an input like the others: the
    product formula is what is tested, in double from these doubles).  Seeds are walked until kappa <= 100 and the
    branch is the kind's own by a clear margin - conditions on the inputs alone."""
    for trial in range(200):
        rng = np.random.default_rng(7000 + 100 * n + trial)
        Z = dense_factor(rng, n)
        if kind == "threshold":
            _, _, s, eta, Bs, _ = threshold_vectors(n, 50 + n)
        else:
            s = rng.normal(size=n)
            Bs = np.linalg.solve(Z @ Z.T, s)
            eta = random_vectors(kind, rng, s, Bs)
        h1, h2 = float(s @ eta), float(s @ Bs)
        if not h2 > 0.0:
            continue
        if kind == "undamped" and not h1 > 0.3 * h2:
            continue
        if kind == "damped" and not h1 < 0.1 * h2:
            continue
        damped = branch_in_double(s, eta, Bs)
        _, info = update_ld(Z, s, eta, Bs, damped)
        if rounding_bound(Z, s, eta, Bs, info)[1] <= 100.0 and np.abs(Z).min() > 0.0:
            return Z, s, eta, Bs, damped
    raise AssertionError("no %s input found for n = %d" % (kind, n))


def undefined_updates(n, rng):
    """(name, s, eta, Bs) of every update that has to be refused, around one defined triple."""
    Z = dense_factor(rng, n)
    s = rng.normal(size=n)
    Bs = np.linalg.solve(Z @ Z.T, s)
    eta = Bs + 0.1 * rng.normal(size=n)
    cases = [("s = 0", np.zeros(n), eta, np.zeros(n)), ("Bs = -s", s, eta, -s)]
    k = n // 2
    for name, base in (("s", s), ("eta", eta), ("Bs", Bs)):
        for bad in (np.nan, np.inf, -np.inf):
            vec = base.copy()
            vec[k] = bad
            trio = {"s": s, "eta": eta, "Bs": Bs}
            trio[name] = vec
            cases.append(("%s[%d] = %r" % (name, k, bad), trio["s"], trio["eta"], trio["Bs"]))
    # (s'eta = -inf with s'Bs > 0 is among them: eta[k] = -inf * sign(s[k]) - the damping would make 0.2 h2 of it)
    return Z, (s, eta, Bs), cases


# ------------------------------------------------------------------------------------------- 1. CPU: the oracle is BFGS
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n", [1, 2, 7, 40])
def test_restated_update_is_damped_bfgs(n, kind):
    """With ``Z+`` from the product formula and ``B+`` from the textbook recursion, both in longdouble and ``Bs = B s``
    exact, ``Z+ Z+' B+ = I`` and the secant equation ``B+ s = r`` hold to ``64 n eps_L cond_2(B+)`` (relative to
    ``|r|_inf`` for the secant equation): an identity in exact arithmetic, so what is left is the rounding of O(n)-term
    longdouble sums amplified by the condition of ``B+``; 64 is slack on that order, not a measurement.  cond_2 <= 1e6 by
    the choice of inputs (asserted).  Then ``bfgs_factor_update`` in double is within ``rounding_bound`` of the
    longdouble ``Z+`` of the same double inputs."""
    rng = np.random.default_rng(100 * n + KINDS.index(kind))
    if kind == "threshold":
        Z, B, s, eta, Bs, down = threshold_vectors(n, n)
        assert float(s @ eta) == 0.2 * float(s @ Bs)             # exactly on the threshold, in double
        B_ld, Bs_ld = ld(B), ld(Bs)
    else:
        for _ in range(50):                                     # (n = 1, 2: until s'eta is on the kind's side by a margin)
            Z = dense_factor(rng, n)
            B_ld = inverse_ld(ld(Z) @ ld(Z).T)
            s = rng.normal(size=n)
            Bs_ld = B_ld @ ld(s)
            Bs = Bs_ld.astype(np.float64)
            eta = random_vectors(kind, rng, s, Bs)
            h1, h2 = float(s @ eta), float(s @ Bs)
            if abs(np.linalg.det(Z)) > 0.2 and (h1 > 0.3 * h2 if kind == "undamped" else h1 < 0.1 * h2):
                break
    damped = branch_in_double(s, eta, Bs)
    assert damped == (kind == "damped")                         # (equality takes the undamped branch: the code tests <)
    # the identity, in longdouble throughout
    Zp, _ = update_ld(Z, s, eta, Bs_ld, damped)
    Bp, r, _ = textbook_bfgs_ld(B_ld, s, eta, damped)
    cond = float(np.linalg.cond(Bp.astype(np.float64)))
    assert cond <= 1e6
    bound = 64 * n * EPS_L * cond
    eye = np.eye(n, dtype=LD)
    identity = float(np.abs(Zp @ Zp.T @ Bp - eye).max())
    secant = float(np.abs(Bp @ ld(s) - r).max() / np.abs(r).max())
    print("n %d %s: identity %.2e secant %.2e bound %.2e (cond %.1e)" % (n, kind, identity, secant, bound, cond))
    assert identity <= bound and secant <= bound
    # the restatement in double against the formula in longdouble, from the same doubles
    want, info = update_ld(Z, s, eta, Bs, damped)
    limit, kappa = rounding_bound(Z, s, eta, Bs, info)
    assert kappa <= 100.0
    got = slsqp_np.bfgs_factor_update(Z, s, eta, Bs)
    assert got is not None and np.all(np.abs(ld(got) - want) <= limit)
    if kind == "threshold":
        # one ulp below the threshold: the damped branch, and the same factor to rounding
        assert branch_in_double(s, down, Bs) is True
        want_dn, info_dn = update_ld(Z, s, down, Bs, True)
        assert abs(1.0 - info_dn["theta"]) < 1e-12               # (theta = 1 - O(u): r is eta to rounding)
        got_dn = slsqp_np.bfgs_factor_update(Z, s, down, Bs)
        assert np.all(np.abs(ld(got_dn) - want_dn) <= rounding_bound(Z, s, down, Bs, info_dn)[0])
        assert np.all(np.abs(got_dn - got) <= limit)


def test_restated_update_refuses_what_is_undefined():
    """``s = 0``, ``h2 < 0`` and a non-finite entry anywhere: ``None`` (the header's contract: update undefined -> factor
    unchanged, the caller resets) - never a factor of NaN.  A strongly negative ``s'eta`` with ``h2 > 0`` is defined."""
    n = 9
    Z, (s, eta, Bs), cases = undefined_updates(n, np.random.default_rng(5))
    for name, s_, eta_, Bs_ in cases:
        with np.errstate(invalid="ignore", over="ignore"):
            assert slsqp_np.bfgs_factor_update(Z, s_, eta_, Bs_) is None, name
    assert float(s @ (-10.0 * Bs)) < 0.0 < float(s @ Bs)
    got = slsqp_np.bfgs_factor_update(Z, s, -10.0 * Bs, Bs)
    want, info = update_ld(Z, s, -10.0 * Bs, Bs, True)
    assert got is not None and np.all(np.abs(ld(got) - want) <= rounding_bound(Z, s, -10.0 * Bs, Bs, info)[0])


DEVICE_SIZES = [1, 2, 15, 16, 17, 63, 64, 65, 255, 256, 257, 1025]


@pytest.mark.parametrize("n", DEVICE_SIZES)
def test_device_update_inputs_are_fair_to_the_restatement(n):
    """The inputs of ``test_gpu_bfgs_at_every_block_and_pitch_edge``, here on the CPU: kappa <= 100, the kind's own
    branch, and ``bfgs_factor_update`` in double inside the derived bound."""
    for kind in KINDS:
        Z, s, eta, Bs, damped = device_update_inputs(kind, n)
        assert damped == (kind == "damped")
        if kind == "threshold":
            assert float(s @ eta) == 0.2 * float(s @ Bs)
        want, info = update_ld(Z, s, eta, Bs, damped)
        limit, kappa = rounding_bound(Z, s, eta, Bs, info)
        assert kappa <= 100.0
        got = slsqp_np.bfgs_factor_update(Z, s, eta, Bs)
        ratio = float((np.abs(ld(got) - want) / ld(limit)).max())
        print("n %d %s: kappa %.1f, restatement at %.3f of the bound" % (n, kind, kappa, ratio))
        assert ratio <= 1.0


# ------------------------------------------------------------------------------------------- 2. GPU: og_qp_bfgs
@pytest.mark.gpu
@pytest.mark.parametrize("n", DEVICE_SIZES)
def test_gpu_bfgs_at_every_block_and_pitch_edge(n, default_forms):
    """``og_qp_bfgs`` on a dense non-symmetric factor, three kinds of (s, eta) per size, against the product formula in
    longdouble, elementwise within ``rounding_bound`` (derived there).  The sizes: the row pitch 16 ceil((n + 1) / 16)
    at n + 1 = 16 and 32; the 64-column workgroups of ``k_gemv_cols`` with fewer rows than its 16 wavefronts, one and
    several workgroups; the 256-column workgroups of ``k_rank1``.  Measured on the MI355X: the core's worst entry is at
    0.010 of the bound (n = 15 and 17, on the threshold) and below 0.005 of it from n = 63 on; the restatement's, on
    the CPU, at 0.007 of it or less."""
    core = _sqp_native.QpCore(n, 0, 0)
    for kind in KINDS:
        Z, s, eta, Bs, damped = device_update_inputs(kind, n)
        want, info = update_ld(Z, s, eta, Bs, damped)
        limit, kappa = rounding_bound(Z, s, eta, Bs, info)
        assert kappa <= 100.0
        core.set_factor(Z)
        assert core.bfgs(s, eta, Bs) is False
        got = core.get_factor()
        ratio = float((np.abs(ld(got) - want) / ld(limit)).max())
        record_measurement("test_gpu_bfgs_at_every_block_and_pitch_edge", n=n, kind=kind, kappa=round(kappa, 2),
                           share_of_bound=ratio)
        print("n %d %s: kappa %.1f, core at %.3f of the bound" % (n, kind, kappa, ratio))
        assert ratio <= 1.0, (kind, ratio)
    core.close()


@pytest.mark.gpu
@pytest.mark.parametrize("n", [15, 16, 17])
def test_gpu_factor_round_trip_is_bit_identical(n, default_forms):
    Z = dense_factor(np.random.default_rng(n), n)
    core = _sqp_native.QpCore(n, 0, 0)
    core.set_factor(Z)
    assert np.array_equal(core.get_factor(), Z)
    core.close()


@pytest.mark.gpu
def test_gpu_bfgs_refuses_what_is_undefined(default_forms):
    """Every undefined update of ``test_restated_update_refuses_what_is_undefined`` on the device at n = 65 (two
    workgroups of ``k_gemv_cols``): the reset is asked for and the factor is the bits that were set.  The strongly damped
    update (``eta = -10 Bs``) is defined and matches the reference."""
    n = 65
    Z, (s, eta, Bs), cases = undefined_updates(n, np.random.default_rng(6))
    core = _sqp_native.QpCore(n, 0, 0)
    for name, s_, eta_, Bs_ in cases:
        core.set_factor(Z)
        assert core.bfgs(s_, eta_, Bs_) is True, name
        assert np.array_equal(core.get_factor(), Z), name
    core.set_factor(Z)
    assert core.bfgs(s, -10.0 * Bs, Bs) is False
    want, info = update_ld(Z, s, -10.0 * Bs, Bs, True)
    limit, kappa = rounding_bound(Z, s, -10.0 * Bs, Bs, info)
    assert kappa <= 100.0 and np.all(np.abs(ld(core.get_factor()) - want) <= limit)
    core.close()


# ------------------------------------------------------------------------------------------- 3. the factor after a solve
def row_sample(meq, extra=()):
    """At most 16 equality rows: the first, the last, ``extra`` (a row that repeats an earlier one stays lower
    triangular: it is looked at), then the rows on either side of every multiple of 64 and of 16, up to the budget."""
    rows = [0, meq - 1] + list(extra)
    for step in (64, 16):
        for edge in range(step, meq, step):
            rows += [edge - 1, edge]
    out = []
    for r in rows:
        if 0 <= r < meq and r not in out:
            out.append(r)
    return out[:16]


def factor_metrics(Z, Zg, C, rows, X):
    """orth: ``max |Zg (Zg'X) - Z (Z'X)| / max |Z (Z'X)|`` on the columns of ``X`` - ``Zg Zg' = Z Z'`` at O(n^2).
    tri: over the sampled equality rows i, ``max_{j > i} |(C_i Zg)_j| / |C_i Zg|_2`` - ``C Zg`` is lower triangular,
    that is, the rotation is the ``Q`` of these equalities.  Both in longdouble."""
    Zl, Zgl, Xl = ld(Z), ld(Zg), ld(X)
    ref = Zl @ (Xl.T @ Zl).T
    got = Zgl @ (Xl.T @ Zgl).T
    orth = float(np.abs(got - ref).max() / np.abs(ref).max())
    tri = 0.0
    for i in rows:
        t = ld(C[i]) @ Zgl
        if i + 1 < t.size:
            tri = max(tri, float(np.abs(t[i + 1:]).max() / np.sqrt(t @ t)))
    return orth, tri


def within_ten_times(measured, base):
    return all(m <= 10.0 * max(b, FLOOR) for m, b in zip(measured, base))


# (shape key: n, m_eq, m_ineq, bounds free, repeated equality)
FACTOR_SHAPES = {
    "panels": (300, 165, 12, True, True),
    "warm": (120, 40, 90, False, False),
    "wide": (2113, 65, 64, True, False),
    "hand-over": (2200, 200, 64, True, False),
}


@functools.lru_cache(maxsize=None)
def factor_problem(key):
    """The subproblem of one shape, the restatement's rotated factor (LAPACK's LQ where no pivot is small) measured by
    the two metrics, and the restatement's steps for the later solves on the handle (all from the ORIGINAL ``Z``)."""
    n, meq, mg, free, repeated = FACTOR_SHAPES[key]
    rng = np.random.default_rng(n + meq + mg)
    Z, g, C, c, G, h, lb, ub = random_qp(rng, n, meq, mg)
    if free:
        lb[:], ub[:] = -np.inf, np.inf
    extra = ()
    if repeated:
        where, src = meq // 2 + 3, meq // 2 - 9
        C[where], c[where] = -1.5 * C[src], -1.5 * c[src]
        extra = (where,)
    g2, g3 = g + 0.2 * rng.normal(size=n), rng.normal(size=n)
    X = rng.normal(size=(n, 4))
    rows = row_sample(meq, extra)
    first = slsqp_np.qp_solve(Z, g, C, c, G, h, lb, ub, lq="lapack")
    assert first[3] == 1
    P = {"n": n, "meq": meq, "mg": mg, "Z": Z, "g": g, "g2": g2, "g3": g3, "C": C, "c": c, "G": G, "h": h, "lb": lb,
         "ub": ub, "A": np.vstack([C, G]), "cc": np.concatenate([c, h]), "X": X, "rows": rows, "where": extra,
         "d": first[0], "base": factor_metrics(Z, first[4], C, rows, X)}
    if key != "hand-over":
        for name in ("g2", "g3"):
            if key == "warm" or name == "g3":
                ref = slsqp_np.qp_solve(Z, P[name], C, c, G, h, lb, ub, lq="lapack")
                assert ref[3] == 1
                P["d_" + name] = ref[0]
    return P


def test_factor_metrics_refuse_wrong_factors():
    """On the restatement's rotated factor at (60, 25, 10): the untouched factor passes 10 x its own measure (floored at
    2^-52); an entry moved by 1e-9, a column scaled by 1 + 1e-9 and a row left unrotated fail; two of the first m_eq
    columns swapped leave ``Zg Zg'`` as it was - orth cannot see it, tri must."""
    n, meq, mg = 60, 25, 10
    rng = np.random.default_rng(60)
    Z, g, C, c, G, h, lb, ub = random_qp(rng, n, meq, mg)
    X = rng.normal(size=(n, 4))
    rows = row_sample(meq)
    assert rows == [0, 24, 15, 16]
    J = slsqp_np.qp_solve(Z, g, C, c, G, h, lb, ub, lq="lapack")[4]
    base = factor_metrics(Z, J, C, rows, X)
    assert base[0] <= 1e-14 and base[1] <= 1e-14 and within_ten_times(base, base)
    moved = J.copy()
    moved[n // 2, 40] += 1e-9
    scaled = J.copy()
    scaled[:, 7] *= 1.0 + 1e-9
    swapped = J.copy()
    swapped[:, [15, 19]] = swapped[:, [19, 15]]
    unrotated = J.copy()
    unrotated[33] = Z[33]
    for name, bad in (("entry", moved), ("column", scaled), ("swap", swapped), ("row", unrotated)):
        measured = factor_metrics(Z, bad, C, rows, X)
        assert not within_ten_times(measured, base), (name, measured)
        if name == "swap":
            assert measured[0] <= 10.0 * max(base[0], FLOOR) and measured[1] > 1e-3


# Measured (orth / tri): the restatement's own factor, then the core's on the MI355X, form by form.
#   panels (300, 165, 12)      restatement 1.3e-15 / 2.2e-16; core: default 5.8e-16 / 1.7e-16, OGSQP_LQ=16 8.5e-16 / 1.7e-16,
#                              OGSQP_LQ=8 6.6e-16 / 2.2e-16
#   warm (120, 40, 90)         restatement 6.6e-16 / 2.0e-16; core: cold 6.1e-16 / 1.8e-16, warm-started 5.5e-16 / 1.9e-16;
#                              OGSQP_WARM=0: 6.1e-16 / 1.8e-16, then 6.8e-16 / 1.8e-16
#   wide (2113, 65, 64)        restatement 8.7e-16 / 2.2e-16; core: default, OGSQP_WIDE_AHEAD=0 and OGSQP_WIDE_INBLOCK=1 alike
#                              8.4e-16 / 2.6e-16; OGSQP_WIDE=0 5.1e-16 / 2.6e-16
#   hand-over (2200, 200, 64)  restatement 1.0e-15 / 2.1e-16; core 1.5e-15 / 3.3e-16
FACTOR_CASES = [
    ("panels", {}), ("panels", {"OGSQP_LQ": "16"}), ("panels", {"OGSQP_LQ": "8"}),
    ("warm", {}), ("warm", {"OGSQP_WARM": "0"}),
    ("wide", {}), ("wide", {"OGSQP_WIDE_AHEAD": "0"}), ("wide", {"OGSQP_WIDE_INBLOCK": "1"}), ("wide", {"OGSQP_WIDE": "0"}),
    ("hand-over", {}),
]


def form_name(env):
    return ",".join("%s=%s" % kv for kv in sorted(env.items())) or "default"


@pytest.mark.gpu
@pytest.mark.parametrize("key,env", FACTOR_CASES, ids=["%s-%s" % (k, form_name(e)) for k, e in FACTOR_CASES])
def test_gpu_factor_a_solve_leaves(key, env, default_forms):
    """``get_factor()`` after a solved subproblem, in every form of the LQ sweep: orth and tri (``factor_metrics``) of
    the core's ``Z Q`` at most 10 x the restatement's own on the same data (floor 2^-52).

    * panels: several 16-reflector panels, a last panel of 5 reflectors, equality ``meq//2 + 3`` = -1.5 x equality
      ``meq//2 - 9`` (no reflector is built from it); look-ahead, separate launches, 8-reflector panels.
    * warm: a second subproblem warm-started on the handle (``g + 0.2 noise``, no ``set_factor``): its warm rows go
      through the sweep and rotate ``Z`` further - orth holds, tri holds for the m_eq equality rows.
    * wide: two wide blocks, the second of one reflector; side streams, one stream, the in-block update in one
      launch, the old 8-reflector kernels.
    * hand-over: wide blocks at k = 0, 64, 128, then the 16-reflector panel from k = 192.

    On the same handle: a relaxed solve (wide) and an incompatible plain solve (panels) leave the factor's bits; and
    the rotated factor is a factor - a further solve WITHOUT ``set_factor``, new ``g``, empty active set, returns the
    restatement's step for the original ``Z`` to 1e-10 max(1, |d|_inf) (panels, warm, wide)."""
    P = factor_problem(key)
    for name, value in env.items():
        default_forms.setenv(name, value)
    n, meq, mg, Z, A, cc, lb, ub = (P[k] for k in ("n", "meq", "mg", "Z", "A", "cc", "lb", "ub"))

    def close_to(d, ref):
        return np.max(np.abs(d - ref)) <= 1e-10 * max(1.0, np.abs(ref).max())

    def measure(stage):
        Zg = core.get_factor()
        got = factor_metrics(Z, Zg, P["C"], P["rows"], P["X"])
        record_measurement("test_gpu_factor_a_solve_leaves", shape=key, form=form_name(env), stage=stage,
                           orth=got[0], tri=got[1], restatement_orth=P["base"][0], restatement_tri=P["base"][1])
        print("%s %s %s: orth %.2e tri %.2e (restatement %.2e %.2e)" % ((key, form_name(env), stage) + got + P["base"]))
        assert within_ten_times(got, P["base"]), (stage, got, P["base"])
        return Zg

    core = _sqp_native.QpCore(n, meq, mg)
    core.set_active()
    core.set_factor(Z)
    d, mult, bm, status, iters = core.solve(A, P["g"], cc, lb, ub)
    assert status == 1 and close_to(d, P["d"])
    if P["where"]:
        assert mult[P["where"][0]] == 0.0
    Zg = measure("cold")
    if key == "warm":
        d2, _, _, status, _ = core.solve(A, P["g2"], cc, lb, ub)
        assert status == 1 and close_to(d2, P["d_g2"])
        Zg = measure("warm-started")
    if key == "wide":
        d4, _, _, status, _ = core.solve(A, P["g"], cc, np.append(lb, 0.0), np.append(ub, 1.0), True, 100.0)
        assert status == 1 and d4.size == n + 1
        assert np.array_equal(core.get_factor(), Zg)                 # relaxed solves never touch the factor
    if key != "hand-over":
        core.set_active()
        d3, _, _, status, _ = core.solve(A, P["g3"], cc, lb, ub)     # on Z Q: the same B
        assert status == 1 and close_to(d3, P["d_g3"])
    if key == "panels":
        Zg = core.get_factor()
        A4, c4 = A.copy(), cc.copy()
        A4[-1], c4[-1] = -A[meq], -cc[meq] - 1.0                      # a'd + h >= 0 and -a'd - h - 1 >= 0
        core.set_active()
        assert core.solve(A4, P["g"], c4, lb, ub)[3] == _sqp_native.QP_INCOMPATIBLE
        assert np.array_equal(core.get_factor(), Zg)                 # a failed solve leaves the factor alone
    assert core.recoveries() == 0
    core.close()


# ------------------------------------------------------------------------------------------- 4. the driver's cycle
CHAIN_STEPS = 6


def chain_problem(n, meq, mg):
    """A convex quadratic ``f = x'Mx/2 + q'x`` (``M`` SPD, eigenvalues log-spaced over [0.01, 1]: cond 100 - below and
    above a fifth of the curvature of the start ``B``, so that both branches of the update are met) under the
    constant linear constraints and the bounds of ``random_qp``; the start x = 0."""
    rng = np.random.default_rng(n + meq + mg)
    Z, q, C, c, G, h, lb, ub = random_qp(rng, n, meq, mg)
    Q, _ = np.linalg.qr(rng.normal(size=(n, n)))
    lam = np.logspace(-2.0, 0.0, n)
    M = (Q * lam) @ Q.T
    M = 0.5 * (M + M.T)
    kicks = rng.normal(size=(CHAIN_STEPS, n))
    return Z, q, M, np.vstack([C, G]), np.concatenate([c, h]), lb, ub, kicks


def run_chain(n, meq, mg, core=None):
    """CHAIN_STEPS major iterations with the driver's own formulas (``sqp.minimize_slsqp_hip`` / ``slsqp_np.slsqp`` with
    a full step): solve -> ``v = g - A'r``, ``Bd = bound_mult - v``, ``s = d``, ``g+ = g + M d``,
    ``eta = (g+ - A'r) - v``, ``c+ = c + A d`` -> BFGS with (s, eta, Bd); a seeded vector is added to g after each
    iteration so that the steps stay O(1).  ``core``: the HIP handle, or None for the restatement in double.  Next to it
    ``B_k`` is carried in longdouble by the textbook recursion from the chain's own (s, eta), with ``B_k s`` exact.
    -> per iteration: |Bd - B_k d|_inf / |B_k d|_inf, max |Z' B_{k+1} Z - I|, and whether the update was damped."""
    Z0, q, M, A, c, lb, ub, kicks = chain_problem(n, meq, mg)
    Z = Z0.copy()
    B = inverse_ld(ld(Z0) @ ld(Z0).T)
    x, g = np.zeros(n), q.copy()
    if core is not None:
        core.set_active()
        core.set_factor(Z0)
    out = []
    for k in range(CHAIN_STEPS):
        dl, du = lb - x, ub - x
        if core is not None:
            d, r, bm, status, _ = core.solve(A, g, c, dl, du)
        else:
            d, lam, mu, status, Z, info = slsqp_np.qp_solve(Z, g, A[:meq], c[:meq], A[meq:], c[meq:], dl, du)
            r, bm = np.concatenate([lam, mu]), info.get("bound_multipliers")
        assert status == 1, (k, status)
        v = g - A.T @ r
        Bd = bm - v
        exact = B @ ld(d)
        stationarity = float(np.abs(ld(Bd) - exact).max() / np.abs(exact).max())
        g_new = g + M @ d
        eta = (g_new - A.T @ r) - v
        h1, h2 = ld(d) @ ld(eta), ld(d) @ exact
        damped = bool(h1 < h2 / LD(5))
        assert abs(float(h1 / h2) - 0.2) > 1e-3                     # (no branch decided by rounding)
        assert branch_in_double(d, eta, Bd) == damped
        B, _, _ = textbook_bfgs_ld(B, d, eta, damped)
        if core is not None:
            assert core.bfgs(d, eta, Bd) is False, k                # no reset
            Z = core.get_factor()
        else:
            Z = slsqp_np.bfgs_factor_update(Z, d, eta, Bd)
            assert Z is not None, k
        Zl = ld(Z)
        out.append((stationarity, float(np.abs(Zl.T @ B @ Zl - np.eye(n, dtype=LD)).max()), damped,
                    float(np.abs(d).max())))
        x = x + d
        c = c + A @ d
        g = g_new + kicks[k]
    return out


# Measured, per iteration k = 0 .. 5, |Bd - B_k d| relative, then max |Z' B_{k+1} Z - I| (the core's on the MI355X):
#   (17, 5, 8)     restatement 7.5e-16 3.6e-15 2.4e-14 1.4e-14 1.3e-13 1.7e-13 | 9.2e-16 2.9e-15 4.0e-15 4.6e-15 1.5e-14 1.6e-13
#                  core        1.0e-15 1.7e-15 3.7e-14 9.9e-15 7.2e-14 2.7e-13 | 7.5e-16 2.6e-15 8.8e-15 1.4e-14 2.8e-14 1.4e-13
#                  (damped at k = 0, 1)
#   (130, 40, 60)  restatement 5.4e-14 4.9e-14 3.4e-14 2.2e-13 4.9e-14 8.8e-14 | 1.6e-15 3.3e-15 2.9e-15 3.3e-15 3.9e-15 3.9e-15
#                  core        4.0e-14 1.9e-13 4.5e-14 1.1e-13 1.8e-13 1.6e-13 | 1.5e-15 4.6e-15 4.2e-15 5.9e-15 7.1e-15 9.5e-15
#                  (damped at k = 3, 4)
CHAIN_SHAPES = [(17, 5, 8), (130, 40, 60)]


@functools.lru_cache(maxsize=None)
def restated_chain(n, meq, mg):
    return run_chain(n, meq, mg)


@pytest.mark.parametrize("n,meq,mg", CHAIN_SHAPES)
def test_restated_chain_is_damped_somewhere_and_never_resets(n, meq, mg):
    """The calibration chain on the CPU: no reset (asserted inside), steps of O(1), the damped branch at least once and
    the undamped one as well - the seed of ``chain_problem`` is chosen so."""
    series = restated_chain(n, meq, mg)
    print([("%.1e %.1e %s" % s[:3]) for s in series])
    assert any(s[2] for s in series) and not all(s[2] for s in series)
    assert all(1e-2 <= s[3] <= 1e2 for s in series)


@pytest.mark.gpu
@pytest.mark.parametrize("n,meq,mg", CHAIN_SHAPES)
def test_gpu_solve_and_update_chained_as_the_driver_does(n, meq, mg, default_forms):
    """At every iteration of ``run_chain`` on the HIP core: no reset; the stationarity identity the driver takes ``B d``
    from, ``|Bd - B_k d|_inf / |B_k d|_inf``, and ``max |Zg' B_{k+1} Zg - I|`` each at most 10 x the restatement chain's
    value at that iteration (floor 2^-52); the damped branch is taken at least once."""
    base = restated_chain(n, meq, mg)
    core = _sqp_native.QpCore(n, meq, mg)
    series = run_chain(n, meq, mg, core)
    core.close()
    record_measurement("test_gpu_solve_and_update_chained_as_the_driver_does", n=n, m_eq=meq, m_ineq=mg,
                       stationarity=[s[0] for s in series], factor=[s[1] for s in series],
                       restatement_stationarity=[s[0] for s in base], restatement_factor=[s[1] for s in base],
                       damped=[s[2] for s in series])
    for k, (got, ref) in enumerate(zip(series, base)):
        print("k %d: core %.2e %.2e damped %s; restatement %.2e %.2e" % (k, got[0], got[1], got[2], ref[0], ref[1]))
    assert any(s[2] for s in series)
    for k, (got, ref) in enumerate(zip(series, base)):
        assert within_ten_times(got[:2], ref[:2]), (k, got, ref)


# ------------------------------------------------------------------------------------------- 5. og_jt_times
@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 3, 4, 5, 9])
def test_gpu_jt_times_on_shapes_of_its_own(n, default_forms):
    """``og_jt_times`` (one wavefront per row, four rows per workgroup: n = 1 .. 9 gives a partial, a full and a partial
    last workgroup) on a device matrix of n rows with ``ld = width + 3`` whose columns >= width hold NaN - a read past
    the width shows in the result - at widths on either side of the wavefront's 64 lanes.  ``coef = e_0`` returns column
    0 bit for bit; a random ``coef`` agrees with the longdouble sum within ``width u sum_k |row_k coef_k|`` per row (a
    sum of ``width`` products in any order)."""
    import torch
    rng = np.random.default_rng(40 + n)
    for width in (1, 2, 63, 64, 65, 130):
        ldim = width + 3
        host = np.full((n, ldim), np.nan)
        host[:, :width] = rng.normal(size=(n, width))
        dev = torch.from_numpy(host).to("cuda")
        torch.cuda.synchronize()
        core = _sqp_native.QpCore(n, 0, width - 1)
        unit = np.zeros(width)
        unit[0] = 1.0
        assert np.array_equal(core.jt_times(dev.data_ptr(), ldim, unit), host[:, 0]), width
        coef = rng.normal(size=width)
        got = core.jt_times(dev.data_ptr(), ldim, coef)
        terms = ld(host[:, :width]) * ld(coef)
        assert np.all(np.abs(ld(got) - terms.sum(axis=1)) <= width * U * np.abs(terms).sum(axis=1)), width
        core.close()
        del dev
    torch.cuda.synchronize()
