"""The HIP QP core at the shapes where its launch forms switch, certified by the extended-precision referee.

Most GPU tests of ``tests/test_slsqp_core.py`` compare one launch form of the core with another, bit for bit: that
catches a form drifting from its siblings, not an error they share, and says nothing of a form at a shape no test
reaches.  Here every answer at such an edge is certified against ``oracle/qp_referee.py``'s refined solution on the
active set the core reports (``qp_referee.certify``: step, dual and primal feasibility, multipliers) - a check that
owes nothing to another form of the same core.

CPU: the certificate itself, on small random QPs solved by the NumPy restatement - it accepts the restatement's answer
and refuses each kind of wrong one (a certificate that cannot fail certifies nothing).

GPU: the edges of the resident one-launch active-set loop (grid of 256 / 257 workgroups, the LDS at qcap 896 / 897,
the mailbox after a launch that gave up) and of the LQ sweep's hand-off from wide column-split blocks to the 16-reflector
panel at rows of 2048 / 2049 entries."""
import time

import numpy as np
import pytest

from conftest import record_measurement
from oracle import qp_referee, slsqp_np
from opengoddard_amd import _sqp_native
from test_slsqp_core import canonical_ids, random_qp

# the referee's bounds: tol_d from test_gpu_lq_panel_at_every_row_length (the core against LAPACK up to n = 1800); the
# core measures 2e-13 or less at every edge below (the numbers at each table)
TOL = {"tol_d": 1e-9, "tol_mu": 1e-7, "tol_p": 1e-7}


# ------------------------------------------------------------------------------------------- CPU: the certificate
def restated(seed, n, meq, mg):
    """A small random QP solved by the restatement, with an active inequality and an inactive one to play with."""
    rng = np.random.default_rng(seed)
    Z, g, C, c, G, h, lb, ub = random_qp(rng, n, meq, mg)
    d, lam, mu, mode, _, info = slsqp_np.qp_solve(Z, g, C, c, G, h, lb, ub)
    assert mode == 1
    data = (Z, g, np.vstack([C, G]), np.concatenate([c, h]), lb, ub, meq)
    answer = (mode, d, np.concatenate([lam, mu]), info["bound_multipliers"], canonical_ids(info["active"], mg))
    return data, answer, mu


CERT_CASES = [(3, 24, 6, 30), (4, 40, 10, 50), (5, 60, 0, 90)]


@pytest.mark.parametrize("seed,n,meq,mg", CERT_CASES)
def test_certificate_accepts_the_restatement(seed, n, meq, mg):
    data, answer, _ = restated(seed, n, meq, mg)
    measured = qp_referee.certify(*data, *answer, **TOL)
    assert measured["step"] <= 1e-12 and measured["multipliers"] <= 1e-9 and measured["referee"] <= 1e-15
    assert measured["active_rows"] > meq                       # (inequalities are active: the checks below bite)


@pytest.mark.parametrize("seed,n,meq,mg", CERT_CASES)
def test_certificate_refuses_a_moved_step(seed, n, meq, mg):
    data, (status, d, mult, bm, active), _ = restated(seed, n, meq, mg)
    scale = max(1.0, np.abs(d).max())
    moved = d.copy()
    moved[n // 2] += 1e-8 * scale
    with pytest.raises(qp_referee.CertificateError) as err:
        qp_referee.certify(*data, status, moved, mult, bm, active, **TOL)
    assert err.value.failed == ["step"], str(err.value)
    assert 0.5e-8 <= err.value.measured["step"] <= 2e-8


@pytest.mark.parametrize("seed,n,meq,mg", CERT_CASES)
def test_certificate_refuses_an_active_set_without_a_binding_row(seed, n, meq, mg):
    """The general inequality with the largest multiplier left out of the active set: the refined step on the rest
    violates it (the step and the multipliers no longer match either - the primal check must be among the failures)."""
    data, (status, d, mult, bm, active), mu = restated(seed, n, meq, mg)
    binding = int(np.argmax(mu))
    assert mu[binding] > 1e-3 and binding in active
    with pytest.raises(qp_referee.CertificateError) as err:
        qp_referee.certify(*data, status, d, mult, bm, [j for j in active if j != binding], **TOL)
    assert "primal feasibility" in err.value.failed, str(err.value)


@pytest.mark.parametrize("seed,n,meq,mg", CERT_CASES)
def test_certificate_refuses_an_active_set_with_a_slack_row(seed, n, meq, mg):
    """The inactive general inequality with the most slack forced into the active set: some multiplier of the
    refined solution comes out negative."""
    data, (status, d, mult, bm, active), _ = restated(seed, n, meq, mg)
    Z, g, A, c, lb, ub, _ = data
    slack = (A[meq:] @ d + c[meq:]) / np.linalg.norm(A[meq:], axis=1)
    slack[np.array([j for j in active if j < mg], dtype=int)] = -np.inf
    extra = int(np.argmax(slack))
    assert slack[extra] > 1e-2
    with pytest.raises(qp_referee.CertificateError) as err:
        qp_referee.certify(*data, status, d, mult, bm, active + [extra], **TOL)
    assert "dual feasibility" in err.value.failed, str(err.value)
    assert err.value.measured["dual"] < -TOL["tol_mu"]


@pytest.mark.parametrize("seed,n,meq,mg", CERT_CASES)
def test_certificate_refuses_an_altered_multiplier(seed, n, meq, mg):
    """One slot at a time - an equality's, an active inequality's, an inactive inequality's (must be zero), an active
    bound's, a free variable's bound slot (must be zero) - moved by 1e-6 of the multipliers' scale."""
    data, (status, d, mult, bm, active), mu = restated(seed, n, meq, mg)
    mscale = max(1.0, np.abs(mult).max(), np.abs(bm).max())
    general = [j for j in active if j < mg]
    free = [i for i in range(n) if bm[i] == 0.0]
    slots = [("mult", meq + general[0]), ("mult", meq + [j for j in range(mg) if j not in general][0]),
             ("bm", int(np.argmax(np.abs(bm)))), ("bm", free[0])]
    if meq:
        slots.append(("mult", meq - 1))
    for which, k in slots:
        mult2, bm2 = mult.copy(), bm.copy()
        (mult2 if which == "mult" else bm2)[k] += 1e-6 * mscale
        with pytest.raises(qp_referee.CertificateError) as err:
            qp_referee.certify(*data, status, d, mult2, bm2, active, **TOL)
        assert err.value.failed == ["multipliers"], (which, k, str(err.value))


def test_certificate_of_the_relaxed_subproblem():
    """An inconsistent QP (mode 4) and its relaxed form built by ``relaxed_subproblem`` - the construction of
    ``gpu_qp`` in test_slsqp_core.py - solved by the restatement and certified; a status other than 1 is refused."""
    rng = np.random.default_rng(9)
    n, meq, mg, rho = 30, 8, 25, 100.0
    Z, g, C, c, G, h, lb, ub = random_qp(rng, n, meq, mg, feasible=False)
    mg = G.shape[0]
    A, cc = np.vstack([C, G]), np.concatenate([c, h])
    first = slsqp_np.qp_solve(Z, g, C, c, G, h, lb, ub)
    assert first[3] == 4
    with pytest.raises(qp_referee.CertificateError) as err:
        qp_referee.certify(Z, g, A, cc, lb, ub, meq, first[3], first[0], np.zeros(meq + mg), np.zeros(n), [], **TOL)
    assert err.value.failed == ["status"]
    Za, ga, Aa, ca, lo, hi = qp_referee.relaxed_subproblem(Z, g, A, cc, lb, ub, meq, rho)
    assert np.array_equal(Aa[:, n], np.concatenate([-c, np.maximum(-h, 0.0)])) and Za[n, n] == 1.0 / rho
    d, lam, mu, mode, _, info = slsqp_np.qp_solve(Za, ga, Aa[:meq], c, Aa[meq:], h, lo, hi)
    assert mode == 1 and 0.0 < d[n] <= 1.0
    measured = qp_referee.certify(Za, ga, Aa, ca, lo, hi, meq, mode, d, np.concatenate([lam, mu]),
                                  info["bound_multipliers"], canonical_ids(info["active"], mg), **TOL)
    assert measured["step"] <= 1e-12


# ------------------------------------------------------------------------------------------- GPU: the edges
RHO = 100.0
FORM_KEYS = ("OGSQP_RESIDENT", "OGSQP_GI", "OGSQP_LQ", "OGSQP_TRSV", "OGSQP_WIDE", "OGSQP_SPIN_LIMIT", "OGSQP_WARM",
             "OGSQP_ROWS", "OGSQP_WARM_SPREAD", "OGSQP_WIDE_AHEAD", "OGSQP_WIDE_INBLOCK")


@pytest.fixture
def default_forms(monkeypatch):
    """The handles of a test are made with the default forms, whatever the suite's environment selects."""
    for key in FORM_KEYS:
        monkeypatch.delenv(key, raising=False)
    return monkeypatch


def compute_units():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


def make_qp(seed, n, meq, mg, free=False):
    """``random_qp`` as plain data ``(Z, g, A, c, lb, ub, meq)``; ``free``: no bounds (a short active-set phase when
    the sweep is what is tested, as in test_gpu_lq_panel_at_every_row_length)."""
    Z, g, C, c, G, h, lb, ub = random_qp(np.random.default_rng(seed), n, meq, mg)
    if free:
        lb[:], ub[:] = -np.inf, np.inf
    return Z, g, np.vstack([C, G]), np.concatenate([c, h]), lb, ub, meq


def solve(core, qp, kind, rep):
    """Subproblem ``rep`` of one kind on the handle: rep 0 cold (``set_active()`` first), rep r > 0 warm-started from the
    one before with ``Z (1 + 0.25 r)`` and ``g (1 + 0.1 r)`` (the scaling of
    test_gpu_resident_active_set_gives_the_bits_of_the_two_launch_form).  -> the answer and what the handle's resident
    launches did during it."""
    Z, g, A, c, lb, ub, meq = qp
    if rep == 0:
        core.set_active()
    core.set_factor(Z * (1.0 + 0.25 * rep))
    before = core.resident_stats()
    if kind == "plain":
        d, mult, bm, status, iters = core.solve(A, g * (1.0 + 0.1 * rep), c, lb, ub)
    else:
        d, mult, bm, status, iters = core.solve(A, g * (1.0 + 0.1 * rep), c, np.append(lb, 0.0), np.append(ub, 1.0),
                                                True, RHO)
    after = core.resident_stats()
    answer = {"kind": kind, "rep": rep, "d": d.copy(), "mult": mult.copy(), "bm": bm.copy(), "status": status,
              "iters": iters, "active": sorted(int(v) for v in core.get_active())}
    return answer, (after[0] - before[0], after[1] - before[1])


def certify(qp, ans):
    """The referee's certificate of one answer (the relaxed subproblem's data from ``qp_referee.relaxed_subproblem``)."""
    Z, g, A, c, lb, ub, meq = qp
    Zs, gs = Z * (1.0 + 0.25 * ans["rep"]), g * (1.0 + 0.1 * ans["rep"])
    data = (Zs, gs, A, c, lb, ub) if ans["kind"] == "plain" else qp_referee.relaxed_subproblem(Zs, gs, A, c, lb, ub, meq, RHO)
    return qp_referee.certify(*data, meq, ans["status"], ans["d"], ans["mult"], ans["bm"], ans["active"], **TOL)


def same_bits(a, b):
    return (a["status"] == b["status"] and a["iters"] == b["iters"] and a["active"] == b["active"] and
            np.array_equal(a["d"], b["d"]) and np.array_equal(a["mult"], b["mult"]) and np.array_equal(a["bm"], b["bm"]))


def record(test, case, form, answers, measured, seconds):
    worst = {key: max(m[key] for m in measured) for key in ("step", "multipliers", "primal", "referee")}
    worst["dual"] = min(m["dual"] for m in measured)            # (the least multiplier of an active row, relative)
    record_measurement(test, case=case, form=form, seconds=round(seconds, 2), iterations=[a["iters"] for a in answers],
                       **worst)
    print("%s: %s; worst step %.2e multipliers %.2e least multiplier %.2e primal %.2e (referee %.1e); %.1f s" % (
        case, form, worst["step"], worst["multipliers"], worst["dual"], worst["primal"], worst["referee"], seconds))


# (case, n, m_eq, m_ineq, subproblem kinds, the resident grid per kind - None: two-launch whatever the device)
# The grid of the resident launch is ceil((m_ineq + nq + qcap) / 15) workgroups, qcap = n + 1 - m_eq, nq = n (plain) or
# n + 1 (relaxed); it runs where that is <= min(256, compute units) and its LDS - 15 rows + 5 vectors of
# max(nr, qcap) rounded to 64 doubles, 4 lists of qcap ints - fits the 161 792 bytes (qcap <= 896).
# Measured on the MI355X (worst of the case's answers; step and multipliers relative to max(1, |.|_inf)): R1+R2 step
# 2.0e-13, multipliers 7.8e-13 (3365 / 47 / 2181 / 219 changes); R3 2.1e-13, 8.8e-13 (3159 / 70); R4 9.6e-15, 7.1e-15;
# R5 7.5e-15, 1.1e-14; every least multiplier of an active row positive, every constraint at d* within 3e-18.
RESIDENT_CASES = [
    # the plain subproblem on 256 workgroups, the relaxed one of the same handle on 257: two-launch; the mailbox is
    # sized for the relaxed grid capped at 256 (before: for ONE workgroup, and the plain launch wrote 6.5 MB past it)
    ("R1+R2", 1199, 400, 1841, ("plain", "relaxed"), {"plain": 256, "relaxed": None}),
    ("R3", 1199, 400, 1826, ("plain",), {"plain": 255}),
    # the LDS edge: qcap 896 -> 157 760 bytes (plain and relaxed); qcap 897 -> 168 000: two-launch
    ("R4", 1500, 605, 200, ("plain", "relaxed"), {"plain": 174, "relaxed": 174}),
    ("R5", 1500, 604, 200, ("plain",), {"plain": None}),
]


@pytest.mark.gpu
@pytest.mark.parametrize("case,n,meq,mg,kinds,grid", RESIDENT_CASES, ids=[c[0] for c in RESIDENT_CASES])
def test_gpu_resident_launch_at_its_edges_is_certified(case, n, meq, mg, kinds, grid, default_forms):
    """The one-launch active-set loop (``k_rows_resident``) at the edges of its grid and of its LDS: each subproblem
    cold, then warm-started (the warm start's removals run in front of the launch); every answer certified by the
    referee; the form that served it read from ``resident_stats()`` (a launch that finished and made the subproblem's
    changes, or none at all); where the resident form served, the same bits as a handle under ``OGSQP_RESIDENT=0``.
    Grids of 255 / 256 workgroups are resident only on a device with that many compute units (MI355X: 256)."""
    t0 = time.time()
    cus = compute_units()
    qp = make_qp(n + meq + mg, n, meq, mg)
    plan = [(kind, rep) for kind in kinds for rep in (0, 1)]
    core = _sqp_native.QpCore(n, meq, mg)
    answers, served = [], []
    for kind, rep in plan:
        ans, (launches, changes) = solve(core, qp, kind, rep)
        wg = grid[kind]
        if wg is not None and wg <= min(256, cus):
            assert launches >= 1 and changes == ans["iters"], (kind, rep, launches, changes, ans["iters"])
            assert rep > 0 or changes > 0
            served.append("resident on %d workgroups" % wg)
        else:
            assert (launches, changes) == (0, 0), (kind, rep, launches, changes)
            served.append("two-launch")
        assert ans["status"] == 1, (kind, rep, ans["status"])
        answers.append(ans)
    assert core.recoveries() == 0
    core.close()
    measured = [certify(qp, ans) for ans in answers]
    if any(s != "two-launch" for s in served):
        default_forms.setenv("OGSQP_RESIDENT", "0")
        core = _sqp_native.QpCore(n, meq, mg)
        for (kind, rep), ans in zip(plan, answers):
            two, stats = solve(core, qp, kind, rep)
            assert stats == (0, 0)
            assert same_bits(ans, two), (kind, rep)
        core.close()
    record("test_gpu_resident_launch_at_its_edges_is_certified", case,
           ", ".join("%s: %s" % (k, s) for k, s in zip([p[0] for p in plan[::2]], served[::2])), answers, measured,
           time.time() - t0)


# (case, n, m_eq, m_ineq, subproblem kinds, bounds free).  Measured on the MI355X (worst step / multipliers, relative):
# L1+L2 1.5e-15 / 2.0e-16, L3 1.3e-15 / 1.3e-16, L4 8.8e-16 / 1.7e-16, L5 4.0e-15 / 3.2e-15 (908 changes cold); every
# least multiplier of an active row positive, every constraint at d* within 1e-17.
LQ_CASES = [
    ("L1+L2", 2048, 300, 64, ("plain", "relaxed"), True),
    ("L3", 2112, 64, 64, ("plain",), True),
    ("L4", 2113, 65, 64, ("plain",), True),
    ("L5", 2049, 1, 64, ("plain",), False),
]


@pytest.mark.gpu
@pytest.mark.parametrize("case,n,meq,mg,kinds,free", LQ_CASES, ids=[c[0] for c in LQ_CASES])
def test_gpu_lq_sweep_hand_off_at_2048_is_certified(case, n, meq, mg, kinds, free, default_forms):
    """The hand-off of the LQ sweep from the wide column-split blocks to the 16-reflector panel at rows of 2048 / 2049
    entries, each subproblem cold and warm-started, every answer certified by the referee.

    The form follows from the rows' length nq (n plain, n + 1 relaxed) by this rule, on a handle with n + 1 > 2048 (the
    wide sweep armed): while nq - k > 2048 the sweep factors 64-reflector blocks of column-split panels
    (``lq_sweep_wide``); from the first multiple of 64 with nq - k <= 2048 on, the 16-reflector panel of
    E = ceil((nq - k) / 256) groups of columns.  So, cold (a warm subproblem appends its warm rows behind the equalities:
    longer sweeps that cross the same edge):

    * L1: nq 2048, 300 equalities - the panel alone, E = 8 from k = 0;
    * L2: the relaxed subproblem of that handle, nq 2049 - one wide block (k = 0 .. 63), then the panel from k = 64;
    * L3: nq 2112, 64 equalities - one wide block that ends the sweep (warm: its warm rows go to the panel from k = 64);
    * L4: nq 2113, 65 equalities - a block of 64, then nq - 64 = 2049 > 2048: a second wide block of ONE reflector;
    * L5: nq 2049, 1 equality - a wide sweep of a single reflector (finite bounds: a long active-set phase as well).

    Null spaces of more than 1024 coordinates: the two-launch active-set form serves all of them (``resident_stats()``
    stays (0, 0))."""
    t0 = time.time()
    qp = make_qp(n + meq + mg, n, meq, mg, free=free)
    core = _sqp_native.QpCore(n, meq, mg)
    answers = []
    for kind in kinds:
        for rep in (0, 1):
            ans, stats = solve(core, qp, kind, rep)
            assert ans["status"] == 1 and stats == (0, 0), (kind, rep, ans["status"], stats)
            answers.append(ans)
    assert core.recoveries() == 0
    core.close()
    measured = [certify(qp, ans) for ans in answers]
    record("test_gpu_lq_sweep_hand_off_at_2048_is_certified", case, "two-launch active set", answers, measured,
           time.time() - t0)


@pytest.mark.gpu
def test_gpu_subproblems_after_a_resident_launch_that_gave_up(default_forms):
    """A resident launch whose waits give up (spin bound 1) publishes records under exchange numbers that the next
    launch on the handle counts through again: the host must clear the mailbox before it gives the attempt up, or the
    next subproblem's workgroups read prices, rows and entries of r of the lost one.  Under ``OGSQP_LQ=16`` and
    ``OGSQP_TRSV=block`` the only inter-workgroup waits of a cold subproblem are the resident launch's: subproblem 1
    with the bound 1 is lost once and recovered by the two-launch form; subproblems 2-4 with the default bound are
    served by resident launches that finish, with no further recovery - and all four are the bits of a handle that
    never launches the resident form, and certified."""
    t0 = time.time()
    n, meq, mg = 900, 200, 120                                  # (a resident grid of 115 workgroups)
    qp = make_qp(17, n, meq, mg)
    default_forms.setenv("OGSQP_LQ", "16")
    default_forms.setenv("OGSQP_TRSV", "block")
    core = _sqp_native.QpCore(n, meq, mg)
    core.set_spin_limit(1)
    first, (launches, changes) = solve(core, qp, "plain", 0)
    assert core.recoveries() == 1 and launches >= 1 and changes == 0, (core.recoveries(), launches, changes)
    core.set_spin_limit(0)
    answers = [first]
    for rep in (1, 2, 3):
        ans, (launches, changes) = solve(core, qp, "plain", rep)
        assert launches >= 1 and changes == ans["iters"] > 0, (rep, launches, changes, ans["iters"])
        answers.append(ans)
    assert core.recoveries() == 1
    core.close()
    default_forms.setenv("OGSQP_RESIDENT", "0")
    core = _sqp_native.QpCore(n, meq, mg)
    for ans in answers:
        two, stats = solve(core, qp, "plain", ans["rep"])
        assert stats == (0, 0) and same_bits(ans, two), ans["rep"]
    core.close()
    assert all(ans["status"] == 1 for ans in answers)
    measured = [certify(qp, ans) for ans in answers]
    record("test_gpu_subproblems_after_a_resident_launch_that_gave_up", "lost, then resident",
           "1: lost resident launch, two-launch recovery; 2-4: resident", answers, measured, time.time() - t0)
