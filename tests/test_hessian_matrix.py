"""The exact sparse Hessian of ``w . F`` without a GPU: the pattern and term lists of ``codegen.HessianPlan``, the host
probe of ``csrc/og_hess.h`` (tests/hess_probe.cpp: the entries the kernels write, in the order of ``csrc/og_adj.h``)
against the existing probe of ``csrc/og_hvp.h`` with all ``n`` unit directions - bit for bit at the owner's orientation,
within the project's bound at the other, exact zeros outside the pattern - and against central differences of the
oracle's complex-step Jacobian, the host logic of ``Problem.hessian_matrix`` / ``evaluate_batch(hessians=)`` on a
stand-in engine, the build of the part and the C signatures.  Cases and the probes' builds are in
``hessian_matrix_cases``.

The reference of test 3 is ``hessian_cases.oracle_products`` with ``v = e_l``: column ``l`` of the Hessian from central
differences of ``oracle.exact_jac.jacobian``, Richardson-extrapolated, with its own error estimate; the probe's stored
entries of the checked columns must be within ten times the shape's worst estimate, in units of ``max(1, S)`` of an entry
(``S``: the sum of the absolute values of its terms) - the criterion of profiles/hessian.md.  ``h`` is 2^-9, and 2^-13 for
``G17`` as in tests/test_hessian.py.  Measured worst ratio probe / estimate per shape (this file writes them to
profiles/hessian_matrix.md): B5 0.68, G17 0.07, layout_8 1.07, P2U 0.76, B90 0.94.

The errors of the C calls that need a live handle are in tests/test_hessian_matrix_gpu.py.
"""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import hessian_cases as hc
import hessian_matrix_cases as mc
import parameter_exact_cases as ec
from opengoddard_amd import _native, build, codegen, optimize

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REPORT = os.path.join(ROOT, "profiles", "hessian_matrix.md")
HEAD = ["# The exact sparse Hessian of w . F: the host probe of csrc/og_hess.h", "",
        "Shapes: n, the stored entries of the lower triangle and the pairs that share a row of the Jacobian pattern; then",
        "per checked column the oracle reference's own error estimate, the probe's worst difference from it (both in units",
        "of max(1, sum of the absolute values of an entry's terms)) and their ratio.  Written by",
        "tests/test_hessian_matrix.py.", "", "| what | figure |", "|---|---|"]
STEP = {"G17": 2.0 ** -13}              # (the others: hessian_cases.H_STEP; tests/test_hessian.py says why)


def _note(key, text):
    """One line of profiles/hessian_matrix.md (the key's line is replaced, not repeated)."""
    try:
        old = open(REPORT).read().split("\n") if os.path.exists(REPORT) else []
        kept = [row for row in (old or HEAD) if not row.startswith("| %s |" % key)]
        while kept and kept[-1] == "":
            kept.pop()
        with open(REPORT, "w") as fh:
            fh.write("\n".join(kept + ["| %s | %s |" % (key, text)]) + "\n")
    except OSError:
        pass


@pytest.fixture(scope="module")
def probe_dir(tmp_path_factory):
    return str(tmp_path_factory.mktemp("hess_probe"))


def _same_bits(a, b):
    return np.array_equal(a, b) and np.array_equal(np.signbit(a), np.signbit(b))


_RUNS = {}


def _runs(key, probe_dir):
    """Per point and parameter set of the shape: the probe's entries and the ``n`` unit-direction products of the
    Hessian-vector probe, both for the eight weight vectors; once per session."""
    if key not in _RUNS:
        C = mc.case(key)
        W = mc.weights(C)
        exe, unit = mc.build_probe(C, probe_dir), hc.build_probe(C, probe_dir)
        out = []
        for ip, x in enumerate(C.points):
            for it, theta in enumerate(C.thetas):
                r = mc.run_probe(C, exe, probe_dir, x, W, theta, "hess_%d_%d" % (ip, it))
                Q, S = mc.unit_products(C, unit, probe_dir, x, W, theta, "unit_%d_%d" % (ip, it))
                out.append((x, theta, r, Q, S))
        _RUNS[key] = (C, W, exe, out)
    return _RUNS[key]


# ------------------------------------------------------------------------------------------------ 1. and 2.
@pytest.mark.parametrize("key", mc.GPU_KEYS)
def test_entries_are_the_unit_products_bits_and_the_pattern_is_complete(key, probe_dir):
    C, W, exe, runs = _runs(key, probe_dir)
    hp = mc.plan(C)
    row, col, owner, partner = mc.pairs_of(hp)
    stored = np.zeros((C.n, C.n), dtype=bool)
    stored[row, col] = stored[col, row] = True
    assert len(runs) == len(C.points) * len(C.thetas) and W.shape[0] == 8
    for x, theta, r, Q, S in runs:
        assert np.all(np.isfinite(Q)) and np.all(np.isfinite(r.H))
        assert _same_bits(r.H, Q[:, partner, owner]), (key, "hvp(w, e_partner)[owner]")
        off = Q[:, ~stored]
        assert not off.any() and not np.signbit(off).any(), (key, "an entry outside the pattern is not +0.0")
        assert np.array_equal(r.terms, hp.terms)


@pytest.mark.parametrize("key", mc.GPU_KEYS)
def test_the_other_orientation_within_the_bound(key, probe_dir):
    C, W, exe, runs = _runs(key, probe_dir)
    row, col, owner, partner = mc.pairs_of(mc.plan(C))
    seen = 0.0
    for x, theta, r, Q, S in runs:
        other = Q[:, owner, partner]                    # hvp(w, e_owner)[partner]
        assert np.all(np.abs(other - r.H) <= mc.BOUND * r.S), key
        seen = max(seen, float(r.S.max()))
    assert seen > 0


# ------------------------------------------------------------------------------------------------ 3. the oracle
def _columns(C):
    """The final time, one control, one state mid-phase, one variable of a row item (other than those), as far as the
    shape has them."""
    P, hp = C.program, mc.plan(C)
    plan = codegen.SweepPlan(P)
    collocated = set()
    for sl in P.mv:
        collocated.update(range(sl.leaf_base, sl.leaf_base + sl.length))
    free = [j for j in range(P.n - len(P.nodes)) if j not in collocated and hp.terms[j] > 0]
    picks = [("final time", P.n - 1)]
    if free:
        picks.append(("control", free[len(free) // 2]))
    picks.append(("state", P.mv[0].leaf_base + P.mv[0].length // 2))
    taken = {j for _, j in picks}
    for j in range(P.n):
        if j not in taken and any(P.groups[gi].kind == "rows" for gi, o, k in plan.items[j]):
            picks.append(("row item", j))
            break
    return picks


@pytest.mark.parametrize("key", mc.GPU_KEYS)
def test_columns_against_differences_of_the_oracle(key, probe_dir, capsys):
    C, W, exe, runs = _runs(key, probe_dir)
    x, theta, r, _, _ = runs[min(1, len(runs) - 1) * len(C.thetas) + len(C.thetas) - 1]   # second point, last set
    hp = mc.plan(C)
    row, col, owner, partner = mc.pairs_of(hp)
    h = STEP.get(key, hc.H_STEP)
    picks = _columns(C)
    assert len(picks) >= 3 and picks[0][1] == C.n - 1
    estimate = worst = 0.0
    for what, l in picks:
        e = np.zeros(C.n)
        e[l] = 1.0
        ref, err = hc.oracle_products(C, x, W, e, theta, h)            # [K, n]: column l of every vector's Hessian
        at = np.flatnonzero((row == l) | (col == l))
        assert at.size > 0, (key, what, l)
        j = np.where(row[at] == l, col[at], row[at])
        scale_full = np.ones((W.shape[0], C.n))
        scale_full[:, j] = np.maximum(1.0, r.S[:, at])
        own = err / scale_full
        smooth = own <= 1e-6                            # (else: a kink inside the stencil)
        assert (~smooth).sum() * 50 <= own.size, (key, what, int((~smooth).sum()))
        col_estimate = float(own[smooth].max())
        diff = np.abs(r.H[:, at] - ref[:, j]).astype(float) / scale_full[:, j]
        col_worst = float(diff[smooth[:, j]].max())
        # outside the pattern the reference sees nothing but its own error
        outside = np.ones(C.n, dtype=bool)
        outside[j] = False
        beyond = np.abs(ref[:, outside]).astype(float)[smooth[:, outside]]
        col_worst = max(col_worst, float(beyond.max()) if beyond.size else 0.0)
        _note("%s %s (x_%d)" % (key, what, l), "estimate %.1e, probe %.1e" % (col_estimate, col_worst))
        with capsys.disabled():
            if os.environ.get("OG_SURFACE_REPORT"):
                print("hessian matrix %-10s %-10s x_%-4d estimate %.2e probe %.2e" % (key, what, l, col_estimate, col_worst))
        estimate, worst = max(estimate, col_estimate), max(worst, col_worst)
    # the criterion of profiles/hessian.md: within ten times the shape's worst estimate
    assert estimate > 0 and worst <= 10.0 * estimate, (key, estimate, worst)
    _note("%s worst ratio" % key, "%.2f (estimate %.1e, probe %.1e)" % (worst / estimate, estimate, worst))


# ------------------------------------------------------------------------------------------------ 4. the pattern
@pytest.mark.parametrize("key", mc.GPU_KEYS)
def test_pattern_sanity(key, probe_dir):
    C, W, exe, runs = _runs(key, probe_dir)
    P, hp = C.program, mc.plan(C)
    indptr, cols, owner, tptr, tlist = hp.arrays()
    row, col, own, partner = mc.pairs_of(hp)
    n = C.n
    assert indptr.size == n + 1 and indptr[-1] == hp.nnz == cols.size and np.all(np.diff(indptr) >= 0)
    assert np.all(col <= row) and np.all((own == row) | (own == col))
    for j in range(n):
        assert np.all(np.diff(cols[indptr[j]:indptr[j + 1]]) > 0)
    # a subset of the pairs that share a row of the Jacobian pattern, and strictly fewer of them
    jp, jrows = codegen.sparsity(P)
    B = np.zeros((n, C.m), dtype=np.int64)
    for j in range(n):
        B[j, jrows[jp[j]:jp[j + 1]]] = 1
    share = np.tril(B @ B.T > 0)
    assert np.all(share[row, col]), key
    assert hp.nnz < int(share.sum()), (key, hp.nnz, int(share.sum()))
    _note("%s pattern" % key, "n %d, nnz %d, pairs that share a Jacobian row %d" % (n, hp.nnz, int(share.sum())))
    # the diagonal of every collocated variable
    stored = set(zip(row.tolist(), col.tolist()))
    for sl in P.mv:
        for j in range(sl.leaf_base, sl.leaf_base + sl.length):
            assert (j, j) in stored
    # the lists: ascending, inside the owner's column; the owner has no more terms than the partner, ties to the larger
    assert tptr.size == hp.nnz + 1 and tptr[0] == 0 and np.all(np.diff(tptr) >= 0)
    terms = np.asarray(hp.terms)
    for q in range(hp.nnz):
        lst = tlist[tptr[q]:tptr[q + 1]]
        assert np.all(np.diff(lst) > 0) and (lst.size == 0 or (lst[0] >= 0 and lst[-1] < terms[own[q]]))
    assert np.all(terms[own] <= terms[partner]) and np.all((terms[own] < terms[partner]) | (own >= partner))
    # a zero weight vector: +0.0 everywhere; vector d of K is the call with that vector alone
    x, theta, r, Q, S = runs[0]
    assert not W[6].any() and not r.H[6].any() and not np.signbit(r.H[6]).any()
    for d in (0, 4, 7):
        one = mc.run_probe(C, exe, probe_dir, x, W[d], theta, "one")
        assert one.H.shape == (1, hp.nnz) and _same_bits(one.H[0], r.H[d]) and np.array_equal(one.F0, r.F0)
    # the matrix forms of the result object against the probe's own Hessian-vector products
    res = optimize.SparseHessian(r.H, indptr, cols)
    V = C.directions()[[3, 4, 2]]
    unit = hc.build_probe(C, probe_dir)
    for d in (2, 3, 5):
        A = res.toarray(d)
        M = res.tocsr(d)
        assert np.array_equal(A, A.T) and abs(M - M.T).nnz == 0 and np.array_equal(M.toarray(), A)
        assert np.array_equal(res.tocsr(d, symmetric=False).toarray(), np.tril(A))
        Sd = np.zeros((n, n))
        Sd[row, col] = Sd[col, row] = r.S[d]
        hv = hc.run_probe(C, unit, probe_dir, x, np.tile(W[d], (3, 1)), V, theta, "matvec")
        for i in range(3):
            got = A.astype(np.longdouble) @ V[i].astype(np.longdouble)
            assert np.all(np.abs(got - hv.Q[i]).astype(float) <= mc.BOUND * (Sd @ np.abs(V[i]))), (key, d, i)
    assert _same_bits(optimize.SparseHessian(r.H[3], indptr, cols).toarray(), res.toarray(3))


def test_the_shapes_cover_every_path_of_the_kernel():
    """Lists of more than 64 terms (a workgroup), of more than 256 (a second pass, two listed terms in one chain), lists
    that are no prefix of the column, entries without a diagonal partner, and variables without any entry."""
    longest, sparse = {}, {}
    for key in mc.GPU_KEYS:
        hp = mc.plan(mc.case(key))
        ln = np.diff(hp.tptr)
        longest[key] = int(ln.max())
        sparse[key] = any(hp.tlist[hp.tptr[q]:hp.tptr[q + 1]] != list(range(ln[q])) for q in range(hp.nnz) if ln[q])
        assert (ln >= 1).all(), key
    assert longest["B90"] == 272 and longest["layout_8"] > 64 and longest["B5"] <= 64 and longest["P2U"] <= 64
    assert all(sparse.values())
    hp = mc.plan(mc.case("layout_8"))
    assert (np.diff(hp.indptr) == 0).sum() >= 130
    # bit 1 of a slot's `reads` word (the dynamics term of every defect row of the own block, not of row k == l alone):
    # NL2's np.sum(x * x) has curvature along x_l in all N rows, so the diagonal entry of x_l lists N terms of the own
    # block; NL0's cos(x - x[0]) couples x_k with x_0 - a stored pair inside one state's slice, its terms in that block
    assert len(mc.GPU_KEYS) == 7
    for key, l, partner, count in (("NL2", 5, 5, 21), ("NL0", 5, 0, 1)):
        C = mc.case(key)
        hp, sl = mc.plan(C), C.program.mv[0]
        assert sl.length == 21 and codegen.SweepPlan(C.program).mv_generic[0] == 1
        j, b = sl.leaf_base + l, sl.leaf_base + partner
        at = [q for q in range(hp.indptr[j], hp.indptr[j + 1]) if hp.cols[q] == b]
        assert len(at) == 1, (key, "the pair is not stored")
        lst = hp.tlist[hp.tptr[at[0]]:hp.tptr[at[0] + 1]]
        items = hp.terms[hp.owner[at[0]]] - sl.length
        assert sum(1 for t in lst if t >= items) == count, (key, lst)


# ------------------------------------------------------------------------------------------------ 5. the probe's own checks
def test_the_probe_refuses_a_malformed_plan_and_runs_clean_under_the_sanitizers(probe_dir):
    C = mc.case("P2U")
    x, theta, W = C.points[0], C.thetas[-1], mc.weights(C)
    exe = mc.build_probe(C, probe_dir)
    good = mc.run_probe(C, exe, probe_dir, x, W, theta, "good")
    san = mc.build_probe(C, probe_dir, "g++", sanitize=True)
    again = mc.run_probe(C, san, probe_dir, x, W, theta, "san")
    assert _same_bits(again.H, good.H) and np.array_equal(again.S, good.S)
    indptr, cols, owner, tptr, tlist = (a.copy() for a in mc.plan(C).arrays())
    broken = []
    t = tlist.copy()
    t[tptr[1] - 1] = mc.plan(C).terms[owner[0]]        # a term the owner does not have
    broken.append((indptr, cols, owner, tptr, t))
    c = cols.copy()
    c[indptr[3]] = 4                                    # a partner above its row
    broken.append((indptr, c, owner, tptr, tlist))
    o = owner.copy()
    o[0] = C.n - 1 if owner[0] != C.n - 1 and cols[0] != C.n - 1 else 1
    broken.append((indptr, cols, o, tptr, tlist))
    for i, arrays in enumerate(broken):
        data, out = os.path.join(probe_dir, "bad_%d.in" % i), os.path.join(probe_dir, "bad_%d.out" % i)
        mc.probe_input(C, x, W, theta, arrays).tofile(data)
        proc = subprocess.run([exe, data, out], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
        assert proc.returncode == 1 and "BAD PLAN" in proc.stdout, (i, proc.returncode, proc.stdout[-500:])


# ------------------------------------------------------------------------------------------------ 6. host logic
class StandIn:
    """``Problem``'s engine protocol without a device: it records its calls and returns entries that name the lane."""

    def __init__(self, prob, obj):
        C = mc.case("P2U")
        self.n, self.m, self.m_eq = C.n, C.m, 0
        self.plan = mc.plan(C)
        self.theta = np.array(list(prob.parameters.values()), dtype=float)
        self.calls = []

    def set_parameters(self, theta):
        self.theta = np.asarray(theta, dtype=float).copy()

    def values(self, p):
        return np.float64(p[0]), np.zeros(2), np.zeros(self.m - 3)

    def hessian_pattern(self):
        return np.array(self.plan.indptr, dtype=np.int32), np.array(self.plan.cols, dtype=np.int32)

    def entries(self, theta, x, W):
        return np.stack([np.sum(theta) + x[0] + np.sum(w) + np.arange(self.plan.nnz) for w in W])

    def hessian_matrix(self, x, W):
        self.calls.append((self.theta.copy(), np.array(x, dtype=float), np.array(W, dtype=float)))
        return self.entries(self.theta, x, W), np.zeros(self.m)


class NoMatrix(StandIn):
    hessian_matrix = property()         # (hasattr is False)


def _p2u():
    C = mc.case("P2U")
    prob, obj = ec.CASES["P2U"][0]()
    return C, prob, obj, mc.weights(C)


def test_problem_hessian_matrix_on_a_stand_in(monkeypatch):
    monkeypatch.setattr(optimize, "ENGINE_FACTORY", StandIn)
    C, prob, obj, W = _p2u()
    indptr, cols = prob.hessian_pattern(obj)
    assert np.array_equal(indptr, mc.plan(C).indptr) and np.array_equal(cols, mc.plan(C).cols)
    res = prob.hessian_matrix(obj, W)
    eng = prob._engine
    assert res.values.shape == (8, mc.plan(C).nnz) and len(eng.calls) == 1
    assert np.array_equal(eng.calls[0][1], prob.p) and np.array_equal(eng.calls[0][2], W)
    assert np.array_equal(res.values, eng.entries(C.thetas[0], np.asarray(prob.p, dtype=float), W))
    assert np.array_equal(res.indptr, indptr) and np.array_equal(res.cols, cols)
    one = prob.hessian_matrix(obj, W[3])
    assert one.values.shape == (mc.plan(C).nnz,) and np.array_equal(one.values, res.values[3])
    assert one.toarray().shape == (C.n, C.n) and one.tocsr().shape == (C.n, C.n)
    with pytest.raises(ValueError):
        prob.hessian_matrix(obj, W[:, :-1])
    with pytest.raises(ValueError):
        prob.hessian_matrix(obj, np.zeros((2, 2, C.m)))
    monkeypatch.setattr(optimize, "ENGINE_FACTORY", NoMatrix)
    C, prob, obj, W = _p2u()
    with pytest.raises(ValueError):
        prob.hessian_matrix(obj, W)


def test_evaluate_batch_hessians_on_a_stand_in(monkeypatch):
    monkeypatch.setattr(optimize, "ENGINE_FACTORY", StandIn)
    C, prob, obj, W = _p2u()
    X = np.stack([C.points[i % len(C.points)] for i in range(4)])
    res = prob.evaluate_batch(obj, X, hessians=W[:4])
    eng = prob._engine
    assert res.hessian.shape == (4, mc.plan(C).nnz) and len(eng.calls) == 4
    for k in range(4):
        assert np.array_equal(res.hessian[k], eng.entries(C.thetas[0], X[k], W[k:k + 1])[0])
    assert np.array_equal(res.hessian_pattern[0], mc.plan(C).indptr)
    # every lane at its own parameters; one point scanned over them takes its one vector along
    TH = np.stack([C.thetas[i % len(C.thetas)] for i in range(3)])
    eng.calls.clear()
    res = prob.evaluate_batch(obj, X[:1], parameters=TH, hessians=W[2:3])
    assert res.hessian.shape == (3, mc.plan(C).nnz) and [c[0].tolist() for c in eng.calls] == TH.tolist()
    assert all(np.array_equal(c[2], W[2:3]) for c in eng.calls)
    # without the keyword nothing is asked of the engine
    eng.calls.clear()
    res = prob.evaluate_batch(obj, X)
    assert res.hessian is None and res.hessian_pattern is None and not eng.calls
    with pytest.raises(ValueError):
        prob.evaluate_batch(obj, X, hessians=W[:3])
    with pytest.raises(ValueError):
        prob.evaluate_batch(obj, X, hessians=W[:4, :-1])
    monkeypatch.setattr(optimize, "ENGINE_FACTORY", NoMatrix)
    C, prob, obj, W = _p2u()
    with pytest.raises(ValueError):
        prob.evaluate_batch(obj, X, hessians=W[:4])


# ------------------------------------------------------------------------------------------------ 7. the build, the ABI
def test_the_part_has_a_path_of_its_own_and_the_header_is_untouched():
    out = build.module_path("0123456789abcdef")
    assert build.hessian_matrix_part_path(out).endswith("libogk_0123456789abcdef.hess.so")
    assert build.hessian_part_path(out).endswith(".hvp.so")
    paths = {f(out) for f in (build.batch_part_path, build.batch_exact_part_path, build.parameter_part_path,
                              build.directional_part_path, build.adjoint_part_path, build.hessian_part_path,
                              build.mix_part_path, build.hessian_matrix_part_path)}
    assert len(paths) == 8 and build.HESSIAN_MATRIX_PART == 11
    assert os.path.join(build.CSRC, "og_hess.h") in build._kernel_sources()
    C = mc.case("B5")
    mc.plan(C)
    assert codegen.emit_header(C.program) == C.header       # the plan is data: nothing of it is in the header
    assert "tlist" not in C.header and "HESS" not in C.header


def test_c_signatures():
    sig = _native.SIGNATURES
    ip = ctypes.POINTER(ctypes.c_int32)
    assert sig["og_hessian_matrix_load"] == (ctypes.c_int, [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_int32] + [ip] * 5)
    assert sig["og_hessian_matrix_nnz"] == (ctypes.c_int32, [ctypes.c_void_p])
    assert len(sig["og_hessian_matrix_dev"][1]) == 7 and len(sig["og_hessian_matrix"][1]) == 6
    assert len(sig["og_hessian_matrix_batch_dev"][1]) == 7 and len(sig["og_hessian_matrix_batch"][1]) == 6
    header = open(os.path.join(ROOT, "include", "ogpsx.h")).read()
    for name in sig:
        if name.startswith("og_hessian_matrix"):
            assert name + "(" in header, name
