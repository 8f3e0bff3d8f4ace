"""The second-order modes (``csrc/og_hvp.h``, ``csrc/og_hess.h`` on ``csrc/og_dual2.h``) over the whole traced surface,
without a GPU: every problem of ``test_exact_surface.PROBLEMS`` - pairwise and sequential sums, ``cumsum``, ``prod``,
``min`` / ``max`` with ties, ``clip``, ``where``, ``maximum``, table lookups, ``%`` / ``mod``, ``heaviside``, mask
assignment, pre-allocated outputs - at its four named points (``guess``, ``generic``, ``switch`` - exactly on every tie,
knot and jump - and ``minus``), with the eight pairs of ``hessian_cases.pairs``.

1. The referee, ``oracle/exact_hess.py`` (a first-order dual number on complex arrays: no stencil, no second-order rule,
   the branch F(x) takes), before it is trusted: its first-order part is ``oracle.exact_jac``'s Jacobian; where the
   function is smooth it agrees with the Richardson differences of ``hessian_cases.oracle_products`` within ten times
   their own error estimate, no column left out; on ``table_ascent``, whose generic point has kinks inside every
   stencil, it lands on the one-sided limit the probe lands on; its unit-direction products are symmetric.
2. The host probes of the kernels' headers (tests/hvp_probe.cpp, tests/hess_probe.cpp) against it: every column of every
   pair at every point, none excluded, in units of the referee's own ``max(1, sum_r |w_r d2F_r/dx_j dv|)``.

Measured worst per problem (this file writes them to profiles/hessian.md): at most 3.1e-15 on seventeen of the
eighteen and on the gallery; ``SURFACE_MEASURED`` holds each figure and the test asserts four times it, the convention
of ``test_hessian.RULE_BOUNDS``, but never less than ``FLOOR`` (1e-15, four ulp of the unit: the referee runs in double
itself and a figure of 1e-17 is its libraries' last bit).

``kinds_gallery`` (``hessian_cases.Gallery``) is a problem of this file's own with the kinds of node the emitter knows and no surface problem contains (``arctan2``, ``tan``, ``log``, ``arcsin``, ``arccos``,
``fmod``, ``>=`` / ``<=`` / ``!=``, ``&`` / ``|``, a table with ``bounds_error``); the last test checks that nothing is
left out.

``table_ascent`` is the exception: 1.4e-11 against the referee in long double, above the project's 1e-12.  The row is
the acceleration limit ``np.sqrt(a_r ** 2 + a_t ** 2) <= MaxG g0`` at a node (rows 328 to 367), the column the radius
at the same node, worst at nodes 8 to 15.  With ``z = a_r ** 2 + a_t ** 2`` the second derivative of ``sqrt(z)`` along the
radius is ``-z'^2 / (4 z^1.5) + z'' / (2 sqrt z)``; at node 10 of the generic point these two are -23386964722.9 and
+23386965226.3 and leave 503.3 - a cancellation by 5e7 inside ONE row, which no sum over the rows sees.  It is the
conditioning of the callback as written, not a lowering error: the referee in double, which shares no rule with the
kernels, is itself 6e-12 from its own long-double run at the same entries.  (``np.hypot`` would not do it:
``og_dual2.h``'s rule for it forms no such difference.)  So the unit of error stays ``sum_r |w_r d2F_r/dx_j dv|`` - it
does not try to see a cancellation inside one row's expression - and this one problem carries its own measured
figures (``SURFACE_MEASURED``, and ``TRIANGLE_MEASURED`` for the two orientations of a Hessian entry, 1.8e-12: the same
entries) instead of a wider bound for all.

At ``table_ascent``'s guess the speed ``sqrt(vr ** 2 + vt ** 2)`` is exactly 0 at node 0: F has a cone there and no
second derivative.  ``og_dual.h`` takes the slope of ``sqrt`` at 0 as 0 and ``og_dual2.h`` its ``dd`` with it; the
referee follows that convention (``exact_hess._unary``), as it follows the real part at every other switch.
"""
import os

import numpy as np
import pytest

import adjoint_cases as ac
import hessian_cases as hc
import hessian_matrix_cases as mc
import og_math_cases
import test_exact_surface as surface
from opengoddard_amd import codegen
from oracle import exact_hess, exact_jac
from test_hessian import STEP, _note

POINTS = surface.POINTS
KEYS = hc.SURFACE_KEYS + (hc.GALLERY,)          # the surface, and the kinds of node no surface problem contains
SEVEN = hc.GPU_KEYS
SMOOTH_PAIRS = (2, 3, 5, 7)             # neither a unit direction nor the zero pair
LONG_DOUBLE = ("table_ascent",)         # the referee in np.clongdouble: its own rounding is then no part of the figure
# the -fsanitize=address,undefined build of the probes: the device's four shapes and the gallery.  wide_reductions' are
# clang++'s and built ahead by ``__graft_entry__.build`` (``adjoint_cases.SANITIZE_WITH_CLANG`` says why), the others g++'s
SANITIZED = hc.GPU_SURFACE_KEYS + (hc.GALLERY,)
FLOOR = 1e-15                           # four ulp of the unit: no bound below what a library's last bit can move

# the probe's worst difference from the referee per problem, in units of max(1, the referee's own scale)
SURFACE_MEASURED = {
    "bryson_denham": 1.39e-17, "constant_scratch_buffers": 5.55e-17, "preallocated_outputs": 1.55e-16,
    "ragged_two_phase": 1.78e-16, "running_cost_shapes": 4.86e-17, "smooth_knots": 3.33e-16, "wide_functions": 3.05e-15,
    "wide_reductions": 1.68e-16, "layout_0": 3.82e-17, "layout_1": 1.60e-16, "layout_2": 1.99e-16, "layout_3": 1.38e-16,
    "layout_4": 1.90e-16, "layout_5": 1.86e-16, "layout_6": 1.67e-16, "layout_7": 1.84e-16, "layout_8": 1.80e-16,
    "table_ascent": 1.4e-11, "kinds_gallery": 2.36e-16,
}
# the two orientations of a stored Hessian entry, in units of max(1, S): the project's bound except where stated above
TRIANGLE_MEASURED = {"table_ascent": 1.8e-12}


@pytest.fixture(scope="module")
def probe_dir(tmp_path_factory):
    return str(tmp_path_factory.mktemp("hess_surface"))


def _same_bits(a, b):
    return np.array_equal(a, b) and np.array_equal(np.signbit(a), np.signbit(b))


def _at(key, point):
    """``(C, x, theta)``: a surface problem at a named point, one of the seven at its existing point and set."""
    C = hc.case(key)
    if point is None:
        return C, C.points[1], C.thetas[-1]
    return C, hc.named_point(C, point), None


def _points_of(key):
    return POINTS if key in KEYS else (None,)


_REF, _PROBED = {}, {}


def _reference(key, point):
    """``(ref[8, n], scale[8, n], J[m, n])`` of the referee for the eight pairs, once per session."""
    if (key, point) not in _REF:
        C, x, theta = _at(key, point)
        W, V = hc.pairs(C)
        dtype = np.clongdouble if key in LONG_DOUBLE else complex
        _, J, H = exact_hess.second(C.at(theta), C.prob, x, V, dtype=dtype)
        terms = H.astype(np.longdouble) * W.astype(np.longdouble)[:, :, None]
        _REF[key, point] = (terms.sum(axis=1), np.abs(terms).sum(axis=1).astype(float), J.astype(float))
    return _REF[key, point]


def _probed(key, point, probe_dir):
    """The g++ probe of ``og_hvp.h`` for the eight pairs, once per session."""
    if (key, point) not in _PROBED:
        C, x, theta = _at(key, point)
        W, V = hc.pairs(C)
        exe = hc.build_probe(C, probe_dir, "g++")
        _PROBED[key, point] = hc.run_probe(C, exe, probe_dir, x, W, V, theta, "surface_%s" % point)
    return _PROBED[key, point]


# ================================================================================================ 1. the referee
@pytest.mark.parametrize("key", KEYS + SEVEN)
def test_the_referees_first_order_part_is_the_complex_step_jacobian(key):
    """The real part of the dual part against ``exact_jac.jacobian``, all columns, ``surface.BOUND`` of the row's largest
    entry; both are finite first."""
    for point in _points_of(key):
        C, x, theta = _at(key, point)
        ref, scale, J = _reference(key, point)
        JC = exact_jac.jacobian(C.at(theta), C.prob, x)             # J_T [n, m]
        assert np.all(np.isfinite(JC)) and np.all(np.isfinite(J)) and np.all(np.isfinite(ref.astype(float))), (key, point)
        assert surface.worst_error(J.T, JC) <= surface.BOUND, (key, point, surface.worst_error(J.T, JC))


@pytest.mark.parametrize("key", hc.SMOOTH_KEYS + (hc.GALLERY,) + SEVEN)
def test_the_referee_against_differences_of_the_oracle_where_F_is_smooth(key, capsys):
    """The criterion of ``test_hessian.test_the_probe_against_differences_of_the_oracle``: within ten times the
    difference reference's own worst error estimate, in units of the referee's ``max(1, scale)``.  On the surface
    problems no column is left out; the seven keep that test's own rule for a kink inside the stencil."""
    estimate = worst = 0.0
    for point in ([p for p in POINTS if p != "switch"] if key in KEYS else [None]):
        C, x, theta = _at(key, point)
        W, V = hc.pairs(C)
        ref, scale, _ = _reference(key, point)
        for d in SMOOTH_PAIRS:
            fd, err = hc.oracle_products(C, x, W[d:d + 1], V[d], theta, STEP.get(key, hc.H_STEP))
            unit = np.maximum(1.0, scale[d])
            own = err[0] / unit
            keep = np.ones(C.n, dtype=bool)
            if key not in KEYS:
                keep = own <= 1e-6
                assert (~keep).sum() * 50 <= C.n, (key, d, int((~keep).sum()))
            estimate = max(estimate, float(own[keep].max()))
            worst = max(worst, float((np.abs(ref[d] - fd[0]).astype(float) / unit)[keep].max()))
    _note("referee " + key, "difference estimate %.1e, referee %.1e" % (estimate, worst))
    with capsys.disabled():
        if os.environ.get("OG_SURFACE_REPORT"):
            print("referee %-26s estimate %.2e referee %.2e" % (key, estimate, worst))
    assert estimate > 0 and worst <= 10.0 * estimate, (key, estimate, worst)


# (pair, column, the probe's figure when the stencils were taken apart): at the generic point of table_ascent
DISPUTED = [(7, 203, None), (7, 206, -0.58502486), (7, 246, None), (2, 124, None), (2, 84, None), (7, 83, -3398.909)]


def test_on_table_ascent_the_referee_lands_on_the_probes_one_sided_limit(probe_dir):
    """The generic point of ``table_ascent`` sits on kinks: central differences give the mean of the two one-sided
    curvatures there.  One-sided differences of ``exact_jac.jacobian`` (h = 2^-17) name the two limits; in each disputed
    column whose limits differ the probe is on one of them - and the referee must be on the same one, not on the
    other and not on their mean."""
    key, point = "table_ascent", "generic"
    C, x, theta = _at(key, point)
    W, V = hc.pairs(C)
    ref, scale, _ = _reference(key, point)
    r = _probed(key, point, probe_dir)
    h = 2.0 ** -17
    J0 = exact_jac.jacobian(C.program, C.prob, x).astype(np.longdouble)
    sided = 0
    for d in sorted({d for d, _, _ in DISPUTED}):
        wl = W[d].astype(np.longdouble)
        fwd = ((exact_jac.jacobian(C.program, C.prob, x + h * V[d]).astype(np.longdouble) - J0) @ wl / h).astype(float)
        bwd = ((J0 - exact_jac.jacobian(C.program, C.prob, x - h * V[d]).astype(np.longdouble)) @ wl / h).astype(float)
        for dd, j, quoted in DISPUTED:
            if dd != d:
                continue
            got, probe, unit = float(ref[d, j]), r.Q[d, j], max(1.0, scale[d, j])
            assert abs(got - probe) <= 4.0 * SURFACE_MEASURED[key] * unit, (d, j, got, probe)
            if quoted is not None:
                assert abs(got - quoted) <= 1e-6 * abs(quoted), (d, j, got, quoted)
            gap = abs(fwd[j] - bwd[j])
            if gap > 1e-4 * unit:                       # a kink: which side?
                sided += 1
                near, far = sorted((abs(probe - fwd[j]), abs(probe - bwd[j])))
                assert near <= 1e-2 * gap < far, (d, j, probe, fwd[j], bwd[j])
                side = fwd[j] if abs(probe - fwd[j]) < abs(probe - bwd[j]) else bwd[j]
                assert abs(got - side) <= 1e-2 * gap, (d, j, got, fwd[j], bwd[j])
    assert sided >= 2


@pytest.mark.parametrize("key", KEYS)
def test_the_referees_unit_direction_products_are_symmetric(key):
    """Row l of ``exact_hess.hessian`` is the product with ``e_l``; nothing in it makes the matrix symmetric.  Within
    ``BOUND`` of ``max(1, S)`` at every point, the switch point too - and nothing non-zero where no two variables share
    a row of the Jacobian pattern (``codegen.sparsity``)."""
    C = hc.case(key)
    jp, jrows = codegen.sparsity(C.program)
    B = np.zeros((C.n, C.m), dtype=np.int64)
    B[np.repeat(np.arange(C.n), np.diff(jp)), jrows] = 1
    share = B @ B.T > 0
    w = hc.pairs(C)[0][3]
    dtype = np.clongdouble if key in LONG_DOUBLE else complex
    for point in POINTS:
        x = hc.named_point(C, point)
        A, S = exact_hess.hessian(C.program, C.prob, x, w, dtype=dtype)
        assert np.all(np.isfinite(A.astype(float))), (key, point)
        unit = np.maximum(1.0, np.maximum(S, S.T))
        worst = float(np.max(np.abs(A - A.T).astype(float) / unit))
        assert worst <= hc.BOUND, (key, point, worst)
        assert np.any(A != 0) and not np.any(A[~share] != 0), (key, point)


# ================================================================================================ 2. the host probes
@pytest.mark.parametrize("key", KEYS)
def test_the_hvp_probe_against_the_referee_at_every_point(key, probe_dir, capsys):
    """Every column of every pair at the four points, none excluded.  ``Probed.S``, the probe's own sum of the absolute
    values of its terms, is cross-checked against the referee's scale with the same bound."""
    C = hc.case(key)
    bound = max(4.0 * SURFACE_MEASURED[key], FLOOR)
    worst = 0.0
    for point in POINTS:
        ref, scale, _ = _reference(key, point)
        r = _probed(key, point, probe_dir)
        assert np.all(np.isfinite(r.Q)) and np.all(np.isfinite(r.S)), (key, point)
        unit = np.maximum(1.0, scale)
        err = np.abs(r.Q - ref).astype(float) / unit
        here = float(err.max())
        with capsys.disabled():
            if os.environ.get("OG_SURFACE_REPORT"):
                d, j = np.unravel_index(np.argmax(err), err.shape)
                print("surface hvp %-26s %-8s %.2e (pair %d, column %d)" % (key, point, here, d, j))
        worst = max(worst, here)
        assert np.all(np.abs(r.S - scale) <= max(bound, hc.BOUND) * unit), (key, point)
    _note("surface " + key, "%.1e" % worst)
    assert worst <= bound, (key, worst, bound)
    if worst > hc.BOUND:
        assert key == "table_ascent", "above the project's bound: a finding (the module's docstring explains the one known)"


@pytest.mark.parametrize("key", KEYS)
def test_first_order_parts_zeros_and_the_other_compilers_bits(key, probe_dir):
    """What ``test_hessian.test_first_order_parts_are_the_adjoint_probes_bits`` asserts for the seven, at all four
    points: ``G`` is the adjoint probe's bits, the zero pair and every unread column are +0.0, F0 is the adjoint
    probe's; the clang++ build (and on the device's four shapes and the gallery the build with the address and
    undefined-behaviour sanitizers) gives the g++ bits."""
    C = hc.case(key)
    W, V = hc.pairs(C)
    others = [hc.build_probe(C, probe_dir, og_math_cases.clangxx())]
    if key in SANITIZED:
        others.append(_sanitized(hc.build_probe, C, probe_dir))
    adj = ac.build_probe(C, probe_dir, "g++")
    for point in POINTS:
        x = hc.named_point(C, point)
        r = _probed(key, point, probe_dir)
        for other in others:
            o = hc.run_probe(C, other, probe_dir, x, W, V, None, "other")
            assert _same_bits(o.Q, r.Q) and _same_bits(o.G, r.G) and np.array_equal(o.S, r.S), (key, point, other)
        G, F0 = ac.run_probe(C, adj, probe_dir, x, W, None, "surface_adj")
        assert _same_bits(r.G, G) and np.array_equal(r.F0, F0), (key, point)
        assert not r.Q[6].any() and not np.signbit(r.Q[6]).any(), "the zero pair: +0.0 everywhere"
        unread = r.terms == 0
        assert not r.Q[:, unread].any() and not np.signbit(r.Q[:, unread]).any()


def _sanitized(build, C, probe_dir):
    """The probe's build with the sanitizers: from the folder ``build()`` filled where there is one."""
    folder = ac.probe_folder(C, probe_dir) if C.key in ac.SANITIZE_WITH_CLANG else probe_dir
    return build(C, folder, ac.sanitizer_compiler(C.key), sanitize=True)


def _matrix_weights(C):
    W = mc.weights(C)
    return W[[2, 3, 7]] if C.key == "wide_reductions" else W            # (its plan stores 66 918 entries)


@pytest.mark.parametrize("key", [pytest.param(key, marks=pytest.mark.slow) if key == "wide_reductions" else key
                                 for key in KEYS])
def test_the_matrix_probe_is_the_unit_products_bits_inside_the_pattern_only(key, probe_dir):
    """tests/hess_probe.cpp at the four points: every stored entry is the Hessian-vector probe's product with the
    partner's unit direction at the owner, bit for bit; nothing non-zero lies outside the plan's pattern; the other
    orientation agrees within the bound in units of ``S``.  (``wide_reductions``: three weight vectors; its four
    unit-direction runs, 3 x 407 pairs over 407 columns each, and the sanitizer build's run take 60 to 75 s together on
    the 8 cores of the build machine: over a minute, hence the ``slow`` mark on that one case.)"""
    C = mc.case(key)
    W = _matrix_weights(C)
    hp = mc.plan(C)
    row, col, owner, partner = mc.pairs_of(hp)
    stored = np.zeros((C.n, C.n), dtype=bool)
    stored[row, col] = stored[col, row] = True
    exe, unit = mc.build_probe(C, probe_dir), hc.build_probe(C, probe_dir)
    if key in SANITIZED:
        san = _sanitized(mc.build_probe, C, probe_dir)
    bound = max(hc.BOUND, 4.0 * TRIANGLE_MEASURED.get(key, 0.0))
    seen = worst = 0.0
    for point in POINTS:
        x = hc.named_point(C, point)
        r = mc.run_probe(C, exe, probe_dir, x, W, None, "surface_hess")
        Q, S = mc.unit_products(C, unit, probe_dir, x, W, None, "surface_unit")
        assert np.all(np.isfinite(Q)) and np.all(np.isfinite(r.H)), (key, point)
        assert _same_bits(r.H, Q[:, partner, owner]), (key, point, "hvp(w, e_partner)[owner]")
        off = Q[:, ~stored]
        assert not off.any() and not np.signbit(off).any(), (key, point, "an entry outside the pattern is not +0.0")
        assert np.array_equal(r.terms, hp.terms)
        if key in SANITIZED and point == "switch":
            again = mc.run_probe(C, san, probe_dir, x, W, None, "surface_san")
            assert _same_bits(again.H, r.H) and np.array_equal(again.S, r.S)
        other = Q[:, owner, partner]                    # hvp(w, e_owner)[partner]
        worst = max(worst, float(np.max(np.abs(other - r.H) / np.maximum(1.0, r.S))))
        assert np.all(np.abs(other - r.H) <= bound * np.maximum(1.0, r.S)), (key, point, worst)
        seen = max(seen, float(r.S.max()))
    assert seen > 0
    _note("surface triangles " + key, "%.1e" % worst)
    if worst > hc.BOUND:
        assert key == "table_ascent", "above the project's bound: a finding (the module's docstring explains the one known)"


# ================================================================================================ 3. coverage
def node_kinds(P):
    """The kinds of element-graph node reachable from the program's rows and collocation operands, as ``codegen``'s
    emitter distinguishes them: a tag, with the operation of a ``un`` / ``bin`` / ``cmp`` / ``logic`` node and the mode
    of a table."""
    seen, out = set(), set()
    stack = [e for _, _, e, _ in P.pieces] + [sl.operand for sl in P.mv]
    while stack:
        e = stack.pop()
        if e in seen:
            continue
        seen.add(e)
        node = P.eg.nodes[e]
        tag = node[0]
        if tag in ("un", "bin", "cmp", "logic"):
            out.add(tag + ":" + node[1])
        elif tag == "interp":
            out.add("interp:%d" % P.tables[node[1]][2])
        elif tag == "CV":
            out.add("CV:parameter" if node[1] == P.par_table and node[3] == 0 else "CV")
        else:
            out.add(tag)
        stack.extend(codegen._children(node))
        if tag == "sum":
            stack.extend(body for _, body in node[1])
    return out


def test_the_second_order_tests_reach_every_kind_of_node_codegen_can_emit():
    """The union over the problems of this file holds every tag the emitter knows, every operation of ``_UN_C``, ``_BIN_C``
    (with ``max`` / ``min``, emitted as ternaries), ``_CMP_C`` and both logical ones, and every table mode; a run-time
    parameter (``par_leaf``) comes from ``P2U`` and ``G17`` among the seven, no surface problem has one.  A kind added to
    the emitter without a problem here fails this test: the tags are read from the source of ``_emit_expr`` (a
    collocation product, ``Y``, is the one tag it never sees), the operations from its tables; only the three table modes
    are written down here, as in ``trace.intercept_interp1d``."""
    import inspect
    import re
    tags = set(re.findall(r'tag == "(\w+)"', inspect.getsource(codegen._Emitter._emit_expr))) | {"Y"}
    assert tags == {"P", "C", "CV", "Y", "un", "interp", "bin", "cmp", "logic", "where", "sum"}, sorted(tags)
    can = {"P", "C", "CV", "CV:parameter", "Y", "where", "sum", "logic:and", "logic:or", "interp:0", "interp:1", "interp:2"}
    can |= {"un:" + op for op in codegen._UN_C} | {"bin:" + op for op in list(codegen._BIN_C) + ["max", "min"]}
    can |= {"cmp:" + op for op in codegen._CMP_C}
    seen = {key: node_kinds(hc.case(key).program) for key in KEYS + SEVEN}
    here = set().union(*(seen[key] for key in KEYS))
    assert "CV:parameter" in seen["P2U"] and "CV:parameter" in seen["G17"]
    assert can - here == {"CV:parameter"}, sorted(can - here - {"CV:parameter"})
    assert set().union(*seen.values()) == can, sorted(set().union(*seen.values()) - can)
    # what the issue names: reductions (a sum node, and min / max folded pairwise), tables, where / mask, mod, cumsum
    surface_only = set().union(*(seen[key] for key in hc.SURFACE_KEYS))
    assert {"sum", "bin:max", "bin:min", "interp:0", "interp:1", "where", "bin:mod", "cmp:eq"} <= surface_only
    gallery = seen[hc.GALLERY]
    assert can - surface_only - {"CV:parameter"} <= gallery, sorted(can - surface_only - gallery)
