"""Exact-Jacobian mode (``jacobian="exact"``: ``og_dual.h``, ``ogk_exact_struct``, ``ogk_exact``,
``ogk_exact_struct_batch``) over the whole traced surface: the 8 edge problems, the 9 random layouts and the table
problem, at four named points each - the guess, a generic point, a point whose chosen variables sit EXACTLY on the
callbacks' switches (``np.where`` thresholds, ties of ``maximum`` / ``min`` / ``max``, both edges of ``np.clip``, table
knots and table ends, the jumps of ``%``, ``abs`` / ``heaviside`` at 0) and a fourth generic point for the batch.

CPU: the twin against complex-step differentiation of the lowered program (``oracle/exact_jac.py``, which shares
neither the generated header nor ``og_dual.h`` with it), all columns, 1e-12 of the row's largest entry - the bound of
``test_exact_jacobian.test_twin_exact_jacobian_of_the_widened_function_set``; and the complex-step Jacobian has no
non-zero outside ``codegen.sparsity``'s pattern.  At a switch the derivative is that of the branch F(x) takes
(DESIGN section 9): both sides choose it from the value at the point.  Every point is one where F and the complex-step
Jacobian are finite; the tests assert that first.

GPU: the structured and the dense exact kernels bit for bit against the twin (full matrix and column ranges), against
the complex step directly, into a registered buffer that an FD sweep left full of NaN, and as lanes of a batch.

The worst figures per problem and point are in profiles/exact_surface.md."""
import os

import numpy as np
import pytest

import test_edge_problems
import test_random_layouts
from opengoddard_amd import _native, codegen, problems
from oracle import exact_jac, np_path, twin
from test_exact_jacobian import _points
from test_module_limits import gather

EDGE = sorted(test_edge_problems.CASES)
LAYOUTS = ["layout_%d" % seed for seed, _ in test_random_layouts.CASES]
PROBLEMS = EDGE + LAYOUTS + ["table_ascent"]
POINTS = ("guess", "generic", "switch", "minus")
BATCHED = ["wide_functions", "running_cost_shapes", "wide_reductions", "ragged_two_phase", "layout_5"]   # batch test
BOUND = 1e-12            # of the row's largest entry (test_twin_exact_jacobian_of_the_widened_function_set)

# ------------------------------------------------------------------------------------------------ the switch recipes
# (block, index of the state / control, phase, nodes, physical value): the variable is set so that the callbacks see
# exactly ``value`` (``surface_points`` finds the scaled number whose product with the unit is that value to the bit).
S, U = "state", "control"
SWITCHES = {
    # u ** 2 at exactly 0 (the power rule's 0 * x ** -1 side) and sin at 0: no switch, but an exact special value
    "bryson_denham": [(U, 0, 0, (4, 11), 0.0), (S, 0, 0, (9,), 0.0)],
    "constant_scratch_buffers": [(U, 0, 0, (1, 3), 0.0)],
    "smooth_knots": [(S, 0, 0, (2,), 0.0), (S, 0, 1, (0, 5), 0.0)],
    "running_cost_shapes": [(U, 0, 0, (3,), 0.0), (U, 0, 1, (36,), 0.0), (S, 1, 1, (7,), 0.0)],
    "ragged_two_phase": [
        (U, 0, 0, (0, 2, 4, 6), 0.2), (U, 0, 1, (0, 2, 4), 0.2),      # np.where(u > 0.2, ...) on its threshold
        (S, 2, 1, (1, 2), 0.5),                                       # tie of np.maximum(., 0.5)
    ],
    "wide_reductions": [
        (U, 0, 0, (5, 40), 1.0), (U, 0, 0, (6, 41), -1.0),            # both edges of np.clip
        (U, 0, 1, (2,), 1.0), (U, 0, 1, (3,), -1.0),
        (S, 0, 0, (10,), -0.5), (S, 0, 0, (11, 50), 0.0), (S, 0, 1, (4,), 0.7),      # table knots
        (S, 0, 0, (20, 70), -2.5),            # below the table's first knot, and the two equal smallest of x
        (S, 0, 1, (30,), 3.5),                # above its last knot
        (S, 1, 0, (15,), 1.75), (S, 1, 1, (8,), 1.75),                # two equal largest of v
        (U, 0, 0, (60,), 1.5), (U, 0, 1, (20,), 1.5),                 # two equal largest of u
        (U, 0, 0, (3,), 0.0),                                         # abs at 0 under the cumsum
    ],
    "preallocated_outputs": [
        (S, 1, 0, (3, 10), 0.0),                                      # np.heaviside(v, 0.5) at 0
        (S, 0, 0, (5,), 0.37), (S, 0, 0, (11,), 0.74), (S, 0, 0, (13,), -0.6),       # the jumps of % and np.mod
        (S, 0, 0, (6,), 0.0),                                         # abs at 0 among x[4:8], and % at 0
        (S, 0, 0, (2,), 0.5), (U, 0, 0, (2,), 0.25),                  # table column 2: u == x ** 2, tie of max(axis=0)
    ],
    "wide_functions": [
        (U, 0, 0, (2, 7), 0.5),                                       # tanh's centre
        (U, 1, 0, (4, 9), 0.0),                                       # w = 0 with v > 0: hypot and cbrt off the origin
    ],
    # altitude exactly on the first knot (0 m), an interior knot (7 km), a knot of the coarse part (40 km) and the
    # last knot (85 km) of the density and sound-speed tables
    "table_ascent": [(S, 0, 0, (0,), 6371000.0), (S, 0, 0, (7,), 6378000.0), (S, 0, 0, (20,), 6411000.0),
                     (S, 0, 0, (33,), 6456000.0)],
}


def _layout_switches(prob):
    """Random layouts: every state of every phase is exactly 0.1 at node 1 and exactly -0.25 at node 2 (the
    thresholds of kinds 6 and 7 of ``test_random_layouts._term``, whichever states the plan applies them to)."""
    out = []
    for phase in range(prob.number_of_section):
        for s in range(prob.number_of_states[phase]):
            out += [(S, s, phase, (1,), 0.1), (S, s, phase, (2,), -0.25)]
    return out


def _scaled(value, unit):
    """The float q with ``q * unit == value`` to the bit (what the callbacks compute from the scaled variable)."""
    q = value / unit
    for cand in (q, np.nextafter(q, np.inf), np.nextafter(q, -np.inf), np.nextafter(np.nextafter(q, np.inf), np.inf),
                 np.nextafter(np.nextafter(q, -np.inf), -np.inf)):
        if cand * unit == value:
            return float(cand)
    raise AssertionError("no float times %r gives %r exactly: choose another value" % (unit, value))


def build_problem(name):
    if name in test_edge_problems.CASES:
        return test_edge_problems.CASES[name]()
    if name.startswith("layout_"):
        seed = int(name[7:])
        return test_random_layouts.make_problem(test_random_layouts.SHAPES[seed], seed)
    return problems.build(name)


def surface_points(name, prob):
    """The named points of one problem: ``guess`` (the clipped guess), ``generic`` (``test_exact_jacobian._points``'
    second point), ``switch`` (the generic point with the recipe's variables exactly on the switches) and ``minus``
    (the generic perturbation with the other sign, the batch's fourth lane)."""
    lb, ub = np_path.bounds_arrays(prob)
    x0, x1 = _points(prob, lb, ub)
    rng = np.random.default_rng(3)                        # _points' own draws, taken with the other sign
    a, b = rng.standard_normal(x0.size), rng.standard_normal(x0.size)
    minus = np.clip(x0 * (1.0 - 1e-3 * a) - 1e-4 * b, lb, ub)
    recipe = _layout_switches(prob) if name.startswith("layout_") else SWITCHES[name]
    xs = x1.copy()
    for block, idx, phase, nodes, value in recipe:
        unit = (prob.unit_states if block == S else prob.unit_controls)[phase][idx]
        index = prob.index_states if block == S else prob.index_controls
        for node in nodes:
            xs[index(idx, phase, node)] = _scaled(value, unit)
    assert recipe and not np.array_equal(xs, x1)
    return {"guess": x0, "generic": x1, "switch": xs, "minus": minus}


class Surface:
    """One problem: traced program, twin, the four points and, computed once and never changed, the complex-step
    Jacobian over all columns at each of them."""

    def __init__(self, name):
        self.name = name
        self.prob, self.obj = build_problem(name)
        self.program = codegen.trace_problem(self.prob, self.obj)
        self.tw = twin.Twin(self.prob, self.obj, program=self.program)
        self.points = surface_points(name, self.prob)
        self._jc, self._exact = {}, {}
        indptr, rows = codegen.sparsity(self.program)
        self.mask = np.zeros((self.program.n, self.program.m), dtype=bool)
        self.mask[np.repeat(np.arange(self.program.n), np.diff(indptr)), rows] = True

    def complex_step(self, point):
        if point not in self._jc:
            JC = exact_jac.jacobian(self.program, self.prob, self.points[point])
            JC.setflags(write=False)
            self._jc[point] = JC
        return self._jc[point]

    def exact(self, point):
        if point not in self._exact:
            F0, JE = self.tw.exact(self.points[point])
            F0.setflags(write=False), JE.setflags(write=False)
            self._exact[point] = (F0, JE)
        return self._exact[point]


_SURFACES = {}


def surface(name):
    if name not in _SURFACES:
        _SURFACES[name] = Surface(name)
    return _SURFACES[name]


def worst_error(JE, JC):
    scale = np.maximum(1.0, np.abs(JC).max(axis=0))[None, :]
    return float(np.max(np.abs(JE - JC) / scale))


# ================================================================================================ CPU
@pytest.mark.parametrize("name", PROBLEMS)
def test_every_point_is_finite_and_the_switch_point_sits_on_its_switches(name):
    """The condition on every point, before anything else: ``np_path.stacked_values`` and the complex-step Jacobian
    are finite everywhere.  And the recipe did what it says: the callbacks' getters return the recipe's values to the
    bit at the switch point."""
    R = surface(name)
    for point in POINTS:
        x = R.points[point]
        assert np.all(np.isfinite(np_path.stacked_values(R.prob, R.obj, x))), (name, point)
        assert np.all(np.isfinite(R.complex_step(point))), (name, point)
    recipe = _layout_switches(R.prob) if name.startswith("layout_") else SWITCHES[name]
    keep = R.prob.p
    try:
        R.prob.p = R.points["switch"].copy()
        for block, idx, phase, nodes, value in recipe:
            got = (R.prob.states if block == S else R.prob.controls)(idx, phase)
            assert all(float(got[node]) == value for node in nodes), (name, block, idx, phase, nodes, value)
        if name == "wide_functions":
            assert np.all(np.asarray(R.prob.states(1, 0))[[4, 9]] > 0)          # hypot / cbrt off the origin
    finally:
        R.prob.p = keep


@pytest.mark.parametrize("name", PROBLEMS)
def test_twin_exact_jacobian_matches_complex_step_over_the_surface(name, capsys):
    """All columns at every point: within 1e-12 of the row's largest entry, and F0 is ``tw.values(x)`` to the bit.
    Measured (profiles/exact_surface.md): at most 4.5e-16 on the 18 problems."""
    R = surface(name)
    for point in POINTS:
        x = R.points[point]
        F0, JE = R.exact(point)
        assert np.array_equal(F0, R.tw.values(x)), (name, point)
        assert np.all(np.isfinite(JE)), (name, point)
        err = worst_error(JE, R.complex_step(point))
        with capsys.disabled():
            if os.environ.get("OG_SURFACE_REPORT"):
                print("surface %-26s %-8s %.2e" % (name, point, err))
        assert err <= BOUND, (name, point, err)


@pytest.mark.parametrize("name", PROBLEMS)
def test_nothing_depends_on_a_variable_outside_the_traced_pattern(name):
    """The complex-step Jacobian over all columns has no non-zero outside ``codegen.sparsity``'s pattern, at the
    guess, the generic and the switch point: what every structured kernel, the registered buffers and the packed
    batch results rely on when they write pattern entries only."""
    R = surface(name)
    for point in ("guess", "generic", "switch"):
        JC = R.complex_step(point)
        outside = np.argwhere((JC != 0) & ~R.mask)
        assert outside.size == 0, "%s at %s: F[%d] depends on x[%d], which the pattern leaves out" % (
            name, point, outside[0][1], outside[0][0])


# ================================================================================================ GPU
@pytest.fixture(scope="module")
def engines():
    """One engine per (problem, sweep layout), compiled once and closed when the module is done."""
    from opengoddard_amd.engine import HipEngine
    made = {}

    def get(name, layout="structured"):
        if (name, layout) not in made:
            R = surface(name)
            before = os.environ.get("OGPSX_SWEEP")
            if layout == "dense":
                os.environ["OGPSX_SWEEP"] = "dense"
            try:
                made[name, layout] = HipEngine(R.prob, R.obj, program=R.program)
            finally:
                if layout == "dense":
                    if before is None:
                        del os.environ["OGPSX_SWEEP"]
                    else:
                        os.environ["OGPSX_SWEEP"] = before
        return made[name, layout]

    yield get
    for eng in made.values():
        eng.close()


def column_ranges(R):
    """[0, 1); the final-time columns alone; a range inside one group of 16 neighbouring columns of a node tile (the
    second tile of state 0 of phase 0 where the phase has one); the empty range."""
    n, phases = R.program.n, len(R.prob.nodes)
    base, N = R.prob.index_states(0, 0, 0), R.prob.nodes[0]
    tile = 16 if N >= 24 else 0
    lo = base + tile + min(2, N - 2)
    hi = min(lo + 5, base + min(N, tile + 15))
    assert base <= lo < hi <= base + N and (lo - base) // 16 == (hi - 1 - base) // 16
    return [(0, 1), (n - phases, n), (lo, hi), (1, 1)]


def _check_against_twin(R, eng):
    for point in POINTS:
        x = R.points[point]
        F0c, JEc = R.exact(point)
        F0, JE = eng.exact_stacked(x)
        assert np.array_equal(F0, F0c) and np.array_equal(F0, eng.eval_stacked(x)), (R.name, point)
        differ = np.argwhere(JE != JEc)
        assert differ.size == 0, "%s at %s: column %d, row %d: device %r, twin %r" % (
            R.name, point, differ[0][0], differ[0][1], JE[tuple(differ[0])], JEc[tuple(differ[0])])
        for lo, hi in column_ranges(R):
            F0r, part = eng.exact_stacked(x, lo, hi)
            assert part.shape == (hi - lo, eng.m) and np.array_equal(part, JEc[lo:hi]), (R.name, point, lo, hi)
            assert np.array_equal(F0r, F0c)


@pytest.mark.gpu
@pytest.mark.parametrize("name", PROBLEMS)
def test_gpu_structured_exact_kernel_is_bit_identical_to_the_twin(name, engines):
    """``ogk_exact_struct`` at every point: F0, the full matrix and the column ranges; and the same matrix against
    the complex step directly, with the CPU test's bound."""
    R = surface(name)
    eng = engines(name)
    assert eng.sweep_mode != "dense"
    _check_against_twin(R, eng)
    for point in POINTS:
        _, JE = eng.exact_stacked(R.points[point])
        assert worst_error(JE, R.complex_step(point)) <= BOUND, (name, point)


@pytest.mark.gpu
@pytest.mark.parametrize("name", EDGE)
def test_gpu_dense_exact_kernel_is_bit_identical_to_the_twin(name, engines):
    """``ogk_exact`` (OGPSX_SWEEP=dense: every row item for every column) on the edge problems, a second engine."""
    R = surface(name)
    eng = engines(name, "dense")
    assert eng.sweep_mode == "dense"
    _check_against_twin(R, eng)
    _, JE = eng.exact_stacked(R.points["switch"])
    assert worst_error(JE, R.complex_step("switch")) <= BOUND


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["running_cost_shapes", "wide_reductions"])
def test_gpu_exact_into_a_registered_buffer_after_a_non_finite_sweep(name, engines):
    """An FD sweep at a point with a NaN state fills the registered buffer's rows with NaN; the exact call at the
    switch point into the same buffer must leave the twin's exact matrix: the fill cleaned, every structural zero an
    exact zero."""
    import torch
    R = surface(name)
    eng = engines(name)
    lb, ub = np_path.bounds_arrays(R.prob)
    n, m = eng.n, eng.m
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream().cuda_stream
    x_bad = R.points["generic"].copy()
    x_bad[R.prob.index_states(1, 0, 7)] = np.nan
    h = _native.fd_step(R.points["generic"], lb, ub)
    d_F = torch.empty(m, dtype=torch.float64, device=dev)
    reg = torch.full((n, m), 7.0, dtype=torch.float64, device=dev)              # garbage before registration
    eng.register_jt_dev(reg.data_ptr(), 0, n, stream)
    try:
        d_x, d_h = torch.from_numpy(x_bad).to(dev), torch.from_numpy(h).to(dev)
        eng.sweep_dev(d_x.data_ptr(), d_h.data_ptr(), 0, n, reg.data_ptr(), d_F.data_ptr(), stream)
        torch.cuda.synchronize()
        assert np.isnan(reg.cpu().numpy()).any() and eng.nonfinite_rows(stream) > 0
        d_x = torch.from_numpy(R.points["switch"]).to(dev)
        eng.exact_dev(d_x.data_ptr(), 0, n, reg.data_ptr(), d_F.data_ptr(), stream)
        torch.cuda.synchronize()
        F0c, JEc = R.exact("switch")
        got = reg.cpu().numpy()
        assert np.array_equal(d_F.cpu().numpy(), F0c)
        assert np.array_equal(got, JEc)
        assert not got[~R.mask].any() and not np.signbit(got[~R.mask]).any()
    finally:
        eng.unregister_jt_dev(reg.data_ptr())


@pytest.mark.gpu
@pytest.mark.parametrize("name", BATCHED)
def test_gpu_batch_exact_lanes_equal_the_single_point_calls(name, engines):
    """``ogk_exact_struct_batch`` with B = 4 lanes (guess, generic, switch, minus): every lane's F and packed values are
    the single-point call's, gathered through the pattern - on problems with one phase (n = 71), two phases whose
    running cost reads a final time (n = 173), 135 nodes (n = 407), ragged phases (n = 48) and three phases (n = 174):
    n is a multiple of 4 and is not, and the final-time (heavy) columns number 1, 2 and 3."""
    R = surface(name)
    eng = engines(name)
    batch = eng.batch(4)
    try:
        P = np.stack([R.points[point] for point in POINTS])
        F0, vals, nonfinite = batch.exact(P)
        assert not nonfinite.any()
        for k, point in enumerate(POINTS):
            F0s, JEs = eng.exact_stacked(P[k])
            assert np.array_equal(F0[k], F0s), (name, point)
            assert np.array_equal(vals[k], gather(eng.program, JEs)), (name, point)
            assert np.array_equal(vals[k], gather(eng.program, R.exact(point)[1])), (name, point)
    finally:
        batch.close()
