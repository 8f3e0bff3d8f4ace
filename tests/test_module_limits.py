"""The limits of a callback module, from both sides.

A module runs evaluation + structured sweep as ONE launch only while the longest phase fits the LDS window of
``ogk_fused`` (``ogk_info.fused_ok``; the arithmetic is restated in ``codegen.lds_window``).  Beyond the window the
handle keeps ``og_sweep_mode == 5`` and takes other routes through the runtime - two launches, a full download for a
registered host matrix, sweep + pack for a shard, one batched evaluation and a sweep per lane for a batch - which no
BASELINE configuration and none of the nine shapes of tests/test_random_layouts.py ever visits.  This module places
randomly composed problems (``test_random_layouts.make_problem``) on either side of every edge and asks both sides
for the CPU twin's bits:

====================  ====================================================================================
fit / do not fit      1 state, no control: 452 / 453 nodes;  16 states, 1 control: 168 / 169 nodes;
                      6 states, 3 controls, two phases, running cost on: [280, 40] / [281, 40] nodes (only the
                      first phase crosses; the running cost's cached sum terms, N_TERMS = 320 / 321, move the
                      edge from 292 / 293 to 280 / 281)
MFMA A operand        16, 13 and 9 states on 17 and on 33 nodes (full and partly filled state rows)
phase count           32 phases of 3 - 5 nodes fit; 33 are refused
evaluation LDS        16 states on 248 nodes use 65 536 bytes and run (two launches); 16 states on 632 nodes use all
                      163 840 bytes of a compute unit (evaluation only: its J_T would be 1 GB); 633 nodes are refused
                      before anything is compiled
====================  ====================================================================================

The mirror (``codegen.lds_window``) and ``ogk_get_info`` of the compiled modules are compared with each other on the
CPU, for every shape here.  Two limits are in play.  64 KiB is the one-launch window: the choice of two ``ogk_fused``
workgroups per compute unit, not a limit of the hardware.  The evaluation kernels ask for their dynamic LDS at any
phase length, and a workgroup of gfx950 can have the compute unit's whole 160 KiB: ``launch4`` on 341 nodes per phase
(8 states per phase, 86*(64 + 32) + 256 doubles = 68 096 bytes) runs beyond 64 KiB in tests/test_gpu_solve.py, and 16
states on 249 nodes (66 560 bytes) are a legal shape like it.  The named refusal (``codegen.check_limits``, and
``eval_lds_fits`` in the module's launcher) is at 160 KiB: 632 | 633 nodes at 16 states.

Every GPU test asserts ``eng.one_launch == codegen.lds_window(program)["one_launch"]``: a test that believes it is at
an edge when it is not fails.  Where the twin's or the NumPy oracle's full sweep would be slow, a SPREAD of columns is
compared: the first and the last column of every state block and every control block, four more inside each block,
and every phase-time column (``spread_columns``; the count goes to the measurement record).
"""
import ctypes as C
import os
import time

import numpy as np
import pytest

from conftest import assert_zero_pattern, fd_noise_bound, record_measurement
from opengoddard_amd import _native, build, codegen, trace
from oracle import np_path, program_eval, twin
from test_random_layouts import make_problem

# key -> (shape of test_random_layouts.make_problem, seed); an even seed turns the running cost on
SHAPES = {
    "s1_n452": (([452], [1], [0], []), 11),
    "s1_n453": (([453], [1], [0], []), 11),
    "s16_n168": (([168], [16], [1], []), 13),
    "s16_n169": (([169], [16], [1], []), 13),
    "s6_n280_40": (([280, 40], [6, 6], [3, 3], [True]), 12),
    "s6_n281_40": (([281, 40], [6, 6], [3, 3], [True]), 12),
    "s16_n17": (([17], [16], [1], []), 21),
    "s16_n33": (([33], [16], [1], []), 22),
    "s13_n17": (([17], [13], [2], []), 23),
    "s13_n33": (([33], [13], [2], []), 24),
    "s9_n17": (([17], [9], [1], []), 25),
    "s9_n33": (([33], [9], [1], []), 26),
    "p32": (([4, 3, 5] * 10 + [4, 3], [2] * 32, [1] * 32, [True, False] * 15 + [True]), 32),
    "s16_n248": (([248], [16], [1], []), 13),
    "s16_n632": (([632], [16], [1], []), 13),
}
EDGE_PAIRS = [("s1_n452", "s1_n453"), ("s16_n168", "s16_n169"), ("s6_n280_40", "s6_n281_40")]
FITTING_EDGES = [a for a, _ in EDGE_PAIRS]
NOT_FITTING = [b for _, b in EDGE_PAIRS] + ["s16_n248"]
OPERAND = ["s16_n17", "s16_n33", "s13_n17", "s13_n33", "s9_n17", "s9_n33"]
ONE_LAUNCH = FITTING_EDGES + OPERAND + ["p32"]
OVER_THE_EVALUATION_LDS = (([633], [16], [1], []), 13)
PHASES_33 = (([4, 3, 5] * 11, [2] * 33, [1] * 33, [True] * 32), 32)
STATES_17 = (([9], [17], [1], []), 5)
BAD_NODE = 2            # state 0 of phase 0 is put below -2 at this node: sqrt(x + 2) is NaN there


def problem(key):
    shape, seed = SHAPES[key]
    return make_problem(shape, seed, sqrt_term=True)


def spread_columns(prob, inside=4):
    """First and last column of every state and control block, ``inside`` more in between, every phase-time column."""
    cols = set()
    for i, N in enumerate(prob.nodes):
        picks = np.unique(np.r_[0, N - 1, np.linspace(0, N - 1, inside + 2).astype(int)])
        for s in range(prob.number_of_states[i]):
            cols |= {prob.index_states(s, i, int(k)) for k in picks}
        for c in range(prob.number_of_controls[i]):
            cols |= {prob.index_controls(c, i, int(k)) for k in picks}
    S = len(prob.nodes)
    cols |= set(range(prob.number_of_variables - S, prob.number_of_variables))
    return np.array(sorted(cols), dtype=np.int32)


def row_scales(program, prob, x, F):
    """Magnitude of the terms summed in each row (tests/test_gpu_parity.py: defect rows sum_l |D_kl| |x_l|)."""
    scale = np.maximum(1.0, np.abs(F))
    for g in program.groups:
        if g.kind != "defect":
            continue
        D = np.abs(prob.D[g.phase])
        for (row, _), slot in zip(g.outputs, g.mv_slots):
            leaf = program.mv[slot].leaf_base
            scale[row:row + g.length] = np.maximum(scale[row:row + g.length], D.dot(np.abs(x[leaf:leaf + g.length])))
    return scale


class Ref:
    """One shape's problem, traced program, points, CPU twin and the twin's results, each made once."""

    def __init__(self, key):
        self.key = key
        self.prob, self.obj = problem(key)
        self.program = codegen.trace_problem(self.prob, self.obj)
        self.header = codegen.emit_header(self.program)
        self.window = codegen.lds_window(self.program)
        self.lb, self.ub = np_path.bounds_arrays(self.prob)
        x_ok = np.clip(self.prob.p, self.lb, self.ub)
        x_bad = x_ok.copy()
        x_bad[self.prob.index_states(0, 0, BAD_NODE)] = -10.0         # (units of 0.5 - 3: -5 or less)
        rng = np.random.default_rng(5)
        x_other = np.clip(x_ok + 1e-3 * rng.standard_normal(x_ok.size), self.lb, self.ub)
        self.x = {"ok": x_ok, "bad": x_bad, "other": x_other}
        self.h = {k: _native.fd_step(v, self.lb, self.ub) for k, v in self.x.items()}
        self._twin = None
        self._sweeps, self._exact = {}, {}
        self.cols = spread_columns(self.prob)
        self.t0 = time.time()

    @property
    def tw(self):
        if self._twin is None:
            self._twin = twin.Twin(self.prob, self.obj, program=self.program, header=self.header)
        return self._twin

    def sweep(self, name):
        """The twin's (F0, J_T) over ALL columns at point ``name``."""
        if name not in self._sweeps:
            self._sweeps[name] = self.tw.sweep(self.x[name], self.h[name])
            assert np.isfinite(self._sweeps[name][0]).all() == (name != "bad"), "the bad point must be the non-finite one"
        return self._sweeps[name]

    def exact(self, name):
        if name not in self._exact:
            self._exact[name] = self.tw.exact(self.x[name])
        return self._exact[name]

    def engine(self):
        from opengoddard_amd.engine import HipEngine
        eng = HipEngine(self.prob, self.obj, program=self.program)
        assert eng.one_launch == self.window["one_launch"], "the mirror and ogk_get_info disagree on %s" % self.key
        return eng

    def record(self, test, eng, columns, **more):
        indptr, _ = codegen.sparsity(self.program)
        record_measurement(test, shape=self.key, one_launch=int(eng.one_launch), eval_bytes=self.window["eval_bytes"],
                           fused_bytes=self.window["fused_bytes"], fill_bytes=self.window["fill_bytes"], n=eng.n,
                           m=eng.m, nnz=int(indptr[-1]), columns=int(columns), seconds=time.time() - self.t0, **more)


_REF = {}


def ref(key):
    """The shape's reference data; one shape is kept at a time (a full J_T of the largest shape is 159 MB)."""
    if key not in _REF:
        _REF.clear()
        _REF[key] = Ref(key)
    _REF[key].t0 = time.time()
    return _REF[key]


def gather(program, JT):
    indptr, rows = codegen.sparsity(program)
    return JT[np.repeat(np.arange(program.n), np.diff(indptr)), rows]


# ================================================================================================ CPU
@pytest.mark.parametrize("key", list(SHAPES))
def test_cpu_chain_on_the_limit_shapes(key):
    """The chain of ``test_random_layout_cpu_chain`` with its bounds: traced program against ``np_path`` bit for bit,
    twin against ``np_path``; the sweep on the spread of columns (32 - 200 columns, ``spread_columns``)."""
    R = ref(key)
    prob, obj, P = R.prob, R.obj, R.program
    x, h = R.x["ok"], R.h["ok"]
    F = np_path.stacked_values(prob, obj, x)
    assert np.array_equal(program_eval.evaluate(P, prob, x), F)
    assert np.all(np.abs(R.tw.values(x) - F) <= 1e-11 * np.maximum(1.0, np.abs(F)) + 1e-9)
    assert np.array_equal(h, np_path.fd_step(x, R.lb, R.ub))
    cols = R.cols
    _, JT = R.tw.sweep(x, h, cols)
    _, _, JTo = np_path.sweep(prob, obj, x, list(cols))
    scale = np.maximum(1.0, np.abs(F)) + 50.0 * max(np.abs(D).max() for D in prob.D)
    bound = 1e-9 * np.abs(JTo) + 64 * np.finfo(float).eps * scale[None, :] / np.abs(h[cols])[:, None]
    assert np.all(np.abs(JT - JTo) <= bound)
    # the non-finite point of the GPU tests is one: the sqrt term, and nothing else, is NaN there
    Fb = R.tw.values(R.x["bad"])
    assert np.array_equal(np.isfinite(Fb), np.isfinite(np_path.stacked_values(prob, obj, R.x["bad"])))
    assert 1 <= np.sum(~np.isfinite(Fb)) <= 2 and np.isfinite(R.tw.values(R.x["other"])).all()


def test_the_mirror_puts_every_edge_pair_on_opposite_sides():
    for fits, does_not in EDGE_PAIRS:
        a, b = ref(fits).window, ref(does_not).window
        assert a["one_launch"] and not b["one_launch"] and a["eval_fits"] and b["eval_fits"], (fits, does_not)
        assert a["fused_bytes"] <= codegen.LDS_BYTES < b["fused_bytes"]
    w = ref("s16_n248").window
    assert w["eval_bytes"] == codegen.LDS_BYTES and w["eval_fits"] and not w["one_launch"]
    w = ref("s16_n632").window
    assert w["eval_bytes"] == codegen.EVAL_LDS_BYTES == 163840 and w["eval_fits"] and not w["one_launch"]
    for shape, fits in ((([249], [16], [1], []), True), (OVER_THE_EVALUATION_LDS[0], False)):
        prob, obj = make_problem(shape, 13)
        assert codegen.lds_window(codegen.trace_problem(prob, obj))["eval_fits"] == fits
    assert ref("s6_n280_40").window["n_terms"] == 320 and ref("s6_n281_40").window["term_doubles"] == 321 + 16
    for key in OPERAND + ["p32"]:
        assert ref(key).window["one_launch"], key
    assert [codegen.max_phase_nodes(s) for s in (1, 2, 6, 8, 16)] == [1188, 1120, 916, 840, 632]


@pytest.mark.parametrize("states,controls,seed", [(1, 0, 11), (2, 1, 11), (6, 3, 11), (16, 1, 13)])
def test_the_window_is_monotone_in_the_node_count(states, controls, seed):
    """Without sum terms (odd seed) the last node count that fits is 452 / 408 / 292 / 168 at 1 / 2 / 6 / 16 states, and
    the byte counts never fall as a phase grows."""
    last = {1: 452, 2: 408, 6: 292, 16: 168}[states]
    before = None
    for N in list(range(last - 9, last + 10)) + [last + 40]:
        prob, obj = make_problem(([N], [states], [controls], []), seed)
        w = codegen.lds_window(codegen.trace_problem(prob, obj))
        assert w["one_launch"] == (N <= last), N
        if before is not None:
            assert w["fused_bytes"] >= before["fused_bytes"] and w["eval_bytes"] >= before["eval_bytes"]
        before = w


def test_17_states_are_refused_by_name():
    prob, obj = make_problem(*STATES_17)
    with pytest.raises(trace.TraceError, match="more than 16 states per phase"):
        codegen.trace_problem(prob, obj)


def test_33_phases_are_refused_by_name_before_any_kernel():
    prob, obj = make_problem(*PHASES_33)
    P = codegen.trace_problem(prob, obj)
    with pytest.raises(codegen.LimitError, match=r"33 phases: more than 32 phases \(OGK_MAX_PHASE\)"):
        codegen.emit_header(P)
    # ... and by og_problem_create itself, which looks at the phase count before it looks for a device or a module
    lib = _native.lib()
    nodes = (C.c_int32 * 33)(*P.nodes)
    desc = _native.OgDesc(abi_version=_native.OG_ABI_VERSION, device=0, n=P.n, m_eq=P.m_eq, m_ineq=P.m_ineq,
                          n_phase=33, nodes=nodes, D=None, cvec=None, n_cvec=0, module_path=b"/nonexistent.so")
    handle = C.c_void_p()
    assert lib.og_problem_create(C.byref(desc), C.byref(handle)) != 0 and not handle.value
    assert b"unsupported phase count" in lib.og_last_error()
    prob, obj = problem("p32")                      # 32 phases pass
    assert len(prob.nodes) == 32 and codegen.emit_header(codegen.trace_problem(prob, obj))


def test_a_phase_beyond_the_evaluation_lds_is_refused_by_name_before_hipcc(monkeypatch):
    """16 states on 633 nodes: ``KS*(64 + 4*16) + 256 = 20 608`` doubles, more than the 160 KiB of a compute unit, for
    ogk_eval, ogk_dense and ogk_eval_batch.  The header is never generated, so nothing is compiled and nothing
    launched."""
    prob, obj = make_problem(*OVER_THE_EVALUATION_LDS)
    P = codegen.trace_problem(prob, obj)
    w = codegen.lds_window(P)
    assert not w["eval_fits"] and w["eval_bytes"] == 8 * 20608
    monkeypatch.setattr(build, "build_module", lambda *a, **k: pytest.fail("the compiler was reached"))
    with pytest.raises(codegen.LimitError, match="evaluation kernel needs 164864 bytes of LDS.*at most 632 nodes, the longest has 633"):
        codegen.emit_header(P)
    with pytest.raises(codegen.LimitError):
        twin.Twin(prob, obj, program=P)


class OgkInfo(C.Structure):
    _fields_ = [(name, C.c_int32) for name in ("abi", "n", "m", "m_eq", "m_ineq", "n_phase", "n_mv", "n_groups",
                                               "n_cvec", "n_y0")] + \
               [("phase_nodes", C.c_int32 * codegen.MAX_PHASES), ("n_eval_blocks", C.c_int32), ("fused_ok", C.c_int32)]


def test_a_module_beyond_the_window_cross_compiles_in_all_its_parts():
    """Every part of a not-fitting module builds for gfx950 (the one-launch part too: its kernel is compiled, never
    launched), and ``ogk_get_info`` - host code - gives the mirror's verdict on both sides of an edge."""
    for key in ("s16_n168", "s16_n169"):
        R = ref(key)
        module = build.build_module(R.header)
        parts = [build.part_path(module, i) for i in range(len(build.MODULE_PARTS))]
        if key in NOT_FITTING:
            parts += [build.build_batch_part(R.header), build.build_batch_exact_part(R.header)]
        for part in parts:
            assert os.path.exists(part), part
            with open(part, "rb") as fh:
                assert b"gfx950" in fh.read()
        info = OgkInfo()
        assert C.CDLL(module).ogk_get_info(C.byref(info)) == 0
        assert info.fused_ok == int(R.window["one_launch"]) == int(key == "s16_n168")
        assert (info.n, info.m, info.n_phase, info.phase_nodes[0]) == (R.program.n, R.program.m, 1, R.prob.nodes[0])


def test_the_mirror_agrees_with_ogk_get_info_of_every_compiled_module():
    """``fused_ok`` of the compiled module (host code of the module: no device needed) against the mirror, for every
    shape of this file, three BASELINE problems and ``launch4`` on 341 nodes per phase."""
    import __graft_entry__ as entry
    from opengoddard_amd import problems
    cases = [(key, problem(key)) for key in SHAPES]
    cases += [(name, problems.build(name)) for name in ("goddard", "polar_tsto", "launch4")]
    cases.append(("launch4 x 341", problems.build("launch4", nodes=entry.NEAR_THE_LIMIT_NODES)))
    for name, (prob, obj) in cases:
        P = codegen.trace_problem(prob, obj)
        module = build.build_module(codegen.emit_header(P))
        info = OgkInfo()
        assert C.CDLL(module).ogk_get_info(C.byref(info)) == 0
        w = codegen.lds_window(P)
        assert info.fused_ok == int(w["one_launch"]), name
        assert w["one_launch"] == (name in ONE_LAUNCH or name in ("goddard", "polar_tsto", "launch4")), name
    prob, obj = problems.build("launch4", nodes=entry.NEAR_THE_LIMIT_NODES)
    w = codegen.lds_window(codegen.trace_problem(prob, obj))
    assert (w["max_nmv"], w["eval_bytes"], w["fused_bytes"]) == (8, 68096, 98912) and w["eval_fits"]


# ================================================================================================ GPU
def _check_against_np_path(R, JT_cols, F0, what):
    """The device's columns against ``np_path.sweep`` on the spread: the project's FD noise bound (factor 4)."""
    x, h, cols = R.x["ok"], R.h["ok"], R.cols
    F_np, h_np, JT_np = np_path.sweep(R.prob, R.obj, x, list(cols))
    assert np.array_equal(h_np, h)
    scale = row_scales(R.program, R.prob, x, F_np)
    assert np.all(np.abs(F0 - F_np) <= 1e-9 * scale), what
    err, bound = np.abs(JT_cols - JT_np), fd_noise_bound(JT_np, scale, h[cols])
    assert np.all(err <= bound), "%s: worst ratio %.3g" % (what, np.max(err / np.maximum(bound, 1e-300)))
    assert_zero_pattern(R.program, cols, JT_cols, JT_np, what)


def _eval_sweep_and_shards(R, eng):
    x, h = R.x["ok"], R.h["ok"]
    F0c, JTc = R.sweep("ok")
    assert np.array_equal(eng.eval_stacked(x), F0c)
    F0, JT = eng.sweep_stacked(x, h)
    assert np.array_equal(F0, F0c) and np.array_equal(JT, JTc)
    for lo, hi in ((0, eng.n // 3), (eng.n // 3, eng.n - 1), (eng.n - 1, eng.n)):
        assert np.array_equal(eng.sweep_stacked(x, h, lo, hi)[1], JTc[lo:hi]), "columns [%d, %d)" % (lo, hi)
    return F0, JT


@pytest.mark.gpu
@pytest.mark.parametrize("key", ONE_LAUNCH)
def test_one_launch_shapes_give_the_twins_bits_in_every_form(key, monkeypatch):
    """The last shapes that fit, the full and partly filled A operand and 32 phases: evaluation, full sweep and three
    column shards equal the twin; OGPSX_SWEEP=split and dense give the same bits; ``np_path.sweep`` on the spread."""
    monkeypatch.delenv("OGPSX_SWEEP", raising=False)
    R = ref(key)
    eng = R.engine()
    assert eng.one_launch and eng.sweep_mode == "fused"
    F0, JT = _eval_sweep_and_shards(R, eng)
    _check_against_np_path(R, JT[R.cols], F0, key)
    R.record("test_one_launch_shapes_give_the_twins_bits_in_every_form", eng, eng.n)
    eng.close()
    for layout in ("split", "dense"):
        monkeypatch.setenv("OGPSX_SWEEP", layout)
        from opengoddard_amd.engine import HipEngine
        other = HipEngine(R.prob, R.obj, program=R.program)
        assert other.sweep_mode == layout and not other.one_launch
        Fl, JTl = other.sweep_stacked(R.x["ok"], R.h["ok"])
        assert np.array_equal(Fl, F0) and np.array_equal(JTl, JT), layout
        other.close()


@pytest.mark.gpu
@pytest.mark.parametrize("key", NOT_FITTING)
def test_a_beyond_the_window_evaluation_sweep_shards_and_exact(key, monkeypatch):
    """(a) default mode, ``one_launch == 0``: evaluation, sweep, column shards and the exact Jacobian equal the twin;
    the exact Jacobian against ``oracle/exact_jac.py`` (1e-12 of the row's largest entry, the bound of
    ``test_gpu_exact_jacobian_against_complex_step_at_baseline_sizes``) and the sweep against ``np_path.sweep``, both
    on the spread of columns."""
    from oracle import exact_jac
    monkeypatch.delenv("OGPSX_SWEEP", raising=False)
    R = ref(key)
    eng = R.engine()
    assert not eng.one_launch and eng.sweep_mode == "fused"
    F0, JT = _eval_sweep_and_shards(R, eng)
    _check_against_np_path(R, JT[R.cols], F0, key)
    Fe, JE = eng.exact_stacked(R.x["ok"])
    Fec, JEc = R.exact("ok")
    assert np.array_equal(Fe, Fec) and np.array_equal(JE, JEc)
    lo, hi = eng.n // 3, eng.n // 3 + 40
    assert np.array_equal(eng.exact_stacked(R.x["ok"], lo, hi)[1], JEc[lo:hi])
    JC = exact_jac.jacobian(R.program, R.prob, R.x["ok"], list(R.cols))
    scale = np.maximum(1.0, np.abs(JC).max(axis=0))[None, :]
    assert np.max(np.abs(JE[R.cols] - JC) / scale) <= 1e-12
    # through a non-finite point and back, host pointers
    for name in ("bad", "bad", "other"):
        Fb, JTb = eng.sweep_stacked(R.x[name], R.h[name])
        assert np.array_equal(Fb, R.sweep(name)[0], equal_nan=True) and np.array_equal(JTb, R.sweep(name)[1], equal_nan=True)
        assert eng.nonfinite_rows(0) == np.sum(~np.isfinite(R.sweep(name)[0]))
    R.record("test_a_beyond_the_window_evaluation_sweep_shards_and_exact", eng, eng.n, exact_columns=int(R.cols.size))
    eng.close()


SEQUENCE = ("ok", "bad", "bad", "ok", "other", "bad", "other")


@pytest.mark.gpu
@pytest.mark.parametrize("key", NOT_FITTING)
def test_b_beyond_the_window_registered_device_buffers(key, monkeypatch):
    """(b) ``og_fd_sweep_dev`` in its two-launch branch (evaluation with ``jt_bump``, then mode 1) into a registered
    buffer, a registered column block next to it and an unregistered buffer pre-filled with a sentinel, through
    finite -> NaN -> NaN -> finite -> other -> NaN -> other with one exact-mode call in between: all three hold the
    twin's matrix after every step."""
    import torch
    monkeypatch.delenv("OGPSX_SWEEP", raising=False)
    R = ref(key)
    eng = R.engine()
    assert not eng.one_launch
    n, m = eng.n, eng.m
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream().cuda_stream
    d_F = torch.empty(m, dtype=torch.float64, device=dev)
    lo, hi = n // 3, n // 3 + max(5, n // 2)
    reg_full = torch.full((n, m), 7.0, dtype=torch.float64, device=dev)       # garbage before registration
    reg_part = torch.full((hi - lo, m), -3.0, dtype=torch.float64, device=dev)
    eng.register_jt_dev(reg_full.data_ptr(), 0, n, stream)
    eng.register_jt_dev(reg_part.data_ptr(), lo, hi, stream)
    plain = torch.empty((n, m), dtype=torch.float64, device=dev)

    def sweep(name, into, c0, c1):
        d_x, d_h = torch.from_numpy(R.x[name]).to(dev), torch.from_numpy(R.h[name]).to(dev)
        eng.sweep_dev(d_x.data_ptr(), d_h.data_ptr(), c0, c1, into.data_ptr(), d_F.data_ptr(), stream)
        torch.cuda.synchronize()
        return into.cpu().numpy()

    for step, name in enumerate(SEQUENCE):
        F_want, want = R.sweep(name)
        plain.fill_(float(step) + 0.5)
        assert np.array_equal(sweep(name, plain, 0, n), want, equal_nan=True), "unregistered buffer at step %d" % step
        assert np.array_equal(d_F.cpu().numpy(), F_want, equal_nan=True)
        assert np.array_equal(sweep(name, reg_full, 0, n), want, equal_nan=True), "registered buffer at step %d" % step
        assert eng.nonfinite_rows(stream) == np.sum(~np.isfinite(F_want)), "count at step %d" % step
        assert np.array_equal(sweep(name, reg_part, lo, hi), want[lo:hi], equal_nan=True), "registered block at step %d" % step
        assert np.isnan(want).any() == (name == "bad")
        if step == 2:            # exact mode into the buffer a NaN fill was left in: cleans it too
            d_x = torch.from_numpy(R.x["ok"]).to(dev)
            eng.exact_dev(d_x.data_ptr(), 0, n, reg_full.data_ptr(), d_F.data_ptr(), stream)
            torch.cuda.synchronize()
            assert np.array_equal(reg_full.cpu().numpy(), R.exact("ok")[1])
    R.record("test_b_beyond_the_window_registered_device_buffers", eng, n)
    eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize("key", NOT_FITTING)
def test_c_beyond_the_window_registered_host_matrix(key, monkeypatch):
    """(c) ``og_jt_register_host`` beyond the window: neither the mapped nor the packed route exists there, the
    persistent matrix receives a full download - the twin's matrix through the same sequence of points, FD and exact."""
    monkeypatch.delenv("OGPSX_SWEEP", raising=False)
    monkeypatch.delenv("OGPSX_HOST", raising=False)
    R = ref(key)
    eng = R.engine()
    assert not eng.one_launch and eng.host_path is None
    paths = []
    for step, name in enumerate(SEQUENCE):
        F_want, JT_want = R.sweep(name)
        F_got, JT_got = eng.sweep_persistent(R.x[name], R.h[name])
        assert JT_got is eng._JT_host
        assert np.array_equal(F_got, F_want, equal_nan=True), "F at step %d" % step
        assert np.array_equal(JT_got, JT_want, equal_nan=True), "J_T at step %d" % step
        paths.append(eng.host_path)
        if step == 2:
            Fp, JTp = eng.sweep_persistent(R.x["ok"], R.h["ok"], exact=True)
            assert np.array_equal(JTp, R.exact("ok")[1]) and np.array_equal(Fp, R.exact("ok")[0])
    assert paths == ["download"] * len(SEQUENCE)            # (it used to say "undecided" for ever)
    (g, Jeq, Jineq), _ = eng.jacobians(R.x["other"], R.lb, R.ub)
    assert np.array_equal(np.vstack([g[None, :], Jeq, Jineq]), R.sweep("other")[1].T)
    R.record("test_c_beyond_the_window_registered_host_matrix", eng, eng.n, host_path=paths[-1])
    eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize("key", NOT_FITTING)
def test_d_beyond_the_window_batches(key, monkeypatch):
    """(d) the batch fallback (one batched evaluation, then the handle's sweep and pack lane by lane), capacity 3:
    host and device-pointer sweeps with and without packed values at counts 1 and 3 with the NaN point in the middle
    lane, the lanes' dense matrices and non-finite counts, the exact batch and ``Problem.evaluate_batch``.  Every lane
    holds the twin's result at its point, whatever its companions are."""
    import torch
    monkeypatch.delenv("OGPSX_SWEEP", raising=False)
    R = ref(key)
    eng = R.engine()
    assert not eng.one_launch
    n, m = eng.n, eng.m
    batch = eng.batch(3)
    nnz = batch.nnz
    packed = {name: gather(R.program, R.sweep(name)[1]) for name in ("ok", "other")}
    bad_rows = int(np.sum(~np.isfinite(R.sweep("bad")[0])))

    def check_lanes(names, F0, vals, nonfinite, what):
        for k, name in enumerate(names):
            F_want, JT_want = R.sweep(name)
            assert np.array_equal(F0[k], F_want, equal_nan=True), "%s: F of lane %d" % (what, k)
            assert np.array_equal(batch.dense(k), JT_want, equal_nan=True), "%s: matrix of lane %d" % (what, k)
            want_bad = bad_rows if name == "bad" else 0
            assert batch.lane_dev(k)[1] == want_bad, "%s: count of lane %d" % (what, k)
            if nonfinite is not None:
                assert nonfinite[k] == want_bad
            if vals is not None and name != "bad":
                assert np.array_equal(vals[k], packed[name]), "%s: packed values of lane %d" % (what, k)

    for names in (("ok", "bad", "other"), ("other",), ("bad", "ok", "ok"), ("ok",), ("other", "other", "ok")):
        X, H = np.stack([R.x[k] for k in names]), np.stack([R.h[k] for k in names])
        F0, vals, nonfinite = batch.sweep(X, H)
        check_lanes(names, F0, vals, nonfinite, "sweep %s" % (names,))
        assert np.array_equal(batch.values(X), np.stack([R.sweep(k)[0] for k in names]), equal_nan=True)
    # device pointers, with and without packed values
    dev = torch.device("cuda", eng.device)
    stream = torch.cuda.current_stream().cuda_stream
    for names, with_vals in ((("other", "bad", "ok"), True), (("ok",), False), (("ok", "bad", "other"), False), (("other",), True)):
        d_X = torch.from_numpy(np.stack([R.x[k] for k in names])).to(dev)
        d_H = torch.from_numpy(np.stack([R.h[k] for k in names])).to(dev)
        d_F = torch.full((len(names), m), -1.0, dtype=torch.float64, device=dev)
        d_V = torch.full((len(names), nnz), -1.0, dtype=torch.float64, device=dev) if with_vals else None
        batch.sweep_dev(len(names), d_X.data_ptr(), d_H.data_ptr(), d_F.data_ptr(),
                        d_V.data_ptr() if with_vals else None, stream)
        torch.cuda.synchronize()
        check_lanes(names, d_F.cpu().numpy(), d_V.cpu().numpy() if with_vals else None, None, "sweep_dev %s" % (names,))
    # exact
    names = ("ok", "other", "ok")
    X = np.stack([R.x[k] for k in names])
    Fe, ve, nfe = batch.exact(X)
    for k, name in enumerate(names):
        assert np.array_equal(Fe[k], R.exact(name)[0]) and np.array_equal(ve[k], gather(R.program, R.exact(name)[1]))
    assert not nfe.any()
    # Problem.evaluate_batch on this engine
    R.prob._engine = eng
    for jacobian in (False, True, "exact"):
        res = R.prob.evaluate_batch(R.obj, X, jacobian=jacobian)
        for k, name in enumerate(names):
            F_want = R.sweep(name)[0]
            assert res.cost[k] == F_want[0] and np.array_equal(res.equality[k], F_want[1:1 + eng.m_eq])
            assert np.array_equal(res.inequality[k], F_want[1 + eng.m_eq:])
            if jacobian is True:
                assert np.array_equal(res.values[k], packed[name]) and np.array_equal(res.steps[k], R.h[name])
            if jacobian == "exact":
                assert np.array_equal(res.values[k], gather(R.program, R.exact(name)[1]))
    R.prob._engine = None
    R.record("test_d_beyond_the_window_batches", eng, n)
    eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize("key", NOT_FITTING)
def test_e_beyond_the_window_shards(key, monkeypatch):
    """(e) ``og_shard_sweep_dev`` as sweep + pack, ``og_shard_unpack_dev``, ``og_pattern`` / pack / unpack and
    ``HipEngine(devices=[0, 0])``: W = 2 and 3 ranks on the one device, every rank's reassembled replica equals the
    twin's full matrix through a finite step, a NaN step and the clean-up step after it."""
    import torch
    from opengoddard_amd import sharding
    from opengoddard_amd.engine import HipEngine
    monkeypatch.delenv("OGPSX_SWEEP", raising=False)
    monkeypatch.setenv("OGPSX_GATHER", "peer")
    R = ref(key)
    eng = R.engine()
    assert not eng.one_launch
    n, m = eng.n, eng.m
    indptr, rows = eng.pattern()
    want_ptr, want_rows = codegen.sparsity(R.program)
    assert np.array_equal(indptr, want_ptr) and np.array_equal(rows, want_rows)
    dev = torch.device("cuda", 0)
    be = sharding.HipBackend(eng, dev)
    for world in (2, 3):
        ranks = [sharding.ShardedSweep(be, n, m, rank, world) for rank in range(world)]
        for step, name in enumerate(("ok", "bad", "other")):
            F_want, JT_want = R.sweep(name)
            d_x, d_h = be.upload(R.x[name]), be.upload(R.h[name])
            for sh in ranks:
                be.sweep_and_pack(sh.rank, d_x, d_h, sh.lo, sh.hi, sh.replica, sh.F0, sh.send)
            torch.cuda.synchronize()
            message = torch.cat([sh.send[:max(sh.block_vals, 1)] for sh in ranks])
            if name != "bad":
                for sh in ranks:                    # the rank's message: its packed non-zeros in pattern order
                    mine = JT_want[np.repeat(np.arange(sh.lo, sh.hi), np.diff(indptr[sh.lo:sh.hi + 1])),
                                   rows[indptr[sh.lo]:indptr[sh.hi]]]
                    assert np.array_equal(sh.send.cpu().numpy()[:mine.size], mine), "message of rank %d" % sh.rank
            for sh in ranks:
                sh.recv.copy_(message)
                be.unpack(sh.rank, sh.recv, sh.replica)
            torch.cuda.synchronize()
            for sh in ranks:
                assert np.array_equal(sh.F0.cpu().numpy(), F_want, equal_nan=True)
                assert np.array_equal(sh.replica.cpu().numpy(), JT_want, equal_nan=True), \
                    "world %d, rank %d, step %d" % (world, sh.rank, step)
        for sh in ranks:
            eng.unregister_jt_dev(sh.replica[sh.lo:sh.hi].data_ptr())
        del ranks
    # og_pack_dev / og_unpack_dev on a column range
    lib = _native.lib()
    stream = torch.cuda.current_stream().cuda_stream
    JT = R.sweep("other")[1]
    lo, hi = n // 5, n // 5 + n // 2
    ip, rw = eng.pattern(lo, hi)
    d_JT = torch.from_numpy(JT[lo:hi].copy()).to(dev)
    d_vals = torch.empty(int(ip[-1]), dtype=torch.float64, device=dev)
    _native.check(lib.og_pack_dev(eng._handle, d_JT.data_ptr(), lo, hi, d_vals.data_ptr(), stream), "og_pack_dev")
    d_out = torch.full((hi - lo, m), 5.0, dtype=torch.float64, device=dev)
    _native.check(lib.og_unpack_dev(eng._handle, d_vals.data_ptr(), lo, hi, d_out.data_ptr(), stream), "og_unpack_dev")
    torch.cuda.synchronize()
    dense = np.zeros((hi - lo, m), dtype=bool)
    dense[np.repeat(np.arange(hi - lo), np.diff(ip)), rw] = True
    out = d_out.cpu().numpy()
    # (packed values come in pattern order - a column's own collocation block first - not sorted by row)
    assert np.array_equal(d_vals.cpu().numpy(), JT[lo:hi][np.repeat(np.arange(hi - lo), np.diff(ip)), rw])
    assert np.array_equal(out[dense], JT[lo:hi][dense]) and np.all(out[~dense] == 5.0)
    eng.close()
    # the multi-device handle, two sub-handles on device 0
    many = HipEngine(R.prob, R.obj, program=R.program, devices=[0, 0])
    assert not many.one_launch
    for name in ("ok", "bad", "other"):
        F_got, JT_got = many.sweep_persistent(R.x[name], R.h[name])
        assert np.array_equal(F_got, R.sweep(name)[0], equal_nan=True)
        assert np.array_equal(JT_got, R.sweep(name)[1], equal_nan=True), "devices=[0, 0] at %s" % name
    R.record("test_e_beyond_the_window_shards", many, n)
    many.close()
    _native.lib().og_comm_finalize()


@pytest.mark.gpu
@pytest.mark.parametrize("key", NOT_FITTING)
def test_f_beyond_the_window_captured_graph(key, monkeypatch):
    """(f) a captured graph of ``og_fd_sweep_dev`` in its two-launch form, replayed at new points.  Outside a capture the
    host alternates between two counters of non-finite rows and each evaluation clears the other one; a replayed graph
    uses ONE counter, so the capturing call clears it as a node of the graph (``clear_count_in_a_capture``,
    csrc/ogpsx_core.hip) - without that the count only grows after a non-finite point and every later replay fills
    with z and marks the buffer (J_T stays right: z is zero where F is finite; ``og_nonfinite_rows`` shows it).
    Asserted: the twin's F and J_T at every replay and the right count, also with eager calls between the replays."""
    import torch
    monkeypatch.delenv("OGPSX_SWEEP", raising=False)
    R = ref(key)
    eng = R.engine()
    assert not eng.one_launch
    n, m = eng.n, eng.m
    dev = torch.device("cuda", 0)
    d_x = torch.zeros(n, dtype=torch.float64, device=dev)
    d_h = torch.zeros(n, dtype=torch.float64, device=dev)
    d_F = torch.empty(m, dtype=torch.float64, device=dev)
    d_JT = torch.empty((n, m), dtype=torch.float64, device=dev)

    def load(name):
        d_x.copy_(torch.from_numpy(R.x[name]))
        d_h.copy_(torch.from_numpy(R.h[name]))

    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        eng.register_jt_dev(d_JT.data_ptr(), 0, n, side.cuda_stream)
        load("ok")
        eng.sweep_dev(d_x.data_ptr(), d_h.data_ptr(), 0, n, d_JT.data_ptr(), d_F.data_ptr(), side.cuda_stream)   # warm
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        eng.sweep_dev(d_x.data_ptr(), d_h.data_ptr(), 0, n, d_JT.data_ptr(), d_F.data_ptr(),
                      torch.cuda.current_stream().cuda_stream)
    for step, name in enumerate(("other", "bad", "bad", "ok", "other", "bad", "ok")):
        load(name)
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        F_want, JT_want = R.sweep(name)
        assert np.array_equal(d_F.cpu().numpy(), F_want, equal_nan=True), "F at replay %d" % step
        assert np.array_equal(d_JT.cpu().numpy(), JT_want, equal_nan=True), "J_T at replay %d" % step
        assert eng.nonfinite_rows(0) == np.sum(~np.isfinite(F_want)), "count of non-finite rows at replay %d" % step
    # an eager call between replays takes the other counter; the replay after it is still right
    for name in ("bad", "ok"):
        assert np.array_equal(eng.sweep_stacked(R.x[name], R.h[name])[1], R.sweep(name)[1], equal_nan=True)
        load("other")
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        assert np.array_equal(d_JT.cpu().numpy(), R.sweep("other")[1]) and np.array_equal(d_F.cpu().numpy(), R.sweep("other")[0])
    R.record("test_f_beyond_the_window_captured_graph", eng, n)
    eng.close()


@pytest.mark.gpu
def test_the_evaluation_lds_edge_is_refused_on_the_device_too():
    """16 states on 633 nodes: ``HipEngine`` raises before it compiles or launches anything.  16 states on 632 nodes use
    the whole LDS of a compute unit: the evaluation equals the twin."""
    from opengoddard_amd.engine import HipEngine
    prob, obj = make_problem(*OVER_THE_EVALUATION_LDS)
    jit_before = set(os.listdir(build.JITDIR))
    with pytest.raises(codegen.LimitError, match="evaluation kernel needs 164864 bytes of LDS"):
        HipEngine(prob, obj)
    assert set(os.listdir(build.JITDIR)) == jit_before
    prob, obj = make_problem(*PHASES_33)
    with pytest.raises(codegen.LimitError, match="more than 32 phases"):
        HipEngine(prob, obj)
    R = ref("s16_n632")
    eng = R.engine()
    assert not eng.one_launch
    for name in ("ok", "bad", "other"):
        F = R.tw.values(R.x[name])
        assert np.array_equal(eng.eval_stacked(R.x[name]), F, equal_nan=True)
        assert eng.nonfinite_rows(0) == np.sum(~np.isfinite(F))
    R.record("test_the_evaluation_lds_edge_is_refused_on_the_device_too", eng, 0)
    eng.close()


@pytest.mark.gpu
def test_launch4_near_the_variable_limit_sweeps_in_two_launches_with_the_twins_bits(monkeypatch):
    """``launch4`` on 341 nodes per phase (n = 16 372), the shape tests/test_gpu_solve.py solves on the HIP SQP core:
    8 states give 16*344 + 8*685 = 10 984 doubles plus 1 380 of sum terms, beyond the window, and its evaluation kernel
    asks for 68 096 bytes of dynamic LDS.  ``one_launch == 0``; the sweep equals the twin on about 200 columns spread over
    every block plus every phase-time column."""
    import __graft_entry__ as entry
    from opengoddard_amd import problems
    from opengoddard_amd.engine import HipEngine
    monkeypatch.delenv("OGPSX_SWEEP", raising=False)
    t0 = time.time()
    prob, obj = problems.build("launch4", nodes=entry.NEAR_THE_LIMIT_NODES)
    eng = HipEngine(prob, obj)
    w = codegen.lds_window(eng.program)
    assert not w["one_launch"] and w["eval_bytes"] == 68096 and w["eval_fits"]
    assert not eng.one_launch and eng.sweep_mode == "fused"
    tw = twin.Twin(prob, obj, program=eng.program, header=eng.header)
    lb, ub = np_path.bounds_arrays(prob)
    x = np.clip(prob.p, lb, ub)
    h = _native.fd_step(x, lb, ub)
    cols = spread_columns(prob, inside=2)
    assert 150 <= cols.size <= 260
    F0c, JTc = tw.sweep(x, h, cols)
    assert np.array_equal(eng.eval_stacked(x), F0c)
    runs = np.split(cols, np.nonzero(np.diff(cols) != 1)[0] + 1)
    for run in runs:                                  # (the full matrix would be 16 372 x 14 000 doubles)
        lo, hi = int(run[0]), int(run[-1]) + 1
        F0, JT = eng.sweep_stacked(x, h, lo, hi)
        at = np.searchsorted(cols, run)
        assert np.array_equal(F0, F0c) and np.array_equal(JT, JTc[at]), "columns [%d, %d)" % (lo, hi)
    indptr, _ = codegen.sparsity(eng.program)
    record_measurement("test_launch4_near_the_variable_limit_sweeps_in_two_launches_with_the_twins_bits",
                       shape="launch4 x 341", one_launch=int(eng.one_launch), eval_bytes=w["eval_bytes"],
                       fused_bytes=w["fused_bytes"], fill_bytes=w["fill_bytes"], n=eng.n, m=eng.m, nnz=int(indptr[-1]),
                       columns=int(cols.size), seconds=time.time() - t0)
    eng.close()
