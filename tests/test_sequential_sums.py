"""Sequential sums (a running cost summed node by node like Python's ``sum()``: ``optimize._assemble_cost`` ->
``trace.seqsum``) on the path only the device takes.

The kernels keep the base terms of every sum in LDS (``fill_terms``, csrc/ogk_kernels.hip) and hand the generated code
an accessor (``XColT``) with ``term_cache / term_q / term_v``; the generated loop (``codegen._cached_sum_lines``) then
adds cached terms, two register buffers of four in turn, one group read ahead, with the one term that reads the lane's
perturbed variable swapped in.  The CPU twin, the interpreter and the exact path have no such accessor and sum in
place, so no other CPU test runs that loop.  This module pins it:

================  ==================================================================================================
host probe        tests/sum_cache_probe.cpp: the accessor on the host against a materialised vector, bit for bit, under
                  AddressSanitizer / UBSan, the cache exactly ``N_TERMS + 16`` doubles with a NaN pad; its counts of
                  cached / in-place / untouched (block, column) pairs against tables derived from each problem
remainders        phase lengths 3..8, 9..15 and 16, 17, 23, 24, 25: every ``ln % 8``, blocks shorter than one group, a
                  loop of 0, 1, 2 and 3 trips; ``np.roll`` by 1 and by 2 for blocks of one and of two terms
relations         how a term can depend on a variable: reversed (17 one-term blocks), rolled, two variables per term, a
                  scalar in every term, a constant, ``mean``, strided pieces, one scalar repeated, a Python ``sum`` in a row
2048 | 2049       the largest cache and the first module without one, both in one launch
64 blocks         twice the term blocks 32 phases can give (``qd[N_TBLK]`` / ``td[N_TBLK]`` per lane)
non-finite        one NaN term: the cost row of EVERY column is NaN, and the next sweep cleans up
================  ==================================================================================================
"""
import math
import os
import re
import subprocess
import time

import numpy as np
import pytest

from conftest import assert_zero_pattern, fd_noise_bound, record_measurement
from opengoddard_amd import _native, build, codegen
from opengoddard_amd.optimize import Condition, Dynamics, Problem
from oracle import np_path, program_eval, twin
from test_module_limits import OgkInfo, row_scales, spread_columns
from test_random_layouts import make_problem

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "opengoddard_amd", "csrc")
PROBE_SOURCE = os.path.join(ROOT, "tests", "sum_cache_probe.cpp")
PROBE_FLAGS = ["-O1", "-std=c++17", "-ffp-contract=off", "-mfma", "-fsanitize=address,undefined", "-I", CSRC]


class Obj:
    pass


def U(prob):
    return prob.controls_all_section(0)


def V(prob):
    return prob.states_all_section(1)


def skeleton(nodes, states, running, seed, python_sum_row=False):
    """The callbacks of ``test_edge_problems.running_cost_shapes`` on any phase lengths, with one or two states and one
    control per phase, smooth knots, the final time as Mayer cost and ``running`` as the running cost."""
    S = len(nodes)

    def dynamics(prob, obj, section):
        dx = Dynamics(prob, section)
        if states == 2:
            dx[0] = prob.states(1, section)
            dx[1] = prob.controls(0, section) - 0.3 * prob.states(0, section)
        else:
            dx[0] = prob.controls(0, section) - 0.3 * prob.states(0, section)
        return dx()

    def equality(prob, obj):
        rows = Condition()
        rows.equal(prob.states(0, 0)[0], 0.1)
        if states == 2:
            rows.equal(prob.states(1, 0)[0], 0.0)
        if python_sum_row:
            u = U(prob)
            rows.equal(sum(u[0:13] ** 2), 3.0)              # Python's sum of traced scalars: a chain of additions
        return rows()

    def inequality(prob, obj):
        rows = Condition()
        rows.upper_bound(U(prob), 2.0)
        for i in range(S):
            rows.lower_bound(prob.time_final(i), 0.2 + i)
        return rows()

    prob = Problem([float(t) for t in range(S + 1)], list(nodes), [states] * S, [1] * S, 3)
    rng = np.random.default_rng(seed)
    prob.p[:-S] = rng.uniform(-1.0, 1.0, prob.number_of_variables - S)
    prob.dynamics = [dynamics] * S
    prob.knot_states_smooth = [True] * (S - 1)
    prob.cost = lambda prob, obj: prob.time_final(-1)
    prob.running_cost = running
    prob.equality = equality
    prob.inequality = inequality
    return prob, Obj()


def half_square(prob, obj):
    return 0.5 * prob.states_all_section(0) ** 2


def half_square_and_a_root(prob, obj):
    x = prob.states_all_section(0)
    return 0.5 * x ** 2 + 0.0 * np.sqrt(x + 2.0)              # NaN where a state is below -2


# name -> (phase lengths, states per phase, running cost, python_sum_row)
BUILDERS = {
    # 1a: remainders
    "rem_3_8": ([3, 4, 5, 6, 7, 8], 1, half_square, False),
    "rem_9_15": ([9, 10, 11, 12, 13, 14, 15], 1, half_square, False),
    "rem_16_25": ([16, 17, 23, 24, 25], 1, half_square, False),
    "roll1": ([11, 6], 2, lambda p, o: U(p) * np.roll(U(p), 1), False),          # blocks of 1, 10, 1, 5 terms
    "roll2": ([11, 6], 2, lambda p, o: U(p) * np.roll(U(p), 2), False),          # blocks of 2, 9, 2, 4 terms
    # 1b: relations between a term and a variable
    "reversed": ([11, 6], 2, lambda p, o: U(p) * U(p)[::-1], False),
    "two_variables": ([13], 2, lambda p, o: V(p) * np.roll(U(p), -3), False),
    "final_time": ([11, 6], 2, lambda p, o: np.where(U(p) > 0, U(p) ** 2, -0.5 * U(p)) * p.time_final(0), False),
    "constant": ([11, 6], 2, lambda p, o: 0.0 * U(p) + 1.0, False),
    "one_scalar": ([11, 6], 2, lambda p, o: U(p) * V(p)[0], False),
    "mean": ([11, 6], 2, lambda p, o: U(p) * U(p).mean(), False),
    "strided": ([12], 2, lambda p, o: np.concatenate((U(p)[::2], V(p)[1::2])) ** 2, False),
    "repeated": ([12], 2, lambda p, o: np.ones(12) * U(p)[3] ** 2, False),
    "python_sum_row": ([11, 6], 2, lambda p, o: 0.5 * U(p) ** 2, True),
    # 1d: many blocks
    "blocks64": ([64], 2, lambda p, o: U(p) * U(p)[::-1], False),
    # 1e: a non-finite term
    "nonfinite": ([9, 10, 11, 12, 13, 14, 15], 1, half_square_and_a_root, False),
}
REMAINDERS = ["rem_3_8", "rem_9_15", "rem_16_25", "roll1", "roll2"]
RELATIONS = ["reversed", "two_variables", "final_time", "constant", "one_scalar", "mean", "strided", "repeated", "python_sum_row"]
SWEPT = REMAINDERS + RELATIONS + ["blocks64"]             # 1a, 1b, 1d
PROBED = SWEPT + ["nonfinite"]
BAD_PHASE, BAD_NODE = 3, 5                               # 1e: this state is put below -2


def term_blocks(name, prob):
    """What the construction of problem ``name`` implies: its term blocks as ``(terms, leaves)``, a leaf ``(first
    variable, stride)`` being one operand of the block's term q, ``x[first + stride*q]``.  Pieces of consecutive
    variables are stride-1 leaves; a scalar (an element picked out of a vector, a reduction's operand, a final time,
    and each element of a reversed or strided view, which the tracer lowers one by one) is a stride-0 leaf."""
    nodes = prob.nodes
    u = [prob.index_controls(0, i, 0) for i in range(len(nodes))]
    s0 = [prob.index_states(0, i, 0) for i in range(len(nodes))]
    s1 = [prob.index_states(1, i, 0) for i in range(len(nodes))] if prob.number_of_states[0] > 1 else None
    all_u = [u[i] + k for i in range(len(nodes)) for k in range(nodes[i])]
    t0 = prob.number_of_variables - len(nodes)
    if name.startswith("rem_") or name == "nonfinite":
        return [(N, [(s0[i], 1)]) for i, N in enumerate(nodes)]
    if name in ("roll1", "roll2"):
        r, (a, b) = int(name[-1]), nodes
        return [(r, [(u[0], 1), (u[1] + b - r, 1)]), (a - r, [(u[0] + r, 1), (u[0], 1)]),
                (r, [(u[1], 1), (u[0] + a - r, 1)]), (b - r, [(u[1] + r, 1), (u[1], 1)])]
    if name in ("reversed", "blocks64"):
        return [(1, [(all_u[i], 1), (all_u[-1 - i], 0)]) for i in range(len(all_u))]
    if name == "two_variables":                     # roll(u, -3)[i] = u[(i + 3) % 13]
        return [(10, [(s1[0], 1), (u[0] + 3, 1)]), (3, [(s1[0] + 10, 1), (u[0], 1)])]
    if name == "final_time":
        return [(N, [(u[i], 1), (t0, 0)]) for i, N in enumerate(nodes)]
    if name in ("constant", "python_sum_row"):
        return [(N, [(u[i], 1)]) for i, N in enumerate(nodes)]
    if name == "one_scalar":
        return [(N, [(u[i], 1), (s1[0], 0)]) for i, N in enumerate(nodes)]
    if name == "mean":
        return [(N, [(u[i], 1)] + [(j, 0) for j in all_u]) for i, N in enumerate(nodes)]
    if name == "strided":
        return [(1, [(u[0] + 2 * k, 0)]) for k in range(6)] + [(1, [(s1[0] + 2 * k + 1, 0)]) for k in range(6)]
    if name == "repeated":
        return [(12, [(u[0] + 3, 0)])]
    raise KeyError(name)


def expected_pairs(n, blocks):
    """(cached, in place, neither) over all (block, column) pairs by the rule ``sum_term_q`` documents: the index of the
    ONE term of the block that reads p[j] through consecutive pieces; in place (-2) when a scalar operand is p[j] -
    every term reads it - or when two different terms read it; neither when no term does."""
    cached = in_place = 0
    for ln, leaves in blocks:
        for j in range(n):
            scalar = any(stride == 0 and base == j for base, stride in leaves)
            qs = {j - base for base, stride in leaves if stride == 1 and base <= j < base + ln}
            if scalar or len(qs) > 1:
                in_place += 1
            elif qs:
                cached += 1
    return cached, in_place, len(blocks) * n - cached - in_place


# name -> (cached, in place): the tables worked out by hand, which ``expected_pairs`` must reproduce.
#   rem_* / nonfinite: every state column is read by exactly one term of its phase's block.
#   roll1 on [11, 6]: the two one-term blocks read two variables each (4); in a block u[q+1]*u[q] the first and the
#     last control of the phase are read by one term (2 per block), the 9 and 4 between them by two.
#   roll2: the two-term blocks read 4 variables each (8); in a block u[q+2]*u[q] the outer two at each end are read
#     once (4 per block), the 7 and 2 between them twice.
#   reversed: block i reads u[i] as a piece (cached) and u[L-1-i] as a scalar (in place); the middle block of an odd
#     L reads the same variable both ways: in place.  L = 17: 16 + 17; L = 64: 64 + 64.
#   two_variables: 13 states and 13 controls, each read by one term.
#   final_time / one_scalar: 17 controls cached, the scalar in place in both blocks.
#   constant / python_sum_row: 17 controls cached.
#   mean: every control is a scalar operand of both blocks: 2 * 17 in place.
#   strided: 12 one-term blocks of one scalar each.    repeated: one block, one scalar.
PAIRS = {"rem_3_8": (33, 0), "rem_9_15": (84, 0), "rem_16_25": (105, 0), "nonfinite": (84, 0), "roll1": (8, 13),
         "roll2": (16, 9), "reversed": (16, 17), "blocks64": (64, 64), "two_variables": (26, 0), "final_time": (17, 2),
         "one_scalar": (17, 2), "constant": (17, 0), "python_sum_row": (17, 0), "mean": (0, 34), "strided": (0, 12),
         "repeated": (0, 1)}


class Ref:
    """One problem with its traced program, header, points, twin and reference sweeps, each made once and never changed."""

    def __init__(self, name, made=None):
        self.name = name
        if made is None:
            nodes, states, running, python_sum_row = BUILDERS[name]
            made = skeleton(nodes, states, running, seed=40 + len(name), python_sum_row=python_sum_row)
        self.prob, self.obj = made
        self.program = codegen.trace_problem(self.prob, self.obj)
        self.header = codegen.emit_header(self.program)
        self.window = codegen.lds_window(self.program)
        self.lb, self.ub = np_path.bounds_arrays(self.prob)
        x0 = np.clip(self.prob.p, self.lb, self.ub)
        rng = np.random.default_rng(5)
        x1 = np.clip(x0 + 1e-3 * rng.standard_normal(x0.size), self.lb, self.ub)
        self.x = {"guess": x0, "near": x1}
        self.h = {k: _native.fd_step(v, self.lb, self.ub) for k, v in self.x.items()}
        self._twin = None
        self._sweeps, self._exact, self._np = {}, {}, {}

    def add_point(self, key, x):
        self.x[key] = x
        self.h[key] = _native.fd_step(x, self.lb, self.ub)

    @property
    def tw(self):
        if self._twin is None:
            self._twin = twin.Twin(self.prob, self.obj, program=self.program, header=self.header)
        return self._twin

    def sweep(self, key):
        if key not in self._sweeps:
            self._sweeps[key] = self.tw.sweep(self.x[key], self.h[key])
        return self._sweeps[key]

    def exact(self, key):
        if key not in self._exact:
            self._exact[key] = self.tw.exact(self.x[key])
        return self._exact[key]

    def np_sweep(self, key, cols=None):
        """``np_path.sweep``: the path that shares no generated code (all columns unless ``cols``)."""
        if key not in self._np:
            self._np[key] = np_path.sweep(self.prob, self.obj, self.x[key], None if cols is None else list(cols))
        return self._np[key]

    def terms(self, key):
        """(Mayer cost, the running cost's terms) at a point, from NumPy."""
        saved = self.prob.p
        try:
            self.prob.p = self.x[key].copy()
            mayer = float(self.prob.cost(self.prob, self.obj))
            t = np.asarray(self.prob.running_cost(self.prob, self.obj) * np.concatenate(self.prob.w), dtype=float)
        finally:
            self.prob.p = saved
        return mayer, t

    def scales(self, key, F):
        """Row scales of the FD noise bound: ``test_module_limits.row_scales``, the cost row by the terms it sums."""
        scale = row_scales(self.program, self.prob, self.x[key], F)
        mayer, t = self.terms(key)
        scale[0] = max(1.0, abs(mayer) + float(np.sum(np.abs(t))))
        return scale

    def engine(self):
        from opengoddard_amd.engine import HipEngine
        eng = HipEngine(self.prob, self.obj, program=self.program)
        assert eng.one_launch == self.window["one_launch"], "the mirror and ogk_get_info disagree on %s" % self.name
        return eng


_REFS = {}


def ref(name):
    if name not in _REFS:
        R = _REFS[name] = Ref(name)
        if name == "nonfinite":
            bad = R.x["guess"].copy()
            bad[R.prob.index_states(0, BAD_PHASE, BAD_NODE)] = -2.5
            R.add_point("bad", bad)
    return _REFS[name]


def header_table(header, name):
    body = re.search(r" %s\[\d+\] = \{\n(.*?)\n\};" % name, header, re.S).group(1)
    return [[int(v) for v in re.findall(r"-?\d+", row)] for row in body.split("\n")]


def term_flags(header):
    """Which kinds of workgroup of this module fill the term cache, from the header's work lists: light groups
    (``OGT_LGRP[].v[7] >> 16``), heavy parts (``OGT_HPART[].v[7] >> 30``), evaluation row waves (``OGT_ROWWAVE[].w``)."""
    return {"light": sum(1 for r in header_table(header, "OGT_LGRP") if r[7] >> 16),
            "heavy": sum(1 for r in header_table(header, "OGT_HPART") if (r[7] >> 30) & 1),
            "rowwave": sum(1 for r in header_table(header, "OGT_ROWWAVE") if r[3])}


def assert_the_suite_has_every_kind_of_workgroup():
    """A light group, a heavy part and an evaluation row wave with the term flag.  ``rem_3_8`` supplies the light groups
    (its state columns read the cost row and nothing heavy exists in it) and the row wave (the cost row's group);
    ``final_time`` supplies the heavy part: the final time of its 11-node phase has 22 + 12 defect items, the cost row
    and its bound - 36 items, above the 32 of a light column - so the phase lengths [11, 6] of the issue needed no
    lengthening.  ``rem_16_25`` has one too (its last phase spans two node tiles)."""
    flags = {name: term_flags(ref(name).header) for name in ("rem_3_8", "final_time", "rem_16_25")}
    assert flags["rem_3_8"]["light"] > 0 and flags["rem_3_8"]["rowwave"] > 0 and flags["rem_3_8"]["heavy"] == 0
    assert flags["final_time"]["heavy"] > 0 and flags["final_time"]["light"] > 0 and flags["final_time"]["rowwave"] > 0
    assert flags["rem_16_25"]["heavy"] > 0
    for name in SWEPT:
        assert ref(name).window["term_doubles"] == ref(name).window["n_terms"] + 16 and ref(name).window["one_launch"]


# ================================================================================================ CPU
def test_the_tables_of_pairs_follow_from_the_construction():
    for name in PROBED:
        R = ref(name)
        blocks = term_blocks(name, R.prob)
        cached, in_place, neither = expected_pairs(R.program.n, blocks)
        assert (cached, in_place) == PAIRS[name], name
        got =re.search(r"TERM_LEN\(const int i\) \{ constexpr int t\[\d+\] = \{([^}]*)\}", R.header).group(1)
        assert [int(v) for v in got.split(",")] == [ln for ln, _ in blocks], name
        assert R.window["n_terms"] == sum(ln for ln, _ in blocks)
    # the Python sum of a row is a chain of additions in that row's code, not a term block
    assert ref("python_sum_row").window["n_terms"] == 17
    assert {ln % 8 for name in REMAINDERS for ln, _ in term_blocks(name, ref(name).prob)} == set(range(8))
    assert {ln // 8 for name in REMAINDERS for ln, _ in term_blocks(name, ref(name).prob)} == {0, 1, 2, 3}
    assert {1, 2} <= {ln for name in REMAINDERS for ln, _ in term_blocks(name, ref(name).prob)}


def test_the_work_lists_have_every_kind_of_workgroup_with_terms():
    assert_the_suite_has_every_kind_of_workgroup()


@pytest.fixture(scope="module")
def probe_dir(tmp_path_factory):
    return str(tmp_path_factory.mktemp("sum_cache_probe"))


def build_probe(R, folder):
    """The probe against this problem's header: its own program, the sanitizers' runtimes linked into it (statically
    where the toolchain has them, so that it starts the same whatever else a machine loads into every process)."""
    header = os.path.join(folder, "og_gen_%s.h" % R.name)
    with open(header, "w") as fh:
        fh.write(R.header)
    exe = os.path.join(folder, "probe_%s" % R.name)
    base = ["g++"] + PROBE_FLAGS + ["-DOG_GEN_HEADER=\"%s\"" % header, PROBE_SOURCE, "-o", exe]
    proc = subprocess.run(base + ["-static-libasan", "-static-libubsan"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if proc.returncode != 0:
        proc = subprocess.run(base, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert proc.returncode == 0, proc.stdout[-3000:]
    return exe


def run_probe(R, exe, folder, key):
    cv = np.ascontiguousarray(R.program.cvec, dtype=np.float64)
    data = os.path.join(folder, "%s_%s.bin" % (R.name, key))
    np.concatenate([R.x[key], R.h[key], cv if cv.size else np.zeros(1)]).tofile(data)
    env = dict(os.environ, UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    proc = subprocess.run([exe, data], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, env=env, timeout=300)
    assert proc.returncode == 0 and "runtime error" not in proc.stdout, proc.stdout[-3000:]
    return {k: int(v) for k, v in re.findall(r"(\w+)=(-?\d+)", proc.stdout.strip().split("\n")[-1])}


@pytest.mark.parametrize("name", PROBED)
def test_host_probe_cached_sums_equal_in_place_sums_under_sanitizers(name, probe_dir):
    R = ref(name)
    exe = build_probe(R, probe_dir)
    n, blocks = R.program.n, term_blocks(name, R.prob)
    cached, in_place = PAIRS[name]
    for key in R.x:
        got = run_probe(R, exe, probe_dir, key)
        assert got["mismatches"] == 0
        assert (got["blocks"], got["terms"], got["columns"]) == (len(blocks), R.window["n_terms"], n)
        assert (got["cached"], got["in_place"], got["neither"]) == (cached, in_place, len(blocks) * n - cached - in_place)
        # the cache was handed out for every pair that is not in place, and for every block at the base point
        assert got["cache_reads"] >= (cached + got["neither"]) + len(blocks)
        assert (got["nan"] > 0) == (key == "bad")


ARITHMETIC = [name for name in PROBED if name != "nonfinite"]       # (sqrt is not arithmetic; its NaN has no bits to compare)


@pytest.mark.parametrize("name", PROBED)
def test_cpu_chain_interpreter_twin_numpy_and_fsum(name):
    R = ref(name)
    prob, obj, P = R.prob, R.obj, R.program
    eps = np.finfo(float).eps
    for key in ("guess", "near"):
        x, h = R.x[key], R.h[key]
        F = np_path.stacked_values(prob, obj, x)
        assert P.m == F.size and np.array_equal(program_eval.evaluate(P, prob, x), F)
        Ft = R.tw.values(x)
        assert np.all(np.abs(Ft - F) <= 1e-11 * np.maximum(1.0, np.abs(F)) + 1e-10)
        assert Ft[0] == F[0], "the twin's cost row has other bits than NumPy's"
        assert np.array_equal(h, np_path.fd_step(x, R.lb, R.ub))
        F0, JT = R.sweep(key)
        F_np, _, JT_np = R.np_sweep(key)
        assert np.array_equal(F0, Ft) and np.array_equal(F_np, F)
        err, bound = np.abs(JT - JT_np), fd_noise_bound(JT_np, R.scales(key, F), h)
        assert np.all(err <= bound), "worst ratio %.3g" % np.max(err / np.maximum(bound, 1e-300))
        assert_zero_pattern(P, np.arange(P.n), JT, JT_np, name)
        # a left-to-right sum of N terms is within (N - 1) eps sum|t| of the exact sum
        mayer, t = R.terms(key)
        assert t.size == R.window["n_terms"]
        assert abs(math.fsum([Ft[0], -mayer] + list(-t))) <= (t.size - 1) * eps * float(np.sum(np.abs(t)))
    if name == "nonfinite":
        Fb = R.tw.values(R.x["bad"])
        assert np.array_equal(np.isnan(Fb), np.isnan(np_path.stacked_values(prob, obj, R.x["bad"])))
        assert np.isnan(Fb[0]) and np.sum(np.isnan(Fb)) == 1


LIMIT = {"terms2048": [293] * 6 + [290], "terms2049": [293] * 6 + [291]}
LIMIT_WINDOW = {"terms2048": (2048, 2064, 59112), "terms2049": (2049, 0, 42600)}


def limit_ref(name):
    """1c: one state, no control, running cost on (even seed).  One shape is kept at a time."""
    if name not in _REFS:
        for other in LIMIT:
            _REFS.pop(other, None)
        nodes = LIMIT[name]
        R = _REFS[name] = Ref(name, make_problem((nodes, [1] * 7, [0] * 7, [True] * 6), seed=12, sqrt_term=True))
        bad = R.x["guess"].copy()
        bad[R.prob.index_states(0, 0, 2)] = -10.0
        R.add_point("bad", bad)
        R.cols = np.unique(np.r_[spread_columns(R.prob), np.arange(0, R.program.n - 7, 97)]).astype(np.int32)
    return _REFS[name]


@pytest.mark.parametrize("name", list(LIMIT))
def test_the_mirror_at_the_cache_limit(name):
    R = limit_ref(name)
    w = R.window
    assert (w["n_terms"], w["term_doubles"], w["fused_bytes"]) == LIMIT_WINDOW[name]
    assert w["one_launch"] and (R.program.n, R.program.m) == (2048 + 7 + (name == "terms2049"), 4398 + 2 * (name == "terms2049"))
    assert ("N_TERMS = %d;" % w["n_terms"]) in R.header
    module = build.build_module(R.header)
    info = OgkInfo()
    import ctypes as C
    assert C.CDLL(module).ogk_get_info(C.byref(info)) == 0
    assert info.fused_ok == 1 and (info.n, info.m) == (R.program.n, R.program.m)


# ================================================================================================ GPU
def _against_np_path(R, key, F0, JT, cols=None):
    F_np, h_np, JT_np = R.np_sweep(key, cols)
    cols = np.arange(R.program.n) if cols is None else cols
    assert np.array_equal(h_np, R.h[key])
    scale = R.scales(key, F_np)
    if R.name in ARITHMETIC:
        assert F0[0] == F_np[0], "cost row of %s at %s" % (R.name, key)
    assert np.all(np.abs(F0 - F_np) <= 1e-9 * scale)
    err, bound = np.abs(JT[cols] - JT_np), fd_noise_bound(JT_np, scale, R.h[key][cols])
    assert np.all(err <= bound), "%s at %s: worst ratio %.3g" % (R.name, key, np.max(err / np.maximum(bound, 1e-300)))
    assert_zero_pattern(R.program, cols, JT[cols], JT_np, "%s at %s" % (R.name, key))


@pytest.mark.gpu
@pytest.mark.parametrize("name", SWEPT)
def test_gpu_cached_sums_give_the_twins_bits_in_every_form(name, monkeypatch):
    """Evaluation, full sweep and column shards cut inside a light workgroup's run of 16 columns, at two points, in the
    one-launch, the split and the dense form: the twin's bits; and ``np_path.sweep`` on every column."""
    from opengoddard_amd.engine import HipEngine
    monkeypatch.delenv("OGPSX_SWEEP", raising=False)
    assert_the_suite_has_every_kind_of_workgroup()
    R = ref(name)
    n = R.program.n
    t0 = time.time()
    eng = R.engine()
    assert eng.one_launch and eng.sweep_mode == "fused"
    seconds_to_build = time.time() - t0
    for key in ("guess", "near"):
        x, h = R.x[key], R.h[key]
        F0c, JTc = R.sweep(key)
        assert np.array_equal(eng.eval_stacked(x), F0c)
        F0, JT = eng.sweep_stacked(x, h)
        assert np.array_equal(F0, F0c) and np.array_equal(JT, JTc), key
        for lo, hi in ((0, 5), (5, 21), (21, n - 1), (n - 1, n)):
            Fs, JTs = eng.sweep_stacked(x, h, lo, hi)
            assert np.array_equal(Fs, F0c) and np.array_equal(JTs, JTc[lo:hi]), "columns [%d, %d) at %s" % (lo, hi, key)
        _against_np_path(R, key, F0, JT)
    eng.close()
    for layout in ("split", "dense"):
        monkeypatch.setenv("OGPSX_SWEEP", layout)
        other = HipEngine(R.prob, R.obj, program=R.program)
        assert other.sweep_mode == layout and not other.one_launch
        for key in ("guess", "near"):
            F0c, JTc = R.sweep(key)
            assert np.array_equal(other.eval_stacked(R.x[key]), F0c)
            Fl, JTl = other.sweep_stacked(R.x[key], R.h[key])
            assert np.array_equal(Fl, F0c) and np.array_equal(JTl, JTc), (layout, key)
            for lo, hi in ((0, 5), (5, 21), (21, n - 1), (n - 1, n)):
                assert np.array_equal(other.sweep_stacked(R.x[key], R.h[key], lo, hi)[1], JTc[lo:hi]), (layout, key, lo)
        other.close()
    if name == "blocks64":
        record_measurement("test_gpu_cached_sums_give_the_twins_bits_in_every_form", shape=name, blocks=64,
                           n_terms=R.window["n_terms"], seconds_to_engine=seconds_to_build, seconds=time.time() - t0)


@pytest.mark.gpu
@pytest.mark.parametrize("name", SWEPT)
def test_gpu_exact_jacobians_of_the_sum_problems(name, monkeypatch):
    """The dual path sums in place on another scalar type: the twin's bits, and complex-step derivatives to 1e-12 of the
    row's largest entry (the bound of ``test_gpu_exact_jacobian_against_complex_step_at_baseline_sizes``)."""
    from oracle import exact_jac
    monkeypatch.delenv("OGPSX_SWEEP", raising=False)
    R = ref(name)
    eng = R.engine()
    for key in ("guess", "near"):
        Fe, JE = eng.exact_stacked(R.x[key])
        Fec, JEc = R.exact(key)
        assert np.array_equal(Fe, Fec) and np.array_equal(JE, JEc), key
        JC = exact_jac.jacobian(R.program, R.prob, R.x[key])
        scale = np.maximum(1.0, np.abs(JC).max(axis=0))[None, :]
        assert np.max(np.abs(JE - JC) / scale) <= 1e-12, key
    lo, hi = 5, min(21, eng.n - 1)
    assert np.array_equal(eng.exact_stacked(R.x["near"], lo, hi)[1], R.exact("near")[1][lo:hi])
    eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["rem_16_25", "mean", "nonfinite"])
def test_gpu_batch_of_three_points_equals_the_single_sweeps(name, monkeypatch):
    """Three lanes at three different points: every lane holds what a sweep of its point alone gives, bit for bit; with
    the non-finite point in the middle lane (``nonfinite``) the NaN stays there."""
    monkeypatch.delenv("OGPSX_SWEEP", raising=False)
    R = ref(name)
    if "far" not in R.x:
        rng = np.random.default_rng(9)
        R.add_point("far", np.clip(R.x["guess"] + 1e-2 * rng.standard_normal(R.program.n), R.lb, R.ub))
    eng = R.engine()
    keys = ("guess", "bad", "far") if name == "nonfinite" else ("guess", "near", "far")
    single = {key: eng.sweep_stacked(R.x[key], R.h[key]) for key in keys}
    batch = eng.batch(3)
    X, H = np.stack([R.x[k] for k in keys]), np.stack([R.h[k] for k in keys])
    F0, vals, nonfinite = batch.sweep(X, H)
    indptr, rows = codegen.sparsity(R.program)
    for lane, key in enumerate(keys):
        F_want, JT_want = R.sweep(key)
        assert np.array_equal(single[key][0], F_want, equal_nan=True) and np.array_equal(single[key][1], JT_want, equal_nan=True)
        assert np.array_equal(F0[lane], F_want, equal_nan=True), "F of lane %d" % lane
        assert np.array_equal(batch.dense(lane), JT_want, equal_nan=True), "matrix of lane %d" % lane
        bad_rows = int(np.sum(~np.isfinite(F_want)))
        assert nonfinite[lane] == bad_rows and (bad_rows > 0) == (key == "bad")
        if key != "bad":
            assert np.isfinite(batch.dense(lane)).all()
            assert np.array_equal(vals[lane], JT_want[np.repeat(np.arange(R.program.n), np.diff(indptr)), rows])
        else:
            assert np.isnan(F_want[0]) and np.isnan(batch.dense(lane)[:, 0]).all()
    assert np.array_equal(batch.values(X), np.stack([R.sweep(k)[0] for k in keys]), equal_nan=True)
    eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize("layout", ["fused", "split"])
def test_gpu_a_nonfinite_term_fills_the_cost_row_of_every_column_and_is_cleaned_up(layout, monkeypatch):
    """finite -> bad -> bad -> finite -> other into a registered device buffer: after each sweep the whole matrix is the
    twin's - NaN in the cost row of every column at the bad point, exact structural zeros afterwards."""
    import torch
    from opengoddard_amd.engine import HipEngine
    monkeypatch.delenv("OGPSX_SWEEP", raising=False)
    if layout == "split":
        monkeypatch.setenv("OGPSX_SWEEP", "split")
    R = ref("nonfinite")
    eng = HipEngine(R.prob, R.obj, program=R.program)
    assert eng.sweep_mode == layout and eng.one_launch == (layout == "fused")
    n, m = eng.n, eng.m
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream().cuda_stream
    d_F = torch.empty(m, dtype=torch.float64, device=dev)
    d_JT = torch.full((n, m), 7.0, dtype=torch.float64, device=dev)
    eng.register_jt_dev(d_JT.data_ptr(), 0, n, stream)
    structural = np.zeros((n, m), dtype=bool)
    indptr, rows = codegen.sparsity(R.program)
    structural[np.repeat(np.arange(n), np.diff(indptr)), rows] = True
    for step, key in enumerate(("guess", "bad", "bad", "guess", "near")):
        F_want, JT_want = R.sweep(key)
        d_x, d_h = torch.from_numpy(R.x[key]).to(dev), torch.from_numpy(R.h[key]).to(dev)
        eng.sweep_dev(d_x.data_ptr(), d_h.data_ptr(), 0, n, d_JT.data_ptr(), d_F.data_ptr(), stream)
        torch.cuda.synchronize()
        JT = d_JT.cpu().numpy()
        assert np.array_equal(d_F.cpu().numpy(), F_want, equal_nan=True), "F at step %d" % step
        assert np.array_equal(JT, JT_want, equal_nan=True), "J_T at step %d" % step
        assert eng.nonfinite_rows(stream) == np.sum(~np.isfinite(F_want)) == (1 if key == "bad" else 0)
        if key == "bad":
            assert np.isnan(F_want[0]) and np.isnan(JT[:, 0]).all() and np.isfinite(JT[:, 1:]).all()
        else:
            assert not JT[~structural].any() and np.isfinite(JT).all()
    eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(LIMIT))
def test_gpu_the_largest_term_cache_and_the_first_module_without_one(name, monkeypatch):
    """``N_TERMS`` = 2048 (2064 doubles of cache) and 2049 (every sum in place, no cache in the LDS window), both in one
    launch: evaluation and full sweep at a finite and a non-finite point, the split form, a registered buffer, a shard
    and a captured graph replayed at another point give the twin's bits; ``np_path.sweep`` on a spread of columns."""
    import torch
    from opengoddard_amd.engine import HipEngine
    monkeypatch.delenv("OGPSX_SWEEP", raising=False)
    t0 = time.time()
    R = limit_ref(name)
    w = R.window
    assert (w["n_terms"], w["term_doubles"], w["fused_bytes"]) == LIMIT_WINDOW[name] and w["one_launch"]
    eng = R.engine()
    assert eng.one_launch and eng.sweep_mode == "fused"
    n, m = eng.n, eng.m
    for key in ("guess", "bad"):
        F0c, JTc = R.sweep(key)
        assert np.isfinite(F0c).all() == (key == "guess")
        assert np.array_equal(eng.eval_stacked(R.x[key]), F0c, equal_nan=True)
        F0, JT = eng.sweep_stacked(R.x[key], R.h[key])
        assert np.array_equal(F0, F0c, equal_nan=True) and np.array_equal(JT, JTc, equal_nan=True), key
        if key == "guess":
            _against_np_path(R, key, F0, JT, R.cols)
    lo, hi = n // 3, n - 1
    assert np.array_equal(eng.sweep_stacked(R.x["guess"], R.h["guess"], lo, hi)[1], R.sweep("guess")[1][lo:hi])
    # a registered device buffer through the non-finite point and back, then a captured graph replayed at another point
    dev = torch.device("cuda", 0)
    d_x = torch.zeros(n, dtype=torch.float64, device=dev)
    d_h = torch.zeros(n, dtype=torch.float64, device=dev)
    d_F = torch.empty(m, dtype=torch.float64, device=dev)
    d_JT = torch.full((n, m), 7.0, dtype=torch.float64, device=dev)

    def load(key):
        d_x.copy_(torch.from_numpy(R.x[key]))
        d_h.copy_(torch.from_numpy(R.h[key]))

    def check(key, what):
        F_want, JT_want = R.sweep(key)
        assert np.array_equal(d_F.cpu().numpy(), F_want, equal_nan=True), what
        assert np.array_equal(d_JT.cpu().numpy(), JT_want, equal_nan=True), what
        assert eng.nonfinite_rows(0) == np.sum(~np.isfinite(F_want)), what

    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        eng.register_jt_dev(d_JT.data_ptr(), 0, n, side.cuda_stream)
        for key in ("guess", "bad", "guess"):
            load(key)
            eng.sweep_dev(d_x.data_ptr(), d_h.data_ptr(), 0, n, d_JT.data_ptr(), d_F.data_ptr(), side.cuda_stream)
            torch.cuda.synchronize()
            check(key, "registered buffer at %s" % key)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        eng.sweep_dev(d_x.data_ptr(), d_h.data_ptr(), 0, n, d_JT.data_ptr(), d_F.data_ptr(),
                      torch.cuda.current_stream().cuda_stream)
    for key in ("near", "bad", "near"):
        load(key)
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        check(key, "replay at %s" % key)
    del graph
    eng.close()
    monkeypatch.setenv("OGPSX_SWEEP", "split")
    other = HipEngine(R.prob, R.obj, program=R.program)
    assert other.sweep_mode == "split" and not other.one_launch
    Fl, JTl = other.sweep_stacked(R.x["guess"], R.h["guess"])
    assert np.array_equal(Fl, R.sweep("guess")[0]) and np.array_equal(JTl, R.sweep("guess")[1])
    other.close()
    record_measurement("test_gpu_the_largest_term_cache_and_the_first_module_without_one", shape=name, n=n, m=m,
                       n_terms=w["n_terms"], term_doubles=w["term_doubles"], fused_bytes=w["fused_bytes"],
                       columns=int(R.cols.size), seconds=time.time() - t0)
