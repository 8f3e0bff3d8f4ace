"""Nonlocal dynamics (a state read across the nodes of its phase) without a GPU: the cases of ``nonlocal_cases`` through
every CPU link of the chain, and the proof that they bite - that a kernel which ignored bit 1 of a slot's ``reads`` word
would be wrong by at least ``nonlocal_cases.BITE`` on them.

* ``oracle.program_eval`` (the NumPy interpreter of the traced program) equals ``oracle.np_path`` (the user's callbacks
  run by NumPy, no generated code) bit for bit;
* the twin's values and its FD sweep are within the bounds of tests/test_random_layouts.py of ``np_path``;
* the twin's exact Jacobian, every column, is within ``test_exact_surface.BOUND`` (1e-12 of the row scale) of the
  complex-step differentiation of ``oracle.exact_jac``; nothing non-zero lies outside ``codegen.sparsity``;
* the ``reads`` words are those of ``nonlocal_cases.READS``, from ``SweepPlan`` and from the adjoint probe's structure
  report, and their union is ``{-1, 1, 2, 3}``;
* the launch geometry the shapes were chosen for is read from the emitted records.

Measured (g++): the twin's exact Jacobian within 2.7e-16 of the complex step at every case; ``max |J - diag_only(J)|`` per
slot with bit 1: 7.1e-3 (``NL3``), 5.0e-2 (``NL2``), 0.48 (``NL0``), 1.0e-2 (``NLS``), 1.2e-3 (``NL130``, analytically
``0.3 / 130 * 0.5``), 1.5e-3 (``NL100``), 7.1e-3 (``NLP``); ``NLX``: 0 - see ``nonlocal_cases.CROSS_ONLY``.
"""
import os
import re

import numpy as np
import pytest

import adjoint_cases as ac
import nonlocal_cases as nl
import test_exact_surface as surface
from opengoddard_amd import _native, codegen
from oracle import exact_jac, np_path, program_eval, twin

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def probe_dir(tmp_path_factory):
    return str(tmp_path_factory.mktemp("nonlocal_probe"))


_TWINS = {}


def _twin(C):
    if C.key not in _TWINS:
        _TWINS[C.key] = twin.Twin(C.prob, C.obj, program=C.program, header=C.header)
    return _TWINS[C.key]


def _mask(C):
    indptr, rows = codegen.sparsity(C.program)
    mask = np.zeros((C.n, C.m), dtype=bool)
    mask[np.repeat(np.arange(C.n), np.diff(indptr)), rows] = True
    return mask


@pytest.mark.parametrize("key", nl.KEYS)
def test_cpu_chain(key):
    """``np_path`` -> ``program_eval`` -> twin, values and FD sweep, with the bounds of ``test_random_layout_cpu_chain``."""
    C = nl.case(key)
    prob, obj = C.prob, C.obj
    lb, ub = np_path.bounds_arrays(prob)
    tw = _twin(C)
    for x in C.points:
        assert np.array_equal(np.clip(x, lb, ub), x)
        F = np_path.stacked_values(prob, obj, x)
        assert np.all(np.isfinite(F))
        assert np.array_equal(program_eval.evaluate(C.program, prob, x), F)
        assert np.all(np.abs(tw.values(x) - F) <= 1e-11 * np.maximum(1.0, np.abs(F)) + 1e-9)
        h = _native.fd_step(x, lb, ub)
        assert np.array_equal(h, np_path.fd_step(x, lb, ub))
        _, JT = tw.sweep(x, h)
        _, _, JTo = np_path.sweep(prob, obj, x)
        scale = np.maximum(1.0, np.abs(F)) + 50.0 * max(np.abs(D).max() for D in prob.D)
        bound = 1e-9 * np.abs(JTo) + 64 * np.finfo(float).eps * scale[None, :] / np.abs(h)[:, None]
        assert np.all(np.abs(JT - JTo) <= bound)
        assert not JT[~_mask(C)].any() and not JTo[~_mask(C)].any()


@pytest.mark.parametrize("key", nl.KEYS)
def test_the_twins_exact_jacobian_and_the_bite(key, capsys):
    """Every column against the complex step; the pattern; and per slot with bit 1 what ignoring the bit would cost."""
    C = nl.case(key)
    tw = _twin(C)
    mask = _mask(C)
    cols = np.arange(C.n, dtype=np.int32)
    worst, bites = 0.0, {}
    for t, theta in enumerate(C.thetas):
        if theta is not None:
            tw._cv[C.program.par_off:] = theta
        for x in C.points:
            F0, JE = tw.exact(x, cols)
            assert np.array_equal(F0, tw.values(x)) and np.all(np.isfinite(JE))
            JC = exact_jac.jacobian(C.at(theta), C.prob, x, list(cols))
            worst = max(worst, surface.worst_error(JE, JC))
            assert not JE[~mask].any() and not JC[~mask].any()
            for slot, gap in nl.bite(JC, C).items():
                bites[slot] = min(bites.get(slot, np.inf), gap)
            # ... and the twin, which the GPU tests compare with bit for bit, carries the same entries
            for slot, gap in nl.bite(JE, C).items():
                bites[slot] = min(bites[slot], gap)
    if C.thetas[0] is not None:
        tw._cv[C.program.par_off:] = C.thetas[0]
    with capsys.disabled():
        if os.environ.get("OG_SURFACE_REPORT"):
            print("nonlocal %-6s twin vs complex step %.2e, bite %s" % (key, worst, {k: "%.2e" % v for k, v in bites.items()}))
    assert worst <= surface.BOUND, (key, worst)
    want = {(phase, state) for phase, state, _, _, _, reads in nl.slots(C) if reads & 2}
    assert set(bites) == want and want, key
    if key in nl.CROSS_ONLY:
        # bit 1 from the other state's row alone: the own blocks are D off the diagonal, nothing here can bite
        assert max(bites.values()) <= surface.BOUND
    else:
        assert min(bites.values()) >= nl.BITE, (key, bites)


def test_every_case_but_the_cross_only_one_bites():
    assert nl.CROSS_ONLY == ("NLX",) and set(nl.CROSS_ONLY) < set(nl.KEYS)
    # the own-block derivative of NLX's terms is node-local whatever the coefficient: d(v - c v.mean() x_k)/dx_l and
    # d(u - .. - c (x * x).sum() + ..)/dv_l vanish for l != k
    C = nl.case("NLX")
    JC = exact_jac.jacobian(C.program, C.prob, C.points[0])
    for phase, state, leaf, N, row0, reads in nl.slots(C):
        block = JC[leaf:leaf + N, row0:row0 + N]
        off = ~np.eye(N, dtype=bool)
        assert reads == 3 and np.max(np.abs(block[off] - np.asarray(C.prob.D[phase]).T[off])) <= surface.BOUND
    # ... while the block between the two states is dense, through the row items
    x0 = [s for s in nl.slots(C) if s[:2] == (0, 0)][0]
    v0 = [s for s in nl.slots(C) if s[:2] == (0, 1)][0]
    cross = JC[v0[2]:v0[2] + v0[3], x0[4]:x0[4] + x0[3]]            # d defect_x(k) / d v(l)
    assert np.abs(cross[~np.eye(x0[3], dtype=bool)]).min() > 0


@pytest.mark.parametrize("key", nl.KEYS)
def test_reads_words(key, probe_dir):
    C = nl.case(key)
    got = nl.slots(C)
    assert [(s[0], s[1]) for s in got] == [(0, 0), (0, 1), (1, 0), (1, 1)]
    assert tuple(s[5] for s in got) == nl.READS[key] * 2, key
    slot_rows = nl.table(C, "OGT_SLOT")
    assert [row[6] for row in slot_rows] == [s[5] for s in got]
    exe = ac.build_probe(C, probe_dir, "g++")
    reads = ac.run_probe(C, exe, probe_dir, C.points[0], ac.weights(C)[:1], C.thetas[0], structure=True)[3]
    want = np.full(C.n, -1)
    for phase, state, leaf, N, row0, word in got:
        want[leaf:leaf + N] = word
    assert np.array_equal(reads, want)


def test_the_union_of_the_reads_words():
    seen = set()
    for key in nl.KEYS:
        seen |= {s[5] for s in nl.slots(nl.case(key))} | {-1}
    assert seen == {-1, 1, 2, 3}
    assert {s[5] for key in nl.DERIVATIVE_KEYS for s in nl.slots(nl.case(key))} == {1, 2, 3}


def test_the_launch_geometry_the_shapes_were_chosen_for():
    """From the emitted records, not from arithmetic on the node counts."""
    waves = codegen.SWEEP_WAVES
    with open(os.path.join(ROOT, "opengoddard_amd", "csrc", "ogk_kernels.hip")) as fh:
        kernels = fh.read()
    # (the rule this test restates: a tile workgroup of nct column tiles has a free wavefront for the diagonal term?)
    assert "const int diag_wave = nct < SWEEP_WAVES - 2 ? SWEEP_WAVES - 3 : -1;" in kernels
    assert re.search(r"constexpr int SWEEP_THREADS = %d;" % (64 * waves), kernels)

    def diag_wave(nct):
        return waves - 3 if nct < waves - 2 else -1

    for key in nl.KEYS:
        C = nl.case(key)
        win = codegen.lds_window(C.program)
        assert win["one_launch"], key
        assert win["fused_bytes"] == {21: 3792, 130: 21088, 100: 16000}[C.prob.nodes[0]]
        ft = [row for row in nl.table(C, "OGT_FTILE") if row[0] == 0]      # slot 0: {slot, first column tile, node tile, tiles}
        groups = sorted({(row[1], row[3]) for row in ft})
        if key == "NL130":
            # nine column tiles over two tile workgroups: the second starts at a column tile that is not the first
            assert groups == [(0, 5), (5, 4)] and any(row[1] > 0 for row in ft)
            assert all(diag_wave(nct) >= 0 for _, nct in groups)
            assert len({row[2] for row in ft}) == 9
        elif key == "NL100":
            # one full workgroup: every wavefront but the last holds a column tile, none is free for the diagonal term
            assert groups == [(0, 7)] and diag_wave(7) < 0
        else:
            assert groups == [(0, 2)] and diag_wave(2) >= 0 and C.prob.nodes[0] % 4 and C.prob.nodes[0] % 16 == 5
    # the heavy columns: the first phase's final time everywhere (its items lie in both node tiles); on NL0 also x[-1] of
    # the long phase, which every defect row of v reads (x[0] and v[0] are read by rows of their OWN state: those entries
    # are the own block's, not items); every state column of the long phase of NLX; 22 of NLS
    tf0 = nl.case("NL3").n - 2
    for key, want in (("NL3", [tf0]), ("NL0", [20, tf0])):
        plan = codegen.SweepPlan(nl.case(key).program)
        many = [j for j, t in enumerate(plan.col_tile) if t == "many"]
        assert many == want and set(many) == set(plan.heavy), key
    for key, count in (("NLX", 44), ("NLS", 22)):
        plan = codegen.SweepPlan(nl.case(key).program)
        assert sum(1 for t in plan.col_tile if t == "many") == count and len(plan.heavy) == count


def test_the_cuts_leave_the_16_column_grid():
    for key in nl.KEYS:
        C = nl.case(key)
        phase, state, leaf, N, row0, reads = nl.slots(C)[0]
        cuts = nl.cuts(C)
        assert cuts[:3] == [(leaf + 3, leaf + 19), (leaf + 16, leaf + N), (C.n - 1, C.n)]
        assert all(0 <= lo < hi <= C.n for lo, hi in cuts)
        if key == "NL130":
            assert len(cuts) == 4 and (cuts[3][0] - leaf) // 16 == 8 and (cuts[3][0] - leaf) % 16
        else:
            assert len(cuts) == 3
