"""Nonlocal dynamics on the GPU: the cases of ``nonlocal_cases`` - every one of them sets bit 1 of a collocation slot's
``reads`` word, which no registered problem does - through every kernel that branches on the bit and takes a Jacobian or
a sweep as its result: ``ogk_fused`` (``fz_tile_body``), ``ogk_eval`` + ``ogk_sweep`` (``tile_body``), the dense sweep,
``ogk_fused_batch``, ``ogk_exact_struct``, ``ogk_exact`` and ``ogk_exact_struct_batch``.  (The derivative kernels -
``ogk_exact_adj``, ``ogk_exact_hvp``, ``ogk_exact_hess``, ``ogk_exact_mix`` - meet ``NL2``, ``NL0`` and ``NLP`` through their
own case tables.)

The CPU twin is the bit reference, as everywhere in this suite; tests/test_nonlocal.py bounds the twin's own distance from
``oracle.np_path`` and ``oracle.exact_jac`` and shows that ignoring bit 1 would move entries of the own blocks by at least
1e-4 on every case but ``NLX``.  ``__graft_entry__.build`` compiles the modules, twins and batch parts ahead of time; a
test takes well under a second of GPU time.
"""
import numpy as np
import pytest

import nonlocal_cases as nl
from conftest import record_measurement
from opengoddard_amd import _native, codegen

pytestmark = pytest.mark.gpu

FORMS = ("fused", "split", "dense")
BAD_KEY, BAD_NODE = "NL2", 3            # x_0[3] = 1e200: np.sum(x * x) is inf, every defect row of x in phase 0 non-finite


class _Ref:
    """One case's references from the CPU twin - F and the FD sweep at the three points (and at the non-finite point of
    ``NL2``), the exact Jacobian at the three points - computed once, shared by the tests below, never written to."""

    def __init__(self, key):
        from oracle import exact_jac, np_path, twin
        import test_exact_surface as surface
        self.C = C = nl.case(key)
        self.tw = tw = twin.Twin(C.prob, C.obj, program=C.program, header=C.header)
        lb, ub = np_path.bounds_arrays(C.prob)
        self.x = {"p%d" % i: x for i, x in enumerate(C.points)}
        if key == BAD_KEY:
            bad = C.points[0].copy()
            bad[C.prob.index_states(0, 0, BAD_NODE)] = 1e200
            self.x["bad"] = bad
        self.h = {k: _native.fd_step(x, lb, ub) for k, x in self.x.items()}
        self.sweep = {k: tw.sweep(self.x[k], self.h[k]) for k in self.x}
        self.exact = {k: tw.exact(self.x[k]) for k in self.x if k != "bad"}
        for k in self.exact:
            assert np.isfinite(self.sweep[k][1]).all() and np.isfinite(self.exact[k][1]).all()
            assert np.array_equal(self.sweep[k][0], self.exact[k][0])
        if key == BAD_KEY:
            F, JT = self.sweep["bad"]
            N = C.prob.nodes[0]
            row0 = [s[4] for s in nl.slots(C) if s[:2] == (0, 0)][0]
            assert np.array_equal(np.flatnonzero(~np.isfinite(F)), np.arange(row0, row0 + N))
            assert np.isnan(JT[:, row0:row0 + N]).all()
        # the twin's own distance from the independent references, for profiles/nonlocal.md
        x = C.points[1]
        F = np_path.stacked_values(C.prob, C.obj, x)
        _, _, JTo = np_path.sweep(C.prob, C.obj, x)
        scale = np.maximum(1.0, np.abs(F)) + 50.0 * max(np.abs(D).max() for D in C.prob.D)
        bound = 1e-9 * np.abs(JTo) + 64 * np.finfo(float).eps * scale[None, :] / np.abs(self.h["p1"])[:, None]
        JC = exact_jac.jacobian(C.at(C.thetas[0]), C.prob, x)
        record_measurement("test_nonlocal_gpu", case=key, n=C.n, m=C.m,
                           values_vs_np_path=float(np.max(np.abs(self.sweep["p1"][0] - F) / np.maximum(1.0, np.abs(F)))),
                           fd_sweep_vs_np_path_in_bounds=float(np.max(np.abs(self.sweep["p1"][1] - JTo) / bound)),
                           exact_vs_complex_step=surface.worst_error(self.exact["p1"][1], JC),
                           bite=min(nl.bite(self.exact["p1"][1], C).values()))

    def engine(self):
        from opengoddard_amd.engine import HipEngine
        eng = HipEngine(self.C.prob, self.C.obj, program=self.C.program)
        assert eng.header == self.C.header and (eng.n, eng.m) == (self.C.n, self.C.m)
        return eng


_REFS = {}


def ref(key):
    if key not in _REFS:
        _REFS[key] = _Ref(key)
    return _REFS[key]


def _form(monkeypatch, form):
    if form == "fused":
        monkeypatch.delenv("OGPSX_SWEEP", raising=False)            # the default
    else:
        monkeypatch.setenv("OGPSX_SWEEP", form)


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(torch.device("cuda", 0))


# ------------------------------------------------------------------------------------------------ 1. evaluation and sweep
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("key", nl.KEYS)
def test_evaluation_sweep_and_column_blocks_equal_the_twin(key, form, monkeypatch):
    R = ref(key)
    _form(monkeypatch, form)
    eng = R.engine()
    assert eng.sweep_mode == form and (form != "fused" or eng.one_launch)
    for k in ("p0", "p1", "p2"):
        F_want, JT_want = R.sweep[k]
        assert np.array_equal(eng.eval_stacked(R.x[k]), F_want), (key, form, k)
        F0, JT = eng.sweep_stacked(R.x[k], R.h[k])
        assert np.array_equal(F0, F_want), (key, form, k)
        assert np.array_equal(JT, JT_want), (key, form, k, np.argwhere(JT != JT_want)[:4])
    # column blocks that cut a state's own slice off the 16-column grid (on NL130: one that starts in the ninth tile)
    F_want, JT_want = R.sweep["p1"]
    for lo, hi in nl.cuts(R.C):
        F0, JT = eng.sweep_stacked(R.x["p1"], R.h["p1"], lo, hi)
        assert np.array_equal(F0, F_want) and np.array_equal(JT, JT_want[lo:hi]), (key, form, lo, hi)
    eng.close()


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("key", nl.KEYS)
def test_one_registered_buffer_through_three_points(key, form, monkeypatch):
    """A registered (persistent-zero) device buffer holds the dense sweep of the twin entry for entry after each of
    three sweeps; on ``NL2`` the second point is non-finite in every defect row of ``x`` in phase 0 (the sum over the
    state's slice is inf): NaN in those rows of every column, the count of the rows, and a clean buffer afterwards."""
    import torch
    R = ref(key)
    _form(monkeypatch, form)
    eng = R.engine()
    stream = torch.cuda.current_stream().cuda_stream
    d_F = torch.empty(eng.m, dtype=torch.float64, device=torch.device("cuda", 0))
    d_JT = torch.full((eng.n, eng.m), 7.0, dtype=torch.float64, device=d_F.device)
    eng.register_jt_dev(d_JT.data_ptr(), 0, eng.n, stream)
    try:
        for k in (("p0", "bad", "p1") if key == BAD_KEY else ("p0", "p1", "p2")):
            F_want, JT_want = R.sweep[k]
            d_x, d_h = _dev(R.x[k]), _dev(R.h[k])
            eng.sweep_dev(d_x.data_ptr(), d_h.data_ptr(), 0, eng.n, d_JT.data_ptr(), d_F.data_ptr(), stream)
            torch.cuda.synchronize()
            assert np.array_equal(d_F.cpu().numpy(), F_want, equal_nan=True), (key, form, k)
            got = d_JT.cpu().numpy()
            assert np.array_equal(np.isnan(got), np.isnan(JT_want)), (key, form, k)
            assert np.array_equal(got, JT_want, equal_nan=True), (key, form, k)
            assert eng.nonfinite_rows(stream) == np.sum(~np.isfinite(F_want)) == (R.C.prob.nodes[0] if k == "bad" else 0)
    finally:
        eng.unregister_jt_dev(d_JT.data_ptr())
    eng.close()


# ------------------------------------------------------------------------------------------------ 2. exact Jacobians
@pytest.mark.parametrize("layout", ["structured", "dense"])
@pytest.mark.parametrize("key", nl.EXACT_KEYS)
def test_exact_jacobian_is_bit_identical_to_the_twin(key, layout, monkeypatch):
    """``ogk_exact_struct`` (the structured sweep's work lists) and ``ogk_exact`` (``OGPSX_SWEEP=dense``)."""
    R = ref(key)
    _form(monkeypatch, "dense" if layout == "dense" else "fused")
    eng = R.engine()
    for k in ("p0", "p1", "p2"):
        F_want, JT_want = R.exact[k]
        F0, JE = eng.exact_stacked(R.x[k])
        assert np.array_equal(F0, F_want) and np.array_equal(F0, eng.eval_stacked(R.x[k])), (key, layout, k)
        assert np.array_equal(JE, JT_want), (key, layout, k, np.argwhere(JE != JT_want)[:4])
    for lo, hi in nl.cuts(R.C) + [(eng.n // 3, 2 * eng.n // 3 + 1)]:
        assert np.array_equal(eng.exact_stacked(R.x["p1"], lo, hi)[1], R.exact["p1"][1][lo:hi]), (key, layout, lo, hi)
    assert eng.exact_stacked(R.x["p1"], 5, 5)[1].shape == (0, eng.m)
    # ... and the entries that only bit 1 brings are there
    assert min(nl.bite(JE, R.C).values()) >= nl.BITE
    eng.close()


# ------------------------------------------------------------------------------------------------ 3. batches
@pytest.mark.parametrize("key", nl.BATCH_KEYS)
def test_a_batch_of_two_in_three_lanes(key, monkeypatch):
    """Capacity 3, count 2, the lanes at two different points: the FD sweep (``ogk_fused_batch``) and the exact Jacobian
    (``ogk_exact_struct_batch``) give the single-point results and the twin's; lane 2's matrix, its count and the third
    rows of the result arrays stay as they were."""
    import torch
    R = ref(key)
    _form(monkeypatch, "fused")
    eng = R.engine()
    indptr, rows = eng.pattern()
    at = np.repeat(np.arange(eng.n), np.diff(indptr))
    batch = eng.batch(3)
    assert batch.capacity == 3 and batch.nnz == indptr[-1]
    stream = torch.cuda.current_stream().cuda_stream
    order = ["p2", "p0", "p1"]
    X, H = np.stack([R.x[k] for k in order]), np.stack([R.h[k] for k in order])
    F0, vals, nonfinite = batch.sweep(X, H)                      # every lane once: lane 2 now holds the sweep at p1
    assert not nonfinite.any()
    for lane, k in enumerate(order):
        assert np.array_equal(F0[lane], R.sweep[k][0]) and np.array_equal(vals[lane], R.sweep[k][1][at, rows])
    lane2 = batch.dense(2)
    assert np.array_equal(lane2, R.sweep["p1"][1])
    two = ["p1", "p2"]                                           # both lanes move to another point
    d_X, d_H = _dev(np.stack([R.x[k] for k in two])), _dev(np.stack([R.h[k] for k in two]))
    for kind in ("sweep", "exact"):
        want = R.sweep if kind == "sweep" else R.exact
        d_F = torch.full((3, eng.m), -7.0, dtype=torch.float64, device=d_X.device)
        d_V = torch.full((3, batch.nnz), -7.0, dtype=torch.float64, device=d_X.device)
        if kind == "sweep":
            batch.sweep_dev(2, d_X.data_ptr(), d_H.data_ptr(), d_F.data_ptr(), d_V.data_ptr(), stream)
        else:
            batch.exact_dev(2, d_X.data_ptr(), d_F.data_ptr(), d_V.data_ptr(), stream)
        torch.cuda.synchronize()
        F, V = d_F.cpu().numpy(), d_V.cpu().numpy()
        for lane, k in enumerate(two):
            single = eng.sweep_stacked(R.x[k], R.h[k]) if kind == "sweep" else eng.exact_stacked(R.x[k])
            assert np.array_equal(single[0], want[k][0]) and np.array_equal(single[1], want[k][1]), (key, kind, k)
            assert np.array_equal(F[lane], want[k][0]), (key, kind, lane)
            assert np.array_equal(V[lane], want[k][1][at, rows]), (key, kind, lane)
            assert np.array_equal(batch.dense(lane), want[k][1]), (key, kind, lane)
            assert batch.lane_dev(lane)[1] == 0
        assert np.all(F[2] == -7.0) and np.all(V[2] == -7.0)
        assert np.array_equal(batch.dense(2), lane2) and batch.lane_dev(2)[1] == 0
    eng.close()


# ------------------------------------------------------------------------------------------------ 4. pattern, pack, shards
def test_pattern_pack_and_unpack():
    """As tests/test_gpu_parity.py's test of that name, on ``NL0``: the own block - here a full one - leads a column's
    packed entries."""
    import torch
    R = ref("NL0")
    eng = R.engine()
    n, m = eng.n, eng.m
    indptr, rows = eng.pattern()
    want_ptr, want_rows = codegen.sparsity(eng.program)
    assert np.array_equal(indptr, want_ptr) and np.array_equal(rows, want_rows)
    for phase, state, leaf, N, row0, reads in nl.slots(R.C):
        for j in (leaf, leaf + N - 1):
            assert np.array_equal(rows[indptr[j]:indptr[j] + N], np.arange(row0, row0 + N))
    lo, hi = n // 5, n // 5 + n // 2
    ip, rw = eng.pattern(lo, hi)
    assert np.array_equal(ip, indptr[lo:hi + 1] - indptr[lo]) and np.array_equal(rw, rows[indptr[lo]:indptr[hi]])
    F0, JT = eng.sweep_stacked(R.x["p1"], R.h["p1"])
    assert np.array_equal(JT, R.sweep["p1"][1])
    dense = np.zeros((n, m), dtype=bool)
    dense[np.repeat(np.arange(n), np.diff(indptr)), rows] = True
    assert not JT[~dense].any()
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream().cuda_stream
    lib = _native.lib()
    d_JT = torch.from_numpy(JT[lo:hi].copy()).to(dev)
    d_vals = torch.empty(int(ip[-1]), dtype=torch.float64, device=dev)
    _native.check(lib.og_pack_dev(eng._handle, d_JT.data_ptr(), lo, hi, d_vals.data_ptr(), stream), "og_pack_dev")
    torch.cuda.synchronize()
    vals = d_vals.cpu().numpy()
    assert np.array_equal(vals, JT[lo:hi][np.repeat(np.arange(hi - lo), np.diff(ip)), rw])
    d_out = torch.full((hi - lo, m), 5.0, dtype=torch.float64, device=dev)
    _native.check(lib.og_unpack_dev(eng._handle, d_vals.data_ptr(), lo, hi, d_out.data_ptr(), stream), "og_unpack_dev")
    torch.cuda.synchronize()
    out = d_out.cpu().numpy()
    assert np.array_equal(out[dense[lo:hi]], JT[lo:hi][dense[lo:hi]]) and np.all(out[~dense[lo:hi]] == 5.0)
    eng.close()


def test_a_sharded_sweep_over_two_and_three_ranges(monkeypatch):
    """``NL0`` in column ranges: plain column blocks, and ``sharding.ShardedSweep`` on the one device - sweep and pack in
    one launch (``fz_tile_body`` writes the packed values of the own blocks itself), the ranks' messages, the reassembled
    replicas."""
    import torch
    from opengoddard_amd import sharding
    R = ref("NL0")
    _form(monkeypatch, "fused")
    eng = R.engine()
    n, m = eng.n, eng.m
    F_want, JT_want = R.sweep["p1"]
    for parts in (2, 3):
        edges = np.linspace(0, n, parts + 1).astype(int)
        pieces = [eng.sweep_stacked(R.x["p1"], R.h["p1"], lo, hi)[1] for lo, hi in zip(edges[:-1], edges[1:])]
        assert np.array_equal(np.vstack(pieces), JT_want)
    indptr, rows = eng.pattern()
    be = sharding.HipBackend(eng, torch.device("cuda", 0))
    for world in (2, 3):
        ranks = [sharding.ShardedSweep(be, n, m, rank, world) for rank in range(world)]
        for k in ("p1", "p2"):
            F_want, JT_want = R.sweep[k]
            d_x, d_h = be.upload(R.x[k]), be.upload(R.h[k])
            for sh in ranks:
                be.sweep_and_pack(sh.rank, d_x, d_h, sh.lo, sh.hi, sh.replica, sh.F0, sh.send)
            torch.cuda.synchronize()
            message = torch.cat([sh.send[:max(sh.block_vals, 1)] for sh in ranks])
            for sh in ranks:
                mine = JT_want[np.repeat(np.arange(sh.lo, sh.hi), np.diff(indptr[sh.lo:sh.hi + 1])),
                               rows[indptr[sh.lo]:indptr[sh.hi]]]
                assert np.array_equal(sh.send.cpu().numpy()[:mine.size], mine), "message of rank %d of %d" % (sh.rank, world)
                sh.recv.copy_(message)
                be.unpack(sh.rank, sh.recv, sh.replica)
            torch.cuda.synchronize()
            for sh in ranks:
                assert np.array_equal(sh.F0.cpu().numpy(), F_want)
                assert np.array_equal(sh.replica.cpu().numpy(), JT_want), "world %d, rank %d at %s" % (world, sh.rank, k)
        for sh in ranks:
            eng.unregister_jt_dev(sh.replica[sh.lo:sh.hi].data_ptr())
        del ranks
    eng.close()
