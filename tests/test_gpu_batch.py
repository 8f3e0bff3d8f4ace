"""Batches of points on the GPU (``og_batch_*``, ``HipEngine.batch``, ``Problem.evaluate_batch``).  Every comparison
is BITWISE against the single-point path of the same build (``HipEngine.eval_stacked`` / ``sweep_stacked`` /
``pattern``), which tests/test_gpu_parity.py pins to the CPU twin, the NumPy restatement and the reference's goldens;
the first test also checks the lanes' matrices against the reference's goldens directly."""
import ctypes as C

import numpy as np
import pytest

from conftest import fd_noise_bound, inject_reference_lgl
from opengoddard_amd import _native, problems

pytestmark = pytest.mark.gpu


def _engine(name, lgl=None):
    from opengoddard_amd.engine import HipEngine
    prob, obj = problems.build(name)
    if lgl is not None:
        inject_reference_lgl(prob, lgl)
    return prob, obj, HipEngine(prob, obj)


def _gather(eng, JT):
    """The entries of a dense n x m matrix at the engine's pattern, in pattern order."""
    indptr, rows = eng.pattern()
    return JT[np.repeat(np.arange(eng.n), np.diff(indptr)), rows]


def _bounds(prob):
    from oracle import np_path
    return np_path.bounds_arrays(prob)


def _bad_point(prob, state):
    """A point whose F has non-finite rows (tests/test_gpu_parity.py: mass = 0 at one node -> division by zero)."""
    lb, ub = _bounds(prob)
    x = np.clip(prob.p, lb, ub)
    x[prob.index_states(state, 0, 7)] = 0.0
    return x, _native.fd_step(x, lb, ub)


def _good_point(prob):
    lb, ub = _bounds(prob)
    x = np.clip(prob.p, lb, ub)
    return x, _native.fd_step(x, lb, ub)


@pytest.mark.parametrize("name", problems.NAMES)
def test_batched_sweep_equals_the_single_point_sweep_and_the_goldens(name, golden, lgl_golden):
    from test_gpu_parity import row_scales
    G = golden("cfg_" + name)
    prob, obj, eng = _engine(name, lgl_golden)
    X, H = np.ascontiguousarray(G["x"]), np.ascontiguousarray(G["h"])
    assert X.shape[0] == 3
    batch = eng.batch(3)
    assert batch.capacity == 3
    F0, vals, nonfinite = batch.sweep(X, H)
    assert not nonfinite.any()
    indptr, rows = batch.pattern
    assert vals.shape == (3, indptr[-1])
    cols = G["cols"]
    for k in range(3):
        F1, JT1 = eng.sweep_stacked(X[k], H[k])
        assert np.array_equal(F0[k], F1), "F differs in lane %d" % k
        assert np.array_equal(vals[k], _gather(eng, JT1)), "packed non-zeros differ in lane %d" % k
        dense = batch.dense(k)
        assert np.array_equal(dense, JT1), "dense matrix differs in lane %d" % k
        # directly, not by transitivity: the lane against the reference's golden
        scale = row_scales(eng, prob, X[k], G["F"][k])
        JTg = G["JT"][k]
        err, bound = np.abs(dense[cols] - JTg), fd_noise_bound(JTg, scale, H[k][cols], factor=4.0)
        assert np.all(err <= bound), "lane %d outside the FD noise bound of the golden: worst ratio %.3g" % \
            (k, np.max(err / np.maximum(bound, 1e-300)))
    eng.close()


@pytest.mark.parametrize("name,state", [("polar_tsto", 4), ("brachistochrone", None)])
def test_a_lane_does_not_depend_on_its_position_or_its_companions(name, state, golden):
    G = golden("cfg_" + name)
    prob, obj, eng = _engine(name)
    cap = 4
    batch = eng.batch(cap)
    x, h = G["x"][0], G["h"][0]
    if state is None:
        bad = (G["x"][1].copy(), G["h"][1].copy())
        bad[0][2] = np.nan
    else:
        bad = _bad_point(prob, state)
    assert not np.isfinite(eng.eval_stacked(bad[0])).all()
    companions = [(G["x"][1], G["h"][1]), bad, (G["x"][2], G["h"][2])]
    F1, JT1 = eng.sweep_stacked(x, h)
    packed1 = _gather(eng, JT1)
    turn = 0
    for count in (1, 2, cap):
        for lane in (0, 1, cap - 1):
            if lane >= count:
                continue
            P, Hs, is_bad = np.empty((count, eng.n)), np.empty((count, eng.n)), np.zeros(count, dtype=bool)
            for k in range(count):
                if k == lane:
                    P[k], Hs[k] = x, h
                else:
                    P[k], Hs[k] = companions[turn % 3]
                    is_bad[k] = turn % 3 == 1
                    turn += 1
            F0, vals, nonfinite = batch.sweep(P, Hs)
            what = "count %d, lane %d" % (count, lane)
            assert np.array_equal(F0[lane], F1), what
            assert np.array_equal(vals[lane], packed1), what
            assert np.array_equal(batch.dense(lane), JT1), what
            assert np.array_equal(nonfinite != 0, is_bad), what
    eng.close()


@pytest.mark.parametrize("name,state", [("goddard", 2), ("polar_tsto", 4)])
def test_non_finite_rows_stay_in_their_lane(name, state):
    """[good, bad, good] -> [bad, good, good] -> [good, good, good]: after each batch every lane holds what a
    single-point handle holds after the same sequence of points (NaN rows in every column at a bad point, cleaned by
    the lane's next sweep), ``nonfinite`` names exactly the bad lanes, nothing lingers at the end."""
    from opengoddard_amd.engine import HipEngine
    prob, obj, eng = _engine(name)
    good, bad = _good_point(prob), _bad_point(prob, state)
    batch = eng.batch(3)
    steps = [[good, bad, good], [bad, good, good], [good, good, good]]
    refs = [HipEngine(*problems.build(name)) for _ in range(3)]
    for step in steps:
        P, H = np.stack([pt[0] for pt in step]), np.stack([pt[1] for pt in step])
        F0, vals, nonfinite = batch.sweep(P, H)
        assert np.array_equal(nonfinite != 0, np.array([pt is bad for pt in step]))
        for k in range(3):
            Fr, JTr = refs[k].sweep_stacked(step[k][0], step[k][1])
            assert np.array_equal(F0[k], Fr, equal_nan=True)
            dense = batch.dense(k)
            assert np.array_equal(np.isnan(dense), np.isnan(JTr)), "lane %d" % k
            assert np.array_equal(dense, JTr, equal_nan=True), "lane %d" % k
            assert batch.lane_dev(k)[1] == nonfinite[k]
            if step[k] is bad:
                assert np.isnan(dense).any() and nonfinite[k] == np.sum(~np.isfinite(Fr))
            else:
                assert np.array_equal(vals[k], _gather(refs[k], JTr))
    for k in range(3):
        assert np.isfinite(batch.dense(k)).all()
    for ref in refs:
        ref.close()
    eng.close()


@pytest.mark.parametrize("name", ["goddard", "polar_tsto"])
def test_batched_values_equal_the_single_evaluations(name, golden):
    G = golden("cfg_" + name)
    prob, obj, eng = _engine(name)
    batch = eng.batch(3)
    X = np.ascontiguousarray(G["x"])
    for _ in range(2):                                # (the two non-finite counters alternate)
        F = batch.values(X)
        for k in range(3):
            assert np.array_equal(F[k], eng.eval_stacked(X[k]))
    F = batch.values(X[1:2])
    assert np.array_equal(F[0], eng.eval_stacked(X[1]))
    # evaluations between sweeps do not disturb a lane's persistent-zero matrix
    F0, vals, _ = batch.sweep(X, np.ascontiguousarray(G["h"]))
    batch.values(X)
    F0b, valsb, _ = batch.sweep(X, np.ascontiguousarray(G["h"]))
    assert np.array_equal(F0, F0b) and np.array_equal(vals, valsb)
    assert np.array_equal(batch.dense(2), eng.sweep_stacked(X[2], G["h"][2])[1])
    eng.close()


@pytest.mark.parametrize("name,state", [("goddard", 2), ("polar_tsto", 4)])
def test_persistent_result_arrays_receive_the_same_bits(name, state, golden):
    """``sweep(persistent=True)``: the launch writes F0 and the packed values straight into page-locked host arrays."""
    G = golden("cfg_" + name)
    prob, obj, eng = _engine(name)
    X, H = np.ascontiguousarray(G["x"]), np.ascontiguousarray(G["h"])
    X[1], H[1] = _bad_point(prob, state)
    batch = eng.batch(4)
    for count in (3, 2, 3):
        F0, vals, nonfinite = batch.sweep(X[:count], H[:count])
        F0p, valsp, nonfinitep = batch.sweep(X[:count], H[:count], persistent=True)
        assert F0p.shape == F0.shape and valsp.shape == vals.shape
        assert np.array_equal(F0p, F0, equal_nan=True) and np.array_equal(nonfinitep, nonfinite)
        assert nonfinite[1] != 0 and not nonfinite[0]
        for k in range(count):
            if not nonfinite[k]:
                assert np.array_equal(valsp[k], vals[k])
                assert np.array_equal(valsp[k], _gather(eng, eng.sweep_stacked(X[k], H[k])[1]))
    eng.close()


@pytest.mark.parametrize("layout", ["split", "dense"])
@pytest.mark.parametrize("name,state", [("goddard", 2), ("polar_tsto", 4)])
def test_validation_forms_give_the_bits_of_the_one_launch_form(name, state, layout, golden, monkeypatch):
    G = golden("cfg_" + name)
    X, H = np.ascontiguousarray(G["x"]), np.ascontiguousarray(G["h"])
    monkeypatch.setenv("OGPSX_SWEEP", "fused")
    prob, obj, eng = _engine(name)
    assert eng.sweep_mode == "fused"
    bad = _bad_point(prob, state)
    batch = eng.batch(3)
    want = [batch.sweep(X, H) + ([batch.dense(k) for k in range(3)],)]
    Xb, Hb = X.copy(), H.copy()
    Xb[1], Hb[1] = bad
    want.append(batch.sweep(Xb, Hb) + ([batch.dense(k) for k in range(3)],))
    want.append(batch.sweep(X, H) + ([batch.dense(k) for k in range(3)],))
    eng.close()
    monkeypatch.setenv("OGPSX_SWEEP", layout)
    prob, obj, eng = _engine(name)
    assert eng.sweep_mode == layout
    batch = eng.batch(3)
    for (P, Hs), (F0w, valsw, nfw, densew) in zip([(X, H), (Xb, Hb), (X, H)], want):
        F0, vals, nf = batch.sweep(P, Hs)
        assert np.array_equal(F0, F0w, equal_nan=True) and np.array_equal(nf, nfw)
        for k in range(3):
            assert np.array_equal(batch.dense(k), densew[k], equal_nan=True)
            if not nf[k]:
                assert np.array_equal(vals[k], valsw[k])
    eng.close()


def test_device_pointer_form_on_a_side_stream_without_host_synchronisation(golden):
    import torch
    name = "polar_tsto"
    G = golden("cfg_" + name)
    prob, obj, eng = _engine(name)
    batch = eng.batch(3)
    nnz = batch.nnz
    dev = torch.device("cuda", eng.device)
    side = torch.cuda.Stream(device=dev)
    order = [[0, 1, 2], [2, 0, 1]]
    with torch.cuda.stream(side):
        outs = []
        for perm in order:
            d_X = torch.from_numpy(np.ascontiguousarray(G["x"][perm])).to(dev)
            d_H = torch.from_numpy(np.ascontiguousarray(G["h"][perm])).to(dev)
            d_F = torch.full((3, eng.m), -1.0, dtype=torch.float64, device=dev)
            d_V = torch.full((3, nnz), -1.0, dtype=torch.float64, device=dev)
            outs.append((d_X, d_H, d_F, d_V))
        for d_X, d_H, d_F, d_V in outs:               # two batches back to back, nothing in between
            batch.sweep_dev(3, d_X.data_ptr(), d_H.data_ptr(), d_F.data_ptr(), d_V.data_ptr(), side.cuda_stream)
        d_E = torch.full((2, eng.m), -1.0, dtype=torch.float64, device=dev)
        batch.values_dev(2, outs[0][0].data_ptr(), d_E.data_ptr(), side.cuda_stream)
        # without packed values: the lanes' matrices are the result
        batch.sweep_dev(2, outs[0][0].data_ptr(), outs[0][1].data_ptr(), outs[0][2].data_ptr(), None, side.cuda_stream)
    side.synchronize()
    single = [eng.sweep_stacked(G["x"][k], G["h"][k]) for k in range(3)]
    for perm, (d_X, d_H, d_F, d_V) in zip(order, outs):
        F, V = d_F.cpu().numpy(), d_V.cpu().numpy()
        for lane, k in enumerate(perm):
            assert np.array_equal(F[lane], single[k][0])
            assert np.array_equal(V[lane], _gather(eng, single[k][1]))
    E = d_E.cpu().numpy()
    for lane, k in enumerate(order[0][:2]):
        assert np.array_equal(E[lane], single[k][0])
        assert np.array_equal(batch.dense(lane), single[k][1])
    assert np.array_equal(batch.dense(2), single[order[1][2]][1])      # lane 2 was not in the last batch
    eng.close()


def test_errors_leave_the_batch_usable(golden):
    name = "goddard"
    G = golden("cfg_" + name)
    prob, obj, eng = _engine(name)
    lib = _native.lib()
    out = C.c_void_p()
    assert lib.og_batch_create(eng._handle, 2, b"/nonexistent/libogk.batch.so", C.byref(out)) != 0
    assert "batch part" in lib.og_last_error().decode() and not out.value
    assert lib.og_batch_create(eng._handle, 0, None, C.byref(out)) != 0
    batch = eng.batch(2)
    X, H = np.ascontiguousarray(G["x"]), np.ascontiguousarray(G["h"])
    with pytest.raises(_native.NativeError, match="exceeds the batch's capacity 2"):
        batch.sweep(X, H)
    with pytest.raises(_native.NativeError, match="count must be at least 1"):
        batch.sweep(X[:0], H[:0])
    with pytest.raises(_native.NativeError, match="exceeds the batch's capacity 2"):
        batch.values(X)
    with pytest.raises(_native.NativeError, match="null argument"):
        batch.sweep_dev(2, 0, 0, 0)
    with pytest.raises(_native.NativeError, match="lane out of range"):
        batch.lane_dev(2)
    with pytest.raises(ValueError):
        batch.sweep(X[:2, :-1], H[:2, :-1])
    F0, vals, nonfinite = batch.sweep(X[:2], H[:2])
    for k in range(2):
        F1, JT1 = eng.sweep_stacked(X[k], H[k])
        assert np.array_equal(F0[k], F1) and np.array_equal(vals[k], _gather(eng, JT1))
    # lanes that cannot be allocated are an error of og_batch_create, and the handle goes on
    too_many = C.c_void_p()
    rc = lib.og_batch_create(eng._handle, 65535, None, C.byref(too_many))
    if rc == 0:                                       # (a device with room for 65535 lanes of this problem)
        lib.og_batch_destroy(too_many)
    else:
        assert "og_batch_create" in lib.og_last_error().decode() and not too_many.value
    assert np.array_equal(batch.sweep(X[:2], H[:2])[1], vals)
    # a batch does not outlive its handle
    handle = C.c_void_p(batch._handle.value)
    eng.close()
    assert not batch._handle.value
    assert lib.og_batch_fd_sweep(handle, 2, _native.dptr(X), _native.dptr(H), _native.dptr(F0), _native.dptr(vals),
                                 None) != 0
    assert "destroyed" in lib.og_last_error().decode()


@pytest.mark.parametrize("name", ["goddard", "polar_tsto"])
def test_problem_evaluate_batch_equals_the_engine_point_by_point(name, golden):
    from opengoddard_amd.engine import HipEngine
    G = golden("cfg_" + name)
    prob, obj = problems.build(name)
    X = np.ascontiguousarray(G["x"])
    p_before = prob.p.copy()
    res = prob.evaluate_batch(obj, X, jacobian=True)
    plain = prob.evaluate_batch(obj, X[:2])
    assert np.array_equal(prob.p, p_before)
    assert isinstance(prob._engine, HipEngine)
    eng = HipEngine(*problems.build(name))            # the single-point path on a handle of its own
    lb, ub = _bounds(prob)
    indptr, rows = res.pattern
    assert np.array_equal(indptr, eng.pattern()[0]) and np.array_equal(rows, eng.pattern()[1])
    for k in range(3):
        cost, ceq, cineq = eng.values(X[k])
        (grad, jeq, jineq), h = eng.jacobians(X[k], lb, ub)
        assert np.array_equal(h, _native.fd_step(X[k], lb, ub))
        assert res.cost[k] == cost and np.array_equal(res.equality[k], ceq)
        assert np.array_equal(res.inequality[k], cineq)
        assert res.violation[k] == np.sum(np.abs(ceq)) + np.sum(np.maximum(-cineq, 0.0))
        assert np.array_equal(res.steps[k], h)
        assert np.array_equal(res.gradient[k], grad)
        JT = np.vstack([grad[None, :], jeq, jineq]).T
        assert np.array_equal(res.values[k], _gather(eng, JT))
        if k < 2:
            assert plain.cost[k] == cost and np.array_equal(plain.equality[k], ceq)
            assert np.array_equal(plain.inequality[k], cineq) and plain.violation[k] == res.violation[k]
    assert plain.gradient is None and plain.values is None
    eng.close()
    prob._engine.close()


@pytest.mark.parametrize("name,state", [("goddard", 2), ("polar_tsto", 4)])
def test_single_point_results_do_not_change_with_a_batch_open(name, state, golden):
    """Single sweeps into a registered device buffer, interleaved with batched sweeps on the same handle, against
    the same single sweeps on a fresh handle."""
    import torch
    G = golden("cfg_" + name)
    X, H = np.ascontiguousarray(G["x"]), np.ascontiguousarray(G["h"])
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream().cuda_stream

    def run(with_batch):
        prob, obj, eng = _engine(name)
        bad = _bad_point(prob, state)
        points = [(X[0], H[0]), bad, (X[1], H[1]), (X[2], H[2])]
        d_JT = torch.empty((eng.n, eng.m), dtype=torch.float64, device=dev)
        d_F = torch.empty(eng.m, dtype=torch.float64, device=dev)
        eng.register_jt_dev(d_JT.data_ptr(), 0, eng.n, stream)
        batch = eng.batch(3) if with_batch else None
        results = []
        for i, (x, h) in enumerate(points):
            if batch is not None:
                Pb, Hb = X.copy(), H.copy()
                if i % 2 == 0:
                    Pb[i % 3], Hb[i % 3] = bad
                batch.sweep(Pb, Hb)
            d_x, d_h = torch.from_numpy(x).to(dev), torch.from_numpy(h).to(dev)
            eng.sweep_dev(d_x.data_ptr(), d_h.data_ptr(), 0, eng.n, d_JT.data_ptr(), d_F.data_ptr(), stream)
            torch.cuda.synchronize()
            results.append((d_F.cpu().numpy().copy(), d_JT.cpu().numpy().copy(), eng.eval_stacked(x)))
            if batch is not None:
                batch.values(X)
        eng.unregister_jt_dev(d_JT.data_ptr())
        eng.close()
        return results

    for (Fa, JTa, Ea), (Fb, JTb, Eb) in zip(run(True), run(False)):
        assert np.array_equal(Fa, Fb, equal_nan=True)
        assert np.array_equal(JTa, JTb, equal_nan=True)
        assert np.array_equal(Ea, Eb, equal_nan=True)


@pytest.mark.parametrize("layout", ["fused", "split", "dense"])
def test_a_lanes_non_finite_count_is_its_own_when_the_lane_count_varies(layout, golden, monkeypatch):
    """[3 points, lane 1 bad] -> [1 point] -> [3 good points], through sweeps and through evaluations: the count of
    non-finite rows is per lane - a launch that runs fewer lanes neither disturbs the counts of the others nor leaves
    anything behind that a later launch would add to."""
    name, state = "goddard", 2
    monkeypatch.setenv("OGPSX_SWEEP", layout)
    G = golden("cfg_" + name)
    prob, obj, eng = _engine(name)
    assert eng.sweep_mode == layout
    X, H = np.ascontiguousarray(G["x"]), np.ascontiguousarray(G["h"])
    Xb, Hb = X.copy(), H.copy()
    Xb[1], Hb[1] = _bad_point(prob, state)
    bad_rows = int(np.sum(~np.isfinite(eng.eval_stacked(Xb[1]))))
    assert bad_rows > 0
    single = [eng.sweep_stacked(X[k], H[k]) for k in range(3)]
    batch = eng.batch(3)

    def counts():
        return [batch.lane_dev(k)[1] for k in range(3)]

    for _ in range(2):                                # (twice: whatever alternates has come round)
        F0, vals, nonfinite = batch.sweep(Xb, Hb)
        assert nonfinite.tolist() == [0, bad_rows, 0] and counts() == [0, bad_rows, 0]
        F0, vals, nonfinite = batch.sweep(X[:1], H[:1])
        assert nonfinite.tolist() == [0]
        assert counts() == [0, bad_rows, 0], "lane 1's most recent point is still the bad one"
        F0, vals, nonfinite = batch.sweep(X, H)
        assert nonfinite.tolist() == [0, 0, 0] and counts() == [0, 0, 0]
        for k in range(3):
            assert np.array_equal(F0[k], single[k][0]) and np.array_equal(batch.dense(k), single[k][1])
            assert np.array_equal(vals[k], _gather(eng, single[k][1]))
        # the same through evaluations
        batch.values(Xb)
        assert counts() == [0, bad_rows, 0]
        batch.values(X[:1])
        assert counts() == [0, bad_rows, 0]
        F = batch.values(X)
        assert counts() == [0, 0, 0]
        assert all(np.array_equal(F[k], single[k][0]) for k in range(3))
        # a sweep of all lanes, an evaluation of one: lanes 1 and 2 keep the sweep's counts
        batch.sweep(Xb, Hb)
        batch.values(X[:1])
        assert counts() == [0, bad_rows, 0]
    eng.close()


@pytest.mark.parametrize("name,state", [("goddard", 2), ("polar_tsto", 4)])
def test_batched_sweep_replays_from_a_captured_graph_between_eager_calls(name, state, golden):
    """A batched sweep captured into a hipGraph (the launch that binds the arrays to the lanes is captured with it)
    and replayed at new points written into the same device arrays, interleaved with eager calls on OTHER arrays: every
    call and every replay works on its own arrays, through non-finite points too."""
    import torch
    G = golden("cfg_" + name)
    prob, obj, eng = _engine(name)
    assert eng.sweep_mode == "fused"
    batch = eng.batch(3)
    nnz, n, m = batch.nnz, eng.n, eng.m
    dev = torch.device("cuda", 0)
    lb, ub = _bounds(prob)
    bad = _bad_point(prob, state)
    rng = np.random.default_rng(5)

    def arrays():
        return (torch.zeros((3, n), dtype=torch.float64, device=dev), torch.zeros((3, n), dtype=torch.float64, device=dev),
                torch.full((3, m), -1.0, dtype=torch.float64, device=dev),
                torch.full((3, nnz), -1.0, dtype=torch.float64, device=dev))

    def points(with_bad):
        P = np.stack([np.clip(G["x"][k] + 1e-3 * rng.standard_normal(n), lb, ub) for k in range(3)])
        Hs = np.stack([_native.fd_step(p, lb, ub) for p in P])
        if with_bad:
            P[2], Hs[2] = bad
        return P, Hs

    def load(arr, P, Hs):
        arr[0].copy_(torch.from_numpy(P))
        arr[1].copy_(torch.from_numpy(Hs))

    def check(arr, P, Hs, what):
        F, V = arr[2].cpu().numpy(), arr[3].cpu().numpy()
        for k in range(3):
            F1, JT1 = eng.sweep_stacked(P[k], Hs[k])
            assert np.array_equal(F[k], F1, equal_nan=True), "%s: F of lane %d" % (what, k)
            if np.isfinite(F1).all():
                assert np.array_equal(V[k], _gather(eng, JT1)), "%s: values of lane %d" % (what, k)
            assert np.array_equal(batch.dense(k), JT1, equal_nan=True), "%s: matrix of lane %d" % (what, k)

    side = torch.cuda.Stream()
    A, B = arrays(), arrays()

    def call(arr, stream):
        batch.sweep_dev(3, arr[0].data_ptr(), arr[1].data_ptr(), arr[2].data_ptr(), arr[3].data_ptr(), stream)

    PA, HA = points(False)
    with torch.cuda.stream(side):
        load(A, PA, HA)
        call(A, side.cuda_stream)                     # warm
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        call(A, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    for step, with_bad in enumerate((False, True, False, True, False)):
        PB, HB = points(step == 2)
        with torch.cuda.stream(side):
            load(B, PB, HB)
            call(B, side.cuda_stream)                 # eager, on B
        torch.cuda.synchronize()
        check(B, PB, HB, "eager call before replay %d" % step)
        PA, HA = points(with_bad)
        load(A, PA, HA)
        F_B = B[2].clone()
        torch.cuda.synchronize()
        graph.replay()                                # on A
        torch.cuda.synchronize()
        check(A, PA, HA, "replay %d" % step)
        assert torch.equal(B[2], F_B) or step == 2, "the replay wrote into the eager call's arrays"
        with torch.cuda.stream(side):
            call(B, side.cuda_stream)                 # eager on B again, same pointers as before the replay
        torch.cuda.synchronize()
        check(B, PB, HB, "eager call after replay %d" % step)
    eng.close()


def test_the_batch_part_is_built_when_a_batch_is_first_asked_for():
    """A problem shape nothing has compiled ahead: constructing the engine builds the module's own parts and not the
    batch part; ``HipEngine.batch`` builds it."""
    import os
    from opengoddard_amd import build
    from opengoddard_amd.engine import HipEngine
    prob, obj = problems.build("brachistochrone", nodes=[13])
    eng = HipEngine(prob, obj)
    part = build.batch_part_path(build.module_path(build.module_digest(eng.header)))
    assert part not in [build.part_path(eng.module_path, i) for i in range(len(build.MODULE_PARTS))]
    existed = os.path.exists(part)                    # (a second run of the suite in the same tree finds it cached)
    batch = eng.batch(2)
    assert os.path.exists(part) and batch.part_path == part
    if not existed:
        assert os.path.getmtime(part) >= os.path.getmtime(eng.module_path)
    lb, ub = _bounds(prob)
    x = np.clip(prob.p, lb, ub)
    h = _native.fd_step(x, lb, ub)
    F0, vals, nonfinite = batch.sweep(np.stack([x, x]), np.stack([h, h]))
    F1, JT1 = eng.sweep_stacked(x, h)
    assert np.array_equal(F0[1], F1) and np.array_equal(vals[0], _gather(eng, JT1)) and not nonfinite.any()
    eng.close()


def test_solve_releases_the_lanes_of_an_earlier_evaluate_batch(golden, capsys):
    prob, obj = problems.build("brachistochrone")
    prob.evaluate_batch(obj, np.ascontiguousarray(golden("cfg_brachistochrone")["x"]))
    batch, engine = prob._batch, prob._engine
    assert batch._handle.value and engine._handle.value
    prob.maxIterator = 1
    prob.solve(obj, maxiter=2)
    assert not batch._handle.value and not engine._handle.value, "the screening engine and its lanes outlived solve()"
    assert prob._engine is not engine
    res = prob.evaluate_batch(obj, np.ascontiguousarray(golden("cfg_brachistochrone")["x"]))   # reuses the solve's engine
    assert prob._batch.engine is prob._engine and len(res) == 3
    prob._engine.close()
