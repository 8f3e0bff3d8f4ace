"""Exact Jacobians of a batch of points on the GPU (``og_jacobian_exact_batch*``, ``BatchSweep.exact``,
``Problem.evaluate_batch(jacobian="exact")``).  Comparisons are BITWISE against the single-point exact path of the same
build (``HipEngine.exact_stacked``), directly against the CPU twin where tests/test_exact_jacobian.py runs it, and - at
the baseline sizes - against the complex-step differentiation of ``oracle/exact_jac.py`` within the bound the
single-point kernel is held to."""
import ctypes as C
import os

import numpy as np
import pytest

from opengoddard_amd import _native, build, problems
from test_exact_jacobian import SMALL, _points
from test_gpu_batch import _bad_point, _bounds, _engine, _gather, _good_point

pytestmark = pytest.mark.gpu

TWIN_NAMES = SMALL + ["polar_tsto"]         # where tests/test_exact_jacobian.py pins the single-point kernel to the twin


@pytest.mark.parametrize("name", problems.NAMES)
def test_batched_exact_jacobian_equals_the_single_point_path_and_the_twin(name, golden):
    from oracle import twin
    G = golden("cfg_" + name)
    prob, obj, eng = _engine(name)
    X = np.ascontiguousarray(G["x"])
    assert X.shape[0] == 3
    batch = eng.batch(3)
    F0, vals, nonfinite = batch.exact(X)
    assert not nonfinite.any()
    indptr, rows = batch.pattern
    assert F0.shape == (3, eng.m) and vals.shape == (3, indptr[-1])
    tw = twin.Twin(prob, obj, program=eng.program, header=eng.header) if name in TWIN_NAMES else None
    for k in range(3):
        F1, JT1 = eng.exact_stacked(X[k])
        assert np.array_equal(F0[k], F1), "F differs in lane %d" % k
        assert np.array_equal(vals[k], _gather(eng, JT1)), "packed non-zeros differ in lane %d" % k
        dense = batch.dense(k)
        assert np.array_equal(dense, JT1), "dense matrix differs in lane %d" % k
        if tw is not None:                              # directly, not by transitivity
            F0c, JTc = tw.exact(X[k])
            assert np.array_equal(F0[k], F0c) and np.array_equal(dense, JTc), "lane %d against the twin" % k
            assert np.array_equal(vals[k], _gather(eng, JTc))
    eng.close()


@pytest.mark.parametrize("name,count", [("polar_tsto", 160), ("low_thrust", 120), ("launch4", 72)])
def test_batched_exact_jacobian_against_complex_step_at_baseline_sizes(name, count):
    """The generic point of tests/test_exact_jacobian.py and two seeded neighbours of it as one batch, the columns
    chosen as there (a spread over every variable block plus all final-time columns, the heavy ones), every lane
    against ``oracle/exact_jac.py`` within 1e-12 of the row scale - the single-point kernel's own bound."""
    from oracle import exact_jac
    prob, obj, eng = _engine(name)
    lb, ub = _bounds(prob)
    x = _points(prob, lb, ub)[1]
    rng = np.random.default_rng(11)
    X = np.stack([x] + [np.clip(x * (1.0 + 1e-3 * rng.standard_normal(x.size)) + 1e-4 * rng.standard_normal(x.size),
                                lb, ub) for _ in range(2)])
    n, S = eng.n, len(prob.nodes)
    cols = np.unique(np.r_[np.linspace(0, n - S - 1, count).astype(int), np.arange(n - S, n)]).astype(np.int32)
    batch = eng.batch(3)
    F0, vals, nonfinite = batch.exact(X)
    assert not nonfinite.any()
    indptr, rows = batch.pattern
    at = np.repeat(np.arange(n), np.diff(indptr))
    for k in range(3):
        assert np.array_equal(F0[k], eng.eval_stacked(X[k]))
        JE = batch.dense(k)
        assert np.all(np.isfinite(JE))
        JC = exact_jac.jacobian(eng.program, prob, X[k], list(cols))
        scale = np.maximum(1.0, np.abs(JC).max(axis=0))[None, :]
        worst = np.max(np.abs(JE[cols] - JC) / scale)
        print("%s lane %d: worst scaled difference to complex step %.3g" % (name, k, worst))
        assert worst <= 1e-12
        # the packed values are the matrix's pattern entries, and there is nothing outside the pattern
        assert np.array_equal(vals[k], JE[at, rows])
        mask = np.zeros(JE.shape, dtype=bool)
        mask[at, rows] = True
        assert not np.any(JE[~mask])
    eng.close()


@pytest.mark.parametrize("name,state", [("polar_tsto", 4), ("brachistochrone", None)])
def test_an_exact_lane_does_not_depend_on_its_position_or_its_companions(name, state, golden):
    G = golden("cfg_" + name)
    prob, obj, eng = _engine(name)
    cap = 4
    batch = eng.batch(cap)
    x = G["x"][0]
    if state is None:
        bad = G["x"][1].copy()
        bad[2] = np.nan
    else:
        bad = _bad_point(prob, state)[0]
    assert not np.isfinite(eng.eval_stacked(bad)).all()
    companions = [G["x"][1], bad, G["x"][2]]
    F1, JT1 = eng.exact_stacked(x)
    packed1 = _gather(eng, JT1)
    turn = 0
    for count in (1, 2, cap):
        for lane in (0, 1, cap - 1):
            if lane >= count:
                continue
            P, is_bad = np.empty((count, eng.n)), np.zeros(count, dtype=bool)
            for k in range(count):
                if k == lane:
                    P[k] = x
                else:
                    P[k] = companions[turn % 3]
                    is_bad[k] = turn % 3 == 1
                    turn += 1
            F0, vals, nonfinite = batch.exact(P)
            what = "count %d, lane %d" % (count, lane)
            assert np.array_equal(F0[lane], F1), what
            assert np.array_equal(vals[lane], packed1), what
            assert np.array_equal(batch.dense(lane), JT1), what
            assert np.array_equal(nonfinite != 0, is_bad), what
    eng.close()


@pytest.mark.parametrize("name,state", [("goddard", 2), ("polar_tsto", 4)])
def test_exact_calls_and_fd_sweeps_share_a_lanes_history(name, state, golden):
    """FD sweep with a bad point in lane 1 (NaN fill) -> exact at good points -> FD sweep at good points -> values:
    after each step every lane holds what a single-point handle holds after the same sequence, the exact call cleans
    the NaN fill the sweep left, and nothing non-finite lingers.  Then: an exact call on lanes 0-1 leaves lane 2 alone."""
    from opengoddard_amd.engine import HipEngine
    G = golden("cfg_" + name)
    prob, obj, eng = _engine(name)
    lb, ub = _bounds(prob)
    good, bad = _good_point(prob), _bad_point(prob, state)
    X = np.ascontiguousarray(G["x"])
    H = np.stack([_native.fd_step(x, lb, ub) for x in X])
    batch = eng.batch(3)
    refs = [HipEngine(*problems.build(name)) for _ in range(3)]

    def lanes_equal(F0, vals, results, packed=True):
        for k, (Fr, JTr) in enumerate(results):
            assert np.array_equal(F0[k], Fr, equal_nan=True), "lane %d" % k
            dense = batch.dense(k)
            assert np.array_equal(np.isnan(dense), np.isnan(JTr)), "lane %d" % k
            assert np.array_equal(dense, JTr, equal_nan=True), "lane %d" % k
            if packed and np.isfinite(Fr).all():
                assert np.array_equal(vals[k], _gather(refs[k], JTr)), "lane %d" % k

    # 1. FD sweep, lane 1 at the bad point
    P1, H1 = np.stack([good[0], bad[0], good[0]]), np.stack([good[1], bad[1], good[1]])
    F0, vals, nonfinite = batch.sweep(P1, H1)
    assert np.array_equal(nonfinite != 0, [False, True, False])
    assert np.isnan(batch.dense(1)).any()
    lanes_equal(F0, vals, [refs[k].sweep_stacked(P1[k], H1[k]) for k in range(3)])
    # 2. exact, all lanes at good points: lane 1's NaN fill is gone
    F0, vals, nonfinite = batch.exact(X)
    assert not nonfinite.any()
    lanes_equal(F0, vals, [refs[k].exact_stacked(X[k]) for k in range(3)])
    assert all(np.isfinite(batch.dense(k)).all() for k in range(3))
    # 3. FD sweep at good points, 4. values
    F0, vals, nonfinite = batch.sweep(X, H)
    assert not nonfinite.any()
    lanes_equal(F0, vals, [refs[k].sweep_stacked(X[k], H[k]) for k in range(3)])
    F = batch.values(X)
    for k in range(3):
        assert np.array_equal(F[k], refs[k].eval_stacked(X[k]))
        assert np.isfinite(batch.dense(k)).all()
    # an exact call at a bad point, then a good one: the single-point path's bits at both
    Pb = X.copy()
    Pb[0] = bad[0]
    F0, vals, nonfinite = batch.exact(Pb)
    assert np.array_equal(nonfinite != 0, [True, False, False])
    results = [refs[k].exact_stacked(Pb[k]) for k in range(3)]
    assert nonfinite[0] == np.sum(~np.isfinite(results[0][0])) == batch.lane_dev(0)[1]
    lanes_equal(F0, vals, results)
    F0, vals, nonfinite = batch.exact(X)
    assert not nonfinite.any()
    lanes_equal(F0, vals, [refs[k].exact_stacked(X[k]) for k in range(3)])
    # lanes 0-1 only: lane 2 keeps its matrix (here: an FD sweep's NaN fill) and its count
    P2, H2 = np.stack([good[0], good[0], bad[0]]), np.stack([good[1], good[1], bad[1]])
    _, _, nonfinite = batch.sweep(P2, H2)
    lane2, count2 = batch.dense(2), int(nonfinite[2])
    assert count2 > 0 and np.isnan(lane2).any()
    F0, vals, nonfinite = batch.exact(X[:2])
    assert not nonfinite.any() and np.array_equal(vals[1], _gather(eng, eng.exact_stacked(X[1])[1]))
    assert np.array_equal(batch.dense(2), lane2, equal_nan=True) and batch.lane_dev(2)[1] == count2
    F0, vals, nonfinite = batch.exact(X)
    assert not nonfinite.any() and all(np.isfinite(batch.dense(k)).all() for k in range(3))
    assert np.array_equal(batch.dense(2), eng.exact_stacked(X[2])[1])
    for ref in refs:
        ref.close()
    eng.close()


@pytest.mark.parametrize("name", ["goddard", "polar_tsto"])
def test_persistent_arrays_device_pointers_and_a_captured_graph_receive_the_same_bits(name, golden):
    import torch
    G = golden("cfg_" + name)
    prob, obj, eng = _engine(name)
    lb, ub = _bounds(prob)
    X = np.ascontiguousarray(G["x"])
    batch = eng.batch(4)
    nnz, n, m = batch.nnz, eng.n, eng.m
    single = [eng.exact_stacked(X[k]) for k in range(3)]
    for count in (3, 2, 3):
        F0, vals, nonfinite = batch.exact(X[:count])
        F0p, valsp, nonfinitep = batch.exact(X[:count], persistent=True)
        assert F0p.shape == F0.shape and valsp.shape == vals.shape
        assert np.array_equal(F0p, F0) and np.array_equal(valsp, vals) and np.array_equal(nonfinitep, nonfinite)
        for k in range(count):
            assert np.array_equal(F0p[k], single[k][0]) and np.array_equal(valsp[k], _gather(eng, single[k][1]))

    # device pointers on a side stream: two calls back to back on different arrays, one without packed values
    dev = torch.device("cuda", eng.device)
    side = torch.cuda.Stream(device=dev)
    order = [[0, 1, 2], [2, 0, 1]]
    with torch.cuda.stream(side):
        outs = []
        for perm in order:
            outs.append((torch.from_numpy(np.ascontiguousarray(X[perm])).to(dev),
                         torch.full((3, m), -1.0, dtype=torch.float64, device=dev),
                         torch.full((3, nnz), -1.0, dtype=torch.float64, device=dev)))
        for d_X, d_F, d_V in outs:
            batch.exact_dev(3, d_X.data_ptr(), d_F.data_ptr(), d_V.data_ptr(), side.cuda_stream)
        d_F2 = torch.full((2, m), -1.0, dtype=torch.float64, device=dev)
        batch.exact_dev(2, outs[0][0].data_ptr(), d_F2.data_ptr(), None, side.cuda_stream)
    side.synchronize()
    for perm, (d_X, d_F, d_V) in zip(order, outs):
        F, V = d_F.cpu().numpy(), d_V.cpu().numpy()
        for lane, k in enumerate(perm):
            assert np.array_equal(F[lane], single[k][0]) and np.array_equal(V[lane], _gather(eng, single[k][1]))
    F2 = d_F2.cpu().numpy()
    for lane, k in enumerate(order[0][:2]):
        assert np.array_equal(F2[lane], single[k][0]) and np.array_equal(batch.dense(lane), single[k][1])
    assert np.array_equal(batch.dense(2), single[order[1][2]][1])      # lane 2 was not in the last call

    # a captured graph of the call (three launches in a line), replayed at new points between eager calls on others
    rng = np.random.default_rng(5)

    def arrays():
        return (torch.zeros((3, n), dtype=torch.float64, device=dev),
                torch.full((3, m), -1.0, dtype=torch.float64, device=dev),
                torch.full((3, nnz), -1.0, dtype=torch.float64, device=dev))

    def points():
        return np.stack([np.clip(X[k] + 1e-3 * rng.standard_normal(n), lb, ub) for k in range(3)])

    def call(arr, stream):
        batch.exact_dev(3, arr[0].data_ptr(), arr[1].data_ptr(), arr[2].data_ptr(), stream)

    def check(arr, P, what):
        F, V = arr[1].cpu().numpy(), arr[2].cpu().numpy()
        for k in range(3):
            F1, JT1 = eng.exact_stacked(P[k])
            assert np.array_equal(F[k], F1), "%s: F of lane %d" % (what, k)
            assert np.array_equal(V[k], _gather(eng, JT1)), "%s: values of lane %d" % (what, k)
            assert np.array_equal(batch.dense(k), JT1), "%s: matrix of lane %d" % (what, k)

    A, B = arrays(), arrays()
    PA = points()
    with torch.cuda.stream(side):
        A[0].copy_(torch.from_numpy(PA))
        call(A, side.cuda_stream)                     # warm
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        call(A, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    for step in range(2):
        PB = points()
        with torch.cuda.stream(side):
            B[0].copy_(torch.from_numpy(PB))
            call(B, side.cuda_stream)                 # eager, on B
        torch.cuda.synchronize()
        check(B, PB, "eager call before replay %d" % step)
        PA = points()
        A[0].copy_(torch.from_numpy(PA))
        F_B, V_B = B[1].clone(), B[2].clone()
        torch.cuda.synchronize()
        graph.replay()                                # on A
        torch.cuda.synchronize()
        check(A, PA, "replay %d" % step)
        assert torch.equal(B[1], F_B) and torch.equal(B[2], V_B), "the replay wrote into the eager call's arrays"
    eng.close()


@pytest.mark.parametrize("name,state", [("goddard", 2), ("polar_tsto", 4)])
def test_the_dense_validation_form_gives_the_bits_of_the_default_form(name, state, golden, monkeypatch):
    G = golden("cfg_" + name)
    X = np.ascontiguousarray(G["x"])
    monkeypatch.setenv("OGPSX_SWEEP", "fused")
    prob, obj, eng = _engine(name)
    lb, ub = _bounds(prob)
    H = np.stack([_native.fd_step(x, lb, ub) for x in X])
    Xb, Hb = X.copy(), H.copy()
    Xb[1], Hb[1] = _bad_point(prob, state)

    def run(engine):
        batch = engine.batch(3)
        out = [batch.exact(X) + ([batch.dense(k) for k in range(3)],)]
        _, _, nonfinite = batch.sweep(Xb, Hb)             # leaves a NaN fill in lane 1 for the next call to clean
        assert nonfinite[1] != 0 and np.isnan(batch.dense(1)).any()
        out.append(batch.exact(X[::-1].copy()) + ([batch.dense(k) for k in range(3)],))
        return out

    want = run(eng)
    eng.close()
    monkeypatch.setenv("OGPSX_SWEEP", "dense")
    prob, obj, eng = _engine(name)
    assert eng.sweep_mode == "dense"
    got = run(eng)
    for (F0, vals, nf, dense), (F0w, valsw, nfw, densew) in zip(got, want):
        assert np.array_equal(F0, F0w) and np.array_equal(vals, valsw) and np.array_equal(nf, nfw) and not nf.any()
        for k in range(3):
            assert np.array_equal(dense[k], densew[k])
    eng.close()


def test_the_exact_batch_part_is_built_by_the_first_exact_call_and_errors_leave_the_batch_usable(golden):
    """A problem shape nothing has compiled ahead: neither the engine, nor ``HipEngine.batch``, nor an FD sweep of the
    batch builds ``<module>.batchx.so``; ``BatchSweep.exact`` does.  The C entry points before the part is loaded, with a
    part that is not there or is another module's, beyond the capacity, and after the handle is gone."""
    import torch
    from opengoddard_amd import codegen
    from opengoddard_amd.engine import HipEngine
    prob, obj = problems.build("brachistochrone", nodes=[11])
    eng = HipEngine(prob, obj)
    part = build.batch_exact_part_path(build.module_path(build.module_digest(eng.header)))
    existed = os.path.exists(part)                    # (a second run of the suite in the same tree finds it cached)
    batch = eng.batch(2)
    lb, ub = _bounds(prob)
    x = np.clip(prob.p, lb, ub)
    h = _native.fd_step(x, lb, ub)
    X2 = np.stack([x, np.clip(x * 1.001, lb, ub)])
    batch.sweep(X2, np.stack([h, _native.fd_step(X2[1], lb, ub)]))
    assert batch.exact_part_path is None
    if not existed:
        assert not os.path.exists(part), "the exact batch part was built before an exact Jacobian was asked for"
    # before the load: error 4 and a text that says what is missing
    lib = _native.lib()
    dev = torch.device("cuda", eng.device)
    d_X = torch.from_numpy(X2).to(dev)
    d_F = torch.zeros((2, eng.m), dtype=torch.float64, device=dev)
    stream = torch.cuda.current_stream().cuda_stream
    assert lib.og_jacobian_exact_batch_dev(batch._handle, 2, d_X.data_ptr(), d_F.data_ptr(), None, stream) == 4
    text = lib.og_last_error().decode()
    assert "og_jacobian_exact_batch_dev" in text and "exact batch part is not loaded" in text
    assert lib.og_jacobian_exact_batch_load(batch._handle, None) == 4
    assert lib.og_jacobian_exact_batch_load(batch._handle, b"/nonexistent/libogk.batchx.so") == 4
    assert "og_jacobian_exact_batch_load" in lib.og_last_error().decode()
    other_prob, other_obj = problems.build("goddard")
    other = build.build_batch_exact_part(codegen.emit_header(codegen.trace_problem(other_prob, other_obj)))
    assert lib.og_jacobian_exact_batch_load(batch._handle, other.encode()) == 5
    assert "does not belong" in lib.og_last_error().decode()
    # the first exact call builds and loads it
    F0, vals, nonfinite = batch.exact(X2)
    assert os.path.exists(part) and batch.exact_part_path == part
    assert part != batch.part_path and part not in [build.part_path(eng.module_path, i)
                                                    for i in range(len(build.MODULE_PARTS))]
    assert lib.og_jacobian_exact_batch_load(batch._handle, None) == 0           # loaded: a no-op, no path needed
    for k in range(2):
        F1, JT1 = eng.exact_stacked(X2[k])
        assert np.array_equal(F0[k], F1) and np.array_equal(vals[k], _gather(eng, JT1)) and not nonfinite[k]
    # a second batch of the handle finds the part loaded
    second = eng.batch(1)
    assert lib.og_jacobian_exact_batch_dev(second._handle, 1, d_X.data_ptr(), d_F.data_ptr(), None, stream) == 0
    torch.cuda.synchronize()
    assert np.array_equal(d_F.cpu().numpy()[0], F0[0]) and np.array_equal(second.dense(0), batch.dense(0))
    # errors
    X3 = np.stack([x, x, x])
    with pytest.raises(_native.NativeError, match="exceeds the batch's capacity 2"):
        batch.exact(X3)
    with pytest.raises(_native.NativeError, match="count must be at least 1"):
        batch.exact(X3[:0])
    with pytest.raises(_native.NativeError, match="null argument"):
        batch.exact_dev(2, 0, 0)
    with pytest.raises(ValueError):
        batch.exact(X2[:, :-1])
    assert np.array_equal(batch.exact(X2)[1], vals)
    handle = C.c_void_p(batch._handle.value)
    eng.close()
    assert not batch._handle.value
    nf = np.zeros(2, dtype=np.int32)
    assert lib.og_jacobian_exact_batch(handle, 2, _native.dptr(X2), _native.dptr(F0), _native.dptr(vals),
                                       nf.ctypes.data_as(C.POINTER(C.c_int32))) != 0
    assert "destroyed" in lib.og_last_error().decode()
    assert lib.og_jacobian_exact_batch_load(handle, None) != 0 and "destroyed" in lib.og_last_error().decode()


@pytest.mark.parametrize("name", ["goddard", "polar_tsto"])
def test_problem_evaluate_batch_with_exact_jacobians_equals_the_engine_point_by_point(name, golden):
    from opengoddard_amd.engine import HipEngine
    G = golden("cfg_" + name)
    prob, obj = problems.build(name)
    X = np.ascontiguousarray(G["x"])
    p_before = prob.p.copy()
    res = prob.evaluate_batch(obj, X, jacobian="exact")
    assert np.array_equal(prob.p, p_before)
    assert isinstance(prob._engine, HipEngine)
    assert res.jacobian == "exact" and res.steps is None
    eng = HipEngine(*problems.build(name))            # the single-point path on a handle of its own
    indptr, rows = res.pattern
    assert np.array_equal(indptr, eng.pattern()[0]) and np.array_equal(rows, eng.pattern()[1])
    for k in range(3):
        cost, ceq, cineq = eng.values(X[k])
        F1, JT1 = eng.exact_stacked(X[k])
        assert res.cost[k] == cost == F1[0] and np.array_equal(res.equality[k], ceq)
        assert np.array_equal(res.inequality[k], cineq)
        assert res.violation[k] == np.sum(np.abs(ceq)) + np.sum(np.maximum(-cineq, 0.0))
        assert np.array_equal(res.gradient[k], JT1[:, 0])
        assert np.array_equal(res.values[k], _gather(eng, JT1))
    # forward differences are still what jacobian=True means on this Problem
    lb, ub = _bounds(prob)
    fd = prob.evaluate_batch(obj, X, jacobian=True)
    assert fd.jacobian == "fd"
    for k in range(3):
        (grad, jeq, jineq), h = eng.jacobians(X[k], lb, ub)
        assert np.array_equal(fd.steps[k], h) and np.array_equal(fd.gradient[k], grad)
        assert np.array_equal(fd.values[k], _gather(eng, np.vstack([grad[None, :], jeq, jineq]).T))
    eng.close()
    prob._engine.close()
