"""Run-time parameters on the GPU (``og_set_parameters*``, ``og_parameters_batch*``, ``HipEngine.set_parameters``,
``BatchSweep.set_parameters``, ``Problem.set_parameter`` / ``evaluate_batch(parameters=...)`` /
``parameter_sensitivity``).  Every comparison is BITWISE against the CPU twin of the same generated header with the
same table (``oracle/twin.py``), or against the single-point path of a second engine that the first test pins to the
twin.  The problems are those of tests/parameter_cases.py; their modules are compiled by ``__graft_entry__.build``."""
import numpy as np
import pytest

import parameter_cases as pc
from opengoddard_amd import _native, build
from oracle import np_path, twin

pytestmark = pytest.mark.gpu


def _make(key, **kw):
    return pc.p2(**kw) if key == "P2" else pc.goddard(int(key[1:]), **kw)


def _thetas(key):
    return pc.P2_THETA if key == "P2" else pc.G_THETA


def _engine(key, **kw):
    from opengoddard_amd.engine import HipEngine
    prob, obj = _make(key, **kw)
    return prob, obj, HipEngine(prob, obj, program=pc.trace(prob, obj))


class Reference:
    """The twin of an engine's header, asked at a parameter vector."""

    def __init__(self, prob, obj, eng):
        self.tw = twin.Twin(prob, obj, program=pc.trace(prob, obj), header=eng.header)
        self.off = self.tw.program.par_off

    def at(self, theta):
        self.tw._cv[self.off:] = theta
        return self.tw


def _point(prob, seed=0):
    lb, ub = np_path.bounds_arrays(prob)
    x = pc.point(prob, seed)
    return x, _native.fd_step(x, lb, ub)


def _gather(eng, JT):
    indptr, rows = eng.pattern()
    return JT[np.repeat(np.arange(eng.n), np.diff(indptr)), rows]


def _nan_theta(key):
    """theta0 with the parameter of a boundary row NaN (P2: ``b``; Goddard: ``Mf``)."""
    theta = _thetas(key)[0].copy()
    theta[1 if key == "P2" else 3] = np.nan
    return theta


# ------------------------------------------------------------------------------------------------ 1. single point
@pytest.mark.parametrize("layout", ["fused", "split", "dense"])
@pytest.mark.parametrize("key", ["P2", "G17"])
def test_a_handle_follows_its_parameters(key, layout, monkeypatch):
    import torch
    monkeypatch.setenv("OGPSX_SWEEP", layout)
    prob, obj, eng = _engine(key)
    assert eng.sweep_mode == layout and eng.n_par == len(prob.parameters) == len(_thetas(key)[0])
    assert eng.parameter_names == tuple(prob.parameters)
    ref = Reference(prob, obj, eng)
    x, h = _point(prob)
    th0, th1, th2 = _thetas(key)
    path = eng.module_path

    def check(theta, what):
        tw = ref.at(theta)
        assert np.array_equal(eng.get_parameters(), theta), what
        F_want, JT_want = tw.sweep(x, h)
        assert np.array_equal(eng.eval_stacked(x), tw.values(x)), what
        F, JT = eng.sweep_stacked(x, h)
        assert np.array_equal(F, F_want) and np.array_equal(JT, JT_want), what
        F, JT = eng.sweep_persistent(x, h)              # every time into the same registered matrix
        assert np.array_equal(F, F_want) and np.array_equal(JT, JT_want), what + " (persistent)"
        FE, JE = eng.exact_stacked(x)
        FE_want, JE_want = tw.exact(x)
        assert np.array_equal(FE, FE_want) and np.array_equal(JE, JE_want), what + " (exact)"
        assert np.array_equal(eng.values(x)[1], F_want[1:1 + eng.m_eq]), what      # (no stale cached values)

    check(th0, "at the values of the trace")
    eng.set_parameters(th1)
    check(th1, "after set_parameters")
    eng.set_parameters(dict(zip(eng.parameter_names, th0)))
    check(th0, "back at the first values")
    d_theta = torch.from_numpy(th2).to(torch.device("cuda", eng.device))
    eng.set_parameters_dev(d_theta.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    check(th2, "after the device-pointer setter")
    assert eng.module_path == path
    # a wrong count is refused by name, and changes nothing
    lib = _native.lib()
    assert lib.og_parameter_count(eng._handle) == eng.n_par
    assert lib.og_set_parameters(eng._handle, _native.dptr(th0), eng.n_par - 1) != 0
    assert b"parameters" in lib.og_last_error()
    assert np.array_equal(eng.get_parameters(), th2)
    if key == "G17" and layout == "fused":
        # the module with theta1 baked in: other kernels, the same bits
        from opengoddard_amd.engine import HipEngine
        eng.set_parameters(th1)
        baked = HipEngine(*pc.goddard(17, th1, baked=True))
        assert baked.module_path != eng.module_path and baked.n_par == 0
        assert np.array_equal(baked.eval_stacked(x), eng.eval_stacked(x))
        for a, b in zip(baked.sweep_stacked(x, h), eng.sweep_stacked(x, h)):
            assert np.array_equal(a, b)
        for a, b in zip(baked.exact_stacked(x), eng.exact_stacked(x)):
            assert np.array_equal(a, b)
        # a handle without parameters: count 0 succeeds, anything else is refused
        assert lib.og_parameter_count(baked._handle) == 0
        assert lib.og_set_parameters(baked._handle, None, 0) == 0
        assert lib.og_set_parameters(baked._handle, _native.dptr(th1), 4) != 0
        baked.close()
    eng.close()


# ------------------------------------------------------------------------------------------------ 2. a NaN parameter
@pytest.mark.parametrize("key", ["P2", "G17"])
def test_a_nan_parameter_fills_its_rows_and_the_next_sweep_cleans_them(key):
    prob, obj, eng = _engine(key)
    ref = Reference(prob, obj, eng)
    x, h = _point(prob)
    th0, bad = _thetas(key)[0], _nan_theta(key)
    F, JT = eng.sweep_persistent(x, h)
    assert np.array_equal(JT, ref.at(th0).sweep(x, h)[1])
    eng.set_parameters(bad)
    F, JT = eng.sweep_persistent(x, h)
    F_want, JT_want = ref.at(bad).sweep(x, h)
    rows = np.flatnonzero(~np.isfinite(F_want))
    assert rows.size >= 1 and np.all(np.isnan(JT[:, rows])) and eng.nonfinite_rows() == rows.size
    assert np.array_equal(F, F_want, equal_nan=True) and np.array_equal(JT, JT_want, equal_nan=True)
    eng.set_parameters(th0)
    F, JT = eng.sweep_persistent(x, h)
    F_want, JT_want = ref.at(th0).sweep(x, h)
    assert np.array_equal(F, F_want) and np.array_equal(JT, JT_want) and eng.nonfinite_rows() == 0
    assert np.count_nonzero(JT) <= eng.pattern()[0][-1]                 # exact zeros again outside the pattern
    eng.close()


# ------------------------------------------------------------------------------------------------ 3. batches
@pytest.mark.parametrize("key", ["P2", "G17"])
def test_every_lane_has_parameters_of_its_own(key):
    prob, obj, eng = _engine(key)
    _, _, single = _engine(key)                 # the single-point path, on a handle of its own
    th = _thetas(key)
    TH = np.stack([th[0], th[1], th[2], 0.5 * (th[0] + th[1]), 0.25 * th[1] + 0.75 * th[2]])
    ALT = TH[::-1].copy()
    pts = [_point(prob, seed) for seed in range(5)]
    same = (np.stack([pts[0][0]] * 5), np.stack([pts[0][1]] * 5))
    five = (np.stack([p[0] for p in pts]), np.stack([p[1] for p in pts]))
    batch = eng.batch(5)
    assert batch.capacity == 5

    def check(count, X, H, lanes_theta, what):
        F0, vals, nonfinite = batch.sweep(X[:count], H[:count])
        FE, vals_e, _ = batch.exact(X[:count])
        FV = batch.values(X[:count])
        for k in range(count):
            single.set_parameters(lanes_theta[k])
            F1, JT1 = single.sweep_stacked(X[k], H[k])
            FX, JX = single.exact_stacked(X[k])
            where = "%s: lane %d of %d" % (what, k, count)
            assert np.array_equal(F0[k], F1, equal_nan=True) and np.array_equal(FV[k], F1, equal_nan=True), where
            assert np.array_equal(FE[k], F1, equal_nan=True), where
            if np.isfinite(F1).all():
                assert nonfinite[k] == 0
                assert np.array_equal(vals[k], _gather(single, JT1)), where
                assert np.array_equal(vals_e[k], _gather(single, JX)), where + " (exact)"
            else:
                assert nonfinite[k] == np.sum(~np.isfinite(F1)), where
        # (the dense matrices are those of the most recent FD sweep: once more, the exact call wrote into them)
        batch.sweep(X[:count], H[:count])
        for k in range(count):
            single.set_parameters(lanes_theta[k])
            JT1 = single.sweep_stacked(X[k], H[k])[1]
            assert np.array_equal(batch.dense(k), JT1, equal_nan=True), "%s: matrix of lane %d" % (what, k)

    # before any parameter call every lane has the handle's values
    check(5, *five, [th[0]] * 5, "fresh batch")
    batch.set_parameters(TH[:3])
    check(3, *same, TH[:3], "count 3, one point")
    batch.set_parameters(TH)
    check(5, *same, TH, "count 5, one point")
    check(5, *five, TH, "count 5, five points")
    # a count-3 call leaves lanes 3 and 4 alone: a later count-5 sweep without a parameter call shows it
    batch.set_parameters(ALT[:3])
    check(5, *five, list(ALT[:3]) + list(TH[3:]), "after a count-3 parameter call")
    # None: the handle's values in every lane, whatever the lanes held
    batch.set_parameters(None)
    check(5, *five, [th[0]] * 5, "after a NULL parameter call")
    # the handle's setter reaches the lanes
    batch.set_parameters(TH)
    eng.set_parameters(th[1])
    check(5, *five, [th[1]] * 5, "after set_parameters on the handle")
    # a NaN lane does not touch its neighbours, and is clean again afterwards
    bad = TH.copy()
    bad[1] = _nan_theta(key)
    batch.set_parameters(bad)
    check(3, *five, bad, "a NaN parameter in lane 1")
    batch.set_parameters(TH)
    check(3, *five, TH, "after the NaN lane")
    assert not np.isnan(batch.dense(1)).any()
    # refused: too many rows, a wrong width
    with pytest.raises(ValueError):
        batch.set_parameters(np.zeros((6, eng.n_par)))
    with pytest.raises(ValueError):
        batch.set_parameters(np.zeros((2, eng.n_par + 1)))
    single.close()
    eng.close()


# ------------------------------------------------------------------------------------------------ 4. captured graph
def test_parameters_and_sweep_replay_from_one_captured_graph():
    import torch
    key = "P2"
    prob, obj, eng = _engine(key)
    _, _, single = _engine(key)
    assert eng.sweep_mode == "fused"
    batch = eng.batch(3)
    n, m, nnz, n_par = eng.n, eng.m, batch.nnz, eng.n_par
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(11)
    lb, ub = np_path.bounds_arrays(prob)

    def arrays():
        return [torch.zeros((3, n_par), dtype=torch.float64, device=dev),
                torch.zeros((3, n), dtype=torch.float64, device=dev), torch.zeros((3, n), dtype=torch.float64, device=dev),
                torch.full((3, m), -1.0, dtype=torch.float64, device=dev),
                torch.full((3, nnz), -1.0, dtype=torch.float64, device=dev)]

    def inputs():
        TH = np.stack(_thetas(key)) * (1.0 + 0.1 * rng.standard_normal((3, n_par)))
        X = np.stack([np.clip(pc.point(prob, int(rng.integers(1000))), lb, ub) for _ in range(3)])
        H = np.stack([_native.fd_step(x, lb, ub) for x in X])
        return TH, X, H

    def load(arr, TH, X, H):
        for t, a in zip(arr[:3], (TH, X, H)):
            t.copy_(torch.from_numpy(a))

    def call(arr, stream):
        batch.set_parameters_dev(3, arr[0].data_ptr(), stream)
        batch.sweep_dev(3, arr[1].data_ptr(), arr[2].data_ptr(), arr[3].data_ptr(), arr[4].data_ptr(), stream)

    def check(arr, TH, X, H, what):
        F, V = arr[3].cpu().numpy(), arr[4].cpu().numpy()
        for k in range(3):
            single.set_parameters(TH[k])
            F1, JT1 = single.sweep_stacked(X[k], H[k])
            assert np.array_equal(F[k], F1), "%s: F of lane %d" % (what, k)
            assert np.array_equal(V[k], _gather(single, JT1)), "%s: values of lane %d" % (what, k)
            assert np.array_equal(batch.dense(k), JT1), "%s: matrix of lane %d" % (what, k)

    side = torch.cuda.Stream()
    A, B = arrays(), arrays()
    inA = inputs()
    with torch.cuda.stream(side):
        load(A, *inA)
        call(A, side.cuda_stream)                         # warm
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        call(A, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    for step in range(3):
        inB = inputs()
        with torch.cuda.stream(side):
            load(B, *inB)
            call(B, side.cuda_stream)                     # a direct call, on other arrays
        torch.cuda.synchronize()
        check(B, *inB, "direct call %d" % step)
        inA = inputs()
        load(A, *inA)                                     # d_TH and d_X overwritten ...
        torch.cuda.synchronize()
        graph.replay()                                    # ... and the graph replayed
        torch.cuda.synchronize()
        check(A, *inA, "replay %d" % step)
    single.close()
    eng.close()


# ------------------------------------------------------------------------------------------------ 5. Problem level
def test_a_second_solve_reuses_the_module_and_continues(monkeypatch, capsys):
    from opengoddard_amd import engine as engine_mod
    compiles, modules = [], []
    real_run, real_build = build._run, build.build_module
    monkeypatch.setattr(build, "_run", lambda cmd: compiles.append(cmd) or real_run(cmd))

    def build_module(*args, **kwargs):
        modules.append(real_build(*args, **kwargs))
        return modules[-1]
    monkeypatch.setattr(build, "build_module", build_module)

    options = dict(sqp_core="scipy", maxiter=4)
    prob, obj = pc.goddard(9)
    assert prob.number_of_variables == 37
    prob.maxIterator = 1
    prob.solve(obj, **options)
    first_p, first_iterator, first_module = prob.p.copy(), prob.iterator, prob._engine.module_path
    assert prob.parameters["T_max"] == 3.5
    prob.set_parameter("T_max", 3.6)
    assert prob._engine.get_parameters()[0] == 3.6           # the live engine follows
    before = len(compiles)
    prob.maxIterator = first_iterator + 1
    prob.solve(obj, **options)
    assert prob._engine.module_path == first_module and modules[-1] == modules[0]
    assert len(compiles) == before, "the second solve ran a compiler"
    assert not np.array_equal(prob.p, first_p)
    # the continuation is what a fresh problem with 3.6 baked in does from the first solve's prob.p
    theta = pc.G_THETA[0].copy()
    theta[0] = 3.6
    fresh, fobj = pc.goddard(9, theta, baked=True)
    fresh.p, fresh.iterator, fresh.maxIterator = first_p.copy(), first_iterator, first_iterator + 1
    fresh.solve(fobj, **options)
    assert fresh._engine.module_path != first_module
    assert np.array_equal(fresh.p, prob.p)
    assert fresh.last_result.nit == prob.last_result.nit and fresh.last_result.fun == prob.last_result.fun
    fresh._engine.close()

    # sensitivities: ONE batched evaluation of n_par + 1 lanes; the quotients of twin values at the same steps
    counts = {"values": 0, "parameters": 0, "lanes": []}
    real_values, real_set = engine_mod.BatchSweep.values, engine_mod.BatchSweep.set_parameters

    def values(self, P):
        counts["values"] += 1
        counts["lanes"].append(np.shape(P)[0])
        return real_values(self, P)

    def set_parameters(self, TH):
        counts["parameters"] += 1
        return real_set(self, TH)
    monkeypatch.setattr(engine_mod.BatchSweep, "values", values)
    monkeypatch.setattr(engine_mod.BatchSweep, "set_parameters", set_parameters)
    x = pc.point(prob, 3)
    dF = prob.parameter_sensitivity(obj, x)
    assert counts == {"values": 1, "parameters": 1, "lanes": [5]}
    eng = prob._engine
    ref = Reference(prob, obj, eng)
    h = _native.fd_step(theta, np.full(4, -np.inf), np.full(4, np.inf))
    F0 = ref.at(theta).values(x)
    assert dF.shape == (4, eng.m)
    for k in range(4):
        moved = theta.copy()
        moved[k] += h[k]
        assert np.array_equal(dF[k], (ref.at(moved).values(x) - F0) / h[k]), pc.G_NAMES[k]
    # a scan at one trajectory through the same lanes, by name
    res = prob.evaluate_batch(obj, x[None, :], jacobian=True, parameters={"Hc": np.array([480.0, 500.0, 520.0])})
    lb, ub = np_path.bounds_arrays(prob)
    hx = _native.fd_step(x, lb, ub)
    for k, hc in enumerate((480.0, 500.0, 520.0)):
        moved = theta.copy()
        moved[1] = hc
        assert np.array_equal(res.parameters[k], moved)
        F_want, JT_want = ref.at(moved).sweep(x, hx)
        assert np.array_equal(np.concatenate([[res.cost[k]], res.equality[k], res.inequality[k]]), F_want)
        assert np.array_equal(res.values[k], _gather(eng, JT_want)) and np.array_equal(res.gradient[k], JT_want[:, 0])
    # ... and without parameters= the earlier per-lane values do not leak
    res = prob.evaluate_batch(obj, np.stack([x, x, x]))
    assert np.array_equal(res.equality[2], ref.at(theta).values(x)[1:1 + eng.m_eq])
    capsys.readouterr()
    eng.close()


# ------------------------------------------------------------------------------------------------ 6. sharding
def test_every_sub_handle_of_a_sharded_solve_takes_the_new_value(monkeypatch, capsys):
    monkeypatch.setenv("OGPSX_GATHER", "peer")          # (lets one device be listed twice: two sub-handles, the real exchange)
    prob, obj = pc.goddard(9)
    prob.maxIterator = 1
    prob.solve(obj, sqp_core="scipy", maxiter=2, devices=[0, 0])
    eng = prob._engine
    assert eng.devices == [0, 0] and eng._multi.value
    ref = Reference(prob, obj, eng)
    x, h = _point(prob, 4)
    F, JT = eng.sweep_persistent(x, h)                  # (og_multi_fd_sweep: each sub-handle sweeps its block of columns)
    F_want, JT_want = ref.at(pc.G_THETA[0]).sweep(x, h)
    assert np.array_equal(F, F_want) and np.array_equal(JT, JT_want)
    prob.set_parameters(pc.G_THETA[1])
    F, JT = eng.sweep_persistent(x, h)
    F_want, JT_want = ref.at(pc.G_THETA[1]).sweep(x, h)
    assert np.array_equal(F, F_want) and np.array_equal(JT, JT_want), "a sub-handle kept the old parameters"
    Fm = np.empty(eng.m)
    _native.check(eng._lib.og_multi_eval(eng._multi, _native.dptr(x), _native.dptr(Fm)), "og_multi_eval")
    assert np.array_equal(Fm, F_want)
    assert eng._lib.og_multi_set_parameters(eng._multi, _native.dptr(pc.G_THETA[1]), 3) != 0
    eng.close()
    prob.maxIterator = prob.iterator + 1
    prob.solve(obj, sqp_core="scipy", maxiter=2, devices=[0, 0])       # the continuation, sharded again
    assert np.array_equal(prob._engine.get_parameters(), pc.G_THETA[1])
    capsys.readouterr()
    prob._engine.close()
    _native.lib().og_comm_finalize()
