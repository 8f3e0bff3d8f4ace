"""Exact dF/dtheta for run-time parameters on the GPU (``og_parameter_jacobian*``, ``HipEngine.parameter_jacobian``,
``BatchSweep.parameter_jacobian``, ``Problem.parameter_sensitivity(exact=True)``,
``evaluate_batch(parameter_jacobian=True)``).  The kernels compute every entry with ``og_par_entry`` (csrc/og_par.h), so
every comparison is BITWISE against the host probe of that function (tests/par_exact_probe.cpp, g++), whose own
distance from the complex step tests/test_parameter_exact.py bounds; the device result is also compared with the
complex step directly, within the same ``BOUND`` - that link shares no generated code with the kernel.  The cases are
those of tests/parameter_exact_cases.py; their modules and parameter parts are compiled by ``__graft_entry__.build``."""

import numpy as np
import pytest

import parameter_cases as pc
import parameter_exact_cases as ec
from opengoddard_amd import _native, build, codegen
from oracle import np_path, twin

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def probe_dir(tmp_path_factory):
    return str(tmp_path_factory.mktemp("par_exact_probe_gpu"))


def _engine(key, theta=None):
    from opengoddard_amd.engine import HipEngine
    prob, obj = ec.CASES[key][0]() if theta is None else ec.CASES[key][0](theta)
    return prob, obj, HipEngine(prob, obj, program=pc.trace(prob, obj))


class Probe:
    """``(dF, F0)`` of the host probe at ``(theta, x)``, computed once per pair."""

    def __init__(self, key, folder):
        self.case, self.folder = ec.case(key), folder
        self.exe = ec.build_probe(self.case, folder)
        self.known = {}

    def __call__(self, theta, x):
        at = (np.asarray(theta, dtype=float).tobytes(), np.asarray(x, dtype=float).tobytes())
        if at not in self.known:
            self.known[at] = ec.run_probe(self.case, self.exe, self.folder, theta, x, "gpu")
        return self.known[at]


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(torch.device("cuda", 0))


# ------------------------------------------------------------------------------------------------ 4. single point
@pytest.mark.parametrize("key", ["P2", "P2U", "G9", "G17", "E"])
def test_a_single_point_equals_the_probe_bit_for_bit(key, probe_dir):
    import torch
    case = ec.case(key)
    prob, obj, eng = _engine(key)
    assert eng.header == case.header
    probe = Probe(key, probe_dir)
    S = codegen.parameter_sparsity(case.program)
    path = eng.module_path
    stream = torch.cuda.current_stream().cuda_stream
    for theta in case.thetas[:3] if key != "E" else case.thetas:
        eng.set_parameters(theta)                       # (no rebuild: the same module and part)
        for x in case.points:
            want, F_want = probe(theta, x)
            d_x = _dev(x)
            d_dF = torch.full((eng.n_par, eng.m), -7.0, dtype=torch.float64, device=d_x.device)
            d_F = torch.full((eng.m,), -7.0, dtype=torch.float64, device=d_x.device)
            eng.parameter_jacobian_dev(d_x.data_ptr(), d_dF.data_ptr(), d_F.data_ptr(), stream)
            torch.cuda.synchronize()
            dF, F0 = d_dF.cpu().numpy(), d_F.cpu().numpy()
            assert np.array_equal(dF, want) and np.array_equal(F0, F_want), (key, theta)
            outside = dF[~S]
            assert not outside.any() and not np.signbit(outside).any()
            d_dF.fill_(-7.0)
            eng.parameter_jacobian_dev(d_x.data_ptr(), d_dF.data_ptr(), None, stream)      # F0 is optional
            torch.cuda.synchronize()
            assert np.array_equal(d_dF.cpu().numpy(), want)
            dF_h, F_h = eng.parameter_jacobian(x)       # the host-pointer form
            assert np.array_equal(dF_h, want) and np.array_equal(F_h, F_want)
            assert ec.worst_error(dF, ec.complex_step(case, theta, x)) <= ec.BOUND
    assert eng.module_path == path and eng.parameter_part_path == build.parameter_part_path(path)
    eng.close()


# ------------------------------------------------------------------------------------------------ 5. batches
@pytest.mark.parametrize("key", ["P2", "G17"])
def test_every_lane_works_at_its_own_point_and_parameters(key, probe_dir):
    import torch
    case = ec.case(key)
    prob, obj, eng = _engine(key)
    probe = Probe(key, probe_dir)
    th = case.thetas
    batch = eng.batch(3)
    X = np.stack([case.points[0], case.points[1], case.points[0]])
    TH = np.stack([th[1], th[2], th[1]])
    batch.set_parameters(TH)
    # the device-pointer form into sentinel-filled arrays: count = 2 of capacity 3
    d_X = _dev(X)
    d_dF = torch.full((3, eng.n_par, eng.m), -7.0, dtype=torch.float64, device=d_X.device)
    d_F = torch.full((3, eng.m), -7.0, dtype=torch.float64, device=d_X.device)
    batch.parameter_jacobian_dev(2, d_X.data_ptr(), d_dF.data_ptr(), d_F.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    dF, F0 = d_dF.cpu().numpy(), d_F.cpu().numpy()
    for k in range(2):
        eng.set_parameters(TH[k])                       # (the single-point call at that point and those values ...
        one, F1 = eng.parameter_jacobian(X[k])
        assert np.array_equal(one, probe(TH[k], X[k])[0])
        batch.set_parameters(TH)                        # ... the handle's setter reaches the lanes: theirs again)
        assert np.array_equal(dF[k], one) and np.array_equal(F0[k], F1), (key, k)
    assert np.all(dF[2] == -7.0) and np.all(F0[2] == -7.0)      # lane 2 and its output are not touched
    # the host form, all three lanes
    dF3, F3 = batch.parameter_jacobian(X)
    assert np.array_equal(dF3[:2], dF[:2]) and np.array_equal(dF3[2], probe(TH[2], X[2])[0])
    assert np.array_equal(F3[2], probe(TH[2], X[2])[1])
    dF2, _ = batch.parameter_jacobian(X, count=2)
    assert dF2.shape == (2, eng.n_par, eng.m) and np.array_equal(dF2, dF[:2])
    # NULL: every lane at the handle's values
    eng.set_parameters(th[0])
    batch.set_parameters(TH)
    batch.set_parameters(None)
    dF3, _ = batch.parameter_jacobian(X)
    for k in range(3):
        assert np.array_equal(dF3[k], probe(th[0], X[k])[0])
    eng.close()

    # Problem level: both Jacobians from one call, the exact one in x bit for bit what it is without the flag
    prob, obj = ec.CASES[key][0]()
    res = prob.evaluate_batch(obj, X, jacobian="exact", parameters=TH, parameter_jacobian=True)
    plain = prob.evaluate_batch(obj, X, jacobian="exact", parameters=TH)
    assert plain.parameter_jacobian is None and res.parameter_jacobian.shape == (3, eng.n_par, eng.m)
    assert np.array_equal(res.values, plain.values) and np.array_equal(res.cost, plain.cost)
    assert np.array_equal(res.equality, plain.equality) and np.array_equal(res.gradient, plain.gradient)
    for k in range(3):
        assert np.array_equal(res.parameter_jacobian[k], probe(TH[k], X[k])[0])
    only = prob.evaluate_batch(obj, X, parameters=TH, parameter_jacobian=True)
    assert np.array_equal(only.parameter_jacobian, res.parameter_jacobian) and np.array_equal(only.cost, res.cost)
    prob._engine.close()


# ------------------------------------------------------------------------------------------------ 6. J_T bookkeeping
def test_the_bookkeeping_of_registered_matrices_is_not_disturbed(probe_dir):
    import torch
    key = "P2"
    case = ec.case(key)
    prob, obj, eng = _engine(key)
    probe = Probe(key, probe_dir)
    tw = twin.Twin(prob, obj, program=case.program, header=eng.header)
    lb, ub = np_path.bounds_arrays(prob)
    xa, xb = case.points
    ha, hb = _native.fd_step(xa, lb, ub), _native.fd_step(xb, lb, ub)
    theta = case.thetas[0]
    bad = theta.copy()
    bad[1] = np.nan                                     # `b`, a boundary row: F has a non-finite row, J_T a NaN fill
    off = case.program.par_off
    want_par = probe(theta, xb)[0]
    stream = torch.cuda.current_stream().cuda_stream
    d_JT = torch.full((eng.n, eng.m), -7.0, dtype=torch.float64, device=torch.device("cuda", 0))
    d_F = torch.zeros(eng.m, dtype=torch.float64, device=d_JT.device)
    d_dF = torch.zeros((eng.n_par, eng.m), dtype=torch.float64, device=d_JT.device)
    eng.register_jt_dev(d_JT.data_ptr(), 0, eng.n, stream)

    def sweep(x, h):
        d_x, d_h = _dev(x), _dev(h)
        eng.sweep_dev(d_x.data_ptr(), d_h.data_ptr(), 0, eng.n, d_JT.data_ptr(), d_F.data_ptr(), stream)
        torch.cuda.synchronize()
        return d_JT.cpu().numpy()

    def parameters(x):
        d_x = _dev(x)
        eng.parameter_jacobian_dev(d_x.data_ptr(), d_dF.data_ptr(), None, stream)
        torch.cuda.synchronize()
        return d_dF.cpu().numpy()

    assert np.array_equal(sweep(xa, ha), tw.sweep(xa, ha)[1])
    assert np.array_equal(parameters(xb), want_par)
    assert np.array_equal(sweep(xb, hb), tw.sweep(xb, hb)[1])           # (dense: the structural zeros are still zeros)
    # a NaN fill, the parameter call, then a good sweep: the call neither cleans the fill nor keeps it from being cleaned
    eng.set_parameters(bad)
    tw._cv[off:] = bad
    JT = sweep(xa, ha)
    assert np.array_equal(JT, tw.sweep(xa, ha)[1], equal_nan=True) and np.isnan(JT).any()
    assert np.array_equal(parameters(xb), probe(bad, xb)[0], equal_nan=True) and eng.nonfinite_rows() == 1
    eng.set_parameters(theta)
    tw._cv[off:] = theta
    assert np.array_equal(parameters(xb), want_par) and eng.nonfinite_rows() == 0
    assert np.array_equal(d_JT.cpu().numpy(), JT, equal_nan=True)       # the fill is where it was
    JT = sweep(xb, hb)
    assert np.array_equal(JT, tw.sweep(xb, hb)[1]) and np.count_nonzero(JT) <= eng.pattern()[0][-1]
    eng.unregister_jt_dev(d_JT.data_ptr())

    # the same in the lanes of a batch (lane 0 at the NaN parameter for one sweep)
    batch = eng.batch(2)
    X, H = np.stack([xa, xb]), np.stack([ha, hb])
    batch.sweep(X, H)
    assert np.array_equal(batch.dense(0), tw.sweep(xa, ha)[1])
    dF, _ = batch.parameter_jacobian(X[::-1].copy())
    assert np.array_equal(dF[0], want_par)
    batch.sweep(X, H)
    assert np.array_equal(batch.dense(1), tw.sweep(xb, hb)[1])
    batch.set_parameters(np.stack([bad, theta]))
    batch.sweep(X, H)
    assert np.isnan(batch.dense(0)).any()
    dF, _ = batch.parameter_jacobian(X[::-1].copy())
    assert np.array_equal(dF[1], probe(theta, xa)[0]) and np.isnan(batch.dense(0)).any()
    batch.set_parameters(None)
    dF, _ = batch.parameter_jacobian(X[::-1].copy())
    assert np.array_equal(dF[0], want_par) and np.isnan(batch.dense(0)).any()
    batch.sweep(X, H)
    for k, (x, h) in enumerate(((xa, ha), (xb, hb))):
        assert np.array_equal(batch.dense(k), tw.sweep(x, h)[1])
    eng.close()


# ------------------------------------------------------------------------------------------------ 7. one captured graph
def test_parameters_and_their_jacobian_replay_from_one_captured_graph(probe_dir):
    import torch
    key = "P2"
    case = ec.case(key)
    prob, obj, eng = _engine(key)
    probe = Probe(key, probe_dir)
    dev = torch.device("cuda", 0)
    d_theta = torch.zeros(eng.n_par, dtype=torch.float64, device=dev)
    d_x = torch.zeros(eng.n, dtype=torch.float64, device=dev)
    d_dF = torch.full((eng.n_par, eng.m), -7.0, dtype=torch.float64, device=dev)
    d_F = torch.full((eng.m,), -7.0, dtype=torch.float64, device=dev)

    def call(stream):                                   # a linear capture: no parallel branches
        eng.set_parameters_dev(d_theta.data_ptr(), stream)
        eng.parameter_jacobian_dev(d_x.data_ptr(), d_dF.data_ptr(), d_F.data_ptr(), stream)

    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        d_theta.copy_(torch.from_numpy(case.thetas[0]))
        d_x.copy_(torch.from_numpy(case.points[0]))
        call(side.cuda_stream)                          # warm: the part is built and loaded outside the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        call(torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    for theta, x in ((case.thetas[1], case.points[1]), (case.thetas[2], case.points[0])):
        d_theta.copy_(torch.from_numpy(theta))
        d_x.copy_(torch.from_numpy(x))
        d_dF.fill_(-7.0)
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        want, F_want = probe(theta, x)
        assert np.array_equal(d_dF.cpu().numpy(), want) and np.array_equal(d_F.cpu().numpy(), F_want)
        assert np.array_equal(eng.get_parameters(), theta)
    eng.close()


# ------------------------------------------------------------------------------------------------ 8. errors
def test_errors_and_a_nan_parameter(probe_dir):
    from opengoddard_amd.engine import HipEngine
    lib = _native.lib()
    key = "P2"
    case = ec.case(key)
    prob, obj, eng = _engine(key)
    x = case.points[0]
    dF, F0 = np.empty((eng.n_par, eng.m)), np.empty(eng.m)
    # before the load: 4
    assert lib.og_parameter_jacobian(eng._handle, _native.dptr(x), _native.dptr(dF), _native.dptr(F0)) == 4
    assert b"og_parameter_jacobian_load" in lib.og_last_error()
    assert lib.og_parameter_jacobian_dev(eng._handle, 8, 8, None, None) == 4
    assert lib.og_parameter_jacobian_load(eng._handle, None) == 4
    assert lib.og_parameter_jacobian_load(eng._handle, b"/nonexistent/part.so") == 4
    # another module's part: 5
    other = build.build_parameter_part(ec.case("G9").header)
    assert lib.og_parameter_jacobian_load(eng._handle, other.encode()) == 5
    assert b"does not belong" in lib.og_last_error()
    # a handle without parameters: 1 and a message, from every call
    baked = HipEngine(*pc.p2(baked=True))
    assert baked.n_par == 0
    part = build.build_parameter_part(eng.header)
    assert lib.og_parameter_jacobian_load(baked._handle, part.encode()) == 1
    assert b"no run-time parameters" in lib.og_last_error()
    assert lib.og_parameter_jacobian(baked._handle, _native.dptr(x), _native.dptr(dF), None) == 1
    assert lib.og_parameter_jacobian_dev(baked._handle, 8, 8, None, None) == 1
    with pytest.raises(ValueError, match="declares no parameter"):
        baked.parameter_jacobian(x)
    baked.close()
    # a NaN parameter: NaN in its dependent rows, the evaluation's count of non-finite rows, clean afterwards
    probe = Probe(key, probe_dir)
    S = codegen.parameter_sparsity(case.program)
    theta = case.thetas[0].copy()
    theta[0] = np.nan                                   # `a` multiplies the control in both phases' dynamics
    eng.set_parameters(theta)
    dF, F0 = eng.parameter_jacobian(x)
    assert np.all(np.isnan(dF[0][S[0]])) and not np.isnan(dF[1:]).any()
    assert np.array_equal(dF[1:], probe(case.thetas[0], x)[0][1:])
    assert eng.nonfinite_rows() == np.sum(~np.isfinite(F0)) == S[0].sum()
    eng.set_parameters(case.thetas[0])
    dF, F0 = eng.parameter_jacobian(x)
    assert np.array_equal(dF, probe(case.thetas[0], x)[0]) and eng.nonfinite_rows() == 0
    eng.close()


# ------------------------------------------------------------------------------------------------ 9. Problem level
def test_exact_sensitivity_on_the_device(probe_dir, capsys):
    key = "G9"
    case = ec.case(key)
    probe = Probe(key, probe_dir)
    prob, obj = ec.CASES[key][0]()
    x = case.points[0]
    got = prob.parameter_sensitivity(obj, x, exact=True)
    assert getattr(prob, "_batch", None) is None        # one engine call, no batch
    assert np.array_equal(got, probe(case.thetas[0], x)[0])
    prob.set_parameters(case.thetas[1])                 # the live engine follows
    got = prob.parameter_sensitivity(obj, x, exact=True)
    want = probe(case.thetas[1], x)[0]
    assert np.array_equal(got, want)
    # the forward-difference form.  The suite's bound for FD noise of J_T against the goldens is for steps in x and does
    # not apply unchanged; both forms are compared with the complex step.  A one-sided difference with h = sqrt(eps)
    # |theta| is off by eps |F| / h + h |F''| / 2: with |F| <= 10 and |F''| <= 10 (the mass row, 2 T tf / (2 c^3)) at
    # theta of order 1 that is below 2e-7 of a row whose scale is at least 1; 1e-6 leaves a factor of five
    ref = ec.complex_step(case, case.thetas[1], x)
    fd = prob.parameter_sensitivity(obj, x)
    assert ec.worst_error(got, ref) <= ec.BOUND
    assert ec.worst_error(fd, ref) <= 1e-6 and ec.worst_error(fd, ref) > ec.worst_error(got, ref)
    capsys.readouterr()
    prob._engine.close()


# ------------------------------------------------------------------------------------------------ 10. sharded
def test_a_sharded_engine_serves_the_call_from_its_first_handle(monkeypatch, probe_dir):
    from opengoddard_amd.engine import HipEngine
    monkeypatch.setenv("OGPSX_GATHER", "peer")          # (lets one device be listed twice: two sub-handles)
    key = "P2"
    case = ec.case(key)
    probe = Probe(key, probe_dir)
    prob, obj = ec.CASES[key][0]()
    eng = HipEngine(prob, obj, program=pc.trace(prob, obj), devices=[0, 0])
    assert eng.devices == [0, 0] and eng._multi.value
    x = case.points[1]
    eng.set_parameters(case.thetas[2])                  # (every sub-handle and the first device's handle)
    dF, F0 = eng.parameter_jacobian(x)
    want, F_want = probe(case.thetas[2], x)
    assert np.array_equal(dF, want) and np.array_equal(F0, F_want)
    Fm = np.empty(eng.m)
    _native.check(eng._lib.og_multi_eval(eng._multi, _native.dptr(x), _native.dptr(Fm)), "og_multi_eval")
    assert np.array_equal(Fm, F_want)
    eng.close()
    _native.lib().og_comm_finalize()
