"""Exact second derivatives of ``w . F`` in the run-time parameters on the GPU (``og_parameter_hessian*``,
``HipEngine.parameter_hessian``, ``BatchSweep.parameter_hessian``, ``Problem.parameter_hessian``,
``evaluate_batch(parameter_hessians=)``).  The kernels sum the entries of ``csrc/og_pp.h`` in the order ``csrc/og_adj.h``
fixes, so every comparison is BITWISE against the host probe of those headers (tests/pp_probe.cpp, g++), whose own
distance from an independent reference tests/test_parameter_hessian.py bounds.  Shapes
(``parameter_hessian_cases.KEYS``; their modules, batch parts and parameter-Hessian parts are compiled by
``__graft_entry__.build``): E - every operator on a parameter, parameter sets on every switch; P2U - the operand term, an
unread parameter, lists of 0, 1, 9 and 20 entries; NLP - a tail that reads across nodes; G17 / G90 / G257 - one partly
filled block of 64 chains, a partly filled second block, a second trip of two chains.  K = 9 is a full chunk of 8 vectors
and a chunk of one."""

import numpy as np
import pytest

import parameter_exact_cases as ec
import parameter_hessian_cases as hc
from opengoddard_amd import _native, build, problems

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def probe_dir(tmp_path_factory):
    return str(tmp_path_factory.mktemp("pp_probe_gpu"))


def _engine(key):
    from opengoddard_amd.engine import HipEngine
    C = hc.case(key)
    eng = HipEngine(C.prob, C.obj, program=C.program)
    assert eng.header == C.header
    return C, eng


class Probe:
    """``(S, F0)`` of the host probe at ``(x, W, theta)``, computed once per argument set."""

    _EXES = {}

    def __init__(self, key, folder):
        self.case, self.folder = hc.case(key), folder
        if (key, folder) not in Probe._EXES:
            Probe._EXES[(key, folder)] = (hc.build_probe(self.case, folder), {})
        self.exe, self.known = Probe._EXES[(key, folder)]

    def __call__(self, x, W, theta):
        W = np.atleast_2d(np.asarray(W, dtype=float))
        at = (np.asarray(x, dtype=float).tobytes(), W.tobytes(), np.asarray(theta, dtype=float).tobytes())
        if at not in self.known:
            r = hc.run_probe(self.case, self.exe, self.folder, x, W, theta, "gpu")
            self.known[at] = (r.S, r.F0)
        return self.known[at]


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(torch.device("cuda", 0))


def _same(a, b):
    """bit for bit, the sign of a zero included"""
    return np.array_equal(a, b) and np.array_equal(np.signbit(a), np.signbit(b))


THREE = [2, 4, 6]                                       # all ones, a seeded one, the zero vector


# ------------------------------------------------------------------------------------------------ 1. single point
@pytest.mark.parametrize("key", hc.KEYS)
def test_a_single_point_equals_the_probe_bit_for_bit(key, probe_dir):
    """Both points, K = 9 / 3 / 1, the device form and the host form, after ``set_parameters`` to each parameter set."""
    import torch
    C, eng = _engine(key)
    probe = Probe(key, probe_dir)
    stream = torch.cuda.current_stream().cuda_stream
    W9 = hc.weights(C)
    P = eng.n_par
    d_W = _dev(W9)
    d_W3 = _dev(W9[THREE])
    d_S = torch.full((10, P, P), -7.0, dtype=torch.float64, device=d_W.device)
    d_F = torch.full((eng.m,), -7.0, dtype=torch.float64, device=d_W.device)
    for it, theta in enumerate(C.thetas):
        eng.set_parameters(theta)                       # (no rebuild: the same module and part)
        for ip, x in enumerate(C.points):
            want, F_want = probe(x, W9, theta)
            d_x = _dev(x)
            d_S.fill_(-7.0)
            eng.parameter_hessian_dev(d_x.data_ptr(), 9, d_W.data_ptr(), d_S.data_ptr(), d_F.data_ptr(), stream)
            torch.cuda.synchronize()
            S, F0 = d_S.cpu().numpy(), d_F.cpu().numpy()
            assert _same(S[:9], want) and _same(F0, F_want), (key, it, ip)
            assert np.all(S[9:] == -7.0)                # nothing past K slices
            assert _same(S[:9], np.transpose(S[:9], (0, 2, 1)))
            assert not S[6].any() and not np.signbit(S[6]).any()        # the zero vector: +0.0 everywhere
            for k in C.unread:                          # a parameter nothing reads: a row and a column of +0.0
                assert not S[:9, k].any() and not np.signbit(S[:9, k]).any()
                assert not S[:9, :, k].any() and not np.signbit(S[:9, :, k]).any()
            # K = 3 and K = 1: vector d of a call with K vectors is the call with that vector alone (F0 is optional)
            d_S.fill_(-7.0)
            eng.parameter_hessian_dev(d_x.data_ptr(), 3, d_W3.data_ptr(), d_S.data_ptr(), None, stream)
            torch.cuda.synchronize()
            S = d_S.cpu().numpy()
            assert _same(S[:3], want[THREE]) and np.all(S[3:] == -7.0), (key, it, ip)
            for d in (0, 8):
                d_S.fill_(-7.0)
                eng.parameter_hessian_dev(d_x.data_ptr(), 1, d_W[d].data_ptr(), d_S.data_ptr(), None, stream)
                torch.cuda.synchronize()
                one = d_S.cpu().numpy()
                assert _same(one[0], want[d]) and np.all(one[1:] == -7.0), (key, it, ip, d)
            S_h, F_h = eng.parameter_hessian(x, W9)     # the host-pointer form, K = 9 and K = 1
            assert _same(S_h, want) and _same(F_h, F_want)
            S_h, F_h = eng.parameter_hessian(x, W9[3:4])
            assert S_h.shape == (1, P, P) and _same(S_h[0], want[3]) and _same(F_h, F_want)
    assert _same(F_want, eng.eval_stacked(C.points[-1]))            # F0 is og_eval's
    assert eng.pp_part_path == build.pp_part_path(eng.module_path)
    eng.close()


# ------------------------------------------------------------------------------------------------ 2. batches
@pytest.mark.parametrize("key", ["P2U", "G257"])
def test_every_lane_works_at_its_own_point_vector_and_parameters(key, probe_dir):
    import torch
    C, eng = _engine(key)
    probe = Probe(key, probe_dir)
    batch = eng.batch(6)
    X = np.stack([C.points[i % 2] for i in range(5)])
    X[3:] *= 1.0 + 1e-3
    W = hc.weights(C)[[3, 2, 8, 0, 5]]
    TH = np.stack([C.thetas[i % len(C.thetas)] for i in (0, 1, 2, 1, 0)])       # every lane with a parameter row of its own
    batch.set_parameters(TH)
    stream = torch.cuda.current_stream().cuda_stream
    P = eng.n_par
    d_X, d_W = _dev(X), _dev(W)
    for B in (1, 5):                                    # of capacity 6
        d_S = torch.full((6, P, P), -7.0, dtype=torch.float64, device=d_X.device)
        d_F = torch.full((6, eng.m), -7.0, dtype=torch.float64, device=d_X.device)
        batch.parameter_hessian_dev(B, d_X.data_ptr(), d_W.data_ptr(), d_S.data_ptr(), d_F.data_ptr(), stream)
        torch.cuda.synchronize()
        S, F0 = d_S.cpu().numpy(), d_F.cpu().numpy()
        for k in range(B):
            eng.set_parameters(TH[k])                   # (the single-point call at that point and those values ...
            one, F1 = eng.parameter_hessian(X[k], W[k:k + 1])
            batch.set_parameters(TH)       # ... the handle's setter reaches the lanes: theirs again)
            want, F_want = probe(X[k], W[k], TH[k])
            assert _same(one[0], want[0]) and _same(F1, F_want), (key, B, k)
            assert _same(S[k], one[0]) and _same(F0[k], F1), (key, B, k)
        assert np.all(S[B:] == -7.0) and np.all(F0[B:] == -7.0)     # the other lanes' outputs are not touched
    S5, F5 = batch.parameter_hessian(X, W)              # the host form
    assert _same(S5, S[:5]) and _same(F5, F0[:5])
    S1, _ = batch.parameter_hessian(X, W, count=1)
    assert S1.shape == (1, P, P) and _same(S1[0], S[0])
    with pytest.raises(ValueError, match="weight vectors for"):
        batch.parameter_hessian(X, W[:1])
    with pytest.raises(ValueError, match="W must have shape"):
        batch.parameter_hessian(X, W[:, :-1])
    eng.close()


def test_evaluate_batch_equals_the_layer_below_and_without_the_keyword_loads_nothing(probe_dir, monkeypatch):
    """``evaluate_batch(parameter_hessians=W)`` on the real engine: every lane at its own point, vector and row of
    ``parameters=``; one point scanned over ``parameters=``; next to ``jacobian="exact"`` and ``parameter_jacobian=``,
    which keep their bits.  Without the keyword the part is neither built nor loaded: the handle's device call answers
    error 4."""
    from opengoddard_amd import engine as engine_module
    key = "P2U"
    C = hc.case(key)
    probe = Probe(key, probe_dir)
    prob, obj = ec.CASES[key][0]()
    X = np.stack([C.points[0], C.points[1], C.points[0]])
    W = hc.weights(C)[[3, 2, 8]]
    TH = np.stack([C.thetas[0], C.thetas[1], C.thetas[2]])
    P = C.n_par
    calls = []
    real_build = build.build_pp_part
    monkeypatch.setattr(build, "build_pp_part", lambda *a, **k: (calls.append("build_pp_part"), real_build(*a, **k))[1])
    for cls, name in ((engine_module.BatchSweep, "parameter_hessian"), (engine_module.HipEngine, "_load_pp_part")):
        real = getattr(cls, name)
        monkeypatch.setattr(cls, name, lambda self, *a, _real=real, _name=name, **k: (calls.append(_name),
                                                                                      _real(self, *a, **k))[1])
    plain = prob.evaluate_batch(obj, X, jacobian="exact", parameters=TH, parameter_jacobian=True)
    assert plain.parameter_hessian is None and calls == []
    eng = prob._engine
    assert getattr(eng, "pp_part_path", None) is None
    lib = _native.lib()
    assert lib.og_parameter_hessian_dev(eng._handle, 8, 1, 8, 8, None, None) == 4     # its load was never called
    assert b"og_parameter_hessian_load" in lib.og_last_error()
    res = prob.evaluate_batch(obj, X, jacobian="exact", parameters=TH, parameter_jacobian=True, parameter_hessians=W)
    assert calls == ["parameter_hessian", "_load_pp_part", "build_pp_part"]
    assert res.parameter_hessian.shape == (3, P, P)
    assert np.array_equal(res.values, plain.values) and np.array_equal(res.cost, plain.cost)
    assert np.array_equal(res.equality, plain.equality) and np.array_equal(res.inequality, plain.inequality)
    assert np.array_equal(res.parameter_jacobian, plain.parameter_jacobian)
    for k in range(3):
        assert _same(res.parameter_hessian[k], probe(X[k], W[k], TH[k])[0][0])
    scan = prob.evaluate_batch(obj, X[:1], parameters=TH, parameter_hessians=W[:1])
    for k in range(3):
        assert _same(scan.parameter_hessian[k], probe(X[0], W[0], TH[k])[0][0])
    prob.set_parameters(TH[1])
    got = prob.parameter_hessian(obj, W[1], X[1])       # the single-point interface, at the current values
    assert got.shape == (P, P) and _same(got, probe(X[1], W[1], TH[1])[0][0])
    many = prob.parameter_hessian(obj, W, X[1])
    assert many.shape == (3, P, P) and _same(many, probe(X[1], W, TH[1])[0])
    prob._engine.close()
    prob._engine = prob._batch = None


# ------------------------------------------------------------------------------------------------ 3. a captured graph
def test_a_captured_graph_replays_on_another_point_other_vectors_and_other_parameters(probe_dir):
    import torch
    key = "G90"
    C, eng = _engine(key)
    probe = Probe(key, probe_dir)
    dev = torch.device("cuda", 0)
    W = hc.weights(C)
    P = eng.n_par
    d_x = torch.zeros(eng.n, dtype=torch.float64, device=dev)
    d_W = torch.zeros((9, eng.m), dtype=torch.float64, device=dev)
    d_S = torch.full((9, P, P), -7.0, dtype=torch.float64, device=dev)
    d_F = torch.full((eng.m,), -7.0, dtype=torch.float64, device=dev)

    def call(stream):                                   # a linear capture: no parallel branches
        eng.parameter_hessian_dev(d_x.data_ptr(), 9, d_W.data_ptr(), d_S.data_ptr(), d_F.data_ptr(), stream)

    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        d_x.copy_(torch.from_numpy(C.points[0]))
        d_W.copy_(torch.from_numpy(W))
        call(side.cuda_stream)                          # warm: the part is built and loaded outside the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        call(torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    x, rows, theta = C.points[1], [3, 8, 5, 0, 1, 2, 4, 6, 7], C.thetas[2]
    eng.set_parameters(theta)                           # new parameter values: the table on the device, not the graph
    d_x.copy_(torch.from_numpy(x))
    d_W.copy_(torch.from_numpy(W[rows]))
    d_S.fill_(-7.0)
    torch.cuda.synchronize()
    graph.replay()                                      # one replay
    torch.cuda.synchronize()
    replayed, F_replayed = d_S.cpu().numpy(), d_F.cpu().numpy()
    want, F_want = probe(x, W[rows], theta)
    assert _same(replayed, want) and _same(F_replayed, F_want)
    assert not _same(want, probe(C.points[0], W, C.thetas[0])[0])       # (... and it is another result)
    eng.close()


# ------------------------------------------------------------------------------------------------ 4. errors
def test_load_errors_and_a_module_without_parameters():
    lib = _native.lib()
    C, eng = _engine("P2U")
    W9 = hc.weights(C)
    x, W = C.points[0], W9[:2].copy()
    P = eng.n_par
    S, F0 = np.empty((2, P, P)), np.empty(eng.m)
    dp = _native.dptr
    # before the load: 4
    assert lib.og_parameter_hessian(eng._handle, dp(x), 2, dp(W), dp(S), dp(F0)) == 4
    assert b"og_parameter_hessian_load" in lib.og_last_error()
    assert lib.og_parameter_hessian_dev(eng._handle, 8, 1, 8, 8, None, None) == 4
    assert lib.og_parameter_hessian_load(eng._handle, None) == 4
    assert lib.og_parameter_hessian_load(eng._handle, b"/nonexistent/part.so") == 4
    # another module's part, and another part of this module: 5
    other = build.build_pp_part(hc.case("G17").header)
    assert lib.og_parameter_hessian_load(eng._handle, other.encode()) == 5
    assert b"does not belong" in lib.og_last_error()
    assert lib.og_parameter_hessian_load(eng._handle, build.build_mix_part(eng.header).encode()) == 5
    batch = eng.batch(2)
    X = np.stack([x, x])
    assert lib.og_parameter_hessian_batch(batch._handle, 2, dp(X), dp(W), None, dp(S)) == 4
    assert lib.og_parameter_hessian_batch_dev(batch._handle, 2, 8, 8, None, 8, None) == 4
    eng._load_pp_part()
    assert lib.og_parameter_hessian_load(eng._handle, None) == 0    # loaded: a no-op
    # kw = 0, a negative kw, kw past 65535, null pointers, a count out of range: 1 and a message
    assert lib.og_parameter_hessian(eng._handle, dp(x), 0, dp(W), dp(S), None) == 1
    assert b"kw must be at least 1" in lib.og_last_error()
    assert lib.og_parameter_hessian_dev(eng._handle, 8, -3, 8, 8, None, None) == 1
    assert lib.og_parameter_hessian_dev(eng._handle, 8, 65536, 8, 8, None, None) == 1
    assert b"exceeds 65535" in lib.og_last_error()
    assert lib.og_parameter_hessian_dev(eng._handle, 8, 1, None, 8, None, None) == 1
    assert lib.og_parameter_hessian(eng._handle, dp(x), 2, None, dp(S), None) == 1
    assert b"null argument" in lib.og_last_error()
    assert lib.og_parameter_hessian_batch(batch._handle, 0, dp(X), dp(W), None, dp(S)) == 1
    assert lib.og_parameter_hessian_batch(batch._handle, 3, dp(X), dp(W), None, dp(S)) == 1
    assert b"capacity" in lib.og_last_error()
    assert lib.og_parameter_hessian_batch_dev(batch._handle, 2, 8, None, None, 8, None) == 1
    with pytest.raises(ValueError, match="weights must have shape"):
        eng.parameter_hessian(x, W[:, :-1])
    # and the good call still works
    assert lib.og_parameter_hessian(eng._handle, dp(x), 2, dp(W), dp(S), None) == 0
    assert np.all(np.isfinite(S))
    eng.close()
    # a problem with N_PAR == 0: 1 from all five, and the message says which
    from opengoddard_amd.engine import HipEngine
    prob, obj = problems.build("brachistochrone")
    plain = HipEngine(prob, obj)
    assert plain.n_par == 0
    assert lib.og_parameter_hessian_load(plain._handle, b"/nonexistent/part.so") == 1
    assert b"no run-time parameters" in lib.og_last_error()
    xp, Wp, Sp = np.asarray(prob.p, dtype=float), np.zeros((1, plain.m)), np.empty((1, 1, 1))
    assert lib.og_parameter_hessian(plain._handle, dp(xp), 1, dp(Wp), dp(Sp), None) == 1
    assert b"og_parameter_hessian: the module has no run-time parameters" in lib.og_last_error()
    assert lib.og_parameter_hessian_dev(plain._handle, 8, 1, 8, 8, None, None) == 1
    pb = plain.batch(1)
    assert lib.og_parameter_hessian_batch(pb._handle, 1, dp(xp), dp(Wp), None, dp(Sp)) == 1
    assert b"no run-time parameters" in lib.og_last_error()
    assert lib.og_parameter_hessian_batch_dev(pb._handle, 1, 8, 8, None, 8, None) == 1
    with pytest.raises(ValueError, match="declares no parameter"):
        plain.parameter_hessian(xp, Wp)
    plain.close()


# ------------------------------------------------------------------------------------------------ 5. what stays as it was
def test_the_sweep_and_the_parameter_jacobian_on_the_same_handle_keep_their_bits():
    """After ``parameter_hessian`` calls on the same handle ``og_fd_sweep`` (``jacobians``) and ``og_parameter_jacobian``
    return the bits they returned before them: the call disturbs no shared state."""
    C, eng = _engine("G17")
    x, theta = C.points[1], C.thetas[1]
    eng.set_parameters(theta)
    lb = np.array([-np.inf if b[0] is None else b[0] for b in C.prob.bounds], dtype=float)
    ub = np.array([np.inf if b[1] is None else b[1] for b in C.prob.bounds], dtype=float)

    def snapshot():
        (grad, jeq, jineq), h = eng.jacobians(x, lb, ub)
        dF, F0 = eng.parameter_jacobian(x)
        return [np.array(a, dtype=float, copy=True) for a in (grad, jeq, jineq, h, dF, F0)]

    before = snapshot()
    W = hc.weights(C)
    S1, _ = eng.parameter_hessian(x, W)
    S2, _ = eng.parameter_hessian(C.points[0], W[2:3])                  # (all ones: the drag's curvature in Hc depends on x)
    after = snapshot()
    for a, b in zip(before, after):
        assert _same(a, b)
    S3, _ = eng.parameter_hessian(x, W)                 # ... and after them the call its own
    assert _same(S1, S3) and not _same(S1[2:3], S2)
    eng.close()
