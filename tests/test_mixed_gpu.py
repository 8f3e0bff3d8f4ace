"""Exact mixed derivatives ``d(F'(x)^T w)/dtheta`` on the GPU (``og_adjoint_parameter*``, ``HipEngine.adjoint_parameter``,
``BatchSweep.adjoint_parameter``, ``Problem.adjoint_parameter_sensitivity``, ``evaluate_batch(adjoint_parameter=)``).  The
kernels sum the terms of ``csrc/og_mix.h`` in the order ``csrc/og_adj.h`` fixes, so every comparison is BITWISE against
the host probe of those headers (tests/mix_probe.cpp, g++), whose own distance from an independent reference
tests/test_mixed.py bounds.  Shapes (``mixed_cases.KEYS``; their modules, batch parts and mixed parts are compiled by
``__graft_entry__.build``): P2U - the operand term, an unread parameter; P2; G9 / G17 - ``n`` no multiple of 4; E - every
operator on a parameter; B90g - 90 nodes, the final time is heavy, reads the parameter and its 272 terms take a thread
through its chain twice.  tests/test_mixed.py checks on the CPU that the shapes contain these."""

import numpy as np
import pytest

import adjoint_cases as ac
import hessian_cases as hc
import mixed_cases as mc
from opengoddard_amd import _native, build, problems

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def probe_dir(tmp_path_factory):
    return str(tmp_path_factory.mktemp("mix_probe_gpu"))


def _engine(key):
    from opengoddard_amd.engine import HipEngine
    C = mc.case(key)
    eng = HipEngine(C.prob, C.obj, program=C.program)
    assert eng.header == C.header
    return C, eng


class Probe:
    """``(S, F0)`` of the host probe at ``(x, W, theta)``, computed once per argument set."""

    def __init__(self, key, folder):
        self.case, self.folder = mc.case(key), folder
        self.exe = mc.build_probe(self.case, folder)
        self.known = {}

    def __call__(self, x, W, theta):
        W = np.atleast_2d(np.asarray(W, dtype=float))
        at = (np.asarray(x, dtype=float).tobytes(), W.tobytes(), np.asarray(theta, dtype=float).tobytes())
        if at not in self.known:
            r = mc.run_probe(self.case, self.exe, self.folder, x, W, theta, "gpu")
            self.known[at] = (r.S, r.F0)
        return self.known[at]


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(torch.device("cuda", 0))


def _same(a, b):
    """bit for bit, the sign of a zero included"""
    return np.array_equal(a, b) and np.array_equal(np.signbit(a), np.signbit(b))


# ------------------------------------------------------------------------------------------------ 1. single point
@pytest.mark.parametrize("key", mc.KEYS)
def test_a_single_point_equals_the_probe_bit_for_bit(key, probe_dir):
    import torch
    C, eng = _engine(key)
    probe = Probe(key, probe_dir)
    stream = torch.cuda.current_stream().cuda_stream
    W9 = mc.weights(C)
    three = [2, 4, 6]                                   # all ones, a seeded one, the zero vector
    theta, x = C.thetas[-1], C.points[-1]
    eng.set_parameters(theta)                           # (no rebuild: the same module and part)
    want, F_want = probe(x, W9, theta)
    assert _same(F_want, eng.eval_stacked(x))           # F0 is og_eval's
    P, n = eng.n_par, eng.n
    d_x, d_W = _dev(x), _dev(W9)
    d_S = torch.full((10, P, n), -7.0, dtype=torch.float64, device=d_x.device)
    d_F = torch.full((eng.m,), -7.0, dtype=torch.float64, device=d_x.device)
    eng.adjoint_parameter_dev(d_x.data_ptr(), 9, d_W.data_ptr(), d_S.data_ptr(), d_F.data_ptr(), stream)
    torch.cuda.synchronize()
    S, F0 = d_S.cpu().numpy(), d_F.cpu().numpy()
    assert _same(S[:9], want) and _same(F0, F_want), key
    assert np.all(S[9:] == -7.0)                        # nothing past K slices
    assert not S[6].any() and not np.signbit(S[6]).any()            # the zero vector: +0.0 everywhere
    for k in C.unread:                                  # a parameter nothing reads: a row of +0.0
        assert not S[:9, k].any() and not np.signbit(S[:9, k]).any()
    # K = 3 and K = 1: vector d of a call with K vectors is the call with that vector alone (F0 is optional)
    d_W3 = _dev(W9[three])
    d_S.fill_(-7.0)
    eng.adjoint_parameter_dev(d_x.data_ptr(), 3, d_W3.data_ptr(), d_S.data_ptr(), None, stream)
    torch.cuda.synchronize()
    S = d_S.cpu().numpy()
    assert _same(S[:3], want[three]) and np.all(S[3:] == -7.0), key
    for d in (0, 5, 8):
        d_S.fill_(-7.0)
        eng.adjoint_parameter_dev(d_x.data_ptr(), 1, d_W[d].data_ptr(), d_S.data_ptr(), None, stream)
        torch.cuda.synchronize()
        one = d_S.cpu().numpy()
        assert _same(one[0], want[d]) and np.all(one[1:] == -7.0), (key, d)
    S_h, F_h = eng.adjoint_parameter(x, W9)             # the host-pointer form, K = 9 and K = 1
    assert _same(S_h, want) and _same(F_h, F_want)
    S_h, F_h = eng.adjoint_parameter(x, W9[3:4])
    assert S_h.shape == (1, P, n) and _same(S_h[0], want[3]) and _same(F_h, F_want)
    assert eng.mix_part_path == build.mix_part_path(eng.module_path)
    eng.close()


def test_after_set_parameters_the_result_is_that_of_the_new_values(probe_dir):
    C, eng = _engine("G9")
    probe = Probe("G9", probe_dir)
    x, W = C.points[0], mc.weights(C)[[3, 4]]
    seen = []
    for theta in (C.thetas[0], C.thetas[2], C.thetas[1]):
        eng.set_parameters(theta)
        S, F0 = eng.adjoint_parameter(x, W)
        want, F_want = probe(x, W, theta)
        assert _same(S, want) and _same(F0, F_want)
        seen.append(S)
    assert not np.array_equal(seen[0], seen[1]) and not np.array_equal(seen[1], seen[2])
    eng.close()


# ------------------------------------------------------------------------------------------------ 2. batches
@pytest.mark.parametrize("key", ["P2U", "B90g"])
def test_every_lane_works_at_its_own_point_vector_and_parameters(key, probe_dir):
    import torch
    C, eng = _engine(key)
    probe = Probe(key, probe_dir)
    batch = eng.batch(4)
    X = np.stack([C.points[0], C.points[1], C.points[0]])
    W = mc.weights(C)[[3, 2, 8]]
    TH = np.stack([C.thetas[0], C.thetas[1], C.thetas[2]])          # every lane with a parameter row of its own
    batch.set_parameters(TH)
    stream = torch.cuda.current_stream().cuda_stream
    P, n = eng.n_par, eng.n
    d_X, d_W = _dev(X), _dev(W)
    for B in (1, 3):                                    # of capacity 4
        d_S = torch.full((4, P, n), -7.0, dtype=torch.float64, device=d_X.device)
        d_F = torch.full((4, eng.m), -7.0, dtype=torch.float64, device=d_X.device)
        batch.adjoint_parameter_dev(B, d_X.data_ptr(), d_W.data_ptr(), d_S.data_ptr(), d_F.data_ptr(), stream)
        torch.cuda.synchronize()
        S, F0 = d_S.cpu().numpy(), d_F.cpu().numpy()
        for k in range(B):
            eng.set_parameters(TH[k])                   # (the single-point call at that point and those values ...
            one, F1 = eng.adjoint_parameter(X[k], W[k:k + 1])
            batch.set_parameters(TH)                    # ... the handle's setter reaches the lanes: theirs again)
            want, F_want = probe(X[k], W[k], TH[k])
            assert _same(one[0], want[0]) and _same(F1, F_want), (key, B, k)
            assert _same(S[k], one[0]) and _same(F0[k], F1), (key, B, k)
        assert np.all(S[B:] == -7.0) and np.all(F0[B:] == -7.0)     # the other lanes' outputs are not touched
    S3, F3 = batch.adjoint_parameter(X, W)              # the host form
    assert _same(S3, S[:3]) and _same(F3, F0[:3])
    S1, _ = batch.adjoint_parameter(X, W, count=1)
    assert S1.shape == (1, P, n) and _same(S1[0], S[0])
    with pytest.raises(ValueError, match="weight vectors for"):
        batch.adjoint_parameter(X, W[:1])
    with pytest.raises(ValueError, match="W must have shape"):
        batch.adjoint_parameter(X, W[:, :-1])
    eng.close()

    # Problem level: next to jacobian="exact" and adjoints=, which are bit for bit what they are without the keyword; and
    # one point scanned over the rows of parameters=
    prob, obj = C.prob, C.obj
    res = prob.evaluate_batch(obj, X, jacobian="exact", parameters=TH, adjoints=W, adjoint_parameter=W)
    plain = prob.evaluate_batch(obj, X, jacobian="exact", parameters=TH, adjoints=W)
    assert plain.adjoint_parameter is None and res.adjoint_parameter.shape == (3, P, n)
    assert np.array_equal(res.values, plain.values) and np.array_equal(res.cost, plain.cost)
    assert np.array_equal(res.equality, plain.equality) and np.array_equal(res.adjoint, plain.adjoint)
    for k in range(3):
        assert _same(res.adjoint_parameter[k], probe(X[k], W[k], TH[k])[0][0])
    scan = prob.evaluate_batch(obj, X[:1], parameters=TH, adjoint_parameter=W[:1])
    for k in range(3):
        assert _same(scan.adjoint_parameter[k], probe(X[0], W[0], TH[k])[0][0])
    prob.set_parameters(TH[1])
    got = prob.adjoint_parameter_sensitivity(obj, W[1], X[1])       # the single-point interface, at the current values
    assert got.shape == (P, n) and _same(got, probe(X[1], W[1], TH[1])[0][0])
    prob.set_parameters(C.thetas[0])
    prob._engine.close()
    prob._engine = prob._batch = None


# ------------------------------------------------------------------------------------------------ 3. a captured graph
def test_a_captured_graph_replays_on_another_point_and_other_vectors(probe_dir):
    import torch
    key = "G17"
    C, eng = _engine(key)
    probe = Probe(key, probe_dir)
    dev = torch.device("cuda", 0)
    W = mc.weights(C)
    P = eng.n_par
    d_x = torch.zeros(eng.n, dtype=torch.float64, device=dev)
    d_W = torch.zeros((3, eng.m), dtype=torch.float64, device=dev)
    d_S = torch.full((3, P, eng.n), -7.0, dtype=torch.float64, device=dev)
    d_F = torch.full((eng.m,), -7.0, dtype=torch.float64, device=dev)

    def call(stream):                                   # a linear capture: no parallel branches
        eng.adjoint_parameter_dev(d_x.data_ptr(), 3, d_W.data_ptr(), d_S.data_ptr(), d_F.data_ptr(), stream)

    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        d_x.copy_(torch.from_numpy(C.points[0]))
        d_W.copy_(torch.from_numpy(W[[0, 1, 2]]))
        call(side.cuda_stream)                          # warm: the part is built and loaded outside the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        call(torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    x, rows = C.points[1], [3, 8, 5]
    d_x.copy_(torch.from_numpy(x))
    d_W.copy_(torch.from_numpy(W[rows]))
    d_S.fill_(-7.0)
    torch.cuda.synchronize()
    graph.replay()                                      # one replay
    torch.cuda.synchronize()
    replayed, F_replayed = d_S.cpu().numpy(), d_F.cpu().numpy()
    want, F_want = probe(x, W[rows], C.thetas[0])
    assert _same(replayed, want) and _same(F_replayed, F_want)
    eng.close()


# ------------------------------------------------------------------------------------------------ 4. errors
def test_errors_before_the_load_for_no_vector_and_without_parameters():
    lib = _native.lib()
    C, eng = _engine("P2U")
    W9 = mc.weights(C)
    x, W = C.points[0], W9[:2].copy()
    P = eng.n_par
    S, F0 = np.empty((2, P, eng.n)), np.empty(eng.m)
    dp = _native.dptr
    # before the load: 4
    assert lib.og_adjoint_parameter(eng._handle, dp(x), 2, dp(W), dp(S), dp(F0)) == 4
    assert b"og_adjoint_parameter_load" in lib.og_last_error()
    assert lib.og_adjoint_parameter_dev(eng._handle, 8, 1, 8, 8, None, None) == 4
    assert lib.og_adjoint_parameter_load(eng._handle, None) == 4
    assert lib.og_adjoint_parameter_load(eng._handle, b"/nonexistent/part.so") == 4
    # another module's part, and another part of this module: 5
    other = build.build_mix_part(mc.case("G17").header)
    assert lib.og_adjoint_parameter_load(eng._handle, other.encode()) == 5
    assert b"does not belong" in lib.og_last_error()
    assert lib.og_adjoint_parameter_load(eng._handle, build.build_adjoint_part(eng.header).encode()) == 5
    batch = eng.batch(2)
    X = np.stack([x, x])
    assert lib.og_adjoint_parameter_batch(batch._handle, 2, dp(X), dp(W), None, dp(S)) == 4
    eng._load_mix_part()
    assert lib.og_adjoint_parameter_load(eng._handle, None) == 0    # loaded: a no-op
    # k = 0, a negative k, k * n_par past 65535, null pointers, a count out of range: 1 and a message
    assert lib.og_adjoint_parameter(eng._handle, dp(x), 0, dp(W), dp(S), None) == 1
    assert b"k must be at least 1" in lib.og_last_error()
    assert lib.og_adjoint_parameter_dev(eng._handle, 8, -3, 8, 8, None, None) == 1
    assert lib.og_adjoint_parameter_dev(eng._handle, 8, 65535 // P + 1, 8, 8, None, None) == 1
    assert b"exceeds 65535" in lib.og_last_error()
    assert lib.og_adjoint_parameter_dev(eng._handle, 8, 1, None, 8, None, None) == 1
    assert lib.og_adjoint_parameter(eng._handle, dp(x), 2, None, dp(S), None) == 1
    assert b"null argument" in lib.og_last_error()
    assert lib.og_adjoint_parameter_batch(batch._handle, 0, dp(X), dp(W), None, dp(S)) == 1
    assert lib.og_adjoint_parameter_batch(batch._handle, 3, dp(X), dp(W), None, dp(S)) == 1
    assert b"capacity" in lib.og_last_error()
    assert lib.og_adjoint_parameter_batch_dev(batch._handle, 2, 8, None, None, 8, None) == 1
    with pytest.raises(ValueError, match="weights must have shape"):
        eng.adjoint_parameter(x, W[:, :-1])
    # and the good call still works
    assert lib.og_adjoint_parameter(eng._handle, dp(x), 2, dp(W), dp(S), None) == 0
    assert np.all(np.isfinite(S))
    eng.close()
    # a problem with N_PAR == 0: 1, and the message says which
    from opengoddard_amd.engine import HipEngine
    prob, obj = problems.build("brachistochrone")
    plain = HipEngine(prob, obj)
    assert plain.n_par == 0
    assert lib.og_adjoint_parameter_load(plain._handle, b"/nonexistent/part.so") == 1
    assert b"no run-time parameters" in lib.og_last_error()
    xp, Wp, Sp = np.asarray(prob.p, dtype=float), np.zeros((1, plain.m)), np.empty((1, 1, plain.n))
    assert lib.og_adjoint_parameter(plain._handle, dp(xp), 1, dp(Wp), dp(Sp), None) == 1
    assert b"og_adjoint_parameter: the module has no run-time parameters" in lib.og_last_error()
    assert lib.og_adjoint_parameter_dev(plain._handle, 8, 1, 8, 8, None, None) == 1
    with pytest.raises(ValueError, match="declares no parameter"):
        plain.adjoint_parameter(xp, Wp)
    plain.close()


# ------------------------------------------------------------------------------------------------ 5. what stays as it was
def test_without_the_keyword_nothing_of_the_feature_runs(monkeypatch):
    """``evaluate_batch(adjoint_parameter=None)``: the mixed part is neither built nor loaded and no entry point of the
    feature is called, and every result is bit for bit what the call with the keyword returns next to the derivative."""
    from opengoddard_amd import engine as engine_module
    C = mc.case("P2U")
    prob, obj = C.prob, C.obj
    X = np.stack([C.points[0], C.points[1]])
    W = mc.weights(C)[[3, 4]]
    calls = []
    real_build = build.build_mix_part
    monkeypatch.setattr(build, "build_mix_part", lambda *a, **k: (calls.append("build_mix_part"), real_build(*a, **k))[1])
    for cls, name in ((engine_module.BatchSweep, "adjoint_parameter"), (engine_module.HipEngine, "_load_mix_part")):
        real = getattr(cls, name)
        monkeypatch.setattr(cls, name, lambda self, *a, _real=real, _name=name, **k: (calls.append(_name),
                                                                                      _real(self, *a, **k))[1])
    plain = prob.evaluate_batch(obj, X, jacobian="exact", parameter_jacobian=True)
    assert plain.adjoint_parameter is None and calls == []
    assert getattr(prob._engine, "mix_part_path", None) is None
    res = prob.evaluate_batch(obj, X, jacobian="exact", parameter_jacobian=True, adjoint_parameter=W)
    assert calls == ["adjoint_parameter", "_load_mix_part", "build_mix_part"]
    assert np.array_equal(res.values, plain.values) and np.array_equal(res.cost, plain.cost)
    assert np.array_equal(res.equality, plain.equality) and np.array_equal(res.inequality, plain.inequality)
    assert np.array_equal(res.parameter_jacobian, plain.parameter_jacobian)
    prob._engine.close()
    prob._engine = prob._batch = None


def test_the_hessian_and_the_adjoint_product_on_the_same_module_keep_their_bits(probe_dir):
    """With the mixed part loaded and used, ``hessian_vector`` and ``adjoint`` of the same handle return the bits of their
    own host probes - what they returned before this part existed."""
    C, eng = _engine("P2U")
    H = hc.case("P2U")                                  # the same program: the Hessian and adjoint tests' view of it
    assert H.header == C.header
    x, theta = C.points[1], C.thetas[1]
    eng.set_parameters(theta)
    W8, V8 = hc.pairs(H)
    eng.adjoint_parameter(x, mc.weights(C))
    hvp = hc.run_probe(H, hc.build_probe(H, probe_dir), probe_dir, x, W8, V8, theta, "keep")
    Q, F0 = eng.hessian_vector(x, W8, V8)
    assert _same(Q, hvp.Q) and _same(F0, hvp.F0)
    G_want, _ = ac.run_probe(H, ac.build_probe(H, probe_dir), probe_dir, x, W8, theta, "keep_adj")
    G, _ = eng.adjoint(x, W8)
    assert _same(G, G_want)
    S, _ = eng.adjoint_parameter(x, mc.weights(C))      # ... and after them the mixed call its own
    assert _same(S, Probe("P2U", probe_dir)(x, mc.weights(C), theta)[0])
    eng.close()
