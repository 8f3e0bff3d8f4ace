"""Exact Hessian-vector products ``grad^2 (w . F)(x) v`` on the GPU (``og_hessian_vector*``, ``HipEngine.hessian_vector``,
``BatchSweep.hessian_vector``, ``Problem.hessian_vector_product``, ``evaluate_batch(hessian_products=)``).  The kernels sum
the terms of ``csrc/og_hvp.h`` in the order ``csrc/og_adj.h`` fixes, so every comparison is BITWISE against the host probe
of those headers (tests/hvp_probe.cpp, g++), whose own distance from an independent reference tests/test_hessian.py
bounds.  Shapes (``hessian_cases.GPU_KEYS``, the adjoint test's seven; their modules, batch parts and Hessian parts are
compiled by ``__graft_entry__.build``): B5 - 5 nodes, light columns only; G17 - 17 nodes, parameterised, one heavy
column; layout_8 - two phases, 130 variables without a term, two heavy columns; P2U - a parameterised module; B90 - 90
nodes, the final time is heavy and its 272 terms take a thread through its chain twice.  tests/test_hessian.py checks on
the CPU that the shapes contain these."""

import numpy as np
import pytest

import hessian_cases as hc
from opengoddard_amd import _native, build, problems
from oracle import np_path

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def probe_dir(tmp_path_factory):
    return str(tmp_path_factory.mktemp("hvp_probe_gpu"))


def _engine(key):
    from opengoddard_amd.engine import HipEngine
    C = hc.case(key)
    eng = HipEngine(C.prob, C.obj, program=C.program)
    assert eng.header == C.header
    return C, eng


class Probe:
    """``(Q, F0)`` of the host probe at ``(x, W, V, theta)``, computed once per argument set."""

    def __init__(self, key, folder):
        self.case, self.folder = hc.case(key), folder
        self.exe = hc.build_probe(self.case, folder)
        self.known = {}

    def __call__(self, x, W, V, theta=None):
        W, V = np.atleast_2d(np.asarray(W, dtype=float)), np.atleast_2d(np.asarray(V, dtype=float))
        at = (np.asarray(x, dtype=float).tobytes(), W.tobytes(), V.tobytes(),
              None if theta is None else np.asarray(theta).tobytes())
        if at not in self.known:
            r = hc.run_probe(self.case, self.exe, self.folder, x, W, V, theta, "gpu")
            self.known[at] = (r.Q, r.F0)
        return self.known[at]


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(torch.device("cuda", 0))


def _same(a, b):
    """bit for bit, the sign of a zero included"""
    return np.array_equal(a, b) and np.array_equal(np.signbit(a), np.signbit(b))


# ------------------------------------------------------------------------------------------------ 1. single point
@pytest.mark.parametrize("key", hc.GPU_KEYS)
def test_a_single_point_equals_the_probe_bit_for_bit(key, probe_dir):
    import torch
    C, eng = _engine(key)
    probe = Probe(key, probe_dir)
    stream = torch.cuda.current_stream().cuda_stream
    W8, V8 = hc.pairs(C)
    rows9 = list(range(8)) + [2]                        # K = 9
    three = [2, 4, 6]                                   # all ones with a random direction, the final time, the zero pair
    theta, x = C.thetas[-1], C.points[-1]
    if theta is not None:
        eng.set_parameters(theta)                       # (no rebuild: the same module and part)
    want, F_want = probe(x, W8, V8, theta)
    assert _same(F_want, eng.eval_stacked(x))           # F0 is og_eval's
    d_x, d_W, d_V = _dev(x), _dev(W8[rows9]), _dev(V8[rows9])
    d_Q = torch.full((10, eng.n), -7.0, dtype=torch.float64, device=d_x.device)
    d_F = torch.full((eng.m,), -7.0, dtype=torch.float64, device=d_x.device)
    eng.hessian_vector_dev(d_x.data_ptr(), 9, d_W.data_ptr(), d_V.data_ptr(), d_Q.data_ptr(), d_F.data_ptr(), stream)
    torch.cuda.synchronize()
    Q, F0 = d_Q.cpu().numpy(), d_F.cpu().numpy()
    assert _same(Q[:9], want[rows9]) and _same(F0, F_want), key
    assert np.all(Q[9:] == -7.0)                        # nothing past K rows
    assert not Q[6].any() and not np.signbit(Q[6]).any()            # the zero pair: +0.0 everywhere
    # K = 3 and K = 1: pair d of a call with K pairs is the call with that pair alone (F0 is optional)
    d_W3, d_V3 = _dev(W8[three]), _dev(V8[three])
    d_Q.fill_(-7.0)
    eng.hessian_vector_dev(d_x.data_ptr(), 3, d_W3.data_ptr(), d_V3.data_ptr(), d_Q.data_ptr(), None, stream)
    torch.cuda.synchronize()
    Q = d_Q.cpu().numpy()
    assert _same(Q[:3], want[three]) and np.all(Q[3:] == -7.0), key
    for d in (0, 5, 7):
        d_Q.fill_(-7.0)
        eng.hessian_vector_dev(d_x.data_ptr(), 1, d_W[d].data_ptr(), d_V[d].data_ptr(), d_Q.data_ptr(), None, stream)
        torch.cuda.synchronize()
        one = d_Q.cpu().numpy()
        assert _same(one[0], want[d]) and np.all(one[1:] == -7.0), (key, d)
    Q_h, F_h = eng.hessian_vector(x, W8, V8)            # the host-pointer form, K = 8 and K = 1
    assert _same(Q_h, want) and _same(F_h, F_want)
    Q_h, F_h = eng.hessian_vector(x, W8[3:4], V8[3:4])
    assert Q_h.shape == (1, eng.n) and _same(Q_h[0], want[3]) and _same(F_h, F_want)
    assert eng.hessian_part_path == build.hessian_part_path(eng.module_path)
    eng.close()


# ------------------------------------------------------------------------------------------------ 2. batches
@pytest.mark.parametrize("key", ["layout_8", "P2U"])
def test_every_lane_works_at_its_own_point_pair_and_parameters(key, probe_dir):
    import torch
    C, eng = _engine(key)
    probe = Probe(key, probe_dir)
    batch = eng.batch(4)
    X = np.stack([C.points[0], C.points[1], C.points[-1]])
    W8, V8 = hc.pairs(C)
    W, V = W8[[3, 2, 7]], V8[[0, 2, 4]]
    TH = None
    if key == "P2U":
        TH = np.stack([C.thetas[0], C.thetas[1], C.thetas[0]])      # lane 1 with a parameter row of its own
        batch.set_parameters(TH)
    theta = (lambda k: None) if TH is None else (lambda k: TH[k])
    stream = torch.cuda.current_stream().cuda_stream
    d_X, d_W, d_V = _dev(X), _dev(W), _dev(V)
    for B in (1, 3):                                    # of capacity 4
        d_Q = torch.full((4, eng.n), -7.0, dtype=torch.float64, device=d_X.device)
        d_F = torch.full((4, eng.m), -7.0, dtype=torch.float64, device=d_X.device)
        batch.hessian_vector_dev(B, d_X.data_ptr(), d_W.data_ptr(), d_V.data_ptr(), d_Q.data_ptr(), d_F.data_ptr(), stream)
        torch.cuda.synchronize()
        Q, F0 = d_Q.cpu().numpy(), d_F.cpu().numpy()
        for k in range(B):
            if TH is not None:
                eng.set_parameters(TH[k])               # (the single-point call at that point and those values ...
            one, F1 = eng.hessian_vector(X[k], W[k:k + 1], V[k:k + 1])
            if TH is not None:
                batch.set_parameters(TH)                # ... the handle's setter reaches the lanes: theirs again)
            want, F_want = probe(X[k], W[k], V[k], theta(k))
            assert _same(one[0], want[0]) and _same(F1, F_want), (key, B, k)
            assert _same(Q[k], one[0]) and _same(F0[k], F1), (key, B, k)
        assert np.all(Q[B:] == -7.0) and np.all(F0[B:] == -7.0)     # the other lanes' outputs are not touched
    Q3, F3 = batch.hessian_vector(X, W, V)              # the host form
    assert _same(Q3, Q[:3]) and _same(F3, F0[:3])
    Q1, _ = batch.hessian_vector(X, W, V, count=1)
    assert Q1.shape == (1, eng.n) and _same(Q1[0], Q[0])
    with pytest.raises(ValueError, match="weight vectors for"):
        batch.hessian_vector(X, W[:1], V)
    with pytest.raises(ValueError, match="V must have shape"):
        batch.hessian_vector(X, W, V[:, :-1])
    eng.close()

    # Problem level: next to jacobian="exact" and adjoints=, which are bit for bit what they are without the keyword
    prob, obj = C.prob, C.obj
    res = prob.evaluate_batch(obj, X, jacobian="exact", parameters=TH, adjoints=W, hessian_products=(W, V))
    plain = prob.evaluate_batch(obj, X, jacobian="exact", parameters=TH, adjoints=W)
    assert plain.hessian_product is None and res.hessian_product.shape == (3, eng.n)
    assert np.array_equal(res.values, plain.values) and np.array_equal(res.cost, plain.cost)
    assert np.array_equal(res.equality, plain.equality) and np.array_equal(res.adjoint, plain.adjoint)
    for k in range(3):
        assert _same(res.hessian_product[k], probe(X[k], W[k], V[k], theta(k))[0][0])
    prob._engine.close()
    prob._engine = prob._batch = None


# ------------------------------------------------------------------------------------------------ 3. a captured graph
def test_a_captured_graph_replays_on_another_point_and_other_pairs(probe_dir):
    import torch
    key = "G17"
    C, eng = _engine(key)
    probe = Probe(key, probe_dir)
    dev = torch.device("cuda", 0)
    W, V = hc.pairs(C)
    d_x = torch.zeros(eng.n, dtype=torch.float64, device=dev)
    d_W = torch.zeros((3, eng.m), dtype=torch.float64, device=dev)
    d_V = torch.zeros((3, eng.n), dtype=torch.float64, device=dev)
    d_Q = torch.full((3, eng.n), -7.0, dtype=torch.float64, device=dev)
    d_F = torch.full((eng.m,), -7.0, dtype=torch.float64, device=dev)

    def call(stream):                                   # a linear capture: no parallel branches
        eng.hessian_vector_dev(d_x.data_ptr(), 3, d_W.data_ptr(), d_V.data_ptr(), d_Q.data_ptr(), d_F.data_ptr(), stream)

    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        d_x.copy_(torch.from_numpy(C.points[0]))
        d_W.copy_(torch.from_numpy(W[[0, 1, 2]]))
        d_V.copy_(torch.from_numpy(V[[0, 1, 2]]))
        call(side.cuda_stream)                          # warm: the part is built and loaded outside the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        call(torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    for x, rows in ((C.points[1], [3, 4, 5]), (C.points[-1], [5, 7, 2])):
        d_x.copy_(torch.from_numpy(x))
        d_W.copy_(torch.from_numpy(W[rows]))
        d_V.copy_(torch.from_numpy(V[rows]))
        d_Q.fill_(-7.0)
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        replayed, F_replayed = d_Q.cpu().numpy(), d_F.cpu().numpy()
        want, F_want = probe(x, W[rows], V[rows], C.thetas[0])
        assert _same(replayed, want) and _same(F_replayed, F_want)
    eng.close()


# ------------------------------------------------------------------------------------------------ 4. errors, bookkeeping
def test_errors_before_the_load_and_for_no_pair():
    lib = _native.lib()
    C, eng = _engine("B5")
    W8, V8 = hc.pairs(C)
    x, W, V = C.points[0], W8[:2].copy(), V8[:2].copy()
    Q, F0 = np.empty((2, eng.n)), np.empty(eng.m)
    dp = _native.dptr
    # before the load: 4
    assert lib.og_hessian_vector(eng._handle, dp(x), 2, dp(W), dp(V), dp(Q), dp(F0)) == 4
    assert b"og_hessian_vector_load" in lib.og_last_error()
    assert lib.og_hessian_vector_dev(eng._handle, 8, 1, 8, 8, 8, None, None) == 4
    assert lib.og_hessian_vector_load(eng._handle, None) == 4
    assert lib.og_hessian_vector_load(eng._handle, b"/nonexistent/part.so") == 4
    # another module's part, and another part of this module: 5
    other = build.build_hessian_part(hc.case("G17").header)
    assert lib.og_hessian_vector_load(eng._handle, other.encode()) == 5
    assert b"does not belong" in lib.og_last_error()
    assert lib.og_hessian_vector_load(eng._handle, build.build_adjoint_part(eng.header).encode()) == 5
    batch = eng.batch(2)
    X = np.stack([x, x])
    assert lib.og_hessian_vector_batch(batch._handle, 2, dp(X), dp(W), dp(V), None, dp(Q)) == 4
    eng._load_hessian_part()
    assert lib.og_hessian_vector_load(eng._handle, None) == 0       # loaded: a no-op
    # k = 0, a negative k, k past 65535, null pointers, a count out of range: 1 and a message
    assert lib.og_hessian_vector(eng._handle, dp(x), 0, dp(W), dp(V), dp(Q), None) == 1
    assert b"k must be at least 1" in lib.og_last_error()
    assert lib.og_hessian_vector_dev(eng._handle, 8, -3, 8, 8, 8, None, None) == 1
    assert lib.og_hessian_vector_dev(eng._handle, 8, 65536, 8, 8, 8, None, None) == 1
    assert b"exceeds 65535" in lib.og_last_error()
    assert lib.og_hessian_vector_dev(eng._handle, 8, 1, 8, None, 8, None, None) == 1
    assert lib.og_hessian_vector(eng._handle, dp(x), 2, None, dp(V), dp(Q), None) == 1
    assert b"null argument" in lib.og_last_error()
    assert lib.og_hessian_vector_batch(batch._handle, 0, dp(X), dp(W), dp(V), None, dp(Q)) == 1
    assert lib.og_hessian_vector_batch(batch._handle, 3, dp(X), dp(W), dp(V), None, dp(Q)) == 1
    assert b"capacity" in lib.og_last_error()
    assert lib.og_hessian_vector_batch_dev(batch._handle, 2, 8, 8, None, None, 8, None) == 1
    with pytest.raises(ValueError, match="weights must have shape"):
        eng.hessian_vector(x, W[:, :-1], V)
    with pytest.raises(ValueError, match="directions must have shape"):
        eng.hessian_vector(x, W, V[:1])
    # and the good call still works
    assert lib.og_hessian_vector(eng._handle, dp(x), 2, dp(W), dp(V), dp(Q), None) == 0
    assert np.all(np.isfinite(Q))
    eng.close()


def test_no_state_word_moves(probe_dir):
    """An FD sweep into a registered buffer gives the bits it gave before a Hessian-vector call (single point and batch)
    came between: the call counts no launch into the buffer's words and leaves the buffer alone."""
    import torch
    key = "layout_8"
    C, eng = _engine(key)
    probe = Probe(key, probe_dir)
    lb, ub = np_path.bounds_arrays(C.prob)
    xa, xb = C.points[1], C.points[-1]
    ha, hb = _native.fd_step(xa, lb, ub), _native.fd_step(xb, lb, ub)
    W8, V8 = hc.pairs(C)
    W, V = W8[[3, 4]], V8[[0, 1]]
    stream = torch.cuda.current_stream().cuda_stream
    dev = torch.device("cuda", 0)
    d_JT = torch.full((eng.n, eng.m), -7.0, dtype=torch.float64, device=dev)
    d_F = torch.zeros(eng.m, dtype=torch.float64, device=dev)
    d_Q = torch.zeros((2, eng.n), dtype=torch.float64, device=dev)
    eng.register_jt_dev(d_JT.data_ptr(), 0, eng.n, stream)

    def sweep(x, h):
        d_x, d_h = _dev(x), _dev(h)
        eng.sweep_dev(d_x.data_ptr(), d_h.data_ptr(), 0, eng.n, d_JT.data_ptr(), d_F.data_ptr(), stream)
        torch.cuda.synchronize()
        return d_JT.cpu().numpy(), d_F.cpu().numpy()

    def product(x):
        d_x, d_W, d_V = _dev(x), _dev(W), _dev(V)
        eng.hessian_vector_dev(d_x.data_ptr(), 2, d_W.data_ptr(), d_V.data_ptr(), d_Q.data_ptr(), None, stream)
        torch.cuda.synchronize()
        return d_Q.cpu().numpy()

    JT_a, F_a = sweep(xa, ha)
    JT_b, F_b = sweep(xb, hb)
    again, F_again = sweep(xa, ha)
    assert not np.array_equal(JT_a, JT_b) and np.array_equal(again, JT_a) and np.array_equal(F_again, F_a)
    assert _same(product(xb), probe(xb, W, V)[0])
    assert np.array_equal(d_JT.cpu().numpy(), JT_a)                 # the buffer is where the sweep left it
    after, F_after = sweep(xb, hb)
    assert np.array_equal(after, JT_b) and np.array_equal(F_after, F_b)
    assert _same(product(xa), probe(xa, W, V)[0])
    after, F_after = sweep(xa, ha)
    assert np.array_equal(after, JT_a) and np.array_equal(F_after, F_a)
    eng.unregister_jt_dev(d_JT.data_ptr())
    # the lanes of a batch: their own registered matrices
    batch = eng.batch(2)
    X, H = np.stack([xa, xb]), np.stack([ha, hb])
    batch.sweep(X, H)
    dense = [batch.dense(k).copy() for k in range(2)]
    assert np.array_equal(dense[0], JT_a) and np.array_equal(dense[1], JT_b)
    Q, F0 = batch.hessian_vector(X[::-1].copy(), W, V)
    assert _same(Q[0], probe(xb, W[0], V[0])[0][0]) and _same(Q[1], probe(xa, W[1], V[1])[0][0])
    assert _same(F0[0], eng.eval_stacked(xb))                       # F0 is the evaluation's
    assert all(np.array_equal(batch.dense(k), dense[k]) for k in range(2))
    batch.sweep(X, H)
    assert all(np.array_equal(batch.dense(k), dense[k]) for k in range(2))
    eng.close()


def test_without_the_keyword_nothing_of_the_feature_runs(monkeypatch):
    """``evaluate_batch(hessian_products=None)``: the Hessian part is neither built nor loaded and no entry point of the
    feature is called, and every result is bit for bit what the call with the keyword returns next to the product."""
    from opengoddard_amd import engine as engine_module
    C = hc.case("P2U")
    prob, obj = C.prob, C.obj
    X = np.stack([C.points[0], C.points[1]])
    W8, V8 = hc.pairs(C)
    W, V = W8[[3, 4]], V8[[0, 1]]
    calls = []
    real_build = build.build_hessian_part
    monkeypatch.setattr(build, "build_hessian_part", lambda *a, **k: (calls.append("build_hessian_part"), real_build(*a, **k))[1])
    for cls, name in ((engine_module.BatchSweep, "hessian_vector"), (engine_module.HipEngine, "_load_hessian_part")):
        real = getattr(cls, name)
        monkeypatch.setattr(cls, name, lambda self, *a, _real=real, _name=name, **k: (calls.append(_name),
                                                                                      _real(self, *a, **k))[1])
    plain = prob.evaluate_batch(obj, X, jacobian="exact")
    assert plain.hessian_product is None and calls == []
    assert getattr(prob._engine, "hessian_part_path", None) is None
    res = prob.evaluate_batch(obj, X, jacobian="exact", hessian_products=(W, V))
    assert calls == ["hessian_vector", "_load_hessian_part", "build_hessian_part"]
    assert np.array_equal(res.values, plain.values) and np.array_equal(res.cost, plain.cost)
    assert np.array_equal(res.equality, plain.equality) and np.array_equal(res.inequality, plain.inequality)
    prob._engine.close()
    prob._engine = prob._batch = None


# ------------------------------------------------------------------------------------------------ 5. Problem level
def test_hessian_vector_product_end_to_end():
    prob, obj = problems.build("brachistochrone")
    C = hc.case("brachistochrone")
    W8, V8 = hc.pairs(C)
    x = np.asarray(prob.p, dtype=float)
    got = prob.hessian_vector_product(obj, W8, V8)      # at prob.p
    assert got.shape == (8, C.n) and getattr(prob, "_batch", None) is None
    direct, _ = prob._engine.hessian_vector(x, W8, V8)
    assert _same(got, direct)
    many = prob.hessian_vector_product(obj, W8[3], V8[:3])          # one weight vector, three directions
    direct, _ = prob._engine.hessian_vector(x, np.tile(W8[3], (3, 1)), V8[:3])
    assert many.shape == (3, C.n) and _same(many, direct) and many.any()
    one = prob.hessian_vector_product(obj, W8[3], V8[1])
    assert one.shape == (C.n,) and _same(one, many[1])
    with pytest.raises(ValueError, match="weights must have"):
        prob.hessian_vector_product(obj, W8[3][:-1], V8[1])
    prob._engine.close()
