"""Exact adjoint products ``F'(x)^T w`` on the GPU (``og_adjoint*``, ``HipEngine.adjoint``, ``BatchSweep.adjoint``,
``Problem.adjoint_product``, ``evaluate_batch(adjoints=)``).  The kernels sum the terms of ``csrc/og_adj.h`` in the order
that header fixes, so every comparison is BITWISE against the host probe of that header (tests/adj_probe.cpp, g++), whose
own distance from the twin's ``J^T w`` tests/test_adjoint.py bounds.  Shapes (``adjoint_cases.GPU_KEYS``; their modules,
batch parts and adjoint parts are compiled by ``__graft_entry__.build``): B5 - 5 nodes, every workgroup mostly idle
lanes; G17 - 17 nodes cross the 16-row block of the operand image, parameterised; layout_8 - phases of 65 and 31 nodes,
a second phase's panel offset, 130 variables without a term; P2U - a parameterised module; B90 - 90 nodes, the final
time's 272 terms take a thread through its chain twice; NL2, NL0 - a slot's ``reads`` word at 2 and 3 (every entry of a
state's own block has a dynamics part).  What each shape covers is stated in ``adjoint_cases`` and
checked on the CPU."""

import numpy as np
import pytest

import adjoint_cases as ac
from opengoddard_amd import _native, build, problems
from oracle import np_path

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def probe_dir(tmp_path_factory):
    return str(tmp_path_factory.mktemp("adj_probe_gpu"))


def _engine(key):
    from opengoddard_amd.engine import HipEngine
    C = ac.case(key)
    eng = HipEngine(C.prob, C.obj, program=C.program)
    assert eng.header == C.header
    return C, eng


class Probe:
    """``(G, F0)`` of the host probe at ``(x, W, theta)``, computed once per triple."""

    def __init__(self, key, folder):
        self.case, self.folder = ac.case(key), folder
        self.exe = ac.build_probe(self.case, folder)
        self.known = {}

    def __call__(self, x, W, theta=None):
        W = np.atleast_2d(np.asarray(W, dtype=float))
        at = (np.asarray(x, dtype=float).tobytes(), W.tobytes(), None if theta is None else np.asarray(theta).tobytes())
        if at not in self.known:
            self.known[at] = ac.run_probe(self.case, self.exe, self.folder, x, W, theta, "gpu")
        return self.known[at]


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(torch.device("cuda", 0))


def _same(a, b):
    """bit for bit, the sign of a zero included"""
    return np.array_equal(a, b) and np.array_equal(np.signbit(a), np.signbit(b))


# ------------------------------------------------------------------------------------------------ 1. single point
@pytest.mark.parametrize("key", ac.GPU_KEYS)
def test_a_single_point_equals_the_probe_bit_for_bit(key, probe_dir):
    import torch
    C, eng = _engine(key)
    probe = Probe(key, probe_dir)
    stream = torch.cuda.current_stream().cuda_stream
    W8 = ac.weights(C)                                  # K = 8: one full chunk of weight vectors
    W11 = np.concatenate([W8, W8[[5, 3, 4]]])           # K = 11: a second, partly filled chunk
    three = [2, 3, 6]                                   # all ones, a random vector, the zero vector
    for theta in C.thetas:
        if theta is not None:
            eng.set_parameters(theta)                   # (no rebuild: the same module and part)
        for x in (C.points[0], C.points[-1]):
            want, F_want = probe(x, W8, theta)
            assert _same(F_want, eng.eval_stacked(x))   # F0 is og_eval's
            d_x, d_W = _dev(x), _dev(W11)
            d_G = torch.full((12, eng.n), -7.0, dtype=torch.float64, device=d_x.device)
            d_F = torch.full((eng.m,), -7.0, dtype=torch.float64, device=d_x.device)
            for K, rows in ((8, list(range(8))), (11, list(range(8)) + [5, 3, 4])):
                d_G.fill_(-7.0)
                eng.adjoint_dev(d_x.data_ptr(), K, d_W.data_ptr(), d_G.data_ptr(), d_F.data_ptr(), stream)
                torch.cuda.synchronize()
                G, F0 = d_G.cpu().numpy(), d_F.cpu().numpy()
                assert _same(G[:K], want[rows]) and _same(F0, F_want), (key, theta, K)
                assert np.all(G[K:] == -7.0)            # nothing past K rows
            assert not G[6].any() and not np.signbit(G[6]).any()        # the zero vector: +0.0 everywhere
            # K = 3 and K = 1: vector d of a call with K vectors is the call with that vector alone (F0 is optional)
            d_W3 = _dev(W8[three])
            d_G.fill_(-7.0)
            eng.adjoint_dev(d_x.data_ptr(), 3, d_W3.data_ptr(), d_G.data_ptr(), None, stream)
            torch.cuda.synchronize()
            G = d_G.cpu().numpy()
            assert _same(G[:3], want[three]) and np.all(G[3:] == -7.0), (key, theta)
            for d in (0, 1, 4, 7):
                d_G.fill_(-7.0)
                eng.adjoint_dev(d_x.data_ptr(), 1, d_W[d].data_ptr(), d_G.data_ptr(), None, stream)
                torch.cuda.synchronize()
                one = d_G.cpu().numpy()
                assert _same(one[0], want[d]) and np.all(one[1:] == -7.0), (key, theta, d)
                assert _same(one[0], probe(x, W8[d], theta)[0][0])
            G_h, F_h = eng.adjoint(x, W8)               # the host-pointer form, K = 8 and K = 1
            assert _same(G_h, want) and _same(F_h, F_want)
            G_h, F_h = eng.adjoint(x, W8[3:4])
            assert G_h.shape == (1, eng.n) and _same(G_h[0], want[3]) and _same(F_h, F_want)
    assert eng.adjoint_part_path == build.adjoint_part_path(eng.module_path)
    eng.close()


# ------------------------------------------------------------------------------------------------ 2. batches
@pytest.mark.parametrize("key", ["layout_8", "P2U"])
def test_every_lane_works_at_its_own_point_vector_and_parameters(key, probe_dir):
    import torch
    C, eng = _engine(key)
    probe = Probe(key, probe_dir)
    batch = eng.batch(4)
    X = np.stack([C.points[0], C.points[1], C.points[-1]])
    W = ac.weights(C)[[3, 2, 7]]
    V = C.directions()[[3, 2, 4]]
    TH = None
    if key == "P2U":
        TH = np.stack([C.thetas[0], C.thetas[1], C.thetas[0]])      # lane 1 with a parameter row of its own
        batch.set_parameters(TH)
    theta = (lambda k: None) if TH is None else (lambda k: TH[k])
    stream = torch.cuda.current_stream().cuda_stream
    d_X, d_W = _dev(X), _dev(W)
    for B in (1, 3):                                    # of capacity 4
        d_G = torch.full((4, eng.n), -7.0, dtype=torch.float64, device=d_X.device)
        d_F = torch.full((4, eng.m), -7.0, dtype=torch.float64, device=d_X.device)
        batch.adjoint_dev(B, d_X.data_ptr(), d_W.data_ptr(), d_G.data_ptr(), d_F.data_ptr(), stream)
        torch.cuda.synchronize()
        G, F0 = d_G.cpu().numpy(), d_F.cpu().numpy()
        for k in range(B):
            if TH is not None:
                eng.set_parameters(TH[k])               # (the single-point call at that point and those values ...
            one, F1 = eng.adjoint(X[k], W[k:k + 1])
            if TH is not None:
                batch.set_parameters(TH)                # ... the handle's setter reaches the lanes: theirs again)
            want, F_want = probe(X[k], W[k], theta(k))
            assert _same(one[0], want[0]) and _same(F1, F_want), (key, B, k)
            assert _same(G[k], one[0]) and _same(F0[k], F1), (key, B, k)
        assert np.all(G[B:] == -7.0) and np.all(F0[B:] == -7.0)     # the other lanes' outputs are not touched
    G3, F3 = batch.adjoint(X, W)                        # the host form
    assert _same(G3, G[:3]) and _same(F3, F0[:3])
    G1, _ = batch.adjoint(X, W, count=1)
    assert G1.shape == (1, eng.n) and _same(G1[0], G[0])
    with pytest.raises(ValueError, match="weight vectors for"):
        batch.adjoint(X, W[:1])
    with pytest.raises(ValueError, match="W must have shape"):
        batch.adjoint(X, W[:, :-1])
    eng.close()

    # Problem level: next to jacobian="exact" and directions=, which are bit for bit what they are without the keyword
    prob, obj = C.prob, C.obj
    parameters = None if TH is None else TH
    res = prob.evaluate_batch(obj, X, jacobian="exact", parameters=parameters, directions=V, adjoints=W)
    plain = prob.evaluate_batch(obj, X, jacobian="exact", parameters=parameters, directions=V)
    assert plain.adjoint is None and res.adjoint.shape == (3, eng.n)
    assert np.array_equal(res.values, plain.values) and np.array_equal(res.cost, plain.cost)
    assert np.array_equal(res.equality, plain.equality) and np.array_equal(res.gradient, plain.gradient)
    assert np.array_equal(res.directional, plain.directional)
    for k in range(3):
        assert _same(res.adjoint[k], probe(X[k], W[k], theta(k))[0][0])
    # w = e_0 is the gradient of the cost: the exact Jacobian's column, entry by entry
    e0 = np.zeros((3, eng.m))
    e0[:, 0] = 1.0
    cost = prob.evaluate_batch(obj, X, jacobian="exact", parameters=parameters, adjoints=e0)
    assert np.array_equal(cost.adjoint, cost.gradient)
    only = prob.evaluate_batch(obj, X, parameters=parameters, adjoints=W)
    assert _same(only.adjoint, res.adjoint) and np.array_equal(only.cost, res.cost)
    prob._engine.close()
    prob._engine = prob._batch = None


# ------------------------------------------------------------------------------------------------ 3. a captured graph
def test_a_captured_graph_replays_on_another_point_and_other_vectors(probe_dir):
    import torch
    key = "G17"
    C, eng = _engine(key)
    probe = Probe(key, probe_dir)
    dev = torch.device("cuda", 0)
    W = ac.weights(C)
    d_x = torch.zeros(eng.n, dtype=torch.float64, device=dev)
    d_W = torch.zeros((3, eng.m), dtype=torch.float64, device=dev)
    d_G = torch.full((3, eng.n), -7.0, dtype=torch.float64, device=dev)
    d_F = torch.full((eng.m,), -7.0, dtype=torch.float64, device=dev)

    def call(stream):                                   # a linear capture: no parallel branches
        eng.adjoint_dev(d_x.data_ptr(), 3, d_W.data_ptr(), d_G.data_ptr(), d_F.data_ptr(), stream)

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
    for x, rows in ((C.points[1], [3, 4, 5]), (C.points[-1], [5, 7, 3])):
        d_x.copy_(torch.from_numpy(x))
        d_W.copy_(torch.from_numpy(W[rows]))
        d_G.fill_(-7.0)
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        replayed, F_replayed = d_G.cpu().numpy(), d_F.cpu().numpy()
        direct, F_direct = eng.adjoint(x, W[rows])
        want, F_want = probe(x, W[rows], C.thetas[0])
        assert _same(replayed, direct) and _same(F_replayed, F_direct)
        assert _same(replayed, want) and _same(F_replayed, F_want)
    eng.close()


# ------------------------------------------------------------------------------------------------ 4. errors, bookkeeping
def test_errors_before_the_load_and_for_no_vector():
    lib = _native.lib()
    C, eng = _engine("B5")
    x, W = C.points[0], ac.weights(C)[:2]
    G, F0 = np.empty((2, eng.n)), np.empty(eng.m)
    # before the load: 4
    assert lib.og_adjoint(eng._handle, _native.dptr(x), 2, _native.dptr(W), _native.dptr(G), _native.dptr(F0)) == 4
    assert b"og_adjoint_load" in lib.og_last_error()
    assert lib.og_adjoint_dev(eng._handle, 8, 1, 8, 8, None, None) == 4
    assert lib.og_adjoint_load(eng._handle, None) == 4
    assert lib.og_adjoint_load(eng._handle, b"/nonexistent/part.so") == 4
    # another module's part, and other parts of this module: 5
    other = build.build_adjoint_part(ac.case("G17").header)
    assert lib.og_adjoint_load(eng._handle, other.encode()) == 5
    assert b"does not belong" in lib.og_last_error()
    batch = eng.batch(2)                                # (its batch part exports the batched entry name too)
    assert lib.og_adjoint_load(eng._handle, build.batch_part_path(eng.module_path).encode()) == 5
    assert lib.og_adjoint_load(eng._handle, build.build_directional_part(eng.header).encode()) == 5
    X = np.stack([x, x])
    assert lib.og_adjoint_batch(batch._handle, 2, _native.dptr(X), _native.dptr(W), None, _native.dptr(G)) == 4
    eng._load_adjoint_part()
    assert lib.og_adjoint_load(eng._handle, None) == 0              # loaded: a no-op
    # k = 0, a negative k, k past 65535, null pointers, a count out of range: 1 and a message
    assert lib.og_adjoint(eng._handle, _native.dptr(x), 0, _native.dptr(W), _native.dptr(G), None) == 1
    assert b"k must be at least 1" in lib.og_last_error()
    assert lib.og_adjoint_dev(eng._handle, 8, 0, 8, 8, None, None) == 1
    assert lib.og_adjoint_dev(eng._handle, 8, -3, 8, 8, None, None) == 1
    assert lib.og_adjoint_dev(eng._handle, 8, 65536, 8, 8, None, None) == 1
    assert b"exceeds 65535" in lib.og_last_error()
    assert lib.og_adjoint_dev(eng._handle, 8, 1, None, 8, None, None) == 1
    assert lib.og_adjoint(eng._handle, _native.dptr(x), 2, None, _native.dptr(G), None) == 1
    assert b"null argument" in lib.og_last_error()
    assert lib.og_adjoint_batch(batch._handle, 0, _native.dptr(X), _native.dptr(W), None, _native.dptr(G)) == 1
    assert lib.og_adjoint_batch(batch._handle, 3, _native.dptr(X), _native.dptr(W), None, _native.dptr(G)) == 1
    assert b"capacity" in lib.og_last_error()
    assert lib.og_adjoint_batch_dev(batch._handle, 2, 8, None, None, 8, None) == 1
    with pytest.raises(ValueError, match="weights must have shape"):
        eng.adjoint(x, W[:, :-1])
    # and the good call still works
    assert lib.og_adjoint(eng._handle, _native.dptr(x), 2, _native.dptr(W), _native.dptr(G), None) == 0
    assert np.all(np.isfinite(G))
    eng.close()


def test_no_state_word_moves(probe_dir):
    """An FD sweep into a registered buffer gives the bits it gave before an adjoint call (single point and batch) came
    between: the call counts no launch into the buffer's words and leaves the buffer and its structural zeros alone."""
    import torch
    key = "layout_8"
    C, eng = _engine(key)
    probe = Probe(key, probe_dir)
    lb, ub = np_path.bounds_arrays(C.prob)
    xa, xb = C.points[1], C.points[-1]
    ha, hb = _native.fd_step(xa, lb, ub), _native.fd_step(xb, lb, ub)
    W = ac.weights(C)[[3, 4]]
    stream = torch.cuda.current_stream().cuda_stream
    dev = torch.device("cuda", 0)
    d_JT = torch.full((eng.n, eng.m), -7.0, dtype=torch.float64, device=dev)
    d_F = torch.zeros(eng.m, dtype=torch.float64, device=dev)
    d_G = torch.zeros((2, eng.n), dtype=torch.float64, device=dev)
    eng.register_jt_dev(d_JT.data_ptr(), 0, eng.n, stream)

    def sweep(x, h):
        d_x, d_h = _dev(x), _dev(h)
        eng.sweep_dev(d_x.data_ptr(), d_h.data_ptr(), 0, eng.n, d_JT.data_ptr(), d_F.data_ptr(), stream)
        torch.cuda.synchronize()
        return d_JT.cpu().numpy(), d_F.cpu().numpy()

    def adjoint(x):
        d_x, d_W = _dev(x), _dev(W)
        eng.adjoint_dev(d_x.data_ptr(), 2, d_W.data_ptr(), d_G.data_ptr(), None, stream)
        torch.cuda.synchronize()
        return d_G.cpu().numpy()

    JT_a, F_a = sweep(xa, ha)
    JT_b, F_b = sweep(xb, hb)
    assert not np.array_equal(JT_a, JT_b) and np.count_nonzero(JT_b) <= eng.pattern()[0][-1]
    again, F_again = sweep(xa, ha)
    assert np.array_equal(again, JT_a) and np.array_equal(F_again, F_a)
    assert _same(adjoint(xb), probe(xb, W)[0])
    assert np.array_equal(d_JT.cpu().numpy(), JT_a)                 # the buffer is where the sweep left it
    after, F_after = sweep(xb, hb)
    assert np.array_equal(after, JT_b) and np.array_equal(F_after, F_b)
    assert _same(adjoint(xa), probe(xa, W)[0])
    after, F_after = sweep(xa, ha)
    assert np.array_equal(after, JT_a) and np.array_equal(F_after, F_a)
    eng.unregister_jt_dev(d_JT.data_ptr())
    # the lanes of a batch: their own registered matrices
    batch = eng.batch(2)
    X, H = np.stack([xa, xb]), np.stack([ha, hb])
    batch.sweep(X, H)
    dense = [batch.dense(k).copy() for k in range(2)]
    assert np.array_equal(dense[0], JT_a) and np.array_equal(dense[1], JT_b)
    G, _ = batch.adjoint(X[::-1].copy(), W)
    assert _same(G[0], probe(xb, W[0])[0][0]) and _same(G[1], probe(xa, W[1])[0][0])
    assert all(np.array_equal(batch.dense(k), dense[k]) for k in range(2))
    batch.sweep(X, H)
    assert all(np.array_equal(batch.dense(k), dense[k]) for k in range(2))
    eng.close()


def test_without_the_keyword_nothing_of_the_feature_runs(monkeypatch):
    """``evaluate_batch(adjoints=None)``: the adjoint part is neither built nor loaded and no adjoint entry point of the
    library is called - without the part there is no kernel that could be launched - and every result is bit for bit
    what the call with the keyword returns next to the adjoint."""
    from opengoddard_amd import engine as engine_module
    C = ac.case("P2U")
    prob, obj = C.prob, C.obj
    X = np.stack([C.points[0], C.points[1]])
    W = ac.weights(C)[[3, 4]]
    calls = []
    for name in ("build_adjoint_part",):
        real = getattr(build, name)
        monkeypatch.setattr(build, name, lambda *a, _real=real, _name=name, **k: (calls.append(_name), _real(*a, **k))[1])
    for cls, name in ((engine_module.BatchSweep, "adjoint"), (engine_module.HipEngine, "_load_adjoint_part")):
        real = getattr(cls, name)
        monkeypatch.setattr(cls, name, lambda self, *a, _real=real, _name=name, **k: (calls.append(_name),
                                                                                      _real(self, *a, **k))[1])
    plain = prob.evaluate_batch(obj, X, jacobian="exact")
    assert plain.adjoint is None and calls == []
    assert getattr(prob._engine, "adjoint_part_path", None) is None
    res = prob.evaluate_batch(obj, X, jacobian="exact", adjoints=W)
    assert calls == ["adjoint", "_load_adjoint_part", "build_adjoint_part"]
    assert np.array_equal(res.values, plain.values) and np.array_equal(res.cost, plain.cost)
    assert np.array_equal(res.equality, plain.equality) and np.array_equal(res.inequality, plain.inequality)
    again = prob.evaluate_batch(obj, X, jacobian="exact")
    assert again.adjoint is None and len(calls) == 3 and np.array_equal(again.values, plain.values)
    prob._engine.close()
    prob._engine = prob._batch = None


# ------------------------------------------------------------------------------------------------ 5. Problem level
def test_adjoint_product_end_to_end():
    prob, obj = problems.build("brachistochrone")
    C = ac.case("brachistochrone")
    W = ac.weights(C)
    got = prob.adjoint_product(obj, W)                  # at prob.p
    assert got.shape == (8, C.n) and getattr(prob, "_batch", None) is None
    F0, JT = prob._engine.exact_stacked(np.asarray(prob.p, dtype=float))
    prod, scale = ac.twin_adjoint(JT, W)
    assert ac.worst_error(got, prod, scale) <= ac.BOUND
    assert np.array_equal(got[0], JT[:, 0])             # the gradient of the cost
    one = prob.adjoint_product(obj, W[3])
    assert one.shape == (C.n,) and _same(one, got[3])
    # with the directional derivative: one operator and its transpose
    V = C.directions()[3:6]
    dF = prob.directional_derivative(obj, V)
    left = W.astype(np.longdouble) @ dF.astype(np.longdouble).T
    right = got.astype(np.longdouble) @ V.astype(np.longdouble).T
    bound = 1e-12 * (np.abs(W).astype(np.longdouble) @ np.abs(JT).astype(np.longdouble).T @ np.abs(V).astype(np.longdouble).T)
    assert np.all(np.abs(left - right) <= bound)
    with pytest.raises(ValueError, match="weights must have"):
        prob.adjoint_product(obj, W[3][:-1])
    prob._engine.close()
