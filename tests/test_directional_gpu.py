"""Exact directional derivatives ``F'(x) v`` on the GPU (``og_directional*``, ``HipEngine.directional``,
``BatchSweep.directional``, ``Problem.directional_derivative``, ``evaluate_batch(directions=)``).  The kernels compute
every entry with ``og_dir_entry`` (csrc/og_dir.h), so every comparison is BITWISE against the host probe of that function
(tests/dir_probe.cpp, g++), whose own distance from the complex step and from the twin's ``J v``
tests/test_directional.py bounds.  Shapes (``directional_cases.GPU_KEYS``; their modules, batch parts and directional
parts are compiled by ``__graft_entry__.build``): B5 - one phase of 5 nodes, N no multiple of 4, one partly filled
workgroup; G17 - 17 nodes cross the 16-row block of the operand image; layout_8 - phases of 65 and 31 nodes, a second
phase's panel offset, 423 entries: a second workgroup, ragged; P2U - a parameterised module; NL2, NL0 - dynamics that
read a state across the nodes of its phase (``nonlocal_cases``)."""

import numpy as np
import pytest

import directional_cases as dc
from opengoddard_amd import _native, build, problems
from oracle import np_path

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def probe_dir(tmp_path_factory):
    return str(tmp_path_factory.mktemp("dir_probe_gpu"))


def _engine(key):
    from opengoddard_amd.engine import HipEngine
    C = dc.case(key)
    eng = HipEngine(C.prob, C.obj, program=C.program)
    assert eng.header == C.header
    return C, eng


class Probe:
    """``(dF, F0)`` of the host probe at ``(x, V, theta)``, computed once per triple."""

    def __init__(self, key, folder):
        self.case, self.folder = dc.case(key), folder
        self.exe = dc.build_probe(self.case, folder)
        self.known = {}

    def __call__(self, x, V, theta=None):
        V = np.atleast_2d(np.asarray(V, dtype=float))
        at = (np.asarray(x, dtype=float).tobytes(), V.tobytes(), None if theta is None else np.asarray(theta).tobytes())
        if at not in self.known:
            self.known[at] = dc.run_probe(self.case, self.exe, self.folder, x, V, theta, "gpu")
        return self.known[at]


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(torch.device("cuda", 0))


# ------------------------------------------------------------------------------------------------ 1. single point
@pytest.mark.parametrize("key", dc.GPU_KEYS)
def test_a_single_point_equals_the_probe_bit_for_bit(key, probe_dir):
    import torch
    C, eng = _engine(key)
    probe = Probe(key, probe_dir)
    stream = torch.cuda.current_stream().cuda_stream
    V3 = C.directions()[[2, 3, 6]]                      # a final time, a random vector, the zero vector
    for theta in C.thetas:
        if theta is not None:
            eng.set_parameters(theta)                   # (no rebuild: the same module and part)
        for x in (C.points[0], C.points[-1]):
            want, F_want = probe(x, V3, theta)
            d_x, d_V = _dev(x), _dev(V3)
            d_dF = torch.full((4, eng.m), -7.0, dtype=torch.float64, device=d_x.device)
            d_F = torch.full((eng.m,), -7.0, dtype=torch.float64, device=d_x.device)
            eng.directional_dev(d_x.data_ptr(), 3, d_V.data_ptr(), d_dF.data_ptr(), d_F.data_ptr(), stream)
            torch.cuda.synchronize()
            dF, F0 = d_dF.cpu().numpy(), d_F.cpu().numpy()
            assert np.array_equal(dF[:3], want) and np.array_equal(F0, F_want), (key, theta)
            assert np.all(dF[3] == -7.0) and not dF[2].any()        # nothing past K rows; the zero direction
            # K = 1: direction d of the K = 3 call is the call on that direction alone (and F0 is optional)
            for d in range(3):
                d_dF.fill_(-7.0)
                eng.directional_dev(d_x.data_ptr(), 1, d_V[d].data_ptr(), d_dF.data_ptr(), None, stream)
                torch.cuda.synchronize()
                one = d_dF.cpu().numpy()
                assert np.array_equal(one[0], want[d]) and np.all(one[1:] == -7.0), (key, theta, d)
                assert np.array_equal(one[0], probe(x, V3[d], theta)[0][0])
            dF_h, F_h = eng.directional(x, V3)          # the host-pointer form, K = 3 and K = 1
            assert np.array_equal(dF_h, want) and np.array_equal(F_h, F_want)
            dF_h, F_h = eng.directional(x, V3[1:2])
            assert dF_h.shape == (1, eng.m) and np.array_equal(dF_h[0], want[1]) and np.array_equal(F_h, F_want)
    assert eng.directional_part_path == build.directional_part_path(eng.module_path)
    eng.close()


# ------------------------------------------------------------------------------------------------ 2. batches
@pytest.mark.parametrize("key", ["layout_8", "P2U"])
def test_every_lane_works_at_its_own_point_direction_and_parameters(key, probe_dir):
    import torch
    C, eng = _engine(key)
    probe = Probe(key, probe_dir)
    batch = eng.batch(4)
    X = np.stack([C.points[0], C.points[1], C.points[-1]])
    V = C.directions()[[3, 2, 4]]
    TH = None
    if key == "P2U":
        TH = np.stack([C.thetas[0], C.thetas[1], C.thetas[0]])      # lane 1 with a parameter row of its own
        batch.set_parameters(TH)
    theta = (lambda k: None) if TH is None else (lambda k: TH[k])
    stream = torch.cuda.current_stream().cuda_stream
    d_X, d_V = _dev(X), _dev(V)
    for B in (1, 3):                                    # of capacity 4
        d_dF = torch.full((4, eng.m), -7.0, dtype=torch.float64, device=d_X.device)
        d_F = torch.full((4, eng.m), -7.0, dtype=torch.float64, device=d_X.device)
        batch.directional_dev(B, d_X.data_ptr(), d_V.data_ptr(), d_dF.data_ptr(), d_F.data_ptr(), stream)
        torch.cuda.synchronize()
        dF, F0 = d_dF.cpu().numpy(), d_F.cpu().numpy()
        for k in range(B):
            if TH is not None:
                eng.set_parameters(TH[k])               # (the single-point call at that point and those values ...
            one, F1 = eng.directional(X[k], V[k:k + 1])
            if TH is not None:
                batch.set_parameters(TH)                # ... the handle's setter reaches the lanes: theirs again)
            want, F_want = probe(X[k], V[k], theta(k))
            assert np.array_equal(one[0], want[0]) and np.array_equal(F1, F_want), (key, B, k)
            assert np.array_equal(dF[k], one[0]) and np.array_equal(F0[k], F1), (key, B, k)
        assert np.all(dF[B:] == -7.0) and np.all(F0[B:] == -7.0)    # the other lanes' outputs are not touched
    dF3, F3 = batch.directional(X, V)                   # the host form
    assert np.array_equal(dF3, dF[:3]) and np.array_equal(F3, F0[:3])
    dF1, _ = batch.directional(X, V, count=1)
    assert dF1.shape == (1, eng.m) and np.array_equal(dF1[0], dF[0])
    eng.close()

    # Problem level: next to any jacobian=, which is bit for bit what it is without the keyword
    prob, obj = C.prob, C.obj
    parameters = None if TH is None else TH
    res = prob.evaluate_batch(obj, X, jacobian="exact", parameters=parameters, directions=V)
    plain = prob.evaluate_batch(obj, X, jacobian="exact", parameters=parameters)
    assert plain.directional is None and res.directional.shape == (3, eng.m)
    assert np.array_equal(res.values, plain.values) and np.array_equal(res.cost, plain.cost)
    assert np.array_equal(res.equality, plain.equality) and np.array_equal(res.gradient, plain.gradient)
    for k in range(3):
        assert np.array_equal(res.directional[k], probe(X[k], V[k], theta(k))[0][0])
    only = prob.evaluate_batch(obj, X, parameters=parameters, directions=V)
    assert np.array_equal(only.directional, res.directional) and np.array_equal(only.cost, res.cost)
    prob._engine.close()
    prob._engine = prob._batch = None


# ------------------------------------------------------------------------------------------------ 3. a captured graph
def test_a_captured_graph_replays_on_another_point_and_other_directions(probe_dir):
    import torch
    key = "G17"
    C, eng = _engine(key)
    probe = Probe(key, probe_dir)
    dev = torch.device("cuda", 0)
    V = C.directions()
    d_x = torch.zeros(eng.n, dtype=torch.float64, device=dev)
    d_V = torch.zeros((3, eng.n), dtype=torch.float64, device=dev)
    d_dF = torch.full((3, eng.m), -7.0, dtype=torch.float64, device=dev)
    d_F = torch.full((eng.m,), -7.0, dtype=torch.float64, device=dev)

    def call(stream):                                   # a linear capture: no parallel branches
        eng.directional_dev(d_x.data_ptr(), 3, d_V.data_ptr(), d_dF.data_ptr(), d_F.data_ptr(), stream)

    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        d_x.copy_(torch.from_numpy(C.points[0]))
        d_V.copy_(torch.from_numpy(V[[0, 1, 2]]))
        call(side.cuda_stream)                          # warm: the part is built and loaded outside the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        call(torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    for x, rows in ((C.points[1], [3, 4, 5]), (C.points[-1], [5, 2, 3])):
        d_x.copy_(torch.from_numpy(x))
        d_V.copy_(torch.from_numpy(V[rows]))
        d_dF.fill_(-7.0)
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        replayed, F_replayed = d_dF.cpu().numpy(), d_F.cpu().numpy()
        direct, F_direct = eng.directional(x, V[rows])
        want, F_want = probe(x, V[rows], C.thetas[0])
        assert np.array_equal(replayed, direct) and np.array_equal(F_replayed, F_direct)
        assert np.array_equal(replayed, want) and np.array_equal(F_replayed, F_want)
    eng.close()


# ------------------------------------------------------------------------------------------------ 4. errors, bookkeeping
def test_errors_before_the_load_and_for_no_direction():
    lib = _native.lib()
    C, eng = _engine("B5")
    x, V = C.points[0], C.directions()[:2]
    dF, F0 = np.empty((2, eng.m)), np.empty(eng.m)
    # before the load: 4
    assert lib.og_directional(eng._handle, _native.dptr(x), 2, _native.dptr(V), _native.dptr(dF), _native.dptr(F0)) == 4
    assert b"og_directional_load" in lib.og_last_error()
    assert lib.og_directional_dev(eng._handle, 8, 1, 8, 8, None, None) == 4
    assert lib.og_directional_load(eng._handle, None) == 4
    assert lib.og_directional_load(eng._handle, b"/nonexistent/part.so") == 4
    # another module's part, and another part of this module: 5
    other = build.build_directional_part(dc.case("G17").header)
    assert lib.og_directional_load(eng._handle, other.encode()) == 5
    assert b"does not belong" in lib.og_last_error()
    batch = eng.batch(2)                                # (its batch part exports the batched entry name too)
    assert lib.og_directional_load(eng._handle, build.batch_part_path(eng.module_path).encode()) == 5
    X = np.stack([x, x])
    assert lib.og_directional_batch(batch._handle, 2, _native.dptr(X), _native.dptr(V), None, _native.dptr(dF)) == 4
    eng._load_directional_part()
    assert lib.og_directional_load(eng._handle, None) == 0          # loaded: a no-op
    # k = 0, a negative k, null pointers, a count out of range: 1 and a message
    assert lib.og_directional(eng._handle, _native.dptr(x), 0, _native.dptr(V), _native.dptr(dF), None) == 1
    assert b"k must be at least 1" in lib.og_last_error()
    assert lib.og_directional_dev(eng._handle, 8, 0, 8, 8, None, None) == 1
    assert lib.og_directional_dev(eng._handle, 8, -3, 8, 8, None, None) == 1
    assert lib.og_directional_dev(eng._handle, 8, 1, None, 8, None, None) == 1
    assert lib.og_directional(eng._handle, _native.dptr(x), 2, None, _native.dptr(dF), None) == 1
    assert b"null argument" in lib.og_last_error()
    assert lib.og_directional_batch(batch._handle, 0, _native.dptr(X), _native.dptr(V), None, _native.dptr(dF)) == 1
    assert lib.og_directional_batch(batch._handle, 3, _native.dptr(X), _native.dptr(V), None, _native.dptr(dF)) == 1
    assert b"capacity" in lib.og_last_error()
    assert lib.og_directional_batch_dev(batch._handle, 2, 8, None, None, 8, None) == 1
    with pytest.raises(ValueError, match="directions must have shape"):
        eng.directional(x, V[:, :-1])
    with pytest.raises(ValueError, match="directions for"):
        batch.directional(X, V[:1])
    # and the good call still works
    assert lib.og_directional(eng._handle, _native.dptr(x), 2, _native.dptr(V), _native.dptr(dF), None) == 0
    assert np.all(np.isfinite(dF))
    eng.close()


def test_no_state_word_moves(probe_dir):
    """An FD sweep into a registered buffer gives the bits it gave before a directional call (single point and batch)
    came between: the call counts no launch into the buffer's words and leaves its structural zeros alone."""
    import torch
    key = "layout_8"
    C, eng = _engine(key)
    probe = Probe(key, probe_dir)
    lb, ub = np_path.bounds_arrays(C.prob)
    xa, xb = C.points[1], C.points[-1]
    ha, hb = _native.fd_step(xa, lb, ub), _native.fd_step(xb, lb, ub)
    V = C.directions()[[3, 4]]
    stream = torch.cuda.current_stream().cuda_stream
    dev = torch.device("cuda", 0)
    d_JT = torch.full((eng.n, eng.m), -7.0, dtype=torch.float64, device=dev)
    d_F = torch.zeros(eng.m, dtype=torch.float64, device=dev)
    d_dF = torch.zeros((2, eng.m), dtype=torch.float64, device=dev)
    eng.register_jt_dev(d_JT.data_ptr(), 0, eng.n, stream)

    def sweep(x, h):
        d_x, d_h = _dev(x), _dev(h)
        eng.sweep_dev(d_x.data_ptr(), d_h.data_ptr(), 0, eng.n, d_JT.data_ptr(), d_F.data_ptr(), stream)
        torch.cuda.synchronize()
        return d_JT.cpu().numpy(), d_F.cpu().numpy()

    def directional(x):
        d_x, d_V = _dev(x), _dev(V)
        eng.directional_dev(d_x.data_ptr(), 2, d_V.data_ptr(), d_dF.data_ptr(), None, stream)
        torch.cuda.synchronize()
        return d_dF.cpu().numpy()

    JT_a, F_a = sweep(xa, ha)
    JT_b, F_b = sweep(xb, hb)
    assert not np.array_equal(JT_a, JT_b) and np.count_nonzero(JT_b) <= eng.pattern()[0][-1]
    again, F_again = sweep(xa, ha)
    assert np.array_equal(again, JT_a) and np.array_equal(F_again, F_a)
    assert np.array_equal(directional(xb), probe(xb, V)[0])
    assert np.array_equal(d_JT.cpu().numpy(), JT_a)                 # the buffer is where the sweep left it
    after, F_after = sweep(xb, hb)
    assert np.array_equal(after, JT_b) and np.array_equal(F_after, F_b)
    assert np.array_equal(directional(xa), probe(xa, V)[0])
    after, F_after = sweep(xa, ha)
    assert np.array_equal(after, JT_a) and np.array_equal(F_after, F_a)
    eng.unregister_jt_dev(d_JT.data_ptr())
    # the lanes of a batch: their own registered matrices
    batch = eng.batch(2)
    X, H = np.stack([xa, xb]), np.stack([ha, hb])
    batch.sweep(X, H)
    dense = [batch.dense(k).copy() for k in range(2)]
    assert np.array_equal(dense[0], JT_a) and np.array_equal(dense[1], JT_b)
    dF, _ = batch.directional(X[::-1].copy(), V)
    assert np.array_equal(dF[0], probe(xb, V[0])[0][0]) and np.array_equal(dF[1], probe(xa, V[1])[0][0])
    assert all(np.array_equal(batch.dense(k), dense[k]) for k in range(2))
    batch.sweep(X, H)
    assert all(np.array_equal(batch.dense(k), dense[k]) for k in range(2))
    eng.close()


# ------------------------------------------------------------------------------------------------ 5. Problem level
def test_directional_derivative_end_to_end():
    prob, obj = problems.build("brachistochrone")
    C = dc.case("brachistochrone")
    V = C.directions()
    got = prob.directional_derivative(obj, V)           # at prob.p
    assert got.shape == (7, C.m) and getattr(prob, "_batch", None) is None
    F0, JT = prob._engine.exact_stacked(np.asarray(prob.p, dtype=float))
    _, scale = dc.twin_product(JT, V)
    assert dc.worst_error(got, dc.complex_step(C, prob.p, V), scale) <= dc.BOUND
    one = prob.directional_derivative(obj, V[3])
    assert one.shape == (C.m,) and np.array_equal(one, got[3])
    with pytest.raises(ValueError, match="directions must have"):
        prob.directional_derivative(obj, V[3][:-1])
    prob._engine.close()
