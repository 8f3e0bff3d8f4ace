"""The exact sparse Hessian of ``w . F`` on the GPU (``og_hessian_matrix*``, ``HipEngine.hessian_matrix``,
``BatchSweep.hessian_matrix``, ``Problem.hessian_matrix``, ``evaluate_batch(hessians=)``).  The kernels sum the terms of
``csrc/og_hess.h`` in the order ``csrc/og_adj.h`` fixes, so every comparison is BITWISE: against the host probe of that
header (tests/hess_probe.cpp, g++), whose own distance from an independent reference tests/test_hessian_matrix.py bounds,
and - independently of the probe - against ``HipEngine.hessian_vector`` with the ``n`` unit directions.  Shapes
(``hessian_cases.GPU_KEYS``; their modules, batch parts, Hessian parts and Hessian-matrix parts are compiled by
``__graft_entry__.build``): B5, G17 and P2U - every entry is summed inside one wavefront; layout_8 - two phases, entries
of up to 192 listed terms (a workgroup), 130 variables without an entry; B90 - the diagonal of the final time lists 272
terms, two of them per chain for sixteen chains, the diagonals of the states 90 and more.  tests/test_hessian_matrix.py
checks on the CPU that the shapes contain these."""

import ctypes

import numpy as np
import pytest

import hessian_matrix_cases as mc
from opengoddard_amd import _native, build, problems

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def probe_dir(tmp_path_factory):
    return str(tmp_path_factory.mktemp("hess_probe_gpu"))


def _engine(key):
    from opengoddard_amd.engine import HipEngine
    C = mc.case(key)
    eng = HipEngine(C.prob, C.obj, program=C.program)
    assert eng.header == C.header
    return C, eng


class Probe:
    """``(H, F0)`` of the host probe at ``(x, W, theta)``, computed once per argument set."""

    def __init__(self, key, folder):
        self.case, self.folder = mc.case(key), folder
        self.exe = mc.build_probe(self.case, folder)
        self.known = {}

    def __call__(self, x, W, theta=None):
        W = np.atleast_2d(np.asarray(W, dtype=float))
        at = (np.asarray(x, dtype=float).tobytes(), W.tobytes(), None if theta is None else np.asarray(theta).tobytes())
        if at not in self.known:
            r = mc.run_probe(self.case, self.exe, self.folder, x, W, theta, "gpu")
            self.known[at] = (r.H, r.F0)
        return self.known[at]


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(torch.device("cuda", 0))


def _same(a, b):
    """bit for bit, the sign of a zero included"""
    return np.array_equal(a, b) and np.array_equal(np.signbit(a), np.signbit(b))


# ------------------------------------------------------------------------------------------------ 1. single point
@pytest.mark.parametrize("key", mc.GPU_KEYS)
def test_a_single_point_equals_the_probe_bit_for_bit(key, probe_dir):
    import torch
    C, eng = _engine(key)
    assert eng.hessian_matrix_part_path is None         # neither built nor loaded until asked for
    assert _native.lib().og_hessian_matrix_nnz(eng._handle) == -1
    probe = Probe(key, probe_dir)
    stream = torch.cuda.current_stream().cuda_stream
    W8 = mc.weights(C)
    nnz = mc.plan(C).nnz
    indptr, cols = eng.hessian_pattern()
    assert np.array_equal(indptr, mc.plan(C).indptr) and np.array_equal(cols, mc.plan(C).cols)
    assert eng.hessian_matrix_part_path is None         # (the pattern is host work)
    rows9 = list(range(8)) + [2]                        # K = 9: a chunk of eight vectors and one of one
    three = [2, 4, 6]                                   # all ones, a seeded one, the zero vector
    for theta in ([C.thetas[0], C.thetas[-1]] if len(C.thetas) > 1 else [C.thetas[0]]):
        x = C.points[-1]
        if theta is not None:
            eng.set_parameters(theta)                   # (no rebuild: the same module, part and plan)
        want, F_want = probe(x, W8, theta)
        assert _same(F_want, eng.eval_stacked(x))       # F0 is og_eval's
        d_x, d_W = _dev(x), _dev(W8[rows9])
        d_H = torch.full((10, nnz), -7.0, dtype=torch.float64, device=d_x.device)
        d_F = torch.full((eng.m,), -7.0, dtype=torch.float64, device=d_x.device)
        eng.hessian_matrix_dev(d_x.data_ptr(), 9, d_W.data_ptr(), d_H.data_ptr(), d_F.data_ptr(), stream)
        torch.cuda.synchronize()
        H, F0 = d_H.cpu().numpy(), d_F.cpu().numpy()
        assert _same(H[:9], want[rows9]) and _same(F0, F_want), key
        assert np.all(H[9:] == -7.0)                    # nothing past K rows
        assert not H[6].any() and not np.signbit(H[6]).any()            # the zero vector: +0.0 everywhere
        # K = 3 and K = 1: vector d of a call with K vectors is the call with that vector alone (F0 is optional)
        d_W3 = _dev(W8[three])
        d_H.fill_(-7.0)
        eng.hessian_matrix_dev(d_x.data_ptr(), 3, d_W3.data_ptr(), d_H.data_ptr(), None, stream)
        torch.cuda.synchronize()
        H = d_H.cpu().numpy()
        assert _same(H[:3], want[three]) and np.all(H[3:] == -7.0), key
        for d in (0, 5, 7):
            d_H.fill_(-7.0)
            eng.hessian_matrix_dev(d_x.data_ptr(), 1, d_W[d].data_ptr(), d_H.data_ptr(), None, stream)
            torch.cuda.synchronize()
            one = d_H.cpu().numpy()
            assert _same(one[0], want[d]) and np.all(one[1:] == -7.0), (key, d)
        H_h, F_h = eng.hessian_matrix(x, W8)            # the host-pointer form, K = 8 and K = 1
        assert _same(H_h, want) and _same(F_h, F_want)
        H_h, F_h = eng.hessian_matrix(x, W8[3:4])
        assert H_h.shape == (1, nnz) and _same(H_h[0], want[3]) and _same(F_h, F_want)
    assert eng.hessian_matrix_part_path == build.hessian_matrix_part_path(eng.module_path)
    assert _native.lib().og_hessian_matrix_nnz(eng._handle) == nnz
    assert getattr(eng, "hessian_part_path", None) is None          # the Hessian-vector part was never needed
    eng.close()


# ------------------------------------------------------------------------------------------------ 2. unit directions
@pytest.mark.parametrize("key", mc.GPU_KEYS)
def test_entries_are_the_unit_hessian_vector_products_of_the_device(key):
    """Independently of the probe: ``eng.hessian_vector`` with K = n unit directions and one weight vector; every stored
    entry is its product at the owner's orientation bit for bit, every entry outside the pattern is +0.0."""
    C, eng = _engine(key)
    hp = mc.plan(C)
    row, col, owner, partner = mc.pairs_of(hp)
    stored = np.zeros((C.n, C.n), dtype=bool)
    stored[row, col] = stored[col, row] = True
    W8 = mc.weights(C)
    x, theta = C.points[1], C.thetas[-1]
    if theta is not None:
        eng.set_parameters(theta)
    H, _ = eng.hessian_matrix(x, W8[[3, 2]])
    for i, d in enumerate((3, 2)):
        Q, _ = eng.hessian_vector(x, np.tile(W8[d], (C.n, 1)), np.eye(C.n))         # Q[l, j] = hvp(w, e_l)[j]
        assert _same(H[i], Q[partner, owner]), (key, d)
        off = Q[~stored]
        assert not off.any() and not np.signbit(off).any(), (key, d)
    assert H.any()
    eng.close()


# ------------------------------------------------------------------------------------------------ 3. batches, a graph
@pytest.mark.parametrize("key", ["layout_8", "P2U"])
def test_every_lane_works_at_its_own_point_vector_and_parameters(key, probe_dir):
    import torch
    C, eng = _engine(key)
    probe = Probe(key, probe_dir)
    nnz = mc.plan(C).nnz
    batch = eng.batch(4)
    X = np.stack([C.points[0], C.points[1], C.points[-1]])
    W = mc.weights(C)[[3, 2, 7]]
    TH = None
    if key == "P2U":
        TH = np.stack([C.thetas[0], C.thetas[1], C.thetas[0]])      # lane 1 with a parameter row of its own
        batch.set_parameters(TH)
    theta = (lambda k: None) if TH is None else (lambda k: TH[k])
    stream = torch.cuda.current_stream().cuda_stream
    d_X, d_W = _dev(X), _dev(W)
    for B in (1, 3):                                    # of capacity 4
        d_H = torch.full((4, nnz), -7.0, dtype=torch.float64, device=d_X.device)
        d_F = torch.full((4, eng.m), -7.0, dtype=torch.float64, device=d_X.device)
        batch.hessian_matrix_dev(B, d_X.data_ptr(), d_W.data_ptr(), d_H.data_ptr(), d_F.data_ptr(), stream)
        torch.cuda.synchronize()
        H, F0 = d_H.cpu().numpy(), d_F.cpu().numpy()
        for k in range(B):
            if TH is not None:
                eng.set_parameters(TH[k])               # (the single-point call at that point and those values ...
            one, F1 = eng.hessian_matrix(X[k], W[k:k + 1])
            if TH is not None:
                batch.set_parameters(TH)                # ... the handle's setter reaches the lanes: theirs again)
            want, F_want = probe(X[k], W[k], theta(k))
            assert _same(one[0], want[0]) and _same(F1, F_want), (key, B, k)
            assert _same(H[k], one[0]) and _same(F0[k], F1), (key, B, k)
        assert np.all(H[B:] == -7.0) and np.all(F0[B:] == -7.0)     # the other lanes' outputs are not touched
    H3, F3 = batch.hessian_matrix(X, W)                 # the host form
    assert _same(H3, H[:3]) and _same(F3, F0[:3])
    H1, _ = batch.hessian_matrix(X, W, count=1)
    assert H1.shape == (1, nnz) and _same(H1[0], H[0])
    with pytest.raises(ValueError, match="weight vectors for"):
        batch.hessian_matrix(X, W[:1])
    eng.close()


def test_a_captured_graph_replays_on_another_point_and_other_vectors(probe_dir):
    import torch
    key = "layout_8"
    C, eng = _engine(key)
    probe = Probe(key, probe_dir)
    nnz = mc.plan(C).nnz
    dev = torch.device("cuda", 0)
    W = mc.weights(C)
    d_x = torch.zeros(eng.n, dtype=torch.float64, device=dev)
    d_W = torch.zeros((3, eng.m), dtype=torch.float64, device=dev)
    d_H = torch.full((3, nnz), -7.0, dtype=torch.float64, device=dev)
    d_F = torch.full((eng.m,), -7.0, dtype=torch.float64, device=dev)

    def call(stream):                                   # a linear capture: no parallel branches
        eng.hessian_matrix_dev(d_x.data_ptr(), 3, d_W.data_ptr(), d_H.data_ptr(), d_F.data_ptr(), stream)

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
    for x, rows in ((C.points[1], [3, 4, 5]), (C.points[-1], [5, 7, 2])):
        d_x.copy_(torch.from_numpy(x))
        d_W.copy_(torch.from_numpy(W[rows]))
        d_H.fill_(-7.0)
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        replayed, F_replayed = d_H.cpu().numpy(), d_F.cpu().numpy()
        want, F_want = probe(x, W[rows], C.thetas[0])
        assert _same(replayed, want) and _same(F_replayed, F_want)
    eng.close()


# ------------------------------------------------------------------------------------------------ 4. errors
def test_errors_before_the_load_for_a_malformed_plan_and_for_bad_arguments():
    lib = _native.lib()
    C, eng = _engine("B5")
    hp = mc.plan(C)
    W = mc.weights(C)[:2].copy()
    x = C.points[0]
    H, F0 = np.empty((2, hp.nnz)), np.empty(eng.m)
    dp = _native.dptr
    ip = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))
    arrays = hp.arrays()
    # before the load: 4
    assert lib.og_hessian_matrix(eng._handle, dp(x), 2, dp(W), dp(H), dp(F0)) == 4
    assert b"og_hessian_matrix_load" in lib.og_last_error()
    assert lib.og_hessian_matrix_dev(eng._handle, 8, 1, 8, 8, None, None) == 4
    assert lib.og_hessian_matrix_load(eng._handle, None, hp.nnz, *map(ip, arrays)) == 4
    assert lib.og_hessian_matrix_load(eng._handle, b"/nonexistent/part.so", hp.nnz, *map(ip, arrays)) == 4
    # another module's part, and another part of this module: 5
    other = build.build_hessian_matrix_part(mc.case("G17").header)
    assert lib.og_hessian_matrix_load(eng._handle, other.encode(), hp.nnz, *map(ip, arrays)) == 5
    assert b"does not belong" in lib.og_last_error()
    assert lib.og_hessian_matrix_load(eng._handle, build.build_hessian_part(eng.header).encode(), hp.nnz, *map(ip, arrays)) == 5
    # a malformed plan: 1, nothing loaded, nothing launched
    part = build.build_hessian_matrix_part(eng.header).encode()
    assert lib.og_hessian_matrix_load(eng._handle, part, hp.nnz, None, *map(ip, arrays[1:])) == 1
    assert lib.og_hessian_matrix_load(eng._handle, part, -1, *map(ip, arrays)) == 1

    def broken(index, at, value):
        out = [a.copy() for a in arrays]
        out[index][at] = value
        return out
    indptr, cols, owner, tptr, tlist = arrays
    for what, bad in (("a term", broken(4, tptr[1] - 1, hp.terms[owner[0]])),           # past the owner's column
                      ("ascend", broken(4, tptr[1] - 1, tlist[tptr[0]])),               # a list that does not ascend
                      ("partner", broken(1, indptr[3], 4)),                             # a partner above its row
                      ("owner", broken(2, 0, C.n - 1 if C.n - 1 not in (owner[0], cols[0]) else 1)),
                      ("indptr", broken(0, 2, indptr[3] + 1)),                          # not monotone
                      ("tptr", broken(3, 1, tptr[2] + 1))):
        assert lib.og_hessian_matrix_load(eng._handle, part, hp.nnz, *map(ip, bad)) == 1, what
        assert b"malformed plan" in lib.og_last_error() and what.encode() in lib.og_last_error(), lib.og_last_error()
        assert lib.og_hessian_matrix_nnz(eng._handle) == -1
        assert lib.og_hessian_matrix(eng._handle, dp(x), 2, dp(W), dp(H), dp(F0)) == 4
    batch = eng.batch(2)
    X = np.stack([x, x])
    assert lib.og_hessian_matrix_batch(batch._handle, 2, dp(X), dp(W), None, dp(H)) == 4
    eng._load_hessian_matrix_part()
    assert lib.og_hessian_matrix_load(eng._handle, None, 0, None, None, None, None, None) == 0      # loaded: a no-op
    assert lib.og_hessian_matrix_nnz(eng._handle) == hp.nnz
    # k = 0, a negative k, k past 65535, null pointers, a count out of range: 1 and a message
    assert lib.og_hessian_matrix(eng._handle, dp(x), 0, dp(W), dp(H), None) == 1
    assert b"k must be at least 1" in lib.og_last_error()
    assert lib.og_hessian_matrix_dev(eng._handle, 8, -3, 8, 8, None, None) == 1
    assert lib.og_hessian_matrix_dev(eng._handle, 8, 65536, 8, 8, None, None) == 1
    assert b"exceeds 65535" in lib.og_last_error()
    assert lib.og_hessian_matrix_dev(eng._handle, 8, 1, None, 8, None, None) == 1
    assert lib.og_hessian_matrix(eng._handle, dp(x), 2, None, dp(H), None) == 1
    assert b"null argument" in lib.og_last_error()
    assert lib.og_hessian_matrix_batch(batch._handle, 0, dp(X), dp(W), None, dp(H)) == 1
    assert lib.og_hessian_matrix_batch(batch._handle, 3, dp(X), dp(W), None, dp(H)) == 1
    assert b"capacity" in lib.og_last_error()
    assert lib.og_hessian_matrix_batch_dev(batch._handle, 2, 8, None, None, 8, None) == 1
    with pytest.raises(ValueError, match="weights must have shape"):
        eng.hessian_matrix(x, W[:, :-1])
    # and the good call still works
    assert lib.og_hessian_matrix(eng._handle, dp(x), 2, dp(W), dp(H), None) == 0
    assert np.all(np.isfinite(H))
    eng.close()


# ------------------------------------------------------------------------------------------------ 5. Problem level
def test_problem_hessian_matrix_and_evaluate_batch_end_to_end():
    prob, obj = problems.build("brachistochrone")
    C = mc.case("brachistochrone")
    W8 = mc.weights(C)
    x = np.asarray(prob.p, dtype=float)
    plain = prob.evaluate_batch(obj, np.stack([x, 1.01 * x]), jacobian="exact")
    assert plain.hessian is None and prob._engine.hessian_matrix_part_path is None      # nothing of the feature ran
    res = prob.hessian_matrix(obj, W8)                  # at prob.p
    indptr, cols = prob.hessian_pattern(obj)
    direct, _ = prob._engine.hessian_matrix(x, W8)
    assert res.values.shape == (8, cols.size) and _same(res.values, direct) and res.values.any()
    assert np.array_equal(res.indptr, indptr) and np.array_equal(res.cols, cols)
    one = prob.hessian_matrix(obj, W8[3])
    assert one.values.shape == (cols.size,) and _same(one.values, direct[3])
    # the matrix forms: the lower triangle mirrored (the entries themselves: the unit-direction test above)
    A, M = one.toarray(), one.tocsr()
    assert A.shape == (C.n, C.n) and np.array_equal(A, A.T) and np.array_equal(M.toarray(), A)
    assert np.array_equal(np.tril(A)[np.repeat(np.arange(C.n), np.diff(indptr)), cols], one.values)
    X = np.stack([x, 1.01 * x])
    both = prob.evaluate_batch(obj, X, jacobian="exact", hessians=W8[[3, 4]])
    assert both.hessian.shape == (2, cols.size) and np.array_equal(both.hessian_pattern[1], cols)
    assert np.array_equal(both.values, plain.values) and np.array_equal(both.cost, plain.cost)
    assert _same(both.hessian[0], direct[3])
    assert _same(both.hessian[1], prob._engine.hessian_matrix(X[1], W8[4:5])[0][0])
    with pytest.raises(ValueError, match="weights must have"):
        prob.hessian_matrix(obj, W8[3][:-1])
    prob._engine.close()
    prob._engine = prob._batch = None
