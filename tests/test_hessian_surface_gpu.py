"""The second-order kernels on their branches (``og_hessian_vector*``, ``og_hessian_matrix*``): four problems of the traced
surface at the points of tests/test_exact_surface.py - ``switch`` sits exactly on every tie, knot and jump of the
callbacks - where the shapes of tests/test_hessian_gpu.py and tests/test_hessian_matrix_gpu.py are smooth and evaluated at a
random perturbation.  Every comparison is BITWISE, the sign of a zero included, against the host probes of the same
headers (tests/hvp_probe.cpp, tests/hess_probe.cpp, g++), whose distance from the independent referee
``oracle/exact_hess.py`` tests/test_hessian_surface.py bounds at the same points.

Shapes (``hessian_cases.GPU_SURFACE_KEYS``; ``__graft_entry__.build`` compiles their modules, batch parts, Hessian parts
and Hessian-matrix parts, and the two host probes of each): ``wide_reductions`` - n 407, 137 heavy columns, one column of
270 terms: reductions, ``clip``, tables and ties through the workgroup path and a chain's second trip; ``table_ascent`` -
n 281, a 200-term final time: table lookups on knots, mask assignment; ``preallocated_outputs`` - n 55: the jumps of
``%`` / ``mod``, ``heaviside`` at 0, a tie of ``max(axis=0)``; ``ragged_two_phase`` - n 48, two phases: a ``where``
threshold, a tie of ``maximum``.  In the batch test the four lanes of ONE launch are the four named points: lanes that
take different branches of the same generated code."""

import numpy as np
import pytest

import hessian_cases as hc
import hessian_matrix_cases as mc
import test_exact_surface as surface

pytestmark = pytest.mark.gpu

KEYS = hc.GPU_SURFACE_KEYS
POINTS = surface.POINTS
LANE_PAIRS = [3, 2, 7, 5]               # the pair (of hessian_cases.pairs) each lane of the batch works on


@pytest.fixture(scope="module")
def probe_dir(tmp_path_factory):
    return str(tmp_path_factory.mktemp("hess_surface_gpu"))


@pytest.fixture(scope="module")
def engines():
    """One engine per problem, made once and closed when the module is done."""
    from opengoddard_amd.engine import HipEngine
    made = {}

    def get(key):
        if key not in made:
            C = hc.case(key)
            made[key] = HipEngine(C.prob, C.obj, program=C.program)
            assert made[key].header == C.header
        return made[key]

    yield get
    for eng in made.values():
        eng.close()


def _weights(C):
    W = mc.weights(C)
    return W[[2, 3, 7]] if C.key == "wide_reductions" else W            # (its plan stores 66 918 entries)


_HVP, _HESS = {}, {}


def _hvp_probe(key, point, folder):
    """``(Q[8, n], F0)`` of the host probe of ``og_hvp.h`` at a named point for the eight pairs, once per session."""
    if (key, point) not in _HVP:
        C = hc.case(key)
        W, V = hc.pairs(C)
        exe = hc.build_probe(C, mc.probe_folder(C, folder))             # (built ahead by __graft_entry__.build)
        r = hc.run_probe(C, exe, folder, hc.named_point(C, point), W, V, None, "gpu_" + point)
        _HVP[key, point] = (r.Q, r.F0)
    return _HVP[key, point]


def _hess_probe(key, point, folder):
    """``(H[K, nnz], F0)`` of the host probe of ``og_hess.h`` at a named point for ``_weights``, once per session."""
    if (key, point) not in _HESS:
        C = mc.case(key)
        exe = mc.build_probe(C, mc.probe_folder(C, folder))             # (built ahead by __graft_entry__.build)
        r = mc.run_probe(C, exe, folder, hc.named_point(C, point), _weights(C), None, "gpu_" + point)
        _HESS[key, point] = (r.H, r.F0)
    return _HESS[key, point]


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(torch.device("cuda", 0))


def _same(a, b):
    """bit for bit, the sign of a zero included"""
    return np.array_equal(a, b) and np.array_equal(np.signbit(a), np.signbit(b))


def _first_difference(got, want):
    at = np.argwhere((got != want) | (np.signbit(got) != np.signbit(want)))
    return None if at.size == 0 else (tuple(int(i) for i in at[0]), got[tuple(at[0])], want[tuple(at[0])])


# ------------------------------------------------------------------------------------------------ 1. single point
@pytest.mark.parametrize("point", ["switch", "minus"])
@pytest.mark.parametrize("key", KEYS)
def test_hessian_vector_at_a_point_on_the_branches_equals_the_probe(key, point, probe_dir, engines):
    import torch
    C, eng = hc.case(key), engines(key)
    x = hc.named_point(C, point)
    W8, V8 = hc.pairs(C)
    want, F_want = _hvp_probe(key, point, probe_dir)
    assert _same(F_want, eng.eval_stacked(x))           # F0 is og_eval's
    stream = torch.cuda.current_stream().cuda_stream
    d_x, d_W, d_V = _dev(x), _dev(W8), _dev(V8)
    d_Q = torch.full((9, eng.n), -7.0, dtype=torch.float64, device=d_x.device)
    d_F = torch.full((eng.m,), -7.0, dtype=torch.float64, device=d_x.device)
    eng.hessian_vector_dev(d_x.data_ptr(), 8, d_W.data_ptr(), d_V.data_ptr(), d_Q.data_ptr(), d_F.data_ptr(), stream)
    torch.cuda.synchronize()
    Q, F0 = d_Q.cpu().numpy(), d_F.cpu().numpy()
    assert _same(Q[:8], want), (key, point, _first_difference(Q[:8], want))
    assert _same(F0, F_want) and np.all(Q[8:] == -7.0)
    assert not Q[6].any() and not np.signbit(Q[6]).any()            # the zero pair: +0.0 everywhere


@pytest.mark.parametrize("point", ["switch", "minus"])
@pytest.mark.parametrize("key", KEYS)
def test_hessian_matrix_at_a_point_on_the_branches_equals_the_probe(key, point, probe_dir, engines):
    import torch
    C, eng = mc.case(key), engines(key)
    x, W = hc.named_point(C, point), _weights(C)
    K, nnz = W.shape[0], mc.plan(C).nnz
    want, F_want = _hess_probe(key, point, probe_dir)
    stream = torch.cuda.current_stream().cuda_stream
    d_x, d_W = _dev(x), _dev(W)
    d_H = torch.full((K + 1, nnz), -7.0, dtype=torch.float64, device=d_x.device)
    d_F = torch.full((eng.m,), -7.0, dtype=torch.float64, device=d_x.device)
    eng.hessian_matrix_dev(d_x.data_ptr(), K, d_W.data_ptr(), d_H.data_ptr(), d_F.data_ptr(), stream)
    torch.cuda.synchronize()
    H, F0 = d_H.cpu().numpy(), d_F.cpu().numpy()
    assert _same(H[:K], want), (key, point, _first_difference(H[:K], want))
    assert _same(F0, F_want) and _same(F0, eng.eval_stacked(x)) and np.all(H[K:] == -7.0)
    assert H[:K].any()


# ------------------------------------------------------------------------------------------------ 2. four lanes, four points
@pytest.mark.parametrize("key", KEYS)
def test_the_four_lanes_of_one_launch_are_the_four_named_points(key, probe_dir, engines):
    """Capacity 4, count 4 and 3: every lane equals the single-point call at its point, for the products and for the
    matrix; the products are the probe's at that point as well; lanes past the count are not touched."""
    import torch
    C, eng = hc.case(key), engines(key)
    nnz = mc.plan(C).nnz
    X = np.stack([hc.named_point(C, point) for point in POINTS])
    W8, V8 = hc.pairs(C)
    W, V = W8[LANE_PAIRS], V8[LANE_PAIRS]
    stream = torch.cuda.current_stream().cuda_stream
    single_Q, single_H, single_F = [], [], []
    for k, point in enumerate(POINTS):
        one, F1 = eng.hessian_vector(X[k], W[k:k + 1], V[k:k + 1])
        assert _same(one[0], _hvp_probe(key, point, probe_dir)[0][LANE_PAIRS[k]]), (key, point)
        mat, F2 = eng.hessian_matrix(X[k], W[k:k + 1])
        assert _same(F1, F2) and _same(F1, _hvp_probe(key, point, probe_dir)[1])
        single_Q.append(one[0]), single_H.append(mat[0]), single_F.append(F1)
    batch = eng.batch(4)
    try:
        d_X, d_W, d_V = _dev(X), _dev(W), _dev(V)
        for B in (4, 3):
            d_Q = torch.full((4, eng.n), -7.0, dtype=torch.float64, device=d_X.device)
            d_H = torch.full((4, nnz), -7.0, dtype=torch.float64, device=d_X.device)
            d_F = torch.full((4, eng.m), -7.0, dtype=torch.float64, device=d_X.device)
            d_G = torch.full((4, eng.m), -7.0, dtype=torch.float64, device=d_X.device)
            batch.hessian_vector_dev(B, d_X.data_ptr(), d_W.data_ptr(), d_V.data_ptr(), d_Q.data_ptr(), d_F.data_ptr(), stream)
            batch.hessian_matrix_dev(B, d_X.data_ptr(), d_W.data_ptr(), d_H.data_ptr(), d_G.data_ptr(), stream)
            torch.cuda.synchronize()
            Q, H, F0, G0 = d_Q.cpu().numpy(), d_H.cpu().numpy(), d_F.cpu().numpy(), d_G.cpu().numpy()
            for k in range(B):
                assert _same(Q[k], single_Q[k]), (key, B, POINTS[k], _first_difference(Q[k], single_Q[k]))
                assert _same(H[k], single_H[k]), (key, B, POINTS[k], _first_difference(H[k], single_H[k]))
                assert _same(F0[k], single_F[k]) and _same(G0[k], single_F[k]), (key, B, POINTS[k])
            for out in (Q, H, F0, G0):
                assert np.all(out[B:] == -7.0)          # the other lanes' outputs are not touched
    finally:
        batch.close()


# ------------------------------------------------------------------------------------------------ 3. the host-pointer forms
@pytest.mark.parametrize("key", KEYS)
def test_the_host_pointer_forms_at_the_switch_point(key, probe_dir, engines):
    C, eng = hc.case(key), engines(key)
    x = hc.named_point(C, "switch")
    W8, V8 = hc.pairs(C)
    want, F_want = _hvp_probe(key, "switch", probe_dir)
    Q, F0 = eng.hessian_vector(x, W8, V8)
    assert _same(Q, want) and _same(F0, F_want), (key, _first_difference(Q, want))
    want, F_want = _hess_probe(key, "switch", probe_dir)
    H, F0 = eng.hessian_matrix(x, _weights(C))
    assert _same(H, want) and _same(F0, F_want), (key, _first_difference(H, want))
    batch = eng.batch(4)
    try:
        X = np.stack([hc.named_point(C, point) for point in POINTS])
        Qb, Fb = batch.hessian_vector(X, W8[LANE_PAIRS], V8[LANE_PAIRS])
        Hb, _ = batch.hessian_matrix(X, W8[LANE_PAIRS])
        assert _same(Qb[2], Q[LANE_PAIRS[2]]) and _same(Fb[2], F_want)          # lane 2 is the switch point
        assert Hb.shape == (4, mc.plan(C).nnz) and _same(Hb[2], eng.hessian_matrix(x, W8[LANE_PAIRS[2]:LANE_PAIRS[2] + 1])[0][0])
    finally:
        batch.close()
