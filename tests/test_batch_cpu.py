"""Batches of points (``og_batch_*``, ``HipEngine.batch``, ``Problem.evaluate_batch``): everything that can be checked
without a GPU - the C ABI's declarations and error paths, the argument checks and host logic of
``Problem.evaluate_batch`` with the NumPy oracle injected, and the cross-compilation of the batch kernels."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from opengoddard_amd import _native, build, codegen, problems
from opengoddard_amd import optimize as og

BATCH_FUNCTIONS = ("og_batch_create", "og_batch_destroy", "og_batch_capacity", "og_batch_eval_dev",
                   "og_batch_fd_sweep_dev", "og_batch_lane_dev", "og_batch_eval", "og_batch_fd_sweep")


def _declared_in_header():
    with open(os.path.join(ROOT, "include", "ogpsx.h")) as fh:
        text = re.sub(r"/\*.*?\*/", "", fh.read(), flags=re.S)
    return set(re.findall(r"\b(og_batch_[a-z_]+)\s*\(", text))


def test_library_exports_the_batch_functions_the_header_declares():
    declared = _declared_in_header()
    assert declared == set(BATCH_FUNCTIONS)
    lib = _native.lib()
    for name in declared:
        assert name in _native.SIGNATURES, name + " has no ctypes signature"
        fn = getattr(lib, name)                       # AttributeError: not exported
        assert fn.argtypes == _native.SIGNATURES[name][1]


def _error_text():
    msg = _native.lib().og_last_error()
    return msg.decode() if msg else ""


def test_null_batch_and_null_handle_are_errors():
    lib = _native.lib()
    out = C.c_void_p(1)
    assert lib.og_batch_create(None, 3, b"/nonexistent.so", C.byref(out)) != 0
    assert "og_batch_create" in _error_text() and not out.value
    x = np.zeros(4)
    ptr = _native.dptr(x)
    bad = np.zeros(1, dtype=np.int32)
    calls = {
        "og_batch_eval_dev": lambda: lib.og_batch_eval_dev(None, 1, 8, 8, None),
        "og_batch_fd_sweep_dev": lambda: lib.og_batch_fd_sweep_dev(None, 1, 8, 8, 8, None, None),
        "og_batch_lane_dev": lambda: lib.og_batch_lane_dev(None, 0, None, bad.ctypes.data_as(C.POINTER(C.c_int32))),
        "og_batch_eval": lambda: lib.og_batch_eval(None, 1, ptr, ptr),
        "og_batch_fd_sweep": lambda: lib.og_batch_fd_sweep(None, 1, ptr, ptr, ptr, ptr, None),
    }
    for name, call in calls.items():
        assert call() != 0, name
        assert name in _error_text() and "null batch" in _error_text()
    assert lib.og_batch_capacity(None) == 0
    lib.og_batch_destroy(None)                       # a no-op, like og_problem_destroy(NULL)


@pytest.fixture
def no_engine(monkeypatch):
    """Any attempt to build an engine fails the test: the argument checks come first."""
    def factory(prob, obj):
        raise AssertionError("an engine was built before the arguments were checked")
    monkeypatch.setattr(og, "ENGINE_FACTORY", factory)


def test_evaluate_batch_checks_its_arguments_before_it_builds_an_engine(no_engine):
    prob, obj = problems.build("brachistochrone")
    n = prob.number_of_variables
    with pytest.raises(AssertionError, match=r"points must have shape \[B, number_of_variables\]"):
        prob.evaluate_batch(obj, np.zeros(n))
    with pytest.raises(AssertionError, match="points must have %d columns" % n):
        prob.evaluate_batch(obj, np.zeros((2, n + 1)))
    with pytest.raises(AssertionError, match="points holds no point"):
        prob.evaluate_batch(obj, np.zeros((0, n)))
    # the texts Problem.solve uses
    bare = og.Problem([0.0, 1.0], [5], [1], [1], 1)
    bare.dynamics = []                               # (as solve: a list without entries is "not set")
    with pytest.raises(AssertionError, match="It must be set dynamics"):
        bare.evaluate_batch(None, np.zeros((1, bare.number_of_variables)))
    bare.dynamics = [lambda prob, obj, section: None]
    with pytest.raises(AssertionError, match="It must be set cost function"):
        bare.evaluate_batch(None, np.zeros((1, bare.number_of_variables)))
    bare.cost = lambda prob, obj: 0.0
    with pytest.raises(AssertionError, match="It must be set equality function"):
        bare.evaluate_batch(None, np.zeros((1, bare.number_of_variables)))
    bare.equality = lambda prob, obj: np.zeros(0)
    with pytest.raises(AssertionError, match="It must be set inequality function"):
        bare.evaluate_batch(None, np.zeros((1, bare.number_of_variables)))


@pytest.fixture
def oracle_engine(monkeypatch):
    from oracle import np_path
    monkeypatch.setattr(og, "ENGINE_FACTORY", np_path.NumpyEngine)


def test_evaluate_batch_serves_a_stand_in_engine_point_by_point(oracle_engine, golden):
    from oracle import np_path
    prob, obj = problems.build("brachistochrone")
    X = golden("cfg_brachistochrone")["x"]
    assert X.shape[0] == 3
    p_before = prob.p.copy()
    res = prob.evaluate_batch(obj, X)
    assert np.array_equal(prob.p, p_before)
    F = np.stack([np_path.stacked_values(prob, obj, x) for x in X])
    m_eq = res.equality.shape[1]
    assert m_eq == np.atleast_1d(np_path.callbacks(prob, obj)[1](X[0])).size
    prob.p = p_before
    assert len(res) == 3 and res.cost.shape == (3,)
    assert np.array_equal(res.cost, F[:, 0])
    assert np.array_equal(res.equality, F[:, 1:1 + m_eq])
    assert np.array_equal(res.inequality, F[:, 1 + m_eq:])
    assert res.inequality.shape[1] == F.shape[1] - 1 - m_eq
    for k in range(3):
        want = np.sum(np.abs(F[k, 1:1 + m_eq])) + np.sum(np.maximum(-F[k, 1 + m_eq:], 0.0))
        assert res.violation[k] == want
    assert res.gradient is None and res.values is None and res.pattern is None
    # with the Jacobians: the stand-in's dense matrices, every entry a pattern entry
    lb, ub = np_path.bounds_arrays(prob)
    resj = prob.evaluate_batch(obj, X[:2], jacobian=True)
    indptr, rows = resj.pattern
    n, m = prob.number_of_variables, F.shape[1]
    assert resj.values.shape == (2, indptr[-1]) and rows.shape == (indptr[-1],)
    for k in range(2):
        F0, h, JT = np_path.sweep(prob, obj, X[k])
        assert np.array_equal(resj.steps[k], h) and np.array_equal(h, np_path.fd_step(X[k], lb, ub))
        assert np.array_equal(resj.gradient[k], JT[:, 0])
        dense = np.zeros((n, m))
        dense[np.repeat(np.arange(n), np.diff(indptr)), rows] = resj.values[k]
        assert np.array_equal(dense, JT)
        assert np.array_equal(resj.cost[k], F0[0])


def test_batch_part_cross_compiles_and_stays_out_of_the_default_build():
    prob, obj = problems.build("brachistochrone")
    header = codegen.emit_header(codegen.trace_problem(prob, obj))
    assert build.MODULE_PARTS == (0, 2, 3, 1), "the default list of parts of a module must not change"
    assert build.BATCH_PART not in build.MODULE_PARTS
    module = build.build_module(header)
    part = build.build_batch_part(header)
    assert os.path.exists(part) and part != module
    assert os.path.dirname(part) == os.path.dirname(module)
    assert part not in [build.part_path(module, i) for i in range(len(build.MODULE_PARTS))]
    assert build.build_batch_part(header) == part                  # cached
    # a gfx950 code object with both kernels in it ...
    with open(part, "rb") as fh:
        blob = fh.read()
    assert b"gfx950" in blob
    assert b"ogk_fused_batch" in blob and b"ogk_eval_batch" in blob
    # ... and the entry point the runtime looks up; the module's own parts do not carry the batch kernels
    lib = C.CDLL(part)
    assert hasattr(lib, "ogk_launch_batch") and hasattr(lib, "ogk_get_info")
    for i in range(len(build.MODULE_PARTS)):
        with open(build.part_path(module, i), "rb") as fh:
            assert b"ogk_fused_batch" not in fh.read()
    nm = subprocess.run(["nm", "-D", module], stdout=subprocess.PIPE, text=True)
    if nm.returncode == 0:
        assert "ogk_launch_batch" not in nm.stdout
