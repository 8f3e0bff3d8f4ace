"""Exact Jacobians of a batch of points (``og_jacobian_exact_batch*``, ``BatchSweep.exact``,
``Problem.evaluate_batch(jacobian="exact")``): everything that can be checked without a GPU - the validation of the
``jacobian`` argument, the host logic with stand-in engines (the NumPy oracle, and the oracle with the CPU twin's exact
derivatives added), the C ABI's declarations and error paths, and the cross-compilation of the kernel as a module part
of its own."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from opengoddard_amd import _native, build, codegen, problems
from opengoddard_amd import optimize as og

EXACT_BATCH_FUNCTIONS = ("og_jacobian_exact_batch_load", "og_jacobian_exact_batch_dev", "og_jacobian_exact_batch")


@pytest.fixture
def no_engine(monkeypatch):
    """Any attempt to build an engine fails the test: the argument checks come first."""
    def factory(prob, obj):
        raise AssertionError("an engine was built before the arguments were checked")
    monkeypatch.setattr(og, "ENGINE_FACTORY", factory)


def test_evaluate_batch_validates_the_jacobian_option_before_it_builds_an_engine(no_engine, golden):
    prob, obj = problems.build("brachistochrone")
    X = golden("cfg_brachistochrone")["x"]
    with pytest.raises(ValueError, match="jacobian must be 'fd' or 'exact', got 'analytic'"):
        prob.evaluate_batch(obj, X, jacobian="analytic")
    with pytest.raises(ValueError, match="jacobian"):
        prob.evaluate_batch(obj, X, jacobian="")                  # a string is never taken for a truth value
    # the valid spellings get as far as the engine
    for mode in ("fd", "exact", True, False, None):
        with pytest.raises(AssertionError, match="an engine was built"):
            prob.evaluate_batch(obj, X, jacobian=mode)


def test_an_engine_without_an_exact_mode_says_so_and_fd_is_what_true_means(monkeypatch, golden):
    from oracle import np_path
    assert not hasattr(np_path.NumpyEngine, "exact_stacked")
    monkeypatch.setattr(og, "ENGINE_FACTORY", np_path.NumpyEngine)
    prob, obj = problems.build("brachistochrone")
    X = golden("cfg_brachistochrone")["x"]
    p_before = prob.p.copy()
    with pytest.raises(ValueError, match="this engine has no exact-Jacobian mode"):
        prob.evaluate_batch(obj, X, jacobian="exact")
    assert np.array_equal(prob.p, p_before)
    by_name, by_truth = prob.evaluate_batch(obj, X, jacobian="fd"), prob.evaluate_batch(obj, X, jacobian=True)
    assert by_name.jacobian == by_truth.jacobian == "fd"
    for field in ("cost", "equality", "inequality", "violation", "nonfinite", "gradient", "values", "steps"):
        assert np.array_equal(getattr(by_name, field), getattr(by_truth, field)), field
    assert all(np.array_equal(a, b) for a, b in zip(by_name.pattern, by_truth.pattern))
    plain = prob.evaluate_batch(obj, X)
    assert plain.jacobian is None and plain.values is None and plain.steps is None


@pytest.mark.parametrize("name", ["brachistochrone", "goddard"])
def test_a_stand_in_engine_with_an_exact_mode_is_served_point_by_point(name, monkeypatch, golden):
    from oracle import np_path, twin

    class ExactOracle(np_path.NumpyEngine):
        """The NumPy oracle plus the exact mode of the CPU twin (the generated code on dual numbers)."""

        def __init__(self, prob, obj):
            super().__init__(prob, obj)
            self.twin = twin.Twin(prob, obj)
            self.calls = 0

        def exact_stacked(self, x):
            self.calls += 1
            return self.twin.exact(x)

    monkeypatch.setattr(og, "ENGINE_FACTORY", ExactOracle)
    prob, obj = problems.build(name)
    X = np.ascontiguousarray(golden("cfg_" + name)["x"])
    p_before = prob.p.copy()
    res = prob.evaluate_batch(obj, X, jacobian="exact")
    assert np.array_equal(prob.p, p_before)
    assert res.jacobian == "exact" and res.steps is None and len(res) == 3
    assert prob._engine.calls == 3
    tw = twin.Twin(prob, obj)
    indptr, rows = res.pattern
    n, m = tw.n, tw.m
    assert res.values.shape == (3, indptr[-1])
    for k in range(3):
        F0, JT = tw.exact(X[k])
        dense = np.zeros((n, m))
        dense[np.repeat(np.arange(n), np.diff(indptr)), rows] = res.values[k]
        assert np.array_equal(dense, JT)
        assert np.array_equal(res.gradient[k], JT[:, 0])
        assert res.cost[k] == F0[0]
        assert np.array_equal(res.equality[k], F0[1:1 + tw.m_eq]) and np.array_equal(res.inequality[k], F0[1 + tw.m_eq:])
    # not the forward differences under another name
    fd = prob.evaluate_batch(obj, X, jacobian=True)
    assert fd.jacobian == "fd" and fd.steps is not None and not np.array_equal(fd.values, res.values)


def _declared_in_header():
    with open(os.path.join(ROOT, "include", "ogpsx.h")) as fh:
        text = re.sub(r"/\*.*?\*/", "", fh.read(), flags=re.S)
    return set(re.findall(r"\b(og_jacobian_exact_batch[a-z_]*)\s*\(", text))


def test_library_exports_the_exact_batch_functions_the_header_declares():
    assert _declared_in_header() == set(EXACT_BATCH_FUNCTIONS)
    lib = _native.lib()
    for name in EXACT_BATCH_FUNCTIONS:
        assert name in _native.SIGNATURES, name + " has no ctypes signature"
        fn = getattr(lib, name)                       # AttributeError: not exported
        assert fn.argtypes == _native.SIGNATURES[name][1]

    def error_text():
        msg = lib.og_last_error()
        return msg.decode() if msg else ""

    x = np.zeros(4)
    ptr = _native.dptr(x)
    calls = {
        "og_jacobian_exact_batch_load": lambda: lib.og_jacobian_exact_batch_load(None, b"/nonexistent.so"),
        "og_jacobian_exact_batch_dev": lambda: lib.og_jacobian_exact_batch_dev(None, 1, 8, 8, None, None),
        "og_jacobian_exact_batch": lambda: lib.og_jacobian_exact_batch(None, 1, ptr, ptr, ptr, None),
    }
    for name, call in calls.items():
        assert call() != 0, name
        text = error_text()
        assert text.startswith(name + ":") and "null batch" in text


def test_exact_batch_part_cross_compiles_as_a_part_of_its_own():
    prob, obj = problems.build("brachistochrone")
    header = codegen.emit_header(codegen.trace_problem(prob, obj))
    assert build.MODULE_PARTS == (0, 2, 3, 1) and build.BATCH_PART == 4
    assert build.BATCH_EXACT_PART not in build.MODULE_PARTS and build.BATCH_EXACT_PART != build.BATCH_PART
    module = build.build_module(header)
    batch_part = build.build_batch_part(header)
    part = build.build_batch_exact_part(header)
    assert part == build.batch_exact_part_path(module) and part.endswith(".batchx.so")
    assert os.path.exists(part) and os.path.dirname(part) == os.path.dirname(module)
    others = [build.part_path(module, i) for i in range(len(build.MODULE_PARTS))] + [batch_part]
    assert part not in others
    stamp = os.path.getmtime(part)
    assert build.build_batch_exact_part(header) == part and os.path.getmtime(part) == stamp      # cached
    with open(part, "rb") as fh:
        blob = fh.read()
    assert b"gfx950" in blob and b"ogk_exact_struct_batch" in blob
    assert b"ogk_fused_batch" not in blob and b"ogk_eval_batch" not in blob
    lib = C.CDLL(part)
    assert hasattr(lib, "ogk_launch_batch") and hasattr(lib, "ogk_get_info")
    # what a user who never asks for a batched exact Jacobian builds and loads does not carry the kernel
    for path in others:
        with open(path, "rb") as fh:
            assert b"ogk_exact_struct_batch" not in fh.read(), path
