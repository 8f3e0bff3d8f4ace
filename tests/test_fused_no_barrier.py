"""The one-launch sweep (``ogk_fused``) at the shapes where its sweep workgroups can go wrong since their wavefronts do
not wait for each other at a staging barrier (``csrc/ogk_kernels.hip``: ``fz_stage_operands``, ``fz_service_tile``,
``fz_chain``): the item wavefronts of a light workgroup or heavy part put the operands into LDS and count up, the service
wavefront takes the D panel straight from memory and runs the chain in whole chunks padded with zero operands, the
hand-over words in LDS are cleared behind a barrier ahead of everything (LDS keeps what the previous launch left).  Bit
for bit against the dense form (``OGPSX_SWEEP=dense``) and against the CPU twin, on

* ``polar_tsto`` on ``[5, 7]``   - one partial tile, N no multiple of 4, phases of different length (the folded panel
  offset of the second phase),
* ``polar_tsto`` on ``[17, 33]`` - a second / third tile with a single live node, KS (5 and 9) no whole chunk of either
  chain (8 k-steps in the light workgroups and heavy parts, 10 in the tile workgroups),
* ``polar_tsto`` on ``[16, 16]`` - exact tiles,
* ``low_thrust`` on ``[11]`` and on ``[6]`` - a sequential sum: the workgroups that keep the barrier behind which the
  base terms are in LDS.  (The problem has one phase - ``nodes=[11, 6]`` is refused by its constructor - so the two
  lengths are two problems and both run.)

* ``launch4`` on ``[6, 5, 7, 5]`` - eight states (one more than a workgroup has item wavefronts: the service wavefront
  puts a slot of operands into LDS too), a sequential sum and four phases, i.e. a workgroup with the sum's barrier and a
  panel offset that is not zero.

``__graft_entry__.build`` compiles the modules and twins of ``SHAPES`` ahead of time; a test takes well under a second.
"""
import os

import numpy as np
import pytest

from opengoddard_amd import _native, problems

pytestmark = pytest.mark.gpu

# key -> (problem, nodes, state whose zero at BAD_NODE makes rows of F(x0) non-finite: the mass)
SHAPES = {"tsto-5-7": ("polar_tsto", [5, 7], 4),
          "tsto-17-33": ("polar_tsto", [17, 33], 4),
          "tsto-16-16": ("polar_tsto", [16, 16], 4),
          "low-thrust-11": ("low_thrust", [11], 6),
          "low-thrust-6": ("low_thrust", [6], 6),
          "launch4-6-5-7-5": ("launch4", [6, 5, 7, 5], 5)}
BAD_NODE = 2


def problem(key):
    name, nodes, _ = SHAPES[key]
    return problems.build(name, nodes=nodes)


class _Case:
    """One shape: the one-launch engine, and F / J_T of three points from the CPU twin and from the dense sweep -
    computed once, shared by the tests below, never written to."""

    def __init__(self, key):
        from opengoddard_amd.engine import HipEngine
        from oracle import np_path, twin
        self.prob, self.obj = problem(key)
        lb, ub = np_path.bounds_arrays(self.prob)
        before = os.environ.get("OGPSX_SWEEP")
        try:
            os.environ["OGPSX_SWEEP"] = "dense"
            dense = HipEngine(self.prob, self.obj)
            assert dense.sweep_mode == "dense"
            os.environ["OGPSX_SWEEP"] = "fused"
            self.eng = HipEngine(self.prob, self.obj)
            assert self.eng.sweep_mode == "fused" and self.eng.one_launch
        finally:
            if before is None:
                os.environ.pop("OGPSX_SWEEP", None)
            else:
                os.environ["OGPSX_SWEEP"] = before
        tw = twin.Twin(self.prob, self.obj, program=self.eng.program, header=self.eng.header)
        self.n, self.m = self.eng.n, self.eng.m
        ok = np.clip(self.prob.p, lb, ub)
        bad = ok.copy()
        bad[self.prob.index_states(SHAPES[key][2], 0, BAD_NODE)] = 0.0
        other = np.clip(ok + 1e-3 * np.random.default_rng(11).standard_normal(self.n), lb, ub)
        self.x = {"ok": ok, "bad": bad, "other": other}
        self.h = {k: _native.fd_step(v, lb, ub) for k, v in self.x.items()}
        self.want = {}
        for k in self.x:
            F_t, JT_t = tw.sweep(self.x[k], self.h[k])
            F_d, JT_d = dense.sweep_stacked(self.x[k], self.h[k])
            assert np.array_equal(F_d, F_t, equal_nan=True) and np.array_equal(JT_d, JT_t, equal_nan=True), \
                "the dense sweep and the CPU twin disagree at '%s'" % k
            self.want[k] = (F_t, JT_t)
        dense.close()
        assert np.isfinite(self.want["ok"][1]).all() and np.isfinite(self.want["other"][1]).all()
        assert not np.isfinite(self.want["bad"][0]).all() and np.isnan(self.want["bad"][1]).any()

    def cut(self):
        """(lo, hi), neither a multiple of 16: lo lies strictly inside a light workgroup's run of columns and strictly
        inside a column tile of a collocation slot, and so does hi (read from the program and the emitted tables)."""
        import re
        from opengoddard_amd import codegen
        src = codegen.emit_header(self.eng.program)
        body = re.search(r"OGT_LGRP\[\d+\] = \{(.*?)\n\};", src, re.S).group(1)
        runs = [[int(v) for v in re.findall(r"-?\d+", row)][:2] for row in re.findall(r"\{\{([^{}]*)\}\}", body)]
        slots = [(sl.leaf_base, sl.length) for sl in self.eng.program.mv]

        def inside_both(j):
            in_run = any(j0 < j < j0 + cnt for j0, cnt in runs)
            in_tile = any(leaf <= j < leaf + N and (j - leaf) % 16 != 0 for leaf, N in slots)
            return j % 16 != 0 and in_run and in_tile

        los = [j for j in range(1, self.n // 2) if inside_both(j)]
        his = [j for j in range(self.n - 1, self.n // 2, -1) if inside_both(j)]
        assert los and his, "no column of this shape cuts a light workgroup and a tile"
        return los[0], his[0]


_cases = {}


@pytest.fixture(scope="module", autouse=True)
def _close_engines():
    yield
    for done in _cases.values():
        done.eng.close()
    _cases.clear()


@pytest.fixture(params=sorted(SHAPES))
def case(request):
    if request.param not in _cases:
        _cases[request.param] = _Case(request.param)
    return _cases[request.param]


def _device(case, key):
    import torch
    dev = torch.device("cuda", 0)
    return torch.from_numpy(case.x[key]).to(dev), torch.from_numpy(case.h[key]).to(dev)


def test_full_range_is_the_dense_sweep_and_the_twin(case):
    """All columns, three times on one handle (the second and third launch find the LDS of the first as it left it)."""
    for _ in range(3):
        F0, JT = case.eng.sweep_stacked(case.x["ok"], case.h["ok"])
        assert np.array_equal(F0, case.want["ok"][0])
        assert np.array_equal(JT, case.want["ok"][1])
    assert (case.want["ok"][1] != 0).any()


def test_column_block_that_cuts_a_light_workgroup_and_a_tile(case):
    """og_fd_sweep_dev on [lo, hi) into a registered block: the lanes of the cut workgroups that lie outside write
    nothing, the ones inside write what the full sweep writes."""
    import torch
    lo, hi = case.cut()
    assert lo % 16 and hi % 16 and 0 < lo < hi < case.n
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream().cuda_stream
    d_F = torch.empty(case.m, dtype=torch.float64, device=dev)
    block = torch.full((hi - lo, case.m), -3.0, dtype=torch.float64, device=dev)
    case.eng.register_jt_dev(block.data_ptr(), lo, hi, stream)
    try:
        for key in ("ok", "other"):
            d_x, d_h = _device(case, key)
            case.eng.sweep_dev(d_x.data_ptr(), d_h.data_ptr(), lo, hi, block.data_ptr(), d_F.data_ptr(), stream)
            torch.cuda.synchronize()
            assert np.array_equal(d_F.cpu().numpy(), case.want[key][0])
            assert np.array_equal(block.cpu().numpy(), case.want[key][1][lo:hi]), "block [%d, %d) at '%s'" % (lo, hi, key)
    finally:
        case.eng.unregister_jt_dev(block.data_ptr())


def test_non_finite_point_then_a_finite_point_on_one_registered_buffer(case):
    """F(x0) with non-finite rows: NaN in those rows of every column, around what the sweep workgroups write; the
    finite point after it finds the buffer cleaned."""
    import torch
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream().cuda_stream
    d_F = torch.empty(case.m, dtype=torch.float64, device=dev)
    d_JT = torch.full((case.n, case.m), 7.0, dtype=torch.float64, device=dev)
    case.eng.register_jt_dev(d_JT.data_ptr(), 0, case.n, stream)
    try:
        for key in ("ok", "bad", "bad", "ok", "other"):
            d_x, d_h = _device(case, key)
            case.eng.sweep_dev(d_x.data_ptr(), d_h.data_ptr(), 0, case.n, d_JT.data_ptr(), d_F.data_ptr(), stream)
            torch.cuda.synchronize()
            assert np.array_equal(d_F.cpu().numpy(), case.want[key][0], equal_nan=True), key
            assert np.array_equal(d_JT.cpu().numpy(), case.want[key][1], equal_nan=True), key
    finally:
        case.eng.unregister_jt_dev(d_JT.data_ptr())


def test_two_consecutive_launches_into_two_buffers(case):
    """Back to back, nothing in between: whatever the first launch's workgroups left in LDS is what the second
    launch's workgroups start on."""
    import torch
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream().cuda_stream
    keys = ("ok", "other")
    d_F = [torch.empty(case.m, dtype=torch.float64, device=dev) for _ in keys]
    d_JT = [torch.full((case.n, case.m), 5.0 + i, dtype=torch.float64, device=dev) for i in range(len(keys))]
    args = [_device(case, key) for key in keys]
    for buf in d_JT:
        case.eng.register_jt_dev(buf.data_ptr(), 0, case.n, stream)
    try:
        for _ in range(2):
            for (d_x, d_h), F, JT in zip(args, d_F, d_JT):
                case.eng.sweep_dev(d_x.data_ptr(), d_h.data_ptr(), 0, case.n, JT.data_ptr(), F.data_ptr(), stream)
            torch.cuda.synchronize()
            for key, F, JT in zip(keys, d_F, d_JT):
                assert np.array_equal(F.cpu().numpy(), case.want[key][0]), key
                assert np.array_equal(JT.cpu().numpy(), case.want[key][1]), key
    finally:
        for buf in d_JT:
            case.eng.unregister_jt_dev(buf.data_ptr())
