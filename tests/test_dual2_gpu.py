"""csrc/og_dual2.h on the device: every rule, in every form, on the records of tests/test_dual2_seeds.py - every zero /
non-zero pattern of the seeds at interior points, the ill-conditioned and edge points, and the og_math case table with
one seed slot zero - gives on gfx950 the bits of the host build (g++), in all eight outputs: the rule's v, d1, d2, dd and
og_dual.h's (v, d) on the two projections.  NaN equals NaN whatever its payload; the sign of zero counts.  With
tests/test_dual2_seeds.py (the host build against the closed-form truth) this gives the device the accuracy results, and
it pins "same source for hipcc and a host compiler" for the rules the five generated headers of
adjoint_cases.GPU_KEYS never call.

The probe (tests/og_dual2_probe.hip) is compiled with build.HIP_FLAGS unchanged, once per content of its sources, next to
the other JIT products; tests/test_dual2_seeds.py cross-compiles it on a machine without a GPU.  One process; a launch
that reports a HIP error stops everything after it (nothing is retried)."""
import numpy as np
import pytest

import dual2_seed_cases as cases
from conftest import record_measurement
from dual2_seed_cases import same_bits

pytestmark = pytest.mark.gpu

BLOCKS = (64, 512)              # one wavefront; the sweep kernels' workgroup
_STATE = {"error": None}


@pytest.fixture(scope="module")
def builds():
    hip, gxx = cases.load("hip"), cases.load("gxx")
    assert hip.lib.og2p_device_count() > 0, "the probe sees no HIP device"
    return hip, gxx


def orders(name, args):
    """table order, sorted by the branch taken and the terms left out (wavefronts uniform), shuffled (neighbouring lanes
    diverge)"""
    n = len(args)
    return (("table", np.arange(n)), ("sorted by branch and seed mask", np.argsort(cases.branch_key(name, args), kind="stable")),
            ("shuffled", np.random.default_rng(99).permutation(n)))


def run_device(hip, name, form, args, block):
    if _STATE["error"]:
        pytest.fail("not launched: an earlier launch failed (%s)" % _STATE["error"])
    err, out = hip.device(name, form, args, block)
    if err != 0:
        _STATE["error"] = "%s form %d, workgroup %d: HIP error %d" % (name, form, block, err)
        pytest.fail(_STATE["error"])
    return out


def compare(builds, name, form, args, totals):
    """one group, three orders, two workgroup sizes -> the number of records whose bits differ from the g++ host build's"""
    hip, gxx = builds
    assert len(args) % 64 != 0                  # a partial wavefront at the end
    want = gxx.host(name, form, args)
    clang = int((~same_bits(hip.host(name, form, args), want).all(axis=1)).sum())      # clang's host half of the module
    differ, where = 0, []
    for order, perm in orders(name, args):
        for block in BLOCKS:
            out = run_device(hip, name, form, np.ascontiguousarray(args[perm]), block)
            back = np.empty_like(out)
            back[perm] = out
            bad = ~same_bits(back, want).all(axis=1)
            if bad.any():
                i = np.flatnonzero(bad)[0]
                where.append("%s order, workgroup %d: %d differ, first at %r: device %r host %r" % (
                    order, block, bad.sum(), args[i].tolist(), back[i].tolist(), want[i].tolist()))
            differ += int(bad.sum())
    entry = totals.setdefault(name, {"inputs": 0, "differ": 0, "clang_differ": 0, "launches": 0})
    entry["inputs"] += len(args)
    entry["differ"] += differ
    entry["clang_differ"] += clang
    entry["launches"] += 3 * len(BLOCKS)
    assert not where, "%s form %d: %s" % (name, form, "; ".join(where[:3]))
    assert clang == 0, "%s form %d: g++ and clang++ host halves differ at %d records" % (name, form, clang)


def _run(builds, test, sections):
    totals = {}
    try:
        for name, form, args in cases.device_groups(sections):
            compare(builds, name, form, args, totals)
    finally:
        record_measurement(test, orders=3, workgroups=list(BLOCKS), ops=len(totals),
                           launches=sum(v["launches"] for v in totals.values()),
                           inputs_per_op={k: v["inputs"] for k, v in totals.items()},
                           differing={k: v["differ"] for k, v in totals.items()},
                           differing_total=sum(v["differ"] for v in totals.values()),
                           host_compilers_differing_total=sum(v["clang_differ"] for v in totals.values()))
    assert len(totals) == len(cases.PROBE_OPS) and all(v["differ"] == 0 and v["clang_differ"] == 0 for v in totals.values())


def test_device_bits_equal_host_bits_under_every_seed_mask_and_at_the_edges(builds):
    """sections 2.1 and 2.2 of tests/test_dual2_seeds.py: some seeds zero and others not, -0.0 / inf / NaN seeds, the
    ill-conditioned and edge points"""
    _run(builds, "test_device_bits_equal_host_bits_under_every_seed_mask_and_at_the_edges", ("seeds",))


def test_device_bits_equal_host_bits_over_the_case_table_with_one_seed_slot_zero(builds):
    """section 2.3: the og_math case table (every branch and special value of the functions behind the rules) under the
    two seed patterns of the kernels; the exact zeros of dd are the host's, so they are the device's"""
    _run(builds, "test_device_bits_equal_host_bits_over_the_case_table_with_one_seed_slot_zero", ("zeros",))
