"""csrc/og_math.h and csrc/og_dual.h on the device: every function, plain and on dual numbers, over the whole case
table (tests/og_math_cases.py) and the random distributions of tests/test_og_math.py - the bits of the gfx950 build
equal the bits of the host build (g++, the twin's compiler), where NaN equals NaN whatever its payload and the sign of
zero counts.  With tests/test_og_math_edges.py (the host build against mpmath) this gives the device the accuracy
results without running mpmath on it.

The probe (tests/og_math_probe.hip) is compiled with build.HIP_FLAGS unchanged - what the product's modules get - once
per content of its sources, next to the other JIT products; tests/test_og_math_edges.py cross-compiles it on a machine
without a GPU.  One process; a launch that reports a HIP error stops everything after it (nothing is retried)."""
import numpy as np
import pytest

import og_math_cases as cases
from conftest import record_measurement
from og_math_cases import same_bits

pytestmark = pytest.mark.gpu

BLOCKS = (64, 512)              # one wavefront; the sweep kernels' workgroup
_STATE = {"error": None}


@pytest.fixture(scope="module")
def builds():
    hip, gxx = cases.load("hip"), cases.load("gxx")
    assert hip.lib.ogp_device_count() > 0, "the probe sees no HIP device"
    return hip, gxx


def branch_key(name, a):
    """the index of the interval between the thresholds of ``name`` that |a| falls in, with sign and NaN apart: inputs of
    one key take the same branches, so sorting by it makes the wavefronts uniform"""
    cuts = np.unique(np.abs(np.array(cases.THRESHOLDS.get(name, []) + [0.0, cases.DBL_MIN, 1.0, np.inf])))
    return np.searchsorted(cuts, np.abs(a), side="right") * 4 + np.signbit(a) * 2 + np.isnan(a)


def orders(name, a, b):
    """table order, sorted by the branch taken (wavefronts uniform), shuffled (neighbouring lanes diverge)"""
    n = a.size
    key = branch_key(name, a) if b is None else branch_key(name, a) * 4096 + branch_key(name, b)
    return (("table", np.arange(n)), ("sorted by branch", np.argsort(key, kind="stable")),
            ("shuffled", np.random.default_rng(99).permutation(n)))


def run_device(hip, label, name, variant, a, b, da, db, tab, block):
    if _STATE["error"]:
        pytest.fail("not launched: an earlier launch failed (%s)" % _STATE["error"])
    err, v, d = hip.device(name, a, b, da, db, variant, tab, block)
    if err != 0:
        _STATE["error"] = "%s, workgroup %d: HIP error %d" % (label, block, err)
        pytest.fail(_STATE["error"])
    return v, d


def compare(builds, label, name, variant, a, b, da, db, tab, totals, guard=None):
    """one array, three orders, two workgroup sizes -> the number of results whose bits differ from the host's"""
    hip, gxx = builds
    if a.size % 64 == 0:                        # partial wavefronts: never a multiple of 64
        cut = lambda v: None if v is None else v[:-1]
        a, b, da, db = a[:-1], cut(b), cut(da), cut(db)
    hv, hd = gxx.host(name, a, b, da, db, variant, tab)
    cv, cd = hip.host(name, a, b, da, db, variant, tab)          # clang's host half of the same module
    differ = int((~(same_bits(hv, cv) & same_bits(hd, cd))).sum())
    where = []
    for order, perm in orders(name, a, b):
        take = lambda v: None if v is None else np.ascontiguousarray(v[perm])
        for block in BLOCKS:
            v, d = run_device(hip, label, name, variant, take(a), take(b), take(da), take(db), tab, block)
            back = np.empty_like(v), np.empty_like(d)
            back[0][perm], back[1][perm] = v, d
            bad = ~(same_bits(back[0], hv) & same_bits(back[1], hd))
            if bad.any():
                i = np.flatnonzero(bad)[0]
                where.append("%s order, workgroup %d: %d differ, first at a=%r b=%r: device (%r, %r) host (%r, %r)" % (
                    order, block, bad.sum(), a[i], None if b is None else b[i], back[0][i], back[1][i], hv[i], hd[i]))
            differ += int(bad.sum())
    entry = totals.setdefault(label.split(" ")[0] + (" dual" if variant else ""), {"inputs": 0, "differ": 0})
    entry["inputs"] += int(a.size)
    entry["differ"] += differ
    assert not where, "%s%s: %s" % (label, " [%s]" % guard if guard else "", "; ".join(where[:3]))
    assert differ == 0, "%s: g++ and clang++ host halves differ" % label


def test_device_bits_equal_host_bits_over_the_case_table(builds):
    totals = {}
    try:
        for label, name, variant, a, b, da, db, tab in cases.all_cases():
            compare(builds, label, name, variant, a, b, da, db, tab, totals)
    finally:
        record_measurement("test_device_bits_equal_host_bits_over_the_case_table", orders=3, workgroups=list(BLOCKS),
                           functions=len(totals), inputs_per_function={k: v["inputs"] for k, v in totals.items()},
                           differing={k: v["differ"] for k, v in totals.items()},
                           differing_total=sum(v["differ"] for v in totals.values()))
    assert len(totals) >= 27 + 26 and all(v["differ"] == 0 for v in totals.values())


def test_device_bits_equal_host_bits_over_the_random_distributions(builds):
    """the samples tests/test_og_math.py compares with NumPy on the host: 200 000 - 300 000 points each"""
    totals = {}
    try:
        for name in cases.FUNCS:
            for k, (a, b) in enumerate(cases.random_inputs(name)):
                compare(builds, "%s random %d" % (name, k), name, 0, a, b, None, None, None, totals)
                if name in cases.DUAL_ONE:
                    compare(builds, "%s random %d dual" % (name, k), name, 1, a, b, np.ones(a.size), None, None, totals)
                if name in cases.DUAL_TWO:
                    compare(builds, "%s random %d dual" % (name, k), name, 1, a, b, np.ones(a.size),
                            np.full(a.size, -0.5), None, totals)
    finally:
        record_measurement("test_device_bits_equal_host_bits_over_the_random_distributions", orders=3,
                           workgroups=list(BLOCKS), functions=len(totals),
                           inputs_per_function={k: v["inputs"] for k, v in totals.items()},
                           differing={k: v["differ"] for k, v in totals.items()},
                           differing_total=sum(v["differ"] for v in totals.values()))
    assert len(totals) >= 2 * 21 and all(v["differ"] == 0 for v in totals.values())


def test_float_to_int_casts_agree_behind_their_guards(builds):
    """An out-of-range float-to-int cast saturates differently on x86 and on gfx950, so every such cast in og_math.h
    stands behind a guard: the inputs just inside and outside each guard give the host's bits on the device (the guard
    is named when they do not)."""
    totals = {}
    for guard, name, xs in cases.CAST_GUARDS:
        a = cases.neighbours(xs, 2)
        compare(builds, "%s casts" % name, name, 0, a, None, None, None, None, totals, guard)
        compare(builds, "%s casts dual" % name, name, 1, a, None, np.ones(a.size), None, None, totals, guard)
    ys = np.concatenate([cases.neighbours(cases.POW_CAST_Y, 1), np.arange(-70.0, 71.0)])
    xs = np.array([-2.0, 2.0, -1.0, -0.5, -1.0 - cases.EPS, -0.0, 0.0, -np.inf, 1.0 + cases.EPS])
    a, b = [g.ravel() for g in np.meshgrid(xs, ys, indexing="ij")]
    guard = "pow_: (int)y behind |y| <= 64, (long long)y behind |y| < 2^53"
    compare(builds, "pow casts", "pow", 0, a, b, None, None, None, totals, guard)
    compare(builds, "pow casts dual", "pow", 1, a, b, np.ones(a.size), np.ones(a.size), None, totals, guard)
    a, k = cases.table("scalb")
    compare(builds, "scalb casts", "scalb", 0, a, k, None, None, None, totals, "scalb_: the table keeps |k| <= 2100")
    record_measurement("test_float_to_int_casts_agree_behind_their_guards",
                       inputs_per_function={k: v["inputs"] for k, v in totals.items()},
                       differing_total=sum(v["differ"] for v in totals.values()))
