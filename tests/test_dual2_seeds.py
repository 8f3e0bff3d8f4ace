"""csrc/og_dual2.h where the kernels use it and tests/test_hessian.py does not look: second-order duals some of whose
seeds are zero and others not (OgHvpX seeds a leaf as (x_i, i == j, v_i, 0), og_mix.h seeds slot 2 of one table entry, so
almost every intermediate is such a number), arguments at the edges of the rules, and the whole og_math case table with
one seed slot zero.  No GPU: the g++ build of tests/og_dual2_probe.hip, ROCm's clang++ build of it and the stand-alone
tests/dual2_probe.cpp (g++, clang++, g++ under AddressSanitizer / UBSan), all of which must give the same bits.

The truth is closed-form partial derivatives in mpmath at 50 digits (dual2_seed_cases.partials), the unit that of
hessian_cases.rule_truth, the bound test_hessian.RULE_BOUNDS - or, where a record's own conditioning puts that out of
reach, four times the error of the same closed form in float64 at that record (dual2_seed_cases.bounds).  Figures:
profiles/dual2_seeds.md (``python tests/dual2_seed_cases.py --report``).

What these tests found in the header as it was (both fixed with them): pow_ gave dd = NaN at x = 0 with the exponent 1
(0 * inf in the curvature term, whose coefficient y (y - 1) is 0), and hypot_ formed its mixed part as the difference of
two numbers that agree to (y/x)^2, so it lost it where one argument is constant or dominant.
"""
import ctypes as C

import numpy as np
import pytest

import dual2_seed_cases as cases
import hessian_cases as hc
import og_math_cases
from dual2_seed_cases import same_bits


@pytest.fixture(scope="module")
def probe():
    return cases.load("gxx")


@pytest.fixture(scope="module")
def probe_dir(tmp_path_factory):
    return str(tmp_path_factory.mktemp("dual2_seeds"))


_JUDGED = {}


def judged(probe, which):
    """records, results, errors, the reference's errors and claims of one section: computed once, shared, left unchanged"""
    if which not in _JUDGED:
        if which == "lattice":
            spec = cases.special_seed_records()
            records = np.concatenate([cases.lattice_records(), spec[np.isfinite(spec).all(axis=1)]])
            pin = np.zeros(len(records), dtype=bool)
        else:
            records, pin = cases.edge_records()
        got = probe.run(records)
        err, ref, claim = cases.judge(records, got)
        for v in (records, pin, got, err, ref, claim):
            v.setflags(write=False)
        _JUDGED[which] = records, pin, got, err, ref, claim
    return _JUDGED[which]


def assert_rule_a(records, got):
    """the projections (v, d1) and (v, d2) are og_dual.h's results on the projections of the arguments, bit for bit"""
    bad = ~(same_bits(got[:, 0], got[:, 4]) & same_bits(got[:, 1], got[:, 5]) & same_bits(got[:, 0], got[:, 6]) &
            same_bits(got[:, 2], got[:, 7]))
    assert not bad.any(), "rule (a) broken at %d records, first %r -> %r" % (bad.sum(), records[bad][0], got[bad][0])


def assert_accurate(records, pin, got, err, ref, claim):
    bnd = cases.bounds(records, ref)
    over = claim & ~pin[:, None] & ~(err <= bnd)
    if over.any():
        worst = {}
        for i, k in zip(*np.nonzero(over)):
            name = cases.PROBE_OPS[int(records[i, 0])]
            if name not in worst or err[i, k] > worst[name][0]:
                worst[name] = (err[i, k], bnd[i, k], ref[i, k], ("v", "d1", "d2", "dd")[k], records[i].tolist(), got[i, :4].tolist())
        text = "; ".join("%s: %s error %.3g, bound %.3g (float64 closed form: %.3g) at %r -> %r" % ((n,) + (w[3], w[0], w[1], w[2], w[4], w[5]))
                         for n, w in sorted(worst.items()))
        pytest.fail("%d parts of %d records beyond their bound; worst per op: %s" % (over.sum(), over.any(axis=1).sum(), text))


# --------------------------------------------------------------------------------------------- 2.1 the seed lattice
def test_the_probe_and_the_cases_name_the_same_ops(probe):
    assert cases.PROBE_OPS[:cases.STANDALONE_OPS] == hc.OPS and cases.PROBE_OPS[cases.STANDALONE_OPS:] == ["interp2"]
    assert probe.lib.og2p_count() == len(cases.PROBE_OPS)              # (load() compared the names both ways)
    rec = cases.lattice_records()
    assert set(cases.PROBE_OPS[int(c)] for c in rec[:, 0]) == set(cases.PROBE_OPS)
    patterns = set(tuple(r != 0.0) for r in rec[rec[:, 1] == 0][:, [3, 4, 5]])
    assert len(patterns) == 8 and len(rec) >= 6360


def test_projections_are_og_duals_bits_under_every_seed_mask(probe):
    records, _, got, _, _, _ = judged(probe, "lattice")
    assert_rule_a(records, got)
    spec = cases.special_seed_records()                                # -0.0, inf and NaN seeds as well
    assert not np.isfinite(spec).all() and np.signbit(spec[:, 3:6][spec[:, 3:6] == 0.0]).any()
    assert_rule_a(spec, probe.run(spec))


def test_every_part_against_the_closed_form_truth_under_every_seed_mask(probe):
    records, pin, got, err, ref, claim = judged(probe, "lattice")
    outside = (records[:, 0] == cases.PROBE_OPS.index("interp2")) & ((records[:, 2] < hc.XG[0]) | (records[:, 2] > hc.XG[-1]))
    assert outside.sum() >= 2 * 8 and np.isnan(got[outside, 0]).all()      # mode 2 beyond the table: NaN, slope 0
    assert claim[:, 1:].all() and claim[~outside, 0].all(), "an interior point whose truth is not finite"
    assert np.isfinite(got[~outside]).all() and np.isfinite(got[outside][:, [1, 2, 3, 5, 7]]).all()
    assert_accurate(records, pin, got, err, ref, claim)


def test_a_left_out_term_is_left_out_whatever_the_other_seeds_are(probe):
    """rule (b) on the lattice: where the seeds of one slot are zero in every argument the form reads, that slot of the
    result is exactly 0, and where the dd of those arguments are zero as well, so is the result's dd - whatever the
    other slot holds."""
    records, _, got, _, _, _ = judged(probe, "lattice")
    binary = np.isin(records[:, 0], [cases.PROBE_OPS.index(n) for n in cases.BINARY])
    reads_a, reads_b = ~binary | (records[:, 1] != 2), binary & (records[:, 1] != 1)
    zero = lambda col_a, col_b: (~reads_a | (records[:, col_a] == 0.0)) & (~reads_b | (records[:, col_b] == 0.0))
    for slot in (0, 1):
        zeroed = zero(3 + slot, 7 + slot)
        assert zeroed.sum() > 1000 and np.all(got[zeroed, 1 + slot] == 0.0)
        both = zeroed & zero(5, 9)
        assert both.sum() > 500 and np.all(got[both, 3] == 0.0)


def test_the_stand_alone_probe_gives_the_same_bits_under_three_builds(probe, probe_dir):
    """tests/dual2_probe.cpp - the program that runs under AddressSanitizer / UBSan - on the records of 2.1 and 2.2"""
    spec = cases.special_seed_records()
    records = np.concatenate([cases.lattice_records(), spec, cases.edge_records()[0]])
    records = records[records[:, 0] < cases.STANDALONE_OPS]
    want = probe.run(records)
    builds = (("g++", False), (og_math_cases.clangxx(), False), ("g++", True))
    for compiler, sanitize in builds:
        exe = hc.build_rules_probe(probe_dir, compiler, sanitize=sanitize)
        got = hc.run_rules_probe(exe, probe_dir, records, "seeds")
        bad = ~same_bits(got, want).all(axis=1)
        assert not bad.any(), "%s%s: %d records differ, first %r: %r, the .hip probe's host loop %r" % (
            compiler, " (sanitized)" if sanitize else "", bad.sum(), records[bad][0], got[bad][0], want[bad][0])


# --------------------------------------------------------------------------------------------- 2.2 the edges
def test_rule_a_and_accuracy_at_the_ill_conditioned_and_edge_points(probe):
    records, pin, got, err, ref, claim = judged(probe, "edges")
    names = set(n for n, *_ in cases.edge_points())
    assert {"hypot", "atan2", "pow", "sqrt", "cbrt", "log", "tan", "fabs", "max", "min", "mod", "fmod", "interp0", "interp1",
            "interp2"} <= names
    assert_rule_a(records, got)
    assert claim[~pin].any(axis=1).all() and claim[~pin, 0].sum() > 0.9 * (~pin).sum()
    assert_accurate(records, pin, got, err, ref, claim)


def test_hypot_keeps_its_mixed_part_next_to_a_dominant_argument(probe):
    """hypot(x, 1e-8) at x = 1, the smoothed |x|: dd = c^2 d1 d2 / h^3 is 1e-16 of the seeds' product and was returned
    as exactly 0; and the two records of the issue that started this file."""
    import mpmath as mp
    args = np.array([[1.0, 0.75, -1.25, 0.0, 1e-8, 0.0, 0.0, 0.0], [-3.0, 0.75, -1.25, 0.0, 0.25, 0.0, 0.0, 0.0]])
    got = probe.host("hypot", 1, args)
    with mp.workdps(50):
        for a, g in zip(args, got):
            x, c = mp.mpf(float(a[0])), mp.mpf(float(a[4]))
            want = c * c * mp.mpf(float(a[1])) * mp.mpf(float(a[2])) / mp.hypot(x, c) ** 3
            assert g[3] != 0.0 and abs(mp.mpf(float(g[3])) - want) <= 4 * 2.0 ** -52 * abs(want), (a, g, want)
    # far from 1 nothing underflows or overflows on the way
    far = np.array([[s * 1e-200, 0.75, -1.25, 0.4375, 1e-200, -0.625, 1.5, -0.3125] for s in (1.0, -1.0)] +
                   [[s * 1e200, 0.75, -1.25, 0.4375, 1e200, -0.625, 1.5, -0.3125] for s in (1.0, -1.0)])
    out = probe.host("hypot", 0, far)
    assert np.isfinite(out).all() and (out[:, 3] != 0.0).all()


def test_pow_at_a_zero_base(probe):
    """x ** y at x = 0.  y constant: x ** 1 is x (dd = x.dd, not 0 * inf), x ** 2 has curvature 2, x ** 3 none.  y seeded:
    the parts with log x stay out where x ** y is 0, as og_dual.h has them - dd is what the same call gives with the
    seeds of y zeroed, bit for bit."""
    x = [0.0, 0.75, -1.25, 0.3]
    for form in (0, 1):
        got = probe.host("pow", form, np.array([x + [y, 0.0, 0.0, 0.0] for y in (1.0, 2.0, 3.0)]))
        assert np.array_equal(got[:, :4], [[0.0, 0.75, -1.25, 0.3], [0.0, 0.0, 0.0, 2.0 * 0.75 * -1.25], [0.0, 0.0, 0.0, 0.0]])
    seeded = np.array([x + [y, -0.625, 1.5, -0.3125] for y in (1.0, 2.0, 3.0, 0.5)])
    plain = seeded.copy()
    plain[:, 5:] = 0.0
    assert same_bits(probe.host("pow", 0, seeded), probe.host("pow", 0, plain)).all()
    # where og_dual.h's own slope is not finite (x ** 0.5 and x ** 0 at 0) nothing is claimed but its bits
    got = probe.host("pow", 1, np.array([x + [0.5, 0.0, 0.0, 0.0], x + [0.0, 0.0, 0.0, 0.0]]))
    assert same_bits(got[:, 1], got[:, 5]).all() and same_bits(got[:, 2], got[:, 7]).all()


def test_piecewise_linear_ops_on_their_kinks_ties_and_jumps(probe):
    seeds = [0.75, -1.25, 0.4375]
    got = probe.host("fabs", 0, np.array([[0.0] + seeds + [0.0] * 4, [-0.0] + seeds + [0.0] * 4]))
    assert np.all(got[:, :4] == 0.0)                                    # sign(0) = 0, as og_dual.h
    a, b = [0.7] + seeds, [0.7, -0.625, 1.5, -0.3125]
    for name in ("max", "min"):                                         # a tie: the generated ternary takes its second arm
        assert np.array_equal(probe.host(name, 0, np.array([a + b]))[0, :4], b)
    for name, q in (("mod", 3.0), ("fmod", 3.0)):                       # on a jump the quotient is the one to the right
        got = probe.host(name, 0, np.array([[7.5] + seeds + [2.5, -0.625, 1.5, -0.3125]]))[0]
        assert np.array_equal(got[:4], [0.0] + [s - q * t for s, t in zip(seeds, (-0.625, 1.5, -0.3125))])
    for name in ("mod", "fmod"):                                        # an infinite quotient: its term is left out of dd too
        for a_v, b_v in ((1.0, 0.0), (1e300, 1e-300)):
            got = probe.host(name, 0, np.array([[a_v] + seeds + [b_v, -0.625, 1.5, -0.3125]]))[0]
            assert np.array_equal(got[1:4], seeds) and same_bits(got[[0, 1, 2]], got[[4, 5, 7]]).all()


def test_interp_linear_at_its_knots_and_ends_in_each_mode(probe):
    seeds = np.array([0.75, -1.25, 0.4375])
    slopes = np.diff(hc.YG) / np.diff(hc.XG)
    below, above = np.nextafter(0.0, -1.0), np.nextafter(4.0, 5.0)
    x = np.array([0.0, 1.0, 2.5, 4.0, below, above])
    args = np.zeros((x.size, 8))
    args[:, 0], args[:, 1:4] = x, seeds
    for mode, name in enumerate(cases.INTERP):
        got = probe.host(name, 0, args)
        inside = [slopes[0], slopes[1], slopes[2], slopes[2]]           # the right-hand segment at a knot, the last at the end
        outside = [slopes[0], slopes[2]] if mode == 1 else [0.0, 0.0]
        want = np.outer(inside + outside, seeds)
        assert np.array_equal(got[:, 1:4], want), (name, got[:, 1:4], want)
        if mode != 1:
            assert np.array_equal(got[:4, 0], hc.YG)                    # a knot's own value
            assert same_bits(got[4:, 0], np.array(hc.FILLS if mode == 0 else [np.nan, np.nan])).all()


# --------------------------------------------------------------------------------------------- 2.3 exact zeros
@pytest.mark.parametrize("name", cases.PROBE_OPS)
def test_dd_is_exactly_zero_when_one_seed_slot_is_zero(probe, name):
    """"exact zeros outside the pattern": with a.d1 = b.d1 = 0 (or the mirror image) and both dd zero the result's dd is
    exactly zero at every value of the case table - NaN, infinite and singular ones included - except in
    ``double / ogdual2`` where og_dual.h's unguarded slope is itself not finite (counted; none of another kind)."""
    args = cases.zero_args(name)
    assert len(args) >= 2 * 1024 or name not in cases.BINARY
    for form in cases.forms(name):
        out = probe.host(name, form, args)
        nonzero, permitted = cases.zero_exceptions(name, form, args, out)
        assert nonzero == permitted, "%s form %d: %d results with dd != 0, %d of the permitted kind; first %r -> %r" % (
            name, form, nonzero, permitted, args[~(out[:, 3] == 0.0)][0], out[~(out[:, 3] == 0.0)][0])
        assert nonzero == 0 or (name == "div" and form == 2)
        assert_rule_a(args, out)
        slot = np.where(args[:, 1] == 0.0, 1, 2)                         # the zero slot's first-order part: zero or NaN ...
        d = out[np.arange(len(out)), slot]
        assert np.all((d == 0.0) | ~np.isfinite(d))                     # ... never a finite non-zero number


# --------------------------------------------------------------------------------------------- 2.4 the builds
def test_two_host_compilers_give_the_same_bits(probe):
    other = cases.load("clang")
    count = 0
    for name, form, args in cases.device_groups():
        bad = ~same_bits(probe.host(name, form, args), other.host(name, form, args)).all(axis=1)
        assert not bad.any(), "%s form %d: g++ and clang++ differ at %r" % (name, form, args[bad][:3])
        count += len(args)
        assert len(args) % 64 != 0
    assert count > 100000


def test_probe_cross_compiles_for_gfx950_with_the_flags_of_the_product(probe):
    """A build break of the device probe is seen on a machine without a GPU."""
    from opengoddard_amd import build
    path = cases.build_probe("hip")
    assert cases.os.path.dirname(path) == build.JITDIR and cases.build_probe("hip") == path
    with open(path, "rb") as fh:
        blob = fh.read()
    assert b"gfx950" in blob and b"og2p_kernel" in blob
    lib = C.CDLL(path)
    for symbol in ("og2p_device", "og2p_device_count", "og2p_host", "og2p_name", "og2p_count"):
        assert hasattr(lib, symbol), symbol
    hip = cases.load("hip")                                             # clang's host loop inside the HIP module
    for name in ("hypot", "pow", "atan2", "tanh", "interp2"):
        for form in cases.forms(name):
            args = cases.zero_args(name)[::7]
            assert same_bits(hip.host(name, form, args), probe.host(name, form, args)).all(), (name, form)
