// og_dual2.h - second-order dual numbers with two seeds: value, the first-order parts along two directions and the
// MIXED second-order part.  What csrc/og_hvp.h evaluates the generated callbacks on to get d2F/dx_j dv.
//
// a = v + d1 e1 + d2 e2 + dd e1 e2 with e1^2 = e2^2 = 0: for a unary f
//     f(a) = f(v) + f'(v) d1 e1 + f'(v) d2 e2 + (f''(v) d1 d2 + f'(v) dd) e1 e2,
// the binary rules are the textbook ones (product: dd = a.dd b.v + a.d1 b.d2 + a.d2 b.d1 + a.v b.dd; the others follow
// from it).  The generated code (codegen.emit_header) is written against `typename X::scalar` and never names a dual
// type, so an accessor whose scalar is ogdual2 is all it takes.
//
// Two rules of og_dual.h carry over:
//   (a) the projections (v, d1) and (v, d2) of every result are, bit for bit, what og_dual.h gives for the projections
//       of the arguments: every d1 / d2 below is og_dual.h's expression for d, with the same og_math.h calls, in the
//       same order (tests/test_hessian.py compares the bits for every operator and function);
//   (b) a contribution whose seed factors are all zero is LEFT OUT, not computed: the f'' term when a.d1 == 0 or
//       a.d2 == 0, the f' term when a.dd == 0, and likewise term by term in the binary rules.  A quantity that does not
//       depend on the seeded variables therefore keeps dd = 0 through sqrt(0), log(0), asin(1), 0/0-type quotients and
//       x^y at x = 0 instead of producing 0 * inf.  (Rule (a) binds d1 and d2 to og_dual.h's expressions, guarded or
//       not; (b) is about dd.)  Where og_dual.h takes the slope as 0 (sqrt, cbrt and hypot at 0), dd is 0 as well.
//       The kernels seed a leaf as (x_i, i == j, v_i, 0), so almost every intermediate has some seeds zero and others
//       not: with one whole slot zero and both dd zero, dd stays exactly 0 whatever the value is.  The one exception is
//       double / ogdual2 at a divisor where og_dual.h's unguarded slope -(q b.d) / b.v is itself not finite.
// Piecewise-linear operations (fabs_, the generated ternaries for max / min, mod_, fmod_, interp_linear) take their
// branch from v and have no curvature of their own: dd is the first-order rule applied to dd.
// A coefficient that is exactly zero is left out like a zero seed where it would meet an infinity (pow_: y (y - 1) at
// y = 1, x = 0), and no mixed part is formed as a difference of nearly equal numbers (hypot_).
//
// Same source for hipcc and a host compiler: tests/test_dual2_gpu.py holds the device to the host's bits for every rule,
// form and seed pattern; tests/test_dual2_seeds.py holds the host to closed-form derivatives.
#ifndef OG_DUAL2_H
#define OG_DUAL2_H

#include "og_dual.h"

struct ogdual2 {
    double v, d1, d2, dd;
    OG_HDI ogdual2() : v(0.0), d1(0.0), d2(0.0), dd(0.0) {}
    OG_HDI ogdual2(const double value) : v(value), d1(0.0), d2(0.0), dd(0.0) {}
    // value and slot-2 seed: what OgGen::par_leaf constructs for an accessor with a member par_seed (csrc/og_mix.h)
    OG_HDI ogdual2(const double value, const double seed2) : v(value), d1(0.0), d2(seed2), dd(0.0) {}
    OG_HDI ogdual2(const double value, const double a, const double b, const double mixed)
        : v(value), d1(a), d2(b), dd(mixed) {}
};

// seed factor times coefficient, left out when the seed factor(s) are zero
OG_HDI double og2_term(const double seed, const double coef) { return seed == 0.0 ? 0.0 : seed * coef; }
OG_HDI double og2_term(const double s1, const double s2, const double coef) {
    return (s1 == 0.0 || s2 == 0.0) ? 0.0 : coef * s1 * s2;
}

OG_HDI ogdual2 operator-(const ogdual2 a) { return ogdual2(-a.v, -a.d1, -a.d2, -a.dd); }
OG_HDI ogdual2 operator+(const ogdual2 a, const ogdual2 b) {
    return ogdual2(a.v + b.v, a.d1 + b.d1, a.d2 + b.d2, a.dd + b.dd);
}
OG_HDI ogdual2 operator-(const ogdual2 a, const ogdual2 b) {
    return ogdual2(a.v - b.v, a.d1 - b.d1, a.d2 - b.d2, a.dd - b.dd);
}
OG_HDI ogdual2 operator*(const ogdual2 a, const ogdual2 b) {
    return ogdual2(a.v * b.v, a.d1 * b.v + a.v * b.d1, a.d2 * b.v + a.v * b.d2,
                   (og2_term(a.dd, b.v) + og2_term(b.dd, a.v)) + (og2_term(a.d1, b.d2, 1.0) + og2_term(a.d2, b.d1, 1.0)));
}
// q = a / b: q b = a differentiated twice gives q.dd b.v = a.dd - q.d1 b.d2 - q.d2 b.d1 - q b.dd
OG_HDI double og2_quot_dd(const double add, const double q, const double q1, const double q2, const ogdual2 b) {
    const bool none = add == 0.0 && b.dd == 0.0 && (q1 == 0.0 || b.d2 == 0.0) && (q2 == 0.0 || b.d1 == 0.0);
    return none ? 0.0 : (((add - og2_term(b.dd, q)) - og2_term(q1, b.d2, 1.0)) - og2_term(q2, b.d1, 1.0)) / b.v;
}
OG_HDI ogdual2 operator/(const ogdual2 a, const ogdual2 b) {
    const double q = a.v / b.v;
    const double q1 = (a.d1 == 0.0 && b.d1 == 0.0) ? 0.0 : (a.d1 - q * b.d1) / b.v;
    const double q2 = (a.d2 == 0.0 && b.d2 == 0.0) ? 0.0 : (a.d2 - q * b.d2) / b.v;
    return ogdual2(q, q1, q2, og2_quot_dd(a.dd, q, q1, q2, b));
}
OG_HDI ogdual2 operator+(const ogdual2 a, const double b) { return ogdual2(a.v + b, a.d1, a.d2, a.dd); }
OG_HDI ogdual2 operator+(const double a, const ogdual2 b) { return ogdual2(a + b.v, b.d1, b.d2, b.dd); }
OG_HDI ogdual2 operator-(const ogdual2 a, const double b) { return ogdual2(a.v - b, a.d1, a.d2, a.dd); }
OG_HDI ogdual2 operator-(const double a, const ogdual2 b) { return ogdual2(a - b.v, -b.d1, -b.d2, -b.dd); }
OG_HDI ogdual2 operator*(const ogdual2 a, const double b) {
    return ogdual2(a.v * b, a.d1 * b, a.d2 * b, og2_term(a.dd, b));
}
OG_HDI ogdual2 operator*(const double a, const ogdual2 b) {
    return ogdual2(a * b.v, a * b.d1, a * b.d2, og2_term(b.dd, a));
}
OG_HDI ogdual2 operator/(const ogdual2 a, const double b) {
    return ogdual2(a.v / b, a.d1 / b, a.d2 / b, a.dd == 0.0 ? 0.0 : a.dd / b);
}
OG_HDI ogdual2 operator/(const double a, const ogdual2 b) {
    const double q = a / b.v;
    const double q1 = -(q * b.d1) / b.v, q2 = -(q * b.d2) / b.v;
    return ogdual2(q, q1, q2, og2_quot_dd(0.0, q, q1, q2, b));
}

#define OG_DUAL2_CMP(op)                                                            \
    OG_HDI bool operator op(const ogdual2 a, const ogdual2 b) { return a.v op b.v; } \
    OG_HDI bool operator op(const ogdual2 a, const double b) { return a.v op b; }    \
    OG_HDI bool operator op(const double a, const ogdual2 b) { return a op b.v; }
OG_DUAL2_CMP(<)
OG_DUAL2_CMP(<=)
OG_DUAL2_CMP(>)
OG_DUAL2_CMP(>=)
OG_DUAL2_CMP(==)
OG_DUAL2_CMP(!=)
#undef OG_DUAL2_CMP

namespace ogm {

// dd of a unary rule: f2 = f''(a.v) on the product of the two first-order seeds, lin = f'(a.v) a.dd as the caller
// formed it (with og_dual.h's expression for d), each left out when its seeds are zero
OG_HDI double og2_mixed(const ogdual2 a, const double f2, const double lin) {
    return og2_term(a.d1, a.d2, f2) + (a.dd == 0.0 ? 0.0 : lin);
}

OG_HDI ogdual2 sqrt_(const ogdual2 a) {
    const double r = sqrt_(a.v);
    if (r == 0.0) return ogdual2(r, 0.0, 0.0, 0.0);
    return ogdual2(r, a.d1 == 0.0 ? 0.0 : a.d1 / (2.0 * r), a.d2 == 0.0 ? 0.0 : a.d2 / (2.0 * r),
                   og2_mixed(a, -1.0 / (4.0 * r * a.v), a.dd / (2.0 * r)));
}
OG_HDI ogdual2 exp_(const ogdual2 a) {
    const double e = exp_(a.v);
    return ogdual2(e, a.d1 * e, a.d2 * e, og2_mixed(a, e, a.dd * e));
}
OG_HDI ogdual2 log_(const ogdual2 a) {
    return ogdual2(log_(a.v), a.d1 == 0.0 ? 0.0 : a.d1 / a.v, a.d2 == 0.0 ? 0.0 : a.d2 / a.v,
                   og2_mixed(a, -1.0 / (a.v * a.v), a.dd / a.v));
}
OG_HDI ogdual2 sin_(const ogdual2 a) {
    const double s = sin_(a.v), c = cos_(a.v);
    return ogdual2(s, a.d1 * c, a.d2 * c, og2_mixed(a, -s, a.dd * c));
}
OG_HDI ogdual2 cos_(const ogdual2 a) {
    const double s = sin_(a.v), c = cos_(a.v);
    return ogdual2(c, -(a.d1 * s), -(a.d2 * s), og2_mixed(a, -c, -(a.dd * s)));
}
OG_HDI ogdual2 tan_(const ogdual2 a) {
    const double t = tan_(a.v), g = 1.0 + t * t;
    return ogdual2(t, a.d1 * g, a.d2 * g, og2_mixed(a, 2.0 * t * g, a.dd * g));
}
OG_HDI ogdual2 fabs_(const ogdual2 a) {
    const double s = a.v > 0.0 ? 1.0 : (a.v < 0.0 ? -1.0 : 0.0);
    return ogdual2(fabs_(a.v), s * a.d1, s * a.d2, s * a.dd);
}
OG_HDI ogdual2 atan_(const ogdual2 a) {
    const double g = 1.0 + a.v * a.v;
    return ogdual2(atan_(a.v), a.d1 / g, a.d2 / g, og2_mixed(a, -2.0 * a.v / (g * g), a.dd / g));
}
OG_HDI ogdual2 asin_(const ogdual2 a) {
    const double g = 1.0 - a.v * a.v, r = sqrt_(g);
    return ogdual2(asin_(a.v), a.d1 == 0.0 ? 0.0 : a.d1 / r, a.d2 == 0.0 ? 0.0 : a.d2 / r,
                   og2_mixed(a, a.v / (g * r), a.dd / r));
}
OG_HDI ogdual2 acos_(const ogdual2 a) {
    const double g = 1.0 - a.v * a.v, r = sqrt_(g);
    return ogdual2(acos_(a.v), a.d1 == 0.0 ? 0.0 : -(a.d1 / r), a.d2 == 0.0 ? 0.0 : -(a.d2 / r),
                   og2_mixed(a, -(a.v / (g * r)), -(a.dd / r)));
}
// atan2(y, x): d = (x y' - y x') / r2, and once more
OG_HDI ogdual2 atan2_(const ogdual2 y, const ogdual2 x) {
    const double r2 = x.v * x.v + y.v * y.v;
    const double d1 = (y.d1 == 0.0 && x.d1 == 0.0) ? 0.0 : (x.v * y.d1 - y.v * x.d1) / r2;
    const double d2 = (y.d2 == 0.0 && x.d2 == 0.0) ? 0.0 : (x.v * y.d2 - y.v * x.d2) / r2;
    const bool first = (y.d1 != 0.0 || x.d1 != 0.0) && (y.d2 != 0.0 || x.d2 != 0.0);
    double dd = 0.0;
    if (first || y.dd != 0.0 || x.dd != 0.0) {
        const double cross = og2_term(x.d2, y.d1, 1.0) - og2_term(y.d2, x.d1, 1.0);
        const double lin = og2_term(y.dd, x.v) - og2_term(x.dd, y.v);
        const double fold = first ? d1 * (2.0 * (x.v * x.d2 + y.v * y.d2)) : 0.0;
        dd = ((cross + lin) - fold) / r2;
    }
    return ogdual2(atan2_(y.v, x.v), d1, d2, dd);
}
OG_HDI ogdual2 atan2_(const ogdual2 y, const double x) { return atan2_(y, ogdual2(x)); }
OG_HDI ogdual2 atan2_(const double y, const ogdual2 x) { return atan2_(ogdual2(y), x); }

OG_HDI ogdual2 tanh_(const ogdual2 a) {
    const double t = tanh_(a.v), g = 1.0 - t * t;
    return ogdual2(t, a.d1 * g, a.d2 * g, og2_mixed(a, -2.0 * t * g, a.dd * g));
}
OG_HDI ogdual2 sinh_(const ogdual2 a) {
    const double s = sinh_(a.v), c = cosh_(a.v);
    return ogdual2(s, a.d1 * c, a.d2 * c, og2_mixed(a, s, a.dd * c));
}
OG_HDI ogdual2 cosh_(const ogdual2 a) {
    const double s = sinh_(a.v), c = cosh_(a.v);
    return ogdual2(c, a.d1 * s, a.d2 * s, og2_mixed(a, c, a.dd * s));
}
OG_HDI ogdual2 expm1_(const ogdual2 a) {
    const double e = exp_(a.v);
    return ogdual2(expm1_(a.v), a.d1 * e, a.d2 * e, og2_mixed(a, e, a.dd * e));
}
OG_HDI ogdual2 log1p_(const ogdual2 a) {
    const double g = 1.0 + a.v;
    return ogdual2(log1p_(a.v), a.d1 == 0.0 ? 0.0 : a.d1 / g, a.d2 == 0.0 ? 0.0 : a.d2 / g,
                   og2_mixed(a, -1.0 / (g * g), a.dd / g));
}
OG_HDI ogdual2 log2_(const ogdual2 a) {
    const double g = a.v * 0.6931471805599453;
    return ogdual2(log2_(a.v), a.d1 == 0.0 ? 0.0 : a.d1 / g, a.d2 == 0.0 ? 0.0 : a.d2 / g,
                   og2_mixed(a, -1.0 / (g * a.v), a.dd / g));
}
OG_HDI ogdual2 log10_(const ogdual2 a) {
    const double g = a.v * 2.302585092994046;
    return ogdual2(log10_(a.v), a.d1 == 0.0 ? 0.0 : a.d1 / g, a.d2 == 0.0 ? 0.0 : a.d2 / g,
                   og2_mixed(a, -1.0 / (g * a.v), a.dd / g));
}
OG_HDI ogdual2 cbrt_(const ogdual2 a) {
    const double c = cbrt_(a.v);
    if (c == 0.0) return ogdual2(c, 0.0, 0.0, 0.0);
    const double g = 3.0 * c * c;
    return ogdual2(c, a.d1 == 0.0 ? 0.0 : a.d1 / g, a.d2 == 0.0 ? 0.0 : a.d2 / g,
                   og2_mixed(a, -2.0 / (3.0 * g * a.v), a.dd / g));
}
// h = hypot(x, y), cx = x / h, cy = y / h: h.dd = (x.d1 x.d2 + y.d1 y.d2 - h.d1 h.d2) / h + cx x.dd + cy y.dd, and by
// Lagrange's identity the bracket is t1 t2 with t = cx y.d - cy x.d along each seed: a product, not the difference of two
// numbers that agree to (y/x)^2 where one argument is constant or dominant (hypot(x, 1e-8), the smoothed |x|).
OG_HDI ogdual2 hypot_(const ogdual2 x, const ogdual2 y) {
    const double h = hypot_(x.v, y.v);
    if (h == 0.0) return ogdual2(h, 0.0, 0.0, 0.0);
    const double d1 = (x.d1 == 0.0 && y.d1 == 0.0) ? 0.0 : (x.v * x.d1 + y.v * y.d1) / h;
    const double d2 = (x.d2 == 0.0 && y.d2 == 0.0) ? 0.0 : (x.v * x.d2 + y.v * y.d2) / h;
    const bool first = (x.d1 != 0.0 || y.d1 != 0.0) && (x.d2 != 0.0 || y.d2 != 0.0);
    double dd = 0.0;
    if (first || x.dd != 0.0 || y.dd != 0.0) {
        const double cx = x.v / h, cy = y.v / h;
        const double t1 = og2_term(y.d1, cx) - og2_term(x.d1, cy), t2 = og2_term(y.d2, cx) - og2_term(x.d2, cy);
        const double lin = og2_term(x.dd, cx) + og2_term(y.dd, cy);
        dd = (first ? t1 * t2 / h : 0.0) + lin;
    }
    return ogdual2(h, d1, d2, dd);
}
OG_HDI ogdual2 hypot_(const ogdual2 x, const double y) { return hypot_(x, ogdual2(y)); }
OG_HDI ogdual2 hypot_(const double x, const ogdual2 y) { return hypot_(ogdual2(x), y); }
// a - q b with q constant between jumps: no curvature
OG_HDI ogdual2 mod_(const ogdual2 a, const ogdual2 b) {
    const double q = floor_(a.v / b.v);
    const bool qf = q - q == 0.0;
    return ogdual2(mod_(a.v, b.v), a.d1 - ((b.d1 == 0.0 || !qf) ? 0.0 : q * b.d1),
                   a.d2 - ((b.d2 == 0.0 || !qf) ? 0.0 : q * b.d2), a.dd - ((b.dd == 0.0 || !qf) ? 0.0 : q * b.dd));
}
OG_HDI ogdual2 mod_(const ogdual2 a, const double b) { return ogdual2(mod_(a.v, b), a.d1, a.d2, a.dd); }
OG_HDI ogdual2 mod_(const double a, const ogdual2 b) { return mod_(ogdual2(a), b); }
OG_HDI ogdual2 fmod_(const ogdual2 a, const ogdual2 b) {
    const double q = trunc_(a.v / b.v);
    const bool qf = q - q == 0.0;
    return ogdual2(fmod_(a.v, b.v), a.d1 - ((b.d1 == 0.0 || !qf) ? 0.0 : q * b.d1),
                   a.d2 - ((b.d2 == 0.0 || !qf) ? 0.0 : q * b.d2), a.dd - ((b.dd == 0.0 || !qf) ? 0.0 : q * b.dd));
}
OG_HDI ogdual2 fmod_(const ogdual2 a, const double b) { return ogdual2(fmod_(a.v, b), a.d1, a.d2, a.dd); }
OG_HDI ogdual2 fmod_(const double a, const ogdual2 b) { return fmod_(ogdual2(a), b); }
// p = x ** y, A = x^(y-1), L = log x: the first-order parts are og_dual.h's  y A x' + p L y'.  Differentiated once more:
//   x.d1 x.d2  y (y - 1) x^(y-2)              y A x.dd
//   x.d1 y.d2  (A + y A L)                    p L y.dd
//   y.d1 x.d2  A      and   y.d1 L times the first-order part along 2 (y A x.d2 + p L y.d2)
// each left out when its seeds are zero; the parts with log x stay out where p is 0, as in og_dual.h, and the curvature
// term where y (y - 1) is exactly 0: x ** 1 is x, also at x = 0 where x^(y-2) is infinite.
OG_HDI ogdual2 pow_(const ogdual2 x, const ogdual2 y) {
    const double p = pow_(x.v, y.v);
    const bool xs = x.d1 != 0.0 || x.d2 != 0.0 || x.dd != 0.0, ys = (y.d1 != 0.0 || y.d2 != 0.0 || y.dd != 0.0) && p != 0.0;
    const double A = xs || ys ? pow_(x.v, y.v - 1.0) : 0.0, L = ys ? log_(x.v) : 0.0;
    double d1 = 0.0, d2 = 0.0, dd = 0.0;
    if (x.d1 != 0.0) d1 += y.v * A * x.d1;
    if (y.d1 != 0.0 && p != 0.0) d1 += p * L * y.d1;
    if (x.d2 != 0.0) d2 += y.v * A * x.d2;
    if (y.d2 != 0.0 && p != 0.0) d2 += p * L * y.d2;
    const double curv = y.v * (y.v - 1.0);
    if (x.d1 != 0.0 && x.d2 != 0.0 && curv != 0.0) dd += curv * pow_(x.v, y.v - 2.0) * x.d1 * x.d2;
    if (x.dd != 0.0) dd += y.v * A * x.dd;
    if (p != 0.0) {
        if (x.d1 != 0.0 && y.d2 != 0.0) dd += (A + y.v * A * L) * x.d1 * y.d2;
        if (y.d1 != 0.0 && x.d2 != 0.0) dd += A * x.d2 * y.d1;
        if (y.d1 != 0.0 && d2 != 0.0) dd += d2 * L * y.d1;
        if (y.dd != 0.0) dd += p * L * y.dd;
    }
    return ogdual2(p, d1, d2, dd);
}
OG_HDI ogdual2 pow_(const ogdual2 x, const double y) { return pow_(x, ogdual2(y)); }
OG_HDI ogdual2 pow_(const double x, const ogdual2 y) { return pow_(ogdual2(x), y); }

// Piecewise-linear table: the slope of the segment the value came from, as og_dual.h finds it; no curvature.
OG_HD ogdual2 interp_linear(const double* xg, const double* yg, const int n, const int mode, const double fill_below,
                            const double fill_above, const ogdual2 x) {
    const ogdual first = interp_linear(xg, yg, n, mode, fill_below, fill_above, ogdual(x.v, 1.0));
    const double slope = first.d;
    return ogdual2(first.v, slope * x.d1, slope * x.d2, slope * x.dd);
}

}  // namespace ogm

#endif /* OG_DUAL2_H */
