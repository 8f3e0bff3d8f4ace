// TEST INFRASTRUCTURE - host probe of the rules of csrc/og_dual2.h (tests/test_hessian.py).
//
// Every operator and every ogm:: function of og_dual2.h, each overload, on arguments the test chooses; next to each
// result the two results of og_dual.h on the projections (v, d1) and (v, d2) of the same arguments, which rule (a) of
// og_dual2.h says are the result's own projections bit for bit.  A program of its own: g++, clang++, and once under
// AddressSanitizer / UBSan.
//
// Input: records of 10 doubles [op, form, a.v, a.d1, a.d2, a.dd, b.v, b.d1, b.d2, b.dd]; form 0: dual o dual, 1: dual o
// double (b.v), 2: double (a.v) o dual; a unary op reads a only.  Output: 8 doubles per record, the result's v, d1, d2,
// dd and og_dual.h's (v, d) along seed 1 and along seed 2.  The ops are numbered as OPS in tests/hessian_cases.py; the
// interpolation table and its fills are the ones below (ops interp0 / interp1: mode 0, fills, and mode 1, extrapolation).
#include <cstdio>
#include <vector>

#include "og_math.h"
#include "og_dual.h"
#include "og_dual2.h"

namespace {

const double XG[4] = {0.0, 1.0, 2.5, 4.0}, YG[4] = {1.0, 3.0, -2.0, 0.5};
const double FILL_BELOW = -7.25, FILL_ABOVE = 11.5;

enum Op {
    ADD, SUB, MUL, DIV, NEG, SQRT, EXP, LOG, SIN, COS, TAN, FABS, ATAN, ASIN, ACOS, ATAN2, TANH, SINH, COSH, EXPM1, LOG1P,
    LOG2, LOG10, CBRT, HYPOT, MOD, FMOD, POW, INTERP0, INTERP1, MAX, MIN, N_OPS
};

// one rule on any of the two dual types: S the scalar, a / b in the three forms
template <class S, class A, class B>
S binary(const int op, const A a, const B b) {
    using namespace ogm;
    switch (op) {
    case ADD: return a + b;
    case SUB: return a - b;
    case MUL: return a * b;
    case DIV: return a / b;
    case ATAN2: return atan2_(a, b);
    case HYPOT: return hypot_(a, b);
    case MOD: return mod_(a, b);
    case FMOD: return fmod_(a, b);
    case POW: return pow_(a, b);
    case MAX: return a > b ? S(a) : S(b);           // the generated ternaries
    case MIN: return a < b ? S(a) : S(b);
    default: return S(0.0);
    }
}

template <class S>
S unary(const int op, const S a) {
    using namespace ogm;
    switch (op) {
    case NEG: return -a;
    case SQRT: return sqrt_(a);
    case EXP: return exp_(a);
    case LOG: return log_(a);
    case SIN: return sin_(a);
    case COS: return cos_(a);
    case TAN: return tan_(a);
    case FABS: return fabs_(a);
    case ATAN: return atan_(a);
    case ASIN: return asin_(a);
    case ACOS: return acos_(a);
    case TANH: return tanh_(a);
    case SINH: return sinh_(a);
    case COSH: return cosh_(a);
    case EXPM1: return expm1_(a);
    case LOG1P: return log1p_(a);
    case LOG2: return log2_(a);
    case LOG10: return log10_(a);
    case CBRT: return cbrt_(a);
    case INTERP0: return interp_linear(XG, YG, 4, 0, FILL_BELOW, FILL_ABOVE, a);
    case INTERP1: return interp_linear(XG, YG, 4, 1, FILL_BELOW, FILL_ABOVE, a);
    default: return S(0.0);
    }
}

bool is_binary(const int op) {
    return op <= DIV || op == ATAN2 || op == HYPOT || op == MOD || op == FMOD || op == POW || op == MAX || op == MIN;
}

template <class S>
S apply(const int op, const int form, const S a, const S b) {
    if (!is_binary(op)) return unary<S>(op, a);
    if (form == 1) return binary<S>(op, a, b.v);
    if (form == 2) return binary<S>(op, a.v, b);
    return binary<S>(op, a, b);
}

}  // namespace

int main(int argc, char** argv) {
    if (argc != 3) {
        std::fprintf(stderr, "usage: %s <records> <output file>\n", argv[0]);
        return 2;
    }
    FILE* fh = std::fopen(argv[1], "rb");
    if (!fh) return 2;
    std::vector<double> out;
    double r[10];
    int records = 0;
    while (std::fread(r, 8, 10, fh) == 10) {
        const int op = (int)r[0], form = (int)r[1];
        if (op < 0 || op >= N_OPS || form < 0 || form > 2) return 2;
        const ogdual2 a(r[2], r[3], r[4], r[5]), b(r[6], r[7], r[8], r[9]);
        const ogdual2 got = apply<ogdual2>(op, form, a, b);
        const ogdual p1 = apply<ogdual>(op, form, ogdual(a.v, a.d1), ogdual(b.v, b.d1));
        const ogdual p2 = apply<ogdual>(op, form, ogdual(a.v, a.d2), ogdual(b.v, b.d2));
        const double rec[8] = {got.v, got.d1, got.d2, got.dd, p1.v, p1.d, p2.v, p2.d};
        out.insert(out.end(), rec, rec + 8);
        ++records;
    }
    std::fclose(fh);
    FILE* fo = std::fopen(argv[2], "wb");
    if (!fo || std::fwrite(out.data(), 8, out.size(), fo) != out.size()) return 2;
    std::fclose(fo);
    std::printf("records=%d\n", records);
    return 0;
}
