// og_dual2_probe.hip - apply ONE rule of csrc/og_dual2.h to arrays of second-order duals, on the host and on the device.
//
// One source, three builds (tests/dual2_seed_cases.py): g++ and clang++ as plain C++ (-x c++: the host loop only) and
// hipcc with the flags of the product's modules (the host loop again, plus a kernel and a launcher).  The tests compare
// the bits of the three.  The order of the names below is the op id: hessian_cases.OPS, then "interp2"
// (dual2_seed_cases.PROBE_OPS must list the same names; checked through og2p_name).
//
// Per element 8 doubles in: a.v, a.d1, a.d2, a.dd, b.v, b.d1, b.d2, b.dd; 8 doubles out: the result's v, d1, d2, dd, then
// og_dual.h's (v, d) on the projections (v, d1) and (v, d2) of the same arguments - which rule (a) of og_dual2.h says are
// the result's own, bit for bit.  form 0: dual o dual, 1: dual o double (b.v), 2: double (a.v) o dual; a unary op reads a
// only.  interp0 / interp1 / interp2 are interp_linear in modes 0 / 1 / 2 on the table the caller passes.
#include "og_math.h"
#include "og_dual.h"
#include "og_dual2.h"

namespace og2p {

struct table { const double* xg; const double* yg; int n; double fill_below, fill_above; };

enum Op {
    ADD, SUB, MUL, DIV, NEG, SQRT, EXP, LOG, SIN, COS, TAN, FABS, ATAN, ASIN, ACOS, ATAN2, TANH, SINH, COSH, EXPM1, LOG1P,
    LOG2, LOG10, CBRT, HYPOT, MOD, FMOD, POW, INTERP0, INTERP1, MAX, MIN, INTERP2, N_OPS
};

// one rule on either dual type: S the scalar, a / b in the three forms
template <class S, class A, class B>
OG_HD S binary(const int op, const A a, const B b) {
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
OG_HD S unary(const int op, const S a, const table t) {
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
        case INTERP0: return interp_linear(t.xg, t.yg, t.n, 0, t.fill_below, t.fill_above, a);
        case INTERP1: return interp_linear(t.xg, t.yg, t.n, 1, t.fill_below, t.fill_above, a);
        case INTERP2: return interp_linear(t.xg, t.yg, t.n, 2, t.fill_below, t.fill_above, a);
        default: return S(0.0);
    }
}

OG_HD bool is_binary(const int op) {
    return op <= DIV || op == ATAN2 || op == HYPOT || op == MOD || op == FMOD || op == POW || op == MAX || op == MIN;
}

template <class S>
OG_HD S apply(const int op, const int form, const S a, const S b, const table t) {
    if (!is_binary(op)) return unary<S>(op, a, t);
    if (form == 1) return binary<S>(op, a, b.v);
    if (form == 2) return binary<S>(op, a.v, b);
    return binary<S>(op, a, b);
}

// one element: in[8] -> out[8]
OG_HD void run(const int op, const int form, const double* in, double* out, const table t) {
    const ogdual2 a(in[0], in[1], in[2], in[3]), b(in[4], in[5], in[6], in[7]);
    const ogdual2 got = apply<ogdual2>(op, form, a, b, t);
    const ogdual p1 = apply<ogdual>(op, form, ogdual(a.v, a.d1), ogdual(b.v, b.d1), t);
    const ogdual p2 = apply<ogdual>(op, form, ogdual(a.v, a.d2), ogdual(b.v, b.d2), t);
    out[0] = got.v, out[1] = got.d1, out[2] = got.d2, out[3] = got.dd;
    out[4] = p1.v, out[5] = p1.d, out[6] = p2.v, out[7] = p2.d;
}

}  // namespace og2p

extern "C" {

int og2p_count() { return og2p::N_OPS; }

const char* og2p_name(const int op) {
    static const char* const names[og2p::N_OPS] = {
        "add", "sub", "mul", "div", "neg", "sqrt", "exp", "log", "sin", "cos", "tan", "fabs", "atan", "asin", "acos",
        "atan2", "tanh", "sinh", "cosh", "expm1", "log1p", "log2", "log10", "cbrt", "hypot", "mod", "fmod", "pow",
        "interp0", "interp1", "max", "min", "interp2"};
    return (op >= 0 && op < og2p::N_OPS) ? names[op] : "";
}

// in[n * 8] -> out[n * 8]
void og2p_host(const int op, const int form, const double* in, double* out, const int n, const double* xg,
               const double* yg, const int tn, const double fill_below, const double fill_above) {
    og2p::table t;
    t.xg = xg, t.yg = yg, t.n = tn, t.fill_below = fill_below, t.fill_above = fill_above;
    for (int i = 0; i < n; ++i) og2p::run(op, form, in + (size_t)i * 8, out + (size_t)i * 8, t);
}

}  // extern "C"

#if defined(__HIPCC__)

template <int BLOCK>
__global__ void __launch_bounds__(BLOCK)
og2p_kernel(const int op, const int form, const double* in, double* out, const int n, const og2p::table t) {
    const int i = (int)(blockIdx.x * BLOCK + threadIdx.x);
    if (i >= n) return;
    double r[8], w[8];
    for (int k = 0; k < 8; ++k) r[k] = in[(size_t)i * 8 + k];
    og2p::run(op, form, r, w, t);
    for (int k = 0; k < 8; ++k) out[(size_t)i * 8 + k] = w[k];
}

extern "C" int og2p_device_count() {
    int count = 0;
    return hipGetDeviceCount(&count) == hipSuccess ? count : 0;
}

// Allocate, copy in, launch with workgroups of `block` (64 or 512) lanes, copy back, free.  -> HIP's error code of the
// first call that failed (0: none), -1 for an argument this launcher does not take.  The table (tn >= 2 entries) is
// read from device memory, as generated code reads its tables.
extern "C" int og2p_device(const int op, const int form, const double* in, double* out, const int n, const int block,
                           const double* xg, const double* yg, const int tn, const double fill_below,
                           const double fill_above) {
    if (n <= 0 || n > (1 << 24) || tn < 2 || (block != 64 && block != 512) || op < 0 || op >= og2p::N_OPS || form < 0 ||
        form > 2)
        return -1;
    const size_t bytes = (size_t)n * 8 * sizeof(double), tbytes = (size_t)tn * sizeof(double);
    double* dev[4] = {nullptr, nullptr, nullptr, nullptr};           // in, out, xg, yg
    hipError_t err = hipSuccess;
    for (int k = 0; k < 2 && err == hipSuccess; ++k) err = hipMalloc((void**)&dev[k], bytes);
    for (int k = 2; k < 4 && err == hipSuccess; ++k) err = hipMalloc((void**)&dev[k], tbytes);
    if (err == hipSuccess) err = hipMemcpy(dev[0], in, bytes, hipMemcpyHostToDevice);
    if (err == hipSuccess) err = hipMemcpy(dev[2], xg, tbytes, hipMemcpyHostToDevice);
    if (err == hipSuccess) err = hipMemcpy(dev[3], yg, tbytes, hipMemcpyHostToDevice);
    if (err == hipSuccess) err = hipMemset(dev[1], 0xff, bytes);
    if (err == hipSuccess) {
        og2p::table t;
        t.xg = dev[2], t.yg = dev[3], t.n = tn, t.fill_below = fill_below, t.fill_above = fill_above;
        const unsigned grid = (unsigned)((n + block - 1) / block);
        if (block == 64)
            hipLaunchKernelGGL(og2p_kernel<64>, dim3(grid), dim3(64), 0, 0, op, form, dev[0], dev[1], n, t);
        else
            hipLaunchKernelGGL(og2p_kernel<512>, dim3(grid), dim3(512), 0, 0, op, form, dev[0], dev[1], n, t);
        err = hipGetLastError();
    }
    if (err == hipSuccess) err = hipDeviceSynchronize();
    if (err == hipSuccess) err = hipMemcpy(out, dev[1], bytes, hipMemcpyDeviceToHost);
    for (int k = 0; k < 4; ++k)
        if (dev[k]) (void)hipFree(dev[k]);
    return (int)err;
}

#endif  // __HIPCC__
