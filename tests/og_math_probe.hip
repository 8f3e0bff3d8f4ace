// og_math_probe.hip - apply ONE function of csrc/og_math.h / csrc/og_dual.h to arrays, on the host and on the device.
//
// One source, three builds (tests/og_math_cases.py): g++ and clang++ as plain C++ (-x c++: the host loop only) and
// hipcc with the flags of the product's modules (the host loop again, plus a kernel and a launcher).  The tests compare
// the bits of the three.  The order of OGP_NAMES is the function id; og_math_cases.FUNCS must list the same names
// (checked through ogp_name).
//
// variant 0: the plain double function.  1: both arguments ogdual (a, da), (b, db).  2: (ogdual, double).
// 3: (double, ogdual) - the mixed overloads of og_dual.h are rules of their own (mod_, fmod_).
#include "og_dual.h"

namespace ogp {

struct out2 { double v, d; };
struct table { const double* xg; const double* yg; int n; int mode; double fill_below, fill_above; };

OG_HD out2 pack(const double v) { out2 r; r.v = v; r.d = 0.0; return r; }
OG_HD out2 pack(const ogdual a) { out2 r; r.v = a.v; r.d = a.d; return r; }
OG_HD out2 none() { return pack(ogm::from_bits(0x7ff8000000000000ULL)); }

enum {
    F_EXP, F_LOG, F_SIN, F_COS, F_TAN, F_ATAN, F_ASIN, F_ACOS, F_EXPM1, F_LOG1P, F_SINH, F_COSH, F_TANH, F_LOG2,
    F_LOG10, F_CBRT, F_SQRT, F_FABS, F_FLOOR, F_TRUNC, F_ATAN2, F_HYPOT, F_POW, F_MOD, F_FMOD, F_SCALB, F_INTERP,
    F_DIV, F_MUL, F_COUNT
};

// the functions only one of the two scalar types has
OG_HD out2 only(const int fid, const double a, const double b) {
    switch (fid) {
        case F_FLOOR: return pack(ogm::floor_(a));
        case F_TRUNC: return pack(ogm::trunc_(a));
        case F_SCALB: return pack(ogm::scalb_(a, (int)b));          // the table keeps b a whole number in [-2100, 2100]
        default: return none();
    }
}
OG_HD out2 only(const int, const ogdual, const ogdual) { return none(); }

template <class A, class B>
OG_HD out2 two(const int fid, const A a, const B b) {
    using namespace ogm;
    switch (fid) {
        case F_ATAN2: return pack(atan2_(a, b));
        case F_HYPOT: return pack(hypot_(a, b));
        case F_POW: return pack(pow_(a, b));
        case F_MOD: return pack(mod_(a, b));
        case F_FMOD: return pack(fmod_(a, b));
        case F_DIV: return pack(a / b);
        case F_MUL: return pack(a * b);
        default: return none();
    }
}

template <class T>
OG_HD out2 apply(const int fid, const T a, const T b, const table t) {
    using namespace ogm;
    switch (fid) {
        case F_EXP: return pack(exp_(a));
        case F_LOG: return pack(log_(a));
        case F_SIN: return pack(sin_(a));
        case F_COS: return pack(cos_(a));
        case F_TAN: return pack(tan_(a));
        case F_ATAN: return pack(atan_(a));
        case F_ASIN: return pack(asin_(a));
        case F_ACOS: return pack(acos_(a));
        case F_EXPM1: return pack(expm1_(a));
        case F_LOG1P: return pack(log1p_(a));
        case F_SINH: return pack(sinh_(a));
        case F_COSH: return pack(cosh_(a));
        case F_TANH: return pack(tanh_(a));
        case F_LOG2: return pack(log2_(a));
        case F_LOG10: return pack(log10_(a));
        case F_CBRT: return pack(cbrt_(a));
        case F_SQRT: return pack(sqrt_(a));
        case F_FABS: return pack(fabs_(a));
        case F_INTERP: return pack(interp_linear(t.xg, t.yg, t.n, t.mode, t.fill_below, t.fill_above, a));
        case F_FLOOR: case F_TRUNC: case F_SCALB: return only(fid, a, b);
        default: return two(fid, a, b);
    }
}

OG_HD out2 run(const int fid, const int variant, const double a, const double b, const double da, const double db,
               const table t) {
    switch (variant) {
        case 0: return apply<double>(fid, a, b, t);
        case 1: return apply<ogdual>(fid, ogdual(a, da), ogdual(b, db), t);
        case 2: return two(fid, ogdual(a, da), b);
        case 3: return two(fid, a, ogdual(b, db));
        default: return none();
    }
}

}  // namespace ogp

extern "C" {

int ogp_count() { return ogp::F_COUNT; }

const char* ogp_name(const int fid) {
    static const char* const names[ogp::F_COUNT] = {
        "exp", "log", "sin", "cos", "tan", "atan", "asin", "acos", "expm1", "log1p", "sinh", "cosh", "tanh", "log2",
        "log10", "cbrt", "sqrt", "fabs", "floor", "trunc", "atan2", "hypot", "pow", "mod", "fmod", "scalb", "interp",
        "div", "mul"};
    return (fid >= 0 && fid < ogp::F_COUNT) ? names[fid] : "";
}

void ogp_host(const int fid, const int variant, const double* a, const double* b, const double* da, const double* db,
              double* ov, double* od, const int n, const double* xg, const double* yg, const int tn, const int mode,
              const double fill_below, const double fill_above) {
    ogp::table t;
    t.xg = xg, t.yg = yg, t.n = tn, t.mode = mode, t.fill_below = fill_below, t.fill_above = fill_above;
    for (int i = 0; i < n; ++i) {
        const ogp::out2 r = ogp::run(fid, variant, a[i], b[i], da[i], db[i], t);
        ov[i] = r.v;
        od[i] = r.d;
    }
}

}  // extern "C"

#if defined(__HIPCC__)

template <int BLOCK>
__global__ void __launch_bounds__(BLOCK)
ogp_kernel(const int fid, const int variant, const double* a, const double* b, const double* da, const double* db,
           double* ov, double* od, const int n, const ogp::table t) {
    const int i = (int)(blockIdx.x * BLOCK + threadIdx.x);
    if (i >= n) return;
    const ogp::out2 r = ogp::run(fid, variant, a[i], b[i], da[i], db[i], t);
    ov[i] = r.v;
    od[i] = r.d;
}

extern "C" int ogp_device_count() {
    int count = 0;
    return hipGetDeviceCount(&count) == hipSuccess ? count : 0;
}

// Allocate, copy in, launch with workgroups of `block` (64 or 512) lanes, copy back, free.  -> HIP's error code of the
// first call that failed (0: none), -1 for an argument this launcher does not take.  The table (tn >= 2 entries) is
// read from device memory, as generated code reads its tables.
extern "C" int ogp_device(const int fid, const int variant, const double* a, const double* b, const double* da,
                          const double* db, double* ov, double* od, const int n, const int block, const double* xg,
                          const double* yg, const int tn, const int mode, const double fill_below,
                          const double fill_above) {
    if (n <= 0 || tn < 2 || (block != 64 && block != 512) || fid < 0 || fid >= ogp::F_COUNT) return -1;
    const size_t bytes = (size_t)n * sizeof(double), tbytes = (size_t)tn * sizeof(double);
    double* dev[8] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    const double* in[4] = {a, b, da, db};
    hipError_t err = hipSuccess;
    for (int k = 0; k < 6 && err == hipSuccess; ++k) err = hipMalloc((void**)&dev[k], bytes);
    for (int k = 6; k < 8 && err == hipSuccess; ++k) err = hipMalloc((void**)&dev[k], tbytes);
    for (int k = 0; k < 4 && err == hipSuccess; ++k) err = hipMemcpy(dev[k], in[k], bytes, hipMemcpyHostToDevice);
    if (err == hipSuccess) err = hipMemcpy(dev[6], xg, tbytes, hipMemcpyHostToDevice);
    if (err == hipSuccess) err = hipMemcpy(dev[7], yg, tbytes, hipMemcpyHostToDevice);
    if (err == hipSuccess) err = hipMemset(dev[4], 0xff, bytes);
    if (err == hipSuccess) err = hipMemset(dev[5], 0xff, bytes);
    if (err == hipSuccess) {
        ogp::table t;
        t.xg = dev[6], t.yg = dev[7], t.n = tn, t.mode = mode, t.fill_below = fill_below, t.fill_above = fill_above;
        const unsigned grid = (unsigned)((n + block - 1) / block);
        if (block == 64)
            hipLaunchKernelGGL(ogp_kernel<64>, dim3(grid), dim3(64), 0, 0, fid, variant, dev[0], dev[1], dev[2], dev[3],
                               dev[4], dev[5], n, t);
        else
            hipLaunchKernelGGL(ogp_kernel<512>, dim3(grid), dim3(512), 0, 0, fid, variant, dev[0], dev[1], dev[2],
                               dev[3], dev[4], dev[5], n, t);
        err = hipGetLastError();
    }
    if (err == hipSuccess) err = hipDeviceSynchronize();
    if (err == hipSuccess) err = hipMemcpy(ov, dev[4], bytes, hipMemcpyDeviceToHost);
    if (err == hipSuccess) err = hipMemcpy(od, dev[5], bytes, hipMemcpyDeviceToHost);
    for (int k = 0; k < 8; ++k)
        if (dev[k]) (void)hipFree(dev[k]);
    return (int)err;
}

#endif  // __HIPCC__
