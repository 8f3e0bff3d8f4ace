// TEST INFRASTRUCTURE - host probe of the cached form of a sequential sum (tests/test_sequential_sums.py).
//
// The generated sum loop (codegen._cached_sum_lines) runs only for an accessor that has term_cache / term_q / term_v,
// and the only such accessor is the kernels' XColT: the CPU twin, the interpreter and the exact path all sum in place.
// This program is that accessor on the host: og_math.h gives OG_ANY and OG_KEEP host meanings, so the loop compiles
// with g++ and runs under AddressSanitizer / UBSan as a plain process (own main, nothing preloaded).
//
//   * the cache is a heap block of exactly N_TERMS + 16 doubles (the kernels' TERM_DOUBLES), filled as fill_terms
//     fills it, the 16 beyond the terms set to NaN: a read past the pad is a sanitizer report, a pad value that
//     reaches a sum is a mismatch;
//   * for j = -1 and every column j the accessor is set up as make_xcolt sets it up - q = sum_term_q(tb, j), the
//     swapped-in term evaluated through the selecting accessor (x0[i], or x0[j] + h[j] for i == j);
//   * every row group (and every defect group's dynamics tail) evaluated through it is compared, bit for bit, with
//     the same function on a materialised x0 + h e_j through a plain vector accessor (the twin's), which sums in place.
//
// Input: one file of doubles, x0[N_VAR] h[N_VAR] cv[max(N_CVEC, 1)].  Output: one line of counts; exit status 0 when
// every value agreed, 1 on a mismatch (the first few are printed), 2 on a usage error.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include OG_GEN_HEADER

namespace {

constexpr int TB_SLOTS = OgGen::N_TBLK > 0 ? OgGen::N_TBLK : 1;
long g_cache_reads = 0;         // term_cache() calls that handed out the cache

struct XVec {                   // a materialised vector: sums are evaluated in place
    typedef double scalar;
    const double* x;
    double operator()(const int i) const { return x[i]; }
    double ldy(const double* p) const { return *p; }
};

struct XSel {                   // the kernels' XCol
    typedef double scalar;
    const double* x0;
    int j;
    double xj;
    double operator()(const int i) const {
        const double v = x0[i];
        return i == j ? xj : v;
    }
    double ldy(const double* p) const { return *p; }
};

struct XCached {                // the kernels' XColT
    typedef double scalar;
    const double* x0;
    int j;
    double xj;
    const double* tc;
    int qd[TB_SLOTS];
    double td[TB_SLOTS];
    double operator()(const int i) const {
        const double v = x0[i];
        return i == j ? xj : v;
    }
    double ldy(const double* p) const { return *p; }
    const double* term_cache(const int tb) const {
        if (tc && qd[tb] != -2) {
            ++g_cache_reads;
            return tc + OgGen::TERM_OFF(tb);
        }
        return nullptr;
    }
    int term_q(const int tb) const { return qd[tb]; }
    double term_v(const int tb) const { return td[tb]; }
};

XCached make_cached(const double* x0, const double* cv, const int j, const double xj, const double* tc) {
    XCached x;
    x.x0 = x0, x.j = j, x.xj = xj, x.tc = tc;
    const XSel plain{x0, j, xj};
    for (int tb = 0; tb < TB_SLOTS; ++tb) {
        x.qd[tb] = -1, x.td[tb] = 0.0;
        if (tc && tb < OgGen::N_TBLK && j >= 0) {
            x.qd[tb] = OgGen::sum_term_q(tb, j);
            if (x.qd[tb] >= 0) x.td[tb] = OgGen::sum_term(tb, x.qd[tb], plain, cv);
        }
    }
    return x;
}

bool same_bits(const double a, const double b) {
    if (std::isnan(a) && std::isnan(b)) return true;
    std::uint64_t ua, ub;
    std::memcpy(&ua, &a, 8);
    std::memcpy(&ub, &b, 8);
    return ua == ub;
}

}  // namespace

int main(int argc, char** argv) {
    const int n = OgGen::N_VAR, ncv = OgGen::N_CVEC > 0 ? OgGen::N_CVEC : 1;
    if (argc != 2) {
        std::fprintf(stderr, "usage: %s <file of x0, h, cv>\n", argv[0]);
        return 2;
    }
    std::vector<double> x0(n), h(n), cv(ncv);
    FILE* fh = std::fopen(argv[1], "rb");
    if (!fh || std::fread(x0.data(), 8, n, fh) != (size_t)n || std::fread(h.data(), 8, n, fh) != (size_t)n ||
        std::fread(cv.data(), 8, ncv, fh) != (size_t)ncv || std::fgetc(fh) != EOF) {
        std::fprintf(stderr, "%s: expected exactly %d doubles\n", argv[1], 2 * n + ncv);
        return 2;
    }
    std::fclose(fh);

    // the cache: exactly what a workgroup has, the pad poisoned
    const int n_cache = OgGen::N_TERMS + 16;
    double* tc = new double[n_cache];
    for (int i = 0; i < n_cache; ++i) tc[i] = std::numeric_limits<double>::quiet_NaN();
    const XVec base{x0.data()};
    for (int tb = 0; tb < OgGen::N_TBLK; ++tb)
        for (int q = 0; q < OgGen::TERM_LEN(tb); ++q) tc[OgGen::TERM_OFF(tb) + q] = OgGen::sum_term(tb, q, base, cv.data());

    long cached = 0, in_place = 0, neither = 0, compared = 0, nan_values = 0, mismatches = 0;
    std::vector<double> x1(x0);
    double got[OgGen::MAX_OUT], want[OgGen::MAX_OUT];       // (a defect group has one output per dynamics tail)
    for (int j = -1; j < n; ++j) {
        const double xj = j >= 0 ? x0[j] + h[j] : 0.0;
        if (j >= 0) x1[j] = xj;
        const XCached xc = make_cached(x0.data(), cv.data(), j, xj, tc);
        const XVec xv{x1.data()};
        if (j >= 0)
            for (int tb = 0; tb < OgGen::N_TBLK; ++tb) {
                if (xc.qd[tb] >= 0) ++cached;
                else if (xc.qd[tb] == -2) ++in_place;
                else ++neither;
            }
        for (int g = 0; g < OgGen::N_GROUPS; ++g) {
            const bool rows = OgGen::G_KIND(g) == 0;
            const int nout = OgGen::G_NOUT(g);
            for (int k = 0; k < OgGen::G_LEN(g); ++k) {
                const double *a = got, *b = want;
                if (rows) {
                    OgGen::group_eval(g, k, xc, (const double*)nullptr, cv.data(), got);
                    OgGen::group_eval(g, k, xv, (const double*)nullptr, cv.data(), want);
                } else {
                    OgGen::defect_tail(g, k, xc, cv.data(), got);
                    OgGen::defect_tail(g, k, xv, cv.data(), want);
                }
                for (int o = 0; o < nout; ++o) {
                    ++compared;
                    if (std::isnan(b[o])) ++nan_values;
                    if (!same_bits(a[o], b[o]) && ++mismatches <= 10)
                        std::printf("MISMATCH column %d group %d (%s) element %d output %d: cached %a, in place %a\n", j, g,
                                    rows ? "rows" : "tail", k, o, a[o], b[o]);
                }
            }
        }
        if (j >= 0) x1[j] = x0[j];
    }
    delete[] tc;
    std::printf("blocks=%d terms=%d columns=%d cached=%ld in_place=%ld neither=%ld cache_reads=%ld compared=%ld nan=%ld "
                "mismatches=%ld\n", OgGen::N_TBLK, OgGen::N_TERMS, n, cached, in_place, neither, g_cache_reads, compared,
                nan_values, mismatches);
    return mismatches ? 1 : 0;
}
