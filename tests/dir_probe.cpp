// TEST INFRASTRUCTURE - host probe of the exact directional derivative F'(x) v (tests/test_directional.py).
//
// The kernels ogk_exact_dir / ogk_exact_dir_batch (csrc/ogk_kernels.hip) compute every entry of F'(x) v with ONE
// function, og_dir_entry (csrc/og_dir.h), from x0, v, y0, cv and the D operand image alone.  This program is that
// function on the host: the same header, the generated header of a problem (with or without run-time parameters) and
// og_dual.h, compiled with g++ and with clang++ (same bits) and once under AddressSanitizer / UBSan as a plain process
// (own main, nothing preloaded).
//
//   * F(x0) and the base collocation products y0 are computed the CPU twin's way (plain loops, the product a
//     left-to-right fma chain over a dense D), so F0 equals oracle/twin.cpp's to the bit;
//   * every D is packed into the MFMA operand image (ogk.h: ogk_frag_pack) in one heap block of exactly the packed size:
//     a read past it is a sanitizer report;
//   * dF is K * m doubles, pre-filled with NaN; every entry is stored at its row, and every row of every direction
//     must have been written exactly once.
//
// Input: one file of doubles, x0[N_VAR] cv[max(N_CVEC, 1)], D[N][N] row-major for every phase, then V[K][N_VAR] (K from
// the file's size, at least 1).  Output file: dF[K][M] F0[M].  A third argument "seeded" (parameterised headers only)
// reads x through an accessor that HAS a member par_seed, set to an index no parameter has: every parameter leaf is
// then a dual number with a zero derivative instead of the plain table entry - the result must not change.
// Exit status 0, 1 when a row is out of range, written twice or not written, 2 on a usage error.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "ogk.h"
#include "og_dual.h"
#include OG_GEN_HEADER
#include "og_dir.h"

namespace {

struct XVec {
    typedef double scalar;
    const double* x;
    double operator()(const int i) const { return x[i]; }
    double ldy(const double* p) const { return *p; }
};

#ifdef OG_GEN_HAS_PAR
// OgDirX with a seed member that matches no parameter (the "seeded" run)
struct DirXSeeded {
    typedef ogdual scalar;
    const double* x0;
    const double* v;
    int par_seed;
    ogdual operator()(const int i) const { return ogdual(x0[i], v[i]); }
    double ldy(const double* p) const { return *p; }
};

// og_dir_entry's walk, on DirXSeeded
double seeded_entry(int e, const double* x0, const double* v, const double* y0, const double* cv, const double* dfrag,
                    int* row) {
    const DirXSeeded xd{x0, v, -1};
    for (int g = 0; g < OgGen::N_GROUPS; ++g) {
        const int N = OgGen::G_LEN(g);
        if (OgGen::G_KIND(g) == 0) {
            if (e < N) return OgGen::item_value(g, 0, e, xd, y0, cv, row).d;
            e -= N;
            continue;
        }
        const int here = N * OgGen::G_NMV(g);
        if (e >= here) {
            e -= here;
            continue;
        }
        const int s = e / N, k = e - s * N, slot = OgGen::G_MV0(g) + s;
        *row = OgGen::G_ROW(g, s) + k;
        const double* dphase = dfrag + OgGen::DFRAG_OFF(OgGen::G_PHASE(g));
        double dy = 0.0;
        for (int l = 0; l < N; ++l)
            dy = __builtin_fma(OgGen::mv_operand(slot, l, xd, cv).d, og_par_dfrag(dphase, N, k, l), dy);
        return dy - OgGen::tail_one(slot, k, xd, cv).d;
    }
    *row = 0;
    return 0.0;
}
#endif

}  // namespace

int main(int argc, char** argv) {
    const int n = OgGen::N_VAR, m = OgGen::M, ncv = OgGen::N_CVEC > 0 ? OgGen::N_CVEC : 1;
    const bool seeded = argc == 4 && !std::strcmp(argv[3], "seeded");
    if (argc != 3 && !seeded) {
        std::fprintf(stderr, "usage: %s <file of x0, cv, D per phase, V> <output file> [seeded]\n", argv[0]);
        return 2;
    }
#ifndef OG_GEN_HAS_PAR
    if (seeded) {
        std::fprintf(stderr, "%s: the header has no run-time parameters\n", argv[0]);
        return 2;
    }
#endif
    std::vector<double> x0(n), cv(ncv), V;
    std::vector<std::vector<double>> D(OgGen::N_PHASE);
    FILE* fh = std::fopen(argv[1], "rb");
    bool ok = fh && std::fread(x0.data(), 8, n, fh) == (size_t)n && std::fread(cv.data(), 8, ncv, fh) == (size_t)ncv;
    long frag_total = 0;
    for (int p = 0; ok && p < OgGen::N_PHASE; ++p) {
        const size_t N = (size_t)OgGen::PHASE_NODES(p);
        D[p].resize(N * N);
        ok = std::fread(D[p].data(), 8, N * N, fh) == N * N;
        if (OgGen::DFRAG_OFF(p) != frag_total) ok = false;
        frag_total += ogk_frag_size((int)N);
    }
    std::vector<double> one(n);
    while (ok && std::fread(one.data(), 8, n, fh) == (size_t)n) V.insert(V.end(), one.begin(), one.end());
    if (!ok || V.empty() || std::fgetc(fh) != EOF) {
        std::fprintf(stderr, "%s: unexpected size\n", argv[1]);
        return 2;
    }
    std::fclose(fh);
    const int K = (int)(V.size() / (size_t)n);

    // F(x0) and y0, as oracle/twin.cpp evaluates
    std::vector<double> F0(m), y0(OgGen::N_Y0);
    const XVec xv{x0.data()};
    double out[OgGen::MAX_OUT > OgGen::MAX_NMV ? OgGen::MAX_OUT : OgGen::MAX_NMV];
    for (int g = 0; g < OgGen::N_GROUPS; ++g) {
        const int L = OgGen::G_LEN(g), nout = OgGen::G_NOUT(g);
        if (OgGen::G_KIND(g) == 0) {
            for (int k = 0; k < L; ++k) {
                OgGen::group_eval(g, k, xv, (const double*)nullptr, cv.data(), out);
                for (int o = 0; o < nout; ++o) F0[OgGen::G_ROW(g, o) + k] = out[o];
            }
            continue;
        }
        const int mv0 = OgGen::G_MV0(g), nmv = OgGen::G_NMV(g);
        const double* Dp = D[OgGen::G_PHASE(g)].data();
        std::vector<double> operand((size_t)L);
        for (int s = 0; s < nmv; ++s) {
            for (int l = 0; l < L; ++l) operand[l] = OgGen::mv_operand(mv0 + s, l, xv, cv.data());
            for (int k = 0; k < L; ++k) {
                double acc = 0.0;
                for (int l = 0; l < L; ++l) acc = __builtin_fma(operand[l], Dp[(size_t)k * L + l], acc);
                y0[OgGen::MV_Y0(mv0 + s) + k] = acc;
            }
        }
        double yk[OgGen::MAX_NMV];
        for (int k = 0; k < L; ++k) {
            for (int s = 0; s < nmv; ++s) yk[s] = y0[OgGen::MV_Y0(mv0 + s) + k];
            OgGen::group_eval(g, k, xv, (const double*)yk, cv.data(), out);
            for (int o = 0; o < nout; ++o) F0[OgGen::G_ROW(g, o) + k] = out[o];
        }
    }

    // the operand images, exactly as large as the device's
    double* dfrag = new double[frag_total > 0 ? frag_total : 1];
    for (int p = 0; p < OgGen::N_PHASE; ++p) ogk_frag_pack(OgGen::PHASE_NODES(p), D[p].data(), dfrag + OgGen::DFRAG_OFF(p));

    std::vector<double> dF((size_t)K * m, std::nan(""));
    std::vector<int> written((size_t)K * m, 0);
    const int entries = og_dir_entries<OgGen>();
    int bad = 0;
    for (int d = 0; d < K; ++d) {
        const double* v = V.data() + (size_t)d * n;
        for (int e = 0; e < entries; ++e) {
            int row = -1;
            double val;
#ifdef OG_GEN_HAS_PAR
            if (seeded) val = seeded_entry(e, x0.data(), v, y0.data(), cv.data(), dfrag, &row);
            else
#endif
                val = og_dir_entry<OgGen>(e, x0.data(), v, y0.data(), cv.data(), dfrag, &row);
            if (row < 0 || row >= m || written[(size_t)d * m + row]++) {
                std::printf("BAD ENTRY direction %d entry %d row %d\n", d, e, row);
                ++bad;
                continue;
            }
            dF[(size_t)d * m + row] = val;
        }
        for (int r = 0; r < m; ++r)
            if (written[(size_t)d * m + r] != 1) {
                std::printf("ROW %d of direction %d written %d times\n", r, d, written[(size_t)d * m + r]);
                ++bad;
            }
    }
    delete[] dfrag;

    FILE* fo = std::fopen(argv[2], "wb");
    if (!fo || std::fwrite(dF.data(), 8, dF.size(), fo) != dF.size() || std::fwrite(F0.data(), 8, m, fo) != (size_t)m) {
        std::fprintf(stderr, "%s: cannot write\n", argv[2]);
        return 2;
    }
    std::fclose(fo);
    std::printf("directions=%d rows=%d entries=%d bad=%d\n", K, m, entries, bad);
    return bad ? 1 : 0;
}
