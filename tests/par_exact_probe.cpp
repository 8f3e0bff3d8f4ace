// TEST INFRASTRUCTURE - host probe of the exact parameter Jacobian (tests/test_parameter_exact.py).
//
// The kernels ogk_exact_par / ogk_exact_par_batch (csrc/ogk_kernels.hip) compute every entry of dF/dtheta with ONE
// function, og_par_entry (csrc/og_par.h), from x0, y0, cv and the D operand image alone.  This program is that function
// on the host: the same header, the generated header of a parameterised problem and og_dual.h, compiled with g++ and with
// clang++ (same bits) and once under AddressSanitizer / UBSan as a plain process (own main, nothing preloaded).
//
//   * F(x0) and the base collocation products y0 are computed the CPU twin's way (plain loops, the product a
//     left-to-right fma chain over a dense D), so F0 equals oracle/twin.cpp's to the bit;
//   * every D is packed into the MFMA operand image (ogk.h: ogk_frag_pack) in one heap block of exactly the packed size:
//     a read past it is a sanitizer report;
//   * dF is n_par * m doubles, zero-filled, then every entry of every parameter's work lists is stored at its row.
//
// Input: one file of doubles, x0[N_VAR] cv[max(N_CVEC, 1)] then D[N][N] row-major for every phase.  Output file:
// dF[N_PAR][M] F0[M].  Exit status 0, 1 when an entry's row is out of range or written twice, 2 on a usage error.
#include <cstdio>
#include <vector>

#include "ogk.h"
#include "og_dual.h"
#include OG_GEN_HEADER
#include "og_par.h"

namespace {

struct XVec {
    typedef double scalar;
    const double* x;
    double operator()(const int i) const { return x[i]; }
    double ldy(const double* p) const { return *p; }
};

}  // namespace

int main(int argc, char** argv) {
    const int n = OgGen::N_VAR, m = OgGen::M, ncv = OgGen::N_CVEC > 0 ? OgGen::N_CVEC : 1, n_par = OgGen::N_PAR;
    if (argc != 3) {
        std::fprintf(stderr, "usage: %s <file of x0, cv, D per phase> <output file>\n", argv[0]);
        return 2;
    }
    std::vector<double> x0(n), cv(ncv);
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
    if (!ok || std::fgetc(fh) != EOF) {
        std::fprintf(stderr, "%s: unexpected size\n", argv[1]);
        return 2;
    }
    std::fclose(fh);

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

    std::vector<double> dF((size_t)n_par * m, 0.0);
    std::vector<char> written((size_t)n_par * m, 0);
    int bad = 0;
    for (int kp = 0; kp < n_par; ++kp)
        for (int e = 0; e < OgGen::PAR_ENTRIES(kp); ++e) {
            int row = -1;
            const double v = og_par_entry<OgGen>(kp, e, x0.data(), y0.data(), cv.data(), dfrag, &row);
            if (row < 0 || row >= m || written[(size_t)kp * m + row]) {
                std::printf("BAD ENTRY parameter %d entry %d row %d\n", kp, e, row);
                ++bad;
                continue;
            }
            written[(size_t)kp * m + row] = 1;
            dF[(size_t)kp * m + row] = v;
        }
    delete[] dfrag;

    FILE* fo = std::fopen(argv[2], "wb");
    if (!fo || std::fwrite(dF.data(), 8, dF.size(), fo) != dF.size() || std::fwrite(F0.data(), 8, m, fo) != (size_t)m) {
        std::fprintf(stderr, "%s: cannot write\n", argv[2]);
        return 2;
    }
    std::fclose(fo);
    std::printf("parameters=%d rows=%d bad=%d\n", n_par, m, bad);
    return bad ? 1 : 0;
}
