// TEST INFRASTRUCTURE - host probe of the exact adjoint product F'(x)^T w (tests/test_adjoint.py).
//
// The kernels ogk_exact_adj / ogk_exact_adj_batch (csrc/ogk_kernels.hip) compute g_j = sum_r w_r dF_r/dx_j from the terms
// and in the ORDER that csrc/og_adj.h defines (og_adj_entry: 256 strided fma chains, then a fixed pairwise tree).  This
// program is that function on the host: the same header, the generated header of a problem (with or without run-time
// parameters) and og_dual.h, compiled with g++ and with clang++ (same bits) and once under AddressSanitizer / UBSan as a
// plain process (own main, nothing preloaded).
//
//   * The work lists OGT_COL / OGT_ELEM / OGT_SLOT are the generated header's own text.  The header emits its device
//     tables for hipcc only, as `static __device__ const int4 NAME[]`; this file reads that section as host arrays: it
//     defines int4, an empty __device__ and the compiler's macro around the include (og_math.h, which picks its
//     qualifiers by the same macro, is included before that and guarded).
//   * F(x0) and the base collocation products y0 are computed the CPU twin's way (plain loops, the product a
//     left-to-right fma chain over a dense D), so F0 equals oracle/twin.cpp's to the bit;
//   * every D is packed into the MFMA operand image (ogk.h: ogk_frag_pack) in one heap block of exactly the packed size,
//     and every weight vector is a heap block of exactly m doubles: a read past either is a sanitizer report;
//   * G is K * n doubles, pre-filled with NaN; every entry must have been written exactly once.
//
// Input: one file of doubles, x0[N_VAR] cv[max(N_CVEC, 1)], D[N][N] row-major for every phase, then W[K][M] (K from the
// file's size, at least 1).  Output file: G[K][N_VAR] F0[M], then per variable j its number of terms and the `reads` word
// of its own collocation slot (-1: x_j is no node of a collocated state), as doubles: terms[N_VAR] reads[N_VAR].
// Exit status 0, 1 when an entry is written twice or not written or a term's row is out of range, 2 on a usage error.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "ogk.h"
#include "og_math.h"
#include "og_dual.h"

struct int4 {
    int x, y, z, w;
};
#define __HIPCC__ 1
#define __device__
#include OG_GEN_HEADER
#undef __device__
#undef __HIPCC__

#include "og_adj.h"

namespace {

struct XVec {
    typedef double scalar;
    const double* x;
    double operator()(const int i) const { return x[i]; }
    double ldy(const double* p) const { return *p; }
};

struct Tables {
    const int4& col(const int j) const { return OGT_COL[j]; }
    const int4& elem(const int e) const { return OGT_ELEM[e]; }
    const ogt_int8& slot(const int s) const { return OGT_SLOT[s]; }
};

}  // namespace

int main(int argc, char** argv) {
    const int n = OgGen::N_VAR, m = OgGen::M, ncv = OgGen::N_CVEC > 0 ? OgGen::N_CVEC : 1;
    if (argc != 3) {
        std::fprintf(stderr, "usage: %s <file of x0, cv, D per phase, W> <output file>\n", argv[0]);
        return 2;
    }
    std::vector<double> x0(n), cv(ncv);
    std::vector<double*> W;
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
    while (ok) {
        double* one = new double[m];
        if (std::fread(one, 8, m, fh) != (size_t)m) {
            delete[] one;
            break;
        }
        W.push_back(one);
    }
    if (!ok || W.empty() || std::fgetc(fh) != EOF) {
        std::fprintf(stderr, "%s: unexpected size\n", argv[1]);
        return 2;
    }
    std::fclose(fh);
    const int K = (int)W.size();

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

    const Tables tab;
    std::vector<double> G((size_t)K * n, std::nan("")), terms(n), reads(n);
    std::vector<int> written((size_t)K * n, 0);
    int bad = 0;
    long total_terms = 0;
    for (int j = 0; j < n; ++j) {
        // every term's row inside [0, m), and no row twice in one column (ogk_exact_struct writes each entry once)
        const OgAdjCol c = og_adj_col<OgGen>(tab, j, x0.data(), cv.data());
        std::vector<int> seen(m, 0);
        for (int t = 0; t < c.terms; ++t) {
            int row = -1;
            (void)og_adj_term<OgGen>(tab, c, j, t, x0.data(), y0.data(), cv.data(), dfrag, &row);
            if (row < 0 || row >= m || seen[row]++) {
                std::printf("BAD TERM column %d term %d row %d\n", j, t, row);
                ++bad;
            }
        }
        terms[j] = c.terms;
        reads[j] = c.slot < 0 ? -1 : c.reads;
        total_terms += c.terms;
        if (bad) continue;
        for (int d = 0; d < K; ++d) {
            const double g = og_adj_entry<OgGen>(tab, j, W[d], x0.data(), y0.data(), cv.data(), dfrag);
            if (written[(size_t)d * n + j]++) ++bad;
            G[(size_t)d * n + j] = g;
        }
    }
    for (size_t i = 0; i < written.size(); ++i)
        if (written[i] != 1) {
            std::printf("ENTRY %d of vector %d written %d times\n", (int)(i % n), (int)(i / n), written[i]);
            ++bad;
        }
    delete[] dfrag;
    for (double* one : W) delete[] one;

    FILE* fo = std::fopen(argv[2], "wb");
    if (!fo || std::fwrite(G.data(), 8, G.size(), fo) != G.size() || std::fwrite(F0.data(), 8, m, fo) != (size_t)m ||
        std::fwrite(terms.data(), 8, n, fo) != (size_t)n || std::fwrite(reads.data(), 8, n, fo) != (size_t)n) {
        std::fprintf(stderr, "%s: cannot write\n", argv[2]);
        return 2;
    }
    std::fclose(fo);
    std::printf("vectors=%d variables=%d terms=%ld bad=%d\n", K, n, total_terms, bad);
    return bad ? 1 : 0;
}
