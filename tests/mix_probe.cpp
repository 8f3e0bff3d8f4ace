// TEST INFRASTRUCTURE - host probe of the exact mixed derivatives d(F'(x)^T w)/dtheta_k (tests/test_mixed.py).
//
// The kernels ogk_exact_mix / ogk_exact_mix_batch (csrc/ogk_kernels.hip) compute s_{k,j} = sum_r w_r d2F_r/dx_j dtheta_k
// from the terms that csrc/og_mix.h defines, in the order of sums of csrc/og_adj.h.  This program is og_mix_entry on the
// host: the same headers and the generated header of a parameterised problem, compiled with g++ and with clang++ (same
// bits) and once under AddressSanitizer / UBSan as a plain process (own main, nothing preloaded).  The tables, F(x0), y0
// and the operand images are read and computed as tests/adj_probe.cpp does.
//
// Input: one file of doubles, x0[N_VAR] cv[N_CVEC], D[N][N] row-major for every phase, then K weight vectors W[K][M]
// (K from the file's size, at least 1).  Output file:
//   S[K][N_PAR][N_VAR]   the mixed derivatives;
//   G[K][N_VAR]          the slot-1 first-order parts of the same terms summed in the same order, which must be
//                        adj_probe's F'(x)^T w bit for bit (they are the same bits for every parameter, or the probe
//                        fails);
//   A[K][N_PAR][N_VAR]   sum_r |w_r d2F_r/dx_j dtheta_k|, the unit of the errors of an entry;
//   F0[M];
//   P[N_PAR][M]          the slot-2 first-order part of the row items of a row, dF_row/dtheta_k by the item - the same
//                        bits from every column that has an item in the row, or the probe fails - and have[M], whether any
//                        column has an item in the row;
//   terms[N_VAR] reads[N_VAR] heavy[N_VAR]   per variable its number of terms, the `reads` word of its own collocation
//                        slot (-1: x_j is no node of a collocated state), whether the tracer marked the column heavy.
// Exit status 0, 1 when an entry is written twice or not written, a term's row is out of range or one of the two
// invariants above fails, 2 on a usage error.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "ogk.h"
#include "og_math.h"
#include "og_dual.h"
#include "og_dual2.h"

struct int4 {
    int x, y, z, w;
};
#define __HIPCC__ 1
#define __device__
#include OG_GEN_HEADER
#undef __device__
#undef __HIPCC__

#include "og_mix.h"

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

// (any NaN equals any NaN: the payload is the compiler's)
bool same_bits(const double a, const double b) { return (a != a && b != b) || std::memcmp(&a, &b, sizeof a) == 0; }

}  // namespace

int main(int argc, char** argv) {
    const int n = OgGen::N_VAR, m = OgGen::M, ncv = OgGen::N_CVEC, n_par = OgGen::N_PAR;
    if (argc != 3) {
        std::fprintf(stderr, "usage: %s <file of x0, cv, D per phase, W> <output file>\n", argv[0]);
        return 2;
    }
    std::vector<double> x0(n), cv(ncv), rest;
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
    double one;
    while (ok && std::fread(&one, 8, 1, fh) == 1) rest.push_back(one);
    if (!ok || rest.empty() || rest.size() % (size_t)m != 0) {
        std::fprintf(stderr, "%s: unexpected size\n", argv[1]);
        return 2;
    }
    std::fclose(fh);
    const int K = (int)(rest.size() / (size_t)m);
    // every weight vector a heap block of exactly its size: a read past it is a sanitizer report
    std::vector<double*> W(K);
    for (int d = 0; d < K; ++d) {
        W[d] = new double[m];
        std::memcpy(W[d], rest.data() + (size_t)d * m, sizeof(double) * m);
    }

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
    const size_t kn = (size_t)K * n, kpn = kn * n_par, pm = (size_t)n_par * m;
    std::vector<double> S(kpn, std::nan("")), G(kn, std::nan("")), A(kpn, std::nan("")), P(pm, 0.0), have(m, 0.0);
    std::vector<double> terms(n), reads(n), heavy(n);
    std::vector<int> written(kpn, 0);
    std::vector<char> set(pm, 0);
    int bad = 0;
    long total_terms = 0;
    for (int j = 0; j < n; ++j) {
        const OgAdjCol c = og_adj_col<OgGen>(tab, j, x0.data(), cv.data());
        terms[j] = c.terms;
        reads[j] = c.slot < 0 ? -1 : c.reads;
        heavy[j] = (OGT_COL[j].w >> 30) & 1;
        total_terms += c.terms;
        for (int kp = 0; kp < n_par; ++kp) {
            const int seed = OgGen::PAR_OFF + kp;
            // the terms once per (column, parameter): every term's row in [0, m) with no row twice in one column, a row
            // item's slot-2 part the same from every column
            std::vector<OgMixTerm> term((size_t)c.terms);
            std::vector<int> rows((size_t)c.terms, -1), seen(m, 0);
            for (int t = 0; t < c.terms; ++t) {
                int row = -1;
                term[t] = og_mix_term<OgGen>(tab, c, j, seed, t, x0.data(), y0.data(), cv.data(), dfrag, &row);
                if (row < 0 || row >= m || seen[row]++) {
                    std::printf("BAD TERM column %d parameter %d term %d row %d\n", j, kp, t, row);
                    ++bad;
                    continue;
                }
                rows[t] = row;
                if (t < c.items) {
                    // (the first column with an item in this row sets it, every later one must agree)
                    double& slot2 = P[(size_t)kp * m + row];
                    if (!set[(size_t)kp * m + row]) {
                        slot2 = term[t].d2;
                        set[(size_t)kp * m + row] = 1;
                    } else if (!same_bits(slot2, term[t].d2)) {
                        std::printf("SLOT 2 of row %d parameter %d differs in column %d\n", row, kp, j);
                        ++bad;
                    }
                    have[row] = 1.0;
                }
            }
            if (bad) continue;
            for (int d = 0; d < K; ++d) {
                // the first-order parts in the chains and the tree of og_adj.h, and the scale
                double p[OG_ADJ_CHAINS];
                double scale = 0.0;
                for (int chain = 0; chain < OG_ADJ_CHAINS; ++chain) {
                    double acc = 0.0;
                    for (int t = chain; t < c.terms; t += OG_ADJ_CHAINS) {
                        acc = __builtin_fma(W[d][rows[t]], term[t].d1, acc);
                        scale += std::fabs(W[d][rows[t]] * term[t].dd);
                    }
                    p[chain] = acc;
                }
                const double g = og_adj_tree(p);
                if (kp == 0) G[(size_t)d * n + j] = g;
                else if (!same_bits(G[(size_t)d * n + j], g)) {
                    std::printf("SLOT 1 of column %d vector %d differs for parameter %d\n", j, d, kp);
                    ++bad;
                }
                const size_t at = ((size_t)d * n_par + kp) * n + j;
                A[at] = scale;
                const double s = og_mix_entry<OgGen>(tab, j, seed, W[d], x0.data(), y0.data(), cv.data(), dfrag);
                if (written[at]++) ++bad;
                S[at] = s;
            }
        }
    }
    for (size_t i = 0; i < written.size(); ++i)
        if (written[i] != 1) {
            std::printf("ENTRY %d written %d times\n", (int)i, written[i]);
            ++bad;
        }
    delete[] dfrag;
    for (int d = 0; d < K; ++d) delete[] W[d];

    FILE* fo = std::fopen(argv[2], "wb");
    if (!fo || std::fwrite(S.data(), 8, kpn, fo) != kpn || std::fwrite(G.data(), 8, kn, fo) != kn ||
        std::fwrite(A.data(), 8, kpn, fo) != kpn || std::fwrite(F0.data(), 8, m, fo) != (size_t)m ||
        std::fwrite(P.data(), 8, pm, fo) != pm || std::fwrite(have.data(), 8, m, fo) != (size_t)m ||
        std::fwrite(terms.data(), 8, n, fo) != (size_t)n || std::fwrite(reads.data(), 8, n, fo) != (size_t)n ||
        std::fwrite(heavy.data(), 8, n, fo) != (size_t)n) {
        std::fprintf(stderr, "%s: cannot write\n", argv[2]);
        return 2;
    }
    std::fclose(fo);
    std::printf("vectors=%d parameters=%d variables=%d terms=%ld bad=%d\n", K, n_par, n, total_terms, bad);
    return bad ? 1 : 0;
}
