// TEST INFRASTRUCTURE - host probe of the exact second derivatives of w . F in the run-time parameters
// (tests/test_parameter_hessian.py).
//
// The kernels ogk_exact_pp / ogk_exact_pp_batch (csrc/ogk_kernels.hip) compute S_kl = sum_r w_r d2F_r/dtheta_k dtheta_l
// from the entries that csrc/og_pp.h defines, in the order of sums of csrc/og_adj.h.  This program is og_pp_entry on the
// host: the same headers and the generated header of a parameterised problem, compiled with a host compiler and once
// under AddressSanitizer / UBSan as a plain process (own main, nothing preloaded).  F(x0), y0 and the operand images are
// computed as tests/mix_probe.cpp does.
//
// Input: one file of doubles, x0[N_VAR] cv[N_CVEC], D[N][N] row-major for every phase, then K weight vectors W[K][M]
// (K from the file's size, at least 1).  Output file, with PAIRS = N_PAR (N_PAR + 1) / 2 pairs (k, l), k <= l, in
// row-major order of the upper triangle:
//   S[K][N_PAR][N_PAR]   the second derivatives (pre-filled with NaN; every entry must be written exactly once);
//   A[K][N_PAR][N_PAR]   sum_r |w_r d2F_r/dtheta_k dtheta_l| over the entries walked, the unit of the errors of an entry;
//   F0[M];
//   owner[PAIRS] partner[PAIRS] entries[PAIRS]   which list the probe walked for the pair and how long it is;
//   D1[PAIRS][M] D2[PAIRS][M] have[PAIRS][M]     the slot-1 and the slot-2 first-order parts of the pair's entries by
//                        row (0 where the owner's list has no entry in the row) and whether it has one;
//   checked2[PAIRS]      the number of the pair's entries whose slot-2 part was held to the partner's og_par_entry.
// The probe fails (exit status 1) unless every entry's slot-1 part is og_par_entry of the owner at that entry bit for
// bit, its slot-2 part og_par_entry of the partner at the same row bit for bit wherever the partner's lists hold the row
// in the same shape (a row item; a collocation entry with the same reads word - see og_pp.h), every row is in range and
// no row appears twice in one list, and every entry of S is written exactly once.  2 on a usage error.
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

#include "og_par.h"
#include "og_pp.h"

namespace {

struct XVec {
    typedef double scalar;
    const double* x;
    double operator()(const int i) const { return x[i]; }
    double ldy(const double* p) const { return *p; }
};

// (any NaN equals any NaN: the payload is the compiler's)
bool same_bits(const double a, const double b) { return (a != a && b != b) || std::memcmp(&a, &b, sizeof a) == 0; }

// the shape of entry e of parameter kp's lists: -1 a row item, else the reads word of its collocation slot
int entry_shape(const int kp, int e) {
    for (int i = OgGen::PAR_ROW_PTR(kp); i < OgGen::PAR_ROW_PTR(kp + 1); ++i) {
        const int len = OgGen::G_LEN(OgGen::PAR_ROW_G(i));
        if (e < len) return -1;
        e -= len;
    }
    for (int i = OgGen::PAR_SLOT_PTR(kp); i < OgGen::PAR_SLOT_PTR(kp + 1); ++i) {
        const int N = OgGen::G_LEN(OgGen::PAR_SLOT_G(i));
        if (e < N) return OgGen::PAR_SLOT_READS(i);
        e -= N;
    }
    return -2;
}

}  // namespace

int main(int argc, char** argv) {
    const int n = OgGen::N_VAR, m = OgGen::M, ncv = OgGen::N_CVEC, n_par = OgGen::N_PAR;
    const int pairs = n_par * (n_par + 1) / 2;
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

    const size_t pp = (size_t)n_par * n_par, kpp = (size_t)K * pp, qm = (size_t)pairs * m;
    std::vector<double> S(kpp, std::nan("")), A(kpp, std::nan("")), D1(qm, 0.0), D2(qm, 0.0), have(qm, 0.0);
    std::vector<double> owner(pairs), partner(pairs), entries(pairs), checked2(pairs, 0.0);
    std::vector<int> written(kpp, 0);
    int bad = 0;
    long total = 0;
    for (int q = 0; q < pairs; ++q) {
        const OgPpPair p = og_pp_pair<OgGen>(q);
        owner[q] = p.owner, partner[q] = p.partner, entries[q] = p.entries;
        total += p.entries;
        if (p.k > p.l || p.l >= n_par || p.entries != OgGen::PAR_ENTRIES(p.owner) ||
            p.entries > OgGen::PAR_ENTRIES(p.partner) || p.owner + p.partner != p.k + p.l) {
            std::printf("BAD PAIR %d: (%d, %d) owner %d partner %d entries %d\n", q, p.k, p.l, p.owner, p.partner, p.entries);
            ++bad;
            continue;
        }
        // the partner's own entries by row: value and shape
        std::vector<double> pval(m, 0.0);
        std::vector<int> pshape(m, -2);
        for (int e = 0; e < OgGen::PAR_ENTRIES(p.partner); ++e) {
            int row = -1;
            const double v = og_par_entry<OgGen>(p.partner, e, x0.data(), y0.data(), cv.data(), dfrag, &row);
            if (row < 0 || row >= m || pshape[row] != -2) {
                std::printf("BAD PARTNER ENTRY pair %d entry %d row %d\n", q, e, row);
                ++bad;
                continue;
            }
            pval[row] = v;
            pshape[row] = entry_shape(p.partner, e);
        }
        std::vector<OgPpTerm> term((size_t)p.entries);
        std::vector<int> rows((size_t)p.entries, -1);
        for (int e = 0; e < p.entries; ++e) {
            int row = -1, row1 = -1;
            term[e] = og_pp_term<OgGen>(p.owner, p.partner, e, x0.data(), y0.data(), cv.data(), dfrag, &row);
            const double first = og_par_entry<OgGen>(p.owner, e, x0.data(), y0.data(), cv.data(), dfrag, &row1);
            if (row < 0 || row >= m || row != row1 || have[(size_t)q * m + row] != 0.0) {
                std::printf("BAD ENTRY pair %d entry %d row %d (og_par_entry: %d)\n", q, e, row, row1);
                ++bad;
                continue;
            }
            rows[e] = row;
            have[(size_t)q * m + row] = 1.0;
            D1[(size_t)q * m + row] = term[e].d1;
            D2[(size_t)q * m + row] = term[e].d2;
            if (!same_bits(term[e].d1, first)) {
                std::printf("SLOT 1 of pair %d entry %d row %d: %.17g, og_par_entry of the owner %.17g\n", q, e, row,
                            term[e].d1, first);
                ++bad;
            }
            if (pshape[row] != -2 && pshape[row] == entry_shape(p.owner, e)) {
                checked2[q] += 1.0;
                if (!same_bits(term[e].d2, pval[row])) {
                    std::printf("SLOT 2 of pair %d entry %d row %d: %.17g, og_par_entry of the partner %.17g\n", q, e, row,
                                term[e].d2, pval[row]);
                    ++bad;
                }
            }
        }
        if (bad) continue;
        for (int d = 0; d < K; ++d) {
            double scale = 0.0;
            for (int e = 0; e < p.entries; ++e) scale += std::fabs(W[d][rows[e]] * term[e].dd);
            const double s = og_pp_entry<OgGen>(q, W[d], x0.data(), y0.data(), cv.data(), dfrag);
            const size_t at = (size_t)d * pp + (size_t)p.k * n_par + p.l, ta = (size_t)d * pp + (size_t)p.l * n_par + p.k;
            ++written[at];
            S[at] = s, A[at] = scale;
            if (ta != at) {
                ++written[ta];
                S[ta] = s, A[ta] = scale;
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
    if (!fo || std::fwrite(S.data(), 8, kpp, fo) != kpp || std::fwrite(A.data(), 8, kpp, fo) != kpp ||
        std::fwrite(F0.data(), 8, m, fo) != (size_t)m || std::fwrite(owner.data(), 8, pairs, fo) != (size_t)pairs ||
        std::fwrite(partner.data(), 8, pairs, fo) != (size_t)pairs ||
        std::fwrite(entries.data(), 8, pairs, fo) != (size_t)pairs || std::fwrite(D1.data(), 8, qm, fo) != qm ||
        std::fwrite(D2.data(), 8, qm, fo) != qm || std::fwrite(have.data(), 8, qm, fo) != qm ||
        std::fwrite(checked2.data(), 8, pairs, fo) != (size_t)pairs) {
        std::fprintf(stderr, "%s: cannot write\n", argv[2]);
        return 2;
    }
    std::fclose(fo);
    std::printf("vectors=%d parameters=%d pairs=%d entries=%ld bad=%d\n", K, n_par, pairs, total, bad);
    return bad ? 1 : 0;
}
