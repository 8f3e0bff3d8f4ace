// TEST INFRASTRUCTURE - host probe of the exact sparse Hessian of w . F (tests/test_hessian_matrix.py).
//
// The kernels ogk_exact_hess / ogk_exact_hess_batch (csrc/ogk_kernels.hip) compute every stored entry of the pattern of
// codegen.HessianPlan from the terms that csrc/og_hess.h defines, in the order of sums of csrc/og_adj.h.  This program is
// og_hess_entry on the host: the same headers and the generated header of a problem, compiled with g++ and once under
// AddressSanitizer / UBSan as a plain process (own main, nothing preloaded).  The tables, F(x0), y0 and the operand images
// are read and computed as tests/hvp_probe.cpp does; the plan is data and comes with the input.
//
// Input: one file of doubles, x0[N_VAR] cv[max(N_CVEC, 1)], D[N][N] row-major for every phase, then the plan - nnz,
// the length of tlist and K, then indptr[N_VAR + 1] cols[nnz] owner[nnz] tptr[nnz + 1] tlist[max(length, 1)], every
// integer as a double - then W[K][M].  Output file: H[K][nnz] in pattern order, S[K][nnz] = sum over the entry's listed
// terms of |w_r d2F_r/dx_owner dx_partner| (the unit of the errors of an entry), F0[M], and terms[N_VAR], the number of
// terms of every column, as doubles.
// Exit status 0, 1 when the plan is malformed (pointers not monotone, an index out of range, a partner above its row, a
// list that does not ascend or names a term the owner does not have), when a stored entry is written twice or not
// written or a term's row is out of range, 2 on a usage error.
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

#include "og_hess.h"

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

// `count` integers stored as doubles -> a heap block of exactly that size
bool take(const std::vector<double>& src, size_t* at, size_t count, std::vector<int>* out) {
    if (*at + count > src.size()) return false;
    out->resize(count);
    for (size_t i = 0; i < count; ++i) {
        const double v = src[*at + i];
        if (!(v >= 0.0 && v < 2147483648.0) || v != std::floor(v)) return false;
        (*out)[i] = (int)v;
    }
    *at += count;
    return true;
}

}  // namespace

int main(int argc, char** argv) {
    const int n = OgGen::N_VAR, m = OgGen::M, ncv = OgGen::N_CVEC > 0 ? OgGen::N_CVEC : 1;
    if (argc != 3) {
        std::fprintf(stderr, "usage: %s <file of x0, cv, D per phase, plan, W> <output file>\n", argv[0]);
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
    if (fh) std::fclose(fh);
    std::vector<int> head, indptr, cols, owner, tptr, tlist;
    size_t at = 0;
    ok = ok && take(rest, &at, 3, &head);
    const int nnz = ok ? head[0] : 0, ntl = ok ? head[1] : 0, K = ok ? head[2] : 0;
    ok = ok && K >= 1 && take(rest, &at, (size_t)n + 1, &indptr) && take(rest, &at, (size_t)nnz, &cols) &&
         take(rest, &at, (size_t)nnz, &owner) && take(rest, &at, (size_t)nnz + 1, &tptr) &&
         take(rest, &at, (size_t)(ntl > 0 ? ntl : 1), &tlist) && rest.size() - at == (size_t)K * m;
    if (!ok) {
        std::fprintf(stderr, "%s: unexpected size or content\n", argv[1]);
        return 2;
    }
    // every weight vector a heap block of exactly its size: a read past it is a sanitizer report
    std::vector<double*> W(K);
    for (int d = 0; d < K; ++d) {
        W[d] = new double[m];
        std::memcpy(W[d], rest.data() + at + (size_t)d * m, sizeof(double) * m);
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
    int bad = 0;
    std::vector<double> terms(n);
    std::vector<OgAdjCol> col(n);
    for (int j = 0; j < n; ++j) {
        col[j] = og_adj_col<OgGen>(tab, j, x0.data(), cv.data());
        terms[j] = col[j].terms;
    }
    // the plan: what og_hessian_matrix_load refuses
    if (indptr[0] != 0 || indptr[n] != nnz || tptr[0] != 0 || tptr[nnz] != ntl) ++bad;
    for (int j = 0; j < n && !bad; ++j)
        if (indptr[j + 1] < indptr[j] || indptr[j + 1] > nnz) ++bad;
    for (int j = 0; j < n && !bad; ++j)
        for (int p = indptr[j]; p < indptr[j + 1]; ++p) {
            const int l = cols[p];
            if (l > j || (p > indptr[j] && l <= cols[p - 1]) || (owner[p] != j && owner[p] != l) || tptr[p + 1] < tptr[p] ||
                tptr[p + 1] > ntl) {
                ++bad;
                break;
            }
            for (int i = tptr[p]; i < tptr[p + 1]; ++i)
                if (tlist[i] >= col[owner[p]].terms || (i > tptr[p] && tlist[i] <= tlist[i - 1])) ++bad;
        }
    if (bad) std::printf("BAD PLAN\n");

    const size_t kz = (size_t)K * nnz;
    std::vector<double> H(kz, std::nan("")), S(kz, std::nan(""));
    std::vector<int> written(kz, 0);
    long listed = 0;
    for (int j = 0; j < n && !bad; ++j)
        for (int p = indptr[j]; p < indptr[j + 1]; ++p) {
            const int own = owner[p], other = own == j ? cols[p] : j, nt = tptr[p + 1] - tptr[p];
            // the list of exactly its size on the heap
            int* list = new int[nt > 0 ? nt : 1];
            std::memcpy(list, tlist.data() + tptr[p], sizeof(int) * nt);
            listed += nt;
            for (int d = 0; d < K; ++d) {
                double scale = 0.0;
                for (int i = 0; i < nt; ++i) {
                    int row = -1;
                    const double e = og_hess_term<OgGen>(tab, col[own], own, other, list[i], x0.data(), y0.data(), cv.data(),
                                                         dfrag, &row);
                    if (row < 0 || row >= m) {
                        std::printf("BAD TERM entry %d term %d row %d\n", p, list[i], row);
                        ++bad;
                        continue;
                    }
                    scale += std::fabs(W[d][row] * e);
                }
                if (bad) continue;
                const size_t at_out = (size_t)d * nnz + p;
                if (written[at_out]++) ++bad;
                S[at_out] = scale;
                H[at_out] = og_hess_entry<OgGen>(tab, own, other, list, nt, W[d], x0.data(), y0.data(), cv.data(), dfrag);
            }
            delete[] list;
        }
    for (size_t i = 0; i < written.size(); ++i)
        if (written[i] != 1) {
            std::printf("ENTRY %d of vector %d written %d times\n", (int)(i % nnz), (int)(i / nnz), written[i]);
            ++bad;
        }
    delete[] dfrag;
    for (int d = 0; d < K; ++d) delete[] W[d];

    FILE* fo = std::fopen(argv[2], "wb");
    if (!fo || std::fwrite(H.data(), 8, kz, fo) != kz || std::fwrite(S.data(), 8, kz, fo) != kz ||
        std::fwrite(F0.data(), 8, m, fo) != (size_t)m || std::fwrite(terms.data(), 8, n, fo) != (size_t)n) {
        std::fprintf(stderr, "%s: cannot write\n", argv[2]);
        return 2;
    }
    std::fclose(fo);
    std::printf("vectors=%d entries=%d listed=%ld bad=%d\n", K, nnz, listed, bad);
    return bad ? 1 : 0;
}
