// og_adj.h - exact adjoint products F'(x)^T w: the terms of one entry of the result and the ORDER of their sum.
//
// g_j = sum_r w_r dF_r/dx_j for a weight vector w over the rows of F = [cost | c_eq | c_ineq].  Column j of the exact
// Jacobian is what ogk_exact_struct (csrc/ogk_kernels.hip) writes with a unit seed on x_j: the row items of
// OGT_ELEM[OGT_COL[j].x .. .y) and, when x_j is node l of a collocated state, that state's N defect rows.  Here each of
// those entries is multiplied by w[row] and summed where it is computed: no J_T, no pattern, no fill, one double per
// variable.
//
// A sum over up to thousands of terms needs a reduction across the threads of a workgroup, so - unlike og_dir.h and
// og_par.h, where one thread computes an entry - the order is part of the definition.  It is fixed here, as the function
// the host probe calls (og_adj_entry), and the kernels ogk_exact_adj / ogk_exact_adj_batch implement the same order:
//   1. the terms of column j are numbered: t in [0, items) is row item OGT_ELEM[OGT_COL[j].x + t]; t = items + k is
//      defect row k of the column's own collocation block (none when x_j is no collocated state);
//   2. OG_ADJ_CHAINS = 256 partial sums: chain c runs over the terms c, c + 256, c + 512, ... in ascending order,
//      acc = fma(w[row], entry, acc) from +0.0 (og_adj_chain);
//   3. a fixed pairwise tree over the 256 partial sums (og_adj_tree): inside every block of 64 chains
//      p[i] = p[i] + p[i + s] for s = 32, 16, 8, 4, 2, 1 (a wavefront's shuffle-down reduction), then
//      (p[0] + p[64]) + (p[128] + p[192]).
// No atomics and nothing that depends on scheduling.  Consequences: a row with w[row] == 0 is NOT skipped (0 * inf is
// NaN, as the product J^T w would give); a variable that no row reads gets +0.0 (every chain is +0.0, and so is every
// sum of the tree); vector d of a call with K weight vectors is bit for bit the call with that vector alone (every vector
// has chains of its own).  Run-time parameters are constants: OgAdjX has no member par_seed.
//
// Same source for hipcc and for a host compiler (tests/adj_probe.cpp).  T is the user's view of the generated tables:
// col(j) and elem(e) return a record with the members x, y, z, w, slot(s) one with int v[8] - the kernels read the
// device tables of the generated header, the probe the same text compiled for the host.
//
// Include after og_dual.h and the generated header (with or without run-time parameters).
#ifndef OG_ADJ_H
#define OG_ADJ_H

#include "og_dual.h"
#include "og_par.h"         // og_par_dfrag: D[k][l] out of the operand image

#define OG_ADJ_CHAINS 256

// x(i) with the unit seed on x_j (ogk_kernels.hip: XDual)
struct OgAdjX {
    typedef ogdual scalar;
    const double* x0;
    int j;
    OG_HDI ogdual operator()(const int i) const { return ogdual(x0[i], i == j ? 1.0 : 0.0); }
    OG_HDI double ldy(const double* p) const { return *p; }
};

// What a column's terms need, found once per column: its row items, and its own collocation block - slot < 0 when x_j
// is no node of a collocated state; else x_j is node l of the state behind collocation slot `slot`, opd the derivative
// of that operand, reads the slot's bits (bit 0: the dynamics term at node k reads the state at node k; bit 1: it reads
// the state's slice in some other way, every node then).
struct OgAdjCol {
    int e0, items, terms;
    int slot, l, N, phase, row0, reads;
    double opd;
};

template <class G, class T>
OG_HDI OgAdjCol og_adj_col(const T& tab, const int j, const double* x0, const double* cv) {
    OgAdjCol c;
    const auto rec = tab.col(j);
    c.e0 = rec.x;
    c.items = rec.y - rec.x;
    c.slot = -1;
    c.l = c.N = c.phase = c.row0 = c.reads = 0;
    c.opd = 0.0;
    const int own_lo = rec.z, own_hi = rec.w & 0x3fffffff;
    if (own_hi > own_lo) {
        for (int s = 0; s < G::N_MV; ++s) {
            const int leaf = tab.slot(s).v[2], len = tab.slot(s).v[0];
            if (j >= leaf && j < leaf + len) {
                c.slot = s;
                c.l = j - leaf;
            }
        }
        if (c.slot >= 0) {
            c.N = tab.slot(c.slot).v[0];
            c.phase = tab.slot(c.slot).v[5];
            c.row0 = tab.slot(c.slot).v[3];
            c.reads = tab.slot(c.slot).v[6];
            c.opd = G::mv_operand(c.slot, c.l, OgAdjX{x0, j}, cv).d;
        }
    }
    c.terms = c.items + c.N;
    return c;
}

// Term t in [0, c.terms) of column j -> the entry dF_row/dx_j, *row its row of F: bit for bit what ogk_exact_struct
// writes at J_T[j][row].  dfrag: the packed operand images of all phases (phase p at G::DFRAG_OFF(p)).
template <class G, class T>
OG_HDI double og_adj_term(const T& tab, const OgAdjCol& c, const int j, const int t, const double* x0, const double* y0,
                          const double* cv, const double* dfrag, int* row) {
    const OgAdjX xd{x0, j};
    if (t < c.items) {
        const auto it = tab.elem(c.e0 + t);
        return G::item_value(it.x, it.y, it.z, xd, y0, cv, row).d;
    }
    const int k = t - c.items;
    *row = c.row0 + k;
    double v = __builtin_fma(c.opd, og_par_dfrag(dfrag + G::DFRAG_OFF(c.phase), c.N, k, c.l), 0.0);
    if ((c.reads & 2) || ((c.reads & 1) && k == c.l)) v = v - G::tail_one(c.slot, k, xd, cv).d;
    return v;
}

// Partial sum `chain` in [0, OG_ADJ_CHAINS) of column j against the weight vector w[M]
template <class G, class T>
OG_HDI double og_adj_chain(const T& tab, const OgAdjCol& c, const int j, const int chain, const double* w,
                           const double* x0, const double* y0, const double* cv, const double* dfrag) {
    double acc = 0.0;
    for (int t = chain; t < c.terms; t += OG_ADJ_CHAINS) {
        int row;
        const double e = og_adj_term<G>(tab, c, j, t, x0, y0, cv, dfrag, &row);
        acc = __builtin_fma(w[row], e, acc);
    }
    return acc;
}

// The tree over the OG_ADJ_CHAINS partial sums (p is overwritten)
OG_HDI double og_adj_tree(double* p) {
    for (int s = 32; s >= 1; s >>= 1)
        for (int b = 0; b < OG_ADJ_CHAINS; b += 64)
            for (int i = 0; i < s; ++i) p[b + i] = p[b + i] + p[b + i + s];
    return (p[0] + p[64]) + (p[128] + p[192]);
}

// g_j of F'(x)^T w: the definition
template <class G, class T>
OG_HDI double og_adj_entry(const T& tab, const int j, const double* w, const double* x0, const double* y0,
                           const double* cv, const double* dfrag) {
    const OgAdjCol c = og_adj_col<G>(tab, j, x0, cv);
    double p[OG_ADJ_CHAINS];
    for (int chain = 0; chain < OG_ADJ_CHAINS; ++chain) p[chain] = og_adj_chain<G>(tab, c, j, chain, w, x0, y0, cv, dfrag);
    return og_adj_tree(p);
}

#endif /* OG_ADJ_H */
