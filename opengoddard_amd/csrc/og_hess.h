// og_hess.h - the exact sparse Hessian of w.F: H_{jl} = sum_r w_r d2F_r/dx_j dx_l, one stored entry per unordered pair
// {j, l} of a static pattern, the terms of one entry and the order of their sum.
//
// The pattern and, per stored entry, its OWNER (one of the pair's two variables) and the list of the owner's term
// numbers that read the other variable - the PARTNER - are data (codegen.HessianPlan), not generated code.  The entry is
// og_hvp_entry (og_hvp.h) for column `owner` with the unit direction on the partner, restricted to the listed terms:
//   - the terms are those og_adj.h enumerates for the owner's column, in its numbering (t < items: row item
//     OGT_ELEM[OGT_COL[owner].x + t]; t = items + k: defect row k of the column's own collocation block);
//   - each listed term is evaluated on second-order dual numbers (og_dual2.h) with the unit seed on x_owner in slot 1
//     and the unit seed on x_partner in slot 2 (OgHessX; owner == partner on the diagonal: both seeds on one variable);
//     the term's value is the mixed part.  The operand term D[k][l] d2(operand_l)/dx_owner dx_partner is kept as in
//     og_hvp_term; for an affine operand it is +0.0, and only the diagonal lists it;
//   - acc = fma(w[row], term, acc) from +0.0 in chain t & 255 of the term's OWN number t, the listed terms in ascending
//     order, then og_adj_tree over the OG_ADJ_CHAINS partial sums - a chain without a listed term stays +0.0.
// A term that is not listed does not read the partner: every seed of slot 2 it sees is zero, so its mixed part is an
// exact zero (og_dual2.h: a part whose seeds are zero is left out), and adding +-0 to a chain that starts at +0.0 does
// not change the chain's bits.  Hence, for finite weights and a finite point, the entry is BIT FOR BIT
// hessian_vector_product(w, e_partner)[owner], sign of zero included - with ONE caveat, underflow: a listed product
// w[row] * term too small for a subnormal rounds to -0.0 when it is negative, and a chain that holds -0.0 and nothing
// else becomes +0.0 in the product (the next unlisted term adds +0.0) and stays -0.0 here.  With an infinite weight or
// a non-finite point the unlisted terms (0 * inf) are not reproduced either.
//
// How a kernel places terms and lanes is free as long as that equality holds.  ogk_exact_hess (csrc/ogk_kernels.hip)
// gives the thread that evaluates list position i the chain tlist[i] & 255 in LDS and applies positions with one chain
// in ascending order; the tree's levels s = 32 .. 1 are a wavefront's shuffle-down reduction.
//
// Consequences, as in og_adj.h: reproducible to the bit; vector d of K is the call with that vector alone; a row with
// w[row] == 0 is NOT skipped; an entry without a listed term is +0.0.  Run-time parameters are constants: OgHessX has
// no member par_seed.
//
// Same source for hipcc (ogk_exact_hess, ogk_exact_hess_batch) and a host compiler (tests/hess_probe.cpp).  Include
// after the generated header.
#ifndef OG_HESS_H
#define OG_HESS_H

#include "og_dual2.h"
#include "og_adj.h"         // og_adj_col, OG_ADJ_CHAINS, og_adj_tree; og_par_dfrag through it

// x(i) with the unit seed on x_j in slot 1 and the unit seed on x_l in slot 2: OgHvpX with v = e_l, without a vector
struct OgHessX {
    typedef ogdual2 scalar;
    const double* x0;
    int j, l;
    OG_HDI ogdual2 operator()(const int i) const { return ogdual2(x0[i], i == j ? 1.0 : 0.0, i == l ? 1.0 : 0.0, 0.0); }
    OG_HDI double ldy(const double* p) const { return *p; }
};

// Term t in [0, c.terms) of column j (c = og_adj_col(j)) with the partner l, *row its row of F -> the mixed part
// d2F_row/dx_j dx_l: og_hvp_term(...).v for v = e_l, bit for bit.
template <class G, class T>
OG_HDI double og_hess_term(const T& tab, const OgAdjCol& c, const int j, const int l, const int t, const double* x0,
                           const double* y0, const double* cv, const double* dfrag, int* row) {
    const OgHessX xd{x0, j, l};
    if (t < c.items) {
        const auto it = tab.elem(c.e0 + t);
        return G::item_value(it.x, it.y, it.z, xd, y0, cv, row).dd;
    }
    const int k = t - c.items;
    *row = c.row0 + k;
    const double D = og_par_dfrag(dfrag + G::DFRAG_OFF(c.phase), c.N, k, c.l);
    double e = __builtin_fma(G::mv_operand(c.slot, c.l, xd, cv).dd, D, 0.0);
    if ((c.reads & 2) || ((c.reads & 1) && k == c.l)) e = e - G::tail_one(c.slot, k, xd, cv).dd;
    return e;
}

// The stored entry of the pair {owner, partner}: tlist[nt] the owner's term numbers that read the partner, ascending.
// The definition.
template <class G, class T>
OG_HDI double og_hess_entry(const T& tab, const int owner, const int partner, const int* tlist, const int nt,
                            const double* w, const double* x0, const double* y0, const double* cv, const double* dfrag) {
    const OgAdjCol c = og_adj_col<G>(tab, owner, x0, cv);
    double p[OG_ADJ_CHAINS];
    for (int chain = 0; chain < OG_ADJ_CHAINS; ++chain) p[chain] = 0.0;
    for (int i = 0; i < nt; ++i) {
        const int t = tlist[i];
        int row;
        const double e = og_hess_term<G>(tab, c, owner, partner, t, x0, y0, cv, dfrag, &row);
        p[t & (OG_ADJ_CHAINS - 1)] = __builtin_fma(w[row], e, p[t & (OG_ADJ_CHAINS - 1)]);
    }
    return og_adj_tree(p);
}

#endif /* OG_HESS_H */
