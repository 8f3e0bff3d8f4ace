// og_mix.h - exact mixed derivatives d(F'(x)^T w)/dtheta_k for run-time parameters: the terms of one entry and the
// order of their sum.
//
// s_{k,j} = sum_r w_r d2F_r/dx_j dtheta_k for weights w over the rows of F = [cost | c_eq | c_ineq] and a declared
// run-time parameter theta_k.  The terms of s_{k,j} are the terms og_adj.h enumerates for column j of the exact Jacobian
// - the row items, then the column's own collocation block - each evaluated on second-order dual numbers (og_dual2.h)
// with the unit seed on x_j in slot 1 and the unit seed on the parameter's table entry (PAR_OFF + k) in slot 2: OgMixX
// has a member par_seed, so OgGen::par_leaf (codegen._parameter_section) constructs scalar(cv[i], seed) for a parameter
// leaf, which for ogdual2 is "value and slot-2 seed".  The term's value is the mixed part.  Where og_adj_term has
// D[k][l] d(operand_l)/dx_j, the term here has D[k][l] d2(operand_l)/dx_j dtheta_k: kept, because a state's unit can be
// a parameter and then the operand reads it.  y0, the base collocation product, enters as a value only (ldy): a row item
// of a defect row is a column of another variable, and D x~ does not depend on that one.
//
// Slot 1 is the x_j seed, so by rule (a) of og_dual2.h a term's .d1 is og_adj_term bit for bit, and a row item's .d2
// is the item derivative of og_par.h.  By rule (b) a quantity that does not depend on both seeds has a mixed part of
// exactly +0.0 and never produces 0 * inf: a parameter nothing reads gets a row of +0.0.
//
// The ORDER of the sum is og_adj.h's and is not restated here: OG_ADJ_CHAINS strided chains
// acc = fma(w[row], term, acc) from +0.0 (og_mix_chain walks the terms as og_adj_chain does), then og_adj_tree.  The
// consequences are the adjoint's: reproducible to the bit; weight vector d of K is the call with that vector alone;
// w_r = 0 is not skipped; a variable nothing reads gets +0.0.
//
// Same source for hipcc (csrc/ogk_kernels.hip: ogk_exact_mix, ogk_exact_mix_batch) and a host compiler
// (tests/mix_probe.cpp).  Include after the generated header.  `seed` below is the TABLE index PAR_OFF + k.
#ifndef OG_MIX_H
#define OG_MIX_H

#include "og_dual2.h"
#include "og_adj.h"         // og_adj_col, OG_ADJ_CHAINS, og_adj_tree; og_par_dfrag through it

// x(i) with the unit seed on x_j in slot 1; the parameter at table index par_seed carries the unit seed of slot 2
struct OgMixX {
    typedef ogdual2 scalar;
    const double* x0;
    int j;
    int par_seed;
    OG_HDI ogdual2 operator()(const int i) const { return ogdual2(x0[i], i == j ? 1.0 : 0.0, 0.0, 0.0); }
    OG_HDI double ldy(const double* p) const { return *p; }
};

// One term: dd the mixed part d2F_row/dx_j dtheta_k - the term of s_{k,j} - d1 the part along x_j (og_adj_term's bits),
// d2 the part along theta_k (of a row item: the item derivative og_par_entry returns for that row)
struct OgMixTerm {
    double dd, d1, d2;
};

// Term t in [0, c.terms) of column j (c = og_adj_col(j)), *row its row of F
template <class G, class T>
OG_HDI OgMixTerm og_mix_term(const T& tab, const OgAdjCol& c, const int j, const int seed, const int t, const double* x0,
                             const double* y0, const double* cv, const double* dfrag, int* row) {
    const OgMixX xd{x0, j, seed};
    if (t < c.items) {
        const auto it = tab.elem(c.e0 + t);
        const ogdual2 e = G::item_value(it.x, it.y, it.z, xd, y0, cv, row);
        return OgMixTerm{e.dd, e.d1, e.d2};
    }
    const int k = t - c.items;
    *row = c.row0 + k;
    const double D = og_par_dfrag(dfrag + G::DFRAG_OFF(c.phase), c.N, k, c.l);
    const ogdual2 op = G::mv_operand(c.slot, c.l, xd, cv);
    OgMixTerm e{__builtin_fma(op.dd, D, 0.0), __builtin_fma(op.d1, D, 0.0), __builtin_fma(op.d2, D, 0.0)};
    if ((c.reads & 2) || ((c.reads & 1) && k == c.l)) {
        const ogdual2 tail = G::tail_one(c.slot, k, xd, cv);
        e = OgMixTerm{e.dd - tail.dd, e.d1 - tail.d1, e.d2 - tail.d2};
    }
    return e;
}

// Partial sum `chain` in [0, OG_ADJ_CHAINS) of column j for the weight vector w[M] and the parameter at table index seed
template <class G, class T>
OG_HDI double og_mix_chain(const T& tab, const OgAdjCol& c, const int j, const int seed, const int chain, const double* w,
                           const double* x0, const double* y0, const double* cv, const double* dfrag) {
    double acc = 0.0;
    for (int t = chain; t < c.terms; t += OG_ADJ_CHAINS) {
        int row;
        const double e = og_mix_term<G>(tab, c, j, seed, t, x0, y0, cv, dfrag, &row).dd;
        acc = __builtin_fma(w[row], e, acc);
    }
    return acc;
}

// s_{k,j} of d(F'(x)^T w)/dtheta_k, seed = PAR_OFF + k: the definition
template <class G, class T>
OG_HDI double og_mix_entry(const T& tab, const int j, const int seed, const double* w, const double* x0, const double* y0,
                           const double* cv, const double* dfrag) {
    const OgAdjCol c = og_adj_col<G>(tab, j, x0, cv);
    double p[OG_ADJ_CHAINS];
    for (int chain = 0; chain < OG_ADJ_CHAINS; ++chain)
        p[chain] = og_mix_chain<G>(tab, c, j, seed, chain, w, x0, y0, cv, dfrag);
    return og_adj_tree(p);
}

#endif /* OG_MIX_H */
