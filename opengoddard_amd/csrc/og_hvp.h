// og_hvp.h - exact Hessian-vector products of w.F: q = grad^2 (w . F)(x) v, the terms of one entry and the order of
// their sum.
//
// q_j = sum_r w_r d2F_r/dx_j dv for weights w over the rows of F = [cost | c_eq | c_ineq] and a direction v in the
// decision vector.  The terms of q_j are the terms og_adj.h enumerates for column j of the exact Jacobian - the row
// items, then the column's own collocation block - each evaluated on second-order dual numbers (og_dual2.h) with the unit
// seed on x_j in one slot and v in the other; the term's value is the mixed part.  Where og_adj_term has
// D[k][l] d(operand_l)/dx_j, the term here has D[k][l] d2(operand_l)/dx_j dv.  (codegen emits an operand as an
// expression like any other (codegen.operand_function) and promises nowhere that it is affine in x, so the term is
// kept; for an affine operand it is +0.0.)  y0, the base collocation product,
// enters as a value only (ldy).  Run-time parameters are constants: OgHvpX has no member par_seed.
//
// The ORDER of the sum is og_adj.h's and is not restated here: OG_ADJ_CHAINS strided chains
// acc = fma(w[row], term, acc) from +0.0 (og_hvp_chain walks the terms as og_adj_chain does), then og_adj_tree.  The
// consequences are the adjoint's: reproducible to the bit; pair d of K is the call with that pair alone; w_r = 0 is not
// skipped; a variable nothing reads gets +0.0.
//
// Same source for hipcc (csrc/ogk_kernels.hip: ogk_exact_hvp, ogk_exact_hvp_batch) and a host compiler
// (tests/hvp_probe.cpp).  Include after the generated header.
#ifndef OG_HVP_H
#define OG_HVP_H

#include "og_dual2.h"
#include "og_adj.h"         // og_adj_col, OG_ADJ_CHAINS, og_adj_tree; og_par_dfrag through it

// x(i) with the unit seed on x_j in slot 1 and v[i] in slot 2
struct OgHvpX {
    typedef ogdual2 scalar;
    const double* x0;
    int j;
    const double* v;
    OG_HDI ogdual2 operator()(const int i) const { return ogdual2(x0[i], i == j ? 1.0 : 0.0, v[i], 0.0); }
    OG_HDI double ldy(const double* p) const { return *p; }
};

// Term t in [0, c.terms) of column j (c = og_adj_col(j)), *row its row of F: .d is dF_row/dx_j - bit for bit og_adj_term,
// by rule (a) of og_dual2.h - and .v is the mixed part d2F_row/dx_j dv, the term of q_j.
template <class G, class T>
OG_HDI ogdual og_hvp_term(const T& tab, const OgAdjCol& c, const int j, const int t, const double* x0, const double* v,
                          const double* y0, const double* cv, const double* dfrag, int* row) {
    const OgHvpX xd{x0, j, v};
    if (t < c.items) {
        const auto it = tab.elem(c.e0 + t);
        const ogdual2 e = G::item_value(it.x, it.y, it.z, xd, y0, cv, row);
        return ogdual(e.dd, e.d1);
    }
    const int k = t - c.items;
    *row = c.row0 + k;
    const double D = og_par_dfrag(dfrag + G::DFRAG_OFF(c.phase), c.N, k, c.l);
    const ogdual2 op = G::mv_operand(c.slot, c.l, xd, cv);
    ogdual e(__builtin_fma(op.dd, D, 0.0), __builtin_fma(op.d1, D, 0.0));
    if ((c.reads & 2) || ((c.reads & 1) && k == c.l)) {
        const ogdual2 tail = G::tail_one(c.slot, k, xd, cv);
        e = ogdual(e.v - tail.dd, e.d - tail.d1);
    }
    return e;
}

// Partial sum `chain` in [0, OG_ADJ_CHAINS) of column j for the pair (w[M], v[N_VAR])
template <class G, class T>
OG_HDI double og_hvp_chain(const T& tab, const OgAdjCol& c, const int j, const int chain, const double* w,
                           const double* v, const double* x0, const double* y0, const double* cv, const double* dfrag) {
    double acc = 0.0;
    for (int t = chain; t < c.terms; t += OG_ADJ_CHAINS) {
        int row;
        const double e = og_hvp_term<G>(tab, c, j, t, x0, v, y0, cv, dfrag, &row).v;
        acc = __builtin_fma(w[row], e, acc);
    }
    return acc;
}

// q_j of grad^2 (w . F)(x) v: the definition
template <class G, class T>
OG_HDI double og_hvp_entry(const T& tab, const int j, const double* w, const double* v, const double* x0,
                           const double* y0, const double* cv, const double* dfrag) {
    const OgAdjCol c = og_adj_col<G>(tab, j, x0, cv);
    double p[OG_ADJ_CHAINS];
    for (int chain = 0; chain < OG_ADJ_CHAINS; ++chain)
        p[chain] = og_hvp_chain<G>(tab, c, j, chain, w, v, x0, y0, cv, dfrag);
    return og_adj_tree(p);
}

#endif /* OG_HVP_H */
