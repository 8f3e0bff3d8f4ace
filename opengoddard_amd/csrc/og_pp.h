// og_pp.h - exact second derivatives of w . F in the run-time parameters, the theta-theta block: the entries of one pair
// of parameters, their terms and the order of their sum.
//
// S_kl = sum_r w_r d2F_r/dtheta_k dtheta_l for weights w over the rows of F = [cost | c_eq | c_ineq] and two declared
// run-time parameters.  With w = [1, lambda] it is d2L/dtheta2; with x held fixed the exact Hessian in theta.
//
// OWNER AND PARTNER.  Of a pair (k, l), k <= l, the OWNER is the parameter with fewer PAR_ENTRIES (a tie: the lower
// index) and the partner the other one; on the diagonal both are the one parameter (og_pp_pair).  The entries of S_kl are
// the entries e in [0, PAR_ENTRIES(owner)) of the owner's work lists in the enumeration order of og_par_entry (og_par.h):
// the row groups first, element by element, then the collocation slots node by node.  A row the owner does not read has
// no second derivative along the owner, so nothing is left out.
//
// EVALUATION.  Every entry is evaluated on second-order dual numbers (og_dual2.h): the unit seed of slot 1 on the owner's
// table entry, the unit seed of slot 2 on the partner's, both on the one leaf on the diagonal - ogdual2(v, 1, 1, 0).
// OgPpX has the members par_seed1 and par_seed2 (and no par_seed), which selects the par_leaf overload of the generated
// header that seeds both slots (codegen._parameter_section); x(i) carries no seed.  A row item's term is its .dd.  A
// collocation entry's term is sum_l' fma(op_l'.dd, D[k][l'], .) ascending from +0.0, only where the slot's reads & 2 (the
// operand reads the owner), minus tail.dd where reads & 1 - the shape of og_par_entry, with the OWNER's reads word.
//
// Slot 1 is the owner's seed, so by rule (a) of og_dual2.h a term's .d1 is og_par_entry of the owner, bit for bit.  Its
// .d2 is og_par_entry of the partner at the same row wherever the partner's work lists hold that row in the same shape:
// always for a row item, for a collocation entry where the partner's reads word of that slot equals the owner's (where
// the owner's word lacks a bit of the partner's, the part of the partner's derivative behind that bit is not evaluated:
// it does not depend on the owner and its mixed part is exactly zero).
//
// The ORDER of the sum is og_adj.h's and is not restated here: OG_ADJ_CHAINS strided chains
// acc = fma(w[row], term, acc) from +0.0 over the entries in ascending order (og_pp_chain), then og_adj_tree.
// Consequences:
//   - the result is reproducible to the bit, whatever the mapping;
//   - weight vector d of K is the call with that vector alone (every vector has chains of its own);
//   - a row with w_r == 0 is NOT skipped (0 * inf is NaN, as the product would give);
//   - an entry of the owner's list that does not read the partner contributes an exact +0.0: rule (b) of og_dual2.h, no
//     0 * inf;
//   - a parameter nothing reads owns every pair it is in (its list is empty): its row and column are +0.0 with no work;
//   - S[l][k] is a copy of S[k][l]: the matrix is symmetric by construction.
//
// Same source for hipcc (csrc/ogk_kernels.hip: ogk_exact_pp, ogk_exact_pp_batch) and a host compiler
// (tests/pp_probe.cpp).  Include after og_dual2.h and the generated header (a header with N_PAR > 0: OG_GEN_HAS_PAR).
#ifndef OG_PP_H
#define OG_PP_H

#include "og_dual2.h"
#include "og_adj.h"         // OG_ADJ_CHAINS, og_adj_tree; og_par_dfrag through it

// x(i) carries no seed; the parameter at table index par_seed1 carries the unit seed of slot 1, the one at par_seed2 that
// of slot 2 (the same index: both seeds on the one leaf)
struct OgPpX {
    typedef ogdual2 scalar;
    const double* x0;
    int par_seed1, par_seed2;
    OG_HDI ogdual2 operator()(const int i) const { return ogdual2(x0[i]); }
    OG_HDI double ldy(const double* p) const { return *p; }      // base collocation product: a value only, as in og_par.h
};

// Pair `pair` in [0, N_PAR (N_PAR + 1) / 2): (k, l) with k <= l in row-major order of the upper triangle, its owner, its
// partner and the number of its entries
struct OgPpPair {
    int k, l, owner, partner, entries;
};

template <class G>
OG_HDI OgPpPair og_pp_pair(const int pair) {
    OgPpPair p;
    int k = 0, first = 0;                           // first: the index of pair (k, k)
    while (pair >= first + (G::N_PAR - k)) {
        first += G::N_PAR - k;
        ++k;
    }
    p.k = k;
    p.l = k + (pair - first);
    const int ek = G::PAR_ENTRIES(p.k), el = G::PAR_ENTRIES(p.l);
    p.owner = el < ek ? p.l : p.k;
    p.partner = el < ek ? p.k : p.l;
    p.entries = el < ek ? el : ek;
    return p;
}

// One entry: dd the term of S_kl, d1 the part along the owner (og_par_entry of the owner, bit for bit), d2 the part along
// the partner
struct OgPpTerm {
    double dd, d1, d2;
};

// Entry e in [0, G::PAR_ENTRIES(owner)) of the owner's work lists, *row its row of F
template <class G>
OG_HDI OgPpTerm og_pp_term(const int owner, const int partner, int e, const double* x0, const double* y0,
                           const double* cv, const double* dfrag, int* row) {
    const OgPpX xd{x0, G::PAR_OFF + owner, G::PAR_OFF + partner};
    for (int i = G::PAR_ROW_PTR(owner); i < G::PAR_ROW_PTR(owner + 1); ++i) {
        const int g = G::PAR_ROW_G(i), len = G::G_LEN(g);
        if (e < len) {
            const ogdual2 v = G::item_value(g, 0, e, xd, y0, cv, row);
            return OgPpTerm{v.dd, v.d1, v.d2};
        }
        e -= len;
    }
    for (int i = G::PAR_SLOT_PTR(owner); i < G::PAR_SLOT_PTR(owner + 1); ++i) {
        const int g = G::PAR_SLOT_G(i), N = G::G_LEN(g);
        if (e >= N) {
            e -= N;
            continue;
        }
        const int slot = G::PAR_SLOT(i), reads = G::PAR_SLOT_READS(i), k = e;
        *row = G::G_ROW(g, slot - G::G_MV0(g)) + k;
        OgPpTerm dy{0.0, 0.0, 0.0};
        if (reads & 2) {
            const double* dphase = dfrag + G::DFRAG_OFF(G::G_PHASE(g));
            for (int l = 0; l < N; ++l) {
                const ogdual2 op = G::mv_operand(slot, l, xd, cv);
                const double D = og_par_dfrag(dphase, N, k, l);
                dy = OgPpTerm{__builtin_fma(op.dd, D, dy.dd), __builtin_fma(op.d1, D, dy.d1), __builtin_fma(op.d2, D, dy.d2)};
            }
        }
        OgPpTerm dt{0.0, 0.0, 0.0};
        if (reads & 1) {
            const ogdual2 tail = G::tail_one(slot, k, xd, cv);
            dt = OgPpTerm{tail.dd, tail.d1, tail.d2};
        }
        return OgPpTerm{dy.dd - dt.dd, dy.d1 - dt.d1, dy.d2 - dt.d2};
    }
    *row = 0;
    return OgPpTerm{0.0, 0.0, 0.0};
}

// Partial sum `chain` in [0, OG_ADJ_CHAINS) of the pair p against the weight vector w[M]
template <class G>
OG_HDI double og_pp_chain(const OgPpPair& p, const int chain, const double* w, const double* x0, const double* y0,
                          const double* cv, const double* dfrag) {
    double acc = 0.0;
    for (int e = chain; e < p.entries; e += OG_ADJ_CHAINS) {
        int row;
        const double t = og_pp_term<G>(p.owner, p.partner, e, x0, y0, cv, dfrag, &row).dd;
        acc = __builtin_fma(w[row], t, acc);
    }
    return acc;
}

// S_kl of pair `pair`: the definition
template <class G>
OG_HDI double og_pp_entry(const int pair, const double* w, const double* x0, const double* y0, const double* cv,
                          const double* dfrag) {
    const OgPpPair p = og_pp_pair<G>(pair);
    double part[OG_ADJ_CHAINS];
    for (int chain = 0; chain < OG_ADJ_CHAINS; ++chain) part[chain] = og_pp_chain<G>(p, chain, w, x0, y0, cv, dfrag);
    return og_adj_tree(part);
}

#endif /* OG_PP_H */
