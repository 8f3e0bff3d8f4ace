// og_dir.h - exact directional derivatives F'(x) v: the seeded accessor and ONE entry of the result.
//
// The generated header emits every function against `typename X::scalar`, so the very functions that give F and dF/dx
// give the derivative of F along a direction v in the decision vector when variable i carries the seed v[i] on
// first-order dual numbers (og_dual.h): one forward-mode pass, the work of one evaluation - no pattern, no J_T, no
// n x m memory, no step.
//
// Same source for hipcc (csrc/ogk_kernels.hip: ogk_exact_dir, ogk_exact_dir_batch) and for a host compiler
// (tests/dir_probe.cpp), as og_par.h is: an entry is computed by one thread from x0, v, y0, cv and the D operand image
// alone, without a reduction across threads, so neither the mapping nor the compiler's target can change a bit.
//
// Include after og_dual.h and the generated header (with or without run-time parameters).
#ifndef OG_DIR_H
#define OG_DIR_H

#include "og_dual.h"
#include "og_par.h"         // og_par_dfrag: D[k][l] out of the operand image

// x(i) carries the seed v[i].  No member par_seed: in a parameterised header par_leaf resolves to the plain table entry,
// so a run-time parameter is a constant along v.
struct OgDirX {
    typedef ogdual scalar;
    const double* x0;
    const double* v;
    OG_HDI ogdual operator()(const int i) const { return ogdual(x0[i], v[i]); }
    OG_HDI double ldy(const double* p) const { return *p; }      // base collocation product: a value only (og_dir_defect
                                                                 // adds D times the operand's derivative itself)
};

// entries of F'(x) v: every element of every row group, and every (collocation slot, node) of every defect group
template <class G>
OG_HDI int og_dir_entries() {
    int total = 0;
    for (int g = 0; g < G::N_GROUPS; ++g) total += G::G_LEN(g) * (G::G_KIND(g) == 0 ? 1 : G::G_NMV(g));
    return total;
}

// d(operand_l)/dv of collocation slot `slot`: what a defect row's sum runs over
template <class G>
OG_HDI double og_dir_operand(const int slot, const int l, const OgDirX& xd, const double* cv) {
    return G::mv_operand(slot, l, xd, cv).d;
}

// The defect row of node k of slot G_MV0(g) + s of defect group g:
//   d(defect)/dv = sum_l D[k][l] d(operand_l)/dv - d(dynamics term at node k)/dv,
// the sum one fma chain over l ascending from 0.0 (the order of the collocation product itself).  opd(l) is
// d(operand_l)/dv - og_dir_operand, evaluated in place (og_dir_entry) or read back from where the threads of a workgroup
// put the N of them, one each (the kernels): the same doubles into the same chain either way.
// dfrag: the packed operand images of all phases (phase p at G::DFRAG_OFF(p)).
template <class G, class OPD>
OG_HDI double og_dir_defect(const int g, const int s, const int k, const OPD& opd, const OgDirX& xd, const double* cv,
                            const double* dfrag, int* row) {
    const int N = G::G_LEN(g), slot = G::G_MV0(g) + s;
    *row = G::G_ROW(g, s) + k;
    const double* dphase = dfrag + G::DFRAG_OFF(G::G_PHASE(g));
    double dy = 0.0;
    for (int l = 0; l < N; ++l) dy = __builtin_fma(opd(l), og_par_dfrag(dphase, N, k, l), dy);
    return dy - G::tail_one(slot, k, xd, cv).d;
}

// Entry e in [0, og_dir_entries<G>()) of F'(x) v -> its value, *row its row of F; every row of [0, M) belongs to exactly
// one entry.  The groups in index order.  A row group: element by element, the item's derivative.  A defect group: slot
// by slot, node by node, og_dir_defect.
template <class G>
OG_HDI double og_dir_entry(int e, const double* x0, const double* v, const double* y0, const double* cv,
                           const double* dfrag, int* row) {
    const OgDirX xd{x0, v};
    for (int g = 0; g < G::N_GROUPS; ++g) {
        const int N = G::G_LEN(g);
        if (G::G_KIND(g) == 0) {
            if (e < N) return G::item_value(g, 0, e, xd, y0, cv, row).d;
            e -= N;
            continue;
        }
        const int here = N * G::G_NMV(g);
        if (e >= here) {
            e -= here;
            continue;
        }
        const int s = e / N, k = e - s * N, slot = G::G_MV0(g) + s;
        struct InPlace {
            int slot;
            const OgDirX& xd;
            const double* cv;
            OG_HDI double operator()(const int l) const { return og_dir_operand<G>(slot, l, xd, cv); }
        };
        return og_dir_defect<G>(g, s, k, InPlace{slot, xd, cv}, xd, cv, dfrag, row);
    }
    *row = 0;
    return 0.0;
}

#endif /* OG_DIR_H */
