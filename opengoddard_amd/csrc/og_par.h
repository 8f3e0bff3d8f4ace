// og_par.h - exact dF/dtheta for run-time parameters: the seeded accessor and ONE entry of the result.
//
// The generated header reads a parameter leaf through OgGen::par_leaf (codegen._parameter_section): for an accessor
// with a member `par_seed` that is the table entry with a unit derivative where its index is the seed, so the very
// functions that give F and dF/dx give dF/dtheta_k on first-order dual numbers (og_dual.h) - no step, no FD noise.
//
// Same source for hipcc (csrc/ogk_kernels.hip: ogk_exact_par, ogk_exact_par_batch) and for a host compiler
// (tests/par_exact_probe.cpp), as og_lgl.h is: an entry is computed by one thread from x0, y0, cv and the D operand
// image alone, without a reduction across threads, so neither the mapping nor the compiler's target can change a bit.
//
// Include after og_dual.h and the generated header (a header with N_PAR > 0: OG_GEN_HAS_PAR).
#ifndef OG_PAR_H
#define OG_PAR_H

#include "og_dual.h"

// x(i) carries no derivative; the parameter at table index par_seed (PAR_OFF + k) carries the unit seed
struct OgParX {
    typedef ogdual scalar;
    const double* x0;
    int par_seed;
    OG_HDI ogdual operator()(const int i) const { return ogdual(x0[i], 0.0); }
    OG_HDI double ldy(const double* p) const { return *p; }      // base collocation product: no parameter reaches D x~
                                                                 // except through the operand (og_par_entry adds that)
};

// D[k][l] of a phase with N nodes out of its MFMA operand image (ogk.h: ogk_frag_pack)
OG_HDI double og_par_dfrag(const double* dfrag_phase, const int N, const int k, const int l) {
    const int KS = (N + 3) >> 2;
    return dfrag_phase[((long)(k >> 4) * KS + (l >> 2)) * 64 + (((l & 3) << 4) | (k & 15))];
}

// Entry e in [0, G::PAR_ENTRIES(kp)) of dF/dtheta_kp -> its value, *row its row of F.  The row groups that read the
// parameter come first, element by element: the item's derivative.  Then the collocation slots, node by node:
//   d(defect)/dtheta = sum_l D[k][l] d(operand_l)/dtheta - d(dynamics term at node k)/dtheta,
// the sum one fma chain over l ascending from 0.0 (the order of the collocation product itself) and only for a slot
// whose operand reads the parameter (a state's unit that is a parameter); the dynamics term only where it reads it.
// dfrag: the packed operand images of all phases (phase p at G::DFRAG_OFF(p)).
template <class G>
OG_HDI double og_par_entry(const int kp, int e, const double* x0, const double* y0, const double* cv,
                           const double* dfrag, int* row) {
    const OgParX xd{x0, G::PAR_OFF + kp};
    for (int i = G::PAR_ROW_PTR(kp); i < G::PAR_ROW_PTR(kp + 1); ++i) {
        const int g = G::PAR_ROW_G(i), len = G::G_LEN(g);
        if (e < len) return G::item_value(g, 0, e, xd, y0, cv, row).d;
        e -= len;
    }
    for (int i = G::PAR_SLOT_PTR(kp); i < G::PAR_SLOT_PTR(kp + 1); ++i) {
        const int g = G::PAR_SLOT_G(i), N = G::G_LEN(g);
        if (e >= N) {
            e -= N;
            continue;
        }
        const int slot = G::PAR_SLOT(i), reads = G::PAR_SLOT_READS(i), k = e;
        *row = G::G_ROW(g, slot - G::G_MV0(g)) + k;
        double dy = 0.0;
        if (reads & 2) {
            const double* dphase = dfrag + G::DFRAG_OFF(G::G_PHASE(g));
            for (int l = 0; l < N; ++l)
                dy = __builtin_fma(G::mv_operand(slot, l, xd, cv).d, og_par_dfrag(dphase, N, k, l), dy);
        }
        const double dt = (reads & 1) ? G::tail_one(slot, k, xd, cv).d : 0.0;
        return dy - dt;
    }
    *row = 0;
    return 0.0;
}

#endif /* OG_PAR_H */
