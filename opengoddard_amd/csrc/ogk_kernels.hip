// ogk_kernels.hip -- hand-written gfx950 sweep kernels, instantiated for one traced problem.
//
// Compiled once per problem as  hipcc --offload-arch=gfx950 -ffp-contract=off -DOG_GEN_HEADER=...
// The generated header only supplies pointwise device functions (OgGen::group_eval,
// OgGen::defect_tail, OgGen::mv_operand) and small index tables; everything about parallel
// decomposition, LDS, MFMA and memory traffic is in this file.
//
// What the kernels replace:
//   a7  solve.equality_add     OpenGoddard/optimize.py:670-698   collocation defects + user rows
//   a10 solve.cost_add         OpenGoddard/optimize.py:700-709
//   a14 _dense_difference      scipy/optimize/_numdiff.py:584-625 forward-difference column loop
//
// Forward-difference column j evaluates F at x0 + h_j e_j.  The stack of n perturbed vectors
// ((n+1) x n doubles in the reference's formulation) is never materialised: every read of the
// decision vector goes through XCol, which returns x0[i] except at i == j.
//
// Launch modes (ogk_launch; ogk.h: enum ogk_mode lists all):
//   OGK_EVAL (0)   ogk_eval   F(x0) -> f0, plus scratch the two-launch sweep reuses: the unperturbed collocation
//                        products y0, the dynamics terms t0 = (tf-t0)/2 f, and z = F0 - F0
//                        (0, or NaN where a row is not finite: what dense FD would produce).
//   OGK_SWEEP (1)  ogk_sweep  structured forward-difference sweep, second of two launches.  Dense FD evaluates
//                        every row for every column although a row changes only when it reads
//                        the perturbed variable; because base and perturbed values come from
//                        the same device functions, every other difference quotient is exactly
//                        (F0-F0)/dx.  This kernel therefore
//                          - lets a workgroup own a few J_T rows (= FD columns): it streams
//                            zeros into them (unless the buffer is a registered persistent-zero one) and
//                            re-evaluates only the (group, output, element)
//                            items whose traced leaves include p[j] (tables OGT_COL/OGT_ELEM);
//                          - runs the collocation product for the N perturbed vectors of each
//                            state slice on v_mfma_f64_16x16x4_f64 (A = 16 perturbed state
//                            vectors, B = the D^T operand image), writing the dense N x N
//                            block d(defect_s)/d(state_s) directly.
//   OGK_FUSED (5)  ogk_fused  OGK_EVAL + OGK_SWEEP as ONE launch writing only the non-zeros (the default; see
//                        below).  The results of OGK_SWEEP, OGK_FUSED and OGK_DENSE are identical (tests compare
//                        them and the CPU twin).
//
// D is kept in HBM/L2 in MFMA B-operand order (ogk.h).  Kernels that reuse a panel across
// wavefronts or states stage it in LDS; the MFMA tiles use each panel once
// per wavefront and read it straight from L2 (measured: no LDS round trip, no barrier, same speed).
//   OGK_DENSE (2)  ogk_dense  the literal dense sweep: all rows for all columns (validation, and the
//                        shape SURVEY.md section 7.2 describes).
//
// The MFMA accumulation is a k-ordered fma chain per output (verified on hardware by
// tools/gpu_probe.hip), identical to oracle/twin.cpp's loop.
#include <hip/hip_runtime.h>
#include "ogk.h"
#include "og_dual.h"
#if defined(OGK_PART) && (OGK_PART == OGK_PART_HVP || OGK_PART == OGK_PART_MIX || OGK_PART == OGK_PART_HESS || \
                          OGK_PART == OGK_PART_PP)
#include "og_dual2.h"       // (ahead of the generated header, whose functions name ogm:: at their definition)
#endif
#include OG_GEN_HEADER

typedef double v4f64 __attribute__((ext_vector_type(4)));

// Timing experiments only (tools/kstats.sh): -DOGK_EXP=<mask> removes pieces of ogk_sweep so that
// rocprof durations attribute time to phases: 8 = no item evaluation, 16 = no fill, 32 = no MFMA
// tiles.  Results are wrong with any bit set.
#ifndef OGK_EXP
#define OGK_EXP 0
#endif

// -DOGK_TRACE=1 (tools/trace_sweep.py): workgroups overwrite the start of one of their J_T rows
// with shader-clock stamps of their phases; results are garbage, timing is the point.
#ifndef OGK_TRACE
#define OGK_TRACE 0
#endif

namespace {

struct XCol {
    typedef double scalar;
    const double* x0;
    int j;          // perturbed index, -1 for none
    double xj;      // x0[j] + h[j]
    __device__ __forceinline__ double operator()(const int i) const {
        const double v = x0[i];
        return i == j ? xj : v;
    }
    // base collocation product y0[slot offset + node]: from the scratch an evaluation left in memory
    __device__ __forceinline__ double ldy(const double* p) const { return *p; }
};

// the same, for a workgroup of the fused launch that keeps the base products of its node tile in LDS
// (an LDS read must not be a flat load through the y0 pointer: a flat load waits for every outstanding
// store of the wavefront, i.e. for the fill that is supposed to drain underneath the item chains)
struct XColL {
    typedef double scalar;
    const double* x0;
    int j;
    double xj;
    const double* y0_first;     // &y0[offset of the group's first slot]
    const double* yl;           // LDS: [state][N]
    __device__ __forceinline__ double operator()(const int i) const {
        const double v = x0[i];
        return i == j ? xj : v;
    }
    __device__ __forceinline__ double ldy(const double* p) const { return yl[(int)(p - y0_first)]; }
};

// XCol with the base terms of the program's sequential sums (a running cost summed node by node like Python's
// sum()) at hand: the workgroup computed them once, cooperatively, into LDS; a lane re-evaluates only the term
// that reads its own perturbed variable.  The additions stay with the caller, in order - same bits, but a
// chain of LDS reads and adds instead of N evaluations with their global loads per lane.
constexpr int TB_SLOTS = OgGen::N_TBLK > 0 ? OgGen::N_TBLK : 1;
struct XColT {
    typedef double scalar;
    const double* x0;
    int j;
    double xj;
    const double* tc;           // [N_TERMS] base terms in LDS, or NULL: evaluate in place
    int qd[TB_SLOTS];           // per term block: the term that reads p[j] (-1 none, -2 several: in place)
    double td[TB_SLOTS];        // ... and its value at x0 + h e_j
    __device__ __forceinline__ double operator()(const int i) const {
        const double v = x0[i];
        return i == j ? xj : v;
    }
    __device__ __forceinline__ double ldy(const double* p) const { return *p; }
    __device__ __forceinline__ const double* term_cache(const int tb) const {
        return (tc && qd[tb] != -2) ? tc + OgGen::TERM_OFF(tb) : nullptr;
    }
    __device__ __forceinline__ int term_q(const int tb) const { return qd[tb]; }
    __device__ __forceinline__ double term_v(const int tb) const { return td[tb]; }
};
__device__ __forceinline__ XColT make_xcolt(const ogk_args& a, const int j, const double xj, const double* tc) {
    XColT x;
    x.x0 = a.x0, x.j = j, x.xj = xj, x.tc = tc;
    const XCol plain{a.x0, j, xj};
#pragma unroll
    for (int tb = 0; tb < TB_SLOTS; ++tb) {
        x.qd[tb] = -1, x.td[tb] = 0.0;
        if (tc && tb < OgGen::N_TBLK && j >= 0) {
            x.qd[tb] = OgGen::sum_term_q(tb, j);
            if (x.qd[tb] >= 0) x.td[tb] = OgGen::sum_term(tb, x.qd[tb], plain, a.cvec);
        }
    }
    return x;
}
constexpr bool TERM_CACHE = OgGen::N_TERMS > 0 && OgGen::N_TERMS <= 2048;      // LDS doubles a workgroup spends on it
constexpr int TERM_DOUBLES = TERM_CACHE ? OgGen::N_TERMS + 16 : 0;     // (+16: the generated sum loops read whole groups of eight, one group ahead)

// all threads of a workgroup: the base terms into LDS (the caller's barrier publishes them)
template <int THREADS>
__device__ __forceinline__ void fill_terms(const ogk_args& a, double* tc) {
    struct XBase {
        typedef double scalar;
        const double* x0;
        __device__ __forceinline__ double operator()(const int i) const { return x0[i]; }
    };
    const XBase xb{a.x0};
#pragma unroll
    for (int tb = 0; tb < OgGen::N_TBLK; ++tb)
        for (int q = (int)threadIdx.x; q < OgGen::TERM_LEN(tb); q += THREADS)
            tc[OgGen::TERM_OFF(tb) + q] = OgGen::sum_term(tb, q, xb, a.cvec);
}

// Persistent-zero output (ogk.h: jt_sparse / jt_launches / jt_state).  A buffer that is known to hold zeros at
// its structural zeros is only written where something can be non-zero; the fill is needed when the
// buffer is not registered, or when the previous launch into it left a NaN fill behind.
__device__ __forceinline__ bool jt_needs_fill(const ogk_args& a) {
    // both written by earlier kernels (agent scope): plain loads.  *jt_launches already counts this launch
    const unsigned st = *a.jt_state, gen = *a.jt_launches;
    return !a.jt_sparse | (st == gen - 1u);
}
// this launch fills with NaN: the next launch into the buffer must clean up
__device__ __forceinline__ void jt_mark_nan_fill(const ogk_args& a) {
    if (a.jt_sparse) __hip_atomic_store(a.jt_state, *a.jt_launches, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

constexpr int ROWS_COLS_PER_THREAD = 8;

__device__ __forceinline__ int defect_block_to_group(int bx, int* nt_out) {
    for (int g = 0; g < OgGen::N_GROUPS; ++g) {
        if (OgGen::G_KIND(g) != 1) continue;
        const int ntiles = (OgGen::G_LEN(g) + 15) >> 4;
        if (bx < ntiles) { *nt_out = bx; return g; }
        bx -= ntiles;
    }
    *nt_out = 0;
    return -1;
}

// The module may be built in parts (-DOGK_PART=<OGK_PART_*>, ogk.h; build.py): OGK_PART_MAIN, OGK_PART_FUSED and
// OGK_PART_SWEEP hold what a solve needs from its first sweep on (evaluation, pattern / pack / unpack; the one-launch
// sweep; the structured sweep), OGK_PART_AUX the validation sweep and the exact-Jacobian kernels.  Each part
// instantiates the generated callbacks only for its own kernels, and the parts compile side by side: the first solve
// of a new problem shape waits for the slowest of them only.
#if !defined(OGK_PART) || OGK_PART == OGK_PART_AUX
#define OGK_HAS_AUX 1        // OGK_DENSE, OGK_EXACT_DENSE, OGK_EXACT: validation sweep, exact Jacobian
#endif
#if !defined(OGK_PART) || OGK_PART == OGK_PART_MAIN
#define OGK_HAS_MAIN 1       // OGK_EVAL, OGK_PATTERN_COUNT ... OGK_COUNT_LAUNCH: evaluation, pattern, pack, unpack
#endif
#if !defined(OGK_PART) || OGK_PART == OGK_PART_FUSED
#define OGK_HAS_FUSED 1      // OGK_FUSED: evaluation + structured sweep in one launch
#endif
#if !defined(OGK_PART) || OGK_PART == OGK_PART_SWEEP
#define OGK_HAS_SWEEP 1      // OGK_SWEEP: the structured sweep as a launch of its own
#endif
#if defined(OGK_PART) && OGK_PART == OGK_PART_BATCH
#define OGK_HAS_BATCH 1      // OGK_BATCH_FUSED, OGK_BATCH_EVAL, OGK_BATCH_BIND; never part of a module's default build
#endif
#if defined(OGK_PART) && OGK_PART == OGK_PART_BATCH_EXACT
#define OGK_HAS_BATCH_EXACT 1    // OGK_BATCH_EXACT: the exact Jacobian of a batch of points; built on demand
#endif
#if defined(OGK_PART) && OGK_PART == OGK_PART_PAR
#define OGK_HAS_PAR 1        // OGK_PAR_JAC, OGK_BATCH_PAR_JAC: exact dF/dtheta for run-time parameters; built on demand
#endif
#if defined(OGK_PART) && OGK_PART == OGK_PART_DIR
#define OGK_HAS_DIR 1        // OGK_DIR, OGK_BATCH_DIR: exact directional derivatives F'(x) v; built on demand
#endif
#if defined(OGK_PART) && OGK_PART == OGK_PART_ADJ
#define OGK_HAS_ADJ 1        // OGK_ADJ, OGK_BATCH_ADJ: exact adjoint products F'(x)^T w; built on demand
#endif
#if defined(OGK_PART) && OGK_PART == OGK_PART_HVP
#define OGK_HAS_HVP 1        // OGK_HVP, OGK_BATCH_HVP: exact Hessian-vector products of w . F; built on demand
#endif
#if defined(OGK_PART) && OGK_PART == OGK_PART_MIX
#define OGK_HAS_MIX 1        // OGK_MIX, OGK_BATCH_MIX: exact mixed derivatives d(F'(x)^T w)/dtheta; built on demand
#endif
#if defined(OGK_PART) && OGK_PART == OGK_PART_HESS
#define OGK_HAS_HESS 1       // OGK_HESS, OGK_BATCH_HESS: the exact sparse Hessian of w . F; built on demand
#endif
#if defined(OGK_PART) && OGK_PART == OGK_PART_PP
#define OGK_HAS_PP 1         // OGK_PP, OGK_BATCH_PP: exact second derivatives of w . F in the parameters; built on demand
#endif
// (the split is at the kernels: a __global__ function is what costs code generation; the device functions below
// them are templates or forced-inline and cost nothing where no kernel of the part uses them)
// ------------------------------------------------------------------------------------------
// Mode 2, dense sweep (validation): collocation workgroup = (phase, 16-node tile, 64 FD
// columns), all states; row workgroup = one thread per (row item, 8 columns).
// ------------------------------------------------------------------------------------------
__device__ __forceinline__ void dense_defect_body(const ogk_args& a, const int bx, const int by,
                                                  double* lds) {
    int nt;
    const int g = defect_block_to_group(bx, &nt);
    if (g < 0) return;
    const int N = OgGen::G_LEN(g);
    const int KS = (N + 3) >> 2;
    const int NP = KS * 4;
    const int phase = OgGen::G_PHASE(g);
    const int mv0 = OgGen::G_MV0(g);
    const int nmv = OgGen::G_NMV(g);
    const int tid = (int)threadIdx.x;

    double* dpanel = lds;
    double* xt = lds + KS * 64;
    const double* src = a.dfrag + a.dfrag_off[phase] + (long)nt * KS * 64;
    for (int i = tid; i < KS * 64; i += 256) dpanel[i] = src[i];
    const XCol base{a.x0, -1, 0.0};
    {
        const int wave_ = tid >> 6, lane_ = tid & 63;
        for (int s = wave_; s < OgGen::MAX_NMV; s += 4)
            for (int l = lane_; l < NP; l += 64)
                xt[s * NP + l] = (s < nmv && l < N) ? OgGen::mv_operand(mv0 + s, l, base, a.cvec) : 0.0;
    }
    __syncthreads();

    const int wave = tid >> 6, lane = tid & 63;
    const int c0 = a.col_lo + (by * 4 + wave) * 16;
    if (c0 >= a.col_hi) return;
    const int lk = lane >> 4;
    const int k = nt * 16 + (lane & 15);

    // the column this lane feeds into the A operand, and the one operand entry it changes
    int hit_s = -1, hit_l = -1;
    double hit_v = 0.0;
    {
        const int ja = c0 + (lane & 15);
        if (ja < a.col_hi) {
            for (int s = 0; s < nmv; ++s) {
                const int leaf = OgGen::MV_LEAF(mv0 + s);
                if (ja >= leaf && ja < leaf + N) {
                    hit_s = s;
                    hit_l = ja - leaf;
                    const XCol xa{a.x0, ja, a.x0[ja] + a.h[ja]};
                    hit_v = OgGen::mv_operand(mv0 + s, hit_l, xa, a.cvec);
                }
            }
        }
    }

    // batched D.X on the matrix cores: acc[s] (16 columns x 16 nodes) += A_s (16x4) * B (4x16)
    // (branch-free over MAX_NMV: unused slots multiply zeros)
    v4f64 acc[OgGen::MAX_NMV];
#pragma unroll
    for (int s = 0; s < OgGen::MAX_NMV; ++s) acc[s] = (v4f64){0.0, 0.0, 0.0, 0.0};
    for (int ks = 0; ks < KS; ++ks) {
        const double b = dpanel[ks * 64 + lane];
        const int l = ks * 4 + lk;
#pragma unroll
        for (int s = 0; s < OgGen::MAX_NMV; ++s) {
            double av = xt[s * NP + l];
            av = (s == hit_s && l == hit_l) ? hit_v : av;
            acc[s] = __builtin_amdgcn_mfma_f64_16x16x4f64(av, b, acc[s], 0, 0, 0);
        }
    }

    // epilogue.  C/D layout of the f64 MFMA: column (node) = lane & 15,
    // row (FD column) = (lane >> 4) + 4 * reg.
    if (k >= N) return;
    double y[OgGen::MAX_NMV];
    double T[OgGen::MAX_NMV];
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) {
        const int j = c0 + lk + 4 * reg;
        if (j >= a.col_hi) continue;
        const double xb = a.x0[j];
        const double xj = xb + a.h[j];
        const double dx = xj - xb;
#pragma unroll
        for (int s = 0; s < OgGen::MAX_NMV; ++s) y[s] = acc[s][reg];
        const XCol xa{a.x0, j, xj};
        OgGen::defect_tail(g, k, xa, a.cvec, T);
#pragma unroll
        for (int s = 0; s < OgGen::MAX_NMV; ++s) {     // static index: keeps y/T in registers
            if (s >= nmv) break;
            const int row = OgGen::G_ROW(g, s) + k;
            const double val = y[s] - T[s];
            a.jt[(long)(j - a.col_lo) * OgGen::M + row] = (val - a.f0[row]) / dx;
        }
    }
}

__device__ __forceinline__ void dense_rows_body(const ogk_args& a, const int bx, const int by) {
    const int ri = bx * 256 + (int)threadIdx.x;
    if (ri >= OgGen::N_ROW_ITEMS) return;
    int g = 0;
    for (; g < OgGen::N_GROUPS; ++g) {
        if (OgGen::G_KIND(g) != 0) continue;
        const int i0 = OgGen::G_ITEM0(g);
        if (ri >= i0 && ri < i0 + OgGen::G_LEN(g)) break;
    }
    if (g >= OgGen::N_GROUPS) return;
    const int k = ri - OgGen::G_ITEM0(g);
    const int nout = OgGen::G_NOUT(g);
    double out[OgGen::MAX_OUT];
    const int j0 = a.col_lo + by * ROWS_COLS_PER_THREAD;
    for (int c = 0; c < ROWS_COLS_PER_THREAD; ++c) {
        const int j = j0 + c;
        if (j >= a.col_hi) break;
        const double xb = a.x0[j];
        const double xj = xb + a.h[j];
        const double dx = xj - xb;
        const XCol xa{a.x0, j, xj};
        OgGen::group_eval(g, k, xa, nullptr, a.cvec, out);
        double* jrow = a.jt + (long)(j - a.col_lo) * OgGen::M;
#pragma unroll
        for (int o = 0; o < OgGen::MAX_OUT; ++o) {
            if (o >= nout) break;
            const int row = OgGen::G_ROW(g, o) + k;
            jrow[row] = (out[o] - a.f0[row]) / dx;
        }
    }
}

#ifdef OGK_HAS_AUX
__global__ __launch_bounds__(256) void ogk_dense(const ogk_args a, const int ndef,
                                                 const int defect_total, const int row_blocks) {
    extern __shared__ __attribute__((aligned(16))) double lds[];
    const int id = (int)blockIdx.x;
    // every entry is written: a registered buffer only has to learn about a NaN fill
    if (id == 0 && threadIdx.x == 0 && *a.nonfinite != 0) jt_mark_nan_fill(a);
    if (id < defect_total) {
        dense_defect_body(a, id % ndef, id / ndef, lds);
    } else {
        const int rid = id - defect_total;
        dense_rows_body(a, rid % row_blocks, rid / row_blocks);
    }
}
#endif

// ------------------------------------------------------------------------------------------
// Mode 3, exact Jacobian: the generated callback code instantiated on
// first-order dual numbers (og_dual.h) with a unit seed on decision variable j gives dF/dx_j without
// a step, a subtraction or FD noise.  One thread per (column j, row item): a row-group element, or a
// collocation node of a defect group, where the derivative of the product D.x~ is one column of D
// times the derivative of the operand the seeded variable feeds (if it is a state of that phase).
// F(x0) and the base products come from mode 0 (same stream, before).  Dense and simple: exactness
// changes the numbers SLSQP sees (it removes the 1e-8 noise of the reference's differences), so this
// is an opt-in mode next to the reference-faithful sweep, not a replacement for it.
struct XDual {
    typedef ogdual scalar;
    const double* x0;
    int j;
    __device__ __forceinline__ ogdual operator()(const int i) const { return ogdual(x0[i], i == j ? 1.0 : 0.0); }
    __device__ __forceinline__ double ldy(const double* p) const { return *p; }
};

__device__ __forceinline__ double dfrag_entry(const ogk_args& a, const int phase, const int N, const int k,
                                              const int l) {
    const int KS = (N + 3) >> 2;
    return a.dfrag[a.dfrag_off[phase] + ((long)(k >> 4) * KS + (l >> 2)) * 64 + (((l & 3) << 4) | (k & 15))];
}

#ifdef OGK_HAS_AUX
__global__ __launch_bounds__(256) void ogk_exact(const ogk_args a, const int n_items) {
    const int item = (int)(blockIdx.x * 256 + threadIdx.x);
    const int j = a.col_lo + (int)blockIdx.y;
    if (item >= n_items || j >= a.col_hi) return;
    // item -> (group, element): row-group items first (G_ITEM0 order), then the defect nodes
    int g = 0, k = -1;
    if (item < OgGen::N_ROW_ITEMS) {
        for (; g < OgGen::N_GROUPS; ++g) {
            if (OgGen::G_KIND(g) != 0) continue;
            const int i0 = OgGen::G_ITEM0(g);
            if (item >= i0 && item < i0 + OgGen::G_LEN(g)) {
                k = item - i0;
                break;
            }
        }
    } else {
        int rest = item - OgGen::N_ROW_ITEMS;
        for (; g < OgGen::N_GROUPS; ++g) {
            if (OgGen::G_KIND(g) != 1) continue;
            if (rest < OgGen::G_LEN(g)) {
                k = rest;
                break;
            }
            rest -= OgGen::G_LEN(g);
        }
    }
    if (k < 0) return;
    const XDual xd{a.x0, j};
    double* jrow = a.jt + (long)(j - a.col_lo) * OgGen::M;
    ogdual out[OgGen::MAX_OUT > OgGen::MAX_NMV ? OgGen::MAX_OUT : OgGen::MAX_NMV];
    const int nout = OgGen::G_NOUT(g);
    if (OgGen::G_KIND(g) == 0) {
        OgGen::group_eval(g, k, xd, (const ogdual*)nullptr, a.cvec, out);
    } else {
        const int N = OgGen::G_LEN(g), phase = OgGen::G_PHASE(g), mv0 = OgGen::G_MV0(g), nmv = OgGen::G_NMV(g);
        ogdual y[OgGen::MAX_NMV];
#pragma unroll
        for (int s = 0; s < OgGen::MAX_NMV; ++s) {
            y[s] = ogdual(0.0);
            if (s < nmv) {
                double dy = 0.0;
                const int leaf = OgGen::MV_LEAF(mv0 + s);
                if (j >= leaf && j < leaf + N) {        // x_j is node l of the state behind this product
                    const int l = j - leaf;
                    const ogdual op = OgGen::mv_operand(mv0 + s, l, xd, a.cvec);
                    dy = __builtin_fma(op.d, dfrag_entry(a, phase, N, k, l), 0.0);
                }
                y[s] = ogdual(a.y0[OgGen::MV_Y0(mv0 + s) + k], dy);
            }
        }
        OgGen::group_eval(g, k, xd, (const ogdual*)y, a.cvec, out);
    }
#pragma unroll
    for (int o = 0; o < (OgGen::MAX_OUT > OgGen::MAX_NMV ? OgGen::MAX_OUT : OgGen::MAX_NMV); ++o) {
        if (o >= nout) break;
        jrow[OgGen::G_ROW(g, o) + k] = out[o].d;
    }
}
#endif

// Mode 4, the same derivatives with the work lists of the structured sweep: a workgroup per column
// zero-fills its row of J_T, then evaluates only the row items that read x_j (OGT_COL / OGT_ELEM) and,
// when x_j is a collocated state, that state's defect rows: column l of D times the operand's derivative,
// minus the dynamics term's derivative on the diagonal.  Same numbers as mode 3 (tests compare both with
// the CPU twin), a fraction of the evaluations.
#ifdef OGK_HAS_AUX
__global__ __launch_bounds__(256) void ogk_exact_struct(const ogk_args a) {
    const int j = a.col_lo + (int)blockIdx.x;
    if (j >= a.col_hi) return;
    const int tid = (int)threadIdx.x;
    double* jrow = a.jt + (long)(j - a.col_lo) * OgGen::M;
    if (jt_needs_fill(a)) {                     // (a registered buffer keeps its structural zeros)
        for (int r = tid; r < OgGen::M; r += 256) jrow[r] = 0.0;
        __syncthreads();
    }
    const XDual xd{a.x0, j};
    const int4 rec = OGT_COL[j];
    for (int e = rec.x + tid; e < rec.y; e += 256) {
        const int4 it = OGT_ELEM[e];
        int row;
        const ogdual v = OgGen::item_value(it.x, it.y, it.z, xd, a.y0, a.cvec, &row);
        jrow[row] = v.d;
    }
    const int own_lo = rec.z, own_hi = rec.w & 0x3fffffff;
    if (own_hi > own_lo) {
        // x_j is node l of the state behind one collocation product
        int si = -1, l = 0;
        for (int s = 0; s < OgGen::N_MV; ++s) {
            const int leaf = OGT_SLOT[s].v[2], len = OGT_SLOT[s].v[0];
            if (j >= leaf && j < leaf + len) {
                si = s;
                l = j - leaf;
            }
        }
        if (si >= 0) {
            const int N = OGT_SLOT[si].v[0], phase = OGT_SLOT[si].v[5], row0 = OGT_SLOT[si].v[3];
            // bit 0: the dynamics term at node k reads the state at node k; bit 1: it reads the
            // state's slice in some other way (every node then)
            const int reads = OGT_SLOT[si].v[6];
            const ogdual op = OgGen::mv_operand(si, l, xd, a.cvec);
            for (int k = tid; k < N; k += 256) {
                double v = __builtin_fma(op.d, dfrag_entry(a, phase, N, k, l), 0.0);
                if ((reads & 2) || ((reads & 1) && k == l)) v = v - OgGen::tail_one(si, k, xd, a.cvec).d;
                jrow[row0 + k] = v;
            }
        }
    }
}
#endif

constexpr int SWEEP_THREADS = 512;   // ogk_sweep / ogk_eval workgroup: 8 wavefronts
constexpr int SWEEP_WAVES = SWEEP_THREADS / 64;

// ------------------------------------------------------------------------------------------
// Mode 0: F(x0) and the scratch the structured sweep reuses.  Collocation workgroup = (phase,
// 16-node tile): the states are the 16 rows of the A operand, so ONE MFMA chain yields every
// state's collocation product for the tile; afterwards each wavefront evaluates one state's
// dynamics term (a short dependent chain each, run concurrently).  Row workgroups: one
// wavefront per 64 elements of one traced output.
// ------------------------------------------------------------------------------------------
template <bool FUSED>
__device__ __forceinline__ void publish_row(const ogk_args& a, const int row, const double val) {
    const double zz = val - val;
    a.f0[row] = val;
    // fused launch: z may be read by other workgroups of the same kernel (non-finite rows only)
    if (FUSED) __hip_atomic_store(&a.z[row], zz, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    else a.z[row] = zz;
    if (zz != zz) atomicAdd(a.nonfinite, 1);
}

template <bool FUSED>
__device__ __forceinline__ void eval_defect_body(const ogk_args& a, const int bx, double* lds) {
    const int4 blk = OGT_EVALBLK[bx];                   // {group, node tile, first slot, #slots}
    const int nt = blk.y, mv0 = blk.z, nmv = blk.w;
    const ogt_int8 rec0 = OGT_SLOT[mv0];
    const int N = rec0.v[0];
    const int KS = (N + 3) >> 2;
    const int NP = KS * 4;
    const int tid = (int)threadIdx.x;
    const int wave = tid >> 6, lane = tid & 63, lk = lane >> 4;

    double* dpanel = lds;
    double* xt = lds + KS * 64;
    double* ybuf = xt + OgGen::MAX_NMV * NP;            // [state][16 nodes]
    const double* src = a.dfrag + a.dfrag_off[rec0.v[5]] + (long)nt * KS * 64;
    constexpr int UNR = 4;
    double pv[UNR];
#pragma unroll
    for (int u = 0; u < UNR; ++u)
        pv[u] = (tid + SWEEP_THREADS * u < KS * 64) ? src[tid + SWEEP_THREADS * u] : 0.0;
    // operands: one collocation slot per wavefront at a time (no divergence in mv_operand)
    const XCol base{a.x0, -1, 0.0};
    for (int s = wave; s < OgGen::MAX_NMV; s += SWEEP_WAVES)
        for (int l = lane; l < NP; l += 64) {
            double v = 0.0;
            if (s < nmv && l < N) {
                v = OgGen::mv_operand(mv0 + s, l, base, a.cvec);
                if (nt == 0) a.xop[OGT_SLOT[mv0 + s].v[4] + l] = v;
            }
            xt[s * NP + l] = v;
        }
#pragma unroll
    for (int u = 0; u < UNR; ++u)
        if (tid + SWEEP_THREADS * u < KS * 64) dpanel[tid + SWEEP_THREADS * u] = pv[u];
    for (int i = tid + SWEEP_THREADS * UNR; i < KS * 64; i += SWEEP_THREADS) dpanel[i] = src[i];
    __syncthreads();

    // The last wavefront runs the MFMA chain; meanwhile the others evaluate the dynamics terms (one state per
    // wavefront at the tile's 16 nodes): those do not depend on the products, only the final subtraction does.
    constexpr int TR = (OgGen::MAX_NMV + SWEEP_WAVES - 1) / SWEEP_WAVES;
    if (wave == SWEEP_WAVES - 1) {
        const int srow = lane & 15;
        v4f64 acc = {0.0, 0.0, 0.0, 0.0};
        const double* xrow = xt + (srow < OgGen::MAX_NMV ? srow : 0) * NP;
        const bool live = srow < nmv;
        // LDS operands of the next chunk are requested before this chunk's MFMAs issue
        constexpr int CH = 8;
        double bv[CH], av[CH];
#pragma unroll
        for (int u = 0; u < CH; ++u) {
            bv[u] = u < KS ? dpanel[u * 64 + lane] : 0.0;
            av[u] = (u < KS && live) ? xrow[u * 4 + lk] : 0.0;
        }
        for (int ks0 = 0; ks0 < KS; ks0 += CH) {
            double bn[CH], an[CH];
#pragma unroll
            for (int u = 0; u < CH; ++u) {
                const int ks = ks0 + CH + u;
                bn[u] = ks < KS ? dpanel[ks * 64 + lane] : 0.0;
                an[u] = (ks < KS && live) ? xrow[ks * 4 + lk] : 0.0;
            }
#pragma unroll
            for (int u = 0; u < CH; ++u)
                if (ks0 + u < KS) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(av[u], bv[u], acc, 0, 0, 0);
#pragma unroll
            for (int u = 0; u < CH; ++u) { bv[u] = bn[u]; av[u] = an[u]; }
        }
        // C/D layout: node = lane & 15, state = (lane >> 4) + 4 * reg
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) ybuf[(lk + 4 * reg) * 16 + (lane & 15)] = acc[reg];
    }
    const int k = nt * 16 + lane;
    const bool node_on = lane < 16 && k < N;
    double T[TR];
#pragma unroll
    for (int r = 0; r < TR; ++r) {
        const int s = wave + r * SWEEP_WAVES;
        T[r] = (node_on && s < nmv) ? OgGen::tail_one(mv0 + s, k, base, a.cvec) : 0.0;
    }
    __syncthreads();
    if (!node_on) return;
#pragma unroll
    for (int r = 0; r < TR; ++r) {
        const int s = wave + r * SWEEP_WAVES;
        if (s >= nmv) break;
        const ogt_int8 rec = OGT_SLOT[mv0 + s];
        const double y = ybuf[s * 16 + lane];
        const int row = rec.v[3] + k;
        publish_row<FUSED>(a, row, y - T[r]);
        a.t0[row] = T[r];
        a.y0[rec.v[4] + k] = y;
    }
}

template <bool FUSED>
__device__ __forceinline__ void eval_rows_body(const ogk_args& a, const int bx, double* lds) {
    // a row whose code contains a sequential sum (the cost with its running-cost quadrature) would be one lane
    // evaluating every term with its loads: the workgroup computes the terms into LDS first
    bool terms = false;
    if (TERM_CACHE) {
#pragma unroll
        for (int u = 0; u < SWEEP_WAVES; ++u) {
            const int w2 = bx * SWEEP_WAVES + u;
            if (w2 < OGT_N_ROWWAVES) terms = terms || OGT_ROWWAVE[w2].w != 0;
        }
        if (terms) {                                      // workgroup-uniform
            fill_terms<SWEEP_THREADS>(a, lds);
            __syncthreads();
        }
    }
    const int w = bx * SWEEP_WAVES + ((int)threadIdx.x >> 6);
    if (w >= OGT_N_ROWWAVES) return;
    const int4 rw = OGT_ROWWAVE[w];                       // {group, first element, group length, has a sum}
    const int k = rw.y + ((int)threadIdx.x & 63);
    if (k >= rw.z) return;
    const XColT base = make_xcolt(a, -1, 0.0, terms ? lds : nullptr);
    int row;
    const double v = OgGen::item_value(rw.x, 0, k, base, a.y0, a.cvec, &row);
    publish_row<FUSED>(a, row, v);
}

#ifdef OGK_HAS_MAIN
__global__ __launch_bounds__(SWEEP_THREADS) void ogk_eval(const ogk_args a, const int ndef) {
    extern __shared__ __attribute__((aligned(16))) double lds[];
    const int id = (int)blockIdx.x;
    // the evaluation after this one counts into the other slot: clear it now (stream order
    // makes this visible to the next launch)
    if (id == 0 && threadIdx.x == 0) {
        *a.nonfinite_next = 0;
        if (a.jt_bump) __hip_atomic_store(a.jt_launches, *a.jt_launches + 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    if (id < ndef) eval_defect_body<false>(a, id, lds);
    else eval_rows_body<false>(a, id - ndef, lds);
}
#endif

// ------------------------------------------------------------------------------------------
// Mode 1: the structured sweep.  At the sizes this engine sees (n ~ 10^2..10^4) a sweep is a
// chain of dependent global loads and dependent f64 operations (~13 ns each on gfx950), so the
// layout below is about latency: every workgroup learns its job from one wide record
// (OGT_COL / OGT_ELEM / OGT_TILE / OGT_SLOT, generated by the tracer), issues all its loads up
// front, and the long arithmetic chains (one traced output each) run in different wavefronts.
//
// Part A - J_T rows (= FD columns).  The owner of a row streams the "no dependency" value into
//   it and then re-evaluates the (group, output, element) items that read p[j].
//     heavy_column_body   a column with many items (phase final times): one workgroup, lanes =
//                         consecutive items (consecutive nodes of one output: same code);
//     light_columns_body  LIGHT_COLS neighbouring columns per workgroup: lane = column,
//                         wavefront = item slot.
// Part B - tile_body: d(defect_s)/d(state_s) for one collocation slot on the matrix cores.
// ------------------------------------------------------------------------------------------
#ifndef OGK_LIGHT_COLS
#define OGK_LIGHT_COLS 4
#endif
constexpr int LIGHT_COLS = OGK_LIGHT_COLS;   // columns per workgroup in light_columns_body
constexpr int HEAVY_FLAG = 1 << 30;  // in OGT_COL[j].w

// Rows are filled with the "no dependency" value EXCEPT at the positions the items (and the
// MFMA tiles) write: a per-row bitmap in LDS marks those, so no ordering between the fill stores
// and the item stores is needed and the fill drains in the background while the wavefronts are
// already in their (latency-bound) item chains.
__device__ __forceinline__ bool marked(const unsigned* bits, const int r) {
    return (bits[r >> 5] >> (r & 31)) & 1u;
}

__device__ __forceinline__ void fill_row(const ogk_args& a, double* jrow, const unsigned* bits,
                                         const int own_lo, const int own_hi, const int first,
                                         const int stride, const bool all_finite,
                                         const bool z_from_this_launch = false) {
    if (OGK_EXP & 16) return;
    if (all_finite) {
        // every row of F(x0) is finite: (F0-F0)/dx is plain zero.  16-byte stores on the aligned
        // pairs that are wholly free, 8-byte stores for the rest.
        const int a0 = (int)((reinterpret_cast<unsigned long long>(jrow) >> 3) & 1);
        const double2 zero2 = make_double2(0.0, 0.0);
        for (int q = first; a0 + 2 * q < OgGen::M; q += stride) {
            const int r = a0 + 2 * q;
            const bool skip0 = (r >= own_lo && r < own_hi) || marked(bits, r);
            const bool has1 = r + 1 < OgGen::M;
            const bool skip1 = !has1 || (r + 1 >= own_lo && r + 1 < own_hi) || marked(bits, r + 1);
            if (!skip0 && !skip1) {
                *reinterpret_cast<double2*>(jrow + r) = zero2;
            } else {
                if (!skip0) jrow[r] = 0.0;
                if (!skip1) jrow[r + 1] = 0.0;
            }
        }
        if (a0 && first == 0 && !(0 >= own_lo && 0 < own_hi) && !marked(bits, 0)) jrow[0] = 0.0;
    } else {                        // z carries NaN for the non-finite rows
        for (int r = first; r < OgGen::M; r += stride)
            if ((r < own_lo || r >= own_hi) && !marked(bits, r))
                jrow[r] = z_from_this_launch ? __hip_atomic_load(&a.z[r], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)
                                             : a.z[r];
    }
}

__device__ __forceinline__ void eval_item(const ogk_args& a, const int4 item, const XCol& xa,
                                          const double dx, double* jrow) {
    int row;
    const double v = OgGen::item_value(item.x, item.y, item.z, xa, a.y0, a.cvec, &row);
    jrow[row] = (v - a.f0[row]) / dx;         // row == item.w (the position marked in the bitmap)
}

constexpr int ROW_WORDS = (OgGen::M + 31) / 32;      // bitmap words per J_T row

__device__ __forceinline__ void heavy_column_body(const ogk_args& a, const int j, unsigned* bits) {
    const int tid = (int)threadIdx.x;
    const int4 col = OGT_COL[j];
    const int own_lo = col.z, own_hi = col.w & ~HEAVY_FLAG;
    const double xb = a.x0[j];
    const double xj = xb + a.h[j];
    const double dx = xj - xb;
    const bool all_finite = *a.nonfinite == 0;
    const bool fill = !all_finite | jt_needs_fill(a);      // workgroup-uniform
    double* jrow = a.jt + (long)(j - a.col_lo) * OgGen::M;
    if (fill) {
        for (int w = tid; w < ROW_WORDS; w += SWEEP_THREADS) bits[w] = 0u;
        __syncthreads();
        for (int e = col.x + tid; e < col.y; e += SWEEP_THREADS) {
            const int r = OGT_ELEM[e].w;
            atomicOr(&bits[r >> 5], 1u << (r & 31));
        }
        __syncthreads();
        fill_row(a, jrow, bits, own_lo, own_hi, tid, SWEEP_THREADS, all_finite);
        if (!all_finite && tid == 0) jt_mark_nan_fill(a);
    }
    const XCol xa{a.x0, j, xj};
    for (int e = col.x + tid; e < ((OGK_EXP & 8) ? 0 : col.y); e += SWEEP_THREADS)
        eval_item(a, OGT_ELEM[e], xa, dx, jrow);
}

__device__ __forceinline__ void light_columns_body(const ogk_args& a, const int first_j,
                                                   unsigned* bits) {
    const int tid = (int)threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
#if OGK_TRACE
    const long long t_begin = __builtin_amdgcn_s_memtime();
    const long long t_real0 = __builtin_amdgcn_s_memrealtime();
#endif
    // ---- everything this thread will need, requested before anything is waited for
    constexpr int WPR = SWEEP_WAVES / LIGHT_COLS;               // wavefronts sharing one row
    const int cf = wave / WPR;                                  // the row this wavefront fills
    const int jf = first_j + cf;
    const int ji = first_j + lane;                              // the column this lane evaluates
    const bool fill_on = jf < a.col_hi;
    const bool item_on = lane < LIGHT_COLS && ji < a.col_hi;
    const int4 colf = OGT_COL[fill_on ? jf : a.col_lo];
    const int4 coli = OGT_COL[item_on ? ji : a.col_lo];
    const double xb = a.x0[item_on ? ji : a.col_lo];
    const double hh = a.h[item_on ? ji : a.col_lo];
    const bool all_finite = *a.nonfinite == 0;
    int4 item = make_int4(0, 0, 0, 0);
    const bool col_live = item_on && !(coli.w & HEAVY_FLAG);
    const bool has_item = col_live && coli.x + wave < coli.y;
    if (has_item) item = OGT_ELEM[coli.x + wave];

    // ---- a registered (persistent-zero) buffer needs no fill while F(x0) is finite: straight to the items
    if (!all_finite | jt_needs_fill(a)) {                        // workgroup-uniform
        // ---- mark the positions the items will write
        for (int w = tid; w < LIGHT_COLS * ROW_WORDS; w += SWEEP_THREADS) bits[w] = 0u;
        __syncthreads();
        if (has_item) {
            unsigned* mine = bits + lane * ROW_WORDS;
            atomicOr(&mine[item.w >> 5], 1u << (item.w & 31));
            for (int e = coli.x + wave + SWEEP_WAVES; e < coli.y; e += SWEEP_WAVES) {
                const int r = OGT_ELEM[e].w;
                atomicOr(&mine[r >> 5], 1u << (r & 31));
            }
        }
        __syncthreads();

        // ---- fill around them (heavy columns are filled by their own workgroup); the stores drain
        //      while the item chains below run
        if (fill_on && !(colf.w & HEAVY_FLAG))
            fill_row(a, a.jt + (long)(jf - a.col_lo) * OgGen::M, bits + cf * ROW_WORDS, colf.z,
                     colf.w, (wave % WPR) * 64 + lane, 64 * WPR, all_finite);
        if (!all_finite && tid == 0) jt_mark_nan_fill(a);
    }
#if OGK_TRACE
    const long long t_filled = __builtin_amdgcn_s_memtime();
#endif
    if (!has_item) return;
    // ---- items: lane = column, wavefront = item slot
    const double xj = xb + hh;
    const double dx = xj - xb;
    double* jrow = a.jt + (long)(ji - a.col_lo) * OgGen::M;
    const XCol xa{a.x0, ji, xj};
#if OGK_TRACE
    const long long t_ready = __builtin_amdgcn_s_memtime();
#endif
    if (!(OGK_EXP & 8)) {
        eval_item(a, item, xa, dx, jrow);
        for (int e = coli.x + wave + SWEEP_WAVES; e < coli.y; e += SWEEP_WAVES)
            eval_item(a, OGT_ELEM[e], xa, dx, jrow);
    }
#if OGK_TRACE
    if (lane == 0) {
        __builtin_amdgcn_s_waitcnt(0);
        double* t = jrow + 8 * wave;
        t[0] = 1.0e6 + wave; t[1] = (double)t_begin; t[2] = (double)t_filled; t[3] = (double)t_ready;
        t[4] = (double)__builtin_amdgcn_s_memtime(); t[5] = (double)(coli.y - coli.x);
        t[6] = (double)t_real0; t[7] = (double)__builtin_amdgcn_s_memrealtime();
    }
#endif
}

// Part B.  One wavefront = one (16 perturbed columns) x (16 nodes) tile of one collocation slot.
// Every wavefront of the sweep uses its D panel exactly once, so the B operands are read straight
// from the L2-resident operand image (512 contiguous bytes per step) into registers, a chunk of
// k-steps ahead of the MFMAs - no LDS round trip and no workgroup barrier on this path (the
// evaluation and dense kernels, which reuse a panel across wavefronts/states, stage it in LDS).
__device__ __forceinline__ void tile_body(const ogk_args& a, const int bx) {
#if OGK_TRACE
    const long long t_begin = __builtin_amdgcn_s_memtime();
    long long t_staged = 0, t_mfma = 0;
#endif
    const int4 tile = OGT_TILE[bx];                    // {slot, tile group, node tile}
    const int slot = tile.x, nt = tile.z;
    const ogt_int8 rec = OGT_SLOT[slot];
    const int N = rec.v[0], g = rec.v[1], leaf = rec.v[2], row0 = rec.v[3], y0off = rec.v[4];
    const bool diag = rec.v[6] & 1, generic = rec.v[6] & 2;
    const int dep0 = rec.v[7] >> 12, ndep = rec.v[7] & 0xfff;
    const int KS = (N + 3) >> 2;
    const int tid = (int)threadIdx.x;
    const int wave = tid >> 6, lane = tid & 63, lk = lane >> 4;
    const int l0 = (tile.y * SWEEP_WAVES + wave) * 16;  // first slice offset of this wave's tile
    if (l0 >= N || leaf + l0 >= a.col_hi || leaf + l0 + 16 <= a.col_lo) return;
    const int k = nt * 16 + (lane & 15);                // output node of this lane
    const int la = l0 + (lane & 15);                    // A-operand row of this lane
    (void)g;

    // ---- requests first: operands of the first chunk, this lane's perturbation, epilogue inputs
    const double* bsrc = a.dfrag + a.dfrag_off[rec.v[5]] + (long)nt * KS * 64 + lane;
    const double* xop = a.xop + y0off;                  // base operands, written by mode 0
    constexpr int CH = 10;                              // k-steps per chunk
    double bv[CH], av[CH];
#pragma unroll
    for (int u = 0; u < CH; ++u) {
        const int l = u * 4 + lk;
        bv[u] = (u < KS) ? bsrc[u * 64] : 0.0;
        av[u] = (u < KS && l < N) ? xop[l] : 0.0;
    }
    const bool a_on = la < N;
    const double xa_b = a.x0[a_on ? leaf + la : leaf];
    const double xa_h = a.h[a_on ? leaf + la : leaf];
    const bool k_on = k < N;
    const int row = row0 + (k_on ? k : 0);
    const double t_base = a.t0[row];
    const double f_base = a.f0[row];
    double xbv[4], hv[4];
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) {
        const int lc = l0 + lk + 4 * reg;
        const int jj = leaf + ((k_on && lc < N) ? lc : 0);
        xbv[reg] = a.x0[jj];
        hv[reg] = a.h[jj];
    }

    // ---- the dynamics term on the diagonal (k == own perturbed node) needs neither the operands
    //      nor the MFMA result: its chain runs while the loads above are in flight
    double t_diag = t_base;
    bool have_diag = false;
    {
        const int lc = k;                                // column whose perturbed node is k
        const int reg = (lc - l0 - lk) >> 2;
        have_diag = diag && k_on && lc >= l0 + lk && ((lc - l0 - lk) & 3) == 0 && reg < 4 && lc < N &&
                    leaf + lc >= a.col_lo && leaf + lc < a.col_hi;
        if (have_diag) {
            const int jd = leaf + lc;
            const double xbd = a.x0[jd];
            const XCol xd{a.x0, jd, xbd + a.h[jd]};
            t_diag = OgGen::tail_one(slot, k, xd, a.cvec);
        }
    }
#if OGK_TRACE
    t_staged = __builtin_amdgcn_s_memtime();
#endif

    // A operand: row (lane & 15) is the state vector with its own element perturbed
    double hit_v = 0.0;
    if (a_on) {
        const XCol xa{a.x0, leaf + la, xa_b + xa_h};
        hit_v = OgGen::mv_operand(slot, la, xa, a.cvec);
    }
    v4f64 acc = {0.0, 0.0, 0.0, 0.0};
    for (int ks0 = 0; ks0 < KS; ks0 += CH) {
        // next chunk's operands are requested before this chunk's MFMAs issue
        double bn[CH], an[CH];
#pragma unroll
        for (int u = 0; u < CH; ++u) {
            const int ks = ks0 + CH + u;
            const int l = ks * 4 + lk;
            bn[u] = (ks < KS) ? bsrc[ks * 64] : 0.0;
            an[u] = (ks < KS && l < N) ? xop[l] : 0.0;
        }
#pragma unroll
        for (int u = 0; u < CH; ++u) {
            const int ks = ks0 + u;
            if (ks < KS) {
                const double aop = (ks * 4 + lk == la) ? hit_v : av[u];
                acc = __builtin_amdgcn_mfma_f64_16x16x4f64(aop, bv[u], acc, 0, 0, 0);
            }
        }
#pragma unroll
        for (int u = 0; u < CH; ++u) { bv[u] = bn[u]; av[u] = an[u]; }
    }
#if OGK_TRACE
    t_mfma = __builtin_amdgcn_s_memtime();
#endif
    if (!k_on) return;
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) {
        const int lc = l0 + lk + 4 * reg;
        const int j = leaf + lc;
        if (lc >= N || j < a.col_lo || j >= a.col_hi) continue;
        const double xj = xbv[reg] + hv[reg];
        const double dx = xj - xbv[reg];
        double t = (have_diag && lc == k) ? t_diag : t_base;
        if (generic) {
            // rare: the dynamics term of node k reads p[j] through something other than the
            // state's own sample at k - take the dependency-table scan
            bool reads = diag && k == lc;
            for (int d = dep0; d < dep0 + ndep; ++d) {
                const int kind = OgGen::DEP_KIND(d), base_d = OgGen::DEP_BASE(d);
                reads = reads || (kind == 1 ? (base_d + k == j)
                                            : (j >= base_d && j < base_d + OgGen::DEP_CNT(d)));
            }
            if (reads) {
                const XCol xg{a.x0, j, xj};
                t = OgGen::tail_one(slot, k, xg, a.cvec);
            }
        }
        const double val = acc[reg] - t;
        a.jt[(long)(j - a.col_lo) * OgGen::M + row] = (val - f_base) / dx;
    }
#if OGK_TRACE
    if (lane == 0 && leaf + l0 >= a.col_lo && leaf + l0 < a.col_hi) {
        __builtin_amdgcn_s_waitcnt(0);
        double* t = a.jt + (long)(leaf + l0 - a.col_lo) * OgGen::M + row0 + nt * 16;
        t[0] = 2.0e6 + wave; t[1] = (double)t_begin; t[2] = (double)t_staged; t[3] = (double)t_mfma;
        t[4] = (double)__builtin_amdgcn_s_memtime(); t[5] = (double)bx;
    }
#endif
}

// ------------------------------------------------------------------------------------------
// Mode 5 (ogk_fused): modes 0 and 1 as ONE launch into a registered persistent-zero buffer.  The first
// workgroups of the grid are the evaluation workgroups (they produce F(x0) for the caller, as in mode 0); the
// sweep workgroups that follow do not consume anything from them: what a difference quotient needs of the
// base point - the base value of a row item, the base collocation products of a node tile - is recomputed by
// the workgroup that uses it, with the same device functions and the same MFMA chain, hence the same bits.  A
// kernel boundary (drain, cache write-back / invalidate, dispatch) between the evaluation and the sweep costs a
// third of a step at the sizes of this engine; loads from another workgroup's results inside one kernel would
// have to bypass the (per-XCD, mutually incoherent) L2s, which is slower still (both measured, round 1).
//   fz_light_body   a run of <= 16 neighbouring columns whose defect items lie in one (defect group, 16-node
//                   tile): the item wavefronts put the group's operands into LDS, a slot each, and go on into
//                   their items' long parts without waiting (lane = column, perturbed | base; wavefront = item
//                   slot); one wavefront runs the tile's MFMA chain with the D^T panel straight from memory.
//   fz_heavy_part   one (defect group, node tile) of a column with many items, served the same way; slots of
//                   items that share their code, one wavefront each (lanes = items, perturbed | base).
//   fz_tile_body    d(defect_s)/d(state_s): <= 7 column tiles per workgroup share ONE base product / base
//                   dynamics term / diagonal term, computed by otherwise idle wavefronts.
// Nothing is filled and nobody waits: the sweep workgroups write the positions that can be non-zero; when F(x0)
// has non-finite rows (or the previous launch left a NaN fill) the LAST evaluation workgroup to finish fills
// the rows from z around those positions (finish_eval).  The launch arguments are pointers only.
// ------------------------------------------------------------------------------------------
// Timing experiments only: -DOGK_FZ=<mask> removes pieces of ogk_fused - 2 = no base-product chain in the light
// workgroups, 4 = no operand staging there (and their service wavefronts do not wait for it), 16 = evaluation
// workgroups do nothing, 32 = heavy columns skipped, 2048 = no light items.  Results are wrong with any bit set.
#ifndef OGK_FZ
#define OGK_FZ 0
#endif


// barrier that orders LDS traffic only: the global stores of the fill keep draining underneath
// (__syncthreads() would wait for them)
__device__ __forceinline__ void lds_barrier() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup", "local");
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup", "local");
}

// What is left of the dependence on the evaluation in the fused launch.  A registered (persistent-zero)
// buffer needs a fill only when F(x0) of THIS launch has non-finite rows (NaN in those rows of every column)
// or when the previous launch into the buffer left such a fill behind.  Nobody waits for that verdict:
// every evaluation workgroup takes a ticket when its results are out, and the one that draws the last
// ticket - by then the count of non-finite rows is complete - looks at it and, in the rare case, fills
// every row of this launch's block from z (0, or NaN) around the positions the sweep workgroups write
// (bitmap per row from the column's item list, as in mode 1).  It also resets the ticket, so that the
// launch arguments do not depend on how many launches went before.
__device__ __forceinline__ void fz_fill_from_z(const ogk_args& a, unsigned* bits) {
    const int tid = (int)threadIdx.x;
    for (int j = a.col_lo; j < a.col_hi; ++j) {
        const int4 col = OGT_COL[j];
        const int own_lo = col.z, own_hi = col.w & ~HEAVY_FLAG;
        for (int w = tid; w < ROW_WORDS; w += SWEEP_THREADS) bits[w] = 0u;
        __syncthreads();
        for (int e = col.x + tid; e < col.y; e += SWEEP_THREADS) {
            const int r = OGT_ELEM[e].w;
            atomicOr(&bits[r >> 5], 1u << (r & 31));
        }
        __syncthreads();
        fill_row(a, a.jt + (long)(j - a.col_lo) * OgGen::M, bits, own_lo, own_hi, tid, SWEEP_THREADS, false, true);
        __syncthreads();
    }
}

__device__ __forceinline__ void finish_eval(const ogk_args& a, const unsigned n_eval, unsigned* bits) {
    __shared__ int s_last;
    __builtin_amdgcn_s_waitcnt(0);          // this wavefront's write-through stores have been acknowledged
    __syncthreads();
    if (threadIdx.x == 0) {
        const unsigned t = __hip_atomic_fetch_add(a.ready, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        int last = 0;
        if (t + 1u == n_eval) {
            // the counts of non-finite rows were performed before their workgroups' tickets, at the memory side.
            // Two independent loads, one round trip; the ticket's reset needs no answer.
            const int bad = __hip_atomic_load(a.nonfinite, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            const unsigned st = __hip_atomic_load(a.jt_state, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            const unsigned gen = __hip_atomic_load(a.jt_launches, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) + 1u;
            __hip_atomic_store(a.ready, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            // this launch's number; the count of non-finite rows moves to where later kernels and the host read
            // it, the counter is zero again for the next launch (nothing of this is a launch argument)
            __hip_atomic_store(a.jt_launches, gen, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_store(a.nonfinite_result, bad, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (a.ptail) a.ptail[OgGen::M] = (double)bad;      // host transfer: the count travels with F(x0)
            __hip_atomic_store(a.nonfinite, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (bad != 0) __hip_atomic_store(a.jt_state, gen, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            last = (bad != 0 || st == gen - 1u) ? 1 : 0;
        }
        s_last = last;
    }
    __syncthreads();
    if (s_last) fz_fill_from_z(a, bits);
}

// One chunk [ks0, ks0 + CH) of a node tile's D^T panel, straight from the operand image into registers.  Every load
// is issued whatever KS is - a k-step past the panel reads the panel's last step again and is replaced by zero - so
// the requests of a chunk leave back to back, with no scalar branch between them.
template <int CH>
__device__ __forceinline__ void fz_load_panel(const double* bsrc, const int ks0, const int KS, double (&bv)[CH]) {
#pragma unroll
    for (int u = 0; u < CH; ++u) {
        const int ks = ks0 + u;
        const double v = bsrc[(ks < KS ? ks : KS - 1) * 64];
        bv[u] = ks < KS ? v : 0.0;
    }
}

// the first two chunks of a panel: asked for as soon as the record that names the panel is there
template <int CH>
__device__ __forceinline__ void fz_load_first(const double* bsrc, const int KS, double (&b0)[CH], double (&b1)[CH]) {
    fz_load_panel<CH>(bsrc, 0, KS, b0);
    if (CH < KS) fz_load_panel<CH>(bsrc, CH, KS, b1);
}

// The k-ordered chain of ogk_eval over a node tile in chunks of CH k-steps.  bsrc: the tile's [KS][64] panel in the
// operand image (+ lane); aop(ks): this lane's A operand of step ks (0 for ks >= KS).  The panel is requested a chunk
// ahead through two register buffers that take turns (no copies; fz_load_first fills them).  A whole chunk is CH
// MFMAs back to back, operands read unconditionally, no branch per k-step; only the last chunk, when KS is no multiple
// of CH, steps over the k-steps it does not have (an MFMA on zero operands would leave the accumulator as it is, bit
// for bit, but costs its 8 passes of the matrix pipe: a quarter more of them at 128 nodes in chunks of 10).
template <int CH, class AOp>
__device__ __forceinline__ v4f64 fz_chain(const double* bsrc, const int KS, double (&b0)[CH], double (&b1)[CH],
                                          const AOp& aop) {
    v4f64 acc = {0.0, 0.0, 0.0, 0.0};
    const auto steps = [&](const double (&bv)[CH], const int ks0) {
        double av[CH];
#pragma unroll
        for (int u = 0; u < CH; ++u) av[u] = aop(ks0 + u);
        if (ks0 + CH <= KS) {
#pragma unroll
            for (int u = 0; u < CH; ++u) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(av[u], bv[u], acc, 0, 0, 0);
        } else {                        // the last chunk when it is not whole: its own steps only
#pragma unroll
            for (int u = 0; u < CH; ++u)
                if (ks0 + u < KS) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(av[u], bv[u], acc, 0, 0, 0);
        }
    };
    for (int ks0 = 0;; ks0 += 2 * CH) {
        steps(b0, ks0);
        if (ks0 + CH >= KS) break;
        if (ks0 + 2 * CH < KS) fz_load_panel<CH>(bsrc, ks0 + 2 * CH, KS, b0);
        steps(b1, ks0 + CH);
        if (ks0 + 2 * CH >= KS) break;
        if (ks0 + 3 * CH < KS) fz_load_panel<CH>(bsrc, ks0 + 3 * CH, KS, b1);
    }
    return acc;
}

constexpr int FZ_COLS = OGT_LGRP_COLS;          // columns of a light workgroup of the fused launch (tracer)
// (F(x0 + h e_j) - F(x0)) / dx for one row item, with the base value from the partner lane (FZ_COLS further on, same item, unperturbed x)
template <class XA>
__device__ __forceinline__ void eval_item_paired(const ogk_args& a, const int4 item, const XA& xa, const bool base_role,
                                                 const double dx, double* jrow, double* packed) {
    int row;
    const double v = OgGen::item_value(item.x, item.y, item.z, xa, a.y0, a.cvec, &row);
    const double v0 = __shfl_down(v, FZ_COLS);
    if (!base_role) {
        const double q = (v - v0) / dx;
        jrow[row] = q;
        if (packed) *packed = q;
    }
}

constexpr int FZ_MAXN = OgGen::MAX_NODES;                      // longest phase
constexpr int FZ_NP = ((FZ_MAXN + 3) / 4) * 4;
constexpr int FZ_ROUNDS = 2;                                    // items per column and wavefront evaluated ahead of the base products
constexpr int FZ_ITEM_WAVES = SWEEP_WAVES - 1;                 // item slots of a light workgroup (the last wavefront
                                                               // runs the MFMA chain instead)
// LDS of a light workgroup: [KS][64] (where the tile's D panel was staged until the chain took it from memory; the
// window keeps its size) | operands [state][NP] | base products [state][N]
constexpr size_t FZ_TILE_DOUBLES = (size_t)(FZ_NP / 4) * 64 + (size_t)OgGen::MAX_NMV * (FZ_NP + FZ_MAXN);
// ... | base terms of the program's sequential sums [N_TERMS] (workgroups with such items)
constexpr size_t FZ_LDS_BYTES = (FZ_TILE_DOUBLES + TERM_DOUBLES) * sizeof(double);

#if OGK_TRACE                           // tools/trace_fused.py: phase stamps of every wavefront, next to the results
#define FZ_TRACE_DECL(kind_) long long tr_[6] = {(long long)__builtin_amdgcn_s_memrealtime(), 0, 0, 0, 0, 0}; \
    const int tr_kind_ = (kind_)
#define FZ_STAMP(i) tr_[i] = (long long)__builtin_amdgcn_s_memrealtime()
#define FZ_STAMP_SET(i, v) tr_[i] = (v)
#define FZ_TRACE_OUT(a_)                                                                                   \
    do {                                                                                                   \
        if (((int)threadIdx.x & 63) == 0 && (a_).trace) {                                                  \
            double* t_ = (a_).trace + ((long)blockIdx.x * SWEEP_WAVES + ((int)threadIdx.x >> 6)) * 8;       \
            t_[0] = (double)tr_kind_; t_[1] = (double)tr_[0]; t_[2] = (double)tr_[1]; t_[3] = (double)tr_[2]; \
            t_[4] = (double)tr_[3]; t_[5] = (double)tr_[4]; t_[6] = (double)tr_[5];                          \
            t_[7] = (double)__builtin_amdgcn_s_memrealtime();                                              \
        }                                                                                                  \
    } while (0)
#else
#define FZ_TRACE_DECL(kind_) do { } while (0)
#define FZ_STAMP(i) do { } while (0)
#define FZ_STAMP_SET(i, v) (void)(v)
#define FZ_TRACE_OUT(a_) do { } while (0)
#endif

// LDS of a workgroup that owns one (defect group, node tile): what its service wavefront needs
struct FzTile {
    double* dpanel;     // [KS][64] not used by the light workgroups and heavy parts any more
    double* xt;         // [state][NP] operands of the group
    double* yb;         // [state][N] base products (the tile's nodes)
};
__device__ __forceinline__ FzTile fz_tile_lds(double* lds) {
    FzTile t;
    t.dpanel = lds;
    t.xt = lds + (FZ_NP / 4) * 64;
    t.yb = t.xt + OgGen::MAX_NMV * FZ_NP;
    return t;
}
// Hand-overs inside a sweep workgroup go through words in LDS, and LDS keeps what the previous workgroup left there:
// the words are cleared behind ONE barrier at the very top of the workgroup, ahead of its first load, where it costs the
// spread of the wavefronts' starts and nothing else.  After it nobody waits for anybody except for the data itself.
__device__ __forceinline__ void fz_sync_reset(int* words, const int n) {
    if ((int)threadIdx.x < n) words[threadIdx.x] = 0;
    lds_barrier();
}
// a producer's results are in LDS: one more of them
__device__ __forceinline__ void lds_count_up(int* word) {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup", "local");     // (LDS only: loads in flight stay in flight)
    __hip_atomic_fetch_add(word, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}
// wait until `need` producers have counted up
__device__ __forceinline__ void lds_count_wait(int* word, const int need) {
    while (*reinterpret_cast<volatile int*>(word) < need) __builtin_amdgcn_s_sleep(1);
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup", "local");
}

// A wavefront's share of the operands of its workgroup's (defect group, node tile): the group's slots wave,
// wave + SWEEP_WAVES, ... as [NP] rows of t.xt, zero-padded to NP - a slot per wavefront, no divergence - and one
// count for the service wavefront.  An item wavefront does not wait for anything: its items' long parts come next.
// (The service wavefront has a slot of its own only in a group of SWEEP_WAVES states or more: nobody does two.)
__device__ __forceinline__ void fz_stage_operands(const ogk_args& a, const FzTile& t, const int mv0, const int nmv,
                                                  const int N, int* staged) {
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int NP = ((N + 3) >> 2) << 2;
    constexpr int ST_S = (OgGen::MAX_NMV + SWEEP_WAVES - 1) / SWEEP_WAVES, ST_L = (FZ_NP + 63) / 64;
    const XCol xbase{a.x0, -1, 0.0};
    if (wave >= nmv) return;
#pragma unroll
    for (int u = 0; u < ST_S; ++u)
#pragma unroll
        for (int q = 0; q < ST_L; ++q) {
            const int sl = wave + u * SWEEP_WAVES, l = lane + q * 64;
            if (sl < nmv && l < NP) t.xt[sl * NP + l] = l < N ? OgGen::mv_operand(mv0 + sl, l, xbase, a.cvec) : 0.0;
        }
    if (lane == 0) lds_count_up(staged);
}

// The service wavefront of a light workgroup or heavy part: the tile's D^T panel straight from the operand image into
// registers - asked for before it waits for the operands, which the wavefronts with a slot (the first
// min(nmv, SWEEP_WAVES) of them) put into LDS -, the chain, the base products [state][N] of the tile's nodes into t.yb.
__device__ __forceinline__ long long fz_service_tile(const ogk_args& a, const FzTile& t, const int nt, const int nmv,
                                                     const int N, const int phase, int* staged) {
    const int lane = (int)threadIdx.x & 63, lk = lane >> 4, srow = lane & 15;
    const int KS = (N + 3) >> 2, NP = KS << 2;
    constexpr int CH = 8;
    const double* bsrc = a.dfrag + OgGen::DFRAG_OFF(phase) + (long)nt * KS * 64 + lane;
    double b0[CH], b1[CH];
    fz_load_first<CH>(bsrc, KS, b0, b1);
    if (!(OGK_FZ & 4)) lds_count_wait(staged, nmv < SWEEP_WAVES ? nmv : SWEEP_WAVES);
    const long long t_seen = OGK_TRACE ? (long long)__builtin_amdgcn_s_memrealtime() : 0;     // (-> the caller's stamp)
    const bool live = srow < nmv;
    const double* xrow = t.xt + (live ? srow : 0) * NP + lk;
    const v4f64 acc = fz_chain<CH>(bsrc, KS, b0, b1, [&](const int ks) {
        const bool on = live && ks < KS;
        const double v = xrow[on ? ks * 4 : 0];
        return on ? v : 0.0;
    });
    // C/D layout: node = lane & 15, state = (lane >> 4) + 4 * reg
    const int k = nt * 16 + (lane & 15);
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) {
        const int st = lk + 4 * reg;
        if (st < nmv && k < N) t.yb[st * N + k] = acc[reg];
    }
    return t_seen;
}

// A light workgroup.  No barrier stands between a wavefront and its work (fz_sync_reset apart): an item wavefront
// puts its slot of the group's operands into LDS, counts up and goes on into the long parts of its items; the service
// wavefront has the tile's panel on its way meanwhile, starts the chain when the count is full and counts the base
// products in; the item wavefronts look for that only when their tails are in registers.  A workgroup whose items
// contain a sequential sum keeps a barrier behind which the sum's base terms are in LDS.
__device__ __forceinline__ void fz_light_body(const ogk_args& a, const int b, double* lds) {
    __shared__ int s_sync[2];           // [0] slots of operands in LDS, [1] base products of the tile in LDS
    FZ_TRACE_DECL(1);
    fz_sync_reset(s_sync, 2);
    // {first column, columns, y0 offset of the tile's first slot, node tile, first slot, slots (0: no defect
    //  items), nodes, phase}
    const ogt_int8 grp = OGT_LGRP[b];
    const int first_j = grp.v[0], cnt = grp.v[1], y0_first = grp.v[2], nt = grp.v[3];
    const int mv0 = grp.v[4], nmv = grp.v[5], N = grp.v[6], phase = grp.v[7] & 0xffff;
    const bool terms = TERM_CACHE && (grp.v[7] >> 16) != 0;     // some item contains a sequential sum
    double* tc = lds + FZ_TILE_DOUBLES;
    const bool has_tile = nmv > 0;
    const int tid = (int)threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const bool service = wave == SWEEP_WAVES - 1;   // no items: the tile's MFMA chain
    const FzTile t = fz_tile_lds(lds);
    // items: lanes 0..FZ_COLS-1 evaluate at x0 + h e_j, the next FZ_COLS lanes the same items at x0 -
    // one instruction stream, so the base value of a row item costs no time; wavefront = item slot
    const int cl = lane % FZ_COLS;
    const bool base_role = lane >= FZ_COLS;
    const int ji = first_j + cl;
    const bool item_on = !service && lane < 2 * FZ_COLS && cl < cnt && ji >= a.col_lo && ji < a.col_hi;
    const int4 coli = OGT_LRNG[b * FZ_COLS + cl];   // {items begin, end} of this lane's column (no OGT_COL round trip)
    const double xb = a.x0[item_on ? ji : first_j];
    const double hh = a.h[item_on ? ji : first_j];
    int4 item = make_int4(0, 0, 0, 0);
    const bool has_item = item_on && coli.x + wave < coli.y;
    if (has_item) item = OGT_ELEM[coli.x + wave];
    // a wavefront first puts its slot of the group's operands into LDS; then, in a workgroup whose items contain a
    // sequential sum, everybody fills the sum's base terms and meets at the barrier that publishes them
    if (has_tile && !(OGK_FZ & 4)) fz_stage_operands(a, t, mv0, nmv, N, &s_sync[0]);
    if (terms) {                                    // (uniform over the workgroup)
        fill_terms<SWEEP_THREADS>(a, tc);
        lds_barrier();        // (only LDS data crosses it: global loads in flight stay in flight)
    }
    FZ_STAMP(1);
    if (service) {
        if (has_tile && !(OGK_FZ & 2)) FZ_STAMP_SET(1, fz_service_tile(a, t, nt, nmv, N, phase, &s_sync[0]));
        FZ_STAMP(2);
        if (lane == 0) lds_count_up(&s_sync[1]);
        FZ_TRACE_OUT(a);
        return;
    }
    if (has_item && !(OGK_FZ & 2048)) {
        const double xj = xb + hh;
        const double dx = xj - xb;
        double* jrow = a.jt + (long)(ji - a.col_lo) * OgGen::M;
        // sharded sweeps: every value also goes straight into this rank's message (the column's packed entries:
        // its collocation block first, then its items in work-list order) - no separate gather kernel
        double* pcol = a.pvals ? a.pvals + a.poff[ji] + (coli.z - coli.x) : nullptr;
        const XColT xa = make_xcolt(a, base_role ? -1 : ji, xj, terms ? tc : nullptr);
        // The long part of an item - its dynamics term, or the whole value of a row item - does not depend on
        // the base products: the first FZ_ROUNDS items of every column are evaluated while the service
        // wavefront is still in its chain; only the subtraction from the product waits for it.
        double tv[FZ_ROUNDS];
        int trow[FZ_ROUNDS], tyo[FZ_ROUNDS];
#pragma unroll
        for (int r = 0; r < FZ_ROUNDS; ++r) {
            const int e = coli.x + wave + r * FZ_ITEM_WAVES;
            tv[r] = 0.0, trow[r] = 0, tyo[r] = -1;
            if (e < coli.y) {
                const int4 it = r == 0 ? item : OGT_ELEM[e];
                tv[r] = OgGen::item_tail(it.x, it.y, it.z, xa, a.cvec, &trow[r], &tyo[r]);
            }
        }
        lds_count_wait(&s_sync[1], 1);
        FZ_STAMP(3);
#pragma unroll
        for (int r = 0; r < FZ_ROUNDS; ++r) {
            const double v = tyo[r] >= 0 ? t.yb[tyo[r] - y0_first] - tv[r] : tv[r];
            const double v0 = __shfl_down(v, FZ_COLS);
            const int e = coli.x + wave + r * FZ_ITEM_WAVES;
            if (!base_role && e < coli.y) {
                const double q = (v - v0) / dx;
                jrow[trow[r]] = q;
                if (pcol) pcol[e] = q;
            }
        }
        // item_value indexes y0 by slot offset + node; the accessor turns that into the LDS tile
        const XColL xl{a.x0, base_role ? -1 : ji, xj, a.y0 + y0_first, t.yb};
        for (int e = coli.x + wave + FZ_ROUNDS * FZ_ITEM_WAVES; e < coli.y; e += FZ_ITEM_WAVES)
            eval_item_paired(a, OGT_ELEM[e], xl, base_role, dx, jrow, pcol ? pcol + e : nullptr);
    }
    FZ_STAMP(4);
    FZ_TRACE_OUT(a);
}

// One part of a heavy column (a phase's final time, say: it moves every defect row of the phase): the column's
// items in ONE (defect group, node tile), served exactly like a light workgroup, or its row items (no tile).
// A slot = up to 32 items with the same code (one output over the tile's nodes / one row group): lanes 0..31 at
// x0 + h e_j, lanes 32..63 the same items at x0, one wavefront per slot.
__device__ __forceinline__ void fz_heavy_part(const ogk_args& a, const int pidx, double* lds) {
    __shared__ int s_sync[2];           // as in fz_light_body
    FZ_TRACE_DECL(2);
    const ogt_int8 rec = OGT_HPART[pidx];      // {column, slots begin, end, y0 offset, node tile, first slot, slots, nodes | phase << 20}
    const int j = rec.v[0];
    if (j < a.col_lo || j >= a.col_hi) return;
    fz_sync_reset(s_sync, 2);
    const int y0_first = rec.v[3], nt = rec.v[4], mv0 = rec.v[5], nmv = rec.v[6];
    const int N = rec.v[7] & 0xfffff, phase = (rec.v[7] >> 20) & 0x3ff;
    const bool terms = TERM_CACHE && ((rec.v[7] >> 30) & 1) != 0;
    double* tc = lds + FZ_TILE_DOUBLES;
    const bool has_tile = nmv > 0;
    const int tid = (int)threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const bool service = wave == SWEEP_WAVES - 1;
    const FzTile t = fz_tile_lds(lds);
    const double xb = a.x0[j];
    const double hh = a.h[j];
    const int il = lane & 31;
    const bool base_role = lane >= 32;
    int4 slot = make_int4(0, 0, 0, 0), item = make_int4(0, 0, 0, 0);
    const bool has_slot = !service && rec.v[1] + wave < rec.v[2];
    if (has_slot) {
        slot = OGT_HSLOT[rec.v[1] + wave];
        item = OGT_HELEM[slot.x + (il < slot.y ? il : 0)];
    }
    if (has_tile) fz_stage_operands(a, t, mv0, nmv, N, &s_sync[0]);
    if (terms) {
        fill_terms<SWEEP_THREADS>(a, tc);
        lds_barrier();
    }
    FZ_STAMP(1);
    if (service) {
        if (has_tile) FZ_STAMP_SET(1, fz_service_tile(a, t, nt, nmv, N, phase, &s_sync[0]));
        FZ_STAMP(2);
        if (lane == 0) lds_count_up(&s_sync[1]);
        FZ_TRACE_OUT(a);
        return;
    }
    if (has_slot) {
        const double xj = xb + hh;
        const double dx = xj - xb;
        double* jrow = a.jt + (long)(j - a.col_lo) * OgGen::M;
        double* pcol = a.pvals ? a.pvals + a.poff[j] : nullptr;
        const XColT xa = make_xcolt(a, base_role ? -1 : j, xj, terms ? tc : nullptr);
        // as in the light workgroups: the items' long chains run while the service wavefront is in its own
        for (int s0 = rec.v[1] + wave; s0 < rec.v[2]; s0 += FZ_ROUNDS * FZ_ITEM_WAVES) {
            double tv[FZ_ROUNDS];
            int trow[FZ_ROUNDS], tyo[FZ_ROUNDS], cnt[FZ_ROUNDS], tpos[FZ_ROUNDS];
#pragma unroll
            for (int r = 0; r < FZ_ROUNDS; ++r) {
                const int s = s0 + r * FZ_ITEM_WAVES;
                tv[r] = 0.0, trow[r] = 0, tyo[r] = -1, cnt[r] = 0, tpos[r] = 0;
                if (s < rec.v[2]) {
                    const int4 sl = (r == 0 && s0 == rec.v[1] + wave) ? slot : OGT_HSLOT[s];
                    const int4 it = (r == 0 && s0 == rec.v[1] + wave) ? item : OGT_HELEM[sl.x + (il < sl.y ? il : 0)];
                    cnt[r] = sl.y;
                    tpos[r] = it.w;                     // the item's place among the column's packed entries
                    tv[r] = OgGen::item_tail(it.x, it.y, it.z, xa, a.cvec, &trow[r], &tyo[r]);
                }
            }
            if (s0 == rec.v[1] + wave) {
                lds_count_wait(&s_sync[1], 1);
                FZ_STAMP(3);
            }
#pragma unroll
            for (int r = 0; r < FZ_ROUNDS; ++r) {
                const double v = tyo[r] >= 0 ? t.yb[tyo[r] - y0_first] - tv[r] : tv[r];
                const double v0 = __shfl_down(v, 32);
                if (!base_role && il < cnt[r]) {
                    const double q = (v - v0) / dx;
                    jrow[trow[r]] = q;
                    if (pcol) pcol[tpos[r]] = q;
                }
            }
        }
    }
    FZ_STAMP(4);
    FZ_TRACE_OUT(a);
}

// MFMA tiles of the fused launch.  Workgroup = (collocation slot, node tile, up to SWEEP_WAVES - 1 column
// tiles): wavefront w < nct owns the (16 perturbed columns) x (16 nodes) tile of column tile ct0 + w - one
// accumulator, its MFMA chain and, on the diagonal tile only, the perturbed dynamics term.  What every column
// tile of the node tile shares - the base product and the base dynamics term of the 16 nodes - is computed
// ONCE per workgroup by the last wavefront (and the one before it when it is free), in parallel, and handed
// over through LDS; the column wavefronts meet it only at their epilogue.  No barrier but fz_sync_reset's: the slot's
// operand vector xt[NP] is put into LDS by the last wavefront (which needs it first and has nothing else to do) and,
// beyond 64 operands, by the first ones, 64 operands each, and counted in; only the wavefronts that run a chain wait for
// that count - with the panel, their own samples of x0 and h and their own perturbed operand already asked for - while
// the wavefronts that compute the dynamics terms, the longest chains of the workgroup, start at once.
__device__ __forceinline__ void fz_tile_body(const ogk_args& a, const int bx, double* lds) {
    __shared__ int s_flags[4];          // [0] base products of the node tile, [1] base dynamics terms, [2] diagonal terms,
                                        // [3] wavefronts whose part of the operand vector is in LDS
    FZ_TRACE_DECL(3);
    fz_sync_reset(s_flags, 4);
    const int4 tile = OGT_FTILE[bx];                   // {slot, first column tile, node tile, column tiles}
    const int slot = tile.x, ct0 = tile.y, nt = tile.z, nct = tile.w;
    const ogt_int8 rec = OGT_SLOT[slot];
    const int N = rec.v[0], leaf = rec.v[2], row0 = rec.v[3];
    const bool diag = rec.v[6] & 1, generic = rec.v[6] & 2;
    const int dep0 = rec.v[7] >> 12, ndep = rec.v[7] & 0xfff;
    const int KS = (N + 3) >> 2;
    const int tid = (int)threadIdx.x;
    const int wave = tid >> 6, lane = tid & 63, lk = lane >> 4, kk = lane & 15;
    double* xt = lds;                                   // [NP] the slot's operand vector
    double* yb = lds + FZ_NP;                           // [16] base products of the node tile
    double* tb = yb + 16;                               // [16] base dynamics terms
    double* td = tb + 16;                               // [16] dynamics terms with the node's own sample perturbed
    const XCol xbase{a.x0, -1, 0.0};
    const int k = nt * 16 + kk;                         // output node of this lane
    const bool k_on = k < N;
    const double* bsrc = a.dfrag + OgGen::DFRAG_OFF(rec.v[5]) + (long)nt * KS * 64 + lane;
    constexpr int CH = 10;                              // k-steps per chunk
    const int prod_wave = SWEEP_WAVES - 1;
    const int term_wave = nct < SWEEP_WAVES - 1 ? SWEEP_WAVES - 2 : SWEEP_WAVES - 1;
    // the diagonal column tile (perturbed node = output node) also needs the dynamics term at x0 + h e_j for its
    // 16 (node, own sample) pairs: a third free wavefront takes that chain off the column wavefront's path
    const bool diag_here = diag && nt >= ct0 && nt < ct0 + nct;
    const int diag_wave = nct < SWEEP_WAVES - 2 ? SWEEP_WAVES - 3 : -1;
    const bool col_wave = wave < nct;
    const int l0 = (ct0 + wave) * 16;                   // first slice offset of a column wavefront's tile
    const bool col_on = col_wave && !(l0 >= N || leaf + l0 >= a.col_hi || leaf + l0 + 16 <= a.col_lo);
    const int la = l0 + kk;                             // A-operand row of this lane
    const bool a_on = col_on && la < N;
    double b0[CH], b1[CH], xbv[4], hv[4], xa_b = 0.0, xa_h = 0.0;
    if (col_on || wave == prod_wave) fz_load_first<CH>(bsrc, KS, b0, b1);
    if (col_on) {
        xa_b = a.x0[a_on ? leaf + la : leaf];
        xa_h = a.h[a_on ? leaf + la : leaf];
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) {
            const int lc = l0 + lk + 4 * reg;
            const int jj = leaf + ((k_on && lc < N) ? lc : 0);
            xbv[reg] = a.x0[jj];
            hv[reg] = a.h[jj];
        }
    }
    const int NP = KS << 2, stage_l = (((wave + 1) & (SWEEP_WAVES - 1)) << 6) + lane;     // wavefront 7, 0, 1, ...
    const int n_stage = (NP + 63) >> 6 < SWEEP_WAVES ? (NP + 63) >> 6 : SWEEP_WAVES;
    if (stage_l - lane < NP) {
        for (int l = stage_l; l < NP; l += SWEEP_THREADS)
            xt[l] = l < N ? OgGen::mv_operand(slot, l, xbase, a.cvec) : 0.0;
        if (lane == 0) lds_count_up(&s_flags[3]);
    }
    double hit_v = 0.0;
    if (a_on) {
        const XCol xa{a.x0, leaf + la, xa_b + xa_h};
        hit_v = OgGen::mv_operand(slot, la, xa, a.cvec);
    }
    if (col_on || wave == prod_wave) lds_count_wait(&s_flags[3], n_stage);
    FZ_STAMP(1);
    if (!col_wave) {
        if (wave == diag_wave) {
            if (diag_here && lk == 0 && k_on && leaf + k >= a.col_lo && leaf + k < a.col_hi) {
                const int jd = leaf + k;
                const double xbd = a.x0[jd];
                const XCol xd{a.x0, jd, xbd + a.h[jd]};
                td[kk] = OgGen::tail_one(slot, k, xd, a.cvec);
            }
            if (lane == 0) lds_count_up(&s_flags[2]);
        }
        if (wave == term_wave && lk == 0) tb[kk] = k_on ? OgGen::tail_one(slot, k, xbase, a.cvec) : 0.0;
        if (wave == term_wave && lane == 0) lds_count_up(&s_flags[1]);
        if (wave == prod_wave) {
            const v4f64 accb = fz_chain<CH>(bsrc, KS, b0, b1, [&](const int ks) {
                const double v = xt[(ks < KS ? ks : 0) * 4 + lk];
                return ks < KS ? v : 0.0;
            });
            if (lk == 0) yb[kk] = accb[0];              // every row of accb holds the base product of node k
            FZ_STAMP(2);
            if (lane == 0) lds_count_up(&s_flags[0]);
        }
        FZ_TRACE_OUT(a);
        return;
    }
    if (!col_on) return;
    const int row = row0 + (k_on ? k : 0);
    // the perturbed dynamics term on the diagonal
    double t_diag = 0.0;
    bool have_diag = false;
    {
        const int lc = k;                                // column whose perturbed node is k
        const int reg = (lc - l0 - lk) >> 2;
        have_diag = diag && k_on && lc >= l0 + lk && ((lc - l0 - lk) & 3) == 0 && reg < 4 && lc < N &&
                    leaf + lc >= a.col_lo && leaf + lc < a.col_hi;
        if (have_diag && diag_wave < 0) {               // no free wavefront in this workgroup: own chain
            const int jd = leaf + lc;
            const double xbd = a.x0[jd];
            const XCol xd{a.x0, jd, xbd + a.h[jd]};
            t_diag = OgGen::tail_one(slot, k, xd, a.cvec);
        }
    }
    const v4f64 acc = fz_chain<CH>(bsrc, KS, b0, b1, [&](const int ks) {
        const int l = (ks < KS ? ks : 0) * 4 + lk;
        const double v = xt[l];
        return ks < KS ? (l == la ? hit_v : v) : 0.0;
    });
    FZ_STAMP(2);
    lds_count_wait(&s_flags[1], 1);
    lds_count_wait(&s_flags[0], 1);
    if (diag_wave >= 0 && l0 == nt * 16) {              // (the diagonal tile: wavefront-uniform)
        lds_count_wait(&s_flags[2], 1);
        if (have_diag) t_diag = td[kk];
    }
    FZ_STAMP(3);
    if (!k_on) return;
    const double t_base = tb[kk];
    const double f_base = yb[kk] - t_base;
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) {
        const int lc = l0 + lk + 4 * reg;
        const int j = leaf + lc;
        if (lc >= N || j < a.col_lo || j >= a.col_hi) continue;
        const double xj = xbv[reg] + hv[reg];
        const double dx = xj - xbv[reg];
        double t = (have_diag && lc == k) ? t_diag : t_base;
        if (generic) {
            bool reads = diag && k == lc;
            for (int d = dep0; d < dep0 + ndep; ++d) {
                const int kind = OgGen::DEP_KIND(d), base_d = OgGen::DEP_BASE(d);
                reads = reads || (kind == 1 ? (base_d + k == j)
                                            : (j >= base_d && j < base_d + OgGen::DEP_CNT(d)));
            }
            if (reads) {
                const XCol xg{a.x0, j, xj};
                t = OgGen::tail_one(slot, k, xg, a.cvec);
            }
        }
        const double val = acc[reg] - t;
        const double q = (val - f_base) / dx;
        a.jt[(long)(j - a.col_lo) * OgGen::M + row] = q;
        if (a.pvals) a.pvals[a.poff[j] + k] = q;        // the column's own block leads its packed entries
    }
    FZ_STAMP(4);
    FZ_TRACE_OUT(a);
}

// At least four wavefronts per SIMD = two workgroups per compute unit = 512 resident workgroups: a problem whose
// callbacks bring the kernel to 129 registers (C5 since round 4) would otherwise run ONE workgroup per compute unit and
// start half of its workgroups microseconds late.  Kernels that need fewer registers (84 at C3) are not affected: the
// attribute is a floor on the occupancy the register allocator must leave possible.
#ifndef OGK_FUSED_ATTR
#define OGK_FUSED_ATTR __attribute__((amdgpu_waves_per_eu(4)))
#endif
#ifdef OGK_HAS_FUSED
__global__ __launch_bounds__(SWEEP_THREADS) OGK_FUSED_ATTR void ogk_fused(const ogk_args a, const int ndef, const int n_eval,
                                                           const int group_lo, const int n_light, const int sum_lo,
                                                           const int n_sum) {
    extern __shared__ __attribute__((aligned(16))) double lds[];
#include "ogk_fused_workgroup.inc"
}
#endif

// ------------------------------------------------------------------------------------------
// Modes 11 - 13 (the batch part, ogk.h: ogk_batch_args): B points of the problem in one launch.  blockIdx.y is the
// lane, blockIdx.x means what it means in ogk_fused / ogk_eval, and the workgroup runs the same device functions on
// the lane's record - so a lane's results are the single-point path's, bit for bit.  Nothing in the one-launch form
// waits for another workgroup (finish_eval takes a ticket), so the grid needs no co-residency: lanes beyond one round
// of residency start later.  The records stay where they are, in the table: the workgroup reads the fields it uses
// through the constant address space (scalar loads, as it reads a launch's argument block) - a copy of a 500-byte
// record in registers would cost the occupancy the amdgpu_waves_per_eu floor is there for.
// ------------------------------------------------------------------------------------------
#if defined(OGK_HAS_BATCH) || defined(OGK_HAS_BATCH_EXACT) || defined(OGK_HAS_PAR) || defined(OGK_HAS_DIR) || \
    defined(OGK_HAS_ADJ) || defined(OGK_HAS_HVP) || defined(OGK_HAS_MIX) || defined(OGK_HAS_HESS) || defined(OGK_HAS_PP)
typedef const ogk_args __attribute__((address_space(4))) * ogk_lane_table;
__device__ __forceinline__ const ogk_args& batch_lane(const ogk_args* lanes) {
    // (written by the host when the batch was created and by ogk_batch_bind in an earlier launch; never by this one)
    return *(const ogk_args*)((ogk_lane_table)lanes + blockIdx.y);
}
#endif

#ifdef OGK_HAS_BATCH
__global__ __launch_bounds__(SWEEP_THREADS) OGK_FUSED_ATTR void ogk_fused_batch(const ogk_args* __restrict__ lanes,
                                                                 const int ndef, const int n_eval, const int group_lo,
                                                                 const int n_light, const int sum_lo, const int n_sum) {
    extern __shared__ __attribute__((aligned(16))) double lds[];
    const ogk_args& a = batch_lane(lanes);
#include "ogk_fused_workgroup.inc"
}

__global__ __launch_bounds__(SWEEP_THREADS) void ogk_eval_batch(const ogk_args* __restrict__ lanes, const int ndef) {
    extern __shared__ __attribute__((aligned(16))) double lds[];
    const ogk_args& a = batch_lane(lanes);
    const int id = (int)blockIdx.x;
    if (id == 0 && threadIdx.x == 0) {                  // as ogk_eval (a lane's nonfinite_next is a word nobody reads:
                                                        // ogk_batch_bind zeroes the counter ahead of this launch)
        *a.nonfinite_next = 0;
        if (a.jt_bump) __hip_atomic_store(a.jt_launches, *a.jt_launches + 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    if (id < ndef) eval_defect_body<false>(a, id, lds);
    else eval_rows_body<false>(a, id - ndef, lds);
}

// where this call's arrays are: one thread per record of the table (every lane of every set: a later launch may run
// more lanes of the same arrays); the lanes an evaluation is about to run get their non-finite counter zeroed
__global__ void ogk_batch_bind(const ogk_batch_args b) {
    const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (i >= OGK_BATCH_SETS * b.capacity) return;
    const int k = i % b.capacity;
    ogk_args& a = b.lanes[i];
    a.x0 = b.X + (long)k * OgGen::N_VAR;
    a.h = b.H ? b.H + (long)k * OgGen::N_VAR : nullptr;
    a.f0 = b.F0 + (long)k * OgGen::M;
    a.pvals = b.vals ? b.vals + (long)k * b.nnz : nullptr;
    if (i / b.capacity == b.clear_set && k < b.count) *a.nonfinite = 0;
}
#endif

// ------------------------------------------------------------------------------------------
// Mode 14, OGK_BATCH_EXACT (the exact batch part, OGK_PART_BATCH_EXACT): ogk_exact_struct for B points in one launch,
// lane = blockIdx.y.  Per column it computes what ogk_exact_struct computes - every entry by one thread from x0, y0, cvec and dfrag alone, so
// who computes an entry cannot change a bit of it - and also stores each value at its place of the lane's packed array
// (pattern order: the own block's row k is entry k, item e is entry own + (e - first item)), so no pack launch follows.
// Mapping: a column has a few dozen entries, a phase's final time a thousand.  The columns the tracer marked heavy
// (HEAVY_FLAG, OGT_HEAVY: longest first) get a workgroup each and lead the grid; every other column gets ONE wavefront,
// four columns per workgroup - a workgroup per column would leave three of four wavefronts without work on almost
// every column and make the grid four times as long, times B.
// ------------------------------------------------------------------------------------------
#ifdef OGK_HAS_BATCH_EXACT
constexpr int XB_THREADS = 256;
constexpr int XB_COLS = XB_THREADS / 64;            // ordinary columns per workgroup: one per wavefront

// column j by the `width` threads that share it; t = this thread's index among them.  (One copy of the callbacks'
// dual-number code for both widths: it is what the part's build time and the kernel's registers consist of.)
__device__ __forceinline__ void exact_column(const ogk_args& a, const int j, const int t, const int width) {
    double* jrow = a.jt + (long)j * OgGen::M;
    const XDual xd{a.x0, j};
    const int4 rec = OGT_COL[j];
    const int own_lo = rec.z, own_hi = rec.w & ~HEAVY_FLAG;
    double* pcol = a.pvals ? a.pvals + a.poff[j] : nullptr;
    double* pitem = pcol ? pcol + (own_hi - own_lo) - rec.x : nullptr;
    for (int e = rec.x + t; e < rec.y; e += width) {
        const int4 it = OGT_ELEM[e];
        int row;
        const ogdual v = OgGen::item_value(it.x, it.y, it.z, xd, a.y0, a.cvec, &row);
        jrow[row] = v.d;
        if (pitem) pitem[e] = v.d;
    }
    if (own_hi > own_lo) {
        // x_j is node l of the state behind one collocation product
        int si = -1, l = 0;
        for (int s = 0; s < OgGen::N_MV; ++s) {
            const int leaf = OGT_SLOT[s].v[2], len = OGT_SLOT[s].v[0];
            if (j >= leaf && j < leaf + len) {
                si = s;
                l = j - leaf;
            }
        }
        if (si >= 0) {
            const int N = OGT_SLOT[si].v[0], phase = OGT_SLOT[si].v[5], row0 = OGT_SLOT[si].v[3];
            const int reads = OGT_SLOT[si].v[6];            // (bits as in ogk_exact_struct)
            const ogdual op = OgGen::mv_operand(si, l, xd, a.cvec);
            for (int k = t; k < N; k += width) {
                double v = __builtin_fma(op.d, dfrag_entry(a, phase, N, k, l), 0.0);
                if ((reads & 2) || ((reads & 1) && k == l)) v = v - OgGen::tail_one(si, k, xd, a.cvec).d;
                jrow[row0 + k] = v;
                if (pcol) pcol[row0 - own_lo + k] = v;
            }
        }
    }
}

__global__ __launch_bounds__(XB_THREADS) void ogk_exact_struct_batch(const ogk_args* __restrict__ lanes) {
    const ogk_args& a = batch_lane(lanes);
    const int id = (int)blockIdx.x, tid = (int)threadIdx.x;
    const bool heavy = id < OgGen::N_HEAVY;
    // heavy: the workgroup's column; else the wavefront's (none past the end, and the heavy ones have their own)
    // (the same in all 64 lanes of a wavefront - said to the compiler, so that the column's tables stay scalar loads)
    int j = heavy ? OGT_HEAVY[id] : (id - OgGen::N_HEAVY) * XB_COLS + __builtin_amdgcn_readfirstlane(tid >> 6);
    if (!heavy && (j >= OgGen::N_VAR || (OGT_COL[j].w & HEAVY_FLAG))) j = -1;
    if (jt_needs_fill(a)) {                     // the same for every workgroup of the lane
        if (j >= 0) {
            double* jrow = a.jt + (long)j * OgGen::M;
            if (heavy) for (int r = tid; r < OgGen::M; r += XB_THREADS) jrow[r] = 0.0;
            else for (int r = tid & 63; r < OgGen::M; r += 64) jrow[r] = 0.0;
        }
        __syncthreads();                        // the zeros of a row before its entries
    }
    if (j < 0) return;
    exact_column(a, j, heavy ? tid : (tid & 63), heavy ? XB_THREADS : 64);
}
#endif

// ------------------------------------------------------------------------------------------
// Modes 15 and 16 (the parameter part, OGK_PART_PAR): exact dF/dtheta for the run-time parameters, dF[n_par][m] dense
// and row-major.  blockIdx.y is the parameter, one workgroup per (parameter, lane): it zero-fills row kp of dF - all m
// doubles, every call; the result is small - and then its threads run over the parameter's work lists (the generated
// header's parameter section), one thread per entry: og_par_entry (og_par.h, the source a host probe shares) computes an
// entry from x0, y0, cvec and the D image alone, so the mapping cannot change a bit of it.  y0 is the evaluation's
// (OGK_EVAL / OGK_BATCH_EVAL before this launch on the same stream).  The parameter index is the workgroup's, so the
// ranges of its work lists are scalar loads; a parameter nothing reads is a fill and nothing else.
// ------------------------------------------------------------------------------------------
#if defined(OGK_HAS_PAR) && defined(OG_GEN_HAS_PAR)
#include "og_par.h"
constexpr int PAR_THREADS = 256;

__device__ __forceinline__ void exact_par_row(const ogk_args& a, double* dF) {
    const int kp = (int)blockIdx.y, tid = (int)threadIdx.x;
    double* drow = dF + (long)kp * OgGen::M;
    for (int r = tid; r < OgGen::M; r += PAR_THREADS) drow[r] = 0.0;
    __syncthreads();                            // (every thread of the workgroup: the zeros of the row before its entries)
    const int entries = OgGen::PAR_ENTRIES(kp);
    for (int e = tid; e < entries; e += PAR_THREADS) {
        int row;
        const double v = og_par_entry<OgGen>(kp, e, a.x0, a.y0, a.cvec, a.dfrag, &row);
        drow[row] = v;
    }
}

__global__ __launch_bounds__(PAR_THREADS) void ogk_exact_par(const ogk_args a) { exact_par_row(a, a.jt); }

// the same on a lane's record (blockIdx.z: the lane; its own cvec gives every lane its own theta); the lane's dF is
// where OGK_BATCH_BIND put the record's pvals
__global__ __launch_bounds__(PAR_THREADS) void ogk_exact_par_batch(const ogk_args* __restrict__ lanes) {
    const ogk_args& a = *(const ogk_args*)((ogk_lane_table)lanes + blockIdx.z);
    exact_par_row(a, a.pvals);
}
#endif

// ------------------------------------------------------------------------------------------
// Modes 17 and 18 (the directional part, OGK_PART_DIR): exact directional derivatives F'(x) v, [m] doubles per
// direction, every entry by the functions of og_dir.h that a host probe shares (og_dir_entry there is these pieces in
// one thread): an entry is computed by ONE thread from x0, v, y0, cvec and the D image, no reduction across threads, so
// the mapping cannot change a bit of it.  Every row of F belongs to exactly one entry: there is no fill, and no entry
// is written twice.  y0 is the evaluation's (OGK_EVAL / OGK_BATCH_EVAL before this launch on the same stream).
// Mapping along blockIdx.x, 256 threads per workgroup:
//   - first the row groups, one WAVEFRONT per (group, 64 elements): a wavefront runs one group's code, not one after
//     the other of every group its 64 entries happen to span (the head of F is dozens of groups of one row each, and
//     each is a chain of dependent loads);
//   - then one workgroup per (defect group, collocation slot): its threads first put the N operand derivatives
//     d(operand_l)/dv into LDS, one each, and after the barrier thread k runs the row's fma chain over them - the same
//     doubles in the same order as the probe's chain, which evaluates them in place.  Measured without the staging (every
//     thread evaluating the N operands inside its chain, a load behind a switch per step): 18 / 60 / 188 us for the
//     kernel at N = 50 / 80 / 128 (C2 / C3 / C5).
// ------------------------------------------------------------------------------------------
#ifdef OGK_HAS_DIR
#include "og_dir.h"
constexpr int DIR_THREADS = 256;
constexpr int DIR_WAVES = DIR_THREADS / 64;

// workgroups of the row groups (DIR_WAVES wavefront units each), and (defect group, slot) units
inline int dir_row_blocks() {
    int waves = 0;
    for (int g = 0; g < OgGen::N_GROUPS; ++g)
        if (OgGen::G_KIND(g) == 0) waves += (OgGen::G_LEN(g) + 63) >> 6;
    return (waves + DIR_WAVES - 1) / DIR_WAVES;
}
inline int dir_defect_units() {
    int units = 0;
    for (int g = 0; g < OgGen::N_GROUPS; ++g)
        if (OgGen::G_KIND(g) == 1) units += OgGen::G_NMV(g);
    return units;
}

__device__ __forceinline__ void exact_dir_block(const ogk_args& a, const double* v, double* dF, const int row_blocks) {
    __shared__ double opd[OgGen::MAX_NODES];
    const int bx = (int)blockIdx.x, tid = (int)threadIdx.x;
    const OgDirX xd{a.x0, v};
    if (bx < row_blocks) {
        // (the same in all 64 lanes of a wavefront - said to the compiler, so that the group's tables stay scalar loads)
        int w = __builtin_amdgcn_readfirstlane(bx * DIR_WAVES + (tid >> 6));
        for (int g = 0; g < OgGen::N_GROUPS; ++g) {
            if (OgGen::G_KIND(g) != 0) continue;
            const int len = OgGen::G_LEN(g), nw = (len + 63) >> 6;
            if (w >= nw) {
                w -= nw;
                continue;
            }
            const int k = w * 64 + (tid & 63);
            if (k < len) {
                int row;
                const double d = OgGen::item_value(g, 0, k, xd, a.y0, a.cvec, &row).d;
                dF[row] = d;
            }
            return;
        }
        return;                                     // (a wavefront past the last group)
    }
    int u = bx - row_blocks;                        // the same for the whole workgroup: every thread reaches the barrier
    for (int g = 0; g < OgGen::N_GROUPS; ++g) {
        if (OgGen::G_KIND(g) != 1) continue;
        const int nmv = OgGen::G_NMV(g);
        if (u >= nmv) {
            u -= nmv;
            continue;
        }
        const int N = OgGen::G_LEN(g), slot = OgGen::G_MV0(g) + u;
        for (int l = tid; l < N; l += DIR_THREADS) opd[l] = og_dir_operand<OgGen>(slot, l, xd, a.cvec);
        __syncthreads();
        for (int k = tid; k < N; k += DIR_THREADS) {
            int row;
            const double d = og_dir_defect<OgGen>(g, u, k, [&](const int l) { return opd[l]; }, xd, a.cvec, a.dfrag, &row);
            dF[row] = d;
        }
        return;
    }
}

// blockIdx.y: the direction, read at h + d * n, written to jt + d * m
__global__ __launch_bounds__(DIR_THREADS) void ogk_exact_dir(const ogk_args a, const int row_blocks) {
    const long d = (long)blockIdx.y;
    exact_dir_block(a, a.h + d * OgGen::N_VAR, a.jt + d * OgGen::M, row_blocks);
}

// the same on a lane's record (blockIdx.z: the lane, as in ogk_exact_par_batch): one direction per lane - the record's
// h - and the result where OGK_BATCH_BIND put the record's pvals
__global__ __launch_bounds__(DIR_THREADS) void ogk_exact_dir_batch(const ogk_args* __restrict__ lanes, const int row_blocks) {
    const ogk_args& a = *(const ogk_args*)((ogk_lane_table)lanes + blockIdx.z);
    exact_dir_block(a, a.h, a.pvals, row_blocks);
}
#endif

// ------------------------------------------------------------------------------------------
// Modes 19 and 20 (the adjoint part, OGK_PART_ADJ): exact adjoint products g = F'(x)^T w, [n] doubles per weight vector.
// g_j is the sum that og_adj.h defines: the entries ogk_exact_struct writes for column j (og_adj_term), each times the
// weight of its row, in 256 strided fma chains and the tree of og_adj_tree.  A thread computes a dual-number entry ONCE
// and applies it to every weight vector of its chunk (ADJ_CHUNK of them: their partial sums are its registers), so K
// vectors do not repeat the forward-mode work.  The 64 chains [64 q, 64 q + 64) are the 64 lanes of a wavefront: the
// tree's levels s = 32 .. 1 are a shuffle-down reduction (adj_block_sums), and what is left is (p0 + p1) + (p2 + p3) of
// the four blocks.  WHO runs block q does not enter the result, so the mapping follows ogk_exact_struct_batch:
//   - a column the tracer marked heavy (HEAVY_FLAG, OGT_HEAVY: longest first; a final time has a thousand terms) gets a
//     workgroup, wavefront q runs block q, the four sums meet in LDS; these workgroups lead the grid;
//   - every other column has a few dozen terms (at most a state's own N defect rows and its row items) and gets ONE
//     wavefront, four columns per workgroup, which runs the four blocks one after the other - a block past the last term
//     is +0.0 without any work; no LDS, no barrier.  Measured with a workgroup per column for all of them (three of four
//     wavefronts idle on almost every column, the grid four times as long): 9.0 / 23.9 / 347 us per call at C2 / C3 / C5
//     and 33 / 255 / 6270 us for 32 lanes, twice the batched exact Jacobian.
// The result is the host probe's (og_adj_entry) bit for bit whatever the scheduling, and vector d of K is the call with
// that vector alone.  Every g_j of every vector is written, +0.0 for a column without terms; nothing else is: no J_T,
// no fill, no jt_state / jt_launches word.  y0 is the evaluation's (OGK_EVAL / OGK_BATCH_EVAL before this launch on the
// same stream).  The column is the workgroup's or the wavefront's, so its records and the slot table stay scalar loads.
// ------------------------------------------------------------------------------------------
#ifdef OGK_HAS_ADJ
#include "og_adj.h"
constexpr int ADJ_THREADS = OG_ADJ_CHAINS;
constexpr int ADJ_WAVES = ADJ_THREADS / 64;
constexpr int ADJ_CHUNK = 8;            // weight vectors per chunk: 16 VGPRs of partial sums per thread
static_assert(ADJ_WAVES == 4 && ADJ_CHUNK <= 64, "og_adj_tree combines four blocks of 64 chains");

struct AdjTables {
    __device__ __forceinline__ int4 col(const int j) const { return OGT_COL[j]; }
    __device__ __forceinline__ int4 elem(const int e) const { return OGT_ELEM[e]; }
    __device__ __forceinline__ const ogt_int8& slot(const int s) const { return OGT_SLOT[s]; }
};

inline int adj_grid() { return OgGen::N_HEAVY + (OgGen::N_VAR + ADJ_WAVES - 1) / ADJ_WAVES; }

// Block q = chain >> 6 of column j for the kc vectors of a chunk, by the 64 lanes of one wavefront (chain: this lane's):
// the chains (og_adj_chain, every entry applied to all vectors), then the levels s = 32 .. 1 of og_adj_tree -> r[d],
// valid in lane 0 (lane i of level s needs lane i + s < 2 s <= 64 only; what the lanes above compute is never used).
// kc and q are the same in all lanes.
__device__ __forceinline__ void adj_block_sums(const ogk_args& a, const AdjTables& tab, const OgAdjCol& c, const int j,
                                               const double* w, const int kc, const int chain, double* r) {
#pragma unroll
    for (int d = 0; d < ADJ_CHUNK; ++d) r[d] = 0.0;
    if ((chain & ~63) >= c.terms) return;           // (no chain of the block has a term: +0.0 all the way up the tree)
    for (int t = chain; t < c.terms; t += OG_ADJ_CHAINS) {
        int row;
        const double e = og_adj_term<OgGen>(tab, c, j, t, a.x0, a.y0, a.cvec, a.dfrag, &row);
#pragma unroll
        for (int d = 0; d < ADJ_CHUNK; ++d)
            if (d < kc) r[d] = __builtin_fma(w[(long)d * OgGen::M + row], e, r[d]);
    }
#pragma unroll
    for (int d = 0; d < ADJ_CHUNK; ++d)
        if (d < kc) {
#pragma unroll
            for (int s = 32; s >= 1; s >>= 1) r[d] = r[d] + __shfl_down(r[d], s, 64);
        }
}

// w: the chunk's first weight vector (the next at w + M), g: row 0 of its part of the result (the next at g + N_VAR),
// kc: the chunk's vectors, 1 .. ADJ_CHUNK.  blockIdx.x: heavy columns first, then four light columns per workgroup.
__device__ __forceinline__ void exact_adj_block(const ogk_args& a, const double* w, double* g, const int kc) {
    __shared__ double part[ADJ_CHUNK][ADJ_WAVES];
    const int id = (int)blockIdx.x, tid = (int)threadIdx.x;
    // (the same in all 64 lanes of a wavefront - said to the compiler, so that the column's tables stay scalar loads)
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const AdjTables tab;
    double r[ADJ_CHUNK];
    if (id < OgGen::N_HEAVY) {                      // the whole workgroup: every thread reaches the barrier
        const int j = OGT_HEAVY[id];
        const OgAdjCol c = og_adj_col<OgGen>(tab, j, a.x0, a.cvec);
        adj_block_sums(a, tab, c, j, w, kc, tid, r);
        if ((tid & 63) == 0) {
#pragma unroll
            for (int d = 0; d < ADJ_CHUNK; ++d) part[d][wave] = r[d];
        }
        __syncthreads();
        if (tid < kc) g[(long)tid * OgGen::N_VAR + j] = (part[tid][0] + part[tid][1]) + (part[tid][2] + part[tid][3]);
        return;
    }
    const int j = (id - OgGen::N_HEAVY) * ADJ_WAVES + wave;
    if (j >= OgGen::N_VAR || (OGT_COL[j].w & HEAVY_FLAG)) return;   // (the whole wavefront; a heavy column has its own)
    const OgAdjCol c = og_adj_col<OgGen>(tab, j, a.x0, a.cvec);
    const int lane = tid & 63;
    double s[ADJ_CHUNK], u[ADJ_CHUNK];
    // (p0 + p1) + (p2 + p3): s = p0, s += p1, u = p2, s += u + p3
#pragma unroll 1
    for (int q = 0; q < ADJ_WAVES; ++q) {
        adj_block_sums(a, tab, c, j, w, kc, q * 64 + lane, r);
#pragma unroll
        for (int d = 0; d < ADJ_CHUNK; ++d) {
            if (q == 0) s[d] = r[d];
            else if (q == 1) s[d] = s[d] + r[d];
            else if (q == 2) u[d] = r[d];
            else s[d] = s[d] + (u[d] + r[d]);
        }
    }
    if (lane == 0) {
#pragma unroll
        for (int d = 0; d < ADJ_CHUNK; ++d)
            if (d < kc) g[(long)d * OgGen::N_VAR + j] = s[d];
    }
}

// blockIdx.y: the chunk of the K = nw weight vectors, read at h + d * m, written to jt + d * n
__global__ __launch_bounds__(ADJ_THREADS) void ogk_exact_adj(const ogk_args a, const int nw) {
    const int d0 = (int)blockIdx.y * ADJ_CHUNK;
    const int kc = nw - d0 < ADJ_CHUNK ? nw - d0 : ADJ_CHUNK;
    exact_adj_block(a, a.h + (long)d0 * OgGen::M, a.jt + (long)d0 * OgGen::N_VAR, kc);
}

// the same on a lane's record (blockIdx.z: the lane): one weight vector per lane, row `lane` of W[count][m], the result
// in row `lane` of G[count][n] (the launch's own arguments: a lane record's h has the stride of a decision vector)
__global__ __launch_bounds__(ADJ_THREADS) void ogk_exact_adj_batch(const ogk_args* __restrict__ lanes, const double* W,
                                                                   double* G) {
    const long lane = (long)blockIdx.z;
    const ogk_args& a = *(const ogk_args*)((ogk_lane_table)lanes + blockIdx.z);
    exact_adj_block(a, W + lane * OgGen::M, G + lane * OgGen::N_VAR, 1);
}
#endif

// ------------------------------------------------------------------------------------------
// Modes 21 and 22 (the Hessian part, OGK_PART_HVP): exact Hessian-vector products q = grad^2 (w . F)(x) v, [n] doubles
// per pair (w, v).  q_j is the sum that og_hvp.h defines: the terms of column j that og_adj.h enumerates, each the mixed
// part of the item on second-order dual numbers (unit seed on x_j, v in the other slot), times the weight of its row, in
// the chains and the tree of og_adj.h.  The forward-mode work depends on v, so - unlike ogk_exact_adj, where a chunk of
// weight vectors shares an entry - there is nothing to share across pairs but the column lookup: one pair per grid slice
// (blockIdx.y for the K pairs of one point, blockIdx.z for the lanes of a batch).  The column mapping is
// ogk_exact_adj's: a heavy column (OGT_HEAVY) gets a workgroup, wavefront q runs block q of 64 chains and the four sums
// meet in LDS; every other column gets one wavefront, four columns per workgroup, which runs the four blocks one after
// the other.  A wavefront's 64 lanes are 64 chains and __shfl_down is the tree's levels s = 32 .. 1.  The column is the
// workgroup's or the wavefront's, so its records stay scalar loads.  Every q_j of every pair is written, +0.0 for a
// column without terms; no J_T, no jt_state / jt_launches word.  y0 is the evaluation's.
// ------------------------------------------------------------------------------------------
#ifdef OGK_HAS_HVP
#include "og_hvp.h"
constexpr int HVP_THREADS = OG_ADJ_CHAINS;
constexpr int HVP_WAVES = HVP_THREADS / 64;
static_assert(HVP_WAVES == 4, "og_adj_tree combines four blocks of 64 chains");

struct HvpTables {
    __device__ __forceinline__ int4 col(const int j) const { return OGT_COL[j]; }
    __device__ __forceinline__ int4 elem(const int e) const { return OGT_ELEM[e]; }
    __device__ __forceinline__ const ogt_int8& slot(const int s) const { return OGT_SLOT[s]; }
};

inline int hvp_grid() { return OgGen::N_HEAVY + (OgGen::N_VAR + HVP_WAVES - 1) / HVP_WAVES; }

// Block chain >> 6 of column j by the 64 lanes of one wavefront (chain: this lane's): the chain (og_hvp_chain), then the
// levels s = 32 .. 1 of og_adj_tree -> valid in lane 0 (lane i of level s needs lane i + s < 2 s <= 64 only).  A block
// past the last term is +0.0 in every lane without any work.
__device__ __forceinline__ double hvp_block_sum(const ogk_args& a, const HvpTables& tab, const OgAdjCol& c, const int j,
                                                const double* w, const double* v, const int chain) {
    double r = og_hvp_chain<OgGen>(tab, c, j, chain, w, v, a.x0, a.y0, a.cvec, a.dfrag);
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) r = r + __shfl_down(r, s, 64);
    return r;
}

// w[M], v[N_VAR]: the pair, q[N_VAR]: its result.  blockIdx.x: heavy columns first, then four light columns per
// workgroup.
__device__ __forceinline__ void exact_hvp_block(const ogk_args& a, const double* w, const double* v, double* q) {
    __shared__ double part[HVP_WAVES];
    const int id = (int)blockIdx.x, tid = (int)threadIdx.x;
    // (the same in all 64 lanes of a wavefront - said to the compiler, so that the column's tables stay scalar loads)
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const HvpTables tab;
    if (id < OgGen::N_HEAVY) {                      // the whole workgroup: every thread reaches the barrier
        const int j = OGT_HEAVY[id];
        const OgAdjCol c = og_adj_col<OgGen>(tab, j, a.x0, a.cvec);
        const double r = hvp_block_sum(a, tab, c, j, w, v, tid);
        if ((tid & 63) == 0) part[wave] = r;
        __syncthreads();
        if (tid == 0) q[j] = (part[0] + part[1]) + (part[2] + part[3]);
        return;
    }
    const int j = (id - OgGen::N_HEAVY) * HVP_WAVES + wave;
    if (j >= OgGen::N_VAR || (OGT_COL[j].w & HEAVY_FLAG)) return;   // (the whole wavefront; a heavy column has its own)
    const OgAdjCol c = og_adj_col<OgGen>(tab, j, a.x0, a.cvec);
    const int lane = tid & 63;
    double s = 0.0, u = 0.0;
    // (p0 + p1) + (p2 + p3): s = p0, s += p1, u = p2, s += u + p3
#pragma unroll 1
    for (int b = 0; b < HVP_WAVES; ++b) {
        const double r = hvp_block_sum(a, tab, c, j, w, v, b * 64 + lane);
        if (b == 0) s = r;
        else if (b == 1) s = s + r;
        else if (b == 2) u = r;
        else s = s + (u + r);
    }
    if (lane == 0) q[j] = s;
}

// blockIdx.y: the pair of the K of this point - weights at h + d * m, direction at pvals + d * n, result at jt + d * n
__global__ __launch_bounds__(HVP_THREADS) void ogk_exact_hvp(const ogk_args a) {
    const long d = (long)blockIdx.y;
    exact_hvp_block(a, a.h + d * OgGen::M, a.pvals + d * OgGen::N_VAR, a.jt + d * OgGen::N_VAR);
}

// the same on a lane's record (blockIdx.z: the lane): the direction is the record's h (bound to row `lane` of
// V[count][n]), the weights row `lane` of W[count][m], the result row `lane` of Q[count][n] (the launch's own arguments)
__global__ __launch_bounds__(HVP_THREADS) void ogk_exact_hvp_batch(const ogk_args* __restrict__ lanes, const double* W,
                                                                   double* Q) {
    const long lane = (long)blockIdx.z;
    const ogk_args& a = *(const ogk_args*)((ogk_lane_table)lanes + blockIdx.z);
    exact_hvp_block(a, W + lane * OgGen::M, a.h, Q + lane * OgGen::N_VAR);
}
#endif

// ------------------------------------------------------------------------------------------
// Modes 23 and 24 (the mixed part, OGK_PART_MIX): exact mixed derivatives s_k = d(F'(x)^T w)/dtheta_k, [n_par][n]
// doubles per weight vector w.  s_{k,j} is the sum that og_mix.h defines: the terms of column j that og_adj.h enumerates,
// each the mixed part of the item on second-order dual numbers (unit seed on x_j, unit seed on the parameter's table
// entry), times the weight of its row, in the chains and the tree of og_adj.h.  It is ogk_exact_hvp with the second slot
// seeded on theta_k instead of on v: the forward-mode work depends on the parameter, so one pair (weight vector d,
// parameter k) per grid slice - blockIdx.y = d * N_PAR + k for the K vectors of one point; blockIdx.y = k, blockIdx.z the
// lane for a batch - and nothing shared across pairs but the column lookup.  The column mapping is ogk_exact_hvp's: a
// heavy column (OGT_HEAVY) gets a workgroup, wavefront q runs block q of 64 chains and the four sums meet in LDS; every
// other column gets one wavefront, four columns per workgroup, which runs the four blocks one after the other.  The
// column and the parameter are the workgroup's or the wavefront's, so the column's records stay scalar loads.  Every
// s_{k,j} of every pair is written, +0.0 for a column without terms and for a parameter nothing reads; no J_T, no
// jt_state / jt_launches word.  y0 is the evaluation's.
// ------------------------------------------------------------------------------------------
#if defined(OGK_HAS_MIX) && defined(OG_GEN_HAS_PAR)
#include "og_mix.h"
constexpr int MIX_THREADS = OG_ADJ_CHAINS;
constexpr int MIX_WAVES = MIX_THREADS / 64;
static_assert(MIX_WAVES == 4, "og_adj_tree combines four blocks of 64 chains");

struct MixTables {
    __device__ __forceinline__ int4 col(const int j) const { return OGT_COL[j]; }
    __device__ __forceinline__ int4 elem(const int e) const { return OGT_ELEM[e]; }
    __device__ __forceinline__ const ogt_int8& slot(const int s) const { return OGT_SLOT[s]; }
};

inline int mix_grid() { return OgGen::N_HEAVY + (OgGen::N_VAR + MIX_WAVES - 1) / MIX_WAVES; }

// Block chain >> 6 of column j by the 64 lanes of one wavefront (chain: this lane's): the chain (og_mix_chain), then the
// levels s = 32 .. 1 of og_adj_tree -> valid in lane 0 (lane i of level s needs lane i + s < 2 s <= 64 only).  A block
// past the last term is +0.0 in every lane without any work.
__device__ __forceinline__ double mix_block_sum(const ogk_args& a, const MixTables& tab, const OgAdjCol& c, const int j,
                                                const int seed, const double* w, const int chain) {
    double r = og_mix_chain<OgGen>(tab, c, j, seed, chain, w, a.x0, a.y0, a.cvec, a.dfrag);
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) r = r + __shfl_down(r, s, 64);
    return r;
}

// w[M]: the weight vector, kp: the parameter, s[N_VAR]: the row of the result.  blockIdx.x: heavy columns first, then
// four light columns per workgroup.
__device__ __forceinline__ void exact_mix_block(const ogk_args& a, const double* w, const int kp, double* s) {
    __shared__ double part[MIX_WAVES];
    const int id = (int)blockIdx.x, tid = (int)threadIdx.x;
    // (the same in all 64 lanes of a wavefront - said to the compiler, so that the column's tables stay scalar loads)
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int seed = OgGen::PAR_OFF + kp;
    const MixTables tab;
    if (id < OgGen::N_HEAVY) {                      // the whole workgroup: every thread reaches the barrier
        const int j = OGT_HEAVY[id];
        const OgAdjCol c = og_adj_col<OgGen>(tab, j, a.x0, a.cvec);
        const double r = mix_block_sum(a, tab, c, j, seed, w, tid);
        if ((tid & 63) == 0) part[wave] = r;
        __syncthreads();
        if (tid == 0) s[j] = (part[0] + part[1]) + (part[2] + part[3]);
        return;
    }
    const int j = (id - OgGen::N_HEAVY) * MIX_WAVES + wave;
    if (j >= OgGen::N_VAR || (OGT_COL[j].w & HEAVY_FLAG)) return;   // (the whole wavefront; a heavy column has its own)
    const OgAdjCol c = og_adj_col<OgGen>(tab, j, a.x0, a.cvec);
    const int lane = tid & 63;
    double acc = 0.0, u = 0.0;
    // (p0 + p1) + (p2 + p3): acc = p0, acc += p1, u = p2, acc += u + p3
#pragma unroll 1
    for (int b = 0; b < MIX_WAVES; ++b) {
        const double r = mix_block_sum(a, tab, c, j, seed, w, b * 64 + lane);
        if (b == 0) acc = r;
        else if (b == 1) acc = acc + r;
        else if (b == 2) u = r;
        else acc = acc + (u + r);
    }
    if (lane == 0) s[j] = acc;
}

// blockIdx.y = d * N_PAR + k: weight vector d of the K of this point at h + d * m, parameter k, its row of the result at
// jt + blockIdx.y * n
__global__ __launch_bounds__(MIX_THREADS) void ogk_exact_mix(const ogk_args a) {
    const int pair = (int)blockIdx.y, d = pair / OgGen::N_PAR, kp = pair - d * OgGen::N_PAR;
    exact_mix_block(a, a.h + (long)d * OgGen::M, kp, a.jt + (long)pair * OgGen::N_VAR);
}

// the same on a lane's record (blockIdx.z: the lane, blockIdx.y: the parameter; the record's own cvec gives every lane
// its own theta): the weights are row `lane` of W[count][m], the result slice `lane` of S[count][n_par][n] (the launch's
// own arguments)
__global__ __launch_bounds__(MIX_THREADS) void ogk_exact_mix_batch(const ogk_args* __restrict__ lanes, const double* W,
                                                                   double* S) {
    const long lane = (long)blockIdx.z;
    const int kp = (int)blockIdx.y;
    const ogk_args& a = *(const ogk_args*)((ogk_lane_table)lanes + blockIdx.z);
    exact_mix_block(a, W + lane * OgGen::M, kp, S + (lane * OgGen::N_PAR + kp) * OgGen::N_VAR);
}
#endif

// ------------------------------------------------------------------------------------------
// Modes 25 and 26 (the Hessian-matrix part, OGK_PART_HESS): the exact sparse Hessian of w . F, [nnz] doubles per weight
// vector in the order of a static lower-triangle pattern.  A stored entry is the sum that og_hess.h defines: the terms of
// its owner's column that read the partner (the device plan, ogk.h: data the runtime uploads, not generated code), each
// the mixed part of the item on second-order dual numbers with one unit seed on the owner and one on the partner, times
// the weight of its row, in the chains and the tree of og_adj.h.  The mixed parts do not depend on w: a thread
// evaluates its term ONCE and applies it to every weight vector of its chunk (HESS_CHUNK of them, blockIdx.y), as
// ogk_exact_adj shares its first-order entries.  A thread takes the list position, not the chain: it adds its product
// into chain t & 255 of its term's own number t in LDS - round r = t >> 8 after round r - 1, so that two listed terms
// of one chain meet in ascending order - and a wavefront's 64 lanes then are 64 chains, __shfl_down the tree's levels
// s = 32 .. 1.  The work items are the stored entries:
//   - an entry with more than OGK_HESS_LIGHT_TERMS listed terms (the diagonal of a final time: all its thousand terms;
//     the diagonal of a state on more than 64 nodes) gets a workgroup, which walks the list 256 positions at a time;
//     wavefront q reduces block q of 64 chains and the four sums meet in LDS; these workgroups lead the grid;
//   - every other entry is summed inside ONE wavefront, a position per lane.  A wavefront takes a run of entries of one
//     owner (a unit of the plan), four units per workgroup, so the owner's column lookup (og_adj_col) and its records
//     stay scalar loads once per run; its 256 chains are its own quarter of the LDS array, a block of 64 chains that
//     no listed term falls into is +0.0 without being read; no workgroup barrier.
// The result is the host probe's (og_hess_entry) bit for bit whatever the scheduling, and vector d of K is the call with
// that vector alone.  Every stored entry of every vector is written, +0.0 for an entry without a listed term; nothing
// else is: no atomics, no J_T, no fill, no jt_state / jt_launches word.  y0 is the evaluation's.
// ------------------------------------------------------------------------------------------
#ifdef OGK_HAS_HESS
#include "og_hess.h"
constexpr int HESS_THREADS = OG_ADJ_CHAINS;
constexpr int HESS_WAVES = HESS_THREADS / 64;
constexpr int HESS_CHUNK = 8;           // weight vectors per chunk: the heavy workgroup's chains, 16 KiB of LDS
static_assert(HESS_WAVES == 4 && HESS_CHUNK >= HESS_WAVES && HESS_CHUNK <= 64 && OGK_HESS_LIGHT_TERMS == 64,
              "og_adj_tree combines four blocks of 64 chains; a light entry is one lane per listed term");

struct HessTables {
    __device__ __forceinline__ int4 col(const int j) const { return OGT_COL[j]; }
    __device__ __forceinline__ int4 elem(const int e) const { return OGT_ELEM[e]; }
    __device__ __forceinline__ const ogt_int8& slot(const int s) const { return OGT_SLOT[s]; }
};

// what a wavefront wrote to LDS is what its other lanes read next (the accesses of one wavefront stay in order)
__device__ __forceinline__ void hess_wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

// the levels s = 32 .. 1 of og_adj_tree over the 64 chains of one block, valid in lane 0
__device__ __forceinline__ double hess_block_tree(double r) {
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) r = r + __shfl_down(r, s, 64);
    return r;
}

// plan: the device plan (ogk.h).  w: the chunk's first weight vector (the next at w + M), H: row 0 of its part of the
// result (the next at H + nnz), kc: the chunk's vectors, 1 .. HESS_CHUNK.  blockIdx.x: the heavy entries first, then four
// units of light entries per workgroup.
__device__ __forceinline__ void exact_hess_block(const ogk_args& a, const int* __restrict__ plan, const double* w,
                                                 double* H, const int kc) {
    __shared__ double chains[HESS_CHUNK][OG_ADJ_CHAINS];
    __shared__ double part[HESS_CHUNK][HESS_WAVES];
    const int id = (int)blockIdx.x, tid = (int)threadIdx.x, lane = tid & 63;
    // (the same in all 64 lanes of a wavefront - said to the compiler, so that the plan and the tables stay scalar loads)
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int nnz = plan[0], n_light = plan[1], n_units = plan[2];
    const int4* ent = (const int4*)(plan + OGK_HESS_HEAD);
    const int* tptr = plan + plan[3];
    const int* tlist = plan + plan[4];
    const int* unit = plan + plan[5];
    const HessTables tab;
    if (id < nnz - n_light) {                       // the whole workgroup: every thread reaches every barrier
        const int4 E = ent[n_light + id];
        const int owner = E.x, partner = E.y, pos = E.z, t0 = tptr[pos], t1 = tptr[pos + 1];
        const OgAdjCol c = og_adj_col<OgGen>(tab, owner, a.x0, a.cvec);
#pragma unroll
        for (int d = 0; d < HESS_CHUNK; ++d) chains[d][tid] = 0.0;
        __syncthreads();
        for (int base = t0; base < t1; base += HESS_THREADS) {
            const int last = (base + HESS_THREADS < t1 ? base + HESS_THREADS : t1) - 1;
            const int r_lo = tlist[base] >> 8, r_hi = tlist[last] >> 8;
            const bool mine = base + tid <= last;
            int t = 0, row = 0;
            double e = 0.0;
            if (mine) {
                t = tlist[base + tid];
                e = og_hess_term<OgGen>(tab, c, owner, partner, t, a.x0, a.y0, a.cvec, a.dfrag, &row);
            }
            for (int r = r_lo; r <= r_hi; ++r) {
                if (mine && (t >> 8) == r) {
                    const int chain = t & (OG_ADJ_CHAINS - 1);
#pragma unroll
                    for (int d = 0; d < HESS_CHUNK; ++d)
                        if (d < kc) chains[d][chain] = __builtin_fma(w[(long)d * OgGen::M + row], e, chains[d][chain]);
                }
                __syncthreads();
            }
        }
#pragma unroll
        for (int d = 0; d < HESS_CHUNK; ++d)
            if (d < kc) {
                const double r = hess_block_tree(chains[d][tid]);
                if (lane == 0) part[d][wave] = r;
            }
        __syncthreads();
        if (tid < kc) H[(long)tid * nnz + pos] = (part[tid][0] + part[tid][1]) + (part[tid][2] + part[tid][3]);
        return;
    }
    const int u = (id - (nnz - n_light)) * HESS_WAVES + wave;
    if (u >= n_units) return;                       // (the whole wavefront)
    const int e_lo = unit[u], e_hi = unit[u + 1];
    const int owner = ent[e_lo].x;
    const OgAdjCol c = og_adj_col<OgGen>(tab, owner, a.x0, a.cvec);
    // this wavefront's 256 chains: a quarter of the array (HESS_CHUNK >= HESS_WAVES), one weight vector at a time
    double* ch = &chains[0][0] + wave * OG_ADJ_CHAINS;
#pragma unroll 1
    for (int en = e_lo; en < e_hi; ++en) {
        const int4 E = ent[en];
        const int partner = E.y, pos = E.z, t0 = tptr[pos], nt = tptr[pos + 1] - t0;
        const bool mine = lane < nt;
        int t = 0, row = 0, r_lo = 0, r_hi = -1;
        double e = 0.0;
        if (nt > 0) r_lo = tlist[t0] >> 8, r_hi = tlist[t0 + nt - 1] >> 8;
        if (mine) {
            t = tlist[t0 + lane];
            e = og_hess_term<OgGen>(tab, c, owner, partner, t, a.x0, a.y0, a.cvec, a.dfrag, &row);
        }
        const int chain = t & (OG_ADJ_CHAINS - 1);
        bool has[HESS_WAVES];                       // does a listed term fall into block q of the chains?
#pragma unroll
        for (int q = 0; q < HESS_WAVES; ++q) has[q] = __ballot(mine && (chain >> 6) == q) != 0;
#pragma unroll 1
        for (int d = 0; d < kc; ++d) {
#pragma unroll
            for (int q = 0; q < HESS_WAVES; ++q)
                if (has[q]) ch[q * 64 + lane] = 0.0;
            hess_wave_sync();
            const double wr = mine ? w[(long)d * OgGen::M + row] : 0.0;
            for (int r = r_lo; r <= r_hi; ++r) {
                if (mine && (t >> 8) == r) ch[chain] = __builtin_fma(wr, e, ch[chain]);
                hess_wave_sync();
            }
            // (p0 + p1) + (p2 + p3); a block without a listed term is +0.0 in every chain and so in its sum
            double p[HESS_WAVES];
#pragma unroll
            for (int q = 0; q < HESS_WAVES; ++q) p[q] = has[q] ? hess_block_tree(ch[q * 64 + lane]) : 0.0;
            if (lane == 0) H[(long)d * nnz + pos] = (p[0] + p[1]) + (p[2] + p[3]);
            hess_wave_sync();
        }
    }
}

// blockIdx.y: the chunk of the K = nw weight vectors, read at h + d * m, written to jt + d * nnz; prow: the device plan
__global__ __launch_bounds__(HESS_THREADS) void ogk_exact_hess(const ogk_args a, const int nw) {
    const int* plan = (const int*)a.prow;
    const int d0 = (int)blockIdx.y * HESS_CHUNK;
    const int kc = nw - d0 < HESS_CHUNK ? nw - d0 : HESS_CHUNK;
    exact_hess_block(a, plan, a.h + (long)d0 * OgGen::M, a.jt + (long)d0 * plan[0], kc);
}

// the same on a lane's record (blockIdx.z: the lane): one weight vector per lane, row `lane` of W[count][m], the result
// in row `lane` of H[count][nnz] (the launch's own arguments, and so is the plan)
__global__ __launch_bounds__(HESS_THREADS) void ogk_exact_hess_batch(const ogk_args* __restrict__ lanes,
                                                                     const int* __restrict__ plan, const double* W,
                                                                     double* H) {
    const long lane = (long)blockIdx.z;
    const ogk_args& a = *(const ogk_args*)((ogk_lane_table)lanes + blockIdx.z);
    exact_hess_block(a, plan, W + lane * OgGen::M, H + lane * plan[0], 1);
}
static_assert(OGK_HESS_WORKGROUPS(9, 2, 5) == 7 + (5 + HESS_WAVES - 1) / HESS_WAVES, "the runtime sizes the grid (ogk.h)");
#endif

// ------------------------------------------------------------------------------------------
// Modes 27 and 28 (the parameter-Hessian part, OGK_PART_PP): exact second derivatives of w . F in the run-time
// parameters, S_kl = sum_r w_r d2F_r/dtheta_k dtheta_l, [n_par][n_par] doubles per weight vector w.  S_kl is the sum that
// og_pp.h defines: the entries of the work lists of the pair's OWNER (the parameter with fewer entries), each the mixed
// part of the entry on second-order dual numbers - unit seed of slot 1 on the owner's table entry, of slot 2 on the
// partner's - times the weight of its row, in the chains and the tree of og_adj.h.  One workgroup of OG_ADJ_CHAINS
// threads serves ONE pair (blockIdx.x, of n_par (n_par + 1) / 2) and one chunk of up to PP_CHUNK weight vectors
// (blockIdx.y; blockIdx.z the lane of a batch, one vector per lane): thread c is chain c, it evaluates each of its
// entries ONCE and applies it to every vector of the chunk - the forward-mode work does not depend on w, which is the
// sharing ogk_exact_mix lacks.  The tree's levels 32 .. 1 are a shuffle-down reduction inside a wavefront and the four
// block sums meet in LDS as (p0 + p1) + (p2 + p3): the heavy path of exact_mix_block.  The pair, its owner and the ranges
// of the owner's lists are the workgroup's, so they stay scalar loads.  Every S[d][k][l] and S[d][l][k] is written on
// every call, +0.0 where the owner's list is empty; no J_T, no jt_state / jt_launches word, no atomics.  y0 is the
// evaluation's (OGK_EVAL / OGK_BATCH_EVAL before this launch on the same stream).
// ------------------------------------------------------------------------------------------
#if defined(OGK_HAS_PP) && defined(OG_GEN_HAS_PAR)
#include "og_pp.h"
constexpr int PP_THREADS = OG_ADJ_CHAINS;
constexpr int PP_WAVES = PP_THREADS / 64;
constexpr int PP_CHUNK = 8;             // weight vectors per chunk: 16 VGPRs of partial sums per thread
constexpr int PP_PAIRS = OgGen::N_PAR * (OgGen::N_PAR + 1) / 2;
static_assert(PP_WAVES == 4 && PP_CHUNK <= 64, "og_adj_tree combines four blocks of 64 chains");

// w: the chunk's first weight vector (the next at w + M), S: the [N_PAR][N_PAR] block of that vector (the next at
// S + N_PAR * N_PAR), kc: the chunk's vectors, 1 .. PP_CHUNK.  Every thread reaches the barrier.
__device__ __forceinline__ void exact_pp_block(const ogk_args& a, const double* w, double* S, const int kc) {
    __shared__ double part[PP_CHUNK][PP_WAVES];
    const int tid = (int)threadIdx.x;
    // (the same in all 64 lanes of a wavefront - said to the compiler, as in exact_adj_block)
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const OgPpPair p = og_pp_pair<OgGen>((int)blockIdx.x);
    double r[PP_CHUNK];
#pragma unroll
    for (int d = 0; d < PP_CHUNK; ++d) r[d] = 0.0;
    for (int e = tid; e < p.entries; e += OG_ADJ_CHAINS) {
        int row;
        const double t = og_pp_term<OgGen>(p.owner, p.partner, e, a.x0, a.y0, a.cvec, a.dfrag, &row).dd;
#pragma unroll
        for (int d = 0; d < PP_CHUNK; ++d)
            if (d < kc) r[d] = __builtin_fma(w[(long)d * OgGen::M + row], t, r[d]);
    }
    // the levels s = 32 .. 1 of og_adj_tree -> valid in lane 0 (lane i of level s needs lane i + s < 2 s <= 64 only)
#pragma unroll
    for (int d = 0; d < PP_CHUNK; ++d)
        if (d < kc) {
#pragma unroll
            for (int s = 32; s >= 1; s >>= 1) r[d] = r[d] + __shfl_down(r[d], s, 64);
        }
    if ((tid & 63) == 0) {
#pragma unroll
        for (int d = 0; d < PP_CHUNK; ++d) part[d][wave] = r[d];
    }
    __syncthreads();
    if (tid < kc) {
        const double v = (part[tid][0] + part[tid][1]) + (part[tid][2] + part[tid][3]);
        double* Sd = S + (long)tid * (OgGen::N_PAR * OgGen::N_PAR);
        Sd[p.k * OgGen::N_PAR + p.l] = v;
        Sd[p.l * OgGen::N_PAR + p.k] = v;
    }
}

// blockIdx.y: the chunk of the K = nw weight vectors, read at h + d * m, written to jt + d * n_par * n_par
__global__ __launch_bounds__(PP_THREADS) void ogk_exact_pp(const ogk_args a, const int nw) {
    const int d0 = (int)blockIdx.y * PP_CHUNK;
    const int kc = nw - d0 < PP_CHUNK ? nw - d0 : PP_CHUNK;
    exact_pp_block(a, a.h + (long)d0 * OgGen::M, a.jt + (long)d0 * (OgGen::N_PAR * OgGen::N_PAR), kc);
}

// the same on a lane's record (blockIdx.z: the lane; the record's own cvec gives every lane its own theta): one weight
// vector per lane, row `lane` of W[count][m], the result slice `lane` of S[count][n_par][n_par] (the launch's own
// arguments)
__global__ __launch_bounds__(PP_THREADS) void ogk_exact_pp_batch(const ogk_args* __restrict__ lanes, const double* W,
                                                                 double* S) {
    const long lane = (long)blockIdx.z;
    const ogk_args& a = *(const ogk_args*)((ogk_lane_table)lanes + blockIdx.z);
    exact_pp_block(a, W + lane * OgGen::M, S + lane * (OgGen::N_PAR * OgGen::N_PAR), 1);
}
#endif

#ifdef OGK_HAS_SWEEP
__global__ __launch_bounds__(SWEEP_THREADS) void ogk_sweep(const ogk_args a) {
    extern __shared__ __attribute__((aligned(16))) double lds[];
    const int id = (int)blockIdx.x;
    if (id < OGT_N_TILES) {
        // MFMA tiles have the longest dependent chain: dispatch them first
        if (!(OGK_EXP & 32)) tile_body(a, id);
    } else if (id < OGT_N_TILES + OgGen::N_HEAVY) {
        // then the columns with many dependent items (e.g. phase final times): a workgroup each
        const int j = OGT_HEAVY[id - OGT_N_TILES];
        if (j >= a.col_lo && j < a.col_hi) heavy_column_body(a, j, reinterpret_cast<unsigned*>(lds));
    } else {
        // all columns of this launch, LIGHT_COLS per workgroup
        light_columns_body(a, a.col_lo + (id - OGT_N_TILES - OgGen::N_HEAVY) * LIGHT_COLS,
                           reinterpret_cast<unsigned*>(lds));
    }
}
#endif

// ------------------------------------------------------------------------------------------
// Modes 6-9: the packed non-zeros.  One wavefront per column; entry i of column j is row own_lo + i for
// i < own_hi - own_lo (the collocation block the MFMA tiles write) and the row of item i - (own_hi - own_lo)
// after that (OGT_ELEM order) - the order codegen.sparsity() documents.
// ------------------------------------------------------------------------------------------
constexpr int PACK_THREADS = 256;
__device__ __forceinline__ int pattern_row(const int4 col, const int own, const int i) {
    return i < own ? col.z + i : OGT_ELEM[col.x + (i - own)].w;
}

#ifdef OGK_HAS_MAIN
__global__ void ogk_count_launch(const ogk_args a) {
    if (threadIdx.x == 0 && blockIdx.x == 0)
        __hip_atomic_store(a.jt_launches, *a.jt_launches + 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
#endif

#ifdef OGK_HAS_MAIN
__global__ __launch_bounds__(PACK_THREADS) void ogk_pattern(const ogk_args a, const int rows_pass) {
    const int j = (int)(blockIdx.x * (PACK_THREADS / 64) + (threadIdx.x >> 6));
    const int lane = (int)threadIdx.x & 63;
    if (j >= OgGen::N_VAR) return;
    const int4 col = OGT_COL[j];
    const int own = (col.w & ~HEAVY_FLAG) - col.z, cnt = own + (col.y - col.x);
    if (!rows_pass) {
        if (lane == 0) a.pint[j] = cnt;
        return;
    }
    for (int i = lane; i < cnt; i += 64) a.pint[a.poff[j] + i] = pattern_row(col, own, i);
}
#endif

// Pack / unpack: one workgroup per column, its entries taken from the flat row-index array of the pattern
// (coalesced; the only dependent access is the J_T entry itself).  A phase's final time has a thousand entries,
// an ordinary column a few dozen: a workgroup per column keeps the long ones from becoming the kernel's tail.
#ifdef OGK_HAS_MAIN
__global__ __launch_bounds__(PACK_THREADS) void ogk_pack(const ogk_args a) {
    const int j = a.col_lo + (int)blockIdx.x;
    const int tid = (int)threadIdx.x;
    if (blockIdx.x == 0 && a.ptail) {
        for (int r = tid; r < OgGen::M; r += PACK_THREADS) a.ptail[r] = a.f0[r];
        if (tid == 0) a.ptail[OgGen::M] = (double)*a.nonfinite;
    }
    if (j >= a.col_hi) return;
    const long base = a.pind[j];
    const int cnt = (int)(a.pind[j + 1] - base);
    const double* jrow = a.jt + (long)(j - a.col_lo) * OgGen::M;
    double* out = a.pvals + a.poff[j];
    const int32_t* rows = a.prow + base;
    for (int i = tid; i < cnt; i += PACK_THREADS) out[i] = jrow[rows[i]];
}
#endif

#ifdef OGK_HAS_MAIN
__global__ __launch_bounds__(PACK_THREADS) void ogk_unpack(const ogk_args a) {
    // rows [ulo, uhi) of the full matrix except this rank's own block
    int j = a.ulo + (int)blockIdx.x;
    if (j >= a.col_lo) j += a.col_hi - a.col_lo;
    const int tid = (int)threadIdx.x;
    // a rank without columns of its own (jt_bump): nobody else records that this step fills with NaN.  The
    // other workgroups' decision below does not depend on this store (they see the same non-zero count)
    if (a.jt_bump && blockIdx.x == 0 && tid == 0 && *a.nonfinite != 0) jt_mark_nan_fill(a);
    if (j >= a.uhi) return;
    const long base = a.pind[j];
    const int cnt = (int)(a.pind[j + 1] - base);
    double* jrow = a.jt + (long)j * OgGen::M;
    // every rank evaluated the same F(x0): its z says which rows are NaN in every column; a fill (NaN now, or
    // zeros to clean up after one) goes first, then the barrier, then the column's entries
    const bool fill = a.jt_sparse && (*a.nonfinite != 0 || *a.jt_state == *a.jt_launches - 1u);
    if (fill) {                                         // workgroup-uniform
        for (int r = tid; r < OgGen::M; r += PACK_THREADS) jrow[r] = a.z[r];
        __builtin_amdgcn_s_waitcnt(0);
        __syncthreads();
    }
    const double* in = a.pvals + a.poff[j];
    const int32_t* rows = a.prow + base;
    for (int i = tid; i < cnt; i += PACK_THREADS) jrow[rows[i]] = in[i];
}
#endif

int defect_blocks() {
    int nb = 0;
    for (int g = 0; g < OgGen::N_GROUPS; ++g)
        if (OgGen::G_KIND(g) == 1) nb += (OgGen::G_LEN(g) + 15) >> 4;
    return nb;
}

size_t defect_lds_bytes() {
    size_t worst = 0;
    for (int g = 0; g < OgGen::N_GROUPS; ++g) {
        if (OgGen::G_KIND(g) != 1) continue;
        const int KS = (OgGen::G_LEN(g) + 3) >> 2;
        const size_t need = ((size_t)KS * 64 + (size_t)OgGen::MAX_NMV * KS * 4 + 256) * sizeof(double);
        worst = need > worst ? need : worst;
    }
    const size_t terms = (size_t)TERM_DOUBLES * sizeof(double);      // evaluation row blocks: cached sum terms
    return worst > terms ? worst : terms;
}

// OGK_EVAL, OGK_DENSE and OGK_BATCH_EVAL ask for defect_lds_bytes() of dynamic LDS whatever the phase lengths are, also
// beyond the 64 KiB of the one-launch window (launch4 on 341 nodes per phase: 68 096 bytes); a compute unit of gfx950 has 160 KiB.
// codegen.emit_header refuses a program beyond that before it is compiled (codegen.check_limits); a module that was
// built some other way answers hipErrorInvalidValue here instead of launching.
bool eval_lds_fits() { return defect_lds_bytes() <= 160 * 1024; }

size_t sweep_lds_bytes() { return (size_t)LIGHT_COLS * ROW_WORDS * sizeof(unsigned); }

// The geometry of the one-launch form (ogk_fused, ogk_fused_batch), in one place: what ogk_get_info promises as
// fused_ok is what OGK_FUSED and OGK_BATCH_FUSED accept.
int eval_row_blocks() { return (OGT_N_ROWWAVES + SWEEP_WAVES - 1) / SWEEP_WAVES; }

// the largest of what its workgroup kinds ask for: collocation and row blocks of the evaluation, the tiles of the
// sweep, finish_eval's bitmap of one row
size_t fused_lds_bytes() {
    size_t bytes = defect_lds_bytes() > FZ_LDS_BYTES ? defect_lds_bytes() : FZ_LDS_BYTES;
    const size_t fill_lds = (size_t)ROW_WORDS * sizeof(unsigned);
    return fill_lds > bytes ? fill_lds : bytes;
}

// its LDS window is 64 KiB, and a ticket needs evaluation workgroups to count
bool fused_fits() { return fused_lds_bytes() <= 64 * 1024 && defect_blocks() + eval_row_blocks() > 0; }

// A grid beyond one round of residency (two workgroups per compute unit, 512 on this part) starts its later
// workgroups microseconds late: the light workgroups with a sequential sum - a chain of as many dependent
// additions as the sum has terms, the longest of the launch - then go first (C5: 29.8 -> 24.6 us per launch;
// a grid that fits one round is left in column order: C4 lost 1.1 us to the other order).  -> the kernel's n_sum:
// how many light workgroups have such a sum, or -1 for column order
int fused_light_order(long workgroups, int n_sum) { return workgroups <= 512 ? -1 : n_sum; }

}  // namespace

// N_PAR and PAR_OFF are in the generated header only when the problem declares run-time parameters
namespace {
template <class G> constexpr auto gen_n_par(int) -> decltype(G::N_PAR) { return G::N_PAR; }
template <class G> constexpr int gen_n_par(long) { return 0; }
template <class G> constexpr auto gen_par_off(int) -> decltype(G::PAR_OFF) { return G::PAR_OFF; }
template <class G> constexpr int gen_par_off(long) { return G::N_CVEC; }
}  // namespace

extern "C" int ogk_get_par_info(ogk_par_info* out) {
    out->n_par = gen_n_par<OgGen>(0);
    out->par_off = gen_par_off<OgGen>(0);
    return 0;
}

extern "C" int ogk_get_info(ogk_info* out) {
    out->abi = OGK_ABI;
    out->n_eval_blocks = defect_blocks() + eval_row_blocks();
    out->fused_ok = fused_fits() ? 1 : 0;
    out->n = OgGen::N_VAR;
    out->m = OgGen::M;
    out->m_eq = OgGen::M_EQ;
    out->m_ineq = OgGen::M_INEQ;
    out->n_phase = OgGen::N_PHASE;
    out->n_mv = OgGen::N_MV;
    out->n_groups = OgGen::N_GROUPS;
    out->n_cvec = OgGen::N_CVEC;
    out->n_y0 = OgGen::N_Y0;
    for (int i = 0; i < OGK_MAX_PHASE; ++i)
        out->phase_nodes[i] = i < OgGen::N_PHASE ? OgGen::PHASE_NODES(i) : 0;
    return 0;
}

// A module may be built in parts (OGK_PART, build.py): a part answers OGK_OTHER_PART for a mode whose kernel it
// does not hold and the runtime turns to the part that does.
extern "C" int ogk_launch(const ogk_args* args, int mode, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    const int ndef = defect_blocks();
    const int ncols = args->col_hi - args->col_lo;
    (void)stream;
    (void)ndef;
    (void)ncols;
#ifdef OGK_HAS_MAIN
    if (mode == OGK_EVAL) {
        if (!eval_lds_fits()) return (int)hipErrorInvalidValue;
        if (ndef + eval_row_blocks() > 0)
            hipLaunchKernelGGL(ogk_eval, dim3(ndef + eval_row_blocks()), dim3(SWEEP_THREADS),
                               defect_lds_bytes(), stream, *args, ndef);
        return (int)hipGetLastError();
    }
    if (mode == OGK_COUNT_LAUNCH) {
        hipLaunchKernelGGL(ogk_count_launch, dim3(1), dim3(64), 0, stream, *args);
        return (int)hipGetLastError();
    }
    if (mode == OGK_PATTERN_COUNT || mode == OGK_PATTERN_ROWS) {
        hipLaunchKernelGGL(ogk_pattern, dim3((OgGen::N_VAR + PACK_THREADS / 64 - 1) / (PACK_THREADS / 64)),
                           dim3(PACK_THREADS), 0, stream, *args, mode == OGK_PATTERN_ROWS ? 1 : 0);
        return (int)hipGetLastError();
    }
    if (mode == OGK_PACK) {
        if (ncols <= 0 && !args->ptail) return 0;
        hipLaunchKernelGGL(ogk_pack, dim3(ncols > 0 ? ncols : 1), dim3(PACK_THREADS), 0, stream, *args);
        return (int)hipGetLastError();
    }
    if (mode == OGK_UNPACK) {
        const int others = (args->uhi - args->ulo) - ncols;
        if (others > 0)
            hipLaunchKernelGGL(ogk_unpack, dim3(others), dim3(PACK_THREADS), 0, stream, *args);
        return (int)hipGetLastError();
    }
#endif
#ifdef OGK_HAS_SWEEP
    if (mode == OGK_SWEEP) {
        if (ncols <= 0) return 0;
        const int light_blocks = (ncols + LIGHT_COLS - 1) / LIGHT_COLS;
        hipLaunchKernelGGL(ogk_sweep, dim3(OGT_N_TILES + OgGen::N_HEAVY + light_blocks),
                           dim3(SWEEP_THREADS), sweep_lds_bytes(), stream, *args);
        return (int)hipGetLastError();
    }
#endif
#ifdef OGK_HAS_FUSED
    if (mode == OGK_FUSED) {
        if (ncols <= 0) return 0;
        // light workgroups whose columns touch [col_lo, col_hi)
        int glo = 0, ghi = OGT_N_LGRP;
        while (glo < ghi && OGH_LGRP_J[glo + 1] <= args->col_lo) ++glo;
        while (ghi > glo && OGH_LGRP_J[ghi - 1] >= args->col_hi) --ghi;
        // the one-launch form writes the non-zeros only: it needs a registered (persistent-zero) output buffer
        // (og_jt_register_dev) and its LDS window (ogk_info.fused_ok); the caller runs OGK_EVAL + OGK_SWEEP otherwise
        if (!args->jt_sparse || !fused_fits()) return (int)hipErrorInvalidValue;
        int sum_lo = 0, n_sum = 0;
        for (int gidx = 0; gidx < ghi; ++gidx) {
            if (gidx < glo) sum_lo += OGH_LGRP_SUM[gidx];
            else n_sum += OGH_LGRP_SUM[gidx];
        }
        const int n_eval = ndef + eval_row_blocks();
        const int grid = n_eval + OGT_N_FTILES + OGT_N_HPART + (ghi - glo);
        hipLaunchKernelGGL(ogk_fused, dim3(grid), dim3(SWEEP_THREADS), fused_lds_bytes(), stream, *args, ndef, n_eval,
                           glo, ghi - glo, sum_lo, fused_light_order(grid, n_sum));
        return (int)hipGetLastError();
    }
#endif
#ifdef OGK_HAS_AUX
    if (mode == OGK_EXACT) {
        if (ncols <= 0) return 0;
        hipLaunchKernelGGL(ogk_exact_struct, dim3(ncols), dim3(256), 0, stream, *args);
        return (int)hipGetLastError();
    }
    if (mode == OGK_EXACT_DENSE) {
        if (ncols <= 0) return 0;
        int n_items = OgGen::N_ROW_ITEMS;
        for (int g = 0; g < OgGen::N_GROUPS; ++g)
            if (OgGen::G_KIND(g) == 1) n_items += OgGen::G_LEN(g);
        if (n_items > 0)
            hipLaunchKernelGGL(ogk_exact, dim3((n_items + 255) / 256, ncols), dim3(256), 0, stream, *args, n_items);
        return (int)hipGetLastError();
    }
    if (mode == OGK_DENSE) {
        if (ncols <= 0) return 0;
        if (!eval_lds_fits()) return (int)hipErrorInvalidValue;
        const int row_blocks = (OgGen::N_ROW_ITEMS + 255) / 256;
        const int defect_total = ndef * ((ncols + 63) / 64);
        const int rows_total = row_blocks * ((ncols + ROWS_COLS_PER_THREAD - 1) / ROWS_COLS_PER_THREAD);
        if (defect_total + rows_total > 0)
            hipLaunchKernelGGL(ogk_dense, dim3(defect_total + rows_total), dim3(256),
                               defect_lds_bytes(), stream, *args, ndef, defect_total, row_blocks);
        return (int)hipGetLastError();
    }
#endif
#ifdef OGK_HAS_PAR
    if (mode == OGK_PAR_JAC) {
#ifdef OG_GEN_HAS_PAR
        if (!args->jt || !args->x0 || !args->y0) return (int)hipErrorInvalidValue;
        hipLaunchKernelGGL(ogk_exact_par, dim3(1, OgGen::N_PAR), dim3(PAR_THREADS), 0, stream, *args);
        return (int)hipGetLastError();
#else
        return (int)hipErrorInvalidValue;           // a module without run-time parameters
#endif
    }
#endif
#ifdef OGK_HAS_DIR
    if (mode == OGK_DIR) {
        // ncols directions (gridDim.y: at most 65535)
        if (!args->jt || !args->x0 || !args->y0 || !args->h || ncols < 1 || ncols > 65535) return (int)hipErrorInvalidValue;
        const int row_blocks = dir_row_blocks(), grid = row_blocks + dir_defect_units();
        if (grid > 0)
            hipLaunchKernelGGL(ogk_exact_dir, dim3(grid, ncols), dim3(DIR_THREADS), 0, stream, *args, row_blocks);
        return (int)hipGetLastError();
    }
#endif
#ifdef OGK_HAS_ADJ
    if (mode == OGK_ADJ) {
        // ncols weight vectors (gridDim.y: their chunks)
        if (!args->jt || !args->x0 || !args->y0 || !args->h || ncols < 1 || ncols > 65535) return (int)hipErrorInvalidValue;
        hipLaunchKernelGGL(ogk_exact_adj, dim3(adj_grid(), (ncols + ADJ_CHUNK - 1) / ADJ_CHUNK), dim3(ADJ_THREADS), 0, stream,
                           *args, ncols);
        return (int)hipGetLastError();
    }
#endif
#ifdef OGK_HAS_HVP
    if (mode == OGK_HVP) {
        // ncols pairs (gridDim.y)
        if (!args->jt || !args->x0 || !args->y0 || !args->h || !args->pvals || ncols < 1 || ncols > 65535)
            return (int)hipErrorInvalidValue;
        hipLaunchKernelGGL(ogk_exact_hvp, dim3(hvp_grid(), ncols), dim3(HVP_THREADS), 0, stream, *args);
        return (int)hipGetLastError();
    }
#endif
#ifdef OGK_HAS_MIX
    if (mode == OGK_MIX) {
#ifdef OG_GEN_HAS_PAR
        // ncols weight vectors, ncols * N_PAR pairs (gridDim.y)
        if (!args->jt || !args->x0 || !args->y0 || !args->h || ncols < 1 || (long)ncols * OgGen::N_PAR > 65535)
            return (int)hipErrorInvalidValue;
        hipLaunchKernelGGL(ogk_exact_mix, dim3(mix_grid(), ncols * OgGen::N_PAR), dim3(MIX_THREADS), 0, stream, *args);
        return (int)hipGetLastError();
#else
        return (int)hipErrorInvalidValue;           // a module without run-time parameters
#endif
    }
#endif
#ifdef OGK_HAS_HESS
    if (mode == OGK_HESS) {
        // ncols weight vectors (gridDim.y: their chunks); uhi - ulo: the workgroups of one chunk (OGK_HESS_WORKGROUPS)
        const int grid = args->uhi - args->ulo;
        if (!args->jt || !args->x0 || !args->y0 || !args->h || !args->prow || ncols < 1 || ncols > 65535 || grid < 0)
            return (int)hipErrorInvalidValue;
        if (grid > 0)
            hipLaunchKernelGGL(ogk_exact_hess, dim3(grid, (ncols + HESS_CHUNK - 1) / HESS_CHUNK), dim3(HESS_THREADS), 0,
                               stream, *args, ncols);
        return (int)hipGetLastError();
    }
#endif
#ifdef OGK_HAS_PP
    if (mode == OGK_PP) {
#ifdef OG_GEN_HAS_PAR
        // ncols weight vectors (gridDim.y: their chunks), one workgroup per pair of parameters and chunk
        if (!args->jt || !args->x0 || !args->y0 || !args->h || ncols < 1 || ncols > 65535) return (int)hipErrorInvalidValue;
        hipLaunchKernelGGL(ogk_exact_pp, dim3(PP_PAIRS, (ncols + PP_CHUNK - 1) / PP_CHUNK), dim3(PP_THREADS), 0, stream,
                           *args, ncols);
        return (int)hipGetLastError();
#else
        return (int)hipErrorInvalidValue;           // a module without run-time parameters
#endif
    }
#endif
    return OGK_OTHER_PART;
}

#ifdef OGK_HAS_BATCH
extern "C" int ogk_launch_batch(const ogk_batch_args* b, int mode, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (!b || !b->lanes || b->count < 1 || b->count > b->capacity) return (int)hipErrorInvalidValue;
    const int ndef = defect_blocks(), n_eval = ndef + eval_row_blocks();
    if (mode == OGK_BATCH_BIND) {
        const int records = OGK_BATCH_SETS * b->capacity;
        hipLaunchKernelGGL(ogk_batch_bind, dim3((records + 63) / 64), dim3(64), 0, stream, *b);
        return (int)hipGetLastError();
    }
    if (mode == OGK_BATCH_EVAL) {
        if (!eval_lds_fits()) return (int)hipErrorInvalidValue;
        if (n_eval > 0)
            hipLaunchKernelGGL(ogk_eval_batch, dim3(n_eval, b->count), dim3(SWEEP_THREADS),
                               defect_lds_bytes(), stream, (const ogk_args*)b->lanes, ndef);
        return (int)hipGetLastError();
    }
    if (mode == OGK_BATCH_FUSED) {
        // the geometry of OGK_FUSED over all n columns, once per lane (the order of a lane's light workgroups goes by
        // the whole launch)
        if (!fused_fits()) return (int)hipErrorInvalidValue;
        int n_sum = 0;
        for (int gidx = 0; gidx < OGT_N_LGRP; ++gidx) n_sum += OGH_LGRP_SUM[gidx];
        const int grid = n_eval + OGT_N_FTILES + OGT_N_HPART + OGT_N_LGRP;
        hipLaunchKernelGGL(ogk_fused_batch, dim3(grid, b->count), dim3(SWEEP_THREADS), fused_lds_bytes(), stream,
                           (const ogk_args*)b->lanes, ndef, n_eval, 0, OGT_N_LGRP, 0,
                           fused_light_order((long)grid * b->count, n_sum));
        return (int)hipGetLastError();
    }
    return (int)hipErrorInvalidValue;
}
#endif

#ifdef OGK_HAS_BATCH_EXACT
// the exact batch part's only mode: it exports the same entry name as the batch part and is looked up in its own
// shared object
extern "C" int ogk_launch_batch(const ogk_batch_args* b, int mode, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (!b || !b->lanes || b->count < 1 || b->count > b->capacity || mode != OGK_BATCH_EXACT) return (int)hipErrorInvalidValue;
    const int grid = OgGen::N_HEAVY + (OgGen::N_VAR + XB_COLS - 1) / XB_COLS;
    hipLaunchKernelGGL(ogk_exact_struct_batch, dim3(grid, b->count), dim3(XB_THREADS), 0, stream,
                       (const ogk_args*)b->lanes);
    return (int)hipGetLastError();
}
#endif

#ifdef OGK_HAS_PAR
// the parameter part's batched mode: it exports the entry name of the batch parts and is looked up in its own shared
// object
extern "C" int ogk_launch_batch(const ogk_batch_args* b, int mode, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (!b || !b->lanes || b->count < 1 || b->count > b->capacity || mode != OGK_BATCH_PAR_JAC) return (int)hipErrorInvalidValue;
#ifdef OG_GEN_HAS_PAR
    hipLaunchKernelGGL(ogk_exact_par_batch, dim3(1, OgGen::N_PAR, b->count), dim3(PAR_THREADS), 0, stream,
                       (const ogk_args*)b->lanes);
    return (int)hipGetLastError();
#else
    (void)stream;
    return (int)hipErrorInvalidValue;               // a module without run-time parameters
#endif
}
#endif

#ifdef OGK_HAS_DIR
// the directional part's batched mode: it exports the entry name of the batch parts and is looked up in its own shared
// object
extern "C" int ogk_launch_batch(const ogk_batch_args* b, int mode, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (!b || !b->lanes || b->count < 1 || b->count > b->capacity || b->count > 65535 || mode != OGK_BATCH_DIR)
        return (int)hipErrorInvalidValue;
    const int row_blocks = dir_row_blocks(), grid = row_blocks + dir_defect_units();
    if (grid > 0)
        hipLaunchKernelGGL(ogk_exact_dir_batch, dim3(grid, 1, b->count), dim3(DIR_THREADS), 0, stream,
                           (const ogk_args*)b->lanes, row_blocks);
    return (int)hipGetLastError();
}
#endif

#ifdef OGK_HAS_ADJ
// the adjoint part's batched mode: it exports the entry name of the batch parts and is looked up in its own shared
// object.  H: the weight vectors W[count][m], vals: the result G[count][n] (the lane records hold neither)
extern "C" int ogk_launch_batch(const ogk_batch_args* b, int mode, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (!b || !b->lanes || b->count < 1 || b->count > b->capacity || b->count > 65535 || mode != OGK_BATCH_ADJ || !b->H ||
        !b->vals)
        return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(ogk_exact_adj_batch, dim3(adj_grid(), 1, b->count), dim3(ADJ_THREADS), 0, stream,
                       (const ogk_args*)b->lanes, b->H, b->vals);
    return (int)hipGetLastError();
}
#endif

#ifdef OGK_HAS_HVP
// the Hessian part's batched mode, under the entry name of the batch parts as the adjoint part's is.  H: the weight
// vectors W[count][m], vals: the result Q[count][n]; the directions are the lane records' h (OGK_BATCH_BIND)
extern "C" int ogk_launch_batch(const ogk_batch_args* b, int mode, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (!b || !b->lanes || b->count < 1 || b->count > b->capacity || b->count > 65535 || mode != OGK_BATCH_HVP || !b->H ||
        !b->vals)
        return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(ogk_exact_hvp_batch, dim3(hvp_grid(), 1, b->count), dim3(HVP_THREADS), 0, stream,
                       (const ogk_args*)b->lanes, b->H, b->vals);
    return (int)hipGetLastError();
}
#endif

#ifdef OGK_HAS_MIX
// the mixed part's batched mode, under the entry name of the batch parts as the adjoint part's is; any other mode is
// another part's.  H: the weight vectors W[count][m], vals: the result S[count][n_par][n] (the lane records hold neither)
extern "C" int ogk_launch_batch(const ogk_batch_args* b, int mode, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (mode != OGK_BATCH_MIX) return OGK_OTHER_PART;
    if (!b || !b->lanes || b->count < 1 || b->count > b->capacity || b->count > 65535 || !b->H || !b->vals)
        return (int)hipErrorInvalidValue;
#ifdef OG_GEN_HAS_PAR
    hipLaunchKernelGGL(ogk_exact_mix_batch, dim3(mix_grid(), OgGen::N_PAR, b->count), dim3(MIX_THREADS), 0, stream,
                       (const ogk_args*)b->lanes, b->H, b->vals);
    return (int)hipGetLastError();
#else
    (void)stream;
    return (int)hipErrorInvalidValue;               // a module without run-time parameters
#endif
}
#endif

#ifdef OGK_HAS_HESS
// the Hessian-matrix part's batched mode, under the entry name of the batch parts as the adjoint part's is; any other mode
// is another part's.  H: the weight vectors W[count][m], vals: the result [count][nnz], X: the device plan, nnz: the
// workgroups of one lane (the lane records hold none of them)
extern "C" int ogk_launch_batch(const ogk_batch_args* b, int mode, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (mode != OGK_BATCH_HESS) return OGK_OTHER_PART;
    if (!b || !b->lanes || b->count < 1 || b->count > b->capacity || b->count > 65535 || !b->H || !b->vals || !b->X ||
        b->nnz < 0 || b->nnz > 0x7fffffff)
        return (int)hipErrorInvalidValue;
    if (b->nnz > 0)
        hipLaunchKernelGGL(ogk_exact_hess_batch, dim3((unsigned)b->nnz, 1, b->count), dim3(HESS_THREADS), 0, stream,
                           (const ogk_args*)b->lanes, (const int*)b->X, b->H, b->vals);
    return (int)hipGetLastError();
}

// terms[n]: items + the nodes of the own collocation block, as og_adj_col counts them.  The tables are device data of
// this module only, so one thread per variable counts on the device (no plan is involved yet) and the counts come back
// with a blocking copy
__global__ __launch_bounds__(256) void ogk_hess_count_terms(int* __restrict__ terms) {
    const int j = (int)(blockIdx.x * 256 + threadIdx.x);
    if (j >= OgGen::N_VAR) return;
    const int4 rec = OGT_COL[j];
    int N = 0;
    if ((rec.w & 0x3fffffff) > rec.z)
        for (int s = 0; s < OgGen::N_MV; ++s) {
            const int leaf = OGT_SLOT[s].v[2], len = OGT_SLOT[s].v[0];
            if (j >= leaf && j < leaf + len) N = len;
        }
    terms[j] = rec.y - rec.x + N;
}

extern "C" int ogk_hess_terms(int32_t* terms) {
    int* d_terms = nullptr;
    hipError_t e = hipMalloc(&d_terms, sizeof(int) * OgGen::N_VAR);
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL(ogk_hess_count_terms, dim3((OgGen::N_VAR + 255) / 256), dim3(256), 0, (hipStream_t)0, d_terms);
    e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpy(terms, d_terms, sizeof(int) * OgGen::N_VAR, hipMemcpyDeviceToHost);
    hipFree(d_terms);
    return (int)e;
}
#endif

#ifdef OGK_HAS_PP
// the parameter-Hessian part's batched mode, under the entry name of the batch parts as the mixed part's is; any other
// mode is another part's.  H: the weight vectors W[count][m], vals: the result S[count][n_par][n_par] (the lane records
// hold neither)
extern "C" int ogk_launch_batch(const ogk_batch_args* b, int mode, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (mode != OGK_BATCH_PP) return OGK_OTHER_PART;
    if (!b || !b->lanes || b->count < 1 || b->count > b->capacity || b->count > 65535 || !b->H || !b->vals)
        return (int)hipErrorInvalidValue;
#ifdef OG_GEN_HAS_PAR
    hipLaunchKernelGGL(ogk_exact_pp_batch, dim3(PP_PAIRS, 1, b->count), dim3(PP_THREADS), 0, stream,
                       (const ogk_args*)b->lanes, b->H, b->vals);
    return (int)hipGetLastError();
#else
    (void)stream;
    return (int)hipErrorInvalidValue;               // a module without run-time parameters
#endif
}
#endif
