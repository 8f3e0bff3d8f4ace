// ogk.h -- internal ABI between libogpsx.so (generic runtime) and a compiled callback module
// libogk_<hash>.so (sweep kernels instantiated for one traced problem).  Not part of the public
// C ABI (include/ogpsx.h); both sides are built from this tree.
#pragma once
#include <stdint.h>

#define OGK_ABI 14
#define OGK_MAX_PHASE 32

// MFMA operand image of a differentiation matrix D (N x N, row-major [k][l]) for
// v_mfma_f64_16x16x4_f64 with the state vectors as A and D^T as B:
//   frag[(nt*KS + ks)*64 + lane] = D[16*nt + (lane & 15)][4*ks + (lane >> 4)]   (0 when padded)
// nt in [0, NT) output-node tiles, ks in [0, KS) steps over the contraction index l.
static inline int ogk_frag_nt(int N) { return (N + 15) / 16; }
static inline int ogk_frag_ks(int N) { return (N + 3) / 4; }
static inline long ogk_frag_size(int N) { return (long)ogk_frag_nt(N) * ogk_frag_ks(N) * 64; }
static inline void ogk_frag_pack(int N, const double* D, double* frag) {
    const int NT = ogk_frag_nt(N), KS = ogk_frag_ks(N);
    for (int nt = 0; nt < NT; ++nt)
        for (int ks = 0; ks < KS; ++ks)
            for (int lane = 0; lane < 64; ++lane) {
                const int k = 16 * nt + (lane & 15), l = 4 * ks + (lane >> 4);
                frag[((long)nt * KS + ks) * 64 + lane] = (k < N && l < N) ? D[(long)k * N + l] : 0.0;
            }
}

#define OGK_OTHER_PART (-4242)   /* ogk_launch: this mode's kernels are in the other part of a two-part module */

// The launch modes of ogk_launch / ogk_launch_batch (what each does: at the two declarations below).  The values of
// OGK_FUSED, OGK_SWEEP and OGK_DENSE are public: og_sweep_mode (include/ogpsx.h) returns them.
enum ogk_mode {
    OGK_EVAL = 0,           // F(x0) and the scratch the sweeps reuse
    OGK_SWEEP = 1,          // structured FD sweep (needs OGK_EVAL at the same x0)
    OGK_DENSE = 2,          // dense FD sweep (validation)
    OGK_EXACT_DENSE = 3,    // exact Jacobian, dense
    OGK_EXACT = 4,          // exact Jacobian with the work lists of the structured sweep
    OGK_FUSED = 5,          // OGK_EVAL + OGK_SWEEP in one launch
    OGK_PATTERN_COUNT = 6,  // the static pattern: entries per column
    OGK_PATTERN_ROWS = 7,   // the static pattern: row indices
    OGK_PACK = 8,           // gather the pattern entries of a block of columns
    OGK_UNPACK = 9,         // scatter packed values into a full matrix
    OGK_COUNT_LAUNCH = 10,  // count one launch into *jt_launches
    OGK_BATCH_FUSED = 11,   // OGK_FUSED for `count` lanes
    OGK_BATCH_EVAL = 12,    // OGK_EVAL for `count` lanes
    OGK_BATCH_BIND = 13,    // bind the caller's arrays to the lane records
    OGK_BATCH_EXACT = 14    // OGK_EXACT for `count` lanes
};

// The two modes of the parameter part (OGK_PART_PAR; macros, so that no other part's text changes): exact dF/dtheta for
// the run-time parameters of one point (ogk_launch) and of `count` lanes (ogk_launch_batch).  Both need an evaluation
// at the same point before them on the same stream (OGK_EVAL / OGK_BATCH_EVAL: y0), write [n_par][m] doubles - every
// one of them, +0.0 where the structure says zero - to args->jt (a lane: to its record's pvals), and touch no
// jt_state / jt_launches word.  A module without parameters answers hipErrorInvalidValue.
#define OGK_PAR_JAC 15
#define OGK_BATCH_PAR_JAC 16

// The two modes of the directional part (OGK_PART_DIR; macros for the same reason): exact directional derivatives
// F'(x) v.  OGK_DIR (ogk_launch): K = col_hi - col_lo directions of one point, direction d read at args->h + d * n (the
// exact path never uses h as a step), its [m] doubles written to args->jt + d * m.  OGK_BATCH_DIR (ogk_launch_batch):
// one direction per lane, the lane record's h, the result at its pvals (OGK_BATCH_BIND with V as H and the output array
// as vals, nnz = m).  Both need an evaluation at the same point before them on the same stream (y0), write every one of
// the m rows, and touch no jt_state / jt_launches word.
#define OGK_DIR 17
#define OGK_BATCH_DIR 18

// The two modes of the adjoint part (OGK_PART_ADJ; macros for the same reason): exact adjoint products F'(x)^T w.
// OGK_ADJ (ogk_launch): K = col_hi - col_lo weight vectors of one point, vector d read at args->h + d * m (the exact path
// never uses h as a step), its [n] doubles written to args->jt + d * n.  OGK_BATCH_ADJ (ogk_launch_batch): one weight
// vector per lane, lane c reads H + c * m and writes vals + c * n of the launch's own ogk_batch_args (OGK_BATCH_BIND
// before it binds X and F0 only: a record's h has the stride of a decision vector).  Both need an evaluation at the same
// point before them on the same stream (y0), write every one of the n entries in the order of sums that og_adj.h fixes,
// and touch no jt_state / jt_launches word.
#define OGK_ADJ 19
#define OGK_BATCH_ADJ 20

// The two modes of the Hessian part (OGK_PART_HVP; macros for the same reason): exact Hessian-vector products
// grad^2 (w . F)(x) v.  OGK_HVP (ogk_launch): K = col_hi - col_lo pairs of one point, weight vector d read at
// args->h + d * m as in OGK_ADJ, direction d at args->pvals + d * n (read only; no packed values travel in this mode),
// its [n] doubles written to args->jt + d * n.  OGK_BATCH_HVP (ogk_launch_batch): one pair per lane, the direction is
// the lane record's h (OGK_BATCH_BIND before it binds X, V as H, and F0), lane c reads its weights at H + c * m and
// writes vals + c * n of the launch's own ogk_batch_args.  Both need an evaluation at the same point before them on the
// same stream (y0), write every one of the n entries in the order of sums that og_adj.h fixes, and touch no
// jt_state / jt_launches word.
#define OGK_HVP 21
#define OGK_BATCH_HVP 22

// The two modes of the mixed part (OGK_PART_MIX; macros for the same reason): exact mixed derivatives
// d(F'(x)^T w)/dtheta_k for every run-time parameter.  OGK_MIX (ogk_launch): K = col_hi - col_lo weight vectors of one
// point, vector d read at args->h + d * m as in OGK_ADJ, its [n_par][n] doubles written to args->jt + d * n_par * n.
// OGK_BATCH_MIX (ogk_launch_batch): one weight vector per lane, lane c reads H + c * m and writes vals + c * n_par * n
// of the launch's own ogk_batch_args (OGK_BATCH_BIND before it binds X and F0 only); every lane at its own parameters,
// its record's cvec.  Both need an evaluation at the same point before them on the same stream (y0), write every one
// of the n_par * n entries in the order of sums that og_adj.h fixes, and touch no jt_state / jt_launches word.  A
// module without parameters answers hipErrorInvalidValue.
#define OGK_MIX 23
#define OGK_BATCH_MIX 24

// The two modes of the Hessian-matrix part (OGK_PART_HESS; macros for the same reason): the exact sparse Hessian of
// w . F, every stored entry of a static pattern (csrc/og_hess.h; the pattern and the entries' term lists are data,
// codegen.HessianPlan, which the runtime uploads as the device plan below).  OGK_HESS (ogk_launch): K = col_hi - col_lo
// weight vectors of one point, vector d read at args->h + d * m as in OGK_ADJ, its [nnz] doubles in pattern order written
// to args->jt + d * nnz; args->prow is the device plan (no packed rows travel in this mode) and uhi - ulo the workgroups
// of one chunk of vectors, OGK_HESS_WORKGROUPS of the plan's head.  OGK_BATCH_HESS
// (ogk_launch_batch): one weight vector per lane, lane c reads H + c * m and writes vals + c * nnz of the launch's own
// ogk_batch_args, whose X is the device plan (cast; OGK_BATCH_BIND before it binds the points) and whose nnz is the
// number of workgroups of one lane; every lane at its own parameters.  Both need an evaluation at the same point before them on the same stream
// (y0), write every stored entry of every vector in the order of sums that og_hess.h fixes, and touch no
// jt_state / jt_launches word.  ogk_hess_terms (exported by this part only): the number of terms of every column, what
// a plan's term numbers are checked against before anything is launched with it.
//
// The device plan, int32 words: [0] nnz, [1] n_light, [2] n_units, [3] [4] [5] the offsets (in words) of tptr, tlist and
// unit, [6] [7] zero; from word 8 on one record {owner, partner, pos, 0} per stored entry - the n_light entries of at
// most OGK_HESS_LIGHT_TERMS listed terms first, grouped by owner, then the others - pos its place in pattern order and
// in the output; tptr[nnz + 1] by pos and tlist as in the plan; unit[n_units + 1]: runs of light entries of ONE owner, at
// most OGK_HESS_UNIT_ENTRIES each (a wavefront's work: the owner's column lookup once per run).
#define OGK_HESS 25
#define OGK_BATCH_HESS 26
#define OGK_HESS_LIGHT_TERMS 64
#define OGK_HESS_UNIT_ENTRIES 16
#define OGK_HESS_HEAD 8
#define OGK_HESS_WORKGROUPS(nnz, n_light, n_units) (((nnz) - (n_light)) + ((n_units) + 3) / 4)   /* four units per workgroup */

// The two modes of the parameter-Hessian part (OGK_PART_PP; macros for the same reason): exact second derivatives
// S_kl = sum_r w_r d2F_r/dtheta_k dtheta_l of w . F in the run-time parameters (csrc/og_pp.h).  OGK_PP (ogk_launch):
// K = col_hi - col_lo weight vectors of one point, vector d read at args->h + d * m as in OGK_ADJ, its [n_par][n_par]
// doubles written to args->jt + d * n_par * n_par.  OGK_BATCH_PP (ogk_launch_batch): one weight vector per lane, lane c
// reads H + c * m and writes vals + c * n_par * n_par of the launch's own ogk_batch_args (OGK_BATCH_BIND before it binds
// X and F0 only); every lane at its own parameters, its record's cvec.  Both need an evaluation at the same point before
// them on the same stream (y0), write every one of the n_par * n_par entries - S[l][k] a copy of S[k][l] - in the order
// of sums that og_adj.h fixes, and touch no jt_state / jt_launches word.  A module without parameters answers
// hipErrorInvalidValue.
#define OGK_PP 27
#define OGK_BATCH_PP 28

// The parts a module is compiled in (-DOGK_PART=<value>, build.py: MODULE_PARTS, BATCH_PART, BATCH_EXACT_PART, PARAMETER_PART,
// DIRECTIONAL_PART, ADJOINT_PART, HESSIAN_PART, MIX_PART, HESSIAN_MATRIX_PART, PP_PART).
// Preprocessor names: csrc/ogk_kernels.hip selects its kernels with them.
#define OGK_PART_MAIN 0         /* <module>.so: OGK_EVAL, OGK_PATTERN_*, OGK_PACK, OGK_UNPACK, OGK_COUNT_LAUNCH */
#define OGK_PART_AUX 1          /* <module>.p3.so: OGK_DENSE, OGK_EXACT_DENSE, OGK_EXACT */
#define OGK_PART_FUSED 2        /* <module>.p1.so: OGK_FUSED */
#define OGK_PART_SWEEP 3        /* <module>.p2.so: OGK_SWEEP */
#define OGK_PART_BATCH 4        /* <module>.batch.so, on demand: OGK_BATCH_FUSED, OGK_BATCH_EVAL, OGK_BATCH_BIND */
#define OGK_PART_BATCH_EXACT 5  /* <module>.batchx.so, on demand: OGK_BATCH_EXACT */
#define OGK_PART_PAR 6          /* <module>.par.so, on demand: OGK_PAR_JAC, OGK_BATCH_PAR_JAC */
#define OGK_PART_DIR 7          /* <module>.dir.so, on demand: OGK_DIR, OGK_BATCH_DIR */
#define OGK_PART_ADJ 8          /* <module>.adj.so, on demand: OGK_ADJ, OGK_BATCH_ADJ */
#define OGK_PART_HVP 9          /* <module>.hvp.so, on demand: OGK_HVP, OGK_BATCH_HVP */
#define OGK_PART_MIX 10         /* <module>.mix.so, on demand: OGK_MIX, OGK_BATCH_MIX */
#define OGK_PART_HESS 11        /* <module>.hess.so, on demand: OGK_HESS, OGK_BATCH_HESS */
#define OGK_PART_PP 12          /* <module>.pp.so, on demand: OGK_PP, OGK_BATCH_PP */

// The words of a handle's (and of every batch lane's) flag block: og_problem_s::d_flags, OGK_FLAG_WORDS ints.
enum ogk_flag {
    OGK_FLAG_COUNT_A = 0,       // two counters of non-finite rows that the two-launch forms use alternately
    OGK_FLAG_COUNT_B = 1,
    OGK_FLAG_TICKET = 2,        // OGK_FUSED: evaluation workgroups that have finished
    OGK_FLAG_FUSED_COUNT = 3,   // OGK_FUSED: non-finite rows of the running launch (zero between launches)
    OGK_FLAG_FUSED_RESULT = 4,  // OGK_FUSED: where its last evaluation workgroup leaves the total
    OGK_FLAG_WORDS = 8
};

#ifdef __cplusplus
static_assert(OGK_FUSED == 5 && OGK_SWEEP == 1 && OGK_DENSE == 2, "og_sweep_mode's values are public (include/ogpsx.h)");
#endif

typedef struct ogk_info {
    int32_t abi;
    int32_t n, m, m_eq, m_ineq;
    int32_t n_phase, n_mv, n_groups, n_cvec;
    int32_t n_y0;           // doubles of scratch for the unperturbed collocation products
    int32_t phase_nodes[OGK_MAX_PHASE];
    int32_t n_eval_blocks;  // evaluation workgroups of one launch (what the OGK_FUSED ticket counts)
    int32_t fused_ok;       // OGK_FUSED runs as ONE launch on this module (its LDS fits); else the caller uses OGK_EVAL + OGK_SWEEP
} ogk_info;

// Run-time parameters: cvec[par_off + i], i in [0, n_par), the tail of the constant table.  The generated functions read
// them like every other table entry; the runtime rewrites them on the device (og_set_parameters, include/ogpsx.h).
// A record of its own, asked for with a call of its own: ogk_info keeps its size.
typedef struct ogk_par_info {
    int32_t n_par, par_off;
} ogk_par_info;

typedef struct ogk_args {
    const double* x0;       // [n] decision vector (device)
    const double* h;        // [n] signed FD steps (device; unused for a plain evaluation)
    const double* dfrag;    // packed D fragments of all phases (device)
    const double* cvec;     // constant table (device, may be NULL when n_cvec == 0); its tail: the run-time parameters
    double* f0;             // [m] F(x0): written by OGK_EVAL, read by OGK_SWEEP and OGK_DENSE
    double* y0;             // [n_y0] base collocation products   (written by OGK_EVAL)
    double* xop;            // [n_y0] base collocation operands   (written by OGK_EVAL)
    double* t0;             // [m] base dynamics terms of defect rows (written by OGK_EVAL)
    double* z;              // [m] F0 - F0: 0, or NaN for non-finite rows (written by OGK_EVAL)
    int* nonfinite;         // number of non-finite rows of F(x0): counted by OGK_EVAL, read by OGK_SWEEP
    int* nonfinite_next;    // the slot the *next* evaluation counts into (OGK_EVAL zeroes it)
    unsigned* ready;        // OGK_FUSED: ticket the evaluation workgroups count into; the last one resets it
    double* jt;             // [(col_hi-col_lo) * m] transposed Jacobian rows (OGK_SWEEP)
    // Persistent-zero output (og_jt_register_dev, include/ogpsx.h).  jt_sparse != 0: the structural zeros of
    // `jt` are known to hold zeros already, so the sweep writes ONLY the positions that can be non-zero (row
    // items and collocation tiles).  The exception is kept on the device, because the asynchronous entry
    // points never learn it - and entirely on the device, so that the launch arguments are the same for
    // every sweep into a buffer (a captured hipGraph can be replayed): jt_launches counts the launches into the
    // buffer; a sweep whose F(x0) has non-finite rows fills its rows completely (NaN where dense FD gives NaN)
    // and stores its own launch number into *jt_state; the next sweep finds *jt_state == its number - 1 and
    // fills completely once more (zeros), which cleans the buffer.  Who counts: the last evaluation workgroup
    // of an OGK_FUSED launch (one thread); thread 0 of an OGK_EVAL launch when jt_bump is set (the evaluation that
    // precedes an OGK_SWEEP / OGK_DENSE / OGK_EXACT launch); a one-thread kernel (OGK_COUNT_LAUNCH) before a lone
    // OGK_SWEEP launch.
    int32_t jt_sparse;
    int32_t jt_bump;        // OGK_EVAL: count one launch into *jt_launches; OGK_UNPACK (of a rank that owns no
                            // columns): mark a NaN fill in *jt_state when F(x0) had non-finite rows
    uint32_t* jt_launches;  // launches into the registered buffer so far
    uint32_t* jt_state;     // number of the last launch into the buffer that left NaN fill behind
    // OGK_FUSED counts the non-finite rows of F(x0) in *nonfinite (zero between launches: its last evaluation
    // workgroup moves the total to *nonfinite_result and clears the counter)
    int* nonfinite_result;
    int32_t col_lo, col_hi; // FD columns handled by this launch
    // Packed non-zeros (OGK_PATTERN_COUNT to OGK_UNPACK).  The static pattern of J_T is the tracer's: column j can be
    // non-zero in the collocation block its state slice owns (N consecutive rows) and at its row items, in that order.
    const int64_t* poff;    // [n] offset of column j's entries in the packed array (OGK_PATTERN_ROWS, OGK_PACK, OGK_UNPACK)
    const int64_t* pind;    // [n+1] the pattern's own prefix sums (OGK_PACK, OGK_UNPACK): column j has pind[j+1]-pind[j] entries
    const int32_t* prow;    // [nnz] row index of every pattern entry, flat (OGK_PACK, OGK_UNPACK): no table walks there
    int32_t* pint;          // OGK_PATTERN_COUNT: [n] entries per column (out); OGK_PATTERN_ROWS: row index of every packed entry (out)
    double* pvals;          // packed values: OGK_PACK writes them, OGK_UNPACK reads them
    double* ptail;          // OGK_PACK: m + 1 doubles that receive F(x0) and the count of non-finite rows, or NULL
    int32_t ulo, uhi;       // OGK_UNPACK: columns to scatter; those inside [col_lo, col_hi) are this rank's own: skipped
    double* trace;          // -DOGK_TRACE builds: [workgroup][8 wavefronts][8] phase stamps (else unused)
    int64_t dfrag_off[OGK_MAX_PHASE];
} ogk_args;

// A batch (og_batch_*, include/ogpsx.h): B points of one problem in one launch, lane = blockIdx.y.  A lane is one
// ogk_args record in a device table that the runtime writes when the batch is created: its own scratch, ticket,
// counters and persistent-zero jt with its own jt_state / jt_launches words; dfrag and the pattern tables are
// the handle's, and so is cvec unless the module has run-time parameters: then every lane has a copy of the constant
// table of its own.  The table holds OGK_BATCH_SETS record sets of `capacity` lanes each: set 0 is what the one-launch
// sweep (OGK_BATCH_FUSED) runs; sets 1 and 2 are what the evaluation (OGK_BATCH_EVAL) runs, with jt_bump = 0 and 1.  What changes
// from call to call - where the caller's X, H, F0 and packed values are - is written into the records by OGK_BATCH_BIND
// (one thread per record) ahead of EVERY OGK_BATCH_FUSED / OGK_BATCH_EVAL launch, stream-ordered before it, so that those launches take
// the table and the lane count only and a captured graph carries its own binding.  OGK_BATCH_BIND also zeroes the non-finite
// counter of the lanes an evaluation is about to run (a lane's count stays where it is while launches run without it).
#define OGK_BATCH_SETS 3
typedef struct ogk_batch_args {
    ogk_args* lanes;        // OGK_BATCH_FUSED, OGK_BATCH_EVAL: the record set to run ([capacity] records); OGK_BATCH_BIND: the whole table
    int32_t count;          // lanes of this launch (<= capacity)
    int32_t capacity;
    // OGK_BATCH_BIND: lane k reads X + k * n (and H + k * n), writes F0 + k * m (and vals + k * nnz; vals may be NULL)
    const double* X;
    const double* H;
    double* F0;
    double* vals;
    int64_t nnz;
    int32_t clear_set;      // OGK_BATCH_BIND: zero *nonfinite of the first `count` records of this set (-1: none)
} ogk_batch_args;

#ifdef __cplusplus
extern "C" {
#endif
// exported by every callback module
int ogk_get_info(ogk_info* out);
int ogk_get_par_info(ogk_par_info* out);    // part 0 (<module>.so) only needs to answer; every part does
// OGK_EVAL: evaluate F(x0) into f0 (+ scratch y0/t0/z).  OGK_SWEEP: structured FD sweep over
// [col_lo, col_hi) into jt (needs OGK_EVAL's outputs at the same x0).  OGK_DENSE: dense FD sweep.
// OGK_EXACT_DENSE / OGK_EXACT: exact Jacobian, dense / structured (needs OGK_EVAL).  OGK_FUSED: OGK_EVAL + OGK_SWEEP
// in one launch.  OGK_PATTERN_COUNT / OGK_PATTERN_ROWS: the static pattern (entries per column / row indices).
// OGK_PACK: gather the pattern entries of the columns [col_lo, col_hi) of `jt` into pvals.  OGK_UNPACK: scatter pvals
// into the rows [ulo, uhi) of a full matrix `jt` (row 0 = column 0), filling those rows from z first when F(x0) has
// non-finite rows or the previous step left such a fill behind.  OGK_COUNT_LAUNCH: count one launch into *jt_launches.
// Only enqueues kernels on `stream`; returns a hipError_t value (0 = success).
int ogk_launch(const ogk_args* args, int mode, void* stream);
// exported by the batch part of a module only (OGK_PART_BATCH, built when a batch is first asked for).
// OGK_BATCH_FUSED: ogk_fused over all n columns for `count` lanes in one launch.  OGK_BATCH_EVAL: ogk_eval for `count`
// lanes.  OGK_BATCH_BIND: bind the caller's arrays to the records (see above).
// The exact batch part (OGK_PART_BATCH_EXACT, <module>.batchx.so, built when a batched exact Jacobian is first asked
// for) exports the same name for its one mode, and ogk_get_info.  OGK_BATCH_EXACT: ogk_exact_struct over all n columns
// for `count` lanes in one launch, on record set 2 after an OGK_BATCH_EVAL launch on the same set (which counts the
// launch into each lane's *jt_launches); every value also goes to its place in the lane's packed array when the
// record's pvals is set.
int ogk_launch_batch(const ogk_batch_args* args, int mode, void* stream);
// exported by the Hessian-matrix part only (OGK_PART_HESS): terms[n], the number of terms of every column of the exact
// Jacobian in the numbering of csrc/og_adj.h (counted on the device from the module's tables, one small blocking launch
// that involves no plan); returns a hipError_t value
int ogk_hess_terms(int32_t* terms);
#ifdef __cplusplus
}
#endif
