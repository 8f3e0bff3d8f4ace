/* ogpsx.h -- C ABI of libogpsx.so, the MI355X (gfx950) pseudospectral NLP evaluation engine.
 *
 * This is the drop-in boundary for the hot path of istellartech/OpenGoddard (SURVEY.md
 * section 8(b)).  The reference has no FFI: its hot path is Python closures that SciPy's SLSQP
 * calls 3n+2 times per major iteration.  Each entry point below names the reference code it
 * replaces (paths relative to the reference checkout; "scipy:" = SciPy 1.15.3's
 * scipy/optimize).  All functions return 0 on success and a non-zero code otherwise;
 * og_last_error() then describes the failure (thread-local string).  Buffers are caller-owned;
 * the library owns only device scratch tied to a handle.  Calls on one handle must not overlap;
 * host-pointer variants block until results are in the caller's buffers.
 */
#ifndef OGPSX_H
#define OGPSX_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define OG_ABI_VERSION 1

typedef struct og_problem_s* og_handle;

/* ---- LGL discretisation ------------------------------------------------------------------
 * Replaces Problem._nodes_LGL / _weight_LGL / _differentiation_matrix_LGL
 * (OpenGoddard/optimize.py:183-213).  tau[N], w[N], D[N*N] row-major.  N >= 3.
 * og_lgl runs on the host; og_lgl_dev runs the HIP kernel on the current device and writes to
 * device pointers (stream may be NULL).  Both produce identical bits. */
int og_lgl(int32_t N, double* tau, double* w, double* D);
int og_lgl_dev(int32_t N, double* d_tau, double* d_w, double* d_D, void* hip_stream);

/* ---- finite-difference step rule -----------------------------------------------------------
 * Replaces the step selection SciPy applies before the column loop (scipy:_numdiff.py:500-515
 * with _adjust_scheme_to_bounds '1-sided', scipy:_numdiff.py:44-70; absolute step
 * 1.4901161193847656e-08 from scipy:_slsqp_py.py:33).  lb/ub use -inf/+inf for "no bound".
 * Writes the signed step h[n]. */
int og_fd_step(int32_t n, const double* x, const double* lb, const double* ub, double* h);

/* ---- problem handle ------------------------------------------------------------------------
 * A handle binds one compiled callback module (the traced dynamics / equality / inequality /
 * cost of one Problem, built by opengoddard_amd.codegen) to a device.  Replaces the closure
 * construction in Problem.solve (OpenGoddard/optimize.py:670-733). */
typedef struct og_desc {
    int32_t abi_version;        /* OG_ABI_VERSION */
    int32_t device;             /* HIP device ordinal */
    int32_t n;                  /* decision variables */
    int32_t m_eq;               /* equality rows (user + defects + knots) */
    int32_t m_ineq;             /* inequality rows */
    int32_t n_phase;
    const int32_t* nodes;       /* [n_phase] LGL nodes per phase */
    const double* const* D;     /* [n_phase] row-major N x N matrices, or NULL: use og_lgl */
    const double* cvec;         /* constant table referenced by the module (may be NULL) */
    int32_t n_cvec;
    const char* module_path;    /* path of the compiled callback module (libogk_<hash>.so) */
} og_desc;

int og_problem_create(const og_desc* desc, og_handle* out);
void og_problem_destroy(og_handle h);

/* Sizes of a handle: n, m = 1 + m_eq + m_ineq, m_eq, m_ineq. */
int og_problem_dims(og_handle h, int32_t* n, int32_t* m, int32_t* m_eq, int32_t* m_ineq);

/* How og_fd_sweep(_dev) runs on this handle: 5 = evaluation and structured sweep in ONE launch (ogk_fused),
 * 1 = the same two kernels as two launches, 2 = evaluation + literal dense sweep (validation).  Chosen at
 * og_problem_create: OGPSX_SWEEP=fused|split|dense; the default is 5 at every size (og_one_launch: whether
 * that is one launch on this handle).  The one-launch form writes
 * the non-zeros only, so it needs a persistent-zero output (og_jt_register_dev / _host; the host-pointer entry
 * points register their own staging buffer): a sweep into an unregistered device buffer runs as the two launches
 * of mode 1 from the same handle, with identical results.
 * No reference counterpart: SciPy's approx_derivative has one way to run (scipy/optimize/_numdiff.py:584-625). */
int og_sweep_mode(og_handle h);

/* The launch form og_sweep_mode == 5 actually takes on this handle: 1 = evaluation and sweep in ONE launch, 0 = two.
 * The one-launch kernel keeps a tile's D panel, the operands and the base products of the longest phase in LDS: a
 * module whose longest phase passes that window (ogk_info.fused_ok; opengoddard_amd.codegen.lds_window states the
 * arithmetic: at 1 / 2 / 6 / 16 states per phase and no running cost the last node counts that fit are 452 / 408 /
 * 292 / 168) keeps og_sweep_mode == 5 and runs every sweep as the two launches of mode 1, the registered host matrix
 * as a full download, og_shard_sweep_dev as sweep + pack and a batch as one batched evaluation + one sweep per lane -
 * with the same bits.  Also 0 under OGPSX_SWEEP=split|dense.  A captured graph of the two-launch form can be replayed
 * like the one-launch form (the capture clears the count of non-finite rows itself).
 * No reference counterpart (see og_sweep_mode). */
int og_one_launch(og_handle h);

/* *rows = the number of non-finite rows of F(x0) that the most recent evaluation, sweep or exact Jacobian enqueued on
 * this handle counted (what makes a sweep fill those rows of J_T with NaN); waits for `hip_stream`, the stream that
 * call was given.  After replays of a captured graph: the count of the last replay, if the captured call was the
 * handle's most recent one.  No reference counterpart: SciPy's dense differences carry the NaN themselves. */
int og_nonfinite_rows(og_handle h, void* hip_stream, int32_t* rows);

/* ---- single evaluation ---------------------------------------------------------------------
 * F(x) = [cost | c_eq | c_ineq], m doubles.  Replaces one call each of cost_add, equality_add
 * and the user inequality (OpenGoddard/optimize.py:670-709, 723-728). */
int og_eval(og_handle h, const double* x, double* F);

/* ---- forward-difference sweep --------------------------------------------------------------
 * Transposed Jacobian rows for decision-vector columns [col_lo, col_hi):
 *     JT[(j - col_lo) * m + r] = (F_r(x + h_j e_j) - F_r(x)) / ((x_j + h_j) - x_j)
 * i.e. exactly SciPy's J_transposed (scipy:_numdiff.py:584-625) for the stacked function
 * [cost | c_eq | c_ineq]; column 0 of a row is the cost gradient entry, columns 1..m_eq the
 * equality Jacobian, the rest the inequality Jacobian.  Also returns F(x) in F0 (may be NULL).
 * Replaces the 3n+2 Python callback evaluations of one SLSQP major iteration
 * (scipy:_slsqp_py.py:299-313, 438-440). */
int og_fd_sweep(og_handle h, const double* x, const double* hstep,
                int32_t col_lo, int32_t col_hi, double* JT, double* F0);

/* Device-pointer variants: all pointers are device memory on the handle's device (for example
 * torch.Tensor.data_ptr()), hip_stream is a hipStream_t (NULL = default stream).  Asynchronous:
 * they only enqueue work.  d_F0 must hold m doubles, d_JT (col_hi-col_lo)*m doubles. */
int og_eval_dev(og_handle h, const double* d_x, double* d_F, void* hip_stream);
int og_fd_sweep_dev(og_handle h, const double* d_x, const double* d_hstep,
                    int32_t col_lo, int32_t col_hi, double* d_JT, double* d_F0,
                    void* hip_stream);

/* Columns only: like og_fd_sweep_dev but d_F0 is an *input* that must already hold F(x) from
 * the most recent og_eval_dev on this handle at the same x (that call also refreshes the
 * handle's sweep scratch).  One kernel launch; this is the unit bench.py times for the
 * roofline figure.
 *
 * Environment: OGPSX_SWEEP=dense (read when a handle is created) selects the literal dense
 * sweep - every row re-evaluated for every column - instead of the default structured sweep
 * that only re-evaluates rows reading the perturbed variable.  Results are identical. */
int og_fd_columns_dev(og_handle h, const double* d_x, const double* d_hstep,
                      int32_t col_lo, int32_t col_hi, double* d_JT, const double* d_F0,
                      void* hip_stream);

/* ---- persistent-zero output buffers ------------------------------------------------------------
 * Most of J_T is structurally zero (a row of F reads a handful of decision variables; the pattern is
 * fixed by the traced callbacks), and SciPy's dense loop recomputes those zeros as (F0 - F0)/dx for
 * every column of every sweep (scipy:_numdiff.py:592-620).  A caller that keeps ONE output buffer per
 * block of columns can register it: og_jt_register_dev zero-fills d_JT ((col_hi-col_lo)*m doubles,
 * enqueued on hip_stream) and from then on og_fd_sweep_dev / og_fd_columns_dev / og_jacobian_exact_dev
 * called with exactly (d_JT, col_lo, col_hi) write only the entries that can be non-zero.  The result
 * in the buffer is the same matrix, entry for entry, as without registration - including sweeps at
 * points where F(x) has non-finite rows (those rows become NaN in every column, as dense differencing
 * makes them; the library re-cleans the buffer on the next sweep by itself).  Contract: between
 * sweeps the caller only reads the buffer; work on it must be stream-ordered after the registration.
 * At most 63 registrations per handle; the host-pointer entry points register their own staging
 * buffer.  No reference counterpart (the reference allocates a fresh dense array per sweep). */
int og_jt_register_dev(og_handle h, double* d_JT, int32_t col_lo, int32_t col_hi, void* hip_stream);
int og_jt_unregister_dev(og_handle h, double* d_JT);

/* The same for a host matrix handed to og_fd_sweep / og_jacobian_exact: og_jt_register_host zero-fills JT
 * ((col_hi-col_lo)*m doubles) and later calls with exactly (JT, col_lo, col_hi) transfer only the packed
 * non-zeros (plus F and the count of non-finite rows, one pinned copy) and scatter them on the host; a sweep
 * with non-finite rows transfers the dense block, and the next call re-zeroes the matrix first.  Contract as
 * above: the caller only reads JT between calls.  This is what Problem.solve uses: SciPy's SLSQP copies the
 * Jacobian it is handed (scipy:_slsqp_py.py:490-511), so one persistent matrix serves every major iteration.
 * Round 6: the registration page-locks JT and maps it into the device's address space (hipHostRegister; undone by
 * og_jt_unregister_host / og_problem_destroy, which must come before the matrix is freed), and og_fd_sweep's one
 * launch then writes the structural non-zeros straight into JT over PCIe - no packed copy, no host scatter (C3:
 * 0.097 -> 0.047 ms per call, C4 0.21 -> 0.088, C5 0.38 -> 0.17; x and h are read in place too, out of a pinned
 * buffer of the handle, instead of being copied first) - under the same persistent-zero protocol as a
 * device buffer (a NaN fill is cleaned by the next sweep).  Where the host refuses the mapping (or OGPSX_HOST=staged)
 * the packed transfer + scatter above is what runs; the matrix in JT is the same either way. */
int og_jt_register_host(og_handle h, double* JT, int32_t col_lo, int32_t col_hi);
/* Which of the two serves og_fd_sweep into the registered host matrix JT: *path = 1 the mapped matrix (the launch writes
 * it over PCIe), 2 the packed copy + host scatter, 0 not decided yet (the first ten sweeps time both - two warm-ups and
 * three timed calls each - and keep the faster: what scattered device writes into host pages cost is the host's doing;
 * on every box of round 6 mapped won, 0.043-0.052 against 0.10-0.12 ms per sweep at C3), 3 neither: both belong to the
 * one-launch form, and a handle without it (og_one_launch == 0) sweeps into its own device matrix and downloads the whole
 * block, -1 JT is not registered.
 * OGPSX_HOST=mapped | staged in the environment decide without the trial.  No reference counterpart. */
int og_jt_host_path(og_handle h, const double* JT, int32_t* path);
/* Page-locked host memory from the HIP runtime (hipHostMalloc) for a matrix that is going to be registered with
 * og_jt_register_host: it is mapped into the device's address space already and lies in the driver's large fragments, so
 * the mapped path needs a handful of address translations per sweep where a malloc'ed matrix of 4 KB pages needs
 * thousands (the engine's own persistent matrix comes from here).  No reference counterpart. */
int og_pinned_alloc(int64_t bytes, void** out);
int og_pinned_free(void* ptr);
int og_jt_unregister_host(og_handle h, double* JT);

/* ---- static pattern and packed non-zeros ---------------------------------------------------------
 * Which entries of J_T can be non-zero is fixed by the traced callbacks: column j reads the collocation
 * block its state slice owns (N consecutive defect rows) and a list of row items.  og_pattern returns that
 * pattern for the columns [col_lo, col_hi) as CSR over columns: *nnz entries, indptr[col_hi-col_lo+1]
 * (relative to the block), rows[*nnz]; any output pointer may be NULL.  og_pack_dev gathers exactly those
 * entries of a dense block (d_JT: (col_hi-col_lo) x m) into d_vals (*nnz doubles, pattern order);
 * og_unpack_dev scatters them back into a dense block whose other entries it leaves alone.  No reference
 * counterpart: the reference's Jacobian is dense (scipy:_numdiff.py:587). */
int og_pattern(og_handle h, int32_t col_lo, int32_t col_hi, int64_t* nnz, int64_t* indptr, int32_t* rows);
int og_pack_dev(og_handle h, const double* d_JT, int32_t col_lo, int32_t col_hi, double* d_vals, void* hip_stream);
int og_unpack_dev(og_handle h, const double* d_vals, int32_t col_lo, int32_t col_hi, double* d_JT, void* hip_stream);

/* ---- column sharding across GPUs ------------------------------------------
 * The n forward-difference columns are independent given x (scipy:_numdiff.py:592-620 has no cross-iteration
 * dependency): rank r of `world` sweeps the block [r*B, min(n, (r+1)*B)), B = ceil(n/world), into ITS rows of
 * a full n x m replica that was zeroed once (register the block: og_jt_register_dev(h, d_JT_full + r*B*m,
 * r*B, ...)), and the ranks exchange only the packed non-zeros: og_shard_plan fixes the layout (*block_vals =
 * doubles per rank's message, padded to the largest block so that one all-gather of equal messages does it);
 * og_shard_pack_dev gathers this rank's non-zeros into d_send (*block_vals doubles); after the all-gather
 * (RCCL ncclAllGather / torch.distributed.all_gather_into_tensor; world * *block_vals doubles in d_recv)
 * og_shard_unpack_dev scatters every other rank's non-zeros into the replica.  When F(x) has non-finite rows,
 * or had in the previous step, the rows of the other ranks are filled from this rank's own F(x) - F(x)
 * first (every rank evaluates the same F(x)), so the replica equals the single-GPU result in that case too.
 * Call order per step on one stream: og_fd_sweep_dev (own block), og_shard_pack_dev, all-gather,
 * og_shard_unpack_dev.  Results are bitwise independent of `world`.  A rank that owns no columns (more ranks
 * than blocks of B columns) evaluates F(x) only (og_shard_sweep_dev / og_eval_dev) and og_shard_unpack_dev keeps
 * the NaN history of its replica in a pair of device words of its own. */
int og_shard_plan(og_handle h, int32_t world, int32_t* block_cols, int64_t* block_vals);
/* The all-gather itself, for one process per GPU, on the caller's stream with no detour through another
 * runtime's streams: rank 0 makes a unique id (og_shard_comm_unique_id: 128 bytes = ncclGetUniqueId), the
 * launcher hands it to every rank (bench.py: torch.distributed.broadcast), every rank calls og_shard_comm_init
 * (ncclCommInitRank on the handle's device; also makes the shard plan for `world`), and per step
 * og_shard_all_gather_dev = ncclAllGather of *block_vals doubles from d_send into d_recv (world * *block_vals).
 * librccl is resolved at run time (the copy already in the process wins).  og_problem_destroy destroys the
 * communicator. */
int og_shard_comm_unique_id(uint8_t* id128);
int og_shard_comm_init(og_handle h, const uint8_t* id128, int32_t rank, int32_t world);
void og_shard_comm_destroy(og_handle h);
/* What RCCL reports about the handle's communicator: ncclCommCount, ncclCommUserRank, ncclCommCuDevice - so that a
 * launcher (bench.py --gpus N) can print that the all-gather really spans N ranks on N devices.  (No reference
 * counterpart: the reference has no multi-device path) */
int og_shard_comm_info(og_handle h, int32_t* nranks, int32_t* rank, int32_t* device);
int og_shard_all_gather_dev(og_handle h, const double* d_send, double* d_recv, void* hip_stream);
int og_shard_pack_dev(og_handle h, int32_t rank, const double* d_JT_block, double* d_send, void* hip_stream);
/* og_fd_sweep_dev of rank's block and og_shard_pack_dev in ONE launch: the sweep kernel stores every non-zero
 * into the block of the replica and into the message (needs the block registered; otherwise it runs the two
 * calls). */
int og_shard_sweep_dev(og_handle h, int32_t rank, const double* d_x, const double* d_hstep, double* d_JT_block,
                       double* d_F0, double* d_send, void* hip_stream);
int og_shard_unpack_dev(og_handle h, int32_t rank, const double* d_recv, double* d_JT_full, void* hip_stream);

/* ---- several GPUs of one node from one process ---------------------------------------------------
 * og_comm_init(G, devs) names the devices the sharded handles use and brings up one RCCL communicator per
 * device (ncclCommInitAll; librccl is loaded at run time - a copy already in the process, e.g. torch's, is
 * reused).  OGPSX_GATHER=peer exchanges the packed blocks with hipMemcpyPeerAsync instead (the reported
 * alternative of SURVEY.md section 8(e); it also allows listing one device several times, which is how the
 * single-GPU test box exercises G > 1), OGPSX_GATHER=rccl makes a missing librccl an error.
 * og_multi_create makes one sub-handle, one stream and one zero-initialised n x m replica of J_T per device
 * (desc->device is ignored).  og_multi_fd_sweep = og_fd_sweep over all n columns, the columns split in G
 * contiguous blocks, the packed non-zeros exchanged by one grouped ncclAllGather over xGMI, the host result
 * (JT: n x m, may be registered with og_multi_jt_register_host; F0 may be NULL) taken from device 0.
 * og_multi_fd_sweep_enqueue does the same without the download and without synchronising: afterwards every
 * device's replica (og_multi_replica_dev: device pointers + the device's stream) holds the whole matrix, for
 * device-side consumers such as the SQP core.  Bitwise the same matrix as a single-device sweep for any G.
 * Replaces the same 3n+2 callback evaluations as og_fd_sweep (scipy:_slsqp_py.py:299-313). */
typedef struct og_multi_s* og_multi;
int og_comm_init(int32_t G, const int32_t* devs);
void og_comm_finalize(void);
int og_comm_size(void);          /* devices named by the last og_comm_init (0: none) */
int og_comm_uses_rccl(void);     /* 1: ncclAllGather, 0: peer copies */
int og_multi_create(const og_desc* desc, og_multi* out);
void og_multi_destroy(og_multi mh);
int og_multi_devices(og_multi mh);
int og_multi_eval(og_multi mh, const double* x, double* F);
int og_multi_fd_sweep(og_multi mh, const double* x, const double* hstep, double* JT, double* F0);
int og_multi_fd_sweep_enqueue(og_multi mh, const double* x, const double* hstep);
int og_multi_synchronize(og_multi mh);
int og_multi_replica_dev(og_multi mh, int32_t g, double** d_JT_full, double** d_F0, void** hip_stream);
int og_multi_jt_register_host(og_multi mh, double* JT);

/* ---- a batch of points of one problem (one device) ------------------------------------------------
 * Everything above works at ONE decision vector; screening initial guesses, evaluating a dispersed family of
 * trajectories or scanning a parameter means many.  A batch is tied to a handle and owns `capacity` lanes: per lane the
 * sweep scratch, F(x), a persistent-zero n x m J_T of its own (zeroed here, never to be written by the caller) and its
 * device words.  One call serves `count` <= capacity points: lane k works at X[k] (row k of a [count][n] array) and the
 * results of a lane are, bit for bit, what og_eval / og_fd_sweep over all n columns give at that point on the same
 * handle - lanes share nothing but the problem, down to the non-finite protocol (a lane whose F(x) has non-finite rows
 * fills ITS matrix with NaN in those rows and cleans it in its next sweep).  The kernels live in a part of the callback
 * module that is built and loaded only for this (batch_part_path: opengoddard_amd.build.build_batch_part; may be NULL
 * once a batch of the handle has loaded it).  How the sweep runs follows og_sweep_mode: 5 = one launch for all lanes,
 * 1 / 2 = one batched evaluation and the handle's sweep kernel per lane (validation).  Every call first enqueues one small
 * launch that tells the lanes where this call's arrays are (no such state is kept on the host), so a call costs two
 * launches and a captured graph of it can be replayed between calls on other arrays.  og_batch_create reports lanes
 * that do not fit the device's memory as an error.  og_problem_destroy destroys the batches of its handle; calls on
 * such a batch fail.  Calls on one batch, and on a batch and its handle, must not overlap.
 * og_batch_create / _destroy / _capacity / _lane_dev have no reference counterpart (the reference has one Problem and
 * one solve at one point at a time). */
typedef struct og_batch_s* og_batch;
int og_batch_create(og_handle h, int32_t capacity, const char* batch_part_path, og_batch* out);
void og_batch_destroy(og_batch b);
int og_batch_capacity(og_batch b);
/* Device pointers on the handle's device, asynchronous.  d_X: [count][n]; d_F: [count][m] receives F(X[k]).  Replaces
 * count times one call each of cost_add, equality_add and the user inequality (OpenGoddard/optimize.py:670-709,
 * 723-728). */
int og_batch_eval_dev(og_batch b, int32_t count, const double* d_X, double* d_F, void* hip_stream);
/* The forward-difference sweep over all n columns at every point.  d_H: [count][n] signed steps (og_fd_step per point);
 * d_F0: [count][m]; d_vals: [count][nnz] receives each lane's structural non-zeros in og_pattern's order (the pattern
 * of the columns [0, n)), or NULL.  The dense matrix of lane k stays in the batch (og_batch_lane_dev).  Replaces count
 * times the 3n+2 callback evaluations of one SLSQP major iteration (scipy:_slsqp_py.py:299-313). */
int og_batch_fd_sweep_dev(og_batch b, int32_t count, const double* d_X, const double* d_H, double* d_F0,
                          double* d_vals, void* hip_stream);
/* Lane `lane` of the batch: *d_JT its n x m matrix on the device (JT[j * m + r], as og_fd_sweep over [0, n) lays it out;
 * valid as long as the batch), *nonfinite_rows the number of non-finite rows of F at the lane's most recent point
 * (this one waits for the stream of the batch's most recent call, not for the device; the count is the lane's own: calls
 * that run fewer lanes leave it alone).  Either pointer may be NULL. */
int og_batch_lane_dev(og_batch b, int32_t lane, double** d_JT, int32_t* nonfinite_rows);
/* Host pointers, blocking.  X, H: [count][n]; F, F0: [count][m]; vals: [count][nnz]; nonfinite: [count] or NULL.  The
 * host form returns the packed non-zeros, not count dense matrices.  The packed form cannot carry a NaN fill of
 * structural zeros: a lane whose F(x) has non-finite rows is reported in nonfinite[k] (the number of such rows), its
 * vals[k] hold what the sweep computed at the pattern's entries only, and its dense matrix - NaN in those rows of
 * every column, as dense differencing makes them - is read from the lane (og_batch_lane_dev + og_device_read).
 * When F0 and vals both lie in page-locked memory the device can address (og_pinned_alloc) the launch writes them in
 * place over PCIe; otherwise they come down through the batch's staging buffers (same values).
 * Replace the same reference code as the device forms. */
int og_batch_eval(og_batch b, int32_t count, const double* X, double* F);
int og_batch_fd_sweep(og_batch b, int32_t count, const double* X, const double* H, double* F0, double* vals,
                      int32_t* nonfinite);

/* ---- exact Jacobian (opt-in, changes the numbers SLSQP sees) ---
 * Same layout as the sweep: JT[(j - col_lo) * m + r] = dF_r/dx_j, but by forward-mode
 * differentiation of the traced callbacks (no step h, no subtraction, no FD noise; where a callback
 * is not differentiable - np.where / maximum at the switch, a table knot - the derivative of the
 * branch F(x) itself takes).  Replaces the same 3n+2 evaluations of `approx_derivative`
 * (`scipy/optimize/_slsqp_py.py:299-313`) as og_fd_sweep; F0 as there. */
int og_jacobian_exact(og_handle h, const double* x, int32_t col_lo, int32_t col_hi, double* JT, double* F0);
int og_jacobian_exact_dev(og_handle h, const double* d_x, int32_t col_lo, int32_t col_hi, double* d_JT,
                          double* d_F0, void* hip_stream);

/* ---- exact Jacobian of a batch of points -----------------------------------------------------------
 * og_jacobian_exact_batch(_dev) is og_jacobian_exact(_dev) over all n columns at `count` points of a batch in one call:
 * three launches whatever `count` is (where the arrays are, the batched evaluation, the batched derivative kernel, which
 * also writes every lane's packed non-zeros) in place of count times og_jacobian_exact_dev + og_pack_dev.  Lane k's F0,
 * packed values and dense matrix (og_batch_lane_dev) are, bit for bit, what the single-point path gives at X[k]; per
 * point it replaces the same 3n+2 evaluations of `approx_derivative` (`scipy/optimize/_slsqp_py.py:299-313`).
 * NaN rule: a lane's results are the single-point path's at that point - F0 with its non-finite rows, nonfinite[k]
 * their count, and in the matrix what the exact kernel computes there (it does not fill rows with NaN as the FD sweep
 * does).  A lane that an FD sweep at a bad point left with a NaN fill is cleaned by its next exact call.
 * Load rule: the kernel lives in a part of the callback module of its own, neither in the module nor in the batch part
 * (exact_part_path: opengoddard_amd.build.build_batch_exact_part).  og_jacobian_exact_batch_load loads it once per
 * handle - a later call on any batch of the handle is a no-op and may pass NULL - and og_problem_destroy closes it;
 * error 4: the part is missing or cannot be loaded, 5: it belongs to another module.  The other two fail with error 4
 * while it is not loaded, except under OGPSX_SWEEP=dense, the validation form (batched evaluation, then the handle's
 * dense exact kernel and the pack lane by lane), which does not need it.
 * _dev: device pointers, asynchronous on hip_stream, capturable; d_X [count][n], d_F0 [count][m], d_vals [count][nnz]
 * in og_pattern's order or NULL (the lanes' matrices are then the result).  Host form: blocking; F0 and vals are
 * written in place when both lie in page-locked memory the device can address, staged otherwise; nonfinite: [count]
 * or NULL. */
int og_jacobian_exact_batch_load(og_batch b, const char* exact_part_path);
int og_jacobian_exact_batch_dev(og_batch b, int32_t count, const double* d_X, double* d_F0, double* d_vals,
                                void* hip_stream);
int og_jacobian_exact_batch(og_batch b, int32_t count, const double* X, double* F0, double* vals,
                            int32_t* nonfinite);

/* ---- run-time parameters --------------------------------------------------------------------------
 * A problem may declare scalar model constants as PARAMETERS (opengoddard_amd: Problem.parameter): the generated
 * functions then read them from the tail of the constant table - cvec[n_cvec - n_par + i] is parameter i, in the order
 * of declaration - instead of carrying them as literals, and the calls below rewrite that tail on the device.  A trade
 * study or a continuation in a constant then runs on ONE module: no trace, no compiler between two values.  The
 * pattern, the registered persistent-zero buffers and the mapped-host path are structural and stay as they are; every
 * later evaluation and sweep of the handle reads the new values.  NaN and infinities are legal values (rows that
 * become non-finite follow the non-finite protocol of the sweep).
 * og_parameter_count: n_par of the handle's module (0: it declares none).
 * og_set_parameters: host pointer, blocking, ordered after everything the device was asked for before (it synchronises
 * the device).  og_set_parameters_dev: d_theta[n_par] on the handle's device, asynchronous on hip_stream, capturable:
 * one small launch of the runtime (one double per thread).  count must be n_par: anything else is hipErrorInvalidValue
 * (1) with a message in og_last_error; on a handle without parameters count = 0 (and d_theta = NULL) succeed and do
 * nothing.  Both also rewrite every lane of every batch of the handle: a handle-level set reaches everything.
 * og_get_parameters: the values on the device now (blocking).
 * A batch of a module with parameters gives every lane a copy of the constant table of its own (capacity x n_cvec
 * doubles, made by og_batch_create from the handle's current table; without parameters the lanes share the handle's).
 * og_parameters_batch_dev scatters d_TH[count][n_par] into the tails of lanes 0 .. count-1 in one launch; lanes count ..
 * capacity-1 keep what they had.  d_TH = NULL: EVERY lane of the batch takes the handle's current values.  The lanes'
 * parameters are device state, like a lane's J_T: they hold until the next such call or the next og_set_parameters(_dev)
 * of the handle, the host keeps no copy, and a captured graph of {og_parameters_batch_dev, og_batch_fd_sweep_dev}
 * replays on new contents of d_TH.  og_parameters_batch: host pointer (or NULL), blocking.  The rule of the batch calls
 * stands: calls on a batch and on its handle must not overlap.
 * og_multi_set_parameters: og_set_parameters on every sub-handle of a multi-device handle.
 * (og_parameters_batch*, like og_jacobian_exact_batch*, are calls ON a batch that are named after what they do: the
 * og_batch_ prefix stays the closed set of the section above.)
 * None of these has a reference counterpart: the reference reads its constants as attributes of a Python object at
 * every callback evaluation (OpenGoddard/optimize.py:670-733 call the user's functions with `obj`), so changing one is
 * an attribute assignment there; here it is what saves a second trace and a second compilation. */
int og_parameter_count(og_handle h);
int og_set_parameters(og_handle h, const double* theta, int32_t count);
int og_set_parameters_dev(og_handle h, const double* d_theta, void* hip_stream);
int og_get_parameters(og_handle h, double* theta, int32_t count);
int og_parameters_batch_dev(og_batch b, int32_t count, const double* d_TH, void* hip_stream);
int og_parameters_batch(og_batch b, int32_t count, const double* TH);
int og_multi_set_parameters(og_multi mh, const double* theta, int32_t count);

/* ---- exact dF/dtheta for the run-time parameters ------------------------------------------------
 * dF[k][r] = d F_r / d theta_k of F = [cost | c_eq | c_ineq], [n_par][m] row-major and dense, by forward-mode
 * differentiation of the traced callbacks with the unit seed on the parameter's table entry (as og_jacobian_exact has it
 * on a decision variable): no step and no forward-difference noise.  Every call writes all n_par * m doubles, an exact
 * +0.0 wherever the structure says the row cannot read the parameter (opengoddard_amd.codegen.parameter_sparsity).
 * Load rule: the kernels live in a part of the callback module of its own (par_part_path:
 * opengoddard_amd.build.build_parameter_part).  og_parameter_jacobian_load loads it once per handle - a later call is a
 * no-op and may pass NULL - and og_problem_destroy closes it; error 4: the part is missing or cannot be loaded, 5: it
 * belongs to another module.  The other four fail with error 4 while it is not loaded, and all five with error 1 (and a
 * message in og_last_error) on a handle whose module has no parameters.
 * og_parameter_jacobian_dev: two launches on hip_stream - the evaluation at d_x (F into d_F0, or into the handle's own
 * array when d_F0 is NULL; og_nonfinite_rows counts its non-finite rows) and the derivative kernel, one workgroup per
 * parameter.  Asynchronous and capturable like og_set_parameters_dev: a captured graph {og_set_parameters_dev,
 * og_parameter_jacobian_dev} replays on new contents of d_theta and d_x.  No J_T is written and no registered buffer's
 * bookkeeping moves.  A non-finite parameter gives what the dual-number rules give (NaN where the parameter enters a
 * product); the next call at finite values is clean.
 * og_parameter_jacobian: host pointers, blocking; F0 may be NULL.
 * The batched forms: lane k works at X[k] and at the lane's own parameters (og_parameters_batch*), and writes
 * dF[k][n_par][m] and F0[k][m] (d_F0 / F0 may be NULL); bit for bit the single-point call at that point and those
 * values.  Three launches whatever count is: bind, the batched evaluation, the derivative kernel.  Lanes count ..
 * capacity-1, their slices of the output and every lane's J_T with its state words are not touched.
 * A multi-device handle (og_multi_*) has no form of this call and does not split it: the result is n_par * m doubles, and
 * the handle of the first device serves it (with og_multi_set_parameters keeping its parameters in step).
 * No reference counterpart: the reference has no derivative with respect to a model constant at all. */
int og_parameter_jacobian_load(og_handle h, const char* par_part_path);
int og_parameter_jacobian_dev(og_handle h, const double* d_x, double* d_dF, double* d_F0, void* hip_stream);
int og_parameter_jacobian(og_handle h, const double* x, double* dF, double* F0);
int og_parameter_jacobian_batch_dev(og_batch b, int32_t count, const double* d_X, double* d_F0, double* d_dF,
                                    void* hip_stream);
int og_parameter_jacobian_batch(og_batch b, int32_t count, const double* X, double* F0, double* dF);

/* ---- exact directional derivatives F'(x) v ---------------------------------------------------------
 * dF[d][r] = sum_j dF_r/dx_j V[d][j] of F = [cost | c_eq | c_ineq], [k][m] row-major and dense, for k directions V[k][n]
 * in the decision vector, WITHOUT forming the Jacobian: one forward-mode pass of the traced callbacks with the seed
 * V[d][i] on variable i (og_jacobian_exact has a unit seed on one variable at a time) - the work of one evaluation on
 * dual numbers per direction, no pattern, no J_T, no n x m memory, no step.  Every call writes all k * m doubles.  A
 * run-time parameter is a constant along v; a direction in parameter space is, by linearity, sum_k w_k dF/dtheta_k from
 * og_parameter_jacobian.  At a switch of the callbacks the derivative is that of the branch F(x) takes, as everywhere in
 * the exact mode.
 * Load rule: the kernels live in a part of the callback module of its own (dir_part_path:
 * opengoddard_amd.build.build_directional_part), for a module with or without parameters.  og_directional_load loads
 * it once per handle - a later call is a no-op and may pass NULL - and og_problem_destroy closes it; error 4: the part
 * is missing or cannot be loaded, 5: it belongs to another module.  The other four fail with error 4 while it is not
 * loaded, and with error 1 (and a message in og_last_error) for null pointers, k < 1 or k > 65535, or a count outside
 * 1 .. capacity.
 * og_directional_dev: two launches on hip_stream - the evaluation at d_x (F into d_F0, or into the handle's own array
 * when d_F0 is NULL; og_nonfinite_rows counts its non-finite rows) and the derivative kernel, one thread per row and
 * direction.  Asynchronous and capturable: a captured graph replays on new contents of d_x and d_V.  No J_T is written
 * and no registered buffer's bookkeeping moves.  Direction d of a call with k directions is bit for bit the call with
 * that direction alone.
 * og_directional: host pointers, blocking; F0 may be NULL.
 * The batched forms: lane c works at X[c], along V[c] - ONE direction per lane; repeat a point for more - and at the
 * lane's own parameters (og_parameters_batch*), and writes dF[c][m] and F0[c][m] (d_F0 / F0 may be NULL); bit for bit
 * the single-point call at that point, direction and those values.  Three launches whatever count is: bind, the batched
 * evaluation, the derivative kernel.  Lanes count .. capacity-1, their slices of the output and every lane's J_T with
 * its state words are not touched.
 * A multi-device handle (og_multi_*) has no form of this call and does not split it: the handle of the first device
 * serves it.
 * No reference counterpart: the reference has no derivative at all. */
int og_directional_load(og_handle h, const char* dir_part_path);
int og_directional_dev(og_handle h, const double* d_x, int32_t k, const double* d_V, double* d_dF, double* d_F0,
                       void* hip_stream);
int og_directional(og_handle h, const double* x, int32_t k, const double* V, double* dF, double* F0);
int og_directional_batch_dev(og_batch b, int32_t count, const double* d_X, const double* d_V, double* d_F0, double* d_dF,
                             void* hip_stream);
int og_directional_batch(og_batch b, int32_t count, const double* X, const double* V, double* F0, double* dF);

/* ---- exact adjoint products F'(x)^T w --------------------------------------------------------------
 * G[d][j] = sum_r W[d][r] dF_r/dx_j of F = [cost | c_eq | c_ineq], [k][n] row-major and dense, for k weight vectors
 * W[k][m] over the rows of F, WITHOUT forming the Jacobian: the transposed half of the matrix-free pair whose other half
 * is og_directional.  W = e_0 gives the gradient of the cost, W = [1, lambda] the gradient of the Lagrangian, W = [0, W c]
 * that of a merit 1/2 c' W c.  One workgroup per variable computes the entries of that variable's column of the exact
 * Jacobian (what og_jacobian_exact writes) once, multiplies each by the weight of its row for every vector and sums them
 * where they are: no pattern, no J_T, no n x m memory, no step.  The ORDER of a sum is fixed (csrc/og_adj.h: 256 strided
 * fma chains in ascending term order, then a fixed pairwise tree - no atomics, nothing that depends on scheduling), so
 * the result is reproducible to the bit and vector d of a call with k vectors is bit for bit the call with that vector
 * alone.  A row whose weight is zero is not skipped (0 * inf is NaN, as the product would give); a variable that no row
 * reads gets +0.0; every call writes all k * n doubles.  A run-time parameter is a constant.  At a switch of the
 * callbacks the derivative is that of the branch F(x) takes, as everywhere in the exact mode.
 * Load rule: the kernels live in a part of the callback module of its own (adj_part_path:
 * opengoddard_amd.build.build_adjoint_part), for a module with or without parameters.  og_adjoint_load loads it once per
 * handle - a later call is a no-op and may pass NULL - and og_problem_destroy closes it; error 4: the part is missing or
 * cannot be loaded, 5: it belongs to another module.  The other four fail with error 4 while it is not loaded, and with
 * error 1 (and a message in og_last_error) for null pointers, k < 1 or k > 65535, or a count outside 1 .. capacity.
 * og_adjoint_dev: two launches on hip_stream - the evaluation at d_x (F into d_F0, or into the handle's own array when
 * d_F0 is NULL; og_nonfinite_rows counts its non-finite rows) and the adjoint kernel.  Asynchronous and capturable: a
 * captured graph replays on new contents of d_x and d_W.  No J_T is written and no registered buffer's bookkeeping
 * moves.
 * og_adjoint: host pointers, blocking; F0 may be NULL.
 * The batched forms: lane c works at X[c], with W[c] - ONE weight vector per lane; repeat a point for more - and at the
 * lane's own parameters (og_parameters_batch*), and writes G[c][n] and F0[c][m] (d_F0 / F0 may be NULL); bit for bit the
 * single-point call at that point, vector and those values.  Three launches whatever count is: bind, the batched
 * evaluation, the adjoint kernel.  Lanes count .. capacity-1, their slices of the output and every lane's J_T with its
 * state words are not touched.
 * A multi-device handle (og_multi_*) has no form of this call and does not split it: the handle of the first device
 * serves it.
 * No reference counterpart: the reference has no derivative at all. */
int og_adjoint_load(og_handle h, const char* adj_part_path);
int og_adjoint_dev(og_handle h, const double* d_x, int32_t k, const double* d_W, double* d_G, double* d_F0,
                   void* hip_stream);
int og_adjoint(og_handle h, const double* x, int32_t k, const double* W, double* G, double* F0);
int og_adjoint_batch_dev(og_batch b, int32_t count, const double* d_X, const double* d_W, double* d_F0, double* d_G,
                         void* hip_stream);
int og_adjoint_batch(og_batch b, int32_t count, const double* X, const double* W, double* F0, double* G);

/* ---- exact Hessian-vector products of w . F ---------------------------------------------------------
 * Q[d][j] = sum_r W[d][r] d2F_r/dx_j dV[d] of F = [cost | c_eq | c_ineq], that is Q[d] = grad^2 (W[d] . F)(x) V[d],
 * [k][n] row-major and dense, for k pairs of a weight vector W[d][m] over the rows of F and a direction V[d][n] in the
 * decision vector, WITHOUT forming a Hessian: with W = [1, lambda] the Hessian of the Lagrangian times a vector - the
 * curvature v' H v along a step, the product a Newton-CG or Lanczos iteration asks for.  The terms of an entry are the
 * terms og_adjoint sums for that variable, each evaluated on second-order dual numbers (csrc/og_dual2.h) with the unit
 * seed on x_j and V[d] as the second seed (csrc/og_hvp.h); the ORDER of the sum is og_adjoint's (csrc/og_adj.h), so the
 * result is reproducible to the bit and pair d of a call with k pairs is bit for bit the call with that pair alone.  A row
 * whose weight is zero is not skipped; a variable that no row reads gets +0.0; every call writes all k * n doubles.  A
 * run-time parameter is a constant (the mixed d2/dx dtheta: og_adjoint_parameter).  At a switch of the callbacks the derivative is that of the
 * branch F(x) takes; fabs, max / min, the remainders and the linear interpolation have no curvature of their own.
 * Load rule: the kernels live in a part of the callback module of its own (hvp_part_path:
 * opengoddard_amd.build.build_hessian_part).  og_hessian_vector_load loads it once per handle - a later call is a no-op
 * and may pass NULL - and og_problem_destroy closes it; error 4: the part is missing or cannot be loaded, 5: it belongs
 * to another module.  The other four fail with error 4 while it is not loaded, and with error 1 (and a message in
 * og_last_error) for null pointers, k < 1 or k > 65535, or a count outside 1 .. capacity.
 * og_hessian_vector_dev: two launches on hip_stream - the evaluation at d_x (F into d_F0, or into the handle's own array
 * when d_F0 is NULL) and the Hessian kernel, one grid slice per pair.  Asynchronous and capturable: a captured graph
 * replays on new contents of d_x, d_W and d_V.  No J_T is written and no registered buffer's bookkeeping moves.
 * og_hessian_vector: host pointers, blocking; F0 may be NULL.
 * The batched forms: lane c works at X[c], with the ONE pair W[c], V[c] and at the lane's own parameters
 * (og_parameters_batch*), and writes Q[c][n] and F0[c][m] (d_F0 / F0 may be NULL); bit for bit the single-point call at
 * that point, pair and those values.  Three launches whatever count is: bind, the batched evaluation, the Hessian kernel.
 * A multi-device handle (og_multi_*) has no form of this call and does not split it.
 * No reference counterpart: the reference has no derivative at all. */
int og_hessian_vector_load(og_handle h, const char* hvp_part_path);
int og_hessian_vector_dev(og_handle h, const double* d_x, int32_t k, const double* d_W, const double* d_V, double* d_Q,
                          double* d_F0, void* hip_stream);
int og_hessian_vector(og_handle h, const double* x, int32_t k, const double* W, const double* V, double* Q, double* F0);
int og_hessian_vector_batch_dev(og_batch b, int32_t count, const double* d_X, const double* d_W, const double* d_V,
                                double* d_F0, double* d_Q, void* hip_stream);
int og_hessian_vector_batch(og_batch b, int32_t count, const double* X, const double* W, const double* V, double* F0,
                            double* Q);

/* ---- exact mixed derivatives d(F'(x)^T w)/dtheta for the run-time parameters ---------------------------
 * S[d][k][j] = sum_r W[d][r] d2F_r/dx_j dtheta_k of F = [cost | c_eq | c_ineq], that is S[d][k] = d(F'(x)^T W[d])/dtheta_k,
 * [kw][n_par][n] row-major and dense, for kw weight vectors W[d][m] over the rows of F and EVERY declared run-time
 * parameter, at the handle's current parameter values: with W = [1, lambda] the block d(grad_x L)/dtheta of the
 * linearised KKT system, the right-hand side of a continuation tangent.  The terms of an entry are the terms og_adjoint
 * sums for that variable, each evaluated on second-order dual numbers (csrc/og_dual2.h) with the unit seed on x_j and the
 * unit seed on the parameter's table entry (csrc/og_mix.h); the ORDER of the sum is og_adjoint's (csrc/og_adj.h), so the
 * result is reproducible to the bit and vector d of a call with kw vectors is bit for bit the call with that vector
 * alone.  A row whose weight is zero is not skipped; a variable that no row reads gets +0.0, and so does the whole row
 * of a parameter that nothing reads; every call writes all kw * n_par * n doubles.  No step in theta, no
 * og_set_parameters launch.  At a switch of the callbacks the derivative is that of the branch F(x) takes.
 * Load rule: the kernels live in a part of the callback module of its own (mix_part_path:
 * opengoddard_amd.build.build_mix_part).  og_adjoint_parameter_load loads it once per handle - a later call is a no-op
 * and may pass NULL - and og_problem_destroy closes it; error 4: the part is missing or cannot be loaded, 5: it belongs
 * to another module.  The other four fail with error 4 while it is not loaded.  All five fail with error 1 (and a
 * message in og_last_error) for a module that declares no run-time parameter, for null pointers, kw < 1 or
 * kw * n_par > 65535, or a count outside 1 .. capacity.
 * og_adjoint_parameter_dev: two launches on hip_stream - the evaluation at d_x (F into d_F0, or into the handle's own
 * array when d_F0 is NULL) and the mixed kernel, one grid slice per pair (weight vector, parameter).  Asynchronous and
 * capturable: a captured graph replays on new contents of d_x and d_W and on new parameter values.  No J_T is written
 * and no registered buffer's bookkeeping moves.  og_adjoint_parameter: host pointers, blocking; F0 may be NULL.
 * The batched forms: lane c works at X[c], with the ONE weight vector W[c] and at the lane's own parameters
 * (og_parameters_batch*), and writes S[c][n_par][n] and F0[c][m] (d_F0 / F0 may be NULL); bit for bit the single-point
 * call at that point, vector and those values.  Three launches whatever count is: bind, the batched evaluation, the
 * mixed kernel.  A multi-device handle (og_multi_*) has no form of this call and does not split it.
 * No reference counterpart: the reference has no derivative at all. */
int og_adjoint_parameter_load(og_handle h, const char* mix_part_path);
int og_adjoint_parameter_dev(og_handle h, const double* d_x, int32_t kw, const double* d_W, double* d_S, double* d_F0,
                             void* hip_stream);
int og_adjoint_parameter(og_handle h, const double* x, int32_t kw, const double* W, double* S, double* F0);
int og_adjoint_parameter_batch_dev(og_batch b, int32_t count, const double* d_X, const double* d_W, double* d_F0,
                                   double* d_S, void* hip_stream);
int og_adjoint_parameter_batch(og_batch b, int32_t count, const double* X, const double* W, double* F0, double* S);

/* ---- the exact sparse Hessian of w . F, assembled -----------------------------------------------------
 * H[d][p] = sum_r W[d][r] d2F_r/dx_j dx_l for every stored pair p = (j, l), l <= j, of a static lower-triangle pattern
 * in CSR form (indptr[n + 1], cols[nnz]: the partners l of variable j at row j), [k][nnz] row-major, for k weight vectors
 * W[d][m] over the rows of F = [cost | c_eq | c_ineq]: with W = [1, lambda] the Hessian of the Lagrangian as a sparse
 * matrix - a sparse-direct Newton or interior-point step, the (1, 1) block of the KKT matrix, a reduced-Hessian check.
 * The pattern and, per stored entry, its owner (the variable of the pair whose column of the exact Jacobian the terms are
 * taken from) and the list of the owner's term numbers that read the other variable are DATA the caller passes once
 * (opengoddard_amd.codegen.HessianPlan: indptr, cols, owner[nnz], tptr[nnz + 1], tlist); every pair outside the pattern is
 * an exact zero of the Hessian.  A stored entry is og_hessian_vector's Q[owner] for the unit direction on the other
 * variable restricted to the listed terms (csrc/og_hess.h): for finite weights and a finite point bit for bit that
 * product (but for a lone product that underflows to -0.0, see the header), reproducible to the bit, vector d of a call
 * with k vectors bit for bit the call with that vector alone.  A row whose weight is zero is not skipped; every call
 * writes all k * nnz doubles, no more; a run-time parameter is a constant.
 * Load rule: the kernels live in a part of the callback module of its own (part_path:
 * opengoddard_amd.build.build_hessian_matrix_part).  og_hessian_matrix_load loads it and uploads the plan once per
 * handle - a later call is a no-op and may pass NULLs - and og_problem_destroy closes and frees both; error 4: the part
 * is missing or cannot be loaded, 5: it belongs to another module, 1 (no kernel ever sees the plan, nothing stays loaded): a null
 * array, nnz < 0, pointers that are not monotone or do not end at nnz / the length of tlist, a partner above its row or
 * not ascending within it, an owner that is neither variable of its pair, a term list that does not ascend or names a
 * term the owner's column does not have.  og_hessian_matrix_nnz: the loaded plan's nnz, -1 while none is loaded.  The
 * other four fail with error 4 while nothing is loaded, and with error 1 (and a message in og_last_error) for null
 * pointers, k < 1 or k > 65535, or a count outside 1 .. capacity.
 * og_hessian_matrix_dev: two launches on hip_stream - the evaluation at d_x (F into d_F0, or into the handle's own array
 * when d_F0 is NULL) and the Hessian-matrix kernel, which evaluates an entry's terms once per chunk of 8 weight vectors.
 * Asynchronous and capturable: a captured graph replays on new contents of d_x and d_W.  No J_T is written and no
 * registered buffer's bookkeeping moves.  og_hessian_matrix: host pointers, blocking; F0 may be NULL.
 * The batched forms: lane c works at X[c], with the ONE weight vector W[c] and at the lane's own parameters
 * (og_parameters_batch*), and writes H[c][nnz] and F0[c][m] (d_F0 / F0 may be NULL); bit for bit the single-point call at
 * that point, vector and those values.  Three launches whatever count is: bind, the batched evaluation, the kernel.
 * A multi-device handle (og_multi_*) has no form of this call and does not split it.
 * No reference counterpart: the reference has no derivative at all. */
int og_hessian_matrix_load(og_handle h, const char* part_path, int32_t nnz, const int32_t* indptr, const int32_t* cols,
                           const int32_t* owner, const int32_t* tptr, const int32_t* tlist);
int32_t og_hessian_matrix_nnz(og_handle h);
int og_hessian_matrix_dev(og_handle h, const double* d_x, int32_t k, const double* d_W, double* d_H, double* d_F0,
                          void* hip_stream);
int og_hessian_matrix(og_handle h, const double* x, int32_t k, const double* W, double* H, double* F0);
int og_hessian_matrix_batch_dev(og_batch b, int32_t count, const double* d_X, const double* d_W, double* d_F0,
                                double* d_H, void* hip_stream);
int og_hessian_matrix_batch(og_batch b, int32_t count, const double* X, const double* W, double* F0, double* H);

/* ---- exact second derivatives of w . F in the run-time parameters: the theta-theta block ---------------
 * S[d][k][l] = sum_r W[d][r] d2F_r/dtheta_k dtheta_l of F = [cost | c_eq | c_ineq], [kw][n_par][n_par] row-major and
 * dense, for kw weight vectors W[d][m] over the rows of F, at the handle's current parameter values: with W = [1, lambda]
 * it is d2L/dtheta2, the third block of the Hessian of the Lagrangian in (x, theta) next to og_hessian_vector /
 * og_hessian_matrix (xx) and og_adjoint_parameter (x theta); with x held fixed the exact Hessian in theta.  For a pair
 * (k, l) the entries summed are those of the work lists of its OWNER - the parameter with fewer entries, a tie to the
 * lower index - each evaluated on second-order dual numbers (csrc/og_dual2.h) with the unit seed of slot 1 on the
 * owner's table entry and the unit seed of slot 2 on the partner's (csrc/og_pp.h); the ORDER of the sum is og_adjoint's
 * (csrc/og_adj.h), so the result is reproducible to the bit and vector d of a call with kw vectors is bit for bit the
 * call with that vector alone.  A row whose weight is zero is not skipped; an entry that does not read the partner
 * contributes an exact +0.0; a parameter that nothing reads gets a row and a column of +0.0; S[d][l][k] is a copy of
 * S[d][k][l]; every call writes all kw * n_par * n_par doubles.  No step in theta, no og_set_parameters launch.  At a
 * switch of the callbacks the derivative is that of the branch F(x) takes.
 * Load rule: the kernels live in a part of the callback module of its own (pp_part_path:
 * opengoddard_amd.build.build_pp_part).  og_parameter_hessian_load loads it once per handle - a later call is a no-op
 * and may pass NULL - and og_problem_destroy closes it; error 4: the part is missing or cannot be loaded, 5: it belongs
 * to another module.  The other four fail with error 4 while it is not loaded.  All five fail with error 1 (and a
 * message in og_last_error) for a module that declares no run-time parameter, for null pointers, kw < 1 or kw > 65535,
 * or a count outside 1 .. capacity.
 * og_parameter_hessian_dev: two launches on hip_stream - the evaluation at d_x (F into d_F0, or into the handle's own
 * array when d_F0 is NULL) and the kernel, one workgroup per pair k <= l and chunk of 8 weight vectors, which evaluates
 * an entry once for all vectors of its chunk.  Asynchronous and capturable: a captured graph replays on new contents of
 * d_x and d_W and on new parameter values.  No J_T is written and no registered buffer's bookkeeping moves.
 * og_parameter_hessian: host pointers, blocking; F0 may be NULL.
 * The batched forms: lane c works at X[c], with the ONE weight vector W[c] and at the lane's own parameters
 * (og_parameters_batch*), and writes S[c][n_par][n_par] and F0[c][m] (d_F0 / F0 may be NULL); bit for bit the
 * single-point call at that point, vector and those values.  Three launches whatever count is: bind, the batched
 * evaluation, the kernel.  A multi-device handle (og_multi_*) has no form of this call and does not split it.
 * No reference counterpart: the reference has no derivative at all. */
int og_parameter_hessian_load(og_handle h, const char* pp_part_path);
int og_parameter_hessian_dev(og_handle h, const double* d_x, int32_t kw, const double* d_W, double* d_S, double* d_F0,
                             void* hip_stream);
int og_parameter_hessian(og_handle h, const double* x, int32_t kw, const double* W, double* S, double* F0);
int og_parameter_hessian_batch_dev(og_batch b, int32_t count, const double* d_X, const double* d_W, double* d_F0,
                                   double* d_S, void* hip_stream);
int og_parameter_hessian_batch(og_batch b, int32_t count, const double* X, const double* W, double* F0, double* S);

/* ---- diagnostics ---------------------------------------------------------------------------*/
const char* og_last_error(void);
/* Diagnostics: synchronise `device` and copy `bytes` bytes of its memory to the host (tests read the replicas of
 * a multi-device handle with it). */
int og_device_read(int32_t device, const void* d_src, void* dst, int64_t bytes);
/* Developer diagnostics: phase stamps (s_memrealtime ticks) written by kernel modules compiled with
 * -DOGK_TRACE=1 on a handle created with OGPSX_TRACE=1 in the environment; 8 doubles per wavefront,
 * 8 wavefronts per workgroup, in grid order (tools/trace_fused.py).  Reads `count` doubles and clears
 * the buffer.  Fails on an ordinary handle. */
int og_trace_read(og_handle h, double* out, int64_t count);
int og_device_count(void);     /* HIP devices visible to the library (0 without a GPU) */
/* Measurement aid: enqueue `count` launches of a kernel that does nothing, `blocks` x `threads`, on `hip_stream`.
 * Timed between two events it gives the launch floor of this box for a grid of the sweep's geometry - what any
 * one-launch step costs before it computes anything (bench.py: roofline.latency_floor_us). */
int og_probe_launch(int32_t blocks, int32_t threads, int32_t count, void* hip_stream);

#ifdef __cplusplus
}
#endif
#endif /* OGPSX_H */
