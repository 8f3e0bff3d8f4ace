// ogpsx_core.hip -- libogpsx.so: the generic runtime behind include/ogpsx.h.
//
// LGL construction (host function + HIP kernel from one shared source, og_lgl.h), SciPy's
// forward-difference step rule, and problem handles that bind a compiled callback module
// (libogk_<hash>.so, built from ogk_kernels.hip + a generated header) to a device.
// Reference lines replaced by each entry point are listed in include/ogpsx.h.
#include <hip/hip_runtime.h>
#include <dlfcn.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/ogpsx.h"
#include "og_lgl.h"
#include "ogk.h"

namespace {

thread_local std::string g_error;

int fail(int code, const std::string& msg) {
    g_error = msg;
    return code;
}

#define OG_HIP(expr)                                                                       \
    do {                                                                                   \
        hipError_t e_ = (expr);                                                            \
        if (e_ != hipSuccess)                                                              \
            return fail(100 + (int)e_, std::string(#expr) + ": " + hipGetErrorString(e_)); \
    } while (0)

// ------------------------------------------------------------------------------ LGL kernels
// One thread per node: Newton iteration for tau_k, then P_{N-1}(tau_k) and the weight.
__global__ void lgl_nodes_kernel(int N, double* tau, double* w, double* pval) {
    const int k = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (k >= N) return;
    const double t = oglgl::node(N, k);
    const double p = oglgl::legendre_at_node(N, t);
    tau[k] = t;
    pval[k] = p;
    w[k] = oglgl::weight(N, p);
}

// One thread per matrix entry, consecutive lanes along a row => coalesced stores.
__global__ void lgl_dmat_kernel(int N, const double* tau, const double* pval, double* D) {
    const int l = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    const int k = (int)blockIdx.y;
    if (l >= N) return;
    D[(long)k * N + l] = oglgl::dmat(N, k, l, tau[k], tau[l], pval[k], pval[l]);
}

typedef int (*ogk_get_info_fn)(ogk_info*);
typedef int (*ogk_launch_fn)(const ogk_args*, int, void*);
typedef int (*ogk_launch_batch_fn)(const ogk_batch_args*, int, void*);

// A callback module is one shared object, or several PARTS of it that were compiled side by side (build.py:
// <module>.so, <module>.p1.so, ...; each holds some of the kernels and answers OGK_OTHER_PART for the modes of the
// others).  Calls go to the part that holds the mode; which one that is is remembered per mode.
struct ogk_module {
    static constexpr int MAX_PARTS = 4, MAX_MODES = 16;
    ogk_launch_fn part[MAX_PARTS] = {nullptr, nullptr, nullptr, nullptr};
    void* handle[MAX_PARTS] = {nullptr, nullptr, nullptr, nullptr};
    int n_parts = 0;
    signed char home[MAX_MODES];
    ogk_module() {
        for (int i = 0; i < MAX_MODES; ++i) home[i] = -1;
    }
    explicit operator bool() const { return n_parts > 0; }
    int operator()(const ogk_args* a, int mode, void* stream) {
        if (mode >= 0 && mode < MAX_MODES && home[mode] >= 0) return part[(int)home[mode]](a, mode, stream);
        for (int i = 0; i < n_parts; ++i) {
            const int rc = part[i](a, mode, stream);
            if (rc != OGK_OTHER_PART) {
                if (mode >= 0 && mode < MAX_MODES) home[mode] = (signed char)i;
                return rc;
            }
        }
        return (int)hipErrorInvalidDeviceFunction;         // no part of the module holds this mode
    }
};

}  // namespace

struct og_batch_s;

struct og_problem_s {
    int device = 0;
    int n = 0, m = 0, m_eq = 0, m_ineq = 0;
    void* module = nullptr;
    ogk_module launch;
    double* d_dfrag = nullptr;
    double* d_cvec = nullptr;
    // run-time parameters: d_cvec[par_off + i], i in [0, n_par): the tail of the constant table (og_set_parameters)
    int n_cvec = 0, n_par = 0, par_off = 0;
    double* d_theta = nullptr;          // [n_par] staging of the host-pointer setter
    int64_t dfrag_off[OGK_MAX_PHASE] = {0};
    // staging buffers for the host-pointer entry points
    double* d_x = nullptr;
    double* d_h = nullptr;
    double* d_f0 = nullptr;
    double* d_jt = nullptr;
    size_t jt_capacity = 0;
    // sweep scratch written by every evaluation (ogk.h): base products / dynamics terms / F0-F0
    double* d_y0 = nullptr;
    double* d_xop = nullptr;
    double* d_t0 = nullptr;
    double* d_z = nullptr;
    int* d_flags = nullptr;             // OGK_FLAG_WORDS ints (ogk.h: enum ogk_flag)
    int flag_slot = 0;                  // which of OGK_FLAG_COUNT_A / _B the latest two-launch evaluation counted into
    int n_eval_blocks = 0;
    double* d_trace = nullptr;          // phase stamps of -DOGK_TRACE kernel builds (tools/trace_fused.py)
    // how og_fd_sweep_dev runs: OGK_FUSED evaluation + structured sweep in one launch (default), OGK_SWEEP the same
    // as two launches (OGPSX_SWEEP=split), OGK_DENSE evaluation + dense sweep (OGPSX_SWEEP=dense).  og_fd_columns_dev
    // (the sweep alone, F(x0) supplied) uses OGK_SWEEP or OGK_DENSE: columns_mode().
    int sweep_mode = OGK_FUSED;
    int exact_mode = OGK_EXACT;         // structured (default), OGK_EXACT_DENSE (OGPSX_SWEEP=dense)
    hipStream_t stream = nullptr;
    // persistent-zero output buffers (og_jt_register_dev): the sweep writes only what can be non-zero.  Each
    // registration owns one word of d_state (ogk.h: jt_state); word 0 is the stand-in for unregistered buffers.
    struct jt_reg {
        double* ptr;
        int lo, hi;
        int slot;                       // d_state[2*slot] = state word, d_state[2*slot + 1] = launch counter
    };
    std::vector<jt_reg> regs;
    uint32_t* d_state = nullptr;
    bool fused_ok = false;              // the module can run evaluation + sweep as one launch
    int* nf_read = nullptr;             // where the most recent evaluation left its count of non-finite rows
    // static pattern of J_T (og_pattern): entries of column j are indptr[j]..indptr[j+1] of the packed order
    bool have_pattern = false;
    std::vector<int64_t> indptr;
    std::vector<int32_t> rows;
    // the same pattern as runs of consecutive rows per column (the defect rows of a variable's own state are one run of
    // N): the host's scatter of a downloaded block is one memcpy per run instead of one store per entry
    std::vector<int64_t> run_ptr;       // n + 1: runs of column j = [run_ptr[j], run_ptr[j + 1])
    std::vector<int32_t> run_row, run_len;
    std::vector<int64_t> run_off;       // per run: where it goes in a full n x m matrix (j * m + row): the scatter is one
                                        // flat loop over runs that asks for the destination lines a few runs ahead
    hipEvent_t down_ev[4] = {nullptr, nullptr, nullptr, nullptr};    // the packed block comes down in up to four pieces
    int64_t* d_indptr = nullptr;
    int32_t* d_rows = nullptr;          // the pattern's row indices, flat (pack / unpack read them coalesced)
    // host-pointer entry points: pinned staging ([x | h] up, [packed non-zeros | F | non-finite count] down)
    double* h_up = nullptr;
    double* h_xh = nullptr;             // mapped host matrix: [x | h] the launch reads in place
    double* h_down = nullptr;
    double* d_down = nullptr;
    size_t down_capacity = 0;
    // host matrices registered as persistent-zero (og_jt_register_host)
    struct host_reg {
        double* ptr;
        int lo, hi;
        bool dirty;                     // holds a NaN fill: zero it before the next scatter
        double* mapped;                 // round 6: the matrix is page-locked and mapped into the device's address space
                                        // (hipHostRegister): the one-launch sweep writes its non-zeros - and F(x0) into
                                        // the pinned staging buffer - straight over PCIe: no packed copy, no host scatter;
                                        // nullptr: the packed download + scatter (registration refused, OGPSX_HOST=staged)
        // Which of the two is faster is the HOST's doing (page size and IOMMU decide what 83 541 scattered 8-byte writes into
        // host pages cost; on every box of round 6 the mapped form won, 0.043-0.052 against 0.10-0.12 ms at C3), so it is
        // measured, not assumed: the first ten sweeps into a mapped matrix time both - two warm-ups and three timed calls
        // each, the fastest call of each counts - and the faster form serves from then on (OGPSX_HOST=mapped / staged decide
        // without the trial).
        int choice = 0;                 // 0 undecided, 1 mapped, 2 staged
        int calls = 0;
        bool last_staged = false;       // the last call scattered on the host (a NaN fill of its is the host's to clean)
        bool registered_here = false;   // hipHostRegister was this library's doing (memory from og_pinned_alloc needs none)
        double best_mapped = 1e30, best_staged = 1e30;
        // does this call of og_fd_sweep take the mapped launch?  (forced: OGPSX_HOST decides without the trial)
        bool take_mapped(bool forced) {
            if (forced) choice = 1;
            return choice == 1 || (choice == 0 && calls < 5);
        }
        // a call of the trial took dt seconds: calls 0-1 mapped (warm-up), 2-4 mapped timed, 5-6 packed (warm-up: pattern,
        // staging, its device buffer), 7-9 packed timed; the FASTEST call of each decides (a mean would carry one-time
        // costs of the first calls)
        void trial_call(double dt) {
            const int c = calls++;
            if (c >= 2 && c <= 4) best_mapped = std::min(best_mapped, dt);
            if (c >= 7 && c <= 9) best_staged = std::min(best_staged, dt);
            if (calls >= 10) choice = best_mapped <= best_staged ? 1 : 2;
        }
    };
    std::vector<host_reg> host_regs;
    // column sharding (og_shard_plan)
    int shard_world = 0;
    int64_t shard_block_vals = 0;
    int64_t* d_shard_off = nullptr;
    void* shard_comm = nullptr;         // ncclComm_t of this rank (og_shard_comm_init), one process per GPU
    int shard_rank = -1;
    // batches of points (og_batch_create): the batch part of the module is loaded by the first of them
    void* batch_module = nullptr;
    ogk_launch_batch_fn batch_launch = nullptr;
    std::vector<og_batch_s*> batches;
    // the exact Jacobian of a batch (og_jacobian_exact_batch_load): a part of its own, loaded when first asked for
    void* batch_exact_module = nullptr;
    ogk_launch_batch_fn batch_exact_launch = nullptr;
    // exact dF/dtheta for the run-time parameters (og_parameter_jacobian_load): a part of its own with a single-point and
    // a batched launcher, loaded when first asked for; d_pj: [n_par][m] staging of the host-pointer call
    void* par_module = nullptr;
    ogk_launch_fn par_launch = nullptr;
    ogk_launch_batch_fn par_launch_batch = nullptr;
    double* d_pj = nullptr;
    // exact directional derivatives (og_directional_load): a part of its own with a single-point and a batched
    // launcher, loaded when first asked for; d_dir: [V[k][n] | dF[k][m]] staging of the host-pointer call, dir_capacity
    // directions large
    void* dir_module = nullptr;
    ogk_launch_fn dir_launch = nullptr;
    ogk_launch_batch_fn dir_launch_batch = nullptr;
    double* d_dir = nullptr;
    size_t dir_capacity = 0;
    // exact adjoint products (og_adjoint_load): the same arrangement; d_adj: [W[k][m] | G[k][n]] staging of the
    // host-pointer call, adj_capacity weight vectors large
    void* adj_module = nullptr;
    ogk_launch_fn adj_launch = nullptr;
    ogk_launch_batch_fn adj_launch_batch = nullptr;
    double* d_adj = nullptr;
    size_t adj_capacity = 0;
    // exact Hessian-vector products (og_hessian_vector_load): the same arrangement; d_hvp: [W[k][m] | V[k][n] | Q[k][n]]
    // staging of the host-pointer call, hvp_capacity pairs large
    void* hvp_module = nullptr;
    ogk_launch_fn hvp_launch = nullptr;
    ogk_launch_batch_fn hvp_launch_batch = nullptr;
    double* d_hvp = nullptr;
    size_t hvp_capacity = 0;
    // exact mixed derivatives d(F'(x)^T w)/dtheta (og_adjoint_parameter_load): the same arrangement;
    // d_mix: [W[k][m] | S[k][n_par][n]] staging of the host-pointer call, mix_capacity weight vectors large
    void* mix_module = nullptr;
    ogk_launch_fn mix_launch = nullptr;
    ogk_launch_batch_fn mix_launch_batch = nullptr;
    double* d_mix = nullptr;
    size_t mix_capacity = 0;
    // the exact sparse Hessian (og_hessian_matrix_load): the same arrangement, and the device plan (csrc/ogk.h) built
    // from the caller's pattern and term lists; hess_nnz < 0: nothing loaded; hess_grid: workgroups of one chunk of
    // weight vectors; d_hess: [W[k][m] | H[k][nnz]] staging of the host-pointer call, hess_capacity vectors large
    void* hess_module = nullptr;
    ogk_launch_fn hess_launch = nullptr;
    ogk_launch_batch_fn hess_launch_batch = nullptr;
    int32_t* d_hess_plan = nullptr;
    int32_t hess_nnz = -1;
    int32_t hess_grid = 0;
    double* d_hess = nullptr;
    size_t hess_capacity = 0;
    // exact second derivatives of w . F in the parameters (og_parameter_hessian_load): the arrangement of the mixed part;
    // d_pp: [W[k][m] | S[k][n_par][n_par]] staging of the host-pointer call, pp_capacity weight vectors large
    void* pp_module = nullptr;
    ogk_launch_fn pp_launch = nullptr;
    ogk_launch_batch_fn pp_launch_batch = nullptr;
    double* d_pp = nullptr;
    size_t pp_capacity = 0;
};
static const int OG_MAX_JT_REGS = 63;
static const size_t OG_TRACE_DOUBLES = (size_t)1 << 20;     // 16384 workgroups x 8 wavefronts x 8 stamps

namespace {

// evaluation + sweep really are ONE launch on this handle (asked for, and the module's LDS window allows it)
bool one_launch(const og_problem_s* p) { return p->sweep_mode == OGK_FUSED && p->fused_ok; }

// the sweep as a launch of its own (F(x0) is there already): the structured kernel unless the dense one is asked for
int columns_mode(const og_problem_s* p) { return p->sweep_mode == OGK_FUSED ? OGK_SWEEP : p->sweep_mode; }

// the registration of exactly this block of columns at this address as a persistent-zero buffer, or nullptr
og_problem_s::jt_reg* find_jt_reg(og_problem_s* p, const double* jt, int lo, int hi) {
    for (auto& r : p->regs)
        if (r.ptr == jt && r.lo == lo && r.hi == hi) return &r;
    return nullptr;
}

void fill_args(og_problem_s* p, ogk_args* a, const double* x, const double* h, double* f0,
               double* jt, int lo, int hi, bool new_launch = true) {
    memset(a, 0, sizeof *a);
    a->x0 = x;
    a->h = h;
    a->dfrag = p->d_dfrag;
    a->cvec = p->d_cvec;
    a->f0 = f0;
    a->y0 = p->d_y0;
    a->xop = p->d_xop;
    a->t0 = p->d_t0;
    a->z = p->d_z;
    a->nonfinite = p->d_flags + p->flag_slot;
    a->nonfinite_next = p->d_flags + (p->flag_slot ^ 1);
    a->ready = reinterpret_cast<unsigned*>(p->d_flags + OGK_FLAG_TICKET);
    a->trace = p->d_trace;
    a->jt = jt;
    a->col_lo = lo;
    a->col_hi = hi;
    // a registered buffer (exactly this block of columns at this address) is written sparsely; its two words
    // (state, launch counter) live on the device - nothing about the history of the buffer is a launch argument
    a->jt_sparse = 0;
    a->jt_bump = 0;
    a->jt_state = p->d_state;
    a->jt_launches = p->d_state + 1;
    a->nonfinite_result = p->d_flags + OGK_FLAG_FUSED_RESULT;
    if (!new_launch && p->nf_read) a->nonfinite = p->nf_read;     // pack / unpack: the count the last evaluation left
    if (const og_problem_s::jt_reg* r = jt ? find_jt_reg(p, jt, lo, hi) : nullptr) {
        a->jt_sparse = 1;
        a->jt_state = p->d_state + 2 * r->slot;
        a->jt_launches = a->jt_state + 1;
    }
    memcpy(a->dfrag_off, p->dfrag_off, sizeof(a->dfrag_off));
}

// The one-launch form (OGK_FUSED) counts non-finite rows in a word of its own, which its last evaluation workgroup
// moves to the result word and clears: the launch arguments depend on nothing but the pointers (a captured graph can
// be replayed).  `a` comes from fill_args.
void one_launch_args(og_problem_s* p, ogk_args* a) {
    a->nonfinite = p->d_flags + OGK_FLAG_FUSED_COUNT;
    p->nf_read = a->nonfinite_result;
}

// the pattern tables of a pack / unpack launch; poff: where column j's entries start in the packed array
void pattern_args(og_problem_s* p, ogk_args* a, const int64_t* poff) {
    a->poff = poff, a->pind = p->d_indptr, a->prow = p->d_rows;
}

// a launcher's code -> 0, or this library's error for it
int launched(int rc, const char* where) {
    return rc ? fail(100 + rc, std::string(where) + ": " + hipGetErrorString((hipError_t)rc)) : 0;
}

// the handle's own Jacobian buffer (host-pointer entry points): sized for this block of columns and
// registered as a persistent-zero buffer, so that every sweep into it writes the non-zeros only
int own_jt(og_problem_s* p, int lo, int hi) {
    const size_t need = (size_t)(hi - lo) * (size_t)p->m;
    if (need > p->jt_capacity) {
        if (p->d_jt) {
            og_jt_unregister_dev(p, p->d_jt);
            OG_HIP(hipFree(p->d_jt));
        }
        p->d_jt = nullptr;
        p->jt_capacity = 0;
        OG_HIP(hipMalloc(&p->d_jt, sizeof(double) * need));
        p->jt_capacity = need;
    }
    if (find_jt_reg(p, p->d_jt, lo, hi)) return 0;
    return og_jt_register_dev(p, p->d_jt, lo, hi, p->stream);
}

// the static pattern, once per handle: entries per column from the module (OGK_PATTERN_COUNT), prefix sums here,
// row indices from the module again (OGK_PATTERN_ROWS)
int ensure_pattern(og_problem_s* p) {
    if (p->have_pattern) return 0;
    OG_HIP(hipSetDevice(p->device));
    const int n = p->n;
    int32_t* d_cnt = nullptr;
    OG_HIP(hipMalloc(&d_cnt, sizeof(int32_t) * (size_t)n));
    ogk_args a;
    fill_args(p, &a, nullptr, nullptr, nullptr, nullptr, 0, 0, false);
    a.pint = d_cnt;
    int rc = p->launch(&a, OGK_PATTERN_COUNT, p->stream);
    std::vector<int32_t> cnt((size_t)n);
    hipError_t e = rc ? (hipError_t)rc : hipMemcpyAsync(cnt.data(), d_cnt, sizeof(int32_t) * (size_t)n,
                                                        hipMemcpyDeviceToHost, p->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(p->stream);
    hipFree(d_cnt);
    if (e != hipSuccess) return fail(100 + (int)e, std::string("og_pattern: ") + hipGetErrorString(e));
    p->indptr.assign((size_t)n + 1, 0);
    for (int j = 0; j < n; ++j) p->indptr[(size_t)j + 1] = p->indptr[(size_t)j] + cnt[(size_t)j];
    const size_t nnz = (size_t)p->indptr[(size_t)n];
    OG_HIP(hipMalloc(&p->d_indptr, sizeof(int64_t) * ((size_t)n + 1)));
    OG_HIP(hipMemcpy(p->d_indptr, p->indptr.data(), sizeof(int64_t) * ((size_t)n + 1), hipMemcpyHostToDevice));
    int32_t* d_rows = nullptr;
    OG_HIP(hipMalloc(&d_rows, sizeof(int32_t) * (nnz ? nnz : 1)));
    a.pint = d_rows;
    a.poff = p->d_indptr;
    rc = p->launch(&a, OGK_PATTERN_ROWS, p->stream);
    p->rows.assign(nnz, 0);
    e = rc ? (hipError_t)rc : hipMemcpyAsync(p->rows.data(), d_rows, sizeof(int32_t) * nnz, hipMemcpyDeviceToHost,
                                             p->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(p->stream);
    if (e != hipSuccess) {
        hipFree(d_rows);
        return fail(100 + (int)e, std::string("og_pattern: ") + hipGetErrorString(e));
    }
    p->d_rows = d_rows;
    p->run_ptr.assign((size_t)n + 1, 0);
    p->run_row.clear();
    p->run_len.clear();
    p->run_off.clear();
    for (int j = 0; j < n; ++j) {
        const int64_t lo = p->indptr[(size_t)j], hi = p->indptr[(size_t)j + 1];
        for (int64_t i = lo; i < hi;) {
            int64_t e = i + 1;
            while (e < hi && p->rows[(size_t)e] == p->rows[(size_t)e - 1] + 1) ++e;
            p->run_row.push_back(p->rows[(size_t)i]);
            p->run_len.push_back((int32_t)(e - i));
            p->run_off.push_back((int64_t)j * (int64_t)p->m + (int64_t)p->rows[(size_t)i]);
            i = e;
        }
        p->run_ptr[(size_t)j + 1] = (int64_t)p->run_row.size();
    }
    p->have_pattern = true;
    return 0;
}

// pinned staging of the host-pointer entry points
int ensure_staging(og_problem_s* p, size_t down_doubles) {
    if (!p->h_up) OG_HIP(hipHostMalloc(&p->h_up, sizeof(double) * 2 * (size_t)p->n, hipHostMallocDefault));
    if (down_doubles > p->down_capacity) {
        if (p->h_down) OG_HIP(hipHostFree(p->h_down));
        if (p->d_down) OG_HIP(hipFree(p->d_down));
        p->h_down = p->d_down = nullptr;
        p->down_capacity = 0;
        OG_HIP(hipHostMalloc(&p->h_down, sizeof(double) * down_doubles, hipHostMallocDefault));
        OG_HIP(hipMalloc(&p->d_down, sizeof(double) * down_doubles));
        p->down_capacity = down_doubles;
    }
    return 0;
}

// x (and h) to the device through the pinned buffer: one copy
int upload_point(og_problem_s* p, const double* x, const double* hstep) {
    int rc = ensure_staging(p, p->down_capacity ? p->down_capacity : (size_t)p->m + 1);
    if (rc) return rc;
    memcpy(p->h_up, x, sizeof(double) * (size_t)p->n);
    if (hstep) memcpy(p->h_up + p->n, hstep, sizeof(double) * (size_t)p->n);
    // d_x and d_h are one allocation: [x | h]
    OG_HIP(hipMemcpyAsync(p->d_x, p->h_up, sizeof(double) * (size_t)p->n * (hstep ? 2 : 1), hipMemcpyHostToDevice,
                          p->stream));
    return 0;
}

og_problem_s::host_reg* find_host_reg(og_problem_s* p, const double* JT, int lo, int hi) {
    for (auto& r : p->host_regs)
        if (r.ptr == JT && r.lo == lo && r.hi == hi) return &r;
    return nullptr;
}

// After a sweep / exact Jacobian into the handle's own registered buffer: bring the result to the host.  A
// registered host matrix receives the packed non-zeros (one pinned copy together with F and the count of
// non-finite rows) and a scatter; anything else, and any sweep with non-finite rows, the dense block.
// OGPSX_TIMING=1: where a host-pointer sweep spends its time (upload enqueue, launch, copy enqueue, wait, scatter),
// averaged over 64 calls, on stderr
struct host_clock {
    bool on = getenv("OGPSX_TIMING") != nullptr;
    double t[6] = {0, 0, 0, 0, 0, 0};
    double last = 0.0;
    int calls = 0;
    static double now() {
        return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count();
    }
    void start() { if (on) last = now(); }
    void mark(int slot) {
        if (!on) return;
        const double n = now();
        t[slot] += n - last;
        last = n;
    }
    void done() {
        if (!on || ++calls < 64) return;
        fprintf(stderr, "[ogpsx timing] host sweep, us per call: upload %.1f, launch %.1f, copy enqueue %.1f, wait %.1f, "
                        "F + flags %.1f, scatter %.1f\n", 1e6 * t[0] / calls, 1e6 * t[1] / calls, 1e6 * t[2] / calls,
                1e6 * t[3] / calls, 1e6 * t[4] / calls, 1e6 * t[5] / calls);
        for (double& v : t) v = 0.0;
        calls = 0;
    }
} g_host_clock;

int download_block(og_problem_s* p, int lo, int hi, double* JT, double* F0, const double* d_src = nullptr,
                   bool already_packed = false) {
    const size_t need = (size_t)(hi - lo) * (size_t)p->m;
    if (!d_src) d_src = p->d_jt;
    og_problem_s::host_reg* reg = find_host_reg(p, JT, lo, hi);
    if (!reg) {
        OG_HIP(hipMemcpyAsync(JT, d_src, sizeof(double) * need, hipMemcpyDeviceToHost, p->stream));
        if (F0) OG_HIP(hipMemcpyAsync(F0, p->d_f0, sizeof(double) * p->m, hipMemcpyDeviceToHost, p->stream));
        OG_HIP(hipStreamSynchronize(p->stream));
        return 0;
    }
    reg->last_staged = true;
    int rc = ensure_pattern(p);
    if (rc) return rc;
    const int64_t first = p->indptr[(size_t)lo], nnz = p->indptr[(size_t)hi] - first;
    const size_t down = (size_t)nnz + (size_t)p->m + 1;
    rc = ensure_staging(p, down);
    if (rc) return rc;
    if (!already_packed) {              // (the one-launch sweep of og_fd_sweep wrote d_down itself)
        ogk_args a;
        fill_args(p, &a, p->d_x, p->d_h, p->d_f0, const_cast<double*>(d_src), lo, hi, false);
        pattern_args(p, &a, p->d_indptr);
        a.pvals = p->d_down - first;
        a.ptail = p->d_down + nnz;
        rc = p->launch(&a, OGK_PACK, p->stream);
        if (rc) return launched(rc, "og_fd_sweep: pack");
    }
    // The packed block comes down in up to four pieces, each with an event behind it, and the host scatters piece c
    // while piece c + 1 crosses PCIe (round 6; measured before, C3: 39 us waiting for upload + launch + ONE copy, then
    // 43 us of scatter - the destination lines of an 18.6 MB matrix are cache misses: the loop asks for them a few runs
    // ahead).  F(x0) and the count of non-finite rows travel behind the last piece.
    static const int pieces_wanted = [] { const char* e = getenv("OGPSX_DOWN_PIECES"); return e ? atoi(e) : 1; }();
    const int64_t run_lo = p->run_ptr[(size_t)lo], run_hi = p->run_ptr[(size_t)hi];
    const int pieces = (int)std::max<int64_t>(1, std::min<int64_t>(std::min(4, pieces_wanted), nnz / 16384));
    int64_t piece_run[5], piece_val[5];
    piece_run[0] = run_lo;
    piece_val[0] = 0;
    {
        // cut at column boundaries nearest to equal shares of the values
        int col = lo;
        for (int c = 1; c < pieces; ++c) {
            const int64_t want = first + nnz * c / pieces;
            col = (int)(std::lower_bound(p->indptr.begin() + col, p->indptr.begin() + hi, want) - p->indptr.begin());
            piece_run[c] = p->run_ptr[(size_t)col];
            piece_val[c] = p->indptr[(size_t)col] - first;
        }
        piece_run[pieces] = run_hi;
        piece_val[pieces] = nnz;
    }
    for (int c = 0; c < pieces; ++c) {
        if (!p->down_ev[c]) OG_HIP(hipEventCreateWithFlags(&p->down_ev[c], hipEventDisableTiming));
        const size_t from = (size_t)piece_val[c], to = c + 1 == pieces ? down : (size_t)piece_val[c + 1];
        if (to > from)
            OG_HIP(hipMemcpyAsync(p->h_down + from, p->d_down + from, sizeof(double) * (to - from), hipMemcpyDeviceToHost,
                                  p->stream));
        OG_HIP(hipEventRecord(p->down_ev[c], p->stream));
    }
    g_host_clock.mark(2);
    if (reg->dirty) {                    // (a NaN fill from the sweep before: the matrix is zeroed while the copies run)
        memset(JT, 0, sizeof(double) * need);
        reg->dirty = false;
    }
    const int64_t base = (int64_t)lo * (int64_t)p->m;
    const int64_t* off = p->run_off.data();
    const int32_t* len = p->run_len.data();
    const double* v = p->h_down;
    static const int AHEAD = [] { const char* e = getenv("OGPSX_AHEAD"); return e ? atoi(e) : 24; }();
    for (int c = 0; c < pieces; ++c) {
        while (true) {                   // (polling: a blocking wait costs a wake-up per piece)
            const hipError_t e = hipEventQuery(p->down_ev[c]);
            if (e == hipSuccess) break;
            if (e != hipErrorNotReady) return fail(100 + (int)e, std::string("og_fd_sweep: download: ") + hipGetErrorString(e));
        }
        if (c == 0) g_host_clock.mark(3);
        const int64_t k1 = piece_run[c + 1];
        for (int64_t k = piece_run[c]; k < k1; ++k) {
            if (k + AHEAD < run_hi) __builtin_prefetch(JT + (off[k + AHEAD] - base), 1, 3);
            const int32_t n_ = len[k];
            double* dst = JT + (off[k] - base);
            if (n_ <= 4) {
                for (int32_t i = 0; i < n_; ++i) dst[i] = v[i];
            } else {
                memcpy(dst, v, sizeof(double) * (size_t)n_);
            }
            v += n_;
        }
    }
    g_host_clock.mark(5);
    const bool bad = p->h_down[(size_t)nnz + (size_t)p->m] != 0.0;
    if (F0) memcpy(F0, p->h_down + nnz, sizeof(double) * (size_t)p->m);
    g_host_clock.mark(4);
    if (bad) {                           // rows of NaN in every column: the dense block (over what was scattered)
        OG_HIP(hipMemcpyAsync(JT, d_src, sizeof(double) * need, hipMemcpyDeviceToHost, p->stream));
        OG_HIP(hipStreamSynchronize(p->stream));
        reg->dirty = true;
    }
    g_host_clock.done();
    return 0;
}

// The three forms of og_fd_sweep (which decides; p->d_jt is registered for [lo, hi) by then).

// Mapped host matrix: ONE launch writes the non-zeros into the caller's matrix and F(x0) + the count of non-finite rows
// into the pinned staging buffer, both over PCIe; the host waits for the launch and is done.  in_place: the launch
// reads x | h out of mapped host memory too and p->d_x | p->d_h are left as they were.
int sweep_mapped(og_problem_s* p, og_problem_s::host_reg* reg, const double* x, const double* hstep, int lo, int hi,
                 double* JT, double* F0, bool in_place) {
    int rc = in_place ? 0 : upload_point(p, x, hstep);
    if (rc) return rc;
    g_host_clock.mark(0);
    rc = ensure_staging(p, (size_t)p->m + 1);
    if (rc) return rc;
    if (reg->dirty && reg->last_staged) {        // (a NaN block the packed path downloaded: not the device's to clean)
        memset(JT, 0, sizeof(double) * (size_t)(hi - lo) * (size_t)p->m);
        reg->dirty = false;
    }
    reg->last_staged = false;
    void* tail = nullptr;
    OG_HIP(hipHostGetDevicePointer(&tail, p->h_down, 0));
    const double *kx = p->d_x, *kh = p->d_h;
    if (in_place) {
        if (!p->h_xh) OG_HIP(hipHostMalloc(&p->h_xh, sizeof(double) * 2 * (size_t)p->n, hipHostMallocNonCoherent | hipHostMallocMapped));
        memcpy(p->h_xh, x, sizeof(double) * (size_t)p->n);
        memcpy(p->h_xh + p->n, hstep, sizeof(double) * (size_t)p->n);
        void* dxh = nullptr;
        OG_HIP(hipHostGetDevicePointer(&dxh, p->h_xh, 0));
        kx = (const double*)dxh;
        kh = kx + p->n;
    }
    ogk_args a;
    fill_args(p, &a, kx, kh, (double*)tail, reg->mapped, lo, hi);
    one_launch_args(p, &a);
    a.ptail = (double*)tail;
    rc = p->launch(&a, OGK_FUSED, p->stream);
    if (rc) return launched(rc, "og_fd_sweep");
    g_host_clock.mark(1);
    OG_HIP(hipStreamSynchronize(p->stream));
    g_host_clock.mark(3);
    if (F0) memcpy(F0, p->h_down, sizeof(double) * (size_t)p->m);
    // (rows of NaN in every column were written by the launch itself and the next sweep cleans them, as in a
    // device buffer; a packed download into this matrix in between - the exact mode - zeroes it first)
    reg->dirty = p->h_down[(size_t)p->m] != 0.0;
    g_host_clock.mark(4);
    g_host_clock.done();
    return 0;
}

// Registered host matrix, packed: ONE launch into the handle's own buffer leaves the packed non-zeros, F(x0) and the
// count of non-finite rows contiguous in the staging buffer, one pinned copy brings them down, the host scatters
int sweep_packed(og_problem_s* p, int lo, int hi, double* JT, double* F0) {
    int rc = ensure_pattern(p);
    if (rc) return rc;
    const int64_t first = p->indptr[(size_t)lo], nnz = p->indptr[(size_t)hi] - first;
    rc = ensure_staging(p, (size_t)nnz + (size_t)p->m + 1);
    if (rc) return rc;
    ogk_args a;
    fill_args(p, &a, p->d_x, p->d_h, p->d_down + nnz, p->d_jt, lo, hi);
    one_launch_args(p, &a);
    a.poff = p->d_indptr;
    a.pvals = p->d_down - first;
    a.ptail = p->d_down + nnz;
    rc = p->launch(&a, OGK_FUSED, p->stream);
    if (rc) return launched(rc, "og_fd_sweep");
    g_host_clock.mark(1);
    return download_block(p, lo, hi, JT, F0, nullptr, true);
}

// Anything else (an unregistered matrix, a handle without the one-launch form): the sweep as og_fd_sweep_dev runs it,
// then the block comes down - packed for a registered matrix, dense otherwise
int sweep_download(og_problem_s* p, int lo, int hi, double* JT, double* F0) {
    const int rc = og_fd_sweep_dev(p, p->d_x, p->d_h, lo, hi, p->d_jt, p->d_f0, p->stream);
    return rc ? rc : download_block(p, lo, hi, JT, F0);
}

}  // namespace

// launch-floor probe (og_probe_launch): a kernel that does nothing, in the geometry asked for
__global__ void og_probe_kernel(int unused) { (void)unused; }

// Run-time parameters (og_set_parameters_dev, og_parameters_batch_dev): the tail of a constant table is rewritten on the
// device, one double per thread.  tail[i] = theta[i], i in [0, n_par).
__global__ void og_par_set_kernel(double* tail, const double* theta, int n_par) {
    const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (i < n_par) tail[i] = theta[i];
}

// The same for `count` lanes of a batch, each with a table of n_cvec doubles of its own whose tail begins at par_off:
// lane k takes TH[k * n_par + i], or - TH == nullptr - shared[i] (the handle's values) like every other lane.
__global__ void og_par_lanes_kernel(double* lane_cvec, long n_cvec, int par_off, int n_par, int count, const double* TH,
                                    const double* shared) {
    const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (long)count * n_par) return;
    const long k = idx / n_par;
    const int i = (int)(idx - k * n_par);
    lane_cvec[k * n_cvec + par_off + i] = TH ? TH[idx] : shared[i];
}

extern "C" {

const char* og_last_error(void) { return g_error.c_str(); }

int og_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

int og_probe_launch(int32_t blocks, int32_t threads, int32_t count, void* hip_stream) {
    if (blocks < 1 || threads < 1 || threads > 1024 || count < 0) return fail(1, "og_probe_launch: bad geometry");
    for (int i = 0; i < count; ++i)
        hipLaunchKernelGGL(og_probe_kernel, dim3((unsigned)blocks), dim3((unsigned)threads), 0, (hipStream_t)hip_stream, 0);
    OG_HIP(hipGetLastError());
    return 0;
}

int og_lgl(int32_t N, double* tau, double* w, double* D) {
    if (N < 3) return fail(1, "og_lgl: N must be >= 3");
    if (!tau || !w || !D) return fail(1, "og_lgl: null output");
    std::vector<double> p(N);
    for (int k = 0; k < N; ++k) tau[k] = oglgl::node(N, k);
    for (int k = 0; k < N; ++k) {
        p[k] = oglgl::legendre_at_node(N, tau[k]);
        w[k] = oglgl::weight(N, p[k]);
    }
    for (int k = 0; k < N; ++k)
        for (int l = 0; l < N; ++l)
            D[(long)k * N + l] = oglgl::dmat(N, k, l, tau[k], tau[l], p[k], p[l]);
    return 0;
}

int og_lgl_dev(int32_t N, double* d_tau, double* d_w, double* d_D, void* hip_stream) {
    if (N < 3) return fail(1, "og_lgl_dev: N must be >= 3");
    hipStream_t s = (hipStream_t)hip_stream;
    double* d_p = nullptr;
    OG_HIP(hipMalloc(&d_p, sizeof(double) * N));
    hipLaunchKernelGGL(lgl_nodes_kernel, dim3((N + 63) / 64), dim3(64), 0, s, N, d_tau, d_w, d_p);
    hipLaunchKernelGGL(lgl_dmat_kernel, dim3((N + 63) / 64, N), dim3(64), 0, s, N, d_tau, d_p, d_D);
    OG_HIP(hipGetLastError());
    OG_HIP(hipStreamSynchronize(s));
    OG_HIP(hipFree(d_p));
    return 0;
}

int og_fd_step(int32_t n, const double* x, const double* lb, const double* ub, double* h) {
    // scipy/optimize/_numdiff.py:500-515 (absolute step with zero-step fallback) followed by
    // _adjust_scheme_to_bounds(x0, h, 1, '1-sided', lb, ub), scipy/optimize/_numdiff.py:44-70.
    const double abs_step = 1.4901161193847656e-08;          // scipy/optimize/_slsqp_py.py:33
    const double root_eps = 1.4901161193847656e-08;          // EPS**0.5 for the 2-point scheme
    const double inf = std::numeric_limits<double>::infinity();
    bool unbounded = true;
    for (int i = 0; i < n; ++i)
        if (!(lb[i] == -inf && ub[i] == inf)) unbounded = false;
    for (int i = 0; i < n; ++i) {
        double hi = abs_step;
        const double dx = (x[i] + hi) - x[i];
        if (dx == 0.0) {
            const double sign = (x[i] >= 0.0) ? 1.0 : -1.0;
            hi = root_eps * sign * std::fmax(1.0, std::fabs(x[i]));
        }
        if (!unbounded) {
            const double lower = x[i] - lb[i], upper = ub[i] - x[i];
            const double xn = x[i] + hi;
            const bool violated = (xn < lb[i]) || (xn > ub[i]);
            const bool fitting = std::fabs(hi) <= std::fmax(lower, upper);
            double adj = hi;
            if (violated && fitting) adj = -adj;
            if (!fitting) adj = (upper >= lower) ? upper : -lower;
            hi = adj;
        }
        h[i] = hi;
    }
    return 0;
}

int og_problem_create(const og_desc* desc, og_handle* out) {
    if (!desc || !out) return fail(1, "og_problem_create: null argument");
    *out = nullptr;
    if (desc->abi_version != OG_ABI_VERSION) return fail(2, "og_problem_create: ABI version mismatch");
    if (desc->n_phase < 1 || desc->n_phase > OGK_MAX_PHASE)
        return fail(2, "og_problem_create: unsupported phase count");
    if (!desc->module_path) return fail(2, "og_problem_create: module_path is null");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1)
        return fail(3, "og_problem_create: no HIP device available");
    if (desc->device < 0 || desc->device >= ndev)
        return fail(3, "og_problem_create: device ordinal out of range");
    OG_HIP(hipSetDevice(desc->device));

    void* mod = dlopen(desc->module_path, RTLD_NOW | RTLD_LOCAL);
    if (!mod) return fail(4, std::string("og_problem_create: dlopen failed: ") + dlerror());
    ogk_get_info_fn get_info = (ogk_get_info_fn)dlsym(mod, "ogk_get_info");
    ogk_launch_fn launch = (ogk_launch_fn)dlsym(mod, "ogk_launch");
    if (!get_info || !launch) {
        dlclose(mod);
        return fail(4, "og_problem_create: module lacks ogk_get_info/ogk_launch");
    }
    ogk_info info;
    memset(&info, 0, sizeof info);
    get_info(&info);
    bool ok = info.abi == OGK_ABI && info.n == desc->n && info.m_eq == desc->m_eq &&
              info.m_ineq == desc->m_ineq && info.n_phase == desc->n_phase &&
              info.n_cvec == desc->n_cvec;
    for (int i = 0; ok && i < desc->n_phase; ++i) ok = info.phase_nodes[i] == desc->nodes[i];
    ogk_par_info par;
    memset(&par, 0, sizeof par);
    typedef int (*ogk_get_par_info_fn)(ogk_par_info*);
    ogk_get_par_info_fn get_par = (ogk_get_par_info_fn)dlsym(mod, "ogk_get_par_info");
    ok = ok && get_par && get_par(&par) == 0;
    ok = ok && par.n_par >= 0 && par.par_off >= 0 && par.par_off + par.n_par == info.n_cvec;       // the table's tail
    if (!ok) {
        dlclose(mod);
        return fail(5, "og_problem_create: descriptor does not match the compiled module");
    }

    og_problem_s* p = new og_problem_s();
    p->device = desc->device;
    p->n = info.n;
    p->m = info.m;
    p->m_eq = info.m_eq;
    p->m_ineq = info.m_ineq;
    p->n_cvec = info.n_cvec;
    p->n_par = par.n_par;
    p->par_off = par.par_off;
    p->module = mod;
    p->launch.part[0] = launch;
    p->launch.handle[0] = mod;
    p->launch.n_parts = 1;
    {
        // further parts of the module, if it was built in parts: <path minus ".so">.p<k>.so
        std::string stem(desc->module_path);
        if (stem.size() > 3 && stem.compare(stem.size() - 3, 3, ".so") == 0) stem.resize(stem.size() - 3);
        for (int k = 1; k < ogk_module::MAX_PARTS; ++k) {
            const std::string path = stem + ".p" + std::to_string(k) + ".so";
            void* more = dlopen(path.c_str(), RTLD_NOW | RTLD_LOCAL);
            if (!more) break;
            ogk_launch_fn fn = (ogk_launch_fn)dlsym(more, "ogk_launch");
            if (!fn) {
                dlclose(more);
                break;
            }
            p->launch.part[p->launch.n_parts] = fn;
            p->launch.handle[p->launch.n_parts] = more;
            ++p->launch.n_parts;
        }
    }

    // pack every phase's D into MFMA operand order and upload
    std::vector<double> frag;
    long total = 0;
    for (int i = 0; i < desc->n_phase; ++i) {
        p->dfrag_off[i] = total;
        total += ogk_frag_size(desc->nodes[i]);
    }
    frag.assign((size_t)total, 0.0);
    for (int i = 0; i < desc->n_phase; ++i) {
        const int N = desc->nodes[i];
        std::vector<double> tmp;
        const double* D = (desc->D && desc->D[i]) ? desc->D[i] : nullptr;
        if (!D) {
            // no matrix supplied: build it on the device with the LGL kernels (bit-identical to
            // og_lgl, tests/test_gpu_parity.py) and bring it back for operand packing
            double *d_tau = nullptr, *d_w = nullptr, *d_D = nullptr;
            tmp.resize((size_t)N * N);
            hipError_t le = hipMalloc(&d_tau, sizeof(double) * N);
            if (le == hipSuccess) le = hipMalloc(&d_w, sizeof(double) * N);
            if (le == hipSuccess) le = hipMalloc(&d_D, sizeof(double) * (size_t)N * N);
            int rc = (le == hipSuccess) ? og_lgl_dev(N, d_tau, d_w, d_D, nullptr) : 100 + (int)le;
            if (!rc && hipMemcpy(tmp.data(), d_D, sizeof(double) * (size_t)N * N,
                                 hipMemcpyDeviceToHost) != hipSuccess)
                rc = 101;
            hipFree(d_tau);
            hipFree(d_w);
            hipFree(d_D);
            if (rc) {
                og_problem_destroy(p);
                return fail(rc, "og_problem_create: device LGL construction failed");
            }
            D = tmp.data();
        }
        ogk_frag_pack(N, D, frag.data() + p->dfrag_off[i]);
    }
    hipError_t e = hipMalloc(&p->d_dfrag, sizeof(double) * (size_t)total);
    if (e == hipSuccess)
        e = hipMemcpy(p->d_dfrag, frag.data(), sizeof(double) * (size_t)total, hipMemcpyHostToDevice);
    if (e == hipSuccess && desc->n_cvec > 0) {
        e = hipMalloc(&p->d_cvec, sizeof(double) * (size_t)desc->n_cvec);
        if (e == hipSuccess)
            e = hipMemcpy(p->d_cvec, desc->cvec, sizeof(double) * (size_t)desc->n_cvec,
                          hipMemcpyHostToDevice);
    }
    if (e == hipSuccess && p->n_par > 0) e = hipMalloc(&p->d_theta, sizeof(double) * (size_t)p->n_par);
    if (e == hipSuccess) e = hipMalloc(&p->d_x, sizeof(double) * 2 * (size_t)p->n);      // [x | h]
    if (e == hipSuccess) p->d_h = p->d_x + p->n;
    if (e == hipSuccess) e = hipMalloc(&p->d_f0, sizeof(double) * (size_t)p->m);
    if (e == hipSuccess) e = hipMalloc(&p->d_y0, sizeof(double) * (size_t)(info.n_y0 > 0 ? info.n_y0 : 1));
    if (e == hipSuccess) e = hipMalloc(&p->d_xop, sizeof(double) * (size_t)(info.n_y0 > 0 ? info.n_y0 : 1));
    if (e == hipSuccess) e = hipMalloc(&p->d_t0, sizeof(double) * (size_t)p->m);
    if (e == hipSuccess) e = hipMalloc(&p->d_z, sizeof(double) * (size_t)p->m);
    if (e == hipSuccess) e = hipMalloc(&p->d_flags, OGK_FLAG_WORDS * sizeof(int));
    if (e == hipSuccess) e = hipMemset(p->d_flags, 0, OGK_FLAG_WORDS * sizeof(int));
    if (e == hipSuccess && getenv("OGPSX_TRACE")) {
        e = hipMalloc(&p->d_trace, sizeof(double) * OG_TRACE_DOUBLES);
        if (e == hipSuccess) e = hipMemset(p->d_trace, 0, sizeof(double) * OG_TRACE_DOUBLES);
    }
    // one pair per registration, pair 0 for unregistered buffers, the last pair for og_shard_unpack_dev of a rank
    // that owns no columns (state: no NaN fill; launches so far: 0)
    if (e == hipSuccess) e = hipMalloc(&p->d_state, 2 * (OG_MAX_JT_REGS + 2) * sizeof(uint32_t));
    if (e == hipSuccess) e = hipMemset(p->d_state, 0xff, 2 * (OG_MAX_JT_REGS + 2) * sizeof(uint32_t));
    if (e == hipSuccess) e = hipMemset(p->d_state + 2 * (OG_MAX_JT_REGS + 1) + 1, 0, sizeof(uint32_t));
    p->n_eval_blocks = info.n_eval_blocks;
    p->fused_ok = info.fused_ok != 0;
    const char* mode_env = getenv("OGPSX_SWEEP");
    // One launch (evaluation + structured sweep) whenever the output is a registered persistent-zero buffer;
    // measured against the two-launch form with such a buffer (bench step, us, one launch / two): C2 4.8 / 8.1,
    // C3 7.6 / 12.4, C4 13.9 / 22.6, C5 23.9 / 33.0.  An unregistered buffer always takes two launches (the
    // module decides: the one-launch form never fills).
    p->sweep_mode = OGK_FUSED;
    if (mode_env && std::string(mode_env) == "dense") p->sweep_mode = OGK_DENSE, p->exact_mode = OGK_EXACT_DENSE;
    if (mode_env && std::string(mode_env) == "split") p->sweep_mode = OGK_SWEEP;
    if (mode_env && std::string(mode_env) == "fused") p->sweep_mode = OGK_FUSED;
    if (p->n_eval_blocks <= 0 && p->sweep_mode == OGK_FUSED) p->sweep_mode = OGK_SWEEP;
    if (e == hipSuccess) e = hipStreamCreate(&p->stream);
    if (e != hipSuccess) {
        og_problem_destroy(p);
        return fail(100 + (int)e, std::string("og_problem_create: ") + hipGetErrorString(e));
    }
    *out = p;
    return 0;
}

void og_problem_destroy(og_handle p) {
    if (!p) return;
    hipSetDevice(p->device);
    while (!p->batches.empty()) og_batch_destroy(p->batches.back());
    if (p->batch_module) dlclose(p->batch_module);
    if (p->batch_exact_module) dlclose(p->batch_exact_module);
    if (p->par_module) dlclose(p->par_module);
    if (p->dir_module) dlclose(p->dir_module);
    if (p->adj_module) dlclose(p->adj_module);
    if (p->hvp_module) dlclose(p->hvp_module);
    if (p->mix_module) dlclose(p->mix_module);
    if (p->hess_module) dlclose(p->hess_module);
    if (p->pp_module) dlclose(p->pp_module);
    og_shard_comm_destroy(p);
    if (p->stream) hipStreamDestroy(p->stream);
    hipFree(p->d_dfrag);
    hipFree(p->d_cvec);
    hipFree(p->d_theta);
    hipFree(p->d_pj);
    hipFree(p->d_dir);
    hipFree(p->d_adj);
    hipFree(p->d_hvp);
    hipFree(p->d_mix);
    hipFree(p->d_pp);
    hipFree(p->d_hess_plan);
    hipFree(p->d_hess);
    hipFree(p->d_x);
    hipFree(p->d_f0);
    hipFree(p->d_jt);
    hipFree(p->d_y0);
    hipFree(p->d_xop);
    hipFree(p->d_t0);
    hipFree(p->d_z);
    hipFree(p->d_flags);
    hipFree(p->d_state);
    hipFree(p->d_trace);
    hipFree(p->d_indptr);
    hipFree(p->d_rows);
    hipFree(p->d_down);
    hipFree(p->d_shard_off);
    for (auto& r : p->host_regs)
        if (r.mapped && r.registered_here) (void)hipHostUnregister(r.ptr);
    (void)hipGetLastError();            // (a matrix its owner has already unmapped or freed: not this handle's error)
    if (p->h_up) hipHostFree(p->h_up);
    if (p->h_xh) hipHostFree(p->h_xh);
    if (p->h_down) hipHostFree(p->h_down);
    for (hipEvent_t ev : p->down_ev)
        if (ev) hipEventDestroy(ev);
    for (int k = 1; k < p->launch.n_parts; ++k)
        if (p->launch.handle[k]) dlclose(p->launch.handle[k]);
    if (p->module) dlclose(p->module);
    delete p;
}

int og_sweep_mode(og_handle p) { return p ? p->sweep_mode : 0; }

int og_one_launch(og_handle p) { return (p && one_launch(p)) ? 1 : 0; }

int og_nonfinite_rows(og_handle p, void* hip_stream, int32_t* rows) {
    if (!p || !rows) return fail(1, "og_nonfinite_rows: null argument");
    if (!p->nf_read) return fail(1, "og_nonfinite_rows: nothing has been evaluated on this handle");
    OG_HIP(hipSetDevice(p->device));
    OG_HIP(hipStreamSynchronize((hipStream_t)hip_stream));
    int count = 0;
    OG_HIP(hipMemcpy(&count, p->nf_read, sizeof(int), hipMemcpyDeviceToHost));
    *rows = count;
    return 0;
}

int og_device_read(int32_t device, const void* d_src, void* dst, int64_t bytes) {
    if (!d_src || !dst || bytes < 0) return fail(1, "og_device_read: bad argument");
    OG_HIP(hipSetDevice(device));
    OG_HIP(hipDeviceSynchronize());
    OG_HIP(hipMemcpy(dst, d_src, (size_t)bytes, hipMemcpyDeviceToHost));
    return 0;
}

int og_trace_read(og_handle p, double* out, int64_t count) {
    if (!p || !out) return fail(1, "og_trace_read: null argument");
    if (!p->d_trace) return fail(1, "og_trace_read: the handle was created without OGPSX_TRACE=1");
    if (count < 0 || (size_t)count > OG_TRACE_DOUBLES) return fail(1, "og_trace_read: bad count");
    OG_HIP(hipSetDevice(p->device));
    OG_HIP(hipDeviceSynchronize());
    OG_HIP(hipMemcpy(out, p->d_trace, sizeof(double) * (size_t)count, hipMemcpyDeviceToHost));
    OG_HIP(hipMemset(p->d_trace, 0, sizeof(double) * OG_TRACE_DOUBLES));
    return 0;
}

int og_jt_register_dev(og_handle p, double* d_JT, int32_t lo, int32_t hi, void* hip_stream) {
    if (!p || !d_JT) return fail(1, "og_jt_register_dev: null argument");
    if (lo < 0 || hi > p->n || lo >= hi) return fail(1, "og_jt_register_dev: bad column range");
    OG_HIP(hipSetDevice(p->device));
    hipStream_t s = (hipStream_t)hip_stream;
    og_problem_s::jt_reg* reg = nullptr;
    for (auto& r : p->regs)
        if (r.ptr == d_JT) reg = &r;
    if (!reg) {
        if ((int)p->regs.size() >= OG_MAX_JT_REGS)
            return fail(6, "og_jt_register_dev: too many registered buffers on this handle");
        // a free state word
        std::vector<char> used(OG_MAX_JT_REGS + 1, 0);
        for (auto& r : p->regs) used[r.slot] = 1;
        int slot = 1;
        while (used[slot]) ++slot;
        p->regs.push_back({d_JT, lo, hi, slot});
        reg = &p->regs.back();
    }
    reg->lo = lo;
    reg->hi = hi;
    OG_HIP(hipMemsetAsync(d_JT, 0, sizeof(double) * (size_t)(hi - lo) * (size_t)p->m, s));
    OG_HIP(hipMemsetAsync(p->d_state + 2 * reg->slot, 0xff, sizeof(uint32_t), s));        // state: no NaN fill
    OG_HIP(hipMemsetAsync(p->d_state + 2 * reg->slot + 1, 0, sizeof(uint32_t), s));       // launches so far
    return 0;
}

int og_jt_unregister_dev(og_handle p, double* d_JT) {
    if (!p) return fail(1, "og_jt_unregister_dev: null handle");
    for (size_t i = 0; i < p->regs.size(); ++i)
        if (p->regs[i].ptr == d_JT) {
            p->regs.erase(p->regs.begin() + (long)i);
            return 0;
        }
    return fail(1, "og_jt_unregister_dev: buffer is not registered");
}

int og_jt_register_host(og_handle p, double* JT, int32_t lo, int32_t hi) {
    if (!p || !JT) return fail(1, "og_jt_register_host: null argument");
    if (lo < 0 || hi > p->n || lo >= hi) return fail(1, "og_jt_register_host: bad column range");
    int rc = ensure_pattern(p);
    if (rc) return rc;
    const size_t bytes = sizeof(double) * (size_t)(hi - lo) * (size_t)p->m;
    memset(JT, 0, bytes);
    for (auto& r : p->host_regs)
        if (r.ptr == JT) {
            r.lo = lo, r.hi = hi, r.dirty = false;
            if (r.mapped && og_jt_register_dev(p, r.mapped, lo, hi, p->stream) == 0) {
                OG_HIP(hipStreamSynchronize(p->stream));
                memset(JT, 0, bytes);
            }
            return 0;
        }
    // Round 6 (0.093 ms per host-pointer sweep at C3, of which 39 us are upload + launch + the packed copy
    // and 43 us the host's scatter of a cache-cold staging buffer): the matrix is page-locked and mapped, the sweep writes
    // its structural non-zeros into it over PCIe itself - the same persistent-zero protocol as a device buffer
    // (og_jt_register_dev on the mapped address: state words on the device, a NaN fill cleans itself with the next
    // sweep).  A host that refuses the registration keeps the packed path.
    double* mapped = nullptr;
    bool registered_here = false;
    static const bool staged = [] { const char* e = getenv("OGPSX_HOST"); return e && std::string(e) == "staged"; }();
    if (!staged && one_launch(p)) {
        OG_HIP(hipSetDevice(p->device));
        void* dev = nullptr;
        // memory that came from og_pinned_alloc / hipHostMalloc is mapped already (and in the driver's own large fragments:
        // a handful of translations per sweep where a page-locked malloc'ed matrix of 4 KB pages needs 4 500)
        hipPointerAttribute_t attr;
        const bool pinned_already = hipPointerGetAttributes(&attr, JT) == hipSuccess && attr.type == hipMemoryTypeHost;
        (void)hipGetLastError();
        if (pinned_already || hipHostRegister(JT, bytes, hipHostRegisterMapped) == hipSuccess) {
            if (hipHostGetDevicePointer(&dev, JT, 0) == hipSuccess && dev &&
                og_jt_register_dev(p, (double*)dev, lo, hi, p->stream) == 0 &&
                hipStreamSynchronize(p->stream) == hipSuccess) {
                mapped = (double*)dev;
                memset(JT, 0, bytes);
                registered_here = !pinned_already;
            } else if (!pinned_already) {
                (void)hipHostUnregister(JT);
            }
        }
        (void)hipGetLastError();
    }
    og_problem_s::host_reg fresh;
    fresh.ptr = JT;
    fresh.lo = lo;
    fresh.hi = hi;
    fresh.dirty = false;
    fresh.mapped = mapped;
    fresh.registered_here = registered_here;
    p->host_regs.push_back(fresh);
    return 0;
}

int og_pinned_alloc(int64_t bytes, void** out) {
    if (bytes <= 0 || !out) return fail(1, "og_pinned_alloc: bad arguments");
    void* ptr = nullptr;
    const hipError_t e = hipHostMalloc(&ptr, (size_t)bytes, hipHostMallocDefault);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        return fail(100 + (int)e, std::string("og_pinned_alloc: ") + hipGetErrorString(e));
    }
    *out = ptr;
    return 0;
}

int og_pinned_free(void* ptr) {
    if (!ptr) return 0;
    const hipError_t e = hipHostFree(ptr);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        return fail(100 + (int)e, std::string("og_pinned_free: ") + hipGetErrorString(e));
    }
    return 0;
}

int og_jt_host_path(og_handle p, const double* JT, int32_t* path) {
    if (!p || !path) return fail(1, "og_jt_host_path: null argument");
    *path = -1;
    for (auto& r : p->host_regs)
        if (r.ptr == JT) *path = !one_launch(p) ? 3 : !r.mapped ? 2 : r.choice;
    return 0;
}

int og_jt_unregister_host(og_handle p, double* JT) {
    if (!p) return fail(1, "og_jt_unregister_host: null handle");
    for (size_t i = 0; i < p->host_regs.size(); ++i)
        if (p->host_regs[i].ptr == JT) {
            if (p->host_regs[i].mapped) {
                (void)hipStreamSynchronize(p->stream);
                (void)og_jt_unregister_dev(p, p->host_regs[i].mapped);
                if (p->host_regs[i].registered_here) (void)hipHostUnregister(JT);
                (void)hipGetLastError();
            }
            p->host_regs.erase(p->host_regs.begin() + (long)i);
            return 0;
        }
    return fail(1, "og_jt_unregister_host: matrix is not registered");
}

int og_pattern(og_handle p, int32_t lo, int32_t hi, int64_t* nnz, int64_t* indptr, int32_t* rows) {
    if (!p) return fail(1, "og_pattern: null handle");
    if (lo < 0 || hi > p->n || lo > hi) return fail(1, "og_pattern: bad column range");
    int rc = ensure_pattern(p);
    if (rc) return rc;
    const int64_t first = p->indptr[(size_t)lo], count = p->indptr[(size_t)hi] - first;
    if (nnz) *nnz = count;
    if (indptr)
        for (int j = lo; j <= hi; ++j) indptr[j - lo] = p->indptr[(size_t)j] - first;
    if (rows && count) memcpy(rows, p->rows.data() + first, sizeof(int32_t) * (size_t)count);
    return 0;
}

int og_pack_dev(og_handle p, const double* d_JT, int32_t lo, int32_t hi, double* d_vals, void* hip_stream) {
    if (!p || !d_JT || !d_vals) return fail(1, "og_pack_dev: null argument");
    if (lo < 0 || hi > p->n || lo > hi) return fail(1, "og_pack_dev: bad column range");
    int rc = ensure_pattern(p);
    if (rc) return rc;
    ogk_args a;
    fill_args(p, &a, nullptr, nullptr, p->d_f0, const_cast<double*>(d_JT), lo, hi, false);
    pattern_args(p, &a, p->d_indptr);
    a.pvals = d_vals - p->indptr[(size_t)lo];
    rc = p->launch(&a, OGK_PACK, hip_stream);
    return launched(rc, "og_pack_dev");
}

int og_unpack_dev(og_handle p, const double* d_vals, int32_t lo, int32_t hi, double* d_JT, void* hip_stream) {
    if (!p || !d_JT || !d_vals) return fail(1, "og_unpack_dev: null argument");
    if (lo < 0 || hi > p->n || lo > hi) return fail(1, "og_unpack_dev: bad column range");
    int rc = ensure_pattern(p);
    if (rc) return rc;
    ogk_args a;
    fill_args(p, &a, nullptr, nullptr, p->d_f0, nullptr, lo, lo, false);
    a.jt = d_JT - (size_t)lo * (size_t)p->m;       // the kernel indexes rows by absolute column
    a.jt_sparse = 0;                               // plain scatter: no fill
    pattern_args(p, &a, p->d_indptr);
    a.pvals = const_cast<double*>(d_vals) - p->indptr[(size_t)lo];
    a.ulo = lo;
    a.uhi = hi;
    rc = p->launch(&a, OGK_UNPACK, hip_stream);
    return launched(rc, "og_unpack_dev");
}

int og_shard_plan(og_handle p, int32_t world, int32_t* block_cols, int64_t* block_vals) {
    if (!p) return fail(1, "og_shard_plan: null handle");
    if (world < 1) return fail(1, "og_shard_plan: world must be >= 1");
    int rc = ensure_pattern(p);
    if (rc) return rc;
    OG_HIP(hipSetDevice(p->device));
    const int n = p->n, B = (n + world - 1) / world;
    int64_t worst = 0;
    for (int r = 0; r < world; ++r) {
        const int lo = std::min(n, r * B), hi = std::min(n, lo + B);
        worst = std::max(worst, p->indptr[(size_t)hi] - p->indptr[(size_t)lo]);
    }
    std::vector<int64_t> off((size_t)n);
    for (int j = 0; j < n; ++j) {
        const int r = j / B;
        off[(size_t)j] = (int64_t)r * worst + p->indptr[(size_t)j] - p->indptr[(size_t)(r * B)];
    }
    if (p->d_shard_off) OG_HIP(hipFree(p->d_shard_off));
    p->d_shard_off = nullptr;
    OG_HIP(hipMalloc(&p->d_shard_off, sizeof(int64_t) * (size_t)(n ? n : 1)));
    OG_HIP(hipMemcpy(p->d_shard_off, off.data(), sizeof(int64_t) * (size_t)n, hipMemcpyHostToDevice));
    p->shard_world = world;
    p->shard_block_vals = worst;
    if (block_cols) *block_cols = B;
    if (block_vals) *block_vals = worst;
    return 0;
}

int og_shard_pack_dev(og_handle p, int32_t rank, const double* d_JT_block, double* d_send, void* hip_stream) {
    if (!p || !d_JT_block || !d_send) return fail(1, "og_shard_pack_dev: null argument");
    if (!p->shard_world || rank < 0 || rank >= p->shard_world)
        return fail(1, "og_shard_pack_dev: no shard plan, or rank out of range");
    const int n = p->n, B = (n + p->shard_world - 1) / p->shard_world;
    const int lo = std::min(n, rank * B), hi = std::min(n, lo + B);
    ogk_args a;
    fill_args(p, &a, nullptr, nullptr, p->d_f0, const_cast<double*>(d_JT_block), lo, hi, false);
    pattern_args(p, &a, p->d_shard_off);
    a.pvals = d_send - (int64_t)rank * p->shard_block_vals;
    int rc = p->launch(&a, OGK_PACK, hip_stream);
    return launched(rc, "og_shard_pack_dev");
}

int og_shard_sweep_dev(og_handle p, int32_t rank, const double* d_x, const double* d_h, double* d_JT_block,
                       double* d_F0, double* d_send, void* hip_stream) {
    if (!p || !d_x || !d_h || !d_JT_block || !d_F0 || !d_send) return fail(1, "og_shard_sweep_dev: null argument");
    if (!p->shard_world || rank < 0 || rank >= p->shard_world)
        return fail(1, "og_shard_sweep_dev: no shard plan, or rank out of range");
    const int n = p->n, B = (n + p->shard_world - 1) / p->shard_world;
    const int lo = std::min(n, rank * B), hi = std::min(n, lo + B);
    if (hi <= lo) return og_eval_dev(p, d_x, d_F0, hip_stream);        // more ranks than columns: F(x0) only
    ogk_args a;
    fill_args(p, &a, d_x, d_h, d_F0, d_JT_block, lo, hi);
    if (one_launch(p) && a.jt_sparse) {
        // ONE launch: F(x0), the block's non-zeros into J_T and, the same values, into this rank's message
        one_launch_args(p, &a);
        a.poff = p->d_shard_off;
        a.pvals = d_send - (int64_t)rank * p->shard_block_vals;
        return launched(p->launch(&a, OGK_FUSED, hip_stream), "og_shard_sweep_dev");
    }
    const int rc = og_fd_sweep_dev(p, d_x, d_h, lo, hi, d_JT_block, d_F0, hip_stream);
    return rc ? rc : og_shard_pack_dev(p, rank, d_JT_block, d_send, hip_stream);
}

int og_shard_unpack_dev(og_handle p, int32_t rank, const double* d_recv, double* d_JT_full, void* hip_stream) {
    if (!p || !d_recv || !d_JT_full) return fail(1, "og_shard_unpack_dev: null argument");
    if (!p->shard_world || rank < 0 || rank >= p->shard_world)
        return fail(1, "og_shard_unpack_dev: no shard plan, or rank out of range");
    const int n = p->n, B = (n + p->shard_world - 1) / p->shard_world;
    const int lo = std::min(n, rank * B), hi = std::min(n, lo + B);
    ogk_args a;
    // the registration of this rank's own block inside the replica tells whether the previous step left a NaN
    // fill behind; same generation as the sweep that was just enqueued (no new launch into the block)
    fill_args(p, &a, nullptr, nullptr, p->d_f0, d_JT_full + (size_t)lo * (size_t)p->m, lo, hi, false);
    if (!a.jt_sparse && hi > lo)
        return fail(1, "og_shard_unpack_dev: this rank's block of the replica is not a registered buffer");
    a.jt = d_JT_full;
    a.jt_sparse = 1;
    pattern_args(p, &a, p->d_shard_off);
    a.pvals = const_cast<double*>(d_recv);
    a.ulo = 0;
    a.uhi = n;
    int rc = 0;
    if (hi <= lo) {
        // more ranks than columns: no sweep of this rank keeps the replica's NaN history, so the unpack does - its
        // own pair of words, one count per step, and the kernel marks a step whose F(x0) had non-finite rows
        a.jt_state = p->d_state + 2 * (OG_MAX_JT_REGS + 1);
        a.jt_launches = a.jt_state + 1;
        a.jt_bump = 1;
        rc = p->launch(&a, OGK_COUNT_LAUNCH, hip_stream);
    }
    if (!rc) rc = p->launch(&a, OGK_UNPACK, hip_stream);
    return launched(rc, "og_shard_unpack_dev");
}

int og_problem_dims(og_handle p, int32_t* n, int32_t* m, int32_t* m_eq, int32_t* m_ineq) {
    if (!p) return fail(1, "og_problem_dims: null handle");
    if (n) *n = p->n;
    if (m) *m = p->m;
    if (m_eq) *m_eq = p->m_eq;
    if (m_ineq) *m_ineq = p->m_ineq;
    return 0;
}

// The two-launch forms count the non-finite rows of F(x0) into one of two words, in turn: outside a capture the
// evaluation before this one has cleared the word this one counts into (ogk_eval: *nonfinite_next = 0).  A replayed
// graph is its own predecessor: it would count on top of the count it left, and after one non-finite point every
// later replay would fill with z, mark the buffer and report rows that are no longer there.  A capture therefore
// clears its word itself, as a node of the graph.
static int clear_count_in_a_capture(int* d_count, void* hip_stream) {
    hipStreamCaptureStatus capturing = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing((hipStream_t)hip_stream, &capturing) != hipSuccess) {
        (void)hipGetLastError();
        return 0;
    }
    if (capturing == hipStreamCaptureStatusActive)
        OG_HIP(hipMemsetAsync(d_count, 0, sizeof(int), (hipStream_t)hip_stream));
    return 0;
}

int og_eval_dev(og_handle p, const double* d_x, double* d_F, void* hip_stream) {
    if (!p || !d_x || !d_F) return fail(1, "og_eval_dev: null argument");
    ogk_args a;
    p->flag_slot ^= 1;                      // this evaluation counts non-finite rows into a fresh slot
    fill_args(p, &a, d_x, nullptr, d_F, nullptr, 0, 0);
    p->nf_read = a.nonfinite;
    int rc = p->launch(&a, OGK_EVAL, hip_stream);
    return launched(rc, "og_eval_dev");
}

int og_fd_sweep_dev(og_handle p, const double* d_x, const double* d_h, int32_t lo, int32_t hi,
                    double* d_JT, double* d_F0, void* hip_stream) {
    if (!p || !d_x || !d_h || !d_JT || !d_F0) return fail(1, "og_fd_sweep_dev: null argument");
    if (lo < 0 || hi > p->n || lo > hi) return fail(1, "og_fd_sweep_dev: bad column range");
    ogk_args a;
    fill_args(p, &a, d_x, d_h, d_F0, d_JT, lo, hi);
    int rc;
    if (one_launch(p) && a.jt_sparse && hi > lo) {
        // ONE launch: the ticket and the buffer's launch number, too, are kept by the kernel itself
        one_launch_args(p, &a);
        rc = p->launch(&a, OGK_FUSED, hip_stream);
    } else {
        p->flag_slot ^= 1;
        a.nonfinite = p->d_flags + p->flag_slot;
        a.nonfinite_next = p->d_flags + (p->flag_slot ^ 1);
        p->nf_read = a.nonfinite;
        a.jt_bump = a.jt_sparse;                    // F(x0) first: the sweep subtracts it; it also counts the launch
        rc = clear_count_in_a_capture(a.nonfinite, hip_stream);
        if (rc) return rc;
        rc = p->launch(&a, OGK_EVAL, hip_stream);
        if (!rc) rc = p->launch(&a, columns_mode(p), hip_stream);
    }
    return launched(rc, "og_fd_sweep_dev");
}

int og_fd_columns_dev(og_handle p, const double* d_x, const double* d_h, int32_t lo, int32_t hi,
                      double* d_JT, const double* d_F0, void* hip_stream) {
    if (!p || !d_x || !d_h || !d_JT || !d_F0) return fail(1, "og_fd_columns_dev: null argument");
    if (lo < 0 || hi > p->n || lo > hi) return fail(1, "og_fd_columns_dev: bad column range");
    ogk_args a;
    fill_args(p, &a, d_x, d_h, const_cast<double*>(d_F0), d_JT, lo, hi);
    int rc = a.jt_sparse ? p->launch(&a, OGK_COUNT_LAUNCH, hip_stream) : 0;     // (into the registered buffer)
    if (!rc) rc = p->launch(&a, columns_mode(p), hip_stream);
    return launched(rc, "og_fd_columns_dev");
}

int og_jacobian_exact_dev(og_handle p, const double* d_x, int32_t lo, int32_t hi, double* d_JT, double* d_F0,
                          void* hip_stream) {
    if (!p || !d_x || !d_JT || !d_F0) return fail(1, "og_jacobian_exact_dev: null argument");
    if (lo < 0 || hi > p->n || lo > hi) return fail(1, "og_jacobian_exact_dev: bad column range");
    ogk_args a;
    p->flag_slot ^= 1;
    fill_args(p, &a, d_x, nullptr, d_F0, d_JT, lo, hi);
    p->nf_read = a.nonfinite;
    a.jt_bump = a.jt_sparse;
    int rc = p->launch(&a, OGK_EVAL, hip_stream);   // F(x0) and the base collocation products
    if (!rc) rc = p->launch(&a, p->exact_mode, hip_stream);   // forward-mode derivatives, column by column
    return launched(rc, "og_jacobian_exact_dev");
}

int og_eval(og_handle p, const double* x, double* F) {
    if (!p || !x || !F) return fail(1, "og_eval: null argument");
    OG_HIP(hipSetDevice(p->device));
    int rc = upload_point(p, x, nullptr);
    if (rc) return rc;
    rc = og_eval_dev(p, p->d_x, p->d_f0, p->stream);
    if (rc) return rc;
    OG_HIP(hipMemcpyAsync(p->h_down, p->d_f0, sizeof(double) * p->m, hipMemcpyDeviceToHost, p->stream));
    OG_HIP(hipStreamSynchronize(p->stream));
    memcpy(F, p->h_down, sizeof(double) * (size_t)p->m);
    return 0;
}

int og_fd_sweep(og_handle p, const double* x, const double* hstep, int32_t lo, int32_t hi,
                double* JT, double* F0) {
    if (!p || !x || !hstep || !JT) return fail(1, "og_fd_sweep: null argument");
    if (lo < 0 || hi > p->n || lo > hi) return fail(1, "og_fd_sweep: bad column range");
    OG_HIP(hipSetDevice(p->device));
    if ((size_t)(hi - lo) * (size_t)p->m == 0) {        // empty column range: only F(x) is produced
        if (!F0) return 0;
        return og_eval(p, x, F0);
    }
    int rc = own_jt(p, lo, hi);
    if (rc) return rc;
    g_host_clock.start();
    // (mapped matrix: the launch also reads x | h in place, out of a pinned buffer of their own - non-coherent host memory,
    // cached in L2 for the launch and visible at its boundary - instead of waiting for their copy: 5 us of a call.
    // OGPSX_HOST=copyx keeps the copy.)
    static const bool readx_mode = [] { const char* e = getenv("OGPSX_HOST"); return !(e && std::string(e) == "copyx"); }();
    og_problem_s::host_reg* reg = find_host_reg(p, JT, lo, hi);
    static const int forced = [] {
        const char* e = getenv("OGPSX_HOST");
        return (e && (std::string(e) == "mapped" || std::string(e) == "copyx")) ? 1 : 0;
    }();
    // Which form this call takes.  The mapped launch needs the matrix mapped AND its mapped address registered on the
    // device for exactly this block; while the trial runs (host_reg) a call that could take it may be sent down the
    // packed form instead.  Everything that is not the mapped launch reads p->d_x | p->d_h and therefore starts with
    // upload_point: no path reaches them with what an in-place call before left there.
    const bool mappable = reg && reg->mapped && one_launch(p) && find_jt_reg(p, reg->mapped, lo, hi);
    const bool mapped = mappable && reg->take_mapped(forced != 0);
    const bool trial = mappable && reg->choice == 0;
    const double t_call = trial ? host_clock::now() : 0.0;
    if (mapped) {
        rc = sweep_mapped(p, reg, x, hstep, lo, hi, JT, F0, readx_mode);
    } else {
        rc = upload_point(p, x, hstep);
        g_host_clock.mark(0);
        if (!rc) rc = reg && one_launch(p) ? sweep_packed(p, lo, hi, JT, F0) : sweep_download(p, lo, hi, JT, F0);
    }
    if (!rc && trial) reg->trial_call(host_clock::now() - t_call);
    return rc;
}

int og_jacobian_exact(og_handle p, const double* x, int32_t lo, int32_t hi, double* JT, double* F0) {
    if (!p || !x || !JT) return fail(1, "og_jacobian_exact: null argument");
    if (lo < 0 || hi > p->n || lo > hi) return fail(1, "og_jacobian_exact: bad column range");
    OG_HIP(hipSetDevice(p->device));
    const size_t need = (size_t)(hi - lo) * (size_t)p->m;
    if (need == 0) {
        if (!F0) return 0;
        return og_eval(p, x, F0);
    }
    {
        const int rcj = own_jt(p, lo, hi);
        if (rcj) return rcj;
    }
    int rc = upload_point(p, x, nullptr);
    if (rc) return rc;
    rc = og_jacobian_exact_dev(p, p->d_x, lo, hi, p->d_jt, p->d_f0, p->stream);
    if (rc) return rc;
    return download_block(p, lo, hi, JT, F0);
}

}  // extern "C"

// ------------------------------------------------------------------------------------------------
// Batches: `capacity` lanes of one handle, each with everything ogk_args makes per-point (scratch, counters, ticket,
// a persistent-zero n x m J_T with its own state words); one launch of the module's batch part (ogk.h:
// ogk_batch_args) runs `count` of them.  The lane records are written once, here; a launch takes the table and the
// lane count, and the one-thread-per-record bind kernel ahead of it says where the caller's arrays are - skipped
// while they are where they were (and never skipped on a capturing stream: a captured graph binds for itself).
// ------------------------------------------------------------------------------------------------
struct og_batch_s {
    og_problem_s* p = nullptr;
    int capacity = 0;
    int64_t nnz = 0;
    ogk_args* d_table = nullptr;            // [OGK_BATCH_SETS][capacity]
    std::vector<ogk_args> table;            // the host's copy (the per-lane launches of the split / dense form use it)
    double* d_jt = nullptr;                 // [capacity][n][m]
    double* d_scratch = nullptr;            // per lane: y0 | xop | t0 | z
    size_t scratch_lane = 0, n_y0 = 0;
    int* d_flags = nullptr;                 // [capacity][OGK_FLAG_WORDS]: as og_problem_s::d_flags
    uint32_t* d_state = nullptr;            // [capacity][2]: jt_state, jt_launches
    // per lane: the word of its d_flags that holds the count of non-finite rows at its most recent point (OGK_FLAG_COUNT_A
    // after an evaluation launch, OGK_FLAG_FUSED_RESULT after a one-launch sweep) - a lane keeps it while later launches
    // run fewer lanes
    std::vector<int> nf_word;
    hipStream_t last_stream = nullptr;      // of the most recent launch (og_batch_lane_dev waits for this one only)
    // host-pointer entry points: device arrays [X | H], F, packed values and their pinned images
    double *d_xh = nullptr, *d_f = nullptr, *d_vals = nullptr;
    double *h_up = nullptr, *h_down = nullptr;
    int* h_flags = nullptr;
    // a module with run-time parameters: every lane's own copy of the constant table ([capacity][n_cvec]; the lane
    // records' cvec point into it), and [capacity][n_par] staging of the host-pointer og_parameters_batch
    double* d_cvec = nullptr;
    double *d_th = nullptr, *h_th = nullptr;
    double* d_pj = nullptr;                 // [capacity][n_par][m] staging of the host-pointer og_parameter_jacobian_batch
    double* d_dj = nullptr;                 // [capacity][m] staging of the host-pointer og_directional_batch
    double* d_aj = nullptr;                 // [W[capacity][m] | G[capacity][n]] staging of the host-pointer og_adjoint_batch
    double* d_hj = nullptr;                 // [W[capacity][m] | Q[capacity][n]] staging of the host-pointer og_hessian_vector_batch
    double* d_mj = nullptr;                 // [W[capacity][m] | S[capacity][n_par][n]] staging of the host-pointer og_adjoint_parameter_batch
    double* d_ppj = nullptr;                // [W[capacity][m] | S[capacity][n_par][n_par]] staging of the host-pointer og_parameter_hessian_batch
    double* d_hm = nullptr;                 // [W[capacity][m] | H[capacity][nnz]] staging of the host-pointer og_hessian_matrix_batch
};

namespace {

// live batches: a batch whose handle is gone is not among them.  Batches of different handles may be used from
// different threads: the list has a lock of its own
std::mutex g_batches_lock;
std::vector<og_batch_s*> g_batches;

og_batch_s* live_batch(og_batch b) {
    std::lock_guard<std::mutex> guard(g_batches_lock);
    for (og_batch_s* q : g_batches)
        if (q == b) return q;
    return nullptr;
}

int batch_check(og_batch b, int32_t count, const char* who) {
    if (!b) return fail(1, std::string(who) + ": null batch");
    if (!live_batch(b)) return fail(1, std::string(who) + ": the batch or its handle has been destroyed");
    if (count < 1) return fail(1, std::string(who) + ": count must be at least 1");
    if (count > b->capacity)
        return fail(1, std::string(who) + ": count " + std::to_string(count) + " exceeds the batch's capacity " +
                           std::to_string(b->capacity));
    return 0;
}

ogk_batch_args batch_args(og_batch_s* b, int set, int count) {
    ogk_batch_args ba;
    memset(&ba, 0, sizeof ba);
    ba.lanes = b->d_table + (size_t)set * (size_t)b->capacity;
    ba.count = count;
    ba.capacity = b->capacity;
    return ba;
}

// Where this call's arrays are, written into the lane records by a one-thread-per-record launch ahead of EVERY batched
// launch: the records are device state that a replayed graph rewrites behind the host's back, so the host keeps no
// memory of what they hold.  The same launch zeroes the non-finite counter of the lanes an evaluation is about to
// run (clear_set: the record set of that evaluation, or -1).
// (vals_stride: doubles per lane of `vals` when it is not an array of packed non-zeros)
int batch_bind(og_batch_s* b, int count, const double* X, const double* H, double* F, double* vals, int clear_set,
               hipStream_t s, const char* who, int64_t vals_stride = -1) {
    ogk_batch_args ba = batch_args(b, 0, count);        // (the whole table)
    ba.X = X, ba.H = H, ba.F0 = F, ba.vals = vals, ba.nnz = vals_stride >= 0 ? vals_stride : b->nnz;
    ba.clear_set = clear_set;
    const int rc = b->p->batch_launch(&ba, OGK_BATCH_BIND, s);
    if (rc) return launched(rc, who);
    b->last_stream = s;
    return 0;
}

// One batched launch of `count` lanes on a record set -> the launcher's code.  An evaluation or a one-launch sweep also
// moves the lanes' counts of non-finite rows (og_batch_s::nf_word).
int batch_run(og_batch_s* b, int set, int mode, int count, hipStream_t s) {
    const ogk_batch_args ba = batch_args(b, set, count);
    if (mode == OGK_BATCH_EXACT) return b->p->batch_exact_launch(&ba, mode, s);
    std::fill_n(b->nf_word.begin(), count, mode == OGK_BATCH_FUSED ? (int)OGK_FLAG_FUSED_RESULT : (int)OGK_FLAG_COUNT_A);
    return b->p->batch_launch(&ba, mode, s);
}

// The validation forms of a batch: after the batched evaluation on record set 2, the handle's own kernel `mode` lane
// by lane on that lane's record, and the pack where packed values are asked for -> the launcher's code
int batch_lanes_run(og_batch_s* b, int count, int mode, const double* d_X, const double* d_H, double* d_F0,
                    double* d_vals, hipStream_t s) {
    og_problem_s* p = b->p;
    int rc = 0;
    for (int k = 0; !rc && k < count; ++k) {
        ogk_args a = b->table[2 * (size_t)b->capacity + (size_t)k];
        a.x0 = d_X + (size_t)k * (size_t)p->n;
        if (d_H) a.h = d_H + (size_t)k * (size_t)p->n;
        a.f0 = d_F0 + (size_t)k * (size_t)p->m;
        rc = p->launch(&a, mode, s);
        if (!rc && d_vals) {
            a.pind = p->d_indptr;
            a.prow = p->d_rows;
            a.pvals = d_vals + (size_t)k * (size_t)b->nnz;
            rc = p->launch(&a, OGK_PACK, s);
        }
    }
    return rc;
}

// An on-demand part of the handle's module (`what`: the batch part, the exact batch part): open it and check that it
// was compiled from the same generated header as the module
int load_module_part(og_problem_s* p, const char* path, const std::string& who, const std::string& what, void** handle,
                     ogk_launch_batch_fn* launch) {
    if (!path) return fail(4, who + ": the module's " + what + " is not loaded and no path was given");
    void* mod = dlopen(path, RTLD_NOW | RTLD_LOCAL);
    if (!mod) return fail(4, who + ": dlopen of the " + what + " failed: " + dlerror());
    ogk_get_info_fn get_info = (ogk_get_info_fn)dlsym(mod, "ogk_get_info");
    ogk_launch_batch_fn fn = (ogk_launch_batch_fn)dlsym(mod, "ogk_launch_batch");
    ogk_info info;
    memset(&info, 0, sizeof info);
    if (get_info && fn) get_info(&info);
    if (!get_info || !fn || info.abi != OGK_ABI || info.n != p->n || info.m != p->m || info.m_eq != p->m_eq ||
        info.n_eval_blocks != p->n_eval_blocks) {
        dlclose(mod);
        return fail(5, who + ": the " + what + " does not belong to the handle's module");
    }
    *handle = mod;
    *launch = fn;
    return 0;
}

// The host-pointer entry points of a batch.  X (and H) of `c` lanes go up through the pinned buffer: the device arrays
// are [capacity][n] each, so [X | H] is one copy when the batch is full and two otherwise
int batch_upload(og_batch_s* b, size_t c, const double* X, const double* H) {
    const size_t n = (size_t)b->p->n, cap = (size_t)b->capacity;
    hipStream_t s = b->p->stream;
    memcpy(b->h_up, X, sizeof(double) * c * n);
    if (H) memcpy(b->h_up + cap * n, H, sizeof(double) * c * n);
    if (H && c == cap) {
        OG_HIP(hipMemcpyAsync(b->d_xh, b->h_up, sizeof(double) * 2 * cap * n, hipMemcpyHostToDevice, s));
        return 0;
    }
    OG_HIP(hipMemcpyAsync(b->d_xh, b->h_up, sizeof(double) * c * n, hipMemcpyHostToDevice, s));
    if (H) OG_HIP(hipMemcpyAsync(b->d_xh + cap * n, b->h_up + cap * n, sizeof(double) * c * n, hipMemcpyHostToDevice, s));
    return 0;
}

// F0 and vals in page-locked memory the device can address (og_pinned_alloc, hipHostRegister): the launch writes them
// over PCIe as it goes -> true and their device addresses; else false and the batch's own device arrays
bool batch_targets(og_batch_s* b, double* F0, double* vals, double** d_f, double** d_vals) {
    void *m_f = nullptr, *m_vals = nullptr;
    const bool mapped = hipHostGetDevicePointer(&m_f, F0, 0) == hipSuccess &&
                        hipHostGetDevicePointer(&m_vals, vals, 0) == hipSuccess && m_f && m_vals;
    if (!mapped) (void)hipGetLastError();
    *d_f = mapped ? (double*)m_f : b->d_f;
    *d_vals = mapped ? (double*)m_vals : b->d_vals;
    return mapped;
}

// The results of `c` lanes to the caller: the lanes' flag blocks for the counts of non-finite rows and, unless the
// launch wrote F0 and vals in place, the two arrays through the pinned buffer
int batch_results(og_batch_s* b, size_t c, bool in_place, double* F0, double* vals, int32_t* nonfinite) {
    const size_t m = (size_t)b->p->m, cap = (size_t)b->capacity, nnz = (size_t)b->nnz;
    hipStream_t s = b->p->stream;
    if (!in_place) {
        if (nnz) OG_HIP(hipMemcpyAsync(b->h_down, b->d_vals, sizeof(double) * c * nnz, hipMemcpyDeviceToHost, s));
        OG_HIP(hipMemcpyAsync(b->h_down + cap * nnz, b->d_f, sizeof(double) * c * m, hipMemcpyDeviceToHost, s));
    }
    OG_HIP(hipMemcpyAsync(b->h_flags, b->d_flags, sizeof(int) * OGK_FLAG_WORDS * c, hipMemcpyDeviceToHost, s));
    OG_HIP(hipStreamSynchronize(s));
    if (!in_place) {
        if (nnz) memcpy(vals, b->h_down, sizeof(double) * c * nnz);
        memcpy(F0, b->h_down + cap * nnz, sizeof(double) * c * m);
    }
    if (nonfinite)
        for (size_t k = 0; k < c; ++k) nonfinite[k] = b->h_flags[OGK_FLAG_WORDS * k + (size_t)b->nf_word[k]];
    return 0;
}

}  // namespace

extern "C" {

void og_batch_destroy(og_batch b) {
    if (!b || !live_batch(b)) return;
    {
        std::lock_guard<std::mutex> guard(g_batches_lock);
        g_batches.erase(std::find(g_batches.begin(), g_batches.end(), b));
    }
    og_problem_s* p = b->p;
    auto it = std::find(p->batches.begin(), p->batches.end(), b);
    if (it != p->batches.end()) p->batches.erase(it);
    hipSetDevice(p->device);
    hipFree(b->d_table);
    hipFree(b->d_jt);
    hipFree(b->d_scratch);
    hipFree(b->d_flags);
    hipFree(b->d_state);
    hipFree(b->d_xh);
    hipFree(b->d_f);
    hipFree(b->d_vals);
    hipFree(b->d_cvec);
    hipFree(b->d_th);
    hipFree(b->d_pj);
    hipFree(b->d_dj);
    hipFree(b->d_aj);
    hipFree(b->d_hj);
    hipFree(b->d_mj);
    hipFree(b->d_ppj);
    hipFree(b->d_hm);
    if (b->h_th) hipHostFree(b->h_th);
    if (b->h_up) hipHostFree(b->h_up);
    if (b->h_down) hipHostFree(b->h_down);
    if (b->h_flags) hipHostFree(b->h_flags);
    (void)hipGetLastError();
    delete b;
}

int og_batch_capacity(og_batch b) { return live_batch(b) ? b->capacity : 0; }

int og_batch_create(og_handle p, int32_t capacity, const char* batch_part_path, og_batch* out) {
    if (out) *out = nullptr;
    if (!p || !out) return fail(1, "og_batch_create: null argument");
    if (capacity < 1 || capacity > 65535) return fail(1, "og_batch_create: capacity must be in [1, 65535]");
    OG_HIP(hipSetDevice(p->device));
    int rc = p->batch_launch ? 0 : load_module_part(p, batch_part_path, "og_batch_create", "batch part",
                                                    &p->batch_module, &p->batch_launch);
    if (!rc) rc = ensure_pattern(p);
    if (rc) return rc;
    ogk_info info;
    memset(&info, 0, sizeof info);
    ((ogk_get_info_fn)dlsym(p->batch_module, "ogk_get_info"))(&info);

    og_batch_s* b = new og_batch_s();
    b->p = p;
    b->capacity = capacity;
    b->nnz = p->indptr[(size_t)p->n];
    b->n_y0 = (size_t)(info.n_y0 > 0 ? info.n_y0 : 1);
    b->scratch_lane = 2 * b->n_y0 + 2 * (size_t)p->m;
    b->nf_word.assign((size_t)capacity, OGK_FLAG_FUSED_RESULT);
    {
        std::lock_guard<std::mutex> guard(g_batches_lock);
        g_batches.push_back(b);
    }
    p->batches.push_back(b);
    const size_t cap = (size_t)capacity, n = (size_t)p->n, m = (size_t)p->m, nnz = (size_t)(b->nnz ? b->nnz : 1);
    // an allocation that does not fit is an error of this call (C5: 304 MB of J_T per lane)
    hipError_t e = hipMalloc(&b->d_jt, sizeof(double) * cap * n * m);
    if (e == hipSuccess) e = hipMemsetAsync(b->d_jt, 0, sizeof(double) * cap * n * m, p->stream);
    if (e == hipSuccess) e = hipMalloc(&b->d_scratch, sizeof(double) * cap * b->scratch_lane);
    if (e == hipSuccess) e = hipMalloc(&b->d_flags, sizeof(int) * OGK_FLAG_WORDS * cap);
    if (e == hipSuccess) e = hipMemsetAsync(b->d_flags, 0, sizeof(int) * OGK_FLAG_WORDS * cap, p->stream);
    if (e == hipSuccess) e = hipMalloc(&b->d_state, sizeof(uint32_t) * 2 * cap);
    if (e == hipSuccess) e = hipMalloc(&b->d_table, sizeof(ogk_args) * OGK_BATCH_SETS * cap);
    if (e == hipSuccess) e = hipMalloc(&b->d_xh, sizeof(double) * 2 * cap * n);
    if (e == hipSuccess) e = hipMalloc(&b->d_f, sizeof(double) * cap * m);
    if (e == hipSuccess) e = hipMalloc(&b->d_vals, sizeof(double) * cap * nnz);
    if (e == hipSuccess) e = hipHostMalloc(&b->h_up, sizeof(double) * 2 * cap * n, hipHostMallocDefault);
    if (e == hipSuccess) e = hipHostMalloc(&b->h_down, sizeof(double) * cap * (nnz + m), hipHostMallocDefault);
    if (e == hipSuccess) e = hipHostMalloc(&b->h_flags, sizeof(int) * OGK_FLAG_WORDS * cap, hipHostMallocDefault);
    if (p->n_par > 0) {
        // every lane's own constant table, filled with the handle's (its parameters at their current values)
        const size_t nc = (size_t)p->n_cvec, np_ = (size_t)p->n_par;
        if (e == hipSuccess) e = hipMalloc(&b->d_cvec, sizeof(double) * cap * nc);
        for (size_t k = 0; e == hipSuccess && k < cap; ++k)
            e = hipMemcpyAsync(b->d_cvec + k * nc, p->d_cvec, sizeof(double) * nc, hipMemcpyDeviceToDevice, p->stream);
        if (e == hipSuccess) e = hipMalloc(&b->d_th, sizeof(double) * cap * np_);
        if (e == hipSuccess) e = hipHostMalloc(&b->h_th, sizeof(double) * cap * np_, hipHostMallocDefault);
    }
    if (e == hipSuccess) {
        // per lane {state: no NaN fill, launches so far: 0}
        std::vector<uint32_t> st(2 * cap);
        for (size_t k = 0; k < cap; ++k) st[2 * k] = 0xffffffffu, st[2 * k + 1] = 0u;
        e = hipMemcpy(b->d_state, st.data(), sizeof(uint32_t) * 2 * cap, hipMemcpyHostToDevice);
    }
    if (e == hipSuccess) {
        b->table.resize((size_t)OGK_BATCH_SETS * cap);
        for (int set = 0; set < OGK_BATCH_SETS; ++set)
            for (size_t k = 0; k < cap; ++k) {
                ogk_args& a = b->table[(size_t)set * cap + k];
                fill_args(p, &a, nullptr, nullptr, nullptr, nullptr, 0, p->n);
                double* scr = b->d_scratch + k * b->scratch_lane;
                int* fl = b->d_flags + OGK_FLAG_WORDS * k;
                a.y0 = scr;
                a.xop = scr + b->n_y0;
                a.t0 = scr + 2 * b->n_y0;
                a.z = a.t0 + m;
                a.trace = nullptr;
                if (b->d_cvec) a.cvec = b->d_cvec + k * (size_t)p->n_cvec;
                a.jt = b->d_jt + k * n * m;
                a.jt_sparse = 1;
                a.jt_state = b->d_state + 2 * k;
                a.jt_launches = a.jt_state + 1;
                a.ready = reinterpret_cast<unsigned*>(fl + OGK_FLAG_TICKET);
                a.nonfinite_result = fl + OGK_FLAG_FUSED_RESULT;
                a.poff = p->d_indptr;
                if (set == 0) {
                    a.nonfinite = fl + OGK_FLAG_FUSED_COUNT;
                    a.nonfinite_next = fl + OGK_FLAG_FUSED_COUNT;
                } else {
                    // an evaluation counts into the first counter, which the bind launch ahead of it zeroes for the lanes
                    // that run; the kernel's own "clear the other counter" goes to a word nobody reads
                    a.nonfinite = fl + OGK_FLAG_COUNT_A;
                    a.nonfinite_next = fl + OGK_FLAG_COUNT_B;
                    a.jt_bump = set - 1;
                }
            }
        e = hipMemcpy(b->d_table, b->table.data(), sizeof(ogk_args) * b->table.size(), hipMemcpyHostToDevice);
    }
    if (e == hipSuccess) e = hipStreamSynchronize(p->stream);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        og_batch_destroy(b);
        return fail(100 + (int)e, std::string("og_batch_create: ") + hipGetErrorString(e) + " (" +
                                      std::to_string(capacity) + " lanes of " +
                                      std::to_string((double)(n * m) * 8.0 / 1048576.0) + " MB each)");
    }
    *out = b;
    return 0;
}

int og_batch_eval_dev(og_batch b, int32_t count, const double* d_X, double* d_F, void* hip_stream) {
    int rc = batch_check(b, count, "og_batch_eval_dev");
    if (rc) return rc;
    if (!d_X || !d_F) return fail(1, "og_batch_eval_dev: null argument");
    hipStream_t s = (hipStream_t)hip_stream;
    rc = batch_bind(b, count, d_X, nullptr, d_F, nullptr, 1, s, "og_batch_eval_dev");
    if (rc) return rc;
    rc = batch_run(b, 1, OGK_BATCH_EVAL, count, s);
    return launched(rc, "og_batch_eval_dev");
}

int og_batch_fd_sweep_dev(og_batch b, int32_t count, const double* d_X, const double* d_H, double* d_F0,
                          double* d_vals, void* hip_stream) {
    int rc = batch_check(b, count, "og_batch_fd_sweep_dev");
    if (rc) return rc;
    if (!d_X || !d_H || !d_F0) return fail(1, "og_batch_fd_sweep_dev: null argument");
    og_problem_s* p = b->p;
    hipStream_t s = (hipStream_t)hip_stream;
    rc = batch_bind(b, count, d_X, d_H, d_F0, d_vals, one_launch(p) ? -1 : 2, s, "og_batch_fd_sweep_dev");
    if (rc) return rc;
    if (one_launch(p)) {
        // ONE launch for all lanes; its arguments are the table and the lane count
        rc = batch_run(b, 0, OGK_BATCH_FUSED, count, s);
    } else {
        // the validation forms (OGPSX_SWEEP=split | dense, or a module whose one-launch form does not fit): one batched
        // evaluation, then the handle's own sweep kernel lane by lane
        rc = batch_run(b, 2, OGK_BATCH_EVAL, count, s);
        if (!rc) rc = batch_lanes_run(b, count, columns_mode(p), d_X, d_H, d_F0, d_vals, s);
    }
    return launched(rc, "og_batch_fd_sweep_dev");
}

int og_batch_lane_dev(og_batch b, int32_t lane, double** d_JT, int32_t* nonfinite_rows) {
    if (!b) return fail(1, "og_batch_lane_dev: null batch");
    if (!live_batch(b)) return fail(1, "og_batch_lane_dev: the batch or its handle has been destroyed");
    if (lane < 0 || lane >= b->capacity) return fail(1, "og_batch_lane_dev: lane out of range");
    if (d_JT) *d_JT = b->d_jt + (size_t)lane * (size_t)b->p->n * (size_t)b->p->m;
    if (nonfinite_rows) {
        // stream-ordered after the batch's most recent launch: waits for that stream, not for the whole device
        OG_HIP(hipSetDevice(b->p->device));
        OG_HIP(hipMemcpyAsync(b->h_flags, b->d_flags + OGK_FLAG_WORDS * (size_t)lane + b->nf_word[(size_t)lane], sizeof(int),
                              hipMemcpyDeviceToHost, b->last_stream));
        OG_HIP(hipStreamSynchronize(b->last_stream));
        *nonfinite_rows = b->h_flags[0];
    }
    return 0;
}

int og_batch_eval(og_batch b, int32_t count, const double* X, double* F) {
    int rc = batch_check(b, count, "og_batch_eval");
    if (rc) return rc;
    if (!X || !F) return fail(1, "og_batch_eval: null argument");
    og_problem_s* p = b->p;
    OG_HIP(hipSetDevice(p->device));
    const size_t m = (size_t)p->m, c = (size_t)count;
    rc = batch_upload(b, c, X, nullptr);
    if (!rc) rc = og_batch_eval_dev(b, count, b->d_xh, b->d_f, p->stream);
    if (rc) return rc;
    OG_HIP(hipMemcpyAsync(b->h_down, b->d_f, sizeof(double) * c * m, hipMemcpyDeviceToHost, p->stream));
    OG_HIP(hipStreamSynchronize(p->stream));
    memcpy(F, b->h_down, sizeof(double) * c * m);
    return 0;
}

int og_batch_fd_sweep(og_batch b, int32_t count, const double* X, const double* H, double* F0, double* vals,
                      int32_t* nonfinite) {
    int rc = batch_check(b, count, "og_batch_fd_sweep");
    if (rc) return rc;
    if (!X || !H || !F0 || !vals) return fail(1, "og_batch_fd_sweep: null argument");
    og_problem_s* p = b->p;
    OG_HIP(hipSetDevice(p->device));
    double *d_f, *d_vals;
    const bool in_place = batch_targets(b, F0, vals, &d_f, &d_vals);
    rc = batch_upload(b, (size_t)count, X, H);
    if (!rc) rc = og_batch_fd_sweep_dev(b, count, b->d_xh, b->d_xh + (size_t)b->capacity * (size_t)p->n, d_f, d_vals, p->stream);
    if (rc) return rc;
    return batch_results(b, (size_t)count, in_place, F0, vals, nonfinite);
}

// ---- run-time parameters (include/ogpsx.h) ----
int og_parameter_count(og_handle p) { return p ? p->n_par : 0; }

// every lane of batch b takes shared[0 .. n_par) (device), on stream s
static int batch_lanes_take(og_batch_s* b, const double* shared, hipStream_t s) {
    const og_problem_s* p = b->p;
    const long total = (long)b->capacity * p->n_par;
    hipLaunchKernelGGL(og_par_lanes_kernel, dim3((unsigned)((total + 63) / 64)), dim3(64), 0, s, b->d_cvec, (long)p->n_cvec,
                       p->par_off, p->n_par, b->capacity, (const double*)nullptr, shared);
    OG_HIP(hipGetLastError());
    b->last_stream = s;
    return 0;
}

int og_set_parameters_dev(og_handle p, const double* d_theta, void* hip_stream) {
    if (!p) return fail(1, "og_set_parameters_dev: null handle");
    if (p->n_par == 0) return d_theta ? fail((int)hipErrorInvalidValue, "og_set_parameters_dev: the module has no parameters") : 0;
    if (!d_theta) return fail(1, "og_set_parameters_dev: null argument");
    hipStream_t s = (hipStream_t)hip_stream;
    hipLaunchKernelGGL(og_par_set_kernel, dim3((unsigned)((p->n_par + 63) / 64)), dim3(64), 0, s, p->d_cvec + p->par_off,
                       d_theta, p->n_par);
    OG_HIP(hipGetLastError());
    // a handle-level set reaches everything: every lane of every batch of the handle, from the table just written
    for (og_batch_s* b : p->batches) {
        const int rc = batch_lanes_take(b, p->d_cvec + p->par_off, s);
        if (rc) return rc;
    }
    return 0;
}

static int parameter_count_check(const og_problem_s* p, int32_t count, const char* who) {
    if (count == p->n_par) return 0;
    return fail((int)hipErrorInvalidValue, std::string(who) + ": count " + std::to_string(count) + ", the module has " +
                                               std::to_string(p->n_par) + " parameters");
}

int og_set_parameters(og_handle p, const double* theta, int32_t count) {
    if (!p) return fail(1, "og_set_parameters: null handle");
    int rc = parameter_count_check(p, count, "og_set_parameters");
    if (rc || count == 0) return rc;
    if (!theta) return fail(1, "og_set_parameters: null argument");
    OG_HIP(hipSetDevice(p->device));
    OG_HIP(hipDeviceSynchronize());             // after everything the handle was asked for, on whatever stream
    OG_HIP(hipMemcpy(p->d_theta, theta, sizeof(double) * (size_t)count, hipMemcpyHostToDevice));
    rc = og_set_parameters_dev(p, p->d_theta, p->stream);
    if (rc) return rc;
    OG_HIP(hipStreamSynchronize(p->stream));
    return 0;
}

int og_get_parameters(og_handle p, double* theta, int32_t count) {
    if (!p) return fail(1, "og_get_parameters: null handle");
    const int rc = parameter_count_check(p, count, "og_get_parameters");
    if (rc || count == 0) return rc;
    if (!theta) return fail(1, "og_get_parameters: null argument");
    OG_HIP(hipSetDevice(p->device));
    OG_HIP(hipDeviceSynchronize());
    OG_HIP(hipMemcpy(theta, p->d_cvec + p->par_off, sizeof(double) * (size_t)count, hipMemcpyDeviceToHost));
    return 0;
}

int og_parameters_batch_dev(og_batch b, int32_t count, const double* d_TH, void* hip_stream) {
    int rc = batch_check(b, count, "og_parameters_batch_dev");
    if (rc) return rc;
    og_problem_s* p = b->p;
    if (p->n_par == 0)
        return d_TH ? fail((int)hipErrorInvalidValue, "og_parameters_batch_dev: the module has no parameters") : 0;
    hipStream_t s = (hipStream_t)hip_stream;
    if (!d_TH) return batch_lanes_take(b, p->d_cvec + p->par_off, s);
    const long total = (long)count * p->n_par;
    hipLaunchKernelGGL(og_par_lanes_kernel, dim3((unsigned)((total + 63) / 64)), dim3(64), 0, s, b->d_cvec, (long)p->n_cvec,
                       p->par_off, p->n_par, (int)count, d_TH, (const double*)nullptr);
    OG_HIP(hipGetLastError());
    b->last_stream = s;
    return 0;
}

int og_parameters_batch(og_batch b, int32_t count, const double* TH) {
    int rc = batch_check(b, count, "og_parameters_batch");
    if (rc) return rc;
    og_problem_s* p = b->p;
    OG_HIP(hipSetDevice(p->device));
    if (TH && p->n_par > 0) {
        const size_t bytes = sizeof(double) * (size_t)count * (size_t)p->n_par;
        OG_HIP(hipStreamSynchronize(p->stream));        // (the staging buffers are free again)
        memcpy(b->h_th, TH, bytes);
        OG_HIP(hipMemcpyAsync(b->d_th, b->h_th, bytes, hipMemcpyHostToDevice, p->stream));
    }
    rc = og_parameters_batch_dev(b, count, (TH && p->n_par > 0) ? b->d_th : TH, p->stream);
    if (rc) return rc;
    OG_HIP(hipStreamSynchronize(p->stream));
    return 0;
}

// ---- the exact Jacobian of a batch (include/ogpsx.h) ----
int og_jacobian_exact_batch_load(og_batch b, const char* exact_part_path) {
    if (!b) return fail(1, "og_jacobian_exact_batch_load: null batch");
    if (!live_batch(b)) return fail(1, "og_jacobian_exact_batch_load: the batch or its handle has been destroyed");
    og_problem_s* p = b->p;
    if (p->batch_exact_launch) return 0;
    return load_module_part(p, exact_part_path, "og_jacobian_exact_batch_load", "exact batch part", &p->batch_exact_module,
                            &p->batch_exact_launch);
}

int og_jacobian_exact_batch_dev(og_batch b, int32_t count, const double* d_X, double* d_F0, double* d_vals,
                                void* hip_stream) {
    int rc = batch_check(b, count, "og_jacobian_exact_batch_dev");
    if (rc) return rc;
    if (!d_X || !d_F0) return fail(1, "og_jacobian_exact_batch_dev: null argument");
    og_problem_s* p = b->p;
    const bool dense = p->exact_mode == OGK_EXACT_DENSE;
    if (!dense && !p->batch_exact_launch)
        return fail(4, "og_jacobian_exact_batch_dev: the module's exact batch part is not loaded "
                       "(og_jacobian_exact_batch_load)");
    hipStream_t s = (hipStream_t)hip_stream;
    // record set 2: the evaluation counts one launch into every lane's *jt_launches, as the evaluation of
    // og_jacobian_exact_dev does for a registered buffer
    rc = batch_bind(b, count, d_X, nullptr, d_F0, d_vals, 2, s, "og_jacobian_exact_batch_dev");
    if (rc) return rc;
    rc = batch_run(b, 2, OGK_BATCH_EVAL, count, s);     // F(X[k]) and the base collocation products of every lane
    // every lane's derivatives and packed values; or the validation form (OGPSX_SWEEP=dense): the handle's dense exact
    // kernel and the pack, lane by lane
    if (!rc) rc = dense ? batch_lanes_run(b, count, OGK_EXACT_DENSE, d_X, nullptr, d_F0, d_vals, s)
                        : batch_run(b, 2, OGK_BATCH_EXACT, count, s);
    return launched(rc, "og_jacobian_exact_batch_dev");
}

int og_jacobian_exact_batch(og_batch b, int32_t count, const double* X, double* F0, double* vals,
                            int32_t* nonfinite) {
    int rc = batch_check(b, count, "og_jacobian_exact_batch");
    if (rc) return rc;
    if (!X || !F0 || !vals) return fail(1, "og_jacobian_exact_batch: null argument");
    og_problem_s* p = b->p;
    OG_HIP(hipSetDevice(p->device));
    // F0 and vals in memory the device can address are written in place, as og_batch_fd_sweep does
    double *d_f, *d_vals;
    const bool in_place = batch_targets(b, F0, vals, &d_f, &d_vals);
    rc = batch_upload(b, (size_t)count, X, nullptr);
    if (!rc) rc = og_jacobian_exact_batch_dev(b, count, b->d_xh, d_f, d_vals, p->stream);
    if (rc) return rc;
    return batch_results(b, (size_t)count, in_place, F0, vals, nonfinite);
}

// ---- exact dF/dtheta for the run-time parameters (include/ogpsx.h) ----
static int parameter_jacobian_check(const og_problem_s* p, const char* who) {
    if (p->n_par == 0) return fail(1, std::string(who) + ": the module has no run-time parameters");
    if (!p->par_launch)
        return fail(4, std::string(who) + ": the module's parameter part is not loaded (og_parameter_jacobian_load)");
    return 0;
}

int og_parameter_jacobian_load(og_handle p, const char* par_part_path) {
    if (!p) return fail(1, "og_parameter_jacobian_load: null handle");
    if (p->n_par == 0) return fail(1, "og_parameter_jacobian_load: the module has no run-time parameters");
    if (p->par_launch) return 0;
    OG_HIP(hipSetDevice(p->device));
    void* mod = nullptr;
    ogk_launch_batch_fn batch_fn = nullptr;
    int rc = load_module_part(p, par_part_path, "og_parameter_jacobian_load", "parameter part", &mod, &batch_fn);
    if (rc) return rc;
    ogk_launch_fn fn = (ogk_launch_fn)dlsym(mod, "ogk_launch");
    ogk_args probe;
    memset(&probe, 0, sizeof probe);
    // (another part of the same module passes the checks above: only the parameter part knows the mode)
    if (!fn || fn(&probe, OGK_PAR_JAC, nullptr) != (int)hipErrorInvalidValue) {
        dlclose(mod);
        return fail(5, "og_parameter_jacobian_load: the parameter part does not belong to the handle's module");
    }
    p->par_module = mod;
    p->par_launch = fn;
    p->par_launch_batch = batch_fn;
    return 0;
}

int og_parameter_jacobian_dev(og_handle p, const double* d_x, double* d_dF, double* d_F0, void* hip_stream) {
    if (!p || !d_x || !d_dF) return fail(1, "og_parameter_jacobian_dev: null argument");
    int rc = parameter_jacobian_check(p, "og_parameter_jacobian_dev");
    if (rc) return rc;
    ogk_args a;
    p->flag_slot ^= 1;
    // (no J_T among the arguments: the evaluation counts no launch into any buffer's words, and nothing here reads them)
    fill_args(p, &a, d_x, nullptr, d_F0 ? d_F0 : p->d_f0, nullptr, 0, 0);
    p->nf_read = a.nonfinite;
    rc = clear_count_in_a_capture(a.nonfinite, hip_stream);
    if (rc) return rc;
    rc = p->launch(&a, OGK_EVAL, hip_stream);       // F(x0) and the base collocation products
    a.jt = d_dF;
    if (!rc) rc = p->par_launch(&a, OGK_PAR_JAC, hip_stream);
    return launched(rc, "og_parameter_jacobian_dev");
}

int og_parameter_jacobian(og_handle p, const double* x, double* dF, double* F0) {
    if (!p || !x || !dF) return fail(1, "og_parameter_jacobian: null argument");
    int rc = parameter_jacobian_check(p, "og_parameter_jacobian");
    if (rc) return rc;
    OG_HIP(hipSetDevice(p->device));
    const size_t count = (size_t)p->n_par * (size_t)p->m;
    if (!p->d_pj) OG_HIP(hipMalloc(&p->d_pj, sizeof(double) * count));
    rc = upload_point(p, x, nullptr);
    if (rc) return rc;
    rc = og_parameter_jacobian_dev(p, p->d_x, p->d_pj, p->d_f0, p->stream);
    if (rc) return rc;
    OG_HIP(hipMemcpyAsync(dF, p->d_pj, sizeof(double) * count, hipMemcpyDeviceToHost, p->stream));
    if (F0) OG_HIP(hipMemcpyAsync(F0, p->d_f0, sizeof(double) * (size_t)p->m, hipMemcpyDeviceToHost, p->stream));
    OG_HIP(hipStreamSynchronize(p->stream));
    return 0;
}

int og_parameter_jacobian_batch_dev(og_batch b, int32_t count, const double* d_X, double* d_F0, double* d_dF,
                                    void* hip_stream) {
    int rc = batch_check(b, count, "og_parameter_jacobian_batch_dev");
    if (rc) return rc;
    if (!d_X || !d_dF) return fail(1, "og_parameter_jacobian_batch_dev: null argument");
    og_problem_s* p = b->p;
    rc = parameter_jacobian_check(p, "og_parameter_jacobian_batch_dev");
    if (rc) return rc;
    hipStream_t s = (hipStream_t)hip_stream;
    // record set 1: its evaluation counts no launch into a lane's *jt_launches - this call writes no J_T; the lanes'
    // pvals are bound to the slices of d_dF
    rc = batch_bind(b, count, d_X, nullptr, d_F0 ? d_F0 : b->d_f, d_dF, 1, s, "og_parameter_jacobian_batch_dev",
                    (int64_t)p->n_par * (int64_t)p->m);
    if (rc) return rc;
    rc = batch_run(b, 1, OGK_BATCH_EVAL, count, s);
    if (!rc) {
        const ogk_batch_args ba = batch_args(b, 1, count);
        rc = p->par_launch_batch(&ba, OGK_BATCH_PAR_JAC, s);
    }
    return launched(rc, "og_parameter_jacobian_batch_dev");
}

int og_parameter_jacobian_batch(og_batch b, int32_t count, const double* X, double* F0, double* dF) {
    int rc = batch_check(b, count, "og_parameter_jacobian_batch");
    if (rc) return rc;
    if (!X || !dF) return fail(1, "og_parameter_jacobian_batch: null argument");
    og_problem_s* p = b->p;
    rc = parameter_jacobian_check(p, "og_parameter_jacobian_batch");
    if (rc) return rc;
    OG_HIP(hipSetDevice(p->device));
    const size_t lane = (size_t)p->n_par * (size_t)p->m, c = (size_t)count;
    if (!b->d_pj) OG_HIP(hipMalloc(&b->d_pj, sizeof(double) * (size_t)b->capacity * lane));
    rc = batch_upload(b, c, X, nullptr);
    if (!rc) rc = og_parameter_jacobian_batch_dev(b, count, b->d_xh, b->d_f, b->d_pj, p->stream);
    if (rc) return rc;
    OG_HIP(hipMemcpyAsync(dF, b->d_pj, sizeof(double) * c * lane, hipMemcpyDeviceToHost, p->stream));
    if (F0) OG_HIP(hipMemcpyAsync(F0, b->d_f, sizeof(double) * c * (size_t)p->m, hipMemcpyDeviceToHost, p->stream));
    OG_HIP(hipStreamSynchronize(p->stream));
    return 0;
}

// ---- exact directional derivatives F'(x) v (include/ogpsx.h) ----
static const int OG_MAX_DIRECTIONS = 65535;         // (one launch: the direction is a grid dimension)

static int directional_check(const og_problem_s* p, const char* who) {
    if (!p->dir_launch)
        return fail(4, std::string(who) + ": the module's directional part is not loaded (og_directional_load)");
    return 0;
}

static int directional_count_check(int32_t k, const char* who) {
    if (k < 1) return fail(1, std::string(who) + ": k must be at least 1");
    if (k > OG_MAX_DIRECTIONS)
        return fail(1, std::string(who) + ": k " + std::to_string(k) + " exceeds " + std::to_string(OG_MAX_DIRECTIONS) +
                           " directions of one call");
    return 0;
}

int og_directional_load(og_handle p, const char* dir_part_path) {
    if (!p) return fail(1, "og_directional_load: null handle");
    if (p->dir_launch) return 0;
    OG_HIP(hipSetDevice(p->device));
    void* mod = nullptr;
    ogk_launch_batch_fn batch_fn = nullptr;
    int rc = load_module_part(p, dir_part_path, "og_directional_load", "directional part", &mod, &batch_fn);
    if (rc) return rc;
    ogk_launch_fn fn = (ogk_launch_fn)dlsym(mod, "ogk_launch");
    ogk_args probe;
    memset(&probe, 0, sizeof probe);
    // (another part of the same module passes the checks above: only the directional part knows the mode)
    if (!fn || fn(&probe, OGK_DIR, nullptr) != (int)hipErrorInvalidValue) {
        dlclose(mod);
        return fail(5, "og_directional_load: the directional part does not belong to the handle's module");
    }
    p->dir_module = mod;
    p->dir_launch = fn;
    p->dir_launch_batch = batch_fn;
    return 0;
}

int og_directional_dev(og_handle p, const double* d_x, int32_t k, const double* d_V, double* d_dF, double* d_F0,
                       void* hip_stream) {
    if (!p || !d_x || !d_V || !d_dF) return fail(1, "og_directional_dev: null argument");
    int rc = directional_check(p, "og_directional_dev");
    if (!rc) rc = directional_count_check(k, "og_directional_dev");
    if (rc) return rc;
    ogk_args a;
    p->flag_slot ^= 1;
    // (no J_T among the arguments: the evaluation counts no launch into any buffer's words, and nothing here reads them;
    // the directions travel in the step pointer, which the evaluation does not read, and their number as a column range)
    fill_args(p, &a, d_x, d_V, d_F0 ? d_F0 : p->d_f0, nullptr, 0, k);
    p->nf_read = a.nonfinite;
    rc = clear_count_in_a_capture(a.nonfinite, hip_stream);
    if (rc) return rc;
    rc = p->launch(&a, OGK_EVAL, hip_stream);       // F(x0) and the base collocation products
    a.jt = d_dF;
    if (!rc) rc = p->dir_launch(&a, OGK_DIR, hip_stream);
    return launched(rc, "og_directional_dev");
}

int og_directional(og_handle p, const double* x, int32_t k, const double* V, double* dF, double* F0) {
    if (!p || !x || !V || !dF) return fail(1, "og_directional: null argument");
    int rc = directional_check(p, "og_directional");
    if (!rc) rc = directional_count_check(k, "og_directional");
    if (rc) return rc;
    OG_HIP(hipSetDevice(p->device));
    const size_t n = (size_t)p->n, m = (size_t)p->m, kk = (size_t)k;
    if (kk > p->dir_capacity) {
        if (p->d_dir) OG_HIP(hipFree(p->d_dir));
        p->d_dir = nullptr;
        p->dir_capacity = 0;
        OG_HIP(hipMalloc(&p->d_dir, sizeof(double) * kk * (n + m)));
        p->dir_capacity = kk;
    }
    double *d_V = p->d_dir, *d_dF = p->d_dir + kk * n;
    rc = upload_point(p, x, nullptr);
    if (rc) return rc;
    OG_HIP(hipMemcpyAsync(d_V, V, sizeof(double) * kk * n, hipMemcpyHostToDevice, p->stream));
    rc = og_directional_dev(p, p->d_x, k, d_V, d_dF, p->d_f0, p->stream);
    if (rc) return rc;
    OG_HIP(hipMemcpyAsync(dF, d_dF, sizeof(double) * kk * m, hipMemcpyDeviceToHost, p->stream));
    if (F0) OG_HIP(hipMemcpyAsync(F0, p->d_f0, sizeof(double) * m, hipMemcpyDeviceToHost, p->stream));
    OG_HIP(hipStreamSynchronize(p->stream));
    return 0;
}

int og_directional_batch_dev(og_batch b, int32_t count, const double* d_X, const double* d_V, double* d_F0, double* d_dF,
                             void* hip_stream) {
    int rc = batch_check(b, count, "og_directional_batch_dev");
    if (rc) return rc;
    if (!d_X || !d_V || !d_dF) return fail(1, "og_directional_batch_dev: null argument");
    og_problem_s* p = b->p;
    rc = directional_check(p, "og_directional_batch_dev");
    if (!rc) rc = directional_count_check(count, "og_directional_batch_dev");
    if (rc) return rc;
    hipStream_t s = (hipStream_t)hip_stream;
    // record set 1: its evaluation counts no launch into a lane's *jt_launches - this call writes no J_T; the lanes' h
    // is bound to the rows of d_V and their pvals to the rows of d_dF
    rc = batch_bind(b, count, d_X, d_V, d_F0 ? d_F0 : b->d_f, d_dF, 1, s, "og_directional_batch_dev", (int64_t)p->m);
    if (rc) return rc;
    rc = batch_run(b, 1, OGK_BATCH_EVAL, count, s);
    if (!rc) {
        const ogk_batch_args ba = batch_args(b, 1, count);
        rc = p->dir_launch_batch(&ba, OGK_BATCH_DIR, s);
    }
    return launched(rc, "og_directional_batch_dev");
}

int og_directional_batch(og_batch b, int32_t count, const double* X, const double* V, double* F0, double* dF) {
    int rc = batch_check(b, count, "og_directional_batch");
    if (rc) return rc;
    if (!X || !V || !dF) return fail(1, "og_directional_batch: null argument");
    og_problem_s* p = b->p;
    rc = directional_check(p, "og_directional_batch");
    if (rc) return rc;
    OG_HIP(hipSetDevice(p->device));
    const size_t m = (size_t)p->m, c = (size_t)count;
    if (!b->d_dj) OG_HIP(hipMalloc(&b->d_dj, sizeof(double) * (size_t)b->capacity * m));
    rc = batch_upload(b, c, X, V);                  // (V where a sweep's steps go: [capacity][n] behind X)
    if (!rc) rc = og_directional_batch_dev(b, count, b->d_xh, b->d_xh + (size_t)b->capacity * (size_t)p->n, b->d_f, b->d_dj,
                                           p->stream);
    if (rc) return rc;
    OG_HIP(hipMemcpyAsync(dF, b->d_dj, sizeof(double) * c * m, hipMemcpyDeviceToHost, p->stream));
    if (F0) OG_HIP(hipMemcpyAsync(F0, b->d_f, sizeof(double) * c * m, hipMemcpyDeviceToHost, p->stream));
    OG_HIP(hipStreamSynchronize(p->stream));
    return 0;
}

// ---- exact adjoint products F'(x)^T w (include/ogpsx.h) ----
static const int OG_MAX_WEIGHT_VECTORS = 65535;     // (one launch; the lanes of a batch are a grid dimension)

static int adjoint_check(const og_problem_s* p, const char* who) {
    if (!p->adj_launch) return fail(4, std::string(who) + ": the module's adjoint part is not loaded (og_adjoint_load)");
    return 0;
}

static int adjoint_count_check(int32_t k, const char* who) {
    if (k < 1) return fail(1, std::string(who) + ": k must be at least 1");
    if (k > OG_MAX_WEIGHT_VECTORS)
        return fail(1, std::string(who) + ": k " + std::to_string(k) + " exceeds " + std::to_string(OG_MAX_WEIGHT_VECTORS) +
                           " weight vectors of one call");
    return 0;
}

int og_adjoint_load(og_handle p, const char* adj_part_path) {
    if (!p) return fail(1, "og_adjoint_load: null handle");
    if (p->adj_launch) return 0;
    OG_HIP(hipSetDevice(p->device));
    void* mod = nullptr;
    ogk_launch_batch_fn batch_fn = nullptr;
    int rc = load_module_part(p, adj_part_path, "og_adjoint_load", "adjoint part", &mod, &batch_fn);
    if (rc) return rc;
    ogk_launch_fn fn = (ogk_launch_fn)dlsym(mod, "ogk_launch");
    ogk_args probe;
    memset(&probe, 0, sizeof probe);
    // (another part of the same module passes the checks above: only the adjoint part knows the mode)
    if (!fn || fn(&probe, OGK_ADJ, nullptr) != (int)hipErrorInvalidValue) {
        dlclose(mod);
        return fail(5, "og_adjoint_load: the adjoint part does not belong to the handle's module");
    }
    p->adj_module = mod;
    p->adj_launch = fn;
    p->adj_launch_batch = batch_fn;
    return 0;
}

int og_adjoint_dev(og_handle p, const double* d_x, int32_t k, const double* d_W, double* d_G, double* d_F0,
                   void* hip_stream) {
    if (!p || !d_x || !d_W || !d_G) return fail(1, "og_adjoint_dev: null argument");
    int rc = adjoint_check(p, "og_adjoint_dev");
    if (!rc) rc = adjoint_count_check(k, "og_adjoint_dev");
    if (rc) return rc;
    ogk_args a;
    p->flag_slot ^= 1;
    // (no J_T among the arguments: the evaluation counts no launch into any buffer's words, and nothing here reads them;
    // the weight vectors travel in the step pointer, which the evaluation does not read, and their number as a column
    // range)
    fill_args(p, &a, d_x, d_W, d_F0 ? d_F0 : p->d_f0, nullptr, 0, k);
    p->nf_read = a.nonfinite;
    rc = clear_count_in_a_capture(a.nonfinite, hip_stream);
    if (rc) return rc;
    rc = p->launch(&a, OGK_EVAL, hip_stream);       // F(x0) and the base collocation products
    a.jt = d_G;
    if (!rc) rc = p->adj_launch(&a, OGK_ADJ, hip_stream);
    return launched(rc, "og_adjoint_dev");
}

int og_adjoint(og_handle p, const double* x, int32_t k, const double* W, double* G, double* F0) {
    if (!p || !x || !W || !G) return fail(1, "og_adjoint: null argument");
    int rc = adjoint_check(p, "og_adjoint");
    if (!rc) rc = adjoint_count_check(k, "og_adjoint");
    if (rc) return rc;
    OG_HIP(hipSetDevice(p->device));
    const size_t n = (size_t)p->n, m = (size_t)p->m, kk = (size_t)k;
    if (kk > p->adj_capacity) {
        if (p->d_adj) OG_HIP(hipFree(p->d_adj));
        p->d_adj = nullptr;
        p->adj_capacity = 0;
        OG_HIP(hipMalloc(&p->d_adj, sizeof(double) * kk * (n + m)));
        p->adj_capacity = kk;
    }
    double *d_W = p->d_adj, *d_G = p->d_adj + kk * m;
    rc = upload_point(p, x, nullptr);
    if (rc) return rc;
    OG_HIP(hipMemcpyAsync(d_W, W, sizeof(double) * kk * m, hipMemcpyHostToDevice, p->stream));
    rc = og_adjoint_dev(p, p->d_x, k, d_W, d_G, p->d_f0, p->stream);
    if (rc) return rc;
    OG_HIP(hipMemcpyAsync(G, d_G, sizeof(double) * kk * n, hipMemcpyDeviceToHost, p->stream));
    if (F0) OG_HIP(hipMemcpyAsync(F0, p->d_f0, sizeof(double) * m, hipMemcpyDeviceToHost, p->stream));
    OG_HIP(hipStreamSynchronize(p->stream));
    return 0;
}

int og_adjoint_batch_dev(og_batch b, int32_t count, const double* d_X, const double* d_W, double* d_F0, double* d_G,
                         void* hip_stream) {
    int rc = batch_check(b, count, "og_adjoint_batch_dev");
    if (rc) return rc;
    if (!d_X || !d_W || !d_G) return fail(1, "og_adjoint_batch_dev: null argument");
    og_problem_s* p = b->p;
    rc = adjoint_check(p, "og_adjoint_batch_dev");
    if (!rc) rc = adjoint_count_check(count, "og_adjoint_batch_dev");
    if (rc) return rc;
    hipStream_t s = (hipStream_t)hip_stream;
    // record set 1: its evaluation counts no launch into a lane's *jt_launches - this call writes no J_T.  The records
    // learn X and F0 only: a record's h has the stride of a decision vector, so the weight vectors [count][m] and the
    // result [count][n] are arguments of the adjoint launch itself
    rc = batch_bind(b, count, d_X, nullptr, d_F0 ? d_F0 : b->d_f, nullptr, 1, s, "og_adjoint_batch_dev");
    if (rc) return rc;
    rc = batch_run(b, 1, OGK_BATCH_EVAL, count, s);
    if (!rc) {
        ogk_batch_args ba = batch_args(b, 1, count);
        ba.H = d_W, ba.vals = d_G, ba.nnz = (int64_t)p->n;
        rc = p->adj_launch_batch(&ba, OGK_BATCH_ADJ, s);
    }
    return launched(rc, "og_adjoint_batch_dev");
}

int og_adjoint_batch(og_batch b, int32_t count, const double* X, const double* W, double* F0, double* G) {
    int rc = batch_check(b, count, "og_adjoint_batch");
    if (rc) return rc;
    if (!X || !W || !G) return fail(1, "og_adjoint_batch: null argument");
    og_problem_s* p = b->p;
    rc = adjoint_check(p, "og_adjoint_batch");
    if (rc) return rc;
    OG_HIP(hipSetDevice(p->device));
    const size_t n = (size_t)p->n, m = (size_t)p->m, c = (size_t)count, cap = (size_t)b->capacity;
    if (!b->d_aj) OG_HIP(hipMalloc(&b->d_aj, sizeof(double) * cap * (m + n)));
    double *d_W = b->d_aj, *d_G = b->d_aj + cap * m;
    rc = batch_upload(b, c, X, nullptr);
    if (rc) return rc;
    OG_HIP(hipMemcpyAsync(d_W, W, sizeof(double) * c * m, hipMemcpyHostToDevice, p->stream));
    rc = og_adjoint_batch_dev(b, count, b->d_xh, d_W, b->d_f, d_G, p->stream);
    if (rc) return rc;
    OG_HIP(hipMemcpyAsync(G, d_G, sizeof(double) * c * n, hipMemcpyDeviceToHost, p->stream));
    if (F0) OG_HIP(hipMemcpyAsync(F0, b->d_f, sizeof(double) * c * m, hipMemcpyDeviceToHost, p->stream));
    OG_HIP(hipStreamSynchronize(p->stream));
    return 0;
}

// ---- exact Hessian-vector products grad^2 (w . F)(x) v (include/ogpsx.h) ----
static int hessian_check(const og_problem_s* p, const char* who) {
    if (!p->hvp_launch)
        return fail(4, std::string(who) + ": the module's Hessian part is not loaded (og_hessian_vector_load)");
    return 0;
}

static int hessian_count_check(int32_t k, const char* who) {
    if (k < 1) return fail(1, std::string(who) + ": k must be at least 1");
    if (k > OG_MAX_WEIGHT_VECTORS)
        return fail(1, std::string(who) + ": k " + std::to_string(k) + " exceeds " + std::to_string(OG_MAX_WEIGHT_VECTORS) +
                           " pairs of one call");
    return 0;
}

int og_hessian_vector_load(og_handle p, const char* hvp_part_path) {
    if (!p) return fail(1, "og_hessian_vector_load: null handle");
    if (p->hvp_launch) return 0;
    OG_HIP(hipSetDevice(p->device));
    void* mod = nullptr;
    ogk_launch_batch_fn batch_fn = nullptr;
    int rc = load_module_part(p, hvp_part_path, "og_hessian_vector_load", "Hessian part", &mod, &batch_fn);
    if (rc) return rc;
    ogk_launch_fn fn = (ogk_launch_fn)dlsym(mod, "ogk_launch");
    ogk_args probe;
    memset(&probe, 0, sizeof probe);
    // (another part of the same module passes the checks above: only the Hessian part knows the mode)
    if (!fn || fn(&probe, OGK_HVP, nullptr) != (int)hipErrorInvalidValue) {
        dlclose(mod);
        return fail(5, "og_hessian_vector_load: the Hessian part does not belong to the handle's module");
    }
    p->hvp_module = mod;
    p->hvp_launch = fn;
    p->hvp_launch_batch = batch_fn;
    return 0;
}

int og_hessian_vector_dev(og_handle p, const double* d_x, int32_t k, const double* d_W, const double* d_V, double* d_Q,
                          double* d_F0, void* hip_stream) {
    if (!p || !d_x || !d_W || !d_V || !d_Q) return fail(1, "og_hessian_vector_dev: null argument");
    int rc = hessian_check(p, "og_hessian_vector_dev");
    if (!rc) rc = hessian_count_check(k, "og_hessian_vector_dev");
    if (rc) return rc;
    ogk_args a;
    p->flag_slot ^= 1;
    // (as og_adjoint_dev: no J_T among the arguments, the weight vectors in the step pointer and the number of pairs as a
    // column range; the directions in the packed-values pointer, which neither launch writes)
    fill_args(p, &a, d_x, d_W, d_F0 ? d_F0 : p->d_f0, nullptr, 0, k);
    p->nf_read = a.nonfinite;
    rc = clear_count_in_a_capture(a.nonfinite, hip_stream);
    if (rc) return rc;
    rc = p->launch(&a, OGK_EVAL, hip_stream);       // F(x0) and the base collocation products
    a.jt = d_Q;
    a.pvals = const_cast<double*>(d_V);
    if (!rc) rc = p->hvp_launch(&a, OGK_HVP, hip_stream);
    return launched(rc, "og_hessian_vector_dev");
}

int og_hessian_vector(og_handle p, const double* x, int32_t k, const double* W, const double* V, double* Q, double* F0) {
    if (!p || !x || !W || !V || !Q) return fail(1, "og_hessian_vector: null argument");
    int rc = hessian_check(p, "og_hessian_vector");
    if (!rc) rc = hessian_count_check(k, "og_hessian_vector");
    if (rc) return rc;
    OG_HIP(hipSetDevice(p->device));
    const size_t n = (size_t)p->n, m = (size_t)p->m, kk = (size_t)k;
    if (kk > p->hvp_capacity) {
        if (p->d_hvp) OG_HIP(hipFree(p->d_hvp));
        p->d_hvp = nullptr;
        p->hvp_capacity = 0;
        OG_HIP(hipMalloc(&p->d_hvp, sizeof(double) * kk * (m + 2 * n)));
        p->hvp_capacity = kk;
    }
    double *d_W = p->d_hvp, *d_V = d_W + kk * m, *d_Q = d_V + kk * n;
    rc = upload_point(p, x, nullptr);
    if (rc) return rc;
    OG_HIP(hipMemcpyAsync(d_W, W, sizeof(double) * kk * m, hipMemcpyHostToDevice, p->stream));
    OG_HIP(hipMemcpyAsync(d_V, V, sizeof(double) * kk * n, hipMemcpyHostToDevice, p->stream));
    rc = og_hessian_vector_dev(p, p->d_x, k, d_W, d_V, d_Q, p->d_f0, p->stream);
    if (rc) return rc;
    OG_HIP(hipMemcpyAsync(Q, d_Q, sizeof(double) * kk * n, hipMemcpyDeviceToHost, p->stream));
    if (F0) OG_HIP(hipMemcpyAsync(F0, p->d_f0, sizeof(double) * m, hipMemcpyDeviceToHost, p->stream));
    OG_HIP(hipStreamSynchronize(p->stream));
    return 0;
}

int og_hessian_vector_batch_dev(og_batch b, int32_t count, const double* d_X, const double* d_W, const double* d_V,
                                double* d_F0, double* d_Q, void* hip_stream) {
    int rc = batch_check(b, count, "og_hessian_vector_batch_dev");
    if (rc) return rc;
    if (!d_X || !d_W || !d_V || !d_Q) return fail(1, "og_hessian_vector_batch_dev: null argument");
    og_problem_s* p = b->p;
    rc = hessian_check(p, "og_hessian_vector_batch_dev");
    if (!rc) rc = hessian_count_check(count, "og_hessian_vector_batch_dev");
    if (rc) return rc;
    hipStream_t s = (hipStream_t)hip_stream;
    // record set 1: its evaluation counts no launch into a lane's *jt_launches - this call writes no J_T.  The records
    // learn X, F0 and - as h, which has the stride of a decision vector - the rows of d_V; the weight vectors
    // [count][m] and the result [count][n] are arguments of the Hessian launch itself
    rc = batch_bind(b, count, d_X, d_V, d_F0 ? d_F0 : b->d_f, nullptr, 1, s, "og_hessian_vector_batch_dev");
    if (rc) return rc;
    rc = batch_run(b, 1, OGK_BATCH_EVAL, count, s);
    if (!rc) {
        ogk_batch_args ba = batch_args(b, 1, count);
        ba.H = d_W, ba.vals = d_Q, ba.nnz = (int64_t)p->n;
        rc = p->hvp_launch_batch(&ba, OGK_BATCH_HVP, s);
    }
    return launched(rc, "og_hessian_vector_batch_dev");
}

int og_hessian_vector_batch(og_batch b, int32_t count, const double* X, const double* W, const double* V, double* F0,
                            double* Q) {
    int rc = batch_check(b, count, "og_hessian_vector_batch");
    if (rc) return rc;
    if (!X || !W || !V || !Q) return fail(1, "og_hessian_vector_batch: null argument");
    og_problem_s* p = b->p;
    rc = hessian_check(p, "og_hessian_vector_batch");
    if (rc) return rc;
    OG_HIP(hipSetDevice(p->device));
    const size_t n = (size_t)p->n, m = (size_t)p->m, c = (size_t)count, cap = (size_t)b->capacity;
    if (!b->d_hj) OG_HIP(hipMalloc(&b->d_hj, sizeof(double) * cap * (m + n)));
    double *d_W = b->d_hj, *d_Q = b->d_hj + cap * m;
    rc = batch_upload(b, c, X, V);                  // (V where a sweep's steps go: [capacity][n] behind X)
    if (rc) return rc;
    OG_HIP(hipMemcpyAsync(d_W, W, sizeof(double) * c * m, hipMemcpyHostToDevice, p->stream));
    rc = og_hessian_vector_batch_dev(b, count, b->d_xh, d_W, b->d_xh + cap * n, b->d_f, d_Q, p->stream);
    if (rc) return rc;
    OG_HIP(hipMemcpyAsync(Q, d_Q, sizeof(double) * c * n, hipMemcpyDeviceToHost, p->stream));
    if (F0) OG_HIP(hipMemcpyAsync(F0, b->d_f, sizeof(double) * c * m, hipMemcpyDeviceToHost, p->stream));
    OG_HIP(hipStreamSynchronize(p->stream));
    return 0;
}

// ---- the exact sparse Hessian of w . F, assembled (include/ogpsx.h) ----
static int hessian_matrix_check(const og_problem_s* p, const char* who) {
    if (!p->hess_launch || p->hess_nnz < 0)
        return fail(4, std::string(who) + ": the module's Hessian-matrix part is not loaded (og_hessian_matrix_load)");
    return 0;
}

// The caller's plan against the term counts of the module's columns -> "" or what is wrong with it
static std::string hessian_plan_fault(int32_t n, int32_t nnz, const int32_t* indptr, const int32_t* cols, const int32_t* owner,
                                      const int32_t* tptr, const int32_t* tlist, const std::vector<int32_t>& terms) {
    if (indptr[0] != 0 || indptr[n] != nnz) return "indptr does not run from 0 to nnz";
    if (tptr[0] != 0) return "tptr does not start at 0";
    for (int32_t j = 0; j < n; ++j)
        if (indptr[j + 1] < indptr[j] || indptr[j + 1] > nnz) return "indptr is not monotone at row " + std::to_string(j);
    for (int32_t q = 0; q < nnz; ++q)               // (before any list is read: every list then ends inside tlist)
        if (tptr[q + 1] < tptr[q]) return "tptr is not monotone at entry " + std::to_string(q);
    for (int32_t j = 0; j < n; ++j)
        for (int32_t q = indptr[j]; q < indptr[j + 1]; ++q) {
            const std::string at = " (entry " + std::to_string(q) + ", row " + std::to_string(j) + ")";
            const int32_t l = cols[q];
            if (l < 0 || l > j) return "a partner outside 0 .. its row" + at;
            if (q > indptr[j] && l <= cols[q - 1]) return "the partners of a row do not ascend" + at;
            if (owner[q] != j && owner[q] != l) return "an owner that is neither variable of its pair" + at;
            for (int32_t i = tptr[q]; i < tptr[q + 1]; ++i) {
                if (tlist[i] < 0 || tlist[i] >= terms[owner[q]]) return "a term the owner's column does not have" + at;
                if (i > tptr[q] && tlist[i] <= tlist[i - 1]) return "a term list that does not ascend" + at;
            }
        }
    return "";
}

int og_hessian_matrix_load(og_handle p, const char* part_path, int32_t nnz, const int32_t* indptr, const int32_t* cols,
                           const int32_t* owner, const int32_t* tptr, const int32_t* tlist) {
    if (!p) return fail(1, "og_hessian_matrix_load: null handle");
    if (p->hess_launch && p->hess_nnz >= 0) return 0;
    if (nnz < 0 || !indptr || !cols || !owner || !tptr || !tlist)
        return fail(1, "og_hessian_matrix_load: null plan array or negative nnz");
    OG_HIP(hipSetDevice(p->device));
    void* mod = nullptr;
    ogk_launch_batch_fn batch_fn = nullptr;
    int rc = load_module_part(p, part_path, "og_hessian_matrix_load", "Hessian-matrix part", &mod, &batch_fn);
    if (rc) return rc;
    ogk_launch_fn fn = (ogk_launch_fn)dlsym(mod, "ogk_launch");
    typedef int (*ogk_hess_terms_fn)(int32_t*);
    ogk_hess_terms_fn terms_fn = (ogk_hess_terms_fn)dlsym(mod, "ogk_hess_terms");
    ogk_args probe;
    memset(&probe, 0, sizeof probe);
    // (another part of the same module passes the checks above: only the Hessian-matrix part knows the mode)
    if (!fn || !terms_fn || fn(&probe, OGK_HESS, nullptr) != (int)hipErrorInvalidValue) {
        dlclose(mod);
        return fail(5, "og_hessian_matrix_load: the Hessian-matrix part does not belong to the handle's module");
    }
    const int32_t n = p->n;
    std::vector<int32_t> terms((size_t)n);
    rc = terms_fn(terms.data());
    if (rc) {
        dlclose(mod);
        return fail(100 + rc, "og_hessian_matrix_load: reading the module's column tables failed");
    }
    const std::string fault = hessian_plan_fault(n, nnz, indptr, cols, owner, tptr, tlist, terms);
    if (!fault.empty()) {
        dlclose(mod);
        return fail(1, "og_hessian_matrix_load: malformed plan: " + fault);
    }
    // the device plan (csrc/ogk.h): light entries grouped by owner - ascending, a stable order - in units of one owner,
    // then the entries a workgroup sums
    const int32_t ntl = tptr[nnz];
    std::vector<int32_t> row_of((size_t)nnz), light, heavy;
    for (int32_t j = 0; j < n; ++j)
        for (int32_t q = indptr[j]; q < indptr[j + 1]; ++q) row_of[q] = j;
    for (int32_t q = 0; q < nnz; ++q) (tptr[q + 1] - tptr[q] <= OGK_HESS_LIGHT_TERMS ? light : heavy).push_back(q);
    std::stable_sort(light.begin(), light.end(), [&](int32_t a, int32_t b) { return owner[a] < owner[b]; });
    std::vector<int32_t> unit;
    for (size_t i = 0; i < light.size(); ++i)
        if (i == 0 || owner[light[i]] != owner[light[i - 1]] || (int32_t)i - unit.back() >= OGK_HESS_UNIT_ENTRIES)
            unit.push_back((int32_t)i);
    const int32_t n_light = (int32_t)light.size(), n_units = (int32_t)unit.size();
    unit.push_back(n_light);
    const size_t off_tptr = OGK_HESS_HEAD + 4 * (size_t)nnz, off_tlist = off_tptr + (size_t)nnz + 1,
                 off_unit = off_tlist + (size_t)ntl, total = off_unit + unit.size();
    if (total > 0x7fffffffu) {
        dlclose(mod);
        return fail(1, "og_hessian_matrix_load: the plan exceeds 2^31 words");
    }
    std::vector<int32_t> plan(total, 0);
    plan[0] = nnz, plan[1] = n_light, plan[2] = n_units;
    plan[3] = (int32_t)off_tptr, plan[4] = (int32_t)off_tlist, plan[5] = (int32_t)off_unit;
    for (int32_t e = 0; e < nnz; ++e) {
        const int32_t q = e < n_light ? light[e] : heavy[e - n_light];
        int32_t* rec = plan.data() + OGK_HESS_HEAD + 4 * (size_t)e;
        rec[0] = owner[q], rec[1] = owner[q] == row_of[q] ? cols[q] : row_of[q], rec[2] = q;
    }
    memcpy(plan.data() + off_tptr, tptr, sizeof(int32_t) * ((size_t)nnz + 1));
    if (ntl > 0) memcpy(plan.data() + off_tlist, tlist, sizeof(int32_t) * (size_t)ntl);
    memcpy(plan.data() + off_unit, unit.data(), sizeof(int32_t) * unit.size());
    int32_t* d_plan = nullptr;
    hipError_t e = hipMalloc(&d_plan, sizeof(int32_t) * total);
    if (e == hipSuccess) e = hipMemcpy(d_plan, plan.data(), sizeof(int32_t) * total, hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        hipFree(d_plan);
        dlclose(mod);
        return fail(100 + (int)e, std::string("og_hessian_matrix_load: ") + hipGetErrorString(e));
    }
    p->hess_module = mod;
    p->hess_launch = fn;
    p->hess_launch_batch = batch_fn;
    p->d_hess_plan = d_plan;
    p->hess_nnz = nnz;
    p->hess_grid = OGK_HESS_WORKGROUPS(nnz, n_light, n_units);
    return 0;
}

int32_t og_hessian_matrix_nnz(og_handle p) { return p && p->hess_launch ? p->hess_nnz : -1; }

int og_hessian_matrix_dev(og_handle p, const double* d_x, int32_t k, const double* d_W, double* d_H, double* d_F0,
                          void* hip_stream) {
    if (!p || !d_x || !d_W || !d_H) return fail(1, "og_hessian_matrix_dev: null argument");
    int rc = hessian_matrix_check(p, "og_hessian_matrix_dev");
    if (!rc) rc = adjoint_count_check(k, "og_hessian_matrix_dev");
    if (rc) return rc;
    ogk_args a;
    p->flag_slot ^= 1;
    // (as og_adjoint_dev: no J_T among the arguments, the weight vectors in the step pointer and their number as a column
    // range; the device plan in the packed-rows pointer and the grid in the unpack range, which neither launch uses)
    fill_args(p, &a, d_x, d_W, d_F0 ? d_F0 : p->d_f0, nullptr, 0, k);
    p->nf_read = a.nonfinite;
    rc = clear_count_in_a_capture(a.nonfinite, hip_stream);
    if (rc) return rc;
    rc = p->launch(&a, OGK_EVAL, hip_stream);       // F(x0) and the base collocation products
    a.jt = d_H;
    a.prow = p->d_hess_plan;
    a.ulo = 0, a.uhi = p->hess_grid;
    if (!rc) rc = p->hess_launch(&a, OGK_HESS, hip_stream);
    return launched(rc, "og_hessian_matrix_dev");
}

int og_hessian_matrix(og_handle p, const double* x, int32_t k, const double* W, double* H, double* F0) {
    if (!p || !x || !W || !H) return fail(1, "og_hessian_matrix: null argument");
    int rc = hessian_matrix_check(p, "og_hessian_matrix");
    if (!rc) rc = adjoint_count_check(k, "og_hessian_matrix");
    if (rc) return rc;
    OG_HIP(hipSetDevice(p->device));
    const size_t m = (size_t)p->m, kk = (size_t)k, nnz = (size_t)p->hess_nnz;
    if (kk > p->hess_capacity) {
        if (p->d_hess) OG_HIP(hipFree(p->d_hess));
        p->d_hess = nullptr;
        p->hess_capacity = 0;
        OG_HIP(hipMalloc(&p->d_hess, sizeof(double) * kk * (m + nnz)));
        p->hess_capacity = kk;
    }
    double *d_W = p->d_hess, *d_H = p->d_hess + kk * m;
    rc = upload_point(p, x, nullptr);
    if (rc) return rc;
    OG_HIP(hipMemcpyAsync(d_W, W, sizeof(double) * kk * m, hipMemcpyHostToDevice, p->stream));
    rc = og_hessian_matrix_dev(p, p->d_x, k, d_W, d_H, p->d_f0, p->stream);
    if (rc) return rc;
    if (nnz) OG_HIP(hipMemcpyAsync(H, d_H, sizeof(double) * kk * nnz, hipMemcpyDeviceToHost, p->stream));
    if (F0) OG_HIP(hipMemcpyAsync(F0, p->d_f0, sizeof(double) * m, hipMemcpyDeviceToHost, p->stream));
    OG_HIP(hipStreamSynchronize(p->stream));
    return 0;
}

int og_hessian_matrix_batch_dev(og_batch b, int32_t count, const double* d_X, const double* d_W, double* d_F0,
                                double* d_H, void* hip_stream) {
    int rc = batch_check(b, count, "og_hessian_matrix_batch_dev");
    if (rc) return rc;
    if (!d_X || !d_W || !d_H) return fail(1, "og_hessian_matrix_batch_dev: null argument");
    og_problem_s* p = b->p;
    rc = hessian_matrix_check(p, "og_hessian_matrix_batch_dev");
    if (!rc) rc = adjoint_count_check(count, "og_hessian_matrix_batch_dev");
    if (rc) return rc;
    hipStream_t s = (hipStream_t)hip_stream;
    // record set 1: its evaluation counts no launch into a lane's *jt_launches - this call writes no J_T.  The records
    // learn X and F0 only; the weight vectors [count][m], the result [count][nnz], the device plan and the grid are
    // arguments of the Hessian-matrix launch itself (csrc/ogk.h: OGK_BATCH_HESS)
    rc = batch_bind(b, count, d_X, nullptr, d_F0 ? d_F0 : b->d_f, nullptr, 1, s, "og_hessian_matrix_batch_dev");
    if (rc) return rc;
    rc = batch_run(b, 1, OGK_BATCH_EVAL, count, s);
    if (!rc) {
        ogk_batch_args ba = batch_args(b, 1, count);
        ba.X = (const double*)p->d_hess_plan;
        ba.H = d_W, ba.vals = d_H, ba.nnz = (int64_t)p->hess_grid;
        rc = p->hess_launch_batch(&ba, OGK_BATCH_HESS, s);
    }
    return launched(rc, "og_hessian_matrix_batch_dev");
}

int og_hessian_matrix_batch(og_batch b, int32_t count, const double* X, const double* W, double* F0, double* H) {
    int rc = batch_check(b, count, "og_hessian_matrix_batch");
    if (rc) return rc;
    if (!X || !W || !H) return fail(1, "og_hessian_matrix_batch: null argument");
    og_problem_s* p = b->p;
    rc = hessian_matrix_check(p, "og_hessian_matrix_batch");
    if (rc) return rc;
    OG_HIP(hipSetDevice(p->device));
    const size_t m = (size_t)p->m, c = (size_t)count, cap = (size_t)b->capacity, nnz = (size_t)p->hess_nnz;
    if (!b->d_hm) OG_HIP(hipMalloc(&b->d_hm, sizeof(double) * cap * (m + nnz)));
    double *d_W = b->d_hm, *d_H = b->d_hm + cap * m;
    rc = batch_upload(b, c, X, nullptr);
    if (rc) return rc;
    OG_HIP(hipMemcpyAsync(d_W, W, sizeof(double) * c * m, hipMemcpyHostToDevice, p->stream));
    rc = og_hessian_matrix_batch_dev(b, count, b->d_xh, d_W, b->d_f, d_H, p->stream);
    if (rc) return rc;
    if (nnz) OG_HIP(hipMemcpyAsync(H, d_H, sizeof(double) * c * nnz, hipMemcpyDeviceToHost, p->stream));
    if (F0) OG_HIP(hipMemcpyAsync(F0, b->d_f, sizeof(double) * c * m, hipMemcpyDeviceToHost, p->stream));
    OG_HIP(hipStreamSynchronize(p->stream));
    return 0;
}

// ---- exact mixed derivatives d(F'(x)^T w)/dtheta_k for the run-time parameters (include/ogpsx.h) ----
static int adjoint_parameter_check(const og_problem_s* p, const char* who) {
    if (p->n_par == 0) return fail(1, std::string(who) + ": the module has no run-time parameters");
    if (!p->mix_launch)
        return fail(4, std::string(who) + ": the module's mixed part is not loaded (og_adjoint_parameter_load)");
    return 0;
}

// (one launch: the pairs of a weight vector and a parameter are a grid dimension, the lanes of a batch another)
static int adjoint_parameter_count_check(const og_problem_s* p, int32_t k, const char* who) {
    if (k < 1) return fail(1, std::string(who) + ": k must be at least 1");
    if ((int64_t)k * (int64_t)p->n_par > OG_MAX_WEIGHT_VECTORS)
        return fail(1, std::string(who) + ": k " + std::to_string(k) + " times " + std::to_string(p->n_par) +
                           " parameters exceeds " + std::to_string(OG_MAX_WEIGHT_VECTORS) + " pairs of one call");
    return 0;
}

int og_adjoint_parameter_load(og_handle p, const char* mix_part_path) {
    if (!p) return fail(1, "og_adjoint_parameter_load: null handle");
    if (p->n_par == 0) return fail(1, "og_adjoint_parameter_load: the module has no run-time parameters");
    if (p->mix_launch) return 0;
    OG_HIP(hipSetDevice(p->device));
    void* mod = nullptr;
    ogk_launch_batch_fn batch_fn = nullptr;
    int rc = load_module_part(p, mix_part_path, "og_adjoint_parameter_load", "mixed part", &mod, &batch_fn);
    if (rc) return rc;
    ogk_launch_fn fn = (ogk_launch_fn)dlsym(mod, "ogk_launch");
    ogk_args probe;
    memset(&probe, 0, sizeof probe);
    // (another part of the same module passes the checks above: only the mixed part knows the mode)
    if (!fn || fn(&probe, OGK_MIX, nullptr) != (int)hipErrorInvalidValue) {
        dlclose(mod);
        return fail(5, "og_adjoint_parameter_load: the mixed part does not belong to the handle's module");
    }
    p->mix_module = mod;
    p->mix_launch = fn;
    p->mix_launch_batch = batch_fn;
    return 0;
}

int og_adjoint_parameter_dev(og_handle p, const double* d_x, int32_t k, const double* d_W, double* d_S, double* d_F0,
                             void* hip_stream) {
    if (!p || !d_x || !d_W || !d_S) return fail(1, "og_adjoint_parameter_dev: null argument");
    int rc = adjoint_parameter_check(p, "og_adjoint_parameter_dev");
    if (!rc) rc = adjoint_parameter_count_check(p, k, "og_adjoint_parameter_dev");
    if (rc) return rc;
    ogk_args a;
    p->flag_slot ^= 1;
    // (as og_adjoint_dev: no J_T among the arguments, the weight vectors in the step pointer and their number as a column
    // range)
    fill_args(p, &a, d_x, d_W, d_F0 ? d_F0 : p->d_f0, nullptr, 0, k);
    p->nf_read = a.nonfinite;
    rc = clear_count_in_a_capture(a.nonfinite, hip_stream);
    if (rc) return rc;
    rc = p->launch(&a, OGK_EVAL, hip_stream);       // F(x0) and the base collocation products
    a.jt = d_S;
    if (!rc) rc = p->mix_launch(&a, OGK_MIX, hip_stream);
    return launched(rc, "og_adjoint_parameter_dev");
}

int og_adjoint_parameter(og_handle p, const double* x, int32_t k, const double* W, double* S, double* F0) {
    if (!p || !x || !W || !S) return fail(1, "og_adjoint_parameter: null argument");
    int rc = adjoint_parameter_check(p, "og_adjoint_parameter");
    if (!rc) rc = adjoint_parameter_count_check(p, k, "og_adjoint_parameter");
    if (rc) return rc;
    OG_HIP(hipSetDevice(p->device));
    const size_t n = (size_t)p->n, m = (size_t)p->m, kk = (size_t)k, out = (size_t)p->n_par * n;
    if (kk > p->mix_capacity) {
        if (p->d_mix) OG_HIP(hipFree(p->d_mix));
        p->d_mix = nullptr;
        p->mix_capacity = 0;
        OG_HIP(hipMalloc(&p->d_mix, sizeof(double) * kk * (m + out)));
        p->mix_capacity = kk;
    }
    double *d_W = p->d_mix, *d_S = d_W + kk * m;
    rc = upload_point(p, x, nullptr);
    if (rc) return rc;
    OG_HIP(hipMemcpyAsync(d_W, W, sizeof(double) * kk * m, hipMemcpyHostToDevice, p->stream));
    rc = og_adjoint_parameter_dev(p, p->d_x, k, d_W, d_S, p->d_f0, p->stream);
    if (rc) return rc;
    OG_HIP(hipMemcpyAsync(S, d_S, sizeof(double) * kk * out, hipMemcpyDeviceToHost, p->stream));
    if (F0) OG_HIP(hipMemcpyAsync(F0, p->d_f0, sizeof(double) * m, hipMemcpyDeviceToHost, p->stream));
    OG_HIP(hipStreamSynchronize(p->stream));
    return 0;
}

int og_adjoint_parameter_batch_dev(og_batch b, int32_t count, const double* d_X, const double* d_W, double* d_F0,
                                   double* d_S, void* hip_stream) {
    int rc = batch_check(b, count, "og_adjoint_parameter_batch_dev");
    if (rc) return rc;
    if (!d_X || !d_W || !d_S) return fail(1, "og_adjoint_parameter_batch_dev: null argument");
    og_problem_s* p = b->p;
    rc = adjoint_parameter_check(p, "og_adjoint_parameter_batch_dev");
    if (!rc && count > OG_MAX_WEIGHT_VECTORS)
        rc = fail(1, "og_adjoint_parameter_batch_dev: count " + std::to_string(count) + " exceeds " +
                         std::to_string(OG_MAX_WEIGHT_VECTORS) + " lanes of one call");
    if (rc) return rc;
    hipStream_t s = (hipStream_t)hip_stream;
    // record set 1: its evaluation counts no launch into a lane's *jt_launches - this call writes no J_T.  The records
    // learn X and F0 only, as in og_adjoint_batch_dev: the weight vectors [count][m] and the result [count][n_par][n]
    // are arguments of the mixed launch itself
    rc = batch_bind(b, count, d_X, nullptr, d_F0 ? d_F0 : b->d_f, nullptr, 1, s, "og_adjoint_parameter_batch_dev");
    if (rc) return rc;
    rc = batch_run(b, 1, OGK_BATCH_EVAL, count, s);
    if (!rc) {
        ogk_batch_args ba = batch_args(b, 1, count);
        ba.H = d_W, ba.vals = d_S, ba.nnz = (int64_t)p->n_par * (int64_t)p->n;
        rc = p->mix_launch_batch(&ba, OGK_BATCH_MIX, s);
    }
    return launched(rc, "og_adjoint_parameter_batch_dev");
}

int og_adjoint_parameter_batch(og_batch b, int32_t count, const double* X, const double* W, double* F0, double* S) {
    int rc = batch_check(b, count, "og_adjoint_parameter_batch");
    if (rc) return rc;
    if (!X || !W || !S) return fail(1, "og_adjoint_parameter_batch: null argument");
    og_problem_s* p = b->p;
    rc = adjoint_parameter_check(p, "og_adjoint_parameter_batch");
    if (rc) return rc;
    OG_HIP(hipSetDevice(p->device));
    const size_t n = (size_t)p->n, m = (size_t)p->m, c = (size_t)count, cap = (size_t)b->capacity;
    const size_t out = (size_t)p->n_par * n;
    if (!b->d_mj) OG_HIP(hipMalloc(&b->d_mj, sizeof(double) * cap * (m + out)));
    double *d_W = b->d_mj, *d_S = b->d_mj + cap * m;
    rc = batch_upload(b, c, X, nullptr);
    if (rc) return rc;
    OG_HIP(hipMemcpyAsync(d_W, W, sizeof(double) * c * m, hipMemcpyHostToDevice, p->stream));
    rc = og_adjoint_parameter_batch_dev(b, count, b->d_xh, d_W, b->d_f, d_S, p->stream);
    if (rc) return rc;
    OG_HIP(hipMemcpyAsync(S, d_S, sizeof(double) * c * out, hipMemcpyDeviceToHost, p->stream));
    if (F0) OG_HIP(hipMemcpyAsync(F0, b->d_f, sizeof(double) * c * m, hipMemcpyDeviceToHost, p->stream));
    OG_HIP(hipStreamSynchronize(p->stream));
    return 0;
}

// ---- exact second derivatives of w . F in the run-time parameters, the theta-theta block (include/ogpsx.h) ----
static int parameter_hessian_check(const og_problem_s* p, const char* who) {
    if (p->n_par == 0) return fail(1, std::string(who) + ": the module has no run-time parameters");
    if (!p->pp_launch)
        return fail(4, std::string(who) + ": the module's parameter-Hessian part is not loaded (og_parameter_hessian_load)");
    return 0;
}

// (one launch: the chunks of weight vectors are a grid dimension, the lanes of a batch another)
static int parameter_hessian_count_check(int32_t kw, const char* who) {
    if (kw < 1) return fail(1, std::string(who) + ": kw must be at least 1");
    if (kw > OG_MAX_WEIGHT_VECTORS)
        return fail(1, std::string(who) + ": kw " + std::to_string(kw) + " exceeds " +
                           std::to_string(OG_MAX_WEIGHT_VECTORS) + " weight vectors of one call");
    return 0;
}

int og_parameter_hessian_load(og_handle p, const char* pp_part_path) {
    if (!p) return fail(1, "og_parameter_hessian_load: null handle");
    if (p->n_par == 0) return fail(1, "og_parameter_hessian_load: the module has no run-time parameters");
    if (p->pp_launch) return 0;
    OG_HIP(hipSetDevice(p->device));
    void* mod = nullptr;
    ogk_launch_batch_fn batch_fn = nullptr;
    int rc = load_module_part(p, pp_part_path, "og_parameter_hessian_load", "parameter-Hessian part", &mod, &batch_fn);
    if (rc) return rc;
    ogk_launch_fn fn = (ogk_launch_fn)dlsym(mod, "ogk_launch");
    ogk_args probe;
    memset(&probe, 0, sizeof probe);
    // (another part of the same module passes the checks above: only the parameter-Hessian part knows the mode)
    if (!fn || fn(&probe, OGK_PP, nullptr) != (int)hipErrorInvalidValue) {
        dlclose(mod);
        return fail(5, "og_parameter_hessian_load: the parameter-Hessian part does not belong to the handle's module");
    }
    p->pp_module = mod;
    p->pp_launch = fn;
    p->pp_launch_batch = batch_fn;
    return 0;
}

int og_parameter_hessian_dev(og_handle p, const double* d_x, int32_t kw, const double* d_W, double* d_S, double* d_F0,
                             void* hip_stream) {
    if (!p || !d_x || !d_W || !d_S) return fail(1, "og_parameter_hessian_dev: null argument");
    int rc = parameter_hessian_check(p, "og_parameter_hessian_dev");
    if (!rc) rc = parameter_hessian_count_check(kw, "og_parameter_hessian_dev");
    if (rc) return rc;
    ogk_args a;
    p->flag_slot ^= 1;
    // (as og_adjoint_parameter_dev: no J_T among the arguments, the weight vectors in the step pointer and their number
    // as a column range)
    fill_args(p, &a, d_x, d_W, d_F0 ? d_F0 : p->d_f0, nullptr, 0, kw);
    p->nf_read = a.nonfinite;
    rc = clear_count_in_a_capture(a.nonfinite, hip_stream);
    if (rc) return rc;
    rc = p->launch(&a, OGK_EVAL, hip_stream);       // F(x0) and the base collocation products
    a.jt = d_S;
    if (!rc) rc = p->pp_launch(&a, OGK_PP, hip_stream);
    return launched(rc, "og_parameter_hessian_dev");
}

int og_parameter_hessian(og_handle p, const double* x, int32_t kw, const double* W, double* S, double* F0) {
    if (!p || !x || !W || !S) return fail(1, "og_parameter_hessian: null argument");
    int rc = parameter_hessian_check(p, "og_parameter_hessian");
    if (!rc) rc = parameter_hessian_count_check(kw, "og_parameter_hessian");
    if (rc) return rc;
    OG_HIP(hipSetDevice(p->device));
    const size_t m = (size_t)p->m, kk = (size_t)kw, out = (size_t)p->n_par * (size_t)p->n_par;
    if (kk > p->pp_capacity) {
        if (p->d_pp) OG_HIP(hipFree(p->d_pp));
        p->d_pp = nullptr;
        p->pp_capacity = 0;
        OG_HIP(hipMalloc(&p->d_pp, sizeof(double) * kk * (m + out)));
        p->pp_capacity = kk;
    }
    double *d_W = p->d_pp, *d_S = d_W + kk * m;
    rc = upload_point(p, x, nullptr);
    if (rc) return rc;
    OG_HIP(hipMemcpyAsync(d_W, W, sizeof(double) * kk * m, hipMemcpyHostToDevice, p->stream));
    rc = og_parameter_hessian_dev(p, p->d_x, kw, d_W, d_S, p->d_f0, p->stream);
    if (rc) return rc;
    OG_HIP(hipMemcpyAsync(S, d_S, sizeof(double) * kk * out, hipMemcpyDeviceToHost, p->stream));
    if (F0) OG_HIP(hipMemcpyAsync(F0, p->d_f0, sizeof(double) * m, hipMemcpyDeviceToHost, p->stream));
    OG_HIP(hipStreamSynchronize(p->stream));
    return 0;
}

int og_parameter_hessian_batch_dev(og_batch b, int32_t count, const double* d_X, const double* d_W, double* d_F0,
                                   double* d_S, void* hip_stream) {
    int rc = batch_check(b, count, "og_parameter_hessian_batch_dev");
    if (rc) return rc;
    if (!d_X || !d_W || !d_S) return fail(1, "og_parameter_hessian_batch_dev: null argument");
    og_problem_s* p = b->p;
    rc = parameter_hessian_check(p, "og_parameter_hessian_batch_dev");
    if (!rc && count > OG_MAX_WEIGHT_VECTORS)
        rc = fail(1, "og_parameter_hessian_batch_dev: count " + std::to_string(count) + " exceeds " +
                         std::to_string(OG_MAX_WEIGHT_VECTORS) + " lanes of one call");
    if (rc) return rc;
    hipStream_t s = (hipStream_t)hip_stream;
    // record set 1, as og_adjoint_parameter_batch_dev: the records learn X and F0 only, the weight vectors [count][m] and
    // the result [count][n_par][n_par] are arguments of the launch itself
    rc = batch_bind(b, count, d_X, nullptr, d_F0 ? d_F0 : b->d_f, nullptr, 1, s, "og_parameter_hessian_batch_dev");
    if (rc) return rc;
    rc = batch_run(b, 1, OGK_BATCH_EVAL, count, s);
    if (!rc) {
        ogk_batch_args ba = batch_args(b, 1, count);
        ba.H = d_W, ba.vals = d_S, ba.nnz = (int64_t)p->n_par * (int64_t)p->n_par;
        rc = p->pp_launch_batch(&ba, OGK_BATCH_PP, s);
    }
    return launched(rc, "og_parameter_hessian_batch_dev");
}

int og_parameter_hessian_batch(og_batch b, int32_t count, const double* X, const double* W, double* F0, double* S) {
    int rc = batch_check(b, count, "og_parameter_hessian_batch");
    if (rc) return rc;
    if (!X || !W || !S) return fail(1, "og_parameter_hessian_batch: null argument");
    og_problem_s* p = b->p;
    rc = parameter_hessian_check(p, "og_parameter_hessian_batch");
    if (rc) return rc;
    OG_HIP(hipSetDevice(p->device));
    const size_t m = (size_t)p->m, c = (size_t)count, cap = (size_t)b->capacity;
    const size_t out = (size_t)p->n_par * (size_t)p->n_par;
    if (!b->d_ppj) OG_HIP(hipMalloc(&b->d_ppj, sizeof(double) * cap * (m + out)));
    double *d_W = b->d_ppj, *d_S = b->d_ppj + cap * m;
    rc = batch_upload(b, c, X, nullptr);
    if (rc) return rc;
    OG_HIP(hipMemcpyAsync(d_W, W, sizeof(double) * c * m, hipMemcpyHostToDevice, p->stream));
    rc = og_parameter_hessian_batch_dev(b, count, b->d_xh, d_W, b->d_f, d_S, p->stream);
    if (rc) return rc;
    OG_HIP(hipMemcpyAsync(S, d_S, sizeof(double) * c * out, hipMemcpyDeviceToHost, p->stream));
    if (F0) OG_HIP(hipMemcpyAsync(F0, b->d_f, sizeof(double) * c * m, hipMemcpyDeviceToHost, p->stream));
    OG_HIP(hipStreamSynchronize(p->stream));
    return 0;
}

}  // extern "C"

// ------------------------------------------------------------------------------------------------
// Column sharding over several devices of one node from ONE process:
// og_comm_init names the devices (and brings up one RCCL communicator per device, ncclCommInitAll, when
// librccl is loadable); an og_multi handle holds one sub-handle, one stream and one full replica of J_T
// per device.  A sweep: every device gets x and h, sweeps ITS block of columns into its replica, packs the
// non-zeros; one grouped ncclAllGather over xGMI (or, OGPSX_GATHER=peer, G-1 hipMemcpyPeerAsync per device)
// exchanges the packed blocks; every device scatters the others' non-zeros into its replica.  The host
// result comes from device 0.
// ------------------------------------------------------------------------------------------------
namespace {

typedef void* ogn_comm;
struct ogn_unique_id { char internal[128]; };      // ncclUniqueId (rccl.h: NCCL_UNIQUE_ID_BYTES)
struct rccl_api {
    void* lib = nullptr;
    int (*CommInitAll)(ogn_comm*, int, const int*) = nullptr;
    int (*GetUniqueId)(ogn_unique_id*) = nullptr;
    int (*CommInitRank)(ogn_comm*, int, ogn_unique_id, int) = nullptr;
    int (*CommDestroy)(ogn_comm) = nullptr;
    int (*AllGather)(const void*, void*, size_t, int, ogn_comm, hipStream_t) = nullptr;
    int (*GroupStart)() = nullptr;
    int (*GroupEnd)() = nullptr;
    const char* (*GetErrorString)(int) = nullptr;
};
const int OGN_FLOAT64 = 8;              // ncclFloat64 (rccl.h)

struct comm_state {
    std::vector<int> devs;
    std::vector<ogn_comm> comms;        // empty: peer copies
    rccl_api api;
} g_comm;

bool load_rccl(rccl_api* api) {
    // a librccl that is already in the process (torch loads its own) wins over the system one
    const char* names[] = {nullptr, "librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"};
    for (const char* nm : names) {
        void* lib = dlopen(nm, RTLD_NOW | RTLD_GLOBAL);
        if (!lib) continue;
        void* sym = dlsym(lib, "ncclCommInitAll");
        if (!sym) continue;
        api->lib = lib;
        api->CommInitAll = (int (*)(ogn_comm*, int, const int*))sym;
        api->GetUniqueId = (int (*)(ogn_unique_id*))dlsym(lib, "ncclGetUniqueId");
        api->CommInitRank = (int (*)(ogn_comm*, int, ogn_unique_id, int))dlsym(lib, "ncclCommInitRank");
        api->CommDestroy = (int (*)(ogn_comm))dlsym(lib, "ncclCommDestroy");
        api->AllGather = (int (*)(const void*, void*, size_t, int, ogn_comm, hipStream_t))dlsym(lib, "ncclAllGather");
        api->GroupStart = (int (*)())dlsym(lib, "ncclGroupStart");
        api->GroupEnd = (int (*)())dlsym(lib, "ncclGroupEnd");
        api->GetErrorString = (const char* (*)(int))dlsym(lib, "ncclGetErrorString");
        return api->CommDestroy && api->AllGather && api->GroupStart && api->GroupEnd;
    }
    return false;
}

}  // namespace

struct og_multi_s {
    int G = 0;
    int n = 0, m = 0, B = 0;
    int64_t block_vals = 0;
    bool rccl = false;
    std::vector<int> devs;              // the handle's own copy of the device list ...
    std::vector<ogn_comm> comms;        // ... and its OWN communicators (ncclCommInitAll at og_multi_create): a later
                                        // og_comm_init, or a second handle on other devices, cannot pull them away
    std::vector<og_problem_s*> sub;
    std::vector<double*> d_full;        // n x m replica per device (rows of the device's block are registered)
    std::vector<double*> d_send, d_recv;
    std::vector<hipEvent_t> packed;     // peer mode: block g's packed values are ready
    std::vector<hipEvent_t> fetched;    // peer mode: device g has copied the other blocks of the previous step
    std::vector<hipEvent_t> uploaded;   // the pinned upload buffer of device g has been read
    bool stepped = false;
};

extern "C" {

// ---- one process per GPU: this rank's own RCCL communicator (the launcher distributes the unique id) ----
int og_shard_comm_unique_id(uint8_t* id128) {
    if (!id128) return fail(1, "og_shard_comm_unique_id: null argument");
    if (!g_comm.api.lib && !load_rccl(&g_comm.api)) return fail(7, "og_shard_comm_unique_id: librccl could not be loaded");
    if (!g_comm.api.GetUniqueId) return fail(7, "og_shard_comm_unique_id: ncclGetUniqueId not found");
    ogn_unique_id id;
    const int rc = g_comm.api.GetUniqueId(&id);
    if (rc != 0) return fail(7, std::string("og_shard_comm_unique_id: ") + (g_comm.api.GetErrorString ? g_comm.api.GetErrorString(rc) : "?"));
    memcpy(id128, id.internal, sizeof id.internal);
    return 0;
}

int og_shard_comm_init(og_handle p, const uint8_t* id128, int32_t rank, int32_t world) {
    if (!p || !id128) return fail(1, "og_shard_comm_init: null argument");
    if (world < 1 || rank < 0 || rank >= world) return fail(1, "og_shard_comm_init: bad rank / world");
    if (!g_comm.api.lib && !load_rccl(&g_comm.api)) return fail(7, "og_shard_comm_init: librccl could not be loaded");
    if (!g_comm.api.CommInitRank) return fail(7, "og_shard_comm_init: ncclCommInitRank not found");
    if (p->shard_world != world) {
        const int rcp = og_shard_plan(p, world, nullptr, nullptr);
        if (rcp) return rcp;
    }
    og_shard_comm_destroy(p);
    OG_HIP(hipSetDevice(p->device));
    ogn_unique_id id;
    memcpy(id.internal, id128, sizeof id.internal);
    ogn_comm comm = nullptr;
    const int rc = g_comm.api.CommInitRank(&comm, world, id, rank);
    if (rc != 0) return fail(7, std::string("og_shard_comm_init: ncclCommInitRank: ") +
                                    (g_comm.api.GetErrorString ? g_comm.api.GetErrorString(rc) : "?"));
    p->shard_comm = comm;
    p->shard_rank = rank;
    return 0;
}

int og_shard_comm_info(og_handle p, int32_t* nranks, int32_t* rank, int32_t* device) {
    if (!p) return fail(1, "og_shard_comm_info: null handle");
    if (!p->shard_comm) return fail(1, "og_shard_comm_info: call og_shard_comm_init first");
    // what RCCL itself says about the communicator (not what the launcher asked for)
    typedef int (*query_fn)(ogn_comm, int*);
    const query_fn count = (query_fn)dlsym(g_comm.api.lib, "ncclCommCount");
    const query_fn user = (query_fn)dlsym(g_comm.api.lib, "ncclCommUserRank");
    const query_fn dev = (query_fn)dlsym(g_comm.api.lib, "ncclCommCuDevice");
    if (!count || !user || !dev) return fail(7, "og_shard_comm_info: ncclCommCount / UserRank / CuDevice not found");
    int v[3] = {-1, -1, -1};
    const int rc = count((ogn_comm)p->shard_comm, &v[0]) | user((ogn_comm)p->shard_comm, &v[1]) |
                   dev((ogn_comm)p->shard_comm, &v[2]);
    if (rc != 0) return fail(7, "og_shard_comm_info: an RCCL query failed");
    if (nranks) *nranks = v[0];
    if (rank) *rank = v[1];
    if (device) *device = v[2];
    return 0;
}

void og_shard_comm_destroy(og_handle p) {
    if (p && p->shard_comm && g_comm.api.CommDestroy) g_comm.api.CommDestroy((ogn_comm)p->shard_comm);
    if (p) p->shard_comm = nullptr;
}

int og_shard_all_gather_dev(og_handle p, const double* d_send, double* d_recv, void* hip_stream) {
    if (!p || !d_send || !d_recv) return fail(1, "og_shard_all_gather_dev: null argument");
    if (!p->shard_comm) return fail(1, "og_shard_all_gather_dev: call og_shard_comm_init first");
    const int rc = g_comm.api.AllGather(d_send, d_recv, (size_t)p->shard_block_vals, OGN_FLOAT64, (ogn_comm)p->shard_comm,
                                        (hipStream_t)hip_stream);
    if (rc != 0) return fail(7, std::string("og_shard_all_gather_dev: ncclAllGather: ") +
                                    (g_comm.api.GetErrorString ? g_comm.api.GetErrorString(rc) : "?"));
    return 0;
}

int og_comm_init(int32_t G, const int32_t* devs) {
    if (G < 1 || !devs) return fail(1, "og_comm_init: need at least one device");
    og_comm_finalize();
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) return fail(3, "og_comm_init: no HIP device available");
    bool distinct = true;
    for (int i = 0; i < G; ++i) {
        if (devs[i] < 0 || devs[i] >= ndev) return fail(3, "og_comm_init: device ordinal out of range");
        for (int k = 0; k < i; ++k) distinct = distinct && devs[k] != devs[i];
    }
    g_comm.devs.assign(devs, devs + G);
    const char* mode = getenv("OGPSX_GATHER");
    const bool want_peer = mode && std::string(mode) == "peer";
    if (!distinct && !want_peer)
        return fail(1, "og_comm_init: a device is listed twice (only allowed with OGPSX_GATHER=peer, for tests)");
    if (!want_peer) {
        if (!load_rccl(&g_comm.api)) {
            if (mode && std::string(mode) == "rccl") return fail(7, "og_comm_init: librccl could not be loaded");
        } else {
            g_comm.comms.assign((size_t)G, nullptr);
            const int rc = g_comm.api.CommInitAll(g_comm.comms.data(), G, g_comm.devs.data());
            if (rc != 0) {
                g_comm.comms.clear();
                return fail(7, std::string("og_comm_init: ncclCommInitAll: ") +
                                   (g_comm.api.GetErrorString ? g_comm.api.GetErrorString(rc) : "?"));
            }
        }
    }
    if (g_comm.comms.empty())            // peer copies: let every pair of distinct devices reach each other
        for (int i = 0; i < G; ++i)
            for (int k = 0; k < G; ++k)
                if (devs[i] != devs[k]) {
                    hipSetDevice(devs[i]);
                    hipDeviceEnablePeerAccess(devs[k], 0);      // "already enabled" is fine
                    (void)hipGetLastError();
                }
    return 0;
}

void og_comm_finalize(void) {
    for (ogn_comm c : g_comm.comms)
        if (c && g_comm.api.CommDestroy) g_comm.api.CommDestroy(c);
    g_comm.comms.clear();
    g_comm.devs.clear();
}

int og_comm_size(void) { return (int)g_comm.devs.size(); }
int og_comm_uses_rccl(void) { return g_comm.comms.empty() ? 0 : 1; }

void og_multi_destroy(og_multi mh) {
    if (!mh) return;
    for (int g = 0; g < (int)mh->sub.size(); ++g) {
        if (!mh->sub[(size_t)g]) continue;
        hipSetDevice(mh->sub[(size_t)g]->device);
        if ((size_t)g < mh->d_full.size()) hipFree(mh->d_full[(size_t)g]);
        if ((size_t)g < mh->d_send.size()) hipFree(mh->d_send[(size_t)g]);
        if ((size_t)g < mh->d_recv.size()) hipFree(mh->d_recv[(size_t)g]);
        if ((size_t)g < mh->packed.size() && mh->packed[(size_t)g]) hipEventDestroy(mh->packed[(size_t)g]);
        if ((size_t)g < mh->fetched.size() && mh->fetched[(size_t)g]) hipEventDestroy(mh->fetched[(size_t)g]);
        if ((size_t)g < mh->uploaded.size() && mh->uploaded[(size_t)g]) hipEventDestroy(mh->uploaded[(size_t)g]);
        og_problem_destroy(mh->sub[(size_t)g]);
    }
    for (ogn_comm c : mh->comms)
        if (c && g_comm.api.CommDestroy) g_comm.api.CommDestroy(c);
    delete mh;
}

int og_multi_create(const og_desc* desc, og_multi* out) {
    if (!desc || !out) return fail(1, "og_multi_create: null argument");
    *out = nullptr;
    const int G = (int)g_comm.devs.size();
    if (G < 1) return fail(1, "og_multi_create: call og_comm_init first");
    og_multi_s* mh = new og_multi_s();
    mh->G = G;
    mh->devs = g_comm.devs;
    mh->rccl = !g_comm.comms.empty();
    if (mh->rccl) {
        // communicators of this handle's own (the ones og_comm_init made stay with the process-wide state)
        mh->comms.assign((size_t)G, nullptr);
        const int rcn = g_comm.api.CommInitAll(mh->comms.data(), G, mh->devs.data());
        if (rcn != 0) {
            mh->comms.clear();
            delete mh;
            return fail(7, std::string("og_multi_create: ncclCommInitAll: ") +
                               (g_comm.api.GetErrorString ? g_comm.api.GetErrorString(rcn) : "?"));
        }
    }
    mh->sub.assign((size_t)G, nullptr);
    mh->fetched.assign((size_t)G, nullptr);
    mh->uploaded.assign((size_t)G, nullptr);
    mh->d_full.assign((size_t)G, nullptr);
    mh->d_send.assign((size_t)G, nullptr);
    mh->d_recv.assign((size_t)G, nullptr);
    mh->packed.assign((size_t)G, nullptr);
    for (int g = 0; g < G; ++g) {
        og_desc d = *desc;
        d.device = mh->devs[(size_t)g];
        int rc = og_problem_create(&d, &mh->sub[(size_t)g]);
        if (rc) {
            og_multi_destroy(mh);
            return rc;
        }
    }
    mh->n = mh->sub[0]->n;
    mh->m = mh->sub[0]->m;
    for (int g = 0; g < G; ++g) {
        og_problem_s* p = mh->sub[(size_t)g];
        int32_t B = 0;
        int64_t bv = 0;
        int rc = og_shard_plan(p, G, &B, &bv);
        if (rc) {
            og_multi_destroy(mh);
            return rc;
        }
        mh->B = B;
        mh->block_vals = bv;
        const size_t full = sizeof(double) * (size_t)mh->n * (size_t)mh->m;
        const size_t blk = sizeof(double) * (size_t)(bv ? bv : 1);
        hipError_t e = hipSetDevice(p->device);
        if (e == hipSuccess) e = hipMalloc(&mh->d_full[(size_t)g], full);
        if (e == hipSuccess) e = hipMemsetAsync(mh->d_full[(size_t)g], 0, full, p->stream);
        if (e == hipSuccess) e = hipMalloc(&mh->d_send[(size_t)g], blk);
        if (e == hipSuccess) e = hipMemsetAsync(mh->d_send[(size_t)g], 0, blk, p->stream);
        if (e == hipSuccess) e = hipMalloc(&mh->d_recv[(size_t)g], blk * (size_t)G);
        if (e == hipSuccess) e = hipEventCreateWithFlags(&mh->packed[(size_t)g], hipEventDisableTiming);
        if (e == hipSuccess) e = hipEventCreateWithFlags(&mh->fetched[(size_t)g], hipEventDisableTiming);
        if (e == hipSuccess) e = hipEventCreateWithFlags(&mh->uploaded[(size_t)g], hipEventDisableTiming);
        if (e != hipSuccess) {
            og_multi_destroy(mh);
            return fail(100 + (int)e, std::string("og_multi_create: ") + hipGetErrorString(e));
        }
        const int lo = std::min(mh->n, g * B), hi = std::min(mh->n, lo + B);
        if (hi > lo) {
            rc = og_jt_register_dev(p, mh->d_full[(size_t)g] + (size_t)lo * (size_t)mh->m, lo, hi, p->stream);
            if (rc) {
                og_multi_destroy(mh);
                return rc;
            }
        }
    }
    *out = mh;
    return 0;
}

int og_multi_devices(og_multi mh) { return mh ? mh->G : 0; }

int og_multi_replica_dev(og_multi mh, int32_t g, double** d_JT_full, double** d_F0, void** hip_stream) {
    if (!mh || g < 0 || g >= mh->G) return fail(1, "og_multi_replica_dev: bad argument");
    if (d_JT_full) *d_JT_full = mh->d_full[(size_t)g];
    if (d_F0) *d_F0 = mh->sub[(size_t)g]->d_f0;
    if (hip_stream) *hip_stream = (void*)mh->sub[(size_t)g]->stream;
    return 0;
}

// enqueue one sharded sweep on every device (x and hstep are host vectors); no synchronisation of the devices.
// Safe to call again before the previous step has finished: the pinned upload buffer is reused only after its
// copy has been read (a host wait on an event that is normally long past), and in peer mode a device overwrites
// its message only after every other device has fetched the previous one.
static int multi_enqueue(og_multi_s* mh, const double* x, const double* hstep) {
    const int G = mh->G, n = mh->n, B = mh->B;
    for (int g = 0; g < G; ++g) {
        og_problem_s* p = mh->sub[(size_t)g];
        OG_HIP(hipSetDevice(p->device));
        if (mh->stepped) OG_HIP(hipEventSynchronize(mh->uploaded[(size_t)g]));
        int rc = upload_point(p, x, hstep);
        if (rc) return rc;
        OG_HIP(hipEventRecord(mh->uploaded[(size_t)g], p->stream));
        if (mh->stepped && !mh->rccl && G > 1)
            for (int r = 0; r < G; ++r)
                if (r != g) OG_HIP(hipStreamWaitEvent(p->stream, mh->fetched[(size_t)r], 0));
        const int lo = std::min(n, g * B), hi = std::min(n, lo + B);
        double* block = mh->d_full[(size_t)g] + (size_t)lo * (size_t)mh->m;
        if (G > 1 || mh->rccl) {         // (one device with RCCL: the collective still runs - a plumbing check)
            // sweep of the device's block, its non-zeros straight into its message (one launch)
            rc = og_shard_sweep_dev(p, g, p->d_x, p->d_h, block, p->d_f0, mh->d_send[(size_t)g], p->stream);
            if (rc) return rc;
            if (!mh->rccl) OG_HIP(hipEventRecord(mh->packed[(size_t)g], p->stream));
        } else {
            if (hi > lo) rc = og_fd_sweep_dev(p, p->d_x, p->d_h, lo, hi, block, p->d_f0, p->stream);
            else rc = og_eval_dev(p, p->d_x, p->d_f0, p->stream);
            if (rc) return rc;
        }
    }
    if (G == 1 && !mh->rccl) {
        mh->stepped = true;
        return 0;
    }
    const size_t count = (size_t)mh->block_vals;
    if (mh->rccl) {
        int rc = g_comm.api.GroupStart();
        for (int g = 0; g < G && rc == 0; ++g)
            rc = g_comm.api.AllGather(mh->d_send[(size_t)g], mh->d_recv[(size_t)g], count, OGN_FLOAT64,
                                      mh->comms[(size_t)g], mh->sub[(size_t)g]->stream);
        const int rc2 = g_comm.api.GroupEnd();
        if (rc == 0) rc = rc2;
        if (rc != 0)
            return fail(7, std::string("og_multi_fd_sweep: ncclAllGather: ") +
                               (g_comm.api.GetErrorString ? g_comm.api.GetErrorString(rc) : "?"));
    } else {
        for (int g = 0; g < G; ++g) {
            og_problem_s* p = mh->sub[(size_t)g];
            OG_HIP(hipSetDevice(p->device));
            for (int r = 0; r < G; ++r) {
                if (r == g) continue;
                OG_HIP(hipStreamWaitEvent(p->stream, mh->packed[(size_t)r], 0));
                OG_HIP(hipMemcpyPeerAsync(mh->d_recv[(size_t)g] + (size_t)r * count, p->device, mh->d_send[(size_t)r],
                                          mh->sub[(size_t)r]->device, sizeof(double) * count, p->stream));
            }
            OG_HIP(hipEventRecord(mh->fetched[(size_t)g], p->stream));
        }
    }
    mh->stepped = true;
    for (int g = 0; g < G; ++g) {
        og_problem_s* p = mh->sub[(size_t)g];
        OG_HIP(hipSetDevice(p->device));
        int rc = og_shard_unpack_dev(p, g, mh->d_recv[(size_t)g], mh->d_full[(size_t)g], p->stream);
        if (rc) return rc;
    }
    return 0;
}

int og_multi_fd_sweep_enqueue(og_multi mh, const double* x, const double* hstep) {
    if (!mh || !x || !hstep) return fail(1, "og_multi_fd_sweep_enqueue: null argument");
    return multi_enqueue(mh, x, hstep);
}

int og_multi_synchronize(og_multi mh) {
    if (!mh) return fail(1, "og_multi_synchronize: null handle");
    for (int g = 0; g < mh->G; ++g) {
        OG_HIP(hipSetDevice(mh->sub[(size_t)g]->device));
        OG_HIP(hipStreamSynchronize(mh->sub[(size_t)g]->stream));
    }
    return 0;
}

int og_multi_fd_sweep(og_multi mh, const double* x, const double* hstep, double* JT, double* F0) {
    if (!mh || !x || !hstep || !JT) return fail(1, "og_multi_fd_sweep: null argument");
    int rc = multi_enqueue(mh, x, hstep);
    if (rc) return rc;
    // devices 1.. finish their replicas too before the call returns (one call in flight per handle)
    for (int g = 1; g < mh->G; ++g) {
        OG_HIP(hipSetDevice(mh->sub[(size_t)g]->device));
        OG_HIP(hipStreamSynchronize(mh->sub[(size_t)g]->stream));
    }
    og_problem_s* p0 = mh->sub[0];
    OG_HIP(hipSetDevice(p0->device));
    return download_block(p0, 0, mh->n, JT, F0, mh->d_full[0]);
}

int og_multi_jt_register_host(og_multi mh, double* JT) {
    if (!mh) return fail(1, "og_multi_jt_register_host: null handle");
    return og_jt_register_host(mh->sub[0], JT, 0, mh->n);
}

int og_multi_set_parameters(og_multi mh, const double* theta, int32_t count) {
    if (!mh) return fail(1, "og_multi_set_parameters: null handle");
    for (og_problem_s* sub : mh->sub) {
        const int rc = og_set_parameters(sub, theta, count);
        if (rc) return rc;
    }
    return 0;
}

int og_multi_eval(og_multi mh, const double* x, double* F) {
    if (!mh) return fail(1, "og_multi_eval: null handle");
    return og_eval(mh->sub[0], x, F);
}

}  // extern "C"
