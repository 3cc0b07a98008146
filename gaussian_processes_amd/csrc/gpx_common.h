// gpx_common.h -- shared internals of libgpx.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <math.h>
#include <type_traits>
#include <vector>

#include "../../include/gpx.h"
#include "gpx_tune.h"

namespace gpx {

void set_error(const char *fmt, ...);
int  hip_fail(hipError_t e, const char *what, const char *file, int line);
int  ensure_device();   // GPX_OK when a GPU is usable

#define GPX_HIP(call)                                                        \
    do {                                                                     \
        hipError_t e__ = (call);                                             \
        if (e__ != hipSuccess) return gpx::hip_fail(e__, #call, __FILE__, __LINE__); \
    } while (0)

#define GPX_TRY(call)                                                        \
    do {                                                                     \
        int rc__ = (call);                                                   \
        if (rc__ != GPX_OK) return rc__;                                     \
    } while (0)

#define GPX_ARG(cond, msg)                                                   \
    do {                                                                     \
        if (!(cond)) { gpx::set_error("%s: %s", __func__, msg); return GPX_ERR_ARG; } \
    } while (0)

#define GPX_LAUNCH_CHECK()                                                   \
    do {                                                                     \
        hipError_t e__ = hipGetLastError();                                  \
        if (e__ != hipSuccess) return gpx::hip_fail(e__, "kernel launch", __FILE__, __LINE__); \
    } while (0)

// Environment switches: ONE table, gpx_tune.h -- every extern "C" entry takes one snapshot of the
// GPX_* variables for the calling thread (tune_refresh), everything below reads tune().field.  Nothing in the library
// calls getenv.

// Route counters (gpx_debug_route_count): which of the alternative routes a call took, counted on the host at the
// point of decision.  Tests that force a route through an environment switch assert it here.
enum Route { RT_TRSV_OPS = 0, RT_TRSV_STEPS = 1, RT_PANEL_RES = 2, RT_PANEL_CHAIN = 3, RT_FIT_RIDE = 4,
             RT_FIT_TWO_SOLVES = 5, RT_GEMM_FAST = 6, RT_GEMM_GENERIC = 7, RT_SYRK_EXACT = 8, RT_SYRK_PATCH = 9,
             RT_MG_BCAST_ONE = 10, RT_MG_BCAST_SAG = 11, RT_FIT_OPS_AHEAD = 12, RT_TRSM_OPS = 13, RT_POTRF_PAIR = 14, RT_VAR_CHUNK = 15, RT_LOO_CHUNK = 16,
             RT_TRSM_L_OPS = 17, RT_GRAD_CHUNK = 18, RT_EXTEND = 19, RT_SAMPLE = 20, RT_KAPPLY_FUSED = 21, RT_KAPPLY_GEMM = 22, RT_PATHS_GRAD_CHUNK = 23, RT_REMOVE = 24, RT_SPARSE_CHUNK = 25, RT_SELECT_STEP = 26, RT_CG_ITER = 27, RT_LOWRANK = 28, RT_COUNT = 29 };
void route_hit(int route);

// LAPACK-style info of a factorisation as the host sees it: > 0 "not positive definite" (the caller's business),
// < 0 an INTERNAL failure of the factorisation (a hand-off inside the resident panel kernel timed out: -7) --
// never to be mistaken for a property of the matrix.  Returns GPX_ERR_INTERNAL for the latter.
int check_internal_info(int info);

static inline hipStream_t S(void *s) { return (hipStream_t)s; }
static inline size_t esize(int dtype) { return dtype == GPX_F64 ? 8 : 4; }
static constexpr int64_t round_up(int64_t v, int64_t m) { return (v + m - 1) / m * m; }
static constexpr int64_t cdiv(int64_t a, int64_t b) { return (a + b - 1) / b; }

// a "now" on `to` after everything enqueued so far on `from`, through an event the caller owns
static inline int order(hipEvent_t e, hipStream_t from, hipStream_t to)
{
    GPX_HIP(hipEventRecord(e, from));
    GPX_HIP(hipStreamWaitEvent(to, e, 0));
    return GPX_OK;
}
// Sync events (no timing) handed out in order, created on demand and reused after rewind().  ONE owner each (a thread's
// look-ahead slot, a multi-GPU handle), who rewinds only when nothing that waits for an event of the round before is pending.
struct EventPool {
    std::vector<hipEvent_t> ev; size_t next = 0;
    int reserve(size_t count)
    {
        while (ev.size() < count) {
            hipEvent_t x;
            GPX_HIP(hipEventCreateWithFlags(&x, hipEventDisableTiming));
            ev.push_back(x);
        }
        return GPX_OK;
    }
    int get(hipEvent_t *e) { GPX_TRY(reserve(next + 1)); *e = ev[next++]; return GPX_OK; }
    void rewind() { next = 0; }
    void destroy() { for (hipEvent_t e : ev) (void)hipEventDestroy(e); ev.clear(); next = 0; }
    int order(hipStream_t from, hipStream_t to) { hipEvent_t e; GPX_TRY(get(&e)); return gpx::order(e, from, to); }
};

// ---- live per-kernel-class timing (HIP events around each launch; off by default) ----
enum ProfClass { PC_KMAT = 0, PC_GEMM = 1, PC_POTRF_DIAG = 2, PC_TRSM_ROWS = 3, PC_TRSV = 4,
                 PC_MEAN = 5, PC_REDUCE = 6, PC_GEMM_SKINNY = 7, PC_GEMM_GENERIC = 8, PC_GEMM_PANEL = 9, PC_GEMM_N64 = 10,
                 PC_TRANSPOSE = 11, PC_PRED_GRAD = 12, PC_EXTEND = 13, PC_RANDN = 14, PC_RFF = 15, PC_KAPPLY = 16, PC_KAPPLY_GRAD = 17, PC_CHOL_DELETE = 18, PC_SPARSE_GRAM = 19, PC_SPARSE_GRAD = 20, PC_SPARSE_ZGRAD = 21, PC_SELECT = 22, PC_CG = 23, PC_LOWRANK = 24, PC_COUNT = 25 };
extern bool g_prof_on;
// the registry is shared by all host threads (mutex inside); a scope ends its OWN record
int  prof_begin(int cls, double work, hipStream_t st);    // record index, -1 when nothing was recorded
void prof_end(int rec, hipStream_t st);
void prof_set_work(int rec, double work);                  // a record whose work is known only once its launches have run
// roctx ranges (GPX_ROCTX=1; libroctx64.so by dlopen): every gpx_gp_* call and every launch class below it is a nested host
// range, so `rocprofv3 --marker-trace --kernel-trace` shows which stage of a fit a kernel belongs to.  Off: one field of the snapshot per scope.
bool roctx_push(const char *name);          // false: ranges are off (or the library is not there): nothing to pop
void roctx_pop();
struct RoctxRange {
    bool on;
    explicit RoctxRange(const char *name) : on(roctx_push(name)) {}
    ~RoctxRange() { if (on) roctx_pop(); }
};
const char *prof_class_name(int cls);

// launches the calling thread makes while this is > 0 are not recorded (the asm leaf's self-check: its nested launches
// are no part of anybody's fit)
extern thread_local int g_prof_mute;
struct ProfScope {
    hipStream_t st; int rec; RoctxRange range;
    ProfScope(int cls, double work, hipStream_t s) : st(s), rec(g_prof_on && g_prof_mute == 0 ? prof_begin(cls, work, s) : -1), range(prof_class_name(cls)) {}
    ~ProfScope() { if (rec >= 0) prof_end(rec, st); }
};

// hipFuncAttributeMaxDynamicSharedMemorySize, once per (kernel, device); thread-safe.  Once: so `bytes` is a constant of the
// kernel, never the size one call happens to need -- LDS_CHUNK_MAX for the kernels that stage a chunk of points and refuse a
// d beyond it (kmat, the streamed kernels), LDS_TILE_MAX for the tile reductions, which do not: the CU's 160 KiB less 4 KiB
// for their static reduction slots (the limit counts dynamic bytes only; a launch beyond it is a HIP launch error).  Through a
// fitted handle kmat's own range of d keeps them below 48 KiB; called with a larger d, fp64 d = 156 .. 158 would have launched
// with the call's exact size as the limit and does not with this constant
int set_max_lds(const void *fn, int bytes);
constexpr int LDS_CHUNK_MAX = 96 * 1024, LDS_TILE_MAX = 156 * 1024;

// Makes `device` current for the calling host thread and restores the previous one on scope
// exit (HIP's current device is per host thread; handles remember the device they live on).
struct DeviceGuard {
    int prev = -1; bool switched = false; int rc = GPX_OK;
    explicit DeviceGuard(int device)
    {
        if (hipGetDevice(&prev) != hipSuccess) { (void)hipGetLastError(); prev = -1; }
        if (device >= 0 && device != prev) {
            hipError_t e = hipSetDevice(device);
            if (e != hipSuccess) rc = hip_fail(e, "hipSetDevice", __FILE__, __LINE__);
            else switched = true;
        }
    }
    ~DeviceGuard() { if (switched && prev >= 0) (void)hipSetDevice(prev); }
};

}  // namespace gpx
#include "gpx_mem.h"   // who owns which device memory; StreamTurn
namespace gpx {

// parameters of a kernel-matrix member, precomputed on the host in f64
struct KParams {
    double c[6];     // member-specific constants (see gpx_kmat.hip)
    double diag_add;
    int kernel;
    int member;
};
int make_kparams(int kernel, int member, const double *params, double diag_add, KParams *out);

// Batched launches: `count` matrices of identical shape; element strides between consecutive
// matrices for the A / B / C operands of a product (one stride for everything else).
// Optional second batch dimension (count2 > 1; launch grid z): matrix (i, i2) sits at i * s + i2 * t.
struct Batch {
    int count; int64_t sA, sB, sC;
    int count2 = 1; int64_t tA = 0, tB = 0, tC = 0;
};

// internal (non-ABI) helpers shared between translation units
// C = beta * C + alpha * A * B^T with beta = 1 (default) or 0 (beta0 != 0: C is not read)
int gemm_nt(int dtype, int64_t M, int64_t N, int64_t K, const void *A, int64_t lda, const void *B,
            int64_t ldb, void *C, int64_t ldc, double alpha, int tri, int64_t row0, int64_t col0,
            hipStream_t st, int beta0 = 0, int ktri = 0, const Batch *bt = nullptr,
            int wide_tiles = 0);   // wide_tiles: 128-wide tiles whatever the tile count (N <= 128: ONE tile per row block,
                                   // which is what makes C == A legal -- a tile reads its rows of A before it stores them)
// (ktri != 0: A == B is upper triangular in (row, k) and M == N == K -- the k-loop of tile row i skips k < i)
// X[r, 0:jb] <- X[r, 0:jb] * Ljj^-T for rows r in [0, rows); Ljj = jb x jb lower block
int trsm_rows(int dtype, void *X, int64_t ldx, int64_t rows, const void *Ljj, int64_t ldl, int jb,
              hipStream_t st, const Batch *bt = nullptr);   // bt: sA = stride of X, sB = stride of Ljj
int syrk_bc(int dtype, int64_t n, int64_t row_begin, void *Cloc, int64_t ldc, int64_t cl0, int64_t cl1,
            const void *Pb, int64_t ldp, int64_t k0, int64_t kb, int64_t nb, int P, int rank,
            hipStream_t st, const int *abort_flag = nullptr, const Batch *bt = nullptr);
// What potrf()'s schedule knows about ONE panel and the launch cannot see, by value down to the resident launch (gpx_panel.hip).
// idle_chip: the panel's FIRST launch will find the chip idle (it is ordered behind the update before it and ahead of the
// one that runs beside it) and may claim whole CUs (GPX_PANEL_EXCL_ROWS); later launches of the same panel (the right half
// of a wide one) start on a chip that the update has filled meanwhile: they must not wait for empty CUs.
// leaf_force: the leaf self-check's own launches: 1 / 4 / 5, no check (0: the leaf is chosen as usual)
struct PanelHints { bool idle_chip = false; int leaf_force = 0; };
// potrf() progress hook (null: none): called with the number of leading columns that are final once `panel_done` has
// fired; single matrices with more than one outer block only.  (gpx_gp_fit builds the solves' block operators while the
// factorisation runs.)
struct PotrfHook { int (*fn)(void *user, int64_t cols_done, hipEvent_t panel_done); void *user; };
// factor rows [r0, n) x columns [c0, c0 + kb) of A whose diagonal block sits at (r0, c0)
// done: an event recorded behind the panel's last launch
int potrf_panel(int dtype, void *A, int64_t lda, int64_t n, int64_t r0, int64_t c0, int64_t kb,
                int *info_dev, hipStream_t st, const Batch *bt = nullptr, int64_t kpre = 0,   // kpre: see potrf_panel_res
                hipEvent_t done = nullptr, PanelHints hints = {});
int potrf(int dtype, void *A, int64_t n, int64_t lda, int *info_dev, hipStream_t st, const Batch *bt = nullptr,
          int64_t xrows = 0,       // xrows: extra rows below the matrix that ride along (A has n + xrows rows)
          bool may_block = false,  // may_block: the caller allows the host to pace the panel launches (hipEventSynchronize
                                   // inside the call); false: a pure enqueue (gpx_d_potrf, anything under stream capture)
          const PotrfHook *hook = nullptr);
// the same panel in ONE launch (gpx_panel.hip): kb a multiple of 64, at most panel_res_max()
int potrf_panel_res(int dtype, void *A, int64_t lda, int64_t n, int64_t r0, int64_t c0, int64_t kb, int *info_dev,
                    hipStream_t st, const Batch *bt = nullptr, int64_t kpre = 0, hipEvent_t done = nullptr, PanelHints hints = {});
int64_t panel_res_max();
// this host thread's look-ahead stream of the blocked factorisation on the current device (nullptr before the first
// one): it lives as long as the thread, so an event may be recorded on it at any time
hipStream_t potrf_side_stream();
// would K(x, x) + s^2 I hold only finite numbers for finite x?  (gpx_gp.hip; the check_finite of the reference's cho_factor)
bool kernel_values_finite(int kernel, const double *p, double s, int dtype);   // in the handle's arithmetic
bool panel_res_fold(int64_t rows, int64_t kpre, int64_t kb, size_t es, int64_t lda, const void *base);
// Per-factor block operators of the single-right-hand-side solves (gpx_solve.hip, "operator form"): owned by
// whoever owns the factor; `valid` must be cleared whenever the factor changes.  nullptr: built per call.
constexpr int TRSV_OPS_BLOCK = 512;          // columns of an operator block: the one copy outside gpx_solve.hip
static inline int64_t trsv_ops_nblocks(int64_t n) { return n / TRSV_OPS_BLOCK; }            // full blocks of n columns
static inline bool trsv_ops_whole_blocks(int64_t n) { return n >= TRSV_OPS_BLOCK && n % TRSV_OPS_BLOCK == 0; }
struct TrsvOps {
    GrowBuf mem;                 // trsv_ops_bytes(dtype, n) of the factor; a view() never release()s
    bool valid = false;          // all blocks of the CURRENT factor have their operators
    int64_t built = 0;           // leading blocks of the current factor that have them (trsv_ops_build_upto)
    void invalidate() { valid = false; built = 0; }   // a new factor: every owner calls this, never `valid = false` alone
    // no operators yet, in `bytes` of somebody else's block (not owned, not freed)
    static TrsvOps view(void *p, size_t bytes) { TrsvOps o; o.mem.p = p; o.mem.bytes = bytes; return o; }
};
// Build the operators of an n x n factor (whole blocks only) ahead of time on `st`; a later trsv_lower with these ops
// takes the operator route whatever n is (the distributed solve prepares each diagonal block right after its panel).
int trsv_ops_build(int dtype, const void *L, int64_t n, int64_t ldl, TrsvOps *ops, hipStream_t st);
// The same in instalments, while the factorisation is still running: the operators of the blocks [ops->built, kend) --
// which need nothing but block columns < kend of L -- on `st`; ops->valid once kend reaches trsv_ops_nblocks(n).  At
// least two whole blocks only (trsv_ops_ahead_ok); the first call of a factor passes ops->built == 0.
bool trsv_ops_ahead_ok(int dtype, const void *L, int64_t n, int64_t ldl);
bool trsm_ops_ok(int dtype, const void *L, int64_t n, int64_t ldl);   // ... and trsm_right_lt would use them (GPX_TRSM_OPS)
size_t trsv_ops_bytes(int dtype, int64_t n);
int trsv_ops_build_upto(int dtype, const void *L, int64_t n, int64_t ldl, TrsvOps *ops, int64_t kend, hipStream_t st);
int trsv_lower(int dtype, const void *L, int64_t n, int64_t ldl, void *b, void *x, int transpose,
               hipStream_t st, const Batch *bt = nullptr,   // bt: sA = stride of L, sB = stride of b / x
               TrsvOps *ops = nullptr);
int trsm_right_lt(int dtype, const void *L, int64_t n, int64_t ldl, void *X, int64_t m, int64_t ldx,
                  hipStream_t st, int x_upper = 0, TrsvOps *ops = nullptr,    // ops: this factor's block operators (completed here if need be): in-block substitution = one product with inv(L_kk)
                  int64_t c0 = 0);   // c0 > 0 (x_upper, a multiple of 64): X is rows [c0, c0 + m) of the identity; the sweep begins at c0 (operator route: at c0's block)
// X (m x n, ldx) <- X * L^-1, in place (gpx_solve.hip): the mirror of trsm_right_lt, block columns from the last to the first.
// ops: this factor's block operators (completed here if need be): in-block solve = one product with Wt_k.  Without them
// (or where trsm_ops_ok says no) the 64-wide route.  Scratch: the transposed row panels of L, at most n x TRSV_OPS_BLOCK.
int trsm_right_l(int dtype, const void *L, int64_t n, int64_t ldl, void *X, int64_t m, int64_t ldx, hipStream_t st,
                 TrsvOps *ops = nullptr);
// Input-space gradient pass (gpx_stream.hip): gpx_d_pred_grad's arguments on GPX_KERNEL_GAUSSIAN / GPX_KERNEL_PERIODIC points;
// col_div (HOST, d doubles, or null): column k of the result is divided by col_div[k] (the ARD family on scaled points).
int pred_grad(int dtype, int kernel, const void *xo, int64_t m, const void *x, int64_t n, int d, const double *params,
              const void *alpha, const void *B, int64_t ldb, double scale, const double *col_div, double *out_dev, hipStream_t st);
// K^-1 = L^-T L^-1 from a factor: X <- L^-T (the identity through trsm_right_lt), W <- X X^T, tri = GPX_FULL or GPX_LOWER (the
// other half cleared).  X, W: n x ldl each.  count == 1: `ops` are the factor's own.  count > 1: a LOCK-STEP group (trsm_ops_ok
// only): factors sL elements apart, X and W blocks n * ldl apart, operators built here into group_ops (count * trsv_ops_bytes).
int inv_from_factor(int dtype, const void *L, int64_t n, int64_t ldl, void *X, void *W, int tri, hipStream_t st,
                    TrsvOps *ops, int count = 1, int64_t sL = 0, void *group_ops = nullptr);
// The small shared blocks (gpx_small.hip).  logdet_chol, dot, sum_f64, diag_sum: one workgroup, fixed order; count > 1: one
// workgroup per matrix / pair.  diag_sum: out_dev[0] = sum A[i, i].  transpose: dst (cols x rows, ldd) <- src (rows x cols, lds)^T;
// mirror != 0: src == dst allowed, only the tiles at or below the diagonal are read and only elements strictly above it are
// written (the lower triangle mirrored into the upper one).  tril: the strict upper triangle <- 0.
int logdet_chol(int dtype, const void *L, int64_t n, int64_t ldl, double *out_dev, hipStream_t st, int count = 1,
                int64_t sL = 0, int64_t so = 0);
int dot(int dtype, const void *a, const void *b, int64_t n, double *out_dev, hipStream_t st, int count = 1,
        int64_t sa = 0, int64_t sb = 0, int64_t so = 0);
int diag_sum(int dtype, const void *A, int64_t n, int64_t lda, double *out_dev, hipStream_t st);
int transpose(int dtype, const void *src, int64_t lds, int64_t rows, int64_t cols, void *dst, int64_t ldd, int mirror, hipStream_t st);
int tril(int dtype, void *A, int64_t n, int64_t lda, hipStream_t st);
// Predictive variance (gpx_solve.hip).  var_rows: out_dev[i] = kdiag(i) - sum_j X[i, j]^2 over a solved rows x n chunk
// (gpx_d_var_rows' arguments), or with accumulate != 0: out_dev[i] += sum_j X[i, j]^2 (no kdiag; the distributed form adds
// its blocks' sums in block order).  var_finish: out_dev[i] = k(xo_i, xo_i) - acc_dev[i].  Sums and outputs are f64.
int var_rows(int dtype, int kernel, const void *X, int64_t rows, int64_t n, int64_t ldx, const void *xo, int d,
             const double *params, const double *kdiag_dev, int accumulate, double *out_dev, hipStream_t st);
int var_finish(int dtype, int kernel, const void *xo, int d, const double *params, const double *acc_dev, int64_t rows,
               double *out_dev, hipStream_t st);
// Leave-one-out from the factor (gpx_solve.hip).  eye_rows (gpx_small.hip): X (rows x ld) <- rows [c0, c0 + rows) of the
// identity, columns [cz, ld) only.  loo_rows: gpx_d_loo_rows' arguments, over the chunk solved from that seed.  loo_points: the same per-point
// quantities from a diagonal kii that is already there.  sum_f64: out_dev[0] = sum a[i], one workgroup, fixed order.
int eye_rows(int dtype, void *X, int64_t rows, int64_t ld, int64_t c0, int64_t cz, hipStream_t st);
int loo_rows(int dtype, const void *X, int64_t rows, int64_t n, int64_t ldx, int64_t c0, const void *y, const void *alpha,
             double *kii, double *mean, double *var, double *logp, hipStream_t st);
int loo_points(int dtype, const double *kii, const void *y, const void *alpha, int64_t n, double *mean, double *var, double *logp,
               hipStream_t st);
int sum_f64(const double *a, int64_t n, double *out_dev, hipStream_t st);
// Growing a fitted handle (gpx_extend.hip).  copy_lower: gpx_d_copy_lower's arguments.  schur_lower: gpx_d_schur_lower's.
int copy_lower(int dtype, const void *src, int64_t lds, void *dst, int64_t ldd, int64_t n, hipStream_t st);
int schur_lower(int dtype, const void *B, int64_t k, int64_t n, int64_t ldb, void *S, int64_t lds, hipStream_t st);
// The slices' partial sums folded (gpx_sparse.hip): gpx_d_sum_slices_lower's arguments; minus_from (n x ldo, or null; may be
// out): the sum is subtracted from it instead
int sum_slices_lower(int dtype, const void *P, int64_t ldp, int64_t sP, int slices, int64_t n, const void *minus_from, void *out, int64_t ldo,
                     hipStream_t st);
// Shrinking one (gpx_remove.hip).  chol_delete: gpx_d_chol_delete's arguments, already checked (the caller holds the StreamTurn).
int chol_delete(int dtype, const void *L, int64_t n, int64_t ldl, const int64_t *idx_host, int64_t k, void *out, int64_t ldo, hipStream_t st);
// Sampling (gpx_sample.hip).  randn: gpx_d_randn's arguments.  mvn_sample: gpx_d_mvn_sample's.
int randn(int dtype, void *out, int64_t rows, int64_t cols, int64_t ld, uint64_t seed, uint64_t stream, uint64_t offset, hipStream_t st);
int mvn_sample(int dtype, void *C, int64_t m, int64_t ldc, const void *mean, double jitter, int64_t S, uint64_t seed, uint64_t stream,
               void *Z, int64_t ldz, void *out, int64_t ldo, int *info_dev, hipStream_t st);
// Posterior paths (gpx_paths.hip).  rff_features: gpx_d_rff_features' arguments.  kmat_apply: gpx_d_kmat_apply's (the caller
// holds the StreamTurn: both routes use this host thread's scratch).  kapply_fused: its fused route (gpx_stream.hip) for a
// (d, S) that kapply_fused_fits takes; kp: member GPX_K of GPX_KERNEL_GAUSSIAN or GPX_KERNEL_PERIODIC.
bool kapply_fused_fits(int dtype, int d, int64_t S);
int kapply_fused(int dtype, const void *xo, int64_t m, const void *x, int64_t n, int d, const KParams &kp, const void *V, int64_t ldv,
                 int64_t S, void *out, int64_t ldo, hipStream_t st);
int rff_features(int dtype, const void *pts, int64_t m, int d, const double *omega_dev, int64_t F, double scale, void *out, int64_t ld,
                 hipStream_t st);
// Their input-space gradients.  rff_features_grad: gpx_d_rff_features_grad's arguments (gpx_paths.hip).  kapply_grad:
// gpx_d_kmat_apply_grad's on GPX_KERNEL_GAUSSIAN points (gpx_stream.hip; the caller holds the StreamTurn).
int rff_features_grad(int dtype, const void *pts, int64_t m, int d, const double *omega_dev, int64_t F, double scale, const double *col_div,
                      void *out, int64_t ld, hipStream_t st);
int kapply_grad(int dtype, const void *xo, int64_t m, const void *x, int64_t n, int d, const double *params, const double *col_div,
                const void *V, int64_t ldv, int64_t S, void *out, int64_t ldo, hipStream_t st);
int kmat_apply(int dtype, int kernel, const void *xo, int64_t m, const void *x, int64_t n, int d, const double *params, const void *V,
               int64_t ldv, int64_t S, void *out, int64_t ldo, hipStream_t st);
// The row chunking of a predictive-variance call (gpx_gp.hip; host arithmetic): *rows per chunk, *chunks, *bytes of device
// memory one chunk needs.  chunk_rows 0: the largest multiple of 128 (at most var_chunk_cap) whose buffers fit a quarter
// of free_bytes.  GPX_ERR_ARG / GPX_ERR_NOMEM as gpx_debug_var_plan documents.
int var_plan(int dtype, int64_t n, int64_t m, int64_t chunk_rows, size_t free_bytes, int64_t *rows, int64_t *chunks, size_t *bytes);
// The fused tile reductions (gpx_kmat.hip; one kernel pair, two host entries): sum_ji coef_ji dk_p(row_j, col_i) with the
// kernel derivatives formed in the tile and ONE matrix in memory, read once.
//   tile_reduce, the symmetric pass over K(x, x), x (n, d): coef = G, M's lower triangle read.  vec_b == nullptr: the marginal
//     likelihood, G = a a^T - M (a = alpha, M = K^-1); otherwise the leave-one-out criterion, G = (b a^T + a b^T) / 2 - M
//     (b = r, M = Pm = K^-1 diag(c) K^-1).  last = trace M.
//   rect_reduce, the rectangular pass over K(x, z), the N-sized pass of the sparse GP's gradient: rows x (n, d), columns
//     z (m, d), coef_ji = P[j, i] + y_j w_i (P: n x ldp; y: n; w: m).  last = sum coef k (ARD: 0, S_0 is that sum).
// kernel == GPX_KERNEL_GAUSSIAN_ARD for either: the points are the SCALED ones and params = iso = (h / sqrt(wbar), 1) --
// reduce_params() hands a caller that pair (in iso2) for the family's own parameters, and `params` itself for the other kernels.
// out (host): [P0, P1, P2, last] for GPX_KERNEL_GAUSSIAN / GPX_KERNEL_PERIODIC, [S_0, S_1 .. S_d, last] for the ARD family
// (S_0 = sum coef k, S_k = sum coef k t_k^2): dloglh_partial_doubles() / 1024 values.  partial_dev: dloglh_partial_doubles()
// DEVICE doubles.  One partial per workgroup and quantity, added by the host in workgroup order: no atomics.  Both
// synchronise `st`.
// grad_from_sums: a symmetric pass's sums -> the gradient (kernel params ..., s); `factor` 1/2 (marginal likelihood) or 1 (LOO).
int tile_reduce(int dtype, int kernel, const void *x, int64_t n, int d, const double *params, const void *vec_a, const void *vec_b,
                const void *M, int64_t ldm, double *partial_dev, double *out, hipStream_t st);
int rect_reduce(int dtype, int kernel, const void *x, int64_t n, const void *z, int64_t m, int d, const double *params, const void *P,
                int64_t ldp, const void *y, const void *w, double *partial_dev, double *out, hipStream_t st);
const double *reduce_params(int kernel, int d, const double *params, double *iso2);
// What the tile reductions of both files (gpx_kmat.hip, gpx_lrgrad.hip) share: the tile edge and the fixed grid, the derivative
// constants of a family (make_grad_params: GPX_KERNEL_GAUSSIAN or GPX_KERNEL_PERIODIC; the latter needs d == 1), the Gaussian
// k's constant and the ladder of the ARD kernels' accumulator counts.
constexpr int GR_T = 64;           // tile edge
constexpr int GR_BLOCKS = 1024;
struct GradParams {
    double c1, c2h, c2w, c3w;      // gaussian: e = c1*d2 ; dK_dh = c2h*exp(e) ; dK_dw = exp(e)*(c3w*d2 - c2w)
    double h, w, p;                // periodic
    int kernel, nkp;
};
int make_grad_params(int kernel, int d, const double *params, GradParams *gpar);
// the Gaussian k's constant, make_kparams' c2 of GPX_K: h^2 sqrt(2 / pi) / (2 w).  (make_kparams multiplies h * h first, which
// rounds differently in one pair of three: one spelling there would move either every entry of K or every gradient by an ulp)
static inline double gaussian_k_const(double h, double w) { return 0.5 * sqrt(2.0 / M_PI) * h * h / w; }
// f(std::integral_constant<int, DMAX>()) for the rung of the ARD kernels' ladder that holds d: `decltype(dm)::value` names DMAX
template <typename F>
static inline int by_dmax(int d, F f)
{
    if (d <= 8) return f(std::integral_constant<int, 8>());
    if (d <= 16) return f(std::integral_constant<int, 16>());
    if (d <= 32) return f(std::integral_constant<int, 32>());
    return f(std::integral_constant<int, 64>());
}
// The low-rank tile reduction (gpx_lrgrad.hip): gpx_d_lowrank_reduce's arguments behind its checks; partial_dev:
// dloglh_partial_doubles() DEVICE doubles.  Synchronises `st`.
int lowrank_reduce(int kernel, const void *x, int64_t n, int d, const double *params, const double *U, const double *V, int64_t ld,
                   int64_t T, double *partial_dev, double *out, hipStream_t st);
// The rectangular pass whose result is per COLUMN point and dimension (gpx_zgrad.hip; the sparse GP's gradient in the inducing
// inputs): gpx_d_rect_zgrad's arguments on GPX_KERNEL_GAUSSIAN / GPX_KERNEL_PERIODIC points (the ARD family: the scaled points,
// iso and col_div = the widths).  partial_dev: rect_zgrad_partial_doubles(kernel, m, d) DEVICE doubles.  Enqueues and returns.
size_t rect_zgrad_partial_doubles(int kernel, int64_t m, int d);
int rect_zgrad(int dtype, int kernel, const void *r, int64_t n, const void *q, int64_t m, int d, const double *params, const void *C,
               int64_t ldc, const void *u, const void *v, double scale, const double *col_div, double *partial_dev, double *out_dev,
               hipStream_t st);
void grad_from_sums(int kernel, int d, const double *params, const double *S, double quad, double noise_scale, double factor,
                    double *out);
// The Gaussian ARD family (gpx_kmat.hip): out <- x / w (w_host: d doubles; out may be x).
// dloglh_partial_doubles: the DEVICE doubles either reduction needs for its per-workgroup partial sums.
struct ArdWidths { double w[GPX_ARD_MAX_D]; };   // the widths as a kernel argument
int scale_points(int dtype, const void *x, int64_t n, int d, const double *w_host, void *out, hipStream_t st);
int ard_scratch(size_t bytes, void **p);         // this host thread's block for the scaled copies of a call's two point sets
// (h / sqrt(wbar), 1) of ARD parameters (h, w_1 ... w_d): wbar = exp(sum log w_k / d) in the host's double arithmetic
void ard_iso(const double *params, int d, double *iso2);
size_t dloglh_partial_doubles(int kernel, int d);
int kmat(int dtype, int kernel, int member, const void *x1, int64_t n, const void *x2, int64_t m,
         int d, const double *params, double diag_add, int tri, void *out, int64_t ld, hipStream_t st);
// The ingredients of the leave-one-out gradient's weights G = (r alpha^T + alpha r^T) / 2 - Pm from a factor (gpx_loograd.hip).
// One system's vectors, all in ONE block of loo_vec_bytes() that the caller owns (loo_vecs_at lays it out):
struct LooVecs {
    double *kii, *logp;          // n doubles each: diag(K^-1) and the per-point log p(y_i | the others)
    double *sums;                // [0]: sum of logp (fixed order: sum_f64)   [1]: r . alpha
    void *u, *sq, *t, *r;        // n each, the system's dtype: alpha / k, sqrt(c), solve scratch, r = K^-1 (alpha / k)
};
size_t loo_vec_bytes(int dtype, int64_t n);
LooVecs loo_vecs_at(void *block, int dtype, int64_t n);
// loo_weights_vectors: behind inv_from_factor(..., GPX_FULL, ...), X = L^-T and W = K^-1 in HBM.  k from the rows of X as
// loo_rows sums them (kii_have != null: that diagonal instead, through loo_points), the criterion's value, c, r by two
// sweeps with the factor, then Y = W diag(sqrt(c)) over X.  loo_weights_product: Pm = Y Y^T, lower triangle, over W, for
// `count` systems n * ldl elements apart in lock-step.  loo_weights_from_factor: all of it for one system.
int loo_weights_vectors(int dtype, const void *L, int64_t n, int64_t ldl, const void *y, const void *alpha, void *X, const void *W,
                        const LooVecs &v, const double *kii_have, TrsvOps *ops, hipStream_t st);
int loo_weights_product(int dtype, int64_t n, int64_t ldl, const void *Y, void *Pm, int count, hipStream_t st);
int loo_weights_from_factor(int dtype, const void *L, int64_t n, int64_t ldl, const void *y, const void *alpha, void *X, void *W,
                            const LooVecs &v, const double *kii_have, TrsvOps *ops, hipStream_t st);

}  // namespace gpx
