// gpx_gp_internal.h -- the fitted-GP handle, shared by gpx_gp.hip and gpx_deriv.hip, and what the other handles share (not part of the ABI).
#pragma once
#include "gpx_common.h"
#include <cstddef>

// The handle's scalars in HBM: what a fit leaves behind, and the two flags of gp_scan_finite.  32 bytes at these offsets
// since the first version (logdet, yta, spare, info as four 8-byte slots); nothing outside this struct spells them out.
struct GpScal {
    double logdet;     // log det K from the factor's diagonal (logdet_chol)
    double yta;        // y^T alpha (dot)
    int x_bad, y_bad;  // gp_scan_finite: non-zero when x / y holds a NaN or an infinity
    int info;          // potrf: 0, the failing pivot (1-based), or < 0 for an internal failure (check_internal_info)
    int pad;
};
static_assert(sizeof(GpScal) == 32 && offsetof(GpScal, x_bad) == 16 && offsetof(GpScal, info) == 24, "GpScal layout");

struct gpx_gp {
    int device;        // the HIP device the handle lives on; every entry point makes it current
    int dtype, kernel, d, nparams;
    int64_t n, lda;
    void *x, *y, *A, *alpha, *t0, *t1;
    void *xs;          // GPX_KERNEL_GAUSSIAN_ARD only: x / w, (n, d) in the handle's dtype (gp_rescale); null otherwise
    GpScal *scal;      // device
    hipStream_t st;
    hipEvent_t ev[6];
    double params[1 + GPX_ARD_MAX_D];
    double iso[2];     // GPX_KERNEL_GAUSSIAN_ARD: (h / sqrt(wbar), 1), the isotropic constants that go with xs
    double s;
    bool have_data, have_params, fitted, have_K;
    bool x_finite, y_finite;   // scipy's check_finite=True (gp/gp.py:294, 332-334): one O(n d) device reduction per set_data
    // fit_batch workspace (grow-only, freed with the handle): the matrices of one chunk + their vectors
    gpx::GrowBuf bw; int64_t bw_cap;        // bw_cap: matrices per chunk the block holds
    // block operators of the triangular solves (built once per factor, reused by every later solve)
    gpx::TrsvOps ops;
    // fit_batch_grad: X = L^-T and W = K^-1 of one matrix at a time + the reduction's partial sums (grow-only), and
    // the block operators of the row being differentiated
    gpx::GrowBuf gw; int64_t gw_cap;   // gw_cap: rows per lock-step gradient group the block holds
    gpx::TrsvOps bops;
    double *kii;          // device, n doubles from the first leave-one-out call on: diag(K^-1) of the CURRENT factor when
    bool have_kii;        // have_kii: cleared by a new fit, and with `fitted`, which gp_unfit alone clears
    hipStream_t st_ops;   // lazily created: where gpx_gp_fit builds `ops` while the factorisation is still running
    hipEvent_t ev_ops;
};

namespace gpx {
// x_finite / y_finite of the handle from its device arrays (one O(n d) reduction; synchronous)
int gp_scan_finite(gpx_gp *g);
// The one staging pair between host float64 and device arrays of a handle's dtype (gpx_gp.hip).  A vector is rows = 1.
// host f64 (rows x cols, lds) -> device dtype (rows x cols, ldd); returns when `src` may be reused.  fp32 goes through a
// float64 staging copy on the device and one conversion launch: `stage`, when given, is that copy's buffer, allocated by
// the first call and kept by the caller (a chunked caller's first chunk is its largest); fp64 is copied straight across
int upload_f64(int dtype, void *dst, int64_t ldd, const double *src, int64_t lds, int64_t rows, int64_t cols, hipStream_t st,
               DevBuf *stage = nullptr);
// device dtype (rows x cols, lds) -> host f64 (rows x cols, ldh); lower_only: zeros above the diagonal
int download_f64(int dtype, double *dst, int64_t ldh, const void *src, int64_t lds, int64_t rows, int64_t cols, int lower_only,
                 hipStream_t st);
// the scalar block on the host: a copy on the handle's stream, a wait for it, and GPX_ERR_INTERNAL for info < 0
int gp_read_scal(gpx_gp *g, GpScal *host);
// ... and for callers that need a factor that exists: GPX_ERR_ARG "... there is no factor <what_for>" when info != 0
int gp_need_factor(gpx_gp *g, const char *what_for);
// whatever changes the data, the parameters or the matrix: no fit any more, and no diag(K^-1) of one
static inline void gp_unfit(gpx_gp *g) { g->fitted = false; g->have_kii = false; }
// The tail of a fit on g->st, behind a factor in g->A: alpha (rhs_is_row_n: L^-1 y rode along as row n of A and only the
// backward sweep is left; otherwise both sweeps from y), logdet, y^T alpha, ev[3], ev[4], fitted.  info (may be null):
// waits for all of it and takes potrf's verdict to the host
int gp_finish_fit(gpx_gp *g, bool rhs_is_row_n, int *info);
// The times of one pass on the handle's stream.  A pass is a sequence of marks: mark() records the next event of a grow-only
// pool and books the interval since the mark before it to a bucket, or to nobody (TL_NOBODY); resolve(), behind the pass's
// last synchronisation, adds the intervals up.  The passes of one handle never overlap: they share the pool
// (the sparse GP's fit and gradient, the iterative GP's solves).
constexpr int TL_NOBODY = -1;
struct PassTimeline {
    std::vector<hipEvent_t> pool;      // grow-only; the handle's destroy destroys them
    std::vector<int> bucket;           // of the marks of the current pass
    PassTimeline &begin() { bucket.clear(); return *this; }
    int mark(hipStream_t st, int b)
    {
        if (bucket.size() == pool.size()) {
            hipEvent_t e;
            GPX_HIP(hipEventCreate(&e));
            pool.push_back(e);
        }
        GPX_HIP(hipEventRecord(pool[bucket.size()], st));
        bucket.push_back(b);
        return GPX_OK;
    }
    // ms[b] (b < count) = the sum of bucket b's intervals; ms[total] = the first mark to the last
    int resolve(float *ms, int count, int total) const
    {
        for (int i = 0; i < count; ++i) ms[i] = 0.0f;
        for (size_t i = 1; i < bucket.size(); ++i) {
            if (bucket[i] == TL_NOBODY) continue;
            float t = 0.0f;
            GPX_HIP(hipEventElapsedTime(&t, pool[i - 1], pool[i]));
            ms[bucket[i]] += t;
        }
        if (bucket.size() > 1) GPX_HIP(hipEventElapsedTime(&ms[total], pool[0], pool[bucket.size() - 1]));
        return GPX_OK;
    }
    // For a pass of many marks: behind a synchronisation, ADD the intervals so far to acc[b] (TL_NOBODY's only to acc[total], which
    // gets every interval) and begin again from the last mark, so that the pass never holds more events than lie between two folds
    int fold(float *acc, int total)
    {
        for (size_t i = 1; i < bucket.size(); ++i) {
            float t = 0.0f;
            GPX_HIP(hipEventElapsedTime(&t, pool[i - 1], pool[i]));
            if (bucket[i] != TL_NOBODY) acc[bucket[i]] += t;
            acc[total] += t;
        }
        if (bucket.size() > 1) { std::swap(pool[0], pool[bucket.size() - 1]); bucket.resize(1); }
        return GPX_OK;
    }
};
// The greedy selection of gpx_sgp_select on points that are ALREADY on the device, for a caller that keeps R there (gpx_select.hip;
// the iterative GP's preconditioner).  kernel: GPX_KERNEL_GAUSSIAN or GPX_KERNEL_PERIODIC with `params` (HOST) -- the ARD family
// passes its scaled points and isotropic constants.  block: select_block_bytes() of device memory, the caller's; *R: where the
// factor lies inside it, m_max x *ldr in the dtype (*ldr = round_up(n, 128); columns [n, *ldr) are never written), *count rows
// valid.  The launches, their order and therefore every bit are gpx_sgp_select's with first = -1.  Synchronises `st`; the
// profile record and the route hits are gpx_sgp_select's.
size_t select_block_bytes(int dtype, int64_t n, int64_t m_max);
int select_on_device(int dtype, int kernel, const void *x_dev, int64_t n, int d, const double *params, int64_t m_max, double tol, void *block,
                     hipStream_t st, int64_t *count, void **R, int64_t *ldr);
// kernel parameters of a family at dimension d
static inline int nparams_of(int kernel, int d) { return kernel == GPX_KERNEL_GAUSSIAN_ARD ? 1 + d : (kernel == GPX_KERNEL_PERIODIC ? 3 : 2); }
// The points and the two isotropic constants this handle's launches use: its own (x, params), or for the ARD family the
// scaled points and (h / sqrt(wbar), 1) as GPX_KERNEL_GAUSSIAN  --  k_ard(a, b; h, w) = k_gaussian(a / w, b / w; h / sqrt(wbar), 1)
struct GpView { int kernel; const void *x; const double *params; };
static inline GpView gp_view(const gpx_gp *g)
{
    if (g->kernel == GPX_KERNEL_GAUSSIAN_ARD) return {GPX_KERNEL_GAUSSIAN, g->xs, g->iso};
    return {g->kernel, g->x, g->params};
}
// ARD: xs <- x / w and iso, enqueued on the handle's stream, once data and parameters are both there (no-op otherwise)
int gp_rescale(gpx_gp *g);
// The reduction half of the leave-one-out gradient (gpx_loograd.hip): (alpha, v.r, Pm) of one system in HBM -> out
// (n_params + 1, order (kernel params..., s)) and the criterion's value (may be null).  pts, params, s_noise, part: as
// grad_reduce's in gpx_gp.hip.  Synchronises g->st.
int loo_grad_reduce(gpx_gp *g, const void *pts, const void *alpha, const double *params, double s_noise, const LooVecs &v,
                    const void *Pm, int64_t ldp, double *part, double *value, double *out);
}

static const char *const NONFINITE_MSG = "array must not contain infs or NaNs";      // scipy's text (gp/gp.py:294, 332-334)

#define GP_NEED_FINITE_Y(g)                                                    \
    do { if (!(g)->y_finite) { gpx::set_error("%s (y)", NONFINITE_MSG); return GPX_ERR_ARG; } } while (0)

// every gpx_gp_* entry: the handle's device becomes current for the duration of the call, and the handle's stream takes
// its turn among the streams this host thread drives (StreamTurn, gpx_mem.h); with GPX_ROCTX=1 the call is a roctx range
#define GP_ENTER(g)                                                          \
    GPX_ARG((g) != nullptr, "gp is NULL");                                   \
    gpx::tune_refresh();                                                     \
    gpx::DeviceGuard guard__((g)->device);                                   \
    if (guard__.rc != GPX_OK) return guard__.rc;                             \
    gpx::StreamTurn turn__((g)->st);                                         \
    gpx::RoctxRange api_range__(__func__)

