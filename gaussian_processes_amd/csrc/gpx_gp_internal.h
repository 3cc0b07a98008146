// gpx_gp_internal.h -- the fitted-GP handle, shared by gpx_gp.hip and gpx_deriv.hip (not part of the ABI).
#pragma once
#include "gpx_common.h"

struct gpx_gp {
    int device;        // the HIP device the handle lives on; every entry point makes it current
    int dtype, kernel, d, nparams;
    int64_t n, lda;
    void *x, *y, *A, *alpha, *t0, *t1;
    void *xs;          // GPX_KERNEL_GAUSSIAN_ARD only: x / w, (n, d) in the handle's dtype (gp_rescale); null otherwise
    double *scal;      // device: [0] logdet [1] y^T alpha [2] spare ; int info at scal + 3
    hipStream_t st;
    hipEvent_t ev[6];
    double params[1 + GPX_ARD_MAX_D];
    double iso[2];     // GPX_KERNEL_GAUSSIAN_ARD: (h / sqrt(wbar), 1), the isotropic constants that go with xs
    double s;
    bool have_data, have_params, fitted, have_K;
    bool x_finite, y_finite;   // scipy's check_finite=True (gp/gp.py:294, 332-334): one O(n d) device reduction per set_data
    float ms[5];
    // fit_batch workspace (grow-only, freed with the handle): the matrices of one chunk + their vectors
    gpx::GrowBuf bw; int64_t bw_cap;        // bw_cap: matrices per chunk the block holds
    // block operators of the triangular solves (built once per factor, reused by every later solve)
    gpx::TrsvOps ops;
    // fit_batch_grad: X = L^-T and W = K^-1 of one matrix at a time + the reduction's partial sums (grow-only), and
    // the block operators of the row being differentiated
    gpx::GrowBuf gw; int64_t gw_cap;   // gw_cap: rows per lock-step gradient group the block holds
    gpx::TrsvOps bops;
    double *kii;          // device, n doubles from the first leave-one-out call on: diag(K^-1) of the CURRENT factor when
    bool have_kii;        // have_kii (cleared wherever `fitted` is, and by a new fit)
    hipStream_t st_ops;   // lazily created: where gpx_gp_fit builds `ops` while the factorisation is still running
    hipEvent_t ev_ops;
};

namespace gpx {
// x_finite / y_finite of the handle from its device arrays (one O(n d) reduction; synchronous)
int gp_scan_finite(gpx_gp *g);
// upload a host f64 array into a device buffer of dtype (gpx_gp.hip); returns when `src` may be reused
int upload_f64(int dtype, void *dst, const double *src, int64_t count, hipStream_t st);
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
}

// every gpx_gp_* entry: the handle's device becomes current for the duration of the call, and the handle's stream takes
// its turn among the streams this host thread drives (StreamTurn, gpx_mem.h); with GPX_ROCTX=1 the call is a roctx range
#define GP_ENTER(g)                                                          \
    GPX_ARG((g) != nullptr, "gp is NULL");                                   \
    gpx::tune_refresh();                                                     \
    gpx::DeviceGuard guard__((g)->device);                                   \
    if (guard__.rc != GPX_OK) return guard__.rc;                             \
    gpx::StreamTurn turn__((g)->st);                                         \
    gpx::RoctxRange api_range__(__func__)

