// gpx_gp.hip -- the fitted-GP device handle and the host-pointer drop-in entry points.
//
// gpx_gp_t keeps one GP resident in HBM and mirrors the memoised properties of
// the reference's gp.GP (gp/gp.py:242-396): Kxx (built lower, + s^2 on the
// diagonal) -> Lxx (in place) -> inv_Kxx_y -> logdet / y^T alpha -> log_lh, then
// posterior mean / covariance (gp/gp.py:574-625).  Data layout in HBM:
//   x      (n, d)  row-major, dtype T
//   y      (n,)
//   A      (n, lda) row-major, lda = round_up(n, 16): lower triangle holds K, then L
//   alpha  (n,)    K^-1 y
//   t0,t1  (n,)    solve scratch
//   scal   GpScal (gpx_gp_internal.h): logdet, y^T alpha, the non-finite flags, potrf's info
#include "gpx_small.h"
#include <cmath>
#include <vector>

#include "gpx_gp_internal.h"

namespace gpx {

// ---- the staging pair: host float64 <-> device arrays of a handle's dtype ---------------------------------------------------
// The conversions are element maps (gpx_small.h); (T)double rounds to nearest.
// a (rows x cols) block of float64 from host to device or back: a vector by a plain copy, a matrix by a pitched one -- also
// where both sides are dense (n = 8192: the plain copy of 512 MiB took 9.50 ms, the pitched one 9.35)
static int copy_rows(void *dst, int64_t ldd, const void *src, int64_t lds, int64_t rows, int64_t cols, hipMemcpyKind kind, hipStream_t st)
{
    if (rows == 1) GPX_HIP(hipMemcpyAsync(dst, src, (size_t)cols * 8, kind, st));
    else GPX_HIP(hipMemcpy2DAsync(dst, (size_t)ldd * 8, src, (size_t)lds * 8, (size_t)cols * 8, (size_t)rows, kind, st));
    return GPX_OK;
}

int upload_f64(int dtype, void *dst, int64_t ldd, const double *src, int64_t lds, int64_t rows, int64_t cols, hipStream_t st, DevBuf *stage)
{
    if (rows <= 0 || cols <= 0) return GPX_OK;
    if (dtype == GPX_F64) {
        GPX_TRY(copy_rows(dst, ldd, src, lds, rows, cols, hipMemcpyHostToDevice, st));
    } else {
        DevBuf mine;
        if (!stage) stage = &mine;
        if (!stage->p) GPX_TRY(stage->alloc((size_t)rows * cols * 8));
        GPX_TRY(copy_rows(stage->p, cols, src, lds, rows, cols, hipMemcpyHostToDevice, st));
        const double *src64 = (const double *)stage->p;
        float *dst32 = (float *)dst;
        GPX_TRY(map_rows(rows, cols, st, [=] __device__(int64_t r, int64_t c) { dst32[r * ldd + c] = (float)src64[r * cols + c]; }));
    }
    GPX_HIP(hipStreamSynchronize(st));
    return GPX_OK;
}

int download_f64(int dtype, double *dst, int64_t ldh, const void *src, int64_t lds, int64_t rows, int64_t cols, int lower_only,
                 hipStream_t st)
{
    if (rows <= 0 || cols <= 0) return GPX_OK;
    DevBuf buf;
    GPX_TRY(buf.alloc((size_t)rows * cols * 8));
    double *tmp = (double *)buf.p;
    GPX_TRY(by_dtype(dtype, [&](auto t) {
        const decltype(t) *s = (const decltype(t) *)src;
        return map_rows(rows, cols, st, [=] __device__(int64_t r, int64_t c) {
            const double v = (double)s[r * lds + c];
            tmp[r * cols + c] = (lower_only && c > r) ? 0.0 : v;
        });
    }));
    GPX_TRY(copy_rows(dst, ldh, tmp, cols, rows, cols, hipMemcpyDeviceToHost, st));
    GPX_HIP(hipStreamSynchronize(st));
    return GPX_OK;
}

int kmat(int dtype, int kernel, int member, const void *x1, int64_t n, const void *x2, int64_t m,
         int d, const double *params, double diag_add, int tri, void *out, int64_t ld, hipStream_t st)
{
    return gpx_d_kmat(dtype, kernel, member, x1, n, x2, m, d, params, diag_add, tri, out, ld, (void *)st);
}

// ARD: the scaled points and the isotropic constants follow every change of x or of the widths
int gp_rescale(gpx_gp *g)
{
    if (g->kernel != GPX_KERNEL_GAUSSIAN_ARD || !g->have_data || !g->have_params) return GPX_OK;
    ard_iso(g->params, g->d, g->iso);
    return scale_points(g->dtype, g->x, g->n, g->d, g->params + 1, g->xs, g->st);
}

// test points of a call: uploaded in the handle's dtype and, for the ARD family, scaled like the training points
static int upload_points(gpx_gp *g, void *dst, const double *xo, int64_t m)
{
    GPX_TRY(upload_f64(g->dtype, dst, m * g->d, xo, m * g->d, 1, m * g->d, g->st));
    if (g->kernel == GPX_KERNEL_GAUSSIAN_ARD) GPX_TRY(scale_points(g->dtype, dst, m, g->d, g->params + 1, dst, g->st));
    return GPX_OK;
}

int gp_read_scal(gpx_gp *g, GpScal *host)
{
    GPX_HIP(hipMemcpyAsync(host, g->scal, sizeof(GpScal), hipMemcpyDeviceToHost, g->st));
    GPX_HIP(hipStreamSynchronize(g->st));
    return check_internal_info(host->info);
}

int gp_need_factor(gpx_gp *g, const char *what_for)
{
    GpScal sc;
    GPX_TRY(gp_read_scal(g, &sc));
    if (sc.info != 0) { set_error("Kxx is not positive definite (info = %d): there is no factor %s", sc.info, what_for); return GPX_ERR_ARG; }
    return GPX_OK;
}

int check_internal_info(int info)
{
    if (info >= 0) return GPX_OK;
    set_error("internal failure inside the factorisation (info = %d: a hand-off between workgroups of the resident "
              "panel kernel timed out); the factor is not valid -- this is NOT a statement about the matrix", info);
    return GPX_ERR_INTERNAL;
}

int gp_finish_fit(gpx_gp *g, bool rhs_is_row_n, int *info)
{
    const size_t es = esize(g->dtype);
    hipStream_t st = g->st;
    // inv_Kxx_y = cho_solve((L, True), y) (gp/gp.py:332-334)
    if (rhs_is_row_n) {
        GPX_TRY(trsv_lower(g->dtype, g->A, g->n, g->lda, (char *)g->A + (size_t)g->n * g->lda * es, g->alpha, 1, st, nullptr, &g->ops));
    } else {
        GPX_HIP(hipMemcpyAsync(g->t0, g->y, (size_t)g->n * es, hipMemcpyDeviceToDevice, st));
        GPX_TRY(trsv_lower(g->dtype, g->A, g->n, g->lda, g->t0, g->t1, 0, st, nullptr, &g->ops));
        GPX_TRY(trsv_lower(g->dtype, g->A, g->n, g->lda, g->t1, g->alpha, 1, st, nullptr, &g->ops));
    }
    GPX_HIP(hipEventRecord(g->ev[3], st));
    // logdet (replaces slogdet(K), gp_c.pyx:21) and y^T alpha (gp_c.pyx:26)
    GPX_TRY(logdet_chol(g->dtype, g->A, g->n, g->lda, &g->scal->logdet, st));
    GPX_TRY(dot(g->dtype, g->y, g->alpha, g->n, &g->scal->yta, st));
    GPX_HIP(hipEventRecord(g->ev[4], st));
    g->fitted = true;
    if (info) {
        GPX_HIP(hipMemcpyAsync(info, &g->scal->info, sizeof(int), hipMemcpyDeviceToHost, st));
        GPX_HIP(hipStreamSynchronize(st));
        GPX_TRY(check_internal_info(*info));
    }
    return GPX_OK;
}

// flag[0] |= 1 when v holds a NaN or an infinity (scipy's asarray_chkfinite on the device, O(n))
template <typename T>
__global__ void nonfinite_kernel(const T *__restrict__ v, int64_t n, int *__restrict__ flag)
{
    bool bad = false;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
        bad = bad || !isfinite(v[i]);
    if (__any(bad) && (threadIdx.x & 63) == 0) atomicOr(flag, 1);
}

// x_finite / y_finite of the handle from its device arrays (synchronous)
int gp_scan_finite(gpx_gp *g)
{
    int *flags = &g->scal->x_bad;                          // x_bad, y_bad
    GPX_HIP(hipMemsetAsync(flags, 0, 2 * sizeof(int), g->st));
    const int64_t nx = g->n * g->d, ny = g->n;
    const unsigned bx = (unsigned)std::min<int64_t>(cdiv(nx, 256), 1024), by = (unsigned)std::min<int64_t>(cdiv(ny, 256), 1024);
    GPX_TRY(by_dtype(g->dtype, [&](auto t) {
        using T = decltype(t);
        hipLaunchKernelGGL((nonfinite_kernel<T>), dim3(bx), dim3(256), 0, g->st, (const T *)g->x, nx, flags);
        hipLaunchKernelGGL((nonfinite_kernel<T>), dim3(by), dim3(256), 0, g->st, (const T *)g->y, ny, flags + 1);
        GPX_LAUNCH_CHECK();
        return GPX_OK;
    }));
    int h[2] = {0, 0};
    GPX_HIP(hipMemcpyAsync(h, flags, sizeof(h), hipMemcpyDeviceToHost, g->st));
    GPX_HIP(hipStreamSynchronize(g->st));
    g->x_finite = h[0] == 0; g->y_finite = h[1] == 0;
    return GPX_OK;
}

// Would K(x, x) + s^2 I hold only finite numbers for finite x?  The kernel's value at r = 0 and at r = 1 in the
// host's double arithmetic: a NaN or infinite parameter (the reference's setters let both through:
// gp/kernels/gaussian.py:62-69 only reject values < EPS, gp/gp.py:192-193 only s < 0) shows up there.
// The kernel's value at r = 0 (plus s^2) and at r = 1, evaluated in the arithmetic the build will use: an fp32 handle
// whose h^2 exceeds FLT_MAX builds an infinite K although the constants are finite in double.
template <typename T>
static bool kernel_values_finite_t(int kernel, const double *p, double s)
{
    T k0, k1;
    if (kernel == GPX_KERNEL_GAUSSIAN) {
        const T c1 = (T)(-0.5 / (p[1] * p[1])), c2 = (T)(0.5 * sqrt(2.0 / M_PI) * p[0] * p[0] / p[1]);   // gaussian_c.pyx:27-28
        k0 = c2; k1 = c2 * (T)exp((double)c1);
    } else {
        const double sn = sin(0.5 / p[2]);                                                            // periodic_c.pyx:27-29
        k0 = (T)(p[0] * p[0]); k1 = k0 * (T)exp(-2.0 * sn * sn / (p[1] * p[1]));
    }
    const T diag = k0 + (T)(s * s);
    return std::isfinite(diag) && std::isfinite(k1);
}
bool kernel_values_finite(int kernel, const double *p, double s, int dtype)
{
    return dtype == GPX_F32 ? kernel_values_finite_t<float>(kernel, p, s) : kernel_values_finite_t<double>(kernel, p, s);
}

// ---- predictive variance: the row chunking -------------------------------------------------------------------------
// Rows per chunk without an explicit request: capped, because a chunk beyond a few thousand rows buys nothing (the TRSM's
// far updates already fill the chip; DESIGN 4 has the measurement behind the figure) and costs HBM.
constexpr int64_t VAR_CHUNK_ALIGN = 128, VAR_CHUNK_CAP = 4096;

// One chunk's device memory: the rows x lda chunk of Kxox that is solved in place, and the rows x TRSV_OPS_BLOCK block the
// operator route of the solve stages its in-block product in.  (xo and the result are O(m d) and O(m): not chunked.)
int var_plan(int dtype, int64_t n, int64_t m, int64_t chunk_rows, size_t free_bytes, int64_t *rows, int64_t *chunks, size_t *bytes)
{
    if (!(dtype == GPX_F64 || dtype == GPX_F32)) { set_error("var plan: dtype must be GPX_F64 or GPX_F32"); return GPX_ERR_ARG; }
    if (n < 1 || m < 0) { set_error("var plan: need n >= 1 and m >= 0"); return GPX_ERR_ARG; }
    if (chunk_rows < 0 || chunk_rows % VAR_CHUNK_ALIGN != 0) {
        set_error("var plan: chunk_rows must be 0 (automatic) or a multiple of %d (got %lld)", (int)VAR_CHUNK_ALIGN, (long long)chunk_rows);
        return GPX_ERR_ARG;
    }
    const size_t per_row = (size_t)(round_up(n, 16) + TRSV_OPS_BLOCK) * esize(dtype), budget = free_bytes / 4;
    const int64_t fit = (int64_t)std::min<size_t>(budget / per_row, (size_t)1 << 40) / VAR_CHUNK_ALIGN * VAR_CHUNK_ALIGN;
    if (fit < VAR_CHUNK_ALIGN) {
        set_error("var plan: not even %d rows of %lld columns fit a quarter of the free device memory (%zu bytes free)",
                  (int)VAR_CHUNK_ALIGN, (long long)n, free_bytes);
        return GPX_ERR_NOMEM;
    }
    int64_t r = chunk_rows ? chunk_rows : std::min(fit, VAR_CHUNK_CAP);
    if (m > 0 && m <= r) r = m;                            // one chunk: exactly the rows there are
    if ((size_t)r * per_row > budget) {
        set_error("var plan: chunk_rows = %lld needs %zu bytes, more than a quarter of the free device memory (%zu bytes free)",
                  (long long)chunk_rows, (size_t)r * per_row, free_bytes);
        return GPX_ERR_NOMEM;
    }
    if (rows) *rows = r;
    if (chunks) *chunks = cdiv(m, r);
    if (bytes) *bytes = (size_t)r * per_row;
    return GPX_OK;
}

// The row chunks of one call and their buffer: gpx_gp_var / var_from_K / var_grad over the test points, the leave-one-out
// sweep over the rows of the identity.  init refuses a bad chunk_rows in the caller's name (`who`), then -- m = 0: nothing to
// do, nothing allocated -- sizes the chunks from the free device memory (var_plan) and allocates X, rows x lda in g's dtype.
struct RowChunks {
    int64_t m = 0, rows = 0, chunks = 0;
    DevBuf X;
    int init(gpx_gp *g, int64_t m_, int64_t chunk_rows, const char *who)
    {
        if (chunk_rows < 0 || chunk_rows % VAR_CHUNK_ALIGN != 0) {
            set_error("%s: chunk_rows must be 0 (automatic) or a multiple of 128", who);
            return GPX_ERR_ARG;
        }
        m = m_;
        if (m == 0) return GPX_OK;
        size_t freeb = 0, totalb = 0;
        GPX_HIP(hipMemGetInfo(&freeb, &totalb));
        GPX_TRY(var_plan(g->dtype, g->n, m, chunk_rows, freeb, &rows, &chunks, nullptr));
        return X.alloc((size_t)rows * g->lda * esize(g->dtype));
    }
    int64_t r0(int64_t c) const { return c * rows; }                        // first row of chunk c
    int64_t rc(int64_t c) const { return std::min(rows, m - c * rows); }    // ... and how many it has
};

// The posterior covariance at m test points, left on the device:  C (m x m, ldc) = Kxoxo - V^T V,  V^T = Kxox L^-T
// (gp/gp.py:622-625 without K^-1).  xo: the test points (built-in families), or Kxox / Kxoxo: the caller's matrices (plugin
// kernels).  mean_dev (may be null; m elements, handle dtype): the posterior mean at the same points, as gpx_gp_mean /
// gpx_gp_mean_from_K compute it -- from Kxox before the sweep overwrites it.  Everything is enqueued on the handle's stream.
struct CovBlock { DevBuf dxo, X, C; int64_t ldc = 0; };
static int gp_cov_device(gpx_gp *g, const double *xo, const double *Kxox, const double *Kxoxo, int64_t m, CovBlock *b, void *mean_dev)
{
    const size_t es = esize(g->dtype);
    const int64_t n = g->n, ldx = g->lda, ldc = round_up(m, 16);
    b->ldc = ldc;
    if (xo) GPX_TRY(b->dxo.alloc((size_t)m * g->d * es));
    GPX_TRY(b->X.alloc((size_t)m * ldx * es));
    GPX_TRY(b->C.alloc((size_t)m * ldc * es));
    if (xo) {
        GPX_TRY(upload_points(g, b->dxo.p, xo, m));
        const GpView v = gp_view(g);
        if (mean_dev)
            GPX_TRY(gpx_d_mean(g->dtype, v.kernel, b->dxo.p, m, v.x, n, g->d, v.params, g->alpha, mean_dev, (void *)g->st));
        GPX_TRY(kmat(g->dtype, v.kernel, GPX_K, b->dxo.p, m, v.x, n, g->d, v.params, 0.0, GPX_FULL, b->X.p, ldx, g->st));
        GPX_TRY(trsm_right_lt(g->dtype, g->A, n, g->lda, b->X.p, m, ldx, g->st, 0, &g->ops));
        GPX_TRY(kmat(g->dtype, v.kernel, GPX_K, b->dxo.p, m, b->dxo.p, m, g->d, v.params, 0.0, GPX_FULL, b->C.p, ldc, g->st));
    } else {
        GPX_TRY(upload_f64(g->dtype, b->X.p, ldx, Kxox, n, m, n, g->st));
        GPX_TRY(upload_f64(g->dtype, b->C.p, ldc, Kxoxo, m, m, m, g->st));
        if (mean_dev) {
            GPX_HIP(hipMemsetAsync(mean_dev, 0, (size_t)m * es, g->st));
            GPX_TRY(gemm_nt(g->dtype, m, 1, n, b->X.p, ldx, g->alpha, ldx, mean_dev, 1, 1.0, GPX_FULL, 0, 0, g->st));
        }
        GPX_TRY(trsm_right_lt(g->dtype, g->A, n, g->lda, b->X.p, m, ldx, g->st, 0, &g->ops));
    }
    return gemm_nt(g->dtype, m, m, n, b->X.p, ldx, b->X.p, ldx, b->C.p, ldc, -1.0, GPX_FULL, 0, 0, g->st);
}

// k(0) of the handle's family from its parameters: the prior variance the automatic jitter of gpx_gp_sample scales with
static double gp_prior_var(const gpx_gp *g)
{
    const GpView v = gp_view(g);
    if (v.kernel == GPX_KERNEL_PERIODIC) return v.params[0] * v.params[0];                // periodic_c.pyx:30 at distance zero
    return 0.5 * sqrt(2.0 / M_PI) * v.params[0] * v.params[0] / v.params[1];              // gaussian_c.pyx:28
}

}  // namespace gpx

using namespace gpx;

extern "C" {

// ------------------------------------------------------------- the handle --
int gpx_gp_create(gpx_gp_t **out, int dtype, int kernel, int64_t n, int d)
{
    GPX_TRY(ensure_device());
    GPX_ARG(out, "gp is NULL");
    *out = nullptr;
    GPX_ARG(dtype == GPX_F64 || dtype == GPX_F32, "dtype must be GPX_F64 or GPX_F32");
    GPX_ARG(kernel == GPX_KERNEL_GAUSSIAN || kernel == GPX_KERNEL_PERIODIC || kernel == GPX_KERNEL_GAUSSIAN_ARD, "unknown kernel family");
    GPX_ARG(n >= 1 && d >= 1, "need n >= 1 and d >= 1");
    GPX_ARG(kernel != GPX_KERNEL_GAUSSIAN_ARD || d <= GPX_ARD_MAX_D, "the ARD family needs d <= GPX_ARD_MAX_D");
    gpx_gp *g = new gpx_gp();
    memset(g, 0, sizeof(*g));
    g->dtype = dtype; g->kernel = kernel; g->n = n; g->d = d;
    if (hipGetDevice(&g->device) != hipSuccess) { (void)hipGetLastError(); g->device = 0; }
    g->nparams = nparams_of(kernel, d);
    g->lda = round_up(n, 16);
    const size_t es = esize(dtype);
    int rc = GPX_OK;
    hipError_t e;
#define GP_ALLOC(field, bytes) if (rc == GPX_OK) rc = dev_alloc((void **)&g->field, (bytes), "hipMalloc " #field)
    GP_ALLOC(x, (size_t)n * d * es);
    if (kernel == GPX_KERNEL_GAUSSIAN_ARD) GP_ALLOC(xs, (size_t)n * d * es);
    GP_ALLOC(y, (size_t)n * es);
    GP_ALLOC(A, (size_t)(n + 1) * g->lda * es);          // (+ one row: the right-hand side rides along in the factorisation)
    GP_ALLOC(alpha, (size_t)n * es);
    GP_ALLOC(t0, (size_t)n * es);
    GP_ALLOC(t1, (size_t)n * es);
    GP_ALLOC(scal, 4 * sizeof(double));
#undef GP_ALLOC
    if (rc == GPX_OK) {
        e = hipStreamCreateWithFlags(&g->st, hipStreamNonBlocking);
        if (e != hipSuccess) rc = hip_fail(e, "hipStreamCreate", __FILE__, __LINE__);
    }
    for (int i = 0; i < 6 && rc == GPX_OK; ++i) {
        e = hipEventCreate(&g->ev[i]);
        if (e != hipSuccess) rc = hip_fail(e, "hipEventCreate", __FILE__, __LINE__);
    }
    if (rc != GPX_OK) { gpx_gp_destroy(g); return rc; }
    *out = g;
    return GPX_OK;
}

int gpx_gp_destroy(gpx_gp_t *g)
{
    if (!g) return GPX_OK;
    gpx::DeviceGuard guard__(g->device);
    if (g->st) (void)hipStreamSynchronize(g->st);
    stream_epoch_bump();                                       // (StreamTurn: a later stream at this one's address is a different stream)
    if (g->st_ops) { (void)hipStreamSynchronize(g->st_ops); (void)hipStreamDestroy(g->st_ops); }
    if (g->ev_ops) (void)hipEventDestroy(g->ev_ops);
    for (void *b : {g->x, g->xs, g->y, g->A, g->alpha, g->t0, g->t1, (void *)g->scal, (void *)g->kii}) dev_free(b);    // gpx_gp_create's fixed-size fields, and kii (n doubles, on first use)
    for (GrowBuf *b : {&g->bw, &g->gw, &g->ops.mem, &g->bops.mem}) b->release();
    for (int i = 0; i < 6; ++i) if (g->ev[i]) (void)hipEventDestroy(g->ev[i]);
    if (g->st) (void)hipStreamDestroy(g->st);
    delete g;
    return GPX_OK;
}

int gpx_gp_set_data(gpx_gp_t *g, const double *x, const double *y)
{
    GP_ENTER(g);
    GPX_ARG(g && x && y, "NULL argument");
    GPX_TRY(upload_f64(g->dtype, g->x, g->n * g->d, x, g->n * g->d, 1, g->n * g->d, g->st));
    GPX_TRY(upload_f64(g->dtype, g->y, g->n, y, g->n, 1, g->n, g->st));
    g->have_data = true; gp_unfit(g);
    GPX_TRY(gp_rescale(g));
    return gp_scan_finite(g);
}

int gpx_gp_set_data_device(gpx_gp_t *g, const void *x_dev, const void *y_dev)
{
    GP_ENTER(g);
    GPX_ARG(g && x_dev && y_dev, "NULL argument");
    const size_t es = esize(g->dtype);
    GPX_HIP(hipMemcpyAsync(g->x, x_dev, (size_t)g->n * g->d * es, hipMemcpyDeviceToDevice, g->st));
    GPX_HIP(hipMemcpyAsync(g->y, y_dev, (size_t)g->n * es, hipMemcpyDeviceToDevice, g->st));
    GPX_HIP(hipStreamSynchronize(g->st));      // the caller may free or overwrite the sources on return
    g->have_data = true; gp_unfit(g);
    GPX_TRY(gp_rescale(g));
    return gp_scan_finite(g);
}

int gpx_gp_set_params(gpx_gp_t *g, const double *params, double s)
{
    GP_ENTER(g);
    GPX_ARG(g && params, "NULL argument");
    GPX_ARG(!(s < 0), "invalid value for s");                  // gp/gp.py:192-193 (`val < 0`: a NaN passes, as in the reference; gpx_gp_fit then rejects it as non-finite)
    for (int i = 0; i < g->nparams; ++i) g->params[i] = params[i];
    g->s = s;
    g->have_params = true; g->have_K = false; gp_unfit(g);
    return gp_rescale(g);
}

int gpx_gp_get_params(gpx_gp_t *g, double *params, int cap, int *count)
{
    GP_ENTER(g);
    GPX_ARG(g->have_params, "no kernel parameters in the handle");
    GPX_ARG(cap >= 0 && (cap == 0 || params), "bad arguments");
    if (count) *count = g->nparams;
    for (int i = 0; i < g->nparams && i < cap; ++i) params[i] = g->params[i];
    return GPX_OK;
}

int gpx_gp_set_K(gpx_gp_t *g, const double *Kxx, int64_t ld)
{
    GP_ENTER(g);
    GPX_ARG(g && Kxx && ld >= g->n, "bad arguments");
    GPX_TRY(upload_f64(g->dtype, g->A, g->lda, Kxx, ld, g->n, g->n, g->st));
    g->have_K = true; gp_unfit(g);
    return GPX_OK;
}

// The block operators of the triangular solves (csrc/gpx_solve.hip: W_k = inv(L_kk) and its products with the neighbour
// blocks, 512 columns a block) need nothing but the block columns of L up to their own.  potrf() reports its progress
// (PotrfHook), and every `group` finished blocks their operators are built on a stream of their own, beside the
// rest of the factorisation: when it ends only the last group is still to do, and the solves take the operator route --
// one launch per block with no chain inside it -- at every size (n = 8192: backward solve 0.53 -> see DESIGN 3.3).
struct OpsAhead { gpx_gp *g; int64_t group, last; };
static int ops_ahead_step(void *user, int64_t cols_done, hipEvent_t panel_done)
{
    OpsAhead *o = (OpsAhead *)user;
    gpx_gp *g = o->g;
    const int64_t ready = std::min(trsv_ops_nblocks(cols_done), o->last);   // (the trailing blocks are left to the sweep's own steps)
    if (ready - g->ops.built < o->group) return GPX_OK;
    GPX_HIP(hipStreamWaitEvent(g->st_ops, panel_done, 0));
    return trsv_ops_build_upto(g->dtype, g->A, g->n, g->lda, &g->ops, ready, g->st_ops);
}

int gpx_gp_fit(gpx_gp_t *g, int *info)
{
    GP_ENTER(g);
    GPX_ARG(g, "gp is NULL");
    GPX_ARG(g->have_data && (g->have_params || g->have_K),
            "set_data and set_params (or set_K) must be called before fit");
    // scipy.linalg.cholesky(Kxx, check_finite=True), gp/gp.py:294: a kernel matrix with NaN / inf entries is a
    // ValueError, not "not positive definite".  K is finite iff x, the kernel's constants and s^2 are.
    const GpView v = gp_view(g);
    if (!g->have_K && (!g->x_finite || !kernel_values_finite(v.kernel, v.params, g->s, g->dtype))) {
        set_error("%s (%s)", NONFINITE_MSG, g->x_finite ? "kernel parameters or s" : "x");
        return GPX_ERR_ARG;
    }
    const size_t es = esize(g->dtype);
    hipStream_t st = g->st;
    GPX_HIP(hipEventRecord(g->ev[0], st));
    // Kxx = K(x, x) + s^2 I, lower triangle only (gp/gp.py:263-266)
    if (!g->have_K)
        GPX_TRY(kmat(g->dtype, v.kernel, GPX_K, v.x, g->n, v.x, g->n, g->d, v.params, g->s * g->s,
                     GPX_LOWER, g->A, g->lda, st));
    g->have_K = false;   // the factor overwrites it
    g->have_kii = false; // ... and diag(K^-1) went with the factor before
    GPX_HIP(hipEventRecord(g->ev[1], st));
    // Lxx (gp/gp.py:294), in place
    // Small and mid sizes: y rides along as row n of the matrix -- every panel substitutes it, every update reduces it,
    // exactly what the forward solve L t = y would do afterwards -- so only the backward solve is left (n = 8192: the
    // two solves were 1.0 ms of an 8 ms fit).  At large n the extra row of tiles in every update costs what it saves.
    const int64_t ride_max = tune().fit_ride_max;
    const bool ride = g->n <= ride_max;
    route_hit(ride ? RT_FIT_RIDE : RT_FIT_TWO_SOLVES);
    if (ride) GPX_HIP(hipMemcpyAsync((char *)g->A + (size_t)g->n * g->lda * es, g->y, (size_t)g->n * es, hipMemcpyDeviceToDevice, st));
    g->ops.invalidate();                                  // a new factor: its block operators are rebuilt once
    const bool ahead = tune().fit_ops_ahead != 0 && g->n >= tune().fit_ops_ahead_min &&
                       trsv_ops_ahead_ok(g->dtype, g->A, g->n, g->lda);
    // ONE instalment, when all but the last `tail` blocks are final: the build is a chain of ~11 launches batched over its
    // blocks (~0.6 ms whatever their number), so instalments of 4 blocks cost the factorisation what the solve saves
    // (n = 8192: fit 6.71 -> 6.73 ms with groups of 4, 6.62 with one; n = 12288: 15.57 -> 15.04; n = 4096: no gain), and
    // the last blocks' operators would only be waited for: the backward sweep takes those blocks by steps
    const int64_t nfull = trsv_ops_nblocks(g->n), tail = tune().fit_ops_tail;
    const int64_t group = std::max<int64_t>(1, std::min(nfull, nfull - tail));
    OpsAhead oa = {g, group, std::max<int64_t>(0, nfull - tail)};
    PotrfHook hook = {ops_ahead_step, &oa};
    if (ahead) {
        if (!g->st_ops) {
            int least = 0, greatest = 0;
            GPX_HIP(hipDeviceGetStreamPriorityRange(&least, &greatest));
            GPX_HIP(hipStreamCreateWithPriority(&g->st_ops, hipStreamNonBlocking, least));
            GPX_HIP(hipEventCreateWithFlags(&g->ev_ops, hipEventDisableTiming));
        }
        GPX_TRY(g->ops.mem.reserve(trsv_ops_bytes(g->dtype, g->n), st));   // (here, not inside the factorisation's launch loop)
        // (the operator buffer may still be read by solves of the factor before this one, queued on st)
        GPX_TRY(order(g->ev_ops, st, g->st_ops));
    }
    GPX_TRY(potrf(g->dtype, g->A, g->n, g->lda, &g->scal->info, st, nullptr, ride ? 1 : 0, /*may_block=*/true, ahead ? &hook : nullptr));
    if (ahead) {
        // the solves wait for the operator stream.  The backward sweep takes the blocks that have no operators yet by
        // steps; a forward sweep (n > ride_max) and every later solve of this factor complete the set first (trsv_lower)
        GPX_TRY(order(g->ev_ops, g->st_ops, st));
        if (g->ops.built > 0) route_hit(RT_FIT_OPS_AHEAD);
    }
    GPX_HIP(hipEventRecord(g->ev[2], st));
    return gp_finish_fit(g, ride, info);
}

static int gp_scalars(gpx_gp_t *g, double *logdet, double *yta, int *info)
{
    GP_ENTER(g);
    GPX_ARG(g && g->fitted, "gp is not fitted");
    GpScal sc;
    GPX_TRY(gp_read_scal(g, &sc));
    if (logdet) *logdet = sc.logdet;
    if (yta) *yta = sc.yta;
    if (info) *info = sc.info;
    return GPX_OK;
}

int gpx_gp_log_lh(gpx_gp_t *g, double *log_lh)
{
    GPX_ARG(log_lh, "log_lh is NULL");
    GPX_ARG(g, "gp is NULL");
    GP_NEED_FINITE_Y(g);                                  // cho_solve(..., check_finite=True), gp/gp.py:332-334
    double logdet, yta; int info;
    GPX_TRY(gp_scalars(g, &logdet, &yta, &info));
    // gp/gp.py:362-365 (LinAlgError -> -inf) and gp_c.pyx:22-29 (sign / MIN clamp)
    if (info != 0 || !(logdet >= GPX_MIN_LOG)) { *log_lh = -INFINITY; return GPX_OK; }
    const double data_fit = -0.5 * yta;
    const double complexity_penalty = -0.5 * logdet;
    const double constant = -0.5 * (double)g->n * log(2 * M_PI);
    *log_lh = data_fit + complexity_penalty + constant;
    return GPX_OK;
}

int gpx_gp_logdet(gpx_gp_t *g, double *logdet)
{
    GPX_ARG(logdet, "logdet is NULL");
    return gp_scalars(g, logdet, nullptr, nullptr);
}

int gpx_gp_info(gpx_gp_t *g, int *info)
{
    GPX_ARG(info, "info is NULL");
    return gp_scalars(g, nullptr, nullptr, info);
}

int gpx_gp_mean(gpx_gp_t *g, const double *xo, int64_t m, double *out)
{
    GP_ENTER(g);
    GPX_ARG(g && g->fitted, "gp is not fitted");
    GP_NEED_FINITE_Y(g);
    GPX_ARG(m >= 0 && (m == 0 || (xo && out)), "bad arguments");
    if (m == 0) return GPX_OK;
    const size_t es = esize(g->dtype);
    DevBuf dxo, dout;
    GPX_TRY(dxo.alloc((size_t)m * g->d * es));
    GPX_TRY(dout.alloc((size_t)m * es));
    GPX_TRY(upload_points(g, dxo.p, xo, m));
    const GpView v = gp_view(g);
    GPX_TRY(gpx_d_mean(g->dtype, v.kernel, dxo.p, m, v.x, g->n, g->d, v.params, g->alpha, dout.p,
                       (void *)g->st));
    return download_f64(g->dtype, out, m, dout.p, m, 1, m, 0, g->st);
}

int gpx_gp_cov(gpx_gp_t *g, const double *xo, int64_t m, double *out)
{
    GP_ENTER(g);
    GPX_ARG(g && g->fitted, "gp is not fitted");
    GPX_ARG(m >= 0 && (m == 0 || (xo && out)), "bad arguments");
    if (m == 0) return GPX_OK;
    CovBlock b;
    GPX_TRY(gp_cov_device(g, xo, nullptr, nullptr, m, &b, nullptr));
    return download_f64(g->dtype, out, m, b.C.p, b.ldc, m, m, 0, g->st);
}

int gpx_gp_mean_from_K(gpx_gp_t *g, const double *Kxox, int64_t m, double *out)
{
    GP_ENTER(g);
    GPX_ARG(g && g->fitted, "gp is not fitted");
    GP_NEED_FINITE_Y(g);
    GPX_ARG(m >= 0 && (m == 0 || (Kxox && out)), "bad arguments");
    if (m == 0) return GPX_OK;
    const size_t es = esize(g->dtype);
    const int64_t n = g->n, ldx = g->lda;
    DevBuf X, o;
    GPX_TRY(X.alloc((size_t)m * ldx * es));
    GPX_TRY(o.alloc((size_t)m * es));
    GPX_HIP(hipMemsetAsync(o.p, 0, (size_t)m * es, g->st));
    GPX_TRY(upload_f64(g->dtype, X.p, ldx, Kxox, n, m, n, g->st));
    GPX_TRY(gemm_nt(g->dtype, m, 1, n, X.p, ldx, g->alpha, ldx, o.p, 1, 1.0, GPX_FULL, 0, 0, g->st));
    return download_f64(g->dtype, out, m, o.p, m, 1, m, 0, g->st);
}

int gpx_gp_cov_from_K(gpx_gp_t *g, const double *Kxox, const double *Kxoxo, int64_t m, double *out)
{
    GP_ENTER(g);
    GPX_ARG(g && g->fitted, "gp is not fitted");
    GPX_ARG(m >= 0 && (m == 0 || (Kxox && Kxoxo && out)), "bad arguments");
    if (m == 0) return GPX_OK;
    CovBlock b;
    GPX_TRY(gp_cov_device(g, nullptr, Kxox, Kxoxo, m, &b, nullptr));
    return download_f64(g->dtype, out, m, b.C.p, b.ldc, m, m, 0, g->st);
}

// Joint posterior samples at m test points: the covariance block of gpx_gp_cov (the very matrix it would download), the
// mean of gpx_gp_mean, then mvn_sample (gpx_sample.hip) with stream 0: out (S x m) = 1 mean^T + Z Lc^T,
// Lc Lc^T = cov + (jitter [+ s^2]) I.  One download of S x m; nothing m x m leaves the device.
static int gp_sample_impl(gpx_gp *g, const double *xo, const double *Kxox, const double *Kxoxo, int64_t m, int64_t S, uint64_t seed,
                          int noise, double jitter, double *out, int *info)
{
    *info = 0;
    GPX_TRY(gp_need_factor(g, "to sample from"));
    route_hit(RT_SAMPLE);
    if (m == 0 || S == 0) return GPX_OK;
    const size_t es = esize(g->dtype);
    if (jitter < 0.0) jitter = sqrt(g->dtype == GPX_F64 ? 2.220446049250313e-16 : 1.1920928955078125e-07) * gp_prior_var(g);
    const double diag_add = jitter + (noise ? g->s * g->s : 0.0);
    GPX_ARG(diag_add <= 1.79769313486231570e308, "jitter must be finite");          // (NaN fails it too)
    const int64_t ldz = round_up(m, 16);
    CovBlock b;
    DevBuf mean, Z, smp, dinfo;
    GPX_TRY(mean.alloc((size_t)m * es));
    GPX_TRY(Z.alloc((size_t)S * ldz * es));
    GPX_TRY(smp.alloc((size_t)S * ldz * es));
    GPX_TRY(dinfo.alloc(sizeof(int)));
    GPX_TRY(gp_cov_device(g, xo, Kxox, Kxoxo, m, &b, mean.p));
    GPX_TRY(mvn_sample(g->dtype, b.C.p, m, b.ldc, mean.p, diag_add, S, seed, 0, Z.p, ldz, smp.p, ldz, (int *)dinfo.p, g->st));
    int host_info = 0;
    GPX_HIP(hipMemcpyAsync(&host_info, dinfo.p, sizeof(int), hipMemcpyDeviceToHost, g->st));
    GPX_HIP(hipStreamSynchronize(g->st));
    GPX_TRY(check_internal_info(host_info));
    *info = host_info;
    if (host_info != 0) return GPX_OK;                     // the caller's matrix, the caller's verdict: out is not written
    return download_f64(g->dtype, out, m, smp.p, ldz, S, m, 0, g->st);
}

int gpx_gp_sample(gpx_gp_t *g, const double *xo, int64_t m, int64_t S, uint64_t seed, int noise, double jitter, double *out, int *info)
{
    GP_ENTER(g);
    GPX_ARG(g->fitted && g->have_data && g->have_params, "gp is not fitted (from kernel parameters: a handle fitted from set_K samples with gpx_gp_sample_from_K)");
    GP_NEED_FINITE_Y(g);
    GPX_ARG(info, "info is NULL");
    GPX_ARG(m >= 0 && S >= 0 && (m == 0 || S == 0 || (xo && out)), "bad arguments");
    GPX_ARG(jitter == jitter, "jitter is NaN");
    return gp_sample_impl(g, xo, nullptr, nullptr, m, S, seed, noise, jitter, out, info);
}

int gpx_gp_sample_from_K(gpx_gp_t *g, const double *Kxox, const double *Kxoxo, int64_t m, int64_t S, uint64_t seed, int noise,
                         double jitter, double *out, int *info)
{
    GP_ENTER(g);
    GPX_ARG(g->fitted, "gp is not fitted");
    GP_NEED_FINITE_Y(g);
    GPX_ARG(info, "info is NULL");
    GPX_ARG(m >= 0 && S >= 0 && (m == 0 || S == 0 || (Kxox && Kxoxo && out)), "bad arguments");
    GPX_ARG(jitter >= 0.0, "jitter must be >= 0 (the automatic value needs kernel parameters: gpx_gp_sample)");
    return gp_sample_impl(g, nullptr, Kxox, Kxoxo, m, S, seed, noise, jitter, out, info);
}

// Predictive variance, diag of RW06 eq. 2.24, in row chunks: X = K(xo_c, x) (or the caller's rows of Kxox), X <- X L^-T
// where gpx_gp_cov runs it (the same operators), out_c = kdiag_c - rowsumsq(X).  One chunk buffer, one double[m] of results,
// one download; nothing m x m exists anywhere.  Kxox != NULL: the plugin form (kdiag is then the caller's too).
static int gp_var_impl(gpx_gp *g, const double *xo, const double *Kxox, const double *kdiag, const RowChunks &ch, double *out)
{
    const size_t es = esize(g->dtype);
    const int64_t n = g->n, ldx = g->lda, m = ch.m;
    const DevBuf &X = ch.X;
    DevBuf dxo, dvar, dk, stage;                           // stage: upload_f64's, one for all chunks
    GPX_TRY(dvar.alloc((size_t)m * sizeof(double)));
    if (Kxox) {
        GPX_TRY(dk.alloc((size_t)m * sizeof(double)));
        GPX_HIP(hipMemcpyAsync(dk.p, kdiag, (size_t)m * sizeof(double), hipMemcpyHostToDevice, g->st));
    } else {
        GPX_TRY(dxo.alloc((size_t)m * g->d * es));
        GPX_TRY(upload_points(g, dxo.p, xo, m));
    }
    const GpView v = gp_view(g);
    for (int64_t c = 0; c < ch.chunks; ++c) {
        const int64_t r0 = ch.r0(c), rc = ch.rc(c);
        route_hit(RT_VAR_CHUNK);
        const void *xo_c = nullptr;
        if (!Kxox) {
            xo_c = (const char *)dxo.p + (size_t)r0 * g->d * es;
            GPX_TRY(kmat(g->dtype, v.kernel, GPX_K, xo_c, rc, v.x, n, g->d, v.params, 0.0, GPX_FULL, X.p, ldx, g->st));
        } else {
            GPX_TRY(upload_f64(g->dtype, X.p, ldx, Kxox + r0 * n, n, rc, n, g->st, &stage));
        }
        GPX_TRY(trsm_right_lt(g->dtype, g->A, n, g->lda, X.p, rc, ldx, g->st, 0, &g->ops));
        GPX_TRY(var_rows(g->dtype, v.kernel, X.p, rc, n, ldx, xo_c, g->d, v.params, Kxox ? (const double *)dk.p + r0 : nullptr, 0,
                         (double *)dvar.p + r0, g->st));
    }
    GPX_HIP(hipMemcpyAsync(out, dvar.p, (size_t)m * sizeof(double), hipMemcpyDeviceToHost, g->st));
    GPX_HIP(hipStreamSynchronize(g->st));
    return GPX_OK;
}

int gpx_gp_var(gpx_gp_t *g, const double *xo, int64_t m, int64_t chunk_rows, double *out)
{
    GP_ENTER(g);
    GPX_ARG(g && g->fitted, "gp is not fitted");
    GPX_ARG(m >= 0 && (m == 0 || (xo && out)), "bad arguments");
    RowChunks ch;
    GPX_TRY(ch.init(g, m, chunk_rows, __func__));
    if (m == 0) return GPX_OK;
    return gp_var_impl(g, xo, nullptr, nullptr, ch, out);
}

int gpx_gp_var_from_K(gpx_gp_t *g, const double *Kxox, const double *kdiag, int64_t m, int64_t chunk_rows, double *out)
{
    GP_ENTER(g);
    GPX_ARG(g && g->fitted, "gp is not fitted");
    GPX_ARG(m >= 0 && (m == 0 || (Kxox && kdiag && out)), "bad arguments");
    RowChunks ch;
    GPX_TRY(ch.init(g, m, chunk_rows, __func__));
    if (m == 0) return GPX_OK;
    return gp_var_impl(g, nullptr, Kxox, kdiag, ch, out);
}

// Input-space gradients of the prediction.  The mean's is one fused pass with w = alpha.  The variance's,
//   dvar_i/dxo_i = -2 sum_j beta_ij dk(xo_i, x_j)/dxo_i,   beta_i = K^-1 k_i = L^-T (L^-1 k_i),
// goes through gpx_gp_var's chunks and buffer: X = K(xo_c, x), X <- X L^-T (the variance falls out here: var_rows), X <- X L^-1
// (trsm_right_l, the handle's operators), then the same fused pass with w = X.  Nothing n x n beside the factor; one
// download at the end.  ARD: everything on the scaled points, column k of the result divided by w_k.
static const double *gp_col_div(const gpx_gp *g) { return g->kernel == GPX_KERNEL_GAUSSIAN_ARD ? g->params + 1 : nullptr; }

int gpx_gp_mean_grad(gpx_gp_t *g, const double *xo, int64_t m, double *grad)
{
    GP_ENTER(g);
    GPX_ARG(g && g->fitted, "gp is not fitted");
    GP_NEED_FINITE_Y(g);
    GPX_ARG(m >= 0 && (m == 0 || (xo && grad)), "bad arguments");
    if (m == 0) return GPX_OK;
    DevBuf dxo, dout;
    GPX_TRY(dxo.alloc((size_t)m * g->d * esize(g->dtype)));
    GPX_TRY(dout.alloc((size_t)m * g->d * sizeof(double)));
    GPX_TRY(upload_points(g, dxo.p, xo, m));
    const GpView v = gp_view(g);
    GPX_TRY(pred_grad(g->dtype, v.kernel, dxo.p, m, v.x, g->n, g->d, v.params, g->alpha, nullptr, 0, 1.0, gp_col_div(g),
                      (double *)dout.p, g->st));
    GPX_HIP(hipMemcpyAsync(grad, dout.p, (size_t)m * g->d * sizeof(double), hipMemcpyDeviceToHost, g->st));
    GPX_HIP(hipStreamSynchronize(g->st));
    return GPX_OK;
}

int gpx_gp_var_grad(gpx_gp_t *g, const double *xo, int64_t m, int64_t chunk_rows, double *var, double *grad)
{
    GP_ENTER(g);
    GPX_ARG(g && g->fitted, "gp is not fitted");
    GPX_ARG(m >= 0 && (m == 0 || (xo && grad)), "bad arguments");
    RowChunks ch;
    GPX_TRY(ch.init(g, m, chunk_rows, __func__));
    if (m == 0) return GPX_OK;
    const size_t es = esize(g->dtype);
    const int64_t n = g->n, ldx = g->lda, d = g->d;
    const DevBuf &X = ch.X;
    DevBuf dxo, dout;                                      // dout: grad (m, d) | var (m)
    GPX_TRY(dout.alloc((size_t)m * (d + 1) * sizeof(double)));
    GPX_TRY(dxo.alloc((size_t)m * d * es));
    GPX_TRY(upload_points(g, dxo.p, xo, m));
    double *dgrad = (double *)dout.p, *dvar = dgrad + m * d;
    const GpView v = gp_view(g);
    for (int64_t c = 0; c < ch.chunks; ++c) {
        const int64_t r0 = ch.r0(c), rc = ch.rc(c);
        route_hit(RT_GRAD_CHUNK);
        const void *xo_c = (const char *)dxo.p + (size_t)r0 * d * es;
        GPX_TRY(kmat(g->dtype, v.kernel, GPX_K, xo_c, rc, v.x, n, g->d, v.params, 0.0, GPX_FULL, X.p, ldx, g->st));
        GPX_TRY(trsm_right_lt(g->dtype, g->A, n, g->lda, X.p, rc, ldx, g->st, 0, &g->ops));
        if (var) GPX_TRY(var_rows(g->dtype, v.kernel, X.p, rc, n, ldx, xo_c, g->d, v.params, nullptr, 0, dvar + r0, g->st));
        GPX_TRY(trsm_right_l(g->dtype, g->A, n, g->lda, X.p, rc, ldx, g->st, &g->ops));
        GPX_TRY(pred_grad(g->dtype, v.kernel, xo_c, rc, v.x, n, g->d, v.params, nullptr, X.p, ldx, -2.0, gp_col_div(g),
                          dgrad + r0 * d, g->st));
    }
    GPX_HIP(hipMemcpyAsync(grad, dgrad, (size_t)m * d * sizeof(double), hipMemcpyDeviceToHost, g->st));
    if (var) GPX_HIP(hipMemcpyAsync(var, dvar, (size_t)m * sizeof(double), hipMemcpyDeviceToHost, g->st));
    GPX_HIP(hipStreamSynchronize(g->st));
    return GPX_OK;
}

// Leave-one-out, RW06 eq. 5.10 - 5.12: everything but diag(K^-1) is in HBM after a fit, and (K^-1)_ii = |L^-1 e_i|^2.  In row
// chunks of the identity (var_plan, as gpx_gp_var): X = E_c L^-T by the sweep that begins at the chunk's own column --
// L^-1 e_i is zero above row i -- then the row sums of squares (loo_rows).  n^3 / 3 flops, one chunk buffer, nothing n x n.
// The diagonal stays in the handle (g->kii) until the factor changes.  mean / var / logp (device, n doubles each; all or
// none): the per-point quantities are written by the same pass.
static int gp_loo_sweep(gpx_gp *g, const RowChunks &ch, double *mean, double *var, double *logp)
{
    const size_t es = esize(g->dtype);
    const int64_t n = g->n, ldx = g->lda;
    const DevBuf &X = ch.X;
    if (!g->kii) GPX_TRY(dev_alloc((void **)&g->kii, (size_t)n * sizeof(double), "hipMalloc kii"));
    for (int64_t c = 0; c < ch.chunks; ++c) {
        const int64_t c0 = ch.r0(c), rc = ch.rc(c);
        route_hit(RT_LOO_CHUNK);
        GPX_TRY(eye_rows(g->dtype, X.p, rc, ldx, c0, c0 / TRSV_OPS_BLOCK * TRSV_OPS_BLOCK, g->st));
        GPX_TRY(trsm_right_lt(g->dtype, g->A, n, g->lda, X.p, rc, ldx, g->st, 1, &g->ops, c0));
        GPX_TRY(loo_rows(g->dtype, X.p, rc, n, ldx, c0, mean ? (const char *)g->y + c0 * es : nullptr,
                         mean ? (const char *)g->alpha + c0 * es : nullptr, g->kii + c0, mean ? mean + c0 : nullptr,
                         mean ? var + c0 : nullptr, mean ? logp + c0 : nullptr, g->st));
    }
    g->have_kii = true;
    return GPX_OK;
}

// (both entry points: the sweep has no chunks when the diagonal is already in the handle, and a bad chunk_rows is refused
// before the factor is asked for)
int gpx_gp_inv_diag(gpx_gp_t *g, int64_t chunk_rows, double *out)
{
    GP_ENTER(g);
    GPX_ARG(g->fitted, "gp is not fitted");
    GPX_ARG(out, "out is NULL");
    RowChunks ch;
    GPX_TRY(ch.init(g, g->have_kii ? 0 : g->n, chunk_rows, __func__));
    GPX_TRY(gp_need_factor(g, "to take diag(K^-1) from"));
    if (!g->have_kii) GPX_TRY(gp_loo_sweep(g, ch, nullptr, nullptr, nullptr));
    GPX_HIP(hipMemcpyAsync(out, g->kii, (size_t)g->n * sizeof(double), hipMemcpyDeviceToHost, g->st));
    GPX_HIP(hipStreamSynchronize(g->st));
    return GPX_OK;
}

int gpx_gp_loo(gpx_gp_t *g, int64_t chunk_rows, double *mean, double *var, double *log_p, double *log_p_sum)
{
    GP_ENTER(g);
    GPX_ARG(g->fitted, "gp is not fitted");
    GP_NEED_FINITE_Y(g);
    RowChunks ch;
    GPX_TRY(ch.init(g, g->have_kii ? 0 : g->n, chunk_rows, __func__));
    GPX_TRY(gp_need_factor(g, "to take diag(K^-1) from"));
    const int64_t n = g->n;
    if (!mean && !var && !log_p && !log_p_sum) {           // nothing asked for: the diagonal, for the calls to come
        if (!g->have_kii) GPX_TRY(gp_loo_sweep(g, ch, nullptr, nullptr, nullptr));
        return GPX_OK;
    }
    DevBuf o;                                              // mean | var | logp | sum of logp
    GPX_TRY(o.alloc((size_t)(3 * n + 1) * sizeof(double)));
    double *dm = (double *)o.p, *dv = dm + n, *dl = dv + n, *ds = dl + n;
    if (!g->have_kii) GPX_TRY(gp_loo_sweep(g, ch, dm, dv, dl));
    else GPX_TRY(loo_points(g->dtype, g->kii, g->y, g->alpha, n, dm, dv, dl, g->st));
    GPX_TRY(sum_f64(dl, n, ds, g->st));                    // one workgroup, fixed order: not a host sum
    if (mean) GPX_HIP(hipMemcpyAsync(mean, dm, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, g->st));
    if (var) GPX_HIP(hipMemcpyAsync(var, dv, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, g->st));
    if (log_p) GPX_HIP(hipMemcpyAsync(log_p, dl, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, g->st));
    if (log_p_sum) GPX_HIP(hipMemcpyAsync(log_p_sum, ds, sizeof(double), hipMemcpyDeviceToHost, g->st));
    GPX_HIP(hipStreamSynchronize(g->st));
    return GPX_OK;
}

int gpx_debug_var_plan(int dtype, int64_t n, int64_t m, int64_t chunk_rows, size_t free_bytes,
                       int64_t *rows_per_chunk, int64_t *chunks, size_t *bytes_per_chunk)
{
    return var_plan(dtype, n, m, chunk_rows, free_bytes, rows_per_chunk, chunks, bytes_per_chunk);
}

int gpx_gp_get_Kxx(gpx_gp_t *g, double *out, int64_t ld)
{
    GP_ENTER(g);
    GPX_ARG(g && g->have_data && g->have_params && out && ld >= g->n, "bad arguments");
    const size_t es = esize(g->dtype);
    DevBuf K;
    GPX_TRY(K.alloc((size_t)g->n * g->lda * es));
    const GpView v = gp_view(g);
    GPX_TRY(kmat(g->dtype, v.kernel, GPX_K, v.x, g->n, v.x, g->n, g->d, v.params, g->s * g->s,
                 GPX_FULL, K.p, g->lda, g->st));
    return download_f64(g->dtype, out, ld, K.p, g->lda, g->n, g->n, 0, g->st);
}

int gpx_gp_get_Lxx(gpx_gp_t *g, double *out, int64_t ld)
{
    GP_ENTER(g);
    GPX_ARG(g && g->fitted && out && ld >= g->n, "bad arguments");
    return download_f64(g->dtype, out, ld, g->A, g->lda, g->n, g->n, 1, g->st);
}

int gpx_gp_get_alpha(gpx_gp_t *g, double *out)
{
    GP_ENTER(g);
    GPX_ARG(g && g->fitted && out, "bad arguments");
    GP_NEED_FINITE_Y(g);                                  // cho_solve(..., check_finite=True), gp/gp.py:332-334
    return download_f64(g->dtype, out, g->n, g->alpha, g->n, 1, g->n, 0, g->st);
}

int gpx_gp_get_inv_Kxx(gpx_gp_t *g, double *out, int64_t ld)
{
    GP_ENTER(g);
    GPX_ARG(g && g->fitted && out && ld >= g->n, "bad arguments");
    const size_t es = esize(g->dtype);
    const int64_t n = g->n, lda = g->lda;
    DevBuf X, C;
    GPX_TRY(X.alloc((size_t)n * lda * es));
    GPX_TRY(C.alloc((size_t)n * lda * es));
    GPX_TRY(inv_from_factor(g->dtype, g->A, n, lda, X.p, C.p, GPX_FULL, g->st, &g->ops));   // gp/gp.py:311-312
    return download_f64(g->dtype, out, ld, C.p, lda, n, n, 0, g->st);
}

// the reduction half of the gradient: W = K^-1 (lower triangle, n x ldw) is in HBM; one fused pass of (alpha alpha^T - W)
// against the kernel derivatives evaluated on the fly (gp_c.pyx:34-49).  Synchronises g->st.
// pts: the points that go with `params` -- g->x, or for the ARD family x / w for THESE widths (the handle's xs, a batch row's copy)
static int grad_reduce(gpx_gp *g, const void *pts, const void *alpha, const double *params, double s_noise, const void *W, int64_t ldw,
                       double *part, double *out)
{
    const int64_t n = g->n;
    double *aa = part + dloglh_partial_doubles(g->kernel, g->d);
    GPX_TRY(dot(g->dtype, alpha, alpha, n, aa, g->st));
    double S[GPX_ARD_MAX_D + 2], iso[2], ata = 0.0;    // ARD: S_0, S_1 .. S_d, tr W; otherwise [P0, P1, P2, tr W]
    GPX_TRY(tile_reduce(g->dtype, g->kernel, pts, n, g->d, reduce_params(g->kernel, g->d, params, iso), alpha, nullptr, W, ldw, part, S, g->st));
    GPX_HIP(hipMemcpyAsync(&ata, aa, sizeof(double), hipMemcpyDeviceToHost, g->st));
    GPX_HIP(hipStreamSynchronize(g->st));
    grad_from_sums(g->kernel, g->d, params, S, ata, s_noise, 0.5, out);
    return GPX_OK;
}

// d log_lh / d(kernel params..., s) from a factor L (n x n, lower, in HBM) and alpha = K^-1 y: X = L^-T by the blocked
// right-looking TRSM, W = K^-1 = X X^T (lower triangle, triangular k-loop) on the MFMA kernel, then ONE fused pass
// reduces (alpha alpha^T - W) against the kernel derivatives evaluated on the fly.  X, W: n x lda scratch; part:
// dloglh_partial_doubles() + 8 doubles; ops: the block operators of THIS factor (completed here).  Synchronises `g->st`.
static int grad_from_factor(gpx_gp *g, const void *pts, const void *L, int64_t lda, const void *alpha, const double *params, double s_noise,
                            void *X, void *W, double *part, TrsvOps *ops, double *out)
{
    GPX_TRY(inv_from_factor(g->dtype, L, g->n, lda, X, W, GPX_LOWER, g->st, ops));
    return grad_reduce(g, pts, alpha, params, s_noise, W, lda, part, out);
}

// Gradient of the log marginal likelihood w.r.t. (kernel params..., s), RW06 eq. 5.9
// (gp/gp.py:398-433 + gp_c.pyx:34-49): K^-1 is formed on the device (X = L^-T by the blocked
// right-looking TRSM, W = X X^T lower triangle on the MFMA kernel), then ONE fused pass
// reduces (alpha alpha^T - W) against the kernel derivatives evaluated on the fly.
int gpx_gp_dloglh_dtheta(gpx_gp_t *g, double *out)
{
    GP_ENTER(g);
    GPX_ARG(g && g->fitted && out, "bad arguments");
    GP_NEED_FINITE_Y(g);
    const size_t es = esize(g->dtype);
    const int64_t n = g->n, lda = g->lda;
    GpScal sc;
    GPX_TRY(gp_read_scal(g, &sc));
    if (sc.info != 0) {                                 // gp/gp.py:424-428: NaN when K is not PD
        for (int i = 0; i <= g->nparams; ++i) out[i] = NAN;
        return GPX_OK;
    }
    DevBuf X, W, part;
    GPX_TRY(X.alloc((size_t)n * lda * es));
    GPX_TRY(W.alloc((size_t)n * lda * es));
    GPX_TRY(part.alloc(dloglh_partial_doubles(g->kernel, g->d) * sizeof(double) + 64));
    return grad_from_factor(g, gp_view(g).x, g->A, lda, g->alpha, g->params, g->s, X.p, W.p, (double *)part.p, &g->ops, out);
}

// Batched ML-II step (BASELINE config 5; the reference's inner step "set params -> read log_lh",
// gp/gp.py:216-223,337-367, for a whole table of restarts): the kernel matrices of up to `B` parameter
// rows live in HBM side by side and are factored in LOCK-STEP -- every launch of the factorisation and
// of the solves covers all of them (grid dimension y / x = matrix index), so the chain of small
// dependent launches that bounds ONE n = 8192 factorisation is paid once per batch and the chip stays
// filled by the trailing updates of all matrices.  Chunked when B matrices do not fit in free HBM.
// loo != 0 (gpx_gp_fit_batch_loo): the criterion is the leave-one-out one.  The factorisation, the solves and the groups are
// the same; a group's K^-1 is formed whole (GPX_FULL), each row's vectors follow (loo_weights_vectors), the group's Y Y^T
// run in lock-step, and the row's value comes out of its gradient pass: `log_lh` and `dloglh` then hold L_LOO and its gradient.
static int fit_batch_impl(gpx_gp_t *g, const double *thetas, int64_t B, double *log_lh, double *dloglh, double *logdet_yta,
                          int *info, int loo = 0)
{
    GPX_ARG(g->have_data, "set_data must be called before fit_batch");
    GPX_ARG(B >= 0 && (B == 0 || (thetas && log_lh)), "bad arguments");
    if (B == 0) return GPX_OK;
    if (dloglh) {
        if (g->kernel == GPX_KERNEL_PERIODIC && g->d != 1) { set_error("periodic gradient needs d == 1"); return GPX_ERR_UNSUPPORTED; }
        // gradient scratch BEFORE the chunk size is taken from what is free: X = L^-T and W = K^-1 of a GROUP of up to 8 rows
        // at a time (the group's TRSM and SYRK run in lock-step: at n = 8192 one system's far update is 1 - 2 rounds of
        // tiles), as many as a sixth of free HBM holds, + their block operators
        const size_t nl = (size_t)g->n * g->lda * esize(g->dtype);
        const bool group_ok = trsm_ops_ok(g->dtype, g->A, g->n, g->lda);
        size_t freeg = 0, totalg = 0;
        GPX_HIP(hipMemGetInfo(&freeg, &totalg));
        const size_t per_row = 2 * nl + (group_ok ? trsv_ops_bytes(g->dtype, g->n) : 0);
        int G = group_ok ? (int)std::max<int64_t>(1, std::min<int64_t>(std::min<int64_t>(8, B), (int64_t)((double)(freeg + g->gw.bytes) / 6.0 / (double)per_row))) : 1;
        if (g->gw_cap >= G && g->gw.p) G = g->gw_cap;
        const size_t gneed = (size_t)G * per_row + (dloglh_partial_doubles(g->kernel, g->d) + 8) * sizeof(double) + 256 +
                             (loo ? (size_t)G * loo_vec_bytes(g->dtype, g->n) + 256 : 0);   // + a group's leave-one-out vectors
        GPX_TRY(g->gw.reserve(gneed, g->st));
        g->gw_cap = G;
    }
    if (!g->x_finite || !g->y_finite) { set_error("%s (%s)", NONFINITE_MSG, g->x_finite ? "y" : "x"); return GPX_ERR_ARG; }
    const int64_t n = g->n, lda = g->lda;
    const size_t es = esize(g->dtype);
    const int np = g->nparams;
    const int64_t ride_max = tune().fit_ride_max;
    const bool ride = n <= ride_max;                      // y rides along as row n of every matrix (see gpx_gp_fit)
    const size_t per = (size_t)(n + (ride ? 1 : 0)) * lda * es;
    // ARD: every row of a chunk has its own widths, so its own scaled copy of x (n x d) beside its matrix
    const bool ard = g->kernel == GPX_KERNEL_GAUSSIAN_ARD;
    const size_t xsz = ard ? ((size_t)n * g->d * es + 255) / 256 * 256 : 0;
    size_t freeb = 0, totalb = 0;
    GPX_HIP(hipMemGetInfo(&freeb, &totalb));
    int64_t Bc = (int64_t)((double)freeb * 0.85 / (double)(per + xsz + 4 * (size_t)n * es + 64));
    if (tune().batch_max_set) Bc = std::min<int64_t>(Bc, std::max<int64_t>(1, tune().batch_max));
    Bc = std::max<int64_t>(1, std::min<int64_t>(Bc, B));
    if (!g->bw.p && (double)per > (double)freeb * 0.85) { set_error("fit_batch: not even one more n x n matrix fits in HBM"); return GPX_ERR_NOMEM; }
    // one block, kept in the handle between calls (an ML-II loop calls this once per sweep; a fresh
    // hipMalloc of tens of GB costs more than the factorisations)
    const size_t vec = ((size_t)n * es + 255) / 256 * 256;
    if (g->bw.p && g->bw_cap >= Bc) Bc = std::min<int64_t>(g->bw_cap, B);
    const size_t need = (size_t)Bc * (per + xsz + 3 * vec) + (size_t)Bc * 2 * sizeof(double) + (size_t)Bc * sizeof(int) + 1024;
    bool grew = false;
    GPX_TRY(g->bw.reserve(need, g->st, &grew));
    if (grew) g->bw_cap = Bc;
    struct Ptr { void *p; } Ab, xb, t0, t1, al, sc, inf;
    {
        char *w = (char *)g->bw.p;
        Ab.p = w; w += (size_t)Bc * per;
        xb.p = w; w += (size_t)Bc * xsz;
        t0.p = w; w += (size_t)Bc * vec;
        t1.p = w; w += (size_t)Bc * vec;
        al.p = w; w += (size_t)Bc * vec;
        sc.p = w; w += ((size_t)Bc * 2 * sizeof(double) + 255) / 256 * 256;
        inf.p = w;
    }
    const int64_t sV = (int64_t)(vec / es);               // element stride between the vectors of a chunk
    hipStream_t st = g->st;
    const int64_t sM = (n + (ride ? 1 : 0)) * lda;
    std::vector<double> hs((size_t)Bc * 2);
    std::vector<int> hi((size_t)Bc), valid((size_t)Bc);
    const double eps = 2.220446049250313e-16;            // gp/kernels/gaussian.py:62-69: parameter < EPS is invalid
    for (int64_t b0 = 0; b0 < B; b0 += Bc) {
        const int cnt = (int)std::min<int64_t>(Bc, B - b0);
        for (int i = 0; i < cnt; ++i) {
            const double *th = thetas + (b0 + i) * (np + 1);
            bool ok = th[np] >= 0 && std::isfinite(th[np]);
            for (int k = 0; k < np; ++k) ok = ok && std::isfinite(th[k]) && !(th[k] < eps);
            valid[i] = ok;
            double safe[1 + GPX_ARD_MAX_D];              // an invalid row still takes part in the lock-step
            for (int k = 0; k < np; ++k) safe[k] = 1.0;
            const double *prm = ok ? th : safe;
            const double s = ok ? th[np] : 1.0;
            int kern = g->kernel;
            const void *pts = g->x;
            double iso[2];
            if (ard) {
                void *xi = (char *)xb.p + (size_t)i * xsz;
                GPX_TRY(scale_points(g->dtype, g->x, n, g->d, prm + 1, xi, st));
                ard_iso(prm, g->d, iso);
                kern = GPX_KERNEL_GAUSSIAN; pts = xi; prm = iso;
            }
            GPX_TRY(kmat(g->dtype, kern, GPX_K, pts, n, pts, n, g->d, prm, s * s, GPX_LOWER,
                         (char *)Ab.p + (size_t)i * per, lda, st));
            char *rhs = ride ? (char *)Ab.p + (size_t)i * per + (size_t)n * lda * es : (char *)t0.p + (size_t)i * vec;
            GPX_HIP(hipMemcpyAsync(rhs, g->y, (size_t)n * es, hipMemcpyDeviceToDevice, st));
        }
        Batch bm; bm.count = cnt; bm.sA = bm.sB = bm.sC = sM;
        GPX_TRY(potrf(g->dtype, Ab.p, n, lda, (int *)inf.p, st, cnt > 1 ? &bm : nullptr, ride ? 1 : 0));
        Batch bs; bs.count = cnt; bs.sA = sM; bs.sB = sV; bs.sC = 0;
        if (ride)      // rows n of the matrices (= L^-1 y) side by side as the backward solves' right-hand sides
            GPX_HIP(hipMemcpy2DAsync(t1.p, vec, (char *)Ab.p + (size_t)n * lda * es, per, (size_t)n * es, (size_t)cnt,
                                     hipMemcpyDeviceToDevice, st));
        else
            GPX_TRY(trsv_lower(g->dtype, Ab.p, n, lda, t0.p, t1.p, 0, st, &bs));
        GPX_TRY(trsv_lower(g->dtype, Ab.p, n, lda, t1.p, al.p, 1, st, &bs));
        GPX_TRY(logdet_chol(g->dtype, Ab.p, n, lda, (double *)sc.p, st, cnt, sM, 2));
        GPX_TRY(dot(g->dtype, g->y, al.p, n, (double *)sc.p + 1, st, cnt, 0, sV, 2));
        GPX_HIP(hipMemcpyAsync(hs.data(), sc.p, (size_t)cnt * 2 * sizeof(double), hipMemcpyDeviceToHost, st));
        GPX_HIP(hipMemcpyAsync(hi.data(), inf.p, (size_t)cnt * sizeof(int), hipMemcpyDeviceToHost, st));
        GPX_HIP(hipStreamSynchronize(st));
        for (int i = 0; i < cnt; ++i) GPX_TRY(check_internal_info(hi[i]));
        for (int i = 0; i < cnt; ++i) {
            const double logdet = hs[2 * i], yta = hs[2 * i + 1];
            double v;
            if (!valid[i]) v = NAN;                               // the reference raises ValueError for this row
            else if (loo) v = hi[i] != 0 ? -INFINITY : NAN;       // (a row with a factor: its value comes with its gradient, below)
            else if (hi[i] != 0 || !(logdet >= GPX_MIN_LOG)) v = -INFINITY;     // gp/gp.py:362-365, gp_c.pyx:22-29
            else v = -0.5 * yta - 0.5 * logdet - 0.5 * (double)n * log(2 * M_PI);
            log_lh[b0 + i] = v;
            if (info) info[b0 + i] = valid[i] ? hi[i] : -1;
            if (logdet_yta) { logdet_yta[2 * (b0 + i)] = valid[i] && hi[i] == 0 ? logdet : NAN; logdet_yta[2 * (b0 + i) + 1] = valid[i] && hi[i] == 0 ? yta : NAN; }
        }
        if (dloglh) {
            // gp/gp.py:398-433 per row, on the row's factor and alpha where the lock-step pass left them.  The reference
            // computes the gradient whenever the factorisation succeeds (no logdet < MIN test there); NaN for a row that
            // is not positive definite (gp/gp.py:424-428) or that the reference would have refused (ValueError).
            const size_t nl = (size_t)n * lda * es;
            const int G = (int)g->gw_cap;
            char *Xs = (char *)g->gw.p, *Ws = Xs + (size_t)G * nl;
            const size_t obytes = G > 1 ? trsv_ops_bytes(g->dtype, n) : 0;
            char *Os = Ws + (size_t)G * nl;
            double *part = (double *)(((uintptr_t)(Os + (size_t)G * obytes) + 255) / 256 * 256);
            const size_t lvb = loo_vec_bytes(g->dtype, n);
            char *Vs = (char *)(((uintptr_t)(part + dloglh_partial_doubles(g->kernel, g->d) + 8) + 255) / 256 * 256);   // loo: a group's vectors
            const int tri = loo ? GPX_FULL : GPX_LOWER;
            for (int i0 = 0; i0 < cnt; i0 += G) {
                const int gc = std::min(G, cnt - i0);
                bool any = false;
                for (int i = i0; i < i0 + gc; ++i) any = any || (valid[i] && hi[i] == 0);
                const bool lock_step = G > 1 && gc > 1 && any;
                if (lock_step) {
                    // the group's K^-1 in lock-step: X = L^-T (operators of every row built first), W = X X^T lower.  Rows that are
                    // invalid or not positive definite take part (their factor is garbage; nothing of theirs is read back).
                    GPX_TRY(inv_from_factor(g->dtype, (const char *)Ab.p + (size_t)i0 * per, n, lda, Xs, Ws, tri, st, nullptr, gc,
                                            (int64_t)(per / es), Os));
                    if (loo) {
                        // every row's k, value, r and Y from its own K^-1, then the group's Pm = Y Y^T in lock-step
                        for (int i = i0; i < i0 + gc; ++i) {
                            if (!valid[i] || hi[i] != 0) continue;
                            GPX_TRY(loo_weights_vectors(g->dtype, (char *)Ab.p + (size_t)i * per, n, lda, g->y, (char *)al.p + (size_t)i * vec,
                                                        Xs + (size_t)(i - i0) * nl, Ws + (size_t)(i - i0) * nl,
                                                        loo_vecs_at(Vs + (size_t)(i - i0) * lvb, g->dtype, n), nullptr, nullptr, st));
                        }
                        GPX_TRY(loo_weights_product(g->dtype, n, lda, Xs, Ws, gc, st));
                    }
                }
                for (int i = i0; i < i0 + gc; ++i) {
                    double *o = dloglh + (b0 + i) * (np + 1);
                    if (!valid[i] || hi[i] != 0) { for (int k = 0; k <= np; ++k) o[k] = NAN; continue; }
                    const double *th = thetas + (b0 + i) * (np + 1);
                    const void *alpha_i = (char *)al.p + (size_t)i * vec;
                    const void *pts_i = ard ? (const void *)((char *)xb.p + (size_t)i * xsz) : (const void *)g->x;
                    if (loo) {
                        const LooVecs lv = loo_vecs_at(Vs + (size_t)(lock_step ? i - i0 : 0) * lvb, g->dtype, n);
                        if (!lock_step) {
                            g->bops.invalidate();
                            GPX_TRY(loo_weights_from_factor(g->dtype, (char *)Ab.p + (size_t)i * per, n, lda, g->y, alpha_i, Xs, Ws, lv, nullptr,
                                                            &g->bops, st));
                        }
                        GPX_TRY(loo_grad_reduce(g, pts_i, alpha_i, th, th[np], lv, Ws + (size_t)(lock_step ? i - i0 : 0) * nl, lda, part,
                                                &log_lh[b0 + i], o));
                    } else if (lock_step) {
                        GPX_TRY(grad_reduce(g, pts_i, alpha_i, th, th[np], Ws + (size_t)(i - i0) * nl, lda, part, o));
                    } else {
                        g->bops.invalidate();
                        GPX_TRY(grad_from_factor(g, pts_i, (char *)Ab.p + (size_t)i * per, lda, alpha_i, th, th[np], Xs, Ws, part, &g->bops, o));
                    }
                }
            }
        }
    }
    return GPX_OK;
}

int gpx_gp_fit_batch(gpx_gp_t *g, const double *thetas, int64_t B, double *log_lh, int *info)
{
    GP_ENTER(g);
    return fit_batch_impl(g, thetas, B, log_lh, nullptr, nullptr, info);
}

// The batched ML-II step WITH its gradient (what turns config 5 from grid / restart evaluation into
// optimisation; gp/gp.py:398-433, gp_c.pyx:34-49 for every row of the table): the lock-step factorisation of
// gpx_gp_fit_batch, then per row K^-1 from the row's factor and the fused trace / quadratic-form pass of
// gpx_gp_dloglh_dtheta.  dloglh: HOST (B, n_params + 1) row-major, order (kernel params..., s).  logdet_yta (may be
// NULL): HOST (B, 2) = (log det K, y^T K^-1 y) per row, NaN where the factorisation failed -- from them a caller forms
// the UNCLAMPED log marginal likelihood where the reference's logdet < MIN clamp (gp_c.pyx:22-29) returns -inf.
int gpx_gp_fit_batch_grad(gpx_gp_t *g, const double *thetas, int64_t B, double *log_lh, double *dloglh, double *logdet_yta,
                          int *info)
{
    GP_ENTER(g);
    GPX_ARG(B == 0 || dloglh, "dloglh is NULL");
    GP_NEED_FINITE_Y(g);
    return fit_batch_impl(g, thetas, B, log_lh, dloglh, logdet_yta, info);
}

// The same table under the leave-one-out criterion: loo_log_lh (B) and dloo (B, n_params + 1) per row, from the row's factor
// where the lock-step pass left it (fit_batch_impl, loo).  An invalid row: NaN and NaN; a row that is not positive
// definite: -inf and NaN; info as gpx_gp_fit_batch_grad sets it.
int gpx_gp_fit_batch_loo(gpx_gp_t *g, const double *thetas, int64_t B, double *loo_log_lh, double *dloo, int *info)
{
    GP_ENTER(g);
    GPX_ARG(B == 0 || dloo, "dloo is NULL");
    GP_NEED_FINITE_Y(g);
    return fit_batch_impl(g, thetas, B, loo_log_lh, dloo, nullptr, info, 1);
}

int gpx_gp_last_timing(gpx_gp_t *g, float *ms5)
{
    GP_ENTER(g);
    GPX_ARG(g && g->fitted && ms5, "bad arguments");
    GPX_HIP(hipEventSynchronize(g->ev[4]));
    for (int i = 0; i < 4; ++i) GPX_HIP(hipEventElapsedTime(&ms5[i], g->ev[i], g->ev[i + 1]));
    GPX_HIP(hipEventElapsedTime(&ms5[4], g->ev[0], g->ev[4]));
    return GPX_OK;
}

int gpx_gp_device_ptrs(gpx_gp_t *g, void **A, int64_t *lda, void **x, void **y, void **alpha,
                       void **stream)
{
    GPX_ARG(g, "gp is NULL");
    if (A) *A = g->A;
    if (lda) *lda = g->lda;
    if (x) *x = g->x;
    if (y) *y = g->y;
    if (alpha) *alpha = g->alpha;
    if (stream) *stream = (void *)g->st;
    return GPX_OK;
}

// ----------------------------------------------- host-pointer drop-ins --
int gpx_gaussian_c(int member, double *out, const double *x1, int64_t n, const double *x2, int64_t m,
                   double h, double w)
{
    const double p[2] = {h, w};
    return gpx_kmat_host(GPX_KERNEL_GAUSSIAN, member, out, x1, n, x2, m, 1, p, 0.0);
}

int gpx_gaussian_c_jacobian(double *out, const double *x1, int64_t n, const double *x2, int64_t m,
                            double h, double w)
{
    // gaussian_c.pyx:39-41
    GPX_TRY(gpx_gaussian_c(GPX_DK_DH, out, x1, n, x2, m, h, w));
    return gpx_gaussian_c(GPX_DK_DW, out + n * m, x1, n, x2, m, h, w);
}

int gpx_gaussian_c_hessian(double *out, const double *x1, int64_t n, const double *x2, int64_t m,
                           double h, double w)
{
    // gaussian_c.pyx:44-48
    const int mem[4] = {GPX_D2K_DHDH, GPX_D2K_DHDW, GPX_D2K_DHDW, GPX_D2K_DWDW};
    for (int i = 0; i < 4; ++i) GPX_TRY(gpx_gaussian_c(mem[i], out + (int64_t)i * n * m, x1, n, x2, m, h, w));
    return GPX_OK;
}

int gpx_periodic_c(int member, double *out, const double *x1, int64_t n, const double *x2, int64_t m,
                   double h, double w, double p)
{
    const double prm[3] = {h, w, p};
    return gpx_kmat_host(GPX_KERNEL_PERIODIC, member, out, x1, n, x2, m, 1, prm, 0.0);
}

int gpx_periodic_c_jacobian(double *out, const double *x1, int64_t n, const double *x2, int64_t m,
                            double h, double w, double p)
{
    // periodic_c.pyx:33-36
    const int mem[3] = {GPX_DK_DH, GPX_DK_DW, GPX_DK_DP};
    for (int i = 0; i < 3; ++i) GPX_TRY(gpx_periodic_c(mem[i], out + (int64_t)i * n * m, x1, n, x2, m, h, w, p));
    return GPX_OK;
}

int gpx_periodic_c_hessian(double *out, const double *x1, int64_t n, const double *x2, int64_t m,
                           double h, double w, double p)
{
    // periodic_c.pyx:39-50
    const int mem[9] = {GPX_D2K_DHDH, GPX_D2K_DHDW, GPX_D2K_DHDP, GPX_D2K_DHDW, GPX_D2K_DWDW,
                        GPX_D2K_DWDP, GPX_D2K_DHDP, GPX_D2K_DWDP, GPX_D2K_DPDP};
    for (int i = 0; i < 9; ++i) GPX_TRY(gpx_periodic_c(mem[i], out + (int64_t)i * n * m, x1, n, x2, m, h, w, p));
    return GPX_OK;
}

int gpx_gemm_nt_host(double *C, const double *A, const double *B, int64_t M, int64_t N, int64_t K)
{
    GPX_TRY(ensure_device());
    GPX_ARG(M >= 0 && N >= 0 && K >= 0, "negative dimension");
    if (M == 0 || N == 0) return GPX_OK;
    GPX_ARG(C && (K == 0 || (A && B)), "NULL pointer");
    const int64_t ldk = round_up(std::max<int64_t>(K, 1), 16), ldc = round_up(N, 16);
    DevBuf a, b, c;
    GPX_TRY(a.alloc((size_t)M * ldk * 8));
    GPX_TRY(c.alloc((size_t)M * ldc * 8));
    GPX_HIP(hipMemset(c.p, 0, (size_t)M * ldc * 8));
    if (K > 0) {
        GPX_HIP(hipMemcpy2D(a.p, (size_t)ldk * 8, A, (size_t)K * 8, (size_t)K * 8, (size_t)M, hipMemcpyHostToDevice));
        const void *bp = a.p;
        if (!(B == A && N == M)) {
            GPX_TRY(b.alloc((size_t)N * ldk * 8));
            GPX_HIP(hipMemcpy2D(b.p, (size_t)ldk * 8, B, (size_t)K * 8, (size_t)K * 8, (size_t)N, hipMemcpyHostToDevice));
            bp = b.p;
        }
        GPX_TRY(gemm_nt(GPX_F64, M, N, K, a.p, ldk, bp, ldk, c.p, ldc, 1.0, GPX_FULL, 0, 0, nullptr));
    }
    GPX_HIP(hipMemcpy2D(C, (size_t)N * 8, c.p, (size_t)ldc * 8, (size_t)N * 8, (size_t)M, hipMemcpyDeviceToHost));
    return GPX_OK;
}

int gpx_cholesky(double *L, const double *A, int64_t n, int *info)
{
    GPX_TRY(ensure_device());
    gpx::StreamTurn turn__(nullptr);                           // (this thread's scratch buffers: one stream at a time, gpx_mem.h)
    GPX_ARG(n >= 0 && info, "bad arguments");
    *info = 0;
    if (n == 0) return GPX_OK;
    GPX_ARG(L && A, "NULL pointer");
    const int64_t lda = round_up(n, 16);
    DevBuf a, inf;
    GPX_TRY(a.alloc((size_t)n * lda * 8));
    GPX_TRY(inf.alloc(sizeof(int)));
    GPX_HIP(hipMemcpy2D(a.p, (size_t)lda * 8, A, (size_t)n * 8, (size_t)n * 8, (size_t)n, hipMemcpyHostToDevice));
    GPX_TRY(potrf(GPX_F64, a.p, n, lda, (int *)inf.p, nullptr, nullptr, 0, /*may_block=*/true));
    GPX_TRY(tril(GPX_F64, a.p, n, lda, nullptr));
    GPX_HIP(hipMemcpy(info, inf.p, sizeof(int), hipMemcpyDeviceToHost));
    GPX_TRY(check_internal_info(*info));
    GPX_HIP(hipMemcpy2D(L, (size_t)n * 8, a.p, (size_t)lda * 8, (size_t)n * 8, (size_t)n, hipMemcpyDeviceToHost));
    return GPX_OK;
}

int gpx_cho_solve(const double *L, int64_t n, double *b)
{
    GPX_TRY(ensure_device());
    gpx::StreamTurn turn__(nullptr);                           // (this thread's scratch buffers: one stream at a time, gpx_mem.h)
    GPX_ARG(n >= 0, "n < 0");
    if (n == 0) return GPX_OK;
    GPX_ARG(L && b, "NULL pointer");
    const int64_t ldl = round_up(n, 16);
    DevBuf l, v0, v1;
    GPX_TRY(l.alloc((size_t)n * ldl * 8));
    GPX_TRY(v0.alloc((size_t)n * 8));
    GPX_TRY(v1.alloc((size_t)n * 8));
    GPX_HIP(hipMemcpy2D(l.p, (size_t)ldl * 8, L, (size_t)n * 8, (size_t)n * 8, (size_t)n, hipMemcpyHostToDevice));
    GPX_HIP(hipMemcpy(v0.p, b, (size_t)n * 8, hipMemcpyHostToDevice));
    GPX_TRY(trsv_lower(GPX_F64, l.p, n, ldl, v0.p, v1.p, 0, nullptr));
    GPX_TRY(trsv_lower(GPX_F64, l.p, n, ldl, v1.p, v0.p, 1, nullptr));
    GPX_HIP(hipMemcpy(b, v0.p, (size_t)n * 8, hipMemcpyDeviceToHost));
    return GPX_OK;
}

int gpx_gp_c_log_lh(const double *y, const double *L, const double *Kiy, int64_t n, double *log_lh)
{
    GPX_TRY(ensure_device());
    GPX_ARG(n >= 0 && log_lh, "bad arguments");
    GPX_ARG(n == 0 || (y && L && Kiy), "NULL pointer");
    double h[2] = {0.0, 0.0};
    if (n > 0) {
        // only the diagonal of L is needed: gather it on the host side of the copy
        DevBuf dg, a, b, sc;
        GPX_TRY(dg.alloc((size_t)n * 8));
        GPX_TRY(a.alloc((size_t)n * 8));
        GPX_TRY(b.alloc((size_t)n * 8));
        GPX_TRY(sc.alloc(2 * sizeof(double)));
        GPX_HIP(hipMemcpy2D(dg.p, 8, L, (size_t)(n + 1) * 8, 8, (size_t)n, hipMemcpyHostToDevice));
        GPX_HIP(hipMemcpy(a.p, y, (size_t)n * 8, hipMemcpyHostToDevice));
        GPX_HIP(hipMemcpy(b.p, Kiy, (size_t)n * 8, hipMemcpyHostToDevice));
        GPX_TRY(logdet_chol(GPX_F64, dg.p, n, 0, (double *)sc.p, nullptr));   // stride = ldl + 1 = 1
        GPX_TRY(dot(GPX_F64, a.p, b.p, n, (double *)sc.p + 1, nullptr));
        GPX_HIP(hipMemcpy(h, sc.p, sizeof(h), hipMemcpyDeviceToHost));
    }
    const double logdet = h[0];
    if (!(logdet >= GPX_MIN_LOG)) { *log_lh = -INFINITY; return GPX_OK; }        // gp_c.pyx:22-23
    *log_lh = -0.5 * h[1] + -0.5 * logdet + -0.5 * (double)n * log(2 * M_PI);     // gp_c.pyx:26-29
    return GPX_OK;
}

}  // extern "C"
