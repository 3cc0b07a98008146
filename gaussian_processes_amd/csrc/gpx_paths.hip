// gpx_paths.hip -- posterior function samples by pathwise conditioning (Matheron's rule; Wilson et al. 2020):
//   f_s(a) = phi(a) . Theta_s + sum_j k(a, x_j) V[s, j],     V_s = alpha - Kxx^-1 (Phi(x) Theta_s + sigma E_s)
// a random-feature draw of the prior plus an exact, data-dependent update.  The device primitives -- the feature map and its
// derivative (gpx_d_rff_features, gpx_d_rff_features_grad) and the kernel matrix applied to several weight vectors at once
// without materialising it (gpx_d_kmat_apply; its input-space gradient gpx_d_kmat_apply_grad is gpx_stream.hip's) -- and the
// handle that owns one set of paths (gpx_gp_paths_create, gpx_paths_*).  include/gpx.h has the
// definition of every random input; tests/_paths_helpers.py restates it in numpy.
#include "gpx_small.h"
#include "gpx_kernels_dev.h"
#include "gpx_gp_internal.h"
#include <algorithm>

struct gpx_paths {
    int device, dtype, kernel, d;      // kernel: the family of the GP the paths came from
    int64_t n, S, F, ldv, ldt;         // ldv: pitch of V (the source's lda); ldt: pitch of theta, round_up(2F, 16)
    uint64_t seed;
    double *omega;                     // (F, d) dense, DOUBLE for both dtypes
    void *theta, *V, *pts;             // (S, 2F) ldt; (S, n) ldv; (n, d): the view's points (x, or x / w for ARD)
    double iso[2];                     // the view's isotropic constants (h_v, w_v)
    double w[GPX_ARD_MAX_D];           // ARD: the widths test points are divided by
    double scale;                      // sqrt(k0 / F)
    float ms[4];                       // gpx_debug_paths_timing: how long the creation took, by stage
    gpx::GrowBuf ws;                   // gpx_paths_eval's and gpx_paths_grad's chunk buffers (grow-only, freed with the handle): points, features, values, staging
    hipStream_t st;
};

namespace gpx {

// ---------------------------------------------------------------------------
// Feature map: out[i, f] = scale cos(omega_f . p_i), out[i, F + f] = scale sin(omega_f . p_i).  One thread per (point,
// frequency), frequencies along the lanes (both stores coalesced; a point's coordinates are wave-uniform), a row loop beyond
// 32768 points.  The projection and the sincos are fp64 for both dtypes; the one rounding to fp32 is the store.
// ---------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void rff_features_kernel(const T *__restrict__ pts, int64_t m, int d, const double *__restrict__ omega,
                                                           int64_t F, double scale, T *__restrict__ out, int64_t ld)
{
    const int64_t f = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (f >= F) return;
    const double *w = omega + f * d;
    for (int64_t i = blockIdx.y; i < m; i += gridDim.y) {
        const T *p = pts + i * d;
        double t = 0.0;
        for (int k = 0; k < d; ++k) t = fma(w[k], (double)p[k], t);
        double sn, cs;
        sincos(t, &sn, &cs);
        out[i * ld + f] = (T)(scale * cs);
        out[i * ld + F + f] = (T)(scale * sn);
    }
}

int rff_features(int dtype, const void *pts, int64_t m, int d, const double *omega_dev, int64_t F, double scale, void *out, int64_t ld,
                 hipStream_t st)
{
    if (m <= 0 || F <= 0) return GPX_OK;
    const dim3 grid((unsigned)cdiv(F, 256), (unsigned)std::min<int64_t>(m, 32768)), block(256);
    ProfScope prof(PC_RFF, 2.0 * (double)m * (double)F * (double)esize(dtype), st);
    return by_dtype(dtype, [&](auto t) {
        using T = decltype(t);
        hipLaunchKernelGGL((rff_features_kernel<T>), grid, block, 0, st, (const T *)pts, m, d, omega_dev, F, scale, (T *)out, ld);
        GPX_LAUNCH_CHECK();
        return GPX_OK;
    });
}

// ---------------------------------------------------------------------------
// The feature map's derivative with respect to the point, row i d + k = d phi(p_i) / d p_ik:
//   out[i d + k, f] = -(scale / div_k) omega[f, k] sin(omega_f . p_i),   out[i d + k, F + f] = (scale / div_k) omega[f, k] cos(omega_f . p_i)
// rff_features_kernel's shape and conventions -- one thread per (point, frequency), frequencies along the lanes, fp64
// projection and sincos, one rounding on the store -- with the sincos formed ONCE for the d rows it feeds.  sd: scale / div_k,
// divided on the host (DIV), else `scale` for every k.
// ---------------------------------------------------------------------------
template <typename T, bool DIV>
__global__ __launch_bounds__(256) void rff_features_grad_kernel(const T *__restrict__ pts, int64_t m, int d, const double *__restrict__ omega,
                                                                int64_t F, double scale, ArdWidths sd, T *__restrict__ out, int64_t ld)
{
    const int64_t f = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (f >= F) return;
    const double *w = omega + f * d;
    for (int64_t i = blockIdx.y; i < m; i += gridDim.y) {
        const T *p = pts + i * d;
        double t = 0.0;
        for (int k = 0; k < d; ++k) t = fma(w[k], (double)p[k], t);
        double sn, cs;
        sincos(t, &sn, &cs);
        T *row = out + i * d * ld;
        for (int k = 0; k < d; ++k) {
            const double c = (DIV ? sd.w[k] : scale) * w[k];
            row[k * ld + f] = (T)(-(c * sn));
            row[k * ld + F + f] = (T)(c * cs);
        }
    }
}

int rff_features_grad(int dtype, const void *pts, int64_t m, int d, const double *omega_dev, int64_t F, double scale, const double *col_div,
                      void *out, int64_t ld, hipStream_t st)
{
    if (m <= 0 || F <= 0) return GPX_OK;
    if (col_div && d > GPX_ARD_MAX_D) { set_error("rff_features_grad: column divisors need d <= %d (got %d)", GPX_ARD_MAX_D, d); return GPX_ERR_ARG; }
    ArdWidths sd;
    for (int k = 0; k < GPX_ARD_MAX_D; ++k) sd.w[k] = (col_div && k < d) ? scale / col_div[k] : scale;
    const dim3 grid((unsigned)cdiv(F, 256), (unsigned)std::min<int64_t>(m, 32768)), block(256);
    ProfScope prof(PC_RFF, 2.0 * (double)m * (double)d * (double)F * (double)esize(dtype), st);
    return by_dtype(dtype, [&](auto t) {
        using T = decltype(t);
        if (col_div) hipLaunchKernelGGL((rff_features_grad_kernel<T, true>), grid, block, 0, st, (const T *)pts, m, d, omega_dev, F, scale, sd, (T *)out, ld);
        else hipLaunchKernelGGL((rff_features_grad_kernel<T, false>), grid, block, 0, st, (const T *)pts, m, d, omega_dev, F, scale, sd, (T *)out, ld);
        GPX_LAUNCH_CHECK();
        return GPX_OK;
    });
}

// ---------------------------------------------------------------------------
// K(xo, x) applied to S weight vectors: the fused route is the streamed apply kernel (gpx_stream.hip); beyond its range of
// (d, S) the product route builds K(xo, x) in row chunks and multiplies.
// ---------------------------------------------------------------------------
static thread_local ThreadScratch g_kapply_scr;   // product route: the chunk of K(xo, x) (live across a kmat call, so not the streamed passes' block)

// the product route's chunk of K(xo, x): a multiple of 128 rows (the shifted C pointer of the product stays aligned), at most
// 4096, within KAPPLY_CHUNK_BYTES
constexpr size_t KAPPLY_CHUNK_BYTES = (size_t)256 << 20;

int kmat_apply(int dtype, int kernel, const void *xo, int64_t m, const void *x, int64_t n, int d, const double *params, const void *V,
               int64_t ldv, int64_t S, void *out, int64_t ldo, hipStream_t st)
{
    if (m <= 0 || S <= 0 || n <= 0) return GPX_OK;
    if (kernel != GPX_KERNEL_GAUSSIAN && kernel != GPX_KERNEL_PERIODIC) {
        set_error("kmat_apply: kernel family %d is not supported (GPX_KERNEL_GAUSSIAN or GPX_KERNEL_PERIODIC; the ARD family on scaled points)", kernel);
        return GPX_ERR_UNSUPPORTED;
    }
    const size_t es = esize(dtype);
    if (S <= tune().kapply_fused_max[dtype] && kapply_fused_fits(dtype, d, S)) {
        KParams kp;
        GPX_TRY(make_kparams(kernel, GPX_K, params, 0.0, &kp));
        route_hit(RT_KAPPLY_FUSED);
        return kapply_fused(dtype, xo, m, x, n, d, kp, V, ldv, S, out, ldo, st);
    }
    // (any base and pitch of V: gemm_nt takes its generic kernel where the LDS-DMA one needs 16-byte alignment)
    const int64_t ldk = round_up(n, 16);
    const int64_t fit = (int64_t)(KAPPLY_CHUNK_BYTES / ((size_t)ldk * es)) / 128 * 128;
    const int64_t rows = std::min<int64_t>(m, std::max<int64_t>(128, std::min<int64_t>(fit, 4096)));
    void *Kc = nullptr;
    GPX_TRY(g_kapply_scr.get((size_t)rows * ldk * es, &Kc));
    for (int64_t r0 = 0; r0 < m; r0 += rows) {
        const int64_t rc = std::min(rows, m - r0);
        route_hit(RT_KAPPLY_GEMM);
        GPX_TRY(kmat(dtype, kernel, GPX_K, (const char *)xo + (size_t)r0 * d * es, rc, x, n, d, params, 0.0, GPX_FULL, Kc, ldk, st));
        GPX_TRY(gemm_nt(dtype, S, rc, n, V, ldv, Kc, ldk, (char *)out + (size_t)r0 * es, ldo, 1.0, GPX_FULL, 0, 0, st));
    }
    return GPX_OK;
}

// ---- the handle's small kernels --------------------------------------------------------------------------------------
// R[s, j] = mul * R[s, j]  (alpha == null)   or   R[s, j] = alpha[j] - R[s, j];   mul in the rows' dtype
static int paths_rows(int dtype, void *R, int64_t ld, int64_t rows, int64_t cols, double mul, const void *alpha, hipStream_t st)
{
    return by_dtype(dtype, [&](auto t) {
        using T = decltype(t);
        T *Rt = (T *)R;
        const T *a = (const T *)alpha;
        const T m = (T)mul;
        return map_rows(rows, cols, st, [=] __device__(int64_t r, int64_t c) { Rt[r * ld + c] = a ? a[c] - Rt[r * ld + c] : m * Rt[r * ld + c]; });
    });
}

// rows of a feature chunk: a multiple of 128 (the shifted C pointer of R += Theta Phi_c^T stays aligned), at most 4096, within
// 128 MiB of features
static int64_t paths_feature_rows(int dtype, int64_t ldphi)
{
    const int64_t fit = (int64_t)(((size_t)128 << 20) / ((size_t)ldphi * esize(dtype))) / 128 * 128;
    return std::max<int64_t>(128, std::min<int64_t>(fit, 4096));
}

// rows of a gradient chunk (gpx_paths_grad): a multiple of 128, at most 4096, whose feature blocks -- rows (d + 1) ldt elements:
// the derivative's rows d and the map's own -- fit 512 MiB; never fewer than 128
static int64_t paths_grad_rows(int dtype, int d, int64_t ldt)
{
    const int64_t fit = (int64_t)(((size_t)512 << 20) / ((size_t)(d + 1) * ldt * esize(dtype))) / 128 * 128;
    return std::max<int64_t>(128, std::min<int64_t>(fit, 4096));
}

// the five stage marks of one creation, destroyed on scope exit
struct StageEvents {
    hipEvent_t e[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
    int create() { for (hipEvent_t &x : e) GPX_HIP(hipEventCreate(&x)); return GPX_OK; }
    ~StageEvents() { for (hipEvent_t x : e) if (x) (void)hipEventDestroy(x); }
};

// everything gpx_gp_paths_create enqueues on the source's stream, into a handle whose fields are allocated
static int paths_build(gpx_gp *g, gpx_paths *p)
{
    const GpView v = gp_view(g);
    const int dtype = g->dtype, d = g->d;
    const int64_t n = g->n, S = p->S, F = p->F;
    const size_t es = esize(dtype);
    hipStream_t st = g->st;
    StageEvents ev;                                         // start | generators, copy | features + products | sweeps | V = alpha - R
    GPX_TRY(ev.create());
    GPX_HIP(hipEventRecord(ev.e[0], st));
    GPX_HIP(hipMemcpyAsync(p->pts, v.x, (size_t)n * d * es, hipMemcpyDeviceToDevice, st));
    // Omega = z(seed, 1, .) / w_v
    GPX_TRY(randn(GPX_F64, p->omega, F, d, d, p->seed, 1, 0, st));
    {                                                      // (a true division, as numpy divides)
        double *omega = p->omega;
        const double div = p->iso[1];
        GPX_TRY(map_vec(F * d, st, [=] __device__(int64_t i) { omega[i] = omega[i] / div; }));
    }
    if (S == 0) { GPX_HIP(hipStreamSynchronize(st)); return GPX_OK; }
    GPX_HIP(hipMemsetAsync(p->theta, 0, (size_t)S * p->ldt * es, st));
    GPX_HIP(hipMemsetAsync(p->V, 0, (size_t)S * p->ldv * es, st));
    GPX_TRY(randn(dtype, p->theta, S, 2 * F, p->ldt, p->seed, 2, 0, st));
    // R = sigma E, then R += Theta Phi(x)^T in row chunks of x: a full n x 2F never exists
    void *R = p->V;
    GPX_TRY(randn(dtype, R, S, n, p->ldv, p->seed, 3, 0, st));
    GPX_TRY(paths_rows(dtype, R, p->ldv, S, n, g->s, nullptr, st));
    const int64_t ldphi = p->ldt, rows = std::min(n, paths_feature_rows(dtype, ldphi));
    DevBuf phi;
    GPX_TRY(phi.alloc((size_t)rows * ldphi * es));
    GPX_HIP(hipEventRecord(ev.e[1], st));
    for (int64_t r0 = 0; r0 < n; r0 += rows) {
        const int64_t rc = std::min(rows, n - r0);
        GPX_TRY(rff_features(dtype, (const char *)p->pts + (size_t)r0 * d * es, rc, d, p->omega, F, p->scale, phi.p, ldphi, st));
        GPX_TRY(gemm_nt(dtype, S, rc, 2 * F, p->theta, p->ldt, phi.p, ldphi, (char *)R + (size_t)r0 * es, p->ldv, 1.0, GPX_FULL, 0, 0, st));
    }
    GPX_HIP(hipEventRecord(ev.e[2], st));
    // R <- R Kxx^-1 (rows are right-hand sides: two sweeps over the factor), V = alpha - R
    GPX_TRY(trsm_right_lt(dtype, g->A, n, g->lda, R, S, p->ldv, st, 0, &g->ops));
    GPX_TRY(trsm_right_l(dtype, g->A, n, g->lda, R, S, p->ldv, st, &g->ops));
    GPX_HIP(hipEventRecord(ev.e[3], st));
    GPX_TRY(paths_rows(dtype, R, p->ldv, S, n, 0.0, g->alpha, st));
    GPX_HIP(hipEventRecord(ev.e[4], st));
    GPX_HIP(hipStreamSynchronize(st));                      // (phi is freed on return)
    GPX_HIP(hipEventElapsedTime(&p->ms[0], ev.e[1], ev.e[2]));
    GPX_HIP(hipEventElapsedTime(&p->ms[1], ev.e[2], ev.e[3]));
    GPX_HIP(hipEventElapsedTime(&p->ms[3], ev.e[0], ev.e[4]));
    p->ms[2] = p->ms[3] - p->ms[0] - p->ms[1];
    return GPX_OK;
}

}  // namespace gpx

using namespace gpx;

// upload_f64 takes its staging copy as a DevBuf; this one looks at memory the handle owns and frees nothing
struct StageView {
    gpx::DevBuf buf;
    explicit StageView(void *p) { buf.p = p; }
    ~StageView() { buf.p = nullptr; }
};

// every gpx_paths_* entry: GP_ENTER's steps for a paths handle
#define PATHS_ENTER(p)                                                       \
    GPX_ARG((p) != nullptr, "paths is NULL");                                \
    gpx::tune_refresh();                                                     \
    gpx::DeviceGuard guard__((p)->device);                                   \
    if (guard__.rc != GPX_OK) return guard__.rc;                             \
    gpx::StreamTurn turn__((p)->st);                                         \
    gpx::RoctxRange api_range__(__func__)

extern "C" {

int gpx_d_rff_features(int dtype, const void *pts, int64_t m, int d, const double *omega_dev, int64_t F, double scale, void *out,
                       int64_t ld, void *stream)
{
    GPX_TRY(ensure_device());
    GPX_ARG(dtype == GPX_F64 || dtype == GPX_F32, "dtype must be GPX_F64 or GPX_F32");
    GPX_ARG(m >= 0 && F >= 0 && d >= 1, "need m, F >= 0 and d >= 1");
    if (m == 0 || F == 0) return GPX_OK;
    GPX_ARG(pts && omega_dev && out, "NULL pointer");
    GPX_ARG(F <= INT64_MAX / 2 && ld >= 2 * F, "ld < 2 F");
    GPX_ARG(m <= INT64_MAX / ld && F <= INT64_MAX / d, "m * ld overflows");
    GPX_ARG(cdiv(F, 256) <= 0x7fffffff, "F is more than one launch covers");
    return rff_features(dtype, pts, m, d, omega_dev, F, scale, out, ld, S(stream));
}

int gpx_d_rff_features_grad(int dtype, const void *pts, int64_t m, int d, const double *omega_dev, int64_t F, double scale,
                            const double *col_div, void *out, int64_t ld, void *stream)
{
    GPX_TRY(ensure_device());
    GPX_ARG(dtype == GPX_F64 || dtype == GPX_F32, "dtype must be GPX_F64 or GPX_F32");
    GPX_ARG(m >= 0 && F >= 0 && d >= 1, "need m, F >= 0 and d >= 1");
    if (m == 0 || F == 0) return GPX_OK;
    GPX_ARG(pts && omega_dev && out, "NULL pointer");
    GPX_ARG(F <= INT64_MAX / 2 && ld >= 2 * F, "ld < 2 F");
    GPX_ARG(m <= INT64_MAX / d && m * d <= INT64_MAX / ld && F <= INT64_MAX / d, "m * d * ld overflows");
    GPX_ARG(cdiv(F, 256) <= 0x7fffffff, "F is more than one launch covers");
    return rff_features_grad(dtype, pts, m, d, omega_dev, F, scale, col_div, out, ld, S(stream));
}

int gpx_d_kmat_apply(int dtype, int kernel, const void *xo, int64_t m, const void *x, int64_t n, int d, const double *params,
                     const void *V, int64_t ldv, int64_t Sn, void *out, int64_t ldo, void *stream)
{
    gpx::StreamTurn turn__((hipStream_t)stream);     // (this thread's scratch buffers: one stream at a time, gpx_mem.h)
    GPX_TRY(ensure_device());
    GPX_ARG(dtype == GPX_F64 || dtype == GPX_F32, "dtype must be GPX_F64 or GPX_F32");
    GPX_ARG(n >= 0 && m >= 0 && Sn >= 0 && d >= 1, "need n, m, S >= 0 and d >= 1");
    if (m == 0 || Sn == 0 || n == 0) return GPX_OK;
    GPX_ARG(xo && x && V && out && params, "NULL pointer");
    GPX_ARG(ldv >= n && ldo >= m, "leading dimension too small");
    GPX_ARG(Sn <= INT64_MAX / ldv && Sn <= INT64_MAX / ldo && cdiv(m, 4) <= 0x7fffffff, "S * ld overflows, or m is more than one launch covers");   // (cdiv(m, 4): the most workgroups along x)
    return kmat_apply(dtype, kernel, xo, m, x, n, d, params, V, ldv, Sn, out, ldo, S(stream));
}

int gpx_paths_destroy(gpx_paths_t *p)
{
    if (!p) return GPX_OK;
    gpx::DeviceGuard guard__(p->device);
    if (p->st) (void)hipStreamSynchronize(p->st);
    stream_epoch_bump();                                       // (StreamTurn: a later stream at this one's address is a different stream)
    for (void *b : {(void *)p->omega, p->theta, p->V, p->pts}) dev_free(b);
    p->ws.release();
    if (p->st) (void)hipStreamDestroy(p->st);
    delete p;
    return GPX_OK;
}

int gpx_gp_paths_create(gpx_gp_t *g, int64_t Sn, int64_t F, uint64_t seed, gpx_paths_t **out)
{
    GPX_ARG(out, "paths is NULL");
    *out = nullptr;
    GP_ENTER(g);
    if (g->kernel == GPX_KERNEL_PERIODIC) {
        set_error("gpx_gp_paths_create: the periodic family is not supported (GPX_KERNEL_GAUSSIAN and GPX_KERNEL_GAUSSIAN_ARD are)");
        return GPX_ERR_UNSUPPORTED;
    }
    GPX_ARG(Sn >= 0 && F >= 1, "need S >= 0 and F >= 1");
    GPX_ARG(g->fitted && g->have_data, "gp is not fitted");
    if (!g->have_params) {
        set_error("gpx_gp_paths_create: a handle fitted from gpx_gp_set_K has no kernel parameters to draw a prior from");
        return GPX_ERR_UNSUPPORTED;
    }
    if (!g->y_finite) { set_error("array must not contain infs or NaNs (y)"); return GPX_ERR_ARG; }
    GPX_ARG(F <= (INT64_MAX / 4) / std::max<int64_t>(Sn, g->d) && Sn <= INT64_MAX / (g->lda * 8), "S * F, F * d or S * n overflows");
    GPX_TRY(gp_need_factor(g, "to condition the paths on"));
    const GpView v = gp_view(g);
    const size_t es = esize(g->dtype);
    gpx_paths *p = new gpx_paths();
    memset(p, 0, sizeof(*p));
    p->device = g->device; p->dtype = g->dtype; p->kernel = g->kernel; p->d = g->d;
    p->n = g->n; p->S = Sn; p->F = F; p->seed = seed;
    p->ldv = g->lda; p->ldt = round_up(2 * F, 16);
    p->iso[0] = v.params[0]; p->iso[1] = v.params[1];
    for (int k = 0; k < GPX_ARD_MAX_D; ++k) p->w[k] = (g->kernel == GPX_KERNEL_GAUSSIAN_ARD && k < g->d) ? g->params[1 + k] : 1.0;
    const double k0 = 0.5 * sqrt(2.0 / M_PI) * p->iso[0] * p->iso[0] / p->iso[1];     // gp_prior_var: h_v^2 / (w_v sqrt(2 pi))
    p->scale = sqrt(k0 / (double)F);
    int rc = GPX_OK;
#define PATHS_ALLOC(field, bytes) if (rc == GPX_OK) rc = dev_alloc((void **)&p->field, (bytes) ? (bytes) : 16, "hipMalloc " #field)
    PATHS_ALLOC(omega, (size_t)F * g->d * sizeof(double));
    PATHS_ALLOC(theta, (size_t)Sn * p->ldt * es);
    PATHS_ALLOC(V, (size_t)Sn * p->ldv * es);
    PATHS_ALLOC(pts, (size_t)g->n * g->d * es);
#undef PATHS_ALLOC
    if (rc == GPX_OK) {
        hipError_t e = hipStreamCreateWithFlags(&p->st, hipStreamNonBlocking);
        if (e != hipSuccess) rc = hip_fail(e, "hipStreamCreate", __FILE__, __LINE__);
    }
    if (rc == GPX_OK) rc = paths_build(g, p);
    if (rc == GPX_OK) {
        hipError_t e = hipStreamSynchronize(g->st);
        if (e != hipSuccess) rc = hip_fail(e, "hipStreamSynchronize", __FILE__, __LINE__);
    }
    if (rc != GPX_OK) { (void)hipStreamSynchronize(g->st); gpx_paths_destroy(p); return rc; }
    *out = p;
    return GPX_OK;
}

int gpx_paths_eval(gpx_paths_t *p, const double *xo, int64_t m, int64_t chunk_rows, double *out)
{
    PATHS_ENTER(p);
    GPX_ARG(m >= 0 && (m == 0 || p->S == 0 || (xo && out)), "bad arguments");
    if (chunk_rows < 0 || chunk_rows % 128 != 0) {
        set_error("gpx_paths_eval: chunk_rows must be 0 (automatic) or a multiple of 128");
        return GPX_ERR_ARG;
    }
    if (m == 0 || p->S == 0) return GPX_OK;
    const int dtype = p->dtype, d = p->d;
    const int64_t S = p->S, F = p->F;
    const size_t es = esize(dtype);
    GPX_ARG(m <= INT64_MAX / (8 * std::max<int64_t>(S, d)), "S * m overflows");
    int64_t rows = chunk_rows ? chunk_rows : paths_feature_rows(dtype, p->ldt);
    if (m <= rows) rows = m;                              // one chunk: exactly the rows there are
    const int64_t ldo = round_up(rows, 16);
    // One chunk's buffers, carved out of the handle's grow-only block: a loop that evaluates round after round allocates once.
    const auto pad = [](size_t b) { return (b + 255) / 256 * 256; };
    const size_t b_xo = pad((size_t)rows * d * es), b_phi = pad((size_t)rows * p->ldt * es), b_out = pad((size_t)S * ldo * es);
    const size_t b_stage = dtype == GPX_F64 ? 0 : pad((size_t)rows * d * sizeof(double));   // upload_f64's float64 copy (fp32 only)
    GPX_TRY(p->ws.reserve(b_xo + b_phi + b_out + b_stage, p->st));
    char *base = (char *)p->ws.p;
    void *dxo = base, *phi = base + b_xo, *outc = base + b_xo + b_phi;
    StageView stage(b_stage ? base + b_xo + b_phi + b_out : nullptr);
    for (int64_t r0 = 0; r0 < m; r0 += rows) {
        const int64_t rc = std::min(rows, m - r0);
        GPX_TRY(upload_f64(dtype, dxo, rc * d, xo + r0 * d, rc * d, 1, rc * d, p->st, b_stage ? &stage.buf : nullptr));
        if (p->kernel == GPX_KERNEL_GAUSSIAN_ARD) GPX_TRY(scale_points(dtype, dxo, rc, d, p->w, dxo, p->st));
        GPX_TRY(rff_features(dtype, dxo, rc, d, p->omega, F, p->scale, phi, p->ldt, p->st));
        GPX_HIP(hipMemsetAsync(outc, 0, (size_t)S * ldo * es, p->st));
        GPX_TRY(gemm_nt(dtype, S, rc, 2 * F, p->theta, p->ldt, phi, p->ldt, outc, ldo, 1.0, GPX_FULL, 0, 0, p->st));
        GPX_TRY(kmat_apply(dtype, GPX_KERNEL_GAUSSIAN, dxo, rc, p->pts, p->n, d, p->iso, p->V, p->ldv, S, outc, ldo, p->st));
        GPX_TRY(download_f64(dtype, out + r0, m, outc, ldo, S, rc, 0, p->st));
    }
    return GPX_OK;
}

int gpx_paths_grad(gpx_paths_t *p, const double *xo, int64_t m, int64_t chunk_rows, double *values, double *grad)
{
    PATHS_ENTER(p);
    GPX_ARG(m >= 0 && (m == 0 || p->S == 0 || (xo && grad)), "bad arguments");
    if (chunk_rows < 0 || chunk_rows % 128 != 0) {
        set_error("gpx_paths_grad: chunk_rows must be 0 (automatic) or a multiple of 128");
        return GPX_ERR_ARG;
    }
    if (m == 0 || p->S == 0) return GPX_OK;
    const int dtype = p->dtype, d = p->d;
    const int64_t S = p->S, F = p->F;
    const size_t es = esize(dtype);
    const bool ard = p->kernel == GPX_KERNEL_GAUSSIAN_ARD;
    GPX_ARG(m <= (INT64_MAX / 8) / (std::max<int64_t>(S, 1) * d), "S * m * d overflows");
    int64_t rows = chunk_rows ? chunk_rows : paths_grad_rows(dtype, d, p->ldt);
    if (m <= rows) rows = m;                              // one chunk: exactly the rows there are
    const int64_t ldo = round_up(rows, 16), ldg = round_up(rows * d, 16);
    // One chunk's buffers, carved out of the handle's grow-only block as gpx_paths_eval's are: points, the derivative's
    // features, the gradient block, and with values the map's own features and the value block
    const auto pad = [](size_t b) { return (b + 255) / 256 * 256; };
    const size_t b_xo = pad((size_t)rows * d * es), b_psi = pad((size_t)rows * d * p->ldt * es), b_g = pad((size_t)S * ldg * es);
    const size_t b_phi = values ? pad((size_t)rows * p->ldt * es) : 0, b_out = values ? pad((size_t)S * ldo * es) : 0;
    const size_t b_stage = dtype == GPX_F64 ? 0 : pad((size_t)rows * d * sizeof(double));   // upload_f64's float64 copy (fp32 only)
    GPX_TRY(p->ws.reserve(b_xo + b_psi + b_g + b_phi + b_out + b_stage, p->st));
    char *base = (char *)p->ws.p;
    void *dxo = base, *psi = base + b_xo, *gc = base + b_xo + b_psi, *phi = base + b_xo + b_psi + b_g, *outc = base + b_xo + b_psi + b_g + b_phi;
    StageView stage(b_stage ? base + b_xo + b_psi + b_g + b_phi + b_out : nullptr);
    const double *col_div = ard ? p->w : nullptr;
    for (int64_t r0 = 0; r0 < m; r0 += rows) {
        const int64_t rc = std::min(rows, m - r0);
        route_hit(RT_PATHS_GRAD_CHUNK);
        GPX_TRY(upload_f64(dtype, dxo, rc * d, xo + r0 * d, rc * d, 1, rc * d, p->st, b_stage ? &stage.buf : nullptr));
        if (ard) GPX_TRY(scale_points(dtype, dxo, rc, d, p->w, dxo, p->st));
        GPX_TRY(rff_features_grad(dtype, dxo, rc, d, p->omega, F, p->scale, col_div, psi, p->ldt, p->st));
        GPX_HIP(hipMemsetAsync(gc, 0, (size_t)S * ldg * es, p->st));
        GPX_TRY(gemm_nt(dtype, S, rc * d, 2 * F, p->theta, p->ldt, psi, p->ldt, gc, ldg, 1.0, GPX_FULL, 0, 0, p->st));
        GPX_TRY(kapply_grad(dtype, dxo, rc, p->pts, p->n, d, p->iso, col_div, p->V, p->ldv, S, gc, ldg, p->st));
        GPX_TRY(download_f64(dtype, grad + r0 * d, m * d, gc, ldg, S, rc * d, 0, p->st));
        if (values) {                                     // gpx_paths_eval's steps on the same uploaded chunk
            GPX_TRY(rff_features(dtype, dxo, rc, d, p->omega, F, p->scale, phi, p->ldt, p->st));
            GPX_HIP(hipMemsetAsync(outc, 0, (size_t)S * ldo * es, p->st));
            GPX_TRY(gemm_nt(dtype, S, rc, 2 * F, p->theta, p->ldt, phi, p->ldt, outc, ldo, 1.0, GPX_FULL, 0, 0, p->st));
            GPX_TRY(kmat_apply(dtype, GPX_KERNEL_GAUSSIAN, dxo, rc, p->pts, p->n, d, p->iso, p->V, p->ldv, S, outc, ldo, p->st));
            GPX_TRY(download_f64(dtype, values + r0, m, outc, ldo, S, rc, 0, p->st));
        }
    }
    return GPX_OK;
}

int gpx_paths_get(gpx_paths_t *p, double *omega, double *theta, double *V)
{
    PATHS_ENTER(p);
    if (omega) {
        GPX_HIP(hipMemcpyAsync(omega, p->omega, (size_t)p->F * p->d * sizeof(double), hipMemcpyDeviceToHost, p->st));
        GPX_HIP(hipStreamSynchronize(p->st));
    }
    if (theta) GPX_TRY(download_f64(p->dtype, theta, 2 * p->F, p->theta, p->ldt, p->S, 2 * p->F, 0, p->st));
    if (V) GPX_TRY(download_f64(p->dtype, V, p->n, p->V, p->ldv, p->S, p->n, 0, p->st));
    return GPX_OK;
}

int gpx_debug_paths_timing(gpx_paths_t *p, float *ms4)
{
    GPX_ARG(p != nullptr && ms4 != nullptr, "NULL argument");
    for (int i = 0; i < 4; ++i) ms4[i] = p->ms[i];
    return GPX_OK;
}

int gpx_paths_describe(gpx_paths_t *p, int *dtype, int *kernel, int64_t *n, int *d, int64_t *Sn, int64_t *F, uint64_t *seed)
{
    GPX_ARG(p != nullptr, "paths is NULL");
    if (dtype) *dtype = p->dtype;
    if (kernel) *kernel = p->kernel;
    if (n) *n = p->n;
    if (d) *d = p->d;
    if (Sn) *Sn = p->S;
    if (F) *F = p->F;
    if (seed) *seed = p->seed;
    return GPX_OK;
}

}  // extern "C"
