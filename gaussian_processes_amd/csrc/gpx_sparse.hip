// gpx_sparse.hip -- sparse GP regression on M inducing points (Titsias 2009, the collapsed bound): gpx_sgp_*.
//
//   Kuu = K(z, z) + eps I = Luu Luu^T      Phi = sum_c K(z, x_c) K(x_c, z)      b = sum_c K(z, x_c) y_c
//   X = Luu^-1 Phi Luu^-T                  B = I + X / s^2 = LB LB^T            c = LB^-1 Luu^-1 b / s
//   elbo = -sum log diag LB - N/2 log 2 pi - N log s - yy / (2 s^2) + c.c / (2 s^2) - (kff - tr X) / (2 s^2)
//   mean(a) = k(a, z) w,  w = Luu^-T LB^-T c / s       var(a) = k(a, a) - |Luu^-1 k(z, a)|^2 + |LB^-1 Luu^-1 k(z, a)|^2
// (Kuu + Phi / s^2 is never factored: log|A| - log|Kuu| cancels badly; B = I + X / s^2 is well conditioned.)
//
// The hot path is the Gram matrix Phi, 2 M^2 N flops: x goes by in column chunks, G = K(z, x_c) is MATERIALISED once per
// chunk (M x c, the chunk's columns contiguous: both operands of G G^T are depth-contiguous, the NT product's layout) and
// multiplied by the product kernel of gpx_gemm.hip on the lower tiles.  Fusing the kernel evaluation into the product
// would re-evaluate each operand panel once per output tile column (M / 128 times) in a build that is VALU-bound.
// Phi is small and the depth enormous -- the opposite of a trailing update -- so the depth of a chunk is split over the
// product's batch dimension: slice p of every chunk adds to partial accumulator p, and sum_slices_lower adds the
// partials in slice order at the end.  No atomics: a repeated fit gives the same bits.
// Everything after that is M x M: potrf, the triangular sweeps and the reductions the library already owns, plus the small
// kernels of this file (B and the trace, the two-block variance rows) and the transpose of gpx_small.hip, mirror mode included.
//
// Layout in HBM (dtype T, ldm = round_up(M, 16)):
//   x (N, d)  y (N)  z (M, d)  [xs, zs: the ARD family's scaled copies]
//   Luu, Phi, Xf, Xt, LB   M x ldm each     (Xf, Xt: work; X ends up in Xt)
//   cvec, w, t0, t1        M each
//   bacc                   M doubles
//   work (grow-only)       every pass lays it out anew, ONCE, with the carver of gpx_mem.h (each sub-block on 128 bytes):
//                          sgp_fit_layout   G (M x cols) | the partial accumulators (slices x M x ldm)
//                          sgp_grad_layout  reduction partials | three M x ldm blocks | K(x_c, z), P (c x ldm each)
//                          and behind them, for the gradient in z: its M x d accumulator (f64) | -w | its slices' partials
// Both passes take their chunks from sgp_plan (the gradient's: gpx_debug_sgp_grad_plan) and their times from the handle's one
// SgpTimeline: a pass is a sequence of marks on the stream, resolved into fit_ms / grad_ms / zgrad_ms when it ends.
//
// The gradient of the bound in the hyper-parameters (gpx_sgp_grad; include/gpx.h has the formulas): everything M x M from the
// factors the fit left (Luu, LB, X in Xt, w) by the sweeps and products the library has, then a second pass over x in
// column chunks: K(x_c, z), ONE product P = K(x_c, z) T, and the rectangular tile reduction of gpx_kmat.hip.  It writes
// Xf, t0 and the work buffer only, so the fit's state -- elbo, the predictions, what gpx_sgp_get returns -- stays as it was.
// The gradient in the inducing inputs (gpx_sgp_grad_z) rides on that pass: the same T, the same P and the same coefficients
// P[j, i] + y_j w_i, contracted against dk/dz_ik by rect_zgrad (gpx_zgrad.hip) beside rect_reduce, and once more on z against
// itself with the mirrored -A A^T / s^4 for Kuu's share.
#include "gpx_small.h"
#include <algorithm>
#include <cmath>
#include <vector>

#include "gpx_gp_internal.h"

// what a fit leaves behind on the device
struct SgpScal {
    double logdetB;    // 2 sum log diag LB (logdet_chol)
    double yy;         // y . y
    double cc;         // c . c
    double k00;        // k(z_0, z_0), the kernel's value at distance zero in the handle's arithmetic
    double trX;        // trace of X
    double zero;       // stays 0: the row sum k(0) is `finished` against
    int info1, info2;  // potrf of Kuu, of B
};

// the times of a pass: the handle's one PassTimeline (gpx_gp_internal.h)
constexpr int SGP_NOBODY = gpx::TL_NOBODY;
using SgpTimeline = gpx::PassTimeline;

struct gpx_sgp {
    int device, dtype, kernel, d, nparams;
    int64_t n, m, ldm;
    void *x, *y, *z, *xs, *zs;
    void *Luu, *Phi, *Xf, *Xt, *LB;
    void *cvec, *w, *t0, *t1;
    double *bacc;
    SgpScal *scal;
    gpx::GrowBuf work;
    hipStream_t st;
    SgpTimeline tl;
    double params[1 + GPX_ARD_MAX_D], iso[2];
    double s, jitter;
    bool have_x, have_y, have_z, fitted, have_grad, have_zgrad;
    int stage, pivot, split;
    SgpScal host;                      // the scalars of the last good fit
    float fit_ms[5], grad_ms[5], zgrad_ms[2];      // the last passes' times, as gpx_sgp_last_{,grad_,zgrad_}timing return them
};

namespace gpx {

constexpr int64_t SGP_CHUNK_ALIGN = 128, SGP_CHUNK_CAP = 16384, SGP_TARGET_WGS = 256, SGP_MIN_SLICES = 8, SGP_MAX_SLICES = 16,
                  SGP_ACC_BYTES = (int64_t)2 << 30;

// ---- the plan: columns per chunk, depth slices ---------------------------------------------------------------------------
struct SgpPlan { int64_t cols, chunks; int slices; int64_t slice_cols; };
enum SgpPass { SGP_FIT, SGP_GRAD };

// the one place chunk_cols is checked.  SGP_GRAD: the fit's columns, with two c x ldm blocks where the fit has one M x c
// (slices and slice_cols stay the fit's: the gradient's product is not split)
static int sgp_plan(SgpPass pass, int dtype, int64_t n, int64_t M, int64_t chunk_cols, int split, size_t free_bytes, SgpPlan *plan)
{
    if (!(dtype == GPX_F64 || dtype == GPX_F32)) { set_error("sparse plan: dtype must be GPX_F64 or GPX_F32"); return GPX_ERR_ARG; }
    if (n < 1 || M < 1) { set_error("sparse plan: need n >= 1 and m_inducing >= 1"); return GPX_ERR_ARG; }
    if (chunk_cols < 0 || chunk_cols % SGP_CHUNK_ALIGN != 0) {
        set_error("sparse plan: chunk_cols must be 0 (automatic) or a multiple of %d (got %lld)", (int)SGP_CHUNK_ALIGN, (long long)chunk_cols);
        return GPX_ERR_ARG;
    }
    if (split < 0) { set_error("sparse plan: split must be >= 0"); return GPX_ERR_ARG; }
    const size_t per_col = (size_t)M * esize(dtype), budget = free_bytes / 4;
    const int64_t fit = (int64_t)std::min<size_t>(budget / per_col, (size_t)1 << 40) / SGP_CHUNK_ALIGN * SGP_CHUNK_ALIGN;
    if (fit < SGP_CHUNK_ALIGN) {
        set_error("sparse plan: not even %d columns of %lld rows fit a quarter of the free device memory (%zu bytes free)",
                  (int)SGP_CHUNK_ALIGN, (long long)M, free_bytes);
        return GPX_ERR_NOMEM;
    }
    int64_t c = chunk_cols ? chunk_cols : std::min(fit, SGP_CHUNK_CAP);
    c = std::min(c, round_up(n, SGP_CHUNK_ALIGN));                     // one chunk: no wider than the data
    if ((size_t)c * per_col > budget) {
        set_error("sparse plan: chunk_cols = %lld needs %zu bytes, more than a quarter of the free device memory (%zu bytes free)",
                  (long long)chunk_cols, (size_t)c * per_col, free_bytes);
        return GPX_ERR_NOMEM;
    }
    // Depth slices: a function of (M, dtype) alone, so that results do not depend on the box.  Enough of them for the tiles
    // of the lower triangle to cover the chip, and never fewer than SGP_MIN_SLICES: the product kernel runs a depth of
    // 2048 columns per workgroup faster than one of 16384 whatever the tile count (fp64, d = 32, N = 2^20, chunk 16384,
    // Gram product TF/s at P = 1 | 2 | 4 | 8 | 16:  M = 1024  4.7 | 9.3 | 18.3 | 35.6 | 38.6,  M = 2048  9.2 | 15.0 | 21.3 |
    // 26.9 | 26.7,  M = 4096  37.0 | 41.5 | 44.5 | 55.3 | 54.5).  The partial accumulators together stay within
    // SGP_ACC_BYTES.
    const int64_t T = cdiv(M, 128), tiles = T * (T + 1) / 2;
    const int64_t acc_fit = std::max<int64_t>(1, SGP_ACC_BYTES / ((int64_t)M * round_up(M, 16) * (int64_t)esize(dtype)));
    const int64_t planned = std::min(acc_fit, std::min(SGP_MAX_SLICES, std::max(SGP_MIN_SLICES, cdiv(SGP_TARGET_WGS, tiles))));
    const int64_t P = split > 0 ? split : planned;
    const int64_t W = round_up(std::max(cdiv(c, P), SGP_CHUNK_ALIGN), SGP_CHUNK_ALIGN);
    const int slices = (int)cdiv(c, W);
    const size_t per_two = (size_t)2 * round_up(M, 16) * esize(dtype);
    if (pass == SGP_GRAD && (size_t)c * per_two > budget) {
        if (chunk_cols == 0) c = std::max(SGP_CHUNK_ALIGN, c / 2 / SGP_CHUNK_ALIGN * SGP_CHUNK_ALIGN);
        if ((size_t)c * per_two > budget) {
            set_error("sparse gradient: two blocks of %lld columns and %lld rows do not fit a quarter of the free device memory (%zu bytes free)",
                      (long long)c, (long long)M, free_bytes);
            return GPX_ERR_NOMEM;
        }
    }
    *plan = {c, cdiv(n, c), slices, W};
    return GPX_OK;
}

// ---- the kernels ---------------------------------------------------------------------------------------------------------
// a 256-thread workgroup's sum, in a fixed order (a binary tree over the thread index); the result is valid in thread 0
__device__ __forceinline__ double block256_sum(double v, double *red)
{
    const int tid = threadIdx.x;
    __syncthreads();                                       // (a previous use of red[] has been read)
    red[tid] = v;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (tid < s) red[tid] += red[tid + s];
        __syncthreads();
    }
    return red[0];
}

// acc[i] += sum_j G[i, j] y[j]: one workgroup per row (grid-stride), every lane its columns in index order, then the tree
template <typename T>
__global__ __launch_bounds__(256) void gemv_acc_kernel(const T *__restrict__ G, int64_t rows, int64_t cols, int64_t ldg,
                                                       const T *__restrict__ y, double *__restrict__ acc)
{
    __shared__ double red[256];
    for (int64_t i = blockIdx.x; i < rows; i += gridDim.x) {
        const T *__restrict__ g = G + i * ldg;
        double v = 0.0;
        for (int64_t j = threadIdx.x; j < cols; j += 256) v = fma((double)g[j], (double)y[j], v);
        const double t = block256_sum(v, red);
        if (threadIdx.x == 0) acc[i] += t;
    }
}

// B[i, j] = (i == j) + X[i, j] / s^2 for j <= i; the workgroups of the extra grid row y == gridDim.y - 1 do not write B:
// the first of them sums the diagonal of X in f64 in a fixed order
template <typename T>
__global__ __launch_bounds__(256) void form_B_kernel(const T *__restrict__ X, int64_t ldx, int64_t n, double s2, T *__restrict__ B,
                                                     int64_t ldb, double *__restrict__ trace)
{
    __shared__ double red[256];
    if (blockIdx.y == gridDim.y - 1) {
        if (blockIdx.x != 0) return;
        double v = 0.0;
        for (int64_t i = threadIdx.x; i < n; i += 256) v += (double)X[i * ldx + i];
        const double t = block256_sum(v, red);
        if (threadIdx.x == 0) trace[0] = t;
        return;
    }
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    for (int64_t i = blockIdx.y; i < n; i += gridDim.y - 1) {
        if (j > i) continue;
        const double v = (double)X[i * ldx + j] / s2 + (i == j ? 1.0 : 0.0);
        B[i * ldb + j] = (T)v;
    }
}

// acc[i] = sum_j V[i, j]^2 - sum_j W[i, j]^2: the two solved blocks of the variance, f64, one workgroup per row
template <typename T>
__global__ __launch_bounds__(256) void rows2_kernel(const T *__restrict__ V, const T *__restrict__ W, int64_t rows, int64_t n, int64_t ldx,
                                                    double *__restrict__ acc)
{
    __shared__ double red[256];
    for (int64_t i = blockIdx.x; i < rows; i += gridDim.x) {
        const T *__restrict__ v = V + i * ldx, *__restrict__ w = W + i * ldx;
        double a = 0.0, b = 0.0;
        for (int64_t j = threadIdx.x; j < n; j += 256) {
            a = fma((double)v[j], (double)v[j], a);
            b = fma((double)w[j], (double)w[j], b);
        }
        const double sa = block256_sum(a, red);
        const double sb = block256_sum(b, red);
        if (threadIdx.x == 0) acc[i] = sa - sb;
    }
}

// dst[i] = (T)(src[i] / div), src DOUBLE;  v[i] = (T)(v[i] / div)
static int cvt_div(int dtype, const double *src, void *dst, int64_t n, double div, hipStream_t st)
{
    return by_dtype(dtype, [&](auto t) {
        using T = decltype(t);
        T *d = (T *)dst;
        return map_vec(n, st, [=] __device__(int64_t i) { d[i] = (T)(src[i] / div); });
    });
}
static int div_vec(int dtype, void *v, int64_t n, double div, hipStream_t st)
{
    return by_dtype(dtype, [&](auto t) {
        using T = decltype(t);
        T *x = (T *)v;
        return map_vec(n, st, [=] __device__(int64_t i) { x[i] = (T)((double)x[i] / div); });
    });
}

// out[i, j] = sum_p P[p sP + i ldp + j], j <= i: the partial accumulators of the depth slices, p ascending, f64, one rounding.
// minus_from (n x ldo, or null; may be out): out[i, j] = minus_from[i, j] - that sum, the subtraction in f64 before the rounding
int sum_slices_lower(int dtype, const void *P, int64_t ldp, int64_t sP, int slices, int64_t n, const void *minus_from, void *out, int64_t ldo,
                     hipStream_t st)
{
    return by_dtype(dtype, [&](auto t) {
        using T = decltype(t);
        const T *Pt = (const T *)P, *from = (const T *)minus_from;
        T *o = (T *)out;
        return map_rows(n, n, st, [=] __device__(int64_t i, int64_t j) {
            if (j > i) return;
            const T *p = Pt + i * ldp + j;
            double acc = 0.0;
            for (int s = 0; s < slices; ++s) acc += (double)p[(int64_t)s * sP];
            o[i * ldo + j] = from ? (T)((double)from[i * ldo + j] - acc) : (T)acc;
        });
    });
}

static int gemv_acc(int dtype, const void *G, int64_t rows, int64_t cols, int64_t ldg, const void *y, double *acc, hipStream_t st)
{
    if (rows <= 0 || cols <= 0) return GPX_OK;
    const dim3 grid((unsigned)std::min<int64_t>(rows, 1 << 20)), block(256);
    return by_dtype(dtype, [&](auto t) {
        using T = decltype(t);
        hipLaunchKernelGGL((gemv_acc_kernel<T>), grid, block, 0, st, (const T *)G, rows, cols, ldg, (const T *)y, acc);
        GPX_LAUNCH_CHECK();
        return GPX_OK;
    });
}

static int form_B(int dtype, const void *X, int64_t ldx, int64_t n, double s, void *B, int64_t ldb, double *trace_dev, hipStream_t st)
{
    if (n <= 0) return GPX_OK;
    const dim3 grid((unsigned)cdiv(n, 256), (unsigned)std::min<int64_t>(n, 32768) + 1), block(256);
    return by_dtype(dtype, [&](auto t) {
        using T = decltype(t);
        hipLaunchKernelGGL((form_B_kernel<T>), grid, block, 0, st, (const T *)X, ldx, n, s * s, (T *)B, ldb, trace_dev);
        GPX_LAUNCH_CHECK();
        return GPX_OK;
    });
}

// out_dev[i] = kdiag(i) - sum V^2 + sum W^2: the row sums here (into acc_dev, rows doubles), kdiag and the subtraction by var_finish (gpx_solve.hip), which
// evaluates k(xo_i, xo_i) as gpx_d_kmat does on its diagonal
static int var_rows2(int dtype, int kernel, const void *V, const void *W, int64_t rows, int64_t n, int64_t ldx, const void *xo, int d,
                     const double *params, double *acc_dev, double *out_dev, hipStream_t st)
{
    if (rows <= 0) return GPX_OK;
    {
        ProfScope prof(PC_REDUCE, 2.0 * (double)rows * (double)n * (double)esize(dtype), st);
        const dim3 grid((unsigned)std::min<int64_t>(rows, 1 << 20)), block(256);
        GPX_TRY(by_dtype(dtype, [&](auto t) {
            using T = decltype(t);
            hipLaunchKernelGGL((rows2_kernel<T>), grid, block, 0, st, (const T *)V, (const T *)W, rows, n, ldx, acc_dev);
            GPX_LAUNCH_CHECK();
            return GPX_OK;
        }));
    }
    return var_finish(dtype, kernel, xo, d, params, acc_dev, rows, out_dev, st);
}

// ---- the handle ----------------------------------------------------------------------------------------------------------
struct SgpView { int kernel; const void *x, *z; const double *params; };
static inline SgpView sgp_view(const gpx_sgp *g)
{
    if (g->kernel == GPX_KERNEL_GAUSSIAN_ARD) return {GPX_KERNEL_GAUSSIAN, g->xs, g->zs, g->iso};
    return {g->kernel, g->x, g->z, g->params};
}

static int sgp_read_info(gpx_sgp *g, int which, int *info)
{
    GPX_HIP(hipMemcpyAsync(info, which == 1 ? &g->scal->info1 : &g->scal->info2, sizeof(int), hipMemcpyDeviceToHost, g->st));
    GPX_HIP(hipStreamSynchronize(g->st));
    return check_internal_info(*info);
}

static void sgp_unfit(gpx_sgp *g) { g->fitted = g->have_grad = g->have_zgrad = false; g->stage = g->pivot = 0; }

// the work buffer of a fit: G (M x cols) | the partial accumulators (slices x M x ldm, p_bytes together)
struct SgpFitLayout { size_t G, Pacc, p_bytes, total; };
constexpr SgpFitLayout sgp_fit_layout(int64_t M, int64_t ldm, int64_t cols, int slices, size_t es)
{
    Carve k;
    const size_t p_bytes = (size_t)slices * M * ldm * es, G = k.take((size_t)M * cols * es), Pacc = k.take(p_bytes);
    return {G, Pacc, p_bytes, k.total()};
}

enum { FIT_KUU, FIT_BUILD, FIT_GRAM, FIT_TAIL, FIT_TOTAL };

// a fit that ends here, its times with it: at the failed factorisation of `stage`, or at the end (stage 0)
static int sgp_fit_ends(gpx_sgp *g, int stage, int pivot)
{
    GPX_HIP(hipStreamSynchronize(g->st));
    GPX_TRY(g->tl.resolve(g->fit_ms, 5, FIT_TOTAL));
    g->stage = stage; g->pivot = pivot; g->fitted = true;
    return GPX_OK;
}

static int sgp_fit(gpx_sgp *g, int64_t chunk_cols)
{
    const int dtype = g->dtype;
    const size_t es = esize(dtype);
    const int64_t n = g->n, M = g->m, ldm = g->ldm;
    hipStream_t st = g->st;
    SgpTimeline &tl = g->tl.begin();
    sgp_unfit(g);
    // the plan and its buffer, before anything is enqueued
    size_t freeb = 0, totalb = 0;
    GPX_HIP(hipMemGetInfo(&freeb, &totalb));
    SgpPlan pl;
    GPX_TRY(sgp_plan(SGP_FIT, dtype, n, M, chunk_cols, g->split, freeb + g->work.bytes, &pl));
    const int64_t cols = pl.cols, chunks = pl.chunks, W = pl.slice_cols, sP = M * ldm;
    const SgpFitLayout lay = sgp_fit_layout(M, ldm, cols, pl.slices, es);
    GPX_TRY(g->work.reserve(lay.total, st));
    char *G = (char *)g->work.p + lay.G, *Pacc = (char *)g->work.p + lay.Pacc;
    if (g->kernel == GPX_KERNEL_GAUSSIAN_ARD) {
        ard_iso(g->params, g->d, g->iso);
        GPX_TRY(scale_points(dtype, g->x, n, g->d, g->params + 1, g->xs, st));
        GPX_TRY(scale_points(dtype, g->z, M, g->d, g->params + 1, g->zs, st));
    }
    const SgpView v = sgp_view(g);
    GPX_HIP(hipMemsetAsync(g->scal, 0, sizeof(SgpScal), st));
    GPX_TRY(tl.mark(st, SGP_NOBODY));
    // 1. Kuu and its factor
    GPX_TRY(kmat(dtype, v.kernel, GPX_K, v.z, M, v.z, M, g->d, v.params, g->jitter, GPX_LOWER, g->Luu, ldm, st));
    GPX_TRY(potrf(dtype, g->Luu, M, ldm, &g->scal->info1, st));
    GPX_TRY(tril(dtype, g->Luu, M, ldm, st));
    GPX_TRY(tl.mark(st, FIT_KUU));
    int info = 0;
    GPX_TRY(sgp_read_info(g, 1, &info));
    if (info != 0) return sgp_fit_ends(g, 1, info);        // (two marks: total == kuu, the rest 0)
    // 2. the chunk loop: Phi's partials, b
    GPX_HIP(hipMemsetAsync(Pacc, 0, lay.p_bytes, st));
    GPX_HIP(hipMemsetAsync(g->bacc, 0, (size_t)M * sizeof(double), st));
    for (int64_t c = 0; c < chunks; ++c) {
        const int64_t c0 = c * cols, cc = std::min(cols, n - c0);
        route_hit(RT_SPARSE_CHUNK);
        GPX_TRY(tl.mark(st, SGP_NOBODY));
        GPX_TRY(kmat(dtype, v.kernel, GPX_K, v.z, M, (const char *)v.x + (size_t)c0 * g->d * es, cc, g->d, v.params, 0.0, GPX_FULL, G, cols, st));
        GPX_TRY(tl.mark(st, FIT_BUILD));
        const int64_t nfull = cc / W, tail = cc - nfull * W;
        {
            ProfScope prof(PC_SPARSE_GRAM, (double)cc * (double)M * (double)(M + 1), st);     // 2 cc flops per element of the lower triangle
            if (nfull > 0) {
                Batch bt; bt.count = (int)nfull; bt.sA = W; bt.sB = W; bt.sC = sP;
                GPX_TRY(gemm_nt(dtype, M, M, W, G, cols, G, cols, Pacc, ldm, 1.0, GPX_LOWER, 0, 0, st, 0, 0, &bt));
            }
            if (tail > 0) {
                const char *Gt = G + (size_t)nfull * W * es;
                GPX_TRY(gemm_nt(dtype, M, M, tail, Gt, cols, Gt, cols, Pacc + (size_t)nfull * sP * es, ldm, 1.0, GPX_LOWER, 0, 0, st));
            }
        }
        GPX_TRY(gemv_acc(dtype, G, M, cc, cols, (const char *)g->y + (size_t)c0 * es, g->bacc, st));
        GPX_TRY(tl.mark(st, FIT_GRAM));
    }
    GPX_HIP(hipMemsetAsync(g->Phi, 0, (size_t)M * ldm * es, st));
    GPX_TRY(sum_slices_lower(dtype, Pacc, ldm, sP, pl.slices, M, nullptr, g->Phi, ldm, st));
    GPX_TRY(tl.mark(st, FIT_GRAM));                         // (the slice sum)
    // 3. the M x M tail
    GPX_TRY(dot(dtype, g->y, g->y, n, &g->scal->yy, st));
    // k(0): the first inducing point against itself, through the variance's finishing pass with a zero sum
    GPX_TRY(var_finish(dtype, v.kernel, v.z, g->d, v.params, &g->scal->zero, 1, &g->scal->k00, st));
    GPX_HIP(hipMemcpyAsync(g->Xf, g->Phi, (size_t)M * ldm * es, hipMemcpyDeviceToDevice, st));
    GPX_TRY(transpose(dtype, g->Xf, ldm, M, M, g->Xf, ldm, 1, st));               // mirror: Phi, full
    GPX_TRY(trsm_right_lt(dtype, g->Luu, M, ldm, g->Xf, M, ldm, st));               // Phi Luu^-T
    GPX_TRY(transpose(dtype, g->Xf, ldm, M, M, g->Xt, ldm, 0, st));               // Luu^-1 Phi
    GPX_TRY(trsm_right_lt(dtype, g->Luu, M, ldm, g->Xt, M, ldm, st));               // X = Luu^-1 Phi Luu^-T
    GPX_TRY(form_B(dtype, g->Xt, ldm, M, g->s, g->LB, ldm, &g->scal->trX, st));
    GPX_TRY(potrf(dtype, g->LB, M, ldm, &g->scal->info2, st));
    GPX_TRY(tril(dtype, g->LB, M, ldm, st));
    GPX_TRY(sgp_read_info(g, 2, &info));
    if (info != 0) {
        GPX_TRY(tl.mark(st, FIT_TAIL));                     // (the tail up to the failed factorisation)
        return sgp_fit_ends(g, 2, info);
    }
    // c = LB^-1 Luu^-1 b / s   (trsv_lower destroys its right-hand side)
    GPX_TRY(cvt_div(dtype, g->bacc, g->t0, M, 1.0, st));
    GPX_TRY(trsv_lower(dtype, g->Luu, M, ldm, g->t0, g->t1, 0, st));
    GPX_TRY(trsv_lower(dtype, g->LB, M, ldm, g->t1, g->cvec, 0, st));
    GPX_TRY(div_vec(dtype, g->cvec, M, g->s, st));
    // w = Luu^-T LB^-T c / s
    GPX_HIP(hipMemcpyAsync(g->t0, g->cvec, (size_t)M * es, hipMemcpyDeviceToDevice, st));
    GPX_TRY(trsv_lower(dtype, g->LB, M, ldm, g->t0, g->t1, 1, st));
    GPX_TRY(trsv_lower(dtype, g->Luu, M, ldm, g->t1, g->w, 1, st));
    GPX_TRY(div_vec(dtype, g->w, M, g->s, st));
    GPX_TRY(logdet_chol(dtype, g->LB, M, ldm, &g->scal->logdetB, st));
    GPX_TRY(dot(dtype, g->cvec, g->cvec, M, &g->scal->cc, st));
    GPX_TRY(tl.mark(st, FIT_TAIL));
    GPX_HIP(hipMemcpyAsync(&g->host, g->scal, sizeof(SgpScal), hipMemcpyDeviceToHost, st));
    return sgp_fit_ends(g, 0, 0);
}

// the test points of mean, var and cov on the device, scaled for the ARD family; m == 0: nothing to do
static int sgp_stage_points(gpx_sgp *g, const double *xo, int64_t m, const double *out, DevBuf *dxo)
{
    if (!(m >= 0 && (m == 0 || (xo && out)))) { set_error("sparse prediction: bad arguments"); return GPX_ERR_ARG; }
    if (m == 0) return GPX_OK;
    GPX_TRY(dxo->alloc((size_t)m * g->d * esize(g->dtype)));
    GPX_TRY(upload_f64(g->dtype, dxo->p, m * g->d, xo, m * g->d, 1, m * g->d, g->st));
    if (g->kernel == GPX_KERNEL_GAUSSIAN_ARD) GPX_TRY(scale_points(g->dtype, dxo->p, m, g->d, g->params + 1, dxo->p, g->st));
    return GPX_OK;
}

// V = K(xo_c, z) Luu^-T and W = V LB^-T of `rows` test points (rows x ldm each), enqueued on the handle's stream
static int sgp_two_blocks(gpx_sgp *g, const void *xo_c, int64_t rows, void *V, void *W)
{
    const SgpView v = sgp_view(g);
    const int64_t M = g->m, ldm = g->ldm;
    GPX_TRY(kmat(g->dtype, v.kernel, GPX_K, xo_c, rows, v.z, M, g->d, v.params, 0.0, GPX_FULL, V, ldm, g->st));
    GPX_TRY(trsm_right_lt(g->dtype, g->Luu, M, ldm, V, rows, ldm, g->st));
    GPX_HIP(hipMemcpyAsync(W, V, (size_t)rows * ldm * esize(g->dtype), hipMemcpyDeviceToDevice, g->st));
    return trsm_right_lt(g->dtype, g->LB, M, ldm, W, rows, ldm, g->st);
}

// ---- the gradient of the bound in (kernel parameters..., s) -----------------------------------------------------------------
// A[i, j] -= v[i] v[j], all of an n x n block
static int sub_outer(int dtype, void *A, int64_t n, int64_t lda, const void *v, hipStream_t st)
{
    return by_dtype(dtype, [&](auto t) {
        using T = decltype(t);
        T *a = (T *)A;
        const T *x = (const T *)v;
        return map_rows(n, n, st, [=] __device__(int64_t i, int64_t j) { a[i * lda + j] = (T)((double)a[i * lda + j] - (double)x[i] * (double)x[j]); });
    });
}

// C (m x n) = alpha A B^T: C is not read where the product kernel's aligned route can start from zero, cleared first elsewhere
static int product_nt(int dtype, int64_t m, int64_t n, int64_t k, const void *A, const void *B, void *C, int64_t ld, double alpha,
                      hipStream_t st)
{
    const bool beta0 = !tune().gemm_no_fast && k % (128 / (int64_t)esize(dtype)) == 0;
    if (!beta0) GPX_HIP(hipMemsetAsync(C, 0, (size_t)m * ld * esize(dtype), st));
    return gemm_nt(dtype, m, n, k, A, ld, B, ld, C, ld, alpha, GPX_FULL, 0, 0, st, beta0 ? 1 : 0);
}

// the work buffer of a gradient pass: the reduction's partials (part_doubles of them and the 8 w . b sits in) | Y A Tm
// (M x ldm) | G P (cols x ldm), and with_z: the M x d accumulator (f64) | -w | zpart_doubles partials of the z kernel (a
// function of M and d: the passes on x and on z share them).  Mm aliases Y, which is done with when Mm is formed.
struct SgpGradLayout { size_t part, Y, A, Tm, G, P, zacc, negw, zpart, total; };
constexpr SgpGradLayout sgp_grad_layout(int64_t M, int64_t ldm, int64_t cols, int d, size_t es, size_t part_doubles, bool with_z,
                                        size_t zpart_doubles)
{
    const size_t mm = (size_t)M * ldm * es, blk = (size_t)cols * ldm * es;
    Carve k;
    const size_t part = k.take((part_doubles + 8) * 8), Y = k.take(mm), A = k.take(mm), Tm = k.take(mm), G = k.take(blk), P = k.take(blk);
    const size_t zacc = with_z ? k.take((size_t)M * d * 8) : 0, negw = with_z ? k.take((size_t)ldm * es) : 0;
    const size_t zpart = with_z ? k.take(zpart_doubles * 8) : 0;
    return {part, Y, A, Tm, G, P, zacc, negw, zpart, k.total()};
}

enum { GRAD_MM, GRAD_BUILD, GRAD_PRODUCT, GRAD_REDUCE, GRAD_TOTAL, ZGRAD_KUU, ZGRAD_CHUNKS, GRAD_BUCKETS };

// grad (may be null when grad_z is not): (kernel parameters..., s).  grad_z (HOST, M x d, or null): the gradient in the inducing
// inputs from the same pass; null leaves the pass exactly the theta-only one -- the same launches, the same bits
static int sgp_grad(gpx_sgp *g, int64_t chunk_cols, double *grad, double *grad_z)
{
    const int dtype = g->dtype, d = g->d, nkp = g->nparams;
    const size_t es = esize(dtype);
    const int64_t n = g->n, M = g->m, ldm = g->ldm;
    hipStream_t st = g->st;
    const bool ard = g->kernel == GPX_KERNEL_GAUSSIAN_ARD;
    g->have_grad = false; g->have_zgrad = false;
    double grad_own[GPX_ARD_MAX_D + 2];
    if (!grad) grad = grad_own;
    // the plan: the fit's, with two c x ldm blocks where the fit has one M x c
    size_t freeb = 0, totalb = 0;
    GPX_HIP(hipMemGetInfo(&freeb, &totalb));
    SgpPlan pl;
    GPX_TRY(sgp_plan(SGP_GRAD, dtype, n, M, chunk_cols, g->split, freeb + g->work.bytes, &pl));
    const int64_t cols = pl.cols, chunks = pl.chunks;
    const SgpView v = sgp_view(g);
    const size_t part_doubles = dloglh_partial_doubles(g->kernel, d), mm = (size_t)M * ldm * es;
    const SgpGradLayout lay = sgp_grad_layout(M, ldm, cols, d, es, part_doubles, grad_z != nullptr,
                                              grad_z ? rect_zgrad_partial_doubles(v.kernel, M, d) : 0);
    GPX_TRY(g->work.reserve(lay.total, st));
    char *base = (char *)g->work.p;
    double *part = (double *)(base + lay.part), *wb_dev = part + part_doubles;
    char *Y = base + lay.Y, *A = base + lay.A, *Tm = base + lay.Tm, *G = base + lay.G, *P = base + lay.P, *Mm = Y, *negw = base + lay.negw;
    double *zacc = (double *)(base + lay.zacc), *zpart = (double *)(base + lay.zpart);
    const double *col_div = ard ? g->params + 1 : nullptr;                           // (the scaled points: d/dz_ik = d/dzs_ik / w_k)
    void *X1 = g->Xf;                                                                // (work of the fit: nobody reads it afterwards)
    SgpTimeline &tl = g->tl.begin();
    const double s = g->s, s2 = s * s, N = (double)n;

    // 1. the M x M part.  Neither Kuu^-1 - Sigma^-1 nor Gu is formed as a difference: in the directions the data do not
    // reach (X ~ 0: those of Kuu's small eigenvalues, where Kuu^-1 is largest) the terms of both cancel, and in fp32 the
    // difference of two inverses of size 1 / jitter is rounding error as large as what is left.  With B - I = X / s^2,
    // Y = Luu^-T LB^-T and A = Luu^-T X LB^-T:
    //   Kuu^-1 - Sigma^-1 = Luu^-T (I - B^-1) Luu^-1 = Luu^-T (X / s^2) B^-1 Luu^-1 = A Y^T / s^2
    //   Gu = Luu^-T (I - B^-1 - X / s^2) Luu^-1 / 2 - w w^T / 2 = -(A A^T / s^4 + w w^T) / 2     (I - B^-1 - (B - I) = -(B - I)^2 B^-1)
    GPX_TRY(tl.mark(st, SGP_NOBODY));
    GPX_TRY(eye_rows(dtype, X1, M, ldm, 0, 0, st));
    GPX_TRY(trsm_right_lt(dtype, g->Luu, M, ldm, X1, M, ldm, st, 1));                 // X1 = Luu^-T
    GPX_HIP(hipMemcpyAsync(Y, X1, mm, hipMemcpyDeviceToDevice, st));
    GPX_TRY(trsm_right_lt(dtype, g->LB, M, ldm, Y, M, ldm, st));                      // Y = Luu^-T LB^-T
    GPX_TRY(product_nt(dtype, M, M, M, X1, g->Xt, A, ldm, 1.0, st));                  // Luu^-T X  (X is symmetric)
    GPX_TRY(trsm_right_lt(dtype, g->LB, M, ldm, A, M, ldm, st));                      // A = Luu^-T X LB^-T
    GPX_TRY(product_nt(dtype, M, M, M, A, Y, Tm, ldm, 1.0 / s2, st));                 // Kuu^-1 - Sigma^-1
    GPX_TRY(sub_outer(dtype, Tm, M, ldm, g->w, st));                                  // T
    GPX_HIP(hipMemsetAsync(Mm, 0, mm, st));
    GPX_TRY(gemm_nt(dtype, M, M, M, A, ldm, A, ldm, Mm, ldm, -1.0 / (s2 * s2), GPX_LOWER, 0, 0, st));   // w w^T - Mm = -2 Gu
    GPX_TRY(cvt_div(dtype, g->bacc, g->t0, M, 1.0, st));
    GPX_TRY(dot(dtype, g->w, g->t0, M, wb_dev, st));                                  // w . b
    // sum (w w^T - Mm) o dKuu = -2 sum Gu o dKuu: the dense gradient's pass on z
    double Suu[GPX_ARD_MAX_D + 2], Srect[GPX_ARD_MAX_D + 2], out[GPX_ARD_MAX_D + 2], wb = 0.0;
    GPX_TRY(tile_reduce(dtype, g->kernel, v.z, M, d, v.params, g->w, nullptr, Mm, ldm, part, Suu, st));
    GPX_HIP(hipMemcpyAsync(&wb, wb_dev, sizeof(double), hipMemcpyDeviceToHost, st));
    GPX_TRY(tl.mark(st, GRAD_MM));
    if (grad_z) {
        // Kuu's share, sum_i' 2 Gu[i, i'] dk(z_i, z_i')/dz_ik with 2 Gu = Mm - w w^T: the same kernel on z against itself, C = Mm
        // mirrored to a full matrix, (u, v) = (-w, w).  The pair i' = i adds exactly 0: its difference is 0.
        GPX_HIP(hipMemsetAsync(zacc, 0, (size_t)M * d * sizeof(double), st));
        GPX_HIP(hipMemcpyAsync(negw, g->w, (size_t)M * es, hipMemcpyDeviceToDevice, st));
        GPX_TRY(div_vec(dtype, negw, M, -1.0, st));
        GPX_TRY(transpose(dtype, Mm, ldm, M, M, Mm, ldm, 1, st));
        GPX_TRY(rect_zgrad(dtype, v.kernel, v.z, M, v.z, M, d, v.params, Mm, ldm, negw, g->w, 1.0, col_div, zpart, zacc, st));
        GPX_TRY(tl.mark(st, ZGRAD_KUU));
    }

    // 2. the pass over x: sum_ji (P[j, i] + y_j w_i) dk(x_j, z_i), P = K(x_c, z) T
    const int width = ard ? d + 2 : 4;
    for (int q = 0; q < width; ++q) Srect[q] = 0.0;
    for (int64_t c = 0; c < chunks; ++c) {
        const int64_t c0 = c * cols, cc = std::min(cols, n - c0);
        const char *xc = (const char *)v.x + (size_t)c0 * d * es;
        route_hit(RT_SPARSE_CHUNK);
        GPX_TRY(tl.mark(st, SGP_NOBODY));
        GPX_TRY(kmat(dtype, v.kernel, GPX_K, xc, cc, v.z, M, d, v.params, 0.0, GPX_FULL, G, ldm, st));
        GPX_TRY(tl.mark(st, GRAD_BUILD));
        GPX_TRY(product_nt(dtype, cc, M, M, G, Tm, P, ldm, 1.0, st));                 // (T is symmetric)
        GPX_TRY(tl.mark(st, GRAD_PRODUCT));
        if (grad_z) {
            // Gf's share on the same G, P: sum_j (P[j, i] + y_j w_i) dk(z_i, x_j)/dz_ik / s^2, ahead of the reduction, whose
            // host sum waits for the stream
            GPX_TRY(rect_zgrad(dtype, v.kernel, xc, cc, v.z, M, d, v.params, P, ldm, (const char *)g->y + (size_t)c0 * es, g->w, 1.0 / s2,
                               col_div, zpart, zacc, st));
            GPX_TRY(tl.mark(st, ZGRAD_CHUNKS));
        }
        GPX_TRY(rect_reduce(dtype, g->kernel, xc, cc, v.z, M, d, v.params, P, ldm, (const char *)g->y + (size_t)c0 * es, g->w, part, out, st));
        GPX_TRY(tl.mark(st, GRAD_REDUCE));                                          // (behind the z kernels when they run)
        for (int q = 0; q < width; ++q) Srect[q] += out[q];
    }
    GPX_TRY(tl.mark(st, SGP_NOBODY));
    if (grad_z) GPX_HIP(hipMemcpyAsync(grad_z, zacc, (size_t)M * d * sizeof(double), hipMemcpyDeviceToHost, st));
    GPX_HIP(hipStreamSynchronize(st));

    // 3. the gradient from the sums.  k(0) = k00 depends on h (and the Gaussian families' on the widths): dk(0)/dh = 2 k(0) / h,
    // Gaussian dk(0)/dw = -k(0) / w; the ARD family's share is the term t = 0 of its sums
    const double k00 = g->host.k00, h = g->params[0];
    if (ard) {
        double S[GPX_ARD_MAX_D + 2];
        for (int q = 0; q <= d; ++q) S[q] = -0.5 * Suu[q] + Srect[q] / s2;
        S[0] -= 0.5 * N * k00 / s2;
        S[d + 1] = 0.0;
        grad_from_sums(g->kernel, d, g->params, S, 0.0, 0.0, 1.0, grad);
    } else {
        for (int p = 0; p < nkp; ++p) grad[p] = -0.5 * Suu[p] + Srect[p] / s2;
        grad[0] -= 0.5 * N * (2.0 * k00 / h) / s2;
        if (g->kernel == GPX_KERNEL_GAUSSIAN) grad[1] += 0.5 * N * (k00 / g->params[1]) / s2;
    }
    const double sumk = ard ? Srect[0] : Srect[3];                                   // tr(T Phi) + w . b
    grad[nkp] = -N / s + (((g->host.yy - wb) - sumk) + N * k00) / (s2 * s);

    float ms[GRAD_BUCKETS];
    GPX_TRY(tl.resolve(ms, GRAD_BUCKETS, GRAD_TOTAL));
    std::copy(ms, ms + 5, g->grad_ms);
    std::copy(ms + ZGRAD_KUU, ms + GRAD_BUCKETS, g->zgrad_ms);
    g->have_grad = true;
    g->have_zgrad = grad_z != nullptr;
    return GPX_OK;
}

}  // namespace gpx

using namespace gpx;

#define SGP_ENTER(g)                                                         \
    GPX_ARG((g) != nullptr, "handle is NULL");                               \
    gpx::tune_refresh();                                                     \
    gpx::DeviceGuard guard__((g)->device);                                   \
    if (guard__.rc != GPX_OK) return guard__.rc;                             \
    gpx::StreamTurn turn__((g)->st);                                         \
    gpx::RoctxRange api_range__(__func__)

#define SGP_NEED_FIT(g)                                                                                              \
    do {                                                                                                             \
        GPX_ARG((g)->fitted, "the sparse GP is not fitted");                                                         \
        if ((g)->stage != 0) {                                                                                       \
            gpx::set_error("%s: %s is not positive definite (stage %d, info = %d): there is nothing to predict from", __func__, \
                           (g)->stage == 1 ? "Kuu" : "B", (g)->stage, (g)->pivot);                                   \
            return GPX_ERR_ARG;                                                                                      \
        }                                                                                                            \
    } while (0)

extern "C" {

int gpx_sgp_create(gpx_sgp_t **out, int dtype, int kernel, int64_t n, int64_t m_inducing, int d)
{
    GPX_TRY(ensure_device());
    GPX_ARG(out, "handle is NULL");
    *out = nullptr;
    GPX_ARG(dtype == GPX_F64 || dtype == GPX_F32, "dtype must be GPX_F64 or GPX_F32");
    GPX_ARG(kernel == GPX_KERNEL_GAUSSIAN || kernel == GPX_KERNEL_PERIODIC || kernel == GPX_KERNEL_GAUSSIAN_ARD, "unknown kernel family");
    GPX_ARG(n >= 1 && m_inducing >= 1 && d >= 1, "need n >= 1, m_inducing >= 1 and d >= 1");
    GPX_ARG(kernel != GPX_KERNEL_GAUSSIAN_ARD || d <= GPX_ARD_MAX_D, "the ARD family needs d <= GPX_ARD_MAX_D");
    gpx_sgp *g = new gpx_sgp();
    g->dtype = dtype; g->kernel = kernel; g->n = n; g->m = m_inducing; g->d = d;
    if (hipGetDevice(&g->device) != hipSuccess) { (void)hipGetLastError(); g->device = 0; }
    g->nparams = nparams_of(kernel, d);
    g->ldm = round_up(m_inducing, 16);
    const size_t es = esize(dtype), mm = (size_t)m_inducing * g->ldm * es, mv = (size_t)g->ldm * es;
    int rc = GPX_OK;
#define SGP_ALLOC(field, bytes) if (rc == GPX_OK) rc = dev_alloc((void **)&g->field, (bytes), "hipMalloc " #field)
    SGP_ALLOC(x, (size_t)n * d * es);
    SGP_ALLOC(y, (size_t)n * es);
    SGP_ALLOC(z, (size_t)m_inducing * d * es);
    if (kernel == GPX_KERNEL_GAUSSIAN_ARD) { SGP_ALLOC(xs, (size_t)n * d * es); SGP_ALLOC(zs, (size_t)m_inducing * d * es); }
    SGP_ALLOC(Luu, mm); SGP_ALLOC(Phi, mm); SGP_ALLOC(Xf, mm); SGP_ALLOC(Xt, mm); SGP_ALLOC(LB, mm);
    SGP_ALLOC(cvec, mv); SGP_ALLOC(w, mv); SGP_ALLOC(t0, mv); SGP_ALLOC(t1, mv);
    SGP_ALLOC(bacc, (size_t)m_inducing * sizeof(double));
    SGP_ALLOC(scal, sizeof(SgpScal));
#undef SGP_ALLOC
    if (rc == GPX_OK) {                                        // (the events: the timeline makes them as a pass first needs them)
        const hipError_t e = hipStreamCreateWithFlags(&g->st, hipStreamNonBlocking);
        if (e != hipSuccess) rc = hip_fail(e, "hipStreamCreate", __FILE__, __LINE__);
    }
    if (rc != GPX_OK) { gpx_sgp_destroy(g); return rc; }
    *out = g;
    return GPX_OK;
}

int gpx_sgp_destroy(gpx_sgp_t *g)
{
    if (!g) return GPX_OK;
    gpx::DeviceGuard guard__(g->device);
    if (g->st) (void)hipStreamSynchronize(g->st);
    stream_epoch_bump();                                       // (StreamTurn: a later stream at this one's address is a different stream)
    for (void *b : {g->x, g->y, g->z, g->xs, g->zs, g->Luu, g->Phi, g->Xf, g->Xt, g->LB, g->cvec, g->w, g->t0, g->t1, (void *)g->bacc,
                    (void *)g->scal})
        dev_free(b);
    g->work.release();
    for (hipEvent_t e : g->tl.pool) (void)hipEventDestroy(e);
    if (g->st) (void)hipStreamDestroy(g->st);
    delete g;
    return GPX_OK;
}

int gpx_sgp_set_data(gpx_sgp_t *g, const double *x, const double *y, const double *z)
{
    SGP_ENTER(g);
    sgp_unfit(g);
    if (x) { GPX_TRY(upload_f64(g->dtype, g->x, g->n * g->d, x, g->n * g->d, 1, g->n * g->d, g->st)); g->have_x = true; }
    if (y) { GPX_TRY(upload_f64(g->dtype, g->y, g->n, y, g->n, 1, g->n, g->st)); g->have_y = true; }
    if (z) { GPX_TRY(upload_f64(g->dtype, g->z, g->m * g->d, z, g->m * g->d, 1, g->m * g->d, g->st)); g->have_z = true; }
    return GPX_OK;
}

int gpx_sgp_fit(gpx_sgp_t *g, const double *params, double s, double jitter, int64_t chunk_cols, int *stage, int *pivot)
{
    SGP_ENTER(g);
    GPX_ARG(params && stage && pivot, "NULL argument");
    GPX_ARG(g->have_x && g->have_y && g->have_z, "no data in the handle (gpx_sgp_set_data)");
    GPX_ARG(s > 0.0 && s <= 1.79769313486231570e308, "s must be positive and finite (the bound divides by s^2)");
    GPX_ARG(jitter >= 0.0 && jitter <= 1.79769313486231570e308, "jitter must be >= 0 and finite");
    for (int i = 0; i < g->nparams; ++i) {
        GPX_ARG(std::isfinite(params[i]), "array must not contain infs or NaNs (kernel parameters)");
        g->params[i] = params[i];
    }
    g->s = s; g->jitter = jitter;
    const int rc = sgp_fit(g, chunk_cols);
    if (rc != GPX_OK) { g->fitted = false; return rc; }
    *stage = g->stage; *pivot = g->pivot;
    return GPX_OK;
}

int gpx_sgp_info(gpx_sgp_t *g, int *stage, int *pivot)
{
    GPX_ARG(g != nullptr && stage && pivot, "NULL argument");
    GPX_ARG(g->fitted, "the sparse GP is not fitted");
    *stage = g->stage; *pivot = g->pivot;
    return GPX_OK;
}

int gpx_sgp_elbo(gpx_sgp_t *g, double *elbo, double *terms5)
{
    GPX_ARG(g != nullptr && elbo, "NULL argument");
    GPX_ARG(g->fitted, "the sparse GP is not fitted");
    double t[5];
    if (g->stage != 0) {
        for (double &v : t) v = NAN;
        *elbo = -INFINITY;
    } else {
        const SgpScal &h = g->host;
        const double s2 = g->s * g->s, N = (double)g->n;
        t[0] = -0.5 * h.logdetB;
        t[1] = -0.5 * N * log(2.0 * M_PI) - N * log(g->s);
        t[2] = -0.5 * h.yy / s2;
        t[3] = 0.5 * h.cc / s2;
        t[4] = -0.5 * (N * h.k00 - h.trX) / s2;
        *elbo = (((t[0] + t[1]) + t[2]) + t[3]) + t[4];
    }
    if (terms5) for (int i = 0; i < 5; ++i) terms5[i] = t[i];
    return GPX_OK;
}

int gpx_sgp_mean(gpx_sgp_t *g, const double *xo, int64_t m, double *out)
{
    SGP_ENTER(g);
    SGP_NEED_FIT(g);
    DevBuf dxo, dout;
    GPX_TRY(sgp_stage_points(g, xo, m, out, &dxo));
    if (m == 0) return GPX_OK;
    GPX_TRY(dout.alloc((size_t)m * esize(g->dtype)));
    const SgpView v = sgp_view(g);
    GPX_TRY(gpx_d_mean(g->dtype, v.kernel, dxo.p, m, v.z, g->m, g->d, v.params, g->w, dout.p, (void *)g->st));
    return download_f64(g->dtype, out, m, dout.p, m, 1, m, 0, g->st);
}

int gpx_sgp_var(gpx_sgp_t *g, const double *xo, int64_t m, int64_t chunk_rows, double *out)
{
    SGP_ENTER(g);
    SGP_NEED_FIT(g);
    GPX_ARG(chunk_rows >= 0 && chunk_rows % 128 == 0, "chunk_rows must be 0 (automatic) or a multiple of 128");
    size_t freeb = 0, totalb = 0;
    GPX_HIP(hipMemGetInfo(&freeb, &totalb));                   // (the plan's: before the call allocates anything)
    DevBuf dxo, V, W, dvar, dacc;
    GPX_TRY(sgp_stage_points(g, xo, m, out, &dxo));
    if (m == 0) return GPX_OK;
    const size_t es = esize(g->dtype);
    int64_t rows = 0, chunks = 0;
    GPX_TRY(var_plan(g->dtype, g->m, m, chunk_rows, freeb / 2, &rows, &chunks, nullptr));      // two blocks a chunk
    GPX_TRY(V.alloc((size_t)rows * g->ldm * es));
    GPX_TRY(W.alloc((size_t)rows * g->ldm * es));
    GPX_TRY(dvar.alloc((size_t)m * sizeof(double)));
    GPX_TRY(dacc.alloc((size_t)rows * sizeof(double)));
    const SgpView v = sgp_view(g);
    for (int64_t c = 0; c < chunks; ++c) {
        const int64_t r0 = c * rows, rc = std::min(rows, m - r0);
        route_hit(RT_VAR_CHUNK);
        const char *xo_c = (const char *)dxo.p + (size_t)r0 * g->d * es;
        GPX_TRY(sgp_two_blocks(g, xo_c, rc, V.p, W.p));
        GPX_TRY(var_rows2(g->dtype, v.kernel, V.p, W.p, rc, g->m, g->ldm, xo_c, g->d, v.params, (double *)dacc.p, (double *)dvar.p + r0, g->st));
    }
    GPX_HIP(hipMemcpyAsync(out, dvar.p, (size_t)m * sizeof(double), hipMemcpyDeviceToHost, g->st));
    GPX_HIP(hipStreamSynchronize(g->st));
    return GPX_OK;
}

int gpx_sgp_cov(gpx_sgp_t *g, const double *xo, int64_t m, double *out)
{
    SGP_ENTER(g);
    SGP_NEED_FIT(g);
    DevBuf dxo, V, W, C;
    GPX_TRY(sgp_stage_points(g, xo, m, out, &dxo));
    if (m == 0) return GPX_OK;
    const size_t es = esize(g->dtype);
    const int64_t ldc = round_up(m, 16), ldm = g->ldm;
    GPX_TRY(V.alloc((size_t)m * ldm * es));
    GPX_TRY(W.alloc((size_t)m * ldm * es));
    GPX_TRY(C.alloc((size_t)m * ldc * es));
    const SgpView v = sgp_view(g);
    GPX_TRY(sgp_two_blocks(g, dxo.p, m, V.p, W.p));
    GPX_TRY(kmat(g->dtype, v.kernel, GPX_K, dxo.p, m, dxo.p, m, g->d, v.params, 0.0, GPX_FULL, C.p, ldc, g->st));
    GPX_TRY(gemm_nt(g->dtype, m, m, g->m, V.p, ldm, V.p, ldm, C.p, ldc, -1.0, GPX_FULL, 0, 0, g->st));
    GPX_TRY(gemm_nt(g->dtype, m, m, g->m, W.p, ldm, W.p, ldm, C.p, ldc, 1.0, GPX_FULL, 0, 0, g->st));
    return download_f64(g->dtype, out, m, C.p, ldc, m, m, 0, g->st);
}

int gpx_sgp_get(gpx_sgp_t *g, double *Luu, double *LB, double *c, double *Phi, double *b)
{
    SGP_ENTER(g);
    GPX_ARG(g->fitted, "the sparse GP is not fitted");
    const int64_t M = g->m, ldm = g->ldm;
    if (Luu) GPX_TRY(download_f64(g->dtype, Luu, M, g->Luu, ldm, M, M, 1, g->st));
    if (LB) GPX_TRY(download_f64(g->dtype, LB, M, g->LB, ldm, M, M, 1, g->st));
    if (c) GPX_TRY(download_f64(g->dtype, c, M, g->cvec, M, 1, M, 0, g->st));
    if (Phi) GPX_TRY(download_f64(g->dtype, Phi, M, g->Phi, ldm, M, M, 1, g->st));
    if (b) {
        GPX_HIP(hipMemcpyAsync(b, g->bacc, (size_t)M * sizeof(double), hipMemcpyDeviceToHost, g->st));
        GPX_HIP(hipStreamSynchronize(g->st));
    }
    return GPX_OK;
}

int gpx_sgp_last_timing(gpx_sgp_t *g, float *ms5)
{
    GPX_ARG(g != nullptr && ms5, "NULL argument");
    GPX_ARG(g->fitted, "the sparse GP is not fitted");
    for (int i = 0; i < 5; ++i) ms5[i] = g->fit_ms[i];
    return GPX_OK;
}

int gpx_sgp_grad(gpx_sgp_t *g, int64_t chunk_cols, double *grad)
{
    SGP_ENTER(g);
    SGP_NEED_FIT(g);
    GPX_ARG(grad, "NULL argument");
    return sgp_grad(g, chunk_cols, grad, nullptr);
}

int gpx_sgp_grad_z(gpx_sgp_t *g, int64_t chunk_cols, double *grad, double *grad_z)
{
    SGP_ENTER(g);
    SGP_NEED_FIT(g);
    GPX_ARG(grad_z, "NULL argument");
    return sgp_grad(g, chunk_cols, grad, grad_z);
}

int gpx_sgp_last_zgrad_timing(gpx_sgp_t *g, float *ms2)
{
    GPX_ARG(g != nullptr && ms2, "NULL argument");
    GPX_ARG(g->fitted && g->have_zgrad, "no gradient in z of the current fit (gpx_sgp_grad_z)");
    for (int i = 0; i < 2; ++i) ms2[i] = g->zgrad_ms[i];
    return GPX_OK;
}

int gpx_sgp_last_grad_timing(gpx_sgp_t *g, float *ms5)
{
    GPX_ARG(g != nullptr && ms5, "NULL argument");
    GPX_ARG(g->fitted && g->have_grad, "no gradient of the current fit (gpx_sgp_grad)");
    for (int i = 0; i < 5; ++i) ms5[i] = g->grad_ms[i];
    return GPX_OK;
}

int gpx_sgp_set_split(gpx_sgp_t *g, int slices)
{
    GPX_ARG(g != nullptr, "handle is NULL");
    GPX_ARG(slices >= 0, "slices must be >= 0");
    g->split = slices;
    sgp_unfit(g);
    return GPX_OK;
}

int gpx_debug_sgp_plan(int dtype, int64_t n, int64_t m_inducing, int64_t chunk_cols, int split, size_t free_bytes, int64_t *cols,
                       int64_t *chunks, int *slices, int64_t *slice_cols)
{
    SgpPlan pl;
    GPX_TRY(sgp_plan(SGP_FIT, dtype, n, m_inducing, chunk_cols, split, free_bytes, &pl));
    if (slices) *slices = pl.slices;
    if (slice_cols) *slice_cols = pl.slice_cols;
    if (cols) *cols = pl.cols;
    if (chunks) *chunks = pl.chunks;
    return GPX_OK;
}

int gpx_debug_sgp_grad_plan(int dtype, int64_t n, int64_t m_inducing, int64_t chunk_cols, int split, size_t free_bytes, int64_t *cols,
                            int64_t *chunks)
{
    SgpPlan pl;
    GPX_TRY(sgp_plan(SGP_GRAD, dtype, n, m_inducing, chunk_cols, split, free_bytes, &pl));
    if (cols) *cols = pl.cols;
    if (chunks) *chunks = pl.chunks;
    return GPX_OK;
}

// ---- the building blocks ---------------------------------------------------------------------------------------------------
#define SGP_D_ENTER()                                                                            \
    gpx::tune_refresh();                                                                         \
    GPX_ARG(dtype == GPX_F64 || dtype == GPX_F32, "dtype must be GPX_F64 or GPX_F32")

int gpx_d_sum_slices_lower(int dtype, const void *P, int64_t ldp, int64_t sP, int slices, int64_t n, void *out, int64_t ldo, void *stream)
{
    SGP_D_ENTER();
    GPX_ARG(n >= 0 && slices >= 1, "need n >= 0 and slices >= 1");
    if (n == 0) return GPX_OK;
    GPX_ARG(P && out && P != out, "NULL pointer or out == P");
    GPX_ARG(ldp >= n && ldo >= n && sP >= 0, "leading dimension too small");
    GPX_TRY(ensure_device());
    return sum_slices_lower(dtype, P, ldp, sP, slices, n, nullptr, out, ldo, S(stream));
}

int gpx_d_gemv_acc(int dtype, const void *G, int64_t rows, int64_t cols, int64_t ldg, const void *y, double *acc_dev, void *stream)
{
    SGP_D_ENTER();
    GPX_ARG(rows >= 0 && cols >= 0, "negative dimension");
    if (rows == 0 || cols == 0) return GPX_OK;
    GPX_ARG(G && y && acc_dev, "NULL pointer");
    GPX_ARG(ldg >= cols, "leading dimension too small");
    GPX_TRY(ensure_device());
    return gemv_acc(dtype, G, rows, cols, ldg, y, acc_dev, S(stream));
}

int gpx_d_mirror_lower(int dtype, void *A, int64_t n, int64_t lda, void *stream)
{
    SGP_D_ENTER();
    GPX_ARG(n >= 0, "n < 0");
    if (n == 0) return GPX_OK;
    GPX_ARG(A && lda >= n, "NULL pointer or leading dimension too small");
    GPX_TRY(ensure_device());
    return transpose(dtype, A, lda, n, n, A, lda, 1, S(stream));
}

int gpx_d_transpose(int dtype, const void *in, int64_t ldi, void *out, int64_t ldo, int64_t n, void *stream)
{
    SGP_D_ENTER();
    GPX_ARG(n >= 0, "n < 0");
    if (n == 0) return GPX_OK;
    GPX_ARG(in && out && in != out, "NULL pointer or out == in");
    GPX_ARG(ldi >= n && ldo >= n, "leading dimension too small");
    GPX_TRY(ensure_device());
    return transpose(dtype, in, ldi, n, n, out, ldo, 0, S(stream));
}

int gpx_d_sgp_form_B(int dtype, const void *X, int64_t ldx, int64_t n, double s, void *B, int64_t ldb, double *trace_dev, void *stream)
{
    SGP_D_ENTER();
    GPX_ARG(n >= 0, "n < 0");
    if (n == 0) return GPX_OK;
    GPX_ARG(X && B && trace_dev && X != B, "NULL pointer or B == X");
    GPX_ARG(ldx >= n && ldb >= n, "leading dimension too small");
    GPX_ARG(s > 0.0, "s must be positive");
    GPX_TRY(ensure_device());
    return form_B(dtype, X, ldx, n, s, B, ldb, trace_dev, S(stream));
}

int gpx_d_var_rows2(int dtype, int kernel, const void *V, const void *W, int64_t rows, int64_t n, int64_t ldx, const void *xo, int d,
                    const double *params, double *out_dev, void *stream)
{
    SGP_D_ENTER();
    GPX_ARG(rows >= 0 && n >= 0, "negative dimension");
    if (rows == 0) return GPX_OK;
    GPX_ARG(V && W && xo && params && out_dev && d >= 1, "NULL pointer or d < 1");
    GPX_ARG(ldx >= n, "leading dimension too small");
    GPX_ARG(kernel == GPX_KERNEL_GAUSSIAN || kernel == GPX_KERNEL_PERIODIC, "unknown kernel family (the ARD family: scaled points and the isotropic constants)");
    GPX_TRY(ensure_device());
    DevBuf acc;                                            // the row sums; the call waits for the stream before it frees them
    GPX_TRY(acc.alloc((size_t)rows * sizeof(double)));
    GPX_TRY(var_rows2(dtype, kernel, V, W, rows, n, ldx, xo, d, params, (double *)acc.p, out_dev, S(stream)));
    GPX_HIP(hipStreamSynchronize(S(stream)));
    return GPX_OK;
}

}  // extern "C"
