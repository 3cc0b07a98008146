// gpx_loograd.hip -- the gradient of the leave-one-out criterion (gpx_gp_loo_grad, gpx_gp_loo_grad_weights).
//
// With W = K^-1, alpha = W y and k_i = W_ii the criterion is  L = sum_i ( log k_i / 2 - alpha_i^2 / (2 k_i) - log(2 pi) / 2 )
// (RW06 eq. 5.10 - 5.12; gpx_gp_loo sums it).  From dW = -W dK W:  dk_i = -(W dK W)_ii,  dalpha = -W dK alpha,  so
//   dL = sum_i [ -c_i (W dK W)_ii + (alpha_i / k_i) (W dK alpha)_i ],      c_i = (1 + alpha_i^2 / k_i) / (2 k_i)  > 0
//      = sum_ab dK_ab G_ab,      G = (r alpha^T + alpha r^T) / 2 - Pm,     r = W (alpha / k),    Pm = W diag(c) W
// which is RW06 eq. 5.13 with the products regrouped: eq. 5.13 as printed takes one n^3 product W dK_j per parameter, this
// form ONE for all of them -- Pm = Y Y^T with Y = W diag(sqrt(c)), a symmetric product, lower triangle only -- and then a
// single fused pass, tile_reduce (gpx_kmat.hip) with two vectors, over (alpha, r, Pm) against the kernel derivatives evaluated on the fly.
// Noise: dK/ds = 2 s I, so dL/ds = 2 s tr G = 2 s (r . alpha - tr Pm).
//
// Memory: the two n x ldl blocks the marginal-likelihood gradient uses and no third.  X = L^-T is dead once k has been read
// from its rows, so Y is written over it; W is dead once Y exists, so Pm is written over W.  No explicit G on this route
// (gpx_gp_loo_grad_weights forms one, in float64, for the caller who asked for it).
// k is read from the rows of X -- k_i = |row i of L^-T|^2, float64 sums, the very kernel gpx_gp_loo's sweep ends with --
// rather than from the diagonal of W, so the value that comes out of this call is gpx_gp_loo's bit for bit, in fp32 too.
#include "gpx_small.h"
#include <cmath>

#include "gpx_gp_internal.h"

namespace gpx {

static inline size_t pad256(size_t b) { return (b + 255) / 256 * 256; }

size_t loo_vec_bytes(int dtype, int64_t n) { return 2 * pad256((size_t)n * 8) + 256 + 4 * pad256((size_t)n * esize(dtype)); }

LooVecs loo_vecs_at(void *block, int dtype, int64_t n)
{
    char *p = (char *)block;
    const size_t d8 = pad256((size_t)n * 8), dt = pad256((size_t)n * esize(dtype));
    LooVecs v;
    v.kii = (double *)p; p += d8;
    v.logp = (double *)p; p += d8;
    v.sums = (double *)p; p += 256;
    v.u = p; p += dt;
    v.sq = p; p += dt;
    v.t = p; p += dt;
    v.r = p;
    return v;
}

int loo_weights_vectors(int dtype, const void *L, int64_t n, int64_t ldl, const void *y, const void *alpha, void *X, const void *W,
                        const LooVecs &v, const double *kii_have, TrsvOps *ops, hipStream_t st)
{
    // k and the per-point terms; their sum in sum_f64's fixed order, as gpx_gp_loo takes it
    const double *kii = kii_have ? kii_have : v.kii;
    if (kii_have) GPX_TRY(loo_points(dtype, kii, y, alpha, n, nullptr, nullptr, v.logp, st));
    else GPX_TRY(loo_rows(dtype, X, n, n, ldl, 0, y, alpha, v.kii, nullptr, nullptr, v.logp, st));
    GPX_TRY(sum_f64(v.logp, n, v.sums, st));
    // u = alpha / k and sqrt(c), in the system's dtype; one thread per point.  k > 0 for every factor that exists.
    GPX_TRY(by_dtype(dtype, [&](auto t) {
        using T = decltype(t);
        const T *al = (const T *)alpha;
        T *u = (T *)v.u, *sq = (T *)v.sq;
        return map_vec(n, st, [=] __device__(int64_t i) {
            const double k = kii[i], a = (double)al[i];
            const double c = 0.5 * (1.0 + a * a / k) / k;
            u[i] = (T)(a / k);
            sq[i] = (T)sqrt(c);
        });
    }));
    // r = W (alpha / k) = L^-T (L^-1 u): two sweeps with the factor (its block operators where it has them), not a product with W
    GPX_TRY(trsv_lower(dtype, L, n, ldl, v.u, v.t, 0, st, nullptr, ops));
    GPX_TRY(trsv_lower(dtype, L, n, ldl, v.t, v.r, 1, st, nullptr, ops));
    GPX_TRY(dot(dtype, v.r, alpha, n, v.sums + 1, st));
    // Y = W diag(sqrt(c)) over X: X's rows have been read (k), nothing else needs L^-T
    // Y[r, c] = W[r, c] sq[c]; columns < n only
    return by_dtype(dtype, [&](auto t) {
        using T = decltype(t);
        const T *w = (const T *)W, *sq = (const T *)v.sq;
        T *Y = (T *)X;
        return map_rows(n, n, st, [=] __device__(int64_t r, int64_t c) { Y[r * ldl + c] = w[r * ldl + c] * sq[c]; });
    });
}

// Pm = Y Y^T, lower triangle, over W (dead: k and Y exist).  gemm_nt on its triangular route: the tiles above the diagonal
// are not computed; cleared first because the route for an n that is no multiple of the k-step accumulates into C.
int loo_weights_product(int dtype, int64_t n, int64_t ldl, const void *Y, void *Pm, int count, hipStream_t st)
{
    const int64_t sX = n * ldl;
    GPX_HIP(hipMemsetAsync(Pm, 0, (size_t)count * sX * esize(dtype), st));
    Batch bw; bw.count = count; bw.sA = bw.sB = bw.sC = sX;
    return gemm_nt(dtype, n, n, n, Y, ldl, Y, ldl, Pm, ldl, 1.0, GPX_LOWER, 0, 0, st, 0, 0, count > 1 ? &bw : nullptr);
}

int loo_weights_from_factor(int dtype, const void *L, int64_t n, int64_t ldl, const void *y, const void *alpha, void *X, void *W,
                            const LooVecs &v, const double *kii_have, TrsvOps *ops, hipStream_t st)
{
    GPX_TRY(inv_from_factor(dtype, L, n, ldl, X, W, GPX_FULL, st, ops));
    GPX_TRY(loo_weights_vectors(dtype, L, n, ldl, y, alpha, X, W, v, kii_have, ops, st));
    return loo_weights_product(dtype, n, ldl, X, W, 1, st);
}

// The reduction half, grad_reduce's counterpart: (alpha, r, Pm) are in HBM; one fused pass (tile_reduce with two vectors),
// then grad_from_sums turns the sums into (d/dh, d/dw ..., d/ds) -- factor 1, not 1/2: dL = sum dK_ab G_ab; noise:
// 2 s (r . alpha - tr Pm).  value (may be null): the criterion.  Synchronises g->st.
int loo_grad_reduce(gpx_gp *g, const void *pts, const void *alpha, const double *params, double s_noise, const LooVecs &v,
                    const void *Pm, int64_t ldp, double *part, double *value, double *out)
{
    const int64_t n = g->n;
    double S[GPX_ARD_MAX_D + 2], iso[2], sums[2] = {0.0, 0.0};
    GPX_TRY(tile_reduce(g->dtype, g->kernel, pts, n, g->d, reduce_params(g->kernel, g->d, params, iso), alpha, v.r, Pm, ldp, part, S, g->st));
    GPX_HIP(hipMemcpyAsync(sums, v.sums, sizeof(sums), hipMemcpyDeviceToHost, g->st));
    GPX_HIP(hipStreamSynchronize(g->st));
    grad_from_sums(g->kernel, g->d, params, S, sums[1], 2.0 * s_noise, 1.0, out);
    if (value) *value = sums[0];
    return GPX_OK;
}

// the handle's own factor: X, W, the vectors and the partial sums in one call's DevBufs; diag(K^-1) stays in the handle
struct LooWork { DevBuf X, W, vec, part; LooVecs v; };
static int loo_weights_of_handle(gpx_gp *g, LooWork *w)
{
    const size_t es = esize(g->dtype);
    const int64_t n = g->n, lda = g->lda;
    GPX_TRY(w->X.alloc((size_t)n * lda * es));
    GPX_TRY(w->W.alloc((size_t)n * lda * es));
    GPX_TRY(w->vec.alloc(loo_vec_bytes(g->dtype, n)));
    w->v = loo_vecs_at(w->vec.p, g->dtype, n);
    if (!g->kii) GPX_TRY(dev_alloc((void **)&g->kii, (size_t)n * sizeof(double), "hipMalloc kii"));
    if (!g->have_kii) w->v.kii = g->kii;                   // written here, as the first gpx_gp_loo would have
    GPX_TRY(loo_weights_from_factor(g->dtype, g->A, n, lda, g->y, g->alpha, w->X.p, w->W.p, w->v, g->have_kii ? g->kii : nullptr,
                                    &g->ops, g->st));
    g->have_kii = true;
    return GPX_OK;
}

}  // namespace gpx

using namespace gpx;

extern "C" {

int gpx_gp_loo_grad(gpx_gp_t *g, double *loo_log_lh, double *grad)
{
    GP_ENTER(g);
    GPX_ARG(g->fitted && loo_log_lh && grad, "bad arguments");
    GP_NEED_FINITE_Y(g);
    if (g->kernel == GPX_KERNEL_PERIODIC && g->d != 1) { set_error("periodic gradient needs d == 1"); return GPX_ERR_UNSUPPORTED; }
    GPX_ARG(g->have_data && g->have_params, "the handle was fitted from a matrix: no kernel to differentiate (gpx_gp_loo_grad_weights)");
    GpScal sc;
    GPX_TRY(gp_read_scal(g, &sc));
    if (sc.info != 0) {                                    // no factor: the criterion is -inf, its gradient NaN (as gpx_gp_dloglh_dtheta)
        *loo_log_lh = -INFINITY;
        for (int i = 0; i <= g->nparams; ++i) grad[i] = NAN;
        return GPX_OK;
    }
    LooWork w;
    GPX_TRY(w.part.alloc(dloglh_partial_doubles(g->kernel, g->d) * sizeof(double) + 64));
    GPX_TRY(loo_weights_of_handle(g, &w));
    return loo_grad_reduce(g, gp_view(g).x, g->alpha, g->params, g->s, w.v, w.W.p, g->lda, (double *)w.part.p, loo_log_lh, grad);
}

int gpx_gp_loo_grad_weights(gpx_gp_t *g, double *G, int64_t ld)
{
    GP_ENTER(g);
    GPX_ARG(g->fitted && G && ld >= g->n, "bad arguments");
    GP_NEED_FINITE_Y(g);
    GPX_TRY(gp_need_factor(g, "to take the leave-one-out weights from"));
    const int64_t n = g->n;
    LooWork w;
    DevBuf Gd;
    GPX_TRY(Gd.alloc((size_t)n * n * sizeof(double)));
    GPX_TRY(loo_weights_of_handle(g, &w));
    // G (n x n float64, dense) from alpha, r and the lower triangle of Pm: entry (a, b) and its mirror from the same
    // expression in the same order of operands, so G is symmetric bit for bit
    GPX_TRY(by_dtype(g->dtype, [&](auto t) {
        using T = decltype(t);
        const T *alpha = (const T *)g->alpha, *rv = (const T *)w.v.r, *Pm = (const T *)w.W.p;
        const int64_t ldp = g->lda;
        double *Gp = (double *)Gd.p;
        return map_rows(n, n, g->st, [=] __device__(int64_t r, int64_t c) {
            const double ac = (double)alpha[c], rc = (double)rv[c];
            const int64_t hi = r > c ? r : c, lo = r > c ? c : r;
            const double ah = r > c ? (double)alpha[r] : ac, rh = r > c ? (double)rv[r] : rc;
            const double al = r > c ? ac : (double)alpha[r], rl = r > c ? rc : (double)rv[r];
            Gp[r * n + c] = 0.5 * (rh * al + ah * rl) - (double)Pm[hi * ldp + lo];
        });
    }));
    return download_f64(GPX_F64, G, ld, Gd.p, n, n, n, 0, g->st);
}

}  // extern "C"
