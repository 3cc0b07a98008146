// gpx_cg.hip -- exact GP regression past the n x n factor: batched preconditioned conjugate gradients on (K + s^2 I) X^T = B^T
// with K never formed (Gardner et al. 2018; Wang et al. 2019).  gpx_cg_*.  Float64 only.
//
//   preconditioner  P = R^T R + s^2 I,  R (k x n) the pivoted partial Cholesky of K(x, x) (select_on_device, gpx_select.hip):
//       C = s^2 I + R R^T = Lc Lc^T (k x k),   P^-1 V = (V - (V R^T) C^-1 R) / s^2        (Woodbury; V holds vectors as ROWS)
//   one iteration of a group of S <= 32 columns (all state S x ldn, ldn = round_up(n, 128); scalars per column on the device):
//       q = s^2 p + K p            the map, then kmat_apply on row blocks of x (the fused route: K is never materialised)
//       delta = p.q   alpha = rho / delta   x += alpha p   r -= alpha q   rr = r.r
//       z = P^-1 r    rho' = r.z   beta = rho' / rho   p = z + beta p
//   A column is FROZEN -- its x, r, p no longer change, its alpha and beta are 0 -- once rr <= tol^2 bb (bb = b.b; the test
//   |r| <= tol |b| without the two roots), from the start when b = 0, and when delta <= 0 or is not finite (its iteration count is
//   then reported negative).  The host reads the group's status block once per iteration and stops when every column is frozen.
//
// Every sum is f64 in a fixed order: cg_dot_kernel / cg_update_kernel leave one partial per workgroup (block_sum_fixed), cg_fin_kernel
// adds them in ascending workgroup order and forms alpha, beta and the freezing flags on the device -- the host never computes
// a scalar of the recurrence.  No atomics: two solves of the same system give the same bits.
//
// Layout in HBM (doubles):
//   x (n, d)  [xs: the ARD family's scaled copy]  y (n)  alpha (n): the last solution for y
//   sel   (grow-only) the selection's block (sel_layout without x): R  rank x ldn | its residuals, partials and state
//   pre   (grow-only) cg_pre_layout:    C  k x ldk | Rt  n x ldk (R^T: the library's product is the NT form) | W  32 x ldk
//   state (grow-only) cg_state_layout:  the scalars | the partials  32 x nwg | B, X, Rv, Z, P, Q  S x ldn each
//   lh    (grow-only) cg_lh_layout, allocated by the first gpx_cg_lh:  the coefficient history  maxiter x 2 x 32 | rho0  32 |
//         Zt  32 x ldn, the first preconditioned residuals | the tile reduction's partials
// Nothing scales with n^2: n (d + 2 rank + 6 S + 2) doubles and small change (7 S with the estimate's block).
//
// The marginal likelihood (gpx_cg_lh): CG's alpha_j, beta_j ARE the Lanczos coefficients of P^-1/2 (K + s^2 I) P^-1/2 started
// at P^-1/2 z, so with probes z ~ N(0, P)  log det (K + s^2 I) = log det P + E[rho0 e1^T log(T) e1], rho0 = z . P^-1 z
// (stochastic Lanczos quadrature; the tridiagonal's eigenproblem is the host's).  cg_fin_kernel writes the coefficients of
// every iteration into the history block -- through a pointer that is null in every other solve -- and the group's history is
// downloaded once.  The gradient's trace term uses E[P^-1 z z^T] = I: tr(K^-1 dK) = E[(K^-1 z)^T dK (P^-1 z)], contracted
// against the kernel derivatives by lowrank_reduce (gpx_lrgrad.hip) with U = -W / T, V = Zt, and once more with U = V = alpha.
#include "gpx_small.h"
#include <algorithm>
#include <cmath>
#include <vector>

#include "gpx_gp_internal.h"
#include "gpx_kernels_dev.h"

constexpr int CG_GROUP = 32;                 // columns per group: GPX_KAPPLY_FUSED_MAX_F64, the fused product's range
static_assert(CG_GROUP == gpx::GPX_KAPPLY_FUSED_MAX_F64, "a group of columns is what the fused product takes at once");
constexpr int CG_ITEMS = 4, CG_WG = 256 * CG_ITEMS;      // elements per thread and per workgroup of the dot and update kernels
constexpr int64_t CG_LD_ALIGN = 128;         // the selection's pitch of R: one pitch for every n-wide array
constexpr int64_t CG_ROW_BLOCK = 65536;      // rows of x per kmat_apply call: bounds the fused kernel's S x rows partial sums

// what the host reads once per iteration
struct CgStatus {
    double rr[CG_GROUP];       // |r|^2 of the recurrence (a frozen column: at its crossing)
    double bb[CG_GROUP];       // |b|^2
    int frozen[CG_GROUP];
    int iters[CG_GROUP];       // the iteration at which the column froze; negative: delta <= 0 or not finite there
};
struct CgScal {
    double rho[CG_GROUP], delta[CG_GROUP], alpha[CG_GROUP], beta[CG_GROUP];
    double acc[CG_GROUP];      // a plain row dot (the variance's b.x)
    CgStatus stat;
};

// what a solve leaves behind for the likelihood estimate (null: nothing recorded)
struct CgRecord {
    double *hist;              // [it - 1][0: alpha, 1: beta][CG_GROUP], cleared by the caller; a frozen column's entries stay 0
    double *rho0;              // CG_GROUP: r0 . P^-1 r0
    double *Zt;                // S x ldn: P^-1 r0 (b.Z is overwritten at every iteration)
};

enum { CG_T_BUILD, CG_T_PRODUCT, CG_T_APPLY, CG_T_VECTOR, CG_T_TOTAL, CG_T_READ, CG_T_COUNT };

struct gpx_cg {
    int device, dtype, kernel, d, nparams;
    int64_t n, ldn;
    void *x, *xs, *y, *alpha;
    gpx::GrowBuf sel, pre, state, lh;
    void *R;                   // inside sel
    int64_t rank, k, ldk;      // rank asked for, rows of R in use, round_up(k, 16)
    hipStream_t st;
    gpx::PassTimeline tl;
    double params[1 + GPX_ARD_MAX_D], iso[2], s;
    double alpha_params[1 + GPX_ARD_MAX_D];
    bool have_x, have_y, have_precond, have_alpha;
    float ms[CG_T_COUNT];
    float acc_ms[CG_T_COUNT];  // of the pass that is running: folded at every status read (PassTimeline::fold)
};

namespace gpx {

// ---- the small kernels ---------------------------------------------------------------------------------------------------
// partial[s, wg] = sum over the workgroup's elements of a[s, i] b[s, i]; DIV: b[s, i] <- b[s, i] / div first (the Woodbury apply's
// last step, in the pass that needs z anyway).  a may be b (no __restrict__).
template <bool DIV>
__global__ __launch_bounds__(256) void cg_dot_kernel(const double *a, double *b, int64_t ld, int64_t n, double div, double *__restrict__ partial,
                                                     int64_t nwg)
{
    __shared__ double red[4][1];
    const int tid = threadIdx.x;
    const int64_t s = blockIdx.y;
    const double *ar = a + s * ld;
    double *br = b + s * ld;
    double acc[1] = {0.0};
#pragma unroll
    for (int e = 0; e < CG_ITEMS; ++e) {
        const int64_t i = (int64_t)blockIdx.x * CG_WG + e * 256 + tid;
        if (i < n) {
            double bv = br[i];
            if (DIV) { bv = bv / div; br[i] = bv; }
            acc[0] = fma(ar[i], bv, acc[0]);
        }
    }
    block_sum_fixed(acc, red, tid);
    __syncthreads();
    if (tid == 0) partial[s * nwg + blockIdx.x] = block_sum_final(red, 0);
}

// x += alpha p, r -= alpha q, partial[s, wg] = the workgroup's share of r.r; a frozen column is left alone
__global__ __launch_bounds__(256) void cg_update_kernel(double *__restrict__ x, double *__restrict__ r, const double *__restrict__ p,
                                                        const double *__restrict__ q, int64_t ld, int64_t n, const CgScal *__restrict__ sc,
                                                        double *__restrict__ partial, int64_t nwg)
{
    __shared__ double red[4][1];
    const int tid = threadIdx.x;
    const int64_t s = blockIdx.y;
    if (sc->stat.frozen[s]) return;                            // (the same for the whole workgroup)
    const double alpha = sc->alpha[s];
    double acc[1] = {0.0};
#pragma unroll
    for (int e = 0; e < CG_ITEMS; ++e) {
        const int64_t i = (int64_t)blockIdx.x * CG_WG + e * 256 + tid;
        if (i < n) {
            const int64_t at = s * ld + i;
            x[at] = fma(alpha, p[at], x[at]);
            const double rv = fma(-alpha, q[at], r[at]);
            r[at] = rv;
            acc[0] = fma(rv, rv, acc[0]);
        }
    }
    block_sum_fixed(acc, red, tid);
    __syncthreads();
    if (tid == 0) partial[s * nwg + blockIdx.x] = block_sum_final(red, 0);
}

// The second launch of every reduction: thread s adds column s's partials in ascending workgroup order and does what the sum is for.
enum { CG_FIN_BB, CG_FIN_RHO0, CG_FIN_DELTA, CG_FIN_RR, CG_FIN_RHO, CG_FIN_ACC };
__global__ __launch_bounds__(64) void cg_fin_kernel(int mode, const double *__restrict__ partial, int64_t nwg, int S, int it, double tol2,
                                                    int rho_is_rr, CgScal *sc, double *hist)
{
    const int s = threadIdx.x;
    if (s >= S) return;
    const bool frozen = mode != CG_FIN_BB && sc->stat.frozen[s] != 0;
    double sum = 0.0;
    if (rho_is_rr && (mode == CG_FIN_RHO0 || mode == CG_FIN_RHO)) sum = sc->stat.rr[s];      // P = I: z is r, and r.r is there already
    else if (!(frozen && mode == CG_FIN_RR))                   // (cg_update_kernel wrote no partials for a frozen column)
        for (int64_t w = 0; w < nwg; ++w) sum += partial[(int64_t)s * nwg + w];
    switch (mode) {
    case CG_FIN_BB:                                            // b.b; a zero right-hand side is frozen from the start
        sc->stat.bb[s] = sum; sc->stat.rr[s] = sum;
        sc->stat.frozen[s] = sum == 0.0 ? 1 : 0; sc->stat.iters[s] = 0;
        sc->alpha[s] = 0.0; sc->beta[s] = 0.0;
        break;
    case CG_FIN_RHO0: sc->rho[s] = sum; break;
    case CG_FIN_DELTA:
        sc->delta[s] = sum;
        if (frozen) sc->alpha[s] = 0.0;
        else if (!(sum > 0.0) || !isfinite(sum)) { sc->stat.frozen[s] = 1; sc->stat.iters[s] = -it; sc->alpha[s] = 0.0; }
        else sc->alpha[s] = sc->rho[s] / sum;
        if (hist) hist[(int64_t)(it - 1) * 2 * CG_GROUP + s] = sc->alpha[s];
        break;
    case CG_FIN_RR:
        if (!frozen) {
            sc->stat.rr[s] = sum;
            if (sum <= tol2 * sc->stat.bb[s]) { sc->stat.frozen[s] = 1; sc->stat.iters[s] = it; }
        }
        break;
    case CG_FIN_RHO:
        if (frozen) sc->beta[s] = 0.0;
        else {
            const double rho = sc->rho[s];
            sc->beta[s] = rho != 0.0 ? sum / rho : 0.0;
            sc->rho[s] = sum;
        }
        if (hist) hist[(int64_t)(it - 1) * 2 * CG_GROUP + CG_GROUP + s] = sc->beta[s];
        break;
    default: sc->acc[s] = sum; break;
    }
}

// ---- layouts -------------------------------------------------------------------------------------------------------------
struct CgPreLayout { size_t C, Rt, W, total; };
constexpr CgPreLayout cg_pre_layout(int64_t n, int64_t k, int64_t ldk)
{
    Carve c;
    const size_t C = c.take((size_t)k * ldk * 8), Rt = c.take((size_t)n * ldk * 8), W = c.take((size_t)CG_GROUP * ldk * 8);
    return {C, Rt, W, c.total()};
}
struct CgStateLayout { size_t B, X, Rv, Z, P, Q, part, scal, total; };
constexpr CgStateLayout cg_state_layout(int64_t ldn, int64_t nwg, int64_t S)
{
    // The scalars and the partials come FIRST and at their full size, so they lie at the same place for every S; behind them every
    // row of every vector array starts a multiple of ldn doubles from one base (ldn * 8 is a multiple of Carve's 128 bytes), for
    // every S: a layout for fewer columns puts rows on rows and pads on pads of the layout the block once grew for.
    Carve c;
    const size_t v = (size_t)S * ldn * 8;
    const size_t scal = c.take(sizeof(CgScal)), part = c.take((size_t)CG_GROUP * nwg * 8);
    const size_t B = c.take(v), X = c.take(v), Rv = c.take(v), Z = c.take(v), P = c.take(v), Q = c.take(v);
    return {B, X, Rv, Z, P, Q, part, scal, c.total()};
}
struct CgBufs {
    double *B = nullptr, *X = nullptr, *Rv = nullptr, *Z = nullptr, *P = nullptr, *Q = nullptr, *part = nullptr;
    CgScal *sc = nullptr;
    CgBufs() = default;
    CgBufs(char *p, const CgStateLayout &l)
        : B((double *)(p + l.B)), X((double *)(p + l.X)), Rv((double *)(p + l.Rv)), Z((double *)(p + l.Z)), P((double *)(p + l.P)),
          Q((double *)(p + l.Q)), part((double *)(p + l.part)), sc((CgScal *)(p + l.scal)) {}
};

struct CgLhLayout { size_t hist, rho0, Zt, part, total; };
static CgLhLayout cg_lh_layout(int64_t ldn, int64_t maxiter, size_t partial_doubles)
{
    Carve c;
    const size_t hist = c.take((size_t)std::max<int64_t>(maxiter, 1) * 2 * CG_GROUP * 8), rho0 = c.take(CG_GROUP * 8);
    const size_t Zt = c.take((size_t)CG_GROUP * ldn * 8), part = c.take(partial_doubles * 8);
    return {hist, rho0, Zt, part, c.total()};
}

static inline int64_t cg_nwg(int64_t n) { return cdiv(n, CG_WG); }

// the state block for groups of S columns; a block that grew is cleared (the columns [n, ldn) of every array stay zero from
// then on: nothing writes them, and the products read them)
static int cg_state(gpx_cg *g, int64_t S, CgBufs *out)
{
    const CgStateLayout lay = cg_state_layout(g->ldn, cg_nwg(g->n), S);
    bool grew = false;
    GPX_TRY(g->state.reserve(lay.total, g->st, &grew));
    if (grew) GPX_HIP(hipMemsetAsync(g->state.p, 0, g->state.bytes, g->st));
    *out = CgBufs((char *)g->state.p, lay);
    return GPX_OK;
}

struct CgView { int kernel; const void *x; const double *params; };
static inline CgView cg_view(const gpx_cg *g)
{
    if (g->kernel == GPX_KERNEL_GAUSSIAN_ARD) return {GPX_KERNEL_GAUSSIAN, g->xs, g->iso};
    return {g->kernel, g->x, g->params};
}

template <bool DIV>
static int cg_dot(const double *a, double *b, int64_t S, const gpx_cg *g, double div, double *partial)
{
    hipLaunchKernelGGL((cg_dot_kernel<DIV>), dim3((unsigned)cg_nwg(g->n), (unsigned)S), dim3(256), 0, g->st, a, b, g->ldn, g->n, div, partial,
                       cg_nwg(g->n));
    GPX_LAUNCH_CHECK();
    return GPX_OK;
}
static int cg_fin(int mode, int64_t S, int it, double tol2, const gpx_cg *g, const CgBufs &b, double *hist = nullptr)
{
    hipLaunchKernelGGL(cg_fin_kernel, dim3(1), dim3(64), 0, g->st, mode, b.part, cg_nwg(g->n), (int)S, it, tol2, g->k > 0 ? 0 : 1, b.sc, hist);
    GPX_LAUNCH_CHECK();
    return GPX_OK;
}

// out = s^2 P^-1 V for S <= 32 rows (S x ldn each, out != V): everything of the Woodbury apply but the division by s^2, which
// the caller fuses into its next pass over out.  k == 0 (P = I): out = V.
static int cg_woodbury(gpx_cg *g, const double *V, int64_t S, double *out)
{
    const int64_t n = g->n, ldn = g->ldn, k = g->k, ldk = g->ldk;
    hipStream_t st = g->st;
    GPX_HIP(hipMemcpyAsync(out, V, (size_t)S * ldn * 8, hipMemcpyDeviceToDevice, st));
    if (k == 0) return GPX_OK;
    const CgPreLayout lay = cg_pre_layout(n, k, ldk);
    char *base = (char *)g->pre.p;
    void *C = base + lay.C, *Rt = base + lay.Rt, *W = base + lay.W;
    GPX_HIP(hipMemsetAsync(W, 0, (size_t)S * ldk * 8, st));
    // W = V R^T over the padded depth ldn (both operands are zero there): the aligned product kernel
    GPX_TRY(gemm_nt(GPX_F64, S, k, ldn, V, ldn, g->R, ldn, W, ldk, 1.0, GPX_FULL, 0, 0, st));
    GPX_TRY(trsm_right_lt(GPX_F64, C, k, ldk, W, S, ldk, st));            // W Lc^-T
    GPX_TRY(trsm_right_l(GPX_F64, C, k, ldk, W, S, ldk, st));             // W Lc^-T Lc^-1 = V R^T C^-1
    // out -= W R, as W Rt^T over the padded depth ldk (W's and Rt's columns [k, ldk) are zero)
    GPX_TRY(gemm_nt(GPX_F64, S, n, ldk, W, ldk, Rt, ldk, out, ldn, -1.0, GPX_FULL, 0, 0, st));
    return GPX_OK;
}

static int cg_read_status(gpx_cg *g, const CgBufs &b, CgStatus *host)
{
    GPX_HIP(hipMemcpyAsync(host, &b.sc->stat, sizeof(CgStatus), hipMemcpyDeviceToHost, g->st));
    GPX_HIP(hipStreamSynchronize(g->st));
    return g->tl.fold(g->acc_ms, CG_T_TOTAL);                   // (every mark so far has passed: the pass keeps a handful of events)
}

static bool cg_all_frozen(const CgStatus &h, int64_t S)
{
    for (int64_t s = 0; s < S; ++s) if (!h.frozen[s]) return false;
    return true;
}

// One group: the right-hand sides are in b.B (S x ldn); the solution is left in b.X.  iters, relres: S entries (host).
// rec (may be null): the coefficient history, rho0 and the first preconditioned residual are kept for gpx_cg_lh.
static int cg_solve_group(gpx_cg *g, const CgBufs &b, int64_t S, double tol, int64_t maxiter, int *iters, double *relres, int64_t *its_done,
                          const CgRecord *rec = nullptr)
{
    const int64_t n = g->n, ldn = g->ldn;
    const size_t vb = (size_t)S * ldn * 8;
    const double s2 = g->s * g->s, tol2 = tol * tol;
    const CgView v = cg_view(g);
    hipStream_t st = g->st;
    PassTimeline &tl = g->tl;
    const bool pre = g->k > 0;
    double *Z = pre ? b.Z : b.Rv;                               // P = I: z IS r
    GPX_HIP(hipMemsetAsync(b.sc, 0, sizeof(CgScal), st));
    GPX_HIP(hipMemsetAsync(b.X, 0, vb, st));
    GPX_HIP(hipMemcpyAsync(b.Rv, b.B, vb, hipMemcpyDeviceToDevice, st));
    GPX_TRY(cg_dot<false>(b.Rv, b.Rv, S, g, 1.0, b.part));
    GPX_TRY(cg_fin(CG_FIN_BB, S, 0, tol2, g, b));
    GPX_TRY(tl.mark(st, CG_T_VECTOR));
    if (pre) {
        GPX_TRY(cg_woodbury(g, b.Rv, S, b.Z));
        GPX_TRY(cg_dot<true>(b.Rv, b.Z, S, g, s2, b.part));
        GPX_TRY(tl.mark(st, CG_T_APPLY));
    }
    GPX_TRY(cg_fin(CG_FIN_RHO0, S, 0, tol2, g, b));
    GPX_HIP(hipMemcpyAsync(b.P, Z, vb, hipMemcpyDeviceToDevice, st));
    double *hist = nullptr;
    if (rec) {
        hist = rec->hist;
        GPX_HIP(hipMemcpyAsync(rec->Zt, Z, vb, hipMemcpyDeviceToDevice, st));
        GPX_HIP(hipMemcpyAsync(rec->rho0, b.sc->rho, sizeof(double) * CG_GROUP, hipMemcpyDeviceToDevice, st));
    }
    GPX_TRY(tl.mark(st, CG_T_VECTOR));
    CgStatus host;
    GPX_TRY(cg_read_status(g, b, &host));
    GPX_TRY(tl.mark(st, CG_T_READ));
    int64_t it = 0;
    while (it < maxiter && !cg_all_frozen(host, S)) {
        ++it;
        route_hit(RT_CG_ITER);
        {
            double *P = b.P, *Q = b.Q;
            GPX_TRY(map_rows(S, n, st, [=] __device__(int64_t r, int64_t c) { Q[r * ldn + c] = s2 * P[r * ldn + c]; }));
        }
        GPX_TRY(tl.mark(st, CG_T_VECTOR));
        for (int64_t r0 = 0; r0 < n; r0 += CG_ROW_BLOCK) {
            const int64_t rc = std::min(CG_ROW_BLOCK, n - r0);
            GPX_TRY(kmat_apply(GPX_F64, v.kernel, (const char *)v.x + (size_t)r0 * g->d * 8, rc, v.x, n, g->d, v.params, b.P, ldn, S, b.Q + r0,
                               ldn, st));
        }
        GPX_TRY(tl.mark(st, CG_T_PRODUCT));
        GPX_TRY(cg_dot<false>(b.P, b.Q, S, g, 1.0, b.part));
        GPX_TRY(cg_fin(CG_FIN_DELTA, S, (int)it, tol2, g, b, hist));
        hipLaunchKernelGGL(cg_update_kernel, dim3((unsigned)cg_nwg(n), (unsigned)S), dim3(256), 0, st, b.X, b.Rv, b.P, b.Q, ldn, n, b.sc, b.part,
                           cg_nwg(n));
        GPX_LAUNCH_CHECK();
        GPX_TRY(cg_fin(CG_FIN_RR, S, (int)it, tol2, g, b));
        GPX_TRY(tl.mark(st, CG_T_VECTOR));
        GPX_TRY(cg_read_status(g, b, &host));
        GPX_TRY(tl.mark(st, CG_T_READ));
        if (it == maxiter || cg_all_frozen(host, S)) break;
        if (pre) {
            GPX_TRY(cg_woodbury(g, b.Rv, S, b.Z));
            GPX_TRY(cg_dot<true>(b.Rv, b.Z, S, g, s2, b.part));
            GPX_TRY(tl.mark(st, CG_T_APPLY));
        }
        GPX_TRY(cg_fin(CG_FIN_RHO, S, (int)it, tol2, g, b, hist));
        {
            double *P = b.P;
            const double *Zc = Z;
            const CgScal *sc = b.sc;
            GPX_TRY(map_rows(S, n, st, [=] __device__(int64_t r, int64_t c) {
                if (sc->stat.frozen[r]) return;
                P[r * ldn + c] = fma(sc->beta[r], P[r * ldn + c], Zc[r * ldn + c]);
            }));
        }
        GPX_TRY(tl.mark(st, CG_T_VECTOR));
    }
    for (int64_t s = 0; s < S; ++s) {
        iters[s] = host.frozen[s] ? host.iters[s] : (int)it;
        relres[s] = host.bb[s] > 0.0 ? sqrt(host.rr[s] / host.bb[s]) : (host.bb[s] == 0.0 ? 0.0 : NAN);
    }
    *its_done = it;
    return GPX_OK;
}

// a pass's profile record (GPX_PROF_CG) and timeline, around every group of one API call
struct CgPass {
    gpx_cg *g; int rec; RoctxRange range; double work = 0.0;
    explicit CgPass(gpx_cg *h) : g(h), rec(-1), range(prof_class_name(PC_CG))
    {
        if (g_prof_on && g_prof_mute == 0) rec = prof_begin(PC_CG, 0.0, g->st);
    }
    int begin()
    {
        for (float &v : g->acc_ms) v = 0.0f;
        g->tl.begin();
        return g->tl.mark(g->st, TL_NOBODY);
    }
    void group(int64_t its) { work += (double)g->n * (double)g->n * (double)its; }
    int end()
    {
        if (rec >= 0) { prof_end(rec, g->st); prof_set_work(rec, work); rec = -1; }
        GPX_HIP(hipStreamSynchronize(g->st));
        GPX_TRY(g->tl.fold(g->acc_ms, CG_T_TOTAL));
        for (int i : {CG_T_PRODUCT, CG_T_APPLY, CG_T_VECTOR, CG_T_TOTAL, CG_T_READ}) g->ms[i] = g->acc_ms[i];
        return GPX_OK;
    }
    ~CgPass() { if (rec >= 0) prof_end(rec, g->st); }
};

// columns per group: what the fused route of kmat_apply takes now (gpx_debug_kapply_fused_max can lower it; the product route
// would materialise an n-wide chunk of K per group, which this solver never does)
static int cg_group_now(int64_t *group)
{
    const int64_t fused = tune().kapply_fused_max[GPX_F64];
    if (fused < 1) { set_error("the fused route of gpx_d_kmat_apply is switched off (gpx_debug_kapply_fused_max): the iterative solver has no other product"); return GPX_ERR_UNSUPPORTED; }
    *group = std::min<int64_t>(CG_GROUP, fused);
    return GPX_OK;
}

static bool cg_same_params(const gpx_cg *g, const double *params, double s)
{
    for (int i = 0; i < g->nparams; ++i) if (params[i] != g->params[i]) return false;
    return s == g->s;
}

// y's and alpha's columns [n, ldn) are read as zeros by the products
static int cg_clear_vectors(gpx_cg *g)
{
    GPX_HIP(hipMemsetAsync(g->y, 0, (size_t)g->ldn * 8, g->st));
    GPX_HIP(hipMemsetAsync(g->alpha, 0, (size_t)g->ldn * 8, g->st));
    return GPX_OK;
}

// Z[r, c] /= div over S x n
static int cg_div_rows(double *Z, int64_t S, int64_t n, int64_t ldn, double div, hipStream_t st)
{
    return map_rows(S, n, st, [=] __device__(int64_t r, int64_t c) { Z[r * ldn + c] = Z[r * ldn + c] / div; });
}

// the preconditioner of (params, s) already in the handle: the selection on the resident points, C and its factor, R^T
static int cg_precond(gpx_cg *g, const double *params, double s, int64_t rank, double tol, int64_t *count)
{
    const int64_t n = g->n, ldn = g->ldn;
    hipStream_t st = g->st;
    g->have_precond = g->have_alpha = false;
    for (int i = 0; i < g->nparams; ++i) g->params[i] = params[i];
    g->s = s; g->rank = rank; g->k = 0; g->ldk = 0; g->R = nullptr;
    PassTimeline &tl = g->tl.begin();
    GPX_TRY(tl.mark(st, TL_NOBODY));
    if (g->kernel == GPX_KERNEL_GAUSSIAN_ARD) {
        ard_iso(g->params, g->d, g->iso);
        GPX_TRY(scale_points(g->dtype, g->x, n, g->d, g->params + 1, g->xs, st));
    }
    const CgView v = cg_view(g);
    {   // the kernel constants are checked before anything is launched with them
        KParams kp;
        GPX_TRY(make_kparams(v.kernel, GPX_K, v.params, 0.0, &kp));
    }
    int64_t k = 0;
    if (rank > 0) {
        // R's block: cleared, so the columns [n, ldn) of R, which the selection never writes, are the zeros the products read
        GPX_TRY(g->sel.reserve(select_block_bytes(g->dtype, n, rank), st));
        GPX_HIP(hipMemsetAsync(g->sel.p, 0, g->sel.bytes, st));
        int64_t ldr = 0;
        GPX_TRY(select_on_device(g->dtype, v.kernel, v.x, n, g->d, v.params, rank, tol, g->sel.p, st, &k, &g->R, &ldr));
        if (ldr != ldn) { set_error("gpx_cg_precond: the selection's pitch %lld is not the handle's %lld", (long long)ldr, (long long)ldn); return GPX_ERR_INTERNAL; }
    }
    if (k > 0) {
        const int64_t ldk = round_up(k, 16);
        const CgPreLayout lay = cg_pre_layout(n, k, ldk);
        GPX_TRY(g->pre.reserve(lay.total, st));
        GPX_HIP(hipMemsetAsync(g->pre.p, 0, lay.total, st));
        char *base = (char *)g->pre.p;
        double *C = (double *)(base + lay.C);
        void *Rt = base + lay.Rt;
        DevBuf info;
        GPX_TRY(info.alloc(sizeof(int)));
        GPX_HIP(hipMemsetAsync(info.p, 0, sizeof(int), st));
        // C = s^2 I + R R^T on the lower triangle (the depth padded to ldn: zeros), its factor, and R^T
        const double s2 = s * s;
        GPX_TRY(map_vec(k, st, [=] __device__(int64_t i) { C[i * ldk + i] = s2; }));
        GPX_TRY(gemm_nt(GPX_F64, k, k, ldn, g->R, ldn, g->R, ldn, C, ldk, 1.0, GPX_LOWER, 0, 0, st));
        GPX_TRY(potrf(GPX_F64, C, k, ldk, (int *)info.p, st));
        GPX_TRY(tril(GPX_F64, C, k, ldk, st));
        GPX_TRY(transpose(GPX_F64, g->R, ldn, k, n, Rt, ldk, 0, st));
        int hinfo = 0;
        GPX_HIP(hipMemcpyAsync(&hinfo, info.p, sizeof(int), hipMemcpyDeviceToHost, st));
        GPX_HIP(hipStreamSynchronize(st));
        GPX_TRY(check_internal_info(hinfo));
        if (hinfo != 0) {
            set_error("gpx_cg_precond: s^2 I + R R^T is not positive definite (pivot %d of %lld)", hinfo, (long long)k);
            return GPX_ERR_ARG;
        }
        g->k = k; g->ldk = ldk;
    }
    GPX_TRY(tl.mark(st, CG_T_BUILD));
    GPX_HIP(hipStreamSynchronize(st));
    float ms[CG_T_COUNT];
    GPX_TRY(tl.resolve(ms, CG_T_COUNT, CG_T_TOTAL));
    g->ms[CG_T_BUILD] = ms[CG_T_BUILD];
    g->have_precond = true;
    *count = k;
    return GPX_OK;
}

// The handle's solution for y: one group of one column; it stays on the device for gpx_cg_mean and gpx_cg_lh.
static int cg_solve_y(gpx_cg *g, const CgBufs &b, double tol, int64_t maxiter, int *iters, double *relres, int64_t *its)
{
    const int64_t ldn = g->ldn;
    GPX_HIP(hipMemcpyAsync(b.B, g->y, (size_t)ldn * 8, hipMemcpyDeviceToDevice, g->st));
    GPX_TRY(g->tl.mark(g->st, TL_NOBODY));
    GPX_TRY(cg_solve_group(g, b, 1, tol, maxiter, iters, relres, its));
    GPX_HIP(hipMemcpyAsync(g->alpha, b.X, (size_t)ldn * 8, hipMemcpyDeviceToDevice, g->st));
    for (int i = 0; i < g->nparams; ++i) g->alpha_params[i] = g->params[i];
    g->have_alpha = true;
    return GPX_OK;
}

// Rows [t0, t0 + S) of the probes z ~ N(0, P) into dst (S x ldn, its pads zero): z = g1 R + s g2 with g2 = randn(T x n; seed,
// stream 4) and g1 = randn(T x k; seed, stream 5); rank 0 (P = I): z = g2.  Row t depends on (seed, t) alone: fewer probes are a
// prefix of more, and a group is generated where it is solved.
static int cg_make_probes(gpx_cg *g, int64_t t0, int64_t S, uint64_t seed, double *dst)
{
    const int64_t n = g->n, ldn = g->ldn, k = g->k, ldk = g->ldk;
    hipStream_t st = g->st;
    GPX_TRY(randn(GPX_F64, dst, S, n, ldn, seed, 4, (uint64_t)t0 * (uint64_t)n, st));
    if (k == 0) return GPX_OK;
    const double sd = g->s;
    GPX_TRY(map_rows(S, n, st, [=] __device__(int64_t r, int64_t c) { dst[r * ldn + c] = sd * dst[r * ldn + c]; }));
    const CgPreLayout lay = cg_pre_layout(n, k, ldk);
    char *base = (char *)g->pre.p;
    void *Rt = base + lay.Rt, *W = base + lay.W;
    GPX_HIP(hipMemsetAsync(W, 0, (size_t)S * ldk * 8, st));
    GPX_TRY(randn(GPX_F64, W, S, k, ldk, seed, 5, (uint64_t)t0 * (uint64_t)k, st));
    // dst += g1 R, as W Rt^T over the padded depth ldk (W's and Rt's columns [k, ldk) are zero)
    return gemm_nt(GPX_F64, S, n, ldk, W, ldk, Rt, ldk, dst, ldn, 1.0, GPX_FULL, 0, 0, st);
}

// log det P = 2 sum log diag(Lc) + (n - k) log s^2; 0 without a preconditioner (P = I).  Synchronises the stream.
static int cg_logdet_precond(gpx_cg *g, double *out)
{
    *out = 0.0;
    const int64_t k = g->k, ldk = g->ldk;
    if (k == 0) return GPX_OK;
    const CgPreLayout lay = cg_pre_layout(g->n, k, ldk);
    const double *C = (const double *)((char *)g->pre.p + lay.C);
    double *W = (double *)((char *)g->pre.p + lay.W);
    GPX_TRY(map_vec(k, g->st, [=] __device__(int64_t i) { W[i] = C[i * ldk + i]; }));
    std::vector<double> diag((size_t)k);
    GPX_HIP(hipMemcpyAsync(diag.data(), W, (size_t)k * 8, hipMemcpyDeviceToHost, g->st));
    GPX_HIP(hipStreamSynchronize(g->st));
    GPX_HIP(hipMemsetAsync(W, 0, (size_t)k * 8, g->st));         // (W's columns [k, ldk) of every row stay zero for the products)
    double sum = 0.0;
    for (int64_t i = 0; i < k; ++i) sum += log(diag[i]);
    *out = 2.0 * sum + (double)(g->n - k) * log(g->s * g->s);
    return GPX_OK;
}

}  // namespace gpx

using namespace gpx;

#define CG_ENTER(g)                                                          \
    GPX_ARG((g) != nullptr, "handle is NULL");                               \
    gpx::tune_refresh();                                                     \
    gpx::DeviceGuard guard__((g)->device);                                   \
    if (guard__.rc != GPX_OK) return guard__.rc;                             \
    gpx::StreamTurn turn__((g)->st);                                         \
    gpx::RoctxRange api_range__(__func__)

// a solve needs data and the preconditioner of exactly its parameters (rank 0 included: gpx_cg_precond is what takes them in)
#define CG_NEED_PRECOND(g, params, s)                                                                                            \
    do {                                                                                                                         \
        GPX_ARG((params) != nullptr, "NULL argument");                                                                           \
        GPX_ARG((g)->have_x && (g)->have_y, "no data in the handle (gpx_cg_set_data)");                                          \
        GPX_ARG((g)->have_precond && gpx::cg_same_params((g), (params), (s)),                                                    \
                "there is no preconditioner for these parameters (gpx_cg_precond first; rank 0 for none)");                      \
    } while (0)

extern "C" {

int gpx_cg_create(gpx_cg_t **out, int dtype, int kernel, int64_t n, int d)
{
    GPX_TRY(ensure_device());
    GPX_ARG(out, "handle is NULL");
    *out = nullptr;
    GPX_ARG(dtype == GPX_F64 || dtype == GPX_F32, "dtype must be GPX_F64 or GPX_F32");
    if (dtype != GPX_F64) {
        set_error("gpx_cg_create: float64 only (an fp32-product, fp64-recurrence solver is not implemented)");
        return GPX_ERR_UNSUPPORTED;
    }
    GPX_ARG(kernel == GPX_KERNEL_GAUSSIAN || kernel == GPX_KERNEL_PERIODIC || kernel == GPX_KERNEL_GAUSSIAN_ARD, "unknown kernel family");
    GPX_ARG(n >= 1 && d >= 1, "need n >= 1 and d >= 1");
    GPX_ARG(kernel != GPX_KERNEL_GAUSSIAN_ARD || d <= GPX_ARD_MAX_D, "the ARD family needs d <= GPX_ARD_MAX_D");
    if (!kapply_fused_fits(dtype, d, CG_GROUP)) {
        set_error("gpx_cg_create: d = %d is beyond the fused route of gpx_d_kmat_apply (and gpx_d_mean), the only product the solver uses", d);
        return GPX_ERR_UNSUPPORTED;
    }
    GPX_ARG(n <= INT64_MAX / (8 * (int64_t)std::max(d, 8 * CG_GROUP)), "n * d overflows");
    gpx_cg *g = new gpx_cg();
    g->dtype = dtype; g->kernel = kernel; g->n = n; g->d = d;
    if (hipGetDevice(&g->device) != hipSuccess) { (void)hipGetLastError(); g->device = 0; }
    g->nparams = nparams_of(kernel, d);
    g->ldn = round_up(n, CG_LD_ALIGN);
    int rc = GPX_OK;
#define CG_ALLOC(field, bytes) if (rc == GPX_OK) rc = dev_alloc((void **)&g->field, (bytes), "hipMalloc " #field)
    CG_ALLOC(x, (size_t)n * d * 8);
    if (kernel == GPX_KERNEL_GAUSSIAN_ARD) CG_ALLOC(xs, (size_t)n * d * 8);
    CG_ALLOC(y, (size_t)g->ldn * 8);
    CG_ALLOC(alpha, (size_t)g->ldn * 8);
#undef CG_ALLOC
    if (rc == GPX_OK) {
        const hipError_t e = hipStreamCreateWithFlags(&g->st, hipStreamNonBlocking);
        if (e != hipSuccess) rc = hip_fail(e, "hipStreamCreate", __FILE__, __LINE__);
    }
    if (rc == GPX_OK) rc = cg_clear_vectors(g);
    if (rc != GPX_OK) { gpx_cg_destroy(g); return rc; }
    *out = g;
    return GPX_OK;
}

int gpx_cg_destroy(gpx_cg_t *g)
{
    if (!g) return GPX_OK;
    gpx::DeviceGuard guard__(g->device);
    if (g->st) (void)hipStreamSynchronize(g->st);
    stream_epoch_bump();                                       // (StreamTurn: a later stream at this one's address is a different stream)
    for (void *b : {g->x, g->xs, g->y, g->alpha}) dev_free(b);
    g->sel.release(); g->pre.release(); g->state.release(); g->lh.release();
    for (hipEvent_t e : g->tl.pool) (void)hipEventDestroy(e);
    if (g->st) (void)hipStreamDestroy(g->st);
    delete g;
    return GPX_OK;
}

int gpx_cg_set_data(gpx_cg_t *g, const double *x, const double *y)
{
    CG_ENTER(g);
    g->have_alpha = false;
    if (x) {
        g->have_precond = false;                                // (R is a function of x; y alone leaves it)
        GPX_TRY(upload_f64(g->dtype, g->x, g->n * g->d, x, g->n * g->d, 1, g->n * g->d, g->st));
        g->have_x = true;
    }
    if (y) { GPX_TRY(upload_f64(g->dtype, g->y, g->n, y, g->n, 1, g->n, g->st)); g->have_y = true; }
    return GPX_OK;
}

int gpx_cg_precond(gpx_cg_t *g, const double *params, double s, int64_t rank, double tol, int64_t *count)
{
    CG_ENTER(g);
    GPX_ARG(params && count, "NULL argument");
    GPX_ARG(g->have_x, "no data in the handle (gpx_cg_set_data)");
    GPX_ARG(s > 0.0 && s <= 1.79769313486231570e308, "s must be positive and finite (the preconditioner divides by s^2)");
    GPX_ARG(rank >= 0 && rank <= g->n, "rank must lie in 0 .. n");
    GPX_ARG(tol >= 0.0 && tol <= 1.79769313486231570e308, "tol must be >= 0 and finite");
    for (int i = 0; i < g->nparams; ++i) GPX_ARG(std::isfinite(params[i]), "array must not contain infs or NaNs (kernel parameters)");
    return cg_precond(g, params, s, rank, tol, count);
}

int gpx_cg_precond_apply(gpx_cg_t *g, const double *V, int64_t Sn, double *out)
{
    CG_ENTER(g);
    GPX_ARG(g->have_precond, "there is no preconditioner (gpx_cg_precond)");
    GPX_ARG(Sn >= 0 && (Sn == 0 || (V && out)), "bad arguments");
    const int64_t n = g->n, ldn = g->ldn;
    const double s2 = g->s * g->s;
    for (int64_t s0 = 0; s0 < Sn; s0 += CG_GROUP) {
        const int64_t S = std::min<int64_t>(CG_GROUP, Sn - s0);
        CgBufs b;
        GPX_TRY(cg_state(g, std::min<int64_t>(CG_GROUP, Sn), &b));
        GPX_TRY(upload_f64(g->dtype, b.B, ldn, V + s0 * n, n, S, n, g->st));
        GPX_TRY(cg_woodbury(g, b.B, S, b.Z));
        if (g->k > 0) GPX_TRY(cg_div_rows(b.Z, S, n, ldn, s2, g->st));
        GPX_TRY(download_f64(g->dtype, out + s0 * n, n, b.Z, ldn, S, n, 0, g->st));
    }
    return GPX_OK;
}

int gpx_cg_solve(gpx_cg_t *g, const double *params, double s, const double *B, int64_t Sn, double tol, int64_t maxiter, double *X,
                 int *iters, double *relres)
{
    CG_ENTER(g);
    CG_NEED_PRECOND(g, params, s);
    GPX_ARG(Sn >= 0 && (B || Sn == 1), "B == NULL (the handle's y) goes with S == 1");
    GPX_ARG(tol >= 0.0 && tol <= 1.79769313486231570e308, "tol must be >= 0 and finite");
    GPX_ARG(maxiter >= 0 && maxiter <= 0x7fffffff, "maxiter must lie in 0 .. 2^31 - 1");
    GPX_ARG(Sn == 0 || (iters && relres && (X || !B)), "NULL argument");
    if (Sn == 0) return GPX_OK;
    const int64_t n = g->n, ldn = g->ldn;
    int64_t G = 0;
    GPX_TRY(cg_group_now(&G));
    CgPass pass(g);
    GPX_TRY(pass.begin());
    for (int64_t s0 = 0; s0 < Sn; s0 += G) {
        const int64_t S = std::min<int64_t>(G, Sn - s0);
        CgBufs b;
        GPX_TRY(cg_state(g, std::min<int64_t>(G, Sn), &b));
        int64_t its = 0;
        if (B) {
            GPX_TRY(upload_f64(g->dtype, b.B, ldn, B + s0 * n, n, S, n, g->st));
            GPX_TRY(g->tl.mark(g->st, TL_NOBODY));
            GPX_TRY(cg_solve_group(g, b, S, tol, maxiter, iters + s0, relres + s0, &its));
        } else GPX_TRY(cg_solve_y(g, b, tol, maxiter, iters, relres, &its));     // the solution for y stays, for gpx_cg_mean
        pass.group(its);
        GPX_TRY(g->tl.mark(g->st, CG_T_VECTOR));
        if (X) GPX_TRY(download_f64(g->dtype, X + s0 * n, n, b.X, ldn, S, n, 0, g->st));
        GPX_TRY(g->tl.mark(g->st, TL_NOBODY));
    }
    GPX_TRY(pass.end());
    return GPX_OK;
}

int gpx_cg_mean(gpx_cg_t *g, const double *params, const double *xo, int64_t m, double *out)
{
    CG_ENTER(g);
    GPX_ARG(params != nullptr, "NULL argument");
    GPX_ARG(g->have_alpha, "there is no solution for y (gpx_cg_solve with B == NULL first)");
    for (int i = 0; i < g->nparams; ++i) GPX_ARG(params[i] == g->alpha_params[i], "the solution for y belongs to other parameters");
    GPX_ARG(m >= 0 && (m == 0 || (xo && out)), "bad arguments");
    if (m == 0) return GPX_OK;
    GPX_ARG(m <= INT64_MAX / (8 * (int64_t)g->d), "m * d overflows");
    DevBuf dxo, dout;
    GPX_TRY(dxo.alloc((size_t)m * g->d * 8));
    GPX_TRY(dout.alloc((size_t)m * 8));
    GPX_TRY(upload_f64(g->dtype, dxo.p, m * g->d, xo, m * g->d, 1, m * g->d, g->st));
    if (g->kernel == GPX_KERNEL_GAUSSIAN_ARD) GPX_TRY(scale_points(g->dtype, dxo.p, m, g->d, g->params + 1, dxo.p, g->st));
    const CgView v = cg_view(g);
    GPX_TRY(gpx_d_mean(g->dtype, v.kernel, dxo.p, m, v.x, g->n, g->d, v.params, g->alpha, dout.p, (void *)g->st));
    return download_f64(g->dtype, out, m, dout.p, m, 1, m, 0, g->st);
}

int gpx_cg_var(gpx_cg_t *g, const double *params, double s, const double *xo, int64_t m, double tol, int64_t maxiter, double *out,
               double *worst_relres)
{
    CG_ENTER(g);
    CG_NEED_PRECOND(g, params, s);
    GPX_ARG(tol >= 0.0 && tol <= 1.79769313486231570e308, "tol must be >= 0 and finite");
    GPX_ARG(maxiter >= 0 && maxiter <= 0x7fffffff, "maxiter must lie in 0 .. 2^31 - 1");
    GPX_ARG(m >= 0 && (m == 0 || (xo && out)), "bad arguments");
    if (worst_relres) *worst_relres = 0.0;
    if (m == 0) return GPX_OK;
    GPX_ARG(m <= INT64_MAX / (8 * (int64_t)g->d), "m * d overflows");
    const int64_t n = g->n, ldn = g->ldn;
    const CgView v = cg_view(g);
    DevBuf dxo, dvar;
    GPX_TRY(dxo.alloc((size_t)m * g->d * 8));
    GPX_TRY(dvar.alloc((size_t)m * 8));
    GPX_TRY(upload_f64(g->dtype, dxo.p, m * g->d, xo, m * g->d, 1, m * g->d, g->st));
    if (g->kernel == GPX_KERNEL_GAUSSIAN_ARD) GPX_TRY(scale_points(g->dtype, dxo.p, m, g->d, g->params + 1, dxo.p, g->st));
    int64_t G = 0;
    GPX_TRY(cg_group_now(&G));
    CgPass pass(g);
    GPX_TRY(pass.begin());
    double worst = 0.0;
    for (int64_t r0 = 0; r0 < m; r0 += G) {
        const int64_t S = std::min<int64_t>(G, m - r0);
        CgBufs b;
        GPX_TRY(cg_state(g, std::min<int64_t>(G, m), &b));
        const char *xo_c = (const char *)dxo.p + (size_t)r0 * g->d * 8;
        GPX_TRY(kmat(g->dtype, v.kernel, GPX_K, xo_c, S, v.x, n, g->d, v.params, 0.0, GPX_FULL, b.B, ldn, g->st));
        GPX_TRY(g->tl.mark(g->st, TL_NOBODY));
        int iters[CG_GROUP];
        double relres[CG_GROUP];
        int64_t its = 0;
        GPX_TRY(cg_solve_group(g, b, S, tol, maxiter, iters, relres, &its));
        pass.group(its);
        for (int64_t i = 0; i < S; ++i) if (!(relres[i] <= worst)) worst = relres[i];        // (a NaN is the worst)
        // var_i = k(xo_i, xo_i) - b_i . x_i
        GPX_TRY(cg_dot<false>(b.B, b.X, S, g, 1.0, b.part));
        GPX_TRY(cg_fin(CG_FIN_ACC, S, 0, 0.0, g, b));
        GPX_TRY(var_finish(g->dtype, v.kernel, xo_c, g->d, v.params, b.sc->acc, S, (double *)dvar.p + r0, g->st));
        GPX_TRY(g->tl.mark(g->st, CG_T_VECTOR));
    }
    GPX_TRY(pass.end());
    GPX_TRY(download_f64(g->dtype, out, m, dvar.p, m, 1, m, 0, g->st));
    if (worst_relres) *worst_relres = worst;
    return GPX_OK;
}

int gpx_cg_probes(gpx_cg_t *g, int64_t T, uint64_t seed, double *out)
{
    CG_ENTER(g);
    GPX_ARG(g->have_precond, "there is no preconditioner (gpx_cg_precond)");
    GPX_ARG(T >= 1, "need T >= 1");
    GPX_ARG(T <= INT64_MAX / g->n, "T * n overflows");
    for (int64_t t0 = 0; t0 < T; t0 += CG_GROUP) {
        const int64_t S = std::min<int64_t>(CG_GROUP, T - t0);
        CgBufs b;
        GPX_TRY(cg_state(g, std::min<int64_t>(CG_GROUP, T), &b));
        GPX_TRY(cg_make_probes(g, t0, S, seed, b.B));
        if (out) GPX_TRY(download_f64(g->dtype, out + t0 * g->n, g->n, b.B, g->ldn, S, g->n, 0, g->st));
    }
    GPX_HIP(hipStreamSynchronize(g->st));
    return GPX_OK;
}

int gpx_cg_lh(gpx_cg_t *g, const double *params, double s, const double *Z, int64_t T, uint64_t seed, double tol, int64_t maxiter,
              int want_grad, double *rho0, int *iters, double *relres, double *coef, double *scalars, double *sums, double *grad)
{
    CG_ENTER(g);
    CG_NEED_PRECOND(g, params, s);
    GPX_ARG(T >= 1, "need T >= 1");
    GPX_ARG(tol >= 0.0 && tol <= 1.79769313486231570e308, "tol must be >= 0 and finite");
    GPX_ARG(maxiter >= 0 && maxiter <= 0x7fffffff, "maxiter must lie in 0 .. 2^31 - 1");
    GPX_ARG(rho0 && iters && relres && coef && scalars && (!want_grad || (sums && grad)), "NULL argument");
    GPX_ARG(T <= INT64_MAX / std::max<int64_t>(g->n, 2 * maxiter), "T * n overflows");
    const int64_t n = g->n, ldn = g->ldn;
    hipStream_t st = g->st;
    int64_t G = 0;
    GPX_TRY(cg_group_now(&G));
    const size_t pdoubles = want_grad ? dloglh_partial_doubles(g->kernel, g->d) : 0;
    const int width = (int)(dloglh_partial_doubles(g->kernel, g->d) / GR_BLOCKS);
    const CgLhLayout lay = cg_lh_layout(ldn, maxiter, pdoubles);
    bool grew = false;
    GPX_TRY(g->lh.reserve(lay.total, st, &grew));
    if (grew) GPX_HIP(hipMemsetAsync(g->lh.p, 0, g->lh.bytes, st));      // (Zt's columns [n, ldn) stay zero: the copies bring zeros)
    char *lb = (char *)g->lh.p;
    const CgRecord rec = {(double *)(lb + lay.hist), (double *)(lb + lay.rho0), (double *)(lb + lay.Zt)};
    double *part = (double *)(lb + lay.part);
    CgPass pass(g);
    GPX_TRY(pass.begin());
    CgBufs b;
    GPX_TRY(cg_state(g, std::min<int64_t>(G, T), &b));
    if (!g->have_alpha) {                                         // by gpx_cg_solve's rules for B == NULL
        int it1 = 0;
        double rr1 = 0.0;
        int64_t its = 0;
        GPX_TRY(cg_solve_y(g, b, tol, maxiter, &it1, &rr1, &its));
        pass.group(its);
    }
    GPX_TRY(cg_dot<false>((const double *)g->y, (double *)g->alpha, 1, g, 1.0, b.part));
    GPX_TRY(cg_fin(CG_FIN_ACC, 1, 0, 0.0, g, b));
    GPX_HIP(hipMemcpyAsync(&scalars[1], b.sc->acc, sizeof(double), hipMemcpyDeviceToHost, st));
    GPX_TRY(cg_logdet_precond(g, &scalars[0]));                   // (synchronises: y . alpha has arrived)
    GPX_TRY(g->tl.mark(st, CG_T_VECTOR));
    const CgView v = cg_view(g);
    double launch[GPX_ARD_MAX_D + 2];
    if (want_grad) for (int q = 0; q < width; ++q) sums[q] = 0.0;
    for (int64_t i = 0; i < T * maxiter * 2; ++i) coef[i] = 0.0;
    std::vector<double> hh;
    double hrho[CG_GROUP];
    for (int64_t t0 = 0; t0 < T; t0 += G) {
        const int64_t S = std::min<int64_t>(G, T - t0);
        if (Z) GPX_TRY(upload_f64(g->dtype, b.B, ldn, Z + t0 * n, n, S, n, st));
        else GPX_TRY(cg_make_probes(g, t0, S, seed, b.B));
        GPX_HIP(hipMemsetAsync(rec.hist, 0, (size_t)maxiter * 2 * CG_GROUP * 8, st));
        GPX_TRY(g->tl.mark(st, TL_NOBODY));
        int64_t its = 0;
        GPX_TRY(cg_solve_group(g, b, S, tol, maxiter, iters + t0, relres + t0, &its, &rec));
        pass.group(its);
        // ONE download of the group's history
        hh.resize((size_t)std::max<int64_t>(its, 1) * 2 * CG_GROUP);
        if (its > 0) GPX_HIP(hipMemcpyAsync(hh.data(), rec.hist, (size_t)its * 2 * CG_GROUP * 8, hipMemcpyDeviceToHost, st));
        GPX_HIP(hipMemcpyAsync(hrho, rec.rho0, sizeof(hrho), hipMemcpyDeviceToHost, st));
        GPX_HIP(hipStreamSynchronize(st));
        for (int64_t c = 0; c < S; ++c) {
            rho0[t0 + c] = hrho[c];
            for (int64_t it = 0; it < its; ++it) {
                coef[((t0 + c) * maxiter + it) * 2] = hh[(size_t)it * 2 * CG_GROUP + c];
                coef[((t0 + c) * maxiter + it) * 2 + 1] = hh[(size_t)it * 2 * CG_GROUP + CG_GROUP + c];
            }
        }
        if (want_grad) {                                          // U = -W / T (in place: b.X is the group's), V = Zt
            double *X = b.X;
            const double scale = -1.0 / (double)T;
            GPX_TRY(map_rows(S, n, st, [=] __device__(int64_t r, int64_t c) { X[r * ldn + c] = scale * X[r * ldn + c]; }));
            GPX_TRY(lowrank_reduce(g->kernel, v.x, n, g->d, v.params, b.X, rec.Zt, ldn, S, part, launch, st));
            for (int q = 0; q < width; ++q) sums[q] += launch[q];
        }
        GPX_TRY(g->tl.mark(st, TL_NOBODY));
    }
    if (want_grad) {
        GPX_TRY(lowrank_reduce(g->kernel, v.x, n, g->d, v.params, (const double *)g->alpha, (const double *)g->alpha, ldn, 1, part, launch, st));
        for (int q = 0; q < width; ++q) sums[q] += launch[q];
        // last = alpha . alpha - the trace's estimate: d/ds = s * last (dK/ds = 2 s I)
        grad_from_sums(g->kernel, g->d, g->params, sums, 0.0, -g->s, 0.5, grad);
        GPX_TRY(g->tl.mark(st, TL_NOBODY));
    }
    GPX_TRY(pass.end());
    return GPX_OK;
}

int gpx_cg_last_timing(gpx_cg_t *g, float *ms6)
{
    GPX_ARG(g != nullptr && ms6, "NULL argument");
    GPX_ARG(g->have_precond, "there is no preconditioner (gpx_cg_precond)");
    for (int i = 0; i < CG_T_COUNT; ++i) ms6[i] = g->ms[i];
    return GPX_OK;
}

int gpx_cg_device_bytes(gpx_cg_t *g, size_t *bytes)
{
    GPX_ARG(g != nullptr && bytes, "NULL argument");
    const size_t pts = (size_t)g->n * g->d * 8;
    *bytes = pts + (g->xs ? pts : 0) + 2 * (size_t)g->ldn * 8 + g->sel.bytes + g->pre.bytes + g->state.bytes + g->lh.bytes;
    return GPX_OK;
}

}  // extern "C"
