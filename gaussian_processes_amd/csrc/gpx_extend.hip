// gpx_extend.hip -- growing a fitted GP by k observations without refactoring (gpx_gp_extend, gpx_gp_extend_from_K).
//
// The Cholesky factor of a bordered matrix is the old factor with k rows appended:
//   K' = [ K   B^T ]     L' = [ L   0  ]     X  = B L^-T                 (k x n)
//        [ B   C   ]          [ X   Ls ]     Ls Ls^T = C - X X^T         (k x k)
//   B = K(x_new, x),  C = K(x_new, x_new) + s^2 I
// One triangular sweep over k right-hand sides (trsm_right_lt, the sweep of cov / var / loo: n^2 k flops), a k x k Schur
// complement and its factorisation, two single-rhs solves for the new alpha (n^2 flops each).  What nothing else in the
// library does well is here: the re-pitched copy of the factor's lower trapezoid (copy_lower) and the Schur complement of
// a FEW rows against MANY columns (schur_lower).
#include "gpx_small.h"
#include <algorithm>

#include "gpx_gp_internal.h"
#include "gpx_kernels_dev.h"

namespace gpx {

// ---- the lower trapezoid of a factor, re-pitched ------------------------------------------------------------------------
// One workgroup per band of CL_ROWS rows; row i moves the 16-byte vectors [0, i / VEC] -- up to the one that holds the
// diagonal, which lies inside both pitches because they are multiples of VEC -- four loads in flight per lane, or, when a
// base or a pitch is not 16-byte aligned, exactly the elements [0, i] one at a time.  n (n + 1) / 2 elements each way: half
// of what a strided memcpy of the square moves.  (Row i is i + 1 elements long: the bands near the top are short, the ones
// near the bottom carry the traffic; 4 rows a band keeps n = 65536 at 16384 workgroups of at most 128 vectors a lane.)
constexpr int CL_ROWS = 4;

template <typename T>
__global__ __launch_bounds__(256) void copy_lower_kernel(const T *__restrict__ src, int64_t lds, T *__restrict__ dst, int64_t ldd,
                                                         int64_t n, int aligned)
{
    constexpr int VEC = Vec<T>::N;
    typedef typename Vec<T>::type VT;
    const int tid = threadIdx.x;
    const int64_t r0 = (int64_t)blockIdx.x * CL_ROWS, r1 = r0 + CL_ROWS < n ? r0 + CL_ROWS : n;
    for (int64_t row = r0; row < r1; ++row) {
        const T *__restrict__ s = src + row * lds;
        T *__restrict__ d = dst + row * ldd;
        if (aligned) {
            const VT *__restrict__ sv = reinterpret_cast<const VT *>(s);
            VT *__restrict__ dv = reinterpret_cast<VT *>(d);
            copy_vecs(sv, dv, row / VEC + 1);              // vectors up to the diagonal's
        } else {
            for (int64_t c = tid; c <= row; c += 256) d[c] = s[c];
        }
    }
}

int copy_lower(int dtype, const void *src, int64_t lds, void *dst, int64_t ldd, int64_t n, hipStream_t st)
{
    if (n <= 0) return GPX_OK;
    const int64_t es = (int64_t)esize(dtype), ch = 16 / es;
    // vector mode: row n - 1 is moved up to column round_up(n, ch) - 1, which both pitches must hold
    const int aligned = lds % ch == 0 && ldd % ch == 0 && ((uintptr_t)src) % 16 == 0 && ((uintptr_t)dst) % 16 == 0 &&
                        lds >= round_up(n, ch) && ldd >= round_up(n, ch);
    const dim3 grid((unsigned)cdiv(n, CL_ROWS)), block(256);
    ProfScope prof(PC_EXTEND, (double)n * (double)(n + 1) * (double)es, st);     // n (n + 1) / 2 elements read and written
    return by_dtype(dtype, [&](auto t) {
        using T = decltype(t);
        hipLaunchKernelGGL((copy_lower_kernel<T>), grid, block, 0, st, (const T *)src, lds, (T *)dst, ldd, n, aligned);
        GPX_LAUNCH_CHECK();
        return GPX_OK;
    });
}

// ---- the Schur complement of few rows against many columns --------------------------------------------------------------
// S (k x k) -= B B^T with B k x n.  As one product this is cdiv(k, 128)^2 tiles that each walk all n columns: k <= 128 and
// n = 65536 is ONE workgroup with 2 * 128^2 * 65536 flops while every other CU idles.  B is cut into column slices; slice s
// yields the partial Gram P_s = B[:, slice] B[:, slice]^T through the product kernel's batch form (count = whole slices,
// sA = sB = slice width, beta = 0; the ragged last slice is a call of its own), and sum_slices_lower (gpx_sparse.hip) forms
// S[i, j] - sum_s P_s[i, j] for j <= i in f64, s ascending, and stores once.  No atomics: the same bits every time.
// The slice width: as many slices as give SCHUR_TARGET_WGS workgroups, but no slice narrower than SCHUR_MIN_SLICE
// columns, rounded up to 128 columns (a multiple of the product kernel's k-step in both dtypes).  Measured on builds with
// other values here (gpx_d_schur_lower alone, fp64, median ms at n = 8192 | 65536; profiles/extend_schur_sweep.json):
//   min slice  128: k = 1 0.051 | 0.203   k = 64 0.061 | 0.225        target  256: k = 1024 0.500 | 3.76
//              256:       0.055 | 0.150          0.060 | 0.161                 512:          0.273 | 1.88
//              512:       0.080 | 0.138          0.084 | 0.142                1024:          0.292 | 1.89
//             1024:       0.080 | 0.207          0.083 | 0.214                2048:          0.328 | 1.92
// One slice (n within a slice, or so many tiles that they fill the chip by themselves): no partials, no scratch, no
// reduction -- one product S -= B B^T on the lower tiles.
constexpr int64_t SCHUR_TARGET_WGS = 1024, SCHUR_MIN_SLICE = 256, SCHUR_SLICE_ALIGN = 128;

static thread_local ThreadScratch g_schur_scr;      // the slices' partial Grams

int schur_lower(int dtype, const void *B, int64_t k, int64_t n, int64_t ldb, void *S, int64_t lds, hipStream_t st)
{
    if (k <= 0 || n <= 0) return GPX_OK;
    const int64_t es = (int64_t)esize(dtype), ch = 16 / es;
    const int64_t tiles = cdiv(k, 128) * cdiv(k, 128);
    const int64_t want = std::max<int64_t>(1, SCHUR_TARGET_WGS / tiles);
    const int64_t W = round_up(std::max(SCHUR_MIN_SLICE, cdiv(n, want)), SCHUR_SLICE_ALIGN);
    const int64_t nfull = n / W, tail = n - nfull * W, slices = nfull + (tail > 0 ? 1 : 0);
    if (slices == 1) return gemm_nt(dtype, k, k, n, B, ldb, B, ldb, S, lds, -1.0, GPX_LOWER, 0, 0, st);
    if (slices > (int64_t)1 << 20) { set_error("schur_lower: too many column slices (%lld)", (long long)slices); return GPX_ERR_ARG; }
    const int64_t ldp = round_up(k, 16), sP = k * ldp;
    void *P = nullptr;
    GPX_TRY(g_schur_scr.get((size_t)slices * sP * es, &P));
    // beta = 0 exists on the aligned product kernel only; elsewhere (an unaligned B, the ragged slice) the partial is
    // cleared first and the product adds to it: one writer per element either way
    const bool fast = !tune().gemm_no_fast && ldb % ch == 0 && ((uintptr_t)B) % 16 == 0;
    if (nfull > 0) {
        Batch bt; bt.count = (int)nfull; bt.sA = W; bt.sB = W; bt.sC = sP;
        if (!fast) GPX_HIP(hipMemsetAsync(P, 0, (size_t)nfull * sP * es, st));
        GPX_TRY(gemm_nt(dtype, k, k, W, B, ldb, B, ldb, P, ldp, 1.0, GPX_FULL, 0, 0, st, fast ? 1 : 0, 0, &bt));
    }
    if (tail > 0) {
        const char *Bt = (const char *)B + nfull * W * es;
        char *Pt = (char *)P + nfull * sP * es;
        GPX_HIP(hipMemsetAsync(Pt, 0, (size_t)sP * es, st));
        GPX_TRY(gemm_nt(dtype, k, k, tail, Bt, ldb, Bt, ldb, Pt, ldp, 1.0, GPX_FULL, 0, 0, st));
    }
    const double elems = 0.5 * (double)k * (double)(k + 1);
    ProfScope prof(PC_EXTEND, elems * (double)(slices + 2) * (double)es, st);   // the partials and S read, S written
    return sum_slices_lower(dtype, P, ldp, sP, (int)slices, k, S, S, lds, st);
}

// ---- the handle ---------------------------------------------------------------------------------------------------------
// potrf of the Schur complement reports its j-th pivot; the whole (n + k) matrix would have reported n + j
__global__ void info_shift_kernel(int *info, int shift)
{
    if (*info > 0) *info += shift;
}

// Kno / Knn: the caller's B = K(x_new, x) and C = K(x_new, x_new) + s^2 I (plugin kernels), or both null
static int extend_impl(gpx_gp *g, const double *x_new, const double *y_new, int64_t k, const double *Kno, const double *Knn,
                       gpx_gp_t **out, int *info)
{
    const int64_t n = g->n, n2 = n + k, d = g->d, lda = g->lda;
    const size_t es = esize(g->dtype);
    GPX_TRY(gp_need_factor(g, "to extend"));
    route_hit(RT_EXTEND);
    gpx_gp_t *g2 = nullptr;
    GPX_TRY(gpx_gp_create(&g2, g->dtype, g->kernel, n2, g->d));
    struct Guard { gpx_gp_t *g; ~Guard() { if (g) gpx_gp_destroy(g); } } guard{g2};
    StreamTurn turn2(g2->st);                              // (this thread's scratch: the new handle's stream takes its turn)
    hipStream_t st = g2->st;
    GPX_TRY(order(g2->ev[5], g->st, st));                  // ... behind whatever the source's stream still holds
    const int64_t lda2 = g2->lda;
    // 1. the data: the old points device to device, the new ones uploaded behind them
    GPX_HIP(hipMemcpyAsync(g2->x, g->x, (size_t)n * d * es, hipMemcpyDeviceToDevice, st));
    GPX_HIP(hipMemcpyAsync(g2->y, g->y, (size_t)n * es, hipMemcpyDeviceToDevice, st));
    GPX_TRY(upload_f64(g->dtype, (char *)g2->x + (size_t)n * d * es, k * d, x_new, k * d, 1, k * d, st));
    GPX_TRY(upload_f64(g->dtype, (char *)g2->y + (size_t)n * es, k, y_new, k, 1, k, st));
    memcpy(g2->params, g->params, sizeof(g->params));
    g2->s = g->s;
    g2->have_data = true; g2->have_params = g->have_params;
    GPX_TRY(gp_rescale(g2));
    GPX_TRY(gp_scan_finite(g2));
    if (!g2->x_finite) { set_error("array must not contain infs or NaNs (x_new)"); return GPX_ERR_ARG; }
    const GpView v = gp_view(g2);
    const char *xn = (const char *)v.x + (size_t)n * d * es;
    char *A2 = (char *)g2->A, *X = A2 + (size_t)n * lda2 * es;     // rows [n, n2): 16-byte aligned, lda2 is a multiple of 16
    int *info_dev = &g2->scal->info;
    GPX_HIP(hipEventRecord(g2->ev[0], st));
    // 2. B = K(x_new, x) into rows [n, n2) x columns [0, n)
    if (Kno) GPX_TRY(upload_f64(g->dtype, X, lda2, Kno, n, k, n, st));
    else GPX_TRY(kmat(g->dtype, v.kernel, GPX_K, xn, k, v.x, n, g->d, v.params, 0.0, GPX_FULL, X, lda2, st));
    GPX_HIP(hipEventRecord(g2->ev[1], st));
    // 3. the old factor, re-pitched
    GPX_TRY(copy_lower(g->dtype, g->A, lda, A2, lda2, n, st));
    // 4. X <- B L^-T against the SOURCE's factor and operators: the operator route exactly where gpx_gp_cov takes it
    GPX_TRY(trsm_right_lt(g->dtype, g->A, n, lda, X, k, lda2, st, 0, &g->ops));
    // 5. C - X X^T in an aligned scratch block (the diagonal block's own base, n (lda2 + 1), is not 16-byte aligned for
    // odd n in fp64 or n % 4 != 0 in fp32), factored there, its lower triangle copied to rows and columns [n, n2)
    const int64_t ldc = round_up(k, 16);
    DevBuf C;
    GPX_TRY(C.alloc((size_t)k * ldc * es));
    if (Knn) GPX_TRY(upload_f64(g->dtype, C.p, ldc, Knn, k, k, k, st));
    else GPX_TRY(kmat(g->dtype, v.kernel, GPX_K, xn, k, xn, k, g->d, v.params, g->s * g->s, GPX_LOWER, C.p, ldc, st));
    GPX_TRY(schur_lower(g->dtype, X, k, n, lda2, C.p, ldc, st));
    GPX_TRY(potrf(g->dtype, C.p, k, ldc, info_dev, st));
    hipLaunchKernelGGL(info_shift_kernel, dim3(1), dim3(1), 0, st, info_dev, (int)n);
    GPX_LAUNCH_CHECK();
    GPX_TRY(copy_lower(g->dtype, C.p, ldc, A2 + ((size_t)n * lda2 + n) * es, lda2, k, st));
    GPX_HIP(hipEventRecord(g2->ev[2], st));
    // 6. the tail of gpx_gp_fit, both sweeps; the new factor's operators are built lazily.  (It waits for the stream: the
    // scratch block C is free to go)
    g2->ops.invalidate();
    GPX_TRY(gp_finish_fit(g2, false, info));
    guard.g = nullptr;
    *out = g2;
    return GPX_OK;
}

}  // namespace gpx

using namespace gpx;

extern "C" {

int gpx_d_copy_lower(int dtype, const void *src, int64_t lds, void *dst, int64_t ldd, int64_t n, void *stream)
{
    gpx::tune_refresh();
    GPX_ARG(dtype == GPX_F64 || dtype == GPX_F32, "dtype must be GPX_F64 or GPX_F32");
    GPX_ARG(n >= 0, "n < 0");
    if (n == 0) return GPX_OK;
    GPX_ARG(src && dst && src != dst, "NULL pointer or src == dst");
    GPX_ARG(lds >= n && ldd >= n, "leading dimension too small");
    GPX_TRY(ensure_device());
    return copy_lower(dtype, src, lds, dst, ldd, n, S(stream));
}

int gpx_d_schur_lower(int dtype, const void *B, int64_t k, int64_t n, int64_t ldb, void *Sm, int64_t lds, void *stream)
{
    gpx::tune_refresh();
    gpx::StreamTurn turn__((hipStream_t)stream);     // (this thread's scratch buffers: one stream at a time, gpx_mem.h)
    GPX_ARG(dtype == GPX_F64 || dtype == GPX_F32, "dtype must be GPX_F64 or GPX_F32");
    GPX_ARG(k >= 0 && n >= 0, "negative dimension");
    if (k == 0 || n == 0) return GPX_OK;
    GPX_ARG(B && Sm, "NULL pointer");
    GPX_ARG(ldb >= n && lds >= k, "leading dimension too small");
    GPX_TRY(ensure_device());
    return schur_lower(dtype, B, k, n, ldb, Sm, lds, S(stream));
}

int gpx_gp_extend(gpx_gp_t *g, const double *x_new, const double *y_new, int64_t k, gpx_gp_t **out, int *info)
{
    if (out) *out = nullptr;
    GP_ENTER(g);
    GPX_ARG(out && info && x_new && y_new, "NULL argument");
    GPX_ARG(k >= 1, "need k >= 1");
    GPX_ARG(g->fitted && g->have_data && g->have_params, "gp is not fitted (from kernel parameters: a handle fitted from set_K extends with gpx_gp_extend_from_K)");
    return extend_impl(g, x_new, y_new, k, nullptr, nullptr, out, info);
}

int gpx_gp_extend_from_K(gpx_gp_t *g, const double *x_new, const double *y_new, int64_t k, const double *Knew_old,
                         const double *Knew_new, gpx_gp_t **out, int *info)
{
    if (out) *out = nullptr;
    GP_ENTER(g);
    GPX_ARG(out && info && x_new && y_new && Knew_old && Knew_new, "NULL argument");
    GPX_ARG(k >= 1, "need k >= 1");
    GPX_ARG(g->fitted && g->have_data, "gp is not fitted");
    return extend_impl(g, x_new, y_new, k, Knew_old, Knew_new, out, info);
}

}  // extern "C"
