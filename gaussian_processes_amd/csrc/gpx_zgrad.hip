// gpx_zgrad.hip -- the rectangular tile pass of the sparse GP's gradient in the inducing inputs (gfx950): rect_zgrad,
// gpx_d_rect_zgrad.  The pieces it shares with the tile reductions of gpx_kmat.hip and the streamed kernels of gpx_stream.hip
// (the pair evaluation, the dtype dispatch, the LDS limit) are those of gpx_kernels_dev.h, gpx_small.h and gpx_common.h.
#include "gpx_common.h"
#include "gpx_kernels_dev.h"
#include "gpx_small.h"
#include <algorithm>

namespace gpx {

// ---------------------------------------------------------------------------
// The rectangular pass whose result is per COLUMN point and dimension, not per workgroup: the sparse GP's gradient in the
// inducing inputs (gpx_sparse.hip),
//   out[i, k] += scale * sum_j (C[j, i] + u_j v_i) dk(q_i, r_j)/dq_ik         rows r (n, d), columns q (m, d), C n x ldc
//   gaussian  dk(a, b)/da_k = -(a_k - b_k) / w^2 * k        periodic (d = 1)  dk(a, b)/da = -sin((a - b) / p) / (p w^2) * k
// rect_tile_kernel's tile (64 x 64, a thread one column and 16 rows, C read coalesced along the columns), but workgroup
// (bx, by, bz) KEEPS column tile bx -- its points are staged once, this window's coordinates of the thread's column live in
// registers -- and walks the by-th slice of the row tiles for the bz-th window of DP dimensions.  Per tile a thread forms the
// squared distances of its 16 pairs over ALL d dimensions and k in T, as the matrix build forms them (the clamp included: a
// clamped pair adds exactly 0), g = coef k in f64, and then for each dimension of the window acc[kk] += g (r_jk - q_ik): the
// difference itself, never q_ik sum g - sum g r_jk, which cancels far from the origin (pred_grad_kernel's rule).  The
// constant of the derivative (1 / w^2, 1 / (p w^2)) and `scale` enter once, in the slice sum.  DP is a compile-time window with
// a uniform `k < d` guard, so every acc[kk] is a register (no scratch: DESIGN 3.3 has the resource lines): a ladder of 4, 16
// and 32, and beyond 32 dimensions cdiv(d, 32) windows, each of which evaluates k again (one window of 32 measured 26 - 34 %
// faster at d = 32 than two of 16: DESIGN 3.3).  The four waves are added through LDS in wave order, one partial is
// written per (row slice, column, dimension), rect_zgrad_sum_kernel adds the slices in slice order INTO out: no atomics.
// ---------------------------------------------------------------------------
constexpr int ZG_T = 64;                 // tile edge (the tile reductions' GR_T)
constexpr int ZG_TARGET_WGS = 1024;      // (column tiles x windows x slices) aimed at: the tile reductions' workgroup count
constexpr int ZG_MAX_SLICES = 64;

template <typename T, int KIND, int DP>
__global__ __launch_bounds__(256) void rect_zgrad_kernel(const T *__restrict__ r, int64_t n, const T *__restrict__ q, int64_t m, int d,
                                                           const T *__restrict__ C, int64_t ldc, const T *__restrict__ u,
                                                           const T *__restrict__ v, KParams kp, int64_t tiles_per_slice,
                                                           double *__restrict__ partial)
{
    static_assert(KIND == GPX_KERNEL_GAUSSIAN || DP == 1, "the periodic pass has d == 1");
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    T *s1 = reinterpret_cast<T *>(smem_raw);          // [ZG_T][d]   rows
    T *s2 = s1 + (size_t)ZG_T * d;                    // [d][ZG_T]   columns, transposed
    T *su = s2 + (size_t)ZG_T * d;                    // u rows
    double *red = reinterpret_cast<double *>(smem_raw);   // [3][DP][ZG_T], once the tiles are done with
    const int tid = threadIdx.x, col = tid & 63;
    const int rg = __builtin_amdgcn_readfirstlane(tid >> 6);      // (the wave's index: uniform, so the row reads broadcast)
    const int64_t c0 = (int64_t)blockIdx.x * ZG_T, gc = c0 + col;
    const int kbeg = (int)blockIdx.z * DP;            // this workgroup's window of dimensions
    for (int idx = tid; idx < ZG_T * d; idx += 256) {
        const int c = idx / d, k = idx - c * d;
        s2[(size_t)k * ZG_T + c] = (c0 + c < m) ? q[(c0 + c) * d + k] : (T)0;
    }
    __syncthreads();
    T qv[DP];
    double acc[DP];
#pragma unroll
    for (int kk = 0; kk < DP; ++kk) {
        qv[kk] = (kbeg + kk < d) ? s2[(size_t)(kbeg + kk) * ZG_T + col] : (T)0;
        acc[kk] = 0.0;
    }
    const double vk = (gc < m) ? (double)v[gc] : 0.0;
    // gaussian: c1, c2 of gaussian_entry; periodic: h, w, p
    const T c1 = (T)kp.c[0], c2 = (T)kp.c[1], per = (T)kp.c[2];
    const int64_t ntr = (n + ZG_T - 1) / ZG_T, tbeg = (int64_t)blockIdx.y * tiles_per_slice, tend = min(ntr, tbeg + tiles_per_slice);
    for (int64_t t = tbeg; t < tend; ++t) {
        const int64_t r0 = t * ZG_T, lim = (n - r0) * d;
        __syncthreads();
        for (int idx = tid; idx < ZG_T * d; idx += 256) s1[idx] = (idx < lim) ? r[r0 * d + idx] : (T)0;
        if (tid < ZG_T) su[tid] = (r0 + tid < n) ? u[r0 + tid] : (T)0;
        __syncthreads();
        // k of this thread's 16 pairs; the periodic kind keeps sin((r - q) / p) = 2 sin cos of the half angle for the pass below
        T kv[16], f[KIND == GPX_KERNEL_GAUSSIAN ? 1 : 16];
        if constexpr (KIND == GPX_KERNEL_GAUSSIAN) {
            T r2[16];
#pragma unroll
            for (int i = 0; i < 16; ++i) r2[i] = (T)0;
#pragma unroll 2
            for (int k = 0; k < d; ++k) {
                const T b = s2[(size_t)k * ZG_T + col];
#pragma unroll
                for (int i = 0; i < 16; ++i) {
                    const T tt = s1[(rg + 4 * i) * d + k] - b;
                    r2[i] = fma(tt, tt, r2[i]);
                }
            }
#pragma unroll
            for (int i = 0; i < 16; ++i) kv[i] = gaussian_entry<T, 0>(r2[i], c1, c2, (T)0, (T)0);
        } else {
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                T sn, cs;
                dev_sincos<T>((T)0.5 * (s1[rg + 4 * i] - qv[0]) / per, &sn, &cs);
                kv[i] = periodic_k<T>(sn * sn, c1, c2);
                f[i] = (T)2.0 * sn * cs;
            }
        }
        // g = coef k (0 for an entry outside the matrix: C is only read inside)
        double g[16];
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int row = rg + 4 * i;
            const int64_t gr = r0 + row;
            double gi = 0.0;
            if (gr < n && gc < m) gi = ((double)C[gr * ldc + gc] + (double)su[row] * vk) * (double)kv[i];
            g[i] = gi;
        }
#pragma unroll
        for (int kk = 0; kk < DP; ++kk) {
            if (kbeg + kk < d) {                                          // (uniform: d and the window are scalars)
                double a2 = 0.0;
#pragma unroll
                for (int i = 0; i < 16; ++i) {
                    const T df = KIND == GPX_KERNEL_GAUSSIAN ? s1[(rg + 4 * i) * d + kbeg + kk] - qv[kk] : f[i];
                    a2 = fma(g[i], (double)df, a2);
                }
                acc[kk] += a2;
            }
        }
    }
    // the four waves, in wave order, through the LDS the tiles no longer need
    __syncthreads();
    if (rg > 0) {
#pragma unroll
        for (int kk = 0; kk < DP; ++kk) red[((size_t)(rg - 1) * DP + kk) * ZG_T + col] = acc[kk];
    }
    __syncthreads();
    if (rg == 0 && gc < m) {
#pragma unroll
        for (int kk = 0; kk < DP; ++kk) {
            if (kbeg + kk < d) {
                const double sum = ((acc[kk] + red[(size_t)kk * ZG_T + col]) + red[((size_t)DP + kk) * ZG_T + col]) +
                                   red[((size_t)2 * DP + kk) * ZG_T + col];
                partial[((int64_t)blockIdx.y * m + gc) * d + kbeg + kk] = sum;
            }
        }
    }
}

// out[i, k] += factor * (sum over the slices, in slice order) [/ div.w[k]]
template <bool DIV>
__global__ void rect_zgrad_sum_kernel(const double *__restrict__ partial, int nslice, int64_t md, int d, double factor, ArdWidths div,
                                      double *__restrict__ out)
{
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= md) return;
    double sum = 0.0;
    for (int y = 0; y < nslice; ++y) sum += partial[(int64_t)y * md + e];
    sum *= factor;
    if (DIV) sum /= div.w[e % d];
    out[e] += sum;
}

// the window of dimensions and the row slices of a pass: functions of (kernel, m, d) alone, so that results do not depend on n's
// split into chunks beyond the order of the additions.  d <= 4: one window of 4; d <= 16: one of 16; else windows of 32;
// enough slices for (column tiles x windows x slices) to reach ZG_TARGET_WGS, at most ZG_MAX_SLICES
static inline int zgrad_dp(int kernel, int d) { return kernel != GPX_KERNEL_GAUSSIAN ? 1 : (d <= 4 ? 4 : (d <= 16 ? 16 : 32)); }
static inline int64_t zgrad_slices(int kernel, int64_t m, int d)
{
    const int64_t wgs = cdiv(m, ZG_T) * cdiv(d, zgrad_dp(kernel, d));
    return std::min<int64_t>(ZG_MAX_SLICES, std::max<int64_t>(1, cdiv(ZG_TARGET_WGS, wgs)));
}

size_t rect_zgrad_partial_doubles(int kernel, int64_t m, int d) { return (size_t)zgrad_slices(kernel, m, d) * (size_t)m * (size_t)d; }

int rect_zgrad(int dtype, int kernel, const void *r, int64_t n, const void *q, int64_t m, int d, const double *params, const void *C,
               int64_t ldc, const void *u, const void *v, double scale, const double *col_div, double *partial_dev, double *out_dev,
               hipStream_t st)
{
    if (n < 1 || m < 1 || d < 1 || ldc < m) { set_error("rect_zgrad: need n, m, d >= 1 and ldc >= m"); return GPX_ERR_ARG; }
    if (kernel != GPX_KERNEL_GAUSSIAN && kernel != GPX_KERNEL_PERIODIC) { set_error("rect_zgrad: unknown kernel family %d", kernel); return GPX_ERR_ARG; }
    if (kernel == GPX_KERNEL_PERIODIC && d != 1) { set_error("rect_zgrad: the periodic family needs d == 1"); return GPX_ERR_UNSUPPORTED; }
    if (col_div && d > GPX_ARD_MAX_D) { set_error("rect_zgrad: column divisors need d <= %d (got %d)", GPX_ARD_MAX_D, d); return GPX_ERR_ARG; }
    KParams kp;
    GPX_TRY(make_kparams(kernel, GPX_K, params, 0.0, &kp));
    const int DP = zgrad_dp(kernel, d);
    const int64_t windows = cdiv(d, DP), ntr = cdiv(n, ZG_T);
    const int64_t tps = cdiv(ntr, std::min(ntr, zgrad_slices(kernel, m, d))), nslice = cdiv(ntr, tps);   // (no slice is empty)
    // the derivative's constant: gaussian 1 / w^2 = -2 c1, periodic 1 / (p w^2)
    const double factor = scale * (kernel == GPX_KERNEL_GAUSSIAN ? -2.0 * kp.c[0] : 1.0 / (kp.c[2] * kp.c[1] * kp.c[1]));
    ArdWidths aw;
    for (int k = 0; k < GPX_ARD_MAX_D; ++k) aw.w[k] = (col_div && k < d) ? col_div[k] : 1.0;
    const dim3 grid((unsigned)cdiv(m, ZG_T), (unsigned)nslice, (unsigned)windows), block(256);
    const int64_t md = m * d;
    ProfScope prof(PC_SPARSE_ZGRAD, (double)n * (double)m * (double)windows, st);
#define GPX_ZGRAD_LAUNCH(KIND, DPV)                                                                                                \
    do {                                                                                                                           \
        if (smem > 48 * 1024) GPX_TRY(set_max_lds((const void *)rect_zgrad_kernel<T, KIND, DPV>, LDS_TILE_MAX));                   \
        hipLaunchKernelGGL((rect_zgrad_kernel<T, KIND, DPV>), grid, block, smem, st, (const T *)r, n, (const T *)q, m, d, (const T *)C, \
                           ldc, (const T *)u, (const T *)v, kp, tps, partial_dev);                                                 \
    } while (0)
    const int rc = by_dtype(dtype, [&](auto t) -> int {
        using T = decltype(t);
        // the staged tile (two point sets and u), then the waves' sums
        const size_t smem = std::max(((size_t)2 * ZG_T * d + ZG_T) * sizeof(T), (size_t)3 * DP * ZG_T * sizeof(double));
        if (smem > (size_t)LDS_TILE_MAX) { set_error("rect_zgrad: d = %d too large for the LDS-staged tile", d); return GPX_ERR_UNSUPPORTED; }
        if (kernel != GPX_KERNEL_GAUSSIAN) GPX_ZGRAD_LAUNCH(GPX_KERNEL_PERIODIC, 1);
        else if (DP == 4) GPX_ZGRAD_LAUNCH(GPX_KERNEL_GAUSSIAN, 4);
        else if (DP == 16) GPX_ZGRAD_LAUNCH(GPX_KERNEL_GAUSSIAN, 16);
        else GPX_ZGRAD_LAUNCH(GPX_KERNEL_GAUSSIAN, 32);
        GPX_LAUNCH_CHECK();
        return GPX_OK;
    });
#undef GPX_ZGRAD_LAUNCH
    GPX_TRY(rc);
    if (col_div)
        hipLaunchKernelGGL((rect_zgrad_sum_kernel<true>), dim3((unsigned)cdiv(md, 256)), dim3(256), 0, st, partial_dev, (int)nslice, md, d, factor, aw, out_dev);
    else
        hipLaunchKernelGGL((rect_zgrad_sum_kernel<false>), dim3((unsigned)cdiv(md, 256)), dim3(256), 0, st, partial_dev, (int)nslice, md, d, factor, aw, out_dev);
    GPX_LAUNCH_CHECK();
    return GPX_OK;
}

}  // namespace gpx

using namespace gpx;

extern "C" {

int gpx_rect_zgrad_scratch(int kernel, int64_t m, int d, size_t *doubles)
{
    GPX_ARG(doubles, "NULL argument");
    GPX_ARG(kernel == GPX_KERNEL_GAUSSIAN || kernel == GPX_KERNEL_PERIODIC, "unknown kernel family (the ARD family: GPX_KERNEL_GAUSSIAN)");
    GPX_ARG(m >= 1 && d >= 1, "need m >= 1 and d >= 1");
    *doubles = rect_zgrad_partial_doubles(kernel, m, d);
    return GPX_OK;
}

int gpx_d_rect_zgrad(int dtype, int kernel, const void *r, int64_t n, const void *q, int64_t m, int d, const double *params,
                     const void *C, int64_t ldc, const void *u, const void *v, double scale, const double *col_div,
                     double *partial_dev, double *out_dev, void *stream)
{
    GPX_TRY(ensure_device());
    GPX_ARG(dtype == GPX_F64 || dtype == GPX_F32, "dtype must be GPX_F64 or GPX_F32");
    GPX_ARG(n >= 0 && m >= 0 && d >= 1, "need n, m >= 0 and d >= 1");
    if (n == 0 || m == 0) return GPX_OK;
    GPX_ARG(r && q && params && C && u && v && partial_dev && out_dev, "NULL pointer");
    GPX_ARG(ldc >= m, "ldc < m");
    GPX_ARG(kernel == GPX_KERNEL_GAUSSIAN || kernel == GPX_KERNEL_PERIODIC,
            "unknown kernel family (the ARD family: scaled points, the isotropic constants and col_div = the widths)");
    return rect_zgrad(dtype, kernel, r, n, q, m, d, params, C, ldc, u, v, scale, col_div, partial_dev, out_dev, S(stream));
}

}  // extern "C"
