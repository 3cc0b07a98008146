// gpx_lrgrad.hip -- the tile reduction whose coefficients are LOW RANK and formed inside the tile (gpx_d_lowrank_reduce):
//   S_p  = sum_{j,i} c_ji dk(x_j, x_i)/dtheta_p,   c_ji = sum_{t<T} U[t, j] V[t, i],   last = sum_j c_jj
// for two blocks U, V of T row vectors (T x ld).  It is the hot kernel of the iterative GP's marginal-likelihood gradient
// (gpx_cg_lh, gpx_cg.hip), whose weights G = alpha alpha^T - (1/T) sum_t w_t zt_t^T exist only as such factors: tile_reduce
// and rect_reduce (gpx_kmat.hip) contract against an n x n matrix in memory, and this route must never have one.  Float64 only.
//
// The slots are tile_reduce's -- [P0, P1, P2, last] for the Gaussian and the periodic family, [S_0, S_1 .. S_d, last] for the
// ARD family on the scaled points with iso -- so grad_from_sums serves unchanged.
//
// Tile: 64 x 64 entries by 256 threads; a thread owns one column and the 16 consecutive rows of its wave.  Per tile the
// workgroup stages its 64 + 64 points (rows as they lie, columns transposed) and the T x 64 slices of U over the rows and
// of V over the columns in LDS: (2 * 64 d + 2 * 64 T) doubles, 64 KiB at d = 32, T = 32.  A thread then forms its 16
// coefficients by a T-long dot -- one conflict-free read of V per t (consecutive lanes, consecutive doubles) against 16 reads
// of U that the whole wave shares (one address: a broadcast, and 16 consecutive doubles: wide reads) -- then each pair's
// distance once and its derivatives once.  The walk covers EVERY tile of the square, not the lower triangle with the symmetrised
// coefficient c_ji + c_ij: that halves the kernel evaluations but doubles both the dots and the staged slices (U and V over the
// rows AND the columns, 96 KiB at d = T = 32: one workgroup per CU instead of two), and the dot is the larger half of a pair's
// work from T = d on.
// At most LR_T = 32 rows go per launch (a group of CG columns); a larger T is several launches whose sums the host adds in
// launch order.  One f64 partial per workgroup and quantity, added in workgroup order by the host: no atomics, the same bits
// in every call.
#include "gpx_small.h"
#include <algorithm>
#include <vector>

#include "gpx_kernels_dev.h"

namespace gpx {

constexpr int LR_T = 32;                      // rows of U and V per launch
constexpr int LR_ROWS = GR_T / 4;             // rows of a tile per wave, and per thread

// FAM: GPX_KERNEL_GAUSSIAN, GPX_KERNEL_PERIODIC (d == 1) or GPX_KERNEL_GAUSSIAN_ARD (x: the scaled points; c2: the Gaussian k's
// constant of iso; DMAX: the rung of the accumulator ladder that holds d -- 0 for the other families).  nt: the tile rows.
template <int FAM, int DMAX>
__global__ __launch_bounds__(256) void lowrank_tile_kernel(const double *__restrict__ x, int64_t n, int d, const double *__restrict__ U,
                                                           const double *__restrict__ V, int64_t ld, int T, GradParams gp, double c2,
                                                           int64_t nt, double *__restrict__ partial)
{
    constexpr bool ARD = FAM == GPX_KERNEL_GAUSSIAN_ARD;
    constexpr int NACC = ARD ? DMAX + 2 : 4;          // ARD: slot 0 S_0, 1 .. DMAX S_k, DMAX + 1 last; otherwise 3 parameters + last
    constexpr int LAST = NACC - 1;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    double *s1 = reinterpret_cast<double *>(smem_raw);        // [GR_T][d]   rows
    double *s2 = s1 + (size_t)GR_T * d;                       // [d][GR_T]   columns, transposed
    double *su = s2 + (size_t)GR_T * d;                       // [T][GR_T]   U over the rows
    double *sv = su + (size_t)T * GR_T;                       // [T][GR_T]   V over the columns
    __shared__ double red[4][NACC];
    const int tid = threadIdx.x, col = tid & 63;
    const int rb = __builtin_amdgcn_readfirstlane(tid >> 6) * LR_ROWS;       // (the wave's first row: uniform, so the row reads broadcast)
    double acc[NACC];
#pragma unroll
    for (int k = 0; k < NACC; ++k) acc[k] = 0.0;
    const int64_t total = nt * nt;
    for (int64_t t = blockIdx.x; t < total; t += gridDim.x) {
        const int64_t tr = t / nt, tc = t - tr * nt;
        const int64_t r0 = tr * GR_T, c0 = tc * GR_T;
        __syncthreads();
        for (int idx = tid; idx < GR_T * d; idx += 256) {
            const int r = idx / d, k = idx - r * d;
            s1[idx] = (r0 + r < n) ? x[(r0 + r) * d + k] : 0.0;
            s2[(size_t)k * GR_T + r] = (c0 + r < n) ? x[(c0 + r) * d + k] : 0.0;
        }
        for (int idx = tid; idx < T * GR_T; idx += 256) {     // (the pads of U and V beyond n are never read)
            const int tt = idx >> 6, c = idx & 63;
            su[idx] = (r0 + c < n) ? U[(int64_t)tt * ld + r0 + c] : 0.0;
            sv[idx] = (c0 + c < n) ? V[(int64_t)tt * ld + c0 + c] : 0.0;
        }
        __syncthreads();
        const int64_t gc = c0 + col;
        // the coefficients of this thread's 16 pairs: c_ji = sum_t U[t, j] V[t, i]
        double cf[LR_ROWS];
#pragma unroll
        for (int i = 0; i < LR_ROWS; ++i) cf[i] = 0.0;
        for (int tt = 0; tt < T; ++tt) {
            const double v = sv[tt * GR_T + col];
            const double *ur = su + tt * GR_T + rb;
#pragma unroll
            for (int i = 0; i < LR_ROWS; ++i) cf[i] = fma(ur[i], v, cf[i]);
        }
        if constexpr (ARD) {
            double r2[LR_ROWS];
#pragma unroll
            for (int i = 0; i < LR_ROWS; ++i) r2[i] = 0.0;
#pragma unroll 2
            for (int k = 0; k < d; ++k) {
                const double b = s2[(size_t)k * GR_T + col];
#pragma unroll
                for (int i = 0; i < LR_ROWS; ++i) {
                    const double tt = s1[(rb + i) * d + k] - b;
                    r2[i] = fma(tt, tt, r2[i]);
                }
            }
            double c[LR_ROWS];                                // c_ji k_ji; 0 for a pair outside the matrix
#pragma unroll
            for (int i = 0; i < LR_ROWS; ++i) {
                const int64_t gr = r0 + rb + i;
                double ci = 0.0;
                if (gr < n && gc < n) {
                    if (gr == gc) acc[LAST] += cf[i];
                    const double e = -0.5 * r2[i];
                    if (!(e < GPX_MIN_LOG)) ci = cf[i] * (c2 * exp(e));
                }
                c[i] = ci;
                acc[0] += ci;
            }
#pragma unroll
            for (int k = 0; k < DMAX; ++k) {
                if (k < d) {
                    const double b = s2[(size_t)k * GR_T + col];
                    double a2 = 0.0;
#pragma unroll
                    for (int i = 0; i < LR_ROWS; ++i) {
                        const double tt = s1[(rb + i) * d + k] - b;
                        a2 = fma(c[i], tt * tt, a2);
                    }
                    acc[1 + k] += a2;
                }
            }
        } else if constexpr (FAM == GPX_KERNEL_GAUSSIAN) {
            double r2[LR_ROWS];
#pragma unroll
            for (int i = 0; i < LR_ROWS; ++i) r2[i] = 0.0;
#pragma unroll 2
            for (int k = 0; k < d; ++k) {
                const double b = s2[(size_t)k * GR_T + col];
#pragma unroll
                for (int i = 0; i < LR_ROWS; ++i) {
                    const double tt = s1[(rb + i) * d + k] - b;
                    r2[i] = fma(tt, tt, r2[i]);
                }
            }
#pragma unroll
            for (int i = 0; i < LR_ROWS; ++i) {
                const int64_t gr = r0 + rb + i;
                if (gr < n && gc < n) {
                    if (gr == gc) acc[LAST] += cf[i];
                    const double e = gp.c1 * r2[i];
                    if (!(e < GPX_MIN_LOG)) {
                        const double ex = exp(e);
                        acc[0] += cf[i] * (gp.c2h * ex);
                        acc[1] += cf[i] * (ex * (gp.c3w * r2[i] - gp.c2w));
                    }
                }
            }
        } else {
#pragma unroll
            for (int i = 0; i < LR_ROWS; ++i) {
                const int64_t gr = r0 + rb + i;
                if (gr < n && gc < n) {
                    if (gr == gc) acc[LAST] += cf[i];
                    const double dd = s1[rb + i] - s2[col];   // d == 1
                    acc[0] += cf[i] * periodic_entry<double>(GPX_DK_DH, dd, gp.h, gp.w, gp.p);
                    acc[1] += cf[i] * periodic_entry<double>(GPX_DK_DW, dd, gp.h, gp.w, gp.p);
                    acc[2] += cf[i] * periodic_entry<double>(GPX_DK_DP, dd, gp.h, gp.w, gp.p);
                }
            }
        }
    }
    block_sum_fixed(acc, red, tid);
    __syncthreads();
    if constexpr (ARD) {
        if (tid < d + 2) partial[(int64_t)blockIdx.x * (d + 2) + tid] = block_sum_final(red, tid <= d ? tid : LAST);
    } else {
        if (tid < 4) partial[(int64_t)blockIdx.x * 4 + tid] = block_sum_final(red, tid);
    }
}

template <int FAM, int DMAX>
static int launch_lowrank(const double *x, int64_t n, int d, const double *U, const double *V, int64_t ld, int T, const GradParams &gpar,
                          double c2, unsigned grid, double *partial_dev, hipStream_t st)
{
    const size_t smem = ((size_t)2 * GR_T * d + (size_t)2 * GR_T * T) * sizeof(double);
    if (smem > (size_t)LDS_TILE_MAX) { set_error("low-rank tile reduction: d = %d too large for the LDS-staged tile", d); return GPX_ERR_UNSUPPORTED; }
    if (smem > 48 * 1024) GPX_TRY(set_max_lds((const void *)lowrank_tile_kernel<FAM, DMAX>, LDS_TILE_MAX));
    hipLaunchKernelGGL((lowrank_tile_kernel<FAM, DMAX>), dim3(grid), dim3(256), smem, st, x, n, d, U, V, ld, T, gpar, c2, cdiv(n, GR_T),
                       partial_dev);
    GPX_LAUNCH_CHECK();
    return GPX_OK;
}

int lowrank_reduce(int kernel, const void *x, int64_t n, int d, const double *params, const double *U, const double *V, int64_t ld,
                   int64_t T, double *partial_dev, double *out, hipStream_t st)
{
    if (n < 1 || T < 1 || ld < n || d < 1) { set_error("lowrank_reduce: need n, T, d >= 1 and ld >= n"); return GPX_ERR_ARG; }
    if (kernel == GPX_KERNEL_GAUSSIAN_ARD && d > GPX_ARD_MAX_D) { set_error("ARD gradient needs 1 <= d <= %d (got %d)", GPX_ARD_MAX_D, d); return GPX_ERR_ARG; }
    const int width = (int)(dloglh_partial_doubles(kernel, d) / GR_BLOCKS);
    const int64_t nt = cdiv(n, GR_T);
    const unsigned grid = (unsigned)std::min<int64_t>(GR_BLOCKS, nt * nt);
    GradParams gpar;
    double c2 = 0.0;
    if (kernel == GPX_KERNEL_GAUSSIAN_ARD) { memset(&gpar, 0, sizeof(gpar)); c2 = gaussian_k_const(params[0], params[1]); }
    else GPX_TRY(make_grad_params(kernel, d, params, &gpar));
    const double *xp = (const double *)x;
    std::vector<double> host((size_t)grid * width);
    for (int q = 0; q < width; ++q) out[q] = 0.0;
    for (int64_t t0 = 0; t0 < T; t0 += LR_T) {
        const int Tc = (int)std::min<int64_t>(LR_T, T - t0);
        const double *Uc = U + t0 * ld, *Vc = V + t0 * ld;
        route_hit(RT_LOWRANK);
        {
            ProfScope prof(PC_LOWRANK, (double)n * (double)n, st);
            if (kernel == GPX_KERNEL_GAUSSIAN_ARD)
                GPX_TRY(by_dmax(d, [&](auto dm) -> int {
                    return launch_lowrank<GPX_KERNEL_GAUSSIAN_ARD, decltype(dm)::value>(xp, n, d, Uc, Vc, ld, Tc, gpar, c2, grid, partial_dev, st);
                }));
            else if (kernel == GPX_KERNEL_GAUSSIAN) GPX_TRY((launch_lowrank<GPX_KERNEL_GAUSSIAN, 0>(xp, n, d, Uc, Vc, ld, Tc, gpar, c2, grid, partial_dev, st)));
            else GPX_TRY((launch_lowrank<GPX_KERNEL_PERIODIC, 0>(xp, n, d, Uc, Vc, ld, Tc, gpar, c2, grid, partial_dev, st)));
        }
        // this launch's partials in workgroup order, then the launches in launch order
        GPX_HIP(hipMemcpyAsync(host.data(), partial_dev, host.size() * sizeof(double), hipMemcpyDeviceToHost, st));
        GPX_HIP(hipStreamSynchronize(st));
        for (int q = 0; q < width; ++q) {
            double sum = 0.0;
            for (unsigned b = 0; b < grid; ++b) sum += host[(size_t)b * width + q];
            out[q] += sum;
        }
    }
    return GPX_OK;
}

static thread_local ThreadScratch g_lr_scr;     // gpx_d_lowrank_reduce: the per-workgroup partial sums

}  // namespace gpx

using namespace gpx;

extern "C" {

int gpx_d_lowrank_reduce(int dtype, int kernel, const void *x, int64_t n, int d, const double *params, const void *U, const void *V,
                         int64_t ld, int64_t T, double *out, void *stream)
{
    tune_refresh();
    GPX_ARG(dtype == GPX_F64 || dtype == GPX_F32, "dtype must be GPX_F64 or GPX_F32");
    if (dtype != GPX_F64) { set_error("gpx_d_lowrank_reduce: float64 only"); return GPX_ERR_UNSUPPORTED; }
    GPX_ARG(kernel == GPX_KERNEL_GAUSSIAN || kernel == GPX_KERNEL_PERIODIC || kernel == GPX_KERNEL_GAUSSIAN_ARD, "unknown kernel family");
    GPX_ARG(x && params && U && V && out, "NULL pointer");
    GPX_ARG(n >= 1 && d >= 1, "need n >= 1 and d >= 1");
    GPX_ARG(T >= 1, "need T >= 1");
    GPX_ARG(ld >= n, "ld < n");
    GPX_ARG(kernel != GPX_KERNEL_PERIODIC || d == 1, "the periodic family needs d == 1");
    GPX_ARG(kernel != GPX_KERNEL_GAUSSIAN_ARD || d <= GPX_ARD_MAX_D, "the ARD family needs d <= GPX_ARD_MAX_D");
    GPX_TRY(ensure_device());
    StreamTurn turn__((hipStream_t)stream);      // (this thread's scratch: one stream at a time, gpx_mem.h)
    void *partial = nullptr;
    GPX_TRY(g_lr_scr.get(dloglh_partial_doubles(kernel, d) * sizeof(double), &partial));
    return lowrank_reduce(kernel, x, n, d, params, (const double *)U, (const double *)V, ld, T, (double *)partial, out, (hipStream_t)stream);
}

}  // extern "C"
