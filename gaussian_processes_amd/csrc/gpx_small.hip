// gpx_small.hip -- the small device blocks that more than one translation unit uses and that are no element map: the
// transpose, the single-workgroup reductions, the identity seed and tril.  (The element maps are one-line lambdas at their
// call sites, through gpx_small.h.)
#include "gpx_small.h"

namespace gpx {

// ---- transpose ---------------------------------------------------------------------------------------------------------
// dst (cols x rows, ldd) <- src (rows x cols, lds)^T through 32 x 32 LDS tiles: loads and stores both run along a row, every
// index is checked against rows / cols.  mirror: src == dst is allowed (no __restrict__), only the tiles at or below the
// diagonal are read and only elements strictly above it are written -- nobody reads what another workgroup writes.
// (32, not the 64 of transpose_subdiag_kernel: measured on every shape the callers have -- squares of 200 to 4096, the
// 256- and 512-row panels of L -- the smaller tile is the faster one in both dtypes, but for the 512 x 8192 fp64 panel,
// where it costs 1.2 us of 12)
template <typename T>
__global__ __launch_bounds__(256) void transpose_kernel(const T *src, int64_t lds, int64_t rows, int64_t cols, T *dst, int64_t ldd, int mirror)
{
    __shared__ T tile[32][33];
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    const int64_t bi = blockIdx.y, bj = blockIdx.x;        // tile row / tile column of src
    if (mirror && bj > bi) return;
    for (int r = ty; r < 32; r += 8) {
        const int64_t i = bi * 32 + r, j = bj * 32 + tx;
        if (i < rows && j < cols) tile[r][tx] = src[i * lds + j];
    }
    __syncthreads();
    for (int r = ty; r < 32; r += 8) {
        const int64_t oi = bj * 32 + r, oj = bi * 32 + tx; // dst[oi, oj] = src[oj, oi] = tile[tx][r]
        if (oi < cols && oj < rows && (!mirror || oj > oi)) dst[oi * ldd + oj] = tile[tx][r];
    }
}

int transpose(int dtype, const void *src, int64_t lds, int64_t rows, int64_t cols, void *dst, int64_t ldd, int mirror, hipStream_t st)
{
    if (rows <= 0 || cols <= 0) return GPX_OK;
    if (cdiv(rows, 32) > 65535) { set_error("transpose: %lld rows are beyond the grid", (long long)rows); return GPX_ERR_ARG; }
    const dim3 grid((unsigned)cdiv(cols, 32), (unsigned)cdiv(rows, 32)), block(256);
    ProfScope prof(PC_TRANSPOSE, (double)rows * (double)cols * (mirror ? 1.0 : 2.0) * (double)esize(dtype), st);
    return by_dtype(dtype, [&](auto t) {
        using T = decltype(t);
        hipLaunchKernelGGL((transpose_kernel<T>), grid, block, 0, st, (const T *)src, lds, rows, cols, (T *)dst, ldd, mirror);
        GPX_LAUNCH_CHECK();
        return GPX_OK;
    });
}

// ---- reductions (single workgroup, fixed order => deterministic) ----------
template <typename T, int MODE>   // MODE 0: sum a[i]*b[i]   1: 2*sum log a[i*stride]   2: sum a[i*stride]
__global__ __launch_bounds__(1024) void reduce_kernel(const T *__restrict__ a, const T *__restrict__ b,
                                                      int64_t n, int64_t stride, double *__restrict__ out,
                                                      int64_t sa, int64_t sb, int64_t so)
{
    // batched: workgroup blockIdx.x reduces vector pair blockIdx.x into out[blockIdx.x * so]
    a += (int64_t)blockIdx.x * sa;
    if (MODE == 0) b += (int64_t)blockIdx.x * sb;
    out += (int64_t)blockIdx.x * so;
    __shared__ double red[16];
    const int tid = threadIdx.x;
    double acc = 0.0;
    for (int64_t i = tid; i < n; i += 1024) {
        if (MODE == 0) acc = fma((double)a[i], (double)b[i], acc);
        else if (MODE == 1) acc += log((double)a[i * stride]);
        else acc += (double)a[i * stride];
    }
    for (int off = 32; off > 0; off >>= 1) acc += __shfl_down(acc, off, 64);
    if ((tid & 63) == 0) red[tid >> 6] = acc;
    __syncthreads();
    if (tid == 0) {
        double s = 0.0;
        for (int w = 0; w < 16; ++w) s += red[w];
        out[0] = (MODE == 1) ? 2.0 * s : s;
    }
}

template <int MODE>
static int reduce(int dtype, const void *a, const void *b, int64_t n, int64_t stride, double *out_dev, hipStream_t st, int count,
                  int64_t sa, int64_t sb, int64_t so)
{
    return by_dtype(dtype, [&](auto t) {
        using T = decltype(t);
        hipLaunchKernelGGL((reduce_kernel<T, MODE>), dim3(count), dim3(1024), 0, st, (const T *)a, (const T *)b, n, stride, out_dev, sa, sb, so);
        GPX_LAUNCH_CHECK();
        return GPX_OK;
    });
}

// count > 1: matrix i at L + i * sL, result in out_dev[i * so]
int logdet_chol(int dtype, const void *L, int64_t n, int64_t ldl, double *out_dev, hipStream_t st, int count, int64_t sL, int64_t so)
{
    return reduce<1>(dtype, L, nullptr, n, ldl + 1, out_dev, st, count, sL, 0, so);
}

// count > 1: pair i is (a + i * sa, b + i * sb), result in out_dev[i * so]
int dot(int dtype, const void *a, const void *b, int64_t n, double *out_dev, hipStream_t st, int count, int64_t sa, int64_t sb, int64_t so)
{
    return reduce<0>(dtype, a, b, n, 1, out_dev, st, count, sa, sb, so);
}

int sum_f64(const double *a, int64_t n, double *out_dev, hipStream_t st) { return reduce<2>(GPX_F64, a, nullptr, n, 1, out_dev, st, 1, 0, 0, 0); }

int diag_sum(int dtype, const void *A, int64_t n, int64_t lda, double *out_dev, hipStream_t st)
{
    return reduce<2>(dtype, A, nullptr, n, lda + 1, out_dev, st, 1, 0, 0, 0);
}

// ---- the identity seed and tril ------------------------------------------------------------------------------------------
// X (rows x ld) <- rows [c0, c0 + rows) of the identity, columns [cz, ld) only (cz <= c0)
int eye_rows(int dtype, void *X, int64_t rows, int64_t ld, int64_t c0, int64_t cz, hipStream_t st)
{
    return by_dtype(dtype, [&](auto t) {
        using T = decltype(t);
        T *x = (T *)X;
        return map_rows(rows, ld - cz, st, [=] __device__(int64_t r, int64_t c) { x[r * ld + cz + c] = (cz + c == c0 + r) ? (T)1 : (T)0; });
    });
}

// the strict upper triangle <- 0.  The grid is shaped for that triangle alone (at most 64 column blocks, each striding on
// from the diagonal of its row): no map_rows
template <typename T>
__global__ void tril_kernel(T *__restrict__ A, int64_t n, int64_t lda)
{
    for (int64_t i = blockIdx.y; i < n; i += gridDim.y)
        for (int64_t c = i + 1 + (int64_t)blockIdx.x * blockDim.x + threadIdx.x; c < n;
             c += (int64_t)gridDim.x * blockDim.x)
            A[i * lda + c] = (T)0;
}

int tril(int dtype, void *A, int64_t n, int64_t lda, hipStream_t st)
{
    if (n <= 1) return GPX_OK;
    const dim3 grid((unsigned)std::min<int64_t>(cdiv(n, 256), 64), (unsigned)std::min<int64_t>(n, 32768)), block(256);
    return by_dtype(dtype, [&](auto t) {
        using T = decltype(t);
        hipLaunchKernelGGL((tril_kernel<T>), grid, block, 0, st, (T *)A, n, lda);
        GPX_LAUNCH_CHECK();
        return GPX_OK;
    });
}

}  // namespace gpx
