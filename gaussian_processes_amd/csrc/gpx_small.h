// gpx_small.h -- the three helpers behind every small element-wise launch: one dtype dispatch, one 2-D and one 1-D map
// kernel (and, at the end, the vector copy loop that the two triangular row copies share).  A wrapper's whole body is  by_dtype(dtype, [&](auto t) { using T = decltype(t); ... map_rows(rows, cols, st,
// [=] __device__(int64_t r, int64_t c) { ... }); });  -- the lambda IS the kernel.  (The blocks that are not templates --
// transpose, the single-workgroup reductions, eye_rows, tril -- are in gpx_small.hip.)
#pragma once
#include "gpx_common.h"
#include <algorithm>

namespace gpx {

// f(double()) or f(float()): inside the generic lambda `using T = decltype(t);` names the element type
template <typename F>
static inline int by_dtype(int dtype, F f) { return dtype == GPX_F64 ? f(double()) : f(float()); }

// f(r, c) for every r < rows, c < cols: grid (column blocks of 256, rows up to 32768), a row loop for what lies beyond
template <typename F>
__global__ __launch_bounds__(256) void map_rows_kernel(int64_t rows, int64_t cols, F f)
{
    const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= cols) return;
    for (int64_t r = blockIdx.y; r < rows; r += gridDim.y) f(r, c);
}

template <typename F>
static int map_rows(int64_t rows, int64_t cols, hipStream_t st, F f)
{
    if (rows <= 0 || cols <= 0) return GPX_OK;
    const dim3 grid((unsigned)cdiv(cols, 256), (unsigned)std::min<int64_t>(rows, 32768)), block(256);
    hipLaunchKernelGGL((map_rows_kernel<F>), grid, block, 0, st, rows, cols, f);
    GPX_LAUNCH_CHECK();
    return GPX_OK;
}

// f(i) for every i < n
template <typename F>
__global__ __launch_bounds__(256) void map_vec_kernel(int64_t n, F f)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) f(i);
}

template <typename F>
static int map_vec(int64_t n, hipStream_t st, F f)
{
    if (n <= 0) return GPX_OK;
    hipLaunchKernelGGL((map_vec_kernel<F>), dim3((unsigned)cdiv(n, 256)), dim3(256), 0, st, n, f);
    GPX_LAUNCH_CHECK();
    return GPX_OK;
}

// dv[v] = sv[v] for v < nv, whole 16-byte vectors, by the 256 threads of a workgroup: four loads in flight per lane, then the
// rest one at a time.  The caller says how far a row's vectors may reach (copy_lower_kernel: the vector that holds the
// diagonal; del_copy_rows_kernel: only whole vectors left of it)
template <typename VT>
__device__ __forceinline__ void copy_vecs(const VT *__restrict__ sv, VT *__restrict__ dv, int64_t nv)
{
    int64_t v = threadIdx.x;
    for (; v + 3 * 256 < nv; v += 4 * 256) {
        VT t[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) t[u] = sv[v + u * 256];
#pragma unroll
        for (int u = 0; u < 4; ++u) dv[v + u * 256] = t[u];
    }
    for (; v < nv; v += 256) dv[v] = sv[v];
}

}  // namespace gpx
