// gpx_kernels_dev.h -- device-side entries of the two kernel families (shared by gpx_kmat.hip, gpx_stream.hip and
// gpx_deriv.hip): gp/ext/gaussian_c.pyx:18-164 and gp/ext/periodic_c.pyx:18-235 per matrix entry, and the pieces every
// kernel that stages points or sums over a workgroup is built from (DESIGN "Streamed reductions").
#pragma once
#include "gpx_common.h"

namespace gpx {

template <typename T> struct Vec;
template <> struct Vec<double> { static constexpr int N = 2; typedef double2 type; };
template <> struct Vec<float>  { static constexpr int N = 4; typedef float4 type; };

template <typename T> __device__ __forceinline__ T dev_exp(T x);
template <> __device__ __forceinline__ double dev_exp<double>(double x) { return exp(x); }
template <> __device__ __forceinline__ float  dev_exp<float>(float x)  { return expf(x); }
template <typename T> __device__ __forceinline__ void dev_sincos(T x, T *s, T *c);
template <> __device__ __forceinline__ void dev_sincos<double>(double x, double *s, double *c) { sincos(x, s, c); }
template <> __device__ __forceinline__ void dev_sincos<float>(float x, float *s, float *c) { sincosf(x, s, c); }

// one kernel-matrix entry from the accumulated squared distance (gaussian) --
// FORM 0: c2*exp(e)   1: exp(e)*(c3*d2 - c2)   2: exp(e)*(c4*d2^2 - c3*d2 + c2)
// with the reference's underflow clamp  e < MIN -> 0  (gaussian_c.pyx:31-34)
template <typename T, int FORM>
__device__ __forceinline__ T gaussian_entry(T d2, T c1, T c2, T c3, T c4)
{
    const T e = c1 * d2;
    T v;
    if (FORM == 0)      v = c2 * dev_exp<T>(e);
    else if (FORM == 1) v = dev_exp<T>(e) * (c3 * d2 - c2);
    else                v = dev_exp<T>(e) * (c4 * (d2 * d2) - c3 * d2 + c2);
    return (e < (T)GPX_MIN_LOG) ? (T)0 : v;
}

// periodic members for d == 1 (periodic_c.pyx), dd = x1[i] - x2[j]
template <typename T>
__device__ __forceinline__ T periodic_entry(int member, T dd, T h, T w, T p)
{
    const T h2 = h * h, w2 = w * w, p2 = p * p;
    const T arg = (T)0.5 * dd / p;
    const T sn = sin(arg), cs = cos(arg);
    const T ex = dev_exp<T>((T)-2.0 * (sn * sn) / w2);
    const T w3 = w2 * w, w4 = w2 * w2, p4 = p2 * p2;
    switch (member) {
    case GPX_K:        return h2 * ex;                                                    // :30
    case GPX_DK_DH:    return (T)2.0 * h * ex;                                            // :65
    case GPX_DK_DW:    return (T)4.0 * h2 * ex * (sn * sn) / w3;                          // :80
    case GPX_DK_DP:    return (T)2.0 * dd * h2 * ex * sn * cs / (p2 * w2);                // :96
    case GPX_D2K_DHDH: return (T)2.0 * ex;                                                // :111
    case GPX_D2K_DHDW: return (T)8.0 * h * ex * (sn * sn) / w3;                           // :126
    case GPX_D2K_DHDP: return (T)4.0 * dd * h * ex * sn * cs / (p2 * w2);                 // :142
    case GPX_D2K_DWDW: return (T)-12.0 * h2 * ex * (sn * sn) / w4                         // :172
                              + (T)16.0 * h2 * ex * (sn * sn) * (sn * sn) / (w4 * w2);
    case GPX_D2K_DWDP: return (T)-4.0 * dd * h2 * ex * sn * cs / (p2 * w3)                // :188
                              + (T)8.0 * dd * h2 * ex * (sn * sn * sn) * cs / (p2 * w3 * w2);
    default:           return (dd * dd) * h2 * ex * (sn * sn) / (p4 * w2)                 // :235
                              - (dd * dd) * h2 * ex * (cs * cs) / (p4 * w2)
                              + (T)4.0 * (dd * dd) * h2 * ex * (sn * sn) * (cs * cs) / (p4 * w4)
                              - (T)4.0 * dd * h2 * ex * sn * cs / (p2 * p * w2);
    }
}

// one dimension's term of a pair, added to r: the squared difference (gaussian) or sin^2 of the half angle (periodic, period per)
template <typename T, int KIND>
__device__ __forceinline__ T pair_term(T a, T b, T per, T r)
{
    if (KIND == GPX_KERNEL_GAUSSIAN) {
        const T t = a - b;
        return fma(t, t, r);
    }
    const T sn = sin((T)0.5 * (a - b) / per);
    return fma(sn, sn, r);
}

// periodic K for any d from r = sum_k sin^2((a_k - b_k) / (2 p))
template <typename T>
__device__ __forceinline__ T periodic_k(T r, T h, T w) { return (h * h) * dev_exp<T>((T)-2.0 * r / (w * w)); }

// 256 threads stage `count` elements of contiguous points (g[idx] = coordinate idx % d of point idx / d) transposed into
// dst[k * pitch + c], zero from element lim on.  Coalesced: consecutive threads -> consecutive elements.  (c0, k0) = (tid / d,
// tid % d) is the thread's first element and idx += 256 <=> (c, k) += (qd, rd) with carry, qd = 256 / d, rd = 256 % d: the
// caller makes the four ONCE, outside its chunk loop (two integer divisions).
// A macro, not a function: this is the one piece whose text the compiler schedules differently once it arrives by inlining --
// one instruction more in the loop and another register assignment in every kernel that stages, the mean 2.9 % slower at
// d = 32 (DESIGN "Streamed reductions") -- and as a macro every user compiles to the instruction stream it had.
#define GPX_STAGE_POINTS_TRANSPOSED(dst, pitch, g, count, lim, d, tid, qd, rd, c0, k0)                  \
    do {                                                                                                \
        int c = (c0), k = (k0);                                                                         \
        for (int idx = (tid); idx < (count); idx += 256) {                                              \
            (dst)[(size_t)k * (pitch) + c] = (idx < (lim)) ? (g)[idx] : (T)0;                           \
            c += (qd); k += (rd);                                                                       \
            if (k >= (d)) { k -= (d); ++c; }                                                            \
        }                                                                                               \
    } while (0)

// The fixed-order sum over a workgroup of four waves: the 64 lanes by shuffles, lane 0 into the wave's slot red[wave][q];
// after the caller's barrier block_sum_final adds the four slots in wave order.  No atomics: bitwise repeatable.
template <int N>
__device__ __forceinline__ void block_sum_fixed(const double (&acc)[N], double (*red)[N], int tid)
{
#pragma unroll
    for (int q = 0; q < N; ++q) {
        double v = acc[q];
        for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
        if ((tid & 63) == 0) red[tid >> 6][q] = v;
    }
}
template <int N>
__device__ __forceinline__ double block_sum_final(const double (*red)[N], int q) { return ((red[0][q] + red[1][q]) + red[2][q]) + red[3][q]; }

// tile t of a lower triangle walked row by row: (tr, tc) with t = tr (tr + 1) / 2 + tc, tc <= tr
__device__ __forceinline__ void tri_tile(int64_t t, int64_t *tr_out, int64_t *tc_out)
{
    int64_t tr = (int64_t)((sqrt(8.0 * (double)t + 1.0) - 1.0) * 0.5);
    while ((tr + 1) * (tr + 2) / 2 <= t) ++tr;
    while (tr * (tr + 1) / 2 > t) --tr;
    *tr_out = tr;
    *tc_out = t - tr * (tr + 1) / 2;
}

}  // namespace gpx
