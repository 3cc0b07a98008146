// gpx_sample.hip -- normal numbers on the device (gpx_d_randn) and the step from a covariance to joint samples
// (gpx_d_mvn_sample); the handle's gpx_gp_sample* (gpx_gp.hip) builds the posterior covariance and calls the latter.
//
// The generator is counter based: element e of the sequence (seed, stream) is a pure function z(seed, stream, e),
//   q = e >> 1
//   (w0, w1, w2, w3) = Philox4x32-10(counter = (lo32 q, hi32 q, lo32 stream, hi32 stream), key = (lo32 seed, hi32 seed))
//   u1 = (2 (((w0 << 32) | w1) >> 12) + 1) 2^-53,  u2 likewise from (w2, w3)       (odd 53-bit integers: exact, in (0, 1))
//   r  = sqrt(-2 ln u1);   z = r cos(2 pi u2) for even e,  r sin(2 pi u2) for odd e    (Box-Muller; |z| <= 8.572)
// with the Philox constants and round of Random123 (Salmon et al., SC11).  Nothing else enters: not the grid, not the pitch, not
// the way a caller cuts a matrix into calls -- element (i, j) of a rows x cols call is e = offset + i cols + j.  All of it is
// fp64 for both dtypes; the one rounding to fp32 is the store.  tests/_sample_helpers.py restates it in numpy.
#include "gpx_small.h"
#include <algorithm>

namespace gpx {

__device__ __forceinline__ void philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1, uint32_t w[4])
{
#pragma unroll
    for (int rnd = 0; rnd < 10; ++rnd) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
        c1 = (uint32_t)p1; c3 = (uint32_t)p0; c0 = n0; c2 = n2;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    w[0] = c0; w[1] = c1; w[2] = c2; w[3] = c3;
}

__device__ __forceinline__ double philox_unit(uint32_t hi, uint32_t lo)
{
    const uint64_t x = ((uint64_t)hi << 32) | lo;
    return (double)(2 * (x >> 12) + 1) * 0x1p-53;
}

// One thread per Philox call = per pair (2q, 2q + 1) of the sequence; thread p of the launch owns q = q0 + p, whose
// elements are t0 = 2 p - odd and t0 + 1 of the call (odd: the call begins at the second half of pair q0).  Either may
// fall outside [0, total): the first of the first pair, the second of the last.
template <typename T>
__global__ __launch_bounds__(256) void randn_kernel(T *__restrict__ out, int64_t cols, int64_t ld, int64_t total, uint64_t q0, int odd,
                                                    int64_t pairs, uint64_t seed, uint64_t stream)
{
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= pairs) return;
    const uint64_t q = q0 + (uint64_t)p;
    uint32_t w[4];
    philox4x32_10((uint32_t)q, (uint32_t)(q >> 32), (uint32_t)stream, (uint32_t)(stream >> 32), (uint32_t)seed, (uint32_t)(seed >> 32), w);
    const double u1 = philox_unit(w[0], w[1]), u2 = philox_unit(w[2], w[3]);
    const double r = sqrt(-2.0 * log(u1));
    double sn, cs;
    sincospi(2.0 * u2, &sn, &cs);                    // (2 u2 is exact: the angle is never rounded)
    const int64_t t0 = 2 * p - odd, t1 = t0 + 1;
    if (t0 >= 0 && t0 < total) out[(t0 / cols) * ld + t0 % cols] = (T)(r * cs);
    if (t1 < total) out[(t1 / cols) * ld + t1 % cols] = (T)(r * sn);
}

int randn(int dtype, void *out, int64_t rows, int64_t cols, int64_t ld, uint64_t seed, uint64_t stream, uint64_t offset, hipStream_t st)
{
    if (rows <= 0 || cols <= 0) return GPX_OK;
    const int64_t total = rows * cols;
    const uint64_t q0 = offset >> 1, q1 = (offset + (uint64_t)total - 1) >> 1;
    const int64_t pairs = (int64_t)(q1 - q0) + 1;
    const int64_t blocks = cdiv(pairs, 256);
    if (blocks > 0x7fffffff) { set_error("randn: %lld elements are more than one launch covers", (long long)total); return GPX_ERR_ARG; }
    ProfScope prof(PC_RANDN, (double)total * (double)esize(dtype), st);
    const dim3 grid((unsigned)blocks), block(256);
    return by_dtype(dtype, [&](auto t) {
        using T = decltype(t);
        hipLaunchKernelGGL((randn_kernel<T>), grid, block, 0, st, (T *)out, cols, ld, total, q0, (int)(offset & 1), pairs, seed, stream);
        GPX_LAUNCH_CHECK();
        return GPX_OK;
    });
}

// ---- from a covariance to samples ---------------------------------------------------------------------------------------
template <typename T>
static int mvn_prepare_t(T *C, int64_t m, int64_t ldc, double jitter, hipStream_t st)
{
    const T v = (T)jitter;
    return map_vec(m, st, [=] __device__(int64_t i) { C[i * ldc + i] += v; });
}

// out[r, c] = mean[c] (null: 0) for r < rows, c < cols
template <typename T>
static int fill_rows_t(T *out, int64_t ldo, const T *mean, int64_t rows, int64_t cols, hipStream_t st)
{
    return map_rows(rows, cols, st, [=] __device__(int64_t r, int64_t c) { out[r * ldo + c] = mean ? mean[c] : (T)0; });
}

// out = 1 mean^T + Z Lc^T:  C + jitter I -> Lc in place (potrf, tril), Z = randn, then ONE full product against the
// factor with its zero upper triangle.  Half of that product's flops meet zeros: S m^2 of them, against potrf's m^3 / 3 --
// a triangular product would be a kernel of its own for less than the factorisation's rounding of the total.
int mvn_sample(int dtype, void *C, int64_t m, int64_t ldc, const void *mean, double jitter, int64_t S, uint64_t seed, uint64_t stream,
               void *Z, int64_t ldz, void *out, int64_t ldo, int *info_dev, hipStream_t st)
{
    if (m <= 0) { GPX_HIP(hipMemsetAsync(info_dev, 0, sizeof(int), st)); return GPX_OK; }
    GPX_TRY(by_dtype(dtype, [&](auto t) { using T = decltype(t); return mvn_prepare_t<T>((T *)C, m, ldc, jitter, st); }));
    GPX_TRY(potrf(dtype, C, m, ldc, info_dev, st));
    GPX_TRY(tril(dtype, C, m, ldc, st));
    if (S <= 0) return GPX_OK;
    GPX_TRY(randn(dtype, Z, S, m, ldz, seed, stream, 0, st));
    GPX_TRY(by_dtype(dtype, [&](auto t) { using T = decltype(t); return fill_rows_t<T>((T *)out, ldo, (const T *)mean, S, m, st); }));
    return gemm_nt(dtype, S, m, m, Z, ldz, C, ldc, out, ldo, 1.0, GPX_FULL, 0, 0, st);
}

}  // namespace gpx

using namespace gpx;

extern "C" {

int gpx_d_randn(int dtype, void *out, int64_t rows, int64_t cols, int64_t ld, uint64_t seed, uint64_t stream, uint64_t offset,
                void *hipstream)
{
    gpx::tune_refresh();
    GPX_ARG(dtype == GPX_F64 || dtype == GPX_F32, "dtype must be GPX_F64 or GPX_F32");
    GPX_ARG(rows >= 0 && cols >= 0, "negative dimension");
    if (rows == 0 || cols == 0) return GPX_OK;
    GPX_ARG(out, "out is NULL");
    GPX_ARG(ld >= cols, "ld < cols");
    GPX_ARG(rows <= INT64_MAX / cols && rows <= INT64_MAX / ld, "rows * cols overflows");
    GPX_ARG(offset <= UINT64_MAX - (uint64_t)(rows * cols), "offset + rows * cols overflows");
    GPX_TRY(ensure_device());
    return randn(dtype, out, rows, cols, ld, seed, stream, offset, S(hipstream));
}

int gpx_d_mvn_sample(int dtype, void *C, int64_t m, int64_t ldc, const void *mean, double jitter, int64_t Sn, uint64_t seed,
                     uint64_t stream, void *Z, int64_t ldz, void *out, int64_t ldo, int *info_dev, void *hipstream)
{
    gpx::tune_refresh();
    gpx::StreamTurn turn__((hipStream_t)hipstream);     // (this thread's scratch buffers: one stream at a time, gpx_mem.h)
    GPX_ARG(dtype == GPX_F64 || dtype == GPX_F32, "dtype must be GPX_F64 or GPX_F32");
    GPX_ARG(m >= 0 && Sn >= 0, "negative dimension");
    GPX_ARG(info_dev, "info_dev is NULL");
    GPX_ARG(jitter >= 0.0 && jitter <= 1.79769313486231570e308, "jitter must be finite and >= 0");
    GPX_TRY(ensure_device());
    if (m > 0) {
        GPX_ARG(C, "C is NULL");
        GPX_ARG(ldc >= m && ldc % 16 == 0 && ((uintptr_t)C) % 16 == 0, "C must be 16-byte aligned with ldc >= m a multiple of 16 elements");
        if (Sn > 0) {
            GPX_ARG(Z && out && Z != out, "NULL pointer or Z == out");
            GPX_ARG(ldz >= m && ldo >= m, "leading dimension too small");
            GPX_ARG(Sn <= INT64_MAX / ldz && Sn <= INT64_MAX / ldo, "S * ld overflows");
        }
    }
    return mvn_sample(dtype, C, m, ldc, mean, jitter, Sn, seed, stream, Z, ldz, out, ldo, info_dev, S(hipstream));
}

}  // extern "C"
