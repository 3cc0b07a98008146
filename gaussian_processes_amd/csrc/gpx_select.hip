// gpx_select.hip -- greedy conditional-variance selection of inducing points (Burt, Rasmussen and van der Wilk 2020): a
// pivoted partial Cholesky of K(x, x) that never forms K.  gpx_sgp_select.
//
//   dres[i] = k(x_i, x_i)                                   the residual diagonal, f64
//   step m:  p = the unpicked index with the largest dres (ties: the SMALLEST index; step 0: `first` when given)
//            stop when dres[p] <= tol
//            R[m, i] = (k(x_p, x_i) - sum_{j < m} R[j, p] R[j, i]) / sqrt(dres[p])      j ascending, the sum in f64
//            dres[i] -= R[m, i]^2       (R[m, i] as stored: rounded to the dtype);  p is picked, its residual counts as 0
//            trace[m + 1] = sum_{i unpicked} dres[i]
//
// The hot path is step 3: a tall matrix-vector product over every row of R stored so far, m * n * sizeof(T) bytes read per
// step and nothing to reuse -- bound by memory bandwidth.  Two kernels per step, enqueued for ALL steps on one stream with no
// host round trip in between:
//   select_pick_kernel   one workgroup: folds the per-workgroup partials (max, its smallest index, sum) the step before left,
//                        in a fixed order; writes trace[m], the pick and its pivot; gathers the m coefficients R[j, p] into
//                        one contiguous f64 vector; raises the device-side `done` word when the stop rule fires
//   select_step_kernel   one thread per Vec<T>::N consecutive columns: k(x_p, x_i), the product with 16-byte loads of
//                        R[j, i..] (eight rows in flight per lane), the new row, dres, the workgroup's partial triple
// No atomics, no flags polled between workgroups, no resident launch: stream order is the only dependency, and after an early
// stop the remaining launches return at once.  The number of workgroups is a function of n alone and every reduction has a
// fixed order, so index, pivot, trace and R repeat bit for bit.
//
// The coefficients are the same for every lane of a wave: `coef` is a const __restrict__ kernel argument read with a
// wave-uniform index, which the compiler turns into scalar loads (eight doubles per s_load in the unrolled loop) -- the route
// the kernel-matrix build found faster than LDS broadcasts for its row points.
//
// Layout in HBM (dtype T, ldr = round_up(n, 128)): ONE block, carved by sel_layout (gpx_mem.h's Carve, each sub-block on 128
// bytes), whose total is also what the call tests against the free memory:
//   x (n, d)  [ARD: scaled in place] | R  m_max x ldr | dres  n doubles | picked  n bytes
//   | the partials: nwg doubles | nwg int64 | nwg doubles | index | pivot | trace | coef | the state word block
//
// Two callers, ONE launch sequence (select_run): gpx_sgp_select, which uploads x and downloads the results, and
// select_on_device (gpx_gp_internal.h) for a handle whose points are resident and which keeps R on the device -- the iterative
// GP's preconditioner (gpx_cg.hip); its block is the same layout without x.
#include "gpx_small.h"
#include <algorithm>
#include <cmath>
#include <vector>

#include "gpx_gp_internal.h"
#include "gpx_kernels_dev.h"

namespace gpx {

struct SelState {
    int64_t p;        // the pick of the current step
    double dp;        // its residual: the pivot
    int64_t count;    // points picked so far
    int done;         // the stop rule has fired: every later launch returns at once
};

// k(a, b) as gpx_d_kmat stores it (member GPX_K, clamp included): c = make_kparams' constants
template <typename T, int KIND>
__device__ __forceinline__ T select_entry(const T *a, const T *b, int d, T c0, T c1, T c2)
{
    T r = (T)0;
#pragma unroll 4
    for (int k = 0; k < d; ++k) r = pair_term<T, KIND>(a[k], b[k], c2, r);
    if (KIND == GPX_KERNEL_GAUSSIAN) return gaussian_entry<T, 0>(r, c0, c1, (T)0, (T)0);
    return periodic_k<T>(r, c0, c1);
}

// (mx, ix) <- the better of itself and (bm, bi): the larger residual, on a tie the smaller index; ix < 0: no candidate yet
__device__ __forceinline__ void select_take(double &mx, int64_t &ix, double bm, int64_t bi)
{
    if (bi >= 0 && (ix < 0 || bm > mx || (bm == mx && bi < ix))) { mx = bm; ix = bi; }
}

// the triple of a 256-thread workgroup, in a fixed order (a binary tree over the thread index); valid in thread 0
__device__ __forceinline__ void select_block_triple(double &mx, int64_t &ix, double &sm, double *smx, int64_t *six, double *ssm)
{
    const int tid = threadIdx.x;
    smx[tid] = mx; six[tid] = ix; ssm[tid] = sm;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (tid < s) {
            select_take(smx[tid], six[tid], smx[tid + s], six[tid + s]);
            ssm[tid] += ssm[tid + s];
        }
        __syncthreads();
    }
    mx = smx[0]; ix = six[0]; sm = ssm[0];
}

// dres[i] = k(x_i, x_i), nobody picked, and the partials step 0 picks from
template <typename T, int KIND>
__global__ __launch_bounds__(256) void select_init_kernel(const T *__restrict__ x, int64_t n, int d, T c0, T c1, T c2,
                                                          double *__restrict__ dres, unsigned char *__restrict__ picked,
                                                          double *__restrict__ pmx, int64_t *__restrict__ pix, double *__restrict__ psm)
{
    constexpr int VEC = Vec<T>::N;
    __shared__ double smx[256], ssm[256];
    __shared__ int64_t six[256];
    const int64_t i0 = ((int64_t)blockIdx.x * 256 + threadIdx.x) * VEC;
    double mx = -INFINITY, sm = 0.0;
    int64_t ix = -1;
    for (int e = 0; e < VEC; ++e) {
        const int64_t i = i0 + e;
        if (i >= n) break;
        const double v = (double)select_entry<T, KIND>(x + i * d, x + i * d, d, c0, c1, c2);
        dres[i] = v;
        picked[i] = 0;
        select_take(mx, ix, v, i);
        sm += v;
    }
    select_block_triple(mx, ix, sm, smx, six, ssm);
    if (threadIdx.x == 0) { pmx[blockIdx.x] = mx; pix[blockIdx.x] = ix; psm[blockIdx.x] = sm; }
}

// Step m's pick from the partials of the step before (m == m_max: only the last trace entry).  One workgroup.
template <typename T>
__global__ __launch_bounds__(256) void select_pick_kernel(int64_t m, int64_t m_max, int64_t nwg, const double *__restrict__ pmx,
                                                          const int64_t *__restrict__ pix, const double *__restrict__ psm, double tol,
                                                          int64_t first, const T *__restrict__ R, int64_t ldr,
                                                          const double *__restrict__ dres, unsigned char *__restrict__ picked,
                                                          SelState *st, int64_t *__restrict__ index, double *__restrict__ pivot,
                                                          double *__restrict__ trace, double *__restrict__ coef)
{
    __shared__ double smx[256], ssm[256];
    __shared__ int64_t six[256];
    __shared__ int64_t sp;
    if (st->done) return;
    const int tid = threadIdx.x;
    double mx = -INFINITY, sm = 0.0;
    int64_t ix = -1;
    for (int64_t w = tid; w < nwg; w += 256) {
        select_take(mx, ix, pmx[w], pix[w]);
        sm += psm[w];
    }
    select_block_triple(mx, ix, sm, smx, six, ssm);      // (every thread has read st->done by now)
    if (tid == 0) {
        trace[m] = sm;
        int64_t p = -1;
        if (m < m_max) {
            p = (m == 0 && first >= 0) ? first : ix;
            const double dp = p >= 0 ? dres[p] : 0.0;
            if (p < 0 || !(dp > tol)) {
                st->done = 1;
                st->count = m;
                p = -1;
            } else {
                st->p = p; st->dp = dp; st->count = m + 1;
                index[m] = p; pivot[m] = dp;
                picked[p] = 1;
            }
        }
        sp = p;
    }
    __syncthreads();
    const int64_t p = sp;
    if (p < 0) return;
    for (int64_t j = tid; j < m; j += 256) coef[j] = (double)R[j * ldr + p];
}

// Row m of R, the residuals behind it and the workgroup's partial triple.  Rprev: rows [0, m), read; Rrow: row m, written.
template <typename T, int KIND>
__global__ __launch_bounds__(256) void select_step_kernel(const T *__restrict__ x, int64_t n, int d, T c0, T c1, T c2, int64_t m,
                                                          const T *__restrict__ Rprev, T *__restrict__ Rrow, int64_t ldr,
                                                          const double *__restrict__ coef, double *__restrict__ dres,
                                                          const unsigned char *__restrict__ picked, const SelState *__restrict__ st,
                                                          double *__restrict__ pmx, int64_t *__restrict__ pix, double *__restrict__ psm)
{
    constexpr int VEC = Vec<T>::N;
    constexpr int UNROLL = 8;
    typedef typename Vec<T>::type VT;
    __shared__ double smx[256], ssm[256];
    __shared__ int64_t six[256];
    if (st->done) return;
    const int64_t p = st->p;
    const double root = sqrt(st->dp);
    const int64_t i0 = ((int64_t)blockIdx.x * 256 + threadIdx.x) * VEC;
    double mx = -INFINITY, sm = 0.0;
    int64_t ix = -1;
    if (i0 < n) {
        const int nv = n - i0 < VEC ? (int)(n - i0) : VEC;           // columns >= n are never read or written
        double acc[VEC];
#pragma unroll
        for (int e = 0; e < VEC; ++e) acc[e] = 0.0;
        const T *__restrict__ rc = Rprev + i0;
        if (nv == VEC) {
            int64_t j = 0;
            for (; j + UNROLL <= m; j += UNROLL) {
                VT v[UNROLL];
#pragma unroll
                for (int u = 0; u < UNROLL; ++u) v[u] = *reinterpret_cast<const VT *>(rc + (j + u) * ldr);
#pragma unroll
                for (int u = 0; u < UNROLL; ++u) {
                    const double c = coef[j + u];
                    const T *pv = reinterpret_cast<const T *>(&v[u]);
#pragma unroll
                    for (int e = 0; e < VEC; ++e) acc[e] = fma(c, (double)pv[e], acc[e]);
                }
            }
            for (; j < m; ++j) {
                const VT v = *reinterpret_cast<const VT *>(rc + j * ldr);
                const double c = coef[j];
                const T *pv = reinterpret_cast<const T *>(&v);
#pragma unroll
                for (int e = 0; e < VEC; ++e) acc[e] = fma(c, (double)pv[e], acc[e]);
            }
        } else {
            for (int64_t j = 0; j < m; ++j) {
                const double c = coef[j];
                for (int e = 0; e < nv; ++e) acc[e] = fma(c, (double)rc[j * ldr + e], acc[e]);
            }
        }
        const T *xp = x + p * d;                                     // wave-uniform: scalar loads
        T row[VEC];
#pragma unroll
        for (int e = 0; e < VEC; ++e) {
            row[e] = (T)0;
            if (e >= nv) continue;
            const int64_t i = i0 + e;
            const double kv = (double)select_entry<T, KIND>(xp, x + i * d, d, c0, c1, c2);
            const T r = (T)((kv - acc[e]) / root);
            row[e] = r;
            const double dv = dres[i] - (double)r * (double)r;
            dres[i] = dv;
            if (!picked[i]) {
                select_take(mx, ix, dv, i);
                sm += dv;
            }
        }
        if (nv == VEC) {
            VT pk;
            memcpy(&pk, row, sizeof(pk));
            *reinterpret_cast<VT *>(Rrow + i0) = pk;
        } else {
            for (int e = 0; e < nv; ++e) Rrow[i0 + e] = row[e];
        }
    }
    select_block_triple(mx, ix, sm, smx, six, ssm);
    if (threadIdx.x == 0) { pmx[blockIdx.x] = mx; pix[blockIdx.x] = ix; psm[blockIdx.x] = sm; }
}

constexpr int64_t SEL_LD_ALIGN = 128;

// Everything a selection holds on the device (the fp32 upload's f64 staging aside), ONE block: declared here, once.  The
// allocation and the test against the free memory take `total`, SelBufs its pointers from the offsets.
struct SelLayout { size_t x, R, dres, picked, pmx, pix, psm, index, pivot, trace, coef, st, total; };
constexpr SelLayout sel_layout(int64_t n, int d, int64_t m_max, size_t es)
{
    const size_t nwg = (size_t)cdiv(n, 256 * (int64_t)(16 / es)), N = (size_t)n, M = (size_t)m_max;
    Carve k;
    const size_t x = k.take(N * d * es), R = k.take(M * (size_t)round_up(n, SEL_LD_ALIGN) * es), dres = k.take(N * 8), picked = k.take(N);
    const size_t pmx = k.take(nwg * 8), pix = k.take(nwg * 8), psm = k.take(nwg * 8);
    const size_t index = k.take(M * 8), pivot = k.take(M * 8), trace = k.take((M + 1) * 8), coef = k.take(M * 8), st = k.take(sizeof(SelState));
    return {x, R, dres, picked, pmx, pix, psm, index, pivot, trace, coef, st, k.total()};
}
// the padding of the twelve sub-blocks: what the layout adds to the sum the twelve separate buffers of this file once made
constexpr size_t sel_padding(int64_t n, int d, int64_t m_max, size_t es)
{
    return sel_layout(n, d, m_max, es).total - ((size_t)m_max * round_up(n, SEL_LD_ALIGN) * es + (size_t)n * d * es + (size_t)n * 9 +
                                                (size_t)cdiv(n, 256 * (int64_t)(16 / es)) * 24 + (size_t)m_max * 32 + 8 + sizeof(SelState));
}
static_assert(sel_padding(1000, 3, 64, 8) <= 12 * 128 && sel_padding(1000, 3, 64, 4) <= 12 * 128, "the selection's layout (unsigned: never less)");

// the pointers of a block laid out so
struct SelBufs {
    void *x, *R;
    double *dres, *pmx, *psm, *pivot, *trace, *coef;
    int64_t *pix, *index;
    unsigned char *picked;
    SelState *st;
    SelBufs(char *p, const SelLayout &l)
        : x(p + l.x), R(p + l.R), dres((double *)(p + l.dres)), pmx((double *)(p + l.pmx)), psm((double *)(p + l.psm)),
          pivot((double *)(p + l.pivot)), trace((double *)(p + l.trace)), coef((double *)(p + l.coef)), pix((int64_t *)(p + l.pix)),
          index((int64_t *)(p + l.index)), picked((unsigned char *)(p + l.picked)), st((SelState *)(p + l.st)) {}
};

// every launch of a selection, enqueued on `st`: init, (pick, step) x m_max, the last trace entry
template <typename T, int KIND>
static int select_enqueue(const SelBufs &b, int64_t n, int d, const KParams &kp, int64_t m_max, double tol, int64_t first, int64_t ldr,
                          hipStream_t st)
{
    const int64_t nwg = cdiv(n, 256 * (int64_t)Vec<T>::N);
    const dim3 grid((unsigned)nwg), block(256);
    const T c0 = (T)kp.c[0], c1 = (T)kp.c[1], c2 = (T)kp.c[2];
    const T *x = (const T *)b.x;
    T *R = (T *)b.R;
    hipLaunchKernelGGL((select_init_kernel<T, KIND>), grid, block, 0, st, x, n, d, c0, c1, c2, b.dres, b.picked, b.pmx, b.pix, b.psm);
    GPX_LAUNCH_CHECK();
    for (int64_t m = 0; m <= m_max; ++m) {
        hipLaunchKernelGGL((select_pick_kernel<T>), dim3(1), block, 0, st, m, m_max, nwg, b.pmx, b.pix, b.psm, tol, first, R, ldr, b.dres,
                           b.picked, b.st, b.index, b.pivot, b.trace, b.coef);
        GPX_LAUNCH_CHECK();
        if (m == m_max) break;
        hipLaunchKernelGGL((select_step_kernel<T, KIND>), grid, block, 0, st, x, n, d, c0, c1, c2, m, R, R + m * ldr, ldr, b.coef, b.dres,
                           b.picked, b.st, b.pmx, b.pix, b.psm);
        GPX_LAUNCH_CHECK();
    }
    return GPX_OK;
}

// One selection on a block laid out by sel_layout whose points (b.x) are in place: the state word cleared, every launch, one
// profile record around them (its work -- the bytes of R read and written -- is known at the end), the count on the host and a
// route hit per pick.  Synchronises `st`.
static int select_run(int dtype, bool periodic, const SelBufs &b, int64_t n, int d, const KParams &kp, int64_t m_max, double tol,
                      int64_t first, int64_t ldr, hipStream_t st, int64_t *count)
{
    GPX_HIP(hipMemsetAsync(b.st, 0, sizeof(SelState), st));
    SelState hs;
    {
        RoctxRange range(prof_class_name(PC_SELECT));
        const int rec = (g_prof_on && g_prof_mute == 0) ? prof_begin(PC_SELECT, 0.0, st) : -1;
        const int rc = by_dtype(dtype, [&](auto t) {
            using T = decltype(t);
            return periodic ? select_enqueue<T, GPX_KERNEL_PERIODIC>(b, n, d, kp, m_max, tol, first, ldr, st)
                            : select_enqueue<T, GPX_KERNEL_GAUSSIAN>(b, n, d, kp, m_max, tol, first, ldr, st);
        });
        if (rec >= 0) prof_end(rec, st);
        GPX_TRY(rc);
        GPX_HIP(hipMemcpyAsync(&hs, b.st, sizeof(SelState), hipMemcpyDeviceToHost, st));
        GPX_HIP(hipStreamSynchronize(st));
        if (rec >= 0) prof_set_work(rec, (double)esize(dtype) * (double)n * (double)hs.count * (double)(hs.count + 1) / 2.0);
    }
    const int64_t cnt = hs.count;
    if (cnt < 0 || cnt > m_max) { set_error("gpx_sgp_select: the device reported %lld picks of at most %lld", (long long)cnt, (long long)m_max); return GPX_ERR_INTERNAL; }
    for (int64_t i = 0; i < cnt; ++i) route_hit(RT_SELECT_STEP);
    *count = cnt;
    return GPX_OK;
}

// The device-pointer entry (gpx_gp_internal.h): the same launches on points the caller keeps in HBM.  The block is sel_layout's
// with no room for x; R stays where it is, for the caller.
size_t select_block_bytes(int dtype, int64_t n, int64_t m_max) { return sel_layout(n, 0, m_max, esize(dtype)).total; }

int select_on_device(int dtype, int kernel, const void *x_dev, int64_t n, int d, const double *params, int64_t m_max, double tol, void *block,
                     hipStream_t st, int64_t *count, void **R, int64_t *ldr)
{
    KParams kp;
    GPX_TRY(make_kparams(kernel, GPX_K, params, 0.0, &kp));
    SelBufs b((char *)block, sel_layout(n, 0, m_max, esize(dtype)));
    b.x = const_cast<void *>(x_dev);
    *ldr = round_up(n, SEL_LD_ALIGN);
    *R = b.R;
    return select_run(dtype, kernel == GPX_KERNEL_PERIODIC, b, n, d, kp, m_max, tol, -1, *ldr, st, count);
}

// a stream of the call's own, gone with it
struct SelStream {
    hipStream_t st = nullptr;
    int create() { GPX_HIP(hipStreamCreateWithFlags(&st, hipStreamNonBlocking)); return GPX_OK; }
    ~SelStream()
    {
        if (!st) return;
        (void)hipStreamSynchronize(st);
        stream_epoch_bump();
        (void)hipStreamDestroy(st);
    }
};

constexpr size_t SEL_DOWNLOAD_BYTES = (size_t)256 << 20;       // the f64 staging copy of R's rows on their way to the host

static int sgp_select(int dtype, int kernel, const double *x, int64_t n, int d, const double *params, int64_t m_max, double tol,
                      int64_t first, int64_t *index, double *pivot, double *trace, double *R, int64_t *count)
{
    const size_t es = esize(dtype);
    const int64_t ldr = round_up(n, SEL_LD_ALIGN);
    const bool ard = kernel == GPX_KERNEL_GAUSSIAN_ARD;
    double iso[2];
    const double *vparams = params;
    if (ard) { ard_iso(params, d, iso); vparams = iso; }
    KParams kp;
    GPX_TRY(make_kparams(ard ? GPX_KERNEL_GAUSSIAN : kernel, GPX_K, vparams, 0.0, &kp));

    // everything the call holds on the device, against the free memory, before anything is allocated
    const SelLayout lay = sel_layout(n, d, m_max, es);
    const size_t r_bytes = (size_t)m_max * ldr * es, need = lay.total + (dtype == GPX_F32 ? (size_t)n * d * 8 : 0);
    size_t freeb = 0, totalb = 0;
    GPX_HIP(hipMemGetInfo(&freeb, &totalb));
    if (need > freeb) {
        set_error("gpx_sgp_select: needs %zu bytes of device memory (R, %lld x %lld: %zu), %zu are free", need, (long long)m_max,
                  (long long)ldr, r_bytes, freeb);
        return GPX_ERR_NOMEM;
    }
    SelStream own;
    GPX_TRY(own.create());
    hipStream_t st = own.st;
    StreamTurn turn(st);
    DevBuf dev;
    GPX_TRY(dev.alloc(lay.total));
    const SelBufs b((char *)dev.p, lay);
    GPX_TRY(upload_f64(dtype, b.x, n * d, x, n * d, 1, n * d, st));
    if (ard) GPX_TRY(scale_points(dtype, b.x, n, d, params + 1, b.x, st));
    std::vector<int64_t> hindex((size_t)m_max);
    std::vector<double> hpivot((size_t)m_max), htrace((size_t)m_max + 1);
    int64_t cnt = 0;
    GPX_TRY(select_run(dtype, kernel == GPX_KERNEL_PERIODIC, b, n, d, kp, m_max, tol, first, ldr, st, &cnt));
    GPX_HIP(hipMemcpyAsync(hindex.data(), b.index, (size_t)m_max * 8, hipMemcpyDeviceToHost, st));
    GPX_HIP(hipMemcpyAsync(hpivot.data(), b.pivot, (size_t)m_max * 8, hipMemcpyDeviceToHost, st));
    GPX_HIP(hipMemcpyAsync(htrace.data(), b.trace, (size_t)(m_max + 1) * 8, hipMemcpyDeviceToHost, st));
    GPX_HIP(hipStreamSynchronize(st));
    if (R && cnt > 0) {
        const int64_t rows_per = std::max<int64_t>(1, (int64_t)(SEL_DOWNLOAD_BYTES / ((size_t)n * 8)));
        for (int64_t r0 = 0; r0 < cnt; r0 += rows_per) {
            const int64_t rows = std::min(rows_per, cnt - r0);
            GPX_TRY(download_f64(dtype, R + r0 * n, n, (const char *)b.R + (size_t)r0 * ldr * es, ldr, rows, n, 0, st));
        }
    }
    std::copy(hindex.begin(), hindex.begin() + cnt, index);
    std::copy(hpivot.begin(), hpivot.begin() + cnt, pivot);
    std::copy(htrace.begin(), htrace.begin() + cnt + 1, trace);
    *count = cnt;
    return GPX_OK;
}

}  // namespace gpx

using namespace gpx;

extern "C" int gpx_sgp_select(int dtype, int kernel, const double *x, int64_t n, int d, const double *params, int64_t m_max, double tol,
                              int64_t first, int64_t *index, double *pivot, double *trace, double *R, int64_t *count)
{
    gpx::tune_refresh();
    GPX_ARG(dtype == GPX_F64 || dtype == GPX_F32, "dtype must be GPX_F64 or GPX_F32");
    GPX_ARG(kernel == GPX_KERNEL_GAUSSIAN || kernel == GPX_KERNEL_PERIODIC || kernel == GPX_KERNEL_GAUSSIAN_ARD, "unknown kernel family");
    GPX_ARG(x && params && index && pivot && trace && count, "NULL argument");
    GPX_ARG(n >= 1, "need n >= 1");
    GPX_ARG(d >= 1, "need d >= 1");
    GPX_ARG(kernel != GPX_KERNEL_GAUSSIAN_ARD || d <= GPX_ARD_MAX_D, "the ARD family needs d <= GPX_ARD_MAX_D");
    // (the kernel-matrix build stages 65 sixteen-byte vectors per dimension and refuses what does not fit its LDS limit)
    GPX_ARG((size_t)d * 65 * 16 <= (size_t)LDS_CHUNK_MAX, "d is beyond what gpx_d_kmat builds");
    GPX_ARG(m_max >= 1 && m_max <= n, "m_max must lie in 1 .. n");
    GPX_ARG(tol >= 0.0 && tol <= 1.79769313486231570e308, "tol must be >= 0 and finite");
    GPX_ARG(first < n, "first must be < n (negative: none)");
    for (int i = 0; i < nparams_of(kernel, d); ++i) GPX_ARG(std::isfinite(params[i]), "array must not contain infs or NaNs (kernel parameters)");
    GPX_TRY(ensure_device());
    gpx::RoctxRange api_range__(__func__);
    return sgp_select(dtype, kernel, x, n, d, params, m_max, tol, first, index, pivot, trace, R, count);
}
