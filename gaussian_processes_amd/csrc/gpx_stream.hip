// gpx_stream.hip -- the streamed reductions over the training set (gfx950): a few test points against ALL of x, which
// passes through LDS in chunks of 256 points.  The fused posterior mean (stream_mean_kernel: gpx_d_mean, gpx_d_mean_member),
// the fused route of gpx_d_kmat_apply (stream_apply_kernel), the fused input-space gradient (pred_grad_kernel:
// gpx_d_pred_grad) and that gradient for several weight vectors at once (stream_apply_grad_kernel: gpx_d_kmat_apply_grad) --
// four kernels from the same pieces -- with the slice plan, the partial-sum scratch and the sliced launcher they share.  The
// pieces (chunk staging, pair term, entry functions, block sum) are gpx_kernels_dev.h's; DESIGN "Streamed reductions".
#include "gpx_common.h"
#include "gpx_kernels_dev.h"
#include <algorithm>

namespace gpx {

constexpr int MCP = 257;           // padded chunk row

// ---------------------------------------------------------------------------
// The slice plan: enough workgroups to fill the chip -- slices of the training set when the `groups` workgroups that the
// test points (and dimension windows, and vector groups) make are too few.  Slices are whole chunks of 256 points.
// ---------------------------------------------------------------------------
struct SlicePlan { int64_t nslice, slice_len; };
static SlicePlan slice_plan(int64_t groups, int64_t n)
{
    const int64_t want = std::max<int64_t>(1, std::min<int64_t>(cdiv(2048, groups), cdiv(n, 256)));
    const int64_t slice_len = cdiv(cdiv(n, want), 256) * 256;
    return SlicePlan{cdiv(n, slice_len), slice_len};
}

// The slices' partial sums of every launcher below.  A block is this host thread's on one device, and every entry that
// reaches it holds a StreamTurn: the thread's calls use it one after another on ONE stream at a time, so a pass's partial
// sums are consumed by its reduce kernel before the next pass on that stream writes them (mean, pred_grad, the fused
// kmat_apply and kmat_apply_grad never nest: none of them calls another).  The product route of kmat_apply keeps a block of its own
// (gpx_paths.hip): that one is live across a gpx_d_kmat call.
static thread_local ThreadScratch g_partial_scr;

// ---------------------------------------------------------------------------
// Entry evaluators of the two apply kernels: step() adds one dimension of a pair to the lane's distance term, entry() makes the
// kernel value from it -- the distance as kmat_kernel accumulates it, the entry function of kmat_kernel, underflow clamp
// included: the value is the element gpx_d_kmat would store.
// ---------------------------------------------------------------------------
// gaussian member of FORM 0..2 (see gaussian_entry)
template <typename T, int FORM>
struct GaussianEval {
    T c1, c2, c3, c4;
    __device__ __forceinline__ explicit GaussianEval(const KParams &kp) : c1((T)kp.c[0]), c2((T)kp.c[1]), c3((T)kp.c[2]), c4((T)kp.c[3]) {}
    __device__ __forceinline__ T step(T a, T b, T r) const { return pair_term<T, GPX_KERNEL_GAUSSIAN>(a, b, (T)0, r); }
    __device__ __forceinline__ T entry(T r) const { return gaussian_entry<T, FORM>(r, c1, c2, c3, c4); }
};
// periodic K, any d
template <typename T>
struct PeriodicEval {
    T h, w, p;
    __device__ __forceinline__ explicit PeriodicEval(const KParams &kp) : h((T)kp.c[0]), w((T)kp.c[1]), p((T)kp.c[2]) {}
    __device__ __forceinline__ T step(T a, T b, T r) const { return pair_term<T, GPX_KERNEL_PERIODIC>(a, b, p, r); }
    __device__ __forceinline__ T entry(T r) const { return periodic_k<T>(r, h, w); }
};
// any periodic member (kp.member) at d == 1: the term is the signed difference
template <typename T>
struct PeriodicMemberEval {
    T h, w, p; int member;
    __device__ __forceinline__ explicit PeriodicMemberEval(const KParams &kp) : h((T)kp.c[0]), w((T)kp.c[1]), p((T)kp.c[2]), member(kp.member) {}
    __device__ __forceinline__ T step(T a, T b, T) const { return a - b; }
    __device__ __forceinline__ T entry(T r) const { return periodic_entry<T>(member, r, h, w, p); }
};

// ---------------------------------------------------------------------------
// The two apply kernels.  Workgroup (bx, by[, bz]) owns MP test points and the by-th slice of the training set, which streams
// through LDS in chunks of 256 points (one per lane, transposed and padded so both the staging stores and the reads are
// conflict-free).  Sums are kept in f64; lanes are added by shuffles, waves through LDS, and a slice's partial sums go to
// `partial`, which apply_reduce_kernel adds in ascending slice order (deterministic: no atomics, bitwise repeatable).
//   stream_mean_kernel: out[i] = sum_j member(xo[i], x[j]) * alpha[j]  (gp/gp.py:597): 8 points, partial[by][i], or with one
//     slice (partial == null) the sum straight to out[i].
//   stream_apply_kernel: partial[slice][s][i] = sum_{j in slice} k(xo_i, x_j) V[s, j] for the bz-th group of AP_SV weight vectors:
//     per chunk a lane loads its weights V[s0 .. s0 + AP_SV, j] once (coalesced across the lanes, zero beyond S), forms each
//     k(xo_p, x_j) once and adds it into AP_MP x AP_SV f64 sums; only a new group of vectors (gridDim.z) evaluates the kernel again.
//     AP_MP x AP_SV <= 32 f64 accumulators are at most 64 VGPRs of the lane's state; DESIGN "Posterior paths" has the compiler's count.
// Two kernels from the same pieces, not one: at one vector the second carries V's pitch, S and the vector group through the
// chunk loop in a scalar file that is at its cap in both, and measured 2 - 5 % slower than the first (DESIGN "Streamed reductions").
// (`const T a = orow[pp][k]` before the step, not as its argument: the call's argument order moves the load and with it the
// schedule of the staging loop.)
// ---------------------------------------------------------------------------
constexpr int MP = 8;

template <typename T, typename EV>
__global__ __launch_bounds__(256) void stream_mean_kernel(const T *__restrict__ xo, int64_t m, const T *__restrict__ x, int64_t n, int d,
                                                          KParams kp, const T *__restrict__ alpha, int64_t slice_len,
                                                          double *__restrict__ partial, T *__restrict__ out)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    T *sx = reinterpret_cast<T *>(smem_raw);            // [d][MCP] chunk of x, transposed
    __shared__ double red[4][MP];

    const int tid = threadIdx.x;
    const int64_t p0 = (int64_t)blockIdx.x * MP;
    double acc[MP];
#pragma unroll
    for (int pp = 0; pp < MP; ++pp) acc[pp] = 0.0;
    const T *orow[MP];
#pragma unroll
    for (int pp = 0; pp < MP; ++pp) orow[pp] = xo + min(p0 + pp, m - 1) * d;

    const EV ev(kp);
    const int qd = 256 / d, rd = 256 - qd * d;          // idx += 256  <=>  (c, k) += (qd, rd) with carry
    const int cst = tid / d, kst = tid - cst * d;
    const int64_t jbeg = (int64_t)blockIdx.y * slice_len, jend = min(n, jbeg + slice_len);
    for (int64_t j0 = jbeg; j0 < jend; j0 += 256) {
        __syncthreads();
        {
            const int64_t lim = (jend - j0) * d;
            const T *g = x + j0 * d;
            GPX_STAGE_POINTS_TRANSPOSED(sx, MCP, g, 256 * d, lim, d, tid, qd, rd, cst, kst);
        }
        __syncthreads();
        const int64_t j = j0 + tid;
        if (j < jend) {
            const T aj = alpha[j];
            T r[MP];
#pragma unroll
            for (int pp = 0; pp < MP; ++pp) r[pp] = (T)0;
            // (the test points are the same for every lane: SGPR operands through the scalar cache, as in kmat_kernel)
            for (int k = 0; k < d; ++k) {
                const T b = sx[(size_t)k * MCP + tid];
#pragma unroll
                for (int pp = 0; pp < MP; ++pp) { const T a = orow[pp][k]; r[pp] = ev.step(a, b, r[pp]); }
            }
#pragma unroll
            for (int pp = 0; pp < MP; ++pp) acc[pp] += (double)ev.entry(r[pp]) * (double)aj;
        }
    }
    // wave reduction (64 lanes), then across the 4 waves in a fixed order
    block_sum_fixed(acc, red, tid);
    __syncthreads();
    if (tid < MP && p0 + tid < m) {
        const double sum = block_sum_final(red, tid);
        if (partial) partial[(int64_t)blockIdx.y * m + p0 + tid] = sum;
        else out[p0 + tid] = (T)sum;
    }
}

template <typename T, typename EV, int AP_MP, int AP_SV>
__global__ __launch_bounds__(256) void stream_apply_kernel(const T *__restrict__ xo, int64_t m, const T *__restrict__ x, int64_t n, int d,
                                                           KParams kp, const T *__restrict__ V, int64_t ldv, int64_t S,
                                                           int64_t slice_len, double *__restrict__ partial)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    T *sx = reinterpret_cast<T *>(smem_raw);            // [d][MCP] chunk of x, transposed
    __shared__ double red[4][AP_MP * AP_SV];

    const int tid = threadIdx.x;
    const int64_t p0 = (int64_t)blockIdx.x * AP_MP;
    const int64_t s0 = (int64_t)blockIdx.z * AP_SV;
    double acc[AP_MP][AP_SV];
#pragma unroll
    for (int pp = 0; pp < AP_MP; ++pp)
#pragma unroll
        for (int sv = 0; sv < AP_SV; ++sv) acc[pp][sv] = 0.0;
    const T *orow[AP_MP];
#pragma unroll
    for (int pp = 0; pp < AP_MP; ++pp) orow[pp] = xo + min(p0 + pp, m - 1) * d;

    const EV ev(kp);
    const int qd = 256 / d, rd = 256 - qd * d;          // idx += 256  <=>  (c, k) += (qd, rd) with carry
    const int cst = tid / d, kst = tid - cst * d;
    const int64_t jbeg = (int64_t)blockIdx.y * slice_len, jend = min(n, jbeg + slice_len);
    for (int64_t j0 = jbeg; j0 < jend; j0 += 256) {
        __syncthreads();
        {
            const int64_t lim = (jend - j0) * d;
            const T *g = x + j0 * d;
            GPX_STAGE_POINTS_TRANSPOSED(sx, MCP, g, 256 * d, lim, d, tid, qd, rd, cst, kst);
        }
        __syncthreads();
        const int64_t j = j0 + tid;
        if (j < jend) {
            double vj[AP_SV];
#pragma unroll
            for (int sv = 0; sv < AP_SV; ++sv) vj[sv] = (s0 + sv < S) ? (double)V[(s0 + sv) * ldv + j] : 0.0;
            T r[AP_MP];
#pragma unroll
            for (int pp = 0; pp < AP_MP; ++pp) r[pp] = (T)0;
            // (the test points are the same for every lane: SGPR operands through the scalar cache, as in kmat_kernel)
            for (int k = 0; k < d; ++k) {
                const T b = sx[(size_t)k * MCP + tid];
#pragma unroll
                for (int pp = 0; pp < AP_MP; ++pp) { const T a = orow[pp][k]; r[pp] = ev.step(a, b, r[pp]); }
            }
#pragma unroll
            for (int pp = 0; pp < AP_MP; ++pp) {
                const double kd = (double)ev.entry(r[pp]);
#pragma unroll
                for (int sv = 0; sv < AP_SV; ++sv) acc[pp][sv] = fma(kd, vj[sv], acc[pp][sv]);
            }
        }
    }
    // wave reduction (64 lanes), then across the 4 waves in a fixed order
    block_sum_fixed(reinterpret_cast<const double (&)[AP_MP * AP_SV]>(acc), red, tid);      // (acc as [pp * AP_SV + sv])
    __syncthreads();
    if (tid < AP_MP * AP_SV) {
        const int pp = tid / AP_SV, sv = tid - pp * AP_SV;
        if (p0 + pp < m && s0 + sv < S) partial[((int64_t)blockIdx.y * S + s0 + sv) * m + p0 + pp] = block_sum_final(red, tid);
    }
}

// the sum over the slices, in slice order; one rounding to T.  ADD: out[s, i] += sum (kmat_apply), else out[s, i] = sum (the mean)
template <typename T, bool ADD>
__global__ __launch_bounds__(256) void apply_reduce_kernel(const double *__restrict__ partial, int nslice, int64_t S, int64_t m,
                                                           T *__restrict__ out, int64_t ldo)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= m) return;
    for (int64_t s = blockIdx.y; s < S; s += gridDim.y) {
        double sum = 0.0;
        for (int y = 0; y < nslice; ++y) sum += partial[((int64_t)y * S + s) * m + i];
        out[s * ldo + i] = ADD ? (T)((double)out[s * ldo + i] + sum) : (T)sum;
    }
}

// the launch every sliced kernel but pred_grad's shares: the slice plan over `groups` workgroups, the partial sums -- `cols` doubles
// a slice; always == false: only when there is more than one slice --, the LDS limit, and the slices' reduction
template <typename Launch, typename Reduce>
static int launch_sliced_with(int64_t groups, int64_t n, size_t smem, size_t cols, bool always, const void *kernel_fn, Launch launch,
                              Reduce reduce)
{
    const SlicePlan sp = slice_plan(groups, n);
    double *partial = nullptr;
    if (always || sp.nslice > 1) {
        void *scr = nullptr;
        GPX_TRY(g_partial_scr.get((size_t)sp.nslice * cols * sizeof(double), &scr));
        partial = (double *)scr;
    }
    // (set_max_lds sets a kernel's limit ONCE per device, so it gets the constant, never the d-dependent size of one call)
    if (smem > 48 * 1024) GPX_TRY(set_max_lds(kernel_fn, LDS_CHUNK_MAX));
    launch(sp, smem, partial);
    GPX_LAUNCH_CHECK();
    if (partial) {
        reduce(partial, (int)sp.nslice);
        GPX_LAUNCH_CHECK();
    }
    return GPX_OK;
}

// ... for the two apply kernels: the chunk of x in LDS, S x m sums a slice, apply_reduce_kernel
template <typename T, bool ADD, typename Launch>
static int launch_sliced(int64_t groups, int64_t n, int d, int64_t S, int64_t m, bool always, const void *kernel_fn, void *out, int64_t ldo,
                         hipStream_t st, Launch launch)
{
    return launch_sliced_with(groups, n, (size_t)d * MCP * sizeof(T), (size_t)S * m, always, kernel_fn, launch, [&](double *partial, int nslice) {
        const dim3 rgrid((unsigned)cdiv(m, 256), (unsigned)std::min<int64_t>(S, 32768));
        hipLaunchKernelGGL((apply_reduce_kernel<T, ADD>), rgrid, dim3(256), 0, st, partial, nslice, S, m, (T *)out, ldo);
    });
}

template <typename T, typename EV>
static int launch_mean_ev(const void *xo, int64_t m, const void *x, int64_t n, int d, const KParams &kp, const void *alpha, void *out,
                          hipStream_t st)
{
    const int64_t gx = cdiv(m, MP);
    return launch_sliced<T, false>(gx, n, d, 1, m, false, (const void *)stream_mean_kernel<T, EV>, out, m, st,
                                   [&](const SlicePlan &sp, size_t smem, double *partial) {
        hipLaunchKernelGGL((stream_mean_kernel<T, EV>), dim3((unsigned)gx, (unsigned)sp.nslice), dim3(256), smem, st, (const T *)xo, m,
                           (const T *)x, n, d, kp, (const T *)alpha, sp.slice_len, partial, (T *)out);
    });
}

template <typename T, typename EV, int AP_MP, int AP_SV>
static int launch_apply(const void *xo, int64_t m, const void *x, int64_t n, int d, const KParams &kp, const void *V, int64_t ldv,
                        int64_t S, void *out, int64_t ldo, hipStream_t st)
{
    const int64_t gx = cdiv(m, AP_MP), gz = cdiv(S, AP_SV);
    ProfScope prof(PC_KAPPLY, (double)m * (double)n * (double)gz, st);
    return launch_sliced<T, true>(gx * gz, n, d, S, m, true, (const void *)stream_apply_kernel<T, EV, AP_MP, AP_SV>, out, ldo, st,
                                  [&](const SlicePlan &sp, size_t smem, double *partial) {
        hipLaunchKernelGGL((stream_apply_kernel<T, EV, AP_MP, AP_SV>), dim3((unsigned)gx, (unsigned)sp.nslice, (unsigned)gz), dim3(256), smem,
                           st, (const T *)xo, m, (const T *)x, n, d, kp, (const T *)V, ldv, S, sp.slice_len, partial);
    });
}

// fused posterior mean: out[i] = sum_j member(xo[i], x[j]) * alpha[j]
template <typename T>
static int launch_mean(int kernel, const void *xo, int64_t m, const void *x, int64_t n, int d,
                       const KParams &kp, const void *alpha, void *out, hipStream_t st)
{
    if ((size_t)d * MCP * sizeof(T) > (size_t)LDS_CHUNK_MAX) {
        set_error("mean: d = %d too large", d);
        return GPX_ERR_UNSUPPORTED;
    }
    ProfScope prof(PC_MEAN, (double)m * n, st);
#define GPX_MEAN_LAUNCH(...) return launch_mean_ev<T, __VA_ARGS__>(xo, m, x, n, d, kp, alpha, out, st)
    if (kernel == GPX_KERNEL_GAUSSIAN) {
        switch ((int)kp.c[4]) {
        case 0: GPX_MEAN_LAUNCH(GaussianEval<T, 0>);
        case 1: GPX_MEAN_LAUNCH(GaussianEval<T, 1>);
        default: GPX_MEAN_LAUNCH(GaussianEval<T, 2>);
        }
    }
    if (kp.member == GPX_K) GPX_MEAN_LAUNCH(PeriodicEval<T>);
    if (d != 1) { set_error("periodic derivative members need d == 1 (got %d)", d); return GPX_ERR_UNSUPPORTED; }
    GPX_MEAN_LAUNCH(PeriodicMemberEval<T>);
#undef GPX_MEAN_LAUNCH
}

// The register block of kmat_apply by the number of weight vectors: (test points per workgroup, vectors per lane).  One vector is
// the mean's own shape; up to four keep its 8 points -- the chunk's staging pass and its two barriers are shared by twice
// the pairs -- and from five on the block is 4 x 8.  (Measured with 4 x 8 alone, DESIGN "Posterior paths": S = 1 took 1.7 times
// gpx_d_mean in fp64 and 2.6 times in fp32, where seven of the eight f64 FMAs per kernel value multiplied zeros.)
struct KaShape { int mp, sv; };
static inline KaShape kapply_shape(int64_t S) { return S == 1 ? KaShape{8, 1} : (S <= 4 ? KaShape{8, 4} : KaShape{4, 8}); }

// does the fused kernel take this (d, S)?  the mean's range of d (the chunk of x in LDS), one grid z per vector group
bool kapply_fused_fits(int dtype, int d, int64_t S)
{
    return (size_t)d * MCP * esize(dtype) <= (size_t)LDS_CHUNK_MAX && cdiv(S, kapply_shape(S).sv) <= 65535;
}

template <typename T, typename EV>
static int kapply_fused_t(const void *xo, int64_t m, const void *x, int64_t n, int d, const KParams &kp, const void *V, int64_t ldv,
                          int64_t S, void *out, int64_t ldo, hipStream_t st)
{
    const KaShape sh = kapply_shape(S);
    if (sh.sv == 1) return launch_apply<T, EV, 8, 1>(xo, m, x, n, d, kp, V, ldv, S, out, ldo, st);
    if (sh.sv == 4) return launch_apply<T, EV, 8, 4>(xo, m, x, n, d, kp, V, ldv, S, out, ldo, st);
    return launch_apply<T, EV, 4, 8>(xo, m, x, n, d, kp, V, ldv, S, out, ldo, st);
}

int kapply_fused(int dtype, const void *xo, int64_t m, const void *x, int64_t n, int d, const KParams &kp, const void *V, int64_t ldv,
                 int64_t S, void *out, int64_t ldo, hipStream_t st)
{
    if (kp.kernel == GPX_KERNEL_GAUSSIAN) {
        if (dtype == GPX_F64) return kapply_fused_t<double, GaussianEval<double, 0>>(xo, m, x, n, d, kp, V, ldv, S, out, ldo, st);
        return kapply_fused_t<float, GaussianEval<float, 0>>(xo, m, x, n, d, kp, V, ldv, S, out, ldo, st);
    }
    if (dtype == GPX_F64) return kapply_fused_t<double, PeriodicEval<double>>(xo, m, x, n, d, kp, V, ldv, S, out, ldo, st);
    return kapply_fused_t<float, PeriodicEval<float>>(xo, m, x, n, d, kp, V, ldv, S, out, ldo, st);
}

// ---------------------------------------------------------------------------
// Fused input-space gradient of a prediction:
//   out[i, k] = scale * sum_j w_ij * dk(xo_i, x_j)/dxo_ik,    w_ij = alpha[j]  (the mean)  or  B[i * ldb + j]  (a solved chunk)
//   gaussian  dk/da_k = -(a_k - b_k) / w^2 * k           periodic  dk/da_k = -sin((a_k - b_k) / p) / (p w^2) * k
// stream_mean_kernel's shape: workgroup (bx, by, bz) owns PTS test points, the by-th slice of the training set -- streamed through
// LDS in chunks of 256 points, one per lane -- and the bz-th window of DP dimensions.  Per pair the lane forms the
// distance over ALL d dimensions once, k_ij once (the entry function of kmat_kernel, clamp included: a clamped pair adds
// exactly 0), g = w_ij k_ij in f64, and then for each dimension of the window the difference a_k - b_k itself (never
// xo_ik sum_j g - sum_j g x_jk, which cancels far from the origin) times g into one of PTS x DP f64 accumulators: that per-lane
// state is what the brackets bound, PTS * DP = PG_ACC = 16 -- d <= 4: DP = 4, 4 points; else DP = 16, 1 point; d > 16 takes cdiv(d, 16) windows,
// each of which evaluates k again.  For the distance the test points are wave-uniform SGPR operands (scalar cache).  Lanes are
// added by shuffles, waves through LDS, slices by pred_grad_reduce_kernel, all in a fixed order: no atomics, bitwise repeatable.
// ---------------------------------------------------------------------------
constexpr int PG_ACC = 16;         // f64 accumulators per lane

template <typename T, int KIND, int DP>
__global__ __launch_bounds__(256) void pred_grad_kernel(const T *__restrict__ xo, int64_t m, const T *__restrict__ x, int64_t n,
                                                        int d, KParams kp, const T *__restrict__ alpha, const T *__restrict__ B,
                                                        int64_t ldb, int64_t slice_len, double *__restrict__ partial)
{
    constexpr int PTS = PG_ACC / DP;
    constexpr int KU = KIND == GPX_KERNEL_GAUSSIAN ? 2 : 1;   // unrolling of the distance loop (periodic: ONE inlined sincos)
    static_assert(KIND == GPX_KERNEL_GAUSSIAN || PTS == 1, "the periodic pass reuses the lane's slot of the chunk");
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    T *sx = reinterpret_cast<T *>(smem_raw);            // [d][MCP] chunk of x, transposed
    __shared__ double red[4][PTS * DP];

    const int tid = threadIdx.x;
    const int64_t p0 = (int64_t)blockIdx.x * PTS;
    const int kbeg = (int)blockIdx.z * DP;              // this workgroup's window of dimensions
    double acc[PTS][DP];
#pragma unroll
    for (int pp = 0; pp < PTS; ++pp)
#pragma unroll
        for (int kk = 0; kk < DP; ++kk) acc[pp][kk] = 0.0;
    const T *brow[PTS];
#pragma unroll
    for (int pp = 0; pp < PTS; ++pp) brow[pp] = B ? B + min(p0 + pp, m - 1) * ldb : alpha;   // (alpha: the same weights for every point)

    // this window's coordinates of the test points live in VECTOR registers (staged through LDS): as SGPR operands like the
    // rest of the point they are PG_ACC loop invariants on top of the pointers and constants, more than the scalar file holds
    T *sa = sx + (size_t)d * MCP;                       // [PTS][d]
    for (int idx = tid; idx < PTS * d; idx += 256) {
        const int pp = PTS == 1 ? 0 : idx / d;
        sa[idx] = xo[min(p0 + pp, m - 1) * d + (idx - pp * d)];
    }
    __syncthreads();
    T av[PTS][DP];
#pragma unroll
    for (int pp = 0; pp < PTS; ++pp)
#pragma unroll
        for (int kk = 0; kk < DP; ++kk) av[pp][kk] = (kbeg + kk < d) ? sa[pp * d + kbeg + kk] : (T)0;

    // gaussian: c1, c2 of gaussian_entry; periodic: h^2, -2 / w^2, p
    const T c1 = KIND == GPX_KERNEL_GAUSSIAN ? (T)kp.c[0] : (T)kp.c[0] * (T)kp.c[0];
    const T c2 = KIND == GPX_KERNEL_GAUSSIAN ? (T)kp.c[1] : (T)-2.0 / ((T)kp.c[1] * (T)kp.c[1]);
    const T per = (T)kp.c[2];
    const int qd = 256 / d, rd = 256 - qd * d;          // idx += 256  <=>  (c, k) += (qd, rd) with carry
    const int cst = tid / d, kst = tid - cst * d;
    const int64_t jbeg = (int64_t)blockIdx.y * slice_len, jend = min(n, jbeg + slice_len);
    for (int64_t j0 = jbeg; j0 < jend; j0 += 256) {
        __syncthreads();
        {
            const int64_t lim = (jend - j0) * d;
            const T *g = x + j0 * d;
            GPX_STAGE_POINTS_TRANSPOSED(sx, MCP, g, 256 * d, lim, d, tid, qd, rd, cst, kst);
        }
        __syncthreads();
        const int64_t j = j0 + tid;
        if (j < jend) {
            T r[PTS];
#pragma unroll
            for (int pp = 0; pp < PTS; ++pp) r[pp] = (T)0;
#pragma unroll KU
            for (int k = 0; k < d; ++k) {
                const T b = sx[(size_t)k * MCP + tid];
#pragma unroll
                for (int pp = 0; pp < PTS; ++pp) {
                    const T a = sa[pp * d + k];
                    if (KIND == GPX_KERNEL_GAUSSIAN) {
                        r[pp] = pair_term<T, GPX_KERNEL_GAUSSIAN>(a, b, per, r[pp]);
                    } else {
                        // PTS == 1: the lane's slot of the chunk is its own from here on, and takes sin((a - b) / p) =
                        // 2 sin cos of the half angle for the pass below -- one sincos per pair and dimension
                        T sn, cs;
                        dev_sincos<T>((T)0.5 * (a - b) / per, &sn, &cs);
                        r[pp] = fma(sn, sn, r[pp]);
                        sx[(size_t)k * MCP + tid] = (T)2.0 * sn * cs;
                    }
                }
            }
            double g[PTS];
#pragma unroll
            for (int pp = 0; pp < PTS; ++pp) {
                const T kv = KIND == GPX_KERNEL_GAUSSIAN ? gaussian_entry<T, 0>(r[pp], c1, c2, (T)0, (T)0)
                                                          : c1 * dev_exp<T>(c2 * r[pp]);
                const T wv = brow[pp][j];
                g[pp] = (double)kv * (double)wv;
            }
#pragma unroll
            for (int kk = 0; kk < DP; ++kk) {
                if (kbeg + kk < d) {                                      // (uniform: d and the window are scalars)
                    const T b = sx[(size_t)(kbeg + kk) * MCP + tid];
#pragma unroll
                    for (int pp = 0; pp < PTS; ++pp) {
                        const T f = KIND == GPX_KERNEL_GAUSSIAN ? av[pp][kk] - b : b;
                        acc[pp][kk] = fma(g[pp], (double)f, acc[pp][kk]);
                    }
                }
            }
        }
    }
    // wave reduction (64 lanes), then across the 4 waves in a fixed order
    block_sum_fixed(reinterpret_cast<const double (&)[PTS * DP]>(acc), red, tid);               // (acc as [pp * DP + kk])
    __syncthreads();
    if (tid < PTS * DP) {
        const int pp = tid / DP, kk = tid - pp * DP;
        if (p0 + pp < m && kbeg + kk < d)
            partial[((int64_t)blockIdx.y * m + p0 + pp) * d + kbeg + kk] = block_sum_final(red, tid);
    }
}

// out[i, k] = factor * sum over the slices (in slice order) [/ div.w[k]]
template <bool DIV>
__global__ void pred_grad_reduce_kernel(const double *__restrict__ partial, int nslice, int64_t md, int d, double factor,
                                        ArdWidths div, double *__restrict__ out)
{
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= md) return;
    double sum = 0.0;
    for (int y = 0; y < nslice; ++y) sum += partial[(int64_t)y * md + e];
    sum *= factor;
    if (DIV) sum /= div.w[e % d];
    out[e] = sum;
}

template <typename T>
static int launch_pred_grad(int kernel, const void *xo, int64_t m, const void *x, int64_t n, int d, const KParams &kp,
                            const void *alpha, const void *B, int64_t ldb, double scale, const double *col_div, double *out,
                            hipStream_t st)
{
    if ((size_t)d * MCP * sizeof(T) > (size_t)LDS_CHUNK_MAX) {        // the mean's range of d
        set_error("pred_grad: d = %d too large", d);
        return GPX_ERR_UNSUPPORTED;
    }
    if (col_div && d > GPX_ARD_MAX_D) { set_error("pred_grad: column divisors need d <= %d (got %d)", GPX_ARD_MAX_D, d); return GPX_ERR_ARG; }
    const int DP = (d <= 4 && kernel == GPX_KERNEL_GAUSSIAN) ? 4 : 16, PTS = PG_ACC / DP;   // (periodic: one point a workgroup)
    const size_t smem = (size_t)d * (MCP + PTS) * sizeof(T);   // the chunk of x and the group's test points
    const int64_t gx = cdiv(m, PTS), gz = cdiv(d, DP);
    const SlicePlan sp = slice_plan(gx * gz, n);
    void *scr = nullptr;
    GPX_TRY(g_partial_scr.get((size_t)sp.nslice * m * d * sizeof(double), &scr));
    double *partial = (double *)scr;
    // the derivative's constant: gaussian -1 / w^2 = 2 c1, periodic -1 / (p w^2)
    const double factor = scale * (kernel == GPX_KERNEL_GAUSSIAN ? 2.0 * kp.c[0] : -1.0 / (kp.c[2] * kp.c[1] * kp.c[1]));
    ArdWidths aw;
    for (int k = 0; k < GPX_ARD_MAX_D; ++k) aw.w[k] = (col_div && k < d) ? col_div[k] : 1.0;
    dim3 grid((unsigned)gx, (unsigned)sp.nslice, (unsigned)gz), block(256);
    ProfScope prof(PC_PRED_GRAD, (double)m * n * gz, st);
    // (the largest d whose chunk fits leaves room for the test points too: fp64 d = 47: 97008 bytes, fp32 d = 95: 98040)
#define GPX_PGRAD_LAUNCH(KIND, DPV)                                                                       \
    do {                                                                                                  \
        if (smem > 48 * 1024) GPX_TRY(set_max_lds((const void *)pred_grad_kernel<T, KIND, DPV>, LDS_CHUNK_MAX));     \
        hipLaunchKernelGGL((pred_grad_kernel<T, KIND, DPV>), grid, block, smem, st, (const T *)xo, m,     \
                           (const T *)x, n, d, kp, (const T *)alpha, (const T *)B, ldb, sp.slice_len, partial); \
    } while (0)
    if (kernel != GPX_KERNEL_GAUSSIAN) GPX_PGRAD_LAUNCH(GPX_KERNEL_PERIODIC, 16);
    else if (DP == 4) GPX_PGRAD_LAUNCH(GPX_KERNEL_GAUSSIAN, 4);
    else GPX_PGRAD_LAUNCH(GPX_KERNEL_GAUSSIAN, 16);
#undef GPX_PGRAD_LAUNCH
    GPX_LAUNCH_CHECK();
    const int64_t md = m * d;
    if (col_div)
        hipLaunchKernelGGL((pred_grad_reduce_kernel<true>), dim3((unsigned)cdiv(md, 256)), dim3(256), 0, st, partial, (int)sp.nslice, md, d, factor, aw, out);
    else
        hipLaunchKernelGGL((pred_grad_reduce_kernel<false>), dim3((unsigned)cdiv(md, 256)), dim3(256), 0, st, partial, (int)sp.nslice, md, d, factor, aw, out);
    GPX_LAUNCH_CHECK();
    return GPX_OK;
}

int pred_grad(int dtype, int kernel, const void *xo, int64_t m, const void *x, int64_t n, int d, const double *params,
              const void *alpha, const void *B, int64_t ldb, double scale, const double *col_div, double *out_dev, hipStream_t st)
{
    if (m <= 0) return GPX_OK;
    if (kernel != GPX_KERNEL_GAUSSIAN && kernel != GPX_KERNEL_PERIODIC) { set_error("pred_grad: unknown kernel family %d", kernel); return GPX_ERR_ARG; }
    if (n <= 0) { GPX_HIP(hipMemsetAsync(out_dev, 0, (size_t)m * d * sizeof(double), st)); return GPX_OK; }
    KParams kp;
    GPX_TRY(make_kparams(kernel, GPX_K, params, 0.0, &kp));
    if (dtype == GPX_F64) return launch_pred_grad<double>(kernel, xo, m, x, n, d, kp, alpha, B, ldb, scale, col_div, out_dev, st);
    return launch_pred_grad<float>(kernel, xo, m, x, n, d, kp, alpha, B, ldb, scale, col_div, out_dev, st);
}

// ---------------------------------------------------------------------------
// The input-space gradient of K(xo, x) applied to S weight vectors (gpx_d_kmat_apply_grad; gaussian only):
//   out[s, i d + k] += (1 / div_k) sum_j V[s, j] dk(xo_i, x_j)/dxo_ik,        dk/da_k = -(a_k - b_k) / w^2 * k
// pred_grad_kernel's pair loop with stream_apply_kernel's register block of weight vectors: workgroup (bx, by, bz) owns PTS
// test points and the window of DP dimensions bx % W (windows are the fast index: neighbours share their points and slice),
// the by-th slice of the training set and the bz-th group of SV weight vectors.  Per pair the lane forms the distance over ALL d
// dimensions once and k_ij once (GaussianEval<T, 0>: the element gpx_d_kmat would store, clamp included: a clamped pair adds
// exactly 0); per chunk it loads V[s0 .. s0 + SV, j] once (coalesced across the lanes, zero beyond S); g_s = k_ij V[s, j] in
// f64, and for each dimension of the window the difference a_k - b_k itself times g_s into one of PTS x SV x DP <= KG_ACC f64
// accumulators.  This window's coordinates of the test points live in vector registers, staged through LDS (pred_grad_kernel
// says why).  Lanes are added by shuffles, waves through LDS, slices by apply_grad_reduce_kernel -- which also applies -1 / w^2,
// the division, the += and the one rounding to T -- all in a fixed order: no atomics, bitwise repeatable.
// ---------------------------------------------------------------------------
constexpr int KG_ACC = 32;         // f64 accumulators per lane at most: stream_apply_kernel's budget

template <typename T, int PTS, int SV, int DP>
__global__ __launch_bounds__(256) void stream_apply_grad_kernel(const T *__restrict__ xo, int64_t m, const T *__restrict__ x, int64_t n,
                                                                int d, int W, KParams kp, const T *__restrict__ V, int64_t ldv, int64_t S,
                                                                int64_t slice_len, double *__restrict__ partial)
{
    static_assert(PTS * SV * DP <= KG_ACC, "the register block is at most KG_ACC f64 accumulators");
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    T *sx = reinterpret_cast<T *>(smem_raw);            // [d][MCP] chunk of x, transposed
    __shared__ double red[4][PTS * SV * DP];

    const int tid = threadIdx.x;
    const int64_t pg = (int64_t)blockIdx.x / W;
    const int64_t p0 = pg * PTS;
    const int kbeg = (int)((int64_t)blockIdx.x - pg * W) * DP;   // this workgroup's window of dimensions
    const int64_t s0 = (int64_t)blockIdx.z * SV;
    double acc[PTS][SV][DP];
#pragma unroll
    for (int pp = 0; pp < PTS; ++pp)
#pragma unroll
        for (int sv = 0; sv < SV; ++sv)
#pragma unroll
            for (int kk = 0; kk < DP; ++kk) acc[pp][sv][kk] = 0.0;

    T *sa = sx + (size_t)d * MCP;                       // [PTS][d]: the group's test points
    for (int idx = tid; idx < PTS * d; idx += 256) {
        const int pp = PTS == 1 ? 0 : idx / d;
        sa[idx] = xo[min(p0 + pp, m - 1) * d + (idx - pp * d)];
    }
    __syncthreads();
    T av[PTS][DP];
#pragma unroll
    for (int pp = 0; pp < PTS; ++pp)
#pragma unroll
        for (int kk = 0; kk < DP; ++kk) av[pp][kk] = (kbeg + kk < d) ? sa[pp * d + kbeg + kk] : (T)0;

    const GaussianEval<T, 0> ev(kp);
    const int qd = 256 / d, rd = 256 - qd * d;          // idx += 256  <=>  (c, k) += (qd, rd) with carry
    const int cst = tid / d, kst = tid - cst * d;
    const int64_t jbeg = (int64_t)blockIdx.y * slice_len, jend = min(n, jbeg + slice_len);
    for (int64_t j0 = jbeg; j0 < jend; j0 += 256) {
        __syncthreads();
        {
            const int64_t lim = (jend - j0) * d;
            const T *g = x + j0 * d;
            GPX_STAGE_POINTS_TRANSPOSED(sx, MCP, g, 256 * d, lim, d, tid, qd, rd, cst, kst);
        }
        __syncthreads();
        const int64_t j = j0 + tid;
        if (j < jend) {
            double vj[SV];
#pragma unroll
            for (int sv = 0; sv < SV; ++sv) vj[sv] = (s0 + sv < S) ? (double)V[(s0 + sv) * ldv + j] : 0.0;
            T r[PTS];
#pragma unroll
            for (int pp = 0; pp < PTS; ++pp) r[pp] = (T)0;
#pragma unroll 2
            for (int k = 0; k < d; ++k) {
                const T b = sx[(size_t)k * MCP + tid];
#pragma unroll
                for (int pp = 0; pp < PTS; ++pp) { const T a = sa[pp * d + k]; r[pp] = ev.step(a, b, r[pp]); }
            }
            double g[PTS][SV];
#pragma unroll
            for (int pp = 0; pp < PTS; ++pp) {
                const double kd = (double)ev.entry(r[pp]);
#pragma unroll
                for (int sv = 0; sv < SV; ++sv) g[pp][sv] = kd * vj[sv];
            }
#pragma unroll
            for (int kk = 0; kk < DP; ++kk) {
                if (kbeg + kk < d) {                                      // (uniform: d and the window are scalars)
                    const T b = sx[(size_t)(kbeg + kk) * MCP + tid];
#pragma unroll
                    for (int pp = 0; pp < PTS; ++pp) {
                        const double f = (double)(av[pp][kk] - b);
#pragma unroll
                        for (int sv = 0; sv < SV; ++sv) acc[pp][sv][kk] = fma(g[pp][sv], f, acc[pp][sv][kk]);
                    }
                }
            }
        }
    }
    // wave reduction (64 lanes), then across the 4 waves in a fixed order
    block_sum_fixed(reinterpret_cast<const double (&)[PTS * SV * DP]>(acc), red, tid);          // (acc as [(pp * SV + sv) * DP + kk])
    __syncthreads();
    if (tid < PTS * SV * DP) {
        const int ps = tid / DP, kk = tid - ps * DP, pp = ps / SV, sv = ps - pp * SV;
        if (p0 + pp < m && s0 + sv < S && kbeg + kk < d)
            partial[(((int64_t)blockIdx.y * S + s0 + sv) * m + p0 + pp) * d + kbeg + kk] = block_sum_final(red, tid);
    }
}

// out[s, e] += factor * sum over the slices (in slice order) [/ div.w[e % d]], e = i d + k; one rounding to T
template <typename T, bool DIV>
__global__ __launch_bounds__(256) void apply_grad_reduce_kernel(const double *__restrict__ partial, int nslice, int64_t S, int64_t md, int d,
                                                                double factor, ArdWidths div, T *__restrict__ out, int64_t ldo)
{
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= md) return;
    for (int64_t s = blockIdx.y; s < S; s += gridDim.y) {
        double sum = 0.0;
        for (int y = 0; y < nslice; ++y) sum += partial[((int64_t)y * S + s) * md + e];
        sum *= factor;
        if (DIV) sum /= div.w[e % d];
        out[s * ldo + e] = (T)((double)out[s * ldo + e] + sum);
    }
}

// The register block of kmat_apply_grad by S and d: (test points per workgroup, vectors per lane, dimensions per window), at
// most KG_ACC accumulators.  d <= 4: one window of 4, and the points make up the budget -- 4 x 1 x 4 (pred_grad_kernel's block),
// 4 x 2 x 4, 2 x 4 x 4.  d > 4: one point -- 1 x 1 x 16 (pred_grad_kernel's block), 1 x 2 x 16, 1 x 4 x 8.  One or two vectors get
// a block of their own: the lesson of kapply_shape -- a block of 4 vectors at S = 1 multiplies zeros in three of its four
// f64 FMAs per difference.  DESIGN "Posterior paths" has the table and the compiler's resources.
struct KgShape { int pts, sv, dp; };
static inline KgShape kapply_grad_shape(int64_t S, int d)
{
    if (d <= 4) return S == 1 ? KgShape{4, 1, 4} : (S == 2 ? KgShape{4, 2, 4} : KgShape{2, 4, 4});
    return S == 1 ? KgShape{1, 1, 16} : (S == 2 ? KgShape{1, 2, 16} : KgShape{1, 4, 8});
}

template <typename T, int PTS, int SV, int DP>
static int launch_apply_grad(const void *xo, int64_t m, const void *x, int64_t n, int d, const KParams &kp, const ArdWidths &aw, bool div,
                             const void *V, int64_t ldv, int64_t S, void *out, int64_t ldo, hipStream_t st)
{
    const int64_t W = cdiv(d, DP), gx = cdiv(m, PTS) * W, gz = cdiv(S, SV), md = m * d;
    const double factor = 2.0 * kp.c[0];                // the derivative's constant: -1 / w^2 = 2 c1
    ProfScope prof(PC_KAPPLY_GRAD, (double)m * (double)n * (double)gz * (double)W, st);
    // (LDS: the chunk of x and the group's test points; the largest d whose chunk fits leaves room for them: fp64 d = 47: 97008
    // bytes, fp32 d = 95: 98040)
    return launch_sliced_with(gx * gz, n, (size_t)d * (MCP + PTS) * sizeof(T), (size_t)S * md, true,
                              (const void *)stream_apply_grad_kernel<T, PTS, SV, DP>,
                              [&](const SlicePlan &sp, size_t smem, double *partial) {
        hipLaunchKernelGGL((stream_apply_grad_kernel<T, PTS, SV, DP>), dim3((unsigned)gx, (unsigned)sp.nslice, (unsigned)gz), dim3(256), smem, st,
                           (const T *)xo, m, (const T *)x, n, d, (int)W, kp, (const T *)V, ldv, S, sp.slice_len, partial);
    }, [&](double *partial, int nslice) {
        const dim3 rgrid((unsigned)cdiv(md, 256), (unsigned)std::min<int64_t>(S, 32768));
        if (div) hipLaunchKernelGGL((apply_grad_reduce_kernel<T, true>), rgrid, dim3(256), 0, st, partial, nslice, S, md, d, factor, aw, (T *)out, ldo);
        else hipLaunchKernelGGL((apply_grad_reduce_kernel<T, false>), rgrid, dim3(256), 0, st, partial, nslice, S, md, d, factor, aw, (T *)out, ldo);
    });
}

template <typename T>
static int kapply_grad_t(const void *xo, int64_t m, const void *x, int64_t n, int d, const KParams &kp, const double *col_div,
                         const void *V, int64_t ldv, int64_t S, void *out, int64_t ldo, hipStream_t st)
{
    ArdWidths aw;
    for (int k = 0; k < GPX_ARD_MAX_D; ++k) aw.w[k] = (col_div && k < d) ? col_div[k] : 1.0;
    const KgShape sh = kapply_grad_shape(S, d);
#define GPX_KGRAD_LAUNCH(P, V_, D) return launch_apply_grad<T, P, V_, D>(xo, m, x, n, d, kp, aw, col_div != nullptr, V, ldv, S, out, ldo, st)
    if (sh.dp == 4) {
        if (sh.sv == 1) GPX_KGRAD_LAUNCH(4, 1, 4);
        if (sh.sv == 2) GPX_KGRAD_LAUNCH(4, 2, 4);
        GPX_KGRAD_LAUNCH(2, 4, 4);
    }
    if (sh.sv == 1) GPX_KGRAD_LAUNCH(1, 1, 16);
    if (sh.sv == 2) GPX_KGRAD_LAUNCH(1, 2, 16);
    GPX_KGRAD_LAUNCH(1, 4, 8);
#undef GPX_KGRAD_LAUNCH
}

int kapply_grad(int dtype, const void *xo, int64_t m, const void *x, int64_t n, int d, const double *params, const double *col_div,
                const void *V, int64_t ldv, int64_t S, void *out, int64_t ldo, hipStream_t st)
{
    if (m <= 0 || S <= 0 || n <= 0) return GPX_OK;
    if ((size_t)d * MCP * esize(dtype) > (size_t)LDS_CHUNK_MAX) {     // the mean's range of d
        set_error("kmat_apply_grad: d = %d too large", d);
        return GPX_ERR_UNSUPPORTED;
    }
    if (col_div && d > GPX_ARD_MAX_D) { set_error("kmat_apply_grad: column divisors need d <= %d (got %d)", GPX_ARD_MAX_D, d); return GPX_ERR_ARG; }
    const KgShape sh = kapply_grad_shape(S, d);
    if (cdiv(S, sh.sv) > 65535) { set_error("kmat_apply_grad: S = %lld is more groups of weight vectors than one launch covers", (long long)S); return GPX_ERR_ARG; }
    if (cdiv(m, sh.pts) > 0x7fffffff / cdiv(d, sh.dp)) { set_error("kmat_apply_grad: m is more than one launch covers"); return GPX_ERR_ARG; }
    KParams kp;
    GPX_TRY(make_kparams(GPX_KERNEL_GAUSSIAN, GPX_K, params, 0.0, &kp));
    if (dtype == GPX_F64) return kapply_grad_t<double>(xo, m, x, n, d, kp, col_div, V, ldv, S, out, ldo, st);
    return kapply_grad_t<float>(xo, m, x, n, d, kp, col_div, V, ldv, S, out, ldo, st);
}

}  // namespace gpx

using namespace gpx;

extern "C" {

int gpx_d_mean_member(int dtype, int kernel, int member, const void *xo, int64_t m, const void *x,
                      int64_t n, int d, const double *params, const void *alpha, void *out, void *stream)
{
    gpx::StreamTurn turn__((hipStream_t)stream);     // (this thread's scratch buffers: one stream at a time, gpx_mem.h)
    GPX_TRY(ensure_device());
    GPX_ARG(dtype == GPX_F64 || dtype == GPX_F32, "dtype must be GPX_F64 or GPX_F32");
    GPX_ARG(n >= 0 && m >= 0 && d >= 1, "need n, m >= 0 and d >= 1");
    if (m == 0) return GPX_OK;
    GPX_ARG(xo && out && (n == 0 || (x && alpha)), "NULL pointer");
    KParams kp;
    GPX_TRY(make_kparams(kernel, member, params, 0.0, &kp));
    if (dtype == GPX_F64) return launch_mean<double>(kernel, xo, m, x, n, d, kp, alpha, out, S(stream));
    return launch_mean<float>(kernel, xo, m, x, n, d, kp, alpha, out, S(stream));
}

int gpx_d_mean(int dtype, int kernel, const void *xo, int64_t m, const void *x, int64_t n, int d,
               const double *params, const void *alpha, void *out, void *stream)
{
    gpx::StreamTurn turn__((hipStream_t)stream);     // (this thread's scratch buffers: one stream at a time, gpx_mem.h)
    return gpx_d_mean_member(dtype, kernel, GPX_K, xo, m, x, n, d, params, alpha, out, stream);
}

int gpx_d_pred_grad(int dtype, int kernel, const void *xo, int64_t m, const void *x, int64_t n, int d, const double *params,
                    const void *alpha, const void *B, int64_t ldb, double scale, double *out_dev, void *stream)
{
    gpx::StreamTurn turn__((hipStream_t)stream);     // (this thread's scratch buffers: one stream at a time, gpx_mem.h)
    GPX_TRY(ensure_device());
    GPX_ARG(dtype == GPX_F64 || dtype == GPX_F32, "dtype must be GPX_F64 or GPX_F32");
    GPX_ARG(n >= 0 && m >= 0 && d >= 1, "need n, m >= 0 and d >= 1");
    GPX_ARG((alpha != nullptr) != (B != nullptr) || n == 0, "exactly one of alpha / B");
    if (m == 0) return GPX_OK;
    GPX_ARG(xo && out_dev && params && (n == 0 || x), "NULL pointer");
    GPX_ARG(!B || ldb >= n, "ldb < n");
    if (kernel == GPX_KERNEL_GAUSSIAN_ARD) {
        // as gpx_d_kmat: the isotropic pass on (xo / w, x / w; h / sqrt(wbar), 1), column k divided by w_k
        GPX_ARG(d <= GPX_ARD_MAX_D, "the ARD family needs d <= GPX_ARD_MAX_D");
        const size_t es = esize(dtype), b1 = ((size_t)m * d * es + 255) / 256 * 256;
        void *scr = nullptr;
        GPX_TRY(ard_scratch(b1 + (size_t)n * d * es, &scr));
        void *s1 = scr, *s2 = (char *)scr + b1;
        GPX_TRY(scale_points(dtype, xo, m, d, params + 1, s1, S(stream)));
        GPX_TRY(scale_points(dtype, x, n, d, params + 1, s2, S(stream)));
        double iso[2];
        ard_iso(params, d, iso);
        return pred_grad(dtype, GPX_KERNEL_GAUSSIAN, s1, m, s2, n, d, iso, alpha, B, ldb, scale, params + 1, out_dev, S(stream));
    }
    return pred_grad(dtype, kernel, xo, m, x, n, d, params, alpha, B, ldb, scale, nullptr, out_dev, S(stream));
}

int gpx_d_kmat_apply_grad(int dtype, int kernel, const void *xo, int64_t m, const void *x, int64_t n, int d, const double *params,
                          const double *col_div, const void *V, int64_t ldv, int64_t Sn, void *out, int64_t ldo, void *stream)
{
    gpx::StreamTurn turn__((hipStream_t)stream);     // (this thread's scratch buffers: one stream at a time, gpx_mem.h)
    GPX_TRY(ensure_device());
    GPX_ARG(dtype == GPX_F64 || dtype == GPX_F32, "dtype must be GPX_F64 or GPX_F32");
    GPX_ARG(n >= 0 && m >= 0 && Sn >= 0 && d >= 1, "need n, m, S >= 0 and d >= 1");
    if (kernel != GPX_KERNEL_GAUSSIAN) {
        set_error("gpx_d_kmat_apply_grad: kernel family %d is not supported (GPX_KERNEL_GAUSSIAN; the ARD family on scaled points with col_div = w)", kernel);
        return GPX_ERR_UNSUPPORTED;
    }
    if (m == 0 || Sn == 0 || n == 0) return GPX_OK;
    GPX_ARG(xo && x && V && out && params, "NULL pointer");
    GPX_ARG(m <= INT64_MAX / d && ldv >= n && ldo >= m * d, "leading dimension too small");
    GPX_ARG(Sn <= INT64_MAX / ldv && Sn <= (INT64_MAX / 8) / ldo, "S * ld overflows");
    return kapply_grad(dtype, xo, m, x, n, d, params, col_div, V, ldv, Sn, out, ldo, S(stream));
}

}  // extern "C"
