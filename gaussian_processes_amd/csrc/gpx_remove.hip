// gpx_remove.hip -- dropping k observations from a fitted GP without refactoring (gpx_d_chol_delete, gpx_gp_remove).
//
// Deleting row / column i of K = L L^T leaves the rows and columns of L before i as they are; the factor behind i takes a
// rank-1 UPDATE,  L33' L33'^T = L33 L33^T + l32 l32^T  (l32: column i below the diagonal), done by Givens rotations: stable
// whatever the matrix, no pivot can turn non-positive, no kernel evaluation.  For k sorted indices r_0 < ... < r_{k-1} the k
// updates are interleaved in ONE pass over the factor.  V (n x k) holds the update vectors; walking the columns j = r_0 ..
// n - 1 in ascending order:
//   for every vector q that is already active (r_q < j), q ascending:
//       a = L[j, j], b = V[j, q], rho = sqrt(a^2 + b^2), c = a / rho, s = b / rho
//       rows t >= j:  L[t, j] <- c L[t, j] + s V[t, q],  V[t, q] <- c V[t, q] - s L[t, j]      (both from the old values)
//   if j == r_q: the column -- rotated by every vector born before it -- becomes vector q (V[t, q] = L[t, j], t > j) and is dropped
// The result is the kept rows and columns, order preserved.  Only two orders matter: for one column the vectors ascend, for
// one vector the columns ascend.  Here: column blocks of DEL_W columns, one launch each (the dependency between blocks is
// carried by V alone: stream order is enough); inside a block groups of G (16 or 32) vectors outermost, then the block's columns,
// then the group's vectors.  Within one column the b's of different vectors do not depend on each other (a rotation only
// clears its own b), so the pivots are the partial sums a^2 + sum b_q^2 and all c, s of a (column, group) are formed at once.
#include "gpx_small.h"
#include <algorithm>

#include "gpx_gp_internal.h"
#include "gpx_kernels_dev.h"

namespace gpx {

// DEL_W columns a launch, DEL_ROWS rows a workgroup (one thread per row); the vectors are taken G at a time (in registers):
// 16 when there are no more than that, otherwise 32.  Every (column, group) step applies all G rotations (the identity for
// vectors that are not active) behind a fixed chain of latencies that 32 vectors share: measured at n = 65536 fp64, 32 against
// 16 made k = 256 25 % faster and k <= 16 30 % slower ("Shrinking a fitted GP")
constexpr int DEL_W = 32, DEL_ROWS = 256, DEL_G_SMALL = 16, DEL_G_LARGE = 32;
// a workgroup: one wave for the chain of the diagonal rows, then one thread per row of the band
constexpr int DEL_THREADS = 64 + DEL_ROWS;

// removed indices below t (idx sorted ascending): the first m with idx[m] >= t
__device__ __forceinline__ int64_t removed_below(const int64_t *__restrict__ idx, int64_t k, int64_t t)
{
    int64_t lo = 0, hi = k;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (idx[mid] < t) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// x of the lane `N` below within its row of 16 lanes, zero where there is none (DPP row_shr: no LDS round trip)
template <int N> __device__ __forceinline__ float row_shr(float x)
{
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(x), 0x110 + N, 0xf, 0xf, true));
}
template <int N> __device__ __forceinline__ double row_shr(double x)
{
    return __hiloint2double(__builtin_amdgcn_update_dpp(0, __double2hiint(x), 0x110 + N, 0xf, 0xf, true),
                            __builtin_amdgcn_update_dpp(0, __double2loint(x), 0x110 + N, 0xf, 0xf, true));
}
// x of lane `lane`, the same for every lane (v_readlane)
__device__ __forceinline__ double lane_value(double x, int lane)
{
    return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(x), lane), __builtin_amdgcn_readlane(__double2loint(x), lane));
}
__device__ __forceinline__ float lane_value(float x, int lane) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(x), lane)); }
// LDS written by one lane of a wave is read by another lane of the SAME wave: the wave's LDS accesses complete in order, the
// compiler must not move them across this point
__device__ __forceinline__ void wave_lds_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// LDS of one workgroup of del_block_kernel<T>, in bytes: the candidates (int64), the T arrays, the int arrays
template <int G> constexpr int del_lds_elems()
{
    return DEL_W * (DEL_W + 1) + DEL_W * (G + 1) + 2 * DEL_W * G * 2 + DEL_ROWS * (DEL_W + 1) + 2;
}
template <typename T, int G> constexpr int del_lds_bytes()
{
    return DEL_W * 8 + del_lds_elems<G>() * (int)sizeof(T) + (DEL_W + (DEL_W + 1) + DEL_ROWS + 1) * 4;
}

// One column block [c0, c0 + wb) of the pass (wb == DEL_W but for the ragged last block, which has no rows below it).
// m0: removed indices below c0 == vectors active when the block begins.  Workgroup 0 owns the block's wb diagonal rows and
// writes them; workgroup 1 + b owns the band of DEL_ROWS rows from c0 + wb + b * DEL_ROWS on (thread 64 + i: row i).  Per
// group of vectors EVERY workgroup walks the diagonal rows itself -- that is where c and s come from; redundantly, a serial chain whose
// cost is the number of instructions on it: ONE wave, in LDS, no workgroup barrier; per column lane r forms c, s of vector
// r (the pivots by a DPP scan over the lanes, one rsqrt each), then lane t rotates row t -- and leaves the table of the
// group's c, s in LDS; the other threads apply the table to their rows of the band, column by column, while the first
// wave is at the next group.
// V[q * n + t]; rows [c0, c0 + wb) of V are read by all and written by none (no later block needs them), the band's rows
// are read and written by their owner alone.
template <typename T, int G>
__global__ __launch_bounds__(DEL_THREADS) void del_block_kernel(const T *__restrict__ L, int64_t ldl, int64_t n, const int64_t *__restrict__ idx,
                                                             int64_t k, int64_t m0, int64_t c0, int wb, T *__restrict__ V,
                                                             T *__restrict__ out, int64_t ldo, int aligned)
{
    constexpr int W = DEL_W, R = DEL_ROWS, NT = DEL_THREADS, PD = W + 1, PV = G + 1, PT = W + 1;
    static_assert(W <= 64 && (G == 16 || G == 32), "the chain is one wave: a lane per diagonal row, one or two DPP rows of 16 lanes for the vectors of the group");
    constexpr int VEC = Vec<T>::N;
    typedef typename Vec<T>::type VT;
    extern __shared__ __align__(16) unsigned char del_smem[];
    long long *cand = reinterpret_cast<long long *>(del_smem);          // [W] the next removed indices from m0 on (-1: none)
    T *D = reinterpret_cast<T *>(cand + W);                             // [W][PD] the diagonal rows, columns of the block
    T *Vd = D + W * PD;                                                 // [W][PV] ... their entries of the group's vectors
    T *tab = Vd + W * PV;                                               // 2 x [W][G][2] c, s of (column, vector); (1, 0): not active.  The group being made, the one being applied
    T *Tt = tab + 2 * W * G * 2;                                        // [R][PT] the band's tile
    T *dnew = Tt + R * PT;                                              // [2] the column's pivot after the group
    int *born = reinterpret_cast<int *>(dnew + 2);                      // [W] 1: the column is a removed index
    int *cnt = born + W;                                                // [W + 1] removed indices in [c0, c0 + jj)
    int *rowm = cnt + W + 1;                                            // [R] removed indices below the band's row, -1: the row is one

    const int tid = threadIdx.x;
    const bool band = blockIdx.x > 0;
    const int64_t tb0 = c0 + wb + (int64_t)(band ? blockIdx.x - 1 : 0) * R;     // the band's first row
    const int bt = tid - 64;                                            // the thread's row of the band; < 0: the chain's wave
    const int64_t trow = tb0 + bt;
    const bool live = band && bt >= 0 && trow < n;

    if (tid < W) cand[tid] = m0 + tid < k ? (long long)idx[m0 + tid] : -1;
    __syncthreads();
    if (tid == 0) {
        int m = 0;
        for (int jj = 0; jj < wb; ++jj) {
            cnt[jj] = m;
            const bool b = cand[m < W ? m : W - 1] == (long long)(c0 + jj) && m < W;
            born[jj] = b ? 1 : 0;
            if (b) ++m;
        }
        cnt[wb] = m;
    }
    // the diagonal rows (lower part) and the band's tile
    for (int i = tid; i < wb * wb; i += NT) {
        const int r = i / wb, c = i - r * wb;
        if (c <= r) D[r * PD + c] = L[(c0 + r) * ldl + c0 + c];
    }
    if (band) {
        if (aligned) {
            constexpr int VW = W / VEC;
            for (int i = tid; i < R * VW; i += NT) {
                const int r = i / VW, cv = i - r * VW;
                if (tb0 + r < n) {
                    const VT v = *reinterpret_cast<const VT *>(L + (tb0 + r) * ldl + c0 + cv * VEC);
                    const T *e = reinterpret_cast<const T *>(&v);
#pragma unroll
                    for (int u = 0; u < VEC; ++u) Tt[r * PT + cv * VEC + u] = e[u];
                }
            }
        } else {
            for (int i = tid; i < R * W; i += NT) {
                const int r = i / W, c = i - r * W;
                if (tb0 + r < n) Tt[r * PT + c] = L[(tb0 + r) * ldl + c0 + c];
            }
        }
        const int64_t m = live ? removed_below(idx, k, trow) : 0;
        if (bt >= 0) rowm[bt] = (live && m < k && idx[m] == trow) ? -1 : (int)(m - m0);     // (relative to m0: fits an int, m - m0 <= rows so far)
    }
    __syncthreads();
    const int64_t mend = m0 + cnt[wb];                    // vectors active when the block ends

    // Group `it` is made by the chain's wave while the bands apply group it - 1 (the two tables alternate): a step costs the
    // longer of the two, not their sum
    const int64_t ngroups = (mend + G - 1) / G;
    for (int64_t it = 0; it <= ngroups; ++it) {
        // 1. the chain (first wave).  Vd: the diagonal rows' entries of the group's vectors -- from V where they were born
        // before this block, zero where they are born inside it
        if (tid < 64 && it < ngroups) {
            const int64_t g0 = it * G;
            T *tabw = tab + (it & 1) * (W * G * 2);
            for (int i = tid; i < wb * G; i += 64) {
                const int r = i / wb, jj = i - r * wb;
                Vd[jj * PV + r] = g0 + r < m0 ? V[(g0 + r) * n + c0 + jj] : (T)0;
            }
            wave_lds_sync();
            for (int jj = 0; jj < wb; ++jj) {
                // vectors of the group active at this column: [0, na); the column is born as vector `na` of the group
                const int64_t act = m0 + cnt[jj] - g0;
                const int na = act < 0 ? 0 : (act > G ? G : (int)act);
                const bool birth = born[jj] != 0 && act >= 0 && act < G;
                if (na == 0 && !birth) continue;
                if (na > 0) {
                    // lane r forms c, s of vector r.  Within one column the b's do not depend on each other: the pivot after
                    // vector r is sqrt(a^2 + sum_{r' <= r} b_r'^2), a scan over the rows of 16 lanes (the second row adds the
                    // first one's total); the vectors that are not active yet get the identity
                    const bool on = tid < na;
                    const T a0 = D[jj * PD + jj], b = on ? Vd[jj * PV + tid] : (T)0, sq = b * b;
                    T inc = sq;
                    inc += row_shr<1>(inc);
                    inc += row_shr<2>(inc);
                    inc += row_shr<4>(inc);
                    inc += row_shr<8>(inc);
                    T excl = row_shr<1>(inc);
                    if (G == 32) { const T first = lane_value(inc, 15); if (tid >= 16) excl += first; }
                    const T post = fma(a0, a0, excl) + sq;
                    const T inv = rsqrt(post), rp = post * inv;
                    T below = row_shr<1>(rp);
                    if (G == 32) { const T last = lane_value(rp, 15); if (tid == 16) below = last; }
                    const T ra = tid == 0 ? a0 : below;
                    if (tid < G) {
                        tabw[(jj * G + tid) * 2] = on ? ra * inv : (T)1;
                        tabw[(jj * G + tid) * 2 + 1] = on ? b * inv : (T)0;
                    }
                    if (tid == na - 1) dnew[0] = rp;
                    wave_lds_sync();
                }
                // lane t rotates row t of the diagonal rows: all G rotations, no branch (c, s and the row's entries of the
                // vectors are loaded ahead of the chain through l)
                if (tid < wb && tid >= jj) {
                    if (tid == jj) {
                        if (na > 0) D[jj * PD + jj] = dnew[0];
                    } else {
                        T l = D[tid * PD + jj];
                        if (na > 0) {
                            T w[G], cs[2 * G];
#pragma unroll
                            for (int r = 0; r < G; ++r) { w[r] = Vd[tid * PV + r]; cs[2 * r] = tabw[(jj * G + r) * 2]; cs[2 * r + 1] = tabw[(jj * G + r) * 2 + 1]; }
#pragma unroll
                            for (int r = 0; r < G; ++r) {
                                const T c = cs[2 * r], sn = cs[2 * r + 1], wr = w[r];
                                w[r] = c * wr - sn * l;
                                l = c * l + sn * wr;
                            }
#pragma unroll
                            for (int r = 0; r < G; ++r) Vd[tid * PV + r] = w[r];
                            D[tid * PD + jj] = l;
                        }
                        if (birth) Vd[tid * PV + na] = l;
                    }
                }
                wave_lds_sync();
            }
        }
        // 2. the bands: thread = row, its entries of the group's vectors in registers, every rotation of the table
        if (band && bt >= 0 && it > 0) {
            const int64_t g0 = (it - 1) * G;
            const T *tabr = tab + ((it - 1) & 1) * (W * G * 2);
            T v[G];
#pragma unroll
            for (int r = 0; r < G; ++r) v[r] = (live && g0 + r < m0) ? V[(g0 + r) * n + trow] : (T)0;
            for (int jj = 0; jj < wb; ++jj) {
                const int64_t act = m0 + cnt[jj] - g0;
                const int na = act < 0 ? 0 : (act > G ? G : (int)act);
                const bool birth = born[jj] != 0 && act >= 0 && act < G;
                if (na == 0 && !birth) continue;
                T l = Tt[bt * PT + jj];
                if (na > 0) {
                    T cs[2 * G];
#pragma unroll
                    for (int r = 0; r < G; ++r) { cs[2 * r] = tabr[(jj * G + r) * 2]; cs[2 * r + 1] = tabr[(jj * G + r) * 2 + 1]; }
#pragma unroll
                    for (int r = 0; r < G; ++r) {
                        const T c = cs[2 * r], sn = cs[2 * r + 1], wr = v[r];
                        v[r] = c * wr - sn * l;
                        l = c * l + sn * wr;
                    }
                    Tt[bt * PT + jj] = l;
                }
#pragma unroll
                for (int r = 0; r < G; ++r) if (birth && r == na) v[r] = l;
            }
            if (live) {
#pragma unroll
                for (int r = 0; r < G; ++r) if (g0 + r < mend) V[(g0 + r) * n + trow] = v[r];
            }
        }
        __syncthreads();
    }

    // the kept rows and columns, compacted
    if (!band) {
        for (int i = tid; i < wb * wb; i += NT) {
            const int r = i / wb, c = i - r * wb;
            if (c <= r && !born[r] && !born[c]) out[(c0 + r - m0 - cnt[r]) * ldo + (c0 + c - m0 - cnt[c])] = D[r * PD + c];
        }
    } else {
        for (int i = tid; i < R * W; i += NT) {
            const int r = i / W, c = i - r * W;
            if (tb0 + r < n && rowm[r] >= 0 && !born[c]) out[(tb0 + r - m0 - rowm[r]) * ldo + (c0 + c - m0 - cnt[c])] = Tt[r * PT + c];
        }
    }
}

// What no rotation touches -- row t < n, columns [0, min(t + 1, cols)) of L with cols <= idx[0] -- to its compacted row of out
// (the columns stay where they are).  DEL_COPY_ROWS rows a workgroup, as copy_lower_kernel; whole 16-byte vectors where both
// sides allow and the rest of the row one element at a time: nothing right of the diagonal is written.
constexpr int DEL_COPY_ROWS = 4;
template <typename T>
__global__ __launch_bounds__(256) void del_copy_rows_kernel(const T *__restrict__ L, int64_t ldl, int64_t n, const int64_t *__restrict__ idx,
                                                            int64_t k, int64_t cols, T *__restrict__ out, int64_t ldo, int aligned)
{
    constexpr int VEC = Vec<T>::N;
    typedef typename Vec<T>::type VT;
    const int tid = threadIdx.x;
    const int64_t t0 = (int64_t)blockIdx.x * DEL_COPY_ROWS, t1 = t0 + DEL_COPY_ROWS < n ? t0 + DEL_COPY_ROWS : n;
    for (int64_t t = t0; t < t1; ++t) {
        const int64_t m = removed_below(idx, k, t);
        if (m < k && idx[m] == t) continue;
        const T *__restrict__ s = L + t * ldl;
        T *__restrict__ d = out + (t - m) * ldo;
        const int64_t nc = t + 1 < cols ? t + 1 : cols, nv = aligned ? nc / VEC : 0;
        const VT *__restrict__ sv = reinterpret_cast<const VT *>(s);
        VT *__restrict__ dv = reinterpret_cast<VT *>(d);
        copy_vecs(sv, dv, nv);
        for (int64_t c = nv * VEC + tid; c < nc; c += 256) d[c] = s[c];
    }
}

// the kept points: row o of (x | y) from row o + #{q: idx[q] - q <= o} of the source; one thread per element
template <typename T>
__global__ __launch_bounds__(256) void del_gather_kernel(const T *__restrict__ x, const T *__restrict__ y, int64_t d, const int64_t *__restrict__ idx,
                                                         int64_t k, int64_t n_out, T *__restrict__ xo, T *__restrict__ yo)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_out * (d + 1)) return;
    const int64_t o = i / (d + 1), c = i - o * (d + 1);
    int64_t lo = 0, hi = k;                               // the first m with idx[m] - m > o  (idx[m] - m: kept rows before idx[m])
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (idx[mid] - mid <= o) lo = mid + 1; else hi = mid;
    }
    const int64_t t = o + lo;
    if (c < d) xo[o * d + c] = x[t * d + c];
    else yo[o] = y[t];
}

// this host thread's block for the indices on the device (k int64) and the vectors V (n x k in the dtype)
static thread_local ThreadScratch g_del_scr;

static int del_scratch(int dtype, int64_t n, const int64_t *idx_host, int64_t k, int64_t **idx_dev, void **V, hipStream_t st)
{
    const size_t ib = (size_t)round_up(k * 8, 16);
    void *p = nullptr;
    GPX_TRY(g_del_scr.get(ib + (size_t)n * k * esize(dtype), &p));
    GPX_HIP(hipMemcpyAsync(p, idx_host, (size_t)k * 8, hipMemcpyHostToDevice, st));
    GPX_HIP(hipStreamSynchronize(st));                     // idx_host may be reused on return
    *idx_dev = (int64_t *)p;
    *V = (char *)p + ib;
    return GPX_OK;
}

template <typename T>
static int chol_delete_t(const T *L, int64_t n, int64_t ldl, const int64_t *idx_host, const int64_t *idx_dev, int64_t k, T *V, T *out,
                         int64_t ldo, hipStream_t st)
{
    constexpr int64_t VEC = Vec<T>::N;
    const int64_t es = (int64_t)sizeof(T);
    const int64_t cfirst = idx_host[0] / DEL_W * DEL_W;    // the first block with anything to do; the columns before it are copied
    const bool src_al = ((uintptr_t)L) % 16 == 0 && ldl % VEC == 0;
    const bool both_al = src_al && ((uintptr_t)out) % 16 == 0 && ldo % VEC == 0;
    const bool large = k > DEL_G_SMALL;
    if (large) GPX_TRY(set_max_lds((const void *)del_block_kernel<T, DEL_G_LARGE>, del_lds_bytes<T, DEL_G_LARGE>()));
    else GPX_TRY(set_max_lds((const void *)del_block_kernel<T, DEL_G_SMALL>, del_lds_bytes<T, DEL_G_SMALL>()));
    // bytes of the launches below: L is read once, its kept part written, V read and written by the bands
    double bytes = 0.5 * ((double)n * (double)(n + 1) + (double)(n - k) * (double)(n - k + 1));
    {
        int64_t m = 0;
        for (int64_t c0 = cfirst; c0 < n; c0 += DEL_W) {
            const int64_t wb = std::min<int64_t>(DEL_W, n - c0), m_begin = m;
            while (m < k && idx_host[m] < c0 + wb) ++m;
            bytes += (double)(n - c0 - wb) * (double)(m_begin + m) + (double)wb * (double)m_begin;
        }
    }
    ProfScope prof(PC_CHOL_DELETE, bytes * (double)es, st);
    if (cfirst > 0) {
        hipLaunchKernelGGL((del_copy_rows_kernel<T>), dim3((unsigned)cdiv(n, DEL_COPY_ROWS)), dim3(256), 0, st, L, ldl, n, idx_dev, k, cfirst,
                           out, ldo, both_al ? 1 : 0);
        GPX_LAUNCH_CHECK();
    }
    int64_t m0 = 0;
    for (int64_t c0 = cfirst; c0 < n; c0 += DEL_W) {
        const int64_t wb = std::min<int64_t>(DEL_W, n - c0);
        const dim3 grid((unsigned)(1 + cdiv(n - c0 - wb, DEL_ROWS)));
        if (large)
            hipLaunchKernelGGL((del_block_kernel<T, DEL_G_LARGE>), grid, dim3(DEL_THREADS), (del_lds_bytes<T, DEL_G_LARGE>()), st, L, ldl, n, idx_dev, k,
                               m0, c0, (int)wb, V, out, ldo, src_al ? 1 : 0);
        else
            hipLaunchKernelGGL((del_block_kernel<T, DEL_G_SMALL>), grid, dim3(DEL_THREADS), (del_lds_bytes<T, DEL_G_SMALL>()), st, L, ldl, n, idx_dev, k,
                               m0, c0, (int)wb, V, out, ldo, src_al ? 1 : 0);
        GPX_LAUNCH_CHECK();
        while (m0 < k && idx_host[m0] < c0 + wb) ++m0;
    }
    return GPX_OK;
}

static int chol_delete_dev(int dtype, const void *L, int64_t n, int64_t ldl, const int64_t *idx_host, const int64_t *idx_dev, int64_t k,
                           void *V, void *out, int64_t ldo, hipStream_t st)
{
    return by_dtype(dtype, [&](auto t) { using T = decltype(t); return chol_delete_t<T>((const T *)L, n, ldl, idx_host, idx_dev, k, (T *)V, (T *)out, ldo, st); });
}

int chol_delete(int dtype, const void *L, int64_t n, int64_t ldl, const int64_t *idx_host, int64_t k, void *out, int64_t ldo, hipStream_t st)
{
    int64_t *idx_dev = nullptr;
    void *V = nullptr;
    GPX_TRY(del_scratch(dtype, n, idx_host, k, &idx_dev, &V, st));
    return chol_delete_dev(dtype, L, n, ldl, idx_host, idx_dev, k, V, out, ldo, st);
}

// 1 <= k < n sorted distinct indices in [0, n)
static bool del_indices_ok(const int64_t *idx, int64_t k, int64_t n)
{
    if (k < 1 || k >= n) return false;
    for (int64_t q = 0; q < k; ++q)
        if (idx[q] < 0 || idx[q] >= n || (q > 0 && idx[q] <= idx[q - 1])) return false;
    return true;
}

// ---- the handle ---------------------------------------------------------------------------------------------------------
static int remove_impl(gpx_gp *g, const int64_t *idx, int64_t k, gpx_gp_t **out, int *info)
{
    const int64_t n = g->n, n2 = n - k, d = g->d;
    GPX_TRY(gp_need_factor(g, "to remove points from"));
    route_hit(RT_REMOVE);
    gpx_gp_t *g2 = nullptr;
    GPX_TRY(gpx_gp_create(&g2, g->dtype, g->kernel, n2, g->d));
    struct Guard { gpx_gp_t *g; ~Guard() { if (g) gpx_gp_destroy(g); } } guard{g2};
    StreamTurn turn2(g2->st);                              // (this thread's scratch: the new handle's stream takes its turn)
    hipStream_t st = g2->st;
    GPX_TRY(order(g2->ev[5], g->st, st));                  // ... behind whatever the source's stream still holds
    int64_t *idx_dev = nullptr;
    void *V = nullptr;
    GPX_TRY(del_scratch(g->dtype, n, idx, k, &idx_dev, &V, st));
    // 1. the kept points, gathered on the device
    const dim3 grid((unsigned)cdiv(n2 * (d + 1), 256)), block(256);
    GPX_TRY(by_dtype(g->dtype, [&](auto t) {
        using T = decltype(t);
        hipLaunchKernelGGL((del_gather_kernel<T>), grid, block, 0, st, (const T *)g->x, (const T *)g->y, d, idx_dev, k, n2, (T *)g2->x, (T *)g2->y);
        GPX_LAUNCH_CHECK();
        return GPX_OK;
    }));
    memcpy(g2->params, g->params, sizeof(g->params));
    g2->s = g->s;
    g2->have_data = true; g2->have_params = g->have_params; g2->have_K = false;    // (a fit has consumed the source's K, if it had one)
    GPX_TRY(gp_rescale(g2));
    GPX_TRY(gp_scan_finite(g2));
    GPX_HIP(hipMemsetAsync(&g2->scal->info, 0, sizeof(int), st));                 // rotations cannot fail: the factor exists
    GPX_HIP(hipEventRecord(g2->ev[0], st));
    GPX_HIP(hipEventRecord(g2->ev[1], st));
    // 2. the factor without the k rows and columns, from the source's A into the new handle's
    GPX_TRY(chol_delete_dev(g->dtype, g->A, n, g->lda, idx, idx_dev, k, V, g2->A, g2->lda, st));
    GPX_HIP(hipEventRecord(g2->ev[2], st));
    // 3. the tail of gpx_gp_fit, both sweeps; the new factor's operators are built lazily
    g2->ops.invalidate();
    GPX_TRY(gp_finish_fit(g2, false, info));
    guard.g = nullptr;
    *out = g2;
    return GPX_OK;
}

}  // namespace gpx

using namespace gpx;

extern "C" {

int gpx_d_chol_delete(int dtype, const void *L, int64_t n, int64_t ldl, const int64_t *idx_host, int64_t k, void *out, int64_t ldo,
                      void *stream)
{
    gpx::tune_refresh();
    gpx::StreamTurn turn__((hipStream_t)stream);     // (this thread's scratch buffers: one stream at a time, gpx_mem.h)
    GPX_ARG(dtype == GPX_F64 || dtype == GPX_F32, "dtype must be GPX_F64 or GPX_F32");
    GPX_ARG(L && out && idx_host && L != out, "NULL pointer or out == L");
    GPX_ARG(n >= 2 && k >= 1 && k < n, "need 1 <= k < n");
    GPX_ARG(del_indices_ok(idx_host, k, n), "idx must hold sorted distinct indices in [0, n)");
    GPX_ARG(ldl >= n && ldo >= n - k, "leading dimension too small");
    GPX_TRY(ensure_device());
    return chol_delete(dtype, L, n, ldl, idx_host, k, out, ldo, S(stream));
}

int gpx_gp_remove(gpx_gp_t *g, const int64_t *idx, int64_t k, gpx_gp_t **out, int *info)
{
    if (out) *out = nullptr;
    GP_ENTER(g);
    GPX_ARG(out && info && idx, "NULL argument");
    GPX_ARG(g->fitted && g->have_data, "gp is not fitted");
    GPX_ARG(del_indices_ok(idx, k, g->n), "idx must hold 1 <= k < n sorted distinct indices in [0, n)");
    return remove_impl(g, idx, k, out, info);
}

}  // extern "C"
