// gpx_solve.hip -- triangular solves and O(n) reductions on the factor (gfx950).
//
// Replaces scipy.linalg.cho_solve((L, True), y) of gp/gp.py:332-334 (LAPACK
// dpotrs), np.linalg.slogdet(K) of gp/ext/gp_c.pyx:21 (a second, redundant LU in
// the reference; here 2*sum(log diag L)), np.dot(y, Kiy) of gp_c.pyx:26, and the
// explicit-inverse route to the posterior covariance (gp/gp.py:311-312,622-625).
//
// Roofline: HBM read bandwidth -- a single-right-hand-side solve reads the
// lower triangle of L once per direction (n^2/2 * sizeof(T) bytes, 2 n^2 flop for
// both directions together).  The 64 x 64 diagonal blocks are inverted up front in
// ONE batched launch (inv64_kernel); the solve then advances 512 columns per launch:
// trsv_fwd_fused / trsv_bwd_fused (steps), or trsv_op_kernel with per-block operators
// built once per factor ("operator form" below; who may use them: ops_usable).
// var_rows_kernel (the predictive variance's finishing pass) reads a solved m x n chunk once: rows n sizeof(T) bytes.
#include "gpx_small.h"
#include "gpx_kernels_dev.h"
#include "gpx_leaf.h"

namespace gpx {

constexpr int SB = 64;                 // the diagonal blocks that are inverted directly
constexpr int OB = TRSV_OPS_BLOCK;     // columns of an operator block ("operator form" below)

// ---- batched inverse of the 64 x 64 diagonal blocks --------------------------
// One 256-thread workgroup per block (all blocks in one launch): the register-resident 4 x 4-tile sweep of the
// factorisation's leaf in its "L is given" mode (gpx_leaf.h) carries X = inv(L_jj) -- 16 steps of two barriers,
// ~10 us per block however many there are (the earlier one-lane-per-column forward substitution through LDS took
// 69 us for the 128 blocks of n = 8192 and 1.16 ms for the 1024 of n = 65536).  Blocks shorter than 64 are
// padded with the identity.  Outputs (each optional): `out` W[blk][64][64] laid out for coalesced mat-vec
// reads, transposed != 0: out[i * 64 + c] = X[c][i] (forward sweep, z = X v), else out[i * 64 + c] = X[i][c]
// (backward, a = X^T v); W / Wt: the diagonal 64-blocks of the 512-block operators (X and X^T).
template <typename T>
__global__ __launch_bounds__(256) void inv64_kernel(const T *__restrict__ L, int64_t ldl, int64_t ncols,
                                                    T *__restrict__ out, int transposed, T *__restrict__ W,
                                                    T *__restrict__ Wt, int64_t bsL, int64_t bsOut)
{
    L += (int64_t)blockIdx.y * bsL;                  // batched: matrix blockIdx.y
    const int tid = threadIdx.x, tr = tid >> 4, tc = tid & 15;
    const int64_t k0 = (int64_t)blockIdx.x * SB;
    const int jb = (int)min((int64_t)SB, ncols - k0);
    const T *blk = L + k0 * ldl + k0;
    T a[4][4], x[4][4];
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const int row = 4 * tr + r, col = 4 * tc + c;
            T v = (row == col) ? (T)1 : (T)0;
            if (row < jb && col <= row) v = blk[(int64_t)row * ldl + col];
            a[r][c] = v;
            x[r][c] = (row == col) ? (T)1 : (T)0;
        }
    factor64<T, true, true>(a, x, jb, 0, nullptr);
    T *o = out ? out + (int64_t)blockIdx.y * bsOut + (int64_t)blockIdx.x * (SB * SB) : nullptr;
    const int64_t kb = blockIdx.x / (OB / SB), pp = blockIdx.x % (OB / SB);
    T *w = W ? W + kb * (int64_t)(OB * OB) + pp * SB * (OB + 1) : nullptr;
    T *wt = Wt ? Wt + kb * (int64_t)(OB * OB) + pp * SB * (OB + 1) : nullptr;
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const int row = 4 * tr + r, col = 4 * tc + c;
            const T v = (col <= row) ? x[r][c] : (T)0;
            if (o) o[transposed ? col * SB + row : row * SB + col] = v;
            if (w) { w[(int64_t)row * OB + col] = v; wt[(int64_t)col * OB + row] = v; }
        }
}

static thread_local ThreadScratch g_scr;        // the block inverses

// ---- fused block steps of the single-right-hand-side solves ----------------
// The solve advances in blocks of TB = 512 columns, ONE launch per block (the chain
// of dependent launches, not bandwidth, bounded the old 64-wide stepping: 2 x 1024
// launches of ~11 us at n = 65536).  In the launch that follows the solution of
// block p:
//   workgroup 0     applies block p to the rows (forward) / columns (backward) of
//                   the NEXT block only -- a TB x TB tile -- and then solves that
//                   block: 64-wide sub-steps, z = inv(L_ss) v by a 64 x 64 mat-vec
//                   with the precomputed inverse, right-looking update inside the
//                   block through LDS;
//   workgroups 1..  stream the rest of block p's panel (everything beyond the next
//                   block) against the same solution -- the HBM-bound part.
// Nothing a later block needs is ever produced by two workgroups of one launch, so
// launch order is the only synchronisation.
constexpr int TB = 512;
constexpr int TBT = 512;          // threads per workgroup
constexpr int TCH = TB / 128;     // 128-column chunks of a block row (2 per lane and chunk)

template <typename T>
__device__ __forceinline__ void load2(const T *p, bool aligned, T &v0, T &v1)
{
    if (aligned) {
        if constexpr (sizeof(T) == 8) {
            const double2 t = *reinterpret_cast<const double2 *>(p);
            v0 = t.x; v1 = t.y;
        } else {
            const float2 t = *reinterpret_cast<const float2 *>(p);
            v0 = t.x; v1 = t.y;
        }
    } else {
        v0 = p[0]; v1 = p[1];
    }
}

// sum over the 16 lanes of a DPP row, result in every lane of the row: two quad
// butterflies, then row_half_mirror and row_mirror (VALU only, no LDS traffic)
template <int CTRL> __device__ __forceinline__ double dpp_mov(double v)
{
    int lo = __double2loint(v), hi = __double2hiint(v);
    lo = __builtin_amdgcn_mov_dpp(lo, CTRL, 0xF, 0xF, true);
    hi = __builtin_amdgcn_mov_dpp(hi, CTRL, 0xF, 0xF, true);
    return __hiloint2double(hi, lo);
}
template <int CTRL> __device__ __forceinline__ float dpp_mov(float v)
{
    return __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(v), CTRL, 0xF, 0xF, true));
}
template <typename T> __device__ __forceinline__ T row16_sum(T v)
{
    v += dpp_mov<0xB1>(v);      // quad_perm [1,0,3,2]
    v += dpp_mov<0x4E>(v);      // quad_perm [2,3,0,1]
    v += dpp_mov<0x141>(v);     // row_half_mirror
    v += dpp_mov<0x140>(v);     // row_mirror
    return v;
}
template <typename T> __device__ __forceinline__ T lanes32_sum(T v)
{
    v = row16_sum(v);
    return v + __shfl_xor(v, 16, 64);
}
template <typename T> __device__ __forceinline__ T lanes64_sum(T v)
{
    v = lanes32_sum(v);
    return v + __shfl_xor(v, 32, 64);
}

// out[i] = sum_c L[r + i, p0 + c] * z[c], i < RU, for one wave: lane owns columns
// 128 j + 2 lane (+1); all RU * TCH loads are issued before the first use.
// FULL: the block has all TB columns (no column guards).
template <typename T, int RU, bool FULL>
__device__ __forceinline__ void rows_dot(const T *__restrict__ L, int64_t ldl, int64_t p0, int pjb,
                                         int64_t r, int64_t rlast, const T (&zr)[TCH][2], int lane,
                                         bool aligned, T (&out)[RU])
{
    T l[RU][TCH][2];
#pragma unroll
    for (int i = 0; i < RU; ++i) {
        const T *row = L + min(r + i, rlast) * ldl + p0;          // clamped: in bounds, result unused
#pragma unroll
        for (int j = 0; j < TCH; ++j) {
            const int c = j * 128 + 2 * lane;
            if (FULL) {
                load2(row + c, aligned, l[i][j][0], l[i][j][1]);
            } else {
                l[i][j][0] = (T)0; l[i][j][1] = (T)0;
                if (c + 1 < pjb) load2(row + c, aligned, l[i][j][0], l[i][j][1]);
                else if (c < pjb) l[i][j][0] = row[c];
            }
        }
    }
#pragma unroll
    for (int i = 0; i < RU; ++i) {
        T acc = (T)0;
#pragma unroll
        for (int j = 0; j < TCH; ++j) { acc = fma(l[i][j][0], zr[j][0], acc); acc = fma(l[i][j][1], zr[j][1], acc); }
        out[i] = lanes64_sum(acc);
    }
}

template <typename T> __device__ __forceinline__ T lanes8_sum(T v)
{
    v += dpp_mov<0xB1>(v);
    v += dpp_mov<0x4E>(v);
    v += dpp_mov<0x141>(v);
    return v;
}

// z = X v (forward) / a = X^T v (backward) for one 64-block by the whole workgroup:
// lane = output row, wave w sums columns 8 w .. 8 w + 7 (li = that slice of the stored
// inverse, already in registers), fixed-order reduction over the 8 waves.
template <typename T>
__device__ __forceinline__ void inv_matvec(const T (&li)[8], const T *sv_s, T *red, T *out64, T *xout,
                                           int nvalid, int tid, int lane, int wave)
{
    T acc = (T)0;
#pragma unroll
    for (int cc = 0; cc < 8; ++cc) acc = fma(li[cc], sv_s[wave * 8 + cc], acc);
    red[wave * SB + lane] = acc;
    __syncthreads();
    if (tid < SB) {
        T z = red[tid];
#pragma unroll
        for (int q = 1; q < 8; ++q) z += red[q * SB + tid];
        out64[tid] = z;
        if (tid < nvalid) xout[tid] = z;
    }
    __syncthreads();
}

// far part of the forward sweep: apply the solved block [p0, p0 + pjb) to 64 rows starting at
// far0 + 64 * slab:  b[r] -= L[r, p0:p0+pjb] . x[p0:p0+pjb]   (whole workgroup of TBT threads; szp: TB + 2 of LDS)
template <typename T>
__device__ __forceinline__ void far_fwd(const T *__restrict__ L, int64_t ldl, T *__restrict__ b,
                                        const T *__restrict__ x, int64_t n, int64_t p0, int pjb, int64_t far0,
                                        int slab, bool aligned, T *szp)
{
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (int i = tid; i < TB + 2; i += TBT) szp[i] = (i < pjb) ? x[p0 + i] : (T)0;
    __syncthreads();
    T zr[TCH][2];
#pragma unroll
    for (int j = 0; j < TCH; ++j) { zr[j][0] = szp[j * 128 + 2 * lane]; zr[j][1] = szp[j * 128 + 2 * lane + 1]; }
    const int64_t rbeg = far0 + (int64_t)slab * 64, rend = min(n, rbeg + 64);
    constexpr int RU = 8;
    for (int64_t r = rbeg + wave * RU; r < rend; r += (TBT / 64) * RU) {
        T acc[RU];
        if (pjb == TB) rows_dot<T, RU, true>(L, ldl, p0, pjb, r, rend - 1, zr, lane, aligned, acc);
        else rows_dot<T, RU, false>(L, ldl, p0, pjb, r, rend - 1, zr, lane, aligned, acc);
        if (lane < RU && r + lane < rend) {
            T mine = acc[0];
#pragma unroll
            for (int i = 1; i < RU; ++i) mine = (lane == i) ? acc[i] : mine;
            b[r + lane] -= mine;
        }
    }
}

// forward.  x[p0:p0+pjb] (block p) is final.  Workgroup 0 solves block [k0, k0+jb)
// from b (nothing when jb == 0); workgroups w >= 1 apply block p to 64 rows each of
// [far0, n):  b[r] -= L[r, p0:p0+pjb] . x[p0:p0+pjb].
template <typename T>
__global__ __launch_bounds__(TBT) void trsv_fwd_fused(const T *__restrict__ L, int64_t ldl,
                                                      const T *__restrict__ Linv, T *__restrict__ b,
                                                      T *__restrict__ x, int64_t n, int64_t k0, int jb,
                                                      int64_t p0, int pjb, int64_t far0, int aligned_i,
                                                      int64_t bsL, int64_t bsLinv, int64_t bsv)
{
    L += (int64_t)blockIdx.y * bsL; Linv += (int64_t)blockIdx.y * bsLinv;    // batched: system blockIdx.y
    b += (int64_t)blockIdx.y * bsv; x += (int64_t)blockIdx.y * bsv;
    __shared__ T szp[TB + 2];       // far workgroups: solution of block p, zero padded
    __shared__ T sv[TB];            // workgroup 0: right-hand side of the block being solved
    __shared__ T szb[TB];           // workgroup 0: solution of the block so far
    __shared__ T red[8 * SB];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const bool aligned = aligned_i != 0;

    if (blockIdx.x != 0) {
        if (pjb <= 0) return;
        far_fwd<T>(L, ldl, b, x, n, p0, pjb, far0, (int)blockIdx.x - 1, aligned, szp);
        return;
    }
    if (jb == 0) return;

    // in-block chain, LEFT-looking over 64-wide sub-blocks: sub-block s subtracts
    // L[rows of s, columns 0 .. 64 s) . z[0 .. 64 s) -- 8 lanes per row, a lane takes 2 of
    // every 16 columns, so each row is read as whole 128-byte lines -- and then forms
    // z_s = inv(L_ss) v_s.  The row block of sub-step s+1 and its inverse are requested as
    // soon as the registers of sub-step s are consumed, ahead of the mat-vec and its barriers.
    constexpr int CG = TB / SB - 1;                     // 7 groups of 4 loads at most
    const int ns = (jb + SB - 1) / SB;
    const int row = tid >> 3, j8 = tid & 7;
    const T *Lblk = L + k0 * ldl + k0;
    const T *Li0 = Linv + (k0 >> 6) * (int64_t)(SB * SB);
    for (int i = tid; i < TB; i += TBT) sv[i] = (i < jb) ? b[k0 + i] : (T)0;
    T li[8], ln[8];
#pragma unroll
    for (int cc = 0; cc < 8; ++cc) li[cc] = Li0[(wave * 8 + cc) * SB + lane];
    T l0[CG][4], l1[CG][4];
    __syncthreads();
    for (int s = 0; s < ns; ++s) {
        if (s > 0) {
            T acc = (T)0;
#pragma unroll
            for (int t = 0; t < CG; ++t) {
                if (t < s) {
#pragma unroll
                    for (int m = 0; m < 4; ++m) {
                        const int c = t * SB + m * 16 + 2 * j8;
                        acc = fma(l0[t][m], szb[c], acc);
                        acc = fma(l1[t][m], szb[c + 1], acc);
                    }
                }
            }
            acc = lanes8_sum(acc);
            if (j8 == 0 && s * SB + row < jb) sv[s * SB + row] -= acc;
        }
        if (s + 1 < ns) {
            const T *Li = Li0 + (s + 1) * (int64_t)(SB * SB);
#pragma unroll
            for (int cc = 0; cc < 8; ++cc) ln[cc] = Li[(wave * 8 + cc) * SB + lane];
            const T *rp = Lblk + (int64_t)min((s + 1) * SB + row, jb - 1) * ldl + 2 * j8;
#pragma unroll
            for (int t = 0; t < CG; ++t) {
                if (t <= s) {
#pragma unroll
                    for (int m = 0; m < 4; ++m) load2(rp + t * SB + m * 16, aligned, l0[t][m], l1[t][m]);
                }
            }
        }
        __syncthreads();
        inv_matvec(li, sv + s * SB, red, szb + s * SB, x + k0 + s * SB, jb - s * SB, tid, lane, wave);
#pragma unroll
        for (int cc = 0; cc < 8; ++cc) li[cc] = ln[cc];
    }
}

// far part of the backward sweep: apply the solved row block [q0, q0 + qjb) to CW columns starting at
// c0 + CW * slab:  b[c] -= L[q0:q0+qjb, c] . x[q0:q0+qjb]   (sa: TB, red: 2 * TB of LDS)
template <typename T, int CW>
__device__ __forceinline__ void far_bwd(const T *__restrict__ L, int64_t ldl, T *__restrict__ b,
                                        const T *__restrict__ x, int64_t q0, int qjb, int64_t c0, int64_t c1,
                                        int slab, bool aligned, T *sa, T *red)
{
    const int tid = threadIdx.x;
        constexpr int LP = CW / 2;                  // lanes (column pairs) per row
        constexpr int NG = TBT / LP;                // row groups
        constexpr int PER = TB / NG;                // rows per thread
        constexpr int BU = PER < 32 ? PER : 32;     // loads in flight per thread and batch
        for (int i = tid; i < TB; i += TBT) sa[i] = (i < qjb) ? x[q0 + i] : (T)0;
        __syncthreads();
        const int64_t cbeg = c0 + (int64_t)slab * CW, cend = min(c1, cbeg + CW);
        const int lp = tid % LP, g = tid / LP;
        const int64_t c = min(cbeg + 2 * lp, cend - 1);
        const bool pair = c + 1 < cend;
        const T *col = L + q0 * ldl + c;
        T a0 = (T)0, a1 = (T)0;
#pragma unroll 1
        for (int u0 = 0; u0 < PER; u0 += BU) {
            T l0[BU], l1[BU];
#pragma unroll
            for (int u = 0; u < BU; ++u) {
                const int i = min(g + (u0 + u) * NG, qjb - 1);
                if (pair) load2(col + (int64_t)i * ldl, aligned, l0[u], l1[u]);
                else { l0[u] = col[(int64_t)i * ldl]; l1[u] = (T)0; }
            }
#pragma unroll
            for (int u = 0; u < BU; ++u) {
                const int i = g + (u0 + u) * NG;
                const T av = (i < qjb) ? sa[i] : (T)0;
                a0 = fma(l0[u], av, a0);
                a1 = fma(l1[u], av, a1);
            }
        }
        red[g * CW + 2 * lp] = a0;
        red[g * CW + 2 * lp + 1] = a1;
        __syncthreads();
        if (tid < CW && cbeg + tid < cend) {
            T sum = red[tid];
            for (int q = 1; q < NG; ++q) sum += red[q * CW + tid];
            b[cbeg + tid] -= sum;
        }
}

// backward (L^T a = v).  x[q0:q0+qjb] (block q, below the block being solved) is final.
// Workgroup 0 solves block [k0, k0+jb) from b (nothing when jb == 0); workgroups
// w >= 1 apply block q to CW columns each of [c0, c1):  b[c] -= L[q0:q0+qjb, c] . x[q0:q0+qjb].
// CW = 128 for the streaming far part (1 KiB per row and wave), 32 for the 512 x 512 tile
// next to the diagonal (16 workgroups instead of 4).
template <typename T, int CW>
__global__ __launch_bounds__(TBT) void trsv_bwd_fused(const T *__restrict__ L, int64_t ldl,
                                                      const T *__restrict__ Linv, T *__restrict__ b,
                                                      T *__restrict__ x, int64_t k0, int jb, int64_t q0,
                                                      int qjb, int64_t c0, int64_t c1, int aligned_i,
                                                      int64_t bsL, int64_t bsLinv, int64_t bsv)
{
    L += (int64_t)blockIdx.y * bsL; Linv += (int64_t)blockIdx.y * bsLinv;
    b += (int64_t)blockIdx.y * bsv; x += (int64_t)blockIdx.y * bsv;
    __shared__ T sa[TB];            // far workgroups: solution of block q
    __shared__ T sv[TB];
    __shared__ T sz[SB];
    __shared__ T red[2 * TB];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const bool aligned = aligned_i != 0;

    if (blockIdx.x != 0) {
        if (qjb <= 0) return;
        far_bwd<T, CW>(L, ldl, b, x, q0, qjb, c0, c1, (int)blockIdx.x - 1, aligned, sa, red);
        return;
    }
    if (jb == 0) return;

    // in-block chain, last sub-block first, right-looking: after a_s = inv(L_ss)^T v_s the
    // rows of sub-block s update every column to their left (thread = column pair, two
    // groups of 32 rows: whole rows are read contiguously).  The tile of a sub-step is
    // requested before the mat-vec that produces its multipliers.
    const int ns = (jb + SB - 1) / SB;
    const int cpair = tid & 255, g = tid >> 8;
    const T *Li0 = Linv + (k0 >> 6) * (int64_t)(SB * SB);
    for (int i = tid; i < TB; i += TBT) sv[i] = (i < jb) ? b[k0 + i] : (T)0;
    T li[8];
    __syncthreads();
    for (int s = ns - 1; s >= 0; --s) {
        const T *Li = Li0 + s * (int64_t)(SB * SB);
        const int ncol = s * SB;
        const int ilim = min(SB, jb - s * SB);
#pragma unroll
        for (int cc = 0; cc < 8; ++cc) li[cc] = Li[(wave * 8 + cc) * SB + lane];
        T l0[32], l1[32];
        const bool act = 2 * cpair < ncol;       // ncol is a multiple of 64: always a pair
        if (act) {
            const T *col = L + (k0 + s * SB) * ldl + k0 + 2 * cpair;
#pragma unroll
            for (int u = 0; u < 32; ++u) {
                const int i = min(g * 32 + u, ilim - 1);
                load2(col + (int64_t)i * ldl, aligned, l0[u], l1[u]);
            }
        }
        inv_matvec(li, sv + s * SB, red, sz, x + k0 + s * SB, jb - s * SB, tid, lane, wave);
        if (ncol > 0) {
            T a0 = (T)0, a1 = (T)0;
            if (act) {
#pragma unroll
                for (int u = 0; u < 32; ++u) {
                    const int i = g * 32 + u;
                    const T av = (i < ilim) ? sz[i] : (T)0;     // rows >= ilim: identity padding, unused
                    a0 = fma(l0[u], av, a0);
                    a1 = fma(l1[u], av, a1);
                }
            }
            red[g * TB + 2 * cpair] = a0;
            red[g * TB + 2 * cpair + 1] = a1;
            __syncthreads();
            if (tid < ncol) sv[tid] -= red[tid] + red[TB + tid];
            __syncthreads();
        }
    }
}

// ---- operator form of the block steps ---------------------------------------------------------------
// The sweep above needs two dependent launches per 512-column block: the near tile (previous block's solution
// into this block's rows) and the in-block chain (8 sub-steps of a 64-wide mat-vec by ONE workgroup, 19 - 31 us:
// at n = 8192 that chain, not bandwidth, is the whole solve).  With per-block operators, precomputed once per
// factor on the MFMA kernel,
//     W_k  = inv(L_kk)             (512 x 512, from the 64 x 64 inverses by recursive doubling, batched over k)
//     Tf_k = W_k L_{k,k-1}         forward :  x_k = W_k  w_k - Tf_k x_{k-1}
//     Tb_k = W_k^T L_{k+1,k}^T     backward:  a_k = W_k^T z_k - Tb_k a_{k+1}
// a block step is ONE launch with no dependency inside it: 32 workgroups do the two 512-wide mat-vecs of block k
// (16 rows each, 32 lanes per row, whole 128-byte lines), all others stream the far panel of the neighbour block
// exactly as before.  w_k / z_k already hold every far contribution (blocks two or more away were streamed by
// earlier launches); the neighbour's contribution comes through Tf / Tb.  A ragged last block (n % 512) keeps
// the old kernels.  Cost of the operators: 2 (n / 512) products of 512^3 + the doubling, ~1.3 ms at n = 65536.
// LT_k[j][m] = L[(OB k + m), OB (k - 1) + j]   for k = 1 .. nfull - 1  (grid: (OB / 64)^2 tiles, k - 1)
template <typename T>
__global__ __launch_bounds__(256) void transpose_subdiag_kernel(const T *__restrict__ L, int64_t ldl, T *__restrict__ LT)
{
    __shared__ T tile[64][65];
    const int64_t k = blockIdx.y + 1;
    const int tm = blockIdx.x >> 3, tj = blockIdx.x & 7;            // tile of rows m (of L), columns j
    const T *src = L + (k * OB + tm * 64) * ldl + (k - 1) * OB + tj * 64;
    for (int idx = threadIdx.x; idx < 64 * 64; idx += 256) {
        const int r = idx >> 6, c = idx & 63;
        tile[r][c] = src[(int64_t)r * ldl + c];
    }
    __syncthreads();
    T *dst = LT + k * (int64_t)(OB * OB) + (int64_t)(tj * 64) * OB + tm * 64;
    for (int idx = threadIdx.x; idx < 64 * 64; idx += 256) {
        const int r = idx >> 6, c = idx & 63;
        dst[(int64_t)r * OB + c] = tile[c][r];
    }
}

// one block step: workgroups [0, nchain) solve block k (rows k0 ..), the others stream the neighbour's far panel.
// OPL = 32 lanes per row: 16 rows a workgroup, 32 workgroups a block -- a workgroup streams 128 KB of operators (with 8
// lanes a row and 8 workgroups it was 512: the block's two mat-vecs are bound by what ONE CU can pull)
constexpr int OPL = 32;
template <typename T, bool FWD>
__global__ __launch_bounds__(TBT) void trsv_op_kernel(const T *__restrict__ Wk, const T *__restrict__ Tk,
                                                      const T *__restrict__ L, int64_t ldl, T *__restrict__ rhs,
                                                      T *__restrict__ x, int64_t n, int64_t k0, int64_t p0, int pjb,
                                                      int64_t f0, int64_t f1, int nchain, int aligned_i)
{
    __shared__ T szp[TB + 2];
    __shared__ T sv[TB];
    __shared__ T red[2 * TB];
    const int tid = threadIdx.x;
    const bool aligned = aligned_i != 0;
    if ((int)blockIdx.x >= nchain) {
        if (pjb <= 0) return;
        if (FWD) far_fwd<T>(L, ldl, rhs, x, n, p0, pjb, f0, (int)blockIdx.x - nchain, aligned, szp);
        else far_bwd<T, 128>(L, ldl, rhs, x, p0, pjb, f0, f1, (int)blockIdx.x - nchain, aligned, szp, red);
        return;
    }
    for (int i = tid; i < TB; i += TBT) {
        sv[i] = rhs[k0 + i];
        szp[i] = (Tk && i < pjb) ? x[p0 + i] : (T)0;
    }
    __syncthreads();
    constexpr int ROWS = TBT / OPL;                   // rows per workgroup
    const int r = tid / OPL, part = tid % OPL;
    const int row = ROWS * (int)blockIdx.x + r;
    const T *wrow = Wk + (int64_t)row * OB, *trow = Tk ? Tk + (int64_t)row * OB : nullptr;
    T acc = (T)0;
    // branch-free on purpose (the zero half of the triangular W_k is read too): with a per-row triangle test
    // the loads cannot be batched and every iteration pays a memory round trip (measured 30 us instead of 8)
    if (trow) {
#pragma unroll 8
        for (int i = 0; i < OB / (2 * OPL); ++i) {
            const int c = 2 * OPL * i + 2 * part;
            T w0, w1, t0, t1;
            load2(wrow + c, true, w0, w1);
            load2(trow + c, true, t0, t1);
            acc = fma(w0, sv[c], acc);
            acc = fma(w1, sv[c + 1], acc);
            acc = fma(-t0, szp[c], acc);
            acc = fma(-t1, szp[c + 1], acc);
        }
    } else {
#pragma unroll 8
        for (int i = 0; i < OB / (2 * OPL); ++i) {
            const int c = 2 * OPL * i + 2 * part;
            T w0, w1;
            load2(wrow + c, true, w0, w1);
            acc = fma(w0, sv[c], acc);
            acc = fma(w1, sv[c + 1], acc);
        }
    }
    acc = lanes32_sum(acc);
    if (part == 0) x[k0 + row] = acc;
}

static thread_local ThreadScratch g_ops;        // home of the operators when the caller brings no cache of its own

// The operator buffer of a factor with nfull = n / OB full blocks: five runs of nfull blocks of OB x OB elements,
//     W_k | Wt_k = W_k^T | P_k (work space of the build; L_{k,k-1}^T in the end) | Tf_k | Tb_k,
// then TAIL elements a block that nothing reads (the size of that block's 64 x 64 inverses, which live in g_scr) and
// 256 bytes.  bytes() is what fit_batch_grad sizes its groups from and what the multi-GPU handle reserves per panel:
// it stays as it is until the tail is dropped in a change of its own.
template <typename T>
struct OpsView {
    static constexpr int64_t BS = (int64_t)OB * OB, TAIL = (int64_t)(OB / SB) * SB * SB;
    T *base; int64_t nfull;
    OpsView(const void *buf, int64_t n) : base((T *)buf), nfull(n / OB) {}
    T *run(int r, int64_t k) const { return base + (r * nfull + k) * BS; }
    T *W(int64_t k) const { return run(0, k); }
    T *Wt(int64_t k) const { return run(1, k); }
    T *P(int64_t k) const { return run(2, k); }
    T *Tf(int64_t k) const { return run(3, k); }
    T *Tb(int64_t k) const { return run(4, k); }
    static size_t bytes(int64_t n) { return (size_t)((n / OB) * (5 * BS + TAIL)) * sizeof(T) + 256; }
};

size_t trsv_ops_bytes(int dtype, int64_t n) { return dtype == GPX_F64 ? OpsView<double>::bytes(n) : OpsView<float>::bytes(n); }

// build W, Wt, Tf, Tb of the blocks [kbeg, kend) of L into `buf` (trsv_ops_bytes): everything is batched over the
// blocks of the range with the pointers moved to its first block.  Block k needs L_kk, L_{k,k-1} and L_{k+1,k}: block
// columns <= k of the factor.  kbeg = 0 also clears the triangular operators' zero halves for ALL blocks, so ranges go
// out in increasing order.
template <typename T>
static int trsv_ops_prepare(const T *L, int64_t n, int64_t ldl, void *buf, hipStream_t st, int64_t kbeg = 0, int64_t kend = -1)
{
    constexpr int dtype = sizeof(T) == 8 ? GPX_F64 : GPX_F32;
    const OpsView<T> V(buf, n);
    const int64_t nfull = V.nfull, rag = n - nfull * OB, BS = V.BS;
    if (kend < 0 || kend > nfull) kend = nfull;
    const int64_t cnt = kend - kbeg;
    if (kbeg == 0) GPX_HIP(hipMemsetAsync(V.W(0), 0, (size_t)(V.P(0) - V.W(0)) * sizeof(T), st));   // every W and Wt
    if (cnt <= 0) return GPX_OK;
    const int64_t dLk = (int64_t)OB * (ldl + 1);                     // L_kk -> L_{k+1,k+1}
    const T *Lk = L + kbeg * dLk;
    T *Wk = V.W(kbeg), *Wtk = V.Wt(kbeg), *Pk = V.P(kbeg);
    hipLaunchKernelGGL((inv64_kernel<T>), dim3((unsigned)(cnt * (OB / SB))), dim3(256), 0, st, Lk, ldl, cnt * OB, (T *)nullptr, 0,
                       Wk, Wtk, (int64_t)0, (int64_t)0);
    GPX_LAUNCH_CHECK();
    for (int64_t s2 = SB; s2 < OB; s2 *= 2) {
        Batch b;
        b.count = (int)cnt; b.count2 = (int)(OB / (2 * s2));
        const int64_t tW = 2 * s2 * OB + 2 * s2, tL = 2 * s2 * ldl + 2 * s2;
        // Pt = W11^T L21^T
        b.sA = BS; b.sB = dLk; b.sC = BS; b.tA = tW; b.tB = tL; b.tC = tW;
        GPX_TRY(gemm_nt(dtype, s2, s2, s2, Wtk, OB, Lk + s2 * ldl, ldl, Pk, OB, 1.0, GPX_FULL, 0, 0, st, 1, 0, &b));
        // W21 = -W22 Pt^T
        b.sA = BS; b.sB = BS; b.sC = BS; b.tA = tW; b.tB = tW; b.tC = tW;
        GPX_TRY(gemm_nt(dtype, s2, s2, s2, Wk + s2 * OB + s2, OB, Pk, OB, Wk + s2 * OB, OB, -1.0, GPX_FULL, 0, 0, st, 1, 0, &b));
        // (W^T)12 = -Pt W22^T
        GPX_TRY(gemm_nt(dtype, s2, s2, s2, Pk, OB, Wk + s2 * OB + s2, OB, Wtk + s2, OB, -1.0, GPX_FULL, 0, 0, st, 1, 0, &b));
    }
    const int64_t ka = std::max<int64_t>(kbeg, 1);                   // Tf_k = W_k L_{k,k-1} = W_k LT_k^T,  k = ka .. kend - 1
    if (kend > ka) {
        // (the transpose kernel numbers its blocks from 1 relative to the base it is given)
        hipLaunchKernelGGL((transpose_subdiag_kernel<T>), dim3((OB / SB) * (OB / SB), (unsigned)(kend - ka)), dim3(256), 0, st,
                           L + (ka - 1) * dLk, ldl, V.P(ka - 1));
        GPX_LAUNCH_CHECK();
        Batch b;
        b.count = (int)(kend - ka);
        b.sA = BS; b.sB = BS; b.sC = BS;
        GPX_TRY(gemm_nt(dtype, OB, OB, OB, V.W(ka), OB, V.P(ka), OB, V.Tf(ka), OB, 1.0, GPX_FULL, 0, 0, st, 1, 0, &b));
    }
    const int64_t kb_end = std::min(kend, nfull - 1);                // Tb_k = W_k^T L_{k+1,k}^T,  k = kbeg .. kb_end - 1
    if (kb_end > kbeg) {
        Batch b;
        b.count = (int)(kb_end - kbeg);
        b.sA = BS; b.sB = dLk; b.sC = BS;
        GPX_TRY(gemm_nt(dtype, OB, OB, OB, Wtk, OB, Lk + (int64_t)OB * ldl, ldl, V.Tb(kbeg), OB, 1.0, GPX_FULL, 0, 0, st, 1, 0, &b));
    }
    if (rag > 0 && kend == nfull) {                                  // the last full block against the ragged one
        T *tb = V.Tb(nfull - 1);
        GPX_HIP(hipMemsetAsync(tb, 0, (size_t)BS * sizeof(T), st));
        GPX_TRY(gemm_nt(dtype, OB, rag, OB, V.Wt(nfull - 1), OB, L + nfull * OB * ldl + (nfull - 1) * OB, ldl, tb, OB,
                        1.0, GPX_FULL, 0, 0, st, 1, 0));
    }
    return GPX_OK;
}

// ---- who may use the operators: two tests, and what each caller asks on top of them --------------------
//   ops_usable(dtype, L, ldl)   GPX_TRSV_OPS on, L on a 16-byte boundary, ldl % (16 / es) == 0
//   trsv_ops_whole_blocks(n)    n % OB == 0 and n >= OB   (gpx_common.h)
//   trsv_ops_build        usable, whole blocks (n == OB too: the multi-GPU fit's 512-wide panels)
//   trsv_ops_ahead_ok     usable, whole blocks, n >= 2 OB   (gpx_gp_fit, trsv_ops_build_upto)
//   trsm_ops_ok           trsv_ops_ahead_ok, GPX_TRSM_OPS on; trsm_right_lt: + the factor's TrsvOps, X and ldx as L and ldl
//   trsv_t, operators     usable, one square system; n >= trsv_ops_min_n() -- ANY such n, the last block may be ragged --
//                         or the caller's operators are complete (whole blocks)
//   trsv_t, mixed         usable, one square system, backward; the caller's operators cover 0 < built leading blocks
// The 16-byte pair implies the step kernels' `aligned` (L % (2 es) == 0, ldl % 2 == 0: two elements in one load), so the
// operator sweeps pass aligned = 1:
static bool ops_usable(int dtype, const void *L, int64_t ldl)
{
    static_assert(16 % (2 * sizeof(double)) == 0 && 16 % (2 * sizeof(float)) == 0, "16 is a multiple of 2 es");
    static_assert((16 / sizeof(double)) % 2 == 0 && (16 / sizeof(float)) % 2 == 0, "16 / es is even");
    return tune().trsv_ops != 0 && ((uintptr_t)L) % 16 == 0 && ldl % (16 / (int64_t)esize(dtype)) == 0;
}
// below this the ~0.7 ms of operator products (11 under-filled launches) costs what the shorter steps save
// (n = 8192: 1.17 vs 1.10 ms for both sweeps; n = 16384: 1.78 vs 2.49; n = 65536: 9.7 vs 12.1)
static int64_t trsv_ops_min_n() { return std::max<int64_t>(2 * OB, tune().trsv_ops_min); }
bool trsv_ops_ahead_ok(int dtype, const void *L, int64_t n, int64_t ldl) { return n >= 2 * OB && trsv_ops_whole_blocks(n) && ops_usable(dtype, L, ldl); }
bool trsm_ops_ok(int dtype, const void *L, int64_t n, int64_t ldl) { return trsv_ops_ahead_ok(dtype, L, n, ldl) && tune().trsm_ops != 0; }

// ---- the sweeps: what the launches of one solve share -----------------------------------------------------
template <typename T>
struct Sweep {
    const T *L; int64_t n, ldl, ncols; T *b, *x; hipStream_t st;
    unsigned nbt; int64_t sL, sv;      // systems solved by the same launches; strides of L, of b and x
    T *Linv; int64_t sLinv;            // the 64 x 64 inverses of the diagonal (g_scr), stride per system
    int aligned;                       // step kernels: two elements in one load
    int64_t nb() const { return cdiv(ncols, TB); }
    int width(int64_t blk) const { return (int)std::min<int64_t>(TB, ncols - blk * TB); }
};

// the inverses of the diagonal 64-blocks from `first` on, laid out for the forward (transposed = 1) / backward sweep
template <typename T>
static void inv64_blocks(const Sweep<T> &S, int64_t first, int transposed)
{
    hipLaunchKernelGGL((inv64_kernel<T>), dim3((unsigned)(cdiv(S.ncols, SB) - first), S.nbt), dim3(256), 0, S.st,
                       S.L + first * SB * (S.ldl + 1), S.ldl, S.ncols - first * SB, S.Linv + first * SB * SB, transposed,
                       (T *)nullptr, (T *)nullptr, S.sL, S.sLinv);
}

// Step sweeps over the blocks [kfirst, nb).  Per block two launches: (N) the 512 x 512 tile that carries the previous
// block's solution into this block's rows/columns, spread over 8-16 workgroups; (F) workgroup 0 solves the block while
// the other workgroups stream the previous block's far panel.
template <typename T>
static void steps_fwd(const Sweep<T> &S, int64_t kfirst)
{
    const int64_t n = S.n, nb = S.nb();
    auto launch = [&](int64_t far_rows, int64_t nn, int64_t k0, int jb, int64_t p0, int pjb, int64_t far0) {
        hipLaunchKernelGGL((trsv_fwd_fused<T>), dim3((unsigned)(1 + cdiv(far_rows, 64)), S.nbt), dim3(TBT), 0, S.st, S.L, S.ldl,
                           S.Linv, S.b, S.x, nn, k0, jb, p0, pjb, far0, S.aligned, S.sL, S.sLinv, S.sv);
    };
    for (int64_t blk = kfirst; blk < nb; ++blk) {
        const int64_t k0 = blk * TB, p0 = std::max<int64_t>(blk - 1, 0) * TB;
        const int jb = S.width(blk), pjb = blk > 0 ? TB : 0;
        if (blk > 0) launch(jb, k0 + jb, k0, 0, p0, pjb, k0);                               // (N)
        launch(blk > 0 ? n - (k0 + jb) : 0, n, k0, jb, p0, pjb, k0 + jb);                   // (F)
    }
    // trapezoid: the last block's panel below the triangle
    if (n > S.ncols) launch(n - S.ncols, n, S.ncols, 0, (nb - 1) * TB, S.width(nb - 1), S.ncols);
}

template <typename T>
static void steps_bwd(const Sweep<T> &S, int64_t kfirst)
{
    const int64_t nb = S.nb();
    for (int64_t blk = nb - 1; blk >= kfirst; --blk) {
        const int64_t k0 = blk * TB, q0 = k0 + TB;
        const int jb = S.width(blk), qjb = blk + 1 < nb ? S.width(blk + 1) : 0;
        if (qjb > 0)
            hipLaunchKernelGGL((trsv_bwd_fused<T, 32>), dim3((unsigned)(1 + cdiv(jb, 32)), S.nbt), dim3(TBT), 0, S.st, S.L,
                               S.ldl, S.Linv, S.b, S.x, k0, 0, q0, qjb, k0, k0 + jb, S.aligned, S.sL, S.sLinv, S.sv);
        hipLaunchKernelGGL((trsv_bwd_fused<T, 128>), dim3((unsigned)(1 + (qjb > 0 ? cdiv(k0, 128) : 0)), S.nbt),
                           dim3(TBT), 0, S.st, S.L, S.ldl, S.Linv, S.b, S.x, k0, jb, q0, qjb, (int64_t)0, k0, S.aligned,
                           S.sL, S.sLinv, S.sv);
    }
}

// Operator sweeps (one system, square): one launch per full block.  A ragged last block is left to the step sweeps.
constexpr int NCH = OB / (TBT / OPL);      // chain workgroups of a block

template <typename T>
static void ops_fwd(const Sweep<T> &S, const OpsView<T> &V)
{
    for (int64_t k = 0; k < V.nfull; ++k) {
        const int64_t k0 = k * OB, far0 = k0 + OB;
        const int64_t nfar = k > 0 ? cdiv(S.n - far0, 64) : 0;
        hipLaunchKernelGGL((trsv_op_kernel<T, true>), dim3((unsigned)(NCH + nfar)), dim3(TBT), 0, S.st, V.W(k),
                           k > 0 ? V.Tf(k) : (const T *)nullptr, S.L, S.ldl, S.b, S.x, S.n, k0, k0 - OB, k > 0 ? OB : 0, far0, S.n, NCH, 1);
    }
}

// blocks kend - 1 .. 0; block kend (steps, or the ragged one) is solved already
template <typename T>
static void ops_bwd(const Sweep<T> &S, const OpsView<T> &V, int64_t kend)
{
    for (int64_t k = kend - 1; k >= 0; --k) {
        const int64_t k0 = k * OB, q0 = k0 + OB;
        const int qjb = (k + 1 < V.nfull) ? OB : (int)(S.n - q0);
        const int64_t nfar = qjb > 0 ? cdiv(k0, 128) : 0;
        hipLaunchKernelGGL((trsv_op_kernel<T, false>), dim3((unsigned)(NCH + nfar)), dim3(TBT), 0, S.st, V.Wt(k),
                           qjb > 0 ? V.Tb(k) : (const T *)nullptr, S.L, S.ldl, S.b, S.x, S.n, k0, q0, qjb, (int64_t)0, k0, NCH, 1);
    }
}

template <typename T>
static int trsv_t(const T *L, int64_t n, int64_t ldl, T *b, T *x, int transpose, hipStream_t st,
                  int64_t ncols = -1, const Batch *bt = nullptr, TrsvOps *ops = nullptr)
{
    constexpr int dtype = sizeof(T) == 8 ? GPX_F64 : GPX_F32;
    // ncols < n (forward only): the matrix is a trapezoid -- an ncols x ncols lower
    // triangle on top of (n - ncols) further rows; x[0:ncols] is solved and the
    // remaining right-hand side b[ncols:n] is reduced by L[ncols:n, 0:ncols] x.
    if (ncols < 0 || ncols > n) ncols = n;
    Sweep<T> S;
    S.L = L; S.n = n; S.ldl = ldl; S.ncols = ncols; S.b = b; S.x = x; S.st = st;
    // bt: bt->count systems solved by the same launches; sA = stride of L, sB = stride of b and x
    S.nbt = (unsigned)(bt ? bt->count : 1); S.sL = bt ? bt->sA : 0; S.sv = bt ? bt->sB : 0;
    ProfScope prof(PC_TRSV, ((double)n * ncols - 0.5 * (double)ncols * (ncols - 1)) * sizeof(T) * S.nbt, st);
    S.sLinv = cdiv(ncols, SB) * SB * SB;
    void *scr = nullptr;
    GPX_TRY(g_scr.get((size_t)S.nbt * S.sLinv * sizeof(T), &scr));
    S.Linv = (T *)scr;
    S.aligned = (((uintptr_t)L) % (2 * sizeof(T)) == 0) && (ldl % 2 == 0);
    // the route (table above)
    const bool usable = !bt && ncols == n && ops_usable(dtype, L, ldl);
    const bool cached = ops && ops->mem.p && n % OB == 0 && ops->mem.bytes >= trsv_ops_bytes(dtype, n);
    const bool prebuilt = cached && ops->valid;
    // operators of the LEADING blocks only (built beside the factorisation, gpx_gp_fit; the caller has ordered `st` behind
    // them): a backward sweep takes the trailing blocks by steps and switches to one launch per block where they begin
    const int64_t kpart = (usable && cached && !ops->valid && ops->built > 0 && transpose) ? std::min(ops->built, n / OB) : 0;
    if (kpart == 0 && usable && (n >= trsv_ops_min_n() || prebuilt)) {
        route_hit(RT_TRSV_OPS);
        void *buf = nullptr;
        if (ops) {                                                   // the caller's cache (one factor, many solves)
            bool grew = false;
            GPX_TRY(ops->mem.reserve(trsv_ops_bytes(dtype, n), st, &grew));
            if (grew) ops->invalidate();
            buf = ops->mem.p;
        } else {
            GPX_TRY(g_ops.get(trsv_ops_bytes(dtype, n), &buf));
        }
        const OpsView<T> V(buf, n);
        // (a factor whose leading blocks already have their operators: only the rest)
        if (!ops || !ops->valid) GPX_TRY(trsv_ops_prepare<T>(L, n, ldl, buf, st, ops ? std::min(ops->built, V.nfull) : 0, V.nfull));
        if (ops) { ops->valid = true; ops->built = V.nfull; }
        const bool ragged = n > V.nfull * OB;
        if (!transpose) {
            ops_fwd(S, V);
            if (ragged) { inv64_blocks(S, 0, 1); steps_fwd(S, V.nfull); }
        } else {
            if (ragged) { inv64_blocks(S, 0, 0); steps_bwd(S, V.nfull); }
            ops_bwd(S, V, V.nfull);
        }
    } else if (!transpose) {
        route_hit(RT_TRSV_STEPS);
        inv64_blocks(S, 0, 1);
        steps_fwd(S, 0);
    } else {                                   // steps for the blocks [kpart, nb); the mixed sweep (kpart > 0): then operators
        route_hit(RT_TRSV_STEPS);
        inv64_blocks(S, kpart * (OB / SB), 0);
        steps_bwd(S, kpart);
        if (kpart > 0) {
            route_hit(RT_TRSV_OPS);
            ops_bwd(S, OpsView<T>(ops->mem.p, n), kpart);
        }
    }
    GPX_LAUNCH_CHECK();
    return GPX_OK;
}

int trsv_lower(int dtype, const void *L, int64_t n, int64_t ldl, void *b, void *x, int transpose,
               hipStream_t st, const Batch *bt, TrsvOps *ops)
{
    if (n <= 0) return GPX_OK;
    return by_dtype(dtype, [&](auto t) {
        using T = decltype(t);
        return trsv_t<T>((const T *)L, n, ldl, (T *)b, (T *)x, transpose, st, -1, bt, ops);
    });
}

int trsv_ops_build(int dtype, const void *L, int64_t n, int64_t ldl, TrsvOps *ops, hipStream_t st)
{
    if (!ops || !trsv_ops_whole_blocks(n) || !ops_usable(dtype, L, ldl)) return GPX_OK;   // the solve takes the step route
    GPX_TRY(ops->mem.reserve(trsv_ops_bytes(dtype, n), st));
    ops->invalidate();
    GPX_TRY(by_dtype(dtype, [&](auto t) { using T = decltype(t); return trsv_ops_prepare<T>((const T *)L, n, ldl, ops->mem.p, st); }));
    ops->valid = true;
    ops->built = n / OB;
    return GPX_OK;
}

int trsv_ops_build_upto(int dtype, const void *L, int64_t n, int64_t ldl, TrsvOps *ops, int64_t kend, hipStream_t st)
{
    if (!ops || !trsv_ops_ahead_ok(dtype, L, n, ldl)) return GPX_OK;
    const int64_t nfull = n / OB;
    kend = std::min(kend, nfull);
    if (ops->built == 0) {
        GPX_TRY(ops->mem.reserve_device(trsv_ops_bytes(dtype, n)));
        ops->valid = false;
    }
    if (kend <= ops->built || !ops->mem.p) return GPX_OK;
    GPX_TRY(by_dtype(dtype, [&](auto t) { using T = decltype(t); return trsv_ops_prepare<T>((const T *)L, n, ldl, ops->mem.p, st, ops->built, kend); }));
    ops->built = kend;
    if (kend == nfull) ops->valid = true;
    return GPX_OK;
}

int trsv_lower_cols(int dtype, const void *L, int64_t n, int64_t ldl, int64_t ncols, void *b, void *x,
                    hipStream_t st)
{
    if (n <= 0 || ncols <= 0) return GPX_OK;
    return by_dtype(dtype, [&](auto t) { using T = decltype(t); return trsv_t<T>((const T *)L, n, ldl, (T *)b, (T *)x, 0, st, ncols); });
}

// y[c] -= sum_r Lp[r, c] * x[r]   (c < ncols <= 1024, r < rows): the transposed
// panel product of the distributed back substitution.  Two stages, fixed
// summation order: 256-row chunks -> partial sums in `work`, then one reduction.
template <typename T>
__global__ __launch_bounds__(256) void panel_gemv_t_partial(const T *__restrict__ Lp, int64_t ldl,
                                                            int64_t rows, int ncols,
                                                            const T *__restrict__ x, double *__restrict__ work)
{
    __shared__ T sx[256];
    const int tid = threadIdx.x;
    const int64_t r0 = (int64_t)blockIdx.x * 256;
    sx[tid] = (r0 + tid < rows) ? x[r0 + tid] : (T)0;
    __syncthreads();
    const int nr = (int)std::min<int64_t>(256, rows - r0);
    for (int c = tid; c < ncols; c += 256) {
        const T *col = Lp + r0 * ldl + c;
        double acc = 0.0;
        for (int i = 0; i < nr; ++i) acc = fma((double)col[(int64_t)i * ldl], (double)sx[i], acc);
        work[(int64_t)blockIdx.x * ncols + c] = acc;
    }
}

template <typename T>
__global__ void panel_gemv_t_reduce(const double *__restrict__ work, int64_t nchunks, int ncols,
                                    T *__restrict__ y)
{
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= ncols) return;
    double acc = 0.0;
    for (int64_t k = 0; k < nchunks; ++k) acc += work[k * ncols + c];
    y[c] = (T)((double)y[c] - acc);
}

int panel_gemv_t(int dtype, const void *Lp, int64_t ldl, int64_t rows, int64_t ncols, const void *x,
                 void *y, double *work, hipStream_t st)
{
    if (rows <= 0 || ncols <= 0) return GPX_OK;
    const int64_t nchunks = cdiv(rows, 256);
    ProfScope prof(PC_TRSV, (double)rows * ncols * esize(dtype), st);
    return by_dtype(dtype, [&](auto t) {
        using T = decltype(t);
        hipLaunchKernelGGL((panel_gemv_t_partial<T>), dim3((unsigned)nchunks), dim3(256), 0, st,
                           (const T *)Lp, ldl, rows, (int)ncols, (const T *)x, work);
        hipLaunchKernelGGL((panel_gemv_t_reduce<T>), dim3((unsigned)cdiv(ncols, 256)), dim3(256), 0, st,
                           work, nchunks, (int)ncols, (T *)y);
        GPX_LAUNCH_CHECK();
        return GPX_OK;
    });
}

static thread_local ThreadScratch g_trsm_scr;   // the operator route: one m x 512 block of X per system

// Operator route of X <- X L^-T for `count` systems in LOCK-STEP (whole blocks, every system's block operators complete in
// ops_base + i * sO): the substitution inside a 512-block,
//   X[:, blk] <- X[:, blk] inv(L_kk)^T,
// is ONE product with W_k = inv(L_kk) (into a scratch block, copied back) instead of eight 64-wide substitutions with
// seven small products between them -- 16 latency-bound launches a block, which were most of a posterior covariance
// (n = 8192, m = 1024: cov 11.0 -> see DESIGN 3.3).  Every launch covers all systems -- at n = 8192 a single system's far
// update is 1 - 2 rounds of tiles (32 x 32 at most), eight of them fill the chip.  L, X, the operators and the scratch
// block are sL / sX / sO / (m * 512) elements apart.
// c0 (x_upper only; 0: the whole sweep): row i of X is zero before column c0 + i -- rows [c0, c0 + m) of the identity.  The
// sweep begins at the block that holds column c0, and a block that ends at column r works on the rows c0 + i < r.
static int trsm_right_lt_ops(int dtype, const void *L, int64_t sL, int64_t n, int64_t ldl, void *X, int64_t sX, int64_t m, int64_t ldx,
                             hipStream_t st, int x_upper, const void *ops_base, int64_t sO, int count, int64_t c0 = 0)
{
    route_hit(RT_TRSM_OPS);
    const size_t es = esize(dtype);
    const int64_t sS = m * OB;
    void *scr = nullptr;
    GPX_TRY(g_trsm_scr.get((size_t)count * sS * es, &scr));
    for (int64_t k = c0 / OB; k < n / OB; ++k) {
        const int64_t k0 = k * OB, r = k0 + OB;
        const int64_t me = x_upper ? std::min(m, r - c0) : m;
        char *Xk = (char *)X + k0 * es;
        const void *Wk = dtype == GPX_F64 ? (void *)OpsView<double>(ops_base, n).W(k) : (void *)OpsView<float>(ops_base, n).W(k);
        Batch b1; b1.count = count; b1.sA = sX; b1.sB = sO; b1.sC = sS;
        GPX_TRY(gemm_nt(dtype, me, OB, OB, Xk, ldx, Wk, OB, scr, OB, 1.0, GPX_FULL, 0, 0, st, 1, 0, &b1));
        for (int i = 0; i < count; ++i)
            GPX_HIP(hipMemcpy2DAsync(Xk + (size_t)i * sX * es, (size_t)ldx * es, (const char *)scr + (size_t)i * sS * es, (size_t)OB * es,
                                     (size_t)OB * es, (size_t)me, hipMemcpyDeviceToDevice, st));
        if (r < n) {
            Batch b2; b2.count = count; b2.sA = sX; b2.sB = sL; b2.sC = sX;
            GPX_TRY(gemm_nt(dtype, me, n - r, OB, Xk, ldx, (const char *)L + (r * ldl + k0) * es, ldl, (char *)X + r * es, ldx,
                            -1.0, GPX_FULL, 0, 0, st, 0, 0, &b2));
        }
    }
    return GPX_OK;
}

// X (m x n) <- X * L^-T, blocked and RIGHT-looking: after the columns of a block are
// solved they are applied at once to every remaining column,
//   X[:, r:] -= X[:, blk] * L[r:, blk]^T      (m x (n - r) output, K = block width),
// which keeps all CUs busy even for few right-hand sides (m ~ 1000 test points); a
// left-looking sweep would launch m/256 x 2 tiles per step.  Inside a block: 64-wide
// substitutions by trsm_rows (shared with the Cholesky panel) with small MFMA updates.
// x_upper: X is upper triangular on entry (the identity, when L^-T itself is wanted): rows beyond
// the current block are still zero in its columns, so every step works on the leading k0 + kb rows
// only -- a third of the flops.
// c0 > 0 (x_upper, a multiple of 64): X holds rows [c0, c0 + m) of the identity, zero before column c0 + i in row i, so the
// sweep is the trailing sub-system from c0 on (the operator route: from the start of c0's block); nothing left of it is touched.
// (64 elements are 256 or 512 bytes: L + c0 (ldl + 1) and X + c0 sit on whatever 16-byte boundary L and X sit on.)
int trsm_right_lt(int dtype, const void *L, int64_t n, int64_t ldl, void *X, int64_t m, int64_t ldx,
                  hipStream_t st, int x_upper, TrsvOps *ops, int64_t c0)
{
    if (n <= 0 || m <= 0) return GPX_OK;
    const size_t es = esize(dtype);
    if (c0 < 0 || c0 >= n || c0 % SB != 0 || (c0 > 0 && !x_upper)) { set_error("trsm_right_lt: bad first column %lld", (long long)c0); return GPX_ERR_ARG; }
    // Operator route (the caller's TrsvOps of THIS factor): completed here if the factor has only some.
    if (ops && trsm_ops_ok(dtype, L, n, ldl) && ldx % (16 / (int64_t)es) == 0 && ((uintptr_t)X) % 16 == 0) {
        if (!ops->valid) GPX_TRY(trsv_ops_build_upto(dtype, L, n, ldl, ops, n / OB, st));
        if (ops->valid && ops->mem.p) return trsm_right_lt_ops(dtype, L, 0, n, ldl, X, 0, m, ldx, st, x_upper, ops->mem.p, 0, 1, c0);
    }
    if (c0 > 0)                                            // the 64-wide route on the trailing sub-system
        return trsm_right_lt(dtype, (const char *)L + c0 * (ldl + 1) * es, n - c0, ldl, (char *)X + c0 * es, m, ldx, st, 1, nullptr, 0);
    const int64_t NB = n >= 8192 ? 512 : 256;
    auto Lp = [&](int64_t r, int64_t c) { return (const char *)L + (r * ldl + c) * es; };
    auto Xp = [&](int64_t c) { return (char *)X + c * es; };
    for (int64_t k0 = 0; k0 < n; k0 += NB) {
        const int64_t kb = std::min(NB, n - k0);
        const int64_t me = x_upper ? std::min(m, k0 + kb) : m;        // rows that can be non-zero here
        for (int64_t j0 = k0; j0 < k0 + kb; j0 += SB) {
            const int jb = (int)std::min<int64_t>(SB, k0 + kb - j0);
            if (j0 > k0)
                GPX_TRY(gemm_nt(dtype, me, jb, j0 - k0, Xp(k0), ldx, Lp(j0, k0), ldl, Xp(j0), ldx, -1.0,
                                GPX_FULL, 0, 0, st));
            GPX_TRY(trsm_rows(dtype, Xp(j0), ldx, me, Lp(j0, j0), ldl, jb, st));
        }
        const int64_t r = k0 + kb;
        if (r < n)
            GPX_TRY(gemm_nt(dtype, me, n - r, kb, Xp(k0), ldx, Lp(r, k0), ldl, Xp(r), ldx, -1.0, GPX_FULL, 0, 0,
                            st));
    }
    return GPX_OK;
}

// ---- X <- X L^-1: the backward sweep over many right-hand sides -------------------------------------------
// X[r, 0:jb] <- X[r, 0:jb] * Ljj^-1 for rows r < rows: trsm_rows (gpx_potrf.hip) mirrored, one lane per row, backward
// substitution along the row:  x_c = (a_c - sum_{t > c} x_t L[t, c]) / L[c, c],  c = jb - 1 .. 0.  All lanes read the same
// element of the staged block at the same time (an LDS broadcast).
template <typename T, bool FULL64>
__global__ __launch_bounds__(256) void trsm_rows_l_kernel(T *__restrict__ X, int64_t ldx, int64_t rows,
                                                          const T *__restrict__ Ljj, int64_t ldl, int jb)
{
    __shared__ T sL[SB * (SB + 1)];
    const int tid = threadIdx.x;
    for (int idx = tid; idx < jb * jb; idx += 256) {
        const int i = idx / jb, c = idx - i * jb;
        sL[i * (SB + 1) + c] = (c <= i) ? Ljj[(int64_t)i * ldl + c] : (T)0;
    }
    __syncthreads();
    const int64_t r = (int64_t)blockIdx.x * 256 + tid;
    if (r >= rows) return;
    T *xr = X + r * ldx;
    if (FULL64) {
        T x[SB];
        constexpr int CH = 16 / sizeof(T);
#pragma unroll
        for (int c = 0; c < SB; c += CH) {
            struct alignas(16) V { T e[CH]; } v = *reinterpret_cast<const V *>(xr + c);
#pragma unroll
            for (int e = 0; e < CH; ++e) x[c + e] = v.e[e];
        }
#pragma unroll
        for (int c = SB - 1; c >= 0; --c) {
            T v = x[c];
#pragma unroll
            for (int t = SB - 1; t > c; --t) v = fma(-x[t], sL[t * (SB + 1) + c], v);
            x[c] = v / sL[c * (SB + 1) + c];
        }
#pragma unroll
        for (int c = 0; c < SB; c += CH) {
            struct alignas(16) V { T e[CH]; } v;
#pragma unroll
            for (int e = 0; e < CH; ++e) v.e[e] = x[c + e];
            *reinterpret_cast<V *>(xr + c) = v;
        }
    } else {
        for (int c = jb - 1; c >= 0; --c) {
            T v = xr[c];
            for (int t = jb - 1; t > c; --t) v = fma(-xr[t], sL[t * (SB + 1) + c], v);
            xr[c] = v / sL[c * (SB + 1) + c];
        }
    }
}

template <typename T>
static int trsm_rows_l(void *X, int64_t ldx, int64_t rows, const void *Ljj, int64_t ldl, int jb, hipStream_t st)
{
    if (rows <= 0 || jb <= 0) return GPX_OK;
    const dim3 grid((unsigned)cdiv(rows, 256)), block(256);
    const bool vec_ok = jb == SB && ldx % (16 / (int64_t)sizeof(T)) == 0 && ((uintptr_t)X) % 16 == 0;
    ProfScope prof(PC_TRSM_ROWS, (double)rows * jb * jb, st);
    if (vec_ok) hipLaunchKernelGGL((trsm_rows_l_kernel<T, true>), grid, block, 0, st, (T *)X, ldx, rows, (const T *)Ljj, ldl, jb);
    else hipLaunchKernelGGL((trsm_rows_l_kernel<T, false>), grid, block, 0, st, (T *)X, ldx, rows, (const T *)Ljj, ldl, jb);
    GPX_LAUNCH_CHECK();
    return GPX_OK;
}

static thread_local ThreadScratch g_trsml_scr;  // X L^-1: the transposed row panel of L of the block being applied

// X (m x n) <- X * L^-1, blocked and RIGHT-looking, block columns from the LAST to the first: after the columns of a block
// are solved they are applied at once to every column before them,
//   X[:, 0:k0] -= X[:, blk] * L[blk, 0:k0]      (m x k0 output, K = block width).
// gemm_nt wants both operands K-contiguous and this one is a ROW panel of L read along its rows, so the panel is staged
// transposed (LT[c][t] = L[k0 + t, c], ld = block width rounded up to 16) in thread scratch first: n^2 / 2 elements moved per sweep.
// Operator route (the caller's TrsvOps of THIS factor, trsm_ops_ok, X and ldx aligned as L and ldl): the in-block solve is ONE
// product with Wt_k = inv(L_kk)^T -- gemm_nt(X_k, Wt_k) = X_k inv(L_kk) -- into the scratch block trsm_right_lt_ops uses,
// copied back.  64-wide route (everything else): two levels as in trsm_right_lt (outer 256 / 512, inner 64); the transposed
// panel includes the outer block's own columns, so the left-looking products inside the block read it too, and a 64 x 64
// diagonal block is solved by substitution along the rows (trsm_rows_l_kernel).
int trsm_right_l(int dtype, const void *L, int64_t n, int64_t ldl, void *X, int64_t m, int64_t ldx, hipStream_t st, TrsvOps *ops)
{
    if (n <= 0 || m <= 0) return GPX_OK;
    const size_t es = esize(dtype);
    auto Lp = [&](int64_t r, int64_t c) { return (const char *)L + (r * ldl + c) * es; };
    auto Xp = [&](int64_t c) { return (char *)X + c * es; };
    if (ops && trsm_ops_ok(dtype, L, n, ldl) && ldx % (16 / (int64_t)es) == 0 && ((uintptr_t)X) % 16 == 0) {
        if (!ops->valid) GPX_TRY(trsv_ops_build_upto(dtype, L, n, ldl, ops, n / OB, st));
        if (ops->valid && ops->mem.p) {
            route_hit(RT_TRSM_L_OPS);
            void *scr = nullptr, *LT = nullptr;
            GPX_TRY(g_trsm_scr.get((size_t)m * OB * es, &scr));
            GPX_TRY(g_trsml_scr.get((size_t)(n - OB) * OB * es, &LT));
            for (int64_t k = n / OB - 1; k >= 0; --k) {
                const int64_t k0 = k * OB;
                const void *Wtk = dtype == GPX_F64 ? (void *)OpsView<double>(ops->mem.p, n).Wt(k) : (void *)OpsView<float>(ops->mem.p, n).Wt(k);
                GPX_TRY(gemm_nt(dtype, m, OB, OB, Xp(k0), ldx, Wtk, OB, scr, OB, 1.0, GPX_FULL, 0, 0, st, 1));
                GPX_HIP(hipMemcpy2DAsync(Xp(k0), (size_t)ldx * es, scr, (size_t)OB * es, (size_t)OB * es, (size_t)m, hipMemcpyDeviceToDevice, st));
                if (k0 > 0) {
                    GPX_TRY(transpose(dtype, Lp(k0, 0), ldl, OB, k0, LT, OB, 0, st));
                    GPX_TRY(gemm_nt(dtype, m, k0, OB, Xp(k0), ldx, LT, OB, X, ldx, -1.0, GPX_FULL, 0, 0, st));
                }
            }
            return GPX_OK;
        }
    }
    const int64_t NB = n >= 8192 ? OB : 256;
    const int64_t ldt = std::min<int64_t>(NB, round_up(n, 16));
    void *LTv = nullptr;
    GPX_TRY(g_trsml_scr.get((size_t)n * ldt * es, &LTv));
    const char *LT = (const char *)LTv;
    for (int64_t k0 = (n - 1) / NB * NB; k0 >= 0; k0 -= NB) {
        const int64_t kb = std::min(NB, n - k0), ke = k0 + kb;
        // LT[c][t] = L[k0 + t, c] for c < ke, t < kb (the block's own columns too: only what lies below a diagonal block is read)
        GPX_TRY(transpose(dtype, Lp(k0, 0), ldl, kb, ke, LTv, ldt, 0, st));
        for (int64_t j0 = k0 + (kb - 1) / SB * SB; j0 >= k0; j0 -= SB) {
            const int jb = (int)std::min<int64_t>(SB, ke - j0);
            const int64_t je = j0 + jb;
            if (je < ke)
                GPX_TRY(gemm_nt(dtype, m, jb, ke - je, Xp(je), ldx, LT + (j0 * ldt + (je - k0)) * es, ldt, Xp(j0), ldx, -1.0,
                                GPX_FULL, 0, 0, st));
            GPX_TRY(by_dtype(dtype, [&](auto t) { return trsm_rows_l<decltype(t)>(Xp(j0), ldx, m, Lp(j0, j0), ldl, jb, st); }));
        }
        if (k0 > 0)
            GPX_TRY(gemm_nt(dtype, m, k0, kb, Xp(k0), ldx, LT, ldt, X, ldx, -1.0, GPX_FULL, 0, 0, st));
    }
    return GPX_OK;
}

// X = I L^-T = L^-T ; K^-1 = L^-T L^-1 = X X^T   (gp/gp.py:311-312; gpx_common.h for the arguments)
int inv_from_factor(int dtype, const void *L, int64_t n, int64_t ldl, void *X, void *W, int tri, hipStream_t st,
                    TrsvOps *ops, int count, int64_t sL, void *group_ops)
{
    const size_t es = esize(dtype), nl = (size_t)n * ldl * es, ob = trsv_ops_bytes(dtype, n);
    if (count > 1 && !trsm_ops_ok(dtype, L, n, ldl)) { set_error("inv_from_factor: a lock-step group needs the operator route"); return GPX_ERR_ARG; }
    for (int i = 0; i < count; ++i) {
        GPX_TRY(eye_rows(dtype, (char *)X + (size_t)i * nl, n, ldl, 0, 0, st));
        if (count > 1) {
            TrsvOps o = TrsvOps::view((char *)group_ops + (size_t)i * ob, ob);
            GPX_TRY(trsv_ops_build_upto(dtype, (const char *)L + (size_t)i * sL * es, n, ldl, &o, n / OB, st));
        }
    }
    GPX_HIP(hipMemsetAsync(W, 0, (size_t)count * nl, st));
    const int64_t sX = (int64_t)(nl / es);
    if (count > 1) GPX_TRY(trsm_right_lt_ops(dtype, L, sL, n, ldl, X, sX, n, ldl, st, 1, group_ops, (int64_t)(ob / es), count));
    else GPX_TRY(trsm_right_lt(dtype, L, n, ldl, X, n, ldl, st, 1, ops));
    Batch bw; bw.count = count; bw.sA = bw.sB = bw.sC = sX;
    return gemm_nt(dtype, n, n, n, X, ldl, X, ldl, W, ldl, 1.0, tri, 0, 0, st, 0, 1, count > 1 ? &bw : nullptr);
}

// ---- predictive variance: the finishing pass over a solved chunk X = K(xo_c, x) L^-T ---------------------------------
// k(xo_i, xo_i) as gpx_d_kmat builds it on its diagonal: the same accumulation of the distance (every term a_k - a_k:
// 0 for finite points, NaN otherwise) through the same entry functions, in the handle's dtype.
template <typename T>
__device__ __forceinline__ T kdiag_entry(const KParams &kp, const T *__restrict__ a, int d)
{
    T acc = (T)0;
    if (kp.kernel == GPX_KERNEL_GAUSSIAN) {
        for (int k = 0; k < d; ++k) { const T t = a[k] - a[k]; acc = fma(t, t, acc); }
        return gaussian_entry<T, 0>(acc, (T)kp.c[0], (T)kp.c[1], (T)kp.c[2], (T)kp.c[3]);
    }
    for (int k = 0; k < d; ++k) { const T sn = sin((T)0.5 * (a[k] - a[k]) / (T)kp.c[2]); acc = fma(sn, sn, acc); }
    return periodic_k<T>(acc, (T)kp.c[0], (T)kp.c[1]);
}

// One workgroup per row (grid-stride over rows): out[i] = kdiag(i) - sum_j X[i, j]^2, or out[i] += sum_j X[i, j]^2.
// Bandwidth bound (rows n es bytes, read once): 16-byte loads, four in flight per lane; every lane sums its elements in
// f64 in index order, the wave is folded by lanes64_sum, the four waves through LDS in wave order -- no atomics, the
// same bits every time.  MODE 0: kdiag from kdiag_dev   1: kdiag from the kernel family at xo   2: accumulate.
template <typename T, int MODE>
__global__ __launch_bounds__(256) void var_rows_kernel(const T *__restrict__ X, int64_t rows, int64_t n, int64_t ldx,
                                                       int aligned, const T *__restrict__ xo, int d, KParams kp,
                                                       const double *__restrict__ kdiag, double *__restrict__ out)
{
    constexpr int VEC = Vec<T>::N;
    typedef typename Vec<T>::type VT;
    __shared__ double red[4];
    const int tid = threadIdx.x;
    const int64_t nv = aligned ? n / VEC : 0;              // whole 16-byte vectors of a row; the rest is the scalar tail
    for (int64_t row = blockIdx.x; row < rows; row += gridDim.x) {
        const T *__restrict__ xr = X + row * ldx;
        const VT *__restrict__ xv = reinterpret_cast<const VT *>(xr);
        double acc = 0.0;
        int64_t v = tid;
        for (; v + 3 * 256 < nv; v += 4 * 256) {
            VT t[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) t[u] = xv[v + u * 256];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const T *e = reinterpret_cast<const T *>(&t[u]);
#pragma unroll
                for (int q = 0; q < VEC; ++q) acc = fma((double)e[q], (double)e[q], acc);
            }
        }
        for (; v < nv; v += 256) {
            const VT t = xv[v];
            const T *e = reinterpret_cast<const T *>(&t);
#pragma unroll
            for (int q = 0; q < VEC; ++q) acc = fma((double)e[q], (double)e[q], acc);
        }
        for (int64_t c = nv * VEC + tid; c < n; c += 256) acc = fma((double)xr[c], (double)xr[c], acc);
        acc = lanes64_sum(acc);
        __syncthreads();                                   // (the row before: red[] has been read)
        if ((tid & 63) == 0) red[tid >> 6] = acc;
        __syncthreads();
        if (tid == 0) {
            const double s = ((red[0] + red[1]) + red[2]) + red[3];
            if (MODE == 2) out[row] += s;
            else if (MODE == 0) out[row] = kdiag[row] - s;
            else out[row] = (double)kdiag_entry<T>(kp, xo + row * d, d) - s;
        }
    }
}

// out[i] = k(xo_i, xo_i) - acc[i]: the distributed form's last step, after the ranks' row sums have been added up
template <typename T>
__global__ void var_finish_kernel(const T *__restrict__ xo, int d, KParams kp, const double *__restrict__ acc, int64_t rows,
                                  double *__restrict__ out)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < rows) out[i] = (double)kdiag_entry<T>(kp, xo + i * d, d) - acc[i];
}

template <typename T>
static int launch_var_rows(const void *X, int64_t rows, int64_t n, int64_t ldx, const void *xo, int d, const KParams &kp,
                           const double *kdiag_dev, int accumulate, double *out_dev, hipStream_t st)
{
    const int aligned = (ldx * (int64_t)sizeof(T)) % 16 == 0 && ((uintptr_t)X) % 16 == 0;
    const dim3 grid((unsigned)std::min<int64_t>(rows, 1 << 20)), block(256);
    ProfScope prof(PC_REDUCE, (double)rows * (double)n * sizeof(T), st);
#define GPX_VAR_LAUNCH(MODE)                                                                                   \
    hipLaunchKernelGGL((var_rows_kernel<T, MODE>), grid, block, 0, st, (const T *)X, rows, n, ldx, aligned,   \
                       (const T *)xo, d, kp, kdiag_dev, out_dev)
    if (accumulate) GPX_VAR_LAUNCH(2);
    else if (kdiag_dev) GPX_VAR_LAUNCH(0);
    else GPX_VAR_LAUNCH(1);
#undef GPX_VAR_LAUNCH
    GPX_LAUNCH_CHECK();
    return GPX_OK;
}

int var_rows(int dtype, int kernel, const void *X, int64_t rows, int64_t n, int64_t ldx, const void *xo, int d,
             const double *params, const double *kdiag_dev, int accumulate, double *out_dev, hipStream_t st)
{
    if (rows <= 0) return GPX_OK;
    KParams kp;
    memset(&kp, 0, sizeof(kp));
    if (!accumulate && !kdiag_dev) GPX_TRY(make_kparams(kernel, GPX_K, params, 0.0, &kp));
    return by_dtype(dtype, [&](auto t) { return launch_var_rows<decltype(t)>(X, rows, n, ldx, xo, d, kp, kdiag_dev, accumulate, out_dev, st); });
}

int var_finish(int dtype, int kernel, const void *xo, int d, const double *params, const double *acc_dev, int64_t rows,
               double *out_dev, hipStream_t st)
{
    if (rows <= 0) return GPX_OK;
    KParams kp;
    GPX_TRY(make_kparams(kernel, GPX_K, params, 0.0, &kp));
    const dim3 grid((unsigned)cdiv(rows, 256)), block(256);
    return by_dtype(dtype, [&](auto t) {
        using T = decltype(t);
        hipLaunchKernelGGL((var_finish_kernel<T>), grid, block, 0, st, (const T *)xo, d, kp, acc_dev, rows, out_dev);
        GPX_LAUNCH_CHECK();
        return GPX_OK;
    });
}

// ---- leave-one-out: the finishing pass over a solved chunk X = E_c L^-T (rows [c0, c0 + rows) of the identity) --------
// RW06 eq. 5.10 - 5.12 from k = (K^-1)_ii, a = alpha_i and y_i: the left-out mean and variance, and log p(y_i | the others)
__device__ __forceinline__ void loo_point(double k, double a, double y, int64_t i, double *__restrict__ mean,
                                          double *__restrict__ var, double *__restrict__ logp)
{
#pragma clang fp contract(off)                             // (both callers round alike: the fused pass and the cached one give the same bits)
    if (mean) mean[i] = y - a / k;
    if (var) var[i] = 1.0 / k;
    if (logp) logp[i] = 0.5 * log(k) - 0.5 * a * a / k - 0.9189385332046727;      // log(2 pi) / 2
}

// One workgroup per row (grid-stride over rows), var_rows_kernel's reduction: kii[i] = sum_j X[i, j]^2 over j in [c0 + i, n)
// -- row i of X is column c0 + i of L^-1, zero (and never written by the sweep) before that column.  The row is read from
// c0 + i rounded down to the 16-byte vector; the columns before c0 + i are masked, nothing outside [that vector, n) is
// loaded.  With y and alpha (the chunk's own rows, handle dtype) the leave-one-out quantities of the row are written too.
template <typename T>
__global__ __launch_bounds__(256) void loo_rows_kernel(const T *__restrict__ X, int64_t rows, int64_t n, int64_t ldx, int64_t c0,
                                                       int aligned, const T *__restrict__ y, const T *__restrict__ alpha,
                                                       double *__restrict__ kii, double *__restrict__ mean,
                                                       double *__restrict__ var, double *__restrict__ logp)
{
    constexpr int VEC = Vec<T>::N;
    typedef typename Vec<T>::type VT;
    __shared__ double red[4];
    const int tid = threadIdx.x;
    const int64_t nv = aligned ? n / VEC : 0;              // whole 16-byte vectors of a row; the rest is the scalar tail
    for (int64_t row = blockIdx.x; row < rows; row += gridDim.x) {
        const T *__restrict__ xr = X + row * ldx;
        const VT *__restrict__ xv = reinterpret_cast<const VT *>(xr);
        const int64_t first = c0 + row;                    // the row's first column
        double acc = 0.0;
#pragma unroll 4
        for (int64_t v = first / VEC + tid; v < nv; v += 256) {
            const VT t = xv[v];
            const T *e = reinterpret_cast<const T *>(&t);
#pragma unroll
            for (int q = 0; q < VEC; ++q) {
                const double x = (v * VEC + q >= first) ? (double)e[q] : 0.0;
                acc = fma(x, x, acc);
            }
        }
        for (int64_t c = max(nv * VEC, first) + tid; c < n; c += 256) acc = fma((double)xr[c], (double)xr[c], acc);
        acc = lanes64_sum(acc);
        __syncthreads();                                   // (the row before: red[] has been read)
        if ((tid & 63) == 0) red[tid >> 6] = acc;
        __syncthreads();
        if (tid == 0) {
            const double k = ((red[0] + red[1]) + red[2]) + red[3];
            if (kii) kii[row] = k;
            if (y) loo_point(k, (double)alpha[row], (double)y[row], row, mean, var, logp);
        }
    }
}

// the same quantities from a diagonal that is already there
template <typename T>
__global__ void loo_point_kernel(const double *__restrict__ kii, const T *__restrict__ y, const T *__restrict__ alpha, int64_t n,
                                 double *__restrict__ mean, double *__restrict__ var, double *__restrict__ logp)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) loo_point(kii[i], (double)alpha[i], (double)y[i], i, mean, var, logp);
}

int loo_rows(int dtype, const void *X, int64_t rows, int64_t n, int64_t ldx, int64_t c0, const void *y, const void *alpha,
             double *kii, double *mean, double *var, double *logp, hipStream_t st)
{
    if (rows <= 0) return GPX_OK;
    const size_t es = esize(dtype);
    const int aligned = (ldx * (int64_t)es) % 16 == 0 && ((uintptr_t)X) % 16 == 0;
    const dim3 grid((unsigned)std::min<int64_t>(rows, 1 << 20)), block(256);
    ProfScope prof(PC_REDUCE, ((double)rows * (double)(n - c0) - 0.5 * (double)rows * (double)rows) * es, st);
    return by_dtype(dtype, [&](auto t) {
        using T = decltype(t);
        hipLaunchKernelGGL((loo_rows_kernel<T>), grid, block, 0, st, (const T *)X, rows, n, ldx, c0, aligned, (const T *)y, (const T *)alpha,
                           kii, mean, var, logp);
        GPX_LAUNCH_CHECK();
        return GPX_OK;
    });
}

int loo_points(int dtype, const double *kii, const void *y, const void *alpha, int64_t n, double *mean, double *var, double *logp,
               hipStream_t st)
{
    if (n <= 0) return GPX_OK;
    const dim3 grid((unsigned)cdiv(n, 256)), block(256);
    return by_dtype(dtype, [&](auto t) {
        using T = decltype(t);
        hipLaunchKernelGGL((loo_point_kernel<T>), grid, block, 0, st, kii, (const T *)y, (const T *)alpha, n, mean, var, logp);
        GPX_LAUNCH_CHECK();
        return GPX_OK;
    });
}

}  // namespace gpx

using namespace gpx;

extern "C" {

int gpx_d_loo_rows(int dtype, const void *X, int64_t rows, int64_t n, int64_t ldx, int64_t c0, const void *y, const void *alpha,
                   double *kii_dev, double *mean_dev, double *var_dev, double *logp_dev, void *stream)
{
    GPX_ARG(dtype == GPX_F64 || dtype == GPX_F32, "dtype must be GPX_F64 or GPX_F32");
    GPX_ARG(rows >= 0 && n >= 0 && ldx >= n && c0 >= 0, "need rows, n, c0 >= 0 and ldx >= n");
    GPX_ARG(c0 + rows <= n, "rows [c0, c0 + rows) must lie within n");
    if (rows == 0) return GPX_OK;
    GPX_ARG(X && (kii_dev || y), "NULL pointer");
    GPX_ARG((y != nullptr) == (alpha != nullptr), "y and alpha go together");
    GPX_ARG(y || !(mean_dev || var_dev || logp_dev), "mean / var / logp need y and alpha");
    GPX_TRY(ensure_device());
    return loo_rows(dtype, X, rows, n, ldx, c0, y, alpha, kii_dev, mean_dev, var_dev, logp_dev, S(stream));
}

int gpx_d_var_rows(int dtype, int kernel, const void *X, int64_t rows, int64_t n, int64_t ldx, const void *xo, int d,
                   const double *params, const double *kdiag_dev, double *out_dev, void *stream)
{
    GPX_ARG(dtype == GPX_F64 || dtype == GPX_F32, "dtype must be GPX_F64 or GPX_F32");
    GPX_ARG(rows >= 0 && n >= 0 && ldx >= n, "need rows, n >= 0 and ldx >= n");
    if (rows == 0) return GPX_OK;
    GPX_ARG(out_dev && (n == 0 || X), "NULL pointer");
    GPX_ARG(kdiag_dev || (xo && params && d >= 1), "need kdiag_dev, or xo, params and d >= 1");
    GPX_ARG(kdiag_dev || kernel == GPX_KERNEL_GAUSSIAN || kernel == GPX_KERNEL_PERIODIC, "unknown kernel family");
    GPX_TRY(ensure_device());
    return var_rows(dtype, kernel, X, rows, n, ldx, xo, d, params, kdiag_dev, 0, out_dev, S(stream));
}

int gpx_d_trsv_lower(int dtype, const void *L, int64_t n, int64_t ldl, void *b, void *x,
                     int transpose, void *stream)
{
    gpx::StreamTurn turn__((hipStream_t)stream);     // (this thread's scratch buffers: one stream at a time, gpx_mem.h)
    GPX_TRY(ensure_device());
    GPX_ARG(dtype == GPX_F64 || dtype == GPX_F32, "dtype must be GPX_F64 or GPX_F32");
    GPX_ARG(n >= 0, "n < 0");
    if (n == 0) return GPX_OK;
    GPX_ARG(L && b && x && b != x, "NULL pointer or b == x");
    GPX_ARG(ldl >= n, "ldl < n");
    return trsv_lower(dtype, L, n, ldl, b, x, transpose, S(stream));
}

int gpx_d_trsm_right_lt(int dtype, const void *L, int64_t n, int64_t ldl, void *X, int64_t m,
                        int64_t ldx, void *stream)
{
    gpx::StreamTurn turn__((hipStream_t)stream);     // (this thread's scratch buffers: one stream at a time, gpx_mem.h)
    GPX_TRY(ensure_device());
    GPX_ARG(dtype == GPX_F64 || dtype == GPX_F32, "dtype must be GPX_F64 or GPX_F32");
    GPX_ARG(n >= 0 && m >= 0, "negative dimension");
    if (n == 0 || m == 0) return GPX_OK;
    GPX_ARG(L && X, "NULL pointer");
    GPX_ARG(ldl >= n && ldx >= n, "leading dimension too small");
    GPX_ARG(ldl % 16 == 0 && ldx % 16 == 0, "ldl/ldx must be multiples of 16 elements");
    GPX_ARG(((uintptr_t)L) % 16 == 0 && ((uintptr_t)X) % 16 == 0, "L/X must be 16-byte aligned");
    return trsm_right_lt(dtype, L, n, ldl, X, m, ldx, S(stream));
}

int gpx_d_trsm_right_l(int dtype, const void *L, int64_t n, int64_t ldl, void *X, int64_t m,
                       int64_t ldx, void *stream)
{
    gpx::StreamTurn turn__((hipStream_t)stream);     // (this thread's scratch buffers: one stream at a time, gpx_mem.h)
    GPX_TRY(ensure_device());
    GPX_ARG(dtype == GPX_F64 || dtype == GPX_F32, "dtype must be GPX_F64 or GPX_F32");
    GPX_ARG(n >= 0 && m >= 0, "negative dimension");
    if (n == 0 || m == 0) return GPX_OK;
    GPX_ARG(L && X, "NULL pointer");
    GPX_ARG(ldl >= n && ldx >= n, "leading dimension too small");
    GPX_ARG(ldl % 16 == 0 && ldx % 16 == 0, "ldl/ldx must be multiples of 16 elements");
    GPX_ARG(((uintptr_t)L) % 16 == 0 && ((uintptr_t)X) % 16 == 0, "L/X must be 16-byte aligned");
    return trsm_right_l(dtype, L, n, ldl, X, m, ldx, S(stream));
}

int gpx_d_logdet_chol(int dtype, const void *L, int64_t n, int64_t ldl, double *out_dev, void *stream)
{
    GPX_TRY(ensure_device());
    GPX_ARG(dtype == GPX_F64 || dtype == GPX_F32, "dtype must be GPX_F64 or GPX_F32");
    GPX_ARG(n >= 0 && out_dev && (n == 0 || L), "bad arguments");
    return logdet_chol(dtype, L, n, ldl, out_dev, S(stream));
}

int gpx_d_dot(int dtype, const void *a, const void *b, int64_t n, double *out_dev, void *stream)
{
    GPX_TRY(ensure_device());
    GPX_ARG(dtype == GPX_F64 || dtype == GPX_F32, "dtype must be GPX_F64 or GPX_F32");
    GPX_ARG(n >= 0 && out_dev && (n == 0 || (a && b)), "bad arguments");
    return dot(dtype, a, b, n, out_dev, S(stream));
}

int gpx_d_trsv_lower_cols(int dtype, const void *L, int64_t n, int64_t ldl, int64_t ncols, void *b,
                          void *x, void *stream)
{
    gpx::StreamTurn turn__((hipStream_t)stream);     // (this thread's scratch buffers: one stream at a time, gpx_mem.h)
    GPX_TRY(ensure_device());
    GPX_ARG(dtype == GPX_F64 || dtype == GPX_F32, "dtype must be GPX_F64 or GPX_F32");
    GPX_ARG(n >= 0 && ncols >= 0 && ncols <= n, "need 0 <= ncols <= n");
    if (n == 0 || ncols == 0) return GPX_OK;
    GPX_ARG(L && b && x && b != x, "NULL pointer or b == x");
    GPX_ARG(ldl >= ncols, "ldl < ncols");
    return trsv_lower_cols(dtype, L, n, ldl, ncols, b, x, S(stream));
}

int gpx_d_panel_gemv_t(int dtype, const void *Lp, int64_t ldl, int64_t rows, int64_t ncols,
                       const void *x, void *y, void *work, void *stream)
{
    GPX_TRY(ensure_device());
    GPX_ARG(dtype == GPX_F64 || dtype == GPX_F32, "dtype must be GPX_F64 or GPX_F32");
    GPX_ARG(rows >= 0 && ncols >= 0, "negative dimension");
    if (rows == 0 || ncols == 0) return GPX_OK;
    GPX_ARG(Lp && x && y && work, "NULL pointer");
    GPX_ARG(ldl >= ncols, "ldl < ncols");
    return panel_gemv_t(dtype, Lp, ldl, rows, ncols, x, y, (double *)work, S(stream));
}

}  // extern "C"
