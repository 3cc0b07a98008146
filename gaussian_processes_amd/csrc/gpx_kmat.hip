// gpx_kmat.hip -- pairwise kernel-matrix build, ARD scaling and the hyper-parameter gradient reductions (gfx950).
//
// Replaces the O(n*m) double loops of gp/ext/gaussian_c.pyx:18-164 and
// gp/ext/periodic_c.pyx:18-235 (one exp per entry, single CPU thread) and the
// `K += eye(n) * s**2` temporaries of gp/gp.py:265.
//
// Roofline: HBM write bandwidth for small d (d = 1: 4.2 TB/s written), the fp64 vector pipe from d ~ 12 up (d = 32:
// 64 instructions per entry for the distance, ~28 for the exp).  Algorithmic bytes per launch = n*m*sizeof(T)
// written (+ (n+m)*d*sizeof(T) read, negligible).  One workgroup owns a 64 x (64*VEC) output tile; its column points
// are staged in LDS once (transposed), every lane owns VEC consecutive columns so that a wave stores 1 KiB contiguous
// per row (16 B per lane); the row points, the same for every lane of a wave, come through the scalar cache into
// SGPRs (as LDS broadcasts they made the LDS return path the bound: N = 65536, d = 32: 9.1-9.6 -> 8.05 ms).  The
// squared distance is accumulated directly as sum_k (a_k - b_k)^2 (never |a|^2+|b|^2-2ab: that loses the digits near
// r = 0 that the reference keeps).
#include "gpx_common.h"
#include "gpx_kernels_dev.h"
#include "gpx_small.h"
#include <type_traits>
#include <vector>

namespace gpx {

// ---------------------------------------------------------------------------
// member constants, precomputed in f64 exactly as the reference spells them
// gaussian (gaussian_c.pyx): c[0]=c1  c[1]=c2  c[2]=c3  c[3]=c4  c[4]=form
// periodic (periodic_c.pyx): c[0]=h  c[1]=w  c[2]=p
// ---------------------------------------------------------------------------
int make_kparams(int kernel, int member, const double *params, double diag_add, KParams *out)
{
    memset(out, 0, sizeof(*out));
    out->kernel = kernel;
    out->member = member;
    out->diag_add = diag_add;
    if (!params) { set_error("params is NULL"); return GPX_ERR_ARG; }
    if (kernel == GPX_KERNEL_GAUSSIAN) {
        const double h = params[0], w = params[1];
        const double S = sqrt(2.0 / M_PI);          // gaussian_c.pyx:14
        const double h2 = h * h, w2 = w * w;
        out->c[0] = -0.5 / w2;                      // c1
        switch (member) {
        case GPX_K:        out->c[1] = 0.5 * S * h2 / w; out->c[4] = 0; break;            // :28
        case GPX_DK_DH:    out->c[1] = S * h / w; out->c[4] = 0; break;                   // :61
        case GPX_DK_DW:    out->c[1] = 0.5 * S * h2 / w2;                                  // :82-83
                           out->c[2] = 0.5 * S * h2 / pow(w, 4); out->c[4] = 1; break;
        case GPX_D2K_DHDH: out->c[1] = S / w; out->c[4] = 0; break;                        // :105
        case GPX_D2K_DHDW: out->c[1] = S * h / w2;                                          // :126-127
                           out->c[2] = S * h / pow(w, 4); out->c[4] = 1; break;
        case GPX_D2K_DWDW: out->c[1] = S * h2 / pow(w, 3);                                  // :153-155
                           out->c[2] = 2.5 * S * h2 / pow(w, 5);
                           out->c[3] = 0.5 * S * h2 / pow(w, 7); out->c[4] = 2; break;
        default: set_error("gaussian kernel has no member %d", member); return GPX_ERR_ARG;
        }
    } else if (kernel == GPX_KERNEL_PERIODIC) {
        if (member < GPX_K || member > GPX_D2K_DPDP) {
            set_error("periodic kernel has no member %d", member);
            return GPX_ERR_ARG;
        }
        out->c[0] = params[0];
        out->c[1] = params[1];
        out->c[2] = params[2];
    } else {
        set_error("unknown kernel family %d", kernel);
        return GPX_ERR_ARG;
    }
    return GPX_OK;
}

struct KP32 { float c[6]; };

constexpr int KM_ROWS = 64;        // tile rows
constexpr int KM_RB = 8;           // rows register-blocked per lane (round 6: 4 -> 8: half the LDS reads and loop overhead per entry,
                                   // N = 65536 d = 32: 7.65 -> 7.3 ms)

// MODE 0..2: gaussian FORM 0..2 ; MODE 3: periodic K, any d ; MODE 4: periodic member, d == 1
template <typename T, int MODE>
__global__ __launch_bounds__(256) void kmat_kernel(const T *__restrict__ x1, int64_t n,
                                                   const T *__restrict__ x2, int64_t m, int d,
                                                   KParams kp, int tri, int aligned,
                                                   T *__restrict__ out, int64_t ld, int rblk)
{
    // rblk: row blocks of KM_ROWS per workgroup.  The column points are staged (transposed) ONCE and serve rblk row
    // blocks (round 6: one block per workgroup paid the 32 KB staging pass and its barrier per 64 rows, and half of
    // the 524 k workgroups of a lower-only N = 65536 build existed only to find themselves above the diagonal)
    constexpr int KIND = MODE == 3 ? GPX_KERNEL_PERIODIC : GPX_KERNEL_GAUSSIAN;   // the pair term (MODE 4 forms none)
    constexpr int VEC = Vec<T>::N;
    constexpr int TN = 64 * VEC;
    constexpr int TNP = TN + VEC;                     // padded row of s2: the transposing stores below
                                                      // (consecutive threads -> consecutive k) spread over the banks
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    // (the row points are staged only where lanes read them as vectors, MODE 4; elsewhere they come through SGPRs)
    T *s1 = reinterpret_cast<T *>(smem_raw);          // [KM_ROWS][d]
    T *s2 = s1 + (MODE == 4 ? (size_t)KM_ROWS * d : (size_t)0);   // [d][TNP]  (transposed: lanes contiguous)

    const int64_t row00 = (int64_t)blockIdx.y * KM_ROWS * rblk;
    const int64_t col0 = (int64_t)blockIdx.x * TN;
    if (tri == GPX_LOWER && col0 > row00 + (int64_t)KM_ROWS * rblk - 1) return;   // every row block strictly above the diagonal

    const int tid = threadIdx.x;
    // stage the two point sets (coalesced: consecutive threads -> consecutive elements)
    // (the tile's points are contiguous in memory: element idx of the tile is x[row0 * d + idx])
    {
        const int64_t lim1 = (n - row00) * d;           // (MODE 4 is launched with rblk = 1)
        const T *g1 = x1 + row00 * d;
        if (MODE == 4)
            for (int idx = tid; idx < KM_ROWS * d; idx += 256) s1[idx] = (idx < lim1) ? g1[idx] : (T)0;
        const int64_t lim2 = (m - col0) * d;
        const T *g2 = x2 + col0 * d;
        const int qd = 256 / d, rd = 256 - qd * d;
        const int cst = tid / d, kst = tid - cst * d;
        GPX_STAGE_POINTS_TRANSPOSED(s2, TNP, g2, TN * d, lim2, d, tid, qd, rd, cst, kst);
    }
    __syncthreads();

    const int lane = tid & 63, wave = tid >> 6;
    const int wave_u = __builtin_amdgcn_readfirstlane(wave);      // (uniform by construction; this tells the compiler)
    const int cbase = lane * VEC;
    const T c1 = (T)kp.c[0], c2 = (T)kp.c[1], c3 = (T)kp.c[2], c4 = (T)kp.c[3];
    const T dadd = (T)kp.diag_add;
#pragma unroll 1
  for (int q = 0; q < rblk; ++q) {
    const int64_t row0 = row00 + (int64_t)q * KM_ROWS;
    if (row0 >= n) break;
    if (tri == GPX_LOWER && col0 > row0 + KM_ROWS - 1) continue;  // this row block is strictly above the diagonal
    // workgroup-uniform: all 64 x TN entries exist, stores are 16-byte aligned, the diagonal (where diag_add
    // goes) does not cross the tile
    const bool interior = aligned && row0 + KM_ROWS <= n && col0 + TN <= m &&
                          (kp.diag_add == 0.0 || col0 >= row0 + KM_ROWS || col0 + TN <= row0);

#pragma unroll 1
    for (int rb = 0; rb < 16; rb += KM_RB) {
        const int rloc = wave * 16 + rb;
        T acc[KM_RB][VEC];
#pragma unroll
        for (int r = 0; r < KM_RB; ++r)
#pragma unroll
            for (int v = 0; v < VEC; ++v) acc[r][v] = (T)0;

        if (MODE == 4) {
            // d == 1: acc holds the signed difference
#pragma unroll
            for (int r = 0; r < KM_RB; ++r)
#pragma unroll
                for (int v = 0; v < VEC; ++v) acc[r][v] = s1[rloc + r] - s2[cbase + v];
        } else {
            // the row points are the same for every lane of a wave: they come through the scalar cache into SGPRs
            // (wave-uniform addresses), not as four 512-byte LDS broadcasts per coordinate -- with those the LDS return
            // path, shared by the four SIMDs, was the bound (24 of its cycles per 64 VALU cycles and SIMD)
            const T *arow[KM_RB];
#pragma unroll
            for (int r = 0; r < KM_RB; ++r)
                arow[r] = x1 + min(row0 + wave_u * 16 + rb + r, n - 1) * d;
#pragma unroll 4
            for (int k = 0; k < d; ++k) {
                T b[VEC];
#pragma unroll
                for (int v = 0; v < VEC; ++v) b[v] = s2[(size_t)k * TNP + cbase + v];
#pragma unroll
                for (int r = 0; r < KM_RB; ++r) {
                    const T a = arow[r][k];
#pragma unroll
                    for (int v = 0; v < VEC; ++v) acc[r][v] = pair_term<T, KIND>(a, b[v], (T)kp.c[2], acc[r][v]);
                }
            }
        }

        if (interior) {
            // the tile lies strictly inside the matrix and off the diagonal: no row / column bounds, no
            // diagonal test, one 16-byte store per lane and row (the guarded path below costs ~30 more vector
            // instructions per entry: per-element predicates and the byte-wise assembly of a partial store)
#pragma unroll
            for (int r = 0; r < KM_RB; ++r) {
                typename Vec<T>::type pk;
                T *pv = reinterpret_cast<T *>(&pk);
#pragma unroll
                for (int v = 0; v < VEC; ++v) {
                    if (MODE <= 2) {
                        pv[v] = gaussian_entry<T, MODE>(acc[r][v], c1, c2, c3, c4);
                    } else if (MODE == 3) {
                        pv[v] = periodic_k<T>(acc[r][v], (T)kp.c[0], (T)kp.c[1]);
                    } else {
                        pv[v] = periodic_entry<T>(kp.member, acc[r][v], (T)kp.c[0], (T)kp.c[1], (T)kp.c[2]);
                    }
                }
                *reinterpret_cast<typename Vec<T>::type *>(out + (row0 + rloc + r) * ld + col0 + cbase) = pk;
            }
            continue;
        }
#pragma unroll
        for (int r = 0; r < KM_RB; ++r) {
            const int64_t gi = row0 + rloc + r;
            if (gi >= n) continue;
            T val[VEC];
#pragma unroll
            for (int v = 0; v < VEC; ++v) {
                T x;
                if (MODE <= 2) {
                    x = gaussian_entry<T, MODE>(acc[r][v], c1, c2, c3, c4);
                } else if (MODE == 3) {
                    x = periodic_k<T>(acc[r][v], (T)kp.c[0], (T)kp.c[1]);
                } else {
                    x = periodic_entry<T>(kp.member, acc[r][v], (T)kp.c[0], (T)kp.c[1], (T)kp.c[2]);
                }
                if (gi == col0 + cbase + v) x += dadd;
                val[v] = x;
            }
            T *dst = out + gi * ld + col0 + cbase;
            if (aligned && col0 + cbase + VEC <= m) {
                typename Vec<T>::type pk;
                memcpy(&pk, val, sizeof(pk));
                *reinterpret_cast<typename Vec<T>::type *>(dst) = pk;
            } else {
#pragma unroll
                for (int v = 0; v < VEC; ++v)
                    if (col0 + cbase + v < m) dst[v] = val[v];
            }
        }
    }
  }
}

template <typename T>
static int launch_kmat(const void *x1, int64_t n, const void *x2, int64_t m, int d,
                       const KParams &kp, int tri, void *out, int64_t ld, hipStream_t st)
{
    constexpr int VEC = Vec<T>::N;
    constexpr int TN = 64 * VEC;
    int mode;
    if (kp.kernel == GPX_KERNEL_GAUSSIAN) mode = (int)kp.c[4];
    else mode = (kp.member == GPX_K) ? 3 : 4;
    if (mode == 4 && d != 1) {
        set_error("periodic derivative members need d == 1 (got %d)", d);
        return GPX_ERR_UNSUPPORTED;
    }
    const size_t smem = ((mode == 4 ? (size_t)KM_ROWS * d : (size_t)0) + (size_t)d * (TN + VEC)) * sizeof(T);
    if (smem > (size_t)LDS_CHUNK_MAX) {
        set_error("kmat: d = %d too large for the LDS-staged tile (96 KiB of column points)", d);
        return GPX_ERR_UNSUPPORTED;
    }
    const int aligned = (ld % VEC == 0) && (((uintptr_t)out) % 16 == 0);
    // four row blocks per workgroup once that still leaves several workgroups per CU
    const int rblk = (mode != 4 && cdiv(m, TN) * cdiv(n, 4 * KM_ROWS) >= 2048) ? 4 : 1;
    dim3 grid((unsigned)cdiv(m, TN), (unsigned)cdiv(n, (int64_t)KM_ROWS * rblk));
    dim3 block(256);
    const T *a = (const T *)x1;
    const T *b = (const T *)x2;
    T *o = (T *)out;
    double bytes = 0;
    if (g_prof_on) {
        // bytes actually written: every tile that is not strictly above the diagonal
        for (int64_t r0 = 0; r0 < n; r0 += KM_ROWS) {
            const int64_t rows = std::min<int64_t>(KM_ROWS, n - r0);
            int64_t cols = m;
            if (tri == GPX_LOWER) cols = std::min<int64_t>(m, ((r0 + KM_ROWS - 1) / TN + 1) * TN);
            bytes += (double)rows * cols * sizeof(T);
        }
    }
    ProfScope prof(PC_KMAT, bytes, st);
#define GPX_KM_LAUNCH(MODE)                                                                   \
    do {                                                                                      \
        if (smem > 48 * 1024) GPX_TRY(set_max_lds((const void *)kmat_kernel<T, MODE>, LDS_CHUNK_MAX)); \
        hipLaunchKernelGGL((kmat_kernel<T, MODE>), grid, block, smem, st, a, n, b, m, d, kp,  \
                           tri, aligned, o, ld, rblk);                                        \
    } while (0)
    switch (mode) {
    case 0: GPX_KM_LAUNCH(0); break;
    case 1: GPX_KM_LAUNCH(1); break;
    case 2: GPX_KM_LAUNCH(2); break;
    case 3: GPX_KM_LAUNCH(3); break;
    default: GPX_KM_LAUNCH(4); break;
    }
#undef GPX_KM_LAUNCH
    GPX_LAUNCH_CHECK();
    return GPX_OK;
}

// ---------------------------------------------------------------------------
// Gaussian ARD (GPX_KERNEL_GAUSSIAN_ARD): k(a, b; h, w) = k_gaussian(a / w, b / w; h / sqrt(wbar), 1), so every build and
// every prediction of the family runs the kernels above on SCALED points.  scale_points_kernel makes them: one thread per
// point, the widths as a kernel argument read with a wave-uniform index (scalar loads), a true division (the fp64 result
// is the correctly rounded quotient, numpy's x / w bit for bit).  In place is fine: a thread reads an element before
// it writes it and nobody else touches it.
// ---------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void scale_points_kernel(const T *x, int64_t n, int d, ArdWidths aw, T *out)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    for (int k = 0; k < d; ++k) out[i * d + k] = x[i * d + k] / (T)aw.w[k];
}

void ard_iso(const double *params, int d, double *iso2)
{
    double sl = 0.0;
    for (int k = 0; k < d; ++k) sl += log(params[1 + k]);
    iso2[0] = params[0] / sqrt(exp(sl / (double)d));
    iso2[1] = 1.0;
}

int scale_points(int dtype, const void *x, int64_t n, int d, const double *w_host, void *out, hipStream_t st)
{
    if (d < 1 || d > GPX_ARD_MAX_D) { set_error("scale_points: need 1 <= d <= %d (got %d)", GPX_ARD_MAX_D, d); return GPX_ERR_ARG; }
    if (n <= 0) return GPX_OK;
    ArdWidths aw;
    for (int k = 0; k < GPX_ARD_MAX_D; ++k) aw.w[k] = k < d ? w_host[k] : 1.0;
    const dim3 grid((unsigned)cdiv(n, 256)), block(256);
    return by_dtype(dtype, [&](auto t) -> int {
        using T = decltype(t);
        hipLaunchKernelGGL((scale_points_kernel<T>), grid, block, 0, st, (const T *)x, n, d, aw, (T *)out);
        GPX_LAUNCH_CHECK();
        return GPX_OK;
    });
}

static thread_local ThreadScratch g_ard_scr;    // gpx_d_kmat and gpx_d_pred_grad on the ARD family: the scaled copies of their two point sets
int ard_scratch(size_t bytes, void **p) { return g_ard_scr.get(bytes, p); }

const double *reduce_params(int kernel, int d, const double *params, double *iso2)
{
    if (kernel != GPX_KERNEL_GAUSSIAN_ARD) return params;
    ard_iso(params, d, iso2);
    return iso2;
}

// ---------------------------------------------------------------------------
// The tile reductions (gp/ext/gp_c.pyx:34-49 without its dense products): sums of a coefficient against the kernel's
// derivatives over the entries of a kernel matrix,
//   out[p] = sum_{j,i} coef_ji * dk_p(row_j, col_i)      p < n_kp,
// with the derivatives evaluated on the fly from the squared distance (no Jacobian is materialised) and ONE matrix M that is
// in memory and read once.  Deterministic: a fixed grid of workgroups walks the 64 x 64 tiles in a fixed order (a thread owns
// one column and 16 rows of a tile), per-workgroup partial sums are written out and added up by the host in index order; f64
// sums for both dtypes, no atomics.  FORM selects the pass.  It guards the tile decode, the column set, the staged vectors,
// the entry guard, the coefficient and the last slot -- nothing else differs, and each instantiation holds exactly one form of
// each:
//   TILE_ML    marginal likelihood: K(x, x), symmetric.  G = a a^T - M, a = alpha, M = W = K^-1 (lower triangle read; G and
//              dK_p are symmetric, so the sum runs over the lower triangle with weight wt = 2 off the diagonal):
//              coef = wt (a_r a_c - M_rc); last slot tr M
//   TILE_LOO   leave-one-out (RW06 eq. 5.13 rearranged; gpx_loograd.hip has the derivation): the same with
//              G = (b a^T + a b^T) / 2 - M, a = alpha, b = r, M = Pm = K^-1 diag(c) K^-1
//   TILE_RECT  the sparse GP's gradient (gpx_sparse.hip): K(x, z), rows x_j (n of them, a column chunk of the data), columns z_i
//              (m inducing points); no symmetry, so no weights and no triangle: every tile of the rectangle, row by row.
//              coef = M_ji + y_j w_i  (M = P, n x ldm; y over the rows, w over the columns); last slot sum coef k(x_j, z_i)
//              (the ARD kernel has that as S_0 already and leaves the slot zero)
// tile_reduce_ard_kernel is ONE text for the three forms; of the isotropic kernel only the two symmetric forms are one text,
// tile_reduce_kernel, and the rectangular one is rect_tile_kernel (as a third form its fp32 instantiation was slower: DESIGN 3.3).
// (FORM as a template parameter and not a __device__ helper around the shared text: the instantiations keep the resource
// lines the separate kernels had)
// ---------------------------------------------------------------------------
enum { TILE_ML = 1, TILE_LOO = 2, TILE_RECT = 3 };

// What only one form reads, as ONE kernel argument specialised per form: the staged vectors, and for TILE_RECT the second
// point set and the tiles of a row.  No form carries a field it does not read (TILE_ML takes no second vector and reserves no
// LDS for one), so the symmetric instantiations have the argument block of the kernels they replaced: with an unused `vec_b`
// in the list the isotropic marginal-likelihood kernel was scheduled differently and measured 2 - 6 % slower.
template <typename T, int FORM> struct TileArgs;
template <typename T> struct TileArgs<T, TILE_ML> { const T *a; };
template <typename T> struct TileArgs<T, TILE_LOO> { const T *a, *b; };
template <typename T> struct TileArgs<T, TILE_RECT> { const T *z; int64_t m; const T *y, *w; int64_t ntiles_c; };

// the origin of tile t: the lower triangle of the tiles of a symmetric pass (tri_tile), the rectangle's tiles row by row
template <typename T, int FORM>
__device__ __forceinline__ void tile_origin(const TileArgs<T, FORM> &a, int64_t t, int64_t *r0, int64_t *c0)
{
    int64_t tr, tc;
    if constexpr (FORM == TILE_RECT) { tr = t / a.ntiles_c; tc = t - tr * a.ntiles_c; }
    else tri_tile(t, &tr, &tc);
    *r0 = tr * GR_T;
    *c0 = tc * GR_T;
}

// the staged vectors of a tile, by the first GR_T threads: a over the rows (below n) and over the columns (below nc) -- y and w
// for TILE_RECT -- and for TILE_LOO b behind them
template <typename T, int FORM>
__device__ __forceinline__ void stage_tile_vecs(const TileArgs<T, FORM> &a, T *sa1, int tid, int64_t r0, int64_t n, int64_t c0, int64_t nc)
{
    if (tid >= GR_T) return;
    const T *vr, *vc;
    if constexpr (FORM == TILE_RECT) { vr = a.y; vc = a.w; }
    else { vr = a.a; vc = a.a; }
    sa1[tid] = (r0 + tid < n) ? vr[r0 + tid] : (T)0;
    sa1[GR_T + tid] = (c0 + tid < nc) ? vc[c0 + tid] : (T)0;
    if constexpr (FORM == TILE_LOO) {
        sa1[2 * GR_T + tid] = (r0 + tid < n) ? a.b[r0 + tid] : (T)0;
        sa1[3 * GR_T + tid] = (c0 + tid < nc) ? a.b[c0 + tid] : (T)0;
    }
}

// The isotropic kernel of the two SYMMETRIC forms (TILE_ML, TILE_LOO; the rectangular pass of these families is
// rect_tile_kernel below).  nt: the tile rows; the pass walks nt (nt + 1) / 2 tiles
template <typename T, int FORM>
__global__ __launch_bounds__(256) void tile_reduce_kernel(const T *__restrict__ x, int64_t n, int d, TileArgs<T, FORM> a,
                                                          const T *__restrict__ M, int64_t ldm, GradParams gp, int64_t nt,
                                                          double *__restrict__ partial)
{
    static_assert(FORM == TILE_ML || FORM == TILE_LOO, "the symmetric forms");
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    T *s1 = reinterpret_cast<T *>(smem_raw);          // [GR_T][d]   rows
    T *s2 = s1 + (size_t)GR_T * d;                    // [d][GR_T]   columns, transposed
    T *sa1 = s2 + (size_t)GR_T * d;                   // a rows
    T *sa2 = sa1 + GR_T;                              // a cols
    T *sb1 = sa2 + GR_T;                              // b rows  (TILE_LOO)
    T *sb2 = sb1 + GR_T;                              // b cols
    __shared__ double red[4][4];
    const int tid = threadIdx.x, col = tid & 63, rg = tid >> 6;
    double acc[4] = {0.0, 0.0, 0.0, 0.0};             // up to 3 kernel params + trace
    const int64_t total = nt * (nt + 1) / 2;
    for (int64_t t = blockIdx.x; t < total; t += gridDim.x) {
        int64_t r0, c0;
        tile_origin(a, t, &r0, &c0);
        __syncthreads();
        for (int idx = tid; idx < GR_T * d; idx += 256) {
            const int r = idx / d, k = idx - r * d;
            s1[idx] = (r0 + r < n) ? x[(r0 + r) * d + k] : (T)0;
            s2[(size_t)k * GR_T + r] = (c0 + r < n) ? x[(c0 + r) * d + k] : (T)0;
        }
        stage_tile_vecs(a, sa1, tid, r0, n, c0, n);
        __syncthreads();
        const int64_t gc = c0 + col;
        const T ak = sa2[col];
        const double bk = FORM == TILE_LOO ? (double)sb2[col] : 0.0;
        for (int i = 0; i < 16; ++i) {
            const int r = rg + 4 * i;
            const int64_t gr = r0 + r;
            if (gr >= n || gc >= n || gc > gr) continue;
            const double wt = (gc == gr) ? 1.0 : 2.0;
            const double mjk = (double)M[gr * ldm + gc];
            const double coef = FORM == TILE_ML ? wt * ((double)sa1[r] * (double)ak - mjk)
                                                : wt * (0.5 * ((double)sb1[r] * (double)ak + (double)sa1[r] * bk) - mjk);
            if (gc == gr) acc[3] += mjk;
            if (gp.kernel == GPX_KERNEL_GAUSSIAN) {
                T d2 = (T)0;
                for (int k = 0; k < d; ++k) {
                    const T tt = s1[r * d + k] - s2[(size_t)k * GR_T + col];
                    d2 = fma(tt, tt, d2);
                }
                const double e = gp.c1 * (double)d2;
                if (!(e < GPX_MIN_LOG)) {
                    const double ex = exp(e);
                    acc[0] += coef * (gp.c2h * ex);
                    acc[1] += coef * (ex * (gp.c3w * (double)d2 - gp.c2w));
                }
            } else {
                const T dd = s1[r] - s2[col];          // d == 1
                acc[0] += coef * (double)periodic_entry<T>(GPX_DK_DH, dd, (T)gp.h, (T)gp.w, (T)gp.p);
                acc[1] += coef * (double)periodic_entry<T>(GPX_DK_DW, dd, (T)gp.h, (T)gp.w, (T)gp.p);
                acc[2] += coef * (double)periodic_entry<T>(GPX_DK_DP, dd, (T)gp.h, (T)gp.w, (T)gp.p);
            }
        }
    }
    block_sum_fixed(acc, red, tid);
    __syncthreads();
    if (tid < 4) partial[(int64_t)blockIdx.x * 4 + tid] = block_sum_final(red, tid);
}

// The isotropic kernel of TILE_RECT: the text above with the rectangle's tile decode, column set, staged vectors, entry guard,
// coefficient and last slot (ck: the Gaussian k's constant; total: the tiles).  It is a kernel of its own and not a third FORM
// of tile_reduce_kernel because as one its fp32 instantiation measured 4 - 6 % slower on the MI355X with the same instructions in
// the tile loop; the ARD kernel below serves all three forms.
template <typename T>
__global__ __launch_bounds__(256) void rect_tile_kernel(const T *__restrict__ x, int64_t n, const T *__restrict__ z, int64_t m, int d,
                                                          const T *__restrict__ P, int64_t ldp, const T *__restrict__ y,
                                                          const T *__restrict__ w, GradParams gp, double ck, int64_t ntiles_c,
                                                          int64_t total, double *__restrict__ partial)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    T *s1 = reinterpret_cast<T *>(smem_raw);          // [GR_T][d]   rows (x)
    T *s2 = s1 + (size_t)GR_T * d;                    // [d][GR_T]   columns (z), transposed
    T *sy = s2 + (size_t)GR_T * d;                    // y rows
    T *sw = sy + GR_T;                                // w cols
    __shared__ double red[4][4];
    const int tid = threadIdx.x, col = tid & 63, rg = tid >> 6;
    double acc[4] = {0.0, 0.0, 0.0, 0.0};             // up to 3 kernel params + the sum against k
    for (int64_t t = blockIdx.x; t < total; t += gridDim.x) {
        const int64_t tr = t / ntiles_c, tc = t - tr * ntiles_c;
        const int64_t r0 = tr * GR_T, c0 = tc * GR_T;
        __syncthreads();
        for (int idx = tid; idx < GR_T * d; idx += 256) {
            const int r = idx / d, k = idx - r * d;
            s1[idx] = (r0 + r < n) ? x[(r0 + r) * d + k] : (T)0;
            s2[(size_t)k * GR_T + r] = (c0 + r < m) ? z[(c0 + r) * d + k] : (T)0;
        }
        if (tid < GR_T) {
            sy[tid] = (r0 + tid < n) ? y[r0 + tid] : (T)0;
            sw[tid] = (c0 + tid < m) ? w[c0 + tid] : (T)0;
        }
        __syncthreads();
        const int64_t gc = c0 + col;
        const double wk = (double)sw[col];
        for (int i = 0; i < 16; ++i) {
            const int r = rg + 4 * i;
            const int64_t gr = r0 + r;
            if (gr >= n || gc >= m) continue;
            const double coef = (double)P[gr * ldp + gc] + (double)sy[r] * wk;
            if (gp.kernel == GPX_KERNEL_GAUSSIAN) {
                T d2 = (T)0;
                for (int k = 0; k < d; ++k) {
                    const T tt = s1[r * d + k] - s2[(size_t)k * GR_T + col];
                    d2 = fma(tt, tt, d2);
                }
                const double e = gp.c1 * (double)d2;
                if (!(e < GPX_MIN_LOG)) {
                    const double ex = exp(e);
                    acc[0] += coef * (gp.c2h * ex);
                    acc[1] += coef * (ex * (gp.c3w * (double)d2 - gp.c2w));
                    acc[3] += coef * (ck * ex);
                }
            } else {
                const T dd = s1[r] - s2[col];          // d == 1
                acc[0] += coef * (double)periodic_entry<T>(GPX_DK_DH, dd, (T)gp.h, (T)gp.w, (T)gp.p);
                acc[1] += coef * (double)periodic_entry<T>(GPX_DK_DW, dd, (T)gp.h, (T)gp.w, (T)gp.p);
                acc[2] += coef * (double)periodic_entry<T>(GPX_DK_DP, dd, (T)gp.h, (T)gp.w, (T)gp.p);
                acc[3] += coef * (double)periodic_entry<T>(GPX_K, dd, (T)gp.h, (T)gp.w, (T)gp.p);
            }
        }
    }
    block_sum_fixed(acc, red, tid);
    __syncthreads();
    if (tid < 4) partial[(int64_t)blockIdx.x * 4 + tid] = block_sum_final(red, tid);
}

// ---------------------------------------------------------------------------
// The same pass for the Gaussian ARD family (d + 1 kernel parameters): with t_k = (a_k - b_k) / w_k (the difference of the
// SCALED points) and c_ab = coef_ab k_ab (coef as above, by FORM) it accumulates
//   S_0 = sum c_ab,   S_k = sum c_ab t_k^2  (k = 1 .. d),   the last slot (tr M; TILE_RECT: 0)
// from which the host forms the gradient (dk/dh = 2k/h, dk/dw_k = k (t_k^2 - 1/d) / w_k: grad_from_sums).
// One read of M, nothing n x n x d anywhere, no atomics; the same fixed grid, tile walk and host summation as above, f64
// sums for both dtypes: bitwise repeatable.
// Per tile a thread (one column, 16 rows) first forms its 16 weights c_ab -- squared distance in T as the matrix build
// forms it, one exp each -- and keeps them in registers, then walks the dimensions once more: S_k += sum_i c_i t_ik^2.
// d is a run-time value and d accumulators indexed by a loop variable would live in scratch memory, so the kernel is
// compiled for DMAX = 8, 16, 32, 64 accumulators and that loop is unrolled over DMAX with a uniform `k < d` guard: every
// acc[k] is a register (no scratch: see DESIGN 3.4 for the compiler's resource line).  The staged points are zero beyond d.
// S_0, the S_k and the last slot share ONE register array, so the block sum is the shared helper's.
// ---------------------------------------------------------------------------
template <typename T, int DMAX, int FORM>
__global__ __launch_bounds__(256) void tile_reduce_ard_kernel(const T *__restrict__ xs, int64_t n, int d, TileArgs<T, FORM> a,
                                                              const T *__restrict__ M, int64_t ldm, double c2, int64_t nt,
                                                              double *__restrict__ partial)
{
    constexpr bool RECT = FORM == TILE_RECT;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    T *s1 = reinterpret_cast<T *>(smem_raw);          // [GR_T][DMAX]   rows
    T *s2 = s1 + (size_t)GR_T * DMAX;                 // [DMAX][GR_T]   columns, transposed
    T *sa1 = s2 + (size_t)GR_T * DMAX;                // a rows  (TILE_RECT: y)
    T *sa2 = sa1 + GR_T;                              // a cols  (TILE_RECT: w)
    T *sb1 = sa2 + GR_T;                              // b rows  (TILE_LOO)
    T *sb2 = sb1 + GR_T;                              // b cols
    __shared__ double red[4][DMAX + 2];
    const int tid = threadIdx.x, col = tid & 63;
    const int rg = __builtin_amdgcn_readfirstlane(tid >> 6);      // (the wave's index: uniform, so the row reads broadcast)
    const T *xc = xs;                                 // the columns' points and their count
    int64_t nc = n;
    if constexpr (RECT) { xc = a.z; nc = a.m; }
    double acc[DMAX + 2];                             // slot 0: S_0, 1 .. DMAX: S_k, DMAX + 1: the last slot
#pragma unroll
    for (int k = 0; k < DMAX + 2; ++k) acc[k] = 0.0;
    const int64_t total = RECT ? nt : nt * (nt + 1) / 2;
    for (int64_t t = blockIdx.x; t < total; t += gridDim.x) {
        int64_t r0, c0;
        tile_origin(a, t, &r0, &c0);
        __syncthreads();
        for (int idx = tid; idx < GR_T * DMAX; idx += 256) {
            const int r = idx / DMAX, k = idx - r * DMAX;
            s1[idx] = (k < d && r0 + r < n) ? xs[(r0 + r) * d + k] : (T)0;
            s2[(size_t)k * GR_T + r] = (k < d && c0 + r < nc) ? xc[(c0 + r) * d + k] : (T)0;
        }
        stage_tile_vecs(a, sa1, tid, r0, n, c0, nc);
        __syncthreads();
        const int64_t gc = c0 + col;
        // the squared distances of this thread's 16 entries, accumulated as kmat_kernel accumulates them
        T r2[16];
#pragma unroll
        for (int i = 0; i < 16; ++i) r2[i] = (T)0;
#pragma unroll 2
        for (int k = 0; k < d; ++k) {
            const T b = s2[(size_t)k * GR_T + col];
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const T tt = s1[(rg + 4 * i) * DMAX + k] - b;
                r2[i] = fma(tt, tt, r2[i]);
            }
        }
        // the weights c_ab (0 for an entry outside the matrix or, in a symmetric pass, above the diagonal: M is only read inside)
        double c[16];
        const double ak = (double)sa2[col], bk = FORM == TILE_LOO ? (double)sb2[col] : 0.0;
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int r = rg + 4 * i;
            const int64_t gr = r0 + r;
            double ci = 0.0;
            if (gr < n && (RECT ? gc < nc : gc <= gr)) {
                const double mjk = (double)M[gr * ldm + gc];
                double coef;
                if constexpr (RECT) {
                    coef = mjk + (double)sa1[r] * ak;
                } else {
                    const double wt = (gc == gr) ? 1.0 : 2.0;
                    coef = FORM == TILE_ML ? wt * ((double)sa1[r] * ak - mjk)
                                           : wt * (0.5 * ((double)sb1[r] * ak + (double)sa1[r] * bk) - mjk);
                    if (gc == gr) acc[DMAX + 1] += mjk;
                }
                const double e = -0.5 * (double)r2[i];
                if (!(e < GPX_MIN_LOG)) ci = coef * (c2 * exp(e));
            }
            c[i] = ci;
            acc[0] += ci;
        }
#pragma unroll
        for (int k = 0; k < DMAX; ++k) {
            if (k < d) {
                const T b = s2[(size_t)k * GR_T + col];
                double a2 = 0.0;
#pragma unroll
                for (int i = 0; i < 16; ++i) {
                    const double tt = (double)(s1[(rg + 4 * i) * DMAX + k] - b);
                    a2 = fma(c[i], tt * tt, a2);
                }
                acc[1 + k] += a2;
            }
        }
    }
    block_sum_fixed(acc, red, tid);
    __syncthreads();
    if (tid < d + 2) partial[(int64_t)blockIdx.x * (d + 2) + tid] = block_sum_final(red, tid <= d ? tid : DMAX + 1);
}

// the partial sums of `width` quantities per workgroup, added on the host in workgroup order
static int sum_partials(const double *partial_dev, int width, double *out, hipStream_t st)
{
    std::vector<double> host((size_t)GR_BLOCKS * width);
    GPX_HIP(hipMemcpyAsync(host.data(), partial_dev, host.size() * sizeof(double), hipMemcpyDeviceToHost, st));
    GPX_HIP(hipStreamSynchronize(st));
    for (int q = 0; q < width; ++q) {
        double v = 0.0;
        for (int b = 0; b < GR_BLOCKS; ++b) v += host[(size_t)b * width + q];
        out[q] = v;
    }
    return GPX_OK;
}

int make_grad_params(int kernel, int d, const double *params, GradParams *gpar)
{
    memset(gpar, 0, sizeof(*gpar));
    gpar->kernel = kernel;
    if (kernel == GPX_KERNEL_GAUSSIAN) {
        const double h = params[0], w = params[1], S = sqrt(2.0 / M_PI);
        gpar->nkp = 2;
        gpar->c1 = -0.5 / (w * w);
        gpar->c2h = S * h / w;                         // gaussian_c.pyx:61
        gpar->c2w = 0.5 * S * h * h / (w * w);         // :82
        gpar->c3w = 0.5 * S * h * h / pow(w, 4);       // :83
    } else {
        if (d != 1) { set_error("periodic gradient needs d == 1"); return GPX_ERR_UNSUPPORTED; }
        gpar->nkp = 3; gpar->h = params[0]; gpar->w = params[1]; gpar->p = params[2];
    }
    return GPX_OK;
}

// the dynamic LDS of a tile: two staged point sets of dk coordinates (d, or the ARD kernels' DMAX) and nvec vectors
static int tile_lds(int dk, int nvec, size_t es, size_t *bytes)
{
    *bytes = ((size_t)2 * GR_T * dk + (size_t)nvec * GR_T) * es;
    if (*bytes <= (size_t)LDS_TILE_MAX) return GPX_OK;
    set_error("tile reduction: d = %d too large for the LDS-staged tile", dk);
    return GPX_ERR_UNSUPPORTED;
}

// one launch of the family's kernel for the form; kernel == GPX_KERNEL_GAUSSIAN_ARD: the points are the SCALED ones and params = iso
template <typename T, int FORM>
static int launch_tile_reduce(int kernel, const void *x, int64_t n, int d, const double *params, const TileArgs<T, FORM> &a, const void *M,
                              int64_t ldm, int64_t nt, double *partial_dev, hipStream_t st)
{
    constexpr int NVEC = FORM == TILE_LOO ? 4 : 2;
    const dim3 grid((unsigned)std::min<int64_t>(GR_BLOCKS, FORM == TILE_RECT ? nt : nt * (nt + 1) / 2)), block(256);
    size_t smem = 0;
    if (kernel == GPX_KERNEL_GAUSSIAN_ARD) {
        const double c2 = gaussian_k_const(params[0], params[1]);
        return by_dmax(d, [&](auto dm) -> int {
            constexpr int DMAX = decltype(dm)::value;
            GPX_TRY(tile_lds(DMAX, NVEC, sizeof(T), &smem));
            if (smem > 48 * 1024) GPX_TRY(set_max_lds((const void *)tile_reduce_ard_kernel<T, DMAX, FORM>, LDS_TILE_MAX));
            hipLaunchKernelGGL((tile_reduce_ard_kernel<T, DMAX, FORM>), grid, block, smem, st, (const T *)x, n, d, a, (const T *)M, ldm,
                               c2, nt, partial_dev);
            GPX_LAUNCH_CHECK();
            return GPX_OK;
        });
    }
    GradParams gpar;
    GPX_TRY(make_grad_params(kernel, d, params, &gpar));
    GPX_TRY(tile_lds(d, NVEC, sizeof(T), &smem));
    if constexpr (FORM == TILE_RECT) {
        const double ck = kernel == GPX_KERNEL_GAUSSIAN ? gaussian_k_const(params[0], params[1]) : 0.0;
        if (smem > 48 * 1024) GPX_TRY(set_max_lds((const void *)rect_tile_kernel<T>, LDS_TILE_MAX));
        hipLaunchKernelGGL((rect_tile_kernel<T>), grid, block, smem, st, (const T *)x, n, a.z, a.m, d, (const T *)M, ldm, a.y, a.w, gpar, ck,
                           a.ntiles_c, nt, partial_dev);
    } else {
        if (smem > 48 * 1024) GPX_TRY(set_max_lds((const void *)tile_reduce_kernel<T, FORM>, LDS_TILE_MAX));
        hipLaunchKernelGGL((tile_reduce_kernel<T, FORM>), grid, block, smem, st, (const T *)x, n, d, a, (const T *)M, ldm, gpar, nt,
                           partial_dev);
    }
    GPX_LAUNCH_CHECK();
    return GPX_OK;
}

size_t dloglh_partial_doubles(int kernel, int d) { return (size_t)GR_BLOCKS * (kernel == GPX_KERNEL_GAUSSIAN_ARD ? d + 2 : 4); }

// what both host entries do around their launch: the ARD family's range of d, the cleared partials, the profile scope, the
// host's sum of the partials into out (dloglh_partial_doubles() / GR_BLOCKS values)
template <typename L>
static int tile_pass(int prof_class, double work, int kernel, int d, double *partial_dev, double *out, hipStream_t st, L launch)
{
    if (kernel == GPX_KERNEL_GAUSSIAN_ARD && (d < 1 || d > GPX_ARD_MAX_D)) {
        set_error("ARD gradient needs 1 <= d <= %d (got %d)", GPX_ARD_MAX_D, d);
        return GPX_ERR_ARG;
    }
    const int width = (int)(dloglh_partial_doubles(kernel, d) / GR_BLOCKS);
    GPX_HIP(hipMemsetAsync(partial_dev, 0, (size_t)GR_BLOCKS * width * sizeof(double), st));
    {
        ProfScope prof(prof_class, work, st);
        GPX_TRY(launch());
    }
    return sum_partials(partial_dev, width, out, st);
}

int tile_reduce(int dtype, int kernel, const void *x, int64_t n, int d, const double *params, const void *vec_a, const void *vec_b,
                const void *M, int64_t ldm, double *partial_dev, double *out, hipStream_t st)
{
    // (the launch's lower triangle of M read once as its byte count)
    return tile_pass(PC_REDUCE, 0.5 * (double)n * (double)(n + 1) * (double)esize(dtype), kernel, d, partial_dev, out, st, [&] {
        return by_dtype(dtype, [&](auto t) -> int {
            using T = decltype(t);
            if (!vec_b) return launch_tile_reduce(kernel, x, n, d, params, TileArgs<T, TILE_ML>{(const T *)vec_a}, M, ldm, cdiv(n, GR_T), partial_dev, st);
            return launch_tile_reduce(kernel, x, n, d, params, TileArgs<T, TILE_LOO>{(const T *)vec_a, (const T *)vec_b}, M, ldm, cdiv(n, GR_T), partial_dev, st);
        });
    });
}

int rect_reduce(int dtype, int kernel, const void *x, int64_t n, const void *z, int64_t m, int d, const double *params, const void *P,
                int64_t ldp, const void *y, const void *w, double *partial_dev, double *out, hipStream_t st)
{
    if (n < 1 || m < 1 || ldp < m) { set_error("rect_reduce: need n, m >= 1 and ldp >= m"); return GPX_ERR_ARG; }
    return tile_pass(PC_SPARSE_GRAD, (double)n * (double)m, kernel, d, partial_dev, out, st, [&] {
        return by_dtype(dtype, [&](auto t) -> int {
            using T = decltype(t);
            const int64_t ntc = cdiv(m, GR_T);
            return launch_tile_reduce(kernel, x, n, d, params, TileArgs<T, TILE_RECT>{(const T *)z, m, (const T *)y, (const T *)w, ntc}, P, ldp,
                                      cdiv(n, GR_T) * ntc, partial_dev, st);
        });
    });
}


// The host half of either gradient: the sums of a pass -> (d/d kernel params ..., d/ds).  factor: 1/2 for the marginal
// likelihood (RW06 eq. 5.9), 1 for the leave-one-out criterion (dL = sum dK_ab G_ab); it enters only as a product by 1/2, 1 or
// 2, all exact, so each output is bit for bit the expression its criterion always computed.  quad: the vectors' part of tr G (alpha .
// alpha, r . alpha); noise_scale multiplies (quad - tr M)  (dK/ds = 2 s I, gp_c.pyx:46).
// ARD: dk/dh = 2 k / h, dk/dw_k = k (t_k^2 - 1 / d) / w_k on the scaled points.
void grad_from_sums(int kernel, int d, const double *params, const double *S, double quad, double noise_scale, double factor,
                    double *out)
{
    if (kernel == GPX_KERNEL_GAUSSIAN_ARD) {
        out[0] = (2.0 * factor) * S[0] / params[0];
        for (int k = 0; k < d; ++k) out[1 + k] = factor * (S[1 + k] / params[1 + k] - S[0] / ((double)d * params[1 + k]));
        out[d + 1] = noise_scale * (quad - S[d + 1]);
        return;
    }
    const int nkp = kernel == GPX_KERNEL_GAUSSIAN ? 2 : 3;
    for (int i = 0; i < nkp; ++i) out[i] = factor * S[i];
    out[nkp] = noise_scale * (quad - S[3]);
}

}  // namespace gpx

using namespace gpx;

extern "C" {

int gpx_d_kmat(int dtype, int kernel, int member, const void *x1, int64_t n, const void *x2,
               int64_t m, int d, const double *params, double diag_add, int tri, void *out,
               int64_t ld, void *stream)
{
    GPX_TRY(ensure_device());
    GPX_ARG(dtype == GPX_F64 || dtype == GPX_F32, "dtype must be GPX_F64 or GPX_F32");
    GPX_ARG(n >= 0 && m >= 0 && d >= 1, "need n, m >= 0 and d >= 1");
    GPX_ARG(ld >= m, "ld < m");
    GPX_ARG(tri == GPX_FULL || tri == GPX_LOWER, "tri must be GPX_FULL or GPX_LOWER");
    if (n == 0 || m == 0) return GPX_OK;
    GPX_ARG(x1 && x2 && out, "NULL pointer");
    if (kernel == GPX_KERNEL_GAUSSIAN_ARD) {
        // scale both point sets into this thread's scratch, then the isotropic build on (x1 / w, x2 / w; h / sqrt(wbar), 1)
        if (member != GPX_K) { set_error("the ARD family has no member %d (GPX_K only)", member); return GPX_ERR_UNSUPPORTED; }
        GPX_ARG(params, "params is NULL");
        GPX_ARG(d <= GPX_ARD_MAX_D, "the ARD family needs d <= GPX_ARD_MAX_D");
        gpx::StreamTurn turn__((hipStream_t)stream);     // (this thread's scratch buffers: one stream at a time, gpx_mem.h)
        const size_t es = esize(dtype), b1 = ((size_t)n * d * es + 255) / 256 * 256;
        const bool same = x2 == x1 && m == n;
        void *scr = nullptr;
        GPX_TRY(g_ard_scr.get(b1 + (same ? 0 : (size_t)m * d * es), &scr));
        void *s1 = scr, *s2 = same ? scr : (void *)((char *)scr + b1);
        GPX_TRY(scale_points(dtype, x1, n, d, params + 1, s1, S(stream)));
        if (!same) GPX_TRY(scale_points(dtype, x2, m, d, params + 1, s2, S(stream)));
        double iso[2];
        ard_iso(params, d, iso);
        return gpx_d_kmat(dtype, GPX_KERNEL_GAUSSIAN, member, s1, n, s2, m, d, iso, diag_add, tri, out, ld, stream);
    }
    KParams kp;
    GPX_TRY(make_kparams(kernel, member, params, diag_add, &kp));
    return by_dtype(dtype, [&](auto t) { return launch_kmat<decltype(t)>(x1, n, x2, m, d, kp, tri, out, ld, S(stream)); });
}

int gpx_d_scale_points(int dtype, const void *x, int64_t n, int d, const double *w_host, void *out, void *stream)
{
    GPX_TRY(ensure_device());
    GPX_ARG(dtype == GPX_F64 || dtype == GPX_F32, "dtype must be GPX_F64 or GPX_F32");
    GPX_ARG(n >= 0 && d >= 1 && d <= GPX_ARD_MAX_D, "need n >= 0 and 1 <= d <= GPX_ARD_MAX_D");
    if (n == 0) return GPX_OK;
    GPX_ARG(x && w_host && out, "NULL pointer");
    return scale_points(dtype, x, n, d, w_host, out, S(stream));
}

}  // extern "C"
