/*
 * gpx.h -- C ABI of libgpx.so: the MI355X (gfx950) GP regression core.
 *
 * This is the drop-in boundary for the GP fit/predict hot path of
 * jhamrick/gaussian_processes.  Every entry point names the reference interface
 * it replaces (paths relative to the reference tree):
 *
 *   gp/ext/gaussian_c.pyx   K, jacobian, hessian, dK_*, d2K_*      (Cython -> C)
 *   gp/ext/periodic_c.pyx   K, jacobian, hessian, dK_*, d2K_*
 *   gp/ext/gp_c.pyx         log_lh
 *   gp/gp.py:294            scipy.linalg.cholesky(Kxx, lower=True)     (LAPACK dpotrf)
 *   gp/gp.py:332-334        scipy.linalg.cho_solve((L, True), y)       (LAPACK dpotrs)
 *   gp/gp.py:311-312        inv(L).T @ inv(L)
 *   gp/gp.py:597, 622-625   posterior mean / covariance
 *
 * Conventions
 *   - plain C: pointers, sizes, scalars.  No torch / numpy types.
 *   - all matrices are ROW-MAJOR (numpy C order, as the reference's
 *     np.ndarray[float64, mode='c']); `ld` = elements between consecutive rows.
 *   - every function returns an int status: GPX_OK (0) or a negative GPX_ERR_*;
 *     gpx_last_error() gives the message (thread-local).  Factorisations report
 *     LAPACK-style `info` (> 0: that leading minor is not positive definite)
 *     through an out-parameter, not through the status.  A HOST-side info is
 *     never negative: an internal failure of the factorisation is the status
 *     GPX_ERR_INTERNAL.
 *   - check_finite: the reference factors with scipy's check_finite=True
 *     (gp/gp.py:294, 332-334) -- NaN / inf in the kernel matrix or in y raise
 *     ValueError("array must not contain infs or NaNs").  The handle does the
 *     same with one O(n d) device reduction over x and y per set_data and a host
 *     check of the kernel constants: gpx_gp_fit returns GPX_ERR_ARG with that
 *     text when x, a kernel parameter or s is not finite; every getter that
 *     involves y (alpha, log_lh, mean, the derivative stack) when y is not.
 *   - "device" entry points (gpx_d_*) take DEVICE pointers and a hipStream_t
 *     passed as void* (NULL = the null stream); they enqueue work and return.
 *     Device matrices must have ld % 16 == 0 and 16-byte aligned bases.
 *     Threading: the library keeps its scratch blocks, the look-ahead side
 *     stream and its event pool PER HOST THREAD.  Work one host thread issues on
 *     two streams therefore takes turns: gpx_d_potrf, gpx_d_potrf_panel,
 *     gpx_d_trsv_lower*, gpx_d_trsm_right_lt, gpx_d_mean* and every gpx_gp_* call
 *     on another stream than the thread's previous call first wait (on the device,
 *     not the host) for that call's work (round 4; before that it was the caller's
 *     duty, and gpx_gp_fit(gp, NULL) on several handles broke it).  Drive streams
 *     that should overlap from different host threads.  Nothing is ordered while a
 *     stream is being captured.  Since round 5 the multi-GPU handle's entries
 *     (gpx_mg_*, on the handle's update stream) and the host-array helpers gpx_cholesky /
 *     gpx_cho_solve (null stream) take their turn in the same way, and "another stream"
 *     is decided by the stream AND an epoch the library bumps whenever it destroys one
 *     (a new stream at a destroyed one's address is a different stream); streams the
 *     caller destroys with HIP directly are the caller's to order.  Handles
 *     (gpx_gp_*) remember the device they were created on and make it current
 *     for the duration of every call (the caller's current device is restored);
 *     they synchronise their stream before they return -- the one exception is
 *     gpx_gp_fit(gp, NULL), which only enqueues -- and different handles are
 *     safe to use concurrently from different host threads.
 *     The first factorisation a host thread issues creates that thread's look-ahead
 *     stream and scratch blocks: tens of ms once (measured with round 2's streams: 8 x n = 8192
 *     lock-step, 29 ms from a long-lived thread, 58 ms from a thread started per call)
 *     -- keep worker threads alive across calls.
 *   - "host" entry points (gpx_gaussian_c_*, gpx_periodic_c_*, gpx_gp_c_*,
 *     gpx_cholesky, gpx_cho_solve ...) take HOST pointers with the reference's
 *     exact argument meaning, run on the current device and return when the
 *     result is in the caller's buffer.
 *   - no CPU fallback exists: without a usable GPU every compute entry point
 *     returns GPX_ERR_NO_DEVICE.
 */
#ifndef GPX_H
#define GPX_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GPX_VERSION 100

/* status codes */
#define GPX_OK              0
#define GPX_ERR_ARG        -1   /* bad argument (maps to ValueError)              */
#define GPX_ERR_HIP        -2   /* HIP runtime failure (maps to RuntimeError)     */
#define GPX_ERR_NO_DEVICE  -3   /* no usable GPU                                  */
#define GPX_ERR_NOMEM      -4   /* device allocation failed                       */
#define GPX_ERR_UNSUPPORTED -5  /* combination not implemented                    */
#define GPX_ERR_INTERNAL   -6   /* the factorisation itself failed (a hand-off between workgroups of the resident
                                   panel kernel timed out: device info < 0).  Maps to RuntimeError -- it is never
                                   reported as "not positive definite" (info > 0) nor as log_lh = -inf        */

/* dtype */
#define GPX_F64 0
#define GPX_F32 1

/* kernel families (gp/kernels/gaussian.py, gp/kernels/periodic.py) */
#define GPX_KERNEL_GAUSSIAN 0   /* params = (h, w)    */
#define GPX_KERNEL_PERIODIC 1   /* params = (h, w, p) */
/* Gaussian with one length-scale per input dimension (ARD, RW06 eq. 5.1; an extension: the reference has none):
 *   k(a, b) = h^2 / sqrt(2 pi wbar^2) * exp(-1/2 sum_k ((a_k - b_k) / w_k)^2),   wbar = (prod_k w_k)^(1/d)
 * -- at equal widths exactly GPX_KERNEL_GAUSSIAN on (n, d) inputs.  Only the function itself is a member (GPX_K). */
#define GPX_KERNEL_GAUSSIAN_ARD 2   /* params = (h, w_1 ... w_d), 1 <= d <= GPX_ARD_MAX_D */
#define GPX_ARD_MAX_D 64

/* members of a kernel family: the function and its parameter derivatives.
 * Gaussian: gaussian_c.pyx:18-164.  Periodic: periodic_c.pyx:18-235. */
#define GPX_K          0
#define GPX_DK_DH      1
#define GPX_DK_DW      2
#define GPX_DK_DP      3   /* periodic only */
#define GPX_D2K_DHDH   4
#define GPX_D2K_DHDW   5   /* == d2K_dwdh */
#define GPX_D2K_DHDP   6   /* periodic only; == d2K_dpdh */
#define GPX_D2K_DWDW   7
#define GPX_D2K_DWDP   8   /* periodic only; == d2K_dpdw */
#define GPX_D2K_DPDP   9   /* periodic only */

/* triangle selector for symmetric builds */
#define GPX_FULL  0
#define GPX_LOWER 1   /* only tiles touching the lower triangle are written */

/* MIN = log(2^-1018): gp/gp.py:17, gaussian_c.pyx:15, gp_c.pyx:14 */
#define GPX_MIN_LOG (-705.6238298100243)

/* ---------------------------------------------------------------- runtime -- */
int         gpx_version(void);
const char *gpx_last_error(void);
int gpx_device_count(int *count);
int gpx_set_device(int device);
int gpx_get_device(int *device);
/* name: caller buffer; cus / clock_mhz / hbm_bytes may be NULL */
int gpx_device_info(int device, char *name, size_t name_len, int *cus,
                    int *clock_mhz, uint64_t *hbm_bytes);

int gpx_malloc(void **dptr, size_t bytes);
int gpx_free(void *dptr);
/* free / total HBM of the current device, bytes (hipMemGetInfo) */
int gpx_mem_info(size_t *free_bytes, size_t *total_bytes);
int gpx_memcpy_h2d(void *dst, const void *src, size_t bytes, void *stream);
int gpx_memcpy_d2h(void *dst, const void *src, size_t bytes, void *stream);
int gpx_memcpy_d2d(void *dst, const void *src, size_t bytes, void *stream);
/* strided copies: `rows` rows of `row_bytes`, pitches in bytes */
int gpx_memcpy2d_h2d(void *dst, size_t dpitch, const void *src, size_t spitch,
                     size_t row_bytes, size_t rows, void *stream);
int gpx_memcpy2d_d2h(void *dst, size_t dpitch, const void *src, size_t spitch,
                     size_t row_bytes, size_t rows, void *stream);
int gpx_memset(void *dst, int value, size_t bytes, void *stream);

int gpx_stream_create(void **stream);
int gpx_stream_destroy(void *stream);
int gpx_stream_sync(void *stream);
int gpx_device_sync(void);
int gpx_event_create(void **event);
int gpx_event_destroy(void *event);
int gpx_event_record(void *event, void *stream);
int gpx_event_sync(void *event);
int gpx_event_elapsed_ms(void *start, void *stop, float *ms);
int gpx_stream_wait_event(void *stream, void *event);

/* Live per-kernel-class timing.  When enabled every launch of the hot-path
 * kernels is bracketed by HIP events on its own stream; gpx_prof_read sums, per
 * class, the launches, their elapsed milliseconds and their ALGORITHMIC work
 * (flops for GPX_PROF_GEMM, bytes for the others).  bench.py derives
 * roofline.achieved from these. */
#define GPX_PROF_KMAT       0   /* bytes written                                  */
#define GPX_PROF_GEMM       1   /* gemm_nt_fast_kernel<T,128,1>: trailing updates (gpx_d_syrk_bc) on 128 x 128 tiles; flops: 2*K per updated element */
#define GPX_PROF_POTRF_DIAG 2   /* flops jb^3/3                                   */
#define GPX_PROF_TRSM_ROWS  3   /* flops rows*jb^2                                */
#define GPX_PROF_TRSV       4   /* bytes of L read                                */
#define GPX_PROF_MEAN       5   /* kernel evaluations m*n                         */
#define GPX_PROF_REDUCE     6   /* bytes read                                     */
#define GPX_PROF_GEMM_SKINNY  7 /* gemm_nt_fast_kernel<T,64> (panel products); flops */
#define GPX_PROF_GEMM_GENERIC 8 /* gemm_nt_kernel<T> (unaligned / K-tail shapes); flops */
#define GPX_PROF_GEMM_PANEL   9 /* gemm_nt_fast_kernel<T,128,0>: panel / covariance products; flops */
#define GPX_PROF_GEMM_N64    10 /* gemm_nt_fast_kernel<T,64,1>: trailing updates of few tiles on 128 x 64 tiles; flops */
#define GPX_PROF_TRANSPOSE   11 /* transpose_kernel: the row panels of L staged for X L^-1; bytes read + written */
#define GPX_PROF_PRED_GRAD   12 /* pred_grad_kernel + its slice reduction; kernel evaluations m*n per window of dimensions */
#define GPX_PROF_EXTEND      13 /* copy_lower_kernel + the fold of the Schur partials (gpx_gp_extend): bytes read + written */
#define GPX_PROF_RANDN       14 /* randn_kernel (gpx_d_randn): bytes written */
#define GPX_PROF_RFF         15 /* rff_features_kernel (gpx_d_rff_features): bytes written */
#define GPX_PROF_KAPPLY      16 /* stream_apply_kernel + its slice reduction (gpx_d_kmat_apply, fused route): kernel evaluations m*n per group of weight vectors */
#define GPX_PROF_KAPPLY_GRAD 17 /* stream_apply_grad_kernel + its slice reduction (gpx_d_kmat_apply_grad): kernel evaluations m*n per group of weight vectors and window of dimensions */
#define GPX_PROF_CHOL_DELETE 18 /* del_copy_rows_kernel + del_block_kernel (gpx_d_chol_delete), ONE record per call around all of its launches: bytes read + written */
#define GPX_PROF_SPARSE_GRAM 19 /* gpx_sgp_fit: the Gram product K(z, x_c) K(x_c, z) of ONE chunk, one record around all of its slice products; flops 2 c per element of the lower triangle.  (The product kernel's own launches are recorded under their classes as well.) */
#define GPX_PROF_SPARSE_GRAD 20 /* rect_tile_kernel / tile_reduce_ard_kernel in its rectangular form (gpx_sgp_grad): the rectangular tile reduction of ONE chunk; kernel-derivative evaluations c * M */
#define GPX_PROF_SPARSE_ZGRAD 21 /* rect_zgrad_kernel and its slice sum (gpx_sgp_grad_z, gpx_d_rect_zgrad): ONE pass of c rows against the M columns; kernel-derivative evaluations c * M per window of dimensions */
#define GPX_PROF_SELECT      22 /* select_pick_kernel + select_step_kernel (gpx_sgp_select), ONE record per call around all of its launches: bytes of R read and written, sizeof(T) n count (count + 1) / 2 */
#define GPX_PROF_CG          23 /* gpx_cg_solve, gpx_cg_var: ONE record per call around all of its launches (the product's and the blocks' own launches are recorded under their classes as well); kernel evaluations n^2 x iterations, summed over the groups of columns */
#define GPX_PROF_LOWRANK     24 /* lowrank_tile_kernel (gpx_d_lowrank_reduce, gpx_cg_lh): ONE launch of at most 32 rows of U and V; kernel-derivative evaluations n^2 */
int gpx_prof_enable(int on);    /* also clears the registry */
int gpx_prof_read(int cls, double *launches, double *total_ms, double *total_work);

/* Route counters: how often each of the alternative host-side routes was taken since the last reset (counted at
 * the point of decision, always on).  Every behaviour switch of the library is an environment variable; each entry point
 * takes one snapshot of them for the calling thread (csrc/gpx_tune.h); a test that forces a route
 * asserts it here. */
#define GPX_ROUTE_TRSV_OPS        0   /* single-rhs solve: operator form (one launch per 512-block step)      */
#define GPX_ROUTE_TRSV_STEPS      1   /* single-rhs solve: two launches per 512-block                         */
#define GPX_ROUTE_PANEL_RES       2   /* panel: the resident one-launch kernel                                */
#define GPX_ROUTE_PANEL_CHAIN     3   /* panel: 64-wide leaf + row substitution launches                      */
#define GPX_ROUTE_FIT_RIDE        4   /* fit: y rode along in the factorisation (forward solve folded in)     */
#define GPX_ROUTE_FIT_TWO_SOLVES  5   /* fit: forward and backward solve after the factorisation              */
#define GPX_ROUTE_GEMM_FAST       6   /* product on the LDS-DMA MFMA kernel                                   */
#define GPX_ROUTE_GEMM_GENERIC    7   /* product on the generic (unaligned / K-tail) kernel                   */
#define GPX_ROUTE_SYRK_EXACT      8   /* trailing update with the exact tile enumeration                      */
#define GPX_ROUTE_SYRK_PATCH      9   /* trailing update on the 1024 x 1024 patch grid                        */
#define GPX_ROUTE_MG_BCAST_ONE   10   /* multi-GPU panel broadcast: one collective per row chunk              */
#define GPX_ROUTE_MG_BCAST_SAG   11   /* multi-GPU panel broadcast: scatter + all-gather (point to point)     */
#define GPX_ROUTE_FIT_OPS_AHEAD  12   /* gpx_gp_fit: block operators of the solves built beside the factorisation */
#define GPX_ROUTE_TRSM_OPS       13   /* X L^-T (posterior covariance, inverse): in-block step as one product with inv(L_kk) */
#define GPX_ROUTE_POTRF_PAIR     14   /* a factorisation that entered the pair phase: far trailing updates of depth K = 2048, one per two panels */
#define GPX_ROUTE_VAR_CHUNK      15   /* predictive variance (gpx_gp_var, gpx_gp_var_from_K, gpx_mg_var): one hit per row chunk */
#define GPX_ROUTE_LOO_CHUNK      16   /* leave-one-out (gpx_gp_inv_diag, gpx_gp_loo): one hit per row chunk of the identity swept; none when the handle still has the diagonal */
#define GPX_ROUTE_TRSM_L_OPS     17   /* X L^-1 (gpx_gp_var_grad): in-block step as one product with inv(L_kk); one hit per sweep */
#define GPX_ROUTE_GRAD_CHUNK     18   /* input-space gradient of the variance (gpx_gp_var_grad): one hit per row chunk */
#define GPX_ROUTE_EXTEND         19   /* gpx_gp_extend / gpx_gp_extend_from_K: one hit per call                        */
#define GPX_ROUTE_SAMPLE         20   /* gpx_gp_sample / gpx_gp_sample_from_K: one hit per call                        */
#define GPX_ROUTE_KAPPLY_FUSED   21   /* gpx_d_kmat_apply: K(xo, x) V^T by the fused kernel, K never materialised; one hit per chunk */
#define GPX_ROUTE_KAPPLY_GEMM    22   /* gpx_d_kmat_apply: gpx_d_kmat into scratch, then gpx_d_gemm_nt; one hit per row chunk of xo  */
#define GPX_ROUTE_PATHS_GRAD_CHUNK 23 /* gpx_paths_grad: one hit per row chunk of xo                                                   */
#define GPX_ROUTE_REMOVE         24   /* gpx_gp_remove: one hit per call                                               */
#define GPX_ROUTE_SPARSE_CHUNK   25   /* gpx_sgp_fit: one hit per column chunk of x                                   */
#define GPX_ROUTE_SELECT_STEP    26   /* gpx_sgp_select: one hit per step that picked a point                          */
#define GPX_ROUTE_CG_ITER        27   /* gpx_cg_solve, gpx_cg_var: one hit per iteration of a group of columns         */
#define GPX_ROUTE_LOWRANK        28   /* gpx_d_lowrank_reduce, gpx_cg_lh: one hit per launch of the low-rank tile reduction      */
int gpx_debug_route_count(int route, int64_t *count);
/* roctx ranges pushed so far (GPX_ROCTX=1: every gpx_gp_* call and every launch class below it is a nested host range for
 * `rocprofv3 --marker-trace`; libroctx64.so is loaded on first use; 0 while the switch is off) */
int gpx_debug_roctx_ranges(int64_t *count);
int gpx_debug_route_reset(void);
/* Switch snapshots taken so far: every entry point re-reads the GPX_* environment variables ONCE for the calling thread
 * (one pass over `environ`; csrc/gpx_tune.h is the table of all of them); nothing below an entry point reads the
 * environment -- libgpx.so does not import getenv. */
int gpx_debug_tune_refreshes(int64_t *count);
/* GPX_KAPPLY_FUSED_MAX: the largest number of weight vectors S for which gpx_d_kmat_apply takes its fused route (defaults per
 * dtype: csrc/gpx_tune.h, measured: DESIGN "Posterior paths").  The one switch that is a call and not an environment variable:
 * value >= 0 sets it for the whole process and both dtypes (0: always the product route), value < 0 restores the defaults;
 * *previous (may be NULL) receives the value that was in force, -1 for the defaults.  Like every switch it enters the calling
 * thread's snapshot at the next entry point. */
int gpx_debug_kapply_fused_max(int64_t value, int64_t *previous);
/* The asm-scheduled MFMA leaf of the panel kernel (csrc/gpx_leaf.h) carries wait states measured on gfx950; before a process
 * first uses it on a device it is checked there against the compiler-scheduled leaf (full-mantissa 256 x 256 panel, alone and
 * beside a product that loads every matrix pipe).  *state: 0 not run yet, 1 passed, 2 failed -- the library then uses the
 * compiler-scheduled leaf and says so on stderr.  run_now != 0: run it now if it has not run. */
int gpx_debug_leaf_selfcheck(int run_now, int *state);

/* ------------------------------------------------- device-level hot path -- */

/* Kernel-matrix build: out[i, j] = member(x1[i, :], x2[j, :]) (+ diag_add if i == j).
 * Replaces gaussian_c.K / periodic_c.K (and the d*K members) plus the
 * `K += eye(n) * s**2` of gp/gp.py:265 (diag_add = s*s, applied where i == j).
 * x1: (n, d), x2: (m, d) row-major, densely packed; out: (n, m) with ld.
 * params: HOST array (h, w[, p]) as doubles.  tri = GPX_LOWER skips tiles that
 * lie strictly above the diagonal (only meaningful for x1 == x2).
 * d > 1 (an extension: the reference is 1-D) uses r2 = sum_k (x1[i,k]-x2[j,k])^2;
 * periodic members other than GPX_K require d == 1.
 * GPX_KERNEL_GAUSSIAN_ARD: params = (h, w_1 ... w_d), member GPX_K only (others: GPX_ERR_UNSUPPORTED); both point sets
 * are scaled into this host thread's scratch (gpx_d_scale_points), then built as GPX_KERNEL_GAUSSIAN. */
int gpx_d_kmat(int dtype, int kernel, int member, const void *x1, int64_t n,
               const void *x2, int64_t m, int d, const double *params,
               double diag_add, int tri, void *out, int64_t ld, void *stream);

/* out[i, k] = x[i, k] / w[k] for i < n, k < d, in `dtype` (a true division: the fp64 result is numpy's x / w bit for
 * bit).  x, out: DEVICE (n, d) densely packed, out may equal x; w_host: HOST d doubles, 1 <= d <= GPX_ARD_MAX_D.
 * The identity behind GPX_KERNEL_GAUSSIAN_ARD:  k_ard(a, b; h, w) = k_gaussian(a / w, b / w; h / sqrt(wbar), 1). */
int gpx_d_scale_points(int dtype, const void *x, int64_t n, int d, const double *w_host, void *out, void *stream);

/* Fused posterior mean  out[i] = sum_j K(xo[i], x[j]) * alpha[j]   (gp/gp.py:597
 * without materialising Kxox).  xo: (m, d), x: (n, d), alpha: (n,), out: (m,). */
int gpx_d_mean(int dtype, int kernel, const void *xo, int64_t m, const void *x,
               int64_t n, int d, const double *params, const void *alpha,
               void *out, void *stream);

/* The same with any member of the kernel family in place of K (the Jacobian / Hessian members of
 * gaussian_c.pyx:51-164, periodic_c.pyx:53-235): out = member(xo, x) @ alpha, never materialised.
 * Periodic members other than GPX_K need d == 1. */
int gpx_d_mean_member(int dtype, int kernel, int member, const void *xo, int64_t m, const void *x,
                      int64_t n, int d, const double *params, const void *alpha, void *out, void *stream);

/* Fused input-space gradient  out_dev[i, k] = scale * sum_j w_ij * dk(xo_i, x_j)/dxo_ik  for i < m, k < d, never
 * materialising dK.  w_ij = alpha[j] (B == NULL: with alpha = K^-1 y and scale = 1 the gradient of the posterior mean) or
 * B[i * ldb + j] (alpha == NULL: a solved chunk B = Kxox K^-1 and scale = -2 give the gradient of the posterior variance);
 * exactly one of the two.  xo: (m, d), x: (n, d), alpha: (n,), B: (m, n) ldb, all DEVICE in `dtype`; out_dev: DEVICE DOUBLE
 * (m, d) dense.  All three families (ARD: computed on x / w, column k divided by w_k); every d gpx_d_mean takes for the
 * dtype, GPX_ERR_UNSUPPORTED beyond.  The differences a_k - b_k are formed directly; a pair the kernel's underflow clamp
 * zeroes adds exactly 0.  f64 accumulation for both dtypes, fixed summation order, no atomics: bitwise repeatable.
 * GPX_PROF_PRED_GRAD. */
int gpx_d_pred_grad(int dtype, int kernel, const void *xo, int64_t m, const void *x, int64_t n, int d,
                    const double *params, const void *alpha, const void *B, int64_t ldb, double scale,
                    double *out_dev, void *stream);

/* C (M x N, ldc) += alpha * A (M x K, lda) * B (N x K, ldb)^T -- the MFMA work-horse.
 * tri = GPX_LOWER: only tiles with some row >= col are touched and elements
 * with col > row are left unchanged (SYRK form; requires M == N geometry with
 * row/col origins equal).  row0/col0 shift the triangle test:
 * element (i, j) is "lower" when row0 + i >= col0 + j. */
int gpx_d_gemm_nt(int dtype, int64_t M, int64_t N, int64_t K, double alpha,
                  const void *A, int64_t lda, const void *B, int64_t ldb, void *C,
                  int64_t ldc, int tri, int64_t row0, int64_t col0, void *stream);

/* Blocked right-looking Cholesky, lower, in place (replaces scipy.linalg.cholesky,
 * gp/gp.py:294 -> LAPACK dpotrf).  Only the lower triangle of A is read; the
 * strict upper triangle is left untouched (use gpx_d_tril to zero it).
 * info_dev: DEVICE int; 0 on success, j (1-based) if the j-th leading minor is
 * not positive definite (pivot <= 0 or NaN), as LAPACK reports it; negative: an
 * internal failure (the host entry points turn that into GPX_ERR_INTERNAL).
 * A pure enqueue at every size (round 4: the host-paced panel launches that made
 * the call block for n <= 16384 are confined to the handle's gpx_gp_fit, which
 * says so; nothing here waits on the host, so the call is legal under stream
 * capture); the result is complete in stream order. */
int gpx_d_potrf(int dtype, void *A, int64_t n, int64_t lda, int *info_dev,
                void *stream);

/* The two building blocks of gpx_d_potrf, exported for multi-GPU drivers (1-D
 * block-cyclic block columns).
 * gpx_d_potrf_panel factors rows [r0, n) x columns [c0, c0 + kb) of A in place; the
 * kb x kb diagonal block sits at (r0, c0) (c0 == r0 on one GPU; a local column
 * offset on a distributed matrix).  info_dev as in gpx_d_potrf (index r0-based
 * global: r0 + j + 1), never cleared here.
 * gpx_d_syrk_bc applies a factored panel Pb (row i = global row k0 + i, kb columns,
 * ldp) to this rank's block columns: local columns [cl0, cl1) of Cloc (n rows,
 * ldc), rows [row_begin, n); local block jl is global block jl * P + rank of width
 * nb;  C[g, c] -= sum_k Pb[g - k0, k] * Pb[gcol(c) - k0, k]  where g >= gcol(c). */
int gpx_d_potrf_panel(int dtype, void *A, int64_t lda, int64_t n, int64_t r0, int64_t c0,
                      int64_t kb, int *info_dev, void *stream);
int gpx_d_syrk_bc(int dtype, int64_t n, int64_t row_begin, void *Cloc, int64_t ldc,
                  int64_t cl0, int64_t cl1, const void *Pb, int64_t ldp, int64_t k0,
                  int64_t kb, int64_t nb, int P, int rank, void *stream);

/* The same two products with the arguments the public entries hide, for tests (tests/test_gpu_gemm.py); the argument checks
 * of gpx_d_gemm_nt / gpx_d_syrk_bc apply.
 * gpx_debug_gemm_nt: beta0 = 1: C = alpha A B^T, C is not read (aligned fast route and tri = GPX_FULL only, GPX_ERR_UNSUPPORTED
 * otherwise); ktri = 1: A == B upper triangular in (row, k) and M == N == K, the k-loop of a tile row skips the zeros (ignored
 * on the generic route); count x count2 products, member (y, z) at A + y sA + z tA (elements), B and C alike; a two-dimensional
 * batch needs the fast route.  C == A is legal when N == K <= 64, beta0 = 1 and ldc == lda: each tile has read all K columns of
 * its own rows before it stores them, and no other tile touches those rows.
 * gpx_debug_syrk_bc: abort_flag_dev: DEVICE int per batch member (NULL: none), a member whose word is non-zero is left
 * untouched (fast route only); count members, panels sP and matrices sC elements apart. */
int gpx_debug_gemm_nt(int dtype, int64_t M, int64_t N, int64_t K, double alpha, const void *A, int64_t lda,
                      const void *B, int64_t ldb, void *C, int64_t ldc, int tri, int64_t row0, int64_t col0,
                      int beta0, int ktri, int count, int64_t sA, int64_t sB, int64_t sC, int count2, int64_t tA,
                      int64_t tB, int64_t tC, void *stream);
int gpx_debug_syrk_bc(int dtype, int64_t n, int64_t row_begin, void *Cloc, int64_t ldc, int64_t cl0, int64_t cl1,
                      const void *Pb, int64_t ldp, int64_t k0, int64_t kb, int64_t nb, int P, int rank,
                      const int *abort_flag_dev, int count, int64_t sP, int64_t sC, void *stream);

/* The panel and the factorisation with the arguments the public entries hide, for tests (tests/test_gpu_potrf.py); host code
 * only, the argument checks of gpx_d_potrf_panel / gpx_d_potrf apply.
 * gpx_debug_potrf_panel: kpre: that many columns immediately to the left of the panel (rows [r0, n), whole 64-column blocks,
 * <= c0 and <= GPX_POTRF_FOLD_K) hold finished columns of L that the launch applies to the panel first; only a panel the
 * resident kernel takes in one launch can do that, any other kb with kpre != 0 is GPX_ERR_ARG.  idle_chip: the hint the
 * factorisation gives a panel launched ahead of the update it runs beside (single matrices of up to GPX_PANEL_EXCL_ROWS rows:
 * a CU of its own per workgroup).  count matrices sA elements apart (sA >= n lda, a multiple of 16) are factored in lock-step,
 * info_dev then holds one word per matrix.
 * gpx_debug_potrf: xrows further rows below the n x n matrix ride along: on return row n + i holds L^-1 applied to what was
 * stored there; count and sA (>= (n + xrows) lda) as above; a pure enqueue, no progress hook.
 * gpx_debug_panel_last: which instantiation of the resident panel kernel the calling thread's last launch on the current
 * device was (recorded on the host next to the launch): *lv, *leaf_mfma: the kernel's LV and LEAF_MFMA (csrc/gpx_panel.hip;
 * LEAF_MFMA = 0: the lean kernel with the VALU leaf) of the launch that held the diagonal blocks; *two_part: the rows below
 * them went out as a second launch; *pad_lds_bytes: dynamic LDS of an exclusive-CU launch, else 0.  Any pointer may be NULL;
 * GPX_ERR_ARG before the thread's first launch. */
int gpx_debug_potrf_panel(int dtype, void *A, int64_t lda, int64_t n, int64_t r0, int64_t c0, int64_t kb,
                          int *info_dev, int64_t kpre, int idle_chip, int count, int64_t sA, void *stream);
int gpx_debug_potrf(int dtype, void *A, int64_t n, int64_t lda, int *info_dev, int64_t xrows, int count, int64_t sA,
                    void *stream);
int gpx_debug_panel_last(int *lv, int *leaf_mfma, int *two_part, int *pad_lds_bytes);

/* Zero the strict upper triangle (scipy's cholesky returns a clean L). */
int gpx_d_tril(int dtype, void *A, int64_t n, int64_t lda, void *stream);

/* x <- L^-1 b (transpose = 0, forward) or x <- L^-T b (transpose = 1, backward),
 * single right-hand side; b is used as scratch and destroyed, x != b.
 * Forward then backward = cho_solve((L, True), b), gp/gp.py:332-334 (dpotrs). */
int gpx_d_trsv_lower(int dtype, const void *L, int64_t n, int64_t ldl, void *b,
                     void *x, int transpose, void *stream);

/* Distributed-solve building blocks (block columns live on different GPUs).
 * gpx_d_trsv_lower_cols: forward substitution through a trapezoid -- an
 * ncols x ncols lower triangle on top of n - ncols further rows (one factored
 * block column, rows from its diagonal down): x[0:ncols] <- solution,
 * b[ncols:n] -= L[ncols:n, 0:ncols] x.  b is scratch, x != b.
 * gpx_d_panel_gemv_t: y[c] -= sum_r Lp[r, c] * x[r] for c < ncols, r < rows (the
 * sub-diagonal part of a block column, transposed); work: cdiv(rows, 256) * ncols
 * doubles of DEVICE scratch.  Deterministic (no atomics). */
int gpx_d_trsv_lower_cols(int dtype, const void *L, int64_t n, int64_t ldl, int64_t ncols,
                          void *b, void *x, void *stream);
int gpx_d_panel_gemv_t(int dtype, const void *Lp, int64_t ldl, int64_t rows, int64_t ncols,
                       const void *x, void *y, void *work, void *stream);

/* X (m x n, ldx) <- X * L^-T  : rows of X are right-hand sides; i.e. solves
 * L * x_row^T = b_row^T for every row.  With X = Kxox this yields V^T where
 * V = L^-1 Kxxo, the factor of the posterior covariance (gp/gp.py:622-625). */
int gpx_d_trsm_right_lt(int dtype, const void *L, int64_t n, int64_t ldl, void *X,
                        int64_t m, int64_t ldx, void *stream);

/* X (m x n, ldx) <- X * L^-1, in place: the mirror of gpx_d_trsm_right_lt (block columns from the last to the first,
 * right-looking; the row panel of L that a far update multiplies by is staged transposed in per-thread scratch, at most
 * n x 512 elements).  After gpx_d_trsm_right_lt on X = Kxox this yields the rows of Kxox K^-1.  Same argument checks;
 * brings no block operators, so the 64-wide route.  Deterministic (no atomics, fixed order). */
int gpx_d_trsm_right_l(int dtype, const void *L, int64_t n, int64_t ldl, void *X,
                       int64_t m, int64_t ldx, void *stream);

/* out_dev[0] = 2 * sum_i log L[i,i]  (f64 accumulation for both dtypes).
 * Replaces the LU-based np.linalg.slogdet(K) of gp_c.pyx:21 given L. */
int gpx_d_logdet_chol(int dtype, const void *L, int64_t n, int64_t ldl,
                      double *out_dev, void *stream);

/* out_dev[i] = kdiag(i) - sum_j X[i, j]^2   for i < rows, j < n;  X: rows x n, ldx, handle dtype;  out_dev: DOUBLE
 * kdiag(i): kdiag_dev[i] (double) when kdiag_dev != NULL, else K(xo[i,:], xo[i,:]) of the kernel family, evaluated by
 * the same device function gpx_d_kmat uses (so it equals the diagonal of gpx_d_kmat(xo, xo) in that dtype).
 * f64 accumulation for both dtypes, fixed summation order, no atomics: bitwise repeatable. */
int gpx_d_var_rows(int dtype, int kernel, const void *X, int64_t rows, int64_t n, int64_t ldx, const void *xo, int d,
                   const double *params, const double *kdiag_dev, double *out_dev, void *stream);
/* (The finishing pass of the predictive variance, on a chunk X = K(xo_c, x) L^-T: rows n sizeof(T) bytes read once;
 * 16-byte loads when ldx and X are 16-byte aligned, scalar loads otherwise.  GPX_PROF_REDUCE.) */

/* The finishing pass of leave-one-out, on a chunk X = E_c L^-T (rows [c0, c0 + rows) of the identity, solved): row i is
 * column c0 + i of L^-1, and kii_dev[i] = sum_j X[i, j]^2 over j in [c0 + i, n) = (K^-1)_{c0+i, c0+i}.  X: rows x n, ldx, handle
 * dtype, c0 + rows <= n.  Row i is read from column c0 + i rounded down to the 16-byte vector (from c0 + i itself when X or
 * ldx is not 16-byte aligned); the columns before c0 + i are masked, whatever they hold, and nothing outside
 * [that column, n) is loaded.  With y and alpha (DEVICE, handle dtype, the chunk's own rows: y[i] goes with row i; both or
 * neither) the leave-one-out quantities of RW06 eq. 5.10 - 5.12 are written by the same pass, each pointer optional,
 * with k = kii[i], a = alpha[i]:   mean_dev[i] = y[i] - a / k    var_dev[i] = 1 / k
 *                                  logp_dev[i] = log(k) / 2 - a^2 / (2 k) - log(2 pi) / 2
 * All outputs DOUBLE; f64 accumulation for both dtypes, fixed summation order, no atomics: bitwise repeatable.
 * One 256-thread workgroup per row; GPX_PROF_REDUCE. */
int gpx_d_loo_rows(int dtype, const void *X, int64_t rows, int64_t n, int64_t ldx, int64_t c0, const void *y, const void *alpha,
                   double *kii_dev, double *mean_dev, double *var_dev, double *logp_dev, void *stream);

/* out_dev[0] = sum_i a[i] * b[i]  (f64 accumulation).  np.dot(y, Kiy), gp_c.pyx:26 */
int gpx_d_dot(int dtype, const void *a, const void *b, int64_t n, double *out_dev,
              void *stream);

/* dst[i, j] = src[i, j] for j <= i < n (lower trapezoid, re-pitched lds -> ldd); 16-byte vectors where both sides allow.
 * Elements of dst to the right of the 16-byte vector that holds the diagonal are not written.
 * (Both bases and both pitches 16-byte aligned: row i moves whole vectors up to the one that holds column i, which stays
 * inside the pitch; otherwise exactly columns [0, i], one element at a time.  n^2 / 2 elements each way, where a strided
 * memcpy of the square moves n^2.  GPX_PROF_EXTEND.) */
int gpx_d_copy_lower(int dtype, const void *src, int64_t lds, void *dst, int64_t ldd, int64_t n, void *stream);
/* S[i, j] -= sum_c B[i, c] B[j, c]  for j <= i < k, c < n  (B: k x n, ldb; S: k x k, lds; strict upper untouched).
 * Split over column slices of B so that few rows still fill the chip; the slices' partial products are summed in f64
 * in ascending slice order and rounded once: no atomics, bitwise repeatable.
 * (The partial products are MFMA products in `dtype` into this host thread's scratch; any base / pitch is accepted, the
 * aligned ones take the fast product kernel.  When all n columns fit ONE slice there are no partials: one product
 * S -= B B^T on the lower tiles, accumulated by the product kernel in `dtype`.) */
int gpx_d_schur_lower(int dtype, const void *B, int64_t k, int64_t n, int64_t ldb, void *S, int64_t lds, void *stream);
/* The Cholesky factor without k of its rows and columns: out (n - k) x (n - k), ldo, lower triangle = the factor of K with
 * rows and columns idx deleted, where L (n x n, ldl, lower, on the device, only read) is the factor of K.  The strict upper
 * triangle of out is not written.  idx_host: k sorted distinct indices in [0, n) on the HOST, 1 <= k < n (it may be reused
 * on return: the call waits for its upload, nothing else).  GPX_ERR_ARG for unsorted, repeated or out-of-range indices,
 * k >= n, out == L or a pitch that is too small.
 * Rows and columns before idx[0] are copied; behind each deleted column the factor takes a rank-1 UPDATE by Givens
 * rotations (stable for any factor, no pivot can fail), all k of them in ONE pass: one launch per block of 32 columns from
 * idx[0]'s block on, in stream order; the k update vectors (n x k in `dtype`) live in this host thread's scratch.
 * O((n - idx[0])^2 k) flops, the factor read once and written once.  The arithmetic is `dtype`'s; no atomics and a fixed
 * order: bitwise repeatable.  Any base / pitch is accepted: 16-byte loads where L's allow.  GPX_PROF_CHOL_DELETE. */
int gpx_d_chol_delete(int dtype, const void *L, int64_t n, int64_t ldl, const int64_t *idx_host, int64_t k, void *out, int64_t ldo,
                      void *stream);

/* Normal numbers, counter based.
 * out[i, j] = z(seed, stream, offset + i * cols + j)  for i < rows, j < cols;  out: rows x cols, ld >= cols, in `dtype`.
 * Elements in the padding [cols, ld) are not written.  GPX_PROF_RANDN (bytes written).
 * z(seed, stream, e) is a pure function of its three arguments -- not of the grid, of ld, or of how a caller splits a matrix
 * into calls (two calls that split a matrix by rows, the second with offset = rows_1 * cols, give the bits of one call):
 *   q = e >> 1
 *   (w0, w1, w2, w3) = Philox4x32-10, counter (q & 0xffffffff, q >> 32, stream & 0xffffffff, stream >> 32),
 *                      key (seed & 0xffffffff, seed >> 32); constants and rounds of Random123: multipliers 0xD2511F53 (on c0)
 *                      and 0xCD9E8D57 (on c2), key increments 0x9E3779B9 and 0xBB67AE85 after every round, one round
 *                      c <- (hi(M1 c2) ^ c1 ^ k0, lo(M1 c2), hi(M0 c0) ^ c3 ^ k1, lo(M0 c0))
 *   u1 = (2 (((w0 << 32) | w1) >> 12) + 1) 2^-53, u2 likewise from (w2, w3): exact in fp64, in [2^-53, 1 - 2^-53], so
 *        log u1 is finite and |z| <= sqrt(106 ln 2) = 8.572
 *   r = sqrt(-2 ln u1);  even e: r cos(2 pi u2), odd e: r sin(2 pi u2)   (sincospi(2 u2): the angle is never rounded)
 * computed in fp64 for both dtypes and rounded once to `dtype`.  One thread per Philox call; the two elements of a pair may
 * lie in different rows (odd cols), and the first or last element of a call may be half a pair (odd offset). */
int gpx_d_randn(int dtype, void *out, int64_t rows, int64_t cols, int64_t ld,
                uint64_t seed, uint64_t stream, uint64_t offset, void *hipstream);

/* out (S x m, ldo) = 1 mean^T + Z Lc^T  with  Lc Lc^T = C + jitter I  and  Z = randn(S x m; seed, stream, offset 0).
 * C: m x m, ldc, lower triangle read, DESTROYED (on return it holds Lc with a zero upper triangle).  mean: (m,) or NULL (zero).
 * Z: S x ldz work block.  info_dev as gpx_d_potrf; when it is non-zero, out is unspecified.  A pure enqueue.
 * (jitter onto the diagonal, gpx_d_potrf, gpx_d_tril, gpx_d_randn into Z, mean into every row of out, then one
 * gpx_d_gemm_nt: out[s, i] += sum_k Z[s, k] Lc[i, k].  C as gpx_d_potrf wants it: 16-byte aligned, ldc a multiple of 16;
 * jitter finite and >= 0.) */
int gpx_d_mvn_sample(int dtype, void *C, int64_t m, int64_t ldc, const void *mean, double jitter, int64_t S,
                     uint64_t seed, uint64_t stream, void *Z, int64_t ldz, void *out, int64_t ldo,
                     int *info_dev, void *hipstream);

/* Random Fourier features of a point set:  out[i, f] = scale cos(omega_f . p_i),  out[i, F + f] = scale sin(omega_f . p_i)
 * for i < m, f < F.  pts: (m, d) densely packed in `dtype`; omega_dev: DEVICE DOUBLE (F, d) densely packed, for both dtypes;
 * out: (m, 2F) with ld >= 2F in `dtype`; the padding [2F, ld) is not written.  The projection and the sincos are fp64 for
 * both dtypes (the point as stored, converted exactly), the result is rounded once on the store.  One launch;
 * GPX_PROF_RFF (bytes written). */
int gpx_d_rff_features(int dtype, const void *pts, int64_t m, int d, const double *omega_dev, int64_t F, double scale,
                       void *out, int64_t ld, void *stream);

/* The derivative of that feature map with respect to the point, as a matrix gpx_d_gemm_nt can consume -- row i d + k is
 * d phi(p_i) / d p_ik:
 *   out[i d + k, f]     = -(scale / div_k) omega[f, k] sin(omega_f . p_i)
 *   out[i d + k, F + f] =  (scale / div_k) omega[f, k] cos(omega_f . p_i)        i < m, k < d, f < F
 * out: (m d, 2F) with ld >= 2F in `dtype`; the padding [2F, ld) is not written.  col_div: HOST, d doubles
 * (d <= GPX_ARD_MAX_D), or NULL for no division (the ARD family on scaled points: div = w).  gpx_d_rff_features'
 * conventions otherwise: fp64 projection and sincos for both dtypes -- formed once per (i, f), not d times -- one
 * rounding on the store, frequencies along the lanes.  One launch; GPX_PROF_RFF (bytes written). */
int gpx_d_rff_features_grad(int dtype, const void *pts, int64_t m, int d, const double *omega_dev, int64_t F, double scale,
                            const double *col_div, void *out, int64_t ld, void *stream);

/* out[s, i] += sum_j K(xo_i, x_j) V[s, j]   for s < S, i < m:  the kernel matrix applied to S weight vectors at once,
 * accumulated INTO out.  xo: (m, d), x: (n, d) densely packed; V: (S, n) ldv; out: (S, m) ldo; all DEVICE in `dtype`.
 * Member GPX_K of GPX_KERNEL_GAUSSIAN and GPX_KERNEL_PERIODIC (any d gpx_d_mean takes); GPX_KERNEL_GAUSSIAN_ARD callers pass
 * scaled points and the isotropic constants (gpx_d_scale_points).  Two routes:
 *   fused (GPX_ROUTE_KAPPLY_FUSED; S <= GPX_KAPPLY_FUSED_MAX and d within gpx_d_mean's range): K(xo, x) is never
 *     materialised.  A workgroup owns 4 test points and a slice of x streamed through LDS, every lane one training point and
 *     a register block of 8 weight vectors (8 points and 1 or 4 vectors for S = 1 and S <= 4); each k(xo_i, x_j) -- the entry
 *     function of gpx_d_kmat, underflow clamp included -- is formed once per group of vectors; f64 sums, slices added in ascending order by a second launch: no atomics,
 *     bitwise repeatable.  GPX_PROF_KAPPLY.
 *   product (GPX_ROUTE_KAPPLY_GEMM): row chunks of xo (a multiple of 128 rows): gpx_d_kmat into this host thread's scratch,
 *     then gpx_d_gemm_nt(S, m_c, n, 1, V, ldv, K_c, ., out + r0, ldo).
 * Both routes take any base and pitch of V and out (the product route's fast kernel wants V 16-byte aligned with ldv a multiple of
 * 16 bytes and takes the generic one otherwise).
 * m == 0, S == 0 or n == 0 leaves out as it is. */
int gpx_d_kmat_apply(int dtype, int kernel, const void *xo, int64_t m, const void *x, int64_t n, int d,
                     const double *params, const void *V, int64_t ldv, int64_t S, void *out, int64_t ldo, void *stream);

/* out[s, i d + k] += (1 / div_k) sum_j V[s, j] dk(xo_i, x_j)/dxo_ik   for s < S, i < m, k < d:  the input-space gradient
 * of the kernel matrix applied to S weight vectors at once, accumulated INTO out; dK is never materialised and each
 * k(xo_i, x_j) is formed once per group of vectors and window of dimensions.  xo: (m, d), x: (n, d) densely packed; V: (S, n)
 * ldv; out: (S, m d) ldo; all DEVICE in `dtype`, any base and pitch of V and out.  col_div: HOST, d doubles
 * (d <= GPX_ARD_MAX_D), or NULL for no division.  GPX_KERNEL_GAUSSIAN only (dk/da_k = -(a_k - b_k) / w^2 k):
 * GPX_KERNEL_GAUSSIAN_ARD callers pass scaled points, the isotropic constants and col_div = w; the periodic and ARD ids
 * return GPX_ERR_UNSUPPORTED.  Every d gpx_d_mean takes for the dtype, GPX_ERR_UNSUPPORTED beyond; every S: groups of
 * weight vectors go on the grid's z (more than 65535 groups: GPX_ERR_ARG).
 * A workgroup owns a few test points, a slice of x streamed through LDS and a window of dimensions, every lane one training
 * point and a register block of weight vectors (at most 32 f64 sums per lane; the block by S and d: DESIGN "Posterior
 * paths").  Per pair the distance over all d dimensions and k_ij -- the entry function of gpx_d_kmat, underflow clamp
 * included: a clamped pair adds exactly 0 -- are formed once, g_s = k_ij V[s, j] in f64, and every difference a_k - b_k
 * directly.  f64 sums for both dtypes; lanes by shuffles, waves through LDS, slices in ascending order by a second launch,
 * which also applies -1 / w^2, the division, the += and the one rounding to `dtype`: no atomics, bitwise repeatable.
 * There is no product route (dK is d times the size of K).  GPX_PROF_KAPPLY_GRAD.
 * m == 0, S == 0 or n == 0 leaves out as it is. */
int gpx_d_kmat_apply_grad(int dtype, int kernel, const void *xo, int64_t m, const void *x, int64_t n, int d,
                          const double *params, const double *col_div, const void *V, int64_t ldv, int64_t S, void *out,
                          int64_t ldo, void *stream);

/* ------------------------------------------------ fitted-GP device handle -- */
/* One handle = one GP resident in HBM: x, y, the kernel matrix / its factor
 * (in place), alpha = K^-1 y, logdet, y^T alpha.  Mirrors the memoised
 * properties of gp.GP (gp/gp.py:242-396). */
typedef struct gpx_gp gpx_gp_t;

int gpx_gp_create(gpx_gp_t **gp, int dtype, int kernel, int64_t n, int d);
int gpx_gp_destroy(gpx_gp_t *gp);
/* x: (n, d) HOST float64; y: (n,) HOST float64 (converted to dtype on upload) */
int gpx_gp_set_data(gpx_gp_t *gp, const double *x, const double *y);
/* same, from DEVICE buffers (on the handle's device) already in the handle's dtype.  The
 * copies run on the handle's own non-blocking stream: whatever produced x_dev / y_dev must
 * have completed (synchronise the producing stream first).  Returns after the copies are
 * done, so the sources may be freed or overwritten at once. */
int gpx_gp_set_data_device(gpx_gp_t *gp, const void *x_dev, const void *y_dev);
/* params = (h, w[, p]), or (h, w_1 ... w_d) for GPX_KERNEL_GAUSSIAN_ARD; s = noise standard deviation (gp/gp.py:190-197) */
int gpx_gp_set_params(gpx_gp_t *gp, const double *params, double s);
/* the kernel parameters the handle holds: *count of them (any family), the first min(cap, *count) written to params */
int gpx_gp_get_params(gpx_gp_t *gp, double *params, int cap, int *count);
/* Plugin kernels (any gp.kernels.Kernel subclass without a native id):
 * the host evaluates its own K(x, x) + s^2 I (gp/gp.py:263-266) and hands the
 * full (n, n) HOST float64 matrix over; gpx_gp_fit then skips the kernel build. */
int gpx_gp_set_K(gpx_gp_t *gp, const double *Kxx, int64_t ld);
/* kernel build (lower) -> potrf -> alpha -> logdet, y^T alpha.  info != NULL: *info (HOST)
 * is filled and the call returns after the fit has completed.  info == NULL: the call returns without waiting for
 * the end of the fit (the next gpx_gp_* getter synchronises); for n <= 16384 it paces its panel launches on the
 * device's progress, so it returns when most of the factorisation has run, not at once. */
int gpx_gp_fit(gpx_gp_t *gp, int *info);
/* log marginal likelihood with the reference's conventions (gp/gp.py:360-367,
 * gp_c.pyx:17-31): -inf when the factorisation failed or logdet < MIN. */
int gpx_gp_log_lh(gpx_gp_t *gp, double *log_lh);
int gpx_gp_logdet(gpx_gp_t *gp, double *logdet);
/* potrf info of the last fit (0 ok, j > 0: j-th leading minor not positive definite) */
int gpx_gp_info(gpx_gp_t *gp, int *info);
/* posterior mean at xo (m, d) HOST float64 -> out (m,) HOST float64 */
int gpx_gp_mean(gpx_gp_t *gp, const double *xo, int64_t m, double *out);
/* posterior covariance at xo -> out (m, m) HOST float64, via V = L^-1 Kxxo */
int gpx_gp_cov(gpx_gp_t *gp, const double *xo, int64_t m, double *out);
/* plugin-kernel forms: the caller supplies Kxox (m, n) [and Kxoxo (m, m)] as HOST
 * float64; mean = Kxox alpha, cov = Kxoxo - (Kxox L^-T)(Kxox L^-T)^T on the device */
int gpx_gp_mean_from_K(gpx_gp_t *gp, const double *Kxox, int64_t m, double *out);
int gpx_gp_cov_from_K(gpx_gp_t *gp, const double *Kxox, const double *Kxoxo, int64_t m,
                      double *out);
/* diag of the posterior covariance at xo (m, d) HOST float64 -> out (m,) HOST float64, in row chunks:
 * per chunk X = K(xo_c, x) (m_c x n), X <- X L^-T, out_c = k(xo_c, xo_c) - rowsumsq(X).  Device memory: one chunk
 * (m_c x lda) whatever m.  chunk_rows: 0 = automatic, else a multiple of 128.  Same preconditions and errors as gpx_gp_cov. */
int gpx_gp_var(gpx_gp_t *gp, const double *xo, int64_t m, int64_t chunk_rows, double *out);
/* plugin kernels: the caller supplies Kxox (m, n) and kdiag (m,) = k(xo_i, xo_i), HOST float64 */
int gpx_gp_var_from_K(gpx_gp_t *gp, const double *Kxox, const double *kdiag, int64_t m, int64_t chunk_rows, double *out);
/* host arithmetic only (no GPU): the chunking of a call -- rows per chunk, number of chunks, device bytes per chunk */
int gpx_debug_var_plan(int dtype, int64_t n, int64_t m, int64_t chunk_rows, size_t free_bytes,
                       int64_t *rows_per_chunk, int64_t *chunks, size_t *bytes_per_chunk);
/* The automatic rule: the largest multiple of 128 rows, at most 4096, whose buffers -- the chunk itself and the solve's
 * staging block, (lda + 512) elements a row -- fit a quarter of free_bytes; m itself when all of m fits one chunk.
 * GPX_ERR_ARG: chunk_rows < 0 or not a multiple of 128, m < 0, n < 1.  GPX_ERR_NOMEM: 128 rows (or the chunk asked for)
 * do not fit.  The variance is not clamped at zero (neither is the diagonal of gpx_gp_cov). */
/* Leave-one-out cross-validation from the fitted factor (RW06 section 5.4.2).  diag(K^-1) -> out (n,) HOST float64:
 * (K^-1)_ii = |L^-1 e_i|^2, in row chunks of the identity: X = E_c L^-T by a sweep that begins at the chunk's own column
 * (L^-1 e_i is zero above row i), then gpx_d_loo_rows.  n^3 / 3 flops; device memory one chunk (as gpx_gp_var: the same
 * chunk_rows, rule, cap and errors, with m = n) plus n doubles that stay in the handle: a second call on the same fit
 * sweeps nothing.  set_data, set_params, set_K and fit drop them.  Preconditions and statuses of gpx_gp_cov, and
 * GPX_ERR_ARG when the last fit was not positive definite (there is no factor). */
int gpx_gp_inv_diag(gpx_gp_t *gp, int64_t chunk_rows, double *out);
/* mean[i], var[i]: the prediction for y_i -- noise included -- of the GP fitted without point i (eq. 5.12); log_p[i] its log
 * density at y_i (eq. 5.10); *log_p_sum their sum (eq. 5.11), reduced on the device in a fixed order.  (n,) HOST float64
 * each; any pointer may be NULL.  As gpx_gp_inv_diag, and y must be finite. */
int gpx_gp_loo(gpx_gp_t *gp, int64_t chunk_rows, double *mean, double *var, double *log_p, double *log_p_sum);
/* The gradient of the leave-one-out criterion L = *log_p_sum above w.r.t. (kernel params..., s), RW06 eq. 5.13 rearranged so
 * that ONE n^3 product serves every parameter.  With W = K^-1, k = diag W, c_i = (1 + alpha_i^2 / k_i) / (2 k_i),
 * r = W (alpha / k) and Pm = W diag(c) W:   dL/dtheta_j = sum_ab (dK/dtheta_j)_ab G_ab,   G = (r alpha^T + alpha r^T) / 2 - Pm,
 * dL/ds = 2 s (r . alpha - tr Pm).  On the device: W by TRSM + SYRK as gpx_gp_dloglh_dtheta forms it (whole, not its lower
 * triangle), k from the rows of L^-T, r by two sweeps with the factor, Pm = Y Y^T (lower triangle) with Y = W diag(sqrt(c))
 * written over L^-T and Pm over W, then one fused pass of (alpha, r, Pm) against the kernel derivatives evaluated on the fly:
 * fixed summation order, f64 sums, bitwise repeatable.  Device memory: gpx_gp_dloglh_dtheta's two n x lda blocks.
 * *loo_log_lh: the criterion itself from the same call, bit for bit gpx_gp_loo's *log_p_sum (the diagonal k stays in the
 * handle, whichever of the two calls came first).  grad: n_params + 1 HOST float64.  GPX_ERR_ARG: NULL arguments, a handle
 * that is not fitted or was fitted from gpx_gp_set_K (no kernel to differentiate), non-finite y.  -inf and an all-NaN gradient
 * when the factorisation failed.  Periodic kernel: d == 1 only (GPX_ERR_UNSUPPORTED). */
int gpx_gp_loo_grad(gpx_gp_t *gp, double *loo_log_lh, double *grad);            /* grad: n_params + 1, order (kernel params..., s) */
/* The weights themselves, for callers who hold the kernel's derivatives (plugin kernels, periodic at d > 1): G (n, n) with
 * leading dimension ld, float64, symmetric bit for bit -- formed in float64 from alpha, r and Pm's lower triangle in one
 * more n x n float64 block on the device, then downloaded.  No kernel is evaluated: any fitted, positive definite handle.
 * dL/dtheta_j = sum(dK_j * G); the noise's share is 2 s trace(G). */
int gpx_gp_loo_grad_weights(gpx_gp_t *gp, double *G, int64_t ld);               /* HOST n x n float64, full symmetric G above */
/* Input-space gradients of the prediction at xo (m, d) HOST float64 -> grad (m, d) HOST float64; m = 0 is legal.
 * gpx_gp_mean_grad: d mean(xo_i) / d xo_i, one fused pass (gpx_d_pred_grad with alpha); needs finite y, as gpx_gp_mean.
 * gpx_gp_var_grad: d var(xo_i) / d xo_i = -2 sum_j beta_ij dk(xo_i, x_j)/dxo_i with beta_i = K^-1 k(x, xo_i), in the row
 * chunks of gpx_gp_var (same chunk_rows, rule, buffer and errors): X = K(xo_c, x), X <- X L^-T, X <- X L^-1, then
 * gpx_d_pred_grad with B = X and scale = -2.  var (m,) HOST float64, optional: the variance itself, taken from the first
 * sweep of the same pass (what gpx_gp_var returns).  Nothing n x n beside the factor exists; one download at the end. */
int gpx_gp_mean_grad(gpx_gp_t *gp, const double *xo, int64_t m, double *grad);
int gpx_gp_var_grad(gpx_gp_t *gp, const double *xo, int64_t m, int64_t chunk_rows, double *var, double *grad);
/* Growing a fitted GP by k observations without refactoring.  The factor of the bordered matrix is the old factor with k
 * rows appended:  K' = [K B^T; B C],  L' = [L 0; X Ls],  X = B L^-T (k x n),  Ls Ls^T = C - X X^T (k x k),
 * B = K(x_new, x), C = K(x_new, x_new) + s^2 I:  one triangular sweep over k right-hand sides (n^2 k flops), a k x k
 * Schur complement and its factorisation, two single-rhs solves for the new alpha.
 * A NEW fitted handle for the n + k points (x; x_new), (y; y_new), same dtype / kernel / params / s as `gp`, whose factor is
 * the factor of `gp` with k rows appended -- no kernel matrix of the old points is rebuilt, nothing n x n is factored.
 * `gp` must be fitted and positive definite (else GPX_ERR_ARG) and is left untouched and usable; k >= 1.
 * x_new (k, d), y_new (k,) HOST float64.  *info (HOST, may not be NULL): 0, or n + j (1-based) when the j-th pivot of the
 * Schur complement is not positive -- exactly what potrf of the whole (n + k) matrix would report; the handle is then
 * "fitted, not PD" like one from gpx_gp_fit.  Synchronous.  On any failure *out = NULL and `gp` is intact.
 * The one thing of `gp` the call may change: block operators of the solves that `gp` has not built yet are completed (on the
 * new handle's stream, which is synchronised before the call returns or the new handle is destroyed), as by any gpx_gp_cov.
 * Source and result coexist: two factors are resident until the caller destroys one.  gpx_gp_last_timing of the new handle:
 * [0] rows of K [1] copy + sweep + Schur + potrf [2] solves [3] reductions [4] total. */
int gpx_gp_extend(gpx_gp_t *gp, const double *x_new, const double *y_new, int64_t k, gpx_gp_t **out, int *info);
/* plugin kernels: the caller supplies B = K(x_new, x) (k, n) and C = K(x_new, x_new) + s^2 I (k, k; lower read), HOST float64 */
int gpx_gp_extend_from_K(gpx_gp_t *gp, const double *x_new, const double *y_new, int64_t k,
                         const double *Knew_old, const double *Knew_new, gpx_gp_t **out, int *info);
/* Shrinking a fitted GP by k observations without refactoring (gpx_d_chol_delete on the handle's factor).
 * A NEW fitted handle for the n - k kept points, in their order, same dtype / kernel / params / s as `gp`: x and y are
 * gathered on the device, the factor is the source's with rows and columns idx deleted, alpha / logdet / y^T alpha come from
 * the tail of gpx_gp_fit.  No kernel is evaluated: a handle fitted from gpx_gp_set_K (plugin kernels) takes the same entry.
 * idx: k sorted distinct indices in [0, n), HOST, 1 <= k < n (else GPX_ERR_ARG).  `gp` must be fitted and positive definite
 * (else GPX_ERR_ARG); it is never written and stays usable.  *info (HOST, may not be NULL): 0 -- the rotations cannot fail.
 * Synchronous.  On any failure *out = NULL and `gp` is intact.  Source and result coexist: two factors are resident until
 * the caller destroys one.  gpx_gp_last_timing of the new handle: [0] 0 [1] the deletion [2] solves [3] reductions [4] total. */
int gpx_gp_remove(gpx_gp_t *gp, const int64_t *idx, int64_t k, gpx_gp_t **out, int *info);
/* Joint posterior samples at xo (m, d) HOST float64 -> out (S, m) HOST float64: row s is one draw of the function values
 * at the m points, mean(xo) + Lc z_s with Lc Lc^T = cov(xo) + (jitter [+ s^2]) I.  The covariance is built exactly as
 * gpx_gp_cov builds it (the matrix that is factored is bit for bit the one it would download), the mean is gpx_gp_mean's, then
 * gpx_d_mvn_sample with stream = 0 on the device: one download of S x m, nothing m x m leaves the device.
 * noise != 0: s^2 is added to the diagonal -- the draw is of new OBSERVATIONS.
 * jitter >= 0: absolute.  jitter < 0: automatic, sqrt(eps_dtype) * k(0) with k(0) the family's prior variance, from the
 * handle's parameters on the host (h^2 / (w sqrt(2 pi)), h^2 for the periodic family, the isotropic constants for ARD).
 * *info (HOST, may not be NULL): 0, or the 1-based failing pivot of the m x m factorisation -- the status is GPX_OK and out is
 * not written; there is no retry with a larger jitter.  m == 0 or S == 0 is legal and writes nothing.
 * Preconditions and statuses of gpx_gp_cov, finite y as gpx_gp_mean, GPX_ERR_ARG when the last fit was not positive definite
 * (there is no factor), GPX_ERR_NOMEM when X (m x lda), C (m x m), Z and the samples (S x m each) do not fit: m is bounded by
 * HBM, nothing is chunked.  GPX_ROUTE_SAMPLE: one hit per call.  gpx_gp_last_timing is untouched. */
int gpx_gp_sample(gpx_gp_t *gp, const double *xo, int64_t m, int64_t S, uint64_t seed, int noise, double jitter,
                  double *out /* (S, m) HOST float64 */, int *info);
/* plugin kernels: the caller supplies Kxox (m, n) and Kxoxo (m, m), HOST float64; jitter >= 0 (no parameters to derive one
 * from).  noise adds the s of gpx_gp_set_params: a handle fitted from gpx_gp_set_K alone has none (its caller folds s^2 into
 * jitter). */
int gpx_gp_sample_from_K(gpx_gp_t *gp, const double *Kxox, const double *Kxoxo, int64_t m, int64_t S, uint64_t seed,
                         int noise, double jitter, double *out, int *info);
/* copy-outs to HOST float64: Kxx is rebuilt (full, + s^2 I); L has zero upper */
int gpx_gp_get_Kxx(gpx_gp_t *gp, double *out, int64_t ld);
int gpx_gp_get_Lxx(gpx_gp_t *gp, double *out, int64_t ld);
int gpx_gp_get_alpha(gpx_gp_t *gp, double *out);
/* K^-1 = L^-T L^-1 (gp/gp.py:311-312) -> out (n, n) HOST float64 */
int gpx_gp_get_inv_Kxx(gpx_gp_t *gp, double *out, int64_t ld);
/* d log_lh / d(theta): out[n_params + 1] HOST float64, order (kernel params..., s).  RW06 eq. 5.9
 * (gp/gp.py:398-433, gp_c.pyx:34-49) computed on the device: K^-1 by TRSM + SYRK on the MFMA
 * kernel, then one fused pass against kernel derivatives evaluated on the fly.  All NaN when the
 * factorisation failed (gp/gp.py:424-428).  Periodic kernel: d == 1 only.
 * GPX_KERNEL_GAUSSIAN_ARD: d + 2 values (h, w_1 ... w_d, s); K^-1 as above, then one pass over its lower triangle that
 * accumulates S_0 = sum c_ab, S_k = sum c_ab t_k^2 (c_ab = (alpha_a alpha_b - W_ab) k_ab, t_k = (a_k - b_k) / w_k) and
 * tr W in f64 with a fixed summation order (bitwise repeatable); dh = S_0 / h, dw_k = (S_k - S_0 / d) / (2 w_k). */
int gpx_gp_dloglh_dtheta(gpx_gp_t *gp, double *out);
/* dlh / d(theta) (gp/gp.py:435-465, gp_c.pyx:52-67) and d2lh / d(theta)^2 (gp/gp.py:467-502,
 * gp_c.pyx:70-111), both HOST float64: dlh[n_params + 1], d2lh[(n_params + 1)^2] row-major, parameter
 * order (kernel params..., s); either pointer may be NULL.  Device resident: K^-1, the products
 * K^-1 dK_i (one MFMA GEMM per kernel parameter) and every trace / quadratic form stay in HBM, the
 * kernel derivatives inside traces and quadratic forms are evaluated on the fly; only the scalars
 * return.  All NaN when the factorisation failed (gp/gp.py:458-462,493-497).  Native kernels only
 * (periodic: d == 1).  d2loglh (extension, may be NULL): the Hessian of the LOG marginal likelihood,
 * d2lh / lh - (dlh / lh)(dlh / lh)^T, from the same pass; it stays finite where lh underflows to 0
 * (log_lh < MIN, i.e. any n beyond a few hundred) and the reference's lh-scaled Hessian is all zeros.
 * GPX_KERNEL_GAUSSIAN_ARD: GPX_ERR_UNSUPPORTED (this entry and gpx_gp_dm_dtheta). */
int gpx_gp_dlh_d2lh(gpx_gp_t *gp, double *dlh, double *d2lh, double *d2loglh);
/* d mean(xo) / d(theta) -> out (n_params + 1, m) HOST float64 (gp/gp.py:627-662, gp_c.pyx:114-131):
 * dK_i(xo, x) alpha - K(xo, x) K^-1 dK_i alpha with fused on-the-fly mat-vecs and two triangular
 * solves per parameter; no n x n matrix is formed. */
int gpx_gp_dm_dtheta(gpx_gp_t *gp, const double *xo, int64_t m, double *out);
/* Batched ML-II step (BASELINE config 5; the reference's inner step "set params -> read log_lh",
 * gp/gp.py:216-223,337-367, for a table of restarts on the handle's data set).
 * thetas: HOST (B, n_params + 1) row-major, rows (kernel params..., s) -- d + 2 values a row for
 * GPX_KERNEL_GAUSSIAN_ARD, whose rows each get a scaled copy of x (n d elements) in the workspace; log_lh: HOST B doubles;
 * info: HOST B ints or NULL (potrf info per row; -1 for a row with invalid parameters).
 * A row whose parameters the reference rejects with ValueError (kernel parameter < EPS, s < 0,
 * non-finite) yields NaN; a non-positive-definite row or logdet < MIN yields -inf.
 * The kernel matrices of the rows are held in HBM together and factored in lock-step (every
 * launch covers all of them); chunked by free memory (cap: environment GPX_BATCH_MAX).
 * Leaves the handle's own fitted state untouched. */
int gpx_gp_fit_batch(gpx_gp_t *gp, const double *thetas, int64_t B, double *log_lh, int *info);
/* The same step WITH the gradient of every row (gp/gp.py:398-433 `dloglh_dtheta`, gp_c.pyx:34-49 -- the quantity the
 * reference's removed `fit_MLII` optimised, CHANGELOG.md:19): the lock-step factorisation above, then per row
 * K^-1 = L^-T L^-1 from the row's own factor and the fused trace / quadratic-form pass of gpx_gp_dloglh_dtheta.
 * dloglh: HOST (B, n_params + 1) row-major, order (kernel params..., s); all NaN for a row that is not positive
 * definite (gp/gp.py:424-428) or has invalid parameters.  logdet_yta (may be NULL): HOST (B, 2) = (log det K,
 * y^T K^-1 y), NaN where the factorisation failed: from them a caller forms the log marginal likelihood WITHOUT the
 * reference's logdet < MIN clamp (gp_c.pyx:22-29), which returns -inf for any well-conditioned n beyond a few
 * thousand and leaves an optimiser nothing to follow (an extension; `log_lh` itself keeps the clamp). */
int gpx_gp_fit_batch_grad(gpx_gp_t *gp, const double *thetas, int64_t B, double *log_lh, double *dloglh,
                          double *logdet_yta, int *info);
/* The same table under the leave-one-out criterion: loo_log_lh HOST B doubles, dloo HOST (B, n_params + 1), what
 * gpx_gp_loo_grad returns for a handle fitted at the row's parameters.  The lock-step factorisation and the groups of
 * gpx_gp_fit_batch_grad; a group's K^-1 whole, its Y Y^T products in lock-step.  A row with invalid parameters: NaN and
 * NaN; a row that is not positive definite: -inf and NaN (no logdet < MIN clamp: the criterion has no determinant);
 * info as above. */
int gpx_gp_fit_batch_loo(gpx_gp_t *gp, const double *thetas, int64_t B, double *loo_log_lh, double *dloo, int *info);
/* Checkpoint of a fitted handle (the reference persists by pickling its memoised host arrays,
 * gp/gp.py:78-92; a 32 GiB factor cannot go that way).  File: header (dtype, kernel, n, d, params, s,
 * logdet, y^T alpha, info), x, y, alpha as float64, then the LOWER trapezoid of L in row blocks
 * (rows [r0, r1) x columns [0, r1), packed, handle dtype).  Streamed through two pinned staging
 * buffers of GPX_IO_BLOCK_BYTES (default 64 MiB) each: host memory use does not grow with n.
 * gpx_gp_load creates a NEW handle on the current device, fitted, without recomputing anything. */
int gpx_gp_save(gpx_gp_t *gp, const char *path);
int gpx_gp_load(gpx_gp_t **gp, const char *path);
/* what a handle holds (any pointer may be NULL); x: (n, d), y: (n,) HOST float64.  params3: (h, NaN, NaN) for
 * GPX_KERNEL_GAUSSIAN_ARD (gpx_gp_get_params has them all); x is what set_data gave, never the scaled copy.
 * Checkpoints of GPX_KERNEL_GAUSSIAN_ARD carry the d widths behind the header; the other families' files are unchanged. */
int gpx_gp_describe(gpx_gp_t *gp, int *dtype, int *kernel, int64_t *n, int *d, double *params3, double *s);
int gpx_gp_get_xy(gpx_gp_t *gp, double *x, double *y);
/* timing of the last fit, milliseconds per stage (HIP events on the handle's
 * stream): [0] kernel build [1] potrf [2] solve [3] logdet+dot [4] total.
 * Up to n = 16384 the forward substitution L t = y is done inside [1] (y is carried
 * as one more row of the matrix through the factorisation) and [2] is the backward
 * solve alone. */
int gpx_gp_last_timing(gpx_gp_t *gp, float *ms5);
/* raw device views for tests / multi-GPU drivers (do not free); A has n + 1 rows of lda
 * elements (row n is the handle's work row, see gpx_gp_last_timing) */
int gpx_gp_device_ptrs(gpx_gp_t *gp, void **A, int64_t *lda, void **x, void **y,
                       void **alpha, void **stream);

/* ------------------------------------------------------- posterior paths -- */
/* S draws of the posterior FUNCTION (pathwise conditioning: Matheron's rule; Wilson et al. 2020), each one weight vector
 * resident in HBM, to be evaluated at any number of points afterwards:
 *   f_s(a) = phi(a) . Theta_s + sum_j k(a, x_j) V[s, j],    V_s = alpha - Kxx^-1 (Phi(x) Theta_s + sigma E_s)
 * GPX_KERNEL_GAUSSIAN and GPX_KERNEL_GAUSSIAN_ARD only.  On the handle's view -- points p = x (Gaussian) or x / w (ARD),
 * isotropic constants (h_v, w_v) = (h, w) or (h / sqrt(wbar), 1), k0 = h_v^2 / (w_v sqrt(2 pi)) -- and with z the sequence
 * of gpx_d_randn (stream 0 stays gpx_gp_sample's; streams 4 and 5 are gpx_cg_probes'):
 *   Omega[f, k] = z(seed, 1, f d + k) / w_v     f < F, k < d    spectral frequencies, DOUBLE for both dtypes
 *   Theta[s, q] = z(seed, 2, s 2F + q)          s < S, q < 2F   feature weights, handle dtype
 *   E[s, j]     = z(seed, 3, s n + j)           j < n           the observation-noise draw; sigma = the GP's s
 *   phi(a)      = sqrt(k0 / F) [cos(Omega a); sin(Omega a)]     (gpx_d_rff_features; no phase term)
 * Row s of Theta and E depends on s alone: the random inputs of S' < S paths are a prefix of those of S.  The approximation
 * lies in the prior only (covariance error O(k0 / sqrt(F))); the data update is exact.  The draws are of the LATENT function:
 * observation noise is not added to the values.
 * gpx_gp_paths_create: on the handle's stream -- Omega, Theta; R = sigma E; R += Theta Phi(x)^T in row chunks of x (a multiple
 * of 128 rows: gpx_d_rff_features, then gpx_d_gemm_nt); R <- R L^-T; R <- R L^-1; V = alpha - R.  Synchronous.  The result
 * owns Omega, Theta, V (S x lda), a copy of the view's points and the constants and never refers to `gp` again: `gp` may
 * be refitted or destroyed, and is itself unchanged except for block operators completed as by any gpx_gp_cov.
 * Preconditions and statuses of gpx_gp_sample (fitted, positive definite, finite y); GPX_ERR_UNSUPPORTED for the periodic
 * family and for a handle fitted from gpx_gp_set_K; GPX_ERR_ARG for S < 0 or F < 1.  On failure *paths = NULL. */
typedef struct gpx_paths gpx_paths_t;
int gpx_gp_paths_create(gpx_gp_t *gp, int64_t S, int64_t F, uint64_t seed, gpx_paths_t **paths);
/* f_s(xo_i) -> out (S, m) HOST float64, xo (m, d) HOST float64, in row chunks of xo (chunk_rows: 0 = automatic, else a
 * multiple of 128; gpx_gp_var's contract).  Per chunk: upload (ARD: gpx_d_scale_points), gpx_d_rff_features,
 * out_c = Theta Phi_c^T by gpx_d_gemm_nt into a zeroed block, gpx_d_kmat_apply, one download.  m == 0 and S == 0 are legal.
 * The chunk's device buffers belong to the paths handle and only ever grow: repeated evaluations allocate once.  One host thread
 * at a time per paths handle. */
int gpx_paths_eval(gpx_paths_t *paths, const double *xo, int64_t m, int64_t chunk_rows, double *out);
/* d f_s(xo_i) / d xo_ik -> grad (S, m, d) HOST float64, and with values != NULL also f_s(xo_i) -> values (S, m); xo (m, d)
 * HOST float64.  On the handle's view (a = xo, or xo / w for ARD, whose component k is then divided by w_k):
 *   d f_s / d a_k = sqrt(k0 / F) sum_f Omega[f, k] (Theta[s, F + f] cos(Omega_f . a) - Theta[s, f] sin(Omega_f . a))
 *                   - 1 / w_v^2 sum_j V[s, j] (a_k - p_jk) k(a, p_j)
 * gpx_paths_eval's contract: chunk_rows 0 (automatic) or a multiple of 128, m == 0 and S == 0 legal, the chunk's buffers
 * carved from the handle's grow-only block, one host thread at a time per handle.  Per chunk (GPX_ROUTE_PATHS_GRAD_CHUNK,
 * one hit each): upload (ARD: gpx_d_scale_points), gpx_d_rff_features_grad, the chunk's S x round_up(rows d, 16) block
 * zeroed, Theta Psi_c^T into it by gpx_d_gemm_nt, gpx_d_kmat_apply_grad into the same block, one download.  With values the
 * steps of gpx_paths_eval run on the same uploaded chunk: the values are bit for bit gpx_paths_eval's for the same
 * chunk_rows.  Automatic chunk: the largest multiple of 128 rows, at most 4096, whose feature blocks -- rows (d + 1)
 * round_up(2F, 16) elements -- fit 512 MiB, never fewer than 128; m <= that takes exactly one chunk. */
int gpx_paths_grad(gpx_paths_t *paths, const double *xo, int64_t m, int64_t chunk_rows, double *values, double *grad);
/* the state as HOST float64: omega (F, d), theta (S, 2F), V (S, n); any pointer may be NULL */
int gpx_paths_get(gpx_paths_t *paths, double *omega, double *theta, double *V);
/* any pointer may be NULL; kernel: the family of the GP the paths came from */
int gpx_paths_describe(gpx_paths_t *paths, int *dtype, int *kernel, int64_t *n, int *d, int64_t *S, int64_t *F, uint64_t *seed);
/* diagnostic (tools/paths_probe.py): how long gpx_gp_paths_create took, milliseconds (HIP events on the source's stream): [0]
 * features + products (R += Theta Phi(x)^T) [1] the two sweeps [2] the rest (generators, the copy of the points, V = alpha - R)
 * [3] total; zeros for S == 0 */
int gpx_debug_paths_timing(gpx_paths_t *paths, float *ms4);
int gpx_paths_destroy(gpx_paths_t *paths);

/* ------------------------------------------- sparse GP on inducing points -- */
/* Titsias' collapsed bound (2009; "SGPR") on M inducing inputs z: O(N M^2) time, O(M^2 + M chunk) memory, nothing N x N.
 * One formulation (DESIGN 3.3 "Sparse GP on inducing points"), s the noise standard deviation, eps the jitter:
 *   Kuu = K(z, z) + eps I = Luu Luu^T        Phi = sum_c K(z, x_c) K(x_c, z)      b = sum_c K(z, x_c) y_c
 *   X = Luu^-1 Phi Luu^-T                    B = I + X / s^2 = LB LB^T            c = LB^-1 Luu^-1 b / s
 *   elbo = [-sum log diag LB] + [-N/2 log 2 pi - N log s] + [-yy / (2 s^2)] + [c.c / (2 s^2)] + [-(kff - tr X) / (2 s^2)]
 *          terms5:  0 log-det        1 noise                  2 data fit        3 quadratic       4 trace
 *   mean(a) = k(a, z) w,  w = Luu^-T LB^-T c / s
 *   var(a)  = k(a, a) - |Luu^-1 k(z, a)|^2 + |LB^-1 Luu^-1 k(z, a)|^2      cov likewise with the two blocks' products
 * Kuu + Phi / s^2 is never factored: log|A| - log|Kuu| cancels badly, B is well conditioned.
 * The handle keeps x (N, d), y, z (M, d) in HBM in its dtype and makes its device current in every call, as gpx_gp_t does;
 * every call is synchronous.  All three kernel families (the ARD family on points scaled by gpx_d_scale_points at fit time),
 * every d gpx_d_kmat takes, both dtypes.  b, yy, kff, tr X and the scalars of the bound are DOUBLE for both dtypes. */
typedef struct gpx_sgp gpx_sgp_t;
int gpx_sgp_create(gpx_sgp_t **h, int dtype, int kernel, int64_t n, int64_t m_inducing, int d);
int gpx_sgp_destroy(gpx_sgp_t *h);
/* x: (n, d), y: (n,), z: (m_inducing, d), HOST float64 (converted on upload); any of them NULL: that array is kept.
 * Forgets the fit. */
int gpx_sgp_set_data(gpx_sgp_t *h, const double *x, const double *y, const double *z);
/* The fit, on the handle's stream:
 *   1. Kuu (gpx_d_kmat, lower, diag_add = jitter), gpx_d_potrf.  A non-zero info: *stage = 1, *pivot = it, and the call returns.
 *   2. the chunk loop over columns of x, chunk_cols wide (0: automatic -- gpx_debug_sgp_plan; else a multiple of 128), one
 *      GPX_ROUTE_SPARSE_CHUNK hit each:  G = K(z, x_c) (M x c, ld = the chunk width) by gpx_d_kmat;  G G^T on the lower tiles
 *      by the product kernel's batched launch as a split over the depth (slices of the plan's width; slice p of every chunk
 *      adds to partial accumulator p; the ragged last slice of the last chunk is a call of its own), GPX_PROF_SPARSE_GRAM
 *      around each chunk's products;  b += G y_c (gpx_d_gemv_acc).  Then the partials are summed in slice order
 *      (gpx_d_sum_slices_lower).  No atomics anywhere: a repeated fit gives the same bits.
 *   3. the M x M tail: gpx_d_mirror_lower, gpx_d_trsm_right_lt, gpx_d_transpose, gpx_d_trsm_right_lt (X);
 *      gpx_d_sgp_form_B (B lower and tr X); gpx_d_potrf (a non-zero info: *stage = 2); two gpx_d_trsv_lower for c, two
 *      more for w; gpx_d_logdet_chol, gpx_d_dot.
 * params as gpx_gp_set_params; s > 0; jitter >= 0, finite.  *stage = *pivot = 0 after a good fit.  The status is GPX_OK
 * whether or not a factorisation failed (the matrix is the caller's); GPX_ERR_INTERNAL as gpx_gp_fit. */
int gpx_sgp_fit(gpx_sgp_t *h, const double *params, double s, double jitter, int64_t chunk_cols, int *stage, int *pivot);
/* stage and pivot of the last fit (both 0: fitted and positive definite) */
int gpx_sgp_info(gpx_sgp_t *h, int *stage, int *pivot);
/* the bound and its five terms (terms5 may be NULL); -inf and NaN terms when a factorisation failed */
int gpx_sgp_elbo(gpx_sgp_t *h, double *elbo, double *terms5);
/* predictions at xo (m, d) HOST float64 -> HOST float64.  GPX_ERR_ARG when the last fit's stage is non-zero.
 * mean: one gpx_d_mean pass against z with w.  var (m,): row chunks as gpx_gp_var (chunk_rows 0 or a multiple of 128, one
 * GPX_ROUTE_VAR_CHUNK hit each): V = K(xo_c, z), V <- V Luu^-T, W <- V LB^-T, gpx_d_var_rows2; not clamped at zero.
 * cov (m, m): K(xo, xo) - V V^T + W W^T by gpx_d_gemm_nt. */
int gpx_sgp_mean(gpx_sgp_t *h, const double *xo, int64_t m, double *out);
int gpx_sgp_var(gpx_sgp_t *h, const double *xo, int64_t m, int64_t chunk_rows, double *out);
int gpx_sgp_cov(gpx_sgp_t *h, const double *xo, int64_t m, double *out);
/* the fit's state as HOST float64, for tests and inspection: Luu, LB (M x M dense, zero upper triangle), c (M), Phi (M x M,
 * lower triangle, zero above), b (M); any pointer may be NULL.  After a stage-1 failure only Luu's leading columns mean
 * anything; after stage 2 everything but LB and c. */
int gpx_sgp_get(gpx_sgp_t *h, double *Luu, double *LB, double *c, double *Phi, double *b);
/* milliseconds of the last fit (HIP events on the handle's stream): [0] Kuu + its factor [1] the chunks' kernel builds
 * [2] the chunks' Gram products, b and the slice sum [3] the M x M tail [4] total */
int gpx_sgp_last_timing(gpx_sgp_t *h, float *ms5);
/* The gradient of the bound in the hyper-parameters, z held fixed (gpx_sgp_grad_z below: the one in z beside it): grad (HOST, nkp + 1 doubles) = d elbo / d (kernel
 * parameters..., s), in the order of gpx_sgp_fit's params.  Needs a fit of stage 0 (GPX_ERR_ARG otherwise, as the predictions).
 * With Sigma = Kuu + Phi / s^2 = Luu B Luu^T and w = Sigma^-1 b / s^2 (the mean's weights, on the device since the fit):
 *   T  = Kuu^-1 - Sigma^-1 - w w^T                         Gu = T / 2 - Kuu^-1 Phi Kuu^-1 / (2 s^2)    = d elbo / d Kuu
 *   Gf = (T K(z, x) + w y^T) / s^2                         = d elbo / d K(z, x)
 *   d elbo / d theta_p = sum Gu o dKuu/dtheta_p + sum Gf o dK(z, x)/dtheta_p - N dk(0)/dtheta_p / (2 s^2)
 *   d elbo / d s       = -N / s + (yy - 2 w.b + N k(0) - tr(T Phi)) / s^3
 * (tr(T Phi) = tr X - tr((Sigma^-1 + w w^T) Phi): the N-sized pass sums it beside the derivatives).
 * The JITTER is held at the value of the fit: it is not differentiated, even where the caller derived it from the kernel's
 * parameters.  Three parts, all on the handle's stream:
 *   1. M x M, O(M^3), blocks the library has (gpx_d_trsm_right_lt on the identity and on products, gpx_d_gemm_nt), from Luu, LB
 *      and the fit's X.  No difference of inverses is formed -- where the data do not reach (X ~ 0, Kuu's small eigenvalues)
 *      Kuu^-1 and Sigma^-1 agree and are of size 1 / jitter, and in fp32 their difference would be rounding error.  With
 *      B - I = X / s^2, Y = Luu^-T LB^-T and A = Luu^-T X LB^-T:
 *        Kuu^-1 - Sigma^-1 = Luu^-T (X / s^2) B^-1 Luu^-1 = A Y^T / s^2          Gu = -(A A^T / s^4 + w w^T) / 2
 *      (I - B^-1 - X / s^2 = -(B - I)^2 B^-1).  The contraction of Gu with dKuu/dtheta is the dense gradient's tile reduction
 *      on z with (a, M) = (w, -A A^T / s^4), for which a a^T - M = -2 Gu.
 *   2. a second pass over x in column chunks -- the fit's plan and chunk_cols rule, but TWO c x M blocks in the work buffer:
 *      an automatic width that does not fit twice is halved (to a multiple of 128) -- one GPX_ROUTE_SPARSE_CHUNK hit each:
 *      K(x_c, z) by gpx_d_kmat;  P = K(x_c, z) T by gpx_d_gemm_nt (2 M^2 c flops);  the rectangular tile reduction
 *      sum_ji (P[j, i] + y_j w_i) dk_p(x_j, z_i), derivatives formed in the tile from the staged points (GPX_PROF_SPARSE_GRAD),
 *      f64 sums for both dtypes, one partial per workgroup and parameter.
 *   3. the host adds the partials in workgroup order and the chunks in chunk order.  No floating-point atomics anywhere: a
 *      repeated call returns the same bits.  Nothing the fit left behind is written: elbo and the predictions are unchanged. */
int gpx_sgp_grad(gpx_sgp_t *h, int64_t chunk_cols, double *grad);
/* milliseconds of the last gpx_sgp_grad (HIP events on the handle's stream): [0] the M x M part (with its reduction on z)
 * [1] the chunks' kernel builds [2] the chunks' products K(x_c, z) T [3] the chunks' tile reductions (with the copy of their
 * partials) [4] total.  GPX_ERR_ARG before the first gradient of the current fit. */
int gpx_sgp_last_grad_timing(gpx_sgp_t *h, float *ms5);
/* The gradient of the bound in the inducing inputs, jointly with the one above: grad_z (HOST, M x d doubles, row i = z_i) =
 * d elbo / d z, grad as gpx_sgp_grad's (it may be NULL here).  kff does not depend on z and the jitter is held fixed, so with Gu
 * and Gf as above (Gf[i, j] = (P[j, i] + y_j w_i) / s^2, P = K(x, z) T):
 *   d elbo / d z_ik = sum_i' 2 Gu[i, i'] dk(z_i, z_i')/dz_ik  +  sum_j Gf[i, j] dk(z_i, x_j)/dz_ik
 *   gaussian families  dk(a, b)/da_k = -(a_k - b_k) / w_k^2 k(a, b)        periodic (d = 1)  -sin((a - b) / p) / (p w^2) k(a, b)
 * (the term i' = i is zero: the kernels are stationary).  Both sums are ONE operation, gpx_d_rect_zgrad below:
 *   over x, per chunk:  C = P, (u, v) = (y_c, w), rows x_c, columns z, scale 1 / s^2 -- beside the tile reduction of part 2, on
 *     the same K(x_c, z) and P: one pass over x gives both gradients, at the same GPX_ROUTE_SPARSE_CHUNK hits;
 *   over z, once:       C = -A A^T / s^4 (part 1's lower triangle, mirrored by gpx_d_mirror_lower), (u, v) = (-w, w), rows =
 *     columns = z, scale 1:  C - w w^T = 2 Gu.
 * The ARD family runs on the scaled points and divides column k by w_k.  The partials of the chunks add into ONE f64 M x d
 * accumulator in chunk order on the handle's stream; no atomics: a repeated call returns the same bits, and grad is bit for
 * bit gpx_sgp_grad's.  The work buffer grows by that accumulator, -w and the kernel's partials; the fit's state is untouched.
 * No bounds on z are known to the library: an optimiser moves it freely. */
int gpx_sgp_grad_z(gpx_sgp_t *h, int64_t chunk_cols, double *grad, double *grad_z);
/* milliseconds of the z-gradient's own kernels in the last gpx_sgp_grad_z: [0] Kuu's share (the mirror and the pass on z) [1] the
 * chunks' passes.  gpx_sgp_last_grad_timing's five stages keep their meaning ([3] begins behind these kernels, [4] includes
 * them).  GPX_ERR_ARG before the first gpx_sgp_grad_z of the current fit. */
int gpx_sgp_last_zgrad_timing(gpx_sgp_t *h, float *ms2);
/* Depth slices per chunk for later fits of this handle: 0 = the plan's (the default), P >= 1 = exactly that many (1: one
 * plain product per chunk).  For measurements (tools/sparse_bench.py); results differ in the last bits between values. */
int gpx_sgp_set_split(gpx_sgp_t *h, int slices);
/* Greedy conditional-variance selection of inducing points (Burt, Rasmussen and van der Wilk 2020): a pivoted partial
 * Cholesky of K(x, x), which is never formed.  No handle: the call uploads x, runs on a stream of its own and is synchronous.
 * All pointers are HOST.  x: (n, d) float64; params: the kernel's, as gpx_sgp_fit's.  All sums are f64 for both dtypes.
 *   dres[i] = k(x_i, x_i), the element gpx_d_kmat would store (the ARD family: points scaled once by gpx_d_scale_points)
 *   step m = 0, 1, ...:
 *     1. p = the unpicked index with the largest dres; on a tie the SMALLEST index.  first >= 0: step 0 takes `first`.
 *     2. dres[p] <= tol: stop, *count = m.
 *     3. R[m, i] = (k(x_p, x_i) - sum_{j < m} R[j, p] R[j, i]) / sqrt(dres[p]) for every i, j ascending; R is kept in the dtype.
 *     4. dres[i] -= R[m, i]^2 with R[m, i] as stored; p is picked and its residual counts as 0 from then on.
 *     5. trace[m + 1] = sum_{i unpicked} dres[i].          trace[0]: that sum before any pick.
 * trace[M] is kff - tr X of the bound at the M picks and jitter 0 -- the curve to choose M from.
 * index, pivot: m_max entries, *count valid (pivot[m] = dres[p] at step m).  trace: m_max + 1 entries, *count + 1 valid.
 * R: NULL, or m_max x n doubles, dense; the first *count rows are written.  On the device R is m_max x round_up(n, 128) in the
 * dtype: GPX_ERR_NOMEM, with the bytes needed in gpx_last_error(), when that does not fit the free memory.
 * Two launches per step (select_pick_kernel: one workgroup; select_step_kernel: one thread per 16 bytes of a row of R), all
 * enqueued at once; stream order is the only dependency, no atomics: every output repeats bit for bit.
 * GPX_ERR_ARG: n < 1, m_max outside 1 .. n, tol negative or not finite, first >= n, a kernel or d gpx_d_kmat refuses, NULL
 * arguments, non-finite params; nothing is written then.  GPX_PROF_SELECT: one record per call.  GPX_ROUTE_SELECT_STEP: one
 * hit per step that picked a point. */
int gpx_sgp_select(int dtype, int kernel, const double *x, int64_t n, int d, const double *params,
                   int64_t m_max, double tol, int64_t first,
                   int64_t *index, double *pivot, double *trace, double *R, int64_t *count);
/* host arithmetic only: the plan of a fit -- columns per chunk, chunks, depth slices per full chunk and their width.
 * chunk_cols 0: the largest multiple of 128, at most 16384, whose M x c block fits a quarter of free_bytes; one chunk of
 * round_up(n, 128) when n is within it.  slices: P = as many as make tiles x P cover 256 workgroups (tiles = the 128 x 128
 * tiles of the lower triangle), at least 8, at most 16, and no more than keep the partial accumulators within 2 GiB -- a
 * function of (m_inducing, dtype) alone; split > 0 replaces P.  No slice is narrower than 128 columns: the width is the
 * chunk's share cols / P rounded up to 128, *slices = cdiv(cols, width) <= P. */
int gpx_debug_sgp_plan(int dtype, int64_t n, int64_t m_inducing, int64_t chunk_cols, int split, size_t free_bytes,
                       int64_t *cols, int64_t *chunks, int *slices, int64_t *slice_cols);
/* the same for the gradient pass (gpx_sgp_grad, gpx_sgp_grad_z), which holds two cols x ldm blocks (ldm = m_inducing rounded
 * up to 16) where the fit holds one m_inducing x cols: the fit's cols; when the two blocks exceed a quarter of free_bytes an
 * automatic plan (chunk_cols 0) halves them once, rounded down to 128 and never below 128; what still does not fit is
 * GPX_ERR_NOMEM.  *chunks = cdiv(n, *cols).  chunk_cols is checked here and in gpx_debug_sgp_plan alike: GPX_ERR_ARG. */
int gpx_debug_sgp_grad_plan(int dtype, int64_t n, int64_t m_inducing, int64_t chunk_cols, int split, size_t free_bytes,
                            int64_t *cols, int64_t *chunks);
/* The new kernels, one building block each (DEVICE pointers, `dtype` unless said otherwise; fixed order, no atomics).
 * gpx_d_sum_slices_lower: out[i, j] = sum_p P[p sP + i ldp + j] for j <= i < n, p ascending, summed in f64, rounded once;
 *   the strict upper triangle of out is not written.
 * gpx_d_gemv_acc: acc[i] += sum_j G[i, j] y[j]  for i < rows, j < cols; acc DOUBLE; one workgroup per row, f64 sums.
 * gpx_d_mirror_lower: A[j, i] = A[i, j] for j < i < n.
 * gpx_d_transpose: out[j, i] = in[i, j] for i, j < n; out != in.
 * gpx_d_sgp_form_B: B[i, j] = (i == j) + X[i, j] / s^2 for j <= i < n (upper not written); trace_dev[0] = sum_i X[i, i]
 *   (DOUBLE, one workgroup, fixed order).
 * gpx_d_var_rows2: out_dev[i] = kdiag(i) - sum_j V[i, j]^2 + sum_j W[i, j]^2 -- gpx_d_var_rows' contract (kdiag from the
 *   kernel family at xo[i], f64 sums, out DOUBLE) with a second block of the same shape and pitch; not clamped.  The row sums
 *   go through a block of `rows` doubles that the call allocates: it waits for the stream before it returns. */
int gpx_d_sum_slices_lower(int dtype, const void *P, int64_t ldp, int64_t sP, int slices, int64_t n, void *out, int64_t ldo, void *stream);
int gpx_d_gemv_acc(int dtype, const void *G, int64_t rows, int64_t cols, int64_t ldg, const void *y, double *acc_dev, void *stream);
int gpx_d_mirror_lower(int dtype, void *A, int64_t n, int64_t lda, void *stream);
int gpx_d_transpose(int dtype, const void *in, int64_t ldi, void *out, int64_t ldo, int64_t n, void *stream);
int gpx_d_sgp_form_B(int dtype, const void *X, int64_t ldx, int64_t n, double s, void *B, int64_t ldb, double *trace_dev, void *stream);
int gpx_d_var_rows2(int dtype, int kernel, const void *V, const void *W, int64_t rows, int64_t n, int64_t ldx, const void *xo, int d,
                    const double *params, double *out_dev, void *stream);
/* gpx_d_rect_zgrad: the rectangular tile pass whose result is per column point and dimension,
 *     out_dev[i, k] += scale * sum_j (C[j, i] + u_j v_i) dk(q_i, r_j)/dq_ik        i < m, k < d, j < n
 *   rows r (n, d), columns q (m, d), C (n x ldc), u (n), v (m) in `dtype`; out_dev (m, d) DOUBLE, ADDED to; kernel
 *   GPX_KERNEL_GAUSSIAN (any d the tile's LDS holds) or GPX_KERNEL_PERIODIC (d = 1), params the family's.  The ARD family: the
 *   points scaled by gpx_d_scale_points, params = (h / sqrt(wbar), 1) and col_div (HOST, d doubles) = the widths -- column k
 *   is divided by col_div[k]; NULL otherwise.  64 x 64 tiles; a workgroup keeps one column tile, walks a slice of the row
 *   tiles and a window of dimensions (4, 16 or 32 wide; beyond d = 32 further windows evaluate k again); k is formed in `dtype` as
 *   gpx_d_kmat forms it (a clamped pair adds exactly 0), the coefficient, the products and the sums in f64, the difference
 *   r_jk - q_ik directly.  One partial per (slice, i, k) into partial_dev -- gpx_rect_zgrad_scratch doubles, a function of
 *   (kernel, m, d) -- and a second kernel adds the slices in slice order.  No atomics; enqueues and returns.
 * gpx_rect_zgrad_scratch: host arithmetic, the DOUBLES partial_dev must hold. */
int gpx_rect_zgrad_scratch(int kernel, int64_t m, int d, size_t *doubles);
int gpx_d_rect_zgrad(int dtype, int kernel, const void *r, int64_t n, const void *q, int64_t m, int d, const double *params,
                     const void *C, int64_t ldc, const void *u, const void *v, double scale, const double *col_div,
                     double *partial_dev, double *out_dev, void *stream);

/* gpx_d_lowrank_reduce: the tile reduction whose coefficient is low rank and formed inside the tile (csrc/gpx_lrgrad.hip),
 *     S_p = sum_{j,i} c_ji dk(x_j, x_i)/dtheta_p,   c_ji = sum_{t<T} U[t, j] V[t, i],   last = sum_j c_jj       j, i < n
 *   x (n, d), U and V (T x ld, ld >= n; the columns [n, ld) are never read) DEVICE float64; out HOST doubles:
 *   [P0, P1, P2, last] for GPX_KERNEL_GAUSSIAN (d up to what the tile's LDS holds) and GPX_KERNEL_PERIODIC (d = 1), params the
 *   family's; [S_0, S_1 .. S_d, last] (S_0 = sum c k, S_k = sum c k t_k^2) for GPX_KERNEL_GAUSSIAN_ARD, where x are the points
 *   scaled by gpx_d_scale_points and params = (h / sqrt(wbar), 1) -- the slots of the dense gradient's reduction.  No n x n
 *   object exists: 64 x 64 tiles of the whole square; a tile stages its 64 + 64 points and the T x 64 slices of U (rows) and V
 *   (columns) in LDS, a pair forms its coefficient by a T-long dot and its distance and derivatives once; everything f64.  At
 *   most 32 rows of U and V go per launch (GPX_ROUTE_LOWRANK, GPX_PROF_LOWRANK: one each); a larger T is several launches whose
 *   sums are added in launch order.  One partial per workgroup and quantity, added by the host in workgroup order: no atomics,
 *   two calls give the same bits.  Synchronous.  GPX_F32 is GPX_ERR_UNSUPPORTED ("float64 only"); GPX_ERR_ARG for NULL
 *   pointers, T < 1, n < 1, ld < n. */
int gpx_d_lowrank_reduce(int dtype, int kernel, const void *x, int64_t n, int d, const double *params, const void *U, const void *V,
                         int64_t ld, int64_t T, double *out, void *stream);

/* ------------------------------------- exact GP past the n x n factor: CG -- */
/* (K + s^2 I) X^T = B^T by batched preconditioned conjugate gradients; K(x, x) is never formed (Gardner et al. 2018; Wang et
 * al. 2019).  Device memory is n (d + 2 rank + 6 S + 2) doubles and small change, S = min(columns, 32): nothing scales with
 * n^2 (DESIGN 3.3 "Exact GP past the factor").  GPX_F64 only: GPX_F32 is GPX_ERR_UNSUPPORTED, and so is a d beyond the fused
 * route of gpx_d_kmat_apply (d <= 47), the only product the solver uses: with GPX_KAPPLY_FUSED_MAX lowered by
 * gpx_debug_kapply_fused_max the groups shrink to that many columns, and at 0 a solve is GPX_ERR_UNSUPPORTED.  All three kernel families (the
 * ARD family on points scaled once by gpx_d_scale_points).  The handle keeps x (n, d) and y (n) in HBM, has one stream, makes
 * its device current in every call as gpx_gp_t does, and every call is synchronous.  All pointers below are HOST.
 *   preconditioner  P = R^T R + s^2 I, R (k x n) the pivoted partial Cholesky of gpx_sgp_select on the resident x
 *   one iteration   q = s^2 p, then gpx_d_kmat_apply(x_rows, x, p -> q) on row blocks of x (at most 32 columns at a time: the
 *                   fused route);  delta = p.q, alpha = rho / delta, x += alpha p, r -= alpha q, rr = r.r;
 *                   z = P^-1 r, rho' = r.z, beta = rho' / rho, p = z + beta p
 * Every dot is f64, summed per workgroup and then in ascending workgroup order by a second launch, which also forms alpha,
 * beta and the flags on the device; no atomics: a repeated solve gives the same bits.
 * Freezing: a column whose rr <= tol^2 b.b (|r| <= tol |b|) is frozen at that iteration -- its x, r and p no longer change
 * whatever its batch companions do, and that iteration is its count.  b = 0: frozen from the start, x = 0, 0 iterations,
 * relres 0.  delta <= 0 or not finite (positive definiteness lost to rounding): frozen, the count is MINUS the iteration.
 * The host reads the group's residual norms and flags once per iteration, in one copy, and stops when every column is frozen
 * or at maxiter.  Not converged at maxiter is not an error: relres holds what was reached. */
typedef struct gpx_cg gpx_cg_t;
int gpx_cg_create(gpx_cg_t **h, int dtype, int kernel, int64_t n, int d);
int gpx_cg_destroy(gpx_cg_t *h);
/* x: (n, d), y: (n,) float64; either may be NULL: that array is kept.  A new x forgets the preconditioner, either forgets
 * the solution for y. */
int gpx_cg_set_data(gpx_cg_t *h, const double *x, const double *y);
/* The preconditioner of (params, s) -- params as gpx_gp_set_params, s > 0 -- which every later solve must name again.
 * rank in 0 .. n; 0: none (P = I).  The selection (tol: its stop rule, as gpx_sgp_select's) runs on the resident x and R stays
 * on the device; *count <= rank rows are used (count < rank is not an error: the selection stopped at tol).  Then
 * C = s^2 I + R R^T (gpx_d_gemm_nt on the lower triangle), C = Lc Lc^T (gpx_d_potrf) and R^T (gpx_d_transpose's kernel).
 * GPX_ERR_ARG naming the pivot when that factorisation fails (it cannot for s > 0 in exact arithmetic).
 * GPX_PROF_SELECT and GPX_ROUTE_SELECT_STEP as gpx_sgp_select. */
int gpx_cg_precond(gpx_cg_t *h, const double *params, double s, int64_t rank, double tol, int64_t *count);
/* out = P^-1 V for S vectors (V, out: S x n dense), by Woodbury: (V - (V R^T) C^-1 R) / s^2 -- two gpx_d_gemm_nt, gpx_d_trsm_right_lt
 * and gpx_d_trsm_right_l on the S x k block, one map.  The block the solver applies, alone. */
int gpx_cg_precond_apply(gpx_cg_t *h, const double *V, int64_t S, double *out);
/* B: S right-hand sides, S x n dense, or NULL with S == 1: the handle's y (that solution stays on the device for gpx_cg_mean).
 * X: S x n (may be NULL with B == NULL).  iters, relres: S entries; relres = sqrt(rr / b.b) of the recurrence.  More than 32
 * columns go in groups of 32 through one set of buffers.  tol >= 0 (the relative residual), maxiter >= 0.  GPX_ERR_ARG when
 * (params, s) are not the preconditioner's.  GPX_PROF_CG: one record per call; GPX_ROUTE_CG_ITER: one hit per iteration of a
 * group. */
int gpx_cg_solve(gpx_cg_t *h, const double *params, double s, const double *B, int64_t S, double tol, int64_t maxiter, double *X,
                 int *iters, double *relres);
/* out[i] = sum_j k(xo_i, x_j) alpha_j, xo (m, d): gpx_d_mean with the last solution for y.  GPX_ERR_ARG if there is none, or
 * if it belongs to other parameters. */
int gpx_cg_mean(gpx_cg_t *h, const double *params, const double *xo, int64_t m, double *out);
/* Predictive variance at xo (m, d), in groups of at most 32 test points: B = K(xo_c, x) (gpx_d_kmat), one batched solve,
 * out[i] = k(xo_i, xo_i) - b_i . x_i (f64, fixed order).  m / 32 solves: for hundreds of points, not millions.  *worst_relres
 * (may be NULL): the largest relres over all columns.  Not clamped at zero. */
int gpx_cg_var(gpx_cg_t *h, const double *params, double s, const double *xo, int64_t m, double tol, int64_t maxiter, double *out,
               double *worst_relres);
/* T probe rows z ~ N(0, P) of the preconditioner in force, made on the device: with g2 = gpx_d_randn(T x n; seed, stream 4)
 * and g1 = gpx_d_randn(T x k; seed, stream 5), z = g1 R + s g2 (one gpx_d_gemm_nt against the resident R^T); rank 0 (P = I):
 * z = g2.  Row t depends on (seed, t) alone: fewer probes are a prefix of more.  out: T x n HOST, or NULL (generated and dropped). */
int gpx_cg_probes(gpx_cg_t *h, int64_t T, uint64_t seed, double *out);
/* One pass of the stochastic estimate of the marginal likelihood and, with want_grad != 0, of its gradient (Gardner et al.
 * 2018): CG's alpha_j, beta_j are the Lanczos coefficients of P^-1/2 (K + s^2 I) P^-1/2 started at P^-1/2 z, so for probes
 * z ~ N(0, P):  log det(K + s^2 I) = log det P + E[rho0 e1^T log(T_z) e1],  rho0 = z . P^-1 z, and
 * tr((K + s^2 I)^-1 dK) = E[w^T dK zt],  w = (K + s^2 I)^-1 z,  zt = P^-1 z  (E[zt z^T] = I).
 * Z: T x n probes (HOST), or NULL: gpx_cg_probes(T, seed).  The handle's solution alpha for y is solved first if it is absent,
 * by the rules of gpx_cg_solve(B == NULL) with this tol and maxiter, and stays.  Per group of at most 32 probes: one solve whose
 * coefficient history cg_fin_kernel records on the device (one download per group; a frozen column's entries are 0) and which
 * keeps W = (K + s^2 I)^-1 Z and Zt; with want_grad one gpx_d_lowrank_reduce over U = -W / T, V = Zt; at the end one for
 * U = V = alpha.  Results (HOST):
 *   rho0, iters, relres  T entries (iters, relres as gpx_cg_solve's)
 *   coef      T x maxiter x 2: coef[t][j] = (alpha_j, beta_j) of probe t, 0 from its last iteration on (beta of the last is 0)
 *   scalars   [0] log det P = 2 sum log diag(Lc) + (n - k) log s^2 (0 at rank 0)   [1] y . alpha
 *   sums      the reduction's slots summed over all launches: G = alpha alpha^T - (1/T) sum_t w_t zt_t^T against dk/dtheta_p
 *   grad      (kernel parameters ..., s) of the estimate: the dense gradient's host half on `sums`; d/ds = s * last
 * sums and grad may be NULL without want_grad.  The estimate's block (history, rho0, Zt, the reduction's partials) is
 * allocated by the first call and only grows: a handle that never asks has the device bytes it had.  GPX_PROF_CG: one record
 * per call; GPX_ROUTE_CG_ITER per iteration of a group; GPX_ROUTE_LOWRANK per launch of the reduction. */
int gpx_cg_lh(gpx_cg_t *h, const double *params, double s, const double *Z, int64_t T, uint64_t seed, double tol, int64_t maxiter,
              int want_grad, double *rho0, int *iters, double *relres, double *coef, double *scalars, double *sums, double *grad);
/* milliseconds (HIP events on the handle's stream): [0] the last gpx_cg_precond; of the last gpx_cg_solve / gpx_cg_var:
 * [1] the products [2] the preconditioner applies (with rho' = r.z) [3] the vector kernels [4] total [5] the status reads --
 * from the end of an iteration's vector kernels to the first launch the host makes once it has the status */
int gpx_cg_last_timing(gpx_cg_t *h, float *ms6);
/* bytes of device memory the handle owns now (this host thread's scratch blocks, which the products use, are not the handle's) */
int gpx_cg_device_bytes(gpx_cg_t *h, size_t *bytes);

/* ------------------------------------------------------------- multi-GPU -- */
/* One GP spread over the GPUs of a node, one PROCESS per GPU (north-star; SURVEY 8e -- the reference has
 * nothing distributed).  1-D block-cyclic block columns of width nb (global block column j on rank
 * j % world); per panel the owner factors, packs and broadcasts it (root = owner, row-chunked so that
 * the next owner's column update hides under the transfer), every rank updates its own block columns;
 * one-panel look-ahead on a high-priority side stream.  The whole schedule -- HIP streams, events and
 * the collectives -- runs in C.
 * Communicator: RCCL over xGMI (librccl is dlopen'ed at first use; libgpx has no link-time dependency on
 * it).  Rank 0 calls gpx_mg_unique_id and distributes the GPX_MG_ID_BYTES out of band (MPI, a file,
 * torch.distributed over gloo ...); every rank then calls gpx_mg_create on its own device
 * (gpx_set_device first).  gpx_mg_create_cb runs the same schedule over host-supplied collectives on
 * DEVICE pointers (tests: several ranks on one GPU over gloo, which RCCL cannot do). */
#define GPX_MG_ID_BYTES 128
typedef struct gpx_mg gpx_mg_t;
typedef int (*gpx_mg_bcast_fn)(void *user, void *dev_ptr, size_t bytes, int root, void *stream);
/* dtype: GPX_F64 / GPX_F32 / 2 (int32); op: 0 sum, 1 max; in place on dev_ptr; 0 = success */
typedef int (*gpx_mg_allreduce_fn)(void *user, void *dev_ptr, size_t count, int dtype, int op, void *stream);
/* can RCCL be used here at all?  dlopen + symbol lookup only (no bootstrap thread, no socket): the pre-flight a
 * launcher runs on every rank before anybody enters ncclCommInitRank */
int gpx_mg_probe(void);
int gpx_mg_unique_id(void *id128);
/* Two-step creation, so that a launcher can AGREE on the outcome of the local step (device memory: the local
 * matrix and two panel buffers; streams) over its own control plane before any rank enters ncclCommInitRank -- a
 * rank that fails to allocate would otherwise leave the others blocked in there for ever:
 *   gpx_mg_create_local (no communicator yet)  ->  all ranks exchange ok / not ok  ->  gpx_mg_connect.
 * gpx_mg_create does both in one call (single process / tests). */
int gpx_mg_create_local(gpx_mg_t **mg, int dtype, int kernel, int64_t n, int d, int64_t nb, int world, int rank);
int gpx_mg_connect(gpx_mg_t *mg, const void *id128);
int gpx_mg_create(gpx_mg_t **mg, int dtype, int kernel, int64_t n, int d, int64_t nb, int world, int rank,
                  const void *id128);
/* what the communicator itself reports (ncclCommCount / ncclCommUserRank / ncclCommCuDevice); nranks = 0 for
 * the callback back-end.  bcast_sag: the panel-broadcast algorithm in force.  Any pointer may be NULL. */
int gpx_mg_comm_info(gpx_mg_t *mg, int *nranks, int *rank, int *device, int *bcast_sag);
/* panel broadcast algorithm: 0 one collective per row chunk (ncclBroadcast), 1 scatter + all-gather by grouped
 * ncclSend / ncclRecv (every xGMI link of the root carries 1 / world of the payload per phase).  Also selected by
 * the environment (GPX_MG_BCAST=sag).  Every rank must set the same mode before the next gpx_mg_fit. */
int gpx_mg_set_bcast(gpx_mg_t *mg, int sag);
/* test hook: the next gpx_mg_fit of this rank behaves as if its factorisation had left `value` in the device
 * info word (value < 0: an internal failure, which every rank must then report as GPX_ERR_INTERNAL) */
int gpx_debug_mg_inject_info(gpx_mg_t *mg, int value);
/* test hook, host arithmetic only (no GPU needed): how panel j of an n x n problem with block width nb on `world`
 * ranks travels -- per row chunk (each its own broadcast + event) six values: first row, end row (relative to the
 * panel's first row; the panel has n + 1 - j nb rows, the rider row included), elements in the chunk, elements per
 * scatter / all-gather piece, elements in the last piece, 1 if the scatter + all-gather form is eligible.
 * Returns the number of chunks (>= 1) or a negative status. */
int gpx_debug_mg_plan(int64_t n, int64_t nb, int world, int chunks, int64_t j, int64_t *out, int cap);
int gpx_mg_create_cb(gpx_mg_t **mg, int dtype, int kernel, int64_t n, int d, int64_t nb, int world, int rank,
                     gpx_mg_bcast_fn bcast, gpx_mg_allreduce_fn allreduce, void *user);
int gpx_mg_destroy(gpx_mg_t *mg);
/* x: (n, d), y: (n,) HOST float64, the same on every rank.  NaN / infinite entries: GPX_ERR_ARG with the
 * check_finite message (as gpx_gp_fit; gpx_mg_fit checks the kernel constants the same way) */
int gpx_mg_set_data(gpx_mg_t *mg, const double *x, const double *y);
/* kernel build (owned block columns) -> distributed Cholesky -> alpha (replicated) -> log_lh with the
 * reference's conventions (gp/gp.py:360-367, gp_c.pyx:17-31); *info = first failing leading minor over
 * all ranks.  Collective: every rank calls it with the same arguments.  Synchronous. */
int gpx_mg_fit(gpx_mg_t *mg, const double *params, double s, double *log_lh, int *info);
/* posterior mean at xo (m, d) HOST float64 -> out (m,) on every rank (each evaluates a slice) */
int gpx_mg_mean(gpx_mg_t *mg, const double *params, const double *xo, int64_t m, double *out);
/* posterior covariance at xo (m, d) HOST float64 -> out (m, m) HOST float64 on every rank: Kxoxo - X X^T with
 * X = Kxox L^-T, L left distributed (a fan-in forward solve over the block columns: one all-reduce of m nb elements
 * per block, one of m x m at the end).  Collective: every rank calls it with the same arguments after the same
 * gpx_mg_fit.  The ranks agree on their local checks and allocations before any work: all go on, or all return the
 * same status (GPX_ERR_ARG when m, xo or params differ between ranks, GPX_ERR_NOMEM when an allocation failed on one).
 * GPX_ERR_ARG after a fit that was not positive definite; GPX_ERR_UNSUPPORTED on a rehearsal handle. */
int gpx_mg_cov(gpx_mg_t *mg, const double *params, const double *xo, int64_t m, double *out);
/* Predictive variance at xo over the distributed factor -> out (m,) HOST float64 on every rank, the same bits everywhere.
 * Collective.  gpx_mg_cov's fan-in forward solve per row chunk of xo (the accumulator is m_c x n instead of m x n), the
 * block owners' row sums of squares (f64, block order) instead of the m x m product, ONE F64 sum all-reduce of m_c values
 * per chunk.  chunk_rows as in gpx_gp_var; 0: the smallest of the ranks' automatic figures.  The ranks agree on m, xo,
 * params and chunk_rows before any work (statuses as gpx_mg_cov: GPX_ERR_ARG when they differ or after a fit that was
 * not positive definite, GPX_ERR_NOMEM when an allocation failed on one, GPX_ERR_UNSUPPORTED on a rehearsal handle). */
int gpx_mg_var(gpx_mg_t *mg, const double *params, const double *xo, int64_t m, int64_t chunk_rows, double *out);
int gpx_mg_get_alpha(gpx_mg_t *mg, double *out);
int gpx_mg_scalars(gpx_mg_t *mg, double *logdet, double *yta, int *info);
/* this rank's times of the last fit, ms (HIP events): [0] kernel build [1] factorisation [2] solves
 * [3] reductions, and the chain inside [1]: [4] panels it factored [5] packs [6] broadcasts (incl.
 * waiting for the root) [7] trailing / column updates */
int gpx_mg_timing(gpx_mg_t *mg, double *ms8);
/* The same with the classes added in round 5 (count <= 13 values): [8] EXPOSED chain time -- how long this rank's update
 * stream sat idle in front of a panel (chunk) that had not arrived yet, summed over the fit; [9] the longest single such
 * wait; [10] the number of waits longer than 20 us; [11] rehearsal only: the modelled transfer time the fit enqueued;
 * [12] rehearsal only: the delays that stood for the remote owners' chains.
 * A hidden chain shows [8] ~ 0 whatever chain_panel / chain_bcast (kernel durations on the other streams) say. */
int gpx_mg_timing_ex(gpx_mg_t *mg, double *ms, int count);
/* ms[j] for j < count: what the owner's chain of panel j cost this rank in the last fit (factor + pack + the last chunk of
 * its column update), 0 for panels it does not own. */
int gpx_mg_chain_by_panel(gpx_mg_t *mg, double *ms, int64_t count);
/* raw device view of this rank's local matrix, (n + 1) x ld, block column j of the rank at column (j / world) nb (tests, the
 * rehearsal's check; do not free) */
int gpx_mg_device_ptrs(gpx_mg_t *mg, void **A, int64_t *ld);
/* Move the RCCL communicator of `from` (same world, rank and device; e.g. a handle of another block-column width) into `mg`,
 * which was made with gpx_mg_create_local and has none yet: ONE ncclCommInitRank per process however many layouts a run
 * tries.  `from` keeps working only as far as it needs no collective (world 1) and may be destroyed. */
int gpx_mg_adopt_comm(gpx_mg_t *mg, gpx_mg_t *from);
/* on != 0: the owner of the next panel factors it before it starts its own share of the trailing update (the panel is the
 * serial chain of the run; default: on for world >= 2, GPX_MG_OWNER_FIRST=0 / 1 overrides). */
int gpx_mg_set_owner_first(gpx_mg_t *mg, int on);
/* on != 0: also time how long the update stream waits in front of panels (chunks) that have not arrived -- values [8] .. [10]
 * of gpx_mg_timing_ex; costs two timing-enabled event records per wait on the stream that bounds the step, so it is OFF by
 * default (bench.py and the rehearsal turn it on; with it off those three values read 0). */
int gpx_mg_set_wait_timing(gpx_mg_t *mg, int on);
/* the schedule parameters IN EFFECT for the next fit (any pointer may be NULL): owner-first, row chunks per panel
 * broadcast, scatter + all-gather broadcast form, wait timing */
int gpx_mg_schedule_info(gpx_mg_t *mg, int *owner_first, int *chunks, int *sag, int *wait_timing);
/* Row chunks per panel broadcast for the following fits (1 .. 16; collective: the same on every rank). */
int gpx_mg_set_chunks(gpx_mg_t *mg, int chunks);
/* REHEARSAL: rank `rank` of a `world`-rank run in ONE process on one GPU, without a communicator.  The rank builds, factors,
 * packs and updates exactly its own block columns; a panel it does not own is copied (device to device) out of L_dev -- a
 * resident factor of the same matrix, (n + 1) x ldl with the right-hand side's row (gpx_gp_fit with the riding solve) --
 * behind a delay that stands for its owner's chain (this rank's own measurement for its nearest panel in the fit before);
 * every broadcast is followed by a delay that MODELS the transfer: bytes / link_GBps for one ring, 2 bytes / (world
 * link_GBps) for scatter + all-gather, + latency_us per collective.  alpha_dev: the solution (for the back substitution's
 * remote blocks).  Scalars of a rehearsal fit are this rank's share only.  Measured compute, modelled transfer. */
int gpx_mg_create_rehearsal(gpx_mg_t **out, int dtype, int kernel, int64_t n, int d, int64_t nb, int world, int rank,
                            const void *L_dev, int64_t ldl, const void *alpha_dev, double link_GBps, double latency_us);

/* ------------------------------------------ host-level drop-in entry points -- */
/* gaussian_c.K(out, x1, x2, h, w) -- gaussian_c.pyx:18 ; and the derivative
 * members through `member`.  out: (n, m) C-contiguous float64. */
int gpx_gaussian_c(int member, double *out, const double *x1, int64_t n,
                   const double *x2, int64_t m, double h, double w);
/* gaussian_c.jacobian(out[2,n,m], ...) :39 ; gaussian_c.hessian(out[2,2,n,m], ...) :44 */
int gpx_gaussian_c_jacobian(double *out, const double *x1, int64_t n,
                            const double *x2, int64_t m, double h, double w);
int gpx_gaussian_c_hessian(double *out, const double *x1, int64_t n,
                           const double *x2, int64_t m, double h, double w);
/* periodic_c.K(out, x1, x2, h, w, p) -- periodic_c.pyx:18 ; members as above */
int gpx_periodic_c(int member, double *out, const double *x1, int64_t n,
                   const double *x2, int64_t m, double h, double w, double p);
int gpx_periodic_c_jacobian(double *out, const double *x1, int64_t n,
                            const double *x2, int64_t m, double h, double w, double p);
int gpx_periodic_c_hessian(double *out, const double *x1, int64_t n,
                           const double *x2, int64_t m, double h, double w, double p);
/* (n, d) generalisation of the two above (BASELINE configs use d = 8/16/32).  OUT-OF-CORE: the matrix
 * is built on the device in row panels of GPX_KMAT_PANEL_BYTES (default 256 MiB) and streamed into
 * `out` with double buffering, so (n, m) may exceed HBM -- `out` can be a memory-mapped file. */
int gpx_kmat_host(int kernel, int member, double *out, const double *x1, int64_t n,
                  const double *x2, int64_t m, int d, const double *params,
                  double diag_add);

/* scipy.linalg.cholesky(A, lower=True) -- gp/gp.py:294.  A, L: (n, n) row-major
 * HOST float64 (may alias).  *info as LAPACK dpotrf. */
int gpx_cholesky(double *L, const double *A, int64_t n, int *info);
/* scipy.linalg.cho_solve((L, True), b) -- gp/gp.py:332-334.  b: (n,) in/out. */
int gpx_cho_solve(const double *L, int64_t n, double *b);
/* gp_c.log_lh(y, K, Kiy) -- gp_c.pyx:17-31.  Given L (not K): the logdet comes
 * from diag(L) instead of the reference's second LU factorisation of K. */
int gpx_gp_c_log_lh(const double *y, const double *L, const double *Kiy, int64_t n,
                    double *log_lh);
/* The derivative glue of gp/ext/gp_c.pyx for PLUGIN kernels, with the reference's own
 * arguments: every array HOST float64, C order; n = number of training points, np =
 * number of KERNEL parameters (outputs have np + 1 entries: the noise s is last);
 * Ki (n, n) = inv(Kxx), Kj (np, n, n) the kernel Jacobian, Kh (np, np, n, n) its
 * Hessian, Kiy (n,) = Ki y.  Every matrix crosses PCIe once; quadratic forms run as
 * matrix-vector work, traces of products as reductions, only the np products
 * dK_i Ki of the second-derivative trace terms as GEMMs (csrc/gpx_deriv.hip, "Glue").
 *   gpx_gp_c_dloglh_dtheta -- gp_c.pyx:34-49     dloglh (np + 1)
 *   gpx_gp_c_dlh_dtheta    -- gp_c.pyx:52-67     dlh    (np + 1)
 *   gpx_gp_c_d2lh_dtheta2  -- gp_c.pyx:70-111    d2lh   (np + 1, np + 1); dlh is an INPUT as there
 *   gpx_gp_c_dm_dtheta     -- gp_c.pyx:114-131   dm     (np + 1, m); Kjxo (np, m, n), Kxox (m, n) */
int gpx_gp_c_dloglh_dtheta(const double *y, const double *Ki, const double *Kj, const double *Kiy,
                           double s, int64_t n, int np, double *dloglh);
int gpx_gp_c_dlh_dtheta(const double *y, const double *Ki, const double *Kj, const double *Kiy,
                        double s, double lh, int64_t n, int np, double *dlh);
int gpx_gp_c_d2lh_dtheta2(const double *y, const double *Ki, const double *Kj, const double *Kh,
                          const double *Kiy, double s, double lh, const double *dlh, int64_t n,
                          int np, double *d2lh);
int gpx_gp_c_dm_dtheta(const double *y, const double *Ki, const double *Kj, const double *Kjxo,
                       const double *Kxox, double s, int64_t n, int np, int64_t m, double *dm);

/* C (M, N) = A (M, K) * B (N, K)^T, all HOST float64 C-contiguous: the np.dot
 * calls of the derivative glue (gp/ext/gp_c.pyx:43-48,61-66,89-110,127-131) on
 * the fp64 matrix cores. */
int gpx_gemm_nt_host(double *C, const double *A, const double *B, int64_t M, int64_t N,
                     int64_t K);

#ifdef __cplusplus
}
#endif
#endif /* GPX_H */
