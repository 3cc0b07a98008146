"""The matrix-core product (csrc/gpx_gemm.hip) alone, on every route, kernel instantiation and mode, both dtypes, through the
two debug entries gpx_debug_gemm_nt / gpx_debug_syrk_bc (the internal gemm_nt / syrk_bc with the arguments the public entries
hide: beta0, ktri, one- and two-dimensional batches, abort_flag).

Conventions of every case
  exact      A, B and C hold integers in [-4, 4] (drawn in float64, cast), alpha is one of 1, -1, 0.5, -0.25: every product and
             every partial sum is exactly representable in fp32 for K <= 2048 whatever the summation order (|sum| <= 16 K =
             2^15, in units of 1/4 that is 2^17 < 2^24), so the result does not depend on what the MFMA does inside.  The
             reference is an int64 product and the comparison is np.array_equal: a wrong k index, a dropped or doubled slice,
             a wrong row, column or batch mapping fails exactly.  test_exactness_is_a_property_of_the_inputs (CPU) checks the
             premise.  A failure names the first wrong (batch, i, j), got and want, and the tile and wave they fall in.
  not read   A and B carry input-NaN in columns K..ld, one guard row of it behind their last row and a gap of it between batch
             members: the fast kernel clamps rows to M - 1 / brows - 1 and reads exactly K columns, the generic one
             zero-fills, so a finite result has read none of it.
  not written  C carries output-NaN (the second payload) in columns N..ldc, in a guard row, between batch members and, under
             GPX_LOWER, in every element with row0 + i < col0 + j; all of it is compared bit for bit afterwards.  With beta0
             ALL of C starts as NaN and the M x N result must be finite and exact.
  route      every launch asserts its route counters (GEMM_FAST / GEMM_GENERIC / SYRK_EXACT / SYRK_PATCH) and, with
             gpx_prof_enable(1), the launch count of exactly one of GPX_PROF_GEMM, _GEMM_PANEL, _GEMM_SKINNY, _GEMM_N64,
             _GEMM_GENERIC -- the kernel instantiation -- the other four being zero.  Switches are environment variables set
             with monkeypatch.setenv; every entry point re-reads them.

epk = 16 (f64) / 32 (f32) elements are one k-slice (128 bytes of a row).

The only cases that round are test_gemm_alpha_rounding's: randn inputs, the reference built from the cast inputs (alpha cast
too) in longdouble, the bound of tests/test_gpu_blocks.py  4 (gamma_k(u_T) (|alpha| sum|a||b| + |c|) + u_T |ref|)  with
k = K + 2 -- the K products, C as one more term, and the rounding of alpha * acc in the atomic epilogue as another -- and
u_acc = u_T because the product accumulates in T.  Each runs twice and must give the same bits."""
import ctypes
import functools

import numpy as np
import pytest

from _block_helpers import DTYPES, LD, Worst, at, bits, nan_in, nan_out, round_up, same_bits
from gaussian_processes_amd import _lib
from gaussian_processes_amd.device import DeviceBuffer, sync

gpu = pytest.mark.gpu
BOTH = pytest.mark.parametrize("dtype", ["f64", "f32"])
WIDTHS = pytest.mark.parametrize("wide", [False, True], ids=["bn64", "bn128"])

EPK = {"f64": 16, "f32": 32}
CH = {"f64": 2, "f32": 4}                 # elements per 16 bytes
ALPHAS = (1.0, -1.0, 0.5, -0.25)
K_MAX = 1024                              # the largest depth of an exact case (gpx_debug_syrk_bc with kb = nb = 1024)
PROF = {"GEMM": 1, "SKINNY": 7, "GENERIC": 8, "PANEL": 9, "N64": 10}         # GPX_PROF_GEMM* of include/gpx.h
ROUTES = {"FAST": _lib.ROUTE_GEMM_FAST, "GENERIC": _lib.ROUTE_GEMM_GENERIC, "EXACT": _lib.ROUTE_SYRK_EXACT,
          "PATCH": _lib.ROUTE_SYRK_PATCH}


def ints(rng, shape, npdt):
    return rng.randint(-4, 5, size=shape, dtype=np.int8).astype(np.float64).astype(npdt)


# ---- the premise of the exact comparison, on the CPU ---------------------------------------------------------------------
def _pairwise(t):
    t = t.copy()
    while t.shape[-1] > 1:
        if t.shape[-1] % 2:
            t = np.concatenate([t[..., :-2], t[..., -2:-1] + t[..., -1:]], axis=-1)
        t = t[..., 0::2] + t[..., 1::2]
    return t[..., 0]


@pytest.mark.parametrize("K", [K_MAX, 2048])
def test_exactness_is_a_property_of_the_inputs(K):
    """float32 sums of the generator's products -- forward, reversed, pairwise -- times every alpha, plus C, equal int64."""
    rng = np.random.RandomState(7)
    a, b, c = ints(rng, (64, K), np.float32), ints(rng, (64, K), np.float32), ints(rng, 64, np.float32)
    a[0], b[0] = 4, -4                                                  # the extreme sums
    a[1], b[1] = -4, -4
    prod = a * b
    assert prod.dtype == np.float32
    want = (a.astype(np.int64) * b.astype(np.int64)).sum(1)
    sums = {"forward": np.cumsum(prod, axis=1, dtype=np.float32)[:, -1],
            "reversed": np.cumsum(prod[:, ::-1], axis=1, dtype=np.float32)[:, -1],
            "pairwise": _pairwise(prod)}
    for name, s in sums.items():
        assert s.dtype == np.float32
        assert np.array_equal(s.astype(np.float64), want.astype(np.float64)), name
        for alpha in ALPHAS:
            got = c + np.float32(alpha) * s                             # float32 arithmetic throughout
            assert got.dtype == np.float32
            assert np.array_equal(got.astype(np.float64), c.astype(np.float64) + alpha * want), (name, alpha)


# ---- one observed launch ------------------------------------------------------------------------------------------------
def observed(call):
    """call() between a reset and a read of the route counters and of the product kernels' launch counts."""
    lib = _lib.load()
    _lib.route_reset()
    _lib.check(lib.gpx_prof_enable(1))
    try:
        rc = call()
        sync()
        routes = {k: _lib.route_count(v) for k, v in ROUTES.items()}
        launches = {}
        for name, cls in PROF.items():
            n = ctypes.c_double(0.0)
            _lib.check(lib.gpx_prof_read(cls, ctypes.byref(n), None, None))
            launches[name] = int(n.value)
    finally:
        lib.gpx_prof_enable(0)
    return rc, routes, launches


def assert_ran_on(routes, launches, route, cls, what, count=1):
    want_r, want_l = dict.fromkeys(ROUTES, 0), dict.fromkeys(PROF, 0)
    if route:
        want_r.update(route if isinstance(route, dict) else {route: count})
    if cls:
        want_l[cls] = count
    assert routes == want_r, "%s: routes %r, expected %r" % (what, routes, want_r)
    assert launches == want_l, "%s: kernel launches %r, expected %r" % (what, launches, want_l)


def first_wrong(got, want, bad, i0, j0, batch, cls, what):
    i, j = np.argwhere(bad)[0]
    gi, gj = int(i) + i0, int(j) + j0
    bn = 64 if cls in ("SKINNY", "N64") else 128
    return ("%s: first wrong element (batch, i, j) = (%s, %d, %d): got %r, want %r; tile (%d, %d) of 128 x %d, wave %d"
            % (what, batch, gi, gj, got[i, j], want[i, j], gi // 128, gj // bn, bn,
               2 * ((gi % 128) // 64) + (gj % bn) // (bn // 2)))


def member(flat, off, rows, ld):
    return flat[off:off + rows * ld].reshape(rows, ld)


def debug_gemm(did, M, N, K, alpha, A, lda, B, ldb, C, ldc, tri=_lib.FULL, row0=0, col0=0, beta0=0, ktri=0, count=1,
               strides=(0, 0, 0), count2=1, strides2=(0, 0, 0)):
    return _lib.load().gpx_debug_gemm_nt(did, M, N, K, alpha, A, lda, B, ldb, C, ldc, tri, row0, col0, beta0, ktri, count,
                                         strides[0], strides[1], strides[2], count2, strides2[0], strides2[1], strides2[2],
                                         None)


def gemm_case(dtype, M, N, K, route, cls, alpha=1.0, tri=_lib.FULL, row0=0, col0=0, beta0=0, ktri=0, count=1, count2=1,
              ldc=None, c_off=0, upper=False, seed=0, rc_want=_lib.OK):
    """One product with everything the conventions ask for.  upper: A == B (one buffer), upper triangular in (row, k).
    rc_want != OK: the call must refuse with that code, count no kernel launch and leave every bit of C."""
    did, npdt, _, _ = DTYPES[dtype]
    es, ch = np.dtype(npdt).itemsize, CH[dtype]
    rng = np.random.RandomState(1000 * seed + M + 3 * N + 7 * K)
    lda, ldb = round_up(K, ch) + ch, round_up(K, ch) + 2 * ch
    ldc = N + 2 if ldc is None else ldc
    even = 1 if beta0 else 0                                            # the vector epilogue wants every member 2-aligned
    sA, sB = (M + 1) * lda + 2 * ch, (N + 1) * ldb + 5 * ch            # ragged and distinct, 16-byte multiples
    sC = (M + 1) * ldc + 7
    sC += even * (sC % 2)
    tA, tB, tC = count * sA + 4 * ch, count * sB + ch, count * sC + 11
    tC += even * (tC % 2)
    if upper:
        assert M == N and count * count2 == 1
        ldb = lda
    A = np.full(count2 * tA, nan_in(npdt), dtype=npdt)
    B = A if upper else np.full(count2 * tB, nan_in(npdt), dtype=npdt)
    C0 = np.full(c_off + count2 * tC, nan_out(npdt), dtype=npdt)
    allowed = np.zeros(C0.size, dtype=bool)                             # what the launch may write
    i, j = np.arange(M)[:, None], np.arange(N)[None, :]
    lower = (row0 + i >= col0 + j) if tri == _lib.LOWER else np.ones((M, N), dtype=bool)
    members = [(y, z) for z in range(count2) for y in range(count)]
    for y, z in members:
        a = ints(rng, (M, K), npdt)
        member(A, y * sA + z * tA, M, lda)[:, :K] = np.triu(a) if upper else a
        if not upper:
            member(B, y * sB + z * tB, N, ldb)[:, :K] = ints(rng, (N, K), npdt)
        c = member(C0, c_off + y * sC + z * tC, M, ldc)
        if not beta0:
            c[:, :N][lower] = ints(rng, (M, N), npdt)[lower]
        member(allowed, c_off + y * sC + z * tC, M, ldc)[:, :N] = lower
    dA = DeviceBuffer.from_host(A)
    dB = dA if upper else DeviceBuffer.from_host(B)
    dC = DeviceBuffer.from_host(C0)
    what = "%s M = %d N = %d K = %d alpha = %g tri = %d (%d, %d) beta0 = %d ktri = %d batch %d x %d ldc = %d c_off = %d" % (
        dtype, M, N, K, alpha, tri, row0, col0, beta0, ktri, count, count2, ldc, c_off)
    rc, routes, launches = observed(lambda: debug_gemm(did, M, N, K, alpha, dA.ptr, lda, dB.ptr, ldb, at(dC, c_off, es), ldc,
                                                       tri, row0, col0, beta0, ktri, count, (sA, sB, sC), count2,
                                                       (tA, tB, tC)))
    assert rc == rc_want, "%s: status %d (%s), expected %d" % (what, rc, _lib.last_error(), rc_want)
    got = dC.to_host()
    if rc_want != _lib.OK:
        assert_ran_on(routes, launches, route, None, what)
        assert same_bits(got, C0), what + ": a refused call wrote to C"
        return
    assert_ran_on(routes, launches, route, cls, what)
    assert same_bits(dA.to_host(), A) and (upper or same_bits(dB.to_host(), B)), what + ": an input changed"
    changed = bits(got) != bits(C0)
    assert not (changed & ~allowed).any(), "%s: wrote outside the result (first at flat element %d)" % (
        what, int(np.flatnonzero(changed & ~allowed)[0]) - c_off)
    for y, z in members:
        a = member(A, y * sA + z * tA, M, lda)[:, :K].astype(np.int64)
        b = member(B, y * sB + z * tB, N, ldb)[:, :K].astype(np.int64)
        g, c = member(got, c_off + y * sC + z * tC, M, ldc)[:, :N], member(C0, c_off + y * sC + z * tC, M, ldc)[:, :N]
        for j0 in range(0, N, 1024):                                    # column blocks: the int64 product only where it counts
            j1 = min(N, j0 + 1024)
            i0 = int(np.argmax(lower[:, j0:j1].any(1))) if lower[:, j0:j1].any() else M
            if i0 == M:
                continue
            low = lower[i0:, j0:j1]
            want = alpha * (a[i0:] @ b[j0:j1].T).astype(np.float64)
            if not beta0:
                want = want + np.where(low, c[i0:, j0:j1], 0).astype(np.float64)
            gb = g[i0:, j0:j1]
            assert np.isfinite(gb[low]).all(), "%s: member (%d, %d) is not finite (something NaN was read, or not written)" % (
                what, y, z)
            bad = low & (gb.astype(np.float64) != want)
            assert not bad.any(), first_wrong(gb, want, bad, i0, j0, (y, z), cls, what)


def narrow(monkeypatch, wide):
    """wide: 128 x 128 tiles for every FULL product wider than 64 columns (class PANEL); else the default, 128 x 64 tiles for
    products of up to 256 tiles (class SKINNY) -- every FULL shape of this file."""
    if wide:
        monkeypatch.setenv("GPX_GEMM_BN64_TILES", "0")
    else:
        monkeypatch.delenv("GPX_GEMM_BN64_TILES", raising=False)


def full_class(N, wide):
    return "PANEL" if wide and N > 64 else "SKINNY"


# ---- k-pipeline ------------------------------------------------------------------------------------------------------------
@gpu
@BOTH
@WIDTHS
def test_gemm_k_pipeline_fast(dtype, wide, monkeypatch):
    """One to five k-slices: the prologue has two stages in flight and re-fetches the last slice when K is shorter."""
    narrow(monkeypatch, wide)
    for M, N in ((129, 65), (257, 130)):
        for slices in (1, 2, 3, 4, 5):
            gemm_case(dtype, M, N, slices * EPK[dtype], "FAST", full_class(N, wide), alpha=ALPHAS[slices % 4], seed=slices)


@gpu
@BOTH
def test_gemm_k_pipeline_generic(dtype, monkeypatch):
    epk = EPK[dtype]
    for M, N in ((129, 65), (257, 130)):
        for n, K in enumerate((1, epk - 1, epk + 1, 3 * epk + 5)):
            gemm_case(dtype, M, N, K, "GENERIC", "GENERIC", alpha=ALPHAS[n], seed=n)
    monkeypatch.setenv("GPX_GEMM_NO_FAST", "1")
    gemm_case(dtype, 257, 130, 2 * epk, "GENERIC", "GENERIC", alpha=-0.25)
    gemm_case(dtype, 257, 130, 2 * epk, "GENERIC", "GENERIC", alpha=0.5, tri=_lib.LOWER, row0=3, col0=40)


# ---- tile edges ------------------------------------------------------------------------------------------------------------
@gpu
@BOTH
@WIDTHS
def test_gemm_tile_edges_full(dtype, wide, monkeypatch):
    narrow(monkeypatch, wide)
    K, n = 2 * EPK[dtype], 0
    for M in (1, 63, 64, 65, 127, 128, 129):
        for N in (1, 2, 63, 64, 65, 129):
            n += 1
            gemm_case(dtype, M, N, K, "FAST", full_class(N, wide), alpha=ALPHAS[n % 4], seed=n)
        gemm_case(dtype, M, 1, K, "FAST", "SKINNY", alpha=-1.0, ldc=1)                  # every predictive mean
        gemm_case(dtype, M, 65, K, "FAST", full_class(65, wide), alpha=0.5, ldc=67)     # N odd, ldc odd
        gemm_case(dtype, M, 64, K, "FAST", "SKINNY", alpha=-0.25, ldc=67)               # N even, ldc odd
    gemm_case(dtype, 129, 130, K, "FAST", full_class(130, wide), alpha=-1.0, c_off=1)  # C's base one element off


@gpu
@BOTH
@WIDTHS
def test_gemm_narrow_patches(dtype, wide, monkeypatch):
    """csh: patches of fewer than 8 tile columns, so that no workgroup is launched for a tile outside a narrow product."""
    narrow(monkeypatch, wide)
    for n, N in enumerate((128, 129, 256, 257, 512, 513)):
        gemm_case(dtype, 1025, N, EPK[dtype], "FAST", full_class(N, wide), alpha=ALPHAS[n % 4], seed=n)


# ---- LOWER on 128 x 128 tiles: one patch column, the staircase, the diagonal split ---------------------------------------------
LOWER_CASES = [(520, 520, 0, 0), (1300, 1024, 0, 0),                     # N <= 1024: a = 0
               (1152, 1152, 0, 0), (2100, 2100, 0, 0),                   # staircase + diagonal split, 2 and 3 diagonal patches
               (2200, 1100, 0, 1024), (2200, 1100, 0, 1030),             # a split with b = 1; no split
               (2200, 1100, 40, 10), (2200, 1100, 10, 40)]               # the triangle shifted either way


@gpu
@BOTH
@pytest.mark.parametrize("M,N,row0,col0", LOWER_CASES)
def test_gemm_lower(dtype, M, N, row0, col0):
    gemm_case(dtype, M, N, EPK[dtype], "FAST", "PANEL", alpha=ALPHAS[(M + col0) % 4], tri=_lib.LOWER, row0=row0, col0=col0)


@gpu
def test_gemm_lower_8320_f32():
    """More than 8 diagonal patches: the diagonal split's decode wraps (dp = (loc2 / 36) * 8 + (b2 & 7)).  The largest case of
    the file, about 280 MB of C."""
    gemm_case("f32", 8320, 8320, 32, "FAST", "PANEL", alpha=-1.0, tri=_lib.LOWER)


# ---- alpha and rounding: the only cases that are not exact -------------------------------------------------------------------
@gpu
@BOTH
@pytest.mark.parametrize("route", ["FAST-bn64", "FAST-bn128", "GENERIC"])
def test_gemm_alpha_rounding(dtype, route, monkeypatch):
    did, npdt, _, ut = DTYPES[dtype]
    epk, ch = EPK[dtype], CH[dtype]
    narrow(monkeypatch, route == "FAST-bn128")
    M, N, K = (130, 70, 3 * epk + 5) if route == "GENERIC" else (257, 300, 4 * epk)
    cls = "GENERIC" if route == "GENERIC" else full_class(N, route == "FAST-bn128")
    rng, worst = np.random.RandomState(77), Worst("gemm_nt %s" % route, dtype)
    lda, ldc = round_up(K, ch) + ch, N + 3
    A, B = np.full((M + 1, lda), nan_in(npdt), dtype=npdt), np.full((N + 1, lda), nan_in(npdt), dtype=npdt)
    C0 = np.full((M + 1, ldc), nan_out(npdt), dtype=npdt)
    A[:M, :K], B[:N, :K], C0[:M, :N] = rng.randn(M, K), rng.randn(N, K), rng.randn(M, N)
    dA, dB = DeviceBuffer.from_host(A), DeviceBuffer.from_host(B)
    prod, mag = np.zeros((M, N), dtype=LD), np.zeros((M, N), dtype=LD)
    for k in range(K):
        t = np.outer(A[:M, k].astype(LD), B[:N, k].astype(LD))
        prod += t
        mag += np.abs(t)
    for alpha in (-1.0, 0.37, -1.0 / 1.3 ** 4):
        al = LD(npdt(alpha))                                            # the kernel multiplies by alpha cast to T
        got = []
        for _ in range(2):
            dC = DeviceBuffer.from_host(C0)
            what = "%s M = %d N = %d K = %d alpha = %g" % (route, M, N, K, alpha)
            rc, routes, launches = observed(lambda: debug_gemm(did, M, N, K, alpha, dA.ptr, lda, dB.ptr, lda, dC.ptr, ldc))
            assert rc == _lib.OK, what
            assert_ran_on(routes, launches, route.split("-")[0], cls, what)
            got.append(dC.to_host())
        assert same_bits(got[0], got[1]), what + ": two runs differ"
        assert same_bits(got[0][:, N:], C0[:, N:]) and same_bits(got[0][M], C0[M]), what + ": padding / guard row of C"
        c = C0[:M, :N].astype(LD)
        worst.check(got[0][:M, :N], c + al * prod, np.abs(al) * mag + np.abs(c), K + 2, ut, what, u_acc=ut)
    worst.report()


# ---- beta0 -----------------------------------------------------------------------------------------------------------------
@gpu
@BOTH
@WIDTHS
def test_gemm_beta0(dtype, wide, monkeypatch):
    """C = alpha A B^T, C never read: N even with an even ldc and an aligned base is the 2-element vector epilogue, anything
    else the scalar one."""
    narrow(monkeypatch, wide)
    K = 2 * EPK[dtype]
    for n, (M, N, ldc, c_off) in enumerate(((129, 130, 132, 0), (129, 131, 132, 0), (257, 64, 64, 0), (200, 63, 64, 0),
                                            (129, 130, 131, 0), (129, 130, 132, 1), (65, 2, 2, 0), (300, 258, 260, 0))):
        gemm_case(dtype, M, N, K, "FAST", full_class(N, wide), alpha=ALPHAS[n % 4], beta0=1, ldc=ldc, c_off=c_off, seed=n)
    for count, count2 in ((3, 1), (2, 2)):
        gemm_case(dtype, 129, 130, K, "FAST", full_class(130, wide), alpha=-0.25, beta0=1, ldc=132, count=count, count2=count2)


@gpu
@BOTH
def test_gemm_beta0_refusals(dtype):
    """beta = 0 on the generic kernel (K tail) and with tri = GPX_LOWER: GPX_ERR_UNSUPPORTED, C keeps every bit.  (LOWER: in
    the vector epilogue a lane pair that straddles the diagonal would store 0, not C, into the first strictly upper element.)"""
    epk = EPK[dtype]
    gemm_case(dtype, 130, 70, epk + 3, "GENERIC", None, beta0=1, rc_want=_lib.ERR_UNSUPPORTED)
    assert "beta = 0" in _lib.last_error()
    for M, N in ((130, 130), (300, 64)):
        gemm_case(dtype, M, N, epk, None, None, beta0=1, tri=_lib.LOWER, rc_want=_lib.ERR_UNSUPPORTED)
        assert "GPX_FULL" in _lib.last_error()
    gemm_case(dtype, 130, 130, epk + 3, None, None, beta0=1, tri=_lib.LOWER, rc_want=_lib.ERR_UNSUPPORTED)


# ---- in place: C == A ------------------------------------------------------------------------------------------------------
@gpu
@BOTH
@pytest.mark.parametrize("count", [1, 3])
def test_gemm_in_place(dtype, count):
    """X <- X B^T on the rows below a factored 64 x 64 block (gpx_potrf.hip, the panel's X inv(L_jj)^T): C == A, beta0,
    N = K = 64; each tile has read all 64 columns of its own rows before it stores them and no other tile touches those rows.
    Columns 64..320 of the rows are other data.  Batch: the strides of that call -- matrices sM apart, blocks 64 * 64."""
    did, npdt, _, _ = DTYPES[dtype]
    M, ld, rng = 300, 320, np.random.RandomState(5)
    sM = (M + 1) * ld + 8
    X0 = np.full(count * sM, nan_in(npdt), dtype=npdt)
    Bs = ints(rng, (count, 64, 64), npdt)
    for y in range(count):
        member(X0, y * sM, M, ld)[:] = ints(rng, (M, ld), npdt)
    dX, dB = DeviceBuffer.from_host(X0), DeviceBuffer.from_host(Bs)
    what = "%s in place, batch of %d" % (dtype, count)
    rc, routes, launches = observed(lambda: debug_gemm(did, M, 64, 64, 1.0, dX.ptr, ld, dB.ptr, 64, dX.ptr, ld, beta0=1,
                                                       count=count, strides=(sM, 64 * 64, sM)))
    assert rc == _lib.OK, what
    assert_ran_on(routes, launches, "FAST", "SKINNY", what)
    got = dX.to_host()
    assert same_bits(dB.to_host(), Bs), what + ": B changed"
    for y in range(count):
        g, x = member(got, y * sM, M + 1, ld), member(X0, y * sM, M + 1, ld)
        assert same_bits(g[:, 64:], x[:, 64:]) and same_bits(g[M], x[M]), "%s: member %d: columns 64.. / the guard row" % (what, y)
        want = (x[:M, :64].astype(np.int64) @ Bs[y].astype(np.int64).T).astype(np.float64)
        bad = g[:M, :64].astype(np.float64) != want
        assert not bad.any(), first_wrong(g[:M, :64], want, bad, 0, 0, y, "SKINNY", what)
    assert same_bits(got[count * sM - 8:], X0[count * sM - 8:]), what + ": the gap"


# ---- ktri ------------------------------------------------------------------------------------------------------------------
@gpu
@BOTH
@pytest.mark.parametrize("tri", [_lib.FULL, _lib.LOWER], ids=["full", "lower"])
def test_gemm_ktri(dtype, tri):
    """A == B upper triangular in (row, k), M == N == K: tile row bm0 starts its k-loop at bm0.  The reference is the full
    product.  128: one tile row, nothing skipped; 384: three; 8 epk + 72 rounded up to a slice (208 / 352): a last tile row
    that ends inside its tile.  K = 100 is no whole slice: the generic kernel, ktri ignored."""
    epk = EPK[dtype]
    for n, size in enumerate((128, 384, round_up(8 * epk + 72, epk))):
        gemm_case(dtype, size, size, size, "FAST", "PANEL", alpha=ALPHAS[n], tri=tri, ktri=1, upper=True, seed=n)
    gemm_case(dtype, 100, 100, 100, "GENERIC", "GENERIC", alpha=-1.0, tri=tri, ktri=1, upper=True)


# ---- batches ---------------------------------------------------------------------------------------------------------------
@gpu
@BOTH
@WIDTHS
def test_gemm_batches_fast(dtype, wide, monkeypatch):
    """blockIdx.y / z pick the member and rotate the tile-to-workgroup map, (bid - y - 3 z) & 7: with ragged, distinct strides
    a swapped stride or a mis-rotated map lands in a NaN gap or in the wrong member."""
    narrow(monkeypatch, wide)
    M, N, K = 200, 130, 2 * EPK[dtype]
    cls = full_class(N, wide)
    for n, (count, count2) in enumerate(((2, 1), (9, 1), (3, 3), (9, 4))):
        gemm_case(dtype, M, N, K, "FAST", cls, alpha=ALPHAS[n], count=count, count2=count2, seed=n)
    gemm_case(dtype, M, N, K, "FAST", "PANEL", alpha=-1.0, tri=_lib.LOWER, row0=5, col0=2, count=9, count2=4)


@gpu
@BOTH
def test_gemm_batches_generic(dtype):
    M, N, K = 200, 130, 2 * EPK[dtype] + 3
    for n, count in enumerate((2, 9)):
        gemm_case(dtype, M, N, K, "GENERIC", "GENERIC", alpha=ALPHAS[n + 1], count=count, seed=n)
    gemm_case(dtype, M, N, K, "GENERIC", "GENERIC", alpha=0.5, tri=_lib.LOWER, row0=1, col0=30, count=9)
    gemm_case(dtype, M, N, K, "GENERIC", None, count=3, count2=3, rc_want=_lib.ERR_UNSUPPORTED)
    assert "two-dimensional" in _lib.last_error()


# ---- gpx_debug_syrk_bc -------------------------------------------------------------------------------------------------------
def debug_syrk(did, n, row_begin, C, ldc, cl0, cl1, Pb, ldp, k0, kb, nb, P=1, rank=0, abort=None, count=1, sP=0, sC=0):
    return _lib.load().gpx_debug_syrk_bc(did, n, row_begin, C, ldc, cl0, cl1, Pb, ldp, k0, kb, nb, P, rank, abort, count, sP, sC,
                                         None)


def syrk_widths(monkeypatch, wide):
    """wide: 128-wide tiles on the exact route (class GEMM); else the default for these sizes, 64-wide (class N64).  The patch
    route only has 128-wide tiles."""
    if wide:
        monkeypatch.setenv("GPX_SYRK_BN64_TILES", "0")
    else:
        monkeypatch.delenv("GPX_SYRK_BN64_TILES", raising=False)


@functools.lru_cache(maxsize=32)
def panel_ints(n, k0, kb):
    """The panel of one (n, k0, kb), shared by both dtypes, tile widths and routes: rows k0..n, float64 integers."""
    return ints(np.random.RandomState(n + 3 * k0 + kb), (n - k0, kb), np.float64)


@functools.lru_cache(maxsize=32)
def panel_gram(n, k0, kb, c0):
    """int64 P[kb:] P[c0:]^T of that panel where (panel) row >= column, kept as int32; column blocks of 256."""
    p = panel_ints(n, k0, kb).astype(np.int64)
    rows, cols = p.shape[0] - kb, p.shape[0] - c0
    out = np.zeros((max(rows, 0), max(cols, 0)), dtype=np.int32)
    for j0 in range(0, cols, 256):
        j1 = min(cols, j0 + 256)
        i0 = max(0, c0 + j0 - kb)                                       # first row at or below the block's first column
        if i0 < rows:
            out[i0:, j0:j1] = p[kb + i0:] @ p[c0 + j0:c0 + j1].T
    return out


@functools.lru_cache(maxsize=2)
def syrk_c0(n, dtype):
    """n x n with NaN above the diagonal, in the pitch and in a guard row; integers on and below it.  Host and device copy."""
    npdt = DTYPES[dtype][1]
    ldc = n + 3
    C0 = np.full((n + 1, ldc), nan_out(npdt), dtype=npdt)
    low = np.tril_indices(n)
    C0[:n, :n][low] = ints(np.random.RandomState(n), low[0].size, npdt)
    return C0, DeviceBuffer.from_host(C0)


SYRK_VARIANTS = ["exact", "plus64", "noexact", "coarse"]


@gpu
@BOTH
@WIDTHS
@pytest.mark.parametrize("variant", SYRK_VARIANTS)
@pytest.mark.parametrize("n", [1280, 2560, 3100])
def test_syrk_bc_single_rank(n, variant, wide, dtype, monkeypatch):
    """P = 1, nb x kb x k: row_begin = k0 + kb with kb = nb is the factorisation's update, triangle aligned to the tiles: the
    exact enumeration (its band search, 64- or 128-wide tiles; `coarse`: chunks of 64 tiles where there are that many).
    `plus64` (row_begin 64 further down) and `noexact` (GPX_GEMM_EXACT=0) take the patch staircase instead, and so does every
    kb < nb here: columns start at k0 then (the fast kernel wants them at a multiple of 128) and row_begin - k0 = kb is no
    multiple of 128.  (`noexact` and `coarse` skip those: they would repeat `exact` launch for launch.)  n = 3100 has a ragged
    last block column; k = 2 with nb = 1024 lies beyond n = 1280: nothing to do, nothing launched."""
    did, npdt, _, _ = DTYPES[dtype]
    es, epk, ch = np.dtype(npdt).itemsize, EPK[dtype], CH[dtype]
    syrk_widths(monkeypatch, wide)
    if variant == "noexact":
        monkeypatch.setenv("GPX_GEMM_EXACT", "0")
    if variant == "coarse":
        monkeypatch.setenv("GPX_GEMM_FINE_TILES", "0")
    lib = _lib.load()
    C0, dC0 = syrk_c0(n, dtype)
    ldc = C0.shape[1]
    dC = DeviceBuffer(C0.shape, npdt)
    for nb in (128, 256, 512, 1024):
        for kb in (epk, 3 * epk, nb):
            for k in (0, 2):
                aligned = kb % 128 == 0
                if variant in ("noexact", "coarse") and not aligned:
                    continue
                k0 = k * nb
                row_begin = k0 + kb + (64 if variant == "plus64" else 0)
                cl0 = k0 + kb if aligned else k0
                what = "%s n = %d nb = %d kb = %d k0 = %d row_begin = %d cl0 = %d %s" % (dtype, n, nb, kb, k0, row_begin, cl0,
                                                                                          variant)
                rows, cols = n - row_begin, n - cl0
                ldp = kb + ch
                if k0 < n:
                    Pb = np.full((n - k0 + 1, ldp), nan_in(npdt), dtype=npdt)
                    Pb[:n - k0, :kb] = panel_ints(n, k0, kb)
                else:
                    Pb = np.full((1, ldp), nan_in(npdt), dtype=npdt)
                dP = DeviceBuffer.from_host(Pb)
                _lib.check(lib.gpx_memcpy_d2d(dC.ptr, dC0.ptr, dC.nbytes, None))
                rc, routes, launches = observed(lambda: debug_syrk(did, n, row_begin, dC.ptr, ldc, cl0, max(n, cl0), dP.ptr, ldp,
                                                                   k0, kb, nb))
                assert rc == _lib.OK, what + ": " + _lib.last_error()
                got = dC.to_host()
                if rows <= 0 or cols <= 0:
                    assert_ran_on(routes, launches, None, None, what)
                    assert same_bits(got, C0), what + ": nothing to update, yet C changed"
                    continue
                exact = aligned and variant in ("exact", "coarse")
                assert_ran_on(routes, launches, "EXACT" if exact else "PATCH", "N64" if exact and not wide else "GEMM", what)
                assert same_bits(dP.to_host(), Pb), what + ": the panel changed"
                changed = bits(got) != bits(C0)
                g = np.arange(row_begin, n)[:, None] >= np.arange(cl0, n)[None, :]      # global row >= global column
                assert not changed[:row_begin].any() and not changed[n:].any(), what + ": wrote above row_begin / in the guard row"
                assert not changed[row_begin:n, :cl0].any() and not changed[row_begin:n, n:].any(), what + ": wrote beside its columns"
                assert not (changed[row_begin:n, cl0:n] & ~g).any(), what + ": wrote above the diagonal"
                gram = panel_gram(n, k0, kb, cl0 - k0)[row_begin - k0 - kb:]
                sub, c = got[row_begin:n, cl0:n], C0[row_begin:n, cl0:n]
                assert np.isfinite(sub[g]).all(), what + ": not finite (something NaN was read)"
                want = np.where(g, c, 0).astype(np.float64) - gram
                bad = g & (sub.astype(np.float64) != want)
                assert not bad.any(), first_wrong(sub, want, bad, 0, 0, 0, "N64" if exact and not wide else "GEMM",
                                                  what + " (indices from (row_begin, cl0))")


@gpu
@BOTH
@WIDTHS
def test_syrk_bc_coarse_chunks_128(dtype, wide, monkeypatch):
    """GPX_GEMM_FINE_TILES=0 only gives chunks of 64 tiles (ecl = 6) to a launch of at least 512 tiles; 128-wide tiles need
    32 tile rows for that: n = 4224, nb = kb = 128 is 528 tiles (1056 of the 64-wide ones)."""
    syrk_widths(monkeypatch, wide)
    monkeypatch.setenv("GPX_GEMM_FINE_TILES", "0")
    syrk_general(dtype, 4224, 128, 128, 0, 1, wide, "EXACT")


def syrk_general(dtype, n, nb, kb, k, P, wide, route, plus=0, count=1, abort=None):
    """Every rank of P, a batch of `count`, abort flags: the block-cyclic layout of tests/test_gpu_parity.py's
    test_syrk_bc_block_cyclic_vs_numpy (local block jl is global block jl * P + rank; the last one may be ragged)."""
    did, npdt, _, _ = DTYPES[dtype]
    es, ch = np.dtype(npdt).itemsize, CH[dtype]
    rng = np.random.RandomState(n + P + kb)
    k0 = k * nb
    row_begin = k0 + nb + plus
    ldp, nblk = kb + ch, -(-n // nb)
    sP = (n - k0 + 1) * ldp + 3 * ch
    panels = np.full(count * sP, nan_in(npdt), dtype=npdt)
    for y in range(count):
        member(panels, y * sP, n - k0, ldp)[:, :kb] = ints(rng, (n - k0, kb), npdt)
    dP = DeviceBuffer.from_host(panels)
    dflag = None if abort is None else DeviceBuffer.from_host(np.asarray(abort, dtype=np.int32))
    cls = "N64" if route == "EXACT" and not wide else "GEMM"
    for rank in range(P):
        gblocks = [j for j in range(nblk) if j % P == rank]
        first = next((jl for jl, j in enumerate(gblocks) if j > k), None)
        if first is None:
            continue
        ncl = len(gblocks) * nb
        ldc, cl0 = ncl + 5, first * nb
        gcol = np.concatenate([j * nb + np.arange(nb) for j in gblocks])
        sC = (n + 1) * ldc + 9
        lower = np.arange(n)[:, None] >= gcol[None, :]                  # also false in the padding columns beyond n
        written = lower & (np.arange(n)[:, None] >= row_begin) & (np.arange(ncl)[None, :] >= cl0)
        C0 = np.full(count * sC, nan_out(npdt), dtype=npdt)
        for y in range(count):
            member(C0, y * sC, n, ldc)[:, :ncl][lower] = ints(rng, int(lower.sum()), npdt)
        dC = DeviceBuffer.from_host(C0)
        what = "%s n = %d nb = %d kb = %d k0 = %d row_begin = %d P = %d rank = %d batch %d abort %r" % (
            dtype, n, nb, kb, k0, row_begin, P, rank, count, abort)
        rc, routes, launches = observed(lambda: debug_syrk(did, n, row_begin, dC.ptr, ldc, cl0, ncl, dP.ptr, ldp, k0, kb, nb, P,
                                                           rank, None if dflag is None else dflag.ptr, count, sP, sC))
        assert rc == _lib.OK, what + ": " + _lib.last_error()
        assert_ran_on(routes, launches, route, cls, what)
        got = dC.to_host()
        assert same_bits(dP.to_host(), panels), what + ": the panel changed"
        changed = bits(got) != bits(C0)
        for y in range(count):
            ch_y = member(changed, y * sC, n + 1, ldc)
            if abort is not None and abort[y]:
                assert not ch_y.any(), what + ": member %d was aborted, yet it changed" % y
                continue
            assert not ch_y[n].any() and not ch_y[:n, ncl:].any() and not (ch_y[:n, :ncl] & ~written).any(), (
                "%s: member %d: wrote outside the update" % (what, y))
            p = member(panels, y * sP, n - k0, ldp)[:, :kb].astype(np.int64)
            g, c = member(got, y * sC, n, ldc)[:, :ncl], member(C0, y * sC, n, ldc)[:, :ncl]
            assert np.isfinite(g[written]).all(), what + ": member %d is not finite (something NaN was read)" % y
            inside = gcol < n
            gram = np.zeros((n - row_begin, ncl), dtype=np.int64)
            gram[:, inside] = p[row_begin - k0:] @ p[np.maximum(gcol[inside] - k0, 0)].T
            want = np.where(written, c, 0).astype(np.float64)[row_begin:] - gram
            bad = written[row_begin:] & (g[row_begin:].astype(np.float64) != want)
            assert not bad.any(), first_wrong(g[row_begin:], want, bad, 0, 0, y, cls, what + " (rows from row_begin, local columns)")
            assert not changed[y * sC + (n + 1) * ldc:(y + 1) * sC].any(), what + ": the gap behind member %d" % y


@gpu
@BOTH
@WIDTHS
@pytest.mark.parametrize("n,nb,P,k", [(1280, 128, 2, 0), (2000, 256, 3, 1), (3100, 512, 2, 0), (3100, 128, 3, 5)])
def test_syrk_bc_block_cyclic(dtype, wide, n, nb, P, k, monkeypatch):
    """P = 2, 3, every rank: the column shift cshift = ((cbase + bn0) / nb) (P - 1) nb of the patch map and etpb / epm1t of the
    exact one; n = 3100 leaves a ragged last block column whose padding columns lie beyond the matrix."""
    syrk_widths(monkeypatch, wide)
    syrk_general(dtype, n, nb, 2 * EPK[dtype], k, P, wide, "EXACT")
    syrk_general(dtype, n, nb, 2 * EPK[dtype], k, P, wide, "PATCH", plus=64)


@gpu
@BOTH
@WIDTHS
@pytest.mark.parametrize("route,plus", [("EXACT", 0), ("PATCH", 64)])
def test_syrk_bc_batch_and_abort(dtype, wide, route, plus, monkeypatch):
    """A lock-step batch of 3; with abort_flag = {0, 7, 0} member 1 keeps every bit, members 0 and 2 are exact."""
    syrk_widths(monkeypatch, wide)
    syrk_general(dtype, 1280, 128, 128, 1, 1, wide, route, plus=plus, count=3)
    syrk_general(dtype, 1280, 128, 128, 1, 1, wide, route, plus=plus, count=3, abort=(0, 7, 0))
    syrk_general(dtype, 1280, 128, 128, 1, 1, wide, route, plus=plus, abort=(0,))
    syrk_general(dtype, 1280, 128, 128, 1, 1, wide, route, plus=plus, abort=(7,))


@gpu
@BOTH
def test_syrk_bc_nb64_per_column(dtype):
    """nb = 64 is no multiple of the tile: one product per block column (each on the fast kernel, 64 columns: class SKINNY),
    the last one ragged (8 columns)."""
    did, npdt, _, _ = DTYPES[dtype]
    n, nb, kb, k0, ch = 520, 64, 64, 64, CH[dtype]
    rng = np.random.RandomState(64)
    row_begin = cl0 = k0 + kb
    ldp, ldc = kb + ch, n + 3
    Pb = np.full((n - k0 + 1, ldp), nan_in(npdt), dtype=npdt)
    Pb[:n - k0, :kb] = ints(rng, (n - k0, kb), npdt)
    C0 = np.full((n + 1, ldc), nan_out(npdt), dtype=npdt)
    low = np.tril_indices(n)
    C0[:n, :n][low] = ints(rng, low[0].size, npdt)
    dP, dC = DeviceBuffer.from_host(Pb), DeviceBuffer.from_host(C0)
    what = "%s n = %d nb = 64" % (dtype, n)
    rc, routes, launches = observed(lambda: debug_syrk(did, n, row_begin, dC.ptr, ldc, cl0, n, dP.ptr, ldp, k0, kb, nb))
    assert rc == _lib.OK, what + ": " + _lib.last_error()
    ncols = -(-(n - cl0) // nb)
    assert_ran_on(routes, launches, "FAST", "SKINNY", what, count=ncols)
    got = dC.to_host()
    written = np.zeros(C0.shape, dtype=bool)
    written[row_begin:n, cl0:n] = np.arange(row_begin, n)[:, None] >= np.arange(cl0, n)[None, :]
    assert not ((bits(got) != bits(C0)) & ~written).any(), what + ": wrote outside the update"
    p = Pb[:n - k0, :kb].astype(np.int64)
    want = np.where(written, C0, 0).astype(np.float64)
    want[row_begin:n, cl0:n] -= p[row_begin - k0:] @ p[cl0 - k0:].T
    assert np.isfinite(got[written]).all(), what
    bad = written & (got.astype(np.float64) != want)
    assert not bad.any(), first_wrong(got, want, bad, 0, 0, 0, "SKINNY", what)


# ---- refusals and empty products -----------------------------------------------------------------------------------------
@gpu
@BOTH
@pytest.mark.parametrize("entry", ["public", "debug"])
def test_refusals_leave_c_alone(dtype, entry):
    did, npdt, _, _ = DTYPES[dtype]
    es, epk, ch, lib = np.dtype(npdt).itemsize, EPK[dtype], CH[dtype], _lib.load()
    rng = np.random.RandomState(9)
    M, N, K = 130, 70, epk
    A, B, C0 = ints(rng, (M + 1, K + ch), npdt), ints(rng, (N + 1, K + ch), npdt), ints(rng, (M + 1, N + 2), npdt)
    dA, dB, dC = DeviceBuffer.from_host(A), DeviceBuffer.from_host(B), DeviceBuffer.from_host(C0)

    def gemm(a, lda, ldc, tri):
        if entry == "public":
            return lib.gpx_d_gemm_nt(did, M, N, K, -1.0, a, lda, dB.ptr, K + ch, dC.ptr, ldc, tri, 0, 0, None)
        return debug_gemm(did, M, N, K, -1.0, a, lda, dB.ptr, K + ch, dC.ptr, ldc, tri)

    for what, args in (("lda no multiple of 16 bytes", (dA.ptr, K + 1, N + 2, _lib.FULL)),
                       ("A misaligned", (at(dA, 1, es), K + ch, N + 2, _lib.FULL)),
                       ("ldc < N", (dA.ptr, K + ch, N - 1, _lib.FULL)),
                       ("tri = 2", (dA.ptr, K + ch, N + 2, 2))):
        rc, routes, launches = observed(lambda: gemm(*args))
        assert rc == _lib.ERR_ARG, what
        assert_ran_on(routes, launches, None, None, what)
        assert same_bits(dC.to_host(), C0), what + ": C changed"
    n, nb = 640, 128
    P0 = ints(rng, (n + 1, nb + ch), npdt)
    S0 = ints(rng, (n + 1, n), npdt)
    dP, dS = DeviceBuffer.from_host(P0), DeviceBuffer.from_host(S0)

    def syrk(row_begin, nb_, P, rank):
        if entry == "public":
            return lib.gpx_d_syrk_bc(did, n, row_begin, dS.ptr, n, nb, n, dP.ptr, nb + ch, 0, nb, nb_, P, rank, None)
        return debug_syrk(did, n, row_begin, dS.ptr, n, nb, n, dP.ptr, nb + ch, 0, nb, nb_, P, rank)

    for what, args in (("k0 + kb > row_begin", (nb - 1, nb, 1, 0)), ("nb = 96", (nb, 96, 1, 0)), ("rank >= P", (nb, nb, 2, 2))):
        rc, routes, launches = observed(lambda: syrk(*args))
        assert rc == _lib.ERR_ARG, what
        assert_ran_on(routes, launches, None, None, what)
        assert same_bits(dS.to_host(), S0), what + ": C changed"
    if entry == "debug":
        for what, kw in (("ktri = 2", dict(ktri=2)), ("count = 0", dict(count=0)), ("count2 = 0", dict(count2=0))):
            assert debug_gemm(did, M, N, K, -1.0, dA.ptr, K + ch, dB.ptr, K + ch, dC.ptr, N + 2, **kw) == _lib.ERR_ARG, what
        assert debug_syrk(did, n, nb, dS.ptr, n, nb, n, dP.ptr, nb + ch, 0, nb, nb, count=0) == _lib.ERR_ARG
        sync()
        assert same_bits(dC.to_host(), C0) and same_bits(dS.to_host(), S0)


@gpu
@BOTH
def test_empty_products(dtype):
    did, lib = DTYPES[dtype][0], _lib.load()
    for M, N, K in ((0, 5, 16), (5, 0, 16), (5, 5, 0)):
        assert lib.gpx_d_gemm_nt(did, M, N, K, -1.0, None, 16, None, 16, None, 16, _lib.FULL, 0, 0, None) == _lib.OK
        rc, routes, launches = observed(lambda: debug_gemm(did, M, N, K, -1.0, None, 16, None, 16, None, 16, count=3, count2=2))
        assert rc == _lib.OK
        assert_ran_on(routes, launches, None, None, "empty product")
    for n, cl1, kb in ((0, 256, 128), (256, 128, 128), (256, 256, 0)):
        assert lib.gpx_d_syrk_bc(did, n, 128, None, 256, 128, cl1, None, 128, 0, kb, 128, 1, 0, None) == _lib.OK
        rc, routes, launches = observed(lambda: debug_syrk(did, n, 128, None, 256, 128, cl1, None, 128, 0, kb, 128, count=3))
        assert rc == _lib.OK
        assert_ran_on(routes, launches, None, None, "empty update")
