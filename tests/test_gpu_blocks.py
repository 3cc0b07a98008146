"""Each small device block (gpx_d_*) alone against a high-precision reference of the same operation, both dtypes.

Conventions of every case
  inputs     drawn in float64 and cast to the block's dtype T; the reference is computed from the CAST values in
             np.longdouble, so the only error left is the block's own.
  padding    columns beyond n (every block sees a leading dimension > n in at least one case) and every region a block's
             comment says it does not read (a strict upper triangle, the gap between two slices) hold NaN: a result that is
             finite has read none of it.  Regions a block does not write are compared bit for bit (NaN payload included)
             with what was uploaded; written arrays carry one guard row (or guard elements) behind their end.
  twice      every reduction runs twice on the same input and must give the same bits (fixed summation order, no atomics).

Tolerances are derived, not measured.  With u = 2^-53 and gamma_k = k u / (1 - k u):
  a sum of k terms accumulated in fp64 in ANY order, products formed by fma, lies within gamma_k * sum|term| of the exact sum
  (Higham, Accuracy and Stability of Numerical Algorithms, section 4.2: the bound holds for every summation tree);
  the final cast to T adds u_T * |ref|, u_T = eps_T / 2 (2^-53 for double outputs, 2^-24 for float ones).
Every comparison asserts, componentwise,

      |got - ref| <= 4 * (gamma_k * sum|term| + u_T * |ref|)

The factor 4 covers what the formula leaves out: the rounding of a division (form_B) or of HIP's double log (within 1 ulp =
2 u, logdet_chol), and the roundings of the one or two subtractions that combine two such sums (var_rows2, panel_gemv_t).
A value that is added to the sum (the preloaded accumulator of gemv_acc, y of panel_gemv_t, the 1 on B's diagonal) counts as
one more term.  Pure data movement (tril, transpose, mirror_lower) is compared with np.array_equal.
Each test prints its worst |got - ref| / (asserted bound) per block and dtype."""
import numpy as np
import pytest

from _block_helpers import DTYPES, LD, U, Worst, at, nan_in, nan_out, padded, round_up, same_bits
from gaussian_processes_amd import _lib
from gaussian_processes_amd.device import DeviceBuffer, sync

pytestmark = pytest.mark.gpu


def scalar_out():
    """A double on the device between two guard doubles: (buffer, pointer to the middle one, the uploaded array)."""
    h = np.full(3, nan_out(np.float64))
    buf = DeviceBuffer.from_host(h)
    return buf, at(buf, 1, 8), h


def read_scalar(buf, h0, what):
    sync()
    h = buf.to_host()
    assert same_bits(h[[0, 2]], h0[[0, 2]]), "%s: wrote beside its output" % what
    return h[1]


# ---- the two single-workgroup reductions -----------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_d_dot(dtype):
    did, npdt, _, _ = DTYPES[dtype]
    lib, rng, worst = _lib.load(), np.random.RandomState(101), Worst("gpx_d_dot", dtype)
    for n in (1, 63, 64, 65, 1023, 1024, 1025, 5000):
        a, b = padded(rng, 1, n, n + 7, npdt)[0], padded(rng, 1, n, n + 7, npdt)[0]        # NaN behind the end
        da, db = DeviceBuffer.from_host(a), DeviceBuffer.from_host(b)
        prod = a[:n].astype(LD) * b[:n].astype(LD)
        got = []
        for _ in range(2):
            out, p, h0 = scalar_out()
            _lib.check(lib.gpx_d_dot(did, da.ptr, db.ptr, n, p, None))
            got.append(read_scalar(out, h0, "dot n = %d" % n))
        assert same_bits(got[0], got[1]), "dot n = %d: two runs differ" % n
        worst.check(got[0], prod.sum(), np.abs(prod).sum(), n, U, "n = %d" % n)
    out, p, h0 = scalar_out()
    assert lib.gpx_d_dot(did, None, None, 0, p, None) == _lib.OK                       # n = 0: nothing is read
    assert read_scalar(out, h0, "dot n = 0") == 0.0
    worst.report()


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_d_logdet_chol(dtype):
    did, npdt, _, _ = DTYPES[dtype]
    lib, rng, worst = _lib.load(), np.random.RandomState(102), Worst("gpx_d_logdet_chol", dtype)
    for n in (1, 63, 64, 65, 1023, 1024, 1025, 5000):
        ldl = n + (1 if n == 5000 else 5)
        L = np.full((n, ldl), nan_in(npdt), dtype=npdt)                                   # NaN everywhere off the diagonal
        L[np.arange(n), np.arange(n)] = rng.uniform(0.5, 2.0, n)
        dL = DeviceBuffer.from_host(L)
        logs = np.log(np.diag(L).astype(LD))
        got = []
        for _ in range(2):
            out, p, h0 = scalar_out()
            _lib.check(lib.gpx_d_logdet_chol(did, dL.ptr, n, ldl, p, None))
            got.append(read_scalar(out, h0, "logdet_chol n = %d" % n))
        assert same_bits(got[0], got[1]), "logdet_chol n = %d: two runs differ" % n
        worst.check(got[0], 2 * logs.sum(), 2 * np.abs(logs).sum(), n, U, "n = %d" % n)
        dL.free()
    out, p, h0 = scalar_out()
    assert lib.gpx_d_logdet_chol(did, None, 0, 0, p, None) == _lib.OK
    assert read_scalar(out, h0, "logdet_chol n = 0") == 0.0
    worst.report()


# ---- pure data movement ----------------------------------------------------------------------------------------------------
def _lower_upper(n, ld):
    i, j = np.arange(n + 1)[:, None], np.arange(ld)[None, :]
    inside = (i < n) & (j < n)
    return inside & (j <= i), inside & (j > i), ~inside                # lower with diagonal, strict upper, padding and guard row


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_d_tril(dtype):
    did, npdt, _, _ = DTYPES[dtype]
    lib, rng = _lib.load(), np.random.RandomState(103)
    for n in (1, 2, 33, 257, 300):
        for lda in (n, round_up(n, 16) + 16):
            low, up, pad = _lower_upper(n, lda)
            A = padded(rng, n + 1, n, lda, npdt)
            A[n, :] = nan_in(npdt)                                      # the guard row
            if lda != n:
                A[up] = nan_in(npdt)                                    # zeroing is a store, whatever was there
            dA = DeviceBuffer.from_host(A)
            _lib.check(lib.gpx_d_tril(did, dA.ptr, n, lda, None))
            sync()
            got = dA.to_host()
            what = "tril n = %d lda = %d" % (n, lda)
            assert np.array_equal(got[up], np.zeros(int(up.sum()), dtype=npdt)), what + ": strict upper triangle"
            assert same_bits(got[low], A[low]), what + ": diagonal / lower triangle"
            assert same_bits(got[pad], A[pad]), what + ": padding"


TRANSPOSE_N = (1, 31, 32, 33, 63, 64, 65, 100, 130, 300)      # around one and two 32-wide tiles, several tiles, a ragged last one


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_d_transpose(dtype):
    did, npdt, _, _ = DTYPES[dtype]
    lib, rng = _lib.load(), np.random.RandomState(104)
    for n in TRANSPOSE_N:
        for ldi, ldo in ((n + 3, round_up(n, 16) + 16), (n + 8, n)):
            _, _, pad = _lower_upper(n, ldo)
            A = padded(rng, n, n, ldi, npdt)
            O = np.full((n + 1, ldo), nan_out(npdt), dtype=npdt)
            dA, dO = DeviceBuffer.from_host(A), DeviceBuffer.from_host(O)
            _lib.check(lib.gpx_d_transpose(did, dA.ptr, ldi, dO.ptr, ldo, n, None))
            sync()
            got = dO.to_host()
            what = "transpose n = %d ldi = %d ldo = %d" % (n, ldi, ldo)
            assert np.array_equal(got[:n, :n], A[:n, :n].T), what
            assert same_bits(got[pad], O[pad]), what + ": padding"
            assert same_bits(dA.to_host(), A), what + ": the input"


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_d_mirror_lower(dtype):
    did, npdt, _, _ = DTYPES[dtype]
    lib, rng = _lib.load(), np.random.RandomState(105)
    for n in TRANSPOSE_N:
        for lda in (n + 3, n):
            low, up, pad = _lower_upper(n, lda)
            A = padded(rng, n + 1, n, lda, npdt)
            A[n, :] = nan_in(npdt)
            A[up] = nan_in(npdt)
            dA = DeviceBuffer.from_host(A)
            _lib.check(lib.gpx_d_mirror_lower(did, dA.ptr, n, lda, None))
            sync()
            got = dA.to_host()
            what = "mirror_lower n = %d lda = %d" % (n, lda)
            sq = got[:n, :n]
            assert not np.isnan(sq).any(), what + ": NaN inside n x n"
            assert np.array_equal(sq, sq.T), what + ": not symmetric"
            assert same_bits(got[low], A[low]), what + ": the lower triangle changed"
            assert np.array_equal(sq, np.tril(A[:n, :n]) + np.tril(A[:n, :n], -1).T), what
            assert same_bits(got[pad], A[pad]), what + ": padding"


# ---- the Schur complement of few rows against many columns ---------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_d_schur_lower(dtype):
    """S (k x k, lower) -= B B^T, B k x n.  k = 70 is one 128-tile, so the slice width is round_up(max(256, cdiv(n, 1024)), 128)
    = 256: n = 600 is two whole slices and a ragged one of 88 columns, their partial Grams folded by sum_slices_lower in its
    subtracting mode (ldb = 608: the aligned product with beta = 0; ldb = 603: the cleared partials); n = 200 is ONE slice,
    the product adds -B B^T straight into S and nothing is folded.
    Bound: entry (i, j) is a sum of n + 1 terms -- S[i, j] and the n products -- whatever the slicing, and the rounding of a
    partial Gram to T is one more node of that summation tree; the product kernel accumulates in T, so gamma_(n+1) is taken
    with u_T (for T = double that is the file's gamma), and the one subtraction's result is rounded to T: u_T |ref|."""
    did, npdt, _, ut = DTYPES[dtype]
    lib, rng, worst = _lib.load(), np.random.RandomState(111), Worst("gpx_d_schur_lower", dtype)
    k = 70
    for n, ldb in ((600, 608), (600, 603), (200, 208)):
        lds = round_up(k, 16) + 16
        low, up, pad = _lower_upper(k, lds)
        B = padded(rng, k, n, ldb, npdt)                                # NaN beyond column n
        S0 = np.full((k + 1, lds), nan_in(npdt), dtype=npdt)            # NaN: the strict upper triangle, the pitch, the guard row
        S0[low] = (rng.randn(int(low.sum())) * np.sqrt(n)).astype(npdt)
        dB = DeviceBuffer.from_host(B)
        got = []
        for _ in range(2):
            dS = DeviceBuffer.from_host(S0)
            _lib.check(lib.gpx_d_schur_lower(did, dB.ptr, k, n, ldb, dS.ptr, lds, None))
            sync()
            got.append(dS.to_host())
        what = "k = %d n = %d ldb = %d lds = %d" % (k, n, ldb, lds)
        assert same_bits(got[0], got[1]), what + ": two runs differ"
        assert same_bits(got[0][up | pad], S0[up | pad]), what + ": strict upper triangle / padding of S"
        assert same_bits(dB.to_host(), B), what + ": the input"
        Bl = B[:, :n].astype(LD)
        il = np.tril_indices(k)
        s0 = S0[:k, :k].astype(LD)[il]
        prod = Bl[il[0]] * Bl[il[1]]                                    # (pairs, n): the n products of every entry
        worst.check(got[0][:k, :k][il], s0 - prod.sum(1), np.abs(s0) + np.abs(prod).sum(1), n + 1, ut, what, u_acc=ut)
    worst.report()


# ---- the sparse fit's small kernels ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_d_sum_slices_lower(dtype):
    did, npdt, _, ut = DTYPES[dtype]
    lib, rng, worst = _lib.load(), np.random.RandomState(106), Worst("gpx_d_sum_slices_lower", dtype)
    for n in (1, 17, 256, 257, 300):
        for slices in (1, 3, 16):
            for ldp, ldo, gap in ((n + 4, n + 7, 16), (n, n, 0)):
                sP = n * ldp + gap
                low, up, pad = _lower_upper(n, ldo)
                P = np.full(slices * sP, nan_in(npdt), dtype=npdt)      # NaN: the gaps, the padding, every strict upper triangle
                il = np.tril_indices(n)
                parts = rng.randn(slices, il[0].size).astype(npdt)
                for s in range(slices):
                    P[s * sP + il[0] * ldp + il[1]] = parts[s]
                O = np.full((n + 1, ldo), nan_out(npdt), dtype=npdt)
                dP = DeviceBuffer.from_host(P)
                got = []
                for _ in range(2):
                    dO = DeviceBuffer.from_host(O)
                    _lib.check(lib.gpx_d_sum_slices_lower(did, dP.ptr, ldp, sP, slices, n, dO.ptr, ldo, None))
                    sync()
                    got.append(dO.to_host())
                what = "n = %d slices = %d ldp = %d sP = %d ldo = %d" % (n, slices, ldp, sP, ldo)
                assert same_bits(got[0], got[1]), what + ": two runs differ"
                assert same_bits(got[0][up | pad], O[up | pad]), what + ": strict upper triangle / padding of out"
                worst.check(got[0][:n, :n][il], parts.astype(LD).sum(0), np.abs(parts.astype(LD)).sum(0), slices, ut, what)
    worst.report()


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_d_gemv_acc(dtype):
    did, npdt, _, _ = DTYPES[dtype]
    es = np.dtype(npdt).itemsize
    lib, rng, worst = _lib.load(), np.random.RandomState(107), Worst("gpx_d_gemv_acc", dtype)
    for rows in (1, 5, 300):
        for cols in (1, 255, 256, 257, 1000):
            ldg = 2 * cols + 3                                          # two column blocks side by side, NaN behind them
            G = padded(rng, rows, 2 * cols, ldg, npdt)
            y = rng.randn(2 * cols).astype(npdt)
            acc0 = np.concatenate([rng.randn(rows), [nan_out(np.float64)]])          # one guard double behind the rows
            dG, dy = DeviceBuffer.from_host(G), DeviceBuffer.from_host(y)
            terms = G[:, :2 * cols].astype(LD) * y.astype(LD)[None, :]
            got = []
            for _ in range(2):
                dacc = DeviceBuffer.from_host(acc0)
                _lib.check(lib.gpx_d_gemv_acc(did, dG.ptr, rows, cols, ldg, dy.ptr, dacc.ptr, None))
                sync()
                one = dacc.to_host()
                _lib.check(lib.gpx_d_gemv_acc(did, at(dG, cols, es), rows, cols, ldg, at(dy, cols, es), dacc.ptr, None))
                sync()
                got.append((one, dacc.to_host()))
            what = "rows = %d cols = %d" % (rows, cols)
            for k in range(2):
                assert same_bits(got[0][k], got[1][k]), what + ": two runs differ"
                assert same_bits(got[0][k][rows:], acc0[rows:]), what + ": wrote behind acc"
            a0 = acc0[:rows].astype(LD)
            for k, name in ((1, "first block"), (2, "second block")):
                t = terms[:, :k * cols]
                worst.check(got[0][k - 1][:rows], a0 + t.sum(1), np.abs(a0) + np.abs(t).sum(1), k * cols + 1, U, "%s, %s" % (what, name))
    worst.report()


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_d_panel_gemv_t(dtype):
    did, npdt, _, ut = DTYPES[dtype]
    lib, rng, worst = _lib.load(), np.random.RandomState(108), Worst("gpx_d_panel_gemv_t", dtype)
    for rows in (1, 255, 256, 257, 700):
        for ncols in (1, 37, 256, 300, 1024):
            for ldl in (ncols, ncols + 8):
                Lp = padded(rng, rows, ncols, ldl, npdt)
                x = padded(rng, 1, rows, rows + 5, npdt)[0]
                y0 = padded(rng, 1, ncols, ncols + 3, npdt, fill=nan_out(npdt))[0]
                nwork = -(-rows // 256) * ncols
                work0 = np.full(nwork + 4, nan_out(np.float64))                          # four guard doubles behind the scratch
                dL, dx = DeviceBuffer.from_host(Lp), DeviceBuffer.from_host(x)
                got = []
                for _ in range(2):
                    dy, dw = DeviceBuffer.from_host(y0), DeviceBuffer.from_host(work0)
                    _lib.check(lib.gpx_d_panel_gemv_t(did, dL.ptr, ldl, rows, ncols, dx.ptr, dy.ptr, dw.ptr, None))
                    sync()
                    got.append(dy.to_host())
                    assert same_bits(dw.to_host()[nwork:], work0[nwork:]), "wrote behind work"
                what = "rows = %d ncols = %d ldl = %d" % (rows, ncols, ldl)
                assert same_bits(got[0], got[1]), what + ": two runs differ"
                assert same_bits(got[0][ncols:], y0[ncols:]), what + ": wrote behind y"
                terms = Lp[:, :ncols].astype(LD) * x[:rows].astype(LD)[:, None]
                yl = y0[:ncols].astype(LD)
                worst.check(got[0][:ncols], yl - terms.sum(0), np.abs(yl) + np.abs(terms).sum(0), rows + 1, ut, what)
    worst.report()


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_d_sgp_form_B(dtype):
    did, npdt, _, ut = DTYPES[dtype]
    lib, rng = _lib.load(), np.random.RandomState(109)
    worst, worst_tr = Worst("gpx_d_sgp_form_B", dtype), Worst("gpx_d_sgp_form_B (trace)", dtype)
    for n in (1, 17, 255, 256, 257, 300):
        for s, (ldx, ldb) in zip((0.5, 1.0, 3.0), ((n + 5, round_up(n, 16) + 16), (n, n + 1), (n + 1, n))):
            low, up, pad = _lower_upper(n, ldb)
            X = padded(rng, n, n, ldx, npdt)
            X[np.triu_indices(n, 1)] = nan_in(npdt)
            B0 = np.full((n + 1, ldb), nan_out(npdt), dtype=npdt)
            dX = DeviceBuffer.from_host(X)
            got, tr = [], []
            for _ in range(2):
                dB = DeviceBuffer.from_host(B0)
                out, p, h0 = scalar_out()
                _lib.check(lib.gpx_d_sgp_form_B(did, dX.ptr, ldx, n, s, dB.ptr, ldb, p, None))
                tr.append(read_scalar(out, h0, "form_B trace"))
                got.append(dB.to_host())
            what = "n = %d s = %g ldx = %d ldb = %d" % (n, s, ldx, ldb)
            assert same_bits(got[0], got[1]) and same_bits(tr[0], tr[1]), what + ": two runs differ"
            assert same_bits(got[0][up | pad], B0[up | pad]), what + ": strict upper triangle / padding of B"
            il = np.tril_indices(n)
            q = X[:n, :n][il].astype(LD) / (LD(s) * LD(s))
            eye = (il[0] == il[1]).astype(LD)
            worst.check(got[0][:n, :n][il], eye + q, eye + np.abs(q), 2, ut, what)
            diag = np.diag(X[:n, :n]).astype(LD)
            worst_tr.check(tr[0], diag.sum(), np.abs(diag).sum(), n, U, what)
    worst.report()
    worst_tr.report()


FAMILIES = {"gaussian": (_lib.KERNEL_GAUSSIAN, np.array([1.3, 0.7])), "periodic": (_lib.KERNEL_PERIODIC, np.array([1.1, 0.8, 2.3]))}


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_d_var_rows2(dtype):
    did, npdt, _, _ = DTYPES[dtype]
    lib, rng, worst = _lib.load(), np.random.RandomState(110), Worst("gpx_d_var_rows2", dtype)
    for family, (kid, params) in sorted(FAMILIES.items()):
        for d in (1, 3):
            for rows in (1, 3, 130):
                xo = rng.uniform(-3, 3, (rows, d)).astype(npdt)
                dxo, dK = DeviceBuffer.from_host(xo), DeviceBuffer((rows, rows), npdt)
                _lib.check(lib.gpx_d_kmat(did, kid, _lib.K, dxo.ptr, rows, dxo.ptr, rows, d, _lib.dptr(params), 0.0, _lib.FULL,
                                          dK.ptr, rows, None))
                sync()
                kdiag = np.diag(dK.to_host()).astype(np.float64)
                assert np.isfinite(kdiag).all()
                for n in (0, 1, 24, 255, 256, 257, 300):
                    ldx = n + 9
                    V, W = padded(rng, rows, n, ldx, npdt), padded(rng, rows, n, ldx, npdt)
                    dV, dW = DeviceBuffer.from_host(V), DeviceBuffer.from_host(W)
                    out0 = np.full(rows + 1, nan_out(np.float64))
                    got = []
                    for _ in range(2):
                        dout = DeviceBuffer.from_host(out0)
                        _lib.check(lib.gpx_d_var_rows2(did, kid, dV.ptr, dW.ptr, rows, n, ldx, dxo.ptr, d, _lib.dptr(params), dout.ptr,
                                                       None))
                        sync()
                        got.append(dout.to_host())
                    what = "%s d = %d rows = %d n = %d" % (family, d, rows, n)
                    assert same_bits(got[0], got[1]), what + ": two runs differ"
                    assert same_bits(got[0][rows:], out0[rows:]), what + ": wrote behind out"
                    if n == 0:
                        assert same_bits(got[0][:rows], kdiag), what + ": not the diagonal of gpx_d_kmat(xo, xo)"
                        continue
                    v2, w2 = V[:, :n].astype(LD) ** 2, W[:, :n].astype(LD) ** 2
                    ref = kdiag.astype(LD) - (v2.sum(1) - w2.sum(1))
                    worst.check(got[0][:rows], ref, v2.sum(1) + w2.sum(1), n, U, what)
    worst.report()
