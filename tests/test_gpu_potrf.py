"""The Cholesky panel and factorisation (csrc/gpx_potrf.hip, csrc/gpx_panel.hip, csrc/gpx_leaf.h) alone, on every route, both
dtypes: gpx_d_potrf_panel / gpx_d_potrf and the two debug entries gpx_debug_potrf_panel / gpx_debug_potrf (the internal
potrf_panel / potrf with the arguments the public entries hide: kpre, the idle-chip hint, lock-step batches, ride-along rows).

Conventions of every case (those of tests/test_gpu_blocks.py)
  matrices   A = fl_T(L0 L0^T), L0 lower triangular with a diagonal uniform in [1, 2] and randn / sqrt(n) below it
             (tests/_block_helpers.py: chol_l0; the product is exact, so it is the np.longdouble product); a panel at r0 > 0 gets
             the Schur complement of the columns before it, taken in np.longdouble from the float64 LAPACK factor and cast to
             T; with kpre > 0 the kpre columns before c0 hold that factor and the panel the Schur complement of the columns
             before those.
  not read   everything a call may not read holds input-NaN: the strict upper triangle (the upper half of every diagonal block
             included), the columns beyond the matrix / the panel up to lda, the rows above r0, the columns left of c0 - kpre,
             one guard row behind the last row and the gap between batch members.  A finite factor has read none of it.
  not written  every element outside the lower part of the region the call factors is compared bit for bit with the upload.
  bound      the computed L is judged by its componentwise backward error, not by its distance from another factor:
                 |A - L L^T|_ij <= 16 K_ij eps_T (|L||L|^T)_ij,   K_ij = min(i, j) + 1 (+ kpre)
             (Higham, Accuracy and Stability, Theorem 10.3: gamma_{K+1} |L||L|^T for any summation order; 16 K eps is the
             constant of tests/test_gpu_xgrad.py for the same construction, an in-block step done as a product with
             inv(L_kk)).  The residual is taken in np.longdouble up to n = 700 and in float64 BLAS above, where the
             product's own gamma_{K+1}(2^-53) |L||L|^T is added.  tests/test_potrf_premise_cpu.py shows LAPACK at 0.02 - 0.1
             of this bound on the same matrices.  Ride-along rows: |z L^T - y| <= 16 n eps_T |z||L^T|.
  twice      every case runs twice from the same upload and must give the same bits.
  route      every call asserts its PANEL_RES / PANEL_CHAIN counts, and a resident launch its instantiation
             (gpx_debug_panel_last: LV, LEAF_MFMA, one launch or two, dynamic LDS).  The asm-scheduled leaf's self-check must
             have passed (module fixture), or the LV = 4 / 5 cases would silently run LV = 1.
Routes whose code says they do the same arithmetic are compared with same_bits; nothing else is compared between routes."""
import ctypes

import numpy as np
import pytest

from _block_helpers import (DTYPES, WorstResidual, bits, chol_panel_input, chol_spd, nan_in, round_up, same_bits)
from gaussian_processes_amd import _lib
from gaussian_processes_amd.device import DeviceBuffer, sync

gpu = pytest.mark.gpu
BOTH = pytest.mark.parametrize("dtype", ["f64", "f32"])
EXACT_N = 700                             # the residual in np.longdouble up to this order
LEAF_ENVS = ("GPX_LEAF", "GPX_LEAF_MFMA_F32_ROWS", "GPX_POTRF_TWO_PART_ROWS", "GPX_RES_STRICT", "GPX_POTRF_RES",
             "GPX_POTRF_TRSM_ROWS", "GPX_POTRF_INV_MAX", "GPX_POTRF_NB", "GPX_POTRF_FOLD_ROWS", "GPX_POTRF_GATE_ROWS",
             "GPX_POTRF_NO_LOOKAHEAD", "GPX_POTRF_WIDTHS", "GPX_PANEL_EXCL_ROWS", "GPX_POTRF_TAPER", "GPX_LEAF4_ROWS")


@pytest.fixture(autouse=True)
def _defaults(monkeypatch):
    for name in LEAF_ENVS:
        monkeypatch.delenv(name, raising=False)


@pytest.fixture(scope="module")
def leaf_checked():
    st = ctypes.c_int(0)
    _lib.check(_lib.load().gpx_debug_leaf_selfcheck(1, ctypes.byref(st)))
    assert st.value == 1, "the asm-scheduled leaf's self-check reports %d: LV = 4 / 5 would run as LV = 1" % st.value


def panel_last():
    v = [ctypes.c_int(-1) for _ in range(4)]
    _lib.check(_lib.load().gpx_debug_panel_last(*[ctypes.byref(x) for x in v]))
    return dict(zip(("lv", "leaf_mfma", "two_part", "pad_lds"), (x.value for x in v)))


def observed(call):
    _lib.route_reset()
    rc = call()
    sync()
    return rc, (_lib.route_count(_lib.ROUTE_PANEL_RES), _lib.route_count(_lib.ROUTE_PANEL_CHAIN))


# ---- one panel call ------------------------------------------------------------------------------------------------------
class Panel(object):
    """`count` panels of kb columns at (r0, c0) with `below` rows under the diagonal block, uploaded once; run() factors a fresh
    copy and returns the host image."""

    def __init__(self, dtype, kb, below, r0=192, c0=None, kpre=0, count=1, seed=0):
        self.dtype, self.kb, self.below, self.r0, self.kpre, self.count = dtype, kb, below, r0, kpre, count
        self.c0 = c0 = r0 if c0 is None else c0
        self.did, self.npdt, _, self.u = DTYPES[dtype]
        self.n = n = r0 + kb + below
        self.lda = round_up(c0 + kb, 16) + 16
        self.sA = (n + 1) * self.lda + 32
        self.host = np.full(count * self.sA, nan_in(self.npdt), dtype=self.npdt)
        self.allowed = np.zeros(self.host.size, dtype=bool)
        i, j = np.arange(n - r0)[:, None], np.arange(kb)[None, :]
        self.low = j <= i
        self.inputs = []
        for m in range(count):
            s, pre = chol_panel_input(n, 100 * seed + 7 * m + kb, r0, kb, kpre)
            s, pre = s.astype(self.npdt), pre.astype(self.npdt)
            a = self.member(self.host, m)
            a[r0:n, c0:c0 + kb][self.low] = s[self.low]
            a[r0:n, c0 - kpre:c0] = pre
            self.member(self.allowed, m)[r0:n, c0:c0 + kb] = self.low
            self.inputs.append((s, pre))
        self.what = "%s kb = %d below = %d (r0, c0) = (%d, %d) kpre = %d batch %d" % (dtype, kb, below, r0, c0, kpre, count)

    def member(self, flat, m):
        return flat[m * self.sA:m * self.sA + (self.n + 1) * self.lda].reshape(self.n + 1, self.lda)

    def region(self, image, m=0):
        return self.member(image, m)[self.r0:self.n, self.c0:self.c0 + self.kb]

    def spoil(self, j, value, m=0):
        """the panel's local diagonal entry j becomes `value`"""
        self.member(self.host, m)[self.r0 + j, self.c0 + j] = value

    def run(self, routes, inst=None, idle=0, public=False, info0=None, rc_want=_lib.OK, twice=True):
        """Factor; assert status, routes, instantiation, that nothing outside the result changed; returns (image, info)."""
        lib = _lib.load()
        images = []
        for _ in range(2 if twice else 1):
            dA = DeviceBuffer.from_host(self.host)
            info = DeviceBuffer.from_host(np.asarray([0] * self.count if info0 is None else info0, dtype=np.int32))
            if public:
                assert self.count == 1 and self.kpre == 0 and not idle
                call = lambda: lib.gpx_d_potrf_panel(self.did, dA.ptr, self.lda, self.n, self.r0, self.c0, self.kb, info.ptr, None)
            else:
                call = lambda: lib.gpx_debug_potrf_panel(self.did, dA.ptr, self.lda, self.n, self.r0, self.c0, self.kb, info.ptr,
                                                         self.kpre, idle, self.count, self.sA, None)
            rc, got_routes = observed(call)
            assert rc == rc_want, "%s: status %d (%s), expected %d" % (self.what, rc, _lib.last_error(), rc_want)
            assert got_routes == tuple(routes), "%s: (PANEL_RES, PANEL_CHAIN) = %r, expected %r" % (self.what, got_routes, routes)
            if inst is not None:
                last = panel_last()
                for key, want in inst.items():
                    ok = last[key] > 0 if want == "> 0" else last[key] == want
                    assert ok, "%s: the launch was %r, expected %s = %s" % (self.what, last, key, want)
            image = dA.to_host()
            changed = bits(image) != bits(self.host)
            assert not (changed & ~self.allowed).any(), "%s: wrote outside the panel's lower part (first at flat element %d)" % (
                self.what, int(np.flatnonzero(changed & ~self.allowed)[0]))
            images.append((image, info.to_host()))
        if twice:
            assert same_bits(images[0][0], images[1][0]) and np.array_equal(images[0][1], images[1][1]), \
                self.what + ": two runs differ"
        return images[0]

    def check(self, worst, image, label=""):
        for m, (s, pre) in enumerate(self.inputs):
            worst.factor(s, self.region(image, m), self.u, "%s %s member %d" % (self.what, label, m), pre=pre,
                         exact=self.n <= EXACT_N)


RES_INST = {"lv": 4, "leaf_mfma": 1, "two_part": 0, "pad_lds": 0}         # a single matrix's short panel by default


@gpu
@BOTH
def test_panel_widths(dtype, leaf_checked):
    """Resident (1 - 4 steps), ragged (chain) and recursive halving: kb = 1024 is 512 (256 + 256 folded), one product, 512."""
    w = WorstResidual("potrf_panel widths", dtype)
    cases = [(64, 192, (1, 0)), (128, 192, (1, 0)), (192, 192, (1, 0)), (256, 192, (1, 0)), (40, 192, (0, 1)),
             (100, 192, (1, 1)), (320, 0, (2, 0)), (512, 0, (2, 0)), (1024, 0, (4, 0))]
    for kb, r0, routes in cases:
        p = Panel(dtype, kb, 65, r0=r0)
        image, info = p.run(routes, inst=RES_INST if routes[0] else None, public=True)
        assert info[0] == 0, p.what
        p.check(w, image)
    w.report()


@gpu
@BOTH
def test_panel_rows_below(dtype, leaf_checked):
    """0 rows below: the grid is the diagonal workgroups alone; 200: a ragged last workgroup."""
    w = WorstResidual("potrf_panel rows below", dtype)
    for kb in (128, 256):
        for below in (0, 1, 63, 64, 65, 200):
            p = Panel(dtype, kb, below, seed=1)
            image, info = p.run((1, 0), inst=RES_INST, public=True)
            assert info[0] == 0, p.what
            p.check(w, image)
    w.report()


@gpu
@BOTH
def test_panel_position(dtype, leaf_checked):
    """c0 != r0 is the multi-GPU layout: the same data at another column offset must give the same bits."""
    w = WorstResidual("potrf_panel position", dtype)
    for kb, routes in ((128, (1, 0)), (100, (1, 1))):
        p = Panel(dtype, kb, 65, r0=0, seed=2)
        image, info = p.run(routes, public=True)
        assert info[0] == 0, p.what
        p.check(w, image)
        p = Panel(dtype, kb, 65, r0=192, seed=2)
        home, info = p.run(routes, public=True)
        assert info[0] == 0, p.what
        p.check(w, home)
        for c0 in (0, 16, 48, 256):
            q = Panel(dtype, kb, 65, r0=192, c0=c0, seed=2)
            image, info = q.run(routes, public=True)
            assert info[0] == 0, q.what
            assert same_bits(q.region(image)[q.low], p.region(home)[p.low]), q.what + ": differs from the r0 == c0 call"
    w.report()


@gpu
@BOTH
def test_panel_leaf(dtype, leaf_checked, monkeypatch):
    """Every leaf: GPX_LEAF = 1 (compiler-scheduled MFMA leaf, in place in the accumulator tiles), 4 and 5 (the asm-scheduled
    two-wave leaf), unset; fp32 also the lean kernel with the VALU leaf (factor64_pipe)."""
    w = WorstResidual("potrf_panel leaves", dtype)
    cases = [(None, None, 4, 1), ("1", None, 1, 1), ("4", None, 4, 1), ("5", None, 5, 1)]
    if dtype == "f32":
        cases += [("1", "0", 1, 0), ("5", "0", 1, 0)]
    for leaf, f32rows, lv, mfma in cases:
        for name, val in (("GPX_LEAF", leaf), ("GPX_LEAF_MFMA_F32_ROWS", f32rows)):
            if val is None:
                monkeypatch.delenv(name, raising=False)
            else:
                monkeypatch.setenv(name, val)
        for kb, below in ((256, 65), (64, 0)):
            p = Panel(dtype, kb, below, seed=3)
            image, info = p.run((1, 0), inst={"lv": lv, "leaf_mfma": mfma, "two_part": 0, "pad_lds": 0})
            assert info[0] == 0, p.what
            p.check(w, image, "GPX_LEAF = %s F32_ROWS = %s" % (leaf, f32rows))
    w.report()


@gpu
@BOTH
def test_panel_hints_and_launches(dtype, leaf_checked, monkeypatch):
    """The exclusive-CU launch (dynamic LDS padding), the two-part launch and the relaxed hand-off do the same arithmetic."""
    w = WorstResidual("potrf_panel hints", dtype)
    p = Panel(dtype, 256, 200, seed=4)
    plain, info = p.run((1, 0), inst=RES_INST)
    assert info[0] == 0
    p.check(w, plain)
    image, _ = p.run((1, 0), inst={"lv": 4, "leaf_mfma": 1, "two_part": 0, "pad_lds": "> 0"}, idle=1)
    assert same_bits(image, plain), p.what + ": idle_chip = 1 differs"
    monkeypatch.setenv("GPX_PANEL_EXCL_ROWS", "100")                     # more rows than that: the hint is not taken
    p.run((1, 0), inst=RES_INST, idle=1, twice=False)
    monkeypatch.delenv("GPX_PANEL_EXCL_ROWS")
    monkeypatch.setenv("GPX_POTRF_TWO_PART_ROWS", "0")
    image, _ = p.run((1, 0), inst={"lv": 4, "leaf_mfma": 1, "two_part": 1, "pad_lds": 0})
    assert same_bits(image, plain), p.what + ": the two-part launch differs"
    monkeypatch.delenv("GPX_POTRF_TWO_PART_ROWS")
    monkeypatch.setenv("GPX_RES_STRICT", "0")
    image, _ = p.run((1, 0), inst=RES_INST)
    assert same_bits(image, plain), p.what + ": GPX_RES_STRICT = 0 differs"
    w.report()


@gpu
@BOTH
def test_panel_fold(dtype, leaf_checked):
    """The folded pre-update (kpre columns to the left applied inside the launch) against the backward-error bound; a kpre the
    resident route cannot take is refused and nothing is written."""
    w = WorstResidual("potrf_panel fold", dtype)
    for kpre in (64, 128, 256):
        for kb, below in ((128, 65), (256, 0)):
            p = Panel(dtype, kb, below, r0=256, kpre=kpre, seed=5)
            image, info = p.run((1, 0), inst=RES_INST)
            assert info[0] == 0, p.what
            p.check(w, image)
    # the same panel with the pre-update done on the host (np.longdouble, cast): kpre = 0 on chol_panel_input
    p = Panel(dtype, 128, 65, r0=256, seed=5)
    image, info = p.run((1, 0), inst=RES_INST)
    assert info[0] == 0
    p.check(w, image, "host pre-update")
    for kb, r0, kpre in ((128, 320, 320), (40, 256, 64), (512, 256, 64)):
        p = Panel(dtype, kb, 65, r0=r0, kpre=kpre, seed=5)
        image, _ = p.run((0, 0), rc_want=_lib.ERR_ARG, twice=False)
        assert same_bits(image, p.host), p.what + ": a refused call wrote"
    w.report()


@gpu
@BOTH
def test_panel_chain(dtype, monkeypatch):
    """GPX_POTRF_RES=0: the leaf (potrf_diag_kernel) + inverse and one product; with GPX_POTRF_TRSM_ROWS=1 or
    GPX_POTRF_INV_MAX=0 the row substitution instead (trsm_rows_kernel: the 64-wide vector form and the ragged form)."""
    w = WorstResidual("potrf_panel chain", dtype)
    monkeypatch.setenv("GPX_POTRF_RES", "0")
    for kb, routes in ((64, (0, 1)), (40, (0, 1)), (128, (0, 2))):
        p = Panel(dtype, kb, 200, seed=6)
        image, info = p.run(routes, public=True)
        assert info[0] == 0, p.what
        p.check(w, image, "inverse + product")
        monkeypatch.setenv("GPX_POTRF_TRSM_ROWS", "1")
        rows, info = p.run(routes, public=True)
        assert info[0] == 0, p.what
        p.check(w, rows, "trsm_rows")
        monkeypatch.delenv("GPX_POTRF_TRSM_ROWS")
        monkeypatch.setenv("GPX_POTRF_INV_MAX", "0")
        image, info = p.run(routes, public=True)
        assert info[0] == 0 and same_bits(image, rows), p.what + ": GPX_POTRF_INV_MAX = 0 differs from GPX_POTRF_TRSM_ROWS = 1"
        monkeypatch.delenv("GPX_POTRF_INV_MAX")
    w.report()


@gpu
@BOTH
def test_panel_batch(dtype, leaf_checked, monkeypatch):
    """Three different matrices in lock-step (LV = 5 by default); a member alone gives the same bits; a non-positive-definite
    member leaves the others and their info words alone."""
    w = WorstResidual("potrf_panel batch", dtype)
    p = Panel(dtype, 256, 65, count=3, seed=7)
    image, info = p.run((1, 0), inst={"lv": 5, "leaf_mfma": 1, "two_part": 0, "pad_lds": 0})
    assert not info.any(), info
    p.check(w, image)
    monkeypatch.setenv("GPX_LEAF", "5")
    forced, info = p.run((1, 0), inst={"lv": 5, "leaf_mfma": 1, "two_part": 0, "pad_lds": 0})
    assert not info.any() and same_bits(forced, image)
    for m in range(3):
        one = Panel(dtype, 256, 65, seed=7)
        one.host[:] = p.host[m * p.sA:(m + 1) * p.sA]
        alone, info = one.run((1, 0), inst={"lv": 5, "leaf_mfma": 1, "two_part": 0, "pad_lds": 0})
        assert info[0] == 0 and same_bits(one.region(alone)[one.low], p.region(image, m)[p.low]), "member %d alone differs" % m
    monkeypatch.delenv("GPX_LEAF")
    p.spoil(70, -1.0, m=1)
    # (once: what a failing member's other workgroups still compute depends on when they start, and is nobody's result)
    bad, info = p.run((1, 0), twice=False)
    assert list(info) == [0, p.r0 + 71, 0], info
    for m in (0, 2):
        assert same_bits(p.member(bad, m), p.member(image, m)), "member %d changed beside a failing one" % m
    w.report()


@gpu
@BOTH
def test_panel_info(dtype, leaf_checked):
    """The first failing pivot is reported as r0 + j + 1, whatever step and leaf row it falls in; a panel that finds info set
    does nothing; the next good panel is factored as if nothing had happened."""
    w = WorstResidual("potrf_panel after a failure", dtype)
    for value in (-1.0, 0.0, float("nan")):
        for j in (0, 63, 64, 130, 255):
            p = Panel(dtype, 256, 65, seed=8)
            p.spoil(j, value)
            _, info = p.run((1, 0), inst=RES_INST, twice=False)
            assert info[0] == p.r0 + j + 1, "%s: pivot %d = %r reported as %d" % (p.what, j, value, info[0])
    p = Panel(dtype, 256, 65, seed=8)
    image, info = p.run((1, 0), inst=RES_INST, info0=[5], twice=False)
    assert info[0] == 5 and same_bits(image, p.host), p.what + ": a panel behind a failure must not compute"
    image, info = p.run((1, 0), inst=RES_INST)
    assert info[0] == 0
    p.check(w, image)
    w.report()


# ---- one factorisation ---------------------------------------------------------------------------------------------------
class Matrix(object):
    """`count` matrices of order n with xrows ride-along rows each, uploaded once."""

    def __init__(self, dtype, n, xrows=0, count=1, seed=0):
        self.dtype, self.n, self.xrows, self.count = dtype, n, xrows, count
        self.did, self.npdt, _, self.u = DTYPES[dtype]
        self.lda = round_up(n, 16) + 16
        rows = n + xrows + 1
        self.sA = rows * self.lda + 48
        self.host = np.full(count * self.sA, nan_in(self.npdt), dtype=self.npdt)
        self.allowed = np.zeros(self.host.size, dtype=bool)
        self.low = np.tril(np.ones((n, n), dtype=bool))
        rng = np.random.RandomState(1000 * seed + n)
        self.inputs = []
        for m in range(count):
            a = chol_spd(n, 100 * seed + 7 * m + n).astype(self.npdt)
            y = rng.randn(xrows, n).astype(self.npdt)
            img = self.member(self.host, m)
            img[:n, :n][self.low] = a[self.low]
            img[n:n + xrows, :n] = y
            ok = self.member(self.allowed, m)
            ok[:n, :n] = self.low
            ok[n:n + xrows, :n] = True
            self.inputs.append((a, y))
        self.what = "%s n = %d xrows = %d batch %d" % (dtype, n, xrows, count)

    def member(self, flat, m):
        rows = self.n + self.xrows + 1
        return flat[m * self.sA:m * self.sA + rows * self.lda].reshape(rows, self.lda)

    def spoil(self, j, value):
        self.member(self.host, 0)[j, j] = value

    def run(self, routes, public=False, twice=True):
        lib = _lib.load()
        images = []
        for _ in range(2 if twice else 1):
            dA = DeviceBuffer.from_host(self.host)
            info = DeviceBuffer.from_host(np.full(self.count, 77, dtype=np.int32))     # (the call clears it)
            if public:
                assert self.count == 1 and self.xrows == 0
                call = lambda: lib.gpx_d_potrf(self.did, dA.ptr, self.n, self.lda, info.ptr, None)
            else:
                call = lambda: lib.gpx_debug_potrf(self.did, dA.ptr, self.n, self.lda, info.ptr, self.xrows, self.count, self.sA,
                                                   None)
            rc, got_routes = observed(call)
            assert rc == _lib.OK, "%s: status %d (%s)" % (self.what, rc, _lib.last_error())
            if routes is not None:
                assert got_routes == tuple(routes), "%s: (PANEL_RES, PANEL_CHAIN) = %r, expected %r" % (self.what, got_routes, routes)
            image = dA.to_host()
            changed = bits(image) != bits(self.host)
            assert not (changed & ~self.allowed).any(), "%s: wrote outside the lower triangle (first at flat element %d)" % (
                self.what, int(np.flatnonzero(changed & ~self.allowed)[0]))
            images.append((image, info.to_host()))
        if twice:
            assert same_bits(images[0][0], images[1][0]) and np.array_equal(images[0][1], images[1][1]), \
                self.what + ": two runs differ"
        return images[0]

    def check(self, worst, image, label=""):
        n = self.n
        for m, (a, y) in enumerate(self.inputs):
            got = self.member(image, m)
            what = "%s %s member %d" % (self.what, label, m)
            worst.factor(a, got[:n, :n], self.u, what, exact=n <= EXACT_N)
            if self.xrows:
                worst.ride(y, got[n:n + self.xrows, :n], got[:n, :n], self.u, what + " ride-along rows")


# (PANEL_RES, PANEL_CHAIN) of one factorisation with the default outer block of 256: 64-column multiples are resident launches
# (the next panel folds the update when it is resident too), a ragged tail halves down to a leaf of the chain
ROUTES = {1: (0, 1), 63: (0, 1), 64: (1, 0), 65: (1, 1), 100: (1, 1), 256: (1, 0), 257: (1, 1), 320: (2, 0), 449: (3, 1),
          1104: (5, 1)}


@gpu
@BOTH
def test_potrf_sizes(dtype, leaf_checked):
    w = WorstResidual("potrf sizes", dtype)
    for n in (1, 63, 64, 65, 100, 256, 257, 320, 449, 1104):
        a = Matrix(dtype, n)
        image, info = a.run(ROUTES[n], public=True)
        assert info[0] == 0, a.what
        a.check(w, image)
    w.report()


@gpu
@BOTH
def test_potrf_forced_widths(dtype, leaf_checked, monkeypatch):
    """GPX_POTRF_NB: folds of 64 / 128 / 256 columns between panels; 512: a panel whose right half folds its left half."""
    w = WorstResidual("potrf forced widths", dtype)
    routes = {(64, 449): (7, 1), (128, 449): (4, 1), (256, 449): (3, 1), (512, 449): (3, 1),
              (64, 1104): (17, 1), (128, 1104): (9, 1), (256, 1104): (5, 1), (512, 1104): (5, 1)}
    for (nb, n), want in sorted(routes.items()):
        monkeypatch.setenv("GPX_POTRF_NB", str(nb))
        a = Matrix(dtype, n)
        image, info = a.run(want, public=True)
        assert info[0] == 0, a.what
        a.check(w, image, "GPX_POTRF_NB = %d" % nb)
    w.report()


@gpu
@BOTH
def test_potrf_schedule_switches(dtype, leaf_checked, monkeypatch):
    w = WorstResidual("potrf schedule switches", dtype)
    a = Matrix(dtype, 1104)
    monkeypatch.setenv("GPX_POTRF_FOLD_ROWS", "0")
    gated, info = a.run((5, 1), public=True)
    assert info[0] == 0
    a.check(w, gated, "GPX_POTRF_FOLD_ROWS = 0")
    monkeypatch.setenv("GPX_POTRF_GATE_ROWS", "0")
    image, info = a.run((5, 1), public=True)
    assert info[0] == 0 and same_bits(image, gated), "GPX_POTRF_GATE_ROWS = 0 differs from the gated run"
    monkeypatch.delenv("GPX_POTRF_GATE_ROWS")
    monkeypatch.delenv("GPX_POTRF_FOLD_ROWS")
    for name, value, routes in (("GPX_POTRF_NO_LOOKAHEAD", "1", (5, 1)), ("GPX_POTRF_RES", "0", (0, 18)),
                                ("GPX_POTRF_RES", "128", (9, 1))):
        monkeypatch.setenv(name, value)
        image, info = a.run(routes, public=True)
        assert info[0] == 0, (name, value)
        a.check(w, image, "%s = %s" % (name, value))
        monkeypatch.delenv(name)
    w.report()


@gpu
@BOTH
def test_potrf_taper(dtype, leaf_checked, monkeypatch):
    """One factorisation that changes its panel width on the way.  GPX_POTRF_WIDTHS = "300,700,1500" at n = 2341: 1024, 512, 512,
    128, 128 and a ragged 37 (the width follows the rows that are left: 1317, 805, 293, 165, 37); "300,900,1500" adds the
    step the first leaves out: 1024, 512, 256, 256, 128, 128, 37."""
    w = WorstResidual("potrf taper", dtype)
    a = Matrix(dtype, 2341)
    for widths in ("300,700,1500", "300,900,1500"):
        monkeypatch.setenv("GPX_POTRF_WIDTHS", widths)
        image, info = a.run((10, 1), public=True, twice=widths == "300,700,1500")
        assert info[0] == 0, widths
        a.check(w, image, "GPX_POTRF_WIDTHS = %s" % widths)
    w.report()


@gpu
@BOTH
def test_potrf_ride_along_rows(dtype, leaf_checked):
    """Rows below the matrix take part in every panel and update as rows: row n + i ends as L^-1 applied to what it held."""
    w = WorstResidual("potrf ride-along rows", dtype)
    for n in (257, 1104):
        for xrows in (1, 3):
            a = Matrix(dtype, n, xrows=xrows, seed=1)
            image, info = a.run(ROUTES[n])
            assert info[0] == 0, a.what
            a.check(w, image)
    w.report()


@gpu
def test_potrf_batches_interleaved(leaf_checked):
    """Lock-step batches of both dtypes and several sizes in turn: the published-block scratch is laid out anew in between."""
    worst = {d: WorstResidual("potrf batches", d) for d in ("f64", "f32")}
    for dtype, n, count, xrows in (("f64", 320, 2, 0), ("f32", 257, 3, 1), ("f64", 257, 1, 0), ("f32", 320, 2, 0),
                                   ("f64", 449, 3, 1), ("f32", 449, 1, 0), ("f64", 320, 2, 0)):
        a = Matrix(dtype, n, xrows=xrows, count=count, seed=2)
        image, info = a.run(ROUTES[n])
        assert not info.any(), (a.what, info)
        a.check(worst[dtype], image)
    for w in worst.values():
        w.report()


@gpu
@BOTH
def test_potrf_info(dtype, leaf_checked):
    """Pivots of 0 and NaN (tests/test_gpu_parity.py has -1) at the first and last index and on both sides of a panel edge."""
    for value in (0.0, float("nan")):
        for j in (0, 255, 256, 1103):
            a = Matrix(dtype, 1104)
            a.spoil(j, value)
            _, info = a.run(None, public=True, twice=False)
            assert info[0] == j + 1, "%s: pivot %d = %r reported as %d" % (a.what, j, value, info[0])
