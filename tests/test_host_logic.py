"""CPU tests (no GPU needed): host-side logic of the drop-in classes, and that
the C-ABI library loads and exports every symbol include/gpx.h declares.
Mirrors gp/tests/test_gp.py:245-432 and gp/tests/test_kernels.py:13-26 where no
device compute is involved."""
import os
import pickle
import re
from copy import copy, deepcopy

import numpy as np
import pytest

import gaussian_processes_amd as gp
from gaussian_processes_amd import _lib
from conftest import ROOT


def make_xy():
    x = np.linspace(-2 * np.pi, 2 * np.pi, 16)
    return x, np.sin(x)


def make_gp():
    x, y = make_xy()
    return gp.GP(gp.GaussianKernel(1, 1), x, y, s=1)


def test_library_exports_every_declared_symbol():
    hdr = open(os.path.join(ROOT, "include", "gpx.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(gpx_[a-z0-9_A-Z]+)\s*\(", hdr))
    declared.discard("gpx_gp")
    assert len(declared) > 50
    lib = _lib.load()
    for name in sorted(declared):
        assert hasattr(lib, name), "libgpx.so does not export %s" % name
    assert declared == set(_lib.EXPORTED_SYMBOLS), declared ^ set(_lib.EXPORTED_SYMBOLS)
    assert lib.gpx_version() == 100


def test_every_device_block_is_named_in_a_gpu_test():
    """Every exported gpx_d_* block occurs, as a word, in at least one tests/test_gpu_*.py: a block does not arrive without a
    test that calls it by name (a text search of the test sources for the API's own names, nothing more)."""
    tests = os.path.join(ROOT, "tests")
    text = "\n".join(open(os.path.join(tests, f)).read() for f in sorted(os.listdir(tests))
                     if f.startswith("test_gpu_") and f.endswith(".py"))
    words = set(re.findall(r"\bgpx_d_[a-zA-Z0-9_]+\b", text))
    blocks = [name for name in _lib.EXPORTED_SYMBOLS if name.startswith("gpx_d_")]
    assert len(blocks) > 30
    missing = [name for name in blocks if name not in words]
    assert not missing, "exported device blocks that no tests/test_gpu_*.py names: %s" % ", ".join(missing)


def test_library_never_calls_getenv():
    """Every GPX_* switch is read through ONE snapshot per API call (csrc/gpx_tune.h: a pass over `environ` at the entry
    point), never by a getenv at its point of use -- round 4 had 66 such sites, a dozen of them per panel launch.  The
    library does not even import getenv; every name in the table is documented in DESIGN.md, and no source file reads a
    switch that is not in the table."""
    import subprocess
    und = subprocess.run(["nm", "-D", "--undefined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert "getenv" not in und, [l for l in und.splitlines() if "getenv" in l]
    csrc = os.path.join(ROOT, "gaussian_processes_amd", "csrc")
    table = open(os.path.join(csrc, "gpx_tune.h")).read()
    names = set(re.findall(r'"(GPX_[A-Z0-9_]+)"', table)) | {"GPX_POTRF_WIDTHS", "GPX_MG_BCAST", "GPX_RCCL_LIB"}
    assert 30 <= len(names) <= 45, len(names)       # round 6: pruned from 61 (the routes two rounds of measurement left neutral or slower)
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    missing = [n for n in sorted(names) if ("`%s`" % n) not in design and ("`%s=" % n) not in design]
    assert not missing, missing
    for f in os.listdir(csrc):
        if f.endswith((".hip", ".h")) and f != "gpx_tune.h":
            src = open(os.path.join(csrc, f)).read()
            assert not re.search(r"\bgetenv\s*\(|env_i64\s*\(|env_set\s*\(", src), f
            for n in re.findall(r'"(GPX_[A-Z0-9_]+)"', src):
                assert n in names, (f, n)
    # a snapshot without a GPU: the counter moves with every entry point (here one that fails for lack of arguments)
    lib = _lib.load()
    import ctypes
    a, b = ctypes.c_int64(), ctypes.c_int64()
    assert lib.gpx_debug_tune_refreshes(ctypes.byref(a)) == 0
    lib.gpx_d_potrf(0, None, -1, 0, None, None)
    assert lib.gpx_debug_tune_refreshes(ctypes.byref(b)) == 0
    assert b.value == a.value + 1


def test_device_memory_has_one_owner():
    """Every allocation and release of device memory inside the library goes through csrc/gpx_mem.h (DevBuf, GrowBuf,
    ThreadScratch, dev_alloc / dev_free): before that header there were about fifty hand-written sites in seven units,
    and the copies had drifted apart (five thread-local scratch allocators leaked a block at every device switch).  The
    only other callers of the HIP allocator are the ABI's gpx_malloc / gpx_free, whose memory belongs to the caller."""
    csrc = os.path.join(ROOT, "gaussian_processes_amd", "csrc")
    call = re.compile(r"\bhip(?:Malloc|Free)\w*\s*\(")
    for f in sorted(os.listdir(csrc)):
        if not f.endswith((".hip", ".h")) or f == "gpx_mem.h":
            continue
        src = open(os.path.join(csrc, f)).read()
        if f == "gpx_runtime.hip":
            for name in ("gpx_malloc", "gpx_free"):           # drop the bodies of the two ABI functions
                m = re.search(r"^int %s\(.*?^}\n" % name, src, re.S | re.M)
                assert m and len(call.findall(m.group(0))) == 1, name
                src = src.replace(m.group(0), "")
        assert not call.search(src), (f, call.findall(src))
    assert len(call.findall(open(os.path.join(csrc, "gpx_mem.h")).read())) == 2


def test_solve_operators_keep_one_launch_site_and_one_block_width():
    """The block operators of the triangular solves (csrc/gpx_solve.hip, "operator form") are on the path of every
    solve, covariance and derivative call.  Two things a later edit could undo without any result changing at once:
    the operator step is launched from ONE forward and ONE backward sweep (the mixed backward sweep and the ragged last
    block call the same pieces; there used to be a second copy of the backward loop), and the width of an operator
    block is known to gpx_solve.hip and the one constant of gpx_common.h -- the units that use the operators ask
    trsv_ops_nblocks / trsv_ops_whole_blocks instead of dividing by a literal."""
    csrc = os.path.join(ROOT, "gaussian_processes_amd", "csrc")

    def code(f):        # without comments and string literals
        src = open(os.path.join(csrc, f)).read()
        return re.sub(r'"(?:\\.|[^"\\])*"', '""', re.sub(r"//[^\n]*", "", src))
    solve = code("gpx_solve.hip")
    assert len(re.findall(r"hipLaunchKernelGGL\(\(trsv_op_kernel<T, true>\)", solve)) == 1
    assert len(re.findall(r"hipLaunchKernelGGL\(\(trsv_op_kernel<T, false>\)", solve)) == 1
    assert len(re.findall(r"\btrsv_op_kernel<", solve)) == 2
    assert len(re.findall(r"\bTRSV_OPS_BLOCK\s*=\s*512\b", code("gpx_common.h"))) == 1
    users = [f for f in sorted(os.listdir(csrc)) if f.endswith((".hip", ".h")) and f not in ("gpx_solve.hip", "gpx_common.h")
             and re.search(r"\b(?:TrsvOps|trsv_ops_\w+|trsm_ops_ok)\b", code(f))]
    assert "gpx_gp.hip" in users and "gpx_mg.hip" in users
    for f in users:
        assert not re.search(r"\b512\b", code(f)), f


def test_cholesky_schedule_state_is_explicit():
    """The host schedule of the blocked Cholesky (csrc/gpx_potrf.hip) passes what a panel launch has to know
    as ARGUMENTS (PanelHints, the PotrfHook pointer): three thread-local side channels used to carry them across
    translation units, consumed by whichever launch came first.  What is thread-local in the factorisation's two units
    is a per-device resource and nothing else; sync events come from an EventPool (gpx_common.h), and the trailing
    update's seventeen positional arguments are written out once."""
    csrc = os.path.join(ROOT, "gaussian_processes_amd", "csrc")

    def code(f):        # without comments and string literals
        src = open(os.path.join(csrc, f)).read()
        return re.sub(r'"(?:\\.|[^"\\])*"', '""', re.sub(r"//[^\n]*", "", src))
    gone = re.compile(r"\b(?:potrf_set_hook|potrf_take_idle_chip_hint|g_idle_chip|g_hook|g_leaf_force)\b")
    for f in sorted(os.listdir(csrc)):
        if f.endswith((".hip", ".h")):
            assert not gone.search(code(f)), (f, gone.findall(code(f)))
    for f in ("gpx_potrf.hip", "gpx_panel.hip"):
        decls = [l.strip() for l in code(f).splitlines() if re.search(r"\bthread_local\b", l)]
        assert decls, f
        for l in decls:
            assert re.match(r"static thread_local (?:ThreadScratch|PerDevice<\w+>) \w+;", l), (f, l)
    for f in ("gpx_potrf.hip", "gpx_mg.hip"):
        assert "hipEventCreateWithFlags" not in code(f), f
    assert 1 <= len(re.findall(r"\bsyrk_bc\s*\(", code("gpx_potrf.hip"))) <= 2


def test_streamed_reductions_keep_one_copy_of_each_piece():
    """The kernels that stream the training set through LDS (csrc/gpx_stream.hip, DESIGN "Streamed reductions") and the tile
    reductions were grown by copying one another: the transposed chunk staging existed four times, the fixed-order block
    sum seven, the triangular tile walk and the host's slice plan three each, and seven launch sites raised the dynamic-LDS
    limit on their own with a size that depended on the call.  Each of these now has ONE definition (csrc/gpx_kernels_dev.h,
    slice_plan, set_max_lds); a new kernel on this path that brings a copy of its own fails here."""
    csrc = os.path.join(ROOT, "gaussian_processes_amd", "csrc")

    def code(f):        # without comments and string literals
        src = open(os.path.join(csrc, f)).read()
        return re.sub(r'"(?:\\.|[^"\\])*"', '""', re.sub(r"//[^\n]*", "", src))
    files = [f for f in sorted(os.listdir(csrc)) if f.endswith((".hip", ".h"))]
    assert "gpx_stream.hip" in files

    def sites(pattern):
        return {f: len(re.findall(pattern, code(f))) for f in files if re.search(pattern, code(f))}
    # the dynamic-LDS limit: set_max_lds (once per kernel and device, a constant) and nobody else
    assert sites(r"\bhipFuncSetAttribute\b") == {"gpx_runtime.hip": 1}
    for f in ("gpx_kmat.hip", "gpx_deriv.hip", "gpx_stream.hip"):
        for arg in re.findall(r"\bset_max_lds\(\(const void \*\)[^;]*?,\s*([^,;]+?)\)\);", code(f)):
            assert arg in ("LDS_CHUNK_MAX", "LDS_TILE_MAX"), (f, arg)
        assert "set_max_lds" in code(f), f
    # the carry loop of the transposed staging, the triangular index inversion, the slice plan
    assert sites(r"k -= \(?d\)?;\s*\+\+c") == {"gpx_kernels_dev.h": 1}
    assert sites(r"sqrt\(8\.0 \* \(double\)t") == {"gpx_kernels_dev.h": 1}
    assert sites(r"\bcdiv\(2048,") == {"gpx_stream.hip": 1}
    # the 64-lane shuffle-down sum: the helper, the one sum that is no four-wave block sum (the 16-wave reduce_kernel of
    # gpx_small.hip, which the strided sum of gpx_deriv.hip has become a mode of), and the one kernel that keeps the text
    # written out because the helper changes its code: member_quad_trace_kernel's interleaved pair (22 more instructions)
    # -- DESIGN "Streamed reductions".  The tile reductions of gpx_kmat.hip all go through the helper (one register array
    # for S_0, the S_k and the trace)
    assert sites(r"off = 32; off > 0; off >>= 1") == {"gpx_kernels_dev.h": 1, "gpx_deriv.hip": 1, "gpx_small.hip": 1}
    # one tile walk for the symmetric passes of both hyper-parameter gradients and, in the ARD kernel, the sparse gradient's
    # rectangular pass: ALL kernels of the file are the build, the ARD scaling, the pair of tile reductions and the one
    # rectangular kernel that measured slower as a third form of tile_reduce_kernel; one host summation of the partials
    kmat = code("gpx_kmat.hip")
    assert re.findall(r"__global__[^;{]*?\bvoid\s+(\w+)\s*\(", kmat) == ["kmat_kernel", "scale_points_kernel", "tile_reduce_kernel", "rect_tile_kernel",
                                                                         "tile_reduce_ard_kernel"]
    for f in files:
        assert "rect_tile_ard" not in open(os.path.join(csrc, f)).read(), f
    assert len(re.findall(r"v \+= host\[", kmat)) == 1
    for f in ("gpx_kmat.hip", "gpx_deriv.hip", "gpx_stream.hip", "gpx_paths.hip"):
        assert "((red[0]" not in code(f), f
    # one partial-sum scratch for the streamed passes; the mean and the apply kernel have one launch site each, behind one
    # launcher that owns the slice plan, the scratch, the LDS limit and the slices' reduction
    stream = code("gpx_stream.hip")
    assert re.findall(r"static thread_local ThreadScratch (\w+);", stream) == ["g_partial_scr"]
    for k in ("stream_mean_kernel", "stream_apply_kernel", "apply_reduce_kernel", "pred_grad_kernel"):
        assert len(re.findall(r"hipLaunchKernelGGL\(\(%s<" % k, stream)) == 1, k
    assert len(re.findall(r"\bslice_plan\(", stream)) == 3          # the definition, the apply launcher, pred_grad
    for f in files:
        assert not re.search(r"\b(?:mean_kernel|kapply_fused_kernel|g_mean_scr|g_pgrad_scr)\b", code(f)), f


def test_small_device_kernels_have_one_home():
    """The element maps, the transposes and the single-workgroup sums were copied from file to file with every feature: ten
    2-D maps with the same grid recipe, seven 1-D ones, three kernels called transpose_kernel, a second copy of the
    single-workgroup sum, and the two-armed dtype dispatch in front of each.  They are now lambdas behind the two map
    kernels of csrc/gpx_small.h, one transpose and one reduce_kernel in csrc/gpx_small.hip, and by_dtype; a new small
    kernel that brings its own copy of either recipe back fails here.  (The files the consolidation left alone, and
    gpx_potrf.hip, which only lost tril, still write the dispatch out.)"""
    csrc = os.path.join(ROOT, "gaussian_processes_amd", "csrc")
    files = [f for f in sorted(os.listdir(csrc)) if f.endswith((".hip", ".h"))]
    src = {f: open(os.path.join(csrc, f)).read() for f in files}
    assert "gpx_small.h" in files and "gpx_small.hip" in files

    def defs(name):
        return {f: n for f, n in ((f, len(re.findall(r"__global__(?:\s+__launch_bounds__\([^)]*\))?\s+void\s+%s\s*\(" % name, src[f]))) for f in files) if n}
    assert defs("transpose_kernel") == {"gpx_small.hip": 1}
    assert defs("map_rows_kernel") == {"gpx_small.h": 1}
    assert defs("map_vec_kernel") == {"gpx_small.h": 1}
    assert defs("reduce_kernel") == {"gpx_small.hip": 1}
    gone = ("cvt_from_f64_2d", "cvt_to_f64_2d", "eye_kernel", "eye_rows_kernel", "col_scale_kernel", "loo_g_kernel", "fill_rows_kernel",
            "paths_rows_kernel", "sum_slices_lower_kernel", "schur_reduce_kernel", "scale_copy_kernel", "sub_kernel", "cvt_div_kernel",
            "div_kernel", "paths_div_kernel", "add_diag_kernel", "loo_weights_kernel", "strided_sum_kernel", "transpose_sq")
    for f in files:
        for name in gone:
            assert not re.search(r"\b%s\b" % name, src[f]), (f, name)
    untouched = ("gpx_gemm.hip", "gpx_panel.hip", "gpx_leaf.h", "gpx_stream.hip", "gpx_kernels_dev.h", "gpx_mg.hip",
                 "gpx_runtime.hip", "gpx_potrf.hip")
    for f in files:
        if f not in untouched:
            for line in src[f].splitlines():
                assert not re.search(r"== GPX_F64\)\s*hipLaunchKernelGGL", line), (f, line)


def test_no_cpu_fallback_without_gpu():
    if _lib.device_count() > 0:
        pytest.skip("a GPU is present")
    k = gp.GaussianKernel(1, 1)
    with pytest.raises(_lib.GpxError):
        k(np.zeros(3), np.zeros(3))
    with pytest.raises(_lib.GpxError):
        make_gp().log_lh


def test_product_path_never_imports_oracle():
    pkg = os.path.join(ROOT, "gaussian_processes_amd")
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".hip", ".h")):
                src = open(os.path.join(dirpath, f)).read()
                assert "oracle" not in src.replace("the oracle's", ""), os.path.join(dirpath, f)


@pytest.mark.parametrize("cls,good", [(gp.GaussianKernel, (0.7, 1.3)), (gp.PeriodicKernel, (0.7, 1.3, 2.0))])
def test_kernel_params_and_validation(cls, good):
    k = cls(*good)
    assert (k.params == np.array(good)).all()
    assert k.params.dtype == np.float64
    k.params = good
    assert (k.params == np.array(good)).all()
    for i in range(len(good)):
        bad = list(good)
        bad[i] = 0
        with pytest.raises(ValueError):
            cls(*bad)
        with pytest.raises(ValueError):
            k.params = bad
    with pytest.raises(ValueError):
        k.set_param("nope", 1.0)
    assert type(k.h) is np.float64


def test_kernel_copy_pickle():
    k1 = gp.GaussianKernel(0.3, 0.9)
    for k2 in (k1.copy(), copy(k1), deepcopy(k1), pickle.loads(pickle.dumps(k1))):
        assert k1.h == k2.h and k1.w == k2.w and k1 is not k2
    k3 = deepcopy(k1)
    assert k1.h is not k3.h
    p1 = gp.PeriodicKernel(0.3, 0.9, 1.7)
    p2 = pickle.loads(pickle.dumps(p1))
    assert (p1.params == p2.params).all()


def test_kernel_buffer_errors():
    from gaussian_processes_amd.ext import gaussian_c
    x = np.linspace(0, 1, 4)
    out = np.empty((4, 4))
    with pytest.raises(ValueError, match="dtype mismatch"):
        gaussian_c.K(out, x.astype(np.float32), x, 1.0, 1.0)
    with pytest.raises(ValueError, match="not C-contiguous"):
        gaussian_c.K(np.empty((4, 8))[:, ::2], x, x, 1.0, 1.0)
    with pytest.raises(ValueError, match="wrong number of dimensions"):
        gaussian_c.K(out, x[:, None], x, 1.0, 1.0)
    with pytest.raises(ValueError, match="shape"):
        gaussian_c.K(np.empty((4, 5)), x, x, 1.0, 1.0)


def test_gp_inputs_are_readonly_float64_copies():
    x, y = make_xy()
    g = gp.GP(gp.GaussianKernel(1, 1), x, y, s=1)
    assert g.x.dtype == np.float64 and g.y.dtype == np.float64 and type(g.s) is np.float64
    assert g.x is not x and not g.x.flags.writeable and not g.y.flags.writeable
    assert g.params.dtype == np.float64 and (g.params == [1, 1, 1]).all()


def test_set_y_shape_and_negative_s():
    g = make_gp()
    with pytest.raises(ValueError):
        g.y = g.y.copy()[:, None]
    x, y = make_xy()
    with pytest.raises(ValueError):
        gp.GP(gp.GaussianKernel(1, 1), x, y, s=-1)


def test_reset_memoized_on_any_setter():
    g = make_gp()
    for prop, val in (("x", g.x.copy() + 1), ("y", g.y.copy() + 1), ("s", g.s + 1),
                      ("params", g.params + 1)):
        g._memoized["sentinel"] = 1
        setattr(g, prop, val)
        assert g._memoized == {}


def test_memoprop_del():
    g = make_gp()
    g._memoized["Kxx"] = "cached"
    assert g.Kxx == "cached"
    del g.Kxx
    assert "Kxx" not in g._memoized


def test_set_params_and_unknown_name():
    g = make_gp()
    g.set_param("h", 1)
    g.set_param("w", 0.2)
    g.set_param("s", 0.01)
    assert g.get_param("w") == 0.2 and g.get_param("s") == 0.01
    with pytest.raises(AttributeError):
        g.set_param("p", 1.1)


def test_copy_semantics():
    g1 = make_gp()
    for g2 in (g1.copy(deep=False), copy(g1)):
        assert g1 is not g2 and g1._x is g2._x and g1._y is g2._y and g1._s is g2._s and g1.K is g2.K
    for g2 in (g1.copy(deep=True), deepcopy(g1), pickle.loads(pickle.dumps(g1))):
        assert g1 is not g2 and g1._x is not g2._x and g1._y is not g2._y and g1.K is not g2.K
        assert g1._s is not g2._s
        assert (g1._x == g2._x).all() and (g1._y == g2._y).all() and g1._s == g2._s
        assert (g1.K.params == g2.K.params).all()


def test_pickle_carries_memoized_host_arrays():
    g1 = make_gp()
    g1._memoized["Kxx"] = np.eye(16)
    g2 = pickle.loads(pickle.dumps(g1))
    assert (g2._memoized["Kxx"] == np.eye(16)).all()


def test_nd_inputs_accepted():
    X = np.random.RandomState(0).randn(10, 3)
    g = gp.GP(gp.GaussianKernel(1, 1), X, np.zeros(10), s=1)
    assert g._n == 10 and g._d == 3
    with pytest.raises(ValueError):
        gp.GP(gp.GaussianKernel(1, 1), X, np.zeros((10, 3)), s=1)


# ---- bench.py as the driver calls it: `python bench.py --gpus P` must start P ranks itself ----
def _run_bench(*argv):
    import subprocess
    import sys
    env = dict(os.environ)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    return subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + list(argv), env=env,
                          stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)


def test_bench_self_launches_ranks_from_a_plain_invocation():
    import json
    r = _run_bench("--gpus", "2", "--launch-check")
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, r.stdout                      # exactly ONE JSON line on stdout
    out = json.loads(lines[0])
    assert out["n_gpus"] == 2 and out["launch_check"] is True and out["rank_sum"] == 3.0


def test_bench_self_launch_propagates_a_rank_failure():
    # without a GPU the ranks refuse to run (no CPU fallback): the launcher must exit non-zero
    # and print no result line
    from gaussian_processes_amd import _lib
    if _lib.device_count() >= 1:
        pytest.skip("a GPU is present: the ranks would run")
    r = _run_bench("--gpus", "2", "--problem-n", "512", "--no-cpu-baseline")
    assert r.returncode != 0
    assert not [ln for ln in r.stdout.splitlines() if ln.startswith("{")]


def test_pickled_state_has_exactly_the_reference_keys():
    # gp/gp.py:78-92: K, _x, _y, _s, _memoized -- nothing else for a GP built the reference's way
    g = make_gp()
    assert sorted(g.__getstate__()) == ["K", "_memoized", "_s", "_x", "_y"]
    g2 = pickle.loads(pickle.dumps(g))
    assert g2._dtype == g._dtype and g2._device is None
    # the opt-in extensions (fp32 device path, explicit device) survive a round trip
    x, y = make_xy()
    g32 = gp.GP(gp.GaussianKernel(1, 1), x, y, s=1, dtype="float32", device=0)
    g3 = pickle.loads(pickle.dumps(g32))
    assert g3._dtype == _lib.F32 and g3._device == 0
