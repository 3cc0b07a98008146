"""CPU tests of multi_gpu.HostStagedCallbacks, the host-staged data plane GlooCallbacks and the tests' ThreadCallbacks
share: what it stages around the exchange hooks, and what becomes of an exception inside one.  "Device" memory is a
numpy array here, and the three library calls of the staging are host copies."""
import ctypes

import numpy as np

from gaussian_processes_amd import _lib, multi_gpu


class _HostLib(object):
    """gpx_stream_sync / gpx_memcpy_d2h / gpx_memcpy_h2d over host memory, with a log of the calls."""

    def __init__(self):
        self.calls = []

    def gpx_stream_sync(self, stream):
        self.calls.append(("sync", stream))
        return 0

    def _copy(self, what, dst, src, nbytes, stream):
        self.calls.append((what, int(nbytes), stream))
        ctypes.memmove(dst, src, nbytes)
        return 0

    def gpx_memcpy_d2h(self, dst, src, nbytes, stream):
        return self._copy("d2h", dst, src, nbytes, stream)

    def gpx_memcpy_h2d(self, dst, src, nbytes, stream):
        return self._copy("h2d", dst, src, nbytes, stream)


class _ListCallbacks(multi_gpu.HostStagedCallbacks):
    """The exchange through a Python list: slot r holds what rank r staged last."""

    def __init__(self, board, rank, lib, explode=None):
        multi_gpu.HostStagedCallbacks.__init__(self, rank, len(board))
        self.board, self.lib, self.explode, self.failed = board, lib, explode, []

    def rank_failed(self, exc):
        self.failed.append(exc)

    def exchange_bcast(self, buf, root):
        if self.explode:
            raise self.explode
        if self.rank == root:
            self.board[root] = buf
        return self.board[root]

    def exchange_allreduce(self, buf, op):
        if self.explode:
            raise self.explode
        self.board[self.rank] = buf
        acc = self.board[0].copy()
        for other in self.board[1:]:
            acc = acc + other if op == 0 else np.maximum(acc, other)
        return acc


def _addr(a):
    return a.ctypes.data


def test_broadcast_stages_the_roots_bytes_and_only_them():
    board, lib = [None, None], _HostLib()
    ranks = [_ListCallbacks(board, r, lib) for r in range(2)]
    dev = [np.arange(24, dtype=np.float32), np.full(24, -1.0, dtype=np.float32)]
    keep = dev[1].copy()
    stream = 0x1234
    # root = 1: the root stages its device bytes out and leaves its own memory alone
    assert ranks[1].bcast(None, _addr(dev[1]), dev[1].nbytes, 1, stream) == 0
    assert board[1].dtype == np.uint8 and board[1].tobytes() == keep.tobytes()
    assert lib.calls == [("sync", stream), ("d2h", 96, stream)]
    # ... and the other rank stages them in, after waiting for its stream, without reading its own memory
    del lib.calls[:]
    assert ranks[0].bcast(None, _addr(dev[0]), dev[0].nbytes, 1, stream) == 0
    assert lib.calls == [("sync", stream), ("h2d", 96, stream)]
    assert np.array_equal(dev[0], keep) and np.array_equal(dev[1], keep)
    assert ranks[0].error is None and ranks[1].error is None and not ranks[0].failed


def test_allreduce_stages_every_dtype_out_and_the_result_in():
    for dtype_id, npdt in ((_lib.F64, np.float64), (_lib.F32, np.float32), (2, np.int32)):
        for op in (0, 1):
            vals = [np.array([1, 5, -3, 7], dtype=npdt), np.array([2, -4, 9, 7], dtype=npdt)]
            want = vals[0] + vals[1] if op == 0 else np.maximum(vals[0], vals[1])
            board, lib = [None, vals[1].copy()], _HostLib()          # (rank 1 has posted its values already)
            cb = _ListCallbacks(board, 0, lib)
            dev = vals[0].copy()
            assert cb.allreduce(None, _addr(dev), dev.size, dtype_id, op, None) == 0
            assert board[0].dtype == npdt and np.array_equal(board[0], vals[0])     # what was staged out
            assert dev.dtype == npdt and np.array_equal(dev, want)                  # what was staged in
            assert lib.calls == [("sync", None), ("d2h", dev.nbytes, None), ("h2d", dev.nbytes, None)]


def test_an_exception_in_a_hook_comes_back_as_return_code_1_with_the_error_kept():
    boom = RuntimeError("the transport is gone")
    cb = _ListCallbacks([None, None], 0, _HostLib(), explode=boom)
    dev = np.zeros(4)
    keep = dev.copy()
    assert cb.bcast(None, _addr(dev), dev.nbytes, 1, None) == 1
    assert cb.error is boom and cb.failed == [boom]
    cb.error = None
    assert cb.allreduce(None, _addr(dev), dev.size, _lib.F64, 0, None) == 1
    assert cb.error is boom and cb.failed == [boom, boom]
    assert np.array_equal(dev, keep)                                 # nothing was staged in
    # an unknown dtype is an error of the callback too, not an exception through the C frames
    cb2 = _ListCallbacks([None, None], 0, _HostLib())
    assert cb2.allreduce(None, _addr(dev), dev.size, 99, 0, None) == 1
    assert isinstance(cb2.error, KeyError) and len(cb2.failed) == 1
