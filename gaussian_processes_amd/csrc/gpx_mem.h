// gpx_mem.h -- every way libgpx.so owns device memory.  Included by gpx_common.h, behind the error
// macros it uses; no other file of the library calls the HIP allocator (gpx_malloc / gpx_free of the ABI aside:
// that memory is the caller's).
//
//   dev_alloc / dev_free   fixed-size fields of a handle, sized at creation and freed by its destroy
//   DevBuf                 a temporary of one call, freed on scope exit
//   GrowBuf                a grow-only block with ONE owner: a handle (fit_batch's workspaces, sag_tmp), a factor (the
//                          TrsvOps below) or, through ThreadScratch, a host thread on one device
//   ThreadScratch          one GrowBuf per device for the calling host thread
//   Carve                  the byte layout of ONE block that holds several arrays: a pass declares it once, in a function
//                          that returns its offsets and the total; the allocation takes the total, the pointers the offsets
//
// Every request is passed to hipMalloc byte for byte: nothing is rounded up, pooled or kept for a later caller.
#pragma once

namespace gpx {

inline int dev_alloc(void **p, size_t bytes, const char *what = "hipMalloc")
{
    hipError_t e = hipMalloc(p, bytes);
    if (e != hipSuccess) { *p = nullptr; return hip_fail(e, what, __FILE__, __LINE__); }
    return GPX_OK;
}
inline void dev_free(void *p) { if (p) (void)hipFree(p); }

struct DevBuf {
    void *p = nullptr;
    ~DevBuf() { dev_free(p); }
    int alloc(size_t bytes) { return dev_alloc(&p, bytes ? bytes : 16); }
};

// Grow-only: a request the block already covers costs nothing; a larger one waits for the work that may still use the
// old block, frees it and allocates exactly the new size.  All-zero memory is a valid empty GrowBuf (gpx_gp_create clears
// its handle with memset), and there is no destructor: owners call release(), views (a TrsvOps over a slice of somebody
// else's block, fit_batch_grad) and thread-local scratch never do.
struct GrowBuf {
    void *p = nullptr; size_t bytes = 0;
    // `st`: the one stream whose work uses the block; *grew (optional): the block was replaced, its contents are gone
    int reserve(size_t need, hipStream_t st, bool *grew = nullptr)
    {
        if (grew) *grew = false;
        if (p && bytes >= need) return GPX_OK;
        if (p) GPX_HIP(hipStreamSynchronize(st));
        return replace(need, grew);
    }
    // the same when any stream of the device may still be using the block
    int reserve_device(size_t need, bool *grew = nullptr)
    {
        if (grew) *grew = false;
        if (p && bytes >= need) return GPX_OK;
        if (p) GPX_HIP(hipDeviceSynchronize());
        return replace(need, grew);
    }
    void release() { dev_free(p); p = nullptr; bytes = 0; }

private:
    int replace(size_t need, bool *grew)
    {
        release();                       // (a failed allocation leaves an EMPTY block, never a stale size)
        GPX_TRY(dev_alloc(&p, need));
        bytes = need;
        if (grew) *grew = true;
        return GPX_OK;
    }
};

// A bump carver over byte offsets: take() returns where the next sub-block starts, total() the size of them all.  No
// memory is touched, so a layout is a constexpr function of the shapes and can be asserted at compile time.
struct Carve {
    size_t end = 0;
    constexpr size_t take(size_t bytes, size_t align = 128) { const size_t at = (end + align - 1) / align * align; end = at + bytes; return at; }
    constexpr size_t total() const { return end; }
};
struct CarveCheck { size_t a, b, c, total; };
constexpr CarveCheck carve_check() { Carve k; CarveCheck l{}; l.a = k.take(100); l.b = k.take(8, 256); l.c = k.take(24); l.total = k.total(); return l; }
static_assert(carve_check().a == 0 && carve_check().b == 256 && carve_check().c == 384, "Carve: offsets ascend, each on its alignment");
static_assert(carve_check().b >= carve_check().a + 100 && carve_check().c >= carve_check().b + 8, "Carve: sub-blocks do not overlap");
static_assert(carve_check().total == carve_check().c + 24, "Carve: the total is the last offset plus its size");

// One slot per device for per-thread state (`static thread_local PerDevice<...>`): a host thread that alternates between
// GPUs finds each device's slot again, and no block is dropped unfreed.  HIP's current device is per host thread, and
// every handle entry makes its device current first (DeviceGuard).  Thread-local blocks are NOT freed at thread or
// process exit: a hipFree from a destructor may run while the runtime is shutting down.
constexpr int MAX_DEVICES = 16;
template <typename Slot>
struct PerDevice {
    Slot slot[MAX_DEVICES];
    int current(Slot **out)
    {
        int dev = 0;
        GPX_HIP(hipGetDevice(&dev));
        if (dev < 0 || dev >= MAX_DEVICES) { set_error("device index %d out of range (per-thread scratch)", dev); return GPX_ERR_ARG; }
        *out = &slot[dev];
        return GPX_OK;
    }
};

// Everything a host thread enqueues through this library shares that thread's grow-only scratch buffers (block inverses and
// operators of the solves, the panels' hand-off blocks, reduction scratch ...).  Calls on ONE stream are ordered by the stream;
// a call on ANOTHER stream first waits for the work of the call before it: handles fitted asynchronously back to back from
// one thread (each on its own stream) would otherwise race on those buffers (seen once as a wrong log_lh in the four-handle
// test of tests/test_gpu_configs.py, when faster panels changed the overlap).  One event record per API call; nothing is
// recorded or waited for while a stream is being captured.
void stream_epoch_bump();          // call before destroying any stream (see TurnState, gpx_runtime.hip)
struct StreamTurn {
    hipStream_t st;
    explicit StreamTurn(hipStream_t s);
    ~StreamTurn();
};

// The scratch itself.  Growing waits for the whole device: the old block may be in use on any stream this thread drove.
struct ThreadScratch : PerDevice<GrowBuf> {
    int get(size_t bytes, void **out)
    {
        GrowBuf *b = nullptr;
        GPX_TRY(current(&b));
        GPX_TRY(b->reserve_device(bytes));
        *out = b->p;
        return GPX_OK;
    }
};

}  // namespace gpx
