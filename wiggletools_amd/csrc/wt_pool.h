// wt_pool.h -- the two process-wide pools of the library (defined once, in wt_pool.hip): page-locked host memory and device
// buffers, kept when their user lets go of them and handed to the next one that asks for the same size.  The pipes
// (wt_pipe.hip), the engine's track sets and window tables (wt_engine.hip) and the temporary buffers of a host entry point
// (wt_devscope.h) draw on the same instance; wtamd_pool_stats / wtamd_pool_trim cover them all.
//
// THE RULE: the pools wait for nothing, so a buffer returns to a pool only after the device has finished with it.  Whoever
// returns buffers waits first (wt_pool_quiesce, or a synchronisation of every stream that touched them) -- once for all the
// buffers it is about to return, not per buffer: wtamd_trackset_destroy, WtDevScope's destructor, once per growth of a table.
#ifndef WT_POOL_H_
#define WT_POOL_H_

#include "wt_host.h"

// Page-locked (hipHostMalloc / hipHostRegister) host memory is readable by kernels; pageable memory
// is not -- such ranges go through hipMemcpyAsync, which stages them.
bool wt_is_pinned(const void *q);

// sizes as the pools see them: multiples of 256 bytes below 1 MB, eighths of their power of two from there
size_t wt_pool_round(size_t bytes);

// page-locked host memory, from the pool where a buffer of the size rests
hipError_t wt_host_alloc(void **out, size_t bytes);
void wt_host_free(void *q);

// device memory of the current device, the same way (file / line: the caller, for WTAMD_TRACE_POOL=1)
hipError_t wt_dev_alloc_bytes(void **out, size_t bytes, const char *file, int line);
template <class T>
static inline hipError_t wt_dev_alloc(T **out, size_t bytes, const char *file = __builtin_FILE(), int line = __builtin_LINE()) {
    void *q = nullptr;
    const hipError_t e = wt_dev_alloc_bytes(&q, bytes, file, line);
    *out = (T *) q;
    return e;
}
hipError_t wt_dev_free(void *q);

// the wait THE RULE asks for where the streams that used the buffers are not known: for the whole device
hipError_t wt_pool_quiesce();

#endif  // WT_POOL_H_
