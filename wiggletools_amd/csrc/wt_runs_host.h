// wt_runs_host.h -- what the host sides of the run-list doors' units share (csrc/wt_cover.hip, wt_region.hip, wt_apply.hip,
// wt_profile.hip): the launcher the doors of wt_cover.h / wt_region.h / wt_apply.h / wt_profile.h are written over, the report of
// a door's result, and the staging of a host run list for the *_host entry points.  A unit adds its kernel template, the
// switch from pass number to instantiation, and its run_* member.
#ifndef WT_RUNS_HOST_H_
#define WT_RUNS_HOST_H_

#include <string>

#include "wt_host.h"
#include "wt_pool.h"
#include "wt_cover.h"

// one pass of wt_cover.h on a stream (csrc/wt_cover.hip), for the units that use them: the union of a mask, the scans
bool wt_cover_run(void *stream, int kernel, long long blocks, const WcvArgs &a);

struct WtRunsLauncher {
    hipStream_t s;
    const char *pool;           // the unit's name (for WTAMD_TRACE_POOL=1): temporary device memory comes from the pool (wt_pool.h);
                                // NULL: from hipMalloc / hipFree
    bool quiet = false;         // nothing has been put on `s` since it was last waited for, and only `s` touches the buffers: they may
                                // return to the pool without the device-wide wait
    void *alloc(size_t bytes) {
        void *p = nullptr;
        return (pool ? wt_dev_alloc_bytes(&p, bytes, pool, __LINE__) : hipMalloc(&p, bytes)) == hipSuccess ? p : nullptr;
    }
    void release(void *p) {
        if (!pool) { (void) hipFree(p); return; }
        if (!quiet) { (void) wt_pool_quiesce(); quiet = true; }
        (void) wt_dev_free(p);
    }
    bool zero(void *p, size_t bytes) { quiet = false; return hipMemsetAsync(p, 0, bytes, s) == hipSuccess; }
    bool sync() { return quiet = hipStreamSynchronize(s) == hipSuccess; }
    bool to_host(void *h, const void *d, size_t bytes) {
        return hipMemcpyAsync(h, d, bytes, hipMemcpyDeviceToHost, s) == hipSuccess && sync();
    }
    bool to_device(void *d, const void *h, size_t bytes) {
        // (the host tables are reused by the caller: the copy has left them when this returns)
        return hipMemcpyAsync(d, h, bytes, hipMemcpyHostToDevice, s) == hipSuccess && sync();
    }
    bool run(int kernel, long long blocks, const WcvArgs &a) { quiet = false; return wt_cover_run((void *) s, kernel, blocks, a); }
    template <class Args> bool launch(void (*kernel)(Args), int threads, long long blocks, const Args &a) {
        if (blocks <= 0) return true;
        if (blocks > 0x7fffffffll) return false;
        quiet = false;
        hipLaunchKernelGGL(kernel, dim3((unsigned) blocks), dim3((unsigned) threads), 0, s, a);
        return hipGetLastError() == hipSuccess;
    }
};

// a door's return value (0 fine, 1 bad argument, 2 launcher failure, 3 capacity) as the WTAMD_* code, recorded for wtamd_last_error
static inline int wt_runs_report(const char *door, int rc, const char *why) {
    if (rc == 0) return WTAMD_OK;
    if (rc == 3) return wt_fail(WTAMD_ERR_CAPACITY, std::string(door) + ": the output arrays are too small (*n_out holds the count needed)");
    if (rc == 1) return wt_fail(WTAMD_ERR_ARG, std::string(door) + ": " + why);
    const hipError_t e = hipGetLastError();
    return wt_fail(WTAMD_ERR_HIP, std::string(door) + ": " + why + " (" + hipGetErrorString(e) + ")");
}

// A run list in HOST memory, staged for a door by a *_host entry point: [2 max(n, 1)] int32 (the starts, then the finishes)
// and, with_value, [max(n, 1)] doubles, out of `sc`; hipMemcpy, so the host arrays are free at once.
struct WtDevRuns {
    int32_t *start = nullptr, *finish = nullptr;
    double *value = nullptr;
};

template <class Scope>
static inline int wt_stage_runs(const char *door, Scope &sc, int64_t n, const int32_t *start, const int32_t *finish, const double *value,
                                bool with_value, WtDevRuns *d) {
    const size_t n1 = (size_t) (n > 0 ? n : 1);
    if (!sc.get(&d->start, 2 * n1) || (with_value && !sc.get(&d->value, n1))) return wt_fail(WTAMD_ERR_HIP, std::string(door) + ": out of device memory");
    d->finish = d->start + n1;
    if (n > 0) {
        WT_HIP(hipMemcpy(d->start, start, sizeof(int32_t) * (size_t) n, hipMemcpyHostToDevice));
        WT_HIP(hipMemcpy(d->finish, finish, sizeof(int32_t) * (size_t) n, hipMemcpyHostToDevice));
        if (with_value) WT_HIP(hipMemcpy(d->value, value, sizeof(double) * (size_t) n, hipMemcpyHostToDevice));
    }
    return WTAMD_OK;
}

#endif  // WT_RUNS_HOST_H_
