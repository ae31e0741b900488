// wt_cover.hip -- coverage and union of overlapping intervals on the device: the reference's CoverageWiggleIterator
// (src/unaryOps.c:303-375, the `coverage` command) and UnionWiggleIterator (:60-92) over whole run lists in HBM.  The passes
// and the two doors are written once in csrc/wt_cover.h (which tests/cover_emu.cpp also compiles for the CPU); this unit
// gives every pass its kernel; the launcher of the doors, the report of their result and the staging of the *_host entry are
// those of csrc/wt_runs_host.h, with memory from hipMalloc.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdlib>
#include <string>
#include <vector>

#include "wt_runs_host.h"

namespace {

template <int K>
__global__ void __launch_bounds__(WCV_BLOCK) wt_cover_kernel(WcvArgs a) {
    __shared__ WcvLds lds;
    wcv_run_block(K, a, (long long) blockIdx.x, &lds);
}

struct HipLauncher : WtRunsLauncher {
    template <int K> bool launch(long long blocks, const WcvArgs &a) { return WtRunsLauncher::launch(wt_cover_kernel<K>, WCV_BLOCK, blocks, a); }
    bool run(int kernel, long long blocks, const WcvArgs &a) {
        switch (kernel) {
        case WCV_K_PRE: return launch<WCV_K_PRE>(blocks, a);
        case WCV_K_MARK: return launch<WCV_K_MARK>(blocks, a);
        case WCV_K_RANK: return launch<WCV_K_RANK>(blocks, a);
        case WCV_K_SCAN_SUM: return launch<WCV_K_SCAN_SUM>(blocks, a);
        case WCV_K_DELTA: return launch<WCV_K_DELTA>(blocks, a);
        case WCV_K_DSUM: return launch<WCV_K_DSUM>(blocks, a);
        case WCV_K_DEPTH: return launch<WCV_K_DEPTH>(blocks, a);
        case WCV_K_EMIT: return launch<WCV_K_EMIT>(blocks, a);
        case WCV_K_SEGOFF: return launch<WCV_K_SEGOFF>(blocks, a);
        case WCV_K_UKEY: return launch<WCV_K_UKEY>(blocks, a);
        case WCV_K_SCAN_MAX: return launch<WCV_K_SCAN_MAX>(blocks, a);
        case WCV_K_UPM: return launch<WCV_K_UPM>(blocks, a);
        case WCV_K_UHEAD: return launch<WCV_K_UHEAD>(blocks, a);
        case WCV_K_UEMIT: return launch<WCV_K_UEMIT>(blocks, a);
        default: return false;
        }
    }
};

long long wcv_budget() {
    const char *e = getenv("WTAMD_COVER_SCRATCH_MB");
    const long long mb = e && atoll(e) > 0 ? atoll(e) : 256;
    return mb << 20;
}

}  // namespace

// one pass of wt_cover.h on a stream, for the other units that use them (csrc/wt_region.hip: the union of a mask, the scan)
bool wt_cover_run(void *stream, int kernel, long long blocks, const WcvArgs &a) {
    HipLauncher l{{(hipStream_t) stream, nullptr}};
    return l.run(kernel, blocks, a);
}

extern "C" {

int wtamd_runs_coverage_flags(int64_t n_seg, const int64_t *seg_off, const int32_t *start, const int32_t *finish, int64_t capacity,
                              int32_t *o_start, int32_t *o_finish, double *o_value, int64_t *o_seg_off, int64_t *n_out, uint32_t flags,
                              void *stream) {
    HipLauncher l{{(hipStream_t) stream, nullptr}};
    const char *why = "";
    const int rc = wcv_coverage_flags(l, (long long) n_seg, seg_off, start, finish, (long long) capacity, o_start, o_finish, o_value,
                                      o_seg_off, n_out, wcv_budget(), flags, &why);
    return wt_runs_report(flags ? "wtamd_runs_coverage_flags" : "wtamd_runs_coverage", rc, why);
}

int wtamd_runs_coverage(int64_t n_seg, const int64_t *seg_off, const int32_t *start, const int32_t *finish, int64_t capacity,
                        int32_t *o_start, int32_t *o_finish, double *o_value, int64_t *o_seg_off, int64_t *n_out, void *stream) {
    return wtamd_runs_coverage_flags(n_seg, seg_off, start, finish, capacity, o_start, o_finish, o_value, o_seg_off, n_out, 0u, stream);
}

int wtamd_runs_union(int64_t n_seg, const int64_t *seg_off, const int32_t *start, const int32_t *finish, const void *value,
                     int value_is_f64, int64_t capacity, int32_t *o_start, int32_t *o_finish, double *o_value, int64_t *o_seg_off,
                     int64_t *n_out, void *stream) {
    HipLauncher l{{(hipStream_t) stream, nullptr}};
    const char *why = "";
    const int rc = wcv_union(l, (long long) n_seg, seg_off, start, finish, value, value_is_f64, (long long) capacity, o_start, o_finish,
                             o_value, o_seg_off, n_out, &why);
    return wt_runs_report("wtamd_runs_union", rc, why);
}

// One segment in HOST memory in, its depth track in HOST memory out (what wtamd_CoverageIterator calls per chromosome).
int wtamd_runs_coverage_host_flags(int64_t n, const int32_t *start, const int32_t *finish, int64_t capacity, int32_t *o_start,
                                   int32_t *o_finish, double *o_value, int64_t *n_out, uint32_t flags) {
    if (n < 0 || !n_out || (n > 0 && (!start || !finish))) return wt_fail(WTAMD_ERR_ARG, "wtamd_runs_coverage_host: bad argument");
    *n_out = 0;
    if (n == 0) return WTAMD_OK;
    const int64_t cap = 2 * n - 1;
    HipLauncher l{{nullptr, nullptr}};
    WcvScope<HipLauncher> sc(l);
    WtDevRuns in;
    int32_t *d_out = nullptr;
    double *d_val = nullptr;
    if (const int e = wt_stage_runs("wtamd_runs_coverage_host", sc, n, start, finish, nullptr, false, &in)) return e;
    if (!sc.get(&d_out, 2 * (size_t) cap) || !sc.get(&d_val, (size_t) cap))
        return wt_fail(WTAMD_ERR_HIP, "wtamd_runs_coverage_host: out of device memory");
    const int64_t seg[2] = {0, n};
    int64_t oseg[2] = {0, 0};
    const int rc = wtamd_runs_coverage_flags(1, seg, in.start, in.finish, cap, d_out, d_out + cap, d_val, oseg, n_out, flags, nullptr);
    if (rc != WTAMD_OK) return rc;
    if (*n_out > capacity) return wt_fail(WTAMD_ERR_CAPACITY, "wtamd_runs_coverage_host: the output arrays are too small (*n_out holds the count needed)");
    if (*n_out > 0) {
        WT_HIP(hipMemcpy(o_start, d_out, sizeof(int32_t) * (size_t) *n_out, hipMemcpyDeviceToHost));
        WT_HIP(hipMemcpy(o_finish, d_out + cap, sizeof(int32_t) * (size_t) *n_out, hipMemcpyDeviceToHost));
        WT_HIP(hipMemcpy(o_value, d_val, sizeof(double) * (size_t) *n_out, hipMemcpyDeviceToHost));
    }
    return WTAMD_OK;
}

int wtamd_runs_coverage_host(int64_t n, const int32_t *start, const int32_t *finish, int64_t capacity, int32_t *o_start,
                             int32_t *o_finish, double *o_value, int64_t *n_out) {
    return wtamd_runs_coverage_host_flags(n, start, finish, capacity, o_start, o_finish, o_value, n_out, 0u);
}

}  // extern "C"
