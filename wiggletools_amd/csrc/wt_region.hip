// wt_region.hip -- the reference's region operators on the device: OverlapWiggleIterator, NoverlapWiggleIterator,
// TrimWiggleIterator and NearestWiggleIterator (src/unaryOps.c:437-639; `overlaps`, `noverlaps`, `trim`, `nearest`) over whole
// run lists in HBM.  The passes and the door are written once in csrc/wt_region.h (which tests/region_emu.cpp also compiles
// for the CPU); this unit gives every pass its kernel; the launcher of the door, the report of its result and the staging of
// the *_host entry are those of csrc/wt_runs_host.h, with memory from hipMalloc.  The union of the mask and the scan of the
// tile counts are passes of csrc/wt_cover.h, launched by csrc/wt_cover.hip (wt_cover_run).
#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>
#include <vector>

#include "wt_runs_host.h"
#include "wt_region.h"

namespace {

template <int K>
__global__ void __launch_bounds__(WRG_BLOCK) wt_region_kernel(WrgArgs a) {
    __shared__ WrgLds lds;
    wrg_run_block(K, a, (long long) blockIdx.x, &lds);
}

struct HipRegionLauncher : WtRunsLauncher {
    template <int K> bool launch(long long blocks, const WrgArgs &a) { return WtRunsLauncher::launch(wt_region_kernel<K>, WRG_BLOCK, blocks, a); }
    bool run_region(int kernel, long long blocks, const WrgArgs &a) {
        switch (kernel) {
        case WRG_K_VALID: return launch<WRG_K_VALID>(blocks, a);
        case WRG_K_COUNT: return launch<WRG_K_COUNT>(blocks, a);
        case WRG_K_EMIT: return launch<WRG_K_EMIT>(blocks, a);
        default: return false;
        }
    }
};

}  // namespace

extern "C" {

int wtamd_runs_region(int op, int64_t n_seg, const int64_t *seg_off, const int32_t *start, const int32_t *finish, const void *value,
                      int value_is_f64, const int64_t *m_seg_off, const int32_t *m_start, const int32_t *m_finish, int64_t capacity,
                      int32_t *o_start, int32_t *o_finish, double *o_value, int64_t *o_seg_off, int64_t *n_out, void *stream) {
    static_assert(WRG_OVERLAPS == WTAMD_REGION_OVERLAPS && WRG_NOVERLAPS == WTAMD_REGION_NOVERLAPS && WRG_TRIM == WTAMD_REGION_TRIM &&
                  WRG_NEAREST == WTAMD_REGION_NEAREST, "wt_region.h and wiggletools_amd.h number the operators alike");
    HipRegionLauncher l{{(hipStream_t) stream, nullptr}};
    const char *why = "";
    const int rc = wrg_region(l, op, (long long) n_seg, seg_off, start, finish, value, value_is_f64, m_seg_off, m_start, m_finish,
                              (long long) capacity, o_start, o_finish, o_value, o_seg_off, n_out, &why);
    return wt_runs_report("wtamd_runs_region", rc, why);
}

// One segment of source and mask in HOST memory in, the result in HOST memory out (what wtamd_RegionIterator calls per
// chromosome).
int wtamd_runs_region_host(int op, int64_t n, const int32_t *start, const int32_t *finish, const double *value, int64_t m,
                           const int32_t *m_start, const int32_t *m_finish, int64_t capacity, int32_t *o_start, int32_t *o_finish,
                           double *o_value, int64_t *n_out) {
    if (n < 0 || m < 0 || capacity < 0 || !n_out || (n > 0 && (!start || !finish || !value)) || (m > 0 && (!m_start || !m_finish)) ||
        (capacity > 0 && (!o_start || !o_finish || !o_value)))
        return wt_fail(WTAMD_ERR_ARG, "wtamd_runs_region_host: bad argument");
    *n_out = 0;
    HipRegionLauncher l{{nullptr, nullptr}};
    WcvScope<HipRegionLauncher> sc(l);
    WtDevRuns in, mask;
    int32_t *d_out = nullptr;
    double *d_oval = nullptr;
    const size_t c1 = (size_t) (capacity > 0 ? capacity : 1);
    if (const int e = wt_stage_runs("wtamd_runs_region_host", sc, n, start, finish, value, true, &in)) return e;
    if (const int e = wt_stage_runs("wtamd_runs_region_host", sc, m, m_start, m_finish, nullptr, false, &mask)) return e;
    if (!sc.get(&d_out, 2 * c1) || !sc.get(&d_oval, c1)) return wt_fail(WTAMD_ERR_HIP, "wtamd_runs_region_host: out of device memory");
    const int64_t seg[2] = {0, n}, mseg[2] = {0, m};
    int64_t oseg[2] = {0, 0};
    const int rc = wtamd_runs_region(op, 1, seg, in.start, in.finish, in.value, 1, mseg, mask.start, mask.finish, capacity, d_out, d_out + c1, d_oval,
                                     oseg, n_out, nullptr);
    if (rc != WTAMD_OK) return rc;
    if (*n_out > 0) {
        WT_HIP(hipMemcpy(o_start, d_out, sizeof(int32_t) * (size_t) *n_out, hipMemcpyDeviceToHost));
        WT_HIP(hipMemcpy(o_finish, d_out + c1, sizeof(int32_t) * (size_t) *n_out, hipMemcpyDeviceToHost));
        WT_HIP(hipMemcpy(o_value, d_oval, sizeof(double) * (size_t) *n_out, hipMemcpyDeviceToHost));
    }
    return WTAMD_OK;
}

}  // extern "C"
