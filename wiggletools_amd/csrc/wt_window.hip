// wt_window.hip -- the window operators on the device: the reference's BinningWiggleIterator (src/unaryOps.c:963-1036, `bin`) and
// SmoothWiggleIterator (:1039-1162, `smooth`) over whole run lists in HBM.  The passes and the two doors are written once in
// csrc/wt_window.h (which tests/window_emu.cpp also compiles for the CPU); this unit gives every pass its kernel; the launcher
// of the doors, the report of their result and the staging of the *_host entries are those of csrc/wt_runs_host.h.  The scans of
// the workgroups' counts are a pass of csrc/wt_cover.h, launched by csrc/wt_cover.hip (wt_cover_run).  Temporary device memory
// comes from the pool (wt_pool.h).
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdlib>
#include <string>
#include <vector>

#include "wt_runs_host.h"
#include "wt_window.h"

namespace {

template <int K>
__global__ void __launch_bounds__(WWN_BLOCK) wt_window_kernel(WwnArgs a) {
    __shared__ WwnLds lds;
    wwn_run_block(K, a, (long long) blockIdx.x, &lds);
}

struct HipWindowLauncher : WtRunsLauncher {
    template <int K> bool launch(long long blocks, const WwnArgs &a) { return WtRunsLauncher::launch(wt_window_kernel<K>, WWN_BLOCK, blocks, a); }
    bool run_window(int kernel, long long blocks, const WwnArgs &a) {
        switch (kernel) {
        case WWN_K_VALID: return launch<WWN_K_VALID>(blocks, a);
        case WWN_K_COUNT: return launch<WWN_K_COUNT>(blocks, a);
        case WWN_K_CUM: return launch<WWN_K_CUM>(blocks, a);
        case WWN_K_BINS: return launch<WWN_K_BINS>(blocks, a);
        case WWN_K_HEAVY: return launch<WWN_K_HEAVY>(blocks, a);
        case WWN_K_ENDS: return launch<WWN_K_ENDS>(blocks, a);
        case WWN_K_SMOOTH: return launch<WWN_K_SMOOTH>(blocks, a);
        default: return false;
        }
    }
};

// One segment in HOST memory in, its result in HOST memory out: device memory from the pool, copies and the call on the null stream.
template <class Door>
int window_host(const char *name, int64_t n, const int32_t *start, const int32_t *finish, const double *value, int64_t capacity, int32_t *o_start,
                int32_t *o_finish, double *o_value, int64_t *n_out, Door door) {
    if (n < 0 || !n_out || capacity < 0 || (n > 0 && (!start || !finish || !value)) || (capacity > 0 && (!o_start || !o_finish || !o_value)))
        return wt_fail(WTAMD_ERR_ARG, std::string(name) + ": bad argument");
    HipWindowLauncher l{{nullptr, __FILE__}};
    WcvScope<HipWindowLauncher> sc(l);
    WtDevRuns in;
    int32_t *d_out = nullptr;
    double *d_val = nullptr;
    const size_t cap = (size_t) (capacity > 0 ? capacity : 1);
    if (const int e = wt_stage_runs(name, sc, n, start, finish, value, true, &in)) return e;
    if (!sc.get(&d_out, 2 * cap) || !sc.get(&d_val, cap)) return wt_fail(WTAMD_ERR_HIP, std::string(name) + ": out of device memory");
    const int64_t seg[2] = {0, n};
    int64_t oseg[2] = {0, 0};
    const int rc = door(seg, in, d_out, d_out + cap, d_val, oseg);
    if (rc != WTAMD_OK) return rc;
    if (*n_out > 0) {
        WT_HIP(hipMemcpy(o_start, d_out, sizeof(int32_t) * (size_t) *n_out, hipMemcpyDeviceToHost));
        WT_HIP(hipMemcpy(o_finish, d_out + cap, sizeof(int32_t) * (size_t) *n_out, hipMemcpyDeviceToHost));
        WT_HIP(hipMemcpy(o_value, d_val, sizeof(double) * (size_t) *n_out, hipMemcpyDeviceToHost));
    }
    l.quiet = true;             // (the call waited for its stream and the copies home for the device: the buffers are idle)
    return WTAMD_OK;
}

}  // namespace

extern "C" {

int wtamd_runs_bin(int64_t n_seg, const int64_t *seg_off, const int32_t *start, const int32_t *finish, const void *value, int value_is_f64,
                   int32_t width, double default_value, int64_t capacity, int32_t *o_start, int32_t *o_finish, double *o_value,
                   int64_t *o_seg_off, int64_t *n_out, void *stream) {
    HipWindowLauncher l{{(hipStream_t) stream, __FILE__}};
    const char *why = "";
    const int rc = wwn_bin_door(l, (long long) n_seg, seg_off, start, finish, value, value_is_f64, (long long) width, default_value, (long long) capacity,
                                o_start, o_finish, o_value, o_seg_off, n_out, &why);
    return wt_runs_report("wtamd_runs_bin", rc, why);
}

int wtamd_runs_smooth(int64_t n_seg, const int64_t *seg_off, const int32_t *start, const int32_t *finish, const void *value, int value_is_f64,
                      int32_t width, int32_t clip_lo, int32_t clip_hi, int64_t capacity, int32_t *o_start, int32_t *o_finish, double *o_value,
                      int64_t *o_seg_off, int64_t *n_out, void *stream) {
    HipWindowLauncher l{{(hipStream_t) stream, __FILE__}};
    const char *why = "";
    const int rc = wwn_smooth_door(l, (long long) n_seg, seg_off, start, finish, value, value_is_f64, (long long) width, (long long) clip_lo,
                                   (long long) clip_hi, (long long) capacity, o_start, o_finish, o_value, o_seg_off, n_out, &why);
    return wt_runs_report("wtamd_runs_smooth", rc, why);
}

int wtamd_runs_bin_host(int64_t n, const int32_t *start, const int32_t *finish, const double *value, int32_t width, double default_value,
                        int64_t capacity, int32_t *o_start, int32_t *o_finish, double *o_value, int64_t *n_out) {
    return window_host("wtamd_runs_bin_host", n, start, finish, value, capacity, o_start, o_finish, o_value, n_out,
                       [&](const int64_t *seg, const WtDevRuns &in, int32_t *ds, int32_t *df, double *dv, int64_t *oseg) {
                           return wtamd_runs_bin(1, seg, in.start, in.finish, in.value, 1, width, default_value, capacity, ds, df, dv, oseg, n_out, nullptr);
                       });
}

int wtamd_runs_smooth_host(int64_t n, const int32_t *start, const int32_t *finish, const double *value, int32_t width, int32_t clip_lo,
                           int32_t clip_hi, int64_t capacity, int32_t *o_start, int32_t *o_finish, double *o_value, int64_t *n_out) {
    return window_host("wtamd_runs_smooth_host", n, start, finish, value, capacity, o_start, o_finish, o_value, n_out,
                       [&](const int64_t *seg, const WtDevRuns &in, int32_t *ds, int32_t *df, double *dv, int64_t *oseg) {
                           return wtamd_runs_smooth(1, seg, in.start, in.finish, in.value, 1, width, clip_lo, clip_hi, capacity, ds, df, dv, oseg, n_out,
                                                    nullptr);
                       });
}

}  // extern "C"
