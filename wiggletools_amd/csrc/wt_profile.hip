// wt_profile.hip -- region profiles on the device: the dataset under every region on `width` bins, as the reference's
// ProfileMultiplexer (src/apply.c; `profile`, `profiles`) computes them through regionProfile (src/plots.c), over whole run
// lists in HBM.  The passes and the door are written once in csrc/wt_profile.h (which tests/profile_emu.cpp also compiles for
// the CPU); this unit gives every pass its kernel; the launcher of the door, the report of its result and the staging of the *_host
// entry are those of csrc/wt_runs_host.h.  The scan of the workgroups' wave-regime counts
// is a pass of csrc/wt_cover.h, launched by csrc/wt_cover.hip (wt_cover_run).  Temporary device memory comes from the pool
// (wt_pool.h).
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdlib>
#include <string>
#include <vector>

#include "wt_runs_host.h"
#include "wt_profile.h"

namespace {

template <int K>
__global__ void __launch_bounds__(WPR_BLOCK) wt_profile_kernel(WprArgs a) {
    __shared__ WprLds lds;
    wpr_run_block(K, a, (long long) blockIdx.x, &lds);
}

struct HipProfileLauncher : WtRunsLauncher {
    template <int K> bool launch(long long blocks, const WprArgs &a) { return WtRunsLauncher::launch(wt_profile_kernel<K>, WPR_BLOCK, blocks, a); }
    bool run_profile(int kernel, long long blocks, const WprArgs &a) {
        switch (kernel) {
        case WPR_K_VALID_D: return launch<WPR_K_VALID_D>(blocks, a);
        case WPR_K_VALID_R: return launch<WPR_K_VALID_R>(blocks, a);
        case WPR_K_BOUNDS: return launch<WPR_K_BOUNDS>(blocks, a);
        case WPR_K_BINS: return launch<WPR_K_BINS>(blocks, a);
        case WPR_K_HEAVY: return launch<WPR_K_HEAVY>(blocks, a);
        case WPR_K_FOLD: return launch<WPR_K_FOLD>(blocks, a);
        case WPR_K_ADD: return launch<WPR_K_ADD>(blocks, a);
        default: return false;
        }
    }
};

// WTAMD_PROFILE_BATCH=<regions>: the batch of the door (rounded down to a power of two); the tests force it small
long long profile_batch() {
    const char *e = getenv("WTAMD_PROFILE_BATCH");
    const long long b = e ? atoll(e) : 0;
    return b > 0 ? b : 0;
}

}  // namespace

extern "C" {

int wtamd_runs_profile(int64_t n_seg, const int64_t *seg_off, const int32_t *start, const int32_t *finish, const void *value, int value_is_f64,
                       const int64_t *r_seg_off, const int32_t *r_start, const int32_t *r_finish, int32_t width, double default_value,
                       uint32_t flags, double *profile, void *stream) {
    static_assert(WPR_SUM == WTAMD_PROFILE_SUM, "wt_profile.h and wiggletools_amd.h name the flag alike");
    HipProfileLauncher l{{(hipStream_t) stream, __FILE__}};
    const char *why = "";
    const int rc = wpr_profile(l, (long long) n_seg, seg_off, start, finish, value, value_is_f64, r_seg_off, r_start, r_finish, (long long) width,
                               default_value, (unsigned int) flags, profile_batch(), profile, &why);
    return wt_runs_report("wtamd_runs_profile", rc, why);
}

// One segment pair in HOST memory in, the rows (or their sum) in HOST memory out: device memory from the pool, copies and the
// call on the null stream.
int wtamd_runs_profile_host(int64_t n, const int32_t *start, const int32_t *finish, const double *value, int64_t n_regions,
                            const int32_t *r_start, const int32_t *r_finish, int32_t width, double default_value, uint32_t flags,
                            double *profile) {
    const bool sum = (flags & WTAMD_PROFILE_SUM) != 0;
    if (n < 0 || n_regions < 0 || width < 1 || (flags & ~WTAMD_PROFILE_SUM) || (n > 0 && (!start || !finish || !value)) ||
        (n_regions > 0 && (!r_start || !r_finish)) || ((n_regions > 0 || sum) && !profile))
        return wt_fail(WTAMD_ERR_ARG, "wtamd_runs_profile_host: bad argument");
    HipProfileLauncher l{{nullptr, __FILE__}};
    WcvScope<HipProfileLauncher> sc(l);
    WtDevRuns in, reg;
    double *d_out = nullptr;
    const size_t n_out = (sum ? (size_t) 1 : (size_t) n_regions) * (size_t) width;
    if (const int e = wt_stage_runs("wtamd_runs_profile_host", sc, n, start, finish, value, true, &in)) return e;
    if (const int e = wt_stage_runs("wtamd_runs_profile_host", sc, n_regions, r_start, r_finish, nullptr, false, &reg)) return e;
    if (!sc.get(&d_out, n_out)) return wt_fail(WTAMD_ERR_HIP, "wtamd_runs_profile_host: out of device memory");
    const int64_t seg[2] = {0, n}, rseg[2] = {0, n_regions};
    const int rc = wtamd_runs_profile(1, seg, in.start, in.finish, in.value, 1, rseg, reg.start, reg.finish, width, default_value, flags, d_out, nullptr);
    if (rc != WTAMD_OK) return rc;
    if (n_out > 0) WT_HIP(hipMemcpy(profile, d_out, sizeof(double) * n_out, hipMemcpyDeviceToHost));
    l.quiet = true;             // (the call waited for its stream and the copy home for the device: the buffers are idle)
    return WTAMD_OK;
}

}  // extern "C"
