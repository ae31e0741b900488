// wt_apply.hip -- per-region statistics on the device: the six moments the reference's ApplyMultiplexer (src/apply.c; `apply`,
// `apply_paste`) needs for AUC meanI varI stddevI CVI maxI minI of a dataset inside every region, over whole run lists in HBM.
// The passes and the door are written once in csrc/wt_apply.h (which tests/apply_emu.cpp also compiles for the CPU); this
// unit gives every pass its kernel; the launcher of the door, the report of its result and the staging of the *_host entry are
// those of csrc/wt_runs_host.h.  The scan of the tiles' chunk counts is a pass of
// csrc/wt_cover.h, launched by csrc/wt_cover.hip (wt_cover_run).  Temporary device memory comes from the pool (wt_pool.h).
#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>
#include <vector>

#include "wt_runs_host.h"
#include "wt_apply.h"

namespace {

template <int K>
__global__ void __launch_bounds__(WAP_BLOCK) wt_apply_kernel(WapArgs a) {
    __shared__ WapLds lds;
    wap_run_block(K, a, (long long) blockIdx.x, &lds);
}

struct HipApplyLauncher : WtRunsLauncher {
    template <int K> bool launch(long long blocks, const WapArgs &a) { return WtRunsLauncher::launch(wt_apply_kernel<K>, WAP_BLOCK, blocks, a); }
    bool run_apply(int kernel, long long blocks, const WapArgs &a) {
        switch (kernel) {
        case WAP_K_VALID_D: return launch<WAP_K_VALID_D>(blocks, a);
        case WAP_K_VALID_R: return launch<WAP_K_VALID_R>(blocks, a);
        case WAP_K_BOUNDS: return launch<WAP_K_BOUNDS>(blocks, a);
        case WAP_K_CHUNK: return launch<WAP_K_CHUNK>(blocks, a);
        case WAP_K_FINAL: return launch<WAP_K_FINAL>(blocks, a);
        default: return false;
        }
    }
};

}  // namespace

extern "C" {

int wtamd_runs_apply(int64_t n_seg, const int64_t *seg_off, const int32_t *start, const int32_t *finish, const void *value, int value_is_f64,
                     const int64_t *r_seg_off, const int32_t *r_start, const int32_t *r_finish, double default_value, uint32_t flags,
                     double *moments6, void *stream) {
    static_assert(WAP_STRICT == WTAMD_APPLY_STRICT, "wt_apply.h and wiggletools_amd.h name the flag alike");
    static_assert(sizeof(WapRegion) == 16 && sizeof(WapPartial) == 64, "the scratch figures of the header");
    HipApplyLauncher l{{(hipStream_t) stream, __FILE__}};
    const char *why = "";
    const int rc = wap_apply(l, (long long) n_seg, seg_off, start, finish, value, value_is_f64, r_seg_off, r_start, r_finish, default_value,
                             (unsigned int) flags, moments6, &why);
    return wt_runs_report("wtamd_runs_apply", rc, why);
}

// One segment pair in HOST memory in, 6 doubles per region in HOST memory out: device memory from the pool, copies and the
// call on the null stream.
int wtamd_runs_apply_host(int64_t n, const int32_t *start, const int32_t *finish, const double *value, int64_t n_regions,
                          const int32_t *r_start, const int32_t *r_finish, double default_value, uint32_t flags, double *moments6) {
    if (n < 0 || n_regions < 0 || (n > 0 && (!start || !finish || !value)) || (n_regions > 0 && (!r_start || !r_finish || !moments6)))
        return wt_fail(WTAMD_ERR_ARG, "wtamd_runs_apply_host: bad argument");
    HipApplyLauncher l{{nullptr, __FILE__}};
    WcvScope<HipApplyLauncher> sc(l);
    WtDevRuns in, reg;
    double *d_out = nullptr;
    if (const int e = wt_stage_runs("wtamd_runs_apply_host", sc, n, start, finish, value, true, &in)) return e;
    if (const int e = wt_stage_runs("wtamd_runs_apply_host", sc, n_regions, r_start, r_finish, nullptr, false, &reg)) return e;
    if (!sc.get(&d_out, 6 * (size_t) (n_regions > 0 ? n_regions : 1))) return wt_fail(WTAMD_ERR_HIP, "wtamd_runs_apply_host: out of device memory");
    const int64_t seg[2] = {0, n}, rseg[2] = {0, n_regions};
    const int rc = wtamd_runs_apply(1, seg, in.start, in.finish, in.value, 1, rseg, reg.start, reg.finish, default_value, flags, d_out, nullptr);
    if (rc != WTAMD_OK) return rc;
    if (n_regions > 0) WT_HIP(hipMemcpy(moments6, d_out, sizeof(double) * 6 * (size_t) n_regions, hipMemcpyDeviceToHost));
    l.quiet = true;             // (the call waited for its stream and the copy home for the device: the buffers are idle)
    return WTAMD_OK;
}

}  // extern "C"
