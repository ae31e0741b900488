// wt_hist.hip -- value histograms on the device: the reference's histogram() (src/plots.c:77-223, `histogram`) over whole run
// lists in HBM.  The passes and the door are written once in csrc/wt_hist.h (which tests/hist_emu.cpp also compiles for the
// CPU); this unit gives every pass its kernel; the launcher of the door, the report of its result and the staging of the *_host
// entry are those of csrc/wt_runs_host.h.  Temporary device memory comes from the pool (wt_pool.h).
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdlib>
#include <string>
#include <vector>

#include "wt_runs_host.h"
#include "wt_hist.h"

namespace {

template <int K>
__global__ void __launch_bounds__(WHS_BLOCK) wt_hist_kernel(WhsArgs a) {
    __shared__ whs_u64 lds[K == WHS_K_BINS ? WHS_LDS_WIDTH : K == WHS_K_RANGE ? WHS_RANGE_WORDS : 1];
    whs_run_words(K, a, (long long) blockIdx.x, lds);
}

struct HipHistLauncher : WtRunsLauncher {
    template <int K> bool launch(long long blocks, const WhsArgs &a) { return WtRunsLauncher::launch(wt_hist_kernel<K>, WHS_BLOCK, blocks, a); }
    bool run_hist(int kernel, long long blocks, const WhsArgs &a) {
        switch (kernel) {
        case WHS_K_RANGE: return launch<WHS_K_RANGE>(blocks, a);
        case WHS_K_LOAD: return launch<WHS_K_LOAD>(blocks, a);
        case WHS_K_BINS: return launch<WHS_K_BINS>(blocks, a);
        case WHS_K_BINSG: return launch<WHS_K_BINSG>(blocks, a);
        case WHS_K_FINISH: return launch<WHS_K_FINISH>(blocks, a);
        default: return false;
        }
    }
};

}  // namespace

extern "C" {

int wtamd_runs_histogram(int64_t n_seg, const int64_t *seg_off, const int32_t *seg_row, int32_t n_rows, const int32_t *start, const int32_t *finish,
                         const void *value, int value_is_f64, int32_t width, uint32_t flags, double *range2, double *hist, void *stream) {
    HipHistLauncher l{{(hipStream_t) stream, __FILE__}};
    const char *why = "";
    const int rc = whs_door(l, (long long) n_seg, seg_off, seg_row, (int) n_rows, start, finish, value, value_is_f64, (int) width, (unsigned int) flags,
                            range2, hist, &why);
    return wt_runs_report("wtamd_runs_histogram", rc, why);
}

// The run lists and the matrix in HOST memory: device memory from the pool, copies and the call on the null stream.
int wtamd_runs_histogram_host(int64_t n_seg, const int64_t *seg_off, const int32_t *seg_row, int32_t n_rows, const int32_t *start, const int32_t *finish,
                              const double *value, int32_t width, uint32_t flags, double *range2, double *hist) {
    const char *bad = whs_check((long long) n_seg, seg_off, seg_row, (int) n_rows, start, finish, value, (int) width, (unsigned int) flags, range2, hist);
    if (*bad) return wt_fail(WTAMD_ERR_ARG, std::string("wtamd_runs_histogram_host: ") + bad);
    HipHistLauncher l{{nullptr, __FILE__}};
    WcvScope<HipHistLauncher> sc(l);
    WtDevRuns in;
    double *d_hist = nullptr;
    const int64_t n = n_seg ? seg_off[n_seg] : 0;
    const size_t cells = (size_t) n_rows * (size_t) width;
    if (const int e = wt_stage_runs("wtamd_runs_histogram_host", sc, n, start, finish, value, true, &in)) return e;
    if (!sc.get(&d_hist, cells)) return wt_fail(WTAMD_ERR_HIP, "wtamd_runs_histogram_host: out of device memory");
    if (flags & WHS_ACCUMULATE) WT_HIP(hipMemcpy(d_hist, hist, sizeof(double) * cells, hipMemcpyHostToDevice));
    double r2[2] = {range2[0], range2[1]};
    const int rc = wtamd_runs_histogram(n_seg, seg_off, seg_row, n_rows, in.start, in.finish, in.value, 1, width, flags, r2, d_hist, nullptr);
    if (rc != WTAMD_OK) return rc;
    WT_HIP(hipMemcpy(hist, d_hist, sizeof(double) * cells, hipMemcpyDeviceToHost));
    range2[0] = r2[0]; range2[1] = r2[1];
    l.quiet = true;             // (the call waited for its stream and the copy home for the device: the buffers are idle)
    return WTAMD_OK;
}

}  // extern "C"
