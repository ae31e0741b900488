// wt_text.hip -- wig and bedGraph text on the device: the reference's writer (printBlock, src/wigWriter.c:55-119; `write`,
// `write_bg`) over whole run lists in HBM.  The passes and the door are written once in csrc/wt_text.h (which tests/text_emu.cpp
// also compiles for the CPU); this unit gives every pass its kernel; the launcher of the door, the report of its result and the
// staging of the *_host entry are those of csrc/wt_runs_host.h.  Temporary device memory comes from the pool (wt_pool.h).
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdlib>
#include <string>
#include <vector>

#include "wt_runs_host.h"
#include "wt_text.h"

namespace {

template <int K>
__global__ void __launch_bounds__(WTX_BLOCK) wt_text_kernel(WtxArgs a) {
    __shared__ WtxLds lds;
    wtx_run_block(K, a, (long long) blockIdx.x, &lds);
}

struct HipTextLauncher : WtRunsLauncher {
    template <int K> bool launch(long long blocks, const WtxArgs &a) { return WtRunsLauncher::launch(wt_text_kernel<K>, WTX_BLOCK, blocks, a); }
    bool run_text(int kernel, long long blocks, const WtxArgs &a) {
        switch (kernel) {
        case WTX_K_MEASURE: return launch<WTX_K_MEASURE>(blocks, a);
        case WTX_K_SCAN: return launch<WTX_K_SCAN>(blocks, a);
        case WTX_K_EMIT: return launch<WTX_K_EMIT>(blocks, a);
        default: return false;
        }
    }
};

static_assert(sizeof(wtamd_text_state) == sizeof(WtxState) && sizeof(WtxState) == 16, "wtamd_text_state is WtxState");

}  // namespace

extern "C" {

int wtamd_runs_text(int64_t n_seg, const int64_t *seg_off, const char *const *seg_name, const int32_t *start, const int32_t *finish,
                    const void *value, int value_is_f64, uint32_t flags, wtamd_text_state *state, char *text, int64_t capacity,
                    int64_t *n_bytes, int64_t *n_wide, void *stream) {
    HipTextLauncher l{{(hipStream_t) stream, __FILE__}};
    const char *why = "";
    const int rc = wtx_door(l, (long long) n_seg, seg_off, seg_name, start, finish, value, value_is_f64, (unsigned int) flags, (WtxState *) state, text,
                            (long long) capacity, n_bytes, n_wide, &why);
    if (rc == 3) return wt_fail(WTAMD_ERR_CAPACITY, "wtamd_runs_text: the text buffer is too small (*n_bytes holds the size needed)");
    return wt_runs_report("wtamd_runs_text", rc, why);
}

// The run lists and the text in HOST memory: device memory from the pool, copies and the call on the null stream.
int wtamd_runs_text_host(int64_t n_seg, const int64_t *seg_off, const char *const *seg_name, const int32_t *start, const int32_t *finish,
                         const double *value, uint32_t flags, wtamd_text_state *state, char *text, int64_t capacity, int64_t *n_bytes,
                         int64_t *n_wide) {
    const char *bad = wtx_check((long long) n_seg, seg_off, seg_name, start, finish, value, (unsigned int) flags, (const WtxState *) state, text,
                                (long long) capacity, n_bytes, n_wide);
    if (*bad) return wt_fail(WTAMD_ERR_ARG, std::string("wtamd_runs_text_host: ") + bad);
    HipTextLauncher l{{nullptr, __FILE__}};
    WcvScope<HipTextLauncher> sc(l);
    WtDevRuns in;
    char *d_text = nullptr;
    const int64_t n = n_seg ? seg_off[n_seg] : 0;
    if (const int e = wt_stage_runs("wtamd_runs_text_host", sc, n, start, finish, value, true, &in)) return e;
    if (!sc.get(&d_text, (size_t) capacity)) return wt_fail(WTAMD_ERR_HIP, "wtamd_runs_text_host: out of device memory");
    const int rc = wtamd_runs_text(n_seg, seg_off, seg_name, in.start, in.finish, in.value, 1, flags, state, d_text, capacity, n_bytes, n_wide, nullptr);
    if (rc != WTAMD_OK) return rc;
    if (*n_bytes > 0) WT_HIP(hipMemcpy(text, d_text, (size_t) *n_bytes, hipMemcpyDeviceToHost));
    l.quiet = true;             // (the call waited for its stream and the copy home for the device: the buffers are idle)
    return WTAMD_OK;
}

}  // extern "C"
