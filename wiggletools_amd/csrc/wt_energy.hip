// wt_energy.hip -- energy spectra on the device: the reference's EnergyIntegrator (src/statistics.c:345-391, `energy`) over whole
// run lists in HBM, every wavelength from one call.  The passes and the door are written once in csrc/wt_energy.h (which
// tests/energy_emu.cpp also compiles for the CPU); this unit gives every pass its kernel; the launcher of the door, the report of
// its result and the staging of the *_host entry are those of csrc/wt_runs_host.h.  Temporary device memory comes from the pool
// (wt_pool.h).
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdlib>
#include <string>
#include <vector>

#include "wt_runs_host.h"
#include "wt_energy.h"

namespace {

template <int K>
__global__ void __launch_bounds__(WEN_BLOCK) wt_energy_kernel(WenArgs a) {
    __shared__ double w[K == WEN_K_MAIN ? WEN_LDS_DOUBLES : K == WEN_K_FINAL ? WEN_BLOCK : 1];
    __shared__ unsigned int bm[WEN_KCHUNK];
    wen_run_words(K, a, (long long) blockIdx.x, w, bm);
}

struct HipEnergyLauncher : WtRunsLauncher {
    template <int K> bool launch(long long blocks, const WenArgs &a) { return WtRunsLauncher::launch(wt_energy_kernel<K>, WEN_BLOCK, blocks, a); }
    bool run_energy(int kernel, long long blocks, const WenArgs &a) {
        switch (kernel) {
        case WEN_K_LAST: return launch<WEN_K_LAST>(blocks, a);
        case WEN_K_MAIN: return launch<WEN_K_MAIN>(blocks, a);
        case WEN_K_FINAL: return launch<WEN_K_FINAL>(blocks, a);
        default: return false;
        }
    }
};

}  // namespace

extern "C" {

int wtamd_runs_energy(int64_t n_seg, const int64_t *seg_off, const int64_t *seg_base, const int32_t *start, const int32_t *finish, const void *value,
                      int value_is_f64, int32_t n_wavelengths, const int32_t *wavelength, double *reim, int64_t *end_base, void *stream) {
    HipEnergyLauncher l{{(hipStream_t) stream, __FILE__}};
    const char *why = "";
    const int rc = wen_door(l, (long long) n_seg, seg_off, seg_base, start, finish, value, value_is_f64, (int) n_wavelengths, wavelength, reim, end_base, &why);
    return wt_runs_report("wtamd_runs_energy", rc, why);
}

// The run lists in HOST memory: device memory from the pool, copies and the call on the null stream.
int wtamd_runs_energy_host(int64_t n_seg, const int64_t *seg_off, const int64_t *seg_base, const int32_t *start, const int32_t *finish,
                           const double *value, int32_t n_wavelengths, const int32_t *wavelength, double *reim, int64_t *end_base) {
    const char *bad = wen_check((long long) n_seg, seg_off, start, finish, value, (int) n_wavelengths, wavelength, reim);
    if (*bad) return wt_fail(WTAMD_ERR_ARG, std::string("wtamd_runs_energy_host: ") + bad);
    HipEnergyLauncher l{{nullptr, __FILE__}};
    WcvScope<HipEnergyLauncher> sc(l);
    WtDevRuns in;
    const int64_t n = n_seg ? seg_off[n_seg] : 0;
    if (const int e = wt_stage_runs("wtamd_runs_energy_host", sc, n, start, finish, value, true, &in)) return e;
    const int rc = wtamd_runs_energy(n_seg, seg_off, seg_base, in.start, in.finish, in.value, 1, n_wavelengths, wavelength, reim, end_base, nullptr);
    l.quiet = true;             // (the call waited for its stream: the buffers are idle)
    return rc;
}

}  // extern "C"
