// wt_profile.hip -- region profiles on the device: the dataset under every region on `width` bins, as the reference's
// ProfileMultiplexer (src/apply.c; `profile`, `profiles`) computes them through regionProfile (src/plots.c), over whole run
// lists in HBM.  The passes and the door are written once in csrc/wt_profile.h (which tests/profile_emu.cpp also compiles for
// the CPU); this unit gives every pass its kernel and the door its launcher.  The scan of the workgroups' wave-regime counts
// is a pass of csrc/wt_cover.h, launched by csrc/wt_cover.hip (wt_cover_run).  Temporary device memory comes from the pool
// (wt_pool.h).
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdlib>
#include <string>
#include <vector>

#include "wt_host.h"
#include "wt_pool.h"
#include "wt_profile.h"

bool wt_cover_run(void *stream, int kernel, long long blocks, const WcvArgs &a);      // csrc/wt_cover.hip

namespace {

template <int K>
__global__ void __launch_bounds__(WPR_BLOCK) wt_profile_kernel(WprArgs a) {
    __shared__ WprLds lds;
    wpr_run_block(K, a, (long long) blockIdx.x, &lds);
}

struct HipProfileLauncher {
    hipStream_t s;
    bool quiet = false;         // as in csrc/wt_apply.hip: the buffers may return to the pool without the device-wide wait
    void *alloc(size_t bytes) {
        void *p = nullptr;
        return wt_dev_alloc_bytes(&p, bytes, __FILE__, __LINE__) == hipSuccess ? p : nullptr;
    }
    void release(void *p) {
        if (!quiet) { (void) wt_pool_quiesce(); quiet = true; }
        (void) wt_dev_free(p);
    }
    bool zero(void *p, size_t bytes) { quiet = false; return hipMemsetAsync(p, 0, bytes, s) == hipSuccess; }
    bool sync() { return quiet = hipStreamSynchronize(s) == hipSuccess; }
    bool to_host(void *h, const void *d, size_t bytes) {
        return hipMemcpyAsync(h, d, bytes, hipMemcpyDeviceToHost, s) == hipSuccess && sync();
    }
    bool to_device(void *d, const void *h, size_t bytes) {
        return hipMemcpyAsync(d, h, bytes, hipMemcpyHostToDevice, s) == hipSuccess && sync();
    }
    bool run(int kernel, long long blocks, const WcvArgs &a) { quiet = false; return wt_cover_run((void *) s, kernel, blocks, a); }
    template <int K> bool launch(long long blocks, const WprArgs &a) {
        if (blocks <= 0) return true;
        if (blocks > 0x7fffffffll) return false;
        quiet = false;
        hipLaunchKernelGGL(wt_profile_kernel<K>, dim3((unsigned) blocks), dim3(WPR_BLOCK), 0, s, a);
        return hipGetLastError() == hipSuccess;
    }
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
    HipProfileLauncher l{(hipStream_t) stream};
    const char *why = "";
    const int rc = wpr_profile(l, (long long) n_seg, seg_off, start, finish, value, value_is_f64, r_seg_off, r_start, r_finish, (long long) width,
                               default_value, (unsigned int) flags, profile_batch(), profile, &why);
    if (rc == 0) return WTAMD_OK;
    if (rc == 1) return wt_fail(WTAMD_ERR_ARG, std::string("wtamd_runs_profile: ") + why);
    const hipError_t e = hipGetLastError();
    return wt_fail(WTAMD_ERR_HIP, std::string("wtamd_runs_profile: ") + why + " (" + hipGetErrorString(e) + ")");
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
    HipProfileLauncher l{nullptr};
    WcvScope<HipProfileLauncher> sc(l);
    int32_t *d_in = nullptr, *d_reg = nullptr;
    double *d_val = nullptr, *d_out = nullptr;
    const size_t n1 = (size_t) (n > 0 ? n : 1), r1 = (size_t) (n_regions > 0 ? n_regions : 1);
    const size_t n_out = (sum ? (size_t) 1 : (size_t) n_regions) * (size_t) width;
    if (!sc.get(&d_in, 2 * n1) || !sc.get(&d_val, n1) || !sc.get(&d_reg, 2 * r1) || !sc.get(&d_out, n_out))
        return wt_fail(WTAMD_ERR_HIP, "wtamd_runs_profile_host: out of device memory");
    if (n > 0) {
        WT_HIP(hipMemcpy(d_in, start, sizeof(int32_t) * (size_t) n, hipMemcpyHostToDevice));
        WT_HIP(hipMemcpy(d_in + n1, finish, sizeof(int32_t) * (size_t) n, hipMemcpyHostToDevice));
        WT_HIP(hipMemcpy(d_val, value, sizeof(double) * (size_t) n, hipMemcpyHostToDevice));
    }
    if (n_regions > 0) {
        WT_HIP(hipMemcpy(d_reg, r_start, sizeof(int32_t) * (size_t) n_regions, hipMemcpyHostToDevice));
        WT_HIP(hipMemcpy(d_reg + r1, r_finish, sizeof(int32_t) * (size_t) n_regions, hipMemcpyHostToDevice));
    }
    const int64_t seg[2] = {0, n}, rseg[2] = {0, n_regions};
    const int rc = wtamd_runs_profile(1, seg, d_in, d_in + n1, d_val, 1, rseg, d_reg, d_reg + r1, width, default_value, flags, d_out, nullptr);
    if (rc != WTAMD_OK) return rc;
    if (n_out > 0) WT_HIP(hipMemcpy(profile, d_out, sizeof(double) * n_out, hipMemcpyDeviceToHost));
    l.quiet = true;             // (the call waited for its stream and the copy home for the device: the buffers are idle)
    return WTAMD_OK;
}

}  // extern "C"
