// wt_region.hip -- the reference's region operators on the device: OverlapWiggleIterator, NoverlapWiggleIterator,
// TrimWiggleIterator and NearestWiggleIterator (src/unaryOps.c:437-639; `overlaps`, `noverlaps`, `trim`, `nearest`) over whole
// run lists in HBM.  The passes and the door are written once in csrc/wt_region.h (which tests/region_emu.cpp also compiles
// for the CPU); this unit gives every pass its kernel and the door its launcher.  The union of the mask and the scan of the
// tile counts are passes of csrc/wt_cover.h, launched by csrc/wt_cover.hip (wt_cover_run).
#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>
#include <vector>

#include "wt_host.h"
#include "wt_region.h"

bool wt_cover_run(void *stream, int kernel, long long blocks, const WcvArgs &a);      // csrc/wt_cover.hip

namespace {

template <int K>
__global__ void __launch_bounds__(WRG_BLOCK) wt_region_kernel(WrgArgs a) {
    __shared__ WrgLds lds;
    wrg_run_block(K, a, (long long) blockIdx.x, &lds);
}

struct HipRegionLauncher {
    hipStream_t s;
    void *alloc(size_t bytes) {
        void *p = nullptr;
        return hipMalloc(&p, bytes) == hipSuccess ? p : nullptr;
    }
    void release(void *p) { (void) hipFree(p); }
    bool zero(void *p, size_t bytes) { return hipMemsetAsync(p, 0, bytes, s) == hipSuccess; }
    bool to_host(void *h, const void *d, size_t bytes) {
        return hipMemcpyAsync(h, d, bytes, hipMemcpyDeviceToHost, s) == hipSuccess && hipStreamSynchronize(s) == hipSuccess;
    }
    bool to_device(void *d, const void *h, size_t bytes) {
        return hipMemcpyAsync(d, h, bytes, hipMemcpyHostToDevice, s) == hipSuccess && hipStreamSynchronize(s) == hipSuccess;
    }
    bool run(int kernel, long long blocks, const WcvArgs &a) { return wt_cover_run((void *) s, kernel, blocks, a); }
    template <int K> bool launch(long long blocks, const WrgArgs &a) {
        if (blocks <= 0) return true;
        if (blocks > 0x7fffffffll) return false;
        hipLaunchKernelGGL(wt_region_kernel<K>, dim3((unsigned) blocks), dim3(WRG_BLOCK), 0, s, a);
        return hipGetLastError() == hipSuccess;
    }
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
    HipRegionLauncher l{(hipStream_t) stream};
    const char *why = "";
    const int rc = wrg_region(l, op, (long long) n_seg, seg_off, start, finish, value, value_is_f64, m_seg_off, m_start, m_finish,
                              (long long) capacity, o_start, o_finish, o_value, o_seg_off, n_out, &why);
    if (rc == 0) return WTAMD_OK;
    if (rc == 3) return wt_fail(WTAMD_ERR_CAPACITY, "wtamd_runs_region: the output arrays are too small (*n_out holds the count needed)");
    if (rc == 1) return wt_fail(WTAMD_ERR_ARG, std::string("wtamd_runs_region: ") + why);
    const hipError_t e = hipGetLastError();
    return wt_fail(WTAMD_ERR_HIP, std::string("wtamd_runs_region: ") + why + " (" + hipGetErrorString(e) + ")");
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
    struct Free { void *p; ~Free() { (void) hipFree(p); } };
    int32_t *d_in = nullptr, *d_mask = nullptr, *d_out = nullptr;
    double *d_val = nullptr, *d_oval = nullptr;
    const size_t n1 = (size_t) (n > 0 ? n : 1), m1 = (size_t) (m > 0 ? m : 1), c1 = (size_t) (capacity > 0 ? capacity : 1);
    WT_HIP(hipMalloc(&d_in, sizeof(int32_t) * 2 * n1));
    Free f1{d_in};
    WT_HIP(hipMalloc(&d_val, sizeof(double) * n1));
    Free f2{d_val};
    WT_HIP(hipMalloc(&d_mask, sizeof(int32_t) * 2 * m1));
    Free f3{d_mask};
    WT_HIP(hipMalloc(&d_out, sizeof(int32_t) * 2 * c1));
    Free f4{d_out};
    WT_HIP(hipMalloc(&d_oval, sizeof(double) * c1));
    Free f5{d_oval};
    if (n > 0) {
        WT_HIP(hipMemcpy(d_in, start, sizeof(int32_t) * (size_t) n, hipMemcpyHostToDevice));
        WT_HIP(hipMemcpy(d_in + n1, finish, sizeof(int32_t) * (size_t) n, hipMemcpyHostToDevice));
        WT_HIP(hipMemcpy(d_val, value, sizeof(double) * (size_t) n, hipMemcpyHostToDevice));
    }
    if (m > 0) {
        WT_HIP(hipMemcpy(d_mask, m_start, sizeof(int32_t) * (size_t) m, hipMemcpyHostToDevice));
        WT_HIP(hipMemcpy(d_mask + m1, m_finish, sizeof(int32_t) * (size_t) m, hipMemcpyHostToDevice));
    }
    const int64_t seg[2] = {0, n}, mseg[2] = {0, m};
    int64_t oseg[2] = {0, 0};
    const int rc = wtamd_runs_region(op, 1, seg, d_in, d_in + n1, d_val, 1, mseg, d_mask, d_mask + m1, capacity, d_out, d_out + c1, d_oval,
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
