// wt_launch.h -- the host arithmetic every persistent-workgroup launcher shares (general, patch, difference-array and
// walking kernels); each launcher keeps only its own grid clamp and its hipLaunchKernelGGL.
#ifndef WT_LAUNCH_H_
#define WT_LAUNCH_H_

#include <hip/hip_runtime.h>
#include <map>
#include <mutex>
#include <tuple>

// Resident workgroups per CU (at least 1) of `kern` at T lanes and `lds` bytes of dynamic LDS.  The attribute and the
// query are made once per device, kernel and launch shape: host calls of 50-150 us each, and they sat between the event
// that starts the reduction's clock and the launch (round 6: the bench's events read 0.12-0.28 ms more per launch than
// rocprofv3's kernel durations).
inline hipError_t wt_blocks_per_cu(const void *kern, int T, int lds, int *per_cu) {
    static std::mutex mu;
    static std::map<std::tuple<int, const void *, int, int>, int> known;
    int dev = 0;
    (void) hipGetDevice(&dev);
    const auto key = std::make_tuple(dev, kern, T, lds);
    {
        std::lock_guard<std::mutex> lk(mu);
        auto it = known.find(key);
        if (it != known.end()) { *per_cu = it->second; return hipSuccess; }
    }
    hipError_t e = lds > 48 * 1024 ? hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, lds) : hipSuccess;
    if (e == hipSuccess) e = hipOccupancyMaxActiveBlocksPerMultiprocessor(per_cu, kern, T, (size_t) lds);
    if (e != hipSuccess) return e;
    if (*per_cu < 1) *per_cu = 1;
    std::lock_guard<std::mutex> lk(mu);
    known[key] = *per_cu;
    return hipSuccess;
}

// The global slab the resident workgroups share: at least `need` bytes behind *slab, which only ever grows
inline hipError_t wt_reserve_slab(char **slab, size_t *bytes, size_t need) {
    if (*bytes >= need) return hipSuccess;
    (void) hipFree(*slab);          // synchronises with earlier launches
    *slab = nullptr; *bytes = 0;
    const hipError_t e = hipMalloc((void **) slab, need);
    if (e == hipSuccess) *bytes = need;
    return e;
}

#endif  // WT_LAUNCH_H_
