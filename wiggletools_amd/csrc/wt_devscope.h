// wt_devscope.h -- temporary device buffers of one host entry point, released on every exit path
// (the WT_HIP-style early returns included).  They come from the device pool (wt_pool.h) and go back to it: the destructor
// waits for the device ONCE, before the first of them returns (an early return may leave a kernel in flight on them).
#ifndef WT_DEVSCOPE_H_
#define WT_DEVSCOPE_H_
#include <hip/hip_runtime.h>

#include <vector>

#include "wt_pool.h"

struct WtDevScope {
    std::vector<void *> ptrs;
    WtDevScope() = default;
    WtDevScope(const WtDevScope &) = delete;
    WtDevScope &operator=(const WtDevScope &) = delete;
    template <class T>
    hipError_t alloc(T **p, size_t bytes, const char *file = __builtin_FILE(), int line = __builtin_LINE()) {
        void *q = nullptr;
        const hipError_t e = wt_dev_alloc_bytes(&q, bytes ? bytes : 1, file, line);
        if (e == hipSuccess) { ptrs.push_back(q); *p = (T *) q; }
        return e;
    }
    ~WtDevScope() {
        if (ptrs.empty()) return;
        (void) wt_pool_quiesce();
        for (void *q : ptrs) (void) wt_dev_free(q);
    }
};

#endif  // WT_DEVSCOPE_H_
