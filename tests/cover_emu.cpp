// cover_emu.cpp -- the coverage / union passes of csrc/wt_cover.h on the CPU (test infrastructure of tests/test_cover_model.py).
// The header is compiled with -DWT_EMU: a pass is a function of (arguments, workgroup index), and this launcher runs the
// workgroups of every pass one after the other, forwards, backwards or shuffled.  The doors (grouping under the scratch
// budget, cuts at positions, capacity) are the product's own templates over this launcher.
#define WT_EMU 1
#include <algorithm>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <numeric>
#include <random>
#include <vector>

#include "../wiggletools_amd/csrc/wt_cover.h"

namespace {

struct CpuLauncher {
    int order;              // 0 forwards, 1 backwards, 2 shuffled
    std::mt19937_64 rng;
    long long launches = 0, peak_alloc = 0;
    void *alloc(size_t bytes) { if ((long long) bytes > peak_alloc) peak_alloc = (long long) bytes; return malloc(bytes); }
    void release(void *p) { free(p); }
    bool zero(void *p, size_t bytes) { memset(p, 0, bytes); return true; }
    bool to_host(void *h, const void *d, size_t bytes) { memcpy(h, d, bytes); return true; }
    bool to_device(void *d, const void *h, size_t bytes) { memcpy(d, h, bytes); return true; }
    bool run(int kernel, long long blocks, const WcvArgs &a) {
        std::vector<long long> idx((size_t) blocks);
        std::iota(idx.begin(), idx.end(), 0ll);
        if (order == 1) std::reverse(idx.begin(), idx.end());
        if (order == 2) std::shuffle(idx.begin(), idx.end(), rng);
        WcvLds lds;
        for (long long b : idx) {
            memset(&lds, 0xa5, sizeof lds);         // nothing may survive in LDS from one workgroup to the next
            wcv_run_block(kernel, a, b, &lds);
        }
        launches++;
        return true;
    }
};

}  // namespace

extern "C" {

int cover_emu_coverage(int order, uint64_t seed, int64_t n_seg, const int64_t *seg_off, const int32_t *start, const int32_t *finish,
                       int64_t capacity, int32_t *o_start, int32_t *o_finish, double *o_value, int64_t *o_seg_off, int64_t *n_out,
                       int64_t budget_bytes, int64_t *launches) {
    CpuLauncher l{order, std::mt19937_64(seed)};
    const char *why = "";
    const int rc = wcv_coverage(l, (long long) n_seg, seg_off, start, finish, (long long) capacity, o_start, o_finish, o_value, o_seg_off,
                                n_out, (long long) budget_bytes, &why);
    if (launches) *launches = l.launches;
    return rc;
}

int cover_emu_union(int order, uint64_t seed, int64_t n_seg, const int64_t *seg_off, const int32_t *start, const int32_t *finish,
                    const void *value, int value_is_f64, int64_t capacity, int32_t *o_start, int32_t *o_finish, double *o_value,
                    int64_t *o_seg_off, int64_t *n_out) {
    CpuLauncher l{order, std::mt19937_64(seed)};
    const char *why = "";
    return wcv_union(l, (long long) n_seg, seg_off, start, finish, value, value_is_f64, (long long) capacity, o_start, o_finish, o_value,
                     o_seg_off, n_out, &why);
}

}  // extern "C"
