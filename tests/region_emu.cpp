// region_emu.cpp -- the region passes of csrc/wt_region.h on the CPU (test infrastructure of tests/test_region_model.py).
// The header is compiled with -DWT_EMU: a pass is a function of (arguments, workgroup index), and this launcher runs the
// workgroups of every pass one after the other, forwards, backwards or shuffled.  The door (validation, union of the mask,
// capacity) is the product's own template over this launcher.
#define WT_EMU 1
#include <algorithm>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <numeric>
#include <random>
#include <vector>

#include "../wiggletools_amd/csrc/wt_region.h"

namespace {

struct CpuLauncher {
    int order;              // 0 forwards, 1 backwards, 2 shuffled
    std::mt19937_64 rng;
    void *alloc(size_t bytes) { return malloc(bytes); }
    void release(void *p) { free(p); }
    bool zero(void *p, size_t bytes) { memset(p, 0, bytes); return true; }
    bool to_host(void *h, const void *d, size_t bytes) { memcpy(h, d, bytes); return true; }
    bool to_device(void *d, const void *h, size_t bytes) { memcpy(d, h, bytes); return true; }
    std::vector<long long> blocks_in_order(long long blocks) {
        std::vector<long long> idx((size_t) blocks);
        std::iota(idx.begin(), idx.end(), 0ll);
        if (order == 1) std::reverse(idx.begin(), idx.end());
        if (order == 2) std::shuffle(idx.begin(), idx.end(), rng);
        return idx;
    }
    bool run(int kernel, long long blocks, const WcvArgs &a) {
        WcvLds lds;
        for (long long b : blocks_in_order(blocks)) {
            memset(&lds, 0xa5, sizeof lds);         // nothing may survive in LDS from one workgroup to the next
            wcv_run_block(kernel, a, b, &lds);
        }
        return true;
    }
    bool run_region(int kernel, long long blocks, const WrgArgs &a) {
        WrgLds lds;
        for (long long b : blocks_in_order(blocks)) {
            memset(&lds, 0xa5, sizeof lds);
            wrg_run_block(kernel, a, b, &lds);
        }
        return true;
    }
};

}  // namespace

extern "C" {

int region_emu(int order, uint64_t seed, int op, int64_t n_seg, const int64_t *seg_off, const int32_t *start, const int32_t *finish,
               const void *value, int value_is_f64, const int64_t *m_seg_off, const int32_t *m_start, const int32_t *m_finish,
               int64_t capacity, int32_t *o_start, int32_t *o_finish, double *o_value, int64_t *o_seg_off, int64_t *n_out) {
    CpuLauncher l{order, std::mt19937_64(seed)};
    const char *why = "";
    return wrg_region(l, op, (long long) n_seg, seg_off, start, finish, value, value_is_f64, m_seg_off, m_start, m_finish,
                      (long long) capacity, o_start, o_finish, o_value, o_seg_off, n_out, &why);
}

}  // extern "C"
