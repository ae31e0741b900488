// profile_emu.cpp -- the profile passes of csrc/wt_profile.h on the CPU (test infrastructure of tests/test_profile_model.py).
// The header is compiled with -DWT_EMU: a pass is a function of (arguments, workgroup index), and this launcher runs the
// workgroups of every pass one after the other, forwards, backwards or shuffled.  The door (validation, bounds, bins, scan,
// heavy, fold, add) is the product's own template over this launcher; profile_host is the product's host sweep.
#define WT_EMU 1
#include <algorithm>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <numeric>
#include <random>
#include <vector>

#include "../wiggletools_amd/csrc/wt_profile.h"

namespace {

struct CpuLauncher {
    int order;              // 0 forwards, 1 backwards, 2 shuffled
    std::mt19937_64 rng;
    void *alloc(size_t bytes) { void *p = malloc(bytes); if (p) memset(p, 0x5a, bytes); return p; }     // (scratch starts out as garbage)
    void release(void *p) { free(p); }
    bool zero(void *p, size_t bytes) { memset(p, 0, bytes); return true; }
    bool to_host(void *h, const void *d, size_t bytes) { memcpy(h, d, bytes); return true; }
    bool to_device(void *d, const void *h, size_t bytes) { memcpy(d, h, bytes); return true; }
    bool sync() { return true; }
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
    bool run_profile(int kernel, long long blocks, const WprArgs &a) {
        static WprLds lds;
        for (long long b : blocks_in_order(blocks)) {
            memset(&lds, 0xa5, sizeof lds);
            wpr_run_block(kernel, a, b, &lds);
        }
        return true;
    }
};

}  // namespace

extern "C" {

int profile_emu(int order, uint64_t seed, int64_t n_seg, const int64_t *seg_off, const int32_t *start, const int32_t *finish, const void *value,
                int value_is_f64, const int64_t *r_seg_off, const int32_t *r_start, const int32_t *r_finish, int32_t width, double default_value,
                uint32_t flags, int64_t batch, double *profile) {
    CpuLauncher l{order, std::mt19937_64(seed)};
    const char *why = "";
    return wpr_profile(l, (long long) n_seg, seg_off, start, finish, value, value_is_f64, r_seg_off, r_start, r_finish, (long long) width,
                       default_value, (unsigned int) flags, (long long) batch, profile, &why);
}

int profile_host(int64_t n, const int32_t *start, const int32_t *finish, const double *value, int64_t n_r, const int32_t *r_start,
                 const int32_t *r_finish, int32_t width, double default_value, uint32_t flags, double *profile) {
    return wpr_profile_host((long long) n, start, finish, value, (long long) n_r, r_start, r_finish, (long long) width, default_value,
                            (unsigned int) flags, profile);
}

}  // extern "C"
