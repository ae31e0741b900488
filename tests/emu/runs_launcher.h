// runs_launcher.h -- the launcher of tests/cover_emu.cpp, region_emu.cpp, apply_emu.cpp and profile_emu.cpp: the doors of
// csrc/wt_cover.h, wt_region.h, wt_apply.h and wt_profile.h are templates over a Launcher, and this one runs the workgroups of
// every pass on the CPU one after the other, forwards, backwards or shuffled.  Included after #define WT_EMU 1; a unit derives
// its launcher and adds its run_* member over run_blocks.
#ifndef WT_RUNS_LAUNCHER_H_
#define WT_RUNS_LAUNCHER_H_

#include <algorithm>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <numeric>
#include <random>
#include <vector>

#include "../../wiggletools_amd/csrc/wt_cover.h"

struct CpuLauncher {
    int order;              // 0 forwards, 1 backwards, 2 shuffled
    std::mt19937_64 rng;
    long long launches = 0, peak_alloc = 0;
    CpuLauncher(int order_, uint64_t seed) : order(order_), rng(seed) {}
    void *alloc(size_t bytes) {
        if ((long long) bytes > peak_alloc) peak_alloc = (long long) bytes;
        void *p = malloc(bytes);
        if (p) memset(p, 0x5a, bytes);              // (scratch starts out as garbage)
        return p;
    }
    void release(void *p) { free(p); }
    bool zero(void *p, size_t bytes) { memset(p, 0, bytes); return true; }
    bool to_host(void *h, const void *d, size_t bytes) { memcpy(h, d, bytes); return true; }
    bool to_device(void *d, const void *h, size_t bytes) { memcpy(d, h, bytes); return true; }
    bool sync() { return true; }
    // `blocks` workgroups of pass `kernel`: block(kernel, a, index, &lds) with an LDS of type Lds
    template <class Lds, class Args, class Block> bool run_blocks(Block block, int kernel, long long blocks, const Args &a) {
        std::vector<long long> idx((size_t) blocks);
        std::iota(idx.begin(), idx.end(), 0ll);
        if (order == 1) std::reverse(idx.begin(), idx.end());
        if (order == 2) std::shuffle(idx.begin(), idx.end(), rng);
        static Lds lds;
        for (long long b : idx) {
            memset(&lds, 0xa5, sizeof lds);         // nothing may survive in LDS from one workgroup to the next
            block(kernel, a, b, &lds);
        }
        launches++;
        return true;
    }
    bool run(int kernel, long long blocks, const WcvArgs &a) { return run_blocks<WcvLds>(wcv_run_block, kernel, blocks, a); }
};

#endif  // WT_RUNS_LAUNCHER_H_
