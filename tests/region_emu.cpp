// region_emu.cpp -- the region passes of csrc/wt_region.h on the CPU (test infrastructure of tests/test_region_model.py).
// The header is compiled with -DWT_EMU: a pass is a function of (arguments, workgroup index), and the launcher of
// tests/emu/runs_launcher.h runs the workgroups of every pass one after the other, forwards, backwards or shuffled.  The
// door (validation, union of the mask, capacity) is the product's own template over this launcher.
#define WT_EMU 1
#include "emu/runs_launcher.h"
#include "../wiggletools_amd/csrc/wt_region.h"

namespace {

struct RegionLauncher : CpuLauncher {
    using CpuLauncher::CpuLauncher;
    bool run_region(int kernel, long long blocks, const WrgArgs &a) { return run_blocks<WrgLds>(wrg_run_block, kernel, blocks, a); }
};

}  // namespace

extern "C" {

int region_emu(int order, uint64_t seed, int op, int64_t n_seg, const int64_t *seg_off, const int32_t *start, const int32_t *finish,
               const void *value, int value_is_f64, const int64_t *m_seg_off, const int32_t *m_start, const int32_t *m_finish,
               int64_t capacity, int32_t *o_start, int32_t *o_finish, double *o_value, int64_t *o_seg_off, int64_t *n_out) {
    RegionLauncher l(order, seed);
    const char *why = "";
    return wrg_region(l, op, (long long) n_seg, seg_off, start, finish, value, value_is_f64, m_seg_off, m_start, m_finish,
                      (long long) capacity, o_start, o_finish, o_value, o_seg_off, n_out, &why);
}

}  // extern "C"
