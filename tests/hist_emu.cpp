// hist_emu.cpp -- the histogram passes of csrc/wt_hist.h on the CPU (test infrastructure of tests/test_hist_emu.py).  The header
// is compiled with -DWT_EMU: a pass is a function of (arguments, workgroup index), and the launcher of
// tests/emu/runs_launcher.h runs the workgroups of every pass one after the other, forwards, backwards or shuffled.  The door
// is the product's own template over this launcher; hist_host is the product's host sweep.
#define WT_EMU 1
#include "emu/runs_launcher.h"
#include "../wiggletools_amd/csrc/wt_hist.h"

namespace {

struct HistLauncher : CpuLauncher {
    using CpuLauncher::CpuLauncher;
    bool run_hist(int kernel, long long blocks, const WhsArgs &a) { return run_blocks<WhsLds>(whs_run_block, kernel, blocks, a); }
};

}  // namespace

extern "C" {

int hist_emu_door(int order, uint64_t seed, int64_t n_seg, const int64_t *seg_off, const int32_t *seg_row, int32_t n_rows, const int32_t *start,
                  const int32_t *finish, const void *value, int value_is_f64, int32_t width, uint32_t flags, double *range2, double *hist,
                  int64_t *launches) {
    HistLauncher l(order, seed);
    const char *why = "";
    const int rc = whs_door(l, (long long) n_seg, seg_off, seg_row, (int) n_rows, start, finish, value, value_is_f64, (int) width, (unsigned int) flags,
                            range2, hist, &why);
    if (launches) *launches = l.launches;
    return rc;
}

int hist_host(int64_t n_seg, const int64_t *seg_off, const int32_t *seg_row, int32_t n_rows, const int32_t *start, const int32_t *finish,
              const double *value, int32_t width, uint32_t flags, double *range2, double *hist) {
    return whs_host((long long) n_seg, seg_off, seg_row, (int) n_rows, start, finish, value, (int) width, (unsigned int) flags, range2, hist);
}

}  // extern "C"
