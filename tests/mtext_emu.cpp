// mtext_emu.cpp -- the tile-text passes of csrc/wt_mtext.h on the CPU (test infrastructure of tests/test_mtext_emu.py).  The
// header is compiled with -DWT_EMU: a pass is a function of (arguments, workgroup index), and the launcher of
// tests/emu/runs_launcher.h runs the workgroups of every pass one after the other, forwards, backwards or shuffled.  The door
// is the product's own template over this launcher; mtext_host is the product's host sweep.
#define WT_EMU 1
#include "emu/runs_launcher.h"
#include "../wiggletools_amd/csrc/wt_mtext.h"

namespace {

struct MtextLauncher : CpuLauncher {
    using CpuLauncher::CpuLauncher;
    bool run_mtext(int kernel, long long blocks, const WtmArgs &a) { return run_blocks<WtmLds>(wtm_run_block, kernel, blocks, a); }
};

}  // namespace

extern "C" {

int mtext_emu_door(int order, uint64_t seed, int64_t n_seg, const int64_t *seg_off, const char *const *seg_name, const int32_t *start,
                   const int32_t *finish, const double *values, int32_t width, const char *prefix, const int64_t *prefix_off, uint32_t flags,
                   WtxState *state, char *text, int64_t capacity, int64_t *n_bytes, int64_t *n_wide, int64_t *launches) {
    MtextLauncher l(order, seed);
    const char *why = "";
    const int rc = wtm_door(l, (long long) n_seg, seg_off, seg_name, start, finish, values, (int) width, prefix, prefix_off, (unsigned int) flags, state,
                            text, (long long) capacity, n_bytes, n_wide, &why);
    if (launches) *launches = l.launches;
    return rc;
}

int mtext_host(int64_t n_seg, const int64_t *seg_off, const char *const *seg_name, const int32_t *start, const int32_t *finish, const double *values,
               int32_t width, const char *prefix, const int64_t *prefix_off, uint32_t flags, WtxState *state, char *text, int64_t capacity,
               int64_t *n_bytes, int64_t *n_wide) {
    return wtm_host((long long) n_seg, seg_off, seg_name, start, finish, values, (int) width, prefix, prefix_off, (unsigned int) flags, state, text,
                    (long long) capacity, n_bytes, n_wide);
}

}  // extern "C"
